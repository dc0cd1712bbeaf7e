// Allen-Cahn 2-D device code: the IMEX step on the matrix cores. Included by mgrit_hip.hip after mgrit_hip_heat2d.inc, whose tile
// product (h2d_kloop), sweep arithmetic (h2d_apply_op) and norm kernels it shares.

// ===============================================================================================================
// AllenCahn, method 'IMEX' (allen_cahn/allen_cahn.py): on the periodic nx x nx grid
//   b   = u + dt/eps^2 * u * (1 - u^nu)                       (pointwise, non-linear)
//   Phi = (I - dt L)^-1 b = T ((T b T) o D) T,                D[i][j] = 1 / (1 + dt (lam_i + lam_j)),
// T the discrete Hartley matrix T[i][k] = (cos(2 pi i k / n) + sin(2 pi i k / n)) / sqrt(n) -- symmetric, orthogonal, its own inverse,
// and a real eigenbasis of the periodic Laplacian with lam_k = (4 / dx^2) sin^2(pi k / n). Four products of the form
//   out[n][m] = sum_k T[k][m] * B[k][n]   (output stored transposed, as Heat2D)
// with the FULL table (no even / odd fold: DESIGN.md 3.9 states what that costs), K ascending, no split-K. State rows hold the whole
// grid in natural order: there is no rim, the "interior" is everything. Work slab items are P x P, P = nx padded to 64; the table's
// rows and columns >= nx are zero, so every pad of every intermediate is zero.
//   1. W1[j][i'] = sum_i  T[i][i']  b[i][j]       b formed from the state row while the B tile is staged (ACPre)
//   2. W0[i'][j'] = sum_j  T[j][j']  W1[j][i']     o D
//   3. W1[j'][i] = sum_i' T[i'][i]  W0[i'][j']
//   4. Phi[i][j] = sum_j' T[j'][j]  W1[j'][i]     through the sweep's arithmetic into the destination rows (or into W0: norms)
// ===============================================================================================================

// b = fma(c, u * (1 - p), u), c = dt * (1 / eps^2) (formed once on the host), p = u^nu by nu - 1 multiplications p = p * u
struct ACPre {
    double c; int nu;
    __device__ __forceinline__ double operator()(double u) const {
        double p = u;
        for (int q = 1; q < nu; ++q) p = p * u;
        return fma(c, u * (1.0 - p), u);
    }
};

enum { AC_FIRST = 0, AC_SCALE = 1, AC_PLAIN = 2, AC_FIN = 3 };

// grid (n tiles, m tiles, items), P / 64 tiles per axis; KP = nx rounded up to the K step (rows beyond hold zeros on both sides)
// AC_FIRST: item b's operand is the state row B[in_idx[b] * in_ld + .] (nx x nx, leading dimension nx), otherwise the work slab item
template <int MODE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) ac_gemm_kernel(
    const double *__restrict__ T, int P, int KP, int nx, const double *__restrict__ B, double *__restrict__ out,
    const double *__restrict__ dinv, size_t bstride, const int32_t *__restrict__ in_idx, int in_ld, ACPre pre, H2DDev H, H2DFin F) {
    __shared__ __attribute__((aligned(16))) double smem[2 * H2D_BK * H2D_LDT];
    double(*Cs)[66] = reinterpret_cast<double(*)[66]>(smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    h2d_stagger();
    const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
    d4_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (d4_t){0.0, 0.0, 0.0, 0.0};
    if (MODE == AC_FIRST)
        h2d_kloop<false, true, ACPre>(acc, smem, T, P, m0, B + (size_t)in_idx[blockIdx.z] * in_ld, nx, n0, KP, nx, 0, 0.0, tid, lane, w,
                                      nx, pre);
    else
        h2d_kloop<false>(acc, smem, T, P, m0, B + (size_t)blockIdx.z * bstride, P, n0, KP, 0, 0, 0.0, tid, lane, w);
    h2d_acc_to_lds(acc, Cs, lane, w);
    __syncthreads();
    double *Ob = out + (size_t)blockIdx.z * bstride;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int n = (tid >> 4) + 16 * p, c = (tid & 15) * 4;
        double v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = Cs[n][c + q];
        if (MODE == AC_FIN) {
            if (n0 + n < nx) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (m0 + c + q < nx) h2d_apply_op(H, F, blockIdx.z, (size_t)(n0 + n) * nx + (m0 + c + q), v[q]);
            }
        } else {
            const size_t o = (size_t)(n0 + n) * P + m0 + c;
            if (MODE == AC_SCALE) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = v[q] * dinv[o + q];
            }
            *reinterpret_cast<double2 *>(Ob + o) = make_double2(v[0], v[1]);
            *reinterpret_cast<double2 *>(Ob + o + 2) = make_double2(v[2], v[3]);
        }
    }
}
