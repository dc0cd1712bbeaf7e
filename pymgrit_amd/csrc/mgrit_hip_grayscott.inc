// Gray-Scott 2-D device code: the IMEX step of a two-species state on the matrix cores. Included by mgrit_hip.hip after
// mgrit_hip_allencahn.inc; it shares the tile product (h2d_kloop, with the two-operand form of its staging map), h2d_acc_to_lds, the
// sweep arithmetic (h2d_apply_op), the Hartley table and the norm kernels with Heat2D and Allen-Cahn.

// ===============================================================================================================
// GrayScott, method 'IMEX' (gray_scott/gray_scott.py; DESIGN.md 3.11): on the periodic nx x nx grid, per species c = u, v
//   b_u = u + dt (a (1 - u) - u v^2),   b_v = v + dt (u v^2 - b v)                (pointwise, couples the two planes)
//   x_c = (I - dt d_c L)^-1 b_c = T ((T b_c T) o D_c) T,                          D_c[i][j] = 1 / (1 + (dt d_c) (lam_i + lam_j)),
// T and lam as for Allen-Cahn. A state row is [u plane | v plane], each nx * nx values in natural row-major order. One Phi of a batch
// is ONE set of four launches for both species: state b of the plan owns the work slab items 2 b (u) and 2 b + 1 (v), blockIdx.z runs
// over 2 * count, the species is z & 1. The four products are those of ac_gemm_kernel per item:
//   1. W1[z][j][i'] = sum_i  T[i][i']  b_c[i][j]     b_c formed from BOTH planes of the state row while the B tile is staged (GSPre)
//   2. W0[z][i'][j'] = sum_j  T[j][j']  W1[z][j][i']  o D_c, the species' table dinv[c]
//   3. W1[z][j'][i] = sum_i' T[i'][i]  W0[z][i'][j']
//   4. x_c[i][j]    = sum_j' T[j'][j]  W1[z][j'][i]  through the sweep's arithmetic at offset c nx^2 + i nx + j of the destination row
// ===============================================================================================================

// own = the staged value of the workgroup's species, other = the other species at the same point. The operand order is the one
// GrayScott._rhs_imex states in numpy:  uv2 = u * (v * v);  b_u = fma(dt, a * (1 - u) - uv2, u);  b_v = fma(dt, uv2 - b * v, v)
struct GSPre {
    static constexpr int operands = 2;
    double dt, a, b; int comp;
    __device__ __forceinline__ double operator()(double own, double other) const {
        const double u = comp ? other : own, v = comp ? own : other;
        const double uv2 = u * (v * v);
        return comp ? fma(dt, uv2 - b * v, v) : fma(dt, a * (1.0 - u) - uv2, u);
    }
};

enum { GS_FIRST = 0, GS_SCALE = 1, GS_PLAIN = 2, GS_FIN = 3 };

// grid (n tiles, m tiles, 2 * states), P / 64 tiles per axis; KP = nx rounded up to the K step
// GS_FIRST: the operand of item z is plane z & 1 of the state row B[in_idx[z >> 1] * in_ld + .], otherwise work slab item z
// GS_SCALE: dinv = [2][P][P], the table of species z & 1
template <int MODE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) gs_gemm_kernel(
    const double *__restrict__ T, int P, int KP, int nx, const double *__restrict__ B, double *__restrict__ out,
    const double *__restrict__ dinv, size_t bstride, const int32_t *__restrict__ in_idx, int in_ld, GSPre pre, H2DDev H, H2DFin F) {
    __shared__ __attribute__((aligned(16))) double smem[2 * H2D_BK * H2D_LDT];
    double(*Cs)[66] = reinterpret_cast<double(*)[66]>(smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int z = blockIdx.z, comp = z & 1;
    const size_t plane = (size_t)nx * nx;
    h2d_stagger();
    const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
    d4_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (d4_t){0.0, 0.0, 0.0, 0.0};
    if (MODE == GS_FIRST) {
        const double *row = B + (size_t)in_idx[z >> 1] * in_ld;
        pre.comp = comp;
        h2d_kloop<false, true, GSPre>(acc, smem, T, P, m0, row + (comp ? plane : 0), nx, n0, KP, nx, 0, 0.0, tid, lane, w, nx, pre,
                                      row + (comp ? 0 : plane));
    } else
        h2d_kloop<false>(acc, smem, T, P, m0, B + (size_t)z * bstride, P, n0, KP, 0, 0, 0.0, tid, lane, w);
    h2d_acc_to_lds(acc, Cs, lane, w);
    __syncthreads();
    double *Ob = out + (size_t)z * bstride;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int n = (tid >> 4) + 16 * p, c = (tid & 15) * 4;
        double v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = Cs[n][c + q];
        if (MODE == GS_FIN) {
            if (n0 + n < nx) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (m0 + c + q < nx) h2d_apply_op(H, F, z >> 1, (comp ? plane : 0) + (size_t)(n0 + n) * nx + (m0 + c + q), v[q]);
            }
        } else {
            const size_t o = (size_t)(n0 + n) * P + m0 + c;
            if (MODE == GS_SCALE) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = v[q] * dinv[(size_t)comp * bstride + o + q];
            }
            *reinterpret_cast<double2 *>(Ob + o) = make_double2(v[0], v[1]);
            *reinterpret_cast<double2 *>(Ob + o + 2) = make_double2(v[2], v[3]);
        }
    }
}
