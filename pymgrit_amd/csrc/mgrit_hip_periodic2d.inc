// The tile product of the periodic nx x nx grid: the one kernel behind the Hartley transforms of Allen-Cahn (IMEX step and the
// preconditioner of its Newton-PCG steps) and Gray-Scott. Included by mgrit_hip.hip after mgrit_hip_heat2d.inc, whose K loop
// (h2d_kloop), h2d_acc_to_lds, h2d_stagger and sweep arithmetic (h2d_apply_op) it shares, and before the two application files,
// which hold the pointwise maps (ACPre, GSPre) the first product applies while it stages its operand.

// ===============================================================================================================
// (I - c L)^-1 b = T ((T b T) o D) T on the periodic grid, D[i][j] = 1 / (shift + c (lam_i + lam_j)): T the discrete Hartley matrix
// T[i][k] = (cos(2 pi i k / n) + sin(2 pi i k / n)) / sqrt(n) -- symmetric, orthogonal, its own inverse, and a real eigenbasis of the
// periodic Laplacian with lam_k = (4 / dx^2) sin^2(pi k / n). Four products of the form
//   out[n][m] = sum_k T[k][m] * B[k][n]   (output stored transposed, as Heat2D)
// with the FULL table (no even / odd fold: DESIGN.md 3.9 states what that costs), K ascending, no split-K. A state row holds
// NC = PRE::operands planes of the whole grid in natural order: there is no rim, the "interior" is everything. State b owns the work
// slab items NC b .. NC b + NC - 1, one per plane; items are P x P, P = nx padded to 64; the table's rows and columns >= nx are zero,
// so every pad of every intermediate is zero. Per item z, plane c = z % NC:
//   1. W1[z][j][i']  = sum_i  T[i][i']  b_c[i][j]      b_c formed from the state row while the B tile is staged (PRE)      P2D_FIRST
//   2. W0[z][i'][j'] = sum_j  T[j][j']  W1[z][j][i']   o D_c, the plane's table dinv[c]                                    P2D_SCALE
//   3. W1[z][j'][i]  = sum_i' T[i'][i]  W0[z][i'][j']                                                                      P2D_PLAIN
//   4. x_c[i][j]     = sum_j' T[j'][j]  W1[z][j'][i]   through the sweep's arithmetic at offset c nx^2 + i nx + j of the
//                                                      destination row (P2D_FIN), or into the work slab (P2D_PLAIN: norms)
// P2D_WORK_PLAIN / P2D_WORK_SCALE: the products of the Newton steps' preconditioners (Allen-Cahn PCG, Gray-Scott BiCGStab) -- as
// P2D_PLAIN / P2D_SCALE, but in_idx[state] is the "inner iteration running" flag of the item's state z / NC and a workgroup of an
// item whose state's flag is 0 returns at once.
// ===============================================================================================================
enum { P2D_FIRST = 0, P2D_SCALE = 1, P2D_PLAIN = 2, P2D_FIN = 3, P2D_WORK_PLAIN = 4, P2D_WORK_SCALE = 5 };

// grid (n tiles, m tiles, NC * states), P / 64 tiles per axis; KP = nx rounded up to the K step (rows beyond hold zeros on both sides)
// P2D_FIRST: the operand of item z is plane z % NC of the state row B[in_idx[z / NC] * in_ld + .] (nx x nx, leading dimension nx), a
// two-operand PRE reads the row's other plane beside it; otherwise the operand is work slab item z. dinv = [NC][P][P].
// NC is a compile-time constant: with one plane the plane terms fold away.
template <int MODE, class PRE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) p2d_gemm_kernel(
    const double *__restrict__ T, int P, int KP, int nx, const double *__restrict__ B, double *__restrict__ out,
    const double *__restrict__ dinv, size_t bstride, const int32_t *__restrict__ in_idx, int in_ld, PRE pre, H2DDev H, H2DFin F) {
    constexpr int NC = PRE::operands;
    static_assert(NC == 1 || NC == 2, "one plane, or two that are each other's second operand");
    __shared__ __attribute__((aligned(16))) double smem[2 * H2D_BK * H2D_LDT];
    double(*Cs)[66] = reinterpret_cast<double(*)[66]>(smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned z = blockIdx.z, st = z / NC, comp = z % NC;   // item, its state, its plane
    const size_t plane = (size_t)nx * nx;
    if (MODE >= P2D_WORK_PLAIN && !in_idx[st]) return;
    h2d_stagger();
    const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
    d4_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (d4_t){0.0, 0.0, 0.0, 0.0};
    if (MODE == P2D_FIRST) {
        const double *row = B + (size_t)in_idx[st] * in_ld;
        if constexpr (NC == 2) {
            pre.comp = comp;
            h2d_kloop<false, true, PRE>(acc, smem, T, P, m0, row + (comp ? plane : 0), nx, n0, KP, nx, 0, 0.0, tid, lane, w, nx, pre,
                                        row + (comp ? 0 : plane));
        } else
            h2d_kloop<false, true, PRE>(acc, smem, T, P, m0, row, nx, n0, KP, nx, 0, 0.0, tid, lane, w, nx, pre);
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
        if (MODE == P2D_FIN) {
            if (n0 + n < nx) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (m0 + c + q < nx) h2d_apply_op(H, F, st, (size_t)comp * plane + (size_t)(n0 + n) * nx + (m0 + c + q), v[q]);
            }
        } else {
            const size_t o = (size_t)(n0 + n) * P + m0 + c;
            if (MODE == P2D_SCALE || MODE == P2D_WORK_SCALE) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = v[q] * dinv[(size_t)comp * bstride + o + q];
            }
            *reinterpret_cast<double2 *>(Ob + o) = make_double2(v[0], v[1]);
            *reinterpret_cast<double2 *>(Ob + o + 2) = make_double2(v[2], v[3]);
        }
    }
}
