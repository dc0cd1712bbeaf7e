// The tile product of the periodic nx x nx grid: the one kernel behind the Hartley transforms of Allen-Cahn (IMEX step and the
// preconditioner of its Newton-PCG steps), Gray-Scott and Cahn-Hilliard. Included by mgrit_hip.hip after mgrit_hip_heat2d.inc, whose K loop
// (h2d_kloop), h2d_acc_to_lds, h2d_stagger and sweep arithmetic (h2d_apply_op) it shares, and before the three application files,
// which hold the pointwise maps (ACPre, GSPre, CHPre) the first product applies while it stages its operand.

// ===============================================================================================================
// (I - c L)^-1 b = T ((T b T) o D) T on the periodic grid, D[i][j] = 1 / (shift + c (lam_i + lam_j)): T the discrete Hartley matrix
// T[i][k] = (cos(2 pi i k / n) + sin(2 pi i k / n)) / sqrt(n) -- symmetric, orthogonal, its own inverse, and a real eigenbasis of the
// periodic Laplacian with lam_k = (4 / dx^2) sin^2(pi k / n). Four products of the form
//   out[n][m] = sum_k T[k][m] * B[k][n]   (output stored transposed, as Heat2D)
// with the FULL table (no even / odd fold: DESIGN.md 3.9 states what that costs), K ascending, no split-K. A state row holds
// NC = PRE::operands planes of the whole grid in natural order: there is no rim, the "interior" is everything. State b owns the work
// slab items NI b .. NI b + NI - 1, NI = PRE::items; items are P x P, P = nx padded to 64; the table's rows and columns >= nx are zero,
// so every pad of every intermediate is zero. Allen-Cahn (1 plane, 1 item) and Gray-Scott (2, 2) have one item per plane; Cahn-Hilliard
// has one plane and two items (u and w(u), staged from the same plane) that p2d_combine_kernel below joins into one. Per item z,
// plane c = z % NC (NI == NC):
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

// grid (n tiles, m tiles, NI * states), P / 64 tiles per axis; KP = nx rounded up to the K step (rows beyond hold zeros on both sides)
// P2D_FIRST: the operand of item z is plane z % NC of the state row B[in_idx[z / NC] * in_ld + .] (nx x nx, leading dimension nx), a
// two-operand PRE reads the row's other plane beside it; otherwise the operand is work slab item z. dinv = [NC][P][P].
// NI == 2 with NC == 1 (P2D_FIRST only): both items of a state are staged from its one plane, pre.item says which map applies.
// NC and NI are compile-time constants: with one plane the plane terms fold away.
template <int MODE, class PRE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) p2d_gemm_kernel(
    const double *__restrict__ T, int P, int KP, int nx, const double *__restrict__ B, double *__restrict__ out,
    const double *__restrict__ dinv, size_t bstride, const int32_t *__restrict__ in_idx, int in_ld, PRE pre, H2DDev H, H2DFin F) {
    constexpr int NC = PRE::operands, NI = PRE::items;
    static_assert(NC == 1 || NC == 2, "one plane, or two that are each other's second operand");
    static_assert(NI == NC || (NC == 1 && NI == 2 && MODE == P2D_FIRST), "an item per plane, or two items staged from one plane");
    __shared__ __attribute__((aligned(16))) double smem[2 * H2D_BK * H2D_LDT];
    double(*Cs)[66] = reinterpret_cast<double(*)[66]>(smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned z = blockIdx.z, st = z / NI, comp = z % NI;   // item, its state, its plane (NI > NC: its place among the state's items)
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
        } else {
            if constexpr (NI == 2) pre.item = comp;
            h2d_kloop<false, true, PRE>(acc, smem, T, P, m0, row, nx, n0, KP, nx, 0, 0.0, tid, lane, w, nx, pre);
        }
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

// The second product of a state whose two items are joined mode by mode (Cahn-Hilliard, mgrit_hip_cahnhilliard.inc):
//   out[st][i'][j'] = (sum_j T[j][j'] B[2 st][j][i']) o D1 + (sum_j T[j][j'] B[2 st + 1][j][i']) o D2,   dinv = [2][P][P] = D1, D2
// grid (n tiles, m tiles, states): one workgroup runs the K loop of both items, each as in P2D_SCALE (K ascending, no split-K), and
// writes ONE P x P item -- the two products that follow run over `states` items, not 2 * states. Each table product is rounded, then
// the sum: no fma (the numpy step's U * D1 + W * D2). Pads: rows and columns >= nx of both accumulators are zero, and so is the table.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) p2d_combine_kernel(
    const double *__restrict__ T, int P, int KP, const double *__restrict__ B, double *__restrict__ out, const double *__restrict__ dinv,
    size_t bstride) {
    __shared__ __attribute__((aligned(16))) double smem[2 * H2D_BK * H2D_LDT];
    double(*Cs)[66] = reinterpret_cast<double(*)[66]>(smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned st = blockIdx.z;
    h2d_stagger();
    const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
    d4_t au[2][2], aw[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { au[a][b] = (d4_t){0.0, 0.0, 0.0, 0.0}; aw[a][b] = (d4_t){0.0, 0.0, 0.0, 0.0}; }
    const double *Bu = B + (size_t)(2 * st) * bstride;
    h2d_kloop<false>(au, smem, T, P, m0, Bu, P, n0, KP, 0, 0, 0.0, tid, lane, w);
    h2d_kloop<false>(aw, smem, T, P, m0, Bu + bstride, P, n0, KP, 0, 0, 0.0, tid, lane, w);
    double *Ob = out + (size_t)st * bstride;
    double v[4][4];
    h2d_acc_to_lds(au, Cs, lane, w);
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int n = (tid >> 4) + 16 * p, c = (tid & 15) * 4;
        const size_t o = (size_t)(n0 + n) * P + m0 + c;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[p][q] = Cs[n][c + q] * dinv[o + q];
    }
    __syncthreads();
    h2d_acc_to_lds(aw, Cs, lane, w);
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int n = (tid >> 4) + 16 * p, c = (tid & 15) * 4;
        const size_t o = (size_t)(n0 + n) * P + m0 + c;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[p][q] = v[p][q] + Cs[n][c + q] * dinv[bstride + o + q];
        *reinterpret_cast<double2 *>(Ob + o) = make_double2(v[p][0], v[p][1]);
        *reinterpret_cast<double2 *>(Ob + o + 2) = make_double2(v[p][2], v[p][3]);
    }
}
