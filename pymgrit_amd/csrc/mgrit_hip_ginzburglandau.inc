// Ginzburg-Landau 2-D device code: the pointwise map of the IMEX step of a complex-valued state and the product that joins the two
// spectra of a state into two items. Included by mgrit_hip.hip after mgrit_hip_periodic2d.inc, whose tile product (p2d_gemm_kernel, here
// with two planes per state and the two-operand form of h2d_kloop's staging map) carries the first, third and fourth Hartley product;
// the Hartley table, the norm kernels and the plane-by-plane periodic transfer are shared with Gray-Scott.

// ===============================================================================================================
// GinzburgLandau2D, method 'IMEX' (ginzburg_landau/ginzburg_landau.py; DESIGN.md 3.15): A_t = A + (1 + i b) Lap A - (1 + i c) |A|^2 A on
// the periodic nx x nx grid, A = x + i y, Lap the periodic 5-point Laplacian / dx^2. Growth and cubic term explicit, diffusion and
// dispersion implicit; in real form, with q = x^2 + y^2,
//   r = x + dt (x - q (x - c y)),   s = y + dt (y - q (c x + y))                         (pointwise, couples the two planes)
//   [ I - dt L     b dt L ] [x_new]   [r]
//   [ -b dt L    I - dt L ] [y_new] = [s]
// The block matrix is diagonalised plane by plane by T (as for Allen-Cahn), which leaves a 2 x 2 block per mode: with mu = lam_i + lam_j,
// a = 1 + dt mu, beta = (b dt) mu, det = a^2 + beta^2, Da = a / det, Db = beta / det,
//   X = T r T,  Y = T s T,     x_new = T (X o Da + Y o Db) T,     y_new = T (Y o Da - X o Db) T.
// A state row is [x plane | y plane], each nx * nx values in natural row-major order; state st of a plan owns the work slab items 2 st (x)
// and 2 st + 1 (y). Four launches per Phi: P2D_FIRST over 2 * count items (GLPre), p2d_cross_kernel over count states, P2D_PLAIN and
// P2D_FIN over 2 * count items. Da^2 + Db^2 = 1 / det <= 1: the modal solve contracts in the 2-norm; mode (0, 0) has Da = 1, Db = 0.
// ===============================================================================================================

// own = the staged value of the workgroup's plane, other = the other plane at the same point. The operand order is the one
// GinzburgLandau2D._rhs_imex states in numpy, no fma:
//   q = x * x + y * y;   r = x + dt * (x - q * (x - c * y));   s = y + dt * (y - q * (c * x + y))
struct GLPre {
    static constexpr int operands = 2, items = 2;
    double dt, c; int comp;
    __device__ __forceinline__ double operator()(double own, double other) const {
        const double x = comp ? other : own, y = comp ? own : other;
        const double q = x * x + y * y;
        return comp ? y + dt * (y - q * (c * x + y)) : x + dt * (x - q * (x - c * y));
    }
};

// The second product of a state whose two spectra are joined mode by mode into TWO items:
//   X = sum_j T[j][j'] B[2 st][j][i'],   Y = sum_j T[j][j'] B[2 st + 1][j][i'],      dinv = [2][P][P] = Da, Db
//   out[2 st] = X o Da + Y o Db,         out[2 st + 1] = Y o Da - X o Db
// grid (n tiles, m tiles, states): one workgroup runs the K loop of both items of its state, each as in P2D_SCALE (K ascending, no
// split-K, h2d_kloop). Each table product is rounded, then the sum or the difference: no fma (the numpy step's X * Da + Y * Db and
// Y * Da - X * Db; -ffp-contract=off). Pads: rows and columns >= nx of both accumulators are zero, so both outputs are zero there
// whatever the table holds (it holds zeros). The accumulators go through the one LDS tile in turn: X's 16 values per thread wait in
// registers (32 VGPRs, in place of the accumulator they came from) while Y passes through, and each group of four outputs of both items
// is stored as soon as it is formed -- the register peak is the K loops' two accumulators, as in p2d_combine_kernel.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) p2d_cross_kernel(
    const double *__restrict__ T, int P, int KP, const double *__restrict__ B, double *__restrict__ out, const double *__restrict__ dinv,
    size_t bstride) {
    __shared__ __attribute__((aligned(16))) double smem[2 * H2D_BK * H2D_LDT];
    double(*Cs)[66] = reinterpret_cast<double(*)[66]>(smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned st = blockIdx.z;
    h2d_stagger();
    const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
    d4_t ax[2][2], ay[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { ax[a][b] = (d4_t){0.0, 0.0, 0.0, 0.0}; ay[a][b] = (d4_t){0.0, 0.0, 0.0, 0.0}; }
    const double *Bx = B + (size_t)(2 * st) * bstride;
    h2d_kloop<false>(ax, smem, T, P, m0, Bx, P, n0, KP, 0, 0, 0.0, tid, lane, w);
    h2d_kloop<false>(ay, smem, T, P, m0, Bx + bstride, P, n0, KP, 0, 0, 0.0, tid, lane, w);
    double *Ox = out + (size_t)(2 * st) * bstride, *Oy = Ox + bstride;
    double X[4][4];
    h2d_acc_to_lds(ax, Cs, lane, w);
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int n = (tid >> 4) + 16 * p, c = (tid & 15) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) X[p][q] = Cs[n][c + q];
    }
    __syncthreads();
    h2d_acc_to_lds(ay, Cs, lane, w);
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int n = (tid >> 4) + 16 * p, c = (tid & 15) * 4;
        const size_t o = (size_t)(n0 + n) * P + m0 + c;
        double vx[4], vy[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double Y = Cs[n][c + q], da = dinv[o + q], db = dinv[bstride + o + q];
            vx[q] = X[p][q] * da + Y * db;
            vy[q] = Y * da - X[p][q] * db;
        }
        *reinterpret_cast<double2 *>(Ox + o) = make_double2(vx[0], vx[1]);
        *reinterpret_cast<double2 *>(Ox + o + 2) = make_double2(vx[2], vx[3]);
        *reinterpret_cast<double2 *>(Oy + o) = make_double2(vy[0], vy[1]);
        *reinterpret_cast<double2 *>(Oy + o + 2) = make_double2(vy[2], vy[3]);
    }
}
