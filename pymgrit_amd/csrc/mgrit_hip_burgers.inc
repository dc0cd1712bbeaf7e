// Burgers 2-D device code: the stencil pass that forms the right-hand sides of the IMEX step of a two-plane state. Included by
// mgrit_hip.hip after mgrit_hip_grayscott.inc: the four Hartley products that follow are the two-plane instances of p2d_gemm_kernel
// (mgrit_hip_periodic2d.inc) Gray-Scott compiles, in their work-slab modes -- no map is applied while an operand is staged.

// ===============================================================================================================
// Burgers2D, method 'IMEX' (burgers/burgers.py; DESIGN.md 3.13): on the periodic nx x nx grid, axis 0 = x, per plane c = u, v
//   ax_c[i][j] = (c[i+1][j] - c[i-1][j]) * inv_2dx,   ay_c[i][j] = (c[i][j+1] - c[i][j-1]) * inv_2dx        (indices mod nx)
//   b_c = c - dt (u ax_c + v ay_c)
//   x_c = (I - dt nu L)^-1 b_c = T ((T b_c T) o D) T,        D[i][j] = 1 / (1 + (dt nu) (lam_i + lam_j)), the same table for both planes.
// A state row is [u plane | v plane] as for Gray-Scott. b_c reads the four neighbours of a point in its own plane, so it cannot be
// formed point by point while the first product stages its operand (ACPre, GSPre, CHPre): it is a launch of its own, row -> W0, and
// one Phi of a batch is five launches (bg_products in mgrit_hip.hip). State b of the plan owns the work slab items 2 b (b_u) and
// 2 b + 1 (b_v), as in the products.
// ===============================================================================================================
constexpr int BG_TI = 32, BG_TJ = 64;   // the tile of one workgroup: BG_TI rows (i) of BG_TJ columns (j, contiguous, across the lanes)
constexpr int BG_LD = BG_TJ + 2;        // a staged row: the tile's columns between the two halo columns

// The grid index behind position g of a staged tile (g = -1 .. nx + tile - 1): the periodic wrap happens at two places only, the halo
// in front of point 0 and the point behind nx - 1. A result > nx - 1 is a pad: nothing is loaded for it.
__device__ __forceinline__ int bg_wrap(int g, int nx) { return g < 0 ? nx - 1 : (g == nx ? 0 : g); }

// b_c at one point from the point's u and v and the plane's four neighbours. The operand order is the one Burgers2D._rhs_imex states
// in numpy:  ax = (c[i+1][j] - c[i-1][j]) * inv_2dx;  ay = (c[i][j+1] - c[i][j-1]) * inv_2dx;  adv = fma(v, ay, u * ax);  b = fma(-dt, adv, c)
__device__ __forceinline__ double bg_rhs(double u, double v, double c, double c_ip, double c_im, double c_jp, double c_jm, double dt,
                                         double inv_2dx) {
    const double ax = (c_ip - c_im) * inv_2dx, ay = (c_jp - c_jm) * inv_2dx;
    return fma(-dt, fma(v, ay, u * ax), c);
}

// grid (P / BG_TJ, P / BG_TI, states). One workgroup stages the (BG_TI + 2) x (BG_TJ + 2) tile of u and of v with its halo ONCE from the
// state row in_slab[in_idx[b]] (8-byte loads: the v plane starts at element nx * nx and a grid row at a multiple of nx, neither
// 16-byte aligned for odd nx) and forms both planes' right-hand sides from it: every value of the state is read from HBM once per
// tile instead of five times per plane. It writes the WHOLE tile of both items, zeros outside nx x nx: the products that follow
// multiply the pads by zero table entries, and a pad that is not zero or not finite would poison them.
__global__ void __launch_bounds__(256) bg_rhs_kernel(int nx, int P, const double *__restrict__ in_slab, const int32_t *__restrict__ in_idx,
                                                     int in_ld, double dt, double inv_2dx, double *__restrict__ W, size_t per) {
    __shared__ double su[BG_TI + 2][BG_LD], sv[BG_TI + 2][BG_LD];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int j0 = blockIdx.x * BG_TJ, i0 = blockIdx.y * BG_TI;
    const bool live = i0 < nx && j0 < nx;   // (of the whole workgroup: a tile outside the grid is zeros)
    if (live) {
        const size_t plane = (size_t)nx * nx;
        const double *row = in_slab + (size_t)in_idx[b] * in_ld;
        for (int q = tid; q < (BG_TI + 2) * BG_LD; q += 256) {
            const int r = q / BG_LD, c = q - r * BG_LD;
            const int gi = bg_wrap(i0 - 1 + r, nx), gj = bg_wrap(j0 - 1 + c, nx);
            double u = 0.0, v = 0.0;
            if (gi < nx && gj < nx) {
                const size_t o = (size_t)gi * nx + gj;
                u = row[o];
                v = row[plane + o];
            }
            su[r][c] = u;
            sv[r][c] = v;
        }
        __syncthreads();
    }
    const int c = tid & 63, j = j0 + c;
    double *Wu = W + (size_t)(2 * b) * per, *Wv = Wu + per;
    for (int r = tid >> 6; r < BG_TI; r += 4) {
        const int i = i0 + r;
        double bu = 0.0, bv = 0.0;
        if (live && i < nx && j < nx) {
            const double u = su[r + 1][c + 1], v = sv[r + 1][c + 1];
            bu = bg_rhs(u, v, u, su[r + 2][c + 1], su[r][c + 1], su[r + 1][c + 2], su[r + 1][c], dt, inv_2dx);
            bv = bg_rhs(u, v, v, sv[r + 2][c + 1], sv[r][c + 1], sv[r + 1][c + 2], sv[r + 1][c], dt, inv_2dx);
        }
        const size_t o = (size_t)i * P + j;
        Wu[o] = bu;
        Wv[o] = bv;
    }
}
