// Navier-Stokes 2-D (vorticity form) device code: the identity map of the product that stages the vorticity for the stream-function
// solve, and the stencil pass between that solve and the diffusion solve. Included by mgrit_hip.hip after mgrit_hip_burgers.inc, whose
// tile (BG_TI x BG_TJ, BG_LD) and wrap rule (bg_wrap) the stencil pass shares. The eight Hartley products around it are one-plane
// instances of p2d_gemm_kernel (mgrit_hip_periodic2d.inc): the first one is new (NSPre), the other seven are the work-slab modes
// Allen-Cahn compiles -- no map is applied while an operand is staged.

// ===============================================================================================================
// NavierStokes2D, method 'IMEX' (navier_stokes/navier_stokes.py; DESIGN.md 3.14): on the periodic nx x nx grid, axis 0 = x, a state is
// the vorticity w, mu = lam_i + lam_j
//   psi = T ((T w T) o S) T,                 S = 1 / mu, S[0][0] = 0          (Lh psi = -(w - mean w))
//   px = (psi[i+1][j] - psi[i-1][j]) * inv_2dx,   py = (psi[i][j+1] - psi[i][j-1]) * inv_2dx,   wx, wy the same of w    (indices mod nx)
//   jac = fma(py, wx, -(px * wy));   b = fma(-dt, jac, w);   with a forcing b = fma(dt, f, b)
//   x   = T ((T b T) o D) T,                 D = 1 / (1 + (dt nu) mu)
// One Phi of a batch is nine launches (ns_products in mgrit_hip.hip): four products row -> psi (a work item, leading dimension P, pads
// zero), the stencil pass below (psi item and state row -> b item), four products b -> the sweep's arithmetic. psi is dead after the
// stencil pass, so the two ping-pong buffers suffice: state b of the plan owns work slab item b of each.
// ===============================================================================================================

// The map of the first product: none. w is staged from the state row as it is (its mean ends in mode (0, 0), which S drops).
struct NSPre {
    static constexpr int operands = 1, items = 1;
    __device__ __forceinline__ double operator()(double w) const { return w; }
};

// b at one point from w there, the four neighbours of psi and the four of w. The operand order is the one NavierStokes2D._rhs_imex
// states in numpy.
__device__ __forceinline__ double ns_rhs(double w, double p_ip, double p_im, double p_jp, double p_jm, double w_ip, double w_im, double w_jp,
                                         double w_jm, double dt, double inv_2dx) {
    const double px = (p_ip - p_im) * inv_2dx, py = (p_jp - p_jm) * inv_2dx;
    const double wx = (w_ip - w_im) * inv_2dx, wy = (w_jp - w_jm) * inv_2dx;
    return fma(-dt, fma(py, wx, -(px * wy)), w);
}

// grid (P / BG_TJ, P / BG_TI, states), the tile of bg_rhs_kernel. One workgroup stages the (BG_TI + 2) x (BG_TJ + 2) tile of psi with its
// halo from work item b of Wpsi (leading dimension P -- but the periodic wrap is at nx, not at P: the neighbour of grid row nx - 1 is
// row 0, never the pad row nx) and the same tile of w from the state row in_slab[in_idx[b]] (leading dimension nx; 8-byte loads: a
// grid row starts at a multiple of nx, not 16-byte aligned for odd nx). With a forcing it reads the tile of f (nx x nx, natural order)
// point by point. It writes the WHOLE tile of item b of W, zeros outside nx x nx: the products that follow multiply the pads by zero
// table entries, and a pad that is not zero or not finite would poison them. Wpsi and W are the two ping-pong buffers, never the same.
__global__ void __launch_bounds__(256) ns_rhs_kernel(int nx, int P, const double *__restrict__ Wpsi, const double *__restrict__ in_slab,
                                                     const int32_t *__restrict__ in_idx, int in_ld, const double *__restrict__ f, double dt,
                                                     double inv_2dx, double *__restrict__ W, size_t per) {
    __shared__ double sp[BG_TI + 2][BG_LD], sw[BG_TI + 2][BG_LD];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int j0 = blockIdx.x * BG_TJ, i0 = blockIdx.y * BG_TI;
    const bool live = i0 < nx && j0 < nx;   // (of the whole workgroup: a tile outside the grid is zeros)
    if (live) {
        const double *row = in_slab + (size_t)in_idx[b] * in_ld, *psi = Wpsi + (size_t)b * per;
        for (int q = tid; q < (BG_TI + 2) * BG_LD; q += 256) {
            const int r = q / BG_LD, c = q - r * BG_LD;
            const int gi = bg_wrap(i0 - 1 + r, nx), gj = bg_wrap(j0 - 1 + c, nx);
            double p = 0.0, w = 0.0;
            if (gi < nx && gj < nx) {
                p = psi[(size_t)gi * P + gj];
                w = row[(size_t)gi * nx + gj];
            }
            sp[r][c] = p;
            sw[r][c] = w;
        }
        __syncthreads();
    }
    const int c = tid & 63, j = j0 + c;
    double *Wb = W + (size_t)b * per;
    for (int r = tid >> 6; r < BG_TI; r += 4) {
        const int i = i0 + r;
        double rhs = 0.0;
        if (live && i < nx && j < nx) {
            rhs = ns_rhs(sw[r + 1][c + 1], sp[r + 2][c + 1], sp[r][c + 1], sp[r + 1][c + 2], sp[r + 1][c], sw[r + 2][c + 1], sw[r][c + 1],
                         sw[r + 1][c + 2], sw[r + 1][c], dt, inv_2dx);
            if (f) rhs = fma(dt, f[(size_t)i * nx + j], rhs);
        }
        Wb[(size_t)i * P + j] = rhs;
    }
}
