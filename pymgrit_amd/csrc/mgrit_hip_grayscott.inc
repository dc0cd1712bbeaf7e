// Gray-Scott 2-D device code: the pointwise map of the IMEX step of a two-species state. Included by mgrit_hip.hip after
// mgrit_hip_periodic2d.inc, whose tile product (p2d_gemm_kernel, here with two planes per state and the two-operand form of
// h2d_kloop's staging map) carries the four Hartley products; the Hartley table and the norm kernels are shared with Allen-Cahn.

// ===============================================================================================================
// GrayScott, method 'IMEX' (gray_scott/gray_scott.py; DESIGN.md 3.11): on the periodic nx x nx grid, per species c = u, v
//   b_u = u + dt (a (1 - u) - u v^2),   b_v = v + dt (u v^2 - b v)                (pointwise, couples the two planes)
//   x_c = (I - dt d_c L)^-1 b_c = T ((T b_c T) o D_c) T,                          D_c[i][j] = 1 / (1 + (dt d_c) (lam_i + lam_j)),
// T and lam as for Allen-Cahn. A state row is [u plane | v plane], each nx * nx values in natural row-major order. One Phi of a batch
// is ONE set of four launches for both species: state b of the plan owns the work slab items 2 b (u) and 2 b + 1 (v), blockIdx.z runs
// over 2 * count, the species is z & 1 (p2d_gemm_kernel with NC = 2); b_c is formed from BOTH planes of the state row while the
// first product stages its B tile (GSPre), the second scales with the species' table D_c.
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
