// Cahn-Hilliard 2-D device code: the pointwise map of the IMEX step. Included by mgrit_hip.hip after mgrit_hip_periodic2d.inc, whose
// tile product (p2d_gemm_kernel) and combine product (p2d_combine_kernel) carry the Hartley products; the Hartley table, the norm
// kernels and the periodic transfer are shared with Allen-Cahn.

// ===============================================================================================================
// CahnHilliard, method 'IMEX' (cahn_hilliard/cahn_hilliard.py; DESIGN.md 3.12): u_t = L (u^3 - u - eps^2 L u) on the periodic nx x nx
// grid, L the periodic 5-point Laplacian / dx^2, linearly stabilised (s = stab >= 0):
//   (I + dt (eps^2 L^2 - s L)) x = u + dt L w,      w = u^3 - (1 + s) u                (pointwise)
//   x = T ((T u T) o D1 + (T w T) o D2) T,          D1[i][j] = 1 / (1 + dt (eps^2 mu^2 + s mu)),  D2 = -(dt mu) D1,  mu = lam_i + lam_j
// T and lam as for Allen-Cahn. A state row is ONE plane; state b of a plan owns the work slab items 2 b (u) and 2 b + 1 (w) through the
// first product, which stages both from the row's one plane (CHPre), and the second; p2d_combine_kernel joins them mode by mode into
// the ONE item b the last two products transform back: six item-products per state. D2 vanishes at mode (0, 0) and D1 is 1 there:
// the mean of u is carried through unchanged up to the rounding of the products.
// ===============================================================================================================

// item 0 stages u itself, item 1 w = (u * u) * u - c1 * u with c1 = 1 + s formed once on the host: the operand order
// CahnHilliard._w states in numpy (no fma)
struct CHPre {
    static constexpr int operands = 1, items = 2;
    double c1; int item;
    __device__ __forceinline__ double operator()(double u) const { return item ? (u * u) * u - c1 * u : u; }
};
