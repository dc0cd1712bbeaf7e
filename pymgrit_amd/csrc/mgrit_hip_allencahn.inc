// Allen-Cahn 2-D device code: the pointwise map of the IMEX step and the kernels of the Newton-PCG steps. Included by mgrit_hip.hip
// after mgrit_hip_periodic2d.inc, whose tile product (p2d_gemm_kernel) carries the four Hartley products of both.

// ===============================================================================================================
// AllenCahn, method 'IMEX' (allen_cahn/allen_cahn.py): on the periodic nx x nx grid
//   b   = u + dt/eps^2 * u * (1 - u^nu)                       (pointwise, non-linear: ACPre, applied while the first product stages b)
//   Phi = (I - dt L)^-1 b = T ((T b T) o D) T,                D[i][j] = 1 / (1 + dt (lam_i + lam_j))
// ===============================================================================================================

// b = fma(c, u * (1 - p), u), c = dt * (1 / eps^2) (formed once on the host), p = u^nu by nu - 1 multiplications p = p * u
struct ACPre {
    static constexpr int operands = 1, items = 1;
    double c; int nu;
    __device__ __forceinline__ double operator()(double u) const {
        double p = u;
        for (int q = 1; q < nu; ++q) p = p * u;
        return fma(c, u * (1.0 - p), u);
    }
};

// ===============================================================================================================
// AllenCahn, methods 'IMPL' and 'CN' with linear_solver = 'pcg' (DESIGN.md 3.9): per item Newton's method on
//   x - fac (L x + r(x) / eps^2) = rhs,   fac = theta dt,  r(v) = v (1 - v^nu),  rhs = u (IMPL) or u + fac (L u + r(u) / eps^2) (CN),
// each correction J delta = g by conjugate gradients preconditioned with P = (1 + fac nu / eps^2) I - fac L through the four Hartley
// products above (no ACPre, the shifted D table). A batch's Phi is a host-driven loop over the kernels below (ACNBatch under newton_phi_batch in
// mgrit_hip.hip); blockIdx.z (or the thread of acn_reduce_kernel) is the item. Work rows are P x P slab items like the products'
// operands, pads zero and never written. Per-item state lives in ACNState: an item whose Newton test has passed is FROZEN (act = 0) --
// every kernel returns at once for it and its x is never written again --; cg = 1 while its inner iteration runs.
// Reductions: wave shuffle, LDS, one partial per workgroup in the item's partials row, the row summed in index order by the item's
// thread of acn_reduce_kernel. No floating-point atomics anywhere: the sums depend on the item's own values and on nothing else, so
// the result of an item is the same bits in any batch.
// ===============================================================================================================
constexpr int ACN_NB = 64;   // workgroups (and partials) per item of the elementwise kernels, at most

struct ACNState {
    int32_t *act, *cg, *n_newton, *n_cg, *k_cg;   // per item: Newton running; CG running; Newton / CG iterations of this Phi; CG iterations of this Newton step
    double *rz, *stop, *alpha, *beta;             // per item: r.z; lin_tol * norm2(g); the CG step lengths
    double *part;                                 // [item][ACN_NB][2] partial sums / maxima of the running reduction
};

struct ACNPar { int nx, P, nu; double inv_dx2, inv_eps2, fac; };

__device__ __forceinline__ size_t acn_at(const ACNPar &A, int q) { return (size_t)(q / A.nx) * A.P + (q % A.nx); }

// periodic 5-point Laplacian at grid point q of the P-strided item v: ((up + down) + (left + right) - 4 v) / dx^2
__device__ __forceinline__ double acn_lap(const ACNPar &A, const double *__restrict__ v, int q) {
    const int i = q / A.nx, j = q % A.nx;
    const int iu = i == 0 ? A.nx - 1 : i - 1, id = i == A.nx - 1 ? 0 : i + 1, jl = j == 0 ? A.nx - 1 : j - 1, jr = j == A.nx - 1 ? 0 : j + 1;
    const double s = (v[(size_t)iu * A.P + j] + v[(size_t)id * A.P + j]) + (v[(size_t)i * A.P + jl] + v[(size_t)i * A.P + jr]);
    return (s - 4.0 * v[(size_t)i * A.P + j]) * A.inv_dx2;
}

__device__ __forceinline__ double acn_pow(double u, int nu) {
    double p = u;
    for (int q = 1; q < nu; ++q) p = p * u;
    return p;
}

// the workgroup's sum of s and maximum of m into part[b][blockIdx.x]: shuffle tree per wave, then the waves in order
__device__ __forceinline__ void acn_block_reduce(double s, double m, double *__restrict__ part) {
    __shared__ double ls[4], lm[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s = s + __shfl_down(s, o, 64);
        m = fmax(m, __shfl_down(m, o, 64));
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { ls[w] = s; lm[w] = m; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *o = part + ((size_t)blockIdx.z * ACN_NB + blockIdx.x) * 2;
        o[0] = ((ls[0] + ls[1]) + ls[2]) + ls[3];
        o[1] = fmax(fmax(lm[0], lm[1]), fmax(lm[2], lm[3]));
    }
}

// x = the input row (natural nx x nx, leading dimension nx) on the padded item; IMPL: rhs = the same; the item's state reset
__global__ void __launch_bounds__(256) acn_init_kernel(ACNPar A, ACNState S, const double *__restrict__ in_slab, const int32_t *__restrict__ in_idx,
                                                       int in_ld, double *__restrict__ x, double *__restrict__ rhs, size_t per) {
    const int b = blockIdx.z, n = A.nx * A.nx;
    const double *u = in_slab + (size_t)in_idx[b] * in_ld;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
        const size_t o = (size_t)b * per + acn_at(A, q);
        const double v = u[q];
        x[o] = v;
        if (rhs) rhs[o] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { S.act[b] = 1; S.cg[b] = 0; S.n_newton[b] = 0; S.n_cg[b] = 0; S.k_cg[b] = 0; }
}

// RHS = false: g = (x - fac (L x + r(x) / eps^2)) - rhs into out (the CG residual row: delta starts at 0), partials sum g^2 and max |g|
// RHS = true (CN): out = x + fac (L x + r(x) / eps^2), the right-hand side from x = u
template <bool RHS>
__global__ void __launch_bounds__(256) acn_residual_kernel(ACNPar A, ACNState S, const double *__restrict__ x, const double *__restrict__ rhs,
                                                           double *__restrict__ out, size_t per) {
    const int b = blockIdx.z, n = A.nx * A.nx;
    if (!S.act[b]) return;
    const double *xb = x + (size_t)b * per;
    double s = 0.0, m = 0.0;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
        const size_t o = acn_at(A, q);
        const double v = xb[o];
        const double t = fma(A.inv_eps2, v * (1.0 - acn_pow(v, A.nu)), acn_lap(A, xb, q));
        if (RHS) {
            out[(size_t)b * per + o] = fma(A.fac, t, v);
        } else {
            const double g = fma(-A.fac, t, v) - rhs[(size_t)b * per + o];
            out[(size_t)b * per + o] = g;
            s = fma(g, g, s);
            m = fmax(m, fabs(g));
        }
    }
    if (!RHS) acn_block_reduce(s, m, S.part);
}

// partials of r.z
__global__ void __launch_bounds__(256) acn_dot_kernel(ACNPar A, ACNState S, const double *__restrict__ r, const double *__restrict__ z, size_t per) {
    const int b = blockIdx.z, n = A.nx * A.nx;
    if (!S.cg[b]) return;
    double s = 0.0;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
        const size_t o = (size_t)b * per + acn_at(A, q);
        s = fma(r[o], z[o], s);
    }
    acn_block_reduce(s, 0.0, S.part);
}

// p = z + beta p (beta = 0 in the first iteration of a Newton step: p is not read)
__global__ void __launch_bounds__(256) acn_dir_kernel(ACNPar A, ACNState S, const double *__restrict__ z, double *__restrict__ p, size_t per) {
    const int b = blockIdx.z, n = A.nx * A.nx;
    if (!S.cg[b]) return;
    const bool first = S.k_cg[b] == 0;
    const double beta = S.beta[b];
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
        const size_t o = (size_t)b * per + acn_at(A, q);
        p[o] = first ? z[o] : fma(beta, p[o], z[o]);
    }
}

// Jp = p - fac (L p + d o p), d = (1 - (nu + 1) x^nu) / eps^2 from x; partials of p.Jp
__global__ void __launch_bounds__(256) acn_jp_kernel(ACNPar A, ACNState S, const double *__restrict__ x, const double *__restrict__ p,
                                                     double *__restrict__ jp, size_t per) {
    const int b = blockIdx.z, n = A.nx * A.nx;
    if (!S.cg[b]) return;
    const double *pb = p + (size_t)b * per;
    double s = 0.0;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
        const size_t o = acn_at(A, q);
        const double d = (1.0 - (double)(A.nu + 1) * acn_pow(x[(size_t)b * per + o], A.nu)) * A.inv_eps2;
        const double pv = pb[o];
        const double v = fma(-A.fac, fma(d, pv, acn_lap(A, pb, q)), pv);
        jp[(size_t)b * per + o] = v;
        s = fma(pv, v, s);
    }
    acn_block_reduce(s, 0.0, S.part);
}

// delta += alpha p (= alpha p in the first iteration), r -= alpha Jp; partials of r.r
__global__ void __launch_bounds__(256) acn_update_kernel(ACNPar A, ACNState S, const double *__restrict__ p, const double *__restrict__ jp,
                                                         double *__restrict__ delta, double *__restrict__ r, size_t per) {
    const int b = blockIdx.z, n = A.nx * A.nx;
    if (!S.cg[b]) return;
    const bool first = S.k_cg[b] == 0;
    const double alpha = S.alpha[b];
    double s = 0.0;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
        const size_t o = (size_t)b * per + acn_at(A, q);
        delta[o] = first ? alpha * p[o] : fma(alpha, p[o], delta[o]);
        const double rv = fma(-alpha, jp[o], r[o]);
        r[o] = rv;
        s = fma(rv, rv, s);
    }
    acn_block_reduce(s, 0.0, S.part);
}

// x -= delta at the end of a Newton step (an inner iteration that ended before its first update leaves x as it is)
__global__ void __launch_bounds__(256) acn_step_kernel(ACNPar A, ACNState S, double *__restrict__ x, const double *__restrict__ delta, size_t per) {
    const int b = blockIdx.z, n = A.nx * A.nx;
    if (!S.act[b] || S.k_cg[b] == 0) return;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
        const size_t o = (size_t)b * per + acn_at(A, q);
        x[o] = x[o] - delta[o];
    }
}

// One thread per item sums the item's partials in index order and takes the item's decision; *word (pinned host memory) = the items
// of the batch still running (Newton: ACN_R_NEWTON; CG: ACN_R_RR) -- the one word the host reads.
enum { ACN_R_NEWTON = 0, ACN_R_RZ = 1, ACN_R_PJP = 2, ACN_R_RR = 3 };
template <int WHAT>
__global__ void __launch_bounds__(256) acn_reduce_kernel(ACNState S, int count, int nb, double newton_tol, double lin_tol, int lin_maxiter,
                                                         unsigned *__restrict__ word) {
    const int b = threadIdx.x;
    int running = 0;
    if (b < count && (WHAT == ACN_R_NEWTON ? S.act[b] : S.cg[b])) {
        const double *pt = S.part + (size_t)b * ACN_NB * 2;
        double s = 0.0, m = 0.0;
        for (int k = 0; k < nb; ++k) { s = s + pt[2 * k]; m = fmax(m, pt[2 * k + 1]); }
        if (WHAT == ACN_R_NEWTON) {
            if (m < newton_tol) {
                S.act[b] = 0;
            } else {
                S.n_newton[b] += 1; S.cg[b] = 1; S.k_cg[b] = 0; S.stop[b] = lin_tol * sqrt(s);
                running = 1;
            }
        } else if (WHAT == ACN_R_RZ) {
            S.beta[b] = S.k_cg[b] == 0 ? 0.0 : s / S.rz[b];
            S.rz[b] = s;
        } else if (WHAT == ACN_R_PJP) {
            if (!(s > 0.0)) S.cg[b] = 0;
            else S.alpha[b] = S.rz[b] / s;
        } else {
            const int k = S.k_cg[b] + 1;
            S.k_cg[b] = k; S.n_cg[b] += 1;
            if (s == 0.0 || sqrt(s) <= S.stop[b] || k >= lin_maxiter) S.cg[b] = 0;
            else running = 1;
        }
    }
    if (WHAT == ACN_R_NEWTON || WHAT == ACN_R_RR) {
        const int total = __syncthreads_count(running);
        if (threadIdx.x == 0) { *word = (unsigned)total; __threadfence_system(); }
    }
}

// the sweep's arithmetic on the converged x (the place of P2D_FIN in the IMEX step): grid point q of item b through h2d_apply_op
__global__ void __launch_bounds__(256) acn_finish_kernel(ACNPar A, const double *__restrict__ x, size_t per, H2DDev H, H2DFin F) {
    const int b = blockIdx.z, n = A.nx * A.nx;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) h2d_apply_op(H, F, b, (size_t)q, x[(size_t)b * per + acn_at(A, q)]);
}

// counts since the last mgrit_hip_newton_stats: Phi evaluated, Newton iterations, CG iterations, items that ended at newton_maxiter
__global__ void __launch_bounds__(256) acn_stats_kernel(ACNState S, int count, unsigned long long *__restrict__ tot) {
    const int b = threadIdx.x;
    if (b >= count) return;
    atomicAdd(tot + 0, 1ull);
    atomicAdd(tot + 1, (unsigned long long)S.n_newton[b]);
    atomicAdd(tot + 2, (unsigned long long)S.n_cg[b]);
    if (S.act[b]) atomicAdd(tot + 3, 1ull);
}
