// Gray-Scott 2-D device code: the pointwise map of the IMEX step of a two-species state and the kernels of the Newton-BiCGStab
// steps (gsn_*, which use the grid helpers and the stencil of mgrit_hip_allencahn.inc). Included by mgrit_hip.hip after
// mgrit_hip_allencahn.inc and mgrit_hip_periodic2d.inc, whose tile product (p2d_gemm_kernel, here with two planes per state and the two-operand form of
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
    static constexpr int operands = 2, items = 2;
    double dt, a, b; int comp;
    __device__ __forceinline__ double operator()(double own, double other) const {
        const double u = comp ? other : own, v = comp ? own : other;
        const double uv2 = u * (v * v);
        return comp ? fma(dt, uv2 - b * v, v) : fma(dt, a * (1.0 - u) - uv2, u);
    }
};

// ===============================================================================================================
// GrayScott, method 'IMPL' with linear_solver = 'bicgstab' (DESIGN.md 3.11, "The Newton-BiCGStab step"; the specification in numpy is
// GrayScott._step_bicgstab): per item Newton's method on F(x) = x - dt rate(x) - w from x = w, each correction J(x) delta = g by
// right-preconditioned BiCGStab with the shadow residual r^ = g, matrix-free, preconditioned with
// P = blockdiag((1 + dt a) I - dt du L, (1 + dt b) I - dt dv L) through the four Hartley products per species (p2d_gemm_kernel in its
// work modes with two planes, the shifted [2][P][P] table). The structure is that of acn_* (mgrit_hip_allencahn.inc): a batch's Phi is
// a host-driven loop over the kernels below (GSNBatch under newton_phi_batch in mgrit_hip.hip); blockIdx.z (or the thread of gsn_reduce_kernel) is the
// item. A work row of an item is two P x P planes [u | v], pads zero and never written. Per-item state lives in GSNState: an item whose
// Newton test has passed is FROZEN (act = 0) -- every kernel returns at once for it and its x is never written again --; lin = 1 while
// its inner iteration runs, half = 1 between the decision that the iteration ends with delta += alpha y only and that update.
// Reductions as acn_block_reduce / acn_reduce_kernel: fixed order, no floating-point atomics, an item's bits do not depend on its batch.
// ===============================================================================================================
constexpr int GSN_NB = 64;   // workgroups (and partials) per item of the elementwise kernels, at most

struct GSNState {
    int32_t *act, *lin, *half, *n_newton, *n_lin, *k_lin;   // per item: Newton running; BiCGStab running; half step pending; Newton /
                                                            // BiCGStab iterations of this Phi; BiCGStab iterations of this Newton step
    double *rho, *stop, *alpha, *omega, *beta;              // per item: r^ . r; lin_tol * norm2(g); the step lengths
    double *part;                                           // [item][GSN_NB][2] partials of the running reduction
};

struct GSNPar { ACNPar g; double du, dv, a, b, dt; };   // g: the grid (nx, P, 1 / dx^2) for acn_at / acn_lap; g.nu, g.inv_eps2, g.fac unused

// the workgroup's two values into part[item][blockIdx.x]: s0 summed; s1 summed, or (MAX) its maximum taken
template <bool MAX>
__device__ __forceinline__ void gsn_block_reduce(double s0, double s1, double *__restrict__ part) {
    __shared__ double l0[4], l1[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s0 = s0 + __shfl_down(s0, o, 64);
        const double t = __shfl_down(s1, o, 64);
        s1 = MAX ? fmax(s1, t) : s1 + t;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { l0[w] = s0; l1[w] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *o = part + ((size_t)blockIdx.z * GSN_NB + blockIdx.x) * 2;
        o[0] = ((l0[0] + l0[1]) + l0[2]) + l0[3];
        o[1] = MAX ? fmax(fmax(l1[0], l1[1]), fmax(l1[2], l1[3])) : ((l1[0] + l1[1]) + l1[2]) + l1[3];
    }
}

// x = w = the input row ([u | v], each plane natural nx x nx) on the item's two padded planes; the item's state reset
__global__ void __launch_bounds__(256) gsn_init_kernel(GSNPar A, GSNState S, const double *__restrict__ in_slab, const int32_t *__restrict__ in_idx,
                                                       int in_ld, double *__restrict__ x, double *__restrict__ w, size_t per) {
    const int b = blockIdx.z, n = A.g.nx * A.g.nx;
    const double *row = in_slab + (size_t)in_idx[b] * in_ld;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
        const size_t o = (size_t)b * 2 * per + acn_at(A.g, q);
        const double u = row[q], v = row[(size_t)n + q];
        x[o] = u; x[o + per] = v;
        w[o] = u; w[o + per] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        S.act[b] = 1; S.lin[b] = 0; S.half[b] = 0; S.n_newton[b] = 0; S.n_lin[b] = 0; S.k_lin[b] = 0;
    }
}

// g = F(x) into r and into the shadow residual r^ (delta starts at 0), partials sum g^2 and max |g|. Operand order of
// GrayScott._residual_bicgstab:  uv2 = u (v v);  rate_u = fma(du, lap u, a (1 - u) - uv2);  rate_v = fma(dv, lap v, uv2 - b v);
// g_c = fma(-dt, rate_c, x_c) - w_c
__global__ void __launch_bounds__(256) gsn_residual_kernel(GSNPar A, GSNState S, const double *__restrict__ x, const double *__restrict__ w,
                                                           double *__restrict__ r, double *__restrict__ rhat, size_t per) {
    const int b = blockIdx.z, n = A.g.nx * A.g.nx;
    if (!S.act[b]) return;
    const size_t base = (size_t)b * 2 * per;
    const double *xu = x + base, *xv = xu + per;
    double s = 0.0, m = 0.0;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
        const size_t o = acn_at(A.g, q);
        const double u = xu[o], v = xv[o];
        const double uv2 = u * (v * v);
        const double gu = fma(-A.dt, fma(A.du, acn_lap(A.g, xu, q), A.a * (1.0 - u) - uv2), u) - w[base + o];
        const double gv = fma(-A.dt, fma(A.dv, acn_lap(A.g, xv, q), uv2 - A.b * v), v) - w[base + per + o];
        r[base + o] = gu; r[base + per + o] = gv;
        rhat[base + o] = gu; rhat[base + per + o] = gv;
        s = fma(gv, gv, fma(gu, gu, s));
        m = fmax(m, fmax(fabs(gu), fabs(gv)));
    }
    gsn_block_reduce<true>(s, m, S.part);
}

// p = r + beta (p - omega v)  (p = r in the first iteration of a Newton step: p and v are not read)
__global__ void __launch_bounds__(256) gsn_dir_kernel(GSNPar A, GSNState S, const double *__restrict__ r, const double *__restrict__ v,
                                                      double *__restrict__ p, size_t per) {
    const int b = blockIdx.z, n = A.g.nx * A.g.nx;
    if (!S.lin[b]) return;
    const bool first = S.k_lin[b] == 0;
    const double beta = S.beta[b], omega = S.omega[b];
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const size_t o = (size_t)b * 2 * per + c * per + acn_at(A.g, q);
            p[o] = first ? r[o] : fma(beta, fma(-omega, v[o], p[o]), r[o]);
        }
    }
}

// out = J(x) y, operand order of GrayScott._jac_apply:  v2 = v v;  c = 2 (u v);
//   t_u = fma(du, lap y_u, -fma(v2 + a, y_u, c y_v));   t_v = fma(dv, lap y_v, fma(v2, y_u, (c - b) y_v));   out_c = fma(-dt, t_c, y_c)
// SECOND = false (v = J y): partial of d . out, d = r^  (sigma);  SECOND = true (t = J z): partials of out . d and out . out, d = s
template <bool SECOND>
__global__ void __launch_bounds__(256) gsn_jy_kernel(GSNPar A, GSNState S, const double *__restrict__ x, const double *__restrict__ y,
                                                     const double *__restrict__ d, double *__restrict__ out, size_t per) {
    const int b = blockIdx.z, n = A.g.nx * A.g.nx;
    if (!S.lin[b]) return;
    const size_t base = (size_t)b * 2 * per;
    const double *yu = y + base, *yv = yu + per;
    double s0 = 0.0, s1 = 0.0;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
        const size_t o = acn_at(A.g, q);
        const double u = x[base + o], v = x[base + per + o], pu = yu[o], pv = yv[o];
        const double v2 = v * v, c = 2.0 * (u * v);
        const double tu = fma(A.du, acn_lap(A.g, yu, q), -fma(v2 + A.a, pu, c * pv));
        const double tv = fma(A.dv, acn_lap(A.g, yv, q), fma(v2, pu, (c - A.b) * pv));
        const double ou = fma(-A.dt, tu, pu), ov = fma(-A.dt, tv, pv);
        out[base + o] = ou; out[base + per + o] = ov;
        s0 = fma(ov, d[base + per + o], fma(ou, d[base + o], s0));
        if (SECOND) s1 = fma(ov, ov, fma(ou, ou, s1));
    }
    gsn_block_reduce<false>(s0, s1, S.part);
}

// s = r - alpha v, partial of s . s
__global__ void __launch_bounds__(256) gsn_s_kernel(GSNPar A, GSNState S, const double *__restrict__ r, const double *__restrict__ v,
                                                    double *__restrict__ s, size_t per) {
    const int b = blockIdx.z, n = A.g.nx * A.g.nx;
    if (!S.lin[b]) return;
    const double alpha = S.alpha[b];
    double sum = 0.0;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const size_t o = (size_t)b * 2 * per + c * per + acn_at(A.g, q);
            const double sv = fma(-alpha, v[o], r[o]);
            s[o] = sv;
            sum = fma(sv, sv, sum);
        }
    }
    gsn_block_reduce<false>(sum, 0.0, S.part);
}

// the end of an inner iteration. lin: delta += alpha y + omega z, r = s - omega t, partials of r . r and r^ . r (the next rho);
// half: delta += alpha y only (r is not needed again). In the first iteration of a Newton step delta is set, not read.
__global__ void __launch_bounds__(256) gsn_update_kernel(GSNPar A, GSNState S, const double *__restrict__ y, const double *__restrict__ z,
                                                         const double *__restrict__ s, const double *__restrict__ t, const double *__restrict__ rhat,
                                                         double *__restrict__ delta, double *__restrict__ r, size_t per) {
    const int b = blockIdx.z, n = A.g.nx * A.g.nx;
    const bool lin = S.lin[b], half = S.half[b];
    if (!lin && !half) return;
    const bool first = S.k_lin[b] == 0;
    const double alpha = S.alpha[b], omega = S.omega[b];
    double s0 = 0.0, s1 = 0.0;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const size_t o = (size_t)b * 2 * per + c * per + acn_at(A.g, q);
            const double step = half ? alpha * y[o] : fma(omega, z[o], alpha * y[o]);
            delta[o] = first ? step : delta[o] + step;
            if (lin) {
                const double rv = fma(-omega, t[o], s[o]);
                r[o] = rv;
                s0 = fma(rv, rv, s0);
                s1 = fma(rhat[o], rv, s1);
            }
        }
    }
    if (lin) gsn_block_reduce<false>(s0, s1, S.part);
}

// x -= delta at the end of a Newton step (an inner iteration that ended before its first update leaves x as it is)
__global__ void __launch_bounds__(256) gsn_step_kernel(GSNPar A, GSNState S, double *__restrict__ x, const double *__restrict__ delta, size_t per) {
    const int b = blockIdx.z, n = A.g.nx * A.g.nx;
    if (!S.act[b] || S.k_lin[b] == 0) return;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const size_t o = (size_t)b * 2 * per + c * per + acn_at(A.g, q);
            x[o] = x[o] - delta[o];
        }
    }
}

// One thread per item sums the item's partials in index order and takes the item's decision; *word (pinned host memory) = the items
// of the batch still running (GSN_R_NEWTON: Newton; GSN_R_FULL: BiCGStab) -- the one word the host reads.
//   GSN_R_NEWTON  max|g| < newton_tol: frozen; else a Newton iteration begins: stop = lin_tol norm2(g), rho = g . g (r^ = r = g)
//   GSN_R_SIGMA   sigma = r^ . v: zero or not finite ends the inner iteration (nothing added); else alpha = rho / sigma
//   GSN_R_HALF    norm2(s) <= stop: the iteration ends with the half step
//   GSN_R_OMEGA   omega = (t . s) / (t . t); t . t = 0, omega = 0 or not finite: the iteration ends with the half step
//   GSN_R_FULL    the iteration is counted; it ends on norm2(r) <= stop, at lin_maxiter, or where the next rho or beta is zero / not finite
enum { GSN_R_NEWTON = 0, GSN_R_SIGMA = 1, GSN_R_HALF = 2, GSN_R_OMEGA = 3, GSN_R_FULL = 4 };
template <int WHAT>
__global__ void __launch_bounds__(256) gsn_reduce_kernel(GSNState S, int count, int nb, double newton_tol, double lin_tol, int lin_maxiter,
                                                         unsigned *__restrict__ word) {
    const int b = threadIdx.x;
    int running = 0;
    if (b < count && WHAT == GSN_R_FULL && S.half[b]) {   // the half step has been added: counted, the item's inner iteration is over
        S.half[b] = 0; S.k_lin[b] += 1; S.n_lin[b] += 1;
    } else if (b < count && (WHAT == GSN_R_NEWTON ? S.act[b] : S.lin[b])) {
        const double *pt = S.part + (size_t)b * GSN_NB * 2;
        double s0 = 0.0, s1 = 0.0;
        for (int k = 0; k < nb; ++k) {
            s0 = s0 + pt[2 * k];
            s1 = WHAT == GSN_R_NEWTON ? fmax(s1, pt[2 * k + 1]) : s1 + pt[2 * k + 1];
        }
        if (WHAT == GSN_R_NEWTON) {
            if (s1 < newton_tol) {
                S.act[b] = 0;
            } else {
                S.n_newton[b] += 1; S.k_lin[b] = 0; S.stop[b] = lin_tol * sqrt(s0); S.rho[b] = s0;
                if (s0 != 0.0 && isfinite(s0) && lin_maxiter > 0) { S.lin[b] = 1; running = 1; }
            }
        } else if (WHAT == GSN_R_SIGMA) {
            const double alpha = S.rho[b] / s0;
            if (s0 == 0.0 || !isfinite(s0) || !isfinite(alpha)) S.lin[b] = 0;
            else S.alpha[b] = alpha;
        } else if (WHAT == GSN_R_HALF) {
            if (sqrt(s0) <= S.stop[b]) { S.lin[b] = 0; S.half[b] = 1; }
        } else if (WHAT == GSN_R_OMEGA) {
            const double omega = s1 != 0.0 ? s0 / s1 : 0.0;
            if (s1 == 0.0 || omega == 0.0 || !isfinite(omega)) { S.lin[b] = 0; S.half[b] = 1; }
            else S.omega[b] = omega;
        } else {
            const int k = S.k_lin[b] + 1;
            S.k_lin[b] = k; S.n_lin[b] += 1;
            const double beta = (s1 / S.rho[b]) * (S.alpha[b] / S.omega[b]);
            if (sqrt(s0) <= S.stop[b] || k >= lin_maxiter || s1 == 0.0 || !isfinite(s1) || !isfinite(beta)) S.lin[b] = 0;
            else { S.beta[b] = beta; S.rho[b] = s1; running = 1; }
        }
    }
    if (WHAT == GSN_R_NEWTON || WHAT == GSN_R_FULL) {
        const int total = __syncthreads_count(running);
        if (threadIdx.x == 0) { *word = (unsigned)total; __threadfence_system(); }
    }
}

// the sweep's arithmetic on the converged x (the place of P2D_FIN in the IMEX step): offset c nx^2 + i nx + j of the destination row
__global__ void __launch_bounds__(256) gsn_finish_kernel(GSNPar A, const double *__restrict__ x, size_t per, H2DDev H, H2DFin F) {
    const int b = blockIdx.z, n = A.g.nx * A.g.nx;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
#pragma unroll
        for (int c = 0; c < 2; ++c) h2d_apply_op(H, F, b, (size_t)c * n + q, x[(size_t)b * 2 * per + c * per + acn_at(A.g, q)]);
    }
}

// counts since the last mgrit_hip_newton_stats: Phi evaluated, Newton iterations, BiCGStab iterations, items that ended at newton_maxiter
__global__ void __launch_bounds__(256) gsn_stats_kernel(GSNState S, int count, unsigned long long *__restrict__ tot) {
    const int b = threadIdx.x;
    if (b >= count) return;
    atomicAdd(tot + 0, 1ull);
    atomicAdd(tot + 1, (unsigned long long)S.n_newton[b]);
    atomicAdd(tot + 2, (unsigned long long)S.n_lin[b]);
    if (S.act[b]) atomicAdd(tot + 3, 1ull);
}
