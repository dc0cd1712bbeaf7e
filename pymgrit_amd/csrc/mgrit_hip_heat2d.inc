// Heat2D device code: the batched FP64 MFMA GEMM and the elementwise rhs / epilogue / norm kernels.
// Included by mgrit_hip.hip inside its anonymous namespace; the host side (tables, batch plans) stays in mgrit_hip.hip.

// ===============================================================================================================
// Heat2D (heat/heat_2d.py:250-366): theta-scheme on the full nx x ny grid. Interior solve by fast diagonalisation
//   U = Qx ((Qx B Qy) o D) Qy,  Qx, Qy orthogonal symmetric sine-transform matrices,
// i.e. four dense FP64 GEMMs per step, batched over all time points a sweep updates at once. The GEMMs run on the matrix
// cores with v_mfma_f64_16x16x4_f64, which accumulates its four k-products as a sequential fma chain (verified on gfx950):
// a K loop in ascending order without split-K is bit-identical to the oracle's plain fma dot product (DESIGN.md 3.5).
// Every product has the form  out[n][m] = sum_k A[k][m] * B[k][n]  (A symmetric table, output stored transposed), so
// all operands are read along their contiguous dimension and the four steps chain without any explicit transpose.
// ===============================================================================================================
enum { H2D_OP_F = 0, H2D_OP_C = 1, H2D_OP_FAS_FINE = 2, H2D_OP_FAS_COARSE = 3, H2D_OP_RESIDUAL = 4, H2D_OP_JUMP = 5,
       /* time-parallel forward solve (DESIGN.md 3.8): dst += value (the propagated part of a block end);
          dst = (a + value) - b (the error a block has accumulated: (g_i + Phi(u_{i-1} + x)) - u_i) */
       H2D_OP_ADD = 6, H2D_OP_DEFECT = 7 };

struct H2DDev {
    int nx, ny, mi, mj, Mi, Mj, K, n_pts, ld, has_w;
    double fx, fy, theta;
    const double *bc;    // [nx*ny] boundary values (zero inside)
    const double *W;     // [Mi][Mj] boundary coupling (zero padded)
    const double *S;     // [K][Mi][Mj] forcing space factors (zero padded)
    const double *tstop; // [K][n_pts] tau_k(t_i)
    const double *dt;    // [n_pts]
    const double *fb;    // general forcing (mgrit_hip_level_heat2d_forcing_rows): [n_pts][Mi][Mj] values rhs(x, y, t_i) on the
                         // padded interior, caller-owned like the state slabs; null: none
};

typedef double d4_t __attribute__((ext_vector_type(4)));
typedef double d2_t __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------------------------
// Half-size sine transforms (DESIGN.md 3.5). The sine matrix Q[i][k] = s sin(pi (i+1)(k+1)/(m+1)) of one axis satisfies
// Q[m-1-i][k] = (-1)^k Q[i][k]: with the folded inputs xe[k] = x[k] + x[m-1-k], xo[k] = x[k] - x[m-1-k] the even modes
// need only Fe[k][e] = Q[k][2e] and the odd modes only Fo[k][o] = Q[k][2o+1], k < ceil(m/2) -- half the matrix-core work of
// the full product. Spectral layout of an axis: even modes in slots [0, HP), odd modes in [HP, 2 HP), HP = the half size
// padded to 64; natural layout: index i in slot i; both have P = 2 HP slots, pads are zero / never read.
//   forward: out[n][slot] = sum_k F[k][slot'] * (B[k][n] +- B[m-1-k][n])      (fold while staging the B tile)
//   inverse: out[n][i] = Pe + Po, out[n][m-1-i] = Pe - Po,  Pe = sum_e FeT[e][i] B[e][n], Po = sum_o FoT[o][i] B[HP+o][n]
// Every dot product is an fma chain over ascending k (the MFMA accumulates its four k-products in order): bit-identical to
// the oracle's loops. 64x64 tile per workgroup, 4 waves x (32x32 = 2x2 MFMA tiles), K step 32 through LDS (rows padded to
// 80 doubles), the operands of the next K step prefetched into registers behind LDS-only barriers.
// ---------------------------------------------------------------------------------------------------------------
constexpr int H2D_BK = 32, H2D_LDT = 80;

// one K loop of the tile product: acc += A[k][m0 + .] x Bop[k][n0 + .], k in [0, KP). FOLD: Bop row k is staged as
// B[k] + sign * B[m-1-k] for k < hO and as B[k] otherwise (fma with the multiplier sign or 0: exactly the sum / difference).
// GRID (with FOLD): Bop is not the padded right-hand side in the work slab but the INTERIOR of a grid row of the state slab itself
// (Bb = the row's point (1, 1), N = ny, n_real = interior columns) -- the homogeneous backward-Euler step, whose right-hand side is
// the interior of u bit for bit (h2d_rhs_kernel with theta = 1, no forcing, no boundary coupling): the tile is staged straight
// from the state, rows >= m_real and columns >= n_real as the zeros the padded slab holds there, and the rhs launch with its
// 2 x 8 B per point of HBM traffic falls away. The interior starts one point into a row, so these loads are 8-byte aligned only.
typedef double d2u_t __attribute__((ext_vector_type(2), aligned(8)));
// PRE (with GRID): a pointwise map applied to every value staged from the state row before it enters the product -- the identity for
// Heat2D, the non-linear right-hand side of the Allen-Cahn IMEX step (mgrit_hip_allencahn.inc). PRE::operands == 2: the map reads a
// second value at the staged point, pre(x, y) with y from Bb2 -- the same point of another plane of the state row, loaded beside x
// with the same clamps (Gray-Scott, mgrit_hip_grayscott.inc: the other species). For operands == 1 Bb2 is never read and the
// instances compile to what they are without it (DESIGN.md 3.11).
struct H2DIdentity {
    static constexpr int operands = 1;
    __device__ __forceinline__ double operator()(double x) const { return x; }
};
template <bool FOLD, bool GRID = false, class PRE = H2DIdentity>
__device__ __forceinline__ void h2d_kloop(d4_t (&acc)[2][2], double *smem, const double *__restrict__ A, int lda, int m0,
                                          const double *__restrict__ Bb, int N, int n0, int KP, int m_real, int hO, double sign,
                                          int tid, int lane, int w, int n_real = 0, PRE pre = PRE(),
                                          const double *__restrict__ Bb2 = nullptr) {
    constexpr bool TWO = PRE::operands == 2;
    static_assert(!TWO || (GRID && !FOLD), "a two-operand map is applied to values staged from a state row");
    double(*As)[H2D_LDT] = reinterpret_cast<double(*)[H2D_LDT]>(smem);
    double(*Bs)[H2D_LDT] = reinterpret_cast<double(*)[H2D_LDT]>(smem + H2D_BK * H2D_LDT);
    const int wm = (w & 1) * 32, wn = (w >> 1) * 32;
    const int lr = lane & 15, lk = lane >> 4;
    const int sr = tid >> 5, sc = (tid & 31) * 2;
    d2_t ra[H2D_BK / 8], rb[H2D_BK / 8], rc[H2D_BK / 8], rb2[H2D_BK / 8];
    const bool cv0 = !GRID || n0 + sc < n_real, cv1 = !GRID || n0 + sc + 1 < n_real;   // (a valid column's pair stays inside its row)
    const double *Ap = A + (size_t)sr * lda + m0 + sc, *Bp = Bb + (cv0 ? n0 + sc : 0);
    const double *Bp2 = TWO ? Bb2 + (cv0 ? n0 + sc : 0) : nullptr;
    auto ldb = [&](const double *q) -> d2_t {
        if (GRID) return (d2_t)*reinterpret_cast<const d2u_t *>(q);
        return *reinterpret_cast<const d2_t *>(q);
    };
    auto fetch = [&](int k0) {
#pragma unroll
        for (int h = 0; h < H2D_BK / 8; ++h) {
            const int k = k0 + sr + 8 * h;
            ra[h] = *reinterpret_cast<const d2_t *>(Ap + (size_t)(k0 + 8 * h) * lda);
            rb[h] = ldb(Bp + (size_t)(GRID && k >= m_real ? m_real - 1 : k) * N);
            if constexpr (TWO) rb2[h] = ldb(Bp2 + (size_t)(k >= m_real ? m_real - 1 : k) * N);
            if (FOLD) {
                const int km = m_real - 1 - k;
                rc[h] = ldb(Bp + (size_t)(km > 0 ? km : 0) * N);
            }
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < KP; k0 += H2D_BK) {
#pragma unroll
        for (int h = 0; h < H2D_BK / 8; ++h) {
            d2_t bv = rb[h];
            if (GRID) {
                const bool rv = (k0 + sr + 8 * h) < m_real;
                if constexpr (TWO) {
                    bv.x = rv && cv0 ? pre(bv.x, rb2[h].x) : 0.0;
                    bv.y = rv && cv1 ? pre(bv.y, rb2[h].y) : 0.0;
                } else {
                    bv.x = rv && cv0 ? pre(bv.x) : 0.0;
                    bv.y = rv && cv1 ? pre(bv.y) : 0.0;
                }
            }
            if (FOLD) {
                const double mult = (k0 + sr + 8 * h) < hO ? sign : 0.0;
                bv.x = fma(mult, GRID && !cv0 ? 0.0 : rc[h].x, bv.x);
                bv.y = fma(mult, GRID && !cv1 ? 0.0 : rc[h].y, bv.y);
            }
            *reinterpret_cast<d2_t *>(&As[sr + 8 * h][sc]) = ra[h];
            *reinterpret_cast<d2_t *>(&Bs[sr + 8 * h][sc]) = bv;
        }
        lds_barrier();
        fetch(k0 + H2D_BK < KP ? k0 + H2D_BK : k0);   // next K step in flight while the matrix cores work (last trip: its own)
#pragma unroll
        for (int kk = 0; kk < H2D_BK / 4; ++kk) {
            const double a0 = As[kk * 4 + lk][wm + lr], a1 = As[kk * 4 + lk][wm + 16 + lr];
            const double b0 = Bs[kk * 4 + lk][wn + lr], b1 = Bs[kk * 4 + lk][wn + 16 + lr];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        lds_barrier();
    }
}

// D[row = lk + 4r][col = lr] of MFMA tile (tm, tn) is element (m = wm + 16 tm + lk + 4r, n = wn + 16 tn + lr): into Cs[n][m]
__device__ __forceinline__ void h2d_acc_to_lds(const d4_t (&acc)[2][2], double (*Cs)[66], int lane, int w) {
    const int wm = (w & 1) * 32, wn = (w >> 1) * 32, lr = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 4; ++r) Cs[wn + 16 * tn + lr][wm + 16 * tm + lk + 4 * r] = acc[tm][tn][r];
}

// The first generation of workgroups of a launch starts staggered by its wave slot (0 .. 3 on a SIMD, a quarter of a tile's
// lifetime apart): four workgroups per CU that start together also reach their epilogues and their successors' prologues together,
// and the matrix pipe idles through all four at once. Measured on config 4's level-0 F-relaxation: 0.735 -> 0.746 of the peak.
__device__ __forceinline__ void h2d_stagger() {
    const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    if (lin < 1024u && gridDim.x * gridDim.y * gridDim.z >= 4096u) {   // (big batches only: a single state's 64 tiles are one generation)
        const unsigned slot = __builtin_amdgcn_s_getreg(6148) & 3u;   // HW_ID bits 3:0 = wave slot: hwreg(4, 0, 4)
        for (unsigned i = 0; i < 2u * slot; ++i) __builtin_amdgcn_s_sleep(127);
    }
}

// forward half transform; grid (n tiles, slot tiles = 2 HP / 64: the first HP / 64 are the even modes, items)
// GRID: item b's operand is the interior of the state row B[in_idx[b] * in_ld + .] (see h2d_kloop), n_real its interior columns
template <bool SCALE, bool GRID = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) h2d_fwd_kernel(const double *__restrict__ Fe, const double *__restrict__ Fo, int m_real,
                                                      int HP, const double *__restrict__ B, int N, double *__restrict__ out,
                                                      const double *__restrict__ dinv, size_t bstride,
                                                      const int32_t *__restrict__ in_idx = nullptr, int in_ld = 0, int n_real = 0) {
    __shared__ __attribute__((aligned(16))) double smem[2 * H2D_BK * H2D_LDT];
    double(*Cs)[66] = reinterpret_cast<double(*)[66]>(smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, P = 2 * HP;
    h2d_stagger();
    const int n0 = blockIdx.x * 64, s0 = blockIdx.y * 64;           // s0: first output slot of the tile
    const bool odd = s0 >= HP;
    const double *Bb = GRID ? B + (size_t)in_idx[blockIdx.z] * in_ld + N + 1 : B + (size_t)blockIdx.z * bstride;
    double *Ob = out + (size_t)blockIdx.z * bstride;
    d4_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (d4_t){0.0, 0.0, 0.0, 0.0};
    h2d_kloop<true, GRID>(acc, smem, odd ? Fo : Fe, HP, odd ? s0 - HP : s0, Bb, N, n0, HP, m_real, m_real / 2, odd ? -1.0 : 1.0,
                          tid, lane, w, n_real);
    h2d_acc_to_lds(acc, Cs, lane, w);
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int n = (tid >> 4) + 16 * p, c = (tid & 15) * 4;
        double v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = Cs[n][c + q];
        const size_t o = (size_t)(n0 + n) * P + s0 + c;
        if (SCALE) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = v[q] * dinv[o + q];
        }
        *reinterpret_cast<double2 *>(Ob + o) = make_double2(v[0], v[1]);
        *reinterpret_cast<double2 *>(Ob + o + 2) = make_double2(v[2], v[3]);
    }
}

// the sweep's own arithmetic on the value phi = Phi(u_in) at grid point p of batch item b (ops: see H2D_OP_*): operands of the
// epilogue kernel h2d_finish_kernel, also applied by the LAST inverse transform itself (h2d_inv_kernel<true>) so that the
// interior of U never travels through HBM between the two
struct H2DFin {
    double *dst_slab; int dst_ld; const int32_t *dst_idx;
    const double *a_slab; const int32_t *a_idx;
    const double *b_slab; const int32_t *b_idx;
    int op, use_g; double w, w1;
};

__device__ __forceinline__ void h2d_apply_op(const H2DDev &H, const H2DFin &F, int b, size_t p, double phi) {
    double *dst = F.dst_slab + (size_t)F.dst_idx[b] * F.dst_ld;
    double v;
    if (F.op == H2D_OP_F) {
        v = F.use_g ? F.a_slab[(size_t)F.a_idx[b] * H.ld + p] + phi : phi;                       // [g_i +] Phi
    } else if (F.op == H2D_OP_C) {
        v = F.use_g ? F.a_slab[(size_t)F.a_idx[b] * H.ld + p] + phi : phi;
        if (F.w != 1.0) v = v * F.w + dst[p] * F.w1;                                             // weighted with the old u_i
    } else if (F.op == H2D_OP_FAS_FINE) {
        const double ui = F.b_slab[(size_t)F.b_idx[b] * H.ld + p];
        v = F.use_g ? (F.a_slab[(size_t)F.a_idx[b] * H.ld + p] - ui) + phi : phi - ui;           // (g_i - u_i) + Phi | Phi - u_i
    } else if (F.op == H2D_OP_ADD) {
        v = dst[p] + phi;
    } else if (F.op == H2D_OP_DEFECT) {
        v = (F.a_slab[(size_t)F.a_idx[b] * H.ld + p] + phi) - F.b_slab[(size_t)F.b_idx[b] * H.ld + p];
    } else {  // H2D_OP_FAS_COARSE: (g_j + v_j) - Phi(v_{j-1})
        v = (F.a_slab[(size_t)F.a_idx[b] * H.ld + p] + F.b_slab[(size_t)F.b_idx[b] * H.ld + p]) - phi;
    }
    dst[p] = v;
}

// inverse half transform; grid (n tiles, i tiles = HP / 64, items): the tile's Pe and Po, then the butterfly.
// FIN (the second inverse transform of a step, out[n][i] = U at interior point (n, i)): the values go through the sweep's
// arithmetic straight into the destination rows (grid point (n + 1, i + 1)) instead of into the work slab; the rim of the grid
// is h2d_rim_kernel's.
template <bool FIN>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) h2d_inv_kernel(const double *__restrict__ FeT, const double *__restrict__ FoT, int m_real,
                                                      int HP, const double *__restrict__ B, int N, double *__restrict__ out,
                                                      size_t bstride, H2DDev H, H2DFin F) {
    __shared__ __attribute__((aligned(16))) double smem[2 * H2D_BK * H2D_LDT];
    double(*Cs)[66] = reinterpret_cast<double(*)[66]>(smem);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, P = 2 * HP;
    h2d_stagger();
    const int n0 = blockIdx.x * 64, i0 = blockIdx.y * 64;
    const int hE = (m_real + 1) / 2, hO = m_real / 2;
    const double *Bb = B + (size_t)blockIdx.z * bstride;
    double *Ob = out + (size_t)blockIdx.z * bstride;
    d4_t pe[2][2], po[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { pe[a][b] = (d4_t){0.0, 0.0, 0.0, 0.0}; po[a][b] = (d4_t){0.0, 0.0, 0.0, 0.0}; }
    h2d_kloop<false>(pe, smem, FeT, HP, i0, Bb, N, n0, HP, 0, 0, 0.0, tid, lane, w);
    h2d_kloop<false>(po, smem, FoT, HP, i0, Bb + (size_t)HP * N, N, n0, HP, 0, 0, 0.0, tid, lane, w);
    d4_t lo[2][2], hi[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { lo[a][b] = pe[a][b] + po[a][b]; hi[a][b] = pe[a][b] - po[a][b]; }
    // out[n][i] = Pe + Po for i < hE (rows of 64 values, stored 16 B at a time)
    h2d_acc_to_lds(lo, Cs, lane, w);
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int n = (tid >> 4) + 16 * p, c = (tid & 15) * 4;
        double *o = Ob + (size_t)(n0 + n) * P + i0 + c;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (i0 + c + q < hE) {
                if (!FIN) o[q] = Cs[n][c + q];
                else if (n0 + n < H.mi) h2d_apply_op(H, F, blockIdx.z, (size_t)(n0 + n + 1) * H.ny + (i0 + c + q + 1), Cs[n][c + q]);
            }
    }
    __syncthreads();
    // out[n][m-1-i] = Pe - Po for i < hO: the mirrored half, a descending run of addresses per row
    h2d_acc_to_lds(hi, Cs, lane, w);
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int n = (tid >> 4) + 16 * p, c = (tid & 15) * 4;
        double *row = Ob + (size_t)(n0 + n) * P;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (i0 + c + q < hO) {
                if (!FIN) row[m_real - 1 - (i0 + c + q)] = Cs[n][c + q];
                else if (n0 + n < H.mi) h2d_apply_op(H, F, blockIdx.z, (size_t)(n0 + n + 1) * H.ny + (m_real - 1 - (i0 + c + q) + 1), Cs[n][c + q]);
            }
    }
}

__device__ __forceinline__ double h2d_lap(const H2DDev &H, const double *u, int gi, int gj) {
    const int ny = H.ny;
    double acc = (2.0 * (H.fx + H.fy)) * u[(size_t)gi * ny + gj];
    acc = fma(-H.fx, u[(size_t)(gi - 1) * ny + gj], acc);
    acc = fma(-H.fx, u[(size_t)(gi + 1) * ny + gj], acc);
    acc = fma(-H.fy, u[(size_t)gi * ny + gj - 1], acc);
    acc = fma(-H.fy, u[(size_t)gi * ny + gj + 1], acc);
    return acc;
}

// right-hand side of the implicit solve on the padded interior: B[b][a][c] (heat_2d.py:289-320, DESIGN.md 3.5)
__global__ void h2d_rhs_kernel(H2DDev H, const double *__restrict__ slab, const int32_t *__restrict__ in_idx,
                               const int32_t *__restrict__ step_idx, double *__restrict__ B) {
    const int b = blockIdx.z, a = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= H.Mj) return;
    double v = 0.0;
    if (a < H.mi && c < H.mj) {
        const double *u = slab + (size_t)in_idx[b] * H.ld;
        const int i = step_idx[b];
        const double dt = H.dt[i], th = H.theta;
        const size_t p = (size_t)(a + 1) * H.ny + (c + 1), q = (size_t)a * H.Mj + c;
        if (th == 1.0) {
            v = u[p];
            for (int k = 0; k < H.K; ++k) v = fma(H.S[(size_t)k * H.Mi * H.Mj + q], H.tstop[(size_t)k * H.n_pts + i] * dt, v);
            if (H.fb) v = fma(H.fb[(size_t)i * H.Mi * H.Mj + q], dt, v);
        } else {
            const double thdt = th * dt, thdt1 = (1.0 - th) * dt;
            v = fma(-thdt, h2d_lap(H, u, a + 1, c + 1), u[p]);
            for (int k = 0; k < H.K; ++k)
                v = fma(H.S[(size_t)k * H.Mi * H.Mj + q],
                        thdt * H.tstop[(size_t)k * H.n_pts + i] + thdt1 * H.tstop[(size_t)k * H.n_pts + i - 1], v);
            if (H.fb) {
                v = fma(H.fb[(size_t)i * H.Mi * H.Mj + q], thdt, v);
                v = fma(H.fb[(size_t)(i - 1) * H.Mi * H.Mj + q], thdt1, v);
            }
        }
        if (H.has_w) v = fma(th * dt, H.W[q], v);
    }
    B[((size_t)b * H.Mi + a) * H.Mj + c] = v;
}

// value of Phi(u_in) at grid point (gi, gj) of batch item b: interior from the GEMM result U (theta > 0) or the explicit
// stencil (theta = 0, heat_2d.py:346-356 incl. the reference's "BC + old boundary" behaviour)
__device__ __forceinline__ double h2d_phi_value(const H2DDev &H, const double *U, const double *uin, int step, int b, int gi,
                                                int gj) {
    const size_t p = (size_t)gi * H.ny + gj;
    const bool rim = gi == 0 || gj == 0 || gi == H.nx - 1 || gj == H.ny - 1;
    if (H.theta == 0.0) {
        if (rim) return H.bc[p] + uin[p];
        const double dt = H.dt[step];
        double v = fma(-dt, h2d_lap(H, uin, gi, gj), uin[p]);
        for (int k = 0; k < H.K; ++k)
            v = fma(H.S[(size_t)k * H.Mi * H.Mj + (size_t)(gi - 1) * H.Mj + (gj - 1)], dt * H.tstop[(size_t)k * H.n_pts + step - 1], v);
        if (H.fb) v = fma(H.fb[((size_t)(step - 1) * H.Mi + (gi - 1)) * H.Mj + (gj - 1)], dt, v);
        return v;
    }
    return rim ? H.bc[p] : U[((size_t)b * H.Mi + (gi - 1)) * H.Mj + (gj - 1)];
}

// sweep epilogue on full-grid rows: one thread per grid point (ops: see H2D_OP_*)
__global__ void h2d_finish_kernel(H2DDev H, const double *__restrict__ U, const double *__restrict__ in_slab,
                                  const int32_t *__restrict__ in_idx, const int32_t *__restrict__ step_idx,
                                  double *__restrict__ dst_slab, int dst_ld, const int32_t *__restrict__ dst_idx,
                                  const double *__restrict__ a_slab, const int32_t *__restrict__ a_idx,
                                  const double *__restrict__ b_slab, const int32_t *__restrict__ b_idx, int op, int use_g,
                                  double w, double w1) {
    const int b = blockIdx.z, gi = blockIdx.y, gj = blockIdx.x * blockDim.x + threadIdx.x;
    if (gj >= H.ny) return;
    const size_t p = (size_t)gi * H.ny + gj;
    const double *uin = in_slab + (size_t)in_idx[b] * H.ld;
    const double phi = h2d_phi_value(H, U, uin, step_idx[b], b, gi, gj);
    const H2DFin F{dst_slab, dst_ld, dst_idx, a_slab, a_idx, b_slab, b_idx, op, use_g, w, w1};
    h2d_apply_op(H, F, b, p, phi);
}

// the rim of the grid of a step whose interior h2d_inv_kernel<true> has written: Phi = the boundary values (theta > 0)
__global__ void h2d_rim_kernel(H2DDev H, H2DFin F) {
    const int b = blockIdx.y, r = blockIdx.x * blockDim.x + threadIdx.x;
    const int n_rim = 2 * H.ny + 2 * (H.nx - 2);
    if (r >= n_rim) return;
    int gi, gj;
    if (r < H.ny) { gi = 0; gj = r; }
    else if (r < 2 * H.ny) { gi = H.nx - 1; gj = r - H.ny; }
    else { const int k = r - 2 * H.ny; gi = 1 + (k >> 1); gj = (k & 1) ? H.ny - 1 : 0; }
    const size_t p = (size_t)gi * H.ny + gj;
    h2d_apply_op(H, F, b, p, H.bc[p]);
}

// residual / jump: per grid row an fma chain over its ny values in ascending order, then the rows in order (h2d_rowsum_kernel).
// One wave per (item, 64 rows): the differences of a 64 x 64 tile are formed with coalesced reads (lane = column) and passed
// through LDS to the lane that owns the row, which adds them in column order -- the chain of the oracle. (Round 4; as a thread
// per row reading its row on its own, 64 rows 4 KB apart per load instruction, the residual check of config 4 took 18.4 us per
// point against 10.5 for the Phi alone.)
// FULL: U holds Phi on the whole grid, no rim (Allen-Cahn: periodic)
// NC > 1 (Gray-Scott): a state row is NC planes of nx x ny values and blockIdx.y runs over (state, plane), the plane fastest -- the work
// slab item of U and the rows of rowsq follow blockIdx.y, so h2d_rowsum_kernel over NC * nx rows adds a state's planes in order
template <bool FULL, int NC = 1>
__global__ void __launch_bounds__(64) h2d_rowsq_kernel(H2DDev H, const double *__restrict__ U, const double *__restrict__ in_slab,
                                                       const int32_t *__restrict__ in_idx, const int32_t *__restrict__ step_idx,
                                                       const double *__restrict__ cmp_slab, const int32_t *__restrict__ cmp_idx, int op,
                                                       double *__restrict__ rowsq) {
    __shared__ double tile[64][65];
    const int b = blockIdx.y, r0 = blockIdx.x * 64, lane = threadIdx.x;
    const int st = NC == 1 ? b : b / NC;                                         // the state of the batch
    const size_t plane = NC == 1 ? 0 : (size_t)(b % NC) * H.nx * H.ny;
    const double *uin = in_slab + (size_t)in_idx[st] * H.ld + plane;
    const double *cmp = cmp_slab + (size_t)cmp_idx[st] * H.ld + plane;
    const int step = step_idx[st];
    double acc = 0.0;
    for (int c0 = 0; c0 < H.ny; c0 += 64) {
        const int gj = c0 + lane;
        for (int rr = 0; rr < 64; ++rr) {
            const int gi = r0 + rr;
            double r = 0.0;
            if (gi < H.nx && gj < H.ny) {
                const size_t p = (size_t)gi * H.ny + gj;
                r = op == H2D_OP_RESIDUAL ? (FULL ? U[((size_t)b * H.Mi + gi) * H.Mj + gj] : h2d_phi_value(H, U, uin, step, b, gi, gj)) - cmp[p]
                                             : uin[p] - cmp[p];
            }
            tile[rr][lane] = r;
        }
        __syncthreads();
        const int nc = H.ny - c0 < 64 ? H.ny - c0 : 64;
        for (int cc = 0; cc < nc; ++cc) {
            const double r = tile[lane][cc];
            acc = fma(r, r, acc);
        }
        __syncthreads();
    }
    if (r0 + lane < H.nx) rowsq[(size_t)b * H.nx + r0 + lane] = acc;
}

// pos: where item b's sum goes (the items of a point list are grouped by time-step size, so a batch is not in list order)
__global__ void h2d_rowsum_kernel(const double *__restrict__ rowsq, int nx, int count, double *__restrict__ out,
                                  const int32_t *__restrict__ pos) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= count) return;
    double tot = 0.0;
    for (int i = 0; i < nx; ++i) tot = tot + rowsq[(size_t)b * nx + i];
    out[pos[b]] = tot;
}


// ---- time-parallel forward solve (DESIGN.md 3.8; backward Euler): the block ends through the transforms above ----------------------
// interior of the rows slab[idx[b]] on the padded Mi x Mj grid (zero padded), the transforms' input layout
__global__ void h2d_pack_kernel(H2DDev H, const double *__restrict__ slab, const int32_t *__restrict__ idx, double *__restrict__ B) {
    const int b = blockIdx.z, a = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= H.Mj) return;
    double v = 0.0;
    if (a < H.mi && c < H.mj) v = slab[(size_t)idx[b] * H.ld + (size_t)(a + 1) * H.ny + (c + 1)];
    B[((size_t)b * H.Mi + a) * H.Mj + c] = v;
}

// full-grid rows: dst[di[k]] = a[ai[k] + a_shift] + b[bi[k]]  (the next step's input u_{i-1} + x; the block end u[e_b] + W_b)
__global__ void h2d_sum_rows_kernel(int ld, int n, double *__restrict__ dst, const int32_t *__restrict__ di,
                                    const double *__restrict__ a, const int32_t *__restrict__ ai, int a_shift,
                                    const double *__restrict__ b, const int32_t *__restrict__ bi) {
    const int k = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    dst[(size_t)di[k] * ld + p] = a[(size_t)(ai[k] + a_shift) * ld + p] + b[(size_t)bi[k] * ld + p];
}

// theta < 1: does any of the rows X[0 .. gridDim.x - 1] (the errors at the block ends the recurrence reads) hold a non-zero value on
// the rim of the nx x ny grid? One workgroup per row; *flag (pinned host memory) is set, never cleared, by the kernel.
__global__ void __launch_bounds__(256) h2d_rim_check_kernel(H2DDev H, const double *__restrict__ X, int ld, unsigned *flag) {
    const double *row = X + (size_t)blockIdx.x * ld;
    const int nx = H.nx, ny = H.ny, count = 2 * ny + 2 * (nx - 2);
    bool hit = false;
    for (int r = threadIdx.x; r < count; r += blockDim.x) {
        int a, q;
        if (r < ny) { a = 0; q = r; }
        else if (r < 2 * ny) { a = nx - 1; q = r - ny; }
        else { const int s = r - 2 * ny; a = 1 + (s >> 1); q = (s & 1) ? ny - 1 : 0; }
        if (row[(size_t)a * ny + q] != 0.0) hit = true;
    }
    if (hit) *flag = 1u;
}

// recurrence over the blocks on the full spectrum, one thread per mode: spec[b] holds what_b on entry and c_b on exit (b >= 1);
// D_b = Dtab[dsel[b]] (blocks with the same step sizes share a table)
__global__ void __launch_bounds__(256) h2d_blk_scan_kernel(double *__restrict__ spec, const double *__restrict__ Dtab,
                                                           const int32_t *__restrict__ dsel, int B, size_t per) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= per) return;
    double uh = spec[q];
    for (int b = 1; b < B; b += 8) {
        double d[8], w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int bb = b + j < B ? b + j : B - 1;
            d[j] = Dtab[(size_t)dsel[bb] * per + q];
            w[j] = spec[(size_t)bb * per + q];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (b + j < B) {
                const double c = d[j] * uh;
                spec[(size_t)(b + j) * per + q] = c;
                if (b + j < B - 1) uh = w[j] + c;
            }
        }
    }
}
