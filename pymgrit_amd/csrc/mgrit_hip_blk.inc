// mgrit_hip_blk.inc -- time-parallel forward solve of a Heat1D level (DESIGN.md 3.8). Included by mgrit_hip.hip inside its
// anonymous namespace.
//
// Mgrit.forward_solve (src/pymgrit/core/mgrit.py:459-486) steps through the coarsest level one point after the other:
// u_i = g_i + Phi_i(u_{i-1}). One Phi of a 16382-value state is ~1 us of dependent latency however it is spread over the chip
// (chain_kernel / chain2_kernel), so 4096 steps cost 5 ms on 16 of 256 CUs. The steps of a Heat1D level are linear maps that
// share their eigenvectors -- the sine modes q_k -- and over a block of K = 16 steps all but the r lowest modes decay below
// 2^-60 (r = 50 for BASELINE config 3's coarsest level: dt * lambda_max = 5e5). So:
//   blk_local_kernel   the scheme works on the DEFECT of the level's current values u (in a FAS cycle: the injected fine values,
//                      whose error shrinks with the MGRIT iteration): every block propagates its defects from a ZERO error,
//                      x = (g_i + Phi(u_{i-1} + x)) - u_i over the block's steps, no dependence on the blocks before it; W_b = x
//                      goes to a side row. Values that already satisfy u_i = g_i + Phi(u_{i-1}) bit for bit give x = 0: the solve
//                      then changes nothing, so the MGRIT iteration converges to rounding level (re-deriving u from scratch would
//                      differ from the stepped values by eps cond(Phi) in every cycle: a floor of 5e-10 on config 3).
//   blk_project_kernel what_b(k) = <q_k, W_b> for all blocks and modes as a GEMM on the FP64 matrix cores: one wave per (16 blocks,
//                      16 modes, chunk of 1024 row positions), a K loop of v_mfma_f64_16x16x4 over the chunk = one fma chain per
//                      entry in position order; blk_sum_chunks_kernel adds the chunks' sums in order. (Round 4's first version
//                      took the products inside blk_local_kernel, every workgroup streaming all r rows of Q through L2: 45 % of
//                      the solve's time.)
//   blk_scan_kernel    one wave, lane k = mode k: c_b = D_b * Uh, Uh = what_b + c_b over the blocks (D_b(k) = the block's
//                      propagator in mode k, host table); a few hundred dependent multiply-adds
//   blk_correct_kernel u[e_b] += W_b + sum_k q_k c_b(k): the same matrix cores, one wave per (16 blocks, 64 row positions), the
//                      accumulator started from W_b and the K loop over the modes in ascending order (= the fma chain of the spec)
//   blk_finish_kernel  every block is stepped again from its corrected start, interior points stored
// 2 Phi per step instead of 1, all of them independent across blocks: two launches of B workgroups stepping K Phi each.
// The arithmetic is specified by (and bit-identical to) oracle/mgrit_oracle.c heat1d_block_solve_spec; every Phi is the step of 3.3
// with its rank-one correction in closed form (the same bits as the table: heat_solve<CLOSED>).
//
// Advection1D (periodic upwind, advection/advection_1d.py:101-143) takes the same scheme with the Fourier modes in the place of
// the sine modes: a circulant step transports, nothing decays, so ALL n modes (n a power of two, 64 .. 8192) take part -- the
// block ends go through a radix-2 FFT inside one workgroup's LDS (adv_fft_rows_kernel: bit-reversed load, log2 n stages of
// butterflies, one barrier each; the butterflies are the oracle's, so any schedule of them gives the same bits), the recurrence
// runs on n complex amplitudes (adv_scan_kernel), the propagated part comes back through the inverse transform. Only B rows are
// ever transformed (B = steps / 16), every other step is the level's ordinary Phi.
//
// Several ranks (aligned splits: a rank's share is whole blocks): first_real = 0 -- the rank's first block starts from zero
// like the others, because the point in front of it (the ghost, slot 0) arrives later; the scan starts from the mode
// amplitudes Uh of the rank before (uh_in) and leaves its own (uh_out) for the next rank: what crosses a rank boundary on the
// sequential path is r <= 64 doubles and one tiny launch, not a pipeline stage of hundreds of steps.

constexpr int BLK_K = MGRIT_HIP_BLOCK_K;        // steps per block
constexpr int BLK_RMAX = MGRIT_HIP_BLOCK_RMAX;  // modes kept at most
constexpr int BLK_FOURIER_MAX_N = 8192;         // Advection1D: n complex values of a row in one workgroup's LDS (128 KB)

struct BlkDev {
    const double *Q;     // [r][ld] q_k in row storage order, zero at the padding positions
    const double *D;     // [B][BLK_RMAX] block propagators
    double *what, *C;    // [B][BLK_RMAX] inner products / propagated amplitudes
    const double *uh_in; // [BLK_RMAX] amplitudes at the point in front of the first block (first_real = 0)
    double *uh_out;      // [BLK_RMAX] amplitudes at the last point (project_last)
    int r, B, n_steps;   // modes, blocks, steps 1 .. n_steps of the level (local slots)
    int first_real;      // block 0 starts from the point in front of it, which holds its final value (one rank / first rank)
    int project_last;    // the amplitudes of the last block's end are wanted too (a rank with a successor)
    int skip_last_row;   // blk_finish_kernel: the last point has been corrected already (blk_last_kernel, sent to the next rank)
    double *Ws;          // [B][ld] the blocks' propagated defects W_b (row storage order)
    const double *cur;   // the level's current values at the points 1 .. n_steps as blk_correct_kernel and blk_local_kernel<.., TWIN> read
                         // them (set per launch, blk_launch): the level's u, or its v while u of those rows was left unstored (the twin record)
    // Advection1D (periodic; all n Fourier modes, n a power of two): what / C / D / uh_in / uh_out hold complex values
    // [B][n] (re, im interleaved), r = n; tw = the n/2 twiddles (cos, -sin)(2 pi t / n)
    const double2 *tw;
    int fourier, lg_n;
};

__device__ __forceinline__ int blk_first(int b) { return BLK_K * b + 1; }
__device__ __forceinline__ int blk_last(const BlkDev &Bk, int b) { return b == Bk.B - 1 ? Bk.n_steps : BLK_K * (b + 1); }

// TWIN: the level's current values come from Bk.cur (all but the point in front of the first block, which is no row of the record).
// An instance of its own: with the pointer beside L.u in the one kernel every instance spilled two more VGPRs (round 12).
template <int KIND, int FORCE, bool TWIN = false>
__global__ void __launch_bounds__(1024) blk_local_kernel(LevelDev L, BlkDev Bk) {
    constexpr bool HEAT = KIND == MGRIT_HIP_STEPPER_HEAT1D;   // closed-form Phi (the forcing factor may live where the table would)
    WG_PROLOGUE;
    /*BSTAMP_INIT*/
    stage_forcing<FORCE>(sm, L, sl);
    for (int b = blockIdx.x; b < Bk.B; b += gridDim.x) {
        const int first = blk_first(b), last = blk_last(Bk, b);
        double x[E], gi[E];
        load_row(((TWIN && b > 0) ? Bk.cur : L.u) + (size_t)(first - 1) * L.ld, sl, x);   // the first step's input: u_{i-1} itself (zero error)
        /*BSTAMP 4*/
        for (int i = first; i <= last; ++i) {
            load_row(L.g + (size_t)i * L.ld, sl, gi);   // in flight while Phi runs (the step's barrier is LDS-only: it does not wait for it)
            phi_apply<KIND, FORCE, HEAT, 0, HEAT>(x, ctx, L, i, sm, t, lane, wave, G);
            /*BSTAMP 5*/
            double cur[E];
            load_row((TWIN ? Bk.cur : L.u) + (size_t)i * L.ld, sl, cur);  // (after Phi: one live vector less while it runs)
#pragma unroll
            for (int e = 0; e < E; ++e) x[e] = (gi[e] + x[e]) - cur[e];   // the error the block has accumulated at point i
            if (i < last) {
#pragma unroll
                for (int e = 0; e < E; ++e) x[e] = cur[e] + x[e];         // the next step's input u_i + x
            }
            /*BSTAMP 6*/
        }
        store_row(Bk.Ws + (size_t)b * L.ld, sl, x);
    }
    /*BSTAMP 7*/
}

typedef double blk_d4 __attribute__((ext_vector_type(4)));

// phase 2a on the matrix cores: part[c][b][k] = sum over the row positions p of chunk c (1024 of them, ascending) of W_b[p] * Q_k[p].
// v_mfma_f64_16x16x4: operand a = A[i = lane & 15][kk = lane >> 4], b = B[kk][j = lane & 15], accumulator element r of a lane =
// D[i = (lane >> 4) + 4 r][j = lane & 15]; the four kk-products of an instruction are accumulated in order (DESIGN.md 3.5).
// grid (block tiles of 16, mode tiles of 16, chunks); one wave. Rows past B and modes past r: clamped / zero rows of Q, not stored.
__global__ void __launch_bounds__(64) blk_project_kernel(BlkDev Bk, int ld, double *__restrict__ part) {
    const int lane = threadIdx.x, lr = lane & 15, lk = lane >> 4;
    const int b0 = blockIdx.x * 16, k0 = blockIdx.y * 16, c = blockIdx.z;
    const int nb = Bk.B - 1 + (Bk.project_last ? 1 : 0);      // blocks whose amplitudes the recurrence reads
    const int br = b0 + lr < nb ? b0 + lr : nb - 1;
    const double *wa = Bk.Ws + (size_t)br * ld + (size_t)c * GROUP + lk;
    const double *qb = Bk.Q + (size_t)(k0 + lr) * ld + (size_t)c * GROUP + lk;
    blk_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
    for (int t = 0; t < GROUP / 4; ++t) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[4 * t], qb[4 * t], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = b0 + lk + 4 * r, k = k0 + lr;
        if (b < nb && k < Bk.r) part[((size_t)c * Bk.B + b) * BLK_RMAX + k] = acc[r];
    }
}

// what_b(k) = the chunks' sums in chunk order
__global__ void __launch_bounds__(BLK_RMAX) blk_sum_chunks_kernel(BlkDev Bk, int n_chunks, const double *__restrict__ part) {
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= Bk.r) return;
    double tot = 0.0;
    for (int c = 0; c < n_chunks; ++c) tot = tot + part[((size_t)c * Bk.B + b) * BLK_RMAX + k];
    Bk.what[(size_t)b * BLK_RMAX + k] = tot;
}

// phase 2c on the matrix cores: u[e_b][p] += W_b[p] + sum_k c_b(k) Q_k[p], the accumulator started from W_b and the modes in
// ascending order (the spec's fma chain; modes past r carry c = 0 and zero rows of Q: fma(0, 0, x) = x). C rows of blocks nothing
// is propagated into hold zeros. grid (block tiles of 16, tiles of 64 row positions); one wave; blocks b_first .. b_end-1 only.
__global__ void __launch_bounds__(64) blk_correct_kernel(LevelDev L, BlkDev Bk, int b_end) {
    const int lane = threadIdx.x, lr = lane & 15, lk = lane >> 4;
    const int b0 = blockIdx.x * 16, p0 = blockIdx.y * 64, ld = L.ld;
    const int ba = b0 + lr < Bk.B ? b0 + lr : Bk.B - 1;
    blk_d4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + lk + 4 * r;
            acc[j][r] = b < Bk.B ? Bk.Ws[(size_t)b * ld + p0 + 16 * j + lr] : 0.0;
        }
    const int kq = (Bk.r + 3) >> 2;
    for (int t = 0; t < kq; ++t) {
        const double a = Bk.C[(size_t)ba * BLK_RMAX + 4 * t + lk];
        const double *q = Bk.Q + (size_t)(4 * t + lk) * ld + p0 + lr;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, q[16 * j], acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = b0 + lk + 4 * r;
        if (b >= b_end) continue;
        double *row = L.u + (size_t)blk_last(Bk, b) * ld + p0 + lr;
        const double *was = Bk.cur + (size_t)blk_last(Bk, b) * ld + p0 + lr;
#pragma unroll
        for (int j = 0; j < 4; ++j) row[16 * j] = was[16 * j] + acc[j][r];
    }
}

// phase 2b. One workgroup of BLK_RMAX threads.
__global__ void __launch_bounds__(BLK_RMAX) blk_scan_kernel(BlkDev Bk) {
    const int k = threadIdx.x;
    if (k >= Bk.r) return;
    double uh;
    int b0;
    if (Bk.first_real) { uh = Bk.what[k]; b0 = 1; }
    else { uh = Bk.uh_in[k]; b0 = 0; }
    // the table entries of 16 blocks are requested together, one batch AHEAD of the dependent chain that uses them (a batch's
    // loads in flight while the batch before it is worked through: 16 round trips to memory at 256 blocks otherwise)
    const double *__restrict__ Dt = Bk.D;
    const double *__restrict__ Wt = Bk.what;
    double *__restrict__ Ct = Bk.C;
    double d[16], w[16], dn[16], wn[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int bb = b0 + j < Bk.B ? b0 + j : Bk.B - 1;
        d[j] = Dt[(size_t)bb * BLK_RMAX + k];
        w[j] = Wt[(size_t)bb * BLK_RMAX + k];
    }
    for (int b = b0; b < Bk.B; b += 16) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int bb = b + 16 + j < Bk.B ? b + 16 + j : Bk.B - 1;
            dn[j] = Dt[(size_t)bb * BLK_RMAX + k];
            wn[j] = Wt[(size_t)bb * BLK_RMAX + k];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (b + j < Bk.B) {
                const double c = d[j] * uh;
                Ct[(size_t)(b + j) * BLK_RMAX + k] = c;
                if (b + j < Bk.B - 1 || Bk.project_last) uh = w[j] + c;
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) { d[j] = dn[j]; w[j] = wn[j]; }
    }
    if (Bk.uh_out) Bk.uh_out[k] = uh;
}

// phase 2c of the LAST point alone (several ranks: it is what the next rank waits for). One WAVE per (group of 1024 values, pair
// slot q), each a workgroup of its own on a CU of its own: a value is an fma chain over the r rows of Q whatever the launch
// shape, and the loads of Q do not depend on the chain -- eight rows are requested at a time. (As ONE workgroup whose lanes walked
// the r rows one after the other this launch took 99 us at config 3 -- 6.5 MB through one CU, a load round trip per row -- on the
// critical path of every hand-over between ranks.)
__global__ void __launch_bounds__(64) blk_last_kernel(LevelDev L, BlkDev Bk) {
    const int t = blockIdx.y * LANES + threadIdx.x, q = blockIdx.x;
    const size_t slot = slot0(t) + (size_t)q * 64;
    __shared__ double c_lds[BLK_RMAX];
    const int b = Bk.B - 1;
    for (int k = (int)threadIdx.x; k < Bk.r; k += LANES) c_lds[k] = Bk.C[(size_t)b * BLK_RMAX + k];   // (one wave, up to BLK_RMAX modes)
    __syncthreads();
    double2 *row = reinterpret_cast<double2 *>(L.u + (size_t)Bk.n_steps * L.ld) + slot;
    double2 w = reinterpret_cast<const double2 *>(Bk.Ws + (size_t)b * L.ld)[slot];
    if (b >= (Bk.first_real ? 1 : 0)) {
        const double2 *Q = reinterpret_cast<const double2 *>(Bk.Q) + slot;
        const size_t ld2 = (size_t)L.ld / 2;
        for (int k0 = 0; k0 < Bk.r; k0 += 8) {
            double2 qv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) qv[j] = k0 + j < Bk.r ? Q[(size_t)(k0 + j) * ld2] : make_double2(0.0, 0.0);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (k0 + j < Bk.r) {
                    const double ck = c_lds[k0 + j];
                    w.x = fma(qv[j].x, ck, w.x);
                    w.y = fma(qv[j].y, ck, w.y);
                }
        }
    }
    double2 x = *row;
    x.x = x.x + w.x;
    x.y = x.y + w.y;
    *row = x;
}

// phase 3. Item b: the interior of block b is stepped from the point in front of it (the corrected end of block b-1; for block 0 the
// level's first point / the ghost point).
template <int KIND, int FORCE>
__global__ void __launch_bounds__(1024) blk_finish_kernel(LevelDev L, BlkDev Bk) {
    constexpr bool HEAT = KIND == MGRIT_HIP_STEPPER_HEAT1D;   // (the block ends have their correction: blk_correct_kernel / adv_fft_rows_kernel)
    WG_PROLOGUE;
    /*BSTAMP_INIT*/
    stage_forcing<FORCE>(sm, L, sl);
    for (int b = blockIdx.x; b < Bk.B; b += gridDim.x) {
        const int start = b == 0 ? 0 : blk_last(Bk, b - 1);
        double x[E], gi[E];
        load_row(L.u + (size_t)start * L.ld, sl, x);
        const int first = blk_first(b), last = blk_last(Bk, b);
        /*BSTAMP 0*/
        if (first < last) load_row(L.g + (size_t)first * L.ld, sl, gi);
        for (int i = first; i < last; ++i) {
            // (LDS-only barrier inside: the row of g and the row store of the step before stay in flight across the solve)
            phi_apply<KIND, FORCE, HEAT, 0, HEAT>(x, ctx, L, i, sm, t, lane, wave, G);
            /*BSTAMP 1*/
#pragma unroll
            for (int e = 0; e < E; ++e) x[e] = gi[e] + x[e];
            // the NEXT step's row of g is requested in front of this step's store: memory operations retire in order, and behind
            // the store the row would arrive a store's drain later than the solve it has to hide under (a row past the block's
            // interior is requested too -- the same address space, never used -- so that the loop has one shape)
            load_row(L.g + (size_t)(i + 1 < last ? i + 1 : i) * L.ld, sl, gi);
            store_row(L.u + (size_t)i * L.ld, sl, x);
            /*BSTAMP 2*/
        }
    }
    /*BSTAMP 3*/
}

// ---- small Heat1D levels: the whole solve in ONE launch -----------------------------------------------------------------------------
// A level of one group (n <= 1024: a state is one wave) with at most BLK_ONE_MAX_B blocks and BLK_ONE_MAX_R modes on one rank: the six
// launches above are five launch gaps and three kernels of a few microseconds of work each around the two passes (config 2: 257
// points, 16 blocks, r = 13 -- 0.13 ms of which the passes are 0.06). Here workgroup b IS block b through all phases -- W_b and
// the propagated amplitudes c_b never leave its registers / LDS -- and the two points where blocks need each other are device-wide
// barriers (blk_grid_sync; every workgroup is resident: B <= 128 single-wave workgroups on 256 CUs):
//   pass 1 (blk_local_kernel's loop)  ->  what_b(k) = 0.0 + the fma chain of W_b[p] Q_k[p] over the row positions in ascending order
//   (lane k = mode k, the table transposed so that a position's modes are one coalesced read: blk_project_kernel's chain, which the
//   matrix instruction runs in the same order, and blk_sum_chunks_kernel's 0.0 + for the one chunk)  ->  barrier  ->  every
//   workgroup runs blk_scan_kernel's recurrence up to its own block (b dependent multiplies: cheaper than a second barrier)  ->
//   its block end += W_b + sum_k c_b(k) Q_k in ascending k, zero amplitudes up to a multiple of four modes as blk_correct_kernel's
//   K loop has them  ->  barrier  ->  pass 2 (blk_finish_kernel's loop). Same operations in the same order on every value: the bits
//   of the six-launch form (tests/test_hip_block_solve.py compares the two).
// Values another workgroup has written in this launch are read with device-scope atomic loads (not through this CU's vector cache).
constexpr int BLK_ONE_MAX_B = 128, BLK_ONE_MAX_R = 64;

__device__ __forceinline__ double blk_ld_coherent(const double *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// sync[0]: arrivals (target = workgroups x barrier number), sync[1]: workgroups that have left (the last one clears both);
// err: pinned host word, set when a barrier gave up (a workgroup that never became resident) -- checked by the host before the
// next solve. Every wait is bounded: the grid drains whatever happens.
__device__ __forceinline__ bool blk_grid_sync(unsigned *sync, unsigned target, unsigned *err, int *ok_lds, int t) {
    __threadfence();
    __syncthreads();
    if (t == 0) {
        __hip_atomic_fetch_add(sync, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        unsigned spins = 0;
        int ok = 1;
        while (__hip_atomic_load(sync, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > (1u << 24)) { ok = 0; *err = 1u; break; }
        }
        *ok_lds = ok;
    }
    __syncthreads();
    __threadfence();
    return *ok_lds != 0;
}

template <int FORCE>
__global__ void __launch_bounds__(64) blk_one_kernel(LevelDev L, BlkDev Bk, const double2 *__restrict__ Qt, unsigned *sync, unsigned *err) {
    constexpr int KIND = MGRIT_HIP_STEPPER_HEAT1D;
    WG_PROLOGUE_TB(LANES);
    /*BSTAMP_INIT*/
    stage_forcing<FORCE>(sm, L, sl);
    __shared__ __attribute__((aligned(16))) double w_lds[GROUP];
    __shared__ double c_lds[BLK_ONE_MAX_R];
    __shared__ int ok_lds;
    const int b = blockIdx.x, first = blk_first(b), last = blk_last(Bk, b);
    const unsigned n_wg = gridDim.x;
    double x[E];
    // ---- pass 1: the block's defects from a zero error (blk_local_kernel's arithmetic; one wave has registers to spare, so the rows
    // of g and u of the NEXT step are requested in front of every Phi)
    {
        double gi[E], cur[E], gn[E], cn[E];
        load_row(L.u + (size_t)(first - 1) * L.ld, sl, x);
        load_row(L.g + (size_t)first * L.ld, sl, gi);
        load_row(L.u + (size_t)first * L.ld, sl, cur);
        for (int i = first; i <= last; ++i) {
            const int in = i < last ? i + 1 : i;
            load_row(L.g + (size_t)in * L.ld, sl, gn);
            load_row(L.u + (size_t)in * L.ld, sl, cn);
            phi_apply<KIND, FORCE, true, 0, true, true>(x, ctx, L, i, sm, t, lane, wave, G);
#pragma unroll
            for (int e = 0; e < E; ++e) x[e] = (gi[e] + x[e]) - cur[e];
            if (i < last) {
#pragma unroll
                for (int e = 0; e < E; ++e) x[e] = cur[e] + x[e];
            }
#pragma unroll
            for (int e = 0; e < E; ++e) { gi[e] = gn[e]; cur[e] = cn[e]; }
        }
    }
    /*BSTAMP 8*/
    // ---- the block's amplitudes: lane k = mode k, positions in ascending order, two positions per 16-byte read, four batches of 16
    // reads in flight (the chain itself is 1024 dependent multiply-adds: 3.4 us; a read's round trip is a third of that)
#pragma unroll
    for (int q = 0; q < 8; ++q) reinterpret_cast<double2 *>(w_lds)[sl + q * 64] = make_double2(x[2 * q], x[2 * q + 1]);
    __syncthreads();
    const int nb = Bk.B - 1 + (Bk.project_last ? 1 : 0);
    if (b < nb) {
        // four named buffers of eight reads each, three of them in flight while the fourth is consumed (an indexed buffer array made
        // the compiler wait for every read on its own: 30 us for this loop). The chain is bound by the instructions a lone wave can
        // issue, so the reads are vector-typed (one 16-byte load each, not two of 8) off two running pointers whose eight row offsets
        // fit the instruction's immediate field: per chain step one multiply-add, half a load, half an LDS read
        typedef double dv2 __attribute__((ext_vector_type(2)));
        constexpr int NB = GROUP / 2 / 8;   // batches of 8 reads (16 positions)
        double acc = 0.0;
        const dv2 *qlo = reinterpret_cast<const dv2 *>(Qt) + lane;                      // rows 0..3 of a batch at qlo[j * 64] ...
        const dv2 *w2 = reinterpret_cast<const dv2 *>(w_lds);
        dv2 b0[8], b1[8], b2[8], b3[8];
        auto fetch = [&](dv2 (&dst)[8], int bi) {
            const dv2 *q = qlo + (size_t)(bi < NB ? bi : NB - 1) * 8 * BLK_ONE_MAX_R, *qh = q + 4 * BLK_ONE_MAX_R;   // ... rows 4..7 at qh[j * 64]
#pragma unroll
            for (int j = 0; j < 4; ++j) { dst[j] = q[j * BLK_ONE_MAX_R]; dst[4 + j] = qh[j * BLK_ONE_MAX_R]; }
        };
        auto use = [&](const dv2 (&src)[8], int bi) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const dv2 wv = w2[bi * 8 + j];
                acc = fma(wv.x, src[j].x, acc);
                acc = fma(wv.y, src[j].y, acc);
            }
        };
        fetch(b0, 0); fetch(b1, 1); fetch(b2, 2);
        for (int bi = 0; bi < NB; bi += 4) {
            fetch(b3, bi + 3); use(b0, bi);
            fetch(b0, bi + 4); use(b1, bi + 1);
            fetch(b1, bi + 5); use(b2, bi + 2);
            fetch(b2, bi + 6); use(b3, bi + 3);
        }
        if (lane < Bk.r) Bk.what[(size_t)b * BLK_RMAX + lane] = 0.0 + acc;
    }
    /*BSTAMP 9*/
    // (the first four mode rows of the correction are requested in front of the barrier: nothing in them depends on other blocks)
    const int k_end = ((Bk.r + 3) >> 2) << 2;
    const double2 *Q2 = reinterpret_cast<const double2 *>(Bk.Q) + sl;
    const size_t ld2 = (size_t)L.ld / 2;
    double2 qa[4][8], qb[4][8];     // two named buffers of four modes, filled and used in turn (no copies between them)
    auto qfetch = [&](double2 (&dst)[4][8], int k0) {
        const int kk = k0 < k_end ? k0 : k_end - 4;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int q = 0; q < 8; ++q) dst[m][q] = Q2[(size_t)(kk + m) * ld2 + q * 64];
    };
    qfetch(qa, 0);
    if (!blk_grid_sync(sync, n_wg, err, &ok_lds, t)) return;
    /*BSTAMP 10*/
    // ---- the recurrence up to this block (blk_scan_kernel), then the block end (blk_correct_kernel)
    {
        double c = 0.0;
        if (lane < Bk.r) {
            double uh;
            int b0;
            if (Bk.first_real) { uh = b >= 1 ? blk_ld_coherent(Bk.what + lane) : 0.0; b0 = 1; }
            else { uh = Bk.uh_in[lane]; b0 = 0; }
            for (int bb = b0; bb <= b; ++bb) {
                c = Bk.D[(size_t)bb * BLK_RMAX + lane] * uh;
                if (bb < b) uh = blk_ld_coherent(Bk.what + (size_t)bb * BLK_RMAX + lane) + c;
            }
            Bk.C[(size_t)b * BLK_RMAX + lane] = c;
        }
        c_lds[lane] = c;
    }
    __syncthreads();
    double gi[E];
    if (first < last) load_row(L.g + (size_t)first * L.ld, sl, gi);   // pass 2's first row of g: in flight across the second barrier
    if (b < Bk.B - (Bk.project_last ? 1 : 0)) {
        double cur[E];
        load_row(L.u + (size_t)last * L.ld, sl, cur);
        auto quse = [&](const double2 (&src)[4][8], int k0) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const double ck = c_lds[k0 + m];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    x[2 * q] = fma(ck, src[m][q].x, x[2 * q]);
                    x[2 * q + 1] = fma(ck, src[m][q].y, x[2 * q + 1]);
                }
            }
        };
        for (int k0 = 0; k0 < k_end; k0 += 8) {   // four modes at a time, the next four requested first
            qfetch(qb, k0 + 4);
            quse(qa, k0);
            qfetch(qa, k0 + 8);
            if (k0 + 4 < k_end) quse(qb, k0 + 4);
        }
#pragma unroll
        for (int e = 0; e < E; ++e) cur[e] = cur[e] + x[e];
        store_row(L.u + (size_t)last * L.ld, sl, cur);
    }
    /*BSTAMP 11*/
    if (!blk_grid_sync(sync, 2u * n_wg, err, &ok_lds, t)) return;
    /*BSTAMP 12*/
    // ---- pass 2: the block's interior from its corrected start (blk_finish_kernel)
    {
        const int start = b == 0 ? 0 : blk_last(Bk, b - 1);
        const double2 *s2 = reinterpret_cast<const double2 *>(L.u + (size_t)start * L.ld) + sl;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            x[2 * q] = blk_ld_coherent(reinterpret_cast<const double *>(s2 + q * 64));
            x[2 * q + 1] = blk_ld_coherent(reinterpret_cast<const double *>(s2 + q * 64) + 1);
        }
        for (int i = first; i < last; ++i) {
            double gn[E];
            load_row(L.g + (size_t)(i + 1 < last ? i + 1 : i) * L.ld, sl, gn);
            phi_apply<KIND, FORCE, true, 0, true, true>(x, ctx, L, i, sm, t, lane, wave, G);
#pragma unroll
            for (int e = 0; e < E; ++e) x[e] = gi[e] + x[e];
            store_row(L.u + (size_t)i * L.ld, sl, x);
#pragma unroll
            for (int e = 0; e < E; ++e) gi[e] = gn[e];
        }
    }
    /*BSTAMP 13*/
    if (t == 0 && __hip_atomic_fetch_add(sync + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == n_wg - 1) {
        __hip_atomic_store(sync, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(sync + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Qt[p / 2][k] = (Q[k][p], Q[k][p + 1]) for the first BLK_ONE_MAX_R modes (zero past q_rows): the layout blk_one_kernel's projection
// reads, a position pair of one mode per lane
__global__ void blk_transpose_modes_kernel(const double *__restrict__ Q, int ld, int q_rows, double2 *__restrict__ Qt) {
    const int pp = blockIdx.x, k = threadIdx.x;
    Qt[(size_t)pp * BLK_ONE_MAX_R + k] = k < q_rows ? make_double2(Q[(size_t)k * ld + 2 * pp], Q[(size_t)k * ld + 2 * pp + 1]) : make_double2(0.0, 0.0);
}

// ---- Advection1D: Fourier modes ----------------------------------------------------------------------------------------------------
// One workgroup per block: mode 0 = what_b = FFT(W_b); mode 1 = u[e_b] += W_b + Re(IFFT(c_b)) / n. Blocks b0 .. b0 + gridDim.x - 1.
// LDS: n complex values. The butterflies and their operand order are orc_fft_spec's.
__global__ void __launch_bounds__(1024) adv_fft_rows_kernel(LevelDev L, BlkDev Bk, int b0, int inverse) {
    extern __shared__ __attribute__((aligned(16))) char fft_raw[];
    double2 *x = reinterpret_cast<double2 *>(fft_raw);
    const int n = L.n, lg = Bk.lg_n, tid = threadIdx.x, nth = blockDim.x;
    const int b = b0 + blockIdx.x;
    double *row = L.u + (size_t)blk_last(Bk, b) * L.ld;
    const double *ws = Bk.Ws + (size_t)b * L.ld;
    if (inverse && b < (Bk.first_real ? 1 : 0)) {   // nothing was propagated into the first block: u[e_0] += W_0
        for (int j = tid; j < n; j += nth) {
            const int p = row_pos(j);
            row[p] = row[p] + ws[p];
        }
        return;
    }
    double2 *spec = reinterpret_cast<double2 *>(inverse ? Bk.C : Bk.what) + (size_t)b * n;
    for (int j = tid; j < n; j += nth) {
        const int r = (int)(__brev((unsigned)j) >> (32 - lg));
        x[r] = inverse ? spec[j] : make_double2(ws[row_pos(j)], 0.0);
    }
    __syncthreads();
    for (int s = 1; s <= lg; ++s) {
        const int half = 1 << (s - 1), stride = n >> s;
        for (int q = tid; q < (n >> 1); q += nth) {
            const int j = q & (half - 1), ia = ((q >> (s - 1)) << s) + j, ib = ia + half;
            double2 w = Bk.tw[j * stride];
            if (inverse) w.y = -w.y;
            const double2 a = x[ia], c = x[ib];
            const double tr = fma(-w.y, c.y, w.x * c.x), ti = fma(w.y, c.x, w.x * c.y);
            x[ia] = make_double2(a.x + tr, a.y + ti);
            x[ib] = make_double2(a.x - tr, a.y - ti);
        }
        __syncthreads();
    }
    if (inverse) {   // u[e_b] += W_b + Re(IFFT(c_b)) / n
        const double inv_n = 1.0 / (double)n;
        for (int j = tid; j < n; j += nth) {
            const int p = row_pos(j);
            row[p] = row[p] + (ws[p] + x[j].x * inv_n);
        }
    } else {
        for (int k = tid; k < n; k += nth) spec[k] = x[k];
    }
}


// ---- Advection1D, n NOT a power of two: the two transforms as plain sums over the table of all n roots of unity (oracle: orc_dft_*) ----
// T[m] = (cos, -sin)(2 pi m / n), m < n (Bk.tw). Every sum is one fma chain in ascending index order from 0.0 -- a K loop of
// v_mfma_f64_16x16x4 (the instruction adds its four products in order onto the accumulator) -- so the transforms are ordered GEMMs
// on the matrix cores: O(n^2) per row, but only B rows are ever transformed, and the table index (j k) mod n advances by a
// constant per K step (one add, one conditional subtract). One wave per tile of 16 blocks x 16 modes (positions), DFT_WAVES tiles
// per workgroup around one copy of the table in LDS (16 KB .. 128 KB).
constexpr int DFT_UNROLL = 8, DFT_WAVES = 4;
// forward: what_b(k) = (sum_j W_b[j] T[(j k) mod n].re, sum_j W_b[j] T[(j k) mod n].im); grid (block tiles, groups of DFT_WAVES mode tiles);
// the two sums of a mode share the operand W_b[j] and one 16-byte read of the table: two accumulators, two MFMA per K step. The
// table sits in LDS (n double2, staged once per workgroup of DFT_WAVES waves: gathered from L2 every K step touched 64 cache lines)
__global__ void __launch_bounds__(64 * DFT_WAVES) adv_dft_fwd_kernel(LevelDev L, BlkDev Bk, int b_first, int b_count) {
    extern __shared__ __attribute__((aligned(16))) char dft_raw[];
    double2 *tw = reinterpret_cast<double2 *>(dft_raw);
    const int n = L.n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) tw[i] = Bk.tw[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
    const int b0 = b_first + blockIdx.x * 16, k0 = (blockIdx.y * DFT_WAVES + wave) * 16;
    if (k0 >= n) return;
    const int b_end = b_first + b_count;
    const int ba = b0 + lr < b_end ? b0 + lr : b_end - 1;          // operand a: block ba, position j = 4 t + lk
    const int kb = k0 + lr < n ? k0 + lr : n - 1;                  // operand b: mode kb
    const double *ws = Bk.Ws + (size_t)ba * L.ld;
    int m = (int)(((long)lk * kb) % n);                            // (j k) mod n at j = lk
    const int inc = (int)((4L * kb) % n);
    blk_d4 acc_re = {0.0, 0.0, 0.0, 0.0}, acc_im = {0.0, 0.0, 0.0, 0.0};
    const int steps = (n + 3) >> 2;
    for (int t0 = 0; t0 < steps; t0 += DFT_UNROLL) {
        double a[DFT_UNROLL];
        double2 w[DFT_UNROLL];
#pragma unroll
        for (int u = 0; u < DFT_UNROLL; ++u) {     // (DFT_UNROLL K steps' operands requested together)
            const int j = 4 * (t0 + u) + lk;
            a[u] = (t0 + u < steps && j < n) ? ws[row_pos(j)] : 0.0;
            w[u] = tw[m];
            m += inc; if (m >= n) m -= n;
        }
#pragma unroll
        for (int u = 0; u < DFT_UNROLL; ++u)
            if (t0 + u < steps) {
                acc_re = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], w[u].x, acc_re, 0, 0, 0);
                acc_im = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], w[u].y, acc_im, 0, 0, 0);
            }
    }
    double2 *out = reinterpret_cast<double2 *>(Bk.what);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = b0 + lk + 4 * r, k = k0 + lr;
        if (b < b_end && k < n) out[(size_t)b * n + k] = make_double2(acc_re[r], acc_im[r]);
    }
}

// inverse: u[e_b][j] += W_b[j] + (sum_k c_b(k).re T[(j k) mod n].re, then c_b(k).im T[(j k) mod n].im) / n; a block nothing was
// propagated into (b < first_real): u[e_b] += W_b. grid (block tiles, groups of DFT_WAVES position tiles); the K loop runs over the
// 2 n reals of c_b.
__global__ void __launch_bounds__(64 * DFT_WAVES) adv_dft_inv_kernel(LevelDev L, BlkDev Bk, int b_first, int b_count) {
    extern __shared__ __attribute__((aligned(16))) char dft_raw[];
    const double *tw = reinterpret_cast<const double *>(dft_raw);
    const int n = L.n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) reinterpret_cast<double2 *>(dft_raw)[i] = Bk.tw[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
    const int b0 = b_first + blockIdx.x * 16, j0 = (blockIdx.y * DFT_WAVES + wave) * 16;
    if (j0 >= n) return;
    const int b_end = b_first + b_count;
    const int ba = b0 + lr < b_end ? b0 + lr : b_end - 1;          // operand a: block ba, real index 4 t + lk of c_b
    const int jb = j0 + lr < n ? j0 + lr : n - 1;                  // operand b: position jb
    const double *cs = Bk.C + (size_t)ba * n * 2;
    const double *tab = tw + (lk & 1);                             // lk even: c.re with T.re, lk odd: c.im with T.im
    int m = (int)(((long)(lk >> 1) * jb) % n);                     // (j k) mod n at k = lk >> 1
    const int inc = (int)((2L * jb) % n);                          // a K step advances k by 2
    blk_d4 acc = {0.0, 0.0, 0.0, 0.0};
    const int steps = (2 * n + 3) >> 2;
    for (int t0 = 0; t0 < steps; t0 += DFT_UNROLL) {
        double a[DFT_UNROLL], w[DFT_UNROLL];
#pragma unroll
        for (int u = 0; u < DFT_UNROLL; ++u) {
            const int kk = 4 * (t0 + u) + lk;
            a[u] = (t0 + u < steps && kk < 2 * n) ? cs[kk] : 0.0;
            w[u] = tab[2 * (size_t)m];
            m += inc; if (m >= n) m -= n;
        }
#pragma unroll
        for (int u = 0; u < DFT_UNROLL; ++u)
            if (t0 + u < steps) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], w[u], acc, 0, 0, 0);
    }
    const double inv_n = 1.0 / (double)n;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = b0 + lk + 4 * r, j = j0 + lr;
        if (b >= b_end || j >= n) continue;
        const int p = row_pos(j);
        double *row = L.u + (size_t)blk_last(Bk, b) * L.ld;
        const double wsv = Bk.Ws[(size_t)b * L.ld + p];
        row[p] = b < (Bk.first_real ? 1 : 0) ? row[p] + wsv : row[p] + (wsv + acc[r] * inv_n);
    }
}

// recurrence over the blocks on n complex amplitudes: one thread per mode
__global__ void __launch_bounds__(256) adv_scan_kernel(BlkDev Bk, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double2 *__restrict__ Dt = reinterpret_cast<const double2 *>(Bk.D);
    const double2 *__restrict__ Wt = reinterpret_cast<const double2 *>(Bk.what);
    double2 *__restrict__ Ct = reinterpret_cast<double2 *>(Bk.C);
    double2 uh;
    int b0;
    if (Bk.first_real) { uh = Wt[k]; b0 = 1; }
    else { uh = reinterpret_cast<const double2 *>(Bk.uh_in)[k]; b0 = 0; }
    for (int b = b0; b < Bk.B; b += 8) {
        double2 d[8], w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int bb = b + j < Bk.B ? b + j : Bk.B - 1;
            d[j] = Dt[(size_t)bb * n + k];
            w[j] = Wt[(size_t)bb * n + k];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (b + j < Bk.B) {
                double2 c;
                c.x = fma(-d[j].y, uh.y, d[j].x * uh.x);
                c.y = fma(d[j].y, uh.x, d[j].x * uh.y);
                Ct[(size_t)(b + j) * n + k] = c;
                if (b + j < Bk.B - 1 || Bk.project_last) { uh.x = w[j].x + c.x; uh.y = w[j].y + c.y; }
            }
        }
    }
    if (Bk.uh_out) reinterpret_cast<double2 *>(Bk.uh_out)[k] = uh;
}
