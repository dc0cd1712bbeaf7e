// mgrit_hip_gen.inc -- whole-level passes for ANY register-resident 1-D stepper and ANY of the library's spatial transfers
// (copy, full weighting / linear interpolation with Dirichlet ends, its periodic analogue). Included by mgrit_hip.hip inside its
// anonymous namespace.
//
// cfas_kernel / ecfr_kernel (mgrit_hip.hip) fuse the sweeps of a level for Heat1D pairs joined by the identity transfer: there the
// coarse Phi runs inside the fine level's kernel and v^{l+1} is the fine C-point bit for bit. With a spatial transfer
// (examples/example_spatial_coarsening.py:33-82; BASELINE config 5) or another stepper (Advection1D) neither holds, and a level's
// way down ran as seven launches (C-relaxation, F-relaxation, restriction of u, clone into v, fine half of the FAS right-hand
// side, its restriction, coarse half), its way up as three (correction, F-relaxation, residual). Here:
//   gen_down_kernel   Mgrit.c_relax, then Mgrit.f_relax, then the FINE half of Mgrit.fas_residual (mgrit.py:335-370, 292-333,
//                     524-532 / 538-543 in the order of Mgrit.iteration, mgrit.py:277-281) in one pass per interval; the F-points are
//                     not stored (the way up rewrites them before anything reads them); the restriction of the C-point and of the
//                     defect row r_i = Phi(u_{i-1}) - u_i [+ g_i] is taken from the registers (a lane's neighbours' end values by
//                     shuffle, a wave's by LDS): u^{l+1} = v^{l+1} = R(u_i) and g^{l+1} = R(r_i) + v^{l+1} are stored. Followed by the
//                     coarse half (fas_coarse_kernel, have_sum): two launches, and no row is written to be read back.
//   gen_up_kernel     Mgrit.error_correction (mgrit.py:715-726) with the interpolation evaluated from the two coarse rows in
//                     registers, then Mgrit.f_relax, then on level 0 Mgrit.compute_residual (mgrit.py:387-413): one launch.
// A workgroup walks a chunk of consecutive intervals with the closing C-point in registers. The way up corrects the C-point an
// interval ENDS on; the corrected value of the C-point a chunk STARTS from belongs to the chunk before it (another workgroup,
// which may or may not have written it yet): the way down leaves the uncorrected value of every chunk's last C-point in a side
// slab (Cb), the way up takes it from there and applies the same correction -- the same bits, no race.
// Arithmetic: exactly that of the separate sweeps (relax_kernel, fas_fine_kernel, interp_rows_kernel, residual_kernel).

// the interpolated correction P(u^{l+1}_j - v^{l+1}_j) added to the 16 values of thread t (interp_rows_kernel's expressions).
// Every thread of the workgroup calls it (shuffles inside). A lane's 16 fine values take 8 coarse ones -- half of a coarse lane's
// 16, four 16-byte slots of the coarse row -- and one more from a neighbour lane (shuffle; a wave's edge lane and the periodic
// wrap read theirs from the row).
__device__ __forceinline__ void gen_correct(double (&x)[E], const LevelDev &L, const LevelDev &Lc, int j, int t, int tkind) {
    const double *uc = Lc.u + (size_t)j * Lc.ld, *vc = Lc.v + (size_t)j * Lc.ld;
    if (tkind == MGRIT_HIP_TRANSFER_COPY) {
        const double2 *u2 = reinterpret_cast<const double2 *>(uc) + slot0(t), *v2 = reinterpret_cast<const double2 *>(vc) + slot0(t);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const double2 a = u2[q * 64], b = v2[q * 64];
            x[2 * q] = x[2 * q] + (a.x - b.x);
            x[2 * q + 1] = x[2 * q + 1] + (a.y - b.y);
        }
        return;
    }
    const int n_f = L.n, n_c = Lc.n, j0 = t * E, lane = t & 63, tc = t >> 1;
    auto at = [&](int c) { const int p = row_pos(c); return uc[p] - vc[p]; };
    double own[8];   // coarse entries 8t .. 8t+7 (zero past the end of the coarse vector)
    if (tc < Lc.T) {
        const unsigned s = slot0(tc) + (unsigned)((t & 1) * 4) * 64;
        const double2 *u2 = reinterpret_cast<const double2 *>(uc) + s, *v2 = reinterpret_cast<const double2 *>(vc) + s;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double2 a = u2[q * 64], b = v2[q * 64];
            own[2 * q] = 8 * t + 2 * q < n_c ? a.x - b.x : 0.0;
            own[2 * q + 1] = 8 * t + 2 * q + 1 < n_c ? a.y - b.y : 0.0;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) own[k] = 0.0;
    }
    if (tkind == MGRIT_HIP_TRANSFER_PERIODIC1D) {
        // fine 2i -> e_i ; fine 2i+1 -> (e_i + e_{(i+1) mod n_c}) / 2 : coarse entries 8t .. 8t+8
        double nxt = __shfl_down(own[0], 1);                 // coarse 8t+8 = the next lane's first
        const int c8 = 8 * t + 8;
        if (c8 >= n_c) nxt = c8 - n_c < n_c && j0 < n_f ? at(c8 - n_c) : 0.0;      // the periodic wrap
        else if (lane == 63) nxt = at(c8);                                        // the next wave's
        if (8 * t < n_c && n_c < c8) {
            // the last coarse entry sits in the middle of this lane's eight (n_c not a multiple of 8): its right neighbour is
            // entry 0, which takes the (masked, otherwise unused) place behind it
            const double e0 = at(0);
#pragma unroll
            for (int m = 1; m < 8; ++m) own[m] = 8 * t + m == n_c ? e0 : own[m];
        }
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const double hi = (k >> 1) + 1 < 8 ? own[(k >> 1) + 1 < 8 ? (k >> 1) + 1 : 0] : nxt;
            const double val = (k & 1) ? (0.0 + 1.0 / 2.0 * own[k >> 1]) + 1.0 / 2.0 * hi : 0.0 + own[k >> 1];
            if (j0 + k < n_f) x[k] = x[k] + val;
        }
        return;
    }
    // MGRIT_HIP_TRANSFER_HEAT1D (n_f = 2 n_c + 1): odd fine j -> e_{(j-1)/2}; even j = 2i -> e_{i-1}/2 + e_i/2 (ends: one term)
    double prv = __shfl_up(own[7], 1);                       // coarse 8t-1 = the lane before's last
    if (lane == 0) prv = (t > 0 && 8 * t - 1 < n_c && j0 < n_f) ? at(8 * t - 1) : 0.0;   // the wave before's; nothing in front of entry 0
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int jf = j0 + k, i = jf >> 1;
        double val;
        if (k & 1) val = 0.0 + own[k >> 1];
        else {
            val = 0.0;
            if (i - 1 >= 0) val = val + 1.0 / 2.0 * (k == 0 ? prv : own[k == 0 ? 0 : (k >> 1) - 1]);
            if (i < n_c) val = val + 1.0 / 2.0 * own[k >> 1];
        }
        if (jf < n_f) x[k] = x[k] + val;
    }
}

constexpr int GEN_HAL = MAX_G + 2;

// R(u_i) and R(r_i) from the registers (fb: the C-point, fr: the defect row) into u^{l+1}_j, v^{l+1}_j and g^{l+1}_j = R(r_i) + v^{l+1}_j
// (restrict_rows_kernel's expressions). Every thread of the workgroup calls it (one barrier inside); hal: 2 * GEN_HAL doubles of
// LDS that nobody else touches until the workgroup's next barrier but one.
__device__ __forceinline__ void gen_restrict_store(const double (&fb)[E], const double (&fr)[E], const LevelDev &L, const LevelDev &Lc,
                                                   int j, int t, int lane, int wave, unsigned sl, int tkind, double *hal) {
    double *uc = Lc.u + (size_t)j * Lc.ld, *vc = Lc.v + (size_t)j * Lc.ld, *gc = Lc.g + (size_t)j * Lc.ld;
    if (tkind == MGRIT_HIP_TRANSFER_COPY) {
        double a[E];
#pragma unroll
        for (int e = 0; e < E; ++e) a[e] = fr[e] + fb[e];
        store_row(uc, sl, fb);
        store_row(vc, sl, fb);
        store_row(gc, sl, a);
        return;
    }
    const int n_c = Lc.n, n_f = L.n;
    double cb[8], cr[8];
    if (tkind == MGRIT_HIP_TRANSFER_PERIODIC1D) {   // coarse i = 8t + k: fine 2i-1 (mod n_f), 2i, 2i+1
        double hb = __shfl_up(fb[E - 1], 1), hr = __shfl_up(fr[E - 1], 1);
        if (lane == 63) { hal[wave] = fb[E - 1]; hal[GEN_HAL + wave] = fr[E - 1]; }
        if (t == ((n_f - 1) >> 4)) {   // the owner of the last fine value: the left neighbour of fine value 0
            const int el = (n_f - 1) & 15;
            double wb = fb[0], wr = fr[0];
#pragma unroll
            for (int e = 1; e < E; ++e) {
                wb = e == el ? fb[e] : wb;
                wr = e == el ? fr[e] : wr;
            }
            hal[MAX_G] = wb; hal[GEN_HAL + MAX_G] = wr;
        }
        __syncthreads();
        if (lane == 0) { const int src = t == 0 ? MAX_G : wave - 1; hb = hal[src]; hr = hal[GEN_HAL + src]; }
        cb[0] = hb * 1.0 / 4.0 + fb[0] * 1.0 / 2.0 + fb[1] * 1.0 / 4.0;
        cr[0] = hr * 1.0 / 4.0 + fr[0] * 1.0 / 2.0 + fr[1] * 1.0 / 4.0;
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            cb[k] = fb[2 * k - 1] * 1.0 / 4.0 + fb[2 * k] * 1.0 / 2.0 + fb[2 * k + 1] * 1.0 / 4.0;
            cr[k] = fr[2 * k - 1] * 1.0 / 4.0 + fr[2 * k] * 1.0 / 2.0 + fr[2 * k + 1] * 1.0 / 4.0;
        }
    } else {   // MGRIT_HIP_TRANSFER_HEAT1D, n_f = 2 n_c + 1: fine 2i, 2i+1, 2i+2
        double hb = __shfl_down(fb[0], 1), hr = __shfl_down(fr[0], 1);
        if (lane == 0) { hal[wave] = fb[0]; hal[GEN_HAL + wave] = fr[0]; }
        __syncthreads();
        if (lane == 63) { hb = hal[wave + 1]; hr = hal[GEN_HAL + wave + 1]; }   // (past the last wave: a value no coarse entry uses)
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            cb[k] = fb[2 * k] * 1.0 / 4.0 + fb[2 * k + 1] * 1.0 / 2.0 + fb[2 * k + 2] * 1.0 / 4.0;
            cr[k] = fr[2 * k] * 1.0 / 4.0 + fr[2 * k + 1] * 1.0 / 2.0 + fr[2 * k + 2] * 1.0 / 4.0;
        }
        cb[7] = fb[14] * 1.0 / 4.0 + fb[15] * 1.0 / 2.0 + hb * 1.0 / 4.0;
        cr[7] = fr[14] * 1.0 / 4.0 + fr[15] * 1.0 / 2.0 + hr * 1.0 / 4.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (8 * t + k >= n_c) { cb[k] = 0.0; cr[k] = 0.0; }
        cr[k] = cr[k] + cb[k];      // g + v
    }
    const int tc = t >> 1;          // the coarse row's thread that holds coarse values 16 tc .. 16 tc + 15: this thread owns half of them
    if (tc < Lc.T) {
        const unsigned s = slot0(tc) + (unsigned)((t & 1) * 4) * 64;
        double2 *u2 = reinterpret_cast<double2 *>(uc) + s, *v2 = reinterpret_cast<double2 *>(vc) + s, *g2 = reinterpret_cast<double2 *>(gc) + s;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u2[q * 64] = make_double2(cb[2 * q], cb[2 * q + 1]);
            v2[q * 64] = make_double2(cb[2 * q], cb[2 * q + 1]);
            g2[q * 64] = make_double2(cr[2 * q], cr[2 * q + 1]);
        }
    }
}

// TB: the workgroup size an instance is compiled for. States of up to 8192 values run in workgroups of at most 512 threads, and
// compiled for 1024 these passes keep to 128 VGPRs by spilling 16-81 of them -- scratch traffic in kernels that are bound by memory
// bandwidth. The TB = 512 instances (149-182 VGPRs, no VGPR spill) take the launches of such levels (instance_tb): config 5
// 5.4 -> 4.9 ms per F-cycle. Same source, same operations, same bits as the 1024-thread instances.
template <int KIND, int FORCE, bool USE_G, int TB = 1024>
__global__ void __launch_bounds__(TB) gen_down_kernel(LevelDev L, LevelDev Lc, IntervalsDev I, double *__restrict__ Cb, int tkind) {
    WG_PROLOGUE;
    __shared__ double gen_hal[2][2 * GEN_HAL];
    for (wq.begin(L.sched, L.xcc0_limit, wgq_slot, t); wq.cur < I.n_chunks; wq.advance(t)) {
        const int k = wq.cur;
        wq.prefetch(t);
        const int i0 = I.chunk_first[k], cnt = I.chunk_len[k];
        double x[E];
        {
            const int cs = I.cstart[i0];
            if (I.chunk_start_coarse[k] >= 0) {   // the C-relaxed value of the chunk's first C-point, recomputed from its old F-point
                load_row(L.u + (size_t)(cs - 1) * L.ld, sl, x);
                phi_apply<KIND, FORCE>(x, ctx, L, cs, sm, t, lane, wave, G);
                if (USE_G) {
                    double gi[E];
                    load_row(L.g + (size_t)cs * L.ld, sl, gi);
#pragma unroll
                    for (int e = 0; e < E; ++e) x[e] = gi[e] + x[e];
                }
            } else {
                load_row(L.u + (size_t)cs * L.ld, sl, x);
            }
        }
        for (int it = i0; it < i0 + cnt; ++it) {
            const int cs = I.cstart[it], ce = I.cend[it];
            for (int i = cs + 1; i < ce; ++i) {   // F-relaxation from the relaxed C-point; not stored
                double gi[E];
                if (USE_G) load_row(L.g + (size_t)i * L.ld, sl, gi);
                phi_apply<KIND, FORCE>(x, ctx, L, i, sm, t, lane, wave, G);
                if (USE_G) {
#pragma unroll
                    for (int e = 0; e < E; ++e) x[e] = gi[e] + x[e];
                }
            }
            double b[E], gc[E];
            if (USE_G) load_row(L.g + (size_t)ce * L.ld, sl, gc);
            load_row(L.u + (size_t)(ce - 1) * L.ld, sl, b);   // C-relaxation: from the OLD last F-point (F rows are not written here)
            phi_apply<KIND, FORCE>(b, ctx, L, ce, sm, t, lane, wave, G);
            if (USE_G) {
#pragma unroll
                for (int e = 0; e < E; ++e) b[e] = gc[e] + b[e];
            }
            store_row(L.u + (size_t)ce * L.ld, sl, b);
            if (it == i0 + cnt - 1) store_row(Cb + (size_t)I.res_pos[it] * L.ld, sl, b);   // the next chunk's way up starts from it
            phi_apply<KIND, FORCE>(x, ctx, L, ce, sm, t, lane, wave, G);                    // Phi(new last F-point)
            if (USE_G) {
#pragma unroll
                for (int e = 0; e < E; ++e) x[e] = (gc[e] - b[e]) + x[e];          // (g_i - u_i) + Phi(u_{i-1})
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) x[e] = x[e] - b[e];                    // Phi(u_{i-1}) - u_i
            }
            gen_restrict_store(b, x, L, Lc, I.cend_coarse[it], t, lane, wave, sl, tkind, gen_hal[it & 1]);
#pragma unroll
            for (int e = 0; e < E; ++e) x[e] = b[e];
        }
    }
    wq.end(t);
}

template <int KIND, int FORCE, bool USE_G, bool RES, int TB = 1024>
__global__ void __launch_bounds__(TB) gen_up_kernel(LevelDev L, LevelDev Lc, IntervalsDev I, const double *__restrict__ Cb,
                                                      double *__restrict__ out, int tkind) {
    WG_PROLOGUE;
    for (wq.begin(L.sched, L.xcc0_limit, wgq_slot, t); wq.cur < I.n_chunks; wq.advance(t)) {
        const int k = wq.cur;
        wq.prefetch(t);
        const int i0 = I.chunk_first[k], cnt = I.chunk_len[k];
        double x[E];
        {
            const int cs = I.cstart[i0], js = I.chunk_start_coarse[k];
            if (js >= 0) {   // the corrected first C-point: the value the way down left in the side slab + the same correction
                load_row(Cb + (size_t)(I.res_pos[i0] - 1) * L.ld, sl, x);
                gen_correct(x, L, Lc, js, t, tkind);
            } else {
                load_row(L.u + (size_t)cs * L.ld, sl, x);
            }
        }
        for (int it = i0; it < i0 + cnt; ++it) {
            const int cs = I.cstart[it], ce = I.cend[it], jc = I.cend_coarse[it];
            for (int i = cs + 1; i < ce; ++i) {
                double gi[E];
                if (USE_G) load_row(L.g + (size_t)i * L.ld, sl, gi);
                phi_apply<KIND, FORCE>(x, ctx, L, i, sm, t, lane, wave, G);
                if (USE_G) {
#pragma unroll
                    for (int e = 0; e < E; ++e) x[e] = gi[e] + x[e];
                }
                store_row(L.u + (size_t)i * L.ld, sl, x);
            }
            double b[E];
            load_row(L.u + (size_t)ce * L.ld, sl, b);
            gen_correct(b, L, Lc, jc, t, tkind);
            store_row(L.u + (size_t)ce * L.ld, sl, b);
            if (RES) {
                phi_apply<KIND, FORCE>(x, ctx, L, ce, sm, t, lane, wave, G);
#pragma unroll
                for (int e = 0; e < E; ++e) x[e] = x[e] - b[e];
                const double tot = block_sumsq(x, sm, L.n, t, lane, wave, G);
                if (t == 0) out[I.res_pos[it]] = tot;
            }
#pragma unroll
            for (int e = 0; e < E; ++e) x[e] = b[e];
        }
    }
    wq.end(t);
}
