// Unstored rows (pending_rows.h, DESIGN.md section 4): the device side of putting them in place, and the gate in front of every entry
// point. Included by mgrit_hip.hip. Everything the ledger decides it decides there; this file launches and reports back.
// held: the rows a deferring mgrit_hip_cf_fas has left out are put in place -- row cend-1 copied to row cend for every
// interval of the list -- and the record is cleared. Never launched into a stream capture: a captured copy would be replayed
// in cycles that have nothing pending.
// back = held_back: 1 = the bits sit in row cend-1 (copied to row cend); 0 = behind a lagged way up they sit in row cend itself,
// and row cend-1 receives them, so that both rows hold what they hold behind every other settle.
__global__ void __launch_bounds__(256) settle_held_kernel(double *__restrict__ u, int ld, const int32_t *__restrict__ cend, int n, int back) {
    for (int it = blockIdx.x; it < n; it += gridDim.x) {
        const int ce = cend[it];   // 2 <= ce < n_pts (mgrit_hip_intervals_create)
        const double2 *src = reinterpret_cast<const double2 *>(u + (size_t)(ce - back) * ld);
        double2 *dst = reinterpret_cast<double2 *>(u + (size_t)(ce - 1 + back) * ld);
        for (int k = threadIdx.x; k < ld / 2; k += blockDim.x) dst[k] = src[k];
    }
}

// lag: the rows a lagging mgrit_hip_ec_relax_res has left out are put in place and the record is cleared. With A the uncorrected
// closing C-point and P = Phi(F''_last) in rows cend-1 / cend (k = 1: A in row cend, P in row cend-1; k = 0: the other way round), row
// cend := A + (uc - A) with uc = row cend_coarse of u^{l+1} -- ecfr_kernel's expression on ecfr_kernel's operands, element by element,
// pad columns included -- and row cend-1 := P: bit for bit what a pass that does not lag leaves. Every lane reads its operands before
// it writes, so the rows are rewritten in place. Never launched into a stream capture, as settle_held_kernel.
__global__ void __launch_bounds__(256) settle_lag_kernel(double *__restrict__ u, const double *__restrict__ uc, int ld, int ldc,
                                                         const int32_t *__restrict__ cend, const int32_t *__restrict__ cend_coarse, int n,
                                                         int k_lag) {
    for (int it = blockIdx.x; it < n; it += gridDim.x) {
        const int ce = cend[it], jc = cend_coarse[it];   // 2 <= ce < n_pts, 0 <= jc < n_pts of the coarse level (mgrit_hip_intervals_create)
        double2 *r1 = reinterpret_cast<double2 *>(u + (size_t)ce * ld);
        double2 *r0 = reinterpret_cast<double2 *>(u + (size_t)(ce - 1) * ld);
        const double2 *rc = reinterpret_cast<const double2 *>(uc + (size_t)jc * ldc);
        for (int k = threadIdx.x; k < ld / 2; k += blockDim.x) {
            const double2 a = k_lag ? r1[k] : r0[k], w = rc[k];
            if (!k_lag) r0[k] = r1[k];
            r1[k] = make_double2(a.x + (w.x - a.x), a.y + (w.y - a.y));
        }
    }
}

// twin: row v of every slot of the pending record copied to row u, the record cleared and marked (it is not deferred again).
// Never launched into a stream capture, as settle_held_kernel.
__global__ void __launch_bounds__(256) settle_twin_kernel(double *__restrict__ u, const double *__restrict__ v, int ld,
                                                          const int32_t *__restrict__ slots, int n) {
    for (int it = blockIdx.x; it < n; it += gridDim.x) {
        const int j = slots[it];   // 0 <= j < n_pts (mgrit_hip_intervals_create / mgrit_hip_pairs_create)
        const double2 *src = reinterpret_cast<const double2 *>(v + (size_t)j * ld);
        double2 *dst = reinterpret_cast<double2 *>(u + (size_t)j * ld);
        for (int k = threadIdx.x; k < ld / 2; k += blockDim.x) dst[k] = src[k];
    }
}

bool capturing(const mgrit_hip_engine *e) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(e->stream, &cs);
    return cs != hipStreamCaptureStatusNone;
}
bool has_links(const mgrit_hip_engine *e) {
    return std::any_of(e->links.begin(), e->links.end(), [](const Link &l) { return l.kind != LINK_NONE; });
}
// one rank, outside a capture: what every decision to leave rows out asks first, once per call (pending_rows.h)
bool may_leave_out(const mgrit_hip_engine *e) { return !has_links(e) && !capturing(e); }
using pending::TWIN_KEEP_OWN; using pending::TWIN_KEEP_BELOW; using pending::LAG_KEEP; using pending::UP_KEEP; using pending::KEEP_ALL;
enum { ONLY_UP = (KEEP_ALL & ~UP_KEEP) | pending::HELD_KEEP, ONLY_UP_AND_LAG = ONLY_UP & ~LAG_KEEP };   // the settles that name their records

int ec_relax_launch(mgrit_hip_engine *e, int lvl, const RunList &rl);   // (behind the launch helpers it needs)

// One step of the settle order. up: the deferred ecf_kernel pass is launched exactly as mgrit_hip_ec_relax would have launched it --
// u^2, g^1 and the uncorrected rows of u^1 are as that call found them, every entry point that could change one comes through here
// first --, so level 1 holds bit for bit what the two passes leave; the lag record behind it stays pending and finds its row of u^1.
int settle(mgrit_hip_engine *e, pending::Step st) {
    pending::Ledger &rows = e->rows;
    Level &lv = e->L[st.level];
    const dim3 block(256);
    const bool cap = capturing(e);
    int rc = 0;
    switch (st.kind) {
    case pending::TWIN: {
        if (cap) return fail(MGRIT_HIP_EINVAL, "level %d has unstored rows of u pending (record %d) inside a stream capture", st.level, rows.L[st.level].twin);
        const pending::Ledger::TwinRec &rec = rows.twin_rec(st.level);
        const int n = (int)rec.slots.size();
        rc = launch(&settle_twin_kernel, dim3(std::min(n, 4096)), block, 0, e->stream, lv.dev.u, (const double *)lv.dev.v, lv.dev.ld, rec.d_slots, n);
        break;
    }
    case pending::UP:
        if (cap) return fail(MGRIT_HIP_EINVAL, "level 1 has its way up pending (run list %d) inside a stream capture", rows.up);
        rc = ec_relax_launch(e, 1, lv.runs[rows.up]);
        break;
    case pending::LAG: {
        if (cap) return fail(MGRIT_HIP_EINVAL, "level 0 has unstored corrected C-points pending (interval list %d) inside a stream capture", rows.lag);
        const Level &lc = e->L[1];
        const int n = lv.ivals_cnt[rows.lag];
        const IntervalsDev &I = lv.ivals[rows.lag];
        rc = launch(&settle_lag_kernel, dim3(std::min(n, 4096)), block, 0, e->stream, lv.dev.u, (const double *)lc.dev.u, lv.dev.ld, lc.dev.ld, I.cend,
                    I.cend_coarse, n, rows.lag_k);
        break;
    }
    case pending::HELD: {
        const int held = rows.L[st.level].held;
        if (cap) return fail(MGRIT_HIP_EINVAL, "level %d has unstored C-points pending (interval list %d) inside a stream capture", st.level, held);
        const int n = lv.ivals_cnt[held];
        rc = launch(&settle_held_kernel, dim3(std::min(n, 4096)), block, 0, e->stream, lv.dev.u, lv.dev.ld, lv.ivals[held].cend, n, rows.L[st.level].held_back);
        break;
    }
    }
    if (!rc) rows.settled(st);
    return rc;
}

// whatever of the settle order is pending for a caller of level lvl (pending::Ledger::settle_steps has the order and the arguments)
int settle_pending(mgrit_hip_engine *e, int lvl, int partner, int keep) {
    for (const pending::Step &st : e->rows.settle_steps(lvl, partner, keep))
        if (const int rc = settle(e, st)) return rc;
    return 0;
}

int check_level(mgrit_hip_engine *e, int lvl, bool need_set = true, int partner = -1, int keep = 0) {
    if (!e) return fail(MGRIT_HIP_EINVAL, "null engine");
    if (lvl < 0 || lvl >= e->n_levels) return fail(MGRIT_HIP_EINVAL, "level %d out of range [0,%d)", lvl, e->n_levels);
    if (need_set && !e->L[lvl].set) return fail(MGRIT_HIP_EINVAL, "level %d has no stepper", lvl);
    return settle_pending(e, lvl, partner, keep);
}
