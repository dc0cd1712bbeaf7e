// mgrit_hip_comm.inc -- the ghost exchange under the C ABI (included by mgrit_hip.hip inside extern "C").
//
// Replaces Mgrit.send / Mgrit.receive of the reference (src/pymgrit/core/mgrit.py:693-713: pickled mpi4py isend + blocking
// recv, tag = op base + per-level counter) and its call sites (mgrit.py:306,310,317,331 f_relax ops 0/1; 348,352 c_relax op 2;
// 399,403 residual op 7; 469,484 forward_solve op 5; 504-517 fas_residual ops 3/4): whole slab rows travel between the owners
// of neighbouring time points as STREAM operations of the engine -- ncclSend / ncclRecv of RCCL (xGMI point-to-point on an
// MI355X node) enqueued on the stream the producing / consuming sweep runs on, so an exchange point is ordered against the
// kernels by the stream alone, costs the host one call and can be part of a captured cycle. Messages of one link are
// matched by their ORDER (both owners walk the same exchange points in the same order), not by tags.
//
// A LINK is one direction of one pair of ranks: an RCCL communicator the caller attaches -- made by mgrit_hip_comm_init_rank
// as a two-rank communicator per link (a communicator is then only ever used from one stream at a time, and a send waiting for
// its receiver never holds back a receive from somebody else), or any ncclComm_t the caller already has -- or, for tests and for bench.py --emulate-rank, where all ranks of a run live in ONE
// process on ONE GPU -- a MAILBOX: a block of device memory both ends know, send = row copied into a slot, receive = slot
// copied into the row; who may touch which slot when is the caller's business (host-side hand-shake).
//
// librccl is loaded on first use (dlopen; the copy PyTorch has already mapped is reused: same SONAME), so the library itself
// has no link-time dependency on it and single-rank users never touch it.

namespace {

struct Rccl {
    void *h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
    ncclResult_t (*CommGetAsyncError)(ncclComm_t, ncclResult_t *) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;

int rccl_load() {
    if (g_rccl.h) return 0;
    void *h = nullptr;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *nm : names)
        if ((h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) return fail(MGRIT_HIP_EUNSUPPORTED, "librccl.so.1 not found (%s): no RCCL links", dlerror());
#define RCCL_SYM(field, name)                                                                         \
    if (!(*reinterpret_cast<void **>(&g_rccl.field) = dlsym(h, name))) {                                \
        dlclose(h);                                                                                   \
        return fail(MGRIT_HIP_EUNSUPPORTED, "librccl: symbol %s missing", name);                      \
    }
    RCCL_SYM(GetUniqueId, "ncclGetUniqueId")
    RCCL_SYM(CommInitRank, "ncclCommInitRank")
    RCCL_SYM(CommDestroy, "ncclCommDestroy")
    RCCL_SYM(CommAbort, "ncclCommAbort")
    RCCL_SYM(CommGetAsyncError, "ncclCommGetAsyncError")
    RCCL_SYM(Send, "ncclSend")
    RCCL_SYM(Recv, "ncclRecv")
    RCCL_SYM(GroupStart, "ncclGroupStart")
    RCCL_SYM(GroupEnd, "ncclGroupEnd")
    RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef RCCL_SYM
    g_rccl.h = h;
    return 0;
}

#define RCCL_TRY(expr)                                                                                          \
    do {                                                                                                        \
        ncclResult_t r__ = (expr);                                                                              \
        if (r__ != ncclSuccess) return fail(MGRIT_HIP_EHIP, "%s: %s", #expr, g_rccl.GetErrorString(r__));        \
    } while (0)

int get_link(mgrit_hip_engine *e, int link, Link **out, bool must_be_open = true) {
    if (!e) return fail(MGRIT_HIP_EINVAL, "null engine");
    if (link < 0 || link >= MGRIT_HIP_MAX_LINKS) return fail(MGRIT_HIP_EINVAL, "link %d outside [0,%d)", link, MGRIT_HIP_MAX_LINKS);
    if ((int)e->links.size() < MGRIT_HIP_MAX_LINKS) e->links.resize(MGRIT_HIP_MAX_LINKS);
    Link &l = e->links[link];
    if (must_be_open && l.kind == LINK_NONE) return fail(MGRIT_HIP_EINVAL, "link %d is not open", link);
    if (!must_be_open && l.kind != LINK_NONE) return fail(MGRIT_HIP_EINVAL, "link %d is already open", link);
    *out = &l;
    return 0;
}

__global__ void copy_doubles_kernel(const double *__restrict__ src, double *__restrict__ dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// mailbox copies as kernels of the engine's stream (kernel nodes of a captured cycle, like the ncclSend / ncclRecv kernels they
// stand for). An exchange point's parts -- the row and what travels behind it, out and in -- go as ONE launch, as the grouped
// ncclSend / ncclRecv of an RCCL link is one kernel (round 5: as a launch per part an emulated rank of 8 issued 16 of them per cycle
// where a real one makes 7 RCCL calls): mgrit_hip_exchange opens a batch, the copies queue up, the batch is flushed at its end.
struct CopySegs { const double *src[4]; double *dst[4]; int n[4]; int count; };
__global__ void copy_segments_kernel(CopySegs S) {
    const int k = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S.n[k]) S.dst[k][i] = S.src[k][i];
}
struct MailboxBatch { CopySegs segs{}; bool open = false; };
thread_local MailboxBatch t_mb_batch;      // (an exchange runs start to end on its caller's thread)

int mailbox_flush(mgrit_hip_engine *e) {
    MailboxBatch &b = t_mb_batch;
    b.open = false;
    if (b.segs.count == 0) return 0;
    int most = 0;
    for (int k = 0; k < b.segs.count; ++k) most = std::max(most, b.segs.n[k]);
    hipLaunchKernelGGL(copy_segments_kernel, dim3((unsigned)((most + 255) / 256), (unsigned)b.segs.count), dim3(256), 0, e->stream, b.segs);
    b.segs.count = 0;
    HIP_TRY(hipGetLastError());
    return 0;
}

int mailbox_copy(mgrit_hip_engine *e, double *dst, const double *src, size_t count) {
    MailboxBatch &b = t_mb_batch;
    if (b.open && count <= 0x7fffffffu) {
        // a part that touches what an earlier part of the batch writes needs an order (a rank that sends to itself through one
        // mailbox slot): the batch so far goes first
        bool clash = b.segs.count >= 4;
        for (int k = 0; k < b.segs.count && !clash; ++k)
            clash = (src < b.segs.dst[k] + b.segs.n[k] && b.segs.dst[k] < src + count) || (dst < b.segs.dst[k] + b.segs.n[k] && b.segs.dst[k] < dst + count) ||
                    (dst < b.segs.src[k] + b.segs.n[k] && b.segs.src[k] < dst + count);
        if (clash) {
            int rc = mailbox_flush(e);
            if (rc) return rc;
            b.open = true;
        }
        b.segs.src[b.segs.count] = src; b.segs.dst[b.segs.count] = dst; b.segs.n[b.segs.count] = (int)count;
        ++b.segs.count;
        return 0;
    }
    hipLaunchKernelGGL(copy_doubles_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, e->stream, src, dst, (int)count);
    HIP_TRY(hipGetLastError());
    return 0;
}

// one message = up to two consecutive parts (row | hand-over of the forward solve)
struct Part { double *ptr; size_t count; };

// ncclGroupStart ... ncclGroupEnd around a few calls: whatever way the enclosing function is left, the group is closed (an
// open group would queue every later RCCL call of the thread without ever issuing it)
struct RcclGroup {
    bool open = false;
    int begin() {
        RCCL_TRY(g_rccl.GroupStart());
        open = true;
        return 0;
    }
    int end() {
        if (!open) return 0;
        open = false;
        RCCL_TRY(g_rccl.GroupEnd());
        return 0;
    }
    ~RcclGroup() { if (open) (void)g_rccl.GroupEnd(); }
};

int link_send(mgrit_hip_engine *e, Link &l, int slot, const Part *parts, int n_parts) {
    size_t total = 0;
    for (int k = 0; k < n_parts; ++k) total += parts[k].count;
    if (l.kind == LINK_MAILBOX) {
        Mailbox *mb = l.mb;
        if (slot < 0 || slot >= mb->n_slots) return fail(MGRIT_HIP_EINVAL, "mailbox slot %d outside [0,%d)", slot, mb->n_slots);
        if (total > (size_t)mb->slot_doubles) return fail(MGRIT_HIP_EINVAL, "message of %zu doubles exceeds the mailbox slot (%d)", total, mb->slot_doubles);
        double *dst = mb->slots + (size_t)slot * mb->slot_doubles;
        for (int k = 0; k < n_parts; ++k) {
            int rc = mailbox_copy(e, dst, parts[k].ptr, parts[k].count);
            if (rc) return rc;
            dst += parts[k].count;
        }
    } else {
        RcclGroup grp;
        int rc;
        if (n_parts > 1 && (rc = grp.begin())) return rc;
        for (int k = 0; k < n_parts; ++k) RCCL_TRY(g_rccl.Send(parts[k].ptr, parts[k].count, ncclFloat64, l.peer, l.comm, e->stream));
        if ((rc = grp.end())) return rc;
    }
    l.messages += 1;
    l.bytes += sizeof(double) * total;
    return 0;
}

int link_recv(mgrit_hip_engine *e, Link &l, int slot, const Part *parts, int n_parts) {
    size_t total = 0;
    for (int k = 0; k < n_parts; ++k) total += parts[k].count;
    if (l.kind == LINK_MAILBOX) {
        Mailbox *mb = l.mb;
        if (slot < 0 || slot >= mb->n_slots) return fail(MGRIT_HIP_EINVAL, "mailbox slot %d outside [0,%d)", slot, mb->n_slots);
        if (total > (size_t)mb->slot_doubles) return fail(MGRIT_HIP_EINVAL, "message of %zu doubles exceeds the mailbox slot (%d)", total, mb->slot_doubles);
        const double *src = mb->slots + (size_t)slot * mb->slot_doubles;
        for (int k = 0; k < n_parts; ++k) {
            int rc = mailbox_copy(e, parts[k].ptr, src, parts[k].count);
            if (rc) return rc;
            src += parts[k].count;
        }
    } else {
        RcclGroup grp;
        int rc;
        if (n_parts > 1 && (rc = grp.begin())) return rc;
        for (int k = 0; k < n_parts; ++k) RCCL_TRY(g_rccl.Recv(parts[k].ptr, parts[k].count, ncclFloat64, l.peer, l.comm, e->stream));
        if ((rc = grp.end())) return rc;
    }
    l.messages_in += 1;
    return 0;
}

int ensure_xscratch(mgrit_hip_engine *e, size_t doubles) {
    if (e->xscratch_len >= doubles) return 0;
    if (e->xscratch) e->L[0].allocs.push_back(e->xscratch);   // kept until the engine goes (a captured cycle may hold its address)
    e->xscratch = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->xscratch), sizeof(double) * doubles));
    HIP_TRY(hipMemset(e->xscratch, 0, sizeof(double) * doubles));
    e->xscratch_len = doubles;
    return 0;
}

// Communicators belong to the caller (mgrit_hip_comm_init_rank ... mgrit_hip_comm_destroy); the engine only ABORTS them when a
// bounded wait has given up, so that the kernels waiting for the peer end and the stream drains. An aborted communicator is
// gone: it is remembered here, and a later mgrit_hip_comm_destroy / a second abort of the same pointer does nothing (one
// ncclCommAbort per communicator, whoever asks first).
// The set is keyed by the communicator's address, which the allocator may hand out again: a communicator that mgrit_hip_comm_init_rank
// creates at a remembered address is a NEW one, so the stale entry goes (comm_forget_aborted). Guarded: engines of several host
// threads (loopback ranks) share it.
std::vector<ncclComm_t> g_aborted;
std::mutex g_aborted_mu;
bool comm_abort_once(ncclComm_t comm) {
    {
        std::lock_guard<std::mutex> lock(g_aborted_mu);
        for (ncclComm_t c : g_aborted)
            if (c == comm) return false;
        g_aborted.push_back(comm);
    }
    if (g_rccl.h) (void)g_rccl.CommAbort(comm);
    return true;
}
// true when the pointer was remembered as aborted (the entry is removed)
bool comm_forget_aborted(ncclComm_t comm) {
    std::lock_guard<std::mutex> lock(g_aborted_mu);
    for (size_t k = 0; k < g_aborted.size(); ++k)
        if (g_aborted[k] == comm) {
            g_aborted.erase(g_aborted.begin() + (long)k);
            return true;
        }
    return false;
}

void links_close(mgrit_hip_engine *e, bool abort) {
    for (auto &l : e->links) {
        if (l.kind == LINK_RCCL && l.comm && abort) (void)comm_abort_once(l.comm);
        l = Link();
    }
}

}  // namespace

extern "C" {

int mgrit_hip_comm_unique_id(void *id_out) {
    if (!id_out) return fail(MGRIT_HIP_EINVAL, "null output");
    int rc = rccl_load();
    if (rc) return rc;
    ncclUniqueId id;
    RCCL_TRY(g_rccl.GetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof(id));
    return 0;
}

int mgrit_hip_comm_init_rank(void **comm_out, const void *unique_id, int nranks, int rank) {
    if (!comm_out || !unique_id || nranks < 1 || rank < 0 || rank >= nranks) return fail(MGRIT_HIP_EINVAL, "bad arguments to mgrit_hip_comm_init_rank");
    int rc = rccl_load();
    if (rc) return rc;
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    ncclComm_t comm = nullptr;
    RCCL_TRY(g_rccl.CommInitRank(&comm, nranks, id, rank));
    (void)comm_forget_aborted(comm);   // an aborted communicator once lived at this address: this one is new
    *comm_out = comm;
    return 0;
}

int mgrit_hip_comm_destroy(void *comm, int abort) {
    if (!comm) return 0;
    int rc = rccl_load();
    if (rc) return rc;
    ncclComm_t c = static_cast<ncclComm_t>(comm);
    if (comm_forget_aborted(c)) return 0;   // aborted already (a bounded wait gave up, mgrit_hip_links_close(…, 1)): nothing is left to free
    if (abort) RCCL_TRY(g_rccl.CommAbort(c));
    else RCCL_TRY(g_rccl.CommDestroy(c));
    return 0;
}

int mgrit_hip_link_attach(mgrit_hip_engine *e, int link, void *nccl_comm, int peer) {
    Link *l;
    int rc = get_link(e, link, &l, false);
    if (rc) return rc;
    if (!nccl_comm || peer < 0) return fail(MGRIT_HIP_EINVAL, "bad arguments to mgrit_hip_link_attach");
    if ((rc = rccl_load())) return rc;
    l->kind = LINK_RCCL; l->comm = static_cast<ncclComm_t>(nccl_comm); l->peer = peer;
    return 0;
}

int mgrit_hip_mailbox_create(void **out, int n_slots, int slot_doubles) {
    if (!out || n_slots < 1 || slot_doubles < 1) return fail(MGRIT_HIP_EINVAL, "bad arguments to mgrit_hip_mailbox_create");
    Mailbox *mb = new Mailbox();
    mb->n_slots = n_slots; mb->slot_doubles = slot_doubles;
    const size_t bytes = sizeof(double) * (size_t)n_slots * slot_doubles;
    if (hipMalloc(reinterpret_cast<void **>(&mb->slots), bytes) != hipSuccess || hipMemset(mb->slots, 0, bytes) != hipSuccess) {
        delete mb;
        return fail(MGRIT_HIP_EHIP, "mailbox of %zu bytes: allocation failed", bytes);
    }
    *out = mb;
    return 0;
}

int mgrit_hip_mailbox_destroy(void *mailbox) {
    Mailbox *mb = static_cast<Mailbox *>(mailbox);
    if (!mb) return 0;
    if (mb->slots) (void)hipFree(mb->slots);
    delete mb;
    return 0;
}

int mgrit_hip_link_mailbox(mgrit_hip_engine *e, int link, void *mailbox) {
    Link *l;
    int rc = get_link(e, link, &l, false);
    if (rc) return rc;
    if (!mailbox) return fail(MGRIT_HIP_EINVAL, "null mailbox");
    l->kind = LINK_MAILBOX; l->mb = static_cast<Mailbox *>(mailbox);
    return 0;
}

int mgrit_hip_link_stats(mgrit_hip_engine *e, int link, uint64_t *messages_sent, uint64_t *bytes_sent, uint64_t *messages_received) {
    Link *l;
    int rc = get_link(e, link, &l);
    if (rc) return rc;
    if (messages_sent) *messages_sent = l->messages;
    if (bytes_sent) *bytes_sent = l->bytes;
    if (messages_received) *messages_received = l->messages_in;
    return 0;
}

int mgrit_hip_links_close(mgrit_hip_engine *e, int abort) {
    if (!e) return fail(MGRIT_HIP_EINVAL, "null engine");
    links_close(e, abort != 0);
    return 0;
}

int mgrit_hip_send(mgrit_hip_engine *e, int link, int slot, const double *rows, int count) {
    Link *l;
    int rc = get_link(e, link, &l);
    if (rc) return rc;
    if (!rows || count < 1) return fail(MGRIT_HIP_EINVAL, "bad message");
    Timed timed(e, MGRIT_HIP_T_EXCHANGE, 0);
    const Part p{const_cast<double *>(rows), (size_t)count};
    return link_send(e, *l, slot, &p, 1);
}

int mgrit_hip_recv(mgrit_hip_engine *e, int link, int slot, double *rows, int count) {
    Link *l;
    int rc = get_link(e, link, &l);
    if (rc) return rc;
    if (!rows || count < 1) return fail(MGRIT_HIP_EINVAL, "bad message");
    Timed timed(e, MGRIT_HIP_T_EXCHANGE, 0);
    const Part p{rows, (size_t)count};
    return link_recv(e, *l, slot, &p, 1);
}

int mgrit_hip_exchange(mgrit_hip_engine *e, int lvl, int op, int send_link, int send_idx, int send_slot, int recv_link,
                       int recv_idx, int recv_slot, int handover) {
    int rc = check_level(e, lvl);
    if (rc) return rc;
    if (op < 0 || op > 7 || op == 6) return fail(MGRIT_HIP_EINVAL, "exchange operation %d (the reference's ops are 0-5 and 7; 6 carries no row)", op);
    Level &lv = e->L[lvl];
    if ((rc = check_bound(lv, false))) return rc;
    const int ld = lv.dev.ld, n_pts = lv.dev.n_pts;
    // what travels behind the point in the hand-over of forward_solve (op 5): nothing, the running state of the overlapped chain
    // (DESIGN.md 3.7), or the mode amplitudes of the time-parallel solve (DESIGN.md 3.8)
    const bool with_chain = op == 5 && handover != 0 && lv.blk.r == 0;
    const bool with_modes = op == 5 && handover != 0 && lv.blk.r > 0;
    if (with_chain && handover != ld + CHAIN_STATE_TAIL)
        return fail(MGRIT_HIP_EINVAL, "hand-over of %d doubles, the level's chain state has %d", handover, ld + CHAIN_STATE_TAIL);
    const int mlen = blk_handover_len(lv);
    if (with_modes && handover != mlen)
        return fail(MGRIT_HIP_EINVAL, "hand-over of %d doubles, the level's time-parallel solve hands over %d", handover, mlen);
    // every argument is checked BEFORE the first RCCL call
    Link *ls = nullptr, *lr = nullptr;
    if (send_link >= 0) {
        if ((rc = get_link(e, send_link, &ls))) return rc;
        if (send_idx < 0 || send_idx >= n_pts) return fail(MGRIT_HIP_EINVAL, "send row %d outside the level's %d local points", send_idx, n_pts);
        if (with_modes && !lv.blk.uh_out) return fail(MGRIT_HIP_EINVAL, "level %d: no amplitudes to hand over (mgrit_hip_block_solve_config, has_successor)", lvl);
    }
    if (recv_link >= 0) {
        if ((rc = get_link(e, recv_link, &lr))) return rc;
        if (recv_idx < 0 || recv_idx >= n_pts) return fail(MGRIT_HIP_EINVAL, "receive row %d outside the level's %d local points", recv_idx, n_pts);
        if (with_modes && !lv.blk.uh_in) return fail(MGRIT_HIP_EINVAL, "level %d: nowhere to receive amplitudes (mgrit_hip_block_solve_config, first_real = 0)", lvl);
    }
    const size_t slen = (size_t)ld + CHAIN_STATE_TAIL;
    if (with_chain && !lv.chain_state && (rc = ensure_xscratch(e, 2 * slen))) return rc;   // [fresh state | dropped state]
    Timed timed(e, MGRIT_HIP_T_EXCHANGE, lvl);
    // a send and a receive on ONE communicator (a communicator of the caller shared by both directions; a rank talking to
    // itself) must be able to progress together: one RCCL group
    RcclGroup grp;
    if (ls && lr && ls->kind == LINK_RCCL && lr->kind == LINK_RCCL && ls->comm == lr->comm && (rc = grp.begin())) return rc;
    struct BatchGuard {      // mailbox links: the exchange point's copies as one launch; flushed however the function is left
        mgrit_hip_engine *e;
        explicit BatchGuard(mgrit_hip_engine *e_) : e(e_) { t_mb_batch.open = true; t_mb_batch.segs.count = 0; }
        ~BatchGuard() { if (t_mb_batch.open) (void)mailbox_flush(e); }
    } batch(e);
    if (ls) {
        double *row = lv.dev.u + (size_t)send_idx * ld;
        Part parts[2] = {{row, (size_t)ld}, {nullptr, 0}};
        int n_parts = 1;
        if (with_chain) {
            double *state = lv.chain_state;
            if (!state) {   // this rank has no step of its own on the level (it owns the first point only): a fresh start -- the
                            // carry-free part of the point is the point itself, the carries are zero. Built contiguously, so that
                            // the message has the two parts the receiver posts (RCCL matches sends and receives one to one)
                state = e->xscratch;
                // (a launch of its own, in front of the batch: the message's second part READS what this copy writes)
                hipLaunchKernelGGL(copy_doubles_kernel, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, e->stream, row, state, ld);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemsetAsync(state + ld, 0, sizeof(double) * CHAIN_STATE_TAIL, e->stream));
            }
            parts[1] = {state, slen};
            n_parts = 2;
        } else if (with_modes) {
            parts[1] = {lv.blk.uh_out, (size_t)mlen};
            n_parts = 2;
        }
        if ((rc = link_send(e, *ls, send_slot, parts, n_parts))) return rc;
    }
    if (lr) {
        double *row = lv.dev.u + (size_t)recv_idx * ld;
        Part parts[2] = {{row, (size_t)ld}, {nullptr, 0}};
        int n_parts = 1;
        if (with_chain) {
            // (no chain state bound: nothing here continues the chain, the state is taken off the link and dropped)
            parts[1] = {lv.chain_state ? lv.chain_state : e->xscratch + slen, slen};
            n_parts = 2;
        } else if (with_modes) {
            parts[1] = {const_cast<double *>(lv.blk.uh_in), (size_t)mlen};
            n_parts = 2;
        }
        if ((rc = link_recv(e, *lr, recv_slot, parts, n_parts))) return rc;
        if (with_chain && lv.chain_state) lv.chain_resume = true;   // the next forward solve continues the sender's chain
    }
    if ((rc = mailbox_flush(e))) return rc;
    return grp.end();
}

int mgrit_hip_error_correction_to(mgrit_hip_engine *e, int lvl, int pairs_id, double *rows_out, int ld_out) {
    PairList *pl;
    int rc = get_pairs(e, lvl, pairs_id, &pl);
    if (rc) return rc;
    Level &lf = e->L[lvl], &lc = e->L[lvl + 1];
    if ((rc = caller_transfer(lf, lvl))) return rc;
    if ((rc = check_bound(lf, false)) || (rc = check_bound(lc, true))) return rc;
    if (!rows_out || ld_out < lf.dev.ld) return fail(MGRIT_HIP_EINVAL, "bad output rows");
    if ((lf.h2d && !transfer_2d(lf)) || is_2pts(lf))
        return fail(MGRIT_HIP_EUNSUPPORTED, "error correction into caller rows: 1-D one-point steppers, or 2-D levels joined by a 2-D library transfer");
    if (pl->n == 0) return 0;
    Timed timed(e, MGRIT_HIP_T_ERROR_CORRECTION, lvl);
    if (transfer_2d(lf)) return interp2d_launch(e, lf, lc, pl, 1, rows_out, ld_out);
    dim3 grid(pl->n, (lf.dev.ld + 255) / 256);
    hipLaunchKernelGGL(interp_rows_kernel, grid, dim3(256), 0, e->stream, lf.dev.u, lf.dev.ld, lf.dev.T, pl->d_fine, lc.dev.u,
                       lc.dev.v, lc.dev.ld, lc.dev.T, pl->d_coarse, lf.dev.n, lc.dev.n, lf.transfer, 1, rows_out, ld_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

__global__ void set_ptr_kernel(double **word, double *value) { *word = value; }

int mgrit_hip_cpoint_mirror(mgrit_hip_engine *e, double *rows, int row0) {
    if (!e || row0 < 0) return fail(MGRIT_HIP_EINVAL, "bad arguments");
    if (!e->mirror_cur) {
        if (!rows) return 0;
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->mirror_cur), sizeof(double *)));
        HIP_TRY(hipMemset(e->mirror_cur, 0, sizeof(double *)));
        e->mirror_row0 = row0;
    }
    if (row0 != e->mirror_row0) return fail(MGRIT_HIP_EINVAL, "the mirror's first row is fixed with the first call (%d)", e->mirror_row0);
    hipLaunchKernelGGL(set_ptr_kernel, dim3(1), dim3(1), 0, e->stream, e->mirror_cur, rows);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mgrit_hip_stream_create_masked(void **stream_out, int first_cu, int n_cus) {
    if (!stream_out || first_cu < 0 || n_cus < 1) return fail(MGRIT_HIP_EINVAL, "bad arguments to mgrit_hip_stream_create_masked");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    const int total = prop.multiProcessorCount;
    if (first_cu + n_cus > total) return fail(MGRIT_HIP_EINVAL, "CUs [%d,%d) outside the device's %d", first_cu, first_cu + n_cus, total);
    std::vector<uint32_t> mask((size_t)(total + 31) / 32, 0u);
    for (int c = first_cu; c < first_cu + n_cus; ++c) mask[(size_t)c / 32] |= 1u << (c % 32);
    hipStream_t st = nullptr;
    HIP_TRY(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()));
    *stream_out = st;
    return 0;
}

int mgrit_hip_stream_destroy(void *stream) {
    if (!stream) return 0;
    HIP_TRY(hipStreamDestroy(static_cast<hipStream_t>(stream)));
    return 0;
}

int mgrit_hip_residual_stash(mgrit_hip_engine *e, int n, double *dst) {
    if (!e || n < 0 || (n > 0 && !dst)) return fail(MGRIT_HIP_EINVAL, "bad arguments");
    if ((size_t)n > e->pinned_len) return fail(MGRIT_HIP_EINVAL, "no %d residual values have been produced", n);
    if (n == 0) return 0;
    hipLaunchKernelGGL(copy_doubles_kernel, dim3((n + 255) / 256), dim3(256), 0, e->stream, e->pinned, dst, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mgrit_hip_sync_bounded(mgrit_hip_engine *e, double timeout_s) {
    if (!e) return fail(MGRIT_HIP_EINVAL, "null engine");
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(e->stream);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) return fail(MGRIT_HIP_EHIP, "hipStreamQuery: %s", hipGetErrorString(q));
        if (timeout_s > 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) {
            links_close(e, true);   // ncclCommAbort: the kernels waiting for the peer give up, the stream drains
            return fail(MGRIT_HIP_EHIP, "the engine's stream did not finish within %.1f s (a neighbouring rank never sent or "
                        "never received): links aborted", timeout_s);
        }
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    return chain_status(e);
}

}  // extern "C"
