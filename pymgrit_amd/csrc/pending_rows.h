// Unstored rows of the Heat1D V-cycle: the four records of rows a pass has left out because their bits sit somewhere else (held, twin,
// lag, up -- DESIGN.md section 4 has the table: producer, rows, where the bits sit, partner, who else settles and in which order,
// waiting rule), every decision about them and the order they are put in place in. Plain host C++, no HIP: the engine
// (mgrit_hip.hip, mgrit_hip_pending.inc) asks, launches, and reports back; tests/host/pending_rows_check.cpp checks this file alone.
// may_leave_out, wherever it appears: one rank, outside a stream capture. A rank with exchange links hands rows to its neighbours and
// would pay a settle per cycle; a graph would bake the decision into cycles it does not hold for. The engine works it out once per call.
#ifndef PYMGRIT_AMD_PENDING_ROWS_H
#define PYMGRIT_AMD_PENDING_ROWS_H
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace pending {
typedef std::vector<int32_t> Ints;
enum Kind { TWIN, UP, LAG, HELD };
// what a caller of settle_steps leaves alone, as the record's partner or because it touches no row of it (KEEP_ALL: list constructors):
// the twin record of the level itself / of the next coarser level, lag, up, the level's held list (HELD_KEEP: the settles that name their records)
enum { TWIN_KEEP_OWN = 1, TWIN_KEEP_BELOW = 2, LAG_KEEP = 4, UP_KEEP = 8, KEEP_ALL = 15, HELD_KEEP = 16 };
enum { TWIN_CFAS = 0, TWIN_FFAS = 1 };   // producer of a twin record: mgrit_hip_cf_fas (interval list) / mgrit_hip_fas_fused_opts (triples list)
struct Step { Kind kind; int level; };
struct Steps { int n = 0; Step s[5]; const Step *begin() const { return s; } const Step *end() const { return s + n; } };

// no value is an element of the ascending list
inline bool names_none_of(const Ints &sorted, const Ints &values) {
    for (int32_t v : values)
        if (std::binary_search(sorted.begin(), sorted.end(), v)) return false;
    return true;
}
inline bool contains_all(const Ints &a, const Ints &b) { return std::includes(a.begin(), a.end(), b.begin(), b.end()); }   // (both ascending)
// the ascending slots are exactly the points a time-parallel solve of n_steps steps writes: 1 .. n_steps, each once
inline bool whole_solve(const Ints &slots, int n_steps) {
    const int n = (int)slots.size();
    return n > 0 && n == n_steps && slots.front() == 1 && slots.back() == n && std::adjacent_find(slots.begin(), slots.end()) == slots.end();
}

struct Ledger {
    struct TwinRec {
        int kind, list;                 // TWIN_CFAS: interval list `list` of the finer level; TWIN_FFAS: its triples list `list`
        const int32_t *d_slots;         // the slots on the device (the finer level's arrays, opaque here) ...
        Ints slots;                     // ... and on the host, ascending
        bool missed = false;            // it had to be settled once: not left out again
        std::map<int, bool> covered;    // TWIN_CFAS: run list id of this level -> its runs' closing points contain every slot
        std::map<int, bool> apart;      // pair list id of the finer level -> none of its coarse points is a slot
    };
    struct Both { Ints slots; const int32_t *d_slots = nullptr, *d_keep = nullptr; };   // d_keep: the list's keep with bit 0 cleared there
    struct Rows {                       // per level
        int held = -1, held_back = 1;   // interval list whose row cend is unstored, and how many rows back its bits sit (0: behind a lag)
        int twin = -1;                  // pending record (index into twin_recs) of THIS level's u, the coarse level of the pair
        std::vector<TwinRec> twin_recs;
        // per interval list: fine rows cend-1 / cend and coarse slots cend_coarse (ascending: what a lag record of the list speaks of), every relaxed C-point a chunk
        // starts from closes an interval of the SAME list (only such a list may lag), the coarse slots whose closing C-point goes to u AND v (keep == 3: twin)
        std::vector<Ints> ivals_rows, ivals_cslots;
        std::vector<char> ivals_lag_ok;
        std::vector<Both> ivals_both;
    };
    std::vector<Rows> L;
    int lag = -1, lag_k = 0;            // level 0: interval list whose corrected closing C-points are unstored, P in row cend-lag_k
    int lag_wait = 2;                   // lag mode 1: partner way ups in a row before a list lags; doubled by every settle of a lag record
    std::map<int, int> lag_streak;      // interval list of level 0 -> consecutive partner way ups with no settle in between
    std::map<std::pair<int, int>, bool> lag_apart;   // (interval list, pair list) of level 0 -> the pairs name none of the record's rows
    int up = -1, up_ivals = -1;         // level 1: run list whose way up was not launched, for the way up of level 0's list up_ivals
    bool up_done = false;               // ... which has run in one pass with it: the lag record is pending with u^1 NOT brought up
    int up_wait = 1, up_skip = 0;       // lag mode 1: ways up of level 1 not deferred behind a miss (a settle with up_done); doubled by each
    int n_levels() const { return (int)L.size(); }
    bool up_pending() const { return n_levels() >= 3 && up >= 0; }
    int up_state() const { return !up_pending() ? 0 : up_done ? 2 : 1; }
    TwinRec &twin_rec(int lvl) { return L[lvl].twin_recs[L[lvl].twin]; }
    // The settle order, written here and nowhere else: twin of the level, of the level below (an entry point of lvl may read u of both), up (levels 0 to 2: it needs u^2,
    // g^1 and the uncorrected u^1 as the deferred pass would have found them), lag behind it (levels 0, 1: it reads u^1), held last. partner: the held list the caller reads
    Steps settle_steps(int lvl, int partner, int keep) const {
        Steps out;
        auto add = [&](Kind k, int l) { out.s[out.n++] = Step{k, l}; };
        if (!(keep & TWIN_KEEP_OWN) && L[lvl].twin >= 0) add(TWIN, lvl);
        if (!(keep & TWIN_KEEP_BELOW) && lvl + 1 < n_levels() && L[lvl + 1].twin >= 0) add(TWIN, lvl + 1);
        if (!(keep & UP_KEEP) && lvl <= 2 && up_pending()) add(UP, 1);
        if (!(keep & LAG_KEEP) && lvl <= 1 && lag >= 0) add(LAG, 0);
        if (!(keep & HELD_KEEP) && L[lvl].held >= 0 && L[lvl].held != partner) add(HELD, lvl);
        return out;
    }
    // the rows are in place. A lag record, and an up record behind the one-pass way up, are misses: the wait doubles, up to 64, never back
    void settled(Step st) {
        Rows &lv = L[st.level];
        if (st.kind == TWIN) { twin_rec(st.level).missed = true; lv.twin = -1; }
        if (st.kind == UP) {
            if (up_done) up_skip = up_wait = std::min(2 * up_wait, 64);
            drop_up();
        }
        if (st.kind == LAG) { lag_streak[lag] = 0; lag_wait = std::min(2 * lag_wait, 64); lag = -1; }
        if (st.kind == HELD) {
            if (st.level == 0) lag_streak[lv.held] = 0;
            lv.held = -1; lv.held_back = 1;
        }
    }
    void drop_up() { up = up_ivals = -1; up_done = false; }
    // new slabs on a level: the records that speak of them are gone, and a lag record behind a one-pass way up with them
    void rebound(int lvl) {
        L[lvl].twin = -1;
        if (lvl <= 1 || (lvl <= 2 && up_pending() && up_done)) lag = -1;
        if (lvl <= 2) drop_up();
    }
    // ---- lag: always (mode 2), or once the list has been the partner of a deferring way down lag_wait times in a row (mode 1: held says it is one now)
    bool lag_due(int list, int store_all_f, int lag_mode, bool held, bool may_leave_out) const {
        if (store_all_f != 2 || !L[0].ivals_lag_ok[list] || !may_leave_out) return false;
        const auto streak = lag_streak.find(list);
        return lag_mode == 2 || (lag_mode == 1 && held && streak != lag_streak.end() && streak->second >= lag_wait);
    }
    // the held list of level 0 if its way up is due to lag and no lag record is pending (what an up record waits for), else -1
    int held_due_to_lag(int lag_mode, bool may_leave_out) const {
        const int list = L[0].held;
        return list >= 0 && lag < 0 && lag_due(list, 2, lag_mode, true, may_leave_out) ? list : -1;
    }
    // the way up of level 0 is about to launch (counted whether or not the launch succeeds) / has run
    void count_way_up(int list, bool held) { int &streak = lag_streak[list]; streak = held ? streak + 1 : 0; }
    void note_way_up(int list, bool held, bool lags, int back) {
        if (held) { L[0].held = -1; L[0].held_back = 1; }
        if (lags) { lag = list; lag_k = 1 - back; }
    }
    // a pair list of level 0 leaves the lag record alone when it names neither a fine row nor a coarse slot of the record (worked out
    // once per record list and pair list); one of level 1 always does: rows of u^1 are read there, none written
    bool lag_keeps_pairs(int pairs_id, const Ints &fine, const Ints &coarse) {
        const auto key = std::make_pair(lag, pairs_id);
        auto seen = lag_apart.find(key);
        if (seen == lag_apart.end())
            seen = lag_apart.emplace(key, names_none_of(L[0].ivals_rows[lag], fine) && names_none_of(L[0].ivals_cslots[lag], coarse)).first;
        return seen->second;
    }
    // ---- up. The waiting rule: behind a miss the next up_wait ways up of level 1 take their turn undeferred (lag mode 1 only)
    bool up_takes_turn(int lag_mode) {
        if (lag_mode != 1 || up_skip == 0) return true;
        --up_skip;
        return false;
    }
    void note_up_deferred(int runs_id) { up = runs_id; up_ivals = L[0].held; up_done = false; }
    void note_up_fused() { up_done = true; }
    bool up_waits_for(int ivals_id) const { return up_pending() && !up_done && up_ivals == ivals_id; }
    // ---- held and the way down (mgrit_hip_cf_fas of level lvl): what it has left out, dropped and read where it was
    void note_way_down(int lvl, int list, bool defer, bool row_ce, bool lag_partner, bool up_drop, int twin) {
        if (defer) { L[lvl].held = list; L[lvl].held_back = row_ce ? 0 : 1; }
        if (lag_partner) lag = -1;
        if (up_drop) drop_up();
        if (twin >= 0) L[lvl + 1].twin = twin;
    }
    // ---- twin, kept on the coarse level lc of a pair: the record of (kind, list), found or made from the slots, or -1 when it may
    // not be left out: it was missed once, or (TWIN_FFAS) is not exactly what the coarsest level's solve of n_steps steps writes
    int twin_offer(int lc, int kind, int list, const Ints &slots, const int32_t *d_slots, int n_steps = 0) {
        std::vector<TwinRec> &recs = L[lc].twin_recs;
        size_t i = 0;
        while (i < recs.size() && (recs[i].kind != kind || recs[i].list != list)) ++i;
        if (i == recs.size()) {
            recs.push_back(TwinRec{kind, list, d_slots, slots, false, {}, {}});
            std::sort(recs[i].slots.begin(), recs[i].slots.end());
        }
        return recs[i].missed || (kind == TWIN_FFAS && !whole_solve(recs[i].slots, n_steps)) ? -1 : (int)i;
    }
    void note_twin(int lc, int twin) { L[lc].twin = twin; }
    void twin_met(int lvl) { L[lvl].twin = -1; }   // the partner has rewritten u of every slot
    // partner of a TWIN_CFAS record: an F-C-relaxation whose runs close on every slot (worked out once per record and run list)
    bool twin_partner_fc(int lvl, int runs_id, int n_runs, const int32_t *start, const int32_t *len) {
        TwinRec &rec = twin_rec(lvl);
        if (rec.kind != TWIN_CFAS) return false;
        const auto seen = rec.covered.find(runs_id);
        if (seen != rec.covered.end()) return seen->second;
        Ints ends(n_runs);
        for (int r = 0; r < n_runs; ++r) ends[r] = start[r] + len[r] - 1;
        std::sort(ends.begin(), ends.end());
        return rec.covered[runs_id] = contains_all(ends, rec.slots);
    }
    // partner of a TWIN_FFAS record: the whole solve of n_steps steps
    bool twin_partner_solve(int lvl, int n_steps) { return twin_rec(lvl).kind == TWIN_FFAS && whole_solve(twin_rec(lvl).slots, n_steps); }
    // a pair list of the finer level none of whose coarse points is a slot of the pending record of lc leaves it pending
    bool twin_keeps_pairs(int lc, int pairs_id, const Ints &coarse) {
        TwinRec &rec = twin_rec(lc);
        auto seen = rec.apart.find(pairs_id);
        if (seen == rec.apart.end()) seen = rec.apart.emplace(pairs_id, names_none_of(rec.slots, coarse)).first;
        return seen->second;
    }
    // ---- a new interval list of level lvl (cf / cc: first interval and coarse start slot per chunk; both: see Rows, slots by both_slots)
    static Ints both_slots(int n, const Ints &kp, const int32_t *cend_coarse, Ints *keep_v) {   // keep_v: kp with bit 0 cleared at the slots
        Ints slots;
        *keep_v = kp;
        for (int i = 0; i < n; ++i)
            if (kp[i] == 3) { slots.push_back(cend_coarse[i]); (*keep_v)[i] = 2; }
        return slots;
    }
    void add_intervals(int lvl, int n, const int32_t *cstart, const int32_t *cend, const int32_t *cend_coarse, const Ints &cf, const Ints &cc,
                       const Both &both) {
        Ints rows, cslots(cend_coarse, cend_coarse + n), ends(cend, cend + n);
        for (int i = 0; i < n; ++i) { rows.push_back(cend[i] - 1); rows.push_back(cend[i]); }
        std::sort(rows.begin(), rows.end());
        std::sort(cslots.begin(), cslots.end());
        std::sort(ends.begin(), ends.end());
        // (as the record's partner the way down reads a chunk's first C-point where the RECORD keeps it: a block's list of a planned
        // cycle starts at another list's closing C-point, a list with gaps likewise -- those never lag)
        bool lag_ok = true;
        for (size_t k = 0; k < cf.size() && lag_ok; ++k) lag_ok = cc[k] < 0 || std::binary_search(ends.begin(), ends.end(), cstart[cf[k]]);
        L[lvl].ivals_rows.push_back(rows);
        L[lvl].ivals_cslots.push_back(cslots);
        L[lvl].ivals_lag_ok.push_back(lag_ok);
        L[lvl].ivals_both.push_back(both);
    }
};

}  // namespace pending
#endif
