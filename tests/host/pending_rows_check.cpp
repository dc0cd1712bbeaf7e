// Stand-alone check of the ledger of unstored rows (pymgrit_amd/csrc/pending_rows.h). Host C++ only; build it with
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I pymgrit_amd/csrc tests/host/pending_rows_check.cpp
// and run it: the settle order against the order written out by hand, the waiting rules on scripted event sequences, the list
// predicates against brute force on 20000 random lists, and the invariants of the records on random event sequences driven the way
// the engine's entry points drive the ledger. Exit status 0 and "ok" when everything holds.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "pending_rows.h"

namespace {

using namespace pending;

int failures = 0;
void expect(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

std::string text(const Steps &st) {
    std::string out;
    for (const Step &s : st) out += std::string(1, "TULH"[s.kind]) + std::to_string(s.level) + " ";
    return out;
}

// one interval list per level: intervals (4i, 4i + 4], chunks of `chunk`, closing on coarse slot i + 1, every fourth one to u and v
void add_list(Ledger &led, int lvl, int n, int chunk, bool lag_ok = true) {
    Ints cstart, cend, cc_end, kp, cf, cc;
    for (int i = 0; i < n; ++i) {
        cstart.push_back(4 * i); cend.push_back(4 * i + 4); cc_end.push_back(i + 1); kp.push_back(i % 4 == 3 ? 3 : 2);
        if (i % chunk == 0) { cf.push_back(i); cc.push_back(i == 0 ? -1 : i); }
    }
    if (!lag_ok) cstart[chunk] += 1;   // a chunk that starts from a C-point no interval of the list closes on
    Ledger::Both both;
    Ints keep_v;
    both.slots = Ledger::both_slots(n, kp, cc_end.data(), &keep_v);
    for (int i = 0; i < n; ++i) expect(keep_v[i] == 2, "bit 0 cleared where both were set");
    led.add_intervals(lvl, n, cstart.data(), cend.data(), cc_end.data(), cf, cc, both);
}

Ledger fresh(int n_levels) {
    Ledger led;
    led.L.resize(n_levels);
    for (int l = 0; l + 1 < n_levels; ++l) { add_list(led, l, 16, 4); add_list(led, l, 16, 4, false); }
    return led;
}

// ---- the settle order --------------------------------------------------------------------------------------------------------------
void everything_pending(Ledger &led) {
    for (int l = 0; l < led.n_levels(); ++l) {
        led.L[l].held = 0;
        led.L[l].twin = led.twin_offer(l, TWIN_CFAS, 0, Ints{1, 2, 3}, nullptr);
    }
    led.lag = 0;
    led.up = 0; led.up_ivals = 0; led.up_done = true;
}

void check_settle_order() {
    // by hand, everything pending, nothing kept: [levels][lvl]
    const char *by_hand[5][4] = {{}, {}, {"T0 T1 L0 H0 ", "T1 L0 H1 "}, {"T0 T1 U1 L0 H0 ", "T1 T2 U1 L0 H1 ", "T2 U1 H2 "},
                                 {"T0 T1 U1 L0 H0 ", "T1 T2 U1 L0 H1 ", "T2 T3 U1 H2 ", "T3 H3 "}};
    const struct { int bit; char letter; int below; } drops[] = {{TWIN_KEEP_OWN, 'T', 0}, {TWIN_KEEP_BELOW, 'T', 1}, {LAG_KEEP, 'L', 0}, {UP_KEEP, 'U', 0}, {HELD_KEEP, 'H', 0}};
    for (int n = 2; n <= 4; ++n) {
        Ledger led = fresh(n);
        everything_pending(led);
        for (int lvl = 0; lvl < n; ++lvl) {
            expect(text(led.settle_steps(lvl, -1, 0)) == by_hand[n][lvl], "settle order, nothing kept");
            expect(text(led.settle_steps(lvl, 1, 0)) == by_hand[n][lvl], "settle order, another list is the partner");
            for (int keep = 0; keep < 32; ++keep)
                for (int partner = -1; partner <= 0; ++partner) {   // every keep bit takes exactly its own step out, the partner its held list
                    std::string want = by_hand[n][lvl];
                    for (const auto &d : drops) {
                        const std::string step = std::string(1, d.letter) + std::to_string(d.letter == 'T' ? lvl + d.below : d.letter == 'H' ? lvl : d.letter == 'U' ? 1 : 0) + " ";
                        const size_t at = want.find(step);
                        if (((keep & d.bit) || (d.letter == 'H' && partner == 0)) && at != std::string::npos) want.erase(at, step.size());
                    }
                    expect(text(led.settle_steps(lvl, partner, keep)) == want, "settle order with keep bits");
                }
            expect(led.settle_steps(lvl, -1, KEEP_ALL | HELD_KEEP).n == 0, "everything kept");
        }
        // nothing pending, nothing to do; and the full order leaves nothing pending
        for (int lvl = 0; lvl < n; ++lvl)
            for (const Step &s : led.settle_steps(lvl, -1, 0)) led.settled(s);
        for (int lvl = 0; lvl < n; ++lvl) expect(led.settle_steps(lvl, -1, 0).n == 0, "nothing pending behind the full order");
        expect(led.lag < 0 && led.up_state() == 0, "lag and up settled");
    }
}

// ---- the waiting rules ---------------------------------------------------------------------------------------------------------------
// one cycle of level 0 as the engine drives it: the way down defers, the way up is its partner; returns whether the way up lagged
bool cycle(Ledger &led, int lag_mode) {
    const bool lag_partner = led.lag == 0;
    led.note_way_down(0, 0, true, lag_partner && led.lag_k == 0, lag_partner, false, -1);
    const bool held = led.L[0].held == 0, lags = led.lag_due(0, 2, lag_mode, held, true);
    const int back = held ? led.L[0].held_back : 0;
    led.count_way_up(0, held);
    led.note_way_up(0, held, lags, back);
    return lags;
}

void check_waiting_rules() {
    Ledger led = fresh(3);
    int wait = 2;
    for (int round = 0; round < 9; ++round) {   // the wait: 2, 4, 8, 16, 32, 64, 64, 64
        expect(led.lag_wait == wait, "lag_wait");
        for (int k = 0; k < wait; ++k) expect(!cycle(led, 1), "a partner way up inside the wait does not lag");
        expect(cycle(led, 1) && led.lag == 0, "the way up behind the wait lags");
        expect(cycle(led, 1) && cycle(led, 1), "... and keeps lagging");
        expect(led.lag_wait == wait, "a wait never shrinks");
        led.settled(Step{LAG, 0});   // a miss
        expect(led.lag < 0 && led.lag_streak[0] == 0, "a settle of the lag record ends the streak");
        wait = std::min(2 * wait, 64);
    }
    expect(led.lag_wait == 64, "the cap is 64");
    // any settle of the list ends the streak: the held list settled in the middle of the wait
    Ledger l2 = fresh(3);
    cycle(l2, 1); cycle(l2, 1);
    l2.note_way_down(0, 0, true, false, false, false, -1);
    l2.settled(Step{HELD, 0});
    expect(l2.lag_streak[0] == 0 && l2.L[0].held < 0 && l2.L[0].held_back == 1, "a settle of the held list ends the streak");
    expect(!cycle(l2, 1) && !cycle(l2, 1), "the streak starts again");
    expect(cycle(l2, 1), "... and the way up behind the wait lags");
    // mode 2 lags at once, mode 0 never, a list that may not lag never, store_all_f < 2 never, more than one rank / a capture never
    Ledger l3 = fresh(3);
    expect(l3.lag_due(0, 2, 2, false, true) && !l3.lag_due(0, 2, 0, true, true) && !l3.lag_due(1, 2, 2, true, true), "modes, lag_ok");
    expect(!l3.lag_due(0, 1, 2, true, true) && !l3.lag_due(0, 2, 2, true, false), "store_all_f, may_leave_out");
    // the up record: a settle behind the one-pass way up is a miss; one before it is not
    Ledger l4 = fresh(3);
    wait = 1;
    for (int round = 0; round < 9; ++round) {
        l4.L[0].held = 0;
        expect(l4.up_takes_turn(1), "no skip left: deferred");
        l4.note_up_deferred(5);
        expect(l4.up_state() == 1 && l4.up_waits_for(0) && !l4.up_waits_for(1), "noted");
        if (round == 0) {   // settled before the one-pass way up: no miss
            l4.settled(Step{UP, 1});
            expect(l4.up_wait == 1 && l4.up_skip == 0 && l4.up_state() == 0, "no miss");
            l4.note_up_deferred(5);
        }
        l4.note_up_fused();
        expect(l4.up_state() == 2 && !l4.up_waits_for(0), "fused");
        l4.settled(Step{UP, 1});
        wait = std::min(2 * wait, 64);
        expect(l4.up_wait == wait && l4.up_skip == wait && l4.up_state() == 0, "a miss doubles the wait, up to 64");
        expect(l4.up_takes_turn(2) && l4.up_skip == wait, "lag mode 2 does not wait");
        for (int k = wait; k > 0; --k) expect(!l4.up_takes_turn(1) && l4.up_skip == k - 1, "up_skip counts down");
    }
    expect(l4.up_wait == 64, "the cap is 64");
}

// ---- the list predicates against brute force -----------------------------------------------------------------------------------------
void check_predicates(std::mt19937 &rng) {
    for (int it = 0; it < 20000; ++it) {
        const int na = rng() % 12, nb = rng() % 6, range = 1 + rng() % 14;
        Ints a(na), b(nb);
        for (int32_t &x : a) x = rng() % range;
        for (int32_t &x : b) x = rng() % range;
        std::sort(a.begin(), a.end());
        bool none = true;
        for (int32_t x : b)
            for (int32_t y : a) none = none && x != y;
        expect(names_none_of(a, b) == none, "names_none_of");
        // contains_all: as multisets (std::includes), b ascending
        std::sort(b.begin(), b.end());
        bool all = true;
        Ints rest(a);
        for (int32_t x : b) {
            size_t k = 0;
            while (k < rest.size() && rest[k] != x) ++k;
            if (k == rest.size()) { all = false; break; }
            rest.erase(rest.begin() + k);
        }
        expect(contains_all(a, b) == all, "contains_all");
        // whole_solve: exactly 1 .. n_steps, each once
        const int n_steps = rng() % 8;
        Ints s;
        if (rng() % 2) for (int j = 1; j <= n_steps; ++j) s.push_back(j);
        else s = a;
        if (!s.empty() && rng() % 4 == 0) s[rng() % s.size()] += (int)(rng() % 3) - 1;
        std::sort(s.begin(), s.end());
        bool whole = n_steps > 0 && (int)s.size() == n_steps;
        for (int j = 0; whole && j < n_steps; ++j) whole = s[j] == j + 1;
        expect(whole_solve(s, n_steps) == whole, "whole_solve");
    }
}

// ---- invariants on random event sequences ---------------------------------------------------------------------------------------------
// The entry points as mgrit_hip.hip drives the ledger (three levels, lists 0 and 1 of level 0, run list 7 of level 1).
struct Engine {
    Ledger led = fresh(3);
    bool may = true, defer = true;
    int lag_mode = 2, up2_mode = 1, twin_mask = 3;
    int noted_with = -2;   // held_due_to_lag at the time the up record was noted

    void enter(int lvl, int partner = -1, int keep = 0) {
        for (const Step &s : led.settle_steps(lvl, partner, keep)) {
            if (s.kind == LAG) expect(led.up_state() == 0, "the up record is settled in front of the lag record");
            led.settled(s);
        }
    }
    void way_down(int list, bool pre) {
        const bool lag_partner = may && pre && led.lag == list && defer, up_drop = lag_partner && led.up_state() == 2;
        enter(0, -1, lag_partner ? (up_drop ? LAG_KEEP | UP_KEEP : LAG_KEEP) : 0);
        const Ledger::Both &both = led.L[0].ivals_both[list];
        const int twin = (twin_mask & 1) && may && !both.slots.empty() ? led.twin_offer(1, TWIN_CFAS, list, both.slots, nullptr) : -1;
        led.note_way_down(0, list, pre && defer && may, lag_partner && led.lag_k == 0, lag_partner, up_drop, twin);
    }
    void way_up_1() {
        enter(1);
        const bool defers = up2_mode == 1 && defer && may && led.held_due_to_lag(lag_mode, true) >= 0 && led.up_takes_turn(lag_mode);
        if (defers) { noted_with = led.held_due_to_lag(lag_mode, true); constructor_seen = false; led.note_up_deferred(7); }
    }
    void way_up_0(int list, int store_all_f) {
        const bool outside = store_all_f == 2 && may, partner = outside && led.L[0].held == list;   // (may: one rank here, so outside a capture)
        const bool up_partner = partner && led.up_waits_for(list) && led.lag_due(list, 2, lag_mode, true, may);
        enter(0, partner ? list : -1, up_partner ? UP_KEEP : 0);
        const bool held = led.L[0].held == list, lags = led.lag_due(list, store_all_f, lag_mode, held, outside);
        const int back = held ? led.L[0].held_back : 0;
        expect(!up_partner || lags, "the one-pass way up lags");
        led.count_way_up(list, held);
        if (up_partner) led.note_up_fused();
        led.note_way_up(list, held, lags, back);
    }
    void fc_relax_1(bool covering) {   // the partner of a TWIN_CFAS record, or not
        const Ints start{1, 5, 9, 13}, len_all{4, 4, 4, 4}, len_short{3, 3, 3, 3};
        const bool partner = led.L[1].twin >= 0 && may && led.twin_partner_fc(1, covering ? 0 : 1, 4, start.data(), (covering ? len_all : len_short).data());
        enter(1, -1, partner ? TWIN_KEEP_OWN : 0);
        if (partner) led.twin_met(1);
    }
    void copy_pairs_0(bool apart) {
        const Ints coarse = apart ? Ints{0} : Ints{0, 4};
        int keep = led.L[1].twin >= 0 && led.twin_keeps_pairs(1, apart ? 0 : 1, coarse) ? TWIN_KEEP_BELOW : 0;
        if (led.lag >= 0) keep |= LAG_KEEP;
        enter(0, -1, keep);
    }
    void restrict_0(bool apart) {
        const Ints fine = apart ? Ints{0} : Ints{0, 8}, coarse = apart ? Ints{0} : Ints{0, 2};
        enter(0, -1, led.lag >= 0 && led.lag_keeps_pairs(apart ? 0 : 1, fine, coarse) ? LAG_KEEP : 0);
    }
    void invariants(const char *after) {
        // noted for a held list that was due to lag, and that list is still the pending one -- or was put in place by a list constructor
        // of level 0, which keeps the four records but not the held list: the way up of level 0 then finds no partner and settles this one
        if (led.up_state() == 1)
            expect(noted_with >= 0 && led.up_ivals == noted_with && led.lag < 0 && (led.L[0].held == led.up_ivals || (led.L[0].held < 0 && constructor_seen)), after);
        if (led.up_state() == 2) expect(led.lag >= 0, after);
        if (!may_ever) expect(nothing_pending(), after);
    }
    bool nothing_pending() const {
        bool none = led.lag < 0 && led.up_state() == 0;
        for (const Ledger::Rows &lv : led.L) none = none && lv.held < 0 && lv.twin < 0;
        return none;
    }
    bool may_ever = true, constructor_seen = false;
};

void check_invariants(std::mt19937 &rng) {
    for (int run = 0; run < 400; ++run) {
        Engine e;
        e.may_ever = run % 4 != 0;   // every fourth run: more than one rank (or a capture) from start to end
        e.may = e.may_ever;
        e.lag_mode = rng() % 3; e.up2_mode = rng() % 2; e.twin_mask = rng() % 4; e.defer = rng() % 8 != 0;
        for (int ev = 0; ev < 300; ++ev) {
            const int what = rng() % 100, list = rng() % 8 == 0 ? 1 : 0;
            if (what < 25) { e.way_down(list, rng() % 8 != 0); e.invariants("behind a way down"); }
            else if (what < 35) { e.fc_relax_1(rng() % 4 != 0); e.invariants("behind an F-C-relaxation of level 1"); }
            else if (what < 50) { e.way_up_1(); e.invariants("behind a way up of level 1"); }
            else if (what < 75) { e.way_up_0(list, rng() % 8 == 0 ? 1 : 2); e.invariants("behind a way up of level 0"); }
            else if (what < 80) { e.enter(rng() % 3); e.invariants("behind another entry point"); }
            else if (what < 84) { e.constructor_seen = true; e.enter(rng() % 3, -1, KEEP_ALL); e.invariants("behind a list constructor"); }
            else if (what < 88) { e.copy_pairs_0(rng() % 2); e.invariants("behind a pair-list copy"); }
            else if (what < 92) { e.restrict_0(rng() % 2); e.invariants("behind a restriction"); }
            else if (what < 94) { e.led.rebound(rng() % 3); e.invariants("behind new slabs"); }
            else if (what < 96) { e.enter(0, -1, TWIN_KEEP_OWN | TWIN_KEEP_BELOW | HELD_KEEP); e.invariants("behind the lag settle"); }
            else if (what < 98) { e.lag_mode = rng() % 3; e.up2_mode = rng() % 2; e.twin_mask = rng() % 4; }
            else if (e.may_ever) e.may = !e.may;   // a capture begins or ends (inside one every settle is refused: none is pending then)
            if (!e.may && e.may_ever && !e.nothing_pending()) e.may = true;   // (the engine refuses a capture over pending rows: not modelled)
            expect(e.led.lag_wait >= 2 && e.led.lag_wait <= 64 && e.led.up_wait >= 1 && e.led.up_wait <= 64 && e.led.up_skip >= 0 && e.led.up_skip <= e.led.up_wait, "waits in range");
        }
        for (int lvl = 0; lvl < 3; ++lvl) e.enter(lvl);
        expect(e.nothing_pending(), "nothing pending behind the full settle order");
    }
}

}  // namespace

int main() {
    std::mt19937 rng(20260319u);
    check_settle_order();
    check_waiting_rules();
    check_predicates(rng);
    check_invariants(rng);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
