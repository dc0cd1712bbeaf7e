// Pairing table of the one-pass way up of levels 1 and 0 (up2_kernel, mgrit_hip.hip): which level-1 point every level-0 interval
// closes on, and how the pass obtains u^1 there without the level-1 way up having stored it. Plain host C++, no HIP.
//
// The level-1 way up (ecf_kernel) walks a run list: run r starts from point start[r] - 1 -- corrected from slot ec_coarse[r] of
// u^2 when ec_coarse[r] >= 0 -- and steps over the F-points start[r] .. start[r] + len[r] - 1. The level-0 way up walks chunks of
// consecutive intervals; interval i closes on level-1 point cend_coarse[i], chunk k starts from level-1 point chunk_start_coarse[k]
// (-1: from a level-0 row). One code per interval and per chunk start:
//   UP2_STEP (-2)  an F-point of a run: one step of level 1 from the value of the point in front of it, which is what the interval
//                  before it in the same chunk closed on or, for a chunk's first interval, the point the chunk starts from
//   j >= 0         the point a run starts from, corrected from slot j of u^2
//   UP2_ROW  (-1)  anything else: the row of u^1 as it stands
#ifndef PYMGRIT_AMD_UP2_TABLE_H
#define PYMGRIT_AMD_UP2_TABLE_H

#include <cstddef>
#include <cstdint>
#include <vector>

namespace up2 {

enum : int32_t { UP2_STEP = -2, UP2_ROW = -1 };

struct Table {
    bool pairs = false;
    std::vector<int32_t> code;         // per interval
    std::vector<int32_t> chunk_slot;   // per chunk: the level-1 point z starts from (chunk_start_coarse, or see below), -1: none
    std::vector<int32_t> chunk_code;   // per chunk: the code of that point, never UP2_STEP
};

// n_pts1: points of level 1 (every index below is checked against it; a list that names a point outside does not pair).
inline Table build_table(int n_pts1, int n_runs, const int32_t *start, const int32_t *len, const int32_t *ec_coarse, int n_ivals,
                         const int32_t *cend_coarse, int n_chunks, const int32_t *chunk_first, const int32_t *chunk_len,
                         const int32_t *chunk_start_coarse) {
    Table tab;
    if (n_pts1 <= 0 || n_runs < 0 || n_ivals < 0 || n_chunks < 0) return tab;
    // role of every level-1 point: 0 nothing, 1 F-point of a run, 2 corrected start of a run (slot in `slot`)
    std::vector<signed char> role((size_t)n_pts1, 0);
    std::vector<int32_t> slot((size_t)n_pts1, -1);
    size_t n_f = 0, n_s = 0;
    for (int r = 0; r < n_runs; ++r) {
        const long long s = start[r], l = len[r];
        if (s < 1 || l < 1 || s + l > n_pts1) return tab;
        for (long long p = s; p < s + l; ++p) {
            if (role[(size_t)p] != 0) return tab;   // a point stepped over twice, or one that another run starts from corrected
            role[(size_t)p] = 1;
            ++n_f;
        }
    }
    for (int r = 0; r < n_runs; ++r) {
        if (ec_coarse[r] < 0) continue;
        const size_t p = (size_t)start[r] - 1;
        if (role[p] != 0) return tab;               // an F-point of another run, or corrected twice
        role[p] = 2;
        slot[p] = ec_coarse[r];
        ++n_s;
    }
    std::vector<char> seen((size_t)n_pts1, 0);      // bit 0: closes an interval, bit 1: starts a chunk
    tab.code.assign((size_t)n_ivals, UP2_ROW);
    tab.chunk_code.assign((size_t)n_chunks, UP2_ROW);
    tab.chunk_slot.assign((size_t)n_chunks, -1);
    const auto fail = [&tab]() { tab.code.clear(); tab.chunk_code.clear(); tab.chunk_slot.clear(); return tab; };
    size_t f_hit = 0, s_hit = 0, covered = 0;
    for (int k = 0; k < n_chunks; ++k) {
        const long long i0 = chunk_first[k], cnt = chunk_len[k];
        if (i0 < 0 || cnt < 1 || i0 + cnt > n_ivals) return fail();
        const int32_t js = chunk_start_coarse[k];
        if (js >= n_pts1) return fail();
        // the level-1 point z starts from: the chunk's first C-point, or -- a chunk that starts from a level-0 row (the first point of
        // the time grid) and whose first interval closes on an F-point of a run -- the point in front of that F-point
        int32_t zs = js;
        if (js < 0) {
            const int32_t j0 = cend_coarse[i0];
            if (j0 >= 1 && j0 < n_pts1 && role[(size_t)j0] == 1) zs = j0 - 1;
        }
        if (zs >= 0) {
            if (role[(size_t)zs] == 1) return fail();   // a chunk starts inside a run
            if (role[(size_t)zs] == 2) {
                tab.chunk_code[(size_t)k] = slot[(size_t)zs];
                if (!(seen[(size_t)zs] & 3)) ++s_hit;
            }
            seen[(size_t)zs] |= 2;
        }
        tab.chunk_slot[(size_t)k] = zs;
        for (long long it = i0; it < i0 + cnt; ++it) {
            const int32_t jc = cend_coarse[it];
            if (jc < 0 || jc >= n_pts1 || (seen[(size_t)jc] & 1)) return fail();
            if (role[(size_t)jc] == 1) {
                if ((it == i0 ? zs : cend_coarse[it - 1]) != jc - 1) return fail();   // z is not the value of the point in front of it
                tab.code[(size_t)it] = UP2_STEP;
                ++f_hit;
            } else if (role[(size_t)jc] == 2) {
                tab.code[(size_t)it] = slot[(size_t)jc];
                if (!(seen[(size_t)jc] & 3)) ++s_hit;
            }
            seen[(size_t)jc] |= 1;
            ++covered;
        }
    }
    // every interval in exactly one chunk, every F-point closes exactly one interval, every corrected start is reached
    tab.pairs = covered == (size_t)n_ivals && f_hit == n_f && s_hit == n_s;
    return tab.pairs ? tab : fail();
}

}  // namespace up2

#endif
