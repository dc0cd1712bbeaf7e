// Stand-alone check of the pairing table of the one-pass way up (pymgrit_amd/csrc/up2_table.h). Host C++ only; build it with
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I pymgrit_amd/csrc tests/host/up2_table_check.cpp
// and run it: the shapes of tests/test_hip_up2.py, lists that must not pair, and random lists (any answer, no bad access; a table
// that pairs is replayed against a model of the two passes). Exit status 0 and "ok" when everything holds.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "up2_table.h"

namespace {

typedef std::vector<int32_t> Vec;

struct Lists {
    int n_pts1 = 0;
    Vec start, len, ec;                                      // the level-1 run list
    Vec cend_coarse, chunk_first, chunk_len, chunk_start;    // the level-0 interval list
};

up2::Table build(const Lists &l) {
    return up2::build_table(l.n_pts1, (int)l.start.size(), l.start.data(), l.len.data(), l.ec.data(), (int)l.cend_coarse.size(),
                            l.cend_coarse.data(), (int)l.chunk_first.size(), l.chunk_first.data(), l.chunk_len.data(), l.chunk_start.data());
}

int failures = 0;
void expect(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

// a regular hierarchy: nt0 points on level 0, coarsening m0 to level 1 and m1 to level 2, level-0 chunks cut where the interval's
// index is a multiple of `chunk` (mgrit_hip_intervals_create), the first point of the grid not corrected
Lists regular(int nt0, int m0, int m1, int chunk) {
    Lists l;
    l.n_pts1 = (nt0 - 1) / m0 + 1;
    for (int c = 0; c < l.n_pts1 - 1; c += m1) {
        const int n = std::min(m1 - 1, l.n_pts1 - 1 - c);
        if (n < 1) break;
        l.start.push_back(c + 1);
        l.len.push_back(n);
        l.ec.push_back(c == 0 ? -1 : c / m1);
    }
    const int n_iv = l.n_pts1 - 1;
    for (int i = 0; i < n_iv; ++i) {
        l.cend_coarse.push_back(i + 1);
        if (i % chunk == 0) {
            l.chunk_first.push_back(i);
            l.chunk_len.push_back(std::min(chunk, n_iv - i));
            l.chunk_start.push_back(i == 0 ? -1 : i);
        }
    }
    return l;
}

// what the two passes compute, as symbols: value id of u^1 at every point after the level-1 way up, against what the table makes z
// at every interval's closing point. An id is (kind << 40 | a << 20 | b): row as it stands, corrected row, or a step from an id's index.
bool replay(const Lists &l, const up2::Table &t) {
    const int n = l.n_pts1;
    std::vector<long long> two(n);
    for (int p = 0; p < n; ++p) two[p] = p;                              // the row as it stands
    for (size_t r = 0; r < l.start.size(); ++r)
        if (l.ec[r] >= 0) two[l.start[r] - 1] = (1LL << 40) | ((long long)(l.start[r] - 1) << 20) | l.ec[r];
    std::vector<std::pair<long long, int>> steps;                        // steps get ids of their own: index into `steps`
    for (size_t r = 0; r < l.start.size(); ++r) {
        long long x = two[l.start[r] - 1];
        for (int p = l.start[r]; p < l.start[r] + l.len[r]; ++p) {
            steps.push_back(std::make_pair(x, p));
            x = two[p] = (2LL << 40) | (long long)(steps.size() - 1);
        }
    }
    auto same = [&](long long a, long long b) {   // structural equality of two value ids
        while ((a >> 40) == 2 && (b >> 40) == 2) {
            const auto &sa = steps[(size_t)(a & 0xffffffffffLL)], &sb = steps[(size_t)(b & 0xffffffffffLL)];
            if (sa.second != sb.second) return false;
            a = sa.first; b = sb.first;
        }
        return a == b;
    };
    for (size_t k = 0; k < l.chunk_first.size(); ++k) {
        long long z = -1;
        const int zs = t.chunk_slot[k];
        if (zs >= 0) {
            z = t.chunk_code[k] >= 0 ? ((1LL << 40) | ((long long)zs << 20) | t.chunk_code[k]) : (long long)zs;
            if (!same(z, two[zs])) return false;
        }
        if (l.chunk_start[k] >= 0 && zs != l.chunk_start[k]) return false;
        for (int it = l.chunk_first[k]; it < l.chunk_first[k] + l.chunk_len[k]; ++it) {
            const int jc = l.cend_coarse[it], cd = t.code[it];
            if (cd == up2::UP2_STEP) {
                if (z < 0) return false;
                steps.push_back(std::make_pair(z, jc));
                z = (2LL << 40) | (long long)(steps.size() - 1);
            } else
                z = cd >= 0 ? ((1LL << 40) | ((long long)jc << 20) | cd) : (long long)jc;
            if (!same(z, two[jc])) return false;
        }
    }
    return true;
}

}  // namespace

int main() {
    // the shapes of the GPU tests: nt = 1025 and 257, m = 4, chunks of 4 and 16 pair; chunks of 3 and m = (4, 3) do not
    for (int nt : {1025, 257})
        for (int chunk : {4, 16, 8}) {
            const Lists l = regular(nt, 4, 4, chunk);
            const up2::Table t = build(l);
            expect(t.pairs, "regular hierarchy pairs");
            if (t.pairs) {
                expect(replay(l, t), "regular hierarchy: the table reproduces the two passes");
                expect(t.code[0] == up2::UP2_STEP && t.chunk_slot[0] == 0 && t.chunk_code[0] == up2::UP2_ROW, "first chunk starts z from point 0");
                expect(t.code.back() == up2::UP2_ROW, "the last C-point of level 1 is taken as it stands");
            }
        }
    expect(!build(regular(1025, 4, 4, 3)).pairs, "chunks of 3 do not pair");
    for (int chunk : {1, 2, 6}) expect(!build(regular(1025, 4, 4, chunk)).pairs, "chunks that are no multiple of the level-1 coarsening do not pair");
    {   // m = (4, 3) with chunks of 4: a chunk starts inside a run
        const Lists l = regular(1021, 4, 3, 4);
        expect(!build(l).pairs, "m = (4, 3), chunks of 4 do not pair");
        const up2::Table t = build(regular(1021, 4, 3, 3));
        expect(t.pairs, "m = (4, 3), chunks of 3 pair");
    }
    {   // a C-point followed by a C-point on level 1: run list with a gap, the second C-point corrected by hand (code -1)
        Lists l = regular(65, 4, 4, 4);
        l.start.erase(l.start.begin() + 1); l.len.erase(l.len.begin() + 1); l.ec.erase(l.ec.begin() + 1);
        const up2::Table t = build(l);
        expect(t.pairs && replay(l, t), "a run list with a gap pairs");
        if (t.pairs) expect(t.code[4] == up2::UP2_ROW && t.code[5] == up2::UP2_ROW, "points outside every run are rows as they stand");
    }
    {   // broken lists
        Lists l = regular(65, 4, 4, 4);
        l.cend_coarse[5] = l.cend_coarse[4];
        expect(!build(l).pairs, "a point that closes two intervals does not pair");
        l = regular(65, 4, 4, 4);
        l.cend_coarse.pop_back(); l.chunk_len.back() -= 1;
        expect(build(l).pairs, "a list that stops short of the last C-point still pairs");
        l = regular(65, 4, 4, 4);
        l.cend_coarse.resize(8); l.chunk_first.resize(2); l.chunk_len.resize(2); l.chunk_start.resize(2);
        expect(!build(l).pairs, "F-points that close no interval do not pair");
        l = regular(65, 4, 4, 4);
        l.start[2] = 100;
        expect(!build(l).pairs, "a run outside level 1 does not pair");
        l = regular(65, 4, 4, 4);
        l.chunk_first[1] = 1000;
        expect(!build(l).pairs, "a chunk outside the list does not pair");
        l = regular(65, 4, 4, 4);
        l.cend_coarse[3] = 99;
        expect(!build(l).pairs, "an interval that closes outside level 1 does not pair");
        Lists empty;
        expect(!build(empty).pairs, "empty lists do not pair");
    }
    // random lists: any answer, no bad access; whatever pairs must replay
    std::mt19937 rng(20261020u);
    int paired = 0;
    for (int trial = 0; trial < 20000; ++trial) {
        Lists l;
        const bool wild = trial % 4 == 0;
        if (!wild) {   // a regular list with a few random defects
            const int m1 = 2 + (int)(rng() % 4), chunk = 1 + (int)(rng() % 9);
            l = regular(1 + 4 * (int)(2 + rng() % 60), 4, m1, chunk);
            const int defects = (int)(rng() % 3);
            for (int d = 0; d < defects && !l.cend_coarse.empty(); ++d)
                switch (rng() % 5) {
                case 0: l.cend_coarse[rng() % l.cend_coarse.size()] += (int)(rng() % 3) - 1; break;
                case 1: if (!l.ec.empty()) l.ec[rng() % l.ec.size()] = (int)(rng() % 40) - 2; break;
                case 2: if (!l.len.empty()) l.len[rng() % l.len.size()] += (int)(rng() % 3) - 1; break;
                case 3: l.chunk_start[rng() % l.chunk_start.size()] += (int)(rng() % 3) - 1; break;
                default: if (l.start.size() > 1) { const size_t r = rng() % l.start.size(); l.start.erase(l.start.begin() + r); l.len.erase(l.len.begin() + r); l.ec.erase(l.ec.begin() + r); }
                }
            for (int32_t &v : l.ec) if (v < -1) v = -1;
            for (int32_t &v : l.chunk_start) if (v < -1) v = -1;
        } else {
            l.n_pts1 = (int)(rng() % 40);
            const int nr = (int)(rng() % 10), ni = (int)(rng() % 40), nc = (int)(rng() % 12);
            for (int r = 0; r < nr; ++r) { l.start.push_back((int)(rng() % 50) - 3); l.len.push_back((int)(rng() % 8) - 1); l.ec.push_back((int)(rng() % 20) - 1); }
            for (int i = 0; i < ni; ++i) l.cend_coarse.push_back((int)(rng() % 50) - 3);
            for (int k = 0; k < nc; ++k) { l.chunk_first.push_back((int)(rng() % 45) - 2); l.chunk_len.push_back((int)(rng() % 8) - 1); l.chunk_start.push_back((int)(rng() % 45) - 1); }
        }
        const up2::Table t = build(l);
        if (t.pairs) {
            ++paired;
            bool sizes = t.code.size() == l.cend_coarse.size() && t.chunk_code.size() == l.chunk_first.size() && t.chunk_slot.size() == l.chunk_first.size();
            expect(sizes, "random list: table sizes");
            if (sizes) expect(replay(l, t), "random list: the table reproduces the two passes");
            for (int32_t c : t.chunk_code) expect(c != up2::UP2_STEP, "random list: a chunk start never steps");
        } else
            expect(t.code.empty() && t.chunk_code.empty() && t.chunk_slot.empty(), "a table that does not pair is empty");
    }
    expect(paired > 500, "the random lists reach tables that pair");
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok (%d random lists paired)\n", paired);
    return 0;
}
