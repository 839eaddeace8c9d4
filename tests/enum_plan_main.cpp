// Host walk of trip_plan (csrc/nlosgr_enum.hpp) over every pass mask of rows of 1 .. 12 cells, K = 2 and 3.
// Built and run by tests/test_enum_plan_cpu.py; exits 0 and prints "ok" when every property holds.
#include <cstdio>
#include <cstdlib>

#include "nlosgr_enum.hpp"

#define CHECK(c)                                                                                      \
    do {                                                                                              \
        if (!(c)) {                                                                                   \
            std::fprintf(stderr, "FAIL %s (K %d, row %d, mask 0x%x, cursor %d)\n", #c, K, L, mask, c0); \
            return 1;                                                                                 \
        }                                                                                             \
    } while (0)

int main() {
    long rows = 0, trips_total = 0, tested_total = 0;
    for (int K = 2; K <= 3; ++K) {
        for (int L = 1; L <= 12; ++L) {
            for (unsigned mask = 0; mask < (1u << L); ++mask) {
                int emitted[12] = {0};
                int glen[12] = {0};   // glen[c] = length of the group that starts at cell c
                int c0 = 0, trips = 0;
                while (c0 < L) {
                    const int n = L - c0 < kTripCells ? L - c0 : kTripCells;
                    const bool cont = L - c0 > kTripCells;
                    // bits past n are set on purpose: the plan must ignore them
                    const unsigned bits = ((mask >> c0) & ((1u << n) - 1u)) | (~0u << n);
                    const TripPlan p = trip_plan(bits, n, cont, K);
                    ++trips;
                    tested_total += n;
                    CHECK(p.consumed >= 1 && p.consumed <= n);
                    CHECK(p.count >= 0 && p.count <= kTripGroups);
                    int prev_end = 0;
                    for (int g = 0; g < p.count; ++g) {
                        CHECK(p.len[g] >= 1 && p.len[g] <= K);
                        CHECK(p.start[g] >= prev_end);   // ordered, disjoint
                        CHECK(p.start[g] + p.len[g] <= p.consumed);
                        prev_end = p.start[g] + p.len[g];
                        for (int u = 0; u < p.len[g]; ++u) {
                            const int c = c0 + p.start[g] + u;
                            CHECK((mask >> c) & 1u);   // no failing cell is emitted (contiguous by construction)
                            ++emitted[c];
                        }
                        glen[c0 + p.start[g]] = p.len[g];
                    }
                    // every passing cell the trip consumed is in one of its groups
                    for (int u = 0; u < p.consumed; ++u)
                        if ((mask >> (c0 + u)) & 1u) CHECK(emitted[c0 + u] == 1);
                    c0 += p.consumed;
                    CHECK(trips <= L);
                }
                for (int c = 0; c < L; ++c) CHECK(emitted[c] == (int)((mask >> c) & 1u));
                // every maximal run is cut into groups of K from its left end: only its last group may be
                // short, so the singles are at most the runs whose length is no multiple of K
                int singles = 0, ragged = 0;
                for (int c = 0; c < L;) {
                    if (!((mask >> c) & 1u)) {
                        ++c;
                        continue;
                    }
                    int e = c;
                    while (e < L && ((mask >> e) & 1u)) ++e;
                    const int len = e - c;
                    ragged += len % K != 0;
                    for (int s = c; s < e; s += K) {
                        const int want = e - s < K ? e - s : K;
                        CHECK(glen[s] == want);
                        singles += want == 1;
                    }
                    c = e;
                }
                CHECK(singles <= ragged);
                ++rows;
                trips_total += trips;
            }
        }
    }
    std::printf("ok: %ld rows, %ld trips, %ld cells tested\n", rows, trips_total, tested_total);
    return 0;
}
