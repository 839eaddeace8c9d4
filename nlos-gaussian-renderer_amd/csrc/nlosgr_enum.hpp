// Trip plan of the forward's run-following enumeration (nlosgr_volume_fwd.hip, enumerate_runs).
//
// A trip tests up to kTripCells consecutive cells of ONE row of a pair's candidate box.  Its passing cells
// are appended to the ray queue as groups of up to K adjacent cells; one group is one queue entry and is
// drained by one lane.  trip_plan is the per-lane decision: which groups the trip appends and how many
// cells it consumes.  It is pure integer code, shared by the kernel and a host test program.
//
// Rules (left to right): a maximal run of passing cells is cut into groups of K from its left end.  A group
// shorter than K that touches the trip's right edge while the row continues is deferred, not appended: the
// trip consumes only the cells before it, and the next trip tests its cells again, so they can join their
// right neighbours.  A short group that starts at the trip's first cell is appended as it is: every trip
// consumes at least one cell, so the enumeration always advances.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NLOSGR_ENUM_HD __host__ __device__ __forceinline__
#else
#define NLOSGR_ENUM_HD inline
#endif

constexpr int kTripCells = 4;    // cells tested per trip
constexpr int kTripGroups = 2;   // a trip appends at most this many groups (K = 2 or 3; see the host test)

struct TripPlan {
    int start[kTripGroups];   // first cell of group g, as an offset into the trip
    int len[kTripGroups];     // its cells, 1 .. K
    int count;                // groups appended, 0 .. kTripGroups
    int consumed;             // cells the cursor advances by, 1 .. n
};

// bits: bit u = cell u passes (bits at or above n are ignored); n: cells in the trip, 1 .. kTripCells;
// cont: the row has cells past the trip; K: the largest group, 2 or 3
NLOSGR_ENUM_HD TripPlan trip_plan(unsigned bits, int n, bool cont, int K) {
    TripPlan p;
    p.start[0] = p.start[1] = 0;
    p.len[0] = p.len[1] = 0;
    p.count = 0;
    p.consumed = n;
    int gs = 0, gl = 0;   // the open group
    bool done = false;    // a group was deferred: the trip ends before it
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int u = 0; u <= kTripCells; ++u) {
        const bool pass = !done && u < n && ((bits >> u) & 1u);
        if (gl > 0 && (!pass || gl == K)) {   // close [gs, gs + gl)
            const bool defer = gl < K && gs + gl == n && cont && gs > 0;
            if (defer) {
                p.consumed = gs;
                done = true;
            } else if (p.count < kTripGroups) {
                const bool first = p.count == 0;
                p.start[0] = first ? gs : p.start[0];
                p.len[0] = first ? gl : p.len[0];
                p.start[1] = first ? p.start[1] : gs;
                p.len[1] = first ? p.len[1] : gl;
                ++p.count;
            }
            gl = 0;
        }
        if (pass && !done) {
            gs = gl == 0 ? u : gs;
            ++gl;
        }
    }
    return p;
}
