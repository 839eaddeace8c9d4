// Transient Gaussian NLOS renderer — the pair-major volume forward (gfx950): the lane-serial drains (float
// claim drain, fixed-point FX drain and its twin), the support counter, the FX unit / bright-list / reduce
// kernels, the dense lane = bin kernel, and their launch dispatch (volume_fx_prepare, volume_fwd).
//
// Work decomposition (4 independent waves per workgroup): workgroup = one wall point x a split of the
// Gaussians.  Lane = (wall point, Gaussian) pair enumerates its candidate rays; passing rays become segments
// in a wave-private LDS queue.  Lane = segment then walks its bins with the exp2 recurrence and adds them
// into a wave-private LDS histogram: at the training cutoff as fixed-point integers, two bins per no-return
// ds_add_u64 (FX drain: no claims, order-independent, exact up to one rounding per term), otherwise as
// float2 read-add-writes with a claim table keeping the lanes' addresses distinct.  Either way the forward
// is bitwise deterministic (FX: integer sums; float: fixed-order wave and split reductions).
#include "nlosgr_volume.hpp"
#include "nlosgr_enum.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

// 1 - exp(-x) for 0 <= x <= 1/64 as x (1 - x/2 + x^2/6 - x^3/24) (truncation x^4/120 <= 5e-10 relative):
// the netf transmittance factor exp(-sigma pdf c dT) without an exp when c dT <= 1/64 (C3: 1.25e-3;
// sigma <= 1, pdf <= 1), a launch-uniform choice
constexpr float kRTf0 = 1.0f / kTf0;
template <int N>
__device__ __forceinline__ constexpr float kTfPow() {   // kTf0^N (exact in float for small N: 1 + N 2^-23)
    float r = 1.0f;
    for (int i = 0; i < N; ++i) r *= kTf0;
    return r;
}
__device__ __forceinline__ float om_exp_small(float x) {
    return x * fmaf(x, fmaf(x, fmaf(x, -1.0f / 24.0f, 1.0f / 6.0f), -0.5f), 1.0f);
}

// group entries (the no-occlusion FX forward, see enumerate_runs and fx_twin_setup): slots are lanes (< 64), so
// bits 6-7 of the slot byte carry the group's length - 1: an entry stands for the adjacent cells (i, j) ..
// (i, j + length - 1) of one pair
constexpr int kGroupShift = 6;
constexpr int kGroupMax = 2;   // rays of one row a lane drains at once (the twin drain)
static_assert(kGroupMax == 2, "fx_twin_setup and the twin round take pairs (trip_plan itself: groups of 2 or 3)");

// Lane-serial drain: lane = one ray segment, walking its bins kSteps at a time and adding each
// value into the wave-private LDS histogram with a plain read-add-write.  At step m every lane
// touches bin pos + m, so the adds of one instruction hit distinct addresses whenever the lanes'
// start bins differ — guaranteed per round by a claim table (owner[pos] = lane; losers retry
// next round).  Lanes that did not win, or ran past their segment, point at private pad bins
// and add 0, so the step body is branch-free.  Idle lanes are refilled from the ray queue.
// round 6: 28-bin rounds (with the refill deal at 56 idle lanes and 2 placement claim rounds) for the
// no-occlusion and bin-integrated forwards: C3 734.8 -> 714.4 ms, C4 binint 1150 -> 1090 ms; netf measured
// 883.7 -> 893.8 ms at 28 and keeps 20
template <int MODE, bool TW = false>
__device__ __forceinline__ constexpr int fsteps() { return TW ? kStepsTwin : (MODE == NLOSGR_MODE_NETF ? kStepsNetf : kSteps); }
#ifndef NLOSGR_REFILL
#define NLOSGR_REFILL 48
#endif
constexpr int kRefill = NLOSGR_REFILL;     // refill once this many lanes are idle (or the queue is final)
#ifndef NLOSGR_REFILL_FX
#define NLOSGR_REFILL_FX 56
#endif
// the no-occlusion FX drain with the refill deal (the twin drain without placement, 44 / 48 / 52 / 56 / 60 idle
// lanes: fwd 502.4 / 501.1 / 502.6 / 504.8 / 511.4 ms, one GPU: within 4 ms, so 56 stays)
constexpr int kRefillFx = NLOSGR_REFILL_FX;

#ifndef NLOSGR_FXPERM
#define NLOSGR_FXPERM 1   // FX refill permutation (the deal, see fx_perm): with the bank placement 745.7 vs 750.6 ms
#endif

// per-lane drain state (one segment)
struct Drain {
    int pos, rem;     // next bin, bins left
    float t;          // pos - ks (bin offset from the closest approach)
    float ga, al;     // log2 value(t) = ga t^2 + al   (noocl: al includes log2 w [+ log2 sin theta])
    float t2, ga2, al2;   // twin drain: the second ray of the lane (al2 = kNoTwin: none), see fx_twin_setup
    float st;         // sin(theta_i) (kept separate only when per-ray outputs are written)
    float sc, wc, T;      // netf: sigma c dT, w c dT, transmittance T at pos (linear: one exp per bin)
    float beta, xlo, elo; // binint: dr sqrt(a/2), lower bin edge beta (kap - 1/2) and erfc(|xlo|)
    int rbase;        // RAYS: ray * nr
    int wrap;         // dense no-occlusion: bins [0, wrap) still to drain after the first piece [start, nr)
    float tw;         // dense no-occlusion: t at bin 0
};

// Dense no-occlusion segments span every bin, so they would all claim start bin 0 and drain in a
// one-winner-per-round staircase.  Each bin's value is evaluated exactly (no recurrence), so a
// segment may start anywhere: it drains [stag, nr) and then wraps to [0, stag).
template <int MODE, bool DENSE>
__device__ __forceinline__ constexpr bool dense_wrap() { return DENSE && MODE == NLOSGR_MODE_NOOCL; }

template <int MODE, bool DENSE, bool RAYS>
__device__ __forceinline__ bool drain_setup(const float* A, const float* u0, float lw, float sc, float wc,
                                            float2 th, float2 ph, int i, int j, int np_, int nr, float mc2,
                                            float r0, float dr, float inv_dr, float f0log2, Drain& d, int stag = 0) {
    Ray R;
    if (!ray_setup<DENSE>(A, u0, th.x * ph.x, th.x * ph.y, th.y, mc2, r0, inv_dr, nr, R)) return false;
    d.pos = R.kl;
    d.rem = R.kh - R.kl + 1;
    d.t = (float)R.kl - R.ks;
    if (dense_wrap<MODE, DENSE>()) {   // (R.kl, R.kh) = (0, nr - 1)
        d.tw = d.t;
        d.pos = stag;
        d.rem = nr - stag;
        d.wrap = stag;
        d.t = (float)stag - R.ks;
    }

    d.ga = -kHalfLog2e * R.a * dr * dr;
    if (MODE == NLOSGR_MODE_NOOCL) {
        d.al = fmaf(-kHalfLog2e, R.m2min, lw);
        if (!RAYS) d.al += flog2(th.x);
        d.st = th.x;
    } else if (MODE == NLOSGR_MODE_BININT) {
        // bin average of exp(-a (r - t*)^2 / 2) over [r_k -+ dr/2] = sqrt(pi)/(2 beta) (erf(x1) - erf(x0))
        d.beta = dr * sqrtf(0.5f * R.a);
        d.al = fmaf(-kHalfLog2e, R.m2min, lw);   // the erf form's sqrt(pi) / (2 beta) is applied per value
        if (!RAYS) d.al += flog2(th.x);
        d.st = th.x;
        d.xlo = d.beta * (d.t - 0.5f);
        d.elo = erfcf(fabsf(d.xlo));
    } else {
        d.al = -kHalfLog2e * R.m2min;
        d.sc = sc;
        d.wc = RAYS ? wc : wc * th.x;   // histogram-only: sin(theta) folded into the weight
        d.T = fast_exp2((float)R.kl * f0log2);   // (1 + 1e-7)^kl: the empty bins before the segment
        d.st = th.x;
    }
    d.rbase = (i * np_ + j) * nr;
    return true;
}

// Run-following enumeration (the twin drain of the no-occlusion FX forward; lane = pair).  A trip tests
// kTripCells consecutive cells of ONE row of the box (one theta read, kTripCells phi reads; cells past the
// row's end repeat its first cell and are masked) and never wraps, so the passing cells of a row pair up
// along their run wherever the trips fall: trip_plan (nlosgr_enum.hpp) cuts every run into groups of K from
// its left end and defers a short group at the trip's right edge to the next trip, which tests those cells
// again.  One group = one queue entry (pack_ray with length - 1 at kGroupShift).  A trip consumes at least one
// cell and appends at most kTripGroups entries: cnt < 64 + kTripGroups * 64 <= kRQ on return.
template <int K>
__device__ __forceinline__ void enumerate_runs(const float* M, int i1, int j0, int j1, bool& more, int& ci, int& cj,
                                               const float2* tth, const float2* tph, int nt1, unsigned* rayq,
                                               int qbase, int& cnt) {
    static_assert(64 + kTripGroups * 64 <= kRQ, "a trip appends at most kTripGroups entries per lane: 64 queued + "
                                                "kTripGroups * 64 appended must fit the ray queue ring");
    const int lane = lane_id();
    do {
        // all table reads are issued before any queue store, the tests are unpredicated
        const int n = min(kTripCells, j1 - cj + 1);   // cells of this trip (>= 1 while more)
        const float2 th = tth[min(ci, nt1)];
        float2 phs[kTripCells];
#pragma unroll
        for (int u = 0; u < kTripCells; ++u) phs[u] = tph[u < n ? cj + u : cj];
        unsigned bits = 0u;
#pragma unroll
        for (int u = 0; u < kTripCells; ++u)
            bits |= (more & (u < n) & (quadric(M, th.x * phs[u].x, th.x * phs[u].y, th.y) >= 0.f)) ? 1u << u : 0u;
        const TripPlan tp = trip_plan(bits, n, cj + kTripCells <= j1, K);
        unsigned es[kTripGroups];
        bool put[kTripGroups];
#pragma unroll
        for (int g = 0; g < kTripGroups; ++g) {
            put[g] = more && g < tp.count;
            es[g] = pack_ray(lane | ((tp.len[g] - 1) << kGroupShift), ci, cj + tp.start[g]);
        }
        {
            const bool wrap = cj + tp.consumed > j1;
            cj = wrap ? j0 : cj + tp.consumed;
            ci += wrap ? 1 : 0;
            more = more & (ci <= i1);
        }
        int at = cnt;
#pragma unroll
        for (int g = 0; g < kTripGroups; ++g) {
            const unsigned long long m = __builtin_amdgcn_ballot_w64(put[g]);
            if (put[g]) rayq[(qbase + at + lanes_below(m)) & (kRQ - 1)] = es[g];
            at += __popcll(m);
        }
        cnt = at;
    } while (cnt < 64 && __builtin_amdgcn_ballot_w64(more));
}

__device__ __forceinline__ void compiler_fence() { __asm__ __volatile__("" ::: "memory"); }

// TAIL (culled histogram at cutoff >= kTailCutoff): the forward drain has no end mask.  A round adds
// kSteps values from the even bin at or below pos (a bin before pos, o = 1, adds 0): the bins past the
// segment's end (up to kSteps - 1) get their exact Gaussian values, each < exp(-m_c^2 / 2) of the
// Gaussian's peak (<= 3.7e-6 at m_c >= kTailCutoff), so the result lies between the culled and the
// dense sum.  Bins past nr land in the zeroed pad row.
// debug build (-DNLOSGR_FCOUNT, scripts/drain_counts.py): count_support runs the TAIL forward and returns
// (wave drain rounds, active lanes summed over rounds, claim winners summed) instead of its work counts
#ifdef NLOSGR_FCOUNT
#define NLOSGR_FCOUNT_ON 1
#else
#define NLOSGR_FCOUNT_ON 0
#endif
constexpr float kBetaSeries = 0.5f;   // bin-integrated TAIL drain: series bin average up to this beta

// Fixed-point drain (FX; TAIL no-occlusion histogram, the training hot path).  The wave's LDS histogram
// holds each bin as an unsigned 32-bit count of units 2^-E; a round adds two bins per lane with ONE
// no-return ds_add_u64 of the packed pair (low word = even bin, high word = odd bin), so no claim table:
// every active lane drains every round, and integer adds make the sum independent of the order (the
// forward is bitwise deterministic whatever the schedule).  A value rounds to the nearest unit
// (v_cvt_rpi_i32_f32).
// The unit (round 6): E is set per launch from the amplitude bounds b_g = sigma_g * rho_max_g of the
// Gaussians (fx_bound_kernel; rho_max by Cauchy-Schwarz on the SH bands) so that the bound of the
// ceil(ng/256)-th brightest Gaussian is < 2^kFxBits units (fx_unit_kernel, a quantile over the bounds'
// binary exponents), not the largest bound: a few very bright Gaussians no longer coarsen the unit of
// all the others (round 5 used the maximum, so 0.1 % of Gaussians 10^3-10^4 x brighter than the rest cost
// the rest 10-13 bits, and their sub-half-unit tails rounded to zero: a one-sided bias).  A segment whose
// peak is >= 2^kFxBits units at refill ("bright"; at most the segments of the ceil(ng/256) Gaussians above
// the quantile, and none unless the bounds spread by more than the C-S slack) bypasses the LDS: its lane
// adds its values as u64 integers straight into the wall point's global u64 row (agent-scope atomics), so
// it is as exact as the rest.  E is clamped to <= E(max bound) + range, range = kFxRange or less when
// (bright Gaussians <= ceil(ng / 256)) x (rays per wall point) bright terms per bin could pass 2^(63 - kFxBits -
// range): the u64 sums cannot wrap (C3 / C5: range 16, at most 2^19 / 2^21 bright terms of < 2^40 units).
// A low word must never carry into its high word: every lane sums the peaks (exp2 of the segment's log2
// amplitude, in units) of the LDS segments it took since the last check; a segment adds at most its peak
// to any bin once, so while every lane's sum stays <= thr the largest field stays <= M + 64 thr < 2^32.
// When a lane passes thr the wave reads its histogram's true maximum M; past 2^31 it moves the fields into
// the u64 row in global memory (integer atomics) and zeroes them.  At the end each workgroup adds its 4
// waves' fields to the global u64 histogram [P][nr] (all Gaussian splits of a wall point meet there), and
// fx_reduce_kernel scales it to floats.
#ifdef NLOSGR_FXCOUNT
__device__ unsigned long long g_fdbg[12];
#endif
constexpr int kFxBits = 24;
constexpr int kFxRange = 16;                 // E <= E(max bound) + kFxRange: u64 terms < 2^(kFxBits + kFxRange)
constexpr float kFxBright = 16777216.0f;     // 2^kFxBits
constexpr float kFxMargin = 1.002f;          // segment peak <= bound x 2^E x kFxMargin (binint 1.001, netf (1+1e-7)^nr)
constexpr float kFxLimit = 4294967040.0f;   // largest float below 2^32
// FX bank placement.  A ds_add_u64 is serviced in 4 groups of 16 lanes; two lanes of a group whose words lie
// on the same bank pair (word index mod 16) serialize.  Every active lane advances 10 words per round, so the
// pairs' residues within a group stay fixed for a segment's life: at refill a new segment may start up to
// kFxShift words (2 bins each) early, on the nearest residue no older lane of its group holds and no lower
// new lane of the group takes (3 claim rounds of row-wide DPP ORs; a segment that finds none keeps its
// start).  The early bins get the Gaussian's exact values (as the TAIL overrun past the end), only while the
// recurrence's seed stays >= 2^-100 units.  Placement never affects correctness, only conflicts.
#ifndef NLOSGR_FXSHIFT
#define NLOSGR_FXSHIFT 4
#endif
constexpr int kFxShift = NLOSGR_FXSHIFT;
#ifndef NLOSGR_FXPLACE_ROUNDS
#define NLOSGR_FXPLACE_ROUNDS 2
#endif
constexpr int kFxPlaceRounds = NLOSGR_FXPLACE_ROUNDS;   // claim rounds of the refill placement
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
__device__ __forceinline__ unsigned row_or(unsigned x) {   // OR over the lane's 16-lane row
    x |= dpp_u<0x121>(x);   // row_ror:1
    x |= dpp_u<0x122>(x);   // row_ror:2
    x |= dpp_u<0x124>(x);   // row_ror:4
    x |= dpp_u<0x128>(x);   // row_ror:8
    return x;
}
__device__ __forceinline__ unsigned row_or_below(unsigned x) {   // OR over the lanes below in the row
    x |= dpp_u<0x111>(x);   // row_shr:1 (lanes shifted in read 0)
    x |= dpp_u<0x112>(x);
    x |= dpp_u<0x114>(x);
    x |= dpp_u<0x118>(x);
    return dpp_u<0x111>(x);
}

// round to nearest (floor(x + 0.5)) as an integer in one VALU instruction; 0 <= x < 2^31
__device__ __forceinline__ unsigned cvt_rpi(float x) {
    int r;
    __asm__("v_cvt_rpi_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return (unsigned)r;
}
// two bins of a TAIL drain round into the wave's LDS histogram: FX = one packed fixed-point ds_add_u64
// (values in units), otherwise a float2 read-add-write (the claim table keeps the lanes' pairs distinct)
template <bool FX>
__device__ __forceinline__ void emit2(float2* at, float v0, float v1) {
    if (FX) {
        const unsigned long long pv = ((unsigned long long)cvt_rpi(v1) << 32) | cvt_rpi(v0);
        __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(at), pv, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WAVEFRONT);
    } else {
        float2 x = *at;
        x.x += v0; x.y += v1;
        *at = x;
        __asm__ __volatile__("" ::: "memory");
    }
}

// FX bright segment: one value (in units, rounded to nearest; non-finite saturates) as a u64 integer add
// into the wall point's global row (agent-scope atomic, no return)
__device__ __forceinline__ void fx_gadd(unsigned long long* at, float v) {
    const unsigned long long u = (unsigned long long)fminf(v + 0.5f, 1.8e19f);
    __hip_atomic_fetch_add(at, u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a lane without a second ray: al2 = kNoTwin makes every value of the second recurrence exp2(-200) = 0
constexpr float kNoTwin = -200.f;
// FX refill placement (see kFxShift): newl = this lane took a new segment, act = it holds one.  Not for the twin
// drain: with two rays per lane its shifts and their extra bins cost more than the conflicts they avoid
// (rejected table)
__device__ __forceinline__ void fx_place(bool newl, bool act, Drain& d) {
    if (!__builtin_amdgcn_ballot_w64(newl)) return;
    const int pb = d.pos >> 1, ph = pb & 15, o = d.pos & 1;
    unsigned occ = row_or((act && !newl) ? (1u << ph) : 0u);
    // reach: the seed exponent at the new start stays >= -100 (no flush to zero), the start >= bin 0
    const float span = d.al + 100.f;
    const float tm = span > 0.f ? __builtin_amdgcn_sqrtf(span * __builtin_amdgcn_rcpf(fmaxf(-d.ga, 1e-30f))) : 0.f;
    const int smax = newl ? min(min(kFxShift, pb), (int)floorf(0.5f * (d.t - (float)o + tm))) : -1;
    bool pend = newl && smax >= 0;
    int sh = 0;
#pragma unroll
    for (int it = 0; it < kFxPlaceRounds; ++it) {
        const unsigned fm = ~occ & 0xFFFFu;
        const unsigned x = ((fm << (15 - ph)) | (fm >> (ph + 1))) & 0xFFFFu;   // bit 15 - k = residue ph - k
        const int dd = x ? (int)__builtin_clz(x) - 16 : 16;
        const bool want = pend && dd <= smax;
        const unsigned bit = want ? 1u << ((ph - dd) & 15) : 0u;
        const bool won = want && !(row_or_below(bit) & bit);
        if (won) sh = dd;
        pend = pend && want && !won;
        occ |= row_or(won ? bit : 0u);
        if (!__builtin_amdgcn_ballot_w64(pend)) break;
    }
    if (sh > 0) {
        const int delta = o + 2 * sh;
        d.pos -= delta;
        d.rem += delta;
        d.t -= (float)delta;
    }
}

// FX refill permutation (no-occlusion FX drain).  Every active lane advances the same kSteps / 2 words per
// round, so the bank pair (word mod 16) of each segment relative to the others is fixed for its life: the
// conflicts of a ds_add_u64 (serviced in 4 groups of 16 lanes, bank pair = word mod 16; scripts/lds_fx_probe.hip
// modes 11-16) are set by which segments share a 16-lane group.  At refill the segments are re-dealt over the
// lanes: sorted by (residue, lane) with the idle lanes last, and position s goes to lane 16 (s mod 4) + s / 4,
// so the segments of one residue land in different groups (a residue held by c segments costs ceil(c / 4) per
// group, the least any assignment can reach) and the active lanes spread evenly over the groups.  The sort is
// bit-serial over ballots (5 key bits, no per-residue tables); the state moves with ds_permute (a bijection).
// The per-lane headroom sums (fxs) stay: their total still bounds every field.
constexpr bool kFxPerm = NLOSGR_FXPERM != 0;   // (default with kRefillFx above)
template <int MODE, bool TW = false>
__device__ __forceinline__ void fx_perm(bool& newl, bool& act, Drain& d, float& fpk) {
    const unsigned res = (unsigned)((d.pos >> 1) & 15);
    // deal: sorted by (residue, lane), idle lanes last; position s -> lane 16 (s mod 4) + s / 4
    const unsigned key = act ? res : 16u;
    unsigned long long eq = ~0ull, lt = 0ull;
#pragma unroll
    for (int b = 4; b >= 0; --b) {
        const bool mine = (key >> b) & 1u;
        const unsigned long long B = __builtin_amdgcn_ballot_w64(mine);
        lt |= mine ? (eq & ~B) : 0ull;
        eq &= mine ? B : ~B;
    }
    const int s = __popcll(lt) + lanes_below(eq);
    const int dst = ((s & 3) << 4) | (s >> 2);
    const int a4 = dst << 2;
    if (TW) {
        // one word carries rem, pos and the two flags: an active lane has 0 < rem and 0 <= pos < pos + rem <= nr,
        // nr <= 4096 (validate), so 13 bits hold each.  The peak sum fpk is not moved: the headroom re-arm, the
        // only reader of a dealt segment's peak, computes it again from al and al2
        const int ri = act ? (d.rem | (d.pos << 13) | (newl ? (1 << 30) : 0)) : 0;
        const int ri2 = __builtin_amdgcn_ds_permute(a4, ri);
        d.t = __int_as_float(__builtin_amdgcn_ds_permute(a4, __float_as_int(d.t)));
        d.ga = __int_as_float(__builtin_amdgcn_ds_permute(a4, __float_as_int(d.ga)));
        d.al = __int_as_float(__builtin_amdgcn_ds_permute(a4, __float_as_int(d.al)));
        d.t2 = __int_as_float(__builtin_amdgcn_ds_permute(a4, __float_as_int(d.t2)));
        d.ga2 = __int_as_float(__builtin_amdgcn_ds_permute(a4, __float_as_int(d.ga2)));
        d.al2 = __int_as_float(__builtin_amdgcn_ds_permute(a4, __float_as_int(d.al2)));
        act = ri2 != 0;
        newl = (ri2 >> 30) & 1;
        d.rem = ri2 & 0x1FFF;
        d.pos = (ri2 >> 13) & 0x1FFF;
        return;
    }
    const int ri = act ? (d.rem | (newl ? (1 << 30) : 0)) : 0;
    const int ri2 = __builtin_amdgcn_ds_permute(a4, ri);
    d.pos = __builtin_amdgcn_ds_permute(a4, d.pos);
    d.t = __int_as_float(__builtin_amdgcn_ds_permute(a4, __float_as_int(d.t)));
    d.ga = __int_as_float(__builtin_amdgcn_ds_permute(a4, __float_as_int(d.ga)));
    d.al = __int_as_float(__builtin_amdgcn_ds_permute(a4, __float_as_int(d.al)));
    fpk = __int_as_float(__builtin_amdgcn_ds_permute(a4, __float_as_int(fpk)));
    if (MODE == NLOSGR_MODE_NETF) {   // the segment's transmittance (carrying its weight) and sigma c dT
        d.T = __int_as_float(__builtin_amdgcn_ds_permute(a4, __float_as_int(d.T)));
        d.sc = __int_as_float(__builtin_amdgcn_ds_permute(a4, __float_as_int(d.sc)));
    }
    act = ri2 != 0;
    newl = (ri2 >> 30) & 1;
    d.rem = ri2 & ((1 << 30) - 1);
}

// One TAIL drain round of a lane's segment (the QUADF histograms at cutoff >= kTailCutoff): kSteps values from
// the even bin at or below pos (slot 0 before pos adds 0 in a segment's first round), every pair of bins to
// emit(kv, v0, v1); t = d.t, T = the round's copy of d.T (netf: updated).  The drain rounds emit into the LDS
// histogram, or (the bright launch, BR) the wall point's global u64 row.
constexpr int kVW = 2;   // bins per LDS access of the vector drain (float2 / packed u64)
template <int MODE, class Emit>
__device__ __forceinline__ void tail_round(const Drain& d, const float t, float& T, Emit&& emit) {
    const int o = d.pos & (kVW - 1);
    if (MODE == NLOSGR_MODE_NOOCL) {
        // the recurrence is seeded at pos (inside the support: a seed one bin further out can
        // underflow for Gaussians much narrower than a bin); slot 0 before pos (o = 1) adds 0
        float cur = fast_exp2(fmaf(d.ga, t * t, d.al));
        float q = fast_exp2(d.ga * fmaf(2.f, t, 1.f));
        const float cc = fast_exp2(2.f * d.ga);
        {
#pragma unroll
            for (int kv = 0; kv < fsteps<MODE>() / kVW; ++kv) {
                const float v0 = (kv == 0 && o) ? 0.f : cur;
                if (kv == 0) {
                    cur = o ? cur : cur * q;
                    q = o ? q : q * cc;
                } else {
                    cur *= q;
                    q *= cc;
                }
                const float v1 = cur;
                cur *= q;
                q *= cc;
                emit(kv, v0, v1);
            }
        }
    } else if (MODE == NLOSGR_MODE_BININT) {
        // bin-integrated (C4), TAIL: the average of exp(-beta^2 t^2) over the bin [t - 1/2, t + 1/2]
        // (t in bins from the closest approach, beta = dr sqrt(a / 2)) is g(t) (1 + sum_n g^(2n)(t) /
        // (2^2n (2n+1)!) / g(t)) = g(t) P(beta^2 t^2), P a cubic from the n <= 3 terms: relative error
        // <= 7e-8 for beta <= kBetaSeries (a Gaussian wider than 1.4 bins along the ray), so g comes
        // from the exp2 recurrence as in the numerical drain and each bin costs a cubic instead of
        // two erfc.  Narrower rays (beta > kBetaSeries) take the erf difference, when a round holds one.
        const float b = d.beta * d.beta;
        const float c3 = b * b * b * (1.0f / 5040.0f);
        const float c2 = b * b * fmaf(b, -1.0f / 672.0f, 1.0f / 120.0f);
        const float c1 = b * fmaf(b, fmaf(b, 1.0f / 448.0f, -1.0f / 40.0f), 1.0f / 6.0f);
        const float c0 = fmaf(b, fmaf(b, fmaf(b, -1.0f / 2688.0f, 1.0f / 160.0f), -1.0f / 12.0f), 1.0f);
        const float t0 = t - (float)o;    // t of slot 0
        float cur = fast_exp2(fmaf(d.ga, t * t, d.al));
        float q = fast_exp2(d.ga * fmaf(2.f, t, 1.f));
        const float cc = fast_exp2(2.f * d.ga);
        const bool series = d.beta <= kBetaSeries;
        const bool anyerf = __builtin_amdgcn_ballot_w64(!series) != 0;   // (EXEC = the winners)
        const float pref = fast_exp2(d.al) * (0.88622692545275801f * frcp(d.beta));
        {
#pragma unroll
            for (int kv = 0; kv < fsteps<MODE>() / kVW; ++kv) {
                float v[kVW];
#pragma unroll
                for (int jj = 0; jj < kVW; ++jj) {
                    const int jslot = kVW * kv + jj;
                    const float tj = t0 + (float)jslot;
                    const float u = b * tj * tj;
                    float val = cur * fmaf(u, fmaf(u, fmaf(u, c3, c2), c1), c0);
                    if (anyerf && !series) {
                        const float x0 = d.beta * (tj - 0.5f), x1 = d.beta * (tj + 0.5f);
                        const float e0 = erfcf(fabsf(x0)), e1 = erfcf(fabsf(x1));
                        const float df = x0 >= 0.f ? e0 - e1 : (x1 <= 0.f ? e1 - e0 : 2.0f - e0 - e1);
                        val = pref * df;
                    }
                    const bool pre = kv == 0 && jj < o;   // slot before pos (first round of a segment)
                    v[jj] = pre ? 0.f : val;
                    cur = pre ? cur : cur * q;
                    q = pre ? q : q * cc;
                }
                emit(kv, v[0], v[1]);
            }
        }
    } else {
        // netf, TAIL: out_k = w c dT sin(theta) pdf_k T_k, T_{k+1} = T_k (exp(-sigma pdf_k c dT)
        // + 1e-7), two bins per float2 read-add-write; slot 0 before pos (o = 1, a segment's
        // first round) adds 0 and leaves T as it is
        float cur = fast_exp2(fmaf(d.ga, t * t, d.al));   // seeded at pos (see above)
        // the recurrence runs on p~_m = pdf_m c0^m and the transmittance on T~_m = T_m / c0^m (m = bins
        // past pos, c0 = kTf0 = 1 + 1e-7): v_m = T~_m p~_m = T_m pdf_m and T~_{m+1} = T~_m f_m / c0 =
        // T~_m + v_m g(p~_m) with g the cubic's p-terms over c0, one fma per bin (T rescaled per round)
        float q = fast_exp2(d.ga * fmaf(2.f, t, 1.f)) * kTf0;
        const float cc = fast_exp2(2.f * d.ga);
        // the TAIL netf forward runs only at c dT <= kSmallX, so x = sigma pdf c dT <= 1/64 and
        // exp(-x) + 1e-7 is the cubic the backward uses (truncation x^4 / 24 <= 2.5e-9): no exp.
        // As a cubic in pdf: f = c0 + e1 pdf + e2 pdf^2 + e3 pdf^3, e1 = -sx, e2 = sx^2 / 2, e3 =
        // -sx^3 / 6 (the 1e-7 folded into c0: 1 + 1e-7 rounds to 1 + 2^-23, 1.9e-8 per bin); g takes
        // p~ for pdf, 1 + 2.4e-6 relative at most within a round: f off by <= 2.4e-6 x per bin
        const float sx = d.sc;
        const float e1 = -sx * kRTf0, e2 = 0.5f * sx * sx * kRTf0, e3 = (-1.0f / 6.0f) * sx * sx * sx * kRTf0;
        auto gfac = [e1, e2, e3](float pv) { return fmaf(pv, fmaf(pv, e3, e2), e1); };
        {
#pragma unroll
            for (int kv = 0; kv < fsteps<MODE>() / kVW; ++kv) {
                const float p0 = cur;
                if (kv == 0) {
                    cur = o ? cur : cur * q;
                    q = o ? q : q * cc;
                } else {
                    cur *= q;
                    q *= cc;
                }
                const float p1 = cur;
                cur *= q;
                q *= cc;
                // T carries w c dT sin(theta) (set at the segment's start); slot 0 before pos adds 0
                // and (v0 = 0) leaves T as it is
                const float v0 = (kv == 0 && o) ? 0.f : T * p0;
                T = fmaf(v0, gfac(p0), T);
                const float v1 = T * p1;
                T = fmaf(v1, gfac(p1), T);
                emit(kv, v0, v1);
            }
        }
        T *= o ? kTfPow<fsteps<MODE>() - 1>() : kTfPow<fsteps<MODE>()>();   // T = T~ c0^(bins advanced)
    }
}

// Twin drain (TW; the no-occlusion FX forward with the refill deal and without the bank placement, the training
// hot path).  The forward is
// paced by the number of ds_add_u64 it issues, and that number is set by rays: a lane that drains the two
// adjacent cells (i, j), (i, j + 1) of one pair at once sums their values in registers and issues one add for
// both (the cells are paired along their row's run of passing cells, see enumerate_runs).
// The two segments' closest-approach bins are a few bins apart, so their union is little longer than
// either (scripts/twin_estimate.py), and both setups share the pair's shuffled A, u0, lw.
// The lane walks the union [min kl, max kh]; each ray's recurrence is seeded at the round's first bin from its
// own (t, ga, al).  Outside its own support a ray adds its exact Gaussian values (< exp(-m_c^2 / 2) of its peak,
// the same tail the TAIL rounds add past a segment's end), provided its seed does not flush to zero before
// its centre (the rest of the round would be lost) and its ratio does not overflow (0 x inf): both rays must
// satisfy fx_place's condition at the union's first bin, seed exponent >= -100 and ratio exponent <= 120.  A
// seed that is fine there is fine at every later round start before the centre (|t| only shrinks).  A twin
// that fails is split: the lane keeps the first ray and the second goes back to the queue as a single entry.
// Returns 0: no segment, 1: one ray, 2: twin, 3: split (d holds the first ray).  pk = the sum of the peaks
// (units).  The work counts (nlosgr_count_support) are not kept here: a counting launch never takes the FX drain.
__device__ __forceinline__ bool fx_seed_ok(float ga, float al, float t) {
    return fmaf(ga, t * t, al) >= -100.f && ga * fmaf(2.f, t, 1.f) <= 120.f;
}
__device__ __forceinline__ int fx_twin_setup(const float* A, const float* u0, float lw, float2 th, float2 pha,
                                             float2 phb, bool twin, int nr, float mc2, float r0, float dr,
                                             float inv_dr, Drain& d, float& pk) {
    Ray Ra, Rb;
    bool gota = ray_setup<false>(A, u0, th.x * pha.x, th.x * pha.y, th.y, mc2, r0, inv_dr, nr, Ra);
    bool gotb = twin && ray_setup<false>(A, u0, th.x * phb.x, th.x * phb.y, th.y, mc2, r0, inv_dr, nr, Rb);
    if (!gota && gotb) {   // only the second cell has bins: it is the lane's one ray
        Ra = Rb;
        gota = true;
        gotb = false;
    }
    if (!gota) return 0;
    const float lst = flog2(th.x);
    d.pos = Ra.kl;
    d.rem = Ra.kh - Ra.kl + 1;
    d.t = (float)Ra.kl - Ra.ks;
    d.ga = -kHalfLog2e * Ra.a * dr * dr;   // (the expressions of drain_setup: a single is bit-identical to it)
    d.al = fmaf(-kHalfLog2e, Ra.m2min, lw) + lst;
    d.t2 = 0.f; d.ga2 = 0.f; d.al2 = kNoTwin;
    pk = fast_exp2(d.al);
    if (!gotb) return 1;
    const float gb = -kHalfLog2e * Rb.a * dr * dr, ab =fmaf(-kHalfLog2e, Rb.m2min, lw) + lst;
    const int pos = min(Ra.kl, Rb.kl), end = max(Ra.kh, Rb.kh);
    const float ta = (float)pos - Ra.ks, tb = (float)pos - Rb.ks;
    if (!(fx_seed_ok(d.ga, d.al, ta) && fx_seed_ok(gb, ab, tb))) return 3;
    d.pos = pos;
    d.rem = end - pos + 1;
    d.t = ta;
    d.t2 = tb; d.ga2 = gb; d.al2 = ab;
    pk += fast_exp2(ab);
    return 2;
}
// one TAIL round of a twin lane (tail_round's no-occlusion body with two recurrences): slot 0 before pos adds
// 0; every pair of bins emits the two rays' sums
template <class Emit>
__device__ __forceinline__ void tail_round_twin(const Drain& d, Emit&& emit) {
    const int o = d.pos & (kVW - 1);
    float cur = fast_exp2(fmaf(d.ga, d.t * d.t, d.al));
    float q = fast_exp2(d.ga * fmaf(2.f, d.t, 1.f));
    const float cc = fast_exp2(2.f * d.ga);
    float cur2 = fast_exp2(fmaf(d.ga2, d.t2 * d.t2, d.al2));
    float q2 = fast_exp2(d.ga2 * fmaf(2.f, d.t2, 1.f));
    const float cc2 = fast_exp2(2.f * d.ga2);
#pragma unroll
    for (int kv = 0; kv < kStepsTwin / kVW; ++kv) {
        const float v0 = (kv == 0 && o) ? 0.f : cur + cur2;
        if (kv == 0) {
            cur = o ? cur : cur * q;
            q = o ? q : q * cc;
            cur2 = o ? cur2 : cur2 * q2;
            q2 = o ? q2 : q2 * cc2;
        } else {
            cur *= q;
            q *= cc;
            cur2 *= q2;
            q2 *= cc2;
        }
        const float v1 = cur + cur2;
        cur *= q;
        q *= cc;
        cur2 *= q2;
        q2 *= cc2;
        emit(kv, v0, v1);
    }
}

template <int PRESET, int MODE, bool DENSE, bool RAYS, bool CACHE, bool TAIL, bool FX, bool BR = false, bool TW = false>
__device__ __forceinline__ void fwd_body(const KArgs& k) {
    extern __shared__ __align__(16) float smem[];
    const int nr = k.geo.nr, nt = k.geo.nt, np_ = k.geo.np;
    const FwdLayout L(nr, nt, np_, FX);
    static_assert(!FX || (TAIL && !DENSE && !RAYS), "fixed-point drain: TAIL histogram drains only");
    float2* tth = reinterpret_cast<float2*>(smem);
    float2* tph = tth + nt;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();   // wave-uniform (SGPR)
    float* wb = smem + wave * L.wave_stride;
    float* hist = wb + L.hist;
    unsigned char* owner = reinterpret_cast<unsigned char*>(wb + L.owner);
    unsigned* rayq = reinterpret_cast<unsigned*>(wb + L.rayq);
    const int p = blockIdx.x;
    // Gaussian split of this wall point (grid.y; 64-aligned ranges): partial histograms are summed
    // in split order by hist_reduce_kernel when gridDim.y > 1
    const int gsplit = blockIdx.y, nsp = gridDim.y;
    // BR (the bright launch): the Gaussians of the bright list instead of all of them
    const int gcount = BR ? k.fx_info[4] : k.g.ng;
    const int gper = (((gcount + nsp - 1) / nsp) + 63) & ~63;
    const int g_lo = gsplit * gper, g_hi = min(gcount, g_lo + gper);

    for (int t = threadIdx.x; t < nt; t += blockDim.x)
        tth[t] = make_float2(k.geo.sin_theta[(size_t)p * nt + t], k.geo.cos_theta[(size_t)p * nt + t]);
    for (int t = threadIdx.x; t < np_; t += blockDim.x)
        tph[t] = make_float2(k.geo.cos_phi[(size_t)p * np_ + t], k.geo.sin_phi[(size_t)p * np_ + t]);
    for (int t = lane; t < (FX ? nr + kStepsPad + 4 : nr + 2 * kStepsPad + 64); t += 64) hist[t] = 0.f;
    __syncthreads();

    const float px = k.geo.wall[3 * p], py = k.geo.wall[3 * p + 1], pz = k.geo.wall[3 * p + 2];
    const float* lin = k.geo.grid_lin + 4 * (size_t)p;
    const float mc2 = k.opt.cutoff * k.opt.cutoff;
    const float r0 = k.geo.r[0];
    const float dr = nr > 1 ? (k.geo.r[nr - 1] - r0) / (float)(nr - 1) : 0.f;
    const float inv_dr = dr > 0.f ? 1.0f / dr : 0.f;
    const float cdt = k.opt.c_deltaT;
    const float f0log2 = log2f(1.0f + 1e-7f);
    float* rout = RAYS ? k.ray_out + (size_t)p * nt * np_ * nr : nullptr;
    const float rscale = k.opt.ray_scale;
    const int flags = k.opt.flags;
    // the trimmed support (fx_trim_m2, nlosgr_volume.hpp): the no-occlusion FX drains, twin, one ray and bright
    constexpr bool TRIMK = FX && MODE == NLOSGR_MODE_NOOCL && !CACHE;
    const bool trim = TRIMK && (flags & NLOSGR_FLAG_FX_TRIM) != 0;   // launch-uniform
    // FX: log2 of the unit scale, folded into every pair's log2 amplitude; per-lane peak bookkeeping
    const float fxE = FX ? (float)k.fx_info[0] : 0.f;
    const float fxS = FX ? fast_exp2(fxE) : 1.f;   // exact: fxE is an integer
    float fthr = kFxLimit / 64.f;   // wave-uniform
    float fpk = 0.f, fxs = 0.f;     // this lane's segment peak, and its peaks since the last check
    unsigned long long* const grow = FX ? k.hfx + (size_t)p * nr : nullptr;
    unsigned* hist32 = reinterpret_cast<unsigned*>(hist);
    const int nfx = nr + kStepsPad + 2;   // fields a round can reach (bins past nr are pad)
    // the float2 drain (two bins per LDS read-add-write; claim keys on bin pairs)
    constexpr bool QUADF = (MODE == NLOSGR_MODE_NOOCL || ((MODE == NLOSGR_MODE_NETF || MODE == NLOSGR_MODE_BININT) && TAIL)) &&
                           !RAYS && !DENSE;
    const int pad = nr + kStepsPad + lane;       // this lane's private pad bins (non-winners)
    const int padq = al4(nr + kStepsPad);        // quad drain: one pad quad row shared by non-winners (they add 0)
    unsigned npair = 0, nseg = 0;
    unsigned long long nsamp = 0;

#ifdef NLOSGR_FXCOUNT
    unsigned long long fdbg[11] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};   // wave-uniform diagnostics
    // ([0..4]: the rounds' bank-pair occupancy; [5..8]: refills, entries taken, refills taking < 32 entries,
    // refills after the chunk's enumeration ended; [9]: rays taken with bins (a twin counts two); [10]: pairs
    // dropped by NLOSGR_FLAG_FX_TRIM because they peak below a quarter unit)
#endif
    Drain d;
    d.pos = 0; d.rem = 0; d.t = 0.f; d.ga = 0.f; d.al = 0.f; d.st = 0.f;
    d.sc = 0.f; d.wc = 0.f; d.T = 0.f; d.rbase = 0;
    d.beta = 0.f; d.xlo = 0.f; d.elo = 0.f;
    d.wrap = 0; d.tw = 0.f;
    d.t2 = 0.f; d.ga2 = 0.f; d.al2 = kNoTwin;
    static_assert(!TW || (FX && !BR && !CACHE && kFxPerm && MODE == NLOSGR_MODE_NOOCL),
                  "twin drain: the no-occlusion FX forward with the refill deal only");
    unsigned ntwin = 0, nsplit = 0;   // TW: twins drained as one segment / split at the merge guard (wave-uniform)
    bool act = false;
    int qhead = 0, qcount = 0;

    constexpr int VW = kVW;

    for (int base = g_lo + wave * 64;; base += kBlock) {
        const bool have = base < g_hi;         // wave-uniform
        Pair P;
        float lw = 0.f, sc = 0.f, wc = 0.f;
        bool more = false;
        int ci = 0, cj = 0;
        unsigned long long crec0 = 0ull, crec1 = 0ull;   // CACHE: passing cells of this lane's box
        int ccell = 0;
        P.i0 = P.i1 = P.j0 = P.j1 = 0;
        if (have) {
            const int gi = base + lane;
            // the record is loaded ahead of the setup math; the SH coefficients are read from global
            // inside the albedo sum (a register copy of the row spilled the setup at 80 VGPRs)
            const int gl = BR ? k.fx_blist[min(gi, g_hi - 1)] : min(gi, k.g.ng - 1);
            const GaussRec nrec = k.recs[gl];
            // FX: Gaussians whose bound reaches 2^kFxBits units (bright, see kFxBits) are the bright launch's:
            // preprocess_kernel stored them with a negative sigma (the same comparison as fx_blist_kernel), so
            // here w <= 0 skips them; the bright launch takes |sigma|
            if (gi < g_hi) {
                float mu[3];
                load_rec(nrec, P, mu);
                if (BR) P.sigma = fabsf(P.sigma);
                pair_setup<PRESET, DENSE, TRIMK>(k, k.g.features + (size_t)gl * k.g.k_feat, mu, px, py, pz, lin, mc2, P,
                                                 fxE, trim);
                more = (P.w > 0.f) && P.i0 <= P.i1 && P.j0 <= P.j1;
                lw = more ? flog2(P.w) + fxE : 0.f;
                if (trim) {   // a pair that peaks below a quarter unit adds nothing
                    const bool dead = more && !(lw + kTrimQuarter > 0.f);
#ifdef NLOSGR_FXCOUNT
                    if (!BR) fdbg[10] += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(dead));
#endif
                    more = more && !dead;
                }
                sc = P.sigma * cdt;
                wc = more ? P.w * cdt * fxS : 0.f;   // netf: the value's scale rides on T
            }
            if (flags & 2) more = false;      // diagnostics: pair setup only
            npair += NLOSGR_FCOUNT_ON ? 0u : (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(more));
            ci = P.i0; cj = P.j0;
        }
        while (true) {
            if (qcount < 64 && __builtin_amdgcn_ballot_w64(more)) {
                wave_sync();
                if (TW)
                    enumerate_runs<kGroupMax>(P.M, P.i1, P.j0, P.j1, more, ci, cj, tth, tph, nt - 1, rayq, qhead, qcount);
                else
                    enumerate_box<DENSE, CACHE>(P.M, P.i1, P.j0, P.j1, more, ci, cj, tth, tph, nt - 1, rayq, qhead,
                                                qcount, &crec0, &crec1, &ccell);
                wave_sync();
            }
            const bool anymore = __builtin_amdgcn_ballot_w64(more) != 0;
            const unsigned long long idle = __builtin_amdgcn_ballot_w64(!act);
            const int nidle = __popcll(idle);
            // the no-occlusion FX drain refills later: the deal's cost is per refill (REFILL 48 / 52 / 56 / 60 / 62:
            // 745.9 / 735.7 / 732.4 / 736.7 / 745.4 ms, same box)
            constexpr int kRef = (FX && !BR && kFxPerm && MODE == NLOSGR_MODE_NOOCL) ? kRefillFx : kRefill;
            // TW, the chunk's tail (every box exhausted): a refill waits until it can take the whole queue or kRef
            // entries, since a refill costs about one drain round whatever it takes (C3: 7.5 % fewer refills for
            // 0.4 % more rounds).  It ends: no lane enumerates, so active lanes only finish and nidle reaches
            // 64 >= min(kRef, qcount); scripts/refill_replay.py replays the loop on the CPU
            const bool refill = TW ? nidle >= (anymore ? kRef : min(kRef, qcount)) : (nidle >= kRef || !anymore);
            if (qcount > 0 && refill) {
#ifdef NLOSGR_FXCOUNT
                if (FX && !BR) {
                    const unsigned long long nt_ = (unsigned long long)min(nidle, qcount);
                    fdbg[5] += 1ull; fdbg[6] += nt_; fdbg[7] += nt_ < 32ull ? 1ull : 0ull; fdbg[8] += anymore ? 0ull : 1ull;
                }
#endif
                // idle lane of rank r takes queue entry qhead + r; pair data come from lane `slot`
                const int r = lanes_below(idle);
                const bool take = !act && r < qcount;
                const unsigned e = take ? rayq[(qhead + r) & (kRQ - 1)] : 0u;
                const int slot = e & (TW ? 0x3F : 0xFF), i = (e >> 8) & 0xFFF, j = e >> 20;
                float A[9], u0[3];
#pragma unroll
                for (int c = 0; c < 9; ++c) A[c] = __shfl(P.A[c], slot);
#pragma unroll
                for (int c = 0; c < 3; ++c) u0[c] = __shfl(P.u0[c], slot);
                const float lws = __shfl(lw, slot);
                const float mc2r = trim ? fx_trim_m2(lws, mc2) : mc2;   // the ray's support radius, squared
                const float scs = MODE == NLOSGR_MODE_NETF ? __shfl(sc, slot) : 0.f;
                const float wcs = MODE == NLOSGR_MODE_NETF ? __shfl(wc, slot) : 0.f;
                bool got = false;
                int tcode = 0;   // TW: fx_twin_setup's result
                if (TW) {
                    if (take && !(flags & 1)) {
                        const bool twin = ((e >> kGroupShift) & 3u) != 0u;
                        float pk = 0.f;
                        // (j + 1 <= j1 < np for a twin entry; a single reads its own cell twice)
                        tcode = fx_twin_setup(A, u0, lws, tth[i], tph[j], tph[twin ? j + 1 : j], twin, nr, mc2r, r0, dr,
                                              inv_dr, d, pk);
                        got = tcode != 0;
                        if ((flags & NLOSGR_FLAG_FX_TWIN_STATS) && tcode == 2) atomicMax(k.fx_info + 7, d.rem);
                        act = got && !(flags & 4);
                        if (act) {
                            fpk = pk;   // the sum of the two peaks: the most the lane adds to any bin
                            fxs += fpk;
                        }
                    }
                } else if (take && !(flags & 1)) {
                    // dense: consecutive queue entries start 37 bins apart (distinct claim keys)
                    const int stag = dense_wrap<MODE, DENSE>() ? (int)(((unsigned)(qhead + r) * 37u) % (unsigned)nr) : 0;
                    got = drain_setup<MODE, DENSE, RAYS>(A, u0, lws, scs, wcs, tth[i], tph[j], i, j, np_, nr, mc2r,
                                                         r0, dr, inv_dr, f0log2, d, stag);
                    if (got && !NLOSGR_FCOUNT_ON) nsamp += (unsigned)(d.rem + (dense_wrap<MODE, DENSE>() ? d.wrap : 0));
                    if (MODE == NLOSGR_MODE_NETF && TAIL && QUADF) d.T *= d.wc;   // the weight rides on T
                    act = got && !(flags & 4);    // diagnostics: segment records only
                    if (FX && act) {
                        // the segment's largest value (t = 0), in units (netf: T <= its start x (1 + 1e-7)^nr)
                        fpk = MODE == NLOSGR_MODE_NETF ? d.T * fast_exp2(d.al) * 1.001f
                                                       : fast_exp2(d.al) * (MODE == NLOSGR_MODE_BININT ? 1.001f : 1.f);
                        fxs += fpk;
                    }
                }
                nseg += NLOSGR_FCOUNT_ON ? 0u : (unsigned)__popcll(__builtin_amdgcn_ballot_w64(got));
#ifdef NLOSGR_FXCOUNT
                if (FX && !BR && !TW) fdbg[9] += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(got));
#endif
                const int ntake = min(nidle, qcount);
                qhead = (qhead + ntake) & (kRQ - 1);
                qcount -= ntake;
                if (TW) {
                    const unsigned long long tm = __builtin_amdgcn_ballot_w64(tcode == 2);
                    const unsigned long long sm = __builtin_amdgcn_ballot_w64(tcode == 3);
                    ntwin += (unsigned)__popcll(tm);
#ifdef NLOSGR_FXCOUNT
                    fdbg[9] += (unsigned long long)(__popcll(__builtin_amdgcn_ballot_w64(tcode != 0)) + __popcll(tm));
#endif
                    if (sm) {
                        // split twins: the second ray returns to the queue's tail as a single entry (the queue
                        // just gave up ntake >= popc(sm) entries, so the ring cannot overflow)
                        if (tcode == 3) rayq[(qhead + qcount + lanes_below(sm)) & (kRQ - 1)] = pack_ray(slot, i, j + 1);
                        qcount += __popcll(sm);
                        nsplit += (unsigned)__popcll(sm);
                        wave_sync();
                    }
                }
                // (netf keeps its start: its transmittance would have to be re-seeded)
                bool newl = take && act;
                // netf has neither the deal (measured slower: its drain is less LDS-bound) nor the refill
                // placement (its transmittance would need re-seeding)
                if (FX && !BR && kFxPerm && MODE == NLOSGR_MODE_NOOCL) fx_perm<MODE, TW>(newl, act, d, fpk);
                if (FX && !BR && !TW && kFxShift > 0 && MODE != NLOSGR_MODE_NETF) fx_place(newl, act, d);
            }
            const bool anyact = __builtin_amdgcn_ballot_w64(act) != 0;
            if (!anyact) {
                if (!anymore && qcount == 0) break;
                continue;
            }
            if (!anymore && qcount == 0 && have) break;   // next Gaussians; segments carry over
            // claim distinct start keys (distinct addresses; vector drain: distinct start pairs)
            constexpr bool QUAD = QUADF;
            bool win = act;   // FX: integer adds, no claims
            if (FX && !BR && __builtin_amdgcn_ballot_w64(fxs > fthr)) {
                // a lane passed its share of the headroom: read the fields' true maximum (and move
                // them to the global u64 histogram once it passes 2^31)
                wave_sync();
                unsigned mx = 0u;
                for (int t = lane; t < nfx; t += 64) mx = max(mx, hist32[t]);
                for (int o2 = 32; o2 > 0; o2 >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o2));
                if (mx >= 0x80000000u) {
                    if (lane == 0) atomicAdd(k.fx_info + 2, 1);
                    for (int t = lane; t < nfx; t += 64) {
                        const unsigned v = hist32[t];
                        if (v && t < nr)
                            __hip_atomic_fetch_add(k.hfx + (size_t)p * nr + t, (unsigned long long)v, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
                        hist32[t] = 0u;
                    }
                    wave_sync();
                    mx = 0u;
                }
                fthr = (kFxLimit - (float)mx) * (1.0f / 64.0f);
                // an active segment may still add up to its peak to any bin (TW: the deal does not move fpk, so
                // the peak sum is computed again from the lane's two amplitudes, as fx_twin_setup did; a lane
                // without a second ray adds exp2(kNoTwin) = 0)
                const float pkn = TW ? fast_exp2(d.al) + fast_exp2(d.al2) : fpk;
                fxs = act ? pkn : 0.f;
            }
            if (!FX) {
                const int key = QUAD ? (d.pos / VW) : d.pos;
                if (act) owner[key] = (unsigned char)lane;
                wave_sync();
                win = act && owner[key] == (unsigned char)lane;
                wave_sync();
            }
            if (NLOSGR_FCOUNT_ON) {
                npair += 1u;
                nseg += (unsigned)__popcll(__builtin_amdgcn_ballot_w64(act));
                nsamp += (unsigned)__popcll(__builtin_amdgcn_ballot_w64(win));   // every lane: / 64 on the host
            }
#ifdef NLOSGR_FXCOUNT
            if (FX && !BR) {   // diagnostics: bank-pair occupancy of this round's ds_add_u64 groups
                const unsigned res = (unsigned)((d.pos >> 1) & 15);
                unsigned long long same = __builtin_amdgcn_ballot_w64(act);
                for (int b = 0; b < 4; ++b) {
                    const unsigned long long B = __builtin_amdgcn_ballot_w64((res >> b) & 1u);
                    same &= ((res >> b) & 1u) ? B : ~B;
                }
                const unsigned long long gm = 0xFFFFull << (lane & 48);
                int cg = act ? __popcll(same & gm) : 0;     // lanes of my group on my bank pair
                for (int o2 = 1; o2 < 16; o2 <<= 1) cg = max(cg, __shfl_xor(cg, o2));
                int cw = act ? __popcll(same) : 0;
                for (int o2 = 1; o2 < 64; o2 <<= 1) cw = max(cw, __shfl_xor(cw, o2));
                unsigned rm = act ? (1u << res) : 0u;
                for (int o2 = 1; o2 < 64; o2 <<= 1) rm |= (unsigned)__shfl_xor((int)rm, o2);
                int sg = 0;
                for (int g4 = 0; g4 < 4; ++g4) sg += __shfl(cg, 16 * g4);
                const int na = __popcll(__builtin_amdgcn_ballot_w64(act));
                fdbg[0] += 1ull; fdbg[1] += (unsigned long long)na; fdbg[2] += (unsigned long long)sg;
                fdbg[3] += (unsigned long long)__popc(rm); fdbg[4] += (unsigned long long)cw;
            }
#endif
            const int remw = win ? d.rem : 0;
            float* hb = hist + (win ? (QUAD ? (d.pos & ~(VW - 1)) : d.pos) : (QUAD ? padq : pad));
            float t = d.t;
            float T = d.T;
            float xlo = d.xlo, elo = d.elo;
            if (QUAD) {
                // kSteps bins from the even bin at or below pos: one ds_read_b64 + ds_write_b64 per 2
                // bins, values by the exp2 recurrence (see kRecurrence).  Slots before pos (first round
                // of a segment only) add 0 and do not advance the recurrence, which starts at pos.
                // The whole round is one EXEC region of the winners (losers take no LDS bank and no
                // per-step mask switching).
                const int o = d.pos & (VW - 1);
                const int lim = remw + o;   // slot j is in the segment iff o <= j < lim
                if (TAIL && win) {
                    // (FX: every emitting lane is a winner, so its row starts at the even bin with no loser select)
                    float2* const hbw = reinterpret_cast<float2*>(FX ? hist + (d.pos & ~(VW - 1)) : hb);
                    if (BR) {   // bright launch: u64 integer adds straight into the wall point's global row
                        const int gb0 = d.pos & ~(VW - 1);
                        tail_round<MODE>(d, t, T, [&](int kv, float v0, float v1) {
                            const int b = gb0 + VW * kv;
                            if (b < nr && v0 > 0.f) fx_gadd(grow + b, v0);
                            if (b + 1 < nr && v1 > 0.f) fx_gadd(grow + b + 1, v1);
                        });
                    } else if (TW) {   // both rays of the lane in one ds_add_u64 per two bins
                        tail_round_twin(d, [&](int kv, float v0, float v1) { emit2<FX>(hbw + kv, v0, v1); });
                    } else {
                        tail_round<MODE>(d, t, T, [&](int kv, float v0, float v1) { emit2<FX>(hbw + kv, v0, v1); });
                    }
                } else if (win) {
                    float cur = fast_exp2(fmaf(d.ga, t * t, d.al));
                    float q = fast_exp2(d.ga * fmaf(2.f, t, 1.f));
                    const float cc = fast_exp2(2.f * d.ga);
                    float2* hb2 = reinterpret_cast<float2*>(hb);
#pragma unroll
                    for (int kv = 0; kv < fsteps<MODE>() / VW; ++kv) {
                        float v[VW];
#pragma unroll
                        for (int jj = 0; jj < VW; ++jj) {
                            const int j = VW * kv + jj;
                            if (kv == 0) {
                                const bool st = jj >= o;
                                v[jj] = (st && j < lim) ? cur : 0.f;
                                cur = st ? cur * q : cur;
                                q = st ? q * cc : q;
                            } else {
                                v[jj] = j < lim ? cur : 0.f;
                                cur *= q;
                                q *= cc;
                            }
                        }
                        float2 x = hb2[kv];
                        x.x += v[0]; x.y += v[1];
                        hb2[kv] = x;
                        compiler_fence();
                    }
                }
                t += (float)(fsteps<MODE, TW>() - o);
            } else {
            // netf, culled: pdf by the exp2 recurrence (kRecurrence), re-seeded per round
            constexpr bool REC = MODE == NLOSGR_MODE_NETF && !DENSE;
            const float nsc = -d.sc * (2.f * kHalfLog2e);   // exp(-sigma c dT pdf) = exp2(pdf nsc)
            float cur = 0.f, rq = 0.f, rcc = 0.f;
            if (REC) {
                cur = fast_exp2(fmaf(d.ga, t * t, d.al));
                rq = fast_exp2(d.ga * fmaf(2.f, t, 1.f));
                rcc = fast_exp2(2.f * d.ga);
            }
#pragma unroll
            for (int m = 0; m < fsteps<MODE>(); ++m) {
                const bool in = m < remw;
                const float e2 = fmaf(d.ga, t * t, d.al);
                float v;
                if (MODE == NLOSGR_MODE_NOOCL) {
                    const float pv = fast_exp2(e2);
                    v = in ? pv : 0.f;
                    if (RAYS) {
                        if (in) atomicAdd(rout + d.rbase + d.pos + m, rscale * pv);
                        v *= d.st;
                    }
                } else if (MODE == NLOSGR_MODE_BININT) {
                    // erf(x1) - erf(x0) from erfc of |x| (no cancellation in the tails)
                    const float x1 = d.beta * (t + 0.5f);
                    const float e1 = erfcf(fabsf(x1));
                    const float df = xlo >= 0.f ? elo - e1 : (x1 <= 0.f ? e1 - elo : 2.0f - elo - e1);
                    xlo = x1;
                    elo = e1;
                    const float pv = fast_exp2(d.al) * (0.88622692545275801f * frcp(d.beta)) * df;
                    v = in ? pv : 0.f;
                    if (RAYS) {
                        if (in) atomicAdd(rout + d.rbase + d.pos + m, rscale * pv);
                        v *= d.st;
                    }
                } else {
                    // T_k = prod_{k' < k} (exp(-sigma pdf_k' c dT) + 1e-7), out_k = w c dT pdf_k T_k
                    float pdf;
                    if (REC) {
                        pdf = cur;
                        cur *= rq;
                        rq *= rcc;
                    } else {
                        pdf = fast_exp2(e2);
                    }
                    const float f = fast_exp2(pdf * nsc) + 1e-7f;
                    const float val = d.wc * T * pdf;
                    if (RAYS && in) atomicAdd(rout + d.rbase + d.pos + m, rscale * val);
                    T *= in ? f : 1.f;
                    v = in ? (RAYS ? val * d.st : val) : 0.f;
                }
                t += 1.f;
                const float x = hb[m];
                hb[m] = x + v;
                compiler_fence();
            }
            }
            if (win) {
                const int adv = QUAD ? fsteps<MODE, TW>() - (d.pos & (VW - 1)) : fsteps<MODE, TW>();
                d.t = t;
                if (TW) d.t2 += (float)(fsteps<MODE, TW>() - (d.pos & (VW - 1)));
                d.T = T;
                d.xlo = xlo;
                d.elo = elo;
                d.pos += adv;
                d.rem -= adv;
                if (dense_wrap<MODE, DENSE>() && d.rem <= 0 && d.wrap > 0) {   // second piece [0, wrap)
                    d.pos = 0;
                    d.rem = d.wrap;
                    d.wrap = 0;
                    d.t = d.tw;
                }
                act = d.rem > 0;
            }
        }
        if (CACHE && have && base + lane < g_hi) {
            // every candidate of this chunk has been tested: record the pair's passing cells
            const int bw = P.j1 - P.j0 + 1, bh = P.i1 - P.i0 + 1;
            const bool live = P.w > 0.f && bw > 0 && bh > 0;
            const size_t o = (size_t)p * k.g.ng + base + lane;
            const bool ok = !live || bw * bh <= kCacheCells;
            k.cmask[o] = live ? make_ulonglong2(crec0, crec1) : make_ulonglong2(0ull, 0ull);
            k.cbox[o] = ok ? cache_box(live ? P.i0 : 0, live ? P.j0 : 0, live ? bw : 1) : 0u;
            k.crho[o] = live ? P.rho : 0.f;
        }
        if (!have) break;
    }
    if (!TW && k.counts) {
        unsigned long long ns = nsamp;
        for (int o = 32; o > 0; o >>= 1) ns += __shfl_xor(ns, o);
        if (lane == 0) {
            atomicAdd(k.counts, (unsigned long long)npair);
            atomicAdd(k.counts + 1, (unsigned long long)nseg);
            atomicAdd(k.counts + 2, ns);
        }
    }
#ifdef NLOSGR_FXCOUNT
    if (lane == 0)
        for (int c = 0; c < 11; ++c) atomicAdd(&g_fdbg[c], fdbg[c]);
#endif
    if (TW && lane == 0) {   // twins formed / split (nlosgr_fx_info)
        if (ntwin) atomicAdd(k.fx_info + 5, (int)ntwin);
        if (nsplit) atomicAdd(k.fx_info + 6, (int)nsplit);
    }
    if (BR) {   // bright segments taken (nlosgr_fx_info)
        if (lane == 0 && nseg) atomicAdd(k.fx_info + 3, (int)nseg);
        return;
    }
    __syncthreads();
    if (FX) {
        // the 4 waves' fields of each bin -> one integer add into the wall point's global u64 row
        for (int t = threadIdx.x; t < nr; t += blockDim.x) {
            unsigned long long s = 0ull;
            for (int w = 0; w < kWaves; ++w)
                s += reinterpret_cast<const unsigned*>(smem + w * L.wave_stride + L.hist)[t];
            if (s) __hip_atomic_fetch_add(k.hfx + (size_t)p * nr + t, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else if (k.hist_out) {
        const float hs = k.geo.hscale[p];
        for (int t = threadIdx.x; t < nr; t += blockDim.x) {
            float s = 0.f;
            for (int w = 0; w < kWaves; ++w) s += smem[w * L.wave_stride + L.hist + t];
            if (nsp > 1)
                k.hpart[((size_t)gsplit * k.geo.nwall + p) * nr + t] = s;
            else
                k.hist_out[(size_t)p * nr + t] = s * k.geo.att[t] * hs;
        }
    }
}

// TW: the twin drain (fx_twin_setup), the default of the no-occlusion FX forward
template <int PRESET, int MODE, bool DENSE, bool RAYS, bool CACHE, bool TAIL = false, bool FX = false, bool TW = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(6, 8))) void fwd_kernel(KArgs k) {
    fwd_body<PRESET, MODE, DENSE, RAYS, CACHE, TAIL, FX, false, TW>(k);
}
// FX bright launch (BR): the Gaussians whose amplitude bound reaches 2^kFxBits units (fx_blist_kernel), every
// segment added as u64 integers straight into the wall point's global row (kFxBits); usually an empty list
template <int PRESET, int MODE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(6, 8))) void fx_bright_kernel(KArgs k) {
    fwd_body<PRESET, MODE, false, false, false, true, true, true>(k);
}
// nlosgr_count_support's launch of the same body under its own name, so profiles tell it apart from the
// timed forward by identity
template <int PRESET, int MODE, bool DENSE, bool TAIL>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(6, 8))) void count_kernel(KArgs k) {
    fwd_body<PRESET, MODE, DENSE, false, false, TAIL, false>(k);
}

// forward Gaussian splits: hist[p,t] = (sum over splits in order) x att[t] x hscale[p]
__global__ __launch_bounds__(kBlock) void hist_reduce_kernel(const float* __restrict__ hpart, int nsp, long long P,
                                                             int nr, const float* __restrict__ att,
                                                             const float* __restrict__ hscale, float* __restrict__ hist) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P * nr) return;
    const long long p = i / nr;
    const int t = (int)(i - p * nr);
    float s = 0.f;
    for (int sp = 0; sp < nsp; ++sp) s += hpart[(size_t)sp * P * nr + i];
    hist[i] = s * att[t] * hscale[p];
}

// FX: each Gaussian's amplitude bound b_g = sigma_g * rho_max_g, rho_max = 0.5 + sum_l |f_l| sqrt((2l+1)/4pi)
// (Cauchy-Schwarz with sum_m Y_lm(d)^2 = (2l+1)/4pi on the unit sphere; 5 % margin for the cuda preset's
// eps-shortened view direction), counted into a histogram of binary exponents (float bits >> 23; a
// workgroup histogram in LDS first, then its non-empty bins into the global one).  Non-finite or zero
// bounds are not counted: a NaN Gaussian is skipped by the drains (w > 0 fails) and must not move the unit
// of the others; an infinite one takes the bright path (saturating, kFxBits).
template <int PRESET>
__global__ __launch_bounds__(kBlock) void fx_bound_kernel(nlosgr_gaussians g, float ascale, unsigned* bins,
                                                         float* bound) {
    __shared__ unsigned lh[kFxBins];
    lh[threadIdx.x] = 0u;
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < g.ng) {
        const float sig = 1.0f / (1.0f + expf(-g.opacity[i]));
        const float* f = g.features + (size_t)i * g.k_feat;
        const int deg = min(g.sh_degree, PRESET == NLOSGR_PRESET_TORCH ? 4 : 3);
        float sh = 0.f;
        for (int l = 0; l <= deg; ++l) {
            float n2 = 0.f;
            for (int c = l * l; c < (l + 1) * (l + 1) && c < g.k_feat; ++c) n2 += f[c] * f[c];
            sh += sqrtf(n2) * sqrtf((2.0f * l + 1.0f) * (0.25f / kPi));
        }
        const float a = sig * (0.5f + 1.05f * sh) * 1.001f * ascale;   // ascale: the mode's factor (netf: c dT)
        if (a > 0.f && a < 3.0e38f) atomicAdd(&lh[__float_as_uint(a) >> 23], 1u);
        // per Gaussian: 0 for NaN (skipped everywhere), +inf past the float range (the bright launch saturates)
        bound[i] = a >= 3.0e38f ? INFINITY : (a > 0.f ? a : 0.f);
    }
    __syncthreads();
    const unsigned c = lh[threadIdx.x];
    if (c) atomicAdd(bins + threadIdx.x, c);
}

// FX: the unit exponent from the bound histogram (one workgroup).  e_q = the largest exponent bin with at
// least ceil(n / 256) counted bounds at or above it (bin e holds bounds in [2^(e-127), 2^(e-126))), so
// fewer than ceil(n / 256) Gaussians have a bound above 2^(e_q - 126); E = kFxBits - (e_q - 126) puts that
// bound below 2^kFxBits units.  E <= E(top bin) + kFxRange.  info[0] = E, info[1] = E of the top bin.
__global__ __launch_bounds__(kFxBins) void fx_unit_kernel(const unsigned* __restrict__ bins, int* info, int maxunit,
                                                         int range) {
    __shared__ unsigned cum[kFxBins];
    const int t = threadIdx.x;
    cum[t] = bins[t];
    __syncthreads();
    for (int off = 1; off < kFxBins; off <<= 1) {   // suffix sums: cum[e] = sum_{e' >= e} bins[e']
        const unsigned v = t + off < kFxBins ? cum[t + off] : 0u;
        __syncthreads();
        cum[t] += v;
        __syncthreads();
    }
    const unsigned n = cum[0];
    const unsigned kq = (n + 255u) / 256u;
    // the largest e with cum[e] >= kq (resp. >= 1 for the top bin): cum is non-increasing in e
    const bool q = n > 0u && cum[t] >= kq && (t + 1 == kFxBins || cum[t + 1] < kq);
    const bool top = n > 0u && cum[t] >= 1u && (t + 1 == kFxBins || cum[t + 1] < 1u);
    __shared__ int eq, et;
    if (t == 0) { eq = 0; et = 0; }
    __syncthreads();
    if (q) eq = t;
    if (top) et = t;
    __syncthreads();
    if (t == 0) {
        auto unit = [](int e) { const int u = kFxBits - (e - 126); return u < -120 ? -120 : (u > 120 ? 120 : u); };
        const int emax = n > 0u ? unit(et) : 0;
        int e = n > 0u ? unit(maxunit ? et : eq) : 0;   // maxunit: round 5's rule (diagnostics)
        if (e > emax + range) e = emax + range;
        info[0] = e;
        info[1] = emax;
    }
}

// FX: the bright Gaussians (bound x 2^E x kFxMargin >= 2^kFxBits, the comparison of fwd_body) appended to a
// list (any order: the bright launch's sums are integers); info[4] = their number
__global__ __launch_bounds__(kBlock) void fx_blist_kernel(const float* __restrict__ bound, int ng, int* info, int* blist) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ng) return;
    const float fxS = ldexpf(1.0f, info[0]);
    if (!(bound[i] * fxS * kFxMargin < kFxBright)) blist[atomicAdd(info + 4, 1)] = i;
}

// FX: hist[p,t] = (u64 count x 2^-E) x att[t] x hscale[p]
__global__ __launch_bounds__(kBlock) void fx_reduce_kernel(const unsigned long long* __restrict__ hfx,
                                                           const int* __restrict__ info, long long P, int nr,
                                                           const float* __restrict__ att,
                                                           const float* __restrict__ hscale, float* __restrict__ hist) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P * nr) return;
    const long long p = i / nr;
    const int t = (int)(i - p * nr);
    const double q = ldexp(1.0, -info[0]);
    hist[i] = (float)((double)hfx[i] * q) * att[t] * hscale[p];
}

// Dense no-occlusion forward (cutoff <= 0: every Gaussian at every sample, the reference's own
// support): every ray covers every bin, so the lane-serial drain above degenerates (all segments
// claim the same bins; read-add-write chains bound by LDS latency).  Here lane = bin instead: a
// wave walks its live pairs one at a time, computes 64 rays of the pair lane-parallel (lane = ray),
// stages their (gamma, alpha, ks) in LDS and then, ray by ray (LDS broadcast), every lane adds the
// exact value of its NB bins (k = lane + 64 b) into register accumulators.  No LDS writes in the
// inner loop, no claims, fixed summation order (deterministic).
struct FwdDenseLayout {
    int rays, hist, total;   // offsets in floats after the float2 angle tables
    __host__ __device__ FwdDenseLayout(int nr, int nt, int np_) {
        const int off = al4(2 * (nt + np_));
        rays = off;                     // float4 [kWaves][64] (gamma, alpha, ks, -)
        hist = rays + kWaves * 64 * 4;  // double [kWaves][nr]
        total = hist + kWaves * nr * 2;
    }
};

template <int PRESET, int NB>
__global__ __launch_bounds__(kBlock) void fwd_dense_kernel(KArgs k) {
    extern __shared__ __align__(16) float smem[];
    const int nr = k.geo.nr, nt = k.geo.nt, np_ = k.geo.np;
    const FwdDenseLayout L(nr, nt, np_);
    float2* tth = reinterpret_cast<float2*>(smem);
    float2* tph = tth + nt;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();   // wave-uniform (SGPR)
    float4* rp = reinterpret_cast<float4*>(smem + L.rays) + wave * 64;
    const int p = blockIdx.x;
    const int gsplit = blockIdx.y, nsp = gridDim.y;
    const int gper = (((k.g.ng + nsp - 1) / nsp) + 63) & ~63;
    const int g_lo = gsplit * gper, g_hi = min(k.g.ng, g_lo + gper);
    for (int t = threadIdx.x; t < nt; t += blockDim.x)
        tth[t] = make_float2(k.geo.sin_theta[(size_t)p * nt + t], k.geo.cos_theta[(size_t)p * nt + t]);
    for (int t = threadIdx.x; t < np_; t += blockDim.x)
        tph[t] = make_float2(k.geo.cos_phi[(size_t)p * np_ + t], k.geo.sin_phi[(size_t)p * np_ + t]);
    __syncthreads();

    const float px = k.geo.wall[3 * p], py = k.geo.wall[3 * p + 1], pz = k.geo.wall[3 * p + 2];
    const float* lin = k.geo.grid_lin + 4 * (size_t)p;
    const float r0 = k.geo.r[0];
    const float dr = nr > 1 ? (k.geo.r[nr - 1] - r0) / (float)(nr - 1) : 0.f;
    const float inv_dr = dr > 0.f ? 1.0f / dr : 0.f;
    const int nray = nt * np_;
    // each 64-ray batch's terms are summed in fp32 registers (<= 64 terms per bin) and folded into the
    // lane's own bins of a wave-private fp64 histogram: a running fp32 total over every (Gaussian, ray)
    // drops the terms below half an ulp of the bin (C2: 1.9e-5 low against float64)
    double* wh = reinterpret_cast<double*>(smem + L.hist) + wave * nr;
    float kf[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        kf[b] = (float)(lane + 64 * b);
        if (lane + 64 * b < nr) wh[lane + 64 * b] = 0.0;
    }

    for (int base = g_lo + wave * 64; base < g_hi; base += kBlock) {
        const int gi = base + lane;
        Pair P;
        float lw = 0.f;
        bool live = false;
        {
            const int gl = min(gi, k.g.ng - 1);
            const GaussRec rec = k.recs[gl];
            float mu[3];
            load_rec(rec, P, mu);
            pair_setup<PRESET, true>(k, k.g.features + (size_t)gl * k.g.k_feat, mu, px, py, pz, lin, 0.f, P);
            live = gi < g_hi && P.w > 0.f;
            lw = live ? flog2(P.w) : 0.f;
        }
        unsigned long long lm = __builtin_amdgcn_ballot_w64(live);
        while (lm) {   // wave-uniform walk over the chunk's live pairs
            const int sl = (int)__builtin_ctzll(lm);
            lm &= lm - 1ull;
            float A[9], u0[3];
#pragma unroll
            for (int c = 0; c < 9; ++c) A[c] = __shfl(P.A[c], sl);
#pragma unroll
            for (int c = 0; c < 3; ++c) u0[c] = __shfl(P.u0[c], sl);
            const float lws = __shfl(lw, sl);
            for (int rb = 0; rb < nray; rb += 64) {
                const int ray = min(rb + lane, nray - 1);
                const int i = ray / np_, j = ray - i * np_;
                const float2 th = tth[i], ph = tph[j];
                Ray R;
                ray_setup<true>(A, u0, th.x * ph.x, th.x * ph.y, th.y, 0.f, r0, inv_dr, nr, R);
                const float ga = -kHalfLog2e * R.a * dr * dr;
                const float al = fmaf(-kHalfLog2e, R.m2min, lws) + flog2(th.x);
                wave_sync();   // the previous batch's broadcasts are done
                rp[lane] = make_float4(ga, al, R.ks, 0.f);
                wave_sync();
                const int nq = min(64, nray - rb);
                float acc[NB];
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[b] = 0.f;
                int q = 0;
                for (; q + 4 <= nq; q += 4) {
                    float4 e[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) e[u] = rp[q + u];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int b = 0; b < NB; ++b) {
                            const float t = kf[b] - e[u].z;
                            acc[b] += fast_exp2(fmaf(e[u].x, t * t, e[u].y));
                        }
                }
                for (; q < nq; ++q) {
                    const float4 e = rp[q];
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const float t = kf[b] - e.z;
                        acc[b] += fast_exp2(fmaf(e.x, t * t, e.y));
                    }
                }
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    if (lane + 64 * b < nr) wh[lane + 64 * b] += (double)acc[b];
            }
        }
    }
    __syncthreads();
    const float hs = k.geo.hscale[p];
    const double* whs = reinterpret_cast<const double*>(smem + L.hist);
    for (int t = threadIdx.x; t < nr; t += blockDim.x) {
        double sd = 0.0;
        for (int w = 0; w < kWaves; ++w) sd += whs[w * nr + t];
        const float s = (float)sd;
        if (nsp > 1)
            k.hpart[((size_t)gsplit * k.geo.nwall + p) * nr + t] = s;
        else
            k.hist_out[(size_t)p * nr + t] = s * k.geo.att[t] * hs;
    }
}

template <int PRESET, int MODE, bool DENSE, bool RAYS, bool CACHE>
void launch_fwd(const KArgs& ka, size_t shm, hipStream_t s) {
    const dim3 grid(ka.geo.nwall, (ka.hpart || ka.hfx) ? ka.nfsplit : 1);
    if constexpr ((MODE == NLOSGR_MODE_NOOCL || MODE == NLOSGR_MODE_NETF || MODE == NLOSGR_MODE_BININT) && !DENSE &&
                  !RAYS && !CACHE) {
        if (ka.hfx) {   // run_fwd decided the fixed-point TAIL drain (fx_eligible)
            // the no-occlusion drain takes two adjacent rays of a pair per lane (NLOSGR_FLAG_FX_NOTWIN: one)
            bool twin = false;
            if constexpr (MODE == NLOSGR_MODE_NOOCL && kFxPerm) {
                twin = !(ka.opt.flags & NLOSGR_FLAG_FX_NOTWIN);
                if (twin)
                    hipLaunchKernelGGL((fwd_kernel<PRESET, MODE, DENSE, RAYS, CACHE, true, true, true>), grid, dim3(kBlock), shm, s, ka);
            }
            if (!twin)
                hipLaunchKernelGGL((fwd_kernel<PRESET, MODE, DENSE, RAYS, CACHE, true, true>), grid, dim3(kBlock), shm, s, ka);
            // the bright Gaussians' launch (one split per wall point; its list is usually empty)
            hipLaunchKernelGGL((fx_bright_kernel<PRESET, MODE>), dim3(ka.geo.nwall, 1), dim3(kBlock), shm, s, ka);
            return;
        }
    }
    constexpr bool kCanTail = (MODE == NLOSGR_MODE_NOOCL || MODE == NLOSGR_MODE_NETF || MODE == NLOSGR_MODE_BININT) &&
                              !DENSE && !RAYS;
    // NLOSGR_FLAG_MASKED_FWD: masked forward drain at every cutoff (A/B and parity cross-check); netf takes
    // the TAIL drain where its backward does (c dT <= 1/64), so both see the same support
    const bool tail = kCanTail && ka.opt.cutoff >= kTailCutoff && (!ka.counts || NLOSGR_FCOUNT_ON) &&
                      !(ka.opt.flags & NLOSGR_FLAG_MASKED_FWD) &&
                      (MODE != NLOSGR_MODE_NETF || ka.opt.c_deltaT <= kSmallX);
    if constexpr (!RAYS && !CACHE) {
        if (ka.counts) {   // nlosgr_count_support
            if (tail) hipLaunchKernelGGL((count_kernel<PRESET, MODE, DENSE, kCanTail>), grid, dim3(kBlock), shm, s, ka);
            else hipLaunchKernelGGL((count_kernel<PRESET, MODE, DENSE, false>), grid, dim3(kBlock), shm, s, ka);
            return;
        }
    }
    if (tail) hipLaunchKernelGGL((fwd_kernel<PRESET, MODE, DENSE, RAYS, CACHE, kCanTail>), grid, dim3(kBlock), shm, s, ka);
    else hipLaunchKernelGGL((fwd_kernel<PRESET, MODE, DENSE, RAYS, CACHE>), grid, dim3(kBlock), shm, s, ka);
}

// the ray cache is used only by the culled, histogram-only variants (the training hot path)
template <int PRESET, int MODE>
void dispatch_fwd(const KArgs& ka, bool dense, bool rays, size_t shm, hipStream_t s) {
    if (dense) {
        if (rays) launch_fwd<PRESET, MODE, true, true, false>(ka, shm, s);
        else launch_fwd<PRESET, MODE, true, false, false>(ka, shm, s);
    } else {
        if (rays) launch_fwd<PRESET, MODE, false, true, false>(ka, shm, s);
        else if (ka.cmask && MODE != NLOSGR_MODE_BININT) launch_fwd<PRESET, MODE, false, false, MODE != NLOSGR_MODE_BININT>(ka, shm, s);
        else launch_fwd<PRESET, MODE, false, false, false>(ka, shm, s);
    }
}

}  // namespace

namespace nlosgr {
namespace detail {

int volume_fx_prepare(const KArgs& ka, unsigned* bins, float* bound, int* blist, hipStream_t s) {
    const nlosgr_gaussians* g = &ka.g;
    const nlosgr_geometry* geo = &ka.geo;
    const nlosgr_options* opt = &ka.opt;
    HIPCHK(hipMemsetAsync(ka.hfx, 0, (size_t)geo->nwall * geo->nr * sizeof(unsigned long long), s));
    HIPCHK(hipMemsetAsync(bins, 0, kFxBins * sizeof(unsigned) + kFxInfoWords * sizeof(int), s));
    const int nb = (g->ng + kBlock - 1) / kBlock;
    const float ascale = opt->mode == NLOSGR_MODE_NETF ? opt->c_deltaT : 1.0f;
    if (g->preset == NLOSGR_PRESET_TORCH)
        hipLaunchKernelGGL(fx_bound_kernel<NLOSGR_PRESET_TORCH>, dim3(nb), dim3(kBlock), 0, s, *g, ascale, bins, bound);
    else
        hipLaunchKernelGGL(fx_bound_kernel<NLOSGR_PRESET_CUDA>, dim3(nb), dim3(kBlock), 0, s, *g, ascale, bins, bound);
    HIPCHK(hipGetLastError());
    // E <= E(max) + range: a bright term < 2^(kFxBits + range) units, and a bin receives at most
    // ceil(ng / 256) x nt x np bright terms per wall point, so its u64 sum stays below 2^63
    int range = kFxRange;
    {
        const double nterm = (double)((g->ng + 255) / 256) * (double)geo->nt * (double)geo->np;
        int bits = 0;
        while (bits < 63 && ldexp(1.0, bits) < nterm) ++bits;
        range = 63 - kFxBits - bits;
        range = range < 0 ? 0 : (range > kFxRange ? kFxRange : range);
    }
    hipLaunchKernelGGL(fx_unit_kernel, dim3(1), dim3(kFxBins), 0, s, bins, ka.fx_info,
                       (opt->flags & NLOSGR_FLAG_FX_MAXUNIT) ? 1 : 0, range);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(fx_blist_kernel, dim3(nb), dim3(kBlock), 0, s, bound, g->ng, ka.fx_info, blist);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

int volume_fwd(const KArgs& ka, hipStream_t s) {
    const nlosgr_gaussians* g = &ka.g;
    const nlosgr_geometry* geo = &ka.geo;
    const nlosgr_options* opt = &ka.opt;
    float* hist_out = ka.hist_out;
    const bool dense = !(opt->cutoff > 0.f);
    const bool rays = ka.ray_out != nullptr;
    const size_t shm = (size_t)FwdLayout(geo->nr, geo->nt, geo->np, ka.hfx != nullptr).total * sizeof(float);
    // NLOSGR_FLAG_LANE_DENSE routes the dense histogram through fwd_kernel instead (parity cross-check)
    if (dense && !rays && !ka.counts && hist_out && opt->mode == NLOSGR_MODE_NOOCL && geo->nr <= 1024 &&
        !(opt->flags & NLOSGR_FLAG_LANE_DENSE)) {
        // dense no-occlusion histogram: lane = bin register accumulation (fwd_dense_kernel)
        if (g->ng > 0 && geo->nwall > 0) {
            const size_t shd = (size_t)FwdDenseLayout(geo->nr, geo->nt, geo->np).total * sizeof(float);
            const dim3 grid(geo->nwall, ka.hpart ? ka.nfsplit : 1);
            const int nb = (geo->nr + 63) / 64;
            const bool tp = g->preset == NLOSGR_PRESET_TORCH;
#define NLOSGR_FD(NBV)                                                                                   \
    do {                                                                                                 \
        if (tp) hipLaunchKernelGGL((fwd_dense_kernel<0, NBV>), grid, dim3(kBlock), shd, s, ka);          \
        else hipLaunchKernelGGL((fwd_dense_kernel<1, NBV>), grid, dim3(kBlock), shd, s, ka);             \
    } while (0)
            if (nb <= 1) NLOSGR_FD(1);
            else if (nb <= 2) NLOSGR_FD(2);
            else if (nb <= 4) NLOSGR_FD(4);
            else if (nb <= 8) NLOSGR_FD(8);
            else NLOSGR_FD(16);
#undef NLOSGR_FD
            HIPCHK(hipGetLastError());
        } else if (geo->nwall > 0) {
            HIPCHK(hipMemsetAsync(hist_out, 0, (size_t)geo->nwall * geo->nr * sizeof(float), s));
        }
    } else if (g->preset == NLOSGR_PRESET_TORCH) {
        if (opt->mode == NLOSGR_MODE_NOOCL) dispatch_fwd<0, 0>(ka, dense, rays, shm, s);
        else if (opt->mode == NLOSGR_MODE_NETF) dispatch_fwd<0, 1>(ka, dense, rays, shm, s);
        else dispatch_fwd<0, 2>(ka, dense, rays, shm, s);
    } else {
        if (opt->mode == NLOSGR_MODE_NOOCL) dispatch_fwd<1, 0>(ka, dense, rays, shm, s);
        else if (opt->mode == NLOSGR_MODE_NETF) dispatch_fwd<1, 1>(ka, dense, rays, shm, s);
        else dispatch_fwd<1, 2>(ka, dense, rays, shm, s);
    }
    HIPCHK(hipGetLastError());
    if (ka.hfx) {
        const long long n = (long long)geo->nwall * geo->nr;
        hipLaunchKernelGGL(fx_reduce_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, ka.hfx,
                           ka.fx_info, (long long)geo->nwall, geo->nr, geo->att, geo->hscale, hist_out);
        HIPCHK(hipGetLastError());
    } else if (ka.hpart) {
        const long long n = (long long)geo->nwall * geo->nr;
        hipLaunchKernelGGL(hist_reduce_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, ka.hpart,
                           ka.nfsplit, (long long)geo->nwall, geo->nr, geo->att, geo->hscale, hist_out);
        HIPCHK(hipGetLastError());
    }
    return NLOSGR_OK;
}

}  // namespace detail
}  // namespace nlosgr

#ifdef NLOSGR_FXCOUNT
extern "C" __attribute__((visibility("default"))) int nlosgr_debug_fx_counts(unsigned long long* out12) {
    if (hipMemcpyFromSymbol(out12, HIP_SYMBOL(g_fdbg), 12 * sizeof(unsigned long long)) != hipSuccess) return -1;
    const unsigned long long zero[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_fdbg), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}
#endif
