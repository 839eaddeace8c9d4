// Transient Gaussian NLOS renderer, pair-major volume path: what its forward (nlosgr_volume_fwd.hip), its
// backward (nlosgr_volume_bwd.hip) and the host side (nlosgr_volume.hip) share, and the kernel files' entry points.
//
// Hot path: for every relay-wall point p and time bin k
//     hist[p,k] = hscale[p] * att[k] * sum_g w_g(p) sum_{i,j} sin(theta_i) pdf_g(p + r_k d_ij)
// (no-occlusion) or the per-Gaussian self-transmittance variant ('netf').
//
// Algebra that makes the inner loop cheap: with u0 = A(p - mu) and v = A d_ij the whitened
// offset along ray ij is u(r) = u0 + r v, a straight line, so each (pair, ray) is a 1-D
// Gaussian in r:  pdf(r) = exp(-(m2min + a (r - t*)^2) / 2),  a = |v|^2, t* = -(u0.v)/a,
// m2min = |u0 + t* v|^2.  The support |u| <= m_c is
//   * per pair: a cone of rays (bounding-sphere test -> (theta, phi) index box), then
//   * per ray:  the quadric d^T M d >= 0,  M = (A^T u0)(A^T u0)^T - (|u0|^2 - m_c^2) A^T A
//               (exactly m2min <= m_c^2), then
//   * per ray:  one contiguous bin range [kl, kh] (a "segment").
#pragma once
#include "nlosgr_common.hpp"

namespace nlosgr {
namespace detail {

// constants of the workspace layout (VolumeWs, nlosgr_volume.hip)
constexpr int kPartStride = 32;       // floats per row of the backward partials (kBwdSlots used)
constexpr int kCacheMaskBytes = 16;   // ray cache, per pair: the cell mask (ulonglong2),
constexpr int kCacheBoxBytes = 4;     //   the box word (cache_box)
constexpr int kCacheRhoBytes = 4;     //   and the albedo rho
constexpr int kDiagTailBytes = 256;   // diagnostics counters of the backward (kFlagDiagCounters)
constexpr int kFlagDiagCounters = 8;  // nlosgr_options.flags: the backward gets the diagnostics tail as counts
constexpr int kFxBins = 256;          // FX bound histogram: one bin per binary exponent (float bits >> 23)
constexpr int kFxInfoWords = 8;       // FX info words (KArgs::fx_info), after the bound histogram
constexpr int kFxTailBytes = 2048;    // FX tail of the workspace: bins u32 [kFxBins] | info int [kFxInfoWords]

struct KArgs {
    nlosgr_gaussians g;
    nlosgr_geometry geo;
    nlosgr_options opt;
    const GaussRec* recs;
    float* hist_out;
    float* ray_out;
    const float* grad_hist;
    const float* grad_ray;
    float* partial;  // [nsplit][ng][kPartStride]
    int nsplit;
    unsigned long long* counts;  // optional [3]: pairs, segments, samples (nlosgr_count_support)
    ulonglong2* cmask;           // ray cache [P][ng]: passing rays of the pair's box (bit = box cell)
    float* drho;                 // backward: dL/drho per pair [P][ng] (0 outside the support) -> sh_kernel
    float* hpart;                // forward Gaussian-split partial histograms [nfsplit][P][nr]
    float* shpart;               // sh_kernel partials [nsh][ng][kShPart]
    int nsh;                     // sh_kernel wall-point splits
    int nfsplit;                 // forward Gaussian splits per wall point (hpart != null)
    int bshared;                 // backward: 4 waves share each wall point's staged row (bwd_shared)
    unsigned* cbox;              // ray cache [P][ng]: i0 | j0 << 12 | width << 24, 0 = not cached
    float* crho;                 // ray cache [P][ng]: the pair's SH albedo rho (1)
    int g_lo, g_hi;              // backward: Gaussians [g_lo, g_hi) (one bucket of the gradient all-reduce)
    int pb0, pnw;                // backward: wall points [pb0, pb0 + pnw) of this launch (a batch; drho rows
                                 // are indexed p - pb0, so the dL/drho buffer holds one batch, not the wall)
    int accum;                   // backward batches after the first add into the partial slabs
    unsigned long long* hfx;     // forward FX drain: fixed-point histogram [P][nr] (u64, integer adds)
    int* fx_info;                // forward FX drain: [0] unit exponent E (fx_unit_kernel), [1] E of the launch's
                                 // largest bound, [2] LDS flushes, [3] bright segments, [4] bright Gaussians,
                                 // [5] groups of two or more rays drained as one segment, [6] groups split
                                 // (fx_twin_setup), [7] the longest group in bins (NLOSGR_FLAG_FX_TWIN_STATS)
    const float* fx_bound;       // forward FX drain: amplitude bound per Gaussian [ng] (fx_bound_kernel)
    const int* fx_blist;         // forward FX drain: the bright Gaussians (fx_blist_kernel), [fx_info[4]]
};

// ray cache: a pair whose (theta, phi) candidate box has at most 128 cells records which cells
// passed the quadric test in the forward; the backward walks those bits instead of re-testing
// (C3: 99.9% of pairs; the rest are re-enumerated)
constexpr int kCacheCells = 128;
__device__ __forceinline__ unsigned cache_box(int i0, int j0, int w) {
    return (unsigned)i0 | ((unsigned)j0 << 12) | ((unsigned)w << 24);
}

// atan2 with |error| < 2e-6 rad (minimax on [0,1] + octant reduction); used only for the
// conservative footprint box, which is widened by kAngMargin.
__device__ __forceinline__ float fast_atan2(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float a = mx > 0.f ? mn * frcp(mx) : 0.f;
    const float s = a * a;
    float r = fmaf(s, -0.01172120f, 0.05265332f);
    r = fmaf(s, r, -0.11643287f);
    r = fmaf(s, r, 0.19354346f);
    r = fmaf(s, r, -0.33262347f);
    r = fmaf(s, r, 0.99997726f);
    r *= a;
    if (ay > ax) r = 1.57079632679f - r;
    if (x < 0.f) r = kPi - r;
    return y < 0.f ? -r : r;
}
constexpr float kAngMargin = 1e-4f;

// kRecurrence: along a segment the log2 value is quadratic in the bin offset t, e(t) = ga t^2 + al,
// so value(t+1) = value(t) * 2^(ga (2t+1)) and that ratio itself scales by 2^(2 ga) per bin.  The
// culled drains (forward and backward, no-occlusion) re-seed value and ratio with exact exp2 once
// per kSteps-bin round and multiply in between: relative error <= kSteps ulp.  Inside the support
// |ga| t^2 <= m_c^2 log2(e) / 2, which bounds |ga (2t+1)| by m_c^2 log2(e) (<= 47 at m_c = 5.7),
// so the ratio never overflows; past the segment end both factors only shrink (no inf * 0).
// Dense mode (unbounded t) keeps the per-bin exp2.

// launch-uniform choices both directions make alike, so that they see the same support
constexpr float kSmallX = 1.0f / 64.0f;   // netf: c dT up to which the transmittance factor needs no exp
constexpr float kTf0 = 1.0f + 1e-7f;   // the netf transmittance factor's constant, exp(0) + 1e-7 in float
constexpr float kTailCutoff = 5.0f;       // cutoff from which the culled histogram drains run without an end mask (TAIL)

// ------------------------------------------------------------------------------------------
// per-(wall point, Gaussian) pair state
// ------------------------------------------------------------------------------------------
struct Pair {
    float A[9], sigma, smax, N[6];
    float q[3];         // p - mu
    float u0[3];        // A (p - mu)
    float dir[3], nrm;  // view direction of mu - p (preset convention)
    float sh, rho, w;
    float M[6];         // quadric (M00, 2M01, 2M02, M11, 2M12, M22)
    int i0, i1, j0, j1;
};

__device__ __forceinline__ void load_rec(const GaussRec& r, Pair& P, float mu[3]) {
    mu[0] = r.a.x; mu[1] = r.a.y; mu[2] = r.a.z; P.sigma = r.a.w;
    P.A[0] = r.b.x; P.A[1] = r.b.y; P.A[2] = r.b.z; P.A[3] = r.b.w;
    P.A[4] = r.c.x; P.A[5] = r.c.y; P.A[6] = r.c.z; P.A[7] = r.c.w;
    P.A[8] = r.d.x; P.smax = r.d.y; P.N[0] = r.d.z; P.N[1] = r.d.w;
    P.N[2] = r.e.x; P.N[3] = r.e.y; P.N[4] = r.e.z; P.N[5] = r.e.w;
}

// Trimmed support of the no-occlusion FX forward (NLOSGR_FLAG_FX_TRIM).  That drain rounds every term to the
// nearest unit 2^-E, and its twin lanes round the SUM of two rays' terms, so a term below a quarter unit adds
// exactly 0.  With lw = log2(w 2^E) the value at Mahalanobis distance m is 2^(lw + log2 sin(theta) - m^2 log2(e) / 2)
// <= 2^(lw - m^2 log2(e) / 2) (sin(theta) <= 1 is ignored), which is below 2^-(2 + kTrimMargin) units for
// m^2 > 2 ln 2 (lw + 2 + kTrimMargin): the pair's support radius is the smaller of that and the cutoff.
// kTrimMargin widens the radius by what the kernel's own value of a dropped term can exceed the exact one,
// in log2: the recurrence's drift within a round, <= kStepsTwin ulp = 36 x 1.2e-7 relative (kRecurrence), 6.2e-6;
// v_log_f32 and v_exp_f32, 1 ulp each, 3.8e-6 of an |lw| <= 32 and 1.7e-7; about ten fp32 roundings of exponent
// terms below 64 (half an ulp each, 3.8e-6), 4e-5; v_rcp / v_sqrt in the half width hk (2 ulp of hk^2, times
// |ga| hk^2 <= m_c^2 log2(e) / 2 = 23.4), 1.1e-5; and the rounding of ks - hk before ceil / floor pick the end
// bins, which moves the edge by up to ulp(ks) / 2 = 2.4e-4 bins at ks < 4096 (validate: nr <= 4096), 2 |ga| hk
// = 46.9 / hk per bin of it, 1.14e-2 for a ray at least one bin wide each side.  Sum 1.15e-2 < 2^-6.  (A ray
// narrower than a bin whose edge lies within ulp(ks) of a bin centre is decided either way by that rounding,
// as it is at the cutoff itself.)  Every decision with the margin is conservative: it only keeps more.
constexpr float kTrimMargin = 0.015625f;             // 2^-6, log2
constexpr float kTrim = 1.38629436111989062f;        // 2 ln 2
constexpr float kTrimQuarter = 2.0f + kTrimMargin;   // a pair with lw + kTrimQuarter <= 0 peaks below a quarter unit
__device__ __forceinline__ float fx_trim_m2(float lw, float mc2) {
    return fminf(mc2, kTrim * (lw + kTrimQuarter));   // (add and multiply by literals: no constant held in a VGPR)
}

// f: the Gaussian's feature row (k_feat floats; registers or global).  TRIM (the no-occlusion FX forward) with
// trim set: the quadric and the box take the pair's trimmed radius (fx_trim_m2 of log2(w) + fxE) for the cutoff
template <int PRESET, bool DENSE, bool TRIM = false>
__device__ __forceinline__ void pair_setup(const KArgs& k, const float* f, const float mu[3], float px, float py,
                                           float pz, const float* lin, float mc2, Pair& P, float fxE = 0.f,
                                           bool trim = false) {
    P.q[0] = px - mu[0]; P.q[1] = py - mu[1]; P.q[2] = pz - mu[2];
    for (int r = 0; r < 3; ++r) P.u0[r] = P.A[3 * r] * P.q[0] + P.A[3 * r + 1] * P.q[1] + P.A[3 * r + 2] * P.q[2];
    view_dir<PRESET>(-P.q[0], -P.q[1], -P.q[2], P.dir[0], P.dir[1], P.dir[2], P.nrm);
    const float sh = sh_dot<PRESET>(k.g.sh_degree, P.dir[0], P.dir[1], P.dir[2], f);
    P.sh = sh;
    P.rho = fmaxf(sh + 0.5f, 0.0f);
    P.w = P.sigma * P.rho;
    const int nt = k.geo.nt, np_ = k.geo.np;
    P.i0 = 0; P.i1 = nt - 1; P.j0 = 0; P.j1 = np_ - 1;
    if (DENSE) return;
    // quadric cone: d^T M d >= 0  <=>  m2min(d) <= m_c^2
    const float wv0 = P.A[0] * P.u0[0] + P.A[3] * P.u0[1] + P.A[6] * P.u0[2];
    const float wv1 = P.A[1] * P.u0[0] + P.A[4] * P.u0[1] + P.A[7] * P.u0[2];
    const float wv2 = P.A[2] * P.u0[0] + P.A[5] * P.u0[1] + P.A[8] * P.u0[2];
    float mp2 = mc2, mcut = k.opt.cutoff;
    if (TRIM && trim) {   // (w <= 0 or NaN: the caller skips such a pair whatever its radius)
        mp2 = fmaxf(fx_trim_m2(flog2(P.w) + fxE, mc2), 0.f);
        mcut = fsqrt(mp2);
    }
    const float kap = P.u0[0] * P.u0[0] + P.u0[1] * P.u0[1] + P.u0[2] * P.u0[2] - mp2;
    P.M[0] = wv0 * wv0 - kap * P.N[0];
    P.M[1] = 2.0f * (wv0 * wv1 - kap * P.N[1]);
    P.M[2] = 2.0f * (wv0 * wv2 - kap * P.N[2]);
    P.M[3] = wv1 * wv1 - kap * P.N[3];
    P.M[4] = 2.0f * (wv1 * wv2 - kap * P.N[4]);
    P.M[5] = wv2 * wv2 - kap * P.N[5];
    // bounding-sphere cone -> (theta, phi) index box (angles via one fast atan2, widened by a margin)
    const float Rb = mcut * P.smax * 1.0001f + 1e-7f;
    const float dx = -P.q[0], dy = -P.q[1], dz = -P.q[2];
    const float rxy2 = dx * dx + dy * dy;
    const float dist2 = rxy2 + dz * dz;
    const float Rb2 = Rb * Rb;
    if (dist2 <= Rb2) return;
    const float rxy = fsqrt(rxy2);
    const float alpha = fast_atan2(Rb, fsqrt(dist2 - Rb2)) + kAngMargin;       // asin(Rb / dist)
    const float thc = fast_atan2(rxy, dz);                                     // acos(dz / dist)
    const float th0 = lin[0], dth = lin[1], ph0 = lin[2], dph = lin[3];
    if (dth > 0.f) {
        const float idth = frcp(dth);
        // samples are points (theta_i = th0 + i dth): the box holds exactly the samples inside the
        // margin-widened cap range, [ceil(lo), floor(hi)] (floor/ceil added one outside row per side)
        P.i0 = fidx(ceilf((thc - alpha - th0) * idth), 0, nt - 1);
        P.i1 = fidx(floorf((thc + alpha - th0) * idth), -1, nt - 1);
    }
    if (thc - alpha > 1e-3f && thc + alpha < kPi - 1e-3f && dph > 0.f) {
        // max |phi - phi_c| on the cone = asin(sin(alpha) / sin(theta_c))
        const float sa = Rb * frcp(fsqrt(dist2));
        const float sth = rxy * frcp(fsqrt(dist2));
        const float ratio = sa * frcp(sth);
        if (ratio < 0.999f) {
            const float dphi = fast_atan2(ratio, fsqrt(1.0f - ratio * ratio)) + kAngMargin;
            const float phc = fast_atan2(dy, dx);
            const float lo = phc - dphi, hi = phc + dphi;
            if (lo > -kPi && hi < kPi) {
                const float idph = frcp(dph);
                P.j0 = fidx(ceilf((lo - ph0) * idph), 0, np_ - 1);
                P.j1 = fidx(floorf((hi - ph0) * idph), -1, np_ - 1);
            }
        }
    }
}

// feature row -> registers (zero past k_feat)
template <int KM>
__device__ __forceinline__ void load_feat(const nlosgr_gaussians& g, int gi, float* f) {
    const float* src = g.features + (size_t)gi * g.k_feat;
    if (KM % 4 == 0 && g.k_feat == KM && (reinterpret_cast<uintptr_t>(g.features) & 15) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
        for (int c = 0; c < KM / 4; ++c) {
            const float4 v = s4[c];
            f[4 * c] = v.x; f[4 * c + 1] = v.y; f[4 * c + 2] = v.z; f[4 * c + 3] = v.w;
        }
        return;
    }
#pragma unroll
    for (int c = 0; c < KM; ++c) f[c] = c < g.k_feat ? src[c] : 0.f;
}

__device__ __forceinline__ float quadric(const float* M, float dx, float dy, float dz) {
    const float t0 = fmaf(M[0], dx, fmaf(M[1], dy, M[2] * dz));
    const float t1 = fmaf(M[3], dy, M[4] * dz);
    return fmaf(dx, t0, fmaf(dy, t1, dz * dz * M[5]));
}

// Ray quantities: v = A d, a = |v|^2, t*, z* = u0 + t* v, m2min, in-support bin range, and
// ks = the (fractional) bin of the closest approach.
struct Ray {
    float v[3], a, ts, zs[3], m2min, ks;
    int kl, kh;
};

template <bool DENSE>
__device__ __forceinline__ bool ray_setup(const float* A, const float* u0, float dx, float dy, float dz, float mc2,
                                          float r0, float inv_dr, int nr, Ray& R) {
    for (int r = 0; r < 3; ++r) R.v[r] = A[3 * r] * dx + A[3 * r + 1] * dy + A[3 * r + 2] * dz;
    R.a = R.v[0] * R.v[0] + R.v[1] * R.v[1] + R.v[2] * R.v[2];
    const float b = u0[0] * R.v[0] + u0[1] * R.v[1] + u0[2] * R.v[2];
    const float ia = frcp(R.a);
    R.ts = -b * ia;
    for (int r = 0; r < 3; ++r) R.zs[r] = u0[r] + R.ts * R.v[r];
    R.m2min = R.zs[0] * R.zs[0] + R.zs[1] * R.zs[1] + R.zs[2] * R.zs[2];
    R.ks = (R.ts - r0) * inv_dr;
    if (DENSE) {
        R.kl = 0; R.kh = nr - 1;
        return true;
    }
    if (!(R.m2min <= mc2)) return false;
    const float hk = fsqrt((mc2 - R.m2min) * ia) * inv_dr;
    R.kl = fidx(ceilf(R.ks - hk), 0, nr);
    R.kh = fidx(floorf(R.ks + hk), -1, nr - 1);
    return R.kl <= R.kh;
}

// LDS carve helper (offsets in floats, 16-byte aligned)
__host__ __device__ __forceinline__ int al4(int n) { return (n + 3) & ~3; }

// ray queue ring per wave: < 64 queued + up to 64 (small ring) or 128 appended per enumeration
constexpr int kRQ = 256;
__device__ __forceinline__ unsigned pack_ray(int slot, int i, int j) {
    return (unsigned)slot | ((unsigned)i << 8) | ((unsigned)j << 20);
}

// Candidate enumeration (lane = pair): quadric test only; passing (pair, ray) entries are appended
// to the ray queue ring at qbase + cnt.  Branch-free body (every lane evaluates a clamped
// candidate, `more` masks the result), two candidates per trip so their table reads overlap;
// returns once cnt >= 64 or every lane exhausted its box (cnt < 64 + 2*64 <= kRQ on return).
template <bool DENSE, bool REC = false>
__device__ __forceinline__ void enumerate_box(const float* M, int i1, int j0, int j1, bool& more, int& ci, int& cj,
                                              const float2* tth, const float2* tph, int nt1, unsigned* rayq,
                                              int qbase, int& cnt, unsigned long long* rec0 = nullptr,
                                              unsigned long long* rec1 = nullptr, int* cell = nullptr) {
    constexpr int NC = 3;
    static_assert(NC >= 1 && 64 + NC * 64 <= kRQ, "enumeration would overflow the ray queue ring");
    const int lane = lane_id();
    do {
        // NC consecutive cells of the box (row-major): all table reads are issued before any queue
        // store (an LDS store in between would order them), the tests are unpredicated
        int cis[NC], cjs[NC];
        bool mores[NC];
        cis[0] = ci; cjs[0] = cj; mores[0] = more;
#pragma unroll
        for (int u = 1; u < NC; ++u) {
            const bool wrap = cjs[u - 1] >= j1;
            cis[u] = cis[u - 1] + (wrap ? 1 : 0);
            cjs[u] = wrap ? j0 : cjs[u - 1] + 1;
            mores[u] = mores[u - 1] & (cis[u] <= i1);
        }
        float2 ths[NC], phs[NC];
#pragma unroll
        for (int u = 0; u < NC; ++u) { ths[u] = tth[min(cis[u], nt1)]; phs[u] = tph[cjs[u]]; }
        bool pass[NC];
#pragma unroll
        for (int u = 0; u < NC; ++u)
            pass[u] = mores[u] & (DENSE || quadric(M, ths[u].x * phs[u].x, ths[u].x * phs[u].y, ths[u].y) >= 0.f);
        if (REC) {   // cell index within the box (only boxes of <= 128 cells are cached)
            const int c0 = *cell;
#pragma unroll
            for (int u = 0; u < NC; ++u) {
                const int cu = c0 + u;
                *rec0 |= (pass[u] & (cu < 64)) ? (1ull << (cu & 63)) : 0ull;
                *rec1 |= (pass[u] & ((cu >> 6) == 1)) ? (1ull << (cu & 63)) : 0ull;
            }
            *cell = c0 + NC;
        }
        unsigned es[NC];
#pragma unroll
        for (int u = 0; u < NC; ++u) es[u] = pack_ray(lane, cis[u], cjs[u]);
        {
            const bool wrap = cjs[NC - 1] >= j1;
            cj = wrap ? j0 : cjs[NC - 1] + 1;
            ci = cis[NC - 1] + (wrap ? 1 : 0);
            more = mores[NC - 1] & (ci <= i1);
        }
        int at = cnt;
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            const unsigned long long m = __builtin_amdgcn_ballot_w64(pass[u]);
            if (pass[u]) rayq[(qbase + at + lanes_below(m)) & (kRQ - 1)] = es[u];
            at += __popcll(m);
        }
        cnt = at;
    } while (cnt < 64 && __builtin_amdgcn_ballot_w64(more));
}

// Ray-cache walk (backward): each lane pops the lowest set cell of its pair's cached mask and
// appends that ray; same queue discipline as enumerate_box (no quadric, no table reads).
__device__ __forceinline__ void enumerate_cached(unsigned long long& bits0, unsigned long long& bits1, int ci0,
                                                 int cj0, int cw, float rcw, unsigned* rayq, int qbase, int& cnt) {
    const int lane = lane_id();
    do {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool lo = bits0 != 0ull;
            const bool pass = lo || bits1 != 0ull;
            const int b = lo ? (int)__builtin_ctzll(bits0) : (pass ? 64 + (int)__builtin_ctzll(bits1) : 0);
            if (lo) bits0 &= bits0 - 1ull;
            else bits1 &= bits1 - 1ull;
            const int di = (int)(((float)b + 0.5f) * rcw);
            const unsigned e = pack_ray(lane, ci0 + di, cj0 + b - di * cw);
            const unsigned long long m = __builtin_amdgcn_ballot_w64(pass);
            if (pass) rayq[(qbase + cnt + lanes_below(m)) & (kRQ - 1)] = e;
            cnt += __popcll(m);
        }
    } while (cnt < 64 && __builtin_amdgcn_ballot_w64((bits0 | bits1) != 0ull));
}

// LDS layouts of the two drains, with the round lengths that size their pads (validate on the host
// needs both; the other tunables live with their kernels)
#ifndef NLOSGR_FSTEPS
#define NLOSGR_FSTEPS 28
#endif
constexpr int kSteps = NLOSGR_FSTEPS;     // bins per lane per drain round (the largest; netf: kStepsNetf)
#ifndef NLOSGR_FSTEPS_NETF
#define NLOSGR_FSTEPS_NETF 20
#endif
constexpr int kStepsNetf = NLOSGR_FSTEPS_NETF;
// the twin drain (fx_twin_setup) runs longer rounds: a round costs two sets of exp2 seeds, and its unions are
// longer than single segments (one GPU, 24 / 28 / 32 bins: fwd 657.6 / 642.2 / 632.5 ms; another, 32 / 36 / 40 /
// 48 bins: 635.7 / 625.1 / 623.7 / 623.6 ms; with run-following pairs, 36 / 40 / 44 bins: 564.5 / 562.0 / 563.0 ms,
// and on another GPU 36 / 40: 566.3 / 564.6 ms: within 2.5 ms of each other, so 36 stays; with the tail refill rule
// and no placement, 32 / 36 / 40 bins: 507.1 / 504.8 / 507.6 ms)
#ifndef NLOSGR_FSTEPS_TWIN
#define NLOSGR_FSTEPS_TWIN 36
#endif
constexpr int kStepsTwin = NLOSGR_FSTEPS_TWIN;
constexpr int kStepsPad = kSteps > kStepsTwin ? kSteps : kStepsTwin;   // the layouts' pads hold the longest round
static_assert(kStepsNetf <= kSteps && kStepsNetf % 2 == 0 && kStepsTwin % 2 == 0, "the layouts' pads hold kStepsPad bins");
struct FwdLayout {
    int hist, owner, rayq, wave_stride, total;  // offsets in floats
    // fx: the fixed-point drain needs no claim table and no per-lane pad bins (22.7 KB per C3
    // workgroup instead of 26.6 KB: 7 workgroups per CU)
    __host__ __device__ FwdLayout(int nr, int nt, int np_, bool fx = false) {
        const int off = al4(2 * (nt + np_));  // float2 theta table [nt], float2 phi table [np]
        hist = 0;                             // [nr + kStepsPad] bins + [kStepsPad + 64] pad bins (fx: [nr + kStepsPad + 2])
        owner = fx ? al4(nr + kStepsPad + 4) : al4(nr + 2 * kStepsPad + 64);   // u8 [nr] claim table
        rayq = owner + (fx ? 0 : al4((nr + 3) / 4));   // uint [kRQ] ring
        wave_stride = al4(rayq + kRQ);
        hist += off; owner += off; rayq += off;
        total = off + kWaves * wave_stride;
    }
};

#ifndef NLOSGR_BSTEPS
#define NLOSGR_BSTEPS 24
#endif
constexpr int kBSteps = NLOSGR_BSTEPS;   // bins per lane per backward drain round
#ifndef NLOSGR_BSTEPS_TAIL_SHR
// the shared-row layout's TAIL rounds (C5: bwd 941 / 855 / 824 ms per shard at 24 / 32 / 40 bins; 40 spills
// 64 B per lane in the wall-point loop, none in the drain)
#define NLOSGR_BSTEPS_TAIL_SHR 40
#endif
#ifndef NLOSGR_BSTEPS_NETF_TAIL
// netf TAIL rounds (round 5: exp-free cubic in pdf, D = drho / (sigma c dT); C3 netf bwd 1500 / 1478 / 1468 /
// 1485 ms at 24 / 28 / 32 / 36 bins; 32 spills 36 B per lane, in the wall-point loop, not in the drain)
#define NLOSGR_BSTEPS_NETF_TAIL 32
#endif
#ifndef NLOSGR_BSTEPS_TAIL
// (round 4's 40-bin rounds spilled 36 B per lane, reloaded and re-stored every wall point: ~1.2 GB of
// scratch writes per launch reached HBM.  The wave index read as an SGPR (readfirstlane) keeps the
// wave-derived LDS bases out of VGPRs and the kernel spill-free at 40; 32 bins cost ~30 ms per step;
// 48 / 56 bins: 767 / 776 vs 773 ms with 16 / 44 B of spills per lane — kept at 40, spill-free)
#define NLOSGR_BSTEPS_TAIL 40
#endif
// the staged gradient row is zero-padded by the longest round (no-occlusion TAIL rounds)
constexpr int kmax_i(int a, int b) { return a > b ? a : b; }
constexpr int kBPad = kmax_i(kmax_i(NLOSGR_BSTEPS_TAIL, kBSteps), kmax_i(NLOSGR_BSTEPS_NETF_TAIL, NLOSGR_BSTEPS_TAIL_SHR));
constexpr int kBwdSlots = 13;   // per-Gaussian backward partial: D[3], K~[3], 0[3] (shape_acc), dMu[3], dsigma
                                // (stride kPartStride in HBM)
constexpr int kShPart = 28;     // sh_kernel partial: dF[KM <= 25], dMu[3] (at KM), pad

// Two layouts.  Per-wave rows (default): each wave walks its own wall points and stages its own
// upstream-gradient row and angle tables.  Shared rows (bwd_shared, long rows): the workgroup's 4
// waves own 4 x 64 Gaussians and walk the same wall points; one double-buffered row + tables per
// workgroup (staged by all 256 threads one wall point ahead, one barrier per wall point), so the
// LDS no longer scales with 4 x nr (C5, nr = 2048: 56 KB -> 39 KB per workgroup, 2 -> 4 per CU).
struct BwdLayout {
    int wave_base, wave_stride, grow, tth, tph, rayq, pdat, red, total, buf_stride;
    __host__ __device__ BwdLayout(int nr, int nt, int np_, bool shared = false) {
        buf_stride = 0;
        if (shared) {
            grow = 0;                                 // buffer b at smem + b * buf_stride
            tth = al4(nr + kBPad);
            tph = tth + al4(2 * nt);
            buf_stride = tph + al4(2 * np_);
            wave_base = 2 * buf_stride;
            rayq = 0;                                 // per-wave region (relative to the wave's base)
            pdat = rayq + kRQ;
            wave_stride = al4(pdat + 64 * 16);
            red = 0;                                  // unused: waves own distinct Gaussians
            total = wave_base + kWaves * wave_stride;
            return;
        }
        wave_base = 0;
        grow = 0;                            // [nr + kBPad] upstream gradient x att x hscale, zero pad
        tth = al4(nr + kBPad);               // float2 [nt]
        tph = tth + al4(2 * nt);             // float2 [np]
        rayq = tph + al4(2 * np_);           // uint [kRQ] ring
        pdat = rayq + kRQ;                   // pair table, 4 planes [4][64] float4: A[0:4] | A[4:8] | A[8], u0 | r2, rho, sigma, r3
        wave_stride = al4(pdat + 64 * 16);
        red = wave_base;                     // final reduction reuses the wave regions
        total = wave_base + kWaves * wave_stride;
        const int need_red = wave_base + kWaves * 64 * kBwdSlots;
        if (need_red > total) total = need_red;
    }
};

// Launch entry points (the host side fills KArgs from the workspace layout).  nlosgr_volume_fwd.hip:
// volume_fx_prepare zeroes the FX drain's u64 row, bound histogram and info words and sets the bounds, the unit
// and the bright list (before the records are made); volume_fwd runs the forward of a filled KArgs (FX iff
// ka.hfx, counting iff ka.counts, per-ray iff ka.ray_out) with its reduction to hist_out.
int volume_fx_prepare(const KArgs& ka, unsigned* bins, float* bound, int* blist, hipStream_t s);
int volume_fwd(const KArgs& ka, hipStream_t s);
// nlosgr_volume_bwd.hip: bwd_kernel and sh_kernel over wall points [ka.pb0, ka.pb0 + ka.pnw); finish_kernel
int volume_bwd_batch(const KArgs& ka, hipStream_t s);
int volume_bwd_finish(const KArgs& ka, float* d_mu, float* d_scaling, float* d_rotation, float* d_opacity,
                      float* d_features, hipStream_t s);

}  // namespace detail
}  // namespace nlosgr
