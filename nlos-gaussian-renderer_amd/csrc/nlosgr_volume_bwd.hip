// Transient Gaussian NLOS renderer — the pair-major volume backward (gfx950): bwd_kernel (the drain and the
// hand-off to the pair lanes), sh_kernel (the view-direction chain), finish_kernel (the splits' partials to
// the raw parameters) and their launch dispatch (volume_bwd_batch, volume_bwd_finish).
//
// Work decomposition (4 independent waves per workgroup): workgroup = 64 Gaussians x a split of the wall;
// wave w walks wall points w, w+4, ...  Lane = segment runs the bins of one ray serially with its sums in
// registers; per-pair sums in LDS; per-Gaussian accumulators stay in registers for the whole split and are
// combined in a fixed order into a partial slab.
#include <type_traits>

#include "nlosgr_volume.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

// Lane-serial backward drain: lane = one ray segment, kBSteps bins per round (the upstream
// gradient reads of a round are issued together), sums S_n = sum H pdf kap^n in registers.  A
// finished ray's closed-form result (dL/du0, dL/dv, dsigma, drho) is handed to the lane that owns
// its pair: finished lanes claim their pair lane with a forward permute (the highest claimant of a
// pair wins), each pair lane gathers its claimant's result with ds_bpermute and folds it into the
// Gaussian's register accumulators.  Losers keep their result and retry next round.  No LDS float
// atomics, no claim tables.
#ifndef NLOSGR_BREFILL
#define NLOSGR_BREFILL 16
#endif
constexpr int kBRefill = NLOSGR_BREFILL;   // refill once this many lanes are idle (or the queue is final)
#ifndef NLOSGR_BSTEPS_NETF
// 20 since round 5 (spill-free with the SGPR wave index; C3 netf bwd 1684 -> 1618 ms; 24 spills 12 B)
#define NLOSGR_BSTEPS_NETF 20
#endif
#ifndef NLOSGR_BWD_WPE
#define NLOSGR_BWD_WPE 4   // backward: minimum waves per SIMD (4: <= 128 VGPRs)
#endif

// per-lane backward segment state
struct BRay {
    int pos, rem, slot, ij, kl, len;
    float kap, kap0, c0, c2, st;
    float S0, S1, S2;
    float zs[3], v[3], ts, w;            // ray geometry for the closed-form result
    float rho, sigma;
    float T, pre, dsig, drho;            // netf: transmittance, prefix of H out, accumulators (part A)
    float S0b, S1b, S2b, dsigb;          // netf: accumulators of part B (scaled by the ray's total at the end)
};

// The pair table is stored as four planes of 64 float4 (plane c = float4 c of every pair slot): a lane's
// ds_read_b128 of slot s starts at bank 4 (s mod 16), so the 16 lanes of a read group spread over the 16
// bank quads (a [64][16] row layout started every row at one of 4 banks: up to 16-way conflicts)
__device__ __forceinline__ void load_pdat(const float* pd, int slot, float* A, float* u0, float& w, float& rho,
                                          float& sigma) {
    const float4* q4 = reinterpret_cast<const float4*>(pd) + slot;
    const float4 a = q4[0], c = q4[64], e = q4[128], g = q4[192];
    A[0] = a.x; A[1] = a.y; A[2] = a.z; A[3] = a.w; A[4] = c.x; A[5] = c.y; A[6] = c.z; A[7] = c.w; A[8] = e.x;
    u0[0] = e.y; u0[1] = e.z; u0[2] = e.w;
    rho = g.y; sigma = g.z;
    w = sigma * rho;   // (= P.w of the pair setup, bit for bit)
}

// grow[k] = dL/dhist[p,k] att[k] hscale[p], zero-padded to nr + kBPad.  Rows of nr % 4 == 0
// are staged with 16-B loads issued together (one memory round trip per 1024 bins per lane).
// lane index the compiler cannot hoist: per-wall-point staging addresses are recomputed (a few
// VALU ops) instead of being kept live across the backward's wall-point loop (they spilled)
__device__ __forceinline__ int lane_opaque() {
    int l = lane_id();
    __asm__ __volatile__("" : "+v"(l));
    return l;
}

__device__ __forceinline__ void stage_grow(const float* grad, const float* att, float hs, int nr, float* grow) {
    const int lane = lane_opaque();
    if (grad && (nr & 3) == 0 && ((reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(att)) & 15) == 0) {
        const float4* g4 = reinterpret_cast<const float4*>(grad);
        const float4* a4 = reinterpret_cast<const float4*>(att);
        const int n4 = nr >> 2;
        for (int t0 = lane; t0 < n4; t0 += 256) {
            float4 gv[4], av[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = t0 + 64 * u;
                if (t < n4) { gv[u] = g4[t]; av[u] = a4[t]; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = t0 + 64 * u;
                if (t < n4)
                    reinterpret_cast<float4*>(grow)[t] =
                        make_float4(gv[u].x * av[u].x * hs, gv[u].y * av[u].y * hs, gv[u].z * av[u].z * hs,
                                    gv[u].w * av[u].w * hs);
            }
        }
    } else {
        for (int t = lane; t < nr; t += 64) grow[t] = grad ? grad[t] * att[t] * hs : 0.f;
    }
    for (int t = nr + lane; t < nr + kBPad; t += 64) grow[t] = 0.f;
}

// shared layout: the whole workgroup stages wall point p's row and tables into one buffer
__device__ __forceinline__ void stage_shared(const KArgs& k, int p, int nr, int nt, int np_, float* grow, float2* tth,
                                             float2* tph) {
    const int t0 = threadIdx.x;
    const float hs = k.geo.hscale[p];
    const float* grad = k.grad_hist ? k.grad_hist + (size_t)p * nr : nullptr;
    const float* att = k.geo.att;
    if (grad && (nr & 3) == 0 && ((reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(att)) & 15) == 0) {
        const float4* g4 = reinterpret_cast<const float4*>(grad);
        const float4* a4 = reinterpret_cast<const float4*>(att);
        const int n4 = nr >> 2;
        for (int t = t0; t < n4; t += kBlock) {
            const float4 gv = g4[t], av = a4[t];
            reinterpret_cast<float4*>(grow)[t] =
                make_float4(gv.x * av.x * hs, gv.y * av.y * hs, gv.z * av.z * hs, gv.w * av.w * hs);
        }
    } else {
        for (int t = t0; t < nr; t += kBlock) grow[t] = grad ? grad[t] * att[t] * hs : 0.f;
    }
    for (int t = nr + t0; t < nr + kBPad; t += kBlock) grow[t] = 0.f;
    for (int t = t0; t < nt; t += kBlock)
        tth[t] = make_float2(k.geo.sin_theta[(size_t)p * nt + t], k.geo.cos_theta[(size_t)p * nt + t]);
    for (int t = t0; t < np_; t += kBlock)
        tph[t] = make_float2(k.geo.cos_phi[(size_t)p * np_ + t], k.geo.sin_phi[(size_t)p * np_ + t]);
}

template <int MODE, bool DENSE>
__device__ __forceinline__ bool bray_setup(const float* pd, float2 th, float2 ph, int slot, int i, int j, int nr,
                                           float mc2, float r0, float dr, float inv_dr, float f0log2, BRay& b) {
    float A[9], u0[3], w, rho, sigma;
    load_pdat(pd, slot, A, u0, w, rho, sigma);
    Ray R;
    if (!ray_setup<DENSE>(A, u0, th.x * ph.x, th.x * ph.y, th.y, mc2, r0, inv_dr, nr, R)) return false;
    b.pos = R.kl; b.kl = R.kl;
    b.len = b.rem = R.kh - R.kl + 1;
    b.slot = slot; b.ij = i | (j << 16);
    b.kap = b.kap0 = (float)R.kl - R.ks;
    b.c0 = -kHalfLog2e * R.m2min;
    b.c2 = -kHalfLog2e * R.a * dr * dr;
    b.st = th.x;
    b.S0 = b.S1 = b.S2 = 0.f;
    for (int r = 0; r < 3; ++r) { b.zs[r] = R.zs[r]; b.v[r] = R.v[r]; }
    b.ts = R.ts;
    b.w = w; b.rho = rho; b.sigma = sigma;
    if (MODE == NLOSGR_MODE_NETF) {
        b.T = fast_exp2((float)R.kl * f0log2);
        b.pre = b.dsig = b.drho = 0.f;
        b.S0b = b.S1b = b.S2b = b.dsigb = 0.f;
    }
    return true;
}

// TAIL (culled no-occlusion histogram backward at cutoff >= kTailCutoff): the drain reads the upstream
// row without the segment-end mask, see BV below

#ifdef NLOSGR_BCOUNT
// debug build (scripts/bwd_counts.py): loop iterations, drain rounds, active lanes, hand-off rounds,
// pending lanes, hand-offs done, refills, rays taken (per wave, summed), read by nlosgr_debug_bwd_counts
__device__ unsigned long long g_bdbg[8];
#define BDBG(i, v) bdbg[i] += (unsigned long long)(v)
#else
#define BDBG(i, v) ((void)0)
#endif

template <int PRESET, int MODE, bool DENSE, bool RAYS, bool CACHE, bool SHR, bool TAIL = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NLOSGR_BWD_WPE, 8))) void bwd_kernel(KArgs k) {
#ifdef NLOSGR_BCOUNT
    unsigned long long bdbg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
    // bins per drain round: netf keeps more per-ray state, so its rounds are shorter (no spill at 128 VGPRs)
    // (the no-occlusion TAIL rounds are longer: 32 bins measured 1137 vs 1170 ms at 24 on C3, and only
    // that variant stays spill-free at 32)
    constexpr int kRS = MODE == NLOSGR_MODE_NETF ? (TAIL && !RAYS && !DENSE ? NLOSGR_BSTEPS_NETF_TAIL : NLOSGR_BSTEPS_NETF)
                        : (MODE == NLOSGR_MODE_NOOCL && TAIL && !RAYS && !DENSE && !CACHE && !SHR) ? NLOSGR_BSTEPS_TAIL
                        : (MODE == NLOSGR_MODE_NOOCL && TAIL && !RAYS && !DENSE && !CACHE && SHR) ? NLOSGR_BSTEPS_TAIL_SHR : kBSteps;
    static_assert(kRS <= kBPad && kRS % 4 == 0, "the staged row is padded by kBPad bins; BV4 reads whole float4s");
    extern __shared__ __align__(16) float smem[];
    const int nr = k.geo.nr, nt = k.geo.nt, np_ = k.geo.np;
    constexpr bool shr = SHR;   // == (k.bshared != 0)
    const BwdLayout L(nr, nt, np_, shr);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();   // wave-uniform (SGPR)
    float* wb = smem + L.wave_base + wave * L.wave_stride;
    float* gbase = shr ? smem : wb;
    float* grow = gbase + L.grow;
    float2* tth = reinterpret_cast<float2*>(gbase + L.tth);
    float2* tph = reinterpret_cast<float2*>(gbase + L.tph);
    unsigned* rayq = reinterpret_cast<unsigned*>(wb + L.rayq);
    float* pdat = wb + L.pdat;

    const int gb = k.g_lo + blockIdx.x * (shr ? kNB * kWaves : kNB);
    const int gi = gb + (shr ? wave * kNB : 0) + lane;
    const bool active = gi < k.g_hi;
    const int split = blockIdx.y;
    const int per = (k.pnw + k.nsplit - 1) / k.nsplit;
    const int pbeg = k.pb0 + split * per, pend = min(k.pb0 + k.pnw, pbeg + per);
    const int deg = k.g.sh_degree;
    const int K = (deg + 1) * (deg + 1);
    const float mc2 = k.opt.cutoff * k.opt.cutoff;
    const float r0 = k.geo.r[0];
    const float dr = nr > 1 ? (k.geo.r[nr - 1] - r0) / (float)(nr - 1) : 0.f;
    const float inv_dr = dr > 0.f ? 1.0f / dr : 0.f;
    const float cdt = k.opt.c_deltaT;
    const bool small_x = cdt <= kSmallX;   // netf: exp-free transmittance factor (om_exp_small)
    const float f0log2 = log2f(1.0f + 1e-7f);
    const float rscale = k.opt.ray_scale;

    // shape accumulators (shape_acc: D = diag of dA A^T, K~ = its rotational part), dL/dmu, dL/dsigma
    float sD[3] = {0.f, 0.f, 0.f}, sK[3] = {0.f, 0.f, 0.f}, dMu[3], dSig = 0.f;
    dMu[0] = dMu[1] = dMu[2] = 0.f;
    // this lane's Gaussian: record and feature row are re-read per wall point (L1/L2 hits) rather
    // than held in registers across the split (VGPR budget)
    // (mu too: a register copy across the wall-point loop spilled at the longer netf rounds)
    const float* feat = k.g.features + (size_t)(active ? gi : 0) * k.g.k_feat;

    if (shr && pbeg < pend) stage_shared(k, pbeg, nr, nt, np_, grow, tth, tph);
    int it = 0;
    for (int p = pbeg + (shr ? 0 : wave); p < pend; p += (shr ? 1 : kWaves), ++it) {
        // stage this wall point's upstream gradient row and tables (wave-private), or (shared) make
        // the buffer staged one wall point ahead current and stage the next one into the other
        const float hs = k.geo.hscale[p];
        wave_sync();
        if (shr) {
            __syncthreads();   // buffer it & 1 complete; every wave is done with wall point p - 1
            float* bnext = smem + ((it + 1) & 1) * L.buf_stride;
            if (p + 1 < pend)
                stage_shared(k, p + 1, nr, nt, np_, bnext + L.grow, reinterpret_cast<float2*>(bnext + L.tth),
                             reinterpret_cast<float2*>(bnext + L.tph));
            float* bcur = smem + (it & 1) * L.buf_stride;
            grow = bcur + L.grow;
            tth = reinterpret_cast<float2*>(bcur + L.tth);
            tph = reinterpret_cast<float2*>(bcur + L.tph);
        } else {
            stage_grow(k.grad_hist ? k.grad_hist + (size_t)p * nr : nullptr, k.geo.att, hs, nr, grow);
            const int ln = lane_opaque();
            for (int t = ln; t < nt; t += 64)
                tth[t] = make_float2(k.geo.sin_theta[(size_t)p * nt + t], k.geo.cos_theta[(size_t)p * nt + t]);
            for (int t = ln; t < np_; t += 64)
                tph[t] = make_float2(k.geo.cos_phi[(size_t)p * np_ + t], k.geo.sin_phi[(size_t)p * np_ + t]);
        }
        const float px = k.geo.wall[3 * p], py = k.geo.wall[3 * p + 1], pz = k.geo.wall[3 * p + 2];
        // per-pair row offset, recomputed per wall point (not hoisted as per-lane 64-bit pointers)
        int gio = gi;
        __asm__ __volatile__("" : "+v"(gio));
        const size_t o = (size_t)p * k.g.ng + gio;
        // pair setup (lane = Gaussian gi at wall point p); the ray pass reads the pair table
        bool more = false;
        float M[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int i0 = 0, i1 = -1, j0 = 0, j1 = -1;
        float wpair = 0.f;
        unsigned bx = 0u;
        if (active) {
            Pair P;
            float mu[3];
            load_rec(k.recs[gi], P, mu);
            if (CACHE) bx = k.cbox[o];
            if (CACHE && bx != 0u) {
                // cached pair: u0 and the forward's albedo; no SH evaluation, no footprint (the
                // recorded cells replace the quadric walk)
                P.q[0] = px - mu[0]; P.q[1] = py - mu[1]; P.q[2] = pz - mu[2];
                for (int r = 0; r < 3; ++r)
                    P.u0[r] = P.A[3 * r] * P.q[0] + P.A[3 * r + 1] * P.q[1] + P.A[3 * r + 2] * P.q[2];
                P.rho = k.crho[o];
                P.w = P.sigma * P.rho;
                P.i0 = P.j0 = 0; P.i1 = P.j1 = 0;
                for (int t = 0; t < 6; ++t) P.M[t] = 0.f;
            } else {
                pair_setup<PRESET, DENSE>(k, feat, mu, px, py, pz, k.geo.grid_lin + 4 * (size_t)p, mc2, P);
            }
            more = (P.w > 0.f) && P.i0 <= P.i1 && P.j0 <= P.j1 && !(k.opt.flags & 2);  // flags 2: setup only
            for (int t = 0; t < 6; ++t) M[t] = P.M[t];
            i0 = P.i0; i1 = P.i1; j0 = P.j0; j1 = P.j1;
            wpair = P.w;
            float4* d4 = reinterpret_cast<float4*>(pdat) + lane;
            d4[0] = make_float4(P.A[0], P.A[1], P.A[2], P.A[3]);
            d4[64] = make_float4(P.A[4], P.A[5], P.A[6], P.A[7]);
            d4[128] = make_float4(P.A[8], P.u0[0], P.u0[1], P.u0[2]);
            float r2, r3;
            scale_ratios(P.A, r2, r3);
            d4[192] = make_float4(r2, P.rho, P.sigma, r3);
        }
        // ray cache of the forward: cached pairs walk their recorded cells instead of enumerating
        unsigned long long cbits0 = 0ull, cbits1 = 0ull;
        int ci0 = 0, cj0 = 0, cw = 1;
        float rcw = 1.f;
        if (CACHE && active) {
            if (bx != 0u) {
                const ulonglong2 cm = k.cmask[o];
                cbits0 = more ? cm.x : 0ull;
                cbits1 = more ? cm.y : 0ull;
                ci0 = bx & 0xFFF; cj0 = (bx >> 12) & 0xFFF; cw = bx >> 24;
                rcw = 1.0f / (float)cw;
                more = false;
            }
        }
        const float* gray = RAYS && k.grad_ray ? k.grad_ray + (size_t)p * nt * np_ * nr : nullptr;
        wave_sync();
        int ci = i0, cj = j0, qhead = 0, qcount = 0;
        bool act = false, pend = false;
        float dU0p[3] = {0.f, 0.f, 0.f}, drho_pair = 0.f, s0_pair = 0.f;
        BRay b;
        b.pos = 0; b.rem = 0; b.slot = lane; b.ij = 0; b.kl = 0; b.len = 0;
        b.kap = b.kap0 = b.c0 = b.c2 = b.st = 0.f;
        b.S0 = b.S1 = b.S2 = 0.f;
        b.zs[0] = b.zs[1] = b.zs[2] = b.v[0] = b.v[1] = b.v[2] = b.ts = b.w = 0.f;
        b.rho = b.sigma = 0.f;
        b.T = b.pre = b.dsig = b.drho = 0.f;
        b.S0b = b.S1b = b.S2b = b.dsigb = 0.f;
        // pending result of a finished ray: dL/du0, dL/dv, dsigma, drho
        // the ray's dL/dA contribution dL/dv d^T goes over as shape_acc's (D, K~), formed at the ray's end (rD, rK)
        float rU[3] = {0.f, 0.f, 0.f}, rD[3] = {0.f, 0.f, 0.f}, rK[3] = {0.f, 0.f, 0.f}, rSig = 0.f, rRho = 0.f;
        while (true) {
            if (CACHE && qcount < 64 && __builtin_amdgcn_ballot_w64((cbits0 | cbits1) != 0ull)) {
                wave_sync();
                enumerate_cached(cbits0, cbits1, ci0, cj0, cw, rcw, rayq, qhead, qcount);
                wave_sync();
            }
            if (qcount < 64 && __builtin_amdgcn_ballot_w64(more)) {
                wave_sync();
                enumerate_box<DENSE>(M, i1, j0, j1, more, ci, cj, tth, tph, nt - 1, rayq, qhead, qcount);
                wave_sync();
            }
            const bool anymore = __builtin_amdgcn_ballot_w64(more || (CACHE && (cbits0 | cbits1) != 0ull)) != 0;
            // a lane whose finished result still waits for its hand-off takes no new ray
            const unsigned long long idle = __builtin_amdgcn_ballot_w64(!act && !pend);
            const int nidle = __popcll(idle);
            if (qcount > 0 && (nidle >= kBRefill || !anymore)) {
                const int r = lanes_below(idle);
                const bool take = !act && !pend && r < qcount;
                if (take && !(k.opt.flags & 1)) {                  // flags 1: enumerate only
                    const unsigned e = rayq[(qhead + r) & (kRQ - 1)];
                    const int slot = e & 0xFF, i = (e >> 8) & 0xFFF, j = e >> 20;
                    act = bray_setup<MODE, DENSE>(pdat, tth[i], tph[j], slot, i, j, nr, mc2, r0, dr,
                                                  inv_dr, f0log2, b) && !(k.opt.flags & 4);  // flags 4: no bins
                    if (MODE == NLOSGR_MODE_NETF && TAIL) b.T *= b.st;   // sin(theta) rides on T (BV rows)
                    if (MODE == NLOSGR_MODE_NETF && TAIL && !DENSE && act) {
                        // part B's sums are a_c sigma sum_j pdf_j (1, kap_j, kap_j^2) over the ray's bins, which the
                        // TAIL rounds cover to past 5 sigma on both sides: they are set here once instead of 3 VALU
                        // per bin.  A ray at least one bin wide (sigma_b^2 = 1 / (a dr^2) >= 1) whose Gaussian lies
                        // inside the histogram by 6 sigma_b on both sides: its own moments 2^c0 sqrt(2 pi) sigma_b
                        // (1, 0, sigma_b^2) (Poisson summation: relative error <= exp(-2 pi^2 sigma_b^2) < 3e-9, plus
                        // the tails past 5 sigma the rounds leave out, < 3e-7 of the ray's sum); any other (narrow, or
                        // cut by the first or last bin): its support bins [kl, kh] summed here
                        const float sb2 = kHalfLog2e * frcp(-b.c2);
                        const float ksb = (float)b.kl - b.kap0;   // the closest approach, in bins
                        const float w6 = 6.0f * __builtin_amdgcn_sqrtf(sb2);
                        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
                        if (sb2 >= 1.0f && ksb - w6 >= 0.f && ksb + w6 <= (float)(nr - 1)) {
                            g0 = fast_exp2(b.c0) * (2.50662827463f * __builtin_amdgcn_sqrtf(sb2));
                            g2 = g0 * sb2;
                        } else {
                            // A segment the last bin clips (kh = nr - 1) is summed through the end of its last
                            // round: the rounds have no end mask, so part A holds -P_j a_c w_j for the slots past
                            // nr - 1 as well (H = 0 there, P_j = E), and on a Gaussian that is still wide there
                            // only the same slots in part B cancel them in A + E B.  (Past an inner end kh < nr - 1
                            // those slots hold the Gaussian's tail beyond the cutoff, which is left out as above.)
                            int jend = b.kl + b.len;
                            if (jend == nr) {
                                const int o0 = b.kl & 1;   // the first round starts at the even bin at or below kl
                                jend = b.kl - o0 + ((b.len + o0 + kRS - 1) / kRS) * kRS;
                            }
                            for (int jb = b.kl; jb < jend; ++jb) {
                                const float kj = b.kap0 + (float)(jb - b.kl);
                                const float pj = fast_exp2(fmaf(b.c2, kj * kj, b.c0));
                                g0 += pj;
                                g1 = fmaf(pj, kj, g1);
                                g2 = fmaf(pj * kj, kj, g2);
                            }
                        }
                        const float acl = -cdt / (1.0f + 1e-7f);
                        b.S0b = b.sigma * acl * g0;
                        b.S1b = b.sigma * acl * g1;
                        b.S2b = b.sigma * acl * g2;
                        b.dsigb = acl * g0;
                    }
                }
                const int ntake = min(nidle, qcount);
                BDBG(6, 1); BDBG(7, ntake);
                qhead = (qhead + ntake) & (kRQ - 1);
                qcount -= ntake;
            }
            const bool anyact = __builtin_amdgcn_ballot_w64(act) != 0;
            const bool anypend = __builtin_amdgcn_ballot_w64(pend) != 0;
            if (!anyact && !anypend) {
                if (!anymore && qcount == 0) break;
                continue;
            }
            BDBG(0, 1);
            if (anyact) { BDBG(1, 1); BDBG(2, __popcll(__builtin_amdgcn_ballot_w64(act))); }
            if (anyact) {
                const int remw = act ? b.rem : 0;
                // BV: the round starts at the even bin at or below pos (float2 row reads, half the LDS
                // instructions); slot j is bin (pos & ~1) + j, in the segment iff o <= j < remw + o
                constexpr bool BV = (MODE == NLOSGR_MODE_NOOCL || (MODE == NLOSGR_MODE_NETF && TAIL)) && !RAYS && !DENSE;
                // BV4 (no-occlusion TAIL): the round starts at the bin at or below pos that is a multiple of
                // 4 and reads the row as float4 (ds_read_b128: 16-lane groups over 16 bank quads conflict
                // less per bin than 32-lane groups over 32 bank pairs, and half the instructions)
                // (netf TAIL measured 20 ms slower with float4 reads: C3 netf bwd 1537 -> 1557 ms)
                constexpr bool BV4 = MODE == NLOSGR_MODE_NOOCL && TAIL && !RAYS && !DENSE;
                constexpr int BVW = BV4 ? 4 : 2;
                const int o = BV && act ? (b.pos & (BVW - 1)) : 0;
                const float* gr = grow + (act ? b.pos - o : 0);
                const float* gw = RAYS && gray ? gray + (size_t)((b.ij & 0xFFFF) * np_ + (b.ij >> 16)) * nr + b.pos
                                               : nullptr;
                float Hs[kRS];
                if (BV4) {
                    // as below, with slots 0..o-1 before pos masked (o <= 3)
                    const float4* g4 = reinterpret_cast<const float4*>(gr);
#pragma unroll
                    for (int m = 0; m < kRS; m += 4) {
                        const float4 h = g4[m / 4];
                        Hs[m] = (m == 0 && o > 0) ? 0.f : h.x;
                        Hs[m + 1] = (m == 0 && o > 1) ? 0.f : h.y;
                        Hs[m + 2] = (m == 0 && o > 2) ? 0.f : h.z;
                        Hs[m + 3] = h.w;
                    }
                } else if (BV && TAIL) {
                    // no end mask: a segment's last round also weighs the bins past its end (up to
                    // kRS - 1 of them) with their exact pdf, < exp(-m_c^2 / 2) of the Gaussian's peak
                    // (<= 3.7e-6 at m_c >= kTailCutoff: the support is a superset of the forward's, closer
                    // to the dense reference; idle and blocked lanes are zeroed through their pdf seed
                    // below).  Slot 0 before pos (o = 1) stays masked: the recurrence starts at pos.
                    const float2* g2 = reinterpret_cast<const float2*>(gr);
#pragma unroll
                    for (int m = 0; m < kRS; m += 2) {
                        const float2 h = g2[m / 2];
                        Hs[m] = (m == 0 && o) ? 0.f : h.x;
                        Hs[m + 1] = h.y;
                    }
                } else if (BV) {
                    const int lim = remw + o;
                    const float2* g2 = reinterpret_cast<const float2*>(gr);
#pragma unroll
                    for (int m = 0; m < kRS; m += 2) {
                        const float2 h = g2[m / 2];
                        Hs[m] = (m >= o && m < lim) ? h.x : 0.f;
                        Hs[m + 1] = (m + 1 < lim) ? h.y : 0.f;
                    }
                } else {
#pragma unroll
                    for (int m = 0; m < kRS; ++m) {
                        float H = gr[m];
                        if (RAYS || MODE == NLOSGR_MODE_NETF) H *= b.st;
                        if (RAYS && gw && m < remw) H += gw[m] * rscale;
                        Hs[m] = m < remw ? H : 0.f;
                    }
                }
                float kap = b.kap;
                if (MODE == NLOSGR_MODE_NOOCL) {
                    float S0 = b.S0, S1 = b.S1, S2 = b.S2;
                    if (!DENSE) {
                        // exp2 recurrence (kRecurrence) and moments about the round's first bin:
                        // U_n = sum_m hp m^n, then S_n += sum_m hp (kap + m)^n
                        float pdf = fast_exp2(fmaf(b.c2, kap * kap, b.c0));
                        // BV reads the row unmasked: idle lanes and blocked ones (finished, rem <= 0, waiting
                        // for their hand-off) contribute through a zero seed
                        if (BV && TAIL && !(act && b.rem > 0)) pdf = 0.f;
                        float q = fast_exp2(b.c2 * fmaf(2.f, kap, 1.f));
                        const float cc = fast_exp2(2.f * b.c2);
                        // three nested running sums (one fma, two adds per bin): with w = kRS - m,
                        // A = sum hp, B = sum hp w, C = sum hp w (w + 1) / 2, hp = H pdf; then about
                        // K = kap at slot kRS: sum hp (K - w)^n for n = 0, 1, 2 (w^2 sums to 2C - B)
                        float A = 0.f, B = 0.f, C = 0.f;
#pragma unroll
                        for (int m = 0; m < kRS; ++m) {
                            A = fmaf(Hs[m], pdf, A);
                            B += A;
                            C += B;
                            if (BV && m < BVW - 1) {   // the recurrence starts at pos (slot o)
                                pdf = m < o ? pdf : pdf * q;
                                q = m < o ? q : q * cc;
                            } else {
                                pdf *= q;
                                q *= cc;
                            }
                        }
                        const float K = kap - (float)o + (float)kRS;
                        S0 += A;
                        S1 += fmaf(K, A, -B);
                        S2 += fmaf(K, fmaf(K, A, -2.f * B), fmaf(2.f, C, -B));
                        kap += (float)(kRS - o);
                    } else
#pragma unroll
                    for (int m = 0; m < kRS; ++m) {
                        const float hp = Hs[m] * fast_exp2(fmaf(b.c2, kap * kap, b.c0));
                        const float t1 = hp * kap;
                        S0 += hp; S1 += t1; S2 = fmaf(t1, kap, S2);
                        kap += 1.f;
                    }
                    b.S0 = S0; b.S1 = S1; b.S2 = S2;
                } else {
                    // dL/dD_j = c rho H_j T_j + a_j (E - P_j),  a_j = f'_j / f_j = -c dT e_j / f_j, P_j = the
                    // prefix sum of H_k out_k through bin j and E its total over the ray.  One pass: every
                    // weighted sum sum_j dL/dD_j w_j splits into part A = sum_j (c rho H_j T_j - P_j a_j) w_j and
                    // part B = sum_j a_j w_j, combined as A + E B once the ray is done (E = P at the end).
                    float T = b.T, pre = b.pre;
                    float S0 = b.S0, S1 = b.S1, S2 = b.S2, dsig = b.dsig, drho = b.drho;
                    float S0b = b.S0b, S1b = b.S1b, S2b = b.S2b, dsigb = b.dsigb;
                    const float kE = -cdt * (2.f * kHalfLog2e) * b.sigma, ncdt = -cdt, crho = cdt * b.rho;
                    // culled: pdf by the exp2 recurrence (kRecurrence), re-seeded per round
                    float cur = 0.f, rq = 0.f, rcc = 0.f;
                    // TAIL: the recurrence starts at slot 0 = bin pos - o; inactive lanes get a zero seed
                    const float kseed = TAIL ? kap - (float)o : kap;
                    if (!DENSE) {
                        cur = fast_exp2(fmaf(b.c2, kseed * kseed, b.c0));
                        rq = fast_exp2(b.c2 * fmaf(2.f, kseed, 1.f));
                        rcc = fast_exp2(2.f * b.c2);
                        if (TAIL && !(act && b.rem > 0)) cur = 0.f;
                    }
                    if (!DENSE && (small_x || TAIL)) {   // (netf TAIL is launched only when small_x)
                        // c dT <= 1/64: x = sigma pdf c dT <= c dT, so exp(-x) = 1 - om_exp_small(x) (no
                        // exp) and a_j = -c dT e_j / (e_j + 1e-7) = -c dT / (1 + 1e-7 / e_j) is the constant
                        // a_c = -c dT / (1 + 1e-7) to 1e-7 x relative (no rcp): part B's sums become
                        // a_c sum pdf (1, m, m^2) (moments about the round's first bin, like U_n above)
                        const float sx = cdt * b.sigma;
                        const float ac = ncdt / (1.0f + 1e-7f);
                        // exp(-x) + 1e-7 for x = sx pdf <= 1/64 as a cubic in pdf (the x^4 / 24 term, <= 2.5e-9,
                        // is dropped; the forward's factor, kTf0 = 1 + 1e-7 in float)
                        const float e1 = -sx, e2 = 0.5f * sx * sx, e3 = (-1.0f / 6.0f) * sx * sx * sx;
                        // the prefix P_j = rho sum_{k<=j} H_k T_k x_k = rho sx D_j with D_j = sum_{k<=j} H_k T_k pdf_k
                        // (this path keeps D in b.drho; rho is the pair's), so part A's weight is
                        // c rho H_j T_j - P_j a_c = crho (HT + kk D) with kk = -a_c sigma; sum_j c1_j pdf_j
                        // (dsigma's part A) is crho UA0, summed per round below
                        const float kk = -ac * b.sigma;
                        // part A's moments by nested running sums (as the no-occlusion drain): UA0 = sum hA,
                        // UA1 = sum hA w, UA2 = sum hA w (w + 1) / 2 with w = kRS - m; part B's directly
                        float UA0 = 0.f, UA1 = 0.f, UA2 = 0.f, UB0 = 0.f, UB1 = 0.f, UB2 = 0.f;
                        constexpr bool UB = !TAIL;   // part B per bin (TAIL: set at the ray's start)
#pragma unroll
                        for (int m = 0; m < kRS; ++m) {
                            // TAIL: no segment-end mask (the bins past the end carry the Gaussian's exact
                            // tail, as in the no-occlusion drains); only slot 0 before pos (o = 1) in a
                            // segment's first round is inactive.  sin(theta) is folded into T (bray start).
                            const bool in = TAIL ? !(m == 0 && o) : m < remw;
                            const float pdf = cur;
                            cur *= rq;
                            rq *= rcc;
                            const float f = fmaf(pdf, fmaf(pdf, fmaf(pdf, e3, e2), e1), kTf0);
                            const float HT = Hs[m] * T;
                            drho = fmaf(HT, pdf, drho);               // D
                            const float c1 = in ? fmaf(kk, drho, HT) : 0.f;
                            UA0 = fmaf(c1, pdf, UA0);                 // x crho sigma at the end
                            UA1 += UA0;
                            UA2 += UA1;
                            if (UB) {
                                const float pin = in ? pdf : 0.f;
                                UB0 += pin;
                                UB1 = fmaf(pin, (float)m, UB1);
                                UB2 = fmaf(pin, (float)(m * m), UB2);
                            }
                            T *= in ? f : 1.f;
                        }
                        dsig = fmaf(crho, UA0, dsig);
                        pre = b.rho * sx * drho;
                        // S_n += sum h (kb + m)^n, kb = the round's first bin offset
                        const float kb = kseed;
                        const float sg = b.sigma * crho;
                        const float sgb = b.sigma * ac;
                        const float KA = kb + (float)kRS;   // kap at slot kRS
                        S0 = fmaf(sg, UA0, S0);
                        S1 = fmaf(sg, fmaf(KA, UA0, -UA1), S1);
                        S2 = fmaf(sg, fmaf(KA, fmaf(KA, UA0, -2.f * UA1), fmaf(2.f, UA2, -UA1)), S2);
                        S0b = fmaf(sgb, UB0, S0b);
                        S1b = fmaf(sgb, fmaf(kb, UB0, UB1), S1b);
                        S2b = fmaf(sgb, fmaf(kb, fmaf(kb, UB0, 2.f * UB1), UB2), S2b);
                        dsigb = fmaf(ac, UB0, dsigb);
                        kap += (float)(kRS - o);
                    } else {
#pragma unroll
                    for (int m = 0; m < kRS; ++m) {
                        const bool in = m < remw;
                        float pdf;
                        if (DENSE) {
                            pdf = fast_exp2(fmaf(b.c2, kap * kap, b.c0));
                        } else {
                            pdf = cur;
                            cur *= rq;
                            rq *= rcc;
                        }
                        // per-ray constants folded: sp = sigma pdf, exp(-sp c dT) = exp2(pdf kE)
                        const float sp = b.sigma * pdf;
                        const float H = Hs[m];
                        const float ee = fast_exp2(pdf * kE);
                        const float f = ee + 1e-7f;
                        const float HT = H * T;
                        const float hdt = HT * (cdt * sp);
                        drho += hdt;
                        pre = fmaf(b.rho, hdt, pre);
                        const float a = in ? (ee * ncdt) * frcp(f) : 0.f;
                        const float c1 = in ? fmaf(-pre, a, crho * HT) : 0.f;
                        const float hA = c1 * sp, hB = a * sp;
                        dsig = fmaf(c1, pdf, dsig);
                        dsigb = fmaf(a, pdf, dsigb);
                        const float tA = hA * kap, tB = hB * kap;
                        S0 += hA; S1 += tA; S2 = fmaf(tA, kap, S2);
                        S0b += hB; S1b += tB; S2b = fmaf(tB, kap, S2b);
                        T *= in ? f : 1.f;
                        kap += 1.f;
                    }
                    }
                    b.T = T; b.pre = pre;
                    b.S0b = S0b; b.S1b = S1b; b.S2b = S2b; b.dsigb = dsigb;
                    b.S0 = S0; b.S1 = S1; b.S2 = S2; b.dsig = dsig; b.drho = drho;
                }
                if (act) {
                    if (b.rem > 0) {   // (a blocked lane, rem <= 0, added zeros and stays put)
                        b.kap = kap;
                        b.pos += kRS - o;
                        b.rem -= kRS - o;
                    }
                    if (b.rem <= 0 && !pend) {
                        // pdf = exp(-|z|^2/2), z = z* + dl v:  dL/du0 = -sum P z,  dL/dv = -sum P dl z
                        float S0 = b.S0, S1 = b.S1, S2 = b.S2;
                        if (MODE == NLOSGR_MODE_NETF) {   // A + E B, E = the ray's total (its final prefix)
                            S0 = fmaf(b.pre, b.S0b, S0);
                            S1 = fmaf(b.pre, b.S1b, S1);
                            S2 = fmaf(b.pre, b.S2b, S2);
                        }
                        S1 = S1 * dr;
                        S2 = S2 * dr * dr;
                        if (MODE == NLOSGR_MODE_NOOCL) {
                            if (!RAYS) { S0 *= b.st; S1 *= b.st; S2 *= b.st; }
                            // no-occlusion: dsigma = S0 rho, drho = S0 sigma; the pair lane applies its own
                            // rho and sigma to the summed S0 (one value handed over instead of two)
                            rSig = S0;
                            rRho = 0.f;
                            S0 *= b.w; S1 *= b.w; S2 *= b.w;
                        } else {
                            rSig = fmaf(b.pre, b.dsigb, b.dsig);
                            // (the exp-free culled drain keeps D = drho / (sigma c dT) in b.drho)
                            rRho = !DENSE && (small_x || TAIL) ? b.drho * (cdt * b.sigma) : b.drho;
                        }
                        float rV[3];
                        for (int r = 0; r < 3; ++r) {
                            const float zv = S0 * b.zs[r] + S1 * b.v[r];
                            rU[r] = -zv;
                            rV[r] = -(b.ts * zv + S1 * b.zs[r] + S2 * b.v[r]);
                        }
                        // dL/dA += dL/dv d^T, in whitened form shape_acc(dL/dv, v = A d) with the pair's
                        // scale ratios (pair table plane 3), formed once here rather than per hand-off round
                        const float4 rr = reinterpret_cast<const float4*>(pdat)[192 + b.slot];   // r2, rho, sigma, r3
                        rD[0] = rD[1] = rD[2] = rK[0] = rK[1] = rK[2] = 0.f;
                        shape_acc(rV, b.v, rr.x, rr.w, rD, rK);
                        act = false;
                        pend = !(k.opt.flags & 32);   // flags 32 (diagnostics): drop results, no hand-off
                    }
                }
            }
            const unsigned long long pmask = __builtin_amdgcn_ballot_w64(pend);
            if (pmask) {
                // hand finished rays to their pair lanes: per pair and round one claimant, its result
                // fetched by the pair lane with bpermute.  The claim is a forward permute (ds_permute_b32,
                // no LDS memory, no fences): every pending lane sends lane + 1 to its pair lane, and of
                // several senders to one lane the highest lane's value arrives (lanes nobody writes
                // receive 0; measured on gfx950, scripts/permute_probe.hip).  Every lane that must
                // receive also sends, so the lanes without a result park a 0 on lane 0 in one permute and
                // on lane 1 in a second; lane 0 reads the second, every other lane the first.
                const int pv = pend ? lane + 1 : 0;
                const int w1 = __builtin_amdgcn_ds_permute((pend ? b.slot : 0) << 2, pv);
                const int w2 = __builtin_amdgcn_ds_permute((pend ? b.slot : 1) << 2, pv);
                const int wcl = lane == 0 ? w2 : w1;
                const bool got = wcl != 0;
                const int src = got ? wcl - 1 : lane;
                // (all lanes execute the bpermute: a source lane inactive in EXEC reads as 0)
                const int wpair = __builtin_amdgcn_ds_bpermute(b.slot << 2, wcl);
                const bool won = pend && wpair == lane + 1;
                const float gm = got ? 1.f : 0.f;
                float gU[3];
                // every lane must execute the bpermute: it cannot read lanes that are inactive in EXEC
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    gU[c] = gm * __shfl(rU[c], src);
                    sD[c] += gm * __shfl(rD[c], src);
                    sK[c] += gm * __shfl(rK[c], src);
                }
                const float gSig = gm * __shfl(rSig, src);
                const float gRho = MODE == NLOSGR_MODE_NOOCL ? 0.f : gm * __shfl(rRho, src);
                for (int r = 0; r < 3; ++r) dU0p[r] += gU[r];
                if (MODE == NLOSGR_MODE_NOOCL) {
                    s0_pair += gSig;
                } else {
                    dSig += gSig;
                    drho_pair += gRho;
                }
                BDBG(3, 1); BDBG(4, __popcll(pmask)); BDBG(5, __popcll(__builtin_amdgcn_ballot_w64(won)));
                if (won) pend = false;
            }
        }
        // chain of this wall point's pair (Gaussian gi, wall point p) through u0 = A (p - mu); the
        // view-direction chain through rho (SH basis, d_features and its d_mu share) runs in
        // sh_kernel from the stored dL/drho, which keeps 16 feature accumulators out of this kernel
        if (MODE == NLOSGR_MODE_NOOCL && active) {
            const float4 wrs = reinterpret_cast<const float4*>(pdat)[192 + lane];   // w, rho, sigma
            dSig += s0_pair * wrs.y;
            drho_pair = s0_pair * wrs.z;
        }
        if (active && wpair > 0.f) {
            // dL/dA += dL/du0 (p - mu)^T, as shape_acc(dL/du0, u0) with u0 = A (p - mu) from the pair table
            const float4* d4 = reinterpret_cast<const float4*>(pdat) + lane;
            const float4 a = d4[0], c = d4[64], e = d4[128], rr = d4[192];
            const float A[9] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w, e.x};
            const float u0[3] = {e.y, e.z, e.w};
            shape_acc(dU0p, u0, rr.x, rr.w, sD, sK);
            for (int cc = 0; cc < 3; ++cc) dMu[cc] -= A[cc] * dU0p[0] + A[3 + cc] * dU0p[1] + A[6 + cc] * dU0p[2];
        }
        if (active) k.drho[(size_t)(p - k.pb0) * k.g.ng + gio] = (wpair > 0.f && !(k.opt.flags & 64)) ? drho_pair : 0.f;
    }
#ifdef NLOSGR_BCOUNT
    if (lane == 0)
        for (int c = 0; c < 8; ++c) atomicAdd(&g_bdbg[c], bdbg[c]);
#endif
    if (shr) {   // shared layout: every wave owns its Gaussians for the whole split
        if (active) {
            // (rows of this split belong to this workgroup only; the first batch overwrites whatever the
            // workspace held, later batches add)
            float* dst = k.partial + ((size_t)split * k.g.ng + gi) * kPartStride;
            float v[kBwdSlots];
            for (int t = 0; t < 3; ++t) { v[t] = sD[t]; v[3 + t] = sK[t]; v[6 + t] = 0.f; }
            v[9] = dMu[0]; v[10] = dMu[1]; v[11] = dMu[2]; v[12] = dSig;
            if (k.accum)
                for (int t = 0; t < kBwdSlots; ++t) v[t] += dst[t];
            for (int t = 0; t < kBwdSlots; ++t) dst[t] = v[t];
        }
        return;
    }
    // fixed-order combination of the 4 waves' accumulators -> partial slab
    __syncthreads();
    float* red = smem + L.red;
    {
        float* dst = red + (wave * 64 + lane) * kBwdSlots;
        for (int t = 0; t < 3; ++t) { dst[t] = sD[t]; dst[3 + t] = sK[t]; dst[6 + t] = 0.f; }
        dst[9] = dMu[0]; dst[10] = dMu[1]; dst[11] = dMu[2];
        dst[12] = dSig;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kNB * kBwdSlots; t += blockDim.x) {
        const int g = t / kBwdSlots, c = t - g * kBwdSlots;
        if (gb + g >= k.g_hi) continue;
        float s = 0.f;
        for (int w = 0; w < kWaves; ++w) s += red[(w * 64 + g) * kBwdSlots + c];
        float* dst = k.partial + ((size_t)split * k.g.ng + gb + g) * kPartStride + c;
        *dst = k.accum ? *dst + s : s;
    }
}

// ------------------------------------------------------------------------------------------
// sh_kernel: the view-direction chain of every pair from the backward's dL/drho (fixed wall-point
// order within each of nsh splits): d_features += drho Y(dir), d_mu += drho (dY/ddir . f) ddir/dmu,
// dir = view direction of mu - p (preset convention; nlos_helpers / cuda_utils.cuh semantics as in
// the forward's pair_setup).  One lane per Gaussian; drho rows [P][ng] are read coalesced.
// ------------------------------------------------------------------------------------------
// KM: coefficient registers (16 up to degree 3, 25 for degree 4); partial rows of kShPart floats
template <int PRESET, int KM>
__global__ __launch_bounds__(kBlock) void sh_kernel(KArgs k) {
    const int gi = k.g_lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= k.g_hi) return;
    const int split = blockIdx.y;
    const int per = (k.pnw + k.nsh - 1) / k.nsh;
    const int pbeg = k.pb0 + split * per, pend = min(k.pb0 + k.pnw, pbeg + per);
    const int deg = k.g.sh_degree;
    const int K = (deg + 1) * (deg + 1);
    const GaussRec rec = k.recs[gi];
    const float mu[3] = {rec.a.x, rec.a.y, rec.a.z};
    float f[KM];
    load_feat<KM>(k.g, gi, f);
    float dF[KM], dMu[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < KM; ++c) dF[c] = 0.f;
    for (int p = pbeg; p < pend; ++p) {
        const float drho = k.drho[(size_t)(p - k.pb0) * k.g.ng + gi];
        if (drho == 0.f) continue;
        const float q[3] = {k.geo.wall[3 * p] - mu[0], k.geo.wall[3 * p + 1] - mu[1], k.geo.wall[3 * p + 2] - mu[2]};
        float dir[3], nrm;
        view_dir<PRESET>(-q[0], -q[1], -q[2], dir[0], dir[1], dir[2], nrm);
        float Y[KM];
        sh_basis<PRESET>(deg, dir[0], dir[1], dir[2], Y);
#pragma unroll
        for (int c = 0; c < KM; ++c)
            if (c < K) dF[c] += drho * Y[c];
        float gx, gy, gz;
        sh_grad_dir<PRESET>(deg, dir[0], dir[1], dir[2], f, gx, gy, gz);
        float ox, oy, oz;
        view_dir_bwd<PRESET>(-q[0], -q[1], -q[2], nrm, drho * gx, drho * gy, drho * gz, ox, oy, oz);
        dMu[0] += ox; dMu[1] += oy; dMu[2] += oz;
    }
    float* dst = k.shpart + ((size_t)split * k.g.ng + gi) * kShPart;
    if (k.accum) {
#pragma unroll
        for (int c = 0; c < KM; ++c) dst[c] += dF[c];
        dst[KM] += dMu[0]; dst[KM + 1] += dMu[1]; dst[KM + 2] += dMu[2];
    } else {
#pragma unroll
        for (int c = 0; c < KM; ++c) dst[c] = dF[c];
        dst[KM] = dMu[0]; dst[KM + 1] = dMu[1]; dst[KM + 2] = dMu[2];
    }
}

// ------------------------------------------------------------------------------------------
// finish: reduce the splits and chain dA / dsigma to the raw parameters
// ------------------------------------------------------------------------------------------
template <int PRESET, int KM>
__global__ __launch_bounds__(kBlock) void finish_kernel(KArgs k, float* d_mu, float* d_scaling, float* d_rot,
                                                        float* d_opac, float* d_feat) {
    const int i = k.g_lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k.g_hi) return;
    float acc[13 + KM];
    for (int t = 0; t < 13 + KM; ++t) acc[t] = 0.f;
    {
        // the wall-point splits' partials summed in fp64 (fixed order): the rotational shape sums are small
        // differences of the splits' contributions
        double sum[kBwdSlots];
        for (int t = 0; t < kBwdSlots; ++t) sum[t] = 0.0;
        for (int s = 0; s < k.nsplit; ++s) {
            const float* src = k.partial + ((size_t)s * k.g.ng + i) * kPartStride;
            for (int t = 0; t < kBwdSlots; ++t) sum[t] += (double)src[t];
        }
        for (int t = 0; t < kBwdSlots; ++t) acc[t] = (float)sum[t];
    }
    for (int s = 0; s < k.nsh; ++s) {   // view-direction chain (sh_kernel)
        const float* src = k.shpart + ((size_t)s * k.g.ng + i) * kShPart;
        for (int t = 0; t < KM; ++t) acc[13 + t] += src[t];
        for (int t = 0; t < 3; ++t) acc[9 + t] += src[KM + t];
    }
    chain_to_raw_shape<PRESET>(k.g, i, acc, acc + 3, d_scaling, d_rot);
    d_mu[3 * i] = acc[9]; d_mu[3 * i + 1] = acc[10]; d_mu[3 * i + 2] = acc[11];
    const float sg = 1.0f / (1.0f + expf(-k.g.opacity[i]));
    d_opac[i] = acc[12] * sg * (1.0f - sg);
    const int kf = k.g.k_feat;
    const int K = (k.g.sh_degree + 1) * (k.g.sh_degree + 1);
#pragma unroll
    for (int c = 0; c < KM; ++c)
        if (c < kf) d_feat[(size_t)i * kf + c] = c < K ? acc[13 + c] : 0.f;
}

template <int PRESET, int MODE, bool DENSE, bool RAYS, bool CACHE>
void launch_bwd(const KArgs& ka, size_t shm, hipStream_t s) {
    const int gpb = ka.bshared ? kNB * kWaves : kNB;
    dim3 grid((ka.g_hi - ka.g_lo + gpb - 1) / gpb, ka.nsplit);
    constexpr bool kCanTail = (MODE == NLOSGR_MODE_NOOCL || MODE == NLOSGR_MODE_NETF) && !DENSE && !RAYS;
    // NLOSGR_FLAG_MASKED_BWD: masked backward drains (A/B, parity cross-check)
    const bool tail = kCanTail && ka.opt.cutoff >= kTailCutoff && !(ka.opt.flags & NLOSGR_FLAG_MASKED_BWD) &&
                      (MODE != NLOSGR_MODE_NETF || ka.opt.c_deltaT <= kSmallX);
    if (ka.bshared) {
        if (tail) hipLaunchKernelGGL((bwd_kernel<PRESET, MODE, DENSE, RAYS, CACHE, true, kCanTail>), grid, dim3(kBlock), shm, s, ka);
        else hipLaunchKernelGGL((bwd_kernel<PRESET, MODE, DENSE, RAYS, CACHE, true>), grid, dim3(kBlock), shm, s, ka);
    } else {
        if (tail) hipLaunchKernelGGL((bwd_kernel<PRESET, MODE, DENSE, RAYS, CACHE, false, kCanTail>), grid, dim3(kBlock), shm, s, ka);
        else hipLaunchKernelGGL((bwd_kernel<PRESET, MODE, DENSE, RAYS, CACHE, false>), grid, dim3(kBlock), shm, s, ka);
    }
}

template <int PRESET, int MODE>
void dispatch_bwd(const KArgs& ka, bool dense, bool rays, size_t shm, hipStream_t s) {
    if (dense) {
        if (rays) launch_bwd<PRESET, MODE, true, true, false>(ka, shm, s);
        else launch_bwd<PRESET, MODE, true, false, false>(ka, shm, s);
    } else {
        if (rays) launch_bwd<PRESET, MODE, false, true, false>(ka, shm, s);
        else if (ka.cmask) launch_bwd<PRESET, MODE, false, false, true>(ka, shm, s);
        else launch_bwd<PRESET, MODE, false, false, false>(ka, shm, s);
    }
}

// the (PRESET, KM) variant of sh_kernel and finish_kernel: 25 coefficient registers only for the torch
// preset's degree 4.  launch(preset, km) gets both as integral constants.
template <class F>
void with_sh_variant(const nlosgr_gaussians& g, F&& launch) {
    using std::integral_constant;
    if (g.preset == NLOSGR_PRESET_TORCH && g.sh_degree == 4)
        launch(integral_constant<int, NLOSGR_PRESET_TORCH>{}, integral_constant<int, kMaxK4>{});
    else if (g.preset == NLOSGR_PRESET_TORCH)
        launch(integral_constant<int, NLOSGR_PRESET_TORCH>{}, integral_constant<int, kMaxK>{});
    else
        launch(integral_constant<int, NLOSGR_PRESET_CUDA>{}, integral_constant<int, kMaxK>{});
}

}  // namespace

namespace nlosgr {
namespace detail {

int volume_bwd_batch(const KArgs& ka, hipStream_t s) {
    const nlosgr_geometry* geo = &ka.geo;
    const nlosgr_options* opt = &ka.opt;
    const size_t shm = (size_t)BwdLayout(geo->nr, geo->nt, geo->np, ka.bshared != 0).total * sizeof(float);
    const bool dense = !(opt->cutoff > 0.f);
    const bool rays = ka.grad_ray != nullptr;
    if (ka.g.preset == NLOSGR_PRESET_TORCH) {
        if (opt->mode == NLOSGR_MODE_NOOCL) dispatch_bwd<0, 0>(ka, dense, rays, shm, s);
        else dispatch_bwd<0, 1>(ka, dense, rays, shm, s);
    } else {
        if (opt->mode == NLOSGR_MODE_NOOCL) dispatch_bwd<1, 0>(ka, dense, rays, shm, s);
        else dispatch_bwd<1, 1>(ka, dense, rays, shm, s);
    }
    HIPCHK(hipGetLastError());
    const dim3 shgrid((ka.g_hi - ka.g_lo + kBlock - 1) / kBlock, ka.nsh);
    with_sh_variant(ka.g, [&](auto preset, auto km) {
        hipLaunchKernelGGL((sh_kernel<decltype(preset)::value, decltype(km)::value>), shgrid, dim3(kBlock), 0, s, ka);
    });
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

int volume_bwd_finish(const KArgs& ka, float* d_mu, float* d_scaling, float* d_rotation, float* d_opacity,
                      float* d_features, hipStream_t s) {
    const int nb = (ka.g_hi - ka.g_lo + kBlock - 1) / kBlock;
    with_sh_variant(ka.g, [&](auto preset, auto km) {
        hipLaunchKernelGGL((finish_kernel<decltype(preset)::value, decltype(km)::value>), dim3(nb), dim3(kBlock), 0, s,
                           ka, d_mu, d_scaling, d_rotation, d_opacity, d_features);
    });
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

}  // namespace detail
}  // namespace nlosgr

#ifdef NLOSGR_BCOUNT
extern "C" __attribute__((visibility("default"))) int nlosgr_debug_bwd_counts(unsigned long long* out8) {
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_bdbg), 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
    const unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_bdbg), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}
#endif
