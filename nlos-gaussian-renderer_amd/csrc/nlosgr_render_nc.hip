// Non-confocal Gaussian renderer (gfx950): Gaussians -> transients of a capture whose laser spots differ from its
// sensed points, and the backward to the raw parameters.  No-occlusion, support selection, histogram only.
//
// Measurement p is sensed at s = wall[p] while the laser lights l = lasers[p]; bin k holds half the path, tau =
// r[k].  Rays leave the sensed point; with Delta = l - s, b^2 = |Delta|^2, c = omega . Delta the point of ray omega
// on the ellipsoid |x - s| + |x - l| = 2 tau is x = s + d omega,
//     D = tau - c/2,   d = tau + (c tau/2 - b^2/4) / D,   dl = 2 tau - d = |x - l|,
// and    hist[p,k] = hscale[p] att[k] sum_ij sin(theta_i) q sum_g w_g(p) pdf_g(x),   q = tau^2 / (dl D)
// (shell measure d^2 sin(theta) (dl / D) times the falloff 1 / (d^2 dl^2), over the confocal sin(theta) / tau^2
// that att already holds).  Bins with tau <= b/2 hold no path: exactly zero, no gradient.  l = s gives d = tau,
// q = 1: the confocal renderer.
//
// A Gaussian on a ray is still a 1-D Gaussian in d (nlosgr_volume.hpp: v = A omega, a, t*, m2min); only the sample
// positions d_k are non-uniform.  d grows with tau and tau(d) = (d + sqrt(d^2 - 2 d c + b^2)) / 2 inverts it, so
// the in-support bins of a ray are one range [kl, kh].
//
// One support: nc_pair_bins (the pair's cull), pair_setup's (theta, phi) box, nc_ray (the ray's [kl, kh]) and
// nc_sample (the bin's validity) are the only deciders, and both directions call them with the same fp32 inputs
// (no contraction inside them), so a (p, i, j, k, g) sample is in the backward iff it is in the forward.  A sample
// outside is never read or multiplied.
//
// Forward: one workgroup per measurement, thread = bin (a pass covers kNcBlock bins).  Per chunk of kNcBlock
//   Gaussians the threads cull in parallel (lane = Gaussian) and compact the survivors into LDS in index order;
//   after a barrier every wave walks the survivors whose bin range meets its 64 bins: its lanes set up the rays of
//   the box (lane = ray), then the passing rays are taken in (i, j) order, their quantities broadcast, each lane
//   adding its own bin's value into one register (fp32 within a batch of 64 rays, the batches in fp64).  The order
//   of a bin's sum is (g, i, j) ascending whatever the launch holds: no atomics, no LDS adds, a row depends on its measurement alone.
// Backward: one wave per Gaussian.  Lanes cull 64 measurements at a time; the wave walks the survivors in order,
//   lanes take the box's rays (cell = lane, lane + 64, ...) and run their bins serially, accumulating the whitened
//   moments U1 = sum c pdf u, U2 = sum c pdf u u^T (c = w W, W the sample's upstream weight) and the pair's
//   P = sum W pdf; P is butterflied per pair and goes through the SH basis in the same wave (dL/drho = sigma P), so
//   no [P][ng] buffer exists.  A fixed butterfly, then nc_finish: dL/dmu = A^T U1 + the SH part, the shape chain
//   from U2 (chain_to_raw_shape), the opacity chain.  A Gaussian's rows depend on that Gaussian alone.
#include "nlosgr_volume.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

constexpr int kNcBlock = 1024;            // forward: threads = bins per pass = Gaussians per cull chunk
constexpr int kNcWaves = kNcBlock / 64;
constexpr int kNcSums = 16;               // backward sums per Gaussian: U1[3], U2[6], dsigma, dmu_sh[3], skipped, pad

struct NArgs {
    KArgs k;               // g, geo, opt, recs, hist_out / grad_hist
    const float* lasers;   // [nlaser][3]
    int nlaser;            // 1 or nwall
    float* sums;           // backward: [ng][kNcSums]
};

// what a measurement adds to the geometry's tables
struct Meas {
    float s[3], dl[3];     // sensed point, Delta = l - s
    float l[3];
    float b2, halfb;       // |Delta|^2, |Delta| / 2
    float r0, inv_dr;
    int nr;
};

__device__ __forceinline__ void load_meas(const NArgs& n, int p, Meas& m) {
#pragma clang fp contract(off)
    const int lp = n.nlaser == 1 ? 0 : p;
    for (int c = 0; c < 3; ++c) {
        m.s[c] = n.k.geo.wall[3 * (size_t)p + c];
        m.l[c] = n.lasers[3 * (size_t)lp + c];
        m.dl[c] = m.l[c] - m.s[c];
    }
    m.b2 = (m.dl[0] * m.dl[0] + m.dl[1] * m.dl[1]) + m.dl[2] * m.dl[2];
    m.halfb = 0.5f * sqrtf(m.b2);
    const int nr = n.k.geo.nr;
    m.nr = nr;
    m.r0 = n.k.geo.r[0];
    const float dr = nr > 1 ? (n.k.geo.r[nr - 1] - m.r0) / (float)(nr - 1) : 0.f;
    m.inv_dr = dr > 0.f ? 1.0f / dr : 0.f;
}

// every float of the record is finite (a Gaussian with NaN / inf parameters is skipped in culled mode)
__device__ __forceinline__ bool rec_finite(const GaussRec& r) {
    const float s = (fabsf(r.a.x) + fabsf(r.a.y) + fabsf(r.a.z) + fabsf(r.a.w)) + (fabsf(r.b.x) + fabsf(r.b.y) + fabsf(r.b.z) + fabsf(r.b.w)) +
                    (fabsf(r.c.x) + fabsf(r.c.y) + fabsf(r.c.z) + fabsf(r.c.w)) + (fabsf(r.d.x) + fabsf(r.d.y) + fabsf(r.d.z) + fabsf(r.d.w)) +
                    (fabsf(r.e.x) + fabsf(r.e.y) + fabsf(r.e.z) + fabsf(r.e.w));
    return s < __builtin_inff();
}

// u0 = A (s - mu), as the rays of both directions use it
__device__ __forceinline__ void nc_u0(const float* A, const float* q, float* u0) {
#pragma clang fp contract(off)
    for (int r = 0; r < 3; ++r) u0[r] = (A[3 * r] * q[0] + A[3 * r + 1] * q[1]) + A[3 * r + 2] * q[2];
}

// The pair's cull: the bins the bounding sphere (centre mu, radius Rb) can reach.  Every point of it has a half
// path within Rb of the centre's, so [klo, khi] holds every in-support bin of every ray (one bin of margin on each
// side); false: the pair has none.  Dense: all bins.
template <bool DENSE>
__device__ __forceinline__ bool nc_pair_bins(const float* q, const float* mu, float smax, float cutoff, const Meas& m,
                                             int& klo, int& khi) {
#pragma clang fp contract(off)
    klo = 0; khi = m.nr - 1;
    if (DENSE) return true;
    const float Rb = cutoff * smax * 1.0001f + 1e-7f;
    const float ds = sqrtf((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    const float ex = m.l[0] - mu[0], ey = m.l[1] - mu[1], ez = m.l[2] - mu[2];
    const float dl = sqrtf((ex * ex + ey * ey) + ez * ez);
    const float gc = 0.5f * (ds + dl);
    const float wide = Rb + 1e-5f * gc;
    klo = fidx(floorf((gc - wide - m.r0) * m.inv_dr) - 1.0f, 0, m.nr);
    khi = fidx(ceilf((gc + wide - m.r0) * m.inv_dr) + 1.0f, -1, m.nr - 1);
    return klo <= khi;
}

// Ray quantities (ray_setup's quadratic in the distance d from the sensed point) and THE bin range of the ray.
struct NcRay {
    float v[3], a, ts, zs[3], m2min, c;
    int kl, kh;
};

__device__ __forceinline__ float nc_tau_of(float d, float c, float b2) {
#pragma clang fp contract(off)
    const float rad = fmaxf((d * d - (2.0f * d) * c) + b2, 0.0f);
    return 0.5f * (d + fsqrt(rad));
}

template <bool DENSE>
__device__ __forceinline__ bool nc_ray(const float* A, const float* u0, float wx, float wy, float wz, float mc2,
                                       const Meas& m, NcRay& R) {
#pragma clang fp contract(off)
    for (int r = 0; r < 3; ++r) R.v[r] = (A[3 * r] * wx + A[3 * r + 1] * wy) + A[3 * r + 2] * wz;
    R.a = (R.v[0] * R.v[0] + R.v[1] * R.v[1]) + R.v[2] * R.v[2];
    const float bq = (u0[0] * R.v[0] + u0[1] * R.v[1]) + u0[2] * R.v[2];
    const float ia = frcp(R.a);
    R.ts = -bq * ia;
    for (int r = 0; r < 3; ++r) R.zs[r] = u0[r] + R.ts * R.v[r];
    R.m2min = (R.zs[0] * R.zs[0] + R.zs[1] * R.zs[1]) + R.zs[2] * R.zs[2];
    R.c = (wx * m.dl[0] + wy * m.dl[1]) + wz * m.dl[2];
    R.kl = 0; R.kh = m.nr - 1;
    if (DENSE) return true;
    if (!(R.m2min <= mc2)) return false;
    const float h = fsqrt((mc2 - R.m2min) * ia);
    const float dlo = R.ts - h, dhi = R.ts + h;
    if (!(dhi > 0.0f)) return false;          // the support lies behind the wall
    // d <= 0 is tau <= b/2: no bin below is valid, so the range starts at bin 0
    if (dlo > 0.0f) R.kl = fidx(ceilf((nc_tau_of(dlo, R.c, m.b2) - m.r0) * m.inv_dr), 0, m.nr);
    R.kh = fidx(floorf((nc_tau_of(dhi, R.c, m.b2) - m.r0) * m.inv_dr), -1, m.nr - 1);
    return R.kl <= R.kh;
}

// The sample of a ray (c = omega . Delta) in the bin of half path tau: false where no path exists (tau <= b/2); else
// its distance d from the sensed point and its weight q (hardware reciprocals, 1 ulp: l = s gives d = tau exactly
// and q = 1 to that ulp).
__device__ __forceinline__ bool nc_sample(float c, const Meas& m, float tau, float& d, float& q) {
#pragma clang fp contract(off)
    if (!(tau > m.halfb)) return false;
    const float D = tau - 0.5f * c;
    if (!(D > 0.0f)) return false;            // (|c| <= b, so D >= tau - b/2 > 0 but for rounding)
    d = tau + ((0.5f * c) * tau - 0.25f * m.b2) * frcp(D);
    const float dl = 2.0f * tau - d;
    q = (tau * tau) * frcp(dl * D);
    return true;
}

// the 1-D Gaussian of the ray at distance d
__device__ __forceinline__ float nc_pdf(float a, float ts, float m2min, float d) {
    const float t = d - ts;
    return fast_exp2(-kHalfLog2e * fmaf(a * t, t, m2min));
}

__device__ __forceinline__ int rfl(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ float rdl(float x, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
}
__device__ __forceinline__ float rflf(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
template <int PRESET, bool DENSE>
__global__ __launch_bounds__(kNcBlock) void nc_fwd_kernel(NArgs n) {
    __shared__ int s_g[kNcBlock];
    __shared__ float s_w[kNcBlock];
    __shared__ unsigned s_bi[kNcBlock], s_bj[kNcBlock], s_bk[kNcBlock];
    __shared__ int s_cnt[kNcWaves];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const nlosgr_geometry& geo = n.k.geo;
    const int nr = geo.nr, nt = geo.nt, np_ = geo.np, ng = n.k.g.ng, kf = n.k.g.k_feat;
    Meas m;
    load_meas(n, p, m);
    const float* lin = geo.grid_lin + 4 * (size_t)p;
    const float* sth = geo.sin_theta + (size_t)p * nt;
    const float* cth = geo.cos_theta + (size_t)p * nt;
    const float* sph = geo.sin_phi + (size_t)p * np_;
    const float* cph = geo.cos_phi + (size_t)p * np_;
    const float cutoff = n.k.opt.cutoff, mc2 = cutoff * cutoff;
    const float hs = geo.hscale[p];

    for (int kb = 0; kb < nr; kb += kNcBlock) {   // a pass: bins [kb, kb + kNcBlock)
        const int k = kb + tid;
        const bool live = k < nr;
        const float tau = live ? geo.r[k] : 0.f;
        const int wk0 = kb + wave * 64, wk1 = min(wk0 + 63, nr - 1);   // this wave's bins
        const int pk1 = min(kb + kNcBlock - 1, nr - 1);
        // a bin's total is kept in fp64: a running fp32 total over every (Gaussian, ray) drops the terms below half
        // an ulp of the bin (measured 1.7e-3 low on 2000 broad Gaussians x 1024 rays); each batch of up to 64 rays
        // is summed in fp32 and folded in, as fwd_dense_kernel does
        double acc = 0.0;
        for (int c0 = 0; c0 < ng; c0 += kNcBlock) {
            // cull, lane = Gaussian
            const int gi = c0 + tid;
            bool keep = false;
            float w = 0.f;
            unsigned bi = 0, bj = 0, bk = 0;
            if (gi < ng) {
                const GaussRec rec = n.k.recs[gi];
                if (DENSE || rec_finite(rec)) {
                    Pair P;
                    float mu[3];
                    load_rec(rec, P, mu);
                    pair_setup<PRESET, DENSE>(n.k, n.k.g.features + (size_t)gi * kf, mu, m.s[0], m.s[1], m.s[2], lin, mc2, P);
                    int klo, khi;
                    keep = nc_pair_bins<DENSE>(P.q, mu, P.smax, cutoff, m, klo, khi) && P.i0 <= P.i1 && P.j0 <= P.j1 &&
                           (DENSE ? !(P.sh + 0.5f < 0.f) : P.w > 0.f) && klo <= pk1 && khi >= kb;
                    w = P.w;
                    bi = (unsigned)P.i0 | ((unsigned)P.i1 << 16);
                    bj = (unsigned)P.j0 | ((unsigned)P.j1 << 16);
                    bk = (unsigned)klo | ((unsigned)khi << 16);
                }
            }
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(keep);
            if (lane == 0) s_cnt[wave] = __popcll(bal);
            __syncthreads();
            int base = 0, total = 0;
            for (int wv = 0; wv < kNcWaves; ++wv) {
                const int cn = s_cnt[wv];
                base += wv < wave ? cn : 0;
                total += cn;
            }
            if (keep) {
                const int slot = base + lanes_below(bal);
                s_g[slot] = gi; s_w[slot] = w; s_bi[slot] = bi; s_bj[slot] = bj; s_bk[slot] = bk;
            }
            __syncthreads();
            // walk, lane = bin
            total = rfl(total);
            if (wk0 < nr) {
                for (int s = 0; s < total; ++s) {
                    const unsigned ubk = (unsigned)rfl((int)s_bk[s]);
                    const int klo = (int)(ubk & 0xFFFFu), khi = (int)(ubk >> 16);
                    if (khi < wk0 || klo > wk1) continue;
                    const int sg = rfl(s_g[s]);
                    const float wg = rflf(s_w[s]);
                    const unsigned ubi = (unsigned)rfl((int)s_bi[s]), ubj = (unsigned)rfl((int)s_bj[s]);
                    const int i0 = (int)(ubi & 0xFFFFu), i1 = (int)(ubi >> 16), j0 = (int)(ubj & 0xFFFFu), j1 = (int)(ubj >> 16);
                    Pair P;
                    float mu[3], q[3], u0[3];
                    load_rec(n.k.recs[sg], P, mu);
                    for (int c = 0; c < 3; ++c) q[c] = m.s[c] - mu[c];
                    nc_u0(P.A, q, u0);
                    // lanes set up the box's rays, 64 cells at a time ((i, j) order); the passing rays whose range
                    // meets this wave's bins are then taken in that order, each lane adding its own bin's sample
                    const int nj = j1 - j0 + 1, ncell = (i1 - i0 + 1) * nj;
                    for (int cell0 = 0; cell0 < ncell; cell0 += 64) {
                        const int cell = cell0 + lane;
                        const bool valid = cell < ncell;
                        const int ii = valid ? cell / nj : 0;
                        const int i = i0 + ii, j = valid ? j0 + (cell - ii * nj) : j0;
                        const float st = sth[i], ct = cth[i];
                        NcRay R;
                        const bool ok = nc_ray<DENSE>(P.A, u0, st * cph[j], st * sph[j], ct, mc2, m, R) && valid &&
                                        R.kh >= wk0 && R.kl <= wk1;
                        const float ws = wg * st;
                        unsigned long long rm = __builtin_amdgcn_ballot_w64(ok);
                        float part = 0.f;
                        while (rm) {
                            const int src = (int)__builtin_ctzll(rm);
                            rm &= rm - 1ull;
                            const int kl = __builtin_amdgcn_readlane(R.kl, src), kh = __builtin_amdgcn_readlane(R.kh, src);
                            const float ra = rdl(R.a, src), rts = rdl(R.ts, src), rm2 = rdl(R.m2min, src);
                            const float rc = rdl(R.c, src), rws = rdl(ws, src);
                            float d, qq;
                            if (live && k >= kl && k <= kh && nc_sample(rc, m, tau, d, qq))
                                part = fmaf(rws * qq, nc_pdf(ra, rts, rm2, d), part);
                        }
                        acc += (double)part;
                    }
                }
            }
            __syncthreads();   // the next chunk overwrites the survivors
        }
        if (live) n.k.hist_out[(size_t)p * nr + k] = hs * geo.att[k] * (float)acc;
    }
}

// ------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------
template <int PRESET, bool DENSE>
__global__ __launch_bounds__(kBlock) void nc_bwd_kernel(NArgs n, float* __restrict__ d_feat) {
    constexpr int MAXK = PRESET == NLOSGR_PRESET_TORCH ? kMaxK4 : kMaxK;
    const int lane = lane_id();
    const int gi = blockIdx.x * kWaves + (threadIdx.x >> 6);
    const nlosgr_geometry& geo = n.k.geo;
    const int ng = n.k.g.ng, kf = n.k.g.k_feat, deg = n.k.g.sh_degree;
    if (gi >= ng) return;   // waves never meet at a barrier
    const int nr = geo.nr, nt = geo.nt, np_ = geo.np, nmeas = geo.nwall;
    const float cutoff = n.k.opt.cutoff, mc2 = cutoff * cutoff;
    float* sums = n.sums + (size_t)gi * kNcSums;
    const GaussRec rec = n.k.recs[gi];
    if (!DENSE && !rec_finite(rec)) {   // skipped, as the forward skips it
        if (lane < kNcSums) sums[lane] = lane == 13 ? 1.0f : 0.0f;
        for (int c = lane; c < kf; c += 64) d_feat[(size_t)gi * kf + c] = 0.f;
        return;
    }
    Pair P;
    float mu[3];
    load_rec(rec, P, mu);
    const float sigma = P.sigma;
    const float* f = n.k.g.features + (size_t)gi * kf;
    float U1[3] = {0.f, 0.f, 0.f}, U2[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // per lane
    float dsig = 0.f, dmush[3] = {0.f, 0.f, 0.f}, dfe[MAXK];                  // wave-uniform
#pragma unroll
    for (int c = 0; c < MAXK; ++c) dfe[c] = 0.f;

    for (int p0 = 0; p0 < nmeas; p0 += 64) {
        // cull, lane = measurement
        const int pl = p0 + lane;
        bool keep = false;
        if (pl < nmeas) {
            Meas ml;
            load_meas(n, pl, ml);
            pair_setup<PRESET, DENSE>(n.k, f, mu, ml.s[0], ml.s[1], ml.s[2], geo.grid_lin + 4 * (size_t)pl, mc2, P);
            int klo, khi;
            keep = nc_pair_bins<DENSE>(P.q, mu, P.smax, cutoff, ml, klo, khi) && P.i0 <= P.i1 && P.j0 <= P.j1 &&
                   !(P.sh + 0.5f < 0.f);
        }
        unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
        while (mask) {
            const int src = (int)__builtin_ctzll(mask);
            mask &= mask - 1ull;
            const int pp = p0 + src;
            Meas m;
            load_meas(n, pp, m);
            const int i0 = __shfl(P.i0, src), i1 = __shfl(P.i1, src), j0 = __shfl(P.j0, src), j1 = __shfl(P.j1, src);
            const float rho = __shfl(P.rho, src), nrm = __shfl(P.nrm, src);
            const float dx = __shfl(P.dir[0], src), dy = __shfl(P.dir[1], src), dz = __shfl(P.dir[2], src);
            float q[3], u0[3];
            for (int c = 0; c < 3; ++c) q[c] = m.s[c] - mu[c];
            nc_u0(P.A, q, u0);
            const float w = sigma * rho;
            const float* G = n.k.grad_hist + (size_t)pp * nr;
            const float hs = geo.hscale[pp];
            const float* sth = geo.sin_theta + (size_t)pp * nt;
            const float* cth = geo.cos_theta + (size_t)pp * nt;
            const float* sph = geo.sin_phi + (size_t)pp * np_;
            const float* cph = geo.cos_phi + (size_t)pp * np_;
            const int nj = j1 - j0 + 1, ncell = (i1 - i0 + 1) * nj;
            float Pp = 0.f;
            for (int cell = lane; cell < ncell; cell += 64) {
                const int ii = cell / nj;
                const int i = i0 + ii, j = j0 + (cell - ii * nj);
                const float st = sth[i], ct = cth[i];
                NcRay R;
                if (!nc_ray<DENSE>(P.A, u0, st * cph[j], st * sph[j], ct, mc2, m, R)) continue;
                const float hst = hs * st;
                for (int k = R.kl; k <= R.kh; ++k) {
                    float d, qq;
                    if (!nc_sample(R.c, m, geo.r[k], d, qq)) continue;
                    const float pw = ((G[k] * geo.att[k]) * (hst * qq)) * nc_pdf(R.a, R.ts, R.m2min, d);
                    Pp += pw;
                    const float cp = w * pw;
                    const float t = d - R.ts;
                    const float ux = fmaf(t, R.v[0], R.zs[0]), uy = fmaf(t, R.v[1], R.zs[1]), uz = fmaf(t, R.v[2], R.zs[2]);
                    const float cx = cp * ux, cy = cp * uy, cz = cp * uz;
                    U1[0] += cx; U1[1] += cy; U1[2] += cz;
                    U2[0] = fmaf(cx, ux, U2[0]);
                    U2[1] = fmaf(cx, uy, U2[1]);
                    U2[2] = fmaf(cx, uz, U2[2]);
                    U2[3] = fmaf(cy, uy, U2[3]);
                    U2[4] = fmaf(cy, uz, U2[4]);
                    U2[5] = fmaf(cz, uz, U2[5]);
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) Pp += __shfl_xor(Pp, off);
            // the pair's albedo: dL/dsigma += rho P, dL/drho = sigma P through the SH basis and the view direction
            dsig = fmaf(rho, Pp, dsig);
            const float gr = sigma * Pp;
            if (gr != 0.f) {
                float Y[MAXK];
                sh_basis<PRESET>(deg, dx, dy, dz, Y);
                const int K = (deg + 1) * (deg + 1);
#pragma unroll
                for (int c = 0; c < MAXK; ++c)
                    if (c < K) dfe[c] = fmaf(gr, Y[c], dfe[c]);
                if (deg > 0) {
                    float gx, gy, gz, ox, oy, oz;
                    sh_grad_dir<PRESET>(deg, dx, dy, dz, f, gx, gy, gz);
                    view_dir_bwd<PRESET>(-q[0], -q[1], -q[2], nrm, gr * gx, gr * gy, gr * gz, ox, oy, oz);
                    dmush[0] += ox; dmush[1] += oy; dmush[2] += oz;
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) U1[t] += __shfl_xor(U1[t], off);
#pragma unroll
    for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) U2[t] += __shfl_xor(U2[t], off);
    if (lane == 0) {
        sums[0] = U1[0]; sums[1] = U1[1]; sums[2] = U1[2];
#pragma unroll
        for (int t = 0; t < 6; ++t) sums[3 + t] = U2[t];
        sums[9] = dsig;
        sums[10] = dmush[0]; sums[11] = dmush[1]; sums[12] = dmush[2];
        sums[13] = 0.f; sums[14] = 0.f; sums[15] = 0.f;
        const int K = (deg + 1) * (deg + 1);
#pragma unroll
        for (int c = 0; c < MAXK; ++c)
            if (c < kf) d_feat[(size_t)gi * kf + c] = c < K ? dfe[c] : 0.f;
    }
}

// one lane per Gaussian: the sums -> the raw parameters' gradients (d_features is already written)
template <int PRESET>
__global__ __launch_bounds__(kBlock) void nc_finish(nlosgr_gaussians g, const GaussRec* __restrict__ recs,
                                                   const float* __restrict__ sums, float* d_mu, float* d_scaling,
                                                   float* d_rot, float* d_opac) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.ng) return;
    const float* S = sums + (size_t)i * kNcSums;
    if (S[13] != 0.f) {   // skipped
        for (int c = 0; c < 3; ++c) d_mu[3 * i + c] = d_scaling[3 * i + c] = 0.f;
        for (int c = 0; c < 4; ++c) d_rot[4 * i + c] = 0.f;
        d_opac[i] = 0.f;
        return;
    }
    const GaussRec rec = recs[i];
    const float A[9] = {rec.b.x, rec.b.y, rec.b.z, rec.b.w, rec.c.x, rec.c.y, rec.c.z, rec.c.w, rec.d.x};
    // dL/dmu = A^T U1 (pdf's gradient in mu is pdf A^T u) plus the albedo's through the view direction
    for (int c = 0; c < 3; ++c) d_mu[3 * i + c] = (A[c] * S[0] + A[3 + c] * S[1] + A[6 + c] * S[2]) + S[10 + c];
    const float sg = 1.0f / (1.0f + expf(-g.opacity[i]));
    d_opac[i] = S[9] * sg * (1.0f - sg);
    // dL/dA = -sum c pdf u d^T: in shape_acc's terms g = -c pdf u, w = u, so with W = U2 (whitened second moment)
    // D_r = -W_rr and K~ = -(ratio differences) x W's off-diagonals (the voxelizer backward's finish)
    const float W01 = S[4], W02 = S[5], W12 = S[7];
    const float n1 = A[0] * A[0] + A[1] * A[1] + A[2] * A[2];
    const float n2 = A[3] * A[3] + A[4] * A[4] + A[5] * A[5];
    const float n3 = A[6] * A[6] + A[7] * A[7] + A[8] * A[8];
    const float d32 = n1 * (n2 - n3) / (n2 * n3), d13 = (n3 - n1) / n3, d21 = (n1 - n2) / n2;
    const float D[3] = {-S[3], -S[6], -S[8]};
    const float K[3] = {-d32 * W12, -d13 * W02, -d21 * W01};
    chain_to_raw_shape<PRESET>(g, i, D, K, d_scaling, d_rot);
}

// workspace: GaussRec [ng] | sums [ng][kNcSums]
struct NcLayout {
    size_t off_sums, total;
    explicit NcLayout(int ng) {
        off_sums = align_up((size_t)ng * sizeof(GaussRec));
        total = off_sums + align_up((size_t)ng * kNcSums * sizeof(float)) + 256;
    }
};

int validate_nc(const nlosgr_gaussians* g, const nlosgr_geometry* geo, const float* lasers, int nlaser, bool need_lasers,
                const nlosgr_options* opt) {
    if (!g || !geo || !opt) return set_err(NLOSGR_E_INVALID, "null argument struct");
    if (g->ng < 0) return set_err(NLOSGR_E_INVALID, "ng must be >= 0");
    if (g->preset != NLOSGR_PRESET_TORCH && g->preset != NLOSGR_PRESET_CUDA)
        return set_err(NLOSGR_E_INVALID, "unknown preset");
    const int max_deg = g->preset == NLOSGR_PRESET_TORCH ? 4 : 3;
    if (g->sh_degree < 0 || g->sh_degree > max_deg)
        return set_err(NLOSGR_E_UNSUPPORTED, g->preset == NLOSGR_PRESET_TORCH ? "active_sh_degree must be in [0, 4]"
                                                                              : "active_sh_degree must be in [0, 3] (cuda preset)");
    const int max_k = g->preset == NLOSGR_PRESET_TORCH ? kMaxK4 : kMaxK;
    if (g->k_feat < (g->sh_degree + 1) * (g->sh_degree + 1) || g->k_feat > max_k)
        return set_err(NLOSGR_E_INVALID, g->preset == NLOSGR_PRESET_TORCH ? "k_feat must satisfy (sh_degree+1)^2 <= k_feat <= 25"
                                                                           : "k_feat must satisfy (sh_degree+1)^2 <= k_feat <= 16");
    if (opt->mode != NLOSGR_MODE_NOOCL)
        return set_err(NLOSGR_E_UNSUPPORTED, "non-confocal renderer: NLOSGR_MODE_NOOCL only");
    if (opt->selection != NLOSGR_SELECT_SUPPORT)
        return set_err(NLOSGR_E_UNSUPPORTED, "non-confocal renderer: NLOSGR_SELECT_SUPPORT only");
    if (opt->ray_cache != 0) return set_err(NLOSGR_E_UNSUPPORTED, "non-confocal renderer: no ray cache (ray_cache must be 0)");
    if (opt->nsplit != 0 || opt->g_begin != 0 || opt->g_end != 0 || opt->flags != 0)
        return set_err(NLOSGR_E_INVALID, "non-confocal renderer: nsplit, g_begin, g_end and flags must be 0");
    if (geo->nwall < 0 || geo->nt < 1 || geo->np < 1 || geo->nr < 1)
        return set_err(NLOSGR_E_INVALID, "bad geometry sizes");
    if (geo->nr > 4096 || geo->nt > 1024 || geo->np > 1024)
        return set_err(NLOSGR_E_UNSUPPORTED, "nr <= 4096 and nt, np <= 1024");
    if (g->ng > 0 && (!g->mu || !g->scaling || !g->rotation || !g->opacity || !g->features))
        return set_err(NLOSGR_E_INVALID, "null Gaussian parameter pointer");
    if (geo->nwall > 0 && (!geo->wall || !geo->sin_theta || !geo->cos_theta || !geo->sin_phi || !geo->cos_phi ||
                           !geo->grid_lin || !geo->hscale || !geo->r || !geo->att))
        return set_err(NLOSGR_E_INVALID, "null geometry pointer");
    if (nlaser != 1 && nlaser != geo->nwall)
        return set_err(NLOSGR_E_INVALID, "nlaser must be 1 (one spot for the capture) or nmeas (one per measurement)");
    if (need_lasers && !lasers) return set_err(NLOSGR_E_INVALID, "null lasers pointer");
    return NLOSGR_OK;
}

void fill_args(NArgs& n, const nlosgr_gaussians* g, const nlosgr_geometry* geo, const float* lasers, int nlaser,
               const nlosgr_options* opt, void* workspace) {
    memset(&n, 0, sizeof(n));
    n.k.g = *g; n.k.geo = *geo; n.k.opt = *opt;
    n.k.recs = (const GaussRec*)workspace;
    n.lasers = lasers; n.nlaser = nlaser;
    n.sums = (float*)((char*)workspace + NcLayout(g->ng).off_sums);
}

}  // namespace

extern "C" {

size_t nlosgr_render_nc_workspace_bytes(const nlosgr_gaussians* g, const nlosgr_geometry* geo, int32_t nlaser,
                                        const nlosgr_options* opt) {
    if (validate_nc(g, geo, nullptr, nlaser, false, opt) != NLOSGR_OK) return 0;
    return NcLayout(g->ng).total;
}

int nlosgr_render_nc_fwd(const nlosgr_gaussians* g, const nlosgr_geometry* geo, const float* lasers, int32_t nlaser,
                         const nlosgr_options* opt, void* workspace, float* hist_out, void* hip_stream) {
    const int rc = validate_nc(g, geo, lasers, nlaser, true, opt);
    if (rc) return rc;
    if (geo->nwall == 0) return NLOSGR_OK;
    if (!hist_out) return set_err(NLOSGR_E_INVALID, "null hist_out");
    hipStream_t s = (hipStream_t)hip_stream;
    if (g->ng == 0) {
        HIPCHK(hipMemsetAsync(hist_out, 0, (size_t)geo->nwall * geo->nr * sizeof(float), s));
        return NLOSGR_OK;
    }
    if (!workspace) return set_err(NLOSGR_E_INVALID, "workspace is null");
    NArgs n;
    fill_args(n, g, geo, lasers, nlaser, opt, workspace);
    n.k.hist_out = hist_out;
    launch_preprocess(g, (GaussRec*)workspace, s);
    const bool dense = !(opt->cutoff > 0.0f);
    const dim3 grid((unsigned)geo->nwall), block(kNcBlock);
    if (g->preset == NLOSGR_PRESET_TORCH) {
        if (dense) hipLaunchKernelGGL((nc_fwd_kernel<NLOSGR_PRESET_TORCH, true>), grid, block, 0, s, n);
        else hipLaunchKernelGGL((nc_fwd_kernel<NLOSGR_PRESET_TORCH, false>), grid, block, 0, s, n);
    } else {
        if (dense) hipLaunchKernelGGL((nc_fwd_kernel<NLOSGR_PRESET_CUDA, true>), grid, block, 0, s, n);
        else hipLaunchKernelGGL((nc_fwd_kernel<NLOSGR_PRESET_CUDA, false>), grid, block, 0, s, n);
    }
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

int nlosgr_render_nc_bwd(const nlosgr_gaussians* g, const nlosgr_geometry* geo, const float* lasers, int32_t nlaser,
                         const nlosgr_options* opt, void* workspace, const float* grad_hist, float* d_mu,
                         float* d_scaling, float* d_rotation, float* d_opacity, float* d_features, void* hip_stream) {
    const int rc = validate_nc(g, geo, lasers, nlaser, true, opt);
    if (rc) return rc;
    if (g->ng == 0) return NLOSGR_OK;
    if (!d_mu || !d_scaling || !d_rotation || !d_opacity || !d_features)
        return set_err(NLOSGR_E_INVALID, "null gradient output pointer");
    if (!workspace) return set_err(NLOSGR_E_INVALID, "workspace is null");
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t ng = (size_t)g->ng;
    if (geo->nwall == 0 || !grad_hist) {
        HIPCHK(hipMemsetAsync(d_mu, 0, ng * 3 * sizeof(float), s));
        HIPCHK(hipMemsetAsync(d_scaling, 0, ng * 3 * sizeof(float), s));
        HIPCHK(hipMemsetAsync(d_rotation, 0, ng * 4 * sizeof(float), s));
        HIPCHK(hipMemsetAsync(d_opacity, 0, ng * sizeof(float), s));
        HIPCHK(hipMemsetAsync(d_features, 0, ng * g->k_feat * sizeof(float), s));
        return NLOSGR_OK;
    }
    NArgs n;
    fill_args(n, g, geo, lasers, nlaser, opt, workspace);
    n.k.grad_hist = grad_hist;
    launch_preprocess(g, (GaussRec*)workspace, s);
    const bool dense = !(opt->cutoff > 0.0f);
    const dim3 grid((unsigned)((g->ng + kWaves - 1) / kWaves)), block(kBlock);
    const dim3 gridf((unsigned)((g->ng + kBlock - 1) / kBlock));
    if (g->preset == NLOSGR_PRESET_TORCH) {
        if (dense) hipLaunchKernelGGL((nc_bwd_kernel<NLOSGR_PRESET_TORCH, true>), grid, block, 0, s, n, d_features);
        else hipLaunchKernelGGL((nc_bwd_kernel<NLOSGR_PRESET_TORCH, false>), grid, block, 0, s, n, d_features);
        hipLaunchKernelGGL(nc_finish<NLOSGR_PRESET_TORCH>, gridf, block, 0, s, *g, n.k.recs, n.sums, d_mu, d_scaling,
                           d_rotation, d_opacity);
    } else {
        if (dense) hipLaunchKernelGGL((nc_bwd_kernel<NLOSGR_PRESET_CUDA, true>), grid, block, 0, s, n, d_features);
        else hipLaunchKernelGGL((nc_bwd_kernel<NLOSGR_PRESET_CUDA, false>), grid, block, 0, s, n, d_features);
        hipLaunchKernelGGL(nc_finish<NLOSGR_PRESET_CUDA>, gridf, block, 0, s, *g, n.k.recs, n.sums, d_mu, d_scaling,
                           d_rotation, d_opacity);
    }
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

}  // extern "C"
