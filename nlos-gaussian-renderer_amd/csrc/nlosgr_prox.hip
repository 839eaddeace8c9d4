// Primal-dual passes (Chambolle-Pock, theta = 1; gfx950): the three passes of one iteration that are not an operator
// application, for   min_v F(A v) + tv sum |a o grad v|_2 + l1 sum |v|   (include/nlosgr.h, "Primal-dual passes").
// The volume is [W][nr][H], axes (n, j, m), P = nr H the plane of one wall column; rows are [H W][nr].
//
//   nlosgr_prox_rows   q <- prox_{sigma F*}(q + sigma z), F the MSE or the Poisson term with a per-bin exposure; emits
//                      F(z) per workgroup.
//   nlosgr_tv_dual     p <- project_{|p|_2 <= tv}(p + sigma a o grad xbar); emits sum |a o grad xbar|_2 and sum |xbar|.
//   nlosgr_tv_primal   u = x - tau (g + (a o grad)^T p); x+ = shrink(u, tau l1), clamped at 0 with nonneg;
//                      xbar <- 2 x+ - x; x <- x+.
//
// Shape.  One launch each, everything in place, one writer per element, no atomics.  The two volume passes give a
// workgroup 1024 consecutive elements of one wall column's (j, m) plane, four per lane, so the lanes run along the
// flattened plane whatever H is: the neighbours along m and j are at +-1 and +-H of the same plane and come from an
// LDS image of the tile and its halo of H elements (read once, coalesced); the neighbour along n is the same plane
// position of the next (dual) or previous (primal) column, 16 bytes a lane straight from memory: the workgroup of
// that column reads the same lines as its own tile at about the same time, so the second read is served by the
// caches, not by HBM.  Where P is a multiple of 4 and the arrays are 16-byte aligned every global access is 16 bytes
// a lane; otherwise the same lanes use 4-byte accesses (the same arithmetic, the same bits).  The rows pass is
// elementwise: 4096 consecutive elements a workgroup, four per lane.
//
// The objective's terms are formed in double from the fp32 inputs, summed per lane in element order, over the wave
// by a butterfly, over the four waves in order, and written as one double (rows) or two (dual) per workgroup: the
// caller adds the partials in a fixed order.  Bitwise repeatable.
#include <initializer_list>

#include "nlosgr_common.hpp"
#include "nlosgr_lattice.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

constexpr int kProxPerLane = 4;
constexpr int kProxTile = kBlock * kProxPerLane;      // volume passes: plane elements per workgroup
constexpr int kProxRowsChunk = 4 * kProxTile;         // rows pass: elements per workgroup
constexpr int kProxHalo = kLatticeMaxExtent;          // H <= 1024

// the sum of v over the workgroup in a fixed order (every lane returns it); sh: kWaves doubles
__device__ __forceinline__ double prox_block_sum(double v, double* sh) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();                                   // sh may still be read from the sum before
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh[0];
    for (int w = 1; w < kWaves; ++w) s += sh[w];
    return s;
}

__device__ __forceinline__ void prox_load4(const float* src, size_t at, int cnt, bool vec, float* v) {
    if (vec && cnt == 4) {
        const float4 f = *reinterpret_cast<const float4*>(src + at);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
        for (int k = 0; k < 4; ++k) v[k] = k < cnt ? src[at + k] : 0.0f;
    }
}

__device__ __forceinline__ void prox_store4(float* dst, size_t at, int cnt, bool vec, const float* v) {
    if (vec && cnt == 4) {
        *reinterpret_cast<float4*>(dst + at) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int k = 0; k < cnt; ++k) dst[at + k] = v[k];
    }
}

// ---- rows ---------------------------------------------------------------------------------------------------------

struct ProxRowsArgs {
    const float* z;
    const float* h;
    const float* e;        // [nr] or NULL
    float* q;
    double* partials;      // [workgroups]
    size_t n;              // H W nr
    int nr;
    float gt, eps, sigma, one_plus_sigma;
};

template <int KIND>
__device__ __forceinline__ float prox_rows_element(const ProxRowsArgs& a, float z, float h, float q, float d, double& F) {
#pragma clang fp contract(off)
    const float u = fmaf(a.sigma, z, q);
    if (KIND == NLOSGR_LOSS_MSE) {
        const double r = (double)z - (double)h;
        F += 0.5 * r * r;
        return fmaf(-a.sigma, h, u) / a.one_plus_sigma;
    }
    const float yp = fmaxf(a.gt * h, 0.0f) + a.eps;
    {
        const double yd = fmax((double)a.gt * (double)h, 0.0) + (double)a.eps;
        const double rho = fmax((double)d * (double)z, 0.0) + (double)a.eps;
        const double t = (rho - yd) / yd;
        F += yd * (t - log1p(t));
    }
    const float d2 = d * d;
    if (!(d2 > 0.0f)) return 0.0f;                     // d = 0, and a d so small (below 2^-75) that d d is 0 in fp32
    const float sp = a.sigma / d2;
    const float s = fmaf(sp, a.eps, u / d);
    const float A = s - 1.0f;
    const float c = (4.0f * sp) * yp;
    const float D = sqrtf(fmaf(A, A, c));
    // 1 + s + D = 2 + A + D >= 2; for A <= 0 the sum A + D is a difference, written as c / (D - A) instead
    const float den = A > 0.0f ? (2.0f + A) + D : 2.0f + (D - A > 0.0f ? c / (D - A) : 0.0f);
    const float num = 2.0f * fmaf(-sp, yp, s);
    return d * (num / den);
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void prox_rows_kernel(ProxRowsArgs a, bool vec) {
    __shared__ double sh[kWaves];
    double F = 0.0;
    const size_t base = (size_t)blockIdx.x * kProxRowsChunk;
    for (int it = 0; it < kProxRowsChunk / kProxTile; ++it) {
        const size_t at = base + (size_t)it * kProxTile + (size_t)threadIdx.x * kProxPerLane;
        if (at >= a.n) break;
        const int cnt = (int)min((size_t)kProxPerLane, a.n - at);
        float z[4], h[4], q[4];
        prox_load4(a.z, at, cnt, vec, z);
        prox_load4(a.h, at, cnt, vec, h);
        prox_load4(a.q, at, cnt, vec, q);
        int j = (int)(at % (size_t)a.nr);
        for (int k = 0; k < cnt; ++k) {
            const float d = (KIND == NLOSGR_LOSS_POISSON && a.e) ? a.e[j] : 1.0f;
            q[k] = prox_rows_element<KIND>(a, z[k], h[k], q[k], d, F);
            if (++j == a.nr) j = 0;
        }
        prox_store4(a.q, at, cnt, vec, q);
    }
    const double s = prox_block_sum(F, sh);
    if (threadIdx.x == 0) a.partials[blockIdx.x] = s;
}

// ---- volume -------------------------------------------------------------------------------------------------------

struct TvArgs {
    const float* xbar_in;  // dual
    float* p;              // [3][W][nr][H]: dual writes, primal reads
    const float* g;        // primal
    float* x;              // primal
    float* xbar;           // primal
    double* partials;      // dual: [workgroups][2]
    int W, nr, H, P, tiles;
    float an, aj, am;
    float step;            // sigma (dual), tau (primal)
    float tv;              // dual
    float thr;             // primal: tau l1
    int nonneg;
};

// block n tiles + tile: plane elements [1024 tile, +1024) of wall column n
__global__ __launch_bounds__(kBlock) void tv_dual_kernel(TvArgs a, bool vec) {
#pragma clang fp contract(off)
    __shared__ __align__(16) float xs[kProxTile + kProxHalo];
    __shared__ double sh[kWaves];
    const int n = blockIdx.x / a.tiles, t0 = (blockIdx.x - n * a.tiles) * kProxTile;
    const size_t col = (size_t)n * a.P;
    const int staged = min(kProxTile + a.H, a.P - t0);       // the tile and its halo along j, inside the plane
    if (vec) {
        const float4* const src = reinterpret_cast<const float4*>(a.xbar_in + col + t0);
        for (int i = threadIdx.x; i < staged / 4; i += kBlock) reinterpret_cast<float4*>(xs)[i] = src[i];
        for (int i = (staged & ~3) + threadIdx.x; i < staged; i += kBlock) xs[i] = a.xbar_in[col + t0 + i];
    } else {
        for (int i = threadIdx.x; i < staged; i += kBlock) xs[i] = a.xbar_in[col + t0 + i];
    }
    __syncthreads();
    const int l0 = threadIdx.x * kProxPerLane, t = t0 + l0;
    double tvsum = 0.0, l1sum = 0.0;
    if (t < a.P) {
        const int cnt = min(kProxPerLane, a.P - t);
        const bool more_n = n < a.W - 1;
        const size_t plane = (size_t)a.W * a.P;
        float xn[4] = {0.f, 0.f, 0.f, 0.f}, pn[4], pj[4], pm[4];
        if (more_n) prox_load4(a.xbar_in, col + a.P + t, cnt, vec, xn);
        prox_load4(a.p, col + t, cnt, vec, pn);
        prox_load4(a.p, plane + col + t, cnt, vec, pj);
        prox_load4(a.p, 2 * plane + col + t, cnt, vec, pm);
        int j = t / a.H, m = t - j * a.H;
        for (int k = 0; k < cnt; ++k) {
            const int l = l0 + k;
            const float xc = xs[l];
            const float gn = more_n ? a.an * (xn[k] - xc) : 0.0f;
            const float gj = j < a.nr - 1 ? a.aj * (xs[l + a.H] - xc) : 0.0f;
            const float gm = m < a.H - 1 ? a.am * (xs[l + 1] - xc) : 0.0f;
            {
                const double dn = more_n ? (double)a.an * ((double)xn[k] - (double)xc) : 0.0;
                const double dj = j < a.nr - 1 ? (double)a.aj * ((double)xs[l + a.H] - (double)xc) : 0.0;
                const double dm = m < a.H - 1 ? (double)a.am * ((double)xs[l + 1] - (double)xc) : 0.0;
                tvsum += sqrt(fma(dm, dm, fma(dj, dj, dn * dn)));
                l1sum += fabs((double)xc);
            }
            const float u0 = fmaf(a.step, gn, pn[k]), u1 = fmaf(a.step, gj, pj[k]), u2 = fmaf(a.step, gm, pm[k]);
            const float nrm = sqrtf(fmaf(u2, u2, fmaf(u1, u1, u0 * u0)));
            if (a.tv == 0.0f) {
                pn[k] = 0.0f; pj[k] = 0.0f; pm[k] = 0.0f;
            } else if (nrm <= a.tv) {
                pn[k] = u0; pj[k] = u1; pm[k] = u2;
            } else {
                const float f = a.tv / nrm;
                pn[k] = u0 * f; pj[k] = u1 * f; pm[k] = u2 * f;
            }
            if (++m == a.H) { m = 0; ++j; }
        }
        prox_store4(a.p, col + t, cnt, vec, pn);
        prox_store4(a.p, plane + col + t, cnt, vec, pj);
        prox_store4(a.p, 2 * plane + col + t, cnt, vec, pm);
    }
    const double s_tv = prox_block_sum(tvsum, sh);
    const double s_l1 = prox_block_sum(l1sum, sh);
    if (threadIdx.x == 0) {
        a.partials[2 * (size_t)blockIdx.x] = s_tv;
        a.partials[2 * (size_t)blockIdx.x + 1] = s_l1;
    }
}

__global__ __launch_bounds__(kBlock) void tv_primal_kernel(TvArgs a, bool vec) {
#pragma clang fp contract(off)
    __shared__ __align__(16) float pjs[kProxHalo + kProxTile];            // p_j[t0 - H .. t0 + 1024): element l at [kProxHalo + l]
    __shared__ __align__(16) float pms[4 + kProxTile];                    // p_m[t0 - 1 .. t0 + 1024): element l at [4 + l]
    const int n = blockIdx.x / a.tiles, t0 = (blockIdx.x - n * a.tiles) * kProxTile;
    const size_t col = (size_t)n * a.P, plane = (size_t)a.W * a.P;
    const float* const pj = a.p + plane + col;
    const float* const pm = a.p + 2 * plane + col;
    const int own = min(kProxTile, a.P - t0), back = min(a.H, t0);
    if (vec) {
        const float4* const sj = reinterpret_cast<const float4*>(pj + t0);
        const float4* const sm = reinterpret_cast<const float4*>(pm + t0);
        for (int i = threadIdx.x; i < own / 4; i += kBlock) {   // (P and t0 are multiples of 4: so is own)
            reinterpret_cast<float4*>(pjs + kProxHalo)[i] = sj[i];
            reinterpret_cast<float4*>(pms + 4)[i] = sm[i];
        }
    } else {
        for (int i = threadIdx.x; i < own; i += kBlock) {
            pjs[kProxHalo + i] = pj[t0 + i];
            pms[4 + i] = pm[t0 + i];
        }
    }
    for (int i = threadIdx.x; i < back; i += kBlock) pjs[kProxHalo - back + i] = pj[t0 - back + i];
    if (threadIdx.x == 0 && t0 > 0) pms[3] = pm[t0 - 1];
    __syncthreads();
    const int l0 = threadIdx.x * kProxPerLane, t = t0 + l0;
    if (t >= a.P) return;
    const int cnt = min(kProxPerLane, a.P - t);
    float pn[4], pb[4] = {0.f, 0.f, 0.f, 0.f}, g[4], x[4], xb[4];
    prox_load4(a.p, col + t, cnt, vec, pn);
    if (n > 0) prox_load4(a.p, col - a.P + t, cnt, vec, pb);
    prox_load4(a.g, col + t, cnt, vec, g);
    prox_load4(a.x, col + t, cnt, vec, x);
    int j = t / a.H, m = t - j * a.H;
    for (int k = 0; k < cnt; ++k) {
        const int l = l0 + k;
        const float dn = a.an * ((n > 0 ? pb[k] : 0.0f) - (n < a.W - 1 ? pn[k] : 0.0f));
        const float dj = a.aj * ((j > 0 ? pjs[kProxHalo + l - a.H] : 0.0f) - (j < a.nr - 1 ? pjs[kProxHalo + l] : 0.0f));
        const float dm = a.am * ((m > 0 ? pms[3 + l] : 0.0f) - (m < a.H - 1 ? pms[4 + l] : 0.0f));
        const float w = g[k] + ((dn + dj) + dm);
        const float u = fmaf(-a.step, w, x[k]);
        const float xp = a.nonneg ? fmaxf(u - a.thr, 0.0f) : copysignf(fmaxf(fabsf(u) - a.thr, 0.0f), u);
        xb[k] = fmaf(2.0f, xp, -x[k]);
        x[k] = xp;
        if (++m == a.H) { m = 0; ++j; }
    }
    prox_store4(a.x, col + t, cnt, vec, x);
    prox_store4(a.xbar, col + t, cnt, vec, xb);
}

inline bool prox_finite_nonneg(float v) { return v >= 0.0f && v <= 3.0e38f; }

inline bool prox_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

inline bool prox_aligned(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if ((uintptr_t)p % 16) return false;
    return true;
}

int tv_check(int32_t W, int32_t nr, int32_t H, float an, float aj, float am, float step, const char* step_error) {
    if (lattice_check_extents("primal-dual extents H, W, nr", H, W, nr) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (!prox_finite_nonneg(an) || !prox_finite_nonneg(aj) || !prox_finite_nonneg(am))
        return set_err(NLOSGR_E_INVALID, "the axis weights must be finite and >= 0");
    if (!lattice_positive(step)) return set_err(NLOSGR_E_INVALID, step_error);
    return NLOSGR_OK;
}

inline unsigned tv_tiles(int32_t nr, int32_t H) { return ((unsigned)nr * (unsigned)H + kProxTile - 1) / kProxTile; }

}  // namespace

extern "C" {

size_t nlosgr_prox_rows_partials(int32_t H, int32_t W, int32_t nr) {
    if (lattice_check_extents("primal-dual extents H, W, nr", H, W, nr) != NLOSGR_OK) return 0;
    return ((size_t)H * W * nr + kProxRowsChunk - 1) / kProxRowsChunk;
}

int nlosgr_prox_rows(const float* z, const float* h, const float* exposure, int32_t H, int32_t W, int32_t nr,
                     int32_t kind, float gt_times, float rate_floor, float sigma, float* q, double* partials,
                     void* hip_stream) {
    if (lattice_check_extents("primal-dual extents H, W, nr", H, W, nr) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (kind != NLOSGR_LOSS_MSE && kind != NLOSGR_LOSS_POISSON)
        return set_err(NLOSGR_E_INVALID, "unknown data term kind (NLOSGR_LOSS_MSE or NLOSGR_LOSS_POISSON)");
    if (!lattice_positive(sigma)) return set_err(NLOSGR_E_INVALID, "sigma must be finite and > 0");
    if (kind == NLOSGR_LOSS_MSE && exposure)
        return set_err(NLOSGR_E_INVALID, "the MSE data term takes no exposure table (pass NULL)");
    if (kind == NLOSGR_LOSS_POISSON) {
        if (!lattice_positive(rate_floor)) return set_err(NLOSGR_E_INVALID, "rate_floor must be finite and > 0");
        if (!(gt_times >= -3.0e38f && gt_times <= 3.0e38f)) return set_err(NLOSGR_E_INVALID, "gt_times must be finite");
    }
    if (!z || !h || !q || !partials) return set_err(NLOSGR_E_INVALID, "null pointer (z, h, q or partials)");
    const size_t n = (size_t)H * W * nr, bytes = n * sizeof(float);
    if (prox_overlap(z, bytes, q, bytes) || prox_overlap(h, bytes, q, bytes))
        return set_err(NLOSGR_E_INVALID, "q is updated in place: it must not alias z or h");
    if (exposure && prox_overlap(exposure, (size_t)nr * sizeof(float), q, bytes))
        return set_err(NLOSGR_E_INVALID, "q is updated in place: it must not alias the exposure table");
    const size_t pbytes = ((n + kProxRowsChunk - 1) / kProxRowsChunk) * sizeof(double);
    if (prox_overlap(partials, pbytes, q, bytes) || prox_overlap(partials, pbytes, z, bytes) ||
        prox_overlap(partials, pbytes, h, bytes) ||
        (exposure && prox_overlap(partials, pbytes, exposure, (size_t)nr * sizeof(float))))
        return set_err(NLOSGR_E_INVALID, "the partials are written: they must not alias z, h, q or the exposure table");
    ProxRowsArgs a;
    a.z = z; a.h = h; a.e = exposure; a.q = q; a.partials = partials; a.n = n; a.nr = nr;
    a.gt = gt_times; a.eps = rate_floor; a.sigma = sigma; a.one_plus_sigma = 1.0f + sigma;
    const bool vec = prox_aligned({z, h, q});
    const dim3 grid((unsigned)((n + kProxRowsChunk - 1) / kProxRowsChunk));
    hipStream_t s = (hipStream_t)hip_stream;
    if (kind == NLOSGR_LOSS_MSE) hipLaunchKernelGGL(prox_rows_kernel<NLOSGR_LOSS_MSE>, grid, dim3(kBlock), 0, s, a, vec);
    else hipLaunchKernelGGL(prox_rows_kernel<NLOSGR_LOSS_POISSON>, grid, dim3(kBlock), 0, s, a, vec);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

size_t nlosgr_tv_dual_partials(int32_t W, int32_t nr, int32_t H) {
    if (lattice_check_extents("primal-dual extents H, W, nr", H, W, nr) != NLOSGR_OK) return 0;
    return 2 * (size_t)W * tv_tiles(nr, H);
}

int nlosgr_tv_dual(const float* xbar, int32_t W, int32_t nr, int32_t H, float a_n, float a_j, float a_m, float sigma,
                   float tv, float* p, double* partials, void* hip_stream) {
    if (tv_check(W, nr, H, a_n, a_j, a_m, sigma, "sigma must be finite and > 0") != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (!(tv >= 0.0f)) return set_err(NLOSGR_E_INVALID, "tv must be >= 0 (+inf: no projection)");
    if (!xbar || !p || !partials) return set_err(NLOSGR_E_INVALID, "null pointer (xbar, p or partials)");
    const size_t bytes = (size_t)W * nr * H * sizeof(float);
    if (prox_overlap(xbar, bytes, p, 3 * bytes))
        return set_err(NLOSGR_E_INVALID, "p is updated in place: it must not alias xbar");
    const size_t pbytes = 2 * (size_t)W * tv_tiles(nr, H) * sizeof(double);
    if (prox_overlap(partials, pbytes, xbar, bytes) || prox_overlap(partials, pbytes, p, 3 * bytes))
        return set_err(NLOSGR_E_INVALID, "the partials are written: they must not alias xbar or p");
    TvArgs a = {};
    a.xbar_in = xbar; a.p = p; a.partials = partials;
    a.W = W; a.nr = nr; a.H = H; a.P = nr * H; a.tiles = (int)tv_tiles(nr, H);
    a.an = a_n; a.aj = a_j; a.am = a_m; a.step = sigma; a.tv = tv;
    const bool vec = a.P % 4 == 0 && prox_aligned({xbar, p});
    hipLaunchKernelGGL(tv_dual_kernel, dim3((unsigned)W * (unsigned)a.tiles), dim3(kBlock), 0, (hipStream_t)hip_stream,
                       a, vec);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

int nlosgr_tv_primal(const float* g, const float* p, int32_t W, int32_t nr, int32_t H, float a_n, float a_j, float a_m,
                     float tau, float l1, int32_t nonneg, float* x, float* xbar, void* hip_stream) {
    if (tv_check(W, nr, H, a_n, a_j, a_m, tau, "tau must be finite and > 0") != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (!prox_finite_nonneg(l1)) return set_err(NLOSGR_E_INVALID, "l1 must be finite and >= 0");
    if (!g || !p || !x || !xbar) return set_err(NLOSGR_E_INVALID, "null pointer (g, p, x or xbar)");
    const size_t bytes = (size_t)W * nr * H * sizeof(float);
    if (prox_overlap(x, bytes, xbar, bytes)) return set_err(NLOSGR_E_INVALID, "x and xbar must not alias");
    if (prox_overlap(g, bytes, x, bytes) || prox_overlap(g, bytes, xbar, bytes))
        return set_err(NLOSGR_E_INVALID, "x and xbar are updated in place: they must not alias g");
    if (prox_overlap(p, 3 * bytes, x, bytes) || prox_overlap(p, 3 * bytes, xbar, bytes))
        return set_err(NLOSGR_E_INVALID, "x and xbar are updated in place: they must not alias p");
    TvArgs a = {};
    a.p = const_cast<float*>(p); a.g = g; a.x = x; a.xbar = xbar;
    a.W = W; a.nr = nr; a.H = H; a.P = nr * H; a.tiles = (int)tv_tiles(nr, H);
    a.an = a_n; a.aj = a_j; a.am = a_m; a.step = tau; a.nonneg = nonneg != 0;
    {
#pragma clang fp contract(off)
        a.thr = tau * l1;
    }
    const bool vec = a.P % 4 == 0 && prox_aligned({g, p, x, xbar});
    hipLaunchKernelGGL(tv_primal_kernel, dim3((unsigned)W * (unsigned)a.tiles), dim3(kBlock), 0, (hipStream_t)hip_stream,
                       a, vec);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

}  // extern "C"
