// Forward projection of a voxel grid to the transients a capture would hold (gfx950): the adjoint of the
// gather of nlosgr_backproject.hip.  One scatter kernel serves nlosgr_forward_project (confocal) and
// nlosgr_forward_project_nc (a laser spot per measurement, or one for the capture).  For voxel centre x (grid
// tables) and measurement i with sensed wall point s_i and laser spot l_i (include/nlosgr.h, ABI 13), all fp32
// with no contraction:
//
//                        confocal                          non-confocal
//     distances          d = |x - s_i|                     ds = |x - s_i|, dl = |x - l_i|
//     bin coordinate     g = d                             g = 0.5f * (dl + ds)
//     weight             d^power as d, d*d, (d*d)*d,       m^(power/2) of m = dl * ds:  1: sqrt(m);  2: m;
//                        (d*d)*(d*d); negative: 1 / that   3: m*sqrt(m);  4: m*m;  negative: 1 / that
//     negative powers    need r0 * inv_dr >= 2             pairs with min(dl, ds) < dmin are left out
//
//     each distance sqrt((dx*dx + dy*dy) + dz*dz), the hardware square root (as the gather forms it)
//     u = (g - r0) * inv_dr,  k = floor(u),  f = u - k
//     rows_i[j] = sum_x weight vol(x) ((1-f) [k == j] + f [k+1 == j]),   0 <= j < nr
//
// With lasers == sensors g is the confocal d exactly and m = d*d, so the even powers give the confocal numbers
// bit for bit; the odd powers differ by the rounding of sqrt(d*d) against d.
//
// A scatter: every voxel adds into two bins of every measurement's row.  No float atomics: each term is rounded
// once to a multiple of the call's quantum q (a power of two, fp_unit below) and added as a 64-bit integer, so
// the order of the additions cannot matter and the result is bitwise the same for every nsplit, launch shape
// and workgroup order.
//
// Shape: one 256-thread workgroup per (W measurements, voxel split) with W int64 LDS rows of nr bins; W = 4, 2 or
// 1 (fp_walls_per_group), so a voxel's value and coordinates are read once for W measurements: with W = 1 the walk
// over the volume was a third of the time.  A lane owns kFpRun voxels adjacent in z (flat index, z fastest), so a
// wave reads 1 KiB of vol contiguously; zero voxels are skipped.  Every remaining (voxel, measurement) pair
// converts its two terms and issues two no-return 64-bit LDS adds (the confocal mode one pair later: DEFER in the
// kernel).  With nsplit == 1 the workgroup scales
// its own rows and stores floats; otherwise the workgroups add their non-zero bins into the int64 [nmeas][nr]
// workspace with 64-bit integer atomics and fp_finish_kernel scales it.
//
// Addresses (contract 7): u is clamped into [-2, nr + 1] (a NaN u goes to -2), k = floor(u) lies in
// [-2, nr + 1], and an add into bin j = k or k + 1 is issued only under (unsigned)j < nr.  Voxel indices stay
// below the split's end <= nvox, and (ix, iy, iz) is the mixed-radix form of such an index, so every table read
// is inside its table.
#include "nlosgr_project.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

constexpr int kFpRun = 4;                 // voxels adjacent in z that one lane owns per step
constexpr int kFpStep = kFpRun * kBlock;   // voxels a workgroup covers per step
constexpr int kFpHeader = 256;             // workspace: [0] the bits of max|vol|; the int64 rows start here
constexpr unsigned kFpTargetGroups = 1024; // the library's nsplit fills 256 CUs four times over
constexpr size_t kFpRowBytes = 32768;      // LDS rows of a workgroup that serves more than one measurement
constexpr double kFpWeightMargin = 1.0 + 1.0 / 524288.0;   // 1 + 2^-19: fp32 error of the weight at the window's end

struct ScatterArgs {
    const float* vol;
    const float* sensors;          // (the confocal capture's wall points)
    const float* lasers;           // kPerMeas: [nmeas][3]; kOneLaser: [3]; kConfocal: unused
    int nmeas, nr;
    ProjGrid g;
    float r0, inv_dr, dmin;        // dmin: non-confocal negative powers
    int accumulate, nsplit;
    unsigned nvox, chunk;          // chunk: voxels per split, a multiple of kFpRun
    int sx, sy, sz;                // kFpStep = (sx * ny + sy) * nz + sz
    int ew, S;                     // wmax < 2^ew; every term is below 2^S quanta
    const unsigned* vmax;          // bits of max|vol| (any non-finite voxel: >= 0x7f800000)
    unsigned long long* acc;       // [nmeas][nr] (nsplit > 1)
    float* out;
};

// scale 2^(S - e) of a term to quanta and 2^(e - S) back, e = ev + ew with max|vol| = m 2^ev, m in [0.5, 1)
__device__ __forceinline__ void fp_unit(unsigned vbits, int ew, int S, double& to_q, double& from_q) {
    int ev;
    (void)frexp((double)__uint_as_float(vbits), &ev);
    to_q = ldexp(1.0, S - (ev + ew));
    from_q = ldexp(1.0, (ev + ew) - S);
}

__global__ __launch_bounds__(kBlock) void fp_vmax_kernel(const float* __restrict__ vol, unsigned n, unsigned* out) {
    unsigned m = 0u;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
        m = max(m, __float_as_uint(vol[i]) & 0x7fffffffu);      // |v| as bits: ordered as the values, NaN on top
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if (lane_id() == 0 && m) atomicMax(out, m);
}

// nsplit > 1: the int64 sums of every (measurement, bin) to floats
__global__ __launch_bounds__(kBlock) void fp_finish_kernel(const unsigned long long* __restrict__ acc, size_t n,
                                                           const unsigned* vmax, int ew, int S, int accumulate,
                                                           float* out) {
    const size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const unsigned vb = *vmax;
    float r;
    if (vb >= 0x7f800000u) {
        r = __uint_as_float(0x7fc00000u);
    } else {
        double to_q, from_q;
        fp_unit(vb, ew, S, to_q, from_q);
        r = (float)((double)(long long)acc[j] * from_q);
    }
    out[j] = accumulate && vb < 0x7f800000u ? out[j] + r : r;
}

// a term in quanta, rounded to nearest (there is no single fp32 -> int64 instruction: through double)
__device__ __forceinline__ long long fp_quanta(float term, double to_q) { return __double2ll_rn((double)term * to_q); }

// v quanta into bin j of an LDS row, if j is a bin of the row
__device__ __forceinline__ void fp_add(unsigned long long* row, int j, int nr, long long v) {
    if ((unsigned)j < (unsigned)nr && v != 0)
        __hip_atomic_fetch_add(row + j, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// a term rounded to the nearest quantum and added into bin j of an LDS row, if j is a bin of the row
__device__ __forceinline__ void fp_add_term(unsigned long long* row, int j, int nr, float term, double to_q) {
    if ((unsigned)j < (unsigned)nr) fp_add(row, j, nr, fp_quanta(term, to_q));
}

template <int POWER, int W, int MODE>
__global__ __launch_bounds__(kBlock) void scatter_kernel(ScatterArgs a) {
    extern __shared__ unsigned long long fp_row[];      // W rows of nr bins
    const int t = threadIdx.x;
    const int grp = blockIdx.x / a.nsplit, sp = blockIdx.x - grp * a.nsplit;
    const int i0 = grp * W, nw = min(W, a.nmeas - i0);   // this workgroup's measurements [i0, i0 + nw)
    const bool single = a.nsplit == 1;
    const int nr = a.nr;
    const int ny = a.g.ny, nz = a.g.nz;
    float* const orow = a.out + (size_t)i0 * nr;
    const unsigned vb = *a.vmax;
    if (vb >= 0x7f800000u || vb == 0u) {                 // a non-finite voxel: NaN rows; a zero volume: zero rows
        if (single && !(vb == 0u && a.accumulate)) {
            const float fill = vb ? __uint_as_float(0x7fc00000u) : 0.0f;
            for (int j = t; j < nw * nr; j += kBlock) orow[j] = fill;
        }
        return;
    }
    for (int j = t; j < W * nr; j += kBlock) fp_row[j] = 0ull;
    __syncthreads();
    double to_q, from_q;
    fp_unit(vb, a.ew, a.S, to_q, from_q);
    // when a pair's two adds are issued.  Confocal: after the next pair's terms are formed (the lane holds one
    // pair's quanta); non-confocal: at once.  The only step the modes do not share, and kept apart on the clock:
    // at once, the confocal power 0 is 1-3 % slower; held back a pair, the non-confocal calls are 2-15 % slower
    // ("Voxel projectors folded").  Integer adds: the form cannot change a bit
    constexpr bool DEFER = MODE == kConfocal;
    // a measurement past the end gets NaN sensor coordinates: its u is NaN, clamped to -2, and every add is masked
    float wx[W], wy[W], wz[W], lx[W], ly[W], lz[W];
    int kc[W];                      // DEFER: the k whose two terms s0, s1 the lane holds (-4: none; k is >= -2)
    long long s0[W], s1[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const bool in = w < nw;
        const size_t o = 3 * (size_t)(i0 + (in ? w : 0));
        const float nan = __uint_as_float(0x7fc00000u);
        wx[w] = in ? a.sensors[o] : nan; wy[w] = in ? a.sensors[o + 1] : nan; wz[w] = in ? a.sensors[o + 2] : nan;
        if (MODE != kConfocal) {
            const size_t ol = MODE == kOneLaser ? 0 : o;
            lx[w] = a.lasers[ol]; ly[w] = a.lasers[ol + 1]; lz[w] = a.lasers[ol + 2];
        }
        kc[w] = -4; s0[w] = 0; s1[w] = 0;
    }
    const float umax = (float)(nr + 1);
    const unsigned v0 = (unsigned)sp * a.chunk, v1 = min(v0 + a.chunk, a.nvox);   // < 2^31: no wrap
    unsigned base = v0 + (unsigned)(kFpRun * t);
    int iz = (int)(base % (unsigned)nz);
    unsigned rest = base / (unsigned)nz;
    int iy = (int)(rest % (unsigned)ny), ix = (int)(rest / (unsigned)ny);
    for (; base < v1; base += kFpStep) {
        float v[kFpRun];
#pragma unroll
        for (int r = 0; r < kFpRun; ++r) v[r] = base + r < v1 ? a.vol[base + r] : 0.0f;
        bool any = false;
#pragma unroll
        for (int r = 0; r < kFpRun; ++r) any |= v[r] != 0.0f;
        if (any) {
            int jx = ix, jy = iy, jz = iz;
#pragma unroll
            for (int r = 0; r < kFpRun; ++r) {
                if (v[r] != 0.0f) {                      // (a non-zero voxel is below v1, so jx < nx)
                    const float x = a.g.xs[jx], y = a.g.ys[jy], z = a.g.zs[jz];
                    float dl1 = 0.0f;
                    if (MODE == kOneLaser) dl1 = nc_dist(nc_ss(x, y, lx[0], ly[0]), z - lz[0]);
#pragma unroll
                    for (int w = 0; w < W; ++w) {
#pragma clang fp contract(off)
                        const float ds = nc_dist(nc_ss(x, y, wx[w], wy[w]), z - wz[w]);
                        float g = ds, wv = v[r], dl = ds;
                        if (MODE == kConfocal) {
                            if (POWER != 0) wv = conf_weight<POWER>(ds) * v[r];
                        } else {
                            dl = MODE == kOneLaser ? dl1 : nc_dist(nc_ss(x, y, lx[w], ly[w]), z - lz[w]);
                            g = 0.5f * (dl + ds);
                            if (POWER != 0) wv = nc_weight<POWER>(dl * ds) * v[r];
                            // a negative power has no bound on its weight next to the laser or the sensor: the
                            // pairs closer than dmin to either are left out (wmax is formed from dmin)
                            if (POWER < 0 && !(fminf(dl, ds) >= a.dmin)) wv = 0.0f;
                        }
                        // clamped to [-2, nr + 1]: both bins are outside the row at either end (NaN goes to -2)
                        const float u = fminf(fmaxf((g - a.r0) * a.inv_dr, -2.0f), umax);
                        const float kf = floorf(u);
                        const int k = (int)kf;
                        const float f = u - kf;
                        if (DEFER) {
                            const long long q0 = fp_quanta(wv * (1.0f - f), to_q);
                            const long long q1 = fp_quanta(wv * f, to_q);
                            fp_add(fp_row + w * nr, kc[w], nr, s0[w]);
                            fp_add(fp_row + w * nr, kc[w] + 1, nr, s1[w]);
                            kc[w] = k; s0[w] = q0; s1[w] = q1;
                        } else {
                            fp_add_term(fp_row + w * nr, k, nr, wv * (1.0f - f), to_q);
                            fp_add_term(fp_row + w * nr, k + 1, nr, wv * f, to_q);
                        }
                    }
                }
                if (++jz == nz) {
                    jz = 0;
                    if (++jy == ny) { jy = 0; ++jx; }
                }
            }
        }
        // the next step's first voxel: one carry per digit (sz < nz, sy < ny)
        iz += a.sz;
        if (iz >= nz) { iz -= nz; ++iy; }
        iy += a.sy;
        if (iy >= ny) { iy -= ny; ++ix; }
        ix += a.sx;
    }
    if (DEFER) {
#pragma unroll
        for (int w = 0; w < W; ++w) {
            fp_add(fp_row + w * nr, kc[w], nr, s0[w]);
            fp_add(fp_row + w * nr, kc[w] + 1, nr, s1[w]);
        }
    }
    __syncthreads();
    if (single) {
        for (int j = t; j < nw * nr; j += kBlock) {
            const float r = (float)((double)(long long)fp_row[j] * from_q);
            orow[j] = a.accumulate ? orow[j] + r : r;
        }
    } else {
        unsigned long long* const g = a.acc + (size_t)i0 * nr;
        for (int j = t; j < nw * nr; j += kBlock) {
            const unsigned long long s = fp_row[j];
            if (s) __hip_atomic_fetch_add(g + j, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

int fp_ceil_log2(unsigned long long v) {      // the least b with v <= 2^b
    int b = 0;
    while ((1ull << b) < v) ++b;
    return b;
}

// measurements per workgroup: the most of 4, 2, 1 that the capture has and whose rows fit kFpRowBytes of LDS
int fp_walls_per_group(int nmeas, int nr) {
    int w = 4;
    while (w > 1 && (w > nmeas || (size_t)w * nr * sizeof(unsigned long long) > kFpRowBytes)) w >>= 1;
    return w;
}

// host validation of every entry point (dmin: non-confocal only); on success the weight bound's exponent and
// the voxel splits per measurement (opt->nsplit: 0 = the library's choice, else forced)
int fp_plan(int mode, int32_t nlaser, int32_t nmeas, int32_t nr, const nlosgr_voxel_grid* grid,
            const nlosgr_forward_project_opts* opt, float dmin, int* ew, int* nsplit) {
    const bool conf = mode == kConfocal;
    if (!grid || !opt) return set_err(NLOSGR_E_INVALID, "null argument struct");
    if (check_grid(grid) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (nr < 1) return set_err(NLOSGR_E_INVALID, "nr must be >= 1");
    if (nr > NLOSGR_IRF_MAX_NR) return set_err(NLOSGR_E_UNSUPPORTED, "nr above NLOSGR_IRF_MAX_NR");
    if (nmeas < 0) return set_err(NLOSGR_E_INVALID, conf ? "nwall must be >= 0" : "nmeas must be >= 0");
    if (check_nlaser(mode, nlaser, nmeas) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (check_power(opt->power, -4) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (check_window(opt->r0, opt->inv_dr) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (opt->power < 0 && conf && !((double)opt->r0 * (double)opt->inv_dr >= 2.0))
        return set_err(NLOSGR_E_INVALID, "a negative power needs r0 * inv_dr >= 2");
    if (opt->power < 0 && !conf && !(dmin > 0.0f && dmin <= 3.0e38f))
        return set_err(NLOSGR_E_INVALID, "a negative power needs a finite dmin > 0");
    if (opt->nsplit < 0) return set_err(NLOSGR_E_INVALID, "nsplit must be >= 0");
    if (!grid->xs || !grid->ys || !grid->zs) return set_err(NLOSGR_E_INVALID, "null voxel grid table");
    // wmax: the largest weight of a contributing pair (u > -1 and u < nr), from the fp32 window in double.
    // power >= 0: a pair contributes only when u < nr, so g < r0 + nr dr up to the fp32 error of u (7 roundings
    // of g + |r0|, far below the one bin R = r0 + (nr + 1) dr leaves); non-confocal m = dl ds <= g^2 by AM-GM.
    // The fp32 m carries the 4 roundings of each distance and 1 of the product, 9 like the confocal d*d; sqrt(m)
    // 5.5, m*sqrt(m) 15.5 and m*m 19, the confocal d^4's count and the largest: (1 + 2^-24)^19 < 1 + 2^-19.
    // power < 0, confocal: u > -1 with r0 * inv_dr >= 2 gives d > R = r0 - 1.5 dr > 0.  Non-confocal: every
    // contributing pair has dl, ds >= dmin, so m >= dmin^2 up to the one rounding of the product and
    // 1 / m^(p/2) <= 1 / dmin^p up to at most 4 more roundings (sqrt, product, reciprocal).
    const double dr = 1.0 / (double)opt->inv_dr;
    const int p = opt->power < 0 ? -opt->power : opt->power;
    double R = opt->power >= 0 ? (double)opt->r0 + (double)(nr + 1) * dr
                               : (conf ? (double)opt->r0 - 1.5 * dr : (double)dmin);
    if (R < 0.0) R = 0.0;
    double w = 1.0;
    for (int q = 0; q < p; ++q) w *= R;
    if (opt->power < 0) w = 1.0 / w;
    w *= kFpWeightMargin;
    if (!(w <= 1.0e300))
        return set_err(NLOSGR_E_INVALID, conf ? "r0 and inv_dr give no finite bound on d^power"
                                              : "r0, inv_dr and dmin give no finite bound on the weight");
    (void)frexp(w, ew);
    const unsigned nvox = (unsigned)grid->nx * grid->ny * grid->nz;
    // the library's choice: no split below one step of a workgroup; a forced count: no split below one lane's run
    const unsigned most = opt->nsplit ? (nvox + kFpRun - 1) / kFpRun : (nvox + kFpStep - 1) / kFpStep;
    const int W = fp_walls_per_group(nmeas, nr);
    const unsigned groups = nmeas > 0 ? (unsigned)((nmeas + W - 1) / W) : 1u;
    unsigned ns = opt->nsplit ? (unsigned)opt->nsplit : (kFpTargetGroups + groups - 1) / groups;
    if (ns > most) ns = most;
    if (ns < 1) ns = 1;
    if ((unsigned long long)ns * groups > 0x7fffffffull)
        return set_err(NLOSGR_E_UNSUPPORTED, "workgroups * nsplit above 2^31 - 1");
    *nsplit = (int)ns;
    return NLOSGR_OK;
}

size_t scatter_workspace_bytes(int mode, int32_t nlaser, int32_t nmeas, int32_t nr, const nlosgr_voxel_grid* grid,
                               const nlosgr_forward_project_opts* opt, float dmin) {
    int ew, ns;
    if (fp_plan(mode, nlaser, nmeas, nr, grid, opt, dmin, &ew, &ns) != NLOSGR_OK) return 0;
    return kFpHeader + (ns > 1 ? align_up((size_t)nmeas * nr * sizeof(unsigned long long)) : 0);
}

// both projectors (confocal: lasers == NULL, the walls as the sensors)
int scatter(int mode, const float* vol, const float* sensors, const float* lasers, int32_t nlaser, int32_t nmeas,
            int32_t nr, const nlosgr_voxel_grid* grid, const nlosgr_forward_project_opts* opt, float dmin,
            void* workspace, float* rows_out, void* hip_stream) {
    int ew, ns;
    const int rc = fp_plan(mode, nlaser, nmeas, nr, grid, opt, dmin, &ew, &ns);
    if (rc != NLOSGR_OK) return rc;
    if (!vol) return set_err(NLOSGR_E_INVALID, "null vol pointer");
    if (!workspace) return set_err(NLOSGR_E_INVALID, "null forward-projection workspace");
    if (nmeas == 0) return NLOSGR_OK;
    if (!sensors) return set_err(NLOSGR_E_INVALID, mode == kConfocal ? "null walls pointer" : "null sensors pointer");
    if (mode != kConfocal && !lasers) return set_err(NLOSGR_E_INVALID, "null lasers pointer");
    if (!rows_out) return set_err(NLOSGR_E_INVALID, "null forward-projection output");
    hipStream_t s = (hipStream_t)hip_stream;
    ScatterArgs a;
    a.vol = vol; a.sensors = sensors; a.lasers = lasers; a.nmeas = nmeas; a.nr = nr;
    a.g = proj_grid(grid);
    a.r0 = opt->r0; a.inv_dr = opt->inv_dr; a.dmin = dmin; a.accumulate = opt->accumulate != 0; a.nsplit = ns;
    a.nvox = (unsigned)grid->nx * grid->ny * grid->nz;
    a.chunk = ((a.nvox + ns - 1) / ns + kFpRun - 1) / kFpRun * kFpRun;
    a.sz = kFpStep % grid->nz; a.sy = (kFpStep / grid->nz) % grid->ny; a.sx = (kFpStep / grid->nz) / grid->ny;
    a.ew = ew; a.S = 62 - fp_ceil_log2(2ull * a.nvox);
    a.vmax = (const unsigned*)workspace;
    a.acc = (unsigned long long*)((char*)workspace + kFpHeader);
    a.out = rows_out;
    const size_t nrow = (size_t)nmeas * nr;
    HIPCHK(hipMemsetAsync(workspace, 0, kFpHeader + (ns > 1 ? nrow * sizeof(unsigned long long) : 0), s));
    const unsigned nb = (a.nvox + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(fp_vmax_kernel, dim3(nb < 1024u ? nb : 1024u), dim3(kBlock), 0, s, vol, a.nvox,
                       (unsigned*)workspace);
    const int W = fp_walls_per_group(nmeas, nr);
    const dim3 g((unsigned)((nmeas + W - 1) / W) * (unsigned)ns);
    const size_t lds = (size_t)W * nr * sizeof(unsigned long long);
    dispatch_int<-4, 4>(opt->power, [&](auto P) {
        dispatch_int<0, 2>(W == 4 ? 2 : W == 2 ? 1 : 0, [&](auto LOG2W) {
            dispatch_int<kConfocal, kOneLaser>(mode, [&](auto MODE) {
                hipLaunchKernelGGL((scatter_kernel<decltype(P)::value, 1 << decltype(LOG2W)::value, decltype(MODE)::value>),
                                   g, dim3(kBlock), lds, s, a);
            });
        });
    });
    HIPCHK(hipGetLastError());
    if (ns > 1) {
        hipLaunchKernelGGL(fp_finish_kernel, dim3((unsigned)((nrow + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a.acc,
                           nrow, a.vmax, ew, a.S, a.accumulate, rows_out);
        HIPCHK(hipGetLastError());
    }
    return NLOSGR_OK;
}

}  // namespace

extern "C" {

size_t nlosgr_forward_project_workspace_bytes(int32_t nwall, int32_t nr, const nlosgr_voxel_grid* grid,
                                              const nlosgr_forward_project_opts* opt) {
    return scatter_workspace_bytes(kConfocal, 0, nwall, nr, grid, opt, 0.0f);
}

int nlosgr_forward_project(const float* vol, const float* walls, int32_t nwall, int32_t nr,
                           const nlosgr_voxel_grid* grid, const nlosgr_forward_project_opts* opt, void* workspace,
                           float* rows_out, void* hip_stream) {
    return scatter(kConfocal, vol, walls, nullptr, 0, nwall, nr, grid, opt, 0.0f, workspace, rows_out, hip_stream);
}

size_t nlosgr_forward_project_nc_workspace_bytes(int32_t nlaser, int32_t nmeas, int32_t nr, const nlosgr_voxel_grid* grid,
                                                 const nlosgr_forward_project_opts* opt, float dmin) {
    return scatter_workspace_bytes(laser_mode(nlaser, nmeas), nlaser, nmeas, nr, grid, opt, dmin);
}

int nlosgr_forward_project_nc(const float* vol, const float* sensors, const float* lasers, int32_t nlaser, int32_t nmeas,
                              int32_t nr, const nlosgr_voxel_grid* grid, const nlosgr_forward_project_opts* opt,
                              float dmin, void* workspace, float* rows_out, void* hip_stream) {
    return scatter(laser_mode(nlaser, nmeas), vol, sensors, lasers, nlaser, nmeas, nr, grid, opt, dmin, workspace, rows_out,
                   hip_stream);
}

}  // extern "C"
