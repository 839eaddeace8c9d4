// Back-projection and forward projection of a NON-confocal capture (gfx950): measurement i has a sensed wall
// point s_i and a laser spot l_i, and the light of voxel x arrives after the path |x - l_i| + |x - s_i|.  Only the
// distance changes against nlosgr_backproject.hip / nlosgr_forward_project.hip; the bin coordinate, the
// two-bin read or splat, the summation contracts and the workspace are theirs (nlosgr_project.hpp).  For voxel
// centre x (grid tables) and measurement i (include/nlosgr.h, ABI 13), all fp32 with no contraction:
//
//     ds = |x - s_i|, dl = |x - l_i|             each sqrt((dx*dx + dy*dy) + dz*dz), the hardware square root
//     g  = 0.5f * (dl + ds)                      half the path: the confocal d, exactly, when l_i == s_i
//     m  = dl * ds                               the confocal d*d when l_i == s_i
//     u  = (g - r0) * inv_dr,  k = floor(u),  f = u - k
//     weight = m^(power/2):  0: 1;  1: sqrt(m);  2: m;  3: m*sqrt(m);  4: m*m;  negative: 1 / that
//
// So with lasers == sensors the even powers give the confocal kernels' numbers bit for bit (0.5f * (d + d) and
// d * d are what bp_tap forms); the odd powers differ by the rounding of sqrt(d*d) against d.
//
// ONE_LASER (one laser spot for the whole capture): dl depends on the voxel alone, so the back-projection forms
// the lane's two dl before its loop over the measurements and stages no laser tile, and the forward projector
// forms dl once per voxel outside its loop over the W measurements.  The arithmetic per pair is the same values
// in the same order as with the laser repeated nmeas times, so both give the same bits.
//
// Addresses: as the confocal kernels.  u is clamped into [-2, nr + 1] (NaN to -2); the back-projection reads
// one 8-byte pair clamped into the row and selects, the forward projector adds only under (unsigned)j < nr.
#include "nlosgr_project.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

// ------------------------------------------------------------------------------------------
// back-projection (nc_weight, nc_ss, nc_dist, nc_tap, nc_point: nlosgr_project.hpp)
// ------------------------------------------------------------------------------------------
struct NcBpArgs {
    const float* rows;
    const float* sensors;
    const float* lasers;
    int nmeas, nr;
    int nx, ny, nz;
    const float *xs, *ys, *zs;
    int nby, nbz;
    float r0, inv_dr;
    int accumulate;
    float* out;
};

// measurements [j, j + N) of the staged tile: every bin offset first, then all 2 N reads, then the sums in
// measurement order.  dl0, dl1: the lane's two laser distances (ONE_LASER)
template <int POWER, bool PAIR, bool ONE_LASER, int N>
__device__ __forceinline__ void nc_bp_step(const float4* stile, const float4* ltile, int j, const float* __restrict__ row,
                                           const NcBpArgs& a, float x, float y, float z0, float z1, float dl0, float dl1,
                                           int kmax, float umax, float& s0, float& s1) {
    BpTap ta[N], tb[N];
    BpBins va[N], vb[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const float4 w = stile[j + q];
        const float ss = nc_ss(x, y, w.x, w.y);
        float la = dl0, lb = dl1;
        if (!ONE_LASER) {
            const float4 l = ltile[j + q];
            const float sl = nc_ss(x, y, l.x, l.y);
            la = nc_dist(sl, z0 - l.z);
            lb = nc_dist(sl, z1 - l.z);
        }
        ta[q] = nc_tap<POWER>(la, nc_dist(ss, z0 - w.z), a.r0, a.inv_dr, kmax, umax);
        tb[q] = nc_tap<POWER>(lb, nc_dist(ss, z1 - w.z), a.r0, a.inv_dr, kmax, umax);
    }
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const char* r = (const char*)(row + (size_t)q * a.nr);
        va[q] = bp_read<PAIR>(r, ta[q].ib);
        vb[q] = bp_read<PAIR>(r, tb[q].ib);
    }
#pragma unroll
    for (int q = 0; q < N; ++q) {
        s0 += bp_eval<POWER>(ta[q], va[q]);
        s1 += bp_eval<POWER>(tb[q], vb[q]);
    }
}

template <int POWER, bool PAIR, bool ONE_LASER>
__global__ __launch_bounds__(kBlock) void nc_backproject_kernel(NcBpArgs a) {
    __shared__ float4 stile[kBpTile];
    __shared__ float4 ltile[ONE_LASER ? 1 : kBpTile];
    const int t = threadIdx.x;
    const int bz = blockIdx.x % a.nbz, by = (blockIdx.x / a.nbz) % a.nby, bx = blockIdx.x / (a.nbz * a.nby);
    // lane -> (x, y, z pair) of the brick, z fastest: a wave covers 2 x 8 x 8 voxels
    const int ix = bx * kBpBrick + (t >> 5), iy = by * kBpBrick + ((t >> 2) & 7), iz = bz * kBpBrick + 2 * (t & 3);
    const float x = a.xs[min(ix, a.nx - 1)], y = a.ys[min(iy, a.ny - 1)];
    const float z0 = a.zs[min(iz, a.nz - 1)], z1 = a.zs[min(iz + 1, a.nz - 1)];
    const float umax = (float)(a.nr + 1);
    const int kmax = max(a.nr - 2, 0);
    float dl0 = 0.0f, dl1 = 0.0f;
    if (ONE_LASER) {
        const float lx = a.lasers[0], ly = a.lasers[1], lz = a.lasers[2];
        const float sl = nc_ss(x, y, lx, ly);
        dl0 = nc_dist(sl, z0 - lz);
        dl1 = nc_dist(sl, z1 - lz);
    }
    double acc0 = 0.0, acc1 = 0.0;
    for (int base = 0; base < a.nmeas; base += kBpTile) {
        __syncthreads();
        stile[t] = nc_point(a.sensors, base + t, a.nmeas);
        if (!ONE_LASER) ltile[t] = nc_point(a.lasers, base + t, a.nmeas);
        __syncthreads();
        const int n = min(kBpTile, a.nmeas - base);
        const float* row = a.rows + (size_t)base * a.nr;
        float s0 = 0.0f, s1 = 0.0f;
        int j = 0;
        for (; j + kBpGroup <= n; j += kBpGroup, row += (size_t)kBpGroup * a.nr)
            nc_bp_step<POWER, PAIR, ONE_LASER, kBpGroup>(stile, ltile, j, row, a, x, y, z0, z1, dl0, dl1, kmax, umax, s0,
                                                         s1);
        for (; j < n; ++j, row += a.nr)
            nc_bp_step<POWER, PAIR, ONE_LASER, 1>(stile, ltile, j, row, a, x, y, z0, z1, dl0, dl1, kmax, umax, s0, s1);
        acc0 += (double)s0;
        acc1 += (double)s1;
    }
    if (ix < a.nx && iy < a.ny && iz < a.nz) {
        const size_t o = ((size_t)ix * a.ny + iy) * a.nz + iz;
        const float r0v = (float)acc0, r1v = (float)acc1;
        a.out[o] = a.accumulate ? a.out[o] + r0v : r0v;
        if (iz + 1 < a.nz) a.out[o + 1] = a.accumulate ? a.out[o + 1] + r1v : r1v;
    }
}

// ------------------------------------------------------------------------------------------
// forward projection
// ------------------------------------------------------------------------------------------
struct NcFpArgs {
    const float* vol;
    const float* sensors;
    const float* lasers;
    int nmeas, nr;
    int nx, ny, nz;
    const float *xs, *ys, *zs;
    float r0, inv_dr, dmin;
    int accumulate, nsplit;
    unsigned nvox, chunk;          // chunk: voxels per split, a multiple of kFpRun
    int sx, sy, sz;                // kFpStep = (sx * ny + sy) * nz + sz
    int ew, S;                     // wmax < 2^ew; every term is below 2^S quanta
    const unsigned* vmax;          // bits of max|vol| (any non-finite voxel: >= 0x7f800000)
    unsigned long long* acc;       // [nmeas][nr] (nsplit > 1)
    float* out;
};

// a term rounded to the nearest quantum and added into bin j of an LDS row, if j is a bin of the row
__device__ __forceinline__ void nc_fp_add(unsigned long long* row, int j, int nr, float term, double to_q) {
    if ((unsigned)j < (unsigned)nr) {
        const long long v = __double2ll_rn((double)term * to_q);
        if (v != 0)
            __hip_atomic_fetch_add(row + j, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

template <int POWER, int W, bool ONE_LASER>
__global__ __launch_bounds__(kBlock) void nc_forward_project_kernel(NcFpArgs a) {
    extern __shared__ unsigned long long nc_row[];      // W rows of nr bins
    const int t = threadIdx.x;
    const int grp = blockIdx.x / a.nsplit, sp = blockIdx.x - grp * a.nsplit;
    const int i0 = grp * W, nw = min(W, a.nmeas - i0);   // this workgroup's measurements [i0, i0 + nw)
    const bool single = a.nsplit == 1;
    const int nr = a.nr;
    float* const orow = a.out + (size_t)i0 * nr;
    const unsigned vb = *a.vmax;
    if (vb >= 0x7f800000u || vb == 0u) {                 // a non-finite voxel: NaN rows; a zero volume: zero rows
        if (single && !(vb == 0u && a.accumulate)) {
            const float fill = vb ? __uint_as_float(0x7fc00000u) : 0.0f;
            for (int j = t; j < nw * nr; j += kBlock) orow[j] = fill;
        }
        return;
    }
    for (int j = t; j < W * nr; j += kBlock) nc_row[j] = 0ull;
    __syncthreads();
    double to_q, from_q;
    fp_unit(vb, a.ew, a.S, to_q, from_q);
    // a measurement past the end gets NaN sensor coordinates: its u is NaN, clamped to -2, and every add is masked
    float wx[W], wy[W], wz[W], lx[W], ly[W], lz[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const bool in = w < nw;
        const size_t o = 3 * (size_t)(i0 + (in ? w : 0));
        const size_t ol = ONE_LASER ? 0 : o;
        const float nan = __uint_as_float(0x7fc00000u);
        wx[w] = in ? a.sensors[o] : nan; wy[w] = in ? a.sensors[o + 1] : nan; wz[w] = in ? a.sensors[o + 2] : nan;
        lx[w] = a.lasers[ol]; ly[w] = a.lasers[ol + 1]; lz[w] = a.lasers[ol + 2];
    }
    const float umax = (float)(nr + 1);
    const unsigned v0 = (unsigned)sp * a.chunk, v1 = min(v0 + a.chunk, a.nvox);   // < 2^31: no wrap
    unsigned base = v0 + (unsigned)(kFpRun * t);
    int iz = (int)(base % (unsigned)a.nz);
    unsigned rest = base / (unsigned)a.nz;
    int iy = (int)(rest % (unsigned)a.ny), ix = (int)(rest / (unsigned)a.ny);
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
                    const float x = a.xs[jx], y = a.ys[jy], z = a.zs[jz];
                    float dl1 = 0.0f;
                    if (ONE_LASER) dl1 = nc_dist(nc_ss(x, y, lx[0], ly[0]), z - lz[0]);
#pragma unroll
                    for (int w = 0; w < W; ++w) {
#pragma clang fp contract(off)
                        const float ds = nc_dist(nc_ss(x, y, wx[w], wy[w]), z - wz[w]);
                        const float dl = ONE_LASER ? dl1 : nc_dist(nc_ss(x, y, lx[w], ly[w]), z - lz[w]);
                        const float g = 0.5f * (dl + ds);
                        // clamped to [-2, nr + 1]: both bins are outside the row at either end (NaN goes to -2)
                        const float u = fminf(fmaxf((g - a.r0) * a.inv_dr, -2.0f), umax);
                        const float kf = floorf(u);
                        const int k = (int)kf;
                        const float f = u - kf;
                        float wv = POWER == 0 ? v[r] : nc_weight<POWER>(dl * ds) * v[r];
                        // a negative power has no bound on its weight next to the laser or the sensor: the pairs
                        // closer than dmin to either are left out (wmax is formed from dmin)
                        if (POWER < 0 && !(fminf(dl, ds) >= a.dmin)) wv = 0.0f;
                        nc_fp_add(nc_row + w * nr, k, nr, wv * (1.0f - f), to_q);
                        nc_fp_add(nc_row + w * nr, k + 1, nr, wv * f, to_q);
                    }
                }
                if (++jz == a.nz) {
                    jz = 0;
                    if (++jy == a.ny) { jy = 0; ++jx; }
                }
            }
        }
        // the next step's first voxel: one carry per digit (sz < nz, sy < ny)
        iz += a.sz;
        if (iz >= a.nz) { iz -= a.nz; ++iy; }
        iy += a.sy;
        if (iy >= a.ny) { iy -= a.ny; ++ix; }
        ix += a.sx;
    }
    __syncthreads();
    if (single) {
        for (int j = t; j < nw * nr; j += kBlock) {
            const float r = (float)((double)(long long)nc_row[j] * from_q);
            orow[j] = a.accumulate ? orow[j] + r : r;
        }
    } else {
        unsigned long long* const g = a.acc + (size_t)i0 * nr;
        for (int j = t; j < nw * nr; j += kBlock) {
            const unsigned long long s = nc_row[j];
            if (s) __hip_atomic_fetch_add(g + j, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

int nc_check_grid(const nlosgr_voxel_grid* grid) {
    if (grid->nx < 1 || grid->ny < 1 || grid->nz < 1 || grid->nx > kBpMaxExtent || grid->ny > kBpMaxExtent ||
        grid->nz > kBpMaxExtent)
        return set_err(NLOSGR_E_INVALID, "voxel grid extents must be in 1..1024");
    return NLOSGR_OK;
}

int nc_check_window(float r0, float inv_dr) {
    if (!(inv_dr > 0.0f) || !(inv_dr <= 3.0e38f)) return set_err(NLOSGR_E_INVALID, "inv_dr must be finite and > 0");
    if (!(fabsf(r0) <= 3.0e38f)) return set_err(NLOSGR_E_INVALID, "r0 must be finite");
    return NLOSGR_OK;
}

// host validation shared by both forward entry points; on success the weight bound's exponent and the split count
int nc_fp_plan(int32_t nlaser, int32_t nmeas, int32_t nr, const nlosgr_voxel_grid* grid,
               const nlosgr_forward_project_opts* opt, float dmin, int* ew, int* nsplit) {
    if (!grid || !opt) return set_err(NLOSGR_E_INVALID, "null argument struct");
    if (nc_check_grid(grid) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (nr < 1) return set_err(NLOSGR_E_INVALID, "nr must be >= 1");
    if (nr > NLOSGR_IRF_MAX_NR) return set_err(NLOSGR_E_UNSUPPORTED, "nr above NLOSGR_IRF_MAX_NR");
    if (nmeas < 0) return set_err(NLOSGR_E_INVALID, "nmeas must be >= 0");
    if (nlaser != 1 && nlaser != nmeas) return set_err(NLOSGR_E_INVALID, "nlaser must be 1 or nmeas");
    if (opt->power < -4 || opt->power > 4)
        return set_err(NLOSGR_E_INVALID, "forward-projection power must be in -4..4");
    if (nc_check_window(opt->r0, opt->inv_dr) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (opt->power < 0 && !(dmin > 0.0f && dmin <= 3.0e38f))
        return set_err(NLOSGR_E_INVALID, "a negative power needs a finite dmin > 0");
    if (opt->nsplit < 0) return set_err(NLOSGR_E_INVALID, "nsplit must be >= 0");
    if (!grid->xs || !grid->ys || !grid->zs) return set_err(NLOSGR_E_INVALID, "null voxel grid table");
    // wmax, the largest weight of a contributing pair, formed as the confocal one.
    // power >= 0: a pair contributes only when u < nr, so g < r0 + nr dr up to the fp32 error of u (7 roundings
    // of g + |r0|, far below the one bin R = r0 + (nr + 1) dr leaves), and m = dl ds <= g^2 by AM-GM.  The fp32
    // m carries the 4 roundings of each distance and 1 of the product, 9 like the confocal d*d; sqrt(m) 5.5,
    // m*sqrt(m) 15.5 and m*m 19, the confocal d^4's count and the largest: (1 + 2^-24)^19 < 1 + 2^-19.
    // power < 0: every contributing pair has dl, ds >= dmin, so m >= dmin^2 up to the one rounding of the
    // product and 1 / m^(p/2) <= 1 / dmin^p up to at most 4 more roundings (sqrt, product, reciprocal).
    const double dr = 1.0 / (double)opt->inv_dr;
    const int p = opt->power < 0 ? -opt->power : opt->power;
    double R = opt->power < 0 ? (double)dmin : (double)opt->r0 + (double)(nr + 1) * dr;
    if (R < 0.0) R = 0.0;
    double w = 1.0;
    for (int q = 0; q < p; ++q) w *= R;
    if (opt->power < 0) w = 1.0 / w;
    w *= kFpWeightMargin;
    if (!(w <= 1.0e300)) return set_err(NLOSGR_E_INVALID, "r0, inv_dr and dmin give no finite bound on the weight");
    (void)frexp(w, ew);
    return fp_split_count(nmeas, nr, grid, opt->nsplit, nsplit);
}

}  // namespace

extern "C" {

int nlosgr_backproject_nc(const float* rows, const float* sensors, const float* lasers, int32_t nlaser, int32_t nmeas,
                          int32_t nr, const nlosgr_voxel_grid* grid, const nlosgr_backproject_opts* opt, float* out,
                          void* hip_stream) {
    if (!grid || !opt) return set_err(NLOSGR_E_INVALID, "null argument struct");
    if (nc_check_grid(grid) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (nr < 1) return set_err(NLOSGR_E_INVALID, "nr must be >= 1");
    if (nmeas < 0) return set_err(NLOSGR_E_INVALID, "nmeas must be >= 0");
    if (nlaser != 1 && nlaser != nmeas) return set_err(NLOSGR_E_INVALID, "nlaser must be 1 or nmeas");
    if (opt->power < 0 || opt->power > 4) return set_err(NLOSGR_E_INVALID, "back-projection power must be in 0..4");
    if (nc_check_window(opt->r0, opt->inv_dr) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (!grid->xs || !grid->ys || !grid->zs) return set_err(NLOSGR_E_INVALID, "null voxel grid table");
    if (!out) return set_err(NLOSGR_E_INVALID, "null back-projection output");
    if (nmeas > 0 && (!rows || !sensors)) return set_err(NLOSGR_E_INVALID, "null rows or sensors pointer");
    if (nmeas > 0 && !lasers) return set_err(NLOSGR_E_INVALID, "null lasers pointer");
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t nvox = (size_t)grid->nx * grid->ny * grid->nz;
    if (nmeas == 0) {
        if (!opt->accumulate) HIPCHK(hipMemsetAsync(out, 0, nvox * sizeof(float), s));
        return NLOSGR_OK;
    }
    NcBpArgs a;
    a.rows = rows; a.sensors = sensors; a.lasers = lasers; a.nmeas = nmeas; a.nr = nr;
    a.nx = grid->nx; a.ny = grid->ny; a.nz = grid->nz;
    a.xs = grid->xs; a.ys = grid->ys; a.zs = grid->zs;
    a.nby = (grid->ny + kBpBrick - 1) / kBpBrick; a.nbz = (grid->nz + kBpBrick - 1) / kBpBrick;
    a.r0 = opt->r0; a.inv_dr = opt->inv_dr; a.accumulate = opt->accumulate != 0;
    a.out = out;
    const unsigned nbricks = (unsigned)((grid->nx + kBpBrick - 1) / kBpBrick) * a.nby * a.nbz;   // <= 128^3
    const bool pair = nr >= 2;
    // (a capture of one measurement is launched as the general case: the same bits, and no third kernel family)
    const bool one = nlaser == 1 && nmeas > 1;
#define NLOSGR_NC_BP_LAUNCH2(P, PAIR)                                                                          \
    if (one) hipLaunchKernelGGL((nc_backproject_kernel<P, PAIR, true>), dim3(nbricks), dim3(kBlock), 0, s, a); \
    else hipLaunchKernelGGL((nc_backproject_kernel<P, PAIR, false>), dim3(nbricks), dim3(kBlock), 0, s, a)
#define NLOSGR_NC_BP_LAUNCH(P)                   \
    if (pair) { NLOSGR_NC_BP_LAUNCH2(P, true); } \
    else { NLOSGR_NC_BP_LAUNCH2(P, false); }     \
    break
    switch (opt->power) {
        case 0: NLOSGR_NC_BP_LAUNCH(0);
        case 1: NLOSGR_NC_BP_LAUNCH(1);
        case 2: NLOSGR_NC_BP_LAUNCH(2);
        case 3: NLOSGR_NC_BP_LAUNCH(3);
        default: NLOSGR_NC_BP_LAUNCH(4);
    }
#undef NLOSGR_NC_BP_LAUNCH
#undef NLOSGR_NC_BP_LAUNCH2
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

size_t nlosgr_forward_project_nc_workspace_bytes(int32_t nlaser, int32_t nmeas, int32_t nr, const nlosgr_voxel_grid* grid,
                                                 const nlosgr_forward_project_opts* opt, float dmin) {
    int ew, ns;
    if (nc_fp_plan(nlaser, nmeas, nr, grid, opt, dmin, &ew, &ns) != NLOSGR_OK) return 0;
    return kFpHeader + (ns > 1 ? align_up((size_t)nmeas * nr * sizeof(unsigned long long)) : 0);
}

int nlosgr_forward_project_nc(const float* vol, const float* sensors, const float* lasers, int32_t nlaser, int32_t nmeas,
                              int32_t nr, const nlosgr_voxel_grid* grid, const nlosgr_forward_project_opts* opt,
                              float dmin, void* workspace, float* rows_out, void* hip_stream) {
    int ew, ns;
    const int rc = nc_fp_plan(nlaser, nmeas, nr, grid, opt, dmin, &ew, &ns);
    if (rc != NLOSGR_OK) return rc;
    if (!vol) return set_err(NLOSGR_E_INVALID, "null vol pointer");
    if (!workspace) return set_err(NLOSGR_E_INVALID, "null forward-projection workspace");
    if (nmeas == 0) return NLOSGR_OK;
    if (!sensors) return set_err(NLOSGR_E_INVALID, "null sensors pointer");
    if (!lasers) return set_err(NLOSGR_E_INVALID, "null lasers pointer");
    if (!rows_out) return set_err(NLOSGR_E_INVALID, "null forward-projection output");
    hipStream_t s = (hipStream_t)hip_stream;
    NcFpArgs a;
    a.vol = vol; a.sensors = sensors; a.lasers = lasers; a.nmeas = nmeas; a.nr = nr;
    a.nx = grid->nx; a.ny = grid->ny; a.nz = grid->nz;
    a.xs = grid->xs; a.ys = grid->ys; a.zs = grid->zs;
    a.r0 = opt->r0; a.inv_dr = opt->inv_dr; a.dmin = dmin; a.accumulate = opt->accumulate != 0; a.nsplit = ns;
    a.nvox = (unsigned)grid->nx * grid->ny * grid->nz;
    a.chunk = ((a.nvox + ns - 1) / ns + kFpRun - 1) / kFpRun * kFpRun;
    a.sz = kFpStep % a.nz; a.sy = (kFpStep / a.nz) % a.ny; a.sx = (kFpStep / a.nz) / a.ny;
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
    const bool one = nlaser == 1 && nmeas > 1;
#define NLOSGR_NC_FP_LAUNCH2(P, W_)                                                                       \
    if (one) hipLaunchKernelGGL((nc_forward_project_kernel<P, W_, true>), g, dim3(kBlock), lds, s, a);   \
    else hipLaunchKernelGGL((nc_forward_project_kernel<P, W_, false>), g, dim3(kBlock), lds, s, a)
#define NLOSGR_NC_FP_LAUNCH(P)                         \
    if (W == 4) { NLOSGR_NC_FP_LAUNCH2(P, 4); }        \
    else if (W == 2) { NLOSGR_NC_FP_LAUNCH2(P, 2); }   \
    else { NLOSGR_NC_FP_LAUNCH2(P, 1); }               \
    break
    switch (opt->power) {
        case -4: NLOSGR_NC_FP_LAUNCH(-4);
        case -3: NLOSGR_NC_FP_LAUNCH(-3);
        case -2: NLOSGR_NC_FP_LAUNCH(-2);
        case -1: NLOSGR_NC_FP_LAUNCH(-1);
        case 0: NLOSGR_NC_FP_LAUNCH(0);
        case 1: NLOSGR_NC_FP_LAUNCH(1);
        case 2: NLOSGR_NC_FP_LAUNCH(2);
        case 3: NLOSGR_NC_FP_LAUNCH(3);
        default: NLOSGR_NC_FP_LAUNCH(4);
    }
#undef NLOSGR_NC_FP_LAUNCH
#undef NLOSGR_NC_FP_LAUNCH2
    HIPCHK(hipGetLastError());
    if (ns > 1) {
        hipLaunchKernelGGL(fp_finish_kernel, dim3((unsigned)((nrow + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a.acc,
                           nrow, a.vmax, ew, a.S, a.accumulate, rows_out);
        HIPCHK(hipGetLastError());
    }
    return NLOSGR_OK;
}

}  // extern "C"
