// Back-projection of a capture onto a regular voxel grid (gfx950): the voxel-wise sum of every measurement's
// histogram at the voxel's time of flight, the baseline every NLOS reconstruction is compared with.  One gather
// kernel serves the three entry points (include/nlosgr.h, ABI 13): nlosgr_backproject (confocal, real rows),
// nlosgr_backproject_nc (a laser spot per measurement or one for the capture, real rows) and
// nlosgr_backproject_phasor (any of the three, complex rows).  For voxel centre x (grid tables) and
// measurement i with sensed wall point s_i and laser spot l_i, all fp32 with no contraction:
//
//     confocal:      d  = |x - s_i|                  sqrt((dx*dx + dy*dy) + dz*dz), the hardware square root
//                    g  = d,  weight = d^power       as d, d*d, (d*d)*d, (d*d)*(d*d)
//     non-confocal:  ds = |x - s_i|, dl = |x - l_i|
//                    g  = 0.5f * (dl + ds)           half the path: the confocal d, exactly, when l_i == s_i
//                    m  = dl * ds,  weight = m^(power/2):  0: 1;  1: sqrt(m);  2: m;  3: m*sqrt(m);  4: m*m
//     u = (g - r0) * inv_dr,  k = floor(u),  f = u - k
//     s_i[c] = (1-f) h_i[k][c] + f h_i[k+1][c]       h_i[j] = 0 for j < 0 or j >= nr
//     out[c](x) = sum_i weight s_i[c]                 c < CH: 1 plane of real rows, 2 (re, im) of complex rows
//     mag(x)    = (float)sqrt((double)re*re + (double)im*im)     of the fp32 plane values (CH = 2, if asked for)
//
// So with lasers == sensors the even powers give the confocal numbers bit for bit; the odd powers differ by the
// rounding of sqrt(d*d) against d.  The tap of a pair (k, f, weight) is formed once and shared by the channels,
// and each channel goes through bp_eval in channel order, so every plane of complex rows is bitwise what the
// real rows of that channel alone give.
//
// Shape: a workgroup owns one 8x8x8 brick, z fastest; a lane owns two voxels adjacent in z and shares
// dx*dx + dy*dy between them, so the 64 gathers a wave issues into one row (2 x 8 x 8 voxels) span a few tens of
// bins: a few consecutive cache lines.  Measurements stream through LDS in tiles of 256 positions (float4,
// w unused; a second tile of laser spots with kPerMeas only), the row base is wave-uniform (scalar), the bin
// index is the lane's.  Every workgroup walks the capture in the same order, so a row is fetched from HBM about
// once and otherwise served by L2 / the Infinity Cache.
//
// Contract: measurements in ascending order, in tiles of 256 counted from this call's measurement 0; a tile is
// summed term by term in fp32 (started at 0), the tile sums are added into a per-voxel, per-channel fp64
// register, rounded to fp32 once at the end.  No atomics: bitwise repeatable, and a voxel's value depends on its
// table coordinates and the capture alone, not on the brick or lane it lands in.  The square root is the hardware
// v_sqrt_f32 (__builtin_amdgcn_sqrtf, 1 ulp): parity is judged against float64, not torch bit-exactness.
// A pair's two bins come from one read clamped into the row (8 bytes of real rows, 16 of complex ones; a
// one-bin row: its bin alone) and the values that are not the pair's bins are dropped by selects, so no lane
// ever reads outside its row, whatever u is.
#include "nlosgr_project.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

constexpr int kBpTile = 256;     // measurements per LDS tile (the summation contract's tile)
constexpr int kBpBrick = 8;      // brick edge (voxels)
constexpr int kBpGroup = 4;      // measurements whose bin reads a lane keeps in flight together

static_assert(kBpTile == kBlock, "one measurement per thread when a tile is staged");
static_assert(kBpBrick * kBpBrick * kBpBrick == 2 * kBlock, "two voxels per lane");

// one (voxel, measurement) pair before its bins are read.  Both bins come from ONE read at bin
// kb = clamp(k, 0, nr - 2) (aligned to a bin, always inside the row), which halves the gather's memory
// instructions; e = k - kb says which of the two values are the pair's bins: 0: (h[k], h[k+1]) = (x, y);
// -1 (k = -1): (0, x);  1 (k = nr - 1): (y, 0);  anything else: both outside the row
struct BpTap {
    unsigned ib;   // byte offset of bin kb into a row of real bins
    int e;
    float f, w;    // f, the pair's weight
};

struct __attribute__((packed, aligned(4))) BpBins {
    float x, y;
};

// weight * ((1-f) h[k] + f h[k+1]); a value that is not one of the pair's bins is dropped by a select, so
// its NaN does not leak
template <int POWER>
__device__ __forceinline__ float bp_eval(const BpTap& t, const BpBins v) {
    const float h0 = t.e == 0 ? v.x : (t.e == 1 ? v.y : 0.0f);
    const float h1 = t.e == 0 ? v.y : (t.e == -1 ? v.x : 0.0f);
    const float s = fmaf(t.f, h1, (1.0f - t.f) * h0);
    return POWER == 0 ? s : t.w * s;
}

// a confocal pair as a BpTap: ss = dx*dx + dy*dy (shared by the lane's two voxels); kmax = max(nr - 2, 0)
template <int POWER>
__device__ __forceinline__ BpTap conf_tap(float ss, float dz, float r0, float inv_dr, int kmax, float umax) {
#pragma clang fp contract(off)
    BpTap t;
    const float d = fsqrt(ss + dz * dz);
    // clamped to [-2, nr + 1]: both bins are outside the row at either end (a NaN u goes to -2: no light)
    const float u = fminf(fmaxf((d - r0) * inv_dr, -2.0f), umax);
    const float kf = floorf(u);
    const int k = (int)kf;
    const int kb = min(max(k, 0), kmax);
    t.f = u - kf;
    t.w = conf_weight<POWER>(d);
    t.ib = 4u * (unsigned)kb;
    t.e = k - kb;
    return t;
}

// a non-confocal pair from its laser and sensor distances: conf_tap with g for d in u and dl * ds for d * d
template <int POWER>
__device__ __forceinline__ BpTap nc_tap(float dl, float ds, float r0, float inv_dr, int kmax, float umax) {
#pragma clang fp contract(off)
    BpTap t;
    const float g = 0.5f * (dl + ds);
    const float u = fminf(fmaxf((g - r0) * inv_dr, -2.0f), umax);
    const float kf = floorf(u);
    const int k = (int)kf;
    const int kb = min(max(k, 0), kmax);
    t.f = u - kf;
    t.w = POWER == 0 ? 1.0f : nc_weight<POWER>(dl * ds);
    t.ib = 4u * (unsigned)kb;
    t.e = k - kb;
    return t;
}

// point i of a [n][3] list as a float4 (w unused), zeros past the end
__device__ __forceinline__ float4 bp_point(const float* p, int i, int n) {
    return i < n ? make_float4(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2], 0.f)
                 : make_float4(0.f, 0.f, 0.f, 0.f);
}

// rows of interleaved (re, im) bins: both complex bins of a pair come from ONE 16-byte read at complex bin kb
// (byte offset 2 * BpTap::ib: 8-byte aligned, always inside the row)
struct __attribute__((packed, aligned(8))) BpBinsC {
    float re0, im0, re1, im1;
};

struct __attribute__((packed, aligned(8))) BpBinC {
    float re, im;
};

// what a lane reads for one pair, by channel count.  PAIR: rows of two or more bins, one read of both; a one-bin
// row reads its bin alone (bin 1 is outside: 0).  channel(v, c): the two values of channel c as bp_eval takes them
template <int CH>
struct BpRow;

template <>
struct BpRow<1> {
    using Bins = BpBins;
    template <bool PAIR>
    static __device__ __forceinline__ Bins read(const char* r, unsigned ib) {
        if (PAIR) return *(const BpBins*)(r + ib);
        BpBins v;
        v.x = *(const float*)r;
        v.y = 0.0f;
        return v;
    }
    static __device__ __forceinline__ BpBins channel(const Bins& v, int) { return v; }
};

template <>
struct BpRow<2> {
    using Bins = BpBinsC;
    template <bool PAIR>
    static __device__ __forceinline__ Bins read(const char* r, unsigned ib) {
        if (PAIR) return *(const BpBinsC*)(r + 2u * ib);
        const BpBinC b = *(const BpBinC*)r;
        BpBinsC v;
        v.re0 = b.re; v.im0 = b.im;
        v.re1 = 0.0f; v.im1 = 0.0f;
        return v;
    }
    static __device__ __forceinline__ BpBins channel(const Bins& v, int c) {
        BpBins b;
        b.x = c ? v.im0 : v.re0;
        b.y = c ? v.im1 : v.re1;
        return b;
    }
};

struct GatherArgs {
    const float* rows;       // [nmeas][nr][CH]
    const float* sensors;    // (the confocal capture's wall points)
    const float* lasers;     // kPerMeas: [nmeas][3]; kOneLaser: [3]; kConfocal: unused
    int nmeas, nr;
    ProjGrid g;
    int nby, nbz;
    float r0, inv_dr;
    int accumulate;
    float* out;              // [CH][nvox]
    float* mag;              // CH = 2: [nvox] or null
};

__device__ __forceinline__ float ph_mag(float re, float im) {
    return (float)sqrt((double)re * (double)re + (double)im * (double)im);
}

// measurements [j, j + N) of the staged tile: every bin offset first, then all 2 N reads, then the sums in
// measurement order, each channel through bp_eval (the reads of N measurements are in flight together; the
// order of the additions is the contract's).  dl0, dl1: the lane's two laser distances (kOneLaser)
template <int POWER, bool PAIR, int MODE, int CH, int N>
__device__ __forceinline__ void gather_step(const float4* stile, const float4* ltile, int j,
                                            const float* __restrict__ row, const GatherArgs& a, float x, float y,
                                            float z0, float z1, float dl0, float dl1, int kmax, float umax,
                                            float (&s0)[CH], float (&s1)[CH]) {
    using Row = BpRow<CH>;
    BpTap ta[N], tb[N];
    typename Row::Bins va[N], vb[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const float4 w = stile[j + q];
        const float ss = nc_ss(x, y, w.x, w.y);
        if (MODE == kConfocal) {
            ta[q] = conf_tap<POWER>(ss, z0 - w.z, a.r0, a.inv_dr, kmax, umax);
            tb[q] = conf_tap<POWER>(ss, z1 - w.z, a.r0, a.inv_dr, kmax, umax);
        } else {
            float la = dl0, lb = dl1;
            if (MODE == kPerMeas) {
                const float4 l = ltile[j + q];
                const float sl = nc_ss(x, y, l.x, l.y);
                la = nc_dist(sl, z0 - l.z);
                lb = nc_dist(sl, z1 - l.z);
            }
            ta[q] = nc_tap<POWER>(la, nc_dist(ss, z0 - w.z), a.r0, a.inv_dr, kmax, umax);
            tb[q] = nc_tap<POWER>(lb, nc_dist(ss, z1 - w.z), a.r0, a.inv_dr, kmax, umax);
        }
    }
#pragma unroll
    for (int q = 0; q < N; ++q) {
        // wave-uniform row base + the lane's 32-bit byte offset (nr <= 2^29 bins is far above any capture)
        const char* r = (const char*)(row + CH * (size_t)q * a.nr);
        va[q] = Row::template read<PAIR>(r, ta[q].ib);
        vb[q] = Row::template read<PAIR>(r, tb[q].ib);
    }
#pragma unroll
    for (int q = 0; q < N; ++q) {
#pragma unroll
        for (int c = 0; c < CH; ++c) s0[c] += bp_eval<POWER>(ta[q], Row::channel(va[q], c));
#pragma unroll
        for (int c = 0; c < CH; ++c) s1[c] += bp_eval<POWER>(tb[q], Row::channel(vb[q], c));
    }
}

template <int POWER, bool PAIR, int MODE, int CH>
__global__ __launch_bounds__(kBlock) void gather_kernel(GatherArgs a) {
    __shared__ float4 stile[kBpTile];
    __shared__ float4 ltile[MODE == kPerMeas ? kBpTile : 1];
    const int t = threadIdx.x;
    const int nx = a.g.nx, ny = a.g.ny, nz = a.g.nz;
    const int bz = blockIdx.x % a.nbz, by = (blockIdx.x / a.nbz) % a.nby, bx = blockIdx.x / (a.nbz * a.nby);
    // lane -> (x, y, z pair) of the brick, z fastest: a wave covers 2 x 8 x 8 voxels
    const int ix = bx * kBpBrick + (t >> 5), iy = by * kBpBrick + ((t >> 2) & 7), iz = bz * kBpBrick + 2 * (t & 3);
    const float x = a.g.xs[min(ix, nx - 1)], y = a.g.ys[min(iy, ny - 1)];
    const float z0 = a.g.zs[min(iz, nz - 1)], z1 = a.g.zs[min(iz + 1, nz - 1)];
    const float umax = (float)(a.nr + 1);
    const int kmax = max(a.nr - 2, 0);
    float dl0 = 0.0f, dl1 = 0.0f;
    if (MODE == kOneLaser) {
        const float lx = a.lasers[0], ly = a.lasers[1], lz = a.lasers[2];
        const float sl = nc_ss(x, y, lx, ly);
        dl0 = nc_dist(sl, z0 - lz);
        dl1 = nc_dist(sl, z1 - lz);
    }
    double acc0[CH], acc1[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc0[c] = acc1[c] = 0.0;
    for (int base = 0; base < a.nmeas; base += kBpTile) {
        __syncthreads();
        stile[t] = bp_point(a.sensors, base + t, a.nmeas);
        if (MODE == kPerMeas) ltile[t] = bp_point(a.lasers, base + t, a.nmeas);
        __syncthreads();
        const int n = min(kBpTile, a.nmeas - base);
        const float* row = a.rows + CH * (size_t)base * a.nr;
        float s0[CH], s1[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) s0[c] = s1[c] = 0.0f;
        int j = 0;
        for (; j + kBpGroup <= n; j += kBpGroup, row += CH * (size_t)kBpGroup * a.nr)
            gather_step<POWER, PAIR, MODE, CH, kBpGroup>(stile, ltile, j, row, a, x, y, z0, z1, dl0, dl1, kmax, umax,
                                                         s0, s1);
        for (; j < n; ++j, row += CH * (size_t)a.nr)
            gather_step<POWER, PAIR, MODE, CH, 1>(stile, ltile, j, row, a, x, y, z0, z1, dl0, dl1, kmax, umax, s0, s1);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            acc0[c] += (double)s0[c];
            acc1[c] += (double)s1[c];
        }
    }
    if (ix < nx && iy < ny && iz < nz) {
        const size_t nvox = (size_t)nx * ny * nz;
        const size_t o = ((size_t)ix * ny + iy) * nz + iz;
        // the lane's voxel at o, then the one at o + 1 if it is inside the grid
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            if (v == 1 && !(iz + 1 < nz)) break;
            float r[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                float* const p = a.out + c * nvox + o + v;
                r[c] = (float)(v ? acc1[c] : acc0[c]);
                if (a.accumulate) r[c] = *p + r[c];
                *p = r[c];
            }
            if (CH == 2 && a.mag) a.mag[o + v] = ph_mag(r[0], r[CH - 1]);
        }
    }
}

// nmeas == 0: the magnitude of the planes as they are
__global__ __launch_bounds__(kBlock) void phasor_mag_kernel(const float* __restrict__ planes, size_t nvox, float* mag) {
    const size_t o = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (o < nvox) mag[o] = ph_mag(planes[o], planes[nvox + o]);
}

// the error texts of an entry point
struct GatherText {
    const char *count, *out, *rows;
};

// all three entry points.  CH planes of nvox floats at out; lasers == NULL: confocal; laser_err: what is wrong
// with the entry's laser count, or NULL; need_lasers: a capture with measurements must have lasers
int gather(int ch, const float* rows, const float* sensors, const float* lasers, int32_t nlaser, const char* laser_err,
           bool need_lasers, int32_t nmeas, int32_t nr, const nlosgr_voxel_grid* grid, const nlosgr_backproject_opts* opt,
           float* out, float* mag, void* hip_stream, const GatherText& text) {
    if (!grid || !opt) return set_err(NLOSGR_E_INVALID, "null argument struct");
    if (check_grid(grid) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (nr < 1) return set_err(NLOSGR_E_INVALID, "nr must be >= 1");
    if (nmeas < 0) return set_err(NLOSGR_E_INVALID, text.count);
    if (laser_err) return set_err(NLOSGR_E_INVALID, laser_err);
    if (check_power(opt->power, 0) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (check_window(opt->r0, opt->inv_dr) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (!grid->xs || !grid->ys || !grid->zs) return set_err(NLOSGR_E_INVALID, "null voxel grid table");
    if (!out) return set_err(NLOSGR_E_INVALID, text.out);
    if (nmeas > 0 && (!rows || !sensors)) return set_err(NLOSGR_E_INVALID, text.rows);
    if (nmeas > 0 && need_lasers && !lasers) return set_err(NLOSGR_E_INVALID, "null lasers pointer");
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t nvox = (size_t)grid->nx * grid->ny * grid->nz;
    if (nmeas == 0) {
        if (!opt->accumulate) HIPCHK(hipMemsetAsync(out, 0, ch * nvox * sizeof(float), s));
        if (mag) {
            hipLaunchKernelGGL(phasor_mag_kernel, dim3((unsigned)((nvox + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                               out, nvox, mag);
            HIPCHK(hipGetLastError());
        }
        return NLOSGR_OK;
    }
    GatherArgs a;
    a.rows = rows; a.sensors = sensors; a.lasers = lasers; a.nmeas = nmeas; a.nr = nr;
    a.g = proj_grid(grid);
    a.nby = (grid->ny + kBpBrick - 1) / kBpBrick; a.nbz = (grid->nz + kBpBrick - 1) / kBpBrick;
    a.r0 = opt->r0; a.inv_dr = opt->inv_dr; a.accumulate = opt->accumulate != 0;
    a.out = out; a.mag = mag;
    const unsigned nbricks = (unsigned)((grid->nx + kBpBrick - 1) / kBpBrick) * a.nby * a.nbz;   // <= 128^3
    const int mode = !lasers ? kConfocal : laser_mode(nlaser, nmeas);
    dispatch_int<0, 4>(opt->power, [&](auto P) {
        dispatch_int<0, 1>(nr >= 2, [&](auto PAIR) {
            dispatch_int<kConfocal, kOneLaser>(mode, [&](auto MODE) {
                dispatch_int<1, 2>(ch, [&](auto CH) {
                    hipLaunchKernelGGL((gather_kernel<decltype(P)::value, decltype(PAIR)::value != 0, decltype(MODE)::value,
                                                      decltype(CH)::value>), dim3(nbricks),
                                       dim3(kBlock), 0, s, a);
                });
            });
        });
    });
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

}  // namespace

extern "C" {

int nlosgr_backproject(const float* rows, const float* walls, int32_t nwall, int32_t nr, const nlosgr_voxel_grid* grid,
                       const nlosgr_backproject_opts* opt, float* out, void* hip_stream) {
    return gather(1, rows, walls, nullptr, 0, nullptr, false, nwall, nr, grid, opt, out, nullptr, hip_stream,
                  {"nwall must be >= 0", "null back-projection output", "null rows or walls pointer"});
}

int nlosgr_backproject_nc(const float* rows, const float* sensors, const float* lasers, int32_t nlaser, int32_t nmeas,
                          int32_t nr, const nlosgr_voxel_grid* grid, const nlosgr_backproject_opts* opt, float* out,
                          void* hip_stream) {
    // (without lasers and without measurements there is nothing to launch; the mode is never confocal here)
    const char* laser_err = nlaser != 1 && nlaser != nmeas ? "nlaser must be 1 or nmeas" : nullptr;
    return gather(1, rows, sensors, lasers, nlaser, laser_err, true, nmeas, nr, grid, opt, out, nullptr, hip_stream,
                  {"nmeas must be >= 0", "null back-projection output", "null rows or sensors pointer"});
}

int nlosgr_backproject_phasor(const float* rows_c, const float* sensors, const float* lasers, int32_t nlaser,
                              int32_t nmeas, int32_t nr, const nlosgr_voxel_grid* grid,
                              const nlosgr_backproject_opts* opt, float* planes, float* mag, void* hip_stream) {
    const char* laser_err = !lasers ? (nlaser != 0 ? "nlaser must be 0 without lasers (confocal)" : nullptr)
                                    : (nlaser != 1 && nlaser != nmeas ? "nlaser must be 1 or nmeas" : nullptr);
    return gather(2, rows_c, sensors, lasers, nlaser, laser_err, false, nmeas, nr, grid, opt, planes, mag, hip_stream,
                  {"nmeas must be >= 0", "null phasor planes output", "null rows or sensors pointer"});
}

}  // extern "C"
