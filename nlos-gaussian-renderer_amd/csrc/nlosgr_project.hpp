// What the confocal voxel operators (nlosgr_backproject.hip, nlosgr_forward_project.hip) and the non-confocal
// ones (nlosgr_nonconfocal.hip) share with each other and with the phasor-field gather (nlosgr_phasor.hip): the
// back-projection's tile shape, its per-pair arithmetic (bp_tap, nc_tap and their weights) and its two-bin read,
// the forward projector's workspace layout, quantum, max|vol| reduction, finish kernel and split count.
// Everything here but the complex read is those operators' code moved unchanged, so their results are bitwise
// what they were.
#pragma once
#include "nlosgr_common.hpp"

namespace nlosgr {
namespace detail {

// ------------------------------------------------------------------------------------------
// back-projection
// ------------------------------------------------------------------------------------------
constexpr int kBpTile = 256;     // wall points per LDS tile (the summation contract's tile)
constexpr int kBpBrick = 8;      // brick edge (voxels)
constexpr int kBpGroup = 4;      // wall points whose bin reads a lane keeps in flight together
constexpr int kBpMaxExtent = 1024;

static_assert(kBpTile == kBlock, "one wall point per thread when a tile is staged");
static_assert(kBpBrick * kBpBrick * kBpBrick == 2 * kBlock, "two voxels per lane");

// one (voxel, wall point) pair before its bins are read.  Both bins come from ONE 8-byte read at bin
// kb = clamp(k, 0, nr - 2) (4-byte aligned, always inside the row), which halves the gather's memory
// instructions; e = k - kb says which of the two values are the pair's bins: 0: (h[k], h[k+1]) = (x, y);
// -1 (k = -1): (0, x);  1 (k = nr - 1): (y, 0);  anything else: both outside the row
struct BpTap {
    unsigned ib;   // byte offset of bin kb into the row
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

// PAIR: rows of two or more bins, one 8-byte read; a one-bin row reads its bin alone (y = 0: bin 1 is outside)
template <bool PAIR>
__device__ __forceinline__ BpBins bp_read(const char* r, unsigned ib) {
    if (PAIR) return *(const BpBins*)(r + ib);
    BpBins v;
    v.x = *(const float*)r;
    v.y = 0.0f;
    return v;
}

// the confocal weight d^POWER
template <int POWER>
__device__ __forceinline__ float bp_weight(float d) {
    if (POWER == 0) return 1.0f;
    if (POWER == 1) return d;
    const float d2 = d * d;
    if (POWER == 2) return d2;
    if (POWER == 3) return d2 * d;
    return d2 * d2;
}

// one (voxel, wall point) pair as a BpTap (the two-bin read and its selects)
// ss = dx*dx + dy*dy (shared by the lane's two voxels); kmax = max(nr - 2, 0)
template <int POWER>
__device__ __forceinline__ BpTap bp_tap(float ss, float dz, float r0, float inv_dr, int kmax, float umax) {
#pragma clang fp contract(off)
    BpTap t;
    const float d = fsqrt(ss + dz * dz);
    // clamped to [-2, nr + 1]: both bins are outside the row at either end (a NaN u goes to -2: no light)
    const float u = fminf(fmaxf((d - r0) * inv_dr, -2.0f), umax);
    const float kf = floorf(u);
    const int k = (int)kf;
    const int kb = min(max(k, 0), kmax);
    t.f = u - kf;
    t.w = bp_weight<POWER>(d);
    t.ib = 4u * (unsigned)kb;
    t.e = k - kb;
    return t;
}

// the non-confocal weight m^(|POWER|/2) from m = dl * ds
template <int POWER>
__device__ __forceinline__ float nc_weight(float m) {
    constexpr int P = POWER < 0 ? -POWER : POWER;
    if (P == 0) return 1.0f;
    float p;
    if (P == 2) p = m;
    else if (P == 4) p = m * m;
    else {
        const float r = fsqrt(m);
        p = P == 1 ? r : m * r;
    }
    return POWER < 0 ? 1.0f / p : p;
}

// ss = dx*dx + dy*dy of a (voxel column, point) pair
__device__ __forceinline__ float nc_ss(float x, float y, float px, float py) {
#pragma clang fp contract(off)
    const float dx = x - px, dy = y - py;
    return dx * dx + dy * dy;
}

__device__ __forceinline__ float nc_dist(float ss, float dz) {
#pragma clang fp contract(off)
    return fsqrt(ss + dz * dz);
}

// one (voxel, measurement) pair of a non-confocal capture before its bins are read; kmax = max(nr - 2, 0)
template <int POWER>
__device__ __forceinline__ BpTap nc_tap(float dl, float ds, float r0, float inv_dr, int kmax, float umax) {
#pragma clang fp contract(off)
    BpTap t;
    const float g = 0.5f * (dl + ds);
    // clamped to [-2, nr + 1]: both bins are outside the row at either end (a NaN u goes to -2: no light)
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
__device__ __forceinline__ float4 nc_point(const float* p, int i, int n) {
    return i < n ? make_float4(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2], 0.f)
                 : make_float4(0.f, 0.f, 0.f, 0.f);
}

// the phasor-field gather (nlosgr_phasor.hip): rows of interleaved (re, im) bins.  Both complex bins of a pair
// come from ONE 16-byte read at complex bin kb (byte offset 2 * BpTap::ib: 8-byte aligned, always inside the
// row); each channel is then a BpBins for bp_eval
struct __attribute__((packed, aligned(8))) BpBinsC {
    float re0, im0, re1, im1;
};

struct __attribute__((packed, aligned(8))) BpBinC {
    float re, im;
};

// PAIR: rows of two or more complex bins, one 16-byte read; a one-bin row reads its bin alone (8 bytes)
template <bool PAIR>
__device__ __forceinline__ BpBinsC bp_read_c(const char* r, unsigned ib) {
    if (PAIR) return *(const BpBinsC*)(r + 2u * ib);
    const BpBinC b = *(const BpBinC*)r;
    BpBinsC v;
    v.re0 = b.re; v.im0 = b.im;
    v.re1 = 0.0f; v.im1 = 0.0f;
    return v;
}

// ------------------------------------------------------------------------------------------
// forward projection
// ------------------------------------------------------------------------------------------
constexpr int kFpRun = 4;                 // voxels adjacent in z that one lane owns per step
constexpr int kFpStep = kFpRun * kBlock;   // voxels a workgroup covers per step
constexpr int kFpMaxExtent = 1024;
constexpr int kFpHeader = 256;             // workspace: [0] the bits of max|vol|; the int64 rows start here
constexpr unsigned kFpTargetGroups = 1024; // the library's nsplit fills 256 CUs four times over
constexpr size_t kFpRowBytes = 32768;      // LDS rows of a workgroup that serves more than one wall point
constexpr double kFpWeightMargin = 1.0 + 1.0 / 524288.0;   // 1 + 2^-19: fp32 error of d^power at the window's end

// scale 2^(S - e) of a term to quanta and 2^(e - S) back, e = ev + ew with max|vol| = m 2^ev, m in [0.5, 1)
__device__ __forceinline__ void fp_unit(unsigned vbits, int ew, int S, double& to_q, double& from_q) {
    int ev;
    (void)frexp((double)__uint_as_float(vbits), &ev);
    to_q = ldexp(1.0, S - (ev + ew));
    from_q = ldexp(1.0, (ev + ew) - S);
}

static __global__ __launch_bounds__(kBlock) void fp_vmax_kernel(const float* __restrict__ vol, unsigned n,
                                                                unsigned* out) {
    unsigned m = 0u;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
        m = max(m, __float_as_uint(vol[i]) & 0x7fffffffu);      // |v| as bits: ordered as the values, NaN on top
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if (lane_id() == 0 && m) atomicMax(out, m);
}

// nsplit > 1: the int64 sums of every (wall point, bin) to floats
static __global__ __launch_bounds__(kBlock) void fp_finish_kernel(const unsigned long long* __restrict__ acc, size_t n,
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

inline int fp_ceil_log2(unsigned long long v) {      // the least b with v <= 2^b
    int b = 0;
    while ((1ull << b) < v) ++b;
    return b;
}

// wall points per workgroup: the most of 4, 2, 1 that the wall has and whose rows fit kFpRowBytes of LDS
inline int fp_walls_per_group(int nwall, int nr) {
#ifdef NLOSGR_FP_ONEWALL
    return 1;                          // A/B build: every workgroup walks the volume for one wall point
#else
    int w = 4;
    while (w > 1 && (w > nwall || (size_t)w * nr * sizeof(unsigned long long) > kFpRowBytes)) w >>= 1;
    return w;
#endif
}

// the voxel splits per wall point of a validated call (opt_nsplit: 0 = the library's choice, else forced)
inline int fp_split_count(int32_t nwall, int32_t nr, const nlosgr_voxel_grid* grid, int32_t opt_nsplit, int* nsplit) {
    const unsigned nvox = (unsigned)grid->nx * grid->ny * grid->nz;
    // the library's choice: no split below one step of a workgroup; a forced count: no split below one lane's run
    const unsigned most = opt_nsplit ? (nvox + kFpRun - 1) / kFpRun : (nvox + kFpStep - 1) / kFpStep;
    const int W = fp_walls_per_group(nwall, nr);
    const unsigned groups = nwall > 0 ? (unsigned)((nwall + W - 1) / W) : 1u;
    unsigned ns = opt_nsplit ? (unsigned)opt_nsplit : (kFpTargetGroups + groups - 1) / groups;
    if (ns > most) ns = most;
    if (ns < 1) ns = 1;
    if ((unsigned long long)ns * groups > 0x7fffffffull)
        return set_err(NLOSGR_E_UNSUPPORTED, "workgroups * nsplit above 2^31 - 1");
    *nsplit = (int)ns;
    return NLOSGR_OK;
}

}  // namespace detail
}  // namespace nlosgr
