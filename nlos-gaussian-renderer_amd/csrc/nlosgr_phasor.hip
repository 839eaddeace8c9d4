// Phasor-field reconstruction (gfx950): the back-projection of COMPLEX rows in one pass.  The rows are the
// capture filtered in time with a complex Morlet wavelet (the virtual illumination; nlosgr/phasor.py), stored
// as interleaved (re, im) bins; the image is the magnitude of their back-projection.  For voxel centre x and
// measurement i (include/nlosgr.h, ABI 13):
//
//     planes[c](x) = sum_i weight_i(x) ((1-f) h_i[k][c] + f h_i[k+1][c])      c = 0 (re), 1 (im)
//     mag(x)       = (float)sqrt((double)re*re + (double)im*im)               of the fp32 plane values
//
// Each plane is bitwise what nlosgr_backproject (lasers == NULL) or nlosgr_backproject_nc gives for that channel
// alone: the per-pair arithmetic is theirs (bp_tap / nc_tap of nlosgr_project.hpp, ONE_LASER's hoist included),
// formed once per pair and shared by both channels, each channel goes through bp_eval, and the summation contract
// is theirs: measurements in ascending order in tiles of 256 counted from measurement 0, an fp32 sum within a tile
// (started at 0), an fp64 sum across tiles, one rounding to fp32.  No atomics.
//
// What is new per pair is the read: ONE 16-byte load of (re[kb], im[kb], re[kb+1], im[kb+1]) at complex bin
// kb = clamp(k, 0, nr - 2): 8-byte aligned and always inside the row (a one-bin row: one 8-byte load of its bin).
// Two real back-projections pay twice for the square roots, floors, clamps and tile staging of every pair and
// issue two 8-byte reads where this issues one.
//
// Shape: as backproject_kernel / nc_backproject_kernel: 8^3 bricks, two z-adjacent voxels per lane, measurements
// staged through LDS in tiles of 256, kBpGroup measurements in flight per lane (2 x 4 x 4 value registers beside
// the taps).
#include "nlosgr_project.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

enum { kPhConfocal = 0, kPhPerMeas = 1, kPhOneLaser = 2 };   // where a pair's laser distance comes from

// measurements in flight per lane.  The summation order does not depend on it (A/B build: -DNLOSGR_PH_GROUP=2)
#ifndef NLOSGR_PH_GROUP
#define NLOSGR_PH_GROUP kBpGroup
#endif
constexpr int kPhGroup = NLOSGR_PH_GROUP;

struct PhArgs {
    const float* rows;       // [nmeas][nr][2]
    const float* sensors;
    const float* lasers;
    int nmeas, nr;
    int nx, ny, nz;
    const float *xs, *ys, *zs;
    int nby, nbz;
    float r0, inv_dr;
    int accumulate;
    float* planes;           // [2][nvox]
    float* mag;              // [nvox] or null
};

__device__ __forceinline__ float ph_mag(float re, float im) {
    return (float)sqrt((double)re * (double)re + (double)im * (double)im);
}

// measurements [j, j + N) of the staged tile: every bin offset first, then all 2 N reads, then the sums in
// measurement order, each channel through bp_eval.  dl0, dl1: the lane's two laser distances (kPhOneLaser)
template <int POWER, bool PAIR, int MODE, int N>
__device__ __forceinline__ void ph_step(const float4* stile, const float4* ltile, int j, const float* __restrict__ row,
                                        const PhArgs& a, float x, float y, float z0, float z1, float dl0, float dl1,
                                        int kmax, float umax, float& re0, float& im0, float& re1, float& im1) {
    BpTap ta[N], tb[N];
    BpBinsC va[N], vb[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const float4 w = stile[j + q];
        const float ss = nc_ss(x, y, w.x, w.y);
        if (MODE == kPhConfocal) {
            ta[q] = bp_tap<POWER>(ss, z0 - w.z, a.r0, a.inv_dr, kmax, umax);
            tb[q] = bp_tap<POWER>(ss, z1 - w.z, a.r0, a.inv_dr, kmax, umax);
        } else {
            float la = dl0, lb = dl1;
            if (MODE == kPhPerMeas) {
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
        // wave-uniform row base + the lane's 32-bit byte offset (8 bytes per complex bin)
        const char* r = (const char*)(row + 2 * (size_t)q * a.nr);
        va[q] = bp_read_c<PAIR>(r, ta[q].ib);
        vb[q] = bp_read_c<PAIR>(r, tb[q].ib);
    }
#pragma unroll
    for (int q = 0; q < N; ++q) {
        BpBins c;
        c.x = va[q].re0; c.y = va[q].re1;
        re0 += bp_eval<POWER>(ta[q], c);
        c.x = va[q].im0; c.y = va[q].im1;
        im0 += bp_eval<POWER>(ta[q], c);
        c.x = vb[q].re0; c.y = vb[q].re1;
        re1 += bp_eval<POWER>(tb[q], c);
        c.x = vb[q].im0; c.y = vb[q].im1;
        im1 += bp_eval<POWER>(tb[q], c);
    }
}

template <int POWER, bool PAIR, int MODE>
__global__ __launch_bounds__(kBlock) void phasor_backproject_kernel(PhArgs a) {
    __shared__ float4 stile[kBpTile];
    __shared__ float4 ltile[MODE == kPhPerMeas ? kBpTile : 1];
    const int t = threadIdx.x;
    const int bz = blockIdx.x % a.nbz, by = (blockIdx.x / a.nbz) % a.nby, bx = blockIdx.x / (a.nbz * a.nby);
    // lane -> (x, y, z pair) of the brick, z fastest: a wave covers 2 x 8 x 8 voxels
    const int ix = bx * kBpBrick + (t >> 5), iy = by * kBpBrick + ((t >> 2) & 7), iz = bz * kBpBrick + 2 * (t & 3);
    const float x = a.xs[min(ix, a.nx - 1)], y = a.ys[min(iy, a.ny - 1)];
    const float z0 = a.zs[min(iz, a.nz - 1)], z1 = a.zs[min(iz + 1, a.nz - 1)];
    const float umax = (float)(a.nr + 1);
    const int kmax = max(a.nr - 2, 0);
    float dl0 = 0.0f, dl1 = 0.0f;
    if (MODE == kPhOneLaser) {
        const float lx = a.lasers[0], ly = a.lasers[1], lz = a.lasers[2];
        const float sl = nc_ss(x, y, lx, ly);
        dl0 = nc_dist(sl, z0 - lz);
        dl1 = nc_dist(sl, z1 - lz);
    }
    double are0 = 0.0, aim0 = 0.0, are1 = 0.0, aim1 = 0.0;
    for (int base = 0; base < a.nmeas; base += kBpTile) {
        __syncthreads();
        stile[t] = nc_point(a.sensors, base + t, a.nmeas);
        if (MODE == kPhPerMeas) ltile[t] = nc_point(a.lasers, base + t, a.nmeas);
        __syncthreads();
        const int n = min(kBpTile, a.nmeas - base);
        const float* row = a.rows + 2 * (size_t)base * a.nr;
        float re0 = 0.0f, im0 = 0.0f, re1 = 0.0f, im1 = 0.0f;
        int j = 0;
        for (; j + kPhGroup <= n; j += kPhGroup, row += 2 * (size_t)kPhGroup * a.nr)
            ph_step<POWER, PAIR, MODE, kPhGroup>(stile, ltile, j, row, a, x, y, z0, z1, dl0, dl1, kmax, umax, re0, im0,
                                                 re1, im1);
        for (; j < n; ++j, row += 2 * (size_t)a.nr)
            ph_step<POWER, PAIR, MODE, 1>(stile, ltile, j, row, a, x, y, z0, z1, dl0, dl1, kmax, umax, re0, im0, re1,
                                          im1);
        are0 += (double)re0;
        aim0 += (double)im0;
        are1 += (double)re1;
        aim1 += (double)im1;
    }
    if (ix < a.nx && iy < a.ny && iz < a.nz) {
        const size_t nvox = (size_t)a.nx * a.ny * a.nz;
        const size_t o = ((size_t)ix * a.ny + iy) * a.nz + iz;
        float* const pre = a.planes;
        float* const pim = a.planes + nvox;
        float re = (float)are0, im = (float)aim0;
        if (a.accumulate) { re = pre[o] + re; im = pim[o] + im; }
        pre[o] = re;
        pim[o] = im;
        if (a.mag) a.mag[o] = ph_mag(re, im);
        if (iz + 1 < a.nz) {
            re = (float)are1; im = (float)aim1;
            if (a.accumulate) { re = pre[o + 1] + re; im = pim[o + 1] + im; }
            pre[o + 1] = re;
            pim[o + 1] = im;
            if (a.mag) a.mag[o + 1] = ph_mag(re, im);
        }
    }
}

// nmeas == 0: the magnitude of the planes as they are
__global__ __launch_bounds__(kBlock) void phasor_mag_kernel(const float* __restrict__ planes, size_t nvox, float* mag) {
    const size_t o = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (o < nvox) mag[o] = ph_mag(planes[o], planes[nvox + o]);
}

template <int POWER, bool PAIR>
void ph_launch(int mode, unsigned nbricks, hipStream_t s, const PhArgs& a) {
    if (mode == kPhConfocal)
        hipLaunchKernelGGL((phasor_backproject_kernel<POWER, PAIR, kPhConfocal>), dim3(nbricks), dim3(kBlock), 0, s, a);
    else if (mode == kPhPerMeas)
        hipLaunchKernelGGL((phasor_backproject_kernel<POWER, PAIR, kPhPerMeas>), dim3(nbricks), dim3(kBlock), 0, s, a);
    else
        hipLaunchKernelGGL((phasor_backproject_kernel<POWER, PAIR, kPhOneLaser>), dim3(nbricks), dim3(kBlock), 0, s, a);
}

}  // namespace

extern "C" {

int nlosgr_backproject_phasor(const float* rows_c, const float* sensors, const float* lasers, int32_t nlaser,
                              int32_t nmeas, int32_t nr, const nlosgr_voxel_grid* grid,
                              const nlosgr_backproject_opts* opt, float* planes, float* mag, void* hip_stream) {
    if (!grid || !opt) return set_err(NLOSGR_E_INVALID, "null argument struct");
    if (grid->nx < 1 || grid->ny < 1 || grid->nz < 1 || grid->nx > kBpMaxExtent || grid->ny > kBpMaxExtent ||
        grid->nz > kBpMaxExtent)
        return set_err(NLOSGR_E_INVALID, "voxel grid extents must be in 1..1024");
    if (nr < 1) return set_err(NLOSGR_E_INVALID, "nr must be >= 1");
    if (nmeas < 0) return set_err(NLOSGR_E_INVALID, "nmeas must be >= 0");
    if (!lasers && nlaser != 0) return set_err(NLOSGR_E_INVALID, "nlaser must be 0 without lasers (confocal)");
    if (lasers && nlaser != 1 && nlaser != nmeas) return set_err(NLOSGR_E_INVALID, "nlaser must be 1 or nmeas");
    if (opt->power < 0 || opt->power > 4) return set_err(NLOSGR_E_INVALID, "back-projection power must be in 0..4");
    if (!(opt->inv_dr > 0.0f) || !(opt->inv_dr <= 3.0e38f))
        return set_err(NLOSGR_E_INVALID, "inv_dr must be finite and > 0");
    if (!(fabsf(opt->r0) <= 3.0e38f)) return set_err(NLOSGR_E_INVALID, "r0 must be finite");
    if (!grid->xs || !grid->ys || !grid->zs) return set_err(NLOSGR_E_INVALID, "null voxel grid table");
    if (!planes) return set_err(NLOSGR_E_INVALID, "null phasor planes output");
    if (nmeas > 0 && (!rows_c || !sensors)) return set_err(NLOSGR_E_INVALID, "null rows or sensors pointer");
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t nvox = (size_t)grid->nx * grid->ny * grid->nz;
    if (nmeas == 0) {
        if (!opt->accumulate) HIPCHK(hipMemsetAsync(planes, 0, 2 * nvox * sizeof(float), s));
        if (mag) {
            hipLaunchKernelGGL(phasor_mag_kernel, dim3((unsigned)((nvox + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                               planes, nvox, mag);
            HIPCHK(hipGetLastError());
        }
        return NLOSGR_OK;
    }
    PhArgs a;
    a.rows = rows_c; a.sensors = sensors; a.lasers = lasers; a.nmeas = nmeas; a.nr = nr;
    a.nx = grid->nx; a.ny = grid->ny; a.nz = grid->nz;
    a.xs = grid->xs; a.ys = grid->ys; a.zs = grid->zs;
    a.nby = (grid->ny + kBpBrick - 1) / kBpBrick; a.nbz = (grid->nz + kBpBrick - 1) / kBpBrick;
    a.r0 = opt->r0; a.inv_dr = opt->inv_dr; a.accumulate = opt->accumulate != 0;
    a.planes = planes; a.mag = mag;
    const unsigned nbricks = (unsigned)((grid->nx + kBpBrick - 1) / kBpBrick) * a.nby * a.nbz;   // <= 128^3
    const bool pair = nr >= 2;
    // (one spot for a capture of one measurement is launched as the general case, as nlosgr_backproject_nc does)
    const int mode = !lasers ? kPhConfocal : (nlaser == 1 && nmeas > 1 ? kPhOneLaser : kPhPerMeas);
#define NLOSGR_PH_LAUNCH(P)                               \
    if (pair) ph_launch<P, true>(mode, nbricks, s, a);    \
    else ph_launch<P, false>(mode, nbricks, s, a);        \
    break
    switch (opt->power) {
        case 0: NLOSGR_PH_LAUNCH(0);
        case 1: NLOSGR_PH_LAUNCH(1);
        case 2: NLOSGR_PH_LAUNCH(2);
        case 3: NLOSGR_PH_LAUNCH(3);
        default: NLOSGR_PH_LAUNCH(4);
    }
#undef NLOSGR_PH_LAUNCH
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

}  // extern "C"
