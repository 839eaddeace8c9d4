// What the voxel gather (nlosgr_backproject.hip: back-projection of confocal, non-confocal and phasor-field
// captures) and the voxel scatter (nlosgr_forward_project.hip: their adjoint) both use: where a pair's laser
// distance comes from, the distances and weights of a (voxel, measurement) pair, the grid part of a kernel's
// arguments, and the host checks with their error texts.  Code that one of the two files uses alone lives in
// that file.
#pragma once
#include "nlosgr_common.hpp"

namespace nlosgr {
namespace detail {

constexpr int kProjMaxExtent = 1024;

// where a pair's laser distance comes from.  kConfocal: the laser is the sensed point, one distance d.
// kPerMeas: lasers[i] belongs to measurement i.  kOneLaser: one spot for the whole capture, so the laser distance
// depends on the voxel alone and is formed outside the loop over the measurements: the same values in the same
// order as with the spot repeated nmeas times, so the same bits.
enum { kConfocal = 0, kPerMeas = 1, kOneLaser = 2 };

// the mode of a capture with lasers (one spot for a capture of one measurement is launched as the general case:
// the same bits, and no more kernels)
inline int laser_mode(int32_t nlaser, int32_t nmeas) { return nlaser == 1 && nmeas > 1 ? kOneLaser : kPerMeas; }

// the confocal weight d^POWER (a negative power: its reciprocal)
template <int POWER>
__device__ __forceinline__ float conf_weight(float d) {
    constexpr int P = POWER < 0 ? -POWER : POWER;
    if (P == 0) return 1.0f;
    const float d2 = d * d;
    const float p = P == 1 ? d : (P == 2 ? d2 : (P == 3 ? d2 * d : d2 * d2));
    return POWER < 0 ? 1.0f / p : p;
}

// the non-confocal weight m^(POWER/2) from m = dl * ds.  With the laser on the sensor m = d*d, so the even
// powers give conf_weight's bits; the odd ones differ by the rounding of sqrt(d*d) against d
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

// sqrt((dx*dx + dy*dy) + dz*dz): fp32, this order, no contraction, the hardware square root
__device__ __forceinline__ float nc_dist(float ss, float dz) {
#pragma clang fp contract(off)
    return fsqrt(ss + dz * dz);
}

// the grid part of a kernel's arguments
struct ProjGrid {
    int nx, ny, nz;
    const float *xs, *ys, *zs;
};

inline ProjGrid proj_grid(const nlosgr_voxel_grid* g) { return {g->nx, g->ny, g->nz, g->xs, g->ys, g->zs}; }

inline int check_grid(const nlosgr_voxel_grid* g) {
    if (g->nx < 1 || g->ny < 1 || g->nz < 1 || g->nx > kProjMaxExtent || g->ny > kProjMaxExtent ||
        g->nz > kProjMaxExtent)
        return set_err(NLOSGR_E_INVALID, "voxel grid extents must be in 1..1024");
    return NLOSGR_OK;
}

inline int check_window(float r0, float inv_dr) {
    if (!(inv_dr > 0.0f) || !(inv_dr <= 3.0e38f)) return set_err(NLOSGR_E_INVALID, "inv_dr must be finite and > 0");
    if (!(fabsf(r0) <= 3.0e38f)) return set_err(NLOSGR_E_INVALID, "r0 must be finite");
    return NLOSGR_OK;
}

// lo = 0: a gather; lo = -4: a scatter
inline int check_power(int power, int lo) {
    if (power >= lo && power <= 4) return NLOSGR_OK;
    return set_err(NLOSGR_E_INVALID, lo < 0 ? "forward-projection power must be in -4..4"
                                            : "back-projection power must be in 0..4");
}

inline int check_nlaser(int mode, int32_t nlaser, int32_t nmeas) {
    if (mode != kConfocal && nlaser != 1 && nlaser != nmeas)
        return set_err(NLOSGR_E_INVALID, "nlaser must be 1 or nmeas");
    return NLOSGR_OK;
}

}  // namespace detail
}  // namespace nlosgr
