// The wall's lattice, shared by the reconstructions that live on it: f-k migration (nlosgr_fk.hip), the light-cone
// transform (nlosgr_lct.hip) and the fast phasor field (nlosgr_rsd.hip).  Device side: how lattice point (m, n) finds
// its row, the radius of a time bin and its power (so every operator weights a capture with the same fp32
// arithmetic), the signed DFT indices of a padded column.  Host side: the argument checks of the three files'
// entry points, one error text each.
#pragma once
#include "nlosgr_common.hpp"

namespace nlosgr {
namespace detail {

constexpr int kLatticeMaxExtent = 1024;   // H, W, nr (voxelize.VoxelGrid's limit: the volume is [W][nr][H])

// The row of lattice point (m, n): perm[m sm + n sn] (perm NULL: m sm + n sn), clamped to the H W rows.  The
// strides are checked on the host (lattice_check_strides); perm is device memory the entry points do not read, so
// the clamp is what holds there: a bad perm entry reads or writes a wrong row, never outside the rows.
__device__ __forceinline__ int lattice_row(const int* perm, int m, int n, int sm, int sn, int H, int W) {
    int v = m * sm + n * sn;
    if (perm) v = perm[v];
    return min(max(v, 0), H * W - 1);
}

// the radius of time bin j: one fma
__device__ __forceinline__ float bin_radius(int j, float r0, float dr) { return fmaf((float)j, dr, r0); }

// r^|power|, power in -4..4, as 1, r, r r, (r r) r, (r r)(r r)
__device__ __forceinline__ float radius_power(float r, int power) {
#pragma clang fp contract(off)
    const float r2 = r * r;
    const int p = power < 0 ? -power : power;
    return p == 0 ? 1.0f : (p == 1 ? r : (p == 2 ? r2 : (p == 3 ? r2 * r : r2 * r2)));
}

// max(h, 0) (r0 + j dr)^POWER, its square root when AMP (the hardware square root, 1 ulp): the falloff-compensated
// bin of a confocal row, in the load passes of f-k migration and of the light-cone transform
template <int POWER, bool AMP>
__device__ __forceinline__ float fk_psi(float h, int j, float r0, float dr) {
#pragma clang fp contract(off)
    const float w = radius_power(bin_radius(j, r0, dr), POWER);
    const float v = fmaxf(h, 0.0f) * w;
    return AMP ? fsqrt(v) : v;
}

// the signed DFT index of position i of an axis of n lattice points padded to 2 n
__device__ __forceinline__ int dft_signed(int i, int n) { return i < n ? i : i - 2 * n; }

// `what` names the extents in the caller's words: "<what> must be in 1..1024"
inline int lattice_check_extents(const char* what, int32_t H, int32_t W, int32_t nr) {
    if (H >= 1 && W >= 1 && nr >= 1 && H <= kLatticeMaxExtent && W <= kLatticeMaxExtent && nr <= kLatticeMaxExtent)
        return NLOSGR_OK;
    snprintf(g_err, sizeof(g_err), "%s must be in 1..%d", what, kLatticeMaxExtent);
    return NLOSGR_E_INVALID;
}

// finite and > 0, in the argument's own precision
template <class T>
inline bool lattice_positive(T v) { return v > (T)0 && v <= (T)3.0e38; }

// the window of the rows: the bin width and the radius of bin 0
template <class T>
inline int lattice_check_window(float r0, T dr) {
    if (!lattice_positive(dr)) return set_err(NLOSGR_E_INVALID, "dr must be finite and > 0");
    if (!(r0 >= 0.0f && r0 <= 3.0e38f)) return set_err(NLOSGR_E_INVALID, "r0 must be finite and >= 0");
    return NLOSGR_OK;
}

inline int lattice_check_strides(int32_t H, int32_t W, int32_t stride_m, int32_t stride_n) {
    if (stride_m < 0 || stride_n < 0 ||
        (long long)(H - 1) * stride_m + (long long)(W - 1) * stride_n >= (long long)H * W)
        return set_err(NLOSGR_E_INVALID, "lattice strides must keep m stride_m + n stride_n inside [0, H W)");
    return NLOSGR_OK;
}

}  // namespace detail
}  // namespace nlosgr
