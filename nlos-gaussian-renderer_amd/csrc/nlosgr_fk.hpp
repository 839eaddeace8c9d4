// The falloff-compensated bin of a confocal row, shared by the load passes of f-k migration (nlosgr_fk.hip) and of
// the light-cone transform (nlosgr_lct.hip), so both weight a capture with the same fp32 arithmetic.
#pragma once
#include "nlosgr_common.hpp"

namespace nlosgr {
namespace detail {

// max(h, 0) (r0 + j dr)^POWER, its square root when AMP: r = fma(j, dr, r0), the power as r, r r, (r r) r,
// (r r)(r r), the hardware square root (1 ulp)
template <int POWER, bool AMP>
__device__ __forceinline__ float fk_psi(float h, int j, float r0, float dr) {
#pragma clang fp contract(off)
    const float r = fmaf((float)j, dr, r0);
    const float r2 = r * r;
    const float w = POWER == 0 ? 1.0f : (POWER == 1 ? r : (POWER == 2 ? r2 : (POWER == 3 ? r2 * r : r2 * r2)));
    const float v = fmaxf(h, 0.0f) * w;
    return AMP ? fsqrt(v) : v;
}

}  // namespace detail
}  // namespace nlosgr
