// What the voxelizer (nlosgr_voxel.hip) and its backward (nlosgr_voxel_bwd.hip) share: the per-Gaussian
// record of the voxel engine with its cutoff box, the kernel that fills it, and the host validation.
// The backward's support is the forward's by construction: the same box, the same VoxAux.
#pragma once
#include "nlosgr_common.hpp"

namespace nlosgr {
namespace detail {

constexpr int kVoxMaxExtent = 1024;
constexpr uint32_t kEmptyBox = 0x0000FFFFu;   // lo = 0xFFFF, hi = 0: overlaps nothing

// per-Gaussian record of the voxel engine: w = sigma rho(cam) and the cutoff box, (lo | hi << 16) per axis
struct __align__(16) VoxAux {
    float w;
    uint32_t bx, by, bz;
};

// inclusive voxel index range of [c - e, c + e] on a uniform ascending table, widened by one voxel
__device__ __forceinline__ uint32_t index_range(float c, float e, const float* tab, int n) {
    float lo = 0.f, hi = 0.f;
    if (n > 1) {
        const float x0 = tab[0];
        const float inv = (float)(n - 1) / (tab[n - 1] - x0);
        lo = floorf((c - e - x0) * inv) - 1.0f;
        hi = ceilf((c + e - x0) * inv) + 1.0f;
    } else {
        lo = (c - e) * 0.f;   // one voxel: any finite box may reach it; non-finite stays non-finite
        hi = (c + e) * 0.f;
    }
    if (!(fabsf(lo) <= 3.0e38f) || !(fabsf(hi) <= 3.0e38f)) return kEmptyBox;   // NaN / inf: skipped
    lo = fmaxf(lo, 0.0f);
    hi = fminf(hi, (float)(n - 1));
    if (lo > hi) return kEmptyBox;
    return (uint32_t)(int)lo | ((uint32_t)(int)hi << 16);
}

template <int PRESET>
__global__ __launch_bounds__(kBlock) void voxel_aux_kernel(nlosgr_gaussians g, const GaussRec* __restrict__ recs,
                                                          const float* __restrict__ cam, nlosgr_voxel_grid grid,
                                                          float cutoff, VoxAux* __restrict__ aux) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.ng) return;
    const float4 a = recs[i].a;
    float dx, dy, dz, nrm;
    view_dir<PRESET>(a.x - cam[0], a.y - cam[1], a.z - cam[2], dx, dy, dz, nrm);
    const float sh = sh_dot<PRESET>(g.sh_degree, dx, dy, dz, g.features + (size_t)i * g.k_feat);
    VoxAux o;
    o.w = a.w * fmaxf(sh + 0.5f, 0.0f);
    o.bx = o.by = o.bz = kEmptyBox;
    if (cutoff > 0.0f) {
        GaussAct act;
        activate<PRESET>(g.scaling + 3 * i, g.rotation + 4 * i, g.opacity[i], g.scaling_modifier, act);
        float e[3];
        for (int c = 0; c < 3; ++c) {
            float v = 0.f;
            for (int r = 0; r < 3; ++r) v += (act.Rp[3 * r + c] * act.st[r]) * (act.Rp[3 * r + c] * act.st[r]);
            e[c] = cutoff * 1.0001f * sqrtf(v) + 1e-7f;
        }
        o.bx = index_range(a.x, e[0], grid.xs, grid.nx);
        o.by = index_range(a.y, e[1], grid.ys, grid.ny);
        o.bz = index_range(a.z, e[2], grid.zs, grid.nz);
        if (o.bx == kEmptyBox || o.by == kEmptyBox || o.bz == kEmptyBox) o.bx = o.by = o.bz = kEmptyBox;
    }
    aux[i] = o;
}

inline void launch_voxel_aux(const nlosgr_gaussians* g, const GaussRec* recs, const float* cam,
                             const nlosgr_voxel_grid* grid, float cutoff, VoxAux* aux, hipStream_t s) {
    const int nbg = (g->ng + kBlock - 1) / kBlock;
    if (g->preset == NLOSGR_PRESET_TORCH)
        hipLaunchKernelGGL(voxel_aux_kernel<NLOSGR_PRESET_TORCH>, dim3(nbg), dim3(kBlock), 0, s, *g, recs, cam, *grid,
                           cutoff, aux);
    else
        hipLaunchKernelGGL(voxel_aux_kernel<NLOSGR_PRESET_CUDA>, dim3(nbg), dim3(kBlock), 0, s, *g, recs, cam, *grid,
                           cutoff, aux);
}

inline int validate_voxel(const nlosgr_gaussians* g, const nlosgr_voxel_grid* grid, const nlosgr_options* opt) {
    if (!g || !grid || !opt) return set_err(NLOSGR_E_INVALID, "null argument struct");
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
    if (opt->mode != 0 || opt->selection != 0 || opt->ray_cache != 0)
        return set_err(NLOSGR_E_INVALID, "voxelize uses opt->cutoff only: mode, selection and ray_cache must be 0");
    if (grid->nx < 1 || grid->ny < 1 || grid->nz < 1 || grid->nx > kVoxMaxExtent || grid->ny > kVoxMaxExtent ||
        grid->nz > kVoxMaxExtent)
        return set_err(NLOSGR_E_INVALID, "voxel grid extents must be in 1..1024");
    if ((long long)grid->nx * grid->ny * grid->nz >= (1ll << 31))
        return set_err(NLOSGR_E_INVALID, "voxel grid must hold fewer than 2^31 voxels");
    if (!grid->xs || !grid->ys || !grid->zs) return set_err(NLOSGR_E_INVALID, "null voxel grid table");
    if (g->ng > 0 && (!g->mu || !g->scaling || !g->rotation || !g->opacity || !g->features))
        return set_err(NLOSGR_E_INVALID, "null Gaussian parameter pointer");
    return NLOSGR_OK;
}

}  // namespace detail
}  // namespace nlosgr
