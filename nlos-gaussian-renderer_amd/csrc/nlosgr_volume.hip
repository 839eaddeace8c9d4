// Transient Gaussian NLOS renderer — the pair-major volume path's host side and the C ABI (gfx950):
// validation, the split heuristics, the workspace layout (VolumeWs), the forward's set-up and the
// extern "C" entry points.  The kernels live in nlosgr_volume_fwd.hip and nlosgr_volume_bwd.hip; what they
// share, with the algebra of the hot path, is in nlosgr_volume.hpp.
#include "nlosgr_volume.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

// 3-sigma AABB: bbox_compute.cuh:23-71 (cuda) / gaussian_model.py:140-178 (torch; clamp 1e-8)
template <int PRESET>
__global__ __launch_bounds__(kBlock) void bbox_kernel(nlosgr_gaussians g, float sig, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.ng) return;
    gauss_bbox<PRESET>(g, i, sig, out + 6 * (size_t)i);
}

// shared-row backward layout when per-wave rows would leave fewer than 4 workgroups per CU
// (long rows, e.g. C5's 2048 bins); NLOSGR_FLAG_BWD_SHARED / _PERWAVE force either layout (A/B timing)
bool bwd_shared(const nlosgr_geometry* geo, const nlosgr_options* opt) {
    if (opt->flags & NLOSGR_FLAG_BWD_SHARED) return true;
    if (opt->flags & NLOSGR_FLAG_BWD_PERWAVE) return false;
    return (size_t)BwdLayout(geo->nr, geo->nt, geo->np).total * 4 > 40 * 1024;
}

int validate(const nlosgr_gaussians* g, const nlosgr_geometry* geo, const nlosgr_options* opt) {
    if (!g || !geo || !opt) return set_err(NLOSGR_E_INVALID, "null argument struct");
    if (g->ng < 0) return set_err(NLOSGR_E_INVALID, "ng must be >= 0");
    if (g->preset != NLOSGR_PRESET_TORCH && g->preset != NLOSGR_PRESET_CUDA)
        return set_err(NLOSGR_E_INVALID, "unknown preset");
    // SH degree 4 exists in the torch preset only (sh_utils.py:102-112; spherical_harmonics.cuh stops at 3)
    const int max_deg = g->preset == NLOSGR_PRESET_TORCH ? 4 : 3;
    if (g->sh_degree < 0 || g->sh_degree > max_deg)
        return set_err(NLOSGR_E_UNSUPPORTED, g->preset == NLOSGR_PRESET_TORCH ? "active_sh_degree must be in [0, 4]"
                                                                              : "active_sh_degree must be in [0, 3] (cuda preset)");
    const int max_k = g->preset == NLOSGR_PRESET_TORCH ? kMaxK4 : kMaxK;
    if (g->k_feat < (g->sh_degree + 1) * (g->sh_degree + 1) || g->k_feat > max_k)
        return set_err(NLOSGR_E_INVALID, g->preset == NLOSGR_PRESET_TORCH ? "k_feat must satisfy (sh_degree+1)^2 <= k_feat <= 25"
                                                                           : "k_feat must satisfy (sh_degree+1)^2 <= k_feat <= 16");
    if (opt->mode != NLOSGR_MODE_NOOCL && opt->mode != NLOSGR_MODE_NETF && opt->mode != NLOSGR_MODE_BININT &&
        opt->mode != NLOSGR_MODE_OCCL)
        return set_err(NLOSGR_E_INVALID, "unknown mode");
    if (geo->nwall < 0 || geo->nt < 1 || geo->np < 1 || geo->nr < 1)
        return set_err(NLOSGR_E_INVALID, "bad geometry sizes");
    if (geo->nr > 4096 || geo->nt > 1024 || geo->np > 1024)
        return set_err(NLOSGR_E_UNSUPPORTED, "nr <= 4096 and nt, np <= 1024");
    if (g->ng > 0 && (!g->mu || !g->scaling || !g->rotation || !g->opacity || !g->features))
        return set_err(NLOSGR_E_INVALID, "null Gaussian parameter pointer");
    if (geo->nwall > 0 && (!geo->wall || !geo->sin_theta || !geo->cos_theta || !geo->sin_phi ||
                           !geo->cos_phi || !geo->grid_lin || !geo->hscale || !geo->r || !geo->att))
        return set_err(NLOSGR_E_INVALID, "null geometry pointer");
    if (tiles_engine(opt)) return tiles_validate(g, geo, opt);
    const size_t lds_f = (size_t)FwdLayout(geo->nr, geo->nt, geo->np).total * 4;
    const size_t lds_b = (size_t)BwdLayout(geo->nr, geo->nt, geo->np, bwd_shared(geo, opt)).total * 4;
    if (lds_f > 160 * 1024 || lds_b > 160 * 1024) return set_err(NLOSGR_E_UNSUPPORTED, "problem exceeds LDS budget");
    return NLOSGR_OK;
}

int bwd_nsplit(const nlosgr_gaussians* g, const nlosgr_geometry* geo, const nlosgr_options* opt, bool shared) {
    const int maxs = geo->nwall > 0 ? geo->nwall : 1;
    if (opt->nsplit > 0) return opt->nsplit < maxs ? opt->nsplit : maxs;
    const int gpb = shared ? kNB * kWaves : kNB;
    const int nblk = (g->ng + gpb - 1) / gpb;
    // aim for ~48k workgroups: with 4 resident per CU a 3k-workgroup grid left a long last round
    // (C3 backward: 2 splits 354 ms, 16 -> 309, 32 -> 305, 64 -> 302)
    int ns = (49152 + nblk - 1) / (nblk > 0 ? nblk : 1);
    if (ns > maxs) ns = maxs;
    // per-wave layout: wave w walks wall points pbeg + w, + 4, ...; a split of fewer than 4 wall
    // points leaves waves idle while the workgroup still holds its LDS (small walls, e.g. C1's
    // 32x32: 1024 splits of one wall point ran one busy wave per workgroup)
    if (!shared && ns > maxs / kWaves) ns = maxs / kWaves;
    if (ns < 1) ns = 1;
    return ns;
}

// The backward runs over batches of wall points so that its dL/drho buffer ([batch][ng], read by
// sh_kernel) is bounded: NLOSGR_DRHO_MB (default 1024) MiB, i.e. C3 6.5 GB -> 1 GiB, a C5 rank 16.4 GB
// -> 1 GiB.  Split counts are sized for one batch; batches after the first add into the partial slabs.
int drho_batch(const nlosgr_gaussians* g, const nlosgr_geometry* geo) {
    const long long budget = (long long)(batch_budgets().drho_mb * 1048576.0);
    const long long per = (long long)(g->ng > 0 ? g->ng : 1) * (long long)sizeof(float);
    long long b = budget / per;
    if (b < 1) b = 1;
    if (b > geo->nwall) b = geo->nwall;
    return (int)(b > 0 ? b : 1);
}

// sh_kernel wall-point splits (>= 8 x 256-lane blocks per split row keep the chip busy at large Ng)
int sh_nsplit(const nlosgr_gaussians* g, const nlosgr_geometry* geo) {
    int ns = geo->nwall / 256;
    const int nblk = (g->ng + kBlock - 1) / kBlock;
    if (ns * nblk > 4096) ns = 4096 / (nblk > 0 ? nblk : 1);
    if (ns > 64) ns = 64;
    return ns < 1 ? 1 : ns;
}
// forward Gaussian splits per wall point: aim for 131072 workgroups (a 16k-workgroup grid of
// one long workgroup per wall point leaves a ragged last round), at least 256 Gaussians per split
#ifndef NLOSGR_FWD_SPLITS_MAX
#define NLOSGR_FWD_SPLITS_MAX 8        // forward Gaussian splits per wall point, at most
#endif
#ifndef NLOSGR_FWD_WG_TARGET
#define NLOSGR_FWD_WG_TARGET 131072    // forward workgroups aimed at (wall points x splits)
#endif
int fwd_nsplit(const nlosgr_gaussians* g, const nlosgr_geometry* geo) {
    if (geo->nwall <= 0) return 1;
    int ns = (NLOSGR_FWD_WG_TARGET + geo->nwall - 1) / geo->nwall;
    const int byg = (g->ng + 255) / 256;
    if (ns > byg) ns = byg;
    if (ns > NLOSGR_FWD_SPLITS_MAX) ns = NLOSGR_FWD_SPLITS_MAX;
    return ns < 1 ? 1 : ns;
}
// the fixed-point TAIL drain serves the culled no-occlusion histogram at cutoff >= kTailCutoff
// (NLOSGR_FLAG_FLOAT_DRAIN: the float claim drain instead, A/B)
bool fx_eligible(const nlosgr_options* opt, bool dense, bool rays, bool counts, bool hist, bool cache) {
    const bool mode_ok = opt->mode == NLOSGR_MODE_NOOCL || opt->mode == NLOSGR_MODE_BININT ||
                         (opt->mode == NLOSGR_MODE_NETF && opt->c_deltaT <= kSmallX);   // (the TAIL drains)
    return mode_ok && opt->cutoff >= kTailCutoff && !dense && !rays && !counts && hist && !cache &&
           !(opt->flags & (NLOSGR_FLAG_FLOAT_DRAIN | NLOSGR_FLAG_MASKED_FWD));
}
// The workspace of the pair-major path, in this order (every region starts 256-byte aligned; P = nwall):
//   recs     GaussRec [ng]
//   part     backward partials, float [nsplit_ws][ng][kPartStride]; nsplit_ws is the larger split count of the
//            two backward layouts, so nothing after it moves with the layout a later backward picks
//   cache    (opt->ray_cache) mask 2 x u64 [P][ng] | box u32 [P][ng] | rho float [P][ng], unaligned within
//   drho     dL/drho of one wall-point batch, float [batch][ng]
//   shpart   sh_kernel partials, float [nsh][ng][kShPart]
//   diag     the backward's diagnostics counters (kFlagDiagCounters), kDiagTailBytes
//   fpart    forward partials, float [nfsplit][P][nr] (nfsplit > 1), or the FX drain's u64 row [P][nr]
//   fxbins   FX tail (kFxTailBytes): bound histogram u32 [kFxBins], then fxinfo, int [kFxInfoWords]
//   fxbound  FX amplitude bounds, float [ng]
//   fxblist  FX bright list, int [ng]
// Built once from (g, geo, opt); everything that sizes or addresses the workspace reads it from here.
struct VolumeWs {
    int batch;           // wall points per backward batch (drho_batch)
    int nsplit_bwd[2];   // backward wall-point splits of one batch: per-wave layout, shared layout
    int nsplit_ws;
    int nsh;             // sh_kernel wall-point splits of one batch
    int nfsplit;         // forward Gaussian splits per wall point
    bool cache;          // the ray cache exists and is not empty
    size_t off_part, off_cmask, off_cbox, off_crho, off_drho, off_shpart, off_diag, off_fpart, off_fxbins, off_fxinfo,
        off_fxbound, off_fxblist, total;   // (recs at 0)

    VolumeWs(const nlosgr_gaussians* g, const nlosgr_geometry* geo, const nlosgr_options* opt) {
        const size_t ng = (size_t)g->ng, P = (size_t)geo->nwall;
        nlosgr_geometry gb = *geo;
        gb.nwall = batch = drho_batch(g, geo);
        nsplit_bwd[0] = bwd_nsplit(g, &gb, opt, false);
        nsplit_bwd[1] = bwd_nsplit(g, &gb, opt, true);
        nsplit_ws = nsplit_bwd[0] > nsplit_bwd[1] ? nsplit_bwd[0] : nsplit_bwd[1];
        nsh = sh_nsplit(g, &gb);
        nfsplit = fwd_nsplit(g, geo);
        cache = opt->ray_cache && ng > 0 && P > 0;
        off_part = align_up(ng * sizeof(GaussRec));
        off_cmask = off_part + align_up((size_t)nsplit_ws * ng * kPartStride * sizeof(float));
        off_cbox = off_cmask + P * ng * kCacheMaskBytes;
        off_crho = off_cbox + P * ng * kCacheBoxBytes;
        off_drho = off_cmask +
                   (opt->ray_cache ? align_up(P * ng * (kCacheMaskBytes + kCacheBoxBytes + kCacheRhoBytes)) : 0);
        off_shpart = off_drho + align_up((size_t)batch * ng * sizeof(float));
        off_diag = off_shpart + align_up((size_t)nsh * ng * kShPart * sizeof(float));
        off_fpart = off_diag + kDiagTailBytes;
        const size_t fl = nfsplit > 1 ? (size_t)nfsplit * P * geo->nr * sizeof(float) : 0;
        const size_t fx = P * geo->nr * sizeof(unsigned long long);
        off_fxbins = off_fpart + align_up(fl > fx ? fl : fx);
        off_fxinfo = off_fxbins + kFxBins * sizeof(unsigned);
        off_fxbound = off_fxbins + kFxTailBytes;
        off_fxblist = off_fxbound + align_up(ng * sizeof(float));
        total = off_fxblist + align_up(ng * sizeof(float));
    }
    template <class T>
    static T* at(const void* ws, size_t off) { return (T*)((char*)ws + off); }
    void cache_ptrs(void* ws, KArgs& ka) const {
        if (!cache) return;
        ka.cmask = at<ulonglong2>(ws, off_cmask);
        ka.cbox = at<unsigned>(ws, off_cbox);
        ka.crho = at<float>(ws, off_crho);
    }
};
static_assert(kFxBins * sizeof(unsigned) + kFxInfoWords * sizeof(int) <= kFxTailBytes, "the FX tail holds bins and info");

int run_fwd(const nlosgr_gaussians* g, const nlosgr_geometry* geo, const nlosgr_options* opt, void* workspace,
            float* hist_out, float* ray_out, unsigned long long* counts, hipStream_t s) {
    if (g->ng > 0 && !workspace) return set_err(NLOSGR_E_INVALID, "workspace is null");
    KArgs ka;
    memset(&ka, 0, sizeof(ka));
    ka.g = *g; ka.geo = *geo; ka.opt = *opt;
    ka.recs = (const GaussRec*)workspace;
    ka.hist_out = hist_out; ka.ray_out = ray_out;
    ka.counts = counts;
    const VolumeWs W(g, geo, opt);
    if (!counts) W.cache_ptrs(workspace, ka);
    const bool dense = !(opt->cutoff > 0.f);
    const bool rays = ray_out != nullptr;
    const bool fx = g->ng > 0 && fx_eligible(opt, dense, rays, counts != nullptr, hist_out != nullptr, ka.cmask != nullptr);
    if (fx) {
        ka.hfx = W.at<unsigned long long>(workspace, W.off_fpart);
        ka.fx_info = W.at<int>(workspace, W.off_fxinfo);
        ka.fx_bound = W.at<float>(workspace, W.off_fxbound);
        ka.fx_blist = W.at<int>(workspace, W.off_fxblist);
        ka.nfsplit = W.nfsplit;
        const int rc = volume_fx_prepare(ka, W.at<unsigned>(workspace, W.off_fxbins), W.at<float>(workspace, W.off_fxbound),
                                         W.at<int>(workspace, W.off_fxblist), s);
        if (rc) return rc;
    } else if (hist_out && W.nfsplit > 1 && g->ng > 0) {
        ka.hpart = W.at<float>(workspace, W.off_fpart);
        ka.nfsplit = W.nfsplit;
    }
    // a forward that does not take the FX drain leaves nlosgr_fx_info all zeros, not an earlier forward's words
    // (the FX tail lies past the float partials)
    if (!fx && g->ng > 0)
        HIPCHK(hipMemsetAsync(W.at<int>(workspace, W.off_fxinfo), 0, kFxInfoWords * sizeof(int), s));
    if (g->ng > 0) {
        // (FX: the bright Gaussians get a negative sigma in the records, see preprocess_kernel)
        launch_preprocess(g, (GaussRec*)workspace, s, ka.hfx ? ka.fx_bound : nullptr, ka.fx_info);
        HIPCHK(hipGetLastError());
    }
    return volume_fwd(ka, s);
}

}  // namespace

extern "C" {

int nlosgr_abi_version(void) { return NLOSGR_ABI_VERSION; }

void nlosgr_set_batch_budgets(double drho_mb, double tile_hpart_mb) {
    BatchBudgets& b = batch_budgets();
    if (drho_mb > 0.0) b.drho_mb = drho_mb;
    if (tile_hpart_mb > 0.0) b.tile_hpart_mb = tile_hpart_mb;
}

void nlosgr_get_batch_budgets(double* drho_mb, double* tile_hpart_mb) {
    const BatchBudgets& b = batch_budgets();
    if (drho_mb) *drho_mb = b.drho_mb;
    if (tile_hpart_mb) *tile_hpart_mb = b.tile_hpart_mb;
}

const char* nlosgr_last_error(void) { return g_err; }

size_t nlosgr_workspace_bytes(const nlosgr_gaussians* g, const nlosgr_geometry* geo, const nlosgr_options* opt) {
    if (validate(g, geo, opt) != NLOSGR_OK) return 0;
    if (tiles_engine(opt)) return tiles_workspace_bytes(g, geo, opt);
    return VolumeWs(g, geo, opt).total;
}

int nlosgr_render_fwd(const nlosgr_gaussians* g, const nlosgr_geometry* geo, const nlosgr_options* opt,
                      void* workspace, float* hist_out, float* ray_out, void* hip_stream) {
    const int rc = validate(g, geo, opt);
    if (rc) return rc;
    if (geo->nwall == 0 || (!hist_out && !ray_out)) return NLOSGR_OK;
    if (tiles_engine(opt)) return tiles_fwd(g, geo, opt, workspace, hist_out, ray_out, (hipStream_t)hip_stream);
    return run_fwd(g, geo, opt, workspace, hist_out, ray_out, nullptr, (hipStream_t)hip_stream);
}

int nlosgr_fx_info(const nlosgr_gaussians* g, const nlosgr_geometry* geo, const nlosgr_options* opt,
                   const void* workspace, int32_t* info_out, void* hip_stream) {
    const int rc = validate(g, geo, opt);
    if (rc) return rc;
    if (!workspace || !info_out) return set_err(NLOSGR_E_INVALID, "null workspace or info_out");
    if (tiles_engine(opt) || g->ng == 0) return set_err(NLOSGR_E_UNSUPPORTED, "fx_info: pair-major forward with ng > 0");
    const VolumeWs W(g, geo, opt);
    HIPCHK(hipMemcpyAsync(info_out, W.at<int>(workspace, W.off_fxinfo), kFxInfoWords * sizeof(int32_t),
                          hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
    return NLOSGR_OK;
}

int nlosgr_count_support(const nlosgr_gaussians* g, const nlosgr_geometry* geo, const nlosgr_options* opt,
                         void* workspace, unsigned long long* counts, void* hip_stream) {
    const int rc = validate(g, geo, opt);
    if (rc) return rc;
    if (!counts) return set_err(NLOSGR_E_INVALID, "counts is null");
    if (tiles_engine(opt)) return set_err(NLOSGR_E_UNSUPPORTED, "count_support: pair-major modes only");
    hipStream_t s = (hipStream_t)hip_stream;
    HIPCHK(hipMemsetAsync(counts, 0, 3 * sizeof(unsigned long long), s));
    if (geo->nwall == 0) return NLOSGR_OK;
    return run_fwd(g, geo, opt, workspace, nullptr, nullptr, counts, s);
}

int nlosgr_render_bwd(const nlosgr_gaussians* g, const nlosgr_geometry* geo, const nlosgr_options* opt,
                      void* workspace, const float* grad_hist, const float* grad_ray, float* d_mu,
                      float* d_scaling, float* d_rotation, float* d_opacity, float* d_features,
                      void* hip_stream) {
    int rc = validate(g, geo, opt);
    if (rc) return rc;
    if (opt->mode == NLOSGR_MODE_BININT)
        return set_err(NLOSGR_E_UNSUPPORTED, "no backward for the bin-integrated (analytic) forward");
    if (g->ng == 0) return NLOSGR_OK;
    if (!workspace) return set_err(NLOSGR_E_INVALID, "workspace is null");
    if (!d_mu || !d_scaling || !d_rotation || !d_opacity || !d_features)
        return set_err(NLOSGR_E_INVALID, "null gradient output pointer");
    if (opt->g_end > 0 && (opt->g_begin < 0 || opt->g_begin >= opt->g_end || opt->g_end > g->ng ||
                           opt->g_begin % 256 != 0 || tiles_engine(opt)))
        return set_err(NLOSGR_E_INVALID, "backward Gaussian range: 0 <= g_begin < g_end <= ng, g_begin % 256 == 0 "
                                         "(pair-major modes)");
    if (tiles_engine(opt))
        return tiles_bwd(g, geo, opt, workspace, grad_hist, grad_ray, d_mu, d_scaling, d_rotation, d_opacity,
                         d_features, (hipStream_t)hip_stream);
    hipStream_t s = (hipStream_t)hip_stream;
    KArgs ka;
    memset(&ka, 0, sizeof(ka));
    ka.g = *g; ka.geo = *geo; ka.opt = *opt;
    ka.recs = (const GaussRec*)workspace;
    const VolumeWs W(g, geo, opt);
    ka.partial = W.at<float>(workspace, W.off_part);
    ka.grad_hist = grad_hist; ka.grad_ray = grad_ray;
    ka.g_lo = opt->g_end > 0 ? opt->g_begin : 0;
    ka.g_hi = opt->g_end > 0 ? opt->g_end : g->ng;
    ka.bshared = bwd_shared(geo, opt) ? 1 : 0;
    ka.nsplit = W.nsplit_bwd[ka.bshared];
    W.cache_ptrs(workspace, ka);
    ka.drho = W.at<float>(workspace, W.off_drho);   // one batch
    ka.shpart = W.at<float>(workspace, W.off_shpart);
    ka.nsh = W.nsh;
    if (opt->flags & kFlagDiagCounters) {
        ka.counts = W.at<unsigned long long>(workspace, W.off_diag);
        HIPCHK(hipMemsetAsync(ka.counts, 0, 8 * sizeof(unsigned long long), s));
    }
    launch_preprocess(g, (GaussRec*)workspace, s);
    HIPCHK(hipGetLastError());
    if (geo->nwall > 0 && (grad_hist || grad_ray)) {
        for (int pb0 = 0; pb0 < geo->nwall; pb0 += W.batch) {   // wall-point batches (drho_batch)
            ka.pb0 = pb0;
            ka.pnw = geo->nwall - pb0 < W.batch ? geo->nwall - pb0 : W.batch;
            ka.accum = pb0 > 0 ? 1 : 0;
            rc = volume_bwd_batch(ka, s);
            if (rc) return rc;
        }
    } else {
        HIPCHK(hipMemsetAsync(ka.partial, 0, (size_t)ka.nsplit * g->ng * kPartStride * sizeof(float), s));
        ka.nsh = 0;
    }
    return volume_bwd_finish(ka, d_mu, d_scaling, d_rotation, d_opacity, d_features, s);
}

int nlosgr_bboxes(const nlosgr_gaussians* g, float sigma_scale, float* bboxes_out, void* hip_stream) {
    if (!g || !bboxes_out) return set_err(NLOSGR_E_INVALID, "null argument");
    if (g->ng <= 0) return NLOSGR_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    const int nb = (g->ng + kBlock - 1) / kBlock;
    if (g->preset == NLOSGR_PRESET_TORCH)
        hipLaunchKernelGGL(bbox_kernel<NLOSGR_PRESET_TORCH>, dim3(nb), dim3(kBlock), 0, s, *g, sigma_scale, bboxes_out);
    else
        hipLaunchKernelGGL(bbox_kernel<NLOSGR_PRESET_CUDA>, dim3(nb), dim3(kBlock), 0, s, *g, sigma_scale, bboxes_out);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

}  // extern "C"
