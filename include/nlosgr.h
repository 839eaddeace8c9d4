/*
 * nlosgr.h — C ABI of the MI355X-native transient Gaussian NLOS renderer.
 *
 * Plain pointers and sizes only (no torch types).  Every device pointer is a gfx950 HBM
 * address owned by the caller; the library never allocates device memory: callers size the
 * scratch with nlosgr_workspace_bytes() and pass it in.  All work is enqueued on the given
 * HIP stream; no call synchronises the device.  Return value 0 = success, otherwise a
 * NLOSGR_E_* code with a message in nlosgr_last_error() (thread-local).
 *
 * Reference interfaces these entry points replace (paths under the reference repo):
 *   nlosgr_render_fwd   <- _C.render_rays            submodules/cuda_renderer/include/volume_renderer.h:8-24,
 *                                                    src/volume_renderer.cu:189-305
 *                       <- GaussianModel.estimate_rho_w_no_occlusion / estimate_rho_w('netf')
 *                          + gaussian_transient_rendering (the dense torch path that actually runs):
 *                          gaussian_model/gaussian_model.py:297-364, nlos_helpers.py:192-232
 *   nlosgr_render_bwd   <- CUDARenderFunction.backward gaussian_model/cuda_autograd.py:110-191
 *                          (zeros in the reference; real gradients here) and torch autograd of path T
 *   nlosgr_rays_analytic <- _C.render_rays_analytic  src/volume_renderer_analytic.cu:178-241
 *   nlosgr_mse / nlosgr_adam <- compute_loss nlos_helpers.py:323-327 + model.optimizer.step()
 *                          main.py:203-213 (torch.optim.Adam groups, gaussian_model.py:223-242)
 *   nlosgr_irf_apply / nlosgr_mse_irf: no counterpart (the reference trains on synthetic transients only);
 *                          the detector's temporal response between the render and a measured capture
 *   nlosgr_loss_irf     no counterpart: the same fused loss with a kind, the MSE or the Poisson deviance of
 *                          photon counts
 *   nlosgr_bboxes       <- compute_gaussian_bboxes_kernel include/bbox_compute.cuh:76-120,
 *                          GaussianModel.get_bboxes gaussian_model/gaussian_model.py:140-178
 *   nlosgr_carve_votes  <- the voting loop of space_carving gaussian_model/gaussian_utils.py:88-99
 *   nlosgr_voxelize     <- evaluation() -> gaussian2volume main.py:374-387, nlos_helpers.py:40-69, with the
 *                          two sums of estimate_rho_w_no_occlusion(out_separately=True)
 *                          gaussian_model/gaussian_model.py:346-364 on a regular voxel grid
 *   nlosgr_mesh_*       <- gaussian2volume(mode='mesh') nlos_helpers.py:50-69: the surface of the density at
 *                          its mean (:51), as an isosurface (marching tetrahedra) in place of the open3d
 *                          Poisson reconstruction
 *   nlosgr_backproject  no counterpart (the reference has no reconstruction from the capture itself): the
 *                          back-projection of the measured histograms onto the voxel grid, the baseline
 *                          reconstruction and a data-driven initial density
 *   nlosgr_forward_project  no counterpart: the adjoint of the back-projection, voxel grid -> transients
 *                          (checks a volume against the capture; the least-squares volume)
 *   nlosgr_*_nc         no counterpart: the two voxel operators for a non-confocal capture (laser spot and
 *                          sensed spot differ)
 *   nlosgr_backproject_phasor  no counterpart: phasor-field reconstruction, the back-projection of complex rows
 *                          (the capture filtered with a Morlet wavelet) in one pass, and its magnitude
 *   nlosgr_render_nc_*  no counterpart: the Gaussian renderer of such a capture, forward and backward (the
 *                          no-occlusion histogram; nlosgr_render_fwd / _bwd stay confocal)
 *   nlosgr_sgld_noise   no counterpart (main.py:163-164, 215-217 leave it as future work): the position noise of
 *                          3DGS-MCMC's SGLD sampler after an optimizer step, from a counter-based generator
 *   nlosgr_fk_*         no counterpart: f-k migration of a confocal capture, the three passes around its two FFTs
 *   nlosgr_rsd_*        no counterpart: fast phasor-field reconstruction (Rayleigh-Sommerfeld diffraction by FFT on the
 *                          wall's lattice), the four passes around its FFTs; confocal or one laser spot
 *   nlosgr_lct_*        no counterpart: the light-cone transform of a confocal capture (Wiener-filtered inversion of the
 *                          confocal measurement operator), the four passes around its FFTs
 */
#ifndef NLOSGR_H
#define NLOSGR_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__) || defined(__clang__)
#define NLOSGR_API __attribute__((visibility("default")))
#else
#define NLOSGR_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define NLOSGR_ABI_VERSION 13

/* convention presets */
enum {
    NLOSGR_PRESET_TORCH = 0, /* path T: s=exp(exp(S)*mod), u=R(x-mu), 3DGS SH signs, no eps */
    NLOSGR_PRESET_CUDA = 1   /* path C: s=exp(S)*mod, u=R^T(x-mu)/(s+1e-8), unsigned SH, eps'd normalise */
};

/* per-sample density model */
enum {
    NLOSGR_MODE_NOOCL = 0, /* rho_d = sum_g sigma pdf rho                  (gaussian_model.py:346-364) */
    NLOSGR_MODE_NETF = 1,  /* per-Gaussian self-transmittance cumprod       (gaussian_model.py:313-324) */
    NLOSGR_MODE_BININT = 2, /* no-occlusion with each sample replaced by the exact average of the pdf
                              over its radial bin [r_k -+ dr/2] (closed-form erf; forward only) — the
                              corrected counterpart of the analytic section path */
    NLOSGR_MODE_OCCL = 3   /* path C use_occlusion=True (volume_renderer.cu:80-137), cuda preset only:
                              per ray, T_k = exp(-c dT sum_{k'<k} D_k'), D = sum_g sigma pdf,
                              rho_d = T_k sum_g (1 - exp(-sigma pdf c dT)) rho, zero where T_k < 1e-4 */
};

/* which Gaussians each ray sums over (nlosgr_options.selection) */
enum {
    NLOSGR_SELECT_SUPPORT = 0, /* every Gaussian, samples within the Mahalanobis cutoff (dense if <= 0) */
    NLOSGR_SELECT_AABB = 1     /* path C's filter (ray_aabb.cu:10-61, volume_renderer.cu:220-245): the first
                                  256 Gaussians by index whose 3-sigma box (bbox_compute.cuh) the ray hits,
                                  each evaluated along the whole ray; cuda preset only */
};

enum {
    NLOSGR_OK = 0,
    NLOSGR_E_INVALID = 1, /* bad argument / shape */
    NLOSGR_E_HIP = 2,     /* HIP launch error */
    NLOSGR_E_UNSUPPORTED = 3
};

/* Gaussians: raw (pre-activation) parameters, exactly the reference GaussianModel tensors. */
typedef struct {
    int32_t ng;               /* number of Gaussians */
    int32_t k_feat;           /* feature row stride K >= (sh_degree+1)^2; K <= 25 (torch preset) / 16 (cuda) */
    int32_t sh_degree;        /* active SH degree: 0..4 torch preset (sh_utils.py:57-112), 0..3 cuda preset */
    int32_t preset;           /* NLOSGR_PRESET_* */
    float scaling_modifier;   /* `mod` */
    const float* mu;          /* [ng,3]  _mu                                         */
    const float* scaling;     /* [ng,3]  _scaling (raw)                              */
    const float* rotation;    /* [ng,4]  _rotation (raw quaternion w,x,y,z)          */
    const float* opacity;     /* [ng]    _opacity (raw logit)                        */
    const float* features;    /* [ng,k_feat] cat(_features_dc,_features_rest) flattened */
} nlosgr_gaussians;

/* Batched spherical sampling geometry: one (theta, phi, r) grid per relay-wall point, i.e. the
 * reference's spherical_sample_histogram (nlos_helpers.py:124-188) for P wall points at once.
 * Sample (p, k, i, j) sits at x = wall[p] + r[k] * (st_i cp_j, st_i sp_j, ct_i). */
typedef struct {
    int32_t nwall;            /* P */
    int32_t nt;               /* theta samples (Ns in the reference) */
    int32_t np;               /* phi samples (Ns in the reference) */
    int32_t nr;               /* radial samples = time bins T */
    const float* wall;        /* [P,3] wall points */
    const float* sin_theta;   /* [P,nt] */
    const float* cos_theta;   /* [P,nt] */
    const float* sin_phi;     /* [P,np] */
    const float* cos_phi;     /* [P,np] */
    const float* grid_lin;    /* [P,4] (theta_min, theta_step, phi_min, phi_step) of the linspace grids */
    const float* hscale;      /* [P] histogram weight per wall point (dtheta*dphi*Y^2[*c*dT]) */
    const float* r;           /* [nr] sample radii (linspace, shared by all wall points) */
    const float* att;         /* [nr] per-bin attenuation (1/dist^2 or 1/(t^2+1e-8)) */
} nlosgr_geometry;

typedef struct {
    int32_t mode;             /* NLOSGR_MODE_* */
    float cutoff;             /* Mahalanobis support radius m_c; <= 0 -> dense (no culling) */
    float c_deltaT;           /* c * deltaT (netf transmittance) */
    float ray_scale;          /* scale applied to the optional per-ray output (e.g. c*dT) */
    int32_t nsplit;           /* backward: wall-point splits (0 -> auto) */
    int32_t flags;            /* 0 in production.  Bits 0-6: phase-ablation diagnostics (wrong results on
                                 purpose); NLOSGR_FLAG_* below: variant selection for A/B timing and parity
                                 cross-checks (ABI 8: these used to be environment variables, so the
                                 library's numerics no longer depend on the caller's environment) */
    int32_t ray_cache;        /* 1: the forward records, per (wall point, Gaussian) pair, which rays
                                 of its candidate box are in support (20 B per pair in the workspace,
                                 see nlosgr_workspace_bytes) and a backward on the SAME workspace with
                                 the SAME inputs walks that record instead of re-testing the rays.
                                 Culled (cutoff > 0), histogram-only calls.  In NLOSGR_MODE_OCCL it is
                                 the row cache instead: the forward stores every ray tile's (D, W) rows
                                 (8 B per wall point x ray x bin; C3 128 GiB) and the backward on the
                                 same workspace reloads them instead of re-running its forward sweep
                                 (and, when the forward was one wall-point launch, its tile bins).
                                 0 = off */
    int32_t selection;        /* NLOSGR_SELECT_*.  OCCL mode and AABB selection run the ray-tile engine
                                 (ray-major, per-ray compositing, deterministic); the ray cache and
                                 nlosgr_count_support do not apply there */
    int32_t g_begin, g_end;   /* backward only: gradients of Gaussians [g_begin, g_end) (g_begin % 256 == 0;
                                 rows outside are left untouched), so a caller can all-reduce one
                                 bucket while the next one is differentiated; g_end = 0 -> all */
} nlosgr_options;

/* nlosgr_options.flags: variant selection (each variant is a correct renderer of the same quantity;
 * they differ in summation order / rounding and speed) */
#define NLOSGR_FLAG_FLOAT_DRAIN  0x100  /* forward: fp32 claim drain instead of the fixed-point (FX) drain */
#define NLOSGR_FLAG_MASKED_FWD   0x200  /* forward: masked (end-of-segment) drains at every cutoff, no TAIL */
#define NLOSGR_FLAG_MASKED_BWD   0x400  /* backward: masked drains at every cutoff, no TAIL */
#define NLOSGR_FLAG_LANE_DENSE   0x800  /* dense no-occlusion histogram through the lane-serial drain
                                           instead of the register (lane = bin) kernel */
#define NLOSGR_FLAG_BWD_SHARED   0x1000 /* backward: shared-row layout (4 waves per staged row) */
#define NLOSGR_FLAG_BWD_PERWAVE  0x2000 /* backward: per-wave row layout (default picks by LDS size) */
#define NLOSGR_FLAG_TILE_NOBIN   0x8000 /* ray-tile engine: cull every Gaussian against every item's cone in the
                                           kernel instead of reading the tile bins (A/B: same selections) */
#define NLOSGR_FLAG_FX_MAXUNIT   0x4000 /* forward FX drain: unit from the largest amplitude bound (the round-5
                                           rule, diagnostics: shows the precision the quantile unit recovers) */
#define NLOSGR_FLAG_FX_NOTWIN    0x10000 /* forward no-occlusion FX drain: one ray per lane (the single-segment
                                            drain) instead of two adjacent rays of a pair per lane (A/B, tests) */
#define NLOSGR_FLAG_FX_TWIN_STATS 0x20000 /* forward twin drain: also record the longest twin (bins) in
                                             nlosgr_fx_info (one global atomic per twin: diagnostics, slow) */
#define NLOSGR_FLAG_FX_TRIM      0x40000 /* forward no-occlusion FX drain: each (wall point, Gaussian) pair's support
                                            ends where its value falls under a quarter of the drain's unit 2^-E,
                                            when that is inside the cutoff; a pair that peaks below a quarter unit is
                                            skipped.  Such terms round to zero units in that drain anyway, so the
                                            histogram keeps its per-term rounding bound; rays are paired differently,
                                            so it is not bitwise the untrimmed one.  Other forwards and the backward
                                            ignore it */

/* Scratch bytes needed by fwd/bwd for this problem (caller allocates, 256-B aligned); includes
 * nwall*ng*24 B for the ray cache when opt->ray_cache is set (OCCL mode: the row cache,
 * nwall * tiles * tile rays * nr * 8 B). */
NLOSGR_API size_t nlosgr_workspace_bytes(const nlosgr_gaussians* g, const nlosgr_geometry* geo,
                              const nlosgr_options* opt);

/* Batch budgets in MiB (values <= 0 keep the current one): the backward's dL/drho buffer, filled in
 * wall-point batches (default 1024), and the ray-tile forward's partial histograms (default 1024).
 * (ABI 8: no environment variables are read.)
 * They set the workspace layout: change them only while no workspace sized under the old values is
 * still in use (a ray-cache backward must run under the forward's budgets). */
NLOSGR_API void nlosgr_set_batch_budgets(double drho_mb, double tile_hpart_mb);
/* The batch budgets in effect (MiB): lets a caller restore exactly what it changed. */
NLOSGR_API void nlosgr_get_batch_budgets(double* drho_mb, double* tile_hpart_mb);

/* Forward.  hist_out [P,nr] (may be NULL):  hscale[p]*att[k]*sum_{g,i,j} w_g(p) sin(theta_i) pdf
 *           ray_out  [P,nt*np,nr] (may be NULL, caller zero-fills): ray_scale*sum_g w_g(p) pdf,
 *           rays in the reference's (i,j) meshgrid('ij') order, samples contiguous — the layout of
 *           _C.render_rays' rho_density [N_rays, N_samples].
 * w_g(p) = sigmoid(opacity_g) * max(0, 0.5 + SH_g(dir(mu_g - wall_p))). */
NLOSGR_API int nlosgr_render_fwd(const nlosgr_gaussians* g, const nlosgr_geometry* geo,
                      const nlosgr_options* opt, void* workspace, float* hist_out,
                      float* ray_out, void* hip_stream);

/* Backward.  grad_hist [P,nr] and/or grad_ray [P,nt*np,nr] (either may be NULL).
 * Writes (overwrites) the gradients of the RAW parameters: d_mu [ng,3], d_scaling [ng,3],
 * d_rotation [ng,4], d_opacity [ng], d_features [ng,k_feat]. */
NLOSGR_API int nlosgr_render_bwd(const nlosgr_gaussians* g, const nlosgr_geometry* geo,
                      const nlosgr_options* opt, void* workspace, const float* grad_hist,
                      const float* grad_ray, float* d_mu, float* d_scaling, float* d_rotation,
                      float* d_opacity, float* d_features, void* hip_stream);

/* Work count of one forward at opt->cutoff (no outputs written): counts (DEVICE, [3] uint64,
 * overwritten) = {in-support (wall point, Gaussian) pairs, in-support rays (pair, i, j),
 * in-support evaluations (pair, i, j, k)} — the unit of the VALU roofline. */
NLOSGR_API int nlosgr_count_support(const nlosgr_gaussians* g, const nlosgr_geometry* geo,
                         const nlosgr_options* opt, void* workspace, unsigned long long* counts,
                         void* hip_stream);

/* Fixed-point forward state after an nlosgr_render_fwd on `workspace` (same g / geo / opt): info_out
 * (DEVICE, [8] int32, overwritten, copied on the stream) = {E: the unit 2^-E of the fixed-point drain,
 * E of the launch's largest amplitude bound, LDS histogram flushes into the u64 row, bright segments
 * (peak >= 2^24 units, added straight into the u64 row), bright Gaussians, groups (two or more adjacent
 * rays of one row of a pair, drained by one lane as one segment; today a group holds two rays), groups split at
 * the merge guard (the rays the lane could not keep are drained as single segments), the longest group in bins
 * (NLOSGR_FLAG_FX_TWIN_STATS only)};
 * all zero when the forward did not take the fixed-point drain.  Diagnostics / tests.  (ABI 10: [8], was [4].) */
NLOSGR_API int nlosgr_fx_info(const nlosgr_gaussians* g, const nlosgr_geometry* geo, const nlosgr_options* opt,
                   const void* workspace, int32_t* info_out, void* hip_stream);

/* 3-sigma (sigma_scale) axis-aligned boxes [ng,6] = (min xyz, max xyz) under the preset's scale
 * convention (bbox_compute.cuh:23-71 for "cuda"; gaussian_model.py:140-178 for "torch"). */
NLOSGR_API int nlosgr_bboxes(const nlosgr_gaussians* g, float sigma_scale, float* bboxes_out, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Path C "rays" API: arbitrary rays x = o + t d (cuda_autograd.py:18-191 -> _C.render_rays,
 * volume_renderer.cu:189-305; _C.filter_gaussians_per_ray, ray_aabb.cu:63-102).
 * ------------------------------------------------------------------------------------- */
#define NLOSGR_MAX_PER_RAY 256   /* MAX_GAUSSIANS_PER_RAY, ray_aabb.cu:6 */

typedef struct nlosgr_rays {
    int32_t nrays;            /* N_rays */
    int32_t nsamp;            /* N_samples (<= 8192) */
    const float* origins;     /* [nrays,3] */
    const float* dirs;        /* [nrays,3], used as given: x = o + t d */
    const float* t;           /* [nsamp] */
    const float* cam;         /* [3] camera position: SH view direction mu - cam */
} nlosgr_rays;

/* Scratch bytes for nlosgr_rays_fwd / nlosgr_rays_bwd. */
NLOSGR_API size_t nlosgr_rays_workspace_bytes(const nlosgr_gaussians* g, const nlosgr_rays* r);

/* filter_out [nrays, 1 + NLOSGR_MAX_PER_RAY] int32: count, then the first (by index) Gaussians
 * whose box bboxes[g] = (min xyz, max xyz) the half-infinite ray hits (slab test with
 * 1/(d + 1e-8), cuda_utils.cuh:97-121), -1 padding — the layout filter_gaussians_per_ray returns. */
NLOSGR_API int nlosgr_filter_rays(const nlosgr_gaussians* g, const nlosgr_rays* r, const float* bboxes,
                       int32_t* filter_out, void* hip_stream);

/* Forward: rho_out, density_out, trans_out [nrays, nsamp] (volume_renderer.cu:16-185):
 *   D = sum_{g in filter} sigmoid(o_g) pdf_g(x);  no occlusion: rho = c dT sum sigma pdf rho_g,
 *   trans = 1;  occlusion: rho = T sum (1 - exp(-sigma pdf c dT)) rho_g, T_s = exp(-c dT
 *   sum_{s'<s} D_s'), all three zero where T_s < 1e-4 (the reference's early exit). */
NLOSGR_API int nlosgr_rays_fwd(const nlosgr_gaussians* g, const nlosgr_rays* r, const int32_t* filter,
                    float c_deltaT, int32_t use_occlusion, void* workspace, float* rho_out,
                    float* density_out, float* trans_out, void* hip_stream);

/* Backward of nlosgr_rays_fwd w.r.t. the RAW parameters (the reference returns zeros,
 * cuda_autograd.py:147-156).  Any of g_rho / g_density / g_trans may be NULL.  nrays == 0 is valid
 * (filter may then be NULL) and gives all-zero gradients; ng == 0 is valid and writes nothing. */
NLOSGR_API int nlosgr_rays_bwd(const nlosgr_gaussians* g, const nlosgr_rays* r, const int32_t* filter,
                    float c_deltaT, int32_t use_occlusion, void* workspace, const float* g_rho,
                    const float* g_density, const float* g_trans, float* d_mu, float* d_scaling,
                    float* d_rotation, float* d_opacity, float* d_features, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Path A "analytic section" API (_C.render_rays_analytic, bindings.cpp:6-24,
 * src/volume_renderer_analytic.cu:178-241): hist_out [nrays] = one value per ray.
 * Per ray: the first 128 filter entries whose sigma_threshold-ellipsoid the line o + t d hits,
 * clipped to [t_min, t_max], stably sorted by entry, composited front to back with the
 * reference's closed-form optical depth (analytic_integration.cuh:123-172, formula as written)
 * and early exit at T < 1e-4.  r->t / r->nsamp are unused; features rows have stride k_feat and
 * SH is evaluated to g->sh_degree (unsigned basis, spherical_harmonics.cuh:20-80).  Forward only.
 * ------------------------------------------------------------------------------------- */
NLOSGR_API int nlosgr_rays_analytic(const nlosgr_gaussians* g, const nlosgr_rays* r, const int32_t* filter,
                         float t_min, float t_max, float sigma_threshold, float* hist_out,
                         void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Fused training step: the loss and the optimizer of the reference's
 * learn_one_iter (main.py:198-254) on the device, with no host synchronisation.
 * ------------------------------------------------------------------------------------- */
#define NLOSGR_ADAM_MAX_GROUPS 8

typedef struct {
    float* param;             /* [n] updated in place */
    const float* grad;        /* [n] */
    float* exp_avg;           /* [n] first-moment state, updated in place (zeros before step 1) */
    float* exp_avg_sq;        /* [n] second-moment state, updated in place */
    long long n;
    double lr;                /* this group's learning rate for this step */
} nlosgr_adam_group;

/* Volume MSE of compute_loss (nlos_helpers.py:323-327) over n elements, target scaled by gt_times:
 * loss_out[4] = {mean((hist - gt*target)^2), loss / mean((gt*target)^2), sum (hist - gt*target)^2,
 * sum (gt*target)^2} (device floats; the raw sums let the ranks of a sharded volume combine exactly);
 * grad_out [n] (may be NULL) = grad_scale * 2 (hist - gt*target) / n.  workspace: caller-owned,
 * nlosgr_mse_workspace_bytes() bytes.  Deterministic (fixed-order reduction, no atomics). */
NLOSGR_API size_t nlosgr_mse_workspace_bytes(void);
NLOSGR_API int nlosgr_mse(const float* hist, const float* target, float gt_times, long long n,
               float grad_scale, float* grad_out, void* workspace, float* loss_out, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Temporal instrument response (ABI 12): a measured transient is the ideal one convolved in time with
 * the system's impulse response (laser pulse (*) detector jitter, often with a diffusion tail) on a
 * constant floor of dark counts and ambient light.  Rows are wall points, the time axis is contiguous
 * ([rows, nr], the layout of hist).  An IRF is ntaps real taps w, a centre c (0 <= c < ntaps) and a
 * background b:
 *   apply:    y[p,t] = b + sum_{j<ntaps} w[j] h[p, t + c - j]      (h = 0 outside [0, nr))
 *   adjoint:  g[p,s] =     sum_{j<ntaps} w[j] z[p, s - c + j]      (z = 0 outside [0, nr))
 * c = 0 is a causal response, c = argmax w keeps a peak where it was; ntaps = 1, w = {1}, c = 0, b = 0 is
 * the identity.  Taps may be negative and are not normalised.  Light from before the rendered window
 * counts as zero: a caller who needs the response of earlier bins widens the window by ntaps bins.
 * Each sum is a sequential fp32 fma chain over the taps (apply: ascending j, adjoint: descending j)
 * started at 0, the background added last; no atomics: results are bitwise repeatable and do not depend
 * on how rows are scheduled.  The taps stay on the device (the host validates sizes and pointers only).
 * nr > NLOSGR_IRF_MAX_NR: NLOSGR_E_UNSUPPORTED.
 * ------------------------------------------------------------------------------------- */
#define NLOSGR_IRF_MAX_TAPS 512
#define NLOSGR_IRF_MAX_NR 8192   /* the cap on samples per ray */

typedef struct nlosgr_irf {
    int32_t ntaps, center;
    const float* taps;        /* DEVICE [ntaps] */
    float background;
} nlosgr_irf;

/* y_out [rows, nr] = apply (adjoint == 0; background added) or adjoint (adjoint != 0; no background) of
 * x [rows, nr].  y_out must not alias x.  rows == 0 is valid (nothing is launched). */
NLOSGR_API int nlosgr_irf_apply(const float* x, long long rows, int32_t nr, const nlosgr_irf* irf, int32_t adjoint,
                     float* y_out, void* hip_stream);

/* nlosgr_mse with y = apply(hist) in place of hist, n = rows * nr:  d = y - gt_times * target,
 * loss_out[4] = {mean d^2, that / mean (gt*target)^2, sum d^2, sum (gt*target)^2},
 * grad_out [rows, nr] (may be NULL) = adjoint(grad_scale * 2 d / n) = dL/dhist, which nlosgr_render_bwd
 * takes unchanged.  One pass: hist and target are read once, grad_out is written once.  The loss sums
 * are per-row fp32 partials (fixed tree) in the workspace, added in double in row order (256 consecutive
 * row blocks, then the blocks in order).  workspace: nlosgr_mse_irf_workspace_bytes(rows) bytes.
 * rows == 0 is valid: loss_out is zeros, as nlosgr_mse gives for n == 0. */
NLOSGR_API size_t nlosgr_mse_irf_workspace_bytes(long long rows);
NLOSGR_API int nlosgr_mse_irf(const float* hist, const float* target, float gt_times, long long rows, int32_t nr,
                   const nlosgr_irf* irf, float grad_scale, float* grad_out, void* workspace, float* loss_out,
                   void* hip_stream);

/* Photon-count likelihood (an addition to ABI 13: two new symbols and one new struct; nothing existing changes
 * its signature or layout, so the ABI number stays).  A measured transient is a histogram of photon counts: its
 * noise is Poisson, the variance of a bin is its rate, and the MSE (the likelihood of constant-variance Gaussian
 * noise) puts nearly all its weight on the bright first-return peak.  The fused loss takes a kind:
 *   NLOSGR_LOSS_MSE      nlosgr_mse_irf bit for bit (the same kernel instantiation; rate_floor is ignored)
 *   NLOSGR_LOSS_POISSON  per element, with lambda = apply(hist) (background included), t the target and
 *                        eps = rate_floor > 0:
 *       y'  = max(gt_times t, 0) + eps           measured counts plus the floor
 *       rho = max(lambda, 0) + eps               model rate plus the same floor
 *       dev = 2 [y' log(y'/rho) - (y' - rho)]    the Poisson deviance: >= 0, and 0 exactly when rho = y'
 *       dL/dlambda = (2 / n) (rho - y') / rho  where lambda >= 0, else 0
 *     No special case for empty bins (y' >= eps > 0).  With non-negative taps, render and background the clamp
 *     on lambda never acts; it keeps filters with negative taps from producing NaN.
 *     loss_out[4] = {sum dev / n, sum dev / sum max(gt t, 0) (deviance per measured count; 0 without counts),
 *     sum dev, sum max(gt t, 0)}: the {a/n, a/b, a, b} of the MSE's four floats, so the ranks of a sharded volume
 *     and the batches of a wall combine [2] and [3] the same way.
 *     grad_out (may be NULL) = adjoint(grad_scale dL/dlambda) = dL/dhist, which nlosgr_render_bwd takes unchanged.
 *     Element sequence, one fp32 operation each and no contraction, so that the error can be bounded:
 *       y = gt t;  y' = max(y, 0) + eps;  rho = max(lambda, 0) + eps;  r = rho - y';
 *       z = lambda >= 0 ? gscale (r / rho) : 0          (gscale = grad_scale 2 / n, formed in double)
 *       e = r / y';  dev = 2 y' (e - log1pf(e))
 *     (rho - y') / rho and not 1 - y'/rho: the subtraction is exact where the fit is good.  e is held at the
 *     float above -1: where rho < 2^-25 y' the fp32 r is -y', the reported deviance is then about 31 y' and no
 *     longer grows with log(y'/rho); the gradient is unaffected.
 * rate_floor: the capture's dark-count level is the natural value, with gt_times the knob that brings the capture
 * to counts; one pseudo-count keeps the gradient of a bin the render does not reach yet at about -y, not -y / eps.
 * One pass, no atomics, no LDS beyond nlosgr_mse_irf's; the two per-row partials go through the same tree and are
 * added in double in row order: bitwise repeatable, and independent of how rows are split over calls.
 * Errors: a null loss, an unknown kind, or (POISSON) a rate_floor that is not finite or not > 0: NLOSGR_E_INVALID;
 * the rest as nlosgr_mse_irf (nr > NLOSGR_IRF_MAX_NR: NLOSGR_E_UNSUPPORTED).  rows == 0 is valid and gives zeros.
 * workspace: nlosgr_loss_irf_workspace_bytes(rows) bytes, the size nlosgr_mse_irf_workspace_bytes gives. */
#define NLOSGR_LOSS_MSE 0
#define NLOSGR_LOSS_POISSON 1

typedef struct nlosgr_loss {
    int32_t kind;             /* NLOSGR_LOSS_* */
    float rate_floor;         /* POISSON: eps, finite and > 0 */
} nlosgr_loss;                /* 8 bytes */

NLOSGR_API size_t nlosgr_loss_irf_workspace_bytes(long long rows);
NLOSGR_API int nlosgr_loss_irf(const float* hist, const float* target, float gt_times, long long rows, int32_t nr,
                    const nlosgr_irf* irf, const nlosgr_loss* loss, float grad_scale, float* grad_out,
                    void* workspace, float* loss_out, void* hip_stream);

/* One torch.optim.Adam step (no weight decay, no amsgrad) over 1..NLOSGR_ADAM_MAX_GROUPS parameter
 * groups; `step` >= 1 is the step count including this update (bias correction).  The scalars are
 * doubles so 1 - beta, the bias corrections and lr / (1 - beta1^t) are formed as torch forms them
 * (Python floats) before the fp32 update.  The reference
 * uses betas (0.9, 0.999), eps 1e-15 and six groups (gaussian_model.py:223-242). */
NLOSGR_API int nlosgr_adam(const nlosgr_adam_group* groups, int32_t ngroups, long long step, double beta1,
                double beta2, double eps, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Space-carving initialisation.  votes[v] (v < nvox) = number of wall points i
 * with radius[i] > 0 and |coords[v] - walls[i]| >= radius[i] (fp32, torch.norm order, no fma):
 * the voting loop of space_carving (gaussian_utils.py:88-99).  coords [nvox][3], walls [nwall][3]
 * and radius [nwall] are device arrays in the same frame; votes [nvox] int32 is overwritten.
 * ------------------------------------------------------------------------------------- */
NLOSGR_API int nlosgr_carve_votes(const float* coords, long long nvox, const float* walls, const float* radius,
                       int32_t nwall, int32_t* votes, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Reconstruction output (ABI 9): the trained Gaussians on a regular voxel grid, and maximum
 * projections of such a volume.  The reference's evaluation() calls gaussian2volume (main.py:374-387,
 * nlos_helpers.py:40-69), which evaluates estimate_rho_w(out_separately=True) at the spherical
 * samples of the central wall point; its per-sample "density" there is a flattened [Ng * Na]
 * per-Gaussian tensor, so the quantities implemented here are the two sums of
 * estimate_rho_w_no_occlusion(out_separately=True) (gaussian_model.py:346-364) at voxel centre x:
 *     density(x)        = sum_g sigma_g pdf_g(x)                  (gaussian_model.py:357)
 *     albedo_density(x) = sum_g sigma_g rho_g(cam) pdf_g(x)       (gaussian_model.py:359)
 * sigma_g = sigmoid(opacity_g), rho_g(cam) = max(0, 0.5 + SH_g(dir(mu_g - cam))) (:350-355), pdf_g under
 * the preset / scaling_modifier / sh_degree of `g` exactly as in nlosgr_render_fwd, zero where the
 * Mahalanobis distance m^2 > cutoff^2 when opt->cutoff > 0 (dense when <= 0).
 * Each voxel's sum is formed in ascending Gaussian-index order without atomics: the outputs are
 * bitwise repeatable and do not depend on how the grid is cut into bricks (a sub-grid with the same
 * table values gives the same numbers).
 * ------------------------------------------------------------------------------------- */
typedef struct nlosgr_voxel_grid {
    int32_t nx, ny, nz;       /* extents, each in 1..1024 */
    const float* xs;          /* [nx] device table of voxel-centre x coordinates: uniform, ascending (the */
    const float* ys;          /* [ny]  caller's linspace; the kernels read the coordinates from the tables, */
    const float* zs;          /* [nz]  like nlosgr_geometry.r) */
} nlosgr_voxel_grid;          /* voxel (ix, iy, iz) is stored at (ix*ny + iy)*nz + iz: meshgrid('ij') order,
                                 as in space_carving (gaussian_utils.py:91-93) */

/* Scratch bytes for nlosgr_voxelize (host only; 0 with a message in nlosgr_last_error on invalid input).
 * Uses opt->cutoff only; a non-zero mode, selection or ray_cache is invalid. */
NLOSGR_API size_t nlosgr_voxel_workspace_bytes(const nlosgr_gaussians* g, const nlosgr_voxel_grid* grid,
                                    const nlosgr_options* opt);

/* density_out / albedo_out [nx,ny,nz] (either may be NULL), overwritten.  cam: DEVICE [3], the position the
 * SH albedo is viewed from (the reference uses the central wall point).  With ng == 0 the outputs are
 * zero-filled.  In culled mode a Gaussian whose cutoff box is not finite (NaN / inf parameters) is skipped,
 * as the forward skips it. */
NLOSGR_API int nlosgr_voxelize(const nlosgr_gaussians* g, const nlosgr_voxel_grid* grid, const float* cam,
                    const nlosgr_options* opt, void* workspace, float* density_out, float* albedo_out,
                    void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Backward of nlosgr_voxelize (ABI 13, an addition): with L a function of the two volumes and
 * grad_density = dL/d density, grad_albedo = dL/d albedo_density [nx,ny,nz] (either may be NULL: that volume
 * does not enter L), the gradients of L with respect to the raw parameters of `g`, in the layout of
 * nlosgr_render_bwd: d_mu [ng,3], d_scaling [ng,3], d_rotation [ng,4], d_opacity [ng], d_features [ng,k_feat]
 * with zero in columns >= (sh_degree+1)^2.  The albedo's clamp passes gradient where 0.5 + SH >= 0.
 *   support      a (voxel, Gaussian) pair contributes iff it contributes to nlosgr_voxelize under the same
 *                arguments (the same cutoff box and the same fp32 mask), and a pair outside is dropped, not
 *                multiplied by zero: a non-finite upstream value reaches exactly the Gaussians whose support
 *                holds that voxel.  cutoff <= 0 is dense (every pair; slow, for tests).  In culled mode a
 *                Gaussian whose cutoff box is empty or not finite gets all-zero rows, as the forward skips it.
 *   determinism  a Gaussian's rows depend on that Gaussian, the grid tables, cam, opt->cutoff and the upstream
 *                alone, not on ng, the other Gaussians or the launch shape; no atomics.  Two runs are bitwise
 *                equal, and permuting the Gaussians permutes the rows bitwise.
 *   outputs      overwritten.  Both upstream pointers NULL: the five outputs are zero-filled.  ng == 0: nothing
 *                is written, nothing is launched.
 *   validation   on the host before any launch: nlosgr_voxelize's, plus NLOSGR_E_INVALID for a NULL cam and,
 *                when ng > 0, a NULL output or workspace.
 * The library neither allocates nor synchronises.
 * ------------------------------------------------------------------------------------- */

/* Scratch bytes for nlosgr_voxelize_bwd (host only; 0 with a message in nlosgr_last_error on invalid input). */
NLOSGR_API size_t nlosgr_voxel_bwd_workspace_bytes(const nlosgr_gaussians* g, const nlosgr_voxel_grid* grid,
                                        const nlosgr_options* opt);

NLOSGR_API int nlosgr_voxelize_bwd(const nlosgr_gaussians* g, const nlosgr_voxel_grid* grid, const float* cam,
                        const nlosgr_options* opt, void* workspace, const float* grad_density,
                        const float* grad_albedo, float* d_mu, float* d_scaling, float* d_rotation,
                        float* d_opacity, float* d_features, void* hip_stream);

/* Maximum of vol [nx,ny,nz] along `axis` (0..2) and the index of that maximum (ties: lowest index, so an
 * all-zero column gives (0, 0)); max_out (float) / argmax_out (int32), either may be NULL, are laid out as
 * the two remaining axes in their original order. */
NLOSGR_API int nlosgr_volume_project(const float* vol, int32_t nx, int32_t ny, int32_t nz, int32_t axis,
                          float* max_out, int32_t* argmax_out, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Surface output (ABI 11): the isosurface {x : vol(x) = level} of a regular-grid volume as an indexed
 * triangle mesh.  It stands where the reference has gaussian2volume(mode='mesh') (nlos_helpers.py:50-69):
 * the same threshold (the caller passes the density's mean, :51), with an isosurface in place of the
 * open3d Poisson reconstruction.  Marching tetrahedra on the Kuhn decomposition (6 tetrahedra per cell,
 * translation invariant, so the index topology is watertight); no atomics, a fixed output order, two runs
 * bitwise equal.
 *   inside      grid point p is inside iff isfinite(vol) && vol >= level (NaN, +-inf: outside)
 *   edges       p owns p -> p + d, d0..d6 = (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1), where the
 *               far end is in the grid; an edge crosses when exactly one end is inside
 *   vertices    one per crossing edge, numbered by owner index (ix*ny + iy)*nz + iz, then d.  With fa, fb at
 *               the owner and the far end: t = (level - fa) / (fb - fa) in fp32, 0.5 if either is not finite;
 *               position (1-t) xa + t xb per axis from the tables (fmaf; exactly the end point at t = 0 / 1),
 *               value (1-t) aa + t ab, normal -normalize((1-t) ga + t gb) with g the central difference
 *               (f[i+1] - f[i-1]) / (x[i+1] - x[i-1]) per axis, one-sided at the ends; (0,0,0) when that
 *               vector has zero or non-finite length.  Normals point from high values to low.
 *   tetrahedra  cell p (ix < nx-1, iy < ny-1, iz < nz-1), tau = 0..5 over the axis permutations (a,b,c) in
 *               lexicographic order: v0 = p, v1 = v0 + e_a, v2 = v1 + e_b, v3 = p + (1,1,1); mask bit i: v_i inside
 *   triangles   (XY = the vertex on edge v_X v_Y) one inside A, outside O1<O2<O3: (AO1, AO2, AO3); three
 *               inside I1<I2<I3, outside D: (I1D, I2D, I3D); two inside A<B, outside C<D: (AC, AD, BD),
 *               (AC, BD, BC); the last two vertices swapped where the same triangle through the edge
 *               midpoints of the unit cell would face the inside corners, so every non-degenerate triangle
 *               is counter-clockwise seen from the low side.  Numbered by cell index
 *               (ix*(ny-1) + iy)*(nz-1) + iz, then tau, then the order above; int32 indices.
 * A corner value equal to `level` gives t = 0 or 1, coincident vertices and zero-area triangles, which are
 * kept: the index topology stays manifold.  Any extent < 2: the mesh is empty.
 * The tables of the grid are read as given (ascending, not assumed uniform).
 * Two calls with one host read of counts_out between them (the library neither allocates nor synchronises).
 * ------------------------------------------------------------------------------------- */

/* Scratch bytes for nlosgr_mesh_count / nlosgr_mesh_emit (host only; 0 with a message in nlosgr_last_error on
 * invalid extents or NULL tables): 12 B per grid point plus block sums. */
NLOSGR_API size_t nlosgr_mesh_workspace_bytes(const nlosgr_voxel_grid* grid);

/* Classifies every grid point and scans the counts into `workspace` (reduce per block / scan of the block
 * sums / add back: three launches, no workgroup waits on another).  counts_out: DEVICE [2] = {nverts, ntris},
 * 64-bit totals; the per-point offsets kept in the workspace are 32-bit. */
NLOSGR_API int nlosgr_mesh_count(const float* vol, const nlosgr_voxel_grid* grid, float level, void* workspace,
                      long long* counts_out, void* hip_stream);

/* Writes the mesh nlosgr_mesh_count counted (same vol, grid, level, workspace).  attr (may be NULL): a second
 * volume of the same shape to interpolate a per-vertex value from.  verts_out [nverts,3], normals_out
 * [nverts,3] (may be NULL), attr_out [nverts] (NULL iff attr is NULL), tris_out [ntris,3].
 * nverts or ntris above 2^31 - 1: NLOSGR_E_UNSUPPORTED.  Counts that disagree with the workspace's totals
 * cannot be seen by the host without a synchronisation: the kernels then write nothing, and no kernel ever
 * writes past nverts / ntris. */
NLOSGR_API int nlosgr_mesh_emit(const float* vol, const float* attr, const nlosgr_voxel_grid* grid, float level,
                     const void* workspace, long long nverts, long long ntris, float* verts_out,
                     float* normals_out, float* attr_out, int32_t* tris_out, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Back-projection of a confocal capture (ABI 13): the voxel-wise sum of each wall point's histogram at the
 * voxel's time of flight.  rows is [nwall][nr] (the layout data.volume_target returns), walls is [nwall][3],
 * out is [nx,ny,nz] in nlosgr_voxel_grid order; all device fp32.
 * For voxel centre x, taken from the grid's tables, and wall point i:
 *   d = sqrt((dx*dx + dy*dy) + dz*dz), in fp32 and in this order, with no contraction, as carve_kernel forms it.
 *   u = (d - r0) * inv_dr, k = floor(u), f = u - k.
 *   s_i = (1-f) h_i[k] + f h_i[k+1], with h_i[j] = 0 for j < 0 or j >= nr.
 *     s_i is continuous in d everywhere, including at both ends of the window.
 *     It is zero for u <= -1 or u >= nr.
 *   out(x) = sum_i d^power s_i.
 * Summation order is fixed and has no atomics: wall points are taken in ascending order, in tiles of 256
 * counted from this call's wall point 0; each tile is summed term by term in fp32; the tile sums are added
 * into a per-voxel fp64 register accumulator, which is rounded to fp32 once at the end.  The result is
 * bitwise repeatable and independent of how the grid is cut into workgroups: a sub-grid with the same table
 * values gives the same numbers.  The square root is the hardware one (1 ulp), d^2 = d*d, d^3 = d^2*d,
 * d^4 = d^2*d^2.
 * accumulate = 1 adds the call's rounded sum to out: one more rounding per call.  It exists so a wall can be
 * back-projected in batches or per rank, and is close to, not bitwise equal to, one call over the whole wall.
 * Non-finite histogram values propagate to the voxels that sample them (0 * NaN included).  nwall == 0
 * zero-fills out, or leaves it untouched with accumulate.  No workspace.
 * ------------------------------------------------------------------------------------- */
typedef struct nlosgr_backproject_opts {
    float   r0;          /* radius of bin 0 of the rows (I1 * c * deltaT) */
    float   inv_dr;      /* 1 / (c * deltaT), the caller's fp32 value */
    int32_t power;       /* weight d^power, 0..4 (falloff compensation) */
    int32_t accumulate;  /* 0: overwrite out; 1: add this call's sum to out */
} nlosgr_backproject_opts;

/* Validated on the host (NLOSGR_E_INVALID): extents 1..1024, nr >= 1, nwall >= 0, power 0..4, inv_dr finite and
 * > 0, r0 finite, null pointers (rows / walls may be NULL only when nwall == 0). */
NLOSGR_API int nlosgr_backproject(const float* rows, const float* walls, int32_t nwall, int32_t nr,
                       const nlosgr_voxel_grid* grid, const nlosgr_backproject_opts* opt,
                       float* out, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Forward projection of a voxel grid (ABI 13, an addition): the transient every wall point of a confocal
 * capture would measure from the volume, the adjoint of the back-projection above.  vol is [nx,ny,nz] in
 * nlosgr_voxel_grid order, walls is [nwall][3], rows_out is [nwall][nr]; all device fp32.
 * With d, u, k, f formed exactly as the back-projection forms them (same fp32 order, no contraction, the
 * hardware square root), for voxel centre x and wall point i:
 *   rows_i[j] = sum_x d^power vol(x) ((1-f) [k == j] + f [k+1 == j]),   0 <= j < nr.
 * Both operators use the same fp32 coefficients, so <A v, h> = <v, A^T h> holds in exact summation for the
 * powers 0..4 they share.  Negative powers are the physical falloff (-4: the confocal 1 / r^4); d^-p is
 * 1 / d^p with d^p formed as the back-projection forms it.
 * Contract:
 *   1. No float atomics.  Every term is rounded once to the nearest multiple of a quantum q and added as a
 *      64-bit integer (two's complement), so the result is bitwise repeatable and independent of nsplit, of
 *      the launch shape and of the order workgroups run in.  A bin's integer sum is converted once:
 *      int64 -> double, times q, -> fp32.  q = 2^(e - S) with
 *        S  = 62 - ceil(log2(2 nvox)), nvox = nx ny nz;
 *        e  = ev + ew;  max|vol| = m 2^ev with m in [0.5, 1) (frexp), found by a device reduction into the
 *             workspace with no host synchronisation;  wmax = m' 2^ew likewise, where wmax is the host's
 *             double-precision bound on the weight of every contributing pair:
 *        wmax = R^|power| (|power| multiplications from 1.0; the reciprocal of that for power < 0) times
 *             (1 + 2^-19), R = max(r0 + (nr + 1) dr, 0) for power >= 0 and R = r0 - 1.5 dr for power < 0,
 *             dr = 1 / inv_dr in double.
 *      So max|vol| wmax < 2^e, every term is below 2^S quanta and a bin's sum of at most nvox terms stays below
 *      2^61.  q depends on (max|vol|, opts, nr, nvox) alone: a volume that is zero outside a sub-grid gives
 *      bitwise the rows of the call on that sub-grid when ceil(log2(2 nvox)) is the same for both.
 *   2. max|vol| == 0: zero rows.
 *   3. Any non-finite voxel makes EVERY output row NaN (the back-projection poisons only the voxels that sample
 *      a NaN bin; here the quantum cannot be formed, and a silent partial result would be worse).
 *   4. nwall == 0 is valid and writes nothing.
 *   5. nr > NLOSGR_IRF_MAX_NR: NLOSGR_E_UNSUPPORTED (the per-wall-point LDS row is 8 nr bytes).
 *   6. Validated on the host before any launch (NLOSGR_E_INVALID): extents 1..1024, nr >= 1, nwall >= 0, power
 *      -4..4, inv_dr finite and > 0, r0 finite, power < 0 only with r0 * inv_dr >= 2 (a pair contributes only
 *      when u > -1, which then bounds d from below), nsplit >= 0, a finite wmax, null structs, tables and
 *      pointers (walls / rows_out may be NULL only when nwall == 0).
 *   7. No lane adds outside its row, whatever u is: u is clamped into [-2, nr + 1] (NaN to -2) and each add is
 *      masked by its bin index.
 * accumulate = 1 adds the call's rounded fp32 sum to rows_out: one more rounding per call (a volume projected
 * as sub-grids or per rank); a non-finite voxel still writes NaN.
 * A workgroup serves W wall points (the most of 4, 2, 1 that the wall has and whose rows fit 32 KiB of LDS) and
 * one of nsplit parts of the voxels; nsplit = 0 lets the library choose (ceil(1024 / ceil(nwall / W)), at most
 * one part per 1024 voxels), another value is forced (at most one part per 4 voxels).  Workspace: 256 bytes, plus
 * 8 nwall nr when more than one part is used; the library neither allocates nor synchronises.
 * ------------------------------------------------------------------------------------- */
typedef struct nlosgr_forward_project_opts {
    float   r0, inv_dr;  /* as nlosgr_backproject_opts */
    int32_t power;       /* weight d^power, -4..4 */
    int32_t accumulate;  /* 0: overwrite rows_out; 1: add this call's rounded sum */
    int32_t nsplit;      /* voxel splits per wall point: 0 = chosen by the library, else forced (tests) */
} nlosgr_forward_project_opts;

/* Scratch bytes (host only; 0 with a message in nlosgr_last_error on the errors of contract 5 and 6). */
NLOSGR_API size_t nlosgr_forward_project_workspace_bytes(int32_t nwall, int32_t nr, const nlosgr_voxel_grid* grid,
                                              const nlosgr_forward_project_opts* opt);

NLOSGR_API int nlosgr_forward_project(const float* vol, const float* walls, int32_t nwall, int32_t nr,
                           const nlosgr_voxel_grid* grid, const nlosgr_forward_project_opts* opt,
                           void* workspace, float* rows_out, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Non-confocal back-projection and forward projection (ABI 13, additions): measurement i is sensed at wall
 * point s_i (sensors [nmeas][3], what the confocal entry points call walls) while the laser lights wall point
 * l_i (lasers [nlaser][3]; nlaser == nmeas: one spot per measurement, nlaser == 1: one spot for the whole
 * capture).  Light of voxel x travels |x - l_i| + |x - s_i|, and the rows' bins hold HALF that path: r0 is the
 * radius of bin 0 and 1 / inv_dr = c deltaT the bin width in half-path units, as in a confocal capture.
 * For voxel centre x and measurement i, all fp32, no contraction, the hardware square root:
 *   ds = |x - s_i|, dl = |x - l_i|, each formed as the confocal d: sqrt((dx*dx + dy*dy) + dz*dz).
 *   g = 0.5f * (dl + ds): half the path.  m = dl * ds.
 *   u = (g - r0) * inv_dr, k = floor(u), f = u - k; clamps and masks as the confocal kernels.
 *   weight = m^(power/2): 0: 1; 1: sqrt(m); 2: m; 3: m * sqrt(m); 4: m * m; a negative power: 1 / that
 *     (-4 is the physical 1 / (dl^2 ds^2)).
 *   back-projection:     out(x)    = sum_i weight ((1-f) h_i[k] + f h_i[k+1])
 *   forward projection:  rows_i[j] = sum_x weight vol(x) ((1-f) [k == j] + f [k+1 == j])
 * With l_i == s_i: g == d and m == d*d exactly, so the even powers give the confocal entry points' results bit
 * for bit; the odd powers differ by the rounding of sqrt(d*d) against d.  nlaser == 1 gives bitwise the result of
 * the same spot repeated nmeas times (the laser distance is then formed once per voxel, not once per pair).
 * The contracts of the confocal entry points carry over unchanged:
 *   back-projection: measurements in ascending order, tiles of 256 counted from measurement 0, an fp32 sum
 *     within a tile, an fp64 sum across tiles, one rounding to fp32; accumulate, NaN bins and nmeas == 0 as there.
 *     Validated as there (power 0..4), plus nlaser in {1, nmeas} and a null lasers pointer.
 *   forward projection: contracts 1..7 of the forward-projection block above (64-bit fixed-point adds, no float
 *     atomics, independent of nsplit and launch shape, a non-finite voxel makes every row NaN, nmeas == 0 writes
 *     nothing, nr > NLOSGR_IRF_MAX_NR is NLOSGR_E_UNSUPPORTED, no add outside a row), the same workspace
 *     layout and size, with two changes to the quantum's wmax:
 *       power >= 0: unchanged, R = max(r0 + (nr + 1) dr, 0): m <= g^2 (AM-GM), and g is inside the window.
 *       power <  0: the window does not bound m from below (a voxel may sit next to the laser while far from
 *         the sensor), so the caller passes dmin: a pair with min(dl, ds) < dmin contributes nothing, and
 *         wmax is formed with R = dmin.  dmin must be finite and > 0 (NLOSGR_E_INVALID otherwise); the confocal
 *         rule r0 * inv_dr >= 2 is not required.  dmin is ignored for power >= 0.
 *     Validated as there, plus nlaser in {1, nmeas}, a null lasers pointer and the dmin rule.
 * ------------------------------------------------------------------------------------- */
NLOSGR_API int nlosgr_backproject_nc(const float* rows, const float* sensors, const float* lasers, int32_t nlaser,
                          int32_t nmeas, int32_t nr, const nlosgr_voxel_grid* grid,
                          const nlosgr_backproject_opts* opt, float* out, void* hip_stream);

/* Scratch bytes (host only; 0 with a message in nlosgr_last_error on a validation error). */
NLOSGR_API size_t nlosgr_forward_project_nc_workspace_bytes(int32_t nlaser, int32_t nmeas, int32_t nr,
                                                 const nlosgr_voxel_grid* grid,
                                                 const nlosgr_forward_project_opts* opt, float dmin);

NLOSGR_API int nlosgr_forward_project_nc(const float* vol, const float* sensors, const float* lasers, int32_t nlaser,
                              int32_t nmeas, int32_t nr, const nlosgr_voxel_grid* grid,
                              const nlosgr_forward_project_opts* opt, float dmin, void* workspace,
                              float* rows_out, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Phasor-field reconstruction (ABI 13, an addition: one new symbol, nothing existing changes): the
 * back-projection of COMPLEX rows in one pass.  rows_c is [nmeas][nr][2], bin j of measurement i stored as
 * (re, im): the capture filtered in time with a complex wavelet (the virtual illumination; nlosgr/phasor.py
 * builds the Morlet wavelet and the rows).  lasers == NULL with nlaser == 0 is a confocal capture and uses
 * nlosgr_backproject's arithmetic per (voxel, measurement) pair (d-based, so every power matches it); otherwise
 * lasers is [nlaser][3] with nlaser in {1, nmeas} and the arithmetic is nlosgr_backproject_nc's.
 *   planes [2][nx][ny][nz]: plane 0 is bitwise what the real entry point gives for the rows' re channel alone,
 *     plane 1 for the im channel: the coordinate, the clamp into [-2, nr + 1], k, f, the weight and the selects
 *     that drop out-of-row values are formed once per pair and shared by both channels; each channel is then
 *     summed under the real entry points' contract (measurements in ascending order, tiles of 256 counted from
 *     measurement 0, an fp32 sum within a tile started at 0, an fp64 sum across tiles, one rounding to fp32).
 *     opt->accumulate adds this call's rounded sums into planes.  No atomics: bitwise repeatable, independent of
 *     bricks; nlaser == 1 gives bitwise the result of that spot repeated nmeas times.  NaN / inf bins reach
 *     exactly the voxels that sample them, per channel.
 *   mag [nx][ny][nz] or NULL: (float)sqrt((double)re*re + (double)im*im) of the fp32 plane values as this call
 *     leaves them (after accumulation), written in the same kernel; NaN where either plane is NaN.
 *   nmeas == 0: planes is zeroed (left as it is under accumulate) and mag is still the magnitude of planes.
 *   One 16-byte read per pair at complex bin clamp(k, 0, nr - 2), 8-byte aligned and inside the row (nr == 1: one
 *     8-byte read): rows_c must be 8-byte aligned.
 *   Validated on the host before any launch as nlosgr_backproject_nc, plus a NULL planes and an nlaser that does
 *     not fit lasers (NLOSGR_E_INVALID).
 * ------------------------------------------------------------------------------------- */
NLOSGR_API int nlosgr_backproject_phasor(const float* rows_c, const float* sensors, const float* lasers,
                              int32_t nlaser, int32_t nmeas, int32_t nr, const nlosgr_voxel_grid* grid,
                              const nlosgr_backproject_opts* opt, float* planes, float* mag, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Non-confocal Gaussian renderer (ABI 13, an addition: three new symbols, nothing existing changes): the
 * histogram nlosgr_render_fwd gives for a confocal capture, for a capture whose measurement p is sensed at
 * s_p = geo->wall[p] while the laser lights l_p (lasers [nlaser][3], nlaser == nmeas = geo->nwall: one spot per
 * measurement; nlaser == 1: one spot for the capture), and its backward.  geo holds the tables of the SENSED
 * points, exactly as for a confocal capture; bin k holds HALF the path, tau_k = geo->r[k], as in the
 * non-confocal voxel operators.  Rays leave the sensed point: omega_ij = (st_i cp_j, st_i sp_j, ct_i).  With
 * Delta = l_p - s_p, b^2 = |Delta|^2 and c = omega . Delta, the point of ray omega on the ellipsoid
 * |x - s| + |x - l| = 2 tau is
 *     D  = tau - c/2
 *     d  = (tau^2 - b^2/4) / D = tau + (c tau/2 - b^2/4) / D     distance from s;  x = s + d omega
 *     dl = 2 tau - d = |x - l|                                   (dl >= D > 0 whenever tau > b/2)
 * and the histogram is
 *     hist[p,k] = hscale[p] att[k] sum_ij sin(theta_i) q_pijk sum_g w_g(p) pdf_g(x_pijk)
 *     q_pijk    = tau_k^2 / (dl D);   q = 0 in bins with tau_k <= b/2 (no such path exists)
 *     w_g(p)    = sigmoid(opacity_g) max(0, 0.5 + SH_g(dir(mu_g - s_p)))          as nlosgr_render_fwd
 * (the shell measure d^2 sin(theta) dtheta dphi (dl / D) dtau times the physical falloff 1 / (d^2 dl^2) is
 * sin(theta) / (dl D); the confocal sin(theta) / tau^2 already sits in att[k], and q is the ratio of the two).
 * With l_p == s_p: q = 1 and d = tau, the confocal renderer's quantity.
 *   scope        NLOSGR_MODE_NOOCL, NLOSGR_SELECT_SUPPORT, the histogram only; both presets with every SH degree
 *                nlosgr_render_fwd takes; cutoff > 0 is culled, cutoff <= 0 dense (every sample; slow, for tests).
 *   validation   on the host before any launch: another mode, NLOSGR_SELECT_AABB or ray_cache != 0:
 *                NLOSGR_E_UNSUPPORTED; a non-zero nsplit, g_begin, g_end or flags, a NULL lasers or nlaser not in
 *                {1, nmeas}: NLOSGR_E_INVALID; otherwise what nlosgr_render_fwd validates, and a NULL hist_out
 *                (nmeas > 0), output or workspace (ng > 0): NLOSGR_E_INVALID.
 *   outputs      overwritten.  ng == 0: hist_out is zero-filled, and the backward writes and launches nothing.
 *                nmeas == 0 is valid (the backward then zero-fills its outputs, as with a NULL grad_hist).  A bin
 *                with tau_k <= b/2 is exactly 0 and takes no gradient.  d_features is [ng,k_feat] with zero in
 *                columns >= (sh_degree+1)^2; the other outputs are laid out as nlosgr_render_bwd's.
 *   determinism  no float atomics.  Two runs are bitwise equal.  Row p of the forward depends on measurement p,
 *                the Gaussians and opt alone (each bin's sum runs over the Gaussians in ascending index, then the
 *                rays in (i, j) order): rendering a subset of the measurements gives bitwise those rows.  In the
 *                backward a Gaussian's five rows depend on that Gaussian, the geometry, the lasers, opt and the
 *                upstream alone, not on the other Gaussians, ng or the order: permuting the Gaussians permutes
 *                the rows bitwise.  nlaser == 1 gives bitwise the result of that spot repeated nmeas times.
 *   one support  the same device functions decide, in both directions and from the same fp32 inputs, a pair's
 *                cull, its (theta, phi) box, a ray's bin range [kl, kh] (the bins whose d lies in the ray's
 *                in-support interval; d grows with tau and tau(d) = (d + sqrt(d^2 - 2 d c + b^2)) / 2 inverts it)
 *                and a bin's validity, so a (p, i, j, k, g) sample is in the backward iff it is in the forward.
 *                A sample outside is dropped, not multiplied by zero.
 *   skipped      in culled mode a Gaussian with a non-finite parameter record is skipped (zero rows).  A clamped
 *                albedo (0.5 + SH < 0) contributes nothing and gets zero feature and mu-through-SH gradient.
 * The library neither allocates nor synchronises.  Sharding needs nothing here: a slice of geo's rows with the
 * same rows of lasers is a valid call, and by the determinism clause gives those rows bitwise.
 * ------------------------------------------------------------------------------------- */

/* Scratch bytes for nlosgr_render_nc_fwd / _bwd (host only; 0 with a message in nlosgr_last_error on invalid input). */
NLOSGR_API size_t nlosgr_render_nc_workspace_bytes(const nlosgr_gaussians* g, const nlosgr_geometry* geo,
                                        int32_t nlaser, const nlosgr_options* opt);

/* hist_out [nmeas, nr]. */
NLOSGR_API int nlosgr_render_nc_fwd(const nlosgr_gaussians* g, const nlosgr_geometry* geo, const float* lasers,
                         int32_t nlaser, const nlosgr_options* opt, void* workspace, float* hist_out,
                         void* hip_stream);

/* grad_hist [nmeas, nr] (NULL: the outputs are zero-filled) -> the gradients of the raw parameters. */
NLOSGR_API int nlosgr_render_nc_bwd(const nlosgr_gaussians* g, const nlosgr_geometry* geo, const float* lasers,
                         int32_t nlaser, const nlosgr_options* opt, void* workspace, const float* grad_hist,
                         float* d_mu, float* d_scaling, float* d_rotation, float* d_opacity, float* d_features,
                         void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * SGLD noise step (an addition to ABI 13: one new symbol and one new struct, nothing existing changes): the
 * position noise of 3DGS-MCMC's sampler, applied after an optimizer step.  Each nearly transparent Gaussian gets a
 * kick shaped by its own covariance; no counterpart in the reference, which leaves the spot open in both training
 * loops (main.py:163-164, 215-217).  One thread per Gaussian; rows are independent; no atomics, no LDS, no
 * workspace, no generator state on the device.  For row i of g, with n = first_index + i:
 *   words     x0..x3 = Philox4x32-10 (Salmon et al. 2011; multipliers D2511F53, CD9E8D57, key increments 9E3779B9,
 *             BB67AE85, ten rounds) of the counter (lo32 n, hi32 n, lo32 iteration, hi32 iteration) under the key
 *             (lo32 seed, hi32 seed).
 *   uniforms  u_j = ((x_j >> 9) + 0.5) 2^-23: exact in fp32, never 0 or 1.
 *   normals   xi0 = sqrt(-2 ln u0) cos(2 pi u1), xi1 = sqrt(-2 ln u0) sin(2 pi u1), xi2 = sqrt(-2 ln u2) cos(2 pi u3)
 *             (Box-Muller; the accurate logf and sqrtf, cos / sin (2 pi u) as cospif / sinpif (2 u): 2 u is exact in
 *             fp32, so each normal carries a few ulp of its own size, also where the cosine is near zero).
 *   gate      sigma = sigmoid(opacity_i) as nlosgr_render_fwd forms it;  a = (1 - sigma) - gate_x0;
 *             gate = 1 / (1 + expf(-gate_k a)): 3DGS-MCMC's op_sigmoid(1 - opacity) with k = 100, x0 = 0.995.  Where
 *             expf overflows to inf the gate is exactly 0 (never NaN).
 *   shape     with s~ and R' of the preset / scaling_modifier of `g` exactly as in nlosgr_render_fwd, the Gaussian's
 *             covariance is Sigma = R'^T diag(s~^2) R' (the inverse of the renderer's N = A^T A), and
 *             Sigma xi = R'^T (s~^2 o (R' xi)); Sigma itself is not formed.  Sigma, not its square root: 3DGS-MCMC's
 *             own rule.
 *   result    delta = (scale gate) (Sigma xi), rounded to fp32, then mu_out[i] = mu[i] + delta in one fp32 addition
 *             (no fma of the two), and noise_out[i] = delta when given: mu + noise_out == mu_out bitwise.
 * The result is a function of (seed, iteration, n) and row i alone: two runs are bitwise equal; a slice of the rows
 * with first_index moved along gives bitwise those rows; every rank that holds the same Gaussians computes the same
 * values, so a wall shard exchanges nothing for it.  mu_out may alias g->mu (each thread reads its row before it
 * writes it).  A non-finite parameter makes that Gaussian's own row non-finite and no other.  sh_degree, k_feat and
 * features of `g` are not read.
 * ng == 0 is valid and launches nothing.  NLOSGR_E_INVALID: a null struct, ng < 0, an unknown preset and, when
 * ng > 0, a null mu, scaling, rotation, opacity or mu_out.  The library neither allocates nor synchronises.
 * ------------------------------------------------------------------------------------- */
typedef struct nlosgr_sgld {
    uint64_t seed;        /* Philox key */
    int64_t  iteration;   /* Philox counter words 2,3 */
    int64_t  first_index; /* index of row 0 of g in the whole model: counter words 0,1 = first_index + i */
    float    scale;       /* noise_lr * lr_mu, formed in double by the caller */
    float    gate_k, gate_x0;   /* 3DGS-MCMC: 100, 0.995 */
} nlosgr_sgld;

NLOSGR_API int nlosgr_sgld_noise(const nlosgr_gaussians* g, const nlosgr_sgld* o,
                      float* mu_out /* [ng,3], may alias g->mu */,
                      float* noise_out /* [ng,3] or NULL */, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * f-k migration of a confocal capture (an addition to ABI 13: three new symbols, nothing existing changes): Lindell,
 * Wetzstein, O'Toole 2019.  No counterpart in the reference.  The transform is
 *     rows -> amplitude -> zero-padded 3-D FFT -> Stolt resampling -> inverse FFT -> |.|^2
 * on the capture's own (wall point x time bin) lattice, O(N^3 log N) against the O(N^5) of a back-projection.  The two
 * FFTs are the caller's (the library links the HIP runtime alone); the three symbols are the passes around them.
 *
 * Input: rows [H W][nr]; lattice point (m, n), 0 <= m < H, 0 <= n < W, is measured at (xs[n], y0, zs[m]) with uniform
 * spacings sx, sz, and its row is rows[perm[m stride_m + n stride_n]] (perm NULL: rows[m stride_m + n stride_n]; the
 * strides are (W, 1) when x runs along the wall's fast index and (1, H) when it runs along the slow one).  r0: radius
 * of bin 0, dr: bin width, both in half-path units.  Nz = 2 H, Nx = 2 W, Nt = 2 nr; the work arrays are complex64
 * [Nz][Nx][Nt], interleaved (re, im).
 *   1 load    psi[m][n][j] = max(rows[v][j], 0) (r0 + j dr)^power, power 0..4 (4: the r^-4 falloff of the renderer's
 *             histograms); with `amplitude` its square root.  pad = psi at [0:H][0:W][0:nr] of a zero array; the
 *             padding is zero-filled in the same pass.
 *   2         S = the unnormalised forward 3-D DFT of pad, exp(-2 pi i ...) (numpy's fftn).
 *   3 stolt   with signed DFT indices c (z), b (x), a (time), gx = Nt dr / (Nx sx), gz = Nt dr / (Nz sz):
 *                 src = sqrt(a^2 + (gx b)^2 + (gz c)^2),  k = floor(src),  f = src - k
 *                 V[c][b][a] = ((1-f) S[c][b][k] + f S[c][b][k+1]) (a / src) exp(-2 pi i (src - a) (r0 / dr) / Nt)
 *             where a > 0 and k + 1 <= Nt/2 - 1;  V = 0 everywhere else (a <= 0, or a source beyond the positive band),
 *             written in the same pass.  The phase factor lets a window start at bin I1 > 0 without I1 bins of padding
 *             in front: it moves the input window back by r0 and the output depth forward by r0.
 *   4         o = the inverse 3-D DFT of V with the 1/N normalisation (numpy's ifftn).
 *   5 store   volume[n][j][m] = |o[m][n][j]|^2 for m < H, n < W, j < nr: [nx = W][ny = nr][nz = H] in the voxel order
 *             (ix ny + iy) nz + iz of nlosgr_voxel_grid; voxel (n, j, m) is the point (xs[n], y0 + r0 + j dr, zs[m]).
 * Each pass reads and writes its array once, without atomics; every element is written by one lane from the inputs
 * alone: bitwise repeatable.  Arithmetic: csrc/nlosgr_fk.hip.  The migrated spectrum must not alias the spectrum.
 * Validated on the host before any launch (NLOSGR_E_INVALID, text in the last-error string): H, W or nr outside
 * 1..1024, power outside 0..4, dr <= 0 or not finite, r0 < 0 or not finite, sx or sz <= 0, strides that leave
 * [0, H W), a null or misaligned pointer (perm may be NULL).  The library neither allocates nor synchronises.
 * ------------------------------------------------------------------------------------- */
NLOSGR_API int nlosgr_fk_load(const float* rows /* [H W][nr] */, const int32_t* perm /* [H W] or NULL */, int32_t H,
                   int32_t W, int32_t nr, int32_t stride_m, int32_t stride_n, float r0, float dr, int32_t power,
                   int32_t amplitude, float* pad /* [2H][2W][2nr][2], 16-byte aligned */, void* hip_stream);
NLOSGR_API int nlosgr_fk_stolt(const float* spec /* [2H][2W][2nr][2] */, int32_t H, int32_t W, int32_t nr, float sx,
                    float sz, float r0, float dr, float* out /* [2H][2W][2nr][2], 16-byte aligned */,
                    void* hip_stream);
NLOSGR_API int nlosgr_fk_store(const float* field /* [2H][2W][2nr][2] */, int32_t H, int32_t W, int32_t nr,
                    float* volume /* [W][nr][H] */, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Fast phasor-field reconstruction (an addition to ABI 13: four new symbols, nothing existing changes): the phasor
 * field evaluated as Rayleigh-Sommerfeld diffraction, RSD (Liu, Bauer, Velten 2020).  No counterpart in the reference.
 * For one depth plane and one temporal frequency the sum over the wall points is a 2-D convolution over the wall's
 * lattice, so an FFT does it: O(N^3 log N) per band frequency against the O(N^5) of nlosgr_backproject_phasor.  It holds
 * for a confocal capture and for one fixed laser spot with a scanned sensor lattice, because the weight of
 * nlosgr_backproject_nc, (|x - laser| |x - wall|)^(power/2), separates into a laser factor and a sensor factor.  The
 * FFTs are the caller's (the library links the HIP runtime alone); the four symbols are the passes around them.
 *
 * Input: rows [H W][nr] fp32; lattice point (m, n) is measured at (xs[n], y0, zs[m]) with uniform spacings sx, sz, and
 * its row is rows[perm[m stride_m + n stride_n]], as for nlosgr_fk_load.  r0: radius of bin 0, dr: bin width, in
 * half-path units.  ys [ny]: an ascending depth table of any spacing, D_j = ys[j] - y0 > 0.  wavelength, cycles: those
 * of the Morlet wavelet of nlosgr/phasor.py (phasor_kernel).  power 0..4.  laser: one point, or none (confocal).  Nt:
 * an even DFT length, nr <= Nt <= 8192.
 *
 * Band (built by the caller in double from the fp32 r0 and dr; nlosgr/rsd.py rsd_band):
 *     P = wavelength / (2 dr), sigma_b = cycles P / 6, theta_q = 2 pi q / Nt, theta_0 = 2 pi / P,
 *     q_0 = Nt / P, sigma_q = Nt / (2 pi sigma_b), q_lo = max(1, ceil(q_0 - 3 sigma_q)),
 *     q_hi = min(Nt/2 - 1, floor(q_0 + 3 sigma_q)), nq = q_hi - q_lo + 1 (1..512),
 *     coef[q] = exp(-(sigma_b (theta_q - theta_0))^2 / 2) exp(-i theta_q r0 / dr) / Nt, rounded to complex64.
 *
 * Stages (all work arrays complex64, interleaved re, im):
 *   1          S = rfft(rows, n = Nt): [H W][Nt/2 + 1] (numpy's rfft: unnormalised, exp(-2 pi i ...)).
 *   2 load     Pw[q - q_lo][m][n] = coef[q] S[row(m, n)][q] for m < H, n < W; zero elsewhere in [nq][2H][2W], written
 *              in the same pass.
 *   3          Pf = the 2-D DFT of every image of Pw (numpy's fft2), once.
 *   then per chunk of depth planes j in [j0, j0 + nj):
 *   5 kernel   K[j - j0][q - q_lo][a][b], a in [0, 2H), b in [0, 2W), with the signed offsets a' = a < H ? a : a - 2H
 *              and b' likewise: K = 0 where a' = -H or b' = -W; otherwise
 *                  d = sqrt((a' sz)^2 + (b' sx)^2 + D_j^2),  K = d^e exp(2 pi i frac(g q (d / dr) / Nt))
 *              with (e, g) = (power, 1) without a laser and (power/2, 1/2) with one.
 *   6          Kf = fft2(K).
 *   7 apply    out[j][q] = Kf[j][q] Pf[q], broadcast over j; out may be Kf itself (in place), or disjoint from it.
 *   8          o = ifft2(out), with the 1/(4 H W) normalisation.
 *   9 gather   Phi[n][j][m] = sum_q L_q o[j - j0][q - q_lo][m][n] for m < H, n < W, q ascending, accumulated in fp32.
 *              Without a laser L_q = 1; with one, dl = |(xs[n], ys[j], zs[m]) - laser| and
 *              L_q = dl^(power/2) exp(2 pi i frac(q (dl / dr) / (2 Nt))); the factor dl^(power/2) multiplies the
 *              finished sum once.  planes[0] = Re Phi and planes[1] = Im Phi in the voxel order [W][ny][H] of
 *              nlosgr_voxel_grid, with the transpose nlosgr_fk_store does; mag (or NULL) as nlosgr_backproject_phasor
 *              defines it: (float)sqrt((double)re*re + (double)im*im) of the fp32 planes.
 *
 * Meaning: Phi(x) = sum_p w(x, p) y_p((u(x, p) - r0) / dr), with u the half path (|x - laser| + |x - p|) / 2 (|x - p|
 * for a confocal capture), w the weight of nlosgr_backproject / nlosgr_backproject_nc, and y_p row p filtered with the
 * untruncated Morlet wavelet, band-limited to +-3 sigma_q, evaluated at the continuous bin coordinate and periodic in
 * Nt.  Against nlosgr_backproject_phasor there is no linear interpolation between bins, no +-3 sigma truncation of the
 * taps, and there is the period: Nt must be long enough that no pair's coordinate wraps onto the data (rsd_nt).
 *
 * Arithmetic: d, dl, d^e (one square root and products, rounded to fp32 once) and the turn count g q (d / dr) / Nt are
 * formed in double; only the turn count's fraction goes to fp32 sincospif, as in nlosgr_fk_stolt (the phase reaches
 * thousands of radians).  load and apply are single fp32 complex products.  No atomics; every output element is written
 * by one lane from the inputs alone: bitwise repeatable.
 * Validated on the host before any launch (NLOSGR_E_INVALID, text in the last-error string): H, W or ny outside 1..1024,
 * depth planes leaving [0, ny), Nt odd or outside 2..8192, a band leaving [1, Nt/2 - 1] or of more than 512 frequencies,
 * power outside 0..4, dr, sx or sz <= 0 or not finite, strides that leave [0, H W), a null or misaligned pointer (perm
 * and mag may be NULL; the tables of gather only when there is no laser), a product that aliases the image spectrum or
 * overlaps the kernel spectrum without being it.  r0 enters through coef alone, so r0 < 0 and a depth <= 0 are refused
 * by the caller (nlosgr/rsd.py).  The library neither allocates nor synchronises.
 * ------------------------------------------------------------------------------------- */
NLOSGR_API int nlosgr_rsd_load(const float* spec /* [H W][Nt/2+1][2] */, const int32_t* perm /* [H W] or NULL */,
                    const float* coef /* [nq][2] */, int32_t H, int32_t W, int32_t Nt, int32_t q_lo, int32_t nq,
                    int32_t stride_m, int32_t stride_n, float* pw /* [nq][2H][2W][2] */, void* hip_stream);
NLOSGR_API int nlosgr_rsd_kernel(const float* ys /* [ny] */, int32_t ny, int32_t j0, int32_t nj, float y0, int32_t H,
                    int32_t W, float sx, float sz, float dr, int32_t Nt, int32_t q_lo, int32_t nq, int32_t power,
                    int32_t laser /* 0: confocal */, float* K /* [nj][nq][2H][2W][2], 16-byte aligned */,
                    void* hip_stream);
NLOSGR_API int nlosgr_rsd_apply(const float* kf /* [nj][nq][2H][2W][2] */, const float* pf /* [nq][2H][2W][2] */,
                    int32_t nj, int32_t nq, int32_t H, int32_t W, float* out /* kf, or disjoint from it */,
                    void* hip_stream);
NLOSGR_API int nlosgr_rsd_gather(const float* field /* [nj][nq][2H][2W][2] */, int32_t H, int32_t W, int32_t nq,
                    int32_t q_lo, int32_t Nt, float dr, int32_t power, const float* xs /* [W] */,
                    const float* ys /* [ny] */, const float* zs /* [H] */, int32_t ny, int32_t j0, int32_t nj,
                    int32_t laser /* 0: confocal */, float lx, float ly, float lz,
                    float* planes /* [2][W][ny][H] */, float* mag /* [W][ny][H] or NULL */, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Light-cone transform, LCT (an addition to ABI 13: four new symbols, nothing existing changes): O'Toole, Lindell,
 * Wetzstein 2018.  No counterpart in the reference.  The project's own discretisation, not a port of the published
 * code.  A confocal row obeys
 *     r^3 tau(x', z', r) = integral rho(x, z, sqrt(u)) / (2 sqrt(u)) delta(rho_lat^2 + u - v) dx dz du,   v = r^2,
 * with r the half path: in (x, z, v) a 3-D convolution with a paraboloid, inverted here by a Wiener filter.  It is
 * shift-invariant in v, so a window that starts at any bin needs no special handling.  The FFTs are the caller's (the
 * library links the HIP runtime alone); the four symbols are the passes around them.
 *
 * Input: rows [H W][nr], the lattice, perm, the strides, r0, dr and power as for nlosgr_fk_load; nv: the number of
 * depth-squared cells, 1..2048.  Nz = 2 H, Nx = 2 W, Nv = 2 nv; the work arrays are complex64 [Nz][Nx][Nv],
 * interleaved (re, im).
 *
 * Edges (formed by the caller in double from the fp32 r0 and dr; nlosgr/lct.py lct_resampling): bin j owns
 * r in [e_j, e_j+1), e_j = r0 + (j - 1/2) dr with e_0 clamped at 0;  v_lo = e_0^2, v_hi = e_nr^2, dv = (v_hi - v_lo) / nv;
 * cell i owns r in [t_i, t_i+1), t_i = sqrt(v_lo + i dv), with t_0 = e_0 and t_nv = e_nr exactly.
 *
 * Resampling operator R [nv][nr]:
 *     R[i][j] = |cell i n bin j| / (t_i+1 - t_i) / ((t_i + t_i+1) / 2),
 * the share of cell i inside bin j over the cell's mean radius (the closed form of (1/dv) integral dv / sqrt(v) over the
 * overlap).  Every row and every column holds one contiguous run of non-zeros, nnz <= nv + nr.  It is passed as run
 * tables, rounded to fp32 from double: row i holds weight[start[i] .. start[i+1]) at the bins first[i], first[i] + 1, ...
 * (first [nv], start [nv + 1], weight [nnz]); R^T likewise, per bin j its run of cells (first [nr], start [nr + 1]).
 * The kernels clamp every table entry before use: a bad table reads a wrong bin, never outside an array.
 *
 * Stages:
 *   1 load    psi[v][j] = max(rows[v][j], 0) (r0 + j dr)^power in fp32, the arithmetic of nlosgr_fk_load without
 *             `amplitude`;  g[m][n][i] = sum_j R[i][j] psi[v][j], j ascending, acc = fma(weight, psi, acc) in fp32.
 *             pad = (g, 0) at [0:H][0:W][0:nv] of a zero array; the padding is zero-filled in the same pass.
 *   2 kernel  with signed DFT indices c (z), b (x):  s = ((b sx)^2 + (c sz)^2) / dv in fp64, k = floor(s), f = s - k;
 *                 K[c][b][k] = scale (1 - f) where k <= nv - 1,  K[c][b][k+1] = scale f where k + 1 <= nv - 1,
 *             zero everywhere else (no anticausal half, nothing at or beyond nv), every element written.  scale =
 *             1 / ||K||_2 is the caller's, in double from the same formula over the 2H x 2W columns.
 *   3         Fk = fftn(K), S = fftn(pad) (numpy's fftn: unnormalised, exp(-2 pi i ...)).
 *   4 filter  G = conj(Fk) / (|Fk|^2 + 1 / snr) (mode 0, Wiener), G = conj(Fk) (mode 1, back-projection), or G = the
 *             array itself (mode 2: an inverse built by an earlier call).  spec NULL: out = G (modes 0, 1); otherwise
 *             out = spec G, elementwise.  out may be kf or spec (in place).  G depends on the lattice and the window
 *             alone, so it can be kept for the next capture; both routes give the same bits.
 *   5         o = ifftn(out), with the 1/N normalisation.
 *   6 store   volume[n][j][m] = max(sum_i R[i][j] Re o[m][n][i], 0), i ascending, acc = fma(weight, Re o, acc) in fp32:
 *             [nx = W][ny = nr][nz = H] in the voxel order of nlosgr_voxel_grid; voxel (n, j, m) is the point
 *             (xs[n], y0 + r0 + j dr, zs[m]), as for nlosgr_fk_store.
 * No atomics; every output element is written by one lane in a fixed summation order: bitwise repeatable.
 * Arithmetic: csrc/nlosgr_lct.hip.
 * Validated on the host before any launch (NLOSGR_E_INVALID, text in the last-error string): H, W or nr outside
 * 1..1024, nv outside 1..2048, power outside 0..4, dr <= 0 or not finite, r0 < 0 or not finite, sx, sz, dv, scale or
 * snr <= 0 or not finite, a mode outside 0..2, strides that leave [0, H W), nnz outside 1..nv + nr, a null or misaligned
 * pointer (perm may be NULL; spec in modes 0 and 1), a volume that aliases the field.  The library neither allocates
 * nor synchronises.
 * ------------------------------------------------------------------------------------- */
NLOSGR_API int nlosgr_lct_load(const float* rows /* [H W][nr] */, const int32_t* perm /* [H W] or NULL */, int32_t H,
                    int32_t W, int32_t nr, int32_t nv, int32_t stride_m, int32_t stride_n, float r0, float dr,
                    int32_t power, const int32_t* first /* [nv] */, const int32_t* start /* [nv + 1] */,
                    const float* weight /* [nnz] */, int32_t nnz,
                    float* pad /* [2H][2W][2nv][2], 16-byte aligned */, void* hip_stream);
NLOSGR_API int nlosgr_lct_kernel(int32_t H, int32_t W, int32_t nv, float sx, float sz, double dv, double scale,
                    float* K /* [2H][2W][2nv][2], 16-byte aligned */, void* hip_stream);
NLOSGR_API int nlosgr_lct_filter(const float* kf /* [2H][2W][2nv][2]: Fk, or G in mode 2 */,
                    const float* spec /* the same shape, or NULL */, int32_t H, int32_t W, int32_t nv, float snr,
                    int32_t mode, float* out /* the same shape; all three 16-byte aligned */, void* hip_stream);
NLOSGR_API int nlosgr_lct_store(const float* field /* [2H][2W][2nv][2] */, int32_t H, int32_t W, int32_t nr,
                    int32_t nv, const int32_t* first /* [nr]: the tables of R^T */,
                    const int32_t* start /* [nr + 1] */, const float* weight /* [nnz] */, int32_t nnz,
                    float* volume /* [W][nr][H] */, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * LCT operator pair (an addition to ABI 13: four new symbols, nothing existing changes).  The confocal measurement
 * operator on the lattice and its exact adjoint, built from the parts of the light-cone transform above: R, K and
 * Fk = fftn(K) are the same, T is the [W, nr, H] <-> [H, W, nr] transpose, and nothing is clamped, so both take a
 * residual.
 *
 *     w_j  = (r0 + j dr)^power, power in -4..4: r = fma(j, dr, r0) in fp32, the power by the multiplications of
 *            nlosgr_fk_load, a negative power as one IEEE division 1 / r^|power|, and 0 where r <= 0.
 *     A    : volume [W][nr][H] -> rows [H W][nr]
 *            g[m][n][i]       = sum_j R[i][j] volume[n][j][m]                        nlosgr_lct_load_volume
 *            o                = Re ifftn( fftn(pad g) Fk )                           nlosgr_lct_filter, mode 2, kf = Fk
 *            rows[v(m,n)][j]  = w_j sum_i R[i][j] o[m][n][i]                         nlosgr_lct_store_rows
 *     A^T  : rows -> volume
 *            g[m][n][i]       = sum_j R[i][j] (w_j rows[v][j])                       nlosgr_lct_load_rows
 *            o                = Re ifftn( fftn(pad g) conj(Fk) )                     nlosgr_lct_filter, mode 1
 *            volume[n][j][m]  = sum_i R[i][j] o[m][n][i]                             nlosgr_lct_store_volume
 *
 * v(m, n) = perm[m stride_m + n stride_n] as in nlosgr_lct_load.  <A v, h> = <v, A^T h> holds for the float64
 * restatement to rounding.  With power = -3, A is the physical confocal transient of forward_project at power -4 up to
 * the factor dv / (2 dr scale) per unit voxel value (scale: nlosgr_lct_kernel's; R carries one 1 / r).
 *
 *   load_volume   j ascending, acc = fma(weight, volume, acc) in fp32; every element of pad is written, the zeros for
 *                 m >= H, n >= W and i >= nv included.  first/start/weight: the tables of R.
 *   store_rows    i ascending, acc = fma(weight, Re field, acc), then one multiply by w_j; signed.  Reads the
 *                 [0:H][0:W][0:nv] corner of field only.  Rows that no lattice point names are left untouched.
 *                 first/start/weight: the tables of R^T.
 *   load_rows     nlosgr_lct_load with psi = rows[v][j] w_j, no clamp, power -4..4.  For power 0..4 and rows >= 0 the
 *                 bits of nlosgr_lct_load.
 *   store_volume  nlosgr_lct_store without the clamp.  Where the sum is >= 0 the bits of nlosgr_lct_store.
 * No atomics, one writer per element in a fixed order: bitwise repeatable.  Table entries are clamped as above.
 * Validated on the host before any launch as the four passes above, with power in -4..4 for load_rows and store_rows;
 * pad and field must be 8-byte aligned (16 for load_rows), and no output may alias its input.
 * ------------------------------------------------------------------------------------- */
NLOSGR_API int nlosgr_lct_load_volume(const float* volume /* [W][nr][H] */, int32_t H, int32_t W, int32_t nr,
                    int32_t nv, const int32_t* first /* [nv] */, const int32_t* start /* [nv + 1] */,
                    const float* weight /* [nnz] */, int32_t nnz, float* pad /* [2H][2W][2nv][2] */,
                    void* hip_stream);
NLOSGR_API int nlosgr_lct_store_rows(const float* field /* [2H][2W][2nv][2] */, const int32_t* perm /* [H W] or NULL */,
                    int32_t H, int32_t W, int32_t nr, int32_t nv, int32_t stride_m, int32_t stride_n, float r0,
                    float dr, int32_t power, const int32_t* first /* [nr]: the tables of R^T */,
                    const int32_t* start /* [nr + 1] */, const float* weight /* [nnz] */, int32_t nnz,
                    float* rows /* [H W][nr] */, void* hip_stream);
NLOSGR_API int nlosgr_lct_load_rows(const float* rows /* [H W][nr] */, const int32_t* perm /* [H W] or NULL */,
                    int32_t H, int32_t W, int32_t nr, int32_t nv, int32_t stride_m, int32_t stride_n, float r0,
                    float dr, int32_t power, const int32_t* first /* [nv] */, const int32_t* start /* [nv + 1] */,
                    const float* weight /* [nnz] */, int32_t nnz,
                    float* pad /* [2H][2W][2nv][2], 16-byte aligned */, void* hip_stream);
NLOSGR_API int nlosgr_lct_store_volume(const float* field /* [2H][2W][2nv][2] */, int32_t H, int32_t W, int32_t nr,
                    int32_t nv, const int32_t* first /* [nr]: the tables of R^T */,
                    const int32_t* start /* [nr + 1] */, const float* weight /* [nnz] */, int32_t nnz,
                    float* volume /* [W][nr][H] */, void* hip_stream);

/* ---------------------------------------------------------------------------------------
 * Primal-dual passes (an addition to ABI 13: five new symbols, nothing existing changes).  The three passes of one
 * Chambolle-Pock iteration (theta = 1) that are not an application of the operator, for
 *
 *     minimise over v (>= 0 with nonneg)   F(A v) + tv sum_voxels |a o grad v|_2 + l1 sum |v|
 *
 * on a volume [W][nr][H], axes (n, j, m), with rows [H W][nr]; A and A^T are the caller's (the LCT operator pair
 * above).  With x the iterate, xbar the extrapolated point, q [H W][nr] the row dual and p [3][W][nr][H] the TV dual
 * (component 0: n, 1: j, 2: m), one iteration is
 *
 *     z = A xbar;   q <- prox_{sigma F*}(q + sigma z)                       nlosgr_prox_rows
 *                   p <- project_{|p|_2 <= tv}(p + sigma a o grad xbar)     nlosgr_tv_dual
 *     g = A^T q;    u = x - tau (g + (a o grad)^T p)
 *                   x+ = max(u - tau l1, 0) (nonneg), sign(u) max(|u| - tau l1, 0) (otherwise)
 *                   xbar <- 2 x+ - x;  x <- x+                              nlosgr_tv_primal
 *
 * Gradient.  Forward differences in index units, axis k scaled by a_k >= 0 (a_n, a_j, a_m), 0 at the last index of
 * an axis (Neumann; an axis of extent 1 contributes nothing):
 *     (a o grad v)_k[i] = a_k (v[i + e_k] - v[i])  where i_k < N_k - 1, else 0        fp32: one subtraction, one product
 * and its exact transpose, which never reads p_k at the last index of axis k:
 *     t_k[i] = a_k ( (i_k > 0 ? p_k[i - e_k] : 0) - (i_k < N_k - 1 ? p_k[i] : 0) )    fp32: one subtraction, one product
 *     ((a o grad)^T p)[i] = (t_n + t_j) + t_m                                          in this order
 * Dual pass, per voxel, one fp32 operation each and no contraction beyond the fma written:
 *     u_k = fma(sigma, (a o grad xbar)_k, p_k);   n = sqrtf(fma(u_2, u_2, fma(u_1, u_1, u_0 u_0)))
 *     p = u where n <= tv, else p_k = u_k (tv / n) with one IEEE division; tv = 0 writes zeros; tv = +inf never
 *     projects (with p = 0 and sigma = 1 the pass is then the plain gradient).
 * Primal pass, per voxel:
 *     w = g + ((t_n + t_j) + t_m);  u = fma(-tau, w, x);  c = tau l1 (one fp32 product, formed once)
 *     x+ = max(u - c, 0) with nonneg, copysign(max(|u| - c, 0), u) otherwise;  xbar = fma(2, x+, -x);  x = x+
 * Rows pass, per element, u = fma(sigma, z, q), with h the target rows and e an optional exposure table [nr], finite
 * and >= 0 (NULL: every entry 1), d = e_j:
 *     NLOSGR_LOSS_MSE      F(z) = 1/2 sum (z - h)^2;  q = fma(-sigma, h, u) / (1 + sigma)  (1 + sigma formed once in
 *                          fp32).  The exposure must be NULL; gt_times and rate_floor are ignored.
 *     NLOSGR_LOSS_POISSON  y' = max(gt_times h, 0) + eps and rho = d z + eps, eps = rate_floor > 0: the y', rho and
 *                          eps of nlosgr_loss_irf;  F(z) = sum [rho - y' + y' log(y'/rho)], half its deviance.
 *                          d = 0, or d so small that d d is 0 in fp32 (d < 2^-75, about 2.6e-23):  q = 0.
 *                          A non-zero d must keep s and 4 sp y' below 2^63 in magnitude (about d >= 1e-9 sqrt(sigma y'));
 *                          below that the squares overflow and q is not meaningful (it may be NaN).  Otherwise
 *                            sp = sigma / (d d) (d d formed once);  s = fma(sp, eps, u / d);  A = s - 1;  c = (4 sp) y';
 *                            D = sqrtf(fma(A, A, c));  den = (2 + A) + D where A > 0, else 2 + c / (D - A);
 *                            q = d ( 2 fma(-sp, y', s) / den )
 *                          This is q = d 2 (s - sp y') / (1 + s + D), the cancellation-free form of d (1 + s - D) / 2.
 *                          Its denominator 1 + s + D = 2 + A + D is >= 2, but for A <= 0 the sum A + D is itself a
 *                          difference that loses ulp(|s|) / 2 of q in fp32 (every digit from s = -2^25 on); there it
 *                          is formed as c / (D - A), a sum of non-negative terms.  q < d, so nothing is clamped.
 * Objective.  Each dual pass emits its term at the point the operator was applied to, formed in double from the fp32
 * inputs: the rows pass F(z) (Poisson: with rho = max(d z, 0) + eps, as y' (t - log1p(t)), t = (rho - y') / y'), the
 * dual pass sum sqrt(fma(g_m, g_m, fma(g_j, g_j, g_n g_n))) of the double gradient of xbar and sum |xbar|.  Each
 * workgroup writes its own partial(s) in double: partials [nlosgr_prox_rows_partials] for the rows pass,
 * [nlosgr_tv_dual_partials] = [workgroups][2] (TV, L1) for the dual pass; the caller adds them in a fixed order.
 * One launch per pass, everything in place, one writer per element, no atomics: bitwise repeatable.
 * Validated on the host before any launch (NLOSGR_E_INVALID): extents in 1..1024; sigma and tau finite and > 0;
 * tv >= 0 or +inf; l1 and the axis weights finite and >= 0; rate_floor finite and > 0 (Poisson); an unknown kind; an
 * exposure with the MSE; null pointers; and the aliasing the in-place scheme forbids (x with xbar, xbar with p, g with
 * x or xbar, p with x, z, h or the exposure table with q, the partials with any array of their pass).  The size queries return 0 for extents out of range.
 * ------------------------------------------------------------------------------------- */
NLOSGR_API size_t nlosgr_prox_rows_partials(int32_t H, int32_t W, int32_t nr);
NLOSGR_API int nlosgr_prox_rows(const float* z /* [H W][nr] */, const float* h /* [H W][nr] */,
                    const float* exposure /* [nr] or NULL */, int32_t H, int32_t W, int32_t nr,
                    int32_t kind /* NLOSGR_LOSS_* */, float gt_times, float rate_floor, float sigma,
                    float* q /* [H W][nr], in place */, double* partials, void* hip_stream);
NLOSGR_API size_t nlosgr_tv_dual_partials(int32_t W, int32_t nr, int32_t H);
NLOSGR_API int nlosgr_tv_dual(const float* xbar /* [W][nr][H] */, int32_t W, int32_t nr, int32_t H, float a_n, float a_j,
                    float a_m, float sigma, float tv, float* p /* [3][W][nr][H], in place */, double* partials,
                    void* hip_stream);
NLOSGR_API int nlosgr_tv_primal(const float* g /* [W][nr][H] */, const float* p /* [3][W][nr][H] */, int32_t W,
                    int32_t nr, int32_t H, float a_n, float a_j, float a_m, float tau, float l1, int32_t nonneg,
                    float* x /* [W][nr][H], in place */, float* xbar /* [W][nr][H], written */, void* hip_stream);

NLOSGR_API const char* nlosgr_last_error(void);
NLOSGR_API int nlosgr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NLOSGR_H */
