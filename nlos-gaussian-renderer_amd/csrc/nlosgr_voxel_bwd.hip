// Backward of the voxelizer (gfx950): dL/d(raw Gaussian parameters) from dL/d density and dL/d albedo_density.
//
// With G_d, G_a the upstream volumes, sigma, rho, w = sigma rho of a Gaussian, d = x - mu, p = exp(-d^T N d / 2)
// and c(x) = sigma G_d(x) + w G_a(x), the sums over the Gaussian's support
//     P_d = sum G_d p,  P_a = sum G_a p,  M1 = sum c p d,  M2 = sum c p d d^T
// give  dL/dsigma = P_d + rho P_a,  dL/drho = sigma P_a,  dL/dmu (direct) = N M1,  dL/dA = -A M2.
//
// Contract: a (voxel, Gaussian) pair is in the backward iff it is in the forward: the box is the forward's
// VoxAux, the exponent is eval_batch's fmaf sequence compared with the same thr, and a pair outside drops out
// by a select (a NaN upstream outside a Gaussian's support does not reach it).  A Gaussian's rows depend on
// that Gaussian, the grid, cam, the cutoff and the upstream alone: no atomics, a summation order fixed by the
// box, so two runs are bitwise equal and permuting the Gaussians permutes the rows.
//
// Pipeline (caller's stream, scratch in the caller's workspace):
//   preprocess_kernel, voxel_aux_kernel   (shared with the forward)
//   voxel_bwd_kernel     one wave per Gaussian, four per workgroup, no workgroup barrier.  Lanes stride over
//                        the box's voxels, z fastest; 11 fp32 accumulators per lane, each one fmaf chain; a
//                        fixed xor butterfly; lane 0 writes the Gaussian's 11 sums.
//   voxel_bwd_wide_kernel  the boxes of more than 2^18 voxels, which the kernel above leaves out (one wave would
//                        walk a grid-covering Gaussian alone): a 1024-thread workgroup walks such a box with all
//                        its threads and adds its 16 waves' sums in wave order.  Which kernel takes a Gaussian is
//                        a function of its box alone, so the rows stay independent of everything else.
//   voxel_bwd_finish     one lane per Gaussian: the whitened second moment W = A M2 A^T feeds the shape form
//                        of the chain (chain_to_raw_shape: the rotation sees only W's off-diagonals times the
//                        scale-ratio differences, never the symmetric bulk), the rest is albedo_chain.
#include "nlosgr_voxel.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

constexpr int kWideVox = 1 << 18;       // a box of more voxels (64^3) is walked by a whole workgroup
constexpr int kWideWaves = 16;
constexpr int kWideBlock = 64 * kWideWaves;
constexpr int kSums = 12;   // floats per Gaussian in the workspace: P_d, P_a, M1[3], M2[6] (xx xy xz yy yz zz), pad

struct BArgs {
    const GaussRec* recs;
    const VoxAux* aux;
    int ng;
    int nx, ny, nz;
    const float *xs, *ys, *zs;
    float thr;         // as the forward's: a pair is in support when its exponent is >= thr
    const float* gd;   // dL/d density (may be null)
    const float* ga;   // dL/d albedo_density (may be null)
    float* sums;       // [ng][kSums]
};

// a Gaussian's box: first voxel and extents per axis (the whole grid in dense mode); false when it is empty
template <bool DENSE>
__device__ __forceinline__ bool box_of(const BArgs& k, int gi, int& x0, int& y0, int& z0, int& ex, int& ey, int& ez) {
    x0 = y0 = z0 = 0;
    ex = k.nx; ey = k.ny; ez = k.nz;
    if (DENSE) return true;
    const VoxAux a = k.aux[gi];
    if (a.bx == kEmptyBox) return false;
    x0 = (int)(a.bx & 0xFFFFu); ex = (int)(a.bx >> 16) - x0 + 1;
    y0 = (int)(a.by & 0xFFFFu); ey = (int)(a.by >> 16) - y0 + 1;
    z0 = (int)(a.bz & 0xFFFFu); ez = (int)(a.bz >> 16) - z0 + 1;
    return true;
}

// The 11 sums of Gaussian gi over the voxels tid, tid + STRIDE, ... of its box (flat index, z fastest), each lane
// one fmaf chain per sum, then the fixed butterfly over the wave: every lane returns its wave's 11 sums.
template <bool DENSE, int STRIDE>
__device__ __forceinline__ void box_sums(const BArgs& k, int gi, int tid, int x0, int y0, int z0, int ex, int ey, int ez,
                                         float* acc) {
    // the forward's batch entry (stage_entry): n = -log2(e)/2 N, off-diagonals doubled
    const float4 p = k.recs[gi].a, d4 = k.recs[gi].d, e4 = k.recs[gi].e;
    const float k1 = -kHalfLog2e, k2 = -2.0f * kHalfLog2e;
    const float4 q = make_float4(k1 * d4.z, k2 * d4.w, k2 * e4.x, k1 * e4.y);
    const float rx = k2 * e4.z, ry = k1 * e4.w;
    const float sigma = p.w, w = k.aux[gi].w;
    const int cnt = ex * ey * ez;   // < 2^31 (validated)
    // the lane's voxel as mixed-radix digits (ix, iy, iz) of its flat box index, advanced by STRIDE per step
    int iz = tid % ez, iy = (tid / ez) % ey, ix = tid / (ez * ey);
    const int sz = STRIDE % ez, sy = (STRIDE / ez) % ey, sx = STRIDE / (ez * ey);
    for (int idx = tid; idx < cnt; idx += STRIDE) {
        const float x = k.xs[x0 + ix], y = k.ys[y0 + iy], z = k.zs[z0 + iz];
        const size_t o = ((size_t)(x0 + ix) * k.ny + (y0 + iy)) * k.nz + (z0 + iz);
        float gd = k.gd ? k.gd[o] : 0.f;
        float ga = k.ga ? k.ga[o] : 0.f;
        const float dx = x - p.x, dy = y - p.y, dz = z - p.z;
        // eval_batch's exponent
        const float t = fmaf(dy, fmaf(rx, dz, q.w * dy), (ry * dz) * dz);
        const float s = fmaf(q.z, dz, q.y * dy);
        const float e0 = fmaf(dx, fmaf(q.x, dx, s), t);
        float pv = fast_exp2(e0);
        if (!DENSE) {
            const bool in = e0 >= k.thr;
            pv = in ? pv : 0.0f;
            gd = in ? gd : 0.0f;
            ga = in ? ga : 0.0f;
        }
        const float cp = fmaf(sigma, gd, w * ga) * pv;
        acc[0] = fmaf(gd, pv, acc[0]);
        acc[1] = fmaf(ga, pv, acc[1]);
        const float cx = cp * dx, cy = cp * dy, cz = cp * dz;
        acc[2] = fmaf(cp, dx, acc[2]);
        acc[3] = fmaf(cp, dy, acc[3]);
        acc[4] = fmaf(cp, dz, acc[4]);
        acc[5] = fmaf(cx, dx, acc[5]);
        acc[6] = fmaf(cx, dy, acc[6]);
        acc[7] = fmaf(cx, dz, acc[7]);
        acc[8] = fmaf(cy, dy, acc[8]);
        acc[9] = fmaf(cy, dz, acc[9]);
        acc[10] = fmaf(cz, dz, acc[10]);
        iz += sz;
        if (iz >= ez) { iz -= ez; ++iy; }
        iy += sy;
        if (iy >= ey) { iy -= ey; ++ix; }
        ix += sx;
    }
#pragma unroll
    for (int t = 0; t < 11; ++t)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[t] += __shfl_xor(acc[t], off);
}

// boxes of up to kWideVox voxels: one wave per Gaussian (a wider box is left to voxel_bwd_wide_kernel)
template <bool DENSE>
__global__ __launch_bounds__(kBlock) void voxel_bwd_kernel(BArgs k) {
    const int lane = lane_id();
    const int gi = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (gi >= k.ng) return;   // waves never meet at a barrier
    int x0, y0, z0, ex, ey, ez;
    const bool some = box_of<DENSE>(k, gi, x0, y0, z0, ex, ey, ez);
    if (some && ex * ey * ez > kWideVox) return;
    float acc[11];
#pragma unroll
    for (int t = 0; t < 11; ++t) acc[t] = 0.f;
    if (some) box_sums<DENSE, 64>(k, gi, lane, x0, y0, z0, ex, ey, ez, acc);
    if (lane == 0) {
        float* o = k.sums + (size_t)gi * kSums;
#pragma unroll
        for (int t = 0; t < 11; ++t) o[t] = acc[t];
        o[11] = 0.f;
    }
}

// boxes of more than kWideVox voxels: a workgroup of kWideWaves waves owns kWideWaves consecutive Gaussians and walks
// each wide one among them with all its threads (stride kWideBlock), then adds the waves' sums in wave order
template <bool DENSE>
__global__ __launch_bounds__(kWideBlock) void voxel_bwd_wide_kernel(BArgs k) {
    __shared__ float s_part[kWideWaves][kSums];
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int j = 0; j < kWideWaves; ++j) {
        const int gi = blockIdx.x * kWideWaves + j;
        if (gi >= k.ng) break;                       // workgroup-uniform
        int x0, y0, z0, ex, ey, ez;
        const bool some = box_of<DENSE>(k, gi, x0, y0, z0, ex, ey, ez);
        if (!some || ex * ey * ez <= kWideVox) continue;   // workgroup-uniform: every thread reads the same box
        float acc[11];
#pragma unroll
        for (int t = 0; t < 11; ++t) acc[t] = 0.f;
        box_sums<DENSE, kWideBlock>(k, gi, tid, x0, y0, z0, ex, ey, ez, acc);
        if ((tid & 63) == 0) {
#pragma unroll
            for (int t = 0; t < 11; ++t) s_part[wave][t] = acc[t];
        }
        __syncthreads();
        if (tid < kSums) {
            float v = 0.f;
            if (tid < 11)
                for (int wv = 0; wv < kWideWaves; ++wv) v += s_part[wv][tid];
            k.sums[(size_t)gi * kSums + tid] = v;
        }
        __syncthreads();
    }
}

template <int PRESET>
__global__ __launch_bounds__(kBlock) void voxel_bwd_finish(nlosgr_gaussians g, BArgs k, const float* __restrict__ cam,
                                                          int culled, float* d_mu, float* d_scaling, float* d_rot,
                                                          float* d_opac, float* d_feat) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.ng) return;
    const int kf = g.k_feat;
    if (culled && k.aux[i].bx == kEmptyBox) {   // no voxel in the box, or a non-finite box: skipped, as the forward
        for (int c = 0; c < 3; ++c) d_mu[3 * i + c] = d_scaling[3 * i + c] = 0.f;
        for (int c = 0; c < 4; ++c) d_rot[4 * i + c] = 0.f;
        d_opac[i] = 0.f;
        for (int c = 0; c < kf; ++c) d_feat[(size_t)i * kf + c] = 0.f;
        return;
    }
    const float* S = k.sums + (size_t)i * kSums;
    const GaussRec rec = k.recs[i];
    const float A[9] = {rec.b.x, rec.b.y, rec.b.z, rec.b.w, rec.c.x, rec.c.y, rec.c.z, rec.c.w, rec.d.x};
    const float N[9] = {rec.d.z, rec.d.w, rec.e.x, rec.d.w, rec.e.y, rec.e.z, rec.e.x, rec.e.z, rec.e.w};
    const float M[9] = {S[5], S[6], S[7], S[6], S[8], S[9], S[7], S[9], S[10]};
    // the albedo as voxel_aux_kernel forms it
    float dx, dy, dz, nrm;
    view_dir<PRESET>(rec.a.x - cam[0], rec.a.y - cam[1], rec.a.z - cam[2], dx, dy, dz, nrm);
    const float sh = sh_dot<PRESET>(g.sh_degree, dx, dy, dz, g.features + (size_t)i * kf);
    const float rho = fmaxf(sh + 0.5f, 0.0f);
    const float dsig = S[0] + rho * S[1];
    const float drho = rec.a.w * S[1];
    float dmu[3];
    for (int r = 0; r < 3; ++r) dmu[r] = N[3 * r] * S[2] + N[3 * r + 1] * S[3] + N[3 * r + 2] * S[4];
    albedo_chain<PRESET, kMaxK4>(g, i, cam, sh, dmu, dsig, drho, d_mu, d_opac, d_feat);
    // dL/dA = -A M2 is a sum of outer products (-c p u) d^T with u = A d, so in shape_acc's terms g = -c p u,
    // w = u: D_r = -W_rr and K~ = -(ratio differences) x W's off-diagonals, W = A M2 A^T
    float T[9], W[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T[3 * r + c] = A[3 * r] * M[c] + A[3 * r + 1] * M[3 + c] + A[3 * r + 2] * M[6 + c];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) W[3 * r + c] = T[3 * r] * A[3 * c] + T[3 * r + 1] * A[3 * c + 1] + T[3 * r + 2] * A[3 * c + 2];
    // the ratio differences r3 - r2, 1 - r3, r2 - 1 (r = scale_ratios) from the differences of A's squared row
    // norms, so an isotropic Gaussian's are exactly zero and a nearly isotropic one's keep their digits
    const float n1 = A[0] * A[0] + A[1] * A[1] + A[2] * A[2];
    const float n2 = A[3] * A[3] + A[4] * A[4] + A[5] * A[5];
    const float n3 = A[6] * A[6] + A[7] * A[7] + A[8] * A[8];
    const float d32 = n1 * (n2 - n3) / (n2 * n3), d13 = (n3 - n1) / n3, d21 = (n1 - n2) / n2;
    const float D[3] = {-W[0], -W[4], -W[8]};
    const float w23 = 0.5f * (W[5] + W[7]), w31 = 0.5f * (W[2] + W[6]), w12 = 0.5f * (W[1] + W[3]);
    const float K[3] = {-d32 * w23, -d13 * w31, -d21 * w12};
    chain_to_raw_shape<PRESET>(g, i, D, K, d_scaling, d_rot);
}

// workspace: GaussRec [ng] | VoxAux [ng] | sums [ng][kSums]
struct BwdLayout {
    size_t off_recs, off_aux, off_sums, total;
    explicit BwdLayout(int ng) {
        off_recs = 0;
        off_aux = off_recs + align_up((size_t)ng * sizeof(GaussRec));
        off_sums = off_aux + align_up((size_t)ng * sizeof(VoxAux));
        total = off_sums + align_up((size_t)ng * kSums * sizeof(float)) + 256;
    }
};

}  // namespace

extern "C" {

size_t nlosgr_voxel_bwd_workspace_bytes(const nlosgr_gaussians* g, const nlosgr_voxel_grid* grid,
                                        const nlosgr_options* opt) {
    if (validate_voxel(g, grid, opt) != NLOSGR_OK) return 0;
    return BwdLayout(g->ng).total;
}

int nlosgr_voxelize_bwd(const nlosgr_gaussians* g, const nlosgr_voxel_grid* grid, const float* cam,
                        const nlosgr_options* opt, void* workspace, const float* grad_density,
                        const float* grad_albedo, float* d_mu, float* d_scaling, float* d_rotation, float* d_opacity,
                        float* d_features, void* hip_stream) {
    const int rc = validate_voxel(g, grid, opt);
    if (rc) return rc;
    if (!cam) return set_err(NLOSGR_E_INVALID, "null camera position");
    if (g->ng == 0) return NLOSGR_OK;
    if (!d_mu || !d_scaling || !d_rotation || !d_opacity || !d_features)
        return set_err(NLOSGR_E_INVALID, "null gradient output pointer");
    if (!workspace) return set_err(NLOSGR_E_INVALID, "null workspace");
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t ng = (size_t)g->ng;
    if (!grad_density && !grad_albedo) {
        HIPCHK(hipMemsetAsync(d_mu, 0, ng * 3 * sizeof(float), s));
        HIPCHK(hipMemsetAsync(d_scaling, 0, ng * 3 * sizeof(float), s));
        HIPCHK(hipMemsetAsync(d_rotation, 0, ng * 4 * sizeof(float), s));
        HIPCHK(hipMemsetAsync(d_opacity, 0, ng * sizeof(float), s));
        HIPCHK(hipMemsetAsync(d_features, 0, ng * g->k_feat * sizeof(float), s));
        return NLOSGR_OK;
    }
    const BwdLayout L(g->ng);
    char* ws = (char*)workspace;
    GaussRec* recs = (GaussRec*)(ws + L.off_recs);
    VoxAux* aux = (VoxAux*)(ws + L.off_aux);
    const bool dense = !(opt->cutoff > 0.0f);

    launch_preprocess(g, recs, s);
    launch_voxel_aux(g, recs, cam, grid, opt->cutoff, aux, s);
    BArgs k;
    k.recs = recs; k.aux = aux; k.ng = g->ng;
    k.nx = grid->nx; k.ny = grid->ny; k.nz = grid->nz;
    k.xs = grid->xs; k.ys = grid->ys; k.zs = grid->zs;
    k.thr = dense ? 0.0f : -kHalfLog2e * opt->cutoff * opt->cutoff;
    k.gd = grad_density; k.ga = grad_albedo;
    k.sums = (float*)(ws + L.off_sums);
    const unsigned nwg = (unsigned)((g->ng + kWaves - 1) / kWaves);
    if (dense) hipLaunchKernelGGL(voxel_bwd_kernel<true>, dim3(nwg), dim3(kBlock), 0, s, k);
    else hipLaunchKernelGGL(voxel_bwd_kernel<false>, dim3(nwg), dim3(kBlock), 0, s, k);
    if ((long long)grid->nx * grid->ny * grid->nz > kWideVox) {   // else no box can be wide
        const unsigned nww = (unsigned)((g->ng + kWideWaves - 1) / kWideWaves);
        if (dense) hipLaunchKernelGGL(voxel_bwd_wide_kernel<true>, dim3(nww), dim3(kWideBlock), 0, s, k);
        else hipLaunchKernelGGL(voxel_bwd_wide_kernel<false>, dim3(nww), dim3(kWideBlock), 0, s, k);
    }
    const unsigned nbg = (unsigned)((g->ng + kBlock - 1) / kBlock);
    if (g->preset == NLOSGR_PRESET_TORCH)
        hipLaunchKernelGGL(voxel_bwd_finish<NLOSGR_PRESET_TORCH>, dim3(nbg), dim3(kBlock), 0, s, *g, k, cam, (int)!dense,
                           d_mu, d_scaling, d_rotation, d_opacity, d_features);
    else
        hipLaunchKernelGGL(voxel_bwd_finish<NLOSGR_PRESET_CUDA>, dim3(nbg), dim3(kBlock), 0, s, *g, k, cam, (int)!dense,
                           d_mu, d_scaling, d_rotation, d_opacity, d_features);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

}  // extern "C"
