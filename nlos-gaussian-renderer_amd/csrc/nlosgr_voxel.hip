// Gaussian-to-voxel reconstruction output (gfx950): the two sums of the reference's
// estimate_rho_w_no_occlusion(out_separately=True) (gaussian_model/gaussian_model.py:346-364) on a regular
// voxel grid, which is what gaussian2volume (nlos_helpers.py:40-69) evaluates for evaluation()
// (main.py:374-387), and maximum projections of such a volume.
//
//     density(x) = sum_g sigma_g pdf_g(x),   albedo_density(x) = sum_g sigma_g rho_g(cam) pdf_g(x)
//
// Contract: every voxel's sums are formed in ascending Gaussian-index order, without atomics, by an
// expression that depends on the voxel's table coordinates and the Gaussian alone (explicit fmaf, no
// contraction choices left to the compiler).  A Gaussian the culling keeps but the exact mask rejects adds
// +0, so the outputs are bitwise repeatable and independent of how the grid is cut into bricks.
//
// Pipeline (all on the caller's stream, scratch in the caller's workspace):
//   preprocess_kernel   (shared)   raw parameters -> GaussRec (mu, sigma, N = A^T A)
//   voxel_aux_kernel    per Gaussian: w = sigma rho(cam) and the cutoff box as inclusive voxel index ranges
//                       (nlosgr_voxel.hpp: the backward, nlosgr_voxel_bwd.hip, takes its support from the same box)
//   voxel_bin_kernel    level 1: per super-brick (32^3 voxels) one ballot word per 64 Gaussians, index order
//   voxel_eval_kernel   level 2 + evaluation: a workgroup owns one 8x8x8 brick, 2 voxels per lane, z fastest.
//                       Each wave owns a 2x8x8 slab of the brick and is self-contained (no workgroup
//                       barrier): it expands its super-brick's words into an ordered candidate list, tests
//                       the candidates' boxes against its slab, compacts the survivors with mbcnt prefixes
//                       into an LDS batch (index order by construction) and evaluates the batch from
//                       same-address LDS broadcasts.  LDS use does not depend on ng.
//   cutoff <= 0: no culling, every wave streams all Gaussians through its batch.
#include "nlosgr_voxel.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

constexpr int kBrick = 8;                   // brick edge (voxels); a workgroup evaluates one brick
constexpr int kSuperBricks = 4;             // bricks per super-brick edge
constexpr int kSuper = kBrick * kSuperBricks;   // super-brick edge (voxels)
constexpr int kSlab = kBrick / kWaves;      // x extent of a wave's slab (2: the two voxels of a lane)
constexpr int kBatch = 64;                  // LDS batch entries per wave
constexpr int kCand = 256;                  // candidate window per wave
constexpr int kMaxExtent = kVoxMaxExtent;

static_assert(kSlab == 2, "a lane evaluates the two x positions of its wave's slab");

struct VArgs {
    const GaussRec* recs;
    const VoxAux* aux;
    const unsigned long long* words;   // [nsb][nwords] level-1 hit words (culled mode)
    int ng, nwords;
    int nx, ny, nz;
    const float *xs, *ys, *zs;
    int nby, nbz;      // bricks along y, z
    int nsby, nsbz;    // super-bricks along y, z
    float thr;         // -log2(e)/2 cutoff^2: a sample is in support when its exponent is >= thr
    float* dens;
    float* alb;
};

__device__ __forceinline__ bool overlaps(uint32_t box, int lo, int hi) {
    return (int)(box & 0xFFFFu) <= hi && (int)(box >> 16) >= lo;
}

// level 1: words[sb][word] = ballot over the word's 64 Gaussians of "box overlaps super-brick sb"
__global__ __launch_bounds__(kBlock) void voxel_bin_kernel(const VoxAux* __restrict__ aux, int ng, int nwords,
                                                          int nsbx, int nsby, int nsbz,
                                                          unsigned long long* __restrict__ words) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int word = i >> 6;
    VoxAux a;
    a.bx = a.by = a.bz = kEmptyBox;
    if (i < ng) a = aux[i];
    const int nsb = nsbx * nsby * nsbz;
    for (int sb = blockIdx.y; sb < nsb; sb += gridDim.y) {
        const int sz = sb % nsbz, sy = (sb / nsbz) % nsby, sx = sb / (nsbz * nsby);
        const bool hit = overlaps(a.bx, sx * kSuper, sx * kSuper + kSuper - 1) &&
                         overlaps(a.by, sy * kSuper, sy * kSuper + kSuper - 1) &&
                         overlaps(a.bz, sz * kSuper, sz * kSuper + kSuper - 1);
        const unsigned long long m = __ballot(hit);
        if (lane_id() == 0 && word < nwords) words[(size_t)sb * nwords + word] = m;
    }
}

// batch entry: 3 float4 = (mu.xyz, sigma), (n00, n01, n02, n11), (n12, n22, w, -) with
// n = -log2(e)/2 N, off-diagonals doubled: the exponent of exp2 is d^T n d
__device__ __forceinline__ void stage_entry(float4* slot, const GaussRec* __restrict__ recs,
                                            const VoxAux* __restrict__ aux, int gi) {
    const float4 a = recs[gi].a, d = recs[gi].d, e = recs[gi].e;
    const float k1 = -kHalfLog2e, k2 = -2.0f * kHalfLog2e;
    slot[0] = a;
    slot[1] = make_float4(k1 * d.z, k2 * d.w, k2 * e.x, k1 * e.y);
    slot[2] = make_float4(k2 * e.z, k1 * e.w, aux[gi].w, 0.f);
}

// adds batch entries [0, n) to the lane's two voxels (x0, y, z) and (x1, y, z), in entry order
template <bool DENSE>
__device__ __forceinline__ void eval_batch(const float4* b, int n, float x0, float x1, float y, float z, float thr,
                                           float& d0, float& a0, float& d1, float& a1) {
    n = __builtin_amdgcn_readfirstlane(n);   // wave-uniform by construction
    for (int e = 0; e < n; ++e) {
        const float4 p = b[3 * e], q = b[3 * e + 1], r = b[3 * e + 2];
        const float dy = y - p.y, dz = z - p.z;
        const float t = fmaf(dy, fmaf(r.x, dz, q.w * dy), (r.y * dz) * dz);
        const float s = fmaf(q.z, dz, q.y * dy);
        const float dx0 = x0 - p.x, dx1 = x1 - p.x;
        const float e0 = fmaf(dx0, fmaf(q.x, dx0, s), t);
        const float e1 = fmaf(dx1, fmaf(q.x, dx1, s), t);
        float p0 = fast_exp2(e0), p1 = fast_exp2(e1);
        if (!DENSE) {
            p0 = e0 >= thr ? p0 : 0.0f;
            p1 = e1 >= thr ? p1 : 0.0f;
        }
        d0 = fmaf(p.w, p0, d0);
        a0 = fmaf(r.z, p0, a0);
        d1 = fmaf(p.w, p1, d1);
        a1 = fmaf(r.z, p1, a1);
    }
}

template <bool DENSE>
__global__ __launch_bounds__(kBlock) void voxel_eval_kernel(VArgs k) {
    __shared__ float4 s_batch[kWaves][kBatch * 3];
    __shared__ uint32_t s_cand[kWaves][kCand];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int bz = blockIdx.x % k.nbz, by = (blockIdx.x / k.nbz) % k.nby, bx = blockIdx.x / (k.nbz * k.nby);
    const int ix0 = bx * kBrick + wave * kSlab;
    if (ix0 >= k.nx) return;   // whole slab outside the grid (waves never meet at a barrier)
    const int iy = by * kBrick + (lane >> 3), iz = bz * kBrick + (lane & 7);
    const float x0 = k.xs[ix0], x1 = k.xs[min(ix0 + 1, k.nx - 1)];
    const float y = k.ys[min(iy, k.ny - 1)], z = k.zs[min(iz, k.nz - 1)];
    float4* batch = s_batch[wave];
    float d0 = 0.f, a0 = 0.f, d1 = 0.f, a1 = 0.f;

    if (DENSE) {
        for (int base = 0; base < k.ng; base += kBatch) {
            const int n = min(kBatch, k.ng - base);
            if (lane < n) stage_entry(batch + 3 * lane, k.recs, k.aux, base + lane);
            wave_sync();
            eval_batch<true>(batch, n, x0, x1, y, z, k.thr, d0, a0, d1, a1);
            wave_sync();
        }
    } else {
        uint32_t* cand = s_cand[wave];
        const int sb = ((bx / kSuperBricks) * k.nsby + by / kSuperBricks) * k.nsbz + bz / kSuperBricks;
        const unsigned long long* words = k.words + (size_t)sb * k.nwords;
        const int xlo = ix0, xhi = ix0 + kSlab - 1;
        const int ylo = by * kBrick, yhi = ylo + kBrick - 1, zlo = bz * kBrick, zhi = zlo + kBrick - 1;
        int nb = 0;   // entries in the batch
        for (int wbase = 0; wbase < k.nwords; wbase += 64) {
            // one hit word per lane; the set bits of the 64 words in (word, bit) order are the candidates
            unsigned long long wd = wbase + lane < k.nwords ? words[wbase + lane] : 0ull;
            int incl = __popcll(wd);
            for (int s = 1; s < 64; s <<= 1) {
                const int up = __shfl_up(incl, s);
                if (lane >= s) incl += up;
            }
            const int total = __shfl(incl, 63);
            int pos = incl - __popcll(wd);   // position of this lane's next candidate
            for (int win = 0; win < total; win += kCand) {
                while (wd != 0ull && pos < win + kCand) {
                    const int bit = __builtin_ctzll(wd);
                    wd &= wd - 1;
                    cand[pos - win] = (uint32_t)(((wbase + lane) << 6) | bit);
                    ++pos;
                }
                wave_sync();
                const int nc = min(kCand, total - win);
                for (int c0 = 0; c0 < nc; c0 += 64) {
                    const int c = c0 + lane;
                    int gi = 0;
                    bool hit = false;
                    if (c < nc) {
                        gi = (int)cand[c];
                        const VoxAux a = k.aux[gi];
                        hit = overlaps(a.bx, xlo, xhi) && overlaps(a.by, ylo, yhi) && overlaps(a.bz, zlo, zhi);
                    }
                    const unsigned long long m = __ballot(hit);
                    const int nh = __popcll(m);
                    if (nb + nh > kBatch) {   // wave-uniform: evaluate what is staged, then stage these
                        wave_sync();
                        eval_batch<false>(batch, nb, x0, x1, y, z, k.thr, d0, a0, d1, a1);
                        wave_sync();
                        nb = 0;
                    }
                    if (hit) stage_entry(batch + 3 * (nb + lanes_below(m)), k.recs, k.aux, gi);
                    nb += nh;
                }
                wave_sync();
            }
        }
        wave_sync();
        eval_batch<false>(batch, nb, x0, x1, y, z, k.thr, d0, a0, d1, a1);
    }

    if (iy < k.ny && iz < k.nz) {
        const size_t o0 = ((size_t)ix0 * k.ny + iy) * k.nz + iz, o1 = o0 + (size_t)k.ny * k.nz;
        const bool two = ix0 + 1 < k.nx;
        if (k.dens) {
            k.dens[o0] = d0;
            if (two) k.dens[o1] = d1;
        }
        if (k.alb) {
            k.alb[o0] = a0;
            if (two) k.alb[o1] = a1;
        }
    }
}

// maximum along one axis: a lane owns one output cell and walks its column (n values, `stride` apart,
// from `base`); first maximum wins, a NaN wins over numbers (numpy.max / numpy.argmax)
__global__ __launch_bounds__(kBlock) void project_kernel(const float* __restrict__ vol, int nx, int ny, int nz,
                                                        int axis, float* __restrict__ max_out,
                                                        int32_t* __restrict__ arg_out) {
    const int n0 = axis == 0 ? ny : nx, n1 = axis == 2 ? ny : nz;   // output [n0, n1]
    const long long cell = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= (long long)n0 * n1) return;
    const int c0 = (int)(cell / n1), c1 = (int)(cell % n1);
    size_t base, stride;
    int n;
    if (axis == 0) { base = (size_t)c0 * nz + c1; stride = (size_t)ny * nz; n = nx; }
    else if (axis == 1) { base = (size_t)c0 * ny * nz + c1; stride = (size_t)nz; n = ny; }
    else { base = ((size_t)c0 * ny + c1) * nz; stride = 1; n = nz; }
    float best = vol[base];
    int arg = 0;
    for (int i = 1; i < n; ++i) {
        const float v = vol[base + (size_t)i * stride];
        if (v > best || (v != v && best == best)) {
            best = v;
            arg = i;
        }
    }
    if (max_out) max_out[cell] = best;
    if (arg_out) arg_out[cell] = arg;
}

int ceil_div(int a, int b) { return (a + b - 1) / b; }

// workspace: GaussRec [ng] | VoxAux [ng] | level-1 words [nsb][nwords] (culled mode only)
struct VoxLayout {
    size_t off_recs, off_aux, off_words, total;
    int nwords, nsbx, nsby, nsbz;
    VoxLayout(const nlosgr_gaussians* g, const nlosgr_voxel_grid* grid, const nlosgr_options* opt) {
        nwords = ceil_div(g->ng, 64);
        nsbx = ceil_div(grid->nx, kSuper); nsby = ceil_div(grid->ny, kSuper); nsbz = ceil_div(grid->nz, kSuper);
        off_recs = 0;
        off_aux = off_recs + align_up((size_t)g->ng * sizeof(GaussRec));
        off_words = off_aux + align_up((size_t)g->ng * sizeof(VoxAux));
        const size_t nw = opt->cutoff > 0.0f ? (size_t)nsbx * nsby * nsbz * nwords : 0;
        total = off_words + align_up(nw * sizeof(unsigned long long)) + 256;
    }
};

}  // namespace

extern "C" {

size_t nlosgr_voxel_workspace_bytes(const nlosgr_gaussians* g, const nlosgr_voxel_grid* grid,
                                    const nlosgr_options* opt) {
    if (validate_voxel(g, grid, opt) != NLOSGR_OK) return 0;
    return VoxLayout(g, grid, opt).total;
}

int nlosgr_voxelize(const nlosgr_gaussians* g, const nlosgr_voxel_grid* grid, const float* cam,
                    const nlosgr_options* opt, void* workspace, float* density_out, float* albedo_out,
                    void* hip_stream) {
    const int rc = validate_voxel(g, grid, opt);
    if (rc) return rc;
    if (!cam) return set_err(NLOSGR_E_INVALID, "null camera position");
    if (!density_out && !albedo_out) return NLOSGR_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t nvox = (size_t)grid->nx * grid->ny * grid->nz;
    if (g->ng == 0) {
        if (density_out) HIPCHK(hipMemsetAsync(density_out, 0, nvox * sizeof(float), s));
        if (albedo_out) HIPCHK(hipMemsetAsync(albedo_out, 0, nvox * sizeof(float), s));
        return NLOSGR_OK;
    }
    if (!workspace) return set_err(NLOSGR_E_INVALID, "null workspace");
    const VoxLayout L(g, grid, opt);
    char* ws = (char*)workspace;
    GaussRec* recs = (GaussRec*)(ws + L.off_recs);
    VoxAux* aux = (VoxAux*)(ws + L.off_aux);
    unsigned long long* words = (unsigned long long*)(ws + L.off_words);
    const bool dense = !(opt->cutoff > 0.0f);

    launch_preprocess(g, recs, s);
    const int nbg = ceil_div(g->ng, kBlock);
    launch_voxel_aux(g, recs, cam, grid, opt->cutoff, aux, s);
    if (!dense) {
        const int nsb = L.nsbx * L.nsby * L.nsbz;
        hipLaunchKernelGGL(voxel_bin_kernel, dim3(nbg, nsb < 1024 ? nsb : 1024), dim3(kBlock), 0, s, aux, g->ng,
                           L.nwords, L.nsbx, L.nsby, L.nsbz, words);
    }
    VArgs k;
    k.recs = recs; k.aux = aux; k.words = words;
    k.ng = g->ng; k.nwords = L.nwords;
    k.nx = grid->nx; k.ny = grid->ny; k.nz = grid->nz;
    k.xs = grid->xs; k.ys = grid->ys; k.zs = grid->zs;
    k.nby = ceil_div(grid->ny, kBrick); k.nbz = ceil_div(grid->nz, kBrick);
    k.nsby = L.nsby; k.nsbz = L.nsbz;
    k.thr = dense ? 0.0f : -kHalfLog2e * opt->cutoff * opt->cutoff;
    k.dens = density_out; k.alb = albedo_out;
    const unsigned nbricks = (unsigned)ceil_div(grid->nx, kBrick) * k.nby * k.nbz;   // <= 128^3
    if (dense) hipLaunchKernelGGL(voxel_eval_kernel<true>, dim3(nbricks), dim3(kBlock), 0, s, k);
    else hipLaunchKernelGGL(voxel_eval_kernel<false>, dim3(nbricks), dim3(kBlock), 0, s, k);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

int nlosgr_volume_project(const float* vol, int32_t nx, int32_t ny, int32_t nz, int32_t axis, float* max_out,
                          int32_t* argmax_out, void* hip_stream) {
    if (nx < 1 || ny < 1 || nz < 1 || nx > kMaxExtent || ny > kMaxExtent || nz > kMaxExtent)
        return set_err(NLOSGR_E_INVALID, "volume extents must be in 1..1024");
    if (axis < 0 || axis > 2) return set_err(NLOSGR_E_INVALID, "axis must be 0, 1 or 2");
    if (!vol) return set_err(NLOSGR_E_INVALID, "null volume pointer");
    if (!max_out && !argmax_out) return set_err(NLOSGR_E_INVALID, "null projection outputs");
    const long long cells = (long long)nx * ny * nz / (axis == 0 ? nx : axis == 1 ? ny : nz);
    hipLaunchKernelGGL(project_kernel, dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)hip_stream, vol, (int)nx, (int)ny, (int)nz, (int)axis, max_out, argmax_out);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

}  // extern "C"
