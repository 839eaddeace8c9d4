// Forward projection of a voxel grid to the transients a confocal capture would hold (gfx950): the adjoint of
// nlosgr_backproject.  For voxel centre x (grid tables) and wall point i (include/nlosgr.h, ABI 13):
//
//     d = sqrt((dx*dx + dy*dy) + dz*dz)          fp32, this order, no contraction (as bp_tap forms it)
//     u = (d - r0) * inv_dr,  k = floor(u),  f = u - k
//     rows_i[j] = sum_x d^power vol(x) ((1-f) [k == j] + f [k+1 == j]),   0 <= j < nr
//
// A scatter: every voxel adds into two bins of every wall point's row.  No float atomics: each term is rounded
// once to a multiple of the call's quantum q (a power of two, fp_unit below) and added as a 64-bit integer, so
// the order of the additions cannot matter and the result is bitwise the same for every nsplit, launch shape
// and workgroup order.
//
// Shape: one 256-thread workgroup per (W wall points, voxel split) with W int64 LDS rows of nr bins; W = 4, 2 or
// 1 (fp_walls_per_group), so a voxel's value and coordinates are read once for W wall points: with W = 1 the walk
// over the volume was a third of the time.  A lane owns kFpRun voxels adjacent in z (flat index, z fastest), so a
// wave reads 1 KiB of vol contiguously; zero voxels are skipped.  Every remaining (voxel, wall point) pair issues
// two no-return 64-bit LDS adds.  (NLOSGR_FP_MERGE, a build option: a lane keeps the two bins of its current k in
// registers while consecutive voxels fall into the same k and adds when k changes; integer adds, so no bit
// changes.  At C3's window a voxel step is six bins and the merge only costs: DESIGN.md section 7.)  With
// nsplit == 1 the workgroup scales its own rows and stores floats; otherwise the workgroups add their non-zero
// bins into the int64 [nwall][nr] workspace with 64-bit integer atomics and fp_finish_kernel scales it.
//
// Addresses (contract 7): u is clamped into [-2, nr + 1] (a NaN u goes to -2), k = floor(u) lies in
// [-2, nr + 1], and an add into bin j = k or k + 1 is issued only under (unsigned)j < nr.  Voxel indices stay
// below the split's end <= nvox, and (ix, iy, iz) is the mixed-radix form of such an index, so every table read
// is inside its table.
#include "nlosgr_project.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

struct FpArgs {
    const float* vol;
    const float* walls;
    int nwall, nr;
    int nx, ny, nz;
    const float *xs, *ys, *zs;
    float r0, inv_dr;
    int accumulate, nsplit;
    unsigned nvox, chunk;          // chunk: voxels per split, a multiple of kFpRun
    int sx, sy, sz;                // kFpStep = (sx * ny + sy) * nz + sz
    int ew, S;                     // wmax < 2^ew; every term is below 2^S quanta
    const unsigned* vmax;          // bits of max|vol| (any non-finite voxel: >= 0x7f800000)
    unsigned long long* acc;       // [nwall][nr] (nsplit > 1)
    float* out;
};

template <int POWER>
__device__ __forceinline__ float fp_weight(float d) {
    constexpr int P = POWER < 0 ? -POWER : POWER;
    if (P == 0) return 1.0f;
    const float d2 = d * d;
    const float p = P == 1 ? d : (P == 2 ? d2 : (P == 3 ? d2 * d : d2 * d2));
    return POWER < 0 ? 1.0f / p : p;
}

// timing-only builds (their rows are wrong): 1 = no LDS adds (the values go into a register sum that is kept
// alive), 2 = no fp32 -> int64 conversion (a bit cast in its place)
#ifndef NLOSGR_FP_TIMING
#define NLOSGR_FP_TIMING 0
#endif

__device__ __forceinline__ void fp_add(unsigned long long* row, int j, int nr, long long v, unsigned long long& sink) {
    if ((unsigned)j < (unsigned)nr && v != 0) {
        if (NLOSGR_FP_TIMING == 1) sink += (unsigned long long)v ^ (unsigned)j;
        else __hip_atomic_fetch_add(row + j, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// a term in quanta, rounded to nearest (there is no single fp32 -> int64 instruction: through double)
__device__ __forceinline__ long long fp_quanta(float term, double to_q) {
    if (NLOSGR_FP_TIMING == 2) return (long long)__float_as_int(term);
    return __double2ll_rn((double)term * to_q);
}

template <int POWER, bool MERGE, int W>
__global__ __launch_bounds__(kBlock) void forward_project_kernel(FpArgs a) {
    extern __shared__ unsigned long long fp_row[];      // W rows of nr bins
    const int t = threadIdx.x;
    const int grp = blockIdx.x / a.nsplit, sp = blockIdx.x - grp * a.nsplit;
    const int i0 = grp * W, nw = min(W, a.nwall - i0);   // this workgroup's wall points [i0, i0 + nw)
    const bool single = a.nsplit == 1;
    const int nr = a.nr;
    float* const orow = a.out + (size_t)i0 * nr;
    const unsigned vb = *a.vmax;
    if (vb >= 0x7f800000u || vb == 0u) {                 // a non-finite voxel: NaN rows; a zero volume: zero rows
        if (single && !(vb == 0u && a.accumulate)) {
            const float fill = vb ? __uint_as_float(0x7fc00000u) : 0.0f;
            for (int j = t; j < nw * nr; j += kBlock) orow[j] = fill;
        }
        return;
    }
    for (int j = t; j < W * nr; j += kBlock) fp_row[j] = 0ull;
    __syncthreads();
    double to_q, from_q;
    fp_unit(vb, a.ew, a.S, to_q, from_q);
    // a wall point past the end gets NaN coordinates: its u is NaN, clamped to -2, and every add is masked
    float wx[W], wy[W], wz[W];
    int kc[W];                      // the k whose two bins the lane holds (-4: none; k itself is >= -2)
    long long s0[W], s1[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const bool in = w < nw;
        const size_t o = 3 * (size_t)(i0 + (in ? w : 0));
        const float nan = __uint_as_float(0x7fc00000u);
        wx[w] = in ? a.walls[o] : nan; wy[w] = in ? a.walls[o + 1] : nan; wz[w] = in ? a.walls[o + 2] : nan;
        kc[w] = -4; s0[w] = 0; s1[w] = 0;
    }
    unsigned long long sink = 0ull;   // (timing-only builds)
    const float umax = (float)(nr + 1);
    const unsigned v0 = (unsigned)sp * a.chunk, v1 = min(v0 + a.chunk, a.nvox);   // < 2^31: no wrap
    unsigned base = v0 + (unsigned)(kFpRun * t);
    int iz = (int)(base % (unsigned)a.nz);
    unsigned rest = base / (unsigned)a.nz;
    int iy = (int)(rest % (unsigned)a.ny), ix = (int)(rest / (unsigned)a.ny);
    for (; base < v1; base += kFpStep) {
        float v[kFpRun];
#pragma unroll
        for (int r = 0; r < kFpRun; ++r) v[r] = base + r < v1 ? a.vol[base + r] : 0.0f;
        bool any = false;
#pragma unroll
        for (int r = 0; r < kFpRun; ++r) any |= v[r] != 0.0f;
        if (any) {
            int jx = ix, jy = iy, jz = iz;
#pragma unroll
            for (int r = 0; r < kFpRun; ++r) {
                if (v[r] != 0.0f) {                      // (a non-zero voxel is below v1, so jx < nx)
                    const float x = a.xs[jx], y = a.ys[jy], z = a.zs[jz];
#pragma unroll
                    for (int w = 0; w < W; ++w) {
#pragma clang fp contract(off)
                        const float dx = x - wx[w], dy = y - wy[w], dz = z - wz[w];
                        const float ss = dx * dx + dy * dy;
                        const float d = fsqrt(ss + dz * dz);
                        // clamped to [-2, nr + 1]: both bins are outside the row at either end (NaN goes to -2)
                        const float u = fminf(fmaxf((d - a.r0) * a.inv_dr, -2.0f), umax);
                        const float kf = floorf(u);
                        const int k = (int)kf;
                        const float f = u - kf;
                        const float wv = POWER == 0 ? v[r] : fp_weight<POWER>(d) * v[r];
                        const long long q0 = fp_quanta(wv * (1.0f - f), to_q);
                        const long long q1 = fp_quanta(wv * f, to_q);
                        if (MERGE && k == kc[w]) {
                            s0[w] += q0;
                            s1[w] += q1;
                        } else {
                            fp_add(fp_row + w * nr, kc[w], nr, s0[w], sink);
                            fp_add(fp_row + w * nr, kc[w] + 1, nr, s1[w], sink);
                            kc[w] = k; s0[w] = q0; s1[w] = q1;
                        }
                    }
                }
                if (++jz == a.nz) {
                    jz = 0;
                    if (++jy == a.ny) { jy = 0; ++jx; }
                }
            }
        }
        // the next step's first voxel: one carry per digit (sz < nz, sy < ny)
        iz += a.sz;
        if (iz >= a.nz) { iz -= a.nz; ++iy; }
        iy += a.sy;
        if (iy >= a.ny) { iy -= a.ny; ++ix; }
        ix += a.sx;
    }
#pragma unroll
    for (int w = 0; w < W; ++w) {
        fp_add(fp_row + w * nr, kc[w], nr, s0[w], sink);
        fp_add(fp_row + w * nr, kc[w] + 1, nr, s1[w], sink);
    }
    if (NLOSGR_FP_TIMING == 1 && sink == 0x0123456789abcdefull) fp_row[0] = sink;
    __syncthreads();
    if (single) {
        for (int j = t; j < nw * nr; j += kBlock) {
            const float r = (float)((double)(long long)fp_row[j] * from_q);
            orow[j] = a.accumulate ? orow[j] + r : r;
        }
    } else {
        unsigned long long* const g = a.acc + (size_t)i0 * nr;
        for (int j = t; j < nw * nr; j += kBlock) {
            const unsigned long long s = fp_row[j];
            if (s) __hip_atomic_fetch_add(g + j, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// host validation shared by both entry points; on success the weight bound's exponent and the split count
int fp_plan(int32_t nwall, int32_t nr, const nlosgr_voxel_grid* grid, const nlosgr_forward_project_opts* opt, int* ew,
            int* nsplit) {
    if (!grid || !opt) return set_err(NLOSGR_E_INVALID, "null argument struct");
    if (grid->nx < 1 || grid->ny < 1 || grid->nz < 1 || grid->nx > kFpMaxExtent || grid->ny > kFpMaxExtent ||
        grid->nz > kFpMaxExtent)
        return set_err(NLOSGR_E_INVALID, "voxel grid extents must be in 1..1024");
    if (nr < 1) return set_err(NLOSGR_E_INVALID, "nr must be >= 1");
    if (nr > NLOSGR_IRF_MAX_NR) return set_err(NLOSGR_E_UNSUPPORTED, "nr above NLOSGR_IRF_MAX_NR");
    if (nwall < 0) return set_err(NLOSGR_E_INVALID, "nwall must be >= 0");
    if (opt->power < -4 || opt->power > 4)
        return set_err(NLOSGR_E_INVALID, "forward-projection power must be in -4..4");
    if (!(opt->inv_dr > 0.0f) || !(opt->inv_dr <= 3.0e38f))
        return set_err(NLOSGR_E_INVALID, "inv_dr must be finite and > 0");
    if (!(fabsf(opt->r0) <= 3.0e38f)) return set_err(NLOSGR_E_INVALID, "r0 must be finite");
    if (opt->power < 0 && !((double)opt->r0 * (double)opt->inv_dr >= 2.0))
        return set_err(NLOSGR_E_INVALID, "a negative power needs r0 * inv_dr >= 2");
    if (opt->nsplit < 0) return set_err(NLOSGR_E_INVALID, "nsplit must be >= 0");
    if (!grid->xs || !grid->ys || !grid->zs) return set_err(NLOSGR_E_INVALID, "null voxel grid table");
    // wmax: the largest weight of a contributing pair (u > -1 and u < nr), from the fp32 window in double
    const double dr = 1.0 / (double)opt->inv_dr;
    const int p = opt->power < 0 ? -opt->power : opt->power;
    double R = opt->power < 0 ? (double)opt->r0 - 1.5 * dr : (double)opt->r0 + (double)(nr + 1) * dr;
    if (R < 0.0) R = 0.0;
    double w = 1.0;
    for (int q = 0; q < p; ++q) w *= R;
    if (opt->power < 0) w = 1.0 / w;
    w *= kFpWeightMargin;
    if (!(w <= 1.0e300)) return set_err(NLOSGR_E_INVALID, "r0 and inv_dr give no finite bound on d^power");
    (void)frexp(w, ew);
    return fp_split_count(nwall, nr, grid, opt->nsplit, nsplit);
}

}  // namespace

extern "C" {

size_t nlosgr_forward_project_workspace_bytes(int32_t nwall, int32_t nr, const nlosgr_voxel_grid* grid,
                                              const nlosgr_forward_project_opts* opt) {
    int ew, ns;
    if (fp_plan(nwall, nr, grid, opt, &ew, &ns) != NLOSGR_OK) return 0;
    return kFpHeader + (ns > 1 ? align_up((size_t)nwall * nr * sizeof(unsigned long long)) : 0);
}

int nlosgr_forward_project(const float* vol, const float* walls, int32_t nwall, int32_t nr,
                           const nlosgr_voxel_grid* grid, const nlosgr_forward_project_opts* opt, void* workspace,
                           float* rows_out, void* hip_stream) {
    int ew, ns;
    const int rc = fp_plan(nwall, nr, grid, opt, &ew, &ns);
    if (rc != NLOSGR_OK) return rc;
    if (!vol) return set_err(NLOSGR_E_INVALID, "null vol pointer");
    if (!workspace) return set_err(NLOSGR_E_INVALID, "null forward-projection workspace");
    if (nwall == 0) return NLOSGR_OK;
    if (!walls) return set_err(NLOSGR_E_INVALID, "null walls pointer");
    if (!rows_out) return set_err(NLOSGR_E_INVALID, "null forward-projection output");
    hipStream_t s = (hipStream_t)hip_stream;
    FpArgs a;
    a.vol = vol; a.walls = walls; a.nwall = nwall; a.nr = nr;
    a.nx = grid->nx; a.ny = grid->ny; a.nz = grid->nz;
    a.xs = grid->xs; a.ys = grid->ys; a.zs = grid->zs;
    a.r0 = opt->r0; a.inv_dr = opt->inv_dr; a.accumulate = opt->accumulate != 0; a.nsplit = ns;
    a.nvox = (unsigned)grid->nx * grid->ny * grid->nz;
    a.chunk = ((a.nvox + ns - 1) / ns + kFpRun - 1) / kFpRun * kFpRun;
    a.sz = kFpStep % a.nz; a.sy = (kFpStep / a.nz) % a.ny; a.sx = (kFpStep / a.nz) / a.ny;
    a.ew = ew; a.S = 62 - fp_ceil_log2(2ull * a.nvox);
    a.vmax = (const unsigned*)workspace;
    a.acc = (unsigned long long*)((char*)workspace + kFpHeader);
    a.out = rows_out;
    const size_t nrow = (size_t)nwall * nr;
    HIPCHK(hipMemsetAsync(workspace, 0, kFpHeader + (ns > 1 ? nrow * sizeof(unsigned long long) : 0), s));
    const unsigned nb = (a.nvox + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(fp_vmax_kernel, dim3(nb < 1024u ? nb : 1024u), dim3(kBlock), 0, s, vol, a.nvox,
                       (unsigned*)workspace);
    const int W = fp_walls_per_group(nwall, nr);
    const dim3 g((unsigned)((nwall + W - 1) / W) * (unsigned)ns);
    const size_t lds = (size_t)W * nr * sizeof(unsigned long long);
#ifdef NLOSGR_FP_MERGE
    constexpr bool merge = true;       // A/B build: a lane holds the two bins of its current k in registers
#else
    constexpr bool merge = false;
#endif
#define NLOSGR_FP_LAUNCH(P)                                                                                     \
    if (W == 4) hipLaunchKernelGGL((forward_project_kernel<P, merge, 4>), g, dim3(kBlock), lds, s, a);          \
    else if (W == 2) hipLaunchKernelGGL((forward_project_kernel<P, merge, 2>), g, dim3(kBlock), lds, s, a);     \
    else hipLaunchKernelGGL((forward_project_kernel<P, merge, 1>), g, dim3(kBlock), lds, s, a);                 \
    break
    switch (opt->power) {
        case -4: NLOSGR_FP_LAUNCH(-4);
        case -3: NLOSGR_FP_LAUNCH(-3);
        case -2: NLOSGR_FP_LAUNCH(-2);
        case -1: NLOSGR_FP_LAUNCH(-1);
        case 0: NLOSGR_FP_LAUNCH(0);
        case 1: NLOSGR_FP_LAUNCH(1);
        case 2: NLOSGR_FP_LAUNCH(2);
        case 3: NLOSGR_FP_LAUNCH(3);
        default: NLOSGR_FP_LAUNCH(4);
    }
#undef NLOSGR_FP_LAUNCH
    HIPCHK(hipGetLastError());
    if (ns > 1) {
        hipLaunchKernelGGL(fp_finish_kernel, dim3((unsigned)((nrow + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a.acc,
                           nrow, a.vmax, ew, a.S, a.accumulate, rows_out);
        HIPCHK(hipGetLastError());
    }
    return NLOSGR_OK;
}

}  // extern "C"
