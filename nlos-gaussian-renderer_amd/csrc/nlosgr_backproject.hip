// Back-projection of a confocal capture onto a regular voxel grid (gfx950): the voxel-wise sum of every wall
// point's histogram at the voxel's time of flight, the baseline every NLOS reconstruction is compared with.
// For voxel centre x (grid tables) and wall point i (include/nlosgr.h, ABI 13):
//
//     d = sqrt((dx*dx + dy*dy) + dz*dz)          fp32, this order, no contraction (as carve_kernel forms it)
//     u = (d - r0) * inv_dr,  k = floor(u),  f = u - k
//     s_i = (1-f) h_i[k] + f h_i[k+1]            h_i[j] = 0 for j < 0 or j >= nr
//     out(x) = sum_i d^power s_i
//
// Shape: a workgroup owns one 8x8x8 brick, z fastest; a lane owns two voxels adjacent in z and shares
// dx*dx + dy*dy between them, so the 64 gathers a wave issues into one row (2 x 8 x 8 voxels) span a few tens of
// bins: a few consecutive cache lines.  Wall points stream through LDS in tiles of 256 positions (float4,
// w unused), the row base is wave-uniform (scalar), the bin index is the lane's.  Every workgroup walks the wall
// in the same order, so a row is fetched from HBM about once and otherwise served by L2 / the Infinity Cache.
//
// Contract: wall points in ascending order, in tiles of 256 counted from this call's wall point 0; a tile is
// summed term by term in fp32 (started at 0), the tile sums are added into a per-voxel fp64 register, rounded
// to fp32 once at the end.  No atomics: bitwise repeatable, and a voxel's value depends on its table
// coordinates and the wall alone, not on the brick or lane it lands in.  The square root is the hardware
// v_sqrt_f32 (__builtin_amdgcn_sqrtf, 1 ulp): parity is judged against float64, not torch bit-exactness.
// A pair's two bins come from one 8-byte read clamped into the row (a one-bin row: its bin alone) and the values
// that are not the pair's bins are dropped by selects, so no lane ever reads outside its row, whatever u is.
#include "nlosgr_project.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

struct BpArgs {
    const float* rows;
    const float* walls;
    int nwall, nr;
    int nx, ny, nz;
    const float *xs, *ys, *zs;
    int nby, nbz;
    float r0, inv_dr;
    int accumulate;
    float* out;
};

// wall points [j, j + N) of the staged tile: every bin offset first, then all 2 N reads, then the sums in
// wall order (the reads of N wall points are in flight together; the order of the additions is the contract's)
template <int POWER, bool PAIR, int N>
__device__ __forceinline__ void bp_step(const float4* tile, int j, const float* __restrict__ row, const BpArgs& a,
                                        float x, float y, float z0, float z1, int kmax, float umax, float& s0,
                                        float& s1) {
    BpTap ta[N], tb[N];
    BpBins va[N], vb[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const float4 w = tile[j + q];
        float ss;
        {
#pragma clang fp contract(off)
            const float dx = x - w.x, dy = y - w.y;
            ss = dx * dx + dy * dy;
        }
        ta[q] = bp_tap<POWER>(ss, z0 - w.z, a.r0, a.inv_dr, kmax, umax);
        tb[q] = bp_tap<POWER>(ss, z1 - w.z, a.r0, a.inv_dr, kmax, umax);
    }
#pragma unroll
    for (int q = 0; q < N; ++q) {
        // wave-uniform row base + the lane's 32-bit byte offset (nr <= 2^29 bins is far above any capture)
        const char* r = (const char*)(row + (size_t)q * a.nr);
        va[q] = bp_read<PAIR>(r, ta[q].ib);
        vb[q] = bp_read<PAIR>(r, tb[q].ib);
    }
#pragma unroll
    for (int q = 0; q < N; ++q) {
        s0 += bp_eval<POWER>(ta[q], va[q]);
        s1 += bp_eval<POWER>(tb[q], vb[q]);
    }
}

template <int POWER, bool PAIR>
__global__ __launch_bounds__(kBlock) void backproject_kernel(BpArgs a) {
    __shared__ float4 tile[kBpTile];
    const int t = threadIdx.x;
    const int bz = blockIdx.x % a.nbz, by = (blockIdx.x / a.nbz) % a.nby, bx = blockIdx.x / (a.nbz * a.nby);
    // lane -> (x, y, z pair) of the brick, z fastest: a wave covers 2 x 8 x 8 voxels
    const int ix = bx * kBpBrick + (t >> 5), iy = by * kBpBrick + ((t >> 2) & 7), iz = bz * kBpBrick + 2 * (t & 3);
    const float x = a.xs[min(ix, a.nx - 1)], y = a.ys[min(iy, a.ny - 1)];
    const float z0 = a.zs[min(iz, a.nz - 1)], z1 = a.zs[min(iz + 1, a.nz - 1)];
    const float umax = (float)(a.nr + 1);
    const int kmax = max(a.nr - 2, 0);
    double acc0 = 0.0, acc1 = 0.0;
    for (int base = 0; base < a.nwall; base += kBpTile) {
        __syncthreads();
        const int i = base + t;
        tile[t] = i < a.nwall ? make_float4(a.walls[3 * (size_t)i], a.walls[3 * (size_t)i + 1],
                                            a.walls[3 * (size_t)i + 2], 0.f)
                              : make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        const int n = min(kBpTile, a.nwall - base);
        const float* row = a.rows + (size_t)base * a.nr;
        float s0 = 0.0f, s1 = 0.0f;
        int j = 0;
        for (; j + kBpGroup <= n; j += kBpGroup, row += (size_t)kBpGroup * a.nr)
            bp_step<POWER, PAIR, kBpGroup>(tile, j, row, a, x, y, z0, z1, kmax, umax, s0, s1);
        for (; j < n; ++j, row += a.nr) bp_step<POWER, PAIR, 1>(tile, j, row, a, x, y, z0, z1, kmax, umax, s0, s1);
        acc0 += (double)s0;
        acc1 += (double)s1;
    }
    if (ix < a.nx && iy < a.ny && iz < a.nz) {
        const size_t o = ((size_t)ix * a.ny + iy) * a.nz + iz;
        const float r0v = (float)acc0, r1v = (float)acc1;
        a.out[o] = a.accumulate ? a.out[o] + r0v : r0v;
        if (iz + 1 < a.nz) a.out[o + 1] = a.accumulate ? a.out[o + 1] + r1v : r1v;
    }
}

}  // namespace

extern "C" {

int nlosgr_backproject(const float* rows, const float* walls, int32_t nwall, int32_t nr, const nlosgr_voxel_grid* grid,
                       const nlosgr_backproject_opts* opt, float* out, void* hip_stream) {
    if (!grid || !opt) return set_err(NLOSGR_E_INVALID, "null argument struct");
    if (grid->nx < 1 || grid->ny < 1 || grid->nz < 1 || grid->nx > kBpMaxExtent || grid->ny > kBpMaxExtent ||
        grid->nz > kBpMaxExtent)
        return set_err(NLOSGR_E_INVALID, "voxel grid extents must be in 1..1024");
    if (nr < 1) return set_err(NLOSGR_E_INVALID, "nr must be >= 1");
    if (nwall < 0) return set_err(NLOSGR_E_INVALID, "nwall must be >= 0");
    if (opt->power < 0 || opt->power > 4) return set_err(NLOSGR_E_INVALID, "back-projection power must be in 0..4");
    if (!(opt->inv_dr > 0.0f) || !(opt->inv_dr <= 3.0e38f))
        return set_err(NLOSGR_E_INVALID, "inv_dr must be finite and > 0");
    if (!(fabsf(opt->r0) <= 3.0e38f)) return set_err(NLOSGR_E_INVALID, "r0 must be finite");
    if (!grid->xs || !grid->ys || !grid->zs) return set_err(NLOSGR_E_INVALID, "null voxel grid table");
    if (!out) return set_err(NLOSGR_E_INVALID, "null back-projection output");
    if (nwall > 0 && (!rows || !walls)) return set_err(NLOSGR_E_INVALID, "null rows or walls pointer");
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t nvox = (size_t)grid->nx * grid->ny * grid->nz;
    if (nwall == 0) {
        if (!opt->accumulate) HIPCHK(hipMemsetAsync(out, 0, nvox * sizeof(float), s));
        return NLOSGR_OK;
    }
    BpArgs a;
    a.rows = rows; a.walls = walls; a.nwall = nwall; a.nr = nr;
    a.nx = grid->nx; a.ny = grid->ny; a.nz = grid->nz;
    a.xs = grid->xs; a.ys = grid->ys; a.zs = grid->zs;
    a.nby = (grid->ny + kBpBrick - 1) / kBpBrick; a.nbz = (grid->nz + kBpBrick - 1) / kBpBrick;
    a.r0 = opt->r0; a.inv_dr = opt->inv_dr; a.accumulate = opt->accumulate != 0;
    a.out = out;
    const unsigned nbricks = (unsigned)((grid->nx + kBpBrick - 1) / kBpBrick) * a.nby * a.nbz;   // <= 128^3
    const bool pair = nr >= 2;
#define NLOSGR_BP_LAUNCH(P)                                                                                   \
    if (pair) hipLaunchKernelGGL((backproject_kernel<P, true>), dim3(nbricks), dim3(kBlock), 0, s, a);       \
    else hipLaunchKernelGGL((backproject_kernel<P, false>), dim3(nbricks), dim3(kBlock), 0, s, a)
    switch (opt->power) {
        case 0: NLOSGR_BP_LAUNCH(0); break;
        case 1: NLOSGR_BP_LAUNCH(1); break;
        case 2: NLOSGR_BP_LAUNCH(2); break;
        case 3: NLOSGR_BP_LAUNCH(3); break;
        default: NLOSGR_BP_LAUNCH(4); break;
    }
#undef NLOSGR_BP_LAUNCH
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

}  // extern "C"
