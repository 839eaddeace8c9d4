// Light-cone transform of a confocal capture (O'Toole, Lindell, Wetzstein 2018; gfx950): the four passes around the
// FFTs of   rows -> resampled to depth-squared cells -> 3-D FFT -> Wiener product with the light cone's spectrum ->
// inverse FFT -> resampled back to time bins.  The FFTs themselves are the caller's (torch.fft: hipFFT); this
// library links the HIP runtime alone.  The work arrays are complex64 [Nz][Nx][Nv] (interleaved re, im) with
// Nz = 2 H, Nx = 2 W, Nv = 2 nv; lattice point (m, n) is measured at (xs[n], y0, zs[m]) and its row is
// rows[perm[m sm + n sn]] (perm NULL: rows[m sm + n sn]): lattice_row of nlosgr_lattice.hpp, as in nlosgr_fk.hip.
//
// The resampling operator R [nv][nr] between time bins j and depth-squared cells i (include/nlosgr.h) comes as run
// tables built by the caller in double: row i of R holds weight[start[i] .. start[i+1]) at bins first[i], first[i]
// + 1, ...; the tables of R^T give, per bin j, its run of cells.  Every row and column is one contiguous run.
//
//   nlosgr_lct_load    pad[m][n][i] = (sum_j R[i][j] psi[j], 0), psi = max(rows[v][j], 0) (r0 + j dr)^power (fk_psi
//                      without the square root, nlosgr_lattice.hpp), j ascending, acc = fmaf(w, psi, acc);
//                      zero for m >= H, n >= W or i >= nv.
//   nlosgr_lct_kernel  with signed DFT indices c (z), b (x): s = ((b sx)^2 + (c sz)^2) / dv, k = floor(s), f = s - k
//                      in fp64 without contraction; K[c][b][k] = (float)(scale (1 - f)) where k <= nv - 1,
//                      K[c][b][k+1] = (float)(scale f) where k + 1 <= nv - 1, zero elsewhere.
//   nlosgr_lct_filter  G = conj(Fk) / (|Fk|^2 + 1/snr) (Wiener), conj(Fk) (back-projection), or the array itself (an
//                      inverse built before); out = G, or spec G.  fp32: |Fk|^2 = fmaf(im, im, re re), two IEEE
//                      divisions, the product as fmaf(sr, gr, -(si gi)), fmaf(sr, gi, si gr).  The stored G and the
//                      G formed on the fly are the same fp32 values, so both routes give the same bits.
//   nlosgr_lct_store   volume[n][j][m] = max(sum_i R[i][j] Re o[m][n][i], 0), i ascending, acc = fmaf(w, o, acc).
//
// The operator pair (A: volume -> rows, A^T: rows -> volume; include/nlosgr.h) adds the passes that run the same two
// resamplings the other way round and the signed variants of load and store.  w_j = (r0 + j dr)^power, power -4..4:
// r = fmaf(j, dr, r0), |power| by the multiplications of fk_psi, a negative power as one IEEE division 1 / r^|power|,
// and 0 where r <= 0.
//
//   nlosgr_lct_load_volume   pad[m][n][i] = (sum_j R[i][j] volume[n][j][m], 0), j ascending, acc = fmaf(w, v, acc);
//                            zero for m >= H, n >= W or i >= nv.  No clamp, no weight.
//   nlosgr_lct_store_rows    rows[v][j] = w_j sum_i R[i][j] Re o[m][n][i], i ascending, fmaf, one multiply at the end.
//   nlosgr_lct_load_rows     nlosgr_lct_load with psi = rows[v][j] w_j (no clamp): the same kernel, another instance.
//   nlosgr_lct_store_volume  nlosgr_lct_store without the clamp: the same kernel, another instance.
//
// Shape.  load, kernel and filter give a workgroup one (c, b) column; a lane writes two adjacent complex cells (16
// bytes), the zeros included, so none needs a memset.  load stages the weighted row in LDS (nr <= 1024 floats) and a
// lane gathers its two cells' short runs from it.  store owns a tile of 64 bins x 64 z of one wall column: the
// tile's cells form one contiguous range, read in chunks of 64 along v (lanes along v, coalesced) into an LDS tile
// padded to 65 floats a row; then lanes run along z, each holding the sums of 16 bins in registers (a wave shares
// its bin, so the run tables are wave-uniform and the LDS reads of a wave hit 64 different banks), and write along z
// coalesced.  No atomics; every output element is written by one lane in a fixed order: bitwise repeatable.  Table
// entries are clamped before use: a bad table reads a wrong bin or cell, never outside an array.
//
// load_volume mirrors store: a workgroup owns 64 cells x 64 z of one wall column.  The tile's bins form one
// contiguous range, read in chunks of 64 bins with lanes along z (the volume's fastest axis, coalesced) into an LDS
// tile [bin][z] padded to 65 floats a row; then lanes run along the cells, each summing its own run for the 16 z of
// its wave (a wave reads addresses bin 65 + z with z wave-uniform: neighbouring cells share a bin, a broadcast, or
// sit in neighbouring bins, distinct banks), and write 8-byte complex cells along i, coalesced.  The same workgroup
// writes the tile's seven zero images in the padding (m + H, n + W, i + nv), so every element of pad has one writer.
// store_rows needs no transpose: a workgroup stages the nv real parts of one lattice column in LDS and lanes run
// along j.
#include "nlosgr_common.hpp"
#include "nlosgr_lattice.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

constexpr int kLctMaxCells = 2048;   // nv
constexpr int kLctTile = 64;         // store: tile edge along bins and along z, and the chunk of cells
constexpr int kLctBinsPerLane = kLctTile / kWaves;

// one run of a table, clamped: entries [s, s + cnt) of weight, positions [f, f + cnt) of an axis of `len`
struct LctRun {
    int f, s, cnt;
};

__device__ __forceinline__ LctRun lct_run(const int* first, const int* start, int row, int len, int nnz) {
    LctRun r;
    r.f = min(max(first[row], 0), len - 1);
    r.s = min(max(start[row], 0), nnz);
    r.cnt = min(max(min(max(start[row + 1], 0), nnz) - r.s, 0), len - r.f);
    return r;
}

struct LctLoadArgs {
    const float* rows;
    const int* perm;
    const int* first;      // [nv]
    const int* start;      // [nv + 1]
    const float* weight;   // [nnz]
    int H, W, nr, nv, nnz, sm, sn;
    float r0, dr;
    int power;             // read by the signed instance alone
    float4* pad;           // [Nz * Nx][nv]: two complex cells each
};

constexpr int kLctSigned = -1;  // lct_load_kernel<kLctSigned>: no clamp, the power (-4..4) from the arguments

// (r0 + j dr)^power, power in -4..4: fk_psi's r and its multiplications (nlosgr_lattice.hpp); 1 / r^|power| by one
// IEEE division, 0 where r <= 0
__device__ __forceinline__ float lct_weight(int power, int j, float r0, float dr) {
#pragma clang fp contract(off)
    const float r = bin_radius(j, r0, dr);
    const float w = radius_power(r, power);
    if (power >= 0) return w;
    return r > 0.0f ? 1.0f / w : 0.0f;
}

__device__ __forceinline__ float lct_cell(const LctLoadArgs& a, const float* psi, int i) {
    const LctRun r = lct_run(a.first, a.start, i, a.nr, a.nnz);
    float acc = 0.0f;
    for (int q = 0; q < r.cnt; ++q) acc = fmaf(a.weight[r.s + q], psi[r.f + q], acc);
    return acc;
}

template <int POWER>
__global__ __launch_bounds__(kBlock) void lct_load_kernel(LctLoadArgs a) {
    __shared__ float psi[kLatticeMaxExtent];
    const int Nx = 2 * a.W;
    const int c = blockIdx.x / Nx, b = blockIdx.x - c * Nx;
    float4* const col = a.pad + (size_t)blockIdx.x * a.nv;
    const bool inside = c < a.H && b < a.W;                 // the same for the whole workgroup
    if (inside) {
        const float* const row = a.rows + (size_t)lattice_row(a.perm, c, b, a.sm, a.sn, a.H, a.W) * a.nr;
        for (int j = threadIdx.x; j < a.nr; j += kBlock) {
            if constexpr (POWER == kLctSigned) psi[j] = row[j] * lct_weight(a.power, j, a.r0, a.dr);
            else psi[j] = fk_psi<POWER, false>(row[j], j, a.r0, a.dr);
        }
        __syncthreads();
    }
    for (int p = threadIdx.x; p < a.nv; p += kBlock) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        const int i = 2 * p;
        if (inside && i < a.nv) {
            o.x = lct_cell(a, psi, i);
            if (i + 1 < a.nv) o.z = lct_cell(a, psi, i + 1);
        }
        col[p] = o;
    }
}

struct LctKernelArgs {
    float4* K;             // [Nz * Nx][nv]: two complex cells each
    int H, W, nv;
    double sx, sz, dv, scale;
};

__global__ __launch_bounds__(kBlock) void lct_kernel_kernel(LctKernelArgs a) {
#pragma clang fp contract(off)
    const int Nx = 2 * a.W;
    const int ci = blockIdx.x / Nx, bi = blockIdx.x - ci * Nx;
    const int c = dft_signed(ci, a.H), b = dft_signed(bi, a.W);
    const double lb = a.sx * (double)b, lc = a.sz * (double)c;
    const double s = (lb * lb + lc * lc) / a.dv;
    const double kf = floor(s);
    int k = -2;                                             // a column beyond the last cell (or a NaN): all zero
    float w0 = 0.0f, w1 = 0.0f;
    if (kf <= (double)(a.nv - 1)) {
        const double f = s - kf;
        k = (int)kf;
        w0 = (float)(a.scale * (1.0 - f));
        w1 = (float)(a.scale * f);
    }
    float4* const col = a.K + (size_t)blockIdx.x * a.nv;
    // pair p holds cells 2p and 2p + 1; the cells from nv on are the padding
    for (int p = threadIdx.x; p < a.nv; p += kBlock) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        const int i = 2 * p;
        if (i < a.nv) {
            o.x = i == k ? w0 : (i == k + 1 ? w1 : 0.0f);
            if (i + 1 < a.nv) o.z = i + 1 == k ? w0 : (i == k ? w1 : 0.0f);
        }
        col[p] = o;
    }
}

struct LctFilterArgs {
    const float4* kf;      // [Nz * Nx][nv]: the kernel's spectrum, or the inverse
    const float4* spec;    // the same shape, or NULL
    float4* out;
    int nv;
    float inv_snr;
};

enum { kLctWiener = 0, kLctBackprop = 1, kLctGiven = 2 };

template <int MODE>
__device__ __forceinline__ float2 lct_inverse(float re, float im, float inv_snr) {
#pragma clang fp contract(off)
    if (MODE == kLctGiven) return make_float2(re, im);
    if (MODE == kLctBackprop) return make_float2(re, -im);
    const float den = fmaf(im, im, re * re) + inv_snr;
    return make_float2(re / den, -im / den);
}

__device__ __forceinline__ float2 lct_cmul(float sr, float si, float2 g) {
#pragma clang fp contract(off)
    return make_float2(fmaf(sr, g.x, -(si * g.y)), fmaf(sr, g.y, si * g.x));
}

template <int MODE, bool APPLY>
__global__ __launch_bounds__(kBlock) void lct_filter_kernel(LctFilterArgs a) {
    const size_t base = (size_t)blockIdx.x * a.nv;
    for (int p = threadIdx.x; p < a.nv; p += kBlock) {
        const float4 k = a.kf[base + p];
        float2 g0 = lct_inverse<MODE>(k.x, k.y, a.inv_snr), g1 = lct_inverse<MODE>(k.z, k.w, a.inv_snr);
        if (APPLY) {
            const float4 s = a.spec[base + p];
            g0 = lct_cmul(s.x, s.y, g0);
            g1 = lct_cmul(s.z, s.w, g1);
        }
        a.out[base + p] = make_float4(g0.x, g0.y, g1.x, g1.y);
    }
}

struct LctStoreArgs {
    const float2* field;   // [Nz][Nx][Nv]
    const int* first;      // [nr]: the tables of R^T
    const int* start;      // [nr + 1]
    const float* weight;   // [nnz]
    float* vol;            // [W][nr][H]
    int H, W, nr, nv, nnz;
};

// block (jt, mt, n): the tile j in [64 jt, +64), m in [64 mt, +64) of wall column n
template <bool CLAMP>
__global__ __launch_bounds__(kBlock) void lct_store_kernel(LctStoreArgs a) {
    __shared__ float cells[kLctTile][kLctTile + 1];         // [z][cell of the chunk]
    __shared__ int run_f[kLctTile], run_s[kLctTile], run_n[kLctTile];
    const int t = threadIdx.x;
    const int j0 = blockIdx.x * kLctTile, m0 = blockIdx.y * kLctTile, n = blockIdx.z;
    const size_t Nx = 2 * (size_t)a.W, Nv = 2 * (size_t)a.nv;
    if (t < kLctTile) {
        LctRun r = {0, 0, 0};
        if (j0 + t < a.nr) r = lct_run(a.first, a.start, j0 + t, a.nv, a.nnz);
        run_f[t] = r.f; run_s[t] = r.s; run_n[t] = r.cnt;
    }
    __syncthreads();
    int ibeg = a.nv, iend = 0;                              // the tile's cells: [ibeg, iend), inside [0, nv)
    for (int q = 0; q < kLctTile; ++q)
        if (run_n[q] > 0) {
            ibeg = min(ibeg, run_f[q]);
            iend = max(iend, run_f[q] + run_n[q]);
        }
    const int lane = t & 63, wave = t >> 6;
    float acc[kLctBinsPerLane];
#pragma unroll
    for (int q = 0; q < kLctBinsPerLane; ++q) acc[q] = 0.0f;
    for (int i0 = ibeg; i0 < iend; i0 += kLctTile) {
        const int i1 = min(i0 + kLctTile, iend);
        __syncthreads();                                    // the chunk before has been read
        for (int mm = wave; mm < kLctTile; mm += kWaves) {
            const int m = m0 + mm, i = i0 + lane;
            if (m < a.H && i < i1) cells[mm][lane] = a.field[((size_t)m * Nx + n) * Nv + i].x;
        }
        __syncthreads();
        if (m0 + lane < a.H) {
#pragma unroll
            for (int q = 0; q < kLctBinsPerLane; ++q) {
                const int jj = wave + q * kWaves;           // the same bin for the whole wave
                const int f = run_f[jj], lo = max(f, i0), hi = min(f + run_n[jj], i1);
                const float* const w = a.weight + run_s[jj];
                for (int i = lo; i < hi; ++i) acc[q] = fmaf(w[i - f], cells[lane][i - i0], acc[q]);
            }
        }
    }
    const int m = m0 + lane;
    if (m < a.H) {
#pragma unroll
        for (int q = 0; q < kLctBinsPerLane; ++q) {
            const int j = j0 + wave + q * kWaves;
            if (j < a.nr) a.vol[((size_t)n * a.nr + j) * a.H + m] = CLAMP ? fmaxf(acc[q], 0.0f) : acc[q];
        }
    }
}

struct LctLoadVolumeArgs {
    const float* vol;      // [W][nr][H]
    const int* first;      // [nv]: the tables of R
    const int* start;      // [nv + 1]
    const float* weight;   // [nnz]
    float2* pad;           // [Nz][Nx][Nv]
    int H, W, nr, nv, nnz;
};

// block (it, mt, n): the tile i in [64 it, +64), m in [64 mt, +64) of wall column n, and its seven zero images
__global__ __launch_bounds__(kBlock) void lct_load_volume_kernel(LctLoadVolumeArgs a) {
    __shared__ float bins[kLctTile][kLctTile + 1];          // [bin of the chunk][z]
    __shared__ int run_f[kLctTile], run_s[kLctTile], run_n[kLctTile];
    const int t = threadIdx.x;
    const int i0 = blockIdx.x * kLctTile, m0 = blockIdx.y * kLctTile, n = blockIdx.z;
    const size_t Nx = 2 * (size_t)a.W, Nv = 2 * (size_t)a.nv;
    if (t < kLctTile) {
        LctRun r = {0, 0, 0};
        if (i0 + t < a.nv) r = lct_run(a.first, a.start, i0 + t, a.nr, a.nnz);
        run_f[t] = r.f; run_s[t] = r.s; run_n[t] = r.cnt;
    }
    __syncthreads();
    int jbeg = a.nr, jend = 0;                              // the tile's bins: [jbeg, jend), inside [0, nr)
    for (int q = 0; q < kLctTile; ++q)
        if (run_n[q] > 0) {
            jbeg = min(jbeg, run_f[q]);
            jend = max(jend, run_f[q] + run_n[q]);
        }
    const int lane = t & 63, wave = t >> 6;
    const int f = run_f[lane], cnt = run_n[lane];           // this lane's cell
    const float* const w = a.weight + run_s[lane];
    const int zn = min(kLctTile, a.H - m0);                 // the tile's z: [0, zn)
    float acc[kLctBinsPerLane];                             // z = wave + q kWaves
#pragma unroll
    for (int q = 0; q < kLctBinsPerLane; ++q) acc[q] = 0.0f;
    for (int j0 = jbeg; j0 < jend; j0 += kLctTile) {
        const int j1 = min(j0 + kLctTile, jend);
        __syncthreads();                                    // the chunk before has been read
        if (lane < zn)
            for (int bb = wave; bb < j1 - j0; bb += kWaves)
                bins[bb][lane] = a.vol[((size_t)n * a.nr + j0 + bb) * a.H + m0 + lane];
        __syncthreads();
        const int lo = max(f, j0), hi = min(f + cnt, j1);
        for (int j = lo; j < hi; ++j) {
            const float wj = w[j - f];
            const float* const row = bins[j - j0];
#pragma unroll
            for (int q = 0; q < kLctBinsPerLane; ++q)
                if (wave + q * kWaves < zn) acc[q] = fmaf(wj, row[wave + q * kWaves], acc[q]);
        }
    }
    const int i = i0 + lane;
    if (i < a.nv) {
#pragma unroll
        for (int q = 0; q < kLctBinsPerLane; ++q) {
            const int m = m0 + wave + q * kWaves;
            if (m < a.H) {
                for (int img = 0; img < 8; ++img) {         // (m, n, i) and its images in the padding
                    const size_t mm = m + (img & 4 ? a.H : 0), nn = n + (img & 2 ? a.W : 0), ii = i + (img & 1 ? a.nv : 0);
                    a.pad[(mm * Nx + nn) * Nv + ii] = make_float2(img == 0 ? acc[q] : 0.0f, 0.0f);
                }
            }
        }
    }
}

struct LctStoreRowsArgs {
    const float2* field;   // [Nz][Nx][Nv]
    const int* perm;
    const int* first;      // [nr]: the tables of R^T
    const int* start;      // [nr + 1]
    const float* weight;   // [nnz]
    float* rows;           // [H W][nr]
    int H, W, nr, nv, nnz, sm, sn, power;
    float r0, dr;
};

// one workgroup per lattice point (m, n)
__global__ __launch_bounds__(kBlock) void lct_store_rows_kernel(LctStoreRowsArgs a) {
    __shared__ float cells[kLctMaxCells];
    const int m = blockIdx.x / a.W, n = blockIdx.x - m * a.W;
    const float2* const col = a.field + ((size_t)m * (2 * (size_t)a.W) + n) * (2 * (size_t)a.nv);
    for (int i = threadIdx.x; i < a.nv; i += kBlock) cells[i] = col[i].x;
    __syncthreads();
    float* const row = a.rows + (size_t)lattice_row(a.perm, m, n, a.sm, a.sn, a.H, a.W) * a.nr;
    for (int j = threadIdx.x; j < a.nr; j += kBlock) {
        const LctRun r = lct_run(a.first, a.start, j, a.nv, a.nnz);
        float acc = 0.0f;
        for (int q = 0; q < r.cnt; ++q) acc = fmaf(a.weight[r.s + q], cells[r.f + q], acc);
        row[j] = acc * lct_weight(a.power, j, a.r0, a.dr);
    }
}

int lct_check_extents(int32_t H, int32_t W, int32_t nr, int32_t nv) {
    if (lattice_check_extents("LCT extents H, W, nr", H, W, nr) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (nv < 1 || nv > kLctMaxCells) return set_err(NLOSGR_E_INVALID, "LCT cell count nv must be in 1..2048");
    return NLOSGR_OK;
}

int lct_check_tables(const int32_t* first, const int32_t* start, const float* weight, int32_t nnz, int32_t nr,
                     int32_t nv) {
    if (nnz < 1 || nnz > nr + nv) return set_err(NLOSGR_E_INVALID, "the resampling tables hold 1..nv + nr weights");
    if (!first || !start || !weight) return set_err(NLOSGR_E_INVALID, "null resampling table pointer");
    return NLOSGR_OK;
}

// the lattice arguments of load, load_rows and store_rows; `lo` is the smallest power the pass takes
int lct_check_lattice(int32_t H, int32_t W, int32_t stride_m, int32_t stride_n, float r0, float dr, int32_t power,
                      int32_t lo) {
    if (power < lo || power > 4)
        return set_err(NLOSGR_E_INVALID, lo < 0 ? "LCT power must be in -4..4" : "LCT power must be in 0..4");
    if (lattice_check_window(r0, (double)dr) != NLOSGR_OK) return NLOSGR_E_INVALID;
    return lattice_check_strides(H, W, stride_m, stride_n);
}

int lct_load_launch(bool sign, const float* rows, const int32_t* perm, int32_t H, int32_t W, int32_t nr, int32_t nv,
                    int32_t stride_m, int32_t stride_n, float r0, float dr, int32_t power, const int32_t* first,
                    const int32_t* start, const float* weight, int32_t nnz, float* pad, void* hip_stream) {
    if (lct_check_extents(H, W, nr, nv) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (lct_check_lattice(H, W, stride_m, stride_n, r0, dr, power, sign ? -4 : 0) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (lct_check_tables(first, start, weight, nnz, nr, nv) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (!rows) return set_err(NLOSGR_E_INVALID, "null rows pointer");
    if (!pad) return set_err(NLOSGR_E_INVALID, "null padded array pointer");
    if ((uintptr_t)pad % 16) return set_err(NLOSGR_E_INVALID, "the padded array must be 16-byte aligned");
    LctLoadArgs a;
    a.rows = rows; a.perm = perm; a.first = first; a.start = start; a.weight = weight;
    a.H = H; a.W = W; a.nr = nr; a.nv = nv; a.nnz = nnz; a.sm = stride_m; a.sn = stride_n;
    a.r0 = r0; a.dr = dr; a.power = power; a.pad = (float4*)pad;
    const unsigned ncol = 4u * (unsigned)H * (unsigned)W;      // <= 2^22
    hipStream_t s = (hipStream_t)hip_stream;
    dispatch_int<kLctSigned, 4>(sign ? kLctSigned : power, [&](auto P) {
        hipLaunchKernelGGL(lct_load_kernel<decltype(P)::value>, dim3(ncol), dim3(kBlock), 0, s, a);
    });
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

int lct_store_launch(bool clamp, const float* field, int32_t H, int32_t W, int32_t nr, int32_t nv, const int32_t* first,
                     const int32_t* start, const float* weight, int32_t nnz, float* volume, void* hip_stream) {
    if (lct_check_extents(H, W, nr, nv) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (lct_check_tables(first, start, weight, nnz, nr, nv) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (!field) return set_err(NLOSGR_E_INVALID, "null field pointer");
    if (!volume) return set_err(NLOSGR_E_INVALID, "null volume pointer");
    if ((uintptr_t)field % 8) return set_err(NLOSGR_E_INVALID, "the field must be 8-byte aligned");
    if ((const void*)field == (const void*)volume) return set_err(NLOSGR_E_INVALID, "the volume must not alias the field");
    LctStoreArgs a;
    a.field = (const float2*)field; a.first = first; a.start = start; a.weight = weight; a.vol = volume;
    a.H = H; a.W = W; a.nr = nr; a.nv = nv; a.nnz = nnz;
    const dim3 grid((nr + kLctTile - 1) / kLctTile, (H + kLctTile - 1) / kLctTile, W);
    if (clamp) hipLaunchKernelGGL(lct_store_kernel<true>, grid, dim3(kBlock), 0, (hipStream_t)hip_stream, a);
    else hipLaunchKernelGGL(lct_store_kernel<false>, grid, dim3(kBlock), 0, (hipStream_t)hip_stream, a);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

}  // namespace

extern "C" {

int nlosgr_lct_load(const float* rows, const int32_t* perm, int32_t H, int32_t W, int32_t nr, int32_t nv,
                    int32_t stride_m, int32_t stride_n, float r0, float dr, int32_t power, const int32_t* first,
                    const int32_t* start, const float* weight, int32_t nnz, float* pad, void* hip_stream) {
    return lct_load_launch(false, rows, perm, H, W, nr, nv, stride_m, stride_n, r0, dr, power, first, start, weight,
                           nnz, pad, hip_stream);
}

int nlosgr_lct_load_rows(const float* rows, const int32_t* perm, int32_t H, int32_t W, int32_t nr, int32_t nv,
                         int32_t stride_m, int32_t stride_n, float r0, float dr, int32_t power, const int32_t* first,
                         const int32_t* start, const float* weight, int32_t nnz, float* pad, void* hip_stream) {
    return lct_load_launch(true, rows, perm, H, W, nr, nv, stride_m, stride_n, r0, dr, power, first, start, weight,
                           nnz, pad, hip_stream);
}

int nlosgr_lct_load_volume(const float* volume, int32_t H, int32_t W, int32_t nr, int32_t nv, const int32_t* first,
                           const int32_t* start, const float* weight, int32_t nnz, float* pad, void* hip_stream) {
    if (lct_check_extents(H, W, nr, nv) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (lct_check_tables(first, start, weight, nnz, nr, nv) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (!volume) return set_err(NLOSGR_E_INVALID, "null volume pointer");
    if (!pad) return set_err(NLOSGR_E_INVALID, "null padded array pointer");
    if ((uintptr_t)pad % 8) return set_err(NLOSGR_E_INVALID, "the padded array must be 8-byte aligned");
    if ((const void*)volume == (const void*)pad)
        return set_err(NLOSGR_E_INVALID, "the padded array must not alias the volume");
    LctLoadVolumeArgs a;
    a.vol = volume; a.first = first; a.start = start; a.weight = weight; a.pad = (float2*)pad;
    a.H = H; a.W = W; a.nr = nr; a.nv = nv; a.nnz = nnz;
    const dim3 grid((nv + kLctTile - 1) / kLctTile, (H + kLctTile - 1) / kLctTile, W);
    hipLaunchKernelGGL(lct_load_volume_kernel, grid, dim3(kBlock), 0, (hipStream_t)hip_stream, a);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

int nlosgr_lct_store_rows(const float* field, const int32_t* perm, int32_t H, int32_t W, int32_t nr, int32_t nv,
                          int32_t stride_m, int32_t stride_n, float r0, float dr, int32_t power, const int32_t* first,
                          const int32_t* start, const float* weight, int32_t nnz, float* rows, void* hip_stream) {
    if (lct_check_extents(H, W, nr, nv) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (lct_check_lattice(H, W, stride_m, stride_n, r0, dr, power, -4) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (lct_check_tables(first, start, weight, nnz, nr, nv) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (!field) return set_err(NLOSGR_E_INVALID, "null field pointer");
    if (!rows) return set_err(NLOSGR_E_INVALID, "null rows pointer");
    if ((uintptr_t)field % 8) return set_err(NLOSGR_E_INVALID, "the field must be 8-byte aligned");
    if ((const void*)field == (const void*)rows) return set_err(NLOSGR_E_INVALID, "the rows must not alias the field");
    LctStoreRowsArgs a;
    a.field = (const float2*)field; a.perm = perm; a.first = first; a.start = start; a.weight = weight; a.rows = rows;
    a.H = H; a.W = W; a.nr = nr; a.nv = nv; a.nnz = nnz; a.sm = stride_m; a.sn = stride_n; a.power = power;
    a.r0 = r0; a.dr = dr;
    hipLaunchKernelGGL(lct_store_rows_kernel, dim3((unsigned)H * (unsigned)W), dim3(kBlock), 0,
                       (hipStream_t)hip_stream, a);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

int nlosgr_lct_kernel(int32_t H, int32_t W, int32_t nv, float sx, float sz, double dv, double scale, float* K,
                      void* hip_stream) {
    if (lct_check_extents(H, W, 1, nv) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (!lattice_positive((double)sx) || !lattice_positive((double)sz))   // (in double, as dv and scale are)
        return set_err(NLOSGR_E_INVALID, "sx and sz must be finite and > 0");
    if (!lattice_positive(dv)) return set_err(NLOSGR_E_INVALID, "dv must be finite and > 0");
    if (!lattice_positive(scale)) return set_err(NLOSGR_E_INVALID, "the kernel's scale must be finite and > 0");
    if (!K) return set_err(NLOSGR_E_INVALID, "null kernel array pointer");
    if ((uintptr_t)K % 16) return set_err(NLOSGR_E_INVALID, "the kernel array must be 16-byte aligned");
    LctKernelArgs a;
    a.K = (float4*)K; a.H = H; a.W = W; a.nv = nv; a.sx = sx; a.sz = sz; a.dv = dv; a.scale = scale;
    hipLaunchKernelGGL(lct_kernel_kernel, dim3(4u * (unsigned)H * (unsigned)W), dim3(kBlock), 0,
                       (hipStream_t)hip_stream, a);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

int nlosgr_lct_filter(const float* kf, const float* spec, int32_t H, int32_t W, int32_t nv, float snr, int32_t mode,
                      float* out, void* hip_stream) {
    if (lct_check_extents(H, W, 1, nv) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (mode < kLctWiener || mode > kLctGiven)
        return set_err(NLOSGR_E_INVALID, "LCT filter mode must be 0 (Wiener), 1 (back-projection) or 2 (a given inverse)");
    if (mode == kLctWiener && !lattice_positive((double)snr))
        return set_err(NLOSGR_E_INVALID, "snr must be finite and > 0");
    if (!kf) return set_err(NLOSGR_E_INVALID, "null kernel spectrum pointer");
    if (!out) return set_err(NLOSGR_E_INVALID, "null filter output pointer");
    if (!spec && mode == kLctGiven)
        return set_err(NLOSGR_E_INVALID, "a given inverse needs a spectrum to apply it to (null spectrum pointer)");
    if ((uintptr_t)kf % 16 || (uintptr_t)spec % 16 || (uintptr_t)out % 16)
        return set_err(NLOSGR_E_INVALID, "the filter's arrays must be 16-byte aligned");
    LctFilterArgs a;
    a.kf = (const float4*)kf; a.spec = (const float4*)spec; a.out = (float4*)out; a.nv = nv;
    a.inv_snr = mode == kLctWiener ? (float)(1.0 / (double)snr) : 0.0f;
    const dim3 grid(4u * (unsigned)H * (unsigned)W);
    hipStream_t s = (hipStream_t)hip_stream;
#define LCT_FILTER(M)                                                                               \
    do {                                                                                            \
        if (spec) hipLaunchKernelGGL((lct_filter_kernel<M, true>), grid, dim3(kBlock), 0, s, a);    \
        else hipLaunchKernelGGL((lct_filter_kernel<M, false>), grid, dim3(kBlock), 0, s, a);        \
    } while (0)
    switch (mode) {
        case kLctWiener: LCT_FILTER(kLctWiener); break;
        case kLctBackprop: LCT_FILTER(kLctBackprop); break;
        default: hipLaunchKernelGGL((lct_filter_kernel<kLctGiven, true>), grid, dim3(kBlock), 0, s, a); break;
    }
#undef LCT_FILTER
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

int nlosgr_lct_store(const float* field, int32_t H, int32_t W, int32_t nr, int32_t nv, const int32_t* first,
                     const int32_t* start, const float* weight, int32_t nnz, float* volume, void* hip_stream) {
    return lct_store_launch(true, field, H, W, nr, nv, first, start, weight, nnz, volume, hip_stream);
}

int nlosgr_lct_store_volume(const float* field, int32_t H, int32_t W, int32_t nr, int32_t nv, const int32_t* first,
                            const int32_t* start, const float* weight, int32_t nnz, float* volume, void* hip_stream) {
    return lct_store_launch(false, field, H, W, nr, nv, first, start, weight, nnz, volume, hip_stream);
}

}  // extern "C"
