// f-k migration of a confocal capture (Lindell, Wetzstein, O'Toole 2019; gfx950): the three passes between the
// two FFTs of   rows -> amplitude -> zero-padded 3-D FFT -> Stolt resampling -> inverse FFT -> |.|^2.
// The FFTs themselves are the caller's (torch.fft: hipFFT); this library links the HIP runtime alone.  The work
// arrays are complex64 [Nz][Nx][Nt] (interleaved re, im) with Nz = 2 H, Nx = 2 W, Nt = 2 nr; lattice point (m, n)
// is measured at (xs[n], y0, zs[m]) and its row is rows[perm[m sm + n sn]] (perm NULL: rows[m sm + n sn]).
//
//   nlosgr_fk_load    pad[m][n][j] = (psi, 0),  psi = max(rows[v][j], 0) (r0 + j dr)^power, its square root when
//                     `amplitude`; zero for m >= H, n >= W or j >= nr.  fp32: r = fma(j, dr, r0), the power as
//                     r, r r, (r r) r, (r r)(r r), the hardware square root (1 ulp): fk_psi of nlosgr_lattice.hpp.
//   nlosgr_fk_stolt   with signed DFT indices c (z), b (x), a (time), gx = Nt dr / (Nx sx), gz = Nt dr / (Nz sz):
//                         src = sqrt(a^2 + (gx b)^2 + (gz c)^2),  k = floor(src),  f = src - k
//                         V[c][b][a] = ((1-f) S[c][b][k] + f S[c][b][k+1]) (a / src) exp(-2 pi i (src - a) (r0/dr) / Nt)
//                     where a > 0 and k + 1 <= Nt/2 - 1, and V = 0 everywhere else.  src, k, f, a / src and the
//                     phase's fraction of a turn are formed in fp64 (one square root per bin: the pass stays
//                     bandwidth-bound), so they stay accurate at Nt = 2048 and r0 / dr in the hundreds; the
//                     interpolation and the complex product are fp32; the sine and cosine are sincospif of the
//                     reduced fraction.
//   nlosgr_fk_store   volume[n][j][m] = re^2 + im^2 of o[m][n][j] for m < H, n < W, j < nr: fmaf(im, im, re * re).
//
// Shape.  All three are single passes: one read and one write of the work array, 8- or 16-byte coalesced, no
// atomics, every output element written by exactly one lane from inputs alone, so results are bitwise repeatable.
// load and stolt give a workgroup one (c, b) column; a lane writes two adjacent complex bins (16 bytes), the zeros
// of the padding and of the masked band included, so neither needs a memset.  In stolt src grows with a at a slope
// <= 1, so the 16-byte reads (S[k], S[k+1]) of a wave cover one contiguous span of the column, already in cache
// from the neighbouring waves.  store transposes (time <-> z) through a 64 x 64 LDS tile padded to 65 floats a
// row: lanes run along time for the 8-byte reads and along z for the writes (16, 8 or 4 bytes per lane as H
// divides by 4, 2 or not).
#include "nlosgr_common.hpp"
#include "nlosgr_lattice.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

constexpr int kFkTile = 64;          // store: tile edge along time and along z

struct FkLoadArgs {
    const float* rows;
    const int* perm;
    int H, W, nr, sm, sn;
    float r0, dr;
    float4* pad;           // [Nz * Nx][nr]: two complex bins each
};

// VEC2: rows are 8-byte aligned and nr is even, so a lane's two bins come from one 8-byte read
template <int POWER, bool AMP, bool VEC2>
__global__ __launch_bounds__(kBlock) void fk_load_kernel(FkLoadArgs a) {
    const int Nx = 2 * a.W;
    const int c = blockIdx.x / Nx, b = blockIdx.x - c * Nx;
    float4* const col = a.pad + (size_t)blockIdx.x * a.nr;
    const float* row = nullptr;
    if (c < a.H && b < a.W) {
        const int v = lattice_row(a.perm, c, b, a.sm, a.sn, a.H, a.W);
        row = a.rows + (size_t)v * a.nr;
    }
    for (int p = threadIdx.x; p < a.nr; p += kBlock) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        const int j = 2 * p;
        if (row && j < a.nr) {
            if (VEC2) {
                const float2 h = *(const float2*)(row + j);
                o.x = fk_psi<POWER, AMP>(h.x, j, a.r0, a.dr);
                o.z = fk_psi<POWER, AMP>(h.y, j + 1, a.r0, a.dr);
            } else {
                o.x = fk_psi<POWER, AMP>(row[j], j, a.r0, a.dr);
                if (j + 1 < a.nr) o.z = fk_psi<POWER, AMP>(row[j + 1], j + 1, a.r0, a.dr);
            }
        }
        col[p] = o;
    }
}

struct FkStoltArgs {
    const float* spec;     // [Nz * Nx][Nt][2]
    float4* out;           // [Nz * Nx][nr]: two complex bins each
    int H, W, nr;
    double gx, gz, qn;     // qn = (r0 / dr) / Nt
};

// two adjacent complex bins in one 16-byte read (8-byte aligned)
struct __attribute__((packed, aligned(8))) FkBins {
    float re0, im0, re1, im1;
};

// V[c][b][a] of the column at `in` (lat2 = (gx b)^2 + (gz c)^2), 0 <= a <= nr
__device__ __forceinline__ float2 fk_stolt_bin(const float* in, int a, int nr, double lat2, double qn) {
    const double src = sqrt((double)a * (double)a + lat2);
    const double kf = floor(src);
    if (!(a >= 1 && kf + 1.0 <= (double)(nr - 1))) return make_float2(0.f, 0.f);   // (a NaN src: no light)
    const int k = (int)kf;                         // 1 <= k <= nr - 2: both bins inside the positive band
    const float f = (float)(src - kf);
    const FkBins v = *(const FkBins*)(in + 2 * (size_t)k);
    double t = (src - (double)a) * qn;
    t -= floor(t);                                 // the phase as a fraction of a turn in [0, 1)
    float sn, cs;
    sincospif(2.0f * (float)t, &sn, &cs);
    const float w = (float)((double)a / src);
    const float re = w * fmaf(f, v.re1, (1.0f - f) * v.re0);
    const float im = w * fmaf(f, v.im1, (1.0f - f) * v.im0);
    // (re + i im) (cs - i sn)
    return make_float2(fmaf(re, cs, im * sn), fmaf(im, cs, -(re * sn)));
}

__global__ __launch_bounds__(kBlock) void fk_stolt_kernel(FkStoltArgs a) {
    const int Nx = 2 * a.W;
    const int ci = blockIdx.x / Nx, bi = blockIdx.x - ci * Nx;
    const int c = dft_signed(ci, a.H), b = dft_signed(bi, a.W);
    const double lb = a.gx * (double)b, lc = a.gz * (double)c;
    const double lat2 = lb * lb + lc * lc;
    const float* const in = a.spec + (size_t)blockIdx.x * a.nr * 4;
    float4* const col = a.out + (size_t)blockIdx.x * a.nr;
    // pair p holds DFT bins 2p and 2p + 1; the bins from Nt/2 = nr on are the negative band (and Nyquist): zero
    for (int p = threadIdx.x; p < a.nr; p += kBlock) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        const int i = 2 * p;
        if (i < a.nr) {
            const float2 v0 = fk_stolt_bin(in, i, a.nr, lat2, a.qn);
            const float2 v1 = fk_stolt_bin(in, i + 1, a.nr, lat2, a.qn);
            o = make_float4(v0.x, v0.y, v1.x, v1.y);
        }
        col[p] = o;
    }
}

struct FkStoreArgs {
    const float2* field;   // [Nz][Nx][Nt]
    float* vol;            // [W][nr][H]
    int H, W, nr;
};

// block (jt, mt, n): the tile j in [64 jt, +64), m in [64 mt, +64) of wall column n.  VEC floats per lane written
template <int VEC>
__global__ __launch_bounds__(kBlock) void fk_store_kernel(FkStoreArgs a) {
    __shared__ float tile[kFkTile][kFkTile + 1];
    const int t = threadIdx.x;
    const int j0 = blockIdx.x * kFkTile, m0 = blockIdx.y * kFkTile, n = blockIdx.z;
    const size_t Nx = 2 * (size_t)a.W, Nt = 2 * (size_t)a.nr;
    {
        const int jj = t & 63, j = j0 + jj;
        for (int mm = t >> 6; mm < kFkTile; mm += kWaves) {
            const int m = m0 + mm;
            if (m < a.H && j < a.nr) {
                const float2 o = a.field[((size_t)m * Nx + n) * Nt + j];
                tile[jj][mm] = fmaf(o.y, o.y, o.x * o.x);
            }
        }
    }
    __syncthreads();
    constexpr int kLanes = kFkTile / VEC;            // lanes per output row of the tile
    const int mm = (t % kLanes) * VEC, m = m0 + mm;
    for (int jj = t / kLanes; jj < kFkTile; jj += kBlock / kLanes) {
        const int j = j0 + jj;
        if (m < a.H && j < a.nr) {                   // H % VEC == 0: the lane's VEC voxels are inside together
            float* const dst = a.vol + ((size_t)n * a.nr + j) * a.H + m;
            if (VEC == 4) *(float4*)dst = make_float4(tile[jj][mm], tile[jj][mm + 1], tile[jj][mm + 2], tile[jj][mm + 3]);
            else if (VEC == 2) *(float2*)dst = make_float2(tile[jj][mm], tile[jj][mm + 1]);
            else *dst = tile[jj][mm];
        }
    }
}

constexpr const char* kFkExtents = "f-k extents H, W, nr";

}  // namespace

extern "C" {

int nlosgr_fk_load(const float* rows, const int32_t* perm, int32_t H, int32_t W, int32_t nr, int32_t stride_m,
                   int32_t stride_n, float r0, float dr, int32_t power, int32_t amplitude, float* pad,
                   void* hip_stream) {
    if (lattice_check_extents(kFkExtents, H, W, nr) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (power < 0 || power > 4) return set_err(NLOSGR_E_INVALID, "f-k power must be in 0..4");
    if (lattice_check_window(r0, dr) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (lattice_check_strides(H, W, stride_m, stride_n) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (!rows) return set_err(NLOSGR_E_INVALID, "null rows pointer");
    if (!pad) return set_err(NLOSGR_E_INVALID, "null padded array pointer");
    if ((uintptr_t)pad % 16) return set_err(NLOSGR_E_INVALID, "the padded array must be 16-byte aligned");
    FkLoadArgs a;
    a.rows = rows; a.perm = perm; a.H = H; a.W = W; a.nr = nr; a.sm = stride_m; a.sn = stride_n;
    a.r0 = r0; a.dr = dr; a.pad = (float4*)pad;
    const bool vec2 = nr % 2 == 0 && (uintptr_t)rows % 8 == 0;
    const unsigned ncol = 4u * (unsigned)H * (unsigned)W;      // <= 2^22
    hipStream_t s = (hipStream_t)hip_stream;
    dispatch_int<0, 4>(power, [&](auto P) {
        dispatch_int<0, 1>(amplitude != 0, [&](auto AMP) {
            dispatch_int<0, 1>(vec2, [&](auto VEC2) {
                hipLaunchKernelGGL((fk_load_kernel<decltype(P)::value, decltype(AMP)::value != 0, decltype(VEC2)::value != 0>),
                                   dim3(ncol), dim3(kBlock), 0, s, a);
            });
        });
    });
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

int nlosgr_fk_stolt(const float* spec, int32_t H, int32_t W, int32_t nr, float sx, float sz, float r0, float dr,
                    float* out, void* hip_stream) {
    if (lattice_check_extents(kFkExtents, H, W, nr) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (lattice_check_window(r0, dr) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (!lattice_positive(sx) || !lattice_positive(sz)) return set_err(NLOSGR_E_INVALID, "sx and sz must be finite and > 0");
    if (!spec) return set_err(NLOSGR_E_INVALID, "null spectrum pointer");
    if (!out) return set_err(NLOSGR_E_INVALID, "null migrated spectrum pointer");
    if (out == spec) return set_err(NLOSGR_E_INVALID, "the migrated spectrum must not alias the spectrum");
    if ((uintptr_t)spec % 8 || (uintptr_t)out % 16)
        return set_err(NLOSGR_E_INVALID, "the spectrum must be 8-byte, the migrated spectrum 16-byte aligned");
    FkStoltArgs a;
    a.spec = spec; a.out = (float4*)out; a.H = H; a.W = W; a.nr = nr;
    const double Nt = 2.0 * nr;
    a.gx = Nt * (double)dr / (2.0 * W * (double)sx);
    a.gz = Nt * (double)dr / (2.0 * H * (double)sz);
    a.qn = ((double)r0 / (double)dr) / Nt;
    hipLaunchKernelGGL(fk_stolt_kernel, dim3(4u * (unsigned)H * (unsigned)W), dim3(kBlock), 0, (hipStream_t)hip_stream, a);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

int nlosgr_fk_store(const float* field, int32_t H, int32_t W, int32_t nr, float* volume, void* hip_stream) {
    if (lattice_check_extents(kFkExtents, H, W, nr) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (!field) return set_err(NLOSGR_E_INVALID, "null field pointer");
    if (!volume) return set_err(NLOSGR_E_INVALID, "null volume pointer");
    if ((uintptr_t)field % 8) return set_err(NLOSGR_E_INVALID, "the field must be 8-byte aligned");
    FkStoreArgs a;
    a.field = (const float2*)field; a.vol = volume; a.H = H; a.W = W; a.nr = nr;
    const dim3 grid((nr + kFkTile - 1) / kFkTile, (H + kFkTile - 1) / kFkTile, W);
    hipStream_t s = (hipStream_t)hip_stream;
    if (H % 4 == 0 && (uintptr_t)volume % 16 == 0)
        hipLaunchKernelGGL(fk_store_kernel<4>, grid, dim3(kBlock), 0, s, a);
    else if (H % 2 == 0 && (uintptr_t)volume % 8 == 0)
        hipLaunchKernelGGL(fk_store_kernel<2>, grid, dim3(kBlock), 0, s, a);
    else
        hipLaunchKernelGGL(fk_store_kernel<1>, grid, dim3(kBlock), 0, s, a);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

}  // extern "C"
