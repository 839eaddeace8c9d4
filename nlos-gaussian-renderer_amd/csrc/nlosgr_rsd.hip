// Fast phasor-field reconstruction (gfx950): the phasor field evaluated as Rayleigh-Sommerfeld diffraction (Liu,
// Bauer, Velten 2020).  For one depth plane and one temporal frequency the sum over the wall points is a 2-D
// convolution over the wall's lattice, done by FFT.  The FFTs are the caller's (torch.fft: hipFFT); this library
// links the HIP runtime alone.  The four passes around them (include/nlosgr.h states every formula):
//
//   nlosgr_rsd_load     Pw[q][m][n] = coef[q] S[row(m, n)][q_lo + q] at [0:H][0:W] of a zero [nq][2H][2W]: the
//                       measurement-major spectrum as frequency-major padded images.  A 32 x 32 LDS tile (33 complex a
//                       row): lanes run along q for the reads and along n for the writes; the padding is written in
//                       the same pass.  One fp32 complex product: re = fma(cr, sr, -(ci si)), im = fma(cr, si, ci sr).
//   nlosgr_rsd_kernel   K[j][q][a][b] = d^e exp(2 pi i frac(g (q_lo + q) (d / dr) / Nt)) with the signed offsets a', b'
//                       of the padded image, d = sqrt((a' sz)^2 + (b' sx)^2 + D_j^2), and 0 at a' = -H or b' = -W.
//                       One lane per (j, a, two adjacent b): d, d^e and x = g (d / dr) / Nt are formed once in fp64,
//                       then per q the turn count q x is reduced in fp64 (t = q x - floor(q x)) and only the fraction
//                       goes to fp32 sincospif, as fk_stolt_bin does: the phase reaches thousands of radians, and an
//                       fp32 phase would cost 1e-4 rad.  d^e is one fp64 square root and products, rounded once.
//                       16-byte stores, coalesced along b, at a stride of one image per q.
//   nlosgr_rsd_apply    out[j][q] = Kf[j][q] Pf[q], two complex per lane (16-byte accesses), in place when out is Kf.
//   nlosgr_rsd_gather   Phi[n][j][m] = dl^(power/2) sum_q exp(2 pi i frac((q_lo + q) (dl / dr) / (2 Nt))) o[j][q][m][n]
//                       (without a laser: the plain sum), q ascending, fp32 fma accumulation; dl and its turn rate in
//                       fp64 once per voxel, outside the q loop.  One voxel per lane, 1024 lanes a block: lanes run
//                       along n for the 8-byte reads; a 32 x 32 LDS tile (33 floats a row) turns the block so the
//                       writes of planes and mag run along m.
//
// No atomics; every output element is written by exactly one lane from the inputs alone: bitwise repeatable.
#include "nlosgr_common.hpp"
#include "nlosgr_lattice.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

constexpr int kRsdMaxNt = 8192;      // DFT length of the rows
constexpr int kRsdMaxBand = 512;     // frequencies in the band
constexpr int kRsdTile = 32;         // load, gather: tile edge
constexpr int kRsdGatherBlock = kRsdTile * kRsdTile;   // gather: one voxel per lane

// d^(halves / 2), halves 0..8: one square root and products in fp64, rounded once
__device__ __forceinline__ float rsd_amp(double d, int halves) {
    double p = (halves & 1) ? sqrt(d) : 1.0;
    for (int i = 0; i < (halves >> 1); ++i) p *= d;
    return (float)p;
}

// exp(2 pi i frac(q x)): the turn count in fp64, its fraction to fp32 sincospif
__device__ __forceinline__ void rsd_phase(double x, int q, float& sn, float& cs) {
    double t = (double)q * x;
    t -= floor(t);
    sincospif(2.0f * (float)t, &sn, &cs);
}

struct RsdLoadArgs {
    const float2* spec;    // [H W][nf]
    const int* perm;
    const float2* coef;    // [nq]
    float2* pw;            // [nq][2H][2W]
    int H, W, nf, q_lo, nq, sm, sn;
};

// block (nt, m, qt): the tile n in [32 nt, +32), q in [32 qt, +32) of padded row m
__global__ __launch_bounds__(kBlock) void rsd_load_kernel(RsdLoadArgs a) {
    __shared__ float2 tile[kRsdTile][kRsdTile + 1];
    const int t = threadIdx.x;
    const int n0 = blockIdx.x * kRsdTile, m = blockIdx.y, q0 = blockIdx.z * kRsdTile;
    const bool data = m < a.H && n0 < a.W;        // (uniform over the block)
    if (data) {
        const int qq = t & 31, q = q0 + qq;
        for (int nn = t >> 5; nn < kRsdTile; nn += kBlock / 32) {
            const int n = n0 + nn;
            if (n < a.W && q < a.nq) {
                const int v = lattice_row(a.perm, m, n, a.sm, a.sn, a.H, a.W);
                const float2 s = a.spec[(size_t)v * a.nf + a.q_lo + q];
                const float2 c = a.coef[q];
                tile[nn][qq] = make_float2(fmaf(c.x, s.x, -(c.y * s.y)), fmaf(c.x, s.y, c.y * s.x));
            }
        }
    }
    __syncthreads();
    const int nn = t & 31, n = n0 + nn;
    const size_t Nz = 2 * (size_t)a.H, Nx = 2 * (size_t)a.W;
    for (int qq = t >> 5; qq < kRsdTile; qq += kBlock / 32) {
        const int q = q0 + qq;
        if (n < 2 * a.W && q < a.nq)
            a.pw[((size_t)q * Nz + m) * Nx + n] = (data && n < a.W) ? tile[nn][qq] : make_float2(0.f, 0.f);
    }
}

struct RsdKernelArgs {
    const float* ys;       // [ny]
    float4* K;             // [nj][nq][2H][W]: two complex each
    int H, W, nq, q_lo, j0, halves;
    float y0;
    double sx, sz, turn;   // turn = g / (dr Nt)
};

__global__ __launch_bounds__(kBlock) void rsd_kernel_kernel(RsdKernelArgs a) {
    const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;     // (a, pair of b) of one image
    const unsigned npair = 2u * (unsigned)a.H * (unsigned)a.W;
    if (idx >= npair) return;
    const int j = blockIdx.y;
    const int ai = (int)(idx / (unsigned)a.W), pb = (int)(idx - (unsigned)ai * (unsigned)a.W);
    const int ap = dft_signed(ai, a.H);
    const double D = (double)a.ys[a.j0 + j] - (double)a.y0;
    const double za = (double)ap * a.sz;
    double x[2];
    float amp[2];
    bool zero[2];
    for (int e = 0; e < 2; ++e) {
        const int bi = 2 * pb + e;
        const int bp = dft_signed(bi, a.W);
        zero[e] = ap == -a.H || bp == -a.W;
        const double xb = (double)bp * a.sx;
        const double d = sqrt(za * za + xb * xb + D * D);
        x[e] = d * a.turn;
        amp[e] = rsd_amp(d, a.halves);
    }
    float4* out = a.K + (size_t)j * a.nq * npair + idx;
    for (int q = 0; q < a.nq; ++q) {
        float s0, c0, s1, c1;
        rsd_phase(x[0], a.q_lo + q, s0, c0);
        rsd_phase(x[1], a.q_lo + q, s1, c1);
        float4 o;
        o.x = zero[0] ? 0.f : amp[0] * c0;
        o.y = zero[0] ? 0.f : amp[0] * s0;
        o.z = zero[1] ? 0.f : amp[1] * c1;
        o.w = zero[1] ? 0.f : amp[1] * s1;
        out[(size_t)q * npair] = o;
    }
}

struct RsdApplyArgs {
    const float4* pf;      // [nq][2H][W]: two complex each
    const float4* kf;      // [nj][nq][2H][W]
    float4* out;
    unsigned npair;        // nq 2H W
};

__global__ __launch_bounds__(kBlock) void rsd_apply_kernel(RsdApplyArgs a) {
    const unsigned idx = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (idx >= a.npair) return;
    const float4 p = a.pf[idx];
    const size_t off = (size_t)blockIdx.y * a.npair + idx;
    const float4 k = a.kf[off];
    a.out[off] = make_float4(fmaf(k.x, p.x, -(k.y * p.y)), fmaf(k.x, p.y, k.y * p.x),
                             fmaf(k.z, p.z, -(k.w * p.w)), fmaf(k.z, p.w, k.w * p.z));
}

struct RsdGatherArgs {
    const float2* field;   // [nj][nq][2H][2W]
    const float *xs, *ys, *zs;
    float* planes;         // [2][W][ny][H]
    float* mag;            // [W][ny][H] or NULL
    int H, W, nq, q_lo, ny, j0, halves;
    float lx, ly, lz;
    double turn;           // 1 / (2 dr Nt)
};

// block (nt, mt, j): the tile n in [32 nt, +32), m in [32 mt, +32) of depth plane j0 + j, one voxel per lane (1024
// lanes: a chunk of few planes is a grid of few blocks, and each lane's q loop is a chain of dependent adds)
template <bool LASER>
__global__ __launch_bounds__(kRsdGatherBlock) void rsd_gather_kernel(RsdGatherArgs a) {
    __shared__ float tre[kRsdTile][kRsdTile + 1], tim[kRsdTile][kRsdTile + 1];
    const int t = threadIdx.x;
    const int n0 = blockIdx.x * kRsdTile, m0 = blockIdx.y * kRsdTile, j = blockIdx.z;
    const size_t Nz = 2 * (size_t)a.H, Nx = 2 * (size_t)a.W;
    {
        const int nn = t & 31, mm = t >> 5, n = n0 + nn, m = m0 + mm;
        float re = 0.f, im = 0.f, amp = 1.f;
        if (n < a.W && m < a.H) {
            double x = 0.0;
            if (LASER) {
                const double dx = (double)a.xs[n] - (double)a.lx, dy = (double)a.ys[a.j0 + j] - (double)a.ly,
                             dz = (double)a.zs[m] - (double)a.lz;
                const double dl = sqrt(dx * dx + dy * dy + dz * dz);
                x = dl * a.turn;
                amp = rsd_amp(dl, a.halves);
            }
            const float2* img = a.field + ((size_t)j * a.nq * Nz + m) * Nx + n;
#pragma unroll 4
            for (int q = 0; q < a.nq; ++q) {
                const float2 o = img[(size_t)q * Nz * Nx];
                if (LASER) {
                    float sn, cs;
                    rsd_phase(x, a.q_lo + q, sn, cs);
                    re = fmaf(-sn, o.y, fmaf(cs, o.x, re));
                    im = fmaf(sn, o.x, fmaf(cs, o.y, im));
                } else {
                    re += o.x;
                    im += o.y;
                }
            }
        }
        tre[nn][mm] = LASER ? amp * re : re;
        tim[nn][mm] = LASER ? amp * im : im;
    }
    __syncthreads();
    const int mm = t & 31, nn = t >> 5, m = m0 + mm, n = n0 + nn;
    if (n < a.W && m < a.H) {
        const size_t off = ((size_t)n * a.ny + a.j0 + j) * a.H + m;
        const float re = tre[nn][mm], im = tim[nn][mm];
        a.planes[off] = re;
        a.planes[(size_t)a.W * a.ny * a.H + off] = im;
        if (a.mag) a.mag[off] = (float)sqrt((double)re * re + (double)im * im);
    }
}

constexpr const char* kRsdExtents = "RSD lattice extents H, W";

int rsd_check_band(int32_t Nt, int32_t q_lo, int32_t nq) {
    if (Nt < 2 || Nt > kRsdMaxNt || Nt % 2) return set_err(NLOSGR_E_INVALID, "Nt must be even and in 2..8192");
    if (nq < 1 || nq > kRsdMaxBand || q_lo < 1 || (long long)q_lo + nq - 1 > Nt / 2 - 1)
        return set_err(NLOSGR_E_INVALID, "the band [q_lo, q_lo + nq) must lie in [1, Nt/2 - 1] and hold 1..512 frequencies");
    return NLOSGR_OK;
}

int rsd_check_planes(int32_t ny, int32_t j0, int32_t nj) {
    if (ny < 1 || ny > kLatticeMaxExtent) return set_err(NLOSGR_E_INVALID, "ny must be in 1..1024");
    if (j0 < 0 || nj < 1 || (long long)j0 + nj > ny)
        return set_err(NLOSGR_E_INVALID, "the depth planes [j0, j0 + nj) must lie in [0, ny) and hold at least one");
    return NLOSGR_OK;
}

bool rsd_overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
}

}  // namespace

extern "C" {

int nlosgr_rsd_load(const float* spec, const int32_t* perm, const float* coef, int32_t H, int32_t W, int32_t Nt,
                    int32_t q_lo, int32_t nq, int32_t stride_m, int32_t stride_n, float* pw, void* hip_stream) {
    if (lattice_check_extents(kRsdExtents, H, W, 1) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (rsd_check_band(Nt, q_lo, nq) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (lattice_check_strides(H, W, stride_m, stride_n) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (!spec) return set_err(NLOSGR_E_INVALID, "null spectrum pointer");
    if (!coef) return set_err(NLOSGR_E_INVALID, "null band coefficient pointer");
    if (!pw) return set_err(NLOSGR_E_INVALID, "null padded image pointer");
    if ((uintptr_t)spec % 8 || (uintptr_t)coef % 8 || (uintptr_t)pw % 8)
        return set_err(NLOSGR_E_INVALID, "the spectrum, the coefficients and the padded images must be 8-byte aligned");
    RsdLoadArgs a;
    a.spec = (const float2*)spec; a.perm = perm; a.coef = (const float2*)coef; a.pw = (float2*)pw;
    a.H = H; a.W = W; a.nf = Nt / 2 + 1; a.q_lo = q_lo; a.nq = nq; a.sm = stride_m; a.sn = stride_n;
    const dim3 grid((2 * W + kRsdTile - 1) / kRsdTile, 2 * H, (nq + kRsdTile - 1) / kRsdTile);
    hipLaunchKernelGGL(rsd_load_kernel, grid, dim3(kBlock), 0, (hipStream_t)hip_stream, a);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

int nlosgr_rsd_kernel(const float* ys, int32_t ny, int32_t j0, int32_t nj, float y0, int32_t H, int32_t W, float sx,
                      float sz, float dr, int32_t Nt, int32_t q_lo, int32_t nq, int32_t power, int32_t laser,
                      float* K, void* hip_stream) {
    if (lattice_check_extents(kRsdExtents, H, W, 1) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (rsd_check_planes(ny, j0, nj) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (rsd_check_band(Nt, q_lo, nq) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (power < 0 || power > 4) return set_err(NLOSGR_E_INVALID, "RSD power must be in 0..4");
    if (!lattice_positive(dr)) return set_err(NLOSGR_E_INVALID, "dr must be finite and > 0");
    if (!lattice_positive(sx) || !lattice_positive(sz)) return set_err(NLOSGR_E_INVALID, "sx and sz must be finite and > 0");
    if (!(y0 >= -3.0e38f && y0 <= 3.0e38f)) return set_err(NLOSGR_E_INVALID, "y0 must be finite");
    if (!ys) return set_err(NLOSGR_E_INVALID, "null depth table pointer");
    if (!K) return set_err(NLOSGR_E_INVALID, "null kernel array pointer");
    if ((uintptr_t)K % 16) return set_err(NLOSGR_E_INVALID, "the kernel array must be 16-byte aligned");
    RsdKernelArgs a;
    a.ys = ys; a.K = (float4*)K; a.H = H; a.W = W; a.nq = nq; a.q_lo = q_lo; a.j0 = j0;
    a.halves = laser ? power : 2 * power;
    a.y0 = y0; a.sx = (double)sx; a.sz = (double)sz;
    a.turn = (laser ? 0.5 : 1.0) / ((double)dr * (double)Nt);
    const unsigned npair = 2u * (unsigned)H * (unsigned)W;
    hipLaunchKernelGGL(rsd_kernel_kernel, dim3((npair + kBlock - 1) / kBlock, nj), dim3(kBlock), 0,
                       (hipStream_t)hip_stream, a);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

int nlosgr_rsd_apply(const float* kf, const float* pf, int32_t nj, int32_t nq, int32_t H, int32_t W, float* out,
                     void* hip_stream) {
    if (lattice_check_extents(kRsdExtents, H, W, 1) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (nj < 1 || nj > kLatticeMaxExtent) return set_err(NLOSGR_E_INVALID, "the number of depth planes must be in 1..1024");
    if (nq < 1 || nq > kRsdMaxBand) return set_err(NLOSGR_E_INVALID, "the band must hold 1..512 frequencies");
    if (!kf) return set_err(NLOSGR_E_INVALID, "null kernel spectrum pointer");
    if (!pf) return set_err(NLOSGR_E_INVALID, "null image spectrum pointer");
    if (!out) return set_err(NLOSGR_E_INVALID, "null product pointer");
    if ((uintptr_t)kf % 16 || (uintptr_t)pf % 16 || (uintptr_t)out % 16)
        return set_err(NLOSGR_E_INVALID, "the spectra and the product must be 16-byte aligned");
    const size_t image = (size_t)nq * 4 * H * W * 8, all = image * nj;
    if (rsd_overlap(pf, image, out, all))
        return set_err(NLOSGR_E_INVALID, "the product must not alias the image spectrum");
    if (out != kf && rsd_overlap(kf, all, out, all))
        return set_err(NLOSGR_E_INVALID, "the product may alias the kernel spectrum only as a whole (in place)");
    RsdApplyArgs a;
    a.pf = (const float4*)pf; a.kf = (const float4*)kf; a.out = (float4*)out;
    a.npair = (unsigned)nq * 2u * (unsigned)H * (unsigned)W;       // <= 2^30
    hipLaunchKernelGGL(rsd_apply_kernel, dim3((a.npair + kBlock - 1) / kBlock, nj), dim3(kBlock), 0,
                       (hipStream_t)hip_stream, a);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

int nlosgr_rsd_gather(const float* field, int32_t H, int32_t W, int32_t nq, int32_t q_lo, int32_t Nt, float dr,
                      int32_t power, const float* xs, const float* ys, const float* zs, int32_t ny, int32_t j0,
                      int32_t nj, int32_t laser, float lx, float ly, float lz, float* planes, float* mag,
                      void* hip_stream) {
    if (lattice_check_extents(kRsdExtents, H, W, 1) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (rsd_check_planes(ny, j0, nj) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (rsd_check_band(Nt, q_lo, nq) != NLOSGR_OK) return NLOSGR_E_INVALID;
    if (power < 0 || power > 4) return set_err(NLOSGR_E_INVALID, "RSD power must be in 0..4");
    if (!lattice_positive(dr)) return set_err(NLOSGR_E_INVALID, "dr must be finite and > 0");
    if (laser && !(fabsf(lx) <= 3.0e38f && fabsf(ly) <= 3.0e38f && fabsf(lz) <= 3.0e38f))
        return set_err(NLOSGR_E_INVALID, "the laser spot must be finite");
    if (!field) return set_err(NLOSGR_E_INVALID, "null field pointer");
    if (!planes) return set_err(NLOSGR_E_INVALID, "null planes pointer");
    if (laser && (!xs || !ys || !zs)) return set_err(NLOSGR_E_INVALID, "null coordinate table pointer");
    if ((uintptr_t)field % 8) return set_err(NLOSGR_E_INVALID, "the field must be 8-byte aligned");
    RsdGatherArgs a;
    a.field = (const float2*)field; a.xs = xs; a.ys = ys; a.zs = zs; a.planes = planes; a.mag = mag;
    a.H = H; a.W = W; a.nq = nq; a.q_lo = q_lo; a.ny = ny; a.j0 = j0; a.halves = power;
    a.lx = lx; a.ly = ly; a.lz = lz;
    a.turn = 0.5 / ((double)dr * (double)Nt);
    const dim3 grid((W + kRsdTile - 1) / kRsdTile, (H + kRsdTile - 1) / kRsdTile, nj);
    hipStream_t s = (hipStream_t)hip_stream;
    if (laser) hipLaunchKernelGGL(rsd_gather_kernel<true>, grid, dim3(kRsdGatherBlock), 0, s, a);
    else hipLaunchKernelGGL(rsd_gather_kernel<false>, grid, dim3(kRsdGatherBlock), 0, s, a);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

}  // extern "C"
