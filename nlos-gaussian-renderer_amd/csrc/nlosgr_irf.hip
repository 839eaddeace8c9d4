// Temporal instrument response (gfx950): the convolution in time between a rendered transient and a
// measured one, its adjoint, and the volume loss fused with both: the MSE (include/nlosgr.h, ABI 12) or the
// Poisson deviance of photon counts (nlosgr_loss_irf).
//
//   apply:    y[p,t] = b + sum_j w[j] h[p, t + c - j]        adjoint:  g[p,s] = sum_j w[j] z[p, s - c + j]
//
// The adjoint is the apply with the taps reversed and the centre mirrored (c' = L-1-c), so one routine
// serves both.  One 256-thread workgroup per row (grid-stride over rows):
//   * the row is staged in LDS between zero halos of the padded tap count on either side;
//   * a lane forms R consecutive outputs (R = 4 up to 1024 bins, else 8; up to 4 such chunks per lane at
//     8192 bins) from a sliding window of R registers: per tap one LDS read and R fmas, the window's
//     register names rotating through a tap loop unrolled by R;
//   * the LDS image is transposed, element i at (i mod R) * W + i / R: a lane's window walks down the
//     rows of that image while the lanes of a wave, R elements apart, read consecutive dwords of one
//     row (no bank conflicts); W = columns rounded up to 64, plus 64 / R, so the transposed fill and
//     write-back spread over the banks too;
//   * the taps sit in a zero-padded LDS copy (loop-uniform index: broadcast reads);
//   * fused loss: y goes back to the LDS image, a coalesced pass reads the target, forms d, the loss
//     partials and z = gscale d in place, then the adjoint runs from the same image and the result
//     leaves through a coalesced pass.  hist and target are read once, grad_out is written once.
//     The Poisson kind differs in that pass alone (the deviance and z = gscale (rho - y') / rho per element):
//     same LDS, same two partials per row, same tree.
//   * the loss sums are per-row partials (block tree as mse_kernel) in the workspace; the finish kernel
//     adds them in double, 256 consecutive row blocks each in row order, then the blocks in order.
// No atomics: every output depends on its own row only, whatever the schedule.
#include "nlosgr_common.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

constexpr int kMaxGrid = 1 << 18;
constexpr int kFixedLds = 2 * NLOSGR_IRF_MAX_TAPS + 2 * kBlock;   // two tap copies + the reduction, floats

struct IrfArgs {
    const float* in;        // [rows, nr] x or hist
    const float* target;    // fused only
    const float* taps;      // DEVICE [L]
    float* out;             // y / g / grad_out (fused: may be NULL)
    float* partial;         // fused only: [rows][2]
    long long rows;
    int nr, L, c, adjoint;
    float b, gt, gscale;
    float eps;              // NLOSGR_LOSS_POISSON: rate_floor
};

__host__ __device__ constexpr int irf_log(int R) { return R == 8 ? 3 : 2; }

// columns of the transposed LDS image of S = 2 Lpad + nrpad + R elements
template <int R>
__host__ __device__ inline int irf_width(int S) {
    return (((S >> irf_log(R)) + 63) & ~63) + 64 / R;
}

template <int R>
__host__ __device__ inline int irf_span(int nr, int L) {
    const int Lpad = (L + R - 1) & ~(R - 1), nrpad = (nr + R - 1) & ~(R - 1);
    return 2 * Lpad + nrpad + R;
}

template <int R>
__device__ __forceinline__ int irf_phys(int i, int W) {
    return (i & (R - 1)) * W + (i >> irf_log(R));
}

// buf: transposed image, data element u at logical index Lpad + u.  Overwrites the data region with
// (t < nr ? add + sum_j tl[j] data[t + cc - j] : 0); tl holds Lpad taps (zeros past L).  Two barriers.
template <int R, int NC>
__device__ __forceinline__ void irf_conv(float* buf, const float* tl, int W, int Lpad, int cc, int nr, float add) {
    constexpr int LOG = irf_log(R);
    const int nchunks = (nr + R - 1) >> LOG;
    const int K = Lpad + cc;   // logical index of data[t + cc] relative to R * chunk
    float acc[NC][R];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const int chunk = threadIdx.x + q * kBlock;
#pragma unroll
        for (int r = 0; r < R; ++r) acc[q][r] = 0.f;
        if (chunk < nchunks) {
            // x[k mod R] = element R chunk + K + k; tap j uses k = r - j for output r
            float x[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int m = K + r;
                x[r] = buf[(m & (R - 1)) * W + (m >> LOG) + chunk];
            }
            for (int j0 = 0; j0 < Lpad; j0 += R) {
                float w[R];
#pragma unroll
                for (int jj = 0; jj < R; ++jj) w[jj] = tl[j0 + jj];
#pragma unroll
                for (int jj = 0; jj < R; ++jj) {
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[q][r] = fmaf(w[jj], x[(r - jj + R) % R], acc[q][r]);
                    const int m = K - j0 - jj - 1;   // >= 0: the left halo is Lpad wide
                    x[R - 1 - jj] = buf[(m & (R - 1)) * W + (m >> LOG) + chunk];
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const int chunk = threadIdx.x + q * kBlock;
        if (chunk < nchunks) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                buf[r * W + (Lpad >> LOG) + chunk] = (chunk * R + r < nr) ? acc[q][r] + add : 0.f;
        }
    }
    __syncthreads();
}

// LOSS (NLOSGR_LOSS_*) is read in the FUSED branch only
template <int R, int NC, bool FUSED, int LOSS>
__global__ __launch_bounds__(kBlock) void irf_kernel(IrfArgs a) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int Lpad = (a.L + R - 1) & ~(R - 1);
    const int S = irf_span<R>(a.nr, a.L);
    const int W = irf_width<R>(S);
    float* buf = lds;                                  // [R * W]
    float* tlf = buf + R * W;                          // taps as given   [NLOSGR_IRF_MAX_TAPS]
    float* tlr = tlf + NLOSGR_IRF_MAX_TAPS;            // taps reversed
    float* red = tlr + NLOSGR_IRF_MAX_TAPS;            // [2][kBlock]
    for (int j = tid; j < Lpad; j += kBlock) {
        tlf[j] = j < a.L ? a.taps[j] : 0.f;
        tlr[j] = j < a.L ? a.taps[a.L - 1 - j] : 0.f;
    }
    for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
        const float* in = a.in + row * a.nr;
        for (int i = tid; i < S; i += kBlock) {
            const int u = i - Lpad;
            buf[irf_phys<R>(i, W)] = (u >= 0 && u < a.nr) ? in[u] : 0.f;
        }
        __syncthreads();
        if (!FUSED) {
            if (a.adjoint)
                irf_conv<R, NC>(buf, tlr, W, Lpad, a.L - 1 - a.c, a.nr, 0.f);
            else
                irf_conv<R, NC>(buf, tlf, W, Lpad, a.c, a.nr, a.b);
        } else {
            irf_conv<R, NC>(buf, tlf, W, Lpad, a.c, a.nr, a.b);
            const float* target = a.target + row * a.nr;
            float se = 0.f, st = 0.f;
            if (LOSS == NLOSGR_LOSS_POISSON) {
                // one fp32 rounding per operation, in the order include/nlosgr.h gives (no contraction):
                // tests/loss_oracle.py bounds the gradient's error by counting them
#pragma clang fp contract(off)
                for (int i = tid; i < a.nr; i += kBlock) {
                    const int p = irf_phys<R>(Lpad + i, W);
                    const float lam = buf[p];
                    const float y = a.gt * target[i];
                    const float yp = fmaxf(y, 0.f) + a.eps;
                    const float rho = fmaxf(lam, 0.f) + a.eps;
                    const float r = rho - yp;
                    buf[p] = lam >= 0.f ? a.gscale * (r / rho) : 0.f;
                    // e > -1 in exact arithmetic; r rounds to -y' once rho < 2^-25 y', and log1pf(-1) = -inf
                    const float e = fmaxf(r / yp, -0x1.fffffep-1f);
                    const float dev = 2.f * yp * (e - log1pf(e));
                    se = se + dev;
                    st = st + fmaxf(y, 0.f);
                }
            } else {
                for (int i = tid; i < a.nr; i += kBlock) {
                    const int p = irf_phys<R>(Lpad + i, W);
                    const float t = target[i] * a.gt;
                    const float d = buf[p] - t;
                    se = fmaf(d, d, se);
                    st = fmaf(t, t, st);
                    buf[p] = a.gscale * d;
                }
            }
            red[tid] = se;
            red[kBlock + tid] = st;
            __syncthreads();
            for (int o = kBlock / 2; o > 0; o >>= 1) {
                if (tid < o) {
                    red[tid] += red[tid + o];
                    red[kBlock + tid] += red[kBlock + tid + o];
                }
                __syncthreads();
            }
            if (tid == 0) {
                a.partial[2 * row] = red[0];
                a.partial[2 * row + 1] = red[kBlock];
            }
            if (a.out) irf_conv<R, NC>(buf, tlr, W, Lpad, a.L - 1 - a.c, a.nr, 0.f);
        }
        if (a.out) {
            float* out = a.out + row * a.nr;
            for (int i = tid; i < a.nr; i += kBlock) out[i] = buf[irf_phys<R>(Lpad + i, W)];
        }
        __syncthreads();   // the image is refilled for the next row
    }
}

// per-row partials -> loss_out[4]; thread k adds rows [k per, (k+1) per) in order, thread 0 the 256 sums in order
__global__ __launch_bounds__(kBlock) void irf_finish_kernel(const float* __restrict__ partial, long long rows, double n,
                                                          float* __restrict__ out) {
    __shared__ double acc[2][kBlock];
    const long long per = (rows + kBlock - 1) / kBlock;
    const long long r0 = threadIdx.x * per, r1 = r0 + per < rows ? r0 + per : rows;
    double se = 0.0, st = 0.0;
    for (long long r = r0; r < r1; ++r) {
        se += partial[2 * r];
        st += partial[2 * r + 1];
    }
    acc[0][threadIdx.x] = se;
    acc[1][threadIdx.x] = st;
    __syncthreads();
    if (threadIdx.x != 0) return;
    se = st = 0.0;
    for (int k = 0; k < kBlock; ++k) {
        se += acc[0][k];
        st += acc[1][k];
    }
    const double loss = se / n;
    out[0] = (float)loss;
    out[1] = st > 0.0 ? (float)(loss / (st / n)) : 0.f;
    out[2] = (float)se;
    out[3] = (float)st;
}

template <int R, int NC, bool FUSED, int LOSS>
void irf_launch_cfg(const IrfArgs& a, hipStream_t s) {
    const int W = irf_width<R>(irf_span<R>(a.nr, a.L));
    const size_t lds = (size_t)(R * W + kFixedLds) * sizeof(float);   // <= 45.3 KB at nr 8192, 512 taps
    const int grid = (int)(a.rows < kMaxGrid ? a.rows : kMaxGrid);
    hipLaunchKernelGGL((irf_kernel<R, NC, FUSED, LOSS>), dim3(grid), dim3(kBlock), lds, s, a);
}

template <bool FUSED, int LOSS = NLOSGR_LOSS_MSE>
void irf_launch(const IrfArgs& a, hipStream_t s) {
    if (a.nr <= 4 * kBlock) irf_launch_cfg<4, 1, FUSED, LOSS>(a, s);
    else if (a.nr <= 8 * kBlock) irf_launch_cfg<8, 1, FUSED, LOSS>(a, s);
    else if (a.nr <= 16 * kBlock) irf_launch_cfg<8, 2, FUSED, LOSS>(a, s);
    else irf_launch_cfg<8, 4, FUSED, LOSS>(a, s);
}

int irf_validate(const nlosgr_irf* irf, long long rows, int32_t nr) {
    if (!irf) return set_err(NLOSGR_E_INVALID, "null irf");
    if (irf->ntaps < 1 || irf->ntaps > NLOSGR_IRF_MAX_TAPS)
        return set_err(NLOSGR_E_INVALID, "1 <= irf.ntaps <= NLOSGR_IRF_MAX_TAPS");
    if (irf->center < 0 || irf->center >= irf->ntaps) return set_err(NLOSGR_E_INVALID, "0 <= irf.center < irf.ntaps");
    if (!irf->taps) return set_err(NLOSGR_E_INVALID, "null irf.taps");
    if (rows < 0) return set_err(NLOSGR_E_INVALID, "rows must be >= 0");
    if (nr < 1) return set_err(NLOSGR_E_INVALID, "nr must be >= 1");
    if (nr > NLOSGR_IRF_MAX_NR) return set_err(NLOSGR_E_UNSUPPORTED, "nr > NLOSGR_IRF_MAX_NR");
    return NLOSGR_OK;
}

int loss_validate(const nlosgr_loss* loss) {
    if (!loss) return set_err(NLOSGR_E_INVALID, "null loss");
    if (loss->kind != NLOSGR_LOSS_MSE && loss->kind != NLOSGR_LOSS_POISSON)
        return set_err(NLOSGR_E_INVALID, "loss.kind must be NLOSGR_LOSS_MSE or NLOSGR_LOSS_POISSON");
    if (loss->kind == NLOSGR_LOSS_POISSON && !(isfinite(loss->rate_floor) && loss->rate_floor > 0.f))
        return set_err(NLOSGR_E_INVALID, "loss.rate_floor must be finite and > 0");
    return NLOSGR_OK;
}

}  // namespace

extern "C" {

int nlosgr_irf_apply(const float* x, long long rows, int32_t nr, const nlosgr_irf* irf, int32_t adjoint, float* y_out,
                     void* hip_stream) {
    if (int rc = irf_validate(irf, rows, nr)) return rc;
    if (rows == 0) return NLOSGR_OK;
    if (!x || !y_out) return set_err(NLOSGR_E_INVALID, "null x/y_out pointer");
    if (x == y_out) return set_err(NLOSGR_E_INVALID, "y_out must not alias x");
    IrfArgs a;
    memset(&a, 0, sizeof(a));
    a.in = x; a.taps = irf->taps; a.out = y_out; a.rows = rows; a.nr = nr; a.L = irf->ntaps; a.c = irf->center;
    a.adjoint = adjoint != 0; a.b = irf->background;
    irf_launch<false>(a, (hipStream_t)hip_stream);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

size_t nlosgr_loss_irf_workspace_bytes(long long rows) {
    return align_up((size_t)2 * sizeof(float) * (size_t)(rows > 0 ? rows : 1));
}

int nlosgr_loss_irf(const float* hist, const float* target, float gt_times, long long rows, int32_t nr,
                    const nlosgr_irf* irf, const nlosgr_loss* loss, float grad_scale, float* grad_out, void* workspace,
                    float* loss_out, void* hip_stream) {
    if (int rc = loss_validate(loss)) return rc;
    if (int rc = irf_validate(irf, rows, nr)) return rc;
    if (!loss_out || !workspace) return set_err(NLOSGR_E_INVALID, "null loss/workspace pointer");
    if (rows > 0 && (!hist || !target)) return set_err(NLOSGR_E_INVALID, "null hist/target pointer");
    hipStream_t s = (hipStream_t)hip_stream;
    const double n = (double)rows * (double)nr;
    if (rows > 0) {
        IrfArgs a;
        memset(&a, 0, sizeof(a));
        a.in = hist; a.target = target; a.taps = irf->taps; a.out = grad_out; a.partial = (float*)workspace;
        a.rows = rows; a.nr = nr; a.L = irf->ntaps; a.c = irf->center; a.b = irf->background; a.gt = gt_times;
        a.gscale = (float)((double)grad_scale * 2.0 / n);
        if (loss->kind == NLOSGR_LOSS_POISSON) {
            a.eps = loss->rate_floor;
            irf_launch<true, NLOSGR_LOSS_POISSON>(a, s);
        } else {
            irf_launch<true, NLOSGR_LOSS_MSE>(a, s);
        }
    }
    // {a / n, a / b, a, b} of the two sums, whatever the kind
    hipLaunchKernelGGL(irf_finish_kernel, dim3(1), dim3(kBlock), 0, s, (const float*)workspace, rows,
                       rows > 0 ? n : 1.0, loss_out);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

size_t nlosgr_mse_irf_workspace_bytes(long long rows) { return nlosgr_loss_irf_workspace_bytes(rows); }

int nlosgr_mse_irf(const float* hist, const float* target, float gt_times, long long rows, int32_t nr,
                   const nlosgr_irf* irf, float grad_scale, float* grad_out, void* workspace, float* loss_out,
                   void* hip_stream) {
    const nlosgr_loss mse = {NLOSGR_LOSS_MSE, 0.f};
    return nlosgr_loss_irf(hist, target, gt_times, rows, nr, irf, &mse, grad_scale, grad_out, workspace, loss_out,
                           hip_stream);
}

}  // extern "C"
