// The SGLD noise step of 3DGS-MCMC ("3D Gaussian Splatting as Markov Chain Monte Carlo", the position update
// after each optimizer step) on the device (gfx950), with no host synchronisation and no generator state:
//
//   sgld_kernel : one thread per Gaussian.  Four Philox4x32-10 words keyed by (seed, iteration, index) ->
//                 four open-interval uniforms -> three Box-Muller normals xi -> delta = scale gate Sigma xi with
//                 Sigma the covariance the renderer gives this Gaussian (activate<PRESET>: Sigma = R'^T diag(s~^2) R',
//                 the inverse of preprocess_kernel's N) and gate = sigmoid(gate_k ((1 - sigma) - gate_x0)), the
//                 3DGS-MCMC switch that is ~1 for a nearly transparent Gaussian and ~0 otherwise -> mu += delta.
//
// Rows are independent: no atomics, no LDS, no workspace.  11 floats read and 3 (6 with noise_out) written per
// Gaussian: bound by launch latency at any model size the renderer handles (include/nlosgr.h states the contract).
#include "nlosgr_common.hpp"
#include "nlosgr_rng.hpp"

using namespace nlosgr;
using namespace nlosgr::detail;

namespace {

struct SgldArgs {
    unsigned long long seed, iteration, first_index;
    float scale, gate_k, gate_x0;
};

template <int PRESET>
__global__ __launch_bounds__(kBlock) void sgld_kernel(nlosgr_gaussians g, SgldArgs a, float* mu_out, float* noise_out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= g.ng) return;
    uint32_t x[4];
    rng::philox_words(a.seed, a.iteration, a.first_index + (unsigned long long)i, x);
    const float u0 = rng::uniform_open(x[0]), u1 = rng::uniform_open(x[1]);
    const float u2 = rng::uniform_open(x[2]), u3 = rng::uniform_open(x[3]);
    // Box-Muller with the accurate logf (ln u next to u = 1 - 2^-24 is what the fast one loses) and the angle
    // 2 pi u through cospif / sinpif of 2 u, which is exact in fp32: rounding 2 pi u itself would leave xi2 with an
    // error of 4e-7 r, not 4e-7 |xi2|, and its sine partner, which carries r when the cosine is small, is not drawn
    const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
    float s0, c0;
    sincospif(2.0f * u1, &s0, &c0);
    const float xi[3] = {r0 * c0, r0 * s0, r1 * cospif(2.0f * u3)};

    const float S[3] = {g.scaling[3 * i], g.scaling[3 * i + 1], g.scaling[3 * i + 2]};
    const float Q[4] = {g.rotation[4 * i], g.rotation[4 * i + 1], g.rotation[4 * i + 2], g.rotation[4 * i + 3]};
    GaussAct act;
    activate<PRESET>(S, Q, g.opacity[i], g.scaling_modifier, act);
    // op_sigmoid(1 - opacity); expf overflowing to inf gives gate = 0 exactly (no NaN: 1 / inf)
    const float ga = (1.0f - act.sigma) - a.gate_x0;
    const float gate = 1.0f / (1.0f + expf(-a.gate_k * ga));
    const float sg = a.scale * gate;
    // Sigma xi = R'^T (s~^2 o (R' xi)), Sigma never formed
    float w[3];
    for (int r = 0; r < 3; ++r) {
        const float v = act.Rp[3 * r] * xi[0] + act.Rp[3 * r + 1] * xi[1] + act.Rp[3 * r + 2] * xi[2];
        w[r] = (act.st[r] * act.st[r]) * v;
    }
    float sx[3];
    for (int c = 0; c < 3; ++c) sx[c] = act.Rp[c] * w[0] + act.Rp[3 + c] * w[1] + act.Rp[6 + c] * w[2];
    for (int c = 0; c < 3; ++c) {
        // delta is rounded before it is added: mu_out == mu + noise_out bitwise.  The pragma keeps the compiler
        // from contracting the two into one fma (the build's default; __fmul_rn is a plain product to it).
#pragma clang fp contract(off)
        const float d = sg * sx[c];
        const float m = g.mu[3 * i + c];
        mu_out[3 * i + c] = m + d;
        if (noise_out) noise_out[3 * i + c] = d;
    }
}

}  // namespace

extern "C" {

int nlosgr_sgld_noise(const nlosgr_gaussians* g, const nlosgr_sgld* o, float* mu_out, float* noise_out,
                      void* hip_stream) {
    if (!g || !o) return set_err(NLOSGR_E_INVALID, "null argument struct");
    if (g->ng < 0) return set_err(NLOSGR_E_INVALID, "ng must be >= 0");
    if (g->preset != NLOSGR_PRESET_TORCH && g->preset != NLOSGR_PRESET_CUDA)
        return set_err(NLOSGR_E_INVALID, "unknown preset");
    if (g->ng == 0) return NLOSGR_OK;
    if (!g->mu || !g->scaling || !g->rotation || !g->opacity) return set_err(NLOSGR_E_INVALID, "null Gaussian parameter pointer");
    if (!mu_out) return set_err(NLOSGR_E_INVALID, "null mu_out pointer");
    SgldArgs a;
    a.seed = (unsigned long long)o->seed;
    a.iteration = (unsigned long long)o->iteration;
    a.first_index = (unsigned long long)o->first_index;
    a.scale = o->scale;
    a.gate_k = o->gate_k;
    a.gate_x0 = o->gate_x0;
    const int nb = (g->ng + kBlock - 1) / kBlock;
    hipStream_t s = (hipStream_t)hip_stream;
    if (g->preset == NLOSGR_PRESET_TORCH)
        hipLaunchKernelGGL(sgld_kernel<NLOSGR_PRESET_TORCH>, dim3(nb), dim3(kBlock), 0, s, *g, a, mu_out, noise_out);
    else
        hipLaunchKernelGGL(sgld_kernel<NLOSGR_PRESET_CUDA>, dim3(nb), dim3(kBlock), 0, s, *g, a, mu_out, noise_out);
    HIPCHK(hipGetLastError());
    return NLOSGR_OK;
}

}  // extern "C"
