// Counter-based random numbers for the device and the host: Philox4x32-10 (Salmon, Moraes, Dror, Shaw,
// "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants) and the open-interval uniform
// the SGLD noise step (nlosgr_sgld.hip) draws from it.  No state: the four output words are a function of the
// 128-bit counter and the 64-bit key alone, so every rank of a wall shard, every launch shape and a stand-alone
// host program get the same words.  Plain C++ (integer arithmetic only up to the uniform), no HIP header needed:
// a host compiler can include this file as it is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NLOSGR_HD __host__ __device__
#else
#define NLOSGR_HD
#endif

namespace nlosgr {
namespace rng {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;   // round multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;   // key increments (Weyl sequence)

// out[0..3] = Philox4x32-10(counter c[0..3], key k[0..1])
NLOSGR_HD inline void philox4x32_10(const uint32_t c[4], const uint32_t k[2], uint32_t out[4]) {
    uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// The words of element n at iteration `it` under `seed`: counter (lo32 n, hi32 n, lo32 it, hi32 it),
// key (lo32 seed, hi32 seed).
NLOSGR_HD inline void philox_words(uint64_t seed, uint64_t it, uint64_t n, uint32_t out[4]) {
    const uint32_t c[4] = {(uint32_t)n, (uint32_t)(n >> 32), (uint32_t)it, (uint32_t)(it >> 32)};
    const uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    philox4x32_10(c, k, out);
}

// u = ((x >> 9) + 0.5) 2^-23: 24 significant bits, so exact in fp32; in [2^-24, 1 - 2^-24], never 0 or 1.
NLOSGR_HD inline float uniform_open(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

}  // namespace rng
}  // namespace nlosgr
