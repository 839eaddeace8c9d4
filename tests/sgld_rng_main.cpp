// Stand-alone host program around csrc/nlosgr_rng.hpp (tests/test_sgld_cpu.py compiles and runs it, with the
// address and undefined-behaviour sanitizers): prints the generator's words for the three Random123 known-answer
// inputs and, for a few (seed, iteration, index) triples, the words and the uniforms the SGLD kernel draws.
//   kat <c0> <c1> <c2> <c3> <k0> <k1> : <x0> <x1> <x2> <x3>           (hex)
//   draw <seed> <iteration> <n> : <x0..x3 hex> : <u0..u3 %.9g>          (decimal inputs)
#include <inttypes.h>
#include <stdio.h>

#include "nlosgr_rng.hpp"

using namespace nlosgr::rng;

int main() {
    const uint32_t kat[3][6] = {
        {0u, 0u, 0u, 0u, 0u, 0u},
        {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
        {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u},
    };
    for (const auto& v : kat) {
        uint32_t out[4];
        philox4x32_10(v, v + 4, out);
        printf("kat %08x %08x %08x %08x %08x %08x : %08x %08x %08x %08x\n", v[0], v[1], v[2], v[3], v[4], v[5], out[0],
               out[1], out[2], out[3]);
    }
    const uint64_t draws[][3] = {
        {0u, 0u, 0u},
        {42u, 5u, 0u},
        {42u, 5u, 1u},
        {42u, 5u, 2u},
        {1234u, 7u, 65535u},
        {(1ull << 40) + 5u, (1ull << 33) + 1u, (1ull << 32) + 3u},
        {5u, 1u, 3u},
        {~0ull, ~0ull, ~0ull},
    };
    for (const auto& d : draws) {
        uint32_t x[4];
        philox_words(d[0], d[1], d[2], x);
        printf("draw %" PRIu64 " %" PRIu64 " %" PRIu64 " : %08x %08x %08x %08x : %.9g %.9g %.9g %.9g\n", d[0], d[1], d[2],
               x[0], x[1], x[2], x[3], (double)uniform_open(x[0]), (double)uniform_open(x[1]),
               (double)uniform_open(x[2]), (double)uniform_open(x[3]));
    }
    // the ends of the uniform's range: never 0, never 1
    printf("ends %.9g %.9g\n", (double)uniform_open(0u), (double)uniform_open(0xffffffffu));
    return 0;
}
