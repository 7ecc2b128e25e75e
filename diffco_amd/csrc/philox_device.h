// philox_device.h — Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) written
// out: a counter-based generator, so a draw is a function of (key, counter) alone and no state travels between launches.
// include/dcx.h ("batched RRT*: samples drawn on the device") pins the key, the counter and the use of every word.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcx {

struct Philox4 {
    uint32_t w[4];
};

// ten rounds; the key is bumped by the Weyl constants between them
__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += W0;
        k1 += W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// a word's upper 24 bits as a uniform of [0, 1), exact in fp32 ...
__host__ __device__ __forceinline__ float philox_u01(uint32_t word) { return (float)(word >> 8) * 0x1p-24f; }
// ... and of (0, 1], where a logarithm follows
__host__ __device__ __forceinline__ float philox_u01_open0(uint32_t word) { return (float)((word >> 8) + 1u) * 0x1p-24f; }

}  // namespace dcx
