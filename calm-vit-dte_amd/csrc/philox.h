// Philox4x32-10 (Salmon et al., SC'11), the counter-based generator of the dropout mask (dropout.hip) and of the
// RandomErasing noise fill (augment.hip): four 32-bit words as a function of a 128-bit counter and a 64-bit key, nothing
// else — no state, so a value depends on what it is the value OF and not on the thread that asks for it.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct PhiloxKey { uint32_t k0, k1, c2, c3; };      // key words and the upper counter words: the same for every element

// (seed, offset) -> key (lo32(seed), hi32(seed)) and upper counter words (lo32(offset), hi32(offset))
__host__ __device__ __forceinline__ PhiloxKey philox_key(uint64_t seed, uint64_t offset) {
    return {(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
}

// Philox4x32-10 of counter (lo32(group), hi32(group), k.c2, k.c3); each 32 x 32 -> 64-bit product is one v_mad_u64_u32
__device__ __forceinline__ u32x4 philox4x32_10(uint64_t group, const PhiloxKey& k) {
    uint32_t c0 = (uint32_t)group, c1 = (uint32_t)(group >> 32), c2 = k.c2, c3 = k.c3;
    uint32_t k0 = k.k0, k1 = k.k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return (u32x4){c0, c1, c2, c3};
}
