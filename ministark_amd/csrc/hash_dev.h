// Device pieces that every byte hash shares.
#pragma once
#include <hip/hip_runtime.h>

namespace mshash {

// Leading zero bits of a digest's byte string, byte 0's high bit first: of each word read big-endian.  BIG_ENDIAN_WORDS: d[] already holds
// the words that way (SHA-256's state); otherwise they are the little-endian words of the bytes and are swapped here.
template <bool BIG_ENDIAN_WORDS>
__device__ __forceinline__ unsigned leading_zero_bits(const uint32_t (&d)[8]) {
    unsigned lz = 0;
    bool done = false;
    #pragma unroll
    for (int q = 0; q < 8; q++) {
        if (!done) {
            const uint32_t w = BIG_ENDIAN_WORDS ? d[q] : __builtin_bswap32(d[q]);
            const unsigned z = w ? (unsigned)__clz(w) : 32u;
            lz += z;
            if (z != 32) done = true;
        }
    }
    return lz;
}

}  // namespace mshash
