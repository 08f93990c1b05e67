// Philox4x32-10 (Salmon et al., SC'11), the library's one counter-based generator: key = (seed lo, seed hi), counter = (block, step lo,
// step hi, array).  The arrays: 0 = eps and 1 = expo of m3pc_draw_variates (select.hip), 2 = the segment draws, 3 / 4 = the round keys
// of the online / offline transition permutation of the replay buffer (replay.hip); 5 / 6 = the dropout keep masks of a matrix site /
// of the attention probabilities (mtm_grad.h, DROPOUT), where block = the group of four elements, step = the draw and the array word
// also carries the site: array | site << 8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace m3pc {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0;
    w[1] = c1;
    w[2] = c2;
    w[3] = c3;
}

}  // namespace m3pc
