// Packed 64-bit selection keys, shared by the top-k kernels (rae_topk.hpp k_topk / k_topk_finish,
// rae_profile.hpp k_ctopk, rae_feature.hpp k_ftopk / k_ftopk_finish).
//
// A key is  orderable(value) << 32 | ~index, so unsigned 64-bit order is value descending, then
// index ascending -- a total order over distinct indices -- and 0 means "no entry".
//   topk_key    a float score: -0 is made +0, then the sign bit of a non-negative score is set and
//               a negative score is inverted.  The smallest real key is -inf's (0x007fffff << 32);
//               a NaN score is no candidate (the caller's test).
//   count_key   a positive 32-bit count as it stands; a count <= 0 is no entry.
// tk_offer keeps the best keys a wave has seen sorted across its lanes; key_unpack_store is the
// (index, score) epilogue of the float keys, padding (-1, -inf).
#pragma once
#include "rae_common.hpp"

namespace rae {

typedef unsigned long long rae_key64;

__device__ __forceinline__ rae_key64 topk_key(float g, unsigned e) {
    g = g == 0.f ? 0.f : g;                                   // -0 -> +0
    const unsigned b = __float_as_uint(g);
    const unsigned ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((rae_key64)ord << 32) | (rae_key64)(~e);
}
__device__ __forceinline__ float topk_score(rae_key64 key) {
    const unsigned ord = (unsigned)(key >> 32);
    return __uint_as_float((ord & 0x80000000u) ? (ord ^ 0x80000000u) : ~ord);
}
__device__ __forceinline__ rae_key64 count_key(int count, unsigned k) {
    return count > 0 ? ((rae_key64)(unsigned)count << 32) | (unsigned)~k : 0ull;
}

// the key held by lane i (i wave-uniform)
__device__ __forceinline__ rae_key64 topk_lane_key(rae_key64 v, int i) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, i);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), i);
    return ((rae_key64)hi << 32) | (rae_key64)lo;
}

// offer one key per lane (0 = none) to the wave's sorted list (lane j the j-th best, the top-th
// the admission threshold); every lane of the wave calls it (the loop and its branch are
// wave-uniform)
__device__ __forceinline__ void tk_offer(rae_key64 v, rae_key64& list, rae_key64& thr, int top,
                                         int lane) {
    unsigned long long cand = __ballot(v > thr);
    while (cand) {
        const int src = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(cand));
        cand &= cand - 1;
        const rae_key64 c = topk_lane_key(v, src);
        if (c > thr) {                                    // the threshold may have risen
            const int pos = __builtin_popcountll(__ballot(list > c));     // keys ahead of c
            const rae_key64 up = __shfl_up(list, 1, 64);
            list = lane < pos ? list : (lane == pos ? c : up);
            thr = topk_lane_key(list, top - 1);
        }
    }
}

// un-pack a float key to (idx_out[at], score_out[at]); no entry: (-1, -inf).  score_out may be NULL
__device__ __forceinline__ void key_unpack_store(rae_key64 key, int32_t* idx_out, float* score_out,
                                                 long long at) {
    const bool has = key != 0ull;
    idx_out[at] = has ? (int32_t)~(unsigned)key : -1;
    if (score_out) score_out[at] = has ? topk_score(key) : -INFINITY;
}

}  // namespace rae
