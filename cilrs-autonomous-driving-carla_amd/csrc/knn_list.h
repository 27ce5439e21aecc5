// The sorted pair list of include/cilrs_hip.h "Nearest neighbours", shared by knn.hip and
// knn_join.hip: a wave holds one list, lane l the l-th best pair (d, i) in the order of the
// definition; an insertion is one shuffle-up and two compares.
#pragma once
#include "common.h"

#include <limits.h>

namespace cilrs {
namespace {

struct __attribute__((aligned(8))) KnnPair { float v; int i; };

// the order of the definition: (d, i) comes before (e, j).  No pair holds a NaN; an empty slot is
// (+inf, INT_MAX), which every row's pair comes before.
__device__ __forceinline__ bool knn_before(const float d, const int i, const float e, const int j) {
    return (d < e) | ((d == e) & (i < j));                   // no short circuit: straight-line code
}

// entry `l` of a list (l wave-uniform), as a scalar
__device__ __forceinline__ int knn_lane(const int x, const int l) { return __builtin_amdgcn_readlane(x, l); }
__device__ __forceinline__ float knn_lane(const float x, const int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l));
}

// insert the wave-uniform pair (d, r) into the sorted list that lane l holds entry l of
__device__ __forceinline__ void knn_insert(float& v, int& i, const float d, const int r, const int lane) {
    // entry lane - 1 (DPP wave_shr:1; lane 0 keeps its own and never reads it)
    const float uv = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, false));
    const int ui = __builtin_amdgcn_update_dpp(0, i, 0x138, 0xf, 0xf, false);
    const bool stays = knn_before(v, i, d, r);              // else it moves down or is replaced
    const bool up_stays = (lane == 0) | knn_before(uv, ui, d, r);
    v = stays ? v : up_stays ? d : uv;
    i = stays ? i : up_stays ? r : ui;
}

// take the pairs (cv, ci), one per lane, into the list: those that come before the K-th, one by one
__device__ __forceinline__ void knn_absorb(float& v, int& i, const float cv, const int ci, const int K,
                                           const int lane) {
    float kd = knn_lane(v, K - 1);
    int ki = knn_lane(i, K - 1);
    unsigned long long m = __ballot(knn_before(cv, ci, kd, ki));
    while (m) {
        const int src = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
        knn_insert(v, i, knn_lane(cv, src), knn_lane(ci, src), lane);
        kd = knn_lane(v, K - 1);
        ki = knn_lane(i, K - 1);
        m &= m - 1;
        m &= __ballot(knn_before(cv, ci, kd, ki));
    }
}

}  // namespace
}  // namespace cilrs
