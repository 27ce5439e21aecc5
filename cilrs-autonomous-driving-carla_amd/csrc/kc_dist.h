// The distance of include/cilrs_hip.h "Greedy k-center", shared by kcenter.hip, knn.hip and
// kmeans.hip: a wave owns a row, lane l holds the columns 256 q + 4 l + e of the row (16-byte loads)
// and of the other point, runs the fmaf chain of the definition and the xor butterfly, so all 64
// lanes end with the same distance.  Include after `#pragma clang fp contract(off)`: the chains are written with fmaf()
// and nothing else may fuse.
#pragma once
#include "common.h"

namespace cilrs {
namespace {

constexpr int kKcMaxGrid = 1024;        // workgroups of 4 waves: 16 waves on each of 256 CUs
constexpr int kKcCentres = 8;           // centres (queries) per LDS chunk
constexpr int kKcMaxN = 1 << 24, kKcMaxD = 2048, kKcMaxM = 65536;

// a lane's quads of one row: columns 256 q + 4 lane .. + 3 where they are below D, else zeros
// (a zero difference leaves the chain as it is)
template <int NQ>
__device__ __forceinline__ void kc_load_row(const float* __restrict__ row, const int D, const int lane,
                                            f32x4 (&x)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int j = q * 256 + lane * 4;
        x[q] = j < D ? *reinterpret_cast<const f32x4*>(row + j) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// a lane's chain of the definition, before the butterfly
template <int NQ>
__device__ __forceinline__ float kc_lane_chain(const f32x4 (&x)[NQ], const f32x4 (&c)[NQ]) {
    float a = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = x[q][e] - c[q][e];
            a = fmaf(t, t, a);
        }
    return a;
}

template <int NQ>
__device__ __forceinline__ float kc_dist(const f32x4 (&x)[NQ], const f32x4 (&c)[NQ]) {
    return wave_sum(kc_lane_chain<NQ>(x, c));          // the order of cilrs_feature_novelty
}

// The butterfly of V = 2^k lane sums at once (kmeans.hip): at the offsets 32, 16, .. a lane keeps
// half of its values and sends the other half, so a value's partial sums live on ever fewer lanes;
// every addition is the a_l + a_{l ^ o} that wave_sum performs for that value (fp32 addition
// commutes), so the bits are wave_sum's.  On return v[0] of lane l is the sum of value
// kc_butterfly_index<V>(l), the same in every lane with that index.
// Which half a lane keeps is a bit mask per offset (all ones where lane & o), made once per kernel
// and opaque to the optimiser: written as `lane & o ? a : b` the selection is moved in front of the
// chains and costs a compare and a select per element instead of two or three bit operations per
// value.  (Plain C on purpose: with the pick as inline v_bfi_b32 the compiler no longer pairs the
// chains of two rows into v_pk_add_f32 / v_pk_fma_f32, 402 instructions per 16 distances at D = 512
// instead of 293.)
struct KcButterflyMasks { unsigned m[6]; };          // for o = 32, 16, 8, 4, 2, 1
__device__ __forceinline__ KcButterflyMasks kc_butterfly_masks(const int lane) {
    KcButterflyMasks k;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        unsigned m = (lane & (32 >> s)) ? ~0u : 0u;
        asm volatile("" : "+v"(m));
        k.m[s] = m;
    }
    return k;
}
__device__ __forceinline__ float kc_pick(const float a, const float b, const unsigned m) {   // m ? b : a
    return __uint_as_float((__float_as_uint(a) & ~m) | (__float_as_uint(b) & m));
}
template <int V>
__device__ __forceinline__ void kc_butterfly(float (&v)[V], const KcButterflyMasks& k) {
    static_assert(V >= 1 && V <= 64 && (V & (V - 1)) == 0, "V is a power of two up to 64");
    int o = 32, s = 0;
#pragma unroll
    for (int n = V; n > 1; n >>= 1, o >>= 1, ++s) {
#pragma unroll
        for (int i = 0; i < n / 2; ++i) {
            const float keep = kc_pick(v[i], v[i + n / 2], k.m[s]), send = kc_pick(v[i + n / 2], v[i], k.m[s]);
            v[i] = keep + __shfl_xor(send, o);
        }
    }
#pragma unroll
    for (; o >= 1; o >>= 1) v[0] += __shfl_xor(v[0], o);
}
template <int V>
__device__ __forceinline__ int kc_butterfly_index(const int lane) {
    int idx = 0, o = 32;
#pragma unroll
    for (int n = V; n > 1; n >>= 1, o >>= 1) idx += (lane & o) ? n / 2 : 0;
    return idx;
}

// stage up to kKcCentres rows of C (columns below D, zeros above) in LDS as cs[m][NQ * 256]
template <int NQ>
__device__ __forceinline__ void kc_stage_rows(float* __restrict__ cs, const float* __restrict__ C,
                                              const size_t ldc, const int nm, const int D, const int tid) {
    for (int e = tid; e < nm * NQ * 64; e += 256) {
        const int m = e / (NQ * 64), j = (e - m * (NQ * 64)) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (j < D) v = *reinterpret_cast<const f32x4*>(C + (size_t)m * ldc + j);
        *reinterpret_cast<f32x4*>(cs + m * (NQ * 256) + j) = v;
    }
}

// the same for any number of rows and a workgroup of T threads (kmeans.hip: up to kKmLdsFloats)
template <int NQ, int T>
__device__ __forceinline__ void kc_stage_rows_wide(float* __restrict__ cs, const float* __restrict__ C,
                                                   const size_t ldc, const int nm, const int D, const int tid) {
    for (int e = tid; e < nm * NQ * 64; e += T) {
        const int m = e / (NQ * 64), j = (e - m * (NQ * 64)) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (j < D) v = *reinterpret_cast<const f32x4*>(C + (size_t)m * ldc + j);
        *reinterpret_cast<f32x4*>(cs + m * (NQ * 256) + j) = v;
    }
}

inline int kc_grid(const int N) { return min(kKcMaxGrid, cdiv(N, 4)); }

}  // namespace
}  // namespace cilrs
