// The distance of include/cilrs_hip.h "Greedy k-center", shared by kcenter.hip and knn.hip: a wave
// owns a row, lane l holds the columns 256 q + 4 l + e of the row (16-byte loads) and of the other
// point, runs the fmaf chain of the definition and the xor butterfly, so all 64 lanes end with the
// same distance.  Include after `#pragma clang fp contract(off)`: the chains are written with fmaf()
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

template <int NQ>
__device__ __forceinline__ float kc_dist(const f32x4 (&x)[NQ], const f32x4 (&c)[NQ]) {
    float a = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = x[q][e] - c[q][e];
            a = fmaf(t, t, a);
        }
    return wave_sum(a);          // the order of cilrs_feature_novelty
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

inline int kc_grid(const int N) { return min(kKcMaxGrid, cdiv(N, 4)); }

}  // namespace
}  // namespace cilrs
