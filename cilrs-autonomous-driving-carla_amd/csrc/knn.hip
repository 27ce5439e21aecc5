// K nearest rows of a pool to each query (cilrs_knn, include/cilrs_hip.h "Nearest neighbours"): which
// recorded frames does this tick look like to the trunk.
//
// One chunk of at most eight queries is two or three launches on the caller's stream and nothing else:
//   knn_sweep_kernel  one streaming pass over X.  The queries are staged in LDS as kc_cover_kernel
//                     stages its centres; a wave owns 4 / 4 / 2 / 1 rows at a time (every 16-byte load
//                     of the batch issued before the first use) and runs the distance of kc_dist.h,
//                     so all 64 lanes end with the same d.  Each query's running list is spread over
//                     the wave's lanes, lane l holding the l-th best pair (d, i) in the order of the
//                     definition: a wave-uniform test against the K-th pair rejects most rows, an
//                     insertion is one shuffle-up and two compares.  At the end the four waves' lists
//                     are merged through LDS and the workgroup stores K pairs per query.
//   knn_fold_kernel   the workgroups' lists of a query, read as one stream of pairs (a lane a pair,
//                     eight loads in flight per lane; a ballot finds the pairs that still enter),
//                     merged the same way; stores idx / dist (either may be pinned host memory).
//                     Where the lists of a query are more than 2,048 pairs a first level of
//                     workgroups folds 2,048 / K lists each and the launch is repeated on theirs.
// Min, comparison and the tie rule are exact and the pairs form a total order, so the result does not
// depend on which wave saw which row; only the distance order fixes bits.  No atomics, no fences, no
// hand-off inside a launch: the kernel boundary is the only ordering used.
#include "common.h"

#include <limits.h>

#pragma clang fp contract(off)      // the chains are written with fmaf(); nothing else fuses

#include "kc_dist.h"                // the distance, shared with kcenter.hip
#include "knn_list.h"               // the sorted pair list, shared with knn_join.hip

namespace cilrs {
namespace {

constexpr int kKnnMaxQ = 65536, kKnnMaxK = 64;
constexpr int kKnnListFloats = kKcCentres * 4 * 64 * 2;     // eight queries x four waves x 64 pairs

struct KnnSweepArgs {
    const float* X;
    size_t ld;
    int N, D;
    const float* Y;             // the chunk's first query
    size_t ldq;
    const long long* skip;      // the chunk's first entry, or NULL
    int nm, K;                  // queries of the chunk (1..8)
    KnnPair* part;              // [nm][gridDim.x][K]
};

template <int NQ, int R>
__global__ __launch_bounds__(256) void knn_sweep_kernel(const KnnSweepArgs a) {
    constexpr int kFloats = kKcCentres * NQ * 256 > kKnnListFloats ? kKcCentres * NQ * 256 : kKnnListFloats;
    __shared__ __align__(16) float smem[kFloats];           // the queries, then the waves' lists
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, D = a.D, K = a.K, nm = a.nm;

    kc_stage_rows<NQ>(smem, a.Y, a.ldq, nm, D, tid);
    float lv[kKcCentres], kd[kKcCentres];
    int li[kKcCentres], ki[kKcCentres], sk[kKcCentres];
#pragma unroll
    for (int k = 0; k < kKcCentres; ++k) {
        lv[k] = kd[k] = __builtin_inff();
        li[k] = ki[k] = INT_MAX;
        long long s = -1;
        if (a.skip != nullptr && k < nm) s = a.skip[k];
        sk[k] = (s >= 0 && s < N) ? (int)s : -1;            // a value outside 0..N-1 excludes nothing
    }
    __syncthreads();

    const int step = gridDim.x * 4 * R;
    for (int r0 = (blockIdx.x * 4 + wave) * R; r0 < N; r0 += step) {
        f32x4 x[R][NQ];
#pragma unroll
        for (int r = 0; r < R; ++r)                          // a batch's tail repeats the last row
            kc_load_row<NQ>(a.X + (size_t)min(r0 + r, N - 1) * a.ld, D, lane, x[r]);
#pragma unroll
        for (int k = 0; k < kKcCentres; ++k) {
            if (k < nm) {
                f32x4 c[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    c[q] = *reinterpret_cast<const f32x4*>(smem + k * (NQ * 256) + q * 256 + lane * 4);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int row = r0 + r;
                    const float d = kc_dist<NQ>(x[r], c);
                    // wave-uniform: a candidate (not NaN, not skipped) that comes before the K-th
                    if (row < N && row != sk[k] && knn_before(d, row, kd[k], ki[k])) {
                        knn_insert(lv[k], li[k], d, row, lane);
                        kd[k] = knn_lane(lv[k], K - 1);
                        ki[k] = knn_lane(li[k], K - 1);
                    }
                }
            }
        }
    }

    // the four waves' lists through LDS; wave w merges queries w and w + 4
    __syncthreads();
    KnnPair* lists = reinterpret_cast<KnnPair*>(smem);
#pragma unroll
    for (int k = 0; k < kKcCentres; ++k)
        lists[(k * 4 + wave) * 64 + lane] = KnnPair{lv[k], li[k]};
    __syncthreads();
    for (int k = wave; k < nm; k += 4) {
        KnnPair p = lists[(k * 4) * 64 + lane];
        float v = p.v;
        int i = p.i;
        for (int w = 1; w < 4; ++w) {
            p = lists[(k * 4 + w) * 64 + lane];
            knn_absorb(v, i, p.v, p.i, K, lane);
        }
        if (lane < K) a.part[((size_t)k * gridDim.x + blockIdx.x) * K + lane] = KnnPair{v, i};
    }
}

constexpr int kKnnFoldPairs = 2048;     // pairs a fold workgroup loads before it merges: 8 per lane

struct KnnFoldArgs {
    const KnnPair* src;         // [nm][P][K]
    int P, K, G;                // lists per query; lists per workgroup
    KnnPair* out;               // [nm][gridDim.x][K] where gridDim.x > 1, else:
    int64_t* idx;               // the chunk's first row of [Q][K]
    float* dist;
};

// grid (cdiv(P, G), nm): workgroup (x, q) merges lists x G .. of query q
__global__ __launch_bounds__(256) void knn_fold_kernel(const KnnFoldArgs a) {
    __shared__ KnnPair lists[4 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, q = blockIdx.y, l0 = blockIdx.x * a.G;
    const int n = min(a.G, a.P - l0) * K;
    const KnnPair* src = a.src + ((size_t)q * a.P + l0) * K;
    float v = __builtin_inff();
    int i = INT_MAX;
    for (int base = 0; base < n; base += kKnnFoldPairs) {   // wave-uniform trip count
        KnnPair p[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {                        // every load before the first merge
            const int e = base + (t * 4 + wave) * 64 + lane;
            p[t] = e < n ? src[e] : KnnPair{__builtin_inff(), INT_MAX};
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) knn_absorb(v, i, p[t].v, p[t].i, K, lane);
    }
    lists[wave * 64 + lane] = KnnPair{v, i};
    __syncthreads();
    if (wave == 0) {
        for (int w = 1; w < 4; ++w) {
            const KnnPair p = lists[w * 64 + lane];
            knn_absorb(v, i, p.v, p.i, K, lane);
        }
        if (lane < K) {
            if (gridDim.x > 1) {
                a.out[((size_t)q * gridDim.x + blockIdx.x) * K + lane] = KnnPair{v, i};
            } else {                                         // fewer than K candidates: -1 / +inf
                a.idx[(size_t)q * K + lane] = i == INT_MAX ? -1 : i;
                a.dist[(size_t)q * K + lane] = v;
            }
        }
    }
}

// the folds after a sweep of g workgroups: one launch where their lists fit one workgroup's load,
// else a first level of cdiv(g, lists) workgroups per query
int knn_fold_lists(const int K) { return max(1, kKnnFoldPairs / K); }
int knn_fold_first(const int g, const int K) { return cdiv(g, knn_fold_lists(K)); }

bool knn_sizes_ok(const int N, const int Q, const int K) {
    return N >= 1 && N <= kKcMaxN && Q >= 1 && Q <= kKnnMaxQ && K >= 1 && K <= kKnnMaxK;
}

}  // namespace

size_t knn_scratch_bytes(int N, int Q, int K) {
    if (!knn_sizes_ok(N, Q, K)) return 0;
    const int g = kc_grid(N), first = knn_fold_first(g, K);
    return (size_t)(g + (first > 1 ? first : 0)) * min(Q, kKcCentres) * K * sizeof(KnnPair);
}

int launch_knn(const KnnArgs& a, hipStream_t s) {
    const int g = kc_grid(a.N);
    const int first = knn_fold_first(g, a.K);
    KnnPair* part = reinterpret_cast<KnnPair*>(a.scratch);          // [<= 8][g][K]
    KnnPair* part2 = part + (size_t)g * min(a.Q, kKcCentres) * a.K;  // [<= 8][first][K]
    for (int q0 = 0; q0 < a.Q; q0 += kKcCentres) {
        const int nm = min(kKcCentres, a.Q - q0);
        const KnnSweepArgs w{a.X, (size_t)a.ld, a.N, a.D, a.Y + (size_t)q0 * a.ldq, (size_t)a.ldq,
                             a.skip ? a.skip + q0 : nullptr, nm, a.K, part};
        if (a.D <= 256) knn_sweep_kernel<1, 4><<<g, 256, 0, s>>>(w);
        else if (a.D <= 512) knn_sweep_kernel<2, 4><<<g, 256, 0, s>>>(w);
        else if (a.D <= 1024) knn_sweep_kernel<4, 2><<<g, 256, 0, s>>>(w);
        else knn_sweep_kernel<8, 1><<<g, 256, 0, s>>>(w);
        CILRS_LAUNCH_CHECK();
        int64_t* idx = a.idx + (size_t)q0 * a.K;
        float* dist = a.dist + (size_t)q0 * a.K;
        if (first > 1) {
            knn_fold_kernel<<<dim3(first, nm), 256, 0, s>>>(
                KnnFoldArgs{part, g, a.K, knn_fold_lists(a.K), part2, nullptr, nullptr});
            CILRS_LAUNCH_CHECK();
            knn_fold_kernel<<<dim3(1, nm), 256, 0, s>>>(KnnFoldArgs{part2, first, a.K, first, nullptr, idx, dist});
        } else {
            knn_fold_kernel<<<dim3(1, nm), 256, 0, s>>>(KnnFoldArgs{part, g, a.K, g, nullptr, idx, dist});
        }
        CILRS_LAUNCH_CHECK();
    }
    return 0;
}

int knn_check(const char* who, const KnnArgs& a, const size_t scratch_bytes) {
    CILRS_CHECK(a.X && a.Y && a.idx && a.dist, "%s: NULL tensor", who);
    CILRS_CHECK(a.N >= 1 && a.N <= kKcMaxN, "%s: N = %d outside 1..%d", who, a.N, kKcMaxN);
    CILRS_CHECK(a.D >= 4 && a.D <= kKcMaxD && a.D % 4 == 0, "%s: D = %d outside 4..%d or not a multiple of 4",
                who, a.D, kKcMaxD);
    CILRS_CHECK(a.ld >= a.D && a.ld % 4 == 0, "%s: ld = %ld below D or not a multiple of 4", who, a.ld);
    CILRS_CHECK(a.ldq >= a.D && a.ldq % 4 == 0, "%s: ldq = %ld below D or not a multiple of 4", who, a.ldq);
    CILRS_CHECK(a.Q >= 1 && a.Q <= kKnnMaxQ, "%s: Q = %d outside 1..%d", who, a.Q, kKnnMaxQ);
    CILRS_CHECK(a.K >= 1 && a.K <= kKnnMaxK, "%s: K = %d outside 1..%d", who, a.K, kKnnMaxK);
    CILRS_CHECK(((uintptr_t)a.X & 15) == 0 && ((uintptr_t)a.Y & 15) == 0,
                "%s: X and Y must be 16-byte aligned", who);
    CILRS_CHECK(a.scratch != nullptr && scratch_bytes >= knn_scratch_bytes(a.N, a.Q, a.K),
                "%s: scratch of %zu bytes, needs %zu", who, a.scratch ? scratch_bytes : (size_t)0,
                knn_scratch_bytes(a.N, a.Q, a.K));
    CILRS_CHECK(((uintptr_t)a.scratch & 15) == 0, "%s: scratch is not 16-byte aligned", who);
    return 0;
}

}  // namespace cilrs

using namespace cilrs;

extern "C" {

size_t cilrs_knn_scratch_bytes(int N, int Q, int K) { return knn_scratch_bytes(N, Q, K); }

int cilrs_knn(const float* X, long ld, int N, int D, const float* Y, long ldq, int Q, const int64_t* skip,
              int K, int64_t* idx, float* dist, void* scratch, size_t scratch_bytes, void* stream) {
    const KnnArgs a{X, ld, N, D, Y, ldq, Q, reinterpret_cast<const long long*>(skip), K, idx, dist, scratch};
    if (knn_check("knn", a, scratch_bytes)) return 1;
    return launch_knn(a, (hipStream_t)stream);
}

}  // extern "C"
