// Greedy k-center (farthest-point) frame selection in feature space (cilrs_kcenter_cover /
// cilrs_kcenter_greedy, include/cilrs_hip.h "Greedy k-center"): which K rows of a pool to label.
//
// One pick is one streaming pass over the pool.  A wave owns a row at a time: lane l holds the
// columns 256 q + 4 l + e of the row (16-byte loads, every load of a batch of rows issued before the
// first use) and of the centre, runs the fmaf chain of the definition and the xor butterfly, so all
// 64 lanes end with the same distance.  The running (value, index) maximum of the rows a wave has
// seen is wave-uniform; a workgroup folds its four waves and stores ONE pair.
//
// cilrs_kcenter_greedy is K + 1 launches on the caller's stream and nothing else:
//   kc_argmax_kernel   the per-workgroup maxima of the caller's mind (no distance).
//   kc_pick_kernel     t = 0..K-1: every workgroup folds the previous launch's pairs (at most 1,024,
//                      double-buffered in the scratch) into the pick i_t, workgroup 0 stores sel[t]
//                      and radius[t]; every wave loads its lanes' share of row X[i_t] straight into
//                      registers (the same 2 KB for every wave of the chip: served by the L2), sweeps
//                      its rows, lowers mind where the new distance is smaller, and the workgroup
//                      stores its pair for the next launch.
// Max, min and the tie rule are exact and the pairs form a total order, so the result does not
// depend on which wave saw which row; only the distance order fixes bits.  No atomics, no fences, no
// hand-off inside a launch: the kernel boundary is the only ordering used.
//
// cilrs_kcenter_cover: one launch.  Eight centres at a time are staged in LDS (64 KB at D = 2048),
// so X is read once per eight centres; a row stays with the same wave over the chunks.
#include "common.h"

#include <limits.h>

#pragma clang fp contract(off)      // the chains are written with fmaf(); nothing else fuses

#include "kc_dist.h"                // the distance, shared with knn.hip

namespace cilrs {
namespace {

struct __attribute__((aligned(8))) KcPair { float v; int i; };

// the tie rule of the definition: a wins over b
__device__ __forceinline__ bool kc_wins(const KcPair a, const KcPair b) {
    return a.v > b.v || (a.v == b.v && a.i < b.i);
}
__device__ __forceinline__ KcPair kc_none() { return KcPair{-__builtin_inff(), INT_MAX}; }

// the largest pair of a workgroup of 256 threads; valid in every thread.  No pair holds a NaN.
__device__ __forceinline__ KcPair kc_block_max(KcPair b, KcPair* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const KcPair o{__shfl_xor(b.v, off), __shfl_xor(b.i, off)};
        if (kc_wins(o, b)) b = o;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = b;
    __syncthreads();
    b = red[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (kc_wins(red[w], b)) b = red[w];
    return b;
}

// Pair 0 of a launch starts from (mind[0], 0) as the definition does, so a NaN in mind[0] stays the
// answer; every other entry competes from (-inf, INT_MAX), which any entry beats and no NaN does.
__global__ __launch_bounds__(256) void kc_argmax_kernel(const float* __restrict__ mind, const int N,
                                                        KcPair* __restrict__ out) {
    __shared__ KcPair red[4];
    KcPair b = kc_none();
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
        const KcPair c{mind[i], i};
        if (kc_wins(c, b)) b = c;
    }
    b = kc_block_max(b, red);
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) {
            const KcPair s{mind[0], 0};
            b = kc_wins(b, s) ? b : s;
        }
        out[blockIdx.x] = b;
    }
}

struct KcPickArgs {
    const float* X;
    size_t ld;
    int N, D;
    float* mind;
    const KcPair* prev;     // the pairs of the previous launch, one per workgroup of this grid
    KcPair* next;
    int64_t* sel;           // &sel[t], &radius[t] of the pick this launch closes
    float* radius;
};

template <int NQ, int R>
__global__ __launch_bounds__(256) void kc_pick_kernel(const KcPickArgs a) {
    __shared__ KcPair red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, D = a.D, P = gridDim.x;

    // the pick: pairs 1.. in any order, then against pair 0 (which may hold a NaN and then stays)
    KcPair b = kc_none();
    for (int p = tid; p < P; p += 256)
        if (p > 0) {
            const KcPair c = a.prev[p];
            if (kc_wins(c, b)) b = c;
        }
    b = kc_block_max(b, red);
    KcPair pick = a.prev[0];
    if (kc_wins(b, pick)) pick = b;
    const int ic = min(max(__builtin_amdgcn_readfirstlane(pick.i), 0), N - 1);
    if (blockIdx.x == 0 && tid == 0) {
        a.sel[0] = ic;
        a.radius[0] = pick.v;
    }

    f32x4 c[NQ];
    kc_load_row<NQ>(a.X + (size_t)ic * a.ld, D, lane, c);

    KcPair wb = kc_none();
    float m0 = 0.f;
    const int step = P * 4 * R;
    for (int r0 = (blockIdx.x * 4 + wave) * R; r0 < N; r0 += step) {
        f32x4 x[R][NQ];
        float mv[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = min(r0 + r, N - 1);          // a batch's tail repeats the last row
            kc_load_row<NQ>(a.X + (size_t)row * a.ld, D, lane, x[r]);
            mv[r] = a.mind[row];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = r0 + r;
            const float d = kc_dist<NQ>(x[r], c);
            if (row < N) {
                float m = mv[r];
                if (d < m) {
                    m = d;
                    if (lane == 0) a.mind[row] = d;
                }
                const KcPair e{m, row};
                if (kc_wins(e, wb)) wb = e;
                if (row == 0) m0 = m;
            }
        }
    }
    b = kc_block_max(wb, red);
    if (tid == 0) {
        if (blockIdx.x == 0) {
            const KcPair s{m0, 0};          // row 0 is wave 0's of workgroup 0: thread 0 holds it
            b = kc_wins(b, s) ? b : s;
        }
        a.next[blockIdx.x] = b;
    }
}

struct KcCoverArgs {
    const float* X;
    size_t ld;
    int N, D;
    const float* C;
    size_t ldc;
    int M;
    float* mind;
};

template <int NQ, int R>
__global__ __launch_bounds__(256) void kc_cover_kernel(const KcCoverArgs a) {
    __shared__ __align__(16) float cs[kKcCentres][NQ * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, D = a.D;
    const int step = gridDim.x * 4 * R;
    for (int m0 = 0; m0 < a.M; m0 += kKcCentres) {
        const int nm = min(kKcCentres, a.M - m0);
        __syncthreads();
        kc_stage_rows<NQ>(&cs[0][0], a.C + (size_t)m0 * a.ldc, a.ldc, nm, D, tid);
        __syncthreads();
        for (int r0 = (blockIdx.x * 4 + wave) * R; r0 < N; r0 += step) {
            f32x4 x[R][NQ];
            float mv[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int row = min(r0 + r, N - 1);
                kc_load_row<NQ>(a.X + (size_t)row * a.ld, D, lane, x[r]);
                mv[r] = a.mind[row];
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float m = mv[r];
                bool lower = false;
                for (int k = 0; k < nm; ++k) {
                    f32x4 c[NQ];
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
                        c[q] = *reinterpret_cast<const f32x4*>(&cs[k][q * 256 + lane * 4]);
                    const float d = kc_dist<NQ>(x[r], c);
                    if (d < m) {
                        m = d;
                        lower = true;
                    }
                }
                if (lower && lane == 0 && r0 + r < N) a.mind[r0 + r] = m;
            }
        }
    }
}

size_t kc_pairs(const int N) { return ((size_t)kc_grid(N) + 1) & ~(size_t)1; }   // per buffer, 16 bytes apart

int kc_check_rows(const char* who, const float* X, long ld, int N, int D, const float* mind) {
    CILRS_CHECK(X && mind, "%s: NULL tensor", who);
    CILRS_CHECK(N >= 1 && N <= kKcMaxN, "%s: N = %d outside 1..%d", who, N, kKcMaxN);
    CILRS_CHECK(D >= 4 && D <= kKcMaxD && D % 4 == 0, "%s: D = %d outside 4..%d or not a multiple of 4",
                who, D, kKcMaxD);
    CILRS_CHECK(ld >= D && ld % 4 == 0, "%s: ld = %ld below D or not a multiple of 4", who, ld);
    CILRS_CHECK(((uintptr_t)X & 15) == 0, "%s: X is not 16-byte aligned", who);
    return 0;
}

}  // namespace
}  // namespace cilrs

using namespace cilrs;

extern "C" {

size_t cilrs_kcenter_scratch_bytes(int N) {
    if (N < 1 || N > kKcMaxN) return 0;
    return 2 * kc_pairs(N) * sizeof(KcPair);
}

int cilrs_kcenter_cover(const float* X, long ld, int N, int D, const float* C, long ldc, int M,
                        float* mind, void* stream) {
    if (kc_check_rows("kcenter_cover", X, ld, N, D, mind)) return 1;
    CILRS_CHECK(M >= 0 && M <= kKcMaxM, "kcenter_cover: M = %d outside 0..%d", M, kKcMaxM);
    if (M == 0) return 0;
    CILRS_CHECK(C != nullptr, "kcenter_cover: NULL tensor");
    CILRS_CHECK(ldc >= D && ldc % 4 == 0, "kcenter_cover: ldc = %ld below D or not a multiple of 4", ldc);
    CILRS_CHECK(((uintptr_t)C & 15) == 0, "kcenter_cover: C is not 16-byte aligned");
    const KcCoverArgs a{X, (size_t)ld, N, D, C, (size_t)ldc, M, mind};
    hipStream_t s = (hipStream_t)stream;
    const int g = kc_grid(N);
    if (D <= 256) kc_cover_kernel<1, 4><<<g, 256, 0, s>>>(a);
    else if (D <= 512) kc_cover_kernel<2, 4><<<g, 256, 0, s>>>(a);
    else if (D <= 1024) kc_cover_kernel<4, 2><<<g, 256, 0, s>>>(a);
    else kc_cover_kernel<8, 1><<<g, 256, 0, s>>>(a);
    CILRS_LAUNCH_CHECK();
    return 0;
}

int cilrs_kcenter_greedy(const float* X, long ld, int N, int D, float* mind, int K, int64_t* sel,
                         float* radius, void* scratch, size_t scratch_bytes, void* stream) {
    if (kc_check_rows("kcenter_greedy", X, ld, N, D, mind)) return 1;
    CILRS_CHECK(sel && radius, "kcenter_greedy: NULL tensor");
    CILRS_CHECK(K >= 1 && K <= N, "kcenter_greedy: K = %d outside 1..N = %d", K, N);
    CILRS_CHECK(scratch != nullptr && scratch_bytes >= cilrs_kcenter_scratch_bytes(N),
                "kcenter_greedy: scratch of %zu bytes, needs %zu", scratch ? scratch_bytes : (size_t)0,
                cilrs_kcenter_scratch_bytes(N));
    CILRS_CHECK(((uintptr_t)scratch & 15) == 0, "kcenter_greedy: scratch is not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int g = kc_grid(N);
    KcPair* buf[2] = {(KcPair*)scratch, (KcPair*)scratch + kc_pairs(N)};
    kc_argmax_kernel<<<g, 256, 0, s>>>(mind, N, buf[0]);
    CILRS_LAUNCH_CHECK();
    for (int t = 0; t < K; ++t) {
        const KcPickArgs a{X, (size_t)ld, N, D, mind, buf[t & 1], buf[(t + 1) & 1], sel + t, radius + t};
        if (D <= 256) kc_pick_kernel<1, 4><<<g, 256, 0, s>>>(a);
        else if (D <= 512) kc_pick_kernel<2, 4><<<g, 256, 0, s>>>(a);
        else if (D <= 1024) kc_pick_kernel<4, 2><<<g, 256, 0, s>>>(a);
        else kc_pick_kernel<8, 1><<<g, 256, 0, s>>>(a);
        CILRS_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
