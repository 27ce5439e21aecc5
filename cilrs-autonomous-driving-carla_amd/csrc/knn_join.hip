// Exact bulk k-NN of many queries on the matrix cores (cilrs_knn_join, include/cilrs_hip.h "Bulk
// nearest neighbours"): the fp32 MFMA only SCREENS, the shared distance of kc_dist.h re-scores the
// survivors and a float64 certificate says per query whether a screened-out row could belong to the
// result.  What is written for a certified query is bit for bit cilrs_knn's.
//
// Six launches on the caller's stream and nothing else:
//   join_norm_kernel    nx_i / ny_q (a wave a row, the lane layout and butterfly of kc_dist.h on
//                       x^2) and the workgroups' partial max of nx;  join_max_kernel folds those.
//   join_screen_kernel  a workgroup owns kJoinTQ = 128 queries and walks a slice of the pool in tiles
//                       of kJoinTN = 128 rows, both staged in LDS in D-chunks of kJoinKC = 16 columns
//                       (zeros past column D and past the last row, never a read there); the next
//                       chunk's global loads are in flight while the current one is multiplied.  A
//                       wave owns 32 queries and all 128 rows: four 32x32 accumulator blocks with the
//                       QUERIES on the column (lane) dimension, so a lane's 64 values per tile are 64
//                       pool rows of ONE query, met in ascending row order.  Each lane keeps a private
//                       threshold and a private sorted list of K_s pairs (s, i) in LDS: the epilogue
//                       is one fma and one compare per value, an insertion is rare after warm-up.
//                       A lane's rows ascend, so a tie in s never enters its list: (s, i) order for
//                       free.  The lanes' lists go to scratch as they are.
//   join_finish_kernel  a wave a query: merges the query's 2 x slices lists into K_s candidates in
//                       the order (s, i) (the lane-spread list of knn_list.h), re-scores them with
//                       kc_load_row / kc_dist (pool row first, query second, as knn_sweep_kernel),
//                       sorts by (d, i) without the NaN, evaluates the certificate in float64 and
//                       writes idx / dist / uncertified.
//   join_count_kernel   n_uncertified, an integer sum in one workgroup.
// No atomics, no fences, no hand-off inside a launch: the kernel boundary is the only ordering used.
// p(q, i) is one accumulator's chain from 0 over the D-chunks in order and a fixed column order in a
// chunk, whatever the tile, slice or call, and min / comparison / tie rule are exact: nothing
// depends on how rows and queries are spread.
#include "common.h"

#include <limits.h>

#pragma clang fp contract(off)      // the chains are written with fmaf(); nothing else fuses

#include "kc_dist.h"                // the distance, shared with kcenter.hip / knn.hip
#include "knn_list.h"               // the sorted pair list, shared with knn.hip

namespace cilrs {
namespace {

constexpr int kJoinMaxQ = 65536, kJoinMaxK = 16, kJoinExtra = 8;        // K_s = K + 8 <= 24
constexpr int kJoinTQ = 128, kJoinTN = 128, kJoinKC = 16;
constexpr int kJoinLd = kJoinKC + 4;        // LDS row pitch: 16-byte reads of 32 rows hit 64 banks once
constexpr int kJoinGroups = 512;            // workgroups aimed at: two on each of 256 CUs

int join_ks(const int K) { return K + kJoinExtra; }

// the pool's tiles are cut into slices of `tps` tiles so that few query tiles still fill the chip
struct JoinSplit { int nt, tps, S; };
JoinSplit join_split(const int N, const int Q) {
    const int nt = cdiv(N, kJoinTN), qt = cdiv(Q, kJoinTQ);
    const int want = min(nt, max(1, cdiv(kJoinGroups, qt)));
    const int tps = cdiv(nt, want);
    return JoinSplit{nt, tps, cdiv(nt, tps)};
}

constexpr size_t align16(const size_t n) { return (n + 15) & ~(size_t)15; }

// scratch: nx [N] | ny [Q] | partial max [kc_grid(N)] | max [1] | lists [Q][S][2][K_s] pairs
struct JoinScratch {
    size_t nx, ny, part, top, lists, bytes;
};
JoinScratch join_scratch(const int N, const int Q, const int K) {
    JoinScratch s;
    s.nx = 0;
    s.ny = s.nx + align16((size_t)N * 4);
    s.part = s.ny + align16((size_t)Q * 4);
    s.top = s.part + align16((size_t)kc_grid(N) * 4);
    s.lists = s.top + 16;
    s.bytes = s.lists + (size_t)Q * join_split(N, Q).S * 2 * join_ks(K) * sizeof(KnnPair);
    return s;
}

bool join_sizes_ok(const int N, const int Q, const int K) {
    return N >= 1 && N <= kKcMaxN && Q >= 1 && Q <= kJoinMaxQ && K >= 1 && K <= kJoinMaxK;
}

// max that keeps a NaN or an infinity as NaN: "every nx is finite" is `top == top` afterwards
__device__ __forceinline__ float join_max(const float a, const float b) {
    return (a != a || b != b) ? __builtin_nanf("") : (a > b ? a : b);
}
__device__ __forceinline__ float join_finite_or_nan(const float a) {
    return fabsf(a) < __builtin_inff() ? a : __builtin_nanf("");
}

// out[r] = sum of squares of row r: lane l runs a = fmaf(x_j, x_j, a) from 0 over its columns
// j = 256 q + 4 l + e < D (q ascending, then e), then the butterfly of wave_sum.  part (or NULL):
// the workgroup's join_max over its rows, -inf for a workgroup without rows.
__global__ __launch_bounds__(256) void join_norm_kernel(const float* __restrict__ A, const size_t ld,
                                                        const int rows, const int D, float* __restrict__ out,
                                                        float* __restrict__ part) {
    __shared__ float tops[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float top = -__builtin_inff();
    for (int r = blockIdx.x * 4 + wave; r < rows; r += gridDim.x * 4) {
        const float* row = A + (size_t)r * ld;
        float a = 0.f;
        for (int j = lane * 4; j < D; j += 256) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(row + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) a = fmaf(x[e], x[e], a);
        }
        a = wave_sum(a);
        if (lane == 0) out[r] = a;
        top = join_max(top, join_finite_or_nan(a));
    }
    if (part == nullptr) return;
    if (lane == 0) tops[wave] = top;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = join_max(join_max(tops[0], tops[1]), join_max(tops[2], tops[3]));
}

__global__ __launch_bounds__(256) void join_max_kernel(const float* __restrict__ part, const int n,
                                                       float* __restrict__ top) {
    __shared__ float tops[256];
    float t = -__builtin_inff();
    for (int e = threadIdx.x; e < n; e += 256) t = join_max(t, part[e]);
    tops[threadIdx.x] = t;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) tops[threadIdx.x] = join_max(tops[threadIdx.x], tops[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) top[0] = tops[0];
}

struct JoinScreenArgs {
    const float* X;
    size_t ld;
    int N, D;
    const float* Y;
    size_t ldq;
    int Q;
    const long long* skip;      // [Q] or NULL
    const float* nx;            // [N]
    int Ks, nt, tps;            // candidates per list; pool tiles; tiles per slice (gridDim.y slices)
    KnnPair* lists;             // [Q][gridDim.y][2][Ks]
};

constexpr int join_screen_lds(const int Ks) {
    return (kJoinTN + kJoinTQ) * kJoinLd * 4 + kJoinTN * 4 + 256 * Ks * (int)sizeof(KnnPair);
}

// grid (query tiles, slices)
__global__ __launch_bounds__(256) void join_screen_kernel(const JoinScreenArgs a) {
    extern __shared__ __align__(16) float join_smem[];
    float* xs = join_smem;                                  // [kJoinTN][kJoinLd]
    float* ys = xs + kJoinTN * kJoinLd;                     // [kJoinTQ][kJoinLd]
    float* nxs = ys + kJoinTQ * kJoinLd;                    // [kJoinTN], NaN past the last row
    KnnPair* mine = reinterpret_cast<KnnPair*>(nxs + kJoinTN) + threadIdx.x;   // entry e at mine[e * 256]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int N = a.N, D = a.D, Q = a.Q, Ks = a.Ks;
    const int q0 = blockIdx.x * kJoinTQ, q = q0 + wave * 32 + l31;
    const int t0 = blockIdx.y * a.tps, t1 = min(a.nt, t0 + a.tps);
    const int nchunk = (D + kJoinKC - 1) / kJoinKC;

    int sk = -1;
    if (a.skip != nullptr && q < Q) {
        const long long s = a.skip[q];
        sk = (s >= 0 && s < N) ? (int)s : -1;               // a value outside 0..N-1 excludes nothing
    }
    // the list's K_s-th s once it is full; NaN before, so that every value takes the slow path; a
    // lane without a query rejects everything but a NaN, which the slow path drops
    float thr = q < Q ? __builtin_nanf("") : -__builtin_inff();
    int cnt = 0;

    // staging: float4 f = tid + 256 r of a [128][16] chunk: row f / 4, columns 4 (f % 4) .. + 3
    f32x4 xr[2], yr[2];
    auto fetch = [&](const int tile, const int chunk) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int f = tid + 256 * r, row = f >> 2, col = chunk * kJoinKC + (f & 3) * 4;
            const int gi = tile * kJoinTN + row, gq = q0 + row;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            xr[r] = (gi < N && col < D) ? *reinterpret_cast<const f32x4*>(a.X + (size_t)gi * a.ld + col) : z;
            yr[r] = (gq < Q && col < D) ? *reinterpret_cast<const f32x4*>(a.Y + (size_t)gq * a.ldq + col) : z;
        }
    };

    // a value that is not >= the threshold: a row past N, the skipped row, a NaN, or an insertion
    auto slow = [&](const float s, const int row) {
        if (q >= Q || row >= N || row == sk || s != s) return;
        int e = cnt < Ks ? cnt : Ks - 1;                     // a full list drops its last entry
        while (e > 0 && s < mine[(e - 1) * 256].v) {         // rows ascend: a tie stays behind
            mine[e * 256] = mine[(e - 1) * 256];
            --e;
        }
        mine[e * 256] = KnnPair{s, row};
        if (cnt < Ks) ++cnt;
        if (cnt == Ks) thr = mine[(Ks - 1) * 256].v;
    };

    fetch(t0, 0);
    for (int tile = t0; tile < t1; ++tile) {
        f32x16 acc[4];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][e] = 0.f;
        for (int c = 0; c < nchunk; ++c) {
            __syncthreads();                                 // the previous chunk / epilogue was read
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int f = tid + 256 * r, row = f >> 2, col = (f & 3) * 4;
                *reinterpret_cast<f32x4*>(xs + row * kJoinLd + col) = xr[r];
                *reinterpret_cast<f32x4*>(ys + row * kJoinLd + col) = yr[r];
            }
            if (c == 0 && tid < kJoinTN) {
                const int gi = tile * kJoinTN + tid;
                nxs[tid] = gi < N ? a.nx[gi] : __builtin_nanf("");
            }
            __syncthreads();
            if (c + 1 < nchunk) fetch(tile, c + 1);          // in flight under the products
            else if (tile + 1 < t1) fetch(tile + 1, 0);
            // MFMA step (u, e) multiplies columns 8 u + e (lanes 0..31) and 8 u + 4 + e (lanes 32..63)
#pragma unroll
            for (int u = 0; u < kJoinKC / 8; ++u) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(ys + (wave * 32 + l31) * kJoinLd + u * 8 + lh * 4);
                f32x4 av[4];
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    av[m] = *reinterpret_cast<const f32x4*>(xs + (m * 32 + l31) * kJoinLd + u * 8 + lh * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m][e], b[e], acc[m], 0, 0, 0);
            }
        }
        // C/D map of the 32x32 MFMA: column = lane & 31 (the query), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 nxv = *reinterpret_cast<const f32x4*>(nxs + m * 32 + 8 * g + 4 * lh);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float s = fmaf(-2.f, acc[m][4 * g + e], nxv[e]);
                    if (!(s >= thr)) slow(s, tile * kJoinTN + m * 32 + 8 * g + 4 * lh + e);
                }
            }
    }

    if (q < Q) {
        KnnPair* out = a.lists + (((size_t)q * gridDim.y + blockIdx.y) * 2 + lh) * Ks;
        for (int e = 0; e < Ks; ++e) out[e] = e < cnt ? mine[e * 256] : KnnPair{__builtin_inff(), INT_MAX};
    }
}

struct JoinFinishArgs {
    const float* X;
    size_t ld;
    int N, D;
    const float* Y;
    size_t ldq;
    int Q;
    const long long* skip;
    int K, Ks, L;               // L: lists per query
    const KnnPair* lists;       // [Q][L][Ks]
    const float* ny;            // [Q]
    const float* top;           // [1]: max nx, NaN where an nx is not finite
    int64_t* idx;
    float* dist;                // [Q][K]
    int32_t* uncertified;       // [Q]
};

__device__ __forceinline__ bool join_finite(const double x) { return fabs(x) < (double)__builtin_inff(); }

// a wave a query
template <int NQ, int R>
__global__ __launch_bounds__(256) void join_finish_kernel(const JoinFinishArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wave;
    if (q >= a.Q) return;                                    // wave-uniform; no barrier below
    const int N = a.N, D = a.D, K = a.K, Ks = a.Ks;

    // the K_s candidates smallest in (s, i)
    float sv = __builtin_inff();
    int si = INT_MAX;
    const int n = a.L * Ks;
    const KnnPair* src = a.lists + (size_t)q * n;
    for (int base = 0; base < n; base += 64) {
        const int e = base + lane;
        const KnnPair p = e < n ? src[e] : KnnPair{__builtin_inff(), INT_MAX};
        knn_absorb(sv, si, p.v, p.i, Ks, lane);
    }
    const int m = __popcll(__ballot(lane < Ks && si != INT_MAX));
    const float sigma = m > 0 ? knn_lane(sv, m - 1) : 0.f;

    // their distances, lane c keeps candidate c's
    f32x4 y[NQ];
    kc_load_row<NQ>(a.Y + (size_t)q * a.ldq, D, lane, y);
    float dd = 0.f;
    for (int c0 = 0; c0 < m; c0 += R) {
        f32x4 x[R][NQ];
#pragma unroll
        for (int r = 0; r < R; ++r)                          // a batch's tail repeats the last candidate
            kc_load_row<NQ>(a.X + (size_t)knn_lane(si, min(c0 + r, m - 1)) * a.ld, D, lane, x[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float d = kc_dist<NQ>(x[r], y);
            if (lane == c0 + r) dd = d;
        }
    }

    // sorted by (d, i), the NaN left out
    float fv = __builtin_inff();
    int fi = INT_MAX;
    for (int c = 0; c < m; ++c) {
        const float d = knn_lane(dd, c);
        if (d == d) knn_insert(fv, fi, d, knn_lane(si, c), lane);
    }

    int skipped = 0;
    if (a.skip != nullptr) {
        const long long s = a.skip[q];
        skipped = (s >= 0 && s < N) ? 1 : 0;
    }
    bool cert = m == N - skipped;                            // (a): every row but the skipped one is a candidate
    if (!cert) {                                             // (b), float64; a NaN makes a comparison false
        const float dk = knn_lane(fv, K - 1);
        const int ik = knn_lane(fi, K - 1);
        const double top = a.top[0], ny = a.ny[q], sg = sigma, u = 1.0 / 16777216.0;
        const double b = (double)(4 * ((D + 255) / 256) + 9) * u;
        const double E = (double)(2 * D + 16) * u * (top + ny);
        cert = ik != INT_MAX && join_finite((double)dk) && join_finite(top) && join_finite(ny) &&
               join_finite(sg) && top + ny < 0x1p125 && (double)dk < (1.0 - b) * (sg + ny - E);
    }
    if (lane < K) {
        a.idx[(size_t)q * K + lane] = !cert ? -2 : fi == INT_MAX ? -1 : fi;
        a.dist[(size_t)q * K + lane] = cert ? fv : __builtin_nanf("");
    }
    if (lane == 0) a.uncertified[q] = cert ? 0 : 1;
}

__global__ __launch_bounds__(256) void join_count_kernel(const int32_t* __restrict__ flags, const int Q,
                                                         int32_t* __restrict__ count) {
    __shared__ int sums[256];
    int t = 0;
    for (int e = threadIdx.x; e < Q; e += 256) t += flags[e];
    sums[threadIdx.x] = t;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) sums[threadIdx.x] += sums[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) count[0] = sums[0];
}

struct JoinArgs {
    KnnArgs k;
    int32_t* uncertified;
    int32_t* n_uncertified;
};

int launch_join(const JoinArgs& j, hipStream_t s) {
    const KnnArgs& a = j.k;
    const JoinScratch o = join_scratch(a.N, a.Q, a.K);
    const JoinSplit sp = join_split(a.N, a.Q);
    const int Ks = join_ks(a.K);
    char* base = reinterpret_cast<char*>(a.scratch);
    float* nx = reinterpret_cast<float*>(base + o.nx);
    float* ny = reinterpret_cast<float*>(base + o.ny);
    float* part = reinterpret_cast<float*>(base + o.part);
    float* top = reinterpret_cast<float*>(base + o.top);
    KnnPair* lists = reinterpret_cast<KnnPair*>(base + o.lists);

    const int lds = join_screen_lds(Ks);
    if (set_max_dynamic_lds(reinterpret_cast<const void*>(join_screen_kernel), join_screen_lds(join_ks(kJoinMaxK))))
        return 1;

    const int gx = kc_grid(a.N);
    join_norm_kernel<<<gx, 256, 0, s>>>(a.X, (size_t)a.ld, a.N, a.D, nx, part);
    CILRS_LAUNCH_CHECK();
    join_max_kernel<<<1, 256, 0, s>>>(part, gx, top);
    CILRS_LAUNCH_CHECK();
    join_norm_kernel<<<kc_grid(a.Q), 256, 0, s>>>(a.Y, (size_t)a.ldq, a.Q, a.D, ny, nullptr);
    CILRS_LAUNCH_CHECK();

    const JoinScreenArgs w{a.X, (size_t)a.ld, a.N, a.D, a.Y, (size_t)a.ldq, a.Q, a.skip, nx, Ks, sp.nt, sp.tps, lists};
    join_screen_kernel<<<dim3(cdiv(a.Q, kJoinTQ), sp.S), 256, lds, s>>>(w);
    CILRS_LAUNCH_CHECK();

    const JoinFinishArgs f{a.X, (size_t)a.ld, a.N, a.D, a.Y, (size_t)a.ldq, a.Q, a.skip, a.K, Ks, sp.S * 2,
                           lists, ny, top, a.idx, a.dist, j.uncertified};
    const int g = cdiv(a.Q, 4);
    if (a.D <= 256) join_finish_kernel<1, 4><<<g, 256, 0, s>>>(f);
    else if (a.D <= 512) join_finish_kernel<2, 4><<<g, 256, 0, s>>>(f);
    else if (a.D <= 1024) join_finish_kernel<4, 2><<<g, 256, 0, s>>>(f);
    else join_finish_kernel<8, 1><<<g, 256, 0, s>>>(f);
    CILRS_LAUNCH_CHECK();
    join_count_kernel<<<1, 256, 0, s>>>(j.uncertified, a.Q, j.n_uncertified);
    CILRS_LAUNCH_CHECK();
    return 0;
}

int join_check(const JoinArgs& j, const size_t scratch_bytes) {
    const KnnArgs& a = j.k;
    const char* who = "knn_join";
    CILRS_CHECK(a.X && a.Y && a.idx && a.dist && j.uncertified && j.n_uncertified, "%s: NULL tensor", who);
    CILRS_CHECK(a.N >= 1 && a.N <= kKcMaxN, "%s: N = %d outside 1..%d", who, a.N, kKcMaxN);
    CILRS_CHECK(a.D >= 4 && a.D <= kKcMaxD && a.D % 4 == 0, "%s: D = %d outside 4..%d or not a multiple of 4",
                who, a.D, kKcMaxD);
    CILRS_CHECK(a.ld >= a.D && a.ld % 4 == 0, "%s: ld = %ld below D or not a multiple of 4", who, a.ld);
    CILRS_CHECK(a.ldq >= a.D && a.ldq % 4 == 0, "%s: ldq = %ld below D or not a multiple of 4", who, a.ldq);
    CILRS_CHECK(a.Q >= 1 && a.Q <= kJoinMaxQ, "%s: Q = %d outside 1..%d", who, a.Q, kJoinMaxQ);
    CILRS_CHECK(a.K >= 1 && a.K <= kJoinMaxK, "%s: K = %d outside 1..%d (cilrs_knn takes K up to 64)", who, a.K,
                kJoinMaxK);
    CILRS_CHECK(((uintptr_t)a.X & 15) == 0 && ((uintptr_t)a.Y & 15) == 0,
                "%s: X and Y must be 16-byte aligned", who);
    const size_t need = join_scratch(a.N, a.Q, a.K).bytes;
    CILRS_CHECK(a.scratch != nullptr && scratch_bytes >= need, "%s: scratch of %zu bytes, needs %zu", who,
                a.scratch ? scratch_bytes : (size_t)0, need);
    CILRS_CHECK(((uintptr_t)a.scratch & 15) == 0, "%s: scratch is not 16-byte aligned", who);
    return 0;
}

}  // namespace
}  // namespace cilrs

using namespace cilrs;

extern "C" {

int cilrs_knn_join_candidates(int K) { return (K >= 1 && K <= kJoinMaxK) ? join_ks(K) : 0; }

size_t cilrs_knn_join_scratch_bytes(int N, int Q, int D, int K) {
    if (!join_sizes_ok(N, Q, K) || D < 4 || D > kKcMaxD || D % 4) return 0;
    return join_scratch(N, Q, K).bytes;
}

int cilrs_knn_join(const float* X, long ld, int N, int D, const float* Y, long ldq, int Q, const int64_t* skip,
                   int K, int64_t* idx, float* dist, int32_t* uncertified, int32_t* n_uncertified, void* scratch,
                   size_t scratch_bytes, void* stream) {
    const JoinArgs j{KnnArgs{X, ld, N, D, Y, ldq, Q, reinterpret_cast<const long long*>(skip), K, idx, dist, scratch},
                     uncertified, n_uncertified};
    if (join_check(j, scratch_bytes)) return 1;
    return launch_join(j, (hipStream_t)stream);
}

}  // extern "C"
