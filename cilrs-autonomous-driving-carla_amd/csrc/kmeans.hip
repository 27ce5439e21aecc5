// Deterministic k-means (Lloyd) over a pool of feature rows (cilrs_kmeans_assign / _update / _lloyd,
// include/cilrs_hip.h "K-means"): what a recorded drive consists of, and how much of each kind.
//
// One Lloyd iteration is seven launches on the caller's stream and nothing else:
//   km_assign_kernel   the hot path.  One workgroup of 16 waves (8 above D = 512) per CU stages up to
//                      128 KiB of centres in LDS (128 / 64 / 32 / 16 centres at D <= 256 / 512 / 1,024 /
//                      2,048), so X is read once per such chunk.  A wave owns 4 / 4 / 2 / 1 rows at a time in the lane layout
//                      of kc_load_row; one ds_read_b128 of a centre quad serves all of them.  The lane
//                      chains of 16 (row, centre) pairs go through ONE butterfly (kc_butterfly: 17
//                      shuffles instead of 96, the additions of wave_sum, the same bits), after which
//                      lane l holds the distance of pair kc_butterfly_index(l) and keeps the running
//                      (d, m) best of its row over its share of the centres; the shares are merged in
//                      the total order of the definition at the end of a chunk.  Min and compare are
//                      exact, so chunking, waves and grid do not show in the result.  With more than
//                      one chunk the running best waits in dist / the scratch between chunks (a row stays
//                      with its wave), and `changed` is counted on the last one, per workgroup.
//   km_hist_kernel     rows in fixed blocks of RB = 256 ceil(N / 2^19): the block's label histogram
//                      (integer LDS atomics) as hist[m][b], and the block's float64 sum of dist in a
//                      fixed order.
//   km_scan_rows_kernel  a workgroup per cluster: the exclusive scan of its block counts, and counts[m].
//   km_scan_kernel     one workgroup: where each cluster starts in the rows sorted by label (with the
//                      launch before: the place of every (cluster, block) run), the work units of the
//                      sums, and the fixed-order totals inertia / changed.
//   km_scatter_kernel  a wave per block writes its rows' indices to their places in row order (a
//                      stable counting sort: ranks from ballots, no atomics).
//   km_segsum_kernel   one workgroup per (cluster, run of RB sorted rows): the gathered rows summed in
//                      float64 as a sequential chain per column, X read once, 16 bytes per lane and
//                      eight rows in flight.
//   km_centre_kernel   per cluster: the runs' sums added in run order, divided in float64, rounded.
// No floating-point atomics, no fences, no hand-off inside a launch: the kernel boundary is the only
// ordering used.  Every float64 order is a function of (N, the labels) alone.
#include "common.h"

#include <limits.h>

#pragma clang fp contract(off)      // the chains are written with fmaf(); nothing else fuses

#include "kc_dist.h"                // the distance, shared with kcenter.hip and knn.hip

namespace cilrs {
namespace {

constexpr int kKmWaves = 16, kKmWavesWide = 8;  // the assign workgroup: 16 waves, 8 above D = 512 (registers)
constexpr int kKmLdsFloats = 32768;         // 128 KiB of centres per chunk
constexpr int kKmVals = 16;                 // (row, centre) pairs per butterfly
constexpr int kKmMaxK = 1024, kKmMaxIters = 10000, kKmMaxGrid = 1024;
constexpr int kKmScanThreads = 1024;

// rows per histogram block, scatter wave and run of the sums: at most 2,048 blocks for any N
inline int km_block_rows(const int N) { return 256 * cdiv(N, 1 << 19); }
inline int km_blocks(const int N) { return cdiv(N, km_block_rows(N)); }

// ---- assign -------------------------------------------------------------------------------------------
struct KmAssignArgs {
    const float* X;
    size_t ld;
    int N, D;
    const float* C;
    size_t ldc;
    int K;
    int* label;
    float* dist;
    int* tmp;               // [N]: the running label between two chunks of centres
    long long* chg;         // [gridDim.x]: rows of this workgroup whose label changed
};

// (od, om) comes before (bd, bm) in the order of the definition; -1 is "no candidate", no d is NaN
__device__ __forceinline__ bool km_before(const float od, const int om, const float bd, const int bm) {
    return (om >= 0) & ((bm < 0) | (od < bd) | ((od == bd) & (om < bm)));
}

template <int NQ, int R, int W>
__global__ __launch_bounds__(W * 64) void km_assign_kernel(const KmAssignArgs a) {
    constexpr int CH = kKmLdsFloats / (NQ * 256), KK = kKmVals / R;
    static_assert(CH % KK == 0, "a chunk is whole groups of centres");
    __shared__ __align__(16) float cs[kKmLdsFloats];
    __shared__ int red[W];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, D = a.D, K = a.K;
    const int vi = kc_butterfly_index<kKmVals>(lane), myr = vi % R, mykk = vi / R;
    const bool writer = (lane & 3) == 0 && mykk == 0;
    const KcButterflyMasks masks = kc_butterfly_masks(lane);
    const int step = gridDim.x * W * R;
    int nchanged = 0;

    for (int m0 = 0; m0 < K; m0 += CH) {
        const int nm = min(CH, K - m0);
        const bool last = m0 + CH >= K;
        __syncthreads();
        kc_stage_rows_wide<NQ, W * 64>(cs, a.C + (size_t)m0 * a.ldc, a.ldc, nm, D, tid);
        __syncthreads();
        for (int r0 = (blockIdx.x * W + wave) * R; r0 < N; r0 += step) {
            f32x4 x[R][NQ];
#pragma unroll
            for (int r = 0; r < R; ++r)                      // a batch's tail repeats the last row
                kc_load_row<NQ>(a.X + (size_t)min(r0 + r, N - 1) * a.ld, D, lane, x[r]);
            const int row = r0 + myr;
            float bd = __builtin_inff();
            int bm = -1;
            for (int k0 = 0; k0 < nm; k0 += KK) {            // rows k0 + kk >= nm of cs: never candidates
                float v[kKmVals];
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    f32x4 c[NQ];
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
                        c[q] = *reinterpret_cast<const f32x4*>(cs + (k0 + kk) * (NQ * 256) + q * 256 + lane * 4);
#pragma unroll
                    for (int r = 0; r < R; ++r) v[kk * R + r] = kc_lane_chain<NQ>(x[r], c);
                }
                kc_butterfly<kKmVals>(v, masks);
                const float d = v[0];
                const int m = k0 + mykk;                     // ascending: an equal d does not replace
                if ((m < nm) & ((d < bd) | ((bm < 0) & (d == d)))) {
                    bd = d;
                    bm = m0 + m;
                }
            }
            // the lanes of a row that took other centres
#pragma unroll
            for (int n = kKmVals, o = 32; n > R; n >>= 1, o >>= 1) {
                const float od = __shfl_xor(bd, o);
                const int om = __shfl_xor(bm, o);
                if (km_before(od, om, bd, bm)) {
                    bd = od;
                    bm = om;
                }
            }
            if (writer && row < N) {
                if (m0 > 0) {                                // earlier chunks hold the lower indices
                    const float pd = a.dist[row];
                    const int pm = a.tmp[row];
                    if (!km_before(bd, bm, pd, pm)) {
                        bd = pd;
                        bm = pm;
                    }
                }
                a.dist[row] = bd;
                if (last) {
                    nchanged += a.label[row] != bm;
                    a.label[row] = bm;
                } else {
                    a.tmp[row] = bm;
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) nchanged += __shfl_xor(nchanged, off);
    if (lane == 0) red[wave] = nchanged;
    __syncthreads();
    if (tid == 0) {
        long long s = 0;
        for (int w = 0; w < W; ++w) s += red[w];
        a.chg[blockIdx.x] = s;
    }
}

// ---- histogram, scan, scatter -----------------------------------------------------------------------
// fixed-shape tree over the T values of a workgroup; the total in every thread
template <typename V, int T>
__device__ __forceinline__ V km_block_tree(V v, V* buf) {
    const int tid = threadIdx.x;
    __syncthreads();
    buf[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = T / 2; s >= 1; s >>= 1) {
        if (tid < s) buf[tid] = buf[tid] + buf[tid + s];
        __syncthreads();
    }
    return buf[0];
}

// grid NB x 256: block b owns the rows b RB .. ; labels outside 0..K-1 take no part
__global__ __launch_bounds__(256) void km_hist_kernel(const int* __restrict__ label, const float* __restrict__ dist,
                                                      const int N, const int K, const int RB, const int NB,
                                                      int* __restrict__ hist, double* __restrict__ ipart) {
    __shared__ int h[kKmMaxK];
    __shared__ double tree[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    for (int m = tid; m < K; m += 256) h[m] = 0;
    __syncthreads();
    const int i1 = min(N, (b + 1) * RB);
    double s = 0.0;
    for (int i = b * RB + tid; i < i1; i += 256) {
        const int l = label[i];
        if (l >= 0 && l < K) {
            atomicAdd(&h[l], 1);
            if (dist != nullptr) s += (double)dist[i];
        }
    }
    __syncthreads();
    for (int m = tid; m < K; m += 256) hist[(size_t)m * NB + b] = h[m];
    if (dist != nullptr) {
        s = km_block_tree<double, 256>(s, tree);
        if (tid == 0) ipart[b] = s;
    }
}

// exclusive scan of one int per thread of a workgroup of T threads; returns the prefix, the total in *total
template <int T>
__device__ __forceinline__ int km_block_scan(const int v, int* buf, int* total) {
    const int tid = threadIdx.x;
    __syncthreads();
    buf[tid] = v;
    __syncthreads();
    for (int s = 1; s < T; s <<= 1) {
        const int add = tid >= s ? buf[tid - s] : 0;
        __syncthreads();
        buf[tid] += add;
        __syncthreads();
    }
    *total = buf[T - 1];
    return buf[tid] - v;
}

// grid K x 256: the exclusive scan of cluster m's NB block counts, in place, and its total
__global__ __launch_bounds__(256) void km_scan_rows_kernel(int* __restrict__ hist, const int NB,
                                                           int* __restrict__ cnt, int64_t* __restrict__ counts) {
    __shared__ int ibuf[256];
    const int tid = threadIdx.x, m = blockIdx.x;
    int* row = hist + (size_t)m * NB;
    const int L = (NB + 255) / 256;                          // at most 8
    const int e0 = min(NB, tid * L), e1 = min(NB, e0 + L);
    int mine = 0;
    for (int e = e0; e < e1; ++e) mine += row[e];
    int total;
    int run = km_block_scan<256>(mine, ibuf, &total);
    for (int e = e0; e < e1; ++e) {
        const int c = row[e];
        row[e] = run;
        run += c;
    }
    if (tid == 0) {
        cnt[m] = total;
        if (counts != nullptr) counts[m] = total;
    }
}

struct KmScanArgs {
    int K, NB, RB, G;       // G: workgroups of the assign launch (0: none)
    const int* cnt;         // [K]
    int* base;              // [K]: where cluster m starts in the rows sorted by label
    int* ustart;            // [K + 1]: first work unit of a cluster, a unit = RB sorted rows of one cluster
    const double* ipart;    // [NB] or NULL
    const long long* chg;   // [G]
    double* inertia;        // one entry, or NULL
    int64_t* changed;
};

// one workgroup: the clusters' places and work units, and the fixed-order totals of an assignment
__global__ __launch_bounds__(kKmScanThreads) void km_scan_kernel(const KmScanArgs a) {
    __shared__ int ibuf[kKmScanThreads];
    __shared__ double dbuf[kKmScanThreads];
    __shared__ long long lbuf[kKmScanThreads];
    const int tid = threadIdx.x, K = a.K;
    const int n = tid < K ? a.cnt[tid] : 0;                  // K <= 1,024 = the workgroup
    int total, units;
    const int start = km_block_scan<kKmScanThreads>(n, ibuf, &total);
    const int first = km_block_scan<kKmScanThreads>((n + a.RB - 1) / a.RB, ibuf, &units);
    if (tid < K) {
        a.base[tid] = start;
        a.ustart[tid] = first;
    }
    if (tid == K - 1) a.ustart[K] = units;
    if (a.inertia != nullptr) {
        double s = 0.0;
        for (int b = tid; b < a.NB; b += kKmScanThreads) s += a.ipart[b];
        s = km_block_tree<double, kKmScanThreads>(s, dbuf);
        long long c = 0;
        for (int g = tid; g < a.G; g += kKmScanThreads) c += a.chg[g];
        c = km_block_tree<long long, kKmScanThreads>(c, lbuf);
        if (tid == 0) {
            a.inertia[0] = s;
            a.changed[0] = c;
        }
    }
}

// grid NB x 64: the wave of block b walks its rows in order; a row's place is the offset of its
// (cluster, block) run plus the rows of that label seen before it
__global__ __launch_bounds__(64) void km_scatter_kernel(const int* __restrict__ label, const int N, const int K,
                                                        const int RB, const int NB, const int* __restrict__ offs,
                                                        const int* __restrict__ base, int* __restrict__ sorted) {
    __shared__ int next[kKmMaxK];
    const int lane = threadIdx.x, b = blockIdx.x;
    for (int m = lane; m < K; m += 64) next[m] = base[m] + offs[(size_t)m * NB + b];
    __syncthreads();
    const int i1 = min(N, (b + 1) * RB);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int i0 = b * RB; i0 < i1; i0 += 64) {
        const int i = i0 + lane;
        int l = i < i1 ? label[i] : -1;
        if (l >= K) l = -1;
        unsigned long long todo = __ballot(l >= 0);
        while (todo) {                                       // wave-uniform: one trip per distinct label
            const int src = __builtin_ctzll(todo);
            const int cur = __shfl(l, src);
            const unsigned long long same = __ballot(l == cur);
            if (l == cur) {
                const int pos = next[cur] + __popcll(same & below);
                if (pos < N) sorted[pos] = i;
            }
            __syncthreads();
            if (lane == src) next[cur] += __popcll(same);
            __syncthreads();
            todo &= ~same;
        }
    }
}

// ---- the sums ----------------------------------------------------------------------------------------
struct KmSumArgs {
    const float* X;
    size_t ld;
    int N, D, K, NB, RB;
    const int* base;        // [K]: where cluster m starts in `sorted`
    const int* cnt;         // [K]
    const int* ustart;      // [K + 1]
    const int* sorted;
    double* part;           // [units][D]
    float* C;
    size_t ldc;
};

// grid (NB + K) x 256 (an upper bound of the units): thread t owns the columns 4 t + 1024 q
__global__ __launch_bounds__(256) void km_segsum_kernel(const KmSumArgs a) {
    const int tid = threadIdx.x, u = blockIdx.x, K = a.K;
    if (u >= a.ustart[K]) return;
    int lo = 0, hi = K - 1;                                  // the last m with ustart[m] <= u
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.ustart[mid] <= u) lo = mid;
        else hi = mid - 1;
    }
    const int m = lo, c = u - a.ustart[m];
    const int n = min(a.RB, a.cnt[m] - c * a.RB);
    const int* idx = a.sorted + a.base[m] + (size_t)c * a.RB;
    for (int j = tid * 4; j < a.D; j += 1024) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int t0 = 0; t0 < n; t0 += 8) {
            f32x4 x[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {                    // every load before the first addition
                const int i = min(max(idx[min(t0 + t, n - 1)], 0), a.N - 1);
                x[t] = *reinterpret_cast<const f32x4*>(a.X + (size_t)i * a.ld + j);
            }
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (t0 + t < n) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[e] += (double)x[t][e];
                }
        }
        double* out = a.part + (size_t)u * a.D + j;
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = s[e];
    }
}

// grid K x 256: an empty cluster keeps its centre
__global__ __launch_bounds__(256) void km_centre_kernel(const KmSumArgs a) {
    const int tid = threadIdx.x, m = blockIdx.x;
    const int n = a.cnt[m];
    if (n == 0) return;
    const int u0 = a.ustart[m], u1 = a.ustart[m + 1];
    for (int j = tid * 4; j < a.D; j += 1024) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int u = u0; u < u1; ++u) {
            const double* p = a.part + (size_t)u * a.D + j;
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += p[e];
        }
        f32x4 c;
#pragma unroll
        for (int e = 0; e < 4; ++e) c[e] = (float)(s[e] / (double)n);
        *reinterpret_cast<f32x4*>(a.C + (size_t)m * a.ldc + j) = c;
    }
}

// ---- host ----------------------------------------------------------------------------------------------
size_t km_up16(const size_t n) { return (n + 15) & ~(size_t)15; }

struct KmScratch {
    int* tmp;               // [N]: assign's running label, then the rows sorted by label
    int* hist;              // [K][NB]
    int* cnt;               // [K]
    int* base;              // [K]
    int* ustart;            // [K + 1]
    long long* chg;         // [kKmMaxGrid]
    double* ipart;          // [NB]
    double* part;           // [NB + K][D]
    size_t bytes;
};

KmScratch km_layout(void* base, const int N, const int D, const int K) {
    const size_t NB = km_blocks(N);
    char* p = (char*)base;
    size_t off = 0;
    KmScratch s;
    auto take = [&](const size_t nbytes) {
        char* at = p + off;
        off += km_up16(nbytes);
        return at;
    };
    s.tmp = (int*)take((size_t)N * 4);
    s.hist = (int*)take((size_t)K * NB * 4);
    s.cnt = (int*)take((size_t)K * 4);
    s.base = (int*)take((size_t)K * 4);
    s.ustart = (int*)take((size_t)(K + 1) * 4);
    s.chg = (long long*)take((size_t)kKmMaxGrid * 8);
    s.ipart = (double*)take(NB * 8);
    s.part = (double*)take((NB + K) * (size_t)D * 8);
    s.bytes = off;
    return s;
}

bool km_sizes_ok(const int N, const int D, const int K) {
    return N >= 1 && N <= kKcMaxN && D >= 4 && D <= kKcMaxD && D % 4 == 0 && K >= 1 && K <= kKmMaxK && K <= N;
}

struct KmProblem {
    const float* X;
    long ld;
    int N, D;
    float* C;
    long ldc;
    int K;
};

int km_check(const char* who, const KmProblem& p, const void* scratch, const size_t scratch_bytes) {
    CILRS_CHECK(p.X && p.C, "%s: NULL tensor", who);
    CILRS_CHECK(p.N >= 1 && p.N <= kKcMaxN, "%s: N = %d outside 1..%d", who, p.N, kKcMaxN);
    CILRS_CHECK(p.D >= 4 && p.D <= kKcMaxD && p.D % 4 == 0, "%s: D = %d outside 4..%d or not a multiple of 4",
                who, p.D, kKcMaxD);
    CILRS_CHECK(p.ld >= p.D && p.ld % 4 == 0, "%s: ld = %ld below D or not a multiple of 4", who, p.ld);
    CILRS_CHECK(p.ldc >= p.D && p.ldc % 4 == 0, "%s: ldc = %ld below D or not a multiple of 4", who, p.ldc);
    CILRS_CHECK(p.K >= 1 && p.K <= kKmMaxK && p.K <= p.N, "%s: K = %d outside 1..min(N, %d)", who, p.K, kKmMaxK);
    CILRS_CHECK(((uintptr_t)p.X & 15) == 0 && ((uintptr_t)p.C & 15) == 0, "%s: X and C must be 16-byte aligned",
                who);
    const size_t need = km_layout(nullptr, p.N, p.D, p.K).bytes;
    CILRS_CHECK(scratch != nullptr && scratch_bytes >= need, "%s: scratch of %zu bytes, needs %zu", who,
                scratch ? scratch_bytes : (size_t)0, need);
    CILRS_CHECK(((uintptr_t)scratch & 15) == 0, "%s: scratch is not 16-byte aligned", who);
    return 0;
}

// the histogram and the scan of the labels: counts, offsets, units (and the totals of an assignment)
int km_launch_count(const KmProblem& p, const KmScratch& w, const int* label, const float* dist, const int G,
                    int64_t* counts, double* inertia, int64_t* changed, hipStream_t s) {
    const int RB = km_block_rows(p.N), NB = km_blocks(p.N);
    km_hist_kernel<<<NB, 256, 0, s>>>(label, dist, p.N, p.K, RB, NB, w.hist, w.ipart);
    CILRS_LAUNCH_CHECK();
    km_scan_rows_kernel<<<p.K, 256, 0, s>>>(w.hist, NB, w.cnt, counts);
    CILRS_LAUNCH_CHECK();
    km_scan_kernel<<<1, kKmScanThreads, 0, s>>>(
        KmScanArgs{p.K, NB, RB, G, w.cnt, w.base, w.ustart, dist ? w.ipart : nullptr, w.chg, inertia, changed});
    CILRS_LAUNCH_CHECK();
    return 0;
}

int km_launch_assign(const KmProblem& p, const KmScratch& w, int* label, float* dist, int64_t* counts,
                     double* inertia, int64_t* changed, hipStream_t s) {
    const int rows = p.D <= 512 ? 4 : p.D <= 1024 ? 2 : 1, waves = p.D <= 512 ? kKmWaves : kKmWavesWide;
    const int cus = device_cus();
    const int g = max(1, min(min(cus > 0 ? cus : 256, kKmMaxGrid), cdiv(p.N, waves * rows)));
    const KmAssignArgs a{p.X, (size_t)p.ld, p.N, p.D, p.C, (size_t)p.ldc, p.K, label, dist, w.tmp, w.chg};
    if (p.D <= 256) km_assign_kernel<1, 4, kKmWaves><<<g, kKmWaves * 64, 0, s>>>(a);
    else if (p.D <= 512) km_assign_kernel<2, 4, kKmWaves><<<g, kKmWaves * 64, 0, s>>>(a);
    else if (p.D <= 1024) km_assign_kernel<4, 2, kKmWavesWide><<<g, kKmWavesWide * 64, 0, s>>>(a);
    else km_assign_kernel<8, 1, kKmWavesWide><<<g, kKmWavesWide * 64, 0, s>>>(a);
    CILRS_LAUNCH_CHECK();
    return km_launch_count(p, w, label, dist, g, counts, inertia, changed, s);
}

// after km_launch_count of the same labels
int km_launch_sums(const KmProblem& p, const KmScratch& w, const int* label, hipStream_t s) {
    const int RB = km_block_rows(p.N), NB = km_blocks(p.N);
    km_scatter_kernel<<<NB, 64, 0, s>>>(label, p.N, p.K, RB, NB, w.hist, w.base, w.tmp);
    CILRS_LAUNCH_CHECK();
    const KmSumArgs a{p.X, (size_t)p.ld, p.N, p.D, p.K, NB, RB, w.base, w.cnt, w.ustart, w.tmp, w.part, p.C, (size_t)p.ldc};
    km_segsum_kernel<<<NB + p.K, 256, 0, s>>>(a);
    CILRS_LAUNCH_CHECK();
    km_centre_kernel<<<p.K, 256, 0, s>>>(a);
    CILRS_LAUNCH_CHECK();
    return 0;
}

}  // namespace
}  // namespace cilrs

using namespace cilrs;

extern "C" {

size_t cilrs_kmeans_scratch_bytes(int N, int D, int K) {
    if (!km_sizes_ok(N, D, K)) return 0;
    return km_layout(nullptr, N, D, K).bytes;
}

int cilrs_kmeans_assign(const float* X, long ld, int N, int D, const float* C, long ldc, int K, int32_t* label,
                        float* dist, int64_t* counts, double* inertia, int64_t* changed, void* scratch,
                        size_t scratch_bytes, void* stream) {
    const KmProblem p{X, ld, N, D, const_cast<float*>(C), ldc, K};
    CILRS_CHECK(label && dist && counts && inertia && changed, "kmeans_assign: NULL tensor");
    if (km_check("kmeans_assign", p, scratch, scratch_bytes)) return 1;
    return km_launch_assign(p, km_layout(scratch, N, D, K), label, dist, counts, inertia, changed,
                            (hipStream_t)stream);
}

int cilrs_kmeans_update(const float* X, long ld, int N, int D, const int32_t* label, float* C, long ldc, int K,
                        int64_t* counts, void* scratch, size_t scratch_bytes, void* stream) {
    const KmProblem p{X, ld, N, D, C, ldc, K};
    CILRS_CHECK(label && counts, "kmeans_update: NULL tensor");
    if (km_check("kmeans_update", p, scratch, scratch_bytes)) return 1;
    const KmScratch w = km_layout(scratch, N, D, K);
    hipStream_t s = (hipStream_t)stream;
    if (km_launch_count(p, w, label, nullptr, 0, counts, nullptr, nullptr, s)) return 1;
    return km_launch_sums(p, w, label, s);
}

int cilrs_kmeans_lloyd(const float* X, long ld, int N, int D, float* C, long ldc, int K, int iters, int32_t* label,
                       float* dist, int64_t* counts, double* inertia, int64_t* changed, void* scratch,
                       size_t scratch_bytes, void* stream) {
    const KmProblem p{X, ld, N, D, C, ldc, K};
    CILRS_CHECK(label && dist && counts && inertia && changed, "kmeans_lloyd: NULL tensor");
    CILRS_CHECK(iters >= 0 && iters <= kKmMaxIters, "kmeans_lloyd: iters = %d outside 0..%d", iters, kKmMaxIters);
    if (km_check("kmeans_lloyd", p, scratch, scratch_bytes)) return 1;
    const KmScratch w = km_layout(scratch, N, D, K);
    hipStream_t s = (hipStream_t)stream;
    for (int t = 0; t <= iters; ++t) {
        if (km_launch_assign(p, w, label, dist, counts, inertia + t, changed + t, s)) return 1;
        if (t < iters && km_launch_sums(p, w, label, s)) return 1;
    }
    return 0;
}

}  // extern "C"
