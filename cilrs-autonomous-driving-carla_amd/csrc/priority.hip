// Loss-prioritised batch sampling: the per-sample loss of a step, a fixed-point priority table in
// device memory and the draw of the next batch's index from it.  include/cilrs_hip.h "prioritised
// sampling" states the arithmetic; the reference samples by command only and has none of it.
//
// The table is uint32 with every entry in [1, 2^32 - 1] and every sum is uint64, so the total, the
// prefix sums and with them the drawn positions do not depend on how the additions are grouped:
// chunk sums by butterflies, the scan by tiles and the lane prefix inside a chunk give the numbers
// a sequential cumsum gives.
//
// cilrs_priority_draw is three launches on one stream: chunk sums (one workgroup per kChunk
// entries), the exclusive scan of the chunk sums (one workgroup), the draw (one workgroup, one wave
// per sample: 64-ary search of the chunk prefix, then the lane prefix of the sample's chunk).  The
// draw is one workgroup because the importance weights are normalised by their maximum over the
// batch, which its waves exchange through LDS.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/cilrs_hip.h"
#include "common.h"

namespace cilrs {
namespace {

typedef unsigned long long u64;

constexpr int kChunk = 1024;                      // table entries per chunk sum: 256 threads x uint4
constexpr int kMaxBatch = 1024;                   // one workgroup: a thread (update) or a slot (draw) each
constexpr long long kMaxEntries = 1ll << 31;      // total < 2^63
constexpr unsigned kQMax = 0xFFFFFFFFu;
constexpr double kFixedOne = 1048576.0;           // 2^20: the fixed-point value of priority 1
constexpr u64 kDrawStride = 0xD1B54A32D192ED03ull;

__global__ __launch_bounds__(256) void loss_rows_kernel(
    const float* __restrict__ pc, const float* __restrict__ tc, const float* __restrict__ ps,
    const float* __restrict__ ts, const int B, const int kind, const float w0, const float w1,
    const float w2, const float w3, const float grad_scale, float* __restrict__ dpc,
    float* __restrict__ dps, float* __restrict__ out, const float* __restrict__ row_weight,
    float* __restrict__ row_loss) {
    loss_block<true>(pc, tc, ps, ts, B, kind, w0, w1, w2, w3, grad_scale, dpc, dps, out, row_weight,
                     row_loss);
}

// llrint(p * 2^20) clamped to [1, 2^32 - 1]; whatever is not below the upper end, NaN included,
// takes it
__device__ __forceinline__ unsigned to_fixed(const double p) {
    const double v = p * kFixedOne;
    if (!(v < 4294967295.0)) return kQMax;
    if (!(v >= 1.0)) return 1u;
    return (unsigned)llrint(v);
}

// x^alpha in double; 0, 1 and 0.5 are exact (1, x, sqrt), every other exponent is pow's
__device__ __forceinline__ double pow_alpha(const double x, const double alpha) {
    if (alpha == 0.0) return 1.0;
    if (alpha == 1.0) return x;
    if (alpha == 0.5) return sqrt(x);
    return pow(x, alpha);
}

// q[i] = fixed(base[i] * pmax / 2^20): what a frame holds before its first visit
__global__ __launch_bounds__(256) void priority_fill_kernel(
    unsigned* __restrict__ q, const long long N, const float* __restrict__ base,
    const unsigned* __restrict__ pmax_state) {
    const double pmax = (double)pmax_state[0] * (1.0 / kFixedOne);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N;
         i += (long long)gridDim.x * 256)
        q[i] = to_fixed((base ? (double)base[i] : 1.0) * pmax);
}

// One workgroup of kMaxBatch threads, thread b for sample b.  A position that repeats is written
// by its highest b alone: every thread looks through LDS for a later sample with its position.
__global__ __launch_bounds__(kMaxBatch) void priority_update_kernel(
    unsigned* __restrict__ q, const long long N, const long long* __restrict__ pos,
    const float* __restrict__ row_loss, const float* __restrict__ base, const double alpha,
    const double eps, unsigned* __restrict__ pmax_state, const int B) {
    __shared__ long long spos[kMaxBatch];
    __shared__ unsigned smax[kMaxBatch / 64];
    const int b = threadIdx.x;
    long long p = -1;
    if (b < B) {
        p = pos[b];
        if (p < 0 || p >= N) p = -1;                // never written, and shadows nothing
    }
    spos[b] = p;
    __syncthreads();
    bool wins = p >= 0;
    for (int j = b + 1; wins && j < B; ++j) wins = spos[j] != p;
    unsigned v = 0;
    if (wins) {
        const float loss = row_loss[b];
        if (!isfinite(loss)) {
            v = kQMax;
        } else {
            const double bs = base ? (double)base[p] : 1.0;
            v = to_fixed(bs * pow_alpha((double)loss + eps, alpha));
        }
        q[p] = v;
    }
    unsigned m = v;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned o = __shfl_xor(m, off);
        m = o > m ? o : m;
    }
    if ((b & 63) == 0) smax[b >> 6] = m;
    __syncthreads();
    if (b == 0) {
        unsigned best = pmax_state[0];
        for (int w = 0; w < kMaxBatch / 64; ++w) best = smax[w] > best ? smax[w] : best;
        pmax_state[0] = best;
    }
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the four entries from i on, zeros from N on (q is 16-byte aligned and i a multiple of 4)
__device__ __forceinline__ uint4 load_quad(const unsigned* __restrict__ q, const long long N,
                                           const long long i) {
    if (i + 4 <= N) return *reinterpret_cast<const uint4*>(q + i);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (i < N) v.x = q[i];
    if (i + 1 < N) v.y = q[i + 1];
    if (i + 2 < N) v.z = q[i + 2];
    return v;
}

// sums[c] = sum of the entries of chunk c, one workgroup each
__global__ __launch_bounds__(256) void priority_chunk_sums_kernel(
    const unsigned* __restrict__ q, const long long N, u64* __restrict__ sums) {
    __shared__ u64 red4[4];
    const uint4 v = load_quad(q, N, (long long)blockIdx.x * kChunk + threadIdx.x * 4);
    const u64 s = wave_sum_u64((u64)v.x + v.y + v.z + v.w);
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = red4[0] + red4[1] + red4[2] + red4[3];
}

// sums[0 .. nchunks) -> their exclusive prefix in place, sums[nchunks] = the total; one workgroup,
// tiles of 256 sums
__global__ __launch_bounds__(256) void priority_scan_kernel(u64* __restrict__ sums,
                                                            const int nchunks) {
    __shared__ u64 wtot[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 carry = 0;
    for (int base = 0; base < nchunks; base += 256) {
        const int i = base + threadIdx.x;
        const u64 v = i < nchunks ? sums[i] : 0;
        u64 incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const u64 o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        u64 before = carry;
        for (int w = 0; w < wave; ++w) before += wtot[w];
        if (i < nchunks) sums[i] = before + incl - v;
        carry += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[nchunks] = carry;
}

// One workgroup of 16 waves; wave w draws samples w, w + 16, ...  prefix = the scanned chunk sums.
__global__ __launch_bounds__(kMaxBatch) void priority_draw_kernel(
    const unsigned* __restrict__ q, const long long N, const long long* __restrict__ subset,
    const u64* __restrict__ prefix, const int nchunks, const u64 seed, const u64 counter,
    const int B, const int stratified, const double beta, long long* __restrict__ out_pos,
    long long* __restrict__ out_index, float* __restrict__ out_weight) {
    __shared__ unsigned qsel[kMaxBatch];
    __shared__ double wmax[kMaxBatch / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 total = prefix[nchunks];
    const u64 quo = total / (u64)B, rem = total % (u64)B;
    for (int b = wave; b < B; b += kMaxBatch / 64) {
        const u64 r = splitmix64(seed + (counter * (u64)B + (u64)b) * kDrawStride);
        u64 t;
        if (stratified && total >= (u64)B) {
            const u64 lo = quo * (u64)b + ((u64)b < rem ? (u64)b : rem);
            const u64 len = quo + ((u64)b < rem ? 1u : 0u);
            t = lo + __umul64hi(r, len);
        } else {
            t = __umul64hi(r, total);
        }
        // the chunk whose exclusive prefix is the last one <= t: 64 probes a round; prefix[lo] <= t
        // throughout, and the probes' answers are true up to some lane and false from there on
        int lo = 0, hi = nchunks;
        while (hi - lo > 1) {
            const int step = (hi - lo + 63) >> 6;
            const long long probe = (long long)lo + (long long)lane * step;
            const bool le = probe < hi && prefix[probe] <= t;
            const int k = __popcll(__ballot(le)) - 1;
            const int nlo = lo + k * step;
            hi = nlo + step < hi ? nlo + step : hi;
            lo = nlo;
        }
        // inside the chunk: 16 entries a lane, the lanes' inclusive prefix, the first lane past left
        const u64 left = t - prefix[lo];
        const long long first = (long long)lo * kChunk + lane * 16;
        unsigned e[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 v = load_quad(q, N, first + k * 4);
            e[k * 4] = v.x; e[k * 4 + 1] = v.y; e[k * 4 + 2] = v.z; e[k * 4 + 3] = v.w;
        }
        u64 mine = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) mine += e[k];
        u64 incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const u64 o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        const u64 past = __ballot(incl > left);     // never empty: left < the chunk's sum
        if (past != 0 && lane == __ffsll((long long)past) - 1) {
            u64 acc = incl - mine;
            int k = -1;
            unsigned ek = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {          // the first entry whose running sum passes left
                acc += e[j];
                if (k < 0 && acc > left) {
                    k = j;
                    ek = e[j];
                }
            }
            const long long p = first + k;
            out_pos[b] = p;
            out_index[b] = subset ? subset[p] : p;
            qsel[b] = ek;
        }
    }
    __syncthreads();
    // importance weights (total / (N q))^beta over their maximum in the batch, in double
    double w = 0.0;
    if ((int)threadIdx.x < B)
        w = pow((double)total / ((double)N * (double)qsel[threadIdx.x]), beta);
    double m = w;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    if (lane == 0) wmax[wave] = m;
    __syncthreads();
    m = wmax[0];
    for (int k = 1; k < kMaxBatch / 64; ++k) m = fmax(m, wmax[k]);
    if ((int)threadIdx.x < B) out_weight[threadIdx.x] = (float)(w / m);
}

bool aligned(const void* p, const uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

long long chunks_of(const long long n) { return (n + kChunk - 1) / kChunk; }

}  // namespace
}  // namespace cilrs

using namespace cilrs;

extern "C" {

int cilrs_loss_fwd_bwd_rows(const float* controls, const float* target_controls,
                            const float* pred_speed, const float* target_speed, int batch, int kind,
                            const float* weights4_host, float grad_scale, float* dcontrols,
                            float* dpred_speed, float* loss_out, const float* row_weight,
                            float* row_loss, void* stream) {
    CILRS_CHECK(controls && target_controls && pred_speed && target_speed && weights4_host &&
                    loss_out, "loss rows: NULL argument");
    CILRS_CHECK(batch >= 1, "loss rows: batch must be >= 1");
    CILRS_CHECK(kind == 0 || kind == 1, "loss rows: kind must be 0 (MSE) or 1 (L1)");
    const float* w = weights4_host;
    loss_rows_kernel<<<1, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        controls, target_controls, pred_speed, target_speed, batch, kind, w[0], w[1], w[2], w[3],
        grad_scale, dcontrols, dpred_speed, loss_out, row_weight, row_loss);
    CILRS_LAUNCH_CHECK();
    return 0;
}

int cilrs_priority_max_batch(void) { return kMaxBatch; }

int cilrs_priority_fill(uint32_t* q, int64_t n, const float* base, const uint32_t* pmax_state,
                        void* stream) {
    CILRS_CHECK(q && pmax_state, "priority fill: NULL q / pmax_state");
    CILRS_CHECK(n >= 1 && n <= kMaxEntries, "priority fill: n = %lld outside [1, 2^31]", (long long)n);
    const long long blocks = (n + 255) / 256;
    priority_fill_kernel<<<(unsigned)(blocks < 4096 ? blocks : 4096), 256, 0,
                           reinterpret_cast<hipStream_t>(stream)>>>(q, n, base, pmax_state);
    CILRS_LAUNCH_CHECK();
    return 0;
}

int cilrs_priority_update(uint32_t* q, int64_t n, const int64_t* pos, const float* row_loss,
                          const float* base, double alpha, double eps, uint32_t* pmax_state,
                          int batch, void* stream) {
    CILRS_CHECK(q && pos && row_loss && pmax_state,
                "priority update: NULL q / pos / row_loss / pmax_state");
    CILRS_CHECK(n >= 1 && n <= kMaxEntries, "priority update: n = %lld outside [1, 2^31]",
                (long long)n);
    CILRS_CHECK(batch >= 1 && batch <= kMaxBatch, "priority update: batch %d outside [1, %d]", batch,
                kMaxBatch);
    CILRS_CHECK(std::isfinite(alpha) && alpha >= 0.0, "priority update: alpha %g must be finite and "
                ">= 0", alpha);
    CILRS_CHECK(std::isfinite(eps) && eps > 0.0, "priority update: eps %g must be finite and > 0",
                eps);
    priority_update_kernel<<<1, kMaxBatch, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        q, n, reinterpret_cast<const long long*>(pos), row_loss, base, alpha, eps, pmax_state, batch);
    CILRS_LAUNCH_CHECK();
    return 0;
}

size_t cilrs_priority_scratch_bytes(int64_t n) {
    if (n < 1 || n > kMaxEntries) return 0;
    return ((size_t)chunks_of(n) + 1) * sizeof(u64);
}

int cilrs_priority_draw(const uint32_t* q, int64_t n, const int64_t* subset, int64_t n_frames,
                        uint64_t seed, uint64_t counter, int batch, int stratified, double beta,
                        int64_t* out_pos, int64_t* out_index, float* out_weight, void* scratch,
                        void* stream) {
    CILRS_CHECK(q && out_pos && out_index && out_weight && scratch,
                "priority draw: NULL q / out_pos / out_index / out_weight / scratch");
    CILRS_CHECK(n >= 1 && n <= kMaxEntries, "priority draw: n = %lld outside [1, 2^31]", (long long)n);
    CILRS_CHECK(subset ? n_frames >= 1 : n_frames >= n, "priority draw: n_frames = %lld cannot hold "
                "the drawn indices", (long long)n_frames);
    CILRS_CHECK(batch >= 1 && batch <= kMaxBatch, "priority draw: batch %d outside [1, %d]", batch,
                kMaxBatch);
    CILRS_CHECK(stratified == 0 || stratified == 1, "priority draw: stratified %d (0 or 1)", stratified);
    CILRS_CHECK(std::isfinite(beta) && beta >= 0.0 && beta <= 1.0, "priority draw: beta %g outside "
                "[0, 1]", beta);
    CILRS_CHECK(aligned(q, 16), "priority draw: q must be 16-byte aligned");
    CILRS_CHECK(aligned(scratch, 8), "priority draw: scratch must be 8-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nchunks = (int)chunks_of(n);
    u64* sums = reinterpret_cast<u64*>(scratch);
    priority_chunk_sums_kernel<<<nchunks, 256, 0, s>>>(q, n, sums);
    CILRS_LAUNCH_CHECK();
    priority_scan_kernel<<<1, 256, 0, s>>>(sums, nchunks);
    CILRS_LAUNCH_CHECK();
    priority_draw_kernel<<<1, kMaxBatch, 0, s>>>(
        q, n, reinterpret_cast<const long long*>(subset), sums, nchunks, seed, counter, batch,
        stratified, beta, reinterpret_cast<long long*>(out_pos),
        reinterpret_cast<long long*>(out_index), out_weight);
    CILRS_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
