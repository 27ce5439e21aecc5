// Sharpness-aware minimisation (SAM / ASAM): the perturbation of a flat range of the parameter
// arena and its bit-exact undo.  include/cilrs_hip.h "sharpness-aware minimisation" states the
// arithmetic; neither the reference nor torch has one.
//
// Work decomposition: the range is cut from its own start into chunks of kChunkFloats floats, one
// workgroup each, whose thread t takes the chunk's quads t, t + 256, ...  cilrs_sam_perturb is three
// launches on one stream: chunk sums (p, g -> one double per chunk), finalise (one workgroup adds
// the chunk sums in index order and writes {S, norm, scale}), apply (p, g -> backup, p) over the same
// chunks.  The sums are butterflies over the 64 lanes of a wave and a fixed tree over the four waves,
// all in double; no atomics, so the result is a function of the range's data alone.
//
// The whole file is compiled without FMA contraction: the apply pass rounds every product and sum
// of the definition separately, and t = |p| * g of the adaptive form is the same fp32 number in the
// norm pass and in the apply pass.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/cilrs_hip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace cilrs {
namespace {

constexpr int kChunkFloats = 4096;                     // 256 threads x 4 quads
constexpr int kChunkQuads = kChunkFloats / 4;
constexpr size_t kMaxFloats = (size_t)1 << 30;         // 2^18 chunk sums: 1,024 per finalise thread

// fixed-order butterfly sum over the 64 lanes of a wave, in double
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// sum over the 256 threads of the workgroup (valid in thread 0): wave butterflies, then
// (w0 + w1) + (w2 + w3)
__device__ __forceinline__ double block_sum_f64(double v, double* red4) {
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red4[0] + red4[1]) + (red4[2] + red4[3]);
}

// quads of chunk c of a range of nquads quads
__device__ __forceinline__ unsigned chunk_quads(const size_t nquads, const size_t c) {
    const size_t left = nquads - c * kChunkQuads;
    return left < (size_t)kChunkQuads ? (unsigned)left : (unsigned)kChunkQuads;
}

template <int ADAPTIVE>
__global__ __launch_bounds__(256) void sam_chunk_sums_kernel(
    const float* __restrict__ p, const float* __restrict__ g, const size_t nquads,
    double* __restrict__ partial) {
    __shared__ double red4[4];
    const size_t c = blockIdx.x;
    const unsigned quads = chunk_quads(nquads, c);
    double s = 0.0;
    for (unsigned q = threadIdx.x; q < quads; q += 256) {
        const size_t i = (c * kChunkQuads + q) * 4;
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
        f32x4 tv = gv;
        if (ADAPTIVE) {
            const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) tv[e] = fabsf(pv[e]) * gv[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) s += (double)tv[e] * (double)tv[e];
    }
    s = block_sum_f64(s, red4);
    if (threadIdx.x == 0) partial[c] = s;
}

// thread l adds the chunk sums l, l + 256, ... in index order, the tree adds the 256 threads
__global__ __launch_bounds__(256) void sam_finalize_kernel(
    const double* __restrict__ partial, const unsigned nchunks, const double rho,
    double* __restrict__ out3) {
    __shared__ double red4[4];
    double s = 0.0;
    for (unsigned c = threadIdx.x; c < nchunks; c += 256) s += partial[c];
    s = block_sum_f64(s, red4);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(s);
    out3[0] = s;
    out3[1] = norm;
    out3[2] = rho / (norm + 1e-12);
}

template <int ADAPTIVE>
__global__ __launch_bounds__(256) void sam_apply_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ backup,
    const size_t nquads, const double* __restrict__ out3) {
    const float s32 = (float)out3[2];
    const size_t c = blockIdx.x;
    const unsigned quads = chunk_quads(nquads, c);
    for (unsigned q = threadIdx.x; q < quads; q += 256) {
        const size_t i = (c * kChunkQuads + q) * 4;
        f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
        *reinterpret_cast<f32x4*>(backup + i) = pv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float d = gv[e];
            if (ADAPTIVE) {
                const float a = fabsf(pv[e]);
                const float t = a * gv[e];
                d = a * t;
            }
            const float step = s32 * d;
            pv[e] = pv[e] + step;
        }
        *reinterpret_cast<f32x4*>(p + i) = pv;
    }
}

__global__ __launch_bounds__(256) void sam_restore_kernel(
    float* __restrict__ p, const float* __restrict__ backup, const size_t nquads) {
    const size_t c = blockIdx.x;
    const unsigned quads = chunk_quads(nquads, c);
    // moved as integers: every bit pattern (-0.0, denormals, NaN payloads) comes back as it was
    for (unsigned q = threadIdx.x; q < quads; q += 256) {
        const size_t i = (c * kChunkQuads + q) * 4;
        *reinterpret_cast<uint4*>(p + i) = *reinterpret_cast<const uint4*>(backup + i);
    }
}

bool aligned(const void* q, const uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; }

bool overlap(const void* a, const void* b, const size_t bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}

size_t chunks_of(const size_t n) { return (n + kChunkFloats - 1) / kChunkFloats; }

}  // namespace
}  // namespace cilrs

using namespace cilrs;

extern "C" {

int cilrs_sam_chunk_floats(void) { return kChunkFloats; }

size_t cilrs_sam_scratch_bytes(size_t n) {
    if (n == 0 || n > kMaxFloats) return 0;
    const size_t bytes = (chunks_of(n) + 3) * sizeof(double);
    return (bytes + 15) / 16 * 16;
}

int cilrs_sam_perturb(float* params, const float* grads, float* backup, size_t n, double rho,
                      int adaptive, void* scratch, double* out3, void* stream) {
    CILRS_CHECK(params && grads && backup && scratch && out3,
                "sam perturb: NULL params / grads / backup / scratch / out3");
    CILRS_CHECK(n > 0 && n % 4 == 0, "sam perturb: n = %zu must be a positive multiple of 4", n);
    CILRS_CHECK(n <= kMaxFloats, "sam perturb: n = %zu above 2^30", n);
    CILRS_CHECK(aligned(params, 16) && aligned(grads, 16) && aligned(backup, 16),
                "sam perturb: params, grads and backup pointers must be 16-byte aligned");
    CILRS_CHECK(aligned(scratch, 16), "sam perturb: scratch must be 16-byte aligned");
    CILRS_CHECK(aligned(out3, 8), "sam perturb: out3 must be 8-byte aligned");
    CILRS_CHECK(!overlap(backup, params, n * sizeof(float)) && !overlap(backup, grads, n * sizeof(float)),
                "sam perturb: backup overlaps params or grads");
    CILRS_CHECK(std::isfinite(rho) && rho >= 0.0, "sam perturb: rho %g must be finite and >= 0", rho);
    CILRS_CHECK(adaptive == 0 || adaptive == 1, "sam perturb: adaptive %d (0 or 1)", adaptive);

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t nquads = n / 4;
    const unsigned nchunks = (unsigned)chunks_of(n);
    double* partial = reinterpret_cast<double*>(scratch);
    if (adaptive)
        sam_chunk_sums_kernel<1><<<nchunks, 256, 0, s>>>(params, grads, nquads, partial);
    else
        sam_chunk_sums_kernel<0><<<nchunks, 256, 0, s>>>(params, grads, nquads, partial);
    CILRS_LAUNCH_CHECK();
    sam_finalize_kernel<<<1, 256, 0, s>>>(partial, nchunks, rho, out3);
    CILRS_LAUNCH_CHECK();
    if (adaptive)
        sam_apply_kernel<1><<<nchunks, 256, 0, s>>>(params, grads, backup, nquads, out3);
    else
        sam_apply_kernel<0><<<nchunks, 256, 0, s>>>(params, grads, backup, nquads, out3);
    CILRS_LAUNCH_CHECK();
    return 0;
}

int cilrs_sam_restore(float* params, const float* backup, size_t n, void* stream) {
    CILRS_CHECK(params && backup, "sam restore: NULL params / backup");
    CILRS_CHECK(n > 0 && n % 4 == 0, "sam restore: n = %zu must be a positive multiple of 4", n);
    CILRS_CHECK(n <= kMaxFloats, "sam restore: n = %zu above 2^30", n);
    CILRS_CHECK(aligned(params, 16) && aligned(backup, 16),
                "sam restore: params and backup pointers must be 16-byte aligned");
    CILRS_CHECK(!overlap(backup, params, n * sizeof(float)), "sam restore: backup overlaps params");
    sam_restore_kernel<<<(unsigned)chunks_of(n), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
        params, backup, n / 4);
    CILRS_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
