// FGSM / PGD on the network's input (Predictor.adversarial, evaluate.adversarial_sweep, the
// adversarial train step of Trainer): the element-wise work between two passes of the network.
//
//   cilrs_adv_start      x_adv = x + e_c * (2u - 1), a uniform start inside the eps ball
//   cilrs_adv_step       keep the best iterate, signed step, projection onto the eps ball (and range)
//   cilrs_adv_direction  per frame: deviation of the outputs, ascent direction, "is this the best"
//   cilrs_adv_quantize   the iterate as an 8-bit camera frame and its distance from the clean frame
//
// The gradients in between are cilrs_net_forward_frozen (or a train-mode forward) +
// cilrs_net_backward_data + cilrs_net_input_grads.  include/cilrs_hip.h "adversarial robustness"
// is the definition.  The reference has no counterpart: it never differentiates with respect to
// the camera frame (model/autonomous_drive.py:908-920).
//
// Every float operation is rounded once, in the order written (plain operators under
// `#pragma clang fp contract(off)`, as in attribution.hip), so each result is the fp32 numpy
// expression bit for bit.  No atomics; the one reduction (linf) is over integers in a fixed order.
//
// Layouts.  The tensors are logical NCHW [B,3,H,W] with element strides.  Two layouts are dense --
// contiguous NCHW, and the loaders' channels-last view with strides (3HW, 1, 3W, 3) -- and when
// every tensor of a call has the same dense layout, H * W is a multiple of 4 and the pointers are
// 16-byte aligned, a thread moves four floats that are adjacent in memory with one 16-byte access
// per tensor (kNCHW: four pixels of one plane; kNHWC: four floats of a row of interleaved pixels,
// their channels (m + j) % 3).  Anything else takes the scalar path: one logical element per thread
// through the strides.  The per-channel constants are picked with selects, never from an indexed
// array: nothing goes to scratch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/cilrs_hip.h"
#include "common.h"

namespace cilrs {
namespace {

#pragma clang fp contract(off)      // keep a * b + c as two roundings: numpy-identical arithmetic

constexpr int kAdvThreads = 256;       // start, step: grid-stride streaming
constexpr int kAdvQuantThreads = 1024;  // quantize: one workgroup per frame (as saliency_map_kernel)
// B * 3 * H * W at most: element indices, and a loop variable one stride past them, fit an int
constexpr long long kAdvMaxElems = 1ll << 30;

enum { kStrided = 0, kNCHW = 1, kNHWC = 2 };

struct Strides {
    long long n, c, h, w;
};

// per-channel constants of one call
struct AdvChan {
    float e0, e1, e2;          // eps255 * chan_scale3[c]
    float a0, a1, a2;          // alpha255 * chan_scale3[c]
    float lo0, lo1, lo2;       // range6 (use_range)
    float hi0, hi1, hi2;
    int use_range;
};

__device__ __forceinline__ float pick(const int c, const float v0, const float v1, const float v2) {
    return c == 0 ? v0 : (c == 1 ? v1 : v2);
}

// the uniform draw of attribution.hip's u1: the first 24-bit field, in (0, 1]
__device__ __forceinline__ float hash_u1(const unsigned long long seed,
                                         const unsigned long long counter) {
    const unsigned long long hsh = splitmix64(seed + counter * 0xD1B54A32D192ED03ull);
    return ((float)(unsigned int)(hsh >> 40) + 1.0f) * (1.0f / 16777216.0f);
}

// projection: the eps ball around x, then the valid range
__device__ __forceinline__ float project(float t, const float x, const int c, const AdvChan& k) {
    const float e = pick(c, k.e0, k.e1, k.e2);
    t = fminf(fmaxf(t, x - e), x + e);
    if (k.use_range)
        t = fminf(fmaxf(t, pick(c, k.lo0, k.lo1, k.lo2)), pick(c, k.hi0, k.hi1, k.hi2));
    return t;
}

__device__ __forceinline__ float start_value(const float x, const int c,
                                             const unsigned long long seed,
                                             const unsigned long long counter, const AdvChan& k) {
    const float u = hash_u1(seed, counter);
    const float r = (u + u) - 1.0f;
    const float t = x + pick(c, k.e0, k.e1, k.e2) * r;
    return project(t, x, c, k);
}

__device__ __forceinline__ float step_value(const float xa, const float x, const float g, const int c,
                                            const float d, const AdvChan& k) {
    const float s = g > 0.f ? 1.0f : (g < 0.f ? -1.0f : 0.f);      // NaN: 0
    const float t = xa + (pick(c, k.a0, k.a1, k.a2) * d) * s;
    return project(t, x, c, k);
}

// Scalar path: logical element i = ((b*3 + c)*H + y)*W + x of a strided tensor.
struct Elem {
    int b, c, y, x;
    __device__ __forceinline__ Elem(const long long i, const int H, const int W) {
        x = (int)(i % W);
        long long t = i / W;
        y = (int)(t % H);
        t /= H;
        c = (int)(t % 3);
        b = (int)(t / 3);
    }
    __device__ __forceinline__ long long at(const Strides& s) const {
        return (long long)b * s.n + (long long)c * s.c + (long long)y * s.h + (long long)x * s.w;
    }
};

// Wide paths: group i = the four floats at memory offset m = 4 i of a dense tensor.  Returns the
// frame; c[j] / counter[j] = the channel and the logical index of float m + j.
template <int L>
__device__ __forceinline__ int decode4(const long long m, const int HW, int c[4],
                                       unsigned long long counter[4]) {
    const long long per = 3ll * HW;
    const int b = (int)(m / per);
    if constexpr (L == kNCHW) {
        const int ch = (int)((m / HW) % 3);      // HW % 4 == 0: one plane for all four
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[j] = ch;
            counter[j] = (unsigned long long)(m + j);
        }
    } else {
        const int rem = (int)(m - (long long)b * per);      // per % 4 == 0: one frame for all four
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = (rem + j) / 3;
            c[j] = (rem + j) - 3 * p;
            counter[j] = ((unsigned long long)b * 3ull + (unsigned long long)c[j]) *
                             (unsigned long long)HW + (unsigned long long)p;
        }
    }
    return b;
}

template <int L>
__global__ __launch_bounds__(kAdvThreads) void adv_start_kernel(
    const float* __restrict__ x, const Strides xs, const int H, const int W, const long long total,
    const int draw, const unsigned long long seed, const AdvChan k, float* __restrict__ x_adv,
    const Strides as) {
    const int HW = H * W;
    for (long long i = (long long)blockIdx.x * kAdvThreads + threadIdx.x; i < total;
         i += (long long)gridDim.x * kAdvThreads) {
        if constexpr (L == kStrided) {
            const Elem el(i, H, W);
            const float v = x[el.at(xs)];
            x_adv[el.at(as)] = draw ? start_value(v, el.c, seed, (unsigned long long)i, k) : v;
        } else {
            const long long m = i * 4;
            f32x4 v = *reinterpret_cast<const f32x4*>(x + m);
            if (draw) {
                int c[4];
                unsigned long long counter[4];
                decode4<L>(m, HW, c, counter);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = start_value(v[j], c[j], seed, counter[j], k);
            }
            *reinterpret_cast<f32x4*>(x_adv + m) = v;
        }
    }
}

// MOVE == 0: the conditional copy alone (alpha255 == 0), x_adv is not written.
template <int L, int MOVE>
__global__ __launch_bounds__(kAdvThreads) void adv_step_kernel(
    const float* __restrict__ x, float* __restrict__ x_adv, const Strides xs,
    const float* __restrict__ g, const Strides gs, const int H, const int W, const long long total,
    const AdvChan k, const float* __restrict__ row_dir, const int* __restrict__ improved,
    float* __restrict__ best, const Strides bs) {
    const int HW = H * W;
    for (long long i = (long long)blockIdx.x * kAdvThreads + threadIdx.x; i < total;
         i += (long long)gridDim.x * kAdvThreads) {
        if constexpr (L == kStrided) {
            const Elem el(i, H, W);
            const long long o = el.at(xs);
            const float xa = x_adv[o];
            if (improved && improved[el.b] != 0) best[el.at(bs)] = xa;
            if constexpr (MOVE) {
                const float d = row_dir ? row_dir[el.b] : 1.0f;
                x_adv[o] = step_value(xa, x[o], g[el.at(gs)], el.c, d, k);
            }
        } else {
            const long long m = i * 4;
            int c[4];
            unsigned long long counter[4];
            const int b = decode4<L>(m, HW, c, counter);
            f32x4 xa = *reinterpret_cast<const f32x4*>(x_adv + m);
            if (improved && improved[b] != 0) *reinterpret_cast<f32x4*>(best + m) = xa;
            if constexpr (MOVE) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(x + m);
                const f32x4 gv = *reinterpret_cast<const f32x4*>(g + m);
                const float d = row_dir ? row_dir[b] : 1.0f;
#pragma unroll
                for (int j = 0; j < 4; ++j) xa[j] = step_value(xa[j], xv[j], gv[j], c[j], d, k);
                *reinterpret_cast<f32x4*>(x_adv + m) = xa;
            }
        }
    }
}

__global__ __launch_bounds__(kAdvThreads) void adv_direction_kernel(
    const float* __restrict__ controls, const float* __restrict__ pred_speed,
    const float* __restrict__ ref_controls, const float* __restrict__ ref_speed, const float w0,
    const float w1, const float w2, const float w3, const int B, const int first,
    float* __restrict__ dev, float* __restrict__ best_dev, float* __restrict__ row_dir,
    int* __restrict__ improved) {
    const int b = blockIdx.x * kAdvThreads + threadIdx.x;
    if (b >= B) return;
    const float* cb = controls + (size_t)b * 3;
    const float* rb = ref_controls + (size_t)b * 3;
    const float d = (w0 * (cb[0] - rb[0]) + w1 * (cb[1] - rb[1])) +
                    (w2 * (cb[2] - rb[2]) + w3 * (pred_speed[b] - ref_speed[b]));
    const bool finite = fabsf(d) <= 3.402823466e38f;      // false for NaN and +-inf
    dev[b] = d;
    row_dir[b] = (!finite || d >= 0.f) ? 1.0f : -1.0f;
    const bool imp = finite && (first || fabsf(d) > fabsf(best_dev[b]));
    improved[b] = imp ? 1 : 0;
    if (imp)
        best_dev[b] = d;
    else if (first)
        best_dev[b] = 0.f;      // nothing kept yet: any finite iterate that moves improves on it
}

__device__ __forceinline__ unsigned int quantize_one(const float xa, const int c) {
    float v = (xa * pick(c, kImageStd[0], kImageStd[1], kImageStd[2]) +
               pick(c, kImageMean[0], kImageMean[1], kImageMean[2])) * 255.0f;
    v = fminf(fmaxf(v, 0.f), 255.0f);      // NaN: 0
    return (unsigned int)rintf(v);
}

__device__ __forceinline__ int absdiff(const unsigned int q, const unsigned int f) {
    const int d = (int)q - (int)f;
    return d < 0 ? -d : d;
}

// One workgroup per frame.  Each thread walks its pixel groups, writes the bytes and keeps the
// largest |q - frame| it saw; the frame's maximum is wave shuffles, then the 16 wave values through
// LDS.  Integer maxima: the order cannot matter, and it is fixed anyway.
template <int L>
__global__ __launch_bounds__(kAdvQuantThreads) void adv_quantize_kernel(
    const float* __restrict__ x_adv, const Strides xs, const unsigned char* __restrict__ frames,
    const int H, const int W, unsigned char* __restrict__ out, int* __restrict__ linf) {
    __shared__ int red[kAdvQuantThreads / 64];
    const int b = blockIdx.x;
    const int HW = H * W;
    const size_t fbase = (size_t)b * HW * 3;
    int m = 0;
    if constexpr (L == kStrided) {
        const float* src = x_adv + (long long)b * xs.n;
        for (int p = threadIdx.x; p < HW; p += kAdvQuantThreads) {
            const int y = p / W, xw = p - y * W;
            const float* px = src + (long long)y * xs.h + (long long)xw * xs.w;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned int q = quantize_one(px[(long long)c * xs.c], c);
                out[fbase + (size_t)p * 3 + c] = (unsigned char)q;
                if (linf) m = max(m, absdiff(q, frames[fbase + (size_t)p * 3 + c]));
            }
        }
    } else if constexpr (L == kNCHW) {
        // four pixels: one 16-byte load per plane, 12 bytes of the frame as three words
        const float* src = x_adv + (size_t)b * 3 * HW;
        for (int p = threadIdx.x * 4; p < HW; p += kAdvQuantThreads * 4) {
            unsigned int q[12];      // HWC order: q[pixel * 3 + c]
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)c * HW + p);
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j * 3 + c] = quantize_one(v[j], c);
            }
            unsigned int* dst = reinterpret_cast<unsigned int*>(out + fbase + (size_t)p * 3);
            const unsigned int* fr =
                reinterpret_cast<const unsigned int*>(frames + fbase + (size_t)p * 3);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                dst[i] = q[i * 4] | (q[i * 4 + 1] << 8) | (q[i * 4 + 2] << 16) | (q[i * 4 + 3] << 24);
                if (linf) {
                    const unsigned int f = fr[i];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        m = max(m, absdiff(q[i * 4 + j], (f >> (8 * j)) & 0xFFu));
                }
            }
        }
    } else {
        // four floats of the interleaved row = four bytes of the frame
        const float* src = x_adv + fbase;
        for (int e = threadIdx.x * 4; e < 3 * HW; e += kAdvQuantThreads * 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + e);
            unsigned int word = 0;
            unsigned int q[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                q[j] = quantize_one(v[j], (e + j) % 3);
                word |= q[j] << (8 * j);
            }
            *reinterpret_cast<unsigned int*>(out + fbase + e) = word;
            if (linf) {
                const unsigned int f = *reinterpret_cast<const unsigned int*>(frames + fbase + e);
#pragma unroll
                for (int j = 0; j < 4; ++j) m = max(m, absdiff(q[j], (f >> (8 * j)) & 0xFFu));
            }
        }
    }
    if (!linf) return;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = red[0];
#pragma unroll
        for (int i = 1; i < kAdvQuantThreads / 64; ++i) t = max(t, red[i]);
        linf[b] = t;
    }
}

int adv_grid(long long total) {
    const long long cap = (long long)device_cus() * 8;
    const long long blocks = (total + kAdvThreads - 1) / kAdvThreads;
    return (int)(blocks < 1 ? 1 : blocks > cap ? cap : blocks);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the dense layout of a strided [B,3,H,W] tensor, or kStrided (a dimension of size 1 has no say)
int layout_of(const Strides& s, int B, int H, int W) {
    const long long HW = (long long)H * W;
    auto is = [](int size, long long stride, long long want) { return size == 1 || stride == want; };
    if (is(B, s.n, 3 * HW) && is(3, s.c, HW) && is(H, s.h, W) && is(W, s.w, 1)) return kNCHW;
    if (is(B, s.n, 3 * HW) && is(3, s.c, 1) && is(H, s.h, 3ll * W) && is(W, s.w, 3)) return kNHWC;
    return kStrided;
}

bool finite_nonneg(float v) { return v >= 0.f && v <= 3.402823466e38f; }

bool shape_ok(int B, int H, int W) {
    return B >= 1 && H >= 1 && W >= 1 && (long long)H * W <= kAdvMaxElems / 3 &&
           (long long)B <= kAdvMaxElems / (3ll * H * W);
}

bool nonneg(const Strides& s) { return s.n >= 0 && s.c >= 0 && s.h >= 0 && s.w >= 0; }

AdvChan chan_of(float eps255, float alpha255, const float* cs3, const float* range6) {
    AdvChan k{};
    k.e0 = eps255 * cs3[0], k.e1 = eps255 * cs3[1], k.e2 = eps255 * cs3[2];
    k.a0 = alpha255 * cs3[0], k.a1 = alpha255 * cs3[1], k.a2 = alpha255 * cs3[2];
    k.use_range = range6 != nullptr;
    if (range6) {
        k.lo0 = range6[0], k.hi0 = range6[1], k.lo1 = range6[2], k.hi1 = range6[3];
        k.lo2 = range6[4], k.hi2 = range6[5];
    }
    return k;
}

}  // namespace
}  // namespace cilrs

using namespace cilrs;

extern "C" {

long long cilrs_adv_max_elements(void) { return kAdvMaxElems; }
int cilrs_adv_quantize_threads(void) { return kAdvQuantThreads; }

int cilrs_adv_start(const float* x, long xn, long xc, long xh, long xw, int B, int H, int W,
                    float eps255, const float* chan_scale3, uint64_t seed, const float* range6,
                    float* x_adv, long an, long ac, long ah, long aw, void* stream) {
    CILRS_CHECK(x && x_adv && chan_scale3, "adv_start: NULL tensor");
    CILRS_CHECK(shape_ok(B, H, W), "adv_start: bad shape [%d,3,%d,%d] (B*3*H*W at most 2^30)", B,
                H, W);
    CILRS_CHECK(finite_nonneg(eps255), "adv_start: eps255 must be finite and >= 0");
    const Strides xs{xn, xc, xh, xw}, as{an, ac, ah, aw};
    CILRS_CHECK(nonneg(xs) && nonneg(as), "adv_start: negative stride");
    const AdvChan k = chan_of(eps255, 0.f, chan_scale3, range6);
    const int draw = eps255 > 0.f ? 1 : 0;
    const long long n = 3ll * B * H * W;
    const int lx = layout_of(xs, B, H, W);
    const bool wide = lx != kStrided && lx == layout_of(as, B, H, W) && ((long long)H * W) % 4 == 0 &&
                      aligned16(x) && aligned16(x_adv);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (wide && lx == kNCHW)
        adv_start_kernel<kNCHW><<<adv_grid(n / 4), kAdvThreads, 0, s>>>(x, xs, H, W, n / 4, draw, seed,
                                                                       k, x_adv, as);
    else if (wide)
        adv_start_kernel<kNHWC><<<adv_grid(n / 4), kAdvThreads, 0, s>>>(x, xs, H, W, n / 4, draw, seed,
                                                                       k, x_adv, as);
    else
        adv_start_kernel<kStrided><<<adv_grid(n), kAdvThreads, 0, s>>>(x, xs, H, W, n, draw, seed, k,
                                                                      x_adv, as);
    CILRS_LAUNCH_CHECK();
    return 0;
}

int cilrs_adv_step(const float* x, float* x_adv, long sn, long sc, long sh, long sw, const float* g,
                   long gn, long gc, long gh, long gw, int B, int H, int W, float alpha255,
                   float eps255, const float* chan_scale3, const float* row_dir,
                   const int32_t* improved, float* best, long bn, long bc, long bh, long bw,
                   const float* range6, void* stream) {
    CILRS_CHECK(x && x_adv && chan_scale3, "adv_step: NULL tensor");
    CILRS_CHECK(shape_ok(B, H, W), "adv_step: bad shape [%d,3,%d,%d] (B*3*H*W at most 2^30)", B,
                H, W);
    CILRS_CHECK(finite_nonneg(eps255), "adv_step: eps255 must be finite and >= 0");
    CILRS_CHECK(finite_nonneg(alpha255), "adv_step: alpha255 must be finite and >= 0");
    CILRS_CHECK(g || !(alpha255 > 0.f), "adv_step: the gradient may be NULL only when alpha255 = 0");
    const Strides xs{sn, sc, sh, sw}, gs{gn, gc, gh, gw}, bs{bn, bc, bh, bw};
    const bool copy = improved && best;
    CILRS_CHECK(nonneg(xs) && (!g || nonneg(gs)) && (!copy || nonneg(bs)),
                "adv_step: negative stride");
    const bool move = alpha255 > 0.f;
    if (!move && !copy) return 0;      // nothing to copy, nothing to move
    if (!copy) improved = nullptr;
    const AdvChan k = chan_of(eps255, alpha255, chan_scale3, range6);
    const long long n = 3ll * B * H * W;
    const int lx = layout_of(xs, B, H, W);
    const bool wide = lx != kStrided && ((long long)H * W) % 4 == 0 && aligned16(x) &&
                      aligned16(x_adv) &&
                      (!move || (lx == layout_of(gs, B, H, W) && aligned16(g))) &&
                      (!copy || (lx == layout_of(bs, B, H, W) && aligned16(best)));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define CILRS_ADV_STEP(L, MOVE, TOTAL)                                                          \
    adv_step_kernel<L, MOVE><<<adv_grid(TOTAL), kAdvThreads, 0, s>>>(x, x_adv, xs, g, gs, H, W, \
                                                                    TOTAL, k, row_dir, improved, \
                                                                    best, bs)
    if (wide && lx == kNCHW) {
        if (move) CILRS_ADV_STEP(kNCHW, 1, n / 4); else CILRS_ADV_STEP(kNCHW, 0, n / 4);
    } else if (wide) {
        if (move) CILRS_ADV_STEP(kNHWC, 1, n / 4); else CILRS_ADV_STEP(kNHWC, 0, n / 4);
    } else {
        if (move) CILRS_ADV_STEP(kStrided, 1, n); else CILRS_ADV_STEP(kStrided, 0, n);
    }
#undef CILRS_ADV_STEP
    CILRS_LAUNCH_CHECK();
    return 0;
}

int cilrs_adv_direction(const float* controls, const float* pred_speed, const float* ref_controls,
                        const float* ref_speed, const float* w4_host, int B, int first, float* dev,
                        float* best_dev, float* row_dir, int32_t* improved, void* stream) {
    CILRS_CHECK(controls && pred_speed && ref_controls && ref_speed && w4_host && dev && best_dev &&
                    row_dir && improved,
                "adv_direction: NULL tensor");
    CILRS_CHECK(B >= 1, "adv_direction: B = %d frames (at least 1)", B);
    adv_direction_kernel<<<(B + kAdvThreads - 1) / kAdvThreads, kAdvThreads, 0,
                           reinterpret_cast<hipStream_t>(stream)>>>(
        controls, pred_speed, ref_controls, ref_speed, w4_host[0], w4_host[1], w4_host[2], w4_host[3],
        B, first ? 1 : 0, dev, best_dev, row_dir, improved);
    CILRS_LAUNCH_CHECK();
    return 0;
}

int cilrs_adv_quantize(const float* x_adv, long sn, long sc, long sh, long sw,
                       const uint8_t* frames_u8, int B, int H, int W, uint8_t* out_u8, int32_t* linf,
                       void* stream) {
    CILRS_CHECK(x_adv && out_u8, "adv_quantize: NULL tensor");
    CILRS_CHECK(frames_u8 || !linf, "adv_quantize: linf needs the clean frames");
    CILRS_CHECK(shape_ok(B, H, W), "adv_quantize: bad shape [%d,3,%d,%d] (B*3*H*W at most 2^30)",
                B, H, W);
    const Strides xs{sn, sc, sh, sw};
    CILRS_CHECK(nonneg(xs), "adv_quantize: negative stride");
    const int lx = layout_of(xs, B, H, W);
    const bool wide = lx != kStrided && ((long long)H * W) % 4 == 0 && aligned16(x_adv) &&
                      (reinterpret_cast<uintptr_t>(out_u8) & 3) == 0 &&
                      (!linf || (reinterpret_cast<uintptr_t>(frames_u8) & 3) == 0);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (wide && lx == kNCHW)
        adv_quantize_kernel<kNCHW><<<B, kAdvQuantThreads, 0, s>>>(x_adv, xs, frames_u8, H, W, out_u8,
                                                                 linf);
    else if (wide)
        adv_quantize_kernel<kNHWC><<<B, kAdvQuantThreads, 0, s>>>(x_adv, xs, frames_u8, H, W, out_u8,
                                                                 linf);
    else
        adv_quantize_kernel<kStrided><<<B, kAdvQuantThreads, 0, s>>>(x_adv, xs, frames_u8, H, W,
                                                                    out_u8, linf);
    CILRS_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
