// SmoothGrad and integrated gradients around the saliency pass (Predictor.attribution): the three
// streaming kernels that keep the S samples of a call on the device.
//
//   cilrs_attr_samples     uint8 frames -> the network inputs of samples [s_begin, s_begin + s_count)
//                          of every frame: noisy copies (SmoothGrad) or points on the straight path
//                          from a baseline frame (integrated gradients, midpoint rule)
//   cilrs_attr_accumulate  acc[b] (+)= the image gradients of frame b's samples, in sample order
//   cilrs_attr_finalize    mean gradient (SmoothGrad) or mean gradient x (x - baseline) (integrated
//                          gradients), its sum over the colour channels and over the frame
//
// The gradients in between are cilrs_net_forward_frozen + cilrs_net_backward_data +
// cilrs_net_input_grads on the batch of samples.  The reference has no counterpart: it never
// differentiates with respect to the camera frame (model/autonomous_drive.py:908-920).
//
// Every float operation is rounded once, in the order written, so the results are the torch fp32
// expressions bit for bit.  hipcc contracts a * b + c to an FMA by default, and the __fmul_rn /
// __fadd_rn intrinsics do not prevent that: they are inline functions of a header compiled with
// contraction on, so their operations still fuse (c0 + alpha * (c - c0) did, measured against the
// torch expression).  Hence plain operators under `#pragma clang fp contract(off)`, as in
// augment.hip: the pragma covers what is written in this file.  No atomics, every sum in a fixed
// order.  Where the frame size allows (H * W a multiple of 4, 16-byte aligned tensors) a thread
// moves four pixels: 12 bytes of a frame as three words, one 16-byte access per plane.
#include "common.h"

namespace cilrs {
namespace {

#pragma clang fp contract(off)      // keep a * b + c as two roundings: torch-identical arithmetic

constexpr int kAttrThreads = 256;      // samples, accumulate: grid-stride streaming
constexpr int kAttrFinThreads = 1024;   // finalize: one workgroup per frame (as saliency_map_kernel)

struct AttrNorm {
    float m[3], d[3];
};
constexpr AttrNorm kAttrNorm = {{kImageMean[0], kImageMean[1], kImageMean[2]},
                                {kImageStd[0], kImageStd[1], kImageStd[2]}};

// the Box-Muller normal of augment.hip's GaussNoise for element `counter` of stream `seed`
__device__ __forceinline__ float hash_normal(const unsigned long long seed,
                                             const unsigned long long counter) {
    const unsigned long long hsh = splitmix64(seed + counter * 0xD1B54A32D192ED03ull);
    const float u1 = ((float)(unsigned int)(hsh >> 40) + 1.0f) * (1.0f / 16777216.0f);
    const float u2 = (float)(unsigned int)((hsh >> 8) & 0xFFFFFFu) * (1.0f / 16777216.0f);
    const float rad = sqrtf(-2.0f * logf(u1));
    return rad * cosf(6.2831853071795864f * u2);
}

// V pixels (3 V bytes, HWC) starting at p; V == 4: p is 4-byte aligned
template <int V>
__device__ __forceinline__ void load_pixels(const unsigned char* __restrict__ p, float c[3 * V]) {
    if constexpr (V == 4) {
        const unsigned int* w = reinterpret_cast<const unsigned int*>(p);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const unsigned int v = w[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) c[i * 4 + j] = (float)((v >> (8 * j)) & 0xFFu);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3 * V; ++i) c[i] = (float)p[i];
    }
}

template <int V>
__device__ __forceinline__ void load_plane(const float* __restrict__ p, float v[V]) {
    if constexpr (V == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = t[q];
    } else {
        v[0] = p[0];
    }
}

template <int V>
__device__ __forceinline__ void store_plane(float* __restrict__ p, const float v[V]) {
    if constexpr (V == 4) {
        f32x4 t;
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = v[q];
        *reinterpret_cast<f32x4*>(p) = t;
    } else {
        p[0] = v[0];
    }
}

// One thread = V adjacent pixels of one output row r = b * s_count + j (sample s_begin + j of
// frame b); `groups` = H * W / V pixel groups per row, `total` = rows * groups.
template <int V>
__global__ __launch_bounds__(kAttrThreads) void attr_samples_kernel(
    const unsigned char* __restrict__ frames, const unsigned char* __restrict__ baseline,
    const int HW, const long long groups, const long long total, const int mode, const int S,
    const int s_begin, const int s_count, const float sigma255, const unsigned long long seed,
    float* __restrict__ out, const AttrNorm nc) {
    for (long long i = (long long)blockIdx.x * kAttrThreads + threadIdx.x; i < total;
         i += (long long)gridDim.x * kAttrThreads) {
        const long long r = i / groups;
        const int p = (int)(i - r * groups) * V;
        const int b = (int)(r / s_count);
        const int s = s_begin + (int)(r - (long long)b * s_count);
        const size_t src = ((size_t)b * HW + p) * 3;
        float c[3 * V];
        load_pixels<V>(frames + src, c);
        if (mode == CILRS_ATTR_INTEGRATED) {
            const float alpha = ((float)s + 0.5f) / (float)S;
            float c0[3 * V];
            if (baseline) {
                load_pixels<V>(baseline + src, c0);
            } else {
#pragma unroll
                for (int e = 0; e < 3 * V; ++e) c0[e] = 0.f;
            }
#pragma unroll
            for (int e = 0; e < 3 * V; ++e)
                c[e] = c0[e] + alpha * (c[e] - c0[e]);
        } else {
            // keyed on the GLOBAL sample index: the same sample whichever chunk produces it
            const unsigned long long base =
                ((unsigned long long)b * (unsigned long long)S + (unsigned long long)s) * 3ull *
                    (unsigned long long)HW + (unsigned long long)p * 3ull;
#pragma unroll
            for (int e = 0; e < 3 * V; ++e)
                c[e] = c[e] + sigma255 * hash_normal(seed, base + e);
        }
        float* dst = out + (size_t)r * 3 * HW + p;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float v[V];
#pragma unroll
            for (int q = 0; q < V; ++q)      // /255, Normalize: augment.hip's operation order
                v[q] = (c[q * 3 + k] / 255.0f - nc.m[k]) / nc.d[k];
            store_plane<V>(dst + (size_t)k * HW, v);
        }
    }
}

// One thread = V adjacent elements (along w) of acc; the chain over the frame's samples is
// sequential, so any split of the samples into chunks gives the same bits.
template <int V>
__global__ __launch_bounds__(kAttrThreads) void attr_accumulate_kernel(
    const float* __restrict__ dimage, const long sn, const long sc, const long sh, const long sw,
    const int s_count, const int H, const int W, const long long total, const int first,
    float* __restrict__ acc) {
    const int WV = W / V;
    for (long long i = (long long)blockIdx.x * kAttrThreads + threadIdx.x; i < total;
         i += (long long)gridDim.x * kAttrThreads) {
        const int wq = (int)(i % WV);
        long long t = i / WV;
        const int h = (int)(t % H);
        t /= H;
        const int c = (int)(t % 3);
        const long long b = t / 3;
        float* dst = acc + (((size_t)b * 3 + c) * H + h) * W + (size_t)wq * V;
        const float* src = dimage + (size_t)b * s_count * sn + (size_t)c * sc + (size_t)h * sh +
                           (size_t)wq * V * sw;
        float a[V];
        if (first) {
#pragma unroll
            for (int q = 0; q < V; ++q) a[q] = 0.f;
        } else {
            load_plane<V>(dst, a);
        }
        for (int j = 0; j < s_count; ++j) {
            float g[V];
            load_plane<V>(src + (size_t)j * sn, g);      // (V == 4 only with sw == 1)
#pragma unroll
            for (int q = 0; q < V; ++q) a[q] = a[q] + g[q];
        }
        store_plane<V>(dst, a);
    }
}

// One workgroup per frame.  Each thread walks its pixel groups, writes attr / signed_map and keeps
// a running sum of the signed values; the frame's total is that chain, then wave shuffles, then
// the 16 wave sums through LDS in index order.
template <int V>
__global__ __launch_bounds__(kAttrFinThreads) void attr_finalize_kernel(
    const float* __restrict__ acc, const unsigned char* __restrict__ frames,
    const unsigned char* __restrict__ baseline, const int HW, const int mode, const float invS,
    const float k0, const float k1, const float k2, float* __restrict__ attr,
    float* __restrict__ signed_map, float* __restrict__ total) {
    __shared__ float red[kAttrFinThreads / 64];
    const int b = blockIdx.x;
    const float* a = acc + (size_t)b * 3 * HW;
    float* o = attr + (size_t)b * 3 * HW;
    const float ks[3] = {k0, k1, k2};
    float sum = 0.f;
    for (int p = threadIdx.x * V; p < HW; p += kAttrFinThreads * V) {
        float f[3][V];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            load_plane<V>(a + (size_t)k * HW + p, f[k]);
#pragma unroll
            for (int q = 0; q < V; ++q) f[k][q] = f[k][q] * invS;
        }
        if (mode == CILRS_ATTR_INTEGRATED) {
            const size_t src = ((size_t)b * HW + p) * 3;
            float c[3 * V], c0[3 * V];
            load_pixels<V>(frames + src, c);
            if (baseline) {
                load_pixels<V>(baseline + src, c0);
            } else {
#pragma unroll
                for (int e = 0; e < 3 * V; ++e) c0[e] = 0.f;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int q = 0; q < V; ++q)      // 8-bit values: the float difference is the integer one
                    f[k][q] = f[k][q] * ((c[q * 3 + k] - c0[q * 3 + k]) * ks[k]);
        }
        float sg[V];
#pragma unroll
        for (int q = 0; q < V; ++q) {
            sg[q] = (f[0][q] + f[1][q]) + f[2][q];
            sum = sum + sg[q];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) store_plane<V>(o + (size_t)k * HW + p, f[k]);
        if (signed_map) store_plane<V>(signed_map + (size_t)b * HW + p, sg);
    }
    if (!total) return;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum = sum + __shfl_xor(sum, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = red[0];
#pragma unroll
        for (int i = 1; i < kAttrFinThreads / 64; ++i) t = t + red[i];
        total[b] = t;
    }
}

int attr_grid(long long total) {
    const long long cap = (long long)device_cus() * 8;
    const long long blocks = (total + kAttrThreads - 1) / kAttrThreads;
    return (int)(blocks < 1 ? 1 : blocks > cap ? cap : blocks);
}

bool aligned_to(const void* p, size_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

bool attr_mode_ok(int mode) { return mode == CILRS_ATTR_SMOOTHGRAD || mode == CILRS_ATTR_INTEGRATED; }

}  // namespace

int attr_finalize_threads() { return kAttrFinThreads; }

int launch_attr_samples(const unsigned char* frames, const unsigned char* baseline, int B, int H,
                        int W, int mode, int S, int s_begin, int s_count, float sigma255,
                        unsigned long long seed, float* out, hipStream_t s) {
    CILRS_CHECK(frames && out, "attr_samples: NULL tensor");
    CILRS_CHECK(attr_mode_ok(mode), "attr_samples: unknown mode %d", mode);
    CILRS_CHECK(B >= 1 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31) / 3,
                "attr_samples: bad shape [%d,%d,%d,3]", B, H, W);
    CILRS_CHECK(S >= 1, "attr_samples: S = %d samples (at least 1)", S);
    CILRS_CHECK(s_begin >= 0 && s_count >= 1 && (long long)s_begin + s_count <= S,
                "attr_samples: chunk [%d, %lld) outside [0, %d)", s_begin,
                (long long)s_begin + s_count, S);
    CILRS_CHECK(sigma255 >= 0.f && sigma255 <= 3.402823466e38f,
                "attr_samples: sigma255 must be finite and >= 0");
    // the noise counter (b * S + s) * 3HW + element stays below 2^63
    const long long per = 3ll * H * W;
    CILRS_CHECK((unsigned __int128)per * (unsigned)B * (unsigned)S < ((unsigned __int128)1 << 63),
                "attr_samples: 3*H*W*B*S = 3*%d*%d*%d*%d reaches 2^63", H, W, B, S);
    CILRS_CHECK((long long)B * s_count <= (1ll << 40) / per,
                "attr_samples: a chunk of %d x %d samples is too large", B, s_count);
    const int HW = H * W;
    const long long rows = (long long)B * s_count;
    const bool vec = HW % 4 == 0 && aligned_to(frames, 4) && aligned_to(out, 16) &&
                     (!baseline || aligned_to(baseline, 4));
    if (vec) {
        const long long groups = HW / 4, total = rows * groups;
        attr_samples_kernel<4><<<attr_grid(total), kAttrThreads, 0, s>>>(
            frames, baseline, HW, groups, total, mode, S, s_begin, s_count, sigma255, seed, out,
            kAttrNorm);
    } else {
        const long long groups = HW, total = rows * groups;
        attr_samples_kernel<1><<<attr_grid(total), kAttrThreads, 0, s>>>(
            frames, baseline, HW, groups, total, mode, S, s_begin, s_count, sigma255, seed, out,
            kAttrNorm);
    }
    CILRS_LAUNCH_CHECK();
    return 0;
}

int launch_attr_accumulate(const float* dimage, long sn, long sc, long sh, long sw, int B,
                           int s_count, int H, int W, int first, float* acc, hipStream_t s) {
    CILRS_CHECK(dimage && acc, "attr_accumulate: NULL tensor");
    CILRS_CHECK(B >= 1 && s_count >= 1 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31) / 3 &&
                    (long long)B * s_count <= (1ll << 40) / (3ll * H * W),
                "attr_accumulate: bad shape [%d*%d,3,%d,%d]", B, s_count, H, W);
    CILRS_CHECK(sn >= 0 && sc >= 0 && sh >= 0 && sw >= 0, "attr_accumulate: negative stride");
    const bool vec = sw == 1 && W % 4 == 0 && sn % 4 == 0 && sc % 4 == 0 && sh % 4 == 0 &&
                     aligned_to(dimage, 16) && aligned_to(acc, 16);
    if (vec) {
        const long long total = (long long)B * 3 * H * (W / 4);
        attr_accumulate_kernel<4><<<attr_grid(total), kAttrThreads, 0, s>>>(
            dimage, sn, sc, sh, sw, s_count, H, W, total, first, acc);
    } else {
        const long long total = (long long)B * 3 * H * W;
        attr_accumulate_kernel<1><<<attr_grid(total), kAttrThreads, 0, s>>>(
            dimage, sn, sc, sh, sw, s_count, H, W, total, first, acc);
    }
    CILRS_LAUNCH_CHECK();
    return 0;
}

int launch_attr_finalize(const float* acc, const unsigned char* frames, const unsigned char* baseline,
                         int B, int H, int W, int mode, int S, const float* chan_scale3, float* attr,
                         float* signed_map, float* total, hipStream_t s) {
    CILRS_CHECK(acc && attr, "attr_finalize: NULL tensor");
    CILRS_CHECK(attr_mode_ok(mode), "attr_finalize: unknown mode %d", mode);
    CILRS_CHECK(mode != CILRS_ATTR_INTEGRATED || (frames && chan_scale3),
                "attr_finalize: integrated gradients need the frames and chan_scale3");
    CILRS_CHECK(B >= 1 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31) / 3,
                "attr_finalize: bad shape [%d,3,%d,%d]", B, H, W);
    CILRS_CHECK(S >= 1, "attr_finalize: S = %d samples (at least 1)", S);
    const int HW = H * W;
    const bool ig = mode == CILRS_ATTR_INTEGRATED;
    const float invS = 1.f / (float)S;           // host division: IEEE, correctly rounded
    const float k0 = ig ? chan_scale3[0] : 1.f, k1 = ig ? chan_scale3[1] : 1.f,
                k2 = ig ? chan_scale3[2] : 1.f;
    const bool vec = HW % 4 == 0 && aligned_to(acc, 16) && aligned_to(attr, 16) &&
                     (!signed_map || aligned_to(signed_map, 16)) &&
                     (!ig || (aligned_to(frames, 4) && (!baseline || aligned_to(baseline, 4))));
    if (vec)
        attr_finalize_kernel<4><<<B, kAttrFinThreads, 0, s>>>(acc, frames, baseline, HW, mode, invS,
                                                             k0, k1, k2, attr, signed_map, total);
    else
        attr_finalize_kernel<1><<<B, kAttrFinThreads, 0, s>>>(acc, frames, baseline, HW, mode, invS,
                                                             k0, k1, k2, attr, signed_map, total);
    CILRS_LAUNCH_CHECK();
    return 0;
}

}  // namespace cilrs
