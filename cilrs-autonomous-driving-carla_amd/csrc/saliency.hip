// Saliency heat map of one batch of image gradients: "which pixels moved this output".
//
// The forward it differentiates is the agent's per-tick call `controls, pred_speed =
// self.model(img_t, speed_t, cmd_t)` (predict_controls, model/autonomous_drive.py:908-920); the
// gradient d(w . outputs) / d image comes from cilrs_net_backward_data + cilrs_net_input_grads.
// The reference has no counterpart: it never differentiates with respect to the camera frame.
//
//   s[b,h,w]  = max_c |dimage[b,c,h,w]| * chan_scale[c]     (chan_scale: 1, or per 8-bit level)
//   peak[b]   = max_hw s[b,h,w]
//   heat      = s / peak          (0 where peak == 0: an all-zero gradient gives an all-zero map)
//   heat_u8   = floor(heat * 255 + 0.5)
//
// One launch, one 1,024-thread workgroup per frame, two sweeps: the first writes s into `heat` and
// keeps each thread's maximum, a fixed-order reduction (wave shuffles, then 16 values through LDS)
// gives the frame's peak, the second sweep divides what the same thread wrote.  No atomics: the
// result is bit-identical from run to run.  Any element strides (NCHW or channels-last gradients).
#include "common.h"

namespace cilrs {
namespace {

constexpr int kSalThreads = 1024;

__global__ __launch_bounds__(kSalThreads) void saliency_map_kernel(
    const float* __restrict__ dimage, const long sn, const long sc, const long sh, const long sw,
    const int H, const int W, const float c0, const float c1, const float c2,
    float* __restrict__ heat, unsigned char* __restrict__ heat_u8, float* __restrict__ peak) {
    __shared__ float red[kSalThreads / 64];
    const int b = blockIdx.x;
    const int HW = H * W;
    const float* src = dimage + (size_t)b * sn;
    float* out = heat + (size_t)b * HW;
    float m = 0.f;
    for (int p = threadIdx.x; p < HW; p += kSalThreads) {
        const int h = p / W, w = p - h * W;
        const float* px = src + (long)h * sh + (long)w * sw;
        const float v0 = __fmul_rn(fabsf(px[0]), c0);
        const float v1 = __fmul_rn(fabsf(px[sc]), c1);
        const float v2 = __fmul_rn(fabsf(px[2 * sc]), c2);
        const float s = fmaxf(fmaxf(v0, v1), v2);
        out[p] = s;
        m = fmaxf(m, s);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    float pk = red[0];
#pragma unroll
    for (int i = 1; i < kSalThreads / 64; ++i) pk = fmaxf(pk, red[i]);
    if (threadIdx.x == 0 && peak) peak[b] = pk;
    for (int p = threadIdx.x; p < HW; p += kSalThreads) {
        // (this thread wrote out[p] in the first sweep)
        const float hv = pk > 0.f ? __fdiv_rn(out[p], pk) : 0.f;
        out[p] = hv;
        if (heat_u8)
            heat_u8[(size_t)b * HW + p] =
                (unsigned char)floorf(__fadd_rn(__fmul_rn(hv, 255.f), 0.5f));
    }
}

}  // namespace

int launch_saliency_map(const float* dimage, long sn, long sc, long sh, long sw, int B, int H, int W,
                        const float* chan_scale3, float* heat, unsigned char* heat_u8, float* peak,
                        hipStream_t s) {
    CILRS_CHECK(dimage && heat, "saliency_map: NULL tensor");
    CILRS_CHECK(B >= 1 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31),
                "saliency_map: bad shape [%d,3,%d,%d]", B, H, W);
    CILRS_CHECK(sn >= 0 && sc >= 0 && sh >= 0 && sw >= 0, "saliency_map: negative stride");
    const float c0 = chan_scale3 ? chan_scale3[0] : 1.f, c1 = chan_scale3 ? chan_scale3[1] : 1.f,
                c2 = chan_scale3 ? chan_scale3[2] : 1.f;
    saliency_map_kernel<<<B, kSalThreads, 0, s>>>(dimage, sn, sc, sh, sw, H, W, c0, c1, c2, heat,
                                                 heat_u8, peak);
    CILRS_LAUNCH_CHECK();
    return 0;
}

}  // namespace cilrs
