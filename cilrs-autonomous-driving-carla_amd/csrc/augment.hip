// Training input pipeline on the device: the reference's albumentations Compose
// (notebook/notebook.ipynb:387-394) + ToTensor/Normalize (:412-414) as ONE kernel over the uint8
// batch.  The reference runs these on two CPU DataLoader workers per frame; here the per-sample
// random parameters are drawn on the host (cilrs_mi355/data.py) and every pixel is one thread.
//
//   RandomBrightnessContrast -> HueSaturationValue -> GaussianBlur -> GaussNoise -> CoarseDropout
//
// albumentations and cv2 are absent from the build image, so each step restates the libraries'
// published behaviour (PARITY UNPINNED against them); the arithmetic below is mirrored operation
// by operation by oracle/augment_oracle.py, which the tests compare against.
//
// Two edges are part of the contract.  The shifted hue lies in [0, 179]: it is the LUT
// trunc(mod(arange(180) + hue, 180)) to within one step (float32 rounds H + hue once), and a
// wrap that rounds up to 180 is folded to 0, never decoded as a seventh sector.  The blur's border
// is reflect-101 with period 2(n - 1) at every n >= 2, so a dimension of two pixels under five
// taps reads indices -2, -1, 2, 3 as 0, 1, 0, 1 (np.pad "reflect", scipy "mirror") and no tap
// leaves the sample's frame.
//
// Weather (cilrs_weather_params: tone, fog, rain) is a second, optional source stage in front of
// those five: a pure function of the uint8 source pixel, its position and the sample's record,
// applied wherever a source pixel is read -- the blur's taps included -- so the `_weather`
// kernels give what the plain ones give on frames that were put through the weather first and
// stored as uint8.  It is the <true> instantiation of the same pixel function; the plain entry
// points keep the <false> one.  No transcendental runs here: what needs exp() is folded into the
// record on the host (cilrs_mi355/data.py), and tests/_weather.py mirrors the arithmetic.
//
// The viewpoint (cilrs_view_params: two inverse homographies split at a row) is a third, optional
// source stage in front of the weather: wherever a source pixel (y, x) is read, the `_view`
// kernels read the virtual frame V(y, x) instead, four stored pixels blended bilinearly and
// rounded to a grey level, so they give what the others give on frames that were warped first
// and stored as uint8.  It is the VW flag of the same pixel function, instantiated only for the
// `_view` entry points; tests/_view.py mirrors the arithmetic.
#include "common.h"

namespace cilrs {
namespace {

#pragma clang fp contract(off)      // keep a*b+c as two roundings: numpy-identical arithmetic

__device__ __forceinline__ float clip255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }

// stages 1-2 for one pixel: brightness/contrast LUT, then the HSV shifts, in place on the
// uint8-valued floats c[3].
__device__ __forceinline__ void colour_stages(const cilrs_aug_params& a, float c[3]) {
    if (a.rbc_on) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float t = c[k] * a.alpha;
            t = t + a.beta255;
            c[k] = truncf(clip255(t));           // LUT built in float32, clip, astype(uint8)
        }
    }
    if (a.hsv_on) {
        const float r = c[0], g = c[1], b = c[2];
        const float v = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
        const float d = v - mn;
        float s = 0.f, h = 0.f;
        if (v > 0.f) s = d * 255.f / v;
        if (d > 0.f) {
            if (v == r) h = 60.f * (g - b) / d;
            else if (v == g) h = 120.f + 60.f * (b - r) / d;
            else h = 240.f + 60.f * (r - g) / d;
            if (h < 0.f) h = h + 360.f;
        }
        // 8-bit HSV as OpenCV stores it: H in half-degrees [0,180), S, V in [0,255]
        float H = rintf(h * 0.5f);
        if (H >= 180.f) H = H - 180.f;
        const float S = rintf(s), V = v;
        // the three LUTs (hue wraps mod 180, sat / val clip), truncated to uint8
        float H2 = fmodf(H + a.hue, 180.f);
        if (H2 < 0.f) H2 = H2 + 180.f;
        if (H2 >= 180.f) H2 = 0.f;               // a tiny negative H2 + 180 rounds to 180: wrap it
        H2 = truncf(H2);
        const float S2 = truncf(clip255(S + a.sat));
        const float V2 = truncf(clip255(V + a.val));
        // HSV -> RGB
        const float hh = H2 * 2.f / 60.f;        // sector coordinate in [0,6)
        const float sec = floorf(hh);
        const float f = hh - sec;
        const float sn = S2 / 255.f;
        const float pp = V2 * (1.f - sn);
        const float qq = V2 * (1.f - sn * f);
        const float tt = V2 * (1.f - sn * (1.f - f));
        const int isec = (int)sec;
        float R, G, B;
        switch (isec) {
            case 0: R = V2; G = tt; B = pp; break;
            case 1: R = qq; G = V2; B = pp; break;
            case 2: R = pp; G = V2; B = tt; break;
            case 3: R = pp; G = qq; B = V2; break;
            case 4: R = tt; G = pp; B = V2; break;
            default: R = V2; G = pp; B = qq; break;
        }
        c[0] = rintf(clip255(R));
        c[1] = rintf(clip255(G));
        c[2] = rintf(clip255(B));
    }
}

// blur_w[|d|] as a select among the three weights read beforehand: an index into the record
// computed at run time would put the whole record into scratch memory
__device__ __forceinline__ float blur_tap(const float w0, const float w1, const float w2,
                                          const int d) {
    const int ad = d < 0 ? -d : d;
    return ad == 0 ? w0 : (ad == 1 ? w1 : w2);
}

// reflect-101 index of i in [-2, n + 1] for any n >= 2: period 2(n - 1), as np.pad "reflect".  The
// second fold leaves [0, n) only when n == 2 (i == 3 -> -1 -> 1); for n >= 3 the last line never
// fires.
__device__ __forceinline__ int reflect101(int i, const int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    if (i < 0) i = -i;
    return i;
}

// Weather for source pixel (y, x), in place on the uint8-valued floats c[3]: tone, fog, rain.
__device__ __forceinline__ void weather_stages(const cilrs_weather_params& w, const int y,
                                               const int x, float c[3]) {
    if (w.tone_on) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float t = c[k] * w.gain[k];
            t = t + w.lift255[k];
            c[k] = truncf(clip255(t));
        }
    }
    if (w.fog_on) {
        // flat-ground pseudo-depth from the row alone, d in (0, 1]; transmission linear in d
        const float yf = (float)y;
        float d = 1.f;
        if (yf > w.fog_horizon) d = w.fog_near / fmaxf(yf - w.fog_horizon, w.fog_near);
        float t = w.fog_t1 * d;
        t = w.fog_t0 + t;
        t = fminf(fmaxf(t, 0.f), 1.f);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float u = c[k] - w.fog_rgb255[k];
            u = u * t;
            u = w.fog_rgb255[k] + u;
            c[k] = rintf(clip255(u));
        }
    }
    const int L = min(w.rain_len, 16);
    if (L > 0) {
        // tail position j of a streak covers (y, x) when (y - j, x - floor(j * slant / 16)) is a
        // head; the smallest covering j gives the largest alpha.  L is uniform over the sample, so
        // the loop runs to its end on every lane and the first hit is selected, not branched on.
        int jmin = L;
        for (int j = L - 1; j >= 0; --j) {
            const int hy = y - j, hx = x - ((j * w.rain_slant_q4) >> 4);
            const unsigned long long e =
                (unsigned long long)(hy + 64) * 65536ull + (unsigned long long)(hx + 64);
            const unsigned long long hsh = splitmix64(w.rain_seed + e * 0xD1B54A32D192ED03ull);
            jmin = ((unsigned int)(hsh >> 40) < w.rain_thresh24) ? j : jmin;
        }
        if (jmin < L) {
            float a = (float)(L - jmin) / (float)L;
            a = w.rain_alpha * a;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float u = w.rain_v255 - c[k];
                u = a * u;
                u = c[k] + u;
                c[k] = rintf(clip255(u));
            }
        }
    }
}

// Pixel (y, x) of the virtual frame of one sample: destination -> source through the record's far
// or ground map, clamped into the frame (replicate border; the nesting sends a NaN to 0, so no
// address outside the frame is formed whatever the record holds), bilinear, rounded to a grey
// level.  The map is selected element by element and the record indexed with constants only.
__device__ __forceinline__ void view_pixel(const unsigned char* __restrict__ img,
                                           const cilrs_view_params& v, const int y, const int x,
                                           const int H, const int W, float c[3]) {
    const float xf = (float)x, yf = (float)y;
    const bool g = yf > v.split_row;
    const float m0 = g ? v.ground[0] : v.far[0], m1 = g ? v.ground[1] : v.far[1];
    const float m2 = g ? v.ground[2] : v.far[2], m3 = g ? v.ground[3] : v.far[3];
    const float m4 = g ? v.ground[4] : v.far[4], m5 = g ? v.ground[5] : v.far[5];
    const float m6 = g ? v.ground[6] : v.far[6], m7 = g ? v.ground[7] : v.far[7];
    const float m8 = g ? v.ground[8] : v.far[8];
    const float u = (m0 * xf + m1 * yf) + m2;
    const float t = (m3 * xf + m4 * yf) + m5;
    const float w = (m6 * xf + m7 * yf) + m8;
    const float sx = fminf(fmaxf(u / w, 0.f), (float)(W - 1));
    const float sy = fminf(fmaxf(t / w, 0.f), (float)(H - 1));
    const int x0 = (int)floorf(sx), y0 = (int)floorf(sy);
    const float ax = sx - (float)x0, ay = sy - (float)y0;
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const unsigned char* r0 = img + (size_t)y0 * W * 3;
    const unsigned char* r1 = img + (size_t)y1 * W * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float p00 = (float)r0[x0 * 3 + k], p01 = (float)r0[x1 * 3 + k];
        const float p10 = (float)r1[x0 * 3 + k], p11 = (float)r1[x1 * 3 + k];
        const float top = p00 + ax * (p01 - p00);
        const float bot = p10 + ax * (p11 - p10);
        c[k] = rintf(clip255(top + ay * (bot - top)));
    }
}

// Source pixel (y, x) of one sample as uint8-valued floats: the stored bytes, or with VW and the
// record on the virtual frame's pixel, behind the sample's weather when WX.  `w` / `v` are not
// read otherwise.
template <bool WX, bool VW>
__device__ __forceinline__ void source_pixel(const unsigned char* __restrict__ img,
                                             const cilrs_weather_params& w,
                                             const cilrs_view_params& v, const int y,
                                             const int x, const int H, const int W, float c[3]) {
    bool stored = true;
    if constexpr (VW) stored = v.on == 0;
    if (stored) {
        const unsigned char* p = img + ((size_t)y * W + x) * 3;
        c[0] = (float)p[0]; c[1] = (float)p[1]; c[2] = (float)p[2];
    } else {
        view_pixel(img, v, y, x, H, W, c);
    }
    if constexpr (WX) weather_stages(w, y, x, c);
}

// Mean / std of the final Normalize, passed by value to the kernels.
struct NormConsts {
    float m0, m1, m2, d0, d1, d2;
};

// Every stage for output pixel (y, x) of one sample: `img` is that sample's uint8 [H][W][3] source
// frame, `i` the pixel's index in the output batch.  The kernels below are this function behind
// two ways of finding `img`, so their results are the same element for element; WX puts the
// sample's weather `wx` in front of every source pixel read, VW its viewpoint `vw` in front of
// that.
template <bool WX, bool VW>
__device__ __forceinline__ void augment_pixel(const unsigned char* __restrict__ img,
                                              const cilrs_aug_params& a,
                                              const cilrs_weather_params& wx,
                                              const cilrs_view_params& vw, const int y,
                                              const int x,
                                              const int H, const int W, const size_t i,
                                              float* __restrict__ out_f32,
                                              unsigned char* __restrict__ out_u8,
                                              const NormConsts& nc) {
    float c[3];
    if (a.blur_k > 1) {
        // separable Gaussian written as one fixed-order 2-D sum over the colour-adjusted taps
        // (cv2.GaussianBlur semantics: reflect-101 border)
        const int r = min(a.blur_k >> 1, 2);
        const float w0 = a.blur_w[0], w1 = a.blur_w[1], w2 = a.blur_w[2];
        float acc[3] = {0.f, 0.f, 0.f};
        for (int dy = -r; dy <= r; ++dy) {
            const int yy = reflect101(y + dy, H);
            float row[3] = {0.f, 0.f, 0.f};
            for (int dx = -r; dx <= r; ++dx) {
                const int xx = reflect101(x + dx, W);
                float t[3];
                source_pixel<WX, VW>(img, wx, vw, yy, xx, H, W, t);
                colour_stages(a, t);
                const float w = blur_tap(w0, w1, w2, dx);
#pragma unroll
                for (int k = 0; k < 3; ++k) row[k] = row[k] + w * t[k];
            }
            const float w = blur_tap(w0, w1, w2, dy);
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k] = acc[k] + w * row[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = rintf(clip255(acc[k]));
    } else {
        source_pixel<WX, VW>(img, wx, vw, y, x, H, W, c);
        colour_stages(a, c);
    }
    if (a.noise_std255 > 0.f) {
        // per-channel Gaussian noise: Box-Muller on a counter-based hash of (seed, element)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned long long e = ((unsigned long long)(y * W + x)) * 3ull + k;
            const unsigned long long hsh = splitmix64(a.noise_seed + e * 0xD1B54A32D192ED03ull);
            const float u1 = ((float)(unsigned int)(hsh >> 40) + 1.0f) * (1.0f / 16777216.0f);
            const float u2 = (float)(unsigned int)((hsh >> 8) & 0xFFFFFFu) * (1.0f / 16777216.0f);
            const float rad = sqrtf(-2.0f * logf(u1));
            const float n = rad * cosf(6.2831853071795864f * u2);
            c[k] = rintf(clip255(c[k] + n * a.noise_std255));
        }
    }
#pragma unroll
    for (int hI = 0; hI < 3; ++hI)               // unrolled: constant indices into the record
        if (hI < a.nholes && y >= a.hole_y0[hI] && y < a.hole_y1[hI] && x >= a.hole_x0[hI] &&
            x < a.hole_x1[hI])
            c[0] = c[1] = c[2] = 0.f;            // CoarseDropout fill = 0
    if (out_u8) {
        unsigned char* o = out_u8 + i * 3;
        o[0] = (unsigned char)c[0]; o[1] = (unsigned char)c[1]; o[2] = (unsigned char)c[2];
    }
    if (out_f32) {
        float* o = out_f32 + i * 3;              // /255, Normalize (notebook.ipynb:412-414)
        o[0] = (c[0] / 255.0f - nc.m0) / nc.d0;
        o[1] = (c[1] / 255.0f - nc.m1) / nc.d1;
        o[2] = (c[2] / 255.0f - nc.m2) / nc.d2;
    }
}

// `weather` [B] is read by the WX instantiations only and `view` [B] by the VW ones (the other
// entry points pass nullptr).
template <bool WX, bool VW>
__global__ __launch_bounds__(256) void augment_u8_kernel(
    const unsigned char* __restrict__ frames, const cilrs_aug_params* __restrict__ params,
    const cilrs_weather_params* __restrict__ weather, const cilrs_view_params* __restrict__ view,
    const int B, const int H, const int W, float* __restrict__ out_f32,
    unsigned char* __restrict__ out_u8, const NormConsts nc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H * W) return;
    const int x = i % W, y = (i / W) % H, b = i / (W * H);
    const cilrs_aug_params a = params[b];
    cilrs_weather_params w;
    if constexpr (WX) w = weather[b];
    cilrs_view_params v;
    if constexpr (VW) v = view[b];
    augment_pixel<WX, VW>(frames + (size_t)b * H * W * 3, a, w, v, y, x, H, W, (size_t)i, out_f32,
                          out_u8, nc);
}

// A whole training batch from the device-resident dataset: sample b of the batch is frame
// index[b] of the cache (64-bit offset: the cache passes 4 GiB at 81.4 K reference-size frames),
// augmented exactly as augment_u8_kernel would, and its labels are gathered by the same index by
// the thread of the sample's first pixel.  An index outside [0, n_frames) is the caller's error
// (checked on the host, cilrs_mi355/data.py); such a sample is skipped, never read.  With VW and
// the sample's record on, the same thread adds the record's steer_delta to the steer label and
// clips it to [-1, 1]; an off record copies the three targets (a stored -0.0 stays -0.0).
struct AssembleLabels {
    const float* speed;
    const long long* command;
    const float* targets;
    float* out_speed;
    long long* out_command;
    float* out_targets;
};

template <bool WX, bool VW>
__global__ __launch_bounds__(256) void batch_assemble_kernel(
    const unsigned char* __restrict__ cache, const long long n_frames,
    const long long* __restrict__ index, const cilrs_aug_params* __restrict__ params,
    const cilrs_weather_params* __restrict__ weather, const cilrs_view_params* __restrict__ view,
    const int B, const int H, const int W, float* __restrict__ out_f32,
    unsigned char* __restrict__ out_u8, const AssembleLabels lab, const NormConsts nc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H * W) return;
    const int x = i % W, y = (i / W) % H, b = i / (W * H);
    const long long src = index[b];
    if (src < 0 || src >= n_frames) return;
    cilrs_view_params v;
    if constexpr (VW) v = view[b];
    if (x == 0 && y == 0) {
        if (lab.out_speed) lab.out_speed[b] = lab.speed[src];
        if (lab.out_command) lab.out_command[b] = lab.command[src];
        if (lab.out_targets) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float t = lab.targets[src * 3 + k];
                if constexpr (VW) {
                    if (k == 0 && v.on != 0) t = fminf(fmaxf(t + v.steer_delta, -1.f), 1.f);
                }
                lab.out_targets[b * 3 + k] = t;
            }
        }
    }
    const cilrs_aug_params a = params[b];
    cilrs_weather_params w;
    if constexpr (WX) w = weather[b];
    augment_pixel<WX, VW>(cache + (size_t)src * H * W * 3, a, w, v, y, x, H, W, (size_t)i, out_f32,
                          out_u8, nc);
}

constexpr NormConsts kNorm = {kImageMean[0], kImageMean[1], kImageMean[2],
                              kImageStd[0],  kImageStd[1],  kImageStd[2]};

// rain heads are hashed from (row + 64, column + 64) packed into 16 bits each
constexpr int kWeatherMaxWidth = 65536 - 128;

template <bool WX, bool VW>
int launch_augment(const unsigned char* frames, const cilrs_aug_params* params,
                   const cilrs_weather_params* weather, const cilrs_view_params* view, int B,
                   int H, int W, float* out_f32, unsigned char* out_u8, hipStream_t s) {
    CILRS_CHECK(B >= 1 && H >= 2 && W >= 2 && (size_t)B * H * W < (1u << 31),
                "augment: bad batch geometry");
    augment_u8_kernel<WX, VW><<<cdiv(B * H * W, 256), 256, 0, s>>>(
        frames, params, weather, view, B, H, W, out_f32, out_u8, kNorm);
    CILRS_LAUNCH_CHECK();
    return 0;
}

template <bool WX, bool VW>
int launch_assemble(const unsigned char* cache, long long n_frames, const AssembleLabels& lab,
                    const long long* index, const cilrs_aug_params* params,
                    const cilrs_weather_params* weather, const cilrs_view_params* view, int B,
                    int H, int W, float* out_f32, unsigned char* out_u8, hipStream_t s) {
    // the guard is on the BATCH (thread and output indices are int); the cache is addressed in
    // 64 bits and may be any size
    CILRS_CHECK(B >= 1 && H >= 2 && W >= 2 && (size_t)B * H * W < (1u << 31),
                "batch_assemble: bad batch geometry");
    CILRS_CHECK(n_frames >= 1, "batch_assemble: empty frame cache");
    batch_assemble_kernel<WX, VW><<<cdiv(B * H * W, 256), 256, 0, s>>>(
        cache, n_frames, index, params, weather, view, B, H, W, out_f32, out_u8, lab, kNorm);
    CILRS_LAUNCH_CHECK();
    return 0;
}

}  // namespace

int launch_augment_u8(const unsigned char* frames, const cilrs_aug_params* params, int B, int H,
                      int W, float* out_f32, unsigned char* out_u8, hipStream_t s) {
    return launch_augment<false, false>(frames, params, nullptr, nullptr, B, H, W, out_f32, out_u8,
                                        s);
}

int launch_augment_weather_u8(const unsigned char* frames, const cilrs_aug_params* params,
                              const cilrs_weather_params* weather, int B, int H, int W,
                              float* out_f32, unsigned char* out_u8, hipStream_t s) {
    CILRS_CHECK(W <= kWeatherMaxWidth, "augment_weather: width %d above %d", W, kWeatherMaxWidth);
    return launch_augment<true, false>(frames, params, weather, nullptr, B, H, W, out_f32, out_u8,
                                       s);
}

int launch_batch_assemble(const unsigned char* cache, long long n_frames, const float* speed,
                          const long long* command, const float* targets, const long long* index,
                          const cilrs_aug_params* params, int B, int H, int W, float* out_f32,
                          unsigned char* out_u8, float* out_speed, long long* out_command,
                          float* out_targets, hipStream_t s) {
    const AssembleLabels lab = {speed, command, targets, out_speed, out_command, out_targets};
    return launch_assemble<false, false>(cache, n_frames, lab, index, params, nullptr, nullptr, B,
                                         H, W, out_f32, out_u8, s);
}

int launch_batch_assemble_weather(const unsigned char* cache, long long n_frames,
                                  const float* speed, const long long* command,
                                  const float* targets, const long long* index,
                                  const cilrs_aug_params* params,
                                  const cilrs_weather_params* weather, int B, int H, int W,
                                  float* out_f32, unsigned char* out_u8, float* out_speed,
                                  long long* out_command, float* out_targets, hipStream_t s) {
    CILRS_CHECK(W <= kWeatherMaxWidth, "batch_assemble_weather: width %d above %d", W,
                kWeatherMaxWidth);
    const AssembleLabels lab = {speed, command, targets, out_speed, out_command, out_targets};
    return launch_assemble<true, false>(cache, n_frames, lab, index, params, weather, nullptr, B, H,
                                        W, out_f32, out_u8, s);
}

// weather may be nullptr (the viewpoint alone); the width limit is the weather's
int launch_augment_view_u8(const unsigned char* frames, const cilrs_aug_params* params,
                           const cilrs_weather_params* weather, const cilrs_view_params* view,
                           int B, int H, int W, float* out_f32, unsigned char* out_u8,
                           hipStream_t s) {
    if (!weather)
        return launch_augment<false, true>(frames, params, nullptr, view, B, H, W, out_f32, out_u8,
                                           s);
    CILRS_CHECK(W <= kWeatherMaxWidth, "augment_view: width %d above %d", W, kWeatherMaxWidth);
    return launch_augment<true, true>(frames, params, weather, view, B, H, W, out_f32, out_u8, s);
}

int launch_batch_assemble_view(const unsigned char* cache, long long n_frames, const float* speed,
                               const long long* command, const float* targets,
                               const long long* index, const cilrs_aug_params* params,
                               const cilrs_weather_params* weather, const cilrs_view_params* view,
                               int B, int H, int W, float* out_f32, unsigned char* out_u8,
                               float* out_speed, long long* out_command, float* out_targets,
                               hipStream_t s) {
    const AssembleLabels lab = {speed, command, targets, out_speed, out_command, out_targets};
    if (!weather)
        return launch_assemble<false, true>(cache, n_frames, lab, index, params, nullptr, view, B,
                                            H, W, out_f32, out_u8, s);
    CILRS_CHECK(W <= kWeatherMaxWidth, "batch_assemble_view: width %d above %d", W,
                kWeatherMaxWidth);
    return launch_assemble<true, true>(cache, n_frames, lab, index, params, weather, view, B, H, W,
                                       out_f32, out_u8, s);
}

}  // namespace cilrs
