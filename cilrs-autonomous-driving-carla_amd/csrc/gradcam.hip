// Grad-CAM: class-activation maps of a trunk group (cilrs_heads_input_grad, cilrs_gradcam_map,
// cilrs_net_gradcam; the definition is in include/cilrs_hip.h).
//
// The reference draws its HUD on every tick (DashboardHUD, model/autonomous_drive.py:178-355) but
// has nothing that says which region of the frame carried the command.  AdaptiveAvgPool2d sits
// directly on layer4 (autonomous_drive.py:365-370), so the gradient of an output with respect to
// the last feature map is d out / d pooled spread evenly over its cells: the channel weights of
// layer4 need the heads alone, forward and backward, 0.36 MFLOP each way.
//
// Two kernels, no atomics, every sum in a fixed order, a frame's result independent of its batch:
//   heads_input_grad_kernel  one 1,024-thread workgroup per frame, the whole chain out of LDS.
//                            Forward GEMVs: a wave per four output features, lanes stride the weight
//                            rows in 16-byte pieces, butterfly sum.  Backward (transposed) GEMVs: a
//                            thread owns four adjacent columns, the rows are split over the thread
//                            groups that fit the workgroup, the groups' partial sums meet in LDS in
//                            group order.  Both keep several rows' loads in flight per thread: one
//                            workgroup has to pull the weights through a single CU.
//                            3.5 MB of weights per frame come from L2.
//   gradcam_map_kernel       one 1,024-thread workgroup per frame: channel weights (from g, or the
//                            pixel mean of dA with the pixels split over thread groups and joined in
//                            LDS in group order), one wave per cell for the channel sum, the peak by
//                            shuffles + LDS, the normalised coarse map in LDS, then the bilinear
//                            upsample with coordinates and blend in double, rounded once.
#include "common.h"

namespace cilrs {
namespace {

constexpr int kGcThreads = 1024;
constexpr int kGcWaves = kGcThreads / 64;

// y[o] = act(W[o][0..K) . x + b[o]) for o in [0, n): a wave takes four rows at a time so that their
// loads are in flight together; lanes stride each row in 16-byte pieces, butterfly sum.  K % 4 == 0,
// n % 4 == 0, x in LDS
__device__ __forceinline__ void gc_rows(const float* __restrict__ W, const int ldw, const int K,
                                        const int n, const float* __restrict__ bias,
                                        const float* x, float* y, const bool relu, const int wave,
                                        const int lane) {
    for (int o0 = wave * 4; o0 < n; o0 += kGcWaves * 4) {
        const float* w = W + (size_t)o0 * ldw;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int q = lane; q < (K >> 2); q += 64) {
            f32x4 wv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                wv[r] = *reinterpret_cast<const f32x4*>(w + (size_t)r * ldw + q * 4);
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + q * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc[r] = fmaf(xv[0], wv[r][0], acc[r]);
                acc[r] = fmaf(xv[1], wv[r][1], acc[r]);
                acc[r] = fmaf(xv[2], wv[r][2], acc[r]);
                acc[r] = fmaf(xv[3], wv[r][3], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = wave_sum(acc[r]) + bias[o0 + r];
            if (lane == 0) y[o0 + r] = relu ? fmaxf(v, 0.f) : v;
        }
    }
}

// y = W[0..256) . x + b: one output of a last Linear, by one wave
__device__ __forceinline__ void gc_row_256(const float* __restrict__ w, const float* __restrict__ bias,
                                           const float* x, float* y, const int lane) {
    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + lane * 4);
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + lane * 4);
    float acc = __fmul_rn(xv[0], wv[0]);
    acc = fmaf(xv[1], wv[1], acc);
    acc = fmaf(xv[2], wv[2], acc);
    acc = fmaf(xv[3], wv[3], acc);
    acc = wave_sum(acc) + bias[0];
    if (lane == 0) y[0] = acc;
}

// part[grp][c] = sum over the group's rows o of W[o][c] * d[o], c in [0, ncols): ncols % 256 == 0,
// ncols <= 4096 (a thread owns four columns, ncols / 4 threads make a group, a group is whole
// waves), rows in ascending order, eight loads in flight; a row behind a dead ReLU unit adds
// W * 0.  nrows divides evenly by 8 * groups.  Returns the number of groups; the caller joins them.
__device__ __forceinline__ int gc_cols_partial(const float* __restrict__ W, const int ldw,
                                               const int ncols, const int nrows, const float* d,
                                               float* part, const int tid) {
    const int per = ncols >> 2;
    const int groups = kGcThreads / per;
    const int grp = tid / per, q = tid - grp * per;
    if (grp < groups) {
        const int rows = nrows / groups;
        const float* w = W + (size_t)(grp * rows) * ldw + q * 4;
        const float* dg = d + grp * rows;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int o = 0; o < rows; o += 8) {
            f32x4 wv[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) wv[r] = *reinterpret_cast<const f32x4*>(w + (size_t)(o + r) * ldw);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float dv = dg[o + r];
                acc[0] = fmaf(wv[r][0], dv, acc[0]);
                acc[1] = fmaf(wv[r][1], dv, acc[1]);
                acc[2] = fmaf(wv[r][2], dv, acc[2]);
                acc[3] = fmaf(wv[r][3], dv, acc[3]);
            }
        }
        *reinterpret_cast<f32x4*>(part + (size_t)grp * ncols + q * 4) = acc;
    }
    return groups;
}

__device__ __forceinline__ float gc_join(const float* part, const int groups, const int ncols,
                                         const int c) {
    float s = part[c];
    for (int g = 1; g < groups; ++g) s += part[(size_t)g * ncols + c];
    return s;
}

__global__ __launch_bounds__(kGcThreads) void heads_input_grad_kernel(const HeadsGradArgs a) {
    __shared__ __align__(16) float comb[kMcMaxFeat + 128];   // [v | f]
    __shared__ __align__(16) float a0[128];
    __shared__ __align__(16) float act[4][256];               // h1, h2, p1, p2
    __shared__ __align__(16) float dv[4][256];                // dh2, dh1, dp2, dp1
    __shared__ __align__(16) float part[4096];                // partial column sums [groups][ncols]
    __shared__ float outv[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const HeadWeights& hw = a.hw;
    const int F = hw.F;
    const int k = command_branch(a.cmd, b, hw.ncmd);
    if (tid == 0 && a.status && (a.cmd[b] < 0 || a.cmd[b] >= hw.ncmd)) a.status[0] = 1;
    for (int c = tid; c < F; c += kGcThreads) comb[c] = pooled_feature(a.src, F, b, c);
    if (tid < 128) a0[tid] = fmaxf(fmaf(hw.se0_w[tid], a.speed[b], hw.se0_b[tid]), 0.f);
    __syncthreads();
    // forward: f, then h1 and p1 (both read comb), h2 and p2, the four outputs
    gc_rows(hw.se3_w, 128, 128, 128, hw.se3_b, a0, comb + F, true, wave, lane);
    __syncthreads();
    gc_rows(hw.br_w[k][0], F + 128, F + 128, 256, hw.br_b[k][0], comb, act[0], true, wave, lane);
    gc_rows(hw.sp0_w, F, F, 256, hw.sp0_b, comb, act[2], true, wave, lane);
    __syncthreads();
    gc_rows(hw.br_w[k][1], 256, 256, 256, hw.br_b[k][1], act[0], act[1], true, wave, lane);
    gc_rows(hw.sp3_w, 256, 256, 256, hw.sp3_b, act[2], act[3], true, wave, lane);
    __syncthreads();
    if (wave < 3) gc_row_256(hw.br_w[k][2] + wave * 256, hw.br_b[k][2] + wave, act[1], outv + wave, lane);
    else if (wave == 3) gc_row_256(hw.sp5_w, hw.sp5_b, act[3], outv + 3, lane);
    // backward of y = w . outputs: dh2 = relu'(h2) W_k5^T w[0..2], dp2 = relu'(p2) W_p5^T w[3]
    if (tid >= 256 && tid < 512) {
        const int j = tid - 256;
        const float* w5 = hw.br_w[k][2];
        float s = __fmul_rn(w5[j], a.w[0]);
        s = fmaf(w5[256 + j], a.w[1], s);
        s = fmaf(w5[512 + j], a.w[2], s);
        dv[0][j] = act[1][j] > 0.f ? s : 0.f;
    } else if (tid >= 512 && tid < 768) {
        const int j = tid - 512;
        dv[2][j] = act[3][j] > 0.f ? __fmul_rn(hw.sp5_w[j], a.w[3]) : 0.f;
    }
    __syncthreads();
    if (a.out4 && tid < 4) a.out4[(size_t)b * 4 + tid] = outv[tid];
    // dh1 = relu'(h1) W_k3^T dh2
    int groups = gc_cols_partial(hw.br_w[k][1], 256, 256, 256, dv[0], part, tid);
    __syncthreads();
    if (tid < 256) dv[1][tid] = act[0][tid] > 0.f ? gc_join(part, groups, 256, tid) : 0.f;
    __syncthreads();
    // dp1 = relu'(p1) W_p3^T dp2
    groups = gc_cols_partial(hw.sp3_w, 256, 256, 256, dv[2], part, tid);
    __syncthreads();
    if (tid < 256) dv[3][tid] = act[2][tid] > 0.f ? gc_join(part, groups, 256, tid) : 0.f;
    __syncthreads();
    // g = W_k0[:, :F]^T dh1 + W_p0^T dp1, the branch first (comb is free now: it holds the first)
    groups = gc_cols_partial(hw.br_w[k][0], F + 128, F, 256, dv[1], part, tid);
    __syncthreads();
    for (int c = tid; c < F; c += kGcThreads) comb[c] = gc_join(part, groups, F, c);
    __syncthreads();
    groups = gc_cols_partial(hw.sp0_w, F, F, 256, dv[3], part, tid);
    __syncthreads();
    float* g = a.g + (size_t)b * F;
    for (int c = tid; c < F; c += kGcThreads) g[c] = __fadd_rn(comb[c], gc_join(part, groups, F, c));
}

__global__ __launch_bounds__(kGcThreads) void gradcam_map_kernel(const GradcamMapArgs a) {
    __shared__ float alpha[kGcMaxC];
    __shared__ float part[kGcMaxC];
    __shared__ float coarse[kGcMaxHW];
    __shared__ float red[kGcWaves];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, hw = a.h * a.w;
    const float* A = a.A + (size_t)b * hw * C;
    // channel weights
    if (a.g) {
        for (int c = tid; c < C; c += kGcThreads) alpha[c] = __fdiv_rn(a.g[(size_t)b * C + c], (float)hw);
    } else {
        const float* dA = a.dA + (size_t)b * hw * C;
        if (C >= kGcThreads) {
            for (int c = tid; c < C; c += kGcThreads) {
                float s = 0.f;
                for (int p = 0; p < hw; ++p) s += dA[(size_t)p * C + c];
                alpha[c] = __fdiv_rn(s, (float)hw);
            }
        } else {
            // the pixels split over kGcThreads / C thread groups: p = grp, grp + groups, ...
            const int groups = kGcThreads / C;
            const int grp = tid / C, c = tid - grp * C;
            float s = 0.f;
            for (int p = grp; p < hw; p += groups) s += dA[(size_t)p * C + c];
            part[tid] = s;
            __syncthreads();
            if (tid < C) {
                float t = part[tid];
                for (int g = 1; g < groups; ++g) t += part[g * C + tid];
                alpha[tid] = __fdiv_rn(t, (float)hw);
            }
        }
    }
    __syncthreads();
    // cam[p] = sum_c alpha[c] A[p][c]: a wave per cell, lane l takes c = l, l + 64, ...
    float* cam = a.cam + (size_t)b * hw;
    float m = 0.f;
    for (int p = wave; p < hw; p += kGcWaves) {
        const float* ap = A + (size_t)p * C;
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) acc = fmaf(alpha[c], ap[c], acc);
        acc = wave_sum(acc);
        if (lane == 0) { cam[p] = acc; coarse[p] = fmaxf(acc, 0.f); }
        m = fmaxf(m, acc);
    }
    if (lane == 0) red[wave] = m;
    __syncthreads();
    float pk = red[0];
#pragma unroll
    for (int i = 1; i < kGcWaves; ++i) pk = fmaxf(pk, red[i]);
    if (tid == 0) a.peak[b] = pk;
    for (int p = tid; p < hw; p += kGcThreads) coarse[p] = pk > 0.f ? __fdiv_rn(coarse[p], pk) : 0.f;
    __syncthreads();
    // bilinear upsample, half-pixel centres (F.interpolate(mode="bilinear", align_corners=False))
    const int H = a.H, W = a.W, h = a.h, w = a.w;
    const double sy = (double)h / (double)H, sx = (double)w / (double)W;
    float* heat = a.heat + (size_t)b * H * W;
    unsigned char* u8 = a.heat_u8 ? a.heat_u8 + (size_t)b * H * W : nullptr;
    for (int i = tid; i < H * W; i += kGcThreads) {
        const int y = i / W, x = i - y * W;
        double fy = ((double)y + 0.5) * sy - 0.5, fx = ((double)x + 0.5) * sx - 0.5;
        fy = fmin(fmax(fy, 0.0), (double)(h - 1));
        fx = fmin(fmax(fx, 0.0), (double)(w - 1));
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
        const double ly = fy - (double)y0, lx = fx - (double)x0;
        const double top = (1.0 - lx) * (double)coarse[y0 * w + x0] + lx * (double)coarse[y0 * w + x1];
        const double bot = (1.0 - lx) * (double)coarse[y1 * w + x0] + lx * (double)coarse[y1 * w + x1];
        const float hv = (float)((1.0 - ly) * top + ly * bot);
        heat[i] = hv;
        if (u8) u8[i] = (unsigned char)floorf(__fadd_rn(__fmul_rn(hv, 255.f), 0.5f));
    }
}

}  // namespace

int launch_heads_input_grad(const HeadsGradArgs& a, hipStream_t s) {
    const int F = a.hw.F;
    CILRS_CHECK((F == 256 || F == 512 || F == 1024 || F == 2048) && F <= kMcMaxFeat,
                "heads_input_grad: feature width %d", F);
    heads_input_grad_kernel<<<a.B, kGcThreads, 0, s>>>(a);
    CILRS_LAUNCH_CHECK();
    return 0;
}

int launch_gradcam_map(const GradcamMapArgs& a, hipStream_t s) {
    CILRS_CHECK(a.A && a.cam && a.peak && a.heat, "gradcam_map: NULL tensor");
    CILRS_CHECK((a.dA != nullptr) != (a.g != nullptr),
                "gradcam_map: exactly one of dA and g must be given");
    CILRS_CHECK(a.B >= 1 && a.h >= 1 && a.w >= 1 && a.H >= 1 && a.W >= 1,
                "gradcam_map: non-positive size (B %d, map %dx%d, heat %dx%d)", a.B, a.h, a.w, a.H, a.W);
    CILRS_CHECK((long long)a.h * a.w <= kGcMaxHW, "gradcam_map: %dx%d cells above %d", a.h, a.w,
                kGcMaxHW);
    CILRS_CHECK((long long)a.H * a.W < (1ll << 31), "gradcam_map: heat map %dx%d too large", a.H, a.W);
    CILRS_CHECK(a.C == 64 || a.C == 128 || a.C == 256 || a.C == 512 || a.C == 1024 || a.C == 2048,
                "gradcam_map: %d channels (64, 128, 256, 512, 1024 or 2048)", a.C);
    gradcam_map_kernel<<<a.B, kGcThreads, 0, s>>>(a);
    CILRS_LAUNCH_CHECK();
    return 0;
}

}  // namespace cilrs
