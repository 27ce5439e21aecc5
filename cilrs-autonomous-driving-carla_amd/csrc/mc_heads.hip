// Monte-Carlo dropout through the heads (cilrs_heads_mc / cilrs_net_heads_mc, include/cilrs_hip.h).
//
// Every Dropout of the network sits in the heads (model/autonomous_drive.py:371-387), so in eval
// mode the trunk is deterministic and runs once; only the heads run S times, each with its own
// keep masks.  Sample s of frame b is row r = b * S + s of a heads batch of B * S rows under the
// train-mode hash (dropout_u in common.h == dropout_kernel / hgemm_kernel), so the S x 4 outputs are
// exactly what a train-mode heads forward over S copies of the frame's features would return with
// BatchNorm left in eval mode.
//
// Three launches, no atomics, no barriers across workgroups, every sum in a fixed order:
//   mc_pre_kernel     what does not depend on the sample: a0 = relu(W_se0 x + b), the visual half of
//                     the commanded branch's first layer hv = W_k0[:, :F] v + b, pp = relu(W_p0 v + b),
//                     each once per frame.  Where the source is a feature map (after the persistent
//                     launch) every one of the frame's 64 workgroups pools it into its own LDS copy
//                     of v: 64 x HW x F reads from L2 (2.7 MB at 88x200) instead of a fourth launch
//                     or a hand-off between workgroups -- per frame, never per sample.
//                     The two GEMVs read 2 * 256 * F weights (1 MB at F = 512, more than all
//                     per-sample weights together): one wave per output feature over 64 workgroups
//                     per frame.
//   mc_sample_kernel  one workgroup per (frame, 32 sample rows, chain): chain 0 = speed encoder +
//                     commanded branch (three GEMMs), chain 1 = speed predictor (one GEMM).  Sample
//                     rows are the M dimension of v_mfma_f32_32x32x2_f32 (exact fp32), activations
//                     live in LDS, weights come straight from L2, each of the eight waves owns one
//                     32-column tile over the whole reduction index -- a row's values depend only on
//                     (seed, r, inputs), never on which rows share its tile.
//   mc_stats_kernel   mean and unbiased std of each frame's S stored fp32 values, two passes in
//                     double in sample order, rounded once.  A call whose samples fit one tile
//                     (S <= 32) runs the same loop at the end of mc_sample_kernel instead.
#include "common.h"

namespace cilrs {
namespace {

constexpr int kMcRows = 32;            // sample rows per workgroup (MFMA M)
constexpr int kMcLd = 260;             // LDS row pitch in floats (256 + 4: rows 16 bytes apart in banks)
constexpr int kMcOutOff = 2 * kMcRows * kMcLd;
constexpr int kMcLdsBytes = (kMcOutOff + kMcRows * 4) * (int)sizeof(float);

__global__ __launch_bounds__(512) void mc_pre_kernel(const McHeadsArgs a) {
    __shared__ float v[kMcMaxFeat];
    const int b = blockIdx.x >> 6, part = blockIdx.x & 63;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const HeadWeights& hw = a.hw;
    const int F = hw.F;
    const int k = command_branch(a.cmd, b, hw.ncmd);
    for (int c = tid; c < F; c += 512) v[c] = pooled_feature(a.src, F, b, c);
    float* sh = a.shared + (size_t)b * kMcSharedFloats;
    if (part == 0) {
        if (tid < 128) sh[tid] = fmaxf(fmaf(hw.se0_w[tid], a.speed[b], hw.se0_b[tid]), 0.f);
        // a command outside 0..ncmd-1: torch.gather would raise; branch 0 is used (sticky word)
        if (tid == 0 && a.status && (a.cmd[b] < 0 || a.cmd[b] >= hw.ncmd)) a.status[0] = 1;
    }
    __syncthreads();
    const int slot = part * 8 + wave;            // 0..255 hv, 256..511 pp
    const int o = slot & 255;
    const bool sp = slot >= 256;
    const float* w = sp ? hw.sp0_w + (size_t)o * F : hw.br_w[k][0] + (size_t)o * (F + 128);
    float acc = 0.f;
    for (int q = lane; q < (F >> 2); q += 64) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w + q * 4);
        const f32x4 xv = *reinterpret_cast<const f32x4*>(v + q * 4);
        acc = fmaf(xv[0], wv[0], acc);
        acc = fmaf(xv[1], wv[1], acc);
        acc = fmaf(xv[2], wv[2], acc);
        acc = fmaf(xv[3], wv[3], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        if (sp) sh[384 + o] = fmaxf(acc + hw.sp0_b[o], 0.f);
        else sh[128 + o] = acc + hw.br_b[k][0][o];
    }
}

// One 32 x 32 output tile: rows = the workgroup's sample rows (LDS, pitch kMcLd), columns n0..n0+31
// of an nn.Linear whose weight rows are ldw floats apart (the reduction runs over columns
// [0, K) of `w`).  Operand and accumulator maps as in hgemm_kernel.
__device__ __forceinline__ f32x16 mc_tile(const float* __restrict__ x, const float* __restrict__ w,
                                          const int ldw, const int K, const int n0, const int lane) {
    const int r = lane & 31, kh = lane >> 5;
    const float* xr = x + r * kMcLd + kh * 4;
    const float* wr = w + (size_t)(n0 + r) * ldw + kh * 4;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll 4
    for (int k0 = 0; k0 < K; k0 += 8) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(wr + k0);
        const f32x4 av = *reinterpret_cast<const f32x4*>(xr + k0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bv[e], acc, 0, 0, 0);
    }
    return acc;
}

// bias (or the frame's shared pre-activation) + ReLU + dropout of one tile, into LDS.
// Accumulator map: column = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5).
__device__ __forceinline__ void mc_store_tile(const f32x16& acc, float* __restrict__ y,
                                              const float* __restrict__ add, const int n0,
                                              const int lane, const int cols, const long long site,
                                              const unsigned row0, const float p,
                                              const unsigned long long seed) {
    const int n = n0 + (lane & 31), kh = lane >> 5;
    const float bn = add[n];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * kh;
        float v = fmaxf(acc[i] + bn, 0.f);
        if (site >= 0 && p > 0.f) {
            const float u = dropout_u(seed, (unsigned long long)site, (row0 + row) * (unsigned)cols + n);
            v = (u >= p) ? v / (1.0f - p) : 0.f;
        }
        y[row * kMcLd + n] = v;
    }
}

// a sample-independent activation row under this row's mask (the first Dropout of a chain)
__device__ __forceinline__ void mc_mask_rows(const float* __restrict__ src, float* __restrict__ y,
                                             const int cols, const long long site,
                                             const unsigned row0, const float p,
                                             const unsigned long long seed, const int tid) {
    for (int i = tid; i < kMcRows * cols; i += 512) {
        const int row = i / cols, c = i - row * cols;
        float v = src[c];
        if (p > 0.f) {
            const float u = dropout_u(seed, (unsigned long long)site, (row0 + row) * (unsigned)cols + c);
            v = (u >= p) ? v / (1.0f - p) : 0.f;
        }
        y[row * kMcLd + c] = v;
    }
}

// mean / unbiased std of S values `stride` floats apart: two passes in double, sample order
__device__ __forceinline__ void mc_stats(const float* __restrict__ x, const int stride, const int S,
                                         float* mean, float* stdv) {
    double s = 0.0;
    for (int i = 0; i < S; ++i) s += (double)x[(size_t)i * stride];
    const double m = s / (double)S;
    double q = 0.0;
    for (int i = 0; i < S; ++i) {
        const double d = (double)x[(size_t)i * stride] - m;
        q += d * d;
    }
    *mean = (float)m;
    *stdv = S > 1 ? (float)sqrt(q / (double)(S - 1)) : 0.f;
}

__global__ __launch_bounds__(512) void mc_sample_kernel(const McHeadsArgs a) {
    extern __shared__ __align__(16) float lds[];
    float* X = lds;                            // s1 / h1 / p1
    float* Y = lds + kMcRows * kMcLd;          // f / h2 / p2
    float* outv = lds + kMcOutOff;             // [32][4] this tile's outputs
    const int b = blockIdx.x / a.nchunks, chain = blockIdx.z;
    const int s0 = (blockIdx.x - b * a.nchunks) * kMcRows;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const HeadWeights& hw = a.hw;
    const int S = a.S, F = hw.F, NC = hw.ncmd;
    const unsigned row0 = (unsigned)(b * S + s0);
    const float p = a.p;
    const unsigned long long seed = a.seed;
    const float* sh = a.shared + (size_t)b * kMcSharedFloats;
    const int k = command_branch(a.cmd, b, hw.ncmd);
    const float* wl;                           // the chain's last Linear
    const float* bl;
    int nout;
    if (chain == 0) {
        // s1 = drop_0(relu(W_se0 x + b)); f = relu(W_se3 s1 + b)
        mc_mask_rows(sh, X, 128, 0, row0, p, seed, tid);
        __syncthreads();
        if (wave < 4) {
            const f32x16 acc = mc_tile(X, hw.se3_w, 128, 128, wave * 32, lane);
            mc_store_tile(acc, Y, hw.se3_b, wave * 32, lane, 128, -1, row0, p, seed);
        }
        __syncthreads();
        // h1 = drop_{1+2k}(relu(W_k0 [v | f] + b)): the visual half and the bias come from hv
        const f32x16 acc1 = mc_tile(Y, hw.br_w[k][0] + F, F + 128, 128, wave * 32, lane);
        mc_store_tile(acc1, X, sh + 128, wave * 32, lane, 256, 1 + 2 * k, row0, p, seed);
        __syncthreads();
        // h2 = drop_{2+2k}(relu(W_k3 h1 + b))
        const f32x16 acc2 = mc_tile(X, hw.br_w[k][1], 256, 256, wave * 32, lane);
        mc_store_tile(acc2, Y, hw.br_b[k][1], wave * 32, lane, 256, 2 + 2 * k, row0, p, seed);
        wl = hw.br_w[k][2]; bl = hw.br_b[k][2]; nout = 3;
    } else {
        // p1 = drop_{2NC+1}(relu(W_p0 v + b)); p2 = relu(W_p3 p1 + b)
        mc_mask_rows(sh + 384, X, 256, 2 * NC + 1, row0, p, seed, tid);
        __syncthreads();
        const f32x16 acc = mc_tile(X, hw.sp3_w, 256, 256, wave * 32, lane);
        mc_store_tile(acc, Y, hw.sp3_b, wave * 32, lane, 256, -1, row0, p, seed);
        wl = hw.sp5_w; bl = hw.sp5_b; nout = 1;
    }
    __syncthreads();
    // last Linear (3 or 1 outputs over 256 inputs): a wave per row, a lane per input quad
    const int col0 = chain == 0 ? 0 : 3;
    for (int row = wave; row < kMcRows; row += 8) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(Y + row * kMcLd + lane * 4);
        for (int o = 0; o < nout; ++o) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + o * 256 + lane * 4);
            float acc = xv[0] * wv[0];
            acc = fmaf(xv[1], wv[1], acc);
            acc = fmaf(xv[2], wv[2], acc);
            acc = fmaf(xv[3], wv[3], acc);
            acc = wave_sum(acc) + bl[o];
            if (lane == 0) {
                outv[row * 4 + col0 + o] = acc;
                if (s0 + row < S) {
                    const size_t at = ((size_t)b * S + s0 + row) * 4 + col0 + o;
                    a.samples[at] = acc;
                    if (a.samples_out) a.samples_out[at] = acc;
                }
            }
        }
    }
    if (S > kMcRows) return;                   // mc_stats_kernel follows
    __syncthreads();
    if (tid < nout)
        mc_stats(outv + col0 + tid, 4, S, a.mean + (size_t)b * 4 + col0 + tid,
                 a.stdv + (size_t)b * 4 + col0 + tid);
}

__global__ __launch_bounds__(64) void mc_stats_kernel(const McHeadsArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;       // (frame, output)
    if (i >= a.B * 4) return;
    const int b = i >> 2, o = i & 3;
    mc_stats(a.samples + (size_t)b * a.S * 4 + o, 4, a.S, a.mean + i, a.stdv + i);
}

}  // namespace

size_t mc_heads_scratch_floats(int batch, int samples) {
    return (size_t)batch * kMcSharedFloats + (size_t)batch * samples * 4;
}

int launch_mc_heads(McHeadsArgs& a, float* scratch, hipStream_t s) {
    CILRS_CHECK(a.hw.F % 4 == 0 && a.hw.F >= 4 && a.hw.F <= kMcMaxFeat, "heads_mc: feature width %d",
                a.hw.F);
    a.shared = scratch;
    a.samples = scratch + (size_t)a.B * kMcSharedFloats;
    if (set_max_dynamic_lds(reinterpret_cast<const void*>(mc_sample_kernel), kMcLdsBytes)) return 1;
    a.nchunks = cdiv(a.S, kMcRows);
    mc_pre_kernel<<<64 * a.B, 512, 0, s>>>(a);
    CILRS_LAUNCH_CHECK();
    mc_sample_kernel<<<dim3(a.nchunks * a.B, 1, 2), 512, kMcLdsBytes, s>>>(a);
    CILRS_LAUNCH_CHECK();
    if (a.S > kMcRows) {
        mc_stats_kernel<<<cdiv(a.B * 4, 64), 64, 0, s>>>(a);
        CILRS_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace cilrs
