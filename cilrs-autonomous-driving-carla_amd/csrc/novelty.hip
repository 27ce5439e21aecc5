// Feature-space novelty score (cilrs_feature_moments / cilrs_feature_novelty and their plan-level
// forms, include/cilrs_hip.h): the Mahalanobis distance of the pooled trunk features to
// command-conditional Gaussians with one tied covariance.
//
// Fit: nov_moments_kernel adds a batch of rows into the float64 moment table.  One workgroup owns
// one 64 x 64 tile of the lower triangle of G; 256 threads, each a 4 x 4 register block of chains.
// The rows' columns of the tile are staged in LDS as x = (double)v - (double)pivot, 32 rows at a
// time, and every entry runs t = fma(x_bi, x_bj, t) over the rows in row order, starting from the
// value in the table: two updates of 2 + 3 rows are bit for bit one update of 5.  The diagonal tiles
// carry the per-command sums of their 64 columns along, tile (0, 0) the counts and the status word.
// No atomics, no hand-off between workgroups.  Where the source is a feature map every workgroup
// pools its own 128 columns (pooled_feature in common.h, as every consumer of a tick's features).
//
// Score: three launches.
//   nov_u_kernel     u[b][c] = v[b][c] - mean[k_b][c] into the caller's scratch (pooling a feature
//                    map first), the status word.
//   nov_gemv_kernel  y = W u over the lower triangle, the ROWS of W split over F / 8 workgroups:
//                    workgroup g owns rows g + (F / 8) r, r = 0..7 (interleaved, so that every
//                    workgroup reads the same share of the triangle), wave w rows r = 2w, 2w + 1.
//                    A wave loads its two rows once into registers -- all loads issued before the
//                    first use, columns j > i never read -- and applies them to every frame, the
//                    frames walking through LDS four at a time.  Writes the per-frame sum of
//                    squares of its eight rows.
//   nov_sum_kernel   d2[b] = the partial sums added in workgroup order.
// Whitening (cilrs_feature_whiten): the first two of those launches with one fixed origin instead
// of the per-frame command mean, y stored instead of summed (nov_u0_kernel, nov_whiten_kernel).
// Every sum runs in a fixed order (include/cilrs_hip.h states it); a frame's arithmetic never
// depends on which frames share its chunk.
#include "common.h"

#pragma clang fp contract(off)      // the chains are written with fma() / fmaf(); nothing else fuses

namespace cilrs {
namespace {

constexpr int kNovTile = 64;           // edge of a G tile
constexpr int kNovRows = 32;           // rows staged per pass of the moment kernel
constexpr int kNovFrames = 4;          // frames per LDS chunk of the triangular GEMV
constexpr int kNovWgRows = 8;          // rows of W per workgroup (two per wave)
constexpr int kNovQuads = kMcMaxFeat / 256;   // float4 per lane and row at the widest trunk

__global__ __launch_bounds__(256) void nov_moments_kernel(const NoveltyMomentsArgs a) {
    __shared__ double xi[kNovRows][kNovTile];
    __shared__ double xj[kNovRows][kNovTile];
    __shared__ int kb[kNovRows];
    // tile (ti, tj), tj <= ti, from the linear index t = ti (ti + 1) / 2 + tj
    int ti = (int)((sqrtf(8.f * (float)blockIdx.x + 1.f) - 1.f) * 0.5f);
    while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ++ti;
    while (ti * (ti + 1) / 2 > (int)blockIdx.x) --ti;
    const int tj = (int)blockIdx.x - ti * (ti + 1) / 2;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int F = a.F, NC = a.NC;
    const int i0 = ti * kNovTile, j0 = tj * kNovTile;
    const bool diag = ti == tj;
    double* G = a.table + (size_t)NC * (F + 1);

    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty * 4 + r, j = j0 + tx * 4 + c;
            acc[r][c] = j <= i ? G[(size_t)i * F + j] : 0.0;
        }
    // per-command sums of the tile's columns (diagonal tiles): chain (k, c) = s0 + 256 * e
    double sum[2] = {0.0, 0.0};
    int sk[2] = {-1, -1}, sc[2] = {0, 0};
    if (diag) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int idx = tid + 256 * e;
            if (idx < NC * kNovTile) {
                sk[e] = idx >> 6; sc[e] = idx & 63;
                sum[e] = a.table[NC + (size_t)sk[e] * F + i0 + sc[e]];
            }
        }
    }
    double cnt = 0.0;
    const bool counts = blockIdx.x == 0 && tid < NC;
    if (counts) cnt = a.table[tid];
    bool bad = false;

    for (int b0 = 0; b0 < a.B; b0 += kNovRows) {
        const int nb = min(kNovRows, a.B - b0);
        __syncthreads();
        for (int e = tid; e < nb * 2 * kNovTile; e += 256) {
            const int b = e >> 7, c = e & 127;
            const int col = c < kNovTile ? i0 + c : j0 + c - kNovTile;
            const float v = pooled_feature(a.src, F, b0 + b, col);
            const double x = (double)v - (double)a.pivot[col];
            if (c < kNovTile) xi[b][c] = x; else xj[b][c - kNovTile] = x;
        }
        if (tid < nb) kb[tid] = command_branch(a.cmd, b0 + tid, NC);
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
            double vi[4], vj[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { vi[r] = xi[b][ty * 4 + r]; vj[r] = xj[b][tx * 4 + r]; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fma(vi[r], vj[c], acc[r][c]);
        }
        if (diag) {
#pragma unroll
            for (int e = 0; e < 2; ++e)
                if (sk[e] >= 0)
                    for (int b = 0; b < nb; ++b)
                        if (kb[b] == sk[e]) sum[e] += xi[b][sc[e]];
        }
        if (counts)
            for (int b = 0; b < nb; ++b) {
                if (kb[b] == tid) cnt += 1.0;
                const long long c = a.cmd[b0 + b];
                bad |= c < 0 || c >= NC;
            }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty * 4 + r, j = j0 + tx * 4 + c;
            if (j <= i) G[(size_t)i * F + j] = acc[r][c];
        }
    if (diag) {
#pragma unroll
        for (int e = 0; e < 2; ++e)
            if (sk[e] >= 0) a.table[NC + (size_t)sk[e] * F + i0 + sc[e]] = sum[e];
    }
    if (counts) {
        a.table[tid] = cnt;
        // a command outside 0..NC-1 counts as command 0 (sticky word)
        if (tid == 0 && bad && a.status) a.status[0] = 1;
    }
}

// row i of W as a wave holds it: columns 256 q + 4 lane + e; zero where j > i (never loaded)
__device__ __forceinline__ void nov_load_w(const float* __restrict__ W, const int F, const int i,
                                           const int lane, f32x4 (&w)[kNovQuads]) {
    const int nq = F >> 8;
    const float* wr = W + (size_t)i * F;
#pragma unroll
    for (int q = 0; q < kNovQuads; ++q) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        const int j = q * 256 + lane * 4;
        if (q < nq) {
            if (j + 3 <= i) {
                v = *reinterpret_cast<const f32x4*>(wr + j);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j + e <= i) v[e] = wr[j + e];
            }
        }
        w[q] = v;
    }
}

// y_i = sum_j W_ij u_j of one frame staged in LDS: the lane chain, then the butterfly
__device__ __forceinline__ float nov_row_dot(const f32x4 (&w)[kNovQuads], const float* __restrict__ us,
                                             const int nq, const int lane) {
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < kNovQuads; ++q) {
        if (q < nq) {
            const f32x4 uv = *reinterpret_cast<const f32x4*>(&us[q * 256 + lane * 4]);
            acc = fmaf(w[q][0], uv[0], acc);
            acc = fmaf(w[q][1], uv[1], acc);
            acc = fmaf(w[q][2], uv[2], acc);
            acc = fmaf(w[q][3], uv[3], acc);
        }
    }
    return wave_sum(acc);
}

// stage frames b0 .. b0 + nb - 1 of u [B][F] in LDS
__device__ __forceinline__ void nov_stage_u(float (*us)[kMcMaxFeat], const float* __restrict__ u,
                                            const int F, const int b0, const int nb, const int tid) {
    for (int e = tid; e < nb * (F >> 2); e += 256) {
        const int b = e / (F >> 2), q = e - b * (F >> 2);
        *reinterpret_cast<f32x4*>(&us[b][q * 4]) =
            *reinterpret_cast<const f32x4*>(u + (size_t)(b0 + b) * F + q * 4);
    }
}

__global__ __launch_bounds__(256) void nov_u_kernel(const NoveltyScoreArgs a) {
    const int parts = a.F >> 8;
    const int b = blockIdx.x / parts, c = (blockIdx.x - b * parts) * 256 + threadIdx.x;
    const int k = command_branch(a.cmd, b, a.NC);
    const float v = pooled_feature(a.src, a.F, b, c);
    a.u[(size_t)b * a.F + c] = v - a.mean[(size_t)k * a.F + c];
    if (c == 0 && a.status && (a.cmd[b] < 0 || a.cmd[b] >= a.NC)) a.status[0] = 1;
}

__global__ __launch_bounds__(256) void nov_gemv_kernel(const NoveltyScoreArgs a) {
    __shared__ __align__(16) float us[kNovFrames][kMcMaxFeat];
    __shared__ float red[4][kNovFrames];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = a.F, nwg = F / kNovWgRows, g = blockIdx.x;
    const int nq = F >> 8;
    f32x4 w[2][kNovQuads];
#pragma unroll
    for (int r = 0; r < 2; ++r) nov_load_w(a.W, F, g + nwg * (2 * wave + r), lane, w[r]);
    for (int b0 = 0; b0 < a.B; b0 += kNovFrames) {
        const int nb = min(kNovFrames, a.B - b0);
        __syncthreads();
        nov_stage_u(us, a.u, F, b0, nb, tid);
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
            float y[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) y[r] = nov_row_dot(w[r], us[b], nq, lane);
            if (lane == 0) red[wave][b] = fmaf(y[1], y[1], y[0] * y[0]);
        }
        __syncthreads();
        if (tid < nb)
            a.part[(size_t)g * a.B + b0 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
}

// u = v - origin (pooling a feature map first); origin NULL: u = v
__global__ __launch_bounds__(256) void nov_u0_kernel(const NoveltyWhitenArgs a) {
    const int parts = a.F >> 8;
    const int b = blockIdx.x / parts, c = (blockIdx.x - b * parts) * 256 + threadIdx.x;
    const float v = pooled_feature(a.src, a.F, b, c);
    a.u[(size_t)b * a.F + c] = a.origin ? v - a.origin[c] : v;
}

// nov_gemv_kernel's product with y stored: workgroup (g, s) writes y[b][g + (F / 8) r], r = 0..7, for
// the frames b of slice s
__global__ __launch_bounds__(256) void nov_whiten_kernel(const NoveltyWhitenArgs a) {
    __shared__ __align__(16) float us[kNovFrames][kMcMaxFeat];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = a.F, nwg = F / kNovWgRows, g = blockIdx.x;
    const int nq = F >> 8;
    f32x4 w[2][kNovQuads];
#pragma unroll
    for (int r = 0; r < 2; ++r) nov_load_w(a.W, F, g + nwg * (2 * wave + r), lane, w[r]);
    // the frames split over gridDim.y in whole LDS chunks: a frame's y does not depend on the split
    const int ny = gridDim.y;
    const int per = ((a.B + ny - 1) / ny + kNovFrames - 1) / kNovFrames * kNovFrames;
    const int bend = min(a.B, ((int)blockIdx.y + 1) * per);
    for (int b0 = blockIdx.y * per; b0 < bend; b0 += kNovFrames) {
        const int nb = min(kNovFrames, bend - b0);
        __syncthreads();
        nov_stage_u(us, a.u, F, b0, nb, tid);
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const float y = nov_row_dot(w[r], us[b], nq, lane);
                if (lane == 0) a.y[(size_t)(b0 + b) * F + g + nwg * (2 * wave + r)] = y;
            }
        }
    }
}

__global__ __launch_bounds__(64) void nov_sum_kernel(const NoveltyScoreArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const int nwg = a.F / kNovWgRows;
    float s = 0.f;
    for (int g = 0; g < nwg; ++g) s += a.part[(size_t)g * a.B + b];
    a.d2[b] = s;
}

}  // namespace

size_t novelty_moments_doubles(int F, int NC) {
    return (size_t)NC * (F + 1) + (size_t)F * F;
}

size_t novelty_scratch_floats(int F, int batch) {
    return (size_t)batch * F + (size_t)(F / kNovWgRows) * batch;
}

int launch_novelty_moments(const NoveltyMomentsArgs& a, hipStream_t s) {
    CILRS_CHECK(a.F % kNovTile == 0 && a.F >= kNovTile && a.F <= kMcMaxFeat,
                "feature_moments: feature width %d", a.F);
    CILRS_CHECK(a.NC >= 1 && a.NC * kNovTile <= 512, "feature_moments: %d commands", a.NC);
    const int t = a.F / kNovTile;
    nov_moments_kernel<<<t * (t + 1) / 2, 256, 0, s>>>(a);
    CILRS_LAUNCH_CHECK();
    return 0;
}

int launch_novelty_score(NoveltyScoreArgs& a, float* scratch, hipStream_t s) {
    CILRS_CHECK(a.F % 256 == 0 && a.F >= 256 && a.F <= kMcMaxFeat, "feature_novelty: feature width %d",
                a.F);
    a.u = scratch;
    a.part = scratch + (size_t)a.B * a.F;
    nov_u_kernel<<<a.B * (a.F >> 8), 256, 0, s>>>(a);
    CILRS_LAUNCH_CHECK();
    nov_gemv_kernel<<<a.F / kNovWgRows, 256, 0, s>>>(a);
    CILRS_LAUNCH_CHECK();
    nov_sum_kernel<<<cdiv(a.B, 64), 64, 0, s>>>(a);
    CILRS_LAUNCH_CHECK();
    return 0;
}

int launch_novelty_whiten(const NoveltyWhitenArgs& a, hipStream_t s) {
    CILRS_CHECK(a.F % 256 == 0 && a.F >= 256 && a.F <= kMcMaxFeat, "feature_whiten: feature width %d",
                a.F);
    nov_u0_kernel<<<a.B * (a.F >> 8), 256, 0, s>>>(a);
    CILRS_LAUNCH_CHECK();
    if (a.W == nullptr) return 0;
    // a pool's worth of frames: enough workgroups for the chip (about eight per CU)
    const int wgs = a.F / kNovWgRows, split = max(1, min(cdiv(a.B, 64), 2048 / wgs));
    nov_whiten_kernel<<<dim3(wgs, split), 256, 0, s>>>(a);
    CILRS_LAUNCH_CHECK();
    return 0;
}

}  // namespace cilrs
