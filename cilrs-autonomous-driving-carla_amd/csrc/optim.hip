// AdamW (decoupled decay) and LAMB (per-tensor trust ratios) over the flat parameter arena.
// include/cilrs_hip.h "AdamW and LAMB" states the arithmetic; the reference has neither optimiser.
//
// Work decomposition: a chunk table built once on the host.  Every chunk is at most kChunkFloats
// floats of ONE segment (= one parameter tensor), counted from that segment's start, and is the work
// of one workgroup, whose thread t takes the chunk's quads t, t + 256, ...  A tensor's chunks, the
// order of its elements inside a thread and the reduction tree are therefore a function of the
// tensor's length alone: its new p, m, v and its trust ratio do not depend on where it sits in the
// arena or on which run of segments a call covers.  A 64-float BatchNorm tensor is a chunk of 16
// quads -- one workgroup, 16 busy lanes; there are 108 such tensors against 5,500 full chunks in the
// ResNet-34 arena.
//
// LAMB is three launches on one stream: moments + partial sums (p, g, m, v -> m, v, two doubles per
// chunk), a finalise (one wave per segment adds that segment's partials in a fixed order and writes
// float(lr * r_s)), and the apply pass (p, m, v -> p) that recomputes u through the same function
// (lamb_u, compiled without FMA contraction so that both passes round it alike).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/cilrs_hip.h"
#include "common.h"

namespace cilrs {
namespace {

constexpr int kChunkFloats = 4096;                     // 256 threads x 4 quads
constexpr int kOptimGroupsMax = 8;
constexpr unsigned kTableMagic = 0x4f50544du;

// kernel-argument table of the <= 8 learning-rate / step-count groups; seg_end = absolute segment
// index one past the group's last segment
struct OptimGroups {
    int n;
    unsigned seg_end[kOptimGroupsMax];
    float a[kOptimGroupsMax];          // AdamW: -lr/bc1            LAMB: 1/bc1
    float bc2_sqrt[kOptimGroupsMax];
    float c[kOptimGroupsMax];          // AdamW: 1 - lr*wd          LAMB: unused
    double lr[kOptimGroupsMax];        // LAMB finalise
};

// device table: uint4 seg[nseg] = {first chunk, chunk count, flags, 0}, then
//               uint4 chunk[nchunks] = {first quad, quads, segment, 0}
__device__ __forceinline__ int group_of(const OptimGroups& t, const unsigned seg) {
    int r = 0;
    while (r + 1 < t.n && seg >= t.seg_end[r]) ++r;
    return r;
}

__global__ __launch_bounds__(256) void adamw_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, const uint4* __restrict__ segs, const uint4* __restrict__ chunks,
    const unsigned chunk0, const float omb1, const float beta2, const float omb2, const float eps,
    const OptimGroups t, const float* __restrict__ gscale_ptr, const float gscale_const) {
    const float gs = gscale_ptr ? gscale_ptr[1] * gscale_const : gscale_const;
    const uint4 ck = chunks[chunk0 + blockIdx.x];
    const unsigned flags = segs[ck.z].z;
    const int r = group_of(t, ck.z);
    const float neg_step_size = t.a[r], bc2_sqrt = t.bc2_sqrt[r];
    const float decay = (flags & CILRS_SEG_NO_DECAY) ? 1.0f : t.c[r];
    for (unsigned q = threadIdx.x; q < ck.y; q += 256) {
        const size_t i = ((size_t)ck.x + q) * 4;
        f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
        f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
        f32x4 mv = *reinterpret_cast<const f32x4*>(m + i);
        f32x4 vv = *reinterpret_cast<const f32x4*>(v + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gg = gv[e] * gs;
            pv[e] = pv[e] * decay;                             // param.mul_(1 - lr * wd)
            mv[e] = mv[e] + omb1 * (gg - mv[e]);
            vv[e] = vv[e] * beta2 + (omb2 * gg) * gg;
            const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
            pv[e] = pv[e] + (neg_step_size * mv[e]) / denom;
        }
        *reinterpret_cast<f32x4*>(p + i) = pv;
        *reinterpret_cast<f32x4*>(m + i) = mv;
        *reinterpret_cast<f32x4*>(v + i) = vv;
    }
}

// u of one element, from the UPDATED moments and the parameter before the step.  Both LAMB passes
// call it; separately rounded operations, so that the two evaluations agree bit for bit whatever the
// compiler does with the code around them.
__device__ __forceinline__ float lamb_u(const float m, const float v, const float p,
                                        const float inv_bc1, const float bc2_sqrt, const float eps,
                                        const float wd) {
#pragma clang fp contract(off)
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    const float q = (m * inv_bc1) / denom;
    const float d = wd * p;
    return q + d;
}

__global__ __launch_bounds__(256) void lamb_moments_kernel(
    const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, const uint4* __restrict__ segs, const uint4* __restrict__ chunks,
    const unsigned chunk0, const float omb1, const float beta2, const float omb2, const float eps,
    const float wd, const OptimGroups t, const float* __restrict__ gscale_ptr,
    const float gscale_const, double* __restrict__ partial) {
    __shared__ double red[2][256];
    const float gs = gscale_ptr ? gscale_ptr[1] * gscale_const : gscale_const;
    const unsigned c = chunk0 + blockIdx.x;
    const uint4 ck = chunks[c];
    const unsigned flags = segs[ck.z].z;
    const int r = group_of(t, ck.z);
    const float inv_bc1 = t.a[r], bc2_sqrt = t.bc2_sqrt[r];
    const float wd_s = (flags & CILRS_SEG_NO_DECAY) ? 0.0f : wd;
    double sp = 0.0, su = 0.0;
    for (unsigned q = threadIdx.x; q < ck.y; q += 256) {
        const size_t i = ((size_t)ck.x + q) * 4;
        const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
        f32x4 mv = *reinterpret_cast<const f32x4*>(m + i);
        f32x4 vv = *reinterpret_cast<const f32x4*>(v + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gg = gv[e] * gs;
            mv[e] = mv[e] + omb1 * (gg - mv[e]);
            vv[e] = vv[e] * beta2 + (omb2 * gg) * gg;
            const float u = lamb_u(mv[e], vv[e], pv[e], inv_bc1, bc2_sqrt, eps, wd_s);
            sp += (double)pv[e] * pv[e];
            su += (double)u * u;
        }
        *reinterpret_cast<f32x4*>(m + i) = mv;
        *reinterpret_cast<f32x4*>(v + i) = vv;
    }
    red[0][threadIdx.x] = sp;
    red[1][threadIdx.x] = su;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[2 * (size_t)c] = red[0][0];
        partial[2 * (size_t)c + 1] = red[1][0];
    }
}

// one wave per segment of the run: lane l adds the segment's chunk sums l, l + 64, ... in table
// order, a fixed tree adds the 64 lanes; then r_s and float(lr * r_s).  (One THREAD per segment, the
// first form, took 0.092 ms of a 0.232 ms step: layer4's 3x3 convolutions are 576 chunks each.)
__global__ __launch_bounds__(64) void lamb_finalize_kernel(
    const uint4* __restrict__ segs, const unsigned seg0, const double* __restrict__ partial,
    const OptimGroups t, const double trust_clip, float* __restrict__ stepf,
    float* __restrict__ ratio_out) {
    __shared__ double red[2][64];
    const unsigned seg = seg0 + blockIdx.x;
    const uint4 sg = segs[seg];
    const bool adapt = !(sg.z & CILRS_SEG_NO_ADAPT);
    double sp = 0.0, su = 0.0;
    if (adapt) {
        for (unsigned c = sg.x + threadIdx.x; c < sg.x + sg.y; c += 64) {
            sp += partial[2 * (size_t)c];
            su += partial[2 * (size_t)c + 1];
        }
    }
    red[0][threadIdx.x] = sp;
    red[1][threadIdx.x] = su;
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double lr = t.lr[group_of(t, seg)];
    double ratio = 1.0;
    if (adapt) {
        double np = sqrt(red[0][0]);
        const double nu = sqrt(red[1][0]);
        if (trust_clip > 0.0 && np > trust_clip) np = trust_clip;
        if (np > 0.0 && nu > 0.0) ratio = np / nu;
    }
    stepf[seg] = (float)(lr * ratio);
    if (ratio_out) ratio_out[seg] = (float)ratio;
}

__global__ __launch_bounds__(256) void lamb_apply_kernel(
    float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
    const uint4* __restrict__ segs, const uint4* __restrict__ chunks, const unsigned chunk0,
    const float eps, const float wd, const OptimGroups t, const float* __restrict__ stepf) {
    const uint4 ck = chunks[chunk0 + blockIdx.x];
    const unsigned flags = segs[ck.z].z;
    const int r = group_of(t, ck.z);
    const float inv_bc1 = t.a[r], bc2_sqrt = t.bc2_sqrt[r];
    const float wd_s = (flags & CILRS_SEG_NO_DECAY) ? 0.0f : wd;
    const float step = stepf[ck.z];
    for (unsigned q = threadIdx.x; q < ck.y; q += 256) {
        const size_t i = ((size_t)ck.x + q) * 4;
        f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
        const f32x4 mv = *reinterpret_cast<const f32x4*>(m + i);
        const f32x4 vv = *reinterpret_cast<const f32x4*>(v + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float u = lamb_u(mv[e], vv[e], pv[e], inv_bc1, bc2_sqrt, eps, wd_s);
            pv[e] = pv[e] - step * u;
        }
        *reinterpret_cast<f32x4*>(p + i) = pv;
    }
}

bool aligned(const void* q, const uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; }

// chunks of a table of `nseg` segments; 0 where the ends are unusable
size_t count_chunks(const size_t* ends, const int nseg) {
    size_t prev = 0, chunks = 0;
    for (int s = 0; s < nseg; ++s) {
        if (ends[s] <= prev) return 0;
        chunks += (ends[s] - prev + kChunkFloats - 1) / kChunkFloats;
        prev = ends[s];
    }
    return chunks;
}

}  // namespace
}  // namespace cilrs

// host mirror of a table: what the step entry validates against without touching the device
struct cilrs_optim_table {
    unsigned magic;
    size_t n;
    std::vector<size_t> ends;              // [nseg]
    std::vector<unsigned> first_chunk;     // [nseg + 1]
    std::vector<uint4> image;              // what the device holds
    const uint4* dev;
};

using namespace cilrs;

extern "C" {

int cilrs_optim_chunk_floats(void) { return kChunkFloats; }

size_t cilrs_optim_table_bytes(const size_t* ends, int nseg) {
    if (!ends || nseg < 1) return 0;
    const size_t chunks = count_chunks(ends, nseg);
    return chunks ? (chunks + (size_t)nseg) * sizeof(uint4) : 0;
}

int cilrs_optim_table_create(const size_t* ends, const int* flags, int nseg, size_t n,
                             void* device_table, size_t device_bytes, void* stream,
                             cilrs_optim_table** out) {
    CILRS_CHECK(out != nullptr, "optim table: out is NULL");
    *out = nullptr;
    CILRS_CHECK(ends && flags, "optim table: NULL ends / flags");
    CILRS_CHECK(nseg >= 1, "optim table: nseg %d < 1", nseg);
    CILRS_CHECK(device_table != nullptr, "optim table: NULL device_table");
    CILRS_CHECK(aligned(device_table, 16), "optim table: device_table must be 16-byte aligned");
    CILRS_CHECK(n % 4 == 0 && n / 4 < (1ull << 32), "optim table: n must be a multiple of 4 below 2^34");
    size_t prev = 0;
    for (int s = 0; s < nseg; ++s) {
        CILRS_CHECK(ends[s] > prev, "optim table: ends must increase (ends[%d] = %zu after %zu)", s,
                    ends[s], prev);
        CILRS_CHECK(ends[s] % 4 == 0, "optim table: ends[%d] = %zu is not a multiple of 4", s,
                    ends[s]);
        CILRS_CHECK((flags[s] & ~(CILRS_SEG_NO_DECAY | CILRS_SEG_NO_ADAPT)) == 0,
                    "optim table: flags[%d] = 0x%x out of range", s, (unsigned)flags[s]);
        prev = ends[s];
    }
    CILRS_CHECK(prev == n, "optim table: the last end %zu must equal n = %zu", prev, n);
    const size_t chunks = count_chunks(ends, nseg);
    CILRS_CHECK(chunks < (1ull << 31), "optim table: too many chunks");
    const size_t bytes = (chunks + (size_t)nseg) * sizeof(uint4);
    CILRS_CHECK(device_bytes >= bytes, "optim table: device_bytes %zu < %zu", device_bytes, bytes);
    cilrs_optim_table* t = new cilrs_optim_table;
    t->magic = kTableMagic;
    t->n = n;
    t->ends.assign(ends, ends + nseg);
    t->first_chunk.resize(nseg + 1);
    t->image.resize(chunks + nseg);
    t->dev = reinterpret_cast<const uint4*>(device_table);
    unsigned c = 0;
    prev = 0;
    for (int s = 0; s < nseg; ++s) {
        t->first_chunk[s] = c;
        const unsigned first = c;
        for (size_t b = prev; b < ends[s]; b += kChunkFloats, ++c) {
            const size_t e = b + kChunkFloats < ends[s] ? b + kChunkFloats : ends[s];
            t->image[nseg + c] = make_uint4((unsigned)(b / 4), (unsigned)((e - b) / 4), (unsigned)s, 0u);
        }
        t->image[s] = make_uint4(first, c - first, (unsigned)flags[s], 0u);
        prev = ends[s];
    }
    t->first_chunk[nseg] = c;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(device_table, t->image.data(), bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        set_error("optim table: upload failed: %s", hipGetErrorString(e));
        delete t;
        return 1;
    }
    *out = t;
    return 0;
}

void cilrs_optim_table_destroy(cilrs_optim_table* table) {
    if (table && table->magic == kTableMagic) {
        table->magic = 0;
        delete table;
    }
}

size_t cilrs_optim_scratch_bytes(const cilrs_optim_table* table) {
    if (!table || table->magic != kTableMagic) return 0;
    return (size_t)table->first_chunk.back() * 2 * sizeof(double) + table->ends.size() * sizeof(float);
}

int cilrs_optim_step(int kind, const cilrs_optim_table* table, int first_seg, int count,
                     float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                     int ngroups, const size_t* group_ends, const double* lrs, const int64_t* steps,
                     double beta1, double beta2, double eps, double weight_decay, double trust_clip,
                     const float* clip_out2, float grad_scale, void* scratch, float* ratio_out,
                     void* stream) {
    CILRS_CHECK(table != nullptr, "optim: NULL table");
    CILRS_CHECK(table->magic == kTableMagic, "optim: table is not a live cilrs_optim_table");
    CILRS_CHECK(kind == CILRS_OPTIM_ADAMW || kind == CILRS_OPTIM_LAMB, "optim: kind %d (1 AdamW, 2 LAMB)",
                kind);
    const int nseg = (int)table->ends.size();
    CILRS_CHECK(first_seg >= 0 && count >= 1 && first_seg <= nseg - count,
                "optim: segments [first_seg %d, +count %d) outside the table's %d", first_seg, count,
                nseg);
    CILRS_CHECK(params && grads && exp_avg && exp_avg_sq, "optim: NULL params / grads / moments");
    CILRS_CHECK(aligned(params, 16) && aligned(grads, 16) && aligned(exp_avg, 16) &&
                    aligned(exp_avg_sq, 16),
                "optim: params, grads and moments pointers must be 16-byte aligned");
    CILRS_CHECK(ngroups >= 1 && ngroups <= kOptimGroupsMax && group_ends && lrs && steps,
                "optim: ngroups 1..%d with group_ends, lrs and steps", kOptimGroupsMax);
    CILRS_CHECK(eps > 0.0, "optim: eps must be positive (the padding floats stay zero through 0 / eps)");
    CILRS_CHECK(trust_clip >= 0.0, "optim: trust_clip %g is negative", trust_clip);
    OptimGroups t = {};
    t.n = ngroups;
    int seg = first_seg;                                   // first segment of the current group
    const int seg_stop = first_seg + count;
    for (int r = 0; r < ngroups; ++r) {
        CILRS_CHECK(steps[r] >= 1, "optim: steps[%d] = %lld, step must be >= 1", r, (long long)steps[r]);
        int e = seg;
        while (e < seg_stop && table->ends[e] < group_ends[r]) ++e;
        CILRS_CHECK(e < seg_stop && table->ends[e] == group_ends[r],
                    "optim: group_ends[%d] = %zu is not a later segment end of the run", r,
                    group_ends[r]);
        seg = e + 1;
        t.seg_end[r] = (unsigned)seg;
        const double bc1 = 1.0 - pow(beta1, (double)steps[r]);
        const double bc2 = 1.0 - pow(beta2, (double)steps[r]);
        t.bc2_sqrt[r] = (float)sqrt(bc2);
        t.lr[r] = lrs[r];
        if (kind == CILRS_OPTIM_ADAMW) {
            t.a[r] = (float)(-(lrs[r] / bc1));
            t.c[r] = (float)(1.0 - lrs[r] * weight_decay);
        } else {
            t.a[r] = (float)(1.0 / bc1);
        }
    }
    CILRS_CHECK(seg == seg_stop, "optim: the last group end must be the end of segment %d",
                seg_stop - 1);
    if (kind == CILRS_OPTIM_LAMB) {
        CILRS_CHECK(scratch != nullptr, "optim: LAMB needs scratch");
        CILRS_CHECK(aligned(scratch, 16), "optim: scratch must be 16-byte aligned");
    }
    CILRS_CHECK(aligned(ratio_out, 4), "optim: ratio_out must be 4-byte aligned");

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint4* segs = table->dev;
    const uint4* chunks = table->dev + nseg;
    const unsigned chunk0 = table->first_chunk[first_seg];
    const unsigned nchunks = table->first_chunk[seg_stop] - chunk0;
    const float omb1 = (float)(1.0 - beta1), b2 = (float)beta2, omb2 = (float)(1.0 - beta2);
    if (kind == CILRS_OPTIM_ADAMW) {
        adamw_kernel<<<nchunks, 256, 0, s>>>(params, grads, exp_avg, exp_avg_sq, segs, chunks, chunk0,
                                             omb1, b2, omb2, (float)eps, t, clip_out2, grad_scale);
        CILRS_LAUNCH_CHECK();
        return 0;
    }
    double* partial = reinterpret_cast<double*>(scratch);
    float* stepf = reinterpret_cast<float*>(partial + 2 * (size_t)table->first_chunk[nseg]);
    lamb_moments_kernel<<<nchunks, 256, 0, s>>>(params, grads, exp_avg, exp_avg_sq, segs, chunks,
                                                chunk0, omb1, b2, omb2, (float)eps,
                                                (float)weight_decay, t, clip_out2, grad_scale,
                                                partial);
    CILRS_LAUNCH_CHECK();
    lamb_finalize_kernel<<<count, 64, 0, s>>>(segs, (unsigned)first_seg, partial, t, trust_clip, stepf,
                                              ratio_out);
    CILRS_LAUNCH_CHECK();
    lamb_apply_kernel<<<nchunks, 256, 0, s>>>(params, exp_avg, exp_avg_sq, segs, chunks, chunk0,
                                              (float)eps, (float)weight_decay, t, stepf);
    CILRS_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
