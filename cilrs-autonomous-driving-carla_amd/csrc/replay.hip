// Closed-loop replay of recorded drives (include/cilrs_hip.h "closed-loop replay", where every
// step is defined; evaluate.replay; tests/_replay.py mirrors the arithmetic in float64 numpy).
//
// The predicted steer of tick k-1 moves a kinematic bicycle relative to the recorded path, and the
// frame of tick k is then shown from where the car now is: the view record this kernel writes is
// what data.view_records computes on the host, and cilrs_batch_assemble_view reads it from device
// memory in the next launch.  So one tick is three launches -- this one, the assemble, the forward
// -- and the host never waits for the controls.
//
// One thread per segment, everything in double, no fused multiply-add, no LDS, no cross-lane work
// and no atomics: a segment is a few hundred flops a tick against a 3.6 ms forward, and what matters
// is that its result is the definition's and does not depend on where it sits in the batch.
#include "common.h"

#include <math.h>
#include <vector>

namespace cilrs {
namespace {

#pragma clang fp contract(off)      // keep a*b+c as two roundings: numpy-identical arithmetic

constexpr int kReplayMaxTaps = 8;
// state row
constexpr int kStE = 0, kStPsi = 1, kStNHist = 2, kStHist = 3, kStPrev = 11, kStHasPrev = 12,
              kStRecoverOpen = 13, kStLateral0 = 14, kStYaw0 = 15, kStStart = 16, kReplayState = 17;
// metrics row
constexpr int kMtTicks = 0, kMtLateral = 1, kMtYaw = 2, kMtNonfinite = 3, kMtSumAbsE = 4,
              kMtSumE2 = 5, kMtMaxAbsE = 6, kMtSumAbsPsi = 7, kMtMaxAbsPsi = 8, kMtSumLabel = 9,
              kMtSumCorrected = 10, kMtSumDs2 = 11, kMtRecoverTick = 12, kMtSteerTicks = 13,
              kReplayMetrics = 14;
constexpr int kFlagLateral = 1, kFlagYaw = 2, kFlagNonfinite = 4, kFlagOn = 8;

__device__ __forceinline__ double clip1(double v) { return fmin(fmax(v, -1.0), 1.0); }

// data.steer_correction
__device__ double steer_delta(const cilrs_replay_config& c, double e, double psi, double v_n) {
    const double v = v_n * c.speed_unit_ms;
    const double look = fmax(c.lookahead_s * v, c.min_lookahead_m);
    const double yt = 0.0 - e * cos(psi) - look * sin(psi);
    return atan(c.wheelbase_m * 2.0 * yt / (look * look)) / c.max_wheel_rad;
}

// out = K * Bm * K^-1 divided by (its third row) . (cx, cy, 1), cast to float32; exactly the
// identity where Bm is (data.view_records: the products run left to right, sums in index order)
__device__ void homography(const cilrs_replay_config& c, const double Bm[9], float out[9]) {
    bool ident = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) ident = ident && (Bm[i] == ((i % 4 == 0) ? 1.0 : 0.0));
    if (ident) {
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] = (i % 4 == 0) ? 1.f : 0.f;
        return;
    }
    const double K[9] = {c.fx, 0.0, c.cx, 0.0, c.fy, c.cy, 0.0, 0.0, 1.0};
    const double Ki[9] = {1.0 / c.fx, 0.0, -c.cx / c.fx, 0.0, 1.0 / c.fy, -c.cy / c.fy,
                          0.0, 0.0, 1.0};
    double KB[9], M[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            KB[i * 3 + j] = (K[i * 3] * Bm[j] + K[i * 3 + 1] * Bm[3 + j]) + K[i * 3 + 2] * Bm[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            M[i * 3 + j] = (KB[i * 3] * Ki[j] + KB[i * 3 + 1] * Ki[3 + j]) + KB[i * 3 + 2] * Ki[6 + j];
    const double norm = (M[6] * c.cx + M[7] * c.cy) + M[8] * 1.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = (float)(M[i] / norm);
}

__device__ void render(const cilrs_replay_config& c, double e, double psi, double v_n,
                       cilrs_view_params* out) {
    cilrs_view_params r;
    r.reserved = 0;
    if (e == 0.0 && psi == 0.0) {                    // data.identity_view, byte for byte
        r.on = 0;
        r.split_row = 0.f;
#pragma unroll
        for (int i = 0; i < 9; ++i) r.far[i] = r.ground[i] = (i % 4 == 0) ? 1.f : 0.f;
        r.steer_delta = r.lateral_m = r.yaw_rad = 0.f;
    } else {
        const double cs = cos(psi), sn = sin(psi);
        double Bm[9] = {cs, 0.0, sn, 0.0, 1.0, 0.0, -sn, 0.0, cs};
        homography(c, Bm, r.far);
        Bm[1] = e / c.height_m;
        homography(c, Bm, r.ground);
        r.on = 1;
        r.split_row = (float)c.cy;
        r.steer_delta = (float)steer_delta(c, e, psi, v_n);
        r.lateral_m = (float)e;
        r.yaw_rad = (float)psi;
    }
    *out = r;
}

struct ReplayArgs {
    cilrs_replay_config cfg;
    int B, tick, advance, render;
    long long n_frames;
    const float* controls;
    const float* speed;
    const float* targets;
    double* state;
    double* metrics;
    long long* index;
    cilrs_view_params* view;
    double* trace_state;
    float* trace_steer;
    unsigned char* trace_flags;
};

__global__ __launch_bounds__(64) void replay_step_kernel(const ReplayArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const cilrs_replay_config& c = a.cfg;
    double* st = a.state + (size_t)b * kReplayState;
    double* mt = a.metrics + (size_t)b * kReplayMetrics;
    const long long start = (long long)st[kStStart];
    // every frame this launch reads lies inside the dataset, or the segment is left alone
    const long long first = start + a.tick - (a.advance ? 1 : 0);
    const long long last = start + a.tick - (a.render ? 0 : 1);
    if (first < 0 || last >= a.n_frames) return;
    double e = st[kStE], psi = st[kStPsi];

    if (a.advance) {
        const long long i = start + a.tick - 1;
        const double v_n = (double)a.speed[i];
        const double sx = clip1((double)a.targets[i * 3]);
        const double raw = (double)a.controls[(size_t)b * 3];
        const bool on = !(e == 0.0 && psi == 0.0);
        const double delta = on ? steer_delta(c, e, psi, v_n) : 0.0;
        const double ae = fabs(e), ap = fabs(psi);
        mt[kMtTicks] += 1.0;
        mt[kMtSumAbsE] += ae;
        mt[kMtSumE2] += e * e;
        mt[kMtMaxAbsE] = fmax(mt[kMtMaxAbsE], ae);
        mt[kMtSumAbsPsi] += ap;
        mt[kMtMaxAbsPsi] = fmax(mt[kMtMaxAbsPsi], ap);
        if (st[kStRecoverOpen] != 0.0 && ae < c.recover_m) {
            mt[kMtRecoverTick] = (double)(a.tick - 1);
            st[kStRecoverOpen] = 0.0;
        }
        if (a.trace_state) {
            a.trace_state[(size_t)b * 2] = e;
            a.trace_state[(size_t)b * 2 + 1] = psi;
        }
        int flags = on ? kFlagOn : 0;
        bool intervene = false;
        double s = __builtin_nan("");
        if (!isfinite(raw)) {
            mt[kMtNonfinite] += 1.0;
            flags |= kFlagNonfinite;
            intervene = true;
        } else {
            int n = (int)st[kStNHist];
            n = n < 0 ? 0 : (n > c.ntaps ? c.ntaps : n);
            if (c.ntaps > 0) {
                if (n == c.ntaps) {
                    for (int j = 1; j < n; ++j) st[kStHist + j - 1] = st[kStHist + j];
                    --n;
                }
                st[kStHist + n] = raw;
                ++n;
            }
            if (c.ntaps == 0 || n == 1) {
                s = raw;
            } else {
                double num = 0.0, den = 0.0;
                for (int j = 0; j < n; ++j) {
                    const double w = c.taps[c.ntaps - n + j];
                    num += w * st[kStHist + j];
                    den += w;
                }
                s = num / den;
            }
            st[kStNHist] = (double)n;
            s = clip1(s);
            mt[kMtSteerTicks] += 1.0;
            mt[kMtSumLabel] += fabs(s - sx);
            mt[kMtSumCorrected] += fabs(s - clip1(sx + delta));
            if (st[kStHasPrev] != 0.0) {
                const double d = s - st[kStPrev];
                mt[kMtSumDs2] += d * d;
            }
            st[kStPrev] = s;
            st[kStHasPrev] = 1.0;
            if (c.closed_loop) {
                const double ds = (v_n * c.speed_unit_ms) * c.dt_s;
                const double e2 = e + ds * sin(psi);
                const double p2 = psi + ds * (tan(s * c.max_wheel_rad) - tan(sx * c.max_wheel_rad))
                                            / c.wheelbase_m;
                if (!(isfinite(e2) && isfinite(p2))) {
                    mt[kMtNonfinite] += 1.0;
                    flags |= kFlagNonfinite;
                    intervene = true;
                } else if (fabs(e2) > c.max_lateral_m) {
                    mt[kMtLateral] += 1.0;
                    flags |= kFlagLateral;
                    intervene = true;
                } else if (fabs(p2) > c.max_yaw_rad) {
                    mt[kMtYaw] += 1.0;
                    flags |= kFlagYaw;
                    intervene = true;
                } else {
                    e = e2;
                    psi = p2;
                }
            }
        }
        if (intervene) {
            if (c.closed_loop) e = psi = 0.0;
            st[kStNHist] = 0.0;
            st[kStHasPrev] = 0.0;
            st[kStRecoverOpen] = 0.0;
        }
        if (a.trace_steer) {
            a.trace_steer[(size_t)b * 2] = (float)raw;
            a.trace_steer[(size_t)b * 2 + 1] = (float)s;
        }
        if (a.trace_flags) a.trace_flags[b] = (unsigned char)flags;
    }

    if (a.render) {
        if (!(isfinite(e) && isfinite(psi))) e = psi = 0.0;      // never a record from such a state
        const long long i = start + a.tick;
        a.index[b] = i;
        render(c, e, psi, (double)a.speed[i], a.view + b);
    }
    st[kStE] = e;
    st[kStPsi] = psi;
}

bool positive(double v) { return std::isfinite(v) && v > 0.0; }

int check_config(const char* who, const cilrs_replay_config* c) {
    CILRS_CHECK(c != nullptr, "%s: NULL configuration", who);
    CILRS_CHECK(positive(c->dt_s) && positive(c->speed_unit_ms) && positive(c->wheelbase_m) &&
                positive(c->max_wheel_rad) && positive(c->min_lookahead_m) &&
                std::isfinite(c->lookahead_s) && c->lookahead_s >= 0.0,
                "%s: dt_s, speed_unit_ms, wheelbase_m, max_wheel_rad and min_lookahead_m must be "
                "finite and positive, lookahead_s finite and non-negative", who);
    CILRS_CHECK(positive(c->fx) && positive(c->fy) && std::isfinite(c->cx) && std::isfinite(c->cy) &&
                positive(c->height_m), "%s: bad camera", who);
    CILRS_CHECK(positive(c->max_lateral_m) && positive(c->max_yaw_rad) && c->max_yaw_rad < 1.5 &&
                std::isfinite(c->recover_m) && c->recover_m >= 0.0,
                "%s: max_lateral_m and max_yaw_rad (below 1.5 rad) must be finite and positive, "
                "recover_m finite and non-negative", who);
    CILRS_CHECK(c->ntaps >= 0 && c->ntaps <= kReplayMaxTaps, "%s: %d filter taps, at most %d", who,
                c->ntaps, kReplayMaxTaps);
    for (int j = 0; j < c->ntaps; ++j)
        CILRS_CHECK(std::isfinite(c->taps[j]) && c->taps[j] >= 0.0,
                    "%s: filter taps must be finite and non-negative", who);
    CILRS_CHECK(c->ntaps == 0 || c->taps[c->ntaps - 1] > 0.0,
                "%s: the newest filter tap must be positive", who);
    return 0;
}

int launch_replay(const ReplayArgs& a, hipStream_t s) {
    replay_step_kernel<<<cdiv(a.B, 64), 64, 0, s>>>(a);
    CILRS_LAUNCH_CHECK();
    return 0;
}

}  // namespace
}  // namespace cilrs

using namespace cilrs;

extern "C" {

int cilrs_replay_state_doubles(void) { return kReplayState; }
int cilrs_replay_metric_doubles(void) { return kReplayMetrics; }

int cilrs_replay_begin(const cilrs_replay_config* cfg, int batch, int ticks, int64_t n_frames,
                       const int64_t* start, const double* lateral0, const double* yaw0,
                       const float* speed, double* state, double* metrics, int64_t* index,
                       cilrs_view_params* view, void* stream) {
    static_assert(sizeof(cilrs_replay_config) == 184, "cilrs_replay_config layout");
    if (check_config("replay_begin", cfg)) return 1;
    CILRS_CHECK(start && lateral0 && yaw0 && speed && state && metrics && index && view,
                "replay_begin: NULL argument");
    CILRS_CHECK(batch >= 1, "replay_begin: batch must be at least 1");
    CILRS_CHECK(ticks >= 1, "replay_begin: ticks must be at least 1");
    CILRS_CHECK(n_frames >= 1, "replay_begin: empty dataset");
    for (int b = 0; b < batch; ++b) {
        CILRS_CHECK(start[b] >= 0 && start[b] <= n_frames - ticks,
                    "replay_begin: segment %d covers frames [%lld, %lld), the dataset has %lld", b,
                    (long long)start[b], (long long)start[b] + ticks, (long long)n_frames);
        CILRS_CHECK(std::isfinite(lateral0[b]) && std::isfinite(yaw0[b]) &&
                    fabs(lateral0[b]) <= cfg->max_lateral_m && fabs(yaw0[b]) <= cfg->max_yaw_rad,
                    "replay_begin: segment %d starts at (%g m, %g rad), outside the box "
                    "(+-%g m, +-%g rad)", b, lateral0[b], yaw0[b], cfg->max_lateral_m,
                    cfg->max_yaw_rad);
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    std::vector<double> host((size_t)batch * (kReplayState + kReplayMetrics), 0.0);
    double* hm = host.data() + (size_t)batch * kReplayState;
    for (int b = 0; b < batch; ++b) {
        double* st = host.data() + (size_t)b * kReplayState;
        st[kStE] = st[kStLateral0] = lateral0[b];
        st[kStPsi] = st[kStYaw0] = yaw0[b];
        st[kStRecoverOpen] = fabs(lateral0[b]) >= cfg->recover_m ? 1.0 : 0.0;
        st[kStStart] = (double)start[b];
        hm[(size_t)b * kReplayMetrics + kMtRecoverTick] = -1.0;
    }
    CILRS_HIP(hipMemcpyAsync(state, host.data(), sizeof(double) * batch * kReplayState,
                             hipMemcpyHostToDevice, s));
    CILRS_HIP(hipMemcpyAsync(metrics, hm, sizeof(double) * batch * kReplayMetrics,
                             hipMemcpyHostToDevice, s));
    CILRS_HIP(hipStreamSynchronize(s));          // `host` goes away with this call
    ReplayArgs a{};
    a.cfg = *cfg;
    a.B = batch; a.tick = 0; a.advance = 0; a.render = 1;
    a.n_frames = n_frames;
    a.speed = speed;
    a.state = state; a.metrics = metrics;
    a.index = reinterpret_cast<long long*>(index);
    a.view = view;
    return launch_replay(a, s);
}

static int replay_advance(const char* who, const cilrs_replay_config* cfg, int batch, int tick,
                          bool render, const float* controls, const float* speed,
                          const float* targets, int64_t n_frames, double* state, double* metrics,
                          int64_t* index, cilrs_view_params* view, double* trace_state,
                          float* trace_steer, uint8_t* trace_flags, void* stream) {
    if (check_config(who, cfg)) return 1;
    CILRS_CHECK(controls && speed && targets && state && metrics && (!render || (index && view)),
                "%s: NULL argument", who);
    CILRS_CHECK(batch >= 1, "%s: batch must be at least 1", who);
    CILRS_CHECK(tick >= 1, "%s: tick must be at least 1", who);
    CILRS_CHECK(n_frames >= 1, "%s: empty dataset", who);
    ReplayArgs a{};
    a.cfg = *cfg;
    a.B = batch; a.tick = tick; a.advance = 1; a.render = render ? 1 : 0;
    a.n_frames = n_frames;
    a.controls = controls; a.speed = speed; a.targets = targets;
    a.state = state; a.metrics = metrics;
    a.index = reinterpret_cast<long long*>(index);
    a.view = view;
    a.trace_state = trace_state; a.trace_steer = trace_steer; a.trace_flags = trace_flags;
    return launch_replay(a, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_replay_step(const cilrs_replay_config* cfg, int batch, int tick, const float* controls,
                      const float* speed, const float* targets, int64_t n_frames, double* state,
                      double* metrics, int64_t* index, cilrs_view_params* view,
                      double* trace_state, float* trace_steer, uint8_t* trace_flags, void* stream) {
    return replay_advance("replay_step", cfg, batch, tick, true, controls, speed, targets, n_frames,
                          state, metrics, index, view, trace_state, trace_steer, trace_flags, stream);
}

int cilrs_replay_finish(const cilrs_replay_config* cfg, int batch, int ticks, const float* controls,
                        const float* speed, const float* targets, int64_t n_frames, double* state,
                        double* metrics, double* trace_state, float* trace_steer,
                        uint8_t* trace_flags, void* stream) {
    return replay_advance("replay_finish", cfg, batch, ticks, false, controls, speed, targets,
                          n_frames, state, metrics, nullptr, nullptr, trace_state, trace_steer,
                          trace_flags, stream);
}

}  // extern "C"
