// Network plan + C-ABI of the CILRS engine.
//
// The plan is the MI355X-side restatement of the graph the reference builds in
// CILRS.__init__/forward (model/autonomous_drive.py:361-399): ResNet-34 trunk (torchvision
// BasicBlock stacks [3,4,6,3]) -> 512-d feature; speed encoder 1->128->128; concat 640; four
// command branches 640->256->256->3 (all evaluated, then gathered by `command`); speed head
// 512->256->256->1.  Parameters live in ONE flat fp32 arena in nn.Module.parameters() order
// (conv weights OHWI); gradients / Adam moments use the same layout, so clip + Adam are single
// launches and data-parallel all-reduce works on contiguous ranges.
#include "common.h"
#include "../../include/cilrs_hip.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

namespace cilrs {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* last_error() { return g_err; }

static int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    return dev;
}
int device_cus() {
    static int cus[64] = {};
    const int dev = current_device();
    if (cus[dev] == 0) {
        hipDeviceProp_t p;
        cus[dev] = (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0)
                       ? p.multiProcessorCount : 256;
    }
    return cus[dev];
}
int set_max_dynamic_lds(const void* kernel, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;     // (kernel, device)
    const std::pair<const void*, int> key(kernel, current_device());
    std::lock_guard<std::mutex> lock(mu);
    if (done.count(key)) return 0;
    CILRS_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.insert(key);
    return 0;
}

#ifdef CILRS_EXPERIMENTS
int experiment_env(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}
#endif
// the run-time switches (common.h); every site keeps the value in a static const: read once per process
int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

// CILRS_PRIO: static wave priorities of the GEMM kernels (common.h wave_priority)
int wave_priority_mode() {
    static const int m = experiment_env("CILRS_PRIO", 0);
    return m;
}

namespace {

// ------------------------------------------------------------------------------------------------
// Architecture: parameter arena layout
// ------------------------------------------------------------------------------------------------
struct ParamT { std::string name; size_t off, numel; int ndim; int shape[4]; };
struct BnT { std::string prefix; int C; size_t gamma, beta, rm, rv; };
struct ConvT { int cin, cout, k, stride, pad; size_t w; int bn; int group; };
struct BlockT { int conv1, conv2, conv3, down; };   // conv3 = -1: BasicBlock; else Bottleneck
struct LinT { int in, out; size_t w, b; };

// variant 0: the reference's network -- ResNet-34 trunk (BasicBlock [3,4,6,3]), 512-d features
//            (model/autonomous_drive.py:365-370)
// variant 1: BASELINE.json configs[3], "ResNet-50 backbone variant": Bottleneck [3,4,6,3] with the
//            stride on the 3x3 convolution (torchvision's ResNet-50 v1.5), 2048-d features into the
//            same heads.  The reference has no such model; parity is against the build's own CPU
//            restatement (oracle/resnet50_oracle.py).  Trains in fp32 through the same kernels;
//            the 16-bit trunks are inference-only.
struct Arch {
    int variant = 0;                    // trunk: 0 ResNet-34 (the reference), 1 ResNet-50 variant
    int ncmd = 4;                       // control branches = commands (autonomous_drive.py:362)
    int feat = 512;                     // trunk feature width (avg-pool output)
    std::vector<ParamT> params;
    std::vector<BnT> bns;
    std::vector<ConvT> convs;           // convs[0] = stem
    std::vector<BlockT> blocks;
    LinT se0, se3, br[kMaxCmd][3], sp0, sp3, sp5;
    size_t arena_floats = 0, count = 0, bn_floats = 0;
    size_t seg_begin[6], seg_end[6];    // 0 heads, 1 layer4, 2 layer3, 3 layer2, 4 layer1, 5 stem
    int layer_first[5];                 // blocks[] index of layer L+1's first block; [4] = blocks.size()

    size_t add_param(const std::string& name, int ndim, int s0, int s1 = 1, int s2 = 1,
                     int s3 = 1) {
        ParamT p;
        p.name = name;
        p.ndim = ndim;
        p.shape[0] = s0; p.shape[1] = s1; p.shape[2] = s2; p.shape[3] = s3;
        p.numel = (size_t)s0 * s1 * s2 * s3;
        p.off = arena_floats;
        arena_floats += (p.numel + 3) / 4 * 4;      // keep every tensor 16-byte aligned
        count += p.numel;
        params.push_back(p);
        return p.off;
    }
    int add_bn(const std::string& prefix, int C) {
        BnT b;
        b.prefix = prefix;
        b.C = C;
        b.gamma = add_param(prefix + ".weight", 1, C);
        b.beta = add_param(prefix + ".bias", 1, C);
        b.rm = bn_floats;
        b.rv = bn_floats + C;
        bn_floats += 2 * (size_t)C;
        bns.push_back(b);
        return (int)bns.size() - 1;
    }
    int add_conv(const std::string& wname, const std::string& bnprefix, int cin, int cout, int k,
                 int stride, int pad, int group) {
        ConvT c;
        c.cin = cin; c.cout = cout; c.k = k; c.stride = stride; c.pad = pad; c.group = group;
        c.w = add_param(wname, 4, cout, cin, k, k);          // logical OIHW, stored OHWI
        c.bn = add_bn(bnprefix, cout);
        convs.push_back(c);
        return (int)convs.size() - 1;
    }
    LinT add_lin(const std::string& prefix, int in, int out) {
        LinT l;
        l.in = in; l.out = out;
        l.w = add_param(prefix + ".weight", 2, out, in);
        l.b = add_param(prefix + ".bias", 1, out);
        return l;
    }

    Arch(int variant_, int ncmd_) : variant(variant_), ncmd(ncmd_) {
        const size_t stem_begin = arena_floats;
        add_conv("visual_encoder.0.weight", "visual_encoder.1", 3, 64, 7, 2, 3, 0);
        size_t layer_begin[5];
        const int nblk[4] = {3, 4, 6, 3};
        const int width[4] = {64, 128, 256, 512};
        const int expansion = variant == 1 ? 4 : 1;
        int inpl = 64;
        for (int L = 0; L < 4; ++L) {
            layer_begin[L] = arena_floats;
            layer_first[L] = (int)blocks.size();
            for (int b = 0; b < nblk[L]; ++b) {
                const std::string p =
                    "visual_encoder." + std::to_string(4 + L) + "." + std::to_string(b);
                const int stride = (b == 0 && L > 0) ? 2 : 1;
                const int outpl = width[L] * expansion;
                BlockT blk;
                if (variant == 1) {     // Bottleneck: 1x1 -> 3x3 (stride) -> 1x1 (x4)
                    blk.conv1 = add_conv(p + ".conv1.weight", p + ".bn1", inpl, width[L], 1, 1, 0,
                                         L + 1);
                    blk.conv2 = add_conv(p + ".conv2.weight", p + ".bn2", width[L], width[L], 3,
                                         stride, 1, L + 1);
                    blk.conv3 = add_conv(p + ".conv3.weight", p + ".bn3", width[L], outpl, 1, 1, 0,
                                         L + 1);
                } else {                // BasicBlock: 3x3 (stride) -> 3x3
                    blk.conv1 = add_conv(p + ".conv1.weight", p + ".bn1", inpl, width[L], 3,
                                         stride, 1, L + 1);
                    blk.conv2 = add_conv(p + ".conv2.weight", p + ".bn2", width[L], width[L], 3, 1,
                                         1, L + 1);
                    blk.conv3 = -1;
                }
                blk.down = -1;
                if (stride != 1 || inpl != outpl)
                    blk.down = add_conv(p + ".downsample.0.weight", p + ".downsample.1", inpl,
                                        outpl, 1, stride, 0, L + 1);
                blocks.push_back(blk);
                inpl = outpl;
            }
        }
        feat = inpl;
        layer_begin[4] = arena_floats;
        layer_first[4] = (int)blocks.size();
        se0 = add_lin("speed_encoder.0", 1, 128);
        se3 = add_lin("speed_encoder.3", 128, 128);
        for (int k = 0; k < ncmd; ++k) {
            const std::string p = "control_branches." + std::to_string(k);
            br[k][0] = add_lin(p + ".0", feat + 128, 256);
            br[k][1] = add_lin(p + ".3", 256, 256);
            br[k][2] = add_lin(p + ".6", 256, 3);
        }
        sp0 = add_lin("speed_predictor.0", feat, 256);
        sp3 = add_lin("speed_predictor.3", 256, 256);
        sp5 = add_lin("speed_predictor.5", 256, 1);
        seg_begin[0] = layer_begin[4]; seg_end[0] = arena_floats;
        for (int L = 0; L < 4; ++L) {          // seg 1 = layer4 ... seg 4 = layer1
            seg_begin[4 - L] = layer_begin[L];
            seg_end[4 - L] = layer_begin[L + 1];
        }
        seg_begin[5] = stem_begin; seg_end[5] = layer_begin[0];
    }
};

constexpr int kNumVariants = 2;
// variant code = trunk | num_commands << 8 (0 in the upper bits = the reference's 4)
inline int code_trunk(int code) { return code & 0xff; }
inline int code_ncmd(int code) { return (code >> 8) == 0 ? 4 : (code >> 8); }
const Arch& arch(int code = 0) {
    static std::map<int, Arch*> cache;
    const int key = code_trunk(code) | (code_ncmd(code) << 8);
    auto it = cache.find(key);
    if (it == cache.end()) it = cache.emplace(key, new Arch(code_trunk(code), code_ncmd(code))).first;
    return *it->second;
}

const char* kGroupName[5] = {"stem", "layer1", "layer2", "layer3", "layer4"};

// ------------------------------------------------------------------------------------------------
// Per-kernel timing
// ------------------------------------------------------------------------------------------------
struct ProfRec { int label; hipEvent_t e0, e1; double flops, bytes; };
struct ProfAgg { long long calls = 0; double ms = 0, flops = 0, bytes = 0; };

struct Prof {
    bool on = false;
    std::vector<std::string> labels;
    std::map<std::string, int> index;
    std::vector<ProfAgg> agg;
    std::vector<ProfRec> pending;
    std::vector<hipEvent_t> pool;

    int label_id(const std::string& s) {
        auto it = index.find(s);
        if (it != index.end()) return it->second;
        const int id = (int)labels.size();
        labels.push_back(s);
        agg.push_back(ProfAgg());
        index[s] = id;
        return id;
    }
    hipEvent_t get_event() {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        // timing events: no system-scope release at the record (hipEventDisableSystemFence is
        // meant for exactly this: the cache write-back / invalidate between two kernels is not
        // part of either kernel, and the unprofiled step does not have it)
        hipEvent_t e;
        const unsigned flags = experiment_env("CILRS_PROF_NOFENCE", 1) ? hipEventDisableSystemFence : 0u;
        if (hipEventCreateWithFlags(&e, flags) != hipSuccess) return nullptr;
        return e;
    }
    int collect() {
        for (auto& r : pending) {
            CILRS_HIP(hipEventSynchronize(r.e1));
            float ms = 0.f;
            CILRS_HIP(hipEventElapsedTime(&ms, r.e0, r.e1));
            ProfAgg& a = agg[r.label];
            a.calls += 1; a.ms += ms; a.flops += r.flops; a.bytes += r.bytes;
            pool.push_back(r.e0);
            pool.push_back(r.e1);
        }
        pending.clear();
        return 0;
    }
    ~Prof() {
        for (auto& r : pending) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
};

}  // namespace
}  // namespace cilrs

using namespace cilrs;

// ------------------------------------------------------------------------------------------------
// The plan
// ------------------------------------------------------------------------------------------------
struct ConvG { int ci /*index in Arch::convs*/, H, W, Ho, Wo, M; size_t y, z, stats; };
// The frozen prefix of a fine-tuning step sends the layers the train plan gives to the Winograd
// kernel through its folded-epilogue variant (conv_wino.hip FOLD) instead of the implicit GEMM
// (DESIGN.md "Fine-tuning" has the per-shape measurement; CILRS_FT_WINO=0 of an experiments
// build puts the implicit GEMM back, read on every call so that tools/finetune_bench.py can
// compare the two in one process).
static bool ft_wino_fold() { return experiment_env("CILRS_FT_WINO", 1) != 0; }

// dy ring: bn_bwd writes each conv's output gradient into the next ring slot; the weight-gradient
// GEMM that consumes it runs on side stream 0 and may lag the data-gradient chain by one
// convolution (deeper rings were measured and bought nothing: DESIGN.md section 3).
constexpr int kDyRing = 2;
constexpr int kNumG = 5;
constexpr int kRingIdx[kDyRing] = {0, 4};

// a HIP handle the plan owns: destroyed with the plan if it was ever created
template <typename T, hipError_t (*Destroy)(T)>
struct Owned {
    T h = nullptr;
    Owned() = default;
    Owned(const Owned&) = delete;
    ~Owned() { if (h) (void)Destroy(h); }
    operator T() const { return h; }
};
using OwnedStream = Owned<hipStream_t, hipStreamDestroy>;
using OwnedEvent = Owned<hipEvent_t, hipEventDestroy>;
using OwnedGraphExec = Owned<hipGraphExec_t, hipGraphExecDestroy>;

struct cilrs_net {
    const Arch* A = nullptr;               // architecture variant of this plan
    int B = 0, H = 0, W = 0;
    std::vector<ConvG> cg;                 // geometry + workspace offsets (floats) per conv
    int H0 = 0, W0 = 0, H1 = 0, W1 = 0, featHW = 0;     // stem conv out, maxpool out, last map's pixels
    // workspace offsets (in floats unless noted)
    size_t x4 = 0, w4 = 0, pool = 0, argmax_b = 0 /*bytes offset*/, combined = 0, s1 = 0, p1 = 0, p2 = 0,
           h1[kMaxCmd] = {}, h2[kMaxCmd] = {}, all_out = 0;
    size_t dcombined = 0, ds1 = 0, dp1 = 0, dp2 = 0, dh1[kMaxCmd] = {}, dh2[kMaxCmd] = {},
           dcomb_part[kMaxCmd + 1] = {}, d_all = 0, speed_in = 0, cmd_b = 0 /*bytes offset*/;
    const void* status_cleared_for = nullptr;   // workspace whose status words have been cleared
    size_t G[kNumG] = {};                  // gradient buffers: [1..3] fixed roles, [0] and [4] = dy ring
    size_t gmax = 0, bn_partial = 0, bn_partial2 = 0, bn_coef = 0, slabs = 0, slabs_floats = 0, ksplit = 0,
           ksplit_floats = 0, status_b = 0, ws_bytes = 0;
    float* ws_base = nullptr;             // workspace of the current call (set by every entry)
    // side streams: independent kernels (weight-gradient vs data-gradient GEMMs, the five head
    // chains) run concurrently so one launch's tail fills with another's blocks
    bool overlap = true;
    bool streams_ready = false;            // ensure_streams has created all of these
    OwnedStream side[1];                   // weight-gradient stream
    OwnedEvent fork_ev, gbuf_ev[kNumG], wprep_ev, branch_ev, heads_ev;
    int side_branch = 0;                  // conv_fwd / conv_fwd16 are building a down-sample branch: no split-K scratch;
                                           // 1 = on the side stream, with column-partial scratch of its own
    bool wprep_pending = false;            // this step's weight images are being built on the side stream
    // What the backward pass carries from one launch to a later one, and from one call to the next
    // (everything else of a call is in its BwdPass).
    struct BwdState {
        // side stream 0 still reads gradient buffer gi.  Set by gbuf_side_end behind a weight
        // gradient, cleared by gbuf_acquire when the main stream has waited for it: gbuf_join_all
        // at the end of every backward call leaves all of them clear.
        bool gbuf_pending[kNumG] = {};
        // the heads' weight gradients are on the side stream.  Set by backward_heads (segment 0),
        // cleared by backward_join at the end of the same call.
        bool heads_pending = false;
        // next slot of the dy ring.  Advanced by BwdPass::next_ring, never reset: it lives as long
        // as the plan, so the two slots may swap roles from one step to the next.
        int dy_pos = 0;
    } bwd;
    BnEvalTable bn_table = {};
    BnStatsTable bn_stats = {};            // re-estimation table layout, indexed by BatchNorm layer
    FoldF16Table f16_table = {};           // fp16 inference: folded weights / biases / activations
    size_t f16_w = 0, f16_bias = 0, f16_act[5] = {}, f16_act_floats = 0;
    size_t stem16_w = 0, stem16_b = 0;     // folded 16-bit stem weights [64][7][8][4] / fp32 shift
    // cached hipGraph of the uint8 inference path (fixed pointers)
    OwnedGraphExec graph_exec;
    int graph_half = 0;
    const void* graph_key[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr};
    bool warmed = false;
    // Weight-derived inference state cached across calls: eval-mode BatchNorm scale/shift of every
    // layer + the channel-padded stem weights (prep_key), and the 16-bit folded weights / biases
    // (fold_key, fold_half).  Valid while the caller's weights key (cilrs_net_set_weights_key:
    // "parameters and BN buffers are unchanged while this value stays the same"; 0 = unknown,
    // never cache) and the buffers are the ones the state was computed from.
    uint64_t weights_key = 0, prep_key = 0, fold_key = 0, graph_wkey = 0;
    int fold_half = 0;
    const void* prep_bufs[3] = {nullptr, nullptr, nullptr};     // params, bn_running, workspace
    // What the plan's last forward left in the workspace; what may follow it is decided from here.
    // Written by fwd_begin (reset, before a forward's first launch) and fwd_commit (at its
    // successful end) alone, but for the two backward fields, which backward_impl keeps.
    struct LastForward {
        enum Kind {
            None,        // no forward yet, or one that did not finish
            Eval,        // z of every layer, pooled fp32 features in `combined`
            EvalB1,      // the persistent launch: pools inside its head stage, keeps no pooled copy
            Train,       // batch statistics, graph kept (cilrs_net_forward train != 0, _ft)
            Frozen,      // running statistics, graph kept (cilrs_net_forward_frozen*)
            StatsOnly    // cilrs_net_forward_bn_stats: the train-mode trunk, no heads, no graph
        } kind = None;
        int half = 0;              // Eval: arithmetic of the trunk (0 fp32, 1 fp16, 2 bf16)
        float dropout = 0.f;       // Train: the heads' dropout probability
        // segments of the backward on this forward whose outputs cilrs_net_input_grads reads:
        // bit 0 = d(speed encoder) of segment 0, bit 5 = d(stem conv output) in G[1]
        unsigned bwd_done = 0;
        // where an unbroken run of backward calls from segment 0 on this forward stopped (G[3] then
        // holds the gradient of trunk group 5 - gc_bwd_end's output; -1: none, or a failed call)
        int gc_bwd_end = -1;
        bool keeps_graph() const { return kind == Train || kind == Frozen; }   // cilrs_net_backward*
        bool frozen() const { return kind == Frozen; }
        // the features of the tick-following entries (heads_mc, gradcam, feature_moments, novelty):
        // none, a train-mode forward's (refused), the last feature map only, else pooled
        bool no_features() const { return kind == None; }
        bool train_features() const { return kind == Train || kind == StatsOnly; }
        bool featmap_only() const { return kind == EvalB1; }
    } last;
    // bf16 training mode (CILRS_PLAN_BF16_TRAIN): the trunk convolutions after the stem multiply
    // bf16 operands on v_mfma_f32_32x32x16_bf16 (fp32 accumulation, fp32 results); everything
    // else -- BatchNorm, residual adds, the stem, the heads, loss, Adam, master weights -- stays
    // fp32.  16-bit shadows (offsets in floats): whole parameter arena, transposed flipped conv
    // weights, every post-BN activation, the max-pool output, the dy ring.
    bool bf16_train = false;
    size_t w16_all = 0, wT16 = 0, pool16 = 0, slabs16 = 0, slabs16_floats = 0;
    size_t z16[kMaxConvs] = {}, wT16_off[kMaxConvs] = {}, G16[kNumG] = {};
    TransposeF16Table tr_table = {};
    // Winograd F(2x2, 3x3) (conv_wino.hip) for the stride-1 3x3 convolutions of fp32 train plans
    // where it beats the implicit GEMM (layers of up to 256 channels with enough blocks to fill
    // the chip; CILRS_WINO=0 turns it off): forward + data gradient.  Both transformed-filter
    // images of every such layer live in the workspace and are rebuilt by ONE launch at the top
    // of each training forward (the weights change every step).
    int wino_slot[kMaxConvs];              // the layer's entry in wino_table, -1: not a Winograd layer
    size_t wino_base = 0;
    WinoWeightTable wino_table = {};
    // Fine-tuning (cilrs_net_forward_ft): leading trunk groups (stem, layer1..layer4) of the last
    // graph-keeping forward that ran in eval mode (ft_bn: BatchNorm folded into the convolution
    // epilogues, nothing kept for a backward pass) / whose parameters take no gradient (ft_grad:
    // where cilrs_net_backward stops); fwd_commit clears the cut for every kind but Eval / EvalB1,
    // cilrs_net_forward_ft sets it.  The prefix's weight-derived state -- scale / shift of its
    // BatchNorms, the padded stem weights, the Winograd filter images of its layers -- is cached
    // under the caller's prefix key.  ft_wino: folded-epilogue Winograd launches of that forward.
    int ft_bn = 0, ft_grad = 0, ft_wino = 0;
    bool ft_route_wino = false;            // conv_fwd is building a frozen prefix
    uint64_t ft_prep_key = 0;
    int ft_prep_groups = 0;
    const void* ft_prep_bufs[3] = {nullptr, nullptr, nullptr};
    // persistent single-frame kernel (infer_b1.hip): stage table + barrier counters in the
    // workspace (offsets in floats; 0 = this plan has none), uploaded once per workspace
    size_t b1_table = 0, b1_sync = 0, b1_stamps = 0, b1_slabs = 0, b1_slab_floats = 0, b1_cmd = 0;
    std::vector<B1Stage> b1_host;
    int b1_blocks = -1;                    // resident grid (one workgroup per CU); -1 = not asked yet
    const void* b1_ready_for = nullptr;
    Prof prof;
    cilrs_net() { std::fill(wino_slot, wino_slot + kMaxConvs, -1); }
};

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Bump {
    size_t off = 0;   // floats
    size_t take(size_t floats) {
        const size_t o = off;
        off = align_up(off + floats, 64);
        return o;
    }
};

#define RUN(NET_, LBL_, FL_, BY_, ST_, CALL_)                                         \
    do {                                                                              \
        Prof& pr_ = (NET_)->prof;                                                     \
        if (pr_.on) {                                                                 \
            ProfRec r_;                                                               \
            r_.label = pr_.label_id(LBL_);                                            \
            r_.flops = (FL_); r_.bytes = (BY_);                                       \
            r_.e0 = pr_.get_event(); r_.e1 = pr_.get_event();                         \
            CILRS_CHECK(r_.e0 && r_.e1, "hipEventCreate failed");                     \
            CILRS_HIP(hipEventRecord(r_.e0, (ST_)));                                  \
            if (CALL_) return 1;                                                      \
            CILRS_HIP(hipEventRecord(r_.e1, (ST_)));                                  \
            pr_.pending.push_back(r_);                                                \
        } else {                                                                      \
            if (CALL_) return 1;                                                      \
        }                                                                             \
    } while (0)

// the int32[4] status words start at zero in every workspace (a C-ABI caller brings its own,
// uninitialised one); afterwards the kernels only ever SET them: "since the caller last cleared"
int clear_status_once(cilrs_net* net, void* workspace, hipStream_t s) {
    if (net->status_cleared_for == workspace) return 0;
    CILRS_HIP(hipMemsetAsync(reinterpret_cast<char*>(workspace) + net->status_b, 0, 16, s));
    net->status_cleared_for = workspace;
    return 0;
}
static int* status_words(const cilrs_net* net, const cilrs_buffers* bufs) {
    return reinterpret_cast<int*>(reinterpret_cast<char*>(bufs->workspace) + net->status_b);
}

// The two writers of cilrs_net::last: every forward calls fwd_begin before its first launch (from
// there on the workspace no longer holds the previous forward) and fwd_commit at its successful end.
int fwd_begin(cilrs_net* net, const cilrs_buffers* bufs, hipStream_t s) {
    net->ws_base = reinterpret_cast<float*>(bufs->workspace);
    net->last = cilrs_net::LastForward();
    return clear_status_once(net, bufs->workspace, s);
}
void fwd_commit(cilrs_net* net, cilrs_net::LastForward::Kind kind, int half = 0, float dropout = 0.f) {
    net->last.kind = kind; net->last.half = half; net->last.dropout = dropout;
    if (kind != cilrs_net::LastForward::Eval && kind != cilrs_net::LastForward::EvalB1)
        net->ft_bn = net->ft_grad = 0;
}
// weights or BatchNorm tables are about to change: the cached eval state goes stale
void drop_eval_state(cilrs_net* net) { net->prep_key = net->fold_key = 0; }

// Events that only order one stream of this device behind another (hipStreamWaitEvent; the host
// never inspects them).  hipEventDisableSystemFence: by default a HIP event performs a SYSTEM-scope
// release when it is recorded -- a cache write-back / invalidate so that the HOST may synchronise
// with it -- ~70 times per backward pass here (one fork and one join per weight gradient).  Without
// it the step is 0.13 ms shorter (9.37 -> 9.25 ms, tools/ab_env.sh CILRS_EVENT_NOFENCE 0 1); the
// device-side ordering of hipStreamWaitEvent is not affected (the kernels' own agent-scope
// releases make their results visible to the other stream).
unsigned stream_event_flags() {
    static const int nofence = experiment_env("CILRS_EVENT_NOFENCE", 1);
    return hipEventDisableTiming | (nofence ? hipEventDisableSystemFence : 0u);
}
int ensure_streams(cilrs_net* net) {
    if (net->streams_ready) return 0;
    // side stream 0 carries the weight-gradient GEMMs.  (what a call that failed half-way had
    // created stays with the plan, which destroys it; a retry creates the rest)
    if (!net->side[0].h) CILRS_HIP(hipStreamCreateWithFlags(&net->side[0].h, hipStreamNonBlocking));
    OwnedEvent* evs[kNumG + 4] = {&net->fork_ev, &net->wprep_ev, &net->branch_ev, &net->heads_ev};
    for (int i = 0; i < kNumG; ++i) evs[4 + i] = &net->gbuf_ev[i];
    for (OwnedEvent* e : evs)
        if (!e->h) CILRS_HIP(hipEventCreateWithFlags(&e->h, stream_event_flags()));
    net->streams_ready = true;
    return 0;
}
// concurrency is switched off while per-kernel timing is on (serial brackets are meaningful)
// (the CONFIGURED state: what an unprofiled step of this plan does)
bool overlap_configured(cilrs_net* net) {
    // CILRS_OVERLAP=0 serialises everything on the caller's stream (rocprofv3 per-kernel durations
    // then match the hipEvent brackets of the profile mode)
    static const int env = env_int("CILRS_OVERLAP", 1);
    return env != 0 && net->overlap;
}
bool use_overlap(cilrs_net* net) { return overlap_configured(net) && !net->prof.on; }
hipStream_t side_or(cilrs_net* net, hipStream_t main, int i) {
    return use_overlap(net) ? net->side[i] : main;
}
// gradient buffer `gi` is about to be overwritten on `main`: wait for a side-stream reader
int gbuf_acquire(cilrs_net* net, hipStream_t main, int gi) {
    if (net->bwd.gbuf_pending[gi]) {
        CILRS_HIP(hipStreamWaitEvent(main, net->gbuf_ev[gi], 0));
        net->bwd.gbuf_pending[gi] = false;
    }
    return 0;
}
// side stream 0 continues from here on `main`: what it runs next sees everything `main` has been
// given so far (the weight images, a down-sample branch, the heads' weight gradients, a fused
// Adam launch, a weight gradient reading the buffer `main` has just produced)
int side_fork(cilrs_net* net, hipStream_t main) {
    if (!use_overlap(net)) return 0;
    if (ensure_streams(net)) return 1;
    CILRS_HIP(hipEventRecord(net->fork_ev, main));
    CILRS_HIP(hipStreamWaitEvent(net->side[0], net->fork_ev, 0));
    return 0;
}
// side stream 0 has been given its reader of gradient buffer `gi`
int gbuf_side_end(cilrs_net* net, int gi) {
    if (!use_overlap(net)) return 0;
    CILRS_HIP(hipEventRecord(net->gbuf_ev[gi], net->side[0]));
    net->bwd.gbuf_pending[gi] = true;
    return 0;
}
int gbuf_join_all(cilrs_net* net, hipStream_t main) {
    for (int gi = 0; gi < kNumG; ++gi)
        if (gbuf_acquire(net, main, gi)) return 1;
    return 0;
}

// ---- one builder per operator's arguments: the geometry of a dense NHWC / OHWI problem.  Pointers,
//      scratch, epilogue and tuning fields are the caller's (the plan's, or an op-level entry's) ----
int out_dim(int in, int k, int s, int p) { return (in + 2 * p - k) / s + 1; }

ConvArgs conv_args(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.N = N; a.H = H; a.W = W; a.Cin = Cin;
    a.Ho = out_dim(H, KH, stride, pad); a.Wo = out_dim(W, KW, stride, pad); a.Cout = Cout;
    a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad;
    a.x_ld = Cin; a.y_ld = Cout; a.w_mode = 0; a.w_cin = Cin;
    return a;
}
DgradArgs dgrad_args(int N, int H, int W, int Cin, int Cout, int K, int stride, int pad) {
    DgradArgs a;
    memset(&a, 0, sizeof(a));
    a.N = N; a.H = H; a.W = W; a.Cin = Cin;
    a.Ho = out_dim(H, K, stride, pad); a.Wo = out_dim(W, K, stride, pad);
    a.Cout = Cout; a.K = K; a.stride = stride; a.pad = pad;
    a.dy_ld = Cout; a.dx_ld = Cin;
    return a;
}
// Cin: channels of x as stored (4 for the stem's channel-padded image), Cin_dst: channels of dw
WgradArgs wgrad_args(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                     int Cin_dst) {
    WgradArgs a;
    memset(&a, 0, sizeof(a));
    a.N = N; a.H = H; a.W = W; a.Cin = Cin;
    a.Ho = out_dim(H, KH, stride, pad); a.Wo = out_dim(W, KW, stride, pad); a.Cout = Cout;
    a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad;
    a.x_ld = Cin; a.dy_ld = Cout; a.Cin_dst = Cin_dst; a.accumulate = 0;
    return a;
}
// a Winograd launch over the plan's [B][H][W] map of convolution g: C channels gathered, K written
WinoArgs wino_args(const cilrs_net* net, const ConvG& g, int C, int K) {
    WinoArgs a;
    memset(&a, 0, sizeof(a));
    a.N = net->B; a.H = g.H; a.W = g.W; a.C = C; a.K = K;
    return a;
}

// ---- profile estimates: the DIRECT convolution's flops, whichever kernel runs it, and ----
double conv_flops(const ConvT& c, const ConvG& g) { return 2.0 * g.M * c.cout * c.k * c.k * c.cin; }
// the bytes of input, output (out_passes 2: a residual read beside the write) and weights (wino: the
// 16-point filter image), each at its element size.  (whole numbers far below 2^53: the sum is exact)
double conv_bytes(const cilrs_net* net, const ConvT& c, const ConvG& g, double in_size,
                  double out_size, double w_size, bool wino = false, double out_passes = 1.0) {
    const double in = (double)net->B * g.H * g.W * c.cin, out = (double)g.M * c.cout;
    const double w = wino ? 16.0 * c.cout * c.cin : (double)c.cout * c.k * c.k * c.cin;
    return in_size * in + out_size * out * out_passes + w_size * w;
}

int conv_fwd(cilrs_net* net, const ConvT& c, const ConvG& g, const float* x, int x_cin,
             const float* w, float* y, float* ws, hipStream_t s, int* bn_nblk = nullptr,
             const float* fold_stats = nullptr, int relu = 0, const float* addend = nullptr,
             int relu_post = 0) {
    auto label = [&] { return std::string("conv_fwd.") + kGroupName[c.group]; };     // (profile mode only)
    const int e = net->wino_slot[g.ci];
    if (bn_nblk && !fold_stats && e >= 0) {      // training forward on the Winograd kernel
        WinoArgs wa = wino_args(net, g, c.cin, c.cout);
        wa.x = x; wa.U = ws + net->wino_base + net->wino_table.u[e]; wa.y = y;
        wa.bn_partial = ws + net->bn_partial;
        wa.slabs = ws + net->ksplit; wa.slab_floats = net->ksplit_floats;
        wa.scratch_partial = ws + net->bn_partial;
        *bn_nblk = wino_rows(net->B, g.H, g.W, c.cout, 0, c.cin, net->ksplit_floats);
        RUN(net, label(), conv_flops(c, g), conv_bytes(net, c, g, 4, 4, 4, true), s,
            launch_conv_wino(wa, s));
        return 0;
    }
    if (fold_stats && net->ft_route_wino && e >= 0 && ft_wino_fold()) {
        // frozen prefix of a fine-tuning step: the Winograd kernel with the folded epilogue
        WinoArgs wa = wino_args(net, g, c.cin, c.cout);
        wa.x = x; wa.U = ws + net->wino_base + net->wino_table.u[e]; wa.y = y; wa.addend = addend;
        const WinoFold f{fold_stats + 2 * c.cout, fold_stats + 3 * c.cout, relu, relu_post};
        RUN(net, label(), conv_flops(c, g), conv_bytes(net, c, g, 4, 4, 4, true, addend ? 2.0 : 1.0), s,
            launch_conv_wino_fold(wa, f, s));
        ++net->ft_wino;
        return 0;
    }
    ConvArgs a = conv_args(net->B, g.H, g.W, x_cin, c.cout, c.k, c.k, c.stride, c.pad);
    a.x = x; a.w = w; a.y = y;
    if (fold_stats) {            // eval-mode BatchNorm (+ReLU / residual) folded into the epilogue
        a.ch_scale = fold_stats + 2 * c.cout;
        a.ch_shift = fold_stats + 3 * c.cout;
        a.relu = relu; a.addend = addend; a.relu_post = relu_post;
    }
    a.scratch = ws + net->ksplit; a.scratch_floats = net->ksplit_floats;
    if (net->side_branch) { a.scratch = nullptr; a.scratch_floats = 0; }     // (no split-K beside the main stream's)
    a.force_cfg = -1;
    if (bn_nblk) {
        a.bn_partial = ws + (net->side_branch == 1 ? net->bn_partial2 : net->bn_partial);
        a.bn_nblk = bn_nblk; *bn_nblk = 0;
    }
    RUN(net, label(), conv_flops(c, g), conv_bytes(net, c, g, 4, 4, 4), s, launch_conv_igemm(a, s));
    return 0;
}

// dx[B,H,W,cin] (+= addend) from dy[B,Ho,Wo,cout]
int conv_dgrad(cilrs_net* net, const ConvT& c, const ConvG& g, const float* dy, const float* w,
               float* dx, const float* addend, float* ws, hipStream_t s,
               const ConvG* bn_of = nullptr, int bn_relu = 1, int* bwd_nblk = nullptr) {
    auto label = [&] { return std::string("conv_dgrad.") + kGroupName[c.group]; };
    const int e = net->wino_slot[g.ci];
    if (e >= 0) {                  // the same convolution with the flipped, transposed filter
        WinoArgs wa = wino_args(net, g, c.cout, c.cin);
        wa.x = dy; wa.U = ws + net->wino_base + net->wino_table.ud[e]; wa.y = dx; wa.addend = addend;
        // the 16-tile tail launch pays in the forward pass only: in the backward pass the weight
        // gradients of the side stream already fill the CUs a last round leaves idle, and a
        // second launch per data gradient costs more in boundaries than it gains (step 11.09 vs
        // 10.99 ms with tails on both sides, profiles/r03_wino_tail.log)
        // Re-measured in round 4 with both kinds of block in ONE launch (CILRS_WINO_DGRAD_TAIL=1 of
        // an experiments build): the data-gradient family 3.29 -> 3.04 ms serialised, the
        // overlapped step 9.32 -> 9.50 ms.
        // (decided by the plan's configuration, not by whether this step is being profiled: the
        //  profiled steps of bench.py must run the kernels the timed steps ran)
        wa.no_tail = (overlap_configured(net) && !experiment_env("CILRS_WINO_DGRAD_TAIL", 0)) ? 1 : 0;
        wa.slabs = ws + net->ksplit; wa.slab_floats = net->ksplit_floats;
        wa.scratch_partial = ws + net->bn_partial;
        if (bwd_nblk) *bwd_nblk = 0;
        if (bn_of && bwd_nblk) {
            wa.bwd_z = ws + bn_of->z; wa.bwd_y = ws + bn_of->y; wa.bwd_stats = ws + bn_of->stats;
            wa.bwd_relu = bn_relu; wa.bwd_partial = ws + net->bn_partial;
            *bwd_nblk = wino_rows(net->B, g.H, g.W, c.cin, wa.no_tail, c.cout, net->ksplit_floats);
        }
        RUN(net, label(), conv_flops(c, g), conv_bytes(net, c, g, 4, 4, 4, true), s,
            launch_conv_wino(wa, s));
        return 0;
    }
    DgradArgs a = dgrad_args(net->B, g.H, g.W, c.cin, c.cout, c.k, c.stride, c.pad);
    a.dy = dy; a.w = w; a.dx = dx; a.addend = addend;
    if (bn_of && bwd_nblk) {       // the BatchNorm layer whose output gradient this call produces
        a.bwd_z = ws + bn_of->z; a.bwd_y = ws + bn_of->y; a.bwd_stats = ws + bn_of->stats;
        a.bwd_relu = bn_relu; a.bwd_partial = ws + net->bn_partial; a.bwd_nblk = bwd_nblk;
        *bwd_nblk = 0;
    }
    a.scratch = ws + net->ksplit; a.scratch_floats = net->ksplit_floats;
    a.force_cfg = -1;
    RUN(net, label(), conv_flops(c, g), conv_bytes(net, c, g, 4, 4, 4), s, launch_conv_dgrad(a, s));
    return 0;
}

// The weight gradient of every 3x3 / stride-1 convolution with channel counts in multiples of 64
// runs in the Winograd domain (conv_wino.hip: 1.09-1.46x the direct kernel at B=128, all four
// layers); CILRS_WINO_WGRAD=0 turns it off.  Independent of CILRS_WINO (forward / data gradient).
static bool wino_wgrad_on(const ConvT& c) {
    static const int env = env_int("CILRS_WINO_WGRAD", 1);
    return env != 0 && wino_wgrad_supported(c.cin, c.cout, c.k, c.stride, c.pad);
}

int conv_wgrad(cilrs_net* net, const ConvT& c, const ConvG& g, const float* x, int x_cin,
               const float* dy, float* dw, float* ws, hipStream_t s) {
    auto label = [&] { return std::string("conv_wgrad.") + kGroupName[c.group]; };
    if (x_cin == c.cin && !net->bf16_train && wino_wgrad_on(c)) {
        WinoWgradArgs wa;
        memset(&wa, 0, sizeof(wa));
        wa.x = x; wa.dy = dy; wa.dw = dw; wa.slabs = ws + net->slabs;
        wa.N = net->B; wa.H = g.H; wa.W = g.W; wa.C = c.cin; wa.K = c.cout;
        CILRS_CHECK(wino_wgrad_scratch_floats(net->B, g.H, g.W, c.cin, c.cout) <= net->slabs_floats,
                    "Winograd wgrad scratch too small");
        RUN(net, label(), conv_flops(c, g), conv_bytes(net, c, g, 4, 4, 4), s,
            launch_conv_wino_wgrad(wa, s));
        return 0;
    }
    // (the arguments plan_sizes sized the slabs from)
    WgradArgs a = wgrad_args(net->B, g.H, g.W, x_cin, c.cout, c.k, c.k, c.stride, c.pad, c.cin);
    a.x = x; a.dy = dy; a.dw = dw; a.slabs = ws + net->slabs;
    CILRS_CHECK(wgrad_scratch_floats(a) <= net->slabs_floats, "wgrad scratch too small");
    RUN(net, label(), conv_flops(c, g), conv_bytes(net, c, g, 4, 4, 4), s, launch_conv_wgrad(a, s));
    return 0;
}

cilrs_half* h16(float* ws, size_t off_floats) {
    return reinterpret_cast<cilrs_half*>(ws + off_floats);
}

// the same three operators on the bf16 matrix pipe (bf16 training mode); profile labels as above.
// Since round 4 the mode keeps every trunk tensor after the stem in bf16 (activations, raw
// convolution outputs, gradients): the raw output y16 of convolution ci lives where the fp32 mode
// keeps its y (same offset, half the bytes), the post-BatchNorm tensor in z16[ci].
cilrs_half* y16_of(const cilrs_net* net, float* ws, int ci) { return h16(ws, net->cg[ci].y); }

int conv_fwd16(cilrs_net* net, const ConvT& c, const ConvG& g, const cilrs_half* x16,
               float* ws, hipStream_t s, int* bn_nblk) {
    ConvF16Args a;
    memset(&a, 0, sizeof(a));
    a.x = x16; a.w = h16(ws, net->w16_all) + c.w; a.y16 = y16_of(net, ws, g.ci);
    a.bn_partial = ws + (net->side_branch == 1 ? net->bn_partial2 : net->bn_partial);
    a.N = net->B; a.H = g.H; a.W = g.W; a.Cin = c.cin; a.Ho = g.Ho; a.Wo = g.Wo; a.Cout = c.cout;
    a.K = c.k; a.stride = c.stride; a.pad = c.pad; a.bf16 = 1;
    *bn_nblk = conv_f16_train_mtiles(a);
    RUN(net, std::string("conv_fwd.") + kGroupName[c.group], conv_flops(c, g),
        conv_bytes(net, c, g, 2, 2, 2), s, launch_conv_f16_train(a, s));
    return 0;
}

// dx (16-bit, or fp32 when dx32 is given: the gradient handed to the fp32 stem) = dgrad(dy16)
// (+ addend16); bn_of: the convolution whose BatchNorm-backward reductions ride on the epilogue
int conv_dgrad16(cilrs_net* net, const ConvT& c, const ConvG& g, const cilrs_half* dy16,
                 cilrs_half* dx16, float* dx32, const cilrs_half* addend16, float* ws,
                 hipStream_t s, const ConvG* bn_of = nullptr, int* bwd_nblk = nullptr) {
    ConvF16Args a;
    memset(&a, 0, sizeof(a));
    a.x = dy16; a.w = h16(ws, net->wT16) + net->wT16_off[g.ci];
    if (dx32) a.y32 = dx32; else a.y16 = dx16;
    a.addend16 = addend16;
    a.N = net->B; a.H = g.Ho; a.W = g.Wo; a.Cin = c.cout;      // gathered tensor = dy
    a.Ho = g.H; a.Wo = g.W; a.Cout = c.cin;                    // enumerated grid = dx
    a.K = c.k; a.bf16 = 1;
    if (c.stride == 1) { a.stride = 1; a.pad = c.k - 1 - c.pad; }
    else { a.stride = 2; a.pad = c.pad; a.up2 = 1; }
    if (bwd_nblk) *bwd_nblk = 0;
    if (bn_of && bwd_nblk && conv_f16_train_can_fuse_bwd(a)) {   // the BatchNorm whose output gradient this is
        a.bwd_z16 = h16(ws, net->z16[bn_of->ci]); a.bwd_y16 = y16_of(net, ws, bn_of->ci);
        a.bwd_stats = ws + bn_of->stats;
        a.bwd_relu = 1; a.bwd_partial = ws + net->bn_partial;
        *bwd_nblk = conv_f16_train_mtiles(a);
    }
    RUN(net, std::string("conv_dgrad.") + kGroupName[c.group], conv_flops(c, g),
        conv_bytes(net, c, g, dx32 ? 4 : 2, 2, 2), s, launch_conv_f16_train(a, s));
    return 0;
}

WgradF16Args wgrad16_args(const cilrs_net* net, const ConvT& c, const ConvG& g) {
    WgradF16Args a;
    memset(&a, 0, sizeof(a));
    a.N = net->B; a.H = g.H; a.W = g.W; a.Cin = c.cin; a.Ho = g.Ho; a.Wo = g.Wo; a.Cout = c.cout;
    a.K = c.k; a.stride = c.stride; a.pad = c.pad; a.bf16 = 1;
    return a;
}

int conv_wgrad16(cilrs_net* net, const ConvT& c, const ConvG& g, const cilrs_half* x16,
                 const cilrs_half* dy16, float* dw, float* ws, hipStream_t s) {
    WgradF16Args a = wgrad16_args(net, c, g);
    a.x = x16; a.dy = dy16; a.dw = dw; a.slabs = ws + net->slabs16;
    CILRS_CHECK(wgrad_f16_scratch_floats(a) <= net->slabs16_floats, "wgrad16 scratch too small");
    RUN(net, std::string("conv_wgrad.") + kGroupName[c.group], conv_flops(c, g),
        conv_bytes(net, c, g, 2, 2, 4), s, launch_wgrad_f16(a, s));
    return 0;
}

}  // namespace

static void bn_stats_layout(const Arch& A, BnStatsTable& t) {
    memset(&t, 0, sizeof(t));
    t.n = (int)A.bns.size();
    size_t off = (size_t)kBnStatsHead * A.bns.size();
    for (int j = 0; j < t.n; ++j) {
        const BnT& b = A.bns[j];
        t.C[j] = b.C;
        t.rm[j] = (unsigned)b.rm; t.rv[j] = (unsigned)b.rv;
        t.head[j] = (unsigned)(kBnStatsHead * j);
        t.sums[j] = (unsigned)off;
        off += (size_t)kBnStatsRows * b.C;
    }
}

// ------------------------------------------------------------------------------------------------
// C-ABI: layout queries
// ------------------------------------------------------------------------------------------------
extern "C" {

int cilrs_version(void) { return 1; }
const char* cilrs_last_error(void) { return last_error(); }
int cilrs_num_params(void) { return (int)arch().params.size(); }
int cilrs_num_bn(void) { return (int)arch().bns.size(); }
size_t cilrs_param_arena_floats(void) { return arch().arena_floats; }
size_t cilrs_param_count(void) { return arch().count; }
size_t cilrs_bn_arena_floats(void) { return arch().bn_floats; }

int cilrs_num_variants(void) { return kNumVariants; }
static bool variant_ok(int v) {
    return v >= 0 && code_trunk(v) < kNumVariants && (v >> 16) == 0 && code_ncmd(v) >= 1 &&
           code_ncmd(v) <= kMaxCmd;
}
int cilrs_variant_num_params(int variant) {
    return variant_ok(variant) ? (int)arch(variant).params.size() : -1;
}
int cilrs_variant_num_bn(int variant) {
    return variant_ok(variant) ? (int)arch(variant).bns.size() : -1;
}
size_t cilrs_variant_param_arena_floats(int variant) {
    return variant_ok(variant) ? arch(variant).arena_floats : 0;
}
size_t cilrs_variant_param_count(int variant) {
    return variant_ok(variant) ? arch(variant).count : 0;
}
size_t cilrs_variant_bn_arena_floats(int variant) {
    return variant_ok(variant) ? arch(variant).bn_floats : 0;
}
int cilrs_variant_feature_width(int variant) {
    return variant_ok(variant) ? arch(variant).feat : -1;
}

int cilrs_param_info(int i, char* name, int name_cap, size_t* offset, size_t* numel, int* ndim,
                     int* shape4) {
    return cilrs_variant_param_info(0, i, name, name_cap, offset, numel, ndim, shape4);
}

int cilrs_variant_param_info(int variant, int i, char* name, int name_cap, size_t* offset,
                             size_t* numel, int* ndim, int* shape4) {
    CILRS_CHECK(variant_ok(variant), "variant %d out of range", variant);
    const Arch& A = arch(variant);
    CILRS_CHECK(i >= 0 && i < (int)A.params.size(), "param index %d out of range", i);
    const ParamT& p = A.params[i];
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", p.name.c_str());
    if (offset) *offset = p.off;
    if (numel) *numel = p.numel;
    if (ndim) *ndim = p.ndim;
    if (shape4) for (int k = 0; k < 4; ++k) shape4[k] = p.shape[k];
    return 0;
}

int cilrs_bn_info(int j, char* prefix, int prefix_cap, int* channels, size_t* rm_offset,
                  size_t* rv_offset) {
    return cilrs_variant_bn_info(0, j, prefix, prefix_cap, channels, rm_offset, rv_offset);
}

int cilrs_variant_bn_info(int variant, int j, char* prefix, int prefix_cap, int* channels,
                          size_t* rm_offset, size_t* rv_offset) {
    CILRS_CHECK(variant_ok(variant), "variant %d out of range", variant);
    const Arch& A = arch(variant);
    CILRS_CHECK(j >= 0 && j < (int)A.bns.size(), "bn index %d out of range", j);
    const BnT& b = A.bns[j];
    if (prefix && prefix_cap > 0) snprintf(prefix, prefix_cap, "%s", b.prefix.c_str());
    if (channels) *channels = b.C;
    if (rm_offset) *rm_offset = b.rm;
    if (rv_offset) *rv_offset = b.rv;
    return 0;
}

// BatchNorm re-estimation table of a variant (doubles): {t, sum M} of layer 0, 1, ... and then the
// layers' [4][C] blocks, in cilrs_variant_bn_info order
size_t cilrs_variant_bn_stats_doubles(int variant) {
    if (!variant_ok(variant)) return 0;
    const Arch& A = arch(variant);
    return (size_t)kBnStatsHead * A.bns.size() + (size_t)(kBnStatsRows / 2) * A.bn_floats;
}

int cilrs_variant_bn_stats_info(int variant, int j, int* channels, size_t* head_offset,
                                size_t* sums_offset) {
    CILRS_CHECK(variant_ok(variant), "variant %d out of range", variant);
    const Arch& A = arch(variant);
    CILRS_CHECK(j >= 0 && j < (int)A.bns.size(), "bn index %d out of range", j);
    BnStatsTable t;
    bn_stats_layout(A, t);
    if (channels) *channels = t.C[j];
    if (head_offset) *head_offset = t.head[j];
    if (sums_offset) *sums_offset = t.sums[j];
    return 0;
}

int cilrs_segment_range(int seg, size_t* begin, size_t* end) {
    return cilrs_variant_segment_range(0, seg, begin, end);
}

int cilrs_variant_segment_range(int variant, int seg, size_t* begin, size_t* end) {
    CILRS_CHECK(variant_ok(variant), "variant %d out of range", variant);
    CILRS_CHECK(seg >= 0 && seg < 6 && begin && end, "segment %d out of range", seg);
    *begin = arch(variant).seg_begin[seg];
    *end = arch(variant).seg_end[seg];
    return 0;
}

// ------------------------------------------------------------------------------------------------
// plan creation
// ------------------------------------------------------------------------------------------------
int cilrs_net_create(int batch, int height, int width, cilrs_net** out) {
    return cilrs_net_create_variant(0, batch, height, width, out);
}

int cilrs_net_create_variant(int variant, int batch, int height, int width, cilrs_net** out) {
    return cilrs_net_create_ex(variant, batch, height, width, 0u, out);
}

// Three kinds of step build a plan, in this order: the geometry (pure), the sizes that follow from
// it (pure), and the placement steps, which take from the Bump in workspace order.
// Geometry: H / W / Ho / Wo / M of every convolution, the stem and max-pool maps, featHW.  No offsets.
static int plan_geometry(cilrs_net* n) {
    const Arch& A = *n->A;
    n->cg.resize(A.convs.size());
    auto set = [&](int ci, int in_h, int in_w) {
        const ConvT& c = A.convs[ci];
        ConvG& g = n->cg[ci];
        g.ci = ci; g.H = in_h; g.W = in_w;
        g.Ho = out_dim(in_h, c.k, c.stride, c.pad); g.Wo = out_dim(in_w, c.k, c.stride, c.pad);
        g.M = n->B * g.Ho * g.Wo;
    };
    set(0, n->H, n->W);
    n->H0 = n->cg[0].Ho; n->W0 = n->cg[0].Wo;
    n->H1 = out_dim(n->H0, 3, 2, 1); n->W1 = out_dim(n->W0, 3, 2, 1);
    int h = n->H1, w = n->W1;
    for (const BlockT& blk : A.blocks) {
        set(blk.conv1, h, w);
        set(blk.conv2, n->cg[blk.conv1].Ho, n->cg[blk.conv1].Wo);
        const int oh = n->cg[blk.conv2].Ho, ow = n->cg[blk.conv2].Wo;
        if (blk.conv3 >= 0) set(blk.conv3, oh, ow);
        if (blk.down >= 0) {
            set(blk.down, h, w);
            CILRS_CHECK(n->cg[blk.down].Ho == oh && n->cg[blk.down].Wo == ow,
                        "downsample geometry mismatch");
        }
        h = oh; w = ow;
    }
    n->featHW = h * w;
    return 0;
}

// Sizes: the maxima over the network that the shared buffers are sized by (floats / elements)
struct PlanSizes { size_t gmax = 0, actmax = 0, slabs_max = 0, ksplit_max = 0, need = 0; };
static PlanSizes plan_sizes(const cilrs_net* n) {
    const Arch& A = *n->A;
    const int B = n->B;
    PlanSizes z;
    auto up = [](size_t& m, size_t v) { if (v > m) m = v; };
    // gmax: the gradient buffers hold d(block input), d(block output) and every conv output's gradient
    up(z.gmax, (size_t)n->cg[0].M * 64);
    for (const BlockT& blk : A.blocks) {
        const ConvG& g1 = n->cg[blk.conv1];
        up(z.gmax, (size_t)B * g1.H * g1.W * A.convs[blk.conv1].cin);
        for (int ci : {blk.conv1, blk.conv2, blk.conv3, blk.down})
            if (ci >= 0) up(z.gmax, (size_t)n->cg[ci].M * A.convs[ci].cout);
    }
    // actmax: the largest trunk tensor (the max-pool output or a convolution's)
    up(z.actmax, (size_t)B * n->H1 * n->W1 * 64);
    z.need = bn_partial_floats(512);
    for (size_t ci = 0; ci < A.convs.size(); ++ci) {
        const ConvT& c = A.convs[ci];
        const ConvG& g = n->cg[ci];
        const size_t fwd = (size_t)g.M * c.cout, bwd = (size_t)B * g.H * g.W * c.cin;
        up(z.actmax, fwd);
        // slabs_max: the weight-gradient slabs of every convolution (the stem reads its channel-padded
        // image), direct and, where conv_wgrad takes it, Winograd.  The stem's own weight-gradient
        // kernel (stem_f32.hip) is NOT sized for: backward_stem uses it when its scratch happens to
        // fit and the direct kernel otherwise.  Sizing for it would move every plan's layout.
        const int x_cin = ci == 0 ? 4 : c.cin;
        up(z.slabs_max, wgrad_scratch_floats(
                            wgrad_args(B, g.H, g.W, x_cin, c.cout, c.k, c.k, c.stride, c.pad, c.cin)));
        if (x_cin == c.cin && wino_wgrad_on(c))
            up(z.slabs_max, wino_wgrad_scratch_floats(B, g.H, g.W, c.cin, c.cout));
        // ksplit_max: split-K scratch, only worthwhile for the small-M layers
        const size_t big = fwd > bwd ? fwd : bwd;
        if (big <= (size_t)6 * 1024 * 1024) up(z.ksplit_max, 8 * big);
        // need: per-tile column partials -- forward (conv output) and backward (the data gradient's
        // output = this conv's input) reductions ride on the GEMM epilogues (+ kConvMultiMax: a
        // position-class launch rounds every class up to whole tiles) -- or the BatchNorm kernels' own
        up(z.need, (size_t)(cdiv(g.M, 64) + kConvMultiMax) * 2 * c.cout);
        if (ci > 0) up(z.need, (size_t)(cdiv(B * g.H * g.W, 64) + kConvMultiMax) * 2 * c.cin);
        up(z.need, bn_partial_floats(c.cout));
    }
    // the heads' wide linears also use the wgrad slabs
    up(z.slabs_max, wgrad_scratch_floats(wgrad_args(B, 1, 1, A.feat + 128, 256, 1, 1, 1, 0, A.feat + 128)));
    return z;
}

// Placement: the order and sizes of these takes ARE the workspace layout (tests/golden/plan_layout.json).
// input image, padded stem weights, then y (pre-BN output, kept for backward) / z / stats of every
// convolution in block order, the max-pool output and its argmax behind the stem's
static void place_trunk(cilrs_net* n, Bump& bump) {
    const Arch& A = *n->A;
    auto place = [&](int ci) {
        ConvG& g = n->cg[ci];
        const int cout = A.convs[ci].cout;
        g.y = bump.take((size_t)g.M * cout);
        g.z = bump.take((size_t)g.M * cout);
        g.stats = bump.take(4 * cout);
    };
    n->x4 = bump.take((size_t)n->B * n->H * n->W * 4);
    n->w4 = bump.take((size_t)64 * 49 * 4);
    place(0);
    const size_t pooled = (size_t)n->B * n->H1 * n->W1 * 64;
    n->pool = bump.take(pooled);
    n->argmax_b = bump.take((pooled + 3) / 4) * sizeof(float);
    for (const BlockT& blk : A.blocks)
        for (int ci : {blk.conv1, blk.conv2, blk.conv3, blk.down})
            if (ci >= 0) place(ci);
}

static void place_heads(cilrs_net* n, Bump& bump) {
    const size_t B = n->B, comb = n->A->feat + 128;
    const int NC = n->A->ncmd;
    n->combined = bump.take(B * comb);
    n->s1 = bump.take(B * 128);
    n->p1 = bump.take(B * 256);
    n->p2 = bump.take(B * 256);
    for (int k = 0; k < NC; ++k) {
        n->h1[k] = bump.take(B * 256);
        n->h2[k] = bump.take(B * 256);
    }
    n->all_out = bump.take(NC * B * 4);
    n->dcombined = bump.take(B * comb);
    n->ds1 = bump.take(B * 128);
    n->dp1 = bump.take(B * 256);
    n->dp2 = bump.take(B * 256);
    for (int k = 0; k < NC; ++k) {
        n->dh1[k] = bump.take(B * 256);
        n->dh2[k] = bump.take(B * 256);
    }
    for (int k = 0; k <= NC; ++k) n->dcomb_part[k] = bump.take(B * comb);
    n->d_all = bump.take(NC * B * 4);
    n->speed_in = bump.take(B);
    n->cmd_b = bump.take(B * 2) * sizeof(float);
}

static void place_gradients(cilrs_net* n, Bump& bump, const PlanSizes& z) {
    n->gmax = z.gmax;
    for (int i = 0; i < kNumG; ++i) n->G[i] = bump.take(z.gmax);
}
static void place_scratch(cilrs_net* n, Bump& bump, const PlanSizes& z) {
    n->bn_partial = bump.take(z.need);
    n->bn_partial2 = bump.take(z.need);      // (the down-sample branch of a block, built beside conv1)
    // [0, 3 x 2048) the BatchNorm-backward coefficients; [3 x 2048, 5 x 2048) where the data-gradient-
    // only backward of a train-mode graph leaves the dgamma / dbeta by-products of its reductions
    n->bn_coef = bump.take(5 * 2048);
    n->slabs_floats = z.slabs_max;
    n->slabs = bump.take(z.slabs_max > 0 ? z.slabs_max : 4);
    n->ksplit_floats = z.ksplit_max;
    n->ksplit = bump.take(z.ksplit_max > 0 ? z.ksplit_max : 4);
    n->status_b = bump.take(64) * sizeof(float);
}

// (nothing placed: the tables point at the parameter arena and at the stats placed above)
static void fill_bn_tables(cilrs_net* n) {
    const Arch& A = *n->A;
    bn_stats_layout(A, n->bn_stats);
    n->bn_table.n = (int)A.convs.size();
    for (size_t ci = 0; ci < A.convs.size(); ++ci) {
        const BnT& b = A.bns[A.convs[ci].bn];
        n->bn_table.C[ci] = b.C;
        n->bn_table.gamma[ci] = (unsigned)b.gamma; n->bn_table.beta[ci] = (unsigned)b.beta;
        n->bn_table.rm[ci] = (unsigned)b.rm; n->bn_table.rv[ci] = (unsigned)b.rv;
        n->bn_table.stats[ci] = (unsigned)n->cg[ci].stats;
    }
}

// 16-bit inference arenas (every conv but the stem): folded weights, biases, activations
static void place_infer16(cilrs_net* n, Bump& bump, const PlanSizes& z) {
    const Arch& A = *n->A;
    size_t halfs = 0, floats = 0;
    n->f16_table.n = (int)A.convs.size() - 1;
    for (size_t ci = 1; ci < A.convs.size(); ++ci) {
        const ConvT& c = A.convs[ci];
        const int e = (int)ci - 1;
        n->f16_table.cout[e] = c.cout;
        n->f16_table.krow[e] = (unsigned)(c.k * c.k * c.cin);
        n->f16_table.w[e] = (unsigned)c.w;
        n->f16_table.stats[e] = (unsigned)n->cg[ci].stats;
        n->f16_table.w16[e] = (unsigned)halfs;
        n->f16_table.bias[e] = (unsigned)floats;
        halfs += (size_t)c.cout * c.k * c.k * c.cin;
        floats += (size_t)c.cout;
    }
    n->f16_w = bump.take((halfs + 1) / 2);
    n->f16_bias = bump.take(floats);
    n->stem16_w = bump.take(64 * 224 / 2);
    n->stem16_b = bump.take(64);
    n->f16_act_floats = (z.actmax + 1) / 2;                              // largest trunk tensor
    for (int k = 0; k < 5; ++k) n->f16_act[k] = bump.take(n->f16_act_floats);
}

// CILRS_PLAN_BF16_TRAIN: 16-bit shadows of the training tensors
static void place_bf16_shadows(cilrs_net* n, Bump& bump, const PlanSizes& z) {
    const Arch& A = *n->A;
    n->w16_all = bump.take((A.arena_floats + 1) / 2);
    size_t halfs = 0, sl = 0;
    for (size_t ci = 1; ci < A.convs.size(); ++ci) {
        const ConvT& c = A.convs[ci];
        const int e = n->tr_table.n++;
        n->tr_table.cout[e] = c.cout; n->tr_table.k[e] = c.k; n->tr_table.cin[e] = c.cin;
        n->tr_table.w[e] = (unsigned)c.w;
        n->tr_table.wT[e] = (unsigned)halfs;
        n->tr_table.tile_begin[e + 1] =
            n->tr_table.tile_begin[e] + c.k * c.k * (c.cout / 32) * (c.cin / 32);
        n->wT16_off[ci] = halfs;
        halfs += ((size_t)c.cout * c.k * c.k * c.cin + 7) / 8 * 8;
        n->z16[ci] = bump.take(((size_t)n->cg[ci].M * c.cout + 1) / 2);
        const size_t f = wgrad_f16_scratch_floats(wgrad16_args(n, c, n->cg[ci]));
        if (f > sl) sl = f;
    }
    n->wT16 = bump.take((halfs + 1) / 2);
    n->pool16 = bump.take(((size_t)n->B * n->H1 * n->W1 * 64 + 1) / 2);
    for (int i = 0; i < kNumG; ++i) n->G16[i] = bump.take((z.gmax + 1) / 2);
    n->slabs16_floats = sl;
    n->slabs16 = bump.take(sl > 0 ? sl : 4);
}

// Winograd filter images of the fp32 train plan's layers (cilrs_net::wino_slot).  wino_prepare sets
// the kernels' attributes here, at plan build: outside any capture.
static int place_wino(cilrs_net* n, Bump& bump) {
    const Arch& A = *n->A;
    WinoWeightTable& t = n->wino_table;
    static const int wino_env = env_int("CILRS_WINO", 1);
    if (n->bf16_train || !wino_env) return 0;
    size_t floats = 0;
    for (size_t ci = 1; ci < A.convs.size(); ++ci) {
        const ConvT& c = A.convs[ci];
        const ConvG& g = n->cg[ci];
        if (!wino_supported(c.cin, c.cout, c.k, c.stride, c.pad) ||
            !wino_supported(c.cout, c.cin, c.k, c.stride, c.pad) || c.cin % 32 != 0 ||
            c.cin > 256 || c.cout > 256)
            continue;
        // one 64-tile x 64-channel block per CU: below ~half a chip of blocks the
        // implicit GEMM (split-K, smaller tiles) wins (tools/wino_bench.py)
        const int blocks = wino_groups(n->B, g.H, g.W) * (std::min(c.cin, c.cout) / 64);
        if (wino_env == 1 && blocks < 128) continue;
        const int e = t.n++;
        t.K[e] = c.cout; t.C[e] = c.cin; t.w[e] = (unsigned)c.w;
        t.u[e] = (unsigned)floats; floats += wino_weight_floats(c.cout, c.cin);
        t.ud[e] = (unsigned)floats; floats += wino_weight_floats(c.cout, c.cin);
        t.blk_begin[e + 1] = t.blk_begin[e] + (c.cout / 8) * (c.cin / 32);
        n->wino_slot[ci] = e;
    }
    CILRS_CHECK(floats < (1ull << 32), "Winograd filter images exceed 32-bit offsets");
    if (t.n == 0) return 0;
    n->wino_base = bump.take(floats);
    return wino_prepare();
}

// the persistent single-frame launch (infer_b1.hip): stage table, barrier counters, stamps, slabs
static void place_b1(cilrs_net* n, Bump& bump) {
    const Arch& A = *n->A;
    n->b1_table = bump.take(kB1MaxStages * sizeof(B1Stage) / sizeof(float));
    n->b1_sync = bump.take(kB1SyncInts);
    n->b1_cmd = bump.take(16);
    n->b1_stamps = bump.take(2 * (10 * (kB1MaxStages + 1) + kB1MaxStages * 512));
    // split-K partial tiles: up to 4 slices of the largest [16-row tiles][Cout] output, twice
    // (a stage may hold two convolutions)
    size_t big = 0;
    for (size_t ci = 1; ci < A.convs.size(); ++ci) {
        const size_t o = (size_t)cdiv(n->cg[ci].M, 16) * 16 * A.convs[ci].cout;
        if (o > big) big = o;
    }
    n->b1_slab_floats = 2 * 4 * big;
    n->b1_slabs = bump.take(n->b1_slab_floats);
}

int cilrs_net_create_ex(int variant, int batch, int height, int width, unsigned flags,
                        cilrs_net** out) {
    CILRS_CHECK(out != nullptr, "cilrs_net_create: out is NULL");
    CILRS_CHECK((flags & ~1u) == 0, "cilrs_net_create: unknown flags 0x%x", flags);
    CILRS_CHECK(variant_ok(variant), "cilrs_net_create: variant %d out of range", variant);
    // 17: every one of the five stride-2 steps (stem, max-pool, layer2-4) still reads a map of at
    // least two rows and columns, as at 32 x 32 (17 -> 9 -> 5 -> 3 -> 2 -> 1)
    CILRS_CHECK(batch >= 1 && height >= 17 && width >= 17, "cilrs_net_create: bad geometry %d %d %d",
                batch, height, width);
    const Arch& A = arch(variant);
    CILRS_CHECK((int)A.convs.size() <= kMaxConvs, "too many convolutions for the BN tables");
    std::unique_ptr<cilrs_net> n(new cilrs_net());      // (every failure below frees it)
    n->A = &A;
    n->B = batch; n->H = height; n->W = width;
    n->bf16_train = (flags & 1u) != 0;
    if (plan_geometry(n.get())) return 1;
    const PlanSizes z = plan_sizes(n.get());
    Bump bump;
    place_trunk(n.get(), bump);
    place_heads(n.get(), bump);
    place_gradients(n.get(), bump, z);
    place_scratch(n.get(), bump, z);
    fill_bn_tables(n.get());
    place_infer16(n.get(), bump, z);
    if (n->bf16_train) place_bf16_shadows(n.get(), bump, z);
    if (place_wino(n.get(), bump)) return 1;
    // (the persistent kernel is built for the reference's trunk and 4 commands)
    if (batch == 1 && A.variant == 0 && A.ncmd == 4) place_b1(n.get(), bump);
    n->ws_bytes = bump.off * sizeof(float);
    *out = n.release();
    return 0;
}

void cilrs_net_destroy(cilrs_net* net) { delete net; }
size_t cilrs_net_workspace_bytes(const cilrs_net* net) { return net ? net->ws_bytes : 0; }
size_t cilrs_net_status_offset(const cilrs_net* net) { return net ? net->status_b : 0; }

int cilrs_net_activation_info(const cilrs_net* net, int conv, size_t* y_offset, size_t* z_offset,
                              size_t* numel, int* channels) {
    CILRS_CHECK(net != nullptr, "activation_info: net is NULL");
    // conv -1: the max-pool output (input of the first residual block)
    if (conv == -1) {
        if (y_offset) *y_offset = net->pool;
        if (z_offset) *z_offset = net->pool;
        if (numel) *numel = (size_t)net->B * net->H1 * net->W1 * 64;
        if (channels) *channels = 64;
        return 0;
    }
    CILRS_CHECK(conv >= 0 && conv < (int)net->cg.size(), "activation_info: conv %d out of range", conv);
    const ConvG& g = net->cg[conv];
    if (y_offset) *y_offset = g.y;
    if (z_offset) *z_offset = g.z;
    if (numel) *numel = (size_t)g.M * net->A->convs[conv].cout;
    if (channels) *channels = net->A->convs[conv].cout;
    return 0;
}

// where convolution `conv`'s BatchNorm keeps its 4*C floats mean | rstd | scale | shift in the
// workspace (floats), the rows M it sees in this plan, and its layer number (cilrs_variant_bn_info)
int cilrs_net_bn_layer_info(const cilrs_net* net, int conv, size_t* stats_offset, int* channels,
                            int* rows, int* bn_index) {
    CILRS_CHECK(net != nullptr, "bn_layer_info: net is NULL");
    CILRS_CHECK(conv >= 0 && conv < (int)net->cg.size(), "bn_layer_info: conv %d out of range", conv);
    if (stats_offset) *stats_offset = net->cg[conv].stats;
    if (channels) *channels = net->A->convs[conv].cout;
    if (rows) *rows = net->cg[conv].M;
    if (bn_index) *bn_index = net->A->convs[conv].bn;
    return 0;
}

int cilrs_net_pool_argmax_info(const cilrs_net* net, size_t* byte_offset, size_t* numel) {
    CILRS_CHECK(net != nullptr, "pool_argmax_info: net is NULL");
    if (byte_offset) *byte_offset = net->argmax_b;
    if (numel) *numel = (size_t)net->B * net->H1 * net->W1 * 64;
    return 0;
}

int cilrs_net_head_activation_info(const cilrs_net* net, int which, int branch, size_t* offset,
                                   int* rows, int* cols, int* ld) {
    CILRS_CHECK(net != nullptr, "head_activation_info: net is NULL");
    CILRS_CHECK(which >= 0 && which <= 5, "head_activation_info: tensor %d out of range", which);
    CILRS_CHECK(which < 4 || (branch >= 0 && branch < net->A->ncmd),
                "head_activation_info: branch %d out of range", branch);
    const int comb = net->A->feat + 128;
    const size_t off[6] = {net->s1, net->combined + (size_t)net->A->feat, net->p1, net->p2,
                           which == 4 ? net->h1[branch] : 0, which == 5 ? net->h2[branch] : 0};
    if (offset) *offset = off[which];
    if (rows) *rows = net->B;
    if (cols) *cols = which < 2 ? 128 : 256;
    if (ld) *ld = which == 1 ? comb : which == 0 ? 128 : 256;
    return 0;
}

int cilrs_net_infer16_conv_info(const cilrs_net* net, int conv, size_t* w16_offset,
                                size_t* bias_offset, size_t* w16_numel, int* channels,
                                int* folded_half) {
    CILRS_CHECK(net != nullptr, "infer16_conv_info: net is NULL");
    CILRS_CHECK(conv >= 0 && conv < (int)net->cg.size(), "infer16_conv_info: conv %d out of range", conv);
    const ConvT& c = net->A->convs[conv];
    if (conv == 0) {         // the stem's [64][7][8][4] layout (kw padded 7 -> 8, c 3 -> 4)
        if (w16_offset) *w16_offset = net->stem16_w * sizeof(float);
        if (bias_offset) *bias_offset = net->stem16_b * sizeof(float);
        if (w16_numel) *w16_numel = 64 * 224;
    } else {
        const int e = conv - 1;
        if (w16_offset) *w16_offset = net->f16_w * sizeof(float) + (size_t)net->f16_table.w16[e] * 2;
        if (bias_offset) *bias_offset = (net->f16_bias + net->f16_table.bias[e]) * sizeof(float);
        if (w16_numel) *w16_numel = (size_t)c.cout * c.k * c.k * c.cin;
    }
    if (channels) *channels = c.cout;
    // (what the arenas hold now: a later fp32 eval_prep of changed weights invalidates them)
    if (folded_half) *folded_half = net->fold_key != 0 ? net->fold_half : 0;
    return 0;
}

int cilrs_net_infer16_io_info(const cilrs_net* net, size_t* x4_offset, size_t* x4_numel,
                              size_t* combined_offset, int* combined_ld, int* features) {
    CILRS_CHECK(net != nullptr, "infer16_io_info: net is NULL");
    if (x4_offset) *x4_offset = net->x4 * sizeof(float);
    if (x4_numel) *x4_numel = (size_t)net->B * net->H * net->W * 4;
    if (combined_offset) *combined_offset = net->combined * sizeof(float);
    if (combined_ld) *combined_ld = net->A->feat + 128;
    if (features) *features = net->A->feat;
    return 0;
}

int cilrs_net_set_weights_key(cilrs_net* net, uint64_t key) {
    CILRS_CHECK(net != nullptr, "set_weights_key: net is NULL");
    net->weights_key = key;
    return 0;
}

int cilrs_dropout(float* a, int rows, int cols, int ld, float p, uint64_t seed, int site,
                  void* stream) {
    CILRS_CHECK(a && rows >= 1 && cols >= 1 && ld >= cols && site >= 0 && site <= 9,
                "dropout: bad argument");
    return launch_dropout(a, rows, cols, ld, p, seed, (unsigned long long)site,
                          reinterpret_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// Weight-derived eval state, cached across calls: the channel-padded stem weights and every
// layer's BatchNorm scale/shift (prep_key, eval_prep), and for half = 1 / 2 the 16-bit folded
// weights / biases (fold_key, fold_half, fold_prep).  Current while the caller's weights key is set
// and unchanged and the buffers are the ones the state was computed from.
static bool eval_state_current(const cilrs_net* net, const cilrs_buffers* bufs, int half) {
    const bool prep = net->weights_key != 0 && net->prep_key == net->weights_key &&
                      net->prep_bufs[0] == (const void*)bufs->params &&
                      net->prep_bufs[1] == (const void*)bufs->bn_running &&
                      net->prep_bufs[2] == (const void*)bufs->workspace;
    return prep && (!half || (net->fold_key == net->weights_key && net->fold_half == half));
}

// eval: running statistics -> per-channel scale/shift (one launch for all 36 layers), folded with
// ReLU / residual add into each conv's epilogue; no pre-BN tensor is stored
static int eval_prep(cilrs_net* net, const cilrs_buffers* bufs, hipStream_t s) {
    if (eval_state_current(net, bufs, 0)) return 0;
    const Arch& A = *net->A;
    float* ws = reinterpret_cast<float*>(bufs->workspace);
    RUN(net, "transform", 0.0, 0.0, s,
        launch_pad_cin3_to_4(bufs->params + A.convs[0].w, ws + net->w4, 64 * 49, s));
    RUN(net, "bn_fwd.eval", 0.0, 0.0, s,
        launch_bn_eval_stats_all(net->bn_table, bufs->params, bufs->bn_running, ws, 1e-5f, s));
    net->prep_key = net->weights_key;
    net->prep_bufs[0] = bufs->params; net->prep_bufs[1] = bufs->bn_running;
    net->prep_bufs[2] = bufs->workspace;
    net->fold_key = 0;
    return 0;
}

// 16-bit eval: BatchNorm folded into the fp16 / bf16 trunk and stem weights (reads the scale/shift
// of eval_prep, which runs first)
static int fold_prep(cilrs_net* net, const cilrs_buffers* bufs, int half, hipStream_t s) {
    if (eval_state_current(net, bufs, half)) return 0;
    const Arch& A = *net->A;
    float* ws = reinterpret_cast<float*>(bufs->workspace);
    const int bf16 = half == 2;
    RUN(net, "transform", 0.0, 0.0, s,
        launch_fold_bn_f16(net->f16_table, bufs->params, ws,
                           reinterpret_cast<cilrs_half*>(ws + net->f16_w), ws + net->f16_bias, bf16,
                           s));
    RUN(net, "transform", 0.0, 0.0, s,
        launch_fold_stem_f16(bufs->params + A.convs[0].w, ws + net->cg[0].stats,
                             h16(ws, net->stem16_w), ws + net->stem16_b, bf16, s));
    net->fold_key = net->weights_key;
    net->fold_half = half;
    return 0;
}

// Entries of the plan's Winograd table whose layers lie in trunk groups [g0, g1) (1 = layer1 ...;
// the table is in layer order, so this is a contiguous run), as a table of its own
static WinoWeightTable wino_subtable(const cilrs_net* net, int g0, int g1) {
    const Arch& A = *net->A;
    const WinoWeightTable& t = net->wino_table;
    WinoWeightTable o;
    memset(&o, 0, sizeof(o));
    for (size_t ci = 0; ci < A.convs.size(); ++ci) {
        const int e = net->wino_slot[ci];
        if (e < 0 || A.convs[ci].group < g0 || A.convs[ci].group >= g1) continue;
        const int k = o.n++;
        o.K[k] = t.K[e]; o.C[k] = t.C[e]; o.w[k] = t.w[e]; o.u[k] = t.u[e]; o.ud[k] = t.ud[e];
        o.blk_begin[k + 1] = o.blk_begin[k] + (t.blk_begin[e + 1] - t.blk_begin[e]);
    }
    return o;
}

// Trunk of the graph-keeping forwards -- the fp32 train step, the bf16 training mode and the frozen
// eval-with-grad forward: BatchNorm on the batch statistics (train) or the running ones (frozen,
// scale/shift from eval_prep); keeps every activation the backward pass reads (y, z, the max-pool
// argmax).  *feat: the last feature map, or nullptr when it is already pooled into `combined`.
// ft_groups > 0 (fine-tuning): the first ft_groups trunk groups were already computed in eval mode
// (trunk_fwd_eval32 up to that group, last output in `start`); this function builds the rest.
// bn_acc (cilrs_net_forward_bn_stats; fp32 train mode, no frozen prefix): the BatchNorm
// re-estimation table -- every layer's batch statistics are added to it and the running buffers /
// num_batches_tracked are left alone; every launch is otherwise the train step's.
static int trunk_fwd_graph(cilrs_net* net, const cilrs_buffers* bufs, int train, bool frozen,
                           hipStream_t s, const float** feat, int ft_groups = 0,
                           const float* start = nullptr, double* bn_acc = nullptr) {
    const Arch& A = *net->A;
    float* ws = reinterpret_cast<float*>(bufs->workspace);
    const float* P = bufs->params;
    float* R = bufs->bn_running;
    long long* const NBT = reinterpret_cast<long long*>(bufs->bn_nbt);
    const int B = net->B;
    const float eps = 1e-5f, mom = 0.1f;
    const bool bf16t = train && net->bf16_train;      // trunk convolutions on the bf16 matrix pipe

    // (residual: fp32 tensor, or the bf16 identity in the bf16 training mode)
    auto bn = [&](int ci, const void* residual_v, int relu, int pre_nblk, hipStream_t st = nullptr,
                  bool side_branch = false) -> int {
        if (st == nullptr) st = s;
        float* const partial = ws + (side_branch ? net->bn_partial2 : net->bn_partial);
        const float* residual = reinterpret_cast<const float*>(residual_v);
        const ConvT& c = A.convs[ci];
        const ConvG& g = net->cg[ci];
        const BnT& b = A.bns[c.bn];
        const double bytes = 4.0 * g.M * c.cout * (residual ? 4.0 : 3.0);
        if (bf16t) {         // 16-bit tensors: residual is the bf16 identity
            RUN(net, std::string("bn_fwd.") + kGroupName[c.group], 0.0, bytes / 2.0, st,
                launch_bn16_train_fwd(y16_of(net, ws, ci), g.M, c.cout, P + b.gamma, P + b.beta,
                                      R + b.rm, R + b.rv,
                                      reinterpret_cast<long long*>(bufs->bn_nbt) + c.bn, mom, eps,
                                      residual, relu, ws + g.stats, partial,
                                      h16(ws, net->z16[ci]), pre_nblk, st));
        } else if (train) {
            RUN(net, std::string("bn_fwd.") + kGroupName[c.group], 0.0, bytes, st,
                launch_bn_train_fwd(ws + g.y, g.M, c.cout, P + b.gamma, P + b.beta,
                                    bn_acc ? nullptr : R + b.rm, bn_acc ? nullptr : R + b.rv,
                                    bn_acc ? nullptr : NBT + c.bn, mom, eps, residual, relu,
                                    ws + g.stats, partial, ws + g.z, pre_nblk, st, nullptr,
                                    bn_acc ? bn_acc + net->bn_stats.head[c.bn] : nullptr,
                                    bn_acc ? bn_acc + net->bn_stats.sums[c.bn] : nullptr));
        } else {
            RUN(net, std::string("bn_fwd.") + kGroupName[c.group], 0.0, bytes, st,
                launch_bn_eval_fwd(ws + g.y, g.M, c.cout, P + b.gamma, P + b.beta, R + b.rm,
                                   R + b.rv, eps, residual, relu, ws + g.stats, ws + g.z, st));
        }
        return 0;
    };

    // ---- stem: conv7x7/s2 + BN + ReLU + maxpool3x3/s2 ----
    // this step's weight images -- the Winograd-transformed filters (forward + data-gradient
    // forms), in the bf16 mode the 16-bit arena and the transposed, tap-flipped copies the data
    // gradients read -- depend on the parameters only: they are built on the side stream while
    // the stem and the max-pool run (memory-bound launches beside a matrix-pipe-bound one); the
    // first residual block waits for them
    {
        hipStream_t ts = s;
        const bool fork = use_overlap(net) && (net->wino_table.n || bf16t);
        if (fork) {
            if (side_fork(net, s)) return 1;
            ts = net->side[0];
        }
        if (net->wino_table.n && ft_groups == 0) {
            RUN(net, "transform", 0.0, 4.0 * 4.6 * (double)net->wino_table.blk_begin[net->wino_table.n] * 256, ts,
                launch_wino_weights_all(net->wino_table, P, ws + net->wino_base, ts));
        } else if (net->wino_table.n) {        // (the frozen layers' images are cached: ft_prep)
            const WinoWeightTable t = wino_subtable(net, ft_groups, 5);
            if (t.n)
                RUN(net, "transform", 0.0, 4.0 * 4.6 * (double)t.blk_begin[t.n] * 256, ts,
                    launch_wino_weights_all(t, P, ws + net->wino_base, ts));
        }
        if (bf16t) {
            RUN(net, "transform", 0.0, 6.0 * A.arena_floats, ts,
                launch_f32_to_f16(P, h16(ws, net->w16_all), A.arena_floats, 1, ts));
            RUN(net, "transform", 0.0, 0.0, ts,
                launch_transpose_flip_f16_all(net->tr_table, P, h16(ws, net->wT16), 1, ts));
        }
        if (fork) {
            CILRS_HIP(hipEventRecord(net->wprep_ev, ts));
            net->wprep_pending = true;
        }
    }
    int nb = 0;                             // batch statistics fused into the conv epilogue
    if (ft_groups > 0) {
        // (frozen stem: nothing of it is kept, the max-pool of the prefix ran without an argmax)
    } else if (const int srows = stem_f32_rows(B, net->H, net->W)) {
        // (weights in registers, k = 7 x 22 instead of 13 x 16: stem_f32.hip)
        RUN(net, "conv_fwd.stem", 2.0 * net->cg[0].M * 64 * 147,
            16.0 * B * net->H * net->W + 4.0 * net->cg[0].M * 64, s,
            launch_stem_f32(ws + net->x4, P + A.convs[0].w, ws + net->cg[0].y,
                            ws + net->bn_partial, B, net->H, net->W, s));
        nb = srows;
    } else if (conv_fwd(net, A.convs[0], net->cg[0], ws + net->x4, 4, ws + net->w4,
                        ws + net->cg[0].y, ws, s, &nb)) {
        return 1;
    }
    // stem BatchNorm: statistics only -- its apply + ReLU is fused into the max-pool, the post-BN
    // tensor (144 MB at B=128) is never written.  (frozen: eval_prep derived every layer's scale /
    // shift from the running statistics; the other BatchNorms re-derive theirs in the bn() apply)
    if (!frozen && ft_groups == 0) {
        const ConvT& c0 = A.convs[0];
        const ConvG& g0 = net->cg[0];
        const BnT& b0 = A.bns[c0.bn];
        RUN(net, "bn_fwd.stem", 0.0, 0.0, s,
            launch_bn_train_fwd(ws + g0.y, g0.M, c0.cout, P + b0.gamma, P + b0.beta,
                                bn_acc ? nullptr : R + b0.rm, bn_acc ? nullptr : R + b0.rv,
                                bn_acc ? nullptr : NBT + c0.bn, mom, eps,
                                nullptr, 1, ws + g0.stats, ws + net->bn_partial, nullptr, nb,
                                s, nullptr, bn_acc ? bn_acc + net->bn_stats.head[c0.bn] : nullptr,
                                bn_acc ? bn_acc + net->bn_stats.sums[c0.bn] : nullptr));
    }
    unsigned char* argmax = reinterpret_cast<unsigned char*>(bufs->workspace) + net->argmax_b;
    if (ft_groups == 0)
        RUN(net, "maxpool", 0.0, 4.0 * net->cg[0].M * 64 * 1.25, s,
            launch_bn_relu_maxpool_fwd(ws + net->cg[0].y, ws + net->cg[0].stats, ws + net->pool,
                                       argmax, B, net->H0, net->W0, 64, s,
                                       bf16t ? (void*)h16(ws, net->pool16) : nullptr));
    // (this step's weight images were requested before the stem, on the side stream)
    if (net->wprep_pending) {
        CILRS_HIP(hipStreamWaitEvent(s, net->wprep_ev, 0));
        net->wprep_pending = false;
    }
    // ---- residual blocks: BasicBlock conv-BN-ReLU-conv-BN-(+id)-ReLU, Bottleneck with a third
    //      conv-BN pair; the identity (or downsample branch) joins at the last BatchNorm ----
    const float* cur = ft_groups > 0 ? start : ws + net->pool;
    const cilrs_half* cur16 = h16(ws, net->pool16);
    for (const BlockT& blk : A.blocks) {
        if (A.convs[blk.conv1].group < ft_groups) continue;
        const int chain[3] = {blk.conv1, blk.conv2, blk.conv3};
        const int nchain = blk.conv3 >= 0 ? 3 : 2;
        const void* identity = bf16t ? (const void*)cur16 : (const void*)cur;
        const float* x = cur;
        const cilrs_half* x16 = cur16;
        // The down-sample branch (1x1 / stride-2 convolution + BatchNorm: three short launches
        // that leave most of the chip idle) depends on the block's input only: it is built on
        // the side stream beside conv1 / bn1 / conv2, with column-partial scratch of its own
        // and no split-K scratch; the block's last BatchNorm -- which adds it -- waits for it.
        bool branch_pending = false;
        const bool branch_aside = blk.down >= 0 && use_overlap(net);
        auto down_branch = [&](hipStream_t st, bool aside) -> int {
            const ConvT& cd = A.convs[blk.down];
            const ConvG& gd = net->cg[blk.down];
            int nbd = 0;
            // (1: beside the main stream, own partial scratch; 2: on the main stream -- in BOTH
            //  cases without split-K, so that the plan, hence the summation order, of this
            //  convolution does not depend on whether the streams overlap)
            net->side_branch = aside ? 1 : 2;
            int rc = bf16t ? conv_fwd16(net, cd, gd, cur16, ws, st, &nbd)
                           : conv_fwd(net, cd, gd, cur, cd.cin, P + cd.w, ws + gd.y, ws, st, &nbd);
            net->side_branch = 0;
            if (rc) return 1;
            if (bn(blk.down, nullptr, 0, nbd, st, aside)) return 1;
            identity = bf16t ? (const void*)h16(ws, net->z16[blk.down]) : (const void*)(ws + gd.z);
            return 0;
        };
        if (branch_aside) {
            if (side_fork(net, s)) return 1;            // the side stream sees the block's input
            if (down_branch(net->side[0], true)) return 1;
            CILRS_HIP(hipEventRecord(net->branch_ev, net->side[0]));
            branch_pending = true;
        }
        for (int i = 0; i < nchain; ++i) {
            const ConvT& c = A.convs[chain[i]];
            const ConvG& g = net->cg[chain[i]];
            nb = 0;
            if (bf16t) {
                if (conv_fwd16(net, c, g, x16, ws, s, &nb)) return 1;
            } else {
                if (conv_fwd(net, c, g, x, c.cin, P + c.w, ws + g.y, ws, s, &nb)) return 1;
            }
            if (i == 0 && blk.down >= 0 && !branch_aside) {
                // (issued after conv1 so that both convolutions reading `cur` are adjacent)
                if (bn(chain[0], nullptr, 1, nb)) return 1;
                if (down_branch(s, false)) return 1;
            } else if (i + 1 < nchain) {
                if (bn(chain[i], nullptr, 1, nb)) return 1;
            } else {
                if (branch_pending) {
                    CILRS_HIP(hipStreamWaitEvent(s, net->branch_ev, 0));
                    branch_pending = false;
                }
                if (bn(chain[i], identity, 1, nb)) return 1;
            }
            x = ws + g.z;
            x16 = h16(ws, net->z16[chain[i]]);
        }
        cur = x;
        cur16 = x16;
    }
    if (bf16t) {         // features from the bf16 feature map
        RUN(net, "heads_fwd", 0.0, 0.0, s,
            launch_avgpool_f16(cur16, ws + net->combined, B, net->featHW, A.feat,
                               A.feat + 128, 1, s));
        cur = nullptr;
    }
    *feat = cur;
    return 0;
}

// fp32 eval trunk: BatchNorm (scale/shift from eval_prep) folded into the conv epilogues
// groups < 5 (fine-tuning): only the first `groups` trunk groups (1 = the stem + max-pool alone);
// *feat is then the last tensor written.
static int trunk_fwd_eval32(cilrs_net* net, const cilrs_buffers* bufs, hipStream_t s,
                            const float** feat, int groups = 5) {
    const Arch& A = *net->A;
    float* ws = reinterpret_cast<float*>(bufs->workspace);
    const float* P = bufs->params;
    const int B = net->B;
    if (conv_fwd(net, A.convs[0], net->cg[0], ws + net->x4, 4, ws + net->w4,
                 ws + net->cg[0].z, ws, s, nullptr, ws + net->cg[0].stats, 1)) return 1;
    RUN(net, "maxpool", 0.0, 4.0 * net->cg[0].M * 64 * 1.25, s,
        launch_maxpool_fwd(ws + net->cg[0].z, ws + net->pool, nullptr, B, net->H0,
                           net->W0, 64, s));
    // a layer with few output pixels (single-frame inference) takes the one-launch
    // latency kernel (conv_small.hip) instead of split-K implicit GEMM + reduce
    auto conv_eval = [&](const ConvT& c, const ConvG& g, const float* x, float* y, int relu,
                         const float* addend, int relu_post) -> int {
        // one 16-wave block per 16x16 tile: worth it while every block gets its own CU
        // CILRS_SMALL_BLOCKS / CILRS_SMALL_K: routing thresholds for tools/infer_ab.py
        static const int max_blocks =
            experiment_env("CILRS_SMALL_BLOCKS", kSmallConvBlocks);
        static const int max_k = experiment_env("CILRS_SMALL_K", kSmallConvK);
        if (cdiv(g.M, 16) * (c.cout / 16) > max_blocks || c.cin % 16 != 0 ||
            c.k * c.k * c.cin > max_k)
            return conv_fwd(net, c, g, x, c.cin, P + c.w, y, ws, s, nullptr, ws + g.stats,
                            relu, addend, relu_post);
        ConvSmallArgs a;
        memset(&a, 0, sizeof(a));
        a.x = x; a.w = P + c.w; a.y = y;
        a.scale = ws + g.stats + 2 * c.cout; a.shift = ws + g.stats + 3 * c.cout;
        a.addend = addend; a.relu = relu; a.relu_post = relu_post;
        a.N = B; a.H = g.H; a.W = g.W; a.Cin = c.cin; a.Ho = g.Ho; a.Wo = g.Wo;
        a.Cout = c.cout; a.K = c.k; a.stride = c.stride; a.pad = c.pad;
        RUN(net, std::string("conv_fwd.") + kGroupName[c.group], conv_flops(c, g), 0.0, s,
            launch_conv_small(a, s));
        return 0;
    };
    const float* cur = ws + net->pool;
    for (const BlockT& blk : A.blocks) {
        if (A.convs[blk.conv1].group >= groups) break;
        const ConvT& c1 = A.convs[blk.conv1];
        const ConvT& c2 = A.convs[blk.conv2];
        const ConvG& g1 = net->cg[blk.conv1];
        const ConvG& g2 = net->cg[blk.conv2];
        if (conv_eval(c1, g1, cur, ws + g1.z, 1, nullptr, 0)) return 1;
        const float* identity = cur;
        if (blk.down >= 0) {
            const ConvT& cd = A.convs[blk.down];
            const ConvG& gd = net->cg[blk.down];
            if (conv_eval(cd, gd, cur, ws + gd.z, 0, nullptr, 0)) return 1;
            identity = ws + gd.z;
        }
        if (blk.conv3 >= 0) {      // Bottleneck: 1x1 -> 3x3 -> 1x1 (+ identity)
            const ConvT& c3 = A.convs[blk.conv3];
            const ConvG& g3 = net->cg[blk.conv3];
            if (conv_eval(c2, g2, ws + g1.z, ws + g2.z, 1, nullptr, 0)) return 1;
            if (conv_eval(c3, g3, ws + g2.z, ws + g3.z, 0, identity, 1)) return 1;
            cur = ws + g3.z;
        } else {
            if (conv_eval(c2, g2, ws + g1.z, ws + g2.z, 0, identity, 1)) return 1;
            cur = ws + g2.z;
        }
    }
    *feat = cur;
    return 0;
}

// ---- fp16 / bf16 trunk (BASELINE config 5; half = 1 / 2): BatchNorm folded into 16-bit weights
//      (fold_prep), 16-bit NHWC activations, v_mfma_f32_32x32x16_f16 with fp32 accumulation
//      (infer_f16.hip).  The features end up pooled into `combined` (*feat = nullptr). ----
static int trunk_fwd_eval16(cilrs_net* net, const cilrs_buffers* bufs, int half, hipStream_t s,
                            const float** feat) {
    const Arch& A = *net->A;
    float* ws = reinterpret_cast<float*>(bufs->workspace);
    const int B = net->B;
    const cilrs_half* w16 = reinterpret_cast<const cilrs_half*>(ws + net->f16_w);
    const float* b16 = ws + net->f16_bias;
    const int bf16 = half == 2;
    cilrs_half* act[5];
    for (int k = 0; k < 5; ++k) act[k] = reinterpret_cast<cilrs_half*>(ws + net->f16_act[k]);
    // stem on the 16-bit pipe too (stem_f16.hip): conv 7x7/s2 + folded BN + ReLU from the
    // channel-padded fp32 image, 16-bit output parked in the (otherwise unused) fp32 stem
    // buffer, then the 16-bit max-pool straight into the first activation buffer
    {
        const ConvG& g0 = net->cg[0];
        RUN(net, "conv_fwd.stem", 2.0 * g0.M * 64 * 147, 16.0 * B * net->H * net->W +
            2.0 * g0.M * 64, s,
            launch_stem_f16(ws + net->x4, h16(ws, net->stem16_w), ws + net->stem16_b,
                            h16(ws, g0.z), B, net->H, net->W, bf16, s));
        RUN(net, "maxpool", 0.0, 2.0 * g0.M * 64 * 1.25, s,
            launch_maxpool_f16(h16(ws, g0.z), act[0], B, net->H0, net->W0, 64, bf16, s));
    }
    int ic = 0;                                  // index of the buffer holding `cur`
    auto conv16 = [&](int ci, const cilrs_half* x, const cilrs_half* residual,
                      cilrs_half* y, int relu) -> int {
        const ConvT& c = A.convs[ci];
        const ConvG& g = net->cg[ci];
        ConvF16Args a;
        memset(&a, 0, sizeof(a));
        a.x = x; a.w = w16 + net->f16_table.w16[ci - 1];
        a.bias = b16 + net->f16_table.bias[ci - 1];
        a.residual = residual; a.y = y; a.bf16 = bf16;
        a.N = B; a.H = g.H; a.W = g.W; a.Cin = c.cin; a.Ho = g.Ho; a.Wo = g.Wo;
        a.Cout = c.cout; a.K = c.k; a.stride = c.stride; a.pad = c.pad; a.relu = relu;
        RUN(net, std::string("conv_fwd.") + kGroupName[c.group], conv_flops(c, g),
            conv_bytes(net, c, g, 2, 2, 2, false, residual ? 2.0 : 1.0), s, launch_conv_f16(a, s));
        return 0;
    };
    for (const BlockT& blk : A.blocks) {
        // five rotating buffers: block input, two intermediates, projected identity, output
        const int it1 = (ic + 1) % 5, it2 = (ic + 2) % 5, iid = (ic + 3) % 5,
                  io = (ic + 4) % 5;
        if (conv16(blk.conv1, act[ic], nullptr, act[it1], 1)) return 1;
        const cilrs_half* identity = act[ic];
        if (blk.down >= 0) {
            if (conv16(blk.down, act[ic], nullptr, act[iid], 0)) return 1;
            identity = act[iid];
        }
        if (blk.conv3 >= 0) {
            if (conv16(blk.conv2, act[it1], nullptr, act[it2], 1)) return 1;
            if (conv16(blk.conv3, act[it2], identity, act[io], 1)) return 1;
        } else {
            if (conv16(blk.conv2, act[it1], identity, act[io], 1)) return 1;
        }
        ic = io;
    }
    RUN(net, "heads_fwd", 0.0, 0.0, s,
        launch_avgpool_f16(act[ic], ws + net->combined, B, net->featHW, A.feat,
                           A.feat + 128, bf16, s));
    *feat = nullptr;
    return 0;
}

// Heads: speed encoder, the command branches and the speed predictor.  `feat`: the trunk's last
// feature map, or nullptr when its features are already pooled into `combined`.  graph: a
// graph-keeping forward (the backward pass needs the heads' inputs); pdrop: training dropout.
static int heads_fwd(cilrs_net* net, const cilrs_buffers* bufs, const float* feat,
                     const float* speed, const int64_t* command, bool graph, float pdrop,
                     uint64_t seed, float* controls, float* pred_speed, hipStream_t s) {
    const Arch& A = *net->A;
    float* ws = reinterpret_cast<float*>(bufs->workspace);
    const float* P = bufs->params;
    const int B = net->B;
    int* status = status_words(net, bufs);
    const int featw = A.feat, comb = A.feat + 128;
    if (!graph && B <= kHeadsSmallMaxB && A.variant == 0) {
        // ---- inference at control-loop batch sizes: 4 launches, commanded branch only ----
        RUN(net, "heads_fwd", 0.0, 0.0, s,
            launch_heads_small_pre(feat, net->featHW, speed, P + A.se0.w, P + A.se0.b, P + A.se3.w,
                                   P + A.se3.b, ws + net->combined, B, s));
        HeadsSmallArgs h;
        memset(&h, 0, sizeof(h));
        h.B = B;
        h.ncmd = A.ncmd;
        h.cmd = reinterpret_cast<const long long*>(command);
        for (int layer = 0; layer < 3; ++layer) {
            for (int k = 0; k < A.ncmd; ++k) {
                h.w[k] = P + A.br[k][layer].w;
                h.b[k] = P + A.br[k][layer].b;
            }
            const LinT& sp = layer == 0 ? A.sp0 : layer == 1 ? A.sp3 : A.sp5;
            h.w[A.ncmd] = P + sp.w;
            h.b[A.ncmd] = P + sp.b;
            h.in[0] = A.br[0][layer].in;
            h.in[1] = sp.in;
            h.x_ld = h.in[0];
            h.x[0] = layer == 0 ? ws + net->combined : layer == 1 ? ws + net->h1[0] : ws + net->h2[0];
            h.x[1] = layer == 0 ? ws + net->combined : layer == 1 ? ws + net->p1 : ws + net->p2;
            h.y[0] = layer == 0 ? ws + net->h1[0] : layer == 1 ? ws + net->h2[0] : controls;
            h.y[1] = layer == 0 ? ws + net->p1 : layer == 1 ? ws + net->p2 : pred_speed;
            h.out[0] = A.br[0][layer].out;
            h.out[1] = sp.out;
            h.y_ld[0] = h.out[0];
            h.y_ld[1] = h.out[1];
            h.relu = layer < 2;
            h.status = layer == 2 ? status : nullptr;
            RUN(net, "heads_fwd", 2.0 * B * (h.in[0] * h.out[0] + h.in[1] * h.out[1]),
                4.0 * (h.in[0] * h.out[0] + h.in[1] * h.out[1]), s,
                launch_heads_small_layer(h, s));
        }
        return 0;
    }

    // ---- avgpool + flatten -> combined[:, 0:512] ----
    if (feat != nullptr)
        RUN(net, "heads_fwd", 0.0, 0.0, s,
            launch_avgpool_fwd(feat, ws + net->combined, B, net->featHW, featw, comb, s));

    if (graph) {   // backward needs the inputs of the heads
        if (launch_keep_head_inputs(speed, reinterpret_cast<const long long*>(command), ws + net->speed_in,
                                    reinterpret_cast<long long*>(reinterpret_cast<char*>(bufs->workspace) +
                                                                 net->cmd_b), B, s)) return 1;
    }
    // Every layer of every chain that can run at the same time is ONE grouped launch
    // (heads_gemm.hip): 7 launches for the whole head instead of ~25 on five side streams.
    auto fwd_group = [&](HGemmGroup& g, const float* x, int x_ld, const LinT& l, float* y, int y_ld,
                         unsigned long long drop_stream) {
        memset(&g, 0, sizeof(g));
        g.A = x; g.lda = x_ld; g.B = P + l.w; g.ldb = l.in; g.bias = P + l.b;
        g.C = y; g.ldc = y_ld; g.M = B; g.N = l.out; g.K = l.in; g.drop_stream = drop_stream;
    };
    auto run_fwd = [&](HGemmArgs& h, int n, int relu) -> int {
        h.ngroups = n; h.relu = relu; h.accumulate = 0; h.drop_p = pdrop; h.seed = seed;
        double fl = 0.0;
        for (int i = 0; i < n; ++i) fl += 2.0 * h.g[i].M * h.g[i].N * h.g[i].K;
        RUN(net, "heads_fwd", fl, 0.0, s, launch_hgemm(0, h, s));
        return 0;
    };
    HGemmArgs h;
    // ---- speed encoder (autonomous_drive.py:371-374, 391) ----
    memset(&h, 0, sizeof(h));
    fwd_group(h.g[0], speed, 1, A.se0, ws + net->s1, 128, 0);
    if (run_fwd(h, 1, 1)) return 1;
    fwd_group(h.g[0], ws + net->s1, 128, A.se3, ws + net->combined + featw, comb, kNoDrop);
    if (run_fwd(h, 1, 1)) return 1;
    // ---- the branches (all evaluated, :394-396) + speed predictor (:383-387, 393), layer by layer;
    //      dropout streams: 1 + 2k / 2 + 2k for branch k, 2 NC + 1 for the speed predictor (= 9 for
    //      the reference's four commands)
    const int NC = A.ncmd;
    for (int k = 0; k < NC; ++k)
        fwd_group(h.g[k], ws + net->combined, comb, A.br[k][0], ws + net->h1[k], 256, 1 + 2 * k);
    fwd_group(h.g[NC], ws + net->combined, comb, A.sp0, ws + net->p1, 256, 2 * NC + 1);
    if (run_fwd(h, NC + 1, 1)) return 1;
    for (int k = 0; k < NC; ++k)
        fwd_group(h.g[k], ws + net->h1[k], 256, A.br[k][1], ws + net->h2[k], 256, 2 + 2 * k);
    fwd_group(h.g[NC], ws + net->p1, 256, A.sp3, ws + net->p2, 256, kNoDrop);
    if (run_fwd(h, NC + 1, 1)) return 1;
    for (int k = 0; k < NC; ++k)
        fwd_group(h.g[k], ws + net->h2[k], 256, A.br[k][2], ws + net->all_out + (size_t)k * B * 4,
                  4, kNoDrop);
    fwd_group(h.g[NC], ws + net->p2, 256, A.sp5, pred_speed, 1, kNoDrop);
    if (run_fwd(h, NC + 1, 0)) return 1;
    // gathered by command (:397-398)
    RUN(net, "heads_fwd", 0.0, 0.0, s,
        launch_branch_gather(ws + net->all_out, reinterpret_cast<const long long*>(command),
                             controls, B, NC, status, s));
    return 0;
}

// Where a forward takes its image from: strided float NCHW (already normalised), uint8 HWC frames
// of the plan's size, or raw camera frames (resized on the way).  stage_input brings it into x4.
struct ImageSrc {
    enum Kind { FloatNCHW, U8HWC, Camera } kind;
    const void* data;
    long sn = 0, sc = 0, sh = 0, sw = 0;                  // FloatNCHW: strides in floats
    int src_h = 0, src_w = 0, pixel_stride = 0;           // Camera: frame size, bytes per pixel
    long row_stride = 0, frame_stride = 0;                // Camera: bytes
};
static ImageSrc camera_src(const uint8_t* frames, int h, int w, int px, long row, long frame) {
    return {ImageSrc::Camera, frames, 0, 0, 0, 0, h, w, px, row, frame};
}
static int stage_input(cilrs_net* net, const cilrs_buffers* bufs, const ImageSrc& src, hipStream_t s) {
    float* x4 = reinterpret_cast<float*>(bufs->workspace) + net->x4;
    const uint8_t* u8 = static_cast<const uint8_t*>(src.data);
    RUN(net, "transform", 0.0, 0.0, s,
        src.kind == ImageSrc::FloatNCHW
            ? launch_nchw3_to_nhwc4(static_cast<const float*>(src.data), x4, net->B, net->H, net->W,
                                    src.sn, src.sc, src.sh, src.sw, s)
        : src.kind == ImageSrc::U8HWC
            ? launch_u8hwc_to_nhwc4(u8, x4, (size_t)net->B * net->H * net->W, kImageMean, kImageStd, s)
            : launch_camera_to_nhwc4(u8, x4, net->B, src.src_h, src.src_w, src.pixel_stride,
                                     src.row_stride, src.frame_stride, net->H, net->W, kImageMean,
                                     kImageStd, s));
    return 0;
}

// What the public forward entries differ in.
struct FwdMode {
    int train = 0; float dropout_p = 0.f; uint64_t seed = 0;
    int half = 0; bool frozen = false;
    // cilrs_net_forward_ft: eval-mode / gradient-free leading trunk groups, the prefix key
    bool ft = false; int ft_e = 0, ft_g = 0; uint64_t ft_key = 0;
};
static const FwdMode kFrozenMode{0, 0.f, 0, 0, true};

// The forward of every entry but the persistent launch and the statistics pass.  Modes: train
// (batch-statistics BatchNorm, dropout), frozen (running statistics, activations kept for the
// backward pass), else eval in fp32 (half = 0), fp16 (1) or bf16 (2).
static int forward_run(cilrs_net* net, const cilrs_buffers* bufs, const ImageSrc& src,
                       const float* speed, const int64_t* command, float* controls,
                       float* pred_speed, hipStream_t s, const FwdMode& m) {
    const int train = m.train, half = m.half;
    const bool frozen = m.frozen;
    if (fwd_begin(net, bufs, s)) return 1;
    CILRS_CHECK(!(frozen && (train || half || net->bf16_train)),
                "frozen forward: fp32 plans only (a CILRS_PLAN_BF16_TRAIN plan rejects it)");
    if (stage_input(net, bufs, src, s)) return 1;
    if (train) {
        // the stem weights are padded every step; the cached eval state goes stale as the
        // weights / BN buffers are about to change
        RUN(net, "transform", 0.0, 0.0, s,
            launch_pad_cin3_to_4(bufs->params + net->A->convs[0].w, net->ws_base + net->w4, 64 * 49, s));
        drop_eval_state(net);
    } else {
        if (eval_prep(net, bufs, s)) return 1;
        if (half && fold_prep(net, bufs, half, s)) return 1;
    }
    // train: batch statistics; frozen: the running statistics -- both keep every activation the
    // backward pass reads (y, z, the max-pool argmax, the head inputs)
    const bool graph = train || frozen;
    const float* feat = nullptr;
    const int rc = graph  ? trunk_fwd_graph(net, bufs, train, frozen, s, &feat)
                   : half ? trunk_fwd_eval16(net, bufs, half, s, &feat)
                          : trunk_fwd_eval32(net, bufs, s, &feat);
    const float pdrop = train ? m.dropout_p : 0.f;
    if (rc || heads_fwd(net, bufs, feat, speed, command, graph, pdrop, m.seed, controls, pred_speed, s))
        return 1;
    using LF = cilrs_net::LastForward;
    fwd_commit(net, train ? LF::Train : frozen ? LF::Frozen : LF::Eval, half, pdrop);
    return 0;
}

// Weight-derived state of a frozen prefix of `groups` trunk groups: the padded stem weights, the
// BatchNorm scale / shift (one launch derives every layer's; only the prefix's are read) and the
// Winograd filter images of the prefix's layers.  Frozen weights do not change from step to step:
// rebuilt only when the caller's prefix key, the cut or the buffers change (key 0: every call).
static int ft_prep(cilrs_net* net, const cilrs_buffers* bufs, int groups, uint64_t prefix_key,
                   hipStream_t s) {
    if (prefix_key != 0 && net->ft_prep_key == prefix_key && net->ft_prep_groups == groups &&
        net->ft_prep_bufs[0] == (const void*)bufs->params &&
        net->ft_prep_bufs[1] == (const void*)bufs->bn_running &&
        net->ft_prep_bufs[2] == (const void*)bufs->workspace)
        return 0;
    const Arch& A = *net->A;
    float* ws = reinterpret_cast<float*>(bufs->workspace);
    RUN(net, "transform", 0.0, 0.0, s,
        launch_pad_cin3_to_4(bufs->params + A.convs[0].w, ws + net->w4, 64 * 49, s));
    RUN(net, "bn_fwd.eval", 0.0, 0.0, s,
        launch_bn_eval_stats_all(net->bn_table, bufs->params, bufs->bn_running, ws, 1e-5f, s));
    if (ft_wino_fold() && net->wino_table.n) {
        const WinoWeightTable t = wino_subtable(net, 1, groups);
        if (t.n)
            RUN(net, "transform", 0.0, 4.0 * 4.6 * (double)t.blk_begin[t.n] * 256, s,
                launch_wino_weights_all(t, bufs->params, ws + net->wino_base, s));
    }
    net->ft_prep_key = prefix_key;
    net->ft_prep_groups = groups;
    net->ft_prep_bufs[0] = bufs->params; net->ft_prep_bufs[1] = bufs->bn_running;
    net->ft_prep_bufs[2] = bufs->workspace;
    return 0;
}

// Train-mode forward behind a frozen prefix of k trunk groups: the prefix like trunk_fwd_eval32
// (z only; eligible 3x3 layers on the Winograd kernel's folded epilogue), the rest of the trunk and
// the heads on the train path, reading the prefix's last tensor.
static int forward_ft_run(cilrs_net* net, const cilrs_buffers* bufs, const ImageSrc& src,
                          const float* speed, const int64_t* command, float* controls,
                          float* pred_speed, hipStream_t s, const FwdMode& m) {
    const int k = m.ft_e;
    if (fwd_begin(net, bufs, s)) return 1;
    if (stage_input(net, bufs, src, s)) return 1;
    drop_eval_state(net);      // the trainable weights / BatchNorm buffers are about to change
    if (ft_prep(net, bufs, k, m.ft_key, s)) return 1;
    const float* mid = nullptr;
    net->ft_wino = 0;
    net->ft_route_wino = true;
    const int rc0 = trunk_fwd_eval32(net, bufs, s, &mid, k);
    net->ft_route_wino = false;
    if (rc0) return 1;
    const float* feat = mid;
    if (k < 5 && trunk_fwd_graph(net, bufs, 1, false, s, &feat, k, mid)) return 1;
    if (heads_fwd(net, bufs, feat, speed, command, true, m.dropout_p, m.seed, controls, pred_speed, s))
        return 1;
    fwd_commit(net, cilrs_net::LastForward::Train, 0, m.dropout_p);
    return 0;
}

static int check_bufs(const cilrs_net* net, const cilrs_buffers* bufs, bool need_grads) {
    CILRS_CHECK(net != nullptr && bufs != nullptr, "net / buffers missing");
    CILRS_CHECK(bufs->params && bufs->bn_running && bufs->bn_nbt && bufs->workspace,
                "cilrs_buffers has NULL members");
    CILRS_CHECK(!need_grads || bufs->grads, "gradient arena missing");
    CILRS_CHECK(((uintptr_t)bufs->params & 15) == 0 && ((uintptr_t)bufs->workspace & 255) == 0,
                "params must be 16-byte and workspace 256-byte aligned");
    return 0;
}

// `who`: the entry's name in its messages
static int forward_entry(cilrs_net* net, const cilrs_buffers* bufs, const char* who,
                         const ImageSrc& src, const float* speed, const int64_t* command,
                         float* controls, float* pred_speed, void* stream, const FwdMode& m) {
    if (check_bufs(net, bufs, false)) return 1;
    CILRS_CHECK(src.data && speed && command && controls && pred_speed, "%s: NULL tensor", who);
    if (m.ft) {
        CILRS_CHECK(0 <= m.ft_g && m.ft_g <= 5 && (m.ft_e == 0 || m.ft_e == m.ft_g),
                    "forward_ft: supported cuts are bn_frozen_groups == grad_frozen_groups in 0..5, or "
                    "bn_frozen_groups == 0 (got %d, %d)", m.ft_e, m.ft_g);
        CILRS_CHECK(!(net->bf16_train && m.ft_g > 0),
                    "forward_ft: a CILRS_PLAN_BF16_TRAIN plan cannot freeze");
    }
    if (m.frozen)
        CILRS_CHECK(!net->bf16_train, "forward_frozen: fp32 plans only (a CILRS_PLAN_BF16_TRAIN plan "
                    "rejects the frozen mode)");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (m.ft_e > 0 ? forward_ft_run(net, bufs, src, speed, command, controls, pred_speed, s, m)
                   : forward_run(net, bufs, src, speed, command, controls, pred_speed, s, m))
        return 1;
    if (m.ft) { net->ft_bn = m.ft_e; net->ft_grad = m.ft_g; }
    return 0;
}

int cilrs_net_forward(cilrs_net* net, const cilrs_buffers* bufs, const float* image, long sn,
                      long sc, long sh, long sw, const float* speed, const int64_t* command,
                      int train, float dropout_p, uint64_t seed, float* controls,
                      float* pred_speed, void* stream) {
    return forward_entry(net, bufs, "forward", {ImageSrc::FloatNCHW, image, sn, sc, sh, sw}, speed,
                         command, controls, pred_speed, stream, {train, dropout_p, seed});
}

// The train-mode trunk of cilrs_net_forward(train = 1) -- the same convolution, BatchNorm and
// max-pool launches in the same order -- with every layer's batch statistics added to `table`
// instead of moving the running buffers (see include/cilrs_hip.h).
int cilrs_net_forward_bn_stats(cilrs_net* net, const cilrs_buffers* bufs, const float* image,
                               long sn, long sc, long sh, long sw, double* table, void* stream) {
    if (check_bufs(net, bufs, false)) return 1;
    CILRS_CHECK(image != nullptr, "forward_bn_stats: NULL image");
    CILRS_CHECK(!net->bf16_train, "forward_bn_stats: fp32 plans only (a CILRS_PLAN_BF16_TRAIN plan "
                "takes its statistics from bf16 tensors)");
    CILRS_CHECK(table != nullptr && ((uintptr_t)table & 7) == 0,
                "forward_bn_stats: the table is NULL or not 8-byte aligned");
    for (size_t ci = 0; ci < net->A->convs.size(); ++ci)
        CILRS_CHECK(net->cg[ci].M >= 2, "forward_bn_stats: BatchNorm %s sees %d value per channel in "
                    "this plan; more than 1 is needed (torch: 'Expected more than 1 value per "
                    "channel when training')", net->A->bns[net->A->convs[ci].bn].prefix.c_str(),
                    net->cg[ci].M);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float* ws = reinterpret_cast<float*>(bufs->workspace);
    if (fwd_begin(net, bufs, s)) return 1;
    drop_eval_state(net);      // the per-layer scale / shift tables are about to hold batch statistics
    if (stage_input(net, bufs, {ImageSrc::FloatNCHW, image, sn, sc, sh, sw}, s)) return 1;
    RUN(net, "transform", 0.0, 0.0, s,
        launch_pad_cin3_to_4(bufs->params + net->A->convs[0].w, ws + net->w4, 64 * 49, s));
    const float* feat = nullptr;
    if (trunk_fwd_graph(net, bufs, 1, false, s, &feat, 0, nullptr, table)) return 1;
    // (no heads ran: nothing here is a graph cilrs_net_backward could walk)
    fwd_commit(net, cilrs_net::LastForward::StatsOnly);
    return 0;
}

int cilrs_bn_stats_finalize(int variant, const double* table, int estimator, float* bn_running,
                            int64_t* bn_nbt, void* stream) {
    CILRS_CHECK(variant_ok(variant), "bn_stats_finalize: variant %d out of range", variant);
    CILRS_CHECK(table && bn_running && bn_nbt, "bn_stats_finalize: NULL tensor");
    CILRS_CHECK(((uintptr_t)table & 7) == 0 && ((uintptr_t)bn_nbt & 7) == 0 &&
                    ((uintptr_t)bn_running & 3) == 0, "bn_stats_finalize: misaligned tensor");
    CILRS_CHECK(estimator == 0 || estimator == 1, "bn_stats_finalize: estimator %d (0 batch_mean, "
                "1 pooled)", estimator);
    const Arch& A = arch(variant);
    BnStatsTable t;
    bn_stats_layout(A, t);
    // a layer that saw no batch has no statistics: the {t, sum M} heads are read back first (this
    // call synchronises the stream; it runs once per re-estimation, not per batch)
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    std::vector<double> head((size_t)kBnStatsHead * t.n);
    CILRS_HIP(hipMemcpyAsync(head.data(), table, head.size() * sizeof(double),
                             hipMemcpyDeviceToHost, s));
    CILRS_HIP(hipStreamSynchronize(s));
    for (int j = 0; j < t.n; ++j) {
        const double tb = head[(size_t)kBnStatsHead * j], rows = head[(size_t)kBnStatsHead * j + 1];
        CILRS_CHECK(tb >= 1.0 && rows >= 2.0 * tb && tb == (double)(long long)tb,
                    "bn_stats_finalize: BatchNorm %s has seen %g batches / %g rows; at least one "
                    "batch is needed", A.bns[j].prefix.c_str(), tb, rows);
    }
    return launch_bn_stats_finalize(t, table, estimator, bn_running,
                                    reinterpret_cast<long long*>(bn_nbt), s);
}

int cilrs_bn_train_stats(const float* y, int M, int C, double* acc, float* partial, void* stream) {
    return launch_bn_train_stats(y, M, C, acc, partial, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_net_forward_frozen(cilrs_net* net, const cilrs_buffers* bufs, const float* image, long sn,
                             long sc, long sh, long sw, const float* speed, const int64_t* command,
                             float* controls, float* pred_speed, void* stream) {
    return forward_entry(net, bufs, "forward_frozen", {ImageSrc::FloatNCHW, image, sn, sc, sh, sw},
                         speed, command, controls, pred_speed, stream, kFrozenMode);
}

// Fine-tuning on top of a pretrained trunk -- the reference's own first remedy for its failure on
// the campus map, "collect a small CUSAT-specific dataset and fine-tune the checkpoint" (reference
// README.md, "Why Results Degraded on CUSAT Map"; configs/train_config.json carries `pretrained`):
// the train-mode forward with the first grad_frozen_groups trunk groups (stem, layer1 .. layer4)
// taking no gradient and the first bn_frozen_groups of them in eval mode.
int cilrs_net_forward_ft(cilrs_net* net, const cilrs_buffers* bufs, const float* image, long sn,
                         long sc, long sh, long sw, const float* speed, const int64_t* command,
                         int bn_frozen_groups, int grad_frozen_groups, uint64_t prefix_key,
                         float dropout_p, uint64_t seed, float* controls, float* pred_speed,
                         void* stream) {
    return forward_entry(net, bufs, "forward_ft", {ImageSrc::FloatNCHW, image, sn, sc, sh, sw}, speed,
                         command, controls, pred_speed, stream,
                         {1, dropout_p, seed, 0, false, true, bn_frozen_groups, grad_frozen_groups,
                          prefix_key});
}
int cilrs_net_ft_wino_convs(cilrs_net* net) { return net ? net->ft_wino : 0; }
int cilrs_net_ft_cut(const cilrs_net* net, int* bn_frozen_groups, int* grad_frozen_groups) {
    CILRS_CHECK(net != nullptr, "ft_cut: net is NULL");
    if (bn_frozen_groups) *bn_frozen_groups = net->ft_bn;
    if (grad_frozen_groups) *grad_frozen_groups = net->ft_grad;
    return 0;
}

// uint8 HWC frames -> eval forward in fp32 (half = 0), fp16 (1) or bf16 (2)
static int forward_u8(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frames,
                      const float* speed, const int64_t* command, float* controls,
                      float* pred_speed, void* stream, int half) {
    const char* who = half == 2 ? "forward_u8_bf16" : half ? "forward_u8_f16" : "forward_u8";
    return forward_entry(net, bufs, who, {ImageSrc::U8HWC, frames}, speed, command, controls, pred_speed,
                         stream, {0, 0.f, 0, half});
}

int cilrs_net_forward_u8(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frames,
                         const float* speed, const int64_t* command, float* controls,
                         float* pred_speed, void* stream) {
    return forward_u8(net, bufs, frames, speed, command, controls, pred_speed, stream, 0);
}

int cilrs_net_forward_frozen_u8(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frames,
                                const float* speed, const int64_t* command, float* controls,
                                float* pred_speed, void* stream) {
    return forward_entry(net, bufs, "forward_frozen_u8", {ImageSrc::U8HWC, frames}, speed, command,
                         controls, pred_speed, stream, kFrozenMode);
}

int cilrs_net_forward_camera(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frames,
                             int src_h, int src_w, int pixel_stride, long row_stride,
                             long frame_stride, const float* speed, const int64_t* command,
                             float* controls, float* pred_speed, void* stream) {
    return forward_entry(net, bufs, "forward_camera",
                         camera_src(frames, src_h, src_w, pixel_stride, row_stride, frame_stride),
                         speed, command, controls, pred_speed, stream, FwdMode());
}

int cilrs_net_forward_frozen_camera(cilrs_net* net, const cilrs_buffers* bufs,
                                    const uint8_t* frames, int src_h, int src_w, int pixel_stride,
                                    long row_stride, long frame_stride, const float* speed,
                                    const int64_t* command, float* controls, float* pred_speed,
                                    void* stream) {
    return forward_entry(net, bufs, "forward_frozen_camera",
                         camera_src(frames, src_h, src_w, pixel_stride, row_stride, frame_stride),
                         speed, command, controls, pred_speed, stream, kFrozenMode);
}

int cilrs_net_forward_u8_f16(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frames,
                             const float* speed, const int64_t* command, float* controls,
                             float* pred_speed, void* stream) {
    return forward_u8(net, bufs, frames, speed, command, controls, pred_speed, stream, 1);
}

int cilrs_net_forward_u8_bf16(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frames,
                              const float* speed, const int64_t* command, float* controls,
                              float* pred_speed, void* stream) {
    return forward_u8(net, bufs, frames, speed, command, controls, pred_speed, stream, 2);
}

// ------------------------------------------------------------------------------------------------
// single-frame inference as ONE persistent launch (infer_b1.hip)
// ------------------------------------------------------------------------------------------------

// Stage table of the persistent kernel for this plan on a grid of `nblk` workgroups.
static int b1_build(cilrs_net* net, int nblk) {
    const Arch& A = *net->A;
    std::vector<B1Stage>& T = net->b1_host;
    T.clear();
    auto fb = [](size_t floats) { return (unsigned)(floats * sizeof(float)); };
    bool magic_ok = true;
    auto magic20 = [&](int d, int xmax) {        // x / d == (x * magic) >> 20 for 0 <= x <= xmax
        const unsigned mg = ((1u << 20) + (unsigned)d - 1u) / (unsigned)d;
        for (int x = 0; x <= xmax; ++x)
            if ((unsigned)(((unsigned long long)x * mg) >> 20) != (unsigned)(x / d) ||
                (unsigned long long)x * mg >= (1ull << 32))
                magic_ok = false;
        return mg;
    };
    auto conv_desc = [&](int ci, size_t x, bool has_add, size_t add, int relu, int relu_post) {
        const ConvT& c = A.convs[ci];
        const ConvG& g = net->cg[ci];
        B1Conv d;
        memset(&d, 0, sizeof(d));
        d.x_off = fb(x); d.y_off = fb(g.z); d.add_off = has_add ? fb(add) : 0u;
        d.scale_off = fb(g.stats + 2 * (size_t)c.cout); d.shift_off = fb(g.stats + 3 * (size_t)c.cout);
        d.H = g.H; d.W = g.W; d.Wo = g.Wo; d.Cout = c.cout; d.K = c.k;
        d.stride = c.stride; d.M = g.M; d.nmt = cdiv(g.M, 16);
        d.ntiles = d.nmt * (c.cout / 16);
        d.relu = relu; d.relu_post = relu_post; d.has_add = has_add ? 1 : 0;
        if (ci == 0) {      // stem: channel-padded image, padded weights in the workspace
            d.Cin = 4; d.w_off = fb(net->w4); d.S = cdiv(c.k * c.k, 4); d.cshift = 0;
        } else {
            d.Cin = c.cin; d.w_off = fb(c.w);
            const int cgn = c.cin / 16;
            d.S = c.k * c.k * cgn;
            while ((1 << d.cshift) < cgn) ++d.cshift;
        }
        d.krow4 = c.k * c.k * d.Cin * 4;
        d.wo_magic = magic20(g.Wo, d.nmt * 16 + 16);
        d.nmt_magic = magic20(d.nmt, d.ntiles);
        return d;
    };
    auto check_conv = [&](int ci) -> bool {
        const ConvT& c = A.convs[ci];
        const int cgn = c.cin / 16;
        return c.cin % 16 == 0 && c.cout % 16 == 0 && (cgn & (cgn - 1)) == 0 &&
               ((c.k == 3 && c.pad == 1) || (c.k == 1 && c.pad == 0));
    };
    // Shape of one stage: waves per unit (wpt), workgroups per tile (split of the reduction index,
    // ks) and channel tiles per unit (nt) of its one or two convolutions.  All units in ONE pass of
    // slots; a wave holds at most kB1MaxK weight fragments.  Cost = k-groups the busiest CU streams
    // after the barrier (activation fragments; the weight fragments are in flight before it and
    // count half; 2 KB each at ~70 GB/s per CU: 35 per microsecond) + ~50 for a ticketed combine.
    constexpr int kB1MaxK = 8;
    bool plan_ok = true;
    auto push_conv_stage = [&](int type, int n0, const B1Conv& c0, int n1, const B1Conv* c1) {
        B1Stage st;
        memset(&st, 0, sizeof(st));
        st.type = type;
        struct Opt { int ks, nt; };
        const Opt opts[5] = {{1, 1}, {2, 1}, {3, 1}, {4, 1}, {1, 2}};
        int best_cost = 1 << 30, bw = 0, b0 = 0, b1 = 0;
        auto units_of = [&](const B1Conv& c, const Opt& o) { return c.ntiles / o.nt * o.ks; };
        auto feasible = [&](const B1Conv& c, const Opt& o, int w) {
            if (o.nt == 2 && (c.Cout % 32 != 0 || type == B1_STEM)) return false;
            if (o.ks > 1 && (type == B1_STEM || o.ks > c.S)) return false;
            return cdiv(cdiv(c.S, o.ks), w) * o.nt <= kB1MaxK;
        };
        for (int w : {16, 8, 4, 2})
            for (int i0 = 0; i0 < 5; ++i0)
                for (int i1 = 0; i1 < (c1 ? 5 : 1); ++i1) {
                    if (!feasible(c0, opts[i0], w) || (c1 && !feasible(*c1, opts[i1], w))) continue;
                    const int units = units_of(c0, opts[i0]) + (c1 ? units_of(*c1, opts[i1]) : 0);
                    if (units > nblk * (16 / w)) continue;
                    auto load = [&](const B1Conv& c, const Opt& o) {
                        const int sp = cdiv(c.S, o.ks);
                        return 2 * sp + sp * o.nt;          // activations + half the weights, x2
                    };
                    int l = load(c0, opts[i0]);
                    if (c1 && load(*c1, opts[i1]) > l) l = load(*c1, opts[i1]);
                    const int cost = cdiv(units, nblk) * l / 2 +
                                     ((opts[i0].ks > 1 || (c1 && opts[i1].ks > 1)) ? 50 : 0);
                    if (cost < best_cost) { best_cost = cost; bw = w; b0 = i0; b1 = i1; }
                }
        if (bw == 0) { plan_ok = false; bw = 2; }
        auto fin = [&](B1Conv d, const Opt& o, int ticket0, size_t slab) {
            d.ksplit = o.ks; d.nt = o.nt;
            d.sper = cdiv(d.S, o.ks); d.per = cdiv(d.sper, bw);
            d.nunits = d.ntiles / o.nt * o.ks;
            d.ks_magic = magic20(o.ks, d.nunits);
            d.nmt_magic = magic20(d.nmt, d.ntiles);
            d.ticket0 = ticket0;
            d.slab_off = fb(slab);
            if (o.ks > 1 && ticket0 + d.ntiles > kB1Tickets) plan_ok = false;
            if (o.ks > 1 && (size_t)o.ks * d.nmt * 16 * d.Cout > net->b1_slab_floats / 2) plan_ok = false;
            return d;
        };
        st.c[0] = fin(c0, opts[b0], 0, net->b1_slabs);
        if (c1) st.c[1] = fin(*c1, opts[b1], c0.ntiles, net->b1_slabs + net->b1_slab_floats / 2);
        st.wpt = bw;
        st.conv_no[0] = n0;
        st.conv_no[1] = c1 ? n1 : -1;
        st.nunits0 = st.c[0].nunits;
        st.total_units = st.c[0].nunits + (c1 ? st.c[1].nunits : 0);
        // same lane-level plan as the previous stage?  (everything but the tensor bases, the
        // epilogue flags and the BatchNorm tables equal)
        if (!T.empty() && T.back().type == B1_CONV && type == B1_CONV && !c1 &&
            T.back().total_units == T.back().nunits0 && T.back().wpt == st.wpt) {
            B1Conv p0 = T.back().c[0], n0 = st.c[0];
            p0.x_off = p0.y_off = p0.add_off = p0.w_off = p0.scale_off = p0.shift_off = 0;
            n0.x_off = n0.y_off = n0.add_off = n0.w_off = n0.scale_off = n0.shift_off = 0;
            p0.relu = p0.relu_post = p0.has_add = n0.relu = n0.relu_post = n0.has_add = 0;
            st.same_shape = memcmp(&p0, &n0, sizeof(B1Conv)) == 0;
        }
        if (experiment_env("CILRS_B1_FINE", 0))
            fprintf(stderr, "b1 stage %2d: wpt %2d units %4d (ks %d nt %d per %d | ks %d nt %d per %d) same %d\n",
                    (int)T.size(), st.wpt, st.total_units, st.c[0].ksplit, st.c[0].nt, st.c[0].per,
                    c1 ? st.c[1].ksplit : 0, c1 ? st.c[1].nt : 0, c1 ? st.c[1].per : 0, st.same_shape);
        T.push_back(st);
    };
    {   // uint8 frame -> normalised NHWC4
        B1Stage st;
        memset(&st, 0, sizeof(st));
        st.type = B1_PRE; st.pH = net->H; st.pW = net->W; st.dst_off = fb(net->x4);
        // (a workgroup parks its run of the frame's bytes in 32 KB of LDS: infer_b1.hip pre_stage)
        CILRS_CHECK(3 * cdiv(net->H * net->W, nblk) + 8 <= 16 * 512 * 4,
                    "persistent kernel: frame too large for %d workgroups", nblk);
        // ... and the speed encoder, evaluated by one block beside the pixel work
        st.h.se_w0 = fb(A.se0.w); st.h.se_b0 = fb(A.se0.b);
        st.h.se_w1 = fb(A.se3.w); st.h.se_b1 = fb(A.se3.b);
        st.h.y_off[0] = fb(net->s1);
        st.cmd_off = fb(net->b1_cmd);
        T.push_back(st);
    }
    push_conv_stage(B1_STEM, 0, conv_desc(0, net->x4, false, 0, 1, 0), -1, nullptr);
    {   // max-pool 3x3/s2/p1
        B1Stage st;
        memset(&st, 0, sizeof(st));
        st.type = B1_POOL; st.src_off = fb(net->cg[0].z); st.dst_off = fb(net->pool);
        st.pH = net->H0; st.pW = net->W0; st.pC = 64; st.pHo = net->H1; st.pWo = net->W1;
        T.push_back(st);
    }
    size_t cur = net->pool;
    for (const BlockT& blk : A.blocks) {
        CILRS_CHECK(blk.conv3 < 0, "infer_b1: BasicBlock networks only");
        CILRS_CHECK(check_conv(blk.conv1) && check_conv(blk.conv2) &&
                        (blk.down < 0 || check_conv(blk.down)),
                    "infer_b1: unsupported convolution shape");
        const B1Conv c1 = conv_desc(blk.conv1, cur, false, 0, 1, 0);
        size_t identity = cur;
        if (blk.down >= 0) {
            const B1Conv cd = conv_desc(blk.down, cur, false, 0, 0, 0);
            push_conv_stage(B1_CONV, blk.conv1, c1, blk.down, &cd);
            identity = net->cg[blk.down].z;
        } else {
            push_conv_stage(B1_CONV, blk.conv1, c1, -1, nullptr);
        }
        push_conv_stage(B1_CONV, blk.conv2,
                        conv_desc(blk.conv2, net->cg[blk.conv1].z, true, identity, 0, 1), -1, nullptr);
        cur = net->cg[blk.conv2].z;
    }
    // heads: commanded branch (chain 0) and speed predictor (chain 1), layer by layer
    for (int layer = 0; layer < 3; ++layer) {
        B1Stage st;
        memset(&st, 0, sizeof(st));
        st.type = B1_HEAD;
        st.cmd_off = fb(net->b1_cmd);
        B1Head& h = st.h;
        for (int k = 0; k < 4; ++k) {
            h.w_off[k] = fb(A.br[k][layer].w);
            h.b_off[k] = fb(A.br[k][layer].b);
        }
        const LinT& sp = layer == 0 ? A.sp0 : layer == 1 ? A.sp3 : A.sp5;
        h.w_off[4] = fb(sp.w); h.b_off[4] = fb(sp.b);
        h.in[0] = A.br[0][layer].in; h.in[1] = sp.in;
        h.out[0] = A.br[0][layer].out; h.out[1] = sp.out;
        h.relu = layer < 2; h.first = layer == 0; h.last = layer == 2;
        h.x_off[0] = fb(layer == 0 ? net->s1 : layer == 1 ? net->h1[0] : net->h2[0]);
        h.x_off[1] = fb(layer == 1 ? net->p1 : net->p2);
        h.y_off[0] = fb(layer == 0 ? net->h1[0] : net->h2[0]);
        h.y_off[1] = fb(layer == 0 ? net->p1 : net->p2);
        if (layer == 0) {
            h.feat_off = fb(cur); h.featHW = net->featHW; h.featC = A.feat;
            CILRS_CHECK(A.feat == 512 && h.in[0] == 640 && h.in[1] == 512,
                        "infer_b1: head geometry");
        }
        CILRS_CHECK(h.in[0] % 4 == 0 && h.in[1] % 4 == 0 && h.in[0] <= 768 && h.in[1] <= 768,
                    "infer_b1: head width");
        T.push_back(st);
    }
    // (the tiling first: a stage without one keeps a placeholder whose unit counts may also be
    // beyond the division constants, and the missing tiling is what the caller needs to hear)
    CILRS_CHECK(plan_ok, "infer_b1: no one-pass tiling of a stage on %d workgroups", nblk);
    CILRS_CHECK(magic_ok, "infer_b1: division constants do not cover this geometry");
    CILRS_CHECK(A.convs[0].k == 7 && A.convs[0].pad == 3 && A.convs[0].stride == 2,
                "infer_b1: stem geometry");
    CILRS_CHECK((int)T.size() <= kB1MaxStages, "infer_b1: %d stages", (int)T.size());
    return 0;
}

// `frame`: a uint8 HWC frame that the kernel's first stage normalises; or `camera`: a raw camera
// frame, staged into x4 by a launch of its own, and the kernel starts at its second stage
static int b1_launch(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frame,
                     const ImageSrc* camera, const float* speed, const int64_t* command,
                     float* controls, float* pred_speed, void* stream, int* done = nullptr,
                     int seq = 0) {
    if (check_bufs(net, bufs, false)) return 1;
    CILRS_CHECK((frame || camera) && speed && command && controls && pred_speed,
                "forward_u8_b1: NULL tensor");
    CILRS_CHECK(net->B == 1 && net->A->variant == 0 && net->b1_table != 0,
                "forward_u8_b1: the persistent kernel serves the reference network at batch 1");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float* ws = reinterpret_cast<float*>(bufs->workspace);
    if (fwd_begin(net, bufs, s)) return 1;
    if (camera && stage_input(net, bufs, *camera, s)) return 1;
    if (net->b1_blocks < 0) {
        int blocks = 0;
        if (infer_b1_grid(&blocks)) return 1;
        CILRS_CHECK(blocks >= 8, "forward_u8_b1: the device cannot keep the persistent grid resident");
        if (b1_build(net, blocks)) return 1;
        net->b1_blocks = blocks;
    }
    if (eval_prep(net, bufs, s)) return 1;
    if (net->b1_ready_for != bufs->workspace) {
        CILRS_HIP(hipMemsetAsync(ws + net->b1_sync, 0, kB1SyncInts * sizeof(int), s));
            CILRS_HIP(hipMemcpyAsync(ws + net->b1_table, net->b1_host.data(),
                                 net->b1_host.size() * sizeof(B1Stage), hipMemcpyHostToDevice, s));
        net->b1_ready_for = bufs->workspace;
    }
    B1Launch a;
    memset(&a, 0, sizeof(a));
    a.table = reinterpret_cast<const B1Stage*>(ws + net->b1_table);
    a.nstages = (int)net->b1_host.size();
    a.first_stage = camera ? 1 : 0;
    a.ws = ws; a.ws_bytes = net->ws_bytes;
    a.params = bufs->params; a.param_bytes = net->A->arena_floats * sizeof(float);
    a.done = done; a.seq = seq;
    a.frame = frame; a.speed = speed; a.cmd = reinterpret_cast<const long long*>(command);
    a.controls = controls; a.pred_speed = pred_speed;
    a.sync = reinterpret_cast<int*>(ws + net->b1_sync);
    a.status = status_words(net, bufs);
    // CILRS_B1_STAMPS=1: block 0 records its clock at every stage (cilrs_net_b1_stage_us)
    static const int stamps_on = env_int("CILRS_B1_STAMPS", 0);
    a.stamps = stamps_on ? reinterpret_cast<long long*>(ws + net->b1_stamps) : nullptr;
    for (int i = 0; i < 3; ++i) { a.mean[i] = kImageMean[i]; a.stdv[i] = kImageStd[i]; }
    RUN(net, "infer_b1", 2.0 * 2.798e9 / 2.0, 0.0, s, launch_infer_b1(a, net->b1_blocks, s));
    fwd_commit(net, cilrs_net::LastForward::EvalB1);
    return 0;
}

int cilrs_net_forward_u8_b1(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frame,
                            const float* speed, const int64_t* command, float* controls,
                            float* pred_speed, void* stream) {
    return b1_launch(net, bufs, frame, nullptr, speed, command, controls, pred_speed, stream);
}

int cilrs_net_forward_camera_b1(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frame,
                                int src_h, int src_w, int pixel_stride, long row_stride,
                                const float* speed, const int64_t* command, float* controls,
                                float* pred_speed, int sync, void* stream) {
    if (check_bufs(net, bufs, false)) return 1;
    CILRS_CHECK(frame != nullptr, "forward_camera_b1: NULL frame");
    const ImageSrc cam = camera_src(frame, src_h, src_w, pixel_stride, row_stride, (long)src_h * row_stride);
    if (b1_launch(net, bufs, nullptr, &cam, speed, command, controls, pred_speed, stream)) return 1;
    if (sync) CILRS_HIP(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    return 0;
}

int cilrs_net_forward_u8_b1_post(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frame,
                                 const float* speed, const int64_t* command, float* controls,
                                 float* pred_speed, int* done, int seq, void* stream) {
    CILRS_CHECK(done != nullptr, "forward_u8_b1_post: NULL completion word");
    return b1_launch(net, bufs, frame, nullptr, speed, command, controls, pred_speed, stream, done,
                     seq);
}

int cilrs_net_forward_u8_b1_sync(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frame,
                                 const float* speed, const int64_t* command, float* controls,
                                 float* pred_speed, void* stream) {
    if (cilrs_net_forward_u8_b1(net, bufs, frame, speed, command, controls, pred_speed, stream))
        return 1;
    CILRS_HIP(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    return 0;
}

int cilrs_net_b1_stage_us(cilrs_net* net, const cilrs_buffers* bufs, float* start_us,
                          float* work_us, int cap) {
    CILRS_CHECK(net && bufs && bufs->workspace && start_us && work_us, "b1_stage_us: NULL");
    CILRS_CHECK(net->b1_table != 0 && net->b1_blocks > 0, "b1_stage_us: no persistent launch yet");
    const int n = (int)net->b1_host.size();
    CILRS_CHECK(cap >= n, "b1_stage_us: need room for %d stages", n);
    std::vector<long long> h(10 * (kB1MaxStages + 1));
    CILRS_HIP(hipMemcpy(h.data(), reinterpret_cast<float*>(bufs->workspace) + net->b1_stamps,
                        h.size() * sizeof(long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {          // 100 MHz clock
        start_us[i] = (float)((h[i] - h[0]) * 0.01);
        work_us[i] = (float)((h[kB1MaxStages + 1 + i] - h[i]) * 0.01);
    }
    if (experiment_env("CILRS_B1_FINE", 0)) {         // when each workgroup finished each stage (us after its start)
        const int nb = net->b1_blocks;
        std::vector<long long> d((size_t)n * nb);
        CILRS_HIP(hipMemcpy(d.data(), reinterpret_cast<long long*>(reinterpret_cast<float*>(bufs->workspace) +
                                                                  net->b1_stamps) + 10 * (kB1MaxStages + 1),
                            d.size() * sizeof(long long), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) {
            std::vector<double> t(nb);
            for (int b = 0; b < nb; ++b) t[b] = (d[(size_t)i * nb + b] - h[i]) * 0.01;
            std::vector<double> srt = t;
            std::sort(srt.begin(), srt.end());
            int worst = 0;
            for (int b = 0; b < nb; ++b) if (t[b] > t[worst]) worst = b;
            fprintf(stderr, "stage %2d done: min %5.2f p50 %5.2f p90 %5.2f max %5.2f (block %d; block 0 %5.2f)\n",
                    i, srt[0], srt[nb / 2], srt[nb * 9 / 10], srt[nb - 1], worst, t[0]);
            if (experiment_env("CILRS_B1_DUMP", 0) && (i == 4 || i == 12 || i == 20 || i == 32)) {
                fprintf(stderr, "stage %2d per block:", i);
                for (int b = 0; b < nb; ++b) fprintf(stderr, " %.2f", t[b]);
                fprintf(stderr, "\n");
            }
        }
    }
    if (experiment_env("CILRS_B1_FINE", 0))           // conv stages: block 0 / wave 0 inside the stage
        for (int i = 0; i < n; ++i) {
            const long long* f = &h[2 * (kB1MaxStages + 1) + 8 * i];
            fprintf(stderr, "stage %2d fine:", i);
            for (int k = 0; k < 8; ++k) fprintf(stderr, " %6.2f", (f[k] - h[i]) * 0.01);
            fprintf(stderr, "\n");
        }
    return 0;
}

int cilrs_net_b1_set_epoch(cilrs_net* net, const cilrs_buffers* bufs, int value, void* stream) {
    CILRS_CHECK(net && bufs && bufs->workspace, "b1_set_epoch: NULL");
    CILRS_CHECK(net->b1_table != 0 && net->b1_ready_for == bufs->workspace,
                "b1_set_epoch: no persistent launch on this workspace yet");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    CILRS_HIP(hipStreamSynchronize(s));
    // the eight arrival shards and the epoch base are equal between launches: re-base all nine
    std::vector<int> h(9 * 32, 0);
    for (int i = 0; i < 9; ++i) h[i * 32] = value;
    CILRS_HIP(hipMemcpy(reinterpret_cast<float*>(bufs->workspace) + net->b1_sync, h.data(),
                        h.size() * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

int cilrs_net_wino_convs(cilrs_net* net) { return net ? net->wino_table.n : 0; }

int cilrs_net_b1_stages(cilrs_net* net) {
    if (!net || net->b1_table == 0) return 0;
    if (net->b1_blocks < 0) return -1;             // not launched yet
    return (int)net->b1_host.size();
}

int cilrs_net_b1_stage_info(const cilrs_net* net, int stage, int* type, int* wpt, int* same_shape,
                            int* workgroups, int* nconv, int* conv, int* ksplit, int* nt) {
    CILRS_CHECK(net != nullptr, "b1_stage_info: net is NULL");
    CILRS_CHECK(net->b1_table != 0 && net->b1_blocks > 0, "b1_stage_info: no persistent launch yet");
    CILRS_CHECK(stage >= 0 && stage < (int)net->b1_host.size(), "b1_stage_info: stage %d out of range",
                stage);
    const B1Stage& st = net->b1_host[stage];
    const bool is_conv = st.type == B1_CONV || st.type == B1_STEM;
    const int n = !is_conv ? 0 : st.total_units != st.nunits0 ? 2 : 1;
    if (type) *type = st.type;
    if (wpt) *wpt = is_conv ? st.wpt : 0;
    if (same_shape) *same_shape = st.same_shape;
    if (workgroups) *workgroups = net->b1_blocks;
    if (nconv) *nconv = n;
    for (int i = 0; i < 2; ++i) {
        if (conv) conv[i] = i < n ? st.conv_no[i] : -1;
        if (ksplit) ksplit[i] = i < n ? st.c[i].ksplit : 0;
        if (nt) nt[i] = i < n ? st.c[i].nt : 0;
    }
    return 0;
}

// Same as cilrs_net_forward_u8, replayed from a cached hipGraph (one launch per frame instead of
// ~80): the B=1 control-loop path (autonomous_drive.py:908-920) is launch-latency bound.  The
// graph is re-captured when any pointer changes.  `stream` must not be the legacy NULL stream.
static int forward_u8_graph(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frames,
                            const float* speed, const int64_t* command, float* controls,
                            float* pred_speed, void* stream, int half) {
    if (check_bufs(net, bufs, false)) return 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    CILRS_CHECK(s != nullptr, "forward_u8_graph: capture needs a non-default stream");
    // (on the capture path forward_u8 runs underneath and keeps a record of its own; the replayed
    //  graph overwrites every z and the head activations like the eval forward it was captured from)
    if (fwd_begin(net, bufs, s)) return 1;
    const void* key[8] = {bufs->params, bufs->bn_running, bufs->workspace, frames, speed, command,
                          controls, pred_speed};
    bool same = net->graph_exec.h != nullptr && net->graph_half == half &&
                net->graph_wkey == net->weights_key;
    for (int i = 0; i < 8 && same; ++i) same = key[i] == net->graph_key[i];
    if (!same) {
        // first call eager: function attributes, side streams, events; and whenever the
        // weight-derived eval state is stale (the weights key moved, or another mode ran in
        // between), so that it is rebuilt OUTSIDE the capture and the graph holds only the
        // per-frame kernels
        if (!net->warmed || !eval_state_current(net, bufs, half)) {
            if (ensure_streams(net)) return 1;
            if (forward_u8(net, bufs, frames, speed, command, controls, pred_speed, stream, half))
                return 1;
            CILRS_HIP(hipStreamSynchronize(s));
            net->warmed = true;
        }
        const bool prof = net->prof.on;
        net->prof.on = false;
        hipGraph_t graph = nullptr;
        CILRS_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int rc = forward_u8(net, bufs, frames, speed, command, controls, pred_speed, stream, half);
        const hipError_t e = hipStreamEndCapture(s, &graph);
        net->prof.on = prof;
        CILRS_CHECK(rc == 0, "forward_u8_graph: capture failed: %s", last_error());
        CILRS_CHECK(e == hipSuccess && graph != nullptr, "hipStreamEndCapture failed: %s",
                    hipGetErrorString(e));
        if (net->graph_exec) { (void)hipGraphExecDestroy(net->graph_exec); net->graph_exec.h = nullptr; }
        const hipError_t e2 = hipGraphInstantiate(&net->graph_exec.h, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        CILRS_CHECK(e2 == hipSuccess, "hipGraphInstantiate failed: %s", hipGetErrorString(e2));
        for (int i = 0; i < 8; ++i) net->graph_key[i] = key[i];
        net->graph_half = half;
        net->graph_wkey = net->weights_key;
    }
    CILRS_HIP(hipGraphLaunch(net->graph_exec, s));
    fwd_commit(net, cilrs_net::LastForward::Eval, half);
    return 0;
}

int cilrs_net_forward_u8_graph(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frames,
                               const float* speed, const int64_t* command, float* controls,
                               float* pred_speed, void* stream) {
    return forward_u8_graph(net, bufs, frames, speed, command, controls, pred_speed, stream, 0);
}

int cilrs_net_forward_u8_f16_graph(cilrs_net* net, const cilrs_buffers* bufs,
                                   const uint8_t* frames, const float* speed,
                                   const int64_t* command, float* controls, float* pred_speed,
                                   void* stream) {
    return forward_u8_graph(net, bufs, frames, speed, command, controls, pred_speed, stream, 1);
}

int cilrs_net_forward_u8_bf16_graph(cilrs_net* net, const cilrs_buffers* bufs,
                                    const uint8_t* frames, const float* speed,
                                    const int64_t* command, float* controls, float* pred_speed,
                                    void* stream) {
    return forward_u8_graph(net, bufs, frames, speed, command, controls, pred_speed, stream, 2);
}

// The features the plan's last eval-mode forward left for the tick-following entries (heads_mc,
// gradcam, feature_moments, novelty): pooled in `combined`, or the last feature map alone.
static FeatureSrc plan_features(const cilrs_net* net, const cilrs_buffers* bufs) {
    const Arch& A = *net->A;
    const float* ws = reinterpret_cast<const float*>(bufs->workspace);
    if (net->last.featmap_only()) {
        const BlockT& blk = A.blocks.back();
        return {nullptr, 0, ws + net->cg[blk.conv3 >= 0 ? blk.conv3 : blk.conv2].z, net->featHW};
    }
    return {ws + net->combined, A.feat + 128, nullptr, 0};
}
static int plan_features_checked(const char* who, const cilrs_net* net, const cilrs_buffers* bufs,
                                 FeatureSrc* src) {
    CILRS_CHECK(!net->last.no_features(), "%s: no forward on this plan yet", who);
    CILRS_CHECK(!net->last.train_features(), "%s: the plan's last forward ran in train mode (batch "
                "statistics); run an eval-mode forward first", who);
    *src = plan_features(net, bufs);
    return 0;
}

// the heads' weights inside the parameter vector P (mc_heads.hip, gradcam.hip)
static HeadWeights head_weights(const Arch& A, const float* P) {
    HeadWeights h{};
    h.se0_w = P + A.se0.w; h.se0_b = P + A.se0.b; h.se3_w = P + A.se3.w; h.se3_b = P + A.se3.b;
    for (int k = 0; k < A.ncmd; ++k)
        for (int l = 0; l < 3; ++l) { h.br_w[k][l] = P + A.br[k][l].w; h.br_b[k][l] = P + A.br[k][l].b; }
    h.sp0_w = P + A.sp0.w; h.sp0_b = P + A.sp0.b; h.sp3_w = P + A.sp3.w; h.sp3_b = P + A.sp3.b;
    h.sp5_w = P + A.sp5.w; h.sp5_b = P + A.sp5.b;
    h.ncmd = A.ncmd; h.F = A.feat;
    return h;
}

// ------------------------------------------------------------------------------------------------
// Monte-Carlo dropout through the heads (mc_heads.hip)
// ------------------------------------------------------------------------------------------------
static int mc_check(const char* who, int batch, int samples, float p, const float* scratch,
                    size_t scratch_floats) {
    CILRS_CHECK(batch >= 1, "%s: batch %d", who, batch);
    CILRS_CHECK(samples >= 1 && samples <= kMcMaxSamples, "%s: samples %d outside 1..%d", who,
                samples, kMcMaxSamples);
    CILRS_CHECK((long long)batch * samples <= kMcMaxRows, "%s: batch * samples %lld above %d", who,
                (long long)batch * samples, kMcMaxRows);
    CILRS_CHECK(p >= 0.f && p < 1.f, "%s: dropout probability %f outside [0, 1)", who, (double)p);
    CILRS_CHECK(scratch != nullptr && scratch_floats >= mc_heads_scratch_floats(batch, samples),
                "%s: scratch of %zu floats, %zu needed", who, scratch_floats,
                mc_heads_scratch_floats(batch, samples));
    return 0;
}

size_t cilrs_heads_mc_scratch_floats(int variant, int batch, int samples) {
    if (!variant_ok(variant) || batch < 1 || samples < 1) return 0;
    return mc_heads_scratch_floats(batch, samples);
}

int cilrs_heads_mc(int variant, const float* params, const float* pooled, int pooled_ld,
                   const float* speed, const int64_t* command, int batch, int samples, float p,
                   uint64_t seed, float* mean, float* std, float* samples_out, float* scratch,
                   size_t scratch_floats, int* status, void* stream) {
    CILRS_CHECK(variant_ok(variant), "heads_mc: unknown architecture code %d", variant);
    CILRS_CHECK(params && pooled && speed && command && mean && std, "heads_mc: NULL tensor");
    if (mc_check("heads_mc", batch, samples, p, scratch, scratch_floats)) return 1;
    const Arch& A = arch(variant);
    CILRS_CHECK(pooled_ld >= A.feat, "heads_mc: pooled_ld %d below the %d features", pooled_ld, A.feat);
    CILRS_CHECK(((uintptr_t)params & 15) == 0, "heads_mc: params must be 16-byte aligned");
    McHeadsArgs a{};
    a.hw = head_weights(A, params);
    a.src = {pooled, pooled_ld, nullptr, 0};
    a.speed = speed; a.cmd = reinterpret_cast<const long long*>(command);
    a.B = batch; a.S = samples; a.p = p; a.seed = seed;
    a.mean = mean; a.stdv = std; a.samples_out = samples_out; a.status = status;
    return launch_mc_heads(a, scratch, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_net_heads_mc(cilrs_net* net, const cilrs_buffers* bufs, const float* speed,
                       const int64_t* command, int samples, float p, uint64_t seed, float* mean,
                       float* std, float* samples_out, float* scratch, size_t scratch_floats,
                       void* stream) {
    if (check_bufs(net, bufs, false)) return 1;
    CILRS_CHECK(speed && command && mean && std, "net_heads_mc: NULL tensor");
    if (mc_check("net_heads_mc", net->B, samples, p, scratch, scratch_floats)) return 1;
    McHeadsArgs a{};
    a.hw = head_weights(*net->A, bufs->params);
    if (plan_features_checked("net_heads_mc", net, bufs, &a.src)) return 1;
    a.speed = speed; a.cmd = reinterpret_cast<const long long*>(command);
    a.B = net->B; a.S = samples; a.p = p; a.seed = seed;
    a.mean = mean; a.stdv = std; a.samples_out = samples_out;
    a.status = status_words(net, bufs);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    RUN(net, "heads_mc", 2.0 * net->B * samples * 180480.0, 0.0, s, launch_mc_heads(a, scratch, s));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Grad-CAM (gradcam.hip)
// ------------------------------------------------------------------------------------------------
static int gc_weights(const char* who, const float* weights4, float* w) {
    CILRS_CHECK(weights4 != nullptr, "%s: NULL tensor (weights4)", who);
    for (int i = 0; i < 4; ++i) {
        CILRS_CHECK(std::isfinite(weights4[i]), "%s: output weight %d is not finite", who, i);
        w[i] = weights4[i];
    }
    return 0;
}

int cilrs_heads_input_grad(int variant, const float* params, const float* pooled, int pooled_ld,
                           const float* featmap, int hw, const float* speed, const int64_t* command,
                           const float* weights4, int batch, float* g, float* out4, int* status,
                           void* stream) {
    CILRS_CHECK(variant_ok(variant), "heads_input_grad: unknown architecture code %d", variant);
    CILRS_CHECK(params && speed && command && g, "heads_input_grad: NULL tensor");
    CILRS_CHECK((pooled != nullptr) != (featmap != nullptr),
                "heads_input_grad: exactly one of pooled and featmap must be given");
    CILRS_CHECK(batch >= 1, "heads_input_grad: batch %d", batch);
    const Arch& A = arch(variant);
    if (pooled) CILRS_CHECK(pooled_ld >= A.feat, "heads_input_grad: pooled_ld %d below the %d features",
                            pooled_ld, A.feat);
    else CILRS_CHECK(hw >= 1, "heads_input_grad: feature map of %d cells", hw);
    CILRS_CHECK(((uintptr_t)params & 15) == 0, "heads_input_grad: params must be 16-byte aligned");
    HeadsGradArgs a{};
    a.hw = head_weights(A, params);
    if (gc_weights("heads_input_grad", weights4, a.w)) return 1;
    a.src = {pooled, pooled_ld, featmap, hw};
    a.speed = speed; a.cmd = reinterpret_cast<const long long*>(command);
    a.B = batch; a.g = g; a.out4 = out4; a.status = status;
    return launch_heads_input_grad(a, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_gradcam_map(const float* A, const float* dA, const float* g, int batch, int h, int w,
                      int channels, int H, int W, float* cam, float* peak, float* heat,
                      uint8_t* heat_u8, void* stream) {
    GradcamMapArgs a;
    a.A = A; a.dA = dA; a.g = g;
    a.B = batch; a.h = h; a.w = w; a.C = channels; a.H = H; a.W = W;
    a.cam = cam; a.peak = peak; a.heat = heat; a.heat_u8 = heat_u8;
    return launch_gradcam_map(a, reinterpret_cast<hipStream_t>(stream));
}

size_t cilrs_gradcam_scratch_floats(int variant, int batch) {
    if (!variant_ok(variant) || batch < 1) return 0;
    return (size_t)batch * (arch(variant).feat + 4);
}

// last convolution of trunk group `layer` (1..4)
static int gc_group_conv(const Arch& A, int layer) {
    const BlockT& blk = A.blocks[A.layer_first[layer] - 1];
    return blk.conv3 >= 0 ? blk.conv3 : blk.conv2;
}

int cilrs_net_gradcam_info(const cilrs_net* net, int layer, size_t* a_offset, size_t* da_offset,
                           int* h, int* w, int* channels) {
    CILRS_CHECK(net != nullptr, "gradcam_info: net is NULL");
    CILRS_CHECK(layer >= 1 && layer <= 4, "gradcam_info: layer %d outside 1..4", layer);
    const int ci = gc_group_conv(*net->A, layer);
    if (a_offset) *a_offset = net->cg[ci].z;
    if (da_offset) *da_offset = net->G[3];
    if (h) *h = net->cg[ci].Ho;
    if (w) *w = net->cg[ci].Wo;
    if (channels) *channels = net->A->convs[ci].cout;
    return 0;
}

int cilrs_net_gradcam(cilrs_net* net, const cilrs_buffers* bufs, const float* speed,
                      const int64_t* command, const float* weights4, int layer, float* cam,
                      float* heat, uint8_t* heat_u8, float* peak, float* scratch,
                      size_t scratch_floats, void* stream) {
    if (check_bufs(net, bufs, false)) return 1;
    CILRS_CHECK(speed && command && cam && heat && peak, "net_gradcam: NULL tensor");
    CILRS_CHECK(layer >= 1 && layer <= 4, "net_gradcam: layer %d outside 1..4", layer);
    const Arch& A = *net->A;
    const size_t need = (size_t)net->B * (A.feat + 4);
    CILRS_CHECK(scratch != nullptr && scratch_floats >= need,
                "net_gradcam: scratch of %zu floats, %zu needed", scratch_floats, need);
    HeadsGradArgs ha{};
    ha.hw = head_weights(A, bufs->params);
    if (gc_weights("net_gradcam", weights4, ha.w)) return 1;
    CILRS_CHECK(!net->bf16_train, "net_gradcam: fp32 plans only (a CILRS_PLAN_BF16_TRAIN plan keeps "
                "16-bit feature maps)");
    CILRS_CHECK(!net->last.no_features(), "net_gradcam: no forward on this plan yet");
    CILRS_CHECK(!(net->last.train_features() && (net->ft_grad > 0 || net->ft_bn > 0)),
                "net_gradcam: the plan's last forward was a fine-tuning step behind a frozen prefix; "
                "run an eval-mode forward first");
    CILRS_CHECK(!net->last.train_features(), "net_gradcam: the plan's last forward ran in train mode (batch "
                "statistics); run an eval-mode forward first");
    CILRS_CHECK(net->last.half == 0, "net_gradcam: the plan's last forward ran a 16-bit (fp16 / bf16) "
                "trunk, whose feature maps are 16-bit; run an fp32 forward first");
    const int ci = gc_group_conv(A, layer);
    float* ws = reinterpret_cast<float*>(bufs->workspace);
    GradcamMapArgs ma;
    ma.A = ws + net->cg[ci].z; ma.dA = nullptr; ma.g = nullptr;
    ma.B = net->B; ma.h = net->cg[ci].Ho; ma.w = net->cg[ci].Wo; ma.C = A.convs[ci].cout;
    ma.H = net->H; ma.W = net->W;
    ma.cam = cam; ma.peak = peak; ma.heat = heat; ma.heat_u8 = heat_u8;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (layer == 4) {
        // the fast path: average pooling sits on layer4, so dA = (dy / d pooled) / (h * w)
        ha.src = plan_features(net, bufs);
        ha.speed = speed; ha.cmd = reinterpret_cast<const long long*>(command);
        ha.B = net->B; ha.g = scratch; ha.out4 = scratch + (size_t)net->B * A.feat;
        ha.status = status_words(net, bufs);
        ma.g = scratch;
        RUN(net, "gradcam", 4.0 * net->B * 180480.0, 0.0, s, launch_heads_input_grad(ha, s));
    } else {
        // the graph path: the data-gradient chain stopped at this group's boundary, G[3] holds dA
        CILRS_CHECK(net->last.frozen() && net->last.gc_bwd_end == 5 - layer,
                    "net_gradcam: layer %d needs cilrs_net_forward_frozen* followed by "
                    "cilrs_net_backward[_data] over segments [0, %d) on this plan: no matching "
                    "backward", layer, 5 - layer);
        ma.dA = ws + net->G[3];
    }
    RUN(net, "gradcam", 2.0 * net->B * ma.h * ma.w * ma.C, 0.0, s, launch_gradcam_map(ma, s));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Feature-space novelty (novelty.hip)
// ------------------------------------------------------------------------------------------------
constexpr int kNovMaxBatch = 65536;

// what both op-level entries check of their feature source and sizes
static int nov_check(const char* who, const float* features, int ld, const float* featmap, int hw,
                     const int64_t* command, int batch, int F, int NC) {
    CILRS_CHECK(command != nullptr, "%s: NULL tensor (command)", who);
    CILRS_CHECK(batch >= 1 && batch <= kNovMaxBatch, "%s: batch %d outside 1..%d", who, batch,
                kNovMaxBatch);
    CILRS_CHECK(F == 512 || F == 2048, "%s: feature width %d (512 or 2048)", who, F);
    CILRS_CHECK(NC >= 1 && NC <= kMaxCmd, "%s: %d commands outside 1..%d", who, NC, kMaxCmd);
    CILRS_CHECK((features != nullptr) != (featmap != nullptr),
                "%s: exactly one of features and featmap must be given", who);
    if (features) CILRS_CHECK(ld >= F, "%s: ld %d below the %d features", who, ld, F);
    else CILRS_CHECK(hw >= 1 && hw <= 65536, "%s: feature map of %d cells", who, hw);
    return 0;
}

static int nov_score_check(const char* who, const float* mean, const float* W, const float* d2,
                           const float* scratch, size_t scratch_floats, int F, int batch) {
    CILRS_CHECK(mean && W && d2, "%s: NULL tensor", who);
    CILRS_CHECK(scratch != nullptr && scratch_floats >= novelty_scratch_floats(F, batch),
                "%s: scratch of %zu floats, %zu needed", who, scratch_floats,
                novelty_scratch_floats(F, batch));
    CILRS_CHECK(((uintptr_t)W & 15) == 0 && ((uintptr_t)scratch & 15) == 0,
                "%s: W and scratch must be 16-byte aligned", who);
    return 0;
}

size_t cilrs_feature_moments_doubles(int F, int NC) {
    if ((F != 512 && F != 2048) || NC < 1 || NC > kMaxCmd) return 0;
    return novelty_moments_doubles(F, NC);
}

int cilrs_feature_moments(const float* features, int ld, const float* featmap, int hw,
                          const int64_t* command, int batch, int F, int NC, const float* pivot,
                          double* table, int* status, void* stream) {
    CILRS_CHECK(pivot && table, "feature_moments: NULL tensor");
    if (nov_check("feature_moments", features, ld, featmap, hw, command, batch, F, NC)) return 1;
    NoveltyMomentsArgs a;
    a.src = {features, ld, featmap, hw};
    a.cmd = reinterpret_cast<const long long*>(command);
    a.B = batch; a.F = F; a.NC = NC; a.pivot = pivot; a.table = table; a.status = status;
    return launch_novelty_moments(a, reinterpret_cast<hipStream_t>(stream));
}

size_t cilrs_feature_novelty_scratch_floats(int F, int batch) {
    if ((F != 512 && F != 2048) || batch < 1 || batch > kNovMaxBatch) return 0;
    return novelty_scratch_floats(F, batch);
}

int cilrs_feature_novelty(const float* features, int ld, const float* featmap, int hw,
                          const int64_t* command, int batch, int F, int NC, const float* mean,
                          const float* W, float* d2, float* scratch, size_t scratch_floats,
                          int* status, void* stream) {
    if (nov_check("feature_novelty", features, ld, featmap, hw, command, batch, F, NC)) return 1;
    if (nov_score_check("feature_novelty", mean, W, d2, scratch, scratch_floats, F, batch)) return 1;
    NoveltyScoreArgs a;
    a.src = {features, ld, featmap, hw};
    a.cmd = reinterpret_cast<const long long*>(command);
    a.B = batch; a.F = F; a.NC = NC; a.mean = mean; a.W = W; a.d2 = d2; a.status = status;
    return launch_novelty_score(a, scratch, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_net_feature_moments(cilrs_net* net, const cilrs_buffers* bufs, const int64_t* command,
                              const float* pivot, double* table, void* stream) {
    if (check_bufs(net, bufs, false)) return 1;
    CILRS_CHECK(command && pivot && table, "net_feature_moments: NULL tensor");
    NoveltyMomentsArgs a;
    if (plan_features_checked("net_feature_moments", net, bufs, &a.src)) return 1;
    const Arch& A = *net->A;
    CILRS_CHECK(net->B <= kNovMaxBatch, "net_feature_moments: batch %d above %d", net->B, kNovMaxBatch);
    a.cmd = reinterpret_cast<const long long*>(command);
    a.B = net->B; a.F = A.feat; a.NC = A.ncmd; a.pivot = pivot; a.table = table;
    a.status = status_words(net, bufs);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    RUN(net, "feature_moments", (double)net->B * A.feat * (A.feat + 1), 0.0, s,
        launch_novelty_moments(a, s));
    return 0;
}

int cilrs_net_novelty(cilrs_net* net, const cilrs_buffers* bufs, const int64_t* command,
                      const float* mean, const float* W, float* d2, float* scratch,
                      size_t scratch_floats, void* stream) {
    if (check_bufs(net, bufs, false)) return 1;
    CILRS_CHECK(command != nullptr, "net_novelty: NULL tensor (command)");
    const Arch& A = *net->A;
    CILRS_CHECK(net->B <= kNovMaxBatch, "net_novelty: batch %d above %d", net->B, kNovMaxBatch);
    if (nov_score_check("net_novelty", mean, W, d2, scratch, scratch_floats, A.feat, net->B)) return 1;
    NoveltyScoreArgs a;
    if (plan_features_checked("net_novelty", net, bufs, &a.src)) return 1;
    a.cmd = reinterpret_cast<const long long*>(command);
    a.B = net->B; a.F = A.feat; a.NC = A.ncmd; a.mean = mean; a.W = W; a.d2 = d2;
    a.status = status_words(net, bufs);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    RUN(net, "novelty", (double)net->B * A.feat * (A.feat + 1), 0.0, s,
        launch_novelty_score(a, scratch, s));
    return 0;
}

size_t cilrs_feature_whiten_scratch_floats(int F, int batch) {
    if ((F != 512 && F != 2048) || batch < 1 || batch > kNovMaxBatch) return 0;
    return (size_t)batch * F;
}

int cilrs_feature_whiten(const float* features, int ld, int batch, int F, const float* origin,
                         const float* W, float* y, float* scratch, size_t scratch_floats,
                         void* stream) {
    CILRS_CHECK(features && origin && W && y, "feature_whiten: NULL tensor");
    CILRS_CHECK(batch >= 1 && batch <= kNovMaxBatch, "feature_whiten: batch %d outside 1..%d", batch,
                kNovMaxBatch);
    CILRS_CHECK(F == 512 || F == 2048, "feature_whiten: feature width %d (512 or 2048)", F);
    CILRS_CHECK(ld >= F, "feature_whiten: ld %d below the %d features", ld, F);
    CILRS_CHECK(scratch != nullptr && scratch_floats >= (size_t)batch * F,
                "feature_whiten: scratch of %zu floats, %zu needed", scratch ? scratch_floats : (size_t)0,
                (size_t)batch * F);
    CILRS_CHECK(((uintptr_t)W & 15) == 0 && ((uintptr_t)scratch & 15) == 0,
                "feature_whiten: W and scratch must be 16-byte aligned");
    const NoveltyWhitenArgs a{{features, ld, nullptr, 0}, batch, F, origin, W, scratch, y};
    return launch_novelty_whiten(a, reinterpret_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------
// Nearest neighbours of the tick's features (knn.hip)
// ------------------------------------------------------------------------------------------------
// scratch: u [B][F] | y [B][F] | the lists of cilrs_knn
size_t cilrs_net_knn_scratch_bytes(int F, int batch, int N, int K) {
    const size_t lists = knn_scratch_bytes(N, batch, K);
    if ((F != 512 && F != 2048) || lists == 0) return 0;
    return 2 * (size_t)batch * F * sizeof(float) + lists;
}

int cilrs_net_knn(cilrs_net* net, const cilrs_buffers* bufs, const float* X, long ld, int N,
                  const float* origin, const float* W, int K, int64_t* idx, float* dist,
                  void* scratch, size_t scratch_bytes, void* stream) {
    if (check_bufs(net, bufs, false)) return 1;
    const Arch& A = *net->A;
    const int F = A.feat, B = net->B;
    CILRS_CHECK((origin != nullptr) == (W != nullptr), "net_knn: origin and W go together");
    CILRS_CHECK(W == nullptr || ((uintptr_t)W & 15) == 0, "net_knn: W must be 16-byte aligned");
    const size_t rows = (size_t)B * F * sizeof(float);
    CILRS_CHECK(scratch != nullptr && scratch_bytes >= 2 * rows,
                "net_knn: scratch of %zu bytes, needs %zu", scratch ? scratch_bytes : (size_t)0,
                cilrs_net_knn_scratch_bytes(F, B, N, K));
    float* u = reinterpret_cast<float*>(scratch);
    KnnArgs k{X, ld, N, F, W ? u + (size_t)B * F : u, F, B, nullptr, K, idx, dist,
              reinterpret_cast<char*>(scratch) + 2 * rows};
    if (knn_check("net_knn", k, scratch_bytes - 2 * rows)) return 1;
    NoveltyWhitenArgs a;
    if (plan_features_checked("net_knn", net, bufs, &a.src)) return 1;
    a.B = B; a.F = F; a.origin = origin; a.W = W; a.u = u; a.y = u + (size_t)B * F;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    RUN(net, "knn_features", W ? (double)B * F * (F + 1) : 0.0, 0.0, s, launch_novelty_whiten(a, s));
    RUN(net, "knn", 3.0 * B * (double)N * F, (double)N * F * 4.0 * ((B + 7) / 8), s, launch_knn(k, s));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
// One backward call: what every launch of the pass is made from.  backward_impl fills it once; the
// per-segment functions below take it and keep nothing of their own between calls (what does
// outlive a launch or a call is cilrs_net::bwd).
struct BwdPass {
    cilrs_net* net;
    const cilrs_buffers* bufs;
    const Arch& A;
    float* ws;
    const float* P;
    float* Gp;                 // the gradient arena; nullptr in a data-only pass
    hipStream_t s;
    // data_only (cilrs_net_backward_data): the data-gradient chain alone -- no weight gradient, no
    // head dW / db, nothing on the side stream, bufs->grads never touched
    bool data_only;
    // data-only pass over a frozen graph: BatchNorm backward without reductions (one launch per
    // layer), data gradients without the BatchNorm-partials epilogue
    bool lean_bn;
    bool bf16t;                // bf16 training mode: the trunk's tensors after the stem are bf16
    // fine-tuning: the graph ends where the frozen prefix begins -- segments of frozen groups are
    // not run, and the first block of the last trainable group hands nothing further down
    int cut;
    // cilrs_net_backward_step: Adam's update of a segment follows its gradients (nullptr: none)
    const cilrs_adam_args* fused_adam;

    // gradient buffers by index: [3] d(block input / output), [1] identity-path gradient, [2]
    // d(input of a main-branch convolution), ring slots = dy tensors; fp32 mode: ws + G[i]; bf16
    // mode: the bf16 buffer G16[i]
    float* Gf(int gi) const { return ws + net->G[gi]; }
    cilrs_half* Gh(int gi) const { return h16(ws, net->G16[gi]); }
    cilrs_half* z16_of(int ci) const { return h16(ws, net->z16[ci]); }
    int next_ring() const {
        const int gi = kRingIdx[net->bwd.dy_pos];
        net->bwd.dy_pos = (net->bwd.dy_pos + 1) % kDyRing;
        return gi;
    }
    // where a BatchNorm backward leaves dgamma / dbeta: the arena, or (data-only pass over a
    // train-mode graph, whose reductions still feed dx) a scratch nobody reads
    float* dgamma_of(const BnT& b) const { return data_only ? ws + net->bn_coef + 3 * 2048 : Gp + b.gamma; }
    float* dbeta_of(const BnT& b) const { return data_only ? ws + net->bn_coef + 4 * 2048 : Gp + b.beta; }

    // weight gradient of conv `c` from dy (buffer gi): runs on side stream 0, concurrently with
    // the data gradients (x: the conv's input activation; x16: its bf16 form)
    int wgrad_side(const ConvT& c, const ConvG& g, const float* x, const cilrs_half* x16, int gi,
                   size_t dw_off) const {
        if (data_only) return 0;
        float* const dwdst = Gp + dw_off;
        if (side_fork(net, s)) return 1;
        if (bf16t) {
            if (conv_wgrad16(net, c, g, x16, Gh(gi), dwdst, ws, side_or(net, s, 0))) return 1;
        } else {
            if (conv_wgrad(net, c, g, x, c.cin, Gf(gi), dwdst, ws, side_or(net, s, 0))) return 1;
        }
        return gbuf_side_end(net, gi);
    }
    // data gradient of conv `ci`: dy (buffer gi) -> buffer go (+ buffer gadd, -1: none); bn_of /
    // nbp: the convolution whose BatchNorm-backward reductions ride on the epilogue, and where the
    // number of partials goes; out32: the bf16 mode's last data gradient of the trunk, handed to
    // the fp32 stem
    int dgrad(int ci, int gi, int go, int gadd, const ConvG* bn_of, int* nbp,
              bool out32 = false) const {
        const ConvT& c = A.convs[ci];
        const ConvG& g = net->cg[ci];
        if (lean_bn) { bn_of = nullptr; nbp = nullptr; }
        if (bf16t)
            return conv_dgrad16(net, c, g, Gh(gi), out32 ? nullptr : Gh(go),
                                out32 ? Gf(go) : nullptr, gadd >= 0 ? Gh(gadd) : nullptr, ws, s,
                                bn_of, nbp);
        return conv_dgrad(net, c, g, Gf(gi), P + c.w, Gf(go), gadd >= 0 ? Gf(gadd) : nullptr, ws, s,
                          bn_of, 1, nbp);
    }
    // BatchNorm backward of conv `ci`: dz (buffer gz) -> dy (buffer gdy), masked gradient ->
    // buffer gg (-1: not needed); pre_nblk: partials a data gradient's epilogue already left
    int bnb(int ci, int gz, int relu, int gdy, int gg, int pre_nblk, double passes) const {
        const ConvT& c = A.convs[ci];
        const ConvG& g = net->cg[ci];
        const BnT& b = A.bns[c.bn];
        const std::string label = std::string("bn_bwd.") + kGroupName[c.group];
        if (lean_bn) {
            RUN(net, label, 0.0,
                4.0 * g.M * c.cout * (2.0 + (relu ? 1.0 : 0.0) + (gg >= 0 ? 1.0 : 0.0)), s,
                launch_bn_bwd_frozen(Gf(gz), relu ? ws + g.z : nullptr, g.M, c.cout, P + b.gamma,
                                     ws + g.stats, relu, Gf(gdy), gg >= 0 ? Gf(gg) : nullptr, s));
        } else if (bf16t) {
            RUN(net, label, 0.0, 2.0 * g.M * c.cout * passes, s,
                launch_bn16_bwd(Gh(gz), relu ? z16_of(ci) : nullptr, y16_of(net, ws, ci), g.M,
                                c.cout, P + b.gamma, ws + g.stats, relu, dgamma_of(b), dbeta_of(b),
                                ws + net->bn_coef, ws + net->bn_partial, Gh(gdy),
                                gg >= 0 ? Gh(gg) : nullptr, pre_nblk, s));
        } else {
            RUN(net, label, 0.0, 4.0 * g.M * c.cout * passes, s,
                launch_bn_bwd(Gf(gz), relu ? ws + g.z : nullptr, ws + g.y, g.M, c.cout, P + b.gamma,
                              ws + g.stats, relu, dgamma_of(b), dbeta_of(b), 0, ws + net->bn_coef,
                              ws + net->bn_partial, Gf(gdy), gg >= 0 ? Gf(gg) : nullptr, pre_nblk,
                              s, nullptr, net->last.frozen() ? 1 : 0));
        }
        return 0;
    }
    // cilrs_net_backward_step: segment `seg`'s gradients are complete once the main stream reaches
    // this point (BatchNorm / head gradients) and the side stream has run what it holds (weight
    // gradients): its Adam update goes on the side stream behind both
    int segment_done(int seg) const {
        const cilrs_adam_args* o = fused_adam;
        if (!o) return 0;
        const size_t b = A.seg_begin[seg], n = A.seg_end[seg] - A.seg_begin[seg];
        hipStream_t st = s;
        if (use_overlap(net)) {
            if (side_fork(net, s)) return 1;       // side waits for the main stream's part
            st = net->side[0];
        }
        RUN(net, "adam", 0.0, 28.0 * n, st,
            launch_adam(bufs->params + b, Gp + b, o->exp_avg + b, o->exp_avg_sq + b, n, o->lr,
                        o->beta1, o->beta2, o->eps, o->weight_decay, (long long)o->step, nullptr,
                        o->grad_scale, st));
        return 0;
    }
};

static int last_conv(const BlockT& blk) { return blk.conv3 >= 0 ? blk.conv3 : blk.conv2; }

// the heads of segment 0: d controls / d predicted speed -> d combined (ws + dcombined), d(speed
// encoder) in ws + ds1, and every head layer's dW / db
static int backward_heads(const BwdPass& bp, const float* dcontrols, const float* dps) {
    cilrs_net* net = bp.net;
    const Arch& A = bp.A;
    const int feat = A.feat, comb = A.feat + 128;
    float* ws = bp.ws;
    const float* P = bp.P;
    float* Gp = bp.Gp;
    const bool data_only = bp.data_only;
    hipStream_t s = bp.s;
    const int B = net->B;
    const float dscale = net->last.dropout > 0.f ? 1.0f / (1.0f - net->last.dropout) : 1.0f;
    const long long* cmd = reinterpret_cast<const long long*>(
        reinterpret_cast<const char*>(bp.bufs->workspace) + net->cmd_b);
    float* dcomb = ws + net->dcombined;

    // weight + bias gradient of layer l:  dW[out][in] = dy^T x,  db = colsum(dy)
    auto wg = [&](HGemmGroup& g, const float* dy, int dy_ld, const float* x, int x_ld,
                  const LinT& l) {
        memset(&g, 0, sizeof(g));
        if (data_only) return;       // (run(2, ...) launches nothing then)
        g.A = dy; g.lda = dy_ld; g.B = x; g.ldb = x_ld; g.C = Gp + l.w; g.ldc = l.in;
        g.dbias = Gp + l.b; g.M = l.out; g.N = l.in; g.K = B;
    };
    // input gradient of layer l:  dx = (dy W) masked by act > 0, scaled
    auto dg = [&](HGemmGroup& g, const float* dy, int dy_ld, const LinT& l, float* dx, int dx_ld,
                  const float* act, int act_ld, float scale) {
        memset(&g, 0, sizeof(g));
        g.A = dy; g.lda = dy_ld; g.B = P + l.w; g.ldb = l.in; g.C = dx; g.ldc = dx_ld;
        g.mask = act; g.ldmask = act_ld; g.mask_scale = scale; g.M = B; g.N = l.in; g.K = l.out;
    };
    // mode 2 = weight + bias gradients: nothing on the main stream reads them -- they go to the side
    // stream (idle at this point of the backward pass, and these launches occupy a handful of
    // CUs), behind the output gradient they multiply; backward_join joins them at the call's end
    auto run = [&](int mode, HGemmArgs& h, int n) -> int {
        if (mode == 2 && data_only) return 0;
        h.ngroups = n; h.relu = 0; h.accumulate = 0; h.drop_p = 0.f; h.seed = 0;
        double fl = 0.0;
        for (int i = 0; i < n; ++i) fl += 2.0 * h.g[i].M * h.g[i].N * h.g[i].K;
        hipStream_t st = s;
        if (mode == 2 && use_overlap(net)) {
            if (side_fork(net, s)) return 1;
            st = net->side[0];
        }
        RUN(net, "heads_bwd", fl, 0.0, st, launch_hgemm(mode, h, st));
        if (st != s) {
            CILRS_HIP(hipEventRecord(net->heads_ev, st));
            net->bwd.heads_pending = true;
        }
        return 0;
    };
    HGemmArgs h;
    memset(&h, 0, sizeof(h));

    // ---- only the commanded branch of each frame receives gradient (gather) ----
    const int NC = A.ncmd;
    RUN(net, "heads_bwd", 0.0, 0.0, s,
        launch_branch_scatter(dcontrols, cmd, ws + net->d_all, B, NC, s));
    const float* d_out[kMaxCmd];
    for (int k = 0; k < NC; ++k) d_out[k] = ws + net->d_all + (size_t)k * B * 4;

    // ---- output layers (256 -> 3 per branch, 256 -> 1 speed predictor) ----
    for (int k = 0; k < NC; ++k) wg(h.g[k], d_out[k], 4, ws + net->h2[k], 256, A.br[k][2]);
    wg(h.g[NC], dps, 1, ws + net->p2, 256, A.sp5);
    if (run(2, h, NC + 1)) return 1;
    for (int k = 0; k < NC; ++k)
        dg(h.g[k], d_out[k], 4, A.br[k][2], ws + net->dh2[k], 256, ws + net->h2[k], 256, dscale);
    dg(h.g[NC], dps, 1, A.sp5, ws + net->dp2, 256, ws + net->p2, 256, 1.0f);
    if (run(1, h, NC + 1)) return 1;
    // ---- middle layers (256 -> 256) ----
    for (int k = 0; k < NC; ++k) wg(h.g[k], ws + net->dh2[k], 256, ws + net->h1[k], 256, A.br[k][1]);
    wg(h.g[NC], ws + net->dp2, 256, ws + net->p1, 256, A.sp3);
    if (run(2, h, NC + 1)) return 1;
    for (int k = 0; k < NC; ++k)
        dg(h.g[k], ws + net->dh2[k], 256, A.br[k][1], ws + net->dh1[k], 256, ws + net->h1[k], 256,
           dscale);
    dg(h.g[NC], ws + net->dp2, 256, A.sp3, ws + net->dp1, 256, ws + net->p1, 256, dscale);
    if (run(1, h, NC + 1)) return 1;
    // ---- first layers (feat+128 -> 256 per branch; feat -> 256 speed predictor, visual half
    //      only; 640 / 512 for the reference's ResNet-34 trunk) ----
    for (int k = 0; k < NC; ++k)
        wg(h.g[k], ws + net->dh1[k], 256, ws + net->combined, comb, A.br[k][0]);
    wg(h.g[NC], ws + net->dp1, 256, ws + net->combined, comb, A.sp0);
    if (run(2, h, NC + 1)) return 1;
    for (int k = 0; k < NC; ++k)
        dg(h.g[k], ws + net->dh1[k], 256, A.br[k][0], ws + net->dcomb_part[k], comb, nullptr, 0, 1.f);
    dg(h.g[NC], ws + net->dp1, 256, A.sp0, ws + net->dcomb_part[NC], comb, nullptr, 0, 1.f);
    if (run(1, h, NC + 1)) return 1;
    // d combined = sum of the branch contributions (comb wide) + speed predictor (feat wide)
    SumParts parts;
    memset(&parts, 0, sizeof(parts));
    parts.n = NC;
    for (int k = 0; k < NC; ++k) parts.p[k] = ws + net->dcomb_part[k];
    parts.tail = ws + net->dcomb_part[NC];
    RUN(net, "heads_bwd", 0.0, 0.0, s, launch_sum_parts(parts, dcomb, B, comb, feat, s));
    // ---- speed encoder (the speed half of `combined`) ----
    RUN(net, "heads_bwd", 0.0, 0.0, s,
        launch_relu_mask(dcomb + feat, ws + net->combined + feat, B, 128, comb, comb, 1.0f, s));
    wg(h.g[0], dcomb + feat, comb, ws + net->s1, 128, A.se3);
    if (run(2, h, 1)) return 1;
    dg(h.g[0], dcomb + feat, comb, A.se3, ws + net->ds1, 128, ws + net->s1, 128, dscale);
    if (run(1, h, 1)) return 1;
    wg(h.g[0], ws + net->ds1, 128, ws + net->speed_in, 1, A.se0);
    if (run(2, h, 1)) return 1;
    return 0;
}

// segment 0: the heads, then d visual -> avgpool backward -> grad of the last block's output, in G[3]
static int backward_head_segment(const BwdPass& bp, const float* dcontrols,
                                 const float* dpred_speed) {
    cilrs_net* net = bp.net;
    const Arch& A = bp.A;
    float* ws = bp.ws;
    hipStream_t s = bp.s;
    CILRS_CHECK(dcontrols && dpred_speed, "backward: output gradients missing");
    if (backward_heads(bp, dcontrols, dpred_speed)) return 1;
    if (bp.cut == 5) {
        // (whole trunk frozen: nobody reads d(feature map))
    } else if (bp.bf16t)
        RUN(net, "heads_bwd", 0.0, 0.0, s,
            launch_avgpool_bwd16(ws + net->dcombined, bp.Gh(3), net->B, net->featHW, A.feat,
                                 A.feat + 128, s));
    else
        RUN(net, "heads_bwd", 0.0, 0.0, s,
            launch_avgpool_bwd(ws + net->dcombined, bp.Gf(3), net->B, net->featHW, A.feat,
                               A.feat + 128, s));
    return bp.segment_done(0);
}

// One residual block, blocks[bi]; the gradient of its output is in G[3], that of its input ends
// there.  boundary: the first block of the last trainable group of a fine-tuning step.
// prev_runs: the block below belongs to this layer walk (it is neither another layer's nor one the
// walk skips).  *nblk_next: BatchNorm-backward partials that the block above left for this
// block's last BatchNorm on its way in, and those this block leaves for the next on its way out.
static int backward_block(const BwdPass& bp, int bi, bool boundary, bool prev_runs,
                          int* nblk_next) {
    cilrs_net* net = bp.net;
    const Arch& A = bp.A;
    float* ws = bp.ws;
    hipStream_t s = bp.s;
    const BlockT& blk = A.blocks[bi];
    // conv-BN pairs of the main branch, in forward order (2: BasicBlock, 3: Bottleneck)
    const int chain[3] = {blk.conv1, blk.conv2, blk.conv3};
    const int nchain = blk.conv3 >= 0 ? 3 : 2;
    const ConvT& c1 = A.convs[blk.conv1];
    const ConvG& g1 = net->cg[blk.conv1];
    // block input activation, and its bf16 form
    const float* xin = bi == 0 ? ws + net->pool : ws + net->cg[last_conv(A.blocks[bi - 1])].z;
    const cilrs_half* xin16 =
        bi == 0 ? h16(ws, net->pool16) : bp.z16_of(last_conv(A.blocks[bi - 1]));
    // 1. out = relu(bn_last(y_last) + identity): masked grad -> [1], dy_last -> ga
    int ga = bp.next_ring();
    if (gbuf_acquire(net, s, ga) || gbuf_acquire(net, s, 1)) return 1;
    if (bp.bnb(chain[nchain - 1], 3, 1, ga, 1, *nblk_next, 8.0)) return 1;
    *nblk_next = 0;
    // 2. walk the main branch backwards: dW_i (side), d(input of conv_i) -> [2], then
    //    a = relu(bn_{i-1}(y_{i-1})): dy_{i-1} -> the next dy buffer
    for (int i = nchain - 1; i >= 1; --i) {
        const ConvT& c = A.convs[chain[i]];
        const ConvG& g = net->cg[chain[i]];
        const ConvG& gp = net->cg[chain[i - 1]];
        if (bp.wgrad_side(c, g, ws + gp.z, bp.z16_of(chain[i - 1]), ga, c.w)) return 1;
        if (gbuf_acquire(net, s, 2)) return 1;
        int nbp = 0;    // the previous BatchNorm's reductions ride on this dgrad's epilogue
        if (bp.dgrad(chain[i], ga, 2, -1, &gp, &nbp)) return 1;
        ga = bp.next_ring();
        if (gbuf_acquire(net, s, ga)) return 1;
        if (bp.bnb(chain[i - 1], 2, 1, ga, -1, nbp, 7.0)) return 1;
    }
    // 3. dW1 (side)
    if (bp.wgrad_side(c1, g1, xin, xin16, ga, c1.w)) return 1;
    if (boundary) {
        // its input belongs to the frozen prefix -- no data gradient leaves it (*nblk_next stays
        // 0); the down-sample branch still takes its own BatchNorm backward and weight gradient
        if (blk.down >= 0) {
            const ConvT& cd = A.convs[blk.down];
            const ConvG& gd = net->cg[blk.down];
            const int gdn = bp.next_ring();
            if (gbuf_acquire(net, s, gdn)) return 1;
            if (bp.bnb(blk.down, 1, 0, gdn, -1, 0, 6.0)) return 1;
            if (bp.wgrad_side(cd, gd, xin, xin16, gdn, cd.w)) return 1;
        }
    } else if (blk.down < 0) {
        // 4. dx = dgrad(conv1) + identity grad [1] -> [3]
        // ... and carries the reductions of the previous block's last BatchNorm
        const ConvG* prev = prev_runs ? &net->cg[last_conv(A.blocks[bi - 1])] : nullptr;
        if (bp.dgrad(blk.conv1, ga, 3, 1, prev, nblk_next, bi == 0)) return 1;
    } else {
        const ConvT& cd = A.convs[blk.down];
        const ConvG& gd = net->cg[blk.down];
        if (bp.dgrad(blk.conv1, ga, 3, -1, nullptr, nullptr)) return 1;
        // 5. identity = bn_d(conv_d(x)) (no ReLU): dy_d -> a dy buffer
        const int gdn = bp.next_ring();
        if (gbuf_acquire(net, s, gdn)) return 1;
        if (bp.bnb(blk.down, 1, 0, gdn, -1, 0, 6.0)) return 1;
        if (bp.wgrad_side(cd, gd, xin, xin16, gdn, cd.w)) return 1;
        // 6. dx += dgrad(conv_d)
        if (bp.dgrad(blk.down, gdn, 3, 3, nullptr, nullptr, bi == 0)) return 1;
    }
    return 0;
}

// segments 1..4 = layer4..layer1: the layer's blocks, last to first
static int backward_layer(const BwdPass& bp, int seg) {
    const int layer = 5 - seg;
    const int first = bp.A.layer_first[layer - 1], end = bp.A.layer_first[layer];
    const int cut_block = layer == bp.cut ? first : -1;      // boundary block of a fine-tuning cut
    // Partials of a block's last BatchNorm backward, written by the data gradient of the block
    // above.  Only a block without a down-sample branch hands them on, and only to a block of the
    // same layer: a layer's first block either has that branch or is block 0, and a boundary block
    // hands on nothing, so the count is 0 wherever a layer ends.
    int nblk_next = 0;
    for (int bi = end - 1; bi >= first; --bi) {
        // (boundary block: no data gradient leaves it, and a data-only pass wants none of its
        //  weight gradients -- nor, in the block above, the reductions nobody would read)
        const bool skipped = bp.data_only && bi == cut_block;
        const bool prev_skipped = bp.data_only && bi - 1 == cut_block;
        if (skipped) continue;
        if (backward_block(bp, bi, bi == cut_block, bi > first && !prev_skipped, &nblk_next))
            return 1;
    }
    // (the segment's weight gradients are complete when this call returns its work: the side
    //  stream joins at the end of the call -- between the segments of ONE call the data-gradient
    //  chain does not wait for the weight gradients any more)
    return bp.segment_done(seg);
}

// segment 5: the stem.  G[3] holds d(maxpool output)
static int backward_stem(const BwdPass& bp) {
    cilrs_net* net = bp.net;
    float* ws = bp.ws;
    const float* P = bp.P;
    hipStream_t s = bp.s;
    const int B = net->B;
    const ConvT& c0 = bp.A.convs[0];
    const ConvG& g0 = net->cg[0];
    const BnT& b0 = bp.A.bns[c0.bn];
    const unsigned char* argmax =
        reinterpret_cast<const unsigned char*>(bp.bufs->workspace) + net->argmax_b;
    // max-pool backward + ReLU mask are rebuilt inside the BatchNorm-backward passes
    if (gbuf_acquire(net, s, 1)) return 1;           // G[1] is rewritten below
    if (bp.lean_bn)
        RUN(net, "bn_bwd.stem", 0.0, 4.0 * g0.M * 64 * 2.5, s,
            launch_bn_bwd_pool_frozen(ws + net->G[3], argmax, ws + g0.y, B, net->H0, net->W0, 64,
                                      P + b0.gamma, ws + g0.stats, ws + net->G[1], s));
    else
        RUN(net, "bn_bwd.stem", 0.0, 4.0 * g0.M * 64 * 3.0, s,
            launch_bn_bwd_pool(ws + net->G[3], argmax, ws + g0.y, B, net->H0, net->W0, 64,
                               P + b0.gamma, ws + g0.stats, bp.dgamma_of(b0), bp.dbeta_of(b0),
                               ws + net->bn_coef, ws + net->bn_partial, ws + net->G[1], s,
                               net->last.frozen() ? 1 : 0));
    // the stem's weight gradient runs on the main stream and uses the same slab scratch as the
    // weight gradients of the side stream: those must have finished (between the segments of one
    // call nothing else joins the two streams any more)
    if (gbuf_join_all(net, s)) return 1;
    const size_t sw = stem_wgrad_f32_scratch_floats(B, net->H, net->W);
    if (bp.data_only) {
        // (no weight gradient)
    } else if (sw > 0 && sw <= net->slabs_floats) {
        // (the reduction over pixels on the matrix pipe, dy from global memory, the input rows in
        //  LDS: stem_f32.hip)
        RUN(net, "conv_wgrad.stem", 2.0 * g0.M * 64 * 147,
            16.0 * B * net->H * net->W + 4.0 * g0.M * 64, s,
            launch_stem_wgrad_f32(ws + net->x4, ws + net->G[1], bp.Gp + c0.w, ws + net->slabs, B,
                                  net->H, net->W, s));
    } else if (conv_wgrad(net, c0, g0, ws + net->x4, 4, ws + net->G[1], bp.Gp + c0.w, ws, s)) {
        return 1;
    }
    return bp.segment_done(5);
}

// end of a call: everything the side stream still runs (weight gradients, the heads' weight
// gradients, fused Adam launches) joins the main stream here
static int backward_join(const BwdPass& bp) {
    cilrs_net* net = bp.net;
    if (gbuf_join_all(net, bp.s)) return 1;
    if (net->bwd.heads_pending) {
        CILRS_HIP(hipStreamWaitEvent(bp.s, net->heads_ev, 0));
        net->bwd.heads_pending = false;
    }
    if (bp.fused_adam && use_overlap(net)) {
        CILRS_HIP(hipEventRecord(net->fork_ev, net->side[0]));
        CILRS_HIP(hipStreamWaitEvent(bp.s, net->fork_ev, 0));
    }
    return 0;
}

// segments [seg_begin, seg_end) of the backward pass on the plan's last graph-keeping forward:
// argument checks, the cut, the record in cilrs_net::last, one function per segment, the join
static int backward_impl(cilrs_net* net, const cilrs_buffers* bufs, const float* dcontrols,
                         const float* dpred_speed, int seg_begin, int seg_end, void* stream,
                         const bool data_only, const cilrs_adam_args* fused_adam = nullptr) {
    if (check_bufs(net, bufs, !data_only)) return 1;
    CILRS_CHECK(net->last.keeps_graph(), "backward needs a preceding train-mode forward on this plan");
    CILRS_CHECK(0 <= seg_begin && seg_begin <= seg_end && seg_end <= 6, "bad segment range");
    const int cut = net->ft_grad;
    if (seg_end > 6 - cut) seg_end = 6 - cut;
    if (seg_begin > seg_end) seg_begin = seg_end;
    float* ws = reinterpret_cast<float*>(bufs->workspace);
    net->ws_base = ws;
    const BwdPass bp{net, bufs, *net->A, ws, bufs->params, data_only ? nullptr : bufs->grads,
                     reinterpret_cast<hipStream_t>(stream), data_only,
                     data_only && net->last.frozen(), net->bf16_train, cut, fused_adam};

    // (segment 0 rewrites d(speed encoder); segments 1..5 cycle the buffer G[1] that segment 5
    //  leaves d(stem conv output) in)
    if (seg_begin == 0) net->last.bwd_done = 0;
    if (seg_begin <= 5 && seg_end > 1) net->last.bwd_done &= ~(1u << 5);
    // where G[3] stands once this call has gone through (cilrs_net_gradcam): a run from segment 0,
    // or the continuation of one (every forward resets gc_bwd_end); until then nothing
    const bool gc_run = seg_begin == 0 || net->last.gc_bwd_end == seg_begin;
    net->last.gc_bwd_end = -1;
    for (int seg = seg_begin; seg < seg_end; ++seg) {
        if (seg == 0) {
            if (backward_head_segment(bp, dcontrols, dpred_speed)) return 1;
            net->last.bwd_done |= 1u;
        } else if (seg <= 4) {
            if (backward_layer(bp, seg)) return 1;
        } else {
            if (backward_stem(bp)) return 1;
            net->last.bwd_done |= 1u << 5;
        }
    }
    if (backward_join(bp)) return 1;
    if (gc_run) net->last.gc_bwd_end = seg_end;
    return 0;
}

int cilrs_net_backward(cilrs_net* net, const cilrs_buffers* bufs, const float* dcontrols,
                       const float* dpred_speed, int seg_begin, int seg_end, void* stream) {
    return backward_impl(net, bufs, dcontrols, dpred_speed, seg_begin, seg_end, stream, false);
}

int cilrs_net_backward_data(cilrs_net* net, const cilrs_buffers* bufs, const float* dcontrols,
                            const float* dpred_speed, int seg_begin, int seg_end, void* stream) {
    return backward_impl(net, bufs, dcontrols, dpred_speed, seg_begin, seg_end, stream, true);
}

// Backward of every segment with torch.optim.Adam.step() (notebook/notebook.ipynb:555) fused in:
// the update of a segment's parameter range is enqueued -- on the weight-gradient stream, behind
// that segment's weight gradients -- as soon as the segment's gradients are complete, so the
// HBM-bound update of layer4 (13 M of the 21 M parameters) runs under the matrix-pipe-bound data
// gradients of layers 3..1 instead of after the stem.  Same arithmetic per element as
// cilrs_adam_step over the whole arena (no gradient clipping: the global norm needs every
// gradient first -- callers that clip use cilrs_net_backward + cilrs_grad_sqnorm + cilrs_adam_step).
int cilrs_net_backward_step(cilrs_net* net, const cilrs_buffers* bufs, const float* dcontrols,
                            const float* dpred_speed, const cilrs_adam_args* opt, void* stream) {
    CILRS_CHECK(net && opt && opt->exp_avg && opt->exp_avg_sq, "backward_step: NULL argument");
    CILRS_CHECK(opt->step >= 1, "backward_step: step must be >= 1");
    CILRS_CHECK(net->ft_grad == 0, "backward_step: the last forward froze %d trunk group(s); one step "
                "count for the whole arena cannot serve it (use cilrs_net_backward + cilrs_adam_step "
                "on the trainable range)", net->ft_grad);
    return backward_impl(net, bufs, dcontrols, dpred_speed, 0, 6, stream, false, opt);
}

int cilrs_net_input_grads(cilrs_net* net, const cilrs_buffers* bufs, float* dimage, long sn, long sc,
                          long sh, long sw, float* dspeed, void* stream) {
    if (check_bufs(net, bufs, false)) return 1;
    CILRS_CHECK(net->last.keeps_graph(), "input_grads needs a preceding graph-keeping forward on this plan");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const Arch& A = *net->A;
    float* ws = reinterpret_cast<float*>(bufs->workspace);
    const int B = net->B;
    if (dspeed) {
        CILRS_CHECK(net->last.bwd_done & 1u, "input_grads: dspeed needs segment 0 (heads) of "
                    "cilrs_net_backward after the forward");
        // speed -> Linear(1, 128): d speed = d(pre-activation) . W_se0 (ds1 is masked by ReLU and
        // dropout and dropout-scaled in backward_heads)
        RUN(net, "heads_bwd.dspeed", 2.0 * B * 128, 4.0 * B * 129, s,
            launch_rowdot(ws + net->ds1, bufs->params + A.se0.w, dspeed, B, 128, 128, s));
    }
    if (dimage) {
        CILRS_CHECK(net->ft_grad == 0, "input_grads: the last forward froze %d trunk group(s); the "
                    "backward pass stops there, there is no image gradient", net->ft_grad);
        CILRS_CHECK(net->last.bwd_done & (1u << 5), "input_grads: dimage needs segment 5 (stem) of "
                    "cilrs_net_backward after the forward");
        const ConvG& g0 = net->cg[0];
        RUN(net, "conv_dgrad.stem", 2.0 * g0.M * 64 * 147,
            4.0 * g0.M * 64 + 12.0 * B * net->H * net->W, s,
            launch_stem_dgrad_f32(ws + net->G[1], bufs->params + A.convs[0].w, dimage, sn, sc, sh, sw,
                                  B, net->H, net->W, s));
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// loss / optimiser / profiling
// ------------------------------------------------------------------------------------------------
int cilrs_loss_fwd_bwd(const float* controls, const float* target_controls,
                       const float* pred_speed, const float* target_speed, int batch, int kind,
                       const float* weights4_host, float grad_scale, float* dcontrols,
                       float* dpred_speed, float* loss_out, void* stream) {
    CILRS_CHECK(controls && target_controls && pred_speed && target_speed && weights4_host &&
                    loss_out, "loss: NULL argument");
    CILRS_CHECK(batch >= 1, "loss: batch must be >= 1");
    return launch_loss(controls, target_controls, pred_speed, target_speed, batch, kind,
                       weights4_host, grad_scale, dcontrols, dpred_speed, loss_out,
                       reinterpret_cast<hipStream_t>(stream));
}

size_t cilrs_sqnorm_scratch_bytes(void) { return sqnorm_scratch_bytes(); }

int cilrs_grad_sqnorm(const float* grads, size_t n, float max_norm, void* scratch, float* out2,
                      void* stream) {
    CILRS_CHECK(grads && scratch && out2, "grad_sqnorm: NULL argument");
    return launch_grad_sqnorm(grads, n, max_norm, reinterpret_cast<double*>(scratch), out2,
                              reinterpret_cast<hipStream_t>(stream));
}

int cilrs_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                    size_t n, double lr, double beta1, double beta2, double eps,
                    double weight_decay, int64_t step, const float* clip_out2, float grad_scale,
                    void* stream) {
    CILRS_CHECK(params && grads && exp_avg && exp_avg_sq, "adam: NULL argument");
    return launch_adam(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay,
                       (long long)step, clip_out2, grad_scale,
                       reinterpret_cast<hipStream_t>(stream));
}

int cilrs_adam_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                           size_t n, int ngroups, const size_t* ends, const double* lrs,
                           const int64_t* steps, double beta1, double beta2, double eps,
                           double weight_decay, const float* clip_out2, float grad_scale,
                           void* stream) {
    CILRS_CHECK(params && grads && exp_avg && exp_avg_sq, "adam: NULL argument");
    long long st[kAdamTableMax];
    for (int r = 0; r < ngroups && r < kAdamTableMax; ++r) st[r] = (long long)steps[r];
    return launch_adam_groups(params, grads, exp_avg, exp_avg_sq, n, ngroups, ends, lrs, st, beta1,
                              beta2, eps, weight_decay, clip_out2, grad_scale,
                              reinterpret_cast<hipStream_t>(stream));
}

// exponential moving average of the weights, on the optimizer step (notebook/notebook.ipynb:555)
int cilrs_ema_update(float* ema, const float* params, size_t n, float w, void* stream) {
    return launch_ema_update(ema, params, n, w, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_swap(float* a, float* b, size_t n, void* stream) {
    return launch_swap(a, b, n, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_adam_step_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                        size_t n, double lr, double beta1, double beta2, double eps,
                        double weight_decay, int64_t step, const float* clip_out2,
                        float grad_scale, float* ema, float ema_w, void* stream) {
    CILRS_CHECK(params && grads && exp_avg && exp_avg_sq, "adam: NULL argument");
    return launch_adam_ema(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps,
                           weight_decay, (long long)step, clip_out2, grad_scale, ema, ema_w,
                           reinterpret_cast<hipStream_t>(stream));
}

int cilrs_adam_step_groups_ema(float* params, const float* grads, float* exp_avg,
                               float* exp_avg_sq, size_t n, int ngroups, const size_t* ends,
                               const double* lrs, const int64_t* steps, double beta1, double beta2,
                               double eps, double weight_decay, const float* clip_out2,
                               float grad_scale, float* ema, float ema_w, void* stream) {
    CILRS_CHECK(params && grads && exp_avg && exp_avg_sq, "adam: NULL argument");
    CILRS_CHECK(ngroups >= 1 && ngroups <= kAdamTableMax && steps, "adam: 1..%d ranges",
                kAdamTableMax);
    long long st[kAdamTableMax];
    for (int r = 0; r < ngroups; ++r) st[r] = (long long)steps[r];
    return launch_adam_groups_ema(params, grads, exp_avg, exp_avg_sq, n, ngroups, ends, lrs, st,
                                  beta1, beta2, eps, weight_decay, clip_out2, grad_scale, ema,
                                  ema_w, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_stem_conv_fwd(const float* x4, const float* w, float* y, float* bn_partial, int N, int H,
                        int W, int* partial_rows, void* stream) {
    CILRS_CHECK(x4 && w && y, "stem_conv_fwd: NULL argument");
    const int rows = stem_f32_rows(N, H, W);
    CILRS_CHECK(rows > 0, "stem_conv_fwd: geometry %dx%dx%d not served", N, H, W);
    if (partial_rows) *partial_rows = rows;
    return launch_stem_f32(x4, w, y, bn_partial, N, H, W, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_stem_conv_dgrad(const float* dy, const float* w, float* dx, long sn, long sc, long sh,
                          long sw, int N, int H, int W, void* stream) {
    CILRS_CHECK(dy && w && dx, "stem_conv_dgrad: NULL argument");
    return launch_stem_dgrad_f32(dy, w, dx, sn, sc, sh, sw, N, H, W,
                                 reinterpret_cast<hipStream_t>(stream));
}

size_t cilrs_stem_conv_wgrad_scratch_floats(int N, int H, int W) {
    return stem_wgrad_f32_scratch_floats(N, H, W);
}
int cilrs_stem_conv_wgrad(const float* x4, const float* dy, float* dw, float* scratch,
                          size_t scratch_floats, int N, int H, int W, void* stream) {
    CILRS_CHECK(x4 && dy && dw && scratch, "stem_conv_wgrad: NULL argument");
    const size_t need = stem_wgrad_f32_scratch_floats(N, H, W);
    CILRS_CHECK(need > 0, "stem_conv_wgrad: geometry %dx%dx%d not served", N, H, W);
    CILRS_CHECK(scratch_floats >= need, "stem_conv_wgrad: scratch too small");
    return launch_stem_wgrad_f32(x4, dy, dw, scratch, N, H, W, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_scale(float* x, size_t n, const float* clip_out2, float c, void* stream) {
    CILRS_CHECK(x != nullptr, "scale: NULL argument");
    return launch_scale(x, n, clip_out2, c, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_augment_u8(const uint8_t* frames, const cilrs_aug_params* params, int batch, int height,
                     int width, float* out_f32, uint8_t* out_u8, void* stream) {
    CILRS_CHECK(frames && params && (out_f32 || out_u8), "augment: NULL argument");
    static_assert(sizeof(cilrs_aug_params) == 112, "cilrs_aug_params layout");
    return launch_augment_u8(frames, params, batch, height, width, out_f32, out_u8,
                             reinterpret_cast<hipStream_t>(stream));
}

int cilrs_batch_assemble(const uint8_t* cache, int64_t n_frames, const float* speed,
                         const int64_t* command, const float* targets, const int64_t* index,
                         const cilrs_aug_params* params, int batch, int height, int width,
                         float* out_f32, uint8_t* out_u8, float* out_speed, int64_t* out_command,
                         float* out_targets, void* stream) {
    CILRS_CHECK(batch >= 1, "batch_assemble: batch must be at least 1");
    CILRS_CHECK(cache && index && params && (out_f32 || out_u8), "batch_assemble: NULL argument");
    CILRS_CHECK((!out_speed || speed) && (!out_command || command) && (!out_targets || targets),
                "batch_assemble: a label output needs its label array");
    return launch_batch_assemble(cache, n_frames, speed,
                                 reinterpret_cast<const long long*>(command), targets,
                                 reinterpret_cast<const long long*>(index), params, batch, height,
                                 width, out_f32, out_u8, out_speed,
                                 reinterpret_cast<long long*>(out_command), out_targets,
                                 reinterpret_cast<hipStream_t>(stream));
}

int cilrs_augment_weather_u8(const uint8_t* frames, const cilrs_aug_params* params,
                             const cilrs_weather_params* weather, int batch, int height, int width,
                             float* out_f32, uint8_t* out_u8, void* stream) {
    CILRS_CHECK(frames && params && weather && (out_f32 || out_u8),
                "augment_weather: NULL argument");
    static_assert(sizeof(cilrs_weather_params) == 96, "cilrs_weather_params layout");
    return launch_augment_weather_u8(frames, params, weather, batch, height, width, out_f32, out_u8,
                                     reinterpret_cast<hipStream_t>(stream));
}

int cilrs_batch_assemble_weather(const uint8_t* cache, int64_t n_frames, const float* speed,
                                 const int64_t* command, const float* targets,
                                 const int64_t* index, const cilrs_aug_params* params,
                                 const cilrs_weather_params* weather, int batch, int height,
                                 int width, float* out_f32, uint8_t* out_u8, float* out_speed,
                                 int64_t* out_command, float* out_targets, void* stream) {
    CILRS_CHECK(batch >= 1, "batch_assemble_weather: batch must be at least 1");
    CILRS_CHECK(cache && index && params && weather && (out_f32 || out_u8),
                "batch_assemble_weather: NULL argument");
    CILRS_CHECK((!out_speed || speed) && (!out_command || command) && (!out_targets || targets),
                "batch_assemble_weather: a label output needs its label array");
    return launch_batch_assemble_weather(cache, n_frames, speed,
                                         reinterpret_cast<const long long*>(command), targets,
                                         reinterpret_cast<const long long*>(index), params, weather,
                                         batch, height, width, out_f32, out_u8, out_speed,
                                         reinterpret_cast<long long*>(out_command), out_targets,
                                         reinterpret_cast<hipStream_t>(stream));
}

int cilrs_augment_view_u8(const uint8_t* frames, const cilrs_aug_params* params,
                          const cilrs_weather_params* weather, const cilrs_view_params* view,
                          int batch, int height, int width, float* out_f32, uint8_t* out_u8,
                          void* stream) {
    CILRS_CHECK(frames && params && view && (out_f32 || out_u8), "augment_view: NULL argument");
    static_assert(sizeof(cilrs_view_params) == 96, "cilrs_view_params layout");
    return launch_augment_view_u8(frames, params, weather, view, batch, height, width, out_f32,
                                  out_u8, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_batch_assemble_view(const uint8_t* cache, int64_t n_frames, const float* speed,
                              const int64_t* command, const float* targets, const int64_t* index,
                              const cilrs_aug_params* params, const cilrs_weather_params* weather,
                              const cilrs_view_params* view, int batch, int height, int width,
                              float* out_f32, uint8_t* out_u8, float* out_speed,
                              int64_t* out_command, float* out_targets, void* stream) {
    CILRS_CHECK(batch >= 1, "batch_assemble_view: batch must be at least 1");
    CILRS_CHECK(cache && index && params && view && (out_f32 || out_u8),
                "batch_assemble_view: NULL argument");
    CILRS_CHECK((!out_speed || speed) && (!out_command || command) && (!out_targets || targets),
                "batch_assemble_view: a label output needs its label array");
    return launch_batch_assemble_view(cache, n_frames, speed,
                                      reinterpret_cast<const long long*>(command), targets,
                                      reinterpret_cast<const long long*>(index), params, weather,
                                      view, batch, height, width, out_f32, out_u8, out_speed,
                                      reinterpret_cast<long long*>(out_command), out_targets,
                                      reinterpret_cast<hipStream_t>(stream));
}

// op-level nn.Linear (the kernels the heads launch, one group)
int cilrs_linear_fwd(const float* x, const float* w, const float* bias, float* y, int batch,
                     int in_features, int out_features, int x_ld, int y_ld, int relu,
                     void* stream) {
    CILRS_CHECK(x && w && y && batch >= 1 && in_features >= 1 && out_features >= 1,
                "linear_fwd: bad argument");
    HGemmArgs h;
    memset(&h, 0, sizeof(h));
    HGemmGroup& g = h.g[0];
    g.A = x; g.lda = x_ld; g.B = w; g.ldb = in_features; g.bias = bias; g.C = y; g.ldc = y_ld;
    g.M = batch; g.N = out_features; g.K = in_features; g.drop_stream = kNoDrop;
    h.ngroups = 1; h.relu = relu;
    return launch_hgemm(0, h, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_linear_bwd(const float* dy, const float* x, const float* w, const float* act,
                     float act_scale, float* dx, float* dw, float* db, int batch,
                     int in_features, int out_features, int dy_ld, int x_ld, int dx_ld,
                     int act_ld, void* stream) {
    CILRS_CHECK(dy && x && w && batch >= 1 && in_features >= 1 && out_features >= 1,
                "linear_bwd: bad argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HGemmArgs h;
    if (dw) {
        memset(&h, 0, sizeof(h));
        HGemmGroup& g = h.g[0];
        g.A = dy; g.lda = dy_ld; g.B = x; g.ldb = x_ld; g.C = dw; g.ldc = in_features;
        g.dbias = db; g.M = out_features; g.N = in_features; g.K = batch;
        h.ngroups = 1;
        if (launch_hgemm(2, h, s)) return 1;
    }
    if (dx) {
        memset(&h, 0, sizeof(h));
        HGemmGroup& g = h.g[0];
        g.A = dy; g.lda = dy_ld; g.B = w; g.ldb = in_features; g.C = dx; g.ldc = dx_ld;
        g.mask = act; g.ldmask = act_ld; g.mask_scale = act_scale;
        g.M = batch; g.N = in_features; g.K = out_features;
        h.ngroups = 1;
        if (launch_hgemm(1, h, s)) return 1;
    }
    return 0;
}

int cilrs_eval_acc_doubles(void) { return kEvalAccDoubles; }

int cilrs_eval_accumulate(const float* controls, const float* pred_speed,
                          const float* target_controls, const float* target_speed,
                          const int64_t* command, int batch, double* acc, float* steer_abs_err,
                          void* stream) {
    CILRS_CHECK(controls && pred_speed && target_controls && target_speed && command && acc,
                "eval_accumulate: NULL argument");
    CILRS_CHECK(batch >= 1, "eval_accumulate: empty batch");
    return launch_eval_accumulate(controls, target_controls, pred_speed, target_speed,
                                  reinterpret_cast<const long long*>(command), batch, acc,
                                  steer_abs_err, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_net_profile_enable(cilrs_net* net, int on) {
    CILRS_CHECK(net != nullptr, "profile: net is NULL");
    net->prof.on = on != 0;
    return 0;
}
int cilrs_net_profile_collect(cilrs_net* net) {
    CILRS_CHECK(net != nullptr, "profile: net is NULL");
    return net->prof.collect();
}
int cilrs_net_profile_count(const cilrs_net* net) { return net ? (int)net->prof.labels.size() : 0; }
int cilrs_net_profile_entry(const cilrs_net* net, int i, char* label, int label_cap,
                            long long* calls, double* total_ms, double* total_flops,
                            double* total_bytes) {
    CILRS_CHECK(net && i >= 0 && i < (int)net->prof.labels.size(), "profile: bad index");
    if (label && label_cap > 0) snprintf(label, label_cap, "%s", net->prof.labels[i].c_str());
    const ProfAgg& a = net->prof.agg[i];
    if (calls) *calls = a.calls;
    if (total_ms) *total_ms = a.ms;
    if (total_flops) *total_flops = a.flops;
    if (total_bytes) *total_bytes = a.bytes;
    return 0;
}
int cilrs_net_profile_reset(cilrs_net* net) {
    CILRS_CHECK(net != nullptr, "profile: net is NULL");
    if (net->prof.collect()) return 1;
    for (auto& a : net->prof.agg) a = ProfAgg();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// op-level entry points (unit parity tests)
// ------------------------------------------------------------------------------------------------
// the problems the op-level convolution entries hand the launchers: dense NHWC / OHWI tensors
static ConvArgs make_conv_fwd(const float* x, const float* w, float* y, int N, int H, int W, int Cin,
                              int Cout, int KH, int KW, int stride, int pad, int force_cfg,
                              int force_splitk, float* scratch, size_t scratch_floats) {
    ConvArgs a = conv_args(N, H, W, Cin, Cout, KH, KW, stride, pad);
    a.x = x; a.w = w; a.y = y;
    a.scratch = scratch; a.scratch_floats = scratch_floats;
    a.force_cfg = force_cfg; a.force_splitk = force_splitk;
    return a;
}

static DgradArgs make_conv_dgrad(const float* dy, const float* w, float* dx, const float* addend,
                                 int N, int H, int W, int Cin, int Cout, int K, int stride, int pad,
                                 int force_cfg, int force_splitk, float* scratch,
                                 size_t scratch_floats) {
    DgradArgs a = dgrad_args(N, H, W, Cin, Cout, K, stride, pad);
    a.dy = dy; a.w = w; a.dx = dx; a.addend = addend;
    a.scratch = scratch; a.scratch_floats = scratch_floats;
    a.force_cfg = force_cfg; a.force_splitk = force_splitk;
    return a;
}

int cilrs_conv2d_fwd(const float* x, const float* w, float* y, int N, int H, int W, int Cin,
                     int Cout, int KH, int KW, int stride, int pad, int force_cfg,
                     int force_splitk, float* scratch, size_t scratch_floats, void* stream) {
    const ConvArgs a = make_conv_fwd(x, w, y, N, H, W, Cin, Cout, KH, KW, stride, pad, force_cfg,
                                     force_splitk, scratch, scratch_floats);
    return launch_conv_igemm(a, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_conv2d_dgrad(const float* dy, const float* w, float* dx, const float* addend, int N,
                       int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                       int force_cfg, int force_splitk, float* scratch, size_t scratch_floats,
                       void* stream) {
    CILRS_CHECK(KH == KW, "dgrad: square kernels only");
    const DgradArgs a = make_conv_dgrad(dy, w, dx, addend, N, H, W, Cin, Cout, KH, stride, pad,
                                        force_cfg, force_splitk, scratch, scratch_floats);
    return launch_conv_dgrad(a, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_conv2d_fwd_stats(const float* x, const float* w, float* y, float* partial, int* nblk,
                           int N, int H, int W, int Cin, int Cout, int K, int stride, int pad,
                           int force_cfg, int force_splitk, float* scratch, size_t scratch_floats,
                           void* stream) {
    CILRS_CHECK(x && w && y && partial && nblk, "conv2d_fwd_stats: NULL argument");
    ConvArgs a = make_conv_fwd(x, w, y, N, H, W, Cin, Cout, K, K, stride, pad, force_cfg,
                               force_splitk, scratch, scratch_floats);
    a.bn_partial = partial; a.bn_nblk = nblk; *nblk = 0;
    // the caller's buffer holds cilrs_bn_partial_floats(Cout): as many row groups as the BatchNorm kernels use
    CILRS_CHECK((size_t)(cdiv(N * a.Ho * a.Wo, 64) + kConvMultiMax) * 2 * Cout <= bn_partial_floats(Cout),
                "conv2d_fwd_stats: more than %zu rows", bn_partial_floats(Cout) / 2 / Cout * 64);
    return launch_conv_igemm(a, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_conv2d_dgrad_bnbwd(const float* dy, const float* w, float* dx, const float* addend,
                             const float* bwd_z, const float* bwd_y, const float* bwd_stats,
                             int bwd_relu, float* partial, int* nblk, int N, int H, int W, int Cin,
                             int Cout, int K, int stride, int pad, int force_cfg, int force_splitk,
                             float* scratch, size_t scratch_floats, void* stream) {
    CILRS_CHECK(dy && w && dx && bwd_y && bwd_stats && partial && nblk && (bwd_z || !bwd_relu),
                "conv2d_dgrad_bnbwd: NULL argument");
    CILRS_CHECK(stride == 1, "conv2d_dgrad_bnbwd: stride 1 only");
    DgradArgs a = make_conv_dgrad(dy, w, dx, addend, N, H, W, Cin, Cout, K, stride, pad, force_cfg,
                                  force_splitk, scratch, scratch_floats);
    a.bwd_z = bwd_z; a.bwd_y = bwd_y; a.bwd_stats = bwd_stats; a.bwd_relu = bwd_relu;
    a.bwd_partial = partial; a.bwd_nblk = nblk; *nblk = 0;
    CILRS_CHECK((size_t)(cdiv(N * H * W, 64) + kConvMultiMax) * 2 * Cin <= bn_partial_floats(Cin),
                "conv2d_dgrad_bnbwd: more than %zu rows", bn_partial_floats(Cin) / 2 / Cin * 64);
    return launch_conv_dgrad(a, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_conv2d_takes_classes(int N, int H, int W, int Cin, int Cout, int K, int stride, int pad,
                               int dgrad, size_t scratch_floats, int force_splitk) {
    return conv_igemm_takes_classes(N, H, W, Cin, Cout, K, stride, pad, dgrad != 0, scratch_floats,
                                    force_splitk) ? 1 : 0;
}

int cilrs_conv2d_plan_info(int N, int H, int W, int Cin, int Cout, int K, int stride, int pad,
                           int dgrad, size_t scratch_floats, int force_cfg, int force_splitk,
                           int* cfg, int* splitk, int* class_tiles, int* parity_fused) {
    CILRS_CHECK(cfg && splitk && class_tiles && parity_fused, "conv2d_plan_info: NULL argument");
    CILRS_CHECK(N >= 1 && K >= 1 && K * K <= 16 && (stride == 1 || stride == 2) && pad >= 0 &&
                    H + 2 * pad >= K && W + 2 * pad >= K,
                "conv2d_plan_info: bad geometry");
    CILRS_CHECK(Cin >= 4 && Cin % 4 == 0 && Cout >= 4 && Cout % 4 == 0 &&
                    (dgrad ? Cin : Cout) % 64 == 0,
                "conv2d_plan_info: channel counts %d -> %d", Cin, Cout);
    // (never read: split-K is only considered when there is a scratch pointer)
    float* const scratch = scratch_floats ? reinterpret_cast<float*>(sizeof(float) * 4) : nullptr;
    ConvPlanInfo info;
    if (dgrad) {
        if (conv_dgrad_plan_info(make_conv_dgrad(nullptr, nullptr, nullptr, nullptr, N, H, W, Cin, Cout,
                                                 K, stride, pad, force_cfg, force_splitk, scratch,
                                                 scratch_floats),
                                 &info))
            return 1;
    } else if (conv_igemm_plan_info(make_conv_fwd(nullptr, nullptr, nullptr, N, H, W, Cin, Cout, K, K,
                                                  stride, pad, force_cfg, force_splitk, scratch,
                                                  scratch_floats),
                                    &info)) {
        return 1;
    }
    *cfg = info.cfg; *splitk = info.splitk; *class_tiles = info.class_tiles;
    *parity_fused = info.parity_fused;
    return 0;
}

int cilrs_net_conv_classes(const cilrs_net* net, int conv, int* fwd, int* dgrad) {
    CILRS_CHECK(net != nullptr, "conv_classes: net is NULL");
    CILRS_CHECK(conv >= 0 && conv < (int)net->cg.size(), "conv_classes: conv %d out of range", conv);
    const ConvT& c = net->A->convs[conv];
    const ConvG& g = net->cg[conv];
    // the stem has kernels of its own; a Winograd layer never reaches the implicit GEMM; the
    // 16-bit train mode runs other kernels
    const bool igemm = conv > 0 && net->wino_slot[conv] < 0 && !net->bf16_train;
    const bool yes_f = igemm && conv_igemm_takes_classes(net->B, g.H, g.W, c.cin, c.cout, c.k, c.stride,
                                                         c.pad, false, net->ksplit_floats);
    const bool yes_d = igemm && conv_igemm_takes_classes(net->B, g.H, g.W, c.cin, c.cout, c.k, c.stride,
                                                         c.pad, true, net->ksplit_floats);
    if (fwd) *fwd = yes_f ? 1 : 0;
    if (dgrad) *dgrad = yes_d ? 1 : 0;
    return 0;
}

size_t cilrs_conv2d_wgrad_scratch_floats(int N, int H, int W, int Cin, int Cout, int KH, int KW,
                                         int stride, int pad) {
    return wgrad_scratch_floats(wgrad_args(N, H, W, Cin, Cout, KH, KW, stride, pad, Cin));
}

int cilrs_conv2d_wgrad(const float* x, const float* dy, float* dw, float* scratch, int N, int H,
                       int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                       int Cin_dst, void* stream) {
    WgradArgs a = wgrad_args(N, H, W, Cin, Cout, KH, KW, stride, pad, Cin_dst);
    a.x = x; a.dy = dy; a.dw = dw; a.slabs = scratch;
    return launch_conv_wgrad(a, reinterpret_cast<hipStream_t>(stream));
}

// ---- the same three convolution operators on the 16-bit matrix pipe (operands rounded to bf16 /
//      fp16, fp32 accumulation and results): the kernels of the bf16 training mode, op by op ----
static size_t up8(size_t v) { return (v + 7) / 8 * 8; }
size_t cilrs_conv2d_16_scratch_halfs(int N, int H, int W, int Cin, int Cout, int K, int stride,
                                     int pad) {
    const int Ho = (H + 2 * pad - K) / stride + 1, Wo = (W + 2 * pad - K) / stride + 1;
    return up8((size_t)N * H * W * Cin) + up8((size_t)N * Ho * Wo * Cout) +
           2 * up8((size_t)Cout * K * K * Cin);
}

int cilrs_conv2d_fwd_16(const float* x, const float* w, float* y, float* bn_partial, int N, int H,
                        int W, int Cin, int Cout, int K, int stride, int pad, int bf16,
                        void* scratch16, void* stream) {
    CILRS_CHECK(x && w && y && scratch16, "conv2d_fwd_16: NULL argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    cilrs_half* x16 = reinterpret_cast<cilrs_half*>(scratch16);
    cilrs_half* w16 = x16 + up8((size_t)N * H * W * Cin);
    if (launch_f32_to_f16(x, x16, (size_t)N * H * W * Cin, bf16, s)) return 1;
    if (launch_f32_to_f16(w, w16, (size_t)Cout * K * K * Cin, bf16, s)) return 1;
    ConvF16Args a;
    memset(&a, 0, sizeof(a));
    a.x = x16; a.w = w16; a.y32 = y; a.bn_partial = bn_partial;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.K = K; a.stride = stride; a.pad = pad;
    a.Ho = (H + 2 * pad - K) / stride + 1; a.Wo = (W + 2 * pad - K) / stride + 1;
    a.bf16 = bf16;
    return launch_conv_f16_train(a, s);
}

int cilrs_conv2d_dgrad_16(const float* dy, const float* w, float* dx, const float* addend, int N,
                          int H, int W, int Cin, int Cout, int K, int stride, int pad, int bf16,
                          void* scratch16, void* stream) {
    CILRS_CHECK(dy && w && dx && scratch16, "conv2d_dgrad_16: NULL argument");
    CILRS_CHECK(stride == 1 || stride == 2, "conv2d_dgrad_16: stride must be 1 or 2");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int Ho = (H + 2 * pad - K) / stride + 1, Wo = (W + 2 * pad - K) / stride + 1;
    cilrs_half* dy16 = reinterpret_cast<cilrs_half*>(scratch16);
    cilrs_half* wT16 = dy16 + up8((size_t)N * Ho * Wo * Cout);
    if (launch_f32_to_f16(dy, dy16, (size_t)N * Ho * Wo * Cout, bf16, s)) return 1;
    if (launch_transpose_flip_f16(w, wT16, Cout, K, Cin, bf16, s)) return 1;
    ConvF16Args a;
    memset(&a, 0, sizeof(a));
    a.x = dy16; a.w = wT16; a.y32 = dx; a.addend32 = addend;
    a.N = N; a.H = Ho; a.W = Wo; a.Cin = Cout;       // gathered tensor = dy
    a.Ho = H; a.Wo = W; a.Cout = Cin;                // enumerated grid = dx
    a.K = K; a.bf16 = bf16;
    if (stride == 1) { a.stride = 1; a.pad = K - 1 - pad; }
    else { a.stride = 2; a.pad = pad; a.up2 = 1; }
    return launch_conv_f16_train(a, s);
}

static WgradF16Args make_wgrad16(const void* x16, const void* dy16, float* dw, float* slabs, int N,
                                 int H, int W, int Cin, int Cout, int K, int stride, int pad,
                                 int bf16) {
    WgradF16Args a;
    memset(&a, 0, sizeof(a));
    a.x = x16; a.dy = dy16; a.dw = dw; a.slabs = slabs;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.K = K; a.stride = stride; a.pad = pad;
    a.Ho = (H + 2 * pad - K) / stride + 1; a.Wo = (W + 2 * pad - K) / stride + 1;
    a.bf16 = bf16;
    return a;
}

size_t cilrs_conv2d_wgrad_16_scratch_floats(int N, int H, int W, int Cin, int Cout, int K,
                                            int stride, int pad) {
    return wgrad_f16_scratch_floats(
        make_wgrad16(nullptr, nullptr, nullptr, nullptr, N, H, W, Cin, Cout, K, stride, pad, 1));
}

int cilrs_conv2d_wgrad_16(const float* x, const float* dy, float* dw, float* scratch32, int N,
                          int H, int W, int Cin, int Cout, int K, int stride, int pad, int bf16,
                          void* scratch16, void* stream) {
    CILRS_CHECK(x && dy && dw && scratch32 && scratch16, "conv2d_wgrad_16: NULL argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int Ho = (H + 2 * pad - K) / stride + 1, Wo = (W + 2 * pad - K) / stride + 1;
    cilrs_half* x16 = reinterpret_cast<cilrs_half*>(scratch16);
    cilrs_half* dy16 = x16 + up8((size_t)N * H * W * Cin);
    if (launch_f32_to_f16(x, x16, (size_t)N * H * W * Cin, bf16, s)) return 1;
    if (launch_f32_to_f16(dy, dy16, (size_t)N * Ho * Wo * Cout, bf16, s)) return 1;
    return launch_wgrad_f16(
        make_wgrad16(x16, dy16, dw, scratch32, N, H, W, Cin, Cout, K, stride, pad, bf16), s);
}

// ---- the bf16 training mode's operators on 16-bit tensors (round 4: activations and gradients
//      live in bf16 end to end), op by op ----
int cilrs_conv2d_train_16(const void* x16, const void* w16, void* y16, float* y32,
                          const void* addend16, float* bn_partial, const void* bwd_z16,
                          const void* bwd_y16, const float* bwd_stats, int bwd_relu,
                          float* bwd_partial, int N, int H, int W, int Cin, int Ho, int Wo, int Cout,
                          int K, int stride, int pad, int up2, int bf16, int* partial_rows,
                          void* stream) {
    CILRS_CHECK(x16 && w16 && (y16 || y32), "conv2d_train_16: NULL argument");
    ConvF16Args a;
    memset(&a, 0, sizeof(a));
    a.x = reinterpret_cast<const cilrs_half*>(x16);
    a.w = reinterpret_cast<const cilrs_half*>(w16);
    a.y16 = reinterpret_cast<cilrs_half*>(y16);
    a.y32 = y16 ? nullptr : y32;
    a.addend16 = reinterpret_cast<const cilrs_half*>(addend16);
    a.bn_partial = bn_partial;
    a.bwd_z16 = reinterpret_cast<const cilrs_half*>(bwd_z16);
    a.bwd_y16 = reinterpret_cast<const cilrs_half*>(bwd_y16);
    a.bwd_stats = bwd_stats; a.bwd_relu = bwd_relu; a.bwd_partial = bwd_partial;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Ho = Ho; a.Wo = Wo; a.Cout = Cout;
    a.K = K; a.stride = stride; a.pad = pad; a.up2 = up2; a.bf16 = bf16;
    CILRS_CHECK(!bwd_partial || conv_f16_train_can_fuse_bwd(a),
                "conv2d_train_16: BatchNorm-backward partials are not available for this launch");
    if (partial_rows) *partial_rows = conv_f16_train_mtiles(a);
    return launch_conv_f16_train(a, reinterpret_cast<hipStream_t>(stream));
}

// ---- the 16-bit INFERENCE trunk's operators (folded BatchNorm, one rounding per stored tensor),
//      op by op: what trunk_fwd_eval16 / fold_prep launch ----
int cilrs_conv2d_infer_16(const void* x16, const void* w16, const float* bias,
                          const void* residual16, void* y16, int N, int H, int W, int Cin, int Cout,
                          int K, int stride, int pad, int relu, int bf16, int tile, void* stream) {
    CILRS_CHECK(x16 && w16 && bias && y16, "conv2d_infer_16: NULL argument");
    CILRS_CHECK(N >= 1 && H >= 1 && W >= 1 && K >= 1 && (stride == 1 || stride == 2) && pad >= 0 &&
                    H + 2 * pad >= K && W + 2 * pad >= K,
                "conv2d_infer_16: bad geometry");
    CILRS_CHECK(tile == 0 || (tile == 128 && Cout % 128 == 0),
                "conv2d_infer_16: tile is 0 (the plan's choice) or 128 (needs Cout %% 128 == 0)");
    CILRS_CHECK(((uintptr_t)x16 & 15) == 0 && ((uintptr_t)w16 & 15) == 0 &&
                    ((uintptr_t)residual16 & 15) == 0 && ((uintptr_t)y16 & 15) == 0,
                "conv2d_infer_16: 16-bit tensors must be 16-byte aligned");
    ConvF16Args a;
    memset(&a, 0, sizeof(a));
    a.x = reinterpret_cast<const cilrs_half*>(x16);
    a.w = reinterpret_cast<const cilrs_half*>(w16);
    a.bias = bias;
    a.residual = reinterpret_cast<const cilrs_half*>(residual16);
    a.y = reinterpret_cast<cilrs_half*>(y16);
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.K = K; a.stride = stride; a.pad = pad;
    a.Ho = (H + 2 * pad - K) / stride + 1; a.Wo = (W + 2 * pad - K) / stride + 1;
    a.relu = relu; a.bf16 = bf16;
    return launch_conv_f16(a, reinterpret_cast<hipStream_t>(stream), tile);
}

int cilrs_stem_fold_16(const float* w, const float* stats, void* w16, float* bias, int bf16,
                       void* stream) {
    CILRS_CHECK(w && stats && w16 && bias, "stem_fold_16: NULL argument");
    return launch_fold_stem_f16(w, stats, w16, bias, bf16, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_stem_infer_16(const float* x4, const void* w16, const float* bias, void* z16, int N, int H,
                        int W, int bf16, void* stream) {
    CILRS_CHECK(x4 && w16 && bias && z16, "stem_infer_16: NULL argument");
    CILRS_CHECK(N >= 1 && H >= 1 && W >= 1, "stem_infer_16: bad geometry");
    CILRS_CHECK(((uintptr_t)x4 & 15) == 0 && ((uintptr_t)w16 & 15) == 0 && ((uintptr_t)z16 & 15) == 0,
                "stem_infer_16: tensors must be 16-byte aligned");
    return launch_stem_f16(x4, w16, bias, z16, N, H, W, bf16, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_maxpool_infer_16(const void* x16, void* out16, int N, int H, int W, int C, int bf16,
                           void* stream) {
    CILRS_CHECK(x16 && out16, "maxpool_infer_16: NULL argument");
    CILRS_CHECK(N >= 1 && H >= 1 && W >= 1 && C >= 8, "maxpool_infer_16: bad geometry");
    CILRS_CHECK(((uintptr_t)x16 & 15) == 0 && ((uintptr_t)out16 & 15) == 0,
                "maxpool_infer_16: tensors must be 16-byte aligned");
    return launch_maxpool_f16(x16, out16, N, H, W, C, bf16, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_avgpool_infer_16(const void* x16, float* out, int N, int HW, int C, int out_ld, int bf16,
                           void* stream) {
    CILRS_CHECK(x16 && out, "avgpool_infer_16: NULL argument");
    CILRS_CHECK(N >= 1 && HW >= 1 && C >= 1 && out_ld >= C, "avgpool_infer_16: bad geometry");
    return launch_avgpool_f16(x16, out, N, HW, C, out_ld, bf16, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_bn16_train_fwd(const void* y16, int M, int C, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, int64_t* nbt, float momentum,
                         float eps, const void* residual16, int relu, float* stats, float* partial,
                         void* z16, int pre_rows, void* stream) {
    CILRS_CHECK(y16 && gamma && beta && stats && partial, "bn16_train_fwd: NULL argument");
    return launch_bn16_train_fwd(y16, M, C, gamma, beta, running_mean, running_var,
                                 reinterpret_cast<long long*>(nbt), momentum, eps, residual16, relu,
                                 stats, partial, z16, pre_rows, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_bn16_bwd(const void* dz16, const void* z16, const void* y16, int M, int C,
                   const float* gamma, const float* stats, int relu, float* dgamma, float* dbeta,
                   float* coef3c, float* partial, void* dy16, void* g_out16, int pre_rows,
                   void* stream) {
    CILRS_CHECK(gamma && stats && dgamma && dbeta && coef3c && partial, "bn16_bwd: NULL argument");
    return launch_bn16_bwd(dz16, z16, y16, M, C, gamma, stats, relu, dgamma, dbeta, coef3c, partial,
                           dy16, g_out16, pre_rows, reinterpret_cast<hipStream_t>(stream));
}

// Winograd F(2x2,3x3) forms of the two operators above (3x3 / stride 1 / pad 1): filter transform
// + fused convolution.  scratch: cilrs_conv2d_wino_scratch_floats(Cin, Cout) floats.
size_t cilrs_conv2d_wino_scratch_floats(int Cin, int Cout) { return wino_weight_floats(Cout, Cin); }

int cilrs_conv2d_wino_fwd(const float* x, const float* w, float* y, int N, int H, int W, int Cin,
                          int Cout, float* scratch, void* stream) {
    CILRS_CHECK(x && w && y && scratch, "conv2d_wino_fwd: NULL argument");
    CILRS_CHECK(wino_supported(Cin, Cout, 3, 1, 1), "conv2d_wino_fwd: Cin %% 8, Cout %% 64");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (launch_wino_weights(w, scratch, Cout, Cin, 0, s)) return 1;
    WinoArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.U = scratch; a.y = y; a.N = N; a.H = H; a.W = W; a.C = Cin; a.K = Cout;
    return launch_conv_wino(a, s);
}

int cilrs_conv2d_wino_fold_fwd(const float* x, const float* w, float* y, const float* scale,
                               const float* shift, const float* addend, int relu, int relu_post,
                               int N, int H, int W, int Cin, int Cout, float* scratch, void* stream) {
    CILRS_CHECK(x && w && y && scale && shift && scratch, "conv2d_wino_fold_fwd: NULL argument");
    CILRS_CHECK(wino_supported(Cin, Cout, 3, 1, 1), "conv2d_wino_fold_fwd: Cin %% 8, Cout %% 64");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (launch_wino_weights(w, scratch, Cout, Cin, 0, s)) return 1;
    WinoArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.U = scratch; a.y = y; a.addend = addend; a.N = N; a.H = H; a.W = W; a.C = Cin; a.K = Cout;
    const WinoFold f{scale, shift, relu, relu_post};
    return launch_conv_wino_fold(a, f, s);
}

size_t cilrs_conv2d_wino_wgrad_scratch_floats(int N, int H, int W, int Cin, int Cout) {
    return wino_wgrad_scratch_floats(N, H, W, Cin, Cout);
}
int cilrs_conv2d_wino_wgrad(const float* x, const float* dy, float* dw, int N, int H, int W, int Cin,
                            int Cout, float* scratch, size_t scratch_floats, void* stream) {
    CILRS_CHECK(x && dy && dw && scratch, "conv2d_wino_wgrad: NULL argument");
    CILRS_CHECK(wino_wgrad_supported(Cin, Cout, 3, 1, 1), "conv2d_wino_wgrad: Cin %% 64, Cout %% 64");
    CILRS_CHECK(scratch_floats >= wino_wgrad_scratch_floats(N, H, W, Cin, Cout),
                "conv2d_wino_wgrad: scratch too small");
    WinoWgradArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.dy = dy; a.dw = dw; a.slabs = scratch;
    a.N = N; a.H = H; a.W = W; a.C = Cin; a.K = Cout;
    return launch_conv_wino_wgrad(a, reinterpret_cast<hipStream_t>(stream));
}

static long long* g_wino_stamps = nullptr;
int cilrs_conv2d_wino_stamps(long long* stamps16) { g_wino_stamps = stamps16; return 0; }

int cilrs_wino_filter_transform(const float* w, float* U, int Cin, int Cout, int dgrad, void* stream) {
    CILRS_CHECK(w && U, "wino_filter_transform: NULL argument");
    return launch_wino_weights(w, U, Cout, Cin, dgrad, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_conv2d_wino_pre(const float* x, const float* U, float* y, const float* addend, int N, int H,
                          int W, int Cred, int Cout, void* stream) {
    CILRS_CHECK(x && U && y, "conv2d_wino_pre: NULL argument");
    WinoArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.U = U; a.y = y; a.addend = addend; a.N = N; a.H = H; a.W = W; a.C = Cred; a.K = Cout;
    a.stamps = g_wino_stamps;        // diagnostics: cilrs_conv2d_wino_stamps (tools/wino_bench.py)
    return launch_conv_wino(a, reinterpret_cast<hipStream_t>(stream));
}

int cilrs_conv2d_wino_split(const float* x, const float* U, float* y, const float* addend,
                            float* bn_partial, int N, int H, int W, int Cred, int Cout, float* slabs,
                            size_t slab_floats, int* csplit, int* partial_rows, void* stream) {
    CILRS_CHECK(x && U && y && bn_partial && slabs, "conv2d_wino_split: NULL argument");
    WinoArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.U = U; a.y = y; a.addend = addend; a.N = N; a.H = H; a.W = W; a.C = Cred; a.K = Cout;
    a.bn_partial = bn_partial; a.slabs = slabs; a.slab_floats = slab_floats;
    a.scratch_partial = bn_partial;
    if (partial_rows) *partial_rows = wino_rows(N, H, W, Cout, 0, Cred, slab_floats);
    const int rc = launch_conv_wino(a, reinterpret_cast<hipStream_t>(stream));
    if (csplit) *csplit = wino_last_csplit();
    return rc;
}

int cilrs_conv2d_wino_dgrad(const float* dy, const float* w, float* dx, const float* addend, int N,
                            int H, int W, int Cin, int Cout, float* scratch, void* stream) {
    CILRS_CHECK(dy && w && dx && scratch, "conv2d_wino_dgrad: NULL argument");
    CILRS_CHECK(wino_supported(Cout, Cin, 3, 1, 1), "conv2d_wino_dgrad: Cout %% 8, Cin %% 64");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (launch_wino_weights(w, scratch, Cout, Cin, 1, s)) return 1;
    WinoArgs a;
    memset(&a, 0, sizeof(a));
    a.x = dy; a.U = scratch; a.y = dx; a.addend = addend;
    a.N = N; a.H = H; a.W = W; a.C = Cout; a.K = Cin;
    return launch_conv_wino(a, s);
}

size_t cilrs_bn_partial_floats(int C) { return bn_partial_floats(C); }

int cilrs_bn_train_fwd(const float* y, int M, int C, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, int64_t* nbt, float momentum,
                       float eps, const float* residual, int relu, float* stats, float* partial,
                       float* z, void* stream) {
    return launch_bn_train_fwd(y, M, C, gamma, beta, running_mean, running_var,
                               reinterpret_cast<long long*>(nbt), momentum, eps, residual, relu,
                               stats, partial, z, 0, reinterpret_cast<hipStream_t>(stream));
}
int cilrs_bn_eval_fwd(const float* y, int M, int C, const float* gamma, const float* beta,
                      const float* running_mean, const float* running_var, float eps,
                      const float* residual, int relu, float* stats, float* z, void* stream) {
    return launch_bn_eval_fwd(y, M, C, gamma, beta, running_mean, running_var, eps, residual,
                              relu, stats, z, reinterpret_cast<hipStream_t>(stream));
}
int cilrs_bn_bwd(const float* dz, const float* z, const float* y, int M, int C,
                 const float* gamma, const float* stats, int relu, float* dgamma, float* dbeta,
                 float* coef3c, float* partial, float* dy, float* g_out, void* stream) {
    return launch_bn_bwd(dz, z, y, M, C, gamma, stats, relu, dgamma, dbeta, 0, coef3c, partial, dy,
                         g_out, 0, reinterpret_cast<hipStream_t>(stream));
}
int cilrs_bn_bwd_frozen(const float* dz, const float* z, int M, int C, const float* gamma,
                        const float* stats, int relu, float* dy, float* g_out, void* stream) {
    return launch_bn_bwd_frozen(dz, z, M, C, gamma, stats, relu, dy, g_out,
                                reinterpret_cast<hipStream_t>(stream));
}
int cilrs_bn_bwd_pool_frozen(const float* dpool, const uint8_t* argmax, const float* y, int N, int H,
                             int W, int C, const float* gamma, const float* stats, float* dy,
                             void* stream) {
    return launch_bn_bwd_pool_frozen(dpool, argmax, y, N, H, W, C, gamma, stats, dy,
                                     reinterpret_cast<hipStream_t>(stream));
}
int cilrs_saliency_map(const float* dimage, long sn, long sc, long sh, long sw, int B, int H, int W,
                       const float* chan_scale3, float* heat, uint8_t* heat_u8, float* peak,
                       void* stream) {
    return launch_saliency_map(dimage, sn, sc, sh, sw, B, H, W, chan_scale3, heat, heat_u8, peak,
                               reinterpret_cast<hipStream_t>(stream));
}
int cilrs_attr_samples(const uint8_t* frames_u8, const uint8_t* baseline_u8, int B, int H, int W,
                       int mode, int S, int s_begin, int s_count, float sigma255, uint64_t seed,
                       float* out, void* stream) {
    return launch_attr_samples(frames_u8, baseline_u8, B, H, W, mode, S, s_begin, s_count, sigma255,
                               seed, out, reinterpret_cast<hipStream_t>(stream));
}
int cilrs_attr_accumulate(const float* dimage, long sn, long sc, long sh, long sw, int B, int s_count,
                          int H, int W, int first, float* acc, void* stream) {
    return launch_attr_accumulate(dimage, sn, sc, sh, sw, B, s_count, H, W, first, acc,
                                  reinterpret_cast<hipStream_t>(stream));
}
int cilrs_attr_finalize(const float* acc, const uint8_t* frames_u8, const uint8_t* baseline_u8, int B,
                        int H, int W, int mode, int S, const float* chan_scale3, float* attr,
                        float* signed_map, float* total, void* stream) {
    return launch_attr_finalize(acc, frames_u8, baseline_u8, B, H, W, mode, S, chan_scale3, attr,
                                signed_map, total, reinterpret_cast<hipStream_t>(stream));
}
int cilrs_attr_finalize_threads(void) { return attr_finalize_threads(); }
int cilrs_maxpool_fwd(const float* x, float* out, uint8_t* argmax, int N, int H, int W, int C,
                      void* stream) {
    return launch_maxpool_fwd(x, out, argmax, N, H, W, C, reinterpret_cast<hipStream_t>(stream));
}
int cilrs_maxpool_bwd(const float* dout, const uint8_t* argmax, float* dx, int N, int H, int W,
                      int C, void* stream) {
    return launch_maxpool_bwd(dout, argmax, dx, N, H, W, C, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
