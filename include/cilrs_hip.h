/* C-ABI of libcilrs_hip.so -- the MI355X (gfx950) engine behind the CILRS operator boundary.
 *
 * The reference has no FFI: its boundary for this path is the torch.nn.Module `CILRS`
 * (model/autonomous_drive.py:361-399 == notebook/notebook.ipynb:440-477), its loss
 * (notebook/notebook.ipynb:504-527) and torch.optim.Adam + clip_grad_norm_
 * (notebook/notebook.ipynb:533-534, 553-555).  Each entry point below names the reference
 * interface it replaces.  The Python mirror of that nn.Module (cilrs_mi355.CILRS) binds these
 * symbols with ctypes -- see INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch-ROCm's allocator) and only
 *    borrowed for the call, except `out_*` scalars explicitly marked host;
 *  - `stream` is a hipStream_t; every function only ENQUEUES work and never synchronises
 *    (cilrs_net_profile_collect excepted);
 *  - return value 0 = ok; non-zero = error, text in cilrs_last_error() (thread-local);
 *  - activations are NHWC fp32, conv weights OHWI fp32 (torch channels_last memory), all
 *    arithmetic fp32 (exact-f32 MFMA), reductions deterministic.
 */
#ifndef CILRS_HIP_H
#define CILRS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cilrs_net cilrs_net;

int cilrs_version(void);
const char* cilrs_last_error(void);

/* ---- parameter / buffer arena layout (replaces nn.Module.parameters()/state_dict() order,
 *      autonomous_drive.py:497 strict key contract) ----------------------- */
/* number of parameter tensors (142), of BatchNorm layers (36) */
int cilrs_num_params(void);
int cilrs_num_bn(void);
/* floats in the parameter arena (each tensor 16-byte aligned; >= 22,421,453) and exact count */
size_t cilrs_param_arena_floats(void);
size_t cilrs_param_count(void);
/* tensor i: state_dict name, float offset into the arena, numel, logical torch shape (ndim<=4).
 * Conv weights are stored OHWI at that offset (logical OIHW shape reported). */
int cilrs_param_info(int i, char* name, int name_cap, size_t* offset, size_t* numel, int* ndim,
                     int* shape4);
/* BatchNorm j: module prefix ("visual_encoder.1", ...), channels, float offsets of running_mean /
 * running_var inside the BN buffer arena; num_batches_tracked lives at int64 index j */
int cilrs_bn_info(int j, char* prefix, int prefix_cap, int* channels, size_t* rm_offset,
                  size_t* rv_offset);
size_t cilrs_bn_arena_floats(void);

/* ---- architecture variants ----------------------------------------------------------------------
 * variant 0: the reference's network (ResNet-34 trunk, autonomous_drive.py:365-370) -- everything
 *            above describes it.
 * variant 1: BASELINE.json configs[3] "ResNet-50 backbone variant": torchvision-style Bottleneck
 *            stacks [3,4,6,3] (stride on the 3x3 convolution), 2048-d features into the same
 *            speed encoder / four branches / speed predictor (first Linear layers 2176 and 2048
 *            wide).  The reference has no such model: parity is against the build's own CPU
 *            restatement (oracle/resnet50_oracle.py).  Trains in fp32 (train-mode forward,
 *            backward, the same segments); the fp16 / bf16 trunks are inference-only.
 * Number of commands: the reference's constructor builds one control branch per command
 * (model/autonomous_drive.py:362, 380-381).  Wherever a `variant` is passed it is the architecture
 * CODE  trunk | num_commands << 8  (trunk 0 or 1 as above; num_commands 1..8; 0 in the upper bits
 * = the 4 every caller of the reference passes).  Parameter names, arena offsets and gradient
 * segments follow the code; the persistent single-frame kernel exists for 4 commands only. */
int cilrs_num_variants(void);
int cilrs_variant_num_params(int variant);
int cilrs_variant_num_bn(int variant);
size_t cilrs_variant_param_arena_floats(int variant);
size_t cilrs_variant_param_count(int variant);
size_t cilrs_variant_bn_arena_floats(int variant);
int cilrs_variant_feature_width(int variant);
int cilrs_variant_param_info(int variant, int i, char* name, int name_cap, size_t* offset,
                             size_t* numel, int* ndim, int* shape4);
int cilrs_variant_bn_info(int variant, int j, char* prefix, int prefix_cap, int* channels,
                          size_t* rm_offset, size_t* rv_offset);

/* ---- network plan ----------------------------------------------------------------------------- */
typedef struct {
    float* params;          /* parameter arena                               */
    float* grads;           /* gradient arena, same layout (may be NULL for inference) */
    float* bn_running;      /* BN running_mean / running_var arena            */
    int64_t* bn_nbt;        /* [36] num_batches_tracked                       */
    void* workspace;        /* cilrs_net_workspace_bytes() bytes              */
} cilrs_buffers;

/* plan for a fixed batch / frame size (reference: B x 3 x 88 x 200); height and width at least 17
 * (smaller frames would leave a stride-2 step a one-pixel map to halve) */
int cilrs_net_create(int batch, int height, int width, cilrs_net** out);
int cilrs_net_create_variant(int variant, int batch, int height, int width, cilrs_net** out);
/* The same with plan options.  CILRS_PLAN_BF16_TRAIN: "bf16 MFMA path" training (BASELINE.json
 * configs[3]) -- in train mode the trunk convolutions after the stem (forward, data gradient,
 * weight gradient) multiply bf16-rounded activations / weights / output gradients on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation; BatchNorm, residual adds, the stem, the heads,
 * the loss, Adam and the master weights stay fp32.  Not the reference's arithmetic (it trains in
 * fp32): outputs and gradients agree with the fp32 path to bf16 rounding (~1e-2), not to 1e-4.
 * Eval-mode entry points are unaffected.  The workspace grows by the 16-bit shadow tensors. */
#define CILRS_PLAN_BF16_TRAIN 1u
int cilrs_net_create_ex(int variant, int batch, int height, int width, unsigned flags,
                        cilrs_net** out);
void cilrs_net_destroy(cilrs_net* net);
size_t cilrs_net_workspace_bytes(const cilrs_net* net);

/* CILRS.forward(image, speed, command) -> (controls[B,3], pred_speed[B])
 * (autonomous_drive.py:389-399).  image: f32 logical NCHW [B,3,H,W] with element strides
 * (sn,sc,sh,sw); speed f32 [B]; command int64 [B] in {0..3}.
 * train != 0: BatchNorm uses batch statistics and updates running stats (model.train());
 * train == 0: running statistics (model.eval()).  dropout_p applies only when train != 0. */
int cilrs_net_forward(cilrs_net* net, const cilrs_buffers* bufs, const float* image, long sn,
                      long sc, long sh, long sw, const float* speed, const int64_t* command,
                      int train, float dropout_p, uint64_t seed, float* controls,
                      float* pred_speed, void* stream);

/* model.eval() forward that keeps its graph -- torch.autograd through the reference's module in
 * eval mode (frozen BatchNorm): the same outputs as cilrs_net_forward(train = 0), computed by the
 * train-mode launch sequence so that every activation cilrs_net_backward and
 * cilrs_net_input_grads read is kept.  Every BatchNorm uses the running statistics; the running
 * buffers and num_batches_tracked are not touched; no dropout.  cilrs_net_backward after it is
 * the backward of that graph (BatchNorm with fixed statistics: d input = gamma * rstd * g).
 * fp32 plans of every variant; a CILRS_PLAN_BF16_TRAIN plan rejects it. */
int cilrs_net_forward_frozen(cilrs_net* net, const cilrs_buffers* bufs, const float* image, long sn,
                             long sc, long sh, long sw, const float* speed, const int64_t* command,
                             float* controls, float* pred_speed, void* stream);

/* BatchNorm re-estimation ("update_bn" of averaged weights; AdaBN, the label-free domain adaptation:
 * every BatchNorm's statistics re-estimated on frames of the target domain).
 *
 * The table (doubles, on the device, zeroed by the caller before the first batch):
 *   cilrs_variant_bn_stats_doubles(variant) entries -- for layer j of cilrs_variant_bn_info, at
 *   head_offset {t, sum_b M_b} (batches and rows seen), and at sums_offset four rows of C_j:
 *     [0] sum_b mean_b   [1] sum_b var_b * M_b / (M_b - 1)   [2] sum_b M_b * mean_b
 *     [3] sum_b M_b * (var_b + mean_b^2)
 *   with mean_b / var_b the batch mean and biased variance the train-mode BatchNorm normalises
 *   with, taken in double where it forms them.  Each chain is continued by one thread, one batch
 *   after the other, every term rounded on its own: no atomics, the table is a function of the
 *   batches and their order alone, and tables of disjoint batch sets add entry by entry (data
 *   parallel ranks all-reduce them).
 *
 * cilrs_net_forward_bn_stats: the train-mode trunk of cilrs_net_forward(train = 1) on batch
 *   statistics -- the same convolution, BatchNorm and max-pool launches in the same order, hence bit
 *   for bit the same per-layer statistics and activations -- adding each layer's batch to `table`.
 *   No heads, no dropout, no loss; bn_running, bn_nbt and the parameters are not written; no host
 *   synchronisation.  Afterwards the plan counts as "train-mode forward last" (the tick-following
 *   entries refuse as after a train step) and holds no graph (cilrs_net_backward refuses).  fp32
 *   plans of every variant.  Refused, nothing launched: a CILRS_PLAN_BF16_TRAIN plan; a NULL or
 *   misaligned table; a plan in which some BatchNorm sees fewer than 2 values per channel (torch
 *   raises "Expected more than 1 value per channel when training"; an unbiased variance does not
 *   exist).
 * cilrs_bn_stats_finalize: ONE launch writes every layer's running_mean / running_var into
 *   bn_running and t into bn_nbt, each value rounded once from double.
 *     estimator 0 ("batch_mean"): running_mean = sum mean_b / t, running_var = sum unbiased var_b / t
 *       -- what torch leaves after reset_running_stats(), momentum = None and the same train-mode
 *       forwards (the cumulative moving average).
 *     estimator 1 ("pooled"): with N = sum M_b, mean = sum M_b mean_b / N,
 *       var = (sum M_b (var_b + mean_b^2) / N - mean^2) * N / (N - 1): the moments of all rows seen;
 *       a short last batch weighs by its rows, and for the stem's BatchNorm the result does not
 *       depend on how the frames were batched.
 *   Reads the {t, sum M} heads back first (synchronises `stream`; not capturable): a layer with
 *   t == 0 is refused, like NULL / misaligned tensors and an unknown estimator, with nothing launched.
 * cilrs_bn_train_stats: the op-level twin -- the stand-alone column reduce of y[M][C] (about its
 *   pivot row, as cilrs_bn_train_fwd) plus the accumulating finalise, nothing else; acc = {t, sum M}
 *   followed by the four rows of C (2 + 4 C doubles), partial: cilrs_bn_partial_floats(C) floats.
 *   M >= 2. */
size_t cilrs_variant_bn_stats_doubles(int variant);
int cilrs_variant_bn_stats_info(int variant, int j, int* channels, size_t* head_offset,
                                size_t* sums_offset);
/* where convolution `conv`'s BatchNorm keeps mean | rstd | scale | shift (4 C floats) in the
 * workspace, in floats; the rows M it sees in this plan; its layer number j */
int cilrs_net_bn_layer_info(const cilrs_net* net, int conv, size_t* stats_offset, int* channels,
                            int* rows, int* bn_index);
int cilrs_net_forward_bn_stats(cilrs_net* net, const cilrs_buffers* bufs, const float* image,
                               long sn, long sc, long sh, long sw, double* table, void* stream);
int cilrs_bn_stats_finalize(int variant, const double* table, int estimator, float* bn_running,
                            int64_t* bn_nbt, void* stream);
int cilrs_bn_train_stats(const float* y, int M, int C, double* acc, float* partial, void* stream);

/* Fine-tuning on top of a pretrained trunk -- the reference's own first remedy for its failure on
 * the campus map: "collect a small CUSAT-specific dataset and fine-tune the checkpoint" (reference
 * README.md, "Why Results Degraded on CUSAT Map"; configs/train_config.json has a `pretrained`
 * key).  The train-mode forward (dropout, batch statistics) of cilrs_net_forward with a frozen
 * prefix of the trunk, counted in groups: 1 = stem, 2 = + layer1, ... 5 = the whole trunk.
 *   grad_frozen_groups (g): the parameters of these groups take no gradient.  cilrs_net_backward
 *     after this forward stops there: segments of frozen groups are not run (a wider segment range
 *     is clamped), the first block of the last trainable group launches only its weight gradients
 *     and the BatchNorm backward of its own layers, and the gradient-arena ranges of the frozen
 *     groups are not written.  cilrs_net_backward_step and the image gradient of
 *     cilrs_net_input_grads refuse such a graph.
 *   bn_frozen_groups (e): these groups run in eval mode -- BatchNorm on the running statistics,
 *     folded with ReLU and the residual add into the convolution epilogues (3x3 / stride-1 layers
 *     that the train plan gives to the Winograd kernel take its folded-epilogue variant); only the
 *     post-activation tensors are written, the running statistics and num_batches_tracked of the
 *     prefix are not touched.  e == g, or e == 0 (requires_grad_(False) alone: torch still uses
 *     the batch statistics there and moves the running buffers, and so does the ordinary train
 *     forward this runs).  Every other pair is an error; so is any freeze on a
 *     CILRS_PLAN_BF16_TRAIN plan.
 *   prefix_key: the frozen prefix's weight-derived state (BatchNorm scale / shift, padded stem
 *     weights, Winograd filter images) is rebuilt only when this value, the cut or the buffers
 *     change; 0 = rebuild on every call.  The caller changes it whenever a parameter or BatchNorm
 *     buffer of the prefix may have changed, and after any other forward on this plan.
 * e == g == 0 is cilrs_net_forward(train = 1), launch for launch. */
int cilrs_net_forward_ft(cilrs_net* net, const cilrs_buffers* bufs, const float* image, long sn,
                         long sc, long sh, long sw, const float* speed, const int64_t* command,
                         int bn_frozen_groups, int grad_frozen_groups, uint64_t prefix_key,
                         float dropout_p, uint64_t seed, float* controls, float* pred_speed,
                         void* stream);
/* folded-epilogue Winograd launches of the last cilrs_net_forward_ft on this plan (= the eligible
 * convolutions of its eval-mode prefix; 0 for small batches, where the train plan has none) */
int cilrs_net_ft_wino_convs(cilrs_net* net);
/* the cut of the plan's last graph-keeping forward: (0, 0) after cilrs_net_forward with train != 0,
 * cilrs_net_forward_frozen* and cilrs_net_forward_bn_stats; an eval-mode forward leaves it as it is */
int cilrs_net_ft_cut(const cilrs_net* net, int* bn_frozen_groups, int* grad_frozen_groups);

/* Byte offset, inside the workspace, of the plan's int32[4] status words.  The library zeroes them
 * ONCE per workspace (the first entry point that sees a workspace pointer); after that the kernels
 * only ever SET them, so a word means "since the caller last cleared it" (sticky): read them after
 * synchronising the stream(s) the forwards ran on, and clear them with a 16-byte memset ordered
 * after those forwards.  Word 0 becomes 1 when a `command` value lies outside {0..num_commands-1}
 * -- the case in which the reference's torch.gather (autonomous_drive.py:397-398) raises; the
 * kernels then use branch 0 so nothing faults.  Word 1: a grid barrier of the persistent
 * single-frame launch gave up (outputs are NaN).  The host mirror reads the words at its next
 * synchronisation (Predictor: with the outputs; Trainer.losses() / validate()) and raises like
 * torch does. */
size_t cilrs_net_status_offset(const cilrs_net* net);

/* Inference between weight updates (the control loop, autonomous_drive.py:908-920, calls forward
 * once per simulator tick on weights loaded once, :496-498): a promise by the caller that the
 * parameter arena and the BatchNorm buffers are unchanged for as long as `key` keeps its value.
 * The plan then keeps what it derives from them -- every layer's eval-mode BatchNorm scale/shift,
 * the channel-padded stem weights, the 16-bit folded weights -- instead of recomputing it on
 * every eval forward (two to three launches per frame).  key 0 (the default) = no promise.
 * The Python mirror derives the key from the arenas' torch version counters plus a counter it
 * bumps on every train-mode forward and optimiser step. */
int cilrs_net_set_weights_key(cilrs_net* net, uint64_t key);

/* Where a train-mode forward left the tensors backward re-reads, as float offsets into the
 * workspace (NHWC, dense): convolution `conv` (parameter order: 0 stem, then every block's conv1,
 * conv2[, conv3][, downsample]) -- y = its raw output (input of its BatchNorm), z = after BatchNorm
 * (+ residual) (+ ReLU); conv -1: the max-pool output.  The stem's z is not materialised in train
 * mode (BatchNorm + ReLU are fused into the max-pool).  Test / diagnostics aid: the parity tests
 * count the ReLU decisions on which the engine and the oracle differ. */
int cilrs_net_activation_info(const cilrs_net* net, int conv, size_t* y_offset, size_t* z_offset,
                              size_t* numel, int* channels);
/* The other decisions a graph-keeping forward (cilrs_net_forward with train != 0, _frozen, or _ft
 * with no eval-mode prefix) left for the backward pass -- test aids like the one above: offsets,
 * no launch, no state.  The mask-matched gradient tests hand them to the float64 oracle.
 * cilrs_net_pool_argmax_info: BYTE offset and element count of the stem max-pool's argmax, uint8
 * [B][Ho][Wo][64], value kh * 3 + kw of the window tap (input row 2 * oh - 1 + kh, column
 * 2 * ow - 1 + kw) the window kept (the first of equal values, kh-major).  A forward with an
 * eval-mode prefix (bn_frozen_groups > 0) does not write it.
 * cilrs_net_head_activation_info: float offset, rows (= batch), columns and row pitch of a head
 * activation the backward re-reads (post-ReLU, and post-dropout where a Dropout follows).  which:
 * 0 s1 (speed_encoder.1 output, 128 wide); 1 the speed-feature columns of `combined`
 * (speed_encoder.4 output, 128 wide, pitch features + 128); 2 p1, 3 p2 (speed_predictor.1 / .4);
 * 4 h1[branch], 5 h2[branch] (control_branches.<branch>.1 / .4; branch < num_commands, ignored
 * for which < 4). */
int cilrs_net_pool_argmax_info(const cilrs_net* net, size_t* byte_offset, size_t* numel);
int cilrs_net_head_activation_info(const cilrs_net* net, int which, int branch, size_t* offset,
                                   int* rows, int* cols, int* ld);

/* Where a 16-bit eval forward (cilrs_net_forward_u8_f16 / _bf16) keeps what its kernels read and
 * write, as BYTE offsets into the workspace -- test aid: the layer-by-layer tests of the 16-bit
 * inference mode read exactly what the engine's kernels read and wrote.
 * cilrs_net_infer16_conv_info: convolution `conv` (numbered as in cilrs_net_activation_info) --
 * its folded 16-bit weights (OHWI [Cout][K][K][Cin]; the stem, conv 0: [64][7][8][4] with the
 * filter row padded 7 -> 8 and the channels 3 -> 4 by zeros), w16_numel 16-bit elements, and its
 * fp32 bias [channels].  *folded_half: 1 / 2 when the arenas hold the fp16 / bf16 fold of the
 * current weights, 0 before the first 16-bit forward (or after the weights changed).
 * cilrs_net_infer16_io_info: the channel-padded fp32 image x4 [B][H][W][4] the u8 entries wrote
 * (x4_numel floats) and the pooled features `combined` [B][combined_ld], features first. */
int cilrs_net_infer16_conv_info(const cilrs_net* net, int conv, size_t* w16_offset,
                                size_t* bias_offset, size_t* w16_numel, int* channels,
                                int* folded_half);
int cilrs_net_infer16_io_info(const cilrs_net* net, size_t* x4_offset, size_t* x4_numel,
                              size_t* combined_offset, int* combined_ld, int* features);

/* nn.Dropout(p) in training mode exactly as the fused heads apply it (inverted dropout, keep
 * where hash(seed, site, row * cols + col) >= p, kept values divided by 1 - p), in place over
 * a [rows][cols] matrix with row pitch ld.  `site` names the Dropout module:
 *   0 speed_encoder.2;  1 + 2k control_branches.k.2;  2 + 2k control_branches.k.5  (k = 0..3);
 *   9 speed_predictor.2      (autonomous_drive.py:371-387).
 * Applied to a matrix of ones it returns the mask (times 1/(1-p)) a train-mode forward with the
 * same seed used: the parity tests feed that mask to the oracle functionally. */
int cilrs_dropout(float* a, int rows, int cols, int ld, float p, uint64_t seed, int site,
                  void* stream);

/* ---- Monte-Carlo dropout through the heads (csrc/mc_heads.hip) ---------------------------------
 * The executed configuration trains with a Dropout after speed_encoder.1, control_branches.k.1,
 * control_branches.k.4 and speed_predictor.1 (autonomous_drive.py:371-387); every Dropout sits in
 * the heads, so in eval mode the trunk is deterministic.  MC dropout keeps BatchNorm in eval mode,
 * draws S dropout masks and reports the mean and spread of the S outputs: the trunk runs once, only
 * the heads run S times.  The reference has no such path; parity is pinned by this definition
 * (restated in float64 by tests/_mc_dropout.py):
 *   Inputs   per frame: pooled features v (fp32, F = 512 / 2048 for the ResNet-34 / ResNet-50
 *            trunk), normalised speed x, command k, architecture code trunk | num_commands << 8
 *            (NC commands).  Call parameters: S samples, dropout probability p in [0, 1), a 64-bit
 *            seed.
 *   Row      sample s of frame b is row r = b * S + s.
 *   Mask     keep(site, r, c, cols) = u >= p, u the fp32 in [0, 1) from the top 24 bits of the hash
 *            of seed * 0x2545F4914F6CDD1D + (site << 40) + (r * cols + c), exactly as cilrs_dropout
 *            computes it.  A kept value is value / (1.0f - p) (an fp32 division), a dropped one 0.
 *   Sites    0: speed_encoder.2 (128 columns); 1 + 2k and 2 + 2k: control_branches.k.2 and .5 (256
 *            columns each); 2 NC + 1: speed_predictor.2 (256 columns; 9 for the reference).
 *   Per row  s1 = drop_0(relu(W_se0 x + b));  f = relu(W_se3 s1 + b);
 *            h1 = drop_{1+2k}(relu(W_k0 [v | f] + b));  h2 = drop_{2+2k}(relu(W_k3 h1 + b));
 *            controls = W_k5 h2 + b;
 *            p1 = drop_{2NC+1}(relu(W_p0 v + b));  p2 = relu(W_p3 p1 + b);  pred_speed = W_p5 p2 + b.
 *   Branch   only the commanded branch is evaluated; a command outside 0..NC-1 uses branch 0 and
 *            sets the status word, as everywhere else in the library.
 *   Stats    per frame and output, over its S stored fp32 sample values: mean = (sum x_s) / S,
 *            std = sqrt(sum (x_s - mean)^2 / (S - 1)) (torch's default unbiased estimate; 0 for
 *            S = 1); both passes in double in sample order, the results rounded once to fp32.
 *   p = 0    every sample is the eval-mode output and std is exactly 0 (the double sum of
 *            S <= 4,096 equal fp32 values is exact).
 * A sample's four values depend only on (seed, r, inputs), not on how many samples the call asks
 * for.  At most three launches, no atomics, every sum in a fixed order.
 *
 * mean, std: [B][4] = steer, throttle, brake, pred_speed; samples_out: [B][S][4] or NULL; all three
 * may be pinned host memory.  status: a device int (set to 1 on an out-of-range command) or NULL.
 * scratch: caller's device memory of cilrs_heads_mc_scratch_floats(variant, batch, samples) floats
 * (0 for an unknown code or a non-positive size).
 * cilrs_heads_mc: the op-level form on caller-supplied pooled features [B][pooled_ld], features
 * first; `variant` is the architecture code (both trunks, 1..8 commands).
 * cilrs_net_heads_mc: the same on the features of the plan's last eval-mode forward -- `combined`
 * after cilrs_net_forward(train = 0), _frozen*, _u8, _camera, the _graph forms and the 16-bit forms;
 * after a persistent single-frame forward, which pools inside its head stage and keeps no pooled
 * copy, the average pool of the last feature map it stored.  Batch = the plan's; status = the
 * plan's word 0.  No launch of any forward entry changes, nor does the workspace layout.
 * Refused (non-zero, text in cilrs_last_error, nothing launched): NULL tensors; samples < 1 or
 * > 4096; batch * samples > 65536; p outside [0, 1) or not finite; a scratch smaller than asked; an
 * unknown architecture code; at plan level no forward yet, or a train-mode forward last. */
size_t cilrs_heads_mc_scratch_floats(int variant, int batch, int samples);
int cilrs_heads_mc(int variant, const float* params, const float* pooled, int pooled_ld,
                   const float* speed, const int64_t* command, int batch, int samples, float p,
                   uint64_t seed, float* mean, float* std, float* samples_out,
                   float* scratch, size_t scratch_floats, int* status, void* stream);
int cilrs_net_heads_mc(cilrs_net* net, const cilrs_buffers* bufs, const float* speed,
                       const int64_t* command, int samples, float p, uint64_t seed,
                       float* mean, float* std, float* samples_out,
                       float* scratch, size_t scratch_floats, void* stream);

/* ---- Grad-CAM: class-activation maps of a trunk group (csrc/gradcam.hip) -----------------------
 * Which region of the feature map carried an output.  The reference has no such path (its
 * DashboardHUD, autonomous_drive.py:178-355, draws the outputs only); parity is pinned by this
 * definition (restated in float64 by tests/_gradcam.py).  Per frame:
 *   y        = w . (steer, throttle, brake, pred_speed) on the raw eval-mode outputs (no dropout,
 *            the commanded branch only; pred_speed not multiplied by 90), w four finite weights.
 *            A command outside 0..NC-1 uses branch 0 and sets status word 0, as everywhere else.
 *   A        the post-ReLU output of trunk group L (layer1..layer4), NHWC [h][w][C]; at 88x200
 *            layer4 is 3x7x512.
 *   dA       dy / dA.  For layer4, where AdaptiveAvgPool2d sits directly on A
 *            (autonomous_drive.py:365-370), dA[c,i,j] = g[c] / (h*w) with g = dy / d pooled, which
 *            the heads give alone: dh2 = relu'(h2) W_k5^T w[0..2], dh1 = relu'(h1) W_k3^T dh2, the
 *            first F columns of W_k0^T dh1; dp2 = relu'(p2) W_p5^T w[3], dp1 = relu'(p1) W_p3^T dp2,
 *            W_p0^T dp1; g = branch part + speed-predictor part, added in that order (names as in
 *            the Monte-Carlo section above, k the commanded branch; relu'(x) = 1 where x > 0).
 *   alpha[c] = (1/(h*w)) sum_ij dA[c,i,j]          (given g: g[c] / (h*w), one fp32 division)
 *   cam[i,j] = sum_c alpha[c] A[c,i,j]             signed, returned as it is
 *   peak     = max_ij max(cam, 0)
 *   n        = max(cam, 0) / peak, and 0 everywhere when peak == 0 (never NaN)
 *   heat[y,x] float32 [H][W]: the bilinear interpolation of n at the network resolution with
 *            half-pixel centres -- source coordinate (y + 0.5) * h / H - 0.5 clamped to [0, h-1], the
 *            upper neighbour clamped to h-1, likewise in x: F.interpolate(mode="bilinear",
 *            align_corners=False).  Coordinates and blend in double, rounded to fp32 once.
 *   heat_u8  = floor(heat * 255 + 0.5) in fp32; optional.
 * Every sum runs in a fixed order without atomics: results are bit-identical from run to run and a
 * frame's result does not depend on the batch it sits in.
 *
 * cilrs_heads_input_grad: the eval-mode heads forward and backward to g [B][F] (F = 512 / 2048), one
 * launch.  Features: exactly one of `pooled` ([B][pooled_ld], features first) and `featmap` (an
 * fp32 map [B][hw][F], which the kernel pools in cell order).  out4 [B][4]: the raw outputs, or
 * NULL.  weights4: HOST memory.  `variant`: the architecture code trunk | num_commands << 8, both
 * trunks, 1..8 commands.  status: a device int (set to 1 on an out-of-range command) or NULL.
 * cilrs_gradcam_map: alpha, cam [B][h][w], peak [B], heat [B][H][W] and optionally heat_u8 from
 * A [B][h][w][C] and exactly one of dA (same shape) and g [B][C]; one launch, one workgroup per
 * frame.  C in {64, 128, 256, 512, 1024, 2048}; h * w <= 4096.
 * cilrs_net_gradcam: the map of trunk group `layer` (1..4) on what the plan's last forward left.
 *   layer 4  after any fp32 eval-mode forward -- cilrs_net_forward(train = 0), _frozen*, _u8, _camera,
 *            _u8_graph, the persistent single-frame forms: A is the stored last feature map, g comes
 *            from cilrs_heads_input_grad on the plan's pooled features (after a persistent launch:
 *            on the stored map); two launches, no backward pass needed.
 *   any other layer  after cilrs_net_forward_frozen* followed by cilrs_net_backward[_data] calls
 *            that began at segment 0 and ended exactly at segment 5 - layer: dA is the gradient the
 *            chain left at that group's boundary; y is then whatever dcontrols / dpred_speed that
 *            backward was given, and weights4 is only checked.  One launch.
 *   cam [B][h][w] (h, w, C: cilrs_net_gradcam_info), heat [B][H][W] and heat_u8 at the plan's frame
 *   size, peak [B]; heat_u8 may be NULL; outputs may be pinned host memory.  scratch: caller's device
 *   memory of cilrs_gradcam_scratch_floats(variant, batch) floats (0 for an unknown code or a
 *   non-positive batch); after a layer-4 call it holds g [B][F] followed by the raw outputs [B][4].
 *   No launch of any other entry changes, nor does the workspace layout.
 * cilrs_net_gradcam_info: workspace offsets (in floats) of A and of the boundary gradient, and the
 * map's shape, for trunk group `layer`.
 * Refused (non-zero, text in cilrs_last_error, nothing launched): NULL tensors; non-positive sizes;
 * an unknown architecture code; both or neither of pooled / featmap, of dA / g; non-finite weights;
 * a channel count or a cell count outside the above; a scratch smaller than asked; at plan level a
 * layer outside 1..4, no forward yet, a train-mode forward last, a fine-tuning step (frozen prefix)
 * last, a 16-bit (fp16 / bf16) forward last (its maps are 16-bit), a CILRS_PLAN_BF16_TRAIN plan, and
 * layers 1..3 without a matching backward (none, another forward since, or another end segment). */
int cilrs_heads_input_grad(int variant, const float* params, const float* pooled, int pooled_ld,
                           const float* featmap, int hw, const float* speed, const int64_t* command,
                           const float* weights4, int batch, float* g, float* out4, int* status,
                           void* stream);
int cilrs_gradcam_map(const float* A, const float* dA, const float* g, int batch, int h, int w,
                      int channels, int H, int W, float* cam, float* peak, float* heat,
                      uint8_t* heat_u8, void* stream);
size_t cilrs_gradcam_scratch_floats(int variant, int batch);
int cilrs_net_gradcam_info(const cilrs_net* net, int layer, size_t* a_offset, size_t* da_offset,
                           int* h, int* w, int* channels);
int cilrs_net_gradcam(cilrs_net* net, const cilrs_buffers* bufs, const float* speed,
                      const int64_t* command, const float* weights4, int layer, float* cam,
                      float* heat, uint8_t* heat_u8, float* peak, float* scratch,
                      size_t scratch_floats, void* stream);

/* ---- Feature-space novelty: Mahalanobis distance of the pooled features (csrc/novelty.hip) ------
 * Monte-Carlo dropout measures how much the heads disagree about a feature vector; it cannot see
 * that the vector itself is unlike anything the trunk produced during training.  This score can:
 * the squared Mahalanobis distance of the eval-mode pooled features to command-conditional
 * Gaussians with one tied covariance (Lee et al., 2018), the classes being the navigation commands.
 * The reference has no such path; parity is pinned by this definition (restated in float64 by
 * tests/_novelty.py).
 *   Inputs   of a fit: N frames, each with v (fp32 pooled features, F = 512 / 2048: the first F
 *            columns of a row, or the cell-order average s / (float)hw of an fp32 map [hw][F],
 *            s += map[p][c] for p = 0..hw-1) and a command k in 0..NC-1, NC <= 8.  A command outside
 *            that range counts as command 0 and sets the status word, as everywhere else.
 *   Pivot    c: a fixed fp32 vector [F] chosen once per fit.  All moments are taken of
 *            x = (double)v - (double)c; the result is algebraically independent of c, which only
 *            keeps G - sum n mu mu^T from cancelling.
 *   Table    float64, cilrs_feature_moments_doubles(F, NC) = NC + NC F + F F values:
 *            n[NC] | s[NC][F] | G[F][F].  n_k counts the rows of command k, s_k sums their x,
 *            G[i][j] = sum_n x_ni x_nj for j <= i, tied over all commands; entries j > i are never
 *            read or written.  Every entry is ONE sequential chain over the rows in row order that
 *            continues from the value already in the table: t = table; per row t = fma(x_bi, x_bj, t)
 *            (s: t = t + x_bi for the rows of command k; n: t = t + 1); table = t.  Updates of 2 + 3
 *            rows are therefore bit for bit one update of 5.  The caller zeroes the table before
 *            the first update.  No atomics.
 *   Finalise (host, float64): mu_k = c + s_k / n_k for the K' commands that occurred;
 *            S_w = G - sum_k n_k (s_k/n_k)(s_k/n_k)^T;  Sigma = S_w / (N - K');
 *            Sigma_l = (1 - l) Sigma + l (tr Sigma / F) I  (shrinkage l > 0 makes it positive
 *            definite whatever dead channels the post-ReLU features have, and for N < F);
 *            Sigma_l = L L^T (Cholesky), W = L^-1 lower triangular; W [F][F] and mean [NC][F] are
 *            rounded once to fp32.
 *   Score    per frame b: u = v - mean[k] in fp32; y_i = sum_{j <= i} W_ij u_j; d2 = sum_i y_i^2,
 *            all in fp32.  Columns j > i of W are never read.  Order of the sums: lane l of a wave
 *            runs a = fmaf(W_ij, u_j, a) from a = 0 over its columns j = 256 q + 4 l + e <= i
 *            (q ascending, then e = 0..3); the 64 lane sums are combined by the xor butterfly
 *            a += shfl_xor(a, o), o = 32, 16, .., 1.  Workgroup g of F / 8 owns rows g + (F / 8) r,
 *            r = 0..7; wave w gives q_w = fmaf(y', y', y y) for rows r = 2w (y) and 2w + 1 (y'); the
 *            workgroup's part is ((q_0 + q_1) + q_2) + q_3; d2 adds the parts from 0 in workgroup
 *            order.  No atomics: results are bit-identical from run to run and a frame's score
 *            does not depend on the batch it sits in.
 * cilrs_feature_moments: one launch; adds `batch` rows into `table`.  Features: exactly one of
 * `features` ([batch][ld], features first) and `featmap` ([batch][hw][F]).
 * cilrs_feature_novelty: three launches (u into the scratch; the triangular product with the rows
 * of W split over F / 8 workgroups; the per-frame sum).  d2 [batch] may be pinned host memory.
 * scratch: caller's device memory of cilrs_feature_novelty_scratch_floats(F, batch) floats (0 for a
 * width other than 512 / 2048 or a batch outside 1..65536), 16-byte aligned like W.
 * status: a device int (set to 1 on an out-of-range command) or NULL.
 * cilrs_net_feature_moments / cilrs_net_novelty: the same on the features the plan's last
 * eval-mode forward left, resolved exactly as cilrs_net_heads_mc resolves them (`combined`, or after
 * a persistent single-frame forward the stored last feature map); F, NC and the batch are the
 * plan's, status its word 0.  16-bit forwards are accepted (`combined` is fp32 there).  No launch of
 * any forward entry changes, nor does the workspace layout.
 * Refused (non-zero, text in cilrs_last_error, nothing launched): NULL tensors; a batch outside
 * 1..65536; F outside {512, 2048}; NC outside 1..8; both or neither of features / featmap; ld < F;
 * hw outside 1..65536; a scratch smaller than asked; a W or scratch that is not 16-byte aligned;
 * at plan level no forward yet, or a train-mode forward last. */
size_t cilrs_feature_moments_doubles(int F, int NC);
int cilrs_feature_moments(const float* features, int ld, const float* featmap, int hw,
                          const int64_t* command, int batch, int F, int NC, const float* pivot,
                          double* table, int* status, void* stream);
size_t cilrs_feature_novelty_scratch_floats(int F, int batch);
int cilrs_feature_novelty(const float* features, int ld, const float* featmap, int hw,
                          const int64_t* command, int batch, int F, int NC, const float* mean,
                          const float* W, float* d2, float* scratch, size_t scratch_floats,
                          int* status, void* stream);
int cilrs_net_feature_moments(cilrs_net* net, const cilrs_buffers* bufs, const int64_t* command,
                              const float* pivot, double* table, void* stream);
int cilrs_net_novelty(cilrs_net* net, const cilrs_buffers* bufs, const int64_t* command,
                      const float* mean, const float* W, float* d2, float* scratch,
                      size_t scratch_floats, void* stream);

/* ---- Greedy k-center: which K frames of a pool to label (csrc/kcenter.hip) -----------------------
 * The novelty score says how far ONE frame is from the fit; the top-K novel frames of a 20 Hz log
 * are near-copies of each other.  The core-set rule (Sener & Savarese, 2018) is greedy k-center
 * (farthest-point selection): start from what is covered, then repeatedly take the row farthest from
 * everything chosen so far.  On rows whitened by the novelty score's W the squared Euclidean
 * distance below is that score's Mahalanobis distance.  The reference has no such path; parity is
 * pinned by this definition (restated in float64 by tests/_kcenter.py).
 *   Inputs   rows X fp32 [N][ld], the first D columns used (columns D.. are never read); mind, a
 *            running minimum-distance vector fp32 [N] that the caller owns and initialises (+inf:
 *            nothing covered yet).
 *   Distance d(x, c) = sum_j t_j^2, t_j = x_j - c_j, all in fp32: lane l of a wave runs
 *            a = fmaf(t_j, t_j, a) from a = 0 over its columns j = 256 q + 4 l + e < D (q ascending,
 *            then e = 0..3); the 64 lane sums are combined by a += shfl_xor(a, o), o = 32, 16, .., 1
 *            (the order of cilrs_feature_novelty).  Nothing else is fused.
 *   Cover    for m = 0..M-1 in order: mind[i] = min(mind[i], d(X_i, C_m)) for centres C fp32
 *            [M][ldc]; min(a, b) is b < a ? b : a, so a NaN distance never replaces a value.
 *   Greedy   for t = 0..K-1: i_t = the index of the largest mind[i], the lowest index among equal
 *            values -- an entry wins by v > best || (v == best && i < besti) starting from
 *            (mind[0], 0), so NaN entries never win; sel[t] = i_t, radius[t] = mind[i_t]; then
 *            mind[i] = min(mind[i], d(X_i, X_{i_t})) for every i, which makes mind[i_t] exactly 0.
 *            Max, min and the tie rule are exact: the result does not depend on how the rows are
 *            spread over workgroups, only the distance order fixes bits, and K1 picks followed by K2
 *            more on the same mind are bit for bit K1 + K2 picks.  Once radius[t] == 0 every row
 *            coincides with a chosen one; later picks are index 0 by the tie rule and carry no
 *            meaning.
 * cilrs_kcenter_cover: one launch (eight centres at a time in LDS: X is read once per eight).
 * cilrs_kcenter_greedy: K + 1 launches on `stream` -- one pass over mind, then one streaming pass
 * over X per pick; no atomics, no fences, no grid barrier, no host synchronisation.  sel int64 [K],
 * radius fp32 [K] and mind are device memory; scratch: cilrs_kcenter_scratch_bytes(N) bytes (0 for
 * an N outside its range), 16-byte aligned, contents irrelevant before and after.
 * Refused (non-zero, text in cilrs_last_error, nothing launched): NULL tensors; N outside 1..2^24;
 * D outside 4..2048 or not a multiple of 4; ld or ldc below D or not a multiple of 4; X, C or the
 * scratch not 16-byte aligned; M outside 0..65536 (M == 0 is a successful no-op); K outside 1..N;
 * a scratch smaller than asked. */
size_t cilrs_kcenter_scratch_bytes(int N);
int cilrs_kcenter_cover(const float* X, long ld, int N, int D, const float* C, long ldc, int M,
                        float* mind, void* stream);
int cilrs_kcenter_greedy(const float* X, long ld, int N, int D, float* mind, int K, int64_t* sel,
                         float* radius, void* scratch, size_t scratch_bytes, void* stream);

/* ---- Nearest neighbours: which rows of a pool a query looks like (csrc/knn.hip) -------------------
 * The novelty score gives one number and assumes Gaussians; the k nearest recorded frames answer
 * with examples, and the distance to the K-th of them is the non-parametric score of Sun et al.
 * (2022).  The reference has no such path; parity is pinned by this definition (restated in float64
 * by tests/_knn.py).
 *   Inputs   rows X fp32 [N][ld] and queries Y fp32 [Q][ldq], the first D columns used (columns D..
 *            are never read); skip int64 [Q] or NULL.
 *   Distance d(x, y) is exactly the distance of "Greedy k-center" above: the same lane chains and
 *            butterfly, the same bits (the device code is shared, csrc/kc_dist.h).
 *   Result   row i is a candidate for query q unless skip[q] == i or d(X_i, Y_q) is NaN; a skip
 *            value outside 0..N-1 excludes nothing (skip is the leave-one-out switch for queries
 *            that are pool rows themselves).  idx[q][0..K-1], dist[q][0..K-1] are the K candidates
 *            smallest in the total order (d, i), ascending: an entry precedes another by
 *            d < d' || (d == d' && i < i'); +inf is an ordinary value.  With fewer than K
 *            candidates the remaining slots hold idx = -1 and dist = +inf.
 *            Min, comparison and the tie rule are exact and every distance has fixed bits: the
 *            result does not depend on how the rows are spread over waves, workgroups or launches,
 *            a query's result does not depend on the queries it shares a call with, and the result
 *            for K is the first K columns of the result for any K' > K.
 * cilrs_knn: per chunk of at most eight queries two or three launches on `stream` -- one streaming
 * pass over X with the queries staged in LDS (X is read once per eight queries), then the fold of
 * the workgroups' lists (in two levels where a query's lists hold more than 2,048 pairs); no
 * atomics, no fences, no grid barrier, no host synchronisation.  idx int64
 * [Q][K] and dist fp32 [Q][K] may be pinned host memory; scratch: cilrs_knn_scratch_bytes(N, Q, K)
 * bytes of device memory (0 for arguments outside the ranges), 16-byte aligned, contents irrelevant
 * before and after.
 * Refused (non-zero, text in cilrs_last_error, nothing launched): NULL tensors (skip is exempt); N
 * outside 1..2^24; D outside 4..2048 or not a multiple of 4; ld or ldq below D or not a multiple of
 * 4; X, Y or the scratch not 16-byte aligned; Q outside 1..65536; K outside 1..64; a scratch
 * smaller than asked.
 *
 * cilrs_feature_whiten: y = tril(W) (v - origin) as fp32 [batch][F] for rows v [batch][ld] -- the
 * first two launches of cilrs_feature_novelty (u = v - origin in fp32; y_i = sum_{j <= i} W_ij u_j
 * in the order of "Score" above) with one fixed origin [F] instead of a per-row command mean, y
 * stored instead of summed.  A row's y does not depend on the batch or its place in it, so a query
 * whitened by this entry is at distance exactly 0 from its own row of a pool whitened by it.
 * scratch: cilrs_feature_whiten_scratch_floats(F, batch) floats (0 for a width other than 512 / 2048
 * or a batch outside 1..65536), 16-byte aligned like W.  Refused: NULL tensors; those widths and
 * batches; ld < F; a scratch smaller than asked; a W or scratch that is not 16-byte aligned.
 *
 * cilrs_net_knn: cilrs_knn of the features the plan's last eval-mode forward left (resolved exactly
 * as cilrs_net_novelty resolves them) against the rows X [N][ld] of an index, D = F and Q = the
 * plan's batch.  With origin and W (both or neither) the features are whitened first; X then holds
 * rows whitened by cilrs_feature_whiten with the same tables.  scratch:
 * cilrs_net_knn_scratch_bytes(F, batch, N, K) bytes.  Refuses what cilrs_knn and cilrs_net_novelty
 * refuse (no forward yet, a train-mode forward last).  No launch of any other entry changes, nor
 * does the workspace layout. */
size_t cilrs_knn_scratch_bytes(int N, int Q, int K);
int cilrs_knn(const float* X, long ld, int N, int D, const float* Y, long ldq, int Q,
              const int64_t* skip, int K, int64_t* idx, float* dist, void* scratch,
              size_t scratch_bytes, void* stream);
size_t cilrs_feature_whiten_scratch_floats(int F, int batch);
int cilrs_feature_whiten(const float* features, int ld, int batch, int F, const float* origin,
                         const float* W, float* y, float* scratch, size_t scratch_floats,
                         void* stream);
size_t cilrs_net_knn_scratch_bytes(int F, int batch, int N, int K);
int cilrs_net_knn(cilrs_net* net, const cilrs_buffers* bufs, const float* X, long ld, int N,
                  const float* origin, const float* W, int K, int64_t* idx, float* dist,
                  void* scratch, size_t scratch_bytes, void* stream);

/* ---- Bulk nearest neighbours: a whole drive against a pool on the matrix cores (csrc/knn_join.hip) --
 * cilrs_knn reads the pool once per eight queries; a recorded drive against the labelled set, or the
 * leave-one-out self-join of a pool, is hundreds of thousands of queries.  The GEMM form
 * |x|^2 + |y|^2 - 2 x.y has other bits than the distance above, so here it only SCREENS: it keeps a
 * few more rows per query than asked for, the shared distance re-scores those, and a derived error
 * bound certifies per query that no other row can belong to the result.  What a certified query gets
 * is bit for bit cilrs_knn's; the others are flagged and left to cilrs_knn.
 *   Inputs   X, Y, skip, candidates, the order (d, i) and the -1 / +inf fill are those of "Nearest
 *            neighbours"; K is 1..16 and K_s = cilrs_knn_join_candidates(K) = K + 8.
 *   Screen   nx_i, ny_q: the fp32 sum of squares of a row -- lane l of a wave runs a = fmaf(x_j, x_j, a)
 *            from a = 0 over its columns j = 256 t + 4 l + e < D (t ascending, then e = 0..3), the 64
 *            lane sums are combined by a += shfl_xor(a, o), o = 32, 16, .., 1.  p(q, i): the fp32 dot
 *            product on v_mfma_f32_32x32x2_f32, one fmaf chain from 0 over the columns in the order
 *            16 c + 8 u + e, 16 c + 8 u + 4 + e for c = 0.., u = 0, 1, e = 0..3 (columns past D are
 *            zeros made in LDS).  s(q, i) = fmaf(-2, p, nx_i).  Row i is screened out if
 *            i == skip[q] or s is NaN; the candidates of q are the K_s remaining rows smallest in
 *            (s, i), or all of them when they are fewer; sigma_q is the largest kept s.
 *   Re-score d(X_i, Y_q) of the candidates is the distance of "Greedy k-center" (csrc/kc_dist.h, the
 *            pool row first as in cilrs_knn: the same bits).  Candidates with a NaN d are dropped, the
 *            rest sorted by (d, i), the first K written.
 *   Certificate  in float64, per query.  q is certified if
 *            (a) every row other than skip[q] is a candidate (none fell to the K_s limit and none
 *                to a NaN s: the re-score then IS the definition), or
 *            (b) max_i nx_i, ny_q and sigma_q are finite, max_i nx_i + ny_q < 2^125, K results exist,
 *                dist[q][K-1] is finite and  dist[q][K-1] < (1 - b) (sigma_q + ny_q - E_q)  with
 *                b = (4 ceil(D / 256) + 9) 2^-24, the bound of one distance (tests/_kcenter.py), and
 *                E_q = c_D 2^-24 (max_i nx_i + ny_q), c_D = 2 D + 16.
 *            Why (b) is sound: with u = 2^-24, the chain of p makes at most D roundings on partial
 *            sums bounded by sum |x_j y_j| <= (nx + ny) / 2, so |2 p - 2 x.y| <= D u (nx + ny); nx_i
 *            and ny_q carry r_D = min(D, 4 ceil(D / 256) + 6) roundings each (a lane's fmas and the
 *            butterfly; below 16 columns the butterfly adds zeros), the final fma one on a value of
 *            at most 2 (nx + ny): in all (D + 2 r_D + 3) u (max nx + ny) to first order, and
 *            2 r_D + 3 <= D + 16 for every D (smallest margin 9 u, at D = 4), which covers the second-order terms.
 *            Hence every row outside the candidates has a true squared distance of at least
 *            sigma_q + ny_q - E_q, its fp32 distance is at least (1 - b) times that, and the strict
 *            inequality keeps it behind the K-th result even on a tie.  Below 2^125 no partial sum of
 *            p overflows, so with finite norms no s is NaN and only skip[q] was screened out.  c_D
 *            comes from the chain lengths, not from measurements.  A pool row or query with a NaN or
 *            an infinity, or a square that overflows, makes (b) false for the queries it touches (a
 *            pool row: for all of them).
 *   Output   certified: idx / dist rows as cilrs_knn writes them, uncertified[q] = 0.  Otherwise
 *            uncertified[q] = 1, idx = -2 and dist = NaN in all K slots.  n_uncertified[0] is the
 *            count.  Everything, flags included, is the same from run to run and does not depend on
 *            how rows and queries are spread over tiles, workgroups, slices or calls: p's chain is
 *            fixed, max / min / comparisons are exact, max_i nx_i belongs to the pool alone.
 * cilrs_knn_join: six launches on `stream` (norms of X, their max, norms of Y, the screen, merge +
 * re-score + certificate, the count); no atomics, no fences, no grid barrier, no host synchronisation.
 * idx, dist, uncertified int32 [Q] and n_uncertified int32 [1] are device memory.  scratch:
 * cilrs_knn_join_scratch_bytes(N, Q, D, K) bytes (0 outside the ranges) =
 * 4 N + 4 Q + 4 min(1024, ceil(N / 4)) + 16, each part rounded up to 16, + 16 Q S K_s for the lanes'
 * lists, S = the pool slices of the screen (1 from 65,536 queries on, so that Q S <= 2 * 65,536:
 * 25 MB at K = 16 and Q = 65,536 whatever N); 16-byte aligned, contents irrelevant before and after.
 * Refused (non-zero, text in cilrs_last_error, nothing launched or written): NULL tensors (skip is
 * exempt); N outside 1..2^24; D outside 4..2048 or not a multiple of 4; ld or ldq below D or not a
 * multiple of 4; X, Y or the scratch not 16-byte aligned; Q outside 1..65536; K outside 1..16; a
 * scratch smaller than asked. */
int cilrs_knn_join_candidates(int K);
size_t cilrs_knn_join_scratch_bytes(int N, int Q, int D, int K);
int cilrs_knn_join(const float* X, long ld, int N, int D, const float* Y, long ldq, int Q,
                   const int64_t* skip, int K, int64_t* idx, float* dist, int32_t* uncertified,
                   int32_t* n_uncertified, void* scratch, size_t scratch_bytes, void* stream);

/* ---- K-means: what a pool consists of, and how much of each kind (csrc/kmeans.hip) ----------------
 * Greedy k-center picks extremes and the neighbour query answers for one tick; neither says which
 * scenario modes a recorded drive holds.  Lloyd's iteration (1982) partitions the pool: centres, a
 * label and a distance per row, the rows per cluster.  The reference balances its sampler by command
 * only; it has no such path, and parity is pinned by this definition (restated in float64 by
 * tests/_kmeans.py).
 *   Inputs   rows X fp32 [N][ld] and centres C fp32 [K][ldc], the first D columns of both used
 *            (columns D.. are never read or written).
 *   Distance d(x, c) is exactly the distance of "Greedy k-center" above: the same lane chains and
 *            butterfly, the same bits (the device code is shared, csrc/kc_dist.h).
 *   Assign   label[i], dist[i]: the centre smallest in the total order (d, m), one entry preceding
 *            another by d < d' || (d == d' && m < m'); a centre whose distance is NaN is no
 *            candidate, +inf is an ordinary value; with no candidate label = -1 and dist = +inf.
 *            By construction bit for bit the nearest-neighbour entry above with X = C, Y = X_i and
 *            K = 1.  changed: the rows whose label differs from the value label[i] held before the
 *            call.  inertia: the float64 sum of dist[i] over the rows with label >= 0, in an order
 *            fixed by N alone (rows in blocks of 256 ceil(N / 2^19); thread t of 256 adds its rows
 *            t, t + 256, .. in turn, a halving tree joins the threads, thread t of 1,024 adds the
 *            blocks t, t + 1,024, .. and a halving tree joins those).  counts int64 [K]: the rows
 *            per label.
 *   Update   for every m with counts[m] > 0: C[m][j] = (float)(S / counts[m]), S the float64 sum of
 *            X[i][j] over the rows labelled m -- the rows in ascending i, cut into runs of
 *            256 ceil(N / 2^19), each run a sequential chain, the runs added in order --, the division
 *            in float64.  A cluster with no rows keeps its centre; rows whose label is outside
 *            0..K-1 (-1 among them) take no part.
 *   Lloyd    `iters` times (assign, update), then one closing assign: at exit label, dist and counts
 *            belong to the returned centres.  inertia float64 [iters + 1] and changed int64
 *            [iters + 1] hold one entry per assignment.  Once changed[t] == 0 every later iteration
 *            is a fixed point bit for bit, so running past convergence is harmless, and iters1
 *            followed by iters2 on the same label / C is iters1 + iters2.
 *            Min, comparison and the tie rule are exact, every distance has fixed bits and every
 *            float64 order is a function of N and the labels alone: the result is bit-identical
 *            from run to run and does not depend on how rows are spread over waves and workgroups.
 * Launches on `stream` and nothing else: per assignment four (the distances with up to 128 KiB of
 * centres staged in LDS, X read once per such chunk; the labels' histogram; its scan in two), per
 * update three more after those (a stable counting sort of the row indices by label, the float64
 * sums of the gathered rows, the centres).  No floating-point atomics (integer LDS atomics build the
 * histogram), no fences, no grid barrier, no host synchronisation.  label int32 [N], dist fp32 [N],
 * counts, inertia, changed and C are device memory; scratch: cilrs_kmeans_scratch_bytes(N, D, K)
 * bytes (0 for arguments outside the ranges), 16-byte aligned, contents irrelevant before and after.
 * Refused (non-zero, text in cilrs_last_error, nothing launched): NULL tensors; N outside 1..2^24;
 * D outside 4..2048 or not a multiple of 4; ld or ldc below D or not a multiple of 4; X, C or the
 * scratch not 16-byte aligned; K outside 1..min(N, 1024); iters outside 0..10,000; a scratch
 * smaller than asked. */
size_t cilrs_kmeans_scratch_bytes(int N, int D, int K);
int cilrs_kmeans_assign(const float* X, long ld, int N, int D, const float* C, long ldc, int K,
                        int32_t* label, float* dist, int64_t* counts, double* inertia,
                        int64_t* changed, void* scratch, size_t scratch_bytes, void* stream);
int cilrs_kmeans_update(const float* X, long ld, int N, int D, const int32_t* label, float* C,
                        long ldc, int K, int64_t* counts, void* scratch, size_t scratch_bytes,
                        void* stream);
int cilrs_kmeans_lloyd(const float* X, long ld, int N, int D, float* C, long ldc, int K, int iters,
                       int32_t* label, float* dist, int64_t* counts, double* inertia,
                       int64_t* changed, void* scratch, size_t scratch_bytes, void* stream);

/* Same, fed with uint8 RGB HWC frames [B,H,W,3]: fuses preprocess_image's /255, HWC->CHW and
 * Normalize(mean,std) (autonomous_drive.py:897-902; the cv2.resize is the caller's). */
int cilrs_net_forward_u8(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frames,
                         const float* speed, const int64_t* command, float* controls,
                         float* pred_speed, void* stream);

/* cilrs_net_forward_frozen (the eval-mode forward that keeps its graph) fed like
 * cilrs_net_forward_u8 / cilrs_net_forward_camera (below): the same preprocessing launch, then the
 * frozen forward.  fp32 plans only. */
int cilrs_net_forward_frozen_u8(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frames,
                                const float* speed, const int64_t* command, float* controls,
                                float* pred_speed, void* stream);
int cilrs_net_forward_frozen_camera(cilrs_net* net, const cilrs_buffers* bufs,
                                    const uint8_t* frames, int src_h, int src_w, int pixel_stride,
                                    long row_stride, long frame_stride, const float* speed,
                                    const int64_t* command, float* controls, float* pred_speed,
                                    void* stream);

/* Same, fed with raw camera frames of any size: fuses preprocess_image completely --
 * cv2.resize(frame, (W, H)) (8-bit INTER_LINEAR, restated; cv2 is absent from the build image so
 * this step is parity-unpinned), /255, HWC->CHW, Normalize (autonomous_drive.py:897-902).
 * frames: [B] images of src_h x src_w pixels, pixel_stride 3 or 4 bytes (the CARLA camera hands
 * over 600x800 BGRA and the agent keeps bytes 0..2 of each pixel, :868-872), row_stride and
 * frame_stride in bytes. */
int cilrs_net_forward_camera(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frames,
                             int src_h, int src_w, int pixel_stride, long row_stride,
                             long frame_stride, const float* speed, const int64_t* command,
                             float* controls, float* pred_speed, void* stream);

/* cilrs_net_forward_u8 with the BasicBlock trunk in fp16 (batched serving, BASELINE config 5):
 * BatchNorm folded into fp16 weights on every call, fp16 NHWC activations, fp16 MFMA with fp32
 * accumulation; the stem runs on the 16-bit pipe too, the heads stay fp32.  The mode is DEFINED by
 * oracle/infer16_emulation.py (one rounding per stored tensor); tests/test_infer16_gpu.py holds
 * every kernel to it layer by layer. */
int cilrs_net_forward_u8_f16(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frames,
                             const float* speed, const int64_t* command, float* controls,
                             float* pred_speed, void* stream);
/* ... replayed from a cached hipGraph (same rules as cilrs_net_forward_u8_graph; one cached graph
 * per plan, re-captured when the mode or a pointer changes). */
int cilrs_net_forward_u8_f16_graph(cilrs_net* net, const cilrs_buffers* bufs,
                                   const uint8_t* frames, const float* speed,
                                   const int64_t* command, float* controls, float* pred_speed,
                                   void* stream);

/* The same with the trunk in bf16 (v_mfma_f32_32x32x16_bf16, fp32 accumulation): the "bf16 MFMA
 * path" of BASELINE.json configs[3]; works for both variants.  Same definition
 * (oracle/infer16_emulation.py) with bf16's 8 significant bits in place of fp16's 11. */
int cilrs_net_forward_u8_bf16(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frames,
                              const float* speed, const int64_t* command, float* controls,
                              float* pred_speed, void* stream);
int cilrs_net_forward_u8_bf16_graph(cilrs_net* net, const cilrs_buffers* bufs,
                                    const uint8_t* frames, const float* speed,
                                    const int64_t* command, float* controls, float* pred_speed,
                                    void* stream);

/* cilrs_net_forward_u8 replayed from a cached hipGraph (re-captured when a pointer changes);
 * `stream` must be a non-default stream.  Single-frame control loop: predict_controls,
 * autonomous_drive.py:908-920. */
int cilrs_net_forward_u8_graph(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frames,
                               const float* speed, const int64_t* command, float* controls,
                               float* pred_speed, void* stream);

/* cilrs_net_forward_u8 for ONE frame as ONE persistent launch (csrc/infer_b1.hip): the agent's
 * per-tick call `controls, pred_speed = self.model(img_t, speed_t, cmd_t)` under model.eval() and
 * torch.no_grad() (predict_controls, model/autonomous_drive.py:908-920).  One 1,024-thread
 * workgroup per CU walks a stage table (preprocess, stem, max-pool, the 16 BasicBlocks, avg-pool,
 * speed encoder, the COMMANDED branch and the speed head) separated by in-launch grid barriers;
 * no hipGraph, no per-layer launches.  Plans of batch 1 of the reference network only.  The device
 * must be able to keep one workgroup per CU resident: a second persistent launch running at the
 * same time on the same device (another stream, another process) can stall both until the bounded
 * barrier spin gives up -- then status word 1 is set and the outputs are NaN.  Status word 0 is
 * SET (never cleared: sticky, see cilrs_net_status_offset) by a call whose command lies outside
 * 0..3, where the reference's torch.gather raises. */
int cilrs_net_forward_u8_b1(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frame,
                            const float* speed, const int64_t* command, float* controls,
                            float* pred_speed, void* stream);
/* The agent's whole tick on a raw camera frame (preprocess_image + model call,
 * model/autonomous_drive.py:897-920): the fused resize / normalise transform of
 * cilrs_net_forward_camera, then the persistent launch from its second stage.  `frame` may be
 * pinned host memory; sync != 0 ends with hipStreamSynchronize(stream). */
int cilrs_net_forward_camera_b1(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frame,
                                int src_h, int src_w, int pixel_stride, long row_stride,
                                const float* speed, const int64_t* command, float* controls,
                                float* pred_speed, int sync, void* stream);
/* ... that posts its completion itself: right after the four outputs the launch stores `seq` into
 * `done` (a word of pinned host memory next to the outputs).  A control loop that keeps frame,
 * outputs and this word in ONE pinned buffer launches, spins on the word and reads the outputs --
 * no stream synchronisation on the tick's critical path (it saves the completion-signal and
 * wake-up latency, ~10 us of a ~0.3 ms tick).  The launch still completes on `stream` as usual. */
int cilrs_net_forward_u8_b1_post(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frame,
                                 const float* speed, const int64_t* command, float* controls,
                                 float* pred_speed, int* done, int seq, void* stream);
/* ... followed by hipStreamSynchronize(stream): one library call per control-loop tick when the
 * frame / speed / command and the outputs live in pinned host memory (the kernel reads and writes
 * them in place; no copy commands). */
int cilrs_net_forward_u8_b1_sync(cilrs_net* net, const cilrs_buffers* bufs, const uint8_t* frame,
                                 const float* speed, const int64_t* command, float* controls,
                                 float* pred_speed, void* stream);
/* how many convolutions of this plan's TRAIN step run on the Winograd F(2x2,3x3) kernel (forward
 * and data gradient each; csrc/conv_wino.hip): the stride-1 3x3 layers of an fp32 train plan with
 * up to 256 channels and at least half a chip of 64-tile x 64-channel blocks.  CILRS_WINO=0 in the
 * environment of the process turns the path off (0 here), CILRS_WINO=2 drops the block-count rule. */
int cilrs_net_wino_convs(cilrs_net* net);
/* number of stages (= grid barriers + 1) of that launch; -1 before the first call, 0 if the plan
 * has no persistent path */
int cilrs_net_b1_stages(cilrs_net* net);
/* test aid: how the planner tiled stage `stage` (0 .. cilrs_net_b1_stages - 1) of that launch, read
 * from the host copy of the stage table.  type: 0 preprocess, 1 convolution, 2 stem, 3 max-pool,
 * 4 head layer; workgroups: the resident grid the table was planned for.  Convolution and stem
 * stages: wpt = waves per unit (2, 4, 8 or 16), same_shape = 1 if the stage reuses the previous
 * stage's lane plan, nconv = 1 or 2 convolutions in the stage, and for each of them (arrays of two,
 * unused entries -1 / 0) its number as in cilrs_net_activation_info, ksplit = workgroups per
 * output tile and nt = channel tiles per unit.  Other stages: wpt 0, nconv 0.  Any pointer may be
 * NULL.  Fails before the plan's first persistent launch. */
int cilrs_net_b1_stage_info(const cilrs_net* net, int stage, int* type, int* wpt, int* same_shape,
                            int* workgroups, int* nconv, int* conv, int* ksplit, int* nt);
/* Re-base the launch's monotonic barrier counters (the eight arrival shards and the epoch word,
 * which are equal between launches) to `value`, after synchronising `stream`.  The counters are
 * compared wrap-safe (unsigned difference), so a long-running control loop never needs this; it
 * exists so that a test can place them just below INT_MAX and watch the launch cross the wrap
 * (tests/test_model_gpu.py), and as a maintenance hook. */
int cilrs_net_b1_set_epoch(cilrs_net* net, const cilrs_buffers* bufs, int value, void* stream);
/* diagnostics (library started with CILRS_B1_STAMPS=1): block 0's clock of the LAST persistent
 * launch -- start_us[i] = when stage i began (relative to stage 0), work_us[i] = how long block 0
 * worked in it before it entered the grid barrier.  Synchronous (one device->host copy). */
int cilrs_net_b1_stage_us(cilrs_net* net, const cilrs_buffers* bufs, float* start_us,
                          float* work_us, int cap);

/* CILRSLoss.forward + its gradient (notebook/notebook.ipynb:514-527).
 * kind 1: w0*L1(steer)+w1*L1(throttle)+w2*L1(brake)+w3*MSE(speed)     (executed config B)
 * kind 0: MSE(controls[B,3]) + w3*MSE(speed)                            (documented config A)
 * loss_out[6] (device) = total, control, steer, throttle, brake, speed.
 * dcontrols[B,3] / dpred_speed[B] = d total / d prediction, times grad_scale. */
int cilrs_loss_fwd_bwd(const float* controls, const float* target_controls,
                       const float* pred_speed, const float* target_speed, int batch, int kind,
                       const float* weights4_host, float grad_scale, float* dcontrols,
                       float* dpred_speed, float* loss_out, void* stream);

/* loss.backward() (notebook/notebook.ipynb:552) for the graph recorded by the last train-mode
 * cilrs_net_forward (or cilrs_net_forward_frozen: BatchNorm with fixed statistics): writes (overwrites) every parameter gradient of the segments
 * [seg_begin, seg_end) into bufs->grads.  Segments, in execution order:
 * 0 heads, 1 layer4, 2 layer3, 3 layer2, 4 layer1, 5 stem  (so data-parallel callers can
 * all-reduce a finished segment's gradient range while the next one runs). */
int cilrs_net_backward(cilrs_net* net, const cilrs_buffers* bufs, const float* dcontrols,
                       const float* dpred_speed, int seg_begin, int seg_end, void* stream);
/* Gradients with respect to the INPUTS (image.grad / speed.grad after loss.backward(), or
 * torch.autograd.grad(out, image) -- saliency maps, d controls / d speed) of the graph of the last
 * cilrs_net_forward(train != 0) or cilrs_net_forward_frozen on this plan, after
 * cilrs_net_backward of that forward: dimage (may be NULL) = logical NCHW f32 [B,3,H,W] with
 * element strides (sn,sc,sh,sw), overwritten -- needs segment 5 of that backward; dspeed (may be
 * NULL) = f32 [B], overwritten -- needs segment 0.  Both are plain sums in a fixed order
 * (bit-identical from run to run). */
int cilrs_net_input_grads(cilrs_net* net, const cilrs_buffers* bufs, float* dimage, long sn, long sc,
                          long sh, long sw, float* dspeed, void* stream);
/* The data-gradient chain of cilrs_net_backward and nothing else -- torch.autograd.grad(out, image)
 * or loss.backward() with every parameter frozen (requires_grad_(False)): the backward of a
 * saliency map.  No weight-gradient launch of any kind (convolutions, the stem, the heads' dW / db),
 * nothing on the weight-gradient stream, bufs->grads is never written and may be NULL.  Sets the
 * same state as cilrs_net_backward, so cilrs_net_input_grads follows it unchanged, and handles a
 * fine-tuning cut the same way (the chain stops at the cut; the image gradient is refused there).
 *   train-mode graphs: the BatchNorm reductions stay (they feed dx); their dgamma / dbeta
 *     by-products go to a workspace scratch.
 *   frozen graphs (cilrs_net_forward_frozen*): every BatchNorm backward is one reduction-free
 *     launch, dy = (z > 0 ? dz : 0) * (gamma * rstd), the pre-BN tensor is not read (the stem, whose
 *     post-BN tensor is never stored, rebuilds its mask from it), and the data gradients run
 *     without the BatchNorm-partials epilogue.
 * The convolution plans are those of cilrs_net_backward: image and speed gradients are equal to
 * what cilrs_net_backward + cilrs_net_input_grads give (element for element under torch.equal). */
int cilrs_net_backward_data(cilrs_net* net, const cilrs_buffers* bufs, const float* dcontrols,
                            const float* dpred_speed, int seg_begin, int seg_end, void* stream);
/* float range [begin,end) of the gradient arena that segment `seg` produces */
int cilrs_segment_range(int seg, size_t* begin, size_t* end);
/* the same for architecture variant `variant` (0 = the reference's ResNet-34, 1 = ResNet-50) */
int cilrs_variant_segment_range(int variant, int seg, size_t* begin, size_t* end);

/* torch.nn.utils.clip_grad_norm_ (notebook/notebook.ipynb:553-554): out[0] = total L2 norm,
 * out[1] = min(1, max_norm/(norm+1e-6)) (1 when max_norm <= 0); device results, no sync.
 * scratch: cilrs_sqnorm_scratch_bytes() bytes. */
size_t cilrs_sqnorm_scratch_bytes(void);
int cilrs_grad_sqnorm(const float* grads, size_t n, float max_norm, void* scratch, float* out2,
                      void* stream);

/* torch.optim.Adam.step() with coupled L2 weight decay (notebook/notebook.ipynb:533-534, 555)
 * over a flat arena; `step` is the 1-based step count; clip_out2 (may be NULL) is the device
 * result of cilrs_grad_sqnorm whose [1] scales the gradients; grad_scale multiplies them too
 * (1/world_size for data parallel sums). */
int cilrs_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                    size_t n, double lr, double beta1, double beta2, double eps,
                    double weight_decay, int64_t step, const float* clip_out2, float grad_scale,
                    void* stream);
/* The same update over `ngroups` (1..8) adjacent ranges [0, ends[0]), [ends[0], ends[1]) ... of the
 * arrays (ends in floats, multiples of 4, the last one = n), each with its own learning rate and
 * 1-based step count -- parameter groups with a learning-rate multiplier, and groups that sat out
 * steps while frozen (torch.optim.Adam keeps `step` per parameter).  One launch; element for
 * element the arithmetic of cilrs_adam_step on each range.  ends / lrs / steps: host arrays. */
int cilrs_adam_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                           size_t n, int ngroups, const size_t* ends, const double* lrs,
                           const int64_t* steps, double beta1, double beta2, double eps,
                           double weight_decay, const float* clip_out2, float grad_scale,
                           void* stream);
int cilrs_scale(float* x, size_t n, const float* clip_out2, float c, void* stream);

/* ---- exponential moving average (EMA) of the weights ---------------------------------------------
 * Rides on optimizer.step() (notebook/notebook.ipynb:555); the reference keeps no such average, so
 * this text is the definition.  After the Adam update of a step, for every element
 *     ema = ema + w * (p_new - ema)
 * as three separately rounded fp32 operations (no FMA contraction); where ema == p the element
 * comes back bit-identical.  w = float32(1 - d_t) is computed by the caller in double and rounded
 * once; 0 <= w <= 1.  All arrays: 16-byte aligned, n a multiple of 4.  Every refusal happens
 * before any launch.
 *
 * cilrs_ema_update: the stand-alone streaming pass (reads params, reads and writes ema); ema may
 * not overlap params. */
int cilrs_ema_update(float* ema, const float* params, size_t n, float w, void* stream);
/* cilrs_adam_step / cilrs_adam_step_groups with the average fused in: the Adam arithmetic is
 * element for element theirs, the EMA line runs on the just-computed parameter while it is still
 * in a register (one more read and one more write of an arena-sized array instead of the two reads,
 * one write and one launch of a separate pass; measured on an MI355X that does not pay --
 * possibly because the separate pass finds the just-written parameters in the last-level cache,
 * which was not confirmed with counters: DESIGN.md section 5c).  ema: n floats, may not be NULL and may not overlap
 * params, grads, exp_avg or exp_avg_sq. */
int cilrs_adam_step_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                        size_t n, double lr, double beta1, double beta2, double eps,
                        double weight_decay, int64_t step, const float* clip_out2,
                        float grad_scale, float* ema, float ema_w, void* stream);
int cilrs_adam_step_groups_ema(float* params, const float* grads, float* exp_avg,
                               float* exp_avg_sq, size_t n, int ngroups, const size_t* ends,
                               const double* lrs, const int64_t* steps, double beta1, double beta2,
                               double eps, double weight_decay, const float* clip_out2,
                               float grad_scale, float* ema, float ema_w, void* stream);
/* ---- AdamW and LAMB with per-tensor trust ratios ---------------------------------------------------
 * The reference trains with torch.optim.Adam alone and torch ships no LAMB, so this text is the
 * definition of both.  All arithmetic is fp32 unless a line says double.  gs is the gradient scale
 * of cilrs_adam_step: clip_out2[1] * grad_scale, or grad_scale alone.  The scalars 1-beta1, beta2,
 * 1-beta2, eps, wd, bc1 = 1-beta1^t, bc2_sqrt = sqrt(1-beta2^t), 1/bc1, -lr/bc1 and 1-lr*wd are
 * prepared on the host in double and rounded to fp32 once.
 *
 * Both kinds share the moment update of cilrs_adam_step without its L2 term:
 *     g' = g * gs
 *     m  = m + (1-beta1) * (g' - m)
 *     v  = v * beta2 + ((1-beta2) * g') * g'
 *     denom = sqrtf(v) / bc2_sqrt + eps
 *
 * A SEGMENT is one parameter tensor: the arena range from its offset to the next tensor's offset.
 * Segment ends are multiples of 4; the padding floats are zero in all four arrays and stay zero.
 * Each segment carries two flag bits: CILRS_SEG_NO_DECAY (the decay term is dropped for that tensor,
 * wd_s = 0; otherwise wd_s = wd) and CILRS_SEG_NO_ADAPT (LAMB only: the trust ratio is 1).
 *
 * CILRS_OPTIM_ADAMW (torch.optim.AdamW, decoupled decay), per element:
 *     p = p * (1 - lr*wd_s)                    [the factor is 1 under NO_DECAY]
 *     p = p + ((-lr/bc1) * m) / denom
 *
 * CILRS_OPTIM_LAMB (You et al. 2020, in the form apex and timm use), per element:
 *     u = (m * (1/bc1)) / denom + wd_s * p     [four separately rounded operations, no FMA]
 * per segment s without NO_ADAPT, np = sqrt(sum p^2) and nu = sqrt(sum u^2), both sums accumulated
 * in double from the fp32 values and the square roots taken in double; if trust_clip > 0,
 * np = min(np, trust_clip); r_s = np / nu in double when both are positive, else 1.  Under NO_ADAPT
 * r_s = 1.  Then
 *     p = p - (float)(lr * r_s) * u            [lr * r_s in double]
 * where the p in u and in the norms is the parameter before the step.
 *
 * Work decomposition: every segment is cut, from its own start, into chunks of at most
 * cilrs_optim_chunk_floats floats; one workgroup reduces one chunk in a fixed tree, and one wave
 * adds a segment's chunk sums (lane l takes sums l, l + 64, ... in table order, a fixed tree adds the
 * lanes).  No floating-point atomics: results are bit-identical from
 * run to run, and a tensor's new p, m, v and r_s are a function of its own data and scalars only --
 * not of where it sits in the arena, what stands before it or how many segments a call covers.
 *
 * The segment table is built and validated once (ends increasing, multiples of 4, the last one = n,
 * flags in range) and uploaded into caller-owned device memory of cilrs_optim_table_bytes bytes
 * (16-byte aligned; 0 = unusable ends); the returned handle keeps the host mirror that every later
 * refusal is decided on.  ends / flags: host arrays of nseg entries. */
#define CILRS_SEG_NO_DECAY 1
#define CILRS_SEG_NO_ADAPT 2
#define CILRS_OPTIM_ADAMW 1
#define CILRS_OPTIM_LAMB 2
typedef struct cilrs_optim_table cilrs_optim_table;
int cilrs_optim_chunk_floats(void);
size_t cilrs_optim_table_bytes(const size_t* ends, int nseg);
int cilrs_optim_table_create(const size_t* ends, const int* flags, int nseg, size_t n,
                             void* device_table, size_t device_bytes, void* stream,
                             cilrs_optim_table** out);
void cilrs_optim_table_destroy(cilrs_optim_table* table);
/* device scratch of a LAMB step over any run of the table: two doubles per chunk, one float per
 * segment; 16-byte aligned */
size_t cilrs_optim_scratch_bytes(const cilrs_optim_table* table);
/* One optimizer step of `kind` over the whole segments [first_seg, first_seg + count) of the table.
 * params / grads / exp_avg / exp_avg_sq: the WHOLE arrays the table describes (n floats, 16-byte
 * aligned); nothing outside the run is read or written.  ngroups (1..8) adjacent groups with a
 * learning rate and a 1-based step count each, as cilrs_adam_step_groups takes them: group_ends are
 * arena offsets in floats, each the end of a segment of the run, increasing, the last one the end of
 * the run; host arrays.  clip_out2 (may be NULL) and grad_scale: as cilrs_adam_step.  trust_clip:
 * 0 = off (LAMB only).  scratch: LAMB only (AdamW: may be NULL).  ratio_out (device, fp32, one per
 * segment OF THE TABLE, may be NULL): LAMB writes r_s of the run's segments at their table index.
 * AdamW is one launch; LAMB is three on `stream` with no host synchronisation.  No allocation or
 * upload per step; every refusal happens before any launch. */
int cilrs_optim_step(int kind, const cilrs_optim_table* table, int first_seg, int count,
                     float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                     int ngroups, const size_t* group_ends, const double* lrs, const int64_t* steps,
                     double beta1, double beta2, double eps, double weight_decay, double trust_clip,
                     const float* clip_out2, float grad_scale, void* scratch, float* ratio_out,
                     void* stream);

/* ---- sharpness-aware minimisation (SAM / ASAM; csrc/sam.hip) ------------------------------------------
 * Foret et al. 2021 and its scale-invariant form (Kwon et al. 2021): the gradient is taken at
 * w + e(w), the worst nearby point to first order, and applied at w.  The reference trains without
 * it and torch ships none, so this text is the definition -- the form of the widely used
 * `adaptive=` implementations, e = rho * w^2 g / || |w| g ||: no eta term, ONE norm over the whole
 * range.  The gradient's own scale cancels in e, so there is no grad_scale or clip argument.
 *
 * Over a flat range of n floats (n a multiple of 4, at most 2^30; all arrays 16-byte aligned: the
 * trainable range of the arena).  fp32 unless a line says double:
 *     t_i   = g_i                          [adaptive = 0]
 *     t_i   = |p_i| * g_i                  [adaptive = 1; one fp32 rounding]
 *     S     = sum_i (double)t_i * (double)t_i      [accumulated in double]
 *     norm  = sqrt(S)                              [double]
 *     scale = rho / (norm + 1e-12)                 [double];  s32 = (float)scale
 *     backup_i = p_i
 *     p_i   = p_i + s32 * g_i              [adaptive = 0; two roundings, no FMA]
 *     p_i   = p_i + s32 * (|p_i| * t_i)    [adaptive = 1; three roundings, no FMA]
 * rho = 0 and g = 0 leave p as it was (S = 0 gives scale = rho * 1e12, times zero); under
 * adaptive = 1 a zero weight stays zero.
 *
 * Summation order: the range is cut, from its own start, into chunks of cilrs_sam_chunk_floats
 * floats.  One workgroup reduces a chunk (thread t of 256 adds the squares of the chunk's quads
 * t, t + 256, ... in element order; a butterfly adds the 64 lanes of a wave, (w0 + w1) + (w2 + w3)
 * the four waves) and writes one double.  One workgroup then adds the chunk sums -- thread l takes
 * sums l, l + 256, ... in index order, the same tree adds the threads -- and writes
 * out3 = {S, norm, scale} (device, double).  No floating-point atomics: results are bit-identical
 * from run to run and a function of the range's own data only -- a sub-range perturbed through
 * offset pointers equals the same data perturbed stand-alone.  No sequential run of additions is
 * longer than 1,024 terms (16 in a chunk), so S is within 2^-40 relative of the exactly rounded sum.
 *
 * scratch: cilrs_sam_scratch_bytes(n) bytes of device memory, 16-byte aligned (0: n unusable): one
 * double per chunk, then room for three more, where out3 may point (out3: any 8-byte aligned device
 * address).  backup: n floats that overlap neither params nor grads.
 *
 * cilrs_sam_perturb is three launches on `stream` (chunk sums, finalise, apply) with no host
 * synchronisation, allocation or upload.  cilrs_sam_restore copies backup over params bit for bit
 * (-0.0, denormals and NaN payloads included): (p + e) - e is not p in fp32, and the weights a step
 * starts from must be the ones the optimizer updates.  Refused, before any launch: NULL pointers;
 * n zero, not a multiple of 4 or above 2^30; misaligned pointers; backup overlapping params or
 * grads; rho negative or not finite; adaptive not 0 or 1. */
int cilrs_sam_chunk_floats(void);
size_t cilrs_sam_scratch_bytes(size_t n);
int cilrs_sam_perturb(float* params, const float* grads, float* backup, size_t n, double rho,
                      int adaptive, void* scratch, double* out3, void* stream);
int cilrs_sam_restore(float* params, const float* backup, size_t n, void* stream);

/* ---- prioritised sampling: per-sample loss, priority table and draw (csrc/priority.hip) -------------
 * Prioritised replay (Schaul et al. 2016) over recorded frames: a step writes its per-sample losses,
 * they become priorities of the frames it saw, and the next batch's index is drawn from the
 * priorities on the device.  The reference samples by command alone (notebook:383-423) and has
 * none of this, so this text is the definition.
 *
 * cilrs_loss_fwd_bwd_rows: cilrs_loss_fwd_bwd plus two device arrays, each of which may be NULL:
 * row_weight [batch] (in) and row_loss [batch] (out).  With d_c = controls[b][c] -
 * target_controls[b][c] and d_s = pred_speed[b] - target_speed[b] (fp32 differences, as in the
 * loss itself; everything after them in double, cast to fp32 once):
 *     kind 0:  l_b = ((d_0^2 + d_1^2) + d_2^2) / 3 + w3 * d_s^2
 *     kind 1:  l_b = ((w0 |d_0| + w1 |d_1|) + w2 |d_2|) + w3 * d_s^2
 *     row_loss[b] = l_b                                         [never weighted]
 * so that mean_b l_b is loss_out[0] without weights.  With weights every gradient element of row b
 * is the unweighted fp32 one times row_weight[b] (one more rounding), and loss_out[0..5] are the
 * weighted means (1 / batch) sum_b row_weight[b] * term.  With row_weight == NULL loss_out,
 * dcontrols and dpred_speed are bit for bit cilrs_loss_fwd_bwd's: one workgroup, the same
 * per-thread sums and the same fold (the two kernels share their body), and all-ones weights give
 * those bits too.
 *
 * The table: q, uint32 [n], every entry in [1, 2^32 - 1]; 2^20 is priority 1.  Sums of entries are
 * uint64 and n is at most 2^31, so the total stays below 2^63 and, integer addition being
 * associative, does not depend on how the device groups it.  fixed(p) = llrint(p * 2^20) clamped to
 * [1, 2^32 - 1]; what is not below the upper end, NaN included, takes it.  pmax_state: one device
 * uint32, the running maximum of every q an update has written (the caller sets it, to 2^20, before
 * the first fill).
 *
 * cilrs_priority_fill: q[i] = fixed(base[i] * pmax_state / 2^20) for all i -- what a frame holds
 * until its first visit, PER's "new samples get the maximum priority" (base NULL: 1).
 *
 * cilrs_priority_update, for b in [0, batch), batch <= cilrs_priority_max_batch() = 1024:
 *     x = (double)row_loss[b] + eps;   x^alpha = 1, x, sqrt(x) for alpha = 0, 1, 0.5, pow otherwise
 *     q[pos[b]] = fixed(base[pos[b]] * x^alpha)          [double]
 *     q[pos[b]] = 2^32 - 1 where row_loss[b] is not finite
 * Where a position repeats inside pos the highest b alone writes; a position outside [0, n) is
 * never written; then pmax_state = max(pmax_state, every q written).  One launch of one workgroup.
 *
 * cilrs_priority_draw, with total = sum q and, for b in [0, batch), batch <= 1024,
 *     r_b = splitmix64(seed + (counter * batch + b) * 0xD1B54A32D192ED03)     [mod 2^64]
 *     stratified and total >= batch:  quo = total / batch, rem = total % batch,
 *         lo_b = quo * b + min(b, rem),  len_b = quo + (b < rem),  t_b = lo_b + mulhi64(r_b, len_b)
 *     otherwise:                      t_b = mulhi64(r_b, total)
 *     out_pos[b]    = the smallest i with q[0] + ... + q[i] > t_b      [< n, all integer so far]
 *     out_index[b]  = subset ? subset[out_pos[b]] : out_pos[b]
 *     out_weight[b] = v_b / max_b' v_b',  v_b = pow(total / (n * q[out_pos[b]]), beta)   [double]
 * beta = 0 gives exactly 1.0f.  subset (int64 [n], or NULL) maps table positions to frames of a
 * dataset of n_frames frames; its values are the caller's to check against n_frames, once.  Three
 * launches on `stream` (sums of chunks of 1,024 entries, their scan, the draw), no host
 * synchronisation, allocation or upload, no floating-point atomics.  scratch:
 * cilrs_priority_scratch_bytes(n) bytes of device memory, 8-byte aligned (0: n unusable); q must be
 * 16-byte aligned.  Refused before any launch: NULL pointers, n outside [1, 2^31], batch outside
 * [1, 1024], alpha negative, eps not positive, beta outside [0, 1], misaligned q or scratch. */
int cilrs_loss_fwd_bwd_rows(const float* controls, const float* target_controls,
                            const float* pred_speed, const float* target_speed, int batch, int kind,
                            const float* weights4_host, float grad_scale, float* dcontrols,
                            float* dpred_speed, float* loss_out, const float* row_weight,
                            float* row_loss, void* stream);
int cilrs_priority_max_batch(void);
int cilrs_priority_fill(uint32_t* q, int64_t n, const float* base, const uint32_t* pmax_state,
                        void* stream);
int cilrs_priority_update(uint32_t* q, int64_t n, const int64_t* pos, const float* row_loss,
                          const float* base, double alpha, double eps, uint32_t* pmax_state,
                          int batch, void* stream);
size_t cilrs_priority_scratch_bytes(int64_t n);
int cilrs_priority_draw(const uint32_t* q, int64_t n, const int64_t* subset, int64_t n_frames,
                        uint64_t seed, uint64_t counter, int batch, int stratified, double beta,
                        int64_t* out_pos, int64_t* out_index, float* out_weight, void* scratch,
                        void* stream);

/* In-place exchange of two arrays of n floats that do not overlap, in one pass.  The plans cache the
 * parameter arena's address: averaged weights are evaluated by swapping them into the arena and
 * out again, never by re-binding pointers. */
int cilrs_swap(float* a, float* b, size_t n, void* stream);

/* op-level stem convolution of the TRAINING step (visual_encoder.0 = torchvision resnet34.conv1,
 * model/autonomous_drive.py:366; trained by notebook/notebook.ipynb:549-555): conv 7x7 / stride 2 /
 * pad 3, fp32, x4 = the channel-padded NHWC image [N,H,W,4], w = OHWI [64,7,7,3], y = [N,Ho,Wo,64];
 * bn_partial (may be NULL) receives the [2][64][*partial_rows] column partials (sum, sum of
 * squares) the following BatchNorm reduces.  Widths up to 445 pixels. */
int cilrs_stem_conv_fwd(const float* x4, const float* w, float* y, float* bn_partial, int N, int H,
                        int W, int* partial_rows, void* stream);

/* ... and its weight gradient (loss.backward() through that layer, notebook/notebook.ipynb:552):
 * dw = OHWI [64,7,7,3] (overwritten) from x4 and dy = [N,Ho,Wo,64]; scratch of
 * cilrs_stem_conv_wgrad_scratch_floats() floats.  Served geometries: rows of 100 or 200 output
 * pixels (the reference's 200x88 frames and the 400x176 variant); _scratch_floats() returns 0
 * otherwise and cilrs_conv2d_wgrad on the channel-padded image is the general path. */
size_t cilrs_stem_conv_wgrad_scratch_floats(int N, int H, int W);
int cilrs_stem_conv_wgrad(const float* x4, const float* dy, float* dw, float* scratch,
                          size_t scratch_floats, int N, int H, int W, void* stream);

/* ... and its data gradient (d image through that layer: torch.nn.grad.conv2d_input):
 * dx = logical NCHW f32 [N,3,H,W] with element strides (sn,sc,sh,sw), overwritten, from
 * dy = [N,Ho,Wo,64] and w = OHWI [64,7,7,3].  Any geometry; no scratch; no atomics. */
int cilrs_stem_conv_dgrad(const float* dy, const float* w, float* dx, long sn, long sc, long sh,
                          long sw, int N, int H, int W, void* stream);

/* loss.backward() + optimizer.step() (notebook/notebook.ipynb:552, 555) in ONE call for steps
 * without gradient clipping: cilrs_net_backward over all six segments, and the Adam update of a
 * segment's parameter range enqueued as soon as that segment's gradients are complete (on the
 * plan's weight-gradient stream, so the HBM-bound update of layer4's 13 M parameters runs under
 * the data gradients of layers 3..1).  Same arithmetic per element as cilrs_adam_step; when the
 * call returns its work to `stream`, parameters, moments and gradients are final.  A step that
 * clips (nb:553-554) needs the global norm first: cilrs_net_backward + cilrs_grad_sqnorm +
 * cilrs_adam_step. */
typedef struct {
    float* exp_avg;         /* arena-shaped first / second moments                     */
    float* exp_avg_sq;
    double lr, beta1, beta2, eps, weight_decay;
    int64_t step;           /* 1-based step count                                       */
    float grad_scale;       /* multiplies the gradients (1 / world_size for summed DP gradients) */
} cilrs_adam_args;
int cilrs_net_backward_step(cilrs_net* net, const cilrs_buffers* bufs, const float* dcontrols,
                            const float* dpred_speed, const cilrs_adam_args* opt, void* stream);

/* ---- training input pipeline on the device ------------------------------------
 * The reference's per-frame CPU augmentation (albumentations Compose, notebook/notebook.ipynb:387-394:
 * RandomBrightnessContrast p.5, HueSaturationValue p.3, GaussianBlur p.2, GaussNoise p.3,
 * CoarseDropout p.2) + /255 + Normalize (:412-414) as one kernel over a uint8 batch.  The random
 * parameters of each sample are drawn by the caller; a step is disabled by its *_on / 0 value.
 * albumentations / cv2 are absent from the build image: the steps restate their published
 * behaviour and are parity-unpinned against the libraries themselves. */
typedef struct {
    uint64_t noise_seed;     /* counter-based RNG key of this sample's Gaussian noise            */
    int rbc_on;              /* v' = trunc(clip(v * alpha + beta255))                             */
    float alpha, beta255;
    int hsv_on;              /* 8-bit HSV (H in half-degrees): H+hue mod 180, S+sat, V+val clipped.
                              * The shifted hue is the LUT trunc(mod(arange(180) + hue, 180)) to
                              * within one step and always lies in [0, 179]: a wrap that float32
                              * rounds up to 180 becomes 0                                         */
    float hue, sat, val;
    int blur_k;              /* 0/1 = off, 3 or 5 = Gaussian taps; blur_w = centre, +-1, +-2.
                              * Border: reflect-101 with period 2(n-1) at every n >= 2, so height
                              * or width 2 is valid with five taps too: indices -2, -1, 2, 3 read
                              * 0, 1, 0, 1 (np.pad "reflect"); no tap leaves the sample's frame    */
    float blur_w[3];
    float noise_std255;      /* 0 = off; sigma in grey levels                                      */
    int nholes;              /* 0..3 rectangles [y0,y1) x [x0,x1) set to 0                         */
    int hole_y0[3], hole_x0[3], hole_y1[3], hole_x1[3];
    int reserved;
} cilrs_aug_params;          /* 112 bytes */

/* frames uint8 [B,H,W,3] (device), params [B] (device) -> out_f32 [B,H,W,3] normalised floats
 * (feed it to cilrs_net_forward as the NCHW view with strides (H*W*3, 1, W*3, 3)) and/or out_u8
 * [B,H,W,3] augmented bytes; either output may be NULL. */
int cilrs_augment_u8(const uint8_t* frames, const cilrs_aug_params* params, int batch, int height,
                     int width, float* out_f32, uint8_t* out_u8, void* stream);

/* A whole training batch from a device-resident dataset in one launch (the decoded frames stay on
 * the device after the first epoch: no JPEG decode, staging buffer or host-to-device copy per step).
 *   cache    uint8 [n_frames][H][W][3]; addressed in 64 bits, so it may exceed 4 GiB
 *   speed    f32 [n_frames], command i64 [n_frames], targets f32 [n_frames][3]
 *   index    i64 [B]: sample b is frame index[b]; values may repeat and come in any order.  Every
 *            value must lie in [0, n_frames): that is the caller's contract (a value outside it
 *            is never read, and that sample's outputs are left unwritten)
 *   params   [B], as for cilrs_augment_u8
 * -> out_f32 / out_u8 [B][H][W][3], element for element what cilrs_augment_u8 gives on the gathered
 * frames (the kernels share their device code); either may be NULL, not both.  out_speed [B],
 * out_command [B], out_targets [B][3] are gathered by the same index; each may be NULL, and a label
 * input is only required when its output is asked for.  B*H*W < 2^31 as above. */
int cilrs_batch_assemble(const uint8_t* cache, int64_t n_frames, const float* speed,
                         const int64_t* command, const float* targets, const int64_t* index,
                         const cilrs_aug_params* params, int batch, int height, int width,
                         float* out_f32, uint8_t* out_u8, float* out_speed, int64_t* out_command,
                         float* out_targets, void* stream);

/* ---- weather on the device: tone, fog and rain in front of the augmentation --------------------
 * The reference scores its checkpoint under five weather profiles (configs/weather_config.json:
 * clear, rain, fog, night, hardrain) and names domain randomisation as a way forward; CARLA's
 * renderer is not available here, so this is a parity-unpinned image-space model.  Weather is a pure
 * function of the uint8 source pixel c, its position (y, x) and the sample's record, applied before
 * the colour stages above to every source pixel they read (the blur's taps included).  All float32,
 * one rounding per operation, nothing transcendental: what needs exp() is folded into the record by
 * the host (cilrs_mi355/data.py).  In order:
 *   tone  c_k = trunc(clip255(c_k * gain_k + lift255_k))
 *   fog   d = 1 for (float)y <= fog_horizon, else fog_near / max((float)y - fog_horizon, fog_near);
 *         t = clip(fog_t0 + fog_t1 * d, 0, 1);  c_k = rint(clip255(A_k + (c_k - A_k) * t)), A = fog_rgb255
 *   rain  a streak head sits at integer (yy, xx), inside the frame or not, when
 *         splitmix64(rain_seed + ((yy + 64) * 65536 + (xx + 64)) * 0xD1B54A32D192ED03) >> 40 < rain_thresh24;
 *         tail position j in [0, rain_len) covers (y, x) when (y - j, x - ((j * rain_slant_q4) >> 4))
 *         is a head; with the smallest covering j, a = rain_alpha * ((float)(L - j) / (float)L) and
 *         c_k = rint(clip255(c_k + a * (rain_v255 - c_k))); uncovered pixels are untouched
 * A record with all three off (zeroes) is the identity. */
typedef struct {
    uint64_t rain_seed;      /* key of this sample's streak heads                                  */
    int tone_on;
    float gain[3], lift255[3];
    int fog_on;
    float fog_t0, fog_t1;    /* transmission = clip(t0 + t1 * d)                                   */
    float fog_horizon, fog_near;     /* rows                                                       */
    float fog_rgb255[3];     /* airlight                                                           */
    int rain_len;            /* 0 = off, at most 16                                                */
    int rain_slant_q4;       /* columns per 16 rows, in [-16, 16]                                  */
    uint32_t rain_thresh24;  /* head probability * 2^24                                            */
    float rain_alpha, rain_v255;
    int reserved[2];
} cilrs_weather_params;      /* 96 bytes */

/* cilrs_augment_u8 / cilrs_batch_assemble with weather [B] (device) in front, one launch each:
 * element for element what the plain entry point gives on frames that were first put through the
 * weather and stored as uint8 (the kernels share their device code).  width <= 65,408. */
int cilrs_augment_weather_u8(const uint8_t* frames, const cilrs_aug_params* params,
                             const cilrs_weather_params* weather, int batch, int height, int width,
                             float* out_f32, uint8_t* out_u8, void* stream);
int cilrs_batch_assemble_weather(const uint8_t* cache, int64_t n_frames, const float* speed,
                                 const int64_t* command, const float* targets,
                                 const int64_t* index, const cilrs_aug_params* params,
                                 const cilrs_weather_params* weather, int batch, int height,
                                 int width, float* out_f32, uint8_t* out_u8, float* out_speed,
                                 int64_t* out_command, float* out_targets, void* stream);

/* ---- viewpoint on the device: lateral offset and yaw in front of everything else ---------------
 * The reference records an expert that never leaves the lane centre (model/collect_data.py: one
 * camera at y = 0, the autopilot, no steering noise), so its network never sees a recovery.  The
 * remedy since PilotNet is shifted and rotated views with a corrected steering label.  Here that is
 * a per-sample piecewise projective warp: two inverse homographies (destination pixel -> source
 * pixel, row-major), `far` for rows at or above split_row and `ground` for the rows below it.
 * Wherever a stage above reads source pixel (y, x) -- the blur's taps after reflect-101 included --
 * it reads pixel (y, x) of the virtual frame V instead.  All float32, one rounding per operation,
 * in this order (p is the stored uint8 frame [H][W][3]):
 *   M  = ((float)y > split_row) ? ground : far
 *   u  = (M0*(float)x + M1*(float)y) + M2;  v = (M3*x + M4*y) + M5;  w = (M6*x + M7*y) + M8
 *   sx = fminf(fmaxf(u / w, 0), (float)(W-1));  sy = fminf(fmaxf(v / w, 0), (float)(H-1))
 *        (replicate border; this nesting sends a NaN to 0, so whatever the record holds no
 *        address outside the sample's frame is formed)
 *   x0 = (int)floorf(sx);  ax = sx - (float)x0;  x1 = min(x0 + 1, W-1);   the same for y
 *   top = p[y0][x0] + ax * (p[y0][x1] - p[y0][x0]);  bot likewise on row y1
 *   V[y][x][k] = rintf(clip255(top + ay * (bot - top)))
 * Weather and the augmentation then act on V at V's own coordinates: the entry points below give,
 * element for element, what cilrs_augment_[weather_]u8 / cilrs_batch_assemble[_weather] give on
 * frames first put through the warp and stored as uint8.  A record with on == 0 reads the stored
 * byte and nothing else.  steer_delta corrects the label (cilrs_batch_assemble_view); lateral_m and
 * yaw_rad are carried for the caller and not read by the kernels. */
typedef struct {
    int on;
    float split_row;         /* rows with (float)y > split_row use `ground`                        */
    float far[9], ground[9]; /* destination -> source, row-major                                   */
    float steer_delta;       /* added to the steer label where on != 0                             */
    float lateral_m, yaw_rad;
    int reserved;
} cilrs_view_params;         /* 96 bytes */

/* cilrs_augment_weather_u8 / cilrs_batch_assemble_weather with view [B] (device, never NULL) in
 * front, one launch each; weather may be NULL (no weather stage, and no width limit).  The assemble
 * entry also corrects the label: where on != 0,
 *   out_targets[b][0] = fminf(fmaxf(targets[index[b]][0] + steer_delta, -1), 1)
 * and where on == 0 the three targets are copied, never added to (a stored -0.0 stays -0.0).
 * Throttle, brake, speed and command are gathered unchanged.  NULL view, bad geometry and, with
 * weather, width > 65,408 are refused before any launch. */
int cilrs_augment_view_u8(const uint8_t* frames, const cilrs_aug_params* params,
                          const cilrs_weather_params* weather, const cilrs_view_params* view,
                          int batch, int height, int width, float* out_f32, uint8_t* out_u8,
                          void* stream);
int cilrs_batch_assemble_view(const uint8_t* cache, int64_t n_frames, const float* speed,
                              const int64_t* command, const float* targets, const int64_t* index,
                              const cilrs_aug_params* params, const cilrs_weather_params* weather,
                              const cilrs_view_params* view, int batch, int height, int width,
                              float* out_f32, uint8_t* out_u8, float* out_speed,
                              int64_t* out_command, float* out_targets, void* stream);

/* ---- closed-loop replay of recorded drives (csrc/replay.hip; evaluate.replay) -------------------
 * B segments of a recorded drive are replayed at once: the predicted steer moves a kinematic
 * bicycle off the recorded path, the next recorded frame is shown from where the car now is
 * (a view record for cilrs_batch_assemble_view), and what a safety driver would have had to do is
 * counted -- PilotNet's re-simulator, without a renderer.  One thread per segment, all in double,
 * a*b+c never fused, no atomics: a segment's result does not depend on its place in the batch.
 *
 * Per segment b: start[b], lateral0[b], yaw0[b]; state e (metres, right positive), psi (radians,
 * right positive), a steer history of at most ntaps values.  Tick k = 0 .. T-1 on frame
 * i = start[b] + k:
 *   render   v_n = (double)speed[i].  e == 0 and psi == 0: the record is off and holds the
 *            identity (the bytes of data.identity_view).  Otherwise on = 1, split_row = cy,
 *              Rt = [c 0 s; 0 1 0; -s 0 c] (c, s = cos, sin psi),  Sh = [c t/h s; 0 1 0; -s 0 c], t = e
 *              far = K Rt K^-1, ground = K Sh K^-1, each divided by (its third row) . (cx, cy, 1)
 *              and exactly the identity where its middle factor is,
 *              L = max(lookahead_s * v, min_lookahead_m), v = v_n * speed_unit_ms
 *              steer_delta = atan(wheelbase_m * 2 (0 - e cos psi - L sin psi) / L^2) / max_wheel_rad
 *            built in double, cast to float32 (data.view_records; lateral_m = e, yaw_rad = psi).
 *            index[b] = i.  The metrics of tick k use this (e, psi).
 *   forward  the caller's: one cilrs_batch_assemble_view launch on (index, view), then the network.
 *   advance  raw = (double)controls[b][0], sx = clip((double)targets[i][0], -1, 1) (the stored
 *            label), delta = the double steer_delta above (0 at e == psi == 0).
 *            ticks += 1; S|e|, Se^2, max|e|, S|psi|, max|psi| take (e, psi); a segment that
 *            started with |lateral0| >= recover_m and has had no intervention yet sets
 *            recover_tick = k at its first |e| < recover_m.
 *            raw not finite: nonfinite += 1, intervene.  Otherwise raw joins the history (the last
 *            ntaps values are kept), s = sum(w * hist) / sum(w) summed oldest to newest with w the
 *            last len(hist) taps (s = raw with ntaps == 0 or one value), s = clip(s, -1, 1);
 *            steer_ticks += 1; S|s - sx|, S|s - clip(sx + delta, -1, 1)|, and S(s - s_prev)^2 where
 *            the previous tick of this stretch had a steer.  Then, when closed_loop:
 *              ds = (v_n * speed_unit_ms) * dt_s
 *              e' = e + ds * sin(psi)
 *              psi' = psi + ds * (tan(s * max_wheel_rad) - tan(sx * max_wheel_rad)) / wheelbase_m
 *              e' or psi' not finite (a non-finite speed or label): nonfinite += 1, intervene
 *              else |e'| > max_lateral_m: lateral += 1, intervene
 *              else |psi'| > max_yaw_rad: yaw += 1, intervene
 *              else (e, psi) = (e', psi').            |e'| == max_lateral_m is no intervention.
 *            An intervention sets e = psi = 0 (closed loop), empties the history and ends the
 *            stretch.  With closed_loop == 0 the state stays (lateral0, yaw0).
 * This is the small-offset Frenet form: the factor cos(psi) / (1 - e kappa) on the expert's
 * curvature is dropped.  Longitudinal motion stays the expert's; throttle and brake are not
 * simulated.  The state is finite after every advance, and a render that finds a non-finite state
 * resets it to (0, 0) first: no record is ever computed from one.
 *
 * metrics [B][cilrs_replay_metric_doubles()]: ticks, lateral, yaw, nonfinite, S|e|, Se^2, max|e|,
 *   S|psi|, max|psi|, S|s - sx|, S|s - corrected|, S(ds)^2, recover_tick (-1: none), steer_ticks.
 * state [B][cilrs_replay_state_doubles()]: e, psi, len(hist), hist[8], s_prev, has_prev,
 *   recover_open, lateral0, yaw0, start.  Both are opaque to everything but the tests. */
typedef struct {
    double dt_s, speed_unit_ms, wheelbase_m, max_wheel_rad, lookahead_s, min_lookahead_m;
    double fx, fy, cx, cy, height_m;           /* the camera at the dataset's H x W */
    double max_lateral_m, max_yaw_rad, recover_m;
    double taps[8];                            /* oldest to newest; the first ntaps are read */
    int ntaps, closed_loop;
} cilrs_replay_config;       /* 184 bytes */

int cilrs_replay_state_doubles(void);
int cilrs_replay_metric_doubles(void);
/* start, lateral0, yaw0: HOST arrays [batch].  Refused before any launch: NULL pointers, batch < 1,
 * ticks < 1, start[b] < 0, start[b] + ticks > n_frames, a non-finite or out-of-box (lateral0, yaw0),
 * ntaps outside 0..8, taps that are not finite and non-negative with the newest positive, and
 * configuration values that are not finite and positive.  Writes state, zeroed metrics, and tick
 * 0's index [batch] and view [batch]; waits once for its own upload. */
int cilrs_replay_begin(const cilrs_replay_config* cfg, int batch, int ticks, int64_t n_frames,
                       const int64_t* start, const double* lateral0, const double* yaw0,
                       const float* speed, double* state, double* metrics, int64_t* index,
                       cilrs_view_params* view, void* stream);
/* tick >= 1: advance tick - 1 on controls [batch][3] (its forward's output), then render `tick`
 * into index and view.  trace_* (each may be NULL) receive tick - 1's row: trace_state [batch][2]
 * = (e, psi) as rendered, trace_steer [batch][2] = (raw, s; s is NaN where raw is not finite),
 * trace_flags [batch] = 1 lateral | 2 yaw | 4 nonfinite | 8 the record was on.  A segment whose
 * frame would fall outside [0, n_frames) is left untouched.  No host synchronisation. */
int cilrs_replay_step(const cilrs_replay_config* cfg, int batch, int tick, const float* controls,
                      const float* speed, const float* targets, int64_t n_frames, double* state,
                      double* metrics, int64_t* index, cilrs_view_params* view,
                      double* trace_state, float* trace_steer, uint8_t* trace_flags, void* stream);
/* folds in the last tick: the advance of cilrs_replay_step at tick = ticks, with no render */
int cilrs_replay_finish(const cilrs_replay_config* cfg, int batch, int ticks, const float* controls,
                        const float* speed, const float* targets, int64_t n_frames, double* state,
                        double* metrics, double* trace_state, float* trace_steer,
                        uint8_t* trace_flags, void* stream);

/* ---- evaluation report accumulators (metrics schema evaluation_report.json:1-73; the reference
 *      ships the report, not the code that made it) ---------------------------------------------
 * acc: cilrs_eval_acc_doubles() doubles on the device, zeroed by the caller before the first
 * batch and ADDED to by every call:
 *   [0..31]  channel c in (steer, throttle, brake, speed) x {n, Sp, St, Spt, Spp, Stt, S|d|, Sdd}
 *   [32..67] command k x {n, S|d_steer|, S|d_throttle|, S|d_brake|, then steer Sp, St, Spt, Spp, Stt}
 *   [68..71] rows with |d_steer| <= 0.01, 0.02, 0.05, 0.1
 * steer_abs_err (may be NULL): [batch] floats, |steer error| per row (for the percentiles). */
int cilrs_eval_acc_doubles(void);
int cilrs_eval_accumulate(const float* controls, const float* pred_speed,
                          const float* target_controls, const float* target_speed,
                          const int64_t* command, int batch, double* acc, float* steer_abs_err,
                          void* stream);

/* ---- per-kernel timing (hipEvents on the launch stream; feeds bench.py's roofline) ---------- */
int cilrs_net_profile_enable(cilrs_net* net, int on);
/* synchronises the recorded events and folds them into the per-label table */
int cilrs_net_profile_collect(cilrs_net* net);
int cilrs_net_profile_count(const cilrs_net* net);
int cilrs_net_profile_entry(const cilrs_net* net, int i, char* label, int label_cap,
                            long long* calls, double* total_ms, double* total_flops,
                            double* total_bytes);
int cilrs_net_profile_reset(cilrs_net* net);

/* ---- op-level entry points (unit parity tests; same kernels the plan launches) -------------- */
/* nn.Conv2d forward, NHWC x [N,H,W,Cin] (Cin % 4 == 0), OHWI w, y [N,Ho,Wo,Cout] (Cout % 64 == 0)
 * force_cfg: -1 auto, 0/1/2 tile config; force_splitk: 0 auto; scratch may be NULL */
int cilrs_conv2d_fwd(const float* x, const float* w, float* y, int N, int H, int W, int Cin,
                     int Cout, int KH, int KW, int stride, int pad, int force_cfg,
                     int force_splitk, float* scratch, size_t scratch_floats, void* stream);
/* d(loss)/dx of the same conv: dy [N,Ho,Wo,Cout] -> dx [N,H,W,Cin] (+ addend if non-NULL) */
int cilrs_conv2d_dgrad(const float* dy, const float* w, float* dx, const float* addend, int N,
                       int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                       int force_cfg, int force_splitk, float* scratch, size_t scratch_floats,
                       void* stream);
/* The same two calls with the BatchNorm reductions the plan fuses into them (test aids: the plan's
 * own hooks, reachable without a plan).  force_cfg -2: auto, but never the position-class launch.
 * cilrs_conv2d_fwd_stats: partial (>= cilrs_bn_partial_floats(Cout) floats) receives the column
 * partials of y, channel-major [2][Cout][*nblk]: sums and sums of squares over *nblk row groups.
 * cilrs_conv2d_dgrad_bnbwd (stride 1): dx is the output gradient of a BatchNorm layer with raw
 * input bwd_y, output bwd_z (read when bwd_relu) and statistics bwd_stats (mean | rstd), all
 * [N*H*W][Cin]; partial receives [2][Cin][*nblk] partial sums of g and g * xhat, g = dx * (z > 0),
 * xhat = (y - mean) * rstd.  *nblk == 0: the launch chosen does not fuse them. */
int cilrs_conv2d_fwd_stats(const float* x, const float* w, float* y, float* partial, int* nblk,
                           int N, int H, int W, int Cin, int Cout, int K, int stride, int pad,
                           int force_cfg, int force_splitk, float* scratch, size_t scratch_floats,
                           void* stream);
int cilrs_conv2d_dgrad_bnbwd(const float* dy, const float* w, float* dx, const float* addend,
                             const float* bwd_z, const float* bwd_y, const float* bwd_stats,
                             int bwd_relu, float* partial, int* nblk, int N, int H, int W, int Cin,
                             int Cout, int K, int stride, int pad, int force_cfg, int force_splitk,
                             float* scratch, size_t scratch_floats, void* stream);
/* Does the implicit GEMM run this stride-1 convolution (forward, or dgrad != 0: its data gradient)
 * as position classes -- corner / edge / interior rectangles of output positions in one launch,
 * each with only the filter taps that meet the image (csrc/conv_igemm.hip)?  Decided from the
 * shape and the split-K scratch available (force_splitk as in cilrs_conv2d_fwd) alone: padded stride-1 maps whose every class has at
 * least 64 rows, whose blocks fit one round on the chip and whose class launch the kernel cost model prices below the single problem.
 * CILRS_IGEMM_CLASSES=0 in the environment of the process turns the path off (0 here).
 * cilrs_net_conv_classes: the same for convolution `conv` of the plan's train step (numbered as in
 * cilrs_net_activation_info); 0 / 0 for a convolution that does not run on the implicit GEMM. */
int cilrs_conv2d_takes_classes(int N, int H, int W, int Cin, int Cout, int K, int stride, int pad,
                               int dgrad, size_t scratch_floats, int force_splitk);
int cilrs_net_conv_classes(const cilrs_net* net, int conv, int* fwd, int* dgrad);
/* What cilrs_conv2d_fwd (dgrad != 0: cilrs_conv2d_dgrad) would launch for this problem with
 * `scratch_floats` floats of split-K scratch and these force_cfg / force_splitk (test aid: the
 * launchers' own decision code, no launch, no state kept).  *cfg: the tile config (as force_cfg);
 * *splitk: the split count (1: unsplit); *class_tiles: tiles of the position-class launch, 0 for a
 * single problem; *parity_fused, for a stride-2 data gradient: 1 = the four output-parity classes
 * in one launch (*cfg / *splitk are that launch's), 0 = four launches, *cfg / *splitk being those of
 * parity class (0,0) (*cfg -1 if no filter tap reaches that class); -1 when the problem has no
 * parity classes.  The fused hooks of cilrs_conv2d_fwd_stats / _dgrad_bnbwd do not change any of it. */
int cilrs_conv2d_plan_info(int N, int H, int W, int Cin, int Cout, int K, int stride, int pad,
                           int dgrad, size_t scratch_floats, int force_cfg, int force_splitk,
                           int* cfg, int* splitk, int* class_tiles, int* parity_fused);
/* d(loss)/dw (OHWI, Cin_dst channels kept); scratch from cilrs_conv2d_wgrad_scratch_floats */
size_t cilrs_conv2d_wgrad_scratch_floats(int N, int H, int W, int Cin, int Cout, int KH, int KW,
                                         int stride, int pad);
int cilrs_conv2d_wgrad(const float* x, const float* dy, float* dw, float* scratch, int N, int H,
                       int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                       int Cin_dst, void* stream);

/* ---- the same operators on the 16-bit matrix pipe (BASELINE.json configs[3] "bf16 MFMA path",
 * training side): x / w / dy are fp32 tensors as above, rounded to bf16 (bf16 = 1) or fp16
 * (bf16 = 0) into `scratch16` (cilrs_conv2d_16_scratch_halfs() 16-bit elements, 16-byte aligned),
 * multiplied on v_mfma_f32_32x32x16_* with fp32 accumulation; results are fp32.  Cin and Cout
 * multiples of 64, square filters K x K (<= 16 taps), stride 1 or 2.  Not the reference's
 * arithmetic (it trains in fp32): checked against the same product of the ROUNDED operands. */
size_t cilrs_conv2d_16_scratch_halfs(int N, int H, int W, int Cin, int Cout, int K, int stride,
                                     int pad);
/* y = conv(x, w); bn_partial (optional): per-64-row-tile column sums / sums of squares of y,
 * channel-major [2][Cout][ceil(M/64)] */
int cilrs_conv2d_fwd_16(const float* x, const float* w, float* y, float* bn_partial, int N, int H,
                        int W, int Cin, int Cout, int K, int stride, int pad, int bf16,
                        void* scratch16, void* stream);
int cilrs_conv2d_dgrad_16(const float* dy, const float* w, float* dx, const float* addend, int N,
                          int H, int W, int Cin, int Cout, int K, int stride, int pad, int bf16,
                          void* scratch16, void* stream);
size_t cilrs_conv2d_wgrad_16_scratch_floats(int N, int H, int W, int Cin, int Cout, int K,
                                            int stride, int pad);
int cilrs_conv2d_wgrad_16(const float* x, const float* dy, float* dw, float* scratch32, int N,
                          int H, int W, int Cin, int Cout, int K, int stride, int pad, int bf16,
                          void* scratch16, void* stream);

/* BatchNorm backward with fixed statistics when no dgamma / dbeta is wanted (what
 * cilrs_net_backward_data runs on a frozen graph): g = relu ? (z > 0 ? dz : 0) : dz;
 * g_out = g (may be NULL); dy = g * (gamma[c] * stats[C + c]) -- stats = [mean | rstd | ...] as
 * cilrs_bn_eval_fwd leaves it.  [M][C] dense tensors, 16-byte aligned; z may be NULL when relu == 0.
 * C/4 must divide 1024 (the BatchNorm channel counts up to 1024, 2048 and 4096; 3072 is refused).
 * cilrs_bn_bwd_pool_frozen: the stem's form, the backward of maxpool3x3/s2/p1(relu(bn(y))) given
 * d(max-pool output) [N][Ho][Wo][C] and the forward's argmax -- scatter, mask by
 * y * stats[2C + c] + stats[3C + c] > 0, scale; dy [N][H][W][C], every element written. */
int cilrs_bn_bwd_frozen(const float* dz, const float* z, int M, int C, const float* gamma,
                        const float* stats, int relu, float* dy, float* g_out, void* stream);
int cilrs_bn_bwd_pool_frozen(const float* dpool, const uint8_t* argmax, const float* y, int N, int H,
                             int W, int C, const float* gamma, const float* stats, float* dy,
                             void* stream);

/* Heat map of an image gradient (csrc/saliency.hip): dimage = logical NCHW f32 [B,3,H,W] with
 * element strides (sn,sc,sh,sw), e.g. what cilrs_net_input_grads wrote.
 *   s[b,h,w] = max_c |dimage[b,c,h,w]| * chan_scale3[c]   (three HOST floats; NULL = 1)
 *   peak[b]  = max_hw s;   heat = s / peak (0 where peak == 0, never NaN) -- f32 [B,H,W];
 *   heat_u8  = floor(heat * 255 + 0.5) -- uint8 [B,H,W].    heat_u8 and peak may be NULL.
 * One launch, one workgroup per frame, fixed-order reduction: bit-identical from run to run. */
int cilrs_saliency_map(const float* dimage, long sn, long sc, long sh, long sw, int B, int H, int W,
                       const float* chan_scale3, float* heat, uint8_t* heat_u8, float* peak,
                       void* stream);

/* SmoothGrad and integrated gradients around that pass (csrc/attribution.hip; Predictor.attribution
 * drives them): S samples per frame go through cilrs_net_forward_frozen + cilrs_net_backward_data +
 * cilrs_net_input_grads a chunk at a time, and these three launches keep every sample on the
 * device.  Streaming kernels, no atomics, every sum in a fixed order, every float operation
 * rounded once (no FMA contraction): each result is the torch fp32 expression bit for bit.
 *
 * cilrs_attr_samples: frames_u8 uint8 [B,H,W,3] -> out f32 contiguous NCHW [B*s_count,3,H,W];
 *   row b*s_count + j is global sample s = s_begin + j of frame b (a frame's samples are adjacent).
 *   With c the 8-bit value as a float and m, d the channel's mean / std:
 *     CILRS_ATTR_SMOOTHGRAD   v = c + sigma255 * n   (no clipping, no rounding: the noise is on the
 *       network input, not on the camera); n = sqrtf(-2 logf u1) * cosf(2 pi u2), u1 / u2 the
 *       24-bit fields of splitmix64(seed + counter * 0xD1B54A32D192ED03) exactly as the GaussNoise
 *       of cilrs_augment_u8 extracts them, counter = (b*S + s)*3HW + (y*W + x)*3 + k: keyed on the
 *       global sample index, so a sample is the same whichever chunk produces it.
 *     CILRS_ATTR_INTEGRATED   v = c0 + alpha_s * (c - c0), c0 the baseline_u8 pixel (NULL: 0, a
 *       black frame), alpha_s = ((float)s + 0.5f) / (float)S  (midpoint rule).
 *   out = (v / 255 - m) / d.  sigma255 = 0, or alpha = 1, is the preprocessing of
 *   cilrs_net_forward_u8 bit for bit.  Refused: NULL tensors, S < 1, a chunk outside [0, S), a
 *   negative or non-finite sigma255, 3*H*W*B*S >= 2^63.
 * cilrs_attr_accumulate: dimage = logical f32 [B*s_count,3,H,W] with non-negative element strides
 *   (what cilrs_net_input_grads wrote for the chunk), acc f32 contiguous [B,3,H,W].  Per element
 *   a = first ? +0 : acc;  a = a + g_j for j = 0 .. s_count-1 in that order;  acc = a -- one
 *   sequential chain, so any split of the S samples into chunks gives the same bits.
 * cilrs_attr_finalize: invS = 1 / (float)S.
 *     SMOOTHGRAD  attr = acc * invS   (chan_scale3, frames_u8, baseline_u8 unused, may be NULL)
 *     INTEGRATED  attr_c = (acc_c * invS) * ((float)(c - c0) * chan_scale3[c]); chan_scale3 = three
 *       HOST floats, 1 / (255 * std_c) for attributions in the network's input units
 *   attr f32 [B,3,H,W]; signed_map (may be NULL) f32 [B,H,W] = (attr_0 + attr_1) + attr_2;
 *   total (may be NULL) f32 [B] = the frame's sum of signed_map, one workgroup of
 *   cilrs_attr_finalize_threads() threads per frame: per-thread chain, wave shuffles, LDS. */
#define CILRS_ATTR_SMOOTHGRAD 0
#define CILRS_ATTR_INTEGRATED 1
int cilrs_attr_samples(const uint8_t* frames_u8, const uint8_t* baseline_u8, int B, int H, int W,
                       int mode, int S, int s_begin, int s_count, float sigma255, uint64_t seed,
                       float* out, void* stream);
int cilrs_attr_accumulate(const float* dimage, long sn, long sc, long sh, long sw, int B, int s_count,
                          int H, int W, int first, float* acc, void* stream);
int cilrs_attr_finalize(const float* acc, const uint8_t* frames_u8, const uint8_t* baseline_u8, int B,
                        int H, int W, int mode, int S, const float* chan_scale3, float* attr,
                        float* signed_map, float* total, void* stream);
int cilrs_attr_finalize_threads(void);

/* Adversarial robustness (csrc/adversarial.hip; Predictor.adversarial, evaluate.adversarial_sweep
 * and the adversarial train step of Trainer drive them): FGSM / PGD on the network's input.  The
 * gradient of an iteration is a forward + cilrs_net_backward_data + cilrs_net_input_grads; these
 * four launches are everything in between.  Streaming kernels, no atomics, every float operation
 * rounded once (no FMA contraction): each result is the fp32 numpy expression bit for bit, and
 * bit-identical from run to run.
 *
 * x = the clean normalised image, x_adv = the iterate, g = the image gradient, best = the kept
 * iterate: logical NCHW f32 [B,3,H,W] with non-negative element strides (sn,sc,sh,sw).  Contiguous
 * NCHW and the channels-last view with strides (3HW, 1, 3W, 3) move 16 bytes per access when every
 * tensor of the call has that layout, H*W % 4 == 0 and the pointers are 16-byte aligned; anything
 * else goes element by element through the strides, with the same results.
 * Sizes are in 8-bit levels: chan_scale3 = three HOST floats, 1 / (255 * std_c) as for
 * cilrs_attr_finalize; e_c = eps255 * chan_scale3[c] and a_c = alpha255 * chan_scale3[c], one fp32
 * product each, formed on the host.  range6 (HOST floats lo_0, hi_0, lo_1, hi_1, lo_2, hi_2; may be
 * NULL) = the images of the bytes 0 and 255 under the preprocessing.
 *   clamp(t) = fminf(fmaxf(t, x - e_c), x + e_c), then, with range6,
 *              fminf(fmaxf(t, lo_c), hi_c)                 (fminf / fmaxf drop a NaN operand)
 *
 * cilrs_adv_start: x_adv = clamp(x + e_c * r), r = (u + u) - 1, u = ((float)(h >> 40) + 1) * 2^-24
 *   with h = splitmix64(seed + counter * 0xD1B54A32D192ED03) -- the first 24-bit field exactly as
 *   cilrs_attr_samples takes u1 -- and counter = the element's LOGICAL index ((b*3 + c)*H + y)*W + x:
 *   the draw does not depend on the strides.  x and x_adv have strides of their own.  eps255 = 0 is a
 *   copy, bit for bit (no draw, no clamp).
 * cilrs_adv_step (x and x_adv share one set of strides; g and best have their own), per element, in
 *   this order:
 *     1. improved != NULL, best != NULL and improved[b] != 0:  best = x_adv  (the iterate the last
 *        forward saw: the value BEFORE this step)
 *     2. s = g > 0 ? 1 : (g < 0 ? -1 : 0)                      (NaN: 0)
 *     3. t = x_adv + (a_c * d_b) * s,  d_b = row_dir ? row_dir[b] : 1
 *     4. x_adv = clamp(t)
 *   alpha255 = 0: only step 1 runs and x_adv is not written -- every bit of it stays; g may be NULL
 *   then, and only then.  With nothing to copy either, nothing is launched.
 * cilrs_adv_direction: one thread per frame.  w4_host = four HOST floats over (steer, throttle,
 *   brake, pred_speed); controls / ref_controls f32 [B,3], pred_speed / ref_speed f32 [B];
 *     dev[b] = (w0*(c0-r0) + w1*(c1-r1)) + (w2*(c2-r2) + w3*(s-rs))       in that association
 *     row_dir[b]  (f32) = dev >= 0 ? +1 : -1           -- ascends |dev|
 *     improved[b] (i32) = first || |dev| > |best_dev[b]|;  where improved, best_dev[b] = dev
 *   A non-finite dev never improves (not even with `first`; best_dev[b] is then set to 0) and gives
 *   row_dir = +1.  ref = the clean prediction ("deviate") or the labels ("error").
 * cilrs_adv_quantize: the iterate as a camera frame.  v = (x_adv * std_c + mean_c) * 255,
 *   q = (uint8) rintf(fminf(fmaxf(v, 0), 255))  (NaN: 0) -> out_u8 uint8 [B,H,W,3];  linf (i32 [B],
 *   may be NULL; needs frames_u8 uint8 [B,H,W,3]) = max |q - frame| over the frame: one workgroup of
 *   cilrs_adv_quantize_threads() threads per frame, per-thread maximum, wave shuffles, LDS --
 *   integers, so the result is exact.
 *
 * Refused (non-zero, text in cilrs_last_error, nothing launched): NULL tensors (the optional ones
 * are exempt); a negative or non-finite eps255 / alpha255; a negative stride; B, H or W < 1 or
 * B*3*H*W > cilrs_adv_max_elements() = 2^30 (element indices are ints in the kernels);
 * g == NULL with alpha255 > 0; linf without frames_u8. */
int cilrs_adv_start(const float* x, long xn, long xc, long xh, long xw, int B, int H, int W,
                    float eps255, const float* chan_scale3, uint64_t seed, const float* range6,
                    float* x_adv, long an, long ac, long ah, long aw, void* stream);
int cilrs_adv_step(const float* x, float* x_adv, long sn, long sc, long sh, long sw, const float* g,
                   long gn, long gc, long gh, long gw, int B, int H, int W, float alpha255,
                   float eps255, const float* chan_scale3, const float* row_dir,
                   const int32_t* improved, float* best, long bn, long bc, long bh, long bw,
                   const float* range6, void* stream);
int cilrs_adv_direction(const float* controls, const float* pred_speed, const float* ref_controls,
                        const float* ref_speed, const float* w4_host, int B, int first, float* dev,
                        float* best_dev, float* row_dir, int32_t* improved, void* stream);
int cilrs_adv_quantize(const float* x_adv, long sn, long sc, long sh, long sw,
                       const uint8_t* frames_u8, int B, int H, int W, uint8_t* out_u8, int32_t* linf,
                       void* stream);
int cilrs_adv_quantize_threads(void);
long long cilrs_adv_max_elements(void);

/* The bf16 training mode's operators on 16-bit tensors (round 4: every trunk tensor after the stem
 * -- activations, raw convolution outputs, gradients -- is stored in bf16; fp32 accumulation,
 * statistics and coefficients).  No reference counterpart (the reference trains in fp32,
 * notebook/notebook.ipynb:549-555); defined by oracle/bf16_emulation.py.
 *
 * cilrs_conv2d_train_16: implicit-GEMM convolution of the 16-bit NHWC tensor x16 [N][H][W][Cin] with
 * 16-bit weights w16 [Cout][K][K][Cin] over the output grid [N][Ho][Wo] (forward: the OHWI weights
 * rounded; data gradient: x16 = dy, w16 = the transposed, tap-flipped weights, pad = K-1-pad_fwd,
 * or up2 = 1 with stride 2 for the gradient of a stride-2 convolution).  Result = acc (+ addend16),
 * ROUNDED to 16 bits into y16, or fp32 into y32 when y16 is NULL.  bn_partial (optional):
 * BatchNorm batch statistics of the stored result as column partials [2][Cout][rows];
 * bwd_partial (optional, with bwd_z16 / bwd_y16 / bwd_stats): BatchNorm-backward reductions of the
 * produced gradient, g = result * (z > 0 if bwd_relu), partials of g and g * xhat.  *partial_rows
 * receives the number of partial rows (the launch's 64- or 128-row tiles). */
int cilrs_conv2d_train_16(const void* x16, const void* w16, void* y16, float* y32,
                          const void* addend16, float* bn_partial, const void* bwd_z16,
                          const void* bwd_y16, const float* bwd_stats, int bwd_relu,
                          float* bwd_partial, int N, int H, int W, int Cin, int Ho, int Wo, int Cout,
                          int K, int stride, int pad, int up2, int bf16, int* partial_rows,
                          void* stream);
/* The 16-bit INFERENCE trunk's operators, op by op (what cilrs_net_forward_u8_f16 / _bf16 launch;
 * bf16 = 0: fp16 tensors, 1: bf16).  No reference counterpart; defined by
 * oracle/infer16_emulation.py.  All 16-bit tensors NHWC, 16-byte aligned.
 *
 * cilrs_conv2d_infer_16: y16 = round(relu?((acc + bias[co]) + residual16)), acc = fp32 sum of the
 * products of x16 [N][H][W][Cin] and the folded weights w16 [Cout][K][K][Cin]; residual16 (y16's
 * layout) may be NULL.  Cin, Cout multiples of 64, K x K <= 16 taps.  tile: 0 = the 64x64 tile every
 * plan uses, 128 = the 128x128 instantiation (Cout % 128 == 0).
 * cilrs_stem_fold_16: w16 [64][7][8][4] = round(w[64][7][7][3] * stats[128 + co]) (zero padding),
 * bias[co] = stats[192 + co]; stats = the eval-mode BatchNorm table [mean | rstd | scale | shift].
 * cilrs_stem_infer_16: z16 [N][Ho][Wo][64] = round(relu(conv7x7/s2/p3(round(x4), w16) + bias)) from
 * the channel-padded fp32 image x4 [N][H][W][4].
 * cilrs_maxpool_infer_16: MaxPool2d(3, 2, 1) of a 16-bit tensor (C % 8 == 0).
 * cilrs_avgpool_infer_16: out[n * out_ld + c] = fp32 mean over the HW pixels of x16 [N][HW][C]. */
int cilrs_conv2d_infer_16(const void* x16, const void* w16, const float* bias,
                          const void* residual16, void* y16, int N, int H, int W, int Cin, int Cout,
                          int K, int stride, int pad, int relu, int bf16, int tile, void* stream);
int cilrs_stem_fold_16(const float* w, const float* stats, void* w16, float* bias, int bf16,
                       void* stream);
int cilrs_stem_infer_16(const float* x4, const void* w16, const float* bias, void* z16, int N, int H,
                        int W, int bf16, void* stream);
int cilrs_maxpool_infer_16(const void* x16, void* out16, int N, int H, int W, int C, int bf16,
                           void* stream);
int cilrs_avgpool_infer_16(const void* x16, float* out, int N, int HW, int C, int out_ld, int bf16,
                           void* stream);
/* BatchNorm2d (training) on bf16 NHWC tensors: statistics of y16 (from `partial` when pre_rows > 0:
 * rows written by cilrs_conv2d_train_16), z16 = round(relu?(bn(y16) (+ residual16))); and its
 * backward: dy16 = round(BatchNorm backward of g = dz16 * (z16 > 0 if relu)), g_out16 = g.
 * Semantics of cilrs_bn_train_fwd / cilrs_bn_bwd otherwise (nn.BatchNorm2d, nb:440-477). */
int cilrs_bn16_train_fwd(const void* y16, int M, int C, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, int64_t* nbt, float momentum,
                         float eps, const void* residual16, int relu, float* stats, float* partial,
                         void* z16, int pre_rows, void* stream);
int cilrs_bn16_bwd(const void* dz16, const void* z16, const void* y16, int M, int C,
                   const float* gamma, const float* stats, int relu, float* dgamma, float* dbeta,
                   float* coef3c, float* partial, void* dy16, void* g_out16, int pre_rows,
                   void* stream);
/* nn.BatchNorm2d training forward (+ optional residual add, ReLU); stats: 4*C floats out */
/* The same 3x3 / stride 1 / pad 1 convolution (nn.Conv2d(C, K, 3, 1, 1, bias=False) of
 * torchvision's BasicBlock: conv1 of every non-first block and every conv2) and its data gradient
 * by Winograd F(2x2, 3x3) on the fp32 matrix pipe: 16 multiplications per 2x2 output tile and
 * channel instead of 36.  fp32 throughout; results differ from the direct sum by rounding
 * (a few 1e-6 relative).  w: OHWI like everywhere; scratch: transformed filters,
 * cilrs_conv2d_wino_scratch_floats(Cin, Cout) floats.  Cin %% 8 == 0, Cout %% 64 == 0 (dgrad: the
 * roles swap). */
size_t cilrs_conv2d_wino_scratch_floats(int Cin, int Cout);
int cilrs_conv2d_wino_fwd(const float* x, const float* w, float* y, int N, int H, int W, int Cin,
                          int Cout, float* scratch, void* stream);
/* The forward form with an eval-mode BatchNorm folded into the epilogue (the frozen prefix of
 * cilrs_net_forward_ft): y = relu_post?(relu?(conv(x, w) * scale[k] + shift[k]) + addend); addend
 * (y's layout) may be NULL; scale / shift: Cout floats, 16-byte aligned. */
int cilrs_conv2d_wino_fold_fwd(const float* x, const float* w, float* y, const float* scale,
                               const float* shift, const float* addend, int relu, int relu_post,
                               int N, int H, int W, int Cin, int Cout, float* scratch, void* stream);
/* the two halves on their own: U = transformed filters ([16][Cred/8][Cout][8]; dgrad = 1: the
 * data gradient's filter, reduction over the forward Cout), and the convolution on a ready U */
int cilrs_wino_filter_transform(const float* w, float* U, int Cin, int Cout, int dgrad, void* stream);
/* diagnostics: 16 int64 device words that block 0's waves 0 and 4 of every later
 * cilrs_conv2d_wino_pre launch fill with shader-cycle counts [prologue, multiply, refill, barrier
 * wait, epilogue, K loop] (NULL: off) */
int cilrs_conv2d_wino_stamps(long long* stamps16);
int cilrs_conv2d_wino_pre(const float* x, const float* U, float* y, const float* addend, int N, int H,
                          int W, int Cred, int Cout, void* stream);
/* cilrs_conv2d_wino_pre with the launch plan of the train step: an under-filled launch (fewer 64-tile
 * x 64-channel blocks than CUs: layer3 at B=128) is cut along the reduction over the Cred input
 * channels into up to four parts per tile, each part writes a slab, and a fixed-order reduce sums
 * them, adds the addend and emits the BatchNorm column partials [2][Cout][*partial_rows].
 * slabs: scratch of slab_floats floats; *csplit = parts per tile the launch used (1: not split). */
int cilrs_conv2d_wino_split(const float* x, const float* U, float* y, const float* addend,
                            float* bn_partial, int N, int H, int W, int Cred, int Cout, float* slabs,
                            size_t slab_floats, int* csplit, int* partial_rows, void* stream);
int cilrs_conv2d_wino_dgrad(const float* dy, const float* w, float* dx, const float* addend, int N,
                            int H, int W, int Cin, int Cout, float* scratch, void* stream);
/* Weight gradient of the same convolution in the Winograd domain (cuDNN conv bwd-filter, i.e. the
 * `loss.backward()` of notebook/notebook.ipynb:551 for a 3x3 / stride-1 layer): dw[Cout][3][3][Cin]
 * from x[N][H][W][Cin] and dy[N][H][W][Cout]; Cin % 64 == 0, Cout % 64 == 0.  scratch:
 * cilrs_conv2d_wino_wgrad_scratch_floats floats (per-split slabs, summed in fixed order). */
size_t cilrs_conv2d_wino_wgrad_scratch_floats(int N, int H, int W, int Cin, int Cout);
int cilrs_conv2d_wino_wgrad(const float* x, const float* dy, float* dw, int N, int H, int W, int Cin,
                            int Cout, float* scratch, size_t scratch_floats, void* stream);
size_t cilrs_bn_partial_floats(int C);
int cilrs_bn_train_fwd(const float* y, int M, int C, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, int64_t* nbt, float momentum,
                       float eps, const float* residual, int relu, float* stats, float* partial,
                       float* z, void* stream);
int cilrs_bn_eval_fwd(const float* y, int M, int C, const float* gamma, const float* beta,
                      const float* running_mean, const float* running_var, float eps,
                      const float* residual, int relu, float* stats, float* z, void* stream);
int cilrs_bn_bwd(const float* dz, const float* z, const float* y, int M, int C,
                 const float* gamma, const float* stats, int relu, float* dgamma, float* dbeta,
                 float* coef3c, float* partial, float* dy, float* g_out, void* stream);
/* nn.Linear forward  y = relu?(x W^T + b)  and backward (autonomous_drive.py:371-387; the heads'
 * grouped kernels with one group): x [batch][in] (row pitch x_ld), w [out][in], y [batch][out].
 * backward: dw [out][in] = dy^T x, db [out] = column sums of dy (either may be NULL together),
 * dx [batch][in] = (dy W), kept where act > 0 and multiplied by act_scale when act != NULL. */
int cilrs_linear_fwd(const float* x, const float* w, const float* bias, float* y, int batch,
                     int in_features, int out_features, int x_ld, int y_ld, int relu,
                     void* stream);
int cilrs_linear_bwd(const float* dy, const float* x, const float* w, const float* act,
                     float act_scale, float* dx, float* dw, float* db, int batch,
                     int in_features, int out_features, int dy_ld, int x_ld, int dx_ld,
                     int act_ld, void* stream);
int cilrs_maxpool_fwd(const float* x, float* out, uint8_t* argmax, int N, int H, int W, int C,
                      void* stream);
int cilrs_maxpool_bwd(const float* dout, const uint8_t* argmax, float* dx, int N, int H, int W,
                      int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CILRS_HIP_H */
