// Model handle internals (host side).  Not part of the public ABI.
#pragma once
#include "../../include/sykepic_hip.h"
#include "spk_common.h"

#include <string>
#include <unordered_map>
#include <vector>

enum ParamKind { PK_CONV_W = 1, PK_BN_W, PK_BN_B, PK_BN_MEAN, PK_BN_VAR, PK_BN_NBT, PK_FC_W, PK_FC_B,
                 PK_SE_W, PK_SE_B };

struct Param {
  std::string key;
  int kind = 0, layer = -1, dtype = 0, ndim = 0;
  int64_t shape[4] = {1, 1, 1, 1};
  int64_t numel = 0;
  bool trainable = false;  // nn.Parameter (true) vs buffer (false)
  int requires_grad = 0;
  int group = -1;          // optimizer param group, -1: not in the optimizer
  size_t off = 0;          // element offset in the flat fp32 buffers
  long step = 0;           // per-tensor step count (torch keeps it per parameter)
  double mu_product = 1.0; // NAdam: running product of the momentum schedule
};

struct TDim {
  int h = 0, w = 0, c = 0;  // c: channels as laid out (padded to 64 for EfficientNet widths)
  bool bf16 = true;
  int c_log = 0;            // logical channels (0: same as c)
};

struct Layer {
  spk_layer_desc d;
  int mode = 0;     // CONV_MODE_*
  int groups = 1;   // Conv2d groups (> 1: CONV_MODE_GROUP, weights [cout][cin / groups][k][k])
  int kpad = 0;     // GEMM K of the packed weights
  int p_w = -1, p_g = -1, p_b = -1, p_mean = -1, p_var = -1, p_nbt = -1;
  int p_w2 = -1, p_b2 = -1;       // SE: fc2 (p_w / p_b hold fc1)
  int cin_p = 0, cout_p = 0;      // channels as laid out in HBM: padded to a multiple of 64 (zeros)
  size_t wpack_off = 0, sb_off = 0;
  size_t wpw_off = 0;             // fragment-ordered image of a 1x1 conv's weights (conv_pw.hip), when pw_ok
  bool pw_ok = false;             // 1x1, stride 1 or 2, no padding anywhere, channels multiples of 64
  bool c3_ok = false;             // 3x3 stride 1 pad 1, cin % 64 == 0, cout % 256 == 0: conv_c3.hip (image at wpw_off)
  bool d3_ok = false;             // 3x3 stride 1 pad 1, cin = cout = 64: conv_d3.hip (image at wd3_off)
  size_t wd3_off = 0;             // its [cout][9 cin] weights in conv_pw.hip's fragment order
  // eval: a block-closing 1x1 conv and the 1x1 shortcut (downsample) conv of its block as ONE K-concatenated GEMM
  // (conv_pw.hip, PwConvArgs::x2): the shortcut tensor is neither written nor re-read
  int dual_src = -1;              // block-closing conv: index of the shortcut conv it absorbs, or -1
  int fused_into = -1;            // shortcut conv: index of the block-closing conv that absorbs it, or -1
  bool dual_ok = false;           // images packed for the current precision settings (spk_commit)
  size_t wdual_off = 0;           // fragment-ordered concatenated weights (elements into spk_model::wdual)
  size_t sdual_off = 0;           // [2^e per cout][summed shifts] (floats into spk_model::sdual)
  // eval, single-weight modes: a block-closing 1x1 conv (256 couts) and the 1x1 conv of the NEXT block that reads its
  // output, as one kernel (conv_pw.hip, PwConvArgs::wpz): the trunk is written but not re-read by that conv
  int chain_next = -1;            // block-closing conv: index of the conv it can also compute, or -1
  int chained_by = -1;            // that conv: index of the block-closing conv
  // eval, single-weight modes: a whole identity bottleneck block - conv1 1x1 -> conv2 3x3 -> conv3 1x1 + shortcut, ReLU behind
  // each BatchNorm - as ONE kernel (conv_bneck.hip): the two mid tensors are never written.  (Or conv2's launch also
  // computes conv3 + shortcut (+ the chained conv): conv_btail_kernel.)  Which form ran: EvalCarry::ran
  int bn_c2 = -1, bn_c3 = -1;     // the block's conv1: indices of its conv2 / conv3, or -1
  int bn_head = -1;               // conv2 / conv3 of such a block: index of its conv1
  size_t mu_off = 0;              // generic convs: offset of this layer's cin input-channel means in spk_model::act_mean
  // fp16 eval of an MBConv block: the squeeze-excitation layer computes its gates only and the project 1x1 conv that is
  // the sole reader of its output multiplies them into its activation operand (conv_igemm.hip, spk_set_gate)
  int gate_conv = -1;             // squeeze-excitation layer: index of that conv, or -1
  int gate_from = -1;             // that conv: index of the squeeze-excitation layer
  // producers and readers the executor needs at a launch (resolved once, spk_graph_build; -1: none)
  int se_dw = -1;                 // squeeze-excitation layer: the depthwise conv that writes its input (and leaves the pool partials)
  int src_se = -1;                // conv: the squeeze-excitation layer that writes its input
  int exp_next = -1;              // conv: the first expand-shaped 1x1 conv that reads its output (fp8: gets the trunk's e4m3 shadow)
  int64_t nbt = 0;  // num_batches_tracked (host copy; exact int64)
  bool trunk_writer = false;  // output is (or is added to) the residual trunk: stem, block-closing conv, downsample
  bool inner3x3 = false;      // 3x3 conv in the middle of a bottleneck block (reads a 1x1 conv's output)
  // fp8 mode of the MBConv interior (spk_model_set_fp8): role of this layer and what calibration measured
  int fp8_role = 0;           // 0 none, 1 expand conv (fp16 in, e4m3 out), 2 depthwise (e4m3 in/out), 3 squeeze-excitation
                              // (gates only), 4 project conv (e4m3 in x gate, fp16 out)
  float amax_in = 0.f, amax_out = 0.f;   // max |x| of the input / output tensor on the calibration batch
  size_t w8_off = 0, s8_off = 0;         // e4m3 weights / [ws, epilogue scale] floats of this layer
  bool side_branch = false;   // output is only ever a shortcut operand (downsample conv): what the block-closing conv can absorb
  int fuse_pool = -1;         // stem conv: index of the 3x3/2 max-pool layer its eval kernel can absorb (conv_stem.hip), or -1
  bool pooled_by_stem = false;  // that max-pool layer
};

// What the eval forward did with one layer (EvalCarry::ran) - the ONE place that says which launch computed a layer and
// whether its output tensor is in the arena; the cases, one by one: DESIGN.md section 1.  form: EF_OWN plus what else its
// launch did, or EF_INSIDE the launch of layer `by` (EF_NONE: has not run in this forward); wrote: the output tensor was
// written.  A layer that finds itself EF_INSIDE when its turn comes has nothing left to do.
enum EvalForm : uint8_t { EF_NONE = 0, EF_OWN = 1, EF_POOL = 2, EF_DUAL = 4, EF_CHAIN = 8, EF_BNECK = 16, EF_BTAIL = 32, EF_GATES = 64, EF_INSIDE = 128 };
struct EvalRan { uint8_t form = EF_NONE; bool wrote = false; int by = -1; };
// The fusions a call of the executor may use, and whether the call is the forward itself.  The tuners time their "two
// kernels" / "three launches" alternatives with the fusion under test (and EVAL_FORWARD) taken out, a read-back recomputes
// with 0: only the forward consults and writes EvalCarry::ran.
enum : unsigned { FUSE_POOL = 1, FUSE_DUAL = 2, FUSE_CHAIN = 4, FUSE_BNECK = 8, FUSE_BTAIL = 16, FUSE_GATE = 32, FUSE_ALL = 63, EVAL_FORWARD = 64 };

// which images of the planned batch a call of the executor works on, and where its launches go
struct EvalCursor { int half = 0, img0 = 0, n = 0; hipStream_t stream = nullptr; };
// what one layer leaves for the next one of ITS chain, and what the chain's forward did with each layer
struct EvalCarry {
  int dw_chunks = 0;            // pool-partial rows per image the depthwise layer that ran last wrote
  const float* gate = nullptr;  // gates of the squeeze-excitation op that ran last (consumed by the project conv)
  int gate_stride = 0;
  int shadow_t = -1;            // fp8 mode: tensor id whose e4m3 copy the last project conv left (-1: none valid)
  int shadow_stride = 0;        // ... and its row stride in bytes
  std::vector<EvalRan> ran;     // per layer: what the last eval forward did with it.  Cleared by spk_eval_begin
};

struct TrainState;

struct spk_model {
  int device = 0;
  int in_chans = 3, num_classes = 0;
  hipStream_t stream = nullptr;
  // eval: the two halves of a batch on two streams (see spk_forward_eval_logits)
  hipStream_t half_stream = nullptr;
  hipEvent_t half_fork = nullptr, half_join = nullptr;
  std::vector<long long> half_warm;   // (n, h, w) keys whose half-batch kernels have been tuned (on a quiet GPU)
  std::vector<Layer> layers;
  std::vector<Param> params;
  std::unordered_map<std::string, int> index;
  int n_tensors = 1;

  float* pbuf = nullptr;       // flat fp32 master parameters + buffers
  size_t n_flat = 0, n_train = 0;
  size_t n_wpack = 0, n_sb = 0, n_dwp = 0, n_wdual = 0, n_sdual = 0;   // elements of the packed images below (spk_graph_build)
  // exponential moving average of pbuf (spk_model_ema_*): a second flat buffer in pbuf's layout, null while off
  float* ema = nullptr;
  bool ema_swapped = false;    // the CONTENTS of pbuf and ema are exchanged: pbuf holds the average, no training step runs
  bf16_t* wpack = nullptr;     // bf16 conv weights, [Cout][K] per layer
  float* scale_bias = nullptr; // eval-BN folded scale/bias per conv
  float* dwpack = nullptr;     // fp32 tap-major weights of depthwise / 3x3-stem layers (EfficientNet)
  bf16_t* wdual = nullptr;     // K-concatenated weight images of the fused (block-closing + shortcut) convs
  float* sdual = nullptr;      // their epilogue factors
  bool fuse_ds = true;         // SPK_FUSE_DS=0 turns the fusion off
  bool fuse_se = true;         // fp16 eval: squeeze-excitation scaling inside the project conv (SPK_SE_FUSE=0: its own pass)
  int chain = 1;               // conv3 -> next conv1 chaining: 1 where it is faster (timed once per problem), SPK_CHAIN=0 never, 2 always
  int bneck = 1;               // whole-bottleneck kernel: 1 where it is faster (rule + timing: bneck_choice), SPK_BNECK=0 never, 2 always
                               // (14-row blocks), 3 always (7-row blocks)
  int btail = 0;              // conv2 + conv3 (+ chained conv) kernel on the stage the whole-block kernel does not take: off - it is
                               // bit-identical but no faster than the launches it replaces; SPK_BTAIL=1
  EvalCarry carry[2];          // the two half-batch chains of the eval forward (index = EvalCursor::half; a single-stream
                               // forward leaves chain 1's record at EF_NONE)
  bool effnet = false;         // EfficientNet graph (widths that are not multiples of 64, depthwise / SE / SiLU ops): its
                               // TRAINING plan pads every activation tensor to a multiple of 64 channels (train_effnet.hip)
  bool mobilenet = false;      // MobileNetV3 arithmetic (a Hardswish layer or a ReLU / Hardsigmoid squeeze-excitation gate):
                               // an MBConv graph that the fp8 mode (SiLU-only kernels, pw_fp8.hip) does not cover
  bool plan_pad = false;       // the current activation plan is the channel-padded one
  size_t se_off = 0;           // arena offset of the squeeze-excitation scratch (partials + scales)
  bool dirty = true;
  int infer_dt = DT_F16;       // 16-bit storage type of the eval path
  int packed_dt = -1;          // dtype the packed weights currently hold
  int packed_split = -1;
  int splitw = 3;              // eval: hi+lo fp16 weights. 0 none, 1 every conv, 2 trunk writers only, 3 all but inner 3x3 (default), 4 per-op mask,
                               // 5 calibrated single pass: the stem only, every other conv zero-sum rounded (zero_sum.hip)
  // zero-sum rounding of the un-split fp16 weights against per-channel activation means (spk_model_calibrate_act_means)
  bool zero_sum = false;       // explicit switch (spk_model_set_zero_sum); splitw == 5 implies it
  bool have_means = false;
  size_t n_means = 0;          // sum of cin over the generic convs
  std::vector<float> act_mean; // host copy, graph order
  float* act_mean_dev = nullptr;
  std::vector<double> cal_sum; // calibration accumulators: sum over rows per channel ...
  std::vector<double> cal_rows;  // ... and rows seen, per generic conv (graph order)
  int packed_zs = -1;
  std::vector<unsigned char> split_mask;  // splitw == 4: one flag per graph op
  int split_epoch = 0, packed_epoch = -1;  // bumps when the mask changes
  int act_dt = DT_F16;         // dtype of the activations now in the arena

  // activations of one (n,h,w) plan
  void* arena = nullptr;
  size_t arena_bytes = 0;
  int cap_n = 0, cap_h = 0, cap_w = 0;
  int mb_limit = 1;
  std::vector<TDim> tdims;
  std::vector<size_t> toff;
  std::vector<size_t> toff_lo;  // 0 = no remainder tensor
  bool precise_res = false;     // keep the 16-bit rounding remainder of shortcut tensors
  size_t logits_off = 0;

  // fp8 (e4m3) eval mode of the EfficientNet MBConv interior — BASELINE config 5
  int fp8 = 0;                  // requested
  bool fp8_calibrated = false;  // roles assigned + activation ranges measured
  bool fp8_packed = false;
  std::vector<unsigned char> fp8_blocks;   // per qualifying MBConv block (graph order): on the e4m3 path?  empty: all
  unsigned char* w8pack = nullptr;
  float* s8 = nullptr;
  unsigned char* fp8_shadow = nullptr;  // fp8 mode: e4m3 copy of the trunk tensor the last project conv wrote (pw_fp8.hip)
  size_t fp8_shadow_bytes = 0;
  size_t fp8_shadow_img = 0;            // bytes per image of the shadow: the largest h * w * stride of any shadowed tensor; a chunk
                                        // [img0, ...) starts at img0 * fp8_shadow_img in every block (disjoint slices per half-batch)
                                        // (0: this forward leaves no copy)
  size_t se_stride = 0;              // floats of squeeze-excitation scratch per image (the halves use disjoint slices)
  std::vector<float> t_fp8_scale;    // per tensor: 0 = 16-bit storage, else value = byte * scale

  // data-parallel overlap (spk_model_set_grad_ready_callback)
  spk_grad_ready_fn grad_cb = nullptr;
  void* grad_cb_user = nullptr;
  hipStream_t comm_stream = nullptr;
  int grad_buckets = 0;
  hipEvent_t grad_ev[3] = {nullptr, nullptr, nullptr};

  // the loss of spk_train_forward_backward and spk_eval_step (spk_model_set_loss): with neither weights nor smoothing
  // the steps launch the plain instantiation of ce_loss_kernel (CeArgs::plain), otherwise the weighted one, which also
  // fills the per-class counters
  float* loss_w = nullptr;      // class weights [num_classes] on the device, or null
  float loss_eps = 0.f;         // label smoothing
  int* class_counts = nullptr;  // int32 [num_classes][2] on the device: (rows seen, rows correct) since the last reset
  bool loss_ex() const { return loss_w != nullptr || loss_eps > 0.f; }

  uint64_t seed = 0;
  float bn_eps = 1e-5f, bn_momentum = 0.1f;   // BatchNorm2d(eps, momentum) of the graph (spk_model_set_bn)
  TrainState* train = nullptr;

  bool fuse_stem_pool = true;   // eval: stem conv + max-pool in one kernel (SPK_FUSE_STEM_POOL=0 turns it off)
  int last_eval_nb = 0;         // images of the last eval micro-batch (read_activation recomputes a tensor it did not write)
  float* P(int pi) const { return pbuf + params[pi].off; }
  void* T(int t) const { return (char*)arena + toff[t]; }
  // tensor t from the cursor's first image on
  void* TI(const EvalCursor& c, int t) const {
    const TDim& d = tdims[t];
    return (char*)arena + toff[t] + (size_t)c.img0 * d.h * d.w * d.c * (d.bf16 ? 2 : 4);
  }
  // ... when it holds e4m3 bytes (fp8 mode: one byte per element in a slot sized for two)
  void* TI8(const EvalCursor& c, int t) const {
    const TDim& d = tdims[t];
    return (char*)arena + toff[t] + (size_t)c.img0 * d.h * d.w * d.c;
  }
  // squeeze-excitation scratch of the cursor's images
  float* SE(const EvalCursor& c) const { return (float*)((char*)arena + se_off) + (size_t)c.img0 * se_stride; }
  void* TLo(int t) const { return toff_lo[t] ? (char*)arena + toff_lo[t] : nullptr; }
};

void spk_set_error(const std::string& s);
#define SPK_LOCAL __attribute__((visibility("hidden")))   // shared between the model_*.hip files, not a symbol of the library
// the one error helper of the host code: records msg for spk_last_error and returns code
SPK_LOCAL int spk_fail(int code, const std::string& msg);
#define HIP_TRY(expr)                                                                                      \
  do {                                                                                                     \
    hipError_t e_ = (expr);                                                                                \
    if (e_ != hipSuccess) return spk_fail(SPK_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define SPK_TRY(expr) do { int r_ = (expr); if (r_ != SPK_OK) return r_; } while (0)

// model_graph.hip: the graph analysis.  No HIP call: fills m->layers (modes, roles, every fusion-candidate index), the
// parameter table with its flat offsets (n_flat, n_train, n_means) and the offsets into the packed images with their sizes
// (spk_model::n_wpack ...)
SPK_LOCAL int spk_graph_build(spk_model* m, const spk_layer_desc* layers, const int32_t* groups, int n);
// tensor t: n_src layers take it as their input, n_res convs add it as their shortcut operand (last: the last of them); producer writes it
struct Readers { int n_src = 0, n_res = 0, last = -1, producer = -1; int total() const { return n_src + n_res; } };
SPK_LOCAL Readers spk_readers_of(const spk_model* m, int t);
// what the fp8 roles ask of an MBConv block's first conv (model_pack.hip; spk_graph_build resolves Layer::exp_next with it)
static inline bool spk_expand_shaped(const spk_layer_desc& d) {
  return d.kind == SPK_OP_CONV && d.k == 1 && d.stride == 1 && d.res < 0 && d.cout % 16 == 0 && d.src != 0;
}
SPK_LOCAL void spk_free_acts(spk_model* m);
// model_pack.hip
int spk_commit(spk_model* m);
// does this conv run with hi/lo split weights in the eval path?  (inline: the executor asks several times per launch)
static inline int layer_split(const spk_model* m, const Layer& L) {
  if (m->infer_dt != DT_F16 || m->splitw == 0) return 0;
  if (m->splitw == 4) return m->split_mask[&L - m->layers.data()] ? 1 : 0;
  // 5: no conv at all - every fp16 weight image is zero-sum rounded instead (the 7x7 stem as whole rows against the
  // image's channel means: raw pixels on a near-constant background are almost all mean)
  if (m->splitw == 5) return 0;
  // 3: every conv except the 3x3 conv in the middle of a BOTTLENECK block, i.e. a 3x3 conv that neither writes the
  // trunk nor reads it (tests/archive/diagnostics/split_rules.py: its weight rounding adds the least logit error per MFMA
  // cycle a lo-product costs).  The first 3x3 conv of a basic block (ResNet-18/34) reads the trunk and stays split:
  // un-split it costs 1.1e-3 of probability on the class-standardised golden fixture (tests/archive/diagnostics/diverse_prec.py)
  // (Round 3 tried splitting the last stage's inner 3x3 convs as well, tests/archive/diagnostics/split_rules.py "all-but-
  // inner3x3(stages1-3)": +0.29 ms per forward and no gain on the class-standardised golden fixture.)
  // EfficientNets: none.  Their error is the fp16 rounding of every stored activation, amplified layer by layer through 16-32
  // SiLU blocks (tests/archive/diagnostics/effnet_prec.py); the weight rounding does not show beside it - goldens 1.2e-4 with
  // hi + lo on every 1x1 conv, 2.4e-4 without, fresh images the same medians and maxima either way
  // (tests/archive/diagnostics/effnet_calibrated.py) - while the lo products cost 7 % of the B4 forward (26.2 -> 28.2 k img/s).
  // MobileNetV3 (Hardswish / Hardsigmoid graphs): every conv.  On a trained MobileNetV3-Large the weight rounding does show:
  // 7.1e-4 ... 1.06e-3 worst of 256 images without the lo products, 3.4e-4 ... 5.8e-4 with them (tests/test_gpu_mobilenet.py).
  if (m->splitw == 3 && m->effnet && !m->mobilenet) return 0;
  if (m->splitw == 3) return L.trunk_writer || L.d.k != 3 || !L.inner3x3 ? 1 : 0;
  return m->splitw == 1 || L.trunk_writer ? 1 : 0;
}
static inline float spk_fp8_scale_of(float amax) {
  // value = byte * scale; 2x headroom over the calibration batch (e4m3 keeps its 3 mantissa bits over 15 binades,
  // so headroom costs no precision); conversion saturates at +-448
  return amax > 0.f ? 2.f * amax / 448.f : 1.f;
}
SPK_LOCAL int spk_fp8_pack(spk_model* m);
int spk_train_join(spk_model* m);   // train.hip: the model's stream waits for the last step's deferred side-stream work
// model.hip: the activation plan and the eval executor
int spk_plan(spk_model* m, int n, int h, int w, bool pad = false);
SPK_LOCAL int spk_micro_batch(spk_model* m, int n);
static inline size_t spk_image_stride_bytes(int c, int h, int w, int dtype) { return (size_t)c * h * w * (dtype == SPK_DTYPE_U8 ? 1 : 4); }
SPK_LOCAL void spk_eval_begin(spk_model* m, int nb);   // a forward of nb images starts: nothing has run, no e4m3 shadow is valid
int spk_run_layer_eval(spk_model* m, Layer& L, const EvalCursor& c, unsigned allow);   // allow: FUSE_* | EVAL_FORWARD
// SpkTwin::user of the eval executor (tune_table.h): what a half's launches know of the other half, set with the cursor
struct EvalTwin {
  const spk_model* m;
  int img0, twin_img0, twin_n;   // this half's first image; the other half's first image and image count
  bool two_streams;              // the halves are live on two streams (not the first forward of a shape, which tunes on one)
};
SPK_LOCAL bool spk_twin_rebase(void* user, const void** p);   // SpkTwin::rebase of the eval executor (user: an EvalTwin)
int spk_forward_eval_logits(spk_model* m, const void* x, int n, int h, int w, int layout, int dtype,
                            float* logits_dev);
int spk_read_flat(spk_model* m, const float* flat, const Param& p, float* host);
int spk_load_flat(spk_model* m, float* flat, const Param& p, const float* host);   // the inverse (state_dict -> device layout)
void spk_train_free(spk_model* m);
// backward of one convolution (train.hip): shared by the training step and the single-operator test hooks
// fuse: (stride 1 only) the BatchNorm-backward reduction of the layer that produced the tensor dx is the gradient of,
// emitted by the dgrad epilogue (ConvArgs::bnb_raw); `tiles` returns the number of [2][cin] partial rows written
struct BnbFuse {
  const bf16_t* raw;
  const unsigned char* mask;   // null: no ReLU behind that BatchNorm
  const float* mean;
  const float* invstd;
  float* partials;
  int tiles;
  // optional: the shortcut gradient is taken from its source instead of from dx (dx is then overwritten, not accumulated):
  // res_src = output gradient of the block-closing conv whose shortcut this tensor is, res_bits = that conv's ReLU bits
  const bf16_t* res_src;
  const unsigned char* res_bits;
};
int spk_conv_dgrad_all(const bf16_t* dy, const bf16_t* wdg, bf16_t* dx, bool accumulate, int n, int oh, int ow,
                       int cout, int ih, int iw, int cin, int k, int stride, int pad, hipStream_t s,
                       BnbFuse* fuse = nullptr);
size_t spk_conv_wgrad_slab_floats(int M, int cin, int cout, int k, bool stem);
int spk_conv_wgrad_slabs(const bf16_t* x, const bf16_t* dy, float* slabs, int n, int ih, int iw, int cin, int oh,
                         int ow, int cout, int k, int stride, int pad, bool stem, hipStream_t s);
int spk_conv_wgrad_reduce(const float* slabs, float* gw, int M, int cin, int cout, int k, bool stem, hipStream_t s,
                          float scale = 1.0f);
void spk_train_mark_dirty(spk_model* m);
