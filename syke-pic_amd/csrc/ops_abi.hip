// Single-operator entry points of the C-ABI (include/sykepic_hip.h, "test hooks: single operators").
// Each one runs the launches a training step or the eval executor makes for ONE layer (the shared helpers of train.hip
// and the spk_launch_* functions), on caller-provided device buffers, so that a parity test can hand a kernel
// known operands and compare its output with autograd evaluated on the same (bf16-rounded) operands:
//   conv + train-mode BatchNorm forward   torch Conv2d + BatchNorm2d(+add)(+ReLU), sykepic/train/train.py:240
//   BatchNorm / conv backward             what loss.backward() runs for that layer,  sykepic/train/train.py:242
//   Linear / softmax / CrossEntropyLoss    spk_op_linear, spk_op_linear_backward, spk_op_softmax, spk_op_cross_entropy,
//                                          spk_op_cross_entropy_ex (class weights, label smoothing, per-class counters),
//                                          spk_op_cross_entropy_pair (the Mixup / CutMix criterion on two label vectors)
//                                          spk_op_cross_entropy_distill (that criterion distilled against a teacher's logits)
//   MaxPool2d / AdaptiveAvgPool2d(1)       spk_op_maxpool, spk_op_maxpool_backward, spk_op_gavgpool, spk_op_gavgpool_backward
//                                          (head.hip, pointwise.hip, train_kernels.hip; exact integer and float64 references)
// The dense conv kernels' argument descriptors come from the builders of conv_args.h, the ones model.hip and train.hip
// call: a hook resolves its own pointers and shape and derives PwConvArgs / C3Args from the ConvArgs as the executor
// does, so the extents, the stem's row pitch and the padding rules a test judges are those of a real forward or step.
// Scratch is allocated and freed inside the call (these are not on any hot path).
#include "model.h"
#include "conv_args.h"
#include "train_effnet.h"
#include "tune_table.h"

#include <algorithm>
#include <cstring>
#include <vector>

static int ofail(int code, const std::string& msg) {
  spk_set_error(msg);
  return code;
}

namespace {
struct Scratch {
  std::vector<void*> p;
  ~Scratch() { for (void* q : p) (void)hipFree(q); }
  template <typename T> T* get(size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, (count ? count : 1) * sizeof(T)) != hipSuccess) return nullptr;
    p.push_back(q);
    return (T*)q;
  }
};
bool stem_shape(int cin, int cout, int k, int stride, int pad) {
  return cin <= 4 && k == 7 && stride == 2 && pad == 3 && cout == 64;
}
}  // namespace

#define O_TRY(expr, what)                                                         \
  do {                                                                            \
    if ((expr) != 0) return ofail(SPK_ERR_HIP, std::string(what) + " failed");    \
  } while (0)

// the end of a hook: its launches have run when it returns, and a fault in one of them is this hook's error
#define O_SYNC(s, msg) do { if (hipStreamSynchronize(s) != hipSuccess) return ofail(SPK_ERR_HIP, msg); } while (0)

// an implicit-GEMM launch: -3 is a candidate pinned by spk_op_conv_pin that is not instantiated for the problem
#define O_CONV(expr, what)                                                                                      \
  do {                                                                                                          \
    const int rc_ = (expr);                                                                                     \
    if (rc_ == -3) return ofail(SPK_ERR_UNSUPPORTED, std::string(what) + ": the pinned candidate does not fit this problem"); \
    if (rc_ != 0) return ofail(SPK_ERR_HIP, std::string(what) + " failed");                                    \
  } while (0)

// Pins the implicit-GEMM candidate (tile config 0..6, main-loop flavour 0..6) and the weight-gradient pipeline depth
// (1 or 2) for every later launch of the process; -1 leaves that choice to the tuner.  The tile and the flavour go
// together: both pinned or neither.
extern "C" int spk_op_conv_pin(int cfg, int dma, int wgrad_nbuf) {
  if (cfg < -1 || cfg > 6 || dma < -1 || dma > 6 || (cfg < 0) != (dma < 0) ||
      (wgrad_nbuf != -1 && wgrad_nbuf != 1 && wgrad_nbuf != 2))
    return ofail(SPK_ERR_ARG, "op_conv_pin: cfg 0..6 and flavour 0..6 together (or both -1), wgrad_nbuf 1, 2 or -1");
  spk_conv_set_pin(cfg, dma, wgrad_nbuf);
  return SPK_OK;
}

// The tuner table by tag name: find (0), store and append (1), forget (2).  Host only.
extern "C" int spk_op_tune_table(int what, const char* tag, const int* key, int n_key, int* vals, int n_vals, int* found) {
  if (what == 2) {
    spk_tune_reset_for_test();
    return SPK_OK;
  }
  if ((what != 0 && what != 1) || !tag || !key || !vals || (what == 0 && !found))
    return ofail(SPK_ERR_ARG, "op_tune_table: what 0 (find), 1 (store) or 2 (forget); tag, key and vals must be given");
  int t = 0;
  while (t < TUNE_NTAGS && !(kTuneSchemas[t].tag && !strcmp(kTuneSchemas[t].tag, tag))) ++t;
  if (t == TUNE_NTAGS) return ofail(SPK_ERR_ARG, std::string("op_tune_table: no tuner writes the tag ") + tag);
  if (n_key != kTuneSchemas[t].n_key || n_vals != kTuneSchemas[t].n_val)
    return ofail(SPK_ERR_ARG, std::string("op_tune_table: wrong field counts for the tag ") + tag);
  if (what == 1) spk_tune_store((TuneTag)t, key, vals, true);
  else *found = spk_tune_find((TuneTag)t, key, vals) ? 1 : 0;
  return SPK_OK;
}

extern "C" int spk_op_conv_bn_train_forward(const void* x, const float* w_ohwi, const float* gamma, const float* beta,
                                            float* running_mean, float* running_var, const void* res, void* out,
                                            void* raw, unsigned char* mask, float* mean_invstd, int n, int h, int w,
                                            int cin, int cout, int k, int stride, int pad, int relu, void* stream) {
  if (!x || !w_ohwi || !gamma || !beta || !running_mean || !running_var || !out || !raw || !mean_invstd || n < 1)
    return ofail(SPK_ERR_ARG, "op_conv_bn_train_forward: bad arguments");
  const bool stem = stem_shape(cin, cout, k, stride, pad);
  if ((!stem && (cin % 64 || cin < 64)) || cout % 64) return ofail(SPK_ERR_UNSUPPORTED, "channels must be multiples of 64 (or the 7x7/2 stem)");
  hipStream_t s = (hipStream_t)stream;
  const ConvGeom g = stem ? spk_stem_geom(n, h, w) : spk_conv_geom(n, h, w, cin, cout, k, stride, pad);
  const int M = n * g.Ho * g.Wo;
  Scratch sc;
  bf16_t* wp = sc.get<bf16_t>((size_t)cout * g.K);
  float* part = sc.get<float>((size_t)((M + 60) / 61) * 2 * cout);
  float* st = sc.get<float>((size_t)2 * cout);
  float* tmp = sc.get<float>((size_t)cout * 2 * 64);
  if (!wp || !part || !st || !tmp) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  O_TRY(spk_launch_pack_weights(w_ohwi, wp, cout, k, k, cin, stem ? CONV_MODE_STEM : CONV_MODE_GENERIC, DT_BF16, 0, s),
        "pack_weights");
  ConvArgs a = spk_conv_args(g, (const bf16_t*)x, wp, (bf16_t*)raw, nullptr, nullptr, nullptr, 0, DT_BF16, 0);
  a.stats = part;
  int m_tiles = 0;
  O_CONV(spk_conv_launch(a, stem ? CONV_MODE_STEM : CONV_MODE_GENERIC, s, &m_tiles), "conv launch");
  O_TRY(spk_launch_bn_finalize(part, m_tiles, cout, (double)M, gamma, beta, running_mean, running_var, mean_invstd,
                               mean_invstd + cout, st, st + cout, 1e-5f, 0.1f, tmp, s), "bn_finalize");
  O_TRY(spk_launch_bn_apply((const bf16_t*)raw, st, st + cout, (const bf16_t*)res, (bf16_t*)out, mask,
                            (size_t)M * cout, cout, relu, s), "bn_apply");
  O_SYNC(s, "op_conv_bn_train_forward: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_bn_backward(const void* g, const unsigned char* mask, const void* raw, const float* mean,
                                  const float* invstd, const float* gamma, float* dgamma, float* dbeta, void* dy,
                                  void* g_res, int res_accumulate, int M, int C, int relu, void* stream) {
  if (!g || !raw || !mean || !invstd || !gamma || !dy || M < 1 || C % 8 || (relu && !mask))
    return ofail(SPK_ERR_ARG, "op_bn_backward: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  Scratch sc;
  int rpb;
  const int nb = spk_bn_bwd_blocks(M, C, &rpb);
  float* part = sc.get<float>((size_t)nb * 2 * C);
  float* coef = sc.get<float>((size_t)3 * C);
  float* tmp = sc.get<float>((size_t)C * 2 * 64);
  if (!part || !coef || !tmp) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  O_TRY(spk_launch_bn_bwd((const bf16_t*)g, mask, (const bf16_t*)raw, mean, invstd, gamma, part, coef, dgamma, dbeta,
                          (bf16_t*)dy, (bf16_t*)g_res, res_accumulate, M, C, relu, tmp, s), "bn_bwd");
  O_SYNC(s, "op_bn_backward: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_conv_dgrad(const void* dy, const float* w_ohwi, void* dx, int accumulate, int n, int h, int w,
                                 int cin, int cout, int k, int stride, int pad, void* stream) {
  if (!dy || !w_ohwi || !dx || n < 1) return ofail(SPK_ERR_ARG, "op_conv_dgrad: bad arguments");
  if (cin % 64 || cout % 64) return ofail(SPK_ERR_UNSUPPORTED, "channels must be multiples of 64");
  hipStream_t s = (hipStream_t)stream;
  const int oh = (h + 2 * pad - k) / stride + 1, ow = (w + 2 * pad - k) / stride + 1;
  Scratch sc;
  bf16_t* wdg = sc.get<bf16_t>((size_t)cin * k * k * cout);
  if (!wdg) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  O_TRY(spk_launch_pack_dgrad(w_ohwi, wdg, cout, k * k, cin, s), "pack_dgrad");
  const int r = spk_conv_dgrad_all((const bf16_t*)dy, wdg, (bf16_t*)dx, accumulate != 0, n, oh, ow, cout, h, w, cin, k,
                                   stride, pad, s);
  if (r != SPK_OK) return r;
  O_SYNC(s, "op_conv_dgrad: kernel failed");
  return SPK_OK;
}

// Data gradient of a stride-1 conv whose epilogue also makes the BatchNorm-backward sums of the layer that PRODUCED the
// conv's input (conv_igemm.hip, spk_set_bnb), followed by that layer's finalize + apply with the reduce pass skipped:
// the launches a training step makes for (consumer conv dgrad, producer BatchNorm backward).  dx (+)= conv_transpose(dy, w)
// is the gradient g of the producer's output; raw / mask / mean / invstd / gamma are the producer's; dy_prod receives the
// gradient of the producer's raw conv output, dgamma / dbeta its parameter gradients.
extern "C" int spk_op_conv_dgrad_bn_backward(const void* dy, const float* w_ohwi, void* dx, int accumulate, const void* raw,
                                             const unsigned char* mask, const float* mean, const float* invstd,
                                             const float* gamma, float* dgamma, float* dbeta, void* dy_prod, int n, int h,
                                             int w, int cin, int cout, int k, int pad, int relu, const void* res_src,
                                             const unsigned char* res_bits, void* stream) {
  if (!dy || !w_ohwi || !dx || !raw || !mean || !invstd || !gamma || !dy_prod || n < 1 || (relu && !mask))
    return ofail(SPK_ERR_ARG, "op_conv_dgrad_bn_backward: bad arguments");
  if (cin % 64 || cout % 64) return ofail(SPK_ERR_UNSUPPORTED, "channels must be multiples of 64");
  hipStream_t s = (hipStream_t)stream;
  const int oh = h + 2 * pad - k + 1, ow = w + 2 * pad - k + 1, M = n * h * w;
  Scratch sc;
  bf16_t* wdg = sc.get<bf16_t>((size_t)cin * k * k * cout);
  float* part = sc.get<float>((size_t)((M + 60) / 61) * 2 * cin);
  float* coef = sc.get<float>((size_t)3 * cin);
  float* tmp = sc.get<float>((size_t)cin * 2 * 64);
  if (!wdg || !part || !coef || !tmp) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  O_TRY(spk_launch_pack_dgrad(w_ohwi, wdg, cout, k * k, cin, s), "pack_dgrad");
  BnbFuse fz;
  fz.raw = (const bf16_t*)raw; fz.mask = relu ? mask : nullptr; fz.mean = mean; fz.invstd = invstd; fz.partials = part; fz.tiles = 0;
  fz.res_src = (const bf16_t*)res_src; fz.res_bits = res_bits;
  if ((res_src != nullptr) != (res_bits != nullptr) || (res_src && accumulate))
    return ofail(SPK_ERR_ARG, "op_conv_dgrad_bn_backward: res_src and res_bits go together and replace accumulate");
  const int r = spk_conv_dgrad_all((const bf16_t*)dy, wdg, (bf16_t*)dx, accumulate != 0, n, oh, ow, cout, h, w, cin, k, 1, pad,
                                   s, &fz);
  if (r != SPK_OK) return r;
  if (fz.tiles < 1) return ofail(SPK_ERR_HIP, "the dgrad launch reported no partial rows");
  O_TRY(spk_launch_bn_bwd((const bf16_t*)dx, mask, (const bf16_t*)raw, mean, invstd, gamma, part, coef, dgamma, dbeta,
                          (bf16_t*)dy_prod, nullptr, 0, M, cin, relu, tmp, s, fz.tiles), "bn_bwd");
  O_SYNC(s, "op_conv_dgrad_bn_backward: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_conv_wgrad(const void* x, const void* dy, float* dw_ohwi, int n, int h, int w, int cin, int cout,
                                 int k, int stride, int pad, void* stream) {
  if (!x || !dy || !dw_ohwi || n < 1) return ofail(SPK_ERR_ARG, "op_conv_wgrad: bad arguments");
  const bool stem = stem_shape(cin, cout, k, stride, pad);
  if ((!stem && cin % 64) || cout % 64) return ofail(SPK_ERR_UNSUPPORTED, "channels must be multiples of 64 (or the 7x7/2 stem)");
  hipStream_t s = (hipStream_t)stream;
  const int oh = (h + 2 * pad - k) / stride + 1, ow = (w + 2 * pad - k) / stride + 1;
  const int M = n * oh * ow;
  Scratch sc;
  float* slabs = sc.get<float>(spk_conv_wgrad_slab_floats(M, cin, cout, k, stem));
  if (!slabs) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  int r = spk_conv_wgrad_slabs((const bf16_t*)x, (const bf16_t*)dy, slabs, n, h, stem ? (w + 1) & ~1 : w, cin, oh, ow,
                               cout, k, stride, pad, stem, s);
  if (r != SPK_OK) return r;
  r = spk_conv_wgrad_reduce(slabs, dw_ohwi, M, cin, cout, k, stem, s);
  if (r != SPK_OK) return r;
  O_SYNC(s, "op_conv_wgrad: kernel failed");
  return SPK_OK;
}

// fp8 (e4m3) pointwise conv of the EfficientNet MBConv interior (pw_fp8.hip) on caller-provided buffers:
// packs the fp32 weights [cout][cin] to e4m3 with per-output-channel scales, folds bn_scale x weight scale x
// a_scale into the epilogue factor and runs the kernel the eval path runs.
extern "C" int spk_op_pw_fp8(const void* x, int a_fp8, const float* w, void* y, int out_fp8, const void* res,
                             const float* bn_scale, const float* bn_bias, const float* gate, int hw, int m_rows, int cin,
                             int cout, int act, float a_scale, float y_scale, void* stream) {
  if (!x || !w || !y || !bn_scale || !bn_bias || m_rows < 1 || cin < 1 || cout < 1 || a_scale <= 0.f || y_scale <= 0.f)
    return ofail(SPK_ERR_ARG, "op_pw_fp8: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const int npad = (cout + 63) / 64 * 64, kpad = (cin + 63) / 64 * 64;
  Scratch sc;
  unsigned char* w8 = sc.get<unsigned char>((size_t)npad * kpad);
  float* f = sc.get<float>((size_t)4 * npad);   // ws, epilogue scale, padded bn scale, padded bias
  if (!w8 || !f) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  if (hipMemsetAsync(f, 0, (size_t)4 * npad * 4, s) != hipSuccess ||
      hipMemcpyAsync(f + 2 * npad, bn_scale, (size_t)cout * 4, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemcpyAsync(f + 3 * npad, bn_bias, (size_t)cout * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return ofail(SPK_ERR_HIP, "op_pw_fp8: staging failed");
  O_TRY(spk_launch_pack_fp8(w, w8, f, cout, cin, npad, kpad, 1.f, s), "pack_fp8");
  O_TRY(spk_launch_mul3(f + 2 * npad, f, a_scale, f + npad, npad, s), "scale folding");
  const int r = spk_launch_pw_fp8(x, a_fp8, w8, y, out_fp8, (const bf16_t*)res, f + npad, f + 3 * npad, gate, cin, hw, m_rows,
                                  kpad, npad, cin, cout, act, 1.f / a_scale, 1.f / y_scale, s);
  if (r == -2) return ofail(SPK_ERR_UNSUPPORTED, "op_pw_fp8: shape not supported (cin % 8 / 16, cout % 8)");
  if (r) return ofail(SPK_ERR_HIP, "op_pw_fp8: launch failed");
  O_SYNC(s, "op_pw_fp8: kernel failed");
  return SPK_OK;
}

// Depthwise conv + folded BN + activation through the LDS-staged kernel (dwconv_lds.hip; lds != 0) or the gather
// kernel (effnet.hip; lds 0), fp16 NHWC tensors, w: float32 [C][k*k].  pool_out (optional): float32 [n][C] sums of the outputs
// over each image (the squeeze-excitation pool numerator).
extern "C" int spk_op_dwconv(const void* x, const float* w, const float* bn_scale, const float* bn_bias, void* y,
                             float* pool_out, int n, int h, int wid, int c, int k, int stride, int act, int lds,
                             void* stream) {
  if (!x || !w || !bn_scale || !bn_bias || !y || n < 1 || c % 8) return ofail(SPK_ERR_ARG, "op_dwconv: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const int pad = (k - 1) / 2, ho = (h + 2 * pad - k) / stride + 1, wo = (wid + 2 * pad - k) / stride + 1;
  Scratch sc;
  float* wt = sc.get<float>((size_t)k * k * c);
  int chunks = lds ? spk_dwconv_lds_chunks(0, n, h, wid, c, ho, wo, k, stride) : spk_dw_chunks(n, ho * ((wo + 3) / 4), c);
  if (lds && chunks <= 0) return ofail(SPK_ERR_UNSUPPORTED, "op_dwconv: this kernel cannot run this shape");
  float* partial = sc.get<float>((size_t)n * chunks * c);
  if (!wt || !partial) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  O_TRY(spk_launch_pack_tapmajor(w, wt, c, k * k, c, s), "pack_tapmajor");
  int r;
  if (lds)
    r = spk_launch_dwconv_lds(0, x, wt, bn_scale, bn_bias, y, partial, n, h, wid, c, ho, wo, k, stride, act, 1.f, 1.f, s);
  else
    r = spk_launch_dwconv((const bf16_t*)x, wt, bn_scale, bn_bias, (bf16_t*)y, partial, n, h, wid, c, ho, wo, k, stride, act,
                          DT_F16, s);
  if (r) return ofail(SPK_ERR_HIP, "op_dwconv: launch failed");
  O_SYNC(s, "op_dwconv: kernel failed");
  if (pool_out) {
    std::vector<float> hp((size_t)n * chunks * c), out((size_t)n * c, 0.f);
    if (hipMemcpy(hp.data(), partial, hp.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return ofail(SPK_ERR_HIP, "copy failed");
    for (int i = 0; i < n; ++i)
      for (int q = 0; q < chunks; ++q)
        for (int ch = 0; ch < c; ++ch) out[(size_t)i * c + ch] += hp[((size_t)i * chunks + q) * c + ch];
    if (hipMemcpy(pool_out, out.data(), out.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return ofail(SPK_ERR_HIP, "copy failed");
  }
  return SPK_OK;
}

// 1x1 convolution + folded BatchNorm (+shortcut) (+ReLU) of the eval path (conv_pw.hip) on caller-provided buffers:
// packs the fp32 weights [cout][cin] into fragment order (hi + lo images when split != 0) and
// runs configuration `cfg` of the kernel; cfg < 0: the implicit-GEMM kernel on the same operands (the reference
// point of the two-kernel tuner).  SPK_ERR_UNSUPPORTED when the configuration does not fit the problem.
extern "C" int spk_op_conv1x1(const void* x, const float* w, const float* bn_scale, const float* bn_bias, const void* res,
                              void* y, int n, int h, int wd, int cin, int cout, int stride, int relu, int split, int cfg,
                              void* stream) {
  if (!x || !w || !bn_scale || !bn_bias || !y || n < 1 || h < 1 || wd < 1 || (stride != 1 && stride != 2))
    return ofail(SPK_ERR_ARG, "op_conv1x1: bad arguments");
  if (cin % 64 || cout % 64) return ofail(SPK_ERR_UNSUPPORTED, "channels must be multiples of 64");
  hipStream_t s = (hipStream_t)stream;
  Scratch sc;
  bf16_t* wp = sc.get<bf16_t>((size_t)2 * cout * cin);
  if (!wp) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  const ConvArgs a = spk_conv_args(spk_conv_geom(n, h, wd, cin, cout, 1, stride, 0), (const bf16_t*)x, wp, (bf16_t*)y,
                                   (const bf16_t*)res, bn_scale, bn_bias, relu, DT_F16, split != 0);
  // 32-bit buffer offsets in both kernels: every operand below 2 GiB (the model executor micro-batches for this)
  if (!spk_below_2gib(a)) return ofail(SPK_ERR_UNSUPPORTED, "op_conv1x1: an operand of 2 GiB or more (split the batch)");
  int r;
  if (cfg < 0) {
    O_TRY(spk_launch_pack_weights(w, wp, cout, 1, 1, cin, CONV_MODE_GENERIC, DT_F16, split != 0, s), "pack_weights");
    O_CONV(spk_conv_launch(a, CONV_MODE_GENERIC, s, nullptr), "conv1x1 launch");
    r = 0;
  } else {
    O_TRY(spk_launch_pack_pw(w, nullptr, wp, cout, cin, DT_F16, split ? 2 : 1, s), "pack_pw");
    r = spk_pw_launch(pw_args(a, wp), cfg, s);
    if (r == -3) return ofail(SPK_ERR_UNSUPPORTED, "this configuration does not fit the problem");
  }
  if (r) return ofail(SPK_ERR_HIP, "conv1x1 launch failed");
  O_SYNC(s, "conv1x1 kernel failed");
  return SPK_OK;
}
extern "C" int spk_op_conv1x1_num_configs(void) { return spk_pw_num_configs(); }

// A block-closing 1x1 conv and the block's 1x1 shortcut (downsample) conv as ONE K-concatenated GEMM (PwConvArgs::x2):
// y = act(BN1(W1 . x) + BN2(W2 . x2[stride2])), what the eval path runs in the first block of a ResNet stage.  The two
// eval-BatchNorm scales are folded into the concatenated fp16 weight rows (spk_launch_pw_dual_prep).  cfg: a configuration
// of spk_pw_launch (SPK_ERR_UNSUPPORTED when it does not fit the problem).
extern "C" int spk_op_conv1x1_dual(const void* x, const float* w1, const float* s1, const float* b1, const void* x2,
                                   const float* w2, const float* s2, const float* b2, void* y, int n, int ho, int wo, int cin,
                                   int h2, int w2d, int cin2, int cout, int stride2, int relu, int split, int cfg,
                                   void* stream) {
  if (!x || !w1 || !s1 || !b1 || !x2 || !w2 || !s2 || !b2 || !y || n < 1 || ho < 1 || wo < 1 || stride2 < 1)
    return ofail(SPK_ERR_ARG, "op_conv1x1_dual: bad arguments");
  if (cin % 64 || cin2 % 64 || cout % 64) return ofail(SPK_ERR_UNSUPPORTED, "channels must be multiples of 64");
  if ((ho - 1) * stride2 >= h2 || (wo - 1) * stride2 >= w2d) return ofail(SPK_ERR_ARG, "op_conv1x1_dual: second source too small");
  hipStream_t s = (hipStream_t)stream;
  const int K = cin + cin2;
  Scratch sc;
  float* wcat = sc.get<float>((size_t)cout * K);
  float* sb = sc.get<float>((size_t)2 * cout);
  bf16_t* wp = sc.get<bf16_t>((size_t)2 * cout * K);
  if (!wcat || !sb || !wp) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  // the block-closing conv as the executor's conv_dual derives it (stride 1, the shortcut inside the GEMM), then the source
  PwConvArgs q = pw_args(spk_conv_args(spk_conv_geom(n, ho, wo, cin, cout, 1, 1, 0), (const bf16_t*)x, nullptr, (bf16_t*)y,
                                       nullptr, sb, sb + cout, relu, DT_F16, split != 0), wp);
  spk_pw_set_second(q, (const bf16_t*)x2, cin2, h2, w2d, stride2);
  if (!spk_below_2gib(q)) return ofail(SPK_ERR_UNSUPPORTED, "op_conv1x1_dual: an operand of 2 GiB or more");
  O_TRY(spk_launch_pw_dual_prep(w1, w2, s1, s2, b1, b2, wcat, sb, sb + cout, cout, cin, cin2, s), "pw_dual_prep");
  O_TRY(spk_launch_pack_pw(wcat, nullptr, wp, cout, K, DT_F16, split ? 2 : 1, s), "pack_pw");
  const int r = spk_pw_launch(q, cfg, s);
  if (r == -3) return ofail(SPK_ERR_UNSUPPORTED, "this configuration does not fit the problem");
  if (r) return ofail(SPK_ERR_HIP, "dual conv1x1 launch failed");
  O_SYNC(s, "dual conv1x1 kernel failed");
  return SPK_OK;
}

// Two chained 1x1 convs in one launch (conv_pw.hip, PwConvArgs::wpz): y = act(BN(W . x) + res) with 256 couts, then
// z = actz(BNz(Wz . y)) from the output tile in registers; single fp16 weight images.  What the eval path runs for a
// bottleneck's block-closing conv and the next block's first conv.  SPK_ERR_UNSUPPORTED: no chained kernel for the shape.
extern "C" int spk_op_conv1x1_chain(const void* x, const float* w, const float* bn_scale, const float* bn_bias, const void* res,
                                    void* y, const float* wz, const float* bnz_scale, const float* bnz_bias, void* z, int n,
                                    int h, int wd, int cin, int cout, int coutz, int relu, int reluz, void* stream) {
  if (!x || !w || !bn_scale || !bn_bias || !res || !y || !wz || !bnz_scale || !bnz_bias || !z || n < 1 || h < 1 || wd < 1)
    return ofail(SPK_ERR_ARG, "op_conv1x1_chain: bad arguments");
  if (cin % 64 || cout % 64 || coutz % 32) return ofail(SPK_ERR_UNSUPPORTED, "channels must be multiples of 64");
  hipStream_t s = (hipStream_t)stream;
  Scratch sc, scz;
  bf16_t* wp = sc.get<bf16_t>((size_t)cout * cin);
  bf16_t* wpz = scz.get<bf16_t>((size_t)coutz * cout);
  if (!wp || !wpz) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  PwConvArgs q = pw_args(spk_conv_args(spk_conv_geom(n, h, wd, cin, cout, 1, 1, 0), (const bf16_t*)x, nullptr, (bf16_t*)y,
                                       (const bf16_t*)res, bn_scale, bn_bias, relu, DT_F16, 0), wp);
  spk_pw_set_chain(q, wpz, (bf16_t*)z, bnz_scale, bnz_bias, coutz, reluz);
  if (!spk_below_2gib(q)) return ofail(SPK_ERR_UNSUPPORTED, "op_conv1x1_chain: an operand of 2 GiB or more");
  O_TRY(spk_launch_pack_pw(w, nullptr, wp, cout, cin, DT_F16, 1, s), "pack_pw");
  O_TRY(spk_launch_pack_pw(wz, nullptr, wpz, coutz, cout, DT_F16, 1, s), "pack_pw");
  const int r = spk_pw_chain_launch(q, s);
  if (r == -3) return ofail(SPK_ERR_UNSUPPORTED, "no chained kernel for this problem");
  if (r) return ofail(SPK_ERR_HIP, "chained conv1x1 launch failed");
  O_SYNC(s, "chained conv1x1 kernel failed");
  return SPK_OK;
}

// 3x3 stride-1 pad-1 convolution + folded BatchNorm (+ReLU) of the eval path (conv_c3.hip) on caller-provided buffers;
// cfg >= 0: that tile configuration (SPK_ERR_UNSUPPORTED when it does not fit), cfg < 0: the implicit-GEMM kernel.
extern "C" int spk_op_conv3x3(const void* x, const float* w_ohwi, const float* bn_scale, const float* bn_bias,
                              const void* res, void* y, int n, int h, int wd, int cin, int cout, int relu, int split,
                              int cfg, void* stream) {
  if (!x || !w_ohwi || !bn_scale || !bn_bias || !y || n < 1 || h < 1 || wd < 1)
    return ofail(SPK_ERR_ARG, "op_conv3x3: bad arguments");
  if (cin % 64 || cout % 64) return ofail(SPK_ERR_UNSUPPORTED, "channels must be multiples of 64");
  hipStream_t s = (hipStream_t)stream;
  Scratch sc;
  bf16_t* wp = sc.get<bf16_t>((size_t)2 * cout * 9 * cin);
  if (!wp) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  const ConvArgs a = spk_conv_args(spk_conv_geom(n, h, wd, cin, cout, 3, 1, 1), (const bf16_t*)x, wp, (bf16_t*)y,
                                   (const bf16_t*)res, bn_scale, bn_bias, relu, DT_F16, split != 0);
  if (!spk_below_2gib(a)) return ofail(SPK_ERR_UNSUPPORTED, "op_conv3x3: an operand of 2 GiB or more (split the batch)");
  int r;
  if (cfg < 0) {
    O_TRY(spk_launch_pack_weights(w_ohwi, wp, cout, 3, 3, cin, CONV_MODE_GENERIC, DT_F16, split != 0, s), "pack_weights");
    O_CONV(spk_conv_launch(a, CONV_MODE_GENERIC, s, nullptr), "conv3x3 launch");
    r = 0;
  } else {
    O_TRY(spk_launch_pack_c3(w_ohwi, wp, cout, cin, split ? 2 : 1, s), "pack_c3");
    r = spk_c3_launch(c3_args(a, wp, split ? 2 : 1), cfg, s);
    if (r == -3) return ofail(SPK_ERR_UNSUPPORTED, "this configuration does not fit the problem");
  }
  if (r) return ofail(SPK_ERR_HIP, "conv3x3 launch failed");
  O_SYNC(s, "conv3x3 kernel failed");
  return SPK_OK;
}
extern "C" int spk_op_conv3x3_num_configs(void) { return spk_c3_num_configs(); }

// The direct 64 -> 64 3x3 kernel (conv_d3.hip) on caller-provided buffers: x [n,h,wd,cin] fp16, w [cout][3][3][cin] fp32.
// cfg >= 0: that configuration, SPK_ERR_UNSUPPORTED ("does not fit") for a problem the kernel does not take (cin or cout
// not 64, stride not 1, split weights) or a configuration it does not have; cfg < 0: the implicit GEMM on the same problem.
// iters > 0: the launch is then repeated iters times between two events and *ms_out is the mean time of one.
extern "C" int spk_op_conv3x3_direct(const void* x, const float* w_ohwi, const float* bn_scale, const float* bn_bias,
                                     const void* res, void* y, int n, int h, int wd, int cin, int cout, int stride, int relu,
                                     int split, int cfg, int iters, float* ms_out, void* stream) {
  if (!x || !w_ohwi || !bn_scale || !bn_bias || !y || n < 1 || h < 1 || wd < 1 || (stride != 1 && stride != 2) || iters < 0)
    return ofail(SPK_ERR_ARG, "op_conv3x3_direct: bad arguments");
  if (cin % 64 || cout % 64) return ofail(SPK_ERR_UNSUPPORTED, "channels must be multiples of 64");
  if (cfg >= 0 && (cin != 64 || cout != 64 || stride != 1 || split))
    return ofail(SPK_ERR_UNSUPPORTED, "this configuration does not fit the problem");
  hipStream_t s = (hipStream_t)stream;
  Scratch sc;
  bf16_t* wp = sc.get<bf16_t>((size_t)2 * cout * 9 * cin);
  if (!wp) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  const ConvArgs a = spk_conv_args(spk_conv_geom(n, h, wd, cin, cout, 3, stride, 1), (const bf16_t*)x, wp, (bf16_t*)y,
                                   (const bf16_t*)res, bn_scale, bn_bias, relu, DT_F16, split != 0);
  if (!spk_below_2gib(a))
    return ofail(SPK_ERR_UNSUPPORTED, "op_conv3x3_direct: an operand of 2 GiB or more (split the batch)");
  const C3Args q = c3_args(a, wp, 1);
  if (cfg < 0) O_TRY(spk_launch_pack_weights(w_ohwi, wp, cout, 3, 3, cin, CONV_MODE_GENERIC, DT_F16, split != 0, s), "pack_weights");
  else O_TRY(spk_launch_pack_pw(w_ohwi, nullptr, wp, cout, 9 * cin, DT_F16, 1, s), "pack_pw");
  auto run = [&]() { return cfg < 0 ? spk_conv_launch(a, CONV_MODE_GENERIC, s, nullptr) : spk_d3_launch(q, cfg, s); };
  const int r = run();
  if (r == -3) return ofail(SPK_ERR_UNSUPPORTED, "this configuration does not fit the problem");
  if (r) return ofail(SPK_ERR_HIP, "conv3x3_direct launch failed");
  O_SYNC(s, "conv3x3_direct kernel failed");
  if (iters > 0 && ms_out) {
    SpkLaunchTimer timer;
    float ms = 0.f;
    if (!timer.ok || !timer.time(s, iters, run, &ms)) return ofail(SPK_ERR_HIP, "conv3x3_direct timing failed");
    *ms_out = ms / (float)iters;
  }
  return SPK_OK;
}
extern "C" int spk_op_conv3x3_direct_num_configs(void) { return spk_d3_num_configs(); }

// A whole identity bottleneck block of the eval path on caller-provided buffers: x, y [n,h,w,4 cm] fp16; fp32 weights
// w1 [cm][4 cm], w2 [cm][3][3][cm], w3 [4 cm][cm]; folded BatchNorm scale / shift per conv.  fused != 0: the one-kernel
// form (conv_bneck.hip; SPK_ERR_UNSUPPORTED when it has no instantiation for the shape); fused == 0: the same block as three
// launches of the eval path's own kernels (conv_pw.hip, conv_c3.hip, conv_pw.hip with the shortcut), mid tensors in
// scratch - the reference point of the parity test and of the tuner.  iters > 0: the launches are repeated and *ms_out
// receives the mean time of one block (events on `stream`).
extern "C" int spk_op_bottleneck(const void* x, const float* w1, const float* w2, const float* w3, const float* s1,
                                 const float* b1, const float* s2, const float* b2, const float* s3, const float* b3, void* y,
                                 int n, int h, int wd, int cm, int fused, int iters, float* ms_out, void* stream,
                                 unsigned long long* stamps_dev, const float* wz, const float* sz, const float* bz, void* z,
                                 int coutz) {
  if (!x || !w1 || !w2 || !w3 || !s1 || !b1 || !s2 || !b2 || !s3 || !b3 || !y || n < 1 || h < 1 || wd < 1 || x == y)
    return ofail(SPK_ERR_ARG, "op_bottleneck: bad arguments");
  if (cm % 64) return ofail(SPK_ERR_UNSUPPORTED, "mid channels must be a multiple of 64");
  hipStream_t s = (hipStream_t)stream;
  const int c4 = 4 * cm, M = n * h * wd;
  Scratch sc;
  bf16_t* p1 = sc.get<bf16_t>((size_t)cm * c4);
  bf16_t* p2 = sc.get<bf16_t>((size_t)9 * cm * cm);
  bf16_t* p3 = sc.get<bf16_t>((size_t)cm * c4);
  bf16_t* y1 = sc.get<bf16_t>((size_t)M * cm);
  bf16_t* y2 = sc.get<bf16_t>((size_t)M * cm);
  bf16_t* pz = sc.get<bf16_t>((size_t)(wz ? coutz : 1) * c4);
  if (!p1 || !p2 || !p3 || !y1 || !y2 || !pz) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  if (wz && (!sz || !bz || !z || coutz % 32)) return ofail(SPK_ERR_ARG, "op_bottleneck: bad chained-conv arguments");
  BneckArgs a = spk_bneck_args((const bf16_t*)x, (bf16_t*)y, p1, p2, p3, s1, b1, s2, b2, s3, b3, n, h, wd, cm);
  a.stamps = stamps_dev;
  a.y1 = y1;
  if (wz) spk_bneck_set_chain(a, pz, (bf16_t*)z, sz, bz, coutz);
  if (!spk_below_2gib(a)) return ofail(SPK_ERR_UNSUPPORTED, "op_bottleneck: an operand of 2 GiB or more");
  if (wz) O_TRY(spk_launch_pack_pw(wz, nullptr, pz, coutz, c4, DT_F16, 1, s), "pack_pw");
  O_TRY(spk_launch_pack_pw(w1, nullptr, p1, cm, c4, DT_F16, 1, s), "pack_pw");
  O_TRY(spk_launch_pack_c3(w2, p2, cm, cm, 1, s), "pack_c3");
  O_TRY(spk_launch_pack_pw(w3, nullptr, p3, c4, cm, DT_F16, 1, s), "pack_pw");
  // one conv of the three-launch form: k x k, stride 1, ReLU, single weight images - the executor's own derivation
  auto conv = [&](const bf16_t* in, bf16_t* out, const bf16_t* res, const float* sc_, const float* sh_, int cin, int cout, int k) {
    return spk_conv_args(spk_conv_geom(n, h, wd, cin, cout, k, 1, k / 2), in, nullptr, out, res, sc_, sh_, 1, DT_F16, 0);
  };
  auto pw = [&](const bf16_t* in, const bf16_t* wp, bf16_t* out, const bf16_t* res, const float* sc_, const float* sh_, int cin,
                int cout) {
    const PwConvArgs q = pw_args(conv(in, out, res, sc_, sh_, cin, cout, 1), wp);
    for (int cfg : {7, 9, 11, 5, 1, 3, 0, 4})    // (every configuration gives the same bits: tests/test_gpu_pw.py)
      if (const int r = spk_pw_launch(q, cfg, s); r != -3) return r;
    return -3;
  };
  auto once = [&]() -> int {
    if (fused == 1) return wz ? -3 : spk_bneck_launch(a, s);
    if (const int r = pw((const bf16_t*)x, p1, y1, nullptr, s1, b1, c4, cm)) return r;
    if (fused == 2) return spk_btail_launch(a, s);     // conv2 + conv3 + shortcut (+ the chained conv) in one kernel
    const C3Args q = c3_args(conv(y1, y2, nullptr, s2, b2, cm, cm, 3), p2, 1);
    int r = -3;
    for (int cfg : {2, 0, 10, 8, 9, 3, 7})       // (likewise: tests/test_gpu_c3.py)
      if ((r = spk_c3_launch(q, cfg, s)) != -3) break;
    if (r) return r;
    if ((r = pw(y2, p3, (bf16_t*)y, (const bf16_t*)x, s3, b3, cm, c4)) != 0 || !wz) return r;
    return pw((const bf16_t*)y, pz, (bf16_t*)z, nullptr, sz, bz, c4, coutz);
  };
  int r = once();
  if (r == -3) return ofail(SPK_ERR_UNSUPPORTED, "no kernel for this bottleneck shape");
  if (r) return ofail(SPK_ERR_HIP, "bottleneck launch failed");
  if (iters > 0 && ms_out) {
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return ofail(SPK_ERR_HIP, "hipEventCreate failed");
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < iters && !r; ++i) r = once();
    (void)hipEventRecord(e1, s);
    float ms = 0.f;
    const bool ok = !r && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (!ok) return ofail(SPK_ERR_HIP, "bottleneck timing failed");
    *ms_out = ms / iters;
  }
  O_SYNC(s, "bottleneck kernel failed");
  return SPK_OK;
}

// Zero-sum rounding of fp32 weight rows to fp16 values (zero_sum.hip) on caller-provided device buffers: w, out
// [rows][row_len] fp32, mu [mu_period] fp32 or null.  The kernel spk_commit runs per conv in the calibrated mode.
extern "C" int spk_op_zero_sum_round(const float* w, const float* mu, float* out, int64_t rows, int row_len, int mu_period,
                                     void* stream) {
  if (!w || !out || rows < 1 || row_len < 1 || mu_period < 1) return ofail(SPK_ERR_ARG, "op_zero_sum_round: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const int r = spk_launch_zero_sum_round(w, mu, out, (size_t)rows, row_len, mu_period, s);
  if (r == -2) return ofail(SPK_ERR_UNSUPPORTED, "op_zero_sum_round: row too long (8192 elements at most)");
  if (r) return ofail(SPK_ERR_HIP, "zero-sum rounding launch failed");
  O_SYNC(s, "zero-sum rounding kernel failed");
  return SPK_OK;
}

// Grouped 3x3 pad-1 convolution (conv_group.hip: conv2 of a ResNeXt bottleneck) - the launches the eval forward, the
// training forward and the training backward make for such a layer.  Weights fp32 [c][3][3][c / groups].
extern "C" int spk_op_conv_group(const void* x, const float* w, const float* bn_scale, const float* bn_bias, void* y, int n,
                                 int h, int wd, int c, int groups, int stride, int relu, int bf16, void* stream) {
  if (!x || !w || !y || n < 1 || h < 1 || wd < 1 || (!bn_scale) != (!bn_bias)) return ofail(SPK_ERR_ARG, "op_conv_group: bad arguments");
  if (!spk_group_conv_ok(c, groups, 3, stride, 1))
    return ofail(SPK_ERR_UNSUPPORTED, "op_conv_group: c a multiple of 16, 4 / 8 / 16 / 32 / 64 channels per group, stride 1 or 2");
  hipStream_t s = (hipStream_t)stream;
  O_TRY(spk_launch_group_fwd((const bf16_t*)x, w, bn_scale, bn_bias, (bf16_t*)y, n, h, wd, c, groups, stride, relu,
                             bf16 ? DT_BF16 : DT_F16, s), "grouped conv");
  O_SYNC(s, "op_conv_group: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_conv_group_dgrad(const void* dy, const float* w, void* dx, int accumulate, int n, int h, int wd, int c,
                                       int groups, int stride, void* stream) {
  if (!dy || !w || !dx || n < 1 || h < 1 || wd < 1) return ofail(SPK_ERR_ARG, "op_conv_group_dgrad: bad arguments");
  if (!spk_group_conv_ok(c, groups, 3, stride, 1))
    return ofail(SPK_ERR_UNSUPPORTED, "op_conv_group_dgrad: c a multiple of 16, 4 / 8 / 16 / 32 / 64 channels per group, stride 1 or 2");
  hipStream_t s = (hipStream_t)stream;
  O_TRY(spk_launch_group_dgrad((const bf16_t*)dy, w, (bf16_t*)dx, accumulate != 0, n, h, wd, c, groups, stride, DT_BF16, s),
        "grouped conv dgrad");
  O_SYNC(s, "op_conv_group_dgrad: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_conv_group_wgrad(const void* x, const void* dy, float* dw, int n, int h, int wd, int c, int groups,
                                       int stride, void* stream) {
  if (!x || !dy || !dw || n < 1 || h < 1 || wd < 1) return ofail(SPK_ERR_ARG, "op_conv_group_wgrad: bad arguments");
  if (!spk_group_conv_ok(c, groups, 3, stride, 1))
    return ofail(SPK_ERR_UNSUPPORTED, "op_conv_group_wgrad: c a multiple of 16, 4 / 8 / 16 / 32 / 64 channels per group, stride 1 or 2");
  hipStream_t s = (hipStream_t)stream;
  const int64_t M = (int64_t)n * ((h - 1) / stride + 1) * ((wd - 1) / stride + 1);
  Scratch sc;
  float* slabs = sc.get<float>(spk_group_wgrad_slab_floats(M, c, groups));
  if (!slabs) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  int chunks = 0;
  O_TRY(spk_launch_group_wgrad((const bf16_t*)x, (const bf16_t*)dy, slabs, n, h, wd, c, groups, stride, DT_BF16, &chunks, s),
        "grouped conv wgrad");
  O_TRY(spk_launch_slab_reduce(slabs, dw, (size_t)c * 9 * (c / groups), chunks, s), "grouped conv wgrad reduce");
  O_SYNC(s, "op_conv_group_wgrad: kernel failed");
  return SPK_OK;
}

// ---- the MBConv training kernels (train_effnet.hip), one layer at a time: the launches spk_train_forward_backward makes
// for a depthwise conv, a BatchNorm + activation, a squeeze-excitation layer and the 3x3 stem of an EfficientNet /
// MobileNetV3 step, on caller-provided buffers.  [M][C] tensors are bf16 with C the padded channel count (a multiple of
// 64), parameters exist for c < c_log. ----
namespace {
bool padded_ok(int C, int c_log) { return C >= 64 && C % 64 == 0 && c_log >= 1 && c_log <= C; }
}  // namespace

extern "C" int spk_op_dw_train(const void* x, const void* dy, const float* w, void* y, void* dx, float* dw, int accumulate,
                               int n, int h, int wd, int C, int c_log, int k, int stride, int pad, void* stream) {
  if (!x || !w || n < 1 || h < 1 || wd < 1 || pad < 0 || ((dx || dw) && !dy) || (!y && !dx && !dw))
    return ofail(SPK_ERR_ARG, "op_dw_train: bad arguments");
  if (!padded_ok(C, c_log) || spk_dw_fwd_form(k, stride, pad) == SPK_DW_FORM_NONE ||
      spk_dw_dgrad_form(k, stride, pad, accumulate) == SPK_DW_FORM_NONE)
    return ofail(SPK_ERR_UNSUPPORTED, "op_dw_train: C a multiple of 64, k 3 or 5, stride 1 or 2");
  const int ho = (h + 2 * pad - k) / stride + 1, wo = (wd + 2 * pad - k) / stride + 1;
  if (h + 2 * pad < k || wd + 2 * pad < k || ho < 1 || wo < 1) return ofail(SPK_ERR_ARG, "op_dw_train: empty output");
  if ((size_t)n * h * wd * C >= ((size_t)1 << 31) || (size_t)n * ho * wo * C >= ((size_t)1 << 31))
    return ofail(SPK_ERR_UNSUPPORTED, "op_dw_train: a tensor of 2^31 elements or more");
  hipStream_t s = (hipStream_t)stream;
  const int taps = k * k, M = n * ho * wo;
  Scratch sc;
  float* wt = sc.get<float>((size_t)2 * taps * C);   // the window and its flipped copy, as the step packs them
  float* unit = sc.get<float>((size_t)2 * C);
  const int cap = dw ? spk_dw_wgrad_rows(M, C) : 0;
  float* slabs = sc.get<float>((size_t)cap * c_log * taps);
  if (!wt || !unit || !slabs) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  std::vector<float> hu((size_t)2 * C, 0.f);
  std::fill(hu.begin(), hu.begin() + C, 1.f);
  if (hipMemcpyAsync(unit, hu.data(), hu.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return ofail(SPK_ERR_HIP, "op_dw_train: staging failed");
  PadPackTable tab;
  memset(&tab, 0, sizeof tab);
  tab.e[0].src = 0; tab.e[0].dst = 0;
  tab.e[0].cout = (unsigned)c_log; tab.e[0].taps = (unsigned)taps; tab.e[0].cout_p = (unsigned)C; tab.e[0].kind = 2;
  tab.count = 1;
  O_TRY(spk_launch_pack_padded_multi(w, nullptr, wt, tab, s), "dw_pack");
  if (y)
    O_TRY(spk_dw_train_forward((const bf16_t*)x, wt, unit, (size_t)C, (bf16_t*)y, n, h, wd, C, k, stride, pad, ho, wo, s),
          "depthwise fwd");
  if (dx)
    O_TRY(spk_dw_train_dgrad((const bf16_t*)dy, wt, unit, (size_t)C, (bf16_t*)dx, accumulate != 0, n, h, wd, C, k, stride,
                             pad, ho, wo, s), "depthwise dgrad");
  if (dw) {
    int rows = 0;
    const WalkGeometry g = spk_dw_wgrad_geometry(n * ho * ((wo + 3) / 4), C);
    if (g.blocks > cap) return ofail(SPK_ERR_STATE, "op_dw_train: spk_dw_wgrad_rows is smaller than the launch's partial rows");
    O_TRY(spk_launch_dw_wgrad((const bf16_t*)x, (const bf16_t*)dy, slabs, n, h, wd, C, c_log, k, stride, pad, ho, wo, &rows,
                              s), "depthwise wgrad");
    O_TRY(spk_launch_slab_reduce(slabs, dw, (size_t)c_log * taps, rows, s), "depthwise wgrad reduce");
  }
  O_SYNC(s, "op_dw_train: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_bna_forward(const void* raw, const float* gamma, const float* beta, float* running_mean,
                                  float* running_var, const void* res, const float* rowscale, void* out, float* pool_part,
                                  float* st, int n, int HW, int C, int c_log, int act, float eps, float momentum,
                                  void* stream) {
  if (!raw || !gamma || !beta || !running_mean || !running_var || !out || !st || n < 1 || HW < 1 || act < 0 || act > 3 ||
      (pool_part && (res || rowscale)))
    return ofail(SPK_ERR_ARG, "op_bna_forward: bad arguments (the pooling form has no shortcut and no row factor)");
  if (!padded_ok(C, c_log) || (size_t)n * HW * C >= ((size_t)1 << 31))
    return ofail(SPK_ERR_UNSUPPORTED, "op_bna_forward: C a multiple of 64, fewer than 2^31 elements");
  hipStream_t s = (hipStream_t)stream;
  const int M = n * HW;
  Scratch sc;
  float* part = sc.get<float>((size_t)spk_walk_geometry(M, C).blocks * 2 * C);
  float* tmp = sc.get<float>((size_t)C * 2 * 64);
  if (!part || !tmp) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  int nbk = 0;
  O_TRY(spk_launch_col_stats((const bf16_t*)raw, part, M, C, &nbk, s), "col_stats");
  O_TRY(spk_launch_bna_finalize(part, nbk, C, c_log, (double)M, gamma, beta, running_mean, running_var, st, eps, momentum,
                                tmp, s), "bn_finalize");
  if (pool_part)
    O_TRY(spk_launch_bna_apply_pool((const bf16_t*)raw, st + 2 * C, st + 3 * C, (bf16_t*)out, pool_part, n, HW, C, act, s),
          "bn_apply + squeeze");
  else
    O_TRY(spk_launch_bna_apply((const bf16_t*)raw, st + 2 * C, st + 3 * C, (const bf16_t*)res, rowscale, (bf16_t*)out, M, C,
                               HW, act, s), "bn_apply");
  O_SYNC(s, "op_bna_forward: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_bna_backward(const void* g, const void* raw, const float* st, const float* gamma,
                                   const float* rowscale, void* dy, float* dgamma, float* dbeta, void* g_res,
                                   int res_accumulate, int n, int HW, int C, int c_log, int act, void* stream) {
  if (!g || !raw || !st || !gamma || !dy || n < 1 || HW < 1 || act < 0 || act > 3)
    return ofail(SPK_ERR_ARG, "op_bna_backward: bad arguments");
  if (!padded_ok(C, c_log) || (size_t)n * HW * C >= ((size_t)1 << 31))
    return ofail(SPK_ERR_UNSUPPORTED, "op_bna_backward: C a multiple of 64, fewer than 2^31 elements");
  hipStream_t s = (hipStream_t)stream;
  const int M = n * HW;
  Scratch sc;
  float* part = sc.get<float>((size_t)spk_walk_geometry(M, C).blocks * 2 * C);
  float* coef = sc.get<float>((size_t)3 * C);
  float* tmp = sc.get<float>((size_t)C * 2 * 64);
  if (!part || !coef || !tmp) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  int nbk = 0;
  O_TRY(spk_launch_bna_bwd_reduce((const bf16_t*)g, (const bf16_t*)raw, st + 2 * C, st + 3 * C, st, st + C, rowscale, part,
                                  M, C, HW, act, &nbk, s), "bn bwd reduce");
  O_TRY(spk_launch_bna_bwd_finalize(part, nbk, C, c_log, (double)M, gamma, st + C, dgamma, dbeta, coef, tmp, s),
        "bn bwd finalize");
  O_TRY(spk_launch_bna_bwd_apply((const bf16_t*)g, (const bf16_t*)raw, st + 2 * C, st + 3 * C, st, st + C, coef, rowscale,
                                 (bf16_t*)dy, (bf16_t*)g_res, g_res ? res_accumulate != 0 : 0, M, C, HW, act, s),
        "bn bwd apply");
  O_SYNC(s, "op_bna_backward: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_se_train_forward(const void* a, const float* pool_part, const float* W1, const float* b1,
                                       const float* W2, const float* b2, float* pooled, float* u1, float* h1, float* gate,
                                       void* out, int n, int HW, int C, int Cl, int S, int gate_kind, void* stream) {
  if ((!a && !pool_part) || (out && !a) || !W1 || !b1 || !W2 || !b2 || !pooled || !u1 || !h1 || !gate || n < 1 || HW < 1 ||
      S < 1)
    return ofail(SPK_ERR_ARG, "op_se_train_forward: bad arguments");
  if (!padded_ok(C, Cl) || S > 256 || (gate_kind != 0 && gate_kind != 1) || (size_t)n * HW * C >= ((size_t)1 << 31))
    return ofail(SPK_ERR_UNSUPPORTED, "op_se_train_forward: C a multiple of 64, 256 hidden units at most, gate kind 0 or 1");
  hipStream_t s = (hipStream_t)stream;
  const int chunks = spk_se_chunks(HW);
  Scratch sc;
  float* part = sc.get<float>(pool_part ? 1 : (size_t)n * chunks * C);
  if (!part) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  // pad columns of the saved vectors: zeroed once by the step's plan, never written by the kernels
  if (hipMemsetAsync(pooled, 0, (size_t)n * C * 4, s) != hipSuccess || hipMemsetAsync(gate, 0, (size_t)n * C * 4, s) != hipSuccess)
    return ofail(SPK_ERR_HIP, "op_se_train_forward: memset failed");
  if (!pool_part) O_TRY(spk_launch_pool_rows((const bf16_t*)a, nullptr, part, n, HW, C, s), "se pool");
  O_TRY(spk_launch_se_gate_fwd(pool_part ? pool_part : part, chunks, 1.f / (float)HW, pooled, W1, b1, W2, b2, u1, h1, gate, n,
                               C, Cl, S, s, gate_kind), "se gates");
  if (out) O_TRY(spk_launch_se_scale((const bf16_t*)a, gate, (bf16_t*)out, n, HW, C, s), "se scale");
  O_SYNC(s, "op_se_train_forward: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_se_train_backward(const void* g, const void* a, const float* gate, const float* u1, const float* h1,
                                        const float* pooled, const float* W1, const float* W2, float* du2, float* du1,
                                        float* pool_part, void* da, float* gW1, float* gb1, float* gW2, float* gb2, int n,
                                        int HW, int C, int Cl, int S, int gate_kind, void* stream) {
  if (!h1 || !pooled || !du2 || !du1 || n < 1 || HW < 1 || S < 1 || (g && (!a || !gate || !u1 || !W1 || !W2 || !da)) ||
      (!g && (da || pool_part)))
    return ofail(SPK_ERR_ARG, "op_se_train_backward: bad arguments");
  if (!padded_ok(C, Cl) || S > 256 || (gate_kind != 0 && gate_kind != 1) || (size_t)n * HW * C >= ((size_t)1 << 31))
    return ofail(SPK_ERR_UNSUPPORTED, "op_se_train_backward: C a multiple of 64, 256 hidden units at most, gate kind 0 or 1");
  hipStream_t s = (hipStream_t)stream;
  const int chunks = spk_se_chunks(HW), tiles = spk_se_gate_tiles(Cl, S);
  Scratch sc;
  float* part = sc.get<float>(pool_part || !g ? 1 : (size_t)n * chunks * C);
  float* dpool = sc.get<float>((size_t)n * C);
  float* tpart = sc.get<float>((size_t)n * tiles * S);
  if (!part || !dpool || !tpart) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  if (pool_part) part = pool_part;
  if (g) {   // g == NULL: the parameter gradients alone, from the caller's du2 / du1
    if (hipMemsetAsync(du2, 0, (size_t)n * C * 4, s) != hipSuccess || hipMemsetAsync(dpool, 0, (size_t)n * C * 4, s) != hipSuccess)
      return ofail(SPK_ERR_HIP, "op_se_train_backward: memset failed");
    O_TRY(spk_launch_pool_rows((const bf16_t*)g, (const bf16_t*)a, part, n, HW, C, s), "se dgate");
    O_TRY(spk_launch_se_gate_bwd(part, chunks, du2, gate, u1, W1, W2, du1, dpool, tpart, n, C, Cl, S, s, gate_kind),
          "se gates bwd");
  }
  if (spk_launch_se_wgrad(du2, h1, du1, pooled, gW1, gb1, gW2, gb2, n, C, Cl, S, s) != 0)
    return ofail(SPK_ERR_HIP, "se wgrad failed");
  if (g) O_TRY(spk_launch_se_bwd_apply((const bf16_t*)g, gate, dpool, (bf16_t*)da, n, HW, C, s), "se bwd apply");
  O_SYNC(s, "op_se_train_backward: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_stem3_train(const void* x, const float* w, const void* dy, void* y, float* dw, int n, int h, int wd,
                                  int cin, int cout, int C, void* stream) {
  if (!x || (!y && !dw) || (y && !w) || (dw && !dy) || n < 1 || h < 1 || wd < 1 || cin < 1 || cin > 4)
    return ofail(SPK_ERR_ARG, "op_stem3_train: bad arguments");
  if (!padded_ok(C, cout) || cout * 9 > 768 || (size_t)n * h * wd * C >= ((size_t)1 << 31))
    return ofail(SPK_ERR_UNSUPPORTED, "op_stem3_train: C a multiple of 64, 85 output channels at most");
  hipStream_t s = (hipStream_t)stream;
  const int wstride = (wd + 1) & ~1, ho = (h - 1) / 2 + 1, wo = (wd - 1) / 2 + 1, M = n * ho * wo;
  if (y)
    O_TRY(spk_launch_stem3_train_fwd((const bf16_t*)x, w, (bf16_t*)y, n, h, wd, wstride, cin, cout, C, ho, wo, s,
                                     1.0f / SPK_INPUT_SCALE), "stem3 fwd");
  if (dw) {
    int ppb, nbk = 0;
    Scratch sc;
    float* slabs = sc.get<float>((size_t)spk_stem3_wgrad_blocks(M, &ppb) * cout * 9 * cin);
    if (!slabs) return ofail(SPK_ERR_HIP, "hipMalloc failed");
    O_TRY(spk_launch_stem3_wgrad((const bf16_t*)x, (const bf16_t*)dy, slabs, n, h, wd, wstride, cin, cout, C, ho, wo, &nbk, s),
          "stem3 wgrad");
    O_TRY(spk_launch_slab_reduce(slabs, dw, (size_t)cout * 9 * cin, nbk, s, 1.0f / SPK_INPUT_SCALE), "stem3 wgrad reduce");
    O_SYNC(s, "op_stem3_train: kernel failed");   // (slabs die here)
    return SPK_OK;
  }
  O_SYNC(s, "op_stem3_train: kernel failed");
  return SPK_OK;
}

// What the launchers of train_effnet.hip would choose for a problem (host only, no GPU): see include/sykepic_hip.h
extern "C" int spk_op_mbconv_geometry(int kind, int M, int C, int HW, int S, int out[8]) {
  if (!out) return ofail(SPK_ERR_ARG, "op_mbconv_geometry: bad arguments");
  for (int i = 0; i < 8; ++i) out[i] = 0;
  auto put = [&](const WalkGeometry& g) {
    out[0] = g.rows_per_block; out[1] = g.blocks; out[2] = g.ctiles; out[3] = g.tile_channels; out[4] = g.rows_in_flight;
    out[5] = g.idle_threads;
    out[6] = C / 8 - (g.ctiles - 1) * (g.tile_channels / 8);   // 8-channel groups of the last tile
  };
  switch (kind) {
    case 0:
    case 1:
      if (M < 1 || C < 64 || C % 64) return ofail(SPK_ERR_ARG, "op_mbconv_geometry: bad arguments");
      put(kind == 0 ? spk_walk_geometry(M, C) : spk_dw_wgrad_geometry(M, C));
      return SPK_OK;
    case 2:
      if (HW < 1 || C < 64 || C % 64) return ofail(SPK_ERR_ARG, "op_mbconv_geometry: bad arguments");
      put(spk_pool_geometry(HW, C));
      return SPK_OK;
    case 3:
      if (M < 1 || S < 1) return ofail(SPK_ERR_ARG, "op_mbconv_geometry: bad arguments");
      if (S > 256) return ofail(SPK_ERR_UNSUPPORTED, "op_mbconv_geometry: 256 hidden units at most");
      out[0] = spk_se_tile_rows(S); out[1] = spk_se_gate_tiles(M, S); out[2] = spk_se_bwd1_nq(S); out[3] = spk_se_wgrad_sj(S);
      out[4] = (M + 63) / 64;   // blocks of se_wgrad per job
      return SPK_OK;
    case 4:
      out[0] = spk_dw_fwd_form(M, C, HW);
      out[1] = spk_dw_dgrad_form(M, C, HW, S);
      return SPK_OK;
  }
  return ofail(SPK_ERR_ARG, "op_mbconv_geometry: kind 0 ... 4");
}

// ---- the MBConv EVAL kernels and the eval stems, one layer at a time: the pack and launch calls spk_commit
// (model_pack.hip) and run_conv_eval / spk_run_layer_eval (model.hip) make for a padded-channel 1x1 conv (with or without the squeeze-
// excitation gates in its operand), a squeeze-excitation layer, the 3x3/2 RGB stem and the 7x7/2 ResNet stem (with or
// without the fused max-pool), on caller-provided fp16 buffers.  Arguments are checked before any HIP call. ----
namespace {
int pad64(int c) { return (c + 63) / 64 * 64; }
bool act_ok(int act) { return act == SPK_ACT_NONE || act == SPK_ACT_RELU || act == SPK_ACT_SILU || act == SPK_ACT_HSWISH; }
// folded BatchNorm vectors as spk_commit lays them out: [scale x factor | shift], cout_p entries each, zeros on padding
float* staged_scale_bias(Scratch& sc, const float* scale, const float* bias, int cout, int cout_p, float factor, hipStream_t s) {
  float* f = sc.get<float>((size_t)2 * cout_p);
  if (!f) return nullptr;
  if (hipMemsetAsync(f, 0, (size_t)2 * cout_p * 4, s) != hipSuccess ||
      hipMemcpyAsync(f, scale, (size_t)cout * 4, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemcpyAsync(f + cout_p, bias, (size_t)cout * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return nullptr;
  if (factor != 1.f && spk_launch_scale_inplace(f, factor, cout, s)) return nullptr;
  return f;
}
}  // namespace

extern "C" int spk_op_conv1x1_padded(const void* x, const float* w, const float* bn_scale, const float* bn_bias,
                                     const void* res, const float* gate, void* y, int n, int h, int wd, int cin, int cout,
                                     int act, int split, void* stream) {
  if (!x || !w || !bn_scale || !bn_bias || !y || n < 1 || h < 1 || wd < 1 || cin < 8 || cout < 8 || cin % 8 || cout % 8 ||
      !act_ok(act))
    return ofail(SPK_ERR_ARG, "op_conv1x1_padded: bad arguments (channels multiples of 8, act 0 ... 3)");
  const int cin_p = pad64(cin), cout_p = pad64(cout);
  ConvGeom g = spk_conv_geom(n, h, wd, cin_p, cout_p, 1, 1, 0);   // the GEMM is padded to 64, ...
  g.Cs = cin;                                                     // ... the tensors are not
  g.Cos = cout;
  hipStream_t s = (hipStream_t)stream;
  Scratch sc;
  bf16_t* wp = sc.get<bf16_t>((size_t)2 * cout_p * cin_p);
  if (!wp) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  float* sb = staged_scale_bias(sc, bn_scale, bn_bias, cout, cout_p, 1.f, s);
  if (!sb) return ofail(SPK_ERR_HIP, "op_conv1x1_padded: staging failed");
  ConvArgs a = spk_conv_args(g, (const bf16_t*)x, wp, (bf16_t*)y, (const bf16_t*)res, sb, sb + cout_p, act, DT_F16, split != 0);
  if (!spk_below_2gib(a))
    return ofail(SPK_ERR_UNSUPPORTED, "op_conv1x1_padded: an operand of 2 GiB or more (split the batch)");
  O_TRY(spk_launch_pack_padded(w, wp, cout, 1, cin, cout_p, cin_p, DT_F16, split != 0, s), "pack_padded");
  if (gate) spk_set_gate(a, gate, cin);
  O_CONV(spk_conv_launch(a, CONV_MODE_GENERIC, s, nullptr), "padded conv1x1 launch");
  O_SYNC(s, "op_conv1x1_padded: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_se_eval(const void* x, const float* partial, int chunks, const float* w1, const float* b1,
                              const float* w2, const float* b2, float* hid_out, float* scale_out, void* y, int n, int hw,
                              int c, int sq, int gate_kind, void* stream) {
  if (!partial || !w1 || !b1 || !w2 || !b2 || !hid_out || !scale_out || (y && !x) || chunks < 1 || n < 1 || hw < 1 ||
      c < 8 || c % 8 || sq < 1 || (gate_kind != 0 && gate_kind != 1))
    return ofail(SPK_ERR_ARG, "op_se_eval: bad arguments (c a multiple of 8, gate kind 0 or 1)");
  // spk_launch_se keeps its hidden vector directly behind the gates, as the model's scratch does
  if (hid_out != scale_out + (size_t)n * c)
    return ofail(SPK_ERR_ARG, "op_se_eval: hid_out must be scale_out + n * c (one buffer, the layout of the model's scratch)");
  if ((size_t)n * hw * c >= ((size_t)1 << 31) || (size_t)n * chunks * c >= ((size_t)1 << 31))
    return ofail(SPK_ERR_UNSUPPORTED, "op_se_eval: a tensor of 2^31 elements or more");
  hipStream_t s = (hipStream_t)stream;
  Scratch sc;
  float* w2t = sc.get<float>((size_t)sq * c);
  if (!w2t) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  O_TRY(spk_launch_pack_tapmajor(w2, w2t, c, sq, c, s), "pack_tapmajor");
  O_TRY(spk_launch_se(y ? (const bf16_t*)x : nullptr, (bf16_t*)y, partial, chunks, scale_out, w1, b1, w2t, b2, n, hw, c, c,
                      sq, DT_F16, s, gate_kind), "squeeze-excitation");
  O_SYNC(s, "op_se_eval: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_stem3_eval(const void* x, const float* w, const float* bn_scale, const float* bn_bias, void* y, int n,
                                 int h, int wd, int cout, int act, void* stream) {
  if (!x || !w || !bn_scale || !bn_bias || !y || n < 1 || h < 1 || wd < 1 || cout < 8 || cout % 8 || !act_ok(act))
    return ofail(SPK_ERR_ARG, "op_stem3_eval: bad arguments (cout a multiple of 8, act 0 ... 3)");
  if (cout > 256) return ofail(SPK_ERR_UNSUPPORTED, "op_stem3_eval: 256 output channels at most");
  hipStream_t s = (hipStream_t)stream;
  const int cout_p = pad64(cout), wst = (wd + 1) & ~1, ho = (h - 1) / 2 + 1, wo = (wd - 1) / 2 + 1;
  Scratch sc;
  float* wt = sc.get<float>((size_t)36 * cout_p);
  if (!wt) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  float* sb = staged_scale_bias(sc, bn_scale, bn_bias, cout, cout_p, 1.0f / SPK_INPUT_SCALE, s);
  if (!sb) return ofail(SPK_ERR_HIP, "op_stem3_eval: staging failed");
  O_TRY(spk_pack_stem3(w, wt, cout, 3, cout_p, s), "pack_stem3");
  const int r = spk_launch_stem3x3((const bf16_t*)x, wt, sb, sb + cout_p, (bf16_t*)y, n, h, wst, wst, ho, wo, cout, cout_p,
                                   act, DT_F16, s);
  if (r == -2) return ofail(SPK_ERR_UNSUPPORTED, "op_stem3_eval: shape not supported");
  if (r) return ofail(SPK_ERR_HIP, "op_stem3_eval: launch failed");
  O_SYNC(s, "op_stem3_eval: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_stem7_eval(const void* x, const float* w, const float* bn_scale, const float* bn_bias, void* y,
                                 void* pool_y, int n, int h, int wd, int split, void* stream) {
  if (!x || !w || !bn_scale || !bn_bias || (!y && !pool_y) || n < 1 || h < 1 || wd < 1)
    return ofail(SPK_ERR_ARG, "op_stem7_eval: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const ConvGeom g = spk_stem_geom(n, h, wd);
  Scratch sc;
  bf16_t* wp = sc.get<bf16_t>((size_t)2 * g.Cout * g.K);
  if (!wp) return ofail(SPK_ERR_HIP, "hipMalloc failed");
  float* sb = staged_scale_bias(sc, bn_scale, bn_bias, 64, 64, 1.0f / SPK_INPUT_SCALE, s);
  if (!sb) return ofail(SPK_ERR_HIP, "op_stem7_eval: staging failed");
  ConvArgs a = spk_conv_args(g, (const bf16_t*)x, wp, (bf16_t*)y, nullptr, sb, sb + 64, 1, DT_F16, split != 0);
  if (!spk_below_2gib(a))
    return ofail(SPK_ERR_UNSUPPORTED, "op_stem7_eval: an operand of 2 GiB or more (split the batch)");
  O_TRY(spk_launch_pack_weights(w, wp, 64, 7, 7, 3, CONV_MODE_STEM, DT_F16, split != 0, s), "pack_weights");
  if (pool_y) {   // the max-pool layer that follows is computed by the stem kernel: only the pooled tensor is written
    a.pool_y = (bf16_t*)pool_y;
    a.pool_ho = (g.Ho - 1) / 2 + 1;
    a.pool_wo = (g.Wo - 1) / 2 + 1;
  }
  O_CONV(spk_conv_launch(a, CONV_MODE_STEM, s, nullptr), "stem launch");
  O_SYNC(s, "op_stem7_eval: kernel failed");
  return SPK_OK;
}

// What the launchers of the eval kernels above would choose for a problem (host only, no GPU): include/sykepic_hip.h
extern "C" int spk_op_mbconv_eval_geometry(int kind, int a, int b, int c, int d, int out[8]) {
  if (!out) return ofail(SPK_ERR_ARG, "op_mbconv_eval_geometry: bad arguments");
  for (int i = 0; i < 8; ++i) out[i] = 0;
  switch (kind) {
    case 0: {   // squeeze-excitation gates: a = n, b = chunks, c = channels, d = hidden units
      if (a < 1 || b < 1 || c < 8 || c % 8 || d < 1) return ofail(SPK_ERR_ARG, "op_mbconv_eval_geometry: bad arguments");
      const int ipb = spk_se_ipb();
      out[0] = spk_se_fc1_ch(b);                               // CH instantiation of se_fc1 (0: the run-time loop)
      out[1] = out[0] ? 0 : (b + 3) / 4 * 4 - b;               // run-time loop: clamped surplus loads of its last step
      out[2] = a - (a - 1) / ipb * ipb;                        // images of the last block (nim)
      out[3] = (d + 3) / 4 * 4 - d;                            // hidden units the last fc1 block row leaves out
      out[4] = (d * ipb + spk_se_fc2_stage() - 1) / spk_se_fc2_stage();   // staging passes of se_fc2
      out[5] = (c + 255) / 256;                                // channel tiles of se_fc2 (blockIdx.y)
      out[6] = c - (out[5] - 1) * 256;                         // channels of the last one
      out[7] = (a + ipb - 1) / ipb;                            // image blocks
      return SPK_OK;
    }
    case 1: {   // se_scale: a = n, b = hw, c = channels
      if (a < 1 || b < 1 || c < 8 || c % 8) return ofail(SPK_ERR_ARG, "op_mbconv_eval_geometry: bad arguments");
      const size_t per_img = (size_t)b * (c / 8);
      out[0] = spk_se_scale_grid(a, per_img);
      out[1] = (int)((per_img + 255) / 256);                   // blocks that would cover an image once
      return SPK_OK;
    }
    case 2: {   // 3x3 stem: a = ho, b = wo, c = cout
      if (a < 1 || b < 1 || c < 8 || c % 8) return ofail(SPK_ERR_ARG, "op_mbconv_eval_geometry: bad arguments");
      out[0] = spk_stem3_gt(c);
      return SPK_OK;
    }
    case 3: {   // padded / gated 1x1 conv: a = tile config, b = flavour, c = GEMM couts, d = split weights + 2 x gated
      if (a < 0 || a > 6 || b < 0 || b > 6 || c < 64 || c % 64 || d < 0 || d > 3)
        return ofail(SPK_ERR_ARG, "op_mbconv_eval_geometry: bad arguments");
      out[0] = spk_conv_narrow_cfg(a, c, d & 1);
      out[1] = spk_conv_padc_flavour(b, (d & 2) != 0);         // DMA template argument, or -3: not instantiated
      return SPK_OK;
    }
  }
  return ofail(SPK_ERR_ARG, "op_mbconv_eval_geometry: kind 0 ... 3");
}

// ---- the classifier head, the loss and the pooling layers (head.hip, pointwise.hip, train_kernels.hip), one layer at a
// time through the launchers model.hip and train.hip call.  Arguments are checked before any HIP call. ----
namespace {
bool below_2g(size_t a, size_t b, size_t c = 1, size_t d = 1) { return a * b * c * d < ((size_t)1 << 31); }
}  // namespace

extern "C" int spk_op_linear(const float* x, const float* w, const float* b, float* y, int n, int in, int out, void* stream) {
  if (!x || !w || !y || n < 1 || in < 1 || out < 1) return ofail(SPK_ERR_ARG, "op_linear: bad arguments");
  if (!below_2g(n, in) || !below_2g(out, in) || !below_2g(n, out))
    return ofail(SPK_ERR_UNSUPPORTED, "op_linear: a tensor of 2^31 elements or more");
  hipStream_t s = (hipStream_t)stream;
  O_TRY(spk_launch_linear_fwd(x, w, b, y, n, in, out, s), "linear");
  O_SYNC(s, "op_linear: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_linear_backward(const float* gy, const float* x, const float* w, float* dw, float* db, float* dx, int n,
                                      int in, int out, int form, void* stream) {
  if (!gy || (!dw && !db && !dx) || (dw && !x) || (dx && !w) || n < 1 || in < 1 || out < 1 || form < -1 || form > 1)
    return ofail(SPK_ERR_ARG, "op_linear_backward: bad arguments (form -1, 0 or 1)");
  if (!below_2g(n, in) || !below_2g(out, in) || !below_2g(n, out))
    return ofail(SPK_ERR_UNSUPPORTED, "op_linear_backward: a tensor of 2^31 elements or more");
  hipStream_t s = (hipStream_t)stream;
  O_TRY(spk_linear_backward(gy, x, w, dw, db, dx, n, in, out, form, s), "linear backward");
  O_SYNC(s, "op_linear_backward: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_softmax(const float* z, float* p, int n, int c, float base, void* stream) {
  if (!z || !p || n < 1 || c < 1 || !(base > 0.f)) return ofail(SPK_ERR_ARG, "op_softmax: bad arguments");
  if (!below_2g(n, c)) return ofail(SPK_ERR_UNSUPPORTED, "op_softmax: a tensor of 2^31 elements or more");
  hipStream_t s = (hipStream_t)stream;
  O_TRY(spk_launch_softmax(z, p, n, c, logf(base), s), "softmax");
  O_SYNC(s, "op_softmax: kernel failed");
  return SPK_OK;
}

namespace {
// what every cross-entropy hook passes on; the rest of CeArgs keeps its defaults unless the hook has it
CeArgs ce_args(const float* z, const int64_t* y, int n, int c, float* stats, float* dz, bool plain) {
  CeArgs a;
  a.z = z, a.ya = y, a.n = n, a.c = c, a.stats = stats, a.dz = dz, a.plain = plain;
  return a;
}
}  // namespace

extern "C" int spk_op_cross_entropy(const float* z, const int64_t* labels, int n, int c, float* stats, float* dz,
                                    void* stream) {
  if (!z || !labels || !stats || n < 1 || c < 1) return ofail(SPK_ERR_ARG, "op_cross_entropy: bad arguments");
  if (!below_2g(n, c)) return ofail(SPK_ERR_UNSUPPORTED, "op_cross_entropy: a tensor of 2^31 elements or more");
  hipStream_t s = (hipStream_t)stream;
  O_TRY(spk_launch_ce(ce_args(z, labels, n, c, stats, dz, true), s), "cross-entropy");
  O_SYNC(s, "op_cross_entropy: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_cross_entropy_ex(const float* z, const int64_t* labels, int n, int c, const float* w,
                                       float label_smoothing, float* stats, int* counts, float* dz, void* stream) {
  if (!z || !labels || !stats || n < 1 || c < 1) return ofail(SPK_ERR_ARG, "op_cross_entropy_ex: bad arguments");
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f))
    return ofail(SPK_ERR_ARG, "op_cross_entropy_ex: label_smoothing must be in [0, 1]");
  if (!below_2g(n, c)) return ofail(SPK_ERR_UNSUPPORTED, "op_cross_entropy_ex: a tensor of 2^31 elements or more");
  hipStream_t s = (hipStream_t)stream;
  CeArgs a = ce_args(z, labels, n, c, stats, dz, false);
  a.w = w, a.eps = label_smoothing, a.counts = counts;
  O_TRY(spk_launch_ce(a, s), "cross-entropy");
  O_SYNC(s, "op_cross_entropy_ex: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_cross_entropy_pair(const float* z, const int64_t* ya, const int64_t* yb, float lam, int n, int c,
                                         const float* w, float label_smoothing, float* stats, int* counts, float* dz,
                                         void* stream) {
  if (!z || !ya || !stats || n < 1 || c < 1) return ofail(SPK_ERR_ARG, "op_cross_entropy_pair: bad arguments");
  if (!(lam >= 0.f && lam <= 1.f)) return ofail(SPK_ERR_ARG, "op_cross_entropy_pair: lam must be in [0, 1]");
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f))
    return ofail(SPK_ERR_ARG, "op_cross_entropy_pair: label_smoothing must be in [0, 1]");
  if (!below_2g(n, c)) return ofail(SPK_ERR_UNSUPPORTED, "op_cross_entropy_pair: a tensor of 2^31 elements or more");
  hipStream_t s = (hipStream_t)stream;
  CeArgs a = ce_args(z, ya, n, c, stats, dz, false);
  a.yb = yb, a.lam = lam, a.w = w, a.eps = label_smoothing, a.counts = counts;
  O_TRY(spk_launch_ce(a, s), "cross-entropy");
  O_SYNC(s, "op_cross_entropy_pair: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_cross_entropy_distill(const float* z, const int64_t* ya, const int64_t* yb, float lam, const float* t,
                                            float alpha, float temperature, int n, int c, const float* w,
                                            float label_smoothing, float* stats, int* counts, float* kd_stats, float* dz,
                                            void* stream) {
  if (!z || !ya || !stats || n < 1 || c < 1) return ofail(SPK_ERR_ARG, "op_cross_entropy_distill: bad arguments");
  if (!(lam >= 0.f && lam <= 1.f)) return ofail(SPK_ERR_ARG, "op_cross_entropy_distill: lam must be in [0, 1]");
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f))
    return ofail(SPK_ERR_ARG, "op_cross_entropy_distill: label_smoothing must be in [0, 1]");
  if (!(alpha >= 0.f && alpha <= 1.f)) return ofail(SPK_ERR_ARG, "op_cross_entropy_distill: alpha must be in [0, 1]");
  if (!(temperature > 0.f) || !(temperature <= 3.4e38f))
    return ofail(SPK_ERR_ARG, "op_cross_entropy_distill: temperature must be a finite number above 0");
  if (kd_stats && !t) return ofail(SPK_ERR_ARG, "op_cross_entropy_distill: kd_stats without teacher logits");
  if (!below_2g(n, c)) return ofail(SPK_ERR_UNSUPPORTED, "op_cross_entropy_distill: a tensor of 2^31 elements or more");
  hipStream_t s = (hipStream_t)stream;
  CeArgs a = ce_args(z, ya, n, c, stats, dz, false);
  a.yb = yb, a.lam = lam, a.teacher = t, a.alpha = alpha, a.T = temperature;
  a.w = w, a.eps = label_smoothing, a.counts = counts, a.kd_stats = kd_stats;
  O_TRY(spk_launch_ce(a, s), "cross-entropy");
  O_SYNC(s, "op_cross_entropy_distill: kernel failed");
  return SPK_OK;
}

namespace {
// shared argument rules of the two max-pool hooks; 0 when the problem can run
int pool_args(const char* who, int n, int h, int w, int c, int k, int stride, int pad, int* ho, int* wo) {
  if (n < 1 || h < 1 || w < 1 || c < 8 || c % 8 || k < 1 || stride < 1 || pad < 0)
    return ofail(SPK_ERR_ARG, std::string(who) + ": bad arguments (c a multiple of 8)");
  if (k * k > 255 || k > 15 || pad > k / 2)
    return ofail(SPK_ERR_UNSUPPORTED, std::string(who) + ": the saved tap is one byte (k * k <= 255) and pad <= k / 2");
  if (h + 2 * pad < k || w + 2 * pad < k) return ofail(SPK_ERR_ARG, std::string(who) + ": empty output");
  *ho = (h + 2 * pad - k) / stride + 1;
  *wo = (w + 2 * pad - k) / stride + 1;
  if (!below_2g(n, h, w, c) || (size_t)n * h > 0x7fffffffull)
    return ofail(SPK_ERR_UNSUPPORTED, std::string(who) + ": a tensor of 2^31 elements or more");
  return SPK_OK;
}
}  // namespace

extern "C" int spk_op_maxpool(const void* x, void* y, unsigned char* idx, int n, int h, int w, int c, int k, int stride,
                              int pad, int dtype, void* stream) {
  if (!x || !y || (dtype != DT_BF16 && dtype != DT_F16)) return ofail(SPK_ERR_ARG, "op_maxpool: bad arguments");
  int ho = 0, wo = 0;
  if (const int r = pool_args("op_maxpool", n, h, w, c, k, stride, pad, &ho, &wo)) return r;
  if (idx && dtype != DT_BF16) return ofail(SPK_ERR_UNSUPPORTED, "op_maxpool: the kernel that saves the taps is bf16 only");
  hipStream_t s = (hipStream_t)stream;
  if (idx)
    O_TRY(spk_launch_maxpool_idx((const bf16_t*)x, (bf16_t*)y, idx, n, h, w, c, k, stride, pad, ho, wo, s), "maxpool");
  else
    O_TRY(spk_launch_maxpool((const bf16_t*)x, (bf16_t*)y, n, h, w, c, k, stride, pad, ho, wo, dtype, s), "maxpool");
  O_SYNC(s, "op_maxpool: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_maxpool_backward(const void* gy, const unsigned char* idx, void* gx, int n, int h, int w, int c, int k,
                                       int stride, int pad, int form, void* stream) {
  if (!gy || !idx || !gx || form < -1 || form > 1)
    return ofail(SPK_ERR_ARG, "op_maxpool_backward: bad arguments (form -1, 0 or 1)");
  int ho = 0, wo = 0;
  if (const int r = pool_args("op_maxpool_backward", n, h, w, c, k, stride, pad, &ho, &wo)) return r;
  if (form == 1 && !spk_maxpool_pair_ok(h, w, k, stride, pad, ho, wo))
    return ofail(SPK_ERR_UNSUPPORTED, "op_maxpool_backward: the pixel-pair kernel needs k 3, stride 2, pad 1 and an even width");
  hipStream_t s = (hipStream_t)stream;
  if (form < 0)
    O_TRY(spk_launch_maxpool_bwd((const bf16_t*)gy, idx, (bf16_t*)gx, n, h, w, c, k, stride, pad, ho, wo, s), "maxpool bwd");
  else
    O_TRY(spk_launch_maxpool_bwd_form((const bf16_t*)gy, idx, (bf16_t*)gx, n, h, w, c, k, stride, pad, ho, wo, form == 1, s),
          "maxpool bwd");
  O_SYNC(s, "op_maxpool_backward: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_gavgpool(const void* x, float* y, int n, int hw, int c, int dtype, void* stream) {
  if (!x || !y || n < 1 || hw < 1 || c < 8 || c % 8 || (dtype != DT_BF16 && dtype != DT_F16))
    return ofail(SPK_ERR_ARG, "op_gavgpool: bad arguments (c a multiple of 8)");
  if (n > 65535 || !below_2g(n, hw, c))
    return ofail(SPK_ERR_UNSUPPORTED, "op_gavgpool: more than 65535 images or a tensor of 2^31 elements or more");
  hipStream_t s = (hipStream_t)stream;
  O_TRY(spk_launch_gavgpool((const bf16_t*)x, y, n, hw, c, dtype, s), "avgpool");
  O_SYNC(s, "op_gavgpool: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_gavgpool_backward(const float* gy, void* gx, int n, int hw, int c, void* stream) {
  if (!gy || !gx || n < 1 || hw < 1 || c < 8 || c % 8)
    return ofail(SPK_ERR_ARG, "op_gavgpool_backward: bad arguments (c a multiple of 8)");
  if (!below_2g(n, hw, c)) return ofail(SPK_ERR_UNSUPPORTED, "op_gavgpool_backward: a tensor of 2^31 elements or more");
  hipStream_t s = (hipStream_t)stream;
  O_TRY(spk_launch_gavgpool_bwd(gy, (bf16_t*)gx, n, hw, c, s), "avgpool bwd");
  O_SYNC(s, "op_gavgpool_backward: kernel failed");
  return SPK_OK;
}

// ---- the two kernels of the weights' moving average (train_kernels.hip) on caller buffers: the launches
// spk_model_ema_update / spk_model_ema_swap make on the model's flat buffers ----
namespace {
// shared argument rules: two disjoint ranges of n >= 1 floats at 4-byte aligned addresses
int stream_pair_args(const char* who, const void* a, const void* b, int64_t n) {
  if (!a || !b) return ofail(SPK_ERR_ARG, std::string(who) + ": null pointer");
  if (n < 1) return ofail(SPK_ERR_ARG, std::string(who) + ": n < 1");
  const size_t ua = (size_t)a, ub = (size_t)b, bytes = (size_t)n * 4;
  if ((ua | ub) & 3) return ofail(SPK_ERR_ARG, std::string(who) + ": buffers not 4-byte aligned");
  if (ua < ub + bytes && ub < ua + bytes) return ofail(SPK_ERR_ARG, std::string(who) + ": the two ranges overlap");
  return SPK_OK;
}
}  // namespace

extern "C" int spk_op_ema_lerp(float* e, const float* p, int64_t n, float w, void* stream) {
  if (const int r = stream_pair_args("op_ema_lerp", e, p, n)) return r;
  if (!(w > 0.f && w < 1.f)) return ofail(SPK_ERR_ARG, "op_ema_lerp: w must be finite and inside (0, 1)");
  hipStream_t s = (hipStream_t)stream;
  O_TRY(spk_launch_ema_lerp(e, p, (size_t)n, w, s), "ema lerp");
  O_SYNC(s, "op_ema_lerp: kernel failed");
  return SPK_OK;
}

extern "C" int spk_op_swap_f32(float* a, float* b, int64_t n, void* stream) {
  if (const int r = stream_pair_args("op_swap_f32", a, b, n)) return r;
  hipStream_t s = (hipStream_t)stream;
  O_TRY(spk_launch_swap_f32(a, b, (size_t)n, s), "swap");
  O_SYNC(s, "op_swap_f32: kernel failed");
  return SPK_OK;
}
