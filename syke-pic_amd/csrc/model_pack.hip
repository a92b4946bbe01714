// Model handle: what a forward needs packed before it runs (host side, no kernel) - which convs split their weights,
// spk_commit (eval-BN fold + every packed weight image), the activation means of the zero-sum rounding, and the fp8
// roles, calibration and e4m3 weights of the MBConv interior.
#include "model.h"

#include <algorithm>
#include <cmath>
#include <cstring>

// ---------------------------------------------------------------------------
// commit: fold eval-BN into per-channel scale/bias, pack bf16 weights
// ---------------------------------------------------------------------------
// is this conv's single fp16 weight image zero-sum rounded against the calibrated input means?
static bool layer_zero_sum(const spk_model* m, const Layer& L) {
  return (m->zero_sum || m->splitw == 5) && m->have_means && m->infer_dt == DT_F16 && L.d.kind == SPK_OP_CONV &&
         (L.mode == CONV_MODE_GENERIC || L.mode == CONV_MODE_STEM) && !layer_split(m, L);
}

int spk_commit(spk_model* m) {
  const int zs_now = (m->zero_sum || m->splitw == 5) && m->have_means ? 1 : 0;
  if (!m->dirty && m->packed_dt == m->infer_dt && m->packed_split == (int)m->splitw &&
      m->packed_epoch == m->split_epoch && m->packed_zs == zs_now)
    return SPK_OK;
  // zero-sum rounded fp32 copy of one layer's weights at a time (the stream orders round -> pack -> next round)
  float* wround = nullptr;
  {
    size_t need = 0;
    for (const Layer& L : m->layers)
      if (layer_zero_sum(m, L)) need = std::max(need, (size_t)L.d.cout * L.d.k * L.d.k * L.d.cin);
    if (need) HIP_TRY(hipMalloc((void**)&wround, need * 4));
  }
  struct Free { float* p; hipStream_t s; ~Free() { if (p) { (void)hipStreamSynchronize(s); (void)hipFree(p); } } } free_wround{wround, m->stream};
  for (Layer& L : m->layers) {
    if (L.d.kind == SPK_OP_SE &&
        spk_launch_pack_tapmajor(m->P(L.p_w2), m->dwpack + L.wpack_off, L.d.cout, L.d.k, L.d.cout, m->stream))
      return spk_fail(SPK_ERR_HIP, "pack (squeeze-excitation) launch failed");
    if (L.d.kind != SPK_OP_CONV && L.d.kind != SPK_OP_DWCONV) continue;
    float* sc = m->scale_bias + L.sb_off;
    float* bi = sc + L.cout_p;
    if (L.cout_p != L.d.cout)  // padded output channels: scale = shift = 0
      HIP_TRY(hipMemsetAsync(sc, 0, (size_t)2 * L.cout_p * 4, m->stream));
    if (spk_launch_bn_fold(m->P(L.p_g), m->P(L.p_b), m->P(L.p_mean), m->P(L.p_var), m->bn_eps, sc, bi,
                           L.d.cout, m->stream))
      return spk_fail(SPK_ERR_HIP, "bn_fold launch failed");
    // the stems read pixel values x 255 (exact in 16 bits, spk_common.h SPK_INPUT_SCALE): their fp32 epilogue scale takes
    // the factor back
    if (L.d.kind == SPK_OP_CONV && (L.mode == CONV_MODE_STEM || L.mode == CONV_MODE_STEM3) &&
        spk_launch_scale_inplace(sc, 1.0f / SPK_INPUT_SCALE, L.d.cout, m->stream))
      return spk_fail(SPK_ERR_HIP, "stem scale launch failed");
    if (L.mode == CONV_MODE_GROUP) continue;   // fp32 master weights, no image (and no zero-sum rounding: nothing is rounded)
    int r;
    // the weights every image of this layer is packed from: the fp32 master, or its zero-sum rounded copy (values that
    // ARE fp16 numbers, so each pack kernel's own conversion is exact): master layout [cout][tap][cin], one balanced
    // group per (cout, tap), weighted with the input-channel means
    const float* wsrc = m->P(L.p_w);
    if (layer_zero_sum(m, L)) {
      // (the stem's 3-channel taps are too short to balance one by one: its 147-weight rows as a whole)
      const bool whole = L.mode == CONV_MODE_STEM;
      if (spk_launch_zero_sum_round(wsrc, m->act_mean_dev + L.mu_off, wround, (size_t)L.d.cout * (whole ? 1 : L.d.k * L.d.k),
                                    whole ? L.d.k * L.d.k * L.d.cin : L.d.cin, L.d.cin, m->stream))
        return spk_fail(SPK_ERR_HIP, std::string("zero-sum rounding launch failed for ") + L.d.name);
      wsrc = wround;
    }
    if (L.d.kind == SPK_OP_DWCONV)
      r = spk_launch_pack_tapmajor(m->P(L.p_w), m->dwpack + L.wpack_off, L.d.cout, L.d.k * L.d.k, L.d.cout, m->stream);
    else if (L.mode == CONV_MODE_STEM3)  // master [cout][kh][kw][cin<=3] -> fp32 [9 taps][4][cout_p]: rows = taps x 4 (cin padded to 4)
      r = spk_pack_stem3(m->P(L.p_w), m->dwpack + L.wpack_off, L.d.cout, L.d.cin, L.cout_p, m->stream);
    else if (L.mode == CONV_MODE_GENERIC && (L.cin_p != L.d.cin || L.cout_p != L.d.cout))
      r = spk_launch_pack_padded(wsrc, m->wpack + L.wpack_off, L.d.cout, L.d.k * L.d.k, L.d.cin, L.cout_p,
                                 L.cin_p, m->infer_dt, layer_split(m, L), m->stream);
    else
      r = spk_launch_pack_weights(wsrc, m->wpack + L.wpack_off, L.d.cout, L.d.k, L.d.k, L.d.cin,
                                  L.mode, m->infer_dt, layer_split(m, L), m->stream);
    if (r) return spk_fail(SPK_ERR_HIP, "pack_weights launch failed");
    // 1x1 convs: second image in MFMA fragment order (conv_pw.hip).  The BatchNorm scale is NOT folded into it: a
    // small scale would push the 16-bit weights into fp16's subnormal range (measured on the calibrated-statistics
    // golden fixture: every conv split, max |dp| 5.9e-4 with the scale in the fp32 epilogue, 1.1e-3 folded)
    if (L.pw_ok && m->infer_dt == DT_F16 &&
        spk_launch_pack_pw(wsrc, nullptr, m->wpack + L.wpw_off, L.d.cout, L.d.cin, DT_F16, layer_split(m, L) ? 2 : 1,
                           m->stream))
      return spk_fail(SPK_ERR_HIP, "pack_pw launch failed");
    if ((L.c3_ok || (L.bn_head >= 0 && L.d.k == 3)) && m->infer_dt == DT_F16 &&
        spk_launch_pack_c3(wsrc, m->wpack + L.wpw_off, L.d.cout, L.d.cin, layer_split(m, L) ? 2 : 1, m->stream))
      return spk_fail(SPK_ERR_HIP, "pack_c3 launch failed");
    // (from the same rounded values as the implicit GEMM's image above: master layout [cout][kh][kw][cin] = [cout][K])
    if (L.d3_ok && m->infer_dt == DT_F16 && !layer_split(m, L) &&
        spk_launch_pack_pw(wsrc, nullptr, m->wpack + L.wd3_off, L.d.cout, 9 * L.d.cin, DT_F16, 1, m->stream))
      return spk_fail(SPK_ERR_HIP, "pack_pw (3x3 panel) launch failed");
  }
  // fused (block-closing + shortcut) convs: K-concatenated weights with both eval-BN scales folded in, normalised per
  // cout by a power of two (exact in the fp32 epilogue), in fragment order
  {
    size_t tmp_floats = 0;
    for (Layer& L : m->layers) {
      L.dual_ok = false;
      if (L.dual_src < 0 || m->infer_dt != DT_F16) continue;
      const Layer& D = m->layers[L.dual_src];
      if ((layer_split(m, L) != 0) != (layer_split(m, D) != 0)) continue;   // one image, one precision
      tmp_floats = std::max(tmp_floats, (size_t)L.d.cout * (L.d.cin + D.d.cin));
    }
    float* wcat = nullptr;
    float* mucat = nullptr;   // dual + zero-sum: the two sources' channel means side by side, then the rounded copy
    bool dual_zs = false;
    for (const Layer& L : m->layers) dual_zs |= L.dual_src >= 0 && layer_zero_sum(m, L) && layer_zero_sum(m, m->layers[L.dual_src]);
    if (tmp_floats) HIP_TRY(hipMalloc((void**)&wcat, tmp_floats * 4 * (dual_zs ? 2 : 1) + (dual_zs ? 16384 * 4 : 0)));
    if (dual_zs) mucat = wcat + 2 * tmp_floats;
    for (Layer& L : m->layers) {
      if (L.dual_src < 0 || m->infer_dt != DT_F16) continue;
      const Layer& D = m->layers[L.dual_src];
      if ((layer_split(m, L) != 0) != (layer_split(m, D) != 0)) continue;
      const float* sL = m->scale_bias + L.sb_off;
      const float* sD = m->scale_bias + D.sb_off;
      float* sd = m->sdual + L.sdual_off;
      int r = spk_launch_pw_dual_prep(m->P(L.p_w), m->P(D.p_w), sL, sD, sL + L.cout_p, sD + D.cout_p, wcat, sd,
                                      sd + L.d.cout, L.d.cout, L.d.cin, D.d.cin, m->stream);
      const float* wc = wcat;
      if (!r && mucat && layer_zero_sum(m, L) && layer_zero_sum(m, D) && L.d.cin + D.d.cin <= 16384) {
        // the fused GEMM rounds the scale-folded concatenated rows: balance THOSE, against [means of y2 | means of x]
        const int K = L.d.cin + D.d.cin;
        if (hipMemcpyAsync(mucat, m->act_mean_dev + L.mu_off, (size_t)L.d.cin * 4, hipMemcpyDeviceToDevice, m->stream) != hipSuccess ||
            hipMemcpyAsync(mucat + L.d.cin, m->act_mean_dev + D.mu_off, (size_t)D.d.cin * 4, hipMemcpyDeviceToDevice,
                           m->stream) != hipSuccess)
          r = -1;
        if (!r) r = spk_launch_zero_sum_round(wcat, mucat, wcat + tmp_floats, (size_t)L.d.cout, K, K, m->stream);
        wc = wcat + tmp_floats;
      }
      if (!r) r = spk_launch_pack_pw(wc, nullptr, m->wdual + L.wdual_off, L.d.cout, L.d.cin + D.d.cin, DT_F16,
                                     layer_split(m, L) ? 2 : 1, m->stream);
      if (r) { (void)hipFree(wcat); return spk_fail(SPK_ERR_HIP, "dual-source weight packing failed"); }
      L.dual_ok = true;
    }
    if (wcat) {
      HIP_TRY(hipStreamSynchronize(m->stream));
      (void)hipFree(wcat);
    }
  }
  // new precision settings mean new tuner keys (nb, shortcut flags) for the same shapes: the next forward of every
  // shape runs on ONE stream again so that candidates are timed on a quiet GPU
  if (m->packed_dt != m->infer_dt || m->packed_split != (int)m->splitw || m->packed_epoch != m->split_epoch)
    m->half_warm.clear();
  m->packed_zs = zs_now;
  m->packed_dt = m->infer_dt;
  m->packed_split = (int)m->splitw;
  m->packed_epoch = m->split_epoch;
  m->dirty = false;
  m->fp8_packed = false;
  return SPK_OK;
}

// ---------------------------------------------------------------------------
// fp8 (e4m3) mode of the EfficientNet MBConv interior — BASELINE config 5
// ---------------------------------------------------------------------------
// expand 1x1 conv -> depthwise conv -> squeeze-excitation -> project 1x1 conv with e4m3 tensors in between
static int assign_fp8_roles(spk_model* m, bool count_only = false) {
  const int nl = (int)m->layers.size();
  int blk = 0;
  auto consumer = [&](int t, int* idx) { const Readers r = spk_readers_of(m, t); *idx = r.last; return r.total(); };
  if (!count_only)
    for (Layer& L : m->layers) L.fp8_role = 0;
  for (int i = 0; i < nl; ++i) {
    Layer& E = m->layers[i];
    if (!spk_expand_shaped(E.d)) continue;
    int di, si, pi;
    if (consumer(E.d.dst, &di) != 1 || m->layers[di].d.kind != SPK_OP_DWCONV) continue;
    if (consumer(m->layers[di].d.dst, &si) != 1 || m->layers[si].d.kind != SPK_OP_SE) continue;
    if (consumer(m->layers[si].d.dst, &pi) != 1) continue;
    Layer& P = m->layers[pi];
    if (P.d.kind != SPK_OP_CONV || P.d.k != 1 || P.d.stride != 1 || P.d.src != m->layers[si].d.dst) continue;
    const int idx = blk++;
    if (count_only) continue;
    // Default (no explicit flags): only blocks that ADD their branch to the trunk.  A block without a shortcut (the first
    // of every stage) replaces the trunk by its e4m3-computed output, ~10 % relative error on the trunk itself, and alone
    // flips more arg-maxes than all residual blocks together (tests/archive/diagnostics/fp8_block_sweep.py).
    if (m->fp8_blocks.empty() ? P.d.res < 0 : (idx >= (int)m->fp8_blocks.size() || !m->fp8_blocks[idx])) continue;
    E.fp8_role = 1; m->layers[di].fp8_role = 2; m->layers[si].fp8_role = 3; P.fp8_role = 4;
  }
  return blk;
}

extern "C" int spk_model_num_fp8_blocks(spk_model* m) { return m ? assign_fp8_roles(m, true) : 0; }

extern "C" int spk_model_set_fp8_blocks(spk_model* m, const unsigned char* flags, int n_blocks) {
  if (!m || n_blocks < 0 || (n_blocks > 0 && !flags)) return spk_fail(SPK_ERR_ARG, "set_fp8_blocks: bad arguments");
  if (n_blocks > 0 && n_blocks != assign_fp8_roles(m, true))
    return spk_fail(SPK_ERR_ARG, "set_fp8_blocks: one flag per qualifying MBConv block (spk_model_num_fp8_blocks)");
  m->fp8_blocks.assign(flags, flags + n_blocks);
  m->fp8_calibrated = false;     // roles are assigned by the next calibration
  m->fp8_packed = false;
  return SPK_OK;
}

extern "C" int spk_model_set_fp8(spk_model* m, int on) {
  if (!m) return spk_fail(SPK_ERR_ARG, "null model");
  if (on && !m->effnet) return spk_fail(SPK_ERR_UNSUPPORTED, "the fp8 mode covers the EfficientNet MBConv blocks only");
  if (on && m->mobilenet)
    return spk_fail(SPK_ERR_UNSUPPORTED, "the fp8 mode covers SiLU MBConv blocks only (this graph has Hardswish / Hardsigmoid)");
  m->fp8 = on ? 1 : 0;
  return SPK_OK;
}

static int fp8_amax(spk_model* m, int t, int nb, unsigned int* dev_word, float* out) {
  const TDim& d = m->tdims[t];
  HIP_TRY(hipMemsetAsync(dev_word, 0, 4, m->stream));
  if (spk_launch_absmax_f16((const bf16_t*)m->T(t), (size_t)nb * d.h * d.w * d.c / 8, dev_word, m->stream))
    return spk_fail(SPK_ERR_HIP, "absmax launch failed");
  unsigned int bits = 0;
  HIP_TRY(hipMemcpyAsync(&bits, dev_word, 4, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  memcpy(out, &bits, 4);
  return SPK_OK;
}

extern "C" int spk_model_calibrate_fp8(spk_model* m, const void* x, int n, int h, int w, int layout, int dtype) {
  if (!m || !x || n <= 0) return spk_fail(SPK_ERR_ARG, "calibrate_fp8: bad arguments");
  if (!m->effnet) return spk_fail(SPK_ERR_UNSUPPORTED, "the fp8 mode covers the EfficientNet MBConv blocks only");
  if (m->infer_dt != DT_F16) return spk_fail(SPK_ERR_STATE, "calibrate_fp8 needs the fp16 eval path");
  HIP_TRY(hipSetDevice(m->device));
  SPK_TRY(spk_plan(m, n, h, w));
  if (n > m->mb_limit) return spk_fail(SPK_ERR_ARG, "calibration batch too large for one pass");
  const int keep = m->fp8;
  m->fp8 = 0;                                    // the calibration forward itself runs in fp16
  float* logits = (float*)((char*)m->arena + m->logits_off);
  const int rc = spk_forward_eval_logits(m, x, n, h, w, layout, dtype, logits);
  m->fp8 = keep;
  if (rc != SPK_OK) return rc;
  assign_fp8_roles(m);
  unsigned int* word = nullptr;
  HIP_TRY(hipMalloc((void**)&word, 4));
  int r = SPK_OK;
  for (Layer& L : m->layers) {
    if (!L.fp8_role || L.fp8_role == 3) continue;
    if (L.fp8_role == 1 && (r = fp8_amax(m, L.d.src, n, word, &L.amax_in)) != SPK_OK) break;   // trunk entering the block
    if (L.fp8_role != 4 && (r = fp8_amax(m, L.d.dst, n, word, &L.amax_out)) != SPK_OK) break;  // expanded / depthwise out
  }
  (void)hipFree(word);
  if (r != SPK_OK) return r;
  // a layer's input range is its producer's output range
  for (Layer& L : m->layers) {
    if (L.fp8_role == 2)
      for (const Layer& Q : m->layers) if (Q.fp8_role == 1 && Q.d.dst == L.d.src) L.amax_in = Q.amax_out;
    if (L.fp8_role == 4) L.amax_in = m->layers[m->layers[L.src_se].se_dw].amax_out;   // (the depthwise conv of its block)
  }
  // storage for the e4m3 weights and their scales
  size_t wb = 0, sf = 0;
  for (Layer& L : m->layers) {
    if (L.fp8_role != 1 && L.fp8_role != 4) continue;
    const int kpad = (L.d.cin + 63) / 64 * 64;
    L.w8_off = wb; wb += (size_t)L.cout_p * kpad;
    L.s8_off = sf; sf += (size_t)2 * L.cout_p;
  }
  if (m->w8pack) { (void)hipFree(m->w8pack); m->w8pack = nullptr; }
  if (m->s8) { (void)hipFree(m->s8); m->s8 = nullptr; }
  HIP_TRY(hipMalloc((void**)&m->w8pack, std::max<size_t>(wb, 64)));
  HIP_TRY(hipMalloc((void**)&m->s8, std::max<size_t>(sf, 64) * 4));
  m->fp8_calibrated = true;
  m->fp8_packed = false;
  return SPK_OK;
}

int spk_fp8_pack(spk_model* m) {
  if (m->fp8_packed) return SPK_OK;
  for (Layer& L : m->layers) {
    if (L.fp8_role != 1 && L.fp8_role != 4) continue;
    const int kpad = (L.d.cin + 63) / 64 * 64;
    float* ws = m->s8 + L.s8_off;
    if (spk_launch_pack_fp8(m->P(L.p_w), m->w8pack + L.w8_off, ws, L.d.cout, L.d.cin, L.cout_p, kpad, 1.f, m->stream))
      return spk_fail(SPK_ERR_HIP, "fp8 weight packing failed");
    // epilogue factor = eval-BN scale x weight scale x scale of the A bytes
    if (spk_launch_mul3(m->scale_bias + L.sb_off, ws, spk_fp8_scale_of(L.amax_in), ws + L.cout_p, L.cout_p, m->stream))
      return spk_fail(SPK_ERR_HIP, "fp8 scale folding failed");
  }
  m->fp8_packed = true;
  return SPK_OK;
}

// ---------------------------------------------------------------------------
// activation means for zero-sum weight rounding (zero_sum.hip)
// ---------------------------------------------------------------------------
extern "C" int64_t spk_model_act_means_size(spk_model* m) { return m ? (int64_t)m->n_means : 0; }

extern "C" int spk_model_set_zero_sum(spk_model* m, int on) {
  if (!m) return spk_fail(SPK_ERR_ARG, "null model");
  m->zero_sum = on != 0;
  return SPK_OK;
}

extern "C" int spk_model_set_act_means(spk_model* m, const float* host, int64_t numel) {
  if (!m) return spk_fail(SPK_ERR_ARG, "null model");
  if (!host || numel == 0) {   // forget them
    m->have_means = false;
    m->act_mean.clear();
    m->packed_zs = -1;
    return SPK_OK;
  }
  if (numel != (int64_t)m->n_means) return spk_fail(SPK_ERR_ARG, "set_act_means: one value per input channel of every conv expected");
  for (int64_t i = 0; i < numel; ++i)
    if (!std::isfinite(host[i])) return spk_fail(SPK_ERR_ARG, "set_act_means: non-finite mean");
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  m->act_mean.assign(host, host + numel);
  HIP_TRY(hipMemcpy(m->act_mean_dev, host, (size_t)numel * 4, hipMemcpyHostToDevice));
  m->have_means = true;
  m->packed_zs = -1;   // re-round at the next commit
  return SPK_OK;
}

extern "C" int spk_model_get_act_means(spk_model* m, float* host, int64_t numel) {
  if (!m || !host) return spk_fail(SPK_ERR_ARG, "get_act_means: bad arguments");
  if (!m->have_means) return spk_fail(SPK_ERR_STATE, "no activation means: calibrate or set them first");
  if (numel != (int64_t)m->n_means) return spk_fail(SPK_ERR_ARG, "get_act_means: size mismatch");
  memcpy(host, m->act_mean.data(), (size_t)numel * 4);
  return SPK_OK;
}

// One calibration batch: the forward in the most accurate mode (every conv hi + lo, nothing fused away, one stream),
// then the per-channel mean of every generic conv's input tensor, accumulated over calls (reset != 0 starts over).
// The means describe the DATA the model will see, not the batch composition of any later call: a model's probabilities
// stay a function of (weights, means, image).  They are stored with the model (`act_means.pth`, sykepic_hip/prob.py).
extern "C" int spk_model_calibrate_act_means(spk_model* m, const void* x, int n, int h, int w, int layout, int dtype,
                                             int reset) {
  if (!m || !x || n <= 0) return spk_fail(SPK_ERR_ARG, "calibrate_act_means: bad arguments");
  if (dtype != SPK_DTYPE_F32 && dtype != SPK_DTYPE_U8) return spk_fail(SPK_ERR_ARG, "calibrate_act_means: dtype must be f32 or u8");
  if (m->infer_dt != DT_F16) return spk_fail(SPK_ERR_STATE, "calibrate_act_means needs the fp16 eval path");
  if (m->n_means == 0) return spk_fail(SPK_ERR_UNSUPPORTED, "the graph has no convolution to calibrate");
  HIP_TRY(hipSetDevice(m->device));
  std::vector<int> gen;   // generic convs and the 7x7 stem, graph order
  for (size_t i = 0; i < m->layers.size(); ++i)
    if (m->layers[i].d.kind == SPK_OP_CONV && (m->layers[i].mode == CONV_MODE_GENERIC || m->layers[i].mode == CONV_MODE_STEM))
      gen.push_back((int)i);
  if (reset || m->cal_sum.size() != m->n_means) {
    m->cal_sum.assign(m->n_means, 0.0);
    m->cal_rows.assign(gen.size(), 0.0);
  }
  // the accurate forward: remember the caller's settings
  const int keep_split = m->splitw, keep_fp8 = m->fp8;
  const bool keep_zs = m->zero_sum, keep_have = m->have_means;
  m->splitw = 1; m->zero_sum = false; m->have_means = false; m->fp8 = 0;
  int rc = spk_commit(m);
  if (rc == SPK_OK) rc = spk_plan(m, n, h, w);
  float *part = nullptr, *mean_dev = nullptr;
  std::vector<float> host(m->n_means + 8);
  if (rc == SPK_OK) {
    int cmax = 8;
    for (int li : gen) cmax = std::max(cmax, m->tdims[m->layers[li].d.src].c);
    if (hipMalloc((void**)&part, (size_t)256 * cmax * 4) != hipSuccess || hipMalloc((void**)&mean_dev, (m->n_means + 8) * 4) != hipSuccess)
      rc = spk_fail(SPK_ERR_HIP, "hipMalloc(calibration scratch) failed");
  }
  const int mb = spk_micro_batch(m, n);
  for (int i0 = 0; i0 < n && rc == SPK_OK; i0 += mb) {
    const int nb = std::min(mb, n - i0);
    const char* xi = (const char*)x + (size_t)i0 * spk_image_stride_bytes(m->in_chans, h, w, dtype);
    m->act_dt = m->infer_dt;
    m->t_fp8_scale.assign(m->n_tensors, 0.f);
    if (spk_launch_to_nhwc4(xi, layout, dtype, nb, m->in_chans, h, w, (bf16_t*)m->T(0), m->infer_dt, m->stream, SPK_INPUT_SCALE)) {
      rc = spk_fail(SPK_ERR_HIP, "input conversion launch failed");
      break;
    }
    // a forward with no fusion allowed: every tensor a conv reads must really be written (no fused stem pool / shortcut conv)
    spk_eval_begin(m, nb);
    const EvalCursor c{0, 0, nb, m->stream};
    for (size_t i = 0; i < m->layers.size() && rc == SPK_OK; ++i) rc = spk_run_layer_eval(m, m->layers[i], c, EVAL_FORWARD);
    for (size_t gi = 0; gi < gen.size() && rc == SPK_OK; ++gi) {
      const Layer& L = m->layers[gen[gi]];
      const TDim& in = m->tdims[L.d.src];
      if (L.mode == CONV_MODE_STEM) {
        // the NHWC4 input image (row pitch padded to an even width with zero pixels): pixel PAIRS as rows of 8 values, into
        // the 8 spare floats behind the vector; folded to per-channel means on the host below
        if (spk_launch_chan_mean((const bf16_t*)m->T(0), part, mean_dev + m->n_means, (size_t)nb * in.h * in.w / 2, 8,
                                 m->infer_dt, m->stream))
          rc = spk_fail(SPK_ERR_HIP, "channel-mean launch failed");
        continue;
      }
      if (in.c != L.d.cin || !in.bf16) { rc = spk_fail(SPK_ERR_UNSUPPORTED, std::string("calibration: unexpected input layout at ") + L.d.name); break; }
      if (spk_launch_chan_mean((const bf16_t*)m->T(L.d.src), part, mean_dev + L.mu_off, (size_t)nb * in.h * in.w, in.c,
                               m->infer_dt, m->stream))
        rc = spk_fail(SPK_ERR_HIP, "channel-mean launch failed");
    }
    if (rc != SPK_OK) break;
    if (hipMemcpyAsync(host.data(), mean_dev, (m->n_means + 8) * 4, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess) {
      rc = spk_fail(SPK_ERR_HIP, "reading the calibration means failed");
      break;
    }
    for (size_t gi = 0; gi < gen.size(); ++gi) {
      const Layer& L = m->layers[gen[gi]];
      const TDim& in = m->tdims[L.d.src];
      if (L.mode == CONV_MODE_STEM) {   // mean over the w real pixels of a row: the pair means carry the zero pad pixel
        const double rows = (double)nb * in.h * w, fix = (double)in.w / (double)w;
        for (int c = 0; c < L.d.cin; ++c)
          m->cal_sum[L.mu_off + c] += 0.5 * ((double)host[m->n_means + c] + (double)host[m->n_means + 4 + c]) * fix * rows /
                                      (double)SPK_INPUT_SCALE;
        m->cal_rows[gi] += rows;
        continue;
      }
      const double rows = (double)nb * in.h * in.w;
      for (int c = 0; c < L.d.cin; ++c) m->cal_sum[L.mu_off + c] += (double)host[L.mu_off + c] * rows;
      m->cal_rows[gi] += rows;
    }
  }
  (void)hipStreamSynchronize(m->stream);
  if (part) (void)hipFree(part);
  if (mean_dev) (void)hipFree(mean_dev);
  m->splitw = keep_split; m->zero_sum = keep_zs; m->have_means = keep_have; m->fp8 = keep_fp8;
  if (rc != SPK_OK) return rc;
  for (size_t gi = 0; gi < gen.size(); ++gi) {
    const Layer& L = m->layers[gen[gi]];
    for (int c = 0; c < L.d.cin; ++c) host[L.mu_off + c] = (float)(m->cal_sum[L.mu_off + c] / m->cal_rows[gi]);
  }
  return spk_model_set_act_means(m, host.data(), (int64_t)m->n_means);
}
