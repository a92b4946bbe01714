// Model handle: the parameter table (state_dict I/O), the weight EMA, and the per-handle knobs (host side, no kernel).
#include "model.h"

#include <cstring>

// ---------------------------------------------------------------------------
// state_dict I/O
// ---------------------------------------------------------------------------
extern "C" int spk_model_num_params(spk_model* m) { return m ? (int)m->params.size() : 0; }

extern "C" int spk_model_param_info(spk_model* m, int idx, char* key, int key_cap, int64_t shape[4],
                                    int* ndim, int* dtype) {
  if (!m || idx < 0 || idx >= (int)m->params.size()) return spk_fail(SPK_ERR_ARG, "param index out of range");
  const Param& p = m->params[idx];
  if (key && key_cap > 0) { strncpy(key, p.key.c_str(), key_cap - 1); key[key_cap - 1] = 0; }
  if (shape) for (int i = 0; i < 4; ++i) shape[i] = i < p.ndim ? p.shape[i] : 1;
  if (ndim) *ndim = p.ndim;
  if (dtype) *dtype = p.dtype;
  return SPK_OK;
}

static Param* find_param(spk_model* m, const char* key) {
  if (!m || !key) return nullptr;
  auto it = m->index.find(key);
  return it == m->index.end() ? nullptr : &m->params[it->second];
}

extern "C" int spk_model_load_param(spk_model* m, const char* key, const void* host, int64_t numel) {
  Param* p = find_param(m, key);
  if (!p) return spk_fail(SPK_ERR_KEY, std::string("unknown state_dict key: ") + (key ? key : "(null)"));
  if (numel != p->numel) return spk_fail(SPK_ERR_ARG, std::string("size mismatch for ") + key);
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (p->dtype == SPK_DTYPE_I64) {
    m->layers[p->layer].nbt = *(const int64_t*)host;
    return SPK_OK;
  }
  SPK_TRY(spk_load_flat(m, m->pbuf, *p, (const float*)host));
  m->dirty = true;
  spk_train_mark_dirty(m);
  return SPK_OK;
}

// a conv weight between OIHW (state_dict) and O,H,W,I (device master layout, K = tap-major)
static void conv_w_layout(const Param& p, const float* src, float* dst, bool to_device) {
  const int64_t O = p.shape[0], I = p.shape[1], H = p.shape[2], W = p.shape[3];
  for (int64_t o = 0; o < O; ++o)
    for (int64_t i = 0; i < I; ++i)
      for (int64_t h = 0; h < H; ++h)
        for (int64_t w = 0; w < W; ++w) {
          const size_t dev = (size_t)(((o * H + h) * W + w) * I + i), sd = (size_t)(((o * I + i) * H + h) * W + w);
          if (to_device) dst[dev] = src[sd];
          else dst[sd] = src[dev];
        }
}

// inverse of spk_read_flat: one tensor in state_dict layout into its slice of a flat device buffer
int spk_load_flat(spk_model* m, float* flat, const Param& p, const float* host) {
  std::vector<float> tmp;
  if (p.kind == PK_CONV_W) {
    tmp.resize((size_t)p.numel);
    conv_w_layout(p, host, tmp.data(), true);
    host = tmp.data();
  }
  HIP_TRY(hipMemcpy(flat + p.off, host, (size_t)p.numel * 4, hipMemcpyHostToDevice));
  return SPK_OK;
}

extern "C" int spk_model_read_param(spk_model* m, const char* key, void* host, int64_t numel) {
  Param* p = find_param(m, key);
  if (!p) return spk_fail(SPK_ERR_KEY, std::string("unknown state_dict key: ") + (key ? key : "(null)"));
  if (numel != p->numel) return spk_fail(SPK_ERR_ARG, std::string("size mismatch for ") + key);
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (p->dtype == SPK_DTYPE_I64) {
    *(int64_t*)host = m->layers[p->layer].nbt;
    return SPK_OK;
  }
  return spk_read_flat(m, m->pbuf, *p, (float*)host);
}

int spk_read_flat(spk_model* m, const float* flat, const Param& p, float* host) {
  if (p.kind != PK_CONV_W) {
    HIP_TRY(hipMemcpy(host, flat + p.off, (size_t)p.numel * 4, hipMemcpyDeviceToHost));
    return SPK_OK;
  }
  std::vector<float> tmp((size_t)p.numel);
  HIP_TRY(hipMemcpy(tmp.data(), flat + p.off, (size_t)p.numel * 4, hipMemcpyDeviceToHost));
  conv_w_layout(p, tmp.data(), host, false);
  return SPK_OK;
}

// ---------------------------------------------------------------------------
// exponential moving average of the weights (include/sykepic_hip.h): a second flat buffer in pbuf's layout
// ---------------------------------------------------------------------------
static bool ema_weight_ok(float w) { return w > 0.f && w < 1.f; }   // (false for NaN; nothing infinite is below 1)

// exchanges the CONTENTS of pbuf and the average on the model's stream: every packed image is rebuilt from pbuf at its
// next use; offsets into pbuf that other code holds stay valid
static int ema_exchange(spk_model* m) {
  SPK_TRY(spk_train_join(m));
  if (spk_launch_swap_f32(m->pbuf, m->ema, m->n_flat, m->stream) != 0) return spk_fail(SPK_ERR_HIP, "model_ema_swap: launch failed");
  m->ema_swapped = !m->ema_swapped;
  m->dirty = true;
  spk_train_mark_dirty(m);
  return SPK_OK;
}

extern "C" int spk_model_ema_enable(spk_model* m, int on) {
  if (!m) return spk_fail(SPK_ERR_ARG, "model_ema_enable: null model");
  if (on && m->ema_swapped)
    return spk_fail(SPK_ERR_STATE, "model_ema_enable: the moving average is swapped in (swap back before starting it again)");
  if (!on && !m->ema) return SPK_OK;
  HIP_TRY(hipSetDevice(m->device));
  if (!on) {
    if (m->ema_swapped) SPK_TRY(ema_exchange(m));   // the model keeps its own weights
    HIP_TRY(hipStreamSynchronize(m->stream));
    HIP_TRY(hipFree(m->ema));
    m->ema = nullptr;
    return SPK_OK;
  }
  SPK_TRY(spk_train_join(m));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (!m->ema) HIP_TRY(hipMalloc((void**)&m->ema, m->n_flat * sizeof(float)));
  HIP_TRY(hipMemcpy(m->ema, m->pbuf, m->n_flat * sizeof(float), hipMemcpyDeviceToDevice));
  return SPK_OK;
}

extern "C" int spk_model_ema_state(spk_model* m, int* enabled, int* swapped) {
  if (!m || !enabled || !swapped) return spk_fail(SPK_ERR_ARG, "model_ema_state: null argument");
  *enabled = m->ema != nullptr;
  *swapped = m->ema_swapped;
  return SPK_OK;
}

extern "C" int spk_model_ema_update(spk_model* m, float w) {
  if (!m) return spk_fail(SPK_ERR_ARG, "model_ema_update: null model");
  if (!ema_weight_ok(w)) return spk_fail(SPK_ERR_ARG, "model_ema_update: w must be finite and inside (0, 1)");
  if (!m->ema) return spk_fail(SPK_ERR_STATE, "model_ema_update: the moving average is not enabled");
  if (m->ema_swapped) return spk_fail(SPK_ERR_STATE, "model_ema_update: the moving average is swapped in");
  HIP_TRY(hipSetDevice(m->device));
  SPK_TRY(spk_train_join(m));
  if (spk_launch_ema_lerp(m->ema, m->pbuf, m->n_flat, w, m->stream) != 0)
    return spk_fail(SPK_ERR_HIP, "model_ema_update: launch failed");
  return SPK_OK;
}

extern "C" int spk_model_ema_swap(spk_model* m) {
  if (!m) return spk_fail(SPK_ERR_ARG, "model_ema_swap: null model");
  if (!m->ema) return spk_fail(SPK_ERR_STATE, "model_ema_swap: the moving average is not enabled");
  HIP_TRY(hipSetDevice(m->device));
  return ema_exchange(m);
}

// the float tensor `key` of the average: argument checks of spk_model_ema_read / spk_model_ema_load
static int ema_param(spk_model* m, const char* key, const void* host, int64_t numel, const char* fn, const Param** out) {
  if (!m || !key || !host) return spk_fail(SPK_ERR_ARG, std::string(fn) + ": null argument");
  if (!m->ema) return spk_fail(SPK_ERR_STATE, std::string(fn) + ": the moving average is not enabled");
  const Param* p = find_param(m, key);
  if (!p) return spk_fail(SPK_ERR_KEY, std::string(fn) + ": unknown state_dict key: " + key);
  if (p->dtype == SPK_DTYPE_I64)
    return spk_fail(SPK_ERR_ARG, std::string(fn) + ": " + key + " is an int64 counter: it is not averaged, the model's own serves");
  if (numel != p->numel) return spk_fail(SPK_ERR_ARG, std::string(fn) + ": size mismatch for " + key);
  *out = p;
  return SPK_OK;
}

extern "C" int spk_model_ema_read(spk_model* m, const char* key, float* host, int64_t numel) {
  const Param* p = nullptr;
  SPK_TRY(ema_param(m, key, host, numel, "model_ema_read", &p));
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return spk_read_flat(m, m->ema, *p, host);
}

extern "C" int spk_model_ema_load(spk_model* m, const char* key, const float* host, int64_t numel) {
  const Param* p = nullptr;
  SPK_TRY(ema_param(m, key, host, numel, "model_ema_load", &p));
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return spk_load_flat(m, m->ema, *p, host);
}

// ---- optimizer membership and the per-handle knobs ----
extern "C" int spk_model_set_requires_grad(spk_model* m, const char* key, int flag) {
  Param* p = find_param(m, key);
  if (!p) return spk_fail(SPK_ERR_KEY, std::string("unknown state_dict key: ") + (key ? key : "(null)"));
  if (!p->trainable) return spk_fail(SPK_ERR_ARG, std::string(key) + " is a buffer, not a parameter");
  p->requires_grad = flag ? 1 : 0;
  return SPK_OK;
}

extern "C" int spk_model_set_param_group(spk_model* m, const char* key, int group) {
  Param* p = find_param(m, key);
  if (!p) return spk_fail(SPK_ERR_KEY, std::string("unknown state_dict key: ") + (key ? key : "(null)"));
  if (!p->trainable || group < -1 || group > 2) return spk_fail(SPK_ERR_ARG, "bad param group");
  p->group = group;
  return SPK_OK;
}

extern "C" int spk_model_set_infer_dtype(spk_model* m, int bf16) {
  if (!m) return spk_fail(SPK_ERR_ARG, "null model");
  m->infer_dt = bf16 ? DT_BF16 : DT_F16;
  return SPK_OK;
}

extern "C" int spk_model_set_precision(spk_model* m, int split_weights, int precise_residual) {
  if (!m) return spk_fail(SPK_ERR_ARG, "null model");
  // MobileNetV3: the single fp16 product of every conv does not hold the 1e-3 probability tolerance on a trained
  // MobileNetV3-Large (5.3e-4 ... 1.05e-3 worst of 256 images, tests/test_gpu_mobilenet.py), zero-sum rounded or not
  if (split_weights == 5 && m->mobilenet)
    return spk_fail(SPK_ERR_UNSUPPORTED, "the calibrated single-pass mode does not hold the tolerance on MobileNetV3 graphs");
  // (4 = mask: spk_model_set_split_ops; 5 = calibrated single pass, needs activation means)
  m->splitw = split_weights < 0 ? 0 : (split_weights == 5 ? 5 : (split_weights > 3 ? 3 : split_weights));
  if ((precise_residual != 0) != m->precise_res) {
    m->precise_res = precise_residual != 0;
    m->cap_n = 0;  // re-plan: remainder tensors appear / disappear
  }
  return SPK_OK;
}

extern "C" int spk_model_set_split_ops(spk_model* m, const unsigned char* flags, int n_ops) {
  if (!m || !flags) return spk_fail(SPK_ERR_ARG, "null argument");
  if (n_ops != (int)m->layers.size()) return spk_fail(SPK_ERR_ARG, "one flag per graph op expected");
  m->split_mask.assign(flags, flags + n_ops);
  m->splitw = 4;
  ++m->split_epoch;
  return SPK_OK;
}

extern "C" int spk_model_set_bn(spk_model* m, float eps, float momentum) {
  if (!m || !(eps > 0.f) || !(momentum >= 0.f && momentum <= 1.f)) return spk_fail(SPK_ERR_ARG, "set_bn: bad arguments");
  m->bn_eps = eps;
  m->bn_momentum = momentum;
  m->dirty = true;   // the eval-BN fold depends on eps
  return SPK_OK;
}

extern "C" int spk_model_set_seed(spk_model* m, uint64_t seed) {
  if (!m) return spk_fail(SPK_ERR_ARG, "null model");
  m->seed = seed;
  return SPK_OK;
}
