// libsykepic_hip.so — C-ABI, model handle and layer executor (host side).
// Public contract and the reference lines each entry point replaces:
// include/sykepic_hip.h.
#include "../../include/sykepic_hip.h"
#include "spk_common.h"
#include "model.h"
#include "tune_table.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static thread_local std::string g_err;

void spk_set_error(const std::string& s) { g_err = s; }

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) {                                                             \
      spk_set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                 \
      return SPK_ERR_HIP;                                                               \
    }                                                                                   \
  } while (0)

#define SPK_TRY(expr)              \
  do {                             \
    int r_ = (expr);               \
    if (r_ != SPK_OK) return r_;   \
  } while (0)

static int fail(int code, const std::string& msg) {
  spk_set_error(msg);
  return code;
}

extern "C" const char* spk_last_error(void) { return g_err.c_str(); }
extern "C" const char* spk_version(void) { return "sykepic_hip 0.1.0 (gfx950)"; }

// ---------------------------------------------------------------------------
// construction
// ---------------------------------------------------------------------------
static int add_param(spk_model* m, const std::string& key, int kind, int layer, int dtype,
                     std::initializer_list<int64_t> shape, bool trainable) {
  Param p;
  p.key = key;
  p.kind = kind;
  p.layer = layer;
  p.dtype = dtype;
  p.ndim = (int)shape.size();
  p.numel = 1;
  int i = 0;
  for (int64_t s : shape) { p.shape[i++] = s; p.numel *= s; }
  p.trainable = trainable;
  p.requires_grad = trainable ? 1 : 0;
  p.group = trainable ? 0 : -1;
  m->index[key] = (int)m->params.size();
  m->params.push_back(p);
  return (int)m->params.size() - 1;
}

extern "C" int spk_model_create(const spk_layer_desc* layers, int n_layers, int in_chans,
                                int num_classes, int device, spk_model** out) {
  return spk_model_create_grouped(layers, nullptr, n_layers, in_chans, num_classes, device, out);
}

extern "C" int spk_model_create_grouped(const spk_layer_desc* layers, const int32_t* groups, int n_layers, int in_chans,
                                        int num_classes, int device, spk_model** out) {
  if (!layers || n_layers <= 0 || !out) return fail(SPK_ERR_ARG, "spk_model_create: bad arguments");
  for (int i = 0; groups && i < n_layers; ++i) {
    const spk_layer_desc& d = layers[i];
    if (groups[i] < 1) return fail(SPK_ERR_ARG, "spk_model_create_grouped: groups must be >= 1");
    if (groups[i] == 1) continue;
    if (d.kind != SPK_OP_CONV || d.cin != d.cout || d.res >= 0 || d.relu > SPK_ACT_RELU ||
        !spk_group_conv_ok(d.cin, groups[i], d.k, d.stride, d.pad))
      return fail(SPK_ERR_UNSUPPORTED, std::string("grouped conv ") + d.name +
                                           ": needs k 3, pad 1, stride 1 or 2, cin == cout a multiple of 16, 4 / 8 / 16 / 32 / "
                                           "64 channels per group, no shortcut, no activation but ReLU");
  }
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev)
    return fail(SPK_ERR_HIP, "spk_model_create: no such HIP device " + std::to_string(device));
  HIP_TRY(hipSetDevice(device));
  spk_model* m = new spk_model();
  m->device = device;
  m->in_chans = in_chans;
  m->num_classes = num_classes;
  if (in_chans < 1 || in_chans > 4) { delete m; return fail(SPK_ERR_UNSUPPORTED, "in_chans must be 1..4"); }

  // torch orders a residual block's modules conv1,bn1,conv2,bn2,(conv3,bn3),
  // downsample; the graph runs the downsample branch earlier.  Register the
  // parameters in state_dict order: stable sort of conv layers inside a block.
  std::vector<int> order;
  for (int i = 0; i < n_layers; ++i) order.push_back(i);
  auto block_of = [&](int i) -> std::string {
    std::string nm = layers[i].name;
    size_t p = nm.find(".downsample.");
    if (p != std::string::npos) return nm.substr(0, p);
    p = nm.rfind('.');
    return (layers[i].kind == SPK_OP_CONV && layers[i].child >= 4 && p != std::string::npos)
               ? nm.substr(0, p) : nm;
  };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    if (layers[a].kind != SPK_OP_CONV || layers[b].kind != SPK_OP_CONV) return false;
    if (block_of(a) != block_of(b)) return false;
    const bool da = strstr(layers[a].name, ".downsample.") != nullptr;
    const bool db = strstr(layers[b].name, ".downsample.") != nullptr;
    return !da && db;
  });

  m->layers.resize(n_layers);
  for (int i = 0; i < n_layers; ++i) {
    Layer& L = m->layers[i];
    L.d = layers[i];
    L.groups = groups ? groups[i] : 1;
    L.d.name[sizeof L.d.name - 1] = 0;
    L.d.bn[sizeof L.d.bn - 1] = 0;
    m->n_tensors = std::max(m->n_tensors, std::max(L.d.dst, std::max(L.d.src, L.d.res)) + 1);
    // GEMM dims of the packed weights: padded to the 64-channel granularity of the implicit-GEMM kernel; the
    // activation tensors keep their own channel count (a multiple of 8: 16-B accesses)
    L.cin_p = (L.d.cin + 63) / 64 * 64;
    L.cout_p = (L.d.cout + 63) / 64 * 64;
    if ((L.d.kind == SPK_OP_CONV || L.d.kind == SPK_OP_DWCONV || L.d.kind == SPK_OP_SE) &&
        (L.d.cout % 8 || (L.d.cin > 4 && L.d.cin % 8))) {
      delete m; return fail(SPK_ERR_UNSUPPORTED, "channel counts must be multiples of 8");
    }
    if ((L.d.kind == SPK_OP_CONV || L.d.kind == SPK_OP_DWCONV) &&
        (L.d.relu < SPK_ACT_NONE || L.d.relu > SPK_ACT_HSWISH)) {
      delete m; return fail(SPK_ERR_UNSUPPORTED, std::string("unknown activation code on ") + L.d.name);
    }
    if (L.d.relu == SPK_ACT_HSWISH) m->mobilenet = true;
    if (L.d.kind == SPK_OP_CONV) {
      const bool stem = (L.d.cin <= 4);
      const bool stem7 = stem && L.d.k == 7 && L.d.stride == 2 && L.d.pad == 3 && L.d.cout == 64;
      const bool stem3 = stem && L.d.k == 3 && L.d.stride == 2 && L.d.pad == 1;
      if (stem && !stem7 && !stem3) {
        delete m; return fail(SPK_ERR_UNSUPPORTED, "stems (Cin<=4): 7x7/2 pad 3 -> 64 or 3x3/2 pad 1");
      }
      if (stem7 && L.d.relu == SPK_ACT_HSWISH) {   // (conv_stem.hip applies ReLU or nothing)
        delete m; return fail(SPK_ERR_UNSUPPORTED, "the 7x7/2 stem: ReLU or no activation");
      }
      if (stem) L.cin_p = 4;
      L.mode = stem7 ? CONV_MODE_STEM : (stem3 ? CONV_MODE_STEM3 : CONV_MODE_GENERIC);
      L.kpad = stem7 ? 256 : L.d.k * L.d.k * L.cin_p;
      if (L.groups > 1) {   // conv_group.hip, on the fp32 master weights: no packed image, no dense or fused kernel
        L.mode = CONV_MODE_GROUP;
        L.kpad = L.d.k * L.d.k * (L.d.cin / L.groups);
      }
      if (stem3 || (!stem && L.cin_p != L.d.cin) || L.cout_p != L.d.cout || L.d.relu == SPK_ACT_SILU ||
          L.d.relu == SPK_ACT_HSWISH)
        m->effnet = true;
    } else if (L.d.kind == SPK_OP_DWCONV) {
      if ((L.d.k != 3 && L.d.k != 5) || L.d.cin != L.d.cout || L.d.pad != (L.d.k - 1) / 2) {
        delete m; return fail(SPK_ERR_UNSUPPORTED, "depthwise conv: k 3 or 5, pad (k-1)/2");
      }
      m->effnet = true;
    } else if (L.d.kind == SPK_OP_SE) {
      if (L.d.cin != L.d.cout || L.d.k < 1 || L.d.k > 1024) {
        delete m; return fail(SPK_ERR_UNSUPPORTED, "squeeze-excitation: cin == cout, 1 <= squeeze <= 1024");
      }
      // the gate pair: 0 SiLU -> Sigmoid (EfficientNet), SPK_ACT_RELU: ReLU -> Hardsigmoid (MobileNetV3)
      if (L.d.relu != SPK_ACT_NONE && L.d.relu != SPK_ACT_RELU) {
        delete m; return fail(SPK_ERR_UNSUPPORTED, "squeeze-excitation: relu 0 (SiLU / Sigmoid) or 1 (ReLU / Hardsigmoid)");
      }
      if (L.d.relu == SPK_ACT_RELU) m->mobilenet = true;
      m->effnet = true;
    }
  }
  // Layers whose rounding errors enter the residual trunk undamped: the stem,
  // every block-closing conv (it has a shortcut operand) and every conv whose
  // output some other layer adds as a shortcut (downsample branches).
  for (Layer& L : m->layers) {
    if (L.d.kind != SPK_OP_CONV) continue;
    if (L.mode == CONV_MODE_STEM || L.d.res >= 0) L.trunk_writer = true;
    for (const Layer& Q : m->layers)
      if (Q.d.kind == SPK_OP_CONV && Q.d.res == L.d.dst) L.trunk_writer = true;
  }
  // shortcut convs (ResNet downsample branches): nothing but a later layer's residual add reads their output, so
  // they are independent of the conv1 -> conv2 chain of their block and may run beside it on a second stream
  for (Layer& L : m->layers) {
    if (L.d.kind != SPK_OP_CONV) continue;
    bool as_src = false, as_res = false;
    for (const Layer& Q : m->layers) {
      as_src |= Q.d.src == L.d.dst;
      as_res |= Q.d.kind == SPK_OP_CONV && Q.d.res == L.d.dst;
    }
    L.side_branch = as_res && !as_src && L.d.dst != m->layers.back().d.dst;
  }
  // the 3x3 conv in the middle of a bottleneck: its input comes from a 1x1 conv that is not a trunk writer
  for (Layer& L : m->layers) {
    if (L.d.kind != SPK_OP_CONV || L.d.k != 3 || L.trunk_writer) continue;
    for (const Layer& Q : m->layers)
      if (Q.d.kind == SPK_OP_CONV && Q.d.dst == L.d.src && Q.d.k == 1 && !Q.trunk_writer) L.inner3x3 = true;
  }
  // the ResNet stem (7x7/2 conv + BN + ReLU) followed by the 3x3/2 pad-1 max-pool that alone reads its output: one
  // kernel in the eval path (conv_stem.hip, POOL variant)
  for (size_t i = 0; i + 1 < m->layers.size(); ++i) {
    Layer& L = m->layers[i];
    Layer& P = m->layers[i + 1];
    if (L.d.kind != SPK_OP_CONV || L.mode != CONV_MODE_STEM || L.d.relu != 1 || L.d.res >= 0) continue;
    if (P.d.kind != SPK_OP_MAXPOOL || P.d.src != L.d.dst || P.d.k != 3 || P.d.stride != 2 || P.d.pad != 1) continue;
    bool other = false;
    for (size_t j = 0; j < m->layers.size(); ++j)
      if (j != i + 1 && (m->layers[j].d.src == L.d.dst || m->layers[j].d.res == L.d.dst)) other = true;
    if (other || L.d.dst == m->layers.back().d.dst) continue;
    L.fuse_pool = (int)(i + 1);
    P.pooled_by_stem = true;
  }
  if (const char* e = getenv("SPK_FUSE_STEM_POOL")) m->fuse_stem_pool = atoi(e) != 0;
  if (const char* e = getenv("SPK_FUSE_DS")) m->fuse_ds = atoi(e) != 0;
  if (const char* e = getenv("SPK_SE_FUSE")) m->fuse_se = atoi(e) != 0;
  for (int oi : order) {
    Layer& L = m->layers[oi];
    const std::string nm = L.d.name, bn = L.d.bn;
    if (L.d.kind == SPK_OP_CONV) {
      L.p_w = add_param(m, nm + ".weight", PK_CONV_W, oi, SPK_DTYPE_F32,
                        {L.d.cout, L.d.cin / L.groups, L.d.k, L.d.k}, true);
      L.p_g = add_param(m, bn + ".weight", PK_BN_W, oi, SPK_DTYPE_F32, {L.d.cout}, true);
      L.p_b = add_param(m, bn + ".bias", PK_BN_B, oi, SPK_DTYPE_F32, {L.d.cout}, true);
      L.p_mean = add_param(m, bn + ".running_mean", PK_BN_MEAN, oi, SPK_DTYPE_F32, {L.d.cout}, false);
      L.p_var = add_param(m, bn + ".running_var", PK_BN_VAR, oi, SPK_DTYPE_F32, {L.d.cout}, false);
      L.p_nbt = add_param(m, bn + ".num_batches_tracked", PK_BN_NBT, oi, SPK_DTYPE_I64, {}, false);
    } else if (L.d.kind == SPK_OP_DWCONV) {
      L.p_w = add_param(m, nm + ".weight", PK_CONV_W, oi, SPK_DTYPE_F32, {L.d.cout, 1, L.d.k, L.d.k}, true);
      L.p_g = add_param(m, bn + ".weight", PK_BN_W, oi, SPK_DTYPE_F32, {L.d.cout}, true);
      L.p_b = add_param(m, bn + ".bias", PK_BN_B, oi, SPK_DTYPE_F32, {L.d.cout}, true);
      L.p_mean = add_param(m, bn + ".running_mean", PK_BN_MEAN, oi, SPK_DTYPE_F32, {L.d.cout}, false);
      L.p_var = add_param(m, bn + ".running_var", PK_BN_VAR, oi, SPK_DTYPE_F32, {L.d.cout}, false);
      L.p_nbt = add_param(m, bn + ".num_batches_tracked", PK_BN_NBT, oi, SPK_DTYPE_I64, {}, false);
    } else if (L.d.kind == SPK_OP_SE) {
      L.p_w = add_param(m, nm + ".fc1.weight", PK_SE_W, oi, SPK_DTYPE_F32, {L.d.k, L.d.cin, 1, 1}, true);
      L.p_b = add_param(m, nm + ".fc1.bias", PK_SE_B, oi, SPK_DTYPE_F32, {L.d.k}, true);
      L.p_w2 = add_param(m, nm + ".fc2.weight", PK_SE_W, oi, SPK_DTYPE_F32, {L.d.cout, L.d.k, 1, 1}, true);
      L.p_b2 = add_param(m, nm + ".fc2.bias", PK_SE_B, oi, SPK_DTYPE_F32, {L.d.cout}, true);
    } else if (L.d.kind == SPK_OP_LINEAR) {
      L.p_w = add_param(m, nm + ".weight", PK_FC_W, oi, SPK_DTYPE_F32, {L.d.cout, L.d.cin}, true);
      L.p_b = add_param(m, nm + ".bias", PK_FC_B, oi, SPK_DTYPE_F32, {L.d.cout}, true);
    }
  }

  // flat fp32 storage: trainable tensors first (this prefix is what the
  // gradient / optimizer-state buffers mirror), then BN running stats.
  size_t off = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (Param& p : m->params) {
      if (p.dtype != SPK_DTYPE_F32 || p.trainable != (pass == 0)) continue;
      p.off = off;
      off += (size_t)((p.numel + 63) / 64 * 64);  // 256-B aligned tensors
    }
    if (pass == 0) m->n_train = off;
  }
  m->n_flat = off;
  if (hipMalloc((void**)&m->pbuf, m->n_flat * sizeof(float)) != hipSuccess) {
    delete m; return fail(SPK_ERR_HIP, "hipMalloc(params) failed");
  }
  hipMemset(m->pbuf, 0, m->n_flat * sizeof(float));
  // BN defaults as torch: gamma 1, running_var 1
  for (Param& p : m->params) {
    if (p.kind == PK_BN_W || p.kind == PK_BN_VAR) {
      std::vector<float> ones((size_t)p.numel, 1.0f);
      hipMemcpy(m->pbuf + p.off, ones.data(), ones.size() * 4, hipMemcpyHostToDevice);
    }
  }
  // identity bottleneck blocks: conv3 (1x1, + shortcut, ReLU) <- conv2 (3x3 stride 1 pad 1, ReLU) <- conv1 (1x1, ReLU) whose
  // input IS conv3's shortcut operand, mid tensors read by nothing else, 4 cm trunk channels (conv_bneck.hip)
  for (size_t i3 = 0; i3 < m->layers.size(); ++i3) {
    Layer& L3 = m->layers[i3];
    if (L3.d.kind != SPK_OP_CONV || L3.d.k != 1 || L3.d.stride != 1 || L3.d.pad != 0 || L3.d.res < 0 || L3.d.relu != 1) continue;
    auto producer = [&](int t) {
      int idx = -1, readers = 0;
      for (size_t j = 0; j < m->layers.size(); ++j) {
        const Layer& Q = m->layers[j];
        if (Q.d.dst == t) idx = (int)j;
        readers += (Q.d.src == t) + (Q.d.kind == SPK_OP_CONV && Q.d.res == t);
      }
      return readers == 1 && t != m->layers.back().d.dst ? idx : -1;
    };
    const int i2 = producer(L3.d.src);
    if (i2 < 0) continue;
    Layer& L2 = m->layers[i2];
    if (L2.d.kind != SPK_OP_CONV || L2.d.k != 3 || L2.d.stride != 1 || L2.d.pad != 1 || L2.d.res >= 0 || L2.d.relu != 1) continue;
    const int i1 = producer(L2.d.src);
    if (i1 < 0) continue;
    Layer& L1 = m->layers[i1];
    if (L1.d.kind != SPK_OP_CONV || L1.d.k != 1 || L1.d.stride != 1 || L1.d.pad != 0 || L1.d.res >= 0 || L1.d.relu != 1) continue;
    const int cm = L1.d.cout;
    if (L1.d.src != L3.d.res || L2.d.cin != cm || L2.d.cout != cm || L3.d.cin != cm || L3.d.cout != 4 * cm || L1.d.cin != 4 * cm ||
        cm % 64 || L1.mode != CONV_MODE_GENERIC || L2.mode != CONV_MODE_GENERIC || L3.mode != CONV_MODE_GENERIC)
      continue;
    L1.bn_c2 = i2; L1.bn_c3 = (int)i3;
    L2.bn_head = L3.bn_head = i1;
  }
  if (const char* e = getenv("SPK_BNECK")) m->bneck = atoi(e);
  if (const char* e = getenv("SPK_BTAIL")) m->btail = atoi(e);
  // packed bf16 weights + folded BN scale/bias
  size_t wpack = 0, sb = 0, dwp = 0;
  for (Layer& L : m->layers) {
    if (L.d.kind == SPK_OP_DWCONV || (L.d.kind == SPK_OP_CONV && L.mode == CONV_MODE_STEM3)) {
      L.wpack_off = dwp;  // fp32, [taps (x4 input channels for the stem)][cout_p]
      dwp += (size_t)L.d.k * L.d.k * (L.d.kind == SPK_OP_CONV ? 4 : 1) * L.cout_p;
    } else if (L.d.kind == SPK_OP_SE) {
      L.wpack_off = dwp;  // fp32 fc2 weights transposed: [squeeze][cout_p]
      dwp += (size_t)L.d.k * L.cout_p;
      continue;
    } else if (L.d.kind == SPK_OP_CONV && L.mode == CONV_MODE_GROUP) {
      // (reads the fp32 master weights: scale / shift only)
    } else if (L.d.kind == SPK_OP_CONV) {
      L.wpack_off = wpack;
      wpack += (size_t)2 * L.cout_p * L.kpad;  // room for the hi + lo halves
      // (Hardswish: the implicit GEMM only - the 1x1 / 3x3 kernels of the 64-channel-multiple shapes have no Hardswish
      // epilogue; no MobileNetV3 conv has such a shape)
      L.pw_ok = L.mode == CONV_MODE_GENERIC && L.d.k == 1 && L.d.pad == 0 && L.cin_p == L.d.cin && L.cout_p == L.d.cout &&
                L.d.cin % 64 == 0 && L.d.cout % 64 == 0 && L.kpad == L.d.cin && L.d.relu != SPK_ACT_HSWISH;
      if (L.pw_ok) {
        L.wpw_off = wpack;
        wpack += (size_t)2 * L.d.cout * L.d.cin;
      }
      // (128 couts: the 3x3 conv of a bottleneck block the whole-block kernel may take (conv_bneck.hip sums in this kernel's K
      // order).  Run on its own - small batches, SPK_BNECK=0 - it must give the same bits, so it takes this kernel too and
      // never the implicit GEMM, whose tap-major sums differ in the last place: a row of probabilities does not depend on
      // the batch it was computed in.)
      L.c3_ok = L.mode == CONV_MODE_GENERIC && L.d.k == 3 && L.d.stride == 1 && L.d.pad == 1 && L.cin_p == L.d.cin &&
                L.cout_p == L.d.cout && L.d.cin % 64 == 0 &&
                (L.d.cout % 256 == 0 || (L.bn_head >= 0 && L.d.cout % 128 == 0)) && L.d.relu != SPK_ACT_HSWISH;
      // (the fragment-ordered 3x3 image also feeds the whole-bottleneck kernel: conv2 of such a block keeps one even where
      // conv_c3.hip itself has no configuration for its width)
      if (L.c3_ok || (L.bn_head >= 0 && L.d.k == 3)) {
        L.wpw_off = wpack;
        wpack += (size_t)2 * L.d.cout * 9 * L.d.cin;
      }
      // the 64 -> 64 3x3 convs (stage 1): a third image, the K = 9 * 64 GEMM panel in the 1x1 kernel's fragment order
      L.d3_ok = L.mode == CONV_MODE_GENERIC && L.d.k == 3 && L.d.stride == 1 && L.d.pad == 1 && L.cin_p == L.d.cin &&
                L.cout_p == L.d.cout && L.d.cin == 64 && L.d.cout == 64 && L.kpad == 9 * L.d.cin && L.d.relu != SPK_ACT_HSWISH;
      if (L.d3_ok) {
        L.wd3_off = wpack;
        wpack += (size_t)L.d.cout * 9 * L.d.cin;
      }
    } else {
      continue;
    }
    L.sb_off = sb;
    sb += (size_t)2 * L.cout_p;
  }
  // block-closing 1x1 conv + the 1x1 shortcut conv whose output only it adds: one K-concatenated GEMM in the eval path
  size_t wdual = 0, sdual = 0;
  for (size_t i = 0; i < m->layers.size(); ++i) {
    Layer& L = m->layers[i];
    if (L.d.kind != SPK_OP_CONV || !L.pw_ok || L.d.res < 0 || L.d.stride != 1) continue;
    for (size_t j = 0; j < m->layers.size(); ++j) {
      Layer& D = m->layers[j];
      if (D.d.kind != SPK_OP_CONV || D.d.dst != L.d.res || !D.pw_ok || !D.side_branch || D.d.relu != 0 || D.d.res >= 0 ||
          D.d.cout != L.d.cout || D.fused_into >= 0)
        continue;
      int readers = 0;
      for (const Layer& Q : m->layers) readers += (Q.d.src == D.d.dst) + (Q.d.kind == SPK_OP_CONV && Q.d.res == D.d.dst);
      if (readers != 1) continue;
      L.dual_src = (int)j;
      D.fused_into = (int)i;
      L.wdual_off = wdual;
      wdual += (size_t)2 * L.d.cout * (L.d.cin + D.d.cin);
      L.sdual_off = sdual;
      sdual += (size_t)2 * L.d.cout;
    }
  }
  // block-closing conv -> the next block's first conv (both 1x1, stride 1, 256 -> 64 / 128 channels in between)
  for (size_t i = 0; i < m->layers.size(); ++i) {
    Layer& L = m->layers[i];
    if (L.d.kind != SPK_OP_CONV || !L.pw_ok || L.d.res < 0 || L.d.stride != 1 || L.d.cout != 256) continue;
    for (size_t j = i + 1; j < m->layers.size(); ++j) {
      Layer& Q = m->layers[j];
      if (Q.d.kind != SPK_OP_CONV || !Q.pw_ok || Q.d.src != L.d.dst || Q.d.stride != 1 || Q.d.res >= 0 || Q.side_branch ||
          (Q.d.cout != 64 && Q.d.cout != 128) || Q.chained_by >= 0)
        continue;
      L.chain_next = (int)j;
      Q.chained_by = (int)i;
      break;
    }
  }
  if (const char* e = getenv("SPK_CHAIN")) m->chain = atoi(e);
  // per-channel means of every generic conv's input (zero_sum.hip): one flat vector, graph order
  for (Layer& L : m->layers) {
    if (L.d.kind != SPK_OP_CONV || (L.mode != CONV_MODE_GENERIC && L.mode != CONV_MODE_STEM)) continue;
    L.mu_off = m->n_means;   // (the 7x7 stem: the image's own channel means)
    m->n_means += (size_t)L.d.cin;
  }
  m->stale.assign(m->n_tensors, 0);
  // squeeze-excitation -> project conv pairs whose scaling the conv can apply itself (fp16 eval)
  for (size_t si = 0; si < m->layers.size(); ++si) {
    Layer& S = m->layers[si];
    if (S.d.kind != SPK_OP_SE) continue;
    int readers = 0, ci = -1;
    for (size_t j = 0; j < m->layers.size(); ++j) {
      const Layer& Q = m->layers[j];
      if (Q.d.src == S.d.dst || (Q.d.kind == SPK_OP_CONV && Q.d.res == S.d.dst)) { ++readers; ci = (int)j; }
    }
    if (readers != 1 || S.d.dst == m->layers.back().d.dst) continue;
    Layer& P = m->layers[ci];
    if (P.d.kind != SPK_OP_CONV || P.mode != CONV_MODE_GENERIC || P.d.k != 1 || P.d.stride != 1 || P.d.pad != 0 ||
        P.d.src != S.d.dst)
      continue;
    S.gate_conv = ci;
    P.gate_from = (int)si;
  }
  if (hipMalloc((void**)&m->act_mean_dev, std::max<size_t>(m->n_means, 8) * 4) != hipSuccess ||
      hipMalloc((void**)&m->wpack, std::max<size_t>(wpack, 8) * 2) != hipSuccess ||
      hipMalloc((void**)&m->dwpack, std::max<size_t>(dwp, 8) * 4) != hipSuccess ||
      hipMalloc((void**)&m->wdual, std::max<size_t>(wdual, 8) * 2) != hipSuccess ||
      hipMalloc((void**)&m->sdual, std::max<size_t>(sdual, 8) * 4) != hipSuccess ||
      hipMalloc((void**)&m->scale_bias, std::max<size_t>(sb, 8) * 4) != hipSuccess) {
    spk_model_destroy(m);
    return fail(SPK_ERR_HIP, "hipMalloc(packed weights) failed");
  }
  m->dirty = true;
  *out = m;
  return SPK_OK;
}

static void free_acts(spk_model* m) {
  if (m->arena) hipFree(m->arena);
  m->arena = nullptr;
  m->arena_bytes = 0;
  m->cap_n = m->cap_h = m->cap_w = 0;
}

extern "C" void spk_model_destroy(spk_model* m) {
  if (!m) return;
  hipSetDevice(m->device);
  hipDeviceSynchronize();
  free_acts(m);
  if (m->pbuf) hipFree(m->pbuf);
  if (m->ema) hipFree(m->ema);
  if (m->wpack) hipFree(m->wpack);
  if (m->scale_bias) hipFree(m->scale_bias);
  if (m->dwpack) hipFree(m->dwpack);
  if (m->wdual) hipFree(m->wdual);
  if (m->sdual) hipFree(m->sdual);
  if (m->act_mean_dev) hipFree(m->act_mean_dev);
  if (m->w8pack) hipFree(m->w8pack);
  if (m->fp8_shadow) hipFree(m->fp8_shadow);
  if (m->s8) hipFree(m->s8);
  if (m->loss_w) hipFree(m->loss_w);
  if (m->class_counts) hipFree(m->class_counts);
  if (m->half_stream) hipStreamDestroy(m->half_stream);
  if (m->half_fork) hipEventDestroy(m->half_fork);
  if (m->half_join) hipEventDestroy(m->half_join);
  spk_train_free(m);
  delete m;
}

extern "C" int spk_model_set_stream(spk_model* m, void* s) {
  if (!m) return fail(SPK_ERR_ARG, "null model");
  if (m->stream == (hipStream_t)s) return SPK_OK;   // (the host side sets the stream in front of every call)
  m->stream = (hipStream_t)s;
  // a training step may have left a weight gradient running on the side stream: what comes next runs on the NEW stream
  if (spk_train_join(m) != SPK_OK) return fail(SPK_ERR_HIP, "set_stream: joining the side stream failed");
  return SPK_OK;
}

// ---------------------------------------------------------------------------
// state_dict I/O
// ---------------------------------------------------------------------------
extern "C" int spk_model_num_params(spk_model* m) { return m ? (int)m->params.size() : 0; }

extern "C" int spk_model_param_info(spk_model* m, int idx, char* key, int key_cap, int64_t shape[4],
                                    int* ndim, int* dtype) {
  if (!m || idx < 0 || idx >= (int)m->params.size()) return fail(SPK_ERR_ARG, "param index out of range");
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
  if (!p) return fail(SPK_ERR_KEY, std::string("unknown state_dict key: ") + (key ? key : "(null)"));
  if (numel != p->numel) return fail(SPK_ERR_ARG, std::string("size mismatch for ") + key);
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

// inverse of spk_read_flat: one tensor in state_dict layout into its slice of a flat device buffer
int spk_load_flat(spk_model* m, float* flat, const Param& p, const float* host) {
  const float* src = host;
  std::vector<float> tmp;
  if (p.kind == PK_CONV_W) {
    // OIHW (state_dict) -> O,H,W,I (device master layout, K = tap-major)
    const int64_t O = p.shape[0], I = p.shape[1], H = p.shape[2], W = p.shape[3];
    tmp.resize((size_t)p.numel);
    for (int64_t o = 0; o < O; ++o)
      for (int64_t i = 0; i < I; ++i)
        for (int64_t h = 0; h < H; ++h)
          for (int64_t w = 0; w < W; ++w)
            tmp[(size_t)(((o * H + h) * W + w) * I + i)] = src[(size_t)(((o * I + i) * H + h) * W + w)];
    src = tmp.data();
  }
  HIP_TRY(hipMemcpy(flat + p.off, src, (size_t)p.numel * 4, hipMemcpyHostToDevice));
  return SPK_OK;
}

extern "C" int spk_model_read_param(spk_model* m, const char* key, void* host, int64_t numel) {
  Param* p = find_param(m, key);
  if (!p) return fail(SPK_ERR_KEY, std::string("unknown state_dict key: ") + (key ? key : "(null)"));
  if (numel != p->numel) return fail(SPK_ERR_ARG, std::string("size mismatch for ") + key);
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
  const int64_t O = p.shape[0], I = p.shape[1], H = p.shape[2], W = p.shape[3];
  for (int64_t o = 0; o < O; ++o)
    for (int64_t i = 0; i < I; ++i)
      for (int64_t h = 0; h < H; ++h)
        for (int64_t w = 0; w < W; ++w)
          host[(size_t)(((o * I + i) * H + h) * W + w)] = tmp[(size_t)(((o * H + h) * W + w) * I + i)];
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
  if (spk_launch_swap_f32(m->pbuf, m->ema, m->n_flat, m->stream) != 0) return fail(SPK_ERR_HIP, "model_ema_swap: launch failed");
  m->ema_swapped = !m->ema_swapped;
  m->dirty = true;
  spk_train_mark_dirty(m);
  return SPK_OK;
}

extern "C" int spk_model_ema_enable(spk_model* m, int on) {
  if (!m) return fail(SPK_ERR_ARG, "model_ema_enable: null model");
  if (on && m->ema_swapped)
    return fail(SPK_ERR_STATE, "model_ema_enable: the moving average is swapped in (swap back before starting it again)");
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
  if (!m || !enabled || !swapped) return fail(SPK_ERR_ARG, "model_ema_state: null argument");
  *enabled = m->ema != nullptr;
  *swapped = m->ema_swapped;
  return SPK_OK;
}

extern "C" int spk_model_ema_update(spk_model* m, float w) {
  if (!m) return fail(SPK_ERR_ARG, "model_ema_update: null model");
  if (!ema_weight_ok(w)) return fail(SPK_ERR_ARG, "model_ema_update: w must be finite and inside (0, 1)");
  if (!m->ema) return fail(SPK_ERR_STATE, "model_ema_update: the moving average is not enabled");
  if (m->ema_swapped) return fail(SPK_ERR_STATE, "model_ema_update: the moving average is swapped in");
  HIP_TRY(hipSetDevice(m->device));
  SPK_TRY(spk_train_join(m));
  if (spk_launch_ema_lerp(m->ema, m->pbuf, m->n_flat, w, m->stream) != 0)
    return fail(SPK_ERR_HIP, "model_ema_update: launch failed");
  return SPK_OK;
}

extern "C" int spk_model_ema_swap(spk_model* m) {
  if (!m) return fail(SPK_ERR_ARG, "model_ema_swap: null model");
  if (!m->ema) return fail(SPK_ERR_STATE, "model_ema_swap: the moving average is not enabled");
  HIP_TRY(hipSetDevice(m->device));
  return ema_exchange(m);
}

// the float tensor `key` of the average: argument checks of spk_model_ema_read / spk_model_ema_load
static int ema_param(spk_model* m, const char* key, const void* host, int64_t numel, const char* fn, const Param** out) {
  if (!m || !key || !host) return fail(SPK_ERR_ARG, std::string(fn) + ": null argument");
  if (!m->ema) return fail(SPK_ERR_STATE, std::string(fn) + ": the moving average is not enabled");
  const Param* p = find_param(m, key);
  if (!p) return fail(SPK_ERR_KEY, std::string(fn) + ": unknown state_dict key: " + key);
  if (p->dtype == SPK_DTYPE_I64)
    return fail(SPK_ERR_ARG, std::string(fn) + ": " + key + " is an int64 counter: it is not averaged, the model's own serves");
  if (numel != p->numel) return fail(SPK_ERR_ARG, std::string(fn) + ": size mismatch for " + key);
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

extern "C" int spk_model_set_requires_grad(spk_model* m, const char* key, int flag) {
  Param* p = find_param(m, key);
  if (!p) return fail(SPK_ERR_KEY, std::string("unknown state_dict key: ") + (key ? key : "(null)"));
  if (!p->trainable) return fail(SPK_ERR_ARG, std::string(key) + " is a buffer, not a parameter");
  p->requires_grad = flag ? 1 : 0;
  return SPK_OK;
}

extern "C" int spk_model_set_param_group(spk_model* m, const char* key, int group) {
  Param* p = find_param(m, key);
  if (!p) return fail(SPK_ERR_KEY, std::string("unknown state_dict key: ") + (key ? key : "(null)"));
  if (!p->trainable || group < -1 || group > 2) return fail(SPK_ERR_ARG, "bad param group");
  p->group = group;
  return SPK_OK;
}

extern "C" int spk_model_set_infer_dtype(spk_model* m, int bf16) {
  if (!m) return fail(SPK_ERR_ARG, "null model");
  m->infer_dt = bf16 ? DT_BF16 : DT_F16;
  return SPK_OK;
}

extern "C" int spk_model_set_precision(spk_model* m, int split_weights, int precise_residual) {
  if (!m) return fail(SPK_ERR_ARG, "null model");
  // MobileNetV3: the single fp16 product of every conv does not hold the 1e-3 probability tolerance on a trained
  // MobileNetV3-Large (5.3e-4 ... 1.05e-3 worst of 256 images, tests/test_gpu_mobilenet.py), zero-sum rounded or not
  if (split_weights == 5 && m->mobilenet)
    return fail(SPK_ERR_UNSUPPORTED, "the calibrated single-pass mode does not hold the tolerance on MobileNetV3 graphs");
  // (4 = mask: spk_model_set_split_ops; 5 = calibrated single pass, needs activation means)
  m->splitw = split_weights < 0 ? 0 : (split_weights == 5 ? 5 : (split_weights > 3 ? 3 : split_weights));
  if ((precise_residual != 0) != m->precise_res) {
    m->precise_res = precise_residual != 0;
    m->cap_n = 0;  // re-plan: remainder tensors appear / disappear
  }
  return SPK_OK;
}

extern "C" int spk_model_set_split_ops(spk_model* m, const unsigned char* flags, int n_ops) {
  if (!m || !flags) return fail(SPK_ERR_ARG, "null argument");
  if (n_ops != (int)m->layers.size()) return fail(SPK_ERR_ARG, "one flag per graph op expected");
  m->split_mask.assign(flags, flags + n_ops);
  m->splitw = 4;
  ++m->split_epoch;
  return SPK_OK;
}

extern "C" int spk_model_set_bn(spk_model* m, float eps, float momentum) {
  if (!m || !(eps > 0.f) || !(momentum >= 0.f && momentum <= 1.f)) return fail(SPK_ERR_ARG, "set_bn: bad arguments");
  m->bn_eps = eps;
  m->bn_momentum = momentum;
  m->dirty = true;   // the eval-BN fold depends on eps
  return SPK_OK;
}

extern "C" int spk_model_set_seed(spk_model* m, uint64_t seed) {
  if (!m) return fail(SPK_ERR_ARG, "null model");
  m->seed = seed;
  return SPK_OK;
}

// ---------------------------------------------------------------------------
// commit: fold eval-BN into per-channel scale/bias, pack bf16 weights
// ---------------------------------------------------------------------------
// does this conv run with hi/lo split weights in the eval path?
static int layer_split(const spk_model* m, const Layer& L) {
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

// is this conv's single fp16 weight image zero-sum rounded against the calibrated input means?
static bool layer_zero_sum(const spk_model* m, const Layer& L) {
  return (m->zero_sum || m->splitw == 5) && m->have_means && m->infer_dt == DT_F16 && L.d.kind == SPK_OP_CONV &&
         (L.mode == CONV_MODE_GENERIC || L.mode == CONV_MODE_STEM) && !layer_split(m, L);
}

// 3x3 RGB stem: master [cout][3][3][cin<=3] -> fp32 [9 taps][4][cout_p] (spk_pack_stem3, effnet.hip)
static int pack_stem3(spk_model* m, const Layer& L) {
  return spk_pack_stem3(m->P(L.p_w), m->dwpack + L.wpack_off, L.d.cout, L.d.cin, L.cout_p, m->stream);
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
      return fail(SPK_ERR_HIP, "pack (squeeze-excitation) launch failed");
    if (L.d.kind != SPK_OP_CONV && L.d.kind != SPK_OP_DWCONV) continue;
    float* sc = m->scale_bias + L.sb_off;
    float* bi = sc + L.cout_p;
    if (L.cout_p != L.d.cout)  // padded output channels: scale = shift = 0
      HIP_TRY(hipMemsetAsync(sc, 0, (size_t)2 * L.cout_p * 4, m->stream));
    if (spk_launch_bn_fold(m->P(L.p_g), m->P(L.p_b), m->P(L.p_mean), m->P(L.p_var), m->bn_eps, sc, bi,
                           L.d.cout, m->stream))
      return fail(SPK_ERR_HIP, "bn_fold launch failed");
    // the stems read pixel values x 255 (exact in 16 bits, spk_common.h SPK_INPUT_SCALE): their fp32 epilogue scale takes
    // the factor back
    if (L.d.kind == SPK_OP_CONV && (L.mode == CONV_MODE_STEM || L.mode == CONV_MODE_STEM3) &&
        spk_launch_scale_inplace(sc, 1.0f / SPK_INPUT_SCALE, L.d.cout, m->stream))
      return fail(SPK_ERR_HIP, "stem scale launch failed");
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
        return fail(SPK_ERR_HIP, std::string("zero-sum rounding launch failed for ") + L.d.name);
      wsrc = wround;
    }
    if (L.d.kind == SPK_OP_DWCONV)
      r = spk_launch_pack_tapmajor(m->P(L.p_w), m->dwpack + L.wpack_off, L.d.cout, L.d.k * L.d.k, L.d.cout, m->stream);
    else if (L.mode == CONV_MODE_STEM3)  // master layout [cout][kh][kw][cin]: rows = taps x 4 (cin padded to 4)
      r = pack_stem3(m, L);
    else if (L.mode == CONV_MODE_GENERIC && (L.cin_p != L.d.cin || L.cout_p != L.d.cout))
      r = spk_launch_pack_padded(wsrc, m->wpack + L.wpack_off, L.d.cout, L.d.k * L.d.k, L.d.cin, L.cout_p,
                                 L.cin_p, m->infer_dt, layer_split(m, L), m->stream);
    else
      r = spk_launch_pack_weights(wsrc, m->wpack + L.wpack_off, L.d.cout, L.d.k, L.d.k, L.d.cin,
                                  L.mode, m->infer_dt, layer_split(m, L), m->stream);
    if (r) return fail(SPK_ERR_HIP, "pack_weights launch failed");
    // 1x1 convs: second image in MFMA fragment order (conv_pw.hip).  The BatchNorm scale is NOT folded into it: a
    // small scale would push the 16-bit weights into fp16's subnormal range (measured on the calibrated-statistics
    // golden fixture: every conv split, max |dp| 5.9e-4 with the scale in the fp32 epilogue, 1.1e-3 folded)
    if (L.pw_ok && m->infer_dt == DT_F16 &&
        spk_launch_pack_pw(wsrc, nullptr, m->wpack + L.wpw_off, L.d.cout, L.d.cin, DT_F16, layer_split(m, L) ? 2 : 1,
                           m->stream))
      return fail(SPK_ERR_HIP, "pack_pw launch failed");
    if ((L.c3_ok || (L.bn_head >= 0 && L.d.k == 3)) && m->infer_dt == DT_F16 &&
        spk_launch_pack_c3(wsrc, m->wpack + L.wpw_off, L.d.cout, L.d.cin, layer_split(m, L) ? 2 : 1, m->stream))
      return fail(SPK_ERR_HIP, "pack_c3 launch failed");
    // (from the same rounded values as the implicit GEMM's image above: master layout [cout][kh][kw][cin] = [cout][K])
    if (L.d3_ok && m->infer_dt == DT_F16 && !layer_split(m, L) &&
        spk_launch_pack_pw(wsrc, nullptr, m->wpack + L.wd3_off, L.d.cout, 9 * L.d.cin, DT_F16, 1, m->stream))
      return fail(SPK_ERR_HIP, "pack_pw (3x3 panel) launch failed");
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
      if (r) { (void)hipFree(wcat); return fail(SPK_ERR_HIP, "dual-source weight packing failed"); }
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
static float fp8_scale_of(float amax) {
  // value = byte * scale; 2x headroom over the calibration batch (e4m3 keeps its 3 mantissa bits over 15 binades,
  // so headroom costs no precision); conversion saturates at +-448
  return amax > 0.f ? 2.f * amax / 448.f : 1.f;
}

// expand 1x1 conv -> depthwise conv -> squeeze-excitation -> project 1x1 conv with e4m3 tensors in between
static int assign_fp8_roles(spk_model* m, bool count_only = false) {
  const int nl = (int)m->layers.size();
  int blk = 0;
  auto consumer = [&](int t, int* idx) {
    int cnt = 0;
    for (int j = 0; j < nl; ++j)
      if (m->layers[j].d.src == t || (m->layers[j].d.kind == SPK_OP_CONV && m->layers[j].d.res == t)) { *idx = j; ++cnt; }
    return cnt;
  };
  if (!count_only)
    for (Layer& L : m->layers) L.fp8_role = 0;
  for (int i = 0; i < nl; ++i) {
    Layer& E = m->layers[i];
    if (E.d.kind != SPK_OP_CONV || E.d.k != 1 || E.d.stride != 1 || E.d.res >= 0 || E.d.cout % 16 || E.d.src == 0) continue;
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
  if (!m || n_blocks < 0 || (n_blocks > 0 && !flags)) return fail(SPK_ERR_ARG, "set_fp8_blocks: bad arguments");
  if (n_blocks > 0 && n_blocks != assign_fp8_roles(m, true))
    return fail(SPK_ERR_ARG, "set_fp8_blocks: one flag per qualifying MBConv block (spk_model_num_fp8_blocks)");
  m->fp8_blocks.assign(flags, flags + n_blocks);
  m->fp8_calibrated = false;     // roles are assigned by the next calibration
  m->fp8_packed = false;
  m->shadow_t_h[0] = m->shadow_t_h[1] = -1;
  return SPK_OK;
}

extern "C" int spk_model_set_fp8(spk_model* m, int on) {
  if (!m) return fail(SPK_ERR_ARG, "null model");
  if (on && !m->effnet) return fail(SPK_ERR_UNSUPPORTED, "the fp8 mode covers the EfficientNet MBConv blocks only");
  if (on && m->mobilenet)
    return fail(SPK_ERR_UNSUPPORTED, "the fp8 mode covers SiLU MBConv blocks only (this graph has Hardswish / Hardsigmoid)");
  m->fp8 = on ? 1 : 0;
  return SPK_OK;
}

static int fp8_amax(spk_model* m, int t, int nb, unsigned int* dev_word, float* out) {
  const TDim& d = m->tdims[t];
  HIP_TRY(hipMemsetAsync(dev_word, 0, 4, m->stream));
  if (spk_launch_absmax_f16((const bf16_t*)m->T(t), (size_t)nb * d.h * d.w * d.c / 8, dev_word, m->stream))
    return fail(SPK_ERR_HIP, "absmax launch failed");
  unsigned int bits = 0;
  HIP_TRY(hipMemcpyAsync(&bits, dev_word, 4, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  memcpy(out, &bits, 4);
  return SPK_OK;
}

extern "C" int spk_model_calibrate_fp8(spk_model* m, const void* x, int n, int h, int w, int layout, int dtype) {
  if (!m || !x || n <= 0) return fail(SPK_ERR_ARG, "calibrate_fp8: bad arguments");
  if (!m->effnet) return fail(SPK_ERR_UNSUPPORTED, "the fp8 mode covers the EfficientNet MBConv blocks only");
  if (m->infer_dt != DT_F16) return fail(SPK_ERR_STATE, "calibrate_fp8 needs the fp16 eval path");
  HIP_TRY(hipSetDevice(m->device));
  SPK_TRY(spk_plan(m, n, h, w));
  if (n > m->mb_limit) return fail(SPK_ERR_ARG, "calibration batch too large for one pass");
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
    if (L.fp8_role == 4)
      for (const Layer& S : m->layers)
        if (S.fp8_role == 3 && S.d.dst == L.d.src)
          for (const Layer& D : m->layers) if (D.fp8_role == 2 && D.d.dst == S.d.src) L.amax_in = D.amax_out;
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

static int fp8_pack(spk_model* m) {
  if (m->fp8_packed) return SPK_OK;
  for (Layer& L : m->layers) {
    if (L.fp8_role != 1 && L.fp8_role != 4) continue;
    const int kpad = (L.d.cin + 63) / 64 * 64;
    float* ws = m->s8 + L.s8_off;
    if (spk_launch_pack_fp8(m->P(L.p_w), m->w8pack + L.w8_off, ws, L.d.cout, L.d.cin, L.cout_p, kpad, 1.f, m->stream))
      return fail(SPK_ERR_HIP, "fp8 weight packing failed");
    // epilogue factor = eval-BN scale x weight scale x scale of the A bytes
    if (spk_launch_mul3(m->scale_bias + L.sb_off, ws, fp8_scale_of(L.amax_in), ws + L.cout_p, L.cout_p, m->stream))
      return fail(SPK_ERR_HIP, "fp8 scale folding failed");
  }
  m->fp8_packed = true;
  return SPK_OK;
}

// ---------------------------------------------------------------------------
// activation planning
// ---------------------------------------------------------------------------
static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int spk_plan(spk_model* m, int n, int h, int w, bool pad) {
  SPK_TRY(spk_train_join(m));   // a deferred weight gradient of the last training step still reads the input tensor
  // pad: the training layout of the EfficientNet graphs (channels of every conv output rounded up to 64, zeros in the
  // pad); the eval kernels work on the tensors' own widths.  Switching between the two only re-addresses the arena
  // (tensor dims and offsets) as long as the new layout fits the allocation - the per-epoch train -> validate -> train
  // switches of `sykepic train` used to free and re-allocate the whole arena twice per epoch.
  if (n <= m->cap_n && h == m->cap_h && w == m->cap_w && pad == m->plan_pad) return SPK_OK;
  HIP_TRY(hipStreamSynchronize(m->stream));
  const bool same_shape = n <= m->cap_n && h == m->cap_h && w == m->cap_w;
  if (same_shape) n = m->cap_n;   // keep the capacity
  m->tdims.assign(m->n_tensors, TDim());
  const int wp = (w + 1) & ~1;
  m->tdims[0] = {h, wp, 4, true};
  for (Layer& L : m->layers) {
    const TDim& in = m->tdims[L.d.src];
    TDim o;
    switch (L.d.kind) {
      case SPK_OP_CONV:
      case SPK_OP_DWCONV:
      case SPK_OP_MAXPOOL: {
        const int ih = in.h, iw = (L.d.src == 0) ? w : in.w;
        o.h = (ih + 2 * L.d.pad - L.d.k) / L.d.stride + 1;
        o.w = (iw + 2 * L.d.pad - L.d.k) / L.d.stride + 1;
        o.c = pad ? (L.d.cout + 63) / 64 * 64 : L.d.cout;
        o.c_log = L.d.cout;
        o.bf16 = true;
        if (o.h < 1 || o.w < 1) { m->cap_n = 0; return fail(SPK_ERR_ARG, "image too small for the network"); }
        if (L.d.kind != SPK_OP_MAXPOOL && L.d.src != 0 && (in.c_log > 0 ? in.c_log : in.c) != L.d.cin) {
          m->cap_n = 0;
          return fail(SPK_ERR_ARG, std::string("channel mismatch at ") + L.d.name);
        }
        break;
      }
      case SPK_OP_GAVGPOOL: o = {1, 1, in.c, false}; break;
      case SPK_OP_LINEAR: o = {1, 1, L.d.cout, false}; break;
      default: o = in; break;
    }
    m->tdims[L.d.dst] = o;
  }
  size_t total = 0;
  size_t max_img_bytes = 1;
  m->toff.assign(m->n_tensors, 0);
  for (int t = 0; t < m->n_tensors; ++t) {
    const TDim& d = m->tdims[t];
    const size_t per_img = (size_t)d.h * d.w * d.c * (d.bf16 ? 2 : 4);
    max_img_bytes = std::max(max_img_bytes, per_img);
    m->toff[t] = total;
    total += align256(per_img * n);
  }
  // rounding-remainder companions of every conv output that a later layer
  // adds as a shortcut (see ConvArgs::y_lo)
  m->toff_lo.assign(m->n_tensors, 0);
  if (m->precise_res) {
    for (const Layer& L : m->layers) {
      if (L.d.kind != SPK_OP_CONV || L.d.res < 0 || m->toff_lo[L.d.res]) continue;
      bool from_conv = false;
      for (const Layer& P : m->layers) from_conv |= (P.d.kind == SPK_OP_CONV && P.d.dst == L.d.res);
      if (!from_conv) continue;
      const TDim& d = m->tdims[L.d.res];
      m->toff_lo[L.d.res] = total;
      total += align256((size_t)d.h * d.w * d.c * 2 * n);
    }
  }
  // squeeze-excitation scratch: pool partials [n][chunks][c] of whichever depthwise kernel runs (chunks <= 64 for all
  // of them), scales [n][c], hidden units [n][squeeze]; largest layer
  size_t se_floats = 0;
  for (const Layer& L : m->layers) {
    if (L.d.kind != SPK_OP_SE) continue;
    const TDim& d = m->tdims[L.d.src];
    se_floats = std::max(se_floats, (size_t)((64 + 1) * d.c + L.d.k));
  }
  m->se_stride = se_floats;   // per image: a chunk of images [img0, img0 + nb) works in its own slice
  se_floats *= (size_t)n;
  m->se_off = total;
  total += align256(se_floats * 4);
  m->logits_off = total;
  total += align256((size_t)n * m->num_classes * 4);
  if (!(same_shape && m->arena && total <= m->arena_bytes)) {
    free_acts(m);
    HIP_TRY(hipMalloc((void**)&m->arena, total));
    m->arena_bytes = total;
  }
  m->cap_n = n;
  m->plan_pad = pad;
  m->cap_h = h;
  m->cap_w = w;
  // 32-bit buffer offsets inside the conv kernel: keep every activation of a
  // micro-batch below 2 GiB
  m->mb_limit = (int)std::max<size_t>(1, ((size_t)1 << 31) / max_img_bytes - 1);
  return SPK_OK;
}

static int micro_batch(spk_model* m, int n) {
  static int env = -1;
  if (env < 0) {
    const char* e = getenv("SPK_MICRO_BATCH");
    env = e ? atoi(e) : 0;
  }
  int mb = std::min(n, m->mb_limit);
  if (env > 0) mb = std::min(mb, env);
  return std::max(mb, 1);
}

// ---------------------------------------------------------------------------
// eval-mode forward of images [i0, i0+nb) into logits rows [i0, i0+nb)
// ---------------------------------------------------------------------------
// eval: does the stem kernel also compute the max-pool that follows it?  (not with the rounding-remainder tensors of
// the precise-residual mode, whose pool works on value + remainder)
static bool stem_pool_fused(const spk_model* m, const Layer& L) {
  return L.fuse_pool >= 0 && m->fuse_stem_pool && !m->precise_res && !m->force_unfused;
}

// eval: does the block-closing conv L absorb its shortcut conv in this forward?
static bool dual_active(const spk_model* m, const Layer& L) {
  return m->fuse_ds && L.dual_src >= 0 && L.dual_ok && m->infer_dt == DT_F16 && !m->precise_res && !m->force_unfused;
}

// eval: may the block whose first conv is L run as the whole-bottleneck kernel (single fp16 weight images, a shape the kernel
// has an instantiation for)?
static bool bneck_shape_ok(int hw_h, int hw_w, int cm) {
  return hw_h == hw_w && ((cm == 256 && hw_h == 14) || (cm == 128 && hw_h == 28));
}
static bool bneck_possible(const spk_model* m, const Layer& L) {
  if (!m->bneck || m->no_bneck_now || L.bn_c2 < 0 || m->infer_dt != DT_F16 || m->precise_res || m->force_unfused) return false;
  if (layer_split(m, L) || layer_split(m, m->layers[L.bn_c2]) || layer_split(m, m->layers[L.bn_c3])) return false;
  const TDim& in = m->tdims[L.d.src];
  return bneck_shape_ok(in.h, in.w, L.d.cout) && in.c == L.d.cin;
}

static bool chain_possible(const spk_model* m, const Layer& L);
// eval: may conv2 (L) of an identity bottleneck also compute the block's conv3 + shortcut (conv_btail_kernel: the stage whose
// trunk is too wide for the whole-block kernel)?
static bool btail_possible(const spk_model* m, const Layer& L) {
  if (!m->btail || m->no_bneck_now || L.bn_head < 0 || L.d.k != 3 || m->infer_dt != DT_F16 || m->precise_res || m->force_unfused)
    return false;
  const Layer& H = m->layers[L.bn_head];
  const Layer& L3 = m->layers[H.bn_c3];
  if (layer_split(m, L) || layer_split(m, L3) || L3.dual_src >= 0) return false;
  if (H.bneck_now_h[m->half]) return false;
  const TDim& in = m->tdims[L.d.src];
  return in.h == in.w && in.h == 56 && L.d.cout == 64 && in.c == 64;
}

// eval: may the block-closing conv L also compute the conv that reads its output (single fp16 weight images only)?
static bool chain_possible(const spk_model* m, const Layer& L) {
  if (!m->chain || m->no_chain_now || L.chain_next < 0 || m->infer_dt != DT_F16 || m->precise_res || m->force_unfused)
    return false;
  const Layer& Q = m->layers[L.chain_next];
  if (layer_split(m, L) || layer_split(m, Q)) return false;
  if (bneck_possible(m, Q)) return false;   // (that conv is the head of a block the whole-bottleneck kernel computes)
  if (L.dual_src >= 0 && !dual_active(m, L)) return false;   // (a shortcut conv that runs on its own: plain res operand)
  return true;
}

static int run_conv_eval(spk_model* m, Layer& L, int nb);

// chained kernel (1) or two kernels (0)?  Timed once per problem (both give the same bits), "chain" entries of the tuner
// table; without tuning the chained kernel, not remembered
static int chain_choice(spk_model* m, Layer& L, const PwConvArgs& q, int nb) {
  if (m->chain >= 2) return 1;
  const int key[] = {q.H, q.W, q.Cin, q.x2 ? q.Cin2 : 0, q.Coutz, q.N};
  int choice = 1;
  if (spk_tune_find(TUNE_CHAIN, key, &choice) || !spk_autotune_on()) return choice;
  SpkLaunchTimer timer;
  if (!timer.ok) return choice;
  Layer& Q = m->layers[L.chain_next];
  auto two = [&]() {
    m->no_chain_now = true;
    int r = run_conv_eval(m, L, nb);
    if (r == SPK_OK) r = run_conv_eval(m, Q, nb);
    m->no_chain_now = false;
    return r;
  };
  auto one = [&]() { return spk_pw_chain_launch(q, m->stream); };
  float t_two = 0.f, t_one = 0.f;
  const bool ok = two() == SPK_OK && one() == 0 &&   // warm-up (and the other kernels' own tuning)
                  timer.time(m->stream, 3, two, &t_two) && timer.time(m->stream, 3, one, &t_one);
  choice = ok && t_one < t_two ? 1 : 0;
  if (spk_tune_log())
    fprintf(stderr, "[spk tune chain] N%d %dx%d C%d+%d->256->%d: two kernels %.1f us, chained %.1f us\n", q.N, q.H, q.W, q.Cin,
            q.x2 ? q.Cin2 : 0, q.Coutz, t_two * 1000.f / 3.f, t_one * 1000.f / 3.f);
  spk_tune_store(TUNE_CHAIN, key, &choice, true);
  return choice;
}

// fills the chained conv's fields of q; false: shapes the kernel does not cover
static bool chain_args(spk_model* m, const Layer& L, PwConvArgs& q, int nb) {
  const Layer& Q = m->layers[L.chain_next];
  const TDim& zo = m->tdims[Q.d.dst];
  const TDim& o = m->tdims[L.d.dst];
  if (zo.h != o.h || zo.w != o.w || zo.c != Q.d.cout || Q.d.cin != L.d.cout) return false;
  q.wpz = m->wpack + Q.wpw_off;
  q.z = (bf16_t*)m->TI(Q.d.dst);
  q.scalez = m->scale_bias + Q.sb_off;
  q.shiftz = q.scalez + Q.cout_p;
  q.Coutz = Q.d.cout;
  q.reluz = Q.d.relu;
  q.z_bytes = (unsigned)((size_t)nb * zo.h * zo.w * zo.c * 2);
  return true;
}

static void bneck_args(spk_model* m, const Layer& L, BneckArgs& a, int nb) {
  const Layer& L2 = m->layers[L.bn_c2];
  const Layer& L3 = m->layers[L.bn_c3];
  const TDim& in = m->tdims[L.d.src];
  memset(&a, 0, sizeof a);
  a.x = (const bf16_t*)m->TI(L.d.src);
  a.y = (bf16_t*)m->TI(L3.d.dst);
  a.w1 = m->wpack + L.wpw_off; a.w2 = m->wpack + L2.wpw_off; a.w3 = m->wpack + L3.wpw_off;
  a.s1 = m->scale_bias + L.sb_off; a.b1 = a.s1 + L.cout_p;
  a.s2 = m->scale_bias + L2.sb_off; a.b2 = a.s2 + L2.cout_p;
  a.s3 = m->scale_bias + L3.sb_off; a.b3 = a.s3 + L3.cout_p;
  a.N = nb; a.H = in.h; a.W = in.w; a.C4 = L.d.cin; a.CM = L.d.cout;
  a.x_bytes = (unsigned)((size_t)nb * in.h * in.w * in.c * 2);
}

// whole-bottleneck kernel or three launches?  0: three launches, 1: blocks of 14 rows x 8 waves (one per CU), 2: blocks of
// 7 rows x 4 waves (two per CU).  Below a quarter of the chip 0 and 2 are timed once per problem (the same bits either
// way), "bneck" entries of the tuner table; without tuning 2, not remembered
static int bneck_choice(spk_model* m, Layer& L, const BneckArgs& a, int nb) {
  if (m->bneck >= 2) return m->bneck == 3 ? 2 : 1;
  const int big_blocks = a.N * (a.H / 14);
  // Two half batches on two streams: each half's large blocks take every other CU (140 KB of LDS: one block per CU), the two
  // launches start a few microseconds apart and their HBM-bound phases do not coincide (ResNet-50, batch 256: 3.33 ms; with
  // the small blocks, which share CUs across the halves and run in step, 3.41).
  if (m->two_streams_now && big_blocks >= 96) return 1;
  // One launch alone on the chip: the small blocks when the large ones would leave CUs idle or run every CU in step
  // (isolated, 14 x 14: 256 images 123 -> 114 us, 128 images 96 -> 67 us, 64 images 89 -> 57 us; 28 x 28: 197 -> 189, 87 -> 79,
  // 65 -> 51 us); below a quarter of the chip the three launches are timed against them.
  if (2 * big_blocks >= 64) return 2;
  const int key[] = {a.H, a.CM, a.N};
  int choice = 2;
  if (spk_tune_find(TUNE_BNECK, key, &choice) || !spk_autotune_on()) return choice;
  SpkLaunchTimer timer;
  if (!timer.ok) return choice;
  BneckArgs as = a;
  as.flags |= 4;
  auto three = [&]() {
    m->no_bneck_now = true;
    int r = run_conv_eval(m, L, nb);
    if (r == SPK_OK) r = run_conv_eval(m, m->layers[L.bn_c2], nb);
    if (r == SPK_OK) r = run_conv_eval(m, m->layers[L.bn_c3], nb);
    m->no_bneck_now = false;
    return r;
  };
  auto one = [&]() { return spk_bneck_launch(as, m->stream); };
  float t_three = 0.f, t_one = 0.f;
  const bool ok = three() == SPK_OK && one() == 0 &&   // warm-up (and the other kernels' own tuning)
                  timer.time(m->stream, 3, three, &t_three) && timer.time(m->stream, 3, one, &t_one);
  choice = ok && t_one < t_three ? 2 : 0;
  if (spk_tune_log())
    fprintf(stderr, "[spk tune bottleneck] N%d %dx%d %d->%d->%d: three kernels %.1f us, one (7-row blocks) %.1f us\n", a.N, a.H, a.W,
            a.C4, a.CM, a.C4, t_three * 1000.f / 3.f, t_one * 1000.f / 3.f);
  spk_tune_store(TUNE_BNECK, key, &choice, true);
  return choice;
}

static int run_conv_eval(spk_model* m, Layer& L, int nb) {
  const TDim& in = m->tdims[L.d.src];
  const TDim& o = m->tdims[L.d.dst];
  // conv2 / conv3 of a bottleneck whose first conv launched the whole-block kernel for this half: done
  if (L.bn_head >= 0 && !m->no_bneck_now && m->layers[L.bn_head].bneck_now_h[m->half]) {
    if (L.d.k == 3) m->stale[L.d.dst] = 3;   // y2 was not written (read_activation recomputes it); conv3's output was
    else m->stale[L.d.dst] = 0;
    return SPK_OK;
  }
  // conv3 of a bottleneck whose conv2 launch computed it too (conv_btail_kernel)
  if (L.bn_head >= 0 && L.d.k == 1 && !m->no_bneck_now && m->layers[m->layers[L.bn_head].bn_c2].btail_now_h[m->half]) {
    m->stale[L.d.dst] = 0;
    return SPK_OK;
  }
  if (L.bn_head >= 0 && L.d.k == 3 && !m->no_bneck_now) L.btail_now_h[m->half] = false;
  if (L.bn_head >= 0 && L.d.k == 3 && btail_possible(m, L)) {
    Layer& H = m->layers[L.bn_head];
    Layer& L3 = m->layers[H.bn_c3];
    BneckArgs ba;
    memset(&ba, 0, sizeof ba);
    ba.x = (const bf16_t*)m->TI(L3.d.res);
    ba.y1 = (const bf16_t*)m->TI(L.d.src);
    ba.y = (bf16_t*)m->TI(L3.d.dst);
    ba.w2 = m->wpack + L.wpw_off; ba.w3 = m->wpack + L3.wpw_off;
    ba.s2 = m->scale_bias + L.sb_off; ba.b2 = ba.s2 + L.cout_p;
    ba.s3 = m->scale_bias + L3.sb_off; ba.b3 = ba.s3 + L3.cout_p;
    ba.N = nb; ba.H = in.h; ba.W = in.w; ba.C4 = L3.d.cout; ba.CM = L.d.cout;
    ba.x_bytes = (unsigned)((size_t)nb * in.h * in.w * L3.d.cout * 2);
    bool chained = false;
    if (chain_possible(m, L3)) {   // the next block's first conv from the output tile in registers, as conv_pw.hip's chained flavour
      PwConvArgs qc;
      memset(&qc, 0, sizeof qc);
      if (chain_args(m, L3, qc, nb)) {
        ba.wz = qc.wpz; ba.z = qc.z; ba.sz = qc.scalez; ba.bz = qc.shiftz; ba.Coutz = qc.Coutz; ba.z_bytes = qc.z_bytes;
        chained = qc.reluz == 1;
        if (!chained) ba.wz = nullptr;
      }
    }
    int r = spk_btail_launch(ba, m->stream);
    if (r == -3 && chained) {      // (no instantiation with this chained width: without it)
      ba.wz = nullptr;
      chained = false;
      r = spk_btail_launch(ba, m->stream);
    }
    if (r == 0) {
      L.btail_now_h[m->half] = true;
      L3.chained_now_h[m->half] = chained;
      m->stale[L.d.dst] = 3;       // y2 was not written
      return SPK_OK;
    }
    (void)hipGetLastError();
  }
  if (L.bn_c2 >= 0 && !m->no_bneck_now) L.bneck_now_h[m->half] = false;
  if (bneck_possible(m, L) && !(L.chained_by >= 0 && m->layers[L.chained_by].chained_now_h[m->half])) {
    BneckArgs ba;
    bneck_args(m, L, ba, nb);
    if (const int form = bneck_choice(m, L, ba, nb)) {
      if (form == 2) ba.flags |= 4;
      const int r = spk_bneck_launch(ba, m->stream);
      if (r == 0) {
        L.bneck_now_h[m->half] = true;
        m->stale[L.d.dst] = 3;               // y1 was not written
        return SPK_OK;
      }
      (void)hipGetLastError();               // (no instantiation after all, or the launch was refused: three launches)
    }
  }
  if (L.chained_by >= 0 && !m->no_chain_now && m->layers[L.chained_by].chained_now_h[m->half]) return SPK_OK;   // done by that launch
  if (L.chain_next >= 0 && !m->no_chain_now) L.chained_now_h[m->half] = false;
  if (L.fused_into >= 0 && dual_active(m, m->layers[L.fused_into])) {
    m->stale[L.d.dst] = 1;   // computed inside the block-closing conv's kernel; read_activation recomputes it on demand
    return SPK_OK;
  }
  if (L.d.dst < (int)m->stale.size()) m->stale[L.d.dst] = 0;
  if (L.mode == CONV_MODE_STEM3) {
    const float* sc = m->scale_bias + L.sb_off;
    if (spk_launch_stem3x3((const bf16_t*)m->TI(L.d.src), m->dwpack + L.wpack_off, sc, sc + L.cout_p,
                           (bf16_t*)m->TI(L.d.dst), nb, in.h, in.w, in.w, o.h, o.w, L.d.cout, L.cout_p, L.d.relu,
                           m->infer_dt, m->stream))
      return fail(SPK_ERR_HIP, std::string("stem launch failed for ") + L.d.name);
    return SPK_OK;
  }
  if (L.mode == CONV_MODE_GROUP) {
    const float* sc = m->scale_bias + L.sb_off;
    if (spk_launch_group_fwd((const bf16_t*)m->TI(L.d.src), m->P(L.p_w), sc, sc + L.cout_p, (bf16_t*)m->TI(L.d.dst), nb,
                             in.h, in.w, L.d.cin, L.groups, L.d.stride, L.d.relu, m->infer_dt, m->stream))
      return fail(SPK_ERR_HIP, std::string("grouped conv launch failed for ") + L.d.name);
    return SPK_OK;
  }
  ConvArgs a;
  memset(&a, 0, sizeof a);
  a.cfg = a.dma = -1;
  a.cls_ph = a.cls_pw = -1;
  a.x = (const bf16_t*)m->TI(L.d.src);
  a.w = m->wpack + L.wpack_off;
  a.y = (bf16_t*)m->TI(L.d.dst);
  a.res = L.d.res >= 0 ? (const bf16_t*)m->TI(L.d.res) : nullptr;
  a.res_lo = L.d.res >= 0 ? (const bf16_t*)m->TLo(L.d.res) : nullptr;
  a.y_lo = (bf16_t*)m->TLo(L.d.dst);
  a.scale = m->scale_bias + L.sb_off;
  a.bias = a.scale + L.cout_p;
  a.N = nb; a.H = in.h; a.W = in.w; a.Cin = L.mode == CONV_MODE_GENERIC ? L.cin_p : in.c;
  a.Ho = o.h; a.Wo = o.w; a.Cout = L.cout_p;
  a.cin_s = in.c != a.Cin ? in.c : 0;       // EfficientNet: tensors are not padded, the GEMM is
  a.cout_s = o.c != a.Cout ? o.c : 0;
  a.kh = a.kw = L.d.k; a.stride = L.d.stride; a.pad = L.d.pad;
  a.M = nb * o.h * o.w;
  a.K = L.kpad;
  a.relu = L.d.relu;
  a.dt = m->infer_dt;
  a.splitw = layer_split(m, L);
  a.x_bytes = (unsigned)((size_t)nb * in.h * in.w * in.c * 2);
  a.w_bytes = (unsigned)((size_t)L.cout_p * L.kpad * 2 * (a.splitw ? 2 : 1));
  if (L.gate_from >= 0 && m->stale[L.d.src] == 2) {
    // the squeeze-excitation layer in front left its gates instead of the scaled tensor: read what IT read
    if (!m->gate_h[m->half]) return fail(SPK_ERR_STATE, std::string("no squeeze-excitation gates for ") + L.d.name);
    a.x = (const bf16_t*)m->TI(m->layers[L.gate_from].d.src);
    spk_set_gate(a, m->gate_h[m->half], m->gate_stride_h[m->half]);
  }
  if (stem_pool_fused(m, L)) {   // the max-pool layer that follows is computed here and skipped below
    const Layer& P = m->layers[L.fuse_pool];
    const TDim& po = m->tdims[P.d.dst];
    a.pool_y = (bf16_t*)m->TI(P.d.dst);
    a.pool_ho = po.h;
    a.pool_wo = po.w;
    m->stale_stem_t = L.d.dst;
  } else if (L.fuse_pool >= 0) {
    m->stale_stem_t = -1;
  }
  if (dual_active(m, L) && !a.y_lo) {
    Layer& D = m->layers[L.dual_src];
    const TDim& din = m->tdims[D.d.src];
    PwConvArgs q;
    memset(&q, 0, sizeof q);
    q.x = a.x; q.wp = m->wdual + L.wdual_off; q.y = a.y;
    q.scale = m->sdual + L.sdual_off; q.shift = q.scale + L.d.cout;
    q.N = nb; q.H = in.h; q.W = in.w; q.Ho = o.h; q.Wo = o.w; q.stride = 1;
    q.Cin = a.Cin; q.Cout = a.Cout; q.M = a.M; q.relu = a.relu; q.dt = DT_F16; q.nb = a.splitw ? 2 : 1;
    q.x_bytes = a.x_bytes; q.y_bytes = (unsigned)((size_t)a.M * a.Cout * 2);
    q.x2 = (const bf16_t*)m->TI(D.d.src); q.Cin2 = D.d.cin; q.H2 = din.h; q.W2 = din.w; q.stride2 = D.d.stride;
    q.x2_bytes = (unsigned)((size_t)nb * din.h * din.w * din.c * 2);
    if (chain_possible(m, L)) {
      PwConvArgs qc = q;
      if (chain_args(m, L, qc, nb) && chain_choice(m, L, qc, nb) == 1 && spk_pw_chain_launch(qc, m->stream) == 0) {
        L.chained_now_h[m->half] = true;
        return SPK_OK;
      }
      (void)hipGetLastError();
    }
    const int r = spk_conv1x1_dual_launch(q, m->stream);
    if (r == 0) return SPK_OK;
    if (r != -3) return fail(SPK_ERR_HIP, std::string("fused 1x1 conv launch failed for ") + L.d.name);
    // no configuration fits this problem: the shortcut conv on its own after all, then this layer the usual way
    m->force_unfused = true;
    const int rd = run_conv_eval(m, D, nb);
    m->force_unfused = false;
    if (rd != SPK_OK) return rd;
    L.dual_ok = false;
  }
  if (L.pw_ok && a.dt == DT_F16 && !a.res_lo && !a.y_lo && !a.cin_s && !a.cout_s && !a.pool_y) {
    PwConvArgs q;
    memset(&q, 0, sizeof q);
    q.x = a.x; q.wp = m->wpack + L.wpw_off; q.y = a.y; q.res = a.res; q.scale = a.scale; q.shift = a.bias;
    q.N = nb; q.H = in.h; q.W = in.w; q.Ho = o.h; q.Wo = o.w; q.stride = L.d.stride;
    q.Cin = a.Cin; q.Cout = a.Cout; q.M = a.M; q.relu = a.relu; q.dt = DT_F16; q.nb = a.splitw ? 2 : 1;
    q.x_bytes = a.x_bytes; q.y_bytes = (unsigned)((size_t)a.M * a.Cout * 2);
    if (chain_possible(m, L) && q.res) {
      PwConvArgs qc = q;
      if (chain_args(m, L, qc, nb) && chain_choice(m, L, qc, nb) == 1 && spk_pw_chain_launch(qc, m->stream) == 0) {
        L.chained_now_h[m->half] = true;
        return SPK_OK;
      }
      (void)hipGetLastError();
    }
    if (spk_conv1x1_launch(a, q, m->stream))
      return fail(SPK_ERR_HIP, std::string("1x1 conv launch failed for ") + L.d.name);
    return SPK_OK;
  }
  static const bool use_c3 = !getenv("SPK_C3") || atoi(getenv("SPK_C3")) != 0;
  if (use_c3 && L.c3_ok && a.dt == DT_F16 && !a.res_lo && !a.y_lo && !a.cin_s && !a.cout_s) {
    C3Args q;
    memset(&q, 0, sizeof q);
    q.x = a.x; q.wp = m->wpack + L.wpw_off; q.y = a.y; q.scale = a.scale; q.shift = a.bias;
    q.N = nb; q.H = in.h; q.W = in.w; q.Cin = a.Cin; q.Cout = a.Cout; q.M = a.M; q.relu = a.relu; q.dt = DT_F16;
    q.nb = a.splitw ? 2 : 1;
    q.x_bytes = a.x_bytes; q.y_bytes = (unsigned)((size_t)a.M * a.Cout * 2);
    q.wp_bytes = (unsigned)((size_t)a.Cout * 9 * a.Cin * 2 * q.nb);
    q.res = a.res;
    const int r = spk_conv3x3_launch(q, m->stream);
    if (r == 0) return SPK_OK;
    if (r != -3) return fail(SPK_ERR_HIP, std::string("3x3 conv launch failed for ") + L.d.name);
  }
  if (L.d3_ok && a.dt == DT_F16 && !a.splitw && !a.res_lo && !a.y_lo && !a.cin_s && !a.cout_s && !a.pool_y) {
    C3Args q;
    memset(&q, 0, sizeof q);
    q.x = a.x; q.wp = m->wpack + L.wd3_off; q.y = a.y; q.scale = a.scale; q.shift = a.bias; q.res = a.res;
    q.N = nb; q.H = in.h; q.W = in.w; q.Cin = a.Cin; q.Cout = a.Cout; q.M = a.M; q.relu = a.relu; q.dt = DT_F16; q.nb = 1;
    q.x_bytes = a.x_bytes; q.y_bytes = (unsigned)((size_t)a.M * a.Cout * 2);
    if (spk_conv3x3_d3_launch(a, q, m->stream))
      return fail(SPK_ERR_HIP, std::string("3x3 conv launch failed for ") + L.d.name);
    return SPK_OK;
  }
  if (spk_conv_launch(a, L.mode, m->stream, nullptr))
    return fail(SPK_ERR_HIP, std::string("conv launch failed for ") + L.d.name);
  return SPK_OK;
}

// Depthwise layers have two kernels (effnet.hip / pw_fp8.hip: per-thread gather; dwconv_lds.hip: input rows staged
// through LDS).  Neither wins everywhere (B4, batch 256: the LDS ring is 1.3-1.6x faster on the k5 stride-1 layers at
// 28^2 / 14^2 and up to 2x slower on the 112^2 / 56^2 layers, whose rows take several passes per iteration), so each
// distinct problem is timed once per process with both and the winner remembered (both give the same values up to
// the fp32 summation order of the pool partials).  SPK_DW_LDS=0 / 1 forces one.  (A third kernel - whole zero-padded
// image of a channel slab in LDS, LDS-DMA double-buffered, one block walking over many images - was built for the
// 14^2 / 7^2 layers and measured no faster than these two on any layer: those layers are VALU-bound, not latency-
// bound; removed.)
static int dw_forced() {
  static const int v = getenv("SPK_DW_LDS") ? atoi(getenv("SPK_DW_LDS")) : -1;
  return v;
}

// The choice stays in the process and matches its problem exactly: the two kernels sum the pool partials in different
// orders, so a choice carried to another run or another batch size would change the bits of that run.
template <class F>
static int dw_choose(int et, int nb, int h, int w, int c, int k, int s, hipStream_t st, F run, const int* chunks) {
  // candidates: 0 gather kernel, 1 LDS ring kernel; chunks[v] == 0: cannot run this problem
  if (dw_forced() >= 0) {
    const int v = dw_forced();
    if (v < 2 && chunks[v] > 0) return v;
    return 0;
  }
  const int key[] = {et, nb, h, w, c, k, s};
  int best = 0;
  if (spk_tune_find(TUNE_DW, key, &best)) return best;
  SpkLaunchTimer timer;
  if (timer.ok) {
    float t[2] = {1e30f, 1e30f};
    for (int v = 0; v < 2; ++v) {
      if (chunks[v] <= 0 || run(v) != 0) continue;   // warm-up
      if (!timer.time(st, 3, [&] { return run(v); }, &t[v])) t[v] = 1e30f;
    }
    if (t[1] < t[0]) best = 1;
    if (spk_tune_log())
      fprintf(stderr, "[spk tune] depthwise et %d N%d %dx%d C%d k%d s%d: gather %.1f us, lds ring %.1f us\n", et, nb, h, w, c, k, s,
              t[0] * 1000.f / 3.f, t[1] * 1000.f / 3.f);
  }
  spk_tune_store(TUNE_DW, key, &best, false);
  return best;
}

// fp8 mode: the four layers of an MBConv block with e4m3 tensors between them (pw_fp8.hip)
static int run_layer_fp8(spk_model* m, Layer& L, int nb) {
  const TDim& in = m->tdims[L.d.src];
  const TDim& o = m->tdims[L.d.dst];
  const float* sc = m->scale_bias + L.sb_off;
  switch (L.fp8_role) {
    case 1: {   // expand: trunk fp16 -> e4m3 in the loader; output e4m3 with the expanded tensor's scale
      const int kpad = (L.d.cin + 63) / 64 * 64;
      const float ys = fp8_scale_of(L.amax_out);
      m->t_fp8_scale[L.d.dst] = ys;
      // the trunk as e4m3 bytes when the previous block's project conv left them (same bytes as converting here)
      const bool shadow = m->shadow_t_h[m->half] == L.d.src && m->fp8_shadow;
      // (the shadow holds the images of this chunk at its own row stride)
      const void* xsrc = shadow ? (const void*)(m->fp8_shadow + (size_t)m->img0 * m->fp8_shadow_img) : m->TI(L.d.src);
      if (spk_launch_pw_fp8(xsrc, shadow ? 1 : 0, m->w8pack + L.w8_off,
                            m->TI8(L.d.dst), 1, nullptr, m->s8 + L.s8_off + L.cout_p, sc + L.cout_p, nullptr, 0, in.h * in.w,
                            nb * o.h * o.w, kpad, L.cout_p, shadow ? m->shadow_stride_h[m->half] : in.c, o.c, L.d.relu,
                            1.f / fp8_scale_of(L.amax_in), 1.f / ys, m->stream))
        return fail(SPK_ERR_HIP, std::string("fp8 expand conv launch failed for ") + L.d.name);
      return SPK_OK;
    }
    case 2: {   // depthwise on e4m3; pool partials for the squeeze-excitation gate as in the fp16 kernel
      const float ys = fp8_scale_of(L.amax_out);
      m->t_fp8_scale[L.d.dst] = ys;
      float* partial = m->SE();
      const float s_in = fp8_scale_of(L.amax_in);
      const int chunks[2] = {spk_dw_chunks(nb, o.h * ((o.w + 1) / 2), in.c),
                             spk_dwconv_lds_chunks(1, nb, in.h, in.w, in.c, o.h, o.w, L.d.k, L.d.stride)};
      auto run = [&](int v) {
        if (v)
          return spk_launch_dwconv_lds(
              1, m->TI8(L.d.src), m->dwpack + L.wpack_off, sc, sc + L.cout_p, m->TI8(L.d.dst), partial, nb, in.h, in.w, in.c,
              o.h, o.w, L.d.k, L.d.stride, L.d.relu, s_in, 1.f / ys, m->stream);
        return spk_launch_dwconv_fp8((const unsigned char*)m->TI8(L.d.src), m->dwpack + L.wpack_off, sc, sc + L.cout_p,
                                     (unsigned char*)m->TI8(L.d.dst), partial, nb, in.h, in.w, in.c, o.h, o.w, L.d.k,
                                     L.d.stride, L.d.relu, chunks[0], s_in, 1.f / ys, m->stream);
      };
      const int v = dw_choose(1, nb, in.h, in.w, in.c, L.d.k, L.d.stride, m->stream, run, chunks);
      m->dw_chunks_h[m->half] = chunks[v];
      if (run(v) != 0)
        return fail(SPK_ERR_HIP, std::string("fp8 depthwise launch failed for ") + L.d.name);
      return SPK_OK;
    }
    case 3: {   // squeeze-excitation: the gates only; the project conv multiplies them into its A operand
      float* partial = m->SE();
      const int chunks = m->dw_chunks_h[m->half];
      float* gate = partial + (size_t)nb * chunks * in.c;
      if (spk_launch_se(nullptr, nullptr, partial, chunks, gate, m->P(L.p_w), m->P(L.p_b), m->dwpack + L.wpack_off,
                        m->P(L.p_b2), nb, in.h * in.w, L.d.cin, in.c, L.d.k, DT_F16, m->stream))
        return fail(SPK_ERR_HIP, std::string("squeeze-excitation launch failed for ") + L.d.name);
      m->gate_h[m->half] = gate;
      m->gate_stride_h[m->half] = in.c;
      m->t_fp8_scale[L.d.dst] = 0.f;   // not materialised
      return SPK_OK;
    }
    default: {  // 4 project: A = the depthwise output (e4m3) x gate; fp16 trunk out (+ shortcut)
      int se_src = -1;
      for (const Layer& S : m->layers) if (S.fp8_role == 3 && S.d.dst == L.d.src) se_src = S.d.src;
      if (se_src < 0 || !m->gate_h[m->half]) return fail(SPK_ERR_STATE, "fp8 project conv without its squeeze-excitation gate");
      const TDim& e = m->tdims[se_src];
      const int kpad = (L.d.cin + 63) / 64 * 64;
      // the next block's expand conv reads this output: leave it an e4m3 copy (one buffer, re-used block after block -
      // the launches are ordered on the stream)
      unsigned char* y8 = nullptr;
      int y8_stride = 0;
      float y8_inv = 0.f;
      m->shadow_t_h[m->half] = -1;
      const char* sh_env = getenv("SPK_FP8_SHADOW");   // 0: the expand convs convert the fp16 trunk themselves (same result)
      for (const Layer& E : m->layers)
        if (E.fp8_role == 1 && E.d.src == L.d.dst && !(sh_env && atoi(sh_env) == 0)) {
          y8_stride = (o.c + 15) / 16 * 16;
          // The copy of a chunk of images [img0, img0 + nb) starts at img0 * fp8_shadow_img in EVERY block, with
          // fp8_shadow_img = the largest per-image size of any shadowed tensor of the graph (inside the chunk the rows are
          // packed at the layer's own stride).  The two half-batch chains of the two-stream forward - ordered only by the
          // fork and join events, one may run a block ahead of the other - therefore never touch each other's slices.
          // (With a per-block base, half A's project conv of block k+1 wrote over the region where half B's block-k copy
          // still waited for its expand conv whenever h * w * stride changed between the blocks.)
          size_t img_bytes = 0;
          for (const Layer& E2 : m->layers)
            if (E2.fp8_role == 1) {
              const TDim& t2 = m->tdims[E2.d.src];
              img_bytes = std::max(img_bytes, (size_t)t2.h * t2.w * ((t2.c + 15) / 16 * 16));
            }
          const size_t need = (size_t)m->cap_n * img_bytes;
          if (need > m->fp8_shadow_bytes || img_bytes != m->fp8_shadow_img) {
            HIP_TRY(hipStreamSynchronize(m->stream));
            if (m->fp8_shadow) HIP_TRY(hipFree(m->fp8_shadow));
            m->fp8_shadow = nullptr;
            m->fp8_shadow_bytes = 0;
            HIP_TRY(hipMalloc((void**)&m->fp8_shadow, need));
            m->fp8_shadow_bytes = need;
            m->fp8_shadow_img = img_bytes;
          }
          y8 = m->fp8_shadow + (size_t)m->img0 * m->fp8_shadow_img;
          y8_inv = 1.f / fp8_scale_of(E.amax_in);
          break;
        }
      if (spk_launch_pw_fp8(m->TI8(se_src), 1, m->w8pack + L.w8_off, m->TI(L.d.dst), 0,
                            L.d.res >= 0 ? (const bf16_t*)m->TI(L.d.res) : nullptr, m->s8 + L.s8_off + L.cout_p, sc + L.cout_p,
                            m->gate_h[m->half], m->gate_stride_h[m->half], e.h * e.w, nb * o.h * o.w, kpad, L.cout_p, e.c, o.c, L.d.relu,
                            1.f, 1.f, m->stream, y8, y8_stride, y8_inv))
        return fail(SPK_ERR_HIP, std::string("fp8 project conv launch failed for ") + L.d.name);
      if (y8) { m->shadow_t_h[m->half] = L.d.dst; m->shadow_stride_h[m->half] = y8_stride; }
      m->t_fp8_scale[L.d.dst] = 0.f;
      return SPK_OK;
    }
  }
}

int spk_run_layer_eval(spk_model* m, Layer& L, int nb) {
  const TDim& in = m->tdims[L.d.src];
  const TDim& o = m->tdims[L.d.dst];
  if (m->fp8 && m->fp8_calibrated && L.fp8_role) return run_layer_fp8(m, L, nb);
  switch (L.d.kind) {
    case SPK_OP_CONV: return run_conv_eval(m, L, nb);
    case SPK_OP_DWCONV: {
      const float* sc = m->scale_bias + L.sb_off;
      float* partial = m->SE();
      // the pool partial sums of the squeeze-excitation gate that follows are a by-product
      const bool f16 = m->infer_dt == DT_F16;
      const int chunks[2] = {spk_dw_chunks(nb, o.h * ((o.w + 3) / 4), in.c),
                             f16 ? spk_dwconv_lds_chunks(0, nb, in.h, in.w, in.c, o.h, o.w, L.d.k, L.d.stride) : 0};
      auto run = [&](int v) {
        if (v)
          return spk_launch_dwconv_lds(
              0, m->TI(L.d.src), m->dwpack + L.wpack_off, sc, sc + L.cout_p, m->TI(L.d.dst), partial, nb, in.h, in.w, in.c,
              o.h, o.w, L.d.k, L.d.stride, L.d.relu, 1.f, 1.f, m->stream);
        return spk_launch_dwconv((const bf16_t*)m->TI(L.d.src), m->dwpack + L.wpack_off, sc, sc + L.cout_p,
                                 (bf16_t*)m->TI(L.d.dst), partial, nb, in.h, in.w, in.c, o.h, o.w, L.d.k, L.d.stride,
                                 L.d.relu, m->infer_dt, m->stream);
      };
      const int v = dw_choose(0, nb, in.h, in.w, in.c, L.d.k, L.d.stride, m->stream, run, chunks);
      m->dw_chunks_h[m->half] = chunks[v];
      if (run(v) != 0)
        return fail(SPK_ERR_UNSUPPORTED, std::string("depthwise conv launch failed (fp16 eval only) for ") + L.d.name);
      return SPK_OK;
    }
    case SPK_OP_SE: {
      // src is the output of a depthwise conv, which left its pool partials in the scratch
      bool from_dw = false;
      for (const Layer& Q : m->layers) from_dw |= (Q.d.kind == SPK_OP_DWCONV && Q.d.dst == L.d.src);
      if (!from_dw) return fail(SPK_ERR_UNSUPPORTED, "squeeze-excitation must follow a depthwise conv");
      float* partial = m->SE();
      const int chunks = m->dw_chunks_h[m->half];   // as the depthwise launch that just ran
      float* scale = partial + (size_t)nb * chunks * in.c;
      // the gates only when the project conv behind this layer multiplies them into its operand (SPK_SE_FUSE=0: never):
      // the scaled tensor - one read and one write of the widest tensor of the block - is then not materialised
      const bool gate_only = m->fuse_se && L.gate_conv >= 0 && m->infer_dt == DT_F16 && !m->force_unfused && !m->precise_res;
      if (spk_launch_se(gate_only ? nullptr : (const bf16_t*)m->TI(L.d.src), gate_only ? nullptr : (bf16_t*)m->TI(L.d.dst),
                        partial, chunks, scale, m->P(L.p_w), m->P(L.p_b), m->dwpack + L.wpack_off, m->P(L.p_b2), nb,
                        in.h * in.w, L.d.cin, in.c, L.d.k, m->infer_dt, m->stream, L.d.relu == SPK_ACT_RELU ? 1 : 0))
        return fail(SPK_ERR_UNSUPPORTED, std::string("squeeze-excitation launch failed (fp16 eval only) for ") + L.d.name);
      m->gate_h[m->half] = gate_only ? scale : nullptr;
      m->gate_stride_h[m->half] = in.c;
      if (L.d.dst < (int)m->stale.size()) m->stale[L.d.dst] = gate_only ? 2 : 0;
      return SPK_OK;
    }
    case SPK_OP_MAXPOOL:
      if (L.pooled_by_stem && m->stale_stem_t == L.d.src) return SPK_OK;   // the stem kernel wrote this layer's output
      if (spk_launch_maxpool((const bf16_t*)m->TI(L.d.src), (bf16_t*)m->TI(L.d.dst), nb, in.h, in.w,
                             in.c, L.d.k, L.d.stride, L.d.pad, o.h, o.w, m->infer_dt, m->stream))
        return fail(SPK_ERR_HIP, "maxpool launch failed");
      return SPK_OK;
    case SPK_OP_GAVGPOOL:
      if (spk_launch_gavgpool((const bf16_t*)m->TI(L.d.src), (float*)m->TI(L.d.dst), nb, in.h * in.w,
                              in.c, m->infer_dt, m->stream))
        return fail(SPK_ERR_HIP, "avgpool launch failed");
      return SPK_OK;
    case SPK_OP_LINEAR:
      if (spk_launch_linear_fwd((const float*)m->TI(L.d.src), m->P(L.p_w), m->P(L.p_b),
                                (float*)m->TI(L.d.dst), nb, L.d.cin, L.d.cout, m->stream))
        return fail(SPK_ERR_HIP, "linear launch failed");
      return SPK_OK;
    case SPK_OP_DROPOUT:  // eval: identity
      HIP_TRY(hipMemcpyAsync(m->TI(L.d.dst), m->TI(L.d.src), (size_t)nb * in.c * 4,
                             hipMemcpyDeviceToDevice, m->stream));
      return SPK_OK;
  }
  return fail(SPK_ERR_UNSUPPORTED, "unknown layer kind");
}

// All layers of one eval forward, in graph order on the handle's stream.  (Two round-2 experiments lived here behind
// environment switches and are gone since round 4, both measured slower on ResNet-50 at batch 256 - DESIGN.md section 5:
// the shortcut convs of a block forked onto a side stream, 5.40 vs 5.30 ms; the leading layers run in 32-64 image chunks so
// that their tensors stay in the 256 MiB Infinity Cache, 5.57-5.62 vs 5.51 ms.)
static int run_layers_eval(spk_model* m, int nb) {
  m->last_eval_nb = nb;
  m->shadow_t_h[0] = m->shadow_t_h[1] = -1;
  for (size_t i = 0; i < m->layers.size(); ++i) SPK_TRY(spk_run_layer_eval(m, m->layers[i], nb));
  return SPK_OK;
}

static size_t image_stride_bytes(int c, int h, int w, int dtype) {
  return (size_t)c * h * w * (dtype == SPK_DTYPE_U8 ? 1 : 4);
}

int spk_forward_eval_logits(spk_model* m, const void* x, int n, int h, int w, int layout, int dtype,
                            float* logits_dev) {
  if (!m || !x || n <= 0) return fail(SPK_ERR_ARG, "forward: bad arguments");
  if (dtype != SPK_DTYPE_F32 && dtype != SPK_DTYPE_U8) return fail(SPK_ERR_ARG, "forward: dtype must be f32 or u8");
  HIP_TRY(hipSetDevice(m->device));
  if (m->splitw == 5 && !m->have_means)
    return fail(SPK_ERR_STATE, "the calibrated single-pass mode needs activation means first: spk_model_calibrate_act_means "
                               "on representative images, or spk_model_set_act_means with stored ones");
  SPK_TRY(spk_commit(m));
  SPK_TRY(spk_plan(m, n, h, w));
  if (m->fp8 && !m->fp8_calibrated)
    return fail(SPK_ERR_STATE, "fp8 mode needs activation ranges first: call spk_model_calibrate_fp8 on a representative batch");
  if (m->fp8) SPK_TRY(fp8_pack(m));
  m->t_fp8_scale.assign(m->n_tensors, 0.f);
  const int mb = micro_batch(m, n);
  const int last = m->layers.back().d.dst;
  m->act_dt = m->infer_dt;
  // Two halves of the batch on two streams (ResNets, one micro-batch, n >= 64): the layers of a forward are a chain,
  // but the two halves are independent, so an HBM-bound layer of one half runs beside an MFMA-bound layer of the other
  // and the tail of every kernel is covered by the other stream's work.  Both halves live in the SAME activation
  // tensors (images [0, n/2) and [n/2, n): spk_model::img0), launches are interleaved layer by layer, the caller's stream
  // forks before the first layer and joins after the last.  Per-image results do not depend on the split.  Measured
  // (ResNet-50, batch 256): 4.52 -> 4.29 ms.  SPK_EVAL_STREAMS=1 keeps one stream.
  static const int n_streams = getenv("SPK_EVAL_STREAMS") ? atoi(getenv("SPK_EVAL_STREAMS")) : 2;
  if (n_streams >= 2 && !m->precise_res && n >= 64 && n <= mb) {
    {
      if (!m->half_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&m->half_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&m->half_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&m->half_join, hipEventDisableTiming));
      }
      const hipStream_t main_s = m->stream;
      // the first forward of a shape runs both halves on the caller's stream: the per-problem kernel tuners time their
      // candidates inside the launches and must not be disturbed by the other half's kernels
      const long long key = ((long long)n << 40) | ((long long)h << 20) | (long long)w;
      const bool warm = std::find(m->half_warm.begin(), m->half_warm.end(), key) != m->half_warm.end();
      if (!warm) m->half_warm.push_back(key);
      const hipStream_t str[2] = {main_s, warm ? m->half_stream : main_s};
      m->two_streams_now = warm;
      const int cnt[2] = {n / 2, n - n / 2}, off[2] = {0, n / 2};
      HIP_TRY(hipEventRecord(m->half_fork, main_s));
      HIP_TRY(hipStreamWaitEvent(m->half_stream, m->half_fork, 0));
      m->last_eval_nb = n;
      m->shadow_t_h[0] = m->shadow_t_h[1] = -1;
      int rc = SPK_OK;
      for (int hf = 0; hf < 2 && rc == SPK_OK; ++hf) {
        m->img0 = off[hf];
        m->stream = str[hf];
        const char* xi = (const char*)x + (size_t)off[hf] * image_stride_bytes(m->in_chans, h, w, dtype);
        if (spk_launch_to_nhwc4(xi, layout, dtype, cnt[hf], m->in_chans, h, w, (bf16_t*)m->TI(0), m->infer_dt, m->stream, SPK_INPUT_SCALE))
          rc = fail(SPK_ERR_HIP, "input conversion launch failed");
      }
      for (size_t i = 0; i < m->layers.size() && rc == SPK_OK; ++i)
        for (int hf = 0; hf < 2 && rc == SPK_OK; ++hf) {
          m->img0 = off[hf];
          m->stream = str[hf];
          m->half = hf;   // what a layer leaves for the next one of ITS chain (pool-partial rows, gates, e4m3 shadow)
          rc = spk_run_layer_eval(m, m->layers[i], cnt[hf]);
        }
      m->half = 0;
      for (int hf = 0; hf < 2 && rc == SPK_OK; ++hf) {
        m->img0 = off[hf];
        m->stream = str[hf];
        if (hipMemcpyAsync(logits_dev + (size_t)off[hf] * m->num_classes, m->TI(last), (size_t)cnt[hf] * m->num_classes * 4,
                           hipMemcpyDeviceToDevice, m->stream) != hipSuccess)
          rc = fail(SPK_ERR_HIP, "logits copy failed");
      }
      m->img0 = 0;
      m->stream = main_s;
      m->two_streams_now = false;
      // (join even after an error: nothing may be left running on the second stream behind the caller's back)
      (void)hipEventRecord(m->half_join, m->half_stream);
      (void)hipStreamWaitEvent(main_s, m->half_join, 0);
      return rc;
    }
  }
  for (int i0 = 0; i0 < n; i0 += mb) {
    const int nb = std::min(mb, n - i0);
    const char* xi = (const char*)x + (size_t)i0 * image_stride_bytes(m->in_chans, h, w, dtype);
    if (spk_launch_to_nhwc4(xi, layout, dtype, nb, m->in_chans, h, w, (bf16_t*)m->T(0), m->infer_dt, m->stream, SPK_INPUT_SCALE))
      return fail(SPK_ERR_HIP, "input conversion launch failed");
    SPK_TRY(run_layers_eval(m, nb));
    HIP_TRY(hipMemcpyAsync(logits_dev + (size_t)i0 * m->num_classes, m->T(last),
                           (size_t)nb * m->num_classes * 4, hipMemcpyDeviceToDevice, m->stream));
  }
  return SPK_OK;
}

// ---------------------------------------------------------------------------
// activation means for zero-sum weight rounding (zero_sum.hip)
// ---------------------------------------------------------------------------
extern "C" int64_t spk_model_act_means_size(spk_model* m) { return m ? (int64_t)m->n_means : 0; }

extern "C" int spk_model_set_zero_sum(spk_model* m, int on) {
  if (!m) return fail(SPK_ERR_ARG, "null model");
  m->zero_sum = on != 0;
  return SPK_OK;
}

extern "C" int spk_model_set_act_means(spk_model* m, const float* host, int64_t numel) {
  if (!m) return fail(SPK_ERR_ARG, "null model");
  if (!host || numel == 0) {   // forget them
    m->have_means = false;
    m->act_mean.clear();
    m->packed_zs = -1;
    return SPK_OK;
  }
  if (numel != (int64_t)m->n_means) return fail(SPK_ERR_ARG, "set_act_means: one value per input channel of every conv expected");
  for (int64_t i = 0; i < numel; ++i)
    if (!std::isfinite(host[i])) return fail(SPK_ERR_ARG, "set_act_means: non-finite mean");
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  m->act_mean.assign(host, host + numel);
  HIP_TRY(hipMemcpy(m->act_mean_dev, host, (size_t)numel * 4, hipMemcpyHostToDevice));
  m->have_means = true;
  m->packed_zs = -1;   // re-round at the next commit
  return SPK_OK;
}

extern "C" int spk_model_get_act_means(spk_model* m, float* host, int64_t numel) {
  if (!m || !host) return fail(SPK_ERR_ARG, "get_act_means: bad arguments");
  if (!m->have_means) return fail(SPK_ERR_STATE, "no activation means: calibrate or set them first");
  if (numel != (int64_t)m->n_means) return fail(SPK_ERR_ARG, "get_act_means: size mismatch");
  memcpy(host, m->act_mean.data(), (size_t)numel * 4);
  return SPK_OK;
}

// One calibration batch: the forward in the most accurate mode (every conv hi + lo, nothing fused away, one stream),
// then the per-channel mean of every generic conv's input tensor, accumulated over calls (reset != 0 starts over).
// The means describe the DATA the model will see, not the batch composition of any later call: a model's probabilities
// stay a function of (weights, means, image).  They are stored with the model (`act_means.pth`, sykepic_hip/prob.py).
extern "C" int spk_model_calibrate_act_means(spk_model* m, const void* x, int n, int h, int w, int layout, int dtype,
                                             int reset) {
  if (!m || !x || n <= 0) return fail(SPK_ERR_ARG, "calibrate_act_means: bad arguments");
  if (dtype != SPK_DTYPE_F32 && dtype != SPK_DTYPE_U8) return fail(SPK_ERR_ARG, "calibrate_act_means: dtype must be f32 or u8");
  if (m->infer_dt != DT_F16) return fail(SPK_ERR_STATE, "calibrate_act_means needs the fp16 eval path");
  if (m->n_means == 0) return fail(SPK_ERR_UNSUPPORTED, "the graph has no convolution to calibrate");
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
      rc = fail(SPK_ERR_HIP, "hipMalloc(calibration scratch) failed");
  }
  const int mb = micro_batch(m, n);
  m->force_unfused = true;   // every tensor a conv reads must really be written (no fused stem pool / shortcut conv)
  for (int i0 = 0; i0 < n && rc == SPK_OK; i0 += mb) {
    const int nb = std::min(mb, n - i0);
    const char* xi = (const char*)x + (size_t)i0 * image_stride_bytes(m->in_chans, h, w, dtype);
    m->act_dt = m->infer_dt;
    m->t_fp8_scale.assign(m->n_tensors, 0.f);
    if (spk_launch_to_nhwc4(xi, layout, dtype, nb, m->in_chans, h, w, (bf16_t*)m->T(0), m->infer_dt, m->stream, SPK_INPUT_SCALE)) {
      rc = fail(SPK_ERR_HIP, "input conversion launch failed");
      break;
    }
    m->last_eval_nb = nb;
    for (size_t i = 0; i < m->layers.size() && rc == SPK_OK; ++i) rc = spk_run_layer_eval(m, m->layers[i], nb);
    for (size_t gi = 0; gi < gen.size() && rc == SPK_OK; ++gi) {
      const Layer& L = m->layers[gen[gi]];
      const TDim& in = m->tdims[L.d.src];
      if (L.mode == CONV_MODE_STEM) {
        // the NHWC4 input image (row pitch padded to an even width with zero pixels): pixel PAIRS as rows of 8 values, into
        // the 8 spare floats behind the vector; folded to per-channel means on the host below
        if (spk_launch_chan_mean((const bf16_t*)m->T(0), part, mean_dev + m->n_means, (size_t)nb * in.h * in.w / 2, 8,
                                 m->infer_dt, m->stream))
          rc = fail(SPK_ERR_HIP, "channel-mean launch failed");
        continue;
      }
      if (in.c != L.d.cin || !in.bf16) { rc = fail(SPK_ERR_UNSUPPORTED, std::string("calibration: unexpected input layout at ") + L.d.name); break; }
      if (spk_launch_chan_mean((const bf16_t*)m->T(L.d.src), part, mean_dev + L.mu_off, (size_t)nb * in.h * in.w, in.c,
                               m->infer_dt, m->stream))
        rc = fail(SPK_ERR_HIP, "channel-mean launch failed");
    }
    if (rc != SPK_OK) break;
    if (hipMemcpyAsync(host.data(), mean_dev, (m->n_means + 8) * 4, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess) {
      rc = fail(SPK_ERR_HIP, "reading the calibration means failed");
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
  m->force_unfused = false;
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

extern "C" int spk_forward_infer(spk_model* m, const void* x, int n, int h, int w, int layout,
                                 int dtype, float softmax_base, float* out_dev) {
  if (!out_dev) return fail(SPK_ERR_ARG, "forward: null output");
  if (softmax_base <= 0.f) return spk_forward_eval_logits(m, x, n, h, w, layout, dtype, out_dev);
  if (!m) return fail(SPK_ERR_ARG, "null model");
  HIP_TRY(hipSetDevice(m->device));
  SPK_TRY(spk_plan(m, n, h, w));
  float* logits = (float*)((char*)m->arena + m->logits_off);
  SPK_TRY(spk_forward_eval_logits(m, x, n, h, w, layout, dtype, logits));
  // softmax(z * ln(base)) == base^z / sum base^z   (probability.py:191-194)
  if (spk_launch_softmax(logits, out_dev, n, m->num_classes, logf(softmax_base), m->stream))
    return fail(SPK_ERR_HIP, "softmax launch failed");
  return SPK_OK;
}

extern "C" int spk_eval_step(spk_model* m, const void* x, int n, int h, int w, int layout, int dtype,
                             const int64_t* y, float* stats, float* logits_out) {
  if (!m || !y || !stats) return fail(SPK_ERR_ARG, "eval_step: bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  SPK_TRY(spk_plan(m, n, h, w));
  float* logits = logits_out ? logits_out : (float*)((char*)m->arena + m->logits_off);
  SPK_TRY(spk_forward_eval_logits(m, x, n, h, w, layout, dtype, logits));
  // CrossEntropyLoss is a batch mean; the caller accumulates loss*n (train.py:269)
  // validation uses the loss the training step uses, as the reference's single loss_fn (spk_model_set_loss)
  if (m->loss_ex() ? spk_launch_ce_ex(logits, y, n, m->num_classes, m->loss_w, m->loss_eps, stats, m->class_counts, nullptr,
                                      m->stream)
                   : spk_launch_ce(logits, y, n, m->num_classes, stats, nullptr, m->stream))
    return fail(SPK_ERR_HIP, "cross-entropy launch failed");
  return SPK_OK;
}

extern "C" int spk_model_read_activation(spk_model* m, int t, int n, float* host, int64_t numel) {
  if (!m || !host || t <= 0 || t >= m->n_tensors || !m->arena || n > m->cap_n)
    return fail(SPK_ERR_ARG, "read_activation: bad arguments or no forward has run");
  const TDim& d = m->tdims[t];
  const int cl = d.c_log > 0 ? d.c_log : d.c;  // the caller sees the logical channels only
  const size_t cnt = (size_t)n * d.h * d.w * d.c;
  if ((int64_t)((size_t)n * d.h * d.w * cl) != numel) return fail(SPK_ERR_ARG, "read_activation: size mismatch");
  HIP_TRY(hipSetDevice(m->device));
  if (t < (int)m->stale.size() && m->stale[t] == 1 && m->last_eval_nb > 0) {
    // a shortcut conv that the last forward computed inside its block-closing conv: run it alone (its input is still there)
    for (Layer& L : m->layers)
      if (L.d.kind == SPK_OP_CONV && L.d.dst == t) {
        m->force_unfused = true;
        const int r = run_conv_eval(m, L, m->last_eval_nb);
        m->force_unfused = false;
        if (r != SPK_OK) return r;
      }
  }
  if (t < (int)m->stale.size() && m->stale[t] == 2 && m->last_eval_nb > 0) {
    // a squeeze-excitation output the last forward applied inside the project conv: the depthwise conv in front (for its
    // pool partial sums) and the layer itself once more, this time writing the scaled tensor
    for (Layer& S : m->layers)
      if (S.d.kind == SPK_OP_SE && S.d.dst == t)
        for (Layer& D : m->layers)
          if (D.d.kind == SPK_OP_DWCONV && D.d.dst == S.d.src) {
            m->force_unfused = true;
            int r = spk_run_layer_eval(m, D, m->last_eval_nb);
            if (r == SPK_OK) r = spk_run_layer_eval(m, S, m->last_eval_nb);
            m->force_unfused = false;
            if (r != SPK_OK) return r;
          }
  }
  if (t < (int)m->stale.size() && m->stale[t] == 3 && m->last_eval_nb > 0) {
    // a mid tensor of a bottleneck block the last forward ran as one kernel: conv1 (and conv2) on their own - the block's
    // input is still there
    for (Layer& L : m->layers)
      if (L.d.kind == SPK_OP_CONV && L.d.dst == t) {
        m->force_unfused = true;
        int r = SPK_OK;
        if (L.bn_head >= 0) r = run_conv_eval(m, m->layers[L.bn_head], m->last_eval_nb);
        if (r == SPK_OK) r = run_conv_eval(m, L, m->last_eval_nb);
        m->force_unfused = false;
        if (r != SPK_OK) return r;
      }
  }
  if (t == m->stale_stem_t && m->last_eval_nb > 0) {
    // the last forward computed stem + max-pool in one kernel and never wrote this tensor: run the stem layer alone
    // (its input is still in the arena)
    for (Layer& L : m->layers)
      if (L.d.kind == SPK_OP_CONV && L.d.dst == t) {
        m->force_unfused = true;
        const int r = run_conv_eval(m, L, m->last_eval_nb);
        m->force_unfused = false;
        if (r != SPK_OK) return r;
      }
  }
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (!d.bf16) {
    HIP_TRY(hipMemcpy(host, m->T(t), cnt * 4, hipMemcpyDeviceToHost));
    return SPK_OK;
  }
  if (t < (int)m->t_fp8_scale.size() && m->t_fp8_scale[t] > 0.f) {   // e4m3 bytes: value = byte * scale
    std::vector<unsigned char> b8(cnt);
    HIP_TRY(hipMemcpy(b8.data(), m->T(t), cnt, hipMemcpyDeviceToHost));
    const float sc8 = m->t_fp8_scale[t];
    for (int i = 0; i < n; ++i)
      for (int y = 0; y < d.h; ++y)
        for (int x = 0; x < d.w; ++x)
          for (int c = 0; c < cl; ++c) {
            const unsigned b = b8[(((size_t)i * d.h + y) * d.w + x) * d.c + c];
            const int e = (b >> 3) & 15, mant = b & 7;
            float f = e ? std::ldexp(1.f + mant / 8.f, e - 7) : std::ldexp(mant / 8.f, -6);
            if (e == 15 && mant == 7) f = NAN;
            host[(((size_t)i * cl + c) * d.h + y) * d.w + x] = (b & 0x80 ? -f : f) * sc8;
          }
    return SPK_OK;
  }
  std::vector<bf16_t> tmp(cnt);
  HIP_TRY(hipMemcpy(tmp.data(), m->T(t), cnt * 2, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i)
    for (int y = 0; y < d.h; ++y)
      for (int x = 0; x < d.w; ++x)
        for (int c = 0; c < cl; ++c) {
          const bf16_t raw = tmp[(((size_t)i * d.h + y) * d.w + x) * d.c + c];
          float f;
          if (m->act_dt == DT_F16) {
            _Float16 hv;
            memcpy(&hv, &raw, 2);
            f = (float)hv;
          } else {
            const unsigned u = (unsigned)raw << 16;
            memcpy(&f, &u, 4);
          }
          host[(((size_t)i * cl + c) * d.h + y) * d.w + x] = f;
        }
  return SPK_OK;
}

// ---------------------------------------------------------------------------
// per-layer timing (bench.py roofline line)
// ---------------------------------------------------------------------------
extern "C" int spk_model_profile_infer(spk_model* m, const void* x, int n, int h, int w, int layout,
                                       int dtype, int iters, spk_layer_time* out, int cap) {
  if (!m || !x || !out || cap <= 0 || iters <= 0) return fail(SPK_ERR_ARG, "profile: bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  SPK_TRY(spk_commit(m));
  SPK_TRY(spk_plan(m, n, h, w));
  const int nb = std::min(n, micro_batch(m, n));
  const int nl = (int)m->layers.size();
  std::vector<hipEvent_t> ev(nl + 2);
  for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
  std::vector<double> ms(nl + 1, 0.0);
  for (int it = 0; it < iters + 1; ++it) {  // first pass is a warm-up
    HIP_TRY(hipEventRecord(ev[0], m->stream));
    if (spk_launch_to_nhwc4(x, layout, dtype, nb, m->in_chans, h, w, (bf16_t*)m->T(0), m->infer_dt, m->stream, SPK_INPUT_SCALE))
      return fail(SPK_ERR_HIP, "input conversion launch failed");
    HIP_TRY(hipEventRecord(ev[1], m->stream));
    for (int i = 0; i < nl; ++i) {
      SPK_TRY(spk_run_layer_eval(m, m->layers[i], nb));
      HIP_TRY(hipEventRecord(ev[i + 2], m->stream));
    }
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (it == 0) continue;
    for (int i = 0; i <= nl; ++i) {
      float t = 0.f;
      HIP_TRY(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
      ms[i] += t;
    }
  }
  for (auto& e : ev) hipEventDestroy(e);
  int cnt = 0;
  auto put = [&](const char* name, double t, double fl, double by) {
    if (cnt >= cap) return;
    memset(&out[cnt], 0, sizeof out[cnt]);
    strncpy(out[cnt].name, name, sizeof out[cnt].name - 1);
    out[cnt].ms = (float)(t / iters);
    out[cnt].flops = fl;
    out[cnt].bytes = by;
    ++cnt;
  };
  put("input.to_nhwc4", ms[0], 0.0,
      (double)nb * h * w * (m->in_chans * (dtype == SPK_DTYPE_U8 ? 1 : 4) + 8));
  for (int i = 0; i < nl; ++i) {
    const Layer& L = m->layers[i];
    const TDim& in = m->tdims[L.d.src];
    const TDim& o = m->tdims[L.d.dst];
    double fl = 0, by = 0;
    const double in_b = (double)nb * in.h * in.w * in.c * (in.bf16 ? 2 : 4);
    const double out_b = (double)nb * o.h * o.w * o.c * (o.bf16 ? 2 : 4);
    char nm[96];
    if (L.d.kind == SPK_OP_CONV) {
      const int cin = L.d.cin;
      fl = 2.0 * nb * o.h * o.w * (double)L.d.cout * cin * L.d.k * L.d.k / L.groups;
      const double real_in = L.mode == CONV_MODE_STEM ? (double)nb * in.h * in.w * 8 : in_b;
      by = real_in + out_b + (L.d.res >= 0 ? out_b : 0) + (double)L.d.cout * L.kpad * 2;
      snprintf(nm, sizeof nm, "%s", L.d.name);
      if (L.fused_into >= 0 && dual_active(m, m->layers[L.fused_into])) by = fl = 0;   // computed inside the block-closing conv
      if (dual_active(m, L)) {   // no shortcut tensor: reads both inputs, writes the output once
        const Layer& D = m->layers[L.dual_src];
        const TDim& din = m->tdims[D.d.src];
        fl += 2.0 * nb * o.h * o.w * (double)D.d.cout * D.d.cin;
        by = in_b + (double)nb * o.h * o.w * din.c * 2 + out_b + (double)L.d.cout * (L.d.cin + D.d.cin) * 2;
        snprintf(nm, sizeof nm, "%s+%s", L.d.name, D.d.name);
      }
      if (L.bn_head >= 0 && m->layers[L.bn_head].bneck_now_h[0]) by = fl = 0;   // computed by the whole-bottleneck kernel
      if (L.bn_head >= 0 && L.d.k == 1 && m->layers[m->layers[L.bn_head].bn_c2].btail_now_h[0]) by = fl = 0;   // by conv2's launch
      if (L.bn_head >= 0 && L.d.k == 3 && L.btail_now_h[0]) {   // conv2 + conv3 + shortcut (+ chained conv): y1 in, x in, out (+ z)
        const Layer& L3 = m->layers[m->layers[L.bn_head].bn_c3];
        const double px = (double)nb * in.h * in.w;
        fl += 2.0 * px * L3.d.cin * L3.d.cout;
        by = in_b + 2.0 * px * L3.d.cout * 2 + (9.0 * L.d.cin * L.d.cout + (double)L3.d.cin * L3.d.cout) * 2;
        snprintf(nm, sizeof nm, "%.40s+conv3 (one kernel)", L.d.name);
        if (L3.chain_next >= 0 && L3.chained_now_h[0]) {
          const Layer& Q = m->layers[L3.chain_next];
          fl += 2.0 * px * Q.d.cin * Q.d.cout;
          by += px * Q.d.cout * 2 + (double)Q.d.cin * Q.d.cout * 2;
          char both[96];
          snprintf(both, sizeof both, "%.60s>%.30s", nm, Q.d.name);
          snprintf(nm, sizeof nm, "%s", both);
        }
      }
      if (L.bn_c2 >= 0 && L.bneck_now_h[0]) {   // ... launched in this conv's place: x in (+ once more as the shortcut), out
        const Layer& L2 = m->layers[L.bn_c2];
        const Layer& L3 = m->layers[L.bn_c3];
        const double px = (double)nb * in.h * in.w;
        fl = 2.0 * px * ((double)L.d.cin * L.d.cout + 9.0 * L2.d.cin * L2.d.cout + (double)L3.d.cin * L3.d.cout);
        by = 3.0 * in_b + ((double)L.d.cin * L.d.cout + 9.0 * L2.d.cin * L2.d.cout + (double)L3.d.cin * L3.d.cout) * 2;
        snprintf(nm, sizeof nm, "%.40s+conv2+conv3 (one kernel)", L.d.name);
      }
      if (L.chained_by >= 0 && m->layers[L.chained_by].chained_now_h[0]) by = fl = 0;   // computed by the block-closing conv's launch
      const bool by_tail = L.bn_head >= 0 && L.d.k == 1 && m->layers[m->layers[L.bn_head].bn_c2].btail_now_h[0];
      if (L.chain_next >= 0 && L.chained_now_h[0] && !by_tail) {   // ... which also read that conv's weights and wrote its output
        const Layer& Q = m->layers[L.chain_next];
        const TDim& zo = m->tdims[Q.d.dst];
        fl += 2.0 * nb * zo.h * zo.w * (double)Q.d.cout * Q.d.cin;
        by += (double)nb * zo.h * zo.w * zo.c * 2 + (double)Q.d.cout * Q.d.cin * 2;
        char both[96];
        snprintf(both, sizeof both, "%.60s>%.30s", nm, Q.d.name);
        snprintf(nm, sizeof nm, "%s", both);
      }
      if (stem_pool_fused(m, L)) {   // the kernel writes the pooled tensor only
        const TDim& po = m->tdims[m->layers[L.fuse_pool].d.dst];
        by = real_in + (double)nb * po.h * po.w * po.c * 2 + (double)L.d.cout * L.kpad * 2;
        snprintf(nm, sizeof nm, "%s+maxpool", L.d.name);
      }
    } else if (L.d.kind == SPK_OP_LINEAR) {
      fl = 2.0 * nb * L.d.cin * L.d.cout;
      by = in_b + out_b + (double)L.d.cin * L.d.cout * 4;
      snprintf(nm, sizeof nm, "%s", L.d.name);
    } else {
      by = in_b + out_b;
      if (L.d.kind == SPK_OP_DWCONV || L.d.kind == SPK_OP_SE) {
        if (L.d.kind == SPK_OP_DWCONV) fl = 2.0 * nb * o.h * o.w * (double)L.d.cout * L.d.k * L.d.k;
        else by = L.d.dst < (int)m->stale.size() && m->stale[L.d.dst] == 2 ? 0.0 : 3 * in_b;  // pooled once, read and written once by the scale pass (none: gates only)
        snprintf(nm, sizeof nm, "%s", L.d.name);
      } else
      snprintf(nm, sizeof nm, "%s@base.%d",
               L.d.kind == SPK_OP_MAXPOOL ? "maxpool" : (L.d.kind == SPK_OP_GAVGPOOL ? "avgpool" : "dropout"),
               L.d.child);
      if (L.pooled_by_stem && m->stale_stem_t == L.d.src) by = 0;   // computed inside the stem kernel
    }
    put(nm, ms[i + 1], fl, by);
  }
  return cnt;
}
