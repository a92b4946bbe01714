// Model handle: creation, destruction, and the graph analysis that everything else trusts (host side, no kernel).
// spk_graph_build makes no HIP call, so the sanitizer driver (asan_driver.hip) checks it on the CPU.
#include "model.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

static thread_local std::string g_err;
void spk_set_error(const std::string& s) { g_err = s; }
int spk_fail(int code, const std::string& msg) { g_err = msg; return code; }

extern "C" const char* spk_last_error(void) { return g_err.c_str(); }
extern "C" const char* spk_version(void) { return "sykepic_hip 0.1.0 (gfx950)"; }

// ---- graph analysis: one function per pass, in the order spk_graph_build calls them ----
// who reads tensor t (layers that take it as their input, convs that add it as their shortcut operand) and who writes it
Readers spk_readers_of(const spk_model* m, int t) {
  Readers r;
  for (size_t j = 0; j < m->layers.size(); ++j) {
    const Layer& Q = m->layers[j];
    const bool as_src = Q.d.src == t, as_res = Q.d.kind == SPK_OP_CONV && Q.d.res == t;
    r.n_src += as_src;
    r.n_res += as_res;
    if (as_src || as_res) r.last = (int)j;
    if (Q.d.dst == t) r.producer = (int)j;
  }
  return r;
}

static int pass_layers(spk_model* m, const spk_layer_desc* layers, const int32_t* groups, int n_layers) {
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
        (L.d.cout % 8 || (L.d.cin > 4 && L.d.cin % 8)))
      return spk_fail(SPK_ERR_UNSUPPORTED, "channel counts must be multiples of 8");
    if ((L.d.kind == SPK_OP_CONV || L.d.kind == SPK_OP_DWCONV) &&
        (L.d.relu < SPK_ACT_NONE || L.d.relu > SPK_ACT_HSWISH))
      return spk_fail(SPK_ERR_UNSUPPORTED, std::string("unknown activation code on ") + L.d.name);
    if (L.d.relu == SPK_ACT_HSWISH) m->mobilenet = true;
    if (L.d.kind == SPK_OP_CONV) {
      const bool stem = (L.d.cin <= 4);
      const bool stem7 = stem && L.d.k == 7 && L.d.stride == 2 && L.d.pad == 3 && L.d.cout == 64;
      const bool stem3 = stem && L.d.k == 3 && L.d.stride == 2 && L.d.pad == 1;
      if (stem && !stem7 && !stem3)
        return spk_fail(SPK_ERR_UNSUPPORTED, "stems (Cin<=4): 7x7/2 pad 3 -> 64 or 3x3/2 pad 1");
      if (stem7 && L.d.relu == SPK_ACT_HSWISH)   // (conv_stem.hip applies ReLU or nothing)
        return spk_fail(SPK_ERR_UNSUPPORTED, "the 7x7/2 stem: ReLU or no activation");
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
      if ((L.d.k != 3 && L.d.k != 5) || L.d.cin != L.d.cout || L.d.pad != (L.d.k - 1) / 2)
        return spk_fail(SPK_ERR_UNSUPPORTED, "depthwise conv: k 3 or 5, pad (k-1)/2");
      m->effnet = true;
    } else if (L.d.kind == SPK_OP_SE) {
      if (L.d.cin != L.d.cout || L.d.k < 1 || L.d.k > 1024)
        return spk_fail(SPK_ERR_UNSUPPORTED, "squeeze-excitation: cin == cout, 1 <= squeeze <= 1024");
      // the gate pair: 0 SiLU -> Sigmoid (EfficientNet), SPK_ACT_RELU: ReLU -> Hardsigmoid (MobileNetV3)
      if (L.d.relu != SPK_ACT_NONE && L.d.relu != SPK_ACT_RELU)
        return spk_fail(SPK_ERR_UNSUPPORTED, "squeeze-excitation: relu 0 (SiLU / Sigmoid) or 1 (ReLU / Hardsigmoid)");
      if (L.d.relu == SPK_ACT_RELU) m->mobilenet = true;
      m->effnet = true;
    }
  }
  return SPK_OK;
}

static void pass_trunk_roles(spk_model* m) {
  for (Layer& L : m->layers) {
    if (L.d.kind != SPK_OP_CONV) continue;
    const Readers r = spk_readers_of(m, L.d.dst);
    // Layers whose rounding errors enter the residual trunk undamped: the stem,
    // every block-closing conv (it has a shortcut operand) and every conv whose
    // output some other layer adds as a shortcut (downsample branches).
    L.trunk_writer = L.mode == CONV_MODE_STEM || L.d.res >= 0 || r.n_res > 0;
    // shortcut convs (ResNet downsample branches): nothing but a later layer's residual add reads their output, so
    // they are independent of the conv1 -> conv2 chain of their block and may run beside it on a second stream
    L.side_branch = r.n_res > 0 && r.n_src == 0 && L.d.dst != m->layers.back().d.dst;
  }
  // the 3x3 conv in the middle of a bottleneck: its input comes from a 1x1 conv that is not a trunk writer
  for (Layer& L : m->layers) {
    if (L.d.kind != SPK_OP_CONV || L.d.k != 3 || L.trunk_writer) continue;
    for (const Layer& Q : m->layers)
      if (Q.d.kind == SPK_OP_CONV && Q.d.dst == L.d.src && Q.d.k == 1 && !Q.trunk_writer) L.inner3x3 = true;
  }
}

// the ResNet stem (7x7/2 conv + BN + ReLU) followed by the 3x3/2 pad-1 max-pool that alone reads its output: one
// kernel in the eval path (conv_stem.hip, POOL variant)
static void pass_stem_pool(spk_model* m) {
  for (size_t i = 0; i + 1 < m->layers.size(); ++i) {
    Layer& L = m->layers[i];
    Layer& P = m->layers[i + 1];
    if (L.d.kind != SPK_OP_CONV || L.mode != CONV_MODE_STEM || L.d.relu != 1 || L.d.res >= 0) continue;
    if (P.d.kind != SPK_OP_MAXPOOL || P.d.src != L.d.dst || P.d.k != 3 || P.d.stride != 2 || P.d.pad != 1) continue;
    if (spk_readers_of(m, L.d.dst).total() != 1 || L.d.dst == m->layers.back().d.dst) continue;
    L.fuse_pool = (int)(i + 1);
    P.pooled_by_stem = true;
  }
}

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

static void pass_params(spk_model* m) {
  // torch orders a residual block's modules conv1,bn1,conv2,bn2,(conv3,bn3),
  // downsample; the graph runs the downsample branch earlier.  Register the
  // parameters in state_dict order: stable sort of conv layers inside a block.
  const int n_layers = (int)m->layers.size();
  std::vector<int> order;
  for (int i = 0; i < n_layers; ++i) order.push_back(i);
  auto block_of = [&](int i) -> std::string {
    const spk_layer_desc& d = m->layers[i].d;
    std::string nm = d.name;
    size_t p = nm.find(".downsample.");
    if (p != std::string::npos) return nm.substr(0, p);
    p = nm.rfind('.');
    return (d.kind == SPK_OP_CONV && d.child >= 4 && p != std::string::npos) ? nm.substr(0, p) : nm;
  };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    const spk_layer_desc &da_ = m->layers[a].d, &db_ = m->layers[b].d;
    if (da_.kind != SPK_OP_CONV || db_.kind != SPK_OP_CONV) return false;
    if (block_of(a) != block_of(b)) return false;
    const bool da = strstr(da_.name, ".downsample.") != nullptr;
    const bool db = strstr(db_.name, ".downsample.") != nullptr;
    return !da && db;
  });
  for (int oi : order) {
    Layer& L = m->layers[oi];
    const std::string nm = L.d.name, bn = L.d.bn;
    if (L.d.kind == SPK_OP_CONV || L.d.kind == SPK_OP_DWCONV) {
      const int64_t cin_g = L.d.kind == SPK_OP_CONV ? L.d.cin / L.groups : 1;
      L.p_w = add_param(m, nm + ".weight", PK_CONV_W, oi, SPK_DTYPE_F32, {L.d.cout, cin_g, L.d.k, L.d.k}, true);
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
}

// identity bottleneck blocks: conv3 (1x1, + shortcut, ReLU) <- conv2 (3x3 stride 1 pad 1, ReLU) <- conv1 (1x1, ReLU) whose
// input IS conv3's shortcut operand, mid tensors read by nothing else, 4 cm trunk channels (conv_bneck.hip)
static void pass_bottlenecks(spk_model* m) {
  for (size_t i3 = 0; i3 < m->layers.size(); ++i3) {
    Layer& L3 = m->layers[i3];
    if (L3.d.kind != SPK_OP_CONV || L3.d.k != 1 || L3.d.stride != 1 || L3.d.pad != 0 || L3.d.res < 0 || L3.d.relu != 1) continue;
    // the writer of t when exactly one layer reads t and t is not the network's output: what a fused kernel may keep to itself
    auto mid = [&](int t) {
      const Readers r = spk_readers_of(m, t);
      return r.total() == 1 && t != m->layers.back().d.dst ? r.producer : -1;
    };
    const int i2 = mid(L3.d.src);
    if (i2 < 0) continue;
    Layer& L2 = m->layers[i2];
    if (L2.d.kind != SPK_OP_CONV || L2.d.k != 3 || L2.d.stride != 1 || L2.d.pad != 1 || L2.d.res >= 0 || L2.d.relu != 1) continue;
    const int i1 = mid(L2.d.src);
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
}

// packed bf16 weights + folded BN scale/bias, and the activation-mean vector
static void pass_packed_layout(spk_model* m) {
  size_t &wpack = m->n_wpack, &sb = m->n_sb, &dwp = m->n_dwp;
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
  // per-channel means of every generic conv's input (zero_sum.hip): one flat vector, graph order
  for (Layer& L : m->layers) {
    if (L.d.kind != SPK_OP_CONV || (L.mode != CONV_MODE_GENERIC && L.mode != CONV_MODE_STEM)) continue;
    L.mu_off = m->n_means;   // (the 7x7 stem: the image's own channel means)
    m->n_means += (size_t)L.d.cin;
  }
}

// block-closing 1x1 conv + the 1x1 shortcut conv whose output only it adds: one K-concatenated GEMM in the eval path
static void pass_dual_pairs(spk_model* m) {
  for (size_t i = 0; i < m->layers.size(); ++i) {
    Layer& L = m->layers[i];
    if (L.d.kind != SPK_OP_CONV || !L.pw_ok || L.d.res < 0 || L.d.stride != 1) continue;
    for (size_t j = 0; j < m->layers.size(); ++j) {
      Layer& D = m->layers[j];
      if (D.d.kind != SPK_OP_CONV || D.d.dst != L.d.res || !D.pw_ok || !D.side_branch || D.d.relu != 0 || D.d.res >= 0 ||
          D.d.cout != L.d.cout || D.fused_into >= 0)
        continue;
      if (spk_readers_of(m, D.d.dst).total() != 1) continue;
      L.dual_src = (int)j;
      D.fused_into = (int)i;
      L.wdual_off = m->n_wdual;
      m->n_wdual += (size_t)2 * L.d.cout * (L.d.cin + D.d.cin);
      L.sdual_off = m->n_sdual;
      m->n_sdual += (size_t)2 * L.d.cout;
    }
  }
}

// block-closing conv -> the next block's first conv (both 1x1, stride 1, 256 -> 64 / 128 channels in between)
static void pass_chain_pairs(spk_model* m) {
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
}

// MBConv blocks: the squeeze-excitation -> project conv pairs whose scaling the conv can apply itself (fp16 eval), and the
// producers / readers the executor would otherwise search for at every launch
static void pass_mbconv(spk_model* m) {
  for (size_t si = 0; si < m->layers.size(); ++si) {
    Layer& S = m->layers[si];
    if (S.d.kind != SPK_OP_SE) continue;
    const int di = spk_readers_of(m, S.d.src).producer;
    if (di >= 0 && m->layers[di].d.kind == SPK_OP_DWCONV) S.se_dw = di;
    for (Layer& P : m->layers)
      if (P.d.kind == SPK_OP_CONV && P.d.src == S.d.dst) P.src_se = (int)si;
    const Readers r = spk_readers_of(m, S.d.dst);
    if (r.total() != 1 || S.d.dst == m->layers.back().d.dst) continue;
    Layer& P = m->layers[r.last];
    if (P.d.kind != SPK_OP_CONV || P.mode != CONV_MODE_GENERIC || P.d.k != 1 || P.d.stride != 1 || P.d.pad != 0 ||
        P.d.src != S.d.dst)
      continue;
    S.gate_conv = r.last;
    P.gate_from = (int)si;
  }
  for (Layer& L : m->layers)
    for (size_t j = 0; j < m->layers.size() && L.d.kind == SPK_OP_CONV && L.exp_next < 0; ++j)
      if (m->layers[j].d.src == L.d.dst && spk_expand_shaped(m->layers[j].d)) L.exp_next = (int)j;
}

int spk_graph_build(spk_model* m, const spk_layer_desc* layers, const int32_t* groups, int n) {
  SPK_TRY(pass_layers(m, layers, groups, n));
  pass_trunk_roles(m);
  pass_stem_pool(m);
  pass_params(m);
  pass_bottlenecks(m);
  pass_packed_layout(m);
  pass_dual_pairs(m);
  pass_chain_pairs(m);
  pass_mbconv(m);
  return SPK_OK;
}

// ---- construction ----
extern "C" int spk_model_create(const spk_layer_desc* layers, int n_layers, int in_chans,
                                int num_classes, int device, spk_model** out) {
  return spk_model_create_grouped(layers, nullptr, n_layers, in_chans, num_classes, device, out);
}

extern "C" int spk_model_create_grouped(const spk_layer_desc* layers, const int32_t* groups, int n_layers, int in_chans,
                                        int num_classes, int device, spk_model** out) {
  if (!layers || n_layers <= 0 || !out) return spk_fail(SPK_ERR_ARG, "spk_model_create: bad arguments");
  for (int i = 0; groups && i < n_layers; ++i) {
    const spk_layer_desc& d = layers[i];
    if (groups[i] < 1) return spk_fail(SPK_ERR_ARG, "spk_model_create_grouped: groups must be >= 1");
    if (groups[i] == 1) continue;
    if (d.kind != SPK_OP_CONV || d.cin != d.cout || d.res >= 0 || d.relu > SPK_ACT_RELU ||
        !spk_group_conv_ok(d.cin, groups[i], d.k, d.stride, d.pad))
      return spk_fail(SPK_ERR_UNSUPPORTED, std::string("grouped conv ") + d.name +
                                               ": needs k 3, pad 1, stride 1 or 2, cin == cout a multiple of 16, 4 / 8 / 16 / 32 / "
                                               "64 channels per group, no shortcut, no activation but ReLU");
  }
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev)
    return spk_fail(SPK_ERR_HIP, "spk_model_create: no such HIP device " + std::to_string(device));
  HIP_TRY(hipSetDevice(device));
  spk_model* m = new spk_model();
  m->device = device;
  m->in_chans = in_chans;
  m->num_classes = num_classes;
  if (in_chans < 1 || in_chans > 4) { delete m; return spk_fail(SPK_ERR_UNSUPPORTED, "in_chans must be 1..4"); }
  if (const int r = spk_graph_build(m, layers, groups, n_layers)) { delete m; return r; }
  if (const char* e = getenv("SPK_FUSE_STEM_POOL")) m->fuse_stem_pool = atoi(e) != 0;
  if (const char* e = getenv("SPK_FUSE_DS")) m->fuse_ds = atoi(e) != 0;
  if (const char* e = getenv("SPK_SE_FUSE")) m->fuse_se = atoi(e) != 0;
  if (const char* e = getenv("SPK_BNECK")) m->bneck = atoi(e);
  if (const char* e = getenv("SPK_BTAIL")) m->btail = atoi(e);
  if (const char* e = getenv("SPK_CHAIN")) m->chain = atoi(e);
  if (hipMalloc((void**)&m->pbuf, m->n_flat * sizeof(float)) != hipSuccess) {
    delete m; return spk_fail(SPK_ERR_HIP, "hipMalloc(params) failed");
  }
  hipMemset(m->pbuf, 0, m->n_flat * sizeof(float));
  // BN defaults as torch: gamma 1, running_var 1
  for (Param& p : m->params) {
    if (p.kind == PK_BN_W || p.kind == PK_BN_VAR) {
      std::vector<float> ones((size_t)p.numel, 1.0f);
      hipMemcpy(m->pbuf + p.off, ones.data(), ones.size() * 4, hipMemcpyHostToDevice);
    }
  }
  if (hipMalloc((void**)&m->act_mean_dev, std::max<size_t>(m->n_means, 8) * 4) != hipSuccess ||
      hipMalloc((void**)&m->wpack, std::max<size_t>(m->n_wpack, 8) * 2) != hipSuccess ||
      hipMalloc((void**)&m->dwpack, std::max<size_t>(m->n_dwp, 8) * 4) != hipSuccess ||
      hipMalloc((void**)&m->wdual, std::max<size_t>(m->n_wdual, 8) * 2) != hipSuccess ||
      hipMalloc((void**)&m->sdual, std::max<size_t>(m->n_sdual, 8) * 4) != hipSuccess ||
      hipMalloc((void**)&m->scale_bias, std::max<size_t>(m->n_sb, 8) * 4) != hipSuccess) {
    spk_model_destroy(m);
    return spk_fail(SPK_ERR_HIP, "hipMalloc(packed weights) failed");
  }
  m->dirty = true;
  *out = m;
  return SPK_OK;
}

void spk_free_acts(spk_model* m) {
  if (m->arena) hipFree(m->arena);
  m->arena = nullptr;
  m->arena_bytes = 0;
  m->cap_n = m->cap_h = m->cap_w = 0;
}

extern "C" void spk_model_destroy(spk_model* m) {
  if (!m) return;
  hipSetDevice(m->device);
  hipDeviceSynchronize();
  spk_free_acts(m);
  for (void* p : {(void*)m->pbuf, (void*)m->ema, (void*)m->wpack, (void*)m->scale_bias, (void*)m->dwpack, (void*)m->wdual,
                  (void*)m->sdual, (void*)m->act_mean_dev, (void*)m->w8pack, (void*)m->fp8_shadow, (void*)m->s8, (void*)m->loss_w,
                  (void*)m->class_counts})
    if (p) hipFree(p);
  if (m->half_stream) hipStreamDestroy(m->half_stream);
  if (m->half_fork) hipEventDestroy(m->half_fork);
  if (m->half_join) hipEventDestroy(m->half_join);
  spk_train_free(m);
  delete m;
}

extern "C" int spk_model_set_stream(spk_model* m, void* s) {
  if (!m) return spk_fail(SPK_ERR_ARG, "null model");
  if (m->stream == (hipStream_t)s) return SPK_OK;   // (the host side sets the stream in front of every call)
  m->stream = (hipStream_t)s;
  // a training step may have left a weight gradient running on the side stream: what comes next runs on the NEW stream
  if (spk_train_join(m) != SPK_OK) return spk_fail(SPK_ERR_HIP, "set_stream: joining the side stream failed");
  return SPK_OK;
}
