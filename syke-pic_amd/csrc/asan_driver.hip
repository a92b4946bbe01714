// Host-side sanitizer driver (the reference has no native code, so no sanitizer story; this
// library has ~9 k lines of it).  Built by `build.sh asan` with -fsanitize=address,undefined on the HOST pass of every
// translation unit and run on the CPU (tests/test_abi.py): it walks the host logic that does not need a GPU - handle
// creation and its error paths, the parameter table, spk_last_error, the graph analysis, the eval executor's cursor
// addressing and twin rebase (on addresses only), the conv descriptor builders (conv_args.h), and the tuner table
// (tune_table.h: one parser for the tags of the tune-cache file, the nearest-batch rule, the appended lines) - so that heap overflows,
// use-after-free and undefined behaviour there abort the run.  With no GPU every HIP call fails and the error paths
// are what runs; on a GPU box the same binary works on real (small) buffers.  argv[1]: the shipped tuning seed
// (default: the source tree's).
#include "model.h"
#include "conv_args.h"
#include "tune_table.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "asan_driver: %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static spk_layer_desc conv(const char* name, const char* bn, int cin, int cout, int k, int s, int p, int src, int dst,
                           int res, int relu, int child) {
  spk_layer_desc d;
  memset(&d, 0, sizeof d);
  d.kind = SPK_OP_CONV; d.cin = cin; d.cout = cout; d.k = k; d.stride = s; d.pad = p; d.relu = relu;
  d.src = src; d.dst = dst; d.res = res; d.child = child;
  snprintf(d.name, sizeof d.name, "%s", name);
  snprintf(d.bn, sizeof d.bn, "%s", bn);
  return d;
}

// ---- the tuner table ----
// every non-comment line of a tune-cache file: its tag and its ints
struct TuneLine { std::string text; int tag; std::vector<int> v; };
static std::vector<TuneLine> read_tune_lines(const std::string& path) {
  std::vector<TuneLine> out;
  FILE* f = fopen(path.c_str(), "r");
  char buf[1024];
  while (f && fgets(buf, sizeof buf, f)) {
    if (buf[0] == '#' || buf[0] == '\n') continue;
    TuneLine l;
    l.text = buf;
    l.tag = -1;
    std::istringstream in(l.text);
    std::string tag;
    in >> tag;
    for (int t = 0; t < TUNE_NTAGS; ++t)
      if (kTuneSchemas[t].tag && tag == kTuneSchemas[t].tag) l.tag = t;
    for (int x; in >> x;) l.v.push_back(x);
    out.push_back(l);
  }
  if (f) fclose(f);
  return out;
}
// -1000: absent, else the (first) stored value
static int look(TuneTag t, std::vector<int> key, int* second = nullptr) {
  int v[2] = {0, 0};
  if (!spk_tune_find(t, key.data(), v)) return -1000;
  if (second) *second = v[1];
  return v[0];
}
static void use_cache(const char* path) {   // what a fresh process with this SPK_TUNE_CACHE would see
  if (path) setenv("SPK_TUNE_CACHE", path, 1);
  else unsetenv("SPK_TUNE_CACHE");
  spk_tune_reset_for_test();
}

static void tuner_table_checks(const std::string& tmp, const std::string& seed_path) {
  const char* seed = seed_path.c_str();
  // the path rule
  unsetenv("SPK_TUNE_CACHE");
  EXPECT(spk_tune_cache_path() == nullptr);
  setenv("SPK_TUNE_CACHE", "", 1);
  EXPECT(spk_tune_cache_path() == nullptr);
  setenv("SPK_TUNE_CACHE", "off", 1);
  EXPECT(spk_tune_cache_path() == nullptr);
  setenv("SPK_TUNE_CACHE", "offline.txt", 1);
  EXPECT(spk_tune_cache_path() && !strcmp(spk_tune_cache_path(), "offline.txt"));

  // the nearest-batch rule, on entries that stay in the process (no file)
  use_cache(nullptr);
  const int a = 3, b = 7;
  const int k64[] = {1, 14, 14, 256, 256, 64}, k256[] = {1, 14, 14, 256, 256, 256}, other[] = {1, 14, 14, 256, 512, 90};
  spk_tune_store(TUNE_C3, k64, &a, true);
  spk_tune_store(TUNE_C3, k256, &b, true);
  spk_tune_store(TUNE_C3, other, &b, true);   // another problem between the two batches: never a match
  EXPECT(look(TUNE_C3, {1, 14, 14, 256, 256, 64}) == a);
  EXPECT(look(TUNE_C3, {1, 14, 14, 256, 256, 100}) == a);
  EXPECT(look(TUNE_C3, {1, 14, 14, 256, 256, 128}) == b);    // a tie goes to the larger batch
  EXPECT(look(TUNE_C3, {1, 14, 14, 256, 256, 512}) == b);
  EXPECT(look(TUNE_C3, {1, 14, 14, 256, 256, 600}) == -1000);
  EXPECT(look(TUNE_C3, {1, 14, 14, 256, 256, 31}) == -1000);
  EXPECT(look(TUNE_C3, {1, 14, 14, 256, 128, 64}) == -1000);
  const int cv[] = {4, 3}, ck[] = {0, 1, 1, 64, 14, 14, 256, 256, 3, 1, 16, 0, 0};   // conv: N is the 4th field
  spk_tune_store(TUNE_CONV, ck, cv, true);
  int dma = -1;
  EXPECT(look(TUNE_CONV, {0, 1, 1, 100, 14, 14, 256, 256, 3, 1, 16, 0, 0}, &dma) == 4 && dma == 3);
  EXPECT(look(TUNE_CONV, {0, 1, 1, 64, 14, 14, 256, 256, 3, 1, 16, 0, 1}) == -1000);
  EXPECT(look(TUNE_CONV, {0, 1, 1, 64, 28, 14, 256, 256, 3, 1, 16, 0, 0}) == -1000);
  const int one = 1, wk[] = {6272, 256, 256, 3, 1, 0, 13, 128128}, dk[] = {0, 64, 28, 28, 240, 5, 1};
  spk_tune_store(TUNE_WGRAD, wk, &one, true);                  // no batch field: exact matches only
  spk_tune_store(TUNE_DW, dk, &one, true);                     // (asked to persist: still never written)
  EXPECT(look(TUNE_WGRAD, {6272, 256, 256, 3, 1, 0, 13, 128128}) == 1);
  EXPECT(look(TUNE_WGRAD, {6273, 256, 256, 3, 1, 0, 13, 128128}) == -1000);
  EXPECT(look(TUNE_WGRAD, {6272, 256, 256, 3, 1, 0, 13, 128129}) == -1000);
  EXPECT(look(TUNE_DW, {0, 64, 28, 28, 240, 5, 1}) == 1);
  EXPECT(look(TUNE_DW, {0, 65, 28, 28, 240, 5, 1}) == -1000);
  EXPECT(look(TUNE_DW, {0, 64, 28, 28, 240, 5, 2}) == -1000);

  // the paired siblings: entries of their own - neither answers for the other - chosen by the thread's twin context
  EXPECT(spk_tune_tag(TUNE_C3) == TUNE_C3 && spk_tune_tag(TUNE_WGRAD) == TUNE_WGRAD);
  spk_twin().mode = SpkTwin::LOOKUP;
  EXPECT(spk_tune_tag(TUNE_CONV) == TUNE_CONV_P && spk_tune_tag(TUNE_PW1) == TUNE_PW1_P && spk_tune_tag(TUNE_PW2) == TUNE_PW2_P &&
         spk_tune_tag(TUNE_C3) == TUNE_C3_P && spk_tune_tag(TUNE_CHAIN) == TUNE_CHAIN_P && spk_tune_tag(TUNE_BNECK) == TUNE_BNECK_P &&
         spk_tune_tag(TUNE_D3) == TUNE_D3_P && spk_tune_tag(TUNE_WGRAD) == TUNE_WGRAD && spk_tune_tag(TUNE_DW) == TUNE_DW);
  EXPECT(look(spk_tune_tag(TUNE_C3), {1, 14, 14, 256, 256, 64}) == -1000);   // the isolated entry above is not a paired one
  const int pk[] = {1, 14, 14, 256, 256, 128}, pv = 11, bk[] = {14, 256, 128}, bv = 1;
  spk_tune_store(spk_tune_tag(TUNE_C3), pk, &pv, true);
  spk_tune_store(spk_tune_tag(TUNE_BNECK), bk, &bv, true);
  EXPECT(look(spk_tune_tag(TUNE_C3), {1, 14, 14, 256, 256, 128}) == pv && look(spk_tune_tag(TUNE_C3), {1, 14, 14, 256, 256, 129}) == pv);
  EXPECT(look(spk_tune_tag(TUNE_BNECK), {14, 256, 128}) == bv);
  spk_twin() = SpkTwin();
  EXPECT(look(spk_tune_tag(TUNE_C3), {1, 14, 14, 256, 256, 128}) == b && look(TUNE_BNECK, {14, 256, 128}) == -1000);
  for (int t = TUNE_CONV_P; t <= TUNE_D3_P; ++t) {   // a paired line is its sibling's line behind another tag
    const TuneSchema &p = kTuneSchemas[t], &q = kTuneSchemas[t - TUNE_CONV_P <= TUNE_BNECK ? t - TUNE_CONV_P : TUNE_D3];
    EXPECT(p.tag && q.tag && std::string(p.tag) == std::string(q.tag) + "_p");
    EXPECT(p.n_key == q.n_key && p.n_pos == q.n_pos && p.n_val == q.n_val && p.val_min == q.val_min && p.val_max == q.val_max);
  }

  // the shipped seed: loads whole, and writing every entry back through spk_tune_store gives the seed's own lines
  std::vector<TuneLine> lines = read_tune_lines(seed);
  EXPECT(lines.size() == 282);
  use_cache(seed);
  (void)look(TUNE_BNECK, {0, 0, 0});
  EXPECT(spk_tune_detail::table().map.size() == lines.size());   // every line an entry, no key twice
  remove(tmp.c_str());
  setenv("SPK_TUNE_CACHE", tmp.c_str(), 1);                      // (the path is looked up when a line is appended)
  bool tags[TUNE_NTAGS] = {};
  for (const TuneLine& l : lines) {
    EXPECT(l.tag >= 0);
    if (l.tag < 0) continue;
    tags[l.tag] = true;
    const TuneSchema& sc = kTuneSchemas[l.tag];
    EXPECT((int)l.v.size() == sc.n_key + sc.n_val);
    int v[2] = {-1000, -1000};
    EXPECT(spk_tune_find((TuneTag)l.tag, l.v.data(), v));
    for (int i = 0; i < sc.n_val; ++i) EXPECT(v[i] == l.v[sc.n_key + i]);
    spk_tune_store((TuneTag)l.tag, l.v.data(), v, true);
  }
  EXPECT(std::count(tags, tags + TUNE_NTAGS, true) == 6);
  std::vector<TuneLine> back = read_tune_lines(tmp);
  auto by_text = [](const TuneLine& x, const TuneLine& y) { return x.text < y.text; };
  std::sort(lines.begin(), lines.end(), by_text);
  std::sort(back.begin(), back.end(), by_text);
  EXPECT(back.size() == lines.size());
  for (size_t i = 0; i < lines.size() && i < back.size(); ++i) EXPECT(back[i].text == lines[i].text);

  // one new entry per tag appended to that file, then a fresh table: each is found (and so is the seed's first line)
  const std::vector<std::vector<int>> fresh = {
      {2, 1, 0, 5, 9, 9, 64, 64, 3, 1, 16, 1, 0, 6, 5}, {1, 9, 9, 64, 64, 1, 0, 1, 5, -1}, {1, 9, 9, 64, 18, 18, 64, 128, 1, 2, 5, 17},
      {2, 9, 9, 64, 64, 5, 13}, {9, 9, 64, 0, 64, 5, 0}, {9, 64, 5, 2}, {81, 64, 64, 3, 1, 0, 1, 64064, 1}};
  for (int t = 0; t < (int)fresh.size(); ++t) spk_tune_store((TuneTag)t, fresh[t].data(), fresh[t].data() + kTuneSchemas[t].n_key, true);
  spk_tune_store(TUNE_DW, dk, &one, true);
  const int d3_fresh[] = {9, 9, 1, 5, kD3NumCfgs - 1};                  // the tag behind the depthwise one: not in `fresh`
  spk_tune_store(TUNE_D3, d3_fresh, d3_fresh + kTuneSchemas[TUNE_D3].n_key, true);
  EXPECT(read_tune_lines(tmp).size() == lines.size() + fresh.size() + 1);   // (nothing for the depthwise choice)
  use_cache(tmp.c_str());
  EXPECT(look(TUNE_D3, {9, 9, 1, 5}) == kD3NumCfgs - 1);
  EXPECT(look(TUNE_D3, {9, 9, 1, 8}) == kD3NumCfgs - 1);                // the nearest-batch rule holds for it too
  EXPECT(look(TUNE_D3, {9, 9, 0, 5}) == -1000);
  for (int t = 0; t < (int)fresh.size(); ++t) {
    int v[2] = {-1000, -1000};
    EXPECT(spk_tune_find((TuneTag)t, fresh[t].data(), v));
    for (int i = 0; i < kTuneSchemas[t].n_val; ++i) EXPECT(v[i] == fresh[t][kTuneSchemas[t].n_key + i]);
  }
  EXPECT(look(TUNE_DW, {0, 64, 28, 28, 240, 5, 1}) == -1000);
  EXPECT(spk_tune_detail::table().map.size() == lines.size() + fresh.size() + 1);
  remove(tmp.c_str());
}

// ---- the graph analysis (spk_graph_build, model_graph.hip): no HIP call, so it runs here whatever the host ----
static spk_layer_desc op(int kind, const char* name, int cin, int cout, int k, int s, int p, int src, int dst, int relu, int child) {
  spk_layer_desc d = conv(name, name, cin, cout, k, s, p, src, dst, -1, relu, child);
  d.kind = kind;
  return d;
}

static void graph_checks() {
  // the ResNet stem + max-pool, a stage-1-shaped stage (a downsample block and two identity blocks, 256-channel trunk, cm 64)
  // and the first (downsample) block of the next stage
  std::vector<spk_layer_desc> g;
  g.push_back(conv("base.0", "base.1", 3, 64, 7, 2, 3, 0, 1, -1, 1, 0));                                     // 0
  g.push_back(op(SPK_OP_MAXPOOL, "base.3", 64, 64, 3, 2, 1, 1, 2, 0, 3));                                    // 1
  g.push_back(conv("base.4.0.conv1", "base.4.0.bn1", 64, 64, 1, 1, 0, 2, 3, -1, 1, 4));                      // 2
  g.push_back(conv("base.4.0.conv2", "base.4.0.bn2", 64, 64, 3, 1, 1, 3, 4, -1, 1, 4));                      // 3
  g.push_back(conv("base.4.0.downsample.0", "base.4.0.downsample.1", 64, 256, 1, 1, 0, 2, 5, -1, 0, 4));     // 4
  g.push_back(conv("base.4.0.conv3", "base.4.0.bn3", 64, 256, 1, 1, 0, 4, 6, 5, 1, 4));                      // 5
  g.push_back(conv("base.4.1.conv1", "base.4.1.bn1", 256, 64, 1, 1, 0, 6, 7, -1, 1, 4));                     // 6
  g.push_back(conv("base.4.1.conv2", "base.4.1.bn2", 64, 64, 3, 1, 1, 7, 8, -1, 1, 4));                      // 7
  g.push_back(conv("base.4.1.conv3", "base.4.1.bn3", 64, 256, 1, 1, 0, 8, 9, 6, 1, 4));                      // 8
  g.push_back(conv("base.4.2.conv1", "base.4.2.bn1", 256, 64, 1, 1, 0, 9, 10, -1, 1, 4));                    // 9
  g.push_back(conv("base.4.2.conv2", "base.4.2.bn2", 64, 64, 3, 1, 1, 10, 11, -1, 1, 4));                    // 10
  g.push_back(conv("base.4.2.conv3", "base.4.2.bn3", 64, 256, 1, 1, 0, 11, 12, 9, 1, 4));                    // 11
  g.push_back(conv("base.5.0.conv1", "base.5.0.bn1", 256, 128, 1, 1, 0, 12, 13, -1, 1, 5));                  // 12
  g.push_back(conv("base.5.0.conv2", "base.5.0.bn2", 128, 128, 3, 2, 1, 13, 14, -1, 1, 5));                  // 13
  g.push_back(conv("base.5.0.downsample.0", "base.5.0.downsample.1", 256, 512, 1, 2, 0, 12, 15, -1, 0, 5));  // 14
  g.push_back(conv("base.5.0.conv3", "base.5.0.bn3", 128, 512, 1, 1, 0, 14, 16, 15, 1, 5));                  // 15
  g.push_back(op(SPK_OP_GAVGPOOL, "base.8", 512, 512, 1, 1, 0, 16, 17, 0, 8));                               // 16
  g.push_back(op(SPK_OP_LINEAR, "head.0", 512, 10, 1, 1, 0, 17, 18, 0, -1));                                 // 17
  {
    spk_model m;
    EXPECT(spk_graph_build(&m, g.data(), nullptr, (int)g.size()) == SPK_OK);
    const std::vector<Layer>& L = m.layers;
    const int nl = (int)L.size();
    EXPECT(nl == 18 && m.n_tensors == 19 && !m.effnet);
    EXPECT(L[0].fuse_pool == 1 && L[1].pooled_by_stem);
    for (int c : {5, 15}) {   // block-closing conv + shortcut conv, the second with a stride-2 shortcut
      EXPECT(L[c].dual_src == c - 1 && L[c - 1].fused_into == c && L[c - 1].side_branch);
    }
    for (int c : {5, 8, 11}) {   // block-closing conv -> the next block's conv1; the last one crosses the stage (256 -> 128)
      EXPECT(L[c].chain_next == c + 1 && L[c + 1].chained_by == c);
    }
    EXPECT(L[15].chain_next == -1);
    for (int h : {6, 9}) {   // the two identity blocks
      EXPECT(L[h].bn_c2 == h + 1 && L[h].bn_c3 == h + 2 && L[h + 1].bn_head == h && L[h + 2].bn_head == h);
    }
    for (int h : {2, 3, 4, 5, 12, 13, 14, 15}) EXPECT(L[h].bn_c2 == -1 && L[h].bn_c3 == -1 && L[h].bn_head == -1);
    for (int c : {3, 7, 10}) EXPECT(L[c].d3_ok && L[c].inner3x3);
    EXPECT(!L[13].d3_ok);
    size_t pairs = 0;
    for (int i = 0; i < nl; ++i) {   // every index in range, every pair closed
      const Layer& Q = L[i];
      for (int idx : {Q.dual_src, Q.fused_into, Q.chain_next, Q.chained_by, Q.bn_c2, Q.bn_c3, Q.bn_head, Q.gate_conv, Q.gate_from,
                      Q.se_dw, Q.src_se, Q.exp_next, Q.fuse_pool})
        EXPECT(idx >= -1 && idx < nl);
      for (int pi : {Q.p_w, Q.p_g, Q.p_b, Q.p_mean, Q.p_var, Q.p_nbt, Q.p_w2, Q.p_b2}) EXPECT(pi >= -1 && pi < (int)m.params.size());
      if (Q.dual_src >= 0) { EXPECT(L[Q.dual_src].fused_into == i); ++pairs; }
      if (Q.chain_next >= 0) { EXPECT(L[Q.chain_next].chained_by == i); ++pairs; }
      EXPECT(Q.gate_conv == -1 && Q.gate_from == -1 && Q.se_dw == -1 && Q.src_se == -1);
    }
    EXPECT(pairs == 5);
    EXPECT(m.n_wpack > 0 && m.n_sb > 0 && m.n_wdual == (size_t)2 * (256 * (64 + 64) + 512 * (128 + 256)) && m.n_sdual == 2 * (256 + 512));
    EXPECT(m.n_flat >= m.n_train && m.n_train > 0 && m.n_means > 0);
    for (const Param& p : m.params) EXPECT(p.dtype != SPK_DTYPE_F32 || p.off + (size_t)p.numel <= m.n_flat);
    // state_dict order: a block's downsample conv is registered behind its conv3
    EXPECT(m.index.at("base.4.0.conv3.weight") < m.index.at("base.4.0.downsample.0.weight"));
  }
  // one MBConv block behind a 3x3 stem: expand 1x1, depthwise, squeeze-excitation, project (+ the trunk)
  std::vector<spk_layer_desc> e;
  e.push_back(conv("base.0.0", "base.0.1", 3, 32, 3, 2, 1, 0, 1, -1, SPK_ACT_SILU, 0));                       // 0
  e.push_back(conv("base.1.0.expand", "base.1.0.bn0", 32, 128, 1, 1, 0, 1, 2, -1, SPK_ACT_SILU, 1));          // 1
  e.push_back(conv("base.1.0.dw", "base.1.0.bn1", 128, 128, 3, 1, 1, 2, 3, -1, SPK_ACT_SILU, 1));             // 2
  e.back().kind = SPK_OP_DWCONV;
  e.push_back(op(SPK_OP_SE, "base.1.0.se", 128, 128, 8, 1, 0, 3, 4, SPK_ACT_NONE, 1));                        // 3
  e.push_back(conv("base.1.0.project", "base.1.0.bn2", 128, 32, 1, 1, 0, 4, 5, 1, SPK_ACT_NONE, 1));          // 4
  e.push_back(conv("base.2.0.expand", "base.2.0.bn0", 32, 128, 1, 1, 0, 5, 6, -1, SPK_ACT_SILU, 2));          // 5: the next block's
  e.push_back(op(SPK_OP_GAVGPOOL, "base.8", 128, 128, 1, 1, 0, 6, 7, 0, 8));                                  // 6
  e.push_back(op(SPK_OP_LINEAR, "head.0", 128, 10, 1, 1, 0, 7, 8, 0, -1));                                    // 7
  {
    spk_model m;
    EXPECT(spk_graph_build(&m, e.data(), nullptr, (int)e.size()) == SPK_OK);
    const std::vector<Layer>& L = m.layers;
    EXPECT(L.size() == 8 && m.effnet && !m.mobilenet);
    EXPECT(L[3].gate_conv == 4 && L[4].gate_from == 3);
    EXPECT(L[3].se_dw == 2 && L[4].src_se == 3);
    // the expand conv behind a conv (what the fp8 project conv leaves its e4m3 copy for); none behind an expand conv itself
    EXPECT(L[0].exp_next == 1 && L[4].exp_next == 5 && L[1].exp_next == -1 && L[5].exp_next == -1);
    for (const Layer& Q : L) EXPECT(Q.dual_src == -1 && Q.chain_next == -1 && Q.bn_c2 == -1 && Q.bn_head == -1 && Q.fuse_pool == -1);
    EXPECT(m.n_dwp > 0 && L[3].p_w2 >= 0 && L[3].p_b2 >= 0);
    // a squeeze-excitation layer must not be wider than 1024 hidden units: the error path leaves nothing behind
    e[3].k = 2000;
    spk_model bad;
    EXPECT(spk_graph_build(&bad, e.data(), nullptr, (int)e.size()) == SPK_ERR_UNSUPPORTED && strlen(spk_last_error()) > 0);
  }
}

// ---- the half-batch cursor and the twin rebase of the eval executor (model.h, model.hip): addresses in a host buffer
// that stands for the arena - nothing is dereferenced, no HIP call ----
static void cursor_checks() {
  spk_model m;
  std::vector<char> arena(1024);
  char* const a = arena.data();
  m.arena = a;
  m.arena_bytes = arena.size();
  m.cap_n = 5;
  m.n_tensors = 3;
  m.tdims = {{2, 2, 4, true}, {1, 3, 8, true}, {1, 1, 10, false}};
  const size_t img[3] = {2 * 2 * 4 * 2, 1 * 3 * 8 * 2, 1 * 1 * 10 * 4};   // bytes per image: two 2-byte tensors, one 4-byte
  m.toff = {0, 256, 512};
  m.se_off = 768;
  m.se_stride = 6;
  const EvalCursor ch[2] = {{0, 0, 2, nullptr}, {1, 2, 3, nullptr}};      // five images as halves of 2 + 3
  EvalTwin tw[2] = {{&m, 0, 2, 3, false}, {&m, 2, 0, 2, false}};
  for (int t = 0; t < 3; ++t)
    for (int hf = 0; hf < 2; ++hf) {
      EXPECT((char*)m.TI(ch[hf], t) == a + m.toff[t] + ch[hf].img0 * img[t]);
      // this half's first image of the tensor becomes the twin's first image, in both directions
      const void* p = m.TI(ch[hf], t);
      EXPECT(spk_twin_rebase(&tw[hf], &p) && p == m.TI(ch[1 - hf], t));
      // any other image of the tensor has no twin
      const void* inner = (char*)m.TI(ch[hf], t) + img[t];
      p = inner;
      EXPECT(!spk_twin_rebase(&tw[hf], &p) && p == inner);
    }
  EXPECT((char*)m.TI8(ch[1], 1) == a + m.toff[1] + 2 * img[1] / 2);
  EXPECT(m.SE(ch[0]) == (float*)(a + m.se_off) && m.SE(ch[1]) == (float*)(a + m.se_off) + 2 * m.se_stride);
  for (int hf = 0; hf < 2; ++hf) {
    // a pointer outside the arena (weights, folded BatchNorm) stays as it is
    const void* outside[2] = {&m, a + arena.size()};
    for (const void* o : outside) {
      const void* p = o;
      EXPECT(spk_twin_rebase(&tw[hf], &p) && p == o);
    }
    // the scratch at and behind se_off is no per-image slice of a tensor
    const void* scratch[3] = {a + m.se_off, m.SE(ch[hf]) + 1, a + arena.size() - 1};
    for (const void* o : scratch) {
      const void* p = o;
      EXPECT(!spk_twin_rebase(&tw[hf], &p) && p == o);
    }
  }
  // a twin whose images would pass the plan's capacity
  EvalTwin past = {&m, 0, 2, 4, false};
  const void* p = m.T(0);
  EXPECT(!spk_twin_rebase(&past, &p) && p == m.T(0));
  past.twin_n = 3;
  EXPECT(spk_twin_rebase(&past, &p) && p == m.TI(ch[1], 0));
}

// ---- the descriptor builders (conv_args.h): derived fields against numbers worked out by hand, and every field a
// builder does not set left at zero.  Pointers are made-up addresses - nothing is dereferenced, no HIP call ----
template <class T> static T zeroed() { T t; memset(&t, 0, sizeof t); return t; }
template <class T> static bool same_bytes(const T& a, const T& b) { return memcmp(&a, &b, sizeof(T)) == 0; }
static void descriptor_checks() {
  bf16_t *const X = (bf16_t*)0x1000, *const Y = (bf16_t*)0x2000, *const Wt = (bf16_t*)0x3000, *const R = (bf16_t*)0x4000,
         *const Z = (bf16_t*)0x5000;
  float *const S = (float*)0x6000, *const B = (float*)0x7000;
  auto cargs = [&](const ConvGeom& g, int split) { return spk_conv_args(g, X, Wt, Y, R, S, B, 1, DT_F16, split); };
  {  // 1x1, stride 2, split weights; the same conv for conv_pw.hip, then a second source and a chained conv on it
    const ConvArgs a = cargs(spk_conv_geom(2, 7, 7, 64, 128, 1, 2, 0), 1);
    EXPECT(a.Ho == 4 && a.Wo == 4 && a.M == 32 && a.K == 64 && a.x_bytes == 12544 && a.w_bytes == 32768 && spk_below_2gib(a));
    ConvArgs e = zeroed<ConvArgs>();
    e.x = X; e.w = Wt; e.y = Y; e.res = R; e.scale = S; e.bias = B;
    e.N = 2; e.H = 7; e.W = 7; e.Cin = 64; e.Ho = 4; e.Wo = 4; e.Cout = 128; e.kh = e.kw = 1; e.stride = 2; e.M = 32; e.K = 64;
    e.relu = 1; e.dt = DT_F16; e.splitw = 1; e.cfg = e.dma = e.cls_ph = e.cls_pw = -1; e.x_bytes = 12544; e.w_bytes = 32768;
    EXPECT(same_bytes(a, e));
    PwConvArgs q = pw_args(a, Wt + 8), f = zeroed<PwConvArgs>();
    f.x = X; f.wp = Wt + 8; f.y = Y; f.res = R; f.scale = S; f.shift = B;
    f.N = 2; f.H = 7; f.W = 7; f.Ho = 4; f.Wo = 4; f.stride = 2; f.Cin = 64; f.Cout = 128; f.M = 32; f.relu = 1; f.dt = DT_F16;
    f.nb = 2; f.x_bytes = 12544; f.y_bytes = 8192;
    EXPECT(q.nb == 2 && q.y_bytes == 8192 && same_bytes(q, f));
    spk_pw_set_second(q, R, 64, 13, 13, 4);
    f.x2 = R; f.Cin2 = 64; f.H2 = 13; f.W2 = 13; f.stride2 = 4; f.x2_bytes = 43264;   // 2 x 13 x 13 x 64 x 2
    EXPECT(q.x2_bytes == 43264 && same_bytes(q, f));
    spk_pw_set_chain(q, Wt + 16, Z, S + 128, B + 128, 32, 1);
    f.wpz = Wt + 16; f.z = Z; f.scalez = S + 128; f.shiftz = B + 128; f.Coutz = 32; f.reluz = 1; f.z_bytes = 2048;
    EXPECT(q.z_bytes == 2048 && same_bytes(q, f) && spk_below_2gib(q));
  }
  {  // the 7x7 stem: four stored channels, an even row pitch, K padded to 256
    const ConvGeom g = spk_stem_geom(1, 9, 9);
    const ConvArgs a = cargs(g, 0);
    EXPECT(g.W == 10 && a.W == 10 && a.H == 9 && a.Cin == 4 && a.Cout == 64 && a.Ho == 5 && a.Wo == 5 && a.M == 25 && a.K == 256);
    EXPECT(a.kh == 7 && a.kw == 7 && a.stride == 2 && a.pad == 3 && !a.cin_s && !a.cout_s && a.x_bytes == 720 && a.w_bytes == 32768);
    EXPECT(cargs(g, 1).w_bytes == 65536 && spk_stem_geom(1, 9, 10).W == 10 && spk_stem_geom(1, 9, 10).Wo == 5);
  }
  {  // EfficientNet 1x1 on unpadded tensors: 24 -> 40 stored channels, a 64 x 64 GEMM
    const ConvArgs a = cargs({1, 5, 5, 24, 5, 5, 40, 64, 64, 64, 1, 1, 0}, 0);
    EXPECT(a.Cin == 64 && a.Cout == 64 && a.cin_s == 24 && a.cout_s == 40 && a.x_bytes == 1200 && a.w_bytes == 8192 && a.M == 25);
  }
  {  // 3x3 through c3_args, hi + lo weight images
    const ConvArgs a = cargs(spk_conv_geom(1, 6, 6, 64, 64, 3, 1, 1), 1);
    C3Args q = c3_args(a, Wt + 8, 2), f = zeroed<C3Args>();
    EXPECT(a.Ho == 6 && a.Wo == 6 && a.K == 576 && q.M == 36 && q.x_bytes == 4608 && q.y_bytes == 4608 && q.wp_bytes == 147456);
    f.x = X; f.wp = Wt + 8; f.y = Y; f.scale = S; f.shift = B; f.res = R;
    f.N = 1; f.H = 6; f.W = 6; f.Cin = 64; f.Cout = 64; f.M = 36; f.relu = 1; f.dt = DT_F16; f.nb = 2;
    f.x_bytes = f.y_bytes = 4608; f.wp_bytes = 147456;
    EXPECT(same_bytes(q, f) && spk_below_2gib(q));
  }
  {  // a whole bottleneck, then the chained conv behind it
    BneckArgs a = spk_bneck_args(X, Y, Wt, Wt + 8, Wt + 16, S, B, S + 1, B + 1, S + 2, B + 2, 2, 14, 14, 64), e = zeroed<BneckArgs>();
    e.x = X; e.y = Y; e.w1 = Wt; e.w2 = Wt + 8; e.w3 = Wt + 16; e.s1 = S; e.b1 = B; e.s2 = S + 1; e.b2 = B + 1; e.s3 = S + 2; e.b3 = B + 2;
    e.N = 2; e.H = 14; e.W = 14; e.C4 = 256; e.CM = 64; e.x_bytes = 200704;
    EXPECT(a.C4 == 256 && a.x_bytes == 200704 && same_bytes(a, e));
    spk_bneck_set_chain(a, Wt + 24, Z, S + 3, B + 3, 128);
    e.wz = Wt + 24; e.z = Z; e.sz = S + 3; e.bz = B + 3; e.Coutz = 128; e.z_bytes = 100352;
    EXPECT(a.z_bytes == 100352 && same_bytes(a, e) && spk_below_2gib(a));
  }
  {  // the 2 GiB limit of the 32-bit buffer offsets: one element (2 bytes) below it passes, at it no more; a count past
     // 32 bits does not wrap to a small extent
    EXPECT(spk_extent(0x7ffffffeull) == 0x7ffffffeu && spk_extent(0x100000010ull) == 0xffffffffu);
    ConvGeom g = {1, 1, (1 << 30) - 1, 1, 1, 1, 64, 64, 64, 64, 1, 1, 0};   // x: 2^30 - 1 one-channel pixels, then 2^30
    EXPECT(cargs(g, 0).x_bytes == 0x7ffffffeu && spk_below_2gib(cargs(g, 0)));
    g.W = 1 << 30;
    EXPECT(cargs(g, 0).x_bytes == 0x80000000u && !spk_below_2gib(cargs(g, 0)));
    g = {1, 1, 1, 64, 1, (1 << 24) - 1, 64, 64, 64, 64, 1, 1, 0};           // y: 2^24 - 1 pixels of 64 channels, then 2^24
    EXPECT(spk_below_2gib(cargs(g, 0)) && spk_below_2gib(pw_args(cargs(g, 0), Wt)) && spk_below_2gib(c3_args(cargs(g, 0), Wt, 1)));
    g.Wo = 1 << 24;
    EXPECT(!spk_below_2gib(cargs(g, 0)) && !spk_below_2gib(pw_args(cargs(g, 0), Wt)) && !spk_below_2gib(c3_args(cargs(g, 0), Wt, 1)));
    EXPECT(spk_below_2gib(spk_bneck_args(X, Y, Wt, Wt, Wt, S, B, S, B, S, B, 1, 1, (1 << 22) - 1, 64)));
    EXPECT(!spk_below_2gib(spk_bneck_args(X, Y, Wt, Wt, Wt, S, B, S, B, S, B, 1, 1, 1 << 22, 64)));
    EXPECT(!spk_below_2gib(spk_bneck_args(X, Y, Wt, Wt, Wt, S, B, S, B, S, B, 64, 1 << 10, 1 << 10, 64)));   // 2^35 bytes
  }
}

int main(int argc, char** argv) {
  int ndev = 0;
  const bool gpu = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
  printf("asan_driver: %d GPU(s)\n", gpu ? ndev : 0);
  graph_checks();
  cursor_checks();
  descriptor_checks();

  // ---- argument errors ----
  spk_model* m = nullptr;
  EXPECT(spk_model_create(nullptr, 0, 3, 10, 0, &m) != SPK_OK);
  EXPECT(strlen(spk_last_error()) > 0);
  EXPECT(spk_model_num_params(nullptr) == 0);
  spk_model_destroy(nullptr);
  {   // the checkpoint entry points look at their arguments before anything else
    float f[4] = {0};
    int64_t step = 0;
    double mu = 0;
    uint64_t steps = 0, seed = 0;
    EXPECT(spk_model_optim_state_read(nullptr, "head.0.weight", 0, f, 4) == SPK_ERR_ARG);
    EXPECT(spk_model_optim_state_load(nullptr, "head.0.weight", 1, f, 4) == SPK_ERR_ARG);
    EXPECT(spk_model_param_counters_get(nullptr, "head.0.weight", &step, &mu) == SPK_ERR_ARG);
    EXPECT(spk_model_param_counters_set(nullptr, "head.0.weight", 1, 1.0) == SPK_ERR_ARG);
    EXPECT(spk_model_train_counters_get(nullptr, &steps, &seed) == SPK_ERR_ARG);
    EXPECT(spk_model_train_counters_set(nullptr, 1, 2) == SPK_ERR_ARG);
    // ... and so do the loss's: a null handle, a smoothing value outside [0, 1] (NaN included), null operands
    int64_t counts[4] = {0};
    int64_t labels[1] = {0};
    EXPECT(spk_model_set_loss(nullptr, f, 0.1f) == SPK_ERR_ARG);
    EXPECT(spk_model_class_counts_read(nullptr, counts, 1) == SPK_ERR_ARG);
    EXPECT(spk_op_cross_entropy_ex(f, labels, 1, 4, nullptr, 1.5f, f, nullptr, nullptr, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_cross_entropy_ex(f, labels, 1, 4, nullptr, NAN, f, nullptr, nullptr, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_cross_entropy_ex(f, nullptr, 1, 4, f, 0.1f, f, nullptr, nullptr, nullptr) == SPK_ERR_ARG);
    // ... and the Mixup / CutMix entry points: lam, the box, the shift, the coefficients, overlapping buffers
    unsigned char img_a[2 * 4 * 4 * 3] = {0}, img_b[2 * 4 * 4 * 3] = {0};
    EXPECT(spk_op_cross_entropy_pair(f, labels, labels, 1.5f, 1, 4, nullptr, 0.f, f, nullptr, nullptr, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_cross_entropy_pair(f, labels, nullptr, NAN, 1, 4, nullptr, 0.f, f, nullptr, nullptr, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_cross_entropy_pair(f, nullptr, labels, 0.5f, 1, 4, nullptr, 0.f, f, nullptr, nullptr, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_train_forward_backward_pair(nullptr, f, 1, 4, 4, SPK_LAYOUT_NCHW, SPK_DTYPE_F32, labels, labels, 0.5f, f, nullptr) == SPK_ERR_ARG);
    // ... the distillation criterion: alpha, the temperature, statistics without a teacher
    EXPECT(spk_op_cross_entropy_distill(f, labels, nullptr, 1.f, f, 1.5f, 2.f, 1, 4, nullptr, 0.f, f, nullptr, f, nullptr, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_cross_entropy_distill(f, labels, nullptr, 1.f, f, NAN, 2.f, 1, 4, nullptr, 0.f, f, nullptr, f, nullptr, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_cross_entropy_distill(f, labels, nullptr, 1.f, f, 0.5f, 0.f, 1, 4, nullptr, 0.f, f, nullptr, f, nullptr, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_cross_entropy_distill(f, labels, nullptr, 1.f, f, 0.5f, INFINITY, 1, 4, nullptr, 0.f, f, nullptr, f, nullptr, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_cross_entropy_distill(f, labels, nullptr, 1.f, nullptr, 0.5f, 2.f, 1, 4, nullptr, 0.f, f, nullptr, f, nullptr, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_train_forward_backward_distill(nullptr, f, 1, 4, 4, SPK_LAYOUT_NCHW, SPK_DTYPE_F32, labels, nullptr, 1.f, f, 0.5f, 2.f, f, f, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_mix_batch(img_a, img_b, 2, 4, 4, 3, SPK_LAYOUT_NHWC, SPK_DTYPE_U8, 2, 0.5f, 0.5f, 0, 0, 4, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_mix_batch(img_a, img_b, 2, 4, 4, 3, SPK_LAYOUT_NHWC, SPK_DTYPE_U8, 1, 0.5f, 0.5f, 0, 0, 5, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_mix_batch(img_a, img_b, 2, 4, 4, 3, SPK_LAYOUT_NHWC, SPK_DTYPE_U8, 1, NAN, 0.5f, 0, 0, 4, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_mix_batch(img_a, img_a + 8, 2, 4, 4, 3, SPK_LAYOUT_NHWC, SPK_DTYPE_U8, 1, 0.5f, 0.5f, 0, 0, 4, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_mix_batch(img_a, img_b, 2, 4, 4, 3, SPK_LAYOUT_NCHW, SPK_DTYPE_U8, 1, 0.5f, 0.5f, 0, 0, 4, 4, nullptr) == SPK_ERR_ARG);
    // ... and the moving average's: a null handle, the weight, null / overlapping / misaligned buffers, the count
    float ea[8] = {0}, eb[8] = {0};
    int en = 0, sw = 0;
    EXPECT(spk_model_ema_enable(nullptr, 1) == SPK_ERR_ARG);
    EXPECT(spk_model_ema_update(nullptr, 0.1f) == SPK_ERR_ARG);
    EXPECT(spk_model_ema_swap(nullptr) == SPK_ERR_ARG);
    EXPECT(spk_model_ema_read(nullptr, "head.0.weight", f, 4) == SPK_ERR_ARG);
    EXPECT(spk_model_ema_load(nullptr, "head.0.weight", f, 4) == SPK_ERR_ARG);
    EXPECT(spk_model_ema_state(nullptr, &en, &sw) == SPK_ERR_ARG);
    EXPECT(spk_op_ema_lerp(ea, eb, 8, 0.f, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_ema_lerp(ea, eb, 8, 1.f, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_ema_lerp(ea, eb, 8, NAN, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_ema_lerp(ea, eb, 0, 0.1f, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_ema_lerp(ea, nullptr, 8, 0.1f, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_ema_lerp(ea, ea + 4, 8, 0.1f, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_swap_f32(ea, ea + 7, 8, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_swap_f32(ea, (float*)((char*)eb + 2), 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_op_swap_f32(nullptr, eb, 8, nullptr) == SPK_ERR_ARG);
    // ... and test-time augmentation's: null pointers, the sizes, the channel count, the batch kind, the number of views, a
    // code outside 0..7, a transposing code on a rectangle, overlapping buffers; the mean's k, numel and overlap
    unsigned char sq_a[2 * 4 * 4 * 3] = {0}, sq_b[8 * 2 * 4 * 4 * 3] = {0};
    const int32_t flips[4] = {0, 1, 2, 3}, nine[9] = {0, 1, 2, 3, 4, 5, 6, 7, 0}, wrong[2] = {0, 8}, neg[1] = {-1}, tp[2] = {0, 5};
    const int U8L = SPK_LAYOUT_NHWC, U8 = SPK_DTYPE_U8;
    EXPECT(spk_tta_views(nullptr, sq_b, 2, 4, 4, 3, U8L, U8, flips, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_views(sq_a, nullptr, 2, 4, 4, 3, U8L, U8, flips, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_views(sq_a, sq_b, 2, 4, 4, 3, U8L, U8, nullptr, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_views(sq_a, sq_b, 0, 4, 4, 3, U8L, U8, flips, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_views(sq_a, sq_b, 2, 0, 4, 3, U8L, U8, flips, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_views(sq_a, sq_b, 2, 4, -1, 3, U8L, U8, flips, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_views(sq_a, sq_b, 2, 4, 4, 2, U8L, U8, flips, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_views(sq_a, sq_b, 2, 4, 4, 3, SPK_LAYOUT_NCHW, U8, flips, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_views(sq_a, sq_b, 2, 4, 4, 3, U8L, SPK_DTYPE_F32, flips, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_views(sq_a, sq_b, 2, 4, 4, 3, U8L, U8, flips, 0, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_views(sq_a, sq_b, 2, 4, 4, 3, U8L, U8, nine, 9, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_views(sq_a, sq_b, 2, 4, 4, 3, U8L, U8, wrong, 2, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_views(sq_a, sq_b, 2, 4, 4, 3, U8L, U8, neg, 1, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_views(sq_a, sq_b, 2, 4, 2, 3, U8L, U8, tp, 2, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_views(sq_b + 96, sq_b, 2, 4, 4, 3, U8L, U8, flips, 4, nullptr) == SPK_ERR_ARG);   // in inside out
    EXPECT(spk_tta_views(sq_b, sq_b + 47, 1, 4, 4, 3, U8L, U8, flips, 4, nullptr) == SPK_ERR_ARG);   // out begins in in's last byte
    EXPECT(strstr(spk_last_error(), "spk_tta_views") != nullptr);
    float pm[8 * 4] = {0}, om[4] = {0};
    EXPECT(spk_tta_mean(nullptr, om, 8, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_mean(pm, nullptr, 8, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_mean(pm, om, 0, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_mean(pm, om, 9, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_mean(pm, om, 8, 0, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_mean(pm, pm + 31, 8, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(spk_tta_mean(pm + 3, pm, 7, 4, nullptr) == SPK_ERR_ARG);
    EXPECT(strstr(spk_last_error(), "spk_tta_mean") != nullptr);
  }

  // ---- a small bottleneck graph: stem, pool, 1x1 / 3x3 / 1x1 + shortcut, pool, head ----
  std::vector<spk_layer_desc> g;
  g.push_back(conv("base.0", "base.1", 3, 64, 7, 2, 3, 0, 1, -1, 1, 0));
  { spk_layer_desc d; memset(&d, 0, sizeof d); d.kind = SPK_OP_MAXPOOL; d.cin = d.cout = 64; d.k = 3; d.stride = 2; d.pad = 1;
    d.src = 1; d.dst = 2; d.res = -1; d.child = 3; snprintf(d.name, sizeof d.name, "base.3"); g.push_back(d); }
  g.push_back(conv("base.4.0.conv1", "base.4.0.bn1", 64, 64, 1, 1, 0, 2, 3, -1, 1, 4));
  g.push_back(conv("base.4.0.conv2", "base.4.0.bn2", 64, 64, 3, 1, 1, 3, 4, -1, 1, 4));
  g.push_back(conv("base.4.0.downsample.0", "base.4.0.downsample.1", 64, 256, 1, 1, 0, 2, 5, -1, 0, 4));
  g.push_back(conv("base.4.0.conv3", "base.4.0.bn3", 64, 256, 1, 1, 0, 4, 6, 5, 1, 4));
  { spk_layer_desc d; memset(&d, 0, sizeof d); d.kind = SPK_OP_GAVGPOOL; d.cin = d.cout = 256; d.src = 6; d.dst = 7; d.res = -1;
    d.child = 8; snprintf(d.name, sizeof d.name, "base.8"); g.push_back(d); }
  { spk_layer_desc d; memset(&d, 0, sizeof d); d.kind = SPK_OP_LINEAR; d.cin = 256; d.cout = 10; d.src = 7; d.dst = 8; d.res = -1;
    d.child = -1; snprintf(d.name, sizeof d.name, "head.0"); g.push_back(d); }
  const int rc = spk_model_create(g.data(), (int)g.size(), 3, 10, 0, &m);
  if (!gpu) {
    EXPECT(rc != SPK_OK && m == nullptr);          // no device: every allocation fails, nothing may leak or dangle
    EXPECT(strlen(spk_last_error()) > 0);
  } else {
    EXPECT(rc == SPK_OK && m != nullptr);
  }
  if (m) {
    const int np = spk_model_num_params(m);
    EXPECT(np > 10);
    for (int i = -1; i <= np; ++i) {
      char key[8];                                  // deliberately short: the name must be truncated, not overrun
      int64_t shape[4];
      int ndim = 0, dtype = 0;
      const int r = spk_model_param_info(m, i, key, (int)sizeof key, shape, &ndim, &dtype);
      EXPECT((r == SPK_OK) == (i >= 0 && i < np));
      if (r == SPK_OK) EXPECT(strlen(key) < sizeof key);
    }
    std::vector<float> w(64 * 3 * 7 * 7, 0.5f);
    EXPECT(spk_model_load_param(m, "no.such.key", w.data(), (int64_t)w.size()) == SPK_ERR_KEY);
    EXPECT(spk_model_load_param(m, "base.0.weight", w.data(), 7) != SPK_OK);           // wrong element count
    EXPECT(spk_model_load_param(m, "base.0.weight", w.data(), (int64_t)w.size()) == SPK_OK);
    EXPECT(spk_model_set_requires_grad(m, "no.such.key", 1) == SPK_ERR_KEY);
    EXPECT(spk_model_set_param_group(m, "base.0.weight", 2) == SPK_OK);
    std::vector<float> mom(w.size(), 1.f);
    EXPECT(spk_model_optim_state_read(m, "no.such.key", 0, mom.data(), (int64_t)mom.size()) == SPK_ERR_KEY);
    EXPECT(spk_model_optim_state_read(m, "base.0.weight", 0, mom.data(), 7) == SPK_ERR_ARG);
    EXPECT(spk_model_optim_state_read(m, "base.0.weight", 0, mom.data(), (int64_t)mom.size()) == SPK_OK && mom[0] == 0.f);
    spk_model_destroy(m);
  }

  // ---- the tuner table: the nearest-batch rule, the shipped seed and the appended lines, then a file with one valid
  // line per tag, a value out of range per range-checked tag, truncated lines, garbage, a comment, over-long lines ----
  const std::string path = std::string(getenv("TMPDIR") ? getenv("TMPDIR") : "/tmp") + "/spk_asan_tune_cache.txt";
  // the shipped seed: argv[1], else where it lies in the source tree as seen from this program (csrc/build/asan/)
  std::string seed = argc > 1 ? argv[1] : std::string(argv[0]);
  if (argc <= 1) seed = seed.substr(0, seed.find_last_of('/') + 1) + "../../../sykepic_hip/tune_seed_gfx950.txt";
  tuner_table_checks(path + ".rt", seed);
  std::string fixture;
  if (FILE* f = fopen(path.c_str(), "w")) {
    fprintf(f, "conv 0 1 1 256 14 14 256 256 3 1 16 0 0 4 3\n");
    fprintf(f, "pw1x1 2 14 14 256 1024 1 1 1 256 7\n");
    fprintf(f, "pw2 1 14 14 256 28 28 512 1024 1 2 256 5\n");
    fprintf(f, "c3 1 14 14 256 256 256 2\n");
    fprintf(f, "chain 14 14 256 0 256 64 0\n");
    fprintf(f, "bneck 14 256 8 1\n");
    fprintf(f, "wgrad 6272 256 256 3 1 0 13 128128 1\n");
    fprintf(f, "d3 56 56 0 128 -1\n");
    fprintf(f, "d3 56 56 1 128 %d\n", kD3NumCfgs);                 // (out of range)
    fprintf(f, "pw1x1 2 14 14 256 2048 1 1 1 256 99999\n");       // values out of range: ignored
    fprintf(f, "pw1x1 2 14 14 256 2048 1 1 1 256 -2\n");
    fprintf(f, "pw2 1 14 14 256 28 28 512 2048 1 2 256 %d\n", kPwNumCfgs);
    fprintf(f, "pw2 1 14 14 256 28 28 512 2048 1 2 256 -1\n");
    fprintf(f, "c3 1 14 14 256 512 256 %d\n", kC3NumCfgs);
    fprintf(f, "chain 14 14 256 0 512 64 2\n");
    fprintf(f, "bneck 28 128 8 3\n");
    fprintf(f, "c3 1 14 14\n");                                    // truncated
    fprintf(f, "bneck 28 128 8\n");
    fprintf(f, "bneck 28 128 8 1 1\n");                            // one field too many
    fprintf(f, "chain 14 14 256 0 512 64 1x\n");                   // not an integer
    fprintf(f, "wgrad 6272 256 512 3 1 0 13 128128 99999999999\n");
    fprintf(f, "# bneck 28 128 8 2\n#bneck 28 128 8 2\n");         // comments
    fprintf(f, "conv x y z\n\n,,,,\nbneck\nbneckx 28 128 8 2\n");
    for (int i = 0; i < 3000; ++i) fputc('9', f);                  // longer than the parser's line buffer: dropped whole,
    fprintf(f, "\n");
    for (int i = 0; i < spk_tune_detail::kLineBuf - 1; ++i) fputc('9', f);
    fprintf(f, "bneck 28 128 8 2\n");                              // even where its tail would read as an entry
    fprintf(f, "wgrad 1 2 3\n");
    fprintf(f, "c3 2 7 7 512 512 128 13");                         // the entry after it; no newline at the end of the file
    fclose(f);
    for (const TuneLine& l : read_tune_lines(path)) fixture += l.text;
  }
  use_cache(path.c_str());
  int dma = -1;
  EXPECT(look(TUNE_CONV, {0, 1, 1, 256, 14, 14, 256, 256, 3, 1, 16, 0, 0}, &dma) == 4 && dma == 3);
  EXPECT(look(TUNE_PW1, {2, 14, 14, 256, 1024, 1, 1, 1, 256}) == 7);
  EXPECT(look(TUNE_PW2, {1, 14, 14, 256, 28, 28, 512, 1024, 1, 2, 256}) == 5);
  EXPECT(look(TUNE_C3, {1, 14, 14, 256, 256, 256}) == 2);
  EXPECT(look(TUNE_CHAIN, {14, 14, 256, 0, 256, 64}) == 0);
  EXPECT(look(TUNE_BNECK, {14, 256, 8}) == 1);
  EXPECT(look(TUNE_WGRAD, {6272, 256, 256, 3, 1, 0, 13, 128128}) == 1);
  EXPECT(look(TUNE_C3, {2, 7, 7, 512, 512, 128}) == 13);
  EXPECT(look(TUNE_D3, {56, 56, 0, 128}) == -1);
  EXPECT(look(TUNE_D3, {56, 56, 1, 128}) == -1000);
  EXPECT(look(TUNE_PW1, {2, 14, 14, 256, 2048, 1, 1, 1, 256}) == -1000);
  EXPECT(look(TUNE_PW2, {1, 14, 14, 256, 28, 28, 512, 2048, 1, 2, 256}) == -1000);
  EXPECT(look(TUNE_C3, {1, 14, 14, 256, 512, 256}) == -1000);
  EXPECT(look(TUNE_CHAIN, {14, 14, 256, 0, 512, 64}) == -1000);
  EXPECT(look(TUNE_BNECK, {28, 128, 8}) == -1000);
  EXPECT(look(TUNE_WGRAD, {6272, 256, 512, 3, 1, 0, 13, 128128}) == -1000);
  EXPECT(spk_tune_detail::table().map.size() == 9);
  setenv("SPK_AUTOTUNE", "0", 1);
  // a problem that is NOT in the file (channels 128), on real buffers when there is a GPU
  const int n = 1, h = 8, wd = 8, cin = 128, cout = 128, M = n * h * wd;
  bf16_t *x = nullptr, *y = nullptr, *wp = nullptr;
  float* sb = nullptr;
  if (gpu) {
    EXPECT(hipMalloc(&x, (size_t)M * cin * 2) == hipSuccess && hipMalloc(&y, (size_t)M * 256 * 2) == hipSuccess);
    EXPECT(hipMalloc(&wp, (size_t)256 * 9 * cin * 4) == hipSuccess && hipMalloc(&sb, (size_t)2 * 256 * 4) == hipSuccess);
    (void)hipMemset(x, 0, (size_t)M * cin * 2);
    (void)hipMemset(wp, 0, (size_t)256 * 9 * cin * 4);
    (void)hipMemset(sb, 0, (size_t)2 * 256 * 4);
  }
  const float* sh = sb ? sb + cout : nullptr;
  const ConvArgs a = spk_conv_args(spk_conv_geom(n, h, wd, cin, cout, 1, 1, 0), x, wp, y, nullptr, sb, sh, 1, DT_F16, 1);
  const PwConvArgs q = pw_args(a, wp);
  const int r1 = spk_conv1x1_launch(a, q, nullptr);               // not tuned, no tuning: the implicit GEMM, nothing stored
  EXPECT(gpu ? r1 == 0 : r1 != 0);
  const C3Args c = c3_args(spk_conv_args(spk_conv_geom(n, h, wd, cin, 256, 3, 1, 1), x, nullptr, y, nullptr, sb,
                                         sb ? sb + 256 : nullptr, 1, DT_F16, 0), wp, 1);
  const int r3 = spk_conv3x3_launch(c, nullptr);                  // not tuned, no tuning: the first configuration that launches
  EXPECT(gpu ? r3 == 0 : r3 != 0);
  if (gpu) {
    (void)hipDeviceSynchronize();
    (void)hipFree(x); (void)hipFree(y); (void)hipFree(wp); (void)hipFree(sb);
  }
  std::string after;                                              // without tuning nothing is appended
  for (const TuneLine& l : read_tune_lines(path)) after += l.text;
  EXPECT(!fixture.empty() && after == fixture);
  remove(path.c_str());
  printf("asan_driver: %s\n", g_fail ? "FAILED" : "ok");
  return g_fail ? 1 : 0;
}
