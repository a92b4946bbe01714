// libsykepic_hip.so — the activation plan and the eval-mode layer executor (host side).  The handle itself, its graph
// analysis, parameter table and packed weights: model_graph.hip, model_params.hip, model_pack.hip.
// Public contract and the reference lines each entry point replaces:
// include/sykepic_hip.h.
#include "model.h"
#include "conv_args.h"
#include "tune_pair.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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
        if (o.h < 1 || o.w < 1) { m->cap_n = 0; return spk_fail(SPK_ERR_ARG, "image too small for the network"); }
        if (L.d.kind != SPK_OP_MAXPOOL && L.d.src != 0 && (in.c_log > 0 ? in.c_log : in.c) != L.d.cin) {
          m->cap_n = 0;
          return spk_fail(SPK_ERR_ARG, std::string("channel mismatch at ") + L.d.name);
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
    spk_free_acts(m);
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

int spk_micro_batch(spk_model* m, int n) {
  static const int env = getenv("SPK_MICRO_BATCH") ? atoi(getenv("SPK_MICRO_BATCH")) : 0;
  int mb = std::min(n, m->mb_limit);
  if (env > 0) mb = std::min(mb, env);
  return std::max(mb, 1);
}

// ---------------------------------------------------------------------------
// eval-mode forward of images [i0, i0+nb) into logits rows [i0, i0+nb)
// ---------------------------------------------------------------------------
// The record (EvalCarry::ran, model.h): written by the forward only - a tuner's timing run or a read-back's recompute
// passes `allow` without EVAL_FORWARD and neither consults nor changes it.
static void note(spk_model* m, const EvalCursor& c, unsigned allow, int li, unsigned form, bool wrote, int by = -1) {
  if (allow & EVAL_FORWARD) m->carry[c.half].ran[li] = {(uint8_t)form, wrote, by};
}
static int index_of(const spk_model* m, const Layer& L) { return (int)(&L - m->layers.data()); }

void spk_eval_begin(spk_model* m, int nb) {
  m->last_eval_nb = nb;
  for (EvalCarry& k : m->carry) {
    k.shadow_t = -1;
    k.ran.assign(m->layers.size(), EvalRan());
  }
}

// eval: does the stem kernel also compute the max-pool that follows it?  (not with the rounding-remainder tensors of
// the precise-residual mode, whose pool works on value + remainder)
static bool stem_pool_fused(const spk_model* m, const Layer& L, unsigned allow) {
  return (allow & FUSE_POOL) && L.fuse_pool >= 0 && m->fuse_stem_pool && !m->precise_res;
}

// eval: does the block-closing conv L absorb its shortcut conv in this forward?
static bool dual_active(const spk_model* m, const Layer& L, unsigned allow) {
  return (allow & FUSE_DUAL) && m->fuse_ds && L.dual_src >= 0 && L.dual_ok && m->infer_dt == DT_F16 && !m->precise_res;
}

// eval: may the block whose first conv is L run as the whole-bottleneck kernel (single fp16 weight images, a shape the kernel
// has an instantiation for)?
static bool bneck_possible(const spk_model* m, const Layer& L, unsigned allow) {
  if (!(allow & FUSE_BNECK) || !m->bneck || L.bn_c2 < 0 || m->infer_dt != DT_F16 || m->precise_res) return false;
  if (layer_split(m, L) || layer_split(m, m->layers[L.bn_c2]) || layer_split(m, m->layers[L.bn_c3])) return false;
  const TDim& in = m->tdims[L.d.src];
  return in.h == in.w && ((L.d.cout == 256 && in.h == 14) || (L.d.cout == 128 && in.h == 28)) && in.c == L.d.cin;
}

// eval: may conv2 (L) of an identity bottleneck also compute the block's conv3 + shortcut (conv_btail_kernel: the stage whose
// trunk is too wide for the whole-block kernel)?
static bool btail_possible(const spk_model* m, const Layer& L, unsigned allow) {
  if (!(allow & FUSE_BTAIL) || !m->btail || L.bn_head < 0 || L.d.k != 3 || m->infer_dt != DT_F16 || m->precise_res) return false;
  const Layer& H = m->layers[L.bn_head];
  const Layer& L3 = m->layers[H.bn_c3];
  if (layer_split(m, L) || layer_split(m, L3) || L3.dual_src >= 0) return false;
  const TDim& in = m->tdims[L.d.src];
  return in.h == in.w && in.h == 56 && L.d.cout == 64 && in.c == 64;
}

// eval: may the block-closing conv L also compute the conv that reads its output (single fp16 weight images only)?
static bool chain_possible(const spk_model* m, const Layer& L, unsigned allow) {
  if (!(allow & FUSE_CHAIN) || !m->chain || L.chain_next < 0 || m->infer_dt != DT_F16 || m->precise_res) return false;
  const Layer& Q = m->layers[L.chain_next];
  if (layer_split(m, L) || layer_split(m, Q)) return false;
  if (bneck_possible(m, Q, allow)) return false;   // (that conv is the head of a block the whole-bottleneck kernel computes)
  if (L.dual_src >= 0 && !dual_active(m, L, allow)) return false;   // (a shortcut conv that runs on its own: plain res operand)
  return true;
}

static int run_conv_eval(spk_model* m, Layer& L, const EvalCursor& c, unsigned allow);

// ---- paired tuning (tune_table.h): what the executor contributes ----
// SpkTwin::rebase: a pointer to the first image of the half in work inside activation tensor t becomes the other half's
// first image of t; pointers outside the activation tensors (weights, folded BatchNorm) stay; anything else has no twin
bool spk_twin_rebase(void* user, const void** p) {
  const EvalTwin& tw = *(const EvalTwin*)user;
  const spk_model* m = tw.m;
  const char* a = (const char*)m->arena;
  const char* q = (const char*)*p;
  if (!a || q < a || q >= a + m->arena_bytes) return true;
  const size_t o = (size_t)(q - a);
  if (o >= m->se_off) return false;   // scratch behind the tensors: not a per-image slice of a tensor
  const int t = (int)(std::upper_bound(m->toff.begin(), m->toff.end(), o) - m->toff.begin()) - 1;
  if (t < 0 || t >= m->n_tensors) return false;
  const TDim& d = m->tdims[t];
  const size_t img = (size_t)d.h * d.w * d.c * (d.bf16 ? 2 : 4);
  if (o != m->toff[t] + (size_t)tw.img0 * img || tw.twin_img0 + tw.twin_n > m->cap_n) return false;
  *p = a + m->toff[t] + (size_t)tw.twin_img0 * img;
  return true;
}
// the twin context of the calling thread as the executor set it, or null; and the other half's cursor (PAIRS: its stream is idle)
static const EvalTwin* eval_twin() { return spk_twin().rebase == spk_twin_rebase ? (const EvalTwin*)spk_twin().user : nullptr; }
static EvalCursor twin_cursor(const EvalCursor& c) {
  const EvalTwin* tw = eval_twin();
  return tw ? EvalCursor{1 - c.half, tw->twin_img0, tw->twin_n, spk_twin().stream} : c;
}

// the unfused forms the choosers below time, as whole layers (and with them the other kernels' own tuning)
static int two_kernels(spk_model* m, Layer& L, const EvalCursor& c, unsigned allow) {
  allow &= ~(FUSE_CHAIN | EVAL_FORWARD);
  SPK_TRY(run_conv_eval(m, L, c, allow));
  return run_conv_eval(m, m->layers[L.chain_next], c, allow);
}
static int three_launches(spk_model* m, Layer& L, const EvalCursor& c, unsigned allow) {
  allow &= ~(FUSE_BNECK | FUSE_BTAIL | EVAL_FORWARD);
  SPK_TRY(run_conv_eval(m, L, c, allow));
  SPK_TRY(run_conv_eval(m, m->layers[L.bn_c2], c, allow));
  return run_conv_eval(m, m->layers[L.bn_c3], c, allow);
}

// chained kernel (1) or two kernels (0)?  Timed once per problem (both give the same bits), "chain" entries of the tuner
// table; without tuning the chained kernel, not remembered
static int chain_choice(spk_model* m, Layer& L, const PwConvArgs& q, const EvalCursor& c, unsigned allow) {
  if (m->chain >= 2) return 1;
  const int key[] = {q.H, q.W, q.Cin, q.x2 ? q.Cin2 : 0, q.Coutz, q.N};
  int choice = 1;
  const TuneTag tag = spk_tune_tag(TUNE_CHAIN);
  if (spk_tune_find(tag, key, &choice) || !spk_autotune_on()) return choice;
  SpkLaunchTimer timer;
  if (!timer.ok) return choice;
  const SpkPair<PwConvArgs> pq(q);
  const EvalCursor cs[2] = {c, twin_cursor(c)};
  auto two = [&](int i, hipStream_t) { return two_kernels(m, L, cs[i], allow); };   // (each on its cursor's stream)
  auto one = [&](int i, hipStream_t st) { return spk_pw_chain_launch(pq[i], st); };
  float t_two = 0.f, t_one = 0.f;
  const bool ok = two(0, c.stream) == SPK_OK && one(0, c.stream) == 0 &&   // warm-up (and the other kernels' own tuning)
                  timer.time(c.stream, 3, pq.ok, two, &t_two) && timer.time(c.stream, 3, pq.ok, one, &t_one);
  choice = ok && t_one < t_two ? 1 : 0;
  if (spk_tune_log())
    fprintf(stderr, "[spk tune chain] N%d %dx%d C%d+%d->256->%d: two kernels %.1f us, chained %.1f us\n", q.N, q.H, q.W, q.Cin,
            q.x2 ? q.Cin2 : 0, q.Coutz, t_two * 1000.f / 3.f, t_one * 1000.f / 3.f);
  spk_tune_store(tag, key, &choice, true);
  return choice;
}

// the conv that L's kernel can compute from its own output tile; null: shapes the chained kernels do not cover
static const Layer* chain_target(spk_model* m, const Layer& L) {
  const Layer& Q = m->layers[L.chain_next];
  const TDim& zo = m->tdims[Q.d.dst];
  const TDim& o = m->tdims[L.d.dst];
  return zo.h != o.h || zo.w != o.w || zo.c != Q.d.cout || Q.d.cin != L.d.cout ? nullptr : &Q;
}

// fills the chained conv's fields of q; false: shapes the kernel does not cover
static bool chain_args(spk_model* m, const Layer& L, PwConvArgs& q, const EvalCursor& c) {
  const Layer* Q = chain_target(m, L);
  if (!Q) return false;
  const float* sz = m->scale_bias + Q->sb_off;
  spk_pw_set_chain(q, m->wpack + Q->wpw_off, (bf16_t*)m->TI(c, Q->d.dst), sz, sz + Q->cout_p, Q->d.cout, Q->d.relu);
  return true;
}

// the identity bottleneck whose first conv is L (pass_bottlenecks: 4 * L.d.cout trunk channels)
static BneckArgs bneck_args(spk_model* m, const Layer& L, const EvalCursor& c) {
  const Layer& L2 = m->layers[L.bn_c2];
  const Layer& L3 = m->layers[L.bn_c3];
  const TDim& in = m->tdims[L.d.src];
  const float *s1 = m->scale_bias + L.sb_off, *s2 = m->scale_bias + L2.sb_off, *s3 = m->scale_bias + L3.sb_off;
  return spk_bneck_args((const bf16_t*)m->TI(c, L.d.src), (bf16_t*)m->TI(c, L3.d.dst), m->wpack + L.wpw_off,
                        m->wpack + L2.wpw_off, m->wpack + L3.wpw_off, s1, s1 + L.cout_p, s2, s2 + L2.cout_p, s3,
                        s3 + L3.cout_p, c.n, in.h, in.w, L.d.cout);
}

static int bneck_choice_paired(spk_model* m, Layer& L, const BneckArgs& a, const EvalCursor& c, unsigned allow, int* choice);

// whole-bottleneck kernel or three launches?  0: three launches, 1: blocks of 14 rows x 8 waves (one per CU), 2: blocks of
// 7 rows x 4 waves (two per CU).  Below a quarter of the chip 0 and 2 are timed once per problem (the same bits either
// way), "bneck" entries of the tuner table; without tuning 2, not remembered
static int bneck_choice(spk_model* m, Layer& L, const BneckArgs& a, const EvalCursor& c, unsigned allow) {
  if (m->bneck >= 2) return m->bneck == 3 ? 2 : 1;
  int paired = 0;
  if (bneck_choice_paired(m, L, a, c, allow, &paired)) return paired;
  const int big_blocks = a.N * (a.H / 14);
  // Two half batches on two streams: each half's large blocks take every other CU (140 KB of LDS: one block per CU), the two
  // launches start a few microseconds apart and their HBM-bound phases do not coincide (ResNet-50, batch 256: 3.33 ms; with
  // the small blocks, which share CUs across the halves and run in step, 3.41).
  if (eval_twin() && eval_twin()->two_streams && big_blocks >= 96) return 1;
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
  auto three = [&]() { return three_launches(m, L, c, allow); };
  auto one = [&]() { return spk_bneck_launch(as, c.stream); };
  float t_three = 0.f, t_one = 0.f;
  const bool ok = three() == SPK_OK && one() == 0 &&   // warm-up (and the other kernels' own tuning)
                  timer.time(c.stream, 3, three, &t_three) && timer.time(c.stream, 3, one, &t_one);
  choice = ok && t_one < t_three ? 2 : 0;
  if (spk_tune_log())
    fprintf(stderr, "[spk tune bottleneck] N%d %dx%d %d->%d->%d: three kernels %.1f us, one (7-row blocks) %.1f us\n", a.N, a.H, a.W,
            a.C4, a.CM, a.C4, t_three * 1000.f / 3.f, t_one * 1000.f / 3.f);
  spk_tune_store(TUNE_BNECK, key, &choice, true);
  return choice;
}

// The same question under a twin context (a half batch of a two-stream forward, tune_table.h): no rule - the three forms
// are timed as pairs beside the other half's launch of the same form, "bneck_p" entries.  (The rule of bneck_choice for
// the two-stream forward, 14-row blocks from 96 large blocks on, was found by hand in whole-forward runs; this
// measures it per problem.)  false: no twin context, or nothing tuned and no tuning now - the rules above decide.
static int bneck_choice_paired(spk_model* m, Layer& L, const BneckArgs& a, const EvalCursor& c, unsigned allow, int* choice) {
  const SpkTwin& tw = spk_twin();
  if (tw.mode == SpkTwin::OFF) return 0;
  const int key[] = {a.H, a.CM, a.N};
  const TuneTag tag = spk_tune_tag(TUNE_BNECK);
  if (spk_tune_find(tag, key, choice)) return 1;
  if (tw.mode != SpkTwin::PAIRS || !spk_autotune_on()) return 0;
  SpkLaunchTimer timer;
  const SpkPair<BneckArgs> pa(a);
  if (!timer.ok || !pa.ok) return 0;
  const EvalCursor cs[2] = {c, twin_cursor(c)};
  float t[3] = {1e30f, 1e30f, 1e30f};
  for (int form = 0; form < 3; ++form) {
    auto run = [&](int i, hipStream_t st) {
      if (form) {
        BneckArgs h = pa[i];
        if (form == 2) h.flags |= 4;
        return spk_bneck_launch(h, st);
      }
      return three_launches(m, L, cs[i], allow);   // (on its cursor's stream)
    };
    float ms = 0.f;
    if (run(0, c.stream) != 0) { (void)hipGetLastError(); continue; }   // warm-up (and the other kernels' own tuning)
    if (timer.time(c.stream, 3, true, run, &ms)) t[form] = ms;
  }
  *choice = (int)(std::min_element(t, t + 3) - t);
  if (t[*choice] >= 1e30f) return 0;
  if (spk_tune_log())
    fprintf(stderr, "[spk tune bottleneck] N%d+%d %dx%d %d->%d->%d, pairs: three kernels %.1f us, one (14-row blocks) %.1f us, one (7-row blocks) %.1f us\n",
            a.N, tw.n_twin, a.H, a.W, a.C4, a.CM, a.C4, t[0] * 1000.f / 3.f, t[1] * 1000.f / 3.f, t[2] * 1000.f / 3.f);
  spk_tune_store(tag, key, choice, true);
  return 1;
}

// ---- one function per form a conv can run in.  FORM_PASS: not this form (or its kernel has no instantiation for the
// problem after all) - run_conv_eval tries the next one ----
enum { FORM_PASS = 1 };

// conv2 (L) + conv3 + shortcut of an identity bottleneck (+ the next block's first conv): conv_btail_kernel
static int conv_block_tail(spk_model* m, Layer& L, const EvalCursor& c, unsigned allow) {
  if (!btail_possible(m, L, allow)) return FORM_PASS;
  const Layer& H = m->layers[L.bn_head];
  const Layer& L3 = m->layers[H.bn_c3];
  BneckArgs ba = bneck_args(m, H, c);   // (the block's input is conv3's shortcut operand; w1 is not used)
  ba.y1 = (const bf16_t*)m->TI(c, L.d.src);
  // the next block's first conv from the output tile in registers, as conv_pw.hip's chained flavour
  const Layer* Q = chain_possible(m, L3, allow) ? chain_target(m, L3) : nullptr;
  bool chained = Q && Q->d.relu == 1;
  if (chained) {
    const float* sz = m->scale_bias + Q->sb_off;
    spk_bneck_set_chain(ba, m->wpack + Q->wpw_off, (bf16_t*)m->TI(c, Q->d.dst), sz, sz + Q->cout_p, Q->d.cout);
  }
  int r = spk_btail_launch(ba, c.stream);
  if (r == -3 && chained) {      // (no instantiation with this chained width: without it)
    ba.wz = nullptr;
    chained = false;
    r = spk_btail_launch(ba, c.stream);
  }
  if (r != 0) {
    (void)hipGetLastError();
    return FORM_PASS;
  }
  const int li = index_of(m, L);
  note(m, c, allow, li, EF_OWN | EF_BTAIL | (chained ? EF_CHAIN : 0), false);   // y2 was not written
  note(m, c, allow, H.bn_c3, EF_INSIDE, true, li);
  if (chained) note(m, c, allow, L3.chain_next, EF_INSIDE, true, li);
  return SPK_OK;
}

// the whole identity bottleneck whose first conv is L: conv_bneck.hip
static int conv_whole_block(spk_model* m, Layer& L, const EvalCursor& c, unsigned allow) {
  if (!bneck_possible(m, L, allow)) return FORM_PASS;
  BneckArgs ba = bneck_args(m, L, c);
  const int form = bneck_choice(m, L, ba, c, allow);
  if (!form) return FORM_PASS;
  if (form == 2) ba.flags |= 4;
  if (spk_bneck_launch(ba, c.stream) != 0) {
    (void)hipGetLastError();               // (no instantiation after all, or the launch was refused: three launches)
    return FORM_PASS;
  }
  const int li = index_of(m, L);
  note(m, c, allow, li, EF_OWN | EF_BNECK, false);          // y1 was not written,
  note(m, c, allow, L.bn_c2, EF_INSIDE, false, li);         // nor y2;
  note(m, c, allow, L.bn_c3, EF_INSIDE, true, li);          // conv3's output was
  return SPK_OK;
}

static int conv_stem3(spk_model* m, const Layer& L, const EvalCursor& c) {
  const TDim& in = m->tdims[L.d.src];
  const TDim& o = m->tdims[L.d.dst];
  const float* sc = m->scale_bias + L.sb_off;
  if (spk_launch_stem3x3((const bf16_t*)m->TI(c, L.d.src), m->dwpack + L.wpack_off, sc, sc + L.cout_p,
                         (bf16_t*)m->TI(c, L.d.dst), c.n, in.h, in.w, in.w, o.h, o.w, L.d.cout, L.cout_p, L.d.relu,
                         m->infer_dt, c.stream))
    return spk_fail(SPK_ERR_HIP, std::string("stem launch failed for ") + L.d.name);
  return SPK_OK;
}

static int conv_grouped(spk_model* m, const Layer& L, const EvalCursor& c) {
  const TDim& in = m->tdims[L.d.src];
  const float* sc = m->scale_bias + L.sb_off;
  if (spk_launch_group_fwd((const bf16_t*)m->TI(c, L.d.src), m->P(L.p_w), sc, sc + L.cout_p, (bf16_t*)m->TI(c, L.d.dst), c.n,
                           in.h, in.w, L.d.cin, L.groups, L.d.stride, L.d.relu, m->infer_dt, c.stream))
    return spk_fail(SPK_ERR_HIP, std::string("grouped conv launch failed for ") + L.d.name);
  return SPK_OK;
}

// the implicit GEMM's arguments: what every dense form below starts from (pw_args / c3_args of conv_args.h derive theirs)
static ConvArgs conv_args(spk_model* m, const Layer& L, const EvalCursor& c) {
  const TDim& in = m->tdims[L.d.src];
  const TDim& o = m->tdims[L.d.dst];
  const float* scale = m->scale_bias + L.sb_off;
  const ConvGeom g = {c.n, in.h, in.w, in.c, o.h, o.w, o.c, L.mode == CONV_MODE_GENERIC ? L.cin_p : in.c, L.cout_p, L.kpad,
                      L.d.k, L.d.stride, L.d.pad};
  ConvArgs a = spk_conv_args(g, (const bf16_t*)m->TI(c, L.d.src), m->wpack + L.wpack_off, (bf16_t*)m->TI(c, L.d.dst),
                             L.d.res >= 0 ? (const bf16_t*)m->TI(c, L.d.res) : nullptr, scale, scale + L.cout_p, L.d.relu,
                             m->infer_dt, layer_split(m, L));
  a.res_lo = L.d.res >= 0 ? (const bf16_t*)m->TLo(L.d.res) : nullptr;
  a.y_lo = (bf16_t*)m->TLo(L.d.dst);
  return a;
}

// the chained flavour of the block-closing conv's launch q: true when it ran - the next block's first conv is done
static bool conv_chained(spk_model* m, Layer& L, const PwConvArgs& q, const EvalCursor& c, unsigned allow) {
  if (!chain_possible(m, L, allow)) return false;
  PwConvArgs qc = q;
  if (chain_args(m, L, qc, c) && chain_choice(m, L, qc, c, allow) == 1 && spk_pw_chain_launch(qc, c.stream) == 0) {
    const int li = index_of(m, L);
    note(m, c, allow, li, EF_OWN | EF_CHAIN | (q.x2 ? EF_DUAL : 0), true);
    note(m, c, allow, L.chain_next, EF_INSIDE, true, li);
    return true;
  }
  (void)hipGetLastError();
  return false;
}

// block-closing conv + the shortcut conv of its block as one K-concatenated GEMM
static int conv_dual(spk_model* m, Layer& L, const EvalCursor& c, unsigned allow, const ConvArgs& a) {
  if (!dual_active(m, L, allow) || a.y_lo) return FORM_PASS;
  Layer& D = m->layers[L.dual_src];
  const TDim& din = m->tdims[D.d.src];
  PwConvArgs q = pw_args(a, m->wdual + L.wdual_off);   // (stride 1: what the pairing asks of L)
  q.res = nullptr;
  q.scale = m->sdual + L.sdual_off; q.shift = q.scale + L.d.cout;
  spk_pw_set_second(q, (const bf16_t*)m->TI(c, D.d.src), D.d.cin, din.h, din.w, D.d.stride);
  if (conv_chained(m, L, q, c, allow)) return SPK_OK;
  const int r = spk_conv1x1_dual_launch(q, c.stream);
  if (r == 0) {
    note(m, c, allow, index_of(m, L), EF_OWN | EF_DUAL, true);
    return SPK_OK;
  }
  if (r != -3) return spk_fail(SPK_ERR_HIP, std::string("fused 1x1 conv launch failed for ") + L.d.name);
  // no configuration fits this problem: the shortcut conv on its own after all, then this layer the usual way
  SPK_TRY(run_conv_eval(m, D, c, 0));
  note(m, c, allow, L.dual_src, EF_OWN, true);
  L.dual_ok = false;
  return FORM_PASS;
}

static int conv_1x1(spk_model* m, Layer& L, const EvalCursor& c, unsigned allow, const ConvArgs& a) {
  if (!(L.pw_ok && a.dt == DT_F16 && !a.res_lo && !a.y_lo && !a.cin_s && !a.cout_s && !a.pool_y)) return FORM_PASS;
  const PwConvArgs q = pw_args(a, m->wpack + L.wpw_off);
  if (q.res && conv_chained(m, L, q, c, allow)) return SPK_OK;
  if (spk_conv1x1_launch(a, q, c.stream))
    return spk_fail(SPK_ERR_HIP, std::string("1x1 conv launch failed for ") + L.d.name);
  return SPK_OK;
}

static int conv_3x3_c3(spk_model* m, const Layer& L, const EvalCursor& c, const ConvArgs& a) {
  static const bool use_c3 = !getenv("SPK_C3") || atoi(getenv("SPK_C3")) != 0;
  if (!(use_c3 && L.c3_ok && a.dt == DT_F16 && !a.res_lo && !a.y_lo && !a.cin_s && !a.cout_s)) return FORM_PASS;
  const int r = spk_conv3x3_launch(c3_args(a, m->wpack + L.wpw_off, a.splitw ? 2 : 1), c.stream);
  if (r == 0) return SPK_OK;
  if (r != -3) return spk_fail(SPK_ERR_HIP, std::string("3x3 conv launch failed for ") + L.d.name);
  return FORM_PASS;
}

static int conv_3x3_d3(spk_model* m, const Layer& L, const EvalCursor& c, const ConvArgs& a) {
  if (!(L.d3_ok && a.dt == DT_F16 && !a.splitw && !a.res_lo && !a.y_lo && !a.cin_s && !a.cout_s && !a.pool_y)) return FORM_PASS;
  if (spk_conv3x3_d3_launch(a, c3_args(a, m->wpack + L.wd3_off, 1), c.stream))
    return spk_fail(SPK_ERR_HIP, std::string("3x3 conv launch failed for ") + L.d.name);
  return SPK_OK;
}

// One conv layer in the first form that applies, in this order of precedence.  (spk_run_layer_eval has recorded it as
// "its own launch, written"; the forms that do more, or less, say so.)
static int run_conv_eval(spk_model* m, Layer& L, const EvalCursor& c, unsigned allow) {
  const int li = index_of(m, L);
  EvalCarry& carry = m->carry[c.half];
  int r;
  if ((r = conv_block_tail(m, L, c, allow)) != FORM_PASS) return r;
  if ((r = conv_whole_block(m, L, c, allow)) != FORM_PASS) return r;
  if (L.fused_into >= 0 && dual_active(m, m->layers[L.fused_into], allow)) {
    note(m, c, allow, li, EF_INSIDE, false, L.fused_into);   // computed inside the block-closing conv's kernel, never written
    return SPK_OK;
  }
  if (L.mode == CONV_MODE_STEM3) return conv_stem3(m, L, c);
  if (L.mode == CONV_MODE_GROUP) return conv_grouped(m, L, c);
  ConvArgs a = conv_args(m, L, c);
  if (L.gate_from >= 0 && (allow & EVAL_FORWARD) && (carry.ran[L.gate_from].form & EF_GATES)) {
    // the squeeze-excitation layer in front left its gates instead of the scaled tensor: read what IT read
    if (!carry.gate) return spk_fail(SPK_ERR_STATE, std::string("no squeeze-excitation gates for ") + L.d.name);
    a.x = (const bf16_t*)m->TI(c, m->layers[L.gate_from].d.src);
    spk_set_gate(a, carry.gate, carry.gate_stride);
  }
  if (stem_pool_fused(m, L, allow)) {   // the max-pool layer that follows is computed here and finds itself done
    const Layer& P = m->layers[L.fuse_pool];
    const TDim& po = m->tdims[P.d.dst];
    a.pool_y = (bf16_t*)m->TI(c, P.d.dst);
    a.pool_ho = po.h;
    a.pool_wo = po.w;
    note(m, c, allow, li, EF_OWN | EF_POOL, false);
    note(m, c, allow, L.fuse_pool, EF_INSIDE, true, li);
  }
  if ((r = conv_dual(m, L, c, allow, a)) != FORM_PASS) return r;
  if ((r = conv_1x1(m, L, c, allow, a)) != FORM_PASS) return r;
  if ((r = conv_3x3_c3(m, L, c, a)) != FORM_PASS) return r;
  if ((r = conv_3x3_d3(m, L, c, a)) != FORM_PASS) return r;
  if (spk_conv_launch(a, L.mode, c.stream, nullptr))
    return spk_fail(SPK_ERR_HIP, std::string("conv launch failed for ") + L.d.name);
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

// fp8 mode, once per forward: does a project conv leave an e4m3 copy of its output for the expand conv that reads it
// (SPK_FP8_SHADOW=0: no, the expand convs convert the fp16 trunk themselves - same result), and is the buffer large enough?
// One buffer, re-used block after block - the launches are ordered on the stream.
static int fp8_shadow_prepare(spk_model* m) {
  const char* sh_env = getenv("SPK_FP8_SHADOW");
  // The copy of a chunk of images [img0, img0 + nb) starts at img0 * fp8_shadow_img in EVERY block, with
  // fp8_shadow_img = the largest per-image size of any shadowed tensor of the graph (inside the chunk the rows are
  // packed at the layer's own stride).  The two half-batch chains of the two-stream forward - ordered only by the
  // fork and join events, one may run a block ahead of the other - therefore never touch each other's slices.
  // (With a per-block base, half A's project conv of block k+1 wrote over the region where half B's block-k copy
  // still waited for its expand conv whenever h * w * stride changed between the blocks.)
  size_t img_bytes = 0;
  bool any = false;
  for (const Layer& L : m->layers) {
    if (L.fp8_role == 1) {
      const TDim& t = m->tdims[L.d.src];
      img_bytes = std::max(img_bytes, (size_t)t.h * t.w * ((t.c + 15) / 16 * 16));
    }
    any |= L.fp8_role == 4 && L.exp_next >= 0 && m->layers[L.exp_next].fp8_role == 1;
  }
  if (!any || (sh_env && atoi(sh_env) == 0)) img_bytes = 0;   // no copy in this forward: fp8_shadow_img == 0 says so
  const size_t need = (size_t)m->cap_n * img_bytes;
  if (img_bytes && (need > m->fp8_shadow_bytes || img_bytes != m->fp8_shadow_img)) {
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (m->fp8_shadow) HIP_TRY(hipFree(m->fp8_shadow));
    m->fp8_shadow = nullptr;
    m->fp8_shadow_bytes = 0;
    HIP_TRY(hipMalloc((void**)&m->fp8_shadow, need));
    m->fp8_shadow_bytes = need;
  }
  m->fp8_shadow_img = img_bytes;
  return SPK_OK;
}

// fp8 mode: the two 1x1 convs of an MBConv block with e4m3 tensors between them (pw_fp8.hip; the depthwise and squeeze-
// excitation layers between them: spk_run_layer_eval)
static int run_layer_fp8(spk_model* m, Layer& L, const EvalCursor& c) {
  EvalCarry& carry = m->carry[c.half];
  const int nb = c.n;
  const TDim& in = m->tdims[L.d.src];
  const TDim& o = m->tdims[L.d.dst];
  const float* sc = m->scale_bias + L.sb_off;
  switch (L.fp8_role) {
    case 1: {   // expand: trunk fp16 -> e4m3 in the loader; output e4m3 with the expanded tensor's scale
      const int kpad = (L.d.cin + 63) / 64 * 64;
      const float ys = spk_fp8_scale_of(L.amax_out);
      m->t_fp8_scale[L.d.dst] = ys;
      // the trunk as e4m3 bytes when the previous block's project conv left them (same bytes as converting here)
      const bool shadow = carry.shadow_t == L.d.src && m->fp8_shadow;
      // (the shadow holds the images of this chunk at its own row stride)
      const void* xsrc = shadow ? (const void*)(m->fp8_shadow + (size_t)c.img0 * m->fp8_shadow_img) : m->TI(c, L.d.src);
      if (spk_launch_pw_fp8(xsrc, shadow ? 1 : 0, m->w8pack + L.w8_off,
                            m->TI8(c, L.d.dst), 1, nullptr, m->s8 + L.s8_off + L.cout_p, sc + L.cout_p, nullptr, 0, in.h * in.w,
                            nb * o.h * o.w, kpad, L.cout_p, shadow ? carry.shadow_stride : in.c, o.c, L.d.relu,
                            1.f / spk_fp8_scale_of(L.amax_in), 1.f / ys, c.stream))
        return spk_fail(SPK_ERR_HIP, std::string("fp8 expand conv launch failed for ") + L.d.name);
      return SPK_OK;
    }
    default: {  // 4 project: A = the depthwise output (e4m3) x gate; fp16 trunk out (+ shortcut)
      if (L.src_se < 0 || m->layers[L.src_se].fp8_role != 3 || !carry.gate)
        return spk_fail(SPK_ERR_STATE, "fp8 project conv without its squeeze-excitation gate");
      const int se_src = m->layers[L.src_se].d.src;
      const TDim& e = m->tdims[se_src];
      const int kpad = (L.d.cin + 63) / 64 * 64;
      // the next block's expand conv reads this output: leave it an e4m3 copy (fp8_shadow_prepare)
      unsigned char* y8 = nullptr;
      int y8_stride = 0;
      float y8_inv = 0.f;
      carry.shadow_t = -1;
      if (m->fp8_shadow_img && L.exp_next >= 0 && m->layers[L.exp_next].fp8_role == 1) {
        y8_stride = (o.c + 15) / 16 * 16;
        y8 = m->fp8_shadow + (size_t)c.img0 * m->fp8_shadow_img;
        y8_inv = 1.f / spk_fp8_scale_of(m->layers[L.exp_next].amax_in);
      }
      if (spk_launch_pw_fp8(m->TI8(c, se_src), 1, m->w8pack + L.w8_off, m->TI(c, L.d.dst), 0,
                            L.d.res >= 0 ? (const bf16_t*)m->TI(c, L.d.res) : nullptr, m->s8 + L.s8_off + L.cout_p, sc + L.cout_p,
                            carry.gate, carry.gate_stride, e.h * e.w, nb * o.h * o.w, kpad, L.cout_p, e.c, o.c, L.d.relu,
                            1.f, 1.f, c.stream, y8, y8_stride, y8_inv))
        return spk_fail(SPK_ERR_HIP, std::string("fp8 project conv launch failed for ") + L.d.name);
      if (y8) { carry.shadow_t = L.d.dst; carry.shadow_stride = y8_stride; }
      m->t_fp8_scale[L.d.dst] = 0.f;
      return SPK_OK;
    }
  }
}

int spk_run_layer_eval(spk_model* m, Layer& L, const EvalCursor& c, unsigned allow) {
  const TDim& in = m->tdims[L.d.src];
  const TDim& o = m->tdims[L.d.dst];
  const int li = index_of(m, L), nb = c.n;
  EvalCarry& carry = m->carry[c.half];
  // an earlier launch of this forward computed this layer too
  if ((allow & EVAL_FORWARD) && (carry.ran[li].form & EF_INSIDE)) return SPK_OK;
  note(m, c, allow, li, EF_OWN, true);   // (what most layers are; the forms that do more, or less, say so)
  // fp8 mode, inside an MBConv block on the e4m3 path (spk_model_set_fp8): tensors of e4m3 bytes, value = byte * scale
  const bool e4m3 = m->fp8 && m->fp8_calibrated && L.fp8_role;
  if (e4m3 && L.d.kind == SPK_OP_CONV) return run_layer_fp8(m, L, c);
  switch (L.d.kind) {
    case SPK_OP_CONV: return run_conv_eval(m, L, c, allow);
    case SPK_OP_DWCONV: {
      const float* sc = m->scale_bias + L.sb_off;
      float* partial = m->SE(c);
      const float s_in = e4m3 ? spk_fp8_scale_of(L.amax_in) : 1.f, ys = e4m3 ? spk_fp8_scale_of(L.amax_out) : 1.f;
      if (e4m3) m->t_fp8_scale[L.d.dst] = ys;
      void *xs = e4m3 ? m->TI8(c, L.d.src) : m->TI(c, L.d.src), *yd = e4m3 ? m->TI8(c, L.d.dst) : m->TI(c, L.d.dst);
      // the pool partial sums of the squeeze-excitation gate that follows are a by-product
      const bool lds = e4m3 || m->infer_dt == DT_F16;
      const int chunks[2] = {spk_dw_chunks(nb, o.h * (e4m3 ? (o.w + 1) / 2 : (o.w + 3) / 4), in.c),
                             lds ? spk_dwconv_lds_chunks(e4m3, nb, in.h, in.w, in.c, o.h, o.w, L.d.k, L.d.stride) : 0};
      auto run = [&](int v) {
        if (v)
          return spk_launch_dwconv_lds(e4m3, xs, m->dwpack + L.wpack_off, sc, sc + L.cout_p, yd, partial, nb, in.h, in.w, in.c,
                                       o.h, o.w, L.d.k, L.d.stride, L.d.relu, s_in, 1.f / ys, c.stream);
        if (e4m3)
          return spk_launch_dwconv_fp8((const unsigned char*)xs, m->dwpack + L.wpack_off, sc, sc + L.cout_p, (unsigned char*)yd,
                                       partial, nb, in.h, in.w, in.c, o.h, o.w, L.d.k, L.d.stride, L.d.relu, chunks[0], s_in,
                                       1.f / ys, c.stream);
        return spk_launch_dwconv((const bf16_t*)xs, m->dwpack + L.wpack_off, sc, sc + L.cout_p, (bf16_t*)yd, partial, nb, in.h,
                                 in.w, in.c, o.h, o.w, L.d.k, L.d.stride, L.d.relu, m->infer_dt, c.stream);
      };
      const int v = dw_choose(e4m3, nb, in.h, in.w, in.c, L.d.k, L.d.stride, c.stream, run, chunks);
      carry.dw_chunks = chunks[v];
      if (run(v) != 0)
        return e4m3 ? spk_fail(SPK_ERR_HIP, std::string("fp8 depthwise launch failed for ") + L.d.name)
                    : spk_fail(SPK_ERR_UNSUPPORTED, std::string("depthwise conv launch failed (fp16 eval only) for ") + L.d.name);
      return SPK_OK;
    }
    case SPK_OP_SE: {
      // src is the output of a depthwise conv, which left its pool partials in the scratch
      if (L.se_dw < 0) return spk_fail(SPK_ERR_UNSUPPORTED, "squeeze-excitation must follow a depthwise conv");
      float* partial = m->SE(c);
      const int chunks = carry.dw_chunks;   // as the depthwise launch that just ran
      float* scale = partial + (size_t)nb * chunks * in.c;
      // the gates only when the project conv behind this layer multiplies them into its operand (SPK_SE_FUSE=0: never; the
      // e4m3 path: always): the scaled tensor - one read and one write of the widest tensor of the block - is then not
      // materialised
      const bool gate_only = e4m3 || ((allow & FUSE_GATE) && m->fuse_se && L.gate_conv >= 0 && m->infer_dt == DT_F16 && !m->precise_res);
      if (spk_launch_se(gate_only ? nullptr : (const bf16_t*)m->TI(c, L.d.src), gate_only ? nullptr : (bf16_t*)m->TI(c, L.d.dst),
                        partial, chunks, scale, m->P(L.p_w), m->P(L.p_b), m->dwpack + L.wpack_off, m->P(L.p_b2), nb,
                        in.h * in.w, L.d.cin, in.c, L.d.k, e4m3 ? DT_F16 : m->infer_dt, c.stream, L.d.relu == SPK_ACT_RELU ? 1 : 0))
        return e4m3 ? spk_fail(SPK_ERR_HIP, std::string("squeeze-excitation launch failed for ") + L.d.name)
                    : spk_fail(SPK_ERR_UNSUPPORTED, std::string("squeeze-excitation launch failed (fp16 eval only) for ") + L.d.name);
      carry.gate = gate_only ? scale : nullptr;
      carry.gate_stride = in.c;
      if (e4m3) m->t_fp8_scale[L.d.dst] = 0.f;   // not materialised
      if (gate_only) note(m, c, allow, li, EF_OWN | EF_GATES, false);
      return SPK_OK;
    }
    case SPK_OP_MAXPOOL:
      if (spk_launch_maxpool((const bf16_t*)m->TI(c, L.d.src), (bf16_t*)m->TI(c, L.d.dst), nb, in.h, in.w,
                             in.c, L.d.k, L.d.stride, L.d.pad, o.h, o.w, m->infer_dt, c.stream))
        return spk_fail(SPK_ERR_HIP, "maxpool launch failed");
      return SPK_OK;
    case SPK_OP_GAVGPOOL:
      if (spk_launch_gavgpool((const bf16_t*)m->TI(c, L.d.src), (float*)m->TI(c, L.d.dst), nb, in.h * in.w,
                              in.c, m->infer_dt, c.stream))
        return spk_fail(SPK_ERR_HIP, "avgpool launch failed");
      return SPK_OK;
    case SPK_OP_LINEAR:
      if (spk_launch_linear_fwd((const float*)m->TI(c, L.d.src), m->P(L.p_w), m->P(L.p_b),
                                (float*)m->TI(c, L.d.dst), nb, L.d.cin, L.d.cout, c.stream))
        return spk_fail(SPK_ERR_HIP, "linear launch failed");
      return SPK_OK;
    case SPK_OP_DROPOUT:  // eval: identity
      HIP_TRY(hipMemcpyAsync(m->TI(c, L.d.dst), m->TI(c, L.d.src), (size_t)nb * in.c * 4,
                             hipMemcpyDeviceToDevice, c.stream));
      return SPK_OK;
  }
  return spk_fail(SPK_ERR_UNSUPPORTED, "unknown layer kind");
}

// All layers of one eval forward, in graph order on the handle's stream.  (Two round-2 experiments lived here behind
// environment switches and are gone since round 4, both measured slower on ResNet-50 at batch 256 - DESIGN.md section 5:
// the shortcut convs of a block forked onto a side stream, 5.40 vs 5.30 ms; the leading layers run in 32-64 image chunks so
// that their tensors stay in the 256 MiB Infinity Cache, 5.57-5.62 vs 5.51 ms.)
static int run_layers_eval(spk_model* m, int nb) {
  const EvalCursor c{0, 0, nb, m->stream};
  spk_eval_begin(m, nb);
  for (Layer& L : m->layers) SPK_TRY(spk_run_layer_eval(m, L, c, FUSE_ALL | EVAL_FORWARD));
  return SPK_OK;
}

int spk_forward_eval_logits(spk_model* m, const void* x, int n, int h, int w, int layout, int dtype,
                            float* logits_dev) {
  if (!m || !x || n <= 0) return spk_fail(SPK_ERR_ARG, "forward: bad arguments");
  if (dtype != SPK_DTYPE_F32 && dtype != SPK_DTYPE_U8) return spk_fail(SPK_ERR_ARG, "forward: dtype must be f32 or u8");
  HIP_TRY(hipSetDevice(m->device));
  if (m->splitw == 5 && !m->have_means)
    return spk_fail(SPK_ERR_STATE, "the calibrated single-pass mode needs activation means first: spk_model_calibrate_act_means "
                                   "on representative images, or spk_model_set_act_means with stored ones");
  SPK_TRY(spk_commit(m));
  SPK_TRY(spk_plan(m, n, h, w));
  if (m->fp8 && !m->fp8_calibrated)
    return spk_fail(SPK_ERR_STATE, "fp8 mode needs activation ranges first: call spk_model_calibrate_fp8 on a representative batch");
  if (m->fp8) SPK_TRY(spk_fp8_pack(m));
  if (m->fp8) SPK_TRY(fp8_shadow_prepare(m));
  m->t_fp8_scale.assign(m->n_tensors, 0.f);
  const int mb = spk_micro_batch(m, n);
  const int last = m->layers.back().d.dst;
  m->act_dt = m->infer_dt;
  // Two halves of the batch on two streams (ResNets, one micro-batch, n >= 64): the layers of a forward are a chain,
  // but the two halves are independent, so an HBM-bound layer of one half runs beside an MFMA-bound layer of the other
  // and the tail of every kernel is covered by the other stream's work.  Both halves live in the SAME activation
  // tensors (images [0, n/2) and [n/2, n): EvalCursor::img0), launches are interleaved layer by layer, the caller's stream
  // forks before the first layer and joins after the last.  Per-image results do not depend on the split.  Measured
  // (ResNet-50, batch 256): 4.52 -> 4.29 ms.  SPK_EVAL_STREAMS=1 keeps one stream.
  static const int n_streams = getenv("SPK_EVAL_STREAMS") ? atoi(getenv("SPK_EVAL_STREAMS")) : 2;
  if (n_streams >= 2 && !m->precise_res && n >= 64 && n <= mb) {
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
    const int cnt[2] = {n / 2, n - n / 2}, off[2] = {0, n / 2};
    // one chain per half: what a layer leaves for the next one of ITS chain (pool-partial rows, gates, e4m3 shadow, the
    // record) is spk_model::carry[half]
    const EvalCursor ch[2] = {{0, off[0], cnt[0], str[0]}, {1, off[1], cnt[1], str[1]}};
    // paired tuning: the tuners reached from a half's launches time their candidates beside the other half's (the first
    // forward, whose second stream is idle) and look their "_p" entries up (every forward); the MBConv networks keep
    // the isolated entries
    const int twin_mode = !spk_tune_paired_on() || m->effnet ? SpkTwin::OFF : (warm ? SpkTwin::LOOKUP : SpkTwin::PAIRS);
    const EvalTwin tw[2] = {{m, off[0], off[1], cnt[1], warm}, {m, off[1], off[0], cnt[0], warm}};
    const SpkTwin twin[2] = {{twin_mode, m->half_stream, cnt[0], cnt[1], spk_twin_rebase, (void*)&tw[0]},
                             {twin_mode, m->half_stream, cnt[1], cnt[0], spk_twin_rebase, (void*)&tw[1]}};
    HIP_TRY(hipEventRecord(m->half_fork, main_s));
    HIP_TRY(hipStreamWaitEvent(m->half_stream, m->half_fork, 0));
    // on every way out: no twin context, and the caller's stream joins the second one (also after an error: nothing may be
    // left running there behind the caller's back)
    struct Leave {
      spk_model* m;
      ~Leave() {
        spk_twin() = SpkTwin();
        (void)hipEventRecord(m->half_join, m->half_stream);
        (void)hipStreamWaitEvent(m->stream, m->half_join, 0);
      }
    } leave{m};
    spk_eval_begin(m, n);
    for (const EvalCursor& c : ch) {
      const char* xi = (const char*)x + (size_t)c.img0 * spk_image_stride_bytes(m->in_chans, h, w, dtype);
      if (spk_launch_to_nhwc4(xi, layout, dtype, c.n, m->in_chans, h, w, (bf16_t*)m->TI(c, 0), m->infer_dt, c.stream, SPK_INPUT_SCALE))
        return spk_fail(SPK_ERR_HIP, "input conversion launch failed");
    }
    for (Layer& L : m->layers)
      for (int hf = 0; hf < 2; ++hf) {
        spk_twin() = twin[hf];
        SPK_TRY(spk_run_layer_eval(m, L, ch[hf], FUSE_ALL | EVAL_FORWARD));
      }
    for (const EvalCursor& c : ch)
      if (hipMemcpyAsync(logits_dev + (size_t)c.img0 * m->num_classes, m->TI(c, last), (size_t)c.n * m->num_classes * 4,
                         hipMemcpyDeviceToDevice, c.stream) != hipSuccess)
        return spk_fail(SPK_ERR_HIP, "logits copy failed");
    return SPK_OK;
  }
  for (int i0 = 0; i0 < n; i0 += mb) {
    const int nb = std::min(mb, n - i0);
    const char* xi = (const char*)x + (size_t)i0 * spk_image_stride_bytes(m->in_chans, h, w, dtype);
    if (spk_launch_to_nhwc4(xi, layout, dtype, nb, m->in_chans, h, w, (bf16_t*)m->T(0), m->infer_dt, m->stream, SPK_INPUT_SCALE))
      return spk_fail(SPK_ERR_HIP, "input conversion launch failed");
    SPK_TRY(run_layers_eval(m, nb));
    HIP_TRY(hipMemcpyAsync(logits_dev + (size_t)i0 * m->num_classes, m->T(last),
                           (size_t)nb * m->num_classes * 4, hipMemcpyDeviceToDevice, m->stream));
  }
  return SPK_OK;
}

extern "C" int spk_forward_infer(spk_model* m, const void* x, int n, int h, int w, int layout,
                                 int dtype, float softmax_base, float* out_dev) {
  if (!out_dev) return spk_fail(SPK_ERR_ARG, "forward: null output");
  if (softmax_base <= 0.f) return spk_forward_eval_logits(m, x, n, h, w, layout, dtype, out_dev);
  if (!m) return spk_fail(SPK_ERR_ARG, "null model");
  HIP_TRY(hipSetDevice(m->device));
  SPK_TRY(spk_plan(m, n, h, w));
  float* logits = (float*)((char*)m->arena + m->logits_off);
  SPK_TRY(spk_forward_eval_logits(m, x, n, h, w, layout, dtype, logits));
  // softmax(z * ln(base)) == base^z / sum base^z   (probability.py:191-194)
  if (spk_launch_softmax(logits, out_dev, n, m->num_classes, logf(softmax_base), m->stream))
    return spk_fail(SPK_ERR_HIP, "softmax launch failed");
  return SPK_OK;
}

extern "C" int spk_eval_step(spk_model* m, const void* x, int n, int h, int w, int layout, int dtype,
                             const int64_t* y, float* stats, float* logits_out) {
  if (!m || !y || !stats) return spk_fail(SPK_ERR_ARG, "eval_step: bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  SPK_TRY(spk_plan(m, n, h, w));
  float* logits = logits_out ? logits_out : (float*)((char*)m->arena + m->logits_off);
  SPK_TRY(spk_forward_eval_logits(m, x, n, h, w, layout, dtype, logits));
  // CrossEntropyLoss is a batch mean; the caller accumulates loss*n (train.py:269)
  // validation uses the loss the training step uses, as the reference's single loss_fn (spk_model_set_loss)
  CeArgs ce;
  ce.z = logits, ce.ya = y, ce.n = n, ce.c = m->num_classes, ce.stats = stats;
  ce.w = m->loss_w, ce.eps = m->loss_eps, ce.counts = m->class_counts;
  ce.plain = !m->loss_ex();
  if (spk_launch_ce(ce, m->stream)) return spk_fail(SPK_ERR_HIP, "cross-entropy launch failed");
  return SPK_OK;
}

// read_activation: tensor t as the plain launches write it, where the last eval forward did not (either half-batch chain's
// record says so).  Whatever the producer needs that the forward did not leave either comes first: conv1 of a bottleneck
// before its conv2 (the block's input is still there), the depthwise conv before a squeeze-excitation layer (for its pool
// partial sums).  No fusion, and the record stays what the forward wrote.
static int materialise(spk_model* m, int t) {
  const EvalCursor c{0, 0, m->last_eval_nb, m->stream};   // all its images at once, on chain 0
  if (c.n <= 0) return SPK_OK;
  for (size_t i = 0; i < m->layers.size(); ++i) {
    Layer& L = m->layers[i];
    if (L.d.dst != t) continue;
    bool missing = false;
    for (const EvalCarry& k : m->carry) missing |= i < k.ran.size() && k.ran[i].form != EF_NONE && !k.ran[i].wrote;
    if (!missing) continue;
    if (L.d.kind == SPK_OP_CONV && L.bn_head >= 0) SPK_TRY(spk_run_layer_eval(m, m->layers[L.bn_head], c, 0));
    if (L.d.kind == SPK_OP_SE && L.se_dw >= 0) SPK_TRY(spk_run_layer_eval(m, m->layers[L.se_dw], c, 0));
    SPK_TRY(spk_run_layer_eval(m, L, c, 0));
  }
  return SPK_OK;
}

extern "C" int spk_model_read_activation(spk_model* m, int t, int n, float* host, int64_t numel) {
  if (!m || !host || t <= 0 || t >= m->n_tensors || !m->arena || n > m->cap_n)
    return spk_fail(SPK_ERR_ARG, "read_activation: bad arguments or no forward has run");
  const TDim& d = m->tdims[t];
  const int cl = d.c_log > 0 ? d.c_log : d.c;  // the caller sees the logical channels only
  const size_t cnt = (size_t)n * d.h * d.w * d.c;
  if ((int64_t)((size_t)n * d.h * d.w * cl) != numel) return spk_fail(SPK_ERR_ARG, "read_activation: size mismatch");
  HIP_TRY(hipSetDevice(m->device));
  SPK_TRY(materialise(m, t));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (!d.bf16) {
    HIP_TRY(hipMemcpy(host, m->T(t), cnt * 4, hipMemcpyDeviceToHost));
    return SPK_OK;
  }
  const float sc8 = t < (int)m->t_fp8_scale.size() ? m->t_fp8_scale[t] : 0.f;   // > 0: e4m3 bytes, value = byte * scale
  const size_t esz = sc8 > 0.f ? 1 : 2;
  std::vector<unsigned char> tmp(cnt * esz);
  HIP_TRY(hipMemcpy(tmp.data(), m->T(t), cnt * esz, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i)
    for (int y = 0; y < d.h; ++y)
      for (int x = 0; x < d.w; ++x)
        for (int c = 0; c < cl; ++c) {
          const unsigned char* raw = &tmp[((((size_t)i * d.h + y) * d.w + x) * d.c + c) * esz];
          float f;
          if (sc8 > 0.f) {
            const unsigned b = raw[0];
            const int e = (b >> 3) & 15, mant = b & 7;
            f = e ? std::ldexp(1.f + mant / 8.f, e - 7) : std::ldexp(mant / 8.f, -6);
            if (e == 15 && mant == 7) f = NAN;
            f = (b & 0x80 ? -f : f) * sc8;
          } else if (m->act_dt == DT_F16) {
            _Float16 hv;
            memcpy(&hv, raw, 2);
            f = (float)hv;
          } else {
            const unsigned u = (unsigned)(raw[0] | raw[1] << 8) << 16;
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
  if (!m || !x || !out || cap <= 0 || iters <= 0) return spk_fail(SPK_ERR_ARG, "profile: bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  SPK_TRY(spk_commit(m));
  SPK_TRY(spk_plan(m, n, h, w));
  if (m->fp8 && m->fp8_calibrated) SPK_TRY(fp8_shadow_prepare(m));
  const int nb = std::min(n, spk_micro_batch(m, n));
  const EvalCursor c{0, 0, nb, m->stream};
  const int nl = (int)m->layers.size();
  std::vector<hipEvent_t> ev(nl + 2);
  for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
  std::vector<double> ms(nl + 1, 0.0);
  for (int it = 0; it < iters + 1; ++it) {  // first pass is a warm-up
    HIP_TRY(hipEventRecord(ev[0], m->stream));
    if (spk_launch_to_nhwc4(x, layout, dtype, nb, m->in_chans, h, w, (bf16_t*)m->T(0), m->infer_dt, m->stream, SPK_INPUT_SCALE))
      return spk_fail(SPK_ERR_HIP, "input conversion launch failed");
    HIP_TRY(hipEventRecord(ev[1], m->stream));
    spk_eval_begin(m, nb);
    for (int i = 0; i < nl; ++i) {
      SPK_TRY(spk_run_layer_eval(m, m->layers[i], c, FUSE_ALL | EVAL_FORWARD));
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
  // names, FLOPs and bytes: what the record of the pass above (one stream: chain 0) says each launch computed
  for (int i = 0; i < nl; ++i) {
    const Layer& L = m->layers[i];
    const unsigned form = m->carry[0].ran[i].form;
    const TDim& in = m->tdims[L.d.src];
    const TDim& o = m->tdims[L.d.dst];
    double fl = 0, by = 0;
    const double in_b = (double)nb * in.h * in.w * in.c * (in.bf16 ? 2 : 4);
    const double out_b = (double)nb * o.h * o.w * o.c * (o.bf16 ? 2 : 4);
    char nm[96];
    // the conv a chained launch also computed: it read that conv's weights and wrote its output
    auto add_chained = [&](const Layer& Q) {
      const TDim& zo = m->tdims[Q.d.dst];
      fl += 2.0 * nb * zo.h * zo.w * (double)Q.d.cout * Q.d.cin;
      by += (double)nb * zo.h * zo.w * zo.c * 2 + (double)Q.d.cout * Q.d.cin * 2;
      char both[96];
      snprintf(both, sizeof both, "%.60s>%.30s", nm, Q.d.name);
      snprintf(nm, sizeof nm, "%s", both);
    };
    if (L.d.kind == SPK_OP_CONV) {
      fl = 2.0 * nb * o.h * o.w * (double)L.d.cout * L.d.cin * L.d.k * L.d.k / L.groups;
      const double real_in = L.mode == CONV_MODE_STEM ? (double)nb * in.h * in.w * 8 : in_b;
      by = real_in + out_b + (L.d.res >= 0 ? out_b : 0) + (double)L.d.cout * L.kpad * 2;
      snprintf(nm, sizeof nm, "%s", L.d.name);
      if (form & EF_INSIDE) by = fl = 0;   // computed by another layer's launch: its row carries this conv
      if (form & EF_DUAL) {   // no shortcut tensor: reads both inputs, writes the output once
        const Layer& D = m->layers[L.dual_src];
        const TDim& din = m->tdims[D.d.src];
        fl += 2.0 * nb * o.h * o.w * (double)D.d.cout * D.d.cin;
        by = in_b + (double)nb * o.h * o.w * din.c * 2 + out_b + (double)L.d.cout * (L.d.cin + D.d.cin) * 2;
        snprintf(nm, sizeof nm, "%s+%s", L.d.name, D.d.name);
      }
      if (form & EF_BTAIL) {   // conv2 + conv3 + shortcut (+ chained conv): y1 in, x in, out (+ z)
        const Layer& L3 = m->layers[m->layers[L.bn_head].bn_c3];
        const double px = (double)nb * in.h * in.w;
        fl += 2.0 * px * L3.d.cin * L3.d.cout;
        by = in_b + 2.0 * px * L3.d.cout * 2 + (9.0 * L.d.cin * L.d.cout + (double)L3.d.cin * L3.d.cout) * 2;
        snprintf(nm, sizeof nm, "%.40s+conv3 (one kernel)", L.d.name);
        if (form & EF_CHAIN) add_chained(m->layers[L3.chain_next]);
      }
      if (form & EF_BNECK) {   // ... launched in this conv's place: x in (+ once more as the shortcut), out
        const Layer& L2 = m->layers[L.bn_c2];
        const Layer& L3 = m->layers[L.bn_c3];
        const double px = (double)nb * in.h * in.w;
        fl = 2.0 * px * ((double)L.d.cin * L.d.cout + 9.0 * L2.d.cin * L2.d.cout + (double)L3.d.cin * L3.d.cout);
        by = 3.0 * in_b + ((double)L.d.cin * L.d.cout + 9.0 * L2.d.cin * L2.d.cout + (double)L3.d.cin * L3.d.cout) * 2;
        snprintf(nm, sizeof nm, "%.40s+conv2+conv3 (one kernel)", L.d.name);
      }
      if ((form & EF_CHAIN) && !(form & EF_BTAIL)) add_chained(m->layers[L.chain_next]);
      if (form & EF_POOL) {   // the kernel writes the pooled tensor only
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
        else by = form & EF_GATES ? 0.0 : 3 * in_b;  // pooled once, read and written once by the scale pass (none: gates only)
        snprintf(nm, sizeof nm, "%s", L.d.name);
      } else
      snprintf(nm, sizeof nm, "%s@base.%d",
               L.d.kind == SPK_OP_MAXPOOL ? "maxpool" : (L.d.kind == SPK_OP_GAVGPOOL ? "avgpool" : "dropout"),
               L.d.child);
      if (form & EF_INSIDE) by = 0;   // computed inside the stem kernel
    }
    put(nm, ms[i + 1], fl, by);
  }
  return cnt;
}
