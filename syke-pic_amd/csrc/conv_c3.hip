// 3x3 stride-1 pad-1 convolution for gfx950 (MI355X), eval path: the 13 of ResNet-50's 16 3x3 convolutions that keep
// the spatial size (sykepic/compute/probability.py:189 reaches them through `net(x)`).
//
// The mirror image of conv_pw.hip.  There the weights sit in LDS and the activations stream into registers; here
//  * the ACTIVATIONS sit in LDS as a halo window - the input rows a tile of consecutive output pixels needs, 64 channels
//    at a time - and every one of the 9 taps reads its MFMA operand from that one window at a constant address offset:
//    the L2 -> LDS fill is 1/9 of what an im2col K loop stages, and there is no per-tap addressing or bounds logic at
//    all (the window carries explicit zero columns left and right of each image row and a zero row between images, so
//    padding taps read zeros);
//  * the WEIGHTS stream from L2 straight into MFMA operand registers: they are packed in fragment order, so a wave's
//    load is 1 KB contiguous, every block reads the same few MB (L2-resident), and a wave only needs the 32 couts it
//    owns - each weight fragment feeds the wave's MTW pixel tiles.
// A wave owns one 32-cout pair x MTW pixel tiles; the 8 waves of a block cover BN = 32 * (8 / WPP) couts x
// BM = 16 * MTW * WPP pixels.  The K loop runs chunk (64 channels) -> tap -> half (32 channels): 18 MFMA steps per
// LDS stage and barrier.  Epilogue from registers as in conv_pw.hip (swapped operand roles: a lane holds 8 consecutive
// couts of one pixel).  MTW (7, 8 or 10 pixel tiles per wave) is tuned per problem: the tile count decides how evenly
// the 256 CUs are filled (14x14 x batch 256: 448 tiles of 112 pixels = 1.75 rounds).
#include "spk_common.h"
#include "tune_pair.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

typedef __attribute__((address_space(3))) const unsigned char* lds_u8_t;
typedef __attribute__((address_space(3))) const u32x4_t* lds_u32x4_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;

// LDS image of a window stage: 8 planes, plane q = 16-byte part q (8 channels) of every window pixel, 16 B per pixel.
// A ds_read_b128 fragment read serves each of its 16-lane groups 16 DIFFERENT pixels (p = 0..15, each once, mixed over
// two parts g): inside a plane 16 consecutive pixels are 256 contiguous bytes = all 64 banks, and planes start on
// 256-byte multiples, so the read is conflict-free at ANY starting pixel - the tap shift is a pixel offset.  (A
// pixel-major image with 144-byte padded pixels, the first version, is 2-way conflicted: lanes of one group carry
// different parts g, and 9 p + g mod 16 collides.)

template <int NB, int MTW, int WPP, int UMAX>
__global__ __launch_bounds__(512, 2) void conv_c3_kernel(C3Args a, int m_tiles, int n_tiles, int rmax) {
  constexpr int NPB = 8 / WPP;            // cout pairs per block
  constexpr int BN = 32 * NPB;
  constexpr int BM = 16 * MTW * WPP;
  constexpr int PW = 3;                   // weight K steps in flight (divides the 18 steps of a chunk)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, p = lane & 15;
  const int pair_l = wave / WPP, pxg = wave % WPP;
  const int H = a.H, W = a.W, HW = H * W, WP = W + 2;
  const int CHN = a.Cin >> 6;             // 64-channel chunks
  const int pairs_total = a.Cout >> 5;

  // block -> tile (XCD-aware bijective map, n tiles of one m tile adjacent)
  const int ntiles = m_tiles * n_tiles, bw = blockIdx.x;
  const int q8 = ntiles >> 3, r8 = ntiles & 7, xcd = bw & 7;
  const int swz = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bw >> 3);
  const int nt = swz % n_tiles, mt = swz / n_tiles;
  const int m0 = mt * BM;
  const int pair_g = nt * NPB + pair_l;   // this wave's pair among all couts

  // virtual rows: image n, row y -> n * (H + 1) + 1 + y; rows n * (H + 1) are all zeros (top / bottom padding)
  const int mlast = min(m0 + BM, a.M) - 1;
  const int n_first = m0 / HW, y_first = (m0 - n_first * HW) / W;
  const int n_last = mlast / HW, y_last = (mlast - n_last * HW) / W;
  const int vr0 = n_first * (H + 1) + 1 + y_first, vr1 = n_last * (H + 1) + 1 + y_last;
  const int R = vr1 - vr0 + 3;            // window rows vr0 - 1 .. vr1 + 1  (<= rmax by the host's sizing)
  const int plane = (rmax * WP * 16 + 255) & ~255;   // bytes of one 16-byte-part plane
  const int stage_bytes = 8 * plane;

  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.wp, 0, a.wp_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, a.y_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)(a.res ? a.res : a.y), 0, a.res ? a.y_bytes : 0, 0x00020000);

  // ---- staging map of this thread: unit u = (window pixel, 16-byte part) -> source byte offset (or dropped) ----
  unsigned soff[UMAX], doff[UMAX];
  const int units = R * WP * 8;
#pragma unroll
  for (int i = 0; i < UMAX; ++i) {
    const int u = tid + i * 512;
    const int wp = u >> 3, part = u & 7;
    const int wr = wp / WP, xc = wp - wr * WP;
    const int vrow = vr0 - 1 + wr;
    const int n = vrow / (H + 1), yy = vrow - n * (H + 1) - 1;
    const bool ok = u < units && xc >= 1 && xc <= W && yy >= 0 && n < a.N;
    soff[i] = ok ? (unsigned)(((n * H + yy) * W + xc - 1) * a.Cin) * 2 + part * 16 : 0x80000000u;
    doff[i] = u < units ? (unsigned)(part * plane + wp * 16) : 0xffffffffu;
  }
  u32x4_t stg[UMAX];
  auto load_stage = [&](int c) {
#pragma unroll
    for (int i = 0; i < UMAX; ++i) stg[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, soff[i], c * 128, 0);
  };
  auto store_stage = [&](int buf) {
#pragma unroll
    for (int i = 0; i < UMAX; ++i)
      if (doff[i] != 0xffffffffu) *(u32x4_t*)(smem + buf * stage_bytes + doff[i]) = stg[i];
  };

  // ---- per-lane operand bases: pixel p of each of the wave's MTW pixel tiles, tap (0,0), channel part g ----
  unsigned abase[MTW], yoff[MTW];
#pragma unroll
  for (int j = 0; j < MTW; ++j) {
    const int m = m0 + (pxg * MTW + j) * 16 + p;
    const bool ok = m < a.M;
    const int mc = ok ? m : mlast;        // (rows past M compute on a valid pixel and are not stored)
    const int n = mc / HW, rem = mc - n * HW, y = rem / W, x = rem - y * W;
    const int wr = n * (H + 1) + 1 + y - vr0;   // window row of tap row 0
    abase[j] = (unsigned)((wr * WP + x) * 16 + g * plane);
    yoff[j] = ok ? (unsigned)m * (unsigned)(a.Cout * 2) + (unsigned)(pair_g * 32 + 8 * g) * 2 : 0x80000000u;
  }

  // ---- weights: fragment-packed [K step][pair][hi|lo][tile][lane][8]; PW steps in flight ----
  const unsigned w_lane = (unsigned)pair_g * (NB * 2048) + lane * 16;
  const unsigned w_step = (unsigned)pairs_total * (NB * 2048);
  u32x4_t wq[PW][NB][2];
  auto load_w = [&](u32x4_t (&d)[NB][2], int step) {
#pragma unroll
    for (int h = 0; h < NB; ++h)
#pragma unroll
      for (int t = 0; t < 2; ++t)
        d[h][t] = __builtin_amdgcn_raw_buffer_load_b128(rw, w_lane + (h * 2 + t) * 1024, step * w_step, 0);
  };

  f32x4_t acc[MTW][2];
#pragma unroll
  for (int j = 0; j < MTW; ++j) acc[j][0] = acc[j][1] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int KSTEPS = CHN * 18;
  load_stage(0);
#pragma unroll
  for (int s = 0; s < PW; ++s) load_w(wq[s], s);
  store_stage(0);
  __syncthreads();

  // Activation fragments: two register sets; the set of K step q+1 is read from LDS while the MFMAs of step q run
  // (left to itself hipcc reads each fragment one or two MFMAs ahead of its use - a full LDS round trip exposed per
  // four MFMAs).  The first step of a chunk is read after the barrier that publishes its stage.
  u32x4_t af[2][MTW];
  auto read_frags = [&](u32x4_t (&d)[MTW], lds_u8_t win, int off) {
#pragma unroll
    for (int j = 0; j < MTW; ++j) d[j] = *(lds_u32x4_t)(win + abase[j] + off);
  };
  for (int c = 0; c < CHN; ++c) {
    if (c + 1 < CHN) load_stage(c + 1);
    const lds_u8_t win = (lds_u8_t)smem + (c & 1) * stage_bytes;
    read_frags(af[0], win, 0);
#pragma unroll
    for (int q = 0; q < 18; ++q) {
      const int sl = q % PW;                        // static: 18 % PW == 0
      const int step = c * 18 + q;
      // hard scheduling fences (not hints): hipcc otherwise sinks every fragment read and every weight load down to
      // its first use to shorten live ranges - one register set, a full round trip exposed per pair of MFMAs
      if (q + 1 < 18) {
        const int tap = (q + 1) >> 1, kk = (q + 1) & 1;
        read_frags(af[(q + 1) & 1], win, ((tap / 3) * WP + (tap % 3)) * 16 + kk * 4 * plane);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < MTW; ++j)
#pragma unroll
        for (int h = 0; h < NB; ++h) {
          acc[j][0] = mfma16<DT_F16>(wq[sl][h][0], af[q & 1][j], acc[j][0]);
          acc[j][1] = mfma16<DT_F16>(wq[sl][h][1], af[q & 1][j], acc[j][1]);
        }
      __builtin_amdgcn_sched_barrier(0);
      // (past the last K step the same fragments are fetched again: no branch in the step)
      load_w(wq[sl], min(step + PW, KSTEPS - 1));
      __builtin_amdgcn_sched_barrier(0);
    }
    if (c + 1 < CHN) store_stage((c + 1) & 1);
    __syncthreads();
  }

  // ---- epilogue from registers: lane holds couts pair*32 + 8g .. +7 of pixel p (tile 0: +0..3, tile 1: +4..7) ----
  const int c0 = pair_g * 32 + 8 * g;
  const f32x4_t sc0 = a.scale ? *(const f32x4_t*)(a.scale + c0) : f32x4_t{1.f, 1.f, 1.f, 1.f};
  const f32x4_t sc1 = a.scale ? *(const f32x4_t*)(a.scale + c0 + 4) : f32x4_t{1.f, 1.f, 1.f, 1.f};
  const f32x4_t sh0 = a.shift ? *(const f32x4_t*)(a.shift + c0) : f32x4_t{0.f, 0.f, 0.f, 0.f};
  const f32x4_t sh1 = a.shift ? *(const f32x4_t*)(a.shift + c0 + 4) : f32x4_t{0.f, 0.f, 0.f, 0.f};
  const float floor_v = a.relu == 1 ? 0.f : -65504.f;
  // shortcut values of the wave's pixel tiles, all requested up front (a zero-record descriptor when there is none: the
  // loads return zeros and cost nothing)
  u32x4_t rq[MTW];
#pragma unroll
  for (int j = 0; j < MTW; ++j) rq[j] = __builtin_amdgcn_raw_buffer_load_b128(rr, yoff[j], 0, 0);
#pragma unroll
  for (int j = 0; j < MTW; ++j) {
    float v[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[r] = __builtin_fmaf(acc[j][0][r], sc0[r], sh0[r]);
      v[4 + r] = __builtin_fmaf(acc[j][1][r], sc1[r], sh1[r]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] += lo_f32<DT_F16>(rq[j][i]);
      v[2 * i + 1] += hi_f32<DT_F16>(rq[j][i]);
    }
    act_apply<8, false, false>(v, a.relu);   // (ReLU: the floor of the clamp below)
    u32x4_t ov;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x2_t t2 = {__builtin_amdgcn_fmed3f(v[2 * i], floor_v, 65504.f),
                          __builtin_amdgcn_fmed3f(v[2 * i + 1], floor_v, 65504.f)};
      ov[i] = __builtin_bit_cast(unsigned int, __builtin_convertvector(t2, f16x2_t));
    }
    __builtin_amdgcn_raw_buffer_store_b128(ov, ry, yoff[j], 0, 0);   // (offset in the VECTOR operand: conv_pw.hip)
  }
}

// master weights [cout][3][3][cin] -> fragment order, K step = (chunk * 9 + tap) * 2 + half
__global__ void pack_c3_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, int cout, int cin, int nb) {
  const int pairs = cout >> 5;
  const long total = (long)(cin >> 6) * 18 * pairs * 128;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int lane = (int)(idx & 63), t = (int)((idx >> 6) & 1);
  const long rest = idx >> 7;
  const int P = (int)(rest % pairs), s = (int)(rest / pairs);
  const int kk = s & 1, tap = (s >> 1) % 9, c = (s >> 1) / 9;
  const int i = lane & 15, gq = lane >> 4;
  const int co = 32 * P + 8 * (i >> 2) + 4 * t + (i & 3);
  const int ch = 64 * c + 32 * kk + 8 * gq;
  unsigned short hi[8], lo[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = w[((size_t)co * 9 + tap) * cin + ch + j];
    hi[j] = to_h16<DT_F16>(v);
    lo[j] = to_h16<DT_F16>(v - (float)__builtin_bit_cast(_Float16, hi[j]));
  }
  bf16_t* d = out + ((((size_t)s * pairs + P) * nb) * 2 + t) * 512 + lane * 8;
#pragma unroll
  for (int j = 0; j < 8; ++j) d[j] = hi[j];
  if (nb == 2) {
    d += 1024;
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = lo[j];
  }
}

int rows_max(int BM, int H, int W) {   // window rows of a BM-pixel tile, worst case
  const int images = (BM + H * W - 1) / (H * W) + 1;   // image boundaries inside the tile add a zero row each
  return (BM + W - 1) / W + 1 + images + 2;
}

template <int NB, int MTW, int WPP>
int launch_c3(const C3Args& a, hipStream_t s) {
  constexpr int NPB = 8 / WPP, BN = 32 * NPB, BM = 16 * MTW * WPP;
  if (a.Cout % BN) return -3;
  const int rmax = rows_max(BM, a.H, a.W);
  // (one 64-channel chunk: one window stage, so two blocks of a CU take turns staging and multiplying)
  const size_t lds = (size_t)(a.Cin > 64 ? 2 : 1) * 8 * (((size_t)rmax * (a.W + 2) * 16 + 255) & ~(size_t)255);
  if (lds > 160 * 1024) return -3;
  const int units = rmax * (a.W + 2) * 8;
  const int m_tiles = (a.M + BM - 1) / BM, n_tiles = a.Cout / BN;
  const int umax = (units + 511) / 512;
  auto go = [&](auto k) {
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(k, dim3(m_tiles * n_tiles), dim3(512), lds, s, a, m_tiles, n_tiles, rmax);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  };
  if (umax <= 4) return go(conv_c3_kernel<NB, MTW, WPP, 4>);
  if (umax <= 8) return go(conv_c3_kernel<NB, MTW, WPP, 8>);
  if constexpr (MTW <= 6)
    if (umax <= 12) return go(conv_c3_kernel<NB, MTW, WPP, 12>);
  return -3;
}

}  // namespace

// cfg: pixel tiles per wave x waves per pair
int spk_c3_num_configs() { return kC3NumCfgs; }
int spk_c3_launch(const C3Args& a, int cfg, hipStream_t s) {
  if (a.Cin % 64 || a.Cout % 64 || a.M <= 0 || a.dt != DT_F16) return -2;
  if ((size_t)a.M * a.Cout * 2 >= 0x80000000ull || (size_t)a.x_bytes >= 0x80000000ull) return -2;
#define C3_GO(MTW, WPP) (a.nb == 2 ? launch_c3<2, MTW, WPP>(a, s) : launch_c3<1, MTW, WPP>(a, s))
  switch (cfg) {
    case 0: return C3_GO(8, 1);    // 128 px x 256 couts
    case 1: return -3;             // (13 pixel tiles per wave: 104 accumulator + 104 fragment registers spill - removed)
    case 2: return C3_GO(7, 1);    // 112 px x 256 couts
    case 3: return C3_GO(8, 2);    // 256 px x 128 couts
    case 4: return -3;
    case 5: return C3_GO(10, 1);   // 160 px x 256 couts
    case 6: return C3_GO(10, 2);   // 320 px x 128 couts
    case 7: return C3_GO(8, 4);    // 512 px x 64 couts
    // the 64 / 128-channel layers only (ResNet-50 stages 1 and 2)
    case 8: return a.Cout >= 256 ? -3 : C3_GO(4, 4);    // 256 px x 64 couts
    case 9: return a.Cout >= 256 ? -3 : C3_GO(6, 4);    // 384 px x 64 couts
    case 10: return a.Cout >= 256 ? -3 : C3_GO(7, 2);   // 224 px x 128 couts
    // small pixel tiles for the 7 x 7 maps of a half batch (6272 pixels: 56 tiles of 112 fill a fifth of the chip's waves)
    case 11: return a.Cout < 256 ? -3 : C3_GO(4, 1);    // 64 px x 256 couts
    case 12: return a.Cout < 256 ? -3 : C3_GO(3, 1);    // 48 px x 256 couts
    case 13: return a.Cout < 256 ? -3 : C3_GO(5, 1);    // 80 px x 256 couts
    default: return -3;
  }
#undef C3_GO
}
int spk_launch_pack_c3(const float* w, bf16_t* out, int cout, int cin, int nb, hipStream_t s) {
  if (cout % 32 || cin % 64) return -2;
  const long total = (long)(cin / 64) * 18 * (cout / 32) * 128;
  hipLaunchKernelGGL(pack_c3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, out, cout, cin, nb);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------
// Eval-path entry: tile configuration tuned once per problem ("c3" entries of the tuner table).  Every configuration
// sums in the same order (chunk -> tap -> half), so the choice never shows in the output; which layers run here at all
// is a static rule of the caller (the sums differ from the implicit GEMM's tap-major order in the last bits, so that
// choice must not depend on the batch).
// ---------------------------------------------------------------------------
int spk_conv3x3_launch(const C3Args& a, hipStream_t s) {
  const int key[] = {a.nb, a.H, a.W, a.Cin, a.Cout, a.N};
  int choice;
  const TuneTag tag = spk_tune_tag(TUNE_C3);
  if (!spk_tune_find(tag, key, &choice)) {
    const bool tune = spk_autotune_on();
    const SpkPair<C3Args> pair(a);
    float best = 1e30f;
    choice = -1;
    SpkLaunchTimer timer;
    if (!timer.ok) return -1;
    for (int cfg = 0; cfg < spk_c3_num_configs(); ++cfg) {
      if (spk_c3_launch(a, cfg, s)) continue;
      if (!tune) { choice = cfg; break; }   // no tuning: the first configuration that launches, for this process only
      float ms = 0.f;
      if (!timer.time(s, 3, pair.ok, [&](int i, hipStream_t st) { return spk_c3_launch(pair[i], cfg, st); }, &ms)) continue;
      if (spk_tune_log() > 1)
        fprintf(stderr, "[spk c3 cand] N%d %dx%d C%d->%d nb%d: cfg %d %.1f us\n", a.N, a.H, a.W, a.Cin, a.Cout, a.nb, cfg, ms * 1000.f / 3.f);
      if (ms < best) { best = ms; choice = cfg; }
    }
    spk_tune_store(tag, key, &choice, tune);
    if (spk_tune_log())
      fprintf(stderr, "[spk tune 3x3] N%d %dx%d C%d->%d nb%d: cfg %d (%.1f us)\n", a.N, a.H, a.W, a.Cin, a.Cout, a.nb, choice,
              best * 1000.f / 3.f);
  }
  if (choice < 0) return -3;
  return spk_c3_launch(a, choice, s);
}
