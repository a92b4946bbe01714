// Direct 3x3 stride-1 pad-1 convolution for Cin = Cout = 64 on gfx950 (MI355X): the conv2 of ResNet-50's stage-1
// bottlenecks and the 56x56 convs of ResNet-18 / -34, fp16 eval, single weight image.
//
// The form is conv_pw.hip's RESIDENT flavour with an im2col gather on the activation load:
//  * The whole [64 couts][K = 9 x 64] panel (73.7 KB, packed by spk_launch_pack_pw over the [Cout][kh][kw][Cin] image:
//    tap major, channel minor) is copied into LDS once per block.  Two blocks fit the 160 KB of a CU.  The block is
//    persistent and walks a contiguous range of pixel tiles; after the copy there is no barrier: every wave is on its own.
//  * A lane's MFMA B fragment of K step (tap, half) - pixel l % 16, channels 32 half + 8 (l / 16) .. + 7 - is 16 bytes
//    of that tap's pixel, loaded straight into VGPRs by a buffer load whose VECTOR offset carries the tap's byte offset
//    (tap offsets are negative on the first row, and soffset takes no part in the range check); a tap that falls on
//    padding, or a pixel past M, uses offset 0x80000000, which the range check answers with zeros.  No LDS fill, no
//    ds_read and no barrier for activations.
//  * Two ways to get the nine taps (template argument PA):
//      PA > 0: one load per tap and half, PA K steps ahead of its MFMAs (across tile boundaries; PA = 18: the whole K of
//        a tile in registers, fetched one tile ahead).  Bounded by the number of loads, whatever PA is: a wave-load
//        touches 16 pixels = 16 cache lines, four lanes each in an order that costs the vector L1 a look-up per lane quad
//        (~65 clocks per wave-load, L1 hits or not) - 60 us per half batch of 128 images, 30 us with the loads dropped.
//      PA = 0 (what runs): one load per filter ROW and half - the centre tap's fragment - one tile ahead; the fragments
//        of the row's left and right taps are that register shifted by one lane inside each row of 16 lanes (DPP), the
//        end lane filled from a second load in which only the lanes at the two ends of a 16-pixel group fetch anything,
//        and zeroed where the pixel sits in the first / last column of its image row.  A third of the full wave-loads.
//  * pixel -> (image, row, column) once per tile and 16-pixel group, one tile ahead, by a multiplication with the
//    reciprocal and a correction step (pixel indices stay below 2^24: they are exact floats) - no integer division.
//  * Swapped operand roles, permuted couts and the register epilogue of conv_pw.hip (fmaf, v_med3, packed convert, one
//    16-byte store per 8 couts of a pixel).
// K order: taps 0..8, each as two 32-deep steps ascending - the implicit GEMM's order for Cin = 64, with the same
// fp32 epilogue: the output is bit-identical to conv_igemm.hip's (tests/test_gpu_d3.py).
#include "spk_common.h"
#include "tune_pair.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

typedef __attribute__((address_space(3))) const unsigned char* lds_u8_t;   // LDS reads stay ds_read (never FLAT)
typedef __attribute__((address_space(3))) const u32x4_t* lds_u32x4_t;
typedef __attribute__((address_space(3))) const f32x4_t* lds_f32x4_t;

typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
__device__ __forceinline__ unsigned int pack2_f16(float lo, float hi) {   // already clamped: v_cvt_pk_f16_f32
  const f32x2_t v = {lo, hi};
  return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, f16x2_t));
}

struct D3Geom {
  int H, W, HW, M;
  float rcp_hw, rcp_w;
};

constexpr int kC = 64;             // channels in and out
constexpr int kKS = 18;            // 32-deep K steps: 9 taps x 2 halves
constexpr int kCH = 2 * 2048;      // bytes of one K step of the panel (two 32-cout pairs)
constexpr int kPanel = kKS * kCH;  // 73 728
constexpr int kLds = kPanel + 2 * kC * 4;

// WAVES waves of MT 16-pixel groups each; activations PA K steps ahead; WPE: waves per SIMD the register budget is for
template <int MT, int WAVES, int PA, int WPE, bool HAS_RES>
__global__ __launch_bounds__(WAVES * 64, WPE) void conv_d3_kernel(C3Args a, D3Geom gm, int m_tiles) {
  constexpr bool REUSE = PA == 0;   // one load per filter ROW and half; the row's outer taps are lane shifts of it
  static_assert(REUSE || kKS % PA == 0, "the register sets rotate with the K steps of a tile");
  constexpr int DT = DT_F16;
  constexpr int NPAIR = 2, NT = 4, BN = kC;
  constexpr int WPX = MT * 16, BM = WAVES * WPX, T = WAVES * 64;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, p = lane & 15;

  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, a.y_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)a.res, 0, HAS_RES ? a.y_bytes : 0, 0x00020000);

  // block -> a contiguous range of pixel tiles (neighbouring tiles share their halo rows through L1 / L2)
  int mt = (int)((long)blockIdx.x * m_tiles / (int)gridDim.x);
  const int mt_end = (int)((long)(blockIdx.x + 1) * m_tiles / (int)gridDim.x);

  unsigned char* const sW = smem;
  float* const sScale = (float*)(smem + kPanel);   // [64] scale, then [64] shift

  // Per tile and 16-pixel group: `off`, the byte offset of the lane's 16-byte chunk g of its pixel (the same in x and y:
  // 128 bytes per pixel in both), or 0x80000000 for a pixel that does not exist; `msk`, bit t set when tap t of that
  // pixel lies inside the image.
  // `ml` / `mr` (REUSE): all ones when the pixel has a left / right neighbour in its image row.
  struct TileState { unsigned off[MT]; unsigned msk[MT]; unsigned ml[MT]; unsigned mr[MT]; };
  auto tile_state = [&](int tile, TileState& st) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int px = tile * BM + wave * WPX + m * 16 + p;
      const bool ok = tile < mt_end && px < gm.M;
      // px = img * HW + rem, rem = row * W + col: quotient by the reciprocal, off by at most one either way
      int img = (int)((float)px * gm.rcp_hw);
      int rem = px - img * gm.HW;
      if (rem < 0) rem += gm.HW;
      else if (rem >= gm.HW) rem -= gm.HW;
      int row = (int)((float)rem * gm.rcp_w);
      int col = rem - row * gm.W;
      if (col < 0) { col += gm.W; --row; }
      else if (col >= gm.W) { col -= gm.W; ++row; }
      const unsigned cm = (col > 0 ? 1u : 0u) | 2u | (col < gm.W - 1 ? 4u : 0u);
      unsigned mk = (row > 0 ? cm : 0u) | (cm << 3) | (row < gm.H - 1 ? cm << 6 : 0u);
      st.msk[m] = ok ? mk : 0u;
      st.ml[m] = ok && col > 0 ? ~0u : 0u;
      st.mr[m] = ok && col < gm.W - 1 ? ~0u : 0u;
      st.off[m] = ok ? (unsigned)px * (unsigned)(kC * 2) + (unsigned)g * 16u : 0x80000000u;
    }
  };

  f32x4_t acc[MT][NT];
  u32x4_t xa[REUSE ? 1 : PA][MT];
  // REUSE: per filter row dy and 16-pixel group, `c[h]` = the fragment of the row's CENTRE tap (pixel p of the group, one
  // row up / the same row / one row down), half h, and `e[h]` = the same 16 bytes of the pixel left of the group in
  // lane p = 0 and of the pixel right of it in lane p = 15 (eight lanes of a wave load something).  The fragment of the
  // left tap is c shifted one lane up inside each row of 16 lanes (DPP row_shr:1, lane 0 keeps e), that of the right tap
  // c shifted one lane down (row_shl:1, lane 15 keeps e); a pixel in the first / last column of its image row gets zeros
  // (`ml` / `mr`).  A wave-load of this kernel touches 16 cache lines, 4 lanes each, in an order that costs the vector L1
  // one tag look-up per lane quad (measured: ~65 clocks per 1-KB wave-load whether the lines hit L1 or not - the nine
  // loads per pixel, not their bytes, bounded the plain form); this form issues three such loads per pixel and half.
  struct RowFrag { u32x4_t c[2], e[2]; };
  RowFrag rows[REUSE ? 3 : 1][MT];

  const int row_bytes = gm.W * (kC * 2);
  // K step u of a tile: tap u / 2 at (u / 2) / 3 - 1 rows, (u / 2) % 3 - 1 columns from the pixel; half u % 2
  auto load_a = [&](u32x4_t (&dst)[MT], const TileState& st, int u) {
    const int t = u >> 1;
    const int tap_off = (t / 3 - 1) * row_bytes + (t % 3 - 1) * (kC * 2);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const unsigned vo = (st.msk[m] >> t) & 1u ? st.off[m] + (unsigned)tap_off : 0x80000000u;
      dst[m] = __builtin_amdgcn_raw_buffer_load_b128(rx, vo, (u & 1) * 64, 0);
    }
  };
  auto load_row = [&](RowFrag (&dst)[MT], const TileState& st, int dy) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const bool rok = (st.msk[m] >> (3 * dy + 1)) & 1u;   // the centre tap of that row exists
      const unsigned vo = rok ? st.off[m] + (unsigned)((dy - 1) * row_bytes) : 0x80000000u;
      const unsigned eo = p == 0 ? (rok && st.ml[m] ? vo - (unsigned)(kC * 2) : 0x80000000u)
                                 : (p == 15 && rok && st.mr[m] ? vo + (unsigned)(kC * 2) : 0x80000000u);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        dst[m].c[h] = __builtin_amdgcn_raw_buffer_load_b128(rx, vo, h * 64, 0);
        dst[m].e[h] = __builtin_amdgcn_raw_buffer_load_b128(rx, eo, h * 64, 0);
      }
    }
  };
  // fragment of tap (dy, dxi) half h out of the row's registers: dxi 0 left, 1 centre, 2 right
  auto tap_frag = [&](u32x4_t (&f)[MT], const RowFrag (&r)[MT], const TileState& st, int dxi, int h) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      if (dxi == 1) { f[m] = r[m].c[h]; continue; }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned s = dxi == 0 ? __builtin_amdgcn_update_dpp(r[m].e[h][k], r[m].c[h][k], 0x111, 0xf, 0xf, false)
                                    : __builtin_amdgcn_update_dpp(r[m].e[h][k], r[m].c[h][k], 0x101, 0xf, 0xf, false);
        f[m][k] = s & (dxi == 0 ? st.ml[m] : st.mr[m]);
      }
    }
  };
  auto init_acc = [&]() {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[m][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  };
  // weight fragments of one 32-cout pair, two register sets ping-pong (conv_pw.hip: the set of the next pair is read from
  // LDS while the MFMAs of this one run)
  struct Frag { u32x4_t w[2]; };
  Frag fr[2];
  auto load_frag = [&](Frag& f, lds_u8_t q) {
    f.w[0] = *(lds_u32x4_t)(q);
    f.w[1] = *(lds_u32x4_t)(q + 1024);
  };
  // one K step out of the LDS image at `base`; fr[0] holds pair 0; `next`: the image of the K step that follows
  auto compute = [&](lds_u8_t base, lds_u8_t next, const u32x4_t (&x)[MT]) {
#pragma unroll
    for (int P = 0; P < NPAIR; ++P) {
      if (P + 1 < NPAIR) load_frag(fr[(P + 1) & 1], base + (P + 1) * 2048 + lane * 16);
      else load_frag(fr[0], next + lane * 16);
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        acc[m][2 * P] = mfma16<DT>(fr[P & 1].w[0], x[m], acc[m][2 * P]);
        acc[m][2 * P + 1] = mfma16<DT>(fr[P & 1].w[1], x[m], acc[m][2 * P + 1]);
      }
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);        // the next pair's ds_reads first ...
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * MT, 0);   // ... then this pair's MFMAs
    }
  };

  // shortcut operand one whole tile ahead, as in conv_pw.hip: the loads of tile i + 1 are issued inside the epilogue of
  // tile i, each right after the register it lands in has been consumed
  u32x4_t rv[HAS_RES ? MT : 1][NPAIR];
  const float out_max = 65504.f;
  const float relu_floor = a.relu == 1 ? 0.f : -out_max;
  auto epilogue = [&](const unsigned (&yoff)[MT], const unsigned (&yoff_next)[MT]) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
      for (int P = 0; P < NPAIR; ++P) {
        // the lane's 8 couts of this pair: 32P + 8g .. +7 (registers 0-3 of tile 2P, then of tile 2P + 1)
        lds_f32x4_t sp = (lds_f32x4_t)(sScale + P * 32 + 8 * g);
        asm volatile("" : "+v"(sp));   // re-read per use instead of 16 VGPRs per pair held across the tile loop
        const f32x4_t sc0 = sp[0], sc1 = sp[1], sh0 = sp[BN / 4], sh1 = sp[BN / 4 + 1];
        float v[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = __builtin_fmaf(acc[m][2 * P][r], sc0[r], sh0[r]);
          v[4 + r] = __builtin_fmaf(acc[m][2 * P + 1][r], sc1[r], sh1[r]);
        }
        if (HAS_RES) {
          const u32x4_t q = rv[HAS_RES ? m : 0][P];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[2 * j] += lo_f32<DT>(q[j]);
            v[2 * j + 1] += hi_f32<DT>(q[j]);
          }
          rv[HAS_RES ? m : 0][P] = __builtin_amdgcn_raw_buffer_load_b128(rr, yoff_next[m] + P * 64, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = __builtin_amdgcn_fmed3f(v[j], relu_floor, out_max);   // ReLU = the floor
        u32x4_t ov;
#pragma unroll
        for (int j = 0; j < 4; ++j) ov[j] = pack2_f16(v[2 * j], v[2 * j + 1]);
        // the pair's column offset stays in the VECTOR offset / immediate, never in soffset (the gfx950 store-data
        // hazard described in conv_pw.hip)
        __builtin_amdgcn_raw_buffer_store_b128(ov, ry, yoff[m] + P * 64, 0, 0);
      }
    }
  };
  // before the first tile: its shortcut loads, interleaved with as many DROPPED stores (zero-record descriptor) as an
  // epilogue issues, so that the tile loop is entered with the sequence of outstanding memory operations it is re-entered
  // with (conv_pw.hip)
  auto prologue_like_an_epilogue = [&](const unsigned (&yoff)[MT]) {
    const __amdgpu_buffer_rsrc_t rnull = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, 0, 0x00020000);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int P = 0; P < NPAIR; ++P) {
        if (HAS_RES) rv[HAS_RES ? m : 0][P] = __builtin_amdgcn_raw_buffer_load_b128(rr, yoff[m] + P * 64, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{0, 0, 0, 0}, rnull, yoff[m] + P * 64, 0, 0);
      }
  };

  for (int c = tid; c < BN; c += T) {
    sScale[c] = a.scale ? a.scale[c] : 1.f;
    sScale[BN + c] = a.shift ? a.shift[c] : 0.f;
  }
  // ---- the whole panel into LDS, once: every load of the thread in flight before the first LDS write (as a loop the
  // compiler waits for each 16 bytes before it asks for the next: 18 dependent round trips in front of the first tile) ----
  {
    constexpr int RD = kPanel / (T * 16);
    static_assert(kPanel % (T * 16) == 0, "whole copy rounds");
    u32x4_t wv[RD];
#pragma unroll
    for (int r = 0; r < RD; ++r) wv[r] = *(const u32x4_t*)((const unsigned char*)a.wp + r * (T * 16) + tid * 16);
#pragma unroll
    for (int r = 0; r < RD; ++r) *(u32x4_t*)(sW + r * (T * 16) + tid * 16) = wv[r];
  }

  TileState cur, nxt;
  tile_state(mt, cur);
  tile_state(mt + 1, nxt);
  if constexpr (REUSE) {
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) load_row(rows[dy], cur, dy);   // the whole first tile
  } else {
#pragma unroll
    for (int u = 0; u < PA; ++u) load_a(xa[u], cur, u);
  }
  prologue_like_an_epilogue(cur.off);
  __syncthreads();
  const lds_u8_t sWl = (lds_u8_t)sW;
  load_frag(fr[0], sWl + lane * 16);
  // Tile loop, straight-line body: 18 K steps, each followed by the load of the step PA ahead into the register set it
  // has just freed - past the last step of this tile, the first steps of the next one.
  while (mt < mt_end) {
    init_acc();
    // one base register per K step, advanced by a VALU add the compiler cannot fold: the panel is larger than the 64 KB
    // reach of the ds_read immediate (conv_pw.hip)
    lds_u8_t sbase = sWl;
#pragma unroll
    for (int u = 0; u < kKS; ++u) {
      lds_u8_t snext = u + 1 < kKS ? sbase + kCH : sWl;
      asm volatile("" : "+v"(snext));
      if constexpr (REUSE) {
        // a filter row's six K steps out of its registers, then the same row of the NEXT tile into them
        const int dy = u / 6, dxi = (u % 6) / 2;
        u32x4_t f[MT];
        tap_frag(f, rows[dy], cur, dxi, u & 1);
        compute(sbase, snext, f);
        if (u % 6 == 5) load_row(rows[dy], nxt, dy);
      } else {
        compute(sbase, snext, xa[u % PA]);
        if (u + PA < kKS) load_a(xa[u % PA], cur, u + PA);
        else load_a(xa[u % PA], nxt, u + PA - kKS);
      }
      sbase = snext;
    }
    epilogue(cur.off, nxt.off);
    ++mt;
    cur = nxt;
    tile_state(mt + 1, nxt);
  }
}

// compute units of the current device (asked once per device of the process; 256 when the runtime does not say)
int d3_cu_count() {
  static std::atomic<int> cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int n = cus[dev].load(std::memory_order_relaxed);
  if (n > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    n = 256;
  }
  cus[dev].store(n, std::memory_order_relaxed);
  return n;
}

template <int MT, int WAVES, int PA, int WPE>
int launch_k(const C3Args& a, int bpc, hipStream_t s) {
  constexpr int BM = WAVES * MT * 16;
  const int m_tiles = (a.M + BM - 1) / BM;
  void (*k)(C3Args, D3Geom, int) = a.res ? conv_d3_kernel<MT, WAVES, PA, WPE, true> : conv_d3_kernel<MT, WAVES, PA, WPE, false>;
  static std::atomic<unsigned long long> attr[2];
  if (!spk_lds_limit_once(attr[a.res != nullptr], (const void*)k, kLds)) return -1;
  D3Geom gm;
  gm.H = a.H; gm.W = a.W; gm.HW = a.H * a.W; gm.M = a.M;
  gm.rcp_hw = 1.0f / (float)gm.HW;
  gm.rcp_w = 1.0f / (float)a.W;
  // persistent: as many blocks as stay resident on this device (bpc per CU; an MI355X has 256 CUs, a partition of it
  // fewer), and no more than there are pixel tiles
  int grid = d3_cu_count() * bpc;
  if (grid > m_tiles) grid = m_tiles;
  hipLaunchKernelGGL(k, dim3(grid), dim3(WAVES * 64), kLds, s, a, gm, m_tiles);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

int spk_d3_num_configs() { return kD3NumCfgs; }

// 0 ok, -1 HIP error, -3 this kernel / configuration does not fit the problem
int spk_d3_launch(const C3Args& a, int cfg, hipStream_t s) {
  if (a.dt != DT_F16 || a.nb != 1 || (a.relu != 0 && a.relu != 1) || a.Cin != kC || a.Cout != kC || a.M <= 0 || a.M != a.N * a.H * a.W) return -3;
  if ((size_t)a.x_bytes >= 0x80000000ull || (size_t)a.y_bytes >= 0x80000000ull) return -3;   // (also: M < 2^24)
  switch (cfg) {   //           MT WAVES PA waves/SIMD   blocks per CU
    case 0: return launch_k<2, 4, 0, 2>(a, 2, s);    // row reuse: 128-pixel tiles of four waves
    case 1: return launch_k<1, 4, 0, 2>(a, 2, s);    // row reuse: 64-pixel tiles of four waves
    case 2: return launch_k<1, 8, 0, 4>(a, 2, s);    // row reuse: 128-pixel tiles of eight waves (four per SIMD, 128 VGPRs)
    case 3: return launch_k<2, 8, 0, 2>(a, 1, s);    // row reuse: 256-pixel tiles of eight waves, one block per CU
    case 4: return launch_k<2, 4, 6, 2>(a, 2, s);    // one load per tap: 128-pixel tiles, six K steps ahead
    case 5: return launch_k<2, 4, 18, 2>(a, 2, s);   // ... the whole K of a tile in registers, fetched one tile ahead
    default: return -3;
  }
}

// ---------------------------------------------------------------------------
// Eval-path entry: one 64 -> 64 3x3 convolution by the implicit GEMM (a) or by the fastest configuration of the kernel
// above (q) - "d3" entries of the tuner table, -1 = implicit GEMM.  Both give the same bits (same K order, same fp32
// epilogue; tests/test_gpu_d3.py), so the choice never shows in the output.  Timed on one stream on the first forward
// of a shape, like the 1x1 chooser, and with its margin: the candidates run back to back on a warm cache.
// SPK_D3: 1 (default) the faster of the two; 0 never this kernel; 2 this kernel wherever it fits.
// ---------------------------------------------------------------------------
namespace {
int d3_mode() {
  static const int v = getenv("SPK_D3") ? atoi(getenv("SPK_D3")) : 1;
  return v;
}
}  // namespace

int spk_conv3x3_d3_launch(const ConvArgs& a, const C3Args& q, hipStream_t s) {
  if (d3_mode() == 0) return spk_conv_launch(a, CONV_MODE_GENERIC, s, nullptr);
  const int key[] = {q.H, q.W, q.res != nullptr, q.N};
  int choice = -1;
  const TuneTag tag = spk_tune_tag(TUNE_D3);
  const bool found = spk_tune_find(tag, key, &choice);
  if (d3_mode() == 2 && (!found || choice < 0)) choice = 0;
  if (!found && spk_autotune_on()) {
    SpkLaunchTimer timer;
    if (!timer.ok) return -1;
    float t_igemm = 1e30f, t_d3 = 1e30f;
    int best_d3 = -1;
    const SpkPair<ConvArgs> pa(a);
    const SpkPair<C3Args> pq(q);
    for (int cfg = (d3_mode() == 2 ? 0 : -1); cfg < kD3NumCfgs; ++cfg) {
      auto run = [&](int i, hipStream_t st) {
        return cfg < 0 ? spk_conv_launch(pa[i], CONV_MODE_GENERIC, st, nullptr) : spk_d3_launch(pq[i], cfg, st);
      };
      if (run(0, s)) continue;   // warm-up (and the implicit GEMM's own tuning); -3: does not fit
      float ms = 0.f;
      if (!timer.time(s, 3, pa.ok && pq.ok, run, &ms)) continue;
      if (spk_tune_log() > 1)
        fprintf(stderr, "[spk d3 cand] N%d %dx%d res%d: %s %d %.1f us\n", q.N, q.H, q.W, q.res != nullptr,
                cfg < 0 ? "igemm" : "d3", cfg, ms * 1000.f / 3.f);
      if (cfg < 0) t_igemm = ms;
      else if (ms < t_d3) { t_d3 = ms; best_d3 = cfg; }
    }
    choice = best_d3 >= 0 && t_d3 < 0.92f * t_igemm ? best_d3 : -1;
    // (SPK_D3=2 did not time the implicit GEMM: its forced winner stays in the process and is not written to the file,
    // where a default run would read it as a choice made with the margin)
    spk_tune_store(tag, key, &choice, d3_mode() != 2);
    if (spk_tune_log())
      fprintf(stderr, "[spk tune d3] N%d %dx%d res%d: %s %d (%.1f us)\n", q.N, q.H, q.W, q.res != nullptr,
              choice < 0 ? "igemm" : "d3", choice, (choice < 0 ? t_igemm : t_d3) * 1000.f / 3.f);
  }
  if (choice >= 0) {
    // a configuration that does not fit this shape or whose launch this device refuses: the implicit GEMM, same bits
    if (spk_d3_launch(q, choice, s) == 0) return 0;
    (void)hipGetLastError();
  }
  return spk_conv_launch(a, CONV_MODE_GENERIC, s, nullptr);
}
