// Implicit-GEMM 2-D convolution for gfx950 (MI355X), bf16 in / fp32 accumulate.
//
// Stands in for the torch Conv2d+BatchNorm2d(+add)(+ReLU) chains that the
// reference reaches through `net(x)` (sykepic/compute/probability.py:189,
// sykepic/train/train.py:240) — SURVEY.md §2.2.
//
// GEMM view: M = N*Ho*Wo output pixels, N = Cout, K = kh*kw*Cin with the
// filter tap major and the channel minor, so that every 16-byte chunk of K is
// 8 consecutive channels of ONE input pixel: NHWC activations are read with
// coalesced 16-B buffer loads, padding taps are dropped by the buffer range
// check (voffset past num_records reads as zero) — no divergent branches.
// Tiles are staged through LDS (XOR-swizzled 128-B rows, conflict-free for the
// 16x16x32 operand reads), double buffered, one barrier per 64-deep K step;
// v_mfma_f32_16x16x32_bf16 accumulates in fp32.  The epilogue goes back
// through LDS so that BN scale/shift, the residual add, ReLU and the bf16
// rounding happen on whole 16-B row segments and the stores are full lines.
//
// Block -> tile mapping is XCD-aware: the 8 XCDs each take a contiguous run
// of tiles, N-tiles of one M-tile adjacent, so the activation tile a block
// streams is an L2 hit for its neighbour.
#include "spk_common.h"
#include "tune_pair.h"

namespace {

constexpr int BK = 64;            // K elements per LDS stage (the default; BKT = 32 instantiations halve it)
constexpr int ROW_BYTES = BK * 2; // 128-B LDS rows

// 16-B chunk swizzle.  128-B rows (BK 64): rows r and r^1 share a 256-B bank row; (row>>1)&7 spreads 16
// consecutive rows of one chunk column over all 16 slots.  64-B rows (BK 32): four rows share a bank row; with
// chunk ^ ((row>>2)&2) every 16-lane group of a ds_read_b128 fragment read (which mixes two chunk columns, see
// MI355X_MICROARCH.md LDS) touches 16 distinct slots.
template <int BKT>
__device__ __forceinline__ int lds_off_t(int row, int chunk) {
  if (BKT == 64) return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
  return row * 64 + ((chunk ^ ((row >> 2) & 2)) << 4);
}
template <int BKT>
__device__ __forceinline__ int src_swizzle(int row) {  // DMA lands lane l in slot l % chunks: fetch chunk slot ^ this
  return BKT == 64 ? ((row >> 1) & 7) : ((row >> 2) & 2);
}

template <int BM, int BN, int WARPS_M, int WARPS_N, int MODE, int DT, int SPLITW, int DMA, int PERSIST, int BKT = 64>
__global__ __launch_bounds__(WARPS_M* WARPS_N * 64, DMA == 3 ? 2 : 1) void conv_igemm_kernel(ConvArgs a, int m_tiles,
                                                                            int n_tiles) {
  // DGRAD_BNB: the data gradient that also makes the BatchNorm-backward sums of the layer behind its output (spk_set_bnb).
  // Its own instantiation: the operands it prefetches cost 16-36 VGPRs (one wave per SIMD on several tiles) that the
  // plain data-gradient launches must not pay.
  constexpr bool IS_DGRAD = MODE == CONV_MODE_DGRAD || MODE == CONV_MODE_DGRAD_BNB;
  // BKT: K elements per LDS stage.  32 halves the stage: twice the resident blocks per CU, whose load, operand-read
  // and MFMA phases (which add up within one block) then overlap across blocks.
  constexpr int BK = BKT;
  constexpr int ROW_BYTES = BK * 2;
  constexpr int CPR = BK / 8;  // 16-B chunks per LDS row
  static_assert(BKT == 64 || (BKT == 32 && MODE != CONV_MODE_STEM && DMA != 3), "K step");
  auto lds_off = [](int row, int chunk) { return lds_off_t<BKT>(row, chunk); };
  constexpr int NTHREADS = WARPS_M * WARPS_N * 64;
  constexpr int ROWS_PER_PASS = NTHREADS / CPR;
  constexpr int WM = BM / WARPS_M, WN = BN / WARPS_N;
  constexpr int MT = WM / 16, NT = WN / 16;
  // SPLITW: weights carried as hi + lo (w = w_hi + w_lo, both 16-bit) and both
  // products accumulated: the weight rounding error (the dominant term of the
  // logit error at 16-bit storage) drops to ~2^-22 for 2x the MFMA work.
  constexpr int NB = SPLITW ? 2 : 1;
  constexpr int A_ITERS = BM / ROWS_PER_PASS, B_ITERS = NB * BN / ROWS_PER_PASS;
  constexpr int A_BYTES = BM * ROW_BYTES, B_BYTES = NB * BN * ROW_BYTES;
  static_assert(A_ITERS >= 1 && B_ITERS >= 1, "tile too small for the block");
  // DMA: tiles go HBM/L2 -> LDS directly (buffer_load ... lds), STAGES deep, so
  // STAGES-1 tiles are in flight while one is multiplied; no staging VGPRs, no
  // ds_write pass.  The LDS image must be lane-linear per wave instruction
  // (8 rows x 128 B), so the bank swizzle is applied to the SOURCE chunk.
  constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
  // DMA == 2: two stages only (half the LDS -> two blocks per CU whose phases interleave)
  // DMA == 3: hybrid, two stages: weights by LDS-DMA, activations through two register sets whose
  // LDS stores are interleaved with the MFMA rows (the LDS-DMA path sustains ~70 GB/s per CU, half
  // of what register loads get from L2: splitting the tile over both paths relieves it)
  // DMA == 4: ONE stage, no prefetch inside the block (load, wait, multiply): a third of the LDS of the two-stage
  // loop at the same tile, so more blocks are resident and THEIR phases overlap
  constexpr int STAGES = DMA == 4 ? 1 : ((!DMA || DMA >= 2) ? 2 : (STAGE_BYTES <= 32768 ? 4 : (STAGE_BYTES <= 49152 ? 3 : 2)));
  static_assert(DMA != 3 || MODE != CONV_MODE_STEM, "no hybrid stem");
  constexpr int PER_TILE = A_ITERS + B_ITERS;  // DMA instructions per wave per tile
  static_assert(!DMA || ROWS_PER_PASS % 16 == 0, "swizzle must not depend on the pass");
  constexpr int PIECE_ROWS = 1024 / ROW_BYTES;  // rows one wave-wide 16-B-per-lane DMA instruction covers

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // one LDS stage when the whole K fits in it (1x1 convs with Cin = 64):
  // half the LDS, twice the resident blocks for these HBM-bound layers
  // (and for the gated operand, PERSIST == 3: the next tile waits in the staging registers, not in a second stage)
  const int nbuf = (a.K > BK && PERSIST != 3) ? 2 : 1;
  unsigned char* const sA = smem;                    // [nbuf][BM][128 B]   (DMA: stage s at s*STAGE_BYTES)
  unsigned char* const sB = smem + (DMA ? A_BYTES : nbuf * A_BYTES);   // [nbuf][NB*BN][128 B]

  const bool cls = IS_DGRAD && a.cls_ph >= 0;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WARPS_N, wn = wave % WARPS_N;

  // Work items: tile w of m_tiles*n_tiles, w = blockIdx.x, += gridDim.x (the
  // register-staged flavour may run persistent: the first loads of the next
  // tile are issued before the epilogue of the current one).  XCD-aware,
  // bijective item -> tile map: items w and w+8 share an XCD and take
  // neighbouring tiles, N tiles of one M tile adjacent.
  const int ntiles = m_tiles * n_tiles;
  int m0 = 0, n0 = 0, mt_idx = 0, nt_idx = 0;

  const __amdgpu_buffer_rsrc_t rx =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, a.w_bytes, 0x00020000);

  // ---- per-thread staging coordinates (fixed over the K loop) ----
  const int srow = tid / CPR;
  // register staging writes chunk c to its swizzled slot; DMA lands lane l of a
  // row in slot l&7, so that lane must FETCH the chunk whose slot that is
  const int chunk_a = tid % CPR;                             // register path: plain chunk, swizzled store
  const int chunk_b = (tid % CPR) ^ src_swizzle<BKT>(srow);  // DMA path: swizzled source chunk
  const int chunk = (DMA && DMA != 3) ? chunk_b : chunk_a;  // chunk of the ACTIVATION loads
  int a_base[A_ITERS], a_h0[A_ITERS], a_w0[A_ITERS];
  int b_off[B_ITERS];
  const int HoWo = a.Ho * a.Wo;
  const int KT = a.kt_count > 0 ? a.kt_count * (64 / BK) : a.K / BK;  // kt_count is in 64-deep steps
  // scalar walk over (tap row r, tap col s, channel block c0) for generic mode
  const int r_first = (IS_DGRAD && cls) ? ((a.cls_ph + a.pad) & 1) : 0;
  const int s_first = (IS_DGRAD && cls) ? ((a.cls_pw + a.pad) & 1) : 0;
  const int tap_step = (IS_DGRAD && cls) ? 2 : 1;
  int kr = r_first, ks_ = s_first, kc0 = 0;
  int wr = r_first, ws = s_first, wc0 = 0;  // tap walk of the weight tiles (dgrad)

  // PERSIST == 2 marks the instantiations for tensors whose stored channel count is not the GEMM's padded one
  // (EfficientNet widths); everywhere else the strides are compile-time equal to Cin / Cout and the checks vanish
  // PERSIST == 3: PADC plus a per-(image, input channel) gate multiplied into the activation operand on its way from the
  // staging registers to LDS (register-staged flavour, 1x1 convs): the squeeze-excitation scaling of an MBConv block
  // applied by the project conv that reads it (spk_set_gate) - x * gate in fp32, rounded to 16 bits, exactly the
  // tensor se_scale_kernel (effnet.hip) would have written and this kernel then read.
  constexpr bool PADC = PERSIST >= 2;
  constexpr bool GATE = PERSIST == 3;
  static_assert(!GATE || (DMA == 0 && MODE == CONV_MODE_GENERIC), "gated operand: register-staged forward conv only");
  const float* const gate = GATE ? (const float*)a.pool_y : nullptr;
  int a_gate[GATE ? A_ITERS : 1];          // gate row of each staged row's image
  f32x4_t rg[GATE ? A_ITERS : 1][2];       // gates of the tile in the staging registers
  const int cin_s = (PADC && a.cin_s > 0) ? a.cin_s : a.Cin;     // channels per stored input pixel
  const int cout_s = (PADC && a.cout_s > 0) ? a.cout_s : a.Cout;  // channels per stored output pixel
  auto set_tile = [&](int w) {
    const int q8 = ntiles >> 3, r8 = ntiles & 7, xcd = w & 7;
    const int swz = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (w >> 3);
    nt_idx = swz % n_tiles;
    mt_idx = swz / n_tiles;
    m0 = mt_idx * BM;
    n0 = nt_idx * BN;
    kr = r_first; ks_ = s_first; kc0 = 0;
    wr = r_first; ws = s_first; wc0 = 0;
#pragma unroll
    for (int i = 0; i < A_ITERS; ++i) {
      const int m = m0 + srow + i * ROWS_PER_PASS;
      const int img = m / HoWo;
      const int rem = m - img * HoWo;
      const int ho = rem / a.Wo;
      const int wo = rem - ho * a.Wo;
      if (MODE == CONV_MODE_STEM) {
        // K row = one filter row: 8 taps x 4 channels starting at pixel 2*wo-4
        const int h0 = ho * 2 - 3, p0 = wo * 2 - 4;
        a_h0[i] = (m < a.M) ? h0 : -(1 << 20);
        a_w0[i] = p0;
        a_base[i] = ((img * a.H + h0) * a.W + p0) * 4;
      } else if (IS_DGRAD) {
        // rows are pixels of the forward conv's INPUT; the "input" tensor is dy.
        // tap (r,s) reads dy[(h+pad-r)/stride][(w+pad-s)/stride] when divisible.
        // stride 2 is decomposed by output parity (cls_ph, cls_pw): the GEMM rows
        // of one launch are the pixels h = 2*ho + ph, w = 2*wo + pw, and only the
        // taps r = (ph+pad)&1, +2, ... can hit them — no MFMA work on taps that
        // never divide.
        const int hh = cls ? 2 * ho + a.cls_ph : ho, ww = cls ? 2 * wo + a.cls_pw : wo;
        a_h0[i] = (m < a.M) ? hh + a.pad : -(1 << 20);
        a_w0[i] = ww + a.pad;
        a_base[i] = img * a.H * a.W * a.Cin + chunk * 8;
      } else {
        const int h0 = ho * a.stride - a.pad, w0 = wo * a.stride - a.pad;
        a_h0[i] = (m < a.M) ? h0 : -(1 << 20);
        a_w0[i] = w0;
        a_base[i] = ((img * a.H + h0) * a.W + w0) * cin_s + chunk * 8;
        if (GATE) a_gate[i] = (img < a.N ? img : a.N - 1) * a.pool_ho;
      }
    }
#pragma unroll
    for (int i = 0; i < B_ITERS; ++i) {
      const int rr = srow + i * ROWS_PER_PASS;  // [0, NB*BN): hi rows then lo rows
      const int half = rr / BN;
      b_off[i] = ((half * a.Cout + n0 + rr - half * BN) * a.K + (DMA ? chunk_b : chunk_a) * 8) * 2;
    }
  };
  int work = blockIdx.x;
  set_tile(work);

  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  int dma_stage = 0;  // LDS stage the next issue_loads() call fills (DMA mode)
  constexpr bool A_LDS = DMA && DMA != 3;  // activations by LDS-DMA (else into registers)
  constexpr bool B_LDS = DMA != 0;         // weights by LDS-DMA
  auto put_a = [&](const __amdgpu_buffer_rsrc_t& rs, unsigned off, u32x4_t& reg, unsigned char* lds_row0) {
    if (A_LDS)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)lds_row0, 16, off, 0, 0, 0);
    else
      reg = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
  };
  auto put_b = [&](const __amdgpu_buffer_rsrc_t& rs, unsigned off, u32x4_t& reg, unsigned char* lds_row0) {
    if (B_LDS)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)lds_row0, 16, off, 0, 0, 0);
    else
      reg = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
  };
  // Activation tile: the next tile of the (kr, ks_, kc0) walk into stage `stage` / registers `ra`.
  // `live` false: the same instructions against a zero-length resource (every lane is range-
  // checked away and reads zeros) - the hybrid loop issues them past the last tile.
  auto issue_a = [&](int kt, u32x4_t (&ra)[A_ITERS], int stage, bool live = true) {
    const __amdgpu_buffer_rsrc_t rs =
        DMA == 3 ? __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, live ? a.x_bytes : 0, 0x00020000) : rx;
    // wave-uniform LDS row of this wave's 8-row piece in pass i: wave*8 + i*ROWS_PER_PASS
    unsigned char* const dA = sA + stage * STAGE_BYTES + wave * (PIECE_ROWS * ROW_BYTES);
    if (MODE == CONV_MODE_STEM) {
      const int krow = kt * 2 + (chunk >> 2);
      const int qq = chunk & 3;
#pragma unroll
      for (int i = 0; i < A_ITERS; ++i) {
        const int hi = a_h0[i] + krow, px = a_w0[i] + 2 * qq;
        const bool ok = (krow < 7) && ((unsigned)hi < (unsigned)a.H) && ((unsigned)px < (unsigned)a.W);
        const unsigned off = ok ? (unsigned)((a_base[i] + (krow * a.W + 2 * qq) * 4) * 2) : 0x80000000u;
        put_a(rs, off, ra[i], dA + i * (ROWS_PER_PASS * ROW_BYTES));
      }
    } else if (IS_DGRAD) {
      const int sh = a.stride == 2 ? 1 : 0;
#pragma unroll
      for (int i = 0; i < A_ITERS; ++i) {
        const int t = a_h0[i] - kr, u = a_w0[i] - ks_;
        const bool ok = (t >= 0) && (u >= 0) && (((t | u) & sh) == 0) && ((t >> sh) < a.H) &&
                        ((u >> sh) < a.W);
        const unsigned off =
            ok ? (unsigned)((a_base[i] + ((t >> sh) * a.W + (u >> sh)) * a.Cin + kc0) * 2) : 0x80000000u;
        put_a(rs, off, ra[i], dA + i * (ROWS_PER_PASS * ROW_BYTES));
      }
      kc0 += BK;
      if (kc0 >= a.Cin) {
        kc0 = 0;
        ks_ += tap_step;
        if (ks_ >= a.kw) { ks_ = s_first; kr += tap_step; }
      }
    } else {
      const int tap_off = (kr * a.W + ks_) * cin_s + kc0;
      const bool chan_ok = !PADC || kc0 + chunk * 8 < cin_s;  // K is padded to 64 per tap, the tensor is not
#pragma unroll
      for (int i = 0; i < A_ITERS; ++i) {
        const bool ok = chan_ok && ((unsigned)(a_h0[i] + kr) < (unsigned)a.H) &&
                        ((unsigned)(a_w0[i] + ks_) < (unsigned)a.W);
        const unsigned off = ok ? (unsigned)((a_base[i] + tap_off) * 2) : 0x80000000u;
        put_a(rs, off, ra[i], dA + i * (ROWS_PER_PASS * ROW_BYTES));
      }
      if (GATE) {
        // (channel chunks past the stored width were loaded as zeros: any gate will do)
        const int gc = kc0 + chunk * 8 < cin_s ? kc0 + chunk * 8 : cin_s - 8;
#pragma unroll
        for (int i = 0; i < A_ITERS; ++i) {
          rg[i][0] = *(const f32x4_t*)(gate + a_gate[i] + gc);
          rg[i][1] = *(const f32x4_t*)(gate + a_gate[i] + gc + 4);
        }
      }
      kc0 += BK;
      if (kc0 >= a.Cin) {
        kc0 = 0;
        if (++ks_ == a.kw) { ks_ = 0; ++kr; }
      }
    }
  };
  // Weight tile kt.  Dgrad walks the taps of the [Cin][kh][kw][Cout] image with its own
  // (wr, ws, wc0) state, so that the two operands of a tile may be issued in different steps.
  auto issue_b = [&](int kt, u32x4_t (&rb)[B_ITERS], int stage, bool live = true) {
    const __amdgpu_buffer_rsrc_t rs =
        DMA == 3 ? __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, live ? a.w_bytes : 0, 0x00020000) : rw;
    unsigned char* const dB = sB + stage * STAGE_BYTES + wave * (PIECE_ROWS * ROW_BYTES);
    int wk = kt * (BK * 2);
    if (IS_DGRAD) {
      wk = ((wr * a.kw + ws) * a.Cin + wc0) * 2;
      wc0 += BK;
      if (wc0 >= a.Cin) {
        wc0 = 0;
        ws += tap_step;
        if (ws >= a.kw) { ws = s_first; wr += tap_step; }
      }
    }
#pragma unroll
    for (int i = 0; i < B_ITERS; ++i)
      put_b(rs, (unsigned)(b_off[i] + wk), rb[i], dB + i * (ROWS_PER_PASS * ROW_BYTES));
  };
  auto issue_loads = [&](int kt, u32x4_t (&ra)[A_ITERS], u32x4_t (&rb)[B_ITERS]) {
    issue_a(kt, ra, dma_stage);
    issue_b(kt, rb, dma_stage);
    if (DMA) dma_stage = dma_stage + 1 == STAGES ? 0 : dma_stage + 1;
  };

  auto store_lds = [&](int buf, const u32x4_t (&ra)[A_ITERS], const u32x4_t (&rb)[B_ITERS]) {
#pragma unroll
    for (int i = 0; i < A_ITERS; ++i) {
      u32x4_t v = ra[i];
      if (GATE) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          v[j] = pack2<DT>(lo_f32<DT>(v[j]) * rg[i][j >> 1][(2 * j) & 3], hi_f32<DT>(v[j]) * rg[i][j >> 1][(2 * j + 1) & 3]);
      }
      *(u32x4_t*)(sA + buf * A_BYTES + lds_off(srow + i * ROWS_PER_PASS, chunk)) = v;
    }
#pragma unroll
    for (int i = 0; i < B_ITERS; ++i)
      *(u32x4_t*)(sB + buf * B_BYTES + lds_off(srow + i * ROWS_PER_PASS, chunk)) = rb[i];
  };

  f32x4_t acc[MT][NT];

  const int frow = lane & 15, fq = lane >> 4;

  auto compute = [&](int buf) {
    const unsigned char* pa = sA + buf * (DMA ? STAGE_BYTES : A_BYTES);
    const unsigned char* pb = sB + buf * (DMA ? STAGE_BYTES : B_BYTES);
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      u32x4_t fa[MT], fb[NT], fl[SPLITW ? NT : 1];
#pragma unroll
      for (int i = 0; i < MT; ++i)
        fa[i] = *(const u32x4_t*)(pa + lds_off(wm * WM + i * 16 + frow, ks * 4 + fq));
#pragma unroll
      for (int j = 0; j < NT; ++j)
        fb[j] = *(const u32x4_t*)(pb + lds_off(wn * WN + j * 16 + frow, ks * 4 + fq));
      if (SPLITW) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
          fl[j] = *(const u32x4_t*)(pb + lds_off(BN + wn * WN + j * 16 + frow, ks * 4 + fq));
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = mfma16<DT>(fa[i], fb[j], acc[i][j]);
      if (SPLITW) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = mfma16<DT>(fa[i], fl[j], acc[i][j]);
      }
    }
  };

  // Register-staged double buffer: the loads of tile kt+1 are issued before
  // tile kt is multiplied out of LDS and written to the other LDS stage after
  // the MFMAs.  (A variant with two tiles in flight in two register sets was
  // measured 10-35 % SLOWER on every ResNet-50 layer as compiled by hipcc 7.2
  // and was removed; deeper pipelining is the job of the LDS-DMA flavour.)
  u32x4_t ra0[A_ITERS], rb0[B_ITERS];
  if (DMA == 3) {
    issue_a(0, ra0, 0);
    issue_b(0, rb0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < A_ITERS; ++i) *(u32x4_t*)(sA + lds_off(srow + i * ROWS_PER_PASS, chunk_a)) = ra0[i];
    issue_a(1, ra0, 0, KT > 1);
  } else if (DMA) {
#pragma unroll
    for (int t = 0; t < STAGES - 1; ++t)
      if (t < KT) issue_loads(t, ra0, rb0);
  } else {
    issue_loads(0, ra0, rb0);
  }

  // GEMM row -> pixel index of the output tensor (identity except for the
  // parity classes of a stride-2 dgrad, whose rows are every other pixel)
  auto out_pixel = [&](int m) -> size_t {
    if (!cls) return (size_t)m;
    const int img = m / HoWo;
    const int rem = m - img * HoWo;
    const int ho = rem / a.Wo;
    const int wo = rem - ho * a.Wo;
    return ((size_t)img * a.oH + 2 * ho + a.cls_ph) * a.oW + 2 * wo + a.cls_pw;
  };

  constexpr int EPI_LD = WN + 4;          // floats per staged row (pad: conflict-free writes)
  constexpr int LPR = WN / 8;             // lanes per output row (8 columns each)
  constexpr int RPP = 64 / LPR;           // rows per pass
  constexpr int PASSES = 16 / RPP;
  static_assert(PASSES >= 1, "WN too large");
  const int ecol = (lane % LPR) * 8;
  const int erow = lane / LPR;
  constexpr bool PREFETCH_RES = MT * PASSES <= 8;
  float* const epi = (float*)smem + wave * (16 * EPI_LD);
  // (with 32-deep K steps K >= 64 means both stages are always allocated)
  static_assert(WARPS_M * WARPS_N * 16 * EPI_LD * 4 <= (BKT == 64 ? 1 : 2) * (A_BYTES + B_BYTES), "epilogue LDS");

  for (;;) {
    // the epilogue of THIS tile runs after the staging coordinates have moved on
    // to the next tile: keep its origin
    const int em0 = m0, emt = mt_idx, en0 = n0;
    const int gcol = en0 + wn * WN + ecol;
    const int next = work + (int)gridDim.x;
    const bool has_next = PERSIST == 1 && !DMA && next < ntiles;

    // epilogue operand prefetch: the shortcut tensor is independent of the K
    // loop, so its loads are issued now and land under the MFMAs
    u32x4_t rres[PREFETCH_RES ? MT : 1][PREFETCH_RES ? PASSES : 1];
    if (PREFETCH_RES && a.res) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
          const int m = em0 + wm * WM + i * 16 + erow + p * RPP;
          rres[i][p] = (m < a.M && (!PADC || gcol < cout_s)) ? *(const u32x4_t*)(a.res + out_pixel(m) * cout_s + gcol)
                                                  : u32x4_t{0, 0, 0, 0};
        }
    }
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    if (DMA == 3) {
      // Hybrid flavour.  Tile kt is multiplied out of LDS stage cs while (a) the weight tile
      // kt+1 streams into the other stage by LDS-DMA, (b) the activation tile kt+1, which
      // landed in registers during the previous step, is stored there between the MFMA rows,
      // and (c) the activation tile kt+2 is fetched into the second register set.
      auto step = [&](int kt, const u32x4_t (&cur)[A_ITERS], u32x4_t (&nxt)[A_ITERS], int cs) {
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // every step issues the same instructions, so that the outstanding-load counts are the
        // same on every path (the compiler's own s_waitcnt placement takes the worst path):
        // past the last tile the loads are dead (range-checked away, zeros)
        issue_b(kt + 1, rb0, cs ^ 1, kt + 1 < KT);
        issue_a(kt + 2, nxt, 0, kt + 2 < KT);
        const unsigned char* pa = sA + cs * STAGE_BYTES;
        const unsigned char* pb = sB + cs * STAGE_BYTES;
        u32x4_t fa[2][MT], fb[2][NT], fl[2][SPLITW ? NT : 1];
#pragma unroll
        for (int i = 0; i < MT; ++i) fa[0][i] = *(const u32x4_t*)(pa + lds_off(wm * WM + i * 16 + frow, fq));
#pragma unroll
        for (int j = 0; j < NT; ++j) fb[0][j] = *(const u32x4_t*)(pb + lds_off(wn * WN + j * 16 + frow, fq));
        if (SPLITW) {
#pragma unroll
          for (int j = 0; j < NT; ++j) fl[0][j] = *(const u32x4_t*)(pb + lds_off(BN + wn * WN + j * 16 + frow, fq));
        }
        // `cur` has landed once only the loads issued in this step are outstanding
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_ITERS + B_ITERS) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        constexpr int NG = 2 * MT;                        // MFMA rows of one K step
        constexpr int NRD = MT + (SPLITW ? 2 : 1) * NT;   // ks = 1 fragment reads
        int piece = 0, rd = 0;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const int ks = g / MT, i = g % MT;
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[i][j] = mfma16<DT>(fa[ks][i], fb[ks][j], acc[i][j]);
          if (SPLITW) {
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = mfma16<DT>(fa[ks][i], fl[ks][j], acc[i][j]);
          }
          if (ks == 0) {  // this row's share of the ks = 1 fragment reads
#pragma unroll
            for (int q = 0; q < (NRD + MT - 1) / MT; ++q, ++rd) {
              if (rd < MT)
                fa[1][rd] = *(const u32x4_t*)(pa + lds_off(wm * WM + rd * 16 + frow, 4 + fq));
              else if (rd < MT + NT)
                fb[1][rd - MT] = *(const u32x4_t*)(pb + lds_off(wn * WN + (rd - MT) * 16 + frow, 4 + fq));
              else if (SPLITW && rd < NRD)
                fl[1][rd - MT - NT] =
                    *(const u32x4_t*)(pb + lds_off(BN + wn * WN + (rd - MT - NT) * 16 + frow, 4 + fq));
            }
          }
          // and of the stores of activation tile kt+1
#pragma unroll
          for (int q = 0; q < (A_ITERS + NG - 1) / NG; ++q, ++piece)
            if (piece < A_ITERS)
              *(u32x4_t*)(sA + (cs ^ 1) * STAGE_BYTES + lds_off(srow + piece * ROWS_PER_PASS, chunk_a)) = cur[piece];
          __builtin_amdgcn_sched_barrier(0);
        }
        // weight tile kt+1 has landed once only the activation loads of tile kt+2 are outstanding
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_ITERS) : "memory");
      };
      u32x4_t ra1[A_ITERS];
      // an odd K-step count runs one dead step (zeros times zeros): the loop body has no branch
      for (int kt = 0; kt < KT; kt += 2) {
        step(kt, ra0, ra1, 0);
        step(kt + 1, ra1, ra0, 1);
      }
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // dead loads/stores of the last step
      __builtin_amdgcn_s_barrier();  // tile buffers are reused by the epilogue
    } else if (DMA == 4) {
      for (int kt = 0; kt < KT; ++kt) {
        if (kt) __builtin_amdgcn_s_barrier();  // every wave is done reading the stage
        issue_loads(kt, ra0, rb0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        compute(0);
      }
      __builtin_amdgcn_s_barrier();  // the tile buffer is reused by the epilogue
    } else if (DMA) {
    // One barrier per K step.  At the top of step kt the wave waits until its own
    // pieces of tile kt have landed (all but the STAGES-2 younger tiles' DMAs
    // retired), the barrier then (a) publishes every wave's pieces of tile kt and
    // (b) proves every wave is done reading tile kt-1, whose stage is refilled at
    // once with tile kt+STAGES-1.
    int cs = 0;  // stage of tile kt
    for (int kt = 0; kt < KT; ++kt) {
      if (kt + STAGES - 2 < KT)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 2) * PER_TILE) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (kt + STAGES - 1 < KT) issue_loads(kt + STAGES - 1, ra0, rb0);
      compute(cs);
      cs = cs + 1 == STAGES ? 0 : cs + 1;
    }
    __builtin_amdgcn_s_barrier();  // tile buffers are reused by the epilogue
    } else if (PERSIST == 3) {
      // one LDS stage (half the LDS: more resident blocks, whose phases overlap), the next tile's global loads in flight
      // in the staging registers while this one is multiplied
      for (int kt = 0; kt < KT; ++kt) {
        store_lds(0, ra0, rb0);
        __syncthreads();
        if (kt + 1 < KT) issue_loads(kt + 1, ra0, rb0);
        compute(0);
        __syncthreads();
      }
    } else {
      store_lds(0, ra0, rb0);
      __syncthreads();
      for (int kt = 0; kt < KT; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < KT) {
          issue_loads(kt + 1, ra0, rb0);
        } else if (has_next) {
          // last K step: start the next tile's first loads; they fly under this
          // tile's MFMAs and its whole epilogue
          set_tile(next);
          issue_loads(0, ra0, rb0);
        }
        compute(buf);
        if (kt + 1 < KT) store_lds(buf ^ 1, ra0, rb0);
        __syncthreads();
      }
    }

    // ---- epilogue: acc -> LDS (fp32, per-wave region) -> fused pointwise -> 16-bit rows ----
    // Each wave stages through its OWN LDS region: LDS operations of one wave
    // execute in order, so no workgroup barrier is needed inside the loop (the
    // K loop's final barrier already retired every read of the tile buffers).
    float sc[8], bi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sc[j] = a.scale ? a.scale[gcol + j] : 1.f;
      bi[j] = a.bias ? a.bias[gcol + j] : 0.f;
    }
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    // dgrad with the BatchNorm-backward reduction of the layer that produced this tensor (spk_set_bnb): sc / bi hold
    // that layer's batch mean / invstd of this lane's 8 channels, a.res_lo is its raw output, a.pool_y its ReLU bits
    constexpr bool bnb = MODE == CONV_MODE_DGRAD_BNB;
    // ... both requested for the whole tile up front: left at their point of use each 16-byte load waited out its own
    // HBM round trip behind the accumulator staging (measured: the fused launches took back what the dropped pass saved)
    u32x4_t rraw[PREFETCH_RES ? MT : 1][PREFETCH_RES ? PASSES : 1];
    unsigned rbit[PREFETCH_RES ? MT : 1][PREFETCH_RES ? PASSES : 1];
    unsigned rbit2[PREFETCH_RES ? MT : 1][PREFETCH_RES ? PASSES : 1];   // ReLU bits of the `res` operand (a.y_lo), see below
    if (PREFETCH_RES && bnb) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
          const int m = em0 + wm * WM + i * 16 + erow + p * RPP;
          const bool ok = m < a.M && (!PADC || gcol < cout_s);
          const size_t o = ok ? out_pixel(m) * cout_s + gcol : 0;
          rraw[PREFETCH_RES ? i : 0][PREFETCH_RES ? p : 0] = ok ? *(const u32x4_t*)(a.res_lo + o) : u32x4_t{0, 0, 0, 0};
          rbit[PREFETCH_RES ? i : 0][PREFETCH_RES ? p : 0] = ok && a.pool_y ? ((const unsigned char*)a.pool_y)[o >> 3] : 0xffu;
          rbit2[PREFETCH_RES ? i : 0][PREFETCH_RES ? p : 0] = ok && a.y_lo ? ((const unsigned char*)a.y_lo)[o >> 3] : 0xffu;
        }
      __builtin_amdgcn_sched_barrier(0);
    }

#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) epi[(fq * 4 + r) * EPI_LD + j * 16 + frow] = acc[i][j][r];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int row = erow + p * RPP;
      const int m = em0 + wm * WM + i * 16 + row;
      const f32x4_t v0 = *(const f32x4_t*)(epi + row * EPI_LD + ecol);
      const f32x4_t v1 = *(const f32x4_t*)(epi + row * EPI_LD + ecol + 4);
      float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      if (m < a.M && (!PADC || gcol < cout_s)) {
        const size_t o = out_pixel(m) * cout_s + gcol;
        if (a.stats && !bnb) {
#pragma unroll
          for (int j = 0; j < 8; ++j) { s1[j] += v[j]; s2[j] += v[j] * v[j]; }
        }
        if (!bnb) {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = v[j] * sc[j] + bi[j];
        }
        if (a.res) {
          const u32x4_t rr = PREFETCH_RES ? rres[PREFETCH_RES ? i : 0][PREFETCH_RES ? p : 0]
                                          : *(const u32x4_t*)(a.res + o);
          if (bnb && a.y_lo) {
            // the `res` operand is the gradient of a LATER layer's output (a block-closing conv whose shortcut is this
            // tensor) and a.y_lo that layer's ReLU bits: res * bit is what its BatchNorm backward would have written into
            // this tensor first - that write (and this launch's read-modify-write of it) is skipped
            const unsigned b2 = PREFETCH_RES ? rbit2[PREFETCH_RES ? i : 0][PREFETCH_RES ? p : 0]
                                             : ((const unsigned char*)a.y_lo)[o >> 3];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              v[2 * j] += (b2 >> (2 * j)) & 1u ? lo_f32<DT>(rr[j]) : 0.f;
              v[2 * j + 1] += (b2 >> (2 * j + 1)) & 1u ? hi_f32<DT>(rr[j]) : 0.f;
            }
          } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[2 * j] += lo_f32<DT>(rr[j]);
            v[2 * j + 1] += hi_f32<DT>(rr[j]);
          }
          }
          if (a.res_lo && !bnb) {  // rounding remainder of the shortcut tensor
            const u32x4_t rl = *(const u32x4_t*)(a.res_lo + o);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              v[2 * j] += lo_f32<DT>(rl[j]);
              v[2 * j + 1] += hi_f32<DT>(rl[j]);
            }
          }
        }
        if (bnb) {   // v = the complete gradient of this element (accumulated contributions included), still fp32
          float rw[8];
          const u32x4_t rq = PREFETCH_RES ? rraw[PREFETCH_RES ? i : 0][PREFETCH_RES ? p : 0] : *(const u32x4_t*)(a.res_lo + o);
#pragma unroll
          for (int j = 0; j < 4; ++j) { rw[2 * j] = lo_f32<DT>(rq[j]); rw[2 * j + 1] = hi_f32<DT>(rq[j]); }
          const unsigned bits = PREFETCH_RES ? rbit[PREFETCH_RES ? i : 0][PREFETCH_RES ? p : 0]
                                             : (a.pool_y ? ((const unsigned char*)a.pool_y)[o >> 3] : 0xffu);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float dz = (bits >> j) & 1u ? v[j] : 0.f;
            s1[j] += dz;
            s2[j] += dz * (rw[j] - sc[j]) * bi[j];
          }
        }
        act_apply<8>(v, a.relu);
        u32x4_t ov;
#pragma unroll
        for (int j = 0; j < 4; ++j) ov[j] = pack2<DT>(v[2 * j], v[2 * j + 1]);
        *(u32x4_t*)(a.y + o) = ov;
        if (a.y_lo && !bnb) {  // what the 16-bit rounding dropped, for the next shortcut add
          u32x4_t lv;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            lv[j] = pack2<DT>(v[2 * j] - lo_f32<DT>(ov[j]), v[2 * j + 1] - hi_f32<DT>(ov[j]));
          *(u32x4_t*)(a.y_lo + o) = lv;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }

  if (a.stats) {
    // per-column partial sums of this block's rows: lanes with equal ecol,
    // then the WARPS_M waves stacked in M (through LDS), fixed order.
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      for (int d = LPR; d < 64; d <<= 1) {
        s1[j] += __shfl_xor(s1[j], d);
        s2[j] += __shfl_xor(s2[j], d);
      }
    }
    __syncthreads();  // every wave is done with its staging region
    float* red = (float*)smem;  // [WARPS_M][2][BN]
    if (erow == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        red[(wm * 2 + 0) * BN + wn * WN + ecol + j] = s1[j];
        red[(wm * 2 + 1) * BN + wn * WN + ecol + j] = s2[j];
      }
    }
    __syncthreads();
    for (int c = tid; c < 2 * BN; c += NTHREADS) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < WARPS_M; ++w) t += red[(w * 2) * BN + c];
      const int which = c / BN, col = c - which * BN;
      a.stats[((size_t)emt * 2 + which) * a.Cout + en0 + col] = t;
    }
  }

    if (!has_next) break;
    work = next;
    __syncthreads();  // staging regions alias the tile buffers the next tile is about to fill
  }
}

// SPK_CONV_DMA=0 selects the register-staged main loop (A/B comparisons)
bool use_dma() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("SPK_CONV_DMA");
    v = e ? atoi(e) != 0 : 1;
  }
  return v != 0;
}

thread_local char g_cfg_name[64] = "";

template <int BM, int BN, int WARPS_M, int WARPS_N, int MODE, int DT, int SPLITW, int DMA, int PERSIST = 0, int BKT = 64>
int launch_one(const ConvArgs& a, hipStream_t s, int m_tiles, int n_tiles) {
  const size_t stage = (size_t)(BM + (SPLITW ? 2 : 1) * BN) * (BKT * 2);
  const int stages = DMA == 4 ? 1 : ((!DMA || DMA >= 2) ? 2 : (stage <= 32768 ? 4 : (stage <= 49152 ? 3 : 2)));
  const size_t lds_full = stages * stage;
  const int kt = a.K / BKT;
  const size_t lds = DMA == 3 ? lds_full : (PERSIST == 3 ? 1 : (kt < stages ? kt : stages)) * stage;  // hybrid: both stages are written
  auto k = conv_igemm_kernel<BM, BN, WARPS_M, WARPS_N, MODE, DT, SPLITW, DMA, PERSIST, BKT>;
  static std::atomic<unsigned long long> attr;
  (void)spk_lds_limit_once(attr, (const void*)k, (int)lds_full);
  int grid = m_tiles * n_tiles;
  if (PERSIST == 1) {
    // persistent: as many blocks as stay resident (LDS-limited, at most 4 per CU)
    int bpc = (int)(163840 / (lds ? lds : 1));
    bpc = bpc < 1 ? 1 : (bpc > 4 ? 4 : bpc);
    if (grid > 256 * bpc) grid = 256 * bpc;
  }
  hipLaunchKernelGGL(k, dim3(grid), dim3(WARPS_M * WARPS_N * 64), lds, s, a, m_tiles, n_tiles);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the hybrid flavour (weights by LDS-DMA, activations through registers) has no stem form
template <int BM, int BN, int WARPS_M, int WARPS_N, int MODE, int DT, int SPLITW>
int launch_hybrid(const ConvArgs& a, hipStream_t s, int m_tiles, int n_tiles) {
  // (256x256 and the 4x1-wave 256x64 tile would need more than 256 VGPRs)
  if constexpr (MODE != CONV_MODE_STEM && BM * BN < 256 * 256 && !(BM == 256 && WARPS_N == 1) &&
                (BM + (SPLITW ? 2 : 1) * BN) * ROW_BYTES * 2 <= 163840)
    return launch_one<BM, BN, WARPS_M, WARPS_N, MODE, DT, SPLITW, 3>(a, s, m_tiles, n_tiles);
  else
    return -3;
}

// 32-deep K steps, LDS-DMA, two stages: half the LDS per block (e.g. 256x128: 48 KB, three blocks per CU)
template <int BM, int BN, int WARPS_M, int WARPS_N, int MODE, int DT, int SPLITW>
int launch_bk32(const ConvArgs& a, hipStream_t s, int m_tiles, int n_tiles) {
  if constexpr (MODE != CONV_MODE_STEM && (WARPS_M * WARPS_N * 64 / 4) % 16 == 0 && BM % (WARPS_M * WARPS_N * 16) == 0 &&
                ((SPLITW ? 2 : 1) * BN) % (WARPS_M * WARPS_N * 16) == 0)
    return launch_one<BM, BN, WARPS_M, WARPS_N, MODE, DT, SPLITW, 2, 0, 32>(a, s, m_tiles, n_tiles);
  else
    return -3;
}

template <int BM, int BN, int WARPS_M, int WARPS_N>
int launch_cfg(const ConvArgs& a, int mode, hipStream_t s, int* m_tiles_out) {
  const int m_tiles = (a.M + BM - 1) / BM;
  const int n_tiles = a.Cout / BN;
  if (m_tiles_out) *m_tiles_out = m_tiles;
  snprintf(g_cfg_name, sizeof g_cfg_name, "%dx%d%s", BM, BN, a.splitw ? "+wlo" : "");
#define SPK_GO(MODE, DT, SW)                                                                   \
  do {                                                                                         \
    if (a.dma >= 0 ? a.dma == 1 : use_dma()) return launch_one<BM, BN, WARPS_M, WARPS_N, MODE, DT, SW, 1>(a, s, m_tiles, n_tiles); \
    if (a.dma == 2) return -3; /* the persistent register-staged flavour never won a layer: not instantiated */ \
    if (a.dma == 3) return launch_one<BM, BN, WARPS_M, WARPS_N, MODE, DT, SW, 2>(a, s, m_tiles, n_tiles); \
    if (a.dma == 4) return launch_hybrid<BM, BN, WARPS_M, WARPS_N, MODE, DT, SW>(a, s, m_tiles, n_tiles); \
    if (a.dma == 5) return launch_bk32<BM, BN, WARPS_M, WARPS_N, MODE, DT, SW>(a, s, m_tiles, n_tiles); \
    if (a.dma == 6) return launch_one<BM, BN, WARPS_M, WARPS_N, MODE, DT, SW, 4>(a, s, m_tiles, n_tiles); \
    return launch_one<BM, BN, WARPS_M, WARPS_N, MODE, DT, SW, 0>(a, s, m_tiles, n_tiles);      \
  } while (0)
  if (mode == CONV_MODE_STEM) {
    if (a.dt == DT_F16) { if (a.splitw) SPK_GO(CONV_MODE_STEM, DT_F16, 1); SPK_GO(CONV_MODE_STEM, DT_F16, 0); }
    SPK_GO(CONV_MODE_STEM, DT_BF16, 0);
  }
  if (mode == CONV_MODE_DGRAD) {
    if (a.stats) SPK_GO(CONV_MODE_DGRAD_BNB, DT_BF16, 0);
    SPK_GO(CONV_MODE_DGRAD, DT_BF16, 0);
  }
  if (a.dt == DT_F16 && a.pool_y) {
    // gated activation operand (spk_set_gate): the register-staged flavour only
    if (a.kh != 1 || a.stride != 1 || a.pad != 0 || spk_conv_padc_flavour(a.dma, true) < 0) return -3;
    if (a.splitw) return launch_one<BM, BN, WARPS_M, WARPS_N, CONV_MODE_GENERIC, DT_F16, 1, 0, 3>(a, s, m_tiles, n_tiles);
    return launch_one<BM, BN, WARPS_M, WARPS_N, CONV_MODE_GENERIC, DT_F16, 0, 0, 3>(a, s, m_tiles, n_tiles);
  }
  if (a.pool_y) return -2;
  if (a.dt == DT_F16 && (a.cin_s > 0 || a.cout_s > 0)) {
    // stored channels != padded GEMM channels: the three flavours instantiated with the channel checks
#define SPK_GO_PAD(SW)                                                                                        \
  do {                                                                                                        \
    const int fl = spk_conv_padc_flavour(a.dma, false);                                                       \
    if (fl == 0) return launch_one<BM, BN, WARPS_M, WARPS_N, CONV_MODE_GENERIC, DT_F16, SW, 0, 2>(a, s, m_tiles, n_tiles); \
    if (fl == 2) return launch_one<BM, BN, WARPS_M, WARPS_N, CONV_MODE_GENERIC, DT_F16, SW, 2, 2>(a, s, m_tiles, n_tiles); \
    if (fl == 4) return launch_one<BM, BN, WARPS_M, WARPS_N, CONV_MODE_GENERIC, DT_F16, SW, 4, 2>(a, s, m_tiles, n_tiles); \
    return -3;                                                                                                \
  } while (0)
    if (a.splitw) SPK_GO_PAD(1);
    SPK_GO_PAD(0);
#undef SPK_GO_PAD
  }
  if (a.cin_s > 0 || a.cout_s > 0) return -2;  // only the fp16 eval path has padded GEMMs
  if (a.dt == DT_F16) { if (a.splitw) SPK_GO(CONV_MODE_GENERIC, DT_F16, 1); SPK_GO(CONV_MODE_GENERIC, DT_F16, 0); }
  SPK_GO(CONV_MODE_GENERIC, DT_BF16, 0);
#undef SPK_GO
}

// tile choice: keep >= ~2 blocks per CU where the problem allows, prefer the
// widest N tile (activations are then streamed once).
int pick_cfg(int M, int Cout) {
  const long blocks128 = (long)((M + 127) / 128) * (Cout / 128 > 0 ? Cout / 128 : 1);
  if (Cout % 128 == 0 && blocks128 >= 512) return 0;  // 128x128
  if (Cout == 64 && M >= 256 * 512) return 1;         // 256x64
  const long blocks12864 = (long)((M + 127) / 128) * (Cout / 64);
  if (blocks12864 >= 384) return 3;                   // 128x64
  return 2;                                           // 64x64
}

}  // namespace

const char* spk_conv_last_config() { return g_cfg_name; }

static int env_cfg() {
  static int v = -2;
  if (v == -2) {
    const char* e = getenv("SPK_CONV_CFG");
    v = e ? atoi(e) : -1;
  }
  return v;
}

int spk_conv_m_tiles(int M, int Cout, int mode) {
  int cfg = env_cfg() >= 0 ? env_cfg() : pick_cfg(M, Cout);
  if (cfg == 5 && Cout % 256) cfg = 4;
  if ((cfg == 0 || cfg == 4) && Cout % 128) cfg = 3;
  const int bm = (cfg == 0 || cfg == 3) ? 128 : ((cfg == 1 || cfg == 4 || cfg == 5 || cfg == 6) ? 256 : 64);
  return (M + bm - 1) / bm;
}

int spk_conv_narrow_cfg(int cfg, int Cout, int splitw) {
  if (cfg == 5 && (Cout % 256 || splitw)) cfg = 4;
  if ((cfg == 0 || cfg == 4) && Cout % 128) cfg = 3;
  return cfg;
}

int spk_conv_padc_flavour(int dma, bool gated) {
  if (gated) return dma == 0 ? 0 : -3;   // gated activation operand: the register-staged flavour only
  if (dma == 0) return 0;                // register-staged
  if (dma < 0 || dma == 3) return 2;     // LDS-DMA, two stages (also the default)
  if (dma == 6) return 4;                // LDS-DMA, one stage
  return -3;
}

static int launch_with(const ConvArgs& a, int mode, int cfg, hipStream_t s, int* m_tiles_out) {
  cfg = spk_conv_narrow_cfg(cfg, a.Cout, a.splitw);
  switch (cfg) {
    case 0: return launch_cfg<128, 128, 2, 2>(a, mode, s, m_tiles_out);
    case 1: return launch_cfg<256, 64, 4, 1>(a, mode, s, m_tiles_out);
    case 3: return launch_cfg<128, 64, 2, 2>(a, mode, s, m_tiles_out);
    case 4: return launch_cfg<256, 128, 4, 2>(a, mode, s, m_tiles_out);
    case 5: return launch_cfg<256, 256, 2, 4>(a, mode, s, m_tiles_out);
    case 6: return launch_cfg<256, 64, 4, 2>(a, mode, s, m_tiles_out);
    default: return launch_cfg<64, 64, 2, 2>(a, mode, s, m_tiles_out);
  }
}

// ---------------------------------------------------------------------------
// Per-problem autotuning (tile config x main-loop flavour), "conv" entries of the tuner table.  The winner differs by
// layer (measured on ResNet-50, batch 256: 128x128 register-staged for the HBM-bound stage-1 layers, 256x256 / 256x128
// LDS-DMA for the deep 3x3 and 1x1 layers), so each distinct problem is timed once on first use.  SPK_AUTOTUNE=0 pins
// the static heuristic.  Every candidate accumulates each output element in the same K order, so results do not
// depend on the choice (only the grouping of the BN partial sums does).
// ---------------------------------------------------------------------------

// Test-hook pin (spk_op_conv_pin): one (tile config, main-loop flavour) for every implicit-GEMM launch of the process
// and one pipeline depth for the weight gradient; -1 = not pinned.  Process-wide, like the tuner's tables.
namespace {
std::atomic<int> g_pin_cfg{-1}, g_pin_dma{-1}, g_pin_wgrad_nbuf{-1};
}  // namespace

void spk_conv_set_pin(int cfg, int dma, int wgrad_nbuf) {
  g_pin_cfg.store(cfg);
  g_pin_dma.store(dma);
  g_pin_wgrad_nbuf.store(wgrad_nbuf);
}

int spk_conv_pinned_wgrad_nbuf() { return g_pin_wgrad_nbuf.load(); }

int spk_conv_launch(const ConvArgs& a_in, int mode, hipStream_t s, int* m_tiles_out) {
  if (a_in.K % BK || a_in.Cout % 64) return -2;
  if (mode == CONV_MODE_DGRAD && a_in.stride != 1 && a_in.cls_ph < 0) return -2;  // stride 2 goes by parity class
  if (mode == CONV_MODE_STEM) {
    // dedicated weights-resident kernel (conv_stem.hip); SPK_STEM_GENERIC=1 forces the implicit GEMM
    static const bool generic = getenv("SPK_STEM_GENERIC") && atoi(getenv("SPK_STEM_GENERIC"));
    if (!generic) {
      const int r = spk_conv_stem_launch(a_in, s, m_tiles_out);
      if (r != -2) return r;
    }
  }
  ConvArgs a = a_in;
  if (const int pin_cfg = g_pin_cfg.load(); pin_cfg >= 0) {
    // pinned: exactly this candidate - no tuner, no tune cache, no fall-back to another flavour (-3: not instantiated)
    a.cfg = pin_cfg;
    a.dma = g_pin_dma.load();
    return launch_with(a, mode, pin_cfg, s, m_tiles_out);
  }
  if (env_cfg() >= 0 || !spk_autotune_on() || a.cfg >= 0) {
    const int cfg = a.cfg >= 0 ? a.cfg : (env_cfg() >= 0 ? env_cfg() : pick_cfg(a.M, a.Cout));
    if (a.dma < 0 && getenv("SPK_CONV_DMA")) a.dma = atoi(getenv("SPK_CONV_DMA"));  // flavour 0..4
    if (mode == CONV_MODE_GENERIC && a.pool_y) a.dma = 0;   // gated operand: one flavour
    const int r = launch_with(a, mode, cfg, s, m_tiles_out);
    if (r != -3) return r;
    a.dma = 3;  // the forced flavour does not exist for this tile
    return launch_with(a, mode, cfg, s, m_tiles_out);
  }
  const int pad_cls = a.pad * 16 + (a.cls_ph >= 0 ? 1 + a.cls_ph * 2 + a.cls_pw : 0);
  const int key[] = {mode, a.dt, a.splitw, a.N, a.H, a.W, a.Cin, a.Cout, a.kh, a.stride, pad_cls, a.stats != nullptr,
                     (a.res != nullptr && (const void*)a.res != (const void*)a.y) + 2 * (a.cin_s > 0) + 4 * (a.cout_s > 0) + 8 * (mode == CONV_MODE_GENERIC && a.pool_y != nullptr)};
  int win[2];   // tile config, main-loop flavour
  const TuneTag tag = spk_tune_tag(TUNE_CONV);   // (the forward convs of a two-stream eval forward: "conv_p", timed as pairs)
  if (!spk_tune_find(tag, key, win)) {
    // in-place accumulation (dgrad into an existing gradient): re-running it would add twice, so the candidates
    // write to a scratch tensor and read the real one as their shortcut operand - same traffic, nothing clobbered
    bf16_t* scratch = nullptr;
    bf16_t* const real_y = a.y;
    if ((const void*)a.res == (const void*)a.y && a.res) {
      const size_t pixels = a.cls_ph >= 0 ? (size_t)a.N * a.oH * a.oW : (size_t)a.M;
      if (hipMalloc((void**)&scratch, pixels * a.Cout * 2) != hipSuccess)
        return launch_with(a, mode, pick_cfg(a.M, a.Cout), s, m_tiles_out);
      a.y = scratch;
    }
    SpkLaunchTimer timer;
    if (!timer.ok) {
      if (scratch) (void)hipFree(scratch);
      return -1;
    }
    float best = 1e30f;
    win[0] = pick_cfg(a.M, a.Cout);
    win[1] = 0;
    const SpkPair<ConvArgs> pair(a);
    const bool twin_ok = pair.ok && (mode == CONV_MODE_GENERIC || mode == CONV_MODE_STEM);
    const int cands[] = {0, 1, 2, 3, 4, 5, 6};
    for (int cfg : cands) {
      const int bn = cfg == 5 ? 256 : ((cfg == 0 || cfg == 4) ? 128 : 64);
      const int bm = (cfg == 0 || cfg == 3) ? 128 : (cfg == 2 ? 64 : 256);
      if (a.Cout % bn) continue;
      if (cfg == 5 && a.splitw) continue;
      if (cfg == 1 && a.Cout != 64) continue;
      // would leave most CUs idle: fewer than 64 M tiles AND fewer than 128 blocks in all (the 7 x 7 layers of a half
      // batch - 6272 pixels x 512 / 2048 couts - get their 128-row tiles timed: 196 / 784 blocks)
      if (bm > 64 && a.M < bm * 64 && (long)((a.M + bm - 1) / bm) * (a.Cout / bn) < 128) continue;
      // 0 register-staged, 1 LDS-DMA, 2 register-staged persistent, 3 LDS-DMA 2-stage, 4 hybrid, 5 LDS-DMA 2-stage BK 32, 6 LDS-DMA 1 stage
      for (int dma = (cfg == 6 ? 3 : 0); dma < 7; ++dma) {
        if (dma == 2) continue;  // 5: LDS-DMA 2-stage, 32-deep K steps; 6: LDS-DMA 1 stage
        a.dma = dma;
        if (launch_with(a, mode, cfg, s, nullptr)) continue;  // warm-up
        float ms = 0.f;
        auto run = [&](int i, hipStream_t st) {
          ConvArgs h = pair[i];
          h.dma = dma;
          return launch_with(h, mode, cfg, st, nullptr);
        };
        if (!timer.time(s, 3, twin_ok, run, &ms)) continue;
        if (spk_tune_log() > 1)
          fprintf(stderr, "[spk cand] %dx%d C%d->%d k%d s%d sw%d: cfg %d dma %d %.1f us\n", a.H, a.W, a.Cin, a.Cout,
                  a.kh, a.stride, a.splitw, cfg, dma, ms * 1000.f / 3.f);
        if (ms < best) { best = ms; win[0] = cfg; win[1] = dma; }
      }
    }
    if (scratch) {
      (void)hipStreamSynchronize(s);
      (void)hipFree(scratch);
      a.y = real_y;
    }
    spk_tune_store(tag, key, win, true);
    if (spk_tune_log())
      fprintf(stderr, "[spk tune] mode %d dt %d sw %d N%d %dx%d C%d->%d k%d s%d: cfg %d dma %d (%.1f us)\n", mode,
              a.dt, a.splitw, a.N, a.H, a.W, a.Cin, a.Cout, a.kh, a.stride, win[0], win[1], best * 1000.f / 3.f);
  }
  a.dma = win[1];
  return launch_with(a, mode, win[0], s, m_tiles_out);
}
