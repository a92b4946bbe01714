// Classifier head on gfx950: the reference's head is a stack of Linear
// layers with NO activation between them (sykepic/train/network.py:58-63,
// quirk Q1), then either the base-1.3 softmax of net_pass
// (sykepic/compute/probability.py:191-194) or CrossEntropyLoss
// (sykepic/train/train.py:127,241).  The head is 0.01 % of the FLOPs, so it
// stays in exact fp32 (LDS-tiled FMA GEMM) — this keeps the logits' error
// budget for the bf16 backbone.
#include "spk_common.h"
#include <cstdlib>

namespace {

// C[i][j] = sum_k A(i,k) * B(j,k) (+ bias[j]);  A(i,k) = A[i*sai + k*sak], B likewise.
// 64x64 tile, 256 threads, 4x4 outputs per thread, K step 16.
__global__ __launch_bounds__(256) void sgemm_strided_kernel(
    const float* __restrict__ A, long sai, long sak, const float* __restrict__ B, long sbj, long sbk,
    const float* __restrict__ bias, float* __restrict__ C, long sci, long scj, int M, int N, int K) {
  __shared__ float sa[16][64 + 4];
  __shared__ float sb[16][64 + 4];
  const int tid = threadIdx.x;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  const int ty = tid >> 4, tx = tid & 15;
  float acc[4][4] = {};
  for (int k0 = 0; k0 < K; k0 += 16) {
    for (int e = tid; e < 64 * 16; e += 256) {
      // choose the element order so the fastest-varying global index is contiguous
      int r, kk;
      if (sak == 1) { kk = e & 15; r = e >> 4; } else { r = e & 63; kk = e >> 6; }
      const int gi = i0 + r, gk = k0 + kk;
      sa[kk][r] = (gi < M && gk < K) ? A[gi * sai + gk * sak] : 0.f;
    }
    for (int e = tid; e < 64 * 16; e += 256) {
      int r, kk;
      if (sbk == 1) { kk = e & 15; r = e >> 4; } else { r = e & 63; kk = e >> 6; }
      const int gj = j0 + r, gk = k0 + kk;
      sb[kk][r] = (gj < N && gk < K) ? B[gj * sbj + gk * sbk] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      float av[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { av[u] = sa[kk][ty * 4 + u]; bv[u] = sb[kk][tx * 4 + u]; }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(av[u], bv[v], acc[u][v]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int gi = i0 + ty * 4 + u;
    if (gi >= M) continue;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int gj = j0 + tx * 4 + v;
      if (gj >= N) continue;
      C[gi * sci + gj * scj] = acc[u][v] + (bias ? bias[gj] : 0.f);
    }
  }
}

// The same product on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32: an fmaf chain per output, k ascending) for ANY strides:
// a wave owns a 16 x 16 output tile, a block 2 x 2 of them; per 4-deep K step a lane supplies ONE element of each operand
// (row lane & 15, k = k0 + (lane >> 4)) - with a unit stride along the rows (the weight-gradient form: A = dY^T, B = X^T,
// K = the batch) the 16 lanes of a k read 64 contiguous bytes.  Eight K steps of loads in flight.  The head's backward
// GEMMs (2048 x 256 x 256 and smaller) took 37 us each on the LDS-tiled FMA kernel above, 0.22 ms of a ResNet-50 step.
__global__ __launch_bounds__(256) void sgemm_mfma_strided_kernel(
    const float* __restrict__ A, long sai, long sak, const float* __restrict__ B, long sbj, long sbk,
    const float* __restrict__ bias, float* __restrict__ C, long sci, long scj, int M, int N, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.y * 32 + (wave >> 1) * 16, j0 = blockIdx.x * 32 + (wave & 1) * 16;
  if (i0 >= M || j0 >= N) return;
  const float* pa = A + (long)min(i0 + r, M - 1) * sai;   // (rows past the edge: clamped, their outputs are not stored)
  const float* pb = B + (long)min(j0 + r, N - 1) * sbj;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  constexpr int U = 8;
  for (int k0 = 0; k0 < K; k0 += 4 * U) {
    float va[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + 4 * u + g;
      const bool ok = k < K;
      const int kc = ok ? k : K - 1;
      va[u] = pa[(long)kc * sak];
      vb[u] = pb[(long)kc * sbk];
      if (!ok) va[u] = 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(va[u], vb[u], acc, 0, 0, 0);
  }
  // C layout: col = lane & 15, row = (lane >> 4) * 4 + reg
  const int gj = j0 + r;
  if (gj >= N) return;
  const float bj = bias ? bias[gj] : 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int gi = i0 + g * 4 + e;
    if (gi >= M) continue;
    C[gi * sci + gj * scj] = acc[e] + bj;
  }
}

// y[n][out] = x[n][in] . w[out][in]^T + b with the exact-fp32 MFMA
// (v_mfma_f32_16x16x4_f32: bitwise an fmaf chain).  One 16x16 output tile per
// block, K split over the 4 waves and summed through LDS in fixed order.
// Operand trick: each lane loads a float4 (k = k0 + 4*(lane>>4) + 0..3) of its
// row; MFMA step s consumes element s of every lane, i.e. the k-set
// {k0+s, k0+4+s, k0+8+s, k0+12+s} — the same set for A and B, any order sums.
__global__ __launch_bounds__(256) void linear_mfma_kernel(const float* __restrict__ x,
                                                          const float* __restrict__ w,
                                                          const float* __restrict__ b,
                                                          float* __restrict__ y, int n, int in,
                                                          int out) {
  __shared__ float red[4][16][17];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
  const int r = lane & 15, g = lane >> 4;
  const int ai = min(i0 + r, n - 1), bj = min(j0 + r, out - 1);  // clamp: extra rows discarded
  const float* pa = x + (size_t)ai * in;
  const float* pb = w + (size_t)bj * in;
  const int kper = ((in + 63) / 64) * 16;  // per-wave K range, multiple of 16
  const int kbeg = wave * kper, kend = min(in, kbeg + kper);
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = kbeg; k0 < kend; k0 += 16) {
    const int k = k0 + 4 * g;
    f32x4_t va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
    if (k + 3 < kend) {
      va = *(const f32x4_t*)(pa + k);
      vb = *(const f32x4_t*)(pb + k);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k + e < kend) { va[e] = pa[k + e]; vb[e] = pb[k + e]; }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(va[e], vb[e], acc, 0, 0, 0);
  }
  // C layout: col = lane&15, row = (lane>>4)*4 + reg
#pragma unroll
  for (int e = 0; e < 4; ++e) red[wave][g * 4 + e][r] = acc[e];
  __syncthreads();
  const int t = threadIdx.x;
  const int ri = t >> 4, cj = t & 15;
  const int gi = i0 + ri, gj = j0 + cj;
  if (gi < n && gj < out)
    y[(size_t)gi * out + gj] = ((red[0][ri][cj] + red[1][ri][cj]) + (red[2][ri][cj] + red[3][ri][cj])) +
                               (b ? b[gj] : 0.f);
}

__device__ __forceinline__ float wave_max(float v) {
  for (int d = 32; d; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// one wave per row: p = softmax(z * scale)
__global__ void softmax_kernel(const float* __restrict__ z, float* __restrict__ p, int n, int c,
                               float scale) {
  // No contraction in this body: `zr[j] * scale - mx` as one fma subtracts the ROUNDED maximum from the UNROUNDED
  // product, so the maximum's own exponent was not 0 and a row of equal logits did not come out as 1 / c
  // (tests/test_gpu_head_pool_ops.py).  The product is rounded in all three passes, as in the max pass.
#pragma clang fp contract(off)
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const float* zr = z + (size_t)row * c;
  float mx = -INFINITY;
  for (int j = lane; j < c; j += 64) mx = fmaxf(mx, zr[j] * scale);
  mx = wave_max(mx);
  float s = 0.f;
  for (int j = lane; j < c; j += 64) s += expf(zr[j] * scale - mx);
  s = wave_sum(s);
  const float inv = 1.0f / s;
  for (int j = lane; j < c; j += 64) p[(size_t)row * c + j] = expf(zr[j] * scale - mx) * inv;
}

// The cross-entropy loss: ce_loss_kernel<EX, PAIR, KD> below, assembled from the pieces in front of it.  ONE block, a row
// per wave at a time (4 waves walked 64 rows each, one latency chain per row: 92 us), so that every float sum has a fixed
// order - a thread's own terms in ascending index, the xor butterfly of a wave, then the 16 waves in ascending order - and
// equal inputs give equal bits; the only atomics are the integer adds of the per-class counters.
constexpr int CE_WAVES = 16;

// the per-wave partial sums of one quantity, in ascending wave order (after a __syncthreads)
__device__ __forceinline__ float sum_waves(const float* part) {
  float t = 0.f;
  for (int q = 0; q < CE_WAVES; ++q) t += part[q];
  return t;
}

// The label-weight sums W_a = sum_i w[ya_i] (PAIR: W_b = sum_i w[yb_i] too) and Sw = sum_c w[c], in one pass over the labels
// in front of the row loop; every thread ends with the same bits.  w == nullptr: all ones, the caller's W = n, Sw = c stand.
template <bool PAIR>
__device__ __forceinline__ void label_weight_sums(const float* w, const int64_t* ya, const int64_t* yb, int n, int c,
                                                  float* s_wa, float* s_wb, float& Wa, float& Wb, float& Sw) {
  if (!w) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float pa = 0.f, pb = 0.f;
  for (int i = threadIdx.x; i < n; i += CE_WAVES * 64) {
    pa += w[(int)ya[i]];
    if constexpr (PAIR) pb += w[(int)yb[i]];
  }
  pa = wave_sum(pa);
  if constexpr (PAIR) pb = wave_sum(pb);
  if (lane == 0) { s_wa[wave] = pa; if constexpr (PAIR) s_wb[wave] = pb; }
  __syncthreads();
  Wa = sum_waves(s_wa);
  if constexpr (PAIR) Wb = sum_waves(s_wb);
  float sp = 0.f;
  for (int j = lane; j < c; j += 64) sp += w[j];
  Sw = wave_sum(sp);
}

// the maximum of a row and its index: a lane takes its elements in ascending index, then the wave reduces
struct RowArgMax {
  float mx = -INFINITY;
  int arg = 0x7fffffff;
  __device__ __forceinline__ void take(float v, int j) { if (v > mx) { mx = v; arg = j; } }
};
// arg-max with torch's tie rule: lowest index among the maxima.  N rows share the steps of one butterfly: a step is a
// round trip through the cross-lane network, and a second butterfly behind the first doubled the wait (+2 us with a teacher).
template <int N>
__device__ __forceinline__ void reduce(RowArgMax (&m)[N]) {
  for (int d = 32; d; d >>= 1) {
    float om[N];
    int oa[N];
    for (int k = 0; k < N; ++k) om[k] = __shfl_xor(m[k].mx, d);
    for (int k = 0; k < N; ++k) oa[k] = __shfl_xor(m[k].arg, d);
    for (int k = 0; k < N; ++k)
      if (om[k] > m[k].mx || (om[k] == m[k].mx && oa[k] < m[k].arg)) { m[k].mx = om[k]; m[k].arg = oa[k]; }
  }
}

// The soft-max of a row about its maximum mx: s = sum_j exp(v_j - mx), lse = mx + log s, p_j = exp(v_j - mx) / s.  For a
// temperature the caller hands in the quotients v_j / T and mx / T, each logit divided by T once (a correctly rounded
// division; T = 1 leaves the bits).  T > 0 and a correctly rounded division are monotone, so the quotient of the maximum
// is the maximum of the quotients; and a quotient is rounded before the maximum is subtracted - a division does not
// contract - so the largest exponent is exactly 0, which softmax_kernel needs a pragma for.
struct RowSoftmax {
  float mx, s = 0.f;
  __device__ __forceinline__ void add(float v) { s += expf(v - mx); }
  __device__ __forceinline__ void reduce() { s = wave_sum(s); }
  __device__ __forceinline__ float lse() const { return mx + logf(s); }
  __device__ __forceinline__ float inv() const { return 1.0f / s; }
  __device__ __forceinline__ float p(float v, float inv) const { return expf(v - mx) * inv; }
};

// The smoothing sum of a row, sum_j w[j] (lse - z[j]), formed term by term: lse Sw - sum w z would cancel.
__device__ __forceinline__ float smoothing_sum(const float* zr, const float* w, int c, float lse) {
  float sm = 0.f;
  for (int j = threadIdx.x & 63; j < c; j += 64) sm += (w ? w[j] : 1.f) * (lse - zr[j]);
  return wave_sum(sm);
}

// The weighted, smoothed row loss aw (lse - z[label]) + b sm of one label before the division by W: aw = (1 - eps) w[label],
// b = eps / c.  FUSED: one fused multiply-add onto the rounded b sm; else both products and their sum are rounded.  Which
// of the two the compiler made of this one expression hung on how it packed a kernel's statistics - fused, except for the
// first label of two - and is pinned here because the statistics are kept bit for bit.
template <bool FUSED>
__device__ __forceinline__ float hard_row_loss(float aw, float lse, float zl, float b, float sm) {
#pragma clang fp contract(off)
  const float d = lse - zl, bs = b * sm;
  if constexpr (FUSED) return fmaf(aw, d, bs);
  return aw * d + bs;
}

// ... and the gradient of that label's loss at class j, ca = aw / W, without its smoothing term
__device__ __forceinline__ float hard_grad(float ca, float p, int j, int label) {
  return ca * (p - (j == label ? 1.f : 0.f));
}

// the per-class counters [c][2] (may be null) += (rows, correct rows) of the row's dominant label
__device__ __forceinline__ void count_row(int* counts, int c, int label, bool hit) {
  if (counts && (unsigned)label < (unsigned)c) {
    atomicAdd(counts + 2 * label, 1);
    if (hit) atomicAdd(counts + 2 * label + 1, 1);
  }
}

// Mean cross-entropy + arg-max accuracy + dlogits, in five instantiations.
// plain (EX false): nn.CrossEntropyLoss(), the reference's loss.  stats[0] += sum_i (lse_i - z[i][y_i]) (the caller's
// running sum of loss * n), dz = (p - onehot) / n.  No weights, no smoothing, no counters: w, eps and counts are not read.
// EX: F.cross_entropy(z, y, weight = w, label_smoothing = eps, reduction = "mean") with the same fused extras.  With
// p = softmax(z_i), W = sum_i w[y_i], Sw = sum_c w[c]:
//   loss     = [ (1 - eps) sum_i w[y_i] (lse_i - z[i][y_i]) + (eps / c) sum_i sum_j w[j] (lse_i - z[i][j]) ] / W
//   dz[i][j] = [ (1 - eps) w[y_i] (p[i][j] - [j == y_i]) + (eps / c) (p[i][j] Sw - w[j]) ] / W
// w == nullptr: all ones.  stats[0] += n loss (the reference accumulates loss.item() * len(y)), stats[1] += rows whose
// arg-max is the label; counts [c][2] (may be null) += per class (rows, correct rows).
// PAIR: the Mixup / CutMix criterion on two label vectors, L = lam CE(z, ya; w, eps) + (1 - lam) CE(z, yb; w, eps), each
// CE the loss above with its own W.  Per row the soft-max, lse and the smoothing sum are computed once; the two row
// losses and the two gradients are formed by the same pieces as the single label's (hard_row_loss says where one of them
// rounds a product more), each with its own label and 1 / W, and only combined at the end:
//   dz[i][j]  = lam g_a + (1 - lam) g_b,       stats[0] += lam (n CE_a) + (1 - lam) (n CE_b),    1 - lam formed in float32
// so the extra roundings over one label are the two products, 1 - lam and the sum (tests/test_gpu_loss_pair_ops.py); no
// combined smoothing coefficient is formed.  stats[1] and the counters go by the dominant label: ya when lam >= 0.5, else yb.
// KD: knowledge distillation, L = (1 - alpha) L_hard + alpha KD against the logits t [n][c] of a teacher, with
//   KD = T^2 / n  sum_i KL(q_i || pT_i),   pT = softmax(z / T),   q = softmax(t / T)       ("batchmean")
//   dz[i][j] = (1 - alpha) g_hard[i][j] + (alpha T / n) (pT[i][j] - q[i][j])
// L_hard is the loss of one label vector or of two (PAIR), and the hard row losses and g_hard are complete before anything
// is combined, so their rounding bounds carry over (tests/test_gpu_distill_ops.py).  Per row three soft-maxes: of z (the
// hard part), of z / T and of t / T.  The KD row sum is formed term by term as
//   q[j] ((t[j] / T - lseT_t) - (z[j] / T - lseT_z)):
// q log q is never formed, a q that underflows to 0 contributes exactly 0, and a row whose two soft-maxes sit on
// different classes gives the finite difference of the logits.
//   stats[0] += (1 - alpha) (n L_hard) + alpha (n KD),  n KD = (T T) sum of the KD rows,  1 - alpha formed in float32
//   kd_stats (may be null): [0] += n KD, [1] += rows whose arg-max of z equals the arg-max of t (the same tie rule)
// What a mode does not need it does not form: `if constexpr`, never arithmetic with neutral elements, so each
// instantiation's float expressions are those of its mode alone and the launcher's fall-throughs are bit for bit.
template <bool EX, bool PAIR, bool KD>
__global__ __launch_bounds__(1024) void ce_loss_kernel(const float* __restrict__ z, const int64_t* __restrict__ ya,
                                                      const int64_t* __restrict__ yb, float lam,
                                                      const float* __restrict__ tz, float alpha, float T, int n, int c,
                                                      const float* __restrict__ w, float eps, float* __restrict__ stats,
                                                      int* __restrict__ counts, float* __restrict__ kd_stats,
                                                      float* __restrict__ dz) {
  static_assert(EX || (!PAIR && !KD), "the plain loss has one label vector and no teacher");
  // (an array that an instantiation does not use takes no LDS in it)
  __shared__ float s_wa[CE_WAVES];
  __shared__ float s_wb[CE_WAVES];
  __shared__ float s_la[CE_WAVES];
  __shared__ float s_lb[CE_WAVES];
  __shared__ float s_corr[CE_WAVES];
  __shared__ float s_kd[CE_WAVES];
  __shared__ float s_agree[CE_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float Wa = (float)n, Wb = (float)n, Sw = (float)c;
  if constexpr (EX) label_weight_sums<PAIR>(w, ya, yb, n, c, s_wa, s_wb, Wa, Wb, Sw);
  const bool smooth = EX && eps > 0.f;
  const bool first = !PAIR || lam >= 0.5f;   // the dominant label
  const float invn = 1.0f / (float)n;        // plain
  const float invWa = 1.0f / Wa, invWb = 1.0f / Wb;
  const float a = 1.0f - eps, b = eps / (float)c;
  const float cba = b * invWa, cbb = b * invWb;
  const float lamb = 1.0f - lam;
  const float hard = 1.0f - alpha;           // the weight of the hard part
  const float ck = alpha * T / (float)n;     // the coefficient of pT - q
  float loss_a = 0.f, loss_b = 0.f, corr = 0.f, kd = 0.f, agree = 0.f;
  for (int row = wave; row < n; row += CE_WAVES) {
    const float* zr = z + (size_t)row * c;
    const float* tr = KD ? tz + (size_t)row * c : nullptr;
    const int la = (int)ya[row];
    int lb = la;
    if constexpr (PAIR) lb = (int)yb[row];
    RowArgMax m[KD ? 2 : 1];   // of z and, at [KD], of the teacher's row
    for (int j = lane; j < c; j += 64) {
      m[0].take(zr[j], j);
      if constexpr (KD) m[KD].take(tr[j], j);
    }
    reduce(m);
    const RowArgMax mz = m[0], mt = m[KD];
    RowSoftmax sz{mz.mx}, szT{mz.mx / T}, stT{mt.mx / T};
    for (int j = lane; j < c; j += 64) {
      sz.add(zr[j]);
      if constexpr (KD) { szT.add(zr[j] / T); stT.add(tr[j] / T); }
    }
    sz.reduce();
    const float lse = sz.lse();
    float lsez = 0.f, lset = 0.f, invz = 0.f, invt = 0.f;
    if constexpr (KD) {
      szT.reduce(), stT.reduce();
      lsez = szT.lse(), lset = stT.lse(), invz = szT.inv(), invt = stT.inv();
    }
    float sm = 0.f;
    if (smooth) sm = smoothing_sum(zr, w, c, lse);
    float kr = 0.f;
    if constexpr (KD) {
      for (int j = lane; j < c; j += 64) {
        const float q = stT.p(tr[j] / T, invt);
        kr += q * ((tr[j] / T - lset) - (zr[j] / T - lsez));
      }
      kr = wave_sum(kr);
    }
    const float awa = a * (w ? w[la] : 1.f), awb = a * (w ? w[lb] : 1.f);   // EX
    if (lane == 0) {
      const int label = first ? la : lb;
      const bool hit = mz.arg == label;
      corr += hit ? 1.f : 0.f;
      if constexpr (!EX) {
        loss_a += lse - zr[la];
      } else {
        loss_a += hard_row_loss<!PAIR>(awa, lse, zr[la], b, sm);
        if constexpr (PAIR) loss_b += hard_row_loss<true>(awb, lse, zr[lb], b, sm);
        count_row(counts, c, label, hit);
      }
      if constexpr (KD) { kd += kr; agree += (mz.arg == mt.arg) ? 1.f : 0.f; }
    }
    if (dz) {
      const float inv = sz.inv();
      const float caa = awa * invWa, cab = awb * invWb;   // EX
      for (int j = lane; j < c; j += 64) {
        const float p = sz.p(zr[j], inv);
        float g;
        if constexpr (!EX) {
          g = (p - (j == la ? 1.f : 0.f)) * invn;
        } else {
          g = hard_grad(caa, p, j, la);
          float gb = 0.f;
          if constexpr (PAIR) gb = hard_grad(cab, p, j, lb);
          if (smooth) {
            const float t = p * Sw - (w ? w[j] : 1.f);
            g += cba * t;
            if constexpr (PAIR) gb += cbb * t;
          }
          if constexpr (PAIR) g = lam * g + lamb * gb;
        }
        if constexpr (KD) {
          const float pT = szT.p(zr[j] / T, invz);
          const float q = stT.p(tr[j] / T, invt);
          g = hard * g + ck * (pT - q);
        }
        dz[(size_t)row * c + j] = g;
      }
    }
  }
  if (lane == 0) {
    s_la[wave] = loss_a;
    s_corr[wave] = corr;
    if constexpr (PAIR) s_lb[wave] = loss_b;
    if constexpr (KD) { s_kd[wave] = kd; s_agree[wave] = agree; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {   // fixed order
    // Every product and sum of the combine is rounded on its own, as the tests count them: left to the compiler, whether
    // lam A + (1 - lam) B or (1 - alpha) H + alpha KD became a fused multiply-add hung on how it packed the two statistics.
#pragma clang fp contract(off)
    float nloss = sum_waves(s_la);                       // plain: the sum of the row losses is n loss
    if constexpr (EX) nloss = nloss * invWa * (float)n;
    if constexpr (PAIR) nloss = lam * nloss + lamb * (sum_waves(s_lb) * invWb * (float)n);
    float nkd = 0.f;
    if constexpr (KD) {
      nkd = (T * T) * sum_waves(s_kd);
      nloss = hard * nloss + alpha * nkd;
    }
    stats[0] += nloss;
    stats[1] += sum_waves(s_corr);
    if constexpr (KD) {
      if (kd_stats) { kd_stats[0] += nkd; kd_stats[1] += sum_waves(s_agree); }
    }
  }
}

// SURVEY.md §8f rank 2 — per-ROI prediction from probabilities and per-class
// thresholds (reference sykepic/compute/prediction.py:49-71): the
// highest-probability class that clears ITS OWN threshold wins (lowest index on
// ties); if none does, arg-max with classified = 0.  thr == nullptr: scalar
// rule, classified = p[argmax] > scalar_thr.  One wave per row.
__global__ void predict_kernel(const float* __restrict__ p, int n, int c, const float* __restrict__ thr,
                               float scalar_thr, int* __restrict__ pred, unsigned char* __restrict__ ok) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const float* pr = p + (size_t)row * c;
  float best = -1.f, bestq = -1.f;
  int arg = 0x7fffffff, argq = 0x7fffffff;
  for (int j = lane; j < c; j += 64) {
    const float v = pr[j];
    if (v > best) { best = v; arg = j; }
    if (thr && v >= thr[j] && v > bestq) { bestq = v; argq = j; }
  }
  for (int d = 32; d; d >>= 1) {
    const float ob = __shfl_xor(best, d), oq = __shfl_xor(bestq, d);
    const int oa = __shfl_xor(arg, d), oaq = __shfl_xor(argq, d);
    if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    if (oq > bestq || (oq == bestq && oaq < argq)) { bestq = oq; argq = oaq; }
  }
  if (lane == 0) {
    if (thr) {
      const bool any = argq != 0x7fffffff;
      pred[row] = any ? argq : arg;
      ok[row] = any ? 1 : 0;
    } else {
      pred[row] = arg;
      ok[row] = best > scalar_thr ? 1 : 0;
    }
  }
}

}  // namespace

int spk_launch_predict(const float* p, int n, int c, const float* thr, float scalar_thr, int* pred,
                       unsigned char* ok, hipStream_t s) {
  hipLaunchKernelGGL(predict_kernel, dim3((n + 3) / 4), dim3(256), 0, s, p, n, c, thr, scalar_thr, pred, ok);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int spk_launch_sgemm_form(const float* A, long sai, long sak, const float* B, long sbj, long sbk,
                          const float* bias, float* C, long sci, long scj, int M, int N, int K, bool fma,
                          hipStream_t s) {
  if (!fma) {
    hipLaunchKernelGGL(sgemm_mfma_strided_kernel, dim3((N + 31) / 32, (M + 31) / 32), dim3(256), 0, s, A, sai, sak, B, sbj, sbk,
                       bias, C, sci, scj, M, N, K);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  }
  dim3 grid((N + 63) / 64, (M + 63) / 64);
  hipLaunchKernelGGL(sgemm_strided_kernel, grid, dim3(256), 0, s, A, sai, sak, B, sbj, sbk, bias, C,
                     sci, scj, M, N, K);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int spk_launch_sgemm(const float* A, long sai, long sak, const float* B, long sbj, long sbk,
                     const float* bias, float* C, long sci, long scj, int M, int N, int K, hipStream_t s) {
  static const bool fma = getenv("SPK_SGEMM_FMA") && atoi(getenv("SPK_SGEMM_FMA")) != 0;   // the LDS-tiled FMA kernel (A/B runs)
  return spk_launch_sgemm_form(A, sai, sak, B, sbj, sbk, bias, C, sci, scj, M, N, K, fma, s);
}

// Backward of y = x . w^T + b for one Linear layer: the launches of a training step (and of spk_op_linear_backward).
// dw [out][in], db [out], dx [n][in]: a null pointer skips that gradient.  form < 0: the kernel spk_launch_sgemm picks,
// 0 the MFMA kernel, 1 the FMA kernel.
int spk_linear_backward(const float* gy, const float* x, const float* w, float* dw, float* db, float* dx, int n, int in,
                        int out, int form, hipStream_t s) {
  auto gemm = [&](const float* A, long sai, long sak, const float* B, long sbj, long sbk, float* C, int M, int N, int K) {
    return form < 0 ? spk_launch_sgemm(A, sai, sak, B, sbj, sbk, nullptr, C, N, 1, M, N, K, s)
                    : spk_launch_sgemm_form(A, sai, sak, B, sbj, sbk, nullptr, C, N, 1, M, N, K, form != 0, s);
  };
  if (dw && gemm(gy, 1, out, x, 1, in, dw, out, in, n)) return -1;   // dW[o][i] = sum_n gy[n][o] * x[n][i]
  if (db && spk_launch_colsum(gy, db, n, out, s)) return -1;
  if (dx && gemm(gy, out, 1, w, 1, in, dx, n, in, out)) return -1;   // dX[n][i] = sum_o gy[n][o] * W[o][i]
  return 0;
}

int spk_launch_linear_fwd(const float* x, const float* w, const float* b, float* y, int n, int in,
                          int out, hipStream_t s) {
  // y[n][out] = x[n][in] . w[out][in]^T + b
  if (in % 4) return spk_launch_sgemm(x, in, 1, w, in, 1, b, y, out, 1, n, out, in, s);
  hipLaunchKernelGGL(linear_mfma_kernel, dim3((out + 15) / 16, (n + 15) / 16), dim3(256), 0, s, x, w, b,
                     y, n, in, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int spk_launch_softmax(const float* z, float* p, int n, int c, float scale, hipStream_t s) {
  hipLaunchKernelGGL(softmax_kernel, dim3((n + 3) / 4), dim3(256), 0, s, z, p, n, c, scale);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The one way to the loss kernel.  The fall-throughs are bit for bit because the instantiation that a rule picks does not
// form what the rule found missing: no teacher or alpha == 0 -> no KD (the teacher is not read, kd_stats not written);
// then no yb or lam == 1 -> no pair.  plain is the caller's word alone, never inferred from w and eps.
int spk_launch_ce(const CeArgs& a, hipStream_t s) {
  const bool kd = a.teacher && a.alpha != 0.0f;
  const bool pair = a.yb && a.lam != 1.0f;
  auto kernel = a.plain ? ce_loss_kernel<false, false, false>
                : kd    ? (pair ? ce_loss_kernel<true, true, true> : ce_loss_kernel<true, false, true>)
                        : (pair ? ce_loss_kernel<true, true, false> : ce_loss_kernel<true, false, false>);
  hipLaunchKernelGGL(kernel, dim3(1), dim3(CE_WAVES * 64), 0, s, a.z, a.ya, a.yb, a.lam, a.teacher, a.alpha, a.T, a.n, a.c,
                     a.w, a.eps, a.stats, a.counts, a.kd_stats, a.dz);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
