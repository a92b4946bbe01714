// Grouped 3x3 convolution (torchvision ResNeXt bottleneck conv2: Conv2d(C, C, 3, stride, 1, groups=g, bias=False)).
// NHWC 16-bit activations, fp32 weights in the model's master layout [C][3][3][C/g] (the state_dict's [C][C/g][3][3] with
// the input channel innermost, as every conv's master copy is kept), fp32 accumulation.
//
// Per group the GEMM is M = N*Ho*Wo, N = C/g, K = 9*C/g: 36..576 for the widths ResNeXt has.  At 4-32 channels per group
// an MFMA tile would be mostly zeros, and the layer moves as many bytes as a dense 1x1 conv of the same width while doing a
// fraction of its arithmetic: these kernels are direct convolutions on the VALU with the block's weights staged in LDS
// and the activations read through the L1 / L2 caches (every input element is re-read by the 9 taps of its neighbours).
//   forward: a thread computes 4 adjacent output channels of one pixel (one group: C/g is a multiple of 4); a block holds
//            64 pixels x 16 channels.  Eval: folded BatchNorm scale / shift (+ ReLU); training: the raw conv output.
//   dgrad:   the same loop over the output gradient with the per-group transposed weights (stride 2: only the taps
//            whose output position is integral).
//   wgrad:   a block sums one fixed chunk of pixels for 16 output channels into a slab; the slabs are reduced in a
//            fixed order (train_kernels.hip slab_reduce), so the result does not depend on scheduling.
// Every output is one fixed-order sum over its own taps and channels: a row's result does not depend on the batch it
// runs in, nor on the tile sizes, which depend on the channel count per group only.
#include "spk_common.h"

#include <algorithm>

namespace {

constexpr int GB_PIX = 64;   // forward / dgrad: pixels per block
constexpr int GB_CH = 16;    // channels per block
constexpr int GW_PIX = 16;   // wgrad: pixels per LDS stage

template <int DT>
__device__ __forceinline__ void load4(const bf16_t* p, float v[4]) {
  const u32x2_t u = *(const u32x2_t*)p;
  v[0] = lo_f32<DT>(u.x); v[1] = hi_f32<DT>(u.x);
  v[2] = lo_f32<DT>(u.y); v[3] = hi_f32<DT>(u.y);
}

// y[m][c] = act(scale[c] * sum_{tap, ci} x[tap(m)][g(c) * CPG + ci] * w[c][tap][ci] + bias[c]); scale == nullptr: raw sum
template <int DT, int CPG>
__global__ void __launch_bounds__(256) group_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ scale, const float* __restrict__ bias,
                                                        bf16_t* __restrict__ y, int N, int H, int W, int C, int Ho,
                                                        int Wo, int stride, int relu) {
  __shared__ __attribute__((aligned(16))) float ws[GB_CH * 9 * CPG];   // [channel of the block][tap][ci]
  const int c_blk = blockIdx.y * GB_CH;
  for (int i = threadIdx.x; i < GB_CH * 9 * CPG; i += 256) {
    const int cl = i / (9 * CPG), r = i - cl * 9 * CPG, tap = r / CPG, ci = r - tap * CPG;
    ws[i] = w[((size_t)(c_blk + cl) * 9 + tap) * CPG + ci];
  }
  __syncthreads();
  const int q = threadIdx.x & 3;
  const int64_t mi = (int64_t)blockIdx.x * GB_PIX + (threadIdx.x >> 2);
  const int64_t M = (int64_t)N * Ho * Wo;
  if (mi >= M) return;
  const int ox = (int)(mi % Wo);
  const int oy = (int)((mi / Wo) % Ho);
  const int n = (int)(mi / ((int64_t)Wo * Ho));
  const int c0 = c_blk + q * 4;
  const int cbase = c0 / CPG * CPG;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const float* wq = ws + q * 4 * 9 * CPG;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy * stride - 1 + ky;
    if (iy < 0 || iy >= H) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ox * stride - 1 + kx;
      if (ix < 0 || ix >= W) continue;
      const bf16_t* px = x + (((size_t)n * H + iy) * W + ix) * C + cbase;
      const int tap = ky * 3 + kx;
#pragma unroll 4
      for (int c4 = 0; c4 < CPG; c4 += 4) {
        float v[4];
        load4<DT>(px + c4, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4_t wv = *(const f32x4_t*)(wq + j * 9 * CPG + tap * CPG + c4);
          acc[j] = fmaf(v[0], wv.x, acc[j]);
          acc[j] = fmaf(v[1], wv.y, acc[j]);
          acc[j] = fmaf(v[2], wv.z, acc[j]);
          acc[j] = fmaf(v[3], wv.w, acc[j]);
        }
      }
    }
  }
  if (scale) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[j] = fmaf(acc[j], scale[c0 + j], bias[c0 + j]);
      if (relu) acc[j] = fmaxf(acc[j], 0.f);
    }
  }
  u32x2_t o;
  o.x = pack2<DT>(acc[0], acc[1]);
  o.y = pack2<DT>(acc[2], acc[3]);
  *(u32x2_t*)(y + (size_t)mi * C + c0) = o;
}

// dx[m][c] (+)= sum_{tap, co in g(c)} dy[out(m, tap)][co] * w[co][tap][c - g(c) * CPG]
template <int DT, int CPG>
__global__ void __launch_bounds__(256) group_dgrad_kernel(const bf16_t* __restrict__ dy, const float* __restrict__ w,
                                                          bf16_t* __restrict__ dx, int accumulate, int N, int H, int W,
                                                          int C, int Ho, int Wo, int stride) {
  __shared__ __attribute__((aligned(16))) float ws[GB_CH * 9 * CPG];   // [input channel of the block][tap][co of its group]
  const int c_blk = blockIdx.y * GB_CH;
  for (int i = threadIdx.x; i < GB_CH * 9 * CPG; i += 256) {
    const int cl = i / (9 * CPG), r = i - cl * 9 * CPG, tap = r / CPG, col = r - tap * CPG;
    const int c = c_blk + cl;
    const int co = c / CPG * CPG + col;
    ws[i] = w[((size_t)co * 9 + tap) * CPG + (c % CPG)];
  }
  __syncthreads();
  const int q = threadIdx.x & 3;
  const int64_t mi = (int64_t)blockIdx.x * GB_PIX + (threadIdx.x >> 2);
  const int64_t M = (int64_t)N * H * W;
  if (mi >= M) return;
  const int ix = (int)(mi % W);
  const int iy = (int)((mi / W) % H);
  const int n = (int)(mi / ((int64_t)W * H));
  const int c0 = c_blk + q * 4;
  const int cobase = c0 / CPG * CPG;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const float* wq = ws + q * 4 * 9 * CPG;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int ty = iy + 1 - ky;
    if (ty < 0 || ty % stride) continue;
    const int oy = ty / stride;
    if (oy >= Ho) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int tx = ix + 1 - kx;
      if (tx < 0 || tx % stride) continue;
      const int ox = tx / stride;
      if (ox >= Wo) continue;
      const bf16_t* pg = dy + (((size_t)n * Ho + oy) * Wo + ox) * C + cobase;
      const int tap = ky * 3 + kx;
#pragma unroll 4
      for (int c4 = 0; c4 < CPG; c4 += 4) {
        float v[4];
        load4<DT>(pg + c4, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4_t wv = *(const f32x4_t*)(wq + j * 9 * CPG + tap * CPG + c4);
          acc[j] = fmaf(v[0], wv.x, acc[j]);
          acc[j] = fmaf(v[1], wv.y, acc[j]);
          acc[j] = fmaf(v[2], wv.z, acc[j]);
          acc[j] = fmaf(v[3], wv.w, acc[j]);
        }
      }
    }
  }
  bf16_t* pd = dx + (size_t)mi * C + c0;
  if (accumulate) {
    float v[4];
    load4<DT>(pd, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += v[j];
  }
  u32x2_t o;
  o.x = pack2<DT>(acc[0], acc[1]);
  o.y = pack2<DT>(acc[2], acc[3]);
  *(u32x2_t*)pd = o;
}

// slabs[chunk][c][tap][ci] = sum over the chunk's output pixels m of dy[m][c] * x[in(m, tap)][g(c) * CPG + ci]
template <int DT, int CPG>
__global__ void __launch_bounds__(256) group_wgrad_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                          float* __restrict__ slabs, int N, int H, int W, int C, int Ho,
                                                          int Wo, int stride, int pix_per_chunk) {
  constexpr int CT = CPG > GB_CH ? CPG : GB_CH;        // input channels one block of 16 output channels reads
  constexpr int NE = (GB_CH * 9 * CPG + 255) / 256;    // weight elements per thread
  __shared__ float dys[GW_PIX * GB_CH];
  __shared__ __attribute__((aligned(16))) float xs[GW_PIX * 9 * CT];
  const int c_blk = blockIdx.y * GB_CH;
  const int ci_base = c_blk / CT * CT;
  int xo[NE], co[NE];
  float acc[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    const int e = threadIdx.x + k * 256;   // [co of the block][tap][ci], the slab's own order
    const int cl = e / (9 * CPG), r = e - cl * 9 * CPG, tap = r / CPG, ci = r - tap * CPG;
    co[k] = e < GB_CH * 9 * CPG ? cl : 0;
    xo[k] = e < GB_CH * 9 * CPG ? tap * CT + ((c_blk + cl) / CPG * CPG - ci_base) + ci : 0;
    acc[k] = 0.f;
  }
  const int64_t M = (int64_t)N * Ho * Wo;
  const int64_t m0 = (int64_t)blockIdx.x * pix_per_chunk;
  const int64_t m1 = m0 + pix_per_chunk < M ? m0 + pix_per_chunk : M;
  for (int64_t ms = m0; ms < m1; ms += GW_PIX) {
    {
      const int p = threadIdx.x / GB_CH, cl = threadIdx.x % GB_CH;
      const int64_t mi = ms + p;
      float v = 0.f;
      if (mi < m1) {
        const bf16_t u = dy[(size_t)mi * C + c_blk + cl];
        v = DT == DT_BF16 ? bf16_to_f32(u) : (float)__builtin_bit_cast(_Float16, u);
      }
      dys[threadIdx.x] = v;
    }
    for (int i = threadIdx.x; i < GW_PIX * 9 * (CT / 4); i += 256) {
      const int p = i / (9 * (CT / 4)), r = i - p * 9 * (CT / 4), tap = r / (CT / 4), c4 = (r - tap * (CT / 4)) * 4;
      const int64_t mi = ms + p;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (mi < m1) {
        const int ox = (int)(mi % Wo);
        const int oy = (int)((mi / Wo) % Ho);
        const int n = (int)(mi / ((int64_t)Wo * Ho));
        const int iy = oy * stride - 1 + tap / 3, ix = ox * stride - 1 + tap % 3;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) load4<DT>(x + (((size_t)n * H + iy) * W + ix) * C + ci_base + c4, v);
      }
      *(f32x4_t*)(xs + (p * 9 + tap) * CT + c4) = f32x4_t{v[0], v[1], v[2], v[3]};
    }
    __syncthreads();
#pragma unroll 2
    for (int p = 0; p < GW_PIX; ++p) {
#pragma unroll
      for (int k = 0; k < NE; ++k) acc[k] = fmaf(dys[p * GB_CH + co[k]], xs[p * 9 * CT + xo[k]], acc[k]);
    }
    __syncthreads();
  }
  float* out = slabs + (size_t)blockIdx.x * C * 9 * CPG + (size_t)c_blk * 9 * CPG;
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    const int e = threadIdx.x + k * 256;
    if (e < GB_CH * 9 * CPG) out[e] = acc[k];
  }
}

template <int DT>
int fwd_dispatch(int cpg, dim3 g, hipStream_t s, const bf16_t* x, const float* w, const float* sc, const float* bi,
                 bf16_t* y, int N, int H, int W, int C, int Ho, int Wo, int stride, int relu) {
#define SPK_GFWD(P) case P: hipLaunchKernelGGL((group_fwd_kernel<DT, P>), g, dim3(256), 0, s, x, w, sc, bi, y, N, H, W, C, Ho, Wo, stride, relu); break;
  switch (cpg) { SPK_GFWD(4) SPK_GFWD(8) SPK_GFWD(16) SPK_GFWD(32) SPK_GFWD(64) default: return -3; }
#undef SPK_GFWD
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int DT>
int dgrad_dispatch(int cpg, dim3 g, hipStream_t s, const bf16_t* dy, const float* w, bf16_t* dx, int acc, int N, int H,
                   int W, int C, int Ho, int Wo, int stride) {
#define SPK_GDG(P) case P: hipLaunchKernelGGL((group_dgrad_kernel<DT, P>), g, dim3(256), 0, s, dy, w, dx, acc, N, H, W, C, Ho, Wo, stride); break;
  switch (cpg) { SPK_GDG(4) SPK_GDG(8) SPK_GDG(16) SPK_GDG(32) SPK_GDG(64) default: return -3; }
#undef SPK_GDG
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int DT>
int wgrad_dispatch(int cpg, dim3 g, hipStream_t s, const bf16_t* x, const bf16_t* dy, float* slabs, int N, int H, int W,
                   int C, int Ho, int Wo, int stride, int ppc) {
#define SPK_GWG(P) case P: hipLaunchKernelGGL((group_wgrad_kernel<DT, P>), g, dim3(256), 0, s, x, dy, slabs, N, H, W, C, Ho, Wo, stride, ppc); break;
  switch (cpg) { SPK_GWG(4) SPK_GWG(8) SPK_GWG(16) SPK_GWG(32) SPK_GWG(64) default: return -3; }
#undef SPK_GWG
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

bool spk_group_conv_ok(int c, int groups, int k, int stride, int pad) {
  if (groups < 2 || c % groups || k != 3 || pad != 1 || (stride != 1 && stride != 2) || c % GB_CH) return false;
  const int cpg = c / groups;
  return cpg == 4 || cpg == 8 || cpg == 16 || cpg == 32 || cpg == 64;
}

static int out_size(int i, int stride) { return (i - 1) / stride + 1; }   // k 3, pad 1

int spk_launch_group_fwd(const bf16_t* x, const float* w, const float* scale, const float* bias, bf16_t* y, int n, int h,
                         int wd, int c, int groups, int stride, int relu, int dt, hipStream_t s) {
  if (!spk_group_conv_ok(c, groups, 3, stride, 1)) return -3;
  const int ho = out_size(h, stride), wo = out_size(wd, stride);
  const int64_t M = (int64_t)n * ho * wo;
  const dim3 g((unsigned)((M + GB_PIX - 1) / GB_PIX), (unsigned)(c / GB_CH));
  return dt == DT_BF16 ? fwd_dispatch<DT_BF16>(c / groups, g, s, x, w, scale, bias, y, n, h, wd, c, ho, wo, stride, relu)
                       : fwd_dispatch<DT_F16>(c / groups, g, s, x, w, scale, bias, y, n, h, wd, c, ho, wo, stride, relu);
}

int spk_launch_group_dgrad(const bf16_t* dy, const float* w, bf16_t* dx, bool accumulate, int n, int h, int wd, int c,
                           int groups, int stride, int dt, hipStream_t s) {
  if (!spk_group_conv_ok(c, groups, 3, stride, 1)) return -3;
  const int ho = out_size(h, stride), wo = out_size(wd, stride);
  const int64_t M = (int64_t)n * h * wd;
  const dim3 g((unsigned)((M + GB_PIX - 1) / GB_PIX), (unsigned)(c / GB_CH));
  return dt == DT_BF16 ? dgrad_dispatch<DT_BF16>(c / groups, g, s, dy, w, dx, accumulate, n, h, wd, c, ho, wo, stride)
                       : dgrad_dispatch<DT_F16>(c / groups, g, s, dy, w, dx, accumulate, n, h, wd, c, ho, wo, stride);
}

// Pixel chunks of the weight gradient: ~256 output pixels each, at most 2^24 slab floats in all; a function of the
// problem's shape only (the reduction order is fixed for a shape).
int spk_group_wgrad_chunks(int64_t M, int c, int groups, int* pix_per_chunk) {
  const int64_t per = (int64_t)c * 9 * (c / groups);
  int64_t chunks = (M + 255) / 256;
  const int64_t cap = std::max<int64_t>(1, ((int64_t)1 << 24) / per);
  if (chunks > cap) chunks = cap;
  int64_t ppc = (M + chunks - 1) / chunks;
  ppc = (ppc + GW_PIX - 1) / GW_PIX * GW_PIX;
  chunks = (M + ppc - 1) / ppc;
  if (pix_per_chunk) *pix_per_chunk = (int)ppc;
  return (int)chunks;
}

size_t spk_group_wgrad_slab_floats(int64_t M, int c, int groups) {
  return (size_t)spk_group_wgrad_chunks(M, c, groups, nullptr) * c * 9 * (c / groups);
}

// slabs: spk_group_wgrad_slab_floats(M, c, groups) floats; *chunks = slab count for spk_launch_slab_reduce
int spk_launch_group_wgrad(const bf16_t* x, const bf16_t* dy, float* slabs, int n, int h, int wd, int c, int groups,
                           int stride, int dt, int* chunks, hipStream_t s) {
  if (!spk_group_conv_ok(c, groups, 3, stride, 1)) return -3;
  const int ho = out_size(h, stride), wo = out_size(wd, stride);
  const int64_t M = (int64_t)n * ho * wo;
  int ppc = 0;
  *chunks = spk_group_wgrad_chunks(M, c, groups, &ppc);
  const dim3 g((unsigned)*chunks, (unsigned)(c / GB_CH));
  return dt == DT_BF16 ? wgrad_dispatch<DT_BF16>(c / groups, g, s, x, dy, slabs, n, h, wd, c, ho, wo, stride, ppc)
                       : wgrad_dispatch<DT_F16>(c / groups, g, s, x, dy, slabs, n, h, wd, c, ho, wo, stride, ppc);
}
