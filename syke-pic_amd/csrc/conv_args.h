// Host-only builders of the dense conv kernels' argument descriptors (spk_common.h: ConvArgs, PwConvArgs, C3Args,
// BneckArgs).  What goes into a launch is written here once: the eval executor (model.hip), the training step (train.hip),
// the single-operator hooks (ops_abi.hip) and the sanitizer driver (asan_driver.hip) resolve their pointers and shapes and
// call these, so a hook's parity test judges the extents and padding rules the executor runs with.  Plain functions of
// pointers and shapes: nothing here knows a model, a layer or a cursor.
#pragma once
#include "spk_common.h"
#include <string.h>

// A buffer-resource extent: the one narrowing of a byte count to the descriptors' 32 bits.  The kernels clamp against
// these and mark "no such element" with bit 31 of a 32-bit offset, so every operand of a launch must stay below 2 GiB
// (spk_below_2gib).  A count past 32 bits saturates: it must not wrap to a small extent that passes for a valid one.
static inline unsigned int spk_extent(size_t bytes) { return bytes > 0xffffffffull ? 0xffffffffu : (unsigned int)bytes; }

// The shape of one dense conv launch.
struct ConvGeom {
  int N, H, W, Cs;     // input as stored: W is the row pitch in pixels, Cs the channels per pixel in HBM
  int Ho, Wo, Cos;     // output as stored
  int Cin, Cout, K;    // the GEMM: channel counts (64-padded where the stored ones are not), reduction length
  int k, stride, pad;
};
// stored channels = GEMM channels, K = k * k * cin
static inline ConvGeom spk_conv_geom(int n, int h, int w, int cin, int cout, int k, int stride, int pad) {
  return {n, h, w, cin, (h + 2 * pad - k) / stride + 1, (w + 2 * pad - k) / stride + 1, cout, cin, cout, k * k * cin,
          k, stride, pad};
}
// the 7x7 stride-2 stem on an image of width w: 4 stored channels, an even row pitch (zero pad column), K padded to 256
static inline ConvGeom spk_stem_geom(int n, int h, int w) {
  return {n, h, (w + 1) & ~1, 4, (h - 1) / 2 + 1, (w - 1) / 2 + 1, 64, 4, 64, 256, 7, 2, 3};
}

// The implicit GEMM's arguments: what every dense form starts from.  Everything not named here is zero (no remainder
// tensors, statistics, pooling, gate or parity class); tile and main loop are left to the tuner.
static inline ConvArgs spk_conv_args(const ConvGeom& g, const bf16_t* x, const bf16_t* w, bf16_t* y, const bf16_t* res,
                                     const float* scale, const float* bias, int relu, int dt, int splitw) {
  ConvArgs a;
  memset(&a, 0, sizeof a);
  a.cfg = a.dma = a.cls_ph = a.cls_pw = -1;
  a.x = x; a.w = w; a.y = y; a.res = res; a.scale = scale; a.bias = bias;
  a.N = g.N; a.H = g.H; a.W = g.W; a.Cin = g.Cin; a.Ho = g.Ho; a.Wo = g.Wo; a.Cout = g.Cout;
  a.cin_s = g.Cs != g.Cin ? g.Cs : 0;       // EfficientNet: tensors are not padded, the GEMM is
  a.cout_s = g.Cos != g.Cout ? g.Cos : 0;
  a.kh = a.kw = g.k; a.stride = g.stride; a.pad = g.pad;
  a.M = g.N * g.Ho * g.Wo; a.K = g.K;
  a.relu = relu; a.dt = dt; a.splitw = splitw;
  a.x_bytes = spk_extent((size_t)g.N * g.H * g.W * g.Cs * 2);
  a.w_bytes = spk_extent((size_t)g.Cout * g.K * 2 * (splitw ? 2 : 1));
  return a;
}

// the same conv for conv_pw.hip / conv_pwr.hip (wp: its fragment-ordered weights) ...
static inline PwConvArgs pw_args(const ConvArgs& a, const bf16_t* wp) {
  PwConvArgs q;
  memset(&q, 0, sizeof q);
  q.x = a.x; q.wp = wp; q.y = a.y; q.res = a.res; q.scale = a.scale; q.shift = a.bias;
  q.N = a.N; q.H = a.H; q.W = a.W; q.Ho = a.Ho; q.Wo = a.Wo; q.stride = a.stride;
  q.Cin = a.Cin; q.Cout = a.Cout; q.M = a.M; q.relu = a.relu; q.dt = DT_F16; q.nb = a.splitw ? 2 : 1;
  q.x_bytes = a.x_bytes; q.y_bytes = spk_extent((size_t)a.M * a.Cout * 2);
  return q;
}
// ... and for conv_c3.hip / conv_d3.hip (nbw weight images at wp)
static inline C3Args c3_args(const ConvArgs& a, const bf16_t* wp, int nbw) {
  C3Args q;
  memset(&q, 0, sizeof q);
  q.x = a.x; q.wp = wp; q.y = a.y; q.scale = a.scale; q.shift = a.bias; q.res = a.res;
  q.N = a.N; q.H = a.H; q.W = a.W; q.Cin = a.Cin; q.Cout = a.Cout; q.M = a.M; q.relu = a.relu; q.dt = DT_F16;
  q.nb = nbw;
  q.x_bytes = a.x_bytes; q.y_bytes = spk_extent((size_t)a.M * a.Cout * 2);
  q.wp_bytes = spk_extent((size_t)a.Cout * 9 * a.Cin * 2 * q.nb);
  return q;
}

// the second activation source of a K-concatenated GEMM: x2 [N,H2,W2,Cin2], read through stride2
static inline void spk_pw_set_second(PwConvArgs& q, const bf16_t* x2, int Cin2, int H2, int W2, int stride2) {
  q.x2 = x2; q.Cin2 = Cin2; q.H2 = H2; q.W2 = W2; q.stride2 = stride2;
  q.x2_bytes = spk_extent((size_t)q.N * H2 * W2 * Cin2 * 2);
}
// the chained conv: z [N,Ho,Wo,Coutz] from the output tile of q
static inline void spk_pw_set_chain(PwConvArgs& q, const bf16_t* wpz, bf16_t* z, const float* scalez, const float* shiftz,
                                    int Coutz, int reluz) {
  q.wpz = wpz; q.z = z; q.scalez = scalez; q.shiftz = shiftz; q.Coutz = Coutz; q.reluz = reluz;
  q.z_bytes = spk_extent((size_t)q.M * Coutz * 2);
}

// a whole identity bottleneck of CM mid channels (4 CM trunk channels); y1, flags and stamps are the caller's
static inline BneckArgs spk_bneck_args(const bf16_t* x, bf16_t* y, const bf16_t* w1, const bf16_t* w2, const bf16_t* w3,
                                       const float* s1, const float* b1, const float* s2, const float* b2, const float* s3,
                                       const float* b3, int N, int H, int W, int CM) {
  BneckArgs a;
  memset(&a, 0, sizeof a);
  a.x = x; a.y = y; a.w1 = w1; a.w2 = w2; a.w3 = w3;
  a.s1 = s1; a.b1 = b1; a.s2 = s2; a.b2 = b2; a.s3 = s3; a.b3 = b3;
  a.N = N; a.H = H; a.W = W; a.C4 = 4 * CM; a.CM = CM;
  a.x_bytes = spk_extent((size_t)N * H * W * a.C4 * 2);
  return a;
}
// spk_btail_launch's chained conv (ReLU behind it): z [N,H,W,Coutz]
static inline void spk_bneck_set_chain(BneckArgs& a, const bf16_t* wz, bf16_t* z, const float* sz, const float* bz, int Coutz) {
  a.wz = wz; a.z = z; a.sz = sz; a.bz = bz; a.Coutz = Coutz;
  a.z_bytes = spk_extent((size_t)a.N * a.H * a.W * Coutz * 2);
}

// every operand of the launch below 2 GiB?  (ConvArgs carries no output extent: M pixels of the stored channels.)
static inline bool spk_below_2gib(unsigned int a, unsigned int b = 0, unsigned int c = 0, unsigned int d = 0) {
  return (a | b | c | d) < 0x80000000u;
}
static inline bool spk_below_2gib(const ConvArgs& a) {
  return spk_below_2gib(a.x_bytes, a.w_bytes, spk_extent((size_t)a.M * (a.cout_s ? a.cout_s : a.Cout) * 2));
}
static inline bool spk_below_2gib(const PwConvArgs& q) { return spk_below_2gib(q.x_bytes, q.y_bytes, q.x2_bytes, q.z_bytes); }
static inline bool spk_below_2gib(const C3Args& q) { return spk_below_2gib(q.x_bytes, q.y_bytes, q.wp_bytes); }
static inline bool spk_below_2gib(const BneckArgs& a) { return spk_below_2gib(a.x_bytes, a.z_bytes); }
