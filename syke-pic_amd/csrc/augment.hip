// Training augmentations on the GPU: the per-sample random transforms the
// reference applies with cv2 in its DataLoader workers (sykepic/train/image.py:80-180 through
// Compose.__call__, image.py:25-56) - flip H/V, translate, zoom, rotate, brightness - on a batch of
// already resized+bordered uint8 NHWC images.  The random draws stay on the host (Python's `random`, in the
// reference's call order, so a seeded run augments exactly like the host pipeline); the kernels apply them.
// Arithmetic replicates sykepic_hip/preprocess.py byte for byte (integer / double without FMA contraction);
// every op rounds to uint8 like the host does between transforms.  One launch per op over the whole batch.
#include "../../include/sykepic_hip.h"
#include "resize_u8.h"

#include <string>

void spk_set_error(const std::string& s);

namespace {

__device__ __forceinline__ int tap_u8(const unsigned char* img, int h, int w, int c, int ch, long long yy,
                                      long long xx, int border) {
  return (yy >= 0 && yy < h && xx >= 0 && xx < w) ? img[((size_t)yy * w + xx) * c + ch] : border;
}

// grid (pixel chunks, n); one thread = one pixel, all channels
__global__ __launch_bounds__(256) void augment_kernel(const unsigned char* __restrict__ in,
                                                      unsigned char* __restrict__ out, int h, int w, int c,
                                                      const spk_aug_op* __restrict__ ops,
                                                      const unsigned char* __restrict__ border) {
#pragma clang fp contract(off)  // numpy evaluates a*x + b*y + c with separate roundings
  const int img = blockIdx.y;
  const spk_aug_op op = ops[img];
  const unsigned char* src = in + (size_t)img * h * w * c;
  unsigned char* dst = out + (size_t)img * h * w * c;
  const unsigned char* bv = border + (size_t)img * 4;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < h * w; p += gridDim.x * blockDim.x) {
    const int y = p / w, x = p - y * w;
    for (int ch = 0; ch < c; ++ch) {
      int v;
      switch (op.kind) {
        case SPK_AUG_FLIP_H: v = src[((size_t)y * w + (op.i0 ? w - 1 - x : x)) * c + ch]; break;
        case SPK_AUG_FLIP_V: v = src[((size_t)(op.i0 ? h - 1 - y : y) * w + x) * c + ch]; break;
        case SPK_AUG_TRANSLATE:  // dst(x, y) = src(x - tx, y - ty), constant border
          // cv2.warpAffine with an integer shift lands on table entry (0,0): weights 32767 on the pixel and 1 on its
          // lower-right neighbour -> (32767 a + b + 16384) >> 15 = a for 8-bit a, b: an exact copy
          v = tap_u8(src, h, w, c, ch, (long long)y - op.i1, (long long)x - op.i0, bv[ch]);
          break;
        case SPK_AUG_ZOOM: {  // cv2.resize(img, None, fx=f, fy=f) to i0 x i0 (source coordinates with scale 1/f),
                              // then centred pad (f < 1) or crop; square images
          const int z = op.i0;
          const double sc = 1.0 / op.d[0];
          if (op.d[0] < 1.0) {
            const int p1 = (w - z) / 2;  // int((w - zw) / 2), non-negative
            const int ry = y - p1, rx = x - p1;
            v = (ry >= 0 && ry < z && rx >= 0 && rx < z) ? resize_u8_at(src + ch, c, w, h, z, z, sc, sc, rx, ry) : bv[ch];
          } else {
            const int c1 = (z - w) / 2;  // int((zw - w) / 2)
            v = resize_u8_at(src + ch, c, w, h, z, z, sc, sc, x + c1, y + c1);
          }
          break;
        }
        case SPK_AUG_ROTATE:  // cv2.warpAffine through the inverted matrix d[0..5] (resize_u8.h), constant border
          v = warp_affine_u8_at(src, h, w, c, ch, op.d, x, y, bv[ch]);
          break;
        case SPK_AUG_BRIGHT: {  // (img * v).clip(0, 255).astype(uint8): truncation
          const double o = (double)src[((size_t)y * w + x) * c + ch] * op.d[0];
          v = (int)fmin(fmax(o, 0.0), 255.0);
          break;
        }
        default: v = src[((size_t)y * w + x) * c + ch]; break;
      }
      dst[((size_t)y * w + x) * c + ch] = (unsigned char)v;
    }
  }
}

// ---- Mixup / CutMix: a batch mixed with a shifted copy of itself (include/sykepic_hip.h, spk_mix_batch) ----
// The batch is one flat array of T (bytes of the uint8 NHWC batch, floats of the float32 NCHW batch).  A thread owns one
// 16-byte chunk of the OUTPUT, counted from the 16-byte boundary at or below `out` (`lead` elements in front of it), so
// every whole chunk is stored with one aligned 16-byte store whatever the pointer and the image size are; the first and
// the last chunk may be partial, and a chunk that straddles two images (h * w * c need not be a multiple of anything)
// goes element by element, as the partial ones do.  The two reads of a whole chunk pick their width from the address
// they get: the partner image starts shift * h * w * c elements away, at any byte offset for uint8.
struct MixArgs {
  const void* in;
  void* out;
  long long total;  // elements in the batch
  long long img;    // elements per image
  int n, h, w, c, shift;
  float ca, cb;
  int y1, x1, y2, x2;
  int lead;  // elements between the 16-byte boundary below `out` and `out`
  int copy;  // (ca, cb) == (0, 1): inside the box the partner's element is copied, no arithmetic
};

// each product rounded, then the sum: what torch computes as ca * a + cb * b in three float32 ops.  HIP's __fmul_rn /
// __fadd_rn are the plain operators (compiled with the default contraction, so a product and the sum still fuse into
// one fma after inlining): the operators are written out here with contraction off, as augment_kernel does.
__device__ __forceinline__ float mix_val(float ca, float a, float cb, float b) {
#pragma clang fp contract(off)
  const float pa = ca * a, pb = cb * b;
  return pa + pb;
}
__device__ __forceinline__ float mix_one(float a, float b, float ca, float cb) { return mix_val(ca, a, cb, b); }
__device__ __forceinline__ unsigned char mix_one(unsigned char a, unsigned char b, float ca, float cb) {
  const float v = rintf(mix_val(ca, (float)a, cb, (float)b));   // ties to even
  return (unsigned char)fminf(fmaxf(v, 0.f), 255.f);
}

// position of an element inside its image: three nested coordinates, p2 innermost - (y, x, channel) for NHWC,
// (channel, y, x) for NCHW
template <bool NHWC>
struct MixPos {
  int p0, p1, p2;
  __device__ __forceinline__ void set(long long r, int d1, int d2) {
    const long long q = r / d2;
    p2 = (int)(r - q * d2);
    p0 = (int)(q / d1);
    p1 = (int)(q - (long long)p0 * d1);
  }
  // one element on; true when that left the image (the position is then the first element of the next one)
  __device__ __forceinline__ bool step(int d0, int d1, int d2) {
    if (++p2 < d2) return false;
    p2 = 0;
    if (++p1 < d1) return false;
    p1 = 0;
    if (++p0 < d0) return false;
    p0 = 0;
    return true;
  }
  __device__ __forceinline__ bool inside(const MixArgs& a) const {
    const int y = NHWC ? p0 : p1, x = NHWC ? p1 : p2;
    return y >= a.y1 && y < a.y2 && x >= a.x1 && x < a.x2;
  }
};

template <typename T>
union MixChunk {
  uint4 q;
  unsigned d[4];
  T e[16 / sizeof(T)];
};

// 16 bytes from p, which lie inside the batch: as wide as the address allows
template <typename T>
__device__ __forceinline__ void mix_load(const T* p, MixChunk<T>& v) {
  const size_t u = (size_t)p;
  if ((u & 15) == 0) {
    v.q = *(const uint4*)p;
  } else if ((u & 3) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v.d[k] = ((const unsigned*)p)[k];
  } else {
#pragma unroll
    for (int k = 0; k < (int)(16 / sizeof(T)); ++k) v.e[k] = p[k];
  }
}

template <typename T, bool NHWC>
__global__ __launch_bounds__(256) void mix_kernel(MixArgs a) {
  constexpr int V = 16 / sizeof(T);
  const T* in = (const T*)a.in;
  T* out = (T*)a.out;
  const int d0 = NHWC ? a.h : a.c, d1 = NHWC ? a.w : a.h, d2 = NHWC ? a.c : a.w;
  const long long chunks = (a.total + a.lead + V - 1) / V;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < chunks; q += (long long)gridDim.x * 256) {
    long long e0 = q * V - a.lead;
    int cnt = V;
    if (e0 < 0) { cnt += (int)e0; e0 = 0; }                      // the chunk `out` starts in
    if (e0 + cnt > a.total) cnt = (int)(a.total - e0);           // the chunk it ends in
    int img = (int)(e0 / a.img);
    const long long r = e0 - (long long)img * a.img;
    MixPos<NHWC> pos;
    pos.set(r, d1, d2);
    int pimg = img - a.shift;
    if (pimg < 0) pimg += a.n;
    if (cnt == V && r + V <= a.img) {   // a whole chunk of one image
      MixChunk<T> xv, pv;
      mix_load(in + e0, xv);
      unsigned mask = 0;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if (pos.inside(a)) mask |= 1u << k;
        pos.step(d0, d1, d2);
      }
      if (mask) {
        mix_load(in + (long long)pimg * a.img + r, pv);
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (mask >> k & 1) xv.e[k] = a.copy ? pv.e[k] : mix_one(xv.e[k], pv.e[k], a.ca, a.cb);
      }
      *(uint4*)(out + e0) = xv.q;
    } else {
      long long rr = r;
      for (int k = 0; k < cnt; ++k) {
        T v = in[e0 + k];
        if (pos.inside(a)) {
          const T pv = in[(long long)pimg * a.img + rr];
          v = a.copy ? pv : mix_one(v, pv, a.ca, a.cb);
        }
        out[e0 + k] = v;
        ++rr;
        if (pos.step(d0, d1, d2)) {
          rr = 0;
          if (++img >= a.n) break;   // (cnt ends there too)
          pimg = img - a.shift;
          if (pimg < 0) pimg += a.n;
        }
      }
    }
  }
}

}  // namespace

// Mixup / CutMix of a batch with itself shifted by `shift` images: out[i] = in[i] outside the box [y1,y2) x [x1,x2),
// ca * in[i] + cb * in[(i - shift) mod n] inside it.  Every argument is checked before any HIP call.
extern "C" int spk_mix_batch(const void* in_dev, void* out_dev, int n, int h, int w, int c, int layout, int dtype, int shift,
                             float ca, float cb, int y1, int x1, int y2, int x2, void* stream) {
  auto bad = [](const char* why) {
    spk_set_error(std::string("spk_mix_batch: ") + why);
    return SPK_ERR_ARG;
  };
  if (!in_dev || !out_dev) return bad("null pointer");
  if (n < 1 || h < 1 || w < 1 || (c != 1 && c != 3)) return bad("n, h, w >= 1 and c 1 or 3");
  const bool u8 = layout == SPK_LAYOUT_NHWC && dtype == SPK_DTYPE_U8;
  const bool f32 = layout == SPK_LAYOUT_NCHW && dtype == SPK_DTYPE_F32;
  if (!u8 && !f32) return bad("layout / dtype must be NHWC uint8 or NCHW float32");
  if (shift < 0 || shift >= n) return bad("shift outside [0, n)");
  if (!(fabsf(ca) <= 3.402823466e38f) || !(fabsf(cb) <= 3.402823466e38f)) return bad("ca / cb not finite");
  if (y1 < 0 || x1 < 0 || y2 < y1 || x2 < x1 || y2 > h || x2 > w) return bad("box outside the image or inverted");
  const size_t esz = u8 ? 1 : 4;
  const size_t img = (size_t)h * w * c, total = img * n, bytes = total * esz;
  const size_t ia = (size_t)in_dev, oa = (size_t)out_dev;
  if (ia < oa + bytes && oa < ia + bytes) return bad("in and out overlap (the mix is out of place)");
  if (f32 && ((ia | oa) & 3)) return bad("float32 batch not 4-byte aligned");
  MixArgs a;
  a.in = in_dev; a.out = out_dev;
  a.total = (long long)total; a.img = (long long)img;
  a.n = n; a.h = h; a.w = w; a.c = c; a.shift = shift;
  a.ca = ca; a.cb = cb;
  a.y1 = y1; a.x1 = x1; a.y2 = y2; a.x2 = x2;
  a.lead = (int)((oa & 15) / esz);
  a.copy = ca == 0.f && cb == 1.f;
  const size_t per = 16 / esz;
  const size_t chunks = (total + a.lead + per - 1) / per;
  size_t gx = (chunks + 255) / 256;
  if (gx > 8192) gx = 8192;
  hipStream_t s = (hipStream_t)stream;
  if (u8)
    hipLaunchKernelGGL((mix_kernel<unsigned char, true>), dim3((unsigned)gx), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((mix_kernel<float, false>), dim3((unsigned)gx), dim3(256), 0, s, a);
  if (hipGetLastError() != hipSuccess) {
    spk_set_error("spk_mix_batch: launch failed");
    return SPK_ERR_HIP;
  }
  return SPK_OK;
}

extern "C" int spk_augment_batch(const unsigned char* in_dev, unsigned char* out_dev, unsigned char* tmp_dev, int n,
                                 int h, int w, int c, const spk_aug_op* ops_dev, int n_ops,
                                 const unsigned char* border_dev, void* stream) {
  if (!in_dev || !out_dev || n < 0 || h <= 0 || w <= 0 || c < 1 || c > 4 || n_ops < 0 ||
      (n_ops > 0 && (!ops_dev || !border_dev)) || (n_ops > 1 && !tmp_dev)) {
    spk_set_error("spk_augment_batch: bad arguments");
    return SPK_ERR_ARG;
  }
  if (n == 0) return SPK_OK;
  hipStream_t s = (hipStream_t)stream;
  const size_t bytes = (size_t)n * h * w * c;
  if (n_ops == 0) {
    if (hipMemcpyAsync(out_dev, in_dev, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) {
      spk_set_error("spk_augment_batch: copy failed");
      return SPK_ERR_HIP;
    }
    return SPK_OK;
  }
  // ping-pong so that the last op lands in out_dev
  const unsigned char* src = in_dev;
  int gx = (h * w + 255) / 256;
  if (gx > 64) gx = 64;
  for (int j = 0; j < n_ops; ++j) {
    unsigned char* dst = ((n_ops - 1 - j) % 2 == 0) ? out_dev : tmp_dev;
    hipLaunchKernelGGL(augment_kernel, dim3(gx, n), dim3(256), 0, s, src, dst, h, w, c, ops_dev + (size_t)j * n,
                       border_dev);
    src = dst;
  }
  if (hipGetLastError() != hipSuccess) {
    spk_set_error("spk_augment_batch: launch failed");
    return SPK_ERR_HIP;
  }
  return SPK_OK;
}
