// Test-time augmentation (include/sykepic_hip.h, spk_tta_views / spk_tta_mean): the dihedral views of an image batch
// and the mean of the probabilities the views give.  Both kernels only move or add: the views are a permutation of the
// batch's elements, the mean is float32 adds in view order and one IEEE division.
#include "../../include/sykepic_hip.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

void spk_set_error(const std::string& s);

namespace {

// ---- the views ----
// The batch is a stack of planes of h x w pixels, a pixel PS elements of T: the n images of a uint8 NHWC batch (PS = c
// bytes), the n * c channel planes of a float32 NCHW batch (PS = 1 float).  A block owns one TILE x TILE pixel tile of
// one plane: it reads the tile's rows from global memory once into LDS and writes it out once per view, so a launch
// reads the batch once however many views it makes.  Every view maps the tile onto a tile of the output plane whose
// rows are contiguous runs of elements, so the loads and the stores of all views walk along rows: a thread owns one
// 16-byte chunk of a row run, counted from the 16-byte boundary at or below the run's first element, which makes every
// whole chunk one aligned 16-byte access whatever the pointer and the row length are; the first and the last chunk of
// a run may be partial and go element by element (as mix_kernel's do, augment.hip).  A transposing view reads the LDS
// tile down its columns instead of touching global memory with a stride.
//
// LDS row pitch: the lanes that work on one row run are V = 16 / sizeof(T) elements apart, so on a column read of
// one-element pixels their LDS addresses are V rows apart, and the runs that neighbouring groups of lanes work on are
// one pixel apart.  uint8 (V = 16): an odd pitch in bytes puts rows 16 apart 4 * pitch = 4 (mod 8) dwords apart - the
// 8 chunks of a 128-pixel run on 8 banks, the neighbouring runs on the same or the next dword (three-byte pixels: rows
// 5 or 6 apart, which the odd pitch scatters likewise).  float32 (V = 4): an odd pitch in dwords puts rows 4 apart on
// banks 4 apart, and a 32-pixel tile keeps a run's 8 chunks on 8 banks with the next three runs on the banks between.
struct TtaArgs {
  const void* in;
  void* out;
  long long plane;        // elements per plane
  long long view_stride;  // elements per view: planes * plane
  long long blocks;       // planes * tiles_y * tiles_x
  int h, w, k, tiles_x, tiles_y;
  int views[8];
};

template <typename T>
union TtaChunk {
  uint4 q;
  T e[16 / sizeof(T)];
};

template <typename T, int PS, int TILE, int PITCH>
__global__ __launch_bounds__(256) void tta_views_kernel(TtaArgs a) {
  constexpr int V = 16 / sizeof(T);
  static_assert(PITCH >= TILE * PS, "a tile row must fit its pitch");
  __shared__ T tile[TILE * PITCH];
  const T* in = (const T*)a.in;
  T* out = (T*)a.out;
  const long long tiles = (long long)a.tiles_x * a.tiles_y;
  const long long row = (long long)a.w * PS;   // elements per image row
  for (long long blk = blockIdx.x; blk < a.blocks; blk += gridDim.x) {
    const long long pl = blk / tiles;
    const int t = (int)(blk - pl * tiles);
    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int y0 = ty * TILE, x0 = tx * TILE;
    const int th = min(TILE, a.h - y0), tw = min(TILE, a.w - x0);
    {   // the tile's rows -> LDS
      const int len = tw * PS;
      const int nch = (len + 2 * V - 2) / V;   // chunks of the worst-aligned run of len elements
      const T* src0 = in + pl * a.plane + (long long)y0 * row + (long long)x0 * PS;
      for (int it = threadIdx.x; it < th * nch; it += 256) {
        const int r = it / nch, kk = it - r * nch;
        const T* src = src0 + (long long)r * row;
        const int lead = (int)(((size_t)src & 15) / sizeof(T));
        const int e0 = kk * V - lead;
        if (e0 >= len) continue;               // this run ends before its last possible chunk
        T* dst = tile + r * PITCH;
        if (e0 >= 0 && e0 + V <= len) {
          TtaChunk<T> c;
          c.q = *(const uint4*)(src + e0);
#pragma unroll
          for (int i = 0; i < V; ++i) dst[e0 + i] = c.e[i];
        } else {
          const int lo = max(e0, 0), hi = min(e0 + V, len);
          for (int e = lo; e < hi; ++e) dst[e] = src[e];
        }
      }
    }
    __syncthreads();
    for (int j = 0; j < a.k; ++j) {
      const int v = a.views[j];
      const bool tr = v & 4, fy = v & 2, fx = v & 1;
      // the output tile: oth rows of otw pixels at (oy0, ox0).  Output pixel (r, p) of it is the tile's pixel
      // (row, column) = (ar, bp) for a plain view and (bp, ar) for a transposing one, ar = r or oth - 1 - r (rows
      // reversed), bp = p or otw - 1 - p (columns reversed).  (h == w for a transposing view.)
      const int oth = tr ? tw : th, otw = tr ? th : tw;
      const int oy0 = tr ? (fy ? a.h - x0 - tw : x0) : (fy ? a.h - y0 - th : y0);
      const int ox0 = tr ? (fx ? a.w - y0 - th : y0) : (fx ? a.w - x0 - tw : x0);
      const int len = otw * PS;
      const int nch = (len + 2 * V - 2) / V;
      const int pixstep = tr ? (fx ? -PITCH : PITCH) : (fx ? -PS : PS);   // LDS elements from output pixel p to p + 1
      const int first = fx ? otw - 1 : 0;                                // bp of p = 0
      T* dst0 = out + (long long)j * a.view_stride + pl * a.plane + (long long)oy0 * row + (long long)ox0 * PS;
      for (int it = threadIdx.x; it < oth * nch; it += 256) {
        const int r = it / nch, kk = it - r * nch;
        T* dst = dst0 + (long long)r * row;
        const int lead = (int)(((size_t)dst & 15) / sizeof(T));
        const int e0 = kk * V - lead;
        if (e0 >= len) continue;
        const int ar = fy ? oth - 1 - r : r;
        const int idx0 = tr ? first * PITCH + ar * PS : ar * PITCH + first * PS;
        const int lo = max(e0, 0), hi = min(e0 + V, len);
        const int p = lo / PS;
        int b = lo - p * PS;                   // element inside the pixel
        int idx = idx0 + p * pixstep + b;
        if (lo == e0 && hi == e0 + V) {
          TtaChunk<T> c;
#pragma unroll
          for (int i = 0; i < V; ++i) {
            c.e[i] = tile[idx];
            if (PS == 1) idx += pixstep;
            else if (++b == PS) { b = 0; idx += pixstep - (PS - 1); }
            else ++idx;
          }
          *(uint4*)(dst + e0) = c.q;
        } else {
          for (int e = lo; e < hi; ++e) {
            dst[e] = tile[idx];
            if (PS == 1) idx += pixstep;
            else if (++b == PS) { b = 0; idx += pixstep - (PS - 1); }
            else ++idx;
          }
        }
      }
    }
    __syncthreads();   // the next tile overwrites the LDS
  }
}

template <typename T, int PS, int TILE, int PITCH>
void tta_views_launch(TtaArgs& a, long long planes, hipStream_t s) {
  a.tiles_x = (a.w + TILE - 1) / TILE;
  a.tiles_y = (a.h + TILE - 1) / TILE;
  a.blocks = planes * a.tiles_x * a.tiles_y;
  const long long gx = a.blocks < (1 << 20) ? a.blocks : (1 << 20);
  hipLaunchKernelGGL((tta_views_kernel<T, PS, TILE, PITCH>), dim3((unsigned)gx), dim3(256), 0, s, a);
}

// ---- the mean ----
// A thread owns one 16-byte chunk of the output, counted from the 16-byte boundary at or below `out` (as mix_kernel);
// the k rows of p start numel floats apart, at any 4-byte offset, so their reads pick the width the address allows.
__device__ __forceinline__ float4 tta_load4(const float* p) {
  if (((size_t)p & 15) == 0) return *(const float4*)p;
  return make_float4(p[0], p[1], p[2], p[3]);
}

// ((p0 + p1) + ...) / k: the adds and the division written out with contraction off (there is nothing to contract, and
// hipcc's float32 division is the correctly rounded one by default; the pragma keeps both facts local to this function)
__device__ __forceinline__ float tta_div(float s, float k) {
#pragma clang fp contract(off)
  return __fdiv_rn(s, k);
}

__global__ __launch_bounds__(256) void tta_mean_kernel(const float* __restrict__ p, float* __restrict__ out, int k,
                                                       long long numel, int lead) {
#pragma clang fp contract(off)
  const float fk = (float)k;
  const long long chunks = (numel + lead + 3) / 4;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < chunks; q += (long long)gridDim.x * 256) {
    const long long e0 = q * 4 - lead;
    if (e0 >= 0 && e0 + 4 <= numel) {
      float4 s = tta_load4(p + e0);
      for (int j = 1; j < k; ++j) {
        const float4 v = tta_load4(p + (long long)j * numel + e0);
        s.x = __fadd_rn(s.x, v.x); s.y = __fadd_rn(s.y, v.y); s.z = __fadd_rn(s.z, v.z); s.w = __fadd_rn(s.w, v.w);
      }
      *(float4*)(out + e0) = make_float4(tta_div(s.x, fk), tta_div(s.y, fk), tta_div(s.z, fk), tta_div(s.w, fk));
    } else {
      const long long lo = e0 < 0 ? 0 : e0, hi = e0 + 4 > numel ? numel : e0 + 4;
      for (long long e = lo; e < hi; ++e) {
        float s = p[e];
        for (int j = 1; j < k; ++j) s = __fadd_rn(s, p[(long long)j * numel + e]);
        out[e] = tta_div(s, fk);
      }
    }
  }
}

}  // namespace

extern "C" int spk_tta_views(const void* in_dev, void* out_dev, int n, int h, int w, int c, int layout, int dtype,
                             const int32_t* views_host, int k, void* stream) {
  auto bad = [](const char* why) {
    spk_set_error(std::string("spk_tta_views: ") + why);
    return SPK_ERR_ARG;
  };
  if (!in_dev || !out_dev || !views_host) return bad("null pointer");
  if (n < 1 || h < 1 || w < 1 || (c != 1 && c != 3)) return bad("n, h, w >= 1 and c 1 or 3");
  const bool u8 = layout == SPK_LAYOUT_NHWC && dtype == SPK_DTYPE_U8;
  const bool f32 = layout == SPK_LAYOUT_NCHW && dtype == SPK_DTYPE_F32;
  if (!u8 && !f32) return bad("layout / dtype must be NHWC uint8 or NCHW float32");
  if (k < 1 || k > 8) return bad("k outside 1..8");
  for (int j = 0; j < k; ++j) {
    if (views_host[j] < 0 || views_host[j] > 7) return bad("view code outside 0..7");
    if ((views_host[j] & 4) && h != w) return bad("a transposing view needs h == w");
  }
  const size_t esz = u8 ? 1 : 4;
  const size_t total = (size_t)h * w * c * n, in_bytes = total * esz, out_bytes = in_bytes * k;
  const size_t ia = (size_t)in_dev, oa = (size_t)out_dev;
  if (ia < oa + out_bytes && oa < ia + in_bytes) return bad("in and out overlap (the views are made out of place)");
  if (f32 && ((ia | oa) & 3)) return bad("float32 batch not 4-byte aligned");
  TtaArgs a;
  a.in = in_dev; a.out = out_dev;
  a.h = h; a.w = w; a.k = k;
  a.view_stride = (long long)total;
  for (int j = 0; j < 8; ++j) a.views[j] = j < k ? views_host[j] : 0;
  hipStream_t s = (hipStream_t)stream;
  if (u8) {
    a.plane = (long long)h * w * c;
    if (c == 1) tta_views_launch<unsigned char, 1, 128, 129>(a, n, s);
    else tta_views_launch<unsigned char, 3, 64, 193>(a, n, s);
  } else {
    a.plane = (long long)h * w;
    tta_views_launch<float, 1, 32, 33>(a, (long long)n * c, s);
  }
  if (hipGetLastError() != hipSuccess) {
    spk_set_error("spk_tta_views: launch failed");
    return SPK_ERR_HIP;
  }
  return SPK_OK;
}

extern "C" int spk_tta_mean(const float* p_dev, float* out_dev, int k, int64_t numel, void* stream) {
  auto bad = [](const char* why) {
    spk_set_error(std::string("spk_tta_mean: ") + why);
    return SPK_ERR_ARG;
  };
  if (!p_dev || !out_dev) return bad("null pointer");
  if (k < 1 || k > 8) return bad("k outside 1..8");
  if (numel < 1) return bad("numel < 1");
  const size_t pa = (size_t)p_dev, oa = (size_t)out_dev;
  const size_t out_bytes = (size_t)numel * 4, p_bytes = out_bytes * k;
  if (pa < oa + out_bytes && oa < pa + p_bytes) return bad("p and out overlap");
  if ((pa | oa) & 3) return bad("buffers not 4-byte aligned");
  const int lead = (int)((oa & 15) / 4);
  const size_t chunks = ((size_t)numel + lead + 3) / 4;
  size_t gx = (chunks + 255) / 256;
  if (gx > 8192) gx = 8192;
  hipLaunchKernelGGL(tta_mean_kernel, dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, p_dev, out_dev, k,
                     (long long)numel, lead);
  if (hipGetLastError() != hipSuccess) {
    spk_set_error("spk_tta_mean: launch failed");
    return SPK_ERR_HIP;
  }
  return SPK_OK;
}
