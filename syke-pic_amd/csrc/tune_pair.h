// Paired tuning (tune_table.h, SpkTwin): the twin of a launch - the same problem on the other half batch's slices of
// the same tensors - derived from the launch's own argument struct.  This is the one place that knows which fields of
// an argument struct are activation pointers, image counts and byte extents; a tuner site holds a SpkPair of its
// arguments and hands p[0] / p[1] to the candidate that SpkLaunchTimer::time asks it to run.  (The context is the eval
// forward's: set beside the cursor of each half batch, SpkTwin::user = that half's EvalTwin; a site never sees the handle.)
#pragma once
#include "spk_common.h"
#include "tune_table.h"

namespace spk_pair_detail {
struct Rebase {
  const SpkTwin& tw;
  bool ok = true;
  template <class T>
  void ptr(T*& p) {
    const void* v = (const void*)p;
    if (v && !(tw.rebase && tw.rebase(tw.user, &v))) ok = false;
    p = (T*)v;
  }
  // a per-batch extent (pixels, bytes) of n_self images as that of n_twin images
  template <class T>
  void extent(T& x) {
    if (x % (T)tw.n_self) ok = false;
    else x = x / (T)tw.n_self * (T)tw.n_twin;
  }
  void images(int& n) {
    if (n != tw.n_self) ok = false;
    n = tw.n_twin;
  }
};
// eval launches only: no BatchNorm statistics, no rounding-remainder tensors, no parity classes of a data gradient, no
// channel-padded (MBConv) tensors - a launch with any of them has no twin and is timed alone
inline bool twin_of(Rebase& r, ConvArgs& a) {
  if (a.stats || a.res_lo || a.y_lo || a.cls_ph >= 0 || a.cin_s || a.cout_s) return false;
  r.ptr(a.x); r.ptr(a.y); r.ptr(a.res); r.ptr(a.pool_y);
  r.extent(a.M); r.extent(a.x_bytes);
  r.images(a.N);
  return r.ok;
}
inline bool twin_of(Rebase& r, PwConvArgs& a) {
  r.ptr(a.x); r.ptr(a.y); r.ptr(a.res); r.ptr(a.x2); r.ptr(a.z);
  r.extent(a.M); r.extent(a.x_bytes); r.extent(a.y_bytes); r.extent(a.x2_bytes); r.extent(a.z_bytes);
  r.images(a.N);
  return r.ok;
}
inline bool twin_of(Rebase& r, C3Args& a) {
  r.ptr(a.x); r.ptr(a.y); r.ptr(a.res);
  r.extent(a.M); r.extent(a.x_bytes); r.extent(a.y_bytes);
  r.images(a.N);
  return r.ok;
}
inline bool twin_of(Rebase& r, BneckArgs& a) {
  if (a.stamps) return false;
  r.ptr(a.x); r.ptr(a.y); r.ptr(a.y1); r.ptr(a.z);
  r.extent(a.x_bytes); r.extent(a.z_bytes);
  r.images(a.N);
  return r.ok;
}
}  // namespace spk_pair_detail

// p[0]: the arguments as given; p[1]: their twin when ok (a PAIRS context is set and every activation pointer of the
// struct is this half's slice of a tensor), else p[0] again
template <class A>
struct SpkPair {
  A self, twin;
  bool ok = false;
  explicit SpkPair(const A& a) : self(a), twin(a) {
    const SpkTwin& tw = spk_twin();
    if (tw.mode != SpkTwin::PAIRS || tw.n_self <= 0 || tw.n_twin <= 0) return;
    spk_pair_detail::Rebase r{tw};
    ok = spk_pair_detail::twin_of(r, twin);
    if (!ok) twin = a;
  }
  const A& operator[](int i) const { return i && ok ? twin : self; }
};
