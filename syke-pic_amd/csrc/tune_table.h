// The tuner table: every per-problem autotuner of the library keeps its winners here, one process-wide map behind one
// mutex (handles may be driven from several host threads).  A tuner site owns its key, its candidates, its decision
// rule and its log line; looking a problem up, remembering and appending a winner, the "nearest tuned batch" rule and
// the event timing of a candidate live here.
//
// SPK_TUNE_CACHE=<file>: winners persist across processes, one text line per problem, appended when the problem is
// tuned; the file is parsed once per process.  Ranks of a data-parallel job and re-runs then pick the same
// configurations, the first call of a process does not pay the tuning, and a rocprofv3 kernel trace of a warm run
// holds steady-state launches only.
//
// The mutex is never held while candidates run: a tuner's warm-up launch may reach the nested tuner of the kernel it
// calls (the chain / bottleneck choosers run whole layers, the 1x1 chooser runs the implicit GEMM).
//
// Paired mode (SpkTwin below).  The two-stream eval forward runs every kernel beside its twin - the same layer of the
// other half batch - so what the step pays for a candidate is the time of the PAIR, not the candidate's time alone on
// the chip.  While the two-stream forward has a twin context set, the seven eval tuners look their problems up under "<tag>_p"
// entries of their own (a miss is tuned, never answered from the isolated entry) and time each candidate as `reps`
// pairs: the candidate on the caller's stream, the same candidate on the other half's slices of the same tensors on the
// twin stream, forked and joined with events.  SPK_TUNE_PAIRED=0: no twin context is ever set, isolated tuning
// everywhere.  Forwards on one stream, batches below 64, the per-layer profile, the single-operator hooks, training
// and the MBConv networks never set one and keep the isolated entries.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <array>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

constexpr int kPwNumCfgs = 18;   // configurations of spk_pw_launch (conv_pw.hip)
constexpr int kC3NumCfgs = 14;   // configurations of spk_c3_launch (conv_c3.hip)
constexpr int kD3NumCfgs = 6;    // configurations of spk_d3_launch (conv_d3.hip)

// One line of the file is "<tag> <n_key ints> <n_val ints>".  n_pos is the position of the batch size N among the key
// fields (-1: the key has none and matches exactly only); values outside [val_min, val_max] are dropped on load.
struct TuneSchema { const char* tag; int n_key, n_pos, n_val, val_min, val_max; };
enum TuneTag { TUNE_CONV, TUNE_PW1, TUNE_PW2, TUNE_C3, TUNE_CHAIN, TUNE_BNECK, TUNE_WGRAD, TUNE_DW, TUNE_D3,
               // the paired siblings of the seven eval tuners (spk_tune_tag below): same key and values, timed beside a twin
               TUNE_CONV_P, TUNE_PW1_P, TUNE_PW2_P, TUNE_C3_P, TUNE_CHAIN_P, TUNE_BNECK_P, TUNE_D3_P, TUNE_NTAGS };
constexpr TuneSchema kTuneSchemas[TUNE_NTAGS] = {
    // mode dt splitw N H W Cin Cout k stride pad_cls stats operands -> tile config, main-loop flavour
    {"conv", 13, 3, 2, INT_MIN, INT_MAX},
    {"pw1x1", 9, 8, 1, -1, kPwNumCfgs - 1},   // nb H W Cin Cout stride res relu N -> -1 implicit GEMM, else configuration
    {"pw2", 11, 10, 1, 0, kPwNumCfgs - 1},    // nb H W Cin H2 W2 Cin2 Cout stride stride2 N -> configuration
    {"c3", 6, 5, 1, -1, kC3NumCfgs - 1},      // nb H W Cin Cout N -> configuration, -1 none fits
    {"chain", 6, 5, 1, 0, 1},                 // H W Cin Cin2 Coutz N -> 0 two kernels, 1 chained
    {"bneck", 3, 2, 1, 0, 2},                 // H CM N -> 0 three launches, 1 / 2 whole-block kernel (14- / 7-row blocks)
    {"wgrad", 8, -1, 1, INT_MIN, INT_MAX},    // M Cin Cout k stride stem splits tile -> pipeline stages
    {nullptr, 7, -1, 1, 0, 1},                // depthwise (never in the file): et N H W C k stride -> 0 gather, 1 LDS ring
    {"d3", 4, 3, 1, -1, kD3NumCfgs - 1},      // H W res N -> -1 implicit GEMM, else configuration of the direct 64 -> 64 3x3 kernel
    {"conv_p", 13, 3, 2, INT_MIN, INT_MAX},   // the fields of the line without "_p"; N is the half batch the entry was timed for
    {"pw1x1_p", 9, 8, 1, -1, kPwNumCfgs - 1},
    {"pw2_p", 11, 10, 1, 0, kPwNumCfgs - 1},
    {"c3_p", 6, 5, 1, -1, kC3NumCfgs - 1},
    {"chain_p", 6, 5, 1, 0, 1},
    {"bneck_p", 3, 2, 1, 0, 2},
    {"d3_p", 4, 3, 1, -1, kD3NumCfgs - 1},
};

// nullptr: no file (SPK_TUNE_CACHE unset, empty or "off")
inline const char* spk_tune_cache_path() {
  const char* e = getenv("SPK_TUNE_CACHE");
  return e && *e && strcmp(e, "off") ? e : nullptr;
}
inline bool spk_autotune_on() {
  static const bool v = !getenv("SPK_AUTOTUNE") || atoi(getenv("SPK_AUTOTUNE")) != 0;
  return v;
}
// 0: quiet, 1: each winner, 2: each candidate too (any other setting of SPK_TUNE_LOG prints the winners)
inline int spk_tune_log() {
  static const int v = getenv("SPK_TUNE_LOG") ? (atoi(getenv("SPK_TUNE_LOG")) > 1 ? atoi(getenv("SPK_TUNE_LOG")) : 1) : 0;
  return v;
}

inline bool spk_tune_paired_on() {
  static const bool v = !getenv("SPK_TUNE_PAIRED") || atoi(getenv("SPK_TUNE_PAIRED")) != 0;
  return v;
}

// The twin context of the calling thread, set by the two-stream branch of spk_forward_eval_logits (model.hip) with the
// cursor of the half batch it passes to the executor, cleared on every way out of that branch, and set nowhere else.  PAIRS: the first forward of a shape - both halves run in order on the caller's stream, `stream` is idle, a
// tuner times pairs.  LOOKUP: the halves are live on their two streams (or a pair is being timed): the paired entries
// are looked up, nothing is launched beside anything.
struct SpkTwin {
  enum Mode { OFF = 0, PAIRS = 1, LOOKUP = 2 };
  int mode = OFF;
  hipStream_t stream = nullptr;   // where the twin's launches go
  int n_self = 0, n_twin = 0;     // images of this half and of the other one
  // *p points at this half's first image of an activation tensor (or outside the activations: weights, folded
  // BatchNorm): makes it the other half's first image of the same tensor; false: neither
  bool (*rebase)(void* user, const void** p) = nullptr;
  void* user = nullptr;           // whatever rebase needs (the executor: an EvalTwin, model.h)
};
inline SpkTwin& spk_twin() {
  static thread_local SpkTwin t;
  return t;
}
// the tag a tuner site works with: its own, or the paired sibling while a twin context is set
inline TuneTag spk_tune_tag(TuneTag t) {
  if (spk_twin().mode == SpkTwin::OFF) return t;
  switch (t) {
    case TUNE_CONV: return TUNE_CONV_P;
    case TUNE_PW1: return TUNE_PW1_P;
    case TUNE_PW2: return TUNE_PW2_P;
    case TUNE_C3: return TUNE_C3_P;
    case TUNE_CHAIN: return TUNE_CHAIN_P;
    case TUNE_BNECK: return TUNE_BNECK_P;
    case TUNE_D3: return TUNE_D3_P;
    default: return t;
  }
}
inline bool spk_tune_tag_is_paired(TuneTag t) { return t >= TUNE_CONV_P && t <= TUNE_D3_P; }

namespace spk_tune_detail {
constexpr int kMaxKey = 13, kMaxVal = 2, kLineBuf = 512;
typedef std::array<int, 1 + kMaxKey> Key;   // tag, the key fields without N, N
typedef std::array<int, kMaxVal> Val;
struct Table {
  std::mutex mu;
  std::map<Key, Val> map;
  bool loaded = false;
};
inline Table& table() {
  static Table t;
  return t;
}
inline Key make_key(TuneTag t, const int* key) {
  const TuneSchema& sc = kTuneSchemas[t];
  Key k{};
  int n = 0;
  k[n++] = t;
  for (int i = 0; i < sc.n_key; ++i)
    if (i != sc.n_pos) k[n++] = key[i];
  if (sc.n_pos >= 0) k[n] = key[sc.n_pos];
  return k;
}
// "<tag> <ints>" -> the entry, or nothing: unknown tag, wrong field count, a field that is no int, a value out of range
inline void parse_line_locked(Table& T, const char* line) {
  for (int t = 0; t < TUNE_NTAGS; ++t) {
    const TuneSchema& sc = kTuneSchemas[t];
    const size_t tl = sc.tag ? strlen(sc.tag) : 0;
    if (!tl || strncmp(line, sc.tag, tl) || line[tl] != ' ') continue;
    int v[kMaxKey + kMaxVal];
    const char* p = line + tl;
    for (int i = 0; i < sc.n_key + sc.n_val; ++i) {
      char* end;
      const long x = strtol(p, &end, 10);
      if (end == p || x < INT_MIN || x > INT_MAX) return;
      v[i] = (int)x;
      p = end;
    }
    if (p[strspn(p, " \t\r\n")]) return;
    Val val{};
    for (int i = 0; i < sc.n_val; ++i) {
      if (v[sc.n_key + i] < sc.val_min || v[sc.n_key + i] > sc.val_max) return;
      val[i] = v[sc.n_key + i];
    }
    T.map[make_key((TuneTag)t, v)] = val;
    return;
  }
}
inline void load_locked(Table& T) {
  if (T.loaded) return;
  T.loaded = true;
  const char* path = spk_tune_cache_path();
  FILE* f = path ? fopen(path, "r") : nullptr;
  if (!f) return;
  char line[kLineBuf];
  bool tail = false;   // inside a line longer than the buffer: dropped whole
  while (fgets(line, sizeof line, f)) {
    const size_t len = strlen(line);
    const bool whole = len && line[len - 1] == '\n';
    if (!tail && (whole || len < sizeof line - 1)) parse_line_locked(T, line);
    tail = !whole;
  }
  fclose(f);
}
}  // namespace spk_tune_detail

// The tuned values of this key (all n_key fields, in the order of the line): the exact entry, else - for keys with a
// batch size - the entry of the nearest tuned batch within a factor of two, so that a ragged tail batch re-uses the
// full batch's choice instead of timing every candidate again.  Walking N upward, a tie goes to the larger batch.
inline bool spk_tune_find(TuneTag t, const int* key, int* val) {
  using namespace spk_tune_detail;
  const TuneSchema& sc = kTuneSchemas[t];
  Table& T = table();
  std::lock_guard<std::mutex> lk(T.mu);
  load_locked(T);
  const Key k = make_key(t, key);
  auto hit = T.map.find(k);
  if (hit == T.map.end() && sc.n_pos >= 0) {
    const int n = k[sc.n_key];
    Key lo = k;
    lo[sc.n_key] = INT_MIN;
    double best_ratio = 2.0 + 1e-9;
    for (auto it = T.map.lower_bound(lo); it != T.map.end() && std::equal(k.begin(), k.begin() + sc.n_key, it->first.begin()); ++it) {
      const int n2 = it->first[sc.n_key];
      const double r = n2 > n ? (double)n2 / n : (double)n / n2;
      if (r <= best_ratio) { best_ratio = r; hit = it; }
    }
  }
  if (hit == T.map.end()) return false;
  for (int i = 0; i < sc.n_val; ++i) val[i] = hit->second[i];
  return true;
}

// Remembers the values for the process; persist: also appends the line to the file (if there is one)
inline void spk_tune_store(TuneTag t, const int* key, const int* val, bool persist) {
  using namespace spk_tune_detail;
  const TuneSchema& sc = kTuneSchemas[t];
  Table& T = table();
  std::lock_guard<std::mutex> lk(T.mu);
  load_locked(T);
  Val v{};
  for (int i = 0; i < sc.n_val; ++i) v[i] = val[i];
  T.map[make_key(t, key)] = v;
  const char* path = persist && sc.tag ? spk_tune_cache_path() : nullptr;
  const bool say = spk_tune_log() && spk_tune_tag_is_paired(t);   // (the sites' own log lines do not name the tag)
  if (!path && !say) return;
  char line[kLineBuf];
  int n = snprintf(line, sizeof line, "%s", sc.tag);
  for (int i = 0; i < sc.n_key; ++i) n += snprintf(line + n, sizeof line - n, " %d", key[i]);
  for (int i = 0; i < sc.n_val; ++i) n += snprintf(line + n, sizeof line - n, " %d", val[i]);
  if (say) fprintf(stderr, "[spk tune paired] %s\n", line);
  if (!path) return;
  if (FILE* f = fopen(path, "a")) {
    fprintf(f, "%s\n", line);
    fclose(f);
  }
}

// Tests only: forget everything; the next find / store reads the file SPK_TUNE_CACHE names then
inline void spk_tune_reset_for_test() {
  using namespace spk_tune_detail;
  Table& T = table();
  std::lock_guard<std::mutex> lk(T.mu);
  T.map.clear();
  T.loaded = false;
}

// Event timing of a candidate: `reps` back-to-back calls of run() on the stream, in milliseconds for all of them
struct SpkLaunchTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  const bool ok;   // false: the events could not be created
  SpkLaunchTimer() : ok(hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {}
  hipEvent_t fork = nullptr, join = nullptr;   // paired timing only, created on first use
  ~SpkLaunchTimer() {
    for (hipEvent_t e : {e0, e1, fork, join})
      if (e) (void)hipEventDestroy(e);
  }
  SpkLaunchTimer(const SpkLaunchTimer&) = delete;
  template <class F>
  bool time(hipStream_t s, int reps, F run, float* ms) {
    (void)hipEventRecord(e0, s);
    for (int r = 0; r < reps; ++r) (void)run();
    (void)hipEventRecord(e1, s);
    return hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(ms, e0, e1) == hipSuccess;
  }
  // The eval tuners' form: run(0, s) launches the candidate for the problem in hand, run(1, twin stream) the same
  // candidate for its twin (twin_ok: the site has the twin's arguments, SpkPair in tune_pair.h).  In a PAIRS context the
  // time is that of `reps` pairs - s forks the twin stream, both run their launches back to back, s waits for the
  // twin - and a candidate that does not launch for the twin is no candidate; otherwise the time of run(0, s) alone.
  // While the pair runs the context is LOOKUP: a launch that reaches another tuner finds what that tuner's own (paired)
  // warm-up stored and starts no pairs of its own.
  template <class F>
  bool time(hipStream_t s, int reps, bool twin_ok, F run, float* ms) {
    SpkTwin& tw = spk_twin();
    if (tw.mode != SpkTwin::PAIRS || !twin_ok || !tw.stream || tw.stream == s)
      return time(s, reps, [&] { return run(0, s); }, ms);
    if (!fork && (hipEventCreateWithFlags(&fork, hipEventDisableTiming) != hipSuccess ||
                  hipEventCreateWithFlags(&join, hipEventDisableTiming) != hipSuccess))
      return false;
    tw.mode = SpkTwin::LOOKUP;
    const hipStream_t ts = tw.stream;
    auto fork_twin = [&] { return hipEventRecord(fork, s) == hipSuccess && hipStreamWaitEvent(ts, fork, 0) == hipSuccess; };
    auto join_twin = [&] { return hipEventRecord(join, ts) == hipSuccess && hipStreamWaitEvent(s, join, 0) == hipSuccess; };
    // the twin's warm-up, outside the timed span (the site has warmed the candidate itself)
    bool ok = fork_twin() && run(1, ts) == 0;
    ok = join_twin() && ok;
    (void)hipEventRecord(e0, s);
    ok = ok && fork_twin();
    for (int r = 0; r < reps && ok; ++r) {
      (void)run(0, s);
      ok = run(1, ts) == 0;
    }
    // (join whatever happened: nothing may be left running on the twin stream behind the caller's back)
    ok = join_twin() && ok;
    (void)hipEventRecord(e1, s);
    tw.mode = SpkTwin::PAIRS;
    return hipEventSynchronize(e1) == hipSuccess && ok && hipEventElapsedTime(ms, e0, e1) == hipSuccess;
  }
};
