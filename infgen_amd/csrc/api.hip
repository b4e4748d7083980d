// extern "C" entry points of libinfgen_hip.so (see include/infgen_hip.h) and the per-step
// launch sequence.  No host synchronisation, no allocation: graph-capturable.
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <string>
#include <vector>
#include <atomic>
#include <mutex>
#include <unordered_map>
#include "kernels.h"
#include "../../include/infgen_hip.h"

using namespace ig;

static thread_local std::string g_err;

static int fail(const char* where, const char* what) {
  g_err = std::string(where) + ": " + what;
  return -1;
}
static int fail(const char* where, const char* prefix, const char* what) { return fail(where, (std::string(prefix) + what).c_str()); }
static int check_launch(const char* where) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(where, hipGetErrorString(e));
  return 0;
}
#define RET_IF(x) do { int _r = (x); if (_r) return _r; } while (0)

extern "C" const char* infgen_last_error(void) { return g_err.c_str(); }

// InfgenSampling (NULL: the defaults) -> the kernels' SamplingCtl: 0 means "unset" and equals 1; the per-row array is the caller's to
// check (device memory: engine.py does, once per load)
static int sampling_ctl(const char* where, const InfgenSampling* s, SamplingCtl* out) {
  *out = SAMPLING_DEFAULT;
  if (!s) return 0;
  if (!std::isfinite(s->temperature) || s->temperature < 0.f) return fail(where, "temperature must be finite and >= 0 (0: unset, i.e. 1)");
  if (s->temperature != 0.f && s->temperature < 1.17549435e-38f) return fail(where, "temperature is a denormal: 1 / T overflows");
  if (!(s->top_p >= 0.f && s->top_p <= 1.f)) return fail(where, "top_p must be in (0, 1] (0: unset, i.e. 1)");
  out->temperature = s->temperature == 0.f ? 1.0f : s->temperature;
  out->top_p = s->top_p == 0.f ? 1.0f : s->top_p;
  out->temperature_row = s->temperature_row;
  return 0;
}

// a token mask as the C ABI passes it (include/infgen_hip.h: five parameters, or a handle of infgen_token_mask_create)
struct TokenMaskDesc { const uint32_t* bits; int n_sets; const int* mask_row; int mask_type[3]; const int* type; };
static TokenMaskDesc token_mask_desc(const uint32_t* bits, int n_sets, const int* mask_row, const int* mask_type, const int* type) {
  return TokenMaskDesc{bits, n_sets, mask_row, {mask_type ? mask_type[0] : -1, mask_type ? mask_type[1] : -1, mask_type ? mask_type[2] : -1}, type};
}
// the registered masks: slot h - 1 serves handle h (in_use false: free).  The rider configurations a mask may carry (kernels.h, next
// to their rules; infgen_token_mask_collision / _road / _score / _route / _signal attach them)
struct RiderCfgs { CollisionCfg coll; RoadCfg road; ScoreCfg score; RouteCfg route; SignalCfg signal; };
constexpr RiderCfgs CFGS_NONE{COLLISION_NONE, ROAD_NONE, SCORE_NONE, ROUTE_NONE, SIGNAL_NONE};
struct TokenMaskSlot { TokenMaskDesc d; bool in_use; RiderCfgs cfg; };
static std::mutex g_mask_mu;
static std::vector<TokenMaskSlot> g_masks;
// what rides on a context's decode step: the static mask as the kernels take it and the configurations of its handle
// (validate fills it).  A new mask rider adds to kernels.h a rule, an Args and a Cfg with its NONE, and here a member of RiderCfgs
// and of any(), a MaskKind, a check, a Cfg constructor and its two entries, a launch, a line in validate and a stage in
// infgen_decode_step.  The members up to `route` are the block infgen_token_mask_riders copies out, byte for byte
// (RIDERS_EXPORT_BYTES); later riders stand behind it
struct StepRiders {
  TokenMaskCtl mask; RiderCfgs cfg;
  bool any() const { return mask.bits || cfg.coll.bits || cfg.road.bits || cfg.score.out || cfg.route.bits || cfg.signal.bits; }
};
constexpr StepRiders RIDERS_NONE{TOKEN_MASK_NONE, CFGS_NONE};
constexpr size_t RIDERS_EXPORT_BYTES = offsetof(StepRiders, cfg) + offsetof(RiderCfgs, signal);
// the one handle lookup: f(slot) under g_mask_mu, or the error `what` where the handle names no registered mask
constexpr const char* NO_TOKEN_MASK = "no such token mask";
template <class F> static int with_mask_slot(const char* where, int handle, const char* what, F f) {
  std::lock_guard<std::mutex> lk(g_mask_mu);
  if (handle < 1 || (size_t)handle > g_masks.size() || !g_masks[handle - 1].in_use) return fail(where, what);
  f(g_masks[handle - 1]);
  return 0;
}

// TokenMaskDesc (NULL: none) -> the kernels' TokenMaskCtl.  out->bits stays NULL - the unmasked kernels, today's bits - unless the
// table can constrain some row: a table, n_sets > 0, and per-row selectors or a per-type set
static int token_mask_ctl(const char* where, const TokenMaskDesc* m, int token_size, TokenMaskCtl* out) {
  *out = TOKEN_MASK_NONE;
  if (!m) return 0;
  if (m->n_sets < 0) return fail(where, "token mask: n_sets must be >= 0");
  if (!m->bits || m->n_sets == 0) return 0;
  const bool by_type = m->mask_type[0] >= 0 || m->mask_type[1] >= 0 || m->mask_type[2] >= 0;
  if (by_type && !m->type) return fail(where, "token mask: a per-type set needs the rows' types");
  if (token_size % 32) return fail(where, "token mask: token_size must be a multiple of 32");
  if (reinterpret_cast<uintptr_t>(m->bits) & 15) return fail(where, "token mask: the table must be 16-byte aligned");
  if (!by_type && !m->mask_row) return 0;
  *out = TokenMaskCtl{m->bits, m->n_sets, m->mask_row, {m->mask_type[0], m->mask_type[1], m->mask_type[2]}, by_type ? m->type : nullptr};
  return 0;
}

extern "C" int infgen_token_mask_create(const uint32_t* mask_bits, int mask_n_sets, const int* mask_row, const int* mask_type,
                                        const int* type) {
  if (mask_n_sets < 0) { fail("infgen_token_mask_create", "token mask: n_sets must be >= 0"); return -1; }
  std::lock_guard<std::mutex> lk(g_mask_mu);
  size_t h = 0;
  while (h < g_masks.size() && g_masks[h].in_use) ++h;
  if (h == g_masks.size()) g_masks.push_back(TokenMaskSlot{});
  g_masks[h] = TokenMaskSlot{token_mask_desc(mask_bits, mask_n_sets, mask_row, mask_type, type), true, CFGS_NONE};
  return (int)h + 1;
}
extern "C" int infgen_token_mask_destroy(int handle) {
  return with_mask_slot("infgen_token_mask_destroy", handle, NO_TOKEN_MASK, [](TokenMaskSlot& s) { s.in_use = false; });
}

// ---------------------------------------------------------------------------------- environment knobs
// Experiment and diagnostic switches (tools/, profiles/): each is read once, when the library is loaded.
static int env_int(const char* name, int dflt, bool* is_set = nullptr) {
  const char* e = getenv(name);
  if (is_set) *is_set = e != nullptr;
  return e ? atoi(e) : dflt;
}
static int env_layers_p() { const int v = env_int("INFGEN_LAYERS_P", 1); return v < 0 ? 0 : v > 2 ? 2 : v; }
static int env_lp_rows_min() {         // INFGEN_LP_ROWS8 (non-zero: 8, zero: 16) takes precedence over INFGEN_LP_ROWS_MIN
  bool set8 = false;
  const int rows8 = env_int("INFGEN_LP_ROWS8", 0, &set8);
  return set8 ? (rows8 ? 8 : 16) : env_int("INFGEN_LP_ROWS_MIN", 4);
}
namespace knob {
const int layers_p = env_layers_p();                              // clamped to 0..2: default of the layers_p option (infgen_set_layers_p)
const int qs_dbg = env_int("INFGEN_QS_DBG", 0);                   // FourierArgs.dbg / AttnHArgs.dbg (diagnostics; wrong results)
const int fh12_min = env_int("INFGEN_FH12_MIN", 150000);          // smallest capacity that takes k_fourier_h12 (0: never)
const int fh12_multi_rows = env_int("INFGEN_FH12_MULTI_ROWS", 0); // smallest launch, in rows, whose multi-set launch takes k_fourier_h12_multi (0: never)
const int fourier_nomulti = env_int("INFGEN_FOURIER_NOMULTI", 0); // 1: the step's Fourier sets one launch each
const int attn_hs_max = env_int("INFGEN_ATTN_HS_MAX", 6144);      // attn_mode 2: most rows that take k_attn_hs
const int attn_waves = env_int("INFGEN_ATTN_WAVES", IG_QSU ? 8 : 4);      // 8: the 128-row variant of k_attn_h
const int warm = env_int("INFGEN_WARM", 1);                       // 0: no warm workgroups
const int warm_max_groups = env_int("INFGEN_WARM_MAX_GROUPS", 128);       // launches of more 16-row groups never carry any
const int edge_dbg = env_int("INFGEN_EDGE_DBG", 0);               // EdgeFusedArgs.dbg (timing experiments; bit 7: trace with -DIG_EF_TRACE=1)
const int edge_noxcd = env_int("INFGEN_EDGE_NOXCD", 0);           // bit 0: no XCD-aware tile order, bit 1: no kv_once
const int edge_small = env_int("INFGEN_EDGE_SMALL", 4096);        // most rows of the one-group-per-workgroup k_edge_fused launch
const int edge_wg2 = env_int("INFGEN_EDGE_WG2", 1);               // 0: one 16-wave workgroup of two groups per CU for large launches
const int edge_lds_pad = env_int("INFGEN_EDGE_LDS_PAD", 0);       // dynamic LDS bytes on top of k_edge_fused3's own (co-residency experiment)
const int heads_nosplit = env_int("INFGEN_HEADS_NOSPLIT", 0);     // 1: k_heads never deals its logit chunks to several workgroups
const int be_wide_scenes = env_int("INFGEN_BE_WIDE_SCENES", 128); // largest batch whose k_build_edges runs 16 waves per workgroup whatever A_cap
const int int_group_scenes = env_int("INFGEN_INT_GROUP_SCENES", 128);     // largest batch whose k_integrate runs 16 rows per workgroup
const int no_tail_fold = env_int("INFGEN_NO_TAIL_FOLD", 0);       // 1: infgen_rollout_run is a loop over infgen_decode_step
const int lp_max_chunks = env_int("INFGEN_LP_MAX_CHUNKS", 2);     // most k_layers_p launches a batch may be split into
const int lp_max_groups = env_int("INFGEN_LP_MAX_GROUPS", 256);   // most workgroups of one k_layers_p launch
const int lp_rows_min = env_lp_rows_min();                        // fewest rows per k_layers_p workgroup (4, 8 or 16)
const int cm_rows = env_int("INFGEN_CM_ROWS", 0);                 // rows of a scene per k_collision_mask workgroup (0: by launch size)
const int lp_trace = env_int("INFGEN_LP_TRACE", 0);               // n: dump the stamps of the n-th k_layers_p launch (tools/lp_trace.py)
// polls at a scene counter before k_layers_p traps (layers_p_launch); any strtoul base, and set differs from unset
const char* const lp_spin_str = getenv("INFGEN_LP_SPIN_LIMIT");
const unsigned lp_spin_limit = lp_spin_str ? (unsigned)strtoul(lp_spin_str, nullptr, 0) : 0u;
}  // namespace knob
// the two knobs of infgen_rollout_run's split mode, read at every call (a process may run both paths: tests/test_split_halves_gpu.py)
static int split_halves_knob() { return env_int("INFGEN_SPLIT_HALVES", 1); }      // 0 never, 1 by the rule of run_split_mode, 2 at every even S
static int split_offset_knob() { return env_int("INFGEN_SPLIT_OFFSET", 4); }      // sublayers (two launches each) the second half's step starts behind the first half's; 0: no phase control

// ---------------------------------------------------------------------------------- options
// Every switch that changes what a launch does lives in an InfgenOptions.  g_def holds the process-wide defaults the
// infgen_set_* functions edit (used by the operator-level entries and by contexts with opts.use == 0); a rollout-level entry
// called with a context whose opts.use != 0 installs that context's block for the duration of the call (thread-local), so
// contexts of one process do not see each other's settings.
namespace {
InfgenOptions g_def = {0, /*attn_mode*/ 2, /*gemm_terms*/ 3, /*fourier_mode*/ 1, /*edge_fuse*/ 1, /*edge_loop*/ 6, /*overlap*/ 0,
                       /*row_group_margin*/ 0, /*layers_p*/ knob::layers_p, /*rhat_format*/ 0, /*edge_kernel*/ 1, 0, nullptr, nullptr};
int g_def_group_rows = 0;                  // rows of the layout the process-wide group list belongs to
const int* g_def_limit_n_agents = nullptr; // process-wide row limits (infgen_set_row_limits)
int g_def_limit_A_cap = 0;
struct Active { const InfgenOptions* o; int group_rows; const int* n_agents; int A_cap; };
thread_local Active tl_active = {nullptr, 0, nullptr, 0};
thread_local InfgenOptions tl_thread_opts;         // infgen_thread_options: the calling thread's block for operator-level entries
thread_local bool tl_thread_set = false;
inline const InfgenOptions& O() { return tl_active.o ? *tl_active.o : tl_thread_set ? tl_thread_opts : g_def; }
inline int group_rows() { return tl_active.o ? tl_active.group_rows : g_def_group_rows; }
inline const int* limit_n_agents() { return tl_active.o ? tl_active.n_agents : g_def_limit_n_agents; }
inline int limit_A_cap() { return tl_active.o ? tl_active.A_cap : g_def_limit_A_cap; }
struct OptScope {
  Active prev;
  explicit OptScope(const InfgenRollout* r) : prev(tl_active) {
    if (r && r->opts.use) tl_active = Active{&r->opts, r->S * r->A_cap, r->opts.row_groups ? r->n_agents : nullptr, r->A_cap};
  }
  ~OptScope() { tl_active = prev; }
};
}  // namespace

extern "C" int infgen_get_options(InfgenOptions* out) {
  if (!out) return fail("infgen_get_options", "null pointer");
  *out = g_def;
  return 0;
}

extern "C" int infgen_thread_options(const InfgenOptions* o) {
  if (o) { tl_thread_opts = *o; tl_thread_opts.row_groups = nullptr; tl_thread_opts.n_row_groups = nullptr; }
  tl_thread_set = o != nullptr;
  return 0;
}

extern "C" int infgen_get_effective_options(InfgenOptions* out) {
  if (!out) return fail("infgen_get_effective_options", "null pointer");
  *out = O();
  return 0;
}

// A half of a split rollout (infgen_rollout_run) is a context of half the scenes inside the caller's arrays.
// What a launch sizes by the WHOLE layout comes from here while a half is being enqueued (thread-local, zero outside):
//   full_rows  the stride of the K / V ring's slots and of the step-major logs (logits, log-probabilities, uniforms)
//   cap_scale  whole / half edge capacity: the by-capacity Fourier variant stays the whole batch's (launch_fourier)
//   mark_ev    recorded on the half's stream behind sublayer mark_at of the step (layers_core): the other half's step waits for it
struct SplitTl { int full_rows; int cap_scale; hipEvent_t mark_ev; int mark_at; };
static thread_local SplitTl tl_split = {0, 1, nullptr, -1};
static inline int stride_rows(const InfgenRollout* r) { return tl_split.full_rows ? tl_split.full_rows : r->S * r->A_cap; }

// ---------------------------------------------------------------------------------- profiling
// Optional, process-global, off by default: HIP events recorded on the launch stream around the
// launches of the selected kernels (bench.py's roofline leg).  Not used by the product path.
namespace {
struct Prof {
  unsigned mask = 0;
  std::vector<hipEvent_t> e0, e1;
  std::vector<int> kid;
  std::vector<int> phase_of;                // 0: prologue / operator-level call, 1: inside a decode step (infgen_decode_step, infgen_rollout_run)
  std::vector<double> macs;                 // algorithmic multiply-accumulates of the launch (0: not a GEMM kernel)
  int stride = 1;                           // of the launches inside decode steps every stride-th is bracketed (infgen_prof_set_stride)
  int seen[INFGEN_KID_COUNT] = {};          // launches of the selected kernels since infgen_prof_enable, bracketed or not
  int seen_step[INFGEN_KID_COUNT] = {};     // ... of them inside decode steps
  size_t used = 0;
  unsigned long long* rows_dev = nullptr;   // [16] device counters: [n] rows processed by k_fourier with n input dims (n < 8);
                                            // [8 + kind] edges built by k_build_edges (kind 0 temporal, 1 map, 2 agent)
} g_prof;

static thread_local int t_prof_phase = 0;       // 1: the calling thread is inside a decode step (ProfPhase below)
static std::mutex g_prof_mu;                    // slot allocation and the launch counters (two host threads may drive two contexts)
struct ProfScope {
  int slot = -1;
  hipStream_t s;
  ProfScope(int kid, void* stream, double macs = 0.0) : s((hipStream_t)stream) {
    if ((g_prof.mask >> kid) & 1u) {
      std::lock_guard<std::mutex> lk(g_prof_mu);
      ++g_prof.seen[kid];
      // an event pair costs ~5 us of launch-stream time: inside the timed region only every stride-th decode-step launch carries one
      const bool take = t_prof_phase != 1 || (g_prof.seen_step[kid]++ % g_prof.stride) == 0;
      if (take && g_prof.used < g_prof.e0.size()) {
        slot = (int)g_prof.used++;
        g_prof.kid[slot] = kid;
        g_prof.phase_of[slot] = t_prof_phase;
        g_prof.macs[slot] = macs;
        (void)hipEventRecord(g_prof.e0[slot], s);
      }
    }
  }
  ~ProfScope() { if (slot >= 0) (void)hipEventRecord(g_prof.e1[slot], s); }
};
// launches issued inside a decode step are tagged (bench.py separates the step's edge launches from the prologue's)
// (per host thread: two threads driving two contexts save / restore their own tag - a shared one could be left at 1 by an
// interleaved save / restore pair, after which every later prologue launch counted as a step launch)
struct ProfPhase {
  int old;
  explicit ProfPhase(int p) : old(t_prof_phase) { t_prof_phase = p; }
  ~ProfPhase() { t_prof_phase = old; }
};
}  // namespace

extern "C" int infgen_prof_enable(unsigned mask, int max_launches) {
  if (mask && (int)g_prof.e0.size() < max_launches) {
    const size_t old = g_prof.e0.size();
    g_prof.e0.resize(max_launches); g_prof.e1.resize(max_launches); g_prof.kid.resize(max_launches);
    g_prof.phase_of.resize(max_launches);
    g_prof.macs.resize(max_launches);
    for (size_t i = old; i < (size_t)max_launches; ++i) {
      if (hipEventCreate(&g_prof.e0[i]) != hipSuccess || hipEventCreate(&g_prof.e1[i]) != hipSuccess)
        return fail("infgen_prof_enable", "hipEventCreate failed");
    }
  }
  if (mask && !g_prof.rows_dev) {
    if (hipMalloc(&g_prof.rows_dev, 16 * sizeof(unsigned long long)) != hipSuccess)
      return fail("infgen_prof_enable", "hipMalloc failed");
  }
  if (g_prof.rows_dev) (void)hipMemset(g_prof.rows_dev, 0, 16 * sizeof(unsigned long long));
  g_prof.mask = mask;
  g_prof.used = 0;
  g_prof.stride = 1;
  for (int k = 0; k < INFGEN_KID_COUNT; ++k) g_prof.seen[k] = g_prof.seen_step[k] = 0;
  return 0;
}
// after infgen_prof_enable: bracket only every stride-th launch of the selected kernels inside decode steps (launches outside
// them are all bracketed); infgen_prof_seen returns how many launches there were, bracketed or not
extern "C" int infgen_prof_set_stride(int stride) {
  if (stride < 1) return fail("infgen_prof_set_stride", "stride must be >= 1");
  g_prof.stride = stride;
  return 0;
}
extern "C" int infgen_prof_seen(int* seen, int* seen_step) {
  for (int k = 0; k < INFGEN_KID_COUNT; ++k) {
    if (seen) seen[k] = g_prof.seen[k];
    if (seen_step) seen_step[k] = g_prof.seen_step[k];
  }
  return 0;
}

// total_ms / calls: [INFGEN_KID_COUNT]; counters: [16] device-side row / edge counts (see Prof::rows_dev).  Synchronises.
static int prof_collect_impl(double* total_ms, int* calls, double* total_macs, unsigned long long* fourier_rows,
                             double* step_ms, int* step_calls) {
  for (int k = 0; k < INFGEN_KID_COUNT; ++k) {
    total_ms[k] = 0.0; calls[k] = 0; total_macs[k] = 0.0;
    if (step_ms) step_ms[k] = 0.0;
    if (step_calls) step_calls[k] = 0;
  }
  if (hipDeviceSynchronize() != hipSuccess) return fail("infgen_prof_collect", "sync failed");
  for (size_t i = 0; i < g_prof.used; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_prof.e0[i], g_prof.e1[i]) != hipSuccess)
      return fail("infgen_prof_collect", "hipEventElapsedTime failed");
    total_ms[g_prof.kid[i]] += ms;
    calls[g_prof.kid[i]] += 1;
    total_macs[g_prof.kid[i]] += g_prof.macs[i];
    if (g_prof.phase_of[i] == 1) {
      if (step_ms) step_ms[g_prof.kid[i]] += ms;
      if (step_calls) step_calls[g_prof.kid[i]] += 1;
    }
  }
  if (fourier_rows) {
    for (int i = 0; i < 16; ++i) fourier_rows[i] = 0;
    if (g_prof.rows_dev) (void)hipMemcpy(fourier_rows, g_prof.rows_dev, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  }
  g_prof.used = 0;
  return 0;
}
extern "C" int infgen_prof_collect(double* total_ms, int* calls, double* total_macs, unsigned long long* fourier_rows) {
  return prof_collect_impl(total_ms, calls, total_macs, fourier_rows, nullptr, nullptr);
}
extern "C" int infgen_prof_collect_steps(double* total_ms, int* calls, double* total_macs, unsigned long long* fourier_rows,
                                         double* step_ms, int* step_calls) {
  return prof_collect_impl(total_ms, calls, total_macs, fourier_rows, step_ms, step_calls);
}

constexpr int ATTN_SPLIT_ROWS = 10240;     // INFGEN_Q_ATTN_SPLIT_ROWS: attn_mode 2 takes the split kernels beyond this many rows (attn_split)
extern "C" int infgen_layout_query(int what) {
  switch (what) {
    case INFGEN_Q_ATTN_PACK_SIZE: return AL_SIZE;
    case INFGEN_Q_FOURIER_PACK_SIZE_N2: return fourier_pack_size(2);
    case INFGEN_Q_FOURIER_PACK_SIZE_N3: return fourier_pack_size(3);
    case INFGEN_Q_FOURIER_PACK_SIZE_N4: return fourier_pack_size(4);
    case INFGEN_Q_TILE_ROWS: return TR;
    case INFGEN_Q_EDGE_ATTN_CAP: return 1 << 30;   /* single-pass kernel: no per-row edge cap */
    case INFGEN_Q_MAX_AGENTS: return MAX_SCENE_AGENTS;
    case INFGEN_Q_ABI_VERSION: return 1;
    case INFGEN_Q_SIZEOF_ROLLOUT: return (int)sizeof(InfgenRollout);
    case INFGEN_Q_ATTN_SPLIT_ROWS: return ATTN_SPLIT_ROWS;
    case INFGEN_Q_HEADS_SAMPLE_K: return HEADS_KS;
    default: return -1;
  }
}

extern "C" int infgen_attn_pack_offset(const char* f) {
#define F(name, val) if (!strcmp(f, name)) return val;
  F("ln_src_g", AL_LN_SRC_G) F("ln_src_b", AL_LN_SRC_B) F("ln_dst_g", AL_LN_DST_G) F("ln_dst_b", AL_LN_DST_B)
  F("wq", AL_WQ) F("bq", AL_BQ) F("wk", AL_WK) F("wv", AL_WV) F("bv", AL_BV)
  F("wkr", AL_WKR) F("wvr", AL_WVR) F("bvr", AL_BVR) F("ws", AL_WS) F("bs", AL_BS)
  F("wg", AL_WG) F("bg", AL_BG) F("wo", AL_WO) F("bo", AL_BO)
  F("ln_post_g", AL_LN_POST_G) F("ln_post_b", AL_LN_POST_B)
  F("ln_ffpre_g", AL_LN_FFPRE_G) F("ln_ffpre_b", AL_LN_FFPRE_B)
  F("w1", AL_W1) F("b1", AL_B1) F("w2", AL_W2) F("b2", AL_B2)
  F("ln_ffpost_g", AL_LN_FFPOST_G) F("ln_ffpost_b", AL_LN_FFPOST_B)
  F("h_hdr", AH_HDR) F("h_pre", AH_PRE) F("h_post", AH_POST)
#undef F
  return -1;
}

extern "C" int infgen_fourier_pack_offset(const char* f, int n, int dim) {
  const int d0 = FE_DIM0 + dim * FD_SIZE;
  const int t0 = FE_DIM0 + n * FD_SIZE;
#define F(name, val) if (!strcmp(f, name)) return val;
  F("freq", FE_FREQ + dim * 64)
  F("w1", d0 + FD_W1) F("w1x", d0 + FD_W1X) F("b1", d0 + FD_B1) F("ln_g", d0 + FD_LN_G) F("ln_b", d0 + FD_LN_B)
  F("w2", d0 + FD_W2)
  F("b2sum", t0 + FT_B2SUM) F("lno_g", t0 + FT_LN_G) F("lno_b", t0 + FT_LN_B) F("w3", t0 + FT_W3) F("b3", t0 + FT_B3)
  // fp16-split section (FourierHLayout)
  const int h0 = fourier_pack_size_f32(n);
  const int hd = h0 + FH_DIM0 + dim * FHD_SIZE;
  F("h_hdr", h0 + FH_HDR) F("h_freq", h0 + FH_FREQ + dim * 64)
  F("h_wx", hd + FHD_WX) F("h_b1", hd + FHD_B1) F("h_g1", hd + FHD_G1) F("h_be1", hd + FHD_BE1)
  F("h_b2sum", h0 + FH_TAIL + FHT_B2SUM) F("h_g2", h0 + FH_TAIL + FHT_G2) F("h_be2", h0 + FH_TAIL + FHT_BE2)
  F("h_b3", h0 + FH_TAIL + FHT_B3)
  F("h_mat", h0 + FH_VEC_SIZE + dim * FH_HALF_MAT_FLOATS)      /* dim = half-matrix index here */
#undef F
  return -1;
}

// ---------------------------------------------------------------------------------- launchers
static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
// 64-row tiles (k_attn_h<4>, k_heads_h, k_map_head_h, k_mlpemb_h): two workgroups per CU, persistent over the tiles beyond that
static inline int grid64(int rows) { const int g = ceil_div(rows, 64); return g > 512 ? 512 : g; }

// The kernels of a split family share one signature: k3 the fp16 three-term split (gemm_terms 3), kb16 bf16-precision operands (2),
// k1 plain fp16 operands (1).  Every launch of such a family picks its kernel here.
template <typename Kern> static Kern by_terms(Kern k3, Kern kb16, Kern k1) {
  switch (O().gemm_terms) {
    case 1: return k1;
    case 2: return kb16;
    default: return k3;
  }
}
// k_fourier_h12 and k_layers_p exist in the three-term form only
static inline bool three_terms() { return O().gemm_terms == 3; }

extern "C" int infgen_linear(const float* X, int ldx, const int* gather, int rows, int K,
                             const float* Wp, int Np, const float* bias, int N,
                             const float* pre_g, const float* pre_b, const float* post_g, const float* post_b, int relu,
                             float* Y, int ldy, void* stream) {
  if (rows <= 0) return 0;
  if (Np % 32) return fail("infgen_linear", "Np must be a multiple of 32");
  if (K > 128 && Np > 128) return fail("infgen_linear", "K > 128 requires N <= 128");
  if ((pre_g && K != 128) || (post_g && (N != 128 || Np != 128)))
    return fail("infgen_linear", "LayerNorm prologue/epilogue needs K == 128 / N == 128");
  LinearArgs a{X, ldx, gather, rows, K, ((K + 7) / 8) * 8, Wp, Np, bias, N, pre_g, pre_b, post_g, post_b, relu, Y, ldy};
  { ProfScope _ps(INFGEN_KID_LINEAR, stream, (double)rows * K * N);
    const int tiles = ceil_div(rows, TR), passes = ceil_div(Np, 128);
    const int gy = (K <= 128 && !post_g && passes > 1 && tiles < 512) ? min(passes, ceil_div(512, tiles)) : 1;
    hipLaunchKernelGGL(k_linear, dim3(tiles, gy), dim3(NT), 0, (hipStream_t)stream, a); }
  return check_launch("infgen_linear");
}

// n (<= 6) independent infgen_linear calls in one launch; desc[i] mirrors infgen_linear's arguments
extern "C" int infgen_linear_multi(const InfgenLinearDesc* desc, int n, void* stream) {
  if (n <= 0) return 0;
  if (n > LINEAR_MULTI_MAX) return fail("infgen_linear_multi", "at most 6 descriptors");
  LinearMultiArgs m;
  int tiles = 0, gy = 1;
  double flops = 0.0;
  for (int i = 0; i < n; ++i) {
    const InfgenLinearDesc& d = desc[i];
    if (d.rows <= 0) return fail("infgen_linear_multi", "empty descriptor");
    if (d.Np % 32) return fail("infgen_linear_multi", "Np must be a multiple of 32");
    if (d.K > 128 && d.Np > 128) return fail("infgen_linear_multi", "K > 128 requires N <= 128");
    if ((d.pre_g && d.K != 128) || (d.post_g && (d.N != 128 || d.Np != 128)))
      return fail("infgen_linear_multi", "LayerNorm prologue/epilogue needs K == 128 / N == 128");
    m.d[i] = LinearArgs{d.X, d.ldx, d.gather, d.rows, d.K, ((d.K + 7) / 8) * 8, d.Wp, d.Np, d.bias, d.N, d.pre_g, d.pre_b,
                        d.post_g, d.post_b, d.relu, d.Y, d.ldy};
    tiles = tiles > ceil_div(d.rows, TR) ? tiles : ceil_div(d.rows, TR);
    const int passes = ceil_div(d.Np, 128);
    if (d.K <= 128 && !d.post_g && passes > gy) gy = passes;
    flops += (double)d.rows * d.K * d.N;
  }
  if (tiles * gy > 2048) gy = 2048 / tiles > 0 ? 2048 / tiles : 1;
  { ProfScope _ps(INFGEN_KID_LINEAR, stream, flops);
    hipLaunchKernelGGL(k_linear_multi, dim3(tiles, gy, n), dim3(NT), 0, (hipStream_t)stream, m); }
  return check_launch("infgen_linear_multi");
}

// counter calibration (tools/calibrate_fetch.sh): stream n_bytes with `width` (8 or 16) bytes per lane; out: [2048] floats
extern "C" int infgen_debug_stream_read(const float* p, unsigned long long n_bytes, int width, float* out, void* stream) {
  if (width != 8 && width != 16) return fail("infgen_debug_stream_read", "width must be 8 or 16");
  if (hipMemsetAsync(out, 0, 2048 * sizeof(float), (hipStream_t)stream) != hipSuccess) return fail("infgen_debug_stream_read", "memset failed");
  if (width == 8) hipLaunchKernelGGL(k_stream_read<8>, dim3(2048), dim3(256), 0, (hipStream_t)stream, p, (size_t)(n_bytes / 4), out);
  else hipLaunchKernelGGL(k_stream_read<16>, dim3(2048), dim3(256), 0, (hipStream_t)stream, p, (size_t)(n_bytes / 4), out);
  return check_launch("infgen_debug_stream_read");
}

extern "C" int infgen_layernorm(const float* X, int rows, const float* gamma, const float* beta, float* Y, void* stream) {
  if (rows <= 0) return 0;
  hipLaunchKernelGGL(k_layernorm, dim3(ceil_div(rows, TR)), dim3(NT), 0, (hipStream_t)stream, X, rows, gamma, beta, Y);
  return check_launch("infgen_layernorm");
}

// 3 (default): fp16 three-term split = fp32 accuracy; 1: only the hi x hi product of the same packed operands, i.e. plain fp16
// arithmetic (11 bits per operand) in the split kernels - the reduced-precision mode for BASELINE config C5 ("bf16"), which
// forfeits the 1e-3 logits bar.  Governs k_fourier_h, k_attn_h, k_mlpemb_h, k_heads_h.
extern "C" int infgen_set_gemm_terms(int terms) {
  if (terms < 1 || terms > 3) return fail("infgen_set_gemm_terms", "terms must be 3 (split, fp32 accuracy), 2 (bf16 operands) or 1 (fp16 operands)");
  g_def.gemm_terms = terms;
  return 0;
}

// fourier_mode 1: fp16 three-term split (k_fourier_h), 0: fp32-input MFMA (k_fourier)
extern "C" int infgen_set_fourier_mode(int mode) {
  if (mode != 0 && mode != 1) return fail("infgen_set_fourier_mode", "mode must be 0 (fp32 MFMA) or 1 (fp16 split)");
  g_def.fourier_mode = mode;
  return 0;
}

// prof: the profiler's row counter, on unless dt_mode == 2 (that launch writes the table, it embeds no rows).  dbg stays 0 here:
// launch_fourier sets it for the single-set kernels, the multi-set launch leaves it 0
static FourierArgs fourier_args(const float* raw, int n, const int* count_dev, int e_cap, const float* pack, const float* cat, int ldcat,
                                float* out, int ldo, int normalize, int out_r24, const float* dt_tab = nullptr, int dt_mode = 0) {
  return FourierArgs{raw, n, count_dev, e_cap, pack, cat, ldcat, out, ldo, normalize,
                     (g_prof.mask >> INFGEN_KID_FOURIER) & 1u && dt_mode != 2 ? g_prof.rows_dev : nullptr, out_r24, dt_tab, dt_mode, 0};
}

// workgroups of a split Fourier launch over `cap` rows: 128-row tiles (8 waves x 16 rows; wide: 192), persistent, one workgroup
// per CU (fourier_h.hip explains why)
static inline int fourier_h_grid(int cap, bool wide) {
  const int grid = ceil_div(cap, wide ? FH12_TILE : FH_TILE);
  return grid > 256 * FH_WG_PER_CU ? 256 * FH_WG_PER_CU : grid;
}

// one set in one launch (the entries below have checked the arguments; the step's own sets need no check)
static int launch_fourier(const FourierArgs& a_in, void* stream) {
  if (a_in.e_cap <= 0) return 0;
  FourierArgs a = a_in;
  a.dbg = knob::qs_dbg;
  { ProfScope _ps(INFGEN_KID_FOURIER, stream);
    if (O().fourier_mode == 0) {
      int grid = ceil_div(a.e_cap, TR);
      if (grid > 2048) grid = 2048;
      hipLaunchKernelGGL(k_fourier, dim3(grid), dim3(NT), 0, (hipStream_t)stream, a);
    } else {
      // large sets: the three-wave-group variant (fourier_h12.hip)
      const bool wide = knob::fh12_min > 0 && (long long)a.e_cap * tl_split.cap_scale >= knob::fh12_min && three_terms() && FH_WAVES == 8;
      const int grid = fourier_h_grid(a.e_cap, wide);
      if (wide) hipLaunchKernelGGL(k_fourier_h12<3>, dim3(grid), dim3(FH12_NT), 0, (hipStream_t)stream, a);
      else hipLaunchKernelGGL(by_terms(k_fourier_h<3>, k_fourier_h_b16<1>, k_fourier_h<1>), dim3(grid), dim3(FH_NT), 0, (hipStream_t)stream, a);
    } }
  return check_launch("infgen_fourier_embed");
}

// out_r24: rows in the packed 24-bit format of kernels.h (k_fourier_h only; the rollout's private rhat buffers)
static int fourier_embed_impl(const float* raw, int n, const int* count_dev, int e_cap, const float* pack,
                              const float* cat, int ldcat, float* out, int ldo, int normalize, int out_r24, void* stream,
                              const float* dt_tab = nullptr, int dt_mode = 0) {
  if (e_cap <= 0) return 0;
  if (n < 1 || n > 4) return fail("infgen_fourier_embed", "n_dims must be in 1..4");
  if (out_r24 && O().fourier_mode == 0) return fail("infgen_fourier_embed", "packed rows need the split kernel");
  if (dt_mode && (O().fourier_mode == 0 || n < 2 || (dt_mode == 1 && !dt_tab)))
    return fail("infgen_fourier_embed", "the last-dim table needs the split kernel, n_dims >= 2 and a table");
  return launch_fourier(fourier_args(raw, n, count_dev, e_cap, pack, cat, ldcat, out, ldo, normalize, out_r24, dt_tab, dt_mode), stream);
}

extern "C" int infgen_fourier_embed(const float* raw, int n, const int* count_dev, int e_cap, const float* pack,
                                    const float* cat, int ldcat, float* out, int ldo, int normalize, void* stream) {
  return fourier_embed_impl(raw, n, count_dev, e_cap, pack, cat, ldcat, out, ldo, normalize, 0, stream);
}

// The last input dim of a FourierEmbedding as a lookup (include/infgen_hip.h): table of its branch at the values 0, -1, ..
extern "C" int infgen_fourier_last_dim_table(const float* pack, int n, float* table, void* stream) {
  return fourier_embed_impl(nullptr, n, nullptr, DT_TAB_ROWS, pack, nullptr, 0, table, 128, 0, 0, stream, nullptr, 2);
}
extern "C" int infgen_fourier_embed_tab(const float* raw, int n, const int* count_dev, int e_cap, const float* pack,
                                        const float* table, float* out, int ldo, int normalize, void* stream) {
  return fourier_embed_impl(raw, n, count_dev, e_cap, pack, nullptr, 0, out, ldo, normalize, 0, stream, table, 1);
}

// 0: fp32-input MFMA (k_attn_pre / k_attn_post), 1: fp16 three-term split on 64-row tiles (k_attn_h), 3: the same arithmetic on
// one 16-row group per eight-wave workgroup (k_attn_hs, low latency), 2 (default): by size - k_attn_h runs one or two workgroups
// per CU on 64-row tiles and wins from ~10 k rows (16 k rows: 99 vs 121 us for the fp32 kernels); below, a launch is one tile's
// dependency chain whatever the row count (k_attn_h 61-69 us, fp32 kernels 48-53 us), which k_attn_hs cuts to 27-32 us up to 4 k
// rows (one 16-row workgroup per CU; every workgroup pulls the layer's 1.2 MB of split weights through its CU's L2 port)
extern "C" int infgen_set_attn_mode(int mode) {
  if (mode < 0 || mode > 3) return fail("infgen_set_attn_mode", "mode must be 0 (fp32 MFMA), 1 (fp16 split), 2 (by size) or 3 (fp16 split, 16-row workgroups)");
  g_def.attn_mode = mode;
  return 0;
}
// the kernels of the other split families (k_heads_h, k_mlpemb_h) keep the by-size rule of the 64-row tiles
static inline bool attn_split_for(int mode, int rows) { return mode == 1 || (mode >= 2 && rows > ATTN_SPLIT_ROWS); }
static inline bool attn_split(int rows) { return attn_split_for(O().attn_mode, rows); }
// How one emission - heads, the draw, the log-probabilities - runs: the one statement of its by-size rules.  Every entry that emits
// motion tokens, validate() and, through the two exported queries, the engine read it; emit_tokens issues what it names
struct EmitPlan {
  bool split;          // the heads run as the split kernel (k_heads_h, 64-row tiles), else as k_heads (fp32 MFMA)
  bool sample_fused;   // the top-k draw runs inside the split kernel (k_heads_h<TERMS, LP, HEADS_KS>): it runs and the beam fits its lists
  bool lp_fused;       // token_logprob comes out of the split kernel: beside the arg-max, or beside the draw made inside it
  bool need_logits;    // the chain reads logits [rows][token_size] from memory: k_sample_topk and / or k_token_logprob after the heads
  int ns;              // the workgroups per row tile that share k_heads' logit chunks (1: no column split, no keys)
};
// k <= 1: arg-max; col_split: keys for k_heads' column split are there and INFGEN_HEADS_NOSPLIT is off.  Pure: it reads nothing but
// its arguments (attn_mode is the caller's: O()'s, or a context's own) and launches nothing
static EmitPlan emit_plan(int attn_mode, int rows, int token_size, int k, bool want_token_lp, bool col_split) {
  const bool split = attn_split_for(attn_mode, rows), sample_fused = k > 1 && k <= HEADS_KS && split;
  const bool lp_fused = want_token_lp && (k > 1 ? sample_fused : split);      // (after k_sample_topk only the chain knows the token)
  const int tiles = ceil_div(rows, TR), nchunk = token_size / 128;
  int ns = 1;
  while (col_split && !split && 2 * ns <= nchunk && nchunk % (2 * ns) == 0 && tiles * 2 * ns <= 512) ns *= 2;
  return EmitPlan{split, sample_fused, lp_fused, (k > 1 && !sample_fused) || (want_token_lp && !lp_fused), ns};
}
extern "C" int infgen_heads_sample_fused(int attn_mode, int rows, int k) { return emit_plan(attn_mode, rows, 0, k, false, false).sample_fused; }
extern "C" int infgen_heads_logprob_fused(int attn_mode, int rows) { return emit_plan(attn_mode, rows, 0, 1, true, false).lp_fused; }
// 0: fp32 kernels, 1: k_attn_h, 2: k_attn_hs
static inline int attn_kind(int rows) {
  switch (O().attn_mode) {
    case 0: return 0;
    case 1: return 1;
    case 3: return 2;
    default: return rows > 10240 ? 1 : rows > knob::attn_hs_max ? 0 : 2;      // (8 k rows: 60 us for k_attn_hs and the fp32 kernels alike)
  }
}

// 64-row tiles, 4 waves, two workgroups per CU (attn_h.hip); INFGEN_ATTN_WAVES=8 selects the 128-row variant
// optional list of the 16-row groups that hold agents (infgen_set_row_groups): applied to every split-kernel launch over
// exactly `g_group_rows` rows, i.e. the [S][A_cap] row arrays of the rollout the caller is running
extern "C" int infgen_set_row_groups(const int* groups, const int* n_groups, int rows) {
  g_def.row_groups = groups; g_def.n_row_groups = n_groups; g_def_group_rows = groups ? rows : 0;
  if (!groups) g_def_limit_n_agents = nullptr;
  return 0;
}

// the same information for the edge kernel (one wave per row): n_agents [S] of the [S][A_cap] layout and the margin the group
// list was built with; applies to launches over exactly the rows given to infgen_set_row_groups
extern "C" int infgen_set_row_limits(const int* n_agents, int A_cap, int margin) {
  g_def_limit_n_agents = n_agents; g_def_limit_A_cap = A_cap; g_def.row_group_margin = margin;
  return 0;
}

extern "C" int infgen_active_row_groups(const int* n_agents, int S, int A_cap, int margin, int* groups, int* n_groups,
                                        void* stream) {
  if (S <= 0 || A_cap <= 0) return fail("infgen_active_row_groups", "empty layout");
  ActiveGroupsArgs a{n_agents, S, A_cap, margin, groups, n_groups};
  hipLaunchKernelGGL(k_active_groups, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  return check_launch("infgen_active_row_groups");
}

// The next small launch's warm workgroups (tile.cuh: WarmArgs): set by the sublayer loop right before the launch that carries them,
// taken (and cleared) by launch_attn_h / edge_fused_launch.  INFGEN_WARM=0 switches them off; launches of more than
// INFGEN_WARM_MAX_GROUPS 16-row groups (default 128) never carry any - they leave no CU idle.
static thread_local WarmArgs t_warm = {};
static void warm_request(const void* p0, int len0, const void* p1, int len1) {
  t_warm.p[0] = (const char*)p0; t_warm.len[0] = p0 ? len0 : 0; t_warm.p[1] = (const char*)p1; t_warm.len[1] = p1 ? len1 : 0;
}
// -> grid with the warm workgroups appended (or the grid as it was)
static int warm_take(WarmArgs& w, int grid) {
  WarmArgs req = t_warm;
  t_warm = WarmArgs{};
  w = WarmArgs{};
  if (!(req.len[0] > 0 || req.len[1] > 0) || grid > (knob::warm ? knob::warm_max_groups : 0)) return grid;
  const int wg0 = (grid + 7) & ~7;
  const int per = (256 - wg0) / 8 < 24 ? (256 - wg0) / 8 : 24;
  if (per <= 0) return grid;
  w = req; w.wg0 = wg0; w.per_xcd = per;
  return wg0 + 8 * per;
}

static void launch_attn_h(const AttnHArgs& a_in, void* stream) {
  AttnHArgs a = a_in;
  a.dbg = knob::qs_dbg;
  if (O().row_groups && a.rows == group_rows()) { a.groups = O().row_groups; a.n_groups = O().n_row_groups; }
  if (attn_kind(a.rows) == 2) {            // one 16-row group per workgroup
    const int grid = warm_take(a.warm, ceil_div(a.rows, 16));
    hipLaunchKernelGGL(by_terms(k_attn_hs<3>, k_attn_hs_b16<1>, k_attn_hs<1>), dim3(grid), dim3(512), 0, (hipStream_t)stream, a);
    return;
  }
  t_warm = WarmArgs{};
  if (knob::attn_waves != 8) {
    auto kern = by_terms(k_attn_h<4, 3>, k_attn_h_b16<4, 1>, k_attn_h<4, 1>);
    hipLaunchKernelGGL(kern, dim3(grid64(a.rows)), dim3(256), 0, (hipStream_t)stream, a);
  } else {
    // the 8-wave variant is launched in its three-term form whatever gemm_terms says ("gemm_terms=2 is not applied
    // uniformly").  Kept as it was: the fix is by_terms() over the 8-wave kernels here.
    int grid = ceil_div(a.rows, 128);
    if (grid > 256) grid = 256;
    hipLaunchKernelGGL((k_attn_h<8, 3>), dim3(grid), dim3(512), 0, (hipStream_t)stream, a);
  }
}

// profiler MAC counts of the node kernels: 16384 per row and 128 x 128 projection (whole numbers below 2^53: exact in any order)
static double attn_pre_macs(int rows, const void* Q, const void* U, const void* K, const void* V) {
  return (double)rows * 16384.0 * ((Q || U ? 1 : 0) + (K ? 1 : 0) + (V ? 1 : 0) + (U ? 1 : 0));
}
// the post part (12 projections' worth, one more with the positional part) and the next layer's pre part
static double attn_post_macs(int rows, int has_pos, const void* next_pack, const void* nQ, const void* nU, const void* nK, const void* nV) {
  return (double)rows * (196608.0 + (has_pos ? 16384.0 : 0.0)) + (next_pack ? attn_pre_macs(rows, nQ, nU, nK, nV) : 0.0);
}
static double heads_macs(int rows, int token_size) { return (double)rows * (2 * 16384.0 + 128.0 * token_size + 384.0); }

extern "C" int infgen_attn_pre(const float* X, int rows, const float* pack, int use_src_ln,
                               float* Q, float* U, float* K, float* V, void* stream) {
  if (rows <= 0) return 0;
  { ProfScope _ps(INFGEN_KID_ATTN_PRE, stream, attn_pre_macs(rows, Q, U, K, V));
    if (attn_kind(rows)) {
      launch_attn_h(AttnHArgs{const_cast<float*>(X), rows, nullptr, nullptr, nullptr, nullptr, 0, pack, use_src_ln, Q, U, K, V}, stream);
    } else {
      AttnPreArgs a{X, rows, pack, use_src_ln, Q, U, K, V};
      hipLaunchKernelGGL(k_attn_pre, dim3(ceil_div(rows, TR)), dim3(NT), 0, (hipStream_t)stream, a);
    } }
  return check_launch("infgen_attn_pre");
}

static int edge_attn_impl(int rows, const float* Q, const float* U, const float* Ksrc, const float* Vsrc,
                          const int* off, const int* cnt, const int* src, const float* rhat,
                          float* AGG, float* Z, float* SIG, int wide, void* stream, const int* row_mask = nullptr) {
  if (rows <= 0) return 0;
  EdgeAttnArgs a{rows, Q, U, Ksrc, Vsrc, EdgeSet{off, cnt, src, rhat}, AGG, Z, SIG, nullptr, nullptr, 0, 0, wide ? row_mask : nullptr};
  if (limit_n_agents() && O().row_groups && rows == group_rows() && !wide) {
    a.n_agents = limit_n_agents(); a.A_cap = limit_A_cap(); a.margin = O().row_group_margin;
  }
  { ProfScope _ps(INFGEN_KID_EDGE_ATTN, stream);
    if (wide) hipLaunchKernelGGL(k_edge_attn_wide, dim3(rows), dim3(512), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_edge_attn, dim3(ceil_div(rows, 4)), dim3(NT), 0, (hipStream_t)stream, a); }
  return check_launch("infgen_edge_attn");
}

// 1 (default): infgen_decode_layers runs the edge side of every sublayer with k_edge_fused - the absorbed query U and the
// positional aggregate Z of a 16-row tile stay on chip (LDS) and the node kernels run with has_pos = 0; 0: the unfused
// sequence with U / Z / SIG in HBM (kept for comparison and used below 257 rows, where k_edge_attn_wide splits long edge lists)
extern "C" int infgen_set_edge_fuse(int mode) {
  if (mode < 0 || mode > 2) return fail("infgen_set_edge_fuse", "mode must be 0 (off), 1 (from 257 rows) or 2 (always)");
  g_def.edge_fuse = mode;
  return 0;
}

// row format of the step's own rhat rows: 0 fp32 (default), 1 packed 24-bit (include/infgen_hip.h)
extern "C" int infgen_set_rhat_format(int format) {
  if (format != 0 && format != 1) return fail("infgen_set_rhat_format", "format must be 0 (fp32 rows) or 1 (packed 24-bit rows)");
  g_def.rhat_format = format;
  return 0;
}

// lane layout of the fused edge kernel's loop: 0 k_edge_fused, 1 k_edge_fused3 for launches beyond 4 k rows, 2 k_edge_fused3 always
extern "C" int infgen_set_edge_kernel(int kernel) {
  if (kernel < 0 || kernel > 2) return fail("infgen_set_edge_kernel", "kernel must be 0, 1 or 2");
  g_def.edge_kernel = kernel;
  return 0;
}

// edges per trip of k_edge_fused's edge loop (their K / V / rhat rows are requested together): 4, 6 (default) or 8
extern "C" int infgen_set_edge_loop(int v) {
  if (v != 4 && v != 6 && v != 8) return fail("infgen_set_edge_loop", "edges per trip must be 4, 6 or 8");
  g_def.edge_loop = v;
  return 0;
}

// resident workgroups per CU the runtime reports for k_edge_fused<6> (diagnostics; tools/edge_probe.sh)
extern "C" int infgen_edge_fused_occupancy(void) {
  int n = -1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_edge_fused<6, true, 1, 8>, 512, 0) != hipSuccess) return -1;
  return n;
}

static int edge_fused_launch(int rows, const float* Q, const float* pack, const float* Ksrc, const float* Vsrc, const EdgeSet& es,
                             float* AGG, int rows_per_scene, int kv_once, void* stream, int r24 = 0) {
  if (rows <= 0) return 0;
  if (!pack || !es.rhat) return fail("infgen_edge_attn_fused", "needs the layer pack and rhat");
  const int dbg = knob::edge_dbg, no_xcd = knob::edge_noxcd, small_max = knob::edge_small, wg2 = knob::edge_wg2;
  const int G = O().edge_loop;
  // small launches: one 16-row group per workgroup (edge_fused.hip), twice the workgroups for the same rows
  const bool small = rows <= small_max && G == 6;
  // large launches: 8-wave workgroups of one 16-row group, two per CU - one's matrix phases run under the other's edge loop
  // (128 vs 140 us per launch at 512 scenes; INFGEN_EDGE_WG2=0: one 16-wave workgroup of two groups per CU)
  const bool two = !small && wg2 && G == 6;
  const int tr = (small || two) ? 16 : 32;          // rows per tile
  EdgeFusedArgs a{rows, Q, pack, Ksrc, Vsrc, es, AGG, nullptr, nullptr, dbg, 0, kv_once};
  int grid = ceil_div(rows, tr);           // with a group list at most that many
  if (O().row_groups && rows == group_rows()) { a.groups = O().row_groups; a.n_groups = O().n_row_groups; }
  else if (rows_per_scene > tr && rows_per_scene % tr == 0 && !(no_xcd & 1)) {
    a.tiles_per_scene = rows_per_scene / tr;
    const int grp = 8 * a.tiles_per_scene;
    grid = ceil_div(grid, grp) * grp;
  }
  if (no_xcd & 2) a.kv_once = 0;
  if (!r24 && (O().edge_kernel == 2 || (O().edge_kernel == 1 && !small))) {
    // k_edge_fused3 (edge_fused3.hip): one 8-wave workgroup per 16-row group at every size, fp32 rhat rows
    EdgeFusedArgs m = a;
    int mg = ceil_div(rows, 16);
    m.tiles_per_scene = 0;
    if (!m.groups && rows_per_scene > 16 && rows_per_scene % 16 == 0 && !(no_xcd & 1)) {
      m.tiles_per_scene = rows_per_scene / 16;
      const int grp = 8 * m.tiles_per_scene;
      mg = ceil_div(mg, grp) * grp;
    }
    m.n_virtual = mg;
    t_warm = WarmArgs{};
    { ProfScope _ps(INFGEN_KID_EDGE_ATTN, stream);
      auto k3 = G == 4 ? k_edge_fused3<4> : G == 8 ? k_edge_fused3<8> : k_edge_fused3<6>;
      // (INFGEN_EDGE_LDS_PAD=<bytes>, experiment: dynamic LDS on top of the kernel's 75 KB - from ~6 KB on only ONE workgroup fits a
      // CU, which leaves room for another stream's node kernel; profiles/r06_coresidency_ab.txt)
      hipLaunchKernelGGL(k3, dim3(mg), dim3(512), knob::edge_lds_pad, (hipStream_t)stream, m); }
    return check_launch("infgen_edge_attn_fused(k_edge_fused3)");
  }
  a.n_virtual = grid;
  if (small) grid = warm_take(a.warm, grid); else t_warm = WarmArgs{};
  static unsigned long long* ef_trace = nullptr;       // (timing experiment: INFGEN_EDGE_DBG bit 7 with an -DIG_EF_TRACE=1 build)
  if (dbg & 128) {
    if (!ef_trace && hipMalloc(&ef_trace, 64 * sizeof(unsigned long long)) != hipSuccess) return fail("infgen_edge_attn_fused", "trace buffer");
    (void)hipMemsetAsync(ef_trace, 0, 64 * sizeof(unsigned long long), (hipStream_t)stream);
    a.dbgbuf = reinterpret_cast<unsigned*>(ef_trace);
  }
  { ProfScope _ps(INFGEN_KID_EDGE_ATTN, stream);
    auto kern = small ? (r24 ? k_edge_fused<6, true, 1, 16> : k_edge_fused<6, false, 1, 16>)
              : two ? (r24 ? k_edge_fused<6, true, 1, 8> : k_edge_fused<6, false, 1, 8>)
              : r24 ? (G == 4 ? k_edge_fused<4, true, 2, 16> : G == 8 ? k_edge_fused<8, true, 2, 16> : k_edge_fused<6, true, 2, 16>)
                    : (G == 4 ? k_edge_fused<4, false, 2, 16> : G == 8 ? k_edge_fused<8, false, 2, 16> : k_edge_fused<6, false, 2, 16>);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(two ? 512 : 1024), 0, (hipStream_t)stream, a); }
  if (dbg & 128) {
    static int dumps = 0;
    if (dumps++ < 3) {
      unsigned long long hst[64];
      (void)hipStreamSynchronize((hipStream_t)stream);
      (void)hipMemcpy(hst, ef_trace, sizeof(hst), hipMemcpyDeviceToHost);
      for (int i = 1; i < 8; ++i) fprintf(stderr, "[ef trace] %d +%lld\n", i, hst[i] && hst[0] ? (long long)(hst[i] - hst[0]) : -1ll);
    }
  }
  return check_launch("infgen_edge_attn_fused");
}

extern "C" int infgen_edge_attn_fused(int rows, const float* Q, const float* pack, const float* Ksrc, const float* Vsrc,
                                      const int* off, const int* cnt, const int* src, const float* rhat,
                                      float* AGG, void* stream) {
  return edge_fused_launch(rows, Q, pack, Ksrc, Vsrc, EdgeSet{off, cnt, src, rhat}, AGG, 0, 0, stream);
}

// the same pair of operators with the rows of rhat in the packed 24-bit form (include/infgen_hip.h): what infgen_decode_layers does
// for its own edge sets, for callers that own the buffer between the two calls (the map encoder of infgen_amd/engine.py)
extern "C" int infgen_fourier_embed_r24(const float* raw, int n, const int* count_dev, int e_cap, const float* pack, void* out,
                                        void* stream) {
  return fourier_embed_impl(raw, n, count_dev, e_cap, pack, nullptr, 0, static_cast<float*>(out), 128, 1, 1, stream);
}

extern "C" int infgen_edge_attn_fused_r24(int rows, const float* Q, const float* pack, const float* Ksrc, const float* Vsrc,
                                          const int* off, const int* cnt, const int* src, const void* rhat24,
                                          float* AGG, void* stream) {
  return edge_fused_launch(rows, Q, pack, Ksrc, Vsrc, EdgeSet{off, cnt, src, static_cast<const float*>(rhat24)}, AGG, 0, 0, stream, 1);
}

// one wave per destination; few destinations (<= 256 rows) get the 8-wave split so that the chip is not idle
extern "C" int infgen_edge_attn(int rows, const float* Q, const float* U, const float* Ksrc, const float* Vsrc,
                                const int* off, const int* cnt, const int* src, const float* rhat,
                                float* AGG, float* Z, float* SIG, void* stream) {
  return edge_attn_impl(rows, Q, U, Ksrc, Vsrc, off, cnt, src, rhat, AGG, Z, SIG, rows <= 256 ? 1 : 0, stream);
}

extern "C" int infgen_edge_attn_mode(int rows, const float* Q, const float* U, const float* Ksrc, const float* Vsrc,
                                     const int* off, const int* cnt, const int* src, const float* rhat,
                                     float* AGG, float* Z, float* SIG, int wide, void* stream) {
  return edge_attn_impl(rows, Q, U, Ksrc, Vsrc, off, cnt, src, rhat, AGG, Z, SIG, wide, stream);
}

static int attn_post_fused(float* X, int rows, const float* pack, const float* AGG, const float* Z, const float* SIG,
                           int has_pos, const float* next_pack, float* nQ, float* nU, float* nK, float* nV, void* stream) {
  if (rows <= 0) return 0;
  { ProfScope _ps(INFGEN_KID_ATTN_POST, stream, attn_post_macs(rows, has_pos, next_pack, nQ, nU, nK, nV));
    if (attn_kind(rows)) {
      launch_attn_h(AttnHArgs{X, rows, pack, AGG, Z, SIG, has_pos, next_pack, 0, nQ, nU, nK, nV}, stream);
    } else {
      AttnPostArgs a{X, rows, pack, AGG, Z, SIG, has_pos, next_pack, nQ, nU, nK, nV};
      hipLaunchKernelGGL(k_attn_post, dim3(ceil_div(rows, TR)), dim3(NT), 0, (hipStream_t)stream, a);
    } }
  return check_launch("infgen_attn_post");
}

extern "C" int infgen_attn_post(float* X, int rows, const float* pack, const float* AGG, const float* Z,
                                const float* SIG, int has_pos, void* stream) {
  return attn_post_fused(X, rows, pack, AGG, Z, SIG, has_pos, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int infgen_attn_post_pre(float* X, int rows, const float* pack, const float* AGG, const float* Z,
                                    const float* SIG, int has_pos, const float* next_pack, float* nQ, float* nU,
                                    float* nK, float* nV, void* stream) {
  return attn_post_fused(X, rows, pack, AGG, Z, SIG, has_pos, next_pack, nQ, nU, nK, nV, stream);
}

extern "C" int infgen_match_agent_tokens(const unsigned char* valid, const float* pos, const float* heading, const float* shape,
                                        const int* type, const float* tok, long long tok_agent_stride, int A, int T, int shift,
                                        int n_token, int* token_index, float* token_contour, void* stream) {
  if (A <= 0) return 0;
  if (shift <= 0 || T <= shift) return fail("infgen_match_agent_tokens", "need 0 < shift < T");
  if (n_token <= 0 || n_token > 2048) return fail("infgen_match_agent_tokens", "n_token must be in 1..2048");
  MatchTokensArgs a{valid, pos, heading, shape, type, tok, tok_agent_stride, A, T, shift, n_token, token_index, token_contour};
  hipLaunchKernelGGL(k_match_tokens, dim3(A), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("infgen_match_agent_tokens");
}

extern "C" int infgen_tokenize_agent(unsigned char* valid, float* pos, float* heading, float* velocity, const int* type,
                                    const float* tok, const float* shape_in, float* shape_out, float* wl_work, int A, int T,
                                    int shift, int current_step, int n_token, int invalid_state, int valid_state,
                                    int enter_state, int exit_state, int predict_state, int* token_index,
                                    float* token_contour, int* state_idx, float* token_pos, float* token_heading,
                                    unsigned char* token_valid, unsigned char* raw_token_valid, void* stream) {
  if (A <= 0) return 0;
  if (shift <= 0 || T <= shift || current_step < shift || current_step >= T)
    return fail("infgen_tokenize_agent", "need 0 < shift <= current_step < T");
  if (n_token <= 0 || n_token > 2048) return fail("infgen_tokenize_agent", "n_token must be in 1..2048");
  TokenizeArgs t{valid, pos, heading, velocity, type, wl_work, shape_in, shape_out, A, T, shift, current_step,
                 invalid_state, valid_state, enter_state, exit_state, predict_state, token_index, token_contour,
                 state_idx, token_pos, token_heading, token_valid, raw_token_valid};
  hipLaunchKernelGGL(k_tokenize_prep, dim3((A + 63) / 64), dim3(64), 0, (hipStream_t)stream, t);
  MatchTokensArgs m{valid, pos, heading, wl_work, type, tok, 0, A, T, shift, n_token, token_index, token_contour};
  hipLaunchKernelGGL(k_match_tokens, dim3(A), dim3(256), 0, (hipStream_t)stream, m);
  hipLaunchKernelGGL(k_tokenize_state, dim3((A + 63) / 64), dim3(64), 0, (hipStream_t)stream, t);
  return check_launch("infgen_tokenize_agent");
}

extern "C" int infgen_fetch_enterings(const float* token_pos, const float* token_heading, const int* state_idx,
                                     const int* agent_ptr, const int* av_index, int B, int max_agents, int T,
                                     const float* grid_xy, int grid_size, float radius, float angle_interval,
                                     int enter_state, int invalid_state, int* grid_token_idx, float* grid_offset_xy,
                                     int* heading_token_idx, int* sort_indices, unsigned char* inrange_mask,
                                     unsigned char* bos_mask, float* pos_xy, float* heading_theta, const float* pt_pos,
                                     int pt_stride, const int* pt_ptr, int M, int* pt_grid_token_idx, void* stream) {
  if (B <= 0 || T <= 0) return 0;
  if (max_agents > 2048) return fail("infgen_fetch_enterings", "more than 2048 agents in a scene");
  if (grid_size <= 0) return fail("infgen_fetch_enterings", "empty grid");
  EnteringsArgs a{token_pos, token_heading, state_idx, agent_ptr, av_index, B, T, grid_xy, grid_size, radius, angle_interval,
                  enter_state, invalid_state, grid_token_idx, grid_offset_xy, heading_token_idx, sort_indices, inrange_mask,
                  bos_mask, pos_xy, heading_theta, pt_pos, pt_stride, pt_ptr, M, pt_grid_token_idx};
  hipLaunchKernelGGL(k_fetch_enterings, dim3(B * T), dim3(256), 0, (hipStream_t)stream, a);
  if (pt_grid_token_idx && M > 0) {
    const long long waves = (long long)T * M;
    hipLaunchKernelGGL(k_pt_grid_cells, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  }
  return check_launch("infgen_fetch_enterings");
}

extern "C" int infgen_distance_to_nearest_object(const float* cx, const float* cy, const float* length, const float* width,
                                                const float* heading, const unsigned char* valid, int B, int N, int T,
                                                int n_eval, float corner_rounding_factor, float* work, float* out,
                                                void* stream) {
  if (B <= 0 || N <= 0 || T <= 0 || n_eval <= 0) return 0;
  if (n_eval > N) return fail("infgen_distance_to_nearest_object", "n_eval > N");
  NearestArgs a{cx, cy, length, width, heading, valid, B, N, T, n_eval, corner_rounding_factor, work, out};
  const long long nbox = (long long)B * N * T, nout = (long long)B * n_eval * T;
  hipLaunchKernelGGL(k_box_corners, dim3((unsigned)((nbox + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(k_nearest_distance, dim3((unsigned)((nout + 127) / 128)), dim3(128), 0, (hipStream_t)stream, a);
  return check_launch("infgen_distance_to_nearest_object");
}

extern "C" int infgen_kinematic_features(const float* x, const float* y, const float* z, const float* heading, int n, int T,
                                        float seconds_per_step, float* speed, float* accel, float* yaw_rate,
                                        float* yaw_accel, void* stream) {
  if (n <= 0 || T <= 0) return 0;
  if (!speed) return fail("infgen_kinematic_features", "speed output is required");
  KinematicArgs a{x, y, z, heading, n, T, seconds_per_step, speed, accel, yaw_rate, yaw_accel};
  const long long tot = (long long)n * T;
  hipLaunchKernelGGL(k_kinematic, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("infgen_kinematic_features");
}

extern "C" int infgen_time_to_collision(const float* cx, const float* cy, const float* length, const float* width,
                                       const float* heading, const float* speed, const unsigned char* valid,
                                       const int* eval_idx, int B, int N, int T, int n_eval, float* out, void* stream) {
  if (B <= 0 || N <= 0 || T <= 0 || n_eval <= 0) return 0;
  TtcArgs a{cx, cy, length, width, heading, speed, valid, eval_idx, B, N, T, n_eval, out};
  const long long tot = (long long)B * n_eval * T;
  hipLaunchKernelGGL(k_ttc, dim3((unsigned)((tot + 127) / 128)), dim3(128), 0, (hipStream_t)stream, a);
  return check_launch("infgen_time_to_collision");
}

extern "C" int infgen_distance_to_road_edge(const float* cx, const float* cy, const float* cz, const float* length,
                                          const float* width, const float* height, const float* heading,
                                          const unsigned char* valid, const int* eval_idx, int B, int N, int T, int n_eval,
                                          const float* polylines, const unsigned char* cyclic, const int* poly_off, int L,
                                          float z_stretch, float* out, void* stream) {
  if (B <= 0 || N <= 0 || T <= 0 || n_eval <= 0) return 0;
  if (L < 2) return fail("infgen_distance_to_road_edge", "polylines need at least two points");
  RoadEdgeArgs a{cx, cy, cz, length, width, height, heading, valid, eval_idx, polylines, cyclic, poly_off,
                 B, N, T, n_eval, L, z_stretch, out};
  const long long boxes = (long long)B * n_eval * T;
  hipLaunchKernelGGL(k_road_edge, dim3((unsigned)((boxes + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("infgen_distance_to_road_edge");
}

extern "C" int infgen_window_log_likelihood(const float* values, const unsigned char* valid, int n, int T, int size, int step,
                                           const float* edges, const float* logp, int num_bins, float* out_sum,
                                           int* out_cnt, void* stream) {
  if (n <= 0) return 0;
  if (size <= 0 || step <= 0 || size > T) return fail("infgen_window_log_likelihood", "need 0 < size <= T and step > 0");
  if (num_bins <= 0 || num_bins > 64) return fail("infgen_window_log_likelihood", "num_bins must be in 1..64");
  WindowLoglikArgs a{values, valid, n, T, size, step, edges, logp, num_bins, out_sum, out_cnt};
  const long long tot = (long long)n * ((T - size) / step + 1);
  hipLaunchKernelGGL(k_window_loglik, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("infgen_window_log_likelihood");
}

extern "C" int infgen_placement_features(const float* x, const float* y, const float* z, const int* state, const int* av_index,
                                        int B, int N, int T, int enter_state, int exit_state, int* num_bos, int* num_eos,
                                        float* bos_distance, float* eos_distance, void* stream) {
  if (B <= 0 || N <= 0 || T <= 0) return 0;
  PlacementArgs a{x, y, z, state, av_index, B, N, T, enter_state, exit_state, num_bos, num_eos, bos_distance, eos_distance};
  hipLaunchKernelGGL(k_placement, dim3(B * T), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("infgen_placement_features");
}

extern "C" int infgen_bundle_scores(const unsigned char* valid, const unsigned char* collision, const float* linear_speed,
                                   const float* linear_acceleration, const float* angular_speed,
                                   const float* angular_acceleration, const float* distance_to_nearest_object,
                                   const float* time_to_collision, const float* distance_placement,
                                   const float* distance_removement, const long long* num_placement,
                                   const long long* num_removement, const int* n_rows, const float* table, int n_scenario,
                                   int n_rollout, int N, int T, int ld, int T2, int ld2, int ldn, int size, int step, int shift,
                                   float* scalars, float* lng, float* long_rollout, int* counters, void* stream) {
  if (n_scenario <= 0) return 0;
  const char* me = "infgen_bundle_scores";
  if (n_rollout <= 0 || N <= 0) return fail(me, "need at least one rollout and one object row per bundle");
  if (shift <= 0 || size <= 0 || step <= 0 || size % shift || step % shift) return fail(me, "size and step must be multiples of shift");
  const int size2 = size / shift, step2 = step / shift;
  if (size > T || size2 > T2) return fail(me, "a window is longer than the series");
  if (ld < T || ld2 < T2 || ldn < T2) return fail(me, "row stride shorter than the row");
  if ((long long)(T2 - 1) * shift >= T) return fail(me, "token columns reach beyond the steps");
  const int W = (T - size) / step + 1;
  if ((T2 - size2) / step2 + 1 != W) return fail(me, "window counts of the two rates differ");
  BundleScoreArgs a{valid, collision, {linear_speed, linear_acceleration, angular_speed, angular_acceleration},
                    distance_to_nearest_object, time_to_collision, distance_placement, distance_removement, num_placement,
                    num_removement, n_rows, table, n_scenario, n_rollout, N, T, ld, T2, ld2, ldn, size, step, size2, step2, shift,
                    W, scalars, lng, long_rollout, counters};
  hipLaunchKernelGGL(k_bundle_field, dim3(BS_FIELDS, n_scenario), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(k_bundle_meta, dim3(n_scenario), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch(me);
}

// ---- validation-step metrics (val_metrics.hip).  Arguments are checked before anything is launched.
static_assert(INFGEN_VM_SCRATCH_DOUBLES == VM_MAX_PARTIALS * 3 && INFGEN_GRID_OVERLAP_MAX_CELLS == GO_MAX_CELLS, "header constants");
static inline int vm_blocks(long long work_items, int per_block) {
  const long long nb = (work_items + per_block - 1) / per_block;
  return (int)(nb < 1 ? 1 : nb > VM_MAX_PARTIALS ? VM_MAX_PARTIALS : nb);
}

// StateAccuracy.update / NumInsertAccuracy.update (infgen/utils/metrics.py:499-543, :632-676)
extern "C" int infgen_state_accuracy(const void* state_idx, int idx64, int N, int T, long long ld, const unsigned char* valid_mask,
                                    long long ld_mask, int invalid_state, int valid_state, int enter_state, int exit_state,
                                    long long* acc, void* stream) {
  const char* me = "infgen_state_accuracy";
  if (N < 0) return fail(me, "N is negative");
  if (T < 1) return fail(me, "T must be at least 1");
  if (!acc) return fail(me, "acc is NULL");
  if (N == 0) return 0;
  if (!state_idx) return fail(me, "state_idx is NULL");
  if (ld < T || (valid_mask && ld_mask < T)) return fail(me, "row stride shorter than the row");
  StateAccArgs a{state_idx, valid_mask, N, T, ld, ld_mask, invalid_state, valid_state, enter_state, exit_state,
                 (unsigned long long*)acc};
  const dim3 grid(vm_blocks(N, 4));
  if (idx64) hipLaunchKernelGGL(k_state_accuracy<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_state_accuracy<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
  return check_launch(me);
}

// GridOverlapRate.update (infgen/utils/metrics.py:574-591)
extern "C" int infgen_grid_overlap(const void* state_token, int state64, long long ld_state, const void* grid_index, int grid64,
                                  long long ld_grid, int N, int num_step, const long long* ptr, int n_group, int grid_size,
                                  int enter_state, int seed_size, long long* acc, void* stream) {
  const char* me = "infgen_grid_overlap";
  if (N < 0 || n_group < 0) return fail(me, "N or n_group is negative");
  if (num_step < 1) return fail(me, "num_step must be at least 1");
  if (grid_size < 1 || grid_size > GO_MAX_CELLS) return fail(me, "grid_size must be in 1..16384 (the LDS bitmaps)");
  if (!acc) return fail(me, "acc is NULL");
  if (!ptr) n_group = 1;
  if (n_group == 0) return 0;
  if (N > 0 && (!state_token || !grid_index)) return fail(me, "state_token or grid_index is NULL");
  if (ld_state < num_step || ld_grid < num_step) return fail(me, "row stride shorter than num_step");
  GridOverlapArgs a{state_token, grid_index, ld_state, ld_grid, ptr, N, num_step, n_group, grid_size, enter_state, seed_size,
                    (unsigned long long*)acc};
  const dim3 grid(num_step, n_group);
  if (state64 && grid64) hipLaunchKernelGGL((k_grid_overlap<true, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else if (state64) hipLaunchKernelGGL((k_grid_overlap<true, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else if (grid64) hipLaunchKernelGGL((k_grid_overlap<false, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((k_grid_overlap<false, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
  return check_launch(me);
}

// minADE.update (infgen/utils/metrics.py:441-464) and minFDE.update (:378-387)
extern "C" int infgen_traj_error(const float* pred, const float* target, const unsigned char* valid, int N, int T, void* ade_acc,
                                void* fde_acc, double* scratch, void* stream) {
  const char* me = "infgen_traj_error";
  if (N < 0) return fail(me, "N is negative");
  if (T < 1) return fail(me, "T must be at least 1");
  if (!ade_acc && !fde_acc) return fail(me, "both accumulators are NULL");
  if (!scratch) return fail(me, "scratch is NULL");
  if (N == 0) return 0;
  if (!pred || !target || !valid) return fail(me, "pred, target or valid is NULL");
  const int nb = vm_blocks(N, 256);
  TrajErrArgs a{pred, target, valid, N, T, ade_acc ? (unsigned long long*)ade_acc + 1 : nullptr,
                fde_acc ? (unsigned long long*)fde_acc + 1 : nullptr, scratch};
  hipLaunchKernelGGL(k_traj_error, dim3(nb), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(k_vm_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)scratch, nb, 2, (double*)ade_acc,
                     (double*)fde_acc, (double*)nullptr);
  return check_launch(me);
}

// minMultiADE.update (infgen/utils/metrics.py:403-424) and minMultiFDE.update (:349-361)
extern "C" int infgen_multi_traj_error(const float* pred, const float* target, const float* prob, const unsigned char* valid, int N,
                                      int M, int T, int max_guesses, int keep_invalid_final_step, int ade_criterion, void* ade_acc,
                                      void* fde_acc, double* scratch, void* stream) {
  const char* me = "infgen_multi_traj_error";
  if (N < 0) return fail(me, "N is negative");
  if (T < 1) return fail(me, "T must be at least 1");
  if (M < 1 || M > MTE_MAX_MODES) return fail(me, "M must be in 1..64");
  if (max_guesses < 1) return fail(me, "max_guesses must be at least 1");
  if (ade_criterion != 0 && ade_criterion != 1) return fail(me, "ade_criterion must be 0 ('FDE') or 1 ('ADE')");
  if (!ade_acc && !fde_acc) return fail(me, "both accumulators are NULL");
  if (!scratch) return fail(me, "scratch is NULL");
  if (N == 0) return 0;
  if (!pred || !target || !valid) return fail(me, "pred, target or valid is NULL");
  const int nb = vm_blocks(N, 256);
  MultiTrajErrArgs a{pred, target, prob, valid, N, M, T, max_guesses < M ? max_guesses : M, keep_invalid_final_step ? 1 : 0,
                     ade_criterion, ade_acc ? (unsigned long long*)ade_acc + 1 : nullptr,
                     fde_acc ? (unsigned long long*)fde_acc + 1 : nullptr, scratch};
  hipLaunchKernelGGL(k_multi_traj_error, dim3(nb), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(k_vm_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)scratch, nb, 2, (double*)ade_acc,
                     (double*)fde_acc, (double*)nullptr);
  return check_launch(me);
}

// batch_nms / new_batch_nms (infgen/utils/metrics.py:198-256, :143-195): "modes" of include/infgen_hip.h
extern "C" int infgen_select_modes(const float* traj, long long group_stride, long long row_stride, long long cand_stride,
                                  long long step_stride, int rows_per_group, long long B, int N, int T, int F, int t_goal, int K,
                                  float dist_thresh, const float* score, int score_per_group, const unsigned char* cand_valid,
                                  const float* cand_state, long long state_group_stride, long long state_row_stride,
                                  long long state_cand_stride, float state_invalid, float state_enter, const int* row_limit,
                                  long long limit_stride, int* mode_idx, float* mode_score, float* mode_traj, void* stream) {
  const char* me = "infgen_select_modes";
  if (B < 0) return fail(me, "B is negative");
  if (N < 1 || N > SM_MAX_CAND) return fail(me, "N must be in 1..64 (one candidate per lane of a wave)");
  if (K < 1 || K > SM_MAX_MODES || K > N) return fail(me, "K must be in 1..min(N, 16)");
  if (T < 1 || F < 2) return fail(me, "T must be at least 1 and F at least 2 (x, y)");
  if (t_goal < 0 || t_goal >= T) return fail(me, "t_goal must be in 0..T-1");
  if (rows_per_group < 1) return fail(me, "rows_per_group must be at least 1");
  if (step_stride < F || group_stride < 0 || row_stride < 0 || cand_stride < 0) return fail(me, "a stride is negative or step_stride < F");
  if (!(dist_thresh == dist_thresh)) return fail(me, "dist_thresh is NaN");
  if (!mode_idx || !mode_score) return fail(me, "mode_idx or mode_score is NULL");
  if (B == 0) return 0;
  if (!traj) return fail(me, "traj is NULL");
  if (B > 4ll * 0x7fffffffll) return fail(me, "too many rows");
  SelectModesArgs a{traj, group_stride, row_stride, cand_stride, step_stride, rows_per_group, B, N, T, F, t_goal, K, dist_thresh,
                    score, score_per_group ? 1 : 0, cand_valid, cand_state, state_group_stride, state_row_stride, state_cand_stride,
                    state_invalid, state_enter, row_limit, limit_stride, mode_idx, mode_score, mode_traj};
  hipLaunchKernelGGL(k_select_modes, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch(me);
}

// pred[mask] + nn.CrossEntropyLoss (infgen/model/infgen.py:147-152, :644, :655)
extern "C" int infgen_masked_cross_entropy(const float* logits, long long ld, const void* target, int target64,
                                          const unsigned char* mask, const float* weight, int R, int C, float label_smoothing,
                                          double* acc, double* scratch, void* stream) {
  const char* me = "infgen_masked_cross_entropy";
  if (R < 0) return fail(me, "R is negative");
  if (C < 1) return fail(me, "C must be at least 1");
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return fail(me, "label_smoothing must be in [0, 1]");
  if (!acc || !scratch) return fail(me, "acc or scratch is NULL");
  if (R == 0) return 0;
  if (!logits || !target || !mask) return fail(me, "logits, target or mask is NULL");
  if (ld < C) return fail(me, "row stride shorter than the row");
  const int nb = vm_blocks(R, 4);
  MaskedCeArgs a{logits, ld, target, mask, weight, R, C, label_smoothing != 0.f ? 1 : 0, scratch};
  if (target64) hipLaunchKernelGGL(k_masked_ce<true>, dim3(nb), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_masked_ce<false>, dim3(nb), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(k_vm_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)scratch, nb, 3, acc, acc + 1, acc + 2);
  return check_launch(me);
}

// TokenCls.update (infgen/utils/metrics.py:326-333)
extern "C" int infgen_token_cls(const void* pred, int pred64, long long ld_pred, int n_guess, const void* target, int target64,
                               const unsigned char* mask, int R, long long* acc, void* stream) {
  const char* me = "infgen_token_cls";
  if (R < 0 || n_guess < 0) return fail(me, "R or n_guess is negative");
  if (!acc) return fail(me, "acc is NULL");
  if (R == 0) return 0;
  if (!pred || !target || !mask) return fail(me, "pred, target or mask is NULL");
  if (ld_pred < n_guess) return fail(me, "row stride shorter than n_guess");
  TokenClsArgs a{pred, ld_pred, n_guess, target, mask, R, (unsigned long long*)acc};
  const dim3 grid(vm_blocks(R, 256));
  if (pred64 && target64) hipLaunchKernelGGL((k_token_cls<true, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else if (pred64) hipLaunchKernelGGL((k_token_cls<true, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else if (target64) hipLaunchKernelGGL((k_token_cls<false, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((k_token_cls<false, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
  return check_launch(me);
}

// AverageMeter.update (infgen/utils/metrics.py:477-479)
extern "C" int infgen_average_meter(const float* val, long long n, void* acc, double* scratch, void* stream) {
  const char* me = "infgen_average_meter";
  if (n < 0) return fail(me, "n is negative");
  if (!acc || !scratch) return fail(me, "acc or scratch is NULL");
  if (n == 0) return 0;
  if (!val) return fail(me, "val is NULL");
  const int nb = vm_blocks(n, 256 * 8);
  hipLaunchKernelGGL(k_vm_sum, dim3(nb), dim3(256), 0, (hipStream_t)stream, val, n, scratch, (unsigned long long*)acc + 1);
  hipLaunchKernelGGL(k_vm_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)scratch, nb, 1, (double*)acc,
                     (double*)nullptr, (double*)nullptr);
  return check_launch(me);
}

extern "C" int infgen_match_map_tokens(const float* traj_pos, const float* theta, const float* sample_pt, int P, int n_token,
                                      int* token_idx, void* stream) {
  if (P <= 0) return 0;
  if (n_token <= 0) return fail("infgen_match_map_tokens", "n_token must be positive");
  MatchMapArgs a{traj_pos, theta, sample_pt, P, n_token, token_idx};
  hipLaunchKernelGGL(k_match_map_tokens, dim3(ceil_div(P, 4)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("infgen_match_map_tokens");
}

// the other split families on 64-row tiles (launch_attn_h is the model)
template <bool MK> static auto heads_h_kernel(const HeadsArgs& a) {
  return a.sample_k > 1
      ? (a.token_logprob ? by_terms(k_heads_h<3, true, HEADS_KS, MK>, k_heads_h_b16<1, true, HEADS_KS, MK>, k_heads_h<1, true, HEADS_KS, MK>)
                         : by_terms(k_heads_h<3, false, HEADS_KS, MK>, k_heads_h_b16<1, false, HEADS_KS, MK>, k_heads_h<1, false, HEADS_KS, MK>))
      : (a.token_logprob ? by_terms(k_heads_h<3, true, 0, MK>, k_heads_h_b16<1, true, 0, MK>, k_heads_h<1, true, 0, MK>)
                         : by_terms(k_heads_h<3, false, 0, MK>, k_heads_h_b16<1, false, 0, MK>, k_heads_h<1, false, 0, MK>));
}
// a kernel with a <MK> instantiation pair: the unmasked one with its block as it was, or, where a mask is set, the masked one
// with the mask appended to the block
template <class KM, class KU, class A>
static void launch_masked(KM masked, KU unmasked, dim3 grid, dim3 block, const A& a, const TokenMaskCtl& mask, void* stream) {
  Masked<A> m;
  static_cast<A&>(m) = a;
  m.mask = mask;
  if (mask.bits) hipLaunchKernelGGL(masked, grid, block, 0, (hipStream_t)stream, m);
  else hipLaunchKernelGGL(unmasked, grid, block, 0, (hipStream_t)stream, a);
}
static void launch_map_head_h(const MapHeadArgs& a, void* stream) {
  hipLaunchKernelGGL(by_terms(k_map_head_h<3>, k_map_head_h_b16<1>, k_map_head_h<1>), dim3(grid64(a.rows)), dim3(256), 0, (hipStream_t)stream, a);
}
static void launch_mlpemb_h(const MlpEmbHArgs& m, void* stream) {
  ProfScope _ps(INFGEN_KID_LINEAR, stream, (double)m.rows * (m.K0 + 128 + 128) * 128.0);
  hipLaunchKernelGGL(by_terms(k_mlpemb_h<3>, k_mlpemb_h_b16<1>, k_mlpemb_h<1>), dim3(grid64(m.rows)), dim3(256), 0, (hipStream_t)stream, m);
}

// One emission: the residual stream X [rows][128] -> next_state, the motion token and up to two log-probabilities.  The first eight
// members are infgen_heads' own parameters in its order (EmitReq{X, ..., next_state}); the rest is set by name, and off where it is not
struct EmitReq {
  const float* X; int rows; const float* tok_pack; const float* st_pack; int token_size;
  float* logits;                      // optional [rows][token_size]: written when set; the plan's chain (need_logits) reads it back
  int* next_token; int* next_state;   // [rows]
  int k = 1; const float* uniform = nullptr;      // k <= 1: the arg-max (uniform, ctl and sample_logprob unused), else the top-k beam
  SamplingCtl ctl = SAMPLING_DEFAULT;             // and its draw: [rows] U[0, 1), temperature / top-p
  TokenMaskCtl mask = TOKEN_MASK_NONE;      // per-row allowed tokens of the arg-max or the draw (bits == NULL: the unmasked kernels)
  bool mask_chain_heads = false;      // heads whose arg-max k_sample_topk overwrites take the mask too (infgen_decode_step; not the entries)
  float* token_logprob = nullptr;     // optional [rows], full softmax: out of the split kernel (plan.lp_fused), else k_token_logprob over logits
  float* sample_logprob = nullptr;    // optional [rows], k > 1: log-probability of the pick under the sampler's own distribution
  unsigned long long* keys = nullptr; // optional rows x 8 bytes: with them k_heads deals the logit chunks of few row tiles to plan.ns
                                      // workgroups per tile - cleared before, decoded after (k_heads_finish) ...
  bool keys_stay = false;             // ... or neither (infgen_rollout_run's folded tail: the previous and this step's k_integrate do)
};
static EmitPlan emit_plan(const EmitReq& q) {
  return emit_plan(O().attn_mode, q.rows, q.token_size, q.k, q.token_logprob != nullptr, q.keys && !knob::heads_nosplit);
}

extern "C" int infgen_token_logprob(const float* logits, int rows, int n, const int* token, float* out, void* stream) {
  if (rows <= 0) return 0;
  if (!logits || !token || !out) return fail("infgen_token_logprob", "null pointer");
  if (n <= 0) return fail("infgen_token_logprob", "n must be positive");
  TokenLogprobArgs a{logits, rows, n, token, out};
  hipLaunchKernelGGL(k_token_logprob, dim3(ceil_div(rows, 4)), dim3(NT), 0, (hipStream_t)stream, a);
  return check_launch("infgen_token_logprob");
}

static int sample_topk_impl(const char* me, const float* logits, int rows, int n, int k, const float* uniform, int* token,
                            float* sample_logprob, const SamplingCtl& ctl, const TokenMaskCtl& mask, int* nucleus, void* stream) {
  if (rows <= 0) return 0;
  if (k < 1 || k > 16) return fail(me, "k must be in 1..16");
  if (k > n) return fail(me, "k must not exceed n");      // (the k-th pick of fewer than k logits is no token)
  SampleArgs a{logits, rows, n, k, uniform, token, sample_logprob, ctl, nucleus};
  launch_masked(k_sample_topk<true>, k_sample_topk<false>, dim3(ceil_div(rows, 4)), dim3(NT), a, mask, stream);
  return check_launch(me);
}

extern "C" int infgen_sample_topk(const float* logits, int rows, int n, int k, const float* uniform, int* token,
                                  void* stream) {
  return sample_topk_impl("infgen_sample_topk", logits, rows, n, k, uniform, token, nullptr, SAMPLING_DEFAULT, TOKEN_MASK_NONE, nullptr, stream);
}

extern "C" int infgen_sample_topk_logprob(const float* logits, int rows, int n, int k, const float* uniform, int* token,
                                          float* sample_logprob, void* stream) {
  return sample_topk_impl("infgen_sample_topk_logprob", logits, rows, n, k, uniform, token, sample_logprob, SAMPLING_DEFAULT, TOKEN_MASK_NONE, nullptr, stream);
}

// ... with temperature and nucleus truncation (sampling == NULL: infgen_sample_topk_logprob); k == 1 is the arg-max, the parameters ignored
extern "C" int infgen_sample_topk_ex(const float* logits, int rows, int n, int k, const float* uniform, const InfgenSampling* sampling,
                                     int* token, float* sample_logprob, int* nucleus, void* stream) {
  const char* me = "infgen_sample_topk_ex";
  SamplingCtl ctl = SAMPLING_DEFAULT;
  if (k > 1) RET_IF(sampling_ctl(me, sampling, &ctl));
  return sample_topk_impl(me, logits, rows, n, k, uniform, token, sample_logprob, ctl, TOKEN_MASK_NONE, nucleus, stream);
}

// ... under a token mask (mask == NULL or inactive: infgen_sample_topk_ex)
extern "C" int infgen_sample_topk_mask(const float* logits, int rows, int n, int k, const float* uniform, const InfgenSampling* sampling,
                                       const uint32_t* mask_bits, int mask_n_sets, const int* mask_row, const int* mask_type,
                                       const int* type, int* token, float* sample_logprob, int* nucleus, void* stream) {
  const char* me = "infgen_sample_topk_mask";
  SamplingCtl ctl = SAMPLING_DEFAULT;
  TokenMaskCtl mk;
  if (k > 1) RET_IF(sampling_ctl(me, sampling, &ctl));
  const TokenMaskDesc md = token_mask_desc(mask_bits, mask_n_sets, mask_row, mask_type, type);
  RET_IF(token_mask_ctl(me, &md, n, &mk));
  return sample_topk_impl(me, logits, rows, n, k, uniform, token, sample_logprob, ctl, mk, nucleus, stream);
}

// The launches the plan names, in order: [keys cleared] the heads - k_heads_h, or k_heads over ns column parts - [k_heads_finish]
// [k_sample_topk] [k_token_logprob].  The heads stage reports as infgen_heads, the log-probability as infgen_token_logprob; `me`
// names the chain's draw.  *split_used: the column split ran (with keys_stay: the keys wait for the caller's k_integrate)
static int emit_tokens(const char* me, const EmitReq& q, const EmitPlan& p, void* stream, bool* split_used = nullptr) {
  if (split_used) *split_used = false;
  if (q.rows <= 0) return 0;
  if (q.token_size % 128) return fail("infgen_heads", "token_size must be a multiple of 128");
  const bool draw_after = q.k > 1 && !p.sample_fused;
  const TokenMaskCtl& heads_mask = draw_after && !q.mask_chain_heads ? TOKEN_MASK_NONE : q.mask;
  HeadsArgs a{q.X, q.rows, q.tok_pack, q.st_pack, q.token_size, q.logits, q.next_token, q.next_state, nullptr, 1,
              p.lp_fused ? q.token_logprob : nullptr, p.sample_fused ? q.k : 0, p.sample_fused ? q.uniform : nullptr,
              p.sample_fused ? q.sample_logprob : nullptr, q.ctl};
  const bool parts = p.ns > 1, finish = parts && !q.keys_stay;
  if (parts) { a.part = q.keys; a.nsplit = p.ns; }
  if (finish && hipMemsetAsync(q.keys, 0, (size_t)q.rows * sizeof(unsigned long long), (hipStream_t)stream) != hipSuccess)
    return fail("infgen_heads", "memset failed");
  { ProfScope _ps(INFGEN_KID_HEADS, stream, heads_macs(q.rows, q.token_size));
    if (p.split) launch_masked(heads_h_kernel<true>(a), heads_h_kernel<false>(a), dim3(grid64(q.rows)), dim3(256), a, heads_mask, stream);
    else launch_masked(k_heads<true>, k_heads<false>, dim3(ceil_div(q.rows, TR), p.ns), dim3(NT), a, heads_mask, stream);
    if (finish)
      hipLaunchKernelGGL(k_heads_finish, dim3(ceil_div(q.rows, NT)), dim3(NT), 0, (hipStream_t)stream, q.keys, q.rows, q.next_token); }
  if (split_used) *split_used = parts;
  RET_IF(check_launch("infgen_heads"));
  if (draw_after)
    RET_IF(sample_topk_impl(me, q.logits, q.rows, q.token_size, q.k, q.uniform, q.next_token, q.sample_logprob, q.ctl, q.mask, nullptr, stream));
  if (q.token_logprob && !p.lp_fused) RET_IF(infgen_token_logprob(q.logits, q.rows, q.token_size, q.next_token, q.token_logprob, stream));
  return 0;
}
// the stand-alone entries: the plan under the caller's switches, refused where its chain would read logits the caller did not pass
static int emit_entry(const char* me, const EmitReq& q, void* stream) {
  const EmitPlan p = emit_plan(q);
  if (p.need_logits && !q.logits)
    return fail(me, q.k > 1 ? "this row count or beam takes k_sample_topk: it needs a logits buffer [rows][token_size]"
                            : "this row count takes k_heads: it needs a logits buffer [rows][token_size]");
  return emit_tokens(me, q, p, stream);
}

extern "C" int infgen_heads(const float* X, int rows, const float* tok_pack, const float* st_pack, int token_size,
                            float* logits, int* next_token, int* next_state, void* stream) {
  return emit_entry("infgen_heads", EmitReq{X, rows, tok_pack, st_pack, token_size, logits, next_token, next_state}, stream);
}

// infgen_heads + the log-probability of next_token: out of the split kernel where the plan says so (logits optional), otherwise
// k_heads into the caller's logits and k_token_logprob over them
extern "C" int infgen_heads_logprob(const float* X, int rows, const float* tok_pack, const float* st_pack, int token_size,
                                    float* logits, int* next_token, int* next_state, float* token_logprob, void* stream) {
  if (rows <= 0) return 0;
  if (!token_logprob) return fail("infgen_heads_logprob", "token_logprob is NULL (infgen_heads is the entry without it)");
  EmitReq q{X, rows, tok_pack, st_pack, token_size, logits, next_token, next_state};
  q.token_logprob = token_logprob;
  return emit_entry("infgen_heads_logprob", q, stream);
}

// infgen_heads with the motion token drawn by top-k sampling (k_sample_topk's order and arithmetic) and, optionally, its two
// log-probabilities: one launch where the plan draws inside the split kernel (logits optional); elsewhere heads into the caller's
// logits, k_sample_topk and k_token_logprob over them.  k == 1 is the arg-max (the greedy variant): a point mass, and log 1
static int heads_sample_impl(const char* me, EmitReq q, const InfgenSampling* sampling, const TokenMaskDesc* mask, void* stream) {
  if (q.rows <= 0) return 0;
  if (mask && q.k < 1) q.k = 1;      // (infgen_heads_sample_mask: k <= 1 is the masked arg-max)
  if (q.k < 1 || q.k > 16) return fail(me, "k must be in 1..16");
  if (q.k > q.token_size) return fail(me, "k must not exceed token_size");
  if (!q.uniform && !(mask && q.k == 1)) return fail(me, "uniform is NULL");
  RET_IF(token_mask_ctl(me, mask, q.token_size, &q.mask));
  if (q.k == 1) {
    if (q.sample_logprob && hipMemsetAsync(q.sample_logprob, 0, (size_t)q.rows * sizeof(float), (hipStream_t)stream) != hipSuccess)
      return fail(me, "memset failed");
    if (q.token_logprob && !q.mask.bits)      // (unmasked: infgen_heads_logprob itself, its refusals under its own name)
      return infgen_heads_logprob(q.X, q.rows, q.tok_pack, q.st_pack, q.token_size, q.logits, q.next_token, q.next_state, q.token_logprob, stream);
  } else RET_IF(sampling_ctl(me, sampling, &q.ctl));
  return emit_entry(me, q, stream);
}

extern "C" int infgen_heads_sample(const float* X, int rows, const float* tok_pack, const float* st_pack, int token_size, int k,
                                   const float* uniform, float* logits, int* next_token, int* next_state, float* token_logprob,
                                   float* sample_logprob, void* stream) {
  EmitReq q{X, rows, tok_pack, st_pack, token_size, logits, next_token, next_state};
  q.k = k; q.uniform = uniform; q.token_logprob = token_logprob; q.sample_logprob = sample_logprob;
  return heads_sample_impl("infgen_heads_sample", q, nullptr, nullptr, stream);
}

// ... with temperature and nucleus truncation (the same draw: topk_inverse_cdf of kernels.h, inside the split kernel or after it)
extern "C" int infgen_heads_sample_ex(const float* X, int rows, const float* tok_pack, const float* st_pack, int token_size, int k,
                                      const float* uniform, const InfgenSampling* sampling, float* logits, int* next_token,
                                      int* next_state, float* token_logprob, float* sample_logprob, void* stream) {
  EmitReq q{X, rows, tok_pack, st_pack, token_size, logits, next_token, next_state};
  q.k = k; q.uniform = uniform; q.token_logprob = token_logprob; q.sample_logprob = sample_logprob;
  return heads_sample_impl("infgen_heads_sample_ex", q, sampling, nullptr, stream);
}

// ... under a token mask (mask == NULL or inactive: infgen_heads_sample_ex); k <= 1 is the masked arg-max
extern "C" int infgen_heads_sample_mask(const float* X, int rows, const float* tok_pack, const float* st_pack, int token_size, int k,
                                        const float* uniform, const InfgenSampling* sampling, const uint32_t* mask_bits,
                                        int mask_n_sets, const int* mask_row, const int* mask_type, const int* type, float* logits,
                                        int* next_token, int* next_state, float* token_logprob, float* sample_logprob, void* stream) {
  const TokenMaskDesc md = token_mask_desc(mask_bits, mask_n_sets, mask_row, mask_type, type);
  if (mask_n_sets < 0) return fail("infgen_heads_sample_mask", "token mask: n_sets must be >= 0");
  EmitReq q{X, rows, tok_pack, st_pack, token_size, logits, next_token, next_state};
  q.k = k; q.uniform = uniform; q.token_logprob = token_logprob; q.sample_logprob = sample_logprob;
  // (no table: infgen_heads_sample_ex, its argument checks included)
  return heads_sample_impl("infgen_heads_sample_mask", q, sampling, mask_bits ? &md : nullptr, stream);
}

// the map encoder's token_predict_head (map_decoder.py:119-121) on the rows gather[k] of X.  Split arithmetic (k_map_head_h: one
// launch, the ranking fused) under gemm_terms 1 / 2 and where attn_split picks it; otherwise the fp32 MFMA path of infgen_heads'
// by-size rule: two k_linear launches through `hidden` [n][128] and k_map_topk
extern "C" int infgen_map_token_head(const float* X, int ldx, const int* gather, int n, const float* pack, int token_size,
                                     float* hidden, float* logits, long long* top_idx, void* stream) {
  if (n <= 0) return 0;
  if (token_size != MAP_HEAD_N) return fail("infgen_map_token_head", "token_size must be 1024 (map_decoder.py:58)");
  if (!X || !gather || !pack || !logits || !top_idx || ldx < D || ldx % 4)
    return fail("infgen_map_token_head", "null pointer, or ldx not a multiple of 4 of at least 128");
  MapHeadArgs a{X, ldx, gather, n, pack, logits, top_idx};
  const hipStream_t s = (hipStream_t)stream;
  ProfScope _ps(INFGEN_KID_MAP_HEAD, stream, (double)n * (16384.0 + 128.0 * token_size));
  if (!three_terms() || attn_split(n)) {
    launch_map_head_h(a, stream);
    return check_launch("infgen_map_token_head");
  }
  if (!hidden) return fail("infgen_map_token_head", "the fp32 path needs hidden [n][128]");
  const int W3 = 16768, tiles = ceil_div(n, TR), passes = token_size / 128;
  LinearArgs l0{X, ldx, gather, n, D, D, pack, D, pack + 16384, D, nullptr, nullptr, pack + 16512, pack + 16640, 1, hidden, D};
  hipLaunchKernelGGL(k_linear, dim3(tiles), dim3(NT), 0, s, l0);
  LinearArgs l1{hidden, D, nullptr, n, D, D, pack + W3, token_size, pack + W3 + (size_t)128 * token_size, token_size,
                nullptr, nullptr, nullptr, nullptr, 0, logits, token_size};
  const int gy = tiles < 512 ? min(passes, ceil_div(512, tiles)) : 1;
  hipLaunchKernelGGL(k_linear, dim3(tiles, gy), dim3(NT), 0, s, l1);
  hipLaunchKernelGGL(k_map_topk, dim3(ceil_div(n, 4)), dim3(256), 0, s, a);
  return check_launch("infgen_map_token_head");
}

extern "C" int infgen_embedding_sum4(const float* tab0, const long long* idx0, int n0, const float* tab1, const long long* idx1, int n1,
                                     const float* tab2, const long long* idx2, int n2, const float* tab3, const long long* idx3, int n3,
                                     int rows, float* out, void* stream) {
  if (rows <= 0) return 0;
  if (!tab0 || !tab1 || !tab2 || !tab3 || !idx0 || !idx1 || !idx2 || !idx3 || !out || n0 < 1 || n1 < 1 || n2 < 1 || n3 < 1)
    return fail("infgen_embedding_sum4", "null table / index array or empty table");
  EmbedSum4Args a{{tab0, tab1, tab2, tab3}, {idx0, idx1, idx2, idx3}, {n0, n1, n2, n3}, rows, out};
  hipLaunchKernelGGL(k_embedding_sum4, dim3((unsigned)(((long long)rows * 32 + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, a);
  return check_launch("infgen_embedding_sum4");
}

extern "C" int infgen_map_graph(int S, int M_cap, const int* n_map, const float* pos, const float* orient,
                                float radius, int max_nbr, int* off, int* cnt, int* src, float* raw, int* total,
                                int cap, void* stream) {
  if (S <= 0 || M_cap <= 0) return 0;
  if (hipMemsetAsync(total, 0, sizeof(int), (hipStream_t)stream) != hipSuccess)
    return fail("infgen_map_graph", "memset failed");
  MapGraphArgs a{S, M_cap, n_map, pos, orient, radius, max_nbr, EdgeBuf{off, cnt, src, raw, total, cap}, 0};
  a.lds_tokens = (M_cap <= 4096 && M_cap % (4 * MAP_GRAPH_C) == 0) ? M_cap : 0;      // (else: the global-memory scan)
  { ProfScope _ps(INFGEN_KID_MAP_GRAPH, stream);
    hipLaunchKernelGGL(k_map_graph, dim3(ceil_div(S * M_cap, 4 * MAP_GRAPH_C)), dim3(NT), (size_t)a.lds_tokens * 12, (hipStream_t)stream, a); }
  return check_launch("infgen_map_graph");
}

// ---------------------------------------------------------------------------------- step riders: the scene they read
// the one args builder of the step riders and the closed-loop operators.  head: the scene as a stand-alone entry's parameters or a
// context give it - a SceneHead, or a mask rider's MaskHead (mask_head below); k: the configuration, which adds the shape, the rule
// and a mask rider's tables (NoCfg: an operator without one, whose head brings the shape).  What a block holds beyond these - a
// step, an output of the rider's own - its launch sets
struct NoCfg {};
template <class A, class Head, class Cfg = NoCfg> static A rider_args(const Head& head, const Cfg& k = Cfg{}) {
  A a{};
  static_cast<Head&>(a) = head;
  if constexpr (!std::is_same_v<Cfg, NoCfg>) {
    a.shape = k.shape;
    static_cast<decltype(Cfg::rule)&>(a) = k.rule;
  }
  if constexpr (std::is_same_v<Head, MaskHead>) { a.end_pose = k.end_pose; a.out_bits = k.bits; a.out_count = k.count; }
  return a;
}
static SceneHead scene_head(const InfgenRollout* r) {
  return SceneHead{r->S, r->A_cap, r->T, r->pos, r->head, r->state, r->n_agents, r->type, nullptr};
}
// column c of a scene under the sets `base`, for a mask rider to refine
static MaskHead mask_head(const SceneHead& sc, int c, const int* first_new, int token_size, const TokenMaskCtl& base) {
  MaskHead h{};
  static_cast<SceneHead&>(h) = sc;
  h.c = c; h.first_new = first_new; h.token_size = token_size; h.base = base;
  return h;
}
// ... as a stand-alone entry's parameters name it: the static mask comes as the C ABI passes it
static int entry_head(const char* me, const SceneHead& sc, int c, const int* first_new, int token_size, const uint32_t* mask_bits,
                      int mask_n_sets, const int* mask_row, const int* mask_type, MaskHead* out) {
  const TokenMaskDesc md = token_mask_desc(mask_bits, mask_n_sets, mask_row, mask_type, sc.type);
  TokenMaskCtl base;
  RET_IF(token_mask_ctl(me, &md, token_size, &base));
  *out = mask_head(sc, c, first_new, token_size, base);
  return 0;
}

// a mask rider's name in the error texts, and which of the optional geometry checks its launches make
enum { GEO_CAP = 1, GEO_ROWS = 2 };
struct MaskKind { const char* prefix; int checks; };
constexpr MaskKind COLLISION_KIND{"collision mask: ", GEO_CAP}, ROAD_KIND{"road mask: ", GEO_ROWS},
    ROUTE_KIND{"route mask: ", GEO_CAP | GEO_ROWS}, SIGNAL_KIND{"signal mask: ", GEO_CAP | GEO_ROWS};
constexpr const char* TOKEN_SIZE_UNFIT = "token_size must be a multiple of 32, at most 4096";
static bool token_size_unfit(int token_size) { return token_size % 32 || token_size > 64 * 32 * RIDER_WPL; }
// the one geometry check of a mask rider's launch (copies: 1 for a rider without scene groups)
static int mask_geometry(const char* where, const MaskKind& k, const MaskHead& a, int copies) {
  if (a.S <= 0 || a.A_cap <= 0 || a.T <= 0) return fail(where, k.prefix, "S, A_cap and T must be positive");
  if ((k.checks & GEO_CAP) && a.A_cap > MAX_SCENE_AGENTS) return fail(where, k.prefix, "A_cap exceeds INFGEN_Q_MAX_AGENTS");
  if (a.S % copies) return fail(where, k.prefix, "S must be a multiple of copies");
  if (a.c < 0 || a.c >= a.T) return fail(where, k.prefix, "column outside [0, T)");
  if (a.token_size <= 0 || token_size_unfit(a.token_size)) return fail(where, k.prefix, TOKEN_SIZE_UNFIT);
  if (!a.pos || !a.head || !a.state || !a.n_agents || !a.type) return fail(where, k.prefix, "null scene array");
  if ((k.checks & GEO_ROWS) && (long long)a.S * a.A_cap > 0x7fffffffLL) return fail(where, k.prefix, "too many rows");
  return 0;
}
// what validate asks of a context that carries the rider
static int mask_fits(const char* where, const MaskKind& k, const InfgenRollout* r, int copies) {
  if (token_size_unfit(r->token_size)) return fail(where, k.prefix, TOKEN_SIZE_UNFIT);
  if (r->S % copies) return fail(where, k.prefix, "S must be a multiple of copies");
  return 0;
}
// the launch of a kernel that takes the S * A_cap rows of the layout one wave each
template <class A> static int launch_rows(const char* where, void (*kernel)(A), const A& a, void* stream) {
  const long long rows = (long long)a.S * a.A_cap;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + RIDER_WAVES - 1) / RIDER_WAVES)), dim3(64 * RIDER_WAVES), 0, (hipStream_t)stream, a);
  return check_launch(where);
}
// the three-entry type switch a configuration holds by value (NULL: the check that follows refuses it)
static const int* types_or_zeros(const int* types) {
  static const int zeros[3] = {0, 0, 0};
  return types ? types : zeros;
}
static bool misaligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 15) != 0;
}

// Every rider below has the same parts.  x_check: what include/infgen_hip.h asks of a configuration (types: the caller's pointer
// behind rule.types); x_cfg: the one place a configuration is built and checked - by the stand-alone entry (ident NULL) and when it
// is attached to a handle, so a launch meets checked configurations only; launch_mask / launch_score: the geometry and the one
// launch of the kernel (t: the decode step, which the signal rule reads)
// ---------------------------------------------------------------------------------- collision masks
static int collision_check(const char* where, const CollisionCfg& k) {
  if (!std::isfinite(k.rule.margin) || k.rule.margin < 0.f) return fail(where, "collision mask: margin must be finite and >= 0");
  if (k.rule.predict != 0 && k.rule.predict != 1) return fail(where, "collision mask: predict must be 0 or 1");
  if (!k.shape) return fail(where, "collision mask: needs the rows' shape array [S][A_cap][3]");
  if (!k.end_pose) return fail(where, "collision mask: needs the end-pose table of infgen_collision_end_poses");
  if (!k.bits) return fail(where, "collision mask: needs the output table");
  if (misaligned16(k.bits, k.end_pose)) return fail(where, "collision mask: the tables must be 16-byte aligned");
  return 0;
}
static int collision_cfg(const char* where, uint32_t* bits, const int* ident, const float* shape, const float* end_pose, int predict,
                         float margin, int* count, CollisionCfg* out) {
  *out = CollisionCfg{bits, ident, shape, end_pose, {predict, margin}, count};
  return collision_check(where, *out);
}
static int launch_mask(const char* where, const MaskHead& h, const CollisionCfg& k, int t, void* stream) {
  RET_IF(mask_geometry(where, COLLISION_KIND, h, 1));
  CollisionArgs a = rider_args<CollisionArgs>(h, k);
  // few rows: one row per wave and workgroup round; many: 16 rows share one staging of their scene's obstacles
  int per = knob::cm_rows > 0 ? knob::cm_rows : ((long long)a.S * a.A_cap > 4096 ? 4 * RIDER_WAVES : RIDER_WAVES);
  per = ceil_div(per, RIDER_WAVES) * RIDER_WAVES;
  a.rows_per_wg = per;
  const size_t lds = (size_t)RIDER_WAVES * 2 * RIDER_LIST * sizeof(float4) + (size_t)CM_STAGE * a.A_cap * sizeof(float);
  hipLaunchKernelGGL(k_collision_mask, dim3(ceil_div(a.A_cap, per), a.S), dim3(64 * RIDER_WAVES), lds, (hipStream_t)stream, a);
  return check_launch(where);
}

extern "C" int infgen_collision_end_poses(const float* vocab, int token_size, float* end_pose, void* stream) {
  const char* me = "infgen_collision_end_poses";
  if (!vocab || !end_pose) return fail(me, "null pointer");
  if (token_size <= 0) return fail(me, "token_size must be positive");
  if ((reinterpret_cast<uintptr_t>(vocab) | reinterpret_cast<uintptr_t>(end_pose)) & 15) return fail(me, "the tables must be 16-byte aligned");
  hipLaunchKernelGGL(k_collision_end_poses, dim3(3), dim3(256), 0, (hipStream_t)stream, EndPoseArgs{vocab, token_size, end_pose});
  return check_launch(me);
}

extern "C" int infgen_collision_mask(const float* pos, const float* head, const int* state, const int* n_agents, const int* first_new,
                                     const int* type, const float* shape, int S, int A_cap, int T, int c, const float* end_pose,
                                     int token_size, int predict, float margin, const uint32_t* mask_bits, int mask_n_sets,
                                     const int* mask_row, const int* mask_type, uint32_t* out_bits, int* out_count, void* stream) {
  const char* me = "infgen_collision_mask";
  MaskHead h;
  RET_IF(entry_head(me, SceneHead{S, A_cap, T, pos, head, state, n_agents, type}, c, first_new, token_size, mask_bits, mask_n_sets, mask_row,
                    mask_type, &h));
  CollisionCfg cfg;
  RET_IF(collision_cfg(me, out_bits, nullptr, shape, end_pose, predict, margin, out_count, &cfg));
  return launch_mask(me, h, cfg, 0, stream);
}

extern "C" int infgen_token_mask_collision(int handle, uint32_t* dyn_bits, const int* identity_row, const float* shape,
                                           const float* end_pose, int predict, float margin, int* count) {
  const char* me = "infgen_token_mask_collision";
  CollisionCfg cfg = COLLISION_NONE;
  if (dyn_bits) {
    RET_IF(collision_cfg(me, dyn_bits, identity_row, shape, end_pose, predict, margin, count, &cfg));
    if (!identity_row) return fail(me, "collision mask: needs the identity selectors [S * A_cap]");
  }
  return with_mask_slot(me, handle, NO_TOKEN_MASK, [&](TokenMaskSlot& s) { s.cfg.coll = cfg; });
}

// ---------------------------------------------------------------------------------- road masks
// what road masks and step scores ask alike of a configuration that reads the road table, in the order both ask it.  (Each keeps
// its margin check in front of this - the scores' dt check sits between the two - and its types check behind its own pointers')
template <class Rule> static int road_table_check(const char* where, const char* prefix, const Rule& r, const float* shape) {
  const char* what = r.sweep != 0 && r.sweep != 1 ? "sweep must be 0 or 1" : r.copies < 1 ? "copies must be at least 1"
                     : r.rec_cap < 0 ? "negative record capacity" : !shape ? "needs the rows' shape array [S][A_cap][3]" : nullptr;
  return what ? fail(where, prefix, what) : 0;
}
static int road_check(const char* where, const RoadCfg& k, const int* types) {
  if (!std::isfinite(k.rule.margin) || k.rule.margin < 0.f) return fail(where, "road mask: margin must be finite and >= 0");
  RET_IF(road_table_check(where, "road mask: ", k.rule, k.shape));
  if (!k.end_pose) return fail(where, "road mask: needs the end-pose table of infgen_collision_end_poses");
  if (!k.rule.paths) return fail(where, "road mask: needs the path table of infgen_road_paths");
  if (!k.rule.records || !k.rule.n_records) return fail(where, "road mask: needs the record table and its counts");
  if (!types) return fail(where, "road mask: needs the three-entry type switch");
  if (!k.bits) return fail(where, "road mask: needs the output table");
  if (misaligned16(k.bits, k.end_pose, k.rule.paths, k.rule.records)) return fail(where, "road mask: the tables must be 16-byte aligned");
  return 0;
}
static int road_cfg(const char* where, uint32_t* bits, const int* ident, const float* shape, const float* end_pose, const float* paths,
                    const float* records, const int* n_records, int rec_cap, int copies, int sweep, float margin, const int* types,
                    int* count, RoadCfg* out) {
  const int* ty = types_or_zeros(types);
  *out = RoadCfg{bits, ident, shape, end_pose, {paths, records, n_records, rec_cap, copies, sweep, margin, {ty[0], ty[1], ty[2]}}, count};
  return road_check(where, *out, types);
}
static int launch_mask(const char* where, const MaskHead& h, const RoadCfg& k, int t, void* stream) {
  RET_IF(mask_geometry(where, ROAD_KIND, h, k.rule.copies));
  return launch_rows(where, k_road_mask, rider_args<RoadArgs>(h, k), stream);
}

extern "C" int infgen_road_records_from_map(const float* map_pos, const float* map_orient, const long long* map_type, const long long* map_tok,
                                            const int* n_map, int S0, int M_cap, const float* map_vocab, int n_token, int detail,
                                            float* records, int rec_cap, int* n_records, void* stream) {
  const char* me = "infgen_road_records_from_map";
  if (!map_pos || !map_orient || !map_type || !map_tok || !n_map || !map_vocab || !records || !n_records) return fail(me, "null pointer");
  if (detail != 1 && detail != 2 && detail != 5 && detail != 10) return fail(me, "road mask: detail must be 1, 2, 5 or 10");
  if (S0 <= 0 || M_cap <= 0 || n_token <= 0 || rec_cap <= 0) return fail(me, "S0, M_cap, n_token and rec_cap must be positive");
  if (misaligned16(records)) return fail(me, "road mask: the tables must be 16-byte aligned");
  hipLaunchKernelGGL(k_road_records_map, dim3(S0), dim3(64), 0, (hipStream_t)stream,
                     RoadMapArgs{map_pos, map_orient, map_type, map_tok, n_map, M_cap, map_vocab, n_token, detail, records, rec_cap, n_records});
  return check_launch(me);
}

extern "C" int infgen_road_records_from_segments(const float* segments, const int* n_segments, int S0, int E, float* records, int rec_cap,
                                                 int* n_records, void* stream) {
  const char* me = "infgen_road_records_from_segments";
  if (!segments || !n_segments || !records || !n_records) return fail(me, "null pointer");
  if (S0 <= 0 || E <= 0 || rec_cap <= 0) return fail(me, "S0, E and rec_cap must be positive");
  if (misaligned16(records, segments)) return fail(me, "road mask: the tables must be 16-byte aligned");
  hipLaunchKernelGGL(k_road_records_seg, dim3(S0), dim3(256), 0, (hipStream_t)stream, RoadSegArgs{segments, n_segments, E, records, rec_cap, n_records});
  return check_launch(me);
}

extern "C" int infgen_road_paths(const float* end_pose, int token_size, float* paths, void* stream) {
  const char* me = "infgen_road_paths";
  if (!end_pose || !paths) return fail(me, "null pointer");
  if (token_size <= 0) return fail(me, "token_size must be positive");
  if (misaligned16(end_pose, paths)) return fail(me, "road mask: the tables must be 16-byte aligned");
  hipLaunchKernelGGL(k_road_paths, dim3(ceil_div(3 * token_size, 256)), dim3(256), 0, (hipStream_t)stream, RoadPathArgs{end_pose, token_size, paths});
  return check_launch(me);
}

extern "C" int infgen_road_mask(const float* pos, const float* head, const int* state, const int* n_agents, const int* first_new,
                                const int* type, const float* shape, int S, int A_cap, int T, int c, const float* end_pose,
                                const float* paths, int token_size, const float* records, const int* n_records, int rec_cap, int copies,
                                int sweep, float margin, const int* types, const uint32_t* mask_bits, int mask_n_sets,
                                const int* mask_row, const int* mask_type, uint32_t* out_bits, int* out_count, void* stream) {
  const char* me = "infgen_road_mask";
  RoadCfg cfg;
  RET_IF(road_cfg(me, out_bits, nullptr, shape, end_pose, paths, records, n_records, rec_cap, copies, sweep, margin, types, out_count, &cfg));
  MaskHead h;
  RET_IF(entry_head(me, SceneHead{S, A_cap, T, pos, head, state, n_agents, type}, c, first_new, token_size, mask_bits, mask_n_sets, mask_row,
                    mask_type, &h));
  return launch_mask(me, h, cfg, 0, stream);
}

extern "C" int infgen_token_mask_road(int handle, uint32_t* road_bits, const int* identity_row, const float* shape, const float* end_pose,
                                      const float* paths, const float* records, const int* n_records, int rec_cap, int copies, int sweep,
                                      float margin, const int* types, int* count) {
  const char* me = "infgen_token_mask_road";
  RoadCfg cfg = ROAD_NONE;
  if (road_bits) {
    RET_IF(road_cfg(me, road_bits, identity_row, shape, end_pose, paths, records, n_records, rec_cap, copies, sweep, margin, types, count, &cfg));
    if (!identity_row) return fail(me, "road mask: needs the identity selectors [S * A_cap]");
  }
  return with_mask_slot(me, handle, NO_TOKEN_MASK, [&](TokenMaskSlot& s) { s.cfg.road = cfg; });
}

// ---------------------------------------------------------------------------------- route masks
static int route_check(const char* where, const RouteCfg& k, const int* types) {
  const RouteRule& r = k.rule;
  if (!std::isfinite(r.corridor) || r.corridor < 0.f) return fail(where, "route mask: corridor must be finite and >= 0");
  if (!std::isfinite(r.back) || r.back < 0.f) return fail(where, "route mask: back must be finite and >= 0");
  if (!std::isfinite(r.finish) || r.finish < 0.f) return fail(where, "route mask: finish must be finite and >= 0");
  if (!(r.pace >= 0.f && r.pace <= 1.f)) return fail(where, "route mask: pace must be in [0, 1]");
  if (r.P < 2 || r.P > RT_MAX_POINTS) return fail(where, "route mask: P must be in 2..32");
  if (r.copies < 1) return fail(where, "route mask: copies must be at least 1");
  if (!k.shape) return fail(where, "route mask: needs the rows' shape array [S][A_cap][3]");
  if (!k.end_pose) return fail(where, "route mask: needs the end-pose table of infgen_collision_end_poses");
  if (!r.records || !r.total) return fail(where, "route mask: needs the record table and the routes' lengths");
  if (!types) return fail(where, "route mask: needs the three-entry type switch");
  if (!k.bits) return fail(where, "route mask: needs the output table");
  if (misaligned16(k.bits, k.end_pose, r.records, k.progress)) return fail(where, "route mask: the tables must be 16-byte aligned");
  return 0;
}
static int route_cfg(const char* where, uint32_t* bits, const int* ident, const float* shape, const float* end_pose, const float* records,
                     const float* total, int P, int copies, float corridor, float back, float pace, float finish, const int* types,
                     int* count, float* progress, RouteCfg* out) {
  const int* ty = types_or_zeros(types);
  *out = RouteCfg{bits, ident, shape, end_pose, {records, total, P, copies, corridor, back, pace, finish, {ty[0], ty[1], ty[2]}}, count, progress};
  return route_check(where, *out, types);
}
static int launch_mask(const char* where, const MaskHead& h, const RouteCfg& k, int t, void* stream) {
  RET_IF(mask_geometry(where, ROUTE_KIND, h, k.rule.copies));
  RouteArgs a = rider_args<RouteArgs>(h, k);
  a.out_progress = k.progress;
  return launch_rows(where, k_route_mask, a, stream);
}

extern "C" int infgen_route_records(const float* routes, const int* n_points, int S, int A_cap, int P, float* records, float* total,
                                    void* stream) {
  const char* me = "infgen_route_records";
  if (!routes || !n_points || !records || !total) return fail(me, "null pointer");
  if (P < 2 || P > RT_MAX_POINTS) return fail(me, "route mask: P must be in 2..32");
  if (S <= 0 || A_cap <= 0) return fail(me, "S and A_cap must be positive");
  if (A_cap > MAX_SCENE_AGENTS) return fail(me, "route mask: A_cap exceeds INFGEN_Q_MAX_AGENTS");
  if (misaligned16(records)) return fail(me, "route mask: the tables must be 16-byte aligned");
  const long long rows = (long long)S * A_cap;
  if (rows > 0x7fffffffLL) return fail(me, "route mask: too many rows");
  hipLaunchKernelGGL(k_route_records, dim3((unsigned)((rows + RIDER_WAVES - 1) / RIDER_WAVES)), dim3(64 * RIDER_WAVES), 0, (hipStream_t)stream,
                     RouteRecArgs{routes, n_points, (int)rows, P, records, total});
  return check_launch(me);
}

extern "C" int infgen_route_mask(const float* pos, const float* head, const int* state, const int* n_agents, const int* first_new,
                                 const int* type, const float* shape, int S, int A_cap, int T, int c, const float* end_pose,
                                 int token_size, const float* records, const float* total, int P, int copies, float corridor, float back,
                                 float pace, float finish, const int* types, const uint32_t* mask_bits, int mask_n_sets,
                                 const int* mask_row, const int* mask_type, uint32_t* out_bits, int* out_count, float* out_progress,
                                 void* stream) {
  const char* me = "infgen_route_mask";
  RouteCfg cfg;
  RET_IF(route_cfg(me, out_bits, nullptr, shape, end_pose, records, total, P, copies, corridor, back, pace, finish, types, out_count,
                   out_progress, &cfg));
  MaskHead h;
  RET_IF(entry_head(me, SceneHead{S, A_cap, T, pos, head, state, n_agents, type}, c, first_new, token_size, mask_bits, mask_n_sets, mask_row,
                    mask_type, &h));
  return launch_mask(me, h, cfg, 0, stream);
}

extern "C" int infgen_token_mask_route(int handle, uint32_t* route_bits, const int* identity_row, const float* shape, const float* end_pose,
                                       const float* records, const float* total, int P, int copies, float corridor, float back, float pace,
                                       float finish, const int* types, int* count, float* progress) {
  const char* me = "infgen_token_mask_route";
  RouteCfg cfg = ROUTE_NONE;
  if (route_bits) {
    RET_IF(route_cfg(me, route_bits, identity_row, shape, end_pose, records, total, P, copies, corridor, back, pace, finish, types, count,
                     progress, &cfg));
    if (!identity_row) return fail(me, "route mask: needs the identity selectors [S * A_cap]");
  }
  return with_mask_slot(me, handle, NO_TOKEN_MASK, [&](TokenMaskSlot& s) { s.cfg.route = cfg; });
}

// ---------------------------------------------------------------------------------- signal masks
static int signal_check(const char* where, const SignalCfg& k, const int* types) {
  const SignalRule& r = k.rule;
  if (!std::isfinite(r.setback) || r.setback < 0.f) return fail(where, "signal mask: setback must be finite and >= 0");
  if (!(r.align >= -1.f && r.align <= 1.f)) return fail(where, "signal mask: align must be in [-1, 1]");
  if (r.K < 1 || r.K > SG_MAX_LINES) return fail(where, "signal mask: K must be in 1..64");
  if (r.n_phase < 1) return fail(where, "signal mask: n_phase must be at least 1");
  if (r.copies < 1) return fail(where, "signal mask: copies must be at least 1");
  if (!k.shape) return fail(where, "signal mask: needs the rows' shape array [S][A_cap][3]");
  if (!k.end_pose) return fail(where, "signal mask: needs the end-pose table of infgen_collision_end_poses");
  if (!r.records || !r.phase) return fail(where, "signal mask: needs the record table and the phase table");
  if (!types) return fail(where, "signal mask: needs the three-entry type switch");
  if (!k.bits) return fail(where, "signal mask: needs the output table");
  if (misaligned16(k.bits, k.end_pose, r.records, k.info)) return fail(where, "signal mask: the tables must be 16-byte aligned");
  return 0;
}
static int signal_cfg(const char* where, uint32_t* bits, const int* ident, const float* shape, const float* end_pose, const float* records,
                      const unsigned char* phase, int n_phase, int K, int copies, float setback, float align, const int* types, int* count,
                      float* info, SignalCfg* out) {
  const int* ty = types_or_zeros(types);
  *out = SignalCfg{bits, ident, shape, end_pose, {records, phase, n_phase, K, copies, setback, align, {ty[0], ty[1], ty[2]}}, count, info};
  return signal_check(where, *out, types);
}
static int launch_mask(const char* where, const MaskHead& h, const SignalCfg& k, int t, void* stream) {
  if (t < 0) return fail(where, "signal mask: step t must be >= 0");
  RET_IF(mask_geometry(where, SIGNAL_KIND, h, k.rule.copies));
  SignalArgs a = rider_args<SignalArgs>(h, k);
  a.t = t; a.out_info = k.info;
  return launch_rows(where, k_signal_mask, a, stream);
}

extern "C" int infgen_signal_records(const float* lines, const int* n_lines, int S0, int K, float* records, void* stream) {
  const char* me = "infgen_signal_records";
  if (!lines || !n_lines || !records) return fail(me, "signal mask: null pointer");
  if (K < 1 || K > SG_MAX_LINES) return fail(me, "signal mask: K must be in 1..64");
  if (S0 <= 0) return fail(me, "signal mask: S0 must be positive");
  if (misaligned16(lines, records)) return fail(me, "signal mask: the tables must be 16-byte aligned");
  const long long n = (long long)S0 * K;
  if (n > 0x7fffffffLL) return fail(me, "signal mask: too many lines");
  const int nt = 64 * RIDER_WAVES;
  hipLaunchKernelGGL(k_signal_records, dim3((unsigned)((n + nt - 1) / nt)), dim3(nt), 0, (hipStream_t)stream,
                     SignalRecArgs{lines, n_lines, S0, K, records});
  return check_launch(me);
}

extern "C" int infgen_signal_mask(const float* pos, const float* head, const int* state, const int* n_agents, const int* first_new,
                                  const int* type, const float* shape, int S, int A_cap, int T, int c, const float* end_pose,
                                  int token_size, const float* records, const unsigned char* phase, int n_phase, int K, int t, int copies,
                                  float setback, float align, const int* types, const uint32_t* mask_bits, int mask_n_sets,
                                  const int* mask_row, const int* mask_type, uint32_t* out_bits, int* out_count, float* out_info,
                                  void* stream) {
  const char* me = "infgen_signal_mask";
  SignalCfg cfg;
  RET_IF(signal_cfg(me, out_bits, nullptr, shape, end_pose, records, phase, n_phase, K, copies, setback, align, types, out_count, out_info,
                    &cfg));
  MaskHead h;
  RET_IF(entry_head(me, SceneHead{S, A_cap, T, pos, head, state, n_agents, type}, c, first_new, token_size, mask_bits, mask_n_sets, mask_row,
                    mask_type, &h));
  return launch_mask(me, h, cfg, t, stream);
}

extern "C" int infgen_token_mask_signal(int handle, uint32_t* signal_bits, const int* identity_row, const float* shape,
                                        const float* end_pose, const float* records, const unsigned char* phase, int n_phase, int K,
                                        int copies, float setback, float align, const int* types, int* count, float* info) {
  const char* me = "infgen_token_mask_signal";
  SignalCfg cfg = SIGNAL_NONE;
  if (signal_bits) {
    RET_IF(signal_cfg(me, signal_bits, identity_row, shape, end_pose, records, phase, n_phase, K, copies, setback, align, types, count, info,
                      &cfg));
    if (!identity_row) return fail(me, "signal mask: needs the identity selectors [S * A_cap]");
  }
  return with_mask_slot(me, handle, NO_TOKEN_MASK, [&](TokenMaskSlot& s) { s.cfg.signal = cfg; });
}

// ---------------------------------------------------------------------------------- step scores
static int score_check(const char* where, const ScoreCfg& k, const int* types) {
  const ScoreRule& r = k.rule;
  if (!std::isfinite(r.margin) || r.margin < 0.f) return fail(where, "step score: road_margin must be finite and >= 0");
  if (!std::isfinite(r.dt) || !(r.dt > 0.f)) return fail(where, "step score: dt must be finite and > 0");
  RET_IF(road_table_check(where, "step score: ", r, k.shape));
  if (!types) return fail(where, "step score: needs the three-entry type switch");
  if (!k.out) return fail(where, "step score: needs the output [S][..][8]");
  if (reinterpret_cast<uintptr_t>(k.out) & 31) return fail(where, "step score: the output must be 32-byte aligned");
  if (r.records && !r.n_records) return fail(where, "step score: a record table needs its counts");
  if (misaligned16(r.records)) return fail(where, "step score: the record table must be 16-byte aligned");
  return 0;
}
// (out, steps: the log of a handle's configuration; a stand-alone entry's holds its output and no steps)
static int score_cfg(const char* where, float* out, int steps, unsigned char* row, const float* shape, const float* records,
                     const int* n_records, int rec_cap, int copies, int sweep, float margin, const int* types, float dt, ScoreCfg* cfg) {
  const int* ty = types_or_zeros(types);
  *cfg = ScoreCfg{out, steps, row, shape, {records, n_records, rec_cap, copies, sweep, margin, {ty[0], ty[1], ty[2]}, dt}};
  return score_check(where, *cfg, types);
}
// column c1 scored into the slots' 8 floats at out + s * out_stride (a context: step t's slice of the configuration's log)
static int launch_score(const char* where, const SceneHead& sc, int c1, const ScoreCfg& k, float* out, long long out_stride, void* stream) {
  if (sc.S <= 0 || sc.A_cap <= 0 || sc.T <= 0) return fail(where, "step score: S, A_cap and T must be positive");
  if (sc.A_cap > MAX_SCENE_AGENTS) return fail(where, "step score: A_cap exceeds INFGEN_Q_MAX_AGENTS");
  if (sc.S % k.rule.copies) return fail(where, "step score: S must be a multiple of copies");
  if (c1 < 0 || c1 >= sc.T) return fail(where, "step score: column outside [0, T)");
  if (out_stride < 8 || out_stride % 8) return fail(where, "step score: the output stride must be a positive multiple of 8 floats");
  if (!sc.pos || !sc.head || !sc.state || !sc.n_agents || !sc.type) return fail(where, "step score: null scene array");
  ScoreArgs a = rider_args<ScoreArgs>(sc, k);
  a.c1 = c1; a.out = out; a.out_stride = out_stride; a.out_row = k.row;
  hipLaunchKernelGGL(k_step_score, dim3((unsigned)a.S), dim3(SC_NT), 0, (hipStream_t)stream, a);
  return check_launch(where);
}

extern "C" int infgen_step_score(const float* pos, const float* head, const int* state, const int* n_agents, const int* type,
                                 const float* shape, int S, int A_cap, int T, int c1, const float* records, const int* n_records,
                                 int rec_cap, int copies, int sweep, float road_margin, const int* types, float dt, float* out_score,
                                 long long out_stride, unsigned char* out_row, void* stream) {
  const char* me = "infgen_step_score";
  ScoreCfg cfg;
  RET_IF(score_cfg(me, out_score, 0, out_row, shape, records, n_records, rec_cap, copies, sweep, road_margin, types, dt, &cfg));
  return launch_score(me, SceneHead{S, A_cap, T, pos, head, state, n_agents, type}, c1, cfg, out_score, out_stride, stream);
}

extern "C" int infgen_token_mask_score(int handle, float* step_score, int steps, unsigned char* score_row, const float* shape,
                                       const float* records, const int* n_records, int rec_cap, int copies, int sweep, float road_margin,
                                       const int* types, float dt) {
  const char* me = "infgen_token_mask_score";
  ScoreCfg cfg = SCORE_NONE;
  if (step_score) {
    RET_IF(score_cfg(me, step_score, steps, score_row, shape, records, n_records, rec_cap, copies, sweep, road_margin, types, dt, &cfg));
    if (steps < 1) return fail(me, "step score: steps must be positive");
  }
  return with_mask_slot(me, handle, NO_TOKEN_MASK, [&](TokenMaskSlot& s) { s.cfg.score = cfg; });
}

// ---------------------------------------------------------------------------------- observations
// the argument checks of include/infgen_hip.h ("observations") and the one launch of k_observe_rows
static int launch_observe(const char* where, const ObserveArgs& a, void* stream) {
  if (a.S <= 0 || a.A_cap <= 0 || a.T <= 0) return fail(where, "observe: S, A_cap and T must be positive");
  if (a.A_cap > MAX_SCENE_AGENTS) return fail(where, "observe: A_cap exceeds INFGEN_Q_MAX_AGENTS");
  if (a.c < 0 || a.c >= a.T) return fail(where, "observe: column outside [0, T)");
  if (a.K < 0 || a.K > OBS_MAX_K || a.Km < 0 || a.Km > OBS_MAX_K) return fail(where, "observe: K and Km must be in 0 .. INFGEN_OBS_MAX_K");
  if (!std::isfinite(a.dt) || !(a.dt > 0.f)) return fail(where, "observe: dt must be finite and > 0");
  if (!(a.radius >= 0.f) || !(a.map_radius >= 0.f)) return fail(where, "observe: a radius must be >= 0 (or +inf)");
  if (a.copies < 1) return fail(where, "observe: copies must be at least 1");
  if (a.S % a.copies) return fail(where, "observe: S must be a multiple of copies");
  if (!a.pos || !a.head || !a.state || !a.n_agents || !a.type || !a.shape) return fail(where, "observe: null scene array");
  const long long rows = (long long)a.S * a.A_cap;
  if (rows > 0x7fffffffLL) return fail(where, "observe: too many rows");
  if (a.N < 0 || (!a.obs_row && a.N != rows)) return fail(where, "observe: N must be S * A_cap without obs_row, and never negative");
  if (!a.self_feat) return fail(where, "observe: needs the output self_feat [N][8]");
  if (a.K > 0 && (!a.nbr_feat || !a.nbr_index || !a.nbr_count)) return fail(where, "observe: K > 0 needs nbr_feat, nbr_index and nbr_count");
  if (a.Km > 0 && (!a.map_feat || !a.map_index || !a.map_count)) return fail(where, "observe: Km > 0 needs map_feat, map_index and map_count");
  if (a.Km > 0 && (!a.map_pos || !a.map_orient || !a.map_type || !a.n_map)) return fail(where, "observe: Km > 0 needs the map arrays");
  if (a.map_pos && (!a.n_map || a.M_cap <= 0)) return fail(where, "observe: map_pos needs n_map and a positive M_cap");
  if (misaligned16(a.self_feat, a.nbr_feat, a.nbr_index, a.nbr_count) || misaligned16(a.map_feat, a.map_index, a.map_count))
    return fail(where, "observe: the outputs must be 16-byte aligned");
  if (a.N == 0) return 0;
  hipLaunchKernelGGL(k_observe_rows, dim3((unsigned)ceil_div(a.N, OB_WAVES)), dim3(64 * OB_WAVES), 0, (hipStream_t)stream, a);
  return check_launch(where);
}

extern "C" int infgen_observe_rows(const float* pos, const float* head, const int* state, const int* n_agents, const int* type,
                                   const float* shape, int S, int A_cap, int T, int c, float dt, const float* map_pos,
                                   const float* map_orient, const long long* map_type, const int* n_map, int M_cap, int copies,
                                   const int* obs_row, int N, int K, float radius, int Km, float map_radius, float* self_feat,
                                   float* nbr_feat, int* nbr_index, int* nbr_count, float* map_feat, int* map_index, int* map_count,
                                   void* stream) {
  const char* me = "infgen_observe_rows";
  ObserveArgs a = rider_args<ObserveArgs>(SceneHead{S, A_cap, T, pos, head, state, n_agents, type, shape});
  a.c = c; a.dt = dt;
  a.map_pos = map_pos; a.map_orient = map_orient; a.map_type = map_type; a.n_map = n_map; a.M_cap = M_cap; a.copies = copies;
  a.obs_row = obs_row; a.N = N; a.K = K; a.Km = Km; a.radius = radius; a.map_radius = map_radius;
  a.self_feat = self_feat; a.nbr_feat = nbr_feat; a.nbr_index = nbr_index; a.nbr_count = nbr_count;
  a.map_feat = map_feat; a.map_index = map_index; a.map_count = map_count;
  return launch_observe(me, a, stream);
}

// ---------------------------------------------------------------------------------- IDM commands
// the argument checks of include/infgen_hip.h ("IDM commands") and the one launch of k_idm_command
extern "C" int infgen_idm_command(const float* pos, const float* head, const int* state, const int* n_agents, const int* type,
                                  const float* shape, const uint8_t* ctl_row, int S, int A_cap, int T, int c, const float* records,
                                  const float* total, int P, int copies, const float* v_des, float dt, const float* v0_type,
                                  float headway, float s_min, float a_max, float b_comf, float b_max, float lateral, float keep,
                                  const int* types, int stop_at_end, float* cmd_pose, float* out_state, int* out_lead, void* stream) {
  const char* me = "infgen_idm_command";
  if (!v0_type || !types) return fail(me, "idm: needs the three desired speeds v0_type and the three-entry type switch");
  const float values[] = {dt, v0_type[0], v0_type[1], v0_type[2], headway, s_min, a_max, b_comf, b_max, lateral, keep};
  for (float x : values)
    if (!std::isfinite(x)) return fail(me, "idm: every parameter must be finite");
  if (!(dt > 0.f) || !(a_max > 0.f) || !(b_comf > 0.f) || !(b_max > 0.f)) return fail(me, "idm: dt, a_max, b_comf and b_max must be > 0");
  if (!(v0_type[0] > 0.f) || !(v0_type[1] > 0.f) || !(v0_type[2] > 0.f)) return fail(me, "idm: every v0_type must be > 0");
  if (headway < 0.f || s_min < 0.f || lateral < 0.f) return fail(me, "idm: headway, s_min and lateral must be >= 0");
  if (keep < 0.f || keep > 1.f) return fail(me, "idm: keep must be in [0, 1]");
  if (P < 2 || P > RT_MAX_POINTS) return fail(me, "idm: P must be in 2..32");
  if (copies < 1) return fail(me, "idm: copies must be at least 1");
  if (S <= 0 || A_cap <= 0 || T <= 0) return fail(me, "idm: S, A_cap and T must be positive");
  if (S % copies) return fail(me, "idm: S must be a multiple of copies");
  if (c < 1 || c >= T) return fail(me, "idm: column outside [1, T)");
  if (A_cap > MAX_SCENE_AGENTS) return fail(me, "idm: A_cap exceeds INFGEN_Q_MAX_AGENTS");
  if (!pos || !head || !state || !n_agents || !type || !shape || !ctl_row) return fail(me, "idm: null scene array");
  if (!records || !total) return fail(me, "idm: needs the record table and the routes' lengths");
  if (!cmd_pose) return fail(me, "idm: needs the pose buffer cmd_pose [S][A_cap][3]");
  if (misaligned16(records, out_state)) return fail(me, "idm: records and out_state must be 16-byte aligned");
  const long long rows = (long long)S * A_cap;
  if (rows > 0x7fffffffLL) return fail(me, "idm: too many rows");
  IdmArgs a = rider_args<IdmArgs>(SceneHead{S, A_cap, T, pos, head, state, n_agents, type, shape});
  a.c = c; a.ctl_row = ctl_row;
  a.records = records; a.total = total; a.P = P; a.copies = copies; a.v_des = v_des;
  a.dt = dt; a.headway = headway; a.s_min = s_min; a.a_max = a_max; a.b_comf = b_comf; a.b_max = b_max; a.lateral = lateral; a.keep = keep;
  for (int i = 0; i < 3; ++i) { a.v0_type[i] = v0_type[i]; a.types[i] = types[i]; }
  a.stop_at_end = stop_at_end;
  a.cmd_pose = cmd_pose; a.out_state = out_state; a.out_lead = out_lead;
  return launch_rows(me, k_idm_command, a, stream);
}

// ---------------------------------------------------------------------------------- rollout context
static SceneState scene_of(const InfgenRollout* r) {
  SceneState st;
  st.S = r->S; st.A_cap = r->A_cap; st.T = r->T; st.M_cap = r->M_cap; st.W = r->W; st.ring = r->ring;
  st.n_agents = r->n_agents; st.n_map = r->n_map; st.av_index = r->av_index;
  st.pos = r->pos; st.head = r->head; st.state = r->state; st.token = r->token; st.grid = r->grid;
  st.tmask = r->tmask; st.imask = r->imask; st.catflag = r->catflag; st.type = r->type; st.bos = r->bos;
  st.map_pos = r->map_pos; st.map_orient = r->map_orient; st.map_scene = r->map_scene;
  st.first_new = r->first_new; st.hv_ovr = r->hv_ovr;
  return st;
}
static EdgeBuf ebuf(const InfgenEdgeBuf& e) { return EdgeBuf{e.off, e.cnt, e.src, e.raw, e.total, e.cap}; }
static EdgeSet eset(const InfgenEdgeBuf& e) { return EdgeSet{e.off, e.cnt, e.src, e.rhat}; }

// ctl (optional): the context's sampling parameters as the kernels take them (the defaults for a greedy context, which ignores them)
// the riders of a registered handle as a context with these row types and token_size sees them
static int handle_riders(const char* where, int handle, const int* type, int token_size, StepRiders* riders) {
  TokenMaskDesc tm;
  RET_IF(with_mask_slot(where, handle, "token_mask is no handle of infgen_token_mask_create", [&](const TokenMaskSlot& s) {
    tm = s.d; riders->cfg = s.cfg;
  }));
  if (!tm.type) tm.type = type;
  TokenMaskCtl ctl;
  RET_IF(token_mask_ctl(where, &tm, token_size, &ctl));
  riders->mask = ctl;
  return 0;
}

// riders (optional): what rides on the context's decode step, from its token-mask handle (RIDERS_NONE without one)
static int validate(const InfgenRollout* r, const char* where, SamplingCtl* ctl = nullptr, StepRiders* riders = nullptr) {
  if (!r) return fail(where, "null context");
  if (r->A_cap > 1024 || r->A_cap <= 0) return fail(where, "A_cap must be in 1..1024");
  if (r->A_cap % 32) return fail(where, "A_cap must be a multiple of 32");
  if (r->num_layers <= 0 || r->num_layers > INFGEN_MAX_LAYERS) return fail(where, "bad num_layers");
  if (r->ring <= r->W) return fail(where, "ring must exceed the temporal window");
  if (r->W > 16) return fail(where, "temporal window larger than 16 columns is not supported");
  if ((r->no_grid_token | r->no_state_token) & ~1) return fail(where, "no_grid_token / no_state_token must be 0 or 1");
  SamplingCtl own;
  if (!ctl) ctl = &own;
  *ctl = SAMPLING_DEFAULT;
  if (r->sample_k > 1 && r->sample_u) {      // (a greedy context ignores the sampling parameters)
    const InfgenSampling sp{r->sample_temperature, r->sample_top_p, r->sample_temp_row};
    RET_IF(sampling_ctl(where, &sp, ctl));
  }
  StepRiders own_riders;
  if (!riders) riders = &own_riders;
  *riders = RIDERS_NONE;
  if (r->token_mask) {      // the context's token mask (registered without types: the context's own row types)
    RET_IF(handle_riders(where, r->token_mask, r->type, r->token_size, riders));
    const auto& [coll, road, score, route, signal] = riders->cfg;
    if (coll.bits) RET_IF(mask_fits(where, COLLISION_KIND, r, 1));
    if (road.bits) RET_IF(mask_fits(where, ROAD_KIND, r, road.rule.copies));
    if (score.out && r->first_new)
      return fail(where, "step score: contexts with scenario insertion cannot be scored: rows appended inside a step are left out");
    if (score.out && r->S % score.rule.copies) return fail(where, "step score: S must be a multiple of copies");
    if (route.bits) RET_IF(mask_fits(where, ROUTE_KIND, r, route.rule.copies));
    if (signal.bits) RET_IF(mask_fits(where, SIGNAL_KIND, r, signal.rule.copies));
  }
  if (r->token_logprob && !(r->store_logits && r->logits) && !r->logits_scratch) {
    // only the fused kernel needs no logits in memory: the plan under the context's own switches
    const int mode = (r->opts.use ? r->opts : O()).attn_mode;
    const int k = r->sample_k > 1 && r->sample_u ? r->sample_k : 1;
    if (emit_plan(mode, r->S * r->A_cap, r->token_size, k, true, false).need_logits)
      return fail(where, "token_logprob needs store_logits or logits_scratch [rows][token_size] (few rows, or sampling)");
  }
  return 0;
}

// test and diagnostic entry: the step riders a context of this token_size (row types `type`) would run under the handle
extern "C" int infgen_token_mask_riders(int handle, const int* type, int token_size, void* out, int capacity) {
  const char* me = "infgen_token_mask_riders";
  if (!out || capacity < (int)RIDERS_EXPORT_BYTES) return fail(me, "needs a buffer of at least the block's size in bytes");
  StepRiders riders;
  std::memset(&riders, 0, sizeof riders);               // (padding bytes too: the caller compares bytes)
  riders.mask = TOKEN_MASK_NONE; riders.cfg = CFGS_NONE;
  if (handle != 0) RET_IF(handle_riders(me, handle, type, token_size, &riders));
  std::memcpy(out, &riders, RIDERS_EXPORT_BYTES);          // (the signal configuration behind it: infgen_token_mask_signal_get)
  return (int)RIDERS_EXPORT_BYTES;
}

extern "C" int infgen_token_mask_signal_get(int handle, void* out, int capacity) {
  const char* me = "infgen_token_mask_signal_get";
  static_assert(sizeof(SignalCfg) == 6 * sizeof(void*) + 8 * sizeof(int) + 2 * sizeof(void*), "SignalCfg has no padding: its bytes are compared");
  if (!out || capacity < (int)sizeof(SignalCfg)) return fail(me, "needs a buffer of at least the configuration's size in bytes");
  SignalCfg cfg = SIGNAL_NONE;
  if (handle != 0) RET_IF(with_mask_slot(me, handle, NO_TOKEN_MASK, [&](const TokenMaskSlot& s) { cfg = s.cfg.signal; }));
  std::memcpy(out, &cfg, sizeof cfg);
  return (int)sizeof cfg;
}

// zero_totals = false: the three totals were cleared by the previous step's k_integrate (IntegrateArgs.edge_totals)
static int build_edges_impl(const InfgenRollout* r, int c, int edgeless, void* stream, bool zero_totals, unsigned long long* clear_keys = nullptr,
                            bool clear_sync = false) {
  RET_IF(validate(r, "infgen_build_edges"));
  OptScope _opts(r);
  hipStream_t s = (hipStream_t)stream;
  if (!edgeless && zero_totals) {
    if (r->em.total == r->et.total + 1 && r->ea.total == r->et.total + 2) {      // laid out back to back: one fill
      if (hipMemsetAsync(r->et.total, 0, 3 * sizeof(int), s) != hipSuccess) return fail("infgen_build_edges", "memset failed");
    } else if (hipMemsetAsync(r->et.total, 0, sizeof(int), s) != hipSuccess ||
               hipMemsetAsync(r->em.total, 0, sizeof(int), s) != hipSuccess ||
               hipMemsetAsync(r->ea.total, 0, sizeof(int), s) != hipSuccess)
      return fail("infgen_build_edges", "memset failed");
  }
  BuildEdgesArgs a;
  a.st = scene_of(r); a.c = c; a.edgeless = edgeless; a.r_map = r->r_map; a.r_agent = r->r_agent;
  a.rows = stride_rows(r); a.t = ebuf(r->et); a.m = ebuf(r->em); a.a = ebuf(r->ea);
  a.clear_keys = clear_keys;
  a.clear_sync = clear_sync ? reinterpret_cast<int*>(r->SIG) : nullptr;      // (k_layers_p's per-scene counters: layers_p_launch)
  a.prof = (g_prof.mask & ((1u << INFGEN_KID_EDGE_ATTN) | (1u << INFGEN_KID_BUILD_EDGES))) ? g_prof.rows_dev : nullptr;
  { ProfScope _ps(INFGEN_KID_BUILD_EDGES, stream);
    a.map_lds = r->M_cap < 4096 ? r->M_cap : 4096;
    const size_t lds = (size_t)a.map_lds * 8;
    // few scenes: 16 waves per workgroup whatever A_cap (INFGEN_BE_WIDE_SCENES: the largest batch that takes them, default 128)
    if (r->A_cap <= 256 && r->S > knob::be_wide_scenes) hipLaunchKernelGGL(k_build_edges<256>, dim3(r->S, 3), dim3(256), lds, s, a);
    else hipLaunchKernelGGL(k_build_edges<1024>, dim3(r->S, 3), dim3(1024), lds, s, a); }
  return check_launch("infgen_build_edges");
}
extern "C" int infgen_build_edges(const InfgenRollout* r, int c, int edgeless, void* stream) {
  return build_edges_impl(r, c, edgeless, stream, true);
}

// all rows of column col; infgen_raw_feature_rows fills in its row list
static RawFeatArgs rawfeat_args(const InfgenRollout* r, int col) {
  RawFeatArgs a;
  a.st = scene_of(r); a.col = col; a.tok_tab = r->tok_tab; a.token_size = r->token_size;
  a.grid_tab = r->grid_tab; a.grid_size = r->grid_size; a.state_emb = r->state_emb;
  a.cat_agent = r->cat_agent; a.cat_seed = r->cat_seed; a.raw2 = r->raw2; a.cat = r->cat; a.fus_in = r->fus_in;
  a.row_list = nullptr; a.row_mask = nullptr; a.n_list = 0; a.no_grid = r->no_grid_token;
  return a;
}

// workgroups per scene of k_integrate: 16 rows each for few scenes (INFGEN_INT_GROUP_SCENES: the largest batch, default 128), else 1.
// With more than one the arg-max keys are reset by the k_build_edges that follows (build_edges_impl: clear_keys), not by k_integrate.
static int integrate_groups(const InfgenRollout* r) {
  return (r->S <= knob::int_group_scenes && r->A_cap % 16 == 0 && r->A_cap > 16) ? r->A_cap / 16 : 1;
}
static int integrate_impl(const InfgenRollout* r, int t, void* stream, unsigned long long* heads_part, bool zero_totals, bool prep, bool zero_sync = false) {
  RET_IF(validate(r, "infgen_integrate"));
  OptScope _opts(r);
  IntegrateArgs a;
  a.heads_part = heads_part; a.next_token_w = r->next_token;
  a.edge_totals = zero_totals ? r->et.total : nullptr;
  a.zero_sync = zero_sync ? reinterpret_cast<int*>(r->SIG) : nullptr;       // (k_layers_p's per-scene counters: layers_p_launch)
  a.do_prep = prep ? 1 : 0;
  if (prep) a.prep = rawfeat_args(r, 2 + t);
  a.st = scene_of(r); a.c = 1 + t; a.t = t; a.R = r->R; a.force_valid = r->force_valid; a.no_state = r->no_state_token;
  a.next_token = r->next_token; a.next_state = r->next_state;
  a.teacher_token = r->teacher_token; a.teacher_state = r->teacher_state; a.teacher_grid = r->teacher_grid;
  a.teacher_pos = r->teacher_pos; a.teacher_head = r->teacher_head; a.replay_row = r->replay_row;
  a.vocab = r->vocab; a.token_size = r->token_size; a.grid_xy = r->grid_xy; a.grid_size = r->grid_size;
  a.pred_traj = r->pred_traj; a.pred_head = r->pred_head; a.pred_state = r->pred_state;
  a.groups = integrate_groups(r);
  { ProfScope _ps(INFGEN_KID_INTEGRATE, stream);
    // 16 waves per workgroup whatever A_cap: the grid-cell search is one wave per agent (4 instead of 16 agents per wave with 256
    // threads: 0.95 -> 0.56 ms per rollout at 8 scenes, 1.23 -> 0.98 at 512); few scenes: 16 rows per workgroup, one wave each
    hipLaunchKernelGGL(k_integrate<1024>, dim3(r->S, a.groups), dim3(1024), 0, (hipStream_t)stream, a); }
  return check_launch("infgen_integrate");
}
extern "C" int infgen_integrate(const InfgenRollout* r, int t, void* stream) {
  return integrate_impl(r, t, stream, nullptr, false, false);
}

// ---- closed-loop sessions: the commands of decode step t -> column 2 + t of the context's plan arrays, in front of the step
static void launch_command_rows(const CommandRowsArgs& a, void* stream) {
  hipLaunchKernelGGL(k_command_rows, dim3(a.A_cap, a.S), dim3(256), 0, (hipStream_t)stream, a);
}
extern "C" int infgen_command_rows(const InfgenRollout* r, int t, int kind, const int* cmd_token, const float* cmd_pose,
                                   const unsigned char* cmd_mask, const float* shape, float* cmd_cost, void* stream) {
  const char* me = "infgen_command_rows";
  if (!r) return fail(me, "null context");
  if (r->S <= 0 || r->S > 65535 || r->A_cap <= 0 || r->A_cap > 1024) return fail(me, "S must be in 1..65535 and A_cap in 1..1024");
  if (!(r->teacher_token && r->teacher_state && r->replay_row))
    return fail(me, "the context has no plan to write: teacher_token, teacher_state and replay_row are needed (a replay context)");
  if ((r->teacher_pos != nullptr) != (r->teacher_head != nullptr)) return fail(me, "teacher_pos and teacher_head come together");
  if (!(r->n_agents && r->state && r->pos && r->head && r->type && r->vocab)) return fail(me, "null scene array");
  if (r->token_size <= 0) return fail(me, "token_size must be positive");
  const int c = 1 + t;
  if (t < 0 || c + 1 > r->T - 1) return fail(me, "step beyond the column range");
  if (kind != 0 && kind != 1) return fail(me, "kind must be 0 (token ids) or 1 (target poses)");
  if (kind == 0 && !cmd_token) return fail(me, "a token command needs cmd_token [S][A_cap]");
  if (kind == 1 && !(cmd_pose && shape)) return fail(me, "a pose command needs cmd_pose [S][A_cap][3] and the shape array [S][A_cap][3]");
  CommandRowsArgs a;
  a.S = r->S; a.A_cap = r->A_cap; a.T = r->T; a.c = c; a.kind = kind; a.token_size = r->token_size;
  a.n_agents = r->n_agents; a.replay_row = r->replay_row; a.state = r->state; a.pos = r->pos; a.head = r->head; a.type = r->type;
  a.vocab = r->vocab; a.shape = shape; a.cmd_token = cmd_token; a.cmd_pose = cmd_pose; a.cmd_mask = cmd_mask;
  a.teacher_token = const_cast<int*>(r->teacher_token); a.teacher_state = const_cast<int*>(r->teacher_state);
  a.teacher_pos = const_cast<float*>(r->teacher_pos); a.teacher_head = const_cast<float*>(r->teacher_head);
  a.cmd_cost = cmd_cost;
  launch_command_rows(a, stream);
  return check_launch(me);
}

// ---- branching rollouts: slot s becomes a clone of slot parent[s] as of the boundary in front of decode step t (k_branch_scenes)
// the segment table: everything a decode step reads that an earlier step (or the prologue) wrote per scene.  What configures a slot
// (uniforms, temperatures, masks, plans, replay flags) and what every step rebuilds before reading it (edge sets, scratch) is not in it.
static int branch_segments(const InfgenRollout* r, int t, BranchSeg* seg, int* n_seg, float* score_log, long long score_bytes) {
  const long long A = r->A_cap, rows = (long long)r->S * A;
  int n = 0, chunk = 0;
  auto add = [&](void* base, long long bytes, int outer, long long outer_stride) {
    if (!base || bytes <= 0 || outer <= 0) return;
    BranchSeg& g = seg[n++];
    g.base = static_cast<char*>(base); g.bytes = bytes; g.outer = outer; g.outer_stride = outer_stride;
    g.per_block = (int)((bytes + BR_CHUNK - 1) / BR_CHUNK);
    g.chunk0 = chunk;
    g.wide = ((reinterpret_cast<uintptr_t>(base) | (uintptr_t)bytes | (uintptr_t)outer_stride) & 15) == 0 ? 1 : 0;
    chunk += g.per_block * outer;
  };
  const long long TA = (long long)r->T * A;
  add(r->pos, TA * 8, 1, 0); add(r->head, TA * 4, 1, 0); add(r->state, TA * 4, 1, 0); add(r->token, TA * 4, 1, 0);
  add(r->grid, TA * 4, 1, 0); add(r->tmask, TA, 1, 0); add(r->imask, TA, 1, 0); add(r->catflag, TA, 1, 0);
  add(r->bos, A * 4, 1, 0);
  for (int l = 0; l < r->num_layers; ++l) {
    add(r->ringK[l], A * D * 4, r->ring, rows * D * 4);
    add(r->ringV[l], A * D * 4, r->ring, rows * D * 4);
  }
  add(r->X, A * D * 4, 1, 0);
  add(r->pred_traj, A * r->R * 8, 1, 0); add(r->pred_head, A * r->R * 4, 1, 0); add(r->pred_state, A * r->R * 4, 1, 0);
  // the step-major logs: the slices of the steps that ran, [0, t)
  add(r->token_logprob, A * 4, t, rows * 4);
  add(r->sample_logprob, A * 4, t, rows * 4);
  add(r->store_logits ? r->logits : nullptr, A * r->token_size * 4, t, rows * r->token_size * 4);
  add(score_log, score_bytes, 1, 0);                                  // the scene's whole [steps][8] block
  *n_seg = n;
  return chunk;
}

extern "C" int infgen_branch_scenes(const InfgenRollout* r, int t, const int* parent, int* n_bad, void* stream) {
  const char* me = "infgen_branch_scenes";
  StepRiders riders;
  RET_IF(validate(r, me, nullptr, &riders));
  if (r->S <= 0 || r->S > 65535) return fail(me, "S must be in 1..65535");
  if (r->T <= 0 || r->R <= 0 || r->ring <= 0 || r->token_size <= 0) return fail(me, "bad sizes");
  if (!parent) return fail(me, "null parent");
  if (r->first_new) return fail(me, "contexts with scenario insertion cannot branch: row counts, types and shapes differ between the copies");
  if (t < 0 || 1 + t > r->T - 1) return fail(me, "t must be in 0..steps (the boundary in front of decode step t)");
  if (!(r->pos && r->head && r->state && r->token && r->grid && r->tmask && r->imask && r->catflag && r->bos && r->X))
    return fail(me, "null scene array");
  static_assert(BR_MAX_SEGS >= 9 + 2 * INFGEN_MAX_LAYERS + 1 + 3 + 4, "segment table too short");
  BranchArgs a{};
  a.S = r->S; a.parent = parent; a.map_scene = r->map_scene; a.n_bad = n_bad;
  const int chunks = branch_segments(r, t, a.seg, &a.n_seg, riders.cfg.score.out, (long long)riders.cfg.score.steps * 8 * 4);
  if (n_bad && hipMemsetAsync(n_bad, 0, sizeof(int), (hipStream_t)stream) != hipSuccess) return fail(me, "memset failed");
  hipLaunchKernelGGL(k_branch_scenes, dim3(chunks, r->S), dim3(BR_NT), 0, (hipStream_t)stream, a);
  return check_launch(me);
}

// ---- snapshots: the segments of branch_segments between the context and a caller's buffer of entries (k_snapshot_scenes)
// the checks both directions and infgen_snapshot_bytes share; fills the segment table and every segment's offset in an entry
static int snapshot_layout(const InfgenRollout* r, int t, const char* me, SnapArgs* a, int* chunks, long long* entry_bytes) {
  StepRiders riders;
  RET_IF(validate(r, me, nullptr, &riders));
  if (r->S <= 0 || r->S > 65535) return fail(me, "S must be in 1..65535");
  if (r->T <= 0 || r->R <= 0 || r->ring <= 0 || r->token_size <= 0) return fail(me, "bad sizes");
  if (r->first_new) return fail(me, "contexts with scenario insertion cannot be saved or restored: row counts, types and shapes differ between the copies");
  if (t < 0 || 1 + t > r->T - 1) return fail(me, "t must be in 0..steps (the boundary in front of decode step t)");
  if (!(r->pos && r->head && r->state && r->token && r->grid && r->tmask && r->imask && r->catflag && r->bos && r->X))
    return fail(me, "null scene array");
  *chunks = branch_segments(r, t, a->seg, &a->n_seg, riders.cfg.score.out, (long long)riders.cfg.score.steps * 8 * 4);
  long long off = 0;
  for (int k = 0; k < a->n_seg; ++k) {
    a->entry_off[k] = off;
    off += ((a->seg[k].bytes + 15) & ~15LL) * a->seg[k].outer;
  }
  *entry_bytes = off;
  a->S = r->S; a->t = t; a->map_scene = r->map_scene;
  return 0;
}
static int snapshot_buffer(const char* me, const void* snap, long long entry_stride, long long entry_bytes, int n) {
  if (n < 0 || n > 65535) return fail(me, "n must be in 0..65535");
  if (!snap) return fail(me, "null snapshot buffer");
  if (reinterpret_cast<uintptr_t>(snap) & 15) return fail(me, "snap must be 16-byte aligned");
  if (entry_stride & 15) return fail(me, "entry_stride must be a multiple of 16");
  if (entry_stride < entry_bytes) return fail(me, "entry_stride is smaller than infgen_snapshot_bytes(r, t)");
  return 0;
}

extern "C" int infgen_snapshot_bytes(const InfgenRollout* r, int t, long long* bytes) {
  SnapArgs a{};
  int chunks;
  if (!bytes) return fail("infgen_snapshot_bytes", "null bytes");
  return snapshot_layout(r, t, "infgen_snapshot_bytes", &a, &chunks, bytes);
}

extern "C" int infgen_snapshot_scenes(const InfgenRollout* r, int t, const int* slots, int n, void* snap, long long entry_stride,
                                      int* head, int* n_bad, void* stream) {
  const char* me = "infgen_snapshot_scenes";
  SnapArgs a{};
  int chunks;
  long long bytes;
  RET_IF(snapshot_layout(r, t, me, &a, &chunks, &bytes));
  if (!slots || !head) return fail(me, "null slots or head");
  RET_IF(snapshot_buffer(me, snap, entry_stride, bytes, n));
  a.n = n; a.sel = slots; a.head = head; a.snap = static_cast<char*>(snap); a.stride = entry_stride; a.n_bad = n_bad;
  if (n_bad && hipMemsetAsync(n_bad, 0, sizeof(int), (hipStream_t)stream) != hipSuccess) return fail(me, "memset failed");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_snapshot_scenes<false>, dim3(chunks, n), dim3(BR_NT), 0, (hipStream_t)stream, a);
  return check_launch(me);
}

extern "C" int infgen_restore_scenes(const InfgenRollout* r, int t, const int* index, const void* snap, long long entry_stride,
                                     const int* head, int n, int* n_bad, void* stream) {
  const char* me = "infgen_restore_scenes";
  SnapArgs a{};
  int chunks;
  long long bytes;
  RET_IF(snapshot_layout(r, t, me, &a, &chunks, &bytes));
  if (!index || !head) return fail(me, "null index or head");
  RET_IF(snapshot_buffer(me, snap, entry_stride, bytes, n));
  a.n = n; a.sel = index; a.head = const_cast<int*>(head); a.snap = static_cast<char*>(const_cast<void*>(snap));
  a.stride = entry_stride; a.n_bad = n_bad;
  if (n_bad && hipMemsetAsync(n_bad, 0, sizeof(int), (hipStream_t)stream) != hipSuccess) return fail(me, "memset failed");
  hipLaunchKernelGGL(k_snapshot_scenes<true>, dim3(chunks, r->S), dim3(BR_NT), 0, (hipStream_t)stream, a);
  return check_launch(me);
}

extern "C" int infgen_resample_parents(const int* ancestor, int S0, int copies, int* parent, void* stream) {
  const char* me = "infgen_resample_parents";
  if (!ancestor || !parent) return fail(me, "null array");
  if (S0 <= 0 || copies <= 0) return fail(me, "S0 and copies must be positive");
  if (copies > RS_NT * RS_ITEMS) return fail(me, "copies must be <= 1024");
  hipLaunchKernelGGL(k_resample_parents, dim3(S0), dim3(RS_NT), 0, (hipStream_t)stream, ResampleArgs{ancestor, copies, parent});
  return check_launch(me);
}

// MLPEmbedding pack (first Linear K0 -> 128): P(K0p,128) b ln_g ln_b | P(128,128) b ln_g ln_b | P(128,128) b
static inline int mlpemb_off2(int K0p) { return K0p * 128 + 3 * 128; }
static inline int mlpemb_off3(int K0p) { return mlpemb_off2(K0p) + 16384 + 3 * 128; }
// the three stages as k_linear launches through tmp1 / tmp2 [rows][128]; K inputs padded to K0p in the pack.  Y may be tmp1 (the
// last stage reads tmp2 only)
static int mlp_embedding_fp32(const float* X, int ldx, int rows, int K, int K0p, const float* P, float* tmp1, float* tmp2, float* Y,
                              int ldy, void* stream) {
  const int o2 = mlpemb_off2(K0p), o3 = mlpemb_off3(K0p);
  RET_IF(infgen_linear(X, ldx, nullptr, rows, K, P, 128, P + K0p * 128, 128, nullptr, nullptr,
                       P + K0p * 128 + 128, P + K0p * 128 + 256, 1, tmp1, 128, stream));
  RET_IF(infgen_linear(tmp1, 128, nullptr, rows, 128, P + o2, 128, P + o2 + 16384, 128, nullptr, nullptr,
                       P + o2 + 16384 + 128, P + o2 + 16384 + 256, 1, tmp2, 128, stream));
  return infgen_linear(tmp2, 128, nullptr, rows, 128, P + o3, 128, P + o3 + 16384, 128, nullptr, nullptr,
                       nullptr, nullptr, 0, Y, ldy, stream);
}

// MLPEmbedding (reference infgen/modules/layers.py:163-192) with K0 = 128 j inputs: Linear LN ReLU Linear LN ReLU Linear.  Split
// arithmetic (attn_mode != 0): the three stages in one launch of k_mlpemb_h (any row count: one 25 us chain instead of three dependent
// fp32 launches of 30-40 us each); attn_mode 0: mlp_embedding_fp32
static int mlp_embedding_impl(const float* X, int ldx, int rows, int K0, const float* P, float* tmp1, float* tmp2, float* Y, int ldy,
                              void* stream, const char* where) {
  if (rows <= 0) return 0;
  if (O().attn_mode != 0) {
    launch_mlpemb_h(MlpEmbHArgs{X, ldx, rows, K0, P, Y, ldy}, stream);
    return check_launch(where);
  }
  if (!tmp1 || !tmp2) return fail(where, "the fp32 kernels need the two scratch arrays");
  return mlp_embedding_fp32(X, ldx, rows, K0, K0, P, tmp1, tmp2, Y, ldy, stream);
}
extern "C" int infgen_mlp_embedding(const float* X, int ldx, int rows, int K0, const float* pack, float* tmp1, float* tmp2,
                                    float* Y, int ldy, void* stream) {
  if (K0 <= 0 || K0 % 128 || K0 > 512) return fail("infgen_mlp_embedding", "K0 must be 128, 256, 384 or 512");
  return mlp_embedding_impl(X, ldx, rows, K0, pack, tmp1, tmp2, Y, ldy, stream, "infgen_mlp_embedding");
}

// inputs of fusion_emb: [token | x_a | state | grid] (K0 = 512), without the grid embedding for use_grid_token = False (K0 = 384)
static inline int fusion_k0(const InfgenRollout* r) { return r->no_grid_token ? 384 : 512; }

// fusion_emb of the gathered rows (fus_in [rows][512]) -> X
static int raw_feature_fusion(const InfgenRollout* r, void* stream) {
  return mlp_embedding_impl(r->fus_in, 512, r->S * r->A_cap, fusion_k0(r), r->fusion_pack, r->tmp1, r->tmp2, r->X, 128, stream,
                            "infgen_raw_feature/fusion");
}

extern "C" int infgen_raw_feature(const InfgenRollout* r, int col, void* stream) {
  RET_IF(validate(r, "infgen_raw_feature"));
  OptScope _opts(r);
  const int rows = r->S * r->A_cap;
  RawFeatArgs a = rawfeat_args(r, col);
  { ProfScope _ps(INFGEN_KID_RAWFEAT, stream);
    hipLaunchKernelGGL(k_rawfeat_prep, dim3(ceil_div(rows * 32, NT)), dim3(NT), 0, (hipStream_t)stream, a); }
  RET_IF(check_launch("infgen_raw_feature/prep"));
  RET_IF(infgen_fourier_embed(r->raw2, 2, nullptr, rows, r->four_xa, r->cat, 128, r->fus_in + 128, 512, 0, stream));
  return raw_feature_fusion(r, stream);
}

// the same for a few rows only (insertion: the rows appended in this sub-loop iteration): row_list[k] = row, used where
// row_mask[k] != 0.  The first n rows of the scratch arrays raw2 / cat / fus_in / tmp1 / tmp2 hold the compact intermediate
// results (every all-rows call rewrites them); X is updated at the listed rows only.
extern "C" int infgen_raw_feature_rows(const InfgenRollout* r, int col, const int* row_list, const int* row_mask, int n,
                                       void* stream) {
  RET_IF(validate(r, "infgen_raw_feature_rows"));
  OptScope _opts(r);
  if (n <= 0) return 0;
  if (n > r->S * r->A_cap) return fail("infgen_raw_feature_rows", "more rows than the layout holds");
  RawFeatArgs a = rawfeat_args(r, col);
  a.row_list = row_list; a.row_mask = row_mask; a.n_list = n;
  { ProfScope _ps(INFGEN_KID_RAWFEAT, stream);
    hipLaunchKernelGGL(k_rawfeat_prep, dim3(ceil_div(n * 32, NT)), dim3(NT), 0, (hipStream_t)stream, a); }
  RET_IF(check_launch("infgen_raw_feature_rows/prep"));
  RET_IF(infgen_fourier_embed(r->raw2, 2, nullptr, n, r->four_xa, r->cat, 128, r->fus_in + 128, 512, 0, stream));
  // fusion_emb of the compact rows into tmp1 (on the fp32 path tmp1 is also the first stage's output: mlp_embedding_impl)
  RET_IF(mlp_embedding_impl(r->fus_in, 512, n, fusion_k0(r), r->fusion_pack, r->tmp1, r->tmp2, r->tmp1, 128, stream,
                            "infgen_raw_feature_rows/fusion"));
  hipLaunchKernelGGL(k_scatter_rows, dim3(ceil_div(n * 32, NT)), dim3(NT), 0, (hipStream_t)stream, r->tmp1, row_list, row_mask, n, r->X);
  return check_launch("infgen_raw_feature_rows/scatter");
}

// Optional: the Fourier embeddings of the map and agent edge sets (matrix-pipe / VALU work) run on a side stream while
// the temporal and map sublayers of the first layer (memory-bound) run on the caller's stream.
static hipStream_t g_side = nullptr;
static hipEvent_t g_ev_fork = nullptr, g_ev_m = nullptr, g_ev_a = nullptr;
extern "C" int infgen_set_overlap(int mode) {
  if (mode != 0 && mode != 1) return fail("infgen_set_overlap", "mode must be 0 or 1");
  if (mode && !g_side) {
    if (hipStreamCreateWithFlags(&g_side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&g_ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g_ev_m, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g_ev_a, hipEventDisableTiming) != hipSuccess)
      return fail("infgen_set_overlap", "stream / event creation failed");
  }
  g_def.overlap = mode;
  return 0;
}

// ---- k_layers_p (layers_p.hip): every sublayer of a step in one launch, one resident workgroup per 16-row group
extern "C" int infgen_set_layers_p(int mode) {        // (process-wide default, like the other infgen_set_*: contexts carry their own copy)
  if (mode < 0 || mode > 2) return fail("infgen_set_layers_p", "mode must be 0, 1 or 2");
  g_def.layers_p = mode;
  return 0;
}
// scenes per launch when the batch needs more than one (0: not eligible): whole scenes, at most `limit` 16-row groups per launch,
// at most INFGEN_LP_MAX_CHUNKS (2) launches - measured with scenes of 64 agents: 96 / 128 scenes 36.6 / 39.6 ms per rollout through the
// per-sublayer launches, whose layers cost 26 - 28 ms there against 2 x 10 ms of two 64-scene launches; from three chunks on the
// big-batch kernels are as fast
static int lp_chunk_scenes(const InfgenRollout* r, int limit) {
  const int gps = r->A_cap / 16;
  if (gps <= 0 || gps > limit) return 0;
  const int per = limit / gps;                       // scenes per launch
  const int chunks = (r->S + per - 1) / per;
  return chunks <= knob::lp_max_chunks ? per : 0;
}
// the launch shape qualifies (the kernel keeps U / Z on chip like k_edge_fused: step_mode treats it as a fused launch)
// k_layers_p's workgroups meet at counters in global memory, so a launch needs ALL of them resident at some point:
//  * the grid is checked against the device's resident capacity for this kernel (hipOccupancyMaxActiveBlocksPerMultiprocessor x CUs:
//    layers_p_shape) - what fits becomes resident as soon as kernels of other streams leave the CUs, so the wait at the counters
//    has no limit (no trap);
//  * launches of different streams of this process are ordered behind each other (two half-resident launches would wait for each
//    other for ever): g_lp_mu / g_lp_order below (an event recorded behind every launch on its own stream);
//  * layers_p == 2 additionally launches through hipLaunchCooperativeKernel (the runtime's own residency contract, and the
//    cooperative queue is device-wide - this also covers another PROCESS running such a kernel on the same GPU); measured cost of
//    the queue hand-over: 8 scenes 9.54 -> 9.97 ms per rollout, 64 scenes 17.01 -> 17.36 (tools/lp_coop_ab.sh).  A refused
//    cooperative launch falls back to the per-sublayer kernels for good (g_lp_refused).
static std::atomic<bool> g_lp_refused{false};
static std::mutex g_lp_mu;                  // orders the k_layers_p launches of the process's streams (per device: LpOrder)
constexpr int LP_MAX_DEVICES = 16;
struct LpOrder { hipEvent_t ev = nullptr; bool any = false; };     // ev: recorded behind the device's last k_layers_p launch, on the
static LpOrder g_lp_order[LP_MAX_DEVICES];                         // stream that launched it (no stream handle is kept)
struct LpDevice { bool init = false; int n_cu = 1; int coop = 0; int wg_per_cu = 0; };
static int lp_current_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
  return dev < 0 || dev >= LP_MAX_DEVICES ? 0 : dev;
}
static const LpDevice& lp_device() {
  static LpDevice devs[LP_MAX_DEVICES];
  static std::mutex mu;
  const int dev = lp_current_device();
  std::lock_guard<std::mutex> lk(mu);
  LpDevice& v = devs[dev];
  if (!v.init) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) {
      v.n_cu = prop.multiProcessorCount;
      (void)hipDeviceGetAttribute(&v.coop, hipDeviceAttributeCooperativeLaunch, dev);
      // resident workgroups per CU of the largest variant (the 120 KB of LDS set it: 1)
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v.wg_per_cu, k_layers_p<true, 16>, 512, 0) != hipSuccess) v.wg_per_cu = 0;
    }
    (void)hipGetLastError();
    v.init = true;
  }
  return v;
}
extern "C" int infgen_layers_p_capacity(void) {       // workgroups one k_layers_p launch may have on the current device (0: not available)
  const LpDevice& d = lp_device();
  if (d.wg_per_cu <= 0) return 0;
  return d.n_cu * (d.wg_per_cu > 1 ? 1 : d.wg_per_cu);      // (the launch shapes assume one workgroup per CU)
}
// workgroups a launch may have: the device's resident capacity (a partition with fewer CUs than 256 - DPX / QPX / CPX modes, smaller
// parts - lowers it), and INFGEN_LP_MAX_GROUPS
static int lp_limit() {
  const int cap = infgen_layers_p_capacity(), mx = knob::lp_max_groups;
  return cap < mx ? cap : mx;
}
static bool is_capturing(void* stream) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing((hipStream_t)stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}
// k_layers_p bounds a row's LayerNorm output with header slots 10..13 of the attention packs; a pack without them (an older or
// foreign packer: slot 14 != AH_HDR_VERSION) would scale its operands by 2^126.  Checked once per pack pointer (a 64-byte
// device -> host copy at a context's first launch); contexts with such a pack take the per-sublayer launches.
static bool lp_packs_ok(const InfgenRollout* r, bool refresh = false, void* stream = nullptr) {
  static std::mutex mu;
  static std::unordered_map<const float*, bool> seen;      // verdict per pack address, overwritten in place on refresh
  std::lock_guard<std::mutex> lk(mu);
  // a pack that was never examined needs a synchronous 64-byte copy: not while `stream` is being captured into a graph (the copy
  // would fail and the verdict would stick) - such a launch takes the per-sublayer kernels, the verdict stays open
  const bool capturing = stream && is_capturing(stream);
  auto ok = [&](const float* pack) {
    if (!pack) return false;
    if (!refresh) { auto it = seen.find(pack); if (it != seen.end()) return it->second; }
    if (capturing) return false;
    float hdr[16] = {};
    const bool good = hipMemcpy(hdr, pack + AH_HDR, sizeof(hdr), hipMemcpyDeviceToHost) == hipSuccess && hdr[14] == AH_HDR_VERSION &&
                      hdr[10] > 0.f && hdr[12] > 0.f;
    seen[pack] = good;
    return good;
  };
  for (int i = 0; i < r->num_layers; ++i)
    if (!ok(r->attn_t[i]) || !ok(r->attn_m[i]) || !ok(r->attn_a[i])) return false;
  return true;
}
static bool split_copy_boundary(const InfgenRollout* r, bool refresh);      // (the split mode of infgen_rollout_run, below)
// A context's packs looked at afresh (a device address may have held another pack before): callers that build a context call
// this once (infgen_amd/engine.py: _build_ctx); without it a pack is examined when its address is first seen.  Synchronous.
extern "C" int infgen_rollout_validate(const InfgenRollout* r) {
  RET_IF(validate(r, "infgen_rollout_validate"));
  if (r->replay_row && !(r->teacher_token && r->teacher_state))
    return fail("infgen_rollout_validate", "replay_row needs teacher_token and teacher_state (the plan the flagged rows follow)");
  if ((r->teacher_pos != nullptr) != (r->teacher_head != nullptr))
    return fail("infgen_rollout_validate", "teacher_pos and teacher_head come together");
  (void)lp_packs_ok(r, true);
  (void)split_copy_boundary(r, true);
  return 0;
}
static bool layers_p_shape(const InfgenRollout* r, int rows, int edgeless, void* stream) {
  const LpDevice& lpd = lp_device();
  if (lpd.wg_per_cu <= 0 || (O().layers_p == 2 && (!lpd.coop || g_lp_refused.load()))) return false;
  // all workgroups must be resident at once (they meet at per-scene counters): at most one workgroup per CU (120 KB of LDS each).
  // Up to that limit the one-launch kernel wins at every size measured (scenes of 64 agents, ms per rollout, k_layers_p vs the
  // per-sublayer launches): 8 scenes 10.7 / 15.4, 16: 11.7 / 16.4, 32: 13.7 / 18.0 (8 rows per workgroup), 48: 16.8 / 20.1,
  // 64: 18.4 / 22.2 (16 rows, 256 workgroups).  (With every wave executing the scene counter's agent-scope fences the crossover
  // sat at ~40 scenes: 2,048 L2 write-backs per layer.)  INFGEN_LP_MAX_GROUPS lowers the limit.
  // (a row-group list of an insertion context is ignored: the launch visits every group - the ones without agents have empty edge
  // lists and run in parallel on CUs that would idle)
  return O().layers_p && O().edge_fuse != 0 && O().attn_mode != 0 && three_terms() && O().fourier_mode != 0 &&
         !(O().overlap && g_side) && r->A_cap % 16 == 0 && lp_chunk_scenes(r, lp_limit()) > 0 &&
          r->num_layers <= LP_MAX_LAYERS && r->U && r->SIG && !r->tap_x && lp_packs_ok(r, false, stream);
}

// ---- a decode step in two halves: the edge sets of a column with their embeddings, and the 18 sublayers that consume them
struct StepMode { bool overlap, fuse, lp; int r24; int ra; const float* dt; };
static StepMode step_mode(const InfgenRollout* r, int rows, int edgeless, void* stream) {
  StepMode m;
  m.overlap = O().overlap && g_side && !edgeless;
  m.lp = layers_p_shape(r, rows, edgeless, stream);
  m.fuse = O().edge_fuse == 2 || (O().edge_fuse == 1 && (rows > 256 || m.lp));      // U / Z / SIG stay on chip inside k_edge_fused / k_layers_p
  // the step's rhat rows never leave the library: fp32 rows by default (the reference's arithmetic); rhat_format 1: packed 24-bit
  // rows (kernels.h) when both ends are the kernels that know them - a reduced-precision mode, tests/test_rollout_gpu.py compares the two
  m.r24 = m.fuse && O().fourier_mode != 0 && O().rhat_format == 1;
  m.ra = m.r24;
  // the temporal set's fourth input (the time gap, one of -1 .. -16) as a lookup of its branch (kernels.h: dt_mode)
  m.dt = O().fourier_mode != 0 ? r->four_t_dt : nullptr;
  return m;
}
// few rows: the step's Fourier embeddings side by side in one launch (k_fourier_h_multi)
static bool fourier_multi_ok(int rows, int edgeless) {
  return !edgeless && O().fourier_mode != 0 && rows <= 10240 && !knob::fourier_nomulti && !(O().overlap && g_side);
}

// The Fourier sets of a step, written once for every launch shape of prepare_edges: the three edge sets (raw -> rhat rows, in the
// row format of the step) and FS_XA, the x_a_emb embedding of the rows' raw features (raw2 / cat -> fus_in, infgen_raw_feature's
// middle launch)
enum FourierSet { FS_TEMPORAL, FS_MAP, FS_AGENT, FS_XA };
static FourierArgs step_fourier_set(const InfgenRollout* r, FourierSet k, const StepMode& sm) {
  switch (k) {
    case FS_TEMPORAL:
      return fourier_args(r->et.raw, 4, r->et.total, r->et.cap, r->four_t, nullptr, 0, r->et.rhat, 128, 1, sm.r24, sm.dt, sm.dt != nullptr);
    case FS_MAP: return fourier_args(r->em.raw, 3, r->em.total, r->em.cap, r->four_m, nullptr, 0, r->em.rhat, 128, 1, sm.r24);
    case FS_AGENT: return fourier_args(r->ea.raw, 3, r->ea.total, r->ea.cap, r->four_a, nullptr, 0, r->ea.rhat, 128, 1, sm.ra);
    default: return fourier_args(r->raw2, 2, nullptr, r->S * r->A_cap, r->four_xa, r->cat, 128, r->fus_in + 128, 512, 0, 0);
  }
}

// edge sets of column c + their Fourier embeddings.  zero_totals = false: the totals were cleared by k_integrate; with_xa: FS_XA
// rides along as a fourth set of the multi launch
static int prepare_edges(const InfgenRollout* r, int c, int edgeless, void* stream, bool zero_totals, bool with_xa,
                         unsigned long long* clear_keys = nullptr, bool clear_sync = false) {
  const int rows = r->S * r->A_cap;
  RET_IF(build_edges_impl(r, c, edgeless, stream, zero_totals, clear_keys, clear_sync));
  const StepMode sm = step_mode(r, rows, edgeless, stream);
  if (sm.overlap) {
    hipStream_t ms = (hipStream_t)stream;
    if (hipEventRecord(g_ev_fork, ms) != hipSuccess || hipStreamWaitEvent(g_side, g_ev_fork, 0) != hipSuccess)
      return fail("infgen_decode_layers", "fork failed");
    RET_IF(launch_fourier(step_fourier_set(r, FS_MAP, sm), g_side));
    if (hipEventRecord(g_ev_m, g_side) != hipSuccess) return fail("infgen_decode_layers", "event failed");
    RET_IF(launch_fourier(step_fourier_set(r, FS_AGENT, sm), g_side));
    if (hipEventRecord(g_ev_a, g_side) != hipSuccess) return fail("infgen_decode_layers", "event failed");
    RET_IF(launch_fourier(step_fourier_set(r, FS_TEMPORAL, sm), stream));
  } else if (fourier_multi_ok(rows, edgeless)) {
    // few rows: the three sets side by side in one launch (each is a handful of 128-edge tiles of 35 - 45 us)
    const int n_sets = with_xa ? 4 : 3;
    FourierMultiArgs m;
    for (int k = 0; k < n_sets; ++k) m.set[k] = step_fourier_set(r, (FourierSet)k, sm);
    int cap = r->et.cap > r->em.cap ? r->et.cap : r->em.cap;
    if (r->ea.cap > cap) cap = r->ea.cap;
    const bool wide = knob::fh12_multi_rows > 0 && rows >= knob::fh12_multi_rows && three_terms() && FH_WAVES == 8;
    const int grid = fourier_h_grid(cap, wide);
    { ProfScope _ps(INFGEN_KID_FOURIER, stream);
      if (wide) hipLaunchKernelGGL(k_fourier_h12_multi<3>, dim3(grid, n_sets), dim3(FH12_NT), 0, (hipStream_t)stream, m);
      else hipLaunchKernelGGL(by_terms(k_fourier_h_multi<3>, k_fourier_h_multi_b16<1>, k_fourier_h_multi<1>), dim3(grid, n_sets),
                              dim3(FH_NT), 0, (hipStream_t)stream, m); }
    RET_IF(check_launch("infgen_decode_layers(fourier)"));
  } else if (!edgeless) {
    for (FourierSet k : {FS_TEMPORAL, FS_MAP, FS_AGENT}) RET_IF(launch_fourier(step_fourier_set(r, k, sm), stream));
  }
  return 0;
}

constexpr int LP_REFUSED = -12345;      // layers_p_launch: the runtime refused the cooperative launch, nothing was enqueued
// sync_clear = false: the scenes' counters are already zero (the k_integrate of the previous decode step cleared them: IntegrateArgs.zero_sync)
static int layers_p_launch(const InfgenRollout* r, int c, const StepMode& sm, void* stream, bool sync_clear = true) {
  const int rows = r->S * r->A_cap;
  LayersPArgs a;
  a.rows = rows; a.A_cap = r->A_cap; a.num_layers = r->num_layers;
  a.X = r->X;
  for (int i = 0; i < r->num_layers; ++i) {
    a.attn_t[i] = r->attn_t[i]; a.attn_m[i] = r->attn_m[i]; a.attn_a[i] = r->attn_a[i];
    a.ringK[i] = r->ringK[i]; a.ringV[i] = r->ringV[i]; a.mapK[i] = r->mapK[i]; a.mapV[i] = r->mapV[i];
  }
  a.slot_off = (size_t)(c % r->ring) * stride_rows(r) * D;
  // the agent set's K / V rows double buffered by layer parity: the context's Ka / Va, and the first rows of its U array (4 KB per
  // row, unused while U stays on chip); the scenes' counters in its SIG array (unused for the same reason)
  a.Ka[0] = r->Ka; a.Va[0] = r->Va; a.Ka[1] = r->U; a.Va[1] = r->U + (size_t)rows * D;
  a.et = eset(r->et); a.em = eset(r->em); a.ea = eset(r->ea);
  a.sync = reinterpret_cast<int*>(r->SIG);
  a.trace = nullptr;
  const int lp_trace = knob::lp_trace;
  static unsigned long long* trace_dev = nullptr;
  if (lp_trace) {
    if (!trace_dev && hipMalloc(&trace_dev, 2048 * sizeof(unsigned long long)) != hipSuccess) return fail("infgen_decode_layers", "trace buffer");
    (void)hipMemsetAsync(trace_dev, 0, 2048 * sizeof(unsigned long long), (hipStream_t)stream);
    a.trace = trace_dev;
  }
  if (sync_clear && hipMemsetAsync(a.sync, 0, (size_t)r->S * sizeof(int), (hipStream_t)stream) != hipSuccess)
    return fail("infgen_decode_layers", "memset failed");
  // fewer rows per workgroup while the launch stays within the limit: 8 (one row per wave in the edge loop) up to 256 workgroups,
  // 4 (a row's edge list halved between two waves) up to 128
  // (every bound below is the launch limit lp_limit() = min(resident capacity of THIS device, INFGEN_LP_MAX_GROUPS): a grid beyond the
  // capacity would leave workgroups that never become resident while the resident ones wait for them at the scene counters)
  const int limit = lp_limit();
  a.rows_per_wg = 16;
  for (int rr = 8; rr >= 4 && rr >= knob::lp_rows_min; rr >>= 1)
    if (r->A_cap % rr == 0 && rows / rr <= (rr == 4 ? limit / 2 : limit)) a.rows_per_wg = rr;
  const int gps = r->A_cap / a.rows_per_wg;
  // a batch beyond one launch's workgroups: chunks of whole scenes, one launch after the other (each launch's workgroups are all
  // resident; the stream orders them).  Only 16-row workgroups get here with more than one chunk (fewer rows per workgroup are
  // chosen only when the whole batch fits), so lp_chunk_scenes' groups per scene are this launch's
  const int per = rows / a.rows_per_wg <= limit ? r->S : (a.rows_per_wg == 16 ? lp_chunk_scenes(r, limit) : 0);
  if (per <= 0 || per * gps > infgen_layers_p_capacity()) return fail("infgen_decode_layers", "k_layers_p: batch does not fit the device's resident capacity");
  auto kern = a.rows_per_wg == 4 ? (sm.r24 ? k_layers_p<true, 4> : k_layers_p<false, 4>)
            : a.rows_per_wg == 8 ? (sm.r24 ? k_layers_p<true, 8> : k_layers_p<false, 8>)
                                 : (sm.r24 ? k_layers_p<true, 16> : k_layers_p<false, 16>);
  // A stream that is being captured into a HIP graph cannot take a cooperative launch or the cross-stream ordering below: the
  // (opt-in) graph modes keep the plain launch with the spin limit - their caller owns the GPU
  const bool capturing = is_capturing(stream);
  // polls at a scene counter before the kernel traps: plain launches 2^24 (tens of seconds - a legitimate wait lasts as long as other
  // streams' kernels, milliseconds; only another process's k_layers_p on the same GPU can hold a workgroup off its CU for longer,
  // and a trap is better than a hung device), cooperative launches unlimited, captured launches 2^22; INFGEN_LP_SPIN_LIMIT overrides
  a.spin_limit = capturing ? (1u << 22) : knob::lp_spin_str ? knob::lp_spin_limit : (O().layers_p == 2 ? 0u : (1u << 24));
  // launches of different streams are ordered behind each other (two half-resident launches would wait for each other for ever):
  // every launch is followed by an event record on ITS stream, the next launch - whatever its stream - waits for that event first
  // (a wait on an event of the same stream is a no-op for the hardware queue).  No stream handle outlives the call: a caller may
  // destroy its stream at any time.
  std::unique_lock<std::mutex> lk(g_lp_mu, std::defer_lock);
  LpOrder& ord = g_lp_order[lp_current_device()];
  if (!capturing) {
    lk.lock();
    if (!ord.ev && hipEventCreateWithFlags(&ord.ev, hipEventDisableTiming) != hipSuccess)
      return fail("infgen_decode_layers", "event creation failed");
    if (ord.any && hipStreamWaitEvent((hipStream_t)stream, ord.ev, 0) != hipSuccess) {
      (void)hipGetLastError();
      ord.any = false;            // (the event is unusable: start over rather than fail every later launch)
    }
  }
  const bool lp_coop = O().layers_p == 2;
  for (int s0 = 0; s0 < r->S; s0 += per) {
    const int ns = r->S - s0 < per ? r->S - s0 : per;
    const int n_wg = ns * gps;
    a.row0 = s0 * r->A_cap;
    a.xcd_order = n_wg % (8 * gps) == 0 ? 1 : 0;
    ProfScope _ps(INFGEN_KID_EDGE_ATTN, stream);
    if (capturing || !lp_coop) {
      hipLaunchKernelGGL(kern, dim3(n_wg), dim3(512), 0, (hipStream_t)stream, a);
    } else {
      void* params[] = {&a};
      const hipError_t e = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(kern), dim3(n_wg), dim3(512), params, 0, (hipStream_t)stream);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        if (s0 > 0) return fail("infgen_decode_layers", "k_layers_p: cooperative launch of a later chunk refused");
        g_lp_refused.store(true);          // this and every later call: the per-sublayer launches
        return LP_REFUSED;
      }
    }
  }
  if (!capturing) {
    ord.any = hipEventRecord(ord.ev, (hipStream_t)stream) == hipSuccess;
    if (!ord.any) (void)hipGetLastError();
    lk.unlock();
  }
  if (lp_trace) {          // synchronous dump of the last launch's stamps (diagnostic runs only)
    static int dumps = 0;
    if (dumps++ == lp_trace) {
      std::vector<unsigned long long> h(2048);
      (void)hipStreamSynchronize((hipStream_t)stream);
      (void)hipMemcpy(h.data(), trace_dev, 2048 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
      for (int i = 0; i < 1024 && (i == 0 || h[2 * i + 1]); ++i)
        fprintf(stderr, "[lp trace] %d %llu %llu\n", i, h[2 * i], i ? h[2 * i + 1] - h[2 * i - 1] : 0ull);
    }
  }
  return check_launch("infgen_decode_layers(k_layers_p)");
}

static int layers_core(const InfgenRollout* r, int c, int edgeless, void* stream, bool lp_sync_clear = true) {
  const int rows = r->S * r->A_cap;
  const StepMode sm = step_mode(r, rows, edgeless, stream);
  // a split rollout's phase mark (tl_split): recorded once per step, behind sublayer mark_at or the step's last launch
  bool marked = tl_split.mark_ev == nullptr;
  auto mark = [&](int sublayer, bool last) {
    if (marked || !(last || sublayer >= tl_split.mark_at)) return 0;
    marked = true;
    return hipEventRecord(tl_split.mark_ev, (hipStream_t)stream) == hipSuccess ? 0 : fail("infgen_rollout_run", "phase mark failed");
  };
  if (sm.lp && sm.fuse) {
    const int rc = layers_p_launch(r, c, sm, stream, lp_sync_clear);
    if (rc != LP_REFUSED) { if (rc == 0) RET_IF(mark(0, true)); return rc; }
    // the runtime refused the cooperative launch: the per-sublayer launches below, with the fused edge kernel (the step's rhat
    // rows are already in its format); later calls do not try again (layers_p_shape)
  }
  const bool overlap = sm.overlap, fuse = sm.fuse; const int r24 = sm.r24;
  const size_t slot = (size_t)(c % r->ring) * stride_rows(r) * D;
  const int L = r->num_layers;
  // prologue of the first (temporal) layer; every later layer's prologue is fused into the previous
  // layer's k_attn_post
  float* U = fuse ? nullptr : r->U;
  const float* Z = fuse ? nullptr : r->Z;
  const float* SIG = fuse ? nullptr : r->SIG;
  const int has_pos = fuse ? 0 : 1;                 // the fused edge kernel already added W'vr z + b' sigma to AGG
  // warm requests (tile.cuh: WarmArgs): an edge launch pulls what the node launch after it reads (the layer's post part without
  // W'vr, the next layer's pre part), a node launch the whole post part of the layer after it (W'vr first: the next edge launch)
  const int QB = 16384;                              // bytes of a quarter-matrix (split.cuh: QUARTER fp16 elements)
  // the edgeless column-0 chain through the fused kernels: a row without edges aggregates exactly zero (agg = z = sigma = 0, so
  // agg + W'vr z + b' sigma = +0 in every column) - AGG is zeroed once and the 18 edge launches (54 us each at 1024 scenes) are skipped
  const bool skip_edges = edgeless && fuse;
  if (skip_edges && hipMemsetAsync(r->AGG, 0, (size_t)rows * D * sizeof(float), (hipStream_t)stream) != hipSuccess)
    return fail("infgen_decode_layers", "memset failed");
  auto edge = [&](const float* pack, const float* Ks, const float* Vs, const InfgenEdgeBuf& e, int kv_once = 0, const float* next_pack = nullptr, int fmt = -1) {
    if (skip_edges) return 0;
    if (fuse && O().attn_mode != 0)
      warm_request(pack + AH_POST + 4 * (QB / 4), 48 * QB, next_pack ? next_pack + AH_PRE : nullptr, 16 * QB);
    return fuse ? edge_fused_launch(rows, r->Q, pack, Ks, Vs, eset(e), r->AGG, r->A_cap, kv_once, stream, fmt < 0 ? r24 : fmt)
                : infgen_edge_attn(rows, r->Q, r->U, Ks, Vs, e.off, e.cnt, e.src, e.rhat, r->AGG, r->Z, r->SIG, stream);
  };
  RET_IF(infgen_attn_pre(r->X, rows, r->attn_t[0], 0, r->Q, U, r->ringK[0] + slot, r->ringV[0] + slot, stream));
  auto warm_post = [&](const float* pack) { if (fuse && O().attn_mode != 0) warm_request(pack + AH_POST, 52 * QB, nullptr, 0); };
  for (int i = 0; i < L; ++i) {
    // temporal: K/V of this column sit in the ring (they are the cached layer inputs' projections)
    RET_IF(edge(r->attn_t[i], r->ringK[i], r->ringV[i], r->et, 1, r->attn_m[i]));
    warm_post(r->attn_m[i]);
    RET_IF(infgen_attn_post_pre(r->X, rows, r->attn_t[i], r->AGG, Z, SIG, has_pos, r->attn_m[i], r->Q, U,
                                nullptr, nullptr, stream));
    RET_IF(mark(3 * i, false));
    // map -> agent (bipartite: K/V of the map tokens are per-scene constants)
    if (overlap && i == 0 && hipStreamWaitEvent((hipStream_t)stream, g_ev_m, 0) != hipSuccess)
      return fail("infgen_decode_layers", "join failed");
    RET_IF(edge(r->attn_m[i], r->mapK[i], r->mapV[i], r->em, 0, r->attn_a[i]));
    warm_post(r->attn_a[i]);
    RET_IF(infgen_attn_post_pre(r->X, rows, r->attn_m[i], r->AGG, Z, SIG, has_pos, r->attn_a[i], r->Q, U,
                                r->Ka, r->Va, stream));
    RET_IF(mark(3 * i + 1, false));
    // agent <-> agent
    if (overlap && i == 0 && hipStreamWaitEvent((hipStream_t)stream, g_ev_a, 0) != hipSuccess)
      return fail("infgen_decode_layers", "join failed");
    RET_IF(edge(r->attn_a[i], r->Ka, r->Va, r->ea, 0, i + 1 < L ? r->attn_t[i + 1] : nullptr, sm.ra));
    if (i + 1 < L) {
      warm_post(r->attn_t[i + 1]);
      RET_IF(infgen_attn_post_pre(r->X, rows, r->attn_a[i], r->AGG, Z, SIG, has_pos, r->attn_t[i + 1], r->Q, U,
                                  r->ringK[i + 1] + slot, r->ringV[i + 1] + slot, stream));
    } else {
      RET_IF(infgen_attn_post(r->X, rows, r->attn_a[i], r->AGG, Z, SIG, has_pos, stream));
    }
    RET_IF(mark(3 * i + 2, i + 1 == L));
    // test hook (InfgenRollout.tap_x): the residual stream after triple i
    if (r->tap_x && hipMemcpyAsync(r->tap_x + (size_t)i * rows * D, r->X, (size_t)rows * D * sizeof(float), hipMemcpyDeviceToDevice,
                                   (hipStream_t)stream) != hipSuccess)
      return fail("infgen_decode_layers", "tap copy failed");
  }
  return 0;
}

extern "C" int infgen_decode_layers(const InfgenRollout* r, int c, int edgeless, void* stream) {
  RET_IF(validate(r, "infgen_decode_layers"));
  OptScope _opts(r);
  ProfPhase _pp(edgeless ? t_prof_phase : 1);        // (the edgeless column-0 chain belongs to the prologue)
  const StepMode sm = step_mode(r, r->S * r->A_cap, edgeless, stream);
  const bool lp = sm.lp && sm.fuse && r->SIG != nullptr;      // (k_build_edges zeroes k_layers_p's counters: infgen_rollout_run)
  RET_IF(prepare_edges(r, c, edgeless, stream, true, false, nullptr, lp));
  return layers_core(r, c, edgeless, stream, !lp);
}

// step t's emission over the context's rows, greedy and bare: logits is store_logits' slice of the step, or NULL
static EmitReq step_emit_req(const InfgenRollout* r, int t) {
  const int rows = r->S * r->A_cap;
  float* lg = (r->store_logits && r->logits) ? r->logits + (size_t)t * stride_rows(r) * r->token_size : nullptr;
  return EmitReq{r->X, rows, r->tok_head_pack, r->st_head_pack, r->token_size, lg, r->next_token, r->next_state};
}

extern "C" int infgen_decode_step(const InfgenRollout* r, int t, void* stream) {
  SamplingCtl ctl;
  StepRiders riders;
  RET_IF(validate(r, "infgen_decode_step", &ctl, &riders));
  TokenMaskCtl& mask = riders.mask;
  const auto& [coll, road, score, route, signal] = riders.cfg;
  OptScope _opts(r);
  ProfPhase _pp(1);
  const int rows = r->S * r->A_cap;
  const int c = 1 + t;
  if (t < 0 || c + 1 > r->T - 1) return fail("infgen_decode_step", "step beyond the column range");
  const SceneHead sc = scene_head(r);
  RET_IF(infgen_decode_layers(r, c, 0, stream));
  // a mask stage: the rider refines the sets so far (static, or an earlier stage's) into this column's own, which the next stage
  // and then the heads read row by row
  auto stage = [&](const auto& k) {
    if (!k.bits) return 0;
    RET_IF(launch_mask("infgen_decode_step", mask_head(sc, c, r->first_new, r->token_size, mask), k, t, stream));
    mask = TokenMaskCtl{k.bits, rows, k.ident, {-1, -1, -1}, nullptr};
    return 0;
  };
  RET_IF(stage(coll));      // collision-aware decoding: without the tokens that end in another agent's box
  RET_IF(stage(road));      // road-aware decoding: without the off-road tokens
  RET_IF(stage(signal));    // signal-aware decoding: without the tokens that run a stop line closed at step t
  RET_IF(stage(route));     // route-following decoding: without the tokens that leave the row's route or fall behind on it
  EmitReq q = step_emit_req(r, t);
  q.ctl = ctl; q.mask = mask; q.mask_chain_heads = true;
  q.keys = reinterpret_cast<unsigned long long*>(r->tmp2);      // (scratch of the raw-feature stage, free here)
  if (r->token_logprob) q.token_logprob = r->token_logprob + (size_t)t * stride_rows(r);
  q.k = r->sample_u ? r->sample_k : 1;
  // a draw outside the split kernel with no logits to draw from: the arg-max, silently (sample_logprob unwritten, like a greedy context's)
  if (q.k > 1 && !q.logits && !r->logits_scratch && !emit_plan(q).sample_fused) q.k = 1;
  if (q.k > 1) {
    q.uniform = r->sample_u + (size_t)t * stride_rows(r);
    if (r->sample_logprob) q.sample_logprob = r->sample_logprob + (size_t)t * stride_rows(r);
  }
  const EmitPlan plan = emit_plan(q);
  if (plan.need_logits && !q.logits) q.logits = r->logits_scratch;      // (validate: token_logprob's chain has one)
  RET_IF(emit_tokens("infgen_sample_topk", q, plan, stream));
  RET_IF(infgen_integrate(r, t, stream));
  if (score.out) {      // step scores: the column this step produced, reduced per scene slot
    if (t >= score.steps) return fail("infgen_decode_step", "step score: the log holds fewer steps");
    RET_IF(launch_score("infgen_decode_step", sc, c + 1, score, score.out + (size_t)t * 8, (long long)score.steps * 8, stream));
  }
  RET_IF(infgen_raw_feature(r, c + 1, stream));
  return 0;
}

// The decode steps t0 .. t1 - 1.  With few rows (the Fourier embeddings of a step fit one multi-set launch) the step's tail is
// folded: the edge sets of column c + 1 are built right after the poses of column c + 1 exist, their embeddings and the rows'
// x_a_emb embedding share one launch, and k_integrate also decodes / clears the split arg-max keys, clears the edge totals and
// gathers the raw features - 8 dependent launches between the last sublayer of a step and the first of the next instead of 13
// (memset, k_heads, k_heads_finish, k_integrate, k_rawfeat_prep, k_fourier_h, k_mlpemb_h, memset, k_build_edges,
// k_fourier_h_multi, k_attn_hs ...).  Same arithmetic on the same data as infgen_decode_step (tests compare the two).
struct RunPlan { bool fold = false, lp_steps = false; unsigned long long* keys = nullptr; StepMode sm0{}; };
// what comes in front of the first step: the fold decision and, folded, the cleared keys and the first column's edge sets
static int run_begin(const InfgenRollout* r, int t0, int t1, void* stream, RunPlan* p) {
  StepRiders riders;
  RET_IF(validate(r, "infgen_rollout_run", nullptr, &riders));
  OptScope _opts(r);
  ProfPhase _pp(1);
  const int rows = r->S * r->A_cap;
  const bool sample = r->sample_k > 1 && r->sample_u;
  p->fold = !knob::no_tail_fold && t1 > t0 && fourier_multi_ok(rows, 0) && O().attn_mode != 0 && !sample && !riders.any() && !r->token_logprob && !r->first_new &&
            r->et.total && r->em.total == r->et.total + 1 && r->ea.total == r->et.total + 2;
  if (!p->fold) return 0;
  if (t0 < 0 || 1 + t1 > r->T - 1) return fail("infgen_rollout_run", "step beyond the column range");
  p->keys = reinterpret_cast<unsigned long long*>(r->tmp2);     // (free scratch under attn_mode != 0)
  if (hipMemsetAsync(p->keys, 0, (size_t)rows * sizeof(unsigned long long), (hipStream_t)stream) != hipSuccess)
    return fail("infgen_rollout_run", "memset failed");
  p->sm0 = step_mode(r, rows, 0, stream);
  p->lp_steps = p->sm0.lp && p->sm0.fuse && r->SIG != nullptr;       // the steps' sublayers run as k_layers_p launches
  // (their per-scene counters are zeroed by the kernel in front of every launch - k_build_edges before the first step, k_integrate
  // before the later ones - not by a fill: one launch less per step, and no memset node between the kernels of a captured graph)
  return prepare_edges(r, 1 + t0, 0, stream, true, false, nullptr, p->lp_steps);
}
static int run_step(const InfgenRollout* r, int t, int t1, void* stream, const RunPlan& p) {
  if (!p.fold) return infgen_decode_step(r, t, stream);
  OptScope _opts(r);
  ProfPhase _pp(1);
  const int c = 1 + t;
  RET_IF(layers_core(r, c, 0, stream, !p.lp_steps));
  EmitReq q = step_emit_req(r, t);
  q.keys = p.keys; q.keys_stay = true;
  bool split = false;
  RET_IF(emit_tokens("infgen_rollout_run", q, emit_plan(q), stream, &split));
  // (the last step keeps its edge totals, like infgen_decode_step: RolloutEngine.edge_totals() / overflow checks read them)
  RET_IF(integrate_impl(r, t, stream, split ? p.keys : nullptr, t + 1 < t1, true, t + 1 < t1 && p.lp_steps));
  if (t + 1 < t1) {
    RET_IF(prepare_edges(r, c + 1, 0, stream, false, true, split && integrate_groups(r) > 1 ? p.keys : nullptr));
  } else {          // after the last step only the raw feature of the new column is left (kept: the context's X stays what
                    // infgen_decode_step leaves)
    RET_IF(launch_fourier(step_fourier_set(r, FS_XA, p.sm0), stream));
  }
  return raw_feature_fusion(r, stream);
}

// ---- the split mode: the batch as two halves of S / 2 scenes on two streams of the library's own, the second
// half a set number of sublayers behind the first, so that one half's edge launches (memory requests in flight) share the CUs
// with the other half's Fourier and node launches (matrix and vector pipes, LDS).  A half is a by-value copy of the context with
// every per-scene and per-row pointer advanced to its first scene: the same kernels on the same rows as the whole batch runs.
namespace {
struct SplitRes {                        // what one caller stream's split rollouts run on (never freed: a handful per process)
  hipStream_t st[2] = {nullptr, nullptr};
  hipEvent_t fork = nullptr, join[2] = {nullptr, nullptr}, mark = nullptr;
  int* totals = nullptr;                 // device [6]: the halves' three edge totals each
};
std::mutex g_split_mu;                   // held while a split rollout is enqueued (the table below, and the halves' launch order)
std::unordered_map<void*, SplitRes> g_split_res;      // by the caller's stream handle (a key only: the handle is never used)
constexpr size_t SPLIT_MAX_STREAMS = 8;  // caller streams beyond these keep the single-stream path
std::atomic<int> g_split_runs{0}, g_single_runs{0};
std::mutex g_split_copy_mu;
std::unordered_map<const int*, std::pair<int, bool>> g_split_copy_ok;      // map_scene -> (S, the middle is a copy-group boundary)
}  // namespace
extern "C" int infgen_split_stats(int* split_runs, int* single_runs) {
  if (split_runs) *split_runs = g_split_runs.load();
  if (single_runs) *single_runs = g_single_runs.load();
  return 0;
}
static SplitRes* split_res(void* stream) {      // g_split_mu held
  auto it = g_split_res.find(stream);
  if (it != g_split_res.end()) return &it->second;
  if (g_split_res.size() >= SPLIT_MAX_STREAMS) return nullptr;
  SplitRes v;
  bool ok = hipMalloc(&v.totals, 8 * sizeof(int)) == hipSuccess;
  for (int h = 0; h < 2 && ok; ++h)
    ok = hipStreamCreateWithFlags(&v.st[h], hipStreamNonBlocking) == hipSuccess &&
         hipEventCreateWithFlags(&v.join[h], hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&v.fork, hipEventDisableTiming) == hipSuccess &&
       hipEventCreateWithFlags(&v.mark, hipEventDisableTiming) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); return nullptr; }      // (the caller keeps the single-stream path)
  return &(g_split_res[stream] = v);
}
// copies of a scene (map_scene) stay in one half: the two entries around the middle, read once per array (8 bytes, synchronous -
// like lp_packs_ok; infgen_rollout_validate looks again)
static bool split_copy_boundary(const InfgenRollout* r, bool refresh) {
  if (!r->map_scene || r->S < 2 || r->S % 2) return true;
  std::lock_guard<std::mutex> lk(g_split_copy_mu);
  auto it = g_split_copy_ok.find(r->map_scene);
  if (!refresh && it != g_split_copy_ok.end() && it->second.first == r->S) return it->second.second;
  int mid[2] = {0, 0};
  const bool ok = hipMemcpy(mid, r->map_scene + r->S / 2 - 1, sizeof(mid), hipMemcpyDeviceToHost) == hipSuccess && mid[0] != mid[1];
  (void)hipGetLastError();
  g_split_copy_ok[r->map_scene] = {r->S, ok};
  return ok;
}
// 0: the single-stream path.  Never: an odd S, a split inside a copy group, scenario insertion, a row-group list, a token-mask handle
// (its riders address rows of the whole layout), the residual tap, per-kernel profiling, a stream under capture (no graph with
// parallel branches comes from here).  INFGEN_SPLIT_HALVES=1 (default) additionally wants every by-size kernel choice of the whole
// batch kept by the halves: the big-batch node / heads / embedding kernels and k_edge_fused3 (more than 10,240 rows per half), no
// k_layers_p, k_build_edges and k_integrate on the same side of their scene thresholds (the Fourier variant is carried: tl_split)
static bool run_split_mode(const InfgenRollout* r, int t0, int t1, void* stream) {
  const int mode = split_halves_knob();
  if (mode <= 0 || t1 <= t0 || r->S < 2 || r->S % 2) return false;
  if (r->first_new || O().row_groups || r->token_mask || r->tap_x || g_prof.mask || tl_split.full_rows) return false;
  if (r->et.cap < 2 || r->em.cap < 2 || r->ea.cap < 2 || !r->et.total || !r->em.total || !r->ea.total) return false;
  if (is_capturing(stream)) return false;
  if (mode == 1) {
    const int rows = r->S * r->A_cap, half = r->S / 2;
    if (rows / 2 <= 10240 || rows / 2 <= knob::edge_small || rows / 2 <= knob::attn_hs_max) return false;
    if ((r->S > knob::be_wide_scenes) != (half > knob::be_wide_scenes) || (r->S > knob::int_group_scenes) != (half > knob::int_group_scenes)) return false;
    if (step_mode(r, rows, 0, stream).lp) return false;
  }
  return split_copy_boundary(r, false);
}
static InfgenRollout split_half(const InfgenRollout* r, int h, int* totals) {
  InfgenRollout q = *r;
  q.S = r->S / 2;
  const size_t s0 = h ? (size_t)q.S : 0, A = r->A_cap, row0 = s0 * A, col0 = s0 * r->T * A, m0 = s0 * r->M_cap;
  auto adv = [](auto*& p, size_t n) { if (p) p += n; };
  adv(q.n_agents, s0); adv(q.av_index, s0);
  if (q.map_scene) adv(q.map_scene, s0);      // the map side is shared and only read; without the indirection it is per scene
  else { adv(q.n_map, s0); adv(q.map_pos, 2 * m0); adv(q.map_orient, m0); }
  adv(q.pos, 2 * col0); adv(q.head, col0); adv(q.state, col0); adv(q.token, col0); adv(q.grid, col0);
  adv(q.tmask, col0); adv(q.imask, col0); adv(q.catflag, col0); adv(q.type, row0); adv(q.bos, row0);
  adv(q.cat_agent, row0 * D);
  for (int l = 0; l < INFGEN_MAX_LAYERS; ++l) {
    adv(q.ringK[l], row0 * D); adv(q.ringV[l], row0 * D);      // (the slots keep the whole layout's stride: stride_rows)
    if (!q.map_scene) { adv(q.mapK[l], m0 * D); adv(q.mapV[l], m0 * D); }
  }
  adv(q.X, row0 * D); adv(q.Q, row0 * D); adv(q.U, row0 * 8 * D); adv(q.Ka, row0 * D); adv(q.Va, row0 * D); adv(q.AGG, row0 * D);
  adv(q.Z, row0 * 8 * D); adv(q.SIG, row0 * 8);
  int k = 0;
  for (InfgenEdgeBuf* e : {&q.et, &q.em, &q.ea}) {      // rows of off / cnt, its own half of the capacity, its own total
    const int capA = e->cap / 2;
    adv(e->off, row0); adv(e->cnt, row0);
    if (h) { adv(e->src, (size_t)capA); adv(e->raw, (size_t)capA * 4); adv(e->rhat, (size_t)capA * D); }
    e->cap = h ? e->cap - capA : capA;
    e->total = totals + 3 * h + k++;
  }
  adv(q.raw2, row0 * 4); adv(q.cat, row0 * D); adv(q.fus_in, row0 * 512); adv(q.tmp1, row0 * D); adv(q.tmp2, row0 * D);
  adv(q.next_token, row0); adv(q.next_state, row0); adv(q.logits, row0 * r->token_size);
  adv(q.teacher_token, col0); adv(q.teacher_state, col0); adv(q.teacher_grid, col0); adv(q.teacher_pos, 2 * col0); adv(q.teacher_head, col0);
  adv(q.replay_row, row0);
  adv(q.pred_traj, row0 * r->R * 2); adv(q.pred_head, row0 * r->R); adv(q.pred_state, row0 * r->R);
  adv(q.sample_u, row0); adv(q.logits_scratch, row0 * r->token_size); adv(q.sample_temp_row, row0);
  adv(q.sample_logprob, row0); adv(q.token_logprob, row0);
  q.opts = O(); q.opts.use = 1;
  q.opts.overlap = 0;                      // (infgen_set_overlap's side stream and the split exclude each other: the split wins)
  return q;
}
// the context's totals from the halves': the sums - or, where a half ran over its own share of the capacity, more than the whole
// capacity, so that the callers' overflow checks answer as they would for the whole batch
__global__ void k_split_totals(const int* half, int* t, int* m, int* a, int cap_t, int cap_m, int cap_a) {
  if (threadIdx.x >= 3 || blockIdx.x) return;
  const int k = threadIdx.x, cap = k == 0 ? cap_t : k == 1 ? cap_m : cap_a, capA = cap / 2;
  const int na = half[k], nb = half[3 + k];
  int n = na + nb;
  if ((na > capA || nb > cap - capA) && n <= cap) n = cap + 1;
  *(k == 0 ? t : k == 1 ? m : a) = n;
}
static int run_split(const InfgenRollout* r, int t0, int t1, void* stream, SplitRes& res) {
  hipStream_t cs = (hipStream_t)stream;
  const int full_rows = r->S * r->A_cap;
  InfgenRollout half[2] = {split_half(r, 0, res.totals), split_half(r, 1, res.totals)};
  const int L3 = 3 * r->num_layers;
  const int off_knob = split_offset_knob(), off = off_knob < 0 ? 0 : off_knob > L3 ? L3 : off_knob;
  if (hipEventRecord(res.fork, cs) != hipSuccess || hipStreamWaitEvent(res.st[0], res.fork, 0) != hipSuccess ||
      hipStreamWaitEvent(res.st[1], res.fork, 0) != hipSuccess)
    return fail("infgen_rollout_run", "fork failed");
  struct TlScope { ~TlScope() { tl_split = SplitTl{0, 1, nullptr, -1}; } } _tl;
  auto body = [&]() {
    RunPlan plan[2];
    for (int h = 0; h < 2; ++h) {
      tl_split = SplitTl{full_rows, 2, nullptr, -1};
      RET_IF(run_begin(&half[h], t0, t1, res.st[h], &plan[h]));
    }
    for (int t = t0; t < t1; ++t) {
      // the first half marks its stream `off` sublayers into the step; the second half's step starts behind the mark
      tl_split = SplitTl{full_rows, 2, off > 0 ? res.mark : nullptr, off - 1};
      RET_IF(run_step(&half[0], t, t1, res.st[0], plan[0]));
      tl_split = SplitTl{full_rows, 2, nullptr, -1};
      if (off > 0 && hipStreamWaitEvent(res.st[1], res.mark, 0) != hipSuccess) return fail("infgen_rollout_run", "phase wait failed");
      RET_IF(run_step(&half[1], t, t1, res.st[1], plan[1]));
    }
    return 0;
  };
  const int rc = body();
  // the join comes whatever happened: the caller's stream stays ordered behind everything that was enqueued
  bool joined = true;
  for (int h = 0; h < 2; ++h)
    joined = hipEventRecord(res.join[h], res.st[h]) == hipSuccess && hipStreamWaitEvent(cs, res.join[h], 0) == hipSuccess && joined;
  if (rc) return rc;
  if (!joined) return fail("infgen_rollout_run", "join failed");
  hipLaunchKernelGGL(k_split_totals, dim3(1), dim3(64), 0, cs, res.totals, r->et.total, r->em.total, r->ea.total, r->et.cap, r->em.cap, r->ea.cap);
  return check_launch("infgen_rollout_run(totals)");
}

extern "C" int infgen_rollout_run(const InfgenRollout* r, int t0, int t1, void* stream) {
  RET_IF(validate(r, "infgen_rollout_run"));
  {
    OptScope _opts(r);
    if (run_split_mode(r, t0, t1, stream)) {
      std::lock_guard<std::mutex> lk(g_split_mu);
      if (SplitRes* res = split_res(stream)) {
        ++g_split_runs;
        return run_split(r, t0, t1, stream, *res);
      }
    }
  }
  ++g_single_runs;
  RunPlan plan;
  RET_IF(run_begin(r, t0, t1, stream, &plan));
  for (int t = t0; t < t1; ++t) RET_IF(run_step(r, t, t1, stream, plan));
  return 0;
}

// ---------------------------------------------------------------------------------- scenario insertion
extern "C" int infgen_occupancy(const InfgenRollout* r, int c, float* occ, void* stream) {
  RET_IF(validate(r, "infgen_occupancy"));
  OccupancyArgs a{scene_of(r), c, r->grid_size, occ};
  hipLaunchKernelGGL(k_occupancy, dim3(r->S), dim3(NT), 0, (hipStream_t)stream, a);
  return check_launch("infgen_occupancy");
}

// occupancy vector AND its embedding (seed_agent_occ_embed, an MLPLayer 1961 -> 128 -> 128) in one launch
static int occupancy_embed_impl(const InfgenRollout* r, int c, float* occ, const float* embed_pack, float* emb, const int* active,
                                void* stream) {
  RET_IF(validate(r, "infgen_occupancy_embed"));
  if (r->grid_size > 2048) return fail("infgen_occupancy_embed", "grid larger than 2048 cells");
  OccEmbedArgs a{scene_of(r), c, r->grid_size, occ, embed_pack, emb, active};
  hipLaunchKernelGGL(k_occupancy_embed, dim3(r->S), dim3(NT), 0, (hipStream_t)stream, a);
  return check_launch("infgen_occupancy_embed");
}

extern "C" int infgen_occupancy_embed(const InfgenRollout* r, int c, float* occ, const float* embed_pack, float* emb, void* stream) {
  return occupancy_embed_impl(r, c, occ, embed_pack, emb, nullptr, stream);
}

extern "C" int infgen_point_edges(const InfgenRollout* r, int c, const int* centre_row, const int* active,
                                  int exclude_centre, int which, float r_agent, int k_agent, float r_map, int k_map,
                                  const InfgenEdgeBuf* ea, const InfgenEdgeBuf* em, void* stream) {
  RET_IF(validate(r, "infgen_point_edges"));
  hipStream_t s = (hipStream_t)stream;
  if (((which & 1) && hipMemsetAsync(ea->total, 0, sizeof(int), s) != hipSuccess) ||
      ((which & 2) && hipMemsetAsync(em->total, 0, sizeof(int), s) != hipSuccess))
    return fail("infgen_point_edges", "memset failed");
  PointEdgesArgs a{scene_of(r), c, centre_row, active, exclude_centre, which, r_agent, k_agent, r_map, k_map,
                   ebuf(*ea), ebuf(*em)};
  hipLaunchKernelGGL(k_point_edges, dim3(r->S), dim3(128), 0, s, a);
  return check_launch("infgen_point_edges");
}

static int insert_decide_impl(const InfgenRollout* r, int t, int force_enter, int max_new,
                              const float* lg_state, const float* lg_type, const float* shape, const float* lg_pos,
                              const float* occ, int* active, int* n_new, int* inserted, int* new_row,
                              float* new_shape, int* new_cell, int sample_k, const float* uniform, void* stream,
                              bool grid = true, float r_seed = 0.f, const InfgenSampling* sampling = nullptr,
                              const InsertMaskCtl* mask = nullptr) {
  RET_IF(validate(r, "infgen_insert_decide"));
  if (sample_k > 16) return fail("infgen_insert_decide", "sample_k must be <= 16");
  if (sample_k > 1 && !uniform) return fail("infgen_insert_decide", "cell sampling needs uniforms");
  InsertDecideArgs a;
  a.ctl = SAMPLING_DEFAULT;
  if (sample_k > 1) RET_IF(sampling_ctl("infgen_insert_decide", sampling, &a.ctl));
  a.ctl.temperature_row = nullptr;         // (one draw per scene: scalars only)
  a.st = scene_of(r); a.c = 1 + t; a.t = t; a.R = r->R; a.grid_size = r->grid_size; a.force_enter = force_enter;
  a.max_new = max_new; a.sample_k = sample_k; a.uniform = uniform;
  a.grid_xy = r->grid_xy; a.lg_state = lg_state; a.lg_type = lg_type; a.shape = shape;
  a.lg_pos = lg_pos; a.occ = occ; a.n_agents = const_cast<int*>(r->n_agents); a.type = const_cast<int*>(r->type);
  a.active = active; a.n_new = n_new; a.inserted = inserted; a.new_row = new_row; a.new_shape = new_shape;
  a.new_cell = new_cell; a.pred_traj = r->pred_traj; a.pred_head = r->pred_head; a.pred_state = r->pred_state;
  a.r_seed = r_seed;
  if (mask) {
    if (!grid) return fail("infgen_insert_decide", "insertion rules: a model without the grid token has no cell to mask");
    InsertDecideMaskArgs ma;
    static_cast<InsertDecideArgs&>(ma) = a;
    ma.m = *mask;
    hipLaunchKernelGGL((k_insert_decide<true, true>), dim3(r->S), dim3(64), 0, (hipStream_t)stream, ma);
  } else if (grid) hipLaunchKernelGGL((k_insert_decide<true, false>), dim3(r->S), dim3(64), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((k_insert_decide<false, false>), dim3(r->S), dim3(64), 0, (hipStream_t)stream, a);
  return check_launch("infgen_insert_decide");
}

// ---------------------------------------------------------------------------------- insertion rules
// the argument checks of include/infgen_hip.h ("insertion rules") and the one launch of k_insert_cell_mask
static int insert_cell_mask_launch(const char* me, const InsertCellMaskArgs& a, void* stream) {
  const float dist[6] = {a.ko_back, a.ko_front, a.ko_half, a.clearance, a.edge_clearance, a.lane_dist};
  for (float x : dist)
    if (!std::isfinite(x) || x < 0.f) return fail(me, "insertion rules: every distance must be finite and >= 0");
  if (a.S < 1 || a.T < 1 || a.A_cap < 1) return fail(me, "insertion rules: empty layout");
  if (a.copies < 1 || a.S % a.copies != 0) return fail(me, "insertion rules: copies must be at least 1 and divide S");
  if (a.G < 1 || a.G > IM_MAX_CELLS) return fail(me, "insertion rules: G must be in 1..8192");
  if (a.W != (a.G + 127) / 128 * 4) return fail(me, "insertion rules: words must be ceil(G / 32) rounded up to a multiple of 4");
  if (a.c < 0 || a.c >= a.T) return fail(me, "insertion rules: column out of range");
  if (a.A_cap > MAX_SCENE_AGENTS) return fail(me, "insertion rules: A_cap exceeds INFGEN_Q_MAX_AGENTS");
  if (a.static_pass < 0 || a.static_pass > 2) return fail(me, "insertion rules: static_pass must be 0, 1 or 2");
  if (a.rules & ~(IM_KEEPOUT | IM_CLEARANCE | IM_EDGES | IM_LANES | IM_ZONES)) return fail(me, "insertion rules: unknown rule bit");
  if (!a.pos || !a.head || !a.state || !a.n_agents || !a.av_index || !a.grid_xy) return fail(me, "insertion rules: needs the scene arrays and the grid");
  if (!a.allowed || !a.allowed_count || !a.live) return fail(me, "insertion rules: needs allowed, allowed_count and live");
  if (a.static_pass != 0 && !a.static_bits) return fail(me, "insertion rules: static_pass 1 and 2 need static_bits");
  if ((a.rules & IM_CLEARANCE) && !a.shape) return fail(me, "insertion rules: clearance needs the rows' shape array [S][A_cap][3]");
  if ((a.rules & IM_EDGES) && (!a.records || !a.n_records || a.rec_cap < 0))
    return fail(me, "insertion rules: edge_clearance needs the road-record table and its counts");
  if ((a.rules & IM_LANES) && (!a.map_pos || !a.map_type || !a.n_map || a.M_cap < 0))
    return fail(me, "insertion rules: near_lane needs map_pos, map_type and n_map");
  if ((a.rules & IM_ZONES) && (!a.zones || !a.n_zones || a.Z < 0)) return fail(me, "insertion rules: zones need the zone table and its counts");
  if (misaligned16(a.allowed, a.static_bits, a.records, a.zones)) return fail(me, "insertion rules: the bit, record and zone tables must be 16-byte aligned");
  hipLaunchKernelGGL(k_insert_cell_mask, dim3(a.S), dim3(IM_NT), 0, (hipStream_t)stream, a);
  return check_launch(me);
}

extern "C" int infgen_insert_cell_mask(const float* pos, const float* head, const int* state, const int* n_agents, const int* av_index,
                                       const float* shape, int S, int A_cap, int T, int c, const float* grid_xy, int G, int rules,
                                       const float* keepout, float clearance, float edge_clearance, float lane_dist,
                                       unsigned lane_types, const float* records, const int* n_records, int rec_cap,
                                       const float* map_pos, const long long* map_type, const int* n_map, int M_cap,
                                       const float* zones, const int* n_zones, int Z, int copies, int static_pass,
                                       uint32_t* static_bits, uint32_t* allowed, int words, int* allowed_count, int* live,
                                       int* count_log, long long count_stride, void* stream) {
  const char* me = "infgen_insert_cell_mask";
  if ((rules & IM_KEEPOUT) && !keepout) return fail(me, "insertion rules: ego_keepout needs its three floats");
  InsertCellMaskArgs a{};
  a.S = S; a.A_cap = A_cap; a.T = T; a.c = c; a.G = G; a.W = words;
  a.pos = pos; a.head = head; a.state = state; a.n_agents = n_agents; a.av_index = av_index; a.shape = shape; a.grid_xy = grid_xy;
  a.rules = rules; a.static_pass = static_pass;
  if (rules & IM_KEEPOUT) { a.ko_back = keepout[0]; a.ko_front = keepout[1]; a.ko_half = keepout[2]; }
  a.clearance = clearance; a.edge_clearance = edge_clearance; a.lane_dist = lane_dist; a.lane_types = lane_types;
  a.records = records; a.n_records = n_records; a.rec_cap = rec_cap;
  a.map_pos = map_pos; a.map_type = map_type; a.n_map = n_map; a.M_cap = M_cap;
  a.zones = zones; a.n_zones = n_zones; a.Z = Z; a.copies = copies;
  a.static_bits = static_bits; a.allowed = allowed; a.allowed_count = allowed_count; a.live = live;
  a.count_log = count_log; a.count_stride = count_stride;
  return insert_cell_mask_launch(me, a, stream);
}

static int insert_mask_ctl(const char* me, int grid_size, const uint32_t* allowed, int words, const int* type_allowed,
                           const int* max_agents, const int* live, float* box_shape, InsertMaskCtl* m) {
  if (!allowed || misaligned16(allowed)) return fail(me, "insertion rules: needs a 16-byte aligned allowed table");
  if (words < (grid_size + 31) / 32) return fail(me, "insertion rules: words is below ceil(grid_size / 32)");
  if (!type_allowed || !(type_allowed[0] || type_allowed[1] || type_allowed[2]))
    return fail(me, "insertion rules: types must allow at least one agent type");
  if (max_agents && !live) return fail(me, "insertion rules: max_agents needs the live counts of infgen_insert_cell_mask");
  *m = InsertMaskCtl{allowed, words, {type_allowed[0], type_allowed[1], type_allowed[2]}, max_agents, live, box_shape};
  return 0;
}

extern "C" int infgen_insert_decide(const InfgenRollout* r, int t, int force_enter, int max_new,
                                    const float* lg_state, const float* lg_type, const float* shape, const float* lg_pos,
                                    const float* occ, int* active, int* n_new, int* inserted, int* new_row,
                                    float* new_shape, int* new_cell, void* stream) {
  return insert_decide_impl(r, t, force_enter, max_new, lg_state, lg_type, shape, lg_pos, occ, active, n_new, inserted, new_row,
                            new_shape, new_cell, 1, nullptr, stream);
}

// the same with the reference's stochastic cell choice (softmax -> topk(insert_beam_size) -> multinomial, agent_decoder.py:1900-1904)
// in a reproducible form: inverse CDF over the sample_k most probable cells with uniform[s]; a sampled cell that is occupied spends
// the iteration and leaves the scene active (:1906-1909)
extern "C" int infgen_insert_decide_topk(const InfgenRollout* r, int t, int force_enter, int max_new,
                                         const float* lg_state, const float* lg_type, const float* shape, const float* lg_pos,
                                         const float* occ, int* active, int* n_new, int* inserted, int* new_row,
                                         float* new_shape, int* new_cell, int sample_k, const float* uniform, void* stream) {
  return insert_decide_impl(r, t, force_enter, max_new, lg_state, lg_type, shape, lg_pos, occ, active, n_new, inserted, new_row,
                            new_shape, new_cell, sample_k, uniform, stream);
}

// ... with temperature and nucleus truncation of the cell draw (scalars; sampling->temperature_row is ignored)
extern "C" int infgen_insert_decide_topk_ex(const InfgenRollout* r, int t, int force_enter, int max_new,
                                            const float* lg_state, const float* lg_type, const float* shape, const float* lg_pos,
                                            const float* occ, int* active, int* n_new, int* inserted, int* new_row,
                                            float* new_shape, int* new_cell, int sample_k, const float* uniform,
                                            const InfgenSampling* sampling, void* stream) {
  return insert_decide_impl(r, t, force_enter, max_new, lg_state, lg_type, shape, lg_pos, occ, active, n_new, inserted, new_row,
                            new_shape, new_cell, sample_k, uniform, stream, true, 0.f, sampling);
}

// ... under insertion rules: banned cells are no candidates, banned types are not chosen, a scene at its budget does not enter
extern "C" int infgen_insert_decide_mask(const InfgenRollout* r, int t, int force_enter, int max_new,
                                         const float* lg_state, const float* lg_type, const float* shape, const float* lg_pos,
                                         const float* occ, int* active, int* n_new, int* inserted, int* new_row,
                                         float* new_shape, int* new_cell, int sample_k, const float* uniform,
                                         const InfgenSampling* sampling, const uint32_t* allowed, int words, const int* type_allowed,
                                         const int* max_agents, const int* live, void* stream) {
  RET_IF(validate(r, "infgen_insert_decide_mask"));
  if (r->no_grid_token) return fail("infgen_insert_decide_mask", "insertion rules: a model without the grid token has no cell to mask");
  InsertMaskCtl m;
  RET_IF(insert_mask_ctl("infgen_insert_decide_mask", r->grid_size, allowed, words, type_allowed, max_agents, live, nullptr, &m));
  return insert_decide_impl(r, t, force_enter, max_new, lg_state, lg_type, shape, lg_pos, occ, active, n_new, inserted, new_row,
                            new_shape, new_cell, sample_k, uniform, stream, true, 0.f, sampling, &m);
}

static int insert_finalize_impl(const InfgenRollout* r, int c, float angle_interval, const int* inserted, const int* new_row,
                                const float* lg_heading, int n_heading, const float* offset, float* hv_ovr, void* stream,
                                bool head_token = true, bool xy_offset = true) {
  RET_IF(validate(r, "infgen_insert_finalize"));
  InsertFinalizeArgs a{scene_of(r), c, angle_interval, inserted, new_row, lg_heading, n_heading, offset, hv_ovr};
  const hipStream_t hs = (hipStream_t)stream;
  if (head_token && xy_offset) hipLaunchKernelGGL((k_insert_finalize<true, true>), dim3(r->S), dim3(64), 0, hs, a);
  else if (xy_offset) hipLaunchKernelGGL((k_insert_finalize<false, true>), dim3(r->S), dim3(64), 0, hs, a);
  else if (head_token) hipLaunchKernelGGL((k_insert_finalize<true, false>), dim3(r->S), dim3(64), 0, hs, a);
  else hipLaunchKernelGGL((k_insert_finalize<false, false>), dim3(r->S), dim3(64), 0, hs, a);
  return check_launch("infgen_insert_finalize");
}

extern "C" int infgen_insert_finalize(const InfgenRollout* r, int c, float angle_interval, const int* inserted,
                                      const int* new_row, const float* lg_heading, int n_heading, const float* offset,
                                      float* hv_ovr, void* stream) {
  return insert_finalize_impl(r, c, angle_interval, inserted, new_row, lg_heading, n_heading, offset, hv_ovr, stream);
}

// ---------------------------------------------------------------------------------- teacher-forced forward
extern "C" int infgen_radius_edges(const InfgenRadiusEdges* r, const InfgenEdgeBuf* e, void* stream) {
  if (!r || !e) return fail("infgen_radius_edges", "null argument");
  if (r->n_q <= 0) return 0;
  if (r->K <= 0) return fail("infgen_radius_edges", "K must be positive");
  if (r->gap_rule < 0 || r->gap_rule > 2) return fail("infgen_radius_edges", "gap_rule must be 0, 1 or 2");
  RadiusEdgesArgs a{r->n_q, r->q_node, r->q_pt, r->q_c0, r->q_c1, r->q_self, r->q_pair_off, r->p_pos, r->p_head, r->p_inv,
                    r->c_pos, r->c_head, r->c_inv, r->c_ok, r->c_src, r->pair_ok, r->radius, r->K, r->gap_rule, r->index_diff,
                    ebuf(*e), r->e_base};
  hipLaunchKernelGGL(k_radius_edges, dim3(ceil_div(r->n_q, 4)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("infgen_radius_edges");
}

extern "C" int infgen_motion_features(const float* pos, const float* head, const int* state, const unsigned char* gap_mask,
                                      int rows, int T, float* out, void* stream) {
  if (rows <= 0 || T <= 0) return 0;
  MotionFeatArgs a{pos, head, state, gap_mask, rows, T, out};
  hipLaunchKernelGGL(k_motion_features, dim3(ceil_div(rows * T, 256)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("infgen_motion_features");
}

// ---------------------------------------------------------------------------------- insertion sub-loop, sequenced here
namespace {
inline int round_up_i(int x, int m) { return (x + m - 1) / m * m; }
// MLPLayer pack (packing.pack_mlp_layer, K0 = 128): two descriptors of infgen_linear_multi
void mlp_layer_descs(const float* X, int rows, const float* pack, int n_out, float* hid, float* out, InfgenLinearDesc& d1,
                     InfgenLinearDesc& d2) {
  const int o_b0 = 128 * 128, o_w3 = o_b0 + 3 * 128, npad = round_up_i(n_out, 32);
  d1 = InfgenLinearDesc{X, 128, nullptr, rows, 128, pack, 128, pack + o_b0, 128, nullptr, nullptr, pack + o_b0 + 128, pack + o_b0 + 256,
                        1, hid, 128};
  d2 = InfgenLinearDesc{hid, 128, nullptr, rows, 128, pack + o_w3, npad, pack + o_w3 + 128 * npad, n_out, nullptr, nullptr, nullptr,
                        nullptr, 0, out, n_out};
}
int gather_rows(const float* src, const int* list, const int* mask, int n, int limit, float* dst, void* stream) {
  hipLaunchKernelGGL(k_gather_rows, dim3(ceil_div(n * 32, NT)), dim3(NT), 0, (hipStream_t)stream, src, list, mask, n, limit, dst);
  return check_launch("k_gather_rows");
}
int scatter_rows2(const float* src0, const float* src1, const int* list, const int* mask, int n, float* dst0, float* dst1,
                  void* stream) {
  hipLaunchKernelGGL(k_scatter_rows2, dim3(ceil_div(n * 32, NT)), dim3(NT), 0, (hipStream_t)stream, src0, src1, list, mask, n, dst0,
                     dst1);
  return check_launch("k_scatter_rows2");
}
// a row without edges has agg = z = sigma = 0: the positional part adds exactly nothing and is skipped
int edgeless(float* X, int rows, const float* pack, const InfgenInsertion* I, void* stream) {
  return infgen_attn_post(X, rows, pack, I->zero_agg, I->zero_z, I->zero_sig, 0, stream);
}
}  // namespace

// the rule arguments of infgen_insert_seed_rules, checked by the two launches they reach
struct InsertSeedRules {
  InsertCellMaskArgs mask;      // the rule parameters and outputs; the scene, the column and the pass are filled in per call
  const int* type_allowed; const int* max_agents; float* box_shape; int log_steps;
};

static int insert_seed_impl(const InfgenRollout* r, const InfgenInsertion* I, int t, int it, int riders, const float* uniform,
                            void* stream, const InsertSeedRules* rules) {
  RET_IF(validate(r, "infgen_insert_seed"));
  if (!I) return fail("infgen_insert_seed", "null insertion block");
  if (I->no_grid_token != r->no_grid_token) return fail("infgen_insert_seed", "no_grid_token differs between the context and the block");
  if (I->no_grid_token && !I->head_pos_xy) return fail("infgen_insert_seed", "no_grid_token needs head_pos_xy");
  InsertMaskCtl rules_ctl;
  if (rules) {
    if (I->no_grid_token) return fail("infgen_insert_seed_rules", "insertion rules: a model without the grid token has no cell to mask");
    if (I->max_new < 1 || I->max_new > 10) return fail("infgen_insert_seed_rules", "insertion rules: per_step must be in 1..10");
    if (!rules->box_shape) return fail("infgen_insert_seed_rules", "insertion rules: needs the rows' shape array [S][A_cap][3]");
    if (rules->mask.count_log && (rules->log_steps < 1 || t >= rules->log_steps))
      return fail("infgen_insert_seed_rules", "insertion rules: the count log is too short");
    RET_IF(insert_mask_ctl("infgen_insert_seed_rules", r->grid_size, rules->mask.allowed, rules->mask.W, rules->type_allowed,
                           rules->max_agents, rules->mask.live, rules->box_shape, &rules_ctl));
  }
  OptScope _opts(r);
  hipStream_t hs = (hipStream_t)stream;
  const int S = r->S, rows = r->S * r->A_cap, c = 1 + t, G = r->grid_size;
  const bool grid = !I->no_grid_token;      // use_grid_token = False: no occupancy, no occ2sa sublayers (agent_decoder.py:1851-1868)
  if (grid) {
    RET_IF(occupancy_embed_impl(r, c, I->occ, I->occ_embed, I->occ_emb, I->active, stream));
    for (int i = 0; i < 3; ++i) RET_IF(infgen_attn_pre(I->occ_emb, S, I->attn_occ2sa[i], 1, nullptr, nullptr, I->Kocc[i], I->Vocc[i], stream));
  }
  // edges into the seed node (the ego's pose): agents every iteration, map tokens once per step
  RET_IF(infgen_point_edges(r, c, r->av_index, I->active, 0, it == 0 ? 3 : 1, I->r_seed, 300, I->r_seed, 2048, &I->ea_s, &I->em_s, stream));
  RET_IF(infgen_fourier_embed(I->ea_s.raw, 3, I->ea_s.total, I->ea_s.cap, I->four_a2sa, nullptr, 0, I->ea_s.rhat, 128, 1, stream));
  if (it == 0) {
    RET_IF(infgen_fourier_embed(I->em_s.raw, 3, I->em_s.total, I->em_s.cap, I->four_pt2sa, nullptr, 0, I->em_s.rhat, 128, 1, stream));
    // every agent row passes every seed sublayer edgelessly; its K / V feed the a2sa layers: all rows once per step
    if (hipMemcpyAsync(I->Xc, r->X, (size_t)rows * D * sizeof(float), hipMemcpyDeviceToDevice, hs) != hipSuccess)
      return fail("infgen_insert_seed", "copy failed");
    for (int i = 0; i < 3; ++i) {
      if (grid) RET_IF(edgeless(I->Xc, rows, I->attn_occ2sa[i], I, stream));
      // the post part of the map sublayer and the K / V projections of the agent sublayer in one launch
      RET_IF(infgen_attn_post_pre(I->Xc, rows, I->attn_pt2sa[i], I->zero_agg, I->zero_z, I->zero_sig, 0, I->attn_a2sa[i], nullptr, nullptr,
                                  I->Ksa[i], I->Vsa[i], stream));
      RET_IF(edgeless(I->Xc, rows, I->attn_a2sa[i], I, stream));
    }
  }
  // the seed rows [0, S) and, edgelessly, the rows the previous iteration appended [S, 2 S) (one slot per scene)
  const int R = riders ? 2 * S : S;
  RET_IF(gather_rows(I->f_seed, nullptr, nullptr, S, 1, I->XS, stream));
  if (riders) RET_IF(gather_rows(r->X, I->prev_row, I->prev_mask, S, rows, I->XS + (size_t)S * D, stream));
  if (grid) RET_IF(infgen_attn_pre(I->XS, R, I->attn_occ2sa[0], 0, I->QS, nullptr, nullptr, nullptr, stream));
  else RET_IF(infgen_attn_pre(I->XS, R, I->attn_pt2sa[0], 0, I->QS, I->US, nullptr, nullptr, stream));
  for (int i = 0; i < 3; ++i) {
    if (grid) {
      RET_IF(infgen_edge_attn(S, I->QS, nullptr, I->Kocc[i], I->Vocc[i], I->occ_off, I->occ_cnt, I->occ_src, nullptr, I->AGGS, nullptr,
                              I->SIGS, stream));
      RET_IF(infgen_attn_post_pre(I->XS, R, I->attn_occ2sa[i], I->AGGS, I->ZS, I->SIGS, 0, I->attn_pt2sa[i], I->QS, I->US, nullptr, nullptr,
                                  stream));
    }
    // (the map edges of a step are built once: scenes that stopped inserting are masked out instead, their seed rows are not read)
    RET_IF(edge_attn_impl(S, I->QS, I->US, I->mapK[i], I->mapV[i], I->em_s.off, I->em_s.cnt, I->em_s.src, I->em_s.rhat, I->AGGS,
                          I->ZS, I->SIGS, 1, stream, I->active));
    RET_IF(infgen_attn_post_pre(I->XS, R, I->attn_pt2sa[i], I->AGGS, I->ZS, I->SIGS, 1, I->attn_a2sa[i], I->QS, I->US,
                                riders ? I->KN : nullptr, riders ? I->VN : nullptr, stream));
    if (riders) {
      RET_IF(scatter_rows2(I->KN + (size_t)S * D, I->VN + (size_t)S * D, I->prev_row, I->prev_mask, S, I->Ksa[i], I->Vsa[i], stream));
    }
    RET_IF(infgen_edge_attn_mode(S, I->QS, I->US, I->Ksa[i], I->Vsa[i], I->ea_s.off, I->ea_s.cnt, I->ea_s.src, I->ea_s.rhat, I->AGGS,
                                 I->ZS, I->SIGS, 1, stream));
    // a2sa[i] feeds occ2sa[i + 1] (full model) or pt2sa[i + 1] (use_grid_token = False)
    if (i < 2 && grid) RET_IF(infgen_attn_post_pre(I->XS, R, I->attn_a2sa[i], I->AGGS, I->ZS, I->SIGS, 1, I->attn_occ2sa[i + 1], I->QS,
                                                   nullptr, nullptr, nullptr, stream));
    else if (i < 2) RET_IF(infgen_attn_post_pre(I->XS, R, I->attn_a2sa[i], I->AGGS, I->ZS, I->SIGS, 1, I->attn_pt2sa[i + 1], I->QS, I->US,
                                                nullptr, nullptr, stream));
    else RET_IF(infgen_attn_post(I->XS, R, I->attn_a2sa[i], I->AGGS, I->ZS, I->SIGS, 1, stream));
  }
  // the four seed heads in two launches (the position head: the cell logits, or the xy regression for use_grid_token = False)
  InfgenLinearDesc d1[4], d2[4];
  const size_t hs_ = (size_t)S * 128;
  mlp_layer_descs(I->XS, S, I->head_state, 2, I->hid, I->lg_state, d1[0], d2[0]);
  mlp_layer_descs(I->XS, S, I->head_type, 3, I->hid + hs_, I->lg_type, d1[1], d2[1]);
  mlp_layer_descs(I->XS, S, I->head_shape, 3, I->hid + 2 * hs_, I->shape, d1[2], d2[2]);
  if (grid) mlp_layer_descs(I->XS, S, I->head_pos, G, I->hid + 3 * hs_, I->lg_pos, d1[3], d2[3]);
  else mlp_layer_descs(I->XS, S, I->head_pos_xy, 2, I->hid + 3 * hs_, I->lg_pos, d1[3], d2[3]);
  RET_IF(infgen_linear_multi(d1, 4, stream));
  RET_IF(infgen_linear_multi(d2, 4, stream));
  if (grid && rules) {
    // the allowed cells of this iteration (the static rules once per step), then the decision under them
    InsertCellMaskArgs ma = rules->mask;
    ma.S = S; ma.A_cap = r->A_cap; ma.T = r->T; ma.c = c; ma.G = G;
    ma.pos = r->pos; ma.head = r->head; ma.state = r->state; ma.n_agents = r->n_agents; ma.av_index = r->av_index;
    ma.shape = rules->box_shape; ma.grid_xy = r->grid_xy; ma.static_pass = it == 0 ? 1 : 2;
    ma.map_pos = r->map_pos; ma.n_map = r->n_map; ma.M_cap = r->M_cap;
    if (it == 0 && ma.count_log) { ma.count_log += t; ma.count_stride = rules->log_steps; }
    else ma.count_log = nullptr;
    RET_IF(insert_cell_mask_launch("infgen_insert_seed_rules", ma, stream));
    const InfgenSampling sp{I->insert_temperature, I->insert_top_p, nullptr};
    RET_IF(insert_decide_impl(r, t, I->force_enter, I->max_new, I->lg_state, I->lg_type, I->shape, I->lg_pos, I->occ, I->active, I->n_new,
                              I->inserted, I->new_row, I->new_shape, I->new_cell, I->insert_k, uniform, stream, true, 0.f, &sp, &rules_ctl));
  } else if (grid) {
    const InfgenSampling sp{I->insert_temperature, I->insert_top_p, nullptr};
    RET_IF(infgen_insert_decide_topk_ex(r, t, I->force_enter, I->max_new, I->lg_state, I->lg_type, I->shape, I->lg_pos, I->occ, I->active,
                                        I->n_new, I->inserted, I->new_row, I->new_shape, I->new_cell, I->insert_k, uniform, &sp, stream));
  } else
    RET_IF(insert_decide_impl(r, t, I->force_enter, I->max_new, I->lg_state, I->lg_type, I->shape, I->lg_pos, nullptr, I->active,
                              I->n_new, I->inserted, I->new_row, I->new_shape, I->new_cell, 1, nullptr, stream, false, I->r_seed));
  // hand-over to the host: did any scene insert, into which rows, which scenes go on?
  // (one copy when the caller laid the three arrays out back to back, as infgen_amd/engine.py does)
  if (I->new_row == I->inserted + S && I->active == I->inserted + 2 * S) {
    if (hipMemcpyAsync(I->host_dec, I->inserted, 3 * (size_t)S * sizeof(int), hipMemcpyDeviceToHost, hs) != hipSuccess)
      return fail("infgen_insert_seed", "hand-over copy failed");
  } else if (hipMemcpyAsync(I->host_dec, I->inserted, S * sizeof(int), hipMemcpyDeviceToHost, hs) != hipSuccess ||
             hipMemcpyAsync(I->host_dec + S, I->new_row, S * sizeof(int), hipMemcpyDeviceToHost, hs) != hipSuccess ||
             hipMemcpyAsync(I->host_dec + 2 * S, I->active, S * sizeof(int), hipMemcpyDeviceToHost, hs) != hipSuccess)
    return fail("infgen_insert_seed", "hand-over copy failed");
  return 0;
}

extern "C" int infgen_insert_seed(const InfgenRollout* r, const InfgenInsertion* I, int t, int it, int riders, const float* uniform,
                                  void* stream) {
  return insert_seed_impl(r, I, t, it, riders, uniform, stream, nullptr);
}

extern "C" int infgen_insert_seed_rules(const InfgenRollout* r, const InfgenInsertion* I, int t, int it, int riders, const float* uniform,
                                        int rules, const float* keepout, float clearance, float edge_clearance, float lane_dist,
                                        unsigned lane_types, const float* records, const int* n_records, int rec_cap,
                                        const long long* map_type, const float* zones, const int* n_zones, int Z, int copies,
                                        const int* type_allowed, const int* max_agents, float* box_shape, uint32_t* static_bits,
                                        uint32_t* allowed, int words, int* allowed_count, int* live, int* count_log, int log_steps,
                                        void* stream) {
  if ((rules & IM_KEEPOUT) && !keepout) return fail("infgen_insert_seed_rules", "insertion rules: ego_keepout needs its three floats");
  InsertSeedRules k{};
  InsertCellMaskArgs& a = k.mask;
  a.W = words; a.rules = rules;
  if (rules & IM_KEEPOUT) { a.ko_back = keepout[0]; a.ko_front = keepout[1]; a.ko_half = keepout[2]; }
  a.clearance = clearance; a.edge_clearance = edge_clearance; a.lane_dist = lane_dist; a.lane_types = lane_types;
  a.records = records; a.n_records = n_records; a.rec_cap = rec_cap; a.map_type = map_type;
  a.zones = zones; a.n_zones = n_zones; a.Z = Z; a.copies = copies;
  a.static_bits = static_bits; a.allowed = allowed; a.allowed_count = allowed_count; a.live = live; a.count_log = count_log;
  k.type_allowed = type_allowed; k.max_agents = max_agents; k.box_shape = box_shape; k.log_steps = log_steps;
  return insert_seed_impl(r, I, t, it, riders, uniform, stream, &k);
}

extern "C" int infgen_insert_heading(const InfgenRollout* r, const InfgenInsertion* I, int t, int h_ready, int riders, void* stream) {
  RET_IF(validate(r, "infgen_insert_heading"));
  if (!I) return fail("infgen_insert_heading", "null insertion block");
  if (I->no_head_token && !I->head_heading_theta) return fail("infgen_insert_heading", "no_head_token needs head_heading_theta");
  OptScope _opts(r);
  hipStream_t hs = (hipStream_t)stream;
  const int S = r->S, rows = r->S * r->A_cap, c = 1 + t;
  // categorical embedding / shape of the new rows (agent_decoder.py:1949-1950, :1993): shape_emb is an MLPEmbedding with K0 = 3
  // (three inputs, padded to 8 in the pack: the fp32 kernels at every attn_mode)
  RET_IF(mlp_embedding_fp32(I->new_shape, 3, S, 3, 8, I->shape_emb, I->t1, I->t2, I->shp, 128, stream));
  InsertCatArgs ca{S, r->A_cap, I->inserted, I->new_row, r->type, I->type_a_emb, I->shp, I->new_shape, const_cast<float*>(r->cat_agent),
                   I->shape_all, I->new_local};
  hipLaunchKernelGGL(k_insert_cat, dim3(ceil_div(S * 32, NT)), dim3(NT), 0, hs, ca);
  RET_IF(check_launch("k_insert_cat"));
  RET_IF(infgen_raw_feature_rows(r, c, I->new_row, I->inserted, S, stream));
  // heading stage: the new row attends agents / map tokens within 10 m through the motion layers 0..2
  RET_IF(infgen_point_edges(r, c, I->new_local, I->inserted, 1, 3, I->r_a2sa, 24, I->r_pl2sa, 128, &I->ea_h, &I->em_h, stream));
  RET_IF(infgen_fourier_embed(I->ea_h.raw, 3, I->ea_h.total, I->ea_h.cap, r->four_a, nullptr, 0, I->ea_h.rhat, 128, 1, stream));
  RET_IF(infgen_fourier_embed(I->em_h.raw, 3, I->em_h.total, I->em_h.cap, r->four_m, nullptr, 0, I->em_h.rhat, 128, 1, stream));
  if (!h_ready) {
    if (hipMemcpyAsync(I->Xc, r->X, (size_t)rows * D * sizeof(float), hipMemcpyDeviceToDevice, hs) != hipSuccess)
      return fail("infgen_insert_heading", "copy failed");
    for (int i = 0; i < 3; ++i) {
      RET_IF(infgen_attn_post_pre(I->Xc, rows, r->attn_m[i], I->zero_agg, I->zero_z, I->zero_sig, 0, r->attn_a[i], nullptr, nullptr,
                                  I->Kh[i], I->Vh[i], stream));
      RET_IF(edgeless(I->Xc, rows, r->attn_a[i], I, stream));
    }
  }
  const int R = riders ? 2 * S : S;
  RET_IF(gather_rows(r->X, I->new_row, nullptr, S, rows, I->XS, stream));
  if (riders) RET_IF(gather_rows(r->X, I->pend_row, I->pend_mask, S, rows, I->XS + (size_t)S * D, stream));
  RET_IF(infgen_attn_pre(I->XS, R, r->attn_m[0], 0, I->QS, I->US, nullptr, nullptr, stream));
  for (int i = 0; i < 3; ++i) {
    RET_IF(infgen_edge_attn(S, I->QS, I->US, r->mapK[i], r->mapV[i], I->em_h.off, I->em_h.cnt, I->em_h.src, I->em_h.rhat, I->AGGS, I->ZS,
                            I->SIGS, stream));
    RET_IF(infgen_attn_post_pre(I->XS, R, r->attn_m[i], I->AGGS, I->ZS, I->SIGS, 1, r->attn_a[i], I->QS, I->US, riders ? I->KN : nullptr,
                                riders ? I->VN : nullptr, stream));
    if (riders) {
      RET_IF(scatter_rows2(I->KN + (size_t)S * D, I->VN + (size_t)S * D, I->pend_row, I->pend_mask, S, I->Kh[i], I->Vh[i], stream));
    }
    RET_IF(infgen_edge_attn(S, I->QS, I->US, I->Kh[i], I->Vh[i], I->ea_h.off, I->ea_h.cnt, I->ea_h.src, I->ea_h.rhat, I->AGGS, I->ZS,
                            I->SIGS, stream));
    if (i < 2) RET_IF(infgen_attn_post_pre(I->XS, R, r->attn_a[i], I->AGGS, I->ZS, I->SIGS, 1, r->attn_m[i + 1], I->QS, I->US, nullptr,
                                           nullptr, stream));
    else RET_IF(infgen_attn_post(I->XS, R, r->attn_a[i], I->AGGS, I->ZS, I->SIGS, 1, stream));
  }
  // heading head (token logits, or the theta regression for use_head_token = False) and, with the grid, the xy-offset head
  InfgenLinearDesc d1[2], d2[2];
  const size_t hs_ = (size_t)S * 128;
  const bool head_tok = !I->no_head_token, offset = !I->no_grid_token;
  if (head_tok) mlp_layer_descs(I->XS, S, I->head_heading, I->n_heading, I->hid + 4 * hs_, I->lg_heading, d1[0], d2[0]);
  else mlp_layer_descs(I->XS, S, I->head_heading_theta, 1, I->hid + 4 * hs_, I->lg_heading, d1[0], d2[0]);
  if (offset) mlp_layer_descs(I->XS, S, I->head_offset, 2, I->hid + 5 * hs_, I->offset, d1[1], d2[1]);
  RET_IF(infgen_linear_multi(d1, offset ? 2 : 1, stream));
  RET_IF(infgen_linear_multi(d2, offset ? 2 : 1, stream));
  RET_IF(insert_finalize_impl(r, c, I->angle_interval, I->inserted, I->new_row, I->lg_heading, head_tok ? I->n_heading : 1, I->offset,
                              I->hv_ovr, stream, head_tok, offset));
  RET_IF(infgen_raw_feature_rows(r, c, I->new_row, I->inserted, S, stream));
  // the rows of this iteration ride along in the next seed chain / heading stage
  hipLaunchKernelGGL(k_note_riders, dim3(ceil_div(S, NT)), dim3(NT), 0, hs, I->new_row, I->inserted, S, I->prev_row, I->prev_mask,
                     I->pend_row, I->pend_mask);
  return check_launch("k_note_riders");
}

// ---------------------------------------------------------------------------------- ragged batch ingest / row pack
extern "C" int infgen_ingest_batch(const InfgenBatchIngest* a, void* stream) {
  if (!a) return fail("infgen_ingest_batch", "null argument block");
  if (a->S <= 0) return 0;
  if (a->copies < 1 || a->S % a->copies) return fail("infgen_ingest_batch", "S must be a positive multiple of copies");
  if (a->A_cap < 1 || a->A_cap > MAX_SCENE_AGENTS) return fail("infgen_ingest_batch", "A_cap must be in 1..INFGEN_Q_MAX_AGENTS");
  if (a->M_cap < 1) return fail("infgen_ingest_batch", "M_cap must be positive");
  if (a->hc < 1 || a->T0 < a->hc || a->T0 > a->T) return fail("infgen_ingest_batch", "need 1 <= hc <= T0 <= T");
  if (a->H < 1 || a->P <= a->H || a->pos_dim < 2 || a->pt_pos_dim < 2 || a->motion_cols < 0)
    return fail("infgen_ingest_batch", "bad step geometry (need P > H >= 1, pos_dim >= 2, pt_pos_dim >= 2)");
  const void* need[] = {a->agent_ptr, a->pt_ptr, a->av_index, a->src_graph, a->state_idx, a->token_idx, a->grid_token_idx,
                        a->token_pos, a->token_heading, a->raw_valid, a->valid_mask, a->shape, a->position, a->heading, a->type,
                        a->id, a->pt_position, a->pt_orientation, a->pt_token_idx, a->pt_type, a->pt_pl_type, a->pt_polygon,
                        a->light_type, a->pos, a->head, a->state, a->token, a->gridtok, a->tmask, a->imask, a->catflag, a->atype,
                        a->bos, a->shape10, a->n_agents, a->av, a->n_map, a->map_pos, a->map_orient, a->map_tok, a->map_type,
                        a->map_pl, a->map_light, a->htok, a->hst, a->p0, a->h0, a->shp, a->gt, a->val, a->ids, a->counts};
  for (const void* p : need)
    if (!p) return fail("infgen_ingest_batch", "null input or destination pointer");
  if (a->replay_row && !(a->replay_in && a->teacher_token && a->teacher_state))
    return fail("infgen_ingest_batch", "replay_row needs replay_in, teacher_token and teacher_state");
  if ((a->teacher_pos != nullptr) != (a->teacher_head != nullptr))
    return fail("infgen_ingest_batch", "teacher_pos and teacher_head come together");
  hipLaunchKernelGGL(k_ingest_batch, dim3(a->S, 3), dim3(256), 0, (hipStream_t)stream, *a);
  return check_launch("infgen_ingest_batch");
}

extern "C" int infgen_pack_rows(int n_keys, const void* const* src, const long long* src_stride, const int* row_bytes,
                                const int* const* counts, const int* count_stride, void* const* dst, int n_scenes, int scene0,
                                int scene_step, void* stream) {
  if (n_keys <= 0 || n_scenes <= 0) return 0;
  if (n_keys > PACK_MAX_KEYS) return fail("infgen_pack_rows", "at most 32 keys per call");
  if (!src || !src_stride || !row_bytes || !counts || !count_stride || !dst || scene0 < 0 || scene_step < 1)
    return fail("infgen_pack_rows", "null key table or bad scene range");
  PackRowsArgs a{};
  for (int k = 0; k < n_keys; ++k) {
    if (!src[k] || !dst[k] || !counts[k] || row_bytes[k] < 0 || count_stride[k] < 1)
      return fail("infgen_pack_rows", "null pointer or bad row size / count stride in the key table");
    a.src[k] = static_cast<const char*>(src[k]); a.dst[k] = static_cast<char*>(dst[k]);
    a.src_stride[k] = src_stride[k]; a.row_bytes[k] = row_bytes[k];
    a.counts[k] = counts[k]; a.count_stride[k] = count_stride[k];
  }
  a.n_keys = n_keys; a.n_scenes = n_scenes; a.scene0 = scene0; a.scene_step = scene_step;
  hipLaunchKernelGGL(k_pack_rows, dim3(n_scenes, n_keys), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("infgen_pack_rows");
}
