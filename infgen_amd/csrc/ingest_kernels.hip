// Ragged batch ingest and ragged row pack (include/infgen_hip.h: infgen_ingest_batch, infgen_pack_rows).
//   k_ingest_batch   grid (S, 3), 256 threads: y = 0 the [S][T][A_cap] / [S][A_cap] rollout arrays + per-scene counts,
//                    y = 1 the epilogue inputs, y = 2 the map side (first copy of every graph only).  Every part first
//                    compacts the graph's rows kept by the filter of agent_decoder.py:1609 (state valid at column hc - 1):
//                    a stable per-scene compaction, ballot + mbcnt rank inside a wave, wave totals through LDS.
//   k_pack_rows      grid (scenes, keys): the exclusive scan of the row counts up to the scene, then one contiguous copy.
// Plain vector stores only; deterministic (no atomics).
#include "kernels.h"
#include "../../include/infgen_hip.h"

namespace ig {

constexpr int ING_NT = 256;
constexpr int ING_WAVES = ING_NT / 64;
constexpr int ING_MAX_ROWS = MAX_SCENE_AGENTS;          // INFGEN_Q_MAX_AGENTS: the LDS tables below hold one graph's rows
static_assert(ING_MAX_ROWS == MAX_SCENE_AGENTS, "the compaction tables must hold every row a scene can have");
constexpr int ING_INVALID = 0, ING_ENTER = 2, ING_EXIT = 3;
constexpr float ING_INVALID_SHAPE = 0.1f;

struct IngestLds {
  int src_row[ING_MAX_ROWS];     // kept row a -> row inside the graph
  int bos[ING_MAX_ROWS], eos[ING_MAX_ROWS];
  int wtot[ING_WAVES];
  int n, av;                     // kept rows, ego row after filtering
  long long red[ING_NT / 64];
};

// stable compaction of the rows of graph g kept by the filter; fills L.src_row / L.n / L.av
__device__ void ingest_compact(const InfgenBatchIngest& a, long long base, int A_raw, long long av_raw, IngestLds& L) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { L.n = 0; L.av = 0; }
  int running = 0;
  for (int c0 = 0; c0 < A_raw; c0 += ING_NT) {
    const int r = c0 + tid;
    const bool keep = r < A_raw && a.state_idx[(base + r) * a.T0 + (a.hc - 1)] != ING_INVALID;
    const unsigned long long m = __ballot(keep);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    if (lane == 0) L.wtot[wave] = __popcll(m);
    __syncthreads();
    int pre = running;
    for (int w = 0; w < wave; ++w) pre += L.wtot[w];
    if (keep && pre + rank < ING_MAX_ROWS) L.src_row[pre + rank] = r;     // (rows past the tables: see the clamp below)
    if (r == av_raw) L.av = pre + rank;          // kept rows before the ego = its row after filtering (agent_decoder.py:1649)
    for (int w = 0; w < ING_WAVES; ++w) running += L.wtot[w];
    __syncthreads();
  }
  // a caller that skipped the offsets check (more kept rows than A_cap / the tables): the scene keeps its first rows only - the
  // kernel never reads or writes past its tables or the scene's A_cap rows
  if (tid == 0) L.n = min(running, min(a.A_cap, ING_MAX_ROWS));
  __syncthreads();
}

// valid (raw_agent_valid_mask padded True, True from column hc on, AND the eval mask at step H - 1) of kept row `row`, column t
__device__ inline bool ingest_valid(const InfgenBatchIngest& a, long long row, int t) {
  const bool v = (t < a.hc && t < a.T0) ? a.raw_valid[row * a.T0 + t] != 0 : true;
  return v && a.valid_mask[row * a.P + (a.H - 1)] != 0;
}

__global__ __launch_bounds__(ING_NT) void k_ingest_batch(InfgenBatchIngest a) {
  __shared__ IngestLds L;
  const int s = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
  if (part == 2 && s % a.copies) return;                        // map side: once per graph
  const int g = a.src_graph[s];
  const long long base = a.agent_ptr[g];
  const int A_raw = (int)(a.agent_ptr[g + 1] - base);
  const long long av_raw = a.av_index[g] - base;
  const int T = a.T, A_cap = a.A_cap, hc = a.hc;

  if (part == 2) {
    const int ms = s / a.copies;
    const long long mb = a.pt_ptr[g];
    const int M = (int)(a.pt_ptr[g + 1] - mb);
    if (tid == 0) a.n_map[ms] = M < a.M_cap ? M : a.M_cap;
    for (int j = tid; j < a.M_cap; j += ING_NT) {
      const size_t o = (size_t)ms * a.M_cap + j;
      float x = 0.f, y = 0.f, th = 0.f;
      long long tok = 0, ty = 0, pl = 0, li = 0;
      if (j < M) {
        const long long p = mb + j;
        x = a.pt_position[p * a.pt_pos_dim]; y = a.pt_position[p * a.pt_pos_dim + 1];
        th = a.pt_orientation[p];
        tok = a.pt_token_idx[p]; ty = a.pt_type[p]; pl = a.pt_pl_type[p];
        const long long e = a.pt_polygon[p];
        li = (e >= 0 && e < a.n_polygons) ? (long long)a.light_type[e] : 0;
      }
      a.map_pos[2 * o] = x; a.map_pos[2 * o + 1] = y; a.map_orient[o] = th;
      a.map_tok[o] = tok; a.map_type[o] = ty; a.map_pl[o] = pl; a.map_light[o] = li;
    }
    return;
  }

  ingest_compact(a, base, A_raw, av_raw, L);
  const int n = L.n, avl = L.av;

  if (part == 1) {
    // epilogue inputs (RolloutEngine._epi): [S][A_cap][...] with the row-major inner dims fastest
    const size_t sa = (size_t)s * A_cap;
    for (int i = tid; i < A_cap * hc; i += ING_NT) {
      const int r = i / hc, t = i % hc;
      long long tk = 0, st = 0;
      if (r < n) { const long long row = base + L.src_row[r]; tk = a.token_idx[row * a.T0 + t]; st = a.state_idx[row * a.T0 + t]; }
      a.htok[sa * hc + i] = tk; a.hst[sa * hc + i] = st;
    }
    // fresh ids of the rows past the kept ones: max kept id + 1 + k (-1 + 1 + k without kept rows)
    constexpr long long NONE = (long long)(-0x7fffffffffffffffLL - 1);
    long long mx = NONE;
    for (int r = tid; r < n; r += ING_NT) {
      const long long v = a.id[base + L.src_row[r]];
      mx = v > mx ? v : mx;
    }
    for (int off = 32; off > 0; off >>= 1) {        // (a lane past the wave's end reads its own value)
      const long long o2 = __shfl_down(mx, off);
      mx = o2 > mx ? o2 : mx;
    }
    if ((tid & 63) == 0) L.red[tid >> 6] = mx;
    __syncthreads();
    long long idmax = NONE;
    for (int w = 0; w < ING_WAVES; ++w) idmax = L.red[w] > idmax ? L.red[w] : idmax;
    if (n == 0) idmax = -1;
    for (int r = tid; r < A_cap; r += ING_NT) {
      const size_t o = sa + r;
      if (r < n) {
        const long long row = base + L.src_row[r];
        a.ids[o] = a.id[row];
        const float* ps = a.position + (size_t)row * a.P * a.pos_dim;
        a.p0[2 * o] = ps[0]; a.p0[2 * o + 1] = ps[1];
        a.h0[o] = a.heading[(size_t)row * a.P];
        const float* sh = a.shape + ((size_t)row * a.P + (hc - 1)) * 3;
        a.shp[3 * o] = sh[0]; a.shp[3 * o + 1] = sh[1]; a.shp[3 * o + 2] = sh[2];
      } else {
        a.ids[o] = idmax + 1 + (r - n);
        a.p0[2 * o] = 0.f; a.p0[2 * o + 1] = 0.f; a.h0[o] = 0.f;
        a.shp[3 * o] = 0.f; a.shp[3 * o + 1] = 0.f; a.shp[3 * o + 2] = 0.f;
      }
    }
    const int Rg = a.P - a.H;
    for (int i = tid; i < A_cap * Rg * 2; i += ING_NT) {
      const int r = i / (Rg * 2), j = (i / 2) % Rg, c = i & 1;
      float v = 0.f;
      if (r < n) v = a.position[((size_t)(base + L.src_row[r]) * a.P + a.H + j) * a.pos_dim + c];
      a.gt[sa * Rg * 2 + i] = v;
    }
    for (int i = tid; i < A_cap * T; i += ING_NT) {
      const int r = i / T, t = i % T;
      a.val[sa * T + i] = r < n ? (unsigned char)ingest_valid(a, base + L.src_row[r], t) : (unsigned char)0;
    }
    return;
  }

  // part 0: bos / eos of every kept row (the padded state is INVALID from column hc on)
  for (int r = tid; r < n; r += ING_NT) {
    const long long row = base + L.src_row[r];
    int b = 0, e = T - 1;
    bool fb = false, fe = false;
    for (int t = 0; t < hc && t < a.T0; ++t) {
      const long long st = a.state_idx[row * a.T0 + t];
      if (!fb && st == ING_ENTER) { b = t; fb = true; }
      if (!fe && st == ING_EXIT) { e = t; fe = true; }
    }
    L.bos[r] = b; L.eos[r] = e;
  }
  __syncthreads();
  // [S][T][A_cap]: the row index fastest (coalesced stores)
  for (int i = tid; i < T * A_cap; i += ING_NT) {
    const int t = i / A_cap, r = i % A_cap;
    const size_t o = (size_t)s * T * A_cap + i;
    float x = 0.f, y = 0.f, hd = 0.f;
    int st = 0, tk = -1, gr = -1;
    unsigned char tm = 0, im = 0, cf = 0;
    if (r < n) {
      const long long row = base + L.src_row[r];
      const bool hist = t < hc && t < a.T0;
      st = hist ? (int)a.state_idx[row * a.T0 + t] : ING_INVALID;
      if (hist) {
        x = a.token_pos[(row * a.T0 + t) * 2]; y = a.token_pos[(row * a.T0 + t) * 2 + 1];
        hd = a.token_heading[row * a.T0 + t];
        tk = (int)a.token_idx[row * a.T0 + t]; gr = (int)a.grid_token_idx[row * a.T0 + t];
      }
      const bool motion = t > L.bos[r] && t <= L.eos[r] && t < a.motion_cols;
      const bool v = ingest_valid(a, row, t);
      tm = (t >= hc || !motion || v) ? 1 : 0;
      const bool nonmotion = !motion && t < a.motion_cols;
      im = (t >= hc || !nonmotion || st == ING_ENTER || r == avl) ? 1 : 0;
      cf = st != ING_INVALID ? 1 : 0;
    }
    a.pos[2 * o] = x; a.pos[2 * o + 1] = y; a.head[o] = hd;
    a.state[o] = st; a.token[o] = tk; a.gridtok[o] = gr;
    a.tmask[o] = tm; a.imask[o] = im; a.catflag[o] = cf;
    if (a.replay_row) {
      // log replay: the future columns zeroed above are kept, for the flagged rows, as the plan the rollout forces
      int ptk = -1, pst = ING_INVALID;
      float px = 0.f, py = 0.f, ph = 0.f;
      if (r < n && t >= hc && t < a.T0) {
        const long long row = base + L.src_row[r];
        if (a.replay_in[row]) {
          const long long i = row * a.T0 + t;
          ptk = (int)(a.plan_token ? a.plan_token : a.token_idx)[i];
          pst = (int)(a.plan_state ? a.plan_state : a.state_idx)[i];
          if (a.teacher_pos) {
            const float* pp = a.plan_pos ? a.plan_pos : a.token_pos;
            px = pp[2 * i]; py = pp[2 * i + 1]; ph = (a.plan_head ? a.plan_head : a.token_heading)[i];
          }
        }
      }
      a.teacher_token[o] = ptk; a.teacher_state[o] = pst;
      if (a.teacher_pos) { a.teacher_pos[2 * o] = px; a.teacher_pos[2 * o + 1] = py; a.teacher_head[o] = ph; }
    }
  }
  for (int r = tid; r < A_cap; r += ING_NT) {
    const size_t o = (size_t)s * A_cap + r;
    int ty = 0, b = 0;
    float s0 = ING_INVALID_SHAPE, s1 = ING_INVALID_SHAPE, s2 = ING_INVALID_SHAPE;
    if (r < n) {
      const long long row = base + L.src_row[r];
      ty = a.type[row]; b = L.bos[r];
      const float* sh = a.shape + ((size_t)row * a.P + (a.H - 1)) * 3;
      s0 = sh[0]; s1 = sh[1]; s2 = sh[2];
    }
    a.atype[o] = ty; a.bos[o] = b;
    if (a.replay_row) a.replay_row[o] = (r < n && a.replay_in[base + L.src_row[r]]) ? 1 : 0;
    a.shape10[3 * o] = s0; a.shape10[3 * o + 1] = s1; a.shape10[3 * o + 2] = s2;
  }
  if (tid == 0) {
    a.n_agents[s] = n; a.av[s] = avl;
    a.counts[3 * s] = n; a.counts[3 * s + 1] = avl; a.counts[3 * s + 2] = (int)av_raw - avl;
  }
}

__global__ __launch_bounds__(ING_NT) void k_pack_rows(PackRowsArgs a) {
  __shared__ long long part[ING_WAVES];
  const int i = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const int* cnt = a.counts[k];
  const int cs = a.count_stride[k];
  // exclusive scan of the row counts of the scenes before this one
  long long acc = 0;
  for (int j = tid; j < i; j += ING_NT) acc += cnt[(size_t)(a.scene0 + j * a.scene_step) * cs];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  long long off_rows = 0;
  for (int w = 0; w < ING_WAVES; ++w) off_rows += part[w];
  const size_t s = (size_t)(a.scene0 + i * a.scene_step);
  const long long rows = cnt[s * cs];
  const long long nb = rows * a.row_bytes[k];
  const char* src = a.src[k] + s * a.src_stride[k];
  char* dst = a.dst[k] + off_rows * a.row_bytes[k];
  const unsigned long long al = (unsigned long long)(size_t)src | (unsigned long long)(size_t)dst | (unsigned long long)nb;
  if ((al & 15) == 0) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (long long j = tid; j < nb / 16; j += ING_NT) d4[j] = s4[j];
  } else if ((al & 3) == 0) {
    const unsigned* s1 = reinterpret_cast<const unsigned*>(src);
    unsigned* d1 = reinterpret_cast<unsigned*>(dst);
    for (long long j = tid; j < nb / 4; j += ING_NT) d1[j] = s1[j];
  } else {
    for (long long j = tid; j < nb; j += ING_NT) dst[j] = src[j];
  }
}

}  // namespace ig
