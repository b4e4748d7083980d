// Branching rollouts (include/infgen_hip.h, "branching"): scene slot s becomes a clone of slot parent[s].
//
// k_branch_scenes      one launch over (chunk, scene).  blockIdx.y = the destination scene s; its workgroups read parent[s] and leave
//                      at once when the entry is the identity or breaks the contract (out of range, another copy group, a source that
//                      is itself moved) - the launch reads nothing outside the layout for any content of `parent`.  blockIdx.x names
//                      a BR_CHUNK-byte piece of one block of one segment (kernels.h: BranchSeg); a lane moves BR_VEC 16-byte words
//                      held in registers, all four loads in flight before the first store (26 VGPRs, no LDS, no scratch).  Sources are fixed points, so no slot is read and written in one
//                      launch: the gather runs in place without a staging copy.  A segment whose base, block size or stride is no
//                      multiple of 16 is moved byte by byte (the library's own layouts never are: A_cap % 32 == 0).
// k_snapshot_scenes    (include/infgen_hip.h, "snapshots") the same segments and the same chunk scheme between the context and
//                      a caller's buffer of entries: <false> saves slot slots[e] into entry e and writes its head, <true> puts entry
//                      index[s] back into slot s where the head allows it.  A workgroup whose entry is skipped returns before it
//                      reads anything else.  The entry side is always 16-byte aligned; an unaligned context side goes byte by byte
//                      (save 62 VGPRs - the byte-wise gather -, restore 30, no LDS, no scratch).
// k_resample_parents   one workgroup per copy group: arbitrary ancestor indices -> a parent vector whose sources are fixed points.
//                      Counts in LDS, one exclusive scan of (free slots, surplus copies) packed into a word, then every ancestor
//                      writes itself into the free slots its surplus owns.
// Bandwidth-bound copies: no LDS in the gather, plain vector loads and stores.
#include "kernels.h"

namespace ig {

// parent[s] where it is a valid source for slot s, else s
__device__ __forceinline__ int branch_source(const BranchArgs& a, int s, bool* bad) {
  const int p = a.parent[s];
  *bad = false;
  if (p == s) return s;
  bool ok = p >= 0 && p < a.S;
  if (ok) ok = a.map_scene != nullptr && a.map_scene[p] == a.map_scene[s] && a.parent[p] == p;
  *bad = !ok;
  return ok ? p : s;
}

__global__ __launch_bounds__(BR_NT) void k_branch_scenes(BranchArgs a) {
  const int s = blockIdx.y;
  bool bad;
  const int p = branch_source(a, s, &bad);
  if (blockIdx.x == 0 && threadIdx.x == 0 && bad && a.n_bad) atomicAdd(a.n_bad, 1);
  if (p == s) return;
  // the segment of this chunk (chunk0 ascends; a short table in the kernel argument)
  int k = 0;
  const int x = blockIdx.x;
  while (k + 1 < a.n_seg && x >= a.seg[k + 1].chunk0) ++k;
  const BranchSeg& g = a.seg[k];
  const int local = x - g.chunk0;
  const int o = local / g.per_block;
  if (o >= g.outer) return;
  const long long off0 = (long long)(local - o * g.per_block) * BR_CHUNK;
  char* blk = g.base + (long long)o * g.outer_stride;
  const char* src = blk + (long long)p * g.bytes;
  char* dst = blk + (long long)s * g.bytes;
  if (g.wide) {
    // the four words stay in registers: every load is unconditional - a lane past the block's end reads the block's first word, which
    // is inside the layout, and stores nothing - so the compiler keeps no conditionally written array (it would move one to LDS)
    const long long o0 = off0 + (long long)threadIdx.x * 16, o1 = o0 + BR_NT * 16, o2 = o1 + BR_NT * 16, o3 = o2 + BR_NT * 16;
    static_assert(BR_VEC == 4, "four named words");
    const uint4 v0 = *reinterpret_cast<const uint4*>(src + (o0 < g.bytes ? o0 : 0));
    const uint4 v1 = *reinterpret_cast<const uint4*>(src + (o1 < g.bytes ? o1 : 0));
    const uint4 v2 = *reinterpret_cast<const uint4*>(src + (o2 < g.bytes ? o2 : 0));
    const uint4 v3 = *reinterpret_cast<const uint4*>(src + (o3 < g.bytes ? o3 : 0));
    if (o0 < g.bytes) *reinterpret_cast<uint4*>(dst + o0) = v0;
    if (o1 < g.bytes) *reinterpret_cast<uint4*>(dst + o1) = v1;
    if (o2 < g.bytes) *reinterpret_cast<uint4*>(dst + o2) = v2;
    if (o3 < g.bytes) *reinterpret_cast<uint4*>(dst + o3) = v3;
  } else {
    const long long end = off0 + BR_CHUNK < g.bytes ? off0 + BR_CHUNK : g.bytes;
    for (long long off = off0 + threadIdx.x; off < end; off += BR_NT) dst[off] = src[off];
  }
}

// ---- snapshots: the same segments between the context and a buffer of entries (kernels.h: SnapArgs)
// 16 bytes of a context-side block that is not 16-byte aligned, byte by byte; bytes past the block's end read as 0 / are not written
__device__ __forceinline__ uint4 snap_load_bytes(const char* p, long long off, long long bytes) {
  unsigned w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long o = off + i * 4 + j;
      const unsigned b = static_cast<unsigned char>(p[o < bytes ? o : 0]);
      v |= (o < bytes ? b : 0u) << (8 * j);
    }
    w[i] = v;
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void snap_store_bytes(char* p, long long off, long long bytes, uint4 v) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long o = off + i * 4 + j;
      if (o < bytes) p[o] = static_cast<char>(w[i] >> (8 * j));
    }
}

template <bool RESTORE> __global__ __launch_bounds__(BR_NT) void k_snapshot_scenes(SnapArgs a) {
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  int slot, e;
  if (!RESTORE) {
    e = blockIdx.y;
    slot = a.sel[e];
    const bool ok = slot >= 0 && slot < a.S;
    if (first) {
      int* h = a.head + 4 * (long long)e;
      h[0] = slot; h[1] = !ok ? -1 : a.map_scene ? a.map_scene[slot] : slot; h[2] = a.t; h[3] = ok ? 1 : 0;
      if (!ok && a.n_bad) atomicAdd(a.n_bad, 1);
    }
    if (!ok) return;
  } else {
    slot = blockIdx.y;
    e = a.sel[slot];
    if (e == -1) return;
    bool ok = e >= 0 && e < a.n;
    if (ok) {
      const int* h = a.head + 4 * (long long)e;
      ok = h[3] != 0 && h[2] == a.t && h[1] == (a.map_scene ? a.map_scene[slot] : slot);
    }
    if (!ok) {
      if (first && a.n_bad) atomicAdd(a.n_bad, 1);
      return;
    }
  }
  int k = 0;
  const int x = blockIdx.x;
  while (k + 1 < a.n_seg && x >= a.seg[k + 1].chunk0) ++k;
  const BranchSeg& g = a.seg[k];
  const int local = x - g.chunk0;
  const int o = local / g.per_block;
  if (o >= g.outer) return;
  const long long off0 = (long long)(local - o * g.per_block) * BR_CHUNK;
  const long long padded = (g.bytes + 15) & ~15LL;          // a block's bytes in the entry
  char* ctx = g.base + (long long)o * g.outer_stride + (long long)slot * g.bytes;
  char* ent = a.snap + (long long)e * a.stride + a.entry_off[k] + (long long)o * padded;
  // as in k_branch_scenes: four words per lane, every load unconditional (a lane past the end reads the block's first word, inside
  // both layouts) and issued before the first store
  const long long o0 = off0 + (long long)threadIdx.x * 16, o1 = o0 + BR_NT * 16, o2 = o1 + BR_NT * 16, o3 = o2 + BR_NT * 16;
  static_assert(BR_VEC == 4, "four named words");
  const bool in0 = o0 < padded, in1 = o1 < padded, in2 = o2 < padded, in3 = o3 < padded;
  const long long l0 = in0 ? o0 : 0, l1 = in1 ? o1 : 0, l2 = in2 ? o2 : 0, l3 = in3 ? o3 : 0;
  uint4 v0, v1, v2, v3;
  if (RESTORE || g.wide) {
    const char* src = RESTORE ? ent : ctx;
    v0 = *reinterpret_cast<const uint4*>(src + l0); v1 = *reinterpret_cast<const uint4*>(src + l1);
    v2 = *reinterpret_cast<const uint4*>(src + l2); v3 = *reinterpret_cast<const uint4*>(src + l3);
  } else {
    v0 = snap_load_bytes(ctx, l0, g.bytes); v1 = snap_load_bytes(ctx, l1, g.bytes);
    v2 = snap_load_bytes(ctx, l2, g.bytes); v3 = snap_load_bytes(ctx, l3, g.bytes);
  }
  if (!RESTORE || g.wide) {
    char* dst = RESTORE ? ctx : ent;
    if (in0) *reinterpret_cast<uint4*>(dst + o0) = v0;
    if (in1) *reinterpret_cast<uint4*>(dst + o1) = v1;
    if (in2) *reinterpret_cast<uint4*>(dst + o2) = v2;
    if (in3) *reinterpret_cast<uint4*>(dst + o3) = v3;
  } else {
    if (in0) snap_store_bytes(ctx, o0, g.bytes, v0);
    if (in1) snap_store_bytes(ctx, o1, g.bytes, v1);
    if (in2) snap_store_bytes(ctx, o2, g.bytes, v2);
    if (in3) snap_store_bytes(ctx, o3, g.bytes, v3);
  }
}
template __global__ void k_snapshot_scenes<false>(SnapArgs a);
template __global__ void k_snapshot_scenes<true>(SnapArgs a);

// ancestor[i] (a global slot index; outside slot i's group: i itself) for the copies of group blockIdx.x -> parent:
//   a slot some entry names keeps itself; the slots nobody names, in ascending order, receive the surplus - ancestor j's count[j] - 1
//   extra copies, in ascending j.  The multiset of ancestors is preserved and every source is a fixed point.
__global__ __launch_bounds__(RS_NT) void k_resample_parents(ResampleArgs a) {
  __shared__ int count[RS_NT * RS_ITEMS];      // per slot of the group: times named
  __shared__ int freelist[RS_NT * RS_ITEMS];   // the unnamed slots in ascending order
  __shared__ int scan[RS_NT];
  const int n = a.copies, g0 = blockIdx.x * n, tid = threadIdx.x;
  for (int j = tid; j < RS_NT * RS_ITEMS; j += RS_NT) count[j] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += RS_NT) {
    int j = a.ancestor[g0 + i] - g0;
    if (j < 0 || j >= n) j = i;
    atomicAdd(&count[j], 1);
  }
  __syncthreads();
  // exclusive scan over the slots of (free ? 1 : 0) << 16 | surplus, both sums <= 1024; a thread owns RS_ITEMS consecutive slots
  int own[RS_ITEMS], sum = 0;
#pragma unroll
  for (int k = 0; k < RS_ITEMS; ++k) {
    const int j = tid * RS_ITEMS + k, c = j < n ? count[j] : 1;
    own[k] = c == 0 ? 1 << 16 : c - 1;
    sum += own[k];
  }
  scan[tid] = sum;
  __syncthreads();
  for (int d = 1; d < RS_NT; d <<= 1) {
    const int v = tid >= d ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  int run = scan[tid] - sum;
  int first[RS_ITEMS];
#pragma unroll
  for (int k = 0; k < RS_ITEMS; ++k) {
    const int j = tid * RS_ITEMS + k;
    first[k] = run & 0xffff;                   // rank of this slot's first surplus copy among all surplus copies
    if (j < n && count[j] == 0) freelist[run >> 16] = j;
    run += own[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < RS_ITEMS; ++k) {
    const int j = tid * RS_ITEMS + k;
    if (j >= n || count[j] == 0) continue;
    a.parent[g0 + j] = g0 + j;
    for (int e = 0; e < count[j] - 1; ++e) a.parent[g0 + freelist[first[k] + e]] = g0 + j;
  }
}

}  // namespace ig
