// Branching rollouts (include/infgen_hip.h, "branching"): scene slot s becomes a clone of slot parent[s].
//
// k_branch_scenes      one launch over (chunk, scene).  blockIdx.y = the destination scene s; its workgroups read parent[s] and leave
//                      at once when the entry is the identity or breaks the contract (out of range, another copy group, a source that
//                      is itself moved) - the launch reads nothing outside the layout for any content of `parent`.  blockIdx.x names
//                      a BR_CHUNK-byte piece of one block of one segment (kernels.h: BranchSeg); a lane moves BR_VEC 16-byte words
//                      held in registers, all four loads in flight before the first store (26 VGPRs, no LDS, no scratch).  Sources are fixed points, so no slot is read and written in one
//                      launch: the gather runs in place without a staging copy.  A segment whose base, block size or stride is no
//                      multiple of 16 is moved byte by byte (the library's own layouts never are: A_cap % 32 == 0).
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
