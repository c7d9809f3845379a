// The selection key and what every selector does with it (drx_topk.hip, drx_recommend.hip, drx_knn.hip): ONE definition of the key, of
// the ordering network over a workgroup's keys, of the merge of a row's split lists and of the plan / layout of those lists.
//
// key = monotone score bits << 32 | index: keys compare as (score, index) pairs do, so "descending key" is heapq.nlargest over
// (score, iid) — descending score, ties to the LARGER index — and keys are unique: "the n best" and "how many are ahead" have one
// answer, which makes a result a function of the inputs alone.
#pragma once
#include <hip/hip_runtime.h>
#include "drx_common.hpp"

namespace drx {

typedef unsigned long long u64;

// The key 0 means "empty slot" everywhere (a masked candidate, a list's free tail, the padding of the network).  No finite float orders
// to 0 bits (that is -NaN with every payload bit set), so a real key is never 0 whatever the sign of its score.  -0.0 orders as +0.0
// (they compare equal in Python), so key_score gives +0.0 back for both.
__device__ __forceinline__ uint32_t ordered_bits(float f) {
  if (f == 0.0f) f = 0.0f;
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_score(u64 key) {
  const uint32_t o = (uint32_t)(key >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}
__device__ __forceinline__ u64 make_key(float score, unsigned index) { return ((u64)ordered_bits(score) << 32) | index; }

// The workgroup's npad keys (a power of two, in LDS) into descending order: a bitonic network, every thread of the workgroup calls it.
// Begins and ends on a barrier: the keys may have been written just before, and may be read just after, by any thread.
__device__ __forceinline__ void order_keys_desc(u64 *keys, int npad) {
  for (int size = 2; size <= npad; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < (npad >> 1); t += kBlock) {
        const int a = 2 * t - (t & (stride - 1));
        const int b = a + stride;
        const u64 ka = keys[a], kb = keys[b];
        const bool desc = (a & size) == 0;
        if (desc ? (ka < kb) : (ka > kb)) { keys[a] = kb; keys[b] = ka; }
      }
    }
  }
  __syncthreads();
}

// ---- lists split over a launch, merged per row ------------------------------------------------------------------------------------------
// A selector whose launch is (row tiles of kListRows, splits of the row's candidates) keeps per tile, split and row TWO lists (one per
// half-wave lane that owns the row) of up to cap keys, the best first after the lane's last compaction, and their lengths:
//   lists [tiles][splits][kListRows][2][cap]      counts [tiles][splits][kListRows][2]
constexpr int kListRows = 128;            // rows of a tile (a workgroup): 32 per wave
constexpr int kListMaxMerge = 16384;      // keys the merge orders in LDS (128 KiB of the CU's 160)

// `units` of work per row (item blocks, row tiles J) dealt to the splits of a launch that aims at `target` workgroups (or at `force`
// splits per tile, if positive), `most` splits at the most: the splits aimed at (room >= count), the units per split, the splits
struct Splits { int room, per, count; };
inline Splits plan_splits(int tiles, int units, int target, int force, int most) {
  int64_t want = force > 0 ? force : (target + tiles - 1) / tiles;
  if (want > most) want = most;
  if (want > units) want = units;
  if (want > 65535) want = 65535;         // (grid.y)
  if (want < 1) want = 1;
  Splits S;
  S.room = (int)want;
  S.per = (int)((units + want - 1) / want);
  S.count = (units + S.per - 1) / S.per;
  return S;
}

struct ListPlan {
  int tiles, splits, per;                 // row tiles, splits (capped so that the merge's keys fit LDS), units per split
  int n, cap, npad;                       // keys wanted per row, a list's capacity, the merge's keys padded to a power of two
  size_t lds_merge;
  u64 *lists;                             // set by carve()
  int *counts;
  void carve(Carver &cv) {
    const size_t n_lists = (size_t)tiles * splits * kListRows * 2;
    lists = cv.take<u64>(n_lists * cap);
    counts = cv.take<int>(n_lists);
  }
};
inline ListPlan list_plan(int tiles, int units, int n, int target, int force = 0) {
  ListPlan P{};
  const Splits S = plan_splits(tiles, units, target, force, kListMaxMerge / (2 * n));
  P.tiles = tiles; P.splits = S.count; P.per = S.per; P.n = n;
  P.cap = 2 * n < 32 ? 32 : 2 * n;
  P.npad = 2;
  while (P.npad < 2 * P.splits * n) P.npad <<= 1;
  P.lds_merge = (size_t)P.npad * sizeof(u64);
  return P;
}

// One workgroup per row: the row's 2 x splits lists ordered in LDS, the n best written out; behind the last entry -1 / `behind`.
// kRows = the lists' rows per tile.  (A template, so that a unit emits the kernel only if it launches it: a plain kernel in a header
// becomes device code of every unit that includes the header; static, because more than one unit launches it.)
template <int kRows>
static __global__ __launch_bounds__(kBlock) void k_lists_merge(const u64 *__restrict__ lists, const int *__restrict__ counts, int n, int cap,
                                                               int splits, int npad, float behind, int32_t *__restrict__ out_idx,
                                                               float *__restrict__ out_val) {
  extern __shared__ __align__(16) unsigned long long keys[];
  const size_t r = blockIdx.x;
  const size_t tile = r / kRows, ul = r % kRows;
  for (int i = threadIdx.x; i < npad; i += kBlock) {
    u64 key = 0ull;
    const int slot = i / n, j = i - slot * n;
    if (slot < 2 * splits) {
      const size_t lid = ((tile * splits + (slot >> 1)) * kRows + ul) * 2 + (slot & 1);
      if (j < min(counts[lid], n)) key = lists[lid * cap + j];
    }
    keys[i] = key;
  }
  order_keys_desc(keys, npad);
  for (int j = threadIdx.x; j < n; j += kBlock) {
    const u64 key = j < npad ? keys[j] : 0ull;
    if (key == 0ull) { out_idx[r * n + j] = -1; out_val[r * n + j] = behind; }
    else { out_idx[r * n + j] = (int32_t)(key & 0xFFFFFFFFull); out_val[r * n + j] = key_score(key); }
  }
}

// the merge of R rows' lists, after the launch that filled them
template <int kRows = kListRows>
static int lists_merge(const ListPlan &P, int R, float behind, int32_t *out_idx, float *out_val, hipStream_t st) {
  DRX_HIP(hipFuncSetAttribute((const void *)k_lists_merge<kRows>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds_merge));
  hipLaunchKernelGGL(k_lists_merge<kRows>, dim3(R), dim3(kBlock), P.lds_merge, st, P.lists, P.counts, P.n, P.cap, P.splits, P.npad, behind,
                     out_idx, out_val);
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

}  // namespace drx
