// Batched top-n recommendation: score[r, i] = epilogue(q[r, :] . T[i, :] (+ bias[i])) for R query rows against a whole table of items,
// the n best eligible items per row — WITHOUT the [R, n_items] score matrix (drx_cdae_forward + drx_topk write and re-read it:
// 4 MB per user at a 1 M-item catalogue).  The epilogue is a template parameter (include/drx.h DRX_REC_*): sigmoid of the biased sum
// (CDAE: q = hidden rows, T = W2T), the biased sum itself (Caser: q = [dense_0 output | user row], T = W1) or the sum clipped at 1e-6
// from below, no bias (DMF: q / T = the l2-normalised tower outputs); everything else is shared.  Columns of q and T between the
// model's width and ld must be ZERO, not merely unused: they are multiplied (0 x NaN would poison a row's scores).  Order = drx_topk's: descending score, ties by LARGER item index (heapq.nlargest over
// (score, iid), cdae.py:103), carried by the same 64-bit key (drx_keys.hpp).
//
// k_recommend   grid (user tiles of 128, item splits).  The products run on the matrix cores in fp32 (v_mfma_f32_32x32x2_f32: bit for
//               bit a k-ordered fmaf chain; the item's bias is added to the finished sum) with the ITEM rows as the A operand and the
//               users' query rows (LDS) as B, so that in the 32 x 32 accumulator tile a lane owns ONE user (column = lane & 31) and
//               16 of its items per tile.  A wave owns 32 users and walks the split's items 128 at a time (4 tiles: 4 independent
//               accumulators); the four waves of a workgroup read the same item rows (L1) for different users.  The W2T fragments
//               of the next k chunk / item block and the block's biases are loaded while the current chunk multiplies.
//               Selection is lane-local: every lane (user, half of the tile's rows) keeps its own candidate list in the scratch, its
//               length, the key of its n-th best so far and a LOGIT bound derived from it in registers.  A finished block costs an add
//               and a compare per score; only logits above the bound get the sigmoid, the exact key compare and a push.  A list that
//               reaches its capacity (2 n) is cut back to its n best ELIGIBLE keys by the whole wave (exclusion lookup = a binary
//               search in the user's CSR row, one key per lane; then the rank of every key among the list's keys, through LDS),
//               which also raises the lane's bound.  No atomic read-modify-write: a list has one writer, and what it ends up
//               holding is the n largest eligible keys its lane saw.
// k_lists_merge (drx_keys.hpp, with the lists' plan and layout)   one workgroup per user: the 2 x splits lists of the user ordered in
//               LDS, the n largest written out, -1 / -inf behind them.
// Every score is the same fmaf chain whatever the tile, the split or the neighbours of its user, and the keys are unique, so the
// result is a function of the inputs alone (bit-identical between calls, request orders and chunkings).
//
// drx_rows_rank_items (k_rank_keys / k_rank_count / k_rank_finish, at the end of this file) answers the other question on the same walk:
// where in the whole catalogue a GIVEN item stands for a row — a count of larger keys instead of a selection.
// drx_rows_pair_scores (k_pair_scores, behind them) answers for given (row, item) pairs with the score alone, from the pair's two rows:
// the same sum as one scalar fmaf chain per pair, no walk.
//
// Host side: the walking calls share one request check (request_ok), one walk plan, one RecArgs builder and one dispatch on the
// epilogue (by_epilogue); the extern "C" functions at the end of the file are the implementations.  The order of refusals is part of
// the ABI: DRX_EINVAL, then DRX_ENOTIMPL, then DRX_ESCRATCH (tests/test_gpu_rows_refusals.py).
#include <climits>
#include <hip/hip_runtime.h>
#include "drx_keys.hpp"

namespace drx {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kRecUsers = kListRows;    // users of a workgroup: 32 per wave
constexpr int kRecItems = 128;          // items of a block step: 4 accumulator tiles of 32
constexpr int kRecKC = 16;              // k columns of a chunk
constexpr int kRecKT = kRecKC / 8;      // k steps of 8 per chunk: 4 MFMAs per tile each
constexpr int kRecMaxN = 128, kRecMaxLd = 256;
constexpr int kRecTargetGroups = 256;   // workgroups a launch aims for: one per CU (the kernel's registers and LDS allow no more)

// A logit bound for a score threshold s: every z below it has sigmoidf_(z) < s STRICTLY, whatever the rounding of expf (taken as
// |computed - true| <= 1e-6 relative; the division and the addition of sigmoidf_ are monotone).  d ln(sigmoid) / dz = 1 - sigmoid:
//   s <= 1/2                 a step of 4e-6 in z lowers the score by more than 2e-6 relative
//   1 - s >= 2^-12           a step of 2e-6 * 4096 < 0.01 does
//   1 - s <  2^-12           (z > 8.3, towards saturation, where many logits share one score) the constant 8: sigmoid(8) = 0.99966
// 0.02 + 1e-5 |z| covers these and the error of the logf below.  s == 0: no bound.
__device__ __forceinline__ float rec_logit_bound(float s) {
  if (!(s > 0.0f)) return -INFINITY;
  const float om = 1.0f - s;
  if (om < 0x1p-12f) return 8.0f;
  const float z = logf(s / om);
  return z - 0.02f - 1e-5f * fabsf(z);
}

// An epilogue: the score of a finished sum z (the item's bias already added where kBias), and for the score s of a list's n-th best a
// bound on z: every z below it scores STRICTLY below s (such a z is dropped after one compare; the others take the exact key compare).
// "No n-th best yet" is never read off a score's sign: rec_compact sets the bound only once a list holds n eligible keys.
// The counting kernels (k_rank_count, below) want the bound from both sides for ONE item's sum z and score s: band(z, s, zlo, zhi) gives
// zlo <= zhi such that every sum above zhi scores STRICTLY above s and every sum below zlo STRICTLY below it; the sums in between
// (the band) take the exact score and key compare, so only speed rests on the band's width.  A side without a proof is open (+-inf).
struct RecSigmoidBias {                   // DRX_REC_SIGMOID_BIAS
  static constexpr bool kBias = true;
  static __device__ __forceinline__ float score(float z) { return sigmoidf_(z); }
  static __device__ __forceinline__ float bound(float s) { return rec_logit_bound(s); }
  // the mirror image of rec_logit_bound, by the same derivation (a step of 0.02 + 1e-5 |z| upwards raises the score by more than
  // 2e-6 relative while 1 - s >= 2^-12).  Towards saturation many sums share the score: open above.  Below 1e-30 (0 included) the
  // quotient of sigmoidf_ leaves the normal floats and the relative-error argument with them: open below, and sigmoid(-60) = 8.7e-27
  // lies above every such s.
  static __device__ __forceinline__ void band(float z, float s, float &zlo, float &zhi) {
    (void)z;
    if (!(s >= 1e-30f)) { zlo = -INFINITY; zhi = -60.0f; return; }
    zlo = rec_logit_bound(s);
    const float om = 1.0f - s;
    if (om < 0x1p-12f) { zhi = INFINITY; return; }
    const float zs = logf(s / om);
    zhi = zs + 0.02f + 1e-5f * fabsf(zs);
  }
};
struct RecBias {                          // DRX_REC_BIAS: the sum is the compared value: exact, no margin (negative scores included)
  static constexpr bool kBias = true;
  static __device__ __forceinline__ float score(float z) { return z; }
  static __device__ __forceinline__ float bound(float s) { return s; }
  static __device__ __forceinline__ void band(float z, float s, float &zlo, float &zhi) { (void)s; zlo = zhi = z; }   // the band: z == zt
};
struct RecClip {                          // DRX_REC_CLIP: at the floor every item ties and the item index decides: no bound there
  static constexpr bool kBias = false;
  static __device__ __forceinline__ float score(float z) { return fmaxf(1e-6f, z); }
  static __device__ __forceinline__ float bound(float s) { return s > 1e-6f ? s : -INFINITY; }
  static __device__ __forceinline__ void band(float z, float s, float &zlo, float &zhi) {
    if (s > 1e-6f) { zlo = zhi = z; return; }       // above the floor the score is the sum
    zlo = -INFINITY; zhi = 1e-6f;                   // at the floor: everything at or below it ties, everything above it is ahead
  }
};

struct RecArgs {
  const float *table, *bias, *q;   // [N][ld] item rows, [N] (null: an epilogue without a bias), [R][ld] query rows
  const int32_t *uid;
  const int64_t *xptr;          // exclusion CSR (or null)
  const int32_t *xidx;
  int R, N, ld;
  int nch;                      // k chunks of kRecKC
  int hs;                       // floats between users' rows in LDS
  int n, cap;                   // list: wanted / capacity
  int splits, ips;              // item splits, items per split (a multiple of kRecItems)
  u64 *lists;                   // [tiles][splits][128][2][cap]
  int *counts;                  // [tiles][splits][128][2]
};

// Table fragments of one chunk of one item block: tile s, k step t: the lane's item row (lane & 31), 4 consecutive k of its half.
// MFMA (t, c) multiplies k = 8 t + c (lanes 0..31) and k = 8 t + 4 + c (lanes 32..63) of the chunk.
__device__ __forceinline__ void rec_load_a(const RecArgs &A, int item0, int kc, int col, int hh, float4 (&a)[4][kRecKT]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const unsigned row = min((unsigned)item0 + 32u * s + col, (unsigned)A.N - 1u);   // (rows behind the catalogue: any valid row, never looked at)
    const float *p = A.table + (size_t)row * A.ld;
#pragma unroll
    for (int t = 0; t < kRecKT; ++t) {
      // (no branch around a load: k steps behind the row read the row's last float4 — their columns of q are ZERO in LDS)
      a[s][t] = *reinterpret_cast<const float4 *>(p + min(kc * kRecKC + 8 * t + 4 * hh, A.ld - 4));
    }
  }
}

// the biases of a block in accumulator layout: register g * 4 + q of tile s = item item0 + 32 s + 8 g + 4 half + q
__device__ __forceinline__ void rec_load_bias(const RecArgs &A, int item0, int hh, f32x16 (&c)[4]) {
  const bool whole = (unsigned)item0 + (unsigned)kRecItems <= (unsigned)A.N;       // wave-uniform: every block but the catalogue's last
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const unsigned base = (unsigned)item0 + 32u * s + 8u * g + 4u * hh, N = (unsigned)A.N;   // (unsigned: n_items may be 2^31 - 1)
      float4 v = f4_zero();
      if (whole) v = *reinterpret_cast<const float4 *>(A.bias + base);
      else {
        if (base < N) v.x = A.bias[base];
        if (base + 1 < N) v.y = A.bias[base + 1];
        if (base + 2 < N) v.z = A.bias[base + 2];
        if (base + 3 < N) v.w = A.bias[base + 3];
      }
      c[s][4 * g] = v.x; c[s][4 * g + 1] = v.y; c[s][4 * g + 2] = v.z; c[s][4 * g + 3] = v.w;
    }
  }
}

__device__ __forceinline__ bool rec_excluded(const int32_t *xidx, int64_t lo, int64_t hi, int item) {
  const int64_t end = hi;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (xidx[mid] < item) lo = mid + 1; else hi = mid;
  }
  return lo < end && xidx[lo] == item;
}

// The list of lane L (wave-uniform) cut back to its n best, in order, by the whole wave; L's registers follow.  The exclusion lookup
// happens HERE, for all keys of the list at once (a push does not wait for a binary search of dependent loads): excluded keys drop
// out before the ranks are taken, so the n-th best — the lane's new bound — is the n-th best ELIGIBLE key.
template <class E>
__device__ __forceinline__ void rec_compact(const RecArgs &A, u64 *wave_lists, u64 *cb, int L, int lane, int64_t xlo, int64_t xhi, int &cnt,
                                            u64 &tkey, float &zt) {
  const int cL = __shfl(cnt, L, kWave);
  const int64_t lo = __shfl(xlo, L, kWave), hi = __shfl(xhi, L, kWave);
  u64 *list = wave_lists + (size_t)(2 * (L & 31) + (L >> 5)) * A.cap;
  // L's pushes have reached the L2 (this fence waits for the wave's stores) and are read from there (the loads pass the L1):
  // writer and readers are lanes of one wave, nothing beyond the CU's own L2 is involved
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  u64 k[4];
  int rank[4];
  int alive = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = lane + 64 * j;
    k[j] = i < cL ? __hip_atomic_load(list + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    if (A.xptr && k[j] != 0ull && rec_excluded(A.xidx, lo, hi, (int)(uint32_t)k[j])) k[j] = 0ull;
    cb[i] = k[j];
    rank[j] = 0;
    alive += __popcll(__ballot(k[j] != 0ull));
  }
  wave_lds_sync();
  for (int i = 0; i < cL; ++i) {
    const u64 o = cb[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) rank[j] += o > k[j] ? 1 : 0;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (k[j] != 0ull && rank[j] < A.n) list[rank[j]] = k[j];        // (keys are unique: the ranks of the live ones are 0 .. alive - 1)
    if (k[j] != 0ull && rank[j] == A.n - 1) cb[256] = k[j];
  }
  wave_lds_sync();
  const u64 nth = cb[256];
  if (lane == L) {
    if (alive >= A.n) { tkey = nth; zt = E::bound(key_score(nth)); }    // (fewer: the bound stays where it was)
    cnt = min(alive, A.n);
  }
  wave_lds_sync();
}

template <class E>
__global__ __launch_bounds__(256) void k_recommend(RecArgs A) {
  extern __shared__ __align__(16) float lds[];
  float *h_s = lds;                                                   // [128][hs]
  float *dump_all = h_s + (size_t)kRecUsers * A.hs;                   // [4 waves][16 registers][64 lanes]
  u64 *cb_all = reinterpret_cast<u64 *>(dump_all + 4 * 16 * 64);      // [4 waves][256 keys + the n-th + pad]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hh = lane >> 5;
  const int tile = blockIdx.x, sp = blockIdx.y;
  const int r0 = tile * kRecUsers;
  const int ldp4 = A.nch * (kRecKC / 4);
  for (int i = tid; i < kRecUsers * ldp4; i += 256) {
    const int u = i / ldp4, c4 = i - u * ldp4;
    float4 v = f4_zero();
    if (r0 + u < A.R && 4 * c4 < A.ld) v = *reinterpret_cast<const float4 *>(A.q + (size_t)(r0 + u) * A.ld + 4 * c4);
    *reinterpret_cast<float4 *>(h_s + (size_t)u * A.hs + 4 * c4) = v;
  }
  __syncthreads();
  if (r0 + wave * 32 >= A.R) return;                                  // (no user in this wave; no barrier below)

  float *dump = dump_all + wave * (16 * 64);
  u64 *cb = cb_all + wave * 258;
  const int ul = wave * 32 + col, r = r0 + ul;
  const bool uvalid = r < A.R;
  int64_t xlo = 0, xhi = 0;
  if (uvalid && A.xptr) { const int u = A.uid[r]; xlo = A.xptr[u]; xhi = A.xptr[u + 1]; }
  const size_t group = (size_t)tile * A.splits + sp;
  u64 *wave_lists = A.lists + ((group * kRecUsers + wave * 32) * 2) * (size_t)A.cap;
  u64 *mylist = wave_lists + (size_t)(2 * col + hh) * A.cap;
  float zt = uvalid ? -INFINITY : INFINITY;                          // logits below it cannot enter the list
  u64 tkey = 0ull;                                                    // the list's n-th best at its last compaction
  int cnt = 0;

  const int i_begin = sp * A.ips, i_end = (int)min((int64_t)A.N, (int64_t)i_begin + A.ips);
  const int nblocks = (int)(((int64_t)i_end - i_begin + kRecItems - 1) / kRecItems);
  const float *hrow = h_s + (size_t)ul * A.hs + 4 * hh;

  f32x16 acc[4], bias[4];
  float4 a0[4][kRecKT], a1[4][kRecKT];            // table fragments of the even / odd chunk in flight (nch is even)
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[s][e] = 0.f;
  rec_load_a(A, i_begin, 0, col, hh, a0);

  // one chunk: 4 MFMAs per tile and k step, the 4 tiles' accumulators back to back (independent)
#define DRX_REC_CHUNK(a, kc)                                                                                         \
  _Pragma("unroll") for (int t = 0; t < kRecKT; ++t) {                                                               \
    if ((kc) * kRecKC + 8 * t < A.ld) {                       /* wave-uniform: k steps behind the row are skipped */  \
      const float4 b = *reinterpret_cast<const float4 *>(hrow + (kc) * kRecKC + 8 * t);                              \
      _Pragma("unroll") for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][t].x, b.x, acc[s], 0, 0, 0); \
      _Pragma("unroll") for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][t].y, b.y, acc[s], 0, 0, 0); \
      _Pragma("unroll") for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][t].z, b.z, acc[s], 0, 0, 0); \
      _Pragma("unroll") for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][t].w, b.w, acc[s], 0, 0, 0); \
    }                                                                                                                \
  }

  for (int blk = 0; blk < nblocks; ++blk) {
    const int item0 = i_begin + blk * kRecItems;
    for (int kc = 0; kc + 2 < A.nch; kc += 2) {                      // the fragments of the next chunk load while this one multiplies
      rec_load_a(A, item0, kc + 1, col, hh, a1);
      DRX_REC_CHUNK(a0, kc)
      rec_load_a(A, item0, kc + 2, col, hh, a0);
      DRX_REC_CHUNK(a1, kc + 1)
    }
    // the block's last two chunks; beside them its biases and the first fragments of the next block
    rec_load_a(A, item0, A.nch - 1, col, hh, a1);
    if constexpr (E::kBias) rec_load_bias(A, item0, hh, bias);
    DRX_REC_CHUNK(a0, A.nch - 2)
    rec_load_a(A, blk + 1 < nblocks ? item0 + kRecItems : item0, 0, col, hh, a0);
    DRX_REC_CHUNK(a1, A.nch - 1)
#undef DRX_REC_CHUNK
    // the block's 128 x 32 sums of this wave: an add (where there is a bias) and a compare per score
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      uint32_t m = 0;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if constexpr (E::kBias) acc[s][e] += bias[s][e];
        m |= (acc[s][e] >= zt) ? (1u << e) : 0u;
      }
      if (__ballot(m != 0)) {                                         // rare once the lists are warm
#pragma unroll
        for (int e = 0; e < 16; ++e) dump[e * 64 + lane] = acc[s][e]; // (a lane reads back its own words only)
        const int ibase = item0 + 32 * s + 4 * hh;
        while (__ballot(m != 0)) {
          if (m != 0) {
            const int e = __ffs(m) - 1;
            m &= m - 1;
            const unsigned item = (unsigned)ibase + 8u * (e >> 2) + (e & 3);
            if (uvalid && item < (unsigned)i_end) {
              const float sc = E::score(dump[e * 64 + lane]);
              const u64 key = make_key(sc, item);
              if (key > tkey) { mylist[cnt] = key; ++cnt; }
            }
          }
          u64 full = __ballot(cnt >= A.cap);
          while (full) {
            const int L = __ffsll((long long)full) - 1;
            full &= full - 1;
            rec_compact<E>(A, wave_lists, cb, L, lane, xlo, xhi, cnt, tkey, zt);
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[s][e] = 0.f;
    }
  }
  // every list down to its n best eligible keys at most, its length beside it
  u64 over = __ballot(cnt > A.n || (A.xptr && cnt > 0));
  while (over) {
    const int L = __ffsll((long long)over) - 1;
    over &= over - 1;
    rec_compact<E>(A, wave_lists, cb, L, lane, xlo, xhi, cnt, tkey, zt);
  }
  if (uvalid) A.counts[(group * kRecUsers + ul) * 2 + hh] = cnt;
}

// ---- the host side every call of this file shares --------------------------------------------------------------------------------------
// What the three walking calls (recommend, rank_items, rank_lists) are asked, as given.
struct RecRequest {
  const float *table, *bias;
  int n_items, ld, epilogue;
  const float *q;
  const int32_t *uid;
  int R;
  const int64_t *xptr;          // exclusion CSR (or null)
  const int32_t *xidx;
};

bool ld_ok(int ld) { return ld >= 4 && !(ld & 3); }
// the clip has no bias, the other two need one
bool epilogue_ok(int epilogue, const float *bias) {
  if (epilogue != DRX_REC_SIGMOID_BIAS && epilogue != DRX_REC_BIAS && epilogue != DRX_REC_CLIP) return false;
  return (epilogue == DRX_REC_CLIP) == (bias == nullptr);
}
// false: DRX_EINVAL, before anything else is looked at (a call adds its own pointers to it)
bool request_ok(const RecRequest &Q) {
  if (!Q.table || !Q.q || Q.R < 1 || Q.n_items < 1 || !ld_ok(Q.ld) || !epilogue_ok(Q.epilogue, Q.bias)) return false;
  return (Q.xptr != nullptr) == (Q.xidx != nullptr) && (!Q.xptr || Q.uid);
}

// fn(E{}) for the epilogue struct E of a checked request
template <class F>
int by_epilogue(int epilogue, F &&fn) {
  switch (epilogue) {
    case DRX_REC_SIGMOID_BIAS: return fn(RecSigmoidBias{});
    case DRX_REC_BIAS: return fn(RecBias{});
    case DRX_REC_CLIP: return fn(RecClip{});
    default: return DRX_EINVAL;
  }
}

// What the walk needs from the shape of a request, before its items are split: false outside the domain (rows wider than 256 floats).
struct WalkPlan {
  int tiles, blocks;             // row tiles of kRecUsers, item blocks of kRecItems
  int nch, hs;
  size_t lds;                    // the tile's query rows and the per-wave dump
};
bool walk_plan(int R, int n_items, int ld, WalkPlan &W) {
  if (R < 1 || n_items < 1 || !ld_ok(ld) || ld > kRecMaxLd) return false;
  W.tiles = (R + kRecUsers - 1) / kRecUsers;
  W.blocks = (int)(((int64_t)n_items + kRecItems - 1) / kRecItems);
  W.nch = 2 * ((ld + 2 * kRecKC - 1) / (2 * kRecKC));                // (even: the kernels alternate two fragment buffers)
  W.hs = W.nch * kRecKC + 4;                                         // + 4: the 32 users of a wave spread over the LDS banks
  W.lds = ((size_t)kRecUsers * W.hs + 4 * 16 * 64) * sizeof(float);
  return true;
}

// the kernels' view of a request: `splits` splits of `bps` item blocks each; the selector adds its lists
RecArgs rec_args(const RecRequest &Q, const WalkPlan &W, int splits, int bps) {
  RecArgs A{};
  A.table = Q.table; A.bias = Q.bias; A.q = Q.q; A.uid = Q.uid; A.xptr = Q.xptr; A.xidx = Q.xidx;
  A.R = Q.R; A.N = Q.n_items; A.ld = Q.ld; A.nch = W.nch; A.hs = W.hs; A.splits = splits; A.ips = bps * kRecItems;
  return A;
}

// ---- the selector: the walk plus the lists (drx_keys.hpp: the splits capped so that the merge's keys fit LDS) ---------------------------
struct RecPlan {
  WalkPlan W;
  ListPlan L;
  size_t lds_main;               // W.lds and the compaction's keys: [4 waves][256 keys + the n-th + pad]
};

bool rec_plan(int R, int n_items, int ld, int n, RecPlan &P) {
  if (n < 1 || n > kRecMaxN || !walk_plan(R, n_items, ld, P.W)) return false;
  P.L = list_plan(P.W.tiles, P.W.blocks, n, kRecTargetGroups);
  P.lds_main = P.W.lds + 4 * 258 * sizeof(u64);
  return true;
}

size_t rec_scratch_bytes(int R, int n_items, int ld, int n) {
  RecPlan P;
  if (!rec_plan(R, n_items, ld, n, P)) return 0;
  Carver cv(nullptr, 0);
  P.L.carve(cv);
  return align_up(cv.off, 256) + 256;
}

// the one host function behind drx_rows_recommend and drx_cdae_recommend
int rec_run(const RecRequest &Q, int n, int32_t *out_idx, float *out_val, void *scratch, size_t scratch_bytes, void *stream) {
  if (!request_ok(Q) || !out_idx || !out_val || n < 1) return DRX_EINVAL;
  RecPlan P;
  if (!rec_plan(Q.R, Q.n_items, Q.ld, n, P)) return DRX_ENOTIMPL;      // n > 128 or rows wider than 256 floats: a score matrix + drx_topk
  if (!scratch) return DRX_ESCRATCH;
  Carver cv(scratch, scratch_bytes);
  P.L.carve(cv);
  if (!cv.ok()) return DRX_ESCRATCH;
  RecArgs A = rec_args(Q, P.W, P.L.splits, P.L.per);
  A.n = n; A.cap = P.L.cap; A.lists = P.L.lists; A.counts = P.L.counts;
  hipStream_t st = (hipStream_t)stream;
  return by_epilogue(Q.epilogue, [&](auto e) -> int {
    using E = decltype(e);
    DRX_HIP(hipFuncSetAttribute((const void *)k_recommend<E>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds_main));
    hipLaunchKernelGGL(k_recommend<E>, dim3(P.W.tiles, P.L.splits), dim3(256), P.lds_main, st, A);
    return lists_merge(P.L, Q.R, -INFINITY, out_idx, out_val, st);
  });
}

// ---- catalogue ranks of given (row, item) pairs (drx_rows_rank_items) ------------------------------------------------------------------
// rank[r] = the number of eligible items i != t[r] whose key is larger than the key of the row's target t[r]: the position of t[r] in
// the list k_recommend + k_lists_merge would give for an unbounded n.  Counting needs no lists: the same product walk, two compares
// per score.
// k_rank_keys    grid (user tiles).  The targets' own sums and keys: a wave walks its 32 rows and computes the 128-item block that holds
//                a row's target (none when it is the block just done), with k_recommend's fragment loads and MFMA order — the same
//                chain, bit for bit.  The lane that owns the element writes tz[r] / tkey[r].
// k_rank_count   grid (user tiles, item splits).  The walk of k_recommend over the split; per lane the target's key and the band
//                zlo <= zhi of its epilogue.  A finished tile gives two bit masks (ahead for certain / in the band); the bits of items
//                behind the split's end, of the target and of excluded items are cleared, the first mask is counted, the band's bits
//                take the exact key compare.  Exclusions: a cursor into the user's ascending CSR row, advanced block by block.
// k_rank_finish  a row's 2 x splits partial counts summed in a fixed order (no atomics anywhere).
struct RankArgs {
  const int32_t *target;         // [R]
  float *tz;                     // [R] the target's biased sum
  u64 *tkey;                     // [R] its key; 0: a target outside the catalogue
  int *partial;                  // [tiles][splits][128][2]
};

// (as the head of k_recommend) the tile's query rows into LDS, zero behind R and behind ld
__device__ __forceinline__ void rank_load_q(const RecArgs &A, float *h_s, int tid, int r0) {
  const int ldp4 = A.nch * (kRecKC / 4);
  for (int i = tid; i < kRecUsers * ldp4; i += 256) {
    const int u = i / ldp4, c4 = i - u * ldp4;
    float4 v = f4_zero();
    if (r0 + u < A.R && 4 * c4 < A.ld) v = *reinterpret_cast<const float4 *>(A.q + (size_t)(r0 + u) * A.ld + 4 * c4);
    *reinterpret_cast<float4 *>(h_s + (size_t)u * A.hs + 4 * c4) = v;
  }
}

// one chunk of k_recommend's walk: 4 MFMAs per tile and k step, in its order
__device__ __forceinline__ void rank_chunk(const RecArgs &A, const float4 (&a)[4][kRecKT], int kc, const float *hrow, f32x16 (&acc)[4]) {
#pragma unroll
  for (int t = 0; t < kRecKT; ++t) {
    if (kc * kRecKC + 8 * t < A.ld) {
      const float4 b = *reinterpret_cast<const float4 *>(hrow + kc * kRecKC + 8 * t);
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][t].x, b.x, acc[s], 0, 0, 0);
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][t].y, b.y, acc[s], 0, 0, 0);
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][t].z, b.z, acc[s], 0, 0, 0);
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][t].w, b.w, acc[s], 0, 0, 0);
    }
  }
}

// The biased sums of the block at item0 in acc (the walk both kernels share).  a0 holds chunk 0 of the block on entry and chunk 0 of
// the block at item_next on return.
template <class E>
__device__ __forceinline__ void rank_block(const RecArgs &A, int item0, int item_next, int col, int hh, const float *hrow,
                                           float4 (&a0)[4][kRecKT], float4 (&a1)[4][kRecKT], f32x16 (&acc)[4]) {
  f32x16 bias[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[s][e] = 0.f;
  for (int kc = 0; kc + 2 < A.nch; kc += 2) {
    rec_load_a(A, item0, kc + 1, col, hh, a1);
    rank_chunk(A, a0, kc, hrow, acc);
    rec_load_a(A, item0, kc + 2, col, hh, a0);
    rank_chunk(A, a1, kc + 1, hrow, acc);
  }
  rec_load_a(A, item0, A.nch - 1, col, hh, a1);
  if constexpr (E::kBias) rec_load_bias(A, item0, hh, bias);
  rank_chunk(A, a0, A.nch - 2, hrow, acc);
  rec_load_a(A, item_next, 0, col, hh, a0);
  rank_chunk(A, a1, A.nch - 1, hrow, acc);
  if constexpr (E::kBias) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[s][e] += bias[s][e];
  }
}

template <class E>
__global__ __launch_bounds__(256) void k_rank_keys(RecArgs A, RankArgs K) {
  extern __shared__ __align__(16) float lds[];
  float *h_s = lds;                                                   // [128][hs]
  float *dump_all = h_s + (size_t)kRecUsers * A.hs;                   // [4 waves][16 registers][64 lanes]
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r0 = blockIdx.x * kRecUsers;
  rank_load_q(A, h_s, tid, r0);
  __syncthreads();
  if (r0 + wave * 32 >= A.R) return;                                  // (no row in this wave; no barrier below)

  float *dump = dump_all + wave * (16 * 64);
  const float *hrow = h_s + (size_t)(wave * 32 + col) * A.hs + 4 * hh;
  f32x16 acc[4];
  float4 a0[4][kRecKT], a1[4][kRecKT];
  int done = -1;                                                      // the block acc holds
  for (int j = 0; j < 32; ++j) {
    const int r = r0 + wave * 32 + j;
    if (r >= A.R) break;
    const int t = __builtin_amdgcn_readfirstlane(K.target[r]);
    if ((unsigned)t >= (unsigned)A.N) {
      if (lane == j) { K.tz[r] = 0.f; K.tkey[r] = 0ull; }
      continue;
    }
    const int item0 = t & ~(kRecItems - 1);
    if (item0 != done) {
      rec_load_a(A, item0, 0, col, hh, a0);
      rank_block<E>(A, item0, item0, col, hh, hrow, a0, a1, acc);
      done = item0;
    }
    // element (item t, row j) of the block: tile ts, register te of the lane with column j in half th
    const int off = t - item0, ts = off >> 5, m = off & 31, te = 4 * (m >> 3) + (m & 3), th = (m >> 2) & 1;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s == ts) {
#pragma unroll
        for (int e = 0; e < 16; ++e) dump[e * 64 + lane] = acc[s][e];   // (a lane reads back its own words only)
      }
    }
    if (lane == 32 * th + j) {
      const float z = dump[te * 64 + lane];
      K.tz[r] = z;
      K.tkey[r] = make_key(E::score(z), (unsigned)t);
    }
  }
}

template <class E>
__global__ __launch_bounds__(256) void k_rank_count(RecArgs A, RankArgs K) {
  extern __shared__ __align__(16) float lds[];
  float *h_s = lds;                                                   // [128][hs]
  float *dump_all = h_s + (size_t)kRecUsers * A.hs;                   // [4 waves][16 registers][64 lanes]
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x, sp = blockIdx.y;
  const int r0 = tile * kRecUsers;
  rank_load_q(A, h_s, tid, r0);
  __syncthreads();
  if (r0 + wave * 32 >= A.R) return;                                  // (no row in this wave; no barrier below)

  float *dump = dump_all + wave * (16 * 64);
  const int ul = wave * 32 + col, r = r0 + ul;
  const bool uvalid = r < A.R;
  const int i_begin = sp * A.ips, i_end = (int)min((int64_t)A.N, (int64_t)i_begin + A.ips);
  const int nblocks = (int)(((int64_t)i_end - i_begin + kRecItems - 1) / kRecItems);
  const float *hrow = h_s + (size_t)ul * A.hs + 4 * hh;

  u64 tkey = 0ull;
  float zlo = INFINITY, zhi = INFINITY;                               // (no row, no target: nothing is counted)
  unsigned t = 0xFFFFFFFFu;
  int64_t xc = 0, xhi = 0;                                            // the cursor into the user's exclusion row, its end
  if (uvalid) {
    tkey = K.tkey[r];
    if (tkey != 0ull) {
      t = (unsigned)tkey;
      E::band(K.tz[r], key_score(tkey), zlo, zhi);
      if (A.xptr) {
        const int u = A.uid[r];
        int64_t lo = A.xptr[u];
        const int64_t end = A.xptr[u + 1];
        xhi = end;
        int64_t hi = end;
        while (lo < hi) {                                             // the first entry at or behind the split's first item
          const int64_t mid = lo + ((hi - lo) >> 1);
          if (A.xidx[mid] < i_begin) lo = mid + 1; else hi = mid;
        }
        xc = lo;
      }
    }
  }
  // the target's place, if it lies in this lane's half of a tile: the tile's first item and the register (else no tile matches)
  const unsigned tm = t & 31u;
  const unsigned t_tile = (t != 0xFFFFFFFFu && ((tm >> 2) & 1u) == (unsigned)hh) ? (t & ~31u) : 0xFFFFFFFFu;
  const uint32_t t_bit = 1u << (4u * (tm >> 3) + (tm & 3u));

  f32x16 acc[4];
  float4 a0[4][kRecKT], a1[4][kRecKT];
  int cnt = 0;
  rec_load_a(A, i_begin, 0, col, hh, a0);
  for (int blk = 0; blk < nblocks; ++blk) {
    const int item0 = i_begin + blk * kRecItems;
    // the excluded items of the block in this lane's half: bit 16 s + e of xm (the loads overlap the products below)
    u64 xm = 0ull;
    while (xc < xhi) {
      const unsigned off = (unsigned)A.xidx[xc] - (unsigned)item0;
      if (off >= (unsigned)kRecItems) break;                          // (behind the block; entries ascend, none lies before it)
      ++xc;
      if (((off >> 2) & 1u) == (unsigned)hh) xm |= 1ull << (16u * (off >> 5) + 4u * ((off & 31u) >> 3) + (off & 3u));
    }
    rank_block<E>(A, item0, blk + 1 < nblocks ? item0 + kRecItems : item0, col, hh, hrow, a0, a1, acc);
    const bool whole = (unsigned)item0 + (unsigned)kRecItems <= (unsigned)i_end;   // wave-uniform: every block but the split's last
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const unsigned ibase = (unsigned)item0 + 32u * s + 4u * hh;
      uint32_t ma = 0, mb = 0, keep = 0xFFFFu;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float z = acc[s][e];
        ma |= (z > zhi) ? (1u << e) : 0u;
        mb |= (z >= zlo && z <= zhi) ? (1u << e) : 0u;
      }
      if (!whole) {
        keep = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) keep |= (ibase + 8u * (e >> 2) + (e & 3) < (unsigned)i_end) ? (1u << e) : 0u;
      }
      keep &= ~(uint32_t)((xm >> (16 * s)) & 0xFFFFull);
      if ((unsigned)item0 + 32u * s == t_tile) keep &= ~t_bit;        // i != t, whatever the band
      ma &= keep;
      mb &= keep;
      cnt += __popc(ma);
      if (__ballot(mb != 0)) {                                        // the band: rare unless many items tie with the target
#pragma unroll
        for (int e = 0; e < 16; ++e) dump[e * 64 + lane] = acc[s][e]; // (a lane reads back its own words only)
        while (mb != 0) {
          const int e = __ffs(mb) - 1;
          mb &= mb - 1;
          const unsigned item = ibase + 8u * (e >> 2) + (e & 3);
          const u64 key = make_key(E::score(dump[e * 64 + lane]), item);
          cnt += key > tkey ? 1 : 0;
        }
      }
    }
  }
  if (uvalid) K.partial[(((size_t)tile * A.splits + sp) * kRecUsers + ul) * 2 + hh] = cnt;
}

__global__ __launch_bounds__(kBlock) void k_rank_finish(const int *__restrict__ partial, const u64 *__restrict__ tkey, int R, int splits,
                                                        int32_t *__restrict__ out_rank, float *__restrict__ out_score) {
  const int r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= R) return;
  const u64 key = tkey[r];
  if (key == 0ull) { out_rank[r] = -1; out_score[r] = -INFINITY; return; }
  const size_t tile = r / kRecUsers, ul = r % kRecUsers;
  int sum = 0;
  for (int sp = 0; sp < splits; ++sp) {
    const int *p = partial + ((tile * splits + sp) * kRecUsers + ul) * 2;
    sum += p[0];
    sum += p[1];
  }
  out_rank[r] = sum;
  out_score[r] = key_score(key);
}

// the walk plan and its splits WITHOUT the merge's cap; S.room = the splits the scratch has room for: what the launch aims at, so that
// a longer catalogue does not size it
struct RankPlan {
  WalkPlan W;
  Splits S;
};
bool rank_plan(int R, int n_items, int ld, RankPlan &P) {
  if (!walk_plan(R, n_items, ld, P.W)) return false;
  P.S = plan_splits(P.W.tiles, P.W.blocks, kRecTargetGroups, 0, INT_MAX);
  return true;
}

RankArgs rank_layout(Carver &cv, const RankPlan &P, int R) {
  RankArgs K;
  K.target = nullptr;
  K.tz = cv.take<float>((size_t)R);
  K.tkey = cv.take<u64>((size_t)R);
  K.partial = cv.take<int>((size_t)P.W.tiles * P.S.room * kRecUsers * 2);
  return K;
}

// ---- catalogue ranks of a row's LIST of targets (drx_rows_rank_lists) ------------------------------------------------------------------
// The pair form above scores a user with T targets against the catalogue T times.  Here row r owns targets[tptr[r] .. tptr[r + 1]),
// ascending, and costs one counting walk per G of them; every rank and score is what the pair form gives for (q[r], uid[r], target),
// bit for bit: the same key from the same rank_block<E>, the same band, the same exclusion rule, integer counts.
// k_rankl_keys    grid (user tiles).  A wave merges the ascending lists of its 32 rows: the next 128-item block is the wave-minimum of
//                 the lanes' cursors, computed ONCE; every lane whose row has targets in it takes them out of the per-wave dump, tile by
//                 tile, and writes tz / tkey.  At most min(sum of the rows' lengths, blocks of the catalogue) blocks per wave.
// k_rankl_count   grid (user tiles, item splits).  k_rank_count's walk; the thresholds (zlo, zhi, tkey) of up to G targets per row and
//                 their running counts live in LDS, [target][row] (a lane's own column: conflict-free), not in registers.  A finished
//                 tile first takes one compare against the row's LOWEST zlo; only a tile in which some score of some lane reaches it
//                 builds the masks per target.  A wave whose longest row holds more than G targets walks again for the next G.
// k_rankl_finish  a target's 2 x splits partial counts summed in a fixed order (no atomics anywhere).
struct RankListArgs {
  const int64_t *tptr;           // [R + 1] offsets into targets / out_rank / out_score (absolute)
  const int32_t *targets;
  int64_t base, P;               // tptr[0] and tptr[R] - tptr[0]: the scratch is indexed by p - base
  float *tz;                     // [P] a target's biased sum
  u64 *tkey;                     // [P] its key; 0: a target outside the catalogue
  int *partial;                  // [P][2 x splits]
  int G;                         // targets of a row whose state LDS holds at a time
};

constexpr int kRankListMaxG = 32;
constexpr size_t kRecLdsBytes = 160 * 1024;                             // LDS of a workgroup on gfx950
constexpr size_t kRankListSlot = (size_t)kRecUsers * (2 * sizeof(float) + sizeof(u64) + 2 * sizeof(int));   // one target of every row

// the targets of row r, clamped into [base, base + P): whatever the offsets hold, no access leaves the scratch
__device__ __forceinline__ void rankl_row(const RankListArgs &K, int r, int R, int64_t &beg, int64_t &end) {
  beg = end = K.base;
  if (r < R) {
    const int64_t hi = K.base + K.P;
    beg = min(max(K.tptr[r], K.base), hi);
    end = min(max(K.tptr[r + 1], beg), hi);
  }
}

template <class E>
__global__ __launch_bounds__(256) void k_rankl_keys(RecArgs A, RankListArgs K) {
  extern __shared__ __align__(16) float lds[];
  float *h_s = lds;                                                   // [128][hs]
  float *dump_all = h_s + (size_t)kRecUsers * A.hs;                   // [4 waves][16 registers][64 lanes]
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r0 = blockIdx.x * kRecUsers;
  rank_load_q(A, h_s, tid, r0);
  __syncthreads();
  if (r0 + wave * 32 >= A.R) return;                                  // (no row in this wave; no barrier below)

  float *dump = dump_all + wave * (16 * 64);
  const float *hrow = h_s + (size_t)(wave * 32 + col) * A.hs + 4 * hh;
  int64_t cur, end;                                                   // the row's cursor (both halves of a column carry it)
  rankl_row(K, r0 + wave * 32 + col, A.R, cur, end);
  f32x16 acc[4];
  float4 a0[4][kRecKT], a1[4][kRecKT];
  for (;;) {
    int t = 0;
    while (cur < end) {                                               // targets outside the catalogue: no key
      t = K.targets[cur];
      if ((unsigned)t < (unsigned)A.N) break;
      if (hh == 0) { K.tz[cur - K.base] = 0.f; K.tkey[cur - K.base] = 0ull; }
      ++cur;
    }
    int b = cur < end ? (t >> 7) : 0x7FFFFFFF;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) b = min(b, __shfl_xor(b, m, kWave));
    b = __builtin_amdgcn_readfirstlane(b);
    if (b == 0x7FFFFFFF) break;                                       // every list is done
    const int item0 = b * kRecItems;
    rec_load_a(A, item0, 0, col, hh, a0);
    rank_block<E>(A, item0, item0, col, hh, hrow, a0, a1, acc);
    // (an unsorted row may leave a target of this block behind: its lane still points at the block, which is then computed again;
    //  the lane that set the minimum always advances, so the loop ends)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const unsigned tile0 = (unsigned)item0 + 32u * s;
      if (__ballot(cur < end && ((unsigned)t & ~31u) == tile0)) {
#pragma unroll
        for (int e = 0; e < 16; ++e) dump[e * 64 + lane] = acc[s][e];   // (a lane reads back its own words only)
        while (cur < end && (unsigned)t < (unsigned)A.N && ((unsigned)t & ~31u) == tile0) {
          const int m = t & 31;
          if (((m >> 2) & 1) == hh) {                                 // element (item t, this column): register te of this half
            const float z = dump[(4 * (m >> 3) + (m & 3)) * 64 + lane];
            K.tz[cur - K.base] = z;
            K.tkey[cur - K.base] = make_key(E::score(z), (unsigned)t);
          }
          ++cur;
          if (cur < end) t = K.targets[cur];
        }
      }
    }
  }
}

template <class E>
__global__ __launch_bounds__(256) void k_rankl_count(RecArgs A, RankListArgs K) {
  extern __shared__ __align__(16) float lds[];
  float *h_s = lds;                                                   // [128][hs]
  float *dump_all = h_s + (size_t)kRecUsers * A.hs;                   // [4 waves][16 registers][64 lanes]
  const int G = K.G;
  float *zlo_s = dump_all + 4 * 16 * 64;                              // [G][128] per target and row: the band,
  float *zhi_s = zlo_s + (size_t)G * kRecUsers;
  u64 *key_s = reinterpret_cast<u64 *>(zhi_s + (size_t)G * kRecUsers);  //                        the target's key
  int *cnt_s = reinterpret_cast<int *>(key_s + (size_t)G * kRecUsers);  // [G][2 halves][128]     and the lane's running count
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x, sp = blockIdx.y;
  const int r0 = tile * kRecUsers;
  rank_load_q(A, h_s, tid, r0);
  __syncthreads();
  if (r0 + wave * 32 >= A.R) return;                                  // (no row in this wave; no barrier below)

  float *dump = dump_all + wave * (16 * 64);
  const int ul = wave * 32 + col, r = r0 + ul;
  const int i_begin = sp * A.ips, i_end = (int)min((int64_t)A.N, (int64_t)i_begin + A.ips);
  const int nblocks = (int)(((int64_t)i_end - i_begin + kRecItems - 1) / kRecItems);
  const float *hrow = h_s + (size_t)ul * A.hs + 4 * hh;
  int64_t beg, end;
  rankl_row(K, r, A.R, beg, end);
  int longest = (int)min(end - beg, (int64_t)0x7FFFFFFF);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) longest = max(longest, __shfl_xor(longest, m, kWave));
  longest = __builtin_amdgcn_readfirstlane(longest);

  f32x16 acc[4];
  float4 a0[4][kRecKT], a1[4][kRecKT];
  for (int g0 = 0; g0 < longest; g0 += G) {                           // wave-uniform: one walk per G targets of the longest row
    const int gw = min(G, longest - g0);
    float zmin = INFINITY;                                            // the row's lowest zlo: below it nothing is counted for any target
    for (int g = 0; g < gw; ++g) {
      const int64_t p = beg + g0 + g;
      u64 tkey = 0ull;
      float zlo = INFINITY, zhi = INFINITY;                           // (no target: nothing is counted)
      if (p < end) {
        tkey = K.tkey[p - K.base];
        if (tkey != 0ull) E::band(K.tz[p - K.base], key_score(tkey), zlo, zhi);
      }
      if (hh == 0) { zlo_s[g * kRecUsers + ul] = zlo; zhi_s[g * kRecUsers + ul] = zhi; key_s[g * kRecUsers + ul] = tkey; }
      cnt_s[(2 * g + hh) * kRecUsers + ul] = 0;
      zmin = fminf(zmin, zlo);
    }
    int64_t xc = 0, xhi = 0;                                          // the cursor into the user's exclusion row, its end
    if (A.xptr && beg + g0 < end) {
      const int u = A.uid[r];
      int64_t lo = A.xptr[u];
      const int64_t xend = A.xptr[u + 1];
      xhi = xend;
      int64_t hi = xend;
      while (lo < hi) {                                               // the first entry at or behind the split's first item
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (A.xidx[mid] < i_begin) lo = mid + 1; else hi = mid;
      }
      xc = lo;
    }
    wave_lds_sync();

    rec_load_a(A, i_begin, 0, col, hh, a0);
    for (int blk = 0; blk < nblocks; ++blk) {
      const int item0 = i_begin + blk * kRecItems;
      u64 xm = 0ull;                                                  // the excluded items of the block in this lane's half (as k_rank_count)
      while (xc < xhi) {
        const unsigned off = (unsigned)A.xidx[xc] - (unsigned)item0;
        if (off >= (unsigned)kRecItems) break;
        ++xc;
        if (((off >> 2) & 1u) == (unsigned)hh) xm |= 1ull << (16u * (off >> 5) + 4u * ((off & 31u) >> 3) + (off & 3u));
      }
      rank_block<E>(A, item0, blk + 1 < nblocks ? item0 + kRecItems : item0, col, hh, hrow, a0, a1, acc);
      const bool whole = (unsigned)item0 + (unsigned)kRecItems <= (unsigned)i_end;   // wave-uniform: every block but the split's last
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        uint32_t m0 = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) m0 |= (acc[s][e] >= zmin) ? (1u << e) : 0u;
        if (!__ballot(m0 != 0)) continue;                             // zlo <= zhi: a score below every zlo is ahead of no target
        const unsigned tile0 = (unsigned)item0 + 32u * s, ibase = tile0 + 4u * hh;
        uint32_t keep = 0xFFFFu;
        if (!whole) {
          keep = 0;
#pragma unroll
          for (int e = 0; e < 16; ++e) keep |= (ibase + 8u * (e >> 2) + (e & 3) < (unsigned)i_end) ? (1u << e) : 0u;
        }
        keep &= ~(uint32_t)((xm >> (16 * s)) & 0xFFFFull);
        bool dumped = false;                                          // wave-uniform
        for (int g = 0; g < gw; ++g) {
          const float zlo = zlo_s[g * kRecUsers + ul], zhi = zhi_s[g * kRecUsers + ul];
          const u64 tkey = key_s[g * kRecUsers + ul];
          uint32_t ma = 0, mb = 0;
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const float z = acc[s][e];
            ma |= (z > zhi) ? (1u << e) : 0u;
            mb |= (z >= zlo && z <= zhi) ? (1u << e) : 0u;
          }
          const unsigned t = (unsigned)tkey, tm = t & 31u;
          uint32_t kg = keep;
          if (tkey != 0ull && (t & ~31u) == tile0 && ((tm >> 2) & 1u) == (unsigned)hh) kg &= ~(1u << (4u * (tm >> 3) + (tm & 3u)));   // i != t
          ma &= kg;
          mb &= kg;
          int c = __popc(ma);
          if (__ballot(mb != 0)) {                                    // the band: rare unless many items tie with the target
            if (!dumped) {
#pragma unroll
              for (int e = 0; e < 16; ++e) dump[e * 64 + lane] = acc[s][e];   // (a lane reads back its own words only)
              dumped = true;
            }
            while (mb != 0) {
              const int e = __ffs(mb) - 1;
              mb &= mb - 1;
              const unsigned item = ibase + 8u * (e >> 2) + (e & 3);
              const u64 key = make_key(E::score(dump[e * 64 + lane]), item);
              c += key > tkey ? 1 : 0;
            }
          }
          cnt_s[(2 * g + hh) * kRecUsers + ul] += c;
        }
      }
    }
    for (int g = 0; g < gw; ++g) {
      const int64_t p = beg + g0 + g;
      if (p < end) K.partial[(size_t)(p - K.base) * (2 * A.splits) + 2 * sp + hh] = cnt_s[(2 * g + hh) * kRecUsers + ul];
    }
    wave_lds_sync();                                                  // (the next group's thresholds overwrite what the other half read)
  }
}

__global__ __launch_bounds__(kBlock) void k_rankl_finish(const int *__restrict__ partial, const u64 *__restrict__ tkey, int64_t base, int64_t P,
                                                         int splits, int32_t *__restrict__ out_rank, float *__restrict__ out_score) {
  const int64_t pi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (pi >= P) return;
  const u64 key = tkey[pi];
  if (key == 0ull) { out_rank[base + pi] = -1; out_score[base + pi] = -INFINITY; return; }
  const int *p = partial + (size_t)pi * (2 * splits);
  int sum = 0;
  for (int j = 0; j < 2 * splits; ++j) sum += p[j];
  out_rank[base + pi] = sum;
  out_score[base + pi] = key_score(key);
}

RankListArgs rankl_layout(Carver &cv, const RankPlan &P, int64_t n_targets) {
  RankListArgs K{};
  K.tz = cv.take<float>((size_t)n_targets);
  K.tkey = cv.take<u64>((size_t)n_targets);
  K.partial = cv.take<int>((size_t)n_targets * 2 * P.S.room);         // (room, not splits: n_items does not size it)
  return K;
}

// ---- scores of given (query row, table row) pairs and nothing else (drx_rows_pair_scores) -------------------------------------------
// out[p] = E::score(q[q_row[p], :] . table[t_row[p], :] (+ bias[t_row[p]])): two rows per pair, no walk, no scratch.  The sum is the
// one k_recommend / k_rank_keys build for the same rows, written out as ONE fmaf chain per pair: from 0.0f, the columns in steps of 8,
// within a step in the order 0, 4, 1, 5, 2, 6, 3, 7 (MFMA (t, c) adds k = 8 t + c from lanes 0..31, then k = 8 t + 4 + c from lanes
// 32..63), steps that begin behind ld skipped, and in a half-covered last step (ld % 8 == 4) the row's last float4 once more against
// ZERO query entries (what rec_load_a's clamp and the zeroed LDS columns multiply); then the bias, then the epilogue.
// k_pair_scores  one wave per workgroup, a lane owns a pair (the chain is sequential in k).  The rows do not reach the lanes by 64
//                strided loads: per chunk of 32 columns (a 128-byte line of a row) 8 lanes load one pair's line as float4, 8 pairs per
//                instruction, into registers and from there into LDS [pair][32 + 4] (the + 4 spreads a lane's float4 reads over the
//                banks); the lane then reads its own pair's chunk.  The registers of chunk kc + 1 load while chunk kc multiplies.
//                Pairs sorted by user give a wave one or two distinct query rows: those loads fall into the same lines (L1).
constexpr int kPairKC = 32;                // columns of a chunk
constexpr int kPairLs = kPairKC + 4;       // floats between two pairs' chunks in LDS
constexpr int kPairMaxGroups = 1 << 20;    // workgroups of a launch; a workgroup strides over the pairs beyond

struct PairArgs {
  const float *table, *bias, *q;   // [n_rows][ld], [n_rows] or null, [n_q][ld]
  const int32_t *q_row, *t_row;    // [P]
  float *out;                      // [P]
  int n_rows, n_q, ld;
  int64_t P;
};

// chunk kc of the 64 rows `myrow` (one per lane, inside the array): instruction j = rows 8 j .. 8 j + 7, 8 lanes of 16 bytes per row.
// kZeroBehind: columns behind ld are ZERO (the query side); else they repeat the row's last float4 (the table side, as rec_load_a).
template <bool kZeroBehind>
__device__ __forceinline__ void pair_load(const float *base, int ld, int myrow, int kc, int lane, float4 (&r)[8]) {
  const int c = kc * kPairKC + 4 * (lane & 7);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = __shfl(myrow, 8 * j + (lane >> 3), kWave);
    float4 v = *reinterpret_cast<const float4 *>(base + (size_t)row * ld + min(c, ld - 4));   // (no branch around a load)
    if (kZeroBehind && c >= ld) v.x = v.y = v.z = v.w = 0.f;
    r[j] = v;
  }
}

__device__ __forceinline__ void pair_stage(float *s, int lane, const float4 (&r)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) *reinterpret_cast<float4 *>(s + (8 * j + (lane >> 3)) * kPairLs + 4 * (lane & 7)) = r[j];
}

template <class E>
__global__ __launch_bounds__(kWave) void k_pair_scores(PairArgs A) {
  __shared__ __align__(16) float t_s[kWave * kPairLs], q_s[kWave * kPairLs];
  const int lane = threadIdx.x;
  const int nch = (A.ld + kPairKC - 1) / kPairKC;
  for (int64_t p0 = (int64_t)blockIdx.x * kWave; p0 < A.P; p0 += (int64_t)gridDim.x * kWave) {
    const int64_t p = p0 + lane;
    int tr = 0, qr = 0;
    bool valid = false;
    if (p < A.P) {
      const int t = A.t_row[p], u = A.q_row[p];
      valid = (unsigned)t < (unsigned)A.n_rows && (unsigned)u < (unsigned)A.n_q;
      if (valid) { tr = t; qr = u; }                                  // (else row 0 of both: loaded, never looked at)
    }
    float4 rt[8], rq[8];
    pair_load<false>(A.table, A.ld, tr, 0, lane, rt);
    pair_load<true>(A.q, A.ld, qr, 0, lane, rq);
    float acc = 0.0f;
    for (int kc = 0; kc < nch; ++kc) {
      pair_stage(t_s, lane, rt);
      pair_stage(q_s, lane, rq);
      __syncthreads();
      if (kc + 1 < nch) {
        pair_load<false>(A.table, A.ld, tr, kc + 1, lane, rt);
        pair_load<true>(A.q, A.ld, qr, kc + 1, lane, rq);
      }
      const float *a = t_s + lane * kPairLs, *b = q_s + lane * kPairLs;
#pragma unroll
      for (int s = 0; s < kPairKC / 8; ++s) {
        if (kc * kPairKC + 8 * s < A.ld) {                            // wave-uniform: k steps behind the row are skipped
          const float4 a0 = *reinterpret_cast<const float4 *>(a + 8 * s), a1 = *reinterpret_cast<const float4 *>(a + 8 * s + 4);
          const float4 b0 = *reinterpret_cast<const float4 *>(b + 8 * s), b1 = *reinterpret_cast<const float4 *>(b + 8 * s + 4);
          acc = fmaf(a0.x, b0.x, acc); acc = fmaf(a1.x, b1.x, acc);
          acc = fmaf(a0.y, b0.y, acc); acc = fmaf(a1.y, b1.y, acc);
          acc = fmaf(a0.z, b0.z, acc); acc = fmaf(a1.z, b1.z, acc);
          acc = fmaf(a0.w, b0.w, acc); acc = fmaf(a1.w, b1.w, acc);
        }
      }
      __syncthreads();
    }
    if (p < A.P) {
      float sc = -INFINITY;
      if (valid) {
        if constexpr (E::kBias) acc += A.bias[tr];
        sc = E::score(acc);
        if (sc == 0.0f) sc = 0.0f;                                    // (-0.0 == 0.0, as the keys of the other entry points carry it)
      }
      A.out[p] = sc;
    }
  }
}

}  // namespace
}  // namespace drx

using namespace drx;

extern "C" int drx_rows_pair_scores(const float *table, const float *bias, int32_t n_rows, int32_t ld, int32_t epilogue, const float *q,
                                    int32_t n_q, const int32_t *q_row, const int32_t *t_row, int64_t P, float *out_score, void *stream) {
  if (!epilogue_ok(epilogue, bias) || !ld_ok(ld) || P < 0) return DRX_EINVAL;
  if (P == 0) return DRX_OK;
  if (!table || !q || !q_row || !t_row || !out_score || n_rows < 1 || n_q < 1) return DRX_EINVAL;
  PairArgs A;
  A.table = table; A.bias = bias; A.q = q; A.q_row = q_row; A.t_row = t_row; A.out = out_score;
  A.n_rows = n_rows; A.n_q = n_q; A.ld = ld; A.P = P;
  const int64_t groups = (P + kWave - 1) / kWave;
  return by_epilogue(epilogue, [&](auto e) -> int {
    hipLaunchKernelGGL(k_pair_scores<decltype(e)>, dim3((unsigned)(groups < kPairMaxGroups ? groups : kPairMaxGroups)), dim3(kWave), 0,
                       (hipStream_t)stream, A);
    DRX_LAUNCH_CHECK();
    return DRX_OK;
  });
}

extern "C" size_t drx_rows_recommend_scratch_bytes(int32_t R, int32_t n_items, int32_t ld, int32_t n) {
  return rec_scratch_bytes(R, n_items, ld, n);
}

extern "C" int drx_rows_recommend(const float *table, const float *bias, int32_t n_items, int32_t ld, int32_t epilogue, const float *q,
                                  const int32_t *uid, int32_t R, int32_t n, const int64_t *excl_indptr, const int32_t *excl_indices,
                                  int32_t *out_idx, float *out_val, void *scratch, size_t scratch_bytes, void *stream) {
  return rec_run({table, bias, n_items, ld, epilogue, q, uid, R, excl_indptr, excl_indices}, n, out_idx, out_val, scratch, scratch_bytes, stream);
}

extern "C" size_t drx_cdae_recommend_scratch_bytes(int32_t R, int32_t n_items, int32_t ld, int32_t n) {
  return rec_scratch_bytes(R, n_items, ld, n);
}

extern "C" int drx_cdae_recommend(const DrxCdaeParams *p, const float *h, const int32_t *uid, int32_t R, int32_t n,
                                  const int64_t *excl_indptr, const int32_t *excl_indices, int32_t *out_idx, float *out_val,
                                  void *scratch, size_t scratch_bytes, void *stream) {
  if (!p || !p->W2T || !p->b2) return DRX_EINVAL;
  return rec_run({p->W2T, p->b2, p->n_items, p->ld, DRX_REC_SIGMOID_BIAS, h, uid, R, excl_indptr, excl_indices}, n, out_idx, out_val, scratch,
                 scratch_bytes, stream);
}

extern "C" size_t drx_rows_rank_items_scratch_bytes(int32_t R, int32_t n_items, int32_t ld) {
  RankPlan P;
  if (!rank_plan(R, n_items, ld, P)) return 0;
  Carver cv(nullptr, 0);
  (void)rank_layout(cv, P, R);
  return align_up(cv.off, 256) + 256;
}

extern "C" int drx_rows_rank_items(const float *table, const float *bias, int32_t n_items, int32_t ld, int32_t epilogue, const float *q,
                                   const int32_t *uid, const int32_t *target, int32_t R, const int64_t *excl_indptr,
                                   const int32_t *excl_indices, int32_t *out_rank, float *out_score, void *scratch, size_t scratch_bytes,
                                   void *stream) {
  const RecRequest Q{table, bias, n_items, ld, epilogue, q, uid, R, excl_indptr, excl_indices};
  if (!request_ok(Q) || !target || !out_rank || !out_score) return DRX_EINVAL;
  RankPlan P;
  if (!rank_plan(R, n_items, ld, P)) return DRX_ENOTIMPL;         // rows wider than 256 floats
  if (!scratch) return DRX_ESCRATCH;
  Carver cv(scratch, scratch_bytes);
  RankArgs K = rank_layout(cv, P, R);
  if (!cv.ok()) return DRX_ESCRATCH;
  K.target = target;
  const RecArgs A = rec_args(Q, P.W, P.S.count, P.S.per);
  hipStream_t st = (hipStream_t)stream;
  return by_epilogue(epilogue, [&](auto e) -> int {
    using E = decltype(e);
    DRX_HIP(hipFuncSetAttribute((const void *)k_rank_keys<E>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.W.lds));
    hipLaunchKernelGGL(k_rank_keys<E>, dim3(P.W.tiles), dim3(256), P.W.lds, st, A, K);
    DRX_HIP(hipFuncSetAttribute((const void *)k_rank_count<E>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.W.lds));
    hipLaunchKernelGGL(k_rank_count<E>, dim3(P.W.tiles, P.S.count), dim3(256), P.W.lds, st, A, K);
    hipLaunchKernelGGL(k_rank_finish, dim3((R + kBlock - 1) / kBlock), dim3(kBlock), 0, st, K.partial, K.tkey, R, P.S.count, out_rank, out_score);
    DRX_LAUNCH_CHECK();
    return DRX_OK;
  });
}

// G: what LDS holds beside the tile's query rows and the dump at this ld
extern "C" int32_t drx_rows_rank_lists_group(int32_t ld) {
  WalkPlan W;
  if (!walk_plan(1, 1, ld, W) || W.lds + kRankListSlot > kRecLdsBytes) return 0;
  const size_t g = (kRecLdsBytes - W.lds) / kRankListSlot;
  return g > (size_t)kRankListMaxG ? kRankListMaxG : (int)g;
}

extern "C" size_t drx_rows_rank_lists_scratch_bytes(int32_t R, int64_t n_targets, int32_t n_items, int32_t ld) {
  RankPlan P;
  if (n_targets < 0 || !rank_plan(R, n_items, ld, P) || drx_rows_rank_lists_group(ld) < 1) return 0;
  Carver cv(nullptr, 0);
  (void)rankl_layout(cv, P, n_targets);
  return align_up(cv.off, 256) + 256;
}

extern "C" int drx_rows_rank_lists(const float *table, const float *bias, int32_t n_items, int32_t ld, int32_t epilogue, const float *q,
                                   const int32_t *uid, int32_t R, const int64_t *target_indptr, const int32_t *targets,
                                   const int64_t *excl_indptr, const int32_t *excl_indices, int32_t *out_rank, float *out_score,
                                   void *scratch, size_t scratch_bytes, void *stream) {
  const RecRequest Q{table, bias, n_items, ld, epilogue, q, uid, R, excl_indptr, excl_indices};
  if (!request_ok(Q) || !target_indptr || !targets || !out_rank || !out_score) return DRX_EINVAL;
  RankPlan P;
  const int G = drx_rows_rank_lists_group(ld);
  if (!rank_plan(R, n_items, ld, P) || G < 1) return DRX_ENOTIMPL;   // rows wider than 256 floats
  hipStream_t st = (hipStream_t)stream;
  int64_t ends[2] = {0, 0};                                           // the offsets are device data: the two that size the call come back
  DRX_HIP(hipMemcpyAsync(&ends[0], target_indptr, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  DRX_HIP(hipMemcpyAsync(&ends[1], target_indptr + R, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  DRX_HIP(hipStreamSynchronize(st));
  const int64_t n_targets = ends[1] - ends[0];
  if (ends[0] < 0 || n_targets < 0 || n_targets > ((int64_t)1 << 40)) return DRX_EINVAL;
  if (n_targets == 0) return DRX_OK;
  if (!scratch || scratch_bytes < drx_rows_rank_lists_scratch_bytes(R, n_targets, n_items, ld)) return DRX_ESCRATCH;   // (to the byte)
  Carver cv(scratch, scratch_bytes);
  RankListArgs K = rankl_layout(cv, P, n_targets);
  if (!cv.ok()) return DRX_ESCRATCH;
  K.tptr = target_indptr; K.targets = targets; K.base = ends[0]; K.P = n_targets; K.G = G;
  const RecArgs A = rec_args(Q, P.W, P.S.count, P.S.per);
  const size_t lds_count = P.W.lds + (size_t)G * kRankListSlot;
  return by_epilogue(epilogue, [&](auto e) -> int {
    using E = decltype(e);
    DRX_HIP(hipFuncSetAttribute((const void *)k_rankl_keys<E>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.W.lds));
    hipLaunchKernelGGL(k_rankl_keys<E>, dim3(P.W.tiles), dim3(256), P.W.lds, st, A, K);
    DRX_HIP(hipFuncSetAttribute((const void *)k_rankl_count<E>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_count));
    hipLaunchKernelGGL(k_rankl_count<E>, dim3(P.W.tiles, P.S.count), dim3(256), lds_count, st, A, K);
    hipLaunchKernelGGL(k_rankl_finish, dim3((unsigned)((n_targets + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, K.partial, K.tkey, K.base,
                       K.P, P.S.count, out_rank, out_score);
    DRX_LAUNCH_CHECK();
    return DRX_OK;
  });
}
