// UserKNN / ItemKNN baselines (DRecPy/Recommender/Baseline): neighbour tables from co-rating sums on the matrix cores, and the
// predictions that walk them.  The arithmetic is stated in include/drx.h (drx_knn_*), the design in DESIGN.md section 3.6.
// k_knn_scatter   the CSR densified into X [R up to 128][C up to 8] fp32 in the scratch (zeroed before): one wave per row.
// k_knn_stats     per row, one thread, sequential double sums in CSR order: count, mean, sqrt(sum x^2), sqrt(sum (x - mean)^2).
// k_knn_tiles     grid (row tiles of 128, J splits).  As k_recommend (drx_recommend.hip): the J rows are the A operand, the I rows whose
//                 neighbours are sought the B operand of v_mfma_f32_32x32x2_f32, so a lane owns ONE row i (column = lane & 31) and 16
//                 rows j of a tile.  A wave owns 32 rows I and walks the split's J tiles; per tile the columns in steps of 8 (within
//                 a step 0, 4, 1, 5, 2, 6, 3, 7), one MFMA per sum the metric reads; M = (X != 0) and X^2 are made in registers.
//                 The epilogue runs in double, rounds to float32 once and makes the key (drx_keys.hpp).  Selection as the
//                 scorer-selector's: a lane's own list in the scratch, cut back to its k best by the whole wave at capacity.
// k_lists_merge   (drx_keys.hpp, with the lists' plan and layout) one workgroup per row: its 2 x splits lists ordered in LDS, the k
//                 largest out, -1 / 0.0 behind them.
// No [R, R] matrix, no atomic read-modify-write; a sum is the same fmaf chain whatever the split: a function of the inputs alone.
// k_knn_score_item / k_knn_score_user / k_knn_pair_scores   predictions for whole rows of R users / for given pairs.
#include <hip/hip_runtime.h>
#include "drx_keys.hpp"

#pragma clang fp contract(off)            // the CPU oracle states the epilogue as single operations: none may fuse here

namespace drx {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kKnnRows = kListRows;       // rows I of a workgroup: 32 per wave
constexpr int kKnnTile = 32;              // rows J of a tile
constexpr int kKnnMaxK = 128;
constexpr int kKnnTargetGroups = 256;     // workgroups a launch aims for: one per CU
constexpr size_t kKnnLdsBytes = 160 * 1024;

// the entries [lo, hi) of CSR row r, clamped into [0, nnz): whatever the offsets hold, no access leaves the arrays
__device__ __forceinline__ void knn_row(const int64_t *indptr, int64_t nnz, int r, int64_t &lo, int64_t &hi) {
  lo = min(max(indptr[r], (int64_t)0), nnz);
  hi = min(max(indptr[r + 1], lo), nnz);
}

__global__ __launch_bounds__(kBlock) void k_knn_scatter(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                        const float *__restrict__ values, int64_t nnz, int R, int C, int Cp,
                                                        float *__restrict__ X) {
  const int r = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  int64_t lo, hi;
  knn_row(indptr, nnz, r, lo, hi);
  for (int64_t p = lo + lane; p < hi; p += kWave) {
    const int c = indices[p];
    if ((unsigned)c < (unsigned)C) X[(size_t)r * Cp + c] = values[p];
  }
}

struct KnnStats {
  int32_t *cnt;                  // [R] non-zero entries of the row
  double *mean, *norm, *cnorm;   // [R] their mean, sqrt(sum x^2), sqrt(sum (x - mean)^2)
};

__global__ __launch_bounds__(kBlock) void k_knn_stats(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                      const float *__restrict__ values, int64_t nnz, int R, int C, KnnStats S) {
  const int r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= R) return;
  int64_t lo, hi;
  knn_row(indptr, nnz, r, lo, hi);
  int cnt = 0;
  double sum = 0.0, full2 = 0.0, c2 = 0.0;
  for (int64_t p = lo; p < hi; ++p) {
    const double v = (double)values[p];
    if (v == 0.0 || (unsigned)indices[p] >= (unsigned)C) continue;      // (what the dense X does not hold)
    ++cnt;
    sum = sum + v;
    full2 = full2 + v * v;
  }
  const double mean = cnt > 0 ? sum / (double)cnt : 0.0;
  for (int64_t p = lo; p < hi; ++p) {
    const double v = (double)values[p];
    if (v == 0.0 || (unsigned)indices[p] >= (unsigned)C) continue;
    const double d = v - mean;
    c2 = c2 + d * d;
  }
  S.cnt[r] = cnt;
  S.mean[r] = mean;
  S.norm[r] = sqrt(full2);
  S.cnorm[r] = sqrt(c2);
}

__global__ __launch_bounds__(kBlock) void k_knn_row_means(const int64_t *__restrict__ indptr, const float *__restrict__ values, int64_t nnz,
                                                          int R, double *__restrict__ out) {
  const int r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= R) return;
  int64_t lo, hi;
  knn_row(indptr, nnz, r, lo, hi);
  double sum = 0.0;
  for (int64_t p = lo; p < hi; ++p) sum = sum + (double)values[p];
  out[r] = hi > lo ? sum / (double)(hi - lo) : 0.0;
}

struct KnnArgs {
  const float *X;                // [Rp][Cp], zero behind R and behind C
  KnnStats S;
  int R, Cp;
  int k, cap, m;
  double shrink, md2;            // shrinkage (negative: none), max_diff^2
  int splits, jps;               // J splits, J tiles per split
  u64 *lists;                    // [tiles][splits][128][2][cap]
  int *counts;                   // [tiles][splits][128][2]
};

// which sums a metric reads (the others are never accumulated)
template <int M> struct KnnSums {
  static constexpr bool xy = M != DRX_KNN_JACCARD;
  static constexpr bool s1 = M == DRX_KNN_ADJUSTED_COSINE || M == DRX_KNN_PEARSON;                       // Sx, Sy
  static constexpr bool s2 = M == DRX_KNN_COSINE_CF || M == DRX_KNN_MSD || M == DRX_KNN_PEARSON;          // Sxx, Syy
};

// The similarity of rows i (the lane's own: ci, mi, di its count, mean and norm) and j as a float32, 0 where the pair is dropped.
// Sums named from row i's side: si = sum of x_i over the common columns, sj of x_j, sii / sjj of the squares.  x is the row with the
// SMALLER id (the reference walks i <= j and stores one value for both), so sim(i, j) == sim(j, i) bit for bit.
template <int M>
__device__ __forceinline__ float knn_sim(const KnnArgs &A, int i, int j, int ci, double mi, double di, float fn, float fxy, float fsi, float fsj,
                                         float fsii, float fsjj) {
  if (!(fn > 0.0f)) return 0.0f;
  if (A.m > 0 && fn < (float)A.m) return 0.0f;
  const double n = (double)fn, Sxy = (double)fxy;
  const bool ilo = i < j;
  const double Sx = (double)(ilo ? fsi : fsj), Sy = (double)(ilo ? fsj : fsi);
  const double Sxx = (double)(ilo ? fsii : fsjj), Syy = (double)(ilo ? fsjj : fsii);
  double s;
  if constexpr (M == DRX_KNN_COSINE) {
    const double den = di * A.S.norm[j];
    if (den == 0.0) return 0.0f;
    s = Sxy / den;
  } else if constexpr (M == DRX_KNN_ADJUSTED_COSINE) {
    const double mj = A.S.mean[j];
    const double ma = ilo ? mi : mj, mb = ilo ? mj : mi;
    const double den = di * A.S.cnorm[j];
    if (den == 0.0) return 0.0f;                 // a row without spread: the reference's normalisation leaves it at 0
    double t = Sxy - mb * Sx;
    t = t - ma * Sy;
    t = t + (n * ma) * mb;
    s = t / den;
  } else if constexpr (M == DRX_KNN_COSINE_CF) {
    if (Sxy == 0.0) return 0.0f;
    s = Sxy / (sqrt(Sxx) * sqrt(Syy));
  } else if constexpr (M == DRX_KNN_JACCARD) {
    s = n / (((double)ci + (double)A.S.cnt[j]) - n);
  } else if constexpr (M == DRX_KNN_MSD) {
    s = 1.0 - (((Sxx + Syy) - 2.0 * Sxy) / A.md2) / n;
  } else {
    const double vx = Sxx - (Sx * Sx) / n, vy = Syy - (Sy * Sy) / n;
    if (!(vx > 0.0) || !(vy > 0.0)) return 0.0f;  // (== 0 for exact sums; rounded sums may land a hair below)
    s = (Sxy - (Sx * Sy) / n) / (sqrt(vx) * sqrt(vy));
  }
  if (A.shrink >= 0.0) s = s * (n / ((n + A.shrink) + 1e-6));
  const float f = (float)s;
  return f > 0.0f ? f : 0.0f;                    // (a NaN is dropped too)
}

// (rec_compact of drx_recommend.hip without exclusions) the list of lane L (wave-uniform) cut back to its k best by the whole wave
__device__ __forceinline__ void knn_compact(const KnnArgs &A, u64 *wave_lists, u64 *cb, int L, int lane, int &cnt, u64 &tkey) {
  const int cL = __shfl(cnt, L, kWave);
  u64 *list = wave_lists + (size_t)(2 * (L & 31) + (L >> 5)) * A.cap;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  u64 k[4];
  int rank[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = lane + 64 * j;
    k[j] = i < cL ? __hip_atomic_load(list + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    cb[i] = k[j];
    rank[j] = 0;
  }
  wave_lds_sync();
  for (int i = 0; i < cL; ++i) {
    const u64 o = cb[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) rank[j] += o > k[j] ? 1 : 0;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (k[j] != 0ull && rank[j] < A.k) list[rank[j]] = k[j];          // (keys are unique: the ranks are 0 .. cL - 1)
    if (k[j] != 0ull && rank[j] == A.k - 1) cb[256] = k[j];
  }
  wave_lds_sync();
  const u64 kth = cb[256];
  if (lane == L) {
    if (cL >= A.k) tkey = kth;
    cnt = min(cL, A.k);
  }
  wave_lds_sync();
}

template <int M>
__global__ __launch_bounds__(256) void k_knn_tiles(KnnArgs A) {
  __shared__ float dump_all[4 * 16 * 64];                             // [4 waves][16 registers][64 lanes]
  __shared__ u64 cb_all[4 * 258];                                     // [4 waves][256 keys + the k-th + pad]
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x, sp = blockIdx.y;
  const int i0 = tile * kKnnRows + wave * 32;
  if (i0 >= A.R) return;                                              // (no row in this wave; no workgroup barrier anywhere below)
  float *dump = dump_all + wave * (16 * 64);
  u64 *cb = cb_all + wave * 258;
  const int i = i0 + col;
  const bool ivalid = i < A.R;
  int ci = 0;
  double mi = 0.0, di = 0.0;
  if (ivalid) {
    ci = A.S.cnt[i];
    mi = A.S.mean[i];
    di = M == DRX_KNN_ADJUSTED_COSINE ? A.S.cnorm[i] : A.S.norm[i];
  }
  const size_t group = (size_t)tile * A.splits + sp;
  u64 *wave_lists = A.lists + ((group * kKnnRows + wave * 32) * 2) * (size_t)A.cap;
  u64 *mylist = wave_lists + (size_t)(2 * col + hh) * A.cap;
  u64 tkey = ivalid ? 0ull : ~0ull;                                   // keys at or below it cannot enter the list
  int cnt = 0;

  const int jtiles = (A.R + kKnnTile - 1) / kKnnTile;
  const int t_begin = sp * A.jps, t_end = min(jtiles, t_begin + A.jps);
  const float *pb = A.X + (size_t)i * A.Cp + 4 * hh;                  // (rows behind R exist in X: zeros)
  for (int t = t_begin; t < t_end; ++t) {
    const int j0 = t * kKnnTile;
    const float *pa = A.X + (size_t)(j0 + col) * A.Cp + 4 * hh;
    f32x16 an, axy, asi, asj, asii, asjj;
#pragma unroll
    for (int e = 0; e < 16; ++e) an[e] = axy[e] = asi[e] = asj[e] = asii[e] = asjj[e] = 0.f;
    float4 a = *reinterpret_cast<const float4 *>(pa), b = *reinterpret_cast<const float4 *>(pb);
    for (int c = 0; c < A.Cp; c += 8) {
      const int cn = min(c + 8, A.Cp - 8);                            // the next step's fragments load while this one multiplies
      const float4 a1 = *reinterpret_cast<const float4 *>(pa + cn), b1 = *reinterpret_cast<const float4 *>(pb + cn);
      // column c + q (lanes 0..31) and c + 4 + q (lanes 32..63): xa of row j, xb of row i
#define DRX_KNN_STEP(xa, xb)                                                                           \
  {                                                                                                    \
    const float ma = (xa) != 0.f ? 1.f : 0.f, mb = (xb) != 0.f ? 1.f : 0.f;                            \
    an = __builtin_amdgcn_mfma_f32_32x32x2f32(ma, mb, an, 0, 0, 0);                                    \
    if constexpr (KnnSums<M>::xy) axy = __builtin_amdgcn_mfma_f32_32x32x2f32((xa), (xb), axy, 0, 0, 0); \
    if constexpr (KnnSums<M>::s1) {                                                                    \
      asi = __builtin_amdgcn_mfma_f32_32x32x2f32(ma, (xb), asi, 0, 0, 0);                              \
      asj = __builtin_amdgcn_mfma_f32_32x32x2f32((xa), mb, asj, 0, 0, 0);                              \
    }                                                                                                  \
    if constexpr (KnnSums<M>::s2) {                                                                    \
      asii = __builtin_amdgcn_mfma_f32_32x32x2f32(ma, (xb) * (xb), asii, 0, 0, 0);                     \
      asjj = __builtin_amdgcn_mfma_f32_32x32x2f32((xa) * (xa), mb, asjj, 0, 0, 0);                     \
    }                                                                                                  \
  }
      DRX_KNN_STEP(a.x, b.x)
      DRX_KNN_STEP(a.y, b.y)
      DRX_KNN_STEP(a.z, b.z)
      DRX_KNN_STEP(a.w, b.w)
#undef DRX_KNN_STEP
      a = a1;
      b = b1;
    }
    // register 4 g + q of the tile = row j0 + 8 g + 4 half + q
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = j0 + 8 * (e >> 2) + 4 * hh + (e & 3);
      float s = 0.0f;
      if (ivalid && j < A.R && j != i) s = knn_sim<M>(A, i, j, ci, mi, di, an[e], axy[e], asi[e], asj[e], asii[e], asjj[e]);
      dump[e * 64 + lane] = s;                                        // (a lane reads back its own words only)
    }
    for (int e = 0; e < 16; ++e) {
      const float s = dump[e * 64 + lane];
      if (s > 0.0f) {
        const unsigned j = (unsigned)(j0 + 8 * (e >> 2) + 4 * hh + (e & 3));
        const u64 key = make_key(s, j);
        if (key > tkey) { mylist[cnt] = key; ++cnt; }
      }
      u64 full = __ballot(cnt >= A.cap);
      while (full) {
        const int L = __ffsll((long long)full) - 1;
        full &= full - 1;
        knn_compact(A, wave_lists, cb, L, lane, cnt, tkey);
      }
    }
  }
  u64 over = __ballot(cnt > A.k);
  while (over) {
    const int L = __ffsll((long long)over) - 1;
    over &= over - 1;
    knn_compact(A, wave_lists, cb, L, lane, cnt, tkey);
  }
  if (ivalid) A.counts[(group * kKnnRows + (size_t)(wave * 32 + col)) * 2 + hh] = cnt;
}

struct KnnPlan {
  int Rp, Cp;                    // X's padded shape
  ListPlan L;                    // the lists of k keys, split over the tiles of 32 rows J
  float *X;                      // set by knn_layout()
  KnnStats S;
};

bool knn_plan(int R, int C, int k, int force_splits, KnnPlan &P) {
  if (R < 1 || C < 1 || k < 1 || k > kKnnMaxK || force_splits < 0) return false;
  if ((int64_t)R + kKnnRows > 0x7FFFFFFFll || (int64_t)C + 8 > 0x7FFFFFFFll) return false;
  const int tiles = (R + kKnnRows - 1) / kKnnRows;
  P.Rp = tiles * kKnnRows;
  P.Cp = (C + 7) / 8 * 8;
  P.L = list_plan(tiles, (R + kKnnTile - 1) / kKnnTile, k, kKnnTargetGroups, force_splits);
  return true;
}

void knn_layout(Carver &cv, KnnPlan &P, int R) {
  P.X = cv.take<float>((size_t)P.Rp * P.Cp);
  P.S.cnt = cv.take<int32_t>((size_t)R);
  P.S.mean = cv.take<double>((size_t)R);
  P.S.norm = cv.take<double>((size_t)R);
  P.S.cnorm = cv.take<double>((size_t)R);
  P.L.carve(cv);
}

size_t knn_scratch_bytes(int R, int C, int k, int force_splits) {
  KnnPlan P;
  if (!knn_plan(R, C, k, force_splits, P)) return 0;
  Carver cv(nullptr, 0);
  knn_layout(cv, P, R);
  return align_up(cv.off, 256) + 256;
}

template <int M>
int knn_launch(const KnnArgs &A, const KnnPlan &P, int32_t *out_idx, float *out_sim, hipStream_t st) {
  hipLaunchKernelGGL(k_knn_tiles<M>, dim3(P.L.tiles, P.L.splits), dim3(256), 0, st, A);
  return lists_merge(P.L, A.R, 0.0f, out_idx, out_sim, st);
}

int knn_run(const int64_t *indptr, const int32_t *indices, const float *values, int64_t nnz, int R, int C, int metric, int k, int m,
            double shrinkage, double max_diff, int force_splits, int32_t *out_idx, float *out_sim, void *scratch, size_t scratch_bytes,
            void *stream) {
  if (metric < DRX_KNN_COSINE || metric > DRX_KNN_PEARSON || k < 1 || k > kKnnMaxK || m < 0 || R < 0 || C < 1 || nnz < 0 || force_splits < 0)
    return DRX_EINVAL;
  if (shrinkage != shrinkage || (metric == DRX_KNN_MSD && !(max_diff > 0.0))) return DRX_EINVAL;
  if (R == 0) return DRX_OK;
  if (!indptr || !out_idx || !out_sim || (nnz > 0 && (!indices || !values))) return DRX_EINVAL;
  KnnPlan P;
  if (!knn_plan(R, C, k, force_splits, P)) return DRX_EINVAL;
  if (!scratch) return DRX_ESCRATCH;
  Carver cv(scratch, scratch_bytes);
  knn_layout(cv, P, R);
  if (!cv.ok()) return DRX_ESCRATCH;
  hipStream_t st = (hipStream_t)stream;
  DRX_HIP(hipMemsetAsync(P.X, 0, (size_t)P.Rp * P.Cp * sizeof(float), st));
  hipLaunchKernelGGL(k_knn_scatter, dim3((R + 3) / 4), dim3(kBlock), 0, st, indptr, indices, values, nnz, R, C, P.Cp, P.X);
  hipLaunchKernelGGL(k_knn_stats, dim3((R + kBlock - 1) / kBlock), dim3(kBlock), 0, st, indptr, indices, values, nnz, R, C, P.S);
  KnnArgs A;
  A.X = P.X; A.S = P.S; A.R = R; A.Cp = P.Cp; A.k = k; A.cap = P.L.cap; A.m = m; A.shrink = shrinkage < 0.0 ? -1.0 : shrinkage;
  A.md2 = max_diff * max_diff; A.splits = P.L.splits; A.jps = P.L.per; A.lists = P.L.lists; A.counts = P.L.counts;
  switch (metric) {
    case DRX_KNN_COSINE: return knn_launch<DRX_KNN_COSINE>(A, P, out_idx, out_sim, st);
    case DRX_KNN_ADJUSTED_COSINE: return knn_launch<DRX_KNN_ADJUSTED_COSINE>(A, P, out_idx, out_sim, st);
    case DRX_KNN_COSINE_CF: return knn_launch<DRX_KNN_COSINE_CF>(A, P, out_idx, out_sim, st);
    case DRX_KNN_JACCARD: return knn_launch<DRX_KNN_JACCARD>(A, P, out_idx, out_sim, st);
    case DRX_KNN_MSD: return knn_launch<DRX_KNN_MSD>(A, P, out_idx, out_sim, st);
    default: return knn_launch<DRX_KNN_PEARSON>(A, P, out_idx, out_sim, st);
  }
}

// ---- predictions -------------------------------------------------------------------------------------------------------------------
// One aggregation for every entry point: the terms in neighbour-list order, double, single operations.
//   weighted mean   num += s * r, den += s          mean   num += r, den += 1          prediction = num / den, none when den == 0
struct KnnModel {
  const int64_t *indptr;         // user-major CSR [n_users + 1], columns ascending
  const int32_t *indices;
  const float *values;
  int64_t nnz;
  int n_users, n_items;
  const int32_t *nb_idx;         // [n_users or n_items][k], -1 behind the last neighbour
  const float *nb_sim;
  int k, type, agg;
};

__device__ __forceinline__ void knn_term(int agg, double s, double r, double &num, double &den) {
  if (agg == DRX_KNN_WEIGHTED_MEAN) {
    num = num + s * r;
    den = den + s;
  } else {
    num = num + r;
    den = den + 1.0;
  }
}

__device__ __forceinline__ void knn_clear_bit(uint32_t *mask, size_t flat) {
  if (!mask) return;
  const uint32_t bit = 1u << (flat & 31);
  if (mask[flat >> 5] & bit) atomicAnd(mask + (flat >> 5), ~bit);     // (words are shared between rows; clearing commutes)
}

// ItemKNN: the user's ratings as a row [n_items] (NaN = none) in LDS, or in the scratch when it does not fit; a lane takes an item and
// walks its neighbours.
__device__ __forceinline__ void knn_item_ratings(const KnnModel &Mo, int u, float *row) {
  const int N = Mo.n_items;
  for (int i = threadIdx.x; i < N; i += kBlock) row[i] = __uint_as_float(0x7FC00000u);
  __syncthreads();
  if ((unsigned)u < (unsigned)Mo.n_users) {
    int64_t lo, hi;
    knn_row(Mo.indptr, Mo.nnz, u, lo, hi);
    for (int64_t p = lo + threadIdx.x; p < hi; p += kBlock) {
      const int c = Mo.indices[p];
      if ((unsigned)c < (unsigned)N) row[c] = Mo.values[p];
    }
  }
  __syncthreads();
}

// the prediction of item i from the ratings row (0 and false where there is none)
__device__ __forceinline__ bool knn_item_predict(const KnnModel &Mo, const float *row, int u, int i, const double *__restrict__ fallback,
                                                 float &pred) {
  const int N = Mo.n_items;
  double num = 0.0, den = 0.0;
  for (int t = 0; t < Mo.k; ++t) {
    const int j = Mo.nb_idx[(size_t)i * Mo.k + t];
    if (j < 0) break;
    if (j >= N) continue;
    const float v = row[j];
    if (v != v) continue;
    knn_term(Mo.agg, (double)Mo.nb_sim[(size_t)i * Mo.k + t], (double)v, num, den);
  }
  pred = 0.0f;
  if (den > 0.0) pred = (float)(num / den);
  else if (fallback && (unsigned)u < (unsigned)Mo.n_users) pred = (float)fallback[u];
  else return false;
  return true;
}

__global__ __launch_bounds__(kBlock) void k_knn_score_item(KnnModel Mo, const int32_t *__restrict__ uid, const double *__restrict__ fallback,
                                                           float *__restrict__ out, uint32_t *mask, float *rows) {
  extern __shared__ __align__(16) float knn_lds_f[];
  const int r = blockIdx.x, N = Mo.n_items;
  float *row = rows ? rows + (size_t)r * N : knn_lds_f;
  const int u = uid[r];
  knn_item_ratings(Mo, u, row);
  for (int i = threadIdx.x; i < N; i += kBlock) {
    float pred;
    if (!knn_item_predict(Mo, row, u, i, fallback, pred)) knn_clear_bit(mask, (size_t)r * N + i);
    out[(size_t)r * N + i] = pred;
  }
}

// UserKNN: the sums of every item [n_items][2] doubles in LDS (or the scratch); the neighbours' CSR rows one after another, a lane per
// entry — a row's columns are distinct, so no two lanes meet.
__device__ __forceinline__ void knn_user_sums(const KnnModel &Mo, int u, double *acc) {
  const int N = Mo.n_items;
  for (int i = threadIdx.x; i < 2 * N; i += kBlock) acc[i] = 0.0;
  __syncthreads();
  if ((unsigned)u < (unsigned)Mo.n_users) {
    for (int t = 0; t < Mo.k; ++t) {
      const int v = Mo.nb_idx[(size_t)u * Mo.k + t];                  // (uniform over the workgroup)
      if (v < 0) break;
      if (v >= Mo.n_users) continue;
      const double s = (double)Mo.nb_sim[(size_t)u * Mo.k + t];
      int64_t lo, hi;
      knn_row(Mo.indptr, Mo.nnz, v, lo, hi);
      for (int64_t p = lo + threadIdx.x; p < hi; p += kBlock) {
        const int c = Mo.indices[p];
        if ((unsigned)c < (unsigned)N) knn_term(Mo.agg, s, (double)Mo.values[p], acc[2 * c], acc[2 * c + 1]);
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ bool knn_user_predict(const double *acc, int i, float &pred) {
  const double num = acc[2 * i], den = acc[2 * i + 1];
  pred = 0.0f;
  if (!(den > 0.0)) return false;
  pred = (float)(num / den);
  return true;
}

__global__ __launch_bounds__(kBlock) void k_knn_score_user(KnnModel Mo, const int32_t *__restrict__ uid, float *__restrict__ out, uint32_t *mask,
                                                           double *rows) {
  extern __shared__ __align__(16) double knn_lds_d[];
  const int r = blockIdx.x, N = Mo.n_items;
  double *acc = rows ? rows + (size_t)r * 2 * N : knn_lds_d;
  knn_user_sums(Mo, uid[r], acc);
  for (int i = threadIdx.x; i < N; i += kBlock) {
    float pred;
    if (!knn_user_predict(acc, i, pred)) knn_clear_bit(mask, (size_t)r * N + i);
    out[(size_t)r * N + i] = pred;
  }
}

// the value of (row, column) in the ascending CSR row [lo, hi), found: whether there is one
__device__ __forceinline__ bool knn_lookup(const KnnModel &Mo, int64_t lo, int64_t hi, int c, float &v) {
  const int64_t end = hi;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (Mo.indices[mid] < c) lo = mid + 1; else hi = mid;
  }
  if (lo < end && Mo.indices[lo] == c) { v = Mo.values[lo]; return true; }
  return false;
}

__global__ __launch_bounds__(kBlock) void k_knn_pair_scores(KnnModel Mo, const int32_t *__restrict__ uid, const int32_t *__restrict__ iid, int64_t P,
                                                            const double *__restrict__ fallback, double *__restrict__ out,
                                                            uint8_t *__restrict__ none) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= P) return;
  const int u = uid[p], i = iid[p];
  double num = 0.0, den = 0.0;
  const bool known = (unsigned)u < (unsigned)Mo.n_users && (unsigned)i < (unsigned)Mo.n_items;
  if (known) {
    const bool user = Mo.type == DRX_KNN_USER;
    const size_t base = (size_t)(user ? u : i) * Mo.k;
    int64_t lo = 0, hi = 0;
    if (!user) knn_row(Mo.indptr, Mo.nnz, u, lo, hi);
    for (int t = 0; t < Mo.k; ++t) {
      const int nb = Mo.nb_idx[base + t];
      if (nb < 0) break;
      float v;
      if (user) {                                 // neighbour user nb: has it rated item i?
        if (nb >= Mo.n_users) continue;
        knn_row(Mo.indptr, Mo.nnz, nb, lo, hi);
        if (!knn_lookup(Mo, lo, hi, i, v)) continue;
      } else if (!knn_lookup(Mo, lo, hi, nb, v)) continue;             // neighbour item nb: has user u rated it?
      knn_term(Mo.agg, (double)Mo.nb_sim[base + t], (double)v, num, den);
    }
  }
  if (den > 0.0) { out[p] = num / den; none[p] = 0; }
  else if (known && fallback) { out[p] = fallback[Mo.type == DRX_KNN_USER ? i : u]; none[p] = 0; }
  else { out[p] = 0.0; none[p] = 1; }
}

bool knn_model_ok(const KnnModel &Mo) {
  if (Mo.type != DRX_KNN_USER && Mo.type != DRX_KNN_ITEM) return false;
  if (Mo.agg != DRX_KNN_MEAN && Mo.agg != DRX_KNN_WEIGHTED_MEAN) return false;
  if (Mo.n_users < 1 || Mo.n_items < 1 || Mo.k < 1 || Mo.k > kKnnMaxK || Mo.nnz < 0) return false;
  if (!Mo.indptr || !Mo.nb_idx || !Mo.nb_sim || (Mo.nnz > 0 && (!Mo.indices || !Mo.values))) return false;
  return true;
}

size_t knn_row_bytes(int type, int n_items) { return (size_t)n_items * (type == DRX_KNN_USER ? 2 * sizeof(double) : sizeof(float)); }

size_t knn_score_scratch_bytes(int type, int R, int n_items) {
  if (R < 1 || n_items < 1 || knn_row_bytes(type, n_items) <= kKnnLdsBytes) return 0;
  return align_up((size_t)R * knn_row_bytes(type, n_items), 256) + 256;
}

// ---- top-n and catalogue ranks where the row lies: no score matrix ----------------------------------------------------------------
// One workgroup per request row, as the score kernels, and their arithmetic (knn_item_predict / knn_user_predict).  The working row
// ends as KEYS: uint32 [n_items], the ordered bits of an item's float32 prediction, 0 where it has none (no float orders to 0).
//   ItemKNN   float ratings [n_items] | uint32 keys [n_items]                                     8 bytes an item
//   UserKNN   double sums [n_items][2], packed down IN PLACE to uint32 keys [n_items]            16 bytes an item
// in LDS while the row and the selection's kKnnFusedTail bytes fit kKnnLdsBytes, else in the scratch (one row per request row).
// An item's full key is (bits << 32 | item): unique, so "the n best" and "how many are ahead" have one answer, ties to the larger id.
constexpr size_t kKnnFusedTail = 64;      // [2][waves] wave maxima of k_knn_recommend, behind the row
constexpr int kKnnMaxTopN = 128;
constexpr int kKnnRankGroup = 4;          // targets a wave counts in one walk of the row

size_t knn_fused_row_bytes(int type, int n_items) { return (size_t)n_items * (type == DRX_KNN_USER ? 2 * sizeof(double) : 2 * sizeof(float)); }
bool knn_fused_in_lds(int type, int n_items) { return knn_fused_row_bytes(type, n_items) + kKnnFusedTail <= kKnnLdsBytes; }
size_t knn_fused_scratch_bytes(int type, int R, int n_items) {
  if (R < 1 || n_items < 1 || knn_fused_in_lds(type, n_items)) return 0;
  return align_up((size_t)R * knn_fused_row_bytes(type, n_items), 256) + 256;
}

__device__ __forceinline__ u64 knn_full_key(uint32_t bits, int i) { return bits ? ((u64)bits << 32) | (unsigned)i : 0ull; }

// The keys of user u's row in the working area ws (all threads; ends on a barrier).
template <int TYPE>
__device__ __forceinline__ uint32_t *knn_row_keys(const KnnModel &Mo, int u, const double *__restrict__ fallback, void *ws) {
  const int N = Mo.n_items;
  if constexpr (TYPE == DRX_KNN_ITEM) {
    float *row = (float *)ws;
    uint32_t *keys = (uint32_t *)(row + N);
    knn_item_ratings(Mo, u, row);
    for (int i = threadIdx.x; i < N; i += kBlock) {
      float pred;
      keys[i] = knn_item_predict(Mo, row, u, i, fallback, pred) ? ordered_bits(pred) : 0u;
    }
    __syncthreads();
    return keys;
  } else {
    double *acc = (double *)ws;
    uint32_t *keys = (uint32_t *)ws;
    knn_user_sums(Mo, u, acc);
    // key i lands on the sums of item i / 4, which this or an earlier round has read: a barrier between a round's reads and its writes
    for (int base = 0; base < N; base += kBlock) {
      const int i = base + (int)threadIdx.x;
      uint32_t key = 0u;
      float pred;
      if (i < N && knn_user_predict(acc, i, pred)) key = ordered_bits(pred);
      __syncthreads();
      if (i < N) keys[i] = key;
    }
    __syncthreads();
    return keys;
  }
}

// the exclusion row of user u, empty without a CSR or for a user outside the model
__device__ __forceinline__ void knn_excl_row(const int64_t *__restrict__ excl_indptr, int u, int n_users, int64_t &lo, int64_t &hi) {
  lo = hi = 0;
  if (!excl_indptr || (unsigned)u >= (unsigned)n_users) return;
  lo = excl_indptr[u];
  hi = excl_indptr[u + 1];
}

struct KnnFused {
  const int32_t *uid;
  const double *fallback;
  const int64_t *excl_indptr;
  const int32_t *excl_indices;
  unsigned char *rows;           // the working rows in the scratch, nullptr: LDS
  size_t row_bytes;
};

// The n best by rounds: every thread holds the largest full key of its own items (i = thread, thread + 256, ...) below the last key
// taken; a round is one maximum over the workgroup (shuffles within a wave, one LDS word a wave, one barrier), and only the thread
// whose key was taken looks through its items again.
template <int TYPE>
__global__ __launch_bounds__(kBlock) void k_knn_recommend(KnnModel Mo, KnnFused F, int n, int32_t *__restrict__ out_idx, float *__restrict__ out_val) {
  extern __shared__ __align__(16) unsigned char knn_lds_fused[];
  const int r = blockIdx.x, N = Mo.n_items, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int kWaves = kBlock / kWave;
  u64 *wmax = (u64 *)(knn_lds_fused + (F.rows ? 0 : F.row_bytes));
  const int u = F.uid[r];
  uint32_t *keys = knn_row_keys<TYPE>(Mo, u, F.fallback, F.rows ? (void *)(F.rows + (size_t)r * F.row_bytes) : (void *)knn_lds_fused);
  int64_t xlo, xhi;
  knn_excl_row(F.excl_indptr, u, Mo.n_users, xlo, xhi);
  for (int64_t p = xlo + tid; p < xhi; p += kBlock) {
    const int c = F.excl_indices[p];
    if ((unsigned)c < (unsigned)N) keys[c] = 0u;
  }
  __syncthreads();
  auto best_below = [&](u64 below) {
    u64 best = 0ull;
    for (int i = tid; i < N; i += kBlock) {
      const u64 key = knn_full_key(keys[i], i);
      if (key < below && key > best) best = key;
    }
    return best;
  };
  u64 cand = best_below(~0ull);
  int32_t *oi = out_idx + (size_t)r * n;
  float *ov = out_val + (size_t)r * n;
  for (int j = 0; j < n; ++j) {
    u64 m = cand;
#pragma unroll
    for (int s = kWave / 2; s >= 1; s >>= 1) {
      const u64 o = __shfl_xor(m, s, kWave);
      m = o > m ? o : m;
    }
    u64 *slot = wmax + (j & 1) * kWaves;                              // (two sets: a round's words are read while the next one's are written)
    if (lane == 0) slot[wave] = m;
    __syncthreads();
    u64 best = slot[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) best = slot[w] > best ? slot[w] : best;
    if (best == 0ull) {                                               // (uniform) no eligible item is left
      for (int t = j + tid; t < n; t += kBlock) { oi[t] = -1; ov[t] = -INFINITY; }
      break;
    }
    if (tid == 0) { oi[j] = (int32_t)(best & 0xFFFFFFFFull); ov[j] = key_score(best); }
    if (cand == best) cand = best_below(best);
  }
}

// Ranks by counting: a wave takes kKnnRankGroup targets of the row at a time and walks the keys once for them; the exclusion row is
// taken off afterwards (the items in it that are ahead), which leaves the target's own exclusion out of it.  No barrier after the keys.
template <int TYPE>
__global__ __launch_bounds__(kBlock) void k_knn_rank_lists(KnnModel Mo, KnnFused F, const int64_t *__restrict__ target_indptr,
                                                           const int32_t *__restrict__ targets, int64_t P, int32_t *__restrict__ out_rank,
                                                           float *__restrict__ out_score) {
  extern __shared__ __align__(16) unsigned char knn_lds_fused[];
  const int r = blockIdx.x, N = Mo.n_items, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t tlo = min(max(target_indptr[r], (int64_t)0), P), thi = min(max(target_indptr[r + 1], tlo), P);
  if (tlo >= thi) return;                                             // (uniform: before any barrier)
  const int u = F.uid[r];
  const uint32_t *keys = knn_row_keys<TYPE>(Mo, u, F.fallback, F.rows ? (void *)(F.rows + (size_t)r * F.row_bytes) : (void *)knn_lds_fused);
  int64_t xlo, xhi;
  knn_excl_row(F.excl_indptr, u, Mo.n_users, xlo, xhi);
  constexpr int G = kKnnRankGroup;
  for (int64_t g = tlo + (int64_t)wave * G; g < thi; g += (int64_t)(kBlock / kWave) * G) {
    u64 tk[G];
    int cnt[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int t = g + j < thi ? targets[g + j] : -1;
      const u64 key = (unsigned)t < (unsigned)N ? knn_full_key(keys[t], t) : 0ull;
      tk[j] = key ? key : ~0ull;                                      // (nothing is ahead of ~0: no prediction, no rank)
      cnt[j] = 0;
    }
    for (int i = lane; i < N; i += kWave) {
      const u64 key = knn_full_key(keys[i], i);
#pragma unroll
      for (int j = 0; j < G; ++j) cnt[j] += key > tk[j] ? 1 : 0;
    }
    for (int64_t p = xlo + lane; p < xhi; p += kWave) {
      const int c = F.excl_indices[p];
      const u64 key = (unsigned)c < (unsigned)N ? knn_full_key(keys[c], c) : 0ull;
#pragma unroll
      for (int j = 0; j < G; ++j) cnt[j] -= key > tk[j] ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
#pragma unroll
      for (int s = kWave / 2; s >= 1; s >>= 1) cnt[j] += __shfl_xor(cnt[j], s, kWave);
      if (lane == j && g + j < thi) {
        const bool has = tk[j] != ~0ull;
        out_rank[g + j] = has ? cnt[j] : -1;
        out_score[g + j] = has ? key_score(tk[j]) : -INFINITY;
      }
    }
  }
}

// what both entry points check before they launch, and where the working rows of R request rows lie
int knn_fused_args(const KnnModel &Mo, const int32_t *uid, int R, const double *fallback, const int64_t *excl_indptr, const int32_t *excl_indices,
                   void *scratch, size_t scratch_bytes, KnnFused &F, size_t &lds) {
  if (!knn_model_ok(Mo) || R < 0 || (fallback && Mo.type != DRX_KNN_ITEM) || (!excl_indptr != !excl_indices)) return DRX_EINVAL;
  if (R > 0 && !uid) return DRX_EINVAL;
  const size_t need = knn_fused_scratch_bytes(Mo.type, R, Mo.n_items);
  if (need && (!scratch || scratch_bytes < need)) return DRX_ESCRATCH;
  F.uid = uid; F.fallback = fallback; F.excl_indptr = excl_indptr; F.excl_indices = excl_indices;
  F.rows = need ? (unsigned char *)scratch : nullptr;
  F.row_bytes = knn_fused_row_bytes(Mo.type, Mo.n_items);
  lds = need ? 0 : F.row_bytes;
  return DRX_OK;
}

// a kernel of one workgroup per request row whose working row may lie in LDS: the attribute, the launch
template <class... P, class... A>
int knn_rows_launch(void (*kernel)(P...), int R, size_t lds, hipStream_t st, A... args) {
  DRX_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kKnnLdsBytes));
  hipLaunchKernelGGL(kernel, dim3(R), dim3(kBlock), lds, st, args...);
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

}  // namespace
}  // namespace drx

extern "C" size_t drx_knn_neighbours_scratch_bytes(int32_t R, int32_t C, int32_t k, int32_t splits) {
  return drx::knn_scratch_bytes(R, C, k, splits);
}

extern "C" int drx_knn_neighbours(const int64_t *indptr, const int32_t *indices, const float *values, int64_t nnz, int32_t R, int32_t C,
                                  int32_t metric, int32_t k, int32_t m, double shrinkage, double max_diff, int32_t splits, int32_t *out_idx,
                                  float *out_sim, void *scratch, size_t scratch_bytes, void *stream) {
  return drx::knn_run(indptr, indices, values, nnz, R, C, metric, k, m, shrinkage, max_diff, splits, out_idx, out_sim, scratch, scratch_bytes,
                      stream);
}

extern "C" int drx_knn_row_means(const int64_t *indptr, const float *values, int64_t nnz, int32_t R, double *out_mean, void *stream) {
  if (R < 0 || nnz < 0) return DRX_EINVAL;
  if (R == 0) return DRX_OK;
  if (!indptr || !out_mean || (nnz > 0 && !values)) return DRX_EINVAL;
  hipLaunchKernelGGL(drx::k_knn_row_means, dim3((R + drx::kBlock - 1) / drx::kBlock), dim3(drx::kBlock), 0, (hipStream_t)stream, indptr, values,
                     nnz, R, out_mean);
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

extern "C" size_t drx_knn_score_rows_scratch_bytes(int32_t type, int32_t R, int32_t n_items) {
  return drx::knn_score_scratch_bytes(type, R, n_items);
}

extern "C" int drx_knn_score_rows(int32_t type, int32_t aggregation, const int64_t *indptr, const int32_t *indices, const float *values,
                                  int64_t nnz, int32_t n_users, int32_t n_items, const int32_t *nb_idx, const float *nb_sim, int32_t k,
                                  const int32_t *uid, int32_t R, const double *fallback, float *out, uint32_t *cand_mask, void *scratch,
                                  size_t scratch_bytes, void *stream) {
  drx::KnnModel Mo{indptr, indices, values, nnz, n_users, n_items, nb_idx, nb_sim, k, type, aggregation};
  if (!drx::knn_model_ok(Mo) || R < 0 || (fallback && type != DRX_KNN_ITEM)) return DRX_EINVAL;
  if ((int64_t)R * n_items > 0x7FFFFFFFll) return DRX_EINVAL;          // the index range of drx_topk, which reads the matrix
  if (R == 0) return DRX_OK;
  if (!uid || !out) return DRX_EINVAL;
  const size_t row = drx::knn_row_bytes(type, n_items), need = drx::knn_score_scratch_bytes(type, R, n_items);
  if (need && (!scratch || scratch_bytes < need)) return DRX_ESCRATCH;
  const size_t lds = need ? 0 : row;
  hipStream_t st = (hipStream_t)stream;
  void *rows = need ? scratch : nullptr;
  if (type == DRX_KNN_ITEM) return drx::knn_rows_launch(drx::k_knn_score_item, R, lds, st, Mo, uid, fallback, out, cand_mask, (float *)rows);
  return drx::knn_rows_launch(drx::k_knn_score_user, R, lds, st, Mo, uid, out, cand_mask, (double *)rows);
}

extern "C" int drx_knn_pair_scores(int32_t type, int32_t aggregation, const int64_t *indptr, const int32_t *indices, const float *values,
                                   int64_t nnz, int32_t n_users, int32_t n_items, const int32_t *nb_idx, const float *nb_sim, int32_t k,
                                   const int32_t *uid, const int32_t *iid, int64_t P, const double *fallback, double *out, uint8_t *none,
                                   void *stream) {
  drx::KnnModel Mo{indptr, indices, values, nnz, n_users, n_items, nb_idx, nb_sim, k, type, aggregation};
  if (!drx::knn_model_ok(Mo) || P < 0) return DRX_EINVAL;
  if (P == 0) return DRX_OK;
  if (!uid || !iid || !out || !none) return DRX_EINVAL;
  const int64_t groups = (P + drx::kBlock - 1) / drx::kBlock;
  if (groups > 0x7FFFFFFFll) return DRX_EINVAL;
  hipLaunchKernelGGL(drx::k_knn_pair_scores, dim3((unsigned)groups), dim3(drx::kBlock), 0, (hipStream_t)stream, Mo, uid, iid, P, fallback, out,
                     none);
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

extern "C" size_t drx_knn_recommend_scratch_bytes(int32_t type, int32_t R, int32_t n_items, int32_t n) {
  if (n < 1 || n > drx::kKnnMaxTopN) return 0;
  return drx::knn_fused_scratch_bytes(type, R, n_items);
}

extern "C" int drx_knn_recommend(int32_t type, int32_t aggregation, const int64_t *indptr, const int32_t *indices, const float *values,
                                 int64_t nnz, int32_t n_users, int32_t n_items, const int32_t *nb_idx, const float *nb_sim, int32_t k,
                                 const int32_t *uid, int32_t R, int32_t n, const double *fallback, const int64_t *excl_indptr,
                                 const int32_t *excl_indices, int32_t *out_idx, float *out_val, void *scratch, size_t scratch_bytes,
                                 void *stream) {
  drx::KnnModel Mo{indptr, indices, values, nnz, n_users, n_items, nb_idx, nb_sim, k, type, aggregation};
  if (n < 1) return DRX_EINVAL;
  if (n > drx::kKnnMaxTopN) return DRX_ENOTIMPL;
  if (R > 0 && (!out_idx || !out_val)) return DRX_EINVAL;
  drx::KnnFused F;
  size_t lds;
  const int rc = drx::knn_fused_args(Mo, uid, R, fallback, excl_indptr, excl_indices, scratch, scratch_bytes, F, lds);
  if (rc != DRX_OK || R == 0) return rc;
  return drx::knn_rows_launch(type == DRX_KNN_ITEM ? drx::k_knn_recommend<DRX_KNN_ITEM> : drx::k_knn_recommend<DRX_KNN_USER>, R,
                              lds + drx::kKnnFusedTail, (hipStream_t)stream, Mo, F, n, out_idx, out_val);
}

extern "C" size_t drx_knn_rank_lists_scratch_bytes(int32_t type, int32_t R, int64_t P, int32_t n_items) {
  if (P < 1) return 0;
  return drx::knn_fused_scratch_bytes(type, R, n_items);
}

extern "C" int drx_knn_rank_lists(int32_t type, int32_t aggregation, const int64_t *indptr, const int32_t *indices, const float *values,
                                  int64_t nnz, int32_t n_users, int32_t n_items, const int32_t *nb_idx, const float *nb_sim, int32_t k,
                                  const int32_t *uid, int32_t R, const int64_t *target_indptr, const int32_t *targets, int64_t P,
                                  const double *fallback, const int64_t *excl_indptr, const int32_t *excl_indices, int32_t *out_rank,
                                  float *out_score, void *scratch, size_t scratch_bytes, void *stream) {
  drx::KnnModel Mo{indptr, indices, values, nnz, n_users, n_items, nb_idx, nb_sim, k, type, aggregation};
  if (R < 0 || P < 0) return DRX_EINVAL;
  const bool work = R > 0 && P > 0;
  if (work && (!target_indptr || !targets || !out_rank || !out_score)) return DRX_EINVAL;
  drx::KnnFused F;
  size_t lds;
  const int rc = drx::knn_fused_args(Mo, uid, work ? R : 0, fallback, excl_indptr, excl_indices, scratch, scratch_bytes, F, lds);
  if (rc != DRX_OK || !work) return rc;
  return drx::knn_rows_launch(type == DRX_KNN_ITEM ? drx::k_knn_rank_lists<DRX_KNN_ITEM> : drx::k_knn_rank_lists<DRX_KNN_USER>, R, lds,
                              (hipStream_t)stream, Mo, F, target_indptr, targets, P, out_rank, out_score);
}
