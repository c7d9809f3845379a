/* drx.h — C ABI of libdrx.so, the MI355X (gfx950) engine behind the DRecPy-compatible Python surface.
 *
 * The reference (fabioiuri/DRecPy) is pure Python and has no FFI of its own: its device boundary is
 * "whatever TensorFlow eager op the hook calls" (DRecPy/Recommender/recommender_abc.py:191-205).  This
 * header is therefore the boundary a maintainer would bind with ctypes; each entry point names the
 * reference lines whose work it replaces.  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - plain C types only; every pointer whose name is not prefixed `h_` is DEVICE memory owned by the
 *     caller (torch-allocated in the Python host); the library never allocates or frees device memory,
 *     never synchronises the device, and keeps no global state.  Work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream).
 *   - return value: 0 on success, <0 = DRX_E* below, >0 = a hipError_t.  Never throws.
 *   - parameter tables are fp32, row-major, row stride `ld` floats (ld % 4 == 0, ld >= k, the
 *     padding columns are zero and stay zero).
 *   - W2T is the reference's W_ [K,N] stored transposed [N,ld] so that an output unit is one row.
 */
#ifndef DRX_H_
#define DRX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRX_VERSION 100

enum {
  DRX_OK = 0,
  DRX_EINVAL = -1,     /* bad argument (null pointer, k > DRX_MAX_K, ld % 4, ...) */
  DRX_ESCRATCH = -2,   /* scratch buffer too small */
  DRX_ENOTIMPL = -3,
  DRX_ERETRY = -4,     /* a sampler gave up after its maximum number of consecutive failed attempts */
  DRX_ECOMM = -5       /* the RCCL transport failed (librccl missing, or an nccl* call: drx_comm_last_error() has the text) */
};

#define DRX_MAX_K 1024
#define DRX_KEY_NONE 0xFFFFFFFFu

enum { DRX_LOSS_BCE = 0, DRX_LOSS_MSE = 1 };           /* cdae.py:30-31 */
enum { DRX_TARGETS_REFERENCE = 0, DRX_TARGETS_PER_ROW = 1 };   /* (B,B,N) broadcast == batch-mean target, cdae.py:78-79 */
/* or-ed into targets_kind of drx_cdae_step_dense: the batch-membership arrays inside `scratch` are known to be zero (zero-initialised
 * scratch, or scratch last used by a COMPLETED dense step of the same batch size: consumers clear what they read) -> no memset */
#define DRX_DENSE_AUX_CLEAN 0x100
enum { DRX_OPT_ADAM = 0, DRX_OPT_ADAGRAD = 1,
       DRX_OPT_ROWWISE_ADAGRAD = 2,  /* sampled mode only: ONE accumulator per table row, kept in the first float of the row's slot
                                        (s1[var][row * ld]): acc += mean_k(g^2), p -= lr * g / (sqrt(acc) + eps); b and b2 per element */
       /* DENSE updates only (drx_opt_*, drx_rows_csr_opt*, drx_cdae_step_dense / drx_cdae_fit_dense): every sparse / sharded entry point
        * returns DRX_EINVAL for them.  g = data gradient + l2 * p; fp32, one operation at a time, in this order (Keras optimizer_v2): */
       DRX_OPT_SGD = 3,              /* no slot:      p -= lr * g */
       DRX_OPT_MOMENTUM = 4,         /* s1 = accumulator (init 0): s1 = s1 * mu - g * lr;  p += s1 */
       DRX_OPT_NESTEROV = 5,         /* s1 as above:  s1 = s1 * mu - g * lr;  p += s1 * mu - g * lr */
       DRX_OPT_RMSPROP = 6,          /* s1 = rms (init 0): s1 += (g * g - s1) * (1 - rho);  p -= lr * g / (sqrt(s1) + eps) */
       DRX_OPT_RMSPROP_MOMENTUM = 7  /* s1 as above, s2 = mom (init 0): s2 = s2 * mu + (g * lr) / sqrt(s1 + eps);  p -= s2 */ };

/* One update rule for the dense entry points.  Which hyper-parameters and slots a kind reads (an absent slot is passed as NULL and is
 * neither read nor written):
 *   kind                      lr                 mu        mu2      eps   s1            s2
 *   DRX_OPT_ADAM              Keras lr_t         beta_1    beta_2   yes   m             v
 *   DRX_OPT_ADAGRAD           learning rate      -         -        yes   accumulator   -
 *   DRX_OPT_SGD               learning rate      -         -        -     -             -
 *   DRX_OPT_MOMENTUM/NESTEROV learning rate      momentum  -        -     accumulator   -
 *   DRX_OPT_RMSPROP           learning rate      -         rho      yes   rms           -
 *   DRX_OPT_RMSPROP_MOMENTUM  learning rate      momentum  rho      yes   rms           mom
 * Entry points with a step size per variable (DrxAdamSegments::alpha, DrxCsrAdamTable::alpha / alpha_s) take it from there (Adam: the
 * variable's lr_t; the other kinds: the learning rate) and ignore `lr`.  DRX_OPT_ROWWISE_ADAGRAD is not a dense rule: DRX_EINVAL. */
typedef struct DrxOptRule {
  int32_t kind;             /* DRX_OPT_* */
  float lr, mu, mu2, eps;
} DrxOptRule;

/* CDAE parameters (cdae.py:34-41) and optimizer slots of the same shapes.
 * Adam uses s1 = m, s2 = v; Adagrad uses s1 = accumulator (s2 unused, may be NULL). */
typedef struct DrxCdaeParams {
  int32_t n_users, n_items, k, ld;
  float *W;    /* [n_items, ld]  cdae.py:36 */
  float *W2T;  /* [n_items, ld]  cdae.py:37 (transposed) */
  float *V;    /* [n_users, ld]  cdae.py:38 */
  float *b;    /* [ld]           cdae.py:40 */
  float *b2;   /* [n_items]      cdae.py:41 */
} DrxCdaeParams;

/* The training set as the hot loop needs it: CSR of each user's POSITIVE items
 * (interaction >= threshold, duplicates merged, columns ascending) — the non-zeros of
 * `select_user_interaction_vec(uid)` after the binarisation of cdae.py:61. */
typedef struct DrxHistory {
  const int64_t *indptr;   /* [n_users + 1] */
  const int32_t *indices;  /* [indptr[n_users]] */
  /* Optional ITEM-MAJOR RANK of every entry (NULL / 0: none): t_rank[p] = the place of entry p = indptr[u] + j (item indices[p] in the
   * row of user u) when all entries are ordered by (item, user) — the permutation that transposes the matrix, inverted.  With it the
   * preparation of a sampled batch whose rows collect long runs of touches (MovieLens shapes: more than 8 touches per table row) lays
   * the batch's touches down item by item through this static order (a count per entry, a scan, a write entry by entry) instead of sorting millions
   * of (row, sample) pairs per step (csrc/drx_prep.hpp). */
  const int32_t *t_rank;   /* [t_nnz] */
  int64_t t_nnz;           /* = indptr[n_users] < 2^30 */
  /* ... and the entries IN that order (the transpose itself): entry e = item t_items[e] in the row of user t_users[e], at position
   * t_pos[e] of that row — t_rank[indptr[t_users[e]] + t_pos[e]] == e.  All four or none. */
  const int32_t *t_users;  /* [t_nnz] */
  const int32_t *t_pos;    /* [t_nnz] */
  const int32_t *t_items;  /* [t_nnz] */
} DrxHistory;

/* One mini-batch (one fit() "epoch", recommender_abc.py:189-205).
 * uid  : the sampled users (PointSampler triples' first field, cdae.py:52).
 * iid,y: sampled output unit and its {0,1} target — used by the sampled-output mode only.
 * Corruption (cdae.py:63): entry j of user uid[b]'s history survives iff
 *     keep != NULL ?  keep[keep_off[b] + j] != 0            (host MT19937 stream, parity mode)
 *                  :  drx_hash_u32(mask_seed, b, j) >= q * 2^32  (counter-based, throughput mode)
 * keep_off[b] = sum_{b' < b} deg(uid[b'])  (exclusive prefix sum, keep_off[B] = total). */
typedef struct DrxBatch {
  int32_t B;
  const int32_t *uid;       /* [B] */
  const int32_t *iid;       /* [B] or NULL */
  const float   *y;         /* [B] or NULL */
  const int32_t *keep_off;  /* [B + 1] */
  const uint8_t *keep;      /* [keep_off[B]] or NULL */
  uint64_t mask_seed;
  float q;                  /* corruption level; survivors are scaled by 1/(1-q) */
  int32_t n_touch_slots;    /* host-known upper bound of keep_off[B] (sizes the sort) */
  uint32_t flags;           /* DRX_BATCH_* (0: none) */
} DrxBatch;
/* Sampled mode, batches in which users REPEAT (B several times the number of users: MovieLens shapes), prepared through the history's
 * transpose (DrxHistory::t_rank; lists of long segments): the triples of one user share their gather and their gradient.  The samples
 * of a user, ascending, are cut into WORK ITEMS of up to 16 triples (csrc/drx_prep.hpp k_tp_item_*):
 *   forward : one workgroup per work item loads every row of the user's history ONCE and adds it into the bags of the item's triples
 *             under their keep bits — a masked matrix product [16 triples x history] x [history x K] (csrc/drx_cdae.hip
 *             k_items_fwd_bwd, v_mfma_f32_16x16x4_f32: fp32, products with 0 / 1) — instead of one gather per triple;
 *   backward: an item row of the user's history receives, per work item,  D_w - sum of dz1[b] over the triples b of the item that
 *             DROPPED it,  D_w = sum of dz1 over the item's triples (a row of its own behind the samples' gradient rows) — where
 *             that is the shorter form (1 + droppers < keepers), else one touch per keeper as without the flag.
 * With corruption level q the touch list shrinks towards q + 1/16 of its plain length (ml-1m shape: 8.0 M -> 2.9 M touches), the rows
 * the forward kernel loads to 1 / (triples per work item) (8.0 M -> 1.0 M).  Another association of the same sums: same oracle, same
 * tolerance; bit-reproducible (every order is a function of the batch).  Prepare and step must see the same flag; it is ignored
 * (plain lists) where the transposed preparation does not apply, rows are narrower than 33 / wider than 255 floats, or the step
 * builds its list inline (drx_cdae_step_sparse: only lists prepared ahead, drx_cdae_sparse_prepare, take the shared form).
 * Single-GPU step only. */
#define DRX_BATCH_SHARE_USERS 1u

typedef struct DrxOptim {
  int32_t kind;             /* DRX_OPT_* */
  float lr, reg_rate;       /* reg is applied as reg_rate / B (cdae.py:82) */
  float beta1, beta2, eps;  /* Adam: .9 .999 1e-7 (Keras); Adagrad: eps 1e-7 */
  /* Per kind (the new kinds: drx_cdae_step_dense / drx_cdae_fit_dense only; DrxOptRule's table has the arithmetic):
   *   ADAM              beta1, beta2, eps, alpha[]; s1 = m, s2 = v          ADAGRAD / ROWWISE_ADAGRAD  lr, eps; s1 (s2 may be NULL)
   *   SGD               lr; no slot (s1, s2 may be NULL)                   MOMENTUM / NESTEROV        lr, beta1 = momentum; s1
   *   RMSPROP           lr, beta2 = rho, eps; s1                           RMSPROP_MOMENTUM           lr, beta1 = momentum, beta2 = rho, eps; s1, s2 */
  /* Keras-Adam lr_t = lr*sqrt(1-b2^t)/(1-b1^t) per variable in registration order W, W_, V, b, b_
   * (recommender_abc.py:328-334 advances the counter once per variable: t = 5*step + j + 1). */
  float alpha[5];
  float *s1[5];             /* slots in the order W, W2T, V, b, b2 */
  float *s2[5];
} DrxOptim;

int drx_version(void);
const char *drx_strerror(int code);

/* Stream-ordering events for the host's run-ahead pipelines (sampler / touch-list preparation on a side stream of the same device):
 * created with hipEventDisableTiming | hipEventDisableSystemFence, i.e. a record is an agent-scope release, not an L2 write-back
 * for host visibility.  NOT for host-side reads of device results other than through drx_event_synchronize + pinned memory. */
void *drx_event_create(void);
void drx_event_destroy(void *ev);
int drx_event_record(void *ev, void *stream);
int drx_stream_wait_event(void *stream, void *ev);
int drx_event_synchronize(void *ev);

/* A stream confined to a slice of the chip, for the run-ahead work that shares it with the training kernels (sampler, touch-list
 * preparation): hipExtStreamCreateWithCUMask.  cus_per_xcd CUs of EVERY XCD (1 .. 32 on gfx950; mask bit i names CU i / 8 of XCD i % 8 —
 * scripts/mb/mb_cumask.hip prints the census), taken from the top of each XCD's CUs.  The preparation's small launches then queue for
 * THEIR CUs instead of displacing the training kernels' waves everywhere.  Returns NULL when the runtime refuses. */
void *drx_stream_create_cu_slice(int32_t cus_per_xcd);
void drx_stream_destroy(void *stream);

/* 64-bit mix used for the counter-based corruption mask; exported so hosts/tests can reproduce it. */
uint32_t drx_hash_u32(uint64_t seed, uint32_t a, uint32_t b);

/* ---- inference ------------------------------------------------------------------------------
 * h[B,ld] = sigmoid(scale * sum_{kept} W[n] + V[uid] + b);  p[B,n_items] = sigmoid(h W_ + b_).
 * Replaces CDAE._reconstruct (cdae.py:73-76) as used by _predict/_rank (cdae.py:67-71,84-103:
 * keep == NULL && q == 0 -> uncorrupted, unscaled) and by _predict_batch (cdae.py:50-65).
 * p may be NULL (hidden layer only). */
int drx_cdae_forward(const DrxCdaeParams *p, const DrxHistory *hist, const DrxBatch *bt,
                     float *h, float *pred, void *stream);

/* ---- scratch sizing ---------------------------------------------------------------------- */
/* dense_mode != 0: drx_cdae_step_dense (per-row batch bitmasks: grows with B * (n_users + n_items) / 8 bytes);
 * dense_mode == 0: drx_cdae_step_sparse* (grows with the number of touches). */
size_t drx_cdae_scratch_bytes(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots, int32_t dense_mode);

/* ---- one reference-mode training step ------------------------------------------------------
 * forward + Keras BCE/MSE against the batch-mean (or per-row) target over ALL output units +
 * L2/B on W, W_, V + backward + dense Adam on every parameter: replaces the body of the fit() loop
 * recommender_abc.py:190-204 for CDAE (cdae.py:50-82).  loss_out (device, 2 floats: prediction
 * loss, regularisation loss) may be NULL. */
int drx_cdae_step_dense(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist,
                        const DrxBatch *bt, int32_t loss_kind, int32_t targets_kind,
                        void *scratch, size_t scratch_bytes, float *loss_out, void *stream);

/* ---- one sampled-output training step (engine mode) ----------------------------
 * per triple (uid, iid, y): one output unit, loss mean over B, L2/B on touched rows, sparse
 * Adagrad / lazy Adam on touched rows of W, W2T, V, b2 and dense update of b.
 * alpha[0] is used as the Adam lr_t for every table. */
int drx_cdae_step_sparse(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist,
                         const DrxBatch *bt, int32_t loss_kind,
                         void *scratch, size_t scratch_bytes, float *loss_out, void *stream);

/* Same step with per-phase timing: `events` holds DRX_SPARSE_PHASES + 1 caller-created hipEvent_t; event i is recorded
 * on `stream` before phase i, the last one after the final phase.  Phases: 0 gather+forward+backward (k_sampled_fwd_bwd),
 * 1 touch sort, 2 segmented reduce + row update (k_seg_reduce), 3 tail launch A (short chunk-crossing segments, and beside
 * them the column-sum partials of the hidden-bias gradient), 4 tail launch B (long segments, and the hidden-bias update). */
#define DRX_SPARSE_PHASES 5
int drx_cdae_step_sparse_timed(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist,
                               const DrxBatch *bt, int32_t loss_kind, void *scratch, size_t scratch_bytes,
                               float *loss_out, void *const *events, void *stream);

/* The touch list of a batch (row keys sorted, with the contributing sample) depends only on the batch, not on the
 * parameters: it can be prepared for batch t+1 on another stream while batch t trains.  `prepared` is an opaque
 * device buffer of drx_cdae_prep_bytes() bytes; events may be NULL (else as in drx_cdae_step_sparse_timed; phase 1 is
 * then empty). */
size_t drx_cdae_prep_bytes(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots);
int drx_cdae_sparse_prepare(const DrxCdaeParams *p, const DrxHistory *hist, const DrxBatch *bt, void *prepared,
                            size_t prepared_bytes, void *stream);
int drx_cdae_step_sparse_prepared(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist, const DrxBatch *bt,
                                  int32_t loss_kind, const void *prepared, size_t prepared_bytes, void *scratch,
                                  size_t scratch_bytes, float *loss_out, void *const *events, void *stream);

/* HOT HEAD of the single-GPU sampled Adagrad step (lists of short segments, ld = 64 / 128 / 256): the kept history entries of the H
 * hottest items leave the touch list (DRX_KEY_NONE, like dropped ones) and set bit b of a transposed 0/1 mask M[h][b / 32] instead;
 * their W rows' gradients are then (1/(1-q)) * M^T * dz1, computed on the matrix cores beside the segmented reduction.  slot[n_items]:
 * the hot slot of an item (-1: cold); item[H]: the item of each slot (device arrays).  H = 0 is no head: the functions below are then
 * the plain ones (drx_cdae_prep_bytes, drx_cdae_sparse_prepare, drx_cdae_step_sparse(_prepared)).  A step given H > 0 on any other path
 * (Adam, row-wise Adagrad, long segments, ld = 256, the column-sharded step) returns DRX_EINVAL.  The prepared buffer carries the mask
 * behind the plain layout.  The library records, by the buffer's address, the H every preparation into a buffer used (the plain ones: 0)
 * — on the host, so that a step queued while its list is still being prepared need not wait for it — and every step on a prepared list
 * (drx_cdae_step_sparse_prepared, drx_cdae_kshard_step, drx_cdae_step_sparse_hot) returns DRX_EINVAL unless it is given that H.  A copy
 * of a list into another buffer carries no record (it reads as H = 0).  drx_cdae_prep_forget drops the record of a buffer that is
 * released. */
typedef struct DrxHotHead {
  int32_t H;                    /* multiple of 32, <= DRX_MAX_HOT */
  const int16_t *slot;
  const int32_t *item;
} DrxHotHead;
#define DRX_MAX_HOT 1024
size_t drx_cdae_prep_bytes_hot(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots, int32_t H);
size_t drx_cdae_scratch_bytes_hot(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots, int32_t H);
int drx_cdae_sparse_prepare_hot(const DrxCdaeParams *p, const DrxHistory *hist, const DrxBatch *bt, const DrxHotHead *hot,
                                void *prepared, size_t prepared_bytes, void *stream);
/* prepared == NULL: the list (and the mask) built inline, in the scratch */
int drx_cdae_step_sparse_hot(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist, const DrxBatch *bt,
                             const DrxHotHead *hot, int32_t loss_kind, const void *prepared, size_t prepared_bytes, void *scratch,
                             size_t scratch_bytes, float *loss_out, void *const *events, void *stream);
/* H where drx_cdae_step_sparse_hot given these arguments (opt_kind: DrxOptim.kind) accepts a head of H rows, 0 where it returns DRX_EINVAL:
 * the library's own answer (the same functions the step asks), for a caller that decides whether to prepare a batch with a head */
int32_t drx_cdae_hot_rows_for(const DrxCdaeParams *p, int32_t opt_kind, int32_t B, int32_t n_touch_slots, int32_t H);
void drx_cdae_prep_forget(const void *prepared);

/* DEBUGGING ENTRY (tests): the first two launches of a preparation on the caller's batch — the touch kernel, then the sort's first
 * launch: its counting launch, or the fold of the per-workgroup counts the touch kernel left (8-bit first digits) — and device copies
 * of what the sort and the launch order consume, before any sort trusts them (a wrong histogram makes the first pass scatter out of
 * range rather than fail):
 *   hist_out    [2048]  the first digit's histogram of the keys that are not DRX_KEY_NONE (2^info_out[0] words written)
 *   buckets_out [256]   samples per degree bucket, bucket = 255 - min((keep_off[b + 1] - keep_off[b]) >> 2, 255)
 *   keys_out / vals_out [n_touch_slots + 2 B]  the list in batch order: slots keep_off[b] + 2 b .. of sample b (its history, then its
 *               output row n_items + iid, then its user row 2 n_items + uid), DRX_KEY_NONE for a dropped or hot entry and behind the batch
 *   mask_out    [H x ceil(B / 32)]  the hot head's transposed mask (hot != NULL with H > 0)
 *   info_out    (HOST) [4]: first digit's bits | partial-count rows folded (0: the counting launch ran) | list slots | touch workgroups
 * hot: NULL or a head as for drx_cdae_sparse_prepare_hot.  present: NULL, or the row-sharded step's presence map (one byte per wire
 * key of an item row, see "row-sharded multi-GPU step"; zeroed by the caller) with its geometry (items per rank, chunk shift, world).
 * prepared: >= drx_cdae_prep_bytes_hot(p, B, n_touch_slots, H) bytes; it holds no list afterwards. */
int drx_debug_prep_counts(const DrxCdaeParams *p, const DrxHistory *hist, const DrxBatch *bt, const DrxHotHead *hot, uint8_t *present,
                          int32_t ipr, int32_t cshift, int32_t world, void *prepared, size_t prepared_bytes, uint32_t *hist_out,
                          uint32_t *buckets_out, uint32_t *keys_out, uint32_t *vals_out, uint32_t *mask_out, int32_t *info_out,
                          void *stream);

/* DEBUGGING ENTRY (tests): device copies of what a finished preparation — drx_cdae_sparse_prepare / _hot of a batch of B samples and
 * n_touch_slots slots, with a head of H rows (0: none) — left in `prepared`, laid out as the step reads it; nothing is launched:
 *   keys_s_out / vals_s_out [n_touch_slots + 2 B]  the sorted list: the touches that are not DRX_KEY_NONE ordered by key, the touches of a
 *               key in a fixed order (sorted: samples ascending; through the history's transpose: user by user, samples ascending inside
 *               a user), the key of a V / W2T row's sole touch blanked to DRX_KEY_NONE where marks are made (ld > 16), its sample kept;
 *               DRX_KEY_NONE behind the list
 *   solo_v_out / solo_o_out [B]  1: sample b is the only one of the batch that touches its V row / its W2T row
 *   order_out   [B]     the forward kernel's launch order: a permutation of the samples, degree buckets ascending
 * prepared: the buffer the preparation wrote, same p, B, n_touch_slots and H. */
int drx_debug_prep_result(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots, int32_t H, const void *prepared, size_t prepared_bytes,
                          uint32_t *keys_s_out, uint32_t *vals_s_out, uint8_t *solo_v_out, uint8_t *solo_o_out, int32_t *order_out,
                          void *stream);

/* DEBUGGING ENTRY (tests): the sampled step's reduction and span launches ALONE, on gradient rows the caller gives.  Everything is the
 * step's (drx_cdae_step_sparse / _prepared / _hot: the same scratch layout, the same launches in the form the step would choose, the list
 * built inline where prepared == NULL) except its forward / backward launch: instead, dz1_in [B, ld], g2_in [B, ld] and dz2_in [B] (device
 * arrays) are copied into the step's gradient buffers and the per-sample losses are zeroed.  So W row n moves by the optimizer's rule on
 * g = (1/(1-q)) * sum of dz1_in[b] over the list's touches (n, b), W2T row i on sum g2_in[b] (b2[i] on sum dz2_in[b]) over the samples of
 * item i, V row u on sum dz1_in[b] over the samples of user u, b on the column sums of dz1_in — each + (reg_rate / B) * the row's value.
 * A V / W2T row whose sole touch a preparation blanked is the forward kernel's to update: here nobody updates it.
 * hot: NULL, or the head the list was prepared with (inline lists: the head to build).  form: 0 — as the step; 1 — the planned kernel
 * where the step would run the streamed one (DRX_EINVAL with a head, or on a list of long segments).  bt->y is not read.
 * scratch: drx_cdae_scratch_bytes(_hot). */
int drx_debug_cdae_reduce(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist, const DrxBatch *bt, const DrxHotHead *hot,
                          const void *prepared, size_t prepared_bytes, const float *dz1_in, const float *g2_in, const float *dz2_in,
                          int32_t form, void *scratch, size_t scratch_bytes, void *stream);

/* DEBUGGING ENTRY (tests): device copies of the span plan a finished preparation left in `prepared` (csrc/drx_segreduce.hpp SpanPlan;
 * the list's chunks are of 32 touches, of 64 where n_touch_slots + 2 B > 8 (2 n_items + n_users)); nothing is launched:
 *   ext_out  [n_chunks] bytes   chunk g also takes the first ext[g] touches of chunk g + 1
 *   desc_out [2 n_chunks] words descriptor i = (first chunk g0, chunks wholly inside | has_end << 31): the short spans from the front,
 *                               the long ones from the back, each group in no particular order
 *   cnt_out  [2]                short spans, long spans
 * prepared: the buffer the preparation wrote, same p, B, n_touch_slots and H. */
int drx_debug_span_plan(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots, int32_t H, const void *prepared, size_t prepared_bytes,
                        uint8_t *ext_out, uint32_t *desc_out, uint32_t *cnt_out, void *stream);

/* off[0] = 0, off[b + 1] = sum_{b' <= b} (indptr[ids[b'] + 1] - indptr[ids[b']]) for device ids: the keep_off of a batch of users (DrxBatch)
 * or the touch offsets of a batch of CSR rows.  scratch: drx_point_sample_scratch_bytes(B). */
int drx_batch_offsets(const int64_t *indptr, const int32_t *ids, int32_t B, int32_t *off, void *scratch, size_t scratch_bytes, void *stream);

/* ---- device-side point sampler (throughput mode; distribution of point_sampler.py:44-61) ------------
 * Draws B triples with a counter-based generator keyed by (seed, b): negatives with probability
 * neg_ratio/(neg_ratio+1) = uniform (u,i) outside u's positives, positives = uniform user then uniform positive.
 * Also writes keep_off[B+1] (exclusive prefix sum of deg(uid[b])).
 * host_mailbox (optional): 8 bytes of PINNED host memory; the last kernel stores ((uint64)tag << 32) | keep_off[B] there with one
 * system-scope store, so a host that runs ahead learns the batch's touch count by polling for its tag — no copy, no event.
 *
 * THE STREAM.  Draw b reads h(k) = drx_hash_u32(seed, b, k), k = 0, 1, 2, ...; every index below is (h * n) >> 32 in 64-bit integers:
 *   k = 0      the kind: a negative iff h(0) * (neg_ratio + 1) > 2^32 (the kernel's double expression, exact in integers: h(0) / 2^32
 *              and its product with neg_ratio + 1 are both representable while neg_ratio < 2^21), else a positive; neg_ratio = 0 never
 *              gives a negative
 *   k = 1 ..   the attempts, each taking the next unused counters, at most 4096 attempts per draw:
 *     negative attempt, TWO counters: user u = (h * n_users) >> 32, then item i = (h * n_items) >> 32; accepted iff i is not in u's row
 *              of `recorded` (of `hist` where recorded is NULL) — a user who records nothing accepts every item
 *     positive attempt, ONE counter: user u = (h * n_users) >> 32; a user without a positive (deg = 0 in hist) is rejected and no second
 *              counter is taken; otherwise a SECOND counter picks position (h * deg) >> 32 of u's row of hist, and the attempt is accepted
 *   uid[b], iid[b] = the accepted pair.
 *   y[b]:  positive: 1 (drx_point_sample*), or the pair's value v = pos_values[position in hist] (drx_point_sample_valued) — raw when
 *          vrange <= 0, (v - vmin) / vrange in float32 (one subtraction, one division) when vrange > 0;
 *          negative: 0, or (0 - vmin) / vrange in float32 where values are given and vrange > 0.
 *   WHEN THE 4096 ATTEMPTS RUN OUT (a frame in which almost no user is eligible) the draw is still written, silently and with a WRONG
 *   label: a negative gets the last rejected pair — a recorded pair — with the negative's target; a positive gets the last user drawn —
 *   who has no positive —, item 0 and y = 1 (values or not).  Callers must not rely on this: it is what the code does today, not a
 *   contract, and no frame should reach it.
 * Restated on the CPU by oracle/data_oracle.py::point_sample_counter (tests/test_gpu_point_sampler.py compares bit for bit, y included). */
size_t drx_point_sample_scratch_bytes(int32_t B);
int drx_point_sample(const DrxHistory *hist, int32_t n_users, int32_t n_items, int32_t B, int32_t neg_ratio,
                     uint64_t seed, int32_t *uid, int32_t *iid, float *y, int32_t *keep_off,
                     void *scratch, size_t scratch_bytes, uint64_t *host_mailbox, uint32_t tag, void *stream);
/* recorded: CSR (columns ascending) of EVERY pair the training set records, whatever its value — the reference draws its negatives among
 * the pairs absent from the frame (point_sampler.py:56, mem_dataset.py:131-163), not among the non-positives; NULL = hist (frames whose
 * recorded pairs all are positives).  drx_point_sample = this with NULL. */
int drx_point_sample_recorded(const DrxHistory *hist, const DrxHistory *recorded, int32_t n_users, int32_t n_items, int32_t B,
                              int32_t neg_ratio, uint64_t seed, int32_t *uid, int32_t *iid, float *y, int32_t *keep_off,
                              void *scratch, size_t scratch_bytes, uint64_t *host_mailbox, uint32_t tag, void *stream);

/* The same draws (the same triples for the same seed), handed out SORTED BY USER, a user's triples in the order they were drawn —
 * for batches whose touch lists are prepared through the history's transpose (DrxHistory::t_rank): with the batch in user order the
 * expanded list has every row's touches sample-ascending, i.e. the reduction streams through the gradient rows instead of hopping,
 * and the triples of one user sit side by side in the forward kernel.  The order of a batch changes no sum's terms. */
size_t drx_point_sample_by_user_scratch_bytes(int32_t B, int32_t n_users);
int drx_point_sample_by_user(const DrxHistory *hist, const DrxHistory *recorded, int32_t n_users, int32_t n_items, int32_t B,
                             int32_t neg_ratio, uint64_t seed, int32_t *uid, int32_t *iid, float *y, int32_t *keep_off, void *scratch,
                             size_t scratch_bytes, uint64_t *host_mailbox, uint32_t tag, void *stream);

/* The same draws carrying VALUES (DMF.fit(device_sampler=True), dmf.py:64-73): y[b] = 0 for a negative, else the drawn pair's
 * interaction value pos_values[position in hist] — standardised (v - vmin) / vrange when vrange > 0 (use_nce:
 * recommender_abc.py:463-465), raw otherwise.  No keep_off / mailbox: DMF needs neither. */
int drx_point_sample_valued(const DrxHistory *hist, const DrxHistory *recorded, const float *pos_values, float vmin, float vrange,
                            int32_t n_users, int32_t n_items, int32_t B, int32_t neg_ratio, uint64_t seed, int32_t *uid, int32_t *iid,
                            float *y, void *stream);

/* ---- device-side list sampler (throughput mode; distribution of list_sampler.py:74-151 as caser.py:72-75 configures it) -----
 * The reference's ListSampler is ONE MT19937 stream: draw d depends on every draw before it, so a reference-exact fit() is bound by
 * one host thread (about 0.5 us per window).  This entry point draws B windows independently with the counter-based generator of
 * the other throughput modes, draw d from drx_hash_u32(seed, d, k):
 *   k = 0      group   = eligible[(h * n_eligible) >> 32]                 (rng.choice over the groups, ineligible ones re-drawn)
 *   k = 1      start   = (h * (rows - n_inputs - n_targets + 1)) >> 32    (rng.randint(0, rows - max_positive_records - n_targets))
 *   k = 2+16i+a  negative i, attempt a: the ((h * n_pop) >> 32)-th id of the ascending complement of the group's ids in
 *              [0, n_ids); an id already drawn for this window is drawn again (a = 1 .. 15), then the next free one is taken
 *              (rng.sample(eligible, n): uniform without replacement)
 * before[d] = the ids of rows start .. start + n_inputs - 1 of the group (rows in the sampler's sort order), after[d] = the ids of
 * the next n_targets rows followed by the n_targets * neg_ratio negatives.  Restated on the CPU by oracle/data_oracle.py::
 * list_sample_counter (the test compares bit for bit). */
typedef struct DrxListGroups {
  const int64_t *indptr;       /* [n_groups + 1] rows of every group */
  const int32_t *seq_ids;      /* [indptr[n_groups]] negative_ids_col value of every row, a group's rows in the sampler's order */
  const int64_t *held_indptr;  /* [n_groups + 1] */
  const int32_t *held;         /* ascending distinct ids among a group's rows */
  const int32_t *group_value;  /* [n_groups] the value of the group column (Caser: uid) */
  const int32_t *eligible;     /* [n_eligible] groups with >= n_inputs + n_targets rows and >= n_targets * neg_ratio ids outside */
  int32_t n_groups, n_eligible, n_ids;
} DrxListGroups;
int drx_list_sample_device(const DrxListGroups *g, int32_t B, int32_t n_inputs, int32_t n_targets, int32_t neg_ratio, uint64_t seed,
                           int32_t *group_out, int32_t *before, int32_t *after, void *stream);

/* ---- column-sharded ("K-sharded") multi-GPU step (no reference equivalent) ------------------------------------------------
 * Every rank holds ALL rows but only its own columns of W, W2T, V and b (DrxCdaeParams describes that slice: k = local columns;
 * b2 is replicated) and trains on the SAME global batch.  The one exchange of a step is the sum over ranks of the per-triple
 * partial dot products: forward -> all-reduce(dot_partial) -> step.  Everything else (touch list, segmented reduction, updates)
 * is the single-GPU step on K/N columns.  drx_cdae_kshard_step is drx_cdae_step_sparse(_prepared) with the forward half
 * replaced by (h, dot_total); `prepared` may be NULL (touch list built inline), `events` as in drx_cdae_step_sparse_timed. */
int drx_cdae_kshard_forward(const DrxCdaeParams *p, const DrxHistory *hist, const DrxBatch *bt, float *h_out /* [B, ld] */,
                            float *dot_partial /* [B] */, void *stream);
/* the same with the batch's prepared list at hand: the triples are launched in the list's order of history lengths (longest first,
 * similar lengths side by side), like the single-GPU forward kernel; prepared == NULL: the batch's own order */
int drx_cdae_kshard_forward_prepared(const DrxCdaeParams *p, const DrxHistory *hist, const DrxBatch *bt, const void *prepared,
                                     size_t prepared_bytes, float *h_out /* [B, ld] */, float *dot_partial /* [B] */, void *stream);
int drx_cdae_kshard_step(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist, const DrxBatch *bt, int32_t loss_kind,
                         const float *h, const float *dot_total, const void *prepared, size_t prepared_bytes, void *scratch,
                         size_t scratch_bytes, float *loss_out, void *const *events, void *stream);

/* The leading drx_cdae_prep_result_bytes of a `prepared` buffer are all that a step reads of it (the sorted list and the
 * sole-toucher marks): a buffer whose leading bytes were copied from another device's drx_cdae_sparse_prepare of the SAME batch
 * (same B, n_touch_slots, n_users, n_items) is a valid `prepared` argument — how one rank of a column-sharded job prepares the
 * list of a step for all the others. */
size_t drx_cdae_prep_result_bytes(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots);

/* Touch list prepared in PARTS (column-sharded layout: all ranks need the same list of the same batch, and sorting it on every
 * rank is the one cost that does not shrink with N).  Part r of `parts` = the touches of the rows with id % parts == r (item id for W
 * and W2T keys, user id for V keys), taken in sample order and sorted by key; the list of the batch is the
 * concatenation of the parts in order (equal keys adjacent, the touches of a key in sample order: all the segmented reduction needs).
 *   drx_cdae_sparse_prepare_part     -> part_out [drx_cdae_prep_part_out_bytes]: 4 int32 (touches, distinct keys, overflow, 0), then per
 *                                       distinct key (key << 32 | first position), then the samples of the touches — 4 bytes a touch
 *   (the host gathers the parts of all ranks, in rank order, into all_parts [parts * part_out_bytes])
 *   drx_cdae_sparse_prepare_assemble -> a `prepared` buffer like drx_cdae_sparse_prepare's; overflow_out[0] (device) = 1 when a part
 *                                       did not fit its fixed capacity (1.25 x the even share): that list is incomplete and the
 *                                       caller must prepare the batch with drx_cdae_sparse_prepare instead. */
size_t drx_cdae_prep_part_out_bytes(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots, int32_t parts);
/* out4 = byte offset of the runs, byte offset of the samples, capacity in runs, capacity in touches (of one part) */
int drx_cdae_prep_part_layout(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots, int32_t parts, size_t *out4);
size_t drx_cdae_prep_part_bytes(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots, int32_t parts);
int drx_cdae_sparse_prepare_part(const DrxCdaeParams *p, const DrxHistory *hist, const DrxBatch *bt, int32_t part, int32_t parts,
                                 void *part_out, size_t part_out_bytes, void *scratch, size_t scratch_bytes, void *stream);
int drx_cdae_sparse_prepare_assemble(const DrxCdaeParams *p, const DrxBatch *bt, const void *all_parts, int32_t parts, void *prepared,
                                     size_t prepared_bytes, int32_t *overflow_out, void *stream);

/* ---- row-sharded multi-GPU step (BASELINE.json configuration 4; no reference equivalent — DRecPy is single-process:
 * recommender_abc.py:16 is its only device line) -------------------------------------------------------------------------------------
 * Per-rank, collective-free pieces of the sampled step; the host (drecpy_amd/dist.py) runs the RCCL all-to-all exchanges between
 * them.  Users (V, histories, samples) are sharded by uid range; item rows (W, W2T, b2) by item range of `items_per_rank` rows; in
 * this mode DrxCdaeParams describes the LOCAL tables (n_users = local users, n_items = items_per_rank).
 *
 * WIRE keys of item rows are UNIT-major (r06).  Item n of owner o = n / ipr has the local key l = 2 * (n - o * ipr) + (W2T row ? 1 : 0);
 * with 1 << shift the smallest power of two >= max(2 * ipr, 8192) and C = `chunks` (a power of two; the library lowers it until
 * cshift = shift - log2 C >= 13), the local keys are cut into C EXCHANGE CHUNKS of 1 << cshift keys, unit v = (l >> cshift) * world + o,
 * and the wire key is (v << cshift) | (l & ((1 << cshift) - 1)).  A rank's distinct keys ("uniq"), ascending, are contiguous per unit,
 * each unit's run closed by one SENTINEL key DRX_KEY_NONE: n_v = distinct rows asked of owner v % world in chunk v / world, + 1.
 * Chunk c of every exchange (keys, rows, gradient rows) is ONE all-to-all over the units c * world .. c * world + world - 1, which are
 * contiguous in `uniq` and in the float buffers: the host pipelines the chunks (gradient rows of chunk c + 1 travel while the owner
 * applies chunk c and gathers chunk c's rows for the next step).  chunks <= 1: one all-to-all per exchange (the r04 / r05 format).
 *
 * EXCHANGE BUFFER (float32, the same geometry in both directions): for every unit, in unit order, a piece of n rows of ld floats
 * followed by n scalars padded to a multiple of 32 floats — n * ld + roundup(n, 32) floats (n = n_v on the requester's side, the
 * received counts on the owner's: one SEGMENT per source rank and chunk).  Row i of a piece answers key i of the unit's run.
 * Owner -> requester: the parameter row, scalar = b2 of a W2T row; the sentinel row is unused.  Requester -> owner: the rank's summed
 * gradient row, scalar = gradient of b2; the SENTINEL rows carry the rank's gradient of the replicated hidden bias b and, as their
 * scalar, the rank's loss sum — the owner adds those of the LAST chunk's `world` segments in rank order, the same rows on every rank,
 * so b needs no all-reduce. */
#define DRX_MAX_WORLD 64                /* world x chunks of one sharded job (per-unit offsets: DRX_MAX_WORLD + 1 entries) */
#define DRX_MAX_MICRO 4                 /* micro-batches of one step (their exchanges overlap each other's compute) */
#define DRX_MAX_CHUNKS 16               /* exchange chunks per owner */
typedef struct DrxShard {
  int32_t world, rank;
  int32_t n_items;          /* global number of items */
  int32_t items_per_rank;   /* ceil(n_items / world) */
  int32_t n_users_local;
  uint32_t flags;           /* DRX_SHARD_* */
  int32_t chunks;           /* exchange chunks per owner: 0 / 1 = one all-to-all per exchange, else a power of two <= DRX_MAX_CHUNKS */
} DrxShard;
/* the chunk count the library actually uses for a description (chunks lowered until every unit spans whole 8192-key tiles), and log2
 * of a unit's key span; 0 for an invalid description */
int32_t drx_shard_chunks(const DrxShard *sh);
int32_t drx_shard_unit_shift(const DrxShard *sh);
/* The rank's OWN item rows never pass through a collective: the forward kernel reads them from the local tables, the gather skips
 * the requests the rank sent to itself, and its own gradient pieces are read by drx_shard_apply where drx_shard_step_local left them.
 * The float exchange buffers then hold the units of the OTHER peers in unit order (split size 0 for the rank itself), and on the
 * requester's side the own units (one per chunk, in chunk order) follow them all (rows_cache never reads them, grad_send keeps
 * them).  The KEY exchange is unchanged. */
#define DRX_SHARD_SELF_BYPASS 1u

/* Parameter-independent preparation of one local batch, built ahead on a side stream: the sorted touch list with its span plan,
 * sole-toucher marks and launch order (as drx_cdae_sparse_prepare), plus the batch's distinct item rows: wire keys with sentinels, their
 * positions in the exchange buffers, per-owner counts.  `prepared` (256-byte aligned, drx_shard_prep_bytes) is opaque except for the
 * two arrays drx_shard_prep_layout names: out4 = { byte offset of uniq (uint32[capacity]), byte offset of counts (int64[world x chunks],
 * OWNER-major: counts[o * chunks + c] = n of unit c * world + o — what the count exchange sends, `chunks` entries per peer),
 * capacity of uniq in keys, bytes a step reads }.  `work` (drx_shard_work_bytes) must be ZERO when first handed in; the library
 * leaves it zero after every call (it may be shared by all preparations issued on one stream). */
size_t drx_shard_prep_bytes(const DrxCdaeParams *p, const DrxShard *sh, int32_t B, int32_t n_touch_slots);
size_t drx_shard_work_bytes(const DrxShard *sh);
int drx_shard_prep_layout(const DrxCdaeParams *p, const DrxShard *sh, int32_t B, int32_t n_touch_slots, size_t *out4);
int drx_shard_prepare(const DrxCdaeParams *p, const DrxShard *sh, const DrxHistory *hist, const DrxBatch *bt, void *prepared,
                      size_t prepared_bytes, void *work, size_t work_bytes, void *stream);
/* Owner side, ONE EXCHANGE CHUNK per call.  The n keys a rank received for chunk `chunk` are `n_segments` = world x (micro-batches of
 * the step, <= DRX_MAX_MICRO) segments, micro-batch-major then source rank, recv_counts[s] (HOST array, sentinel included) keys in
 * segment s.  drx_shard_owner_index: parameter-independent, run when the keys arrive: table[local key][segment] = index of the key in
 * the chunk's key array (drx_shard_owner_table_bytes; ONE table for all chunks of a step — a call clears and fills the rows of its
 * chunk's key range only).  drx_shard_gather_rows: the requested rows + scalars into an exchange buffer of the geometry above
 * (segment after segment). */
size_t drx_shard_owner_table_bytes(const DrxShard *sh, int32_t n_segments);
int drx_shard_owner_index(const DrxShard *sh, const uint32_t *recv_keys, int32_t n, const int32_t *recv_counts, int32_t n_segments,
                          int32_t chunk, void *table, size_t table_bytes, void *stream);
int drx_shard_gather_rows(const DrxCdaeParams *p, const DrxShard *sh, const uint32_t *recv_keys, int32_t n, const int32_t *recv_counts,
                          int32_t n_segments, float *out, void *stream);
/* Requester side, three launches: forward + backward of the local triples against the received rows (`rows_cache`; V rows and W2T
 * gradient rows only one triple touches are finished there), the planned segmented reduction and its span launch: one summed
 * gradient row per distinct item row into `grad_send` (same geometry as rows_cache), shared V rows updated in place, the bias
 * gradient + loss sum into the sentinel rows.  Losses and L2 are normalised by b_norm, the GLOBAL batch size.
 * events: NULL or 4 hipEvent_t recorded before / between / after the launches. */
size_t drx_shard_step_scratch_bytes(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots);
int drx_shard_step_local(const DrxCdaeParams *p, const DrxOptim *opt, const DrxShard *sh, const DrxHistory *hist, const DrxBatch *bt,
                         const void *prepared, size_t prepared_bytes, const float *rows_cache, float *grad_send, int32_t b_norm,
                         int32_t loss_kind, void *scratch, size_t scratch_bytes, void *const *events, void *stream);
/* Owner side, one exchange chunk per call: sum the gradient rows received for each owned row of the chunk in segment order and apply
 * the optimizer ONCE per row; with the LAST chunk (chunk == chunks - 1) one extra workgroup sums the sentinel rows in segment order,
 * updates b and writes loss_out[0] = global loss sum / b_norm (loss_out may be NULL).  `table` = what drx_shard_owner_index built from
 * the same keys.  With DRX_SHARD_SELF_BYPASS: own_grad[m] = the grad_send buffer of the step's micro-batch m, own_off[m] = float offset
 * of the rank's own piece OF THIS CHUNK in it; otherwise both NULL. */
int drx_shard_apply(const DrxCdaeParams *p, const DrxOptim *opt, const DrxShard *sh, int32_t b_norm, const uint32_t *recv_keys,
                    const float *grad_recv, int32_t n, const int32_t *recv_counts, int32_t n_segments, int32_t chunk, const void *table,
                    const float *const *own_grad, const int64_t *own_off, float *loss_out, void *stream);

/* ---- RCCL transport of the row-sharded step (no reference equivalent; SURVEY §8b allows this one piece of state) ------------------------
 * One communicator per rank (process) with a HIP stream of its own.  drx_comm_unique_id on one rank, the 128 bytes handed to the others
 * by the host (torch.distributed's store, a file, ...), drx_comm_create on every rank with its device current.  librccl is opened at run
 * time: without it these calls return DRX_ECOMM and everything else in the library works.
 * drx_comm_alltoallv: peer p is sent send[send_off[p] .. + send_bytes[p]) and this rank receives recv_bytes[p] bytes from it at
 *   recv + recv_off[p] (HOST arrays of `world` entries; zero sizes allowed, the rank itself included) — one group of ncclSend / ncclRecv
 *   pairs on the communicator's stream, behind everything `after_stream` has queued so far.  Returns a ticket (>= 0) or a negative code.
 * drx_comm_wait: `stream` waits for the exchange with that ticket (and, the communicator's stream being in order, all before it).
 * The buffers must stay allocated until a stream that waited for the ticket has passed that point.
 * DRX_COMM_THREAD: the nccl* calls are made by a thread of the communicator's own (drx_comm_alltoallv only posts the request; the buffers'
 * addresses and sizes are copied); drx_comm_wait then first waits (on the host, microseconds) until that thread has enqueued the
 * exchange.  A failure of the issuing thread is returned by the next drx_comm_* call. */
#define DRX_COMM_ID_BYTES 128
#define DRX_COMM_THREAD 1u
typedef struct DrxComm DrxComm;
int drx_comm_unique_id(void *id128);
int drx_comm_create(const void *id128, int32_t world, int32_t rank, uint32_t flags, DrxComm **out);
int drx_comm_destroy(DrxComm *c);
void *drx_comm_stream(DrxComm *c);
int64_t drx_comm_alltoallv(DrxComm *c, const void *send, const int64_t *send_off, const int64_t *send_bytes, void *recv,
                           const int64_t *recv_off, const int64_t *recv_bytes, void *after_stream);
int drx_comm_wait(DrxComm *c, int64_t ticket, void *stream);
const char *drx_comm_last_error(void);

/* ---- the exchange PHASES of a row-sharded step, issued from C (r06; no reference equivalent) -------------------------------------------
 * What drecpy_amd/dist.py does between the drx_shard_* launches — offsets of every unit's piece, one drx_comm_alltoallv per chunk, the
 * waits — as four calls per step with the split sizes READ FROM THE COUNT EXCHANGE'S PINNED MAILBOX: the chunked schedule of a step is
 * 2 + 3 C exchanges, 2 C waits and 3 C launches, and issued from Python the host was the next wall behind the links.
 * One micro-batch per step; one DrxShardExchange per prepared batch, filled by the caller:
 *   send_counts / recv_counts  HOST arrays [world x chunks] as the count exchange delivers them: send_counts[o * chunks + c] = rows
 *                              (sentinel included) this rank asks of owner o in chunk c, recv_counts[s * chunks + c] = rows rank s asks
 *                              of this rank in chunk c
 *   uniq                       device: the rank's distinct wire keys (drx_shard_prepare)
 *   req                        device: the keys this rank receives, chunk after chunk, per chunk source after source (sizes[2] keys)
 *   table                      device: drx_shard_owner_table_bytes(sh, world)
 *   rows_cache, grad_send      device: the requester's exchange buffers (sizes[0] floats each; geometry: "EXCHANGE BUFFER" above)
 *   rows_send, grad_recv       device: the owner's (sizes[1] floats each): chunk after chunk, per chunk one segment per source rank
 *   rows_ticket / grad_ticket  written by the phases: the communicator tickets of the chunk's row / gradient exchange
 * drx_shard_exchange_sizes: sizes4 = { requester floats, owner floats, keys received, keys sent } (every buffer: at least 32 elements).
 * drx_shard_phase_keys  (parameter-independent, on the run-ahead stream): per chunk the key all-to-all, then drx_shard_owner_index.
 * drx_shard_phase_rows  one chunk: drx_shard_gather_rows of the rows asked of this rank as they are NOW, then their all-to-all
 *                       (-> rows_ticket[chunk]).  Head of a step for all chunks, or — pipelined — by drx_shard_phase_tail.
 * drx_shard_phase_local `stream` waits for the row tickets, then drx_shard_step_local (events as there).
 * drx_shard_phase_tail  posts the gradient all-to-all of every chunk; then chunk by chunk: wait, drx_shard_apply, and — `next` not NULL —
 *                       drx_shard_phase_rows(next, chunk): the rows of a chunk leave for the NEXT step right behind their update. */
typedef struct DrxShardExchange {
  const int64_t *send_counts;
  const int64_t *recv_counts;
  const uint32_t *uniq;
  uint32_t *req;
  void *table;
  size_t table_bytes;
  float *rows_cache;
  float *rows_send;
  float *grad_send;
  float *grad_recv;
  int64_t rows_ticket[DRX_MAX_CHUNKS];
  int64_t grad_ticket[DRX_MAX_CHUNKS];
} DrxShardExchange;
int drx_shard_exchange_sizes(const DrxCdaeParams *p, const DrxShard *sh, const int64_t *send_counts, const int64_t *recv_counts,
                             int64_t *sizes4);
/* the phases' geometry for tests (host arithmetic only): out[12 world + 3], see csrc/drx_shard_phase.cpp */
int drx_shard_phase_layout(const DrxCdaeParams *p, const DrxShard *sh, const int64_t *send_counts, const int64_t *recv_counts, int32_t chunk,
                           int64_t *out);
int drx_shard_phase_keys(const DrxShard *sh, DrxComm *comm, DrxShardExchange *x, void *stream);
int drx_shard_phase_rows(const DrxCdaeParams *p, const DrxShard *sh, DrxComm *comm, DrxShardExchange *x, int32_t chunk, void *stream);
int drx_shard_phase_local(const DrxCdaeParams *p, const DrxOptim *opt, const DrxShard *sh, const DrxHistory *hist, const DrxBatch *bt,
                          DrxComm *comm, DrxShardExchange *x, const void *prepared, size_t prepared_bytes, int32_t b_norm,
                          int32_t loss_kind, void *scratch, size_t scratch_bytes, void *const *events, void *stream);
int drx_shard_phase_tail(const DrxCdaeParams *p, const DrxOptim *opt, const DrxShard *sh, DrxComm *comm, DrxShardExchange *x,
                         DrxShardExchange *next, int32_t b_norm, float *loss_out, void *stream);

/* drx_copy_f4: dst[0 .. n_bytes) = src[0 .. n_bytes) on the device (16-B aligned, n_bytes a multiple of 16, no overlap): a streaming
 *   float4 copy kernel — table snapshots (recommender_abc.py:336-352 keeps a copy of every weight per epoch), and the rate bench.py
 *   reports as `hbm_copy_achievable` (the achievable HBM rate measured on the box next to the nominal peak). */
int drx_copy_f4(void *dst, const void *src, size_t n_bytes, void *stream);
/* the same with the kernel's form chosen by the caller (0 .. 4: csrc/drx_generic.hip; scripts/copy_bench.py times them side by side) */
int drx_copy_f4_variant(void *dst, const void *src, size_t n_bytes, int32_t variant, void *stream);

/* ---- model-independent pieces of the dense (Keras-Adam) steps of DMF / Caser ------------------------------------
 * drx_adam_dense: p, m, v [n] (16-B aligned): g_total = g + l2_coef * p (g may be NULL); TF ApplyAdam update with the
 *   given lr_t `alpha`.  One call = one optimizer.apply_gradients on one variable (recommender_abc.py:328-334). */
int drx_adam_dense(float *p, float *m, float *v, const float *g, int64_t n, float alpha, float l2_coef, float beta1, float beta2,
                   float eps, void *stream);
/* drx_scatter_rows: out[key] = sum over touches t with keys[t] == key of coef[t] * src[src_index[t]]  (and
 *   out_s[key] = sum coef[t] * src_s[src_index[t]]), summed in touch order (deterministic).  Rows of `out` that no
 *   touch names are left untouched (zero them first).  keys may hold DRX_KEY_NONE (ignored).  This is the gradient
 *   of an embedding lookup (tf.nn.embedding_lookup / Keras Embedding, caser.py:99-100,117-118; dmf.py:89-90 first layer). */
size_t drx_scatter_scratch_bytes(int32_t ld, int32_t n_touches, int32_t n_rows);
/* The same gradient for a table whose optimizer is DENSE (Keras Adam on an Embedding / Dense kernel: every row's moments decay every
 * step), fused with that optimizer's update — replaces drx_scatter_rows + drx_adam_dense (tape.gradient through the lookup and
 * apply_gradients, recommender_abc.py:203-204, 328-334; caser.py:47-50, 66-69) without touch keys on the device, a sort or a zeroed
 * gradient table.  row_ptr [n_rows + 1] / order [T]: the lookups grouped by the row they name, a row's lookups in batch order
 * (drx_batch_csr on the host; device copies here).  Row r: g = sum of src[order[q]] for q in [row_ptr[r], row_ptr[r + 1]), ascending;
 * p, m, v <- ApplyAdam(g + l2_coef * p) with lr_t = alpha.  src_s / p_s / m_s / v_s (all or none): one scalar per lookup / row
 * updated the same way with alpha_s and no l2 (caser.py:69's dense_1_b next to dense_1_W). */
int drx_rows_csr_adam(const int32_t *row_ptr, const int32_t *order, const float *src, const float *src_s, int32_t ld, int32_t n_rows,
                      float *p, float *m, float *v, float *p_s, float *m_s, float *v_s, float alpha, float alpha_s, float l2_coef,
                      float beta1, float beta2, float eps, void *stream);
/* The same where the gradient row of lookup o is an OUTER PRODUCT the producer did not write out: scale[o] * src[o / group]
 * (src [T / group, ld]; `group` consecutive lookups share a row of src), and scale[o] itself is the lookup's scalar gradient (p_s, m_s,
 * v_s required).  Caser's dense_1: the gradient of dense_1_W[n] through target j of sample b is dscore[b, j] * [dense_0 output | user
 * row](b) (caser.py:115-120) — drx_caser_fwd_bwd with dW1 == NULL writes the B hidden rows (cat_out) and the B * Tp score gradients
 * (db1) instead of B * Tp rows: 1.6 MB instead of 19.7 MB at examples/caser.py's batch of 4096. */
int drx_rows_csr_adam_outer(const int32_t *row_ptr, const int32_t *order, const float *scale, const float *src, int32_t group, int32_t ld,
                            int32_t n_rows, float *p, float *m, float *v, float *p_s, float *m_s, float *v_s, float alpha, float alpha_s,
                            float l2_coef, float beta1, float beta2, float eps, void *stream);
/* Several tables in ONE launch (ld <= 256 each): the arguments of drx_rows_csr_adam per table; group > 0 selects the outer-product form
 * of drx_rows_csr_adam_outer (scale required), group == 0 the plain one (scale = the optional per-lookup scalars src_s). */
#define DRX_MAX_CSR_TABLES 4
typedef struct DrxCsrAdamTable {
  const int32_t *row_ptr, *order;
  const float *src, *scale;
  int32_t group, ld, n_rows;
  float *p, *m, *v, *p_s, *m_s, *v_s;
  float alpha, alpha_s, l2_coef;
} DrxCsrAdamTable;
int drx_rows_csr_adam_multi(const DrxCsrAdamTable *tables, int32_t n_tables, float beta1, float beta2, float eps, void *stream);
/* The dense family with the update rule as an argument (DrxOptRule above): the `_adam` entry points are these with
 * {DRX_OPT_ADAM, alpha, beta1, beta2, eps}, bit for bit.  s1 / s2 (and s1_s / s2_s, DrxCsrAdamTable's m / v / m_s / v_s) are the slots the
 * rule has; one the rule lacks is passed as NULL and never dereferenced, one it has must be there (DRX_EINVAL).  Every row / element is
 * updated every step, also a table row no lookup names (g = l2_coef * p: its accumulators decay or advance as in Keras's dense
 * apply).  Nothing is launched when DRX_EINVAL is returned.
 *   drx_opt_dense          drx_adam_dense's sweep; step size rule->lr
 *   drx_rows_csr_opt       drx_rows_csr_adam; step sizes alpha / alpha_s
 *   drx_rows_csr_opt_outer drx_rows_csr_adam_outer
 *   drx_rows_csr_opt_multi drx_rows_csr_adam_multi; one rule for all tables of the call, step sizes from the tables */
int drx_opt_dense(float *p, float *s1, float *s2, const float *g, int64_t n, const DrxOptRule *rule, float l2_coef, void *stream);
int drx_rows_csr_opt(const int32_t *row_ptr, const int32_t *order, const float *src, const float *src_s, int32_t ld, int32_t n_rows,
                     float *p, float *s1, float *s2, float *p_s, float *s1_s, float *s2_s, float alpha, float alpha_s, float l2_coef,
                     const DrxOptRule *rule, void *stream);
int drx_rows_csr_opt_outer(const int32_t *row_ptr, const int32_t *order, const float *scale, const float *src, int32_t group, int32_t ld,
                           int32_t n_rows, float *p, float *s1, float *s2, float *p_s, float *s1_s, float *s2_s, float alpha,
                           float alpha_s, float l2_coef, const DrxOptRule *rule, void *stream);
int drx_rows_csr_opt_multi(const DrxCsrAdamTable *tables, int32_t n_tables, const DrxOptRule *rule, void *stream);
/* host: first[c] = first position of code c in codes[0..n), -1 when absent; returns the number of distinct codes (Dataset.unique on
 * dense integer code columns, mem_dataset.py's drop_duplicates, without a sort) */
int64_t drx_first_occurrence(const int64_t *codes, int64_t n, int64_t n_codes, int64_t *first);
/* host: 1 as soon as *p >= at_least, 0 after poll_us microseconds of polling (the hand-over between fit()'s issuing thread and its
 * sampling worker thread: drecpy_amd/_spinpool.py; recommender_abc.py:186-188 draws the batch inline) */
int drx_spin_until(const int64_t *p, int64_t at_least, int32_t poll_us);
/* host: keys [T] in [0, n_rows) -> row_ptr [n_rows + 1], order [T] (stable counting sort) */
int drx_batch_csr(const int32_t *keys, int32_t T, int32_t n_rows, int32_t *row_ptr, int32_t *order);
/* The same on the DEVICE, for up to DRX_MAX_CSR_TABLES key lists in one go (batches drawn on the device: Caser.fit(device_sampler=True)
 * then takes the fused drx_rows_csr_adam_multi update too, instead of scatter + dense Adam per table): ONE stable sort of all lists'
 * (row, lookup) pairs, row_ptr by a binary search per row.  keys must lie in [0, n_rows) (not checked on the device).
 * scratch: drx_batch_csr_device_bytes (0 = invalid description). */
typedef struct DrxCsrList {
  const int32_t *keys;       /* device [T] */
  int32_t T, n_rows;
  int32_t *row_ptr, *order;  /* device [n_rows + 1], [T] */
} DrxCsrList;
size_t drx_batch_csr_device_bytes(const DrxCsrList *lists, int32_t n_lists);
int drx_batch_csr_device(const DrxCsrList *lists, int32_t n_lists, void *scratch, size_t scratch_bytes, void *stream);
int drx_scatter_rows(const uint32_t *keys, int32_t T, const float *src, const uint32_t *src_index, const float *coef,
                     const float *src_s, int32_t ld, int32_t n_rows, float *out, float *out_s, void *scratch,
                     size_t scratch_bytes, void *stream);
/* drx_sumsq: out[0] (+)= sum_i x[i]^2, accumulated in double in a fixed order; out = device double [1 + 1024] (out[1..] is scratch).
 * The VALUE of an L2 term for the loss log (cdae.py:82 tf.nn.l2_loss, the Keras l2 regularizers of dmf.py / caser.py) — the training
 * path never needs it (the update kernels apply reg * p themselves). */
int drx_sumsq(const float *x, int64_t n, double *out, int32_t accumulate, void *stream);
/* drx_rows_dot: out[b, n] = x[b, :] . table[n, :] + bias[n]   (all-item scoring, caser.py:137) */
int drx_rows_dot(const float *x, int32_t B, const float *table, int32_t n_rows, int32_t ld, const float *bias, float *out,
                 void *stream);

/* Adam over up to DRX_MAX_SEGMENTS slices of one flat array, each with its own Keras lr_t and L2 coefficient: the
 * small conv/dense weights of a model, one slice per registered layer kernel / bias (recommender_abc.py:328-334). */
#define DRX_MAX_SEGMENTS 24   /* (Caser with L = 8: 2 L + 4 = 20 registered kernels and biases) */
typedef struct DrxAdamSegments {
  int32_t n;
  int32_t start[DRX_MAX_SEGMENTS], len[DRX_MAX_SEGMENTS];
  float alpha[DRX_MAX_SEGMENTS], l2_coef[DRX_MAX_SEGMENTS];
} DrxAdamSegments;
int drx_adam_segments(float *p, float *m, float *v, const float *g, const DrxAdamSegments *sg, float beta1, float beta2, float eps,
                      void *stream);
/* The same under any dense rule (DrxOptRule; step size per segment from sg->alpha, rule->lr ignored); s1 / s2: the slots the rule has,
 * NULL where it has none.  drx_adam_segments is this with {DRX_OPT_ADAM, -, beta1, beta2, eps}. */
int drx_opt_segments(float *p, float *s1, float *s2, const float *g, const DrxAdamSegments *sg, const DrxOptRule *rule, void *stream);

/* ---- Caser (DRecPy/Recommender/caser.py) ------------------------------------------------------------------------
 * Tables: item_emb [N, ld], user_emb [U, ld] (caser.py:47-50), W1 [N, ld2] = dense_1_W rows (first d columns meet
 * dense_0's output, the next d the user embedding, caser.py:66,115-120), b1 [N] (caser.py:69).  Small weights `sw`
 * (one flat array, channel-fastest): conv_v kernel [L][n_v][ld] at off_kv + bias [n_v] at off_bv (caser.py:53);
 * convs_h[i] kernel [i+1][n_h][ld] at off_kh[i] + bias [n_h] at off_bh[i] (caser.py:55-58); dense_0 kernel
 * [n_v + L*n_h][ld] at off_wd + bias [ld] at off_bd (caser.py:63). */
enum { DRX_ACT_RELU = 0, DRX_ACT_TANH = 1, DRX_ACT_SIGMOID = 2, DRX_ACT_LINEAR = 3 };
typedef struct DrxCaserDims {
  int32_t L, T, Tp, d, ld, ld2, n_v, n_h, n_small;   /* Tp = T + T*neg_ratio targets per sample */
  int32_t off_kv, off_bv, off_kh[8], off_bh[8], off_wd, off_bd;
  int32_t act_h, act_mlp;   /* DRX_ACT_*: activation of the horizontal convolutions and of dense_0 (caser.py:29-30; default relu) */
} DrxCaserDims;
typedef struct DrxCaserArgs {
  const float *item_emb, *user_emb, *W1, *b1, *sw;
  const int32_t *uid;      /* [B] */
  const int32_t *before;   /* [B, L]  last L items (caser.py:79-83) */
  const int32_t *after;    /* [B, Tp] T targets then T*neg negatives */
  const uint8_t *keep;     /* [B, n_v + L*n_h] dropout keep mask (TF's RNG cannot be reproduced) or NULL = no dropout */
  float rate;
  int32_t B;
  float *dE;               /* [B*L, ld]   gradient row of every item lookup */
  float *dW1;              /* [B*Tp, ld2] gradient row of every dense_1_W lookup = db1[row] * cat_out[row / Tp]; NULL: not written
                            * (cat_out required then: drx_rows_csr_adam_outer forms the rows where it sums them) */
  float *db1;              /* [B*Tp] */
  float *dPu;              /* [B, ld]     gradient row of every user lookup */
  float *gsw_part;         /* [drx_caser_grid(), n_small] */
  float *loss_part;        /* [drx_caser_grid()] */
  float *cat_out;          /* [B, ld2] [dense_0 output | user row] of every sample: drx_caser_hidden; drx_caser_fwd_bwd when non-NULL */
  uint64_t mask_seed;      /* keep == NULL and rate > 0: dropout keeps element (b, j) iff drx_hash_u32(mask_seed, b, j) >= rate * 2^32 —
                            * a counter-based mask evaluated in the kernel (TF's dropout stream cannot be reproduced either way) */
} DrxCaserArgs;
int drx_caser_grid(const DrxCaserDims *D, int32_t B);
/* forward + Keras BCE + backward (caser.py:86-120 under the tape of recommender_abc.py:191-203): fills the lookup
 * gradient rows above and gsw_out[0..n_small) = gradient of the small weights, gsw_out[n_small] = prediction loss. */
int drx_caser_fwd_bwd(const DrxCaserDims *D, const DrxCaserArgs *A, float *gsw_out, void *stream);
/* The same followed by the small weights' update in the launch that sums the workgroups' partial gradients: gsw_out as above, then
 * sw, sw_m, sw_v <- l2 + Keras Adam per segment (drx_adam_segments' arithmetic; sw must be A->sw: the step's own weights, updated in
 * place once the training kernel has read them). */
int drx_caser_step_small(const DrxCaserDims *D, const DrxCaserArgs *A, float *gsw_out, float *sw, float *sw_m, float *sw_v,
                         const DrxAdamSegments *sg, float beta1, float beta2, float eps, void *stream);
/* The same under any dense rule (DrxOptRule; drx_opt_segments' arithmetic, step size per segment from sg->alpha): sw_s1 / sw_s2 are the
 * slots the rule has, NULL where it has none.  drx_caser_step_small is this with {DRX_OPT_ADAM, -, beta1, beta2, eps}. */
int drx_caser_step_small_opt(const DrxCaserDims *D, const DrxCaserArgs *A, float *gsw_out, float *sw, float *sw_s1, float *sw_s2,
                             const DrxAdamSegments *sg, const DrxOptRule *rule, void *stream);
/* inference hidden state cat_out[b] = [dense_0 output | user embedding] (caser.py:97-115 with training=False) */
int drx_caser_hidden(const DrxCaserDims *D, const DrxCaserArgs *A, void *stream);

/* ---- DMF (DRecPy/Recommender/dmf.py) ---------------------------------------------------------------------------
 * Tower 0 = user_nn (input: the user's interaction ROW over items), tower 1 = item_nn (input: the item's COLUMN over
 * users), both l2-normalised when l2_norm_vectors (dmf.py:75-86).  First-layer kernels K0u [n_items, ld0[0]] and
 * K0i [n_users, ld0[1]] are tables; every other weight lives in one flat array `sw`: layer l >= 1 kernel [f[l-1]][f[l]]
 * at off_k[tw][l], layer l >= 0 bias [f[l]] at off_b[tw][l].  Layer widths <= 64, <= 4 layers per tower.
 * gsw_out of drx_dmf_fwd_bwd holds the gradient of `sw` slot for slot (the scalar at off_scale included). */
typedef struct DrxDmfDims {
  int32_t n_layers[2];
  int32_t f[2][4];
  int32_t ld0[2];
  int32_t off_k[2][4], off_b[2][4];
  int32_t n_small;
  int32_t l2_norm_vectors;
  int32_t off_scale;         /* offset in `sw` of a registered scalar that multiplies every prediction, or -1: the extra
                              * tf.Variable of examples/extending_recommender_dmf.py:9-18 (ModifiedDMF, BASELINE config 3) */
} DrxDmfDims;
typedef struct DrxDmfArgs {
  const float *K0u, *K0i, *sw;
  const int64_t *u_indptr; const int32_t *u_indices; const float *u_values;   /* CSR [U, N], raw interaction values */
  const int64_t *i_indptr; const int32_t *i_indices; const float *i_values;   /* CSC (= CSR of the transpose) [N, U] */
  const int32_t *uid, *iid;  /* [B] */
  const float *y;            /* [B] targets (standardised when use_nce, dmf.py:69) */
  int32_t target_mode;       /* 0: BCE(y[b], pred[b]) (dmf.py:98-99).  1: BCE(y_mean, pred[b]) = the mean of Keras' (B,B) broadcast of
                              * (B,) targets against (B,1) predictions (ModifiedDMF's list of (1,)-tensors) */
  float y_mean;              /* mean of y over the batch (target_mode 1) */
  const int32_t *off_u, *off_i;   /* [B+1] prefix sums of the row / column lengths of the batch */
  int32_t B;
  float *dz0u, *dz0i;        /* [B, ld0] gradient wrt the first-layer pre-activation */
  uint32_t *tkeys_u, *tsrc_u; float *tcoef_u;   /* [off_u[B]] first-layer touches: kernel row, sample, input value */
  uint32_t *tkeys_i, *tsrc_i; float *tcoef_i;   /* [off_i[B]] */
  float *gsw_part, *loss_part;                  /* [drx_dmf_grid(B), n_small], [drx_dmf_grid(B)] */
  float *pred_out;           /* [B]      (drx_dmf_predict) max(1e-6, cosine) */
  float *rep_u_out, *rep_i_out;   /* [B, 64] (drx_dmf_predict, optional) l2-normalised tower outputs */
  float *work;               /* drx_dmf_work_bytes(B) bytes (drx_dmf_fwd_bwd): per-id first-layer sums, per-sample activations and
                              * pre-activation gradients handed from the gather kernel to the dense one and to the weight-gradient one */
  /* drx_dmf_fwd_bwd works on the DISTINCT users / items of the batch (a tower's first layer depends on the id alone): there
   * uid [n_du] / iid [n_di] hold the distinct ids, off_u [n_du+1] / off_i [n_di+1] their touch offsets, dz0u [n_du, ld0] / dz0i
   * [n_di, ld0] and the touches' sample field refer to distinct ids, and
   *   inv_u / inv_i [B]        : index of sample b's user / item among the distinct ones
   *   gptr_* [n_d+1], grows_* [B] : CSR of the samples per distinct id, samples ascending (order of the gradient sums)
   * (drx_dmf_predict takes uid / iid per pair as before and ignores these) */
  const int32_t *inv_u, *inv_i, *gptr_u, *gptr_i, *grows_u, *grows_i;
  int32_t n_du, n_di;
  /* Alternative to the touches (tkeys_* / tsrc_* / tcoef_* / off_* may then be NULL): drx_dmf_fwd_bwd records, for every distinct id
   * of the batch, map[id] = (stamp << 32) | its distinct index, for drx_dmf_k0_update.  map_u [n_users] / map_i [n_items]:
   * zero-initialised ONCE by the caller, never cleared; stamp: non-zero and different in every step. */
  unsigned long long *map_u, *map_i;
  /* l2 normalisers of every user row [n_users] / item column [n_items] of the interaction matrix (dmf.py:75-86), computed once per
   * dataset by drx_dmf_norms: required with the maps, optional otherwise (NULL: drx_dmf_fwd_bwd forms them per batch id) */
  const float *rho_u, *rho_i;
  uint32_t stamp;
  /* A batch prepared ON THE DEVICE (drx_dmf_batch_distinct_device): the numbers of distinct ids and the batch mean of y are only known
   * there.  nd_dev [2] = {n_du, n_di} (n_du / n_di above then are upper bounds that size the launches), y_mean_dev [1]; or NULL. */
  const int32_t *nd_dev;
  const float *y_mean_dev;
  /* r06, optional (NULL: one work item per distinct id, in their own order; ignored with nd_dev): the first-layer gather's n_work work
   * items, entry = distinct index (users 0 .. n_du - 1, items n_du ..) | segment << 24.  LONGEST rows / columns FIRST — the gather of a
   * popular item's column (thousands of non-zeros) is the launch's critical path when it happens to start late — and long ones CUT
   * into segments of seg_len non-zeros (0: uncut): segment 0 leaves the id's first-layer sum, segment g > 0 the partial row
   * zpart[(zseg[i] >> 8) + g - 1] (rows of 64 floats per unit slot), which the dense kernel adds in segment order (zseg[i] & 255 of
   * them).  drx_dmf_work_order builds order and zseg on the host. */
  const int32_t *work_order;
  int32_t n_work, seg_len;
  const int32_t *zseg;
  float *zpart;
  /* the list built on the DEVICE (drx_dmf_work_order_device, for batches prepared there: nd_dev set): n_work_dev [2] = {its entries, its
   * partial rows} — n_work above is then the list's CAPACITY and sizes the launch; a list of NO partial rows is read as uncut whatever
   * seg_len says (the device decides that after the host filled this struct); zpart holds the partial rows that list can have (at most
   * 2 nnz / seg_len).  NULL: a host-built list (ignored with nd_dev), or none */
  const int32_t *n_work_dev;
} DrxDmfArgs;
/* Host helper for DrxDmfArgs::work_order / zseg: the gather's work items (distinct users 0 .. n_u - 1 with off_u[i + 1] - off_u[i]
 * non-zeros, then distinct items), ordered by the bit length of their degree, descending, stable inside a class — O(n) — and cut into
 * segments of at most seg_len non-zeros (0: uncut): entry = work index | segment << 24; zseg[i] = first partial row << 8 | number of
 * partial rows of work index i (0: none).  Returns the number of entries, DRX_ESCRATCH when they exceed order_cap (use seg_len = 0
 * then), DRX_EINVAL when a row would need more than 255 segments; *n_part = partial rows. */
int32_t drx_dmf_work_order(const int32_t *off_u, int32_t n_u, const int32_t *off_i, int32_t n_i, int32_t seg_len, int32_t *order,
                           int32_t order_cap, int32_t *zseg, int32_t *n_part);
/* The same list for a batch whose distinct ids live on the device (drx_dmf_batch_distinct_device: du / di, nd_dev = {n_du, n_di}): degrees
 * from the interaction matrix's two index pointers, one workgroup, classes by bit length of the degree (descending; inside a class in no
 * particular order: a work item writes its own row, the result does not depend on the order).  out2 = {entries, partial rows}.  A
 * caller that wants segments guarantees that the entries fit — order_cap >= 2 B + 2 nnz / seg_len (every distinct id brings its own row or
 * column once) — and that no id needs more than 255 of them (seg_len >= longest row or column / 255).  Where either does not hold the
 * WHOLE list comes out uncut instead (the host helper's DRX_ESCRATCH / DRX_EINVAL, answered on the device): one entry per distinct id,
 * every zseg 0, out2 = {n_du + n_di, 0}, which the gather reads as seg_len = 0.  order_cap >= n_du + n_di always. */
int drx_dmf_work_order_device(const int64_t *u_indptr, const int64_t *i_indptr, const int32_t *du, const int32_t *di, const int32_t *nd_dev,
                              int32_t seg_len, int32_t *order, int32_t order_cap, int32_t *zseg, int32_t *out2, void *stream);
/* Host helper for the arrays above: the distinct ids of a batch, ascending.  distinct [<= B], inv [B], gptr [<= B+1], grows [B],
 * off [<= B+1] (prefix sums of indptr row lengths of the distinct ids; NULL to skip) are host arrays;
 * scratch = int32 [n_rows], all -1 on entry and again on return (the caller keeps it between steps).  Returns the number of distinct
 * ids, or a negative DRX_E* code (an id outside [0, n_rows); DRX_EINVAL when the prefix sums do not fit int32 — touch offsets would overlap). */
int32_t drx_batch_distinct(const int32_t *ids, int32_t B, int32_t n_rows, const int64_t *indptr, int32_t *scratch, int32_t *distinct,
                           int32_t *inv, int32_t *gptr, int32_t *grows, int32_t *off);
/* The same on the device, both towers at once, for batches drawn there (DMF.fit(device_sampler=True)): uid / iid / y [B] device
 * arrays in; du, di [B], inv_u, inv_i [B], gptr_u, gptr_i [B + 1], grows_u, grows_i [B], nd [2] = {distinct users, distinct items},
 * y_mean [1] out — what DrxDmfArgs wants (uid = du, iid = di, nd_dev = nd, y_mean_dev = y_mean).  One stable sort of the 2B
 * (id, sample) pairs + one workgroup that numbers the runs.  n_users + n_items < 2^31, B <= 2^20. */
size_t drx_dmf_distinct_scratch_bytes(int32_t B, int32_t n_users, int32_t n_items);
int drx_dmf_batch_distinct_device(const int32_t *uid, const int32_t *iid, const float *y, int32_t B, int32_t n_users, int32_t n_items,
                                  int32_t *du, int32_t *di, int32_t *inv_u, int32_t *inv_i, int32_t *gptr_u, int32_t *gptr_i,
                                  int32_t *grows_u, int32_t *grows_i, int32_t *nd, float *y_mean, void *scratch, size_t scratch_bytes,
                                  void *stream);
/* out[id] = 1 / max(|row id|_2, 1e-6) (1 when l2_norm_vectors == 0) for the n rows of a CSR, with the summation order of the towers */
int drx_dmf_norms(const DrxDmfDims *D, const int64_t *indptr, const float *values, int32_t n, float *out, void *stream);
int drx_dmf_grid(int32_t B);      /* rows of gsw_part / entries of loss_part */
size_t drx_dmf_work_bytes(int32_t B);
/* forward + Keras BCE + backward (dmf.py:88-99 under the tape): dz0 rows + touches for drx_scatter_rows,
 * gsw_out[0..n_small) small-weight gradients, gsw_out[n_small] = prediction loss */
int drx_dmf_fwd_bwd(const DrxDmfDims *D, const DrxDmfArgs *A, float *gsw_out, void *stream);
/* The same with the small weights' Keras Adam (what drx_adam_segments does with gsw_out afterwards) in the launch that sums the chunks'
 * partial gradients: one launch less per step (r06; drx_dmf_k0_update reads none of `sw` and may follow). */
int drx_dmf_step_small(const DrxDmfDims *D, const DrxDmfArgs *A, float *gsw_out, float *sw, float *sw_m, float *sw_v,
                       const DrxAdamSegments *sg, float beta1, float beta2, float eps, void *stream);
/* The same under any dense rule (DrxOptRule; drx_opt_segments' arithmetic, step size per segment from sg->alpha): sw_s1 / sw_s2 are the
 * slots the rule has, NULL where it has none.  drx_dmf_step_small is this with {DRX_OPT_ADAM, -, beta1, beta2, eps}. */
int drx_dmf_step_small_opt(const DrxDmfDims *D, const DrxDmfArgs *A, float *gsw_out, float *sw, float *sw_s1, float *sw_s2,
                           const DrxAdamSegments *sg, const DrxOptRule *rule, void *stream);
int drx_dmf_predict(const DrxDmfDims *D, const DrxDmfArgs *A, void *stream);
/* The update of the first-layer kernels (tf.keras Dense kernels [N, f0] of user_nn / [U, f0] of item_nn, dmf.py:44-60) after
 * drx_dmf_fwd_bwd ran with the id maps: gradient (+ l2_coef * K0, dmf.py:101-103) and dense Keras Adam in one pass over both tables —
 * replaces recommender_abc.py:328-334 for these two variables without a touch list, sort or gradient arena.  Row n of K0u collects
 * from column n of the interaction matrix (i_* of A) the entries whose user carries this step's stamp in map_u; K0i likewise from
 * u_* and map_i.  Cost per step: one walk over all non-zeros (8 bytes each) — pays while nnz is within ~64x the batch's touches;
 * beyond that use the touches + drx_scatter_rows + drx_adam_dense. */
typedef struct DrxDmfK0Update {
  float *K0u, *m_u, *v_u;    /* [n_items, ld0[0]] kernel, Adam moments (another rule: its slots s1, s2; NULL where it has none) */
  float *K0i, *m_i, *v_i;    /* [n_users, ld0[1]] */
  int32_t n_items, n_users;
  float alpha_u, alpha_i;    /* Keras-Adam lr_t of the apply_gradients call each kernel belongs to */
  float l2_coef, beta1, beta2, eps;
  /* r06, optional (NULL: rows in table order, a workgroup each): a permutation of 0 .. n_items + n_users - 1 (K0u rows, then K0i rows),
   * the rows with the longest columns / rows of the interaction matrix first (static per dataset).  Its first n_long rows take a
   * workgroup each — every row whose walk is longer than 1024 entries must be among them —, the others a WAVE each, four per workgroup. */
  const int32_t *row_order;
  int32_t n_long;
  /* the update rule, a dense DRX_OPT_* (0 = DRX_OPT_ADAM: a zero-initialised field is the update this was).  Another rule reads alpha_u /
   * alpha_i as its learning rate, beta1 as DrxOptRule's mu (momentum), beta2 as mu2 (rho), and the slots it has in m_* (s1) and v_* (s2). */
  int32_t opt_kind;
} DrxDmfK0Update;
int drx_dmf_k0_update(const DrxDmfDims *D, const DrxDmfArgs *A, const DrxDmfK0Update *up, void *stream);
/* all-pairs cosine scores on the matrix cores: out[u, n] = max(1e-6, ru[u,:kdim] . ri[n,:kdim]) with bf16 operands /
 * fp32 accumulation (v_mfma_f32_32x32x16_bf16); ru, ri = l2-normalised tower outputs, kdim % 16 == 0 (dmf.py:92-95
 * evaluated for a block of users against all items instead of one _predict per pair, recommender_abc.py:460). */
int drx_score_pairs_bf16(const float *ru, int32_t n_u, const float *ri, int32_t n_i, int32_t ld, int32_t kdim,
                         const float *scale /* device scalar multiplying every score, or NULL */,
                         float *out, int32_t out_ld /* floats between rows of out (>= n_i; a multiple of 32 keeps every 128-byte
                                                       line inside one 64 x 64 tile, i.e. one workgroup / one XCD) */, void *stream);

/* ---- ranking (cdae.py:90-103, recommender_abc.py:454-461) --------------------------------
 * For each of R rows of `scores` [R, n] select the top `k` entries among those with
 * cand_mask == NULL || bit (r*n + i) set; order = descending score, ties by larger index
 * (heapq.nlargest over (score, iid) tuples).  out_idx/out_val [R,k]; missing = -1 / -inf. */
size_t drx_topk_scratch_bytes_k(int32_t R, int32_t n, int32_t k);   /* 0 for n <= 16384 (LDS bitonic path, scratch may be NULL); longer rows:
                                                                       * the k keys a radix select picks per row (+ sort space when k > 16384) */
size_t drx_topk_scratch_bytes(int32_t R, int32_t n);                 /* the same for k = n (an upper bound for every k) */
int drx_topk(const float *scores, const uint32_t *cand_mask, int32_t R, int32_t n, int32_t k,
             int32_t *out_idx, float *out_val, void *scratch, size_t scratch_bytes, void *stream);

/* ---- batched top-n recommendation for CDAE (no reference equivalent: recommender_abc.py:445-461 ranks one user per call) ---------------
 * For each of R users: the n best items of the whole catalogue by score[r, i] = sigmoid(h[r, :] . W2T[i, :] + b2[i]) among those not in
 * the user's row of the exclusion CSR — order as drx_topk (descending score, ties by larger index), out_idx / out_val [R, n], missing
 * = -1 / -inf.  The [R, n_items] score matrix is never written: the products run on the matrix cores in fp32 (a k-ordered fmaf chain,
 * then the bias; drx_cdae_forward sums the same products in another order, so a score may differ from its prediction in the last ulp),
 * the selection in registers, and the scratch holds candidate keys only: R (rounded up to 128) x item splits x 2 lists of max(2 n, 32)
 * keys, whatever n_items.  The result is a function of the inputs alone: bit-identical between calls, request orders and chunkings.
 *   h            [R, ld] hidden rows as drx_cdae_forward writes them (bt->uid = uid, pred = NULL)
 *   uid          [R] the users (names the rows of the exclusion CSR; may be NULL without one)
 *   excl_indptr  [n_users + 1], excl_indices: items never returned for a user, columns ascending and unique; both NULL = none
 * Fused domain: ld <= 256, n <= 128; outside it DRX_ENOTIMPL (drx_cdae_recommend_scratch_bytes: 0) and the caller takes
 * drx_cdae_forward + drx_topk. */
size_t drx_cdae_recommend_scratch_bytes(int32_t R, int32_t n_items, int32_t ld, int32_t n);
int drx_cdae_recommend(const DrxCdaeParams *p, const float *h, const int32_t *uid, int32_t R, int32_t n, const int64_t *excl_indptr,
                       const int32_t *excl_indices, int32_t *out_idx, float *out_val, void *scratch, size_t scratch_bytes, void *stream);

/* ---- the same scorer-selector for any rows x table problem: score[r, i] = epilogue(q[r, :] . table[i, :] (+ bias[i])) ------------------
 * drx_cdae_recommend is this call with table = W2T, bias = b2, DRX_REC_SIGMOID_BIAS; Caser.recommend_batch gives it the rows of
 * drx_caser_hidden (cat_out) against dense_1 (W1, b1) with DRX_REC_BIAS — logits, as Caser's _rank returns them —, DMF.recommend_batch
 * the l2-normalised tower outputs of drx_dmf_predict (rep_u_out of the requested users against rep_i_out of every item) with
 * DRX_REC_CLIP.  Same contract as drx_cdae_recommend: order as drx_topk, -1 / -inf behind the last eligible item, scratch of candidate
 * keys only, a result that is a function of the inputs alone; fused domain ld <= 256, ld % 4 == 0, n <= 128, outside it DRX_ENOTIMPL
 * (scratch bytes 0).  DRX_EINVAL: an unknown epilogue, a bias with DRX_REC_CLIP, no bias with the other two.
 *   table  [n_items, ld], q [R, ld]: columns between the model's width and ld must be ZERO (they are multiplied, not skipped)
 *   bias   [n_items] or NULL (DRX_REC_CLIP)
 * A score is a k-ordered fmaf chain (then the bias): it may differ in the last ulp from what the model's per-pair / per-row predict
 * computes, so exact near-ties may come out in another order than a per-user rank gives. */
#define DRX_REC_SIGMOID_BIAS 0   /* sigmoid(q . T[i] + bias[i])        (CDAE)  */
#define DRX_REC_BIAS         1   /* q . T[i] + bias[i]                 (Caser) */
#define DRX_REC_CLIP         2   /* max(1e-6, q . T[i]), bias == NULL  (DMF)   */
size_t drx_rows_recommend_scratch_bytes(int32_t R, int32_t n_items, int32_t ld, int32_t n);
int drx_rows_recommend(const float *table, const float *bias, int32_t n_items, int32_t ld, int32_t epilogue,
                       const float *q, const int32_t *uid, int32_t R, int32_t n,
                       const int64_t *excl_indptr, const int32_t *excl_indices,
                       int32_t *out_idx, float *out_val, void *scratch, size_t scratch_bytes, void *stream);

/* ---- catalogue ranks of given (row, item) pairs: where in the WHOLE catalogue an item stands for a query row -------------------------
 * For each of R rows (query row q[r, :], user uid[r], target item target[r]):
 *   out_rank[r]  = #{ i != target[r], i not in the exclusion row of uid[r], key(r, i) > key(r, target[r]) }
 *   out_score[r] = the target's score
 * with key = drx_rows_recommend's (monotone score bits << 32 | item; the score is the same k-ordered fmaf chain, then the bias, then the
 * epilogue): out_rank[r] is the position of target[r] in the list drx_rows_recommend would return for the row if n were unbounded, bit
 * for bit, ties to the larger item index.  The target's own exclusion is ignored here (the caller decides what an excluded target
 * means).  A target outside [0, n_items) gives out_rank = -1, out_score = -inf.  One target per row: through THIS entry point a user with T
 * held-out items costs T rows and T catalogue walks (drx_rows_rank_lists below takes a row's items as one list).  No score matrix and no lists: the scratch holds two words per row and the rows' partial counts (R rounded up to 128 x item
 * splits x 2), whatever n_items.  Counts are summed in a fixed order without atomics: the result is a function of the inputs alone.
 * Arguments, padding columns (ZERO), epilogues and argument errors as drx_rows_recommend; fused domain ld <= 256, ld % 4 == 0, outside
 * it DRX_ENOTIMPL (scratch bytes 0). */
size_t drx_rows_rank_items_scratch_bytes(int32_t R, int32_t n_items, int32_t ld);
int drx_rows_rank_items(const float *table, const float *bias, int32_t n_items, int32_t ld, int32_t epilogue,
                        const float *q, const int32_t *uid, const int32_t *target, int32_t R,
                        const int64_t *excl_indptr, const int32_t *excl_indices,
                        int32_t *out_rank, float *out_score, void *scratch, size_t scratch_bytes, void *stream);

/* ---- the same for rows that own a LIST of targets: all of a user's held-out items in one scoring pass ---------------------------------
 * R query rows (q [R, ld], uid [R]); row r owns targets[target_indptr[r] .. target_indptr[r + 1]).  target_indptr is a DEVICE pointer to
 * R + 1 offsets, absolute into targets, out_rank and out_score: a chunk of rows is launched with target_indptr + lo and the same three
 * pointers.  P = target_indptr[R] - target_indptr[0] sizes the scratch (the call reads the two offsets back: one synchronisation of
 * the stream); P = 0 returns DRX_OK and writes nothing, slots outside [target_indptr[0], target_indptr[R]) are never written.
 * A row's targets ascend as signed ints, duplicates allowed; a row may be empty; an unsorted row is memory-safe, its results unspecified.
 * For every target p of row r, out_rank[p] / out_score[p] are bit for bit what drx_rows_rank_items returns for the single pair
 * (q[r], uid[r], targets[p]): -1 / -inf outside [0, n_items), the target's own exclusion ignored, the row's other targets counted like
 * any item.  Cost: the blocks that hold a target once per 32 rows, then ONE counting walk of the catalogue per
 * drx_rows_rank_lists_group(ld) targets of the longest row of a wave's 32 rows (G: what the workgroup's local memory holds beside
 * the tile's query rows: 32 up to ld = 64, 26 at 128, 4 at 256) — split longer rows into rows of at most G that share q and uid.
 * No atomics, sums in a fixed order: a function of the inputs alone.  The scratch holds two words and 2 x splits partial counts per
 * target, no score matrix, and does not depend on n_items once the catalogue has more 128-item blocks than the launch has splits.
 * Epilogues, padding columns (ZERO) and argument errors as drx_rows_rank_items; fused domain ld <= 256, ld % 4 == 0, outside it
 * DRX_ENOTIMPL (group and scratch bytes 0). */
int32_t drx_rows_rank_lists_group(int32_t ld);
size_t drx_rows_rank_lists_scratch_bytes(int32_t R, int64_t P, int32_t n_items, int32_t ld);
int drx_rows_rank_lists(const float *table, const float *bias, int32_t n_items, int32_t ld, int32_t epilogue,
                        const float *q, const int32_t *uid, int32_t R,
                        const int64_t *target_indptr, const int32_t *targets,
                        const int64_t *excl_indptr, const int32_t *excl_indices,
                        int32_t *out_rank, float *out_score, void *scratch, size_t scratch_bytes, void *stream);

/* ---- scores of given (query row, table row) pairs and nothing else: what predict_pairs / predictive_evaluation stand on ---------------
 *   out_score[p] = epilogue(q[q_row[p], :] . table[t_row[p], :] (+ bias[t_row[p]]))        for p in [0, P)
 * q_row and t_row index ROWS, not users or items: the caller passes one query row per DISTINCT user (q [n_q, ld]; no [P, ld] gather as
 * drx_rows_rank_items needs) and may pass a table of the distinct items' rows only (DMF: the item tower never runs over the catalogue).
 * t_row[p] outside [0, n_rows) or q_row[p] outside [0, n_q) gives -inf.  P == 0 returns DRX_OK and writes nothing; slots from P on are
 * never written.  No scratch and no atomics: two rows per pair are read, the result is a function of the inputs alone.
 * One serving arithmetic: for ld <= 256 a pair's score equals, as a float32 value, the out_score drx_rows_rank_items returns for the same
 * query row and item (and so what drx_rows_recommend lists): the sum starts from 0.0f and takes the columns in steps of 8, within a
 * step in the order 0, 4, 1, 5, 2, 6, 3, 7, one fmaf each; steps whose first column is >= ld are skipped; then the bias, then the
 * epilogue; a score of -0.0 is written as +0.0, as the keys of the other entry points carry it.  Above ld = 256 the same chain
 * continues (the 256-float limit of the matrix-core scorers does not exist here).
 * Domain: ld % 4 == 0, ld >= 4, any size, else DRX_EINVAL; n_rows, n_q >= 1.  Epilogues, padding columns (ZERO in q and table) and
 * argument errors as drx_rows_recommend: DRX_EINVAL for an unknown epilogue, a bias with DRX_REC_CLIP, no bias with the other two.
 * Pairs sorted by q_row read their query rows from the L1; any order gives the same values. */
int drx_rows_pair_scores(const float *table, const float *bias, int32_t n_rows, int32_t ld, int32_t epilogue,
                         const float *q, int32_t n_q, const int32_t *q_row, const int32_t *t_row, int64_t P,
                         float *out_score, void *stream);

/* ---- UserKNN / ItemKNN baselines (DRecPy/Recommender/Baseline: base_knn.py, similarity.py, aggregation.py) ---------------------------
 * X is the [R, C] rating matrix in the orientation being compared (UserKNN: users x items; ItemKNN: items x users), given as a CSR:
 * indptr int64 [R + 1], columns int32 ascending and unique per row, float values, nnz entries; an entry of value 0 or with a column
 * outside [0, C) counts as absent, offsets are clamped into [0, nnz].  With M = (X != 0), a row pair's sums over its common columns
 *   n = sum 1, Sxy = sum x y, Sx = sum x, Sy = sum y, Sxx = sum x^2, Syy = sum y^2          (x: the row with the SMALLER id)
 * are fp32 products on the matrix cores (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, exact for integer ratings below 2^24), and
 * per row cnt, mean, full2 = sum x^2 and c2 = sum (x - mean)^2 are sequential double sums in CSR order.  The similarity is computed in
 * double, single operations in this order (no contraction), and the pair is DROPPED where stated:
 *   DRX_KNN_COSINE           Sxy / (sqrt(full2_x) * sqrt(full2_y))
 *   DRX_KNN_ADJUSTED_COSINE  (((Sxy - mean_y * Sx) - mean_x * Sy) + (n * mean_x) * mean_y) / (sqrt(c2_x) * sqrt(c2_y));  denominator == 0
 *   DRX_KNN_COSINE_CF        Sxy / (sqrt(Sxx) * sqrt(Syy));                                                              Sxy == 0
 *   DRX_KNN_JACCARD          n / ((cnt_x + cnt_y) - n)
 *   DRX_KNN_MSD              1 - (((Sxx + Syy) - 2 * Sxy) / (max_diff * max_diff)) / n
 *   DRX_KNN_PEARSON          (Sxy - (Sx * Sy) / n) / (sqrt(vx) * sqrt(vy)), vx = Sxx - (Sx * Sx) / n, vy likewise;    vx <= 0 or vy <= 0
 * always when n == 0, and when m > 0 and n < m.  Then s = s * (n / ((n + shrinkage) + 1e-6)) unless shrinkage < 0 (none), and s is
 * rounded to float32 once.  The neighbours of row i are the k largest among the rows j != i with s > 0 in heapq.nlargest((s, j)) order
 * (descending s, ties to the larger id): out_idx / out_sim [R, k], -1 / 0 behind the last neighbour.  sim(i, j) == sim(j, i) bit for bit.
 * No [R, R] matrix is written; the scratch holds the dense X (R up to 128 x C up to 8 floats: the caller bounds it), the row statistics
 * and candidate keys.  No atomics, fixed summation order: the result is a function of the inputs alone, the same for every `splits`
 * (0: chosen to fill the chip; > 0: that many J ranges per row tile at most, for tests of the merge).
 * Domain: 1 <= k <= 128, m >= 0, C >= 1, max_diff > 0 for DRX_KNN_MSD, else DRX_EINVAL; R == 0 returns DRX_OK and writes nothing. */
#define DRX_KNN_COSINE          0
#define DRX_KNN_ADJUSTED_COSINE 1
#define DRX_KNN_COSINE_CF       2
#define DRX_KNN_JACCARD         3
#define DRX_KNN_MSD             4
#define DRX_KNN_PEARSON         5
#define DRX_KNN_USER            0   /* neighbour table over users  */
#define DRX_KNN_ITEM            1   /* neighbour table over items  */
#define DRX_KNN_MEAN            0   /* sum r / count               */
#define DRX_KNN_WEIGHTED_MEAN   1   /* sum s r / sum s             */
size_t drx_knn_neighbours_scratch_bytes(int32_t R, int32_t C, int32_t k, int32_t splits);
int drx_knn_neighbours(const int64_t *indptr, const int32_t *indices, const float *values, int64_t nnz, int32_t R, int32_t C,
                       int32_t metric, int32_t k, int32_t m, double shrinkage, double max_diff, int32_t splits,
                       int32_t *out_idx, float *out_sim, void *scratch, size_t scratch_bytes, void *stream);

/* out_mean[r] = the mean of ALL entries of CSR row r (a sequential double sum in CSR order / the count), 0 for an empty row: the
 * fallback of use_averages (the user's mean for ItemKNN, the item's for UserKNN on the transposed CSR). */
int drx_knn_row_means(const int64_t *indptr, const float *values, int64_t nnz, int32_t R, double *out_mean, void *stream);

/* Predictions from a neighbour table (nb_idx / nb_sim [n_users or n_items, k] as drx_knn_neighbours writes them) and the USER-major CSR
 * of the ratings (indptr [n_users + 1], columns ascending), whatever the type.  The terms are taken in neighbour-list order among the
 * entries whose interaction exists — DRX_KNN_ITEM: the neighbours of the item that the user rated; DRX_KNN_USER: the neighbours of
 * the user that rated the item — and summed in double, single operations: weighted mean num += s * r, den += s; mean num += r,
 * den += 1; the prediction is num / den in the raw rating scale, and there is NONE where there is no term (and no fallback).
 * drx_knn_score_rows: for the R users uid[r] every item's prediction, rounded to float32 once, out [R, n_items] (0 where none);
 *   cand_mask (optional, drx_topk's layout: bit r * n_items + i) is in/out: the bit is cleared where the model has no prediction.
 *   fallback (optional, DRX_KNN_ITEM only, [n_users], read at uid[r]): the row's prediction where it has no term (use_averages: the
 *   users' means, the array drx_knn_pair_scores takes).
 *   One workgroup per user; its row lives in LDS, or in the scratch (drx_knn_score_rows_scratch_bytes, 0 while it fits) when
 *   n_items floats (ITEM) / 2 n_items doubles (USER) exceed 160 KiB.  R * n_items < 2^31 (drx_topk reads the matrix).
 * drx_knn_pair_scores: the same for P given pairs, out double [P] (0 where none) and none uint8 [P]; the interaction lookup is a
 *   binary search in the CSR row; fallback (optional) is indexed by the USER for DRX_KNN_ITEM (user means) and by the ITEM for
 *   DRX_KNN_USER (item means).  A user or item outside the model: none.
 * Argument errors DRX_EINVAL; R == 0 / P == 0 return DRX_OK and write nothing. */
size_t drx_knn_score_rows_scratch_bytes(int32_t type, int32_t R, int32_t n_items);
int drx_knn_score_rows(int32_t type, int32_t aggregation, const int64_t *indptr, const int32_t *indices, const float *values, int64_t nnz,
                       int32_t n_users, int32_t n_items, const int32_t *nb_idx, const float *nb_sim, int32_t k,
                       const int32_t *uid, int32_t R, const double *fallback, float *out, uint32_t *cand_mask,
                       void *scratch, size_t scratch_bytes, void *stream);
int drx_knn_pair_scores(int32_t type, int32_t aggregation, const int64_t *indptr, const int32_t *indices, const float *values, int64_t nnz,
                        int32_t n_users, int32_t n_items, const int32_t *nb_idx, const float *nb_sim, int32_t k,
                        const int32_t *uid, const int32_t *iid, int64_t P, const double *fallback, double *out, uint8_t *none,
                        void *stream);

/* Top-n and catalogue ranks from the same predictions WITHOUT the [R, n_items] matrix of drx_knn_score_rows and without a candidate
 * mask: the model arguments, uid [R] and fallback (DRX_KNN_ITEM only, else DRX_EINVAL) as drx_knn_score_rows takes them, the optional
 * exclusion CSR over users (excl_indptr [n_users + 1] / excl_indices, columns ascending and unique; both NULL = none) as
 * drx_rows_recommend takes it.  The prediction of (r, i) is drx_knn_score_rows' value bit for bit (the same device code: the same terms
 * in the same order, double, one rounding to float32).  An item is ELIGIBLE for row r when it has a prediction (a term, or the
 * fallback) and is not in the exclusion row of uid[r]; a uid[r] outside [0, n_users) has no eligible item.  Order is drx_topk's:
 * descending prediction, ties to the larger item index (key = ordered float bits << 32 | item, -0.0 carried as +0.0).
 * drx_knn_recommend: out_idx / out_val [R, n] = the n best eligible items of each row, -1 / -inf behind the last one.  Domain
 *   1 <= n <= 128; a larger n returns DRX_ENOTIMPL (scratch bytes 0) and the caller keeps drx_knn_score_rows + drx_topk.
 * drx_knn_rank_lists: row r owns targets[target_indptr[r] .. target_indptr[r + 1]) (target_indptr a DEVICE pointer to R + 1 offsets,
 *   clamped into [0, P]; P is given, nothing is read back), in any order, duplicates allowed, possibly empty.  For a target t of row r
 *     out_rank  = #{ i != t, i eligible for r, (prediction_i, i) > (prediction_t, t) }      out_score = t's prediction
 *   — the position t has in drx_knn_recommend's list for that row with n unbounded.  The target's own exclusion is ignored (the
 *   caller decides what an excluded target means).  A target outside [0, n_items), a target without a prediction and a uid outside
 *   the model give -1 / -inf.  P == 0 or R == 0 returns DRX_OK and writes nothing; slots from P on are never written.
 * One workgroup per row.  Its working row — DRX_KNN_ITEM: the user's ratings and the prediction keys, 8 bytes an item; DRX_KNN_USER:
 * the [n_items][2] double sums, overwritten in place by the keys, 16 bytes an item — lives in LDS while it fits 160 KiB less 64 bytes
 * (n_items <= 20472 / 10236; scratch bytes 0), beyond that in the scratch (R rows of that size, the only thing of size [R, n_items]
 * ever written).  The exclusion row is applied in the workgroup; the selection takes n rounds of "the largest key below the last
 * one", the ranks one counting walk of the row per 4 targets.  No atomics, every order fixed: the result is a function of the
 * inputs alone, the same for every request order and chunking.  Argument errors DRX_EINVAL (also NULL outputs with work to do, one
 * half of the exclusion CSR without the other), a short scratch DRX_ESCRATCH. */
size_t drx_knn_recommend_scratch_bytes(int32_t type, int32_t R, int32_t n_items, int32_t n);
int drx_knn_recommend(int32_t type, int32_t aggregation, const int64_t *indptr, const int32_t *indices, const float *values, int64_t nnz,
                      int32_t n_users, int32_t n_items, const int32_t *nb_idx, const float *nb_sim, int32_t k,
                      const int32_t *uid, int32_t R, int32_t n, const double *fallback,
                      const int64_t *excl_indptr, const int32_t *excl_indices,
                      int32_t *out_idx, float *out_val, void *scratch, size_t scratch_bytes, void *stream);
size_t drx_knn_rank_lists_scratch_bytes(int32_t type, int32_t R, int64_t P, int32_t n_items);
int drx_knn_rank_lists(int32_t type, int32_t aggregation, const int64_t *indptr, const int32_t *indices, const float *values, int64_t nnz,
                       int32_t n_users, int32_t n_items, const int32_t *nb_idx, const float *nb_sim, int32_t k,
                       const int32_t *uid, int32_t R, const int64_t *target_indptr, const int32_t *targets, int64_t P,
                       const double *fallback, const int64_t *excl_indptr, const int32_t *excl_indices,
                       int32_t *out_rank, float *out_score, void *scratch, size_t scratch_bytes, void *stream);

/* ---- stable device radix sort of (key, val) pairs (the inverted-index builder of the sparse steps; ties keep their input order).
 * Every key must be < 2^key_bits: the sort runs ceil(key_bits / digit) passes of 8-, 10- or 11-bit digits, i.e. it orders on
 * passes * digit >= key_bits bits — bits above key_bits are NOT ignored (DRX_EINVAL is not raised for them: the result is then ordered
 * on those bits too).  keys_out / vals_out must not alias the inputs.  temp: >= drx_sort_pairs_temp_bytes(n, key_bits). */
size_t drx_sort_pairs_temp_bytes(int64_t n, int32_t key_bits);
int drx_sort_pairs(const uint32_t *keys_in, uint32_t *keys_out, const uint32_t *vals_in, uint32_t *vals_out, int64_t n, int32_t key_bits,
                   void *temp, size_t temp_bytes, void *stream);
/* DEBUGGING ENTRY (tests): the sort as a preparation calls it — pairs whose key is DRX_KEY_NONE take no part: keys_out = the other
 * pairs sorted, then DRX_KEY_NONE up to n; vals_out is written for the sorted pairs only (the words behind them keep what they held).
 * Every other key must be < 2^key_bits (key_bits = 32: <= 0xFFFFFFFE).  pre_zeroed != 0: the sort is told that its caller has cleared
 * the counters and tile words of `temp` (the library's preparations do that in a kernel of their own); this entry clears exactly
 * that range first, with one memset, and nothing else of `temp`.  Arguments and return codes as drx_sort_pairs. */
int drx_debug_sort_pairs_drop(const uint32_t *keys_in, uint32_t *keys_out, const uint32_t *vals_in, uint32_t *vals_out, int64_t n,
                              int32_t key_bits, int32_t pre_zeroed, void *temp, size_t temp_bytes, void *stream);

/* ---- raw -> internal id map (mem_dataset.py:309-330) --------------------------------------
 * codes[r] = rank of first appearance of raw[r] (int64 raw ids), bit-exact.
 * n_unique (device int32) receives the number of categories; uniques[c] the raw id of code c.
 * scratch: >= drx_idmap_scratch_bytes(n). */
size_t drx_idmap_scratch_bytes(int64_t n);
int drx_idmap_build(const int64_t *raw, int64_t n, int32_t *codes, int64_t *uniques,
                    int32_t *n_unique, void *scratch, size_t scratch_bytes, void *stream);

/* ---- host-side sampler (point_sampler.py:44-61; mem_dataset.py:111-163) ---------------------
 * CPython-exact MT19937 streams (random.Random(seed): init_by_array, 53-bit random(),
 * getrandbits-rejection randint).  All pointers here are HOST memory. */
typedef struct DrxSampler DrxSampler;
DrxSampler *drx_sampler_create(const int32_t *h_uid, const int32_t *h_iid, const double *h_val, int64_t n_rows,
                               int32_t neg_ratio, int32_t has_threshold, double threshold, int64_t seed);
int drx_sampler_sample(DrxSampler *s, int32_t n, int32_t *h_uid_out, int32_t *h_iid_out, double *h_val_out);
/* kind: DRX_DRAW_MIXED = PointSampler.sample, DRX_DRAW_NEGATIVE = sample_negative, DRX_DRAW_POSITIVE = sample_positive
 * (point_sampler.py:74-96); each advances only the stream(s) the reference method advances.
 * h_neg_out (optional): 1 where the draw is a negative (a pair absent from the frame, value 0). */
enum { DRX_DRAW_MIXED = 0, DRX_DRAW_NEGATIVE = 1, DRX_DRAW_POSITIVE = 2 };
int drx_sampler_draw(DrxSampler *s, int32_t kind, int32_t n, int32_t *h_uid_out, int32_t *h_iid_out, double *h_val_out,
                     uint8_t *h_neg_out);
void drx_sampler_destroy(DrxSampler *s);

/* ---- host-side ListSampler (list_sampler.py:76-151) ---------------------------------------------------------------------
 * The draw loop of ListSampler.sample_group_records with the stream of random.Random(seed): choice of a group, window start,
 * inputs / targets, rng.sample over the eligible negative ids in CPython's set iteration order (the ids are dense ints in
 * [0, n_ids), all present in the dataset).  Groups come in unique_groups order; group g owns the dataset rows
 * grp_rows[grp_indptr[g] .. grp_indptr[g+1]) — already filtered by interaction_threshold and ordered by sort_column — whose
 * negative_ids_col values are grp_ids[...].  n_targets < 0 / max_positive < 0 mean None.  All pointers are HOST memory. */
typedef struct DrxListSampler DrxListSampler;
DrxListSampler *drx_list_sampler_create(const int64_t *grp_indptr, const int64_t *grp_rows, const int32_t *grp_ids, int32_t n_groups,
                                        int32_t n_ids, int32_t neg_ratio, int32_t n_targets, int32_t min_positive,
                                        int32_t max_positive, int64_t seed);
/* n draws: group_out[n]; in_off / tg_off / ng_off [n+1] prefix offsets into in_rows / tg_rows (dataset rows of the inputs /
 * targets) and neg_ids.  DRX_ESCRATCH: a capacity is too small; DRX_ERETRY: more than 20 consecutive failed attempts
 * (drx_list_sampler_last_hint: 1 = too few positive records, 2 = too few eligible negatives). */
int drx_list_sampler_sample(DrxListSampler *s, int32_t n, int32_t *group_out, int64_t *in_off, int64_t *in_rows, int64_t in_cap,
                            int64_t *tg_off, int64_t *tg_rows, int64_t tg_cap, int64_t *ng_off, int32_t *neg_ids, int64_t ng_cap);
int32_t drx_list_sampler_last_hint(const DrxListSampler *s);
void drx_list_sampler_destroy(DrxListSampler *s);

/* CDAE corruption stream (cdae.py:63, RecommenderABC._rng of recommender_abc.py:74): draws
 * n_items uniforms per row, in batch order, and writes keep flags for the positives of each row. */
typedef struct DrxRng DrxRng;
DrxRng *drx_rng_create(int64_t seed);
void drx_rng_destroy(DrxRng *r);
double drx_rng_random(DrxRng *r);
int64_t drx_rng_randint(DrxRng *r, int64_t a, int64_t b);
/* advances the stream by n_words 32-bit outputs without producing them (a uniform(0,1) draw consumes two) */
void drx_rng_discard(DrxRng *r, uint64_t n_words);
int drx_rng_corruption_keep(DrxRng *r, const int64_t *h_indptr, const int32_t *h_indices, int32_t n_items,
                            const int32_t *h_uid, int32_t B, double q,
                            int32_t *h_keep_off, uint8_t *h_keep, int64_t keep_capacity);

/* One reference-mode CDAE batch in one call, for worker threads drawing ahead of the training step (cdae.py:47-63: B sampler
 * triples, then N uniform draws per batch row): waits until *turn == ticket, draws (DRX_DRAW_MIXED), stores ticket + 1 into
 * *turn, advances `rng` by discard_words outputs (batches drawn by other workers from their own generator of the same seed)
 * and fills keep_off / keep like drx_rng_corruption_keep. */
int drx_cdae_reference_draw(DrxSampler *smp, DrxRng *rng, int64_t *turn, int64_t ticket, uint64_t discard_words,
                            const int64_t *h_indptr, const int32_t *h_indices, int32_t n_items, int32_t B, double q,
                            int32_t *h_uid_out, int32_t *h_iid_out, double *h_val_out, uint8_t *h_neg_out, int32_t *h_keep_off,
                            uint8_t *h_keep, int64_t keep_capacity);

/* Draw-ahead workers for the loop above: two native threads (one per corruption generator `gen`), each running the jobs submitted
 * to it in order through drx_cdae_reference_draw with a turn counter of their own (tickets 0, 1, 2, ... in submission order
 * across both).  They and drx_drawahead_wait poll for a few hundred microseconds before sleeping, so a fit() that needs a batch
 * every 40-70 us never pays a thread wake-up.  The buffers of a job belong to the caller and must stay valid until its wait
 * returns; at most 8 jobs per generator may be outstanding (DRX_ERETRY otherwise).  submit returns the job's index (>= 0). */
typedef struct DrxDrawAhead DrxDrawAhead;
DrxDrawAhead *drx_drawahead_create(DrxSampler *smp, DrxRng *rng0, DrxRng *rng1, const int64_t *h_indptr, const int32_t *h_indices,
                                   int32_t n_items);
int64_t drx_drawahead_submit(DrxDrawAhead *d, int32_t gen, int64_t ticket, uint64_t discard_words, int32_t B, double q,
                             int32_t *h_uid_out, int32_t *h_iid_out, double *h_val_out, uint8_t *h_neg_out, int32_t *h_keep_off,
                             uint8_t *h_keep, int64_t keep_capacity);
int drx_drawahead_wait(DrxDrawAhead *d, int32_t gen, int64_t job);
void drx_drawahead_destroy(DrxDrawAhead *d);

/* ---- the quiet fit() loop of reference-mode CDAE in one call ------------------------------------------------------------------
 * n_steps iterations of recommender_abc.py:189-205 for the case in which nothing observes single steps (verbose off, no early-
 * stopping rule: no per-step loss, callback or log line): per step, wait for the drawn batch (draw-ahead workers above), queue
 * drx_cdae_step_dense on `stream`, submit the draws of later steps — at most 4 in flight and never beyond the last step, so the
 * sampler and corruption streams end exactly where the reference's do.  The Python loop does the same through _sample_batch /
 * _do_batch at ~40 us of interpreter time per step, which exceeds the device time of the ml-100k-shaped step.
 *   cursor[4] (in/out)  next sampler ticket, word of the corruption stream where the next batch begins, words consumed by
 *                       generator 0 and 1 of `draws` (what the Python loop keeps in _draw_ticket / _mask_pos / _mask_at)
 *   h_alphas            n_steps x 5 Keras-Adam lr_t, host memory (opt->alpha is ignored)
 *   h_slots             n_slots (8..64) staging slots of slot_bytes >= drx_cdae_fit_slot_bytes(B, keep_capacity) each, pinned host
 *                       memory addressable from the device (the step's kernels read the batch in place); keep_capacity >= the
 *                       largest possible sum of the B history lengths
 *   d_stage             device memory, d_stage_bytes >= 2 * slot_bytes, or NULL: the step of batch s copies what step s+1 reads of
 *                       its slot there from the last workgroup of its parameter sweep, so that only the first batch of a call is
 *                       read over PCIe by the gather kernel itself (NULL: every batch is)
 *   scratch             dense-step scratch (drx_cdae_scratch_bytes(p, B, 0, 1)) whose batch-membership arrays are zero
 *                       (DRX_DENSE_AUX_CLEAN is implied)
 * Returns after the queued steps have completed (the slots are the caller's again).  On error the draws in flight are waited for
 * and the cursor says what was consumed. */
size_t drx_cdae_fit_slot_bytes(int32_t B, int64_t keep_capacity);
int drx_cdae_fit_dense(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist, DrxDrawAhead *draws, int64_t *cursor,
                       int32_t B, float q, int64_t keep_capacity, int32_t loss_kind, int32_t targets_kind, int64_t n_steps,
                       const float *h_alphas, void *h_slots, size_t slot_bytes, int32_t n_slots, void *d_stage,
                       size_t d_stage_bytes, void *scratch, size_t scratch_bytes, void *stream);

/* ---- BPR-MF (Rendle et al. 2009; csrc/drx_bpr.hip) ----------------------------------------------------
 * Score x(u, i) = P[u] . Q[i] + bq[i]  (DRX_REC_BIAS of the fused scorer).  P [n_users, ld], Q [n_items, ld], bq [n_items]; ld = K
 * rounded up to a multiple of 4, 4 <= ld <= 256, the padding columns zero — every call below keeps them zero.
 *
 * THE TRIPLE STREAM (counter-based, no retry loop; every index is (h * n) >> 32 in 64-bit integers, h = drx_hash_u32(seed, a, b)).
 * With r = neg_ratio >= 1, triple t of a batch belongs to pair p = t / r:
 *     u = eligible[(h(p, 0) * n_eligible) >> 32]
 *     i = the positive of u at position (h(p, 1) * deg_u) >> 32 of u's row of `hist`
 *     j = the item at rank (h(t, 2) * (n_items - nrec_u)) >> 32 of the ascending complement of u's row of `recorded`
 * hist: CSR of the positives (columns ascending); recorded: CSR of every pair the frame holds (NULL = hist), as in
 * drx_point_sample_recorded.  eligible: the users with at least one positive and fewer than n_items recorded items (built by the caller,
 * device int32 [n_eligible]); a listed user who is not eligible gets -1 for the id that cannot be drawn.  One thread per triple.
 * DRX_EINVAL, and nothing launched: a NULL pointer (hist or its arrays, the arrays of a given `recorded`, eligible, uid, pos, neg),
 * n_eligible < 1, n_items < 1, T < 1, neg_ratio < 1. */
int drx_bpr_sample(const DrxHistory *hist, const DrxHistory *recorded, const int32_t *eligible, int32_t n_eligible, int32_t n_items,
                   int32_t T, int32_t neg_ratio, uint64_t seed, int32_t *uid, int32_t *pos, int32_t *neg, void *stream);
/* out[r, :] = table[ids[r], :] for n device ids in [0, table rows) (not checked on the device): the query rows of the fused scorer */
int drx_bpr_gather_rows(const float *table, int32_t ld, const int32_t *ids, int32_t n, float *out, void *stream);
/* ONE TRAINING STEP on T triples (uid, pos, neg: device int32 [T], ids in range — not checked on the device):
 *     D_t = x(u, i) - x(u, j);   loss = (1 / T) sum_t softplus(-D_t);   g_t = -sigmoid(-D_t) / T
 *     dP[u] += g_t (Q[i] - Q[j]);  dQ[i] += g_t P[u];  dQ[j] -= g_t P[u];  dbq[i] += g_t;  dbq[j] -= g_t
 * then EVERY row of P and Q gets reg * row added to its gradient (bq none) and every row and bias is updated by `rule`, a dense rule
 * (DrxOptRule): the step sweeps both tables like the other dense steps.  alphas: HOST float [3], the step sizes of P, Q and bq (Adam:
 * the variable's lr_t; the other rules: the learning rate); rule->lr is ignored.  Slots (P_s1 .. bq_s2): those the rule has, shaped
 * like their parameter; one it lacks may be NULL and is not touched.
 * k_bpr_fwd_bwd reads the three rows of a triple once (a group of pick_geom(ld) lanes per triple, one float4 per lane) and writes, per
 * triple, the gradient row of P[u], a copy of P[u] and the scalars (g_t, -g_t); drx_batch_csr_device groups the T user keys and the
 * 2 T item keys (i_t, j_t interleaved); ONE drx_rows_csr_opt_multi call updates P (plain form) and Q with bq (outer-product form,
 * group 2: lookup o has the gradient row scale[o] * copy[o / 2] and the bias gradient scale[o]).  No atomics: every sum runs in an
 * order fixed by the batch, so equal inputs give equal bits.  The rows are read before the update launch writes them (stream order).
 * loss_out: device double [1] or NULL (then no loss is summed); the workgroups' partial sums (double) are added in a fixed order.
 * scratch: drx_bpr_step_scratch_bytes (0 = an invalid description).
 * DRX_EINVAL, and nothing launched: a NULL pointer among P, Q, bq, uid, pos, neg, rule, alphas, scratch; T < 1; n_users or n_items
 * < 1; ld outside 4..256 or no multiple of 4; no dense rule; a slot the rule has is NULL; a table or slot not 16-byte aligned.
 * DRX_ESCRATCH: scratch too small. */
size_t drx_bpr_step_scratch_bytes(int32_t T, int32_t ld, int32_t n_users, int32_t n_items);
int drx_bpr_step(float *P, float *Q, float *bq, float *P_s1, float *P_s2, float *Q_s1, float *Q_s2, float *bq_s1, float *bq_s2, int32_t ld,
                 int32_t n_users, int32_t n_items, const int32_t *uid, const int32_t *pos, const int32_t *neg, int32_t T,
                 const DrxOptRule *rule, const float *alphas, float reg, double *loss_out, void *scratch, size_t scratch_bytes,
                 void *stream);

/* ---- ALS / WMF (Hu, Koren, Volinsky 2008; csrc/drx_als.hip) ----------------------------------------------
 * Score x(u, i) = X[u] . Y[i]  (DRX_REC_BIAS of the fused scorer with a zero bias).  X [n_users, ld], Y [n_items, ld]; ld = K rounded
 * up to a multiple of 4, 4 <= ld <= 128, the padding columns zero — every call below keeps them zero.  A positive (u, i) has
 * preference 1 and confidence 1 + w, w >= 0 given per entry of a CSR of the positives (indptr int64, indices int32, weights float;
 * user-major for the user half, item-major for the item half).  Objective over ALL n_users x n_items cells:
 *     L = sum_ui c_ui (p_ui - x_u . y_i)^2 + lambda (|X|^2 + |Y|^2)
 * Nothing below uses an atomic on a float: every sum runs in an order fixed by its inputs, so equal inputs give equal bits.
 * Every scratch companion returns 0 for a description outside the domain.
 *
 * G = T^T T, out_G [ld, ld] row-major, symmetric bit for bit.  Workgroups take strips of at least 64 rows and accumulate the 16 x 16
 * tiles of the lower triangle with v_mfma_f32_16x16x4_f32 (an element is a row-ordered fmaf chain per strip); a second launch adds
 * the strips' tiles in ascending order and mirrors the triangle.
 * DRX_EINVAL, and nothing launched: a NULL pointer (table, out_G, scratch); n_rows < 1; ld outside 4..128 or no multiple of 4; table or
 * out_G not 16-byte aligned.  DRX_ESCRATCH: scratch smaller than drx_als_gram_scratch_bytes. */
size_t drx_als_gram_scratch_bytes(int32_t n_rows, int32_t ld);
int drx_als_gram(const float *table, int32_t n_rows, int32_t ld, float *out_G, void *scratch, size_t scratch_bytes, void *stream);
/* ONE HALF-SWEEP: for every row r of the CSR, with S_r its entries,
 *     A_r = G + sum_{j in S_r} w_j y_j y_j^T + lambda I,   b_r = sum_{j in S_r} (1 + w_j) y_j,   out[r] = A_r^-1 b_r
 * y_j = other[indices[j]], G = other^T other (drx_als_gram).  A row without entries is written as zeros.  One workgroup per row;
 * order: device int32 [n_rows] or NULL — workgroup g takes row order[g] (the caller's longest-first order), NULL = g; a value outside
 * [0, n_rows) is skipped.  An index outside [0, n_other) counts as a zero row.  The entries are taken in rounds of 32 in CSR order
 * (fp32 MFMA for A, k = the entries of a round; fmaf chains for b), the lower triangle of [A; b^T] is factorised in LDS by a
 * right-looking column Cholesky over the ld columns, then L^T x = L^-1 b, then ONE step of iterative refinement: the residual
 * r = sum_j [(1 + w_j) - w_j (y_j . x)] y_j - G x - lambda x is summed in double from the definition (the entries read once more), L L^T d = r
 * is solved in fp32 and x += d — what is left of the error is the rounding of G and of x, not cond(A) x eps of the fp32 A.  With lambda = 0 a zero column of `other` (its padding
 * included) is a zero pivot.
 * fail_count: device int32 [1], incremented once per row whose factorisation met a pivot <= 0 or a non-finite one; that row is written
 * as zeros; the call still returns DRX_OK.  scratch: drx_als_solve_rows_scratch_bytes (this form carves nothing from it).
 * DRX_EINVAL, and nothing launched: a NULL pointer (all but order); n_rows or n_other < 1; ld outside 4..128 or no multiple of 4;
 * lambda < 0 or non-finite; out, other or G not 16-byte aligned.  DRX_ESCRATCH: scratch too small. */
size_t drx_als_solve_rows_scratch_bytes(int32_t n_rows, int32_t n_other, int32_t ld);
int drx_als_solve_rows(float *out, const float *other, const float *G, const int64_t *indptr, const int32_t *indices, const float *weights,
                       const int32_t *order, int32_t n_rows, int32_t n_other, int32_t ld, float lambda, int32_t *fail_count, void *scratch,
                       size_t scratch_bytes, void *stream);
/* out_loss[0] (device double) = <Gx, Gy>_F + sum over the entries of [(1 + w) (1 - s)^2 - s^2] + lambda (tr Gx + tr Gy), s = X[u] . Y[i]
 * in fp32, every sum in double; Gx = X^T X and Gy = Y^T Y as drx_als_gram gives them.  indptr / indices / weights: the user-major CSR.
 * Workgroups take users b, b + grid, ...; their partial sums are added in ascending order.
 * DRX_EINVAL, and nothing launched: a NULL pointer; n_users or n_items < 1; ld outside 4..128 or no multiple of 4; lambda < 0 or
 * non-finite; X, Y, Gx or Gy not 16-byte aligned.  DRX_ESCRATCH: scratch smaller than drx_als_loss_scratch_bytes. */
size_t drx_als_loss_scratch_bytes(int32_t n_users, int32_t ld);
int drx_als_loss(const float *X, const float *Y, const float *Gx, const float *Gy, const int64_t *indptr, const int32_t *indices,
                 const float *weights, int32_t n_users, int32_t n_items, int32_t ld, float lambda, double *out_loss, void *scratch,
                 size_t scratch_bytes, void *stream);

/* ---- FPMC (Rendle, Freudenthaler, Schmidt-Thieme 2010; csrc/drx_fpmc.hip) ---------------------------------
 * Four factor tables and an item bias: P [n_users, ld] (user), Q (item as target of the user term), M (item as previous item),
 * N (item as target of the transition term), b [n_items].  ld = K rounded up to a multiple of 4, 4 <= ld <= 128.  The item side is
 * ONE table QN [n_items, 2 ld] = [Q[i] | N[i]], each half with its own zero padding; M is [n_items, ld].  A window w = (user u, the
 * ordered L items S before the target, target i, negatives j_1 .. j_r), 1 <= L <= 8, 1 <= r <= 16 (the forward kernel takes the
 * negatives' rows in at most two rounds of eight):
 *     c(u, S) = [P[u] | (1 / |S|) sum_{l in S} M[l]]          (2 ld floats; the sum positions ascending in fp32, then ONE multiply)
 *     x(u, S, i) = c . QN[i] + b[i]                           (DRX_REC_BIAS of the fused scorer at rows of 2 ld floats)
 *     D_wk = x(u, S, i) - x(u, S, j_k);  loss = (1 / (B r)) sum_w sum_k softplus(-D_wk);  g_wk = -sigmoid(-D_wk) / (B r)
 *     d_w = sum_k g_wk (QN[i] - QN[j_k]):  dP[u] += first half of d_w;  dM[l] += (1 / L) second half of d_w for every l in S
 *     dQN[i] += (sum_k g_wk) c;  dQN[j_k] -= g_wk c;  db[i] += sum_k g_wk;  db[j_k] -= g_wk
 * ONE TRAINING STEP on B windows in the layout drx_list_sample_device returns at n_targets = 1: uid [B], before [B, L],
 * after [B, 1 + r] (the target first), device int32, ids in range (not checked on the device).  Then EVERY row of P, M and QN gets
 * reg * row added to its gradient (b none) and every row and bias is updated by `rule`, a dense rule (DrxOptRule).  alphas: HOST
 * float [4], the step sizes of P, M, QN and b (Adam: the variable's lr_t; the other rules: the learning rate); rule->lr is ignored.
 * Slots (P_s1 .. b_s2): those the rule has, shaped like their parameter; one it lacks may be NULL and is not touched.
 * k_fpmc_fwd_bwd gives a window to a group of pick_geom(2 ld) lanes, one float4 of a 2 ld row per lane; it forms c once per window and
 * writes c, the first half of d_w, L copies of the second half times 1 / L and the 1 + r scales (sum_k g_wk, -g_w1 .. -g_wr);
 * drx_batch_csr_device groups the B user keys, the B L previous-item keys and the B (1 + r) item keys (uid, before, after as they
 * are); ONE drx_rows_csr_opt_multi call updates P and M (plain form) and QN with b (outer-product form, group 1 + r, the written c as
 * its rows).  No atomics: every sum runs in an order fixed by the batch, so equal inputs give equal bits.
 * loss_out: device double [1] or NULL (then no loss is summed); the workgroups' partial sums (double) are added in a fixed order.
 * scratch: drx_fpmc_step_scratch_bytes (0 = a description outside the domain).
 * DRX_EINVAL, and nothing launched: a NULL pointer among P, M, QN, b, uid, before, after, rule, alphas, scratch; B < 1; L outside
 * 1..8; neg_ratio outside 1..16; n_users or n_items < 1; ld outside 4..128 or no multiple of 4; no dense rule; a slot the rule has is
 * NULL; a table or slot not 16-byte aligned.  DRX_ESCRATCH: scratch too small. */
size_t drx_fpmc_step_scratch_bytes(int32_t B, int32_t L, int32_t neg_ratio, int32_t ld, int32_t n_users, int32_t n_items);
int drx_fpmc_step(float *P, float *M, float *QN, float *b, float *P_s1, float *P_s2, float *M_s1, float *M_s2, float *QN_s1, float *QN_s2,
                  float *b_s1, float *b_s2, int32_t ld, int32_t n_users, int32_t n_items, const int32_t *uid, const int32_t *before,
                  const int32_t *after, int32_t B, int32_t L, int32_t neg_ratio, const DrxOptRule *rule, const float *alphas, float reg,
                  double *loss_out, void *scratch, size_t scratch_bytes, void *stream);
/* out[q, :] = c(uid[q], the basket of uid[q]) for n device user ids (in range, not checked on the device): the query rows of the fused
 * scorer, out [n, 2 ld].  baskets: device int32 [n_users, L], -1 = an absent position; the mean runs over the entries present in
 * position order, an empty basket gives a zero second half.  The same summation function as the step: a full basket gives the bits
 * of the context row the step forms for that window.
 * DRX_EINVAL, and nothing launched: a NULL pointer; n < 1; L outside 1..8; ld outside 4..128 or no multiple of 4; P, M or out not
 * 16-byte aligned. */
int drx_fpmc_query_rows(const float *P, const float *M, int32_t ld, const int32_t *baskets, int32_t L, const int32_t *uid, int32_t n,
                        float *out, void *stream);

/* ---- NeuMF (He, Liao, Zhang, Nie, Hu, Chua 2017; csrc/drx_ncf.hip) ------------------------------------------
 * Tables U [n_users, ldg + ldm] = [Pg[u] | Pm[u]] and V [n_items, ldg + ldm] = [Qg[i] | Qm[i]]: the GMF half of kg floats and the MLP
 * half of km floats, each rounded up to a multiple of 4 with its own ZERO padding.  One flat array sw of small weights, in this order
 * (all row-major, DrxNcfDims has the offsets, which must be exactly these):
 *     W_1 [2 km, f_1], b_1 [f_1], W_l [f_{l-1}, f_l], b_l [f_l] (l = 2 .. n), h = [hg (kg) | hm (f_n)], b0
 *     a_0 = [Pm[u] ; Qm[i]],  a_l = relu(W_l^T a_{l-1} + b_l),  x(u, i) = sum_k hg[k] Pg[u, k] Qg[i, k] + hm . a_n + b0
 * (relu's derivative at 0 is 0: A > 0 <=> Z > 0).  Domain: 1 <= kg, km <= 64, 1 <= n <= 4 layers, 1 <= f_l <= 64.  Everything is fp32;
 * no float atomics; every sum runs in an order fixed by the arguments: equal inputs give equal bits.  All launches are plain. */
#define DRX_NCF_MAX_LAYERS 4
typedef struct DrxNcfDims {
  int32_t n_users, n_items;
  int32_t kg, km, ldg, ldm;
  int32_t n_layers, f[DRX_NCF_MAX_LAYERS];
  int32_t off_w[DRX_NCF_MAX_LAYERS], off_b[DRX_NCF_MAX_LAYERS], off_h, off_b0, n_small;
} DrxNcfDims;
/* ONE TRAINING STEP on B point samples (uid, iid: device int32 [B], ids in range — not checked on the device; y: device float [B]):
 *     loss = (1 / B) sum_b [max(x_b, 0) - y_b x_b + log1p(exp(-|x_b|))],   g_b = (sigmoid(x_b) - y_b) / B
 * then EVERY row of U and V, every entry of the W_l and of h gets reg * itself added to its gradient (the b_l and b0 none) and
 * everything is updated by `rule`, a dense rule (DrxOptRule).  alphas: HOST float [3], the step sizes of U, V and sw (Adam: the
 * variable's lr_t; the other rules: the learning rate); rule->lr is ignored.  Slots: those the rule has, shaped like their parameter;
 * one it lacks may be NULL and is not touched.
 * k_ncf_tile: workgroups of four waves, drx_ncf_grid of them = min(tiles, 256), walk tiles of 16 samples (tile t to workgroup
 * t % grid, ascending).  A tile
 * gathers its rows into LDS, runs every layer forward and backward as v_mfma_f32_16x16x4_f32 products out of LDS (M = the tile, the
 * waves split the 16-column tiles) and writes one gradient row per sample for U and V ([B, ldg + ldm]: the GMF half g hg (.) the other
 * side's row, the MLP half the two halves of W_1 dz_1); the workgroup adds its tiles' gradients of sw (dW_l = A_{l-1}^T dZ_l on the
 * matrix cores) into ITS row of [grid, n_small] and its loss into one double.  One launch adds those rows in workgroup order and
 * updates sw by segments (drx_opt_segments' arithmetic); drx_batch_csr_device groups the two key lists and ONE
 * drx_rows_csr_opt_multi call updates U and V (plain form, the written rows as src).
 * loss_out: device double [1] or NULL.  scratch: drx_ncf_step_scratch_bytes (0 = a description outside the domain).
 * DRX_EINVAL, and nothing launched: a NULL pointer among D, U, V, sw, uid, iid, y, rule, alphas, scratch; B < 1 (or >= 2^24); a width
 * outside the domain; ldg / ldm / offsets / n_small that are not the layout above; n_users or n_items < 1; no dense rule; a slot the
 * rule has is NULL; a table or table slot not 16-byte aligned.  DRX_ESCRATCH: scratch too small. */
int drx_ncf_grid(int32_t B);
size_t drx_ncf_step_scratch_bytes(const DrxNcfDims *D, int32_t B);
int drx_ncf_step(const DrxNcfDims *D, float *U, float *V, float *sw, float *U_s1, float *U_s2, float *V_s1, float *V_s2, float *sw_s1,
                 float *sw_s2, const int32_t *uid, const int32_t *iid, const float *y, int32_t B, const DrxOptRule *rule,
                 const float *alphas, float reg, double *loss_out, void *scratch, size_t scratch_bytes, void *stream);
/* What a pair's logit needs from ONE side, for n device ids (ids NULL: rows 0 .. n - 1 of the table), out [n, hw] with
 * hw = drx_ncf_half_width(D) = f_1 rounded up to 4, plus ldg; padding ZERO:
 *     side 0 (users, table = U):  [W_1[:km]^T Pm[u] + b_1 (f_1) | hg (.) Pg[u] (ldg)]
 *     side 1 (items, table = V):  [W_1[km:]^T Qm[i]       (f_1) | Qg[i]        (ldg)]
 * The product runs on MFMA tiles of 16 rows, k ascending in steps of 4 (the matrix core's own order inside a step).
 * DRX_EINVAL, and nothing launched: a NULL pointer among D, table, sw, out; n < 1; side not 0 / 1; dims outside the domain; table or
 * out not 16-byte aligned. */
int32_t drx_ncf_half_width(const DrxNcfDims *D);
int drx_ncf_half_rows(const DrxNcfDims *D, const float *table, const float *sw, const int32_t *ids, int32_t n, int32_t side, float *out,
                      void *stream);
/* out[r, i] = x(user of uhalf row r, item i) for R rows of user half rows against the half rows of ALL n_items items (ihalf
 * [D->n_items, hw]), out [R, n_items]: a workgroup takes a strip of 64 items and a block of users, keeps the strip's half rows and
 * the kernels of layers 2 .. n in LDS, forms relu(A_u + B_i) for tiles of 16 pairs (one wave each), runs the layers on
 * v_mfma_f32_16x16x4_f32, reduces with hm and adds the GMF dot and b0.
 * drx_ncf_pair_scores: out[p] = x(uhalf row urow[p], ihalf row irow[p]) for P pairs (urow, irow: device int32 [P], rows in range —
 * not checked on the device) through the SAME device function: the order of a pair's sums does not depend on the pair's place in
 * a tile, so a pair's logit has the same bits from either call.
 * DRX_EINVAL, and nothing launched: a NULL pointer; R / P < 1; R above 65535 blocks of 32 users (callers chunk the score matrix long
 * before); dims outside the domain; uhalf, ihalf not 16-byte aligned. */
int drx_ncf_score_rows(const DrxNcfDims *D, const float *sw, const float *uhalf, const float *ihalf, int32_t R, float *out, void *stream);
int drx_ncf_pair_scores(const DrxNcfDims *D, const float *sw, const float *uhalf, const float *ihalf, const int32_t *urow,
                        const int32_t *irow, int32_t P, float *out, void *stream);

/* ---- GRU4Rec (Hidasi, Karatzoglou, Baltrunas, Tikk 2016; csrc/drx_gru.hip) ----------------------------------
 * Tables E [n_items, ldk] (input embeddings, k floats of a row used) and Q [n_items, ldh] (output rows, h floats used), b [n_items];
 * ldk / ldh = k / h rounded up to a multiple of 4, the padding columns ZERO.  One flat array sw of small weights, in this order, all
 * row-major and WITHOUT padding (no row, gate block or bias is padded; DrxGruDims has the offsets, which must be exactly these):
 *     Wx [k, 3 h] at off_wx = 0 | Wh [h, 3 h] at off_wh = 3 k h | bx [3 h] at off_bx = 3 (k + h) h | bhn [h] at off_bhn = off_bx + 3 h
 *     n_small = off_bhn + h;  the 3 h gate columns are the blocks z | r | n of h columns each (column g h + c = gate g, unit c).
 * For a window's ordered items s_1 .. s_L, h_0 = 0, x_t = E[s_t]:
 *     z_t = sigmoid(x_t Wx_z + h_{t-1} Wh_z + bx_z),  r_t = sigmoid(x_t Wx_r + h_{t-1} Wh_r + bx_r)
 *     n_t = tanh(x_t Wx_n + bx_n + r_t (.) (h_{t-1} Wh_n + bhn)),  h_t = (1 - z_t) (.) n_t + z_t (.) h_{t-1}        (torch's GRU cell)
 *     x(S, i) = h_L . Q[i] + b[i]                                  (DRX_REC_BIAS of the fused scorer at rows of ldh floats)
 *     D_wk = x(S, i) - x(S, j_k);  loss = (1 / (B r)) sum_w sum_k softplus(-D_wk);  g_wk = -sigmoid(-D_wk) / (B r)
 * A position whose id is < 0 is no step: the row keeps its h (serving's short baskets; a step's windows hold L ids >= 0).
 * Domain: 1 <= k, h <= 64, 1 <= L <= 8, 1 <= neg_ratio <= 16.  Everything is fp32; no float atomics; every sum runs in an order fixed by
 * the arguments: equal inputs give equal bits.  All launches are plain. */
typedef struct DrxGruDims {
  int32_t n_items;
  int32_t k, h, ldk, ldh;
  int32_t off_wx, off_wh, off_bx, off_bhn, n_small;
} DrxGruDims;
/* ONE TRAINING STEP on B windows in the layout drx_list_sample_device returns at n_targets = 1: before [B, L], after [B, 1 + r] (the
 * target first), device int32, ids in range (not checked on the device).  Then EVERY row of E and Q and every entry of Wx, Wh gets
 * reg * itself added to its gradient (bx, bhn, b none) and everything is updated by `rule`, a dense rule (DrxOptRule).  alphas: HOST
 * float [3], the step sizes of E, sw and Q with b (Adam: the variable's lr_t; the other rules: the learning rate); rule->lr is ignored.
 * Slots: those the rule has, shaped like their parameter; one it lacks may be NULL and is not touched.
 * k_gru_tile: workgroups of four waves, drx_gru_grid of them = min(tiles, 256), walk tiles of 16 windows (tile t to workgroup
 * t % grid, ascending); wave w takes the 16-column tiles w, w + 4, w + 8 of the 3 h gate columns.  A tile gathers x_1 .. x_L into LDS,
 * runs the L steps forward (x_t Wx and h_{t-1} Wh as v_mfma_f32_16x16x4_f32 products, Wx / Wh read from global memory as the B
 * operand, every h_t kept in LDS), forms dh_L = sum_k g_wk (Q[i] - Q[j_k]), then runs the L steps backward: a step's gates are
 * recomputed from x_t and h_{t-1} by the forward's own function, dgates Wx^T gives the gradient row of E for (window, t) ([B L, ldk]),
 * dgates Wh^T the dh of the step before, and x_t^T dgates, h_{t-1}^T dgates add to the wave's tiles of dWx, dWh, which stay in
 * registers over all steps and tiles of the workgroup.  It writes h_L [B, ldh] and the 1 + r scales (sum_k g_wk, -g_w1 .. -g_wr) per
 * window, its gradient of sw into ITS row of [grid, n_small] and its loss into one double.  One launch adds those rows in workgroup
 * order and updates sw by segments (drx_opt_segments' arithmetic); drx_batch_csr_device groups the B L input keys and the
 * B (1 + r) item keys; ONE drx_rows_csr_opt_multi call updates E (plain form) and Q with b (outer-product form, group 1 + r, the
 * written h_L as its rows).
 * loss_out: device double [1] or NULL.  scratch: drx_gru_step_scratch_bytes (0 = a description outside the domain).
 * DRX_EINVAL, and nothing launched: a NULL pointer among D, E, sw, Q, b, before, after, rule, alphas, scratch; B < 1 (or >= 2^24); k or h
 * outside 1..64; L outside 1..8; neg_ratio outside 1..16; n_items < 1; ldk / ldh / offsets / n_small that are not the layout above; no
 * dense rule; a slot the rule has is NULL; E, Q or a slot of theirs not 16-byte aligned.  DRX_ESCRATCH: scratch too small. */
int drx_gru_grid(int32_t B);
size_t drx_gru_step_scratch_bytes(const DrxGruDims *D, int32_t B, int32_t L, int32_t neg_ratio);
int drx_gru_step(const DrxGruDims *D, float *E, float *sw, float *Q, float *b, float *E_s1, float *E_s2, float *sw_s1, float *sw_s2,
                 float *Q_s1, float *Q_s2, float *b_s1, float *b_s2, const int32_t *before, const int32_t *after, int32_t B, int32_t L,
                 int32_t neg_ratio, const DrxOptRule *rule, const float *alphas, float reg, double *loss_out, void *scratch,
                 size_t scratch_bytes, void *stream);
/* out[q, :] = h after the cell has run over the basket of uid[q], for n device user ids (in range, not checked on the device): the
 * query rows of the fused scorer, out [n, ldh], padding zero.  baskets: device int32 [n_users, L], -1 = an absent position (no step);
 * an empty basket gives a zero row.  Tiles of 16 users through the SAME device function as the step's forward pass; a row's bits
 * depend neither on its place in a tile nor on the other rows, and a basket of m < L items gives the bits of m steps.
 * DRX_EINVAL, and nothing launched: a NULL pointer; n < 1; L outside 1..8; dims outside the domain or not the layout above; E or out
 * not 16-byte aligned. */
int drx_gru_query_rows(const float *E, const float *sw, const DrxGruDims *D, const int32_t *baskets, int32_t L, const int32_t *uid,
                       int32_t n, float *out, void *stream);

/* ---- SASRec (Kang & McAuley 2018; csrc/drx_sas.hip) -----------------------------------------------------------
 * Tables E [n_items, ldh] (input embeddings) and Q [n_items, ldh] (output rows), h floats of a row used, b [n_items]; ldh = h rounded
 * up to a multiple of 4, the padding columns ZERO.  There is no user table.  One flat array sw of small weights, all row-major and
 * WITHOUT padding, every regularised entry first and every unregularised one behind (DrxSasDims has the offsets, which must be exactly
 * these):
 *     Pos [L, h] at off_pos = 0 | block 0: Wq Wk Wv W1 W2 [h, h] each, from off_blk = L h | block 1 the same | ...
 *     off_vec = off_blk + 5 h h blocks: block 0: b1 b2 ln1_g ln1_b ln2_g ln2_b [h] each | block 1 the same | ...
 *     off_lnf = off_vec + 6 h blocks: lnf_g lnf_b [h] each;  n_small = off_lnf + 2 h.
 * A sequence of m <= L items occupies the positions L - m .. L - 1 (the newest item at L - 1); absent positions are never keys and
 * are not computed as queries.  For position t holding item s, one head:
 *     X0_t = E[s] + Pos[t];  LN(x) = (x - mean) / sqrt(var + 1e-5) g + beta, the biased variance over the h columns
 *     per block: A = LN(X; ln1);  q, k, v = A Wq, A Wk, A Wv;  S_tj = q_t . k_j / sqrt(h) for present j <= t;  P = softmax_j(S);
 *                X' = X + P v;  F = LN(X'; ln2);  X'' = X' + relu(F W1 + b1) W2 + b2
 *     h(S) = LN(X_{L-1}; lnf) after the last block; an empty sequence: h = 0 exactly
 *     x(S, i) = h(S) . Q[i] + b[i]                                 (DRX_REC_BIAS of the fused scorer at rows of ldh floats)
 *     D_wk = x(S, i) - x(S, j_k);  loss = (1 / (B r)) sum_w sum_k softplus(-D_wk);  g_wk = -sigmoid(-D_wk) / (B r)
 * Domain: 1 <= h <= 64, 1 <= L <= 16, blocks 1 or 2, 1 <= neg_ratio <= 16.  Everything is fp32; no float atomics; every sum runs in an
 * order fixed by the arguments: equal inputs give equal bits.  All launches are plain. */
typedef struct DrxSasDims {
  int32_t n_items;
  int32_t h, ldh, L, blocks;
  int32_t off_pos, off_blk, off_vec, off_lnf, n_small;
} DrxSasDims;
/* ONE TRAINING STEP on B windows in the layout drx_list_sample_device returns at n_targets = 1: before [B, L] (full windows, ids >= 0),
 * after [B, 1 + r] (the target first), device int32, ids in range (not checked on the device).  Then EVERY row of E and Q and every
 * entry of Pos and of the five matrices of every block gets reg * itself added to its gradient (the biases, the LN gains and offsets and
 * b none) and everything is updated by `rule`, a dense rule (DrxOptRule).  alphas: HOST float [3], the step sizes of E, sw and Q with b
 * (Adam: the variable's lr_t; the other rules: the learning rate); rule->lr is ignored.  Slots: those the rule has, shaped like their
 * parameter; one it lacks may be NULL and is not touched.
 * k_sas_tile: workgroups of four waves, drx_sas_grid of them = min(B, 256), walk the windows (window w to workgroup w % grid,
 * ascending).  ONE WINDOW IS ONE MFMA TILE whose 16 rows are the positions, so S = q k^T is one 16 x 16 accumulator and the causal and
 * presence masks are a test on (row, column); wave w takes the 16-column tile w of h.  The projections, q k^T, P v, the two FFN
 * layers, their transposes in the backward pass and the x^T dY weight gradients are v_mfma_f32_16x16x4_f32 products, the weights read
 * from global memory as the B operand; LN, the softmax and ReLU run row-wise on the VALU.  Every activation of the window's forward pass
 * stays in LDS for its backward pass (nothing is recomputed but the LN statistics; nothing goes to scratch).  A wave's tiles of the
 * five weight gradients of every block stay in registers over all windows of the workgroup; the gradients of Pos and of the vectors
 * add up in LDS.  The kernel writes the gradient rows of E [B L, ldh], h [B, ldh] and the 1 + r scales (sum_k g_wk, -g_w1 .. -g_wr)
 * per window, its gradient of sw into ITS row of [grid, n_small] and its loss into one double.  One launch adds those rows in workgroup
 * order and updates sw by two segments (drx_opt_segments' arithmetic); drx_batch_csr_device groups the B L input keys and the
 * B (1 + r) item keys; ONE drx_rows_csr_opt_multi call updates E (plain form) and Q with b (outer-product form, group 1 + r, the
 * written h as its rows).
 * loss_out: device double [1] or NULL.  scratch: drx_sas_step_scratch_bytes (0 = a description outside the domain).
 * DRX_EINVAL, and nothing launched or written: a NULL pointer among D, E, sw, Q, b, before, after, rule, alphas, scratch; B < 1 (or
 * >= 2^24); h outside 1..64; L outside 1..16; blocks outside 1..2; neg_ratio outside 1..16; n_items < 1; ldh / offsets / n_small that
 * are not the layout above; no dense rule; a slot the rule has is NULL; E, Q or a slot of theirs not 16-byte aligned.  DRX_ESCRATCH:
 * scratch too small. */
int drx_sas_grid(int32_t B);
size_t drx_sas_step_scratch_bytes(const DrxSasDims *D, int32_t B, int32_t neg_ratio);
int drx_sas_step(const DrxSasDims *D, float *E, float *sw, float *Q, float *b, float *E_s1, float *E_s2, float *sw_s1, float *sw_s2,
                 float *Q_s1, float *Q_s2, float *b_s1, float *b_s2, const int32_t *before, const int32_t *after, int32_t B,
                 int32_t neg_ratio, const DrxOptRule *rule, const float *alphas, float reg, double *loss_out, void *scratch,
                 size_t scratch_bytes, void *stream);
/* out[q, :] = h of the basket of uid[q], for n device user ids (in range, not checked on the device): the query rows of the fused
 * scorer, out [n, ldh], padding zero.  baskets: device int32 [n_users, L], LEFT-aligned, -1 = an absent position; the kernel shifts a
 * basket of m items to the positions L - m .. L - 1.  An empty basket gives a zero row.  One user per tile through the SAME device
 * function as the step's forward pass: a row's bits depend neither on its place in the request nor on the other rows, and a full
 * basket gives the bits of the h the step writes for the same window.
 * DRX_EINVAL, and nothing launched: a NULL pointer; n < 1; dims outside the domain or not the layout above; E or out not 16-byte
 * aligned. */
int drx_sas_query_rows(const float *E, const float *sw, const DrxSasDims *D, const int32_t *baskets, const int32_t *uid, int32_t n,
                       float *out, void *stream);

/* ---- Mult-VAE / Mult-DAE (Liang, Krishnan, Hoffman, Jebara 2018; csrc/drx_vae.hip) ---------------------------
 * Tables W_in [n_items, ldh] (the embedding-bag first layer) and W_out [n_items, ldh] (the output rows), h floats of a row used,
 * b_out [n_items]; ldh = h rounded up to a multiple of 4, the padding columns ZERO.  One flat array sw of small weights, all row-major
 * and WITHOUT padding, the regularised entries first (DrxVaeDims has the offsets, which must be exactly these; e = 2 latent where
 * variational, else latent):
 *     W_e [h, e] at off_we = 0 | W_d [latent, h] at off_wd = h e || off_vec = off_wd + latent h: b_in [h] | b_e [e] | b_d [h];
 *     n_small = off_vec + 2 h + e.
 * For batch row b with user u, P_u the user's row of the positives CSR (ascending items), N_u = |P_u|:
 *     x1 = c_b sum_{kept lookups j} W_in[P_u[j]] + b_in,  c_b = 1 / (sqrt(N_u) (1 - dropout));  h1 = tanh(x1)
 *     [mu | logvar] = h1 W_e + b_e;  z = mu + eps exp(logvar / 2) (variational and eps given), else z = mu
 *     h2 = tanh(z W_d + b_d);  logit_i = h2 . W_out[i] + b_out[i] for EVERY item  (DRX_REC_BIAS of the fused scorer at rows of ldh)
 *     loss_b = -sum_{i in P_u} log softmax(logit)_i + kl_weight KL_b,  KL_b = -1/2 sum (1 + logvar - mu^2 - exp(logvar));
 *     loss = mean_b loss_b;  dlogit_bi = (N_u softmax_i - [i in P_u]) / B
 * Domain: 1 <= h <= 128, 1 <= latent <= 64, 1 <= B <= 65536.  Everything is fp32; no float atomics; every sum runs in an order fixed by
 * the arguments: equal inputs give equal bits.  All launches are plain. */
typedef struct DrxVaeDims {
  int32_t n_items;
  int32_t h, ldh, latent, variational, e;
  int32_t off_we, off_wd, off_vec, n_small;
} DrxVaeDims;
/* ONE TRAINING STEP on the B users uid (device int32, in range: not checked on the device).  Hst: the positives CSR on the device.
 * boff [B + 1] (device int32): boff[b] = sum of N_u over the rows before b — lookup j of row b is lookup boff[b] + j of the batch;
 * T = boff[B] >= 1; max_len >= every N_u of the batch (T <= B max_len < 2^31).  eps [B, latent] floats or NULL (z = mu); keep [T]
 * bytes or NULL (every lookup kept): what drx_vae_noise writes, or explicit arrays.  kl_weight: beta_t of the step.  Then EVERY row of
 * W_in and W_out and every entry of W_e and W_d gets reg * itself added to its gradient (the biases none) and everything is updated by
 * `rule`, a dense rule.  alphas: HOST float [3], the step sizes of W_in, sw and W_out with b_out; rule->lr is ignored.
 * No array of B x n_items floats exists.  k_vae_encode (row tiles of 16): the bag, h1, [mu | logvar], z, h2, the KL partials, the keys
 * and scales (keep ? c_b : 0) of the W_in update.  k_vae_lse (pass 1): min(item tiles, 128) persistent workgroups walk the item tiles
 * g, g + grid, ..; the logits of a 16 x 16 tile are one MFMA accumulator; a running (max, sum) per row and workgroup, combined in
 * workgroup order (k_vae_lse_combine).  k_vae_out (pass 2, same grid): the tile's logits again, dlogit (membership by a binary search
 * in the user's CSR row), the tile's dW_out / db_out over ALL rows (the four waves' sums added in wave order) and the dense rule on
 * its rows of W_out, b_out and their slots in place, and the workgroup's slab of dh2 = dlogit W_out.  k_vae_back (row tiles): the
 * slabs summed in slab order, the backward pass of the small layers, dx1 [B, ldh], the workgroup's row of small-weight partials.  One
 * k_small_opt launch updates sw; drx_batch_csr_device groups the T lookups by item; ONE drx_rows_csr_opt_multi call updates W_in in
 * the outer-product form (group max_len, the rows of dx1, the scales).
 * loss_out: device double [1] or NULL.  scratch: drx_vae_step_scratch_bytes (0 = a description outside the domain).
 * DRX_EINVAL, and nothing launched or written: a NULL pointer among D, W_in, sw, W_out, b_out, Hst and its arrays, uid, boff, rule,
 * alphas, scratch; h outside 1..128; latent outside 1..64; B outside 1..65536; T < 1; max_len outside 1..n_items; T > B max_len or
 * B max_len >= 2^31; dropout outside [0, 1); kl_weight < 0; offsets / ldh / e / n_small that are not the layout above; no dense
 * rule; a slot the rule has is NULL; W_in, W_out or a slot of theirs not 16-byte aligned.  DRX_ESCRATCH: scratch too small. */
size_t drx_vae_step_scratch_bytes(const DrxVaeDims *D, int32_t B, int32_t T, int32_t max_len);
int drx_vae_step(const DrxVaeDims *D, float *W_in, float *sw, float *W_out, float *b_out, float *W_in_s1, float *W_in_s2, float *sw_s1,
                 float *sw_s2, float *W_out_s1, float *W_out_s2, float *b_out_s1, float *b_out_s2, const DrxHistory *Hst,
                 const int32_t *uid, const int32_t *boff, int32_t B, int32_t T, int32_t max_len, const float *eps, const uint8_t *keep,
                 float dropout, float kl_weight, const DrxOptRule *rule, const float *alphas, float reg, double *loss_out, void *scratch,
                 size_t scratch_bytes, void *stream);
/* The randomness of a step, a function of `seed` alone: keep[boff[b] + j] = drx_hash_u32(2 seed, b, j) >= q_threshold(dropout);
 * words[2 (b latent + c)], words[.. + 1] = w1, w2 = drx_hash_u32(2 seed + 1, b, 2 c), (.., 2 c + 1);  eps[b latent + c] =
 * sqrt(-2 ln u1) cos(2 pi u2) in fp32 with u1 = (w1 + 1) / 2^32, u2 = w2 / 2^32.  eps, keep, words: each may be NULL (not written).
 * DRX_EINVAL: boff NULL; B outside 1..65536; T < 0; latent outside 1..64; dropout outside [0, 1). */
int drx_vae_noise(uint64_t seed, const int32_t *boff, int32_t B, int32_t T, int32_t latent, float dropout, float *eps, uint8_t *keep,
                  uint32_t *words, void *stream);
/* out[q, :] = h2 of user uid[q] at z = mu, no dropout, every positive kept, for n device user ids (in range, not checked): the query
 * rows of the fused scorer, out [n, ldh], padding zero; a user without positives gives tanh(b_in) onwards.  Tiles of 16 users through
 * the SAME device function as the step's forward pass: a row's bits depend neither on its place nor on the other rows.
 * DRX_EINVAL, and nothing launched: a NULL pointer; n < 1; dims outside the domain or not the layout above; W_in or out not 16-byte
 * aligned. */
int drx_vae_query_rows(const float *W_in, const float *sw, const DrxVaeDims *D, const DrxHistory *Hst, const int32_t *uid, int32_t n,
                       float *out, void *stream);

/* ---- LightGCN (He, Deng, Wang, Li, Zhang, Wang 2020; csrc/drx_lgcn.hip) --------------------------------------
 * Nodes: the n_users users, then the n_items items, N = n_users + n_items.  E0 = [P ; Q], [N, ld], ld = K rounded up to a multiple of
 * 4, 4 <= ld <= 256, the padding columns zero — every call below keeps them zero.  A = the symmetric normalised adjacency of the
 * positives: A[r, c] = w[r] w[c] on every edge, w[v] = deg(v)^(-1/2), 0 for a node without edges.  Final embeddings
 * Ebar = (1 / (layers + 1)) sum_{l = 0 .. layers} A^l E0; score x(u, i) = Ebar[u] . Ebar[n_users + i] (DRX_REC_BIAS of the fused scorer
 * with a zero bias).  0 <= layers <= DRX_LGCN_MAX_LAYERS.
 *
 * THE GRAPH (built once by the host, arrays on the device): the CSR of the symmetric adjacency — a user row lists n_users + iid
 * ascending, an item row lists uids ascending —, w, and the cut of long rows: row r is cut into max(1, ceil(len_r / S)) segments of
 * S = drx_lgcn_row_split() entries (the last one shorter), seg_ptr [N + 1] their prefix sums, seg_row [n_seg] the row of every segment,
 * cut_rows [n_cut] the rows of more than one segment, ascending (NULL where n_cut == 0).  Indices lie in [0, N) and the segment arrays
 * fit the CSR (neither is checked on the device). */
#define DRX_LGCN_MAX_LAYERS 4
typedef struct DrxLgcnGraph {
  const int64_t *indptr;     /* [N + 1] */
  const int32_t *indices;    /* [nnz2] */
  const float *w;            /* [N] */
  const int32_t *seg_row;    /* [n_seg] */
  const int32_t *seg_ptr;    /* [N + 1] */
  const int32_t *cut_rows;   /* [n_cut] */
  int32_t N, n_seg, n_cut;
} DrxLgcnGraph;
/* S: rows of more than S entries are cut (0 would mean: never) */
int32_t drx_lgcn_row_split(void);
/* ONE PROPAGATION   out[r, :] = scale (base[r, :] + w[r] sum_{c in row r, CSR order} w[c] in[c, :])      (base NULL: no base term)
 * A group of pick_geom(ld) lanes per segment, one float4 per lane, 4 neighbour rows in flight per group; a row of one segment is
 * finished where it is summed, a cut row leaves one partial row per segment in `part` and a second launch adds them in segment order.
 * No atomics: the sum of a row runs in an order fixed by the CSR and S alone, so equal inputs give equal bits.  `base` may be `in`;
 * `out` must be neither.  part: device, drx_lgcn_part_bytes (0 = an invalid description); may be NULL where no row is cut.
 * DRX_EINVAL, and nothing launched: graph NULL or one of its arrays NULL (cut_rows with n_cut > 0), N < 1, n_seg < N; in or out NULL;
 * out == in or out == base; ld outside 4..256 or no multiple of 4; base, in, out or part not 16-byte aligned; part NULL with a cut row.
 * DRX_ESCRATCH: part too small. */
size_t drx_lgcn_part_bytes(const DrxLgcnGraph *graph, int32_t ld);
int drx_lgcn_propagate(const DrxLgcnGraph *graph, const float *base, const float *in, float *out, int32_t ld, float scale, void *part,
                       size_t part_bytes, void *stream);
/* THE FINAL EMBEDDINGS in Horner form: S <- E0, `layers` times S <- E0 + A S (drx_lgcn_propagate with base = E0), the last one with
 * scale = 1 / (layers + 1), into out [N, ld]; layers == 0: a copy of E0.  It is the function the step's forward pass calls: out has the
 * bits the next drx_lgcn_step on the same E0 computes.  scratch: drx_lgcn_final_scratch_bytes (0 = an invalid description).
 * DRX_EINVAL, and nothing launched: a NULL pointer (E0, out, scratch, graph and its arrays); out == E0; N < 1; ld outside 4..256 or no
 * multiple of 4; layers outside 0..4; E0 or out not 16-byte aligned.  DRX_ESCRATCH: scratch too small. */
size_t drx_lgcn_final_scratch_bytes(const DrxLgcnGraph *graph, int32_t ld);
int drx_lgcn_final(const float *E0, const DrxLgcnGraph *graph, int32_t layers, int32_t ld, float *out, void *scratch, size_t scratch_bytes,
                   void *stream);
/* ONE TRAINING STEP on T triples (uid, pos, neg: device int32 [T], user and item ids in range — not checked on the device):
 *     D_t = x(u, i) - x(u, j);   loss = (1 / T) sum_t softplus(-D_t);   g_t = -sigmoid(-D_t) / T
 *     G[u] += g_t (Ebar[i'] - Ebar[j']);  G[i'] += g_t Ebar[u];  G[j'] -= g_t Ebar[u]          (i' = n_users + i, j' = n_users + j)
 *     dE0 = (1 / (layers + 1)) sum_l A^l G   (A is symmetric), by the same Horner recurrence on G
 * then EVERY row of E0 gets reg * row added to its gradient and is updated by `rule`, a dense rule (DrxOptRule).  alphas: HOST float
 * [2], the step sizes of P (rows 0 .. n_users) and Q (the rest); rule->lr is ignored.  Slots: those the rule has, shaped like P and Q;
 * one it lacks may be NULL and is not touched.
 * One call: the forward recurrence into the scratch; k_lgcn_fwd_bwd (a lane group per triple, the three rows read once, the loss
 * partials summed in double in workgroup order) leaves three gradient rows per triple; drx_batch_csr_device groups the 3 T node keys;
 * one kernel over all N rows sums each row's lookups in batch order into the dense G, zeros included; the backward recurrence;
 * drx_opt_dense on each half.  layers == 0 runs no propagation (matrix factorisation without a bias).  No atomics, equal inputs give
 * equal bits.  loss_out: device double [1] or NULL.  scratch: drx_lgcn_step_scratch_bytes (0 = an invalid description); for
 * layers >= 1 the forward's Ebar [N, ld] is left at its first 256-byte boundary.
 * DRX_EINVAL, and nothing launched or written: a NULL pointer among E0, graph and its arrays, uid, pos, neg, rule, alphas, scratch;
 * T < 1 (or >= 2^27); N < 1; n_users outside 1..N-1; ld outside 4..256 or no multiple of 4; layers outside 0..4; no dense rule; a slot
 * the rule has is NULL; E0 or a slot not 16-byte aligned.  DRX_ESCRATCH: scratch too small. */
size_t drx_lgcn_step_scratch_bytes(const DrxLgcnGraph *graph, int32_t T, int32_t ld, int32_t n_users);
int drx_lgcn_step(float *E0, float *P_s1, float *P_s2, float *Q_s1, float *Q_s2, int32_t ld, int32_t n_users, const DrxLgcnGraph *graph,
                  const int32_t *uid, const int32_t *pos, const int32_t *neg, int32_t T, int32_t layers, const DrxOptRule *rule,
                  const float *alphas, float reg, double *loss_out, void *scratch, size_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DRX_H_ */
