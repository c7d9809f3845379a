"""Device-side state of a UserKNN / ItemKNN model and the calls into libdrx.so (include/drx.h drx_knn_*).

Holds both orientations of the rating CSR, the neighbour table and the fallback means as torch tensors on one MI355X — torch is the
container; every number is computed by the HIP kernels of csrc/drx_knn.hip.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .engine_rows import RowsRecommender, pack_mask_bits


class KnnEngine(RowsRecommender):
    DENSE_BUDGET_BYTES = 8 << 30        # the dense fp32 matrix drx_knn_neighbours stages in its scratch
    MAX_K = 128                         # the kernel's domain
    FUSED_MAX_N = 128                   # the longest list drx_knn_recommend selects (a longer one: score_rows + topk)
    SCRATCH_CHUNK_BYTES = 1 << 30       # rows past LDS: the working rows of one launch of the fused kernels stay within this

    def __init__(self, n_users, n_items, kind, device='cuda:0'):
        assert kind in ('user', 'item'), kind
        self.n_users, self.n_items, self.kind = int(n_users), int(n_items), kind
        self.type = _lib.KNN_USER if kind == 'user' else _lib.KNN_ITEM
        self.device = torch.device(device)
        self.k = None
        self.nb_idx = self.nb_sim = None
        self.fused = True               # False: recommend_batch / catalogue_ranks of the public classes keep the score-matrix route

    # ---- the ratings ---------------------------------------------------------------------------------------------------------------
    def _upload_csr(self, csr, n_rows):
        indptr, indices, values = csr
        ip = np.ascontiguousarray(indptr, dtype=np.int64)
        assert len(ip) == n_rows + 1 and int(ip[-1]) == len(indices) == len(values)
        ix = np.ascontiguousarray(indices, dtype=np.int32)
        v = np.ascontiguousarray(values, dtype=np.float32)
        pad = (lambda a: a if len(a) else np.zeros(1, a.dtype))
        return (torch.as_tensor(ip).to(self.device), torch.as_tensor(pad(ix)).to(self.device), torch.as_tensor(pad(v)).to(self.device),
                int(ip[-1]))

    def set_interactions(self, csr, csr_t):
        """The [n_users, n_items] CSR (indptr, columns ascending and unique, values) and its transpose; the means of both sides."""
        self._u = self._upload_csr(csr, self.n_users)
        self._i = self._upload_csr(csr_t, self.n_items)
        self.user_mean = self._row_means(self._u, self.n_users)
        self.item_mean = self._row_means(self._i, self.n_items)

    def _row_means(self, d_csr, n_rows):
        out = torch.empty(n_rows, dtype=torch.float64, device=self.device)
        check(lib().drx_knn_row_means(ptr(d_csr[0]), ptr(d_csr[2]), d_csr[3], n_rows, ptr(out), stream_ptr(self.device)), 'drx_knn_row_means')
        return out

    def dense_bytes(self):
        R, C = (self.n_users, self.n_items) if self.kind == 'user' else (self.n_items, self.n_users)
        return ((R + 127) // 128 * 128) * ((C + 7) // 8 * 8) * 4

    # ---- the neighbour table -------------------------------------------------------------------------------------------------------
    def neighbours(self, metric, k, m, shrinkage, max_diff=1.0, splits=0):
        """Builds the table (int32 [R, k] ids, float32 [R, k] similarities, on the device) over users (UserKNN) or items (ItemKNN)."""
        if metric not in _lib.KNN_METRICS:
            raise Exception(f'There is no similarity metric corresponding to the name "{metric}".')
        k = int(k)
        if not 1 <= k <= self.MAX_K:
            raise ValueError(f'k = {k} is outside the neighbour kernel\'s domain 1..{self.MAX_K}')
        if self.dense_bytes() > self.DENSE_BUDGET_BYTES:
            raise MemoryError(f'the dense rating matrix of this model takes {self.dense_bytes()} bytes, above '
                              f'KnnEngine.DENSE_BUDGET_BYTES = {self.DENSE_BUDGET_BYTES}')
        d_csr, R, C = (self._u, self.n_users, self.n_items) if self.kind == 'user' else (self._i, self.n_items, self.n_users)
        L = lib()
        need = int(L.drx_knn_neighbours_scratch_bytes(R, C, k, int(splits)))
        assert need > 0, (R, C, k, splits)
        scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        idx = torch.empty(R, k, dtype=torch.int32, device=self.device)
        sim = torch.empty(R, k, dtype=torch.float32, device=self.device)
        check(L.drx_knn_neighbours(ptr(d_csr[0]), ptr(d_csr[1]), ptr(d_csr[2]), d_csr[3], R, C, _lib.KNN_METRICS[metric], k, int(m),
                                   -1.0 if shrinkage is None else float(shrinkage), float(max_diff), int(splits), ptr(idx), ptr(sim),
                                   ptr(scratch), need, stream_ptr(self.device)), 'drx_knn_neighbours')
        self.set_table(idx, sim)
        return idx, sim

    def set_table(self, idx, sim):
        idx = torch.as_tensor(idx).to(self.device, torch.int32).contiguous()
        sim = torch.as_tensor(sim).to(self.device, torch.float32).contiguous()
        assert idx.shape == sim.shape and idx.shape[0] == (self.n_users if self.kind == 'user' else self.n_items)
        self.nb_idx, self.nb_sim, self.k = idx, sim, int(idx.shape[1])

    def get_params(self):
        return {'nb_idx': self.nb_idx.cpu().numpy(), 'nb_sim': self.nb_sim.cpu().numpy()}

    # ---- predictions ---------------------------------------------------------------------------------------------------------------
    def _model_args(self, aggregation):
        ip, ix, v, nnz = self._u
        return (self.type, _lib.KNN_AGGREGATIONS[aggregation], ptr(ip), ptr(ix), ptr(v), nnz, self.n_users, self.n_items, ptr(self.nb_idx),
                ptr(self.nb_sim), self.k)

    def score_rows(self, uids, cand, aggregation, use_averages=False):
        """(scores float32 [R, n_items], the packed candidate mask with the items the model has no prediction for cleared), both on
        the device: what topk() takes.  cand: host bool [R, n_items].  use_averages (ItemKNN): a user's mean where an item has no
        term, so every candidate keeps its bit."""
        uid = self._dev_i32(uids)
        R = int(uid.numel())
        out = torch.empty(R, self.n_items, dtype=torch.float32, device=self.device)
        mask = torch.as_tensor(pack_mask_bits(cand).view(np.int32)).to(self.device)
        L = lib()
        need = int(L.drx_knn_score_rows_scratch_bytes(self.type, R, self.n_items))
        scratch = torch.empty(need, dtype=torch.uint8, device=self.device) if need else None
        fb = self.user_mean if use_averages and self.kind == 'item' else None
        check(L.drx_knn_score_rows(*self._model_args(aggregation), ptr(uid), R, ptr(fb), ptr(out), ptr(mask), ptr(scratch), need,
                                   stream_ptr(self.device)), 'drx_knn_score_rows')
        return out, mask

    def unpack_mask(self, mask, R):
        """the device mask of score_rows as a host bool [R, n_items]"""
        bits = np.unpackbits(mask.cpu().numpy().view(np.uint8), bitorder='little')[:R * self.n_items]
        return bits.astype(bool).reshape(R, self.n_items)

    def pair_scores(self, uids, iids, aggregation, use_averages=False):
        """(float64 [P], uint8 [P] 1 = no prediction) on the device for parallel internal ids"""
        uid, iid = self._dev_i32(uids), self._dev_i32(iids)
        P = int(uid.numel())
        assert P == int(iid.numel()), 'pair_scores takes parallel users and items'
        out = torch.empty(P, dtype=torch.float64, device=self.device)
        none = torch.empty(P, dtype=torch.uint8, device=self.device)
        fb = (self.user_mean if self.kind == 'item' else self.item_mean) if use_averages else None
        check(lib().drx_knn_pair_scores(*self._model_args(aggregation), ptr(uid), ptr(iid), P, ptr(fb), ptr(out), ptr(none),
                                        stream_ptr(self.device)), 'drx_knn_pair_scores')
        return out, none

    # ---- top-n and catalogue ranks without the score matrix (include/drx.h drx_knn_recommend / drx_knn_rank_lists) -----------------------
    def _fallback(self, use_averages):
        return self.user_mean if use_averages and self.kind == 'item' else None

    def recommend(self, uids, n, aggregation, use_averages=False, exclude=None, chunk_bytes=None):
        """(idx int32 [R, n], val float32 [R, n]) on the device: per user the n <= FUSED_MAX_N best items the model has a prediction
        for, drx_topk's order, -1 / -inf behind the last; exclude: without the user's row of set_exclusions().  One launch while a
        working row fits LDS; past it `chunk_bytes` (SCRATCH_CHUNK_BYTES) of working rows at a time."""
        uid, n, excl, out_idx, out_val = self._recommend_request(uids, n, exclude)
        R = int(uid.numel())
        L = lib()
        if not 1 <= n <= self.FUSED_MAX_N:
            raise _lib.DrxError(f'drx_knn_recommend: n = {n} lies outside the fused domain 1..{self.FUSED_MAX_N}')
        per = self._fused_chunk(int(L.drx_knn_recommend_scratch_bytes(self.type, 1, self.n_items, n)), R, chunk_bytes)
        fb = self._fallback(use_averages)
        for lo, hi in self._chunks(R, per):
            r = hi - lo
            need = int(L.drx_knn_recommend_scratch_bytes(self.type, r, self.n_items, n))
            sc = self._rows_scratch(need)
            check(L.drx_knn_recommend(*self._model_args(aggregation), ptr(uid[lo:lo + r]), r, n, ptr(fb), *self._excl_ptrs(excl),
                                      ptr(out_idx[lo:lo + r]), ptr(out_val[lo:lo + r]), ptr(sc), need,
                                      stream_ptr(self.device)), 'drx_knn_recommend')
        return out_idx, out_val

    def _fused_chunk(self, one_row_bytes, R, chunk_bytes):
        """rows per launch: all of them while the kernels need no scratch"""
        if one_row_bytes == 0:
            return max(R, 1)
        return max(1, int(chunk_bytes or self.SCRATCH_CHUNK_BYTES) // one_row_bytes)

    def rank_lists(self, uids, indptr, targets, aggregation, use_averages=False, exclude=None, chunk_bytes=None):
        """(rank int32 [P], score float32 [P]) on the device, parallel to `targets`: row r (user uids[r]) owns targets[indptr[r] :
        indptr[r + 1]]; the rank is the number of eligible items ahead of the target in recommend()'s order with n unbounded, -1 / -inf
        for a target outside the catalogue or without a prediction.  A target's own exclusion is ignored."""
        uid, ip, d_ip, tg, excl = self._rank_lists_request(uids, indptr, targets, exclude)
        R, P = int(uid.numel()), int(tg.numel())
        out_rank, out_score = self._outputs(P)
        if R == 0 or P == 0:
            return out_rank, out_score
        L = lib()
        per = self._fused_chunk(int(L.drx_knn_rank_lists_scratch_bytes(self.type, 1, P, self.n_items)), R, chunk_bytes)
        fb = self._fallback(use_averages)
        for lo, hi in self._chunks(R, per):
            r = hi - lo
            need = int(L.drx_knn_rank_lists_scratch_bytes(self.type, r, P, self.n_items))
            sc = self._rows_scratch(need)
            check(L.drx_knn_rank_lists(*self._model_args(aggregation), ptr(uid[lo:lo + r]), r, ptr(d_ip[lo:]), ptr(tg), P, ptr(fb),
                                       *self._excl_ptrs(excl), ptr(out_rank), ptr(out_score),
                                       ptr(sc), need, stream_ptr(self.device)), 'drx_knn_rank_lists')
        return out_rank, out_score
