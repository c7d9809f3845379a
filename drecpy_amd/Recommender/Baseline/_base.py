"""What the factor baselines share (DESIGN.md sections 3.7 - 3.11).  A new baseline starts from these two classes:

    FactorServing     prediction and serving of a model whose engine is a RowsRecommender: x(u, i) = query row . table row + bias on the
                      fused scorer (ALS, BPR, FPMC, GRU4Rec), the candidate ranking of rank() on the engine's score matrix (NeuMF too).
    SampledDenseFit   the fit() half of a model trained on sampled batches by one fused dense step (BPR, FPMC, NeuMF, GRU4Rec): the refusals,
                      the seed of every draw, the apply positions of the step and the softplus batch loss.

A model says what differs as class data (MODEL, NEGATIVES_PER, MAX_NEG_RATIO, DENSE_UPDATE_OF) and keeps its own _pre_fit, sampler and
engine."""
import numpy as np

from ..recommender_abc import RecommenderABC

_DENSE_KINDS = ('adam', 'adagrad', 'sgd', 'momentum', 'nesterov', 'rmsprop', 'rmsprop_momentum')


def last_items_baskets(sampler, n_users, L):
    """[n_users, L] int32, left-aligned, -1 = absent: the last min(L, len) ids of every user's sequence as the list sampler orders and
    thresholds it — the serving baskets of the sequence-aware baselines (FPMC, GRU4Rec)"""
    out = np.full((int(n_users), int(L)), -1, dtype=np.int32)
    if getattr(sampler, '_native', None) is None:
        return out
    indptr, row_ids, _ = sampler._twin_arrays
    for g, u in enumerate(np.asarray(sampler._group_values).tolist()):
        row = row_ids[max(int(indptr[g]), int(indptr[g + 1]) - int(L)):int(indptr[g + 1])]
        out[int(u), :len(row)] = row
    return out


class FactorServing(RecommenderABC):
    _reported_value = None          # what rank() reports for a device score; None: the score as it is (NeuMF: its sigmoid)

    def _predict(self, uid, iid, **kwds):
        if uid is None or iid is None:
            return None
        with self._device_lock:
            return float(self._engine.pair_scores(np.array([uid], dtype=np.int32), np.array([iid], dtype=np.int32)).cpu().numpy()[0])

    def _recorded_items(self, uid):
        """every item the frame records for the user, whatever its value (what novelty removes)"""
        indptr, cols = self._exclusion_csr()
        return np.asarray(cols[indptr[uid]:indptr[uid + 1]], dtype=np.int64)

    def _rank(self, uid, iids, n, novelty):
        """Top-n of the candidates by (score, iid) — heapq.nlargest order — on the device."""
        return self._rank_rows([uid], [list(iids)], n, novelty)[0]

    def _rank_rows(self, uids, iid_lists, n, novelty):
        """_rank for many users in one engine call: row r holds the top-n of the candidates iid_lists[r] for the internal user uids[r]."""
        cand = self._candidate_rows(iid_lists)
        if novelty:
            for r, uid in enumerate(uids):
                cand[r, self._recorded_items(uid)] = False
        rows = self._topk_of_candidates(cand, n, lambda: self._engine.score_matrix(np.asarray(uids, dtype=np.int32)))
        value = self._reported_value
        return rows if value is None else [[(float(value(x)), i) for x, i in row] for row in rows]

    def _recommend_batch(self, uids, n, novelty):
        """Top-n of the whole catalogue for many users in one engine call (the fused scorer-selector); lists longer than its domain
        (n > 128): one _recommend per user."""
        if not self._engine.recommend_is_fused(self._engine.rank_ld(), min(int(n), self.n_items)):
            return super()._recommend_batch(uids, n, novelty)
        return self._recommend_batch_fused(uids, n, novelty)

    def _catalogue_ranks(self, uids, iids, novelty):
        if not self._engine.rank_is_fused(self._engine.rank_ld()):
            return super()._catalogue_ranks(uids, iids, novelty)
        return self._catalogue_ranks_fused(uids, iids, novelty)

    def _predict_pairs(self, uids, iids):
        if type(self)._predict is not FactorServing._predict:
            return super()._predict_pairs(uids, iids)
        return self._predict_pairs_fused(uids, iids)


class SampledDenseFit(FactorServing):
    MODEL = None                    # the model's name in its messages
    NEGATIVES_PER = None            # what neg_ratio counts, in the words of its refusal
    MAX_NEG_RATIO = None            # None: no upper bound
    DENSE_UPDATE_OF = None          # what the dense rules update, in the words of _configure_optimizer's refusal

    def _start_sampled_fit(self, neg_ratio):
        """the refusals every sampled fit() opens with; then draw 1 is the next"""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            raise Exception(f'{self.MODEL}.fit under a torch.distributed process group: {self.MODEL} trains on a single GPU only.')
        top = self.MAX_NEG_RATIO
        if not (isinstance(neg_ratio, (int, np.integer)) and neg_ratio >= 1 and (top is None or neg_ratio <= top)):
            raise Exception(f'{self.MODEL}.fit(neg_ratio={neg_ratio!r}): neg_ratio must be an integer '
                            f'{">= 1" if top is None else f"in 1..{top}"} ({self.NEGATIVES_PER}).')
        self._neg_ratio = int(neg_ratio)
        self._draws = 0

    def _positives_frame(self):
        """(positives CSR, recorded CSR or None, eligible users) of the bound dataset"""
        indptr, cols, vals = self.interaction_dataset.interaction_csr()
        thr = self.interaction_threshold
        keep = np.ones(len(vals), bool) if thr is None else (np.asarray(vals) >= thr)
        if keep.all():
            positives, recorded, deg = (indptr, cols), None, np.diff(indptr)
        else:
            rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))[keep]
            ip = np.zeros(len(indptr), dtype=np.int64)
            ip[1:] = np.cumsum(np.bincount(rows, minlength=len(indptr) - 1))
            positives, recorded, deg = (ip, np.asarray(cols)[keep]), (indptr, cols), np.diff(ip)
        eligible = np.flatnonzero((deg >= 1) & (np.diff(indptr) < self.n_items)).astype(np.int32)
        return positives, recorded, eligible

    def _configure_optimizer(self):
        o = self.optimizer
        if getattr(o, 'kind', None) not in _DENSE_KINDS:
            raise Exception(f'{self.MODEL} trains with the dense rules adam, adagrad, sgd, rmsprop (dense update of {self.DENSE_UPDATE_OF}); '
                            f'got {o!r}')
        self._engine.set_optimizer(o)

    def _draw_seed(self, k):
        """the seed of the k-th batch (k = 1, 2, ...) of a fit()"""
        return (int(self.seed) if self.seed is not None else 0) * 1000003 + int(k)

    def _next_draw_seed(self):
        self._draws += 1
        return self._draw_seed(self._draws)

    def _do_batch(self, batch_samples, step=0, want_loss=False, **kwds):
        # one apply_gradients per registered item, in registration-list order
        applies = (len(self._apply_order()),) + tuple(self._apply_position(h) for h in self._fused_trainables())
        return self._engine.step(step, *batch_samples[:3], want_loss=want_loss, applies=applies)

    def _compute_batch_loss(self, predictions, desired_values, **kwds):
        """mean softplus(-d) of the pairwise differences d"""
        d = -np.asarray(predictions, dtype=np.float64)
        return float(np.mean(np.maximum(d, 0.0) + np.log1p(np.exp(-np.abs(d)))))
