"""BPR-MF (Rendle, Freudenthaler, Gantner, Schmidt-Thieme: "BPR: Bayesian Personalized Ranking from Implicit Feedback", UAI 2009) on the
MI355X engine — the matrix-factorisation baseline the CDAE and Caser papers report against.  The reference has no such model; the
definition of record is tests/bpr_oracle.py, the arithmetic csrc/drx_bpr.hip behind include/drx.h ("BPR-MF").

    score    x(u, i) = P[u] . Q[i] + bq[i]                      (`_predict` returns it as it is: a ranking score, not a rating)
    batch    batch_size (user, positive, negative) triples drawn on the device by a counter-based generator (drx_bpr_sample): a uniform
             eligible user, a uniform positive of it (interaction >= interaction_threshold), and for each of `neg_ratio` triples of that
             pair a uniform item the frame records nothing about for the user.  Draw k of a fit() uses the seed `_draw_seed(k)`.
    step     loss = mean softplus(-(x(u, i) - x(u, j))); reg_rate * row added to the gradient of EVERY row of P and Q (dense, like the
             other dense steps here; the biases are not regularised); one of the dense rules of fit(optimizer=...), Adam by default,
             P registered first, then Q with bq.

Prediction and serving run through the fused hooks of RecommenderABC (recommend_batch, catalogue_ranks, predict_pairs) on the engine's
DRX_REC_BIAS scorer; rank() / ranking_evaluation select on a score matrix (drx_rows_dot + drx_topk).  Single GPU only.
"""
import numpy as np

from ..recommender_abc import RecommenderABC

_DENSE_KINDS = ('adam', 'adagrad', 'sgd', 'momentum', 'nesterov', 'rmsprop', 'rmsprop_momentum')


class BPR(RecommenderABC):
    MAX_FACTORS = 256

    def __init__(self, factors=64, init_std=0.01, device='cuda:0', **kwds):
        super().__init__(**kwds)
        self.factors = factors
        self.init_std = init_std
        self.device = device

    # ---- fit -----------------------------------------------------------------------------------------------------------------------
    def _check_factors(self):
        if not (isinstance(self.factors, (int, np.integer)) and 1 <= self.factors <= self.MAX_FACTORS):
            raise Exception(f'BPR(factors={self.factors!r}): factors must be an integer in 1..{self.MAX_FACTORS}.')

    def _frame(self):
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

    def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            raise Exception('BPR.fit under a torch.distributed process group: BPR trains on a single GPU only.')
        if not (isinstance(neg_ratio, (int, np.integer)) and neg_ratio >= 1):
            raise Exception(f'BPR.fit(neg_ratio={neg_ratio!r}): neg_ratio must be an integer >= 1 (negatives drawn per positive pair).')
        self._check_factors()
        positives, recorded, eligible = self._frame()
        if len(eligible) == 0:
            raise Exception('BPR.fit: the dataset has no eligible user (one with an interaction >= interaction_threshold and at least '
                            'one item it has no interaction with).')
        from ...engine_bpr import BprEngine
        self._engine = BprEngine(self.n_users, self.n_items, int(self.factors), device=self.device)
        self._engine.lr, self._engine.reg = float(learning_rate), float(reg_rate)
        self._engine.set_sampler_frame(positives, recorded, eligible)
        weights = kwds.get('initial_weights')
        if weights is None:
            rng = np.random.default_rng(self.seed)
            weights = {'P': rng.normal(0.0, self.init_std, size=(self.n_users, self.factors)),
                       'Q': rng.normal(0.0, self.init_std, size=(self.n_items, self.factors)), 'bq': np.zeros(self.n_items)}
        self._engine.set_params(weights)
        self._register_trainables([self._engine.user_emb, self._engine.item_emb])
        self._neg_ratio = int(neg_ratio)
        self._draws = 0

    def _restore_engine(self, params):
        """RecommenderABC.load: the engine rebuilt from the saved weights (serving needs no sampler frame)"""
        from ...engine_bpr import BprEngine
        self._engine = BprEngine(self.n_users, self.n_items, int(self.factors), device=self.device)
        self._engine.set_params(params)

    def _fused_trainables(self):
        return [self._engine.user_emb, self._engine.item_emb]

    def _configure_optimizer(self):
        o = self.optimizer
        if getattr(o, 'kind', None) not in _DENSE_KINDS:
            raise Exception(f'BPR trains with the dense rules adam, adagrad, sgd, rmsprop (dense update of both factor tables); got {o!r}')
        self._engine.set_optimizer(o)

    def _draw_seed(self, k):
        """the seed of the k-th batch (k = 1, 2, ...) of a fit()"""
        return (int(self.seed) if self.seed is not None else 0) * 1000003 + int(k)

    def _sample_batch(self, batch_size, **kwds):
        self._draws += 1
        with self._device_lock:
            return self._engine.sample(batch_size, self._neg_ratio, self._draw_seed(self._draws))

    def _do_batch(self, batch_samples, step=0, want_loss=False, **kwds):
        e = self._engine
        # one apply_gradients per registered item, in registration-list order
        applies = (len(self._apply_order()), self._apply_position(e.user_emb), self._apply_position(e.item_emb))
        return e.step(step, *batch_samples[:3], want_loss=want_loss, applies=applies)

    def _predict_batch(self, batch_samples, **kwds):
        """x(u, i) - x(u, j) of the batch's triples (numpy float64 [T]) against the target 1 — the reference's training hook, kept for
        callers; the fused step computes its loss itself."""
        u, i, j = batch_samples[:3]
        with self._device_lock:
            xi, xj = self._engine.pair_scores(u, i).cpu().numpy(), self._engine.pair_scores(u, j).cpu().numpy()
        return xi.astype(np.float64) - xj.astype(np.float64), np.ones(len(xi))

    def _compute_batch_loss(self, predictions, desired_values, **kwds):
        d = -np.asarray(predictions, dtype=np.float64)
        return float(np.mean(np.maximum(d, 0.0) + np.log1p(np.exp(-np.abs(d)))))

    # ---- prediction and serving ------------------------------------------------------------------------------------------------------
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
        return self._topk_of_candidates(cand, n, lambda: self._engine.score_matrix(np.asarray(uids, dtype=np.int32)))

    def _recommend_batch(self, uids, n, novelty):
        """Top-n of the whole catalogue for many users in one engine call (the fused scorer-selector); lists longer than its domain
        (n > 128): one _recommend per user."""
        if not self._engine.recommend_is_fused(self._engine.ld, min(int(n), self.n_items)):
            return super()._recommend_batch(uids, n, novelty)
        return self._recommend_batch_fused(uids, n, novelty)

    def _catalogue_ranks(self, uids, iids, novelty):
        if not self._engine.rank_is_fused(self._engine.ld):
            return super()._catalogue_ranks(uids, iids, novelty)
        return self._catalogue_ranks_fused(uids, iids, novelty)

    def _predict_pairs(self, uids, iids):
        if type(self)._predict is not BPR._predict:
            return super()._predict_pairs(uids, iids)
        return self._predict_pairs_fused(uids, iids)
