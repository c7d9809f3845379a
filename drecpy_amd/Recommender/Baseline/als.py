"""ALS: weighted matrix factorisation for implicit feedback trained by alternating least squares (Hu, Koren, Volinsky: "Collaborative
Filtering for Implicit Feedback Datasets", ICDM 2008) on the MI355X engine — the pointwise, whole-matrix baseline the CDAE paper calls
"MF".  The reference has no such model; the definition of record is tests/als_oracle.py, the arithmetic csrc/drx_als.hip behind
include/drx.h ("ALS / WMF").

    frame    an entry (u, i, r) of the bound dataset with r >= interaction_threshold (every entry without a threshold) is a positive:
             preference 1, confidence 1 + alpha r.  Every other cell of the n_users x n_items matrix has preference 0, confidence 1.
    loss     L = sum over ALL cells of c (p - x_u . y_i)^2 + reg_rate (|X|^2 + |Y|^2)
    epoch    one sweep: every x_u solved exactly with Y fixed, then every y_i with the new X fixed.  The logged loss is L after it.
    score    x(u, i) = X[u] . Y[i]                             (`_predict` returns it as it is: a ranking score, not a rating)

fit() accepts batch_size, learning_rate and neg_ratio and ignores them: a sweep has no batch, no step size and no sampled negatives.
It refuses optimizer=, a process group, factors outside 1..128, reg_rate <= 0, alpha < 0, a negative weight and a frame without a
positive.  Prediction and serving run through the fused hooks of RecommenderABC on the engine's DRX_REC_BIAS scorer (zero bias);
rank() / ranking_evaluation select on a score matrix (drx_rows_dot + drx_topk): FactorServing's (_base.py).  Single GPU only.
"""
import numpy as np

from ._base import FactorServing


class ALS(FactorServing):
    MAX_FACTORS = 128

    def __init__(self, factors=64, alpha=40.0, init_std=0.01, device='cuda:0', **kwds):
        super().__init__(**kwds)
        self.factors = factors
        self.alpha = alpha
        self.init_std = init_std
        self.device = device

    # ---- fit -----------------------------------------------------------------------------------------------------------------------
    def _frame(self):
        """((indptr, indices), weights) of the positives, user-major and item-major"""
        out = []
        for transpose in (False, True):
            indptr, cols, vals = self.interaction_dataset.interaction_csr(transpose=transpose)
            vals = np.asarray(vals, dtype=np.float64)
            thr = self.interaction_threshold
            keep = np.ones(len(vals), bool) if thr is None else (vals >= thr)
            rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))[keep]
            ip = np.zeros(len(indptr), dtype=np.int64)
            ip[1:] = np.cumsum(np.bincount(rows, minlength=len(indptr) - 1))
            out.append(((ip, np.asarray(cols)[keep].astype(np.int32)), float(self.alpha) * vals[keep]))
        return out

    def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            raise Exception('ALS.fit under a torch.distributed process group: ALS trains on a single GPU only.')
        if kwds.get('optimizer') is not None:
            raise Exception('ALS.fit(optimizer=...): a sweep solves every row exactly; there is no gradient step an optimizer could take.')
        if not (isinstance(self.factors, (int, np.integer)) and 1 <= self.factors <= self.MAX_FACTORS):
            raise Exception(f'ALS(factors={self.factors!r}): factors must be an integer in 1..{self.MAX_FACTORS}.')
        if not (np.isfinite(reg_rate) and reg_rate > 0):
            raise Exception(f'ALS.fit(reg_rate={reg_rate!r}): reg_rate must be > 0 (it is what makes every row\'s system positive definite).')
        if not (np.isfinite(self.alpha) and self.alpha >= 0):
            raise Exception(f'ALS(alpha={self.alpha!r}): alpha must be >= 0 (confidence 1 + alpha r).')
        (csr, w), (csr_t, w_t) = self._frame()
        if len(w) == 0:
            raise Exception('ALS.fit: the dataset has no positive (no interaction >= interaction_threshold).')
        if (w < 0).any():
            raise Exception('ALS.fit: a negative weight alpha * r (an interaction below zero among the positives): confidence must be >= 1.')
        from ...engine_als import AlsEngine
        self._engine = AlsEngine(self.n_users, self.n_items, int(self.factors), device=self.device)
        self._engine.reg = float(reg_rate)
        self._engine.set_frame(csr, csr_t, w, w_t)
        weights = kwds.get('initial_weights')
        if weights is None:
            rng = np.random.default_rng(self.seed)
            weights = {'X': rng.normal(0.0, self.init_std, size=(self.n_users, self.factors)),
                       'Y': rng.normal(0.0, self.init_std, size=(self.n_items, self.factors))}
        self._engine.set_params(weights)
        self._register_trainables([self._engine.user_emb, self._engine.item_emb])

    def _restore_engine(self, params):
        """RecommenderABC.load: the engine rebuilt from the saved weights (serving needs no frame)"""
        from ...engine_als import AlsEngine
        self._engine = AlsEngine(self.n_users, self.n_items, int(self.factors), device=self.device)
        self._engine.set_params(params)

    def _fused_trainables(self):
        return [self._engine.user_emb, self._engine.item_emb]

    def _sample_batch(self, batch_size, **kwds):
        return ()

    def _do_batch(self, batch_samples, step=0, want_loss=False, **kwds):
        return self._engine.sweep(want_loss=want_loss)

    def _predict_batch(self, batch_samples, **kwds):
        raise NotImplementedError('ALS has no batch: a sweep solves every row of X, then of Y (_do_batch).')

    def _compute_batch_loss(self, predictions, desired_values, **kwds):
        raise NotImplementedError('ALS has no batch loss: the sweep returns the whole-matrix objective.')
