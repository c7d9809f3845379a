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
DRX_REC_BIAS scorer; rank() / ranking_evaluation select on a score matrix (drx_rows_dot + drx_topk): FactorServing's (_base.py), as the
refusals, the draw seeds and _do_batch are SampledDenseFit's.  Single GPU only.
"""
import numpy as np

from ._base import SampledDenseFit


class BPR(SampledDenseFit):
    MAX_FACTORS = 256
    MODEL, NEGATIVES_PER, DENSE_UPDATE_OF = 'BPR', 'negatives drawn per positive pair', 'both factor tables'

    def __init__(self, factors=64, init_std=0.01, device='cuda:0', **kwds):
        super().__init__(**kwds)
        self.factors = factors
        self.init_std = init_std
        self.device = device

    # ---- fit -----------------------------------------------------------------------------------------------------------------------
    def _check_factors(self):
        if not (isinstance(self.factors, (int, np.integer)) and 1 <= self.factors <= self.MAX_FACTORS):
            raise Exception(f'BPR(factors={self.factors!r}): factors must be an integer in 1..{self.MAX_FACTORS}.')

    def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
        self._start_sampled_fit(neg_ratio)
        self._check_factors()
        positives, recorded, eligible = self._positives_frame()
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
        self._register_trainables(self._fused_trainables())

    def _restore_engine(self, params):
        """RecommenderABC.load: the engine rebuilt from the saved weights (serving needs no sampler frame)"""
        from ...engine_bpr import BprEngine
        self._engine = BprEngine(self.n_users, self.n_items, int(self.factors), device=self.device)
        self._engine.set_params(params)

    def _fused_trainables(self):
        return [self._engine.user_emb, self._engine.item_emb]

    def _sample_batch(self, batch_size, **kwds):
        seed = self._next_draw_seed()
        with self._device_lock:
            return self._engine.sample(batch_size, self._neg_ratio, seed)

    def _predict_batch(self, batch_samples, **kwds):
        """x(u, i) - x(u, j) of the batch's triples (numpy float64 [T]) against the target 1 — the reference's training hook, kept for
        callers; the fused step computes its loss itself."""
        u, i, j = batch_samples[:3]
        with self._device_lock:
            xi, xj = self._engine.pair_scores(u, i).cpu().numpy(), self._engine.pair_scores(u, j).cpu().numpy()
        return xi.astype(np.float64) - xj.astype(np.float64), np.ones(len(xi))
