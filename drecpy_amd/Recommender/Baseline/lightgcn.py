"""LightGCN (He, Deng, Wang, Li, Zhang, Wang: "LightGCN: Simplifying and Powering Graph Convolution Network for Recommendation", SIGIR
2020) on the MI355X engine — the graph-convolution successor of BPR-MF and NeuMF.  The reference has no such model; the definition of
record is tests/lgcn_oracle.py, the arithmetic csrc/drx_lgcn.hip behind include/drx.h ("LightGCN").

    nodes    the users, then the items; E0 = [P ; Q]
    graph    the bipartite graph of the positives of the bound dataset (interaction >= interaction_threshold, the frame the sampler
             draws from, duplicates merged); A[r, c] = (deg r deg c)^(-1/2) on every edge
    final    Ebar = (1 / (layers + 1)) sum_{l = 0 .. layers} A^l E0; a node without edges keeps E0 / (layers + 1)
    score    x(u, i) = Ebar[u] . Ebar[n_users + i], no bias          (`_predict` returns it as it is: a ranking score, not a rating)
    batch    BPR's: batch_size (user, positive, negative) triples from drx_bpr_sample with the seed `_draw_seed(k)`, neg_ratio >= 1
             negatives per drawn pair
    step     loss = mean softplus(-(x(u, i) - x(u, j))); reg_rate * row added to the gradient of EVERY row of E0 — the project's dense
             regularisation, NOT the paper's term over the rows a batch names —; one of the dense rules of fit(optimizer=...), Adam by
             default, P registered first, then Q.  Every step propagates over the whole graph, `layers` times forward and backward.

No edge or message dropout, uniform layer weights, at most 4 layers, factors <= 256, fp32 rows.  Prediction and serving run through the
fused hooks of RecommenderABC on the engine's DRX_REC_BIAS scorer over the cached final embeddings: FactorServing's (_base.py), as the
refusals, the draw seeds and _do_batch are SampledDenseFit's.  Single GPU only.
"""
import numpy as np

from ._base import SampledDenseFit


class LightGCN(SampledDenseFit):
    MAX_FACTORS, MAX_LAYERS = 256, 4
    MODEL, NEGATIVES_PER, DENSE_UPDATE_OF = 'LightGCN', 'negatives drawn per positive pair', 'the embedding table'

    def __init__(self, factors=64, layers=3, init_std=0.01, device='cuda:0', **kwds):
        super().__init__(**kwds)
        self.factors = factors
        self.layers = layers
        self.init_std = init_std
        self.device = device

    # ---- fit -----------------------------------------------------------------------------------------------------------------------
    def _check_shape(self):
        if not (isinstance(self.factors, (int, np.integer)) and 1 <= self.factors <= self.MAX_FACTORS):
            raise Exception(f'LightGCN(factors={self.factors!r}): factors must be an integer in 1..{self.MAX_FACTORS}.')
        if not (isinstance(self.layers, (int, np.integer)) and 0 <= self.layers <= self.MAX_LAYERS):
            raise Exception(f'LightGCN(layers={self.layers!r}): layers must be an integer in 0..{self.MAX_LAYERS}.')

    def _new_engine(self, positives):
        from ...engine_lgcn import LgcnEngine
        self._engine = LgcnEngine(self.n_users, self.n_items, int(self.factors), int(self.layers), device=self.device)
        self._engine.set_graph(positives)

    def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
        self._start_sampled_fit(neg_ratio)
        self._check_shape()
        positives, recorded, eligible = self._positives_frame()
        if len(eligible) == 0:
            raise Exception('LightGCN.fit: the dataset has no eligible user (one with an interaction >= interaction_threshold and at '
                            'least one item it has no interaction with).')
        self._new_engine(positives)
        self._engine.lr, self._engine.reg = float(learning_rate), float(reg_rate)
        self._engine.set_sampler_frame(positives, recorded, eligible)
        weights = kwds.get('initial_weights')
        if weights is None:
            rng = np.random.default_rng(self.seed)
            weights = {'P': rng.normal(0.0, self.init_std, size=(self.n_users, self.factors)),
                       'Q': rng.normal(0.0, self.init_std, size=(self.n_items, self.factors))}
        self._engine.set_params(weights)
        self._register_trainables(self._fused_trainables())

    def _restore_engine(self, params):
        """RecommenderABC.load: the engine rebuilt from the saved weights, the graph from the pickled dataset's positives"""
        self._new_engine(self._positives_frame()[0])
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
