"""FPMC (Rendle, Freudenthaler, Schmidt-Thieme: "Factorizing Personalized Markov Chains for Next-Basket Recommendation", WWW 2010) on the
MI355X engine — the sequence-aware baseline of Caser's comparison (Tang & Wang 2018), on the windows Caser trains on.  The reference
has no such model; the definition of record is tests/fpmc_oracle.py, the arithmetic csrc/drx_fpmc.hip behind include/drx.h ("FPMC";
DESIGN.md section 3.9).

    score    x(u, S, i) = P[u] . Q[i] + mean_{l in S} M[l] . N[i] + b[i]   (`_predict(u, i)` returns x(u, S_u, i), S_u the user's basket:
             the last min(L, len) items of its sequence — a ranking score, not a rating)
    batch    batch_size windows drawn on the device by the list sampler's counter-based twin (drx_list_sample_device, n_targets = 1):
             a uniform user holding a window, a uniform window of L consecutive items + the next item as the target, and `neg_ratio`
             negatives uniform without replacement among the items the user's sequence does not hold.  Sequences follow `sort_column`
             and keep the records with interaction >= interaction_threshold.  Draw k of a fit() uses the seed `_draw_seed(k)`.
    step     loss = mean softplus(-(x(u, S, i) - x(u, S, j))); reg_rate * row added to the gradient of EVERY row of P, M, Q and N (dense,
             like the other dense steps here; the biases are not regularised); one of the dense rules of fit(optimizer=...), Adam by
             default, P registered first, then M, then [Q | N] with b.

Deviations from Rendle et al.: mini-batches under a dense rule instead of single-sample SGD; an item bias; the mean over an ordered
window of L items instead of over the previous basket; negatives from the items the user's whole sequence does not hold (the list
sampler's rule) instead of those outside the target basket; the logged loss is the data term alone.  L = 1 is the first-order chain.

Prediction and serving run through the fused hooks of RecommenderABC (recommend_batch, catalogue_ranks, predict_pairs) on the engine's
DRX_REC_BIAS scorer at rows of 2 ld floats; rank() / ranking_evaluation select on a score matrix: FactorServing's (_base.py), as the
refusals, the draw seeds and _do_batch are SampledDenseFit's.  Single GPU only.
"""
import numpy as np

from ._base import SampledDenseFit, last_items_baskets


class FPMC(SampledDenseFit):
    MODEL, NEGATIVES_PER, DENSE_UPDATE_OF = 'FPMC', 'negatives drawn per window', 'every factor table'
    MAX_FACTORS = 128
    MAX_L = 8
    MAX_NEG_RATIO = 16

    def __init__(self, factors=64, L=1, init_std=0.01, sort_column='timestamp', device='cuda:0', **kwds):
        super().__init__(**kwds)
        self.factors = factors
        self.L = L
        self.init_std = init_std
        self.sort_column = sort_column
        self.device = device

    # ---- fit -----------------------------------------------------------------------------------------------------------------------
    def _check_shape(self):
        if not (isinstance(self.factors, (int, np.integer)) and 1 <= self.factors <= self.MAX_FACTORS):
            raise Exception(f'FPMC(factors={self.factors!r}): factors must be an integer in 1..{self.MAX_FACTORS}.')
        if not (isinstance(self.L, (int, np.integer)) and 1 <= self.L <= self.MAX_L):
            raise Exception(f'FPMC(L={self.L!r}): L must be an integer in 1..{self.MAX_L}.')

    def _list_sampler(self, neg_ratio):
        """the window stream of Caser._pre_fit at n_targets = 1 (its MT19937 stream is not used: the seed only has to be an integer)"""
        from ...Sampler import ListSampler
        return ListSampler(self.interaction_dataset, ['uid'], neg_ratio=neg_ratio, n_targets=1,
                           interaction_threshold=self.interaction_threshold, negative_ids_col='iid', min_positive_records=int(self.L),
                           max_positive_records=int(self.L), sort_column=self.sort_column,
                           seed=int(self.seed) if self.seed is not None else 0)

    def _baskets(self, sampler):
        """[n_users, L] int32, -1 = absent: the last min(L, len) ids of every user's sequence as the sampler orders and thresholds it"""
        return last_items_baskets(sampler, self.n_users, self.L)

    def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
        self._start_sampled_fit(neg_ratio)
        self._check_shape()
        from ...engine_fpmc import FpmcEngine
        self._sampler = self._list_sampler(self._neg_ratio)
        if getattr(self._sampler, '_native', None) is None:
            raise Exception('FPMC.fit: the dataset holds no sequence to draw windows from (Failed to sample group records).')
        self._sampler.device_twin(self.device)         # (raises the sampler's message where no user holds a window)
        self._engine = FpmcEngine(self.n_users, self.n_items, int(self.factors), int(self.L), device=self.device)
        self._engine.lr, self._engine.reg = float(learning_rate), float(reg_rate)
        self._engine.set_baskets(self._baskets(self._sampler))
        weights = kwds.get('initial_weights')
        if weights is None:
            rng = np.random.default_rng(self.seed)
            draw = lambda n: rng.normal(0.0, self.init_std, size=(n, self.factors))
            weights = {'P': draw(self.n_users), 'Q': draw(self.n_items), 'M': draw(self.n_items), 'N': draw(self.n_items),
                       'b': np.zeros(self.n_items)}
        self._engine.set_params(weights)
        self._register_trainables(self._fused_trainables())

    def _restore_engine(self, params):
        """RecommenderABC.load: the engine rebuilt from the saved weights, the baskets from the bound dataset (no window is drawn)"""
        from ...engine_fpmc import FpmcEngine
        self._engine = FpmcEngine(self.n_users, self.n_items, int(self.factors), int(self.L), device=self.device)
        self._engine.set_params(params)
        self._engine.set_baskets(self._baskets(self._list_sampler(getattr(self, '_neg_ratio', 1))))

    def _fused_trainables(self):
        e = self._engine
        return [e.user_emb, e.trans_emb, e.item_emb]

    def _sample_batch(self, batch_size, **kwds):
        seed = self._next_draw_seed()
        with self._device_lock:
            return self._sampler.sample_device(int(batch_size), seed)

    def _predict_batch(self, batch_samples, **kwds):
        """x(u, S, i) - x(u, S, j) of the batch's windows (numpy float64 [B r]) against the target 1 — the reference's training hook,
        kept for callers, never on the training path (the fused step computes its loss itself): the definition on the host, from a
        copy of the parameters."""
        as_np = lambda a: a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)
        uid, before, after = (as_np(a).astype(np.int64) for a in batch_samples[:3])
        with self._device_lock:
            p = {k: v.astype(np.float64) for k, v in self._engine.get_params().items()}
        c = np.concatenate([p['P'][uid], p['M'][before].mean(axis=1)], axis=1)
        x = np.einsum('wf,wjf->wj', c, np.concatenate([p['Q'], p['N']], axis=1)[after]) + p['b'][after]
        d = (x[:, :1] - x[:, 1:]).reshape(-1)
        return d, np.ones(len(d))
