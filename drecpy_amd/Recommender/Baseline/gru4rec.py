"""GRU4Rec (Hidasi, Karatzoglou, Baltrunas, Tikk: "Session-based Recommendations with Recurrent Neural Networks", ICLR 2016) on the
MI355X engine — the recurrent baseline of Caser's comparison (Tang & Wang 2018), on the windows Caser and FPMC train on.  The reference
has no such model; the definition of record is tests/gru_oracle.py, the arithmetic csrc/drx_gru.hip behind include/drx.h ("GRU4Rec";
DESIGN.md section 3.11).

    cell     h_0 = 0, x_t = E[s_t];  z_t = sigmoid(x_t Wx_z + h_{t-1} Wh_z + bx_z);  r_t = sigmoid(x_t Wx_r + h_{t-1} Wh_r + bx_r);
             n_t = tanh(x_t Wx_n + bx_n + r_t (.) (h_{t-1} Wh_n + bhn));  h_t = (1 - z_t) (.) n_t + z_t (.) h_{t-1}   (torch's GRU cell)
    score    x(S, i) = h_L(S) . Q[i] + b[i]   (`_predict(u, i)` returns x(S_u, i), S_u the user's basket: the last min(L, len) items of
             its sequence; a shorter basket runs only its own steps, an empty one scores b[i] — a ranking score, not a rating).
             There is no user table: the user's sequence is the session.
    batch    batch_size windows drawn on the device by the list sampler's counter-based twin (drx_list_sample_device, n_targets = 1):
             a uniform user holding a window, a uniform window of L consecutive items + the next item as the target, and `neg_ratio`
             negatives uniform without replacement among the items the user's sequence does not hold.  Sequences follow `sort_column`
             and keep the records with interaction >= interaction_threshold.  Draw k of a fit() uses the seed `_draw_seed(k)`.
    step     loss = mean softplus(-(x(S, i) - x(S, j))); reg_rate * value added to the gradient of EVERY row of E and Q and every
             entry of Wx and Wh (dense; the biases bx, bhn, b are not regularised); one of the dense rules of fit(optimizer=...), Adam
             by default, E registered first, then the small weights (Wx, Wh, bx, bhn), then Q with b.
    weights  initial_weights(): from np.random.default_rng(seed), in this order: E ~ N(0, init_std) [n_items, factors],
             Wx ~ U(-1/sqrt(hidden), 1/sqrt(hidden)) [factors, 3 hidden], Wh the same [hidden, 3 hidden], Q ~ N(0, init_std)
             [n_items, hidden]; the biases are zero.  Gate columns: z | r | n.

Deviations from Hidasi et al.: fixed windows of L items instead of session-parallel mini-batches; sampled negatives (the list
sampler's rule: items the user's sequence does not hold) instead of the other sessions' items of the batch; the BPR loss only, no
TOP1; one layer; an input embedding instead of the one-hot item vector; an item bias; the logged loss is the data term alone.

Prediction and serving run through the fused hooks of RecommenderABC (recommend_batch, catalogue_ranks, predict_pairs) on the engine's
DRX_REC_BIAS scorer at rows of `hidden` floats; rank() / ranking_evaluation select on a score matrix: FactorServing's (_base.py), as the
refusals, the draw seeds and _do_batch are SampledDenseFit's.  Single GPU only.
"""
import numpy as np

from ._base import SampledDenseFit, last_items_baskets


class GRU4Rec(SampledDenseFit):
    """GRU4Rec(factors=64, hidden=64, L=5, init_std=0.01, sort_column='timestamp', device='cuda:0'): one GRU layer over the input
    embeddings of the L items before the target, score h_L . Q[i] + b[i]; 1 <= factors, hidden <= 64, 1 <= L <= 8, 1 <= neg_ratio <= 16,
    single GPU.

    Deviations from Hidasi et al. 2016: fixed windows of L items instead of session-parallel mini-batches; sampled negatives (the list
    sampler's rule: items the user's sequence does not hold) instead of the in-batch ones; the BPR loss only, no TOP1; one layer; an
    input embedding instead of the one-hot item vector; an item bias."""
    MODEL, NEGATIVES_PER, DENSE_UPDATE_OF = 'GRU4Rec', 'negatives drawn per window', 'both item tables and the gate weights'
    MAX_FACTORS = 64
    MAX_HIDDEN = 64
    MAX_L = 8
    MAX_NEG_RATIO = 16

    def __init__(self, factors=64, hidden=64, L=5, init_std=0.01, sort_column='timestamp', device='cuda:0', **kwds):
        super().__init__(**kwds)
        self.factors = factors
        self.hidden = hidden
        self.L = L
        self.init_std = init_std
        self.sort_column = sort_column
        self.device = device

    # ---- fit -----------------------------------------------------------------------------------------------------------------------
    def _check_shape(self):
        integer = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, bool)
        if not (integer(self.factors) and 1 <= self.factors <= self.MAX_FACTORS):
            raise Exception(f'GRU4Rec(factors={self.factors!r}): factors must be an integer in 1..{self.MAX_FACTORS}.')
        if not (integer(self.hidden) and 1 <= self.hidden <= self.MAX_HIDDEN):
            raise Exception(f'GRU4Rec(hidden={self.hidden!r}): hidden must be an integer in 1..{self.MAX_HIDDEN}.')
        if not (integer(self.L) and 1 <= self.L <= self.MAX_L):
            raise Exception(f'GRU4Rec(L={self.L!r}): L must be an integer in 1..{self.MAX_L}.')

    def _list_sampler(self, neg_ratio):
        """the window stream of Caser._pre_fit at n_targets = 1 (its MT19937 stream is not used: the seed only has to be an integer)"""
        from ...Sampler import ListSampler
        return ListSampler(self.interaction_dataset, ['uid'], neg_ratio=neg_ratio, n_targets=1,
                           interaction_threshold=self.interaction_threshold, negative_ids_col='iid', min_positive_records=int(self.L),
                           max_positive_records=int(self.L), sort_column=self.sort_column,
                           seed=int(self.seed) if self.seed is not None else 0)

    def _baskets(self, sampler):
        """[n_users, L] int32, -1 = absent: the last min(L, len) ids of every user's sequence (FPMC's baskets: _base.last_items_baskets)"""
        return last_items_baskets(sampler, self.n_users, self.L)

    def initial_weights(self):
        """the seven arrays of a fresh model, drawn in the order of the module docstring"""
        K, H, N = int(self.factors), int(self.hidden), int(self.n_items)
        rng = np.random.default_rng(self.seed)
        bound = 1.0 / np.sqrt(H)
        E = rng.normal(0.0, self.init_std, size=(N, K))
        Wx = rng.uniform(-bound, bound, size=(K, 3 * H))
        Wh = rng.uniform(-bound, bound, size=(H, 3 * H))
        Q = rng.normal(0.0, self.init_std, size=(N, H))
        return {'E': E, 'Wx': Wx, 'Wh': Wh, 'bx': np.zeros(3 * H), 'bhn': np.zeros(H), 'Q': Q, 'b': np.zeros(N)}

    def _new_engine(self):
        from ...engine_gru import GruEngine
        return GruEngine(self.n_users, self.n_items, int(self.factors), int(self.hidden), int(self.L), device=self.device)

    def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
        self._start_sampled_fit(neg_ratio)
        self._check_shape()
        self._sampler = self._list_sampler(self._neg_ratio)
        if getattr(self._sampler, '_native', None) is None:
            raise Exception('GRU4Rec.fit: the dataset holds no sequence to draw windows from (Failed to sample group records).')
        self._sampler.device_twin(self.device)         # (raises the sampler's message where no user holds a window)
        self._engine = self._new_engine()
        self._engine.lr, self._engine.reg = float(learning_rate), float(reg_rate)
        self._engine.set_baskets(self._baskets(self._sampler))
        weights = kwds.get('initial_weights')
        self._engine.set_params(weights if weights is not None else self.initial_weights())
        self._register_trainables(self._fused_trainables())

    def _restore_engine(self, params):
        """RecommenderABC.load: the engine rebuilt from the saved weights, the baskets from the bound dataset (no window is drawn)"""
        self._engine = self._new_engine()
        self._engine.set_params(params)
        self._engine.set_baskets(self._baskets(self._list_sampler(getattr(self, '_neg_ratio', 1))))

    def _fused_trainables(self):
        e = self._engine
        return [e.input_emb, e.small, e.item_emb]

    def _sample_batch(self, batch_size, **kwds):
        seed = self._next_draw_seed()
        with self._device_lock:
            return self._sampler.sample_device(int(batch_size), seed)

    def _predict_batch(self, batch_samples, **kwds):
        """x(S, i) - x(S, j) of the batch's windows (numpy float64 [B r]) against the target 1 — the reference's training hook, kept
        for callers, never on the training path (the fused step computes its loss itself): the definition on the host, from a copy
        of the parameters."""
        as_np = lambda a: a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)
        _, before, after = (as_np(a).astype(np.int64) for a in batch_samples[:3])
        with self._device_lock:
            p = {k: v.astype(np.float64) for k, v in self._engine.get_params().items()}
        H = p['Wh'].shape[0]
        sig = lambda a: 1.0 / (1.0 + np.exp(-a))
        h = np.zeros((len(before), H))
        for t in range(before.shape[1]):
            px, ph = p['E'][before[:, t]] @ p['Wx'] + p['bx'], h @ p['Wh']
            z, r = sig(px[:, :H] + ph[:, :H]), sig(px[:, H:2 * H] + ph[:, H:2 * H])
            n = np.tanh(px[:, 2 * H:] + r * (ph[:, 2 * H:] + p['bhn']))
            h = (1.0 - z) * n + z * h
        x = np.einsum('wh,wjh->wj', h, p['Q'][after]) + p['b'][after]
        d = (x[:, :1] - x[:, 1:]).reshape(-1)
        return d, np.ones(len(d))
