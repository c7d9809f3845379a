"""SASRec (Kang & McAuley: "Self-Attentive Sequential Recommendation", ICDM 2018) on the MI355X engine — the self-attention model
that superseded Caser, GRU4Rec and FPMC, on the windows they train on.  The reference has no such model; the definition of record is
tests/sasrec_oracle.py, the arithmetic csrc/drx_sas.hip behind include/drx.h ("SASRec").

    forward  a sequence of m <= L items occupies the positions L - m .. L - 1; X0_t = E[s_t] + Pos[t]; per block (one head):
             A = LN(X; ln1), q, k, v = A Wq, A Wk, A Wv, S_tj = q_t . k_j / sqrt(hidden) for present j <= t, P = softmax_j(S),
             X' = X + P v, F = LN(X'; ln2), X'' = X' + relu(F W1 + b1) W2 + b2;  h = LN(X_{L-1}; lnf) after the last block;
             LN(x) = (x - mean) / sqrt(var + 1e-5) g + beta with the biased variance over the hidden columns
    score    x(S, i) = h(S) . Q[i] + b[i]   (`_predict(u, i)` returns x(S_u, i), S_u the user's basket: the last min(L, len) items of
             its sequence; an empty one gives h = 0 and scores b[i] — a ranking score, not a rating).  There is no user table.
    batch    batch_size windows drawn on the device by the list sampler's counter-based twin (drx_list_sample_device, n_targets = 1):
             a uniform user holding a window, a uniform window of L consecutive items + the next item as the target, and `neg_ratio`
             negatives uniform without replacement among the items the user's sequence does not hold.  Sequences follow `sort_column`
             and keep the records with interaction >= interaction_threshold.  Draw k of a fit() uses the seed `_draw_seed(k)`.
    step     loss = mean softplus(-(x(S, i) - x(S, j))) at the last position; reg_rate * value added to the gradient of EVERY row of E
             and Q and every entry of Pos and of the five matrices of every block (dense; the biases, the LN gains and offsets and b
             are not regularised); one of the dense rules of fit(optimizer=...), Adam by default, E registered first, then the small
             weights, then Q with b.
    weights  initial_weights(): from np.random.default_rng(seed), in this order: E ~ N(0, init_std) [n_items, hidden], Pos ~ N(0,
             init_std) [L, hidden], per block Wq, Wk, Wv, W1, W2 ~ U(-1/sqrt(hidden), 1/sqrt(hidden)) [hidden, hidden], Q ~ N(0, init_std)
             [n_items, hidden]; the LN gains are one, the offsets and biases zero.

Deviations from Kang & McAuley: fixed windows of L <= 16 items instead of the whole sequence cut to n; the loss at the last position
only, against `neg_ratio` sampled negatives, instead of one negative at every position; a separate output table Q with an item bias
instead of the shared item embedding; no dropout; one head; the pairwise softplus loss instead of the binary cross-entropy; no
sqrt(d) scaling of the embeddings; LN epsilon 1e-5; the logged loss is the data term alone.

Prediction and serving run through the fused hooks of RecommenderABC (recommend_batch, catalogue_ranks, predict_pairs) on the engine's
DRX_REC_BIAS scorer at rows of `hidden` floats; rank() / ranking_evaluation select on a score matrix: FactorServing's (_base.py), as the
refusals, the draw seeds and _do_batch are SampledDenseFit's.  Single GPU only.
"""
import numpy as np

from ._base import SampledDenseFit, last_items_baskets

_MATRICES = ('Wq', 'Wk', 'Wv', 'W1', 'W2')
_VECTORS = ('b1', 'b2', 'ln1_g', 'ln1_b', 'ln2_g', 'ln2_b')


class SASRec(SampledDenseFit):
    """SASRec(hidden=64, L=10, blocks=2, init_std=0.01, sort_column='timestamp', device='cuda:0'): `blocks` one-head self-attention
    blocks over the input embeddings plus learned positions of the L items before the target, score h . Q[i] + b[i]; 1 <= hidden <= 64,
    1 <= L <= 16, blocks 1 or 2, 1 <= neg_ratio <= 16, single GPU.

    Deviations from Kang & McAuley 2018: fixed windows of L <= 16 items instead of the whole sequence cut to n; the loss at the last
    position only, against `neg_ratio` sampled negatives, instead of one negative at every position; a separate output table Q with an
    item bias instead of the shared item embedding; no dropout; one head; the pairwise softplus loss instead of BCE; no sqrt(d)
    scaling of the embeddings; LN epsilon 1e-5."""
    MODEL, NEGATIVES_PER, DENSE_UPDATE_OF = 'SASRec', 'negatives drawn per window', 'both item tables and the attention weights'
    MAX_HIDDEN = 64
    MAX_L = 16
    MAX_BLOCKS = 2
    MAX_NEG_RATIO = 16

    def __init__(self, hidden=64, L=10, blocks=2, init_std=0.01, sort_column='timestamp', device='cuda:0', **kwds):
        super().__init__(**kwds)
        self.hidden = hidden
        self.L = L
        self.blocks = blocks
        self.init_std = init_std
        self.sort_column = sort_column
        self.device = device

    # ---- fit -----------------------------------------------------------------------------------------------------------------------
    def _check_shape(self):
        integer = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, bool)
        if not (integer(self.hidden) and 1 <= self.hidden <= self.MAX_HIDDEN):
            raise Exception(f'SASRec(hidden={self.hidden!r}): hidden must be an integer in 1..{self.MAX_HIDDEN}.')
        if not (integer(self.L) and 1 <= self.L <= self.MAX_L):
            raise Exception(f'SASRec(L={self.L!r}): L must be an integer in 1..{self.MAX_L}.')
        if not (integer(self.blocks) and 1 <= self.blocks <= self.MAX_BLOCKS):
            raise Exception(f'SASRec(blocks={self.blocks!r}): blocks must be an integer in 1..{self.MAX_BLOCKS}.')

    def _list_sampler(self, neg_ratio):
        """the window stream of Caser._pre_fit at n_targets = 1 (its MT19937 stream is not used: the seed only has to be an integer)"""
        from ...Sampler import ListSampler
        return ListSampler(self.interaction_dataset, ['uid'], neg_ratio=neg_ratio, n_targets=1,
                           interaction_threshold=self.interaction_threshold, negative_ids_col='iid', min_positive_records=int(self.L),
                           max_positive_records=int(self.L), sort_column=self.sort_column,
                           seed=int(self.seed) if self.seed is not None else 0)

    def _baskets(self, sampler):
        """[n_users, L] int32, left-aligned, -1 = absent: the last min(L, len) ids of every user's sequence (_base.last_items_baskets)"""
        return last_items_baskets(sampler, self.n_users, self.L)

    def initial_weights(self):
        """the arrays of a fresh model, drawn in the order of the module docstring"""
        H, L, N = int(self.hidden), int(self.L), int(self.n_items)
        rng = np.random.default_rng(self.seed)
        bound = 1.0 / np.sqrt(H)
        w = {'E': rng.normal(0.0, self.init_std, size=(N, H)), 'Pos': rng.normal(0.0, self.init_std, size=(L, H))}
        for b in range(int(self.blocks)):
            for m in _MATRICES:
                w[f'{m}{b}'] = rng.uniform(-bound, bound, size=(H, H))
        for b in range(int(self.blocks)):
            for v in _VECTORS:
                w[f'{v}{b}'] = np.ones(H) if v.endswith('_g') else np.zeros(H)
        w.update({'lnf_g': np.ones(H), 'lnf_b': np.zeros(H), 'Q': rng.normal(0.0, self.init_std, size=(N, H)), 'b': np.zeros(N)})
        return w

    def _new_engine(self):
        from ...engine_sas import SasEngine
        return SasEngine(self.n_users, self.n_items, int(self.hidden), int(self.L), int(self.blocks), device=self.device)

    def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
        self._start_sampled_fit(neg_ratio)
        self._check_shape()
        self._sampler = self._list_sampler(self._neg_ratio)
        if getattr(self._sampler, '_native', None) is None:
            raise Exception('SASRec.fit: the dataset holds no sequence to draw windows from (Failed to sample group records).')
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
        """x(S, i) - x(S, j) of the batch's (full) windows (numpy float64 [B r]) against the target 1 — the reference's training hook,
        kept for callers, never on the training path (the fused step computes its loss itself): the definition on the host, from a
        copy of the parameters."""
        as_np = lambda a: a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)
        _, before, after = (as_np(a).astype(np.int64) for a in batch_samples[:3])
        with self._device_lock:
            p = {k: v.astype(np.float64) for k, v in self._engine.get_params().items()}
        L, H = p['Pos'].shape

        def ln(x, g, beta):
            xc = x - x.mean(axis=-1, keepdims=True)
            return xc / np.sqrt((xc * xc).mean(axis=-1, keepdims=True) + 1e-5) * g + beta

        x = p['E'][before] + p['Pos'][None]
        causal = np.tril(np.ones((L, L), bool))[None]
        for b in range(int(self.blocks)):
            a = ln(x, p[f'ln1_g{b}'], p[f'ln1_b{b}'])
            s = np.where(causal, np.einsum('bth,bjh->btj', a @ p[f'Wq{b}'], a @ p[f'Wk{b}']) / np.sqrt(H), -np.inf)
            e = np.exp(s - s.max(axis=2, keepdims=True))
            x = x + np.einsum('btj,bjh->bth', e / e.sum(axis=2, keepdims=True), a @ p[f'Wv{b}'])
            f = ln(x, p[f'ln2_g{b}'], p[f'ln2_b{b}'])
            x = x + np.maximum(f @ p[f'W1{b}'] + p[f'b1{b}'], 0.0) @ p[f'W2{b}'] + p[f'b2{b}']
        h = ln(x[:, L - 1], p['lnf_g'], p['lnf_b'])
        sc = np.einsum('wh,wjh->wj', h, p['Q'][after]) + p['b'][after]
        d = (sc[:, :1] - sc[:, 1:]).reshape(-1)
        return d, np.ones(len(d))
