"""NeuMF (He, Liao, Zhang, Nie, Hu, Chua: "Neural Collaborative Filtering", WWW 2017) on the MI355X engine — the neural baseline the DMF
paper (Xue et al., IJCAI 2017) reports against.  The reference has no such model; the definition of record is tests/ncf_oracle.py, the
arithmetic csrc/drx_ncf.hip behind include/drx.h ("NeuMF").

    logit    x(u, i) = sum_k hg[k] Pg[u, k] Qg[i, k] + hm . a_n + b0,  a_0 = [Pm[u] ; Qm[i]],  a_l = relu(W_l^T a_{l-1} + b_l)
    batch    batch_size point samples (user, item, y) drawn on the device by the counter-based point sampler
             (drx_point_sample_recorded): positives are the interactions >= interaction_threshold (y = 1), negatives pairs the frame
             does not record (y = 0), a negative with probability neg_ratio / (neg_ratio + 1).  Draw k of a fit() uses `_draw_seed(k)`.
    step     loss = mean BCE from the logit; reg_rate * w added to the gradient of EVERY row of both tables, every kernel W_l and h
             (dense, like the other dense steps here; the biases b_l and b0 are not regularised); one of the dense rules of
             fit(optimizer=...), Adam by default; registered: the user table, the item table, the small weights.
    values   the device ranks on LOGITS; predict / predict_pairs / recommend / recommend_batch / rank / catalogue_ranks report
             1 / (1 + exp(-x)) of the fp32 logit, computed in float64 at this boundary: a saturated sigmoid never creates ties in
             the order.  interaction_threshold compares these probabilities.

Every ranking call goes through the score matrix (drx_ncf_half_rows + drx_ncf_score_rows, then drx_topk).  Single GPU only.
"""
import numpy as np

from ._base import SampledDenseFit


def _sigmoid(x):
    """1 / (1 + exp(-x)) in float64, -inf -> -inf kept as the mark of a missing entry"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over='ignore'):
        return np.where(np.isneginf(x), -np.inf, 1.0 / (1.0 + np.exp(-x)))


class NeuMF(SampledDenseFit):
    MODEL, NEGATIVES_PER, DENSE_UPDATE_OF = 'NeuMF', 'negatives drawn per positive, on average', 'both tables and the small weights'
    _reported_value = staticmethod(_sigmoid)
    MATRIX_BUDGET_BYTES = 1 << 30          # the score matrix of one chunk of recommend_batch / catalogue_ranks

    def __init__(self, factors=8, mlp_factors=32, layers=(32, 16, 8), init_std=0.01, device='cuda:0', **kwds):
        super().__init__(**kwds)
        self.factors = factors
        self.mlp_factors = mlp_factors
        self.layers = layers
        self.init_std = init_std
        self.device = device

    # ---- fit -----------------------------------------------------------------------------------------------------------------------
    def _check_shape(self):
        from ...engine_ncf import check_shape
        try:
            return check_shape(self.factors, self.mlp_factors, self.layers, who='NeuMF')
        except Exception as e:
            raise Exception(str(e)) from None

    def _init_weights(self, Kg, Km, layers):
        rng = np.random.default_rng(self.seed)
        w = {'Pg': rng.normal(0.0, self.init_std, size=(self.n_users, Kg)), 'Pm': rng.normal(0.0, self.init_std, size=(self.n_users, Km)),
             'Qg': rng.normal(0.0, self.init_std, size=(self.n_items, Kg)), 'Qm': rng.normal(0.0, self.init_std, size=(self.n_items, Km))}
        fin = 2 * Km
        for l, fo in enumerate(layers, 1):
            lim = np.sqrt(6.0 / (fin + fo))                      # Glorot-uniform
            w[f'W{l}'], w[f'b{l}'] = rng.uniform(-lim, lim, size=(fin, fo)), np.zeros(fo)
            fin = fo
        lim = np.sqrt(3.0 / (Kg + fin))
        w['hg'], w['hm'], w['b0'] = rng.uniform(-lim, lim, size=Kg), rng.uniform(-lim, lim, size=fin), np.zeros(1)
        return w

    def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
        self._start_sampled_fit(neg_ratio)
        Kg, Km, layers = self._check_shape()
        positives, recorded, _ = self._positives_frame()
        if len(positives[1]) == 0:
            raise Exception('NeuMF.fit: the dataset has no positive (no interaction >= interaction_threshold).')
        if not (np.diff(self.interaction_dataset.interaction_csr()[0]) < self.n_items).any():
            raise Exception('NeuMF.fit: no user has an unrecorded item (no negative can be drawn).')
        from ...engine_ncf import NcfEngine
        self._engine = NcfEngine(self.n_users, self.n_items, Kg, Km, layers, device=self.device)
        self._engine.lr, self._engine.reg = float(learning_rate), float(reg_rate)
        self._engine.set_sampler_frame(positives, recorded)
        weights = kwds.get('initial_weights')
        self._engine.set_params(weights if weights is not None else self._init_weights(Kg, Km, layers))
        self._register_trainables(self._fused_trainables())

    def _restore_engine(self, params):
        """RecommenderABC.load: the engine rebuilt from the saved weights (serving needs no sampler frame)"""
        from ...engine_ncf import NcfEngine
        self._engine = NcfEngine(self.n_users, self.n_items, *self._check_shape(), device=self.device)
        self._engine.set_params(params)

    def _fused_trainables(self):
        e = self._engine
        return [e.user_emb, e.item_emb, e.small]

    def _sample_batch(self, batch_size, **kwds):
        seed = self._next_draw_seed()
        with self._device_lock:
            return self._engine.sample(batch_size, self._neg_ratio, seed)

    def _predict_batch(self, batch_samples, **kwds):
        """the logits of the batch's pairs (numpy float64 [B]) against their targets — the reference's training hook, kept for
        callers; the fused step computes its loss itself."""
        u, i, y = batch_samples[:3]
        with self._device_lock:
            x = self._engine.pair_scores(u, i).cpu().numpy()
            y = y.cpu().numpy() if hasattr(y, 'cpu') else np.asarray(y)
        return x.astype(np.float64), y.astype(np.float64)

    def _compute_batch_loss(self, predictions, desired_values, **kwds):
        x, y = np.asarray(predictions, dtype=np.float64), np.asarray(desired_values, dtype=np.float64)
        return float(np.mean(np.maximum(x, 0.0) - y * x + np.log1p(np.exp(-np.abs(x)))))

    # ---- prediction and serving ------------------------------------------------------------------------------------------------------
    def _predict(self, uid, iid, **kwds):
        if uid is None or iid is None:
            return None
        return float(self._predict_pairs(np.array([uid]), np.array([iid]))[0][0])

    def _predict_pairs(self, uids, iids):
        if type(self)._predict is not NeuMF._predict:
            return super()._predict_pairs(uids, iids)
        with self._device_lock:
            x = self._engine.pair_scores(np.asarray(uids, dtype=np.int32), np.asarray(iids, dtype=np.int32)).cpu().numpy()
        return _sigmoid(x), np.zeros(len(x), dtype=bool)

    def _chunk_lists(self, uids, k, novelty):
        """(idx int64 [R, k], logits float32 [R, k]) of the users' full-catalogue order, a chunk of users at a time: score_matrix + topk,
        under novelty with the exclusion mask; -1 / -inf behind a row's last eligible item"""
        uids = np.asarray(uids, dtype=np.int64)
        idx, val = np.full((len(uids), k), -1, np.int64), np.full((len(uids), k), -np.inf, np.float32)
        with self._device_lock:
            eng = self._engine
            self._upload_exclusions(novelty)
            per = eng.matrix_chunk_users(self.n_items, self.MATRIX_BUDGET_BYTES)
            for lo in range(0, len(uids), per):
                u = uids[lo:lo + per]
                scores = eng.score_matrix(u.astype(np.int32))
                i, v = eng.masked_topk(scores, eng._exclusion_mask(u), k) if novelty else eng.topk(scores, k)
                idx[lo:lo + per], val[lo:lo + per] = i.cpu().numpy(), v.cpu().numpy()
        return idx, val

    def _recommend_batch(self, uids, n, novelty):
        """Top-n of the whole catalogue for many users: chunks of matrix_chunk_users users, each one score matrix and one drx_topk"""
        k = min(int(n), self.n_items)
        idx, val = self._chunk_lists(uids, k, novelty)
        out_idx, out_val = np.full((len(idx), n), -1, np.int64), np.full((len(idx), n), -np.inf, np.float64)
        out_idx[:, :k], out_val[:, :k] = idx, _sigmoid(val)
        return out_idx, out_val

    def _catalogue_ranks(self, uids, iids, novelty):
        """positions in the full lists of the request's distinct users, from the same chunks at k = n_items"""
        uids, iids = np.asarray(uids, dtype=np.int64), np.asarray(iids, dtype=np.int64)
        users, row = np.unique(uids, return_inverse=True)
        idx, val = self._chunk_lists(users, self.n_items, novelty)
        place = np.full((len(users), self.n_items + 1), -1, np.int64)          # (column n_items: where the -1 entries of a list land)
        at = np.where(idx >= 0, idx, self.n_items)
        np.put_along_axis(place, at, np.broadcast_to(np.arange(self.n_items), idx.shape), axis=1)
        place[:, self.n_items] = -1
        known = (iids >= 0) & (iids < self.n_items)
        ranks = np.where(known, place[row, np.where(known, iids, 0)], -1)
        scores = np.full(len(uids), -np.inf, np.float64)
        listed = ranks >= 0
        scores[listed] = _sigmoid(val[row[listed], ranks[listed]])
        return ranks.astype(np.int64), scores
