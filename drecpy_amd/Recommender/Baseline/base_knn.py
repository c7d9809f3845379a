"""What UserKNN and ItemKNN share (DRecPy/Recommender/Baseline/base_knn.py): the constructor, the neighbour table built on the device
(KnnEngine.neighbours: co-rating sums on the matrix cores) and the prediction hooks that walk it."""
from abc import ABC

import numpy as np

from ..recommender_abc import RecommenderABC

SIM_METRICS = ('adjusted_cosine', 'cosine', 'cosine_cf', 'jaccard', 'msd', 'pearson')
AGGREGATIONS = ('mean', 'weighted_mean')
_MATRIX_CHUNK_BYTES = 1 << 30        # device bytes of one chunk's [R, n_items] prediction matrix in recommend_batch


class BaseKNN(RecommenderABC, ABC):
    """k: neighbours used for a prediction; m: minimum number of co-ratings for a similarity to count; sim_metric: 'adjusted_cosine',
    'cosine', 'cosine_cf', 'jaccard', 'msd' or 'pearson'; aggregation: 'mean' or 'weighted_mean'; shrinkage: discount of similarities
    with few co-ratings (None: none); use_averages: predict the item's (UserKNN) / user's (ItemKNN) mean when no neighbour has a term."""
    type = None

    def __init__(self, k=20, m=5, sim_metric='adjusted_cosine', aggregation='weighted_mean', shrinkage=100, use_averages=False,
                 device='cuda:0', **kwds):
        super().__init__(**kwds)
        if sim_metric not in SIM_METRICS:
            raise Exception(f'There is no similarity metric corresponding to the name "{sim_metric}".')
        if aggregation not in AGGREGATIONS:
            raise Exception(f'There is no aggregation approach corresponding to the name "{aggregation}".')
        from ...engine_knn import KnnEngine
        if not 1 <= int(k) <= KnnEngine.MAX_K:
            raise Exception(f'k = {k} is outside the domain of the neighbour kernel (1..{KnnEngine.MAX_K}).')
        self.k, self.m, self.sim_metric, self.aggregation = int(k), int(m), sim_metric, aggregation
        self.shrinkage, self.use_averages, self.device = shrinkage, use_averages, device
        self._neighbours = dict()

    # ---- fit ------------------------------------------------------------------------------------------------------------------------
    def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
        ds = self.interaction_dataset
        csr = ds.interaction_csr()
        if int(csr[0][-1]) != len(ds):
            raise Exception(f'{type(self).__name__} takes one rating per (user, item): the dataset holds duplicate (user, item) rows.')
        if np.any(np.asarray(ds._col('interaction')) == 0):
            raise Exception(f'{type(self).__name__} takes non-zero ratings: the dataset holds a zero-valued interaction (absent and '
                            f'zero cannot be told apart in the rating matrix).')
        self._info('Computing neighbours...')
        self._build_engine()
        values = csr[2]
        lo, hi = float(values.min()), float(values.max())
        if len(values) < self.n_users * self.n_items:      # msd's max_diff: the sparse matrix's minimum counts its implicit zeros
            lo, hi = min(lo, 0.0), max(hi, 0.0)
        with self._device_lock:
            idx, sim = self._engine.neighbours(self.sim_metric, self.k, self.m, self.shrinkage, max_diff=(hi - lo) or 1.0)
            self._set_host_table(idx.cpu().numpy(), sim.cpu().numpy())

    def _build_engine(self):
        from ...engine_knn import KnnEngine
        ds = self.interaction_dataset
        self._engine = KnnEngine(self.n_users, self.n_items, self.type, device=self.device)
        if self._engine.dense_bytes() > KnnEngine.DENSE_BUDGET_BYTES:
            raise MemoryError(f'the dense rating matrix of this model takes {self._engine.dense_bytes()} bytes, above '
                              f'KnnEngine.DENSE_BUDGET_BYTES = {KnnEngine.DENSE_BUDGET_BYTES}')
        csr = ds.interaction_csr()
        self._engine.set_interactions(csr, ds.interaction_csr(transpose=True))
        self._ui = (np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int64), np.asarray(csr[2], np.float32))
        self._user_mean = self._engine.user_mean.cpu().numpy()
        self._item_mean = self._engine.item_mean.cpu().numpy()

    def _set_host_table(self, idx, sim):
        """self._neighbours as the reference keeps it: {id: [(similarity, id), ...]} in nlargest order"""
        self._neighbours = {r: [(float(s), int(j)) for s, j in zip(sim[r], idx[r]) if j >= 0] for r in range(len(idx))}

    def _restore_engine(self, params):
        """RecommenderABC.load: the engine rebuilt from the saved dataset and the saved neighbour table"""
        self._build_engine()
        self._engine.set_table(params['nb_idx'], params['nb_sim'])

    def _sample_batch(self, batch_size, **kwds):
        raise NotImplementedError

    def _predict_batch(self, batch_samples, **kwds):
        raise NotImplementedError

    def _compute_batch_loss(self, predictions, desired_values, **kwds):
        raise NotImplementedError

    def _compute_reg_loss(self, reg_rate, batch_size, **kwds):
        raise NotImplementedError

    # ---- predictions ----------------------------------------------------------------------------------------------------------------
    def _get_interaction(self, uid, iid):
        """the rating of (uid, iid) as the device holds it (float32), or None"""
        indptr, cols, vals = self._ui
        lo, hi = indptr[uid], indptr[uid + 1]
        at = lo + np.searchsorted(cols[lo:hi], iid)
        return float(vals[at]) if at < hi and cols[at] == iid else None

    def _predict(self, uid, iid, **kwds):
        """base_knn.py:94-107 from the host table: the terms in neighbour-list order, then the aggregation (aggregation.py)"""
        if uid is None or iid is None:
            return None
        user = self.type == 'user'
        num = den = 0.0
        for similarity, neighbour in self._neighbours[uid if user else iid]:
            r = self._get_interaction(neighbour, iid) if user else self._get_interaction(uid, neighbour)
            if r is None:
                continue
            if self.aggregation == 'weighted_mean':
                num = num + similarity * r
                den = den + similarity
            else:
                num = num + r
                den = den + 1.0
        if den > 0:
            return num / den
        return float(self._item_mean[iid] if user else self._user_mean[uid]) if self.use_averages else None

    def _predict_pairs(self, uids, iids):
        with self._device_lock:
            out, none = self._engine.pair_scores(np.asarray(uids, np.int32), np.asarray(iids, np.int32), self.aggregation, self.use_averages)
            return out.cpu().numpy(), none.cpu().numpy().astype(bool)

    def _rank(self, uid, iids, n, novelty):
        return self._rank_rows([uid], [list(iids)], n, novelty)[0]

    def _rank_rows(self, uids, iid_lists, n, novelty):
        """_rank for many users in one engine call: row r holds the at most n best candidates of iid_lists[r] the model has a
        prediction for, by (prediction, iid) descending — KnnEngine.score_rows, then the masked top-k."""
        cand = self._candidate_rows(iid_lists)
        if novelty:
            indptr, cols, _ = self._ui
            for r, uid in enumerate(uids):
                cand[r, cols[indptr[uid]:indptr[uid + 1]]] = False
        return self._ranked(np.asarray(uids, np.int32), cand, n)

    def _ranked(self, uids, cand, n):
        k = min(int(n), int(cand.sum(axis=1).max()) if len(cand) else 0)
        if k <= 0:
            return [[] for _ in cand]
        with self._device_lock:
            scores, mask = self._engine.score_rows(uids, cand, self.aggregation, self.use_averages)
            idx, val = self._engine.topk(scores, k, mask)
            idx, val = idx.cpu().numpy(), val.cpu().numpy()
        return [[(float(v), int(i)) for v, i in zip(vr, ir) if i >= 0] for vr, ir in zip(val, idx)]

    def _recommend_batch(self, uids, n, novelty):
        """Top-n of the whole catalogue for many users.  n <= KnnEngine.FUSED_MAX_N: ONE KnnEngine.recommend (drx_knn_recommend:
        predictions, exclusions and selection in the workgroup that holds the user's row), the predictions and
        the order of recommend() bit for bit.  A longer list (n=None), or an engine with fused = False: the score-matrix route."""
        eng = self._engine
        if not (eng.fused and 1 <= int(n) <= eng.FUSED_MAX_N):
            return self._recommend_batch_by_matrix(uids, n, novelty)
        with self._device_lock:
            self._upload_exclusions(novelty)
            idx, val = eng.recommend(np.asarray(uids, np.int32), int(n), self.aggregation, self.use_averages, exclude=bool(novelty),
                                     chunk_bytes=_MATRIX_CHUNK_BYTES)
            return idx.cpu().numpy().astype(np.int64), val.cpu().numpy().astype(np.float64)

    def _recommend_batch_by_matrix(self, uids, n, novelty):
        """The same in chunks whose prediction matrix stays within a budget; excluded under novelty: the rows of _exclusion_csr
        (every (uid, iid) row of the frame)."""
        idx = np.full((len(uids), n), -1, dtype=np.int64)
        val = np.full((len(uids), n), -np.inf, dtype=np.float64)
        per = self._engine.matrix_chunk_users(max(self.n_items, 1), _MATRIX_CHUNK_BYTES)
        xptr, xidx = self._exclusion_csr() if novelty else (None, None)
        for lo in range(0, len(uids), per):
            chunk = np.asarray(uids[lo:lo + per], np.int64)
            cand = np.ones((len(chunk), self.n_items), dtype=bool)
            if novelty:
                for r, uid in enumerate(chunk):
                    cand[r, xidx[xptr[uid]:xptr[uid + 1]]] = False
            for r, ranked in enumerate(self._ranked(chunk.astype(np.int32), cand, min(int(n), self.n_items))):
                for j, (score, iid) in enumerate(ranked):
                    idx[lo + r, j], val[lo + r, j] = iid, score
        return idx, val

    def _catalogue_ranks(self, uids, iids, novelty):
        """The pairs grouped by user (one row a user, however many items) and ONE KnnEngine.rank_lists (drx_knn_rank_lists: the ranks
        counted on the user's row where it lies); the positions and values of recommend()'s list bit for bit.  The device ignores a
        target's own exclusion: an excluded pair is set to -1 / -inf here, as an unknown item (iid -1) comes back."""
        eng = self._engine
        if not eng.fused:
            return super()._catalogue_ranks(uids, iids, novelty)
        uids, iids = np.asarray(uids, dtype=np.int64), np.asarray(iids, dtype=np.int64)
        with self._device_lock:
            self._upload_exclusions(novelty)
            order, starts, indptr = self._grouped_pairs(uids, iids, len(uids) + 1)
            r, s = eng.rank_lists(uids[order[starts]].astype(np.int32), indptr, iids[order].astype(np.int32), self.aggregation,
                                  self.use_averages, exclude=bool(novelty), chunk_bytes=_MATRIX_CHUNK_BYTES)
            rank, score = np.empty(len(uids), np.int64), np.empty(len(uids), np.float64)
            rank[order], score[order] = r.cpu().numpy(), s.cpu().numpy()
            if novelty:
                self._unlist_excluded(uids, iids, rank, score)
        return rank, score
