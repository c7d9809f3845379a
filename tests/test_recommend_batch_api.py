"""RecommenderABC.recommend_batch and recommendation_evaluation(batched=True) on a model that defines nothing but _predict: the
base-class default (one _recommend per user) must give exactly what per-user recommend() gives.  No GPU."""
import numpy as np
import pytest


def _stub():
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender.recommender_abc import RecommenderABC

    class Stub(RecommenderABC):
        """only _predict: a fixed score table with exact ties in it"""

        def _pre_fit(self, *a, **k):
            pass

        def _sample_batch(self, *a, **k):
            pass

        def _predict_batch(self, *a, **k):
            pass

        def _compute_batch_loss(self, *a, **k):
            pass

        def _predict(self, uid, iid, **kwds):
            return float(self.table[uid, iid])

    rng = np.random.default_rng(4)
    U, N, rows = 12, 40, 150
    frame = {'user': rng.integers(100, 100 + U, rows), 'item': rng.integers(500, 500 + N, rows), 'interaction': rng.integers(0, 6, rows)}
    frame['user'][:U] = np.arange(100, 100 + U)
    frame['item'][:N] = np.arange(500, 500 + N)
    ds = InteractionDataset.read_df(frame, verbose=False)
    m = Stub(verbose=False, seed=1)
    m._bind_dataset(ds, False)
    m.fitted = True
    m.table = np.round(rng.random((m.n_users, m.n_items)), 1)            # one decimal: many exact ties
    users = [int(u) for u in rng.permutation(np.arange(100, 100 + U))[:9]]
    return m, ds, users


@pytest.mark.parametrize('novelty', [True, False])
@pytest.mark.parametrize('n', [1, 7, 40, 60])
def test_default_equals_per_user_recommend(n, novelty):
    m, ds, users = _stub()
    got = m.recommend_batch(users, n=n, novelty=novelty)
    want = [m.recommend(u, n=n, novelty=novelty) for u in users]
    assert got == want
    assert all(type(s) is type(w) and type(i) is type(j) for a, b in zip(got, want) for (s, i), (w, j) in zip(a, b))
    got = m.recommend_batch(users + users[:2], n=n, novelty=novelty, interaction_threshold=0.5)
    want = [m.recommend(u, n=n, novelty=novelty, interaction_threshold=0.5) for u in users + users[:2]]
    assert got == want and (n < 40 or any(len(a) < min(n, m.n_items) for a in got))      # (the threshold does cut long lists)


def test_as_arrays_carries_the_same_content():
    m, ds, users = _stub()
    lists = m.recommend_batch(users, n=9, interaction_threshold=0.4)
    scores, items, counts = m.recommend_batch(users, n=9, interaction_threshold=0.4, as_arrays=True)
    assert scores.shape == items.shape == (len(users), 9) and scores.dtype == np.float32 and counts.tolist() == [len(a) for a in lists]
    for r, lst in enumerate(lists):
        assert [(np.float32(s), i) for s, i in lst] == list(zip(scores[r, :counts[r]], items[r, :counts[r]]))
        assert np.isneginf(scores[r, counts[r]:]).all() and all(i is None for i in items[r, counts[r]:])


def test_unknown_user_raises_and_empty_request():
    m, ds, users = _stub()
    with pytest.raises(AssertionError, match='was not found'):
        m.recommend_batch(users[:2] + [99999], n=3)
    assert m.recommend_batch([], n=3) == []
    unfitted = type(m)(verbose=False)
    with pytest.raises(AssertionError, match='fitted'):
        unfitted.recommend_batch([1], n=3)


@pytest.mark.parametrize('novelty', [True, False])
def test_batched_recommendation_evaluation_equals_the_loop(novelty):
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Evaluation import recommendation_evaluation
    m, ds, users = _stub()
    rng = np.random.default_rng(9)
    rows = 80
    test = {'user': rng.integers(100, 114, rows), 'item': rng.integers(500, 540, rows), 'interaction': rng.integers(0, 6, rows)}   # users 112, 113: unknown
    ds_te = InteractionDataset.read_df(test, verbose=False)
    for kw in (dict(k=[1, 5, 10]), dict(k=5, n_pos_interactions=2, seed=3), dict(k=10, n_test_users=6, ignore_low_predictions_threshold=0.3)):
        a = recommendation_evaluation(m, ds_te, novelty=novelty, verbose=False, **kw)
        calls = {'batch': 0, 'single': 0}
        m.recommend_batch = lambda *x, _f=type(m).recommend_batch, **y: (calls.__setitem__('batch', calls['batch'] + 1), _f(m, *x, **y))[1]
        m.recommend = lambda *x, **y: calls.__setitem__('single', calls['single'] + 1)
        b = recommendation_evaluation(m, ds_te, novelty=novelty, verbose=False, batched=True, **kw)
        del m.recommend_batch, m.recommend
        assert a == b and a, kw
        assert calls == {'batch': 1, 'single': 0}, calls            # one call for all users, none per user
