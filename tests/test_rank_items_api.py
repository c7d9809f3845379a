"""RecommenderABC.catalogue_ranks and recommendation_evaluation(batched='ranks') on a model that defines nothing but _predict (the
stub of test_recommend_batch_api.py: a score table with many exact ties): the base-class default must give exactly the positions of
per-user recommend(), and the evaluation rebuilt from ranks exactly the loop's numbers.  No GPU."""
import numpy as np
import pytest

from test_recommend_batch_api import _stub


@pytest.mark.parametrize('novelty', [True, False])
def test_ranks_are_the_positions_in_recommend(novelty):
    m, ds, users = _stub()
    items = list(range(500, 540))
    pair_users = [u for u in users for _ in items]
    pair_items = items * len(users)
    ranks, scores = m.catalogue_ranks(pair_users, pair_items, novelty=novelty, return_scores=True)
    assert ranks.dtype == np.int64 and ranks.shape == (len(pair_users),) and scores.shape == ranks.shape
    assert (m.catalogue_ranks(pair_users, pair_items, novelty=novelty) == ranks).all()
    n_excluded = 0
    for j, u in enumerate(users):
        listed = m.recommend(u, n=None, novelty=novelty)
        place = {item: (p, score) for p, (score, item) in enumerate(listed)}
        for i, item in enumerate(items):
            got = (int(ranks[j * len(items) + i]), float(scores[j * len(items) + i]))
            assert got == place.get(item, (-1, -np.inf)), (u, item)
        n_excluded += len(items) - len(listed)
        if novelty:                                                   # (the excluded ones are the user's rows of the frame)
            assert {item for item in items if item not in place} == set(ds.select(f'user == {u}').values_list('item', to_list=True))
    assert (n_excluded > 0) == novelty and (ranks == -1).sum() == n_excluded


def test_unknown_items_unknown_users_and_empty_requests():
    m, ds, users = _stub()
    ranks, scores = m.catalogue_ranks([users[0], users[1], users[0]], [99999, 500, 77777], novelty=False, return_scores=True)
    assert ranks[0] == -1 and ranks[2] == -1 and ranks[1] >= 0 and np.isneginf(scores[[0, 2]]).all() and np.isfinite(scores[1])
    with pytest.raises(AssertionError, match='was not found'):
        m.catalogue_ranks([users[0], 99999], [500, 501])
    with pytest.raises(AssertionError, match='parallel'):
        m.catalogue_ranks(users[:2], [500])
    assert m.catalogue_ranks([], []).shape == (0,)
    with pytest.raises(AssertionError, match='fitted'):
        type(m)(verbose=False).catalogue_ranks([1], [1])


@pytest.mark.parametrize('novelty', [True, False])
@pytest.mark.parametrize('n_pos', [None, 1])
def test_evaluation_from_ranks_equals_the_loop(novelty, n_pos):
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Evaluation import recommendation_evaluation
    m, ds, users = _stub()
    rng = np.random.default_rng(9)
    rows = 80
    test = {'user': rng.integers(100, 114, rows), 'item': rng.integers(500, 544, rows), 'interaction': rng.integers(0, 6, rows)}   # users 112, 113 and items 540 ..: unknown
    ds_te = InteractionDataset.read_df(test, verbose=False)
    kw = dict(k=[1, 5, 40], n_pos_interactions=n_pos, novelty=novelty, seed=3, verbose=False)
    want = recommendation_evaluation(m, ds_te, **kw)
    calls = {'ranks': 0, 'other': 0}
    m.catalogue_ranks = lambda *x, _f=type(m).catalogue_ranks, **y: (calls.__setitem__('ranks', calls['ranks'] + 1), _f(m, *x, **y))[1]
    m.recommend = m.recommend_batch = lambda *x, **y: calls.__setitem__('other', calls['other'] + 1)
    got = recommendation_evaluation(m, ds_te, batched='ranks', **kw)
    del m.catalogue_ranks, m.recommend, m.recommend_batch
    assert got == want and want and any(v > 0 for v in want.values())
    assert calls == {'ranks': 1, 'other': 0}, calls                  # one call for all pairs, no list asked for
    assert recommendation_evaluation(m, ds_te, batched=True, **kw) == want


def test_a_threshold_on_predictions_is_refused():
    from drecpy_amd.Evaluation import recommendation_evaluation
    m, ds, users = _stub()
    with pytest.raises(AssertionError, match='ignore_low_predictions_threshold'):
        recommendation_evaluation(m, ds, k=5, batched='ranks', ignore_low_predictions_threshold=0.3, verbose=False)
    with pytest.raises(AssertionError, match='ranks'):
        recommendation_evaluation(m, ds, k=5, batched='rank', verbose=False)
