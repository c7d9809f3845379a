"""drecpy_amd.Recommender.Baseline.LightGCN on the device against tests/lgcn_oracle.py (NumPy float64): fit on the seeded draws, the
serving calls of the base classes, a served list after a further step (the cached final embeddings must be dropped), save / load, early
stopping, the registration lists and the refusals by name.  The frame and the gate are tests/test_gpu_lgcn.py's."""
import numpy as np
import pytest

import bpr_oracle as bo
import lgcn_oracle as lo
from test_gpu_fpmc import _gate
from test_gpu_lgcn import ISOLATED_ITEM, ISOLATED_USER, N, THR, U, _all_scores, _padding_is_zero, _pairs

pytestmark = pytest.mark.gpu

K, LAYERS = 10, 3
G = 1e-5
FIT = dict(epochs=20, batch_size=64, learning_rate=1e-2, neg_ratio=3, reg_rate=1e-3)


def _dataset():
    from drecpy_amd.Dataset import InteractionDataset
    u, i, v = (np.array(c) for c in zip(*_pairs()))
    return InteractionDataset.from_arrays(u.astype(np.int64), i.astype(np.int64), v.astype(np.float64))


def _model(**kw):
    from drecpy_amd.Recommender.Baseline import LightGCN
    return LightGCN(**dict(dict(factors=K, layers=LAYERS, seed=3, interaction_threshold=THR, verbose=False), **kw))


def _raw_ids_are_internal(model):
    ds = model.interaction_dataset
    known = [i for i in range(N) if i != ISOLATED_ITEM]
    assert model.n_users == U and model.n_items == N - 1                        # nobody records item 52: it is not in the catalogue
    assert all(ds.user_to_uid(u) == u for u in range(U)) and all(ds.item_to_iid(i) == i for i in known)


def _oracle_fit(w, frame, A, model, steps, fit=FIT, layers=LAYERS):
    out = []
    for q in (w, lo.replay32(w)):
        p = {k: v.copy() for k, v in q.items()}
        st = lo.init_state(p, 'adam')
        for s in range(steps):
            lo.step(p, st, A, layers, s, *bo.sample(frame, fit['batch_size'], fit['neg_ratio'], model._draw_seed(s + 1)))
        out += [p, st]
    return out


@pytest.fixture(scope='module')
def catalogue():
    """(frame, adjacency) of the dataset's catalogue: the 52 items somebody records"""
    f = bo.Frame(U, N - 1, _pairs(), THR)
    return f, lo.adjacency(f.positives, N - 1)


@pytest.fixture(scope='module')
def fitted(catalogue):
    """(model, oracle parameters, their float32 replay) after the same 20 steps on the same draws"""
    f, A = catalogue
    w = lo.init_params(np.random.default_rng(42), U, N - 1, K)
    model = _model()
    model.fit(_dataset(), initial_weights=w, **FIT)
    _raw_ids_are_internal(model)
    p, _, p32, _ = _oracle_fit(w, f, A, model, FIT['epochs'])
    return model, p, p32


def test_fit_equals_the_oracle_fit_on_the_same_draws(fitted, catalogue):
    model, p, p32 = fitted
    A = catalogue[1]
    x = lo.scores(p, A, LAYERS)
    _gate('scores after fit(epochs=20)', _all_scores(model._engine), x, lo.scores(p32, A, LAYERS))
    _padding_is_zero(model._engine)
    assert list(model._engine.get_params()) == list(lo.NAMES)
    for u in (0, ISOLATED_USER, 2, 5):
        assert model.predict(u, 7) == pytest.approx(x[u, 7], abs=G)
    assert isinstance(model.predict(5, 7), float)
    # the training hook on the host: the pairwise differences of a batch
    uid, pos, neg = bo.sample(catalogue[0], 32, 2, 5)
    d, ones = model._predict_batch((uid, pos, neg))
    want = lo.differences(lo.final(p, A, LAYERS), U, uid, pos, neg)
    assert np.max(np.abs(d - want)) <= G * max(1.0, np.max(np.abs(want))) and ones.all()
    assert model._compute_batch_loss(d, ones) == pytest.approx(lo.loss(p, A, LAYERS, uid, pos, neg), abs=G)


def test_the_registration_lists(fitted):
    model, _, _ = fitted
    e = model._engine
    assert model.trainable_models == [e.user_emb, e.item_emb] and model.trainable_weights == [] and model.trainable_layers == []
    assert [model._apply_position(h) for h in model._fused_trainables()] == [0, 1]
    assert [tuple(v.shape) for h in model.trainable_models for v in h.trainable_weights] == [(U, K), (N - 1, K)]
    assert e.P.data_ptr() == e.E0.data_ptr() and e.Q.data_ptr() == e.E0.data_ptr() + U * e.ld * 4       # one allocation


def test_recommend_batch_equals_recommend_and_the_oracle_order(fitted, catalogue):
    model, p, _ = fitted
    n_items = N - 1
    x = lo.scores(p, catalogue[1], LAYERS)
    users = [0, ISOLATED_USER, 2, 3, 5, 17, 36, 5]
    for n in (1, 10, n_items):
        for novelty in (True, False):
            lists = model.recommend_batch(users, n=n, novelty=novelty)
            for u, got in zip(users, lists):
                one = model.recommend(u, n=n, novelty=novelty)
                assert [i for _, i in got] == [i for _, i in one], (u, n, novelty)
                assert np.allclose([s for s, _ in got], [s for s, _ in one], rtol=0, atol=G)
                allowed = [i for i in range(n_items) if not (novelty and i in model._recorded_items(u))]
                assert len(got) == min(n, len(allowed)) and all(i in allowed for _, i in got)
                if not got:
                    continue
                _gate(f'user {u} values', [s for s, _ in got], [x[u, i] for _, i in got], [x[u, i] for _, i in got])
                for (_, a), (_, b) in zip(got, got[1:]):       # the oracle's order wherever its scores differ by more than the gate
                    assert x[u, a] >= x[u, b] - 2 * G, (u, a, b)
    assert model.recommend_batch([2], n=5, novelty=True) == [[]]                 # user 2 records the whole catalogue
    # pairs below the threshold are no edges of the graph, but novelty excludes them
    assert not {0, 1} & {i for _, i in model.recommend_batch([ISOLATED_USER], n=n_items, novelty=True)[0]}
    assert {0, 1} <= {i for _, i in model.recommend_batch([ISOLATED_USER], n=n_items, novelty=False)[0]}


def test_a_step_after_serving_drops_the_cached_embeddings(catalogue):
    f, A = catalogue
    w = lo.init_params(np.random.default_rng(6), U, N - 1, K)
    model = _model()
    model.fit(_dataset(), initial_weights=w, **dict(FIT, epochs=2))
    p, st, p32, st32 = _oracle_fit(w, f, A, model, 2)
    users = [0, 3, 5, 17, 36]
    x0 = lo.scores(p, A, LAYERS)
    first = model.recommend_batch(users, n=10, novelty=False)
    for u, got in zip(users, first):
        _gate(f'user {u} before the step', [s for s, _ in got], [x0[u, i] for _, i in got], [x0[u, i] for _, i in got])
    # one further step with a step size that moves every score by far more than the gate
    hp = dict(lo.HP, lr=0.1)
    triples = bo.sample(f, 64, 3, 99)
    model._engine.lr = hp['lr']
    for q, s in ((p, st), (p32, st32)):
        lo.step(q, s, A, LAYERS, 2, *triples, hp=hp)
    model._engine.step(2, *triples)
    x, x32 = lo.scores(p, A, LAYERS), lo.scores(p32, A, LAYERS)
    second = model.recommend_batch(users, n=10, novelty=False)
    for u, got in zip(users, second):
        items = [i for _, i in got]
        assert np.max(np.abs(x[u, items] - x0[u, items])) > 100 * G          # stale embeddings cannot pass the gate below
        _gate(f'user {u} after the step', [s for s, _ in got], x[u, items], x32[u, items])
        for a, b in zip(items, items[1:]):
            assert x[u, a] >= x[u, b] - 2 * G, (u, a, b)
    _gate('all scores after the step', _all_scores(model._engine), x, x32)


def test_catalogue_ranks_are_positions_in_the_full_list(fitted):
    model, _, _ = fitted
    users, items = [2, 5, 5, 17, 36, 36, 36, ISOLATED_USER], [17, 0, 51, 30, 1, 2, 3, 4]
    for novelty in (True, False):
        ranks, scores = model.catalogue_ranks(users, items, novelty=novelty, return_scores=True)
        full = {u: model.recommend(u, n=None, novelty=novelty) for u in set(users)}
        for u, i, r, s in zip(users, items, ranks, scores):
            place = {item: (j, v) for j, (v, item) in enumerate(full[u])}
            if i in place:
                assert r == place[i][0] and s == pytest.approx(place[i][1], abs=G), (u, i, novelty)
            else:
                assert r == -1 and s == -np.inf, (u, i, novelty)


def test_predict_pairs_equals_predict(fitted, catalogue):
    model, p, p32 = fitted
    A = catalogue[1]
    rng = np.random.default_rng(8)
    users, items = rng.integers(0, U, size=200), rng.integers(0, N - 1, size=200)
    got = model.predict_pairs(users.tolist(), items.tolist())
    assert got.dtype == np.float64
    assert np.array_equal(got, np.array([model.predict(int(u), int(i)) for u, i in zip(users, items)]))
    _gate('predict_pairs', got, lo.scores(p, A, LAYERS)[users, items], lo.scores(p32, A, LAYERS)[users, items])
    assert np.isnan(model.predict_pairs([1, 999], [1, 1], skip_errors=True)[1])


def test_rank_and_evaluations_batched_and_not(fitted, catalogue):
    from drecpy_amd.Evaluation import predictive_evaluation, ranking_evaluation, recommendation_evaluation
    model, p, _ = fitted
    x = lo.scores(p, catalogue[1], LAYERS)
    cands = [3, 8, 11, 20, 33, 39]
    got = model.rank(5, cands, novelty=False)
    assert sorted(i for _, i in got) == cands
    for (_, a), (_, b) in zip(got, got[1:]):
        assert x[5, a] >= x[5, b] - 2 * G
    kw = dict(n_pos_interactions=3, n_neg_interactions=10, generate_negative_pairs=True, k=[1, 5], seed=4, verbose=False)
    a = ranking_evaluation(model, batched=True, **kw)
    b = ranking_evaluation(model, batched=False, **kw)
    assert a == b and a and any(v > 0 for v in a.values()), (a, b)
    r = [recommendation_evaluation(model, _dataset(), k=[1, 5], novelty=False, seed=4, verbose=False, batched=batched)
         for batched in (False, True, 'ranks')]
    assert r[0] == r[1] == r[2] and r[0] and any(v > 0 for v in r[0].values()), r
    e = [predictive_evaluation(model, n_test_predictions=100, skip_errors=True, verbose=False, **kw) for kw in ({}, {'batched': False})]
    assert e[0] and all(np.isfinite(v) for v in e[0].values()) and e[0] == pytest.approx(e[1], rel=1e-12), e


def test_save_and_load_predict_identically(fitted, tmp_path):
    from drecpy_amd.Recommender.Baseline import LightGCN
    model, _, _ = fitted
    path = str(tmp_path / 'lightgcn.pkl')
    model.save(path)
    other = LightGCN.load(path)
    assert isinstance(other, LightGCN) and other._engine._graph.nnz2 == model._engine._graph.nnz2
    users, items = list(range(U)) * 2, [(7 * k) % (N - 1) for k in range(2 * U)]
    assert np.array_equal(other.predict_pairs(users, items), model.predict_pairs(users, items))
    assert other.recommend_batch([5, 36, ISOLATED_USER], n=7) == model.recommend_batch([5, 36, ISOLATED_USER], n=7)
    assert other.recommend(5, n=7) == model.recommend(5, n=7)


def test_two_epochs_with_a_callback_early_stopping_and_the_revert(catalogue):
    from drecpy_amd.Recommender.early_stopping import MaxValidationValueRule
    f, A = catalogue
    w = lo.init_params(np.random.default_rng(9), U, N - 1, 6)
    seen = []
    model = _model(factors=6, layers=2, seed=1)
    model.fit(_dataset(), epochs=2, batch_size=32, learning_rate=1e-2, neg_ratio=2, reg_rate=1e-3, initial_weights=w,
              epoch_callback_fn=lambda m: seen.append(float(m.predict(5, 7))) or {'score': len(seen)}, epoch_callback_freq=1,
              early_stopping_rule=MaxValidationValueRule('score'), early_stopping_freq=999)      # (a callback runs where a rule logs)
    assert len(seen) == 2 and seen[0] != seen[1] and model.fitted
    seen.clear()
    model = _model(factors=6, layers=2, seed=1)
    model.fit(_dataset(), epochs=6, batch_size=32, learning_rate=1e-2, neg_ratio=2, reg_rate=1e-3, initial_weights=w,
              epoch_callback_fn=lambda m: seen.append(float(m.predict(5, 7))) or {'score': -len(seen)}, epoch_callback_freq=2,
              early_stopping_rule=MaxValidationValueRule('score'), early_stopping_freq=2)
    assert len(seen) >= 1 and model.fitted
    # the best epoch is the first one evaluated (the score falls): the weights are those of epoch 2, and so is what is served
    fit = dict(batch_size=32, neg_ratio=2)
    p, _, p32, _ = _oracle_fit(w, f, A, model, 2, fit, 2)
    _gate('scores after the revert to epoch 2', _all_scores(model._engine), lo.scores(p, A, 2), lo.scores(p32, A, 2))


def test_the_seed_draws_the_initial_weights_as_bpr_does():
    from drecpy_amd.Recommender.Baseline import BPR
    a, b = _model(seed=11, layers=0), BPR(factors=K, seed=11, interaction_threshold=THR, verbose=False)
    a.fit(_dataset(), **dict(FIT, epochs=1, learning_rate=0.0, reg_rate=0.0))
    b.fit(_dataset(), **dict(FIT, epochs=1, learning_rate=0.0, reg_rate=0.0))
    pa, pb = a._engine.get_params(), b._engine.get_params()
    assert np.array_equal(pa['P'], pb['P']) and np.array_equal(pa['Q'], pb['Q']) and np.abs(pa['P']).max() < 0.1


@pytest.mark.parametrize('what,kw', [('factors', dict(factors=0)), ('factors', dict(factors=257)), ('factors', dict(factors=2.5)),
                                     ('layers', dict(layers=-1)), ('layers', dict(layers=5)), ('layers', dict(layers=1.5))])
def test_fit_refuses_by_name(what, kw):
    with pytest.raises(Exception, match=rf'LightGCN\({what}='):
        _model(**kw).fit(_dataset(), epochs=1, batch_size=8)


def test_other_refusals_carry_the_name(tmp_path):
    import torch.distributed as dist
    from drecpy_amd.Dataset import InteractionDataset
    with pytest.raises(Exception, match=r'LightGCN.fit\(neg_ratio=0\)'):
        _model().fit(_dataset(), neg_ratio=0, epochs=1, batch_size=8)
    with pytest.raises(Exception, match=r'LightGCN trains with the dense rules adam, adagrad, sgd, rmsprop \(dense update of the embedding '
                                        r'table\)'):
        _model().fit(_dataset(), optimizer='rowwise_adagrad', epochs=1, batch_size=8)
    full = InteractionDataset.from_arrays(np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1]), np.array([2.0, 2.0, 0.5, 0.25]))
    with pytest.raises(Exception, match='LightGCN.fit: the dataset has no eligible user'):
        _model().fit(full, epochs=1, batch_size=8)
    if dist.is_available():
        dist.init_process_group('gloo', init_method=f'file://{tmp_path}/rdzv', rank=0, world_size=1)
        try:
            with pytest.raises(Exception, match='LightGCN.fit under a torch.distributed process group: LightGCN trains on a single GPU only.'):
                _model().fit(_dataset(), epochs=1, batch_size=8)
        finally:
            dist.destroy_process_group()
