"""drecpy_amd.Recommender.Baseline.SASRec on the device against tests/sasrec_oracle.py (NumPy float64): fit on the list sampler's
stream, the serving calls of the base classes, save / load, callbacks, and the refusals by name.  The frame and its sequences are
those of tests/test_gpu_fpmc.py (23 users x 41 items); the gate is the project's (see tests/test_gpu_sasrec.py)."""
import numpy as np
import pytest

import sasrec_oracle as so
from oracle.data_oracle import list_sample_counter
from test_gpu_fpmc import LF, N, RF, THR, U, _dataset, _gate, _records
from test_gpu_gru_api import ordered_sequences
from test_gpu_sasrec import _all_scores, _padding_is_zero

pytestmark = pytest.mark.gpu

H, BLOCKS = 12, 2
FIT = dict(epochs=20, batch_size=64, learning_rate=1e-2, neg_ratio=RF, reg_rate=1e-3)


def _oracle_fit(w, twin, model, epochs, B, r):
    out = []
    for q in (w, so.replay32(w)):
        p = {k: v.copy() for k, v in q.items()}
        st = so.init_state(p, 'adam')
        for s in range(epochs):
            so.step(p, st, s, *list_sample_counter(twin, B, LF, 1, r, model._draw_seed(s + 1)), 'adam')
        out.append(p)
    return out


@pytest.fixture(scope='module')
def fitted():
    """(model, oracle parameters, their float32 replay, baskets) after the same 20 steps on the same draws"""
    from drecpy_amd.Recommender.Baseline import SASRec
    w = so.init_params(np.random.default_rng(42), N, H, LF, BLOCKS)
    model = SASRec(hidden=H, L=LF, blocks=BLOCKS, seed=3, interaction_threshold=THR, verbose=False)
    model.fit(_dataset(), initial_weights=w, **FIT)
    ds = model.interaction_dataset
    assert all(ds.user_to_uid(u) == u for u in range(U)) and all(ds.item_to_iid(i) == i for i in range(N))
    twin = so.twin_of(_records()[1], N, LF, RF)
    p, p32 = _oracle_fit(w, twin, model, FIT['epochs'], FIT['batch_size'], RF)
    return model, p, p32, so.baskets_of(twin, U, LF)


def test_the_windows_fed_to_the_step_are_the_oracle_streams(fitted):
    model, _, _, baskets = fitted
    seqs = _records()[1]
    twin = so.twin_of(seqs, N, LF, RF)
    for n, seed in ((1, 0), (257, model._draw_seed(1)), (1000, 0xFEDCBA9876543210)):
        got = [t.cpu().numpy() for t in model._sampler.sample_device(n, seed)]
        want = so.windows(twin, n, LF, RF, seed & ((1 << 64) - 1))
        for g, w_, name in zip(got, want, ('uid', 'before', 'after')):
            assert g.dtype == np.int32 and np.array_equal(g, w_), f'{name} differs at n {n}'
    assert np.array_equal(model._engine.baskets.cpu().numpy(), baskets)
    assert baskets[1].tolist() == [seqs[1][0], -1] and baskets[2].tolist() == [-1, -1] and baskets[3].tolist() == seqs[3][-2:]


def test_fit_equals_the_oracle_fit_on_the_same_draws(fitted):
    model, p, p32, baskets = fitted
    x = so.scores(p, baskets)
    _gate('scores after fit(epochs=20)', _all_scores(model._engine), x, so.scores(p32, baskets))
    _padding_is_zero(model._engine)
    assert list(model._engine.get_params()) == so.names(BLOCKS)
    for u in (1, 2, 5):                                     # fewer than L items, an empty basket, an ordinary user
        assert model.predict(u, 7) == pytest.approx(x[u, 7], abs=1e-5)
    assert isinstance(model.predict(5, 7), float)
    assert model.predict(2, 7) == pytest.approx(p['b'][7], abs=1e-5)
    # the training hook on the host gives the oracle's differences
    uid, before, after = so.windows(so.twin_of(_records()[1], N, LF, RF), 16, LF, RF, 5)
    d, ones = model._predict_batch((uid, before, after))
    assert np.max(np.abs(d - so.deltas(p, before, after).reshape(-1))) <= 1e-4 and ones.all()


def test_recommend_batch_equals_recommend_and_the_oracle_order(fitted):
    model, p, _, baskets = fitted
    x = so.scores(p, baskets)
    G = 1e-5
    users = [0, 1, 2, 3, 5, 17, 22, 5]
    for n in (1, 10, N):
        for novelty in (True, False):
            lists = model.recommend_batch(users, n=n, novelty=novelty)
            for u, got in zip(users, lists):
                one = model.recommend(u, n=n, novelty=novelty)
                assert [i for _, i in got] == [i for _, i in one], (u, n, novelty)
                assert np.allclose([s for s, _ in got], [s for s, _ in one], rtol=0, atol=G)
                allowed = [i for i in range(N) if not (novelty and i in model._recorded_items(u))]
                assert len(got) == min(n, len(allowed)) and all(i in allowed for _, i in got)
                assert np.max(np.abs(np.array([s for s, _ in got]) - np.array([x[u, i] for _, i in got]))) <= G * max(1.0, np.abs(x).max())
                for (_, a), (_, b) in zip(got, got[1:]):       # the oracle's order wherever its scores differ by more than the gate
                    assert x[u, a] >= x[u, b] - 2 * G, (u, a, b)
                best = sorted(allowed, key=lambda i: -x[u, i])[:len(got)]
                if len(allowed) == len(got) or x[u, best[-1]] - max([x[u, i] for i in allowed if i not in best], default=-np.inf) > 2 * G:
                    assert sorted(best) == sorted(i for _, i in got), (u, n, novelty)
    assert len(model.recommend_batch([0], n=N, novelty=True)[0]) == RF             # user 0 records all but RF items


def test_catalogue_ranks_are_positions_in_the_full_list(fitted):
    model, _, _, _ = fitted
    requests = (([2, 5, 5, 17, 22, 22, 22, 1], [17, 0, 40, 30, 1, 2, 3, 4]), ([5] * 9 + [22] * 9, [(5 * k) % N for k in range(18)]))
    for (users, items), novelty in ((r, nov) for r in requests for nov in (True, False)):
        ranks, scores = model.catalogue_ranks(users, items, novelty=novelty, return_scores=True)
        full = {u: model.recommend(u, n=None, novelty=novelty) for u in set(users)}
        for u, i, r, s in zip(users, items, ranks, scores):
            place = {item: (j, v) for j, (v, item) in enumerate(full[u])}
            if i in place:
                assert r == place[i][0] and s == pytest.approx(place[i][1], abs=1e-5), (u, i, novelty)
            else:
                assert r == -1 and s == -np.inf, (u, i, novelty)


def test_predict_pairs_equals_predict(fitted):
    model, p, p32, baskets = fitted
    rng = np.random.default_rng(8)
    users, items = rng.integers(0, U, size=200), rng.integers(0, N, size=200)
    got = model.predict_pairs(users.tolist(), items.tolist())
    assert got.dtype == np.float64
    assert np.array_equal(got, np.array([model.predict(int(u), int(i)) for u, i in zip(users, items)]))
    _gate('predict_pairs', got, so.scores(p, baskets)[users, items], so.scores(p32, baskets)[users, items])
    assert np.isnan(model.predict_pairs([1, 999], [1, 1], skip_errors=True)[1])


def test_rank_and_evaluations_batched_and_not(fitted):
    from drecpy_amd.Evaluation import predictive_evaluation, ranking_evaluation, recommendation_evaluation
    model, p, _, baskets = fitted
    x = so.scores(p, baskets)
    cands = [3, 8, 11, 20, 33, 40]
    got = model.rank(5, cands, novelty=False)
    assert sorted(i for _, i in got) == cands
    for (_, a), (_, b) in zip(got, got[1:]):
        assert x[5, a] >= x[5, b] - 2e-5
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
    from drecpy_amd.Recommender.Baseline import SASRec
    model, _, _, baskets = fitted
    path = str(tmp_path / 'sasrec.pkl')
    model.save(path)
    other = SASRec.load(path)
    assert isinstance(other, SASRec)
    assert np.array_equal(other._engine.baskets.cpu().numpy(), baskets)                       # rebuilt from the dataset
    users, items = list(range(U)) * 2, [(7 * k) % N for k in range(2 * U)]
    assert np.array_equal(other.predict_pairs(users, items), model.predict_pairs(users, items))
    assert other.recommend_batch([5, 22, 1, 2], n=7) == model.recommend_batch([5, 22, 1, 2], n=7)
    assert other.recommend(5, n=7) == model.recommend(5, n=7)


def test_callbacks_early_stopping_and_loss():
    from drecpy_amd.Recommender.Baseline import SASRec
    from drecpy_amd.Recommender.early_stopping import MaxValidationValueRule
    w = so.init_params(np.random.default_rng(9), N, 5, LF, 1)
    seen = []
    model = SASRec(hidden=5, L=LF, blocks=1, seed=1, interaction_threshold=THR, verbose=False)
    model.fit(_dataset(), epochs=6, batch_size=32, learning_rate=1e-2, neg_ratio=2, reg_rate=1e-3, initial_weights=w,
              epoch_callback_fn=lambda m: seen.append(float(m.predict(5, 7))) or {'score': -len(seen)}, epoch_callback_freq=2,
              early_stopping_rule=MaxValidationValueRule('score'), early_stopping_freq=2)
    assert len(seen) >= 1 and model.fitted
    # the best epoch is the first one evaluated (the score falls): the weights are those of epoch 2
    twin = so.twin_of(_records()[1], N, LF, 2)
    p, p32 = _oracle_fit(w, twin, model, 2, 32, 2)
    baskets = so.baskets_of(twin, U, LF)
    _gate('scores after the revert to epoch 2', _all_scores(model._engine), so.scores(p, baskets), so.scores(p32, baskets))


def test_the_loss_falls_on_sequences_with_a_rule():
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender.Baseline import SASRec
    from drecpy_amd.Recommender.early_stopping import MaxValidationValueRule
    seqs = ordered_sequences()
    u = np.concatenate([[g] * len(s) for g, s in enumerate(seqs)]).astype(np.int64)
    i = np.concatenate(seqs).astype(np.int64)
    t = np.concatenate([np.arange(len(s)) for s in seqs]).astype(np.int64)
    ds = InteractionDataset.from_arrays(u, i, np.full(len(u), 2.0), timestamp=t)
    model = SASRec(hidden=16, L=2, blocks=2, seed=5, interaction_threshold=THR, verbose=False)
    model.fit(ds, epochs=200, batch_size=64, learning_rate=2e-2, neg_ratio=2, reg_rate=1e-5,
              early_stopping_rule=MaxValidationValueRule('x'), early_stopping_freq=999)   # (a rule makes fit() log the loss of every step)
    losses = model._loss_tracker.epoch_losses
    assert len(losses) == 200
    first, last = float(np.mean(losses[:10])), float(np.mean(losses[-10:]))
    print(f'mean logged loss: first 10 steps {first:.4f}, last 10 steps {last:.4f}')
    assert last < first, (first, last)


@pytest.mark.parametrize('what', ['neg_ratio 0', 'neg_ratio 17', 'hidden 2.5', 'hidden 65', 'blocks 3', 'L 17', 'no sequence', 'keras',
                                  'optimizer'])
def test_fit_refuses_by_name(what):
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender.Baseline import SASRec
    ds = _dataset()
    kw = dict(epochs=1, batch_size=8)
    small = dict(hidden=4, L=LF, interaction_threshold=THR, verbose=False)
    if what.startswith('neg_ratio'):
        with pytest.raises(Exception, match='neg_ratio'):
            SASRec(**small).fit(ds, neg_ratio=int(what.split()[1]), **kw)
    elif what.startswith('hidden'):
        with pytest.raises(Exception, match='hidden'):
            SASRec(**dict(small, hidden=float(what.split()[1]) if '.' in what else int(what.split()[1]))).fit(ds, **kw)
    elif what.startswith('blocks'):
        with pytest.raises(Exception, match='blocks must'):
            SASRec(blocks=3, **small).fit(ds, **kw)
    elif what.startswith('L'):
        with pytest.raises(Exception, match=r'L must'):
            SASRec(**dict(small, L=17)).fit(ds, **kw)
    elif what == 'optimizer':
        # the base class's words
        with pytest.raises(Exception, match='SASRec trains with the dense rules adam, adagrad, sgd, rmsprop '
                                            r'\(dense update of both item tables and the attention weights\)'):
            SASRec(**small).fit(ds, optimizer='rowwise_adagrad', **kw)
    elif what == 'keras':
        class KerasLike:                                    # an optimizer object that is none of drecpy_amd.optimizers
            learning_rate = 1e-3
        with pytest.raises(Exception, match='Unsupported optimizer'):
            SASRec(**small).fit(ds, optimizer=KerasLike(), **kw)
        with pytest.raises(Exception, match='Unsupported optimizer'):
            SASRec(**small).fit(ds, optimizer='lion', **kw)
    else:
        # no user holds L + 1 = 4 records: no sequence to draw a window from
        short = InteractionDataset.from_arrays(np.array([0, 0, 1, 1, 1]), np.array([0, 1, 0, 1, 2]), np.full(5, 2.0), timestamp=np.arange(5))
        with pytest.raises(Exception, match='Failed to sample group records'):
            SASRec(**dict(small, L=3)).fit(short, **kw)
