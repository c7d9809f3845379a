"""Scores of given (query row, table row) pairs: drx_rows_pair_scores (k_pair_scores), the engines' pair_scores,
RecommenderABC.predict_pairs and predictive_evaluation.  Nothing here reads the reference.

  1. integer problems (the construction of tests/test_gpu_rank_items.py: table in {-1, 0, 1}, six +-1 per query row, integer biases):
     every sum is an integer in [-8, 8] whatever the summation order, so the biased sum and the clipped sum are expected EXACTLY; the
     sigmoid of an integer z is expected within 2e-6 relative of the fp64 one (expf to 1e-6 relative — rec_logit_bound's assumption
     in drx_recommend.hip —, then one fp32 addition and one division, 6e-8 each) and bit-equal between pairs of equal z;
  2. float problems, the contract: for ld <= 256 the value equals the out_score of drx_rows_rank_items for the same rows, exactly;
  3. float problems against fp64 numpy at every ld, 260 (beyond the matrix-core scorers) included: sigmoid and clip within the project's
     1e-5 relative, logits within the bound of a length-ld fp32 chain, (ld + 2) 2^-24 (sum |q_k t_k| + |b|).  The clip problems hold
     cosines of about +-0.64 (entries of one sign): at the floor a score is 1e-6 on both sides, above it the relative error is that of
     the chain, about sqrt(ld) 2^-24 in the typical case, 1.6e-5 only in the worst one no random problem meets;
  4. reproducibility; 5. the engines against their rank_items; 6. the public layer on fitted models; 7. predictive_evaluation.
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIGMOID_BIAS, BIAS, CLIP = 0, 1, 2
FLOOR = np.float32(1e-6)
DRX_EINVAL = -1
LDS = (4, 12, 52, 128, 256, 260)


def _dev(a, dtype):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to('cuda:0')


def _pair_call(table, bias, ld, epilogue, q, q_row, t_row, room=0):
    """(return code, out float32 [P + room] pre-filled with the sentinel 7.0) of one direct call"""
    import torch
    from drecpy_amd import _lib
    L = _lib.lib()
    P = len(q_row)
    d_table, d_q = _dev(table, np.float32), _dev(q, np.float32)
    d_bias = None if bias is None else _dev(bias, np.float32)
    d_qr, d_tr = _dev(q_row, np.int32), _dev(t_row, np.int32)
    out = torch.full((P + room,), 7.0, dtype=torch.float32, device='cuda:0')
    rc = L.drx_rows_pair_scores(_lib.ptr(d_table), _lib.ptr(d_bias), table.shape[0], ld, epilogue, _lib.ptr(d_q),
                                q.shape[0], _lib.ptr(d_qr), _lib.ptr(d_tr), P, _lib.ptr(out),
                                _lib.stream_ptr(torch.device('cuda:0')))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _k_of(ld):
    return {52: 50, 12: 10}.get(ld, ld)


# ---- 1. exact integer problems --------------------------------------------------------------------------------------------------------
def _integer_parts(rng, N, U, ld, with_bias):
    from test_gpu_rank_items import _integer_parts as parts
    K = _k_of(ld)
    if K >= 6:
        return parts(rng, N, U, K, ld, with_bias)
    table = rng.integers(-1, 2, (N, ld)).astype(np.float32)            # ld = 4: every column takes a +-1
    q = rng.choice([-1.0, 1.0], (U, ld)).astype(np.float32)
    return table, (rng.integers(-2, 3, N).astype(np.float32) if with_bias else None), q


def _sigmoid64(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


@pytest.mark.parametrize('ld', LDS)
def test_integer_problems(ld):
    U = 9
    for n_rows in (1, 127, 300):
        for epilogue in (SIGMOID_BIAS, BIAS, CLIP):
            rng = np.random.default_rng(ld * 1000 + n_rows * 3 + epilogue)
            table, bias, q = _integer_parts(rng, n_rows, U, ld, epilogue != CLIP)
            z = q.astype(np.float64) @ table.astype(np.float64).T + (0 if bias is None else bias.astype(np.float64))
            assert (z == np.rint(z)).all() and np.abs(z).max() <= 8
            for P in (1, 63, 64, 65, 1000):
                q_row = np.sort(rng.integers(0, U, P)) if P == 65 else rng.integers(0, U, P)      # repeated; sorted or permuted
                t_row = rng.integers(0, n_rows, P)
                rc, out = _pair_call(table, bias, ld, epilogue, q, q_row, t_row, room=70)
                assert rc == 0
                assert (out[P:] == 7.0).all(), (ld, n_rows, epilogue, P)                         # nothing is written from slot P on
                zp = z[q_row, t_row]
                if epilogue == BIAS:
                    assert np.array_equal(out[:P], zp.astype(np.float32)), (ld, n_rows, P)
                elif epilogue == CLIP:
                    assert np.array_equal(out[:P], np.maximum(FLOOR, zp.astype(np.float32))), (ld, n_rows, P)
                else:
                    want = _sigmoid64(zp)
                    assert (np.abs(out[:P] - want) <= 2e-6 * want).all(), (ld, n_rows, P)
                    for v in np.unique(zp):
                        assert len(np.unique(out[:P][zp == v])) == 1


def test_rows_out_of_range_empty_calls_and_argument_errors():
    rng = np.random.default_rng(2)
    n_rows, U, ld = 127, 9, 52
    for epilogue in (SIGMOID_BIAS, BIAS, CLIP):
        table, bias, q = _integer_parts(rng, n_rows, U, ld, epilogue != CLIP)
        q_row = np.array([0, -1, U, 3, 8, 2_000_000_000, 4, 5, -2_147_483_648, 8], np.int64)
        t_row = np.array([-1, 5, 7, n_rows, 126, 3, 2_000_000_000, -2_147_483_648, 0, 0], np.int64)
        rc, out = _pair_call(table, bias, ld, epilogue, q, q_row, t_row, room=3)
        assert rc == 0 and np.isneginf(out[[0, 1, 2, 3, 5, 6, 7, 8]]).all() and np.isfinite(out[[4, 9]]).all() and (out[10:] == 7.0).all()
        rc, out = _pair_call(table, bias, ld, epilogue, q, q_row[:0], t_row[:0], room=4)            # P = 0: OK, nothing written
        assert rc == 0 and (out == 7.0).all()
    table, bias, q = _integer_parts(rng, n_rows, U, ld, True)
    one = np.zeros(1, np.int64)
    for bad in (dict(ld=6), dict(ld=0), dict(epilogue=3), dict(epilogue=CLIP), dict(bias=None), dict(bias=None, epilogue=BIAS)):
        kw = dict(table=table, bias=bias, ld=ld, epilogue=SIGMOID_BIAS, q=q, q_row=one, t_row=one, room=1)
        kw.update(bad)
        rc, out = _pair_call(**kw)
        assert rc == DRX_EINVAL and (out == 7.0).all(), bad


def test_a_zero_score_is_written_as_plus_zero():
    """a product below the smallest denormal leaves the chain at -0.0; with a bias of -0.0 the biased sum is -0.0: the score written is
    +0.0, the value drx_rows_rank_items reports through its key"""
    ld = 12
    table, q = np.zeros((3, ld), np.float32), np.zeros((2, ld), np.float32)
    table[1, 0], q[1, 0] = -1e-30, 1e-30
    bias = np.array([-0.0, -0.0, 1.0], np.float32)
    q_row, t_row = np.array([1, 0, 1]), np.array([1, 1, 2])
    rc, out = _pair_call(table, bias, ld, BIAS, q, q_row, t_row)
    assert rc == 0 and out.tolist() == [0.0, 0.0, 1.0] and not np.signbit(out).any()
    assert np.array_equal(out.view(np.uint32), _rank_items_scores(table, bias, ld, BIAS, q, q_row, t_row).view(np.uint32))


# ---- 2 / 3. float problems ------------------------------------------------------------------------------------------------------------
N_ROWS, N_Q, N_PAIRS = 300, 40, 500


@functools.lru_cache(maxsize=None)
def _float_problem(ld, epilogue, near_zero):
    """(table, bias, q, q_row, t_row): negative logits, sigmoid saturation on both sides (biases of +-20), scores at DMF's floor;
    near_zero (the contract only): clip rows of random signs too, cosines around 0 on either side of the floor"""
    rng = np.random.default_rng(ld * 10 + epilogue)
    K = _k_of(ld)
    table, q = np.zeros((N_ROWS, ld), np.float32), np.zeros((N_Q, ld), np.float32)
    if epilogue == CLIP:
        table[:, :K] = np.abs(rng.normal(0, 1, (N_ROWS, K)))
        q[:, :K] = np.abs(rng.normal(0, 1, (N_Q, K)))
        q[N_Q // 2:] *= -1                                             # half the query rows: every cosine below the floor
        if near_zero:
            table[::3, :K] = rng.normal(0, 1, (len(table[::3]), K))
        table /= np.linalg.norm(table, axis=1, keepdims=True)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        bias = None
    else:
        table[:, :K] = rng.normal(0, 2.0 / np.sqrt(K), (N_ROWS, K))
        q[:, :K] = rng.normal(0, 0.5, (N_Q, K))
        bias = rng.normal(0, 0.3, N_ROWS).astype(np.float32)
        if epilogue == SIGMOID_BIAS:
            bias[rng.choice(N_ROWS, 40, replace=False)] = np.repeat([20.0, -20.0], 20)
    q_row, t_row = rng.integers(0, N_Q, N_PAIRS), rng.integers(0, N_ROWS, N_PAIRS)
    return table, bias, q, q_row, t_row


def _rank_items_scores(table, bias, ld, epilogue, q, q_row, t_row):
    """out_score of drx_rows_rank_items, called directly on the gathered rows"""
    import torch
    from drecpy_amd import _lib
    L = _lib.lib()
    P, N = len(q_row), table.shape[0]
    d_table, d_q = _dev(table, np.float32), _dev(q[q_row], np.float32)
    d_bias = None if bias is None else _dev(bias, np.float32)
    d_t = _dev(t_row, np.int32)
    out_rank = torch.empty(P, dtype=torch.int32, device='cuda:0')
    out_score = torch.empty(P, dtype=torch.float32, device='cuda:0')
    sb = int(L.drx_rows_rank_items_scratch_bytes(P, N, ld))
    assert sb > 0
    sc = torch.empty(sb, dtype=torch.uint8, device='cuda:0')
    _lib.check(L.drx_rows_rank_items(_lib.ptr(d_table), _lib.ptr(d_bias), N, ld, epilogue, _lib.ptr(d_q), None, _lib.ptr(d_t), P, None, None,
                                     _lib.ptr(out_rank), _lib.ptr(out_score), _lib.ptr(sc), sb, _lib.stream_ptr(torch.device('cuda:0'))),
               'drx_rows_rank_items')
    return out_score.cpu().numpy()


@pytest.mark.parametrize('epilogue', [SIGMOID_BIAS, BIAS, CLIP])
@pytest.mark.parametrize('ld', [12, 52, 64, 128, 256])
def test_a_pairs_score_is_rank_items_score(ld, epilogue):
    """the contract: one serving arithmetic"""
    table, bias, q, q_row, t_row = _float_problem(ld, epilogue, True)
    rc, got = _pair_call(table, bias, ld, epilogue, q, q_row, t_row)
    assert rc == 0
    want = _rank_items_scores(table, bias, ld, epilogue, q, q_row, t_row)
    differ = np.flatnonzero(got != want)
    print(f'ld {ld} epilogue {epilogue}: {len(differ)} of {len(got)} pairs differ',
          [(float(got[j]), float(want[j])) for j in differ[:5]])
    assert np.array_equal(got, want)
    if epilogue == SIGMOID_BIAS:
        assert (got == 1.0).sum() > 10 and (got < 1e-6).sum() > 10     # saturated on both sides
    elif epilogue == BIAS:
        assert (got < 0).sum() > 100
    else:
        assert (got == FLOOR).sum() > 100 and (got > FLOOR).sum() > 100


@pytest.mark.parametrize('epilogue', [SIGMOID_BIAS, BIAS, CLIP])
@pytest.mark.parametrize('ld', LDS)
def test_against_fp64_numpy(ld, epilogue):
    table, bias, q, q_row, t_row = _float_problem(ld, epilogue, False)
    rc, got = _pair_call(table, bias, ld, epilogue, q, q_row, t_row)
    assert rc == 0
    a, b = q.astype(np.float64)[q_row], table.astype(np.float64)[t_row]
    bp = np.zeros(len(q_row)) if bias is None else bias.astype(np.float64)[t_row]
    z = (a * b).sum(axis=1) + bp
    if epilogue == BIAS:
        bound = (ld + 2) * 2.0 ** -24 * (np.abs(a * b).sum(axis=1) + np.abs(bp))
        print(f'ld {ld} logits: largest error / bound {float((np.abs(got - z) / bound).max()):.3f}')
        assert (np.abs(got - z) <= bound).all()
    else:
        want = _sigmoid64(z) if epilogue == SIGMOID_BIAS else np.maximum(1e-6, z)
        rel = np.abs(got - want) / want
        print(f'ld {ld} epilogue {epilogue}: largest relative error {float(rel.max()):.3g}')
        assert (rel <= 1e-5).all()


# ---- 4. reproducibility (through an engine: its chunked launch) -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cdae_engine(K=50):
    from test_gpu_rank_items import _cdae_engine as make
    return make(U=90, N=6000, K=K)


def test_bit_identical_between_calls_orders_and_chunkings():
    import torch
    eng = _cdae_engine()
    rng = np.random.default_rng(5)
    P = 300
    uid, items = rng.integers(0, 90, P).astype(np.int32), rng.integers(0, 6000, P).astype(np.int32)
    a = eng.pair_scores(uid, items)
    assert a.dtype == torch.float32 and tuple(a.shape) == (P,) and torch.isfinite(a).all()
    assert torch.equal(a, eng.pair_scores(uid, items))
    perm = rng.permutation(P)
    inv = torch.as_tensor(np.argsort(perm)).to(eng.device)
    for chunk in (7, 64, None):
        assert torch.equal(a, eng.pair_scores(uid[perm], items[perm], chunk_pairs=chunk)[inv]), chunk
        assert torch.equal(a, eng.pair_scores(uid, items, chunk_pairs=chunk)), chunk
    assert eng.pair_scores(np.zeros(0, np.int32), np.zeros(0, np.int32)).numel() == 0


# ---- 5. the engines: pair_scores is rank_items' score -----------------------------------------------------------------------------------
def test_cdae_engine_and_rows_wider_than_256_floats():
    import torch
    eng = _cdae_engine()
    rng = np.random.default_rng(6)
    uid = np.sort(rng.integers(0, 90, 400)).astype(np.int32)
    items = rng.integers(0, 6000, 400).astype(np.int32)
    items[:3] = [-1, 6000, 5999]
    got = eng.pair_scores(uid, items)
    _, want = eng.rank_items(uid, items, exclude=False)
    assert torch.equal(got, want) and torch.isneginf(got[:2]).all() and torch.isfinite(got[2:]).all()
    wide = _cdae_engine(K=300)                                        # outside the matrix-core scorers' domain: answered all the same
    assert wide.ld == 300 and not wide.rank_is_fused(wide.ld)
    got = wide.pair_scores(uid[3:], items[3:]).cpu().numpy()
    _, pred = wide.forward(np.arange(90, dtype=np.int32))
    want = pred.cpu().numpy().astype(np.float64)[uid[3:], items[3:]]
    assert (np.abs(got - want) <= 1e-5 * want).all()


def test_dmf_engine_runs_the_item_tower_on_the_distinct_items_only(monkeypatch):
    import torch
    import test_gpu_recommend_models as tm
    from drecpy_amd import _lib
    rng = np.random.default_rng(9)
    U, N, factors = 120, 400, (64, 32)
    dense = tm._dmf_dense(rng, U, N, 20, 60)
    eng = tm._dmf_engine(tm._dmf_spread(rng, U, N, factors), dense, factors, None)
    uid = rng.integers(0, U, 500).astype(np.int32)
    items = rng.choice(rng.choice(N, 37, replace=False), 500).astype(np.int32)
    items[:2] = [-3, N]
    _, want = eng.rank_items(uid, items, exclude=False)
    L, sizes = _lib.lib(), []
    orig = L.drx_dmf_predict

    def counted(D, A, stream):
        sizes.append(int(A._obj.B))
        return orig(D, A, stream)
    monkeypatch.setattr(L, 'drx_dmf_predict', counted)
    got = eng.pair_scores(uid, items)
    n_items, n_users = len(np.unique(items[2:])), len(np.unique(uid))
    assert sizes == [n_items, n_users] and n_items <= 37               # each tower once, over the distinct ids of the call
    assert torch.equal(got, want) and torch.isneginf(got[:2]).all()
    assert (got == float(FLOOR)).sum() + (got > float(FLOOR)).sum() == 498
    sizes.clear()
    assert torch.equal(eng.pair_scores(uid, items, chunk_pairs=64), want)
    assert sizes[0] == n_items and len(sizes) == 1 + (500 + 63) // 64
    assert torch.isneginf(eng.pair_scores(uid[:2], items[:2])).all()   # no item of the catalogue at all


def test_caser_engine():
    import torch
    import test_gpu_recommend_models as tm
    rng = np.random.default_rng(10)
    U, N, L, d = 50, 700, 5, 50
    eng = tm._caser_engine(tm._caser_spread(rng, U, N, L, d), U, N, L, d, None)
    P = 300
    uid, before = rng.integers(0, U, P).astype(np.int32), rng.integers(0, N, (P, L)).astype(np.int32)
    items = rng.integers(0, N, P).astype(np.int32)
    items[0] = N
    got = eng.pair_scores(uid, before, items)
    _, want = eng.rank_items(uid, before, items, exclude=False)
    assert torch.equal(got, want) and torch.isneginf(got[0]) and (got[1:] < 0).any() and (got[1:] > 0).any()      # logits
    assert torch.equal(eng.pair_scores(uid, before, items, chunk_pairs=33), want)


# ---- 6. the public layer on fitted models ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fitted(kind):
    from test_gpu_rank_items import _fitted as fitted
    return fitted(kind)


def _modified_dmf():
    import test_gpu_recommend_models as tm
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    try:
        from extending_recommender_dmf import ModifiedDMF
    finally:
        sys.path.pop(0)
    return tm._fitted('dmf', cls=ModifiedDMF, epochs=2)[0]


def _count_predict(monkeypatch, cls):
    calls, orig = [], cls._predict

    def counted(model, uid, iid, **kwds):
        calls.append((int(uid), int(iid)))
        return orig(model, uid, iid, **kwds)
    monkeypatch.setattr(cls, '_predict', counted)
    return calls


@pytest.mark.parametrize('kind', ['cdae', 'cdae_sampled', 'dmf'])
def test_predict_pairs_on_a_fitted_model(kind):
    model, frame = _fitted(kind)
    rng = np.random.default_rng(12)
    raw_users = [int(u) for u in rng.permutation(np.arange(1000, 1060))[:20]]
    users = [u for u in raw_users for _ in range(40)]
    items = [70000 + int(i) for _ in raw_users for i in rng.choice(600, size=40, replace=False)]
    got = model.predict_pairs(users, items)
    assert got.dtype == np.float64 and got.shape == (800,) and np.isfinite(got).all()
    # one serving arithmetic: the value recommend_batch lists for the item, wherever it lists it
    place = [{item: s for s, item in a} for a in model.recommend_batch(raw_users, n=128, novelty=False)]
    listed = 0
    for u, i, v in zip(users, items, got.tolist()):
        s = place[raw_users.index(u)].get(i)
        if s is not None:
            assert v == s, (u, i, v, s)
            listed += 1
    assert listed > 100
    own = np.array([model.predict(u, i) for u, i in zip(users, items)], np.float64)
    rel = np.abs(got - own) / np.abs(own)
    print(f'{kind}: largest relative difference to predict() {float(rel.max()):.3g}')
    assert (rel <= 1e-5).all()
    perm = rng.permutation(800)
    assert np.array_equal(model.predict_pairs([users[j] for j in perm], [items[j] for j in perm]), got[perm])
    assert model.predict_pairs([], []).shape == (0,)
    # an unknown user or item: predict's message, or NaN
    with pytest.raises(AssertionError, match='User 5 was not found.'):
        model.predict_pairs([raw_users[0], 5], [70000, 70001])
    with pytest.raises(AssertionError, match='Item 5 was not found.'):
        model.predict_pairs([raw_users[0], raw_users[1]], [70000, 5])
    some = model.predict_pairs([raw_users[0], 5, raw_users[1], raw_users[2]], [70000, 70001, 5, 70002], skip_errors=True)
    assert np.isnan(some).tolist() == [False, True, True, False]
    assert some[0] == model.predict_pairs([raw_users[0]], [70000])[0] and some[3] == model.predict_pairs([raw_users[2]], [70002])[0]


def test_the_default_hook_answers_a_dmf_subclass_and_caser(monkeypatch):
    modified = _modified_dmf()
    calls = _count_predict(monkeypatch, type(modified))
    users, items = [1002, 1017, 1002, 1040, 1017], [70010, 70011, 70012, 70013, 70400]
    got = modified.predict_pairs(users, items)
    ds = modified.interaction_dataset
    assert calls == [(ds.user_to_uid(u), ds.item_to_iid(i)) for u, i in zip(users, items)]
    assert got.tolist() == [modified.predict(u, i) for u, i in zip(users, items)]
    import test_gpu_recommend_models as tm
    caser, _ = tm._fitted('caser', epochs=1)
    with pytest.raises(NotImplementedError):
        caser.predict_pairs(users, items)
    assert np.isnan(caser.predict_pairs(users, items, skip_errors=True)).all()


# ---- 7. predictive_evaluation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['cdae', 'dmf'])
def test_predictive_evaluation_on_a_fitted_model(kind, monkeypatch):
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Evaluation import MAE, MSE, RMSE, predictive_evaluation
    model, frame = _fitted(kind)
    rng = np.random.default_rng(14)
    tu = [int(u) for u in rng.integers(1000, 1060, 60)]
    ti = [70000 + int(i) for i in rng.integers(0, 600, 60)]
    ti[7], ti[31] = 5, 5                                               # an item the model has never seen
    tv = [int(v) for v in rng.integers(1, 6, 60)]
    ds_te = InteractionDataset.read_df({'user': np.array(tu), 'item': np.array(ti), 'interaction': np.array(tv)}, verbose=False)
    metrics = [RMSE(), MSE(), MAE()]
    own = [model.predict(u, i, skip_errors=True) for u, i in zip(tu, ti)]
    # (CDAE's _predict answers an unknown item — iid None — with the user's whole row, as the reference's does: no point prediction)
    own = [None if v is None or np.ndim(v) else v for v in own]
    assert [j for j, v in enumerate(own) if v is None] == [7, 31]
    for kw in (dict(), dict(count_none_predictions=True), dict(n_test_predictions=30), dict(n_test_predictions=30, count_none_predictions=True)):
        n = kw.get('n_test_predictions', 60)
        pairs = [(t, 0.0 if p is None else p) for t, p in zip(tv, own) if p is not None or kw.get('count_none_predictions')][:n]
        want = {m.name: round(m([t for t, _ in pairs], [p for _, p in pairs]), 4) for m in metrics}
        loop = predictive_evaluation(model, ds_te, metrics=metrics, verbose=False, batched=False, **kw)
        calls = _count_predict(monkeypatch, type(model))
        fused = predictive_evaluation(model, ds_te, metrics=metrics, verbose=False, **kw)
        monkeypatch.undo()
        assert calls == []                                            # the batched run: no per-pair prediction
        assert loop == want and set(fused) == set(want) == {'RMSE', 'MSE', 'MAE'}
        for name in want:
            assert abs(fused[name] - loop[name]) <= 1e-4, (kw, name, fused, loop)
    with pytest.raises(AssertionError, match='Item 5 was not found.'):
        predictive_evaluation(model, ds_te, verbose=False, skip_errors=False)
    assert set(predictive_evaluation(model, ds_te, verbose=False, skip_errors=False, n_test_predictions=7)) == {'RMSE', 'MSE'}
