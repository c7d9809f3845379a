"""BPR-MF on the device against tests/bpr_oracle.py (NumPy float64), through the C ABI (drx_bpr_sample, drx_bpr_step) and the public class
(drecpy_amd.Recommender.Baseline.BPR).

The gate is the project's: max error <= 1e-5 * max(1, max |x|) on the scores of ALL (user, item) pairs and on the loss.  The test
weights are uniform(-0.5, 0.5) / sqrt(K), so scores are O(0.1 - 1).  Rows no triple of a batch names are compared bit for bit with an
fp32 NumPy replay of their reg-only update (the kernels' operations, a * b + c fused or not)."""
import ctypes as C

import numpy as np
import pytest

import bpr_oracle as bo
from test_optim_oracle import _rule32

pytestmark = pytest.mark.gpu

U, N, THR = 37, 53, 1.0
F = np.float32
D = np.float64
GATE = 1e-5
EINVAL = -1


def _pairs():
    """(user, item, interaction) rows of a 37 x 53 frame, users and items in first-appearance order (internal id == raw id): user 0 records
    all 53 items, 1 has no positive (two low pairs), 2 records all items but 17, 3 has one pair below the threshold, the others 3 - 12
    pairs with values on both sides of it"""
    rng = np.random.default_rng(2024)
    pairs = [(0, i, 2.0) for i in range(N)]
    pairs += [(1, 4, 0.5), (1, 9, 0.25)]
    pairs += [(2, i, 1.0 + (i % 3)) for i in range(N) if i != 17]
    pairs += [(3, 30, 0.5)]
    for u in range(4, U):
        items = rng.choice(N, size=int(rng.integers(3, 13)), replace=False)
        pairs += [(u, int(i), float(rng.choice([0.5, 1.0, 2.0, 3.0]))) for i in items]
    return pairs


@pytest.fixture(scope='module')
def frame():
    f = bo.Frame(U, N, _pairs(), THR)
    assert 0 not in f.eligible and 1 not in f.eligible and 3 not in f.eligible and 2 in f.eligible and len(f.eligible) >= 30
    return f


def _dev(a, dtype):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to('cuda:0')


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def _gate(got, want, what):
    got, want = np.asarray(got, D), np.asarray(want, D)
    err, bound = float(np.max(np.abs(got - want))), GATE * max(1.0, float(np.max(np.abs(want))))
    print(f'{what}: max error {err:.3e} (gate {bound:.3e})')
    assert err <= bound, f'{what}: max error {err:.3e} > {bound:.3e}'


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------
def _device_frame(frame):
    from drecpy_amd._lib import History, ptr
    pos, rec = bo.Frame.csr(frame.positives), bo.Frame.csr(frame.recorded)
    keep = [_dev(pos[0], np.int64), _dev(pos[1], np.int32), _dev(rec[0], np.int64), _dev(rec[1], np.int32), _dev(frame.eligible, np.int32)]
    return History(ptr(keep[0]), ptr(keep[1])), History(ptr(keep[2]), ptr(keep[3])), keep[4], keep


@pytest.mark.parametrize('seed', [0, 0xFEDCBA9876543210])
@pytest.mark.parametrize('r', [1, 3])
def test_sampler_is_bit_equal_to_the_oracle(frame, r, seed):
    import torch
    from drecpy_amd._lib import check, lib, ptr
    H, R, elig, keep = _device_frame(frame)
    for T in (1, 63, 65, 257, 1000):
        out = torch.full((3, T), -7, dtype=torch.int32, device='cuda:0')
        check(lib().drx_bpr_sample(C.byref(H), C.byref(R), ptr(elig), elig.numel(), N, T, r, seed, ptr(out[0]), ptr(out[1]), ptr(out[2]), None),
              'drx_bpr_sample')
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        want = bo.sample(frame, T, r, seed)
        for g, w, name in zip(got, want, ('uid', 'pos', 'neg')):
            assert np.array_equal(g, w), f'{name} differs at T {T}, r {r}: first at {int(np.flatnonzero(g != w)[0])}'


def test_sampler_refusals(frame):
    import torch
    from drecpy_amd._lib import History, lib, ptr
    H, R, elig, keep = _device_frame(frame)
    out = torch.full((3, 8), -7, dtype=torch.int32, device='cuda:0')
    good = [C.byref(H), C.byref(R), ptr(elig), elig.numel(), N, 8, 2, 5, ptr(out[0]), ptr(out[1]), ptr(out[2]), None]
    bad = {'hist': (0, None), 'hist arrays': (0, C.byref(History(None, None))), 'recorded arrays': (1, C.byref(History(None, None))),
           'eligible': (2, None), 'n_eligible': (3, 0), 'n_items': (4, 0), 'T': (5, 0), 'neg_ratio 0': (6, 0), 'neg_ratio -1': (6, -1),
           'uid': (8, None), 'pos': (9, None), 'neg': (10, None)}
    for what, (at, value) in bad.items():
        args = list(good)
        args[at] = value
        assert lib().drx_bpr_sample(*args) == EINVAL, what
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all()
    assert lib().drx_bpr_sample(*good) == 0


# ---- the step --------------------------------------------------------------------------------------------------------------------------
USER_POOL = [2, 4, 5, 6, 8, 11, 12, 19, 20, 36]            # the batches' users: they repeat; the others are never looked up
ITEM_POOL = list(range(0, 40))                              # items 40 .. 52 are never looked up


def _batch(T, seed):
    """T triples in which users repeat, items 3 and 7 are each a positive in one triple and the negative in another (both rows collect
    both signs), and — from 257 triples on — item 7 is the negative of 100 triples (more lookups than the update's split threshold)"""
    rng = np.random.default_rng(seed)
    uid = rng.choice(USER_POOL, size=T)
    pos = rng.choice(ITEM_POOL, size=T)
    neg = (pos + 1 + rng.integers(0, len(ITEM_POOL) - 1, size=T)) % len(ITEM_POOL)
    if T >= 5:
        uid[:3], pos[:3], neg[:3] = [4, 4, 5], [3, 7, 3], [7, 3, 9]
    if T >= 257:
        at = rng.choice(np.arange(3, T), size=100, replace=False)
        neg[at] = 7
        pos[at] = np.where(pos[at] == 7, 8, pos[at])
    assert (pos != neg).all()
    return uid.astype(np.int32), pos.astype(np.int32), neg.astype(np.int32)


def _optimizer(kind, lr):
    from drecpy_amd import optimizers as op
    return {'adam': lambda: op.Adam(lr), 'adagrad': lambda: op.Adagrad(lr), 'sgd': lambda: op.SGD(lr), 'momentum': lambda: op.SGD(lr, bo.HP['mu']),
            'nesterov': lambda: op.SGD(lr, bo.HP['mu'], nesterov=True), 'rmsprop': lambda: op.RMSprop(lr, bo.HP['rho'])}[kind]()


def _engine(K, p, kind='adam'):
    from drecpy_amd.engine_bpr import BprEngine
    e = BprEngine(U, N, K)
    e.set_params(p)
    e.set_optimizer(_optimizer(kind, bo.HP['lr']))
    e.reg = bo.HP['reg']
    return e


def _padding_is_zero(e):
    """the padding columns of both tables, and of the slots that start at zero (Adagrad's accumulator starts at 0.1 in every column)"""
    slots = [] if e.opt_kind == 'adagrad' else [s for n in ('P', 'Q') for s in e.state[n] if s is not None]
    for t in [e.P, e.Q] + slots:
        assert not t[:, e.K:].cpu().numpy().any(), 'a padding column moved'


def _all_scores(e):
    return e.score_matrix(np.arange(U, dtype=np.int32)).cpu().numpy()


def _adam32(p, m, v, alpha, l2c, fused):
    """TF's ApplyAdam on gt = l2c p (no data gradient) in NumPy fp32; fused: every a * b + c rounds once"""
    alpha, l2c, eps = F(alpha), F(l2c), F(bo.HP['eps'])
    o1, o2 = F(1.0) - F(bo.HP['b1']), F(1.0) - F(bo.HP['b2'])
    fma = (lambda a, b, c: (a.astype(D) * b.astype(D) + c.astype(D)).astype(F)) if fused else (lambda a, b, c: a * b + c)
    gt = l2c * p
    m1 = fma(gt - m, np.full_like(p, o1), m)
    v1 = fma(fma(gt, gt, -v), np.full_like(p, o2), v)
    return p - (m1 * alpha) / (np.sqrt(v1) + eps), m1, v1


def _idle_replay(kind, p, l2c, alpha):
    """[(p, s1, s2) fused, (p, s1, s2) unfused]: one reg-only step of fp32 rows p from fresh slots"""
    n = 2 if kind == 'adam' else bo.oo.N_SLOTS[kind]
    init = F(0.1 if kind == 'adagrad' else 0.0)
    s1, s2 = (np.full_like(p, init) if s < n else None for s in range(2))
    if kind == 'adam':
        return [_adam32(p, s1, s2, alpha, l2c, fused) for fused in (True, False)]
    forms = [_rule32(kind, p, s1, s2, np.zeros_like(p), alpha, l2c, bo.HP['mu'], bo.HP['rho'], bo.HP['eps'], fused) for fused in (True, False)]
    if kind == 'nesterov':
        # a1 mu - gt lr has two fused forms: fma(a1, mu, -(gt lr)) (the replay's) and fma(-gt, lr, a1 mu)
        gt, a1, mu = F(l2c) * p, forms[0][1], F(bo.HP['mu'])
        forms.append((p + ((-gt).astype(D) * D(F(alpha)) + (a1 * mu).astype(D)).astype(F), a1, None))
    return forms


def _check_idle_rows(e, kind, p0, uid, pos, neg, alphas):
    """rows of P, Q and bq that no triple names: bit-equal to the fp32 replay of their reg-only update (parameters and slots)"""
    idle_u = np.setdiff1d(np.arange(U), uid)
    idle_i = np.setdiff1d(np.arange(N), np.concatenate([pos, neg]))
    assert len(idle_u) >= 20 and len(idle_i) >= 13
    for name, idle, l2c, alpha in (('P', idle_u, bo.HP['reg'], alphas[0]), ('Q', idle_i, bo.HP['reg'], alphas[1]), ('bq', idle_i, 0.0, alphas[1])):
        start = p0[name].astype(F)[idle]
        forms = _idle_replay(kind, start, l2c, alpha)
        got = [getattr(e, name)] + list(e.state[name])
        for k, what in enumerate(('p', 's1', 's2')):
            if forms[0][k] is None:
                continue
            g = got[k].cpu().numpy()
            g = (g[:, :e.K] if g.ndim == 2 else g)[idle]
            same = np.logical_or.reduce([_bits(g) == _bits(f[k]) for f in forms])
            assert same.all(), f'{kind} {name} {what}: {int((~same).sum())} idle elements differ from the fp32 replay, first {np.argwhere(~same)[0]}'
        if kind in ('adam', 'momentum', 'nesterov') and l2c:
            assert (_bits(got[0].cpu().numpy()[idle][..., :e.K]) != _bits(start)).any(), f'{kind} {name}: the reg-only update moved nothing'


@pytest.mark.parametrize('K', [1, 5, 64, 256])
@pytest.mark.parametrize('T', [1, 5, 64, 257])
def test_adam_steps_match_the_oracle_after_1_and_10_steps(T, K):
    p = bo.init_params(np.random.default_rng(100 + K), U, N, K)
    p0 = {k: v.copy() for k, v in p.items()}
    st = bo.init_state(p, 'adam')
    e = _engine(K, p)
    for s in range(10):
        uid, pos, neg = _batch(T, 1000 * T + s)
        want = bo.step(p, st, s, uid, pos, neg, 'adam')
        got = e.step(s, uid, pos, neg, want_loss=True)
        _gate(got, want, f'T {T} K {K} step {s} loss')
        if s in (0, 9):
            _gate(_all_scores(e), bo.scores(p), f'T {T} K {K} scores after {s + 1} step(s)')
            _padding_is_zero(e)
        if s == 0:
            _check_idle_rows(e, 'adam', p0, uid, pos, neg, e._step_sizes(0, (2, 0, 1)))
    for name in bo.NAMES:                                   # the slots too: Adam's m and v of every row
        for k in range(2):
            got = e.state[name][k].cpu().numpy()
            got = got[:, :K] if got.ndim == 2 else got
            scale = max(1e-30, float(np.max(np.abs(st[name][k]))))
            assert np.max(np.abs(got - st[name][k])) <= 1e-4 * scale, (name, k)


@pytest.mark.parametrize('K', [5, 64])
@pytest.mark.parametrize('kind', ['adam', 'adagrad', 'sgd', 'momentum', 'nesterov', 'rmsprop'])
def test_one_step_under_every_rule(kind, K):
    T = 64
    p = bo.init_params(np.random.default_rng(7 + K), U, N, K)
    p0 = {k: v.copy() for k, v in p.items()}
    st = bo.init_state(p, kind)
    e = _engine(K, p, kind)
    uid, pos, neg = _batch(T, 77)
    want = bo.step(p, st, 0, uid, pos, neg, kind)
    got = e.step(0, uid, pos, neg, want_loss=True)
    _gate(got, want, f'{kind} K {K} loss')
    _gate(_all_scores(e), bo.scores(p), f'{kind} K {K} scores')
    _padding_is_zero(e)
    _check_idle_rows(e, kind, p0, uid, pos, neg, e._step_sizes(0, (2, 0, 1)))
    n = 2 if kind == 'adam' else bo.oo.N_SLOTS[kind]
    assert [s is not None for s in e.state['Q']] == [k < n for k in range(2)]


def test_the_same_inputs_give_the_same_bits():
    K, T = 20, 257
    p = bo.init_params(np.random.default_rng(1), U, N, K)
    runs = []
    for _ in range(2):
        e = _engine(K, p)
        for s in range(3):
            e.step(s, *_batch(T, 5 + s))
        runs.append([t.cpu().numpy().copy() for t in (e.P, e.Q, e.bq)] + [x.cpu().numpy().copy() for n in bo.NAMES for x in e.state[n]])
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(*runs))
    assert not np.array_equal(runs[0][0][:, :K], p['P'].astype(F))


def test_step_refusals_leave_the_parameters_alone():
    import torch
    from drecpy_amd import _lib
    from drecpy_amd._lib import lib, ptr
    K, T = 8, 16
    p = bo.init_params(np.random.default_rng(2), U, N, K)
    e = _engine(K, p)
    uid, pos, neg = (_dev(a, np.int32) for a in _batch(T, 3))
    need = int(lib().drx_bpr_step_scratch_bytes(T, e.ld, U, N))
    assert need > 0
    for bad in ((0, e.ld, U, N), (-1, e.ld, U, N), (T, 0, U, N), (T, 6, U, N), (T, 260, U, N), (T, e.ld, 0, N), (T, e.ld, U, 0)):
        assert lib().drx_bpr_step_scratch_bytes(*bad) == 0, bad
    sc = torch.zeros(need, dtype=torch.uint8, device='cuda:0')
    alphas = (C.c_float * 3)(1e-2, 1e-2, 1e-2)
    slots = [ptr(s) for n in bo.NAMES for s in e.state[n]]                      # P m, P v, Q m, Q v, bq m, bq v
    adam, momentum = _lib.OptRule(0, 0.0, 0.9, 0.999, 1e-7), _lib.OptRule(4, 0.0, 0.9, 0.0, 0.0)
    rowwise, unknown = _lib.OptRule(2, 0.0, 0.0, 0.0, 1e-7), _lib.OptRule(99, 0.0, 0.0, 0.0, 0.0)
    good = [ptr(e.P), ptr(e.Q), ptr(e.bq)] + slots + [e.ld, U, N, ptr(uid), ptr(pos), ptr(neg), T, C.byref(adam), alphas, 1e-3, None, ptr(sc),
                                                      need, None]
    before = [t.cpu().numpy().copy() for t in (e.P, e.Q, e.bq)]
    bad = {'P': (0, None), 'Q': (1, None), 'bq': (2, None), 'uid': (12, None), 'pos': (13, None), 'neg': (14, None), 'rule': (16, None),
           'alphas': (17, None), 'scratch': (20, None), 'T 0': (15, 0), 'T -3': (15, -3), 'ld 0': (9, 0), 'ld 2': (9, 2), 'ld 6': (9, 6),
           'ld 260': (9, 260), 'n_users 0': (10, 0), 'n_items 0': (11, 0), 'adam without P m': (3, None), 'adam without Q v': (6, None),
           'adam without bq m': (7, None), 'momentum without Q s1': (5, None), 'row-wise adagrad': (16, C.byref(rowwise)),
           'an unknown rule': (16, C.byref(unknown)), 'a misaligned table': (1, C.c_void_p(e.Q.data_ptr() + 4))}
    for what, (at, value) in bad.items():
        args = list(good)
        args[at] = value
        if what.startswith('momentum'):
            args[16] = C.byref(momentum)
        assert lib().drx_bpr_step(*args) == EINVAL, what
    small = list(good)
    small[21] = need // 2
    assert lib().drx_bpr_step(*small) == -2                                      # DRX_ESCRATCH
    torch.cuda.synchronize()
    for t, b in zip((e.P, e.Q, e.bq), before):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(b))
    assert not sc.cpu().numpy().any(), 'a refused call wrote its scratch'
    assert lib().drx_bpr_step(*good) == 0                                        # momentum needs no second slot; the good call runs
    torch.cuda.synchronize()
    assert not np.array_equal(_bits(e.P.cpu().numpy()), _bits(before[0]))


def test_engine_refuses_factors_outside_its_domain():
    from drecpy_amd._lib import DrxError
    from drecpy_amd.engine_bpr import BprEngine
    for K in (0, 257, 2.5):
        with pytest.raises(DrxError, match='factors'):
            BprEngine(U, N, K)


# ---- the public class ------------------------------------------------------------------------------------------------------------------
def _dataset():
    from drecpy_amd.Dataset import InteractionDataset
    u, i, v = (np.array(c) for c in zip(*_pairs()))
    return InteractionDataset.from_arrays(u.astype(np.int64), i.astype(np.int64), v.astype(np.float64))


FIT = dict(epochs=20, batch_size=64, learning_rate=1e-2, neg_ratio=3, reg_rate=1e-3)


@pytest.fixture(scope='module')
def fitted(frame):
    """(model, oracle parameters) after the same 20 steps on the same draws"""
    from drecpy_amd.Recommender.Baseline import BPR
    K = 10
    w = bo.init_params(np.random.default_rng(42), U, N, K)
    model = BPR(factors=K, seed=3, interaction_threshold=THR, verbose=False)
    model.fit(_dataset(), initial_weights=w, **FIT)
    ds = model.interaction_dataset
    assert all(ds.user_to_uid(u) == u for u in range(U)) and all(ds.item_to_iid(i) == i for i in range(N))
    p = {k: v.copy() for k, v in w.items()}
    st = bo.init_state(p, 'adam')
    for s in range(FIT['epochs']):
        bo.step(p, st, s, *bo.sample(frame, FIT['batch_size'], FIT['neg_ratio'], model._draw_seed(s + 1)), 'adam')
    return model, p


def test_fit_equals_the_oracle_fit_on_the_same_draws(fitted):
    model, p = fitted
    x = bo.scores(p)
    _gate(_all_scores(model._engine), x, 'scores after fit(epochs=20)')
    _padding_is_zero(model._engine)
    assert model.predict(5, 7) == pytest.approx(x[5, 7], abs=GATE)
    assert isinstance(model.predict(5, 7), float)


def test_recommend_batch_equals_recommend_and_the_oracle_order(fitted):
    model, p = fitted
    x = bo.scores(p)
    users = [0, 1, 2, 3, 5, 17, 36, 5]
    for novelty in (True, False):
        lists = model.recommend_batch(users, n=10, novelty=novelty)
        for u, got in zip(users, lists):
            one = model.recommend(u, n=10, novelty=novelty)
            assert [i for _, i in got] == [i for _, i in one], (u, novelty)
            assert np.allclose([s for s, _ in got], [s for s, _ in one], rtol=0, atol=GATE)
            allowed = [i for i in range(N) if not (novelty and i in model._recorded_items(u))]
            assert len(got) == min(10, len(allowed)) and all(i in allowed for _, i in got)
            if not got:
                continue
            _gate([s for s, _ in got], [x[u, i] for _, i in got], f'user {u} values')
            # the oracle's order wherever its scores differ by more than the gate
            for (_, a), (_, b) in zip(got, got[1:]):
                assert x[u, a] >= x[u, b] - 2 * GATE, (u, a, b)
            best = sorted(allowed, key=lambda i: -x[u, i])[:len(got)]
            if len(best) and (len(allowed) == len(got) or x[u, best[-1]] - max([x[u, i] for i in allowed if i not in best], default=-np.inf) > 2 * GATE):
                assert sorted(best) == sorted(i for _, i in got), (u, novelty)
    assert model.recommend_batch([0], n=5, novelty=True) == [[]]                 # user 0 records the whole catalogue


def test_catalogue_ranks_are_positions_in_the_full_list(fitted):
    model, _ = fitted
    # scattered pairs (one catalogue walk per pair), then many pairs of two users (the list form: one walk per user)
    requests = (([2, 5, 5, 17, 36, 36, 36, 1], [17, 0, 52, 30, 1, 2, 3, 4]), ([5] * 9 + [36] * 9, [(5 * k) % N for k in range(18)]))
    for (users, items), novelty in ((r, nov) for r in requests for nov in (True, False)):
        ranks, scores = model.catalogue_ranks(users, items, novelty=novelty, return_scores=True)
        full = {u: model.recommend_batch([u], n=N, novelty=novelty)[0] for u in set(users)}
        for u, i, r, s in zip(users, items, ranks, scores):
            place = {item: (j, v) for j, (v, item) in enumerate(full[u])}
            if i in place:
                assert r == place[i][0] and s == pytest.approx(place[i][1], abs=GATE), (u, i, novelty)
            else:
                assert r == -1 and s == -np.inf, (u, i, novelty)
    assert model.catalogue_ranks([2], [17], novelty=True)[0] == 0                 # the only item user 2 has not recorded


def test_predict_pairs_equals_predict(fitted):
    model, p = fitted
    rng = np.random.default_rng(8)
    users, items = rng.integers(0, U, size=200), rng.integers(0, N, size=200)
    got = model.predict_pairs(users.tolist(), items.tolist())
    assert got.dtype == np.float64
    assert np.array_equal(got, np.array([model.predict(int(u), int(i)) for u, i in zip(users, items)]))
    _gate(got, bo.scores(p)[users, items], 'predict_pairs')
    assert np.isnan(model.predict_pairs([1, 999], [1, 1], skip_errors=True)[1])


def test_evaluations_batched_and_not(fitted):
    from drecpy_amd.Evaluation import ranking_evaluation, recommendation_evaluation
    model, _ = fitted
    kw = dict(n_pos_interactions=3, n_neg_interactions=10, generate_negative_pairs=True, k=[1, 5], seed=4, verbose=False)
    a = ranking_evaluation(model, batched=True, **kw)
    b = ranking_evaluation(model, batched=False, **kw)
    assert a == b and a and any(v > 0 for v in a.values()), (a, b)
    r = [recommendation_evaluation(model, _dataset(), k=[1, 5], novelty=False, seed=4, verbose=False, batched=batched)
         for batched in (False, True, 'ranks')]
    assert r[0] == r[1] == r[2] and r[0] and any(v > 0 for v in r[0].values()), r


def test_save_and_load_predict_identically(fitted, tmp_path):
    from drecpy_amd.Recommender.Baseline import BPR
    model, _ = fitted
    path = str(tmp_path / 'bpr.pkl')
    model.save(path)
    other = BPR.load(path)
    assert isinstance(other, BPR)
    users, items = list(range(U)) * 2, [(7 * k) % N for k in range(2 * U)]
    assert np.array_equal(other.predict_pairs(users, items), model.predict_pairs(users, items))
    assert other.recommend_batch([5, 36], n=7) == model.recommend_batch([5, 36], n=7)
    assert other.recommend(5, n=7) == model.recommend(5, n=7)


def test_callbacks_early_stopping_and_loss(frame):
    from drecpy_amd.Recommender.Baseline import BPR
    from drecpy_amd.Recommender.early_stopping import MaxValidationValueRule
    K = 6
    w = bo.init_params(np.random.default_rng(9), U, N, K)
    seen = []
    model = BPR(factors=K, seed=1, interaction_threshold=THR, verbose=False)
    model.fit(_dataset(), epochs=6, batch_size=32, learning_rate=1e-2, neg_ratio=2, reg_rate=1e-3, initial_weights=w,
              epoch_callback_fn=lambda m: seen.append(float(m.predict(5, 7))) or {'score': -len(seen)}, epoch_callback_freq=2,
              early_stopping_rule=MaxValidationValueRule('score'), early_stopping_freq=2)
    assert len(seen) >= 1 and model.fitted
    # the best epoch is the first one evaluated (the score falls): the weights are those of epoch 2
    p = {k: v.copy() for k, v in w.items()}
    st = bo.init_state(p, 'adam')
    for s in range(2):
        bo.step(p, st, s, *bo.sample(frame, 32, 2, model._draw_seed(s + 1)), 'adam')
    _gate(_all_scores(model._engine), bo.scores(p), 'scores after the revert to epoch 2')


@pytest.mark.parametrize('what', ['neg_ratio', 'K 0', 'K 257', 'no eligible user', 'optimizer'])
def test_fit_refuses_by_name(what):
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender.Baseline import BPR
    ds = _dataset()
    kw = dict(epochs=1, batch_size=8)
    if what == 'neg_ratio':
        with pytest.raises(Exception, match='neg_ratio'):
            BPR(factors=4, interaction_threshold=THR, verbose=False).fit(ds, neg_ratio=0, **kw)
    elif what.startswith('K'):
        with pytest.raises(Exception, match='factors'):
            BPR(factors=int(what[2:]), interaction_threshold=THR, verbose=False).fit(ds, **kw)
    elif what == 'optimizer':
        with pytest.raises(Exception, match='dense rules'):
            BPR(factors=4, interaction_threshold=THR, verbose=False).fit(ds, optimizer='rowwise_adagrad', **kw)
    else:
        # every user either has no positive or records the whole catalogue
        full = InteractionDataset.from_arrays(np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1]), np.array([2.0, 2.0, 0.5, 0.25]))
        with pytest.raises(Exception, match='eligible'):
            BPR(factors=4, interaction_threshold=THR, verbose=False).fit(full, **kw)
