"""FPMC on the device against tests/fpmc_oracle.py (NumPy float64), through the C ABI (drx_fpmc_step, drx_fpmc_query_rows) and the public
class (drecpy_amd.Recommender.Baseline.FPMC).

The gate on ALL scores (every user's serving basket x every item) and on the loss is

    err(GPU) <= max(1e-5, 4 err(replay)) * max(1, max |x|)

where the replay is the oracle itself on float32 arrays (gradients formed in float32, every stored value rounded to float32) — the form
of ALS's gate with the floor of BPR's.  Every (GPU, replay) pair is printed (pytest -s); DESIGN.md section 3.9 has the table.  The test
weights are uniform(-0.5, 0.5) / sqrt(K), so scores are O(0.1 - 1).  Rows no window of a batch names are compared bit for bit with an
fp32 NumPy replay of their reg-only update."""
import ctypes as C

import numpy as np
import pytest

import bpr_oracle as bo
import fpmc_oracle as fo
from oracle.data_oracle import list_sample_counter
from test_gpu_bpr import _bits, _dev, _idle_replay, _optimizer

pytestmark = pytest.mark.gpu

U, N, THR = 23, 41, 1.0
F = np.float32
D = np.float64
EINVAL = -1
MAX_R = 16                                                  # the largest neg_ratio drx_fpmc_step accepts


def _gate(what, got, want, replay):
    got, want, replay = (np.asarray(a, D) for a in (got, want, replay))
    scale = max(1.0, float(np.max(np.abs(want))))
    gpu, rep = float(np.max(np.abs(got - want))), float(np.max(np.abs(replay - want)))
    bound = max(1e-5, 4.0 * rep) * scale
    print(f'{what}: GPU error {gpu:.3e}, replay error {rep:.3e} (gate {bound:.3e})')
    assert gpu <= bound, f'{what}: GPU error {gpu:.3e} > {bound:.3e} (replay {rep:.3e})'


# ---- the step --------------------------------------------------------------------------------------------------------------------------
USER_POOL = [1, 2, 4, 5, 8, 11, 12, 19, 20, 22]             # the batches' users: they repeat; the others are never looked up
N_POOL = 31                                                 # items 31 .. 40 are never looked up


def _batch(B, L, r, seed):
    """B windows in which users repeat; from 5 windows on, window 0's L inputs are one item, and item 3 is a previous item in window 1,
    the target of window 2 and a negative of window 3; from 257 on item 7 is a negative of 100 windows (more lookups than the update's
    split threshold)"""
    rng = np.random.default_rng(seed)
    uid = rng.choice(USER_POOL, size=B)
    before = rng.integers(0, N_POOL, size=(B, L))
    after = np.stack([rng.permutation(N_POOL)[:1 + r] for _ in range(B)])          # target and negatives distinct
    if B >= 5:
        before[0, :] = 9
        before[1, 0] = 3
        after[2] = (np.arange(1 + r) * 2 + 3) % N_POOL
        after[3] = (np.arange(1 + r) * 2 + 1) % N_POOL                            # 1, 3, ...
        if r == 1:
            after[3] = [1, 3]
        assert 3 in after[3, 1:] and after[2, 0] == 3
    if B >= 257:
        for w in rng.choice(np.arange(4, B), size=100, replace=False):
            if 7 not in after[w]:
                after[w, 1] = 7
            elif after[w, 0] == 7:
                after[w, 0], after[w, 1] = after[w, 1], 7
    assert all(len(set(a)) == 1 + r for a in after.tolist())
    return uid.astype(np.int32), before.astype(np.int32), after.astype(np.int32)


def _serving_baskets(L, seed=0):
    """[U, L]: user 0 an empty basket, 1 one item, 2 L - 1 items, 3 a full one, the others random lengths"""
    rng = np.random.default_rng(50 + seed)
    out = np.full((U, L), -1, np.int32)
    for u, n in enumerate([0, 1, L - 1, L] + [int(x) for x in rng.integers(0, L + 1, size=U - 4)]):
        out[u, :n] = rng.integers(0, N, size=n)
    return out


def _engine(K, L, p, kind='adam', baskets=None):
    from drecpy_amd.engine_fpmc import FpmcEngine
    e = FpmcEngine(U, N, K, L)
    e.set_params(p)
    e.set_optimizer(_optimizer(kind, fo.HP['lr']))
    e.reg = fo.HP['reg']
    e.set_baskets(_serving_baskets(L) if baskets is None else baskets)
    return e


def _tables(e):
    """{oracle name: [U or N, K] numpy view of the device table}, and the same for the two slots"""
    K, ld = e.K, e.ld
    cut = {'P': ('P', slice(0, K)), 'M': ('M', slice(0, K)), 'Q': ('QN', slice(0, K)), 'N': ('QN', slice(ld, ld + K)), 'b': ('b', None)}
    get = lambda t, c: None if t is None else (t.cpu().numpy() if c is None else t.cpu().numpy()[:, c])
    return ({n: get(getattr(e, t), c) for n, (t, c) in cut.items()},
            [{n: get(e.state[t][k], c) for n, (t, c) in cut.items()} for k in range(2)])


def _padding_is_zero(e):
    """the padding columns of P, M and both halves of QN, and of the slots that start at zero"""
    slots = [] if e.opt_kind == 'adagrad' else [(n, s) for n in ('P', 'M', 'QN') for s in e.state[n] if s is not None]
    for name, t in [('P', e.P), ('M', e.M), ('QN', e.QN)] + slots:
        a = t.cpu().numpy()
        pads = [a[:, e.K:e.ld]] + ([a[:, e.ld + e.K:]] if name == 'QN' else [])
        assert not any(x.any() for x in pads), f'a padding column of {name} moved'


def _all_scores(e):
    return e.score_matrix(np.arange(U, dtype=np.int32)).cpu().numpy()


def _check_idle_rows(e, kind, p0, uid, before, after, alphas):
    """rows of P, M, Q, N and b that no window names: bit-equal to the fp32 replay of their reg-only update (parameters and slots)"""
    idle_u = np.setdiff1d(np.arange(U), uid)
    idle_m = np.setdiff1d(np.arange(N), before)
    idle_i = np.setdiff1d(np.arange(N), after)
    assert len(idle_u) >= 13 and len(idle_m) >= 10 and len(idle_i) >= 10
    tabs, slots = _tables(e)
    reg = fo.HP['reg']
    for name, idle, l2c, alpha in (('P', idle_u, reg, alphas[0]), ('M', idle_m, reg, alphas[1]), ('Q', idle_i, reg, alphas[2]),
                                   ('N', idle_i, reg, alphas[2]), ('b', idle_i, 0.0, alphas[3])):
        start = p0[name].astype(F)[idle]
        forms = _idle_replay(kind, start, l2c, alpha)
        got = [tabs[name], slots[0][name], slots[1][name]]
        for k, what in enumerate(('p', 's1', 's2')):
            if forms[0][k] is None:
                continue
            g = got[k][idle]
            same = np.logical_or.reduce([_bits(g) == _bits(f[k]) for f in forms])
            assert same.all(), f'{kind} {name} {what}: {int((~same).sum())} idle elements differ from the fp32 replay, first {np.argwhere(~same)[0]}'
        if kind in ('adam', 'momentum', 'nesterov') and l2c:
            assert (_bits(got[0][idle]) != _bits(start)).any(), f'{kind} {name}: the reg-only update moved nothing'


def _run_against_the_oracle(B, K, L, r, kind='adam', steps=10, batches=None, check_at=(0, 9)):
    p = fo.init_params(np.random.default_rng(100 + K), U, N, K)
    p0 = {k: v.copy() for k, v in p.items()}
    p32 = fo.replay32(p)
    st, st32 = fo.init_state(p, kind), fo.init_state(p32, kind)
    e = _engine(K, L, p, kind)
    baskets = e.baskets.cpu().numpy()
    what = f'B {B} K {K} L {L} r {r} {kind}'
    for s in range(steps):
        uid, before, after = batches[s] if batches is not None else _batch(B, L, r, 1000 * B + 10 * L + s)
        want = fo.step(p, st, s, uid, before, after, kind)
        rep = fo.step(p32, st32, s, uid, before, after, kind)
        got = e.step(s, uid, before, after, want_loss=True)
        _gate(f'{what} step {s} loss', got, want, rep)
        if s in check_at:
            _gate(f'{what} scores after {s + 1} step(s)', _all_scores(e), fo.scores(p, baskets), fo.scores(p32, baskets))
            _padding_is_zero(e)
        if s == 0:
            _check_idle_rows(e, kind, p0, uid, before, after, e._step_sizes(0, (3, 0, 1, 2)))
    return e, p, st


@pytest.mark.parametrize('K', [1, 5, 64, 128])
@pytest.mark.parametrize('B', [1, 5, 64, 257])
def test_adam_steps_match_the_oracle_after_1_and_10_steps(B, K):
    e, p, st = _run_against_the_oracle(B, K, 1, 1)
    _, slots = _tables(e)
    for name in fo.NAMES:                                   # the slots too: Adam's m and v of every row
        for k in range(2):
            scale = max(1e-30, float(np.max(np.abs(st[name][k]))))
            assert np.max(np.abs(slots[k][name] - st[name][k])) <= 1e-4 * scale, (name, k)


@pytest.mark.parametrize('K', [5, 64])
@pytest.mark.parametrize('L,r', [(2, 3), (5, 4), (8, 8)])
def test_longer_windows_and_more_negatives_match_the_oracle(L, r, K):
    _run_against_the_oracle(64, K, L, r)


def test_the_largest_neg_ratio_at_the_widest_rows_matches_the_oracle():
    _run_against_the_oracle(257, 128, 3, MAX_R)


def test_hand_made_batches_match_the_oracle():
    L, r, K = 3, 2, 5
    same_user = (np.full(9, 4, np.int32), np.arange(27, dtype=np.int32).reshape(9, 3) % N_POOL, _batch(9, L, r, 1)[2])
    one_item = (np.array([1, 2], np.int32), np.array([[6, 6, 6], [6, 6, 6]], np.int32), np.array([[6, 2, 3], [1, 6, 0]], np.int32))
    # the id 5: a user, a previous item, a target and a negative
    shared_id = (np.array([5, 5, 8], np.int32), np.array([[5, 1, 5], [2, 5, 3], [5, 5, 5]], np.int32), np.array([[5, 0, 1], [4, 5, 6], [5, 7, 8]], np.int32))
    for name, batch in (('same user', same_user), ('one item', one_item), ('shared id', shared_id)):
        print(name)
        _run_against_the_oracle(len(batch[0]), K, L, r, steps=2, batches=[batch, batch], check_at=(0, 1))


@pytest.mark.parametrize('K', [5, 64])
@pytest.mark.parametrize('kind', ['adam', 'adagrad', 'sgd', 'momentum', 'nesterov', 'rmsprop'])
def test_one_step_under_every_rule(kind, K):
    e, _, _ = _run_against_the_oracle(64, K, 2, 3, kind, steps=1, check_at=(0,))
    n = 2 if kind == 'adam' else bo.oo.N_SLOTS[kind]
    assert [s is not None for s in e.state['QN']] == [k < n for k in range(2)]


@pytest.mark.parametrize('K', [1, 5])
def test_padding_stays_zero_over_ten_steps(K):
    p = fo.init_params(np.random.default_rng(3), U, N, K)
    e = _engine(K, 4, p)
    for s in range(10):
        e.step(s, *_batch(64, 4, 3, 40 + s))
    _padding_is_zero(e)
    assert e.QN[:, e.ld:e.ld + K].cpu().numpy().any() and e.M[:, :K].cpu().numpy().any()


def test_the_same_inputs_give_the_same_bits():
    K, B, L, r = 20, 257, 3, 5
    p = fo.init_params(np.random.default_rng(1), U, N, K)
    runs = []
    for _ in range(2):
        e = _engine(K, L, p)
        losses = [e.step(s, *_batch(B, L, r, 5 + s), want_loss=True) for s in range(3)]
        runs.append([t.cpu().numpy().copy() for t in e.tensors().values()] + [x.cpu().numpy().copy() for n in e.state for x in e.state[n]]
                    + [np.array(losses)])
    assert all(np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)) for a, b in zip(*runs))
    assert not np.array_equal(runs[0][0][:, :K], p['P'].astype(F))


# ---- the query rows --------------------------------------------------------------------------------------------------------------------
def _context32(P, M, u, ids):
    """NumPy float32 in the kernel's stated order: positions ascending, then one multiply by 1.0f / (the number present)"""
    acc = np.zeros(M.shape[1], F)
    ids = [int(i) for i in ids if i >= 0]
    for i in ids:
        acc = acc + M[i]
    if ids:
        acc = acc * (F(1.0) / F(len(ids)))
    return np.concatenate([P[u], acc])


@pytest.mark.parametrize('K', [1, 5, 64, 128])
@pytest.mark.parametrize('L', [1, 4, 8])
def test_query_rows_are_bit_equal_to_the_fp32_replay_and_to_the_steps_context(L, K):
    import torch
    p =fo.init_params(np.random.default_rng(9 + K), U, N, K)
    baskets = _serving_baskets(L, seed=L)
    baskets[4] = [7, -1, 5, -1, -1, 2, -1, 6][:L]          # absent positions between present ones
    e = _engine(K, L, p, baskets=baskets)
    users = np.array(list(range(U)) + [3, 0, 3], np.int32)
    got = e._query_rows(_dev(users, np.int32)).cpu().numpy()
    assert got.shape == (len(users), 2 * e.ld)
    P, M = e.P.cpu().numpy(), e.M.cpu().numpy()
    want = np.stack([_context32(P, M, u, baskets[u]) for u in users])
    assert np.array_equal(_bits(got), _bits(want))
    assert not got[0, e.ld:].any() and got[3, e.ld:e.ld + K].any()
    # the windows of a step = the full baskets: the context rows the step wrote (the head of its scratch) are these rows
    full = np.flatnonzero((baskets >= 0).all(axis=1)).astype(np.int32)
    assert len(full) >= 1
    after = np.stack([np.arange(3) + k for k in range(len(full))]).astype(np.int32)
    e.step(0, full, baskets[full], after)
    assert e._scratch.data_ptr() % 256 == 0
    ctx = e._scratch[:len(full) * 2 * e.ld * 4].view(torch.float32).cpu().numpy().reshape(len(full), 2 * e.ld)
    assert np.array_equal(_bits(ctx), _bits(got[full]))


def test_query_rows_refusals():
    import torch
    from drecpy_amd._lib import lib, ptr
    e = _engine(5, 3, fo.init_params(np.random.default_rng(2), U, N, 5))
    uid = _dev(np.arange(4), np.int32)
    out = torch.full((4, 2 * e.ld + 4), -7.0, dtype=torch.float32, device='cuda:0')
    good = [ptr(e.P), ptr(e.M), e.ld, ptr(e.baskets), 3, ptr(uid), 4, ptr(out), None]
    bad = {'P': (0, None), 'M': (1, None), 'baskets': (3, None), 'uid': (5, None), 'out': (7, None), 'n 0': (6, 0), 'L 0': (4, 0), 'L 9': (4, 9),
           'ld 0': (2, 0), 'ld 6': (2, 6), 'ld 132': (2, 132), 'a misaligned out': (7, C.c_void_p(out.data_ptr() + 4))}
    for what, (at, value) in bad.items():
        args = list(good)
        args[at] = value
        assert lib().drx_fpmc_query_rows(*args) == EINVAL, what
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()
    assert lib().drx_fpmc_query_rows(*good) == 0


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_step_refusals_leave_the_parameters_alone():
    import torch
    from drecpy_amd import _lib
    from drecpy_amd._lib import lib, ptr
    K, B, L, r = 8, 16, 2, 3
    p = fo.init_params(np.random.default_rng(2), U, N, K)
    e = _engine(K, L, p)
    uid, before, after = (_dev(a, np.int32) for a in _batch(B, L, r, 3))
    need = int(lib().drx_fpmc_step_scratch_bytes(B, L, r, e.ld, U, N))
    assert need > 0
    for bad in ((0, L, r, e.ld, U, N), (-1, L, r, e.ld, U, N), (B, 0, r, e.ld, U, N), (B, 9, r, e.ld, U, N), (B, L, 0, e.ld, U, N),
                (B, L, MAX_R + 1, e.ld, U, N), (B, L, r, 0, U, N), (B, L, r, 6, U, N), (B, L, r, 132, U, N), (B, L, r, e.ld, 0, N),
                (B, L, r, e.ld, U, 0)):
        assert lib().drx_fpmc_step_scratch_bytes(*bad) == 0, bad
    assert lib().drx_fpmc_step_scratch_bytes(B, 8, MAX_R, 128, U, N) > 0
    sc = torch.zeros(need, dtype=torch.uint8, device='cuda:0')
    alphas = (C.c_float * 4)(1e-2, 1e-2, 1e-2, 1e-2)
    slots = [ptr(s) for n in ('P', 'M', 'QN', 'b') for s in e.state[n]]         # P m, P v, M m, M v, QN m, QN v, b m, b v
    adam, momentum = _lib.OptRule(0, 0.0, 0.9, 0.999, 1e-7), _lib.OptRule(4, 0.0, 0.9, 0.0, 0.0)
    rowwise, unknown = _lib.OptRule(2, 0.0, 0.0, 0.0, 1e-7), _lib.OptRule(99, 0.0, 0.0, 0.0, 0.0)
    good = [ptr(e.P), ptr(e.M), ptr(e.QN), ptr(e.b)] + slots + [e.ld, U, N, ptr(uid), ptr(before), ptr(after), B, L, r, C.byref(adam), alphas,
                                                                1e-3, None, ptr(sc), need, None]
    params = list(e.tensors().values())
    start = [t.cpu().numpy().copy() for t in params]
    bad = {'P': (0, None), 'M': (1, None), 'QN': (2, None), 'b': (3, None), 'uid': (15, None), 'before': (16, None), 'after': (17, None),
           'rule': (21, None), 'alphas': (22, None), 'scratch': (25, None), 'B 0': (18, 0), 'B -3': (18, -3), 'L 0': (19, 0), 'L 9': (19, 9),
           'r 0': (20, 0), 'r 17': (20, MAX_R + 1), 'ld 0': (12, 0), 'ld 2': (12, 2), 'ld 6': (12, 6), 'ld 132': (12, 132),
           'n_users 0': (13, 0), 'n_items 0': (14, 0), 'adam without P m': (4, None), 'adam without M v': (7, None),
           'adam without QN m': (8, None), 'adam without b v': (11, None), 'momentum without M s1': (6, None),
           'row-wise adagrad': (21, C.byref(rowwise)), 'an unknown rule': (21, C.byref(unknown)),
           'a misaligned P': (0, C.c_void_p(e.P.data_ptr() + 4)), 'a misaligned M': (1, C.c_void_p(e.M.data_ptr() + 4)),
           'a misaligned QN': (2, C.c_void_p(e.QN.data_ptr() + 8))}
    for what, (at, value) in bad.items():
        args = list(good)
        args[at] = value
        if what.startswith('momentum'):
            args[21] = C.byref(momentum)
        assert lib().drx_fpmc_step(*args) == EINVAL, what
    small = list(good)
    small[26] = need // 2
    assert lib().drx_fpmc_step(*small) == -2                                     # DRX_ESCRATCH
    torch.cuda.synchronize()
    for t, b in zip(params, start):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(b))
    assert not sc.cpu().numpy().any(), 'a refused call wrote its scratch'
    assert lib().drx_fpmc_step(*good) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(_bits(e.P.cpu().numpy()), _bits(start[0]))


def test_engine_refuses_shapes_outside_its_domain():
    from drecpy_amd._lib import DrxError
    from drecpy_amd.engine_fpmc import FpmcEngine
    for K in (0, 129, 2.5):
        with pytest.raises(DrxError, match='factors'):
            FpmcEngine(U, N, K, 1)
    for L in (0, 9):
        with pytest.raises(DrxError, match='L must'):
            FpmcEngine(U, N, 4, L)
    e = _engine(4, 2, fo.init_params(np.random.default_rng(0), U, N, 4))
    with pytest.raises(DrxError, match='outside its'):
        e.step(0, *_batch(8, 2, MAX_R + 1, 0))
    with pytest.raises(DrxError, match='baskets'):
        e.set_baskets(np.full((U, 2), N))


# ---- the public class ------------------------------------------------------------------------------------------------------------------
LF, RF = 2, 3                                               # the fitted model's window and neg_ratio


def _records():
    """(user, item, interaction, timestamp) rows of a 23 x 41 frame, users and items in first-appearance order (internal id == raw id),
    and every user's sequence (records >= THR by timestamp).  User 0 holds all but RF items, 1 one item (fewer than L), 2 nothing at or
    above the threshold (an empty basket), 3 exactly L + 1, the others 4 - 14 records on both sides of the threshold; timestamps are not
    in record order."""
    rng = np.random.default_rng(2025)
    rows = [(0, i, 2.0) for i in range(N - RF)] + [(1, N - 3, 1.0), (2, N - 2, 0.5), (3, N - 1, 2.0), (3, 5, 1.0), (3, 9, 3.0)]
    for u in range(4, U):
        items = rng.choice(N, size=int(rng.integers(4, 15)), replace=False)
        rows += [(u, int(i), float(rng.choice([0.5, 1.0, 2.0, 3.0], p=[0.2, 0.3, 0.3, 0.2]))) for i in items]
    ts = rng.permutation(len(rows))
    rows = [(u, i, v, int(t)) for (u, i, v), t in zip(rows, ts)]
    seqs = [[i for _, i, v, _ in sorted((r for r in rows if r[0] == u), key=lambda r: r[3]) if v >= THR] for u in range(U)]
    assert len(seqs[0]) == N - RF and len(seqs[1]) == 1 and seqs[2] == [] and len(seqs[3]) == LF + 1
    return rows, seqs


def _dataset():
    from drecpy_amd.Dataset import InteractionDataset
    u, i, v, t = (np.array(c) for c in zip(*_records()[0]))
    return InteractionDataset.from_arrays(u.astype(np.int64), i.astype(np.int64), v.astype(np.float64), timestamp=t.astype(np.int64))


FIT = dict(epochs=20, batch_size=64, learning_rate=1e-2, neg_ratio=RF, reg_rate=1e-3)


def _oracle_fit(w, twin, model, epochs, B, r):
    out = []
    for q in (w, fo.replay32(w)):
        p = {k: v.copy() for k, v in q.items()}
        st = fo.init_state(p, 'adam')
        for s in range(epochs):
            fo.step(p, st, s, *list_sample_counter(twin, B, LF, 1, r, model._draw_seed(s + 1)), 'adam')
        out.append(p)
    return out


@pytest.fixture(scope='module')
def fitted():
    """(model, oracle parameters, their float32 replay, baskets) after the same 20 steps on the same draws"""
    from drecpy_amd.Recommender.Baseline import FPMC
    K = 10
    w = fo.init_params(np.random.default_rng(42), U, N, K)
    model = FPMC(factors=K, L=LF, seed=3, interaction_threshold=THR, verbose=False)
    model.fit(_dataset(), initial_weights=w, **FIT)
    ds = model.interaction_dataset
    assert all(ds.user_to_uid(u) == u for u in range(U)) and all(ds.item_to_iid(i) == i for i in range(N))
    twin = fo.twin_of(_records()[1], N, LF, RF)
    p, p32 = _oracle_fit(w, twin, model, FIT['epochs'], FIT['batch_size'], RF)
    return model, p, p32, fo.baskets_of(twin, U, LF)


def test_the_windows_fed_to_the_step_are_the_oracle_streams(fitted):
    model, _, _, baskets = fitted
    seqs = _records()[1]
    twin = fo.twin_of(seqs, N, LF, RF)
    mine = model._sampler.twin_host_arrays()
    for k in ('indptr', 'seq_ids', 'held_indptr', 'held', 'group_value', 'eligible'):
        assert np.array_equal(np.asarray(mine[k]), twin[k]), k
    assert 0 in twin['eligible'] and 3 in twin['eligible'] and 1 not in twin['eligible'] and 2 not in twin['eligible']
    for n, seed in ((1, 0), (257, model._draw_seed(1)), (1000, 0xFEDCBA9876543210)):
        got = [t.cpu().numpy() for t in model._sampler.sample_device(n, seed)]
        want = list_sample_counter(twin, n, LF, 1, RF, seed & ((1 << 64) - 1))
        for g, w_, name in zip(got, want, ('uid', 'before', 'after')):
            assert g.dtype == np.int32 and np.array_equal(g, w_), f'{name} differs at n {n}'
    assert np.array_equal(model._engine.baskets.cpu().numpy(), baskets)
    assert baskets[1].tolist() == [seqs[1][0], -1] and baskets[2].tolist() == [-1, -1] and baskets[3].tolist() == seqs[3][-2:]


def test_fit_equals_the_oracle_fit_on_the_same_draws(fitted):
    model, p, p32, baskets = fitted
    x = fo.scores(p, baskets)
    _gate('scores after fit(epochs=20)', _all_scores(model._engine), x, fo.scores(p32, baskets))
    _padding_is_zero(model._engine)
    for u in (1, 2, 5):                                     # fewer than L items, an empty basket, an ordinary user
        assert model.predict(u, 7) == pytest.approx(x[u, 7], abs=1e-5)
    assert isinstance(model.predict(5, 7), float)


def test_recommend_batch_equals_recommend_and_the_oracle_order(fitted):
    model, p, _, baskets = fitted
    x = fo.scores(p, baskets)
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
        full = {u: model.recommend_batch([u], n=N, novelty=novelty)[0] for u in set(users)}
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
    _gate('predict_pairs', got, fo.scores(p, baskets)[users, items], fo.scores(p32, baskets)[users, items])
    assert np.isnan(model.predict_pairs([1, 999], [1, 1], skip_errors=True)[1])


def test_rank_and_evaluations_batched_and_not(fitted):
    from drecpy_amd.Evaluation import predictive_evaluation, ranking_evaluation, recommendation_evaluation
    model, p, _, baskets = fitted
    x = fo.scores(p, baskets)
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
    from drecpy_amd.Recommender.Baseline import FPMC
    model, _, _, baskets = fitted
    path = str(tmp_path / 'fpmc.pkl')
    model.save(path)
    other = FPMC.load(path)
    assert isinstance(other, FPMC)
    assert np.array_equal(other._engine.baskets.cpu().numpy(), baskets)                       # rebuilt from the dataset
    users, items = list(range(U)) * 2, [(7 * k) % N for k in range(2 * U)]
    assert np.array_equal(other.predict_pairs(users, items), model.predict_pairs(users, items))
    assert other.recommend_batch([5, 22, 1, 2], n=7) == model.recommend_batch([5, 22, 1, 2], n=7)
    assert other.recommend(5, n=7) == model.recommend(5, n=7)


def test_callbacks_early_stopping_and_loss():
    from drecpy_amd.Recommender.Baseline import FPMC
    from drecpy_amd.Recommender.early_stopping import MaxValidationValueRule
    K = 6
    w = fo.init_params(np.random.default_rng(9), U, N, K)
    seen = []
    model = FPMC(factors=K, L=LF, seed=1, interaction_threshold=THR, verbose=False)
    model.fit(_dataset(), epochs=6, batch_size=32, learning_rate=1e-2, neg_ratio=2, reg_rate=1e-3, initial_weights=w,
              epoch_callback_fn=lambda m: seen.append(float(m.predict(5, 7))) or {'score': -len(seen)}, epoch_callback_freq=2,
              early_stopping_rule=MaxValidationValueRule('score'), early_stopping_freq=2)
    assert len(seen) >= 1 and model.fitted
    # the best epoch is the first one evaluated (the score falls): the weights are those of epoch 2
    twin = fo.twin_of(_records()[1], N, LF, 2)
    p, p32 = _oracle_fit(w, twin, model, 2, 32, 2)
    baskets = fo.baskets_of(twin, U, LF)
    _gate('scores after the revert to epoch 2', _all_scores(model._engine), fo.scores(p, baskets), fo.scores(p32, baskets))


@pytest.mark.parametrize('what', ['neg_ratio 0', 'neg_ratio 17', 'K 0', 'K 129', 'L 0', 'L 9', 'no window', 'optimizer'])
def test_fit_refuses_by_name(what):
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender.Baseline import FPMC
    ds = _dataset()
    kw = dict(epochs=1, batch_size=8)
    if what.startswith('neg_ratio'):
        with pytest.raises(Exception, match='neg_ratio'):
            FPMC(factors=4, interaction_threshold=THR, verbose=False).fit(ds, neg_ratio=int(what.split()[1]), **kw)
    elif what.startswith('K'):
        with pytest.raises(Exception, match='factors'):
            FPMC(factors=int(what[2:]), interaction_threshold=THR, verbose=False).fit(ds, **kw)
    elif what.startswith('L'):
        with pytest.raises(Exception, match=r'L must'):
            FPMC(factors=4, L=int(what[2:]), interaction_threshold=THR, verbose=False).fit(ds, **kw)
    elif what == 'optimizer':
        with pytest.raises(Exception, match='dense rules'):
            FPMC(factors=4, interaction_threshold=THR, verbose=False).fit(ds, optimizer='rowwise_adagrad', **kw)
    else:
        # no user holds L + 1 = 4 records
        short = InteractionDataset.from_arrays(np.array([0, 0, 1, 1, 1]), np.array([0, 1, 0, 1, 2]), np.full(5, 2.0), timestamp=np.arange(5))
        with pytest.raises(Exception, match='Failed to sample group records'):
            FPMC(factors=4, L=3, interaction_threshold=THR, verbose=False).fit(short, **kw)
