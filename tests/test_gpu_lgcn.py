"""LightGCN on the device against tests/lgcn_oracle.py (NumPy float64), through the C ABI (drx_lgcn_propagate, drx_lgcn_final,
drx_lgcn_step) and drecpy_amd.engine_lgcn.LgcnEngine.  (The public class: tests/test_gpu_lgcn_api.py.)

drx_lgcn_propagate alone is held BIT FOR BIT to an integer oracle: node weights that are 1 or powers of two and integer-valued inputs in
-8 .. 8 make every sum exact in fp32 (at most 2 S + 1 = 257 terms of magnitude <= 8, far below 2^24), whatever the order.

The gate of the step on ALL scores (every user x every item) and on the loss is the project's, from tests/test_gpu_fpmc.py:

    err(GPU) <= max(1e-5, 4 err(replay)) * max(1, max |x|)

where the replay is the oracle itself on float32 arrays.  Every (GPU, replay) pair is printed (pytest -s); DESIGN.md section 3.14 has the
table.  The standing graph has 37 users x 53 items: user 1 has no positive (two pairs below the threshold), item 52 is held by nobody,
item 0 by every user with a positive (the long row), user 2 holds every item but 52, the others 7 - 19 items with values on both sides
of the threshold.  The final embeddings of a step are read from its scratch (LgcnEngine.step_ebar) and compared bit for bit with
drx_lgcn_final on the parameters the step started from."""
import ctypes as C

import numpy as np
import pytest

import bpr_oracle as bo
import lgcn_oracle as lo
from test_gpu_bpr import _bits, _dev, _idle_replay, _optimizer
from test_gpu_fpmc import _gate

pytestmark = pytest.mark.gpu

U, N, THR = 37, 53, 1.0
F = np.float32
EINVAL, ESCRATCH = -1, -2
ISOLATED_USER, ISOLATED_ITEM = 1, 52


def _pairs():
    """(user, item, interaction) rows, users and items in first-appearance order (internal id == raw id)"""
    rng = np.random.default_rng(2027)
    pairs = [(0, 0, 2.0), (1, 0, 0.5), (1, 1, 0.25)]
    pairs += [(2, i, 1.0 + (i % 3)) for i in range(N - 1)]
    for u in [0] + list(range(3, U)):
        items = rng.choice(np.arange(1, N - 1), size=int(rng.integers(6, 19)), replace=False)
        pairs += [(u, 0, 2.0)] * (u != 0) + [(u, int(i), float(rng.choice([0.5, 1.0, 2.0, 3.0]))) for i in items]
    return pairs


@pytest.fixture(scope='module')
def frame():
    f = bo.Frame(U, N, _pairs(), THR)
    assert not f.positives[ISOLATED_USER] and len(f.recorded[ISOLATED_USER]) == 2
    assert all(ISOLATED_ITEM not in row for row in f.recorded) and f.positives[2] == list(range(N - 1))
    assert all(0 in f.positives[u] for u in range(U) if u != ISOLATED_USER)
    assert any(len(f.recorded[u]) > len(f.positives[u]) for u in range(3, U))
    assert 330 <= sum(len(r) for r in f.positives) <= 470
    return f


@pytest.fixture(scope='module')
def adjacency(frame):
    return lo.adjacency(frame.positives, N)


def _symmetric_csr(rows, n_items):
    """(indptr, indices) of the symmetric adjacency of per-user item lists: user rows list n_users + iid, item rows list uids"""
    nu = len(rows)
    lists = [[nu + i for i in sorted(set(r))] for r in rows] + [[u for u in range(nu) if i in rows[u]] for i in range(n_items)]
    indptr = np.zeros(len(lists) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in lists])
    return indptr, np.asarray([c for r in lists for c in r], np.int32)


# ---- drx_lgcn_propagate alone -------------------------------------------------------------------------------------------------------------
def _exact_propagate(indptr, indices, w, base, x, scale):
    out = np.zeros_like(x, dtype=np.float64)
    for r in range(len(indptr) - 1):
        cols = indices[indptr[r]:indptr[r + 1]]
        out[r] = w[r] * (w[cols][:, None] * x[cols]).sum(axis=0)
    return scale * (out + (0 if base is None else base))


def _check_propagate(indptr, indices, ld, seed):
    import torch
    from drecpy_amd.engine_lgcn import LgcnGraph, propagate
    n = len(indptr) - 1
    K = max(1, ld - 3)                                                # the last columns are padding: zero in, zero out
    rng = np.random.default_rng(seed)
    for w in (np.ones(n), 2.0 ** -rng.integers(0, 3, size=n)):
        g = LgcnGraph(indptr, indices, w)
        x, b = (np.zeros((n, ld)) for _ in range(2))
        x[:, :K], b[:, :K] = rng.integers(-8, 9, size=(n, K)), rng.integers(-8, 9, size=(n, K))
        for base, scale in ((None, 1.0), (b, 1.0), (b, 0.25)):
            out = torch.full((n, ld), 777.0, dtype=torch.float32, device='cuda:0')
            propagate(g, _dev(x, F), None if base is None else _dev(base, F), scale, out=out)
            torch.cuda.synchronize()
            got, want = out.cpu().numpy(), _exact_propagate(indptr, indices, w, base, x, scale)
            assert np.array_equal(want.astype(F).astype(np.float64), want)
            bad = np.argwhere(_bits(got) != _bits(want))
            assert len(bad) == 0, f'ld {ld} base {base is not None} scale {scale}: {len(bad)} elements differ, first {bad[0]}'
            assert not got[:, K:].any()


@pytest.mark.parametrize('ld', [4, 8, 64, 68, 256])
def test_propagate_is_bit_equal_to_the_integer_oracle_on_the_standing_graph(frame, ld):
    indptr, indices = _symmetric_csr(frame.positives, N)
    assert np.diff(indptr).max() == N - 1 and np.diff(indptr)[U] == U - 1 and (np.diff(indptr) == 0).sum() == 2
    _check_propagate(indptr, indices, ld, 10 + ld)


@pytest.mark.parametrize('ld', [4, 8, 64, 68, 256])
def test_propagate_at_the_borders_of_the_row_split(ld):
    from drecpy_amd._lib import lib
    S = int(lib().drx_lgcn_row_split())
    lengths = [0, 1, 2, S - 1, S, S + 1, 2 * S + 1] if S > 0 else [0, 1, 2, 63, 64, 65, 257]
    n = 301                                                          # 43 rows of every length: more row groups than one workgroup
    rng = np.random.default_rng(ld)
    rows = [np.sort(rng.choice(n, size=lengths[r % len(lengths)], replace=False)) for r in range(n)]
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    _check_propagate(indptr, np.concatenate(rows).astype(np.int32), ld, 20 + ld)


def test_propagate_refusals_write_nothing(frame):
    import torch
    from drecpy_amd import _lib
    from drecpy_amd._lib import lib, ptr
    from drecpy_amd.engine_lgcn import LgcnGraph
    S = int(lib().drx_lgcn_row_split())
    n, ld = 4, 8
    indptr = np.array([0, S + 1, S + 2, S + 2, S + 3], np.int64)     # one cut row
    indices = np.concatenate([np.arange(S + 1) % n, [0, 1]]).astype(np.int32)
    g = LgcnGraph(indptr, indices, np.ones(n))
    assert g.n_cut == 1 and g.n_seg == 5
    x = torch.ones(n, ld, device='cuda:0')
    out = torch.full((n, ld), 777.0, device='cuda:0')
    need = int(lib().drx_lgcn_part_bytes(C.byref(g.struct), ld))
    part = torch.zeros(need, dtype=torch.uint8, device='cuda:0')
    assert need > 0 and lib().drx_lgcn_part_bytes(C.byref(g.struct), 6) == 0 and lib().drx_lgcn_part_bytes(None, ld) == 0
    good = [C.byref(g.struct), ptr(x), ptr(x), ptr(out), ld, 1.0, ptr(part), need, None]
    fields = [f for f, _ in _lib.LgcnGraph._fields_]

    def broken(**kw):
        s = _lib.LgcnGraph(*[kw.get(f, getattr(g.struct, f)) for f in fields])
        return C.byref(s)
    bad = {'graph': (0, None), 'indptr': (0, broken(indptr=None)), 'indices': (0, broken(indices=None)), 'w': (0, broken(w=None)),
           'seg_row': (0, broken(seg_row=None)), 'seg_ptr': (0, broken(seg_ptr=None)), 'cut_rows': (0, broken(cut_rows=None)),
           'N 0': (0, broken(N=0)), 'n_seg < N': (0, broken(n_seg=3)), 'in': (2, None), 'out': (3, None), 'out == in': (3, ptr(x)),
           'ld 0': (4, 0), 'ld 6': (4, 6), 'ld 260': (4, 260), 'a misaligned in': (2, C.c_void_p(x.data_ptr() + 4)),
           'no part with a cut row': (6, None)}
    for what, (at, value) in bad.items():
        args = list(good)
        args[at] = value
        assert lib().drx_lgcn_propagate(*args) == EINVAL, what
    args = list(good)
    args[7] = 64
    assert lib().drx_lgcn_propagate(*args) == ESCRATCH
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 777.0).all() and not part.cpu().numpy().any()
    assert lib().drx_lgcn_propagate(*good) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[:, 0], 1.0 + np.diff(indptr))


# ---- the step --------------------------------------------------------------------------------------------------------------------------
USER_POOL = [2, 4, 5, 6, 8, 11, 12, 19, 20, 36]            # the pool batches' users; user 1 is never named
ITEM_POOL = list(range(0, 40))                              # item 52 is never named


def _pool_batch(T, seed):
    rng = np.random.default_rng(seed)
    uid = rng.choice(USER_POOL, size=T)
    pos = rng.choice(ITEM_POOL, size=T)
    neg = (pos + 1 + rng.integers(0, len(ITEM_POOL) - 1, size=T)) % len(ITEM_POOL)
    uid[:3], pos[:3], neg[:3] = [4, 4, 5], [3, 7, 3], [7, 3, 9]   # items 3 and 7 collect both signs
    return uid.astype(np.int32), pos.astype(np.int32), neg.astype(np.int32)


def _engine(frame, K, layers, p, kind='adam'):
    from drecpy_amd.engine_lgcn import LgcnEngine
    e = LgcnEngine(U, N, K, layers)
    e.set_params(p)
    e.set_optimizer(_optimizer(kind, lo.HP['lr']))
    e.reg = lo.HP['reg']
    e.set_graph(bo.Frame.csr(frame.positives))
    return e


def _all_scores(e):
    return e.score_matrix(np.arange(U, dtype=np.int32)).cpu().numpy()


def _padding_is_zero(e):
    slots = [] if e.opt_kind == 'adagrad' else [s for n in ('P', 'Q') for s in e.state[n] if s is not None]
    for t in [e.E0, e.final_embeddings()] + slots:
        assert not t[:, e.K:].cpu().numpy().any(), 'a padding column moved'


def _check_isolated_rows(e, kind, p0, alphas):
    """the rows of the user without a positive and of the item nobody holds, named by no triple: bit-equal to the fp32 replay of their
    reg-only update (parameters and slots)"""
    for name, row, alpha in (('P', ISOLATED_USER, alphas[0]), ('Q', ISOLATED_ITEM, alphas[1])):
        start = p0[name].astype(F)[[row]]
        forms = _idle_replay(kind, start, lo.HP['reg'], alpha)
        got = [getattr(e, name)] + list(e.state[name])
        for k, what in enumerate(('p', 's1', 's2')):
            if forms[0][k] is None:
                continue
            g = got[k].cpu().numpy()[[row], :e.K]
            same = np.logical_or.reduce([_bits(g) == _bits(f[k]) for f in forms])
            assert same.all(), f'{kind} {name} {what}: {int((~same).sum())} elements of the isolated row differ from the fp32 replay'
        if kind in ('adam', 'momentum', 'nesterov'):
            assert (_bits(got[0].cpu().numpy()[[row], :e.K]) != _bits(start)).any(), f'{kind} {name}: the reg-only update moved nothing'


@pytest.mark.parametrize('r', [1, 4])
@pytest.mark.parametrize('layers', [0, 1, 3, 4])
@pytest.mark.parametrize('K', [5, 64])
def test_adam_steps_match_the_oracle_after_1_and_10_steps(frame, adjacency, K, layers, r):
    T = 96
    p = lo.init_params(np.random.default_rng(100 + K + layers), U, N, K)
    p32 = lo.replay32(p)
    st, st32 = lo.init_state(p, 'adam'), lo.init_state(p32, 'adam')
    e = _engine(frame, K, layers, p)
    what = f'K {K} layers {layers} r {r}'
    for s in range(10):
        uid, pos, neg = bo.sample(frame, T, r, 1000 * r + s)
        want = lo.step(p, st, adjacency, layers, s, uid, pos, neg)
        rep = lo.step(p32, st32, adjacency, layers, s, uid, pos, neg)
        got = e.step(s, uid, pos, neg, want_loss=True)
        _gate(f'{what} step {s} loss', got, want, rep)
        if s in (0, 9):
            _gate(f'{what} scores after {s + 1} step(s)', _all_scores(e), lo.scores(p, adjacency, layers), lo.scores(p32, adjacency, layers))
            _padding_is_zero(e)
    for name in lo.NAMES:                                   # the slots too: Adam's m and v of every row
        for k in range(2):
            got = e.state[name][k].cpu().numpy()[:, :K]
            scale = max(1e-30, float(np.max(np.abs(st[name][k]))))
            assert np.max(np.abs(got - st[name][k])) <= 1e-3 * scale, (name, k)


@pytest.mark.parametrize('kind', ['adam', 'adagrad', 'sgd', 'momentum', 'nesterov', 'rmsprop'])
def test_one_step_under_every_rule_and_the_isolated_rows(frame, adjacency, kind):
    K, layers, T = 20, 2, 64
    p = lo.init_params(np.random.default_rng(7), U, N, K)
    p0 = {k: v.copy() for k, v in p.items()}
    p32 = lo.replay32(p)
    st, st32 = lo.init_state(p, kind), lo.init_state(p32, kind)
    e = _engine(frame, K, layers, p, kind)
    uid, pos, neg = _pool_batch(T, 77)
    want = lo.step(p, st, adjacency, layers, 0, uid, pos, neg, kind)
    rep = lo.step(p32, st32, adjacency, layers, 0, uid, pos, neg, kind)
    got = e.step(0, uid, pos, neg, want_loss=True)
    _gate(f'{kind} loss', got, want, rep)
    _gate(f'{kind} scores', _all_scores(e), lo.scores(p, adjacency, layers), lo.scores(p32, adjacency, layers))
    _padding_is_zero(e)
    _check_isolated_rows(e, kind, p0, e._step_sizes(0, (2, 0, 1)))
    n = 2 if kind == 'adam' else bo.oo.N_SLOTS[kind]
    assert [s is not None for s in e.state['Q']] == [k < n for k in range(2)]


def test_the_same_inputs_give_the_same_bits(frame):
    K, T = 20, 257
    p = lo.init_params(np.random.default_rng(1), U, N, K)
    runs = []
    for _ in range(2):
        e = _engine(frame, K, 3, p)
        for s in range(3):
            e.step(s, *_pool_batch(T, 5 + s))
        runs.append([e.E0.cpu().numpy().copy()] + [x.cpu().numpy().copy() for n in lo.NAMES for x in e.state[n]])
    assert len(runs[0]) == 5 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(*runs))
    assert not np.array_equal(runs[0][0][:U, :K], p['P'].astype(F))


def test_padding_stays_zero_over_ten_steps(frame):
    K = 5
    e = _engine(frame, K, 3, lo.init_params(np.random.default_rng(2), U, N, K))
    for s in range(10):
        e.step(s, *_pool_batch(96, 40 + s))
        for t in [e.E0] + [x for n in lo.NAMES for x in e.state[n]]:
            assert not t.cpu().numpy()[:, K:].any(), f'step {s}: a padding column moved'
    assert not e.final_embeddings().cpu().numpy()[:, K:].any() and not e.step_ebar().cpu().numpy()[:, K:].any()


@pytest.mark.parametrize('layers', [0, 1, 2, 3, 4])
def test_final_embeddings_have_the_bits_of_the_next_steps_forward(frame, adjacency, layers):
    K = 12
    p = lo.init_params(np.random.default_rng(3), U, N, K)
    e = _engine(frame, K, layers, p)
    e.step(0, *_pool_batch(64, 1))
    served = e.final_embeddings().cpu().numpy().copy()             # after step 0: what the next step's forward must compute
    start = e.E0.cpu().numpy().copy()
    if layers == 0:
        assert np.array_equal(_bits(served), _bits(start))
        return
    e.step(1, *_pool_batch(64, 2))
    assert np.array_equal(_bits(e.step_ebar().cpu().numpy()), _bits(served))
    assert not np.array_equal(_bits(e.final_embeddings().cpu().numpy()), _bits(served))      # the cache was dropped by the step
    q = dict(zip(lo.NAMES, (start[:U, :K].astype(np.float64), start[U:, :K].astype(np.float64))))
    assert np.max(np.abs(served[:, :K] - lo.final(q, adjacency, layers))) <= 1e-5


def test_step_refusals_leave_the_parameters_alone(frame):
    import torch
    from drecpy_amd import _lib
    from drecpy_amd._lib import lib, ptr
    K, T, layers = 8, 16, 2
    e = _engine(frame, K, layers, lo.init_params(np.random.default_rng(2), U, N, K))
    g = e._graph.struct
    uid, pos, neg = (_dev(a, np.int32) for a in _pool_batch(T, 3))
    need = int(lib().drx_lgcn_step_scratch_bytes(C.byref(g), T, e.ld, U))
    assert need > 0
    for bad in ((None, T, e.ld, U), (C.byref(g), 0, e.ld, U), (C.byref(g), -1, e.ld, U), (C.byref(g), T, 0, U), (C.byref(g), T, 6, U),
                (C.byref(g), T, 260, U), (C.byref(g), T, e.ld, 0), (C.byref(g), T, e.ld, U + N)):
        assert lib().drx_lgcn_step_scratch_bytes(*bad) == 0, bad
    sc = torch.zeros(need, dtype=torch.uint8, device='cuda:0')
    alphas = (C.c_float * 2)(1e-2, 1e-2)
    slots = [ptr(s) for n in lo.NAMES for s in e.state[n]]                      # P m, P v, Q m, Q v
    adam, momentum = _lib.OptRule(0, 0.0, 0.9, 0.999, 1e-7), _lib.OptRule(4, 0.0, 0.9, 0.0, 0.0)
    rowwise, unknown = _lib.OptRule(2, 0.0, 0.0, 0.0, 1e-7), _lib.OptRule(99, 0.0, 0.0, 0.0, 0.0)
    fields = [f for f, _ in _lib.LgcnGraph._fields_]
    no_w = _lib.LgcnGraph(*[None if f == 'w' else getattr(g, f) for f in fields])
    good = [ptr(e.E0)] + slots + [e.ld, U, C.byref(g), ptr(uid), ptr(pos), ptr(neg), T, layers, C.byref(adam), alphas, 1e-3, None, ptr(sc),
                                  need, None]
    before = e.E0.cpu().numpy().copy()
    bad = {'E0': (0, None), 'graph': (7, None), 'graph w': (7, C.byref(no_w)), 'uid': (8, None), 'pos': (9, None), 'neg': (10, None),
           'rule': (13, None), 'alphas': (14, None), 'scratch': (17, None), 'T 0': (11, 0), 'T -3': (11, -3), 'ld 0': (5, 0), 'ld 2': (5, 2),
           'ld 6': (5, 6), 'ld 260': (5, 260), 'n_users 0': (6, 0), 'n_users N': (6, U + N), 'layers -1': (12, -1), 'layers 5': (12, 5),
           'adam without P m': (1, None), 'adam without Q v': (4, None), 'momentum without Q s1': (3, None),
           'row-wise adagrad': (13, C.byref(rowwise)), 'an unknown rule': (13, C.byref(unknown)),
           'a misaligned table': (0, C.c_void_p(e.E0.data_ptr() + 4)), 'a misaligned slot': (2, C.c_void_p(e.state['P'][1].data_ptr() + 4))}
    for what, (at, value) in bad.items():
        args = list(good)
        args[at] = value
        if what.startswith('momentum'):
            args[13] = C.byref(momentum)
        assert lib().drx_lgcn_step(*args) == EINVAL, what
    small = list(good)
    small[18] = need // 2
    assert lib().drx_lgcn_step(*small) == ESCRATCH
    # drx_lgcn_final's own
    out = torch.full((U + N, e.ld), 777.0, device='cuda:0')
    fneed = int(lib().drx_lgcn_final_scratch_bytes(C.byref(g), e.ld))
    fgood = [ptr(e.E0), C.byref(g), layers, e.ld, ptr(out), ptr(sc), fneed, None]
    assert 0 < fneed <= need and lib().drx_lgcn_final_scratch_bytes(C.byref(g), 6) == 0
    fbad = {'E0': (0, None), 'graph': (1, None), 'layers -1': (2, -1), 'layers 5': (2, 5), 'ld 6': (3, 6), 'ld 260': (3, 260), 'out': (4, None),
            'out == E0': (4, ptr(e.E0)), 'scratch': (5, None), 'a misaligned out': (4, C.c_void_p(out.data_ptr() + 4))}
    for what, (at, value) in fbad.items():
        args = list(fgood)
        args[at] = value
        assert lib().drx_lgcn_final(*args) == EINVAL, what
    args = list(fgood)
    args[6] = 16
    assert lib().drx_lgcn_final(*args) == ESCRATCH
    torch.cuda.synchronize()
    assert np.array_equal(_bits(e.E0.cpu().numpy()), _bits(before)) and (out.cpu().numpy() == 777.0).all()
    assert not sc.cpu().numpy().any(), 'a refused call wrote its scratch'
    assert lib().drx_lgcn_step(*good) == 0 and lib().drx_lgcn_final(*fgood) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(_bits(e.E0.cpu().numpy()), _bits(before)) and np.isfinite(out.cpu().numpy()).all()


def test_engine_refuses_factors_and_layers_outside_its_domain():
    from drecpy_amd._lib import DrxError
    from drecpy_amd.engine_lgcn import LgcnEngine
    for K in (0, 257, 2.5):
        with pytest.raises(DrxError, match='factors'):
            LgcnEngine(U, N, K)
    for layers in (-1, 5, 1.5):
        with pytest.raises(DrxError, match='layers'):
            LgcnEngine(U, N, 8, layers)
    with pytest.raises(DrxError, match='set_graph'):
        LgcnEngine(U, N, 8, 1).final_embeddings()
