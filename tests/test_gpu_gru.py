"""GRU4Rec on the device against tests/gru_oracle.py (NumPy float64), through the C ABI (drx_gru_step, drx_gru_query_rows) and
drecpy_amd.engine_gru.GruEngine.  (The public class: tests/test_gpu_gru_api.py.)

The gate on ALL scores (every user's serving basket x every item) and on the loss is the project's, from tests/test_gpu_fpmc.py:

    err(GPU) <= max(1e-5, 4 err(replay)) * max(1, max |x|)

where the replay is the oracle itself on float32 arrays.  Every (GPU, replay) pair is printed (pytest -s); DESIGN.md section 3.11 has
the table.  The test weights are uniform(-0.5, 0.5) / sqrt(width) (biases: width 1), so the gates leave the linear range of sigmoid and
tanh and scores are O(0.1 - 1).  Rows of E, Q and b no window of a batch names are compared bit for bit with an fp32 NumPy replay of
their reg-only update."""
import ctypes as C

import numpy as np
import pytest

import bpr_oracle as bo
import gru_oracle as go
from test_gpu_bpr import _bits, _dev, _idle_replay
from test_gpu_fpmc import N, N_POOL, U, _batch, _gate, _serving_baskets
from test_gru_oracle import dims_of, hand_made_batch

pytestmark = pytest.mark.gpu

F = np.float32
EINVAL, ESCRATCH = -1, -2
MAX_R = 16
KINDS = ('adam', 'adagrad', 'sgd', 'momentum', 'nesterov', 'rmsprop', 'rmsprop_momentum')      # Baseline._base._DENSE_KINDS


def _optimizer(kind, lr):
    from drecpy_amd import optimizers as op
    hp = bo.HP
    return {'adam': lambda: op.Adam(lr), 'adagrad': lambda: op.Adagrad(lr), 'sgd': lambda: op.SGD(lr), 'momentum': lambda: op.SGD(lr, hp['mu']),
            'nesterov': lambda: op.SGD(lr, hp['mu'], nesterov=True), 'rmsprop': lambda: op.RMSprop(lr, hp['rho']),
            'rmsprop_momentum': lambda: op.RMSprop(lr, hp['rho'], hp['mu'], hp['eps'])}[kind]()


def _engine(K, H, L, p, kind='adam', baskets=None):
    from drecpy_amd.engine_gru import GruEngine
    e = GruEngine(U, N, K, H, L)
    e.set_params(p)
    e.set_optimizer(_optimizer(kind, go.HP['lr']))
    e.reg = go.HP['reg']
    e.set_baskets(_serving_baskets(L) if baskets is None else baskets)
    return e


def _all_scores(e):
    return e.score_matrix(np.arange(U, dtype=np.int32)).cpu().numpy()


def _padding_is_zero(e):
    """the padding columns of E and Q and of the slots that start at zero; sw has none: it holds exactly the n_small logical entries"""
    assert e.sw.numel() == 3 * (e.K + e.H) * e.H + 4 * e.H
    slots = [] if e.opt_kind == 'adagrad' else [(n, s) for n in ('E', 'Q') for s in e.state[n] if s is not None]
    for name, t in [('E', e.E), ('Q', e.Q)] + slots:
        a = t.cpu().numpy()
        assert not a[:, e.K if name == 'E' else e.H:].any(), f'a padding column of {name} moved'


def _check_idle_rows(e, kind, p0, before, after, alphas):
    """rows of E, Q and b that no window names: bit-equal to the fp32 replay of their reg-only update (parameters and slots)"""
    idle_e = np.setdiff1d(np.arange(N), before)
    idle_i = np.setdiff1d(np.arange(N), after)
    assert len(idle_e) >= 10 and len(idle_i) >= 10
    reg = go.HP['reg']
    cut = {'E': slice(0, e.K), 'Q': slice(0, e.H), 'b': None}
    for name, idle, l2c, alpha in (('E', idle_e, reg, alphas[0]), ('Q', idle_i, reg, alphas[2]), ('b', idle_i, 0.0, alphas[2])):
        start = p0[name].astype(F)[idle]
        forms = _idle_replay(kind, start, l2c, alpha)
        got = [getattr(e, name)] + list(e.state[name])
        for k, what in enumerate(('p', 's1', 's2')):
            if forms[0][k] is None:
                continue
            g = got[k].cpu().numpy()
            g = (g if cut[name] is None else g[:, cut[name]])[idle]
            same = np.logical_or.reduce([_bits(g) == _bits(f[k]) for f in forms])
            assert same.all(), f'{kind} {name} {what}: {int((~same).sum())} idle elements differ from the fp32 replay, first {np.argwhere(~same)[0]}'
        if kind in ('adam', 'momentum', 'nesterov') and l2c:
            assert (_bits(e.views()[name].cpu().numpy()[idle]) != _bits(start)).any(), f'{kind} {name}: the reg-only update moved nothing'


def _run_against_the_oracle(B, K, H, L, r, kind='adam', steps=10, batches=None, check_at=(0, 9), idle=True):
    p = go.init_params(np.random.default_rng(100 + K + H), N, K, H)
    p0 = {k: v.copy() for k, v in p.items()}
    p32 = go.replay32(p)
    st, st32 = go.init_state(p, kind), go.init_state(p32, kind)
    e = _engine(K, H, L, p, kind)
    baskets = e.baskets.cpu().numpy()
    what = f'B {B} K {K} H {H} L {L} r {r} {kind}'
    for s in range(steps):
        uid, before, after = batches[s] if batches is not None else _batch(B, L, r, 1000 * B + 10 * L + s)
        want = go.step(p, st, s, uid, before, after, kind)
        rep = go.step(p32, st32, s, uid, before, after, kind)
        got = e.step(s, uid, before, after, want_loss=True)
        _gate(f'{what} step {s} loss', got, want, rep)
        if s in check_at:
            _gate(f'{what} scores after {s + 1} step(s)', _all_scores(e), go.scores(p, baskets), go.scores(p32, baskets))
            _padding_is_zero(e)
        if s == 0 and idle:
            _check_idle_rows(e, kind, p0, before, after, e._step_sizes(0, (3, 0, 1, 2)))
    return e, p, st


# degenerate widths | padding, 3 H = 21 no multiple of 16 or 4, a partial tile | a gate block that crosses a 16-column tile | every limit
# at once | K != H at two waves' worth of columns
@pytest.mark.parametrize('K,H,L,r,B', [(1, 1, 1, 1, 1), (5, 7, 3, 2, 17), (16, 17, 2, 1, 16), (64, 64, 8, 16, 33), (64, 33, 5, 4, 257)])
def test_adam_steps_match_the_oracle_after_1_and_10_steps(K, H, L, r, B):
    e, p, st = _run_against_the_oracle(B, K, H, L, r)
    cut = {'E': ('E', lambda a: a[:, :K]), 'Q': ('Q', lambda a: a[:, :H]), 'b': ('b', lambda a: a)}
    cut.update({n: ('sw', lambda a, n=n: a[e.slices[n][0]:e.slices[n][0] + int(np.prod(e.slices[n][1]))].reshape(e.slices[n][1])) for n in go.SMALL})
    for name in go.NAMES:                                   # the slots too: Adam's m and v of every row and every small weight
        for k in range(2):
            scale = max(1e-30, float(np.max(np.abs(st[name][k]))))
            got = cut[name][1](e.state[cut[name][0]][k].cpu().numpy())
            assert np.max(np.abs(got - st[name][k])) <= 1e-4 * scale, (name, k)


def test_a_workgroup_that_walks_two_tiles_matches_the_oracle():
    from drecpy_amd._lib import lib
    B = 16 * 256 + 1                                        # one tile more than the grid holds workgroups
    assert lib().drx_gru_grid(B) == 256 and lib().drx_gru_grid(B - 1) == 256 and lib().drx_gru_grid(16 * 255) == 255
    _run_against_the_oracle(B, 8, 8, 2, 1)                  # after 1 and 10 steps, like every other row of the shape table


def test_hand_made_batches_match_the_oracle():
    K, H, L = 5, 7, 3
    uid, before, after = hand_made_batch(L)
    assert (before[0] == before[0, 0]).all() and 2 in before[1] and after[2, 0] == 2 and 2 in after[3, 1:]
    one_item = (np.zeros(2), np.array([[6, 6, 6], [6, 6, 6]]), np.array([[6, 2, 3], [1, 6, 0]]))
    for name, batch in (('the batch of the CPU test', (uid, before, after)), ('one item', one_item)):
        print(name)
        _run_against_the_oracle(len(batch[1]), K, H, L, 2, steps=2, batches=[batch, batch], check_at=(0, 1), idle=False)


@pytest.mark.parametrize('K,H', [(5, 7), (64, 64)])
@pytest.mark.parametrize('kind', KINDS)
def test_one_step_under_every_rule(kind, K, H):
    e, _, _ = _run_against_the_oracle(64, K, H, 2, 3, kind, steps=1, check_at=(0,))
    n = bo.oo.N_SLOTS[kind]
    for name in ('E', 'sw', 'Q', 'b'):
        assert [s is not None for s in e.state[name]] == [k < n for k in range(2)]


@pytest.mark.parametrize('K,H', [(1, 1), (5, 7)])
def test_padding_stays_zero_over_ten_steps(K, H):
    p = go.init_params(np.random.default_rng(3), N, K, H)
    e = _engine(K, H, 4, p)
    for s in range(10):
        e.step(s, *_batch(64, 4, 3, 40 + s))
    _padding_is_zero(e)
    assert not np.array_equal(e.E[:, :K].cpu().numpy(), p['E'].astype(F)) and not np.array_equal(e.sw.cpu().numpy()[:3 * K * H],
                                                                                                  p['Wx'].astype(F).reshape(-1))


def test_the_same_inputs_give_the_same_bits():
    K, H, B, L, r = 20, 33, 257, 3, 5
    p = go.init_params(np.random.default_rng(1), N, K, H)
    runs = []
    for _ in range(2):
        e = _engine(K, H, L, p)
        losses = [e.step(s, *_batch(B, L, r, 5 + s), want_loss=True) for s in range(3)]
        runs.append([t.cpu().numpy().copy() for t in e.tensors().values()] + [x.cpu().numpy().copy() for n in e.state for x in e.state[n]]
                    + [np.array(losses), e._query_rows(_dev(np.arange(U), np.int32)).cpu().numpy()])
    assert all(np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)) for a, b in zip(*runs))
    assert not np.array_equal(runs[0][0][:, :K], p['E'].astype(F)) and not np.array_equal(runs[0][1][:3 * K * H], p['Wx'].astype(F).reshape(-1))


# ---- the query rows --------------------------------------------------------------------------------------------------------------------
def _rows(e, users):
    return e._query_rows(_dev(np.asarray(users), np.int32)).cpu().numpy()


@pytest.mark.parametrize('K,H', [(1, 1), (5, 7), (16, 17), (64, 64), (64, 33)])
@pytest.mark.parametrize('L', [1, 4, 8])
def test_query_rows_match_the_oracle_for_every_basket_length(L, K, H):
    p = go.init_params(np.random.default_rng(9 + K), N, K, H)
    baskets = _serving_baskets(L, seed=L)                   # user 0 empty, 1 one item, 2 L - 1 items, 3 full, the others random lengths
    e = _engine(K, H, L, p, baskets=baskets)
    users = np.array(list(range(U)) + [3, 0, 3], np.int32)
    got = _rows(e, users)
    assert got.shape == (len(users), e.ldh)
    _gate(f'query rows K {K} H {H} L {L}', got[:, :H], go.query_rows(p, baskets, users), go.query_rows(go.replay32(p), baskets, users))
    assert not got[:, H:].any(), 'a padding column of a query row is not zero'
    assert not got[0].any() and _bits(got[0]).max() == 0 and not got[-2].any(), 'an empty basket must give an exactly zero row'
    assert got[3, :H].any() and np.array_equal(_bits(got[3]), _bits(got[-1]))
    # scores of an empty basket are b[i]
    x = _all_scores(e)
    assert np.array_equal(_bits(x[0]), _bits(e.b.cpu().numpy()))


@pytest.mark.parametrize('K,H', [(5, 7), (64, 64)])
def test_a_short_basket_gives_the_bits_of_a_shorter_engine(K, H):
    L = 5
    p = go.init_params(np.random.default_rng(4), N, K, H)
    rng = np.random.default_rng(6)
    items = rng.integers(0, N, size=(U, L)).astype(np.int32)
    for m in range(1, L):
        baskets = items.copy()
        baskets[:, m:] = -1
        long_, short = _engine(K, H, L, p, baskets=baskets), _engine(K, H, m, p, baskets=items[:, :m].copy())
        a, b = _rows(long_, np.arange(U)), _rows(short, np.arange(U))
        assert a[:, :H].any() and np.array_equal(_bits(a), _bits(b)), m


def test_rows_do_not_depend_on_their_place_or_their_neighbours():
    K, H, L = 16, 17, 4
    p = go.init_params(np.random.default_rng(5), N, K, H)
    e = _engine(K, H, L, p, baskets=_serving_baskets(L, seed=3))
    users = np.arange(33) % U                               # 33 request rows: three tiles, the last with one row
    full = _rows(e, users)
    perm = np.random.default_rng(8).permutation(33)
    assert np.array_equal(_bits(_rows(e, users[perm])), _bits(full[perm]))
    for n in (1, 16, 17, 33):
        assert np.array_equal(_bits(_rows(e, users[:n])), _bits(full[:n])), n
    assert np.array_equal(_bits(_rows(e, users[::-1].copy())), _bits(full[::-1]))


def test_query_rows_refusals():
    import torch
    from drecpy_amd._lib import lib, ptr
    K, H, L = 5, 7, 3
    e = _engine(K, H, L, go.init_params(np.random.default_rng(2), N, K, H))
    uid = _dev(np.arange(4), np.int32)
    out = torch.full((4, e.ldh + 4), -7.0, dtype=torch.float32, device='cuda:0')
    good = [ptr(e.E), ptr(e.sw), C.byref(e.dims), ptr(e.baskets), L, ptr(uid), 4, ptr(out), None]
    wrong = dims_of(K, H, N)
    wrong.off_wh += 4
    wide = dims_of(K, 65, N)
    bad = {'E': (0, None), 'sw': (1, None), 'D': (2, None), 'baskets': (3, None), 'uid': (5, None), 'out': (7, None), 'n 0': (6, 0),
           'L 0': (4, 0), 'L 9': (4, 9), 'an offset off the layout': (2, C.byref(wrong)), 'h 65': (2, C.byref(wide)),
           'a misaligned out': (7, C.c_void_p(out.data_ptr() + 4)), 'a misaligned E': (0, C.c_void_p(e.E.data_ptr() + 4))}
    for what, (at, value) in bad.items():
        args = list(good)
        args[at] = value
        assert lib().drx_gru_query_rows(*args) == EINVAL, what
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()
    assert lib().drx_gru_query_rows(*good) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy().reshape(-1)[:4 * e.ldh] != -7.0).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_step_refusals_leave_the_parameters_and_slots_alone():
    import torch
    from drecpy_amd import _lib
    from drecpy_amd._lib import lib, ptr
    K, H, B, L, r = 8, 12, 16, 2, 3
    p = go.init_params(np.random.default_rng(2), N, K, H)
    e = _engine(K, H, L, p)
    _, before, after = (_dev(a, np.int32) for a in _batch(B, L, r, 3))
    need = int(lib().drx_gru_step_scratch_bytes(C.byref(e.dims), B, L, r))
    assert need > 0
    sc = torch.zeros(need, dtype=torch.uint8, device='cuda:0')
    alphas = (C.c_float * 3)(1e-2, 1e-2, 1e-2)
    names = ('E', 'sw', 'Q', 'b')
    slots = [ptr(s) for n in names for s in e.state[n]]                           # E m, E v, sw m, sw v, Q m, Q v, b m, b v
    adam, momentum = _lib.OptRule(0, 0.0, 0.9, 0.999, 1e-7), _lib.OptRule(4, 0.0, 0.9, 0.0, 0.0)
    rowwise, unknown = _lib.OptRule(2, 0.0, 0.0, 0.0, 1e-7), _lib.OptRule(99, 0.0, 0.0, 0.0, 0.0)
    good = [C.byref(e.dims), ptr(e.E), ptr(e.sw), ptr(e.Q), ptr(e.b)] + slots + [ptr(before), ptr(after), B, L, r, C.byref(adam), alphas, 1e-3,
                                                                                 None, ptr(sc), need, None]

    def dims(**change):
        d = dims_of(K, H, N)
        for k, v in change.items():
            setattr(d, k, v)
        return C.byref(d)

    d0 = dims_of(K, H, N)
    bad = {'D': (0, None), 'E': (1, None), 'sw': (2, None), 'Q': (3, None), 'b': (4, None), 'before': (13, None), 'after': (14, None),
           'rule': (18, None), 'alphas': (19, None), 'scratch': (22, None), 'B 0': (15, 0), 'B -3': (15, -3), 'L 0': (16, 0), 'L 9': (16, 9),
           'r 0': (17, 0), 'r 17': (17, MAX_R + 1),
           'k 0': (0, C.byref(dims_of(0, H, N))), 'k 65': (0, C.byref(dims_of(65, H, N))), 'h 0': (0, C.byref(dims_of(K, 0, N))),
           'h 65': (0, C.byref(dims_of(K, 65, N))), 'n_items 0': (0, dims(n_items=0)), 'ldk': (0, dims(ldk=d0.ldk + 4)),
           'ldh': (0, dims(ldh=d0.ldh + 4)), 'off_wx': (0, dims(off_wx=4)), 'off_wh': (0, dims(off_wh=d0.off_wh + 4)),
           'off_bx': (0, dims(off_bx=d0.off_bx + 4)), 'off_bhn': (0, dims(off_bhn=d0.off_bhn + 4)), 'n_small': (0, dims(n_small=d0.n_small + 4)),
           'adam without E m': (5, None), 'adam without sw v': (8, None), 'adam without Q m': (9, None), 'adam without b v': (12, None),
           'momentum without sw s1': (7, None), 'row-wise adagrad': (18, C.byref(rowwise)), 'an unknown rule': (18, C.byref(unknown)),
           'a misaligned E': (1, C.c_void_p(e.E.data_ptr() + 4)), 'a misaligned Q': (3, C.c_void_p(e.Q.data_ptr() + 8)),
           'a misaligned slot of E': (5, C.c_void_p(e.state['E'][0].data_ptr() + 4))}
    held = list(e.tensors().values()) + [s for n in names for s in e.state[n]]
    start = [t.cpu().numpy().copy() for t in held]

    def nothing_changed(what):
        torch.cuda.synchronize()
        for t, b in zip(held, start):
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(b)), what
        assert not sc.cpu().numpy().any(), f'{what}: a refused call wrote its scratch'

    for what, (at, value) in bad.items():
        args = list(good)
        args[at] = value
        if what.startswith('momentum'):
            args[18] = C.byref(momentum)
        assert lib().drx_gru_step(*args) == EINVAL, what
        nothing_changed(what)
    small = list(good)
    small[23] = need // 2
    assert lib().drx_gru_step(*small) == ESCRATCH
    nothing_changed('too small a scratch')
    assert lib().drx_gru_step(*good) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(_bits(e.E.cpu().numpy()), _bits(start[0])) and not np.array_equal(_bits(e.sw.cpu().numpy()), _bits(start[1]))


def test_engine_refuses_shapes_outside_its_domain():
    from drecpy_amd._lib import DrxError
    from drecpy_amd.engine_gru import GruEngine
    for H in (0, 65, 2.5):
        with pytest.raises(DrxError, match='hidden'):
            GruEngine(U, N, 4, H, 1)
    for K in (0, 65):
        with pytest.raises(DrxError, match='factors'):
            GruEngine(U, N, K, 4, 1)
    for L in (0, 9):
        with pytest.raises(DrxError, match='L must'):
            GruEngine(U, N, 4, 4, L)
    e = _engine(4, 4, 2, go.init_params(np.random.default_rng(0), N, 4, 4))
    with pytest.raises(DrxError, match='outside its'):
        e.step(0, *_batch(8, 2, MAX_R + 1, 0))
    with pytest.raises(DrxError, match='baskets'):
        e.set_baskets(np.full((U, 2), N))
    assert e.rank_ld() == 4 and e.EPILOGUE is not None
    assert list(e.views()) == ['E', 'Wx', 'Wh', 'bx', 'bhn', 'Q', 'b']
    assert {k: tuple(v.shape) for k, v in e.views().items()} == {'E': (N, 4), 'Wx': (4, 12), 'Wh': (4, 12), 'bx': (12,), 'bhn': (4,),
                                                                  'Q': (N, 4), 'b': (N,)}
