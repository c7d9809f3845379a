"""SASRec on the device against tests/sasrec_oracle.py (NumPy float64), through the C ABI (drx_sas_step, drx_sas_query_rows) and
drecpy_amd.engine_sas.SasEngine.  (The public class: tests/test_gpu_sasrec_api.py.)

The gate on ALL scores (every user's serving basket x every item) and on the loss is the project's, from tests/test_gpu_fpmc.py:

    err(GPU) <= max(1e-5, 4 err(replay)) * max(1, max |x|)

where the replay is the oracle itself on float32 arrays.  Every (GPU, replay) pair is printed (pytest -s); DESIGN.md section 3.12 has
the table.  The test weights are uniform(-0.5, 0.5) / sqrt(width) (biases: width 1) with LN gains 1 + uniform(-0.5, 0.5) and offsets
uniform(-0.5, 0.5), so the softmax is not flat and the LN gradients are exercised.  Rows of E, Q and b no window of a batch names are
compared bit for bit with an fp32 NumPy replay of their reg-only update."""
import ctypes as C

import numpy as np
import pytest

import bpr_oracle as bo
import sasrec_oracle as so
from test_gpu_bpr import _bits, _dev, _idle_replay
from test_gpu_fpmc import N, U, _batch, _gate, _serving_baskets
from test_gpu_gru import KINDS, _optimizer
from test_gru_oracle import hand_made_batch
from test_sasrec_oracle import dims_of

pytestmark = pytest.mark.gpu

F = np.float32
EINVAL, ESCRATCH = -1, -2
MAX_R = 16


def _engine(H, L, blocks, p, kind='adam', baskets=None):
    from drecpy_amd.engine_sas import SasEngine
    e = SasEngine(U, N, H, L, blocks)
    e.set_params(p)
    e.set_optimizer(_optimizer(kind, so.HP['lr']))
    e.reg = so.HP['reg']
    e.set_baskets(_serving_baskets(L) if baskets is None else baskets)
    return e


def _all_scores(e):
    return e.score_matrix(np.arange(U, dtype=np.int32)).cpu().numpy()


def _padding_is_zero(e):
    """the padding columns of E and Q and of the slots that start at zero; sw has none: it holds exactly the n_small logical entries"""
    assert e.sw.numel() == e.L * e.H + e.blocks * (5 * e.H * e.H + 6 * e.H) + 2 * e.H
    slots = [] if e.opt_kind == 'adagrad' else [(n, s) for n in ('E', 'Q') for s in e.state[n] if s is not None]
    for name, t in [('E', e.E), ('Q', e.Q)] + slots:
        assert not t.cpu().numpy()[:, e.H:].any(), f'a padding column of {name} moved'


def _check_idle_rows(e, kind, p0, before, after, alphas):
    """rows of E, Q and b that no window names: bit-equal to the fp32 replay of their reg-only update (parameters and slots)"""
    idle_e = np.setdiff1d(np.arange(N), before)
    idle_i = np.setdiff1d(np.arange(N), after)
    assert len(idle_e) >= 10 and len(idle_i) >= 10
    reg = so.HP['reg']
    for name, idle, l2c, alpha in (('E', idle_e, reg, alphas[0]), ('Q', idle_i, reg, alphas[2]), ('b', idle_i, 0.0, alphas[2])):
        start = p0[name].astype(F)[idle]
        forms = _idle_replay(kind, start, l2c, alpha)
        got = [getattr(e, name)] + list(e.state[name])
        for k, what in enumerate(('p', 's1', 's2')):
            if forms[0][k] is None:
                continue
            g = got[k].cpu().numpy()
            g = (g if name == 'b' else g[:, :e.H])[idle]
            same = np.logical_or.reduce([_bits(g) == _bits(f[k]) for f in forms])
            assert same.all(), f'{kind} {name} {what}: {int((~same).sum())} idle elements differ from the fp32 replay, first {np.argwhere(~same)[0]}'
        if kind in ('adam', 'momentum', 'nesterov') and l2c:
            assert (_bits(e.views()[name].cpu().numpy()[idle]) != _bits(start)).any(), f'{kind} {name}: the reg-only update moved nothing'


def _run_against_the_oracle(B, H, L, blocks, r, kind='adam', steps=10, batches=None, check_at=(0, 9), idle=True):
    p = so.init_params(np.random.default_rng(100 + H + L), N, H, L, blocks)
    p0 = {k: v.copy() for k, v in p.items()}
    p32 = so.replay32(p)
    st, st32 = so.init_state(p, kind), so.init_state(p32, kind)
    e = _engine(H, L, blocks, p, kind)
    baskets = e.baskets.cpu().numpy()
    what = f'B {B} H {H} L {L} blocks {blocks} r {r} {kind}'
    for s in range(steps):
        uid, before, after = batches[s] if batches is not None else _batch(B, L, r, 1000 * B + 10 * L + s)
        want = so.step(p, st, s, uid, before, after, kind)
        rep = so.step(p32, st32, s, uid, before, after, kind)
        got = e.step(s, uid, before, after, want_loss=True)
        _gate(f'{what} step {s} loss', got, want, rep)
        if s in check_at:
            _gate(f'{what} scores after {s + 1} step(s)', _all_scores(e), so.scores(p, baskets), so.scores(p32, baskets))
            _padding_is_zero(e)
        if s == 0 and idle:
            _check_idle_rows(e, kind, p0, before, after, e._step_sizes(0, (3, 0, 1, 2)))
    return e, p, st


def _cut(e, name):
    """(the engine tensor that holds oracle array `name`, its part of it)"""
    if name in ('E', 'Q'):
        return name, lambda a: a[:, :e.H]
    if name == 'b':
        return name, lambda a: a
    off, shape = e.slices[name]
    return 'sw', lambda a: a[off:off + int(np.prod(shape))].reshape(shape)


# LN of one column has zero variance, softmax over one key | padding columns, H no multiple of 4, a partial tile | a column tile
# boundary, full L | every limit at once | an item with more lookups than the update's split threshold
@pytest.mark.parametrize('H,L,blocks,r,B', [(1, 1, 1, 1, 1), (7, 3, 2, 2, 17), (17, 16, 1, 1, 16), (64, 16, 2, 16, 33), (33, 5, 2, 4, 257)])
def test_adam_steps_match_the_oracle_after_1_and_10_steps(H, L, blocks, r, B):
    e, p, st = _run_against_the_oracle(B, H, L, blocks, r)
    for name in so.names(blocks):                           # the slots too: Adam's m and v of every row and every small weight
        tensor, part = _cut(e, name)
        for k in range(2):
            scale = max(1e-30, float(np.max(np.abs(st[name][k]))))
            got = part(e.state[tensor][k].cpu().numpy())
            assert np.max(np.abs(got - st[name][k])) <= 1e-4 * scale, (name, k)


def test_a_workgroup_that_walks_two_windows_matches_the_oracle():
    from drecpy_amd._lib import lib
    B = 256 + 1                                             # one tile (a window) more than the grid holds workgroups
    assert lib().drx_sas_grid(B) == 256 and lib().drx_sas_grid(B - 1) == 256 and lib().drx_sas_grid(255) == 255
    _run_against_the_oracle(B, 8, 2, 1, 1)                  # after 1 and 10 steps, like every other row of the shape table


def test_hand_made_batches_match_the_oracle():
    H, L, blocks = 7, 3, 2
    uid, before, after = hand_made_batch(L)
    assert (before[0] == before[0, 0]).all() and 2 in before[1] and after[2, 0] == 2 and 2 in after[3, 1:]
    one_item = (np.zeros(2), np.array([[6, 6, 6], [6, 6, 6]]), np.array([[6, 2, 3], [1, 6, 0]]))
    for name, batch in (('the batch of the CPU test', (uid, before, after)), ('one item', one_item)):
        print(name)
        _run_against_the_oracle(len(batch[1]), H, L, blocks, 2, steps=2, batches=[batch, batch], check_at=(0, 1), idle=False)


@pytest.mark.parametrize('H,blocks', [(7, 2), (64, 1)])
@pytest.mark.parametrize('kind', KINDS)
def test_one_step_under_every_rule(kind, H, blocks):
    e, _, _ = _run_against_the_oracle(64, H, 3, blocks, 3, kind, steps=1, check_at=(0,))
    n = bo.oo.N_SLOTS[kind]
    for name in ('E', 'sw', 'Q', 'b'):
        assert [s is not None for s in e.state[name]] == [k < n for k in range(2)]


@pytest.mark.parametrize('H', [1, 7])
def test_padding_stays_zero_over_ten_steps(H):
    p = so.init_params(np.random.default_rng(3), N, H, 4, 2)
    e = _engine(H, 4, 2, p)
    for s in range(10):
        e.step(s, *_batch(64, 4, 3, 40 + s))
    _padding_is_zero(e)
    assert not np.array_equal(e.Q[:, :H].cpu().numpy(), p['Q'].astype(F)) and not np.array_equal(e.sw.cpu().numpy()[:4 * H],
                                                                                                  p['Pos'].astype(F).reshape(-1))


def test_the_same_inputs_give_the_same_bits():
    H, B, L, blocks, r = 33, 257, 3, 2, 5
    p = so.init_params(np.random.default_rng(1), N, H, L, blocks)
    runs = []
    for _ in range(2):
        e = _engine(H, L, blocks, p)
        losses = [e.step(s, *_batch(B, L, r, 5 + s), want_loss=True) for s in range(3)]
        runs.append([t.cpu().numpy().copy() for t in e.tensors().values()] + [x.cpu().numpy().copy() for n in e.state for x in e.state[n]]
                    + [np.array(losses), e._query_rows(_dev(np.arange(U), np.int32)).cpu().numpy()])
    assert all(np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)) for a, b in zip(*runs))
    assert not np.array_equal(runs[0][0][:, :H], p['E'].astype(F)) and not np.array_equal(runs[0][1][:L * H], p['Pos'].astype(F).reshape(-1))


# ---- the query rows --------------------------------------------------------------------------------------------------------------------
def _rows(e, users):
    return e._query_rows(_dev(np.asarray(users), np.int32)).cpu().numpy()


@pytest.mark.parametrize('H,blocks', [(1, 1), (7, 2), (17, 1), (64, 2)])
@pytest.mark.parametrize('L', [1, 4, 16])
def test_query_rows_match_the_oracle_for_every_basket_length(L, H, blocks):
    p = so.init_params(np.random.default_rng(9 + H), N, H, L, blocks)
    rng = np.random.default_rng(L)
    baskets = np.full((U, L), -1, np.int32)                 # user u holds min(u, L) items: every length 0 .. L (U > 16)
    for u in range(U):
        baskets[u, :min(u, L)] = rng.integers(0, N, size=min(u, L))
    assert U > L and sorted(set((baskets >= 0).sum(axis=1).tolist())) == list(range(L + 1))
    e = _engine(H, L, blocks, p, baskets=baskets)
    users = np.array(list(range(U)) + [L, 0, L], np.int32)
    got = _rows(e, users)
    assert got.shape == (len(users), e.ldh)
    _gate(f'query rows H {H} L {L} blocks {blocks}', got[:, :H], so.query_rows(p, baskets, users), so.query_rows(so.replay32(p), baskets, users))
    assert not got[:, H:].any(), 'a padding column of a query row is not zero'
    assert not got[0].any() and _bits(got[0]).max() == 0 and not got[-2].any(), 'an empty basket must give an exactly zero row'
    assert got[L, :H].any() and np.array_equal(_bits(got[L]), _bits(got[-1]))
    x = _all_scores(e)                                      # scores of an empty basket are b[i]
    assert np.array_equal(_bits(x[0]), _bits(e.b.cpu().numpy()))


def test_rows_do_not_depend_on_their_place_or_their_neighbours():
    H, L, blocks = 17, 4, 2
    p = so.init_params(np.random.default_rng(5), N, H, L, blocks)
    e = _engine(H, L, blocks, p, baskets=_serving_baskets(L, seed=3))
    users = np.arange(33) % U
    full = _rows(e, users)
    perm = np.random.default_rng(8).permutation(33)
    assert np.array_equal(_bits(_rows(e, users[perm])), _bits(full[perm]))
    for n in (1, 16, 17, 33):
        assert np.array_equal(_bits(_rows(e, users[:n])), _bits(full[:n])), n
    assert np.array_equal(_bits(_rows(e, users[::-1].copy())), _bits(full[::-1]))


@pytest.mark.parametrize('H,L,blocks', [(7, 3, 2), (64, 16, 2), (17, 16, 1)])
def test_a_full_baskets_row_is_the_h_the_step_wrote(H, L, blocks):
    """serving and the step run one forward function: the row of a full basket has the bits of the h the step wrote for that window
    (read from the step's scratch; the step runs SGD at rate 0 without regularisation, so the parameters stay what they were)"""
    from drecpy_amd import optimizers as op
    p = so.init_params(np.random.default_rng(12), N, H, L, blocks)
    _, before, after = _batch(U, L, 2, 77)
    e = _engine(H, L, blocks, p, baskets=before)
    e.set_optimizer(op.SGD(0.0))
    e.reg = 0.0
    start = [t.cpu().numpy().copy() for t in e.tensors().values()]
    e.step(0, np.zeros(U), before, after)
    assert all(np.array_equal(_bits(t.cpu().numpy()), _bits(s)) for t, s in zip(e.tensors().values(), start))
    h = e.step_hidden(U).cpu().numpy()
    rows = _rows(e, np.arange(U))
    assert rows[:, :H].any() and np.array_equal(_bits(rows), _bits(h))


def test_query_rows_refusals():
    import torch
    from drecpy_amd._lib import lib, ptr
    H, L, blocks = 7, 3, 2
    e = _engine(H, L, blocks, so.init_params(np.random.default_rng(2), N, H, L, blocks))
    uid = _dev(np.arange(4), np.int32)
    out = torch.full((4, e.ldh + 4), -7.0, dtype=torch.float32, device='cuda:0')
    good = [ptr(e.E), ptr(e.sw), C.byref(e.dims), ptr(e.baskets), ptr(uid), 4, ptr(out), None]
    wrong = dims_of(H, L, blocks, N)
    wrong.off_vec += 4
    bad = {'E': (0, None), 'sw': (1, None), 'D': (2, None), 'baskets': (3, None), 'uid': (4, None), 'out': (6, None), 'n 0': (5, 0),
           'L 0': (2, C.byref(dims_of(H, 0, blocks, N))), 'L 17': (2, C.byref(dims_of(H, 17, blocks, N))),
           'blocks 3': (2, C.byref(dims_of(H, L, 3, N))), 'an offset off the layout': (2, C.byref(wrong)),
           'h 65': (2, C.byref(dims_of(65, L, blocks, N))), 'a misaligned out': (6, C.c_void_p(out.data_ptr() + 4)),
           'a misaligned E': (0, C.c_void_p(e.E.data_ptr() + 4))}
    for what, (at, value) in bad.items():
        args = list(good)
        args[at] = value
        assert lib().drx_sas_query_rows(*args) == EINVAL, what
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()
    assert lib().drx_sas_query_rows(*good) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy().reshape(-1)[:4 * e.ldh] != -7.0).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_step_refusals_leave_the_parameters_and_slots_alone():
    import torch
    from drecpy_amd import _lib
    from drecpy_amd._lib import lib, ptr
    H, B, L, blocks, r = 12, 16, 2, 2, 3
    p = so.init_params(np.random.default_rng(2), N, H, L, blocks)
    e = _engine(H, L, blocks, p)
    _, before, after = (_dev(a, np.int32) for a in _batch(B, L, r, 3))
    need = int(lib().drx_sas_step_scratch_bytes(C.byref(e.dims), B, r))
    assert need > 0
    sc = torch.zeros(need, dtype=torch.uint8, device='cuda:0')
    alphas = (C.c_float * 3)(1e-2, 1e-2, 1e-2)
    names = ('E', 'sw', 'Q', 'b')
    slots = [ptr(s) for n in names for s in e.state[n]]                           # E m, E v, sw m, sw v, Q m, Q v, b m, b v
    adam, momentum = _lib.OptRule(0, 0.0, 0.9, 0.999, 1e-7), _lib.OptRule(4, 0.0, 0.9, 0.0, 0.0)
    rowwise, unknown = _lib.OptRule(2, 0.0, 0.0, 0.0, 1e-7), _lib.OptRule(99, 0.0, 0.0, 0.0, 0.0)
    good = [C.byref(e.dims), ptr(e.E), ptr(e.sw), ptr(e.Q), ptr(e.b)] + slots + [ptr(before), ptr(after), B, r, C.byref(adam), alphas, 1e-3,
                                                                                 None, ptr(sc), need, None]

    def dims(**change):
        d = dims_of(H, L, blocks, N)
        for k, v in change.items():
            setattr(d, k, v)
        return C.byref(d)

    d0 = dims_of(H, L, blocks, N)
    bad = {'D': (0, None), 'E': (1, None), 'sw': (2, None), 'Q': (3, None), 'b': (4, None), 'before': (13, None), 'after': (14, None),
           'rule': (17, None), 'alphas': (18, None), 'scratch': (21, None), 'B 0': (15, 0), 'B -3': (15, -3), 'B 2^24': (15, 1 << 24),
           'r 0': (16, 0), 'r 17': (16, MAX_R + 1),
           'h 0': (0, C.byref(dims_of(0, L, blocks, N))), 'h 65': (0, C.byref(dims_of(65, L, blocks, N))),
           'L 0': (0, C.byref(dims_of(H, 0, blocks, N))), 'L 17': (0, C.byref(dims_of(H, 17, blocks, N))),
           'blocks 0': (0, C.byref(dims_of(H, L, 0, N))), 'blocks 3': (0, C.byref(dims_of(H, L, 3, N))),
           'n_items 0': (0, dims(n_items=0)), 'ldh': (0, dims(ldh=d0.ldh + 4)), 'off_pos': (0, dims(off_pos=4)),
           'off_blk': (0, dims(off_blk=d0.off_blk + 4)), 'off_vec': (0, dims(off_vec=d0.off_vec + 4)),
           'off_lnf': (0, dims(off_lnf=d0.off_lnf + 4)), 'n_small': (0, dims(n_small=d0.n_small + 4)),
           'adam without E m': (5, None), 'adam without sw v': (8, None), 'adam without Q m': (9, None), 'adam without b v': (12, None),
           'momentum without sw s1': (7, None), 'row-wise adagrad': (17, C.byref(rowwise)), 'an unknown rule': (17, C.byref(unknown)),
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
            args[17] = C.byref(momentum)
        assert lib().drx_sas_step(*args) == EINVAL, what
        nothing_changed(what)
    small = list(good)
    small[22] = need // 2
    assert lib().drx_sas_step(*small) == ESCRATCH
    nothing_changed('too small a scratch')
    assert lib().drx_sas_step(*good) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(_bits(e.E.cpu().numpy()), _bits(start[0])) and not np.array_equal(_bits(e.sw.cpu().numpy()), _bits(start[1]))


def test_engine_refuses_shapes_outside_its_domain():
    from drecpy_amd._lib import DrxError
    from drecpy_amd.engine_sas import SasEngine
    for H in (0, 65, 2.5):
        with pytest.raises(DrxError, match='hidden must'):
            SasEngine(U, N, H, 1, 1)
    for L in (0, 17):
        with pytest.raises(DrxError, match='L must'):
            SasEngine(U, N, 4, L, 1)
    for blocks in (0, 3, True):
        with pytest.raises(DrxError, match='blocks must'):
            SasEngine(U, N, 4, 2, blocks)
    e = _engine(4, 2, 2, so.init_params(np.random.default_rng(0), N, 4, 2, 2))
    with pytest.raises(DrxError, match='outside its'):
        e.step(0, *_batch(8, 2, MAX_R + 1, 0))
    with pytest.raises(DrxError, match='baskets'):
        e.set_baskets(np.full((U, 2), N))
    assert e.rank_ld() == 4 and e.EPILOGUE is not None
    assert list(e.views()) == so.names(2)
    shapes = {'E': (N, 4), 'Pos': (2, 4), 'Q': (N, 4), 'b': (N,)}
    assert {k: tuple(v.shape) for k, v in e.views().items()} == \
        {k: shapes.get(k, (4, 4) if k[:2] in ('Wq', 'Wk', 'Wv', 'W1', 'W2') else (4,)) for k in so.names(2)}
