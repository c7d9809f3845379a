"""NeuMF on the device against tests/ncf_oracle.py (NumPy float64), through the C ABI (drx_ncf_step, drx_ncf_half_rows,
drx_ncf_score_rows, drx_ncf_pair_scores) and the public class (drecpy_amd.Recommender.Baseline.NeuMF).

The gate on ALL n_users x n_items logits and on the loss is the project's own

    err(GPU) <= max(1e-5, 4 err(replay)) * max(1, max |x|)

where the replay is the oracle itself on float32 arrays (gradients formed in float32, every stored value rounded to float32).  Every
(GPU, replay) pair is printed (pytest -s); DESIGN.md section 3.10 has the table.  Biases start at non-zero random values; every run
asserts that the smallest |z| over all hidden pre-activations the oracle evaluated is >= 1e-6 — a condition on the inputs (the seeds
were chosen on the CPU with the oracle), not a tolerance: relu's kink is where fp32 and float64 may part by a whole gradient."""
import ctypes as C
import functools

import numpy as np
import pytest

import bpr_oracle as bo
import ncf_oracle as no
from oracle.data_oracle import point_sample_counter
from test_gpu_bpr import _bits, _dev, _idle_replay, _optimizer

pytestmark = pytest.mark.gpu

U, N, THR = 23, 41, 1.0
F = np.float32
D = np.float64
EINVAL, ESCRATCH = -1, -2
MIN_Z = 1e-6
DEFAULT = (8, 32, (32, 16, 8))
WIDEST = (64, 64, (64, 64, 64, 64))


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


def _batch(B, seed):
    """B point samples in which users and items repeat; from 5 samples on, samples 0 and 1 are the same pair with both targets and
    sample 2 shares its item with them; from 257 on item 7 is looked up by 100 samples (more than the update's split threshold)"""
    rng = np.random.default_rng(seed)
    uid, iid = rng.choice(USER_POOL, size=B), rng.integers(0, N_POOL, size=B)
    y = rng.integers(0, 2, size=B).astype(F)
    if B >= 5:
        uid[1], iid[1], iid[2] = uid[0], iid[0], iid[0]
        y[0], y[1] = 1.0, 0.0
    if B >= 257:
        iid[rng.choice(np.arange(4, B), size=100, replace=False)] = 7
    return uid.astype(np.int32), iid.astype(np.int32), y


def _params(shape, seed=0, n_items=N):
    Kg, Km, layers = shape
    return no.init_params(np.random.default_rng(100 + 7 * Kg + Km + len(layers) + 1000 * seed), U, n_items, Kg, Km, layers)


# The weights' seed per case, where seed 0 puts a pre-activation of the oracle within 1e-6 of relu's kink (found on the CPU with the oracle:
# the first seed 0, 1, 2, ... whose run keeps the margin; the widest shapes evaluate half a million pre-activations per run).
STEP_SEEDS = {(16, (8, 32, (32, 16, 8)), 'adam'): 1, (17, (5, 5, (17, 16)), 'adam'): 1, (64, (64, 64, (64, 64, 64, 64)), 'adam'): 25,
              (257, (64, 64, (64, 64, 64, 64)), 'adam'): 18, (1, (64, 64, (64, 64, 64, 64)), 'adam'): 5,
              (4113, (5, 5, (17, 16)), 'adam'): 4, (4113, (8, 32, (32, 16, 8)), 'adam'): 3}
SERVE_SEEDS = {((8, 32, (32, 16, 8)), 16): 1, ((8, 32, (32, 16, 8)), 257): 1, ((64, 64, (64, 64, 64, 64)), 41): 1,
               ((64, 64, (64, 64, 64, 64)), 257): 15}
FIT_SEED = 42


@functools.lru_cache(maxsize=None)
def _oracle_run(B, shape, kind='adam', steps=10, check_at=(0, 9)):
    """The oracle and its float32 replay over `steps` steps on _batch(B, .): per step the two losses, at check_at all logits of both, the
    final parameters and Adam state, and the smallest |z| evaluated.  Computed once per case and left unchanged."""
    p = _params(shape, STEP_SEEDS.get((B, shape, kind), 0))
    p0 = {k: v.copy() for k, v in p.items()}
    p32 = no.replay32(p)
    st, st32 = no.init_state(p, kind), no.init_state(p32, kind)
    no.reset_seen()
    out = {'p0': p0, 'batches': [], 'loss': [], 'logits': {}}
    for s in range(steps):
        batch = _batch(B, 1000 * B + s)
        out['batches'].append(batch)
        out['loss'].append((no.step(p, st, s, *batch, kind), no.step(p32, st32, s, *batch, kind)))
        if s in check_at:
            out['logits'][s] = (no.logits(p), no.logits(p32))
    out.update(p=p, state=st, min_abs_z=no.seen['min_abs_z'])
    return out


def _engine(shape, p, kind='adam', n_items=N):
    from drecpy_amd.engine_ncf import NcfEngine
    Kg, Km, layers = shape
    e = NcfEngine(U, n_items, Kg, Km, layers)
    e.set_params(p)
    e.set_optimizer(_optimizer(kind, no.HP['lr']))
    e.reg = no.HP['reg']
    return e


def _tables(e):
    """{oracle name: numpy view of the device parameter}, and the same for the two slots"""
    Kg, Km, ldg = e.Kg, e.Km, e.ldg
    cut = {'Pg': ('U', slice(0, Kg)), 'Pm': ('U', slice(ldg, ldg + Km)), 'Qg': ('V', slice(0, Kg)), 'Qm': ('V', slice(ldg, ldg + Km))}

    def view(tensors):
        out = {}
        for n, (t, c) in cut.items():
            out[n] = None if tensors[t] is None else tensors[t].cpu().numpy()[:, c]
        for n, (off, shp) in e.slices.items():
            out[n] = None if tensors['sw'] is None else tensors['sw'].cpu().numpy()[off:off + int(np.prod(shp))].reshape(shp)
        return out
    return view(e.tensors()), [view({k: e.state[k][s] for k in e.state}) for s in range(2)]


def _padding_is_zero(e):
    """the padding columns of both halves of both tables, and of the slots that start at zero"""
    slots = [] if e.opt_kind == 'adagrad' else [s for n in ('U', 'V') for s in e.state[n] if s is not None]
    for t in [e.U, e.V] + slots:
        a = t.cpu().numpy()
        assert not a[:, e.Kg:e.ldg].any() and not a[:, e.ldg + e.Km:].any(), 'a padding column moved'


def _all_logits(e):
    return e.score_matrix(np.arange(U, dtype=np.int32)).cpu().numpy()


def _check_idle_rows(e, kind, p0, uid, iid, alphas):
    """rows of both tables that no sample names: bit-equal to the fp32 replay of their reg-only update (parameters and slots)"""
    idle_u, idle_i = np.setdiff1d(np.arange(U), uid), np.setdiff1d(np.arange(N), iid)
    assert len(idle_u) >= 13 and len(idle_i) >= 10
    tabs, slots = _tables(e)
    reg = no.HP['reg']
    for name, idle, alpha in (('Pg', idle_u, alphas[0]), ('Pm', idle_u, alphas[0]), ('Qg', idle_i, alphas[1]), ('Qm', idle_i, alphas[1])):
        start = p0[name].astype(F)[idle]
        forms = _idle_replay(kind, start, reg, alpha)
        got = [tabs[name], slots[0][name], slots[1][name]]
        for k, what in enumerate(('p', 's1', 's2')):
            if forms[0][k] is None:
                continue
            g = got[k][idle]
            same = np.logical_or.reduce([_bits(g) == _bits(f[k]) for f in forms])
            assert same.all(), f'{kind} {name} {what}: {int((~same).sum())} idle elements differ from the fp32 replay, first {np.argwhere(~same)[0]}'
        if kind in ('adam', 'momentum', 'nesterov'):
            assert (_bits(got[0][idle]) != _bits(start)).any(), f'{kind} {name}: the reg-only update moved nothing'


def _run_against_the_oracle(B, shape, kind='adam', steps=10, check_at=(0, 9)):
    o = _oracle_run(B, shape, kind, steps, check_at)
    print(f'smallest |z| the oracle evaluated: {o["min_abs_z"]:.3e}')
    assert o['min_abs_z'] >= MIN_Z, 'a pre-activation of the oracle sits at the kink: the inputs of this case must change'
    e = _engine(shape, o['p0'], kind)
    what = f'B {B} (Kg, Km, layers) {shape} {kind}'
    for s in range(steps):
        uid, iid, y = o['batches'][s]
        got = e.step(s, uid, iid, y, want_loss=True)
        _gate(f'{what} step {s} loss', got, *o['loss'][s])
        if s in check_at:
            _gate(f'{what} logits after {s + 1} step(s)', _all_logits(e), *o['logits'][s])
            _padding_is_zero(e)
        if s == 0:
            _check_idle_rows(e, kind, o['p0'], uid, iid, e._step_sizes(0, (3, 0, 1, 2)))
    return e, o


# every B, every (Kg, Km) and every layer list at least once; the extremes together
STEP_CASES = [(1, (1, 1, (1,))), (15, (5, 5, (5,))), (16, DEFAULT), (17, (5, 5, (17, 16))), (64, DEFAULT), (64, WIDEST), (257, WIDEST),
              (257, (1, 1, (1,))), (1, WIDEST), (257, (5, 5, (17, 16)))]


@pytest.mark.parametrize('B,shape', STEP_CASES)
def test_adam_steps_match_the_oracle_after_1_and_10_steps(B, shape):
    e, o = _run_against_the_oracle(B, shape)
    _, slots = _tables(e)
    for name in no.names(o['p']):                           # the slots too: Adam's m and v of every parameter
        for k in range(2):
            scale = max(1e-30, float(np.max(np.abs(o['state'][name][k]))))
            assert np.max(np.abs(slots[k][name] - o['state'][name][k])) <= 1e-4 * scale, (name, k)


@pytest.mark.parametrize('shape', [(5, 5, (17, 16)), DEFAULT])
def test_a_workgroup_that_walks_several_tiles_matches_the_oracle(shape):
    """B = 4113: 258 tiles for drx_ncf_grid's 256 workgroups — two of them add a second tile into their partial gradients"""
    from drecpy_amd._lib import lib
    B = 4113
    assert lib().drx_ncf_grid(B) == 256 < (B + 15) // 16 and lib().drx_ncf_grid(4096) == 256 and lib().drx_ncf_grid(17) == 2
    _run_against_the_oracle(B, shape, steps=2, check_at=(0, 1))


@pytest.mark.parametrize('shape', [(5, 5, (17, 16)), DEFAULT])
@pytest.mark.parametrize('kind', ['adam', 'adagrad', 'sgd', 'momentum', 'nesterov', 'rmsprop'])
def test_one_step_under_every_rule(kind, shape):
    e, _ = _run_against_the_oracle(64, shape, kind, steps=1, check_at=(0,))
    n = 2 if kind == 'adam' else bo.oo.N_SLOTS[kind]
    for name in ('U', 'V', 'sw'):
        assert [s is not None for s in e.state[name]] == [k < n for k in range(2)]


@pytest.mark.parametrize('shape', [(1, 1, (1,)), (5, 5, (17, 16)), (7, 30, (33, 9))])
def test_padding_stays_zero_over_ten_steps(shape):
    e = _engine(shape, _params(shape, seed=3))
    for s in range(10):
        e.step(s, *_batch(64, 40 + s))
    _padding_is_zero(e)
    assert e.U[:, e.ldg:e.ldg + e.Km].cpu().numpy().any() and e.V[:, :e.Kg].cpu().numpy().any()
    f1 = shape[2][0]
    for side in (0, 1):
        h = e.half_rows(side).cpu().numpy()
        assert h.shape[1] == e.hw == (f1 + 3) // 4 * 4 + e.ldg
        assert h[:, :f1].any() and not h[:, f1:e.hw - e.ldg].any() and not h[:, e.hw - e.ldg + e.Kg:].any()


def test_the_same_inputs_give_the_same_bits():
    shape, B = (6, 20, (24, 12)), 257
    p = _params(shape, seed=1)
    runs = []
    for _ in range(2):
        e = _engine(shape, p)
        losses = [e.step(s, *_batch(B, 5 + s), want_loss=True) for s in range(3)]
        runs.append([t.cpu().numpy().copy() for t in e.tensors().values()] + [x.cpu().numpy().copy() for n in e.state for x in e.state[n]]
                    + [np.array(losses), _all_logits(e)])
    assert all(np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)) for a, b in zip(*runs))
    assert not np.array_equal(runs[0][0][:, :6], p['Pg'].astype(F))


# ---- serving ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _serving_case(shape, n_items):
    """(parameters, oracle logits, replay logits, oracle half rows, replay half rows), computed once"""
    p = _params(shape, seed=SERVE_SEEDS.get((shape, n_items), 0), n_items=n_items)
    no.reset_seen()
    x = no.logits(p)
    assert no.seen['min_abs_z'] >= MIN_Z
    p32 = no.replay32(p)
    return p, x, no.logits_split(p32), no.half_rows(p), no.half_rows(p32)


@pytest.mark.parametrize('shape', [(1, 1, (1,)), (5, 5, (17, 16)), DEFAULT, WIDEST])
@pytest.mark.parametrize('n_items', [1, 15, 16, 17, 41, 257])
def test_score_rows_and_half_rows_match_the_oracle(n_items, shape):
    p, x, x32, halves, halves32 = _serving_case(shape, n_items)
    e = _engine(shape, p, n_items=n_items)
    f1 = shape[2][0]
    strip = lambda h: np.concatenate([h[:, :f1], h[:, e.hw - e.ldg:e.hw - e.ldg + e.Kg]], axis=1)
    for side in (0, 1):
        _gate(f'{shape} n_items {n_items} half rows of side {side}', strip(e.half_rows(side).cpu().numpy()), halves[side], halves32[side])
    some = _dev([3, 0, 3], np.int32)
    assert np.array_equal(_bits(e.half_rows(0, some).cpu().numpy()), _bits(e.half_rows(0).cpu().numpy()[[3, 0, 3]]))
    full = e.score_matrix(np.arange(U, dtype=np.int32)).cpu().numpy()
    for R in (1, 5, 17):
        users = (np.arange(R) * 7 + 3) % U
        got = e.score_matrix(users.astype(np.int32)).cpu().numpy()
        assert got.shape == (R, n_items)
        _gate(f'{shape} n_items {n_items} R {R} logits', got, x[users], x32[users])
        assert np.array_equal(_bits(got), _bits(full[users])), 'a logit depends on the block its user sits in'


@pytest.mark.parametrize('shape', [(1, 1, (1,)), (5, 5, (17, 16)), (7, 30, (33, 9)), DEFAULT, WIDEST])
def test_half_rows_are_bit_equal_to_the_k_ordered_fmaf_replay(shape):
    """the fp32 matrix core's sum is a k-ordered fmaf chain from zero: the half rows are that chain, then one fp32 addition of b_1 (users),
    and hg[k] * Pg[u, k] as one fp32 product; ids NULL and ids given; 23 and 41 rows are one full tile of 16 and a partial one"""
    p = _params(shape, seed=2)
    e = _engine(shape, p)
    Kg, Km, layers = shape
    f1 = layers[0]
    q = {k: v.astype(F) for k, v in p.items()}
    fma = lambda a, b, c: (a.astype(D) * b.astype(D) + c.astype(D)).astype(F)      # (exact product, one rounding of the sum)

    def chain(rows, W):
        acc = np.zeros((len(rows), f1), F)
        for k in range(Km):
            acc = fma(rows[:, k:k + 1], W[k:k + 1, :], acc)
        return acc
    want = [np.concatenate([chain(q['Pm'], q['W1'][:Km]) + q['b1'], q['hg'] * q['Pg']], axis=1),
            np.concatenate([chain(q['Qm'], q['W1'][Km:]), q['Qg']], axis=1)]
    for side in (0, 1):
        h = e.half_rows(side).cpu().numpy()
        got = np.concatenate([h[:, :f1], h[:, e.hw - e.ldg:e.hw - e.ldg + Kg]], axis=1)
        assert np.array_equal(_bits(got), _bits(want[side])), f'side {side}: {int((_bits(got) != _bits(want[side])).sum())} elements differ'
        ids = np.array([3, 0, 3, 22, 7] * 4, np.int32)
        assert np.array_equal(_bits(e.half_rows(side, _dev(ids, np.int32)).cpu().numpy()), _bits(h[ids]))


@pytest.mark.parametrize('shape', [(1, 1, (1,)), (5, 5, (17, 16)), DEFAULT, WIDEST])
def test_pair_scores_are_the_bits_of_the_matrix_cells(shape):
    """repeated pairs, one user's pairs across the border of a 16-pair tile and of a 64-pair workgroup, an item outside the catalogue"""
    p, x, x32, _, _ = _serving_case(shape, N)
    e = _engine(shape, p)
    full = _all_logits(e)
    rng = np.random.default_rng(4)
    users, items = rng.integers(0, U, size=150), rng.integers(0, N, size=150)
    users[10:22], items[10:22] = 5, np.arange(12)                          # user 5 straddles the tile border at 16
    users[60:70], items[60:70] = 9, np.arange(10) + 20                     # user 9 the workgroup border at 64
    users[100], items[100], users[101], items[101] = users[3], items[3], users[3], items[3]
    for P in (1, 16, 17, 150):
        got = e.pair_scores(users[:P].astype(np.int32), items[:P].astype(np.int32)).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(full[users[:P], items[:P]])), P
    _gate(f'{shape} pair logits', got, x[users, items], x32[users, items])
    out = e.pair_scores(np.array([1, 2, 3], np.int32), np.array([4, N, -1], np.int32)).cpu().numpy()
    assert out[0] == full[1, 4] and np.isneginf(out[1]) and np.isneginf(out[2])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _broken_dims(e):
    """{what: a copy of the engine's dims with one field outside the domain or off the layout}"""
    from drecpy_amd._lib import NcfDims

    def copy(**kw):
        d = NcfDims.from_buffer_copy(e.dims)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return d
    return {'kg 0': copy(kg=0), 'kg 65': copy(kg=65), 'km 0': copy(km=0), 'km 65': copy(km=65), 'ldg off': copy(ldg=e.ldg + 4),
            'ldm off': copy(ldm=e.ldm + 4), 'no layer': copy(n_layers=0), '5 layers': copy(n_layers=5), 'f 0': copy(f=(0, 0)),
            'f 65': copy(f=(1, 65)), 'off_w off': copy(off_w=(1, e.dims.off_w[1] + 1)), 'off_b off': copy(off_b=(0, e.dims.off_b[0] - 1)),
            'off_h off': copy(off_h=e.dims.off_h + 1), 'off_b0 off': copy(off_b0=e.dims.off_b0 - 1), 'n_small off': copy(n_small=e.n_small + 1),
            'n_users 0': copy(n_users=0), 'n_items 0': copy(n_items=0)}


def test_step_refusals_leave_the_parameters_alone():
    import torch
    from drecpy_amd import _lib
    from drecpy_amd._lib import lib, ptr
    shape, B = (6, 10, (12, 8)), 16
    e = _engine(shape, _params(shape, seed=2))
    uid, iid, y = _batch(B, 3)
    uid, iid, y = _dev(uid, np.int32), _dev(iid, np.int32), _dev(y, F)
    dims = C.byref(e.dims)
    need = int(lib().drx_ncf_step_scratch_bytes(dims, B))
    assert need > 0
    for b in (0, -1, 1 << 24):
        assert lib().drx_ncf_step_scratch_bytes(dims, b) == 0, b
    broken = _broken_dims(e)
    for what, d in broken.items():
        assert lib().drx_ncf_step_scratch_bytes(C.byref(d), B) == 0, what
    sc = torch.zeros(need, dtype=torch.uint8, device='cuda:0')
    alphas = (C.c_float * 3)(1e-2, 1e-2, 1e-2)
    slots = [ptr(s) for n in ('U', 'V', 'sw') for s in e.state[n]]             # U m, U v, V m, V v, sw m, sw v
    adam, momentum = _lib.OptRule(0, 0.0, 0.9, 0.999, 1e-7), _lib.OptRule(4, 0.0, 0.9, 0.0, 0.0)
    rowwise, unknown = _lib.OptRule(2, 0.0, 0.0, 0.0, 1e-7), _lib.OptRule(99, 0.0, 0.0, 0.0, 0.0)
    good = [dims, ptr(e.U), ptr(e.V), ptr(e.sw)] + slots + [ptr(uid), ptr(iid), ptr(y), B, C.byref(adam), alphas, 1e-3, None, ptr(sc), need, None]
    params = list(e.tensors().values())
    start = [t.cpu().numpy().copy() for t in params]
    bad = {'D': (0, None), 'U': (1, None), 'V': (2, None), 'sw': (3, None), 'uid': (10, None), 'iid': (11, None), 'y': (12, None),
           'rule': (14, None), 'alphas': (15, None), 'scratch': (18, None), 'B 0': (13, 0), 'B -3': (13, -3),
           'adam without U m': (4, None), 'adam without V v': (7, None), 'adam without sw m': (8, None), 'momentum without V s1': (6, None),
           'row-wise adagrad': (14, C.byref(rowwise)), 'an unknown rule': (14, C.byref(unknown)),
           'a misaligned U': (1, C.c_void_p(e.U.data_ptr() + 4)), 'a misaligned V': (2, C.c_void_p(e.V.data_ptr() + 8))}
    bad.update({what: (0, C.byref(d)) for what, d in broken.items()})
    for what, (at, value) in bad.items():
        args = list(good)
        args[at] = value
        if what.startswith('momentum'):
            args[14] = C.byref(momentum)
        assert lib().drx_ncf_step(*args) == EINVAL, what
    small = list(good)
    small[19] = need // 2
    assert lib().drx_ncf_step(*small) == ESCRATCH
    torch.cuda.synchronize()
    for t, b in zip(params, start):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(b))
    assert not sc.cpu().numpy().any(), 'a refused call wrote its scratch'
    assert lib().drx_ncf_step(*good) == 0
    torch.cuda.synchronize()
    assert all(not np.array_equal(_bits(t.cpu().numpy()), _bits(b)) for t, b in zip(params, start))


def test_serving_refusals_leave_the_outputs_alone():
    import torch
    from drecpy_amd._lib import lib, ptr
    shape = (6, 10, (12, 8))
    e = _engine(shape, _params(shape, seed=2))
    dims, L = C.byref(e.dims), lib()
    broken = _broken_dims(e)
    ids = _dev(np.arange(4), np.int32)
    out = torch.full((U * N + 8,), -7.0, dtype=torch.float32, device='cuda:0')
    uh, ih = e.half_rows(0), e.half_rows(1)
    rows = _dev(np.arange(4), np.int32)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)
    calls = {
        'drx_ncf_half_rows': ([dims, ptr(e.U), ptr(e.sw), ptr(ids), 4, 0, ptr(out), None],
                              {'D': (0, None), 'table': (1, None), 'sw': (2, None), 'out': (6, None), 'n 0': (4, 0), 'side 2': (5, 2),
                               'side -1': (5, -1), 'a misaligned table': (1, off(e.U, 4)), 'a misaligned out': (6, off(out, 4))}),
        'drx_ncf_score_rows': ([dims, ptr(e.sw), ptr(uh), ptr(ih), 5, ptr(out), None],
                               {'D': (0, None), 'sw': (1, None), 'uhalf': (2, None), 'ihalf': (3, None), 'out': (5, None), 'R 0': (4, 0),
                                'a misaligned uhalf': (2, off(uh, 4)), 'a misaligned ihalf': (3, off(ih, 8))}),
        'drx_ncf_pair_scores': ([dims, ptr(e.sw), ptr(uh), ptr(ih), ptr(rows), ptr(rows), 4, ptr(out), None],
                                {'D': (0, None), 'sw': (1, None), 'uhalf': (2, None), 'ihalf': (3, None), 'urow': (4, None), 'irow': (5, None),
                                 'out': (7, None), 'P 0': (6, 0), 'a misaligned ihalf': (3, off(ih, 4))})}
    for name, (good, bad) in calls.items():
        bad = dict(bad, **{what: (0, C.byref(d)) for what, d in broken.items()})
        for what, (at, value) in bad.items():
            args = list(good)
            args[at] = value
            assert getattr(L, name)(*args) == EINVAL, (name, what)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()
    for name, (good, _) in calls.items():
        assert getattr(L, name)(*good) == 0, name
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[:4] != -7.0).all()


def test_engine_refuses_by_name():
    from drecpy_amd._lib import DrxError
    from drecpy_amd.engine_ncf import NcfEngine
    for K in (0, 65, 2.5):
        with pytest.raises(DrxError, match=r'\bfactors must'):
            NcfEngine(U, N, K, 4, (4,))
        with pytest.raises(DrxError, match='mlp_factors must'):
            NcfEngine(U, N, 4, K, (4,))
    for layers in ((), (4,) * 5, (0,), (65,), (4, 2.5), 8):
        with pytest.raises(DrxError, match='layers must'):
            NcfEngine(U, N, 4, 4, layers)
    e = _engine((4, 4, (4,)), _params((4, 4, (4,))))
    for call in ('recommend', 'rank_items', 'rank_lists'):
        with pytest.raises(DrxError, match='not a dot product'):
            getattr(e, call)(np.arange(3), 5)
    with pytest.raises(DrxError, match='lacks'):
        e.set_params({'Pg': np.zeros((U, 4))})


# ---- the public class ------------------------------------------------------------------------------------------------------------------
RF = 3                                                      # the fitted model's neg_ratio
SHAPE = (5, 6, (12, 7))
FIT = dict(epochs=20, batch_size=64, learning_rate=1e-2, neg_ratio=RF, reg_rate=1e-3)


@functools.lru_cache(maxsize=None)
def _records():
    """(user, item, interaction) rows of a 23 x 41 frame, users and items in first-appearance order (internal id == raw id).  User 0
    records all but three items, 1 one positive, 2 one pair below the threshold (no positive), the others 4 - 14 pairs on both sides
    of the threshold."""
    rng = np.random.default_rng(2025)
    rows = [(0, i, 2.0) for i in range(N - 3)] + [(1, N - 3, 1.0), (2, N - 2, 0.5), (3, N - 1, 2.0), (3, 5, 1.0), (3, 9, 3.0)]
    for u in range(4, U):
        items = rng.choice(N, size=int(rng.integers(4, 15)), replace=False)
        rows += [(u, int(i), float(rng.choice([0.5, 1.0, 2.0, 3.0], p=[0.2, 0.3, 0.3, 0.2]))) for i in items]
    return rows


def _dataset():
    from drecpy_amd.Dataset import InteractionDataset
    u, i, v = (np.array(c) for c in zip(*_records()))
    return InteractionDataset.from_arrays(u.astype(np.int64), i.astype(np.int64), v.astype(np.float64))


@functools.lru_cache(maxsize=None)
def _frame():
    """the arguments of point_sample_counter for _records()"""
    f = bo.Frame(U, N, _records(), THR)
    return bo.Frame.csr(f.positives) + bo.Frame.csr(f.recorded) + (U, N)


def _model(**kw):
    from drecpy_amd.Recommender.Baseline import NeuMF
    Kg, Km, layers = SHAPE
    return NeuMF(factors=Kg, mlp_factors=Km, layers=layers, interaction_threshold=THR, verbose=False, **kw)


def _oracle_fit(w, model, epochs, B, r):
    out = []
    for q in (w, no.replay32(w)):
        p = {k: v.copy() for k, v in q.items()}
        no.fit(p, _frame(), epochs, B, r, model._draw_seed)
        out.append(p)
    return out


def _start_weights(seed):
    return no.init_params(np.random.default_rng(seed), U, N, *SHAPE)


@pytest.fixture(scope='module')
def fitted():
    """(model, oracle parameters, their float32 replay) after the same 20 steps on the same draws"""
    w = _start_weights(FIT_SEED)
    model = _model(seed=3)
    model.fit(_dataset(), initial_weights=w, **FIT)
    ds = model.interaction_dataset
    assert all(ds.user_to_uid(u) == u for u in range(U)) and all(ds.item_to_iid(i) == i for i in range(N))
    no.reset_seen()
    p, p32 = _oracle_fit(w, model, FIT['epochs'], FIT['batch_size'], RF)
    no.logits(p)
    assert no.seen['min_abs_z'] >= MIN_Z
    return model, p, p32


def test_the_batches_fed_to_the_step_are_the_oracle_stream(fitted):
    model, _, _ = fitted
    for n, seed in ((1, 0), (257, model._draw_seed(1)), (1000, 0xFEDCBA9876543210)):
        got = [t.cpu().numpy() for t in model._engine.sample(n, RF, seed)]
        want = point_sample_counter(*_frame(), n, RF, seed & bo.M64)
        assert not want[4].any()
        for g, w_, name in zip(got, want, ('uid', 'iid', 'y')):
            assert g.dtype == w_.dtype and np.array_equal(g, w_), f'{name} differs at n {n}'
        uid, iid, y = want[:3]
        recorded = set((u, i) for u, i, _ in _records())
        positive = set((u, i) for u, i, v in _records() if v >= THR)
        assert all(((u, i) in positive) if t == 1 else ((u, i) not in recorded) for u, i, t in zip(uid.tolist(), iid.tolist(), y.tolist()))


def test_fit_equals_the_oracle_fit_on_the_same_draws(fitted):
    model, p, p32 = fitted
    x = no.logits(p)
    _gate('logits after fit(epochs=20)', _all_logits(model._engine), x, no.logits(p32))
    _padding_is_zero(model._engine)
    for u in (1, 2, 5):                                     # one positive, no positive, an ordinary user
        assert model.predict(u, 7) == pytest.approx(1 / (1 + np.exp(-x[u, 7])), abs=1e-5)
    assert isinstance(model.predict(5, 7), float) and 0.0 < model.predict(5, 7) < 1.0
    saved = model._engine.get_params()
    assert sorted(saved) == sorted(p) and all(saved[k].shape == p[k].shape for k in p)


def test_recommend_batch_equals_recommend_and_the_oracle_order(fitted):
    model, p, _ = fitted
    x = no.logits(p)
    prob = 1 / (1 + np.exp(-x))
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
                assert np.max(np.abs(np.array([s for s, _ in got]) - np.array([prob[u, i] for _, i in got]))) <= G
                for (_, a), (_, b) in zip(got, got[1:]):       # the oracle's order wherever its logits differ by more than the gate
                    assert x[u, a] >= x[u, b] - 2 * G, (u, a, b)
                best = sorted(allowed, key=lambda i: -x[u, i])[:len(got)]
                if len(allowed) == len(got) or x[u, best[-1]] - max([x[u, i] for i in allowed if i not in best], default=-np.inf) > 2 * G:
                    assert sorted(best) == sorted(i for _, i in got), (u, n, novelty)
    assert len(model.recommend_batch([0], n=N, novelty=True)[0]) == 3              # user 0 records all but three items
    thr = float(np.median(prob[5]))                         # interaction_threshold compares the reported probabilities
    some = model.recommend_batch([5], n=N, novelty=False, interaction_threshold=thr)[0]
    assert 0 < len(some) < N and all(s >= thr for s, _ in some) and some == model.recommend(5, novelty=False, interaction_threshold=thr)


def test_catalogue_ranks_are_positions_in_the_full_list(fitted):
    model, _, _ = fitted
    requests = (([2, 5, 5, 17, 22, 22, 22, 1], [17, 0, 40, 30, 1, 2, 3, 4]), ([5] * 9 + [22] * 9, [(5 * k) % N for k in range(18)]),
                ([5, 5], [3, 999]))                                  # (999: an item the model does not know)
    for (users, items), novelty in ((r, nov) for r in requests for nov in (True, False)):
        ranks, scores = model.catalogue_ranks(users, items, novelty=novelty, return_scores=True)
        full = {u: model.recommend_batch([u], n=N, novelty=novelty)[0] for u in set(users)}
        for u, i, r, s in zip(users, items, ranks, scores):
            place = {item: (j, v) for j, (v, item) in enumerate(full[u])}
            if i in place:
                assert r == place[i][0] and s == place[i][1], (u, i, novelty)
            else:
                assert r == -1 and s == -np.inf, (u, i, novelty)


def test_predict_pairs_equals_predict(fitted):
    model, p, p32 = fitted
    rng = np.random.default_rng(8)
    users, items = rng.integers(0, U, size=200), rng.integers(0, N, size=200)
    got = model.predict_pairs(users.tolist(), items.tolist())
    assert got.dtype == np.float64
    assert np.array_equal(got, np.array([model.predict(int(u), int(i)) for u, i in zip(users, items)]))
    sig = lambda a: 1 / (1 + np.exp(-np.asarray(a, D)))
    _gate('predict_pairs', got, sig(no.logits(p)[users, items]), sig(no.logits(p32)[users, items]))
    assert np.isnan(model.predict_pairs([1, 999], [1, 1], skip_errors=True)[1])


def test_reported_values_are_sigmoids_and_the_order_is_the_logits(fitted, tmp_path):
    """user 6 gets weights under which five logits exceed 35: their reported values are all exactly 1.0 (float64's sigmoid is
    saturated) while the lists still follow the logits"""
    from drecpy_amd.Recommender.Baseline import NeuMF
    model, p, _ = fitted
    path = str(tmp_path / 'ncf_saturated.pkl')
    model.save(path)
    other = NeuMF.load(path)
    q = {k: v.copy() for k, v in p.items()}
    q['hg'][0] = 1.0
    q['Pg'][:, 0], q['Qg'][:, 0] = 0.0, 0.0
    hot = [4, 30, 12, 40, 21]                                # ascending logit in this order
    q['Pg'][6, 0] = 50.0
    q['Qg'][hot, 0] = 1.0 + 0.1 * np.arange(5)
    q = {k: v.astype(F).astype(D) for k, v in q.items()}
    other._engine.set_params(q)
    x = no.logits(q)
    assert (x[6, hot] > 35).all() and (np.delete(x[6], hot) < 20).all() and (np.diff(x[6, hot]) > 1).all()
    logit = other._engine.score_matrix(np.array([6], np.int32)).cpu().numpy()[0]
    assert np.max(np.abs(logit - x[6])) <= 1e-5 * np.abs(x).max()
    for got in (other.recommend(6, n=8, novelty=False), other.recommend_batch([6], n=8, novelty=False)[0],
                other.rank(6, list(range(N)), novelty=False, n=8)):
        assert [i for _, i in got[:5]] == hot[::-1]
        assert all(s == 1.0 for s, _ in got[:5]) and all(0.0 < s < 1.0 for s, _ in got[5:])
        assert [i for _, i in got] == [int(i) for i in sorted(range(N), key=lambda i: (-logit[i], -i))[:8]]
    ranks, scores = other.catalogue_ranks([6] * 5, hot, novelty=False, return_scores=True)
    assert ranks.tolist() == [4, 3, 2, 1, 0] and (scores == 1.0).all()
    assert other.predict(6, 40) == 1.0 and np.array_equal(other.predict_pairs([6, 6], [4, 21]), [1.0, 1.0])


def test_rank_and_evaluations_batched_and_not(fitted):
    from drecpy_amd.Evaluation import predictive_evaluation, ranking_evaluation, recommendation_evaluation
    model, p, _ = fitted
    x = no.logits(p)
    cands = [3, 8, 11, 20, 33, 40]
    got = model.rank(5, cands, novelty=False)
    assert sorted(i for _, i in got) == cands
    for (sa, a), (sb, b) in zip(got, got[1:]):
        assert x[5, a] >= x[5, b] - 2e-5 and sa >= sb
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
    from drecpy_amd.Recommender.Baseline import NeuMF
    model, _, _ = fitted
    path = str(tmp_path / 'ncf.pkl')
    model.save(path)
    other = NeuMF.load(path)
    assert isinstance(other, NeuMF)
    users, items = list(range(U)) * 2, [(7 * k) % N for k in range(2 * U)]
    assert np.array_equal(other.predict_pairs(users, items), model.predict_pairs(users, items))
    assert other.recommend_batch([5, 22, 1, 2], n=7) == model.recommend_batch([5, 22, 1, 2], n=7)
    assert other.recommend(5, n=7) == model.recommend(5, n=7)


def test_callbacks_early_stopping_and_loss():
    from drecpy_amd.Recommender.early_stopping import MaxValidationValueRule
    w = _start_weights(9)
    seen = []
    model = _model(seed=1)
    model.fit(_dataset(), epochs=6, batch_size=32, learning_rate=1e-2, neg_ratio=2, reg_rate=1e-3, initial_weights=w,
              epoch_callback_fn=lambda m: seen.append(float(m.predict(5, 7))) or {'score': -len(seen)}, epoch_callback_freq=2,
              early_stopping_rule=MaxValidationValueRule('score'), early_stopping_freq=2)
    assert len(seen) >= 1 and model.fitted
    # the best epoch is the first one evaluated (the score falls): the weights are those of epoch 2
    p, p32 = _oracle_fit(w, model, 2, 32, 2)
    _gate('logits after the revert to epoch 2', _all_logits(model._engine), no.logits(p), no.logits(p32))


def test_default_initialisation_is_the_seeds_and_trains():
    """without initial_weights: N(0, init_std) tables, Glorot-uniform kernels, h uniform in +-sqrt(3 / (Kg + f_n)), zero biases, from
    default_rng(seed); one step from them is the oracle's"""
    from drecpy_amd.Recommender.Baseline import NeuMF
    model = NeuMF(seed=11, interaction_threshold=THR, verbose=False)
    model.fit(_dataset(), epochs=1, batch_size=64, neg_ratio=RF)
    w = model._init_weights(8, 32, (32, 16, 8))
    assert abs(np.std(w['Pm']) - 0.01) < 2e-3 and not w['b1'].any() and not w['b0'].any()
    assert np.abs(w['W1']).max() <= np.sqrt(6 / 96) and np.abs(w['W1']).max() > 0.9 * np.sqrt(6 / 96)
    assert np.abs(np.concatenate([w['hg'], w['hm']])).max() <= np.sqrt(3 / 16)
    again = NeuMF(seed=11, interaction_threshold=THR, verbose=False)
    again.fit(_dataset(), epochs=1, batch_size=64, neg_ratio=RF)
    a, b = model._engine.get_params(), again._engine.get_params()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    w64 = {k: np.asarray(v, F).astype(D) for k, v in w.items()}
    uid, iid, y, _, _ = point_sample_counter(*_frame(), 64, RF, model._draw_seed(1) & bo.M64)
    st = no.init_state(w64, 'adam')
    no.step(w64, st, 0, uid, iid, y, hp=dict(no.HP, lr=1e-3, reg=1e-3))
    assert np.max(np.abs(_all_logits(model._engine) - no.logits(w64))) <= 1e-5


@pytest.mark.parametrize('what', ['neg_ratio 0', 'factors 0', 'factors 65', 'mlp_factors 0', 'mlp_factors 65', 'layers ()', 'layers 5', 'layers 65',
                                  'no positive', 'no unrecorded item', 'optimizer'])
def test_fit_refuses_by_name(what):
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender.Baseline import NeuMF
    ds = _dataset()
    kw = dict(epochs=1, batch_size=8)
    mk = lambda **k: NeuMF(interaction_threshold=THR, verbose=False, **k)
    if what == 'neg_ratio 0':
        with pytest.raises(Exception, match='neg_ratio'):
            mk().fit(ds, neg_ratio=0, **kw)
    elif what.startswith('factors'):
        with pytest.raises(Exception, match=r'NeuMF: factors must'):
            mk(factors=int(what.split()[1])).fit(ds, **kw)
    elif what.startswith('mlp_factors'):
        with pytest.raises(Exception, match='mlp_factors must'):
            mk(mlp_factors=int(what.split()[1])).fit(ds, **kw)
    elif what.startswith('layers'):
        layers = {'()': (), '5': (4,) * 5, '65': (65,)}[what.split()[1]]
        with pytest.raises(Exception, match='layers must'):
            mk(layers=layers).fit(ds, **kw)
    elif what == 'optimizer':
        with pytest.raises(Exception, match='dense rules'):
            mk().fit(ds, optimizer='rowwise_adagrad', **kw)
    elif what == 'no positive':
        low = InteractionDataset.from_arrays(np.array([0, 0, 1]), np.array([0, 1, 2]), np.full(3, 0.5))
        with pytest.raises(Exception, match='no positive'):
            mk().fit(low, **kw)
    else:
        full = InteractionDataset.from_arrays(np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1]), np.full(4, 2.0))
        with pytest.raises(Exception, match='unrecorded item'):
            mk().fit(full, **kw)


def test_fit_refuses_a_process_group(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    with pytest.raises(Exception, match='process group'):
        _model().fit(_dataset(), epochs=1, batch_size=8)
