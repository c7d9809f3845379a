"""Mult-VAE on the device against tests/vae_oracle.py (NumPy float64), through the C ABI (drx_vae_step, drx_vae_noise,
drx_vae_query_rows) and drecpy_amd.engine_vae.VaeEngine.  (The public class: tests/test_gpu_vae_api.py.)

The gate on ALL scores (every user x every item) and on the loss is the project's, from tests/test_gpu_fpmc.py:

    err(GPU) <= max(1e-5, 4 err(replay)) * max(1, max |x|)

where the replay is the oracle itself on float32 arrays.  Every (GPU, replay) pair is printed (pytest -s); DESIGN.md section 3.13 has
the table.  The test weights are uniform(-0.5, 0.5) / sqrt(width), so the softmax is not flat.  The step runs with explicit eps and
keep arrays from the oracle's restatement of the generator.  Every data set holds a user whose positives are the whole catalogue, one
with a single item and (n_items > 1) an item nobody but the first holds; the batch of step 0 leaves the first user out, so that item's
row of W_in is idle there and is compared bit for bit with an fp32 replay of its reg-only update, as are W_out and b_out at
n_items = 1, where dlogit is exactly zero."""
import ctypes as C

import numpy as np
import pytest

import bpr_oracle as bo
import vae_oracle as vo
from test_gpu_bpr import _bits, _idle_replay
from test_gpu_fpmc import _gate
from test_gpu_gru import KINDS, _optimizer

pytestmark = pytest.mark.gpu

F = np.float32
EINVAL, ESCRATCH = -1, -2
DROPOUT, BETA = 0.5, 0.2
SHAPES = [(1, 1, 1, 1), (17, 7, 3, 17), (67, 33, 17, 16), (300, 128, 64, 33), (1100, 64, 32, 257)]     # n_items, hidden, latent, B


def _data(N, B, seed=0):
    """rows of B + 2 users: user 0 holds the whole catalogue, user 1 one item, item N - 1 is held by user 0 alone, item 5 % N by every
    user from 2 on (at B = 257: more lookups than the split threshold of the CSR update, 64)"""
    rng = np.random.default_rng(1000 + N + seed)
    rows = [np.arange(N), np.array([min(3, N - 1)])]
    for u in range(2, B + 2):
        held = np.flatnonzero(rng.random(max(N - 1, 1)) < 0.3)
        rows.append(np.unique(np.concatenate([held, [5 % N, u % max(N - 1, 1)]])) if N > 1 else np.array([0]))
    return [r.astype(np.int64) for r in rows]


def _csr(rows):
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows).astype(np.int32)


def _engine(rows, N, H, L, p, kind='adam', variational=True, dropout=DROPOUT, beta=BETA, anneal=0):
    from drecpy_amd.engine_vae import VaeEngine
    e = VaeEngine(len(rows), N, H, L, variational)
    e.set_params(p)
    e.set_optimizer(_optimizer(kind, vo.HP['lr']))
    e.reg = vo.HP['reg']
    e.set_positives(_csr(rows))
    e.dropout, e.beta, e.anneal_steps = dropout, beta, anneal
    return e


def _batch(rows, B, s, dropout, L, variational):
    """(uid [B], keep flat or None, eps or None): step 0 leaves user 0 out; row 2 of a batch has every lookup dropped"""
    U = len(rows)
    uid = np.arange(1, B + 1) if s == 0 else np.random.default_rng(50 + s).permutation(U)[:B]
    if s > 0 and 0 not in uid:
        uid[0] = 0
    lens = [len(rows[u]) for u in uid]
    keep = None
    if dropout > 0:
        keep = vo.keep_bits(77 + s, lens, dropout)
        if B > 2:
            start = int(np.sum(lens[:2]))
            keep[start:start + lens[2]] = False
    eps = vo.noise_of(vo.noise_words(77 + s, B, L), F) if variational else None
    return uid.astype(np.int32), keep, eps


def _all_scores(e):
    return e.score_matrix(np.arange(e.n_users, dtype=np.int32)).cpu().numpy()


def _padding_is_zero(e):
    assert e.sw.numel() == e.H * e.E + e.latent * e.H + 2 * e.H + e.E
    slots = [] if e.opt_kind == 'adagrad' else [(n, s) for n in ('W_in', 'W_out') for s in e.state[n] if s is not None]
    for name, t in [('W_in', e.W_in), ('W_out', e.W_out)] + slots:
        assert not t.cpu().numpy()[:, e.H:].any(), f'a padding column of {name} moved'


def _check_idle(e, kind, p0, names_idle, alphas):
    reg = vo.HP['reg']
    l2 = {'W_in': reg, 'W_out': reg, 'b_out': 0.0}
    alpha = {'W_in': alphas[0], 'W_out': alphas[2], 'b_out': alphas[2]}
    for name, idle in names_idle:
        start = p0[name].astype(F)[idle]
        forms = _idle_replay(kind, start, l2[name], alpha[name])
        got = [getattr(e, name)] + list(e.state[name])
        for k, what in enumerate(('p', 's1', 's2')):
            if forms[0][k] is None:
                continue
            g = got[k].cpu().numpy()
            g = (g if name == 'b_out' else g[:, :e.H])[idle]
            same = np.logical_or.reduce([_bits(g) == _bits(f[k]) for f in forms])
            assert same.all(), f'{kind} {name} {what}: {int((~same).sum())} idle elements differ from the fp32 replay'


def _run(N, H, L, B, kind='adam', steps=10, check_at=(0, 9), variational=True, dropout=DROPOUT, anneal=0, scale_out=None, idle=True):
    rows = _data(N, B)
    p = vo.init_params(np.random.default_rng(100 + H + L), N, H, L, variational)
    if scale_out is not None:
        top = np.max(np.abs(vo.scores(p, rows)))
        for name in ('W_out', 'b_out'):
            p[name] = (p[name] * (scale_out / top)).astype(F).astype(np.float64)
    p0 = {k: v.copy() for k, v in p.items()}
    p32 = vo.replay32(p)
    st, st32 = vo.init_state(p, kind), vo.init_state(p32, kind)
    e = _engine(rows, N, H, L, p, kind, variational, dropout, BETA, anneal)
    what = f'N {N} H {H} L {L} B {B} {kind}{"" if variational else " dae"}{f" anneal {anneal}" if anneal else ""}'
    for s in range(steps):
        uid, keep, eps = _batch(rows, B, s, dropout, L, variational)
        brows = [rows[u] for u in uid]
        ks = None if keep is None else vo.split(keep, [len(r) for r in brows])
        klw = vo.beta_t(BETA, anneal, s)
        want, _ = vo.step(p, st, s, brows, ks, eps, dropout, klw, kind)
        rep, _ = vo.step(p32, st32, s, brows, ks, eps, dropout, klw, kind)
        got = e.step(s, uid, want_loss=True, eps=eps, keep=keep)
        assert np.isfinite(got)
        _gate(f'{what} step {s} loss', got, want, rep)
        if s in check_at:
            _gate(f'{what} scores after {s + 1} step(s)', _all_scores(e), vo.scores(p, rows), vo.scores(p32, rows))
            _padding_is_zero(e)
        if s == 0 and idle:
            alphas = e._step_sizes(0, (3, 0, 1, 2))
            if N > 1:
                held = np.unique(np.concatenate(brows))
                idle_in = np.setdiff1d(np.arange(N), held)
                assert N - 1 in idle_in
                _check_idle(e, kind, p0, [('W_in', idle_in)], alphas)
            else:
                _check_idle(e, kind, p0, [('W_out', np.arange(1)), ('b_out', np.arange(1))], alphas)
    return e, p, st


# softmax over one item | partial row and item tiles, widths no multiple of 4 | column-tile borders | every limit, several item tiles
# per workgroup (19 tiles on 19 workgroups; 1100 items: 69 tiles) | more row tiles than a round of waves, an item in 257 rows
@pytest.mark.parametrize('N,H,L,B', SHAPES)
def test_adam_steps_match_the_oracle_after_1_and_10_steps(N, H, L, B):
    e, p, st = _run(N, H, L, B)
    views = {'W_in': lambda a: a[:, :e.H], 'W_out': lambda a: a[:, :e.H], 'b_out': lambda a: a}
    for name in ('W_in', 'W_out', 'b_out'):                 # the slots too
        for k in range(2):
            scale = max(1e-30, float(np.max(np.abs(st[name][k]))))
            got = views[name](e.state[name][k].cpu().numpy())
            assert np.max(np.abs(got - st[name][k])) <= 1e-4 * scale, (name, k)


def test_more_item_tiles_than_persistent_workgroups():
    """129 item tiles on 128 workgroups: workgroup 0 walks two tiles, its slab and its (max, sum) partials take the second form"""
    _run(16 * 128 + 1, 8, 4, 5, steps=2, check_at=(0, 1))


@pytest.mark.parametrize('N,H,L,B', [(17, 7, 3, 17), (300, 128, 64, 33)])
@pytest.mark.parametrize('kind', [k for k in KINDS if k != 'adam'])
def test_one_step_under_every_other_rule(kind, N, H, L, B):
    e, _, _ = _run(N, H, L, B, kind, steps=1, check_at=(0,))
    n = bo.oo.N_SLOTS[kind]
    for name in ('W_in', 'sw', 'W_out', 'b_out'):
        assert [s is not None for s in e.state[name]] == [k < n for k in range(2)]


@pytest.mark.parametrize('N,H,L,B', [(17, 7, 3, 17), (67, 33, 17, 16)])
def test_the_denoising_autoencoder(N, H, L, B):
    _run(N, H, L, B, variational=False, steps=2, check_at=(0, 1))


def test_annealing_across_the_knee():
    _run(67, 33, 17, 16, anneal=4, steps=6, check_at=(0, 5))


def test_logits_of_80_stay_finite_and_inside_the_gate():
    """W_out and b_out scaled until the largest |logit| of serving is 80 (training's z moves it further): exp(80) = 5.5e34 is near the
    top of fp32 and a row's sum of 67 such terms, or exp of a logit of 89, is past it — a softmax without the max subtraction gives
    inf / inf here"""
    e, p, _ = _run(67, 33, 17, 16, steps=2, check_at=(0, 1), scale_out=80.0, idle=False)
    assert np.isfinite(_all_scores(e)).all()


@pytest.mark.parametrize('H', [1, 7])
def test_padding_stays_zero_over_ten_steps(H):
    rows = _data(17, 9)
    p = vo.init_params(np.random.default_rng(3), 17, H, 3)
    e = _engine(rows, 17, H, 3, p)
    for s in range(10):
        uid, keep, eps = _batch(rows, 9, s, DROPOUT, 3, True)
        e.step(s, uid, eps=eps, keep=keep)
    _padding_is_zero(e)


def test_two_runs_give_equal_bits():
    N, H, L, B = 300, 33, 17, 33
    rows = _data(N, B)
    p = vo.init_params(np.random.default_rng(5), N, H, L)
    runs = []
    for _ in range(2):
        e = _engine(rows, N, H, L, p)
        for s in range(5):
            uid, keep, eps = _batch(rows, B, s, DROPOUT, L, True)
            e.step(s, uid, eps=eps, keep=keep)
        runs.append({n: [t.cpu().numpy()] + [x.cpu().numpy() for x in e.state[n]] for n, t in e.tensors().items()})
    for n in runs[0]:
        for a, b in zip(runs[0][n], runs[1][n]):
            assert (_bits(a) == _bits(b)).all(), n


@pytest.mark.parametrize('N,H,L,B', [(17, 7, 3, 17), (300, 128, 64, 33)])
def test_query_rows_have_the_bits_of_the_steps_h2(N, H, L, B):
    rows = _data(N, B)
    p = vo.init_params(np.random.default_rng(6), N, H, L, False)
    e = _engine(rows, N, H, L, p, variational=False, dropout=0.0)
    uid = np.random.default_rng(1).permutation(len(rows))[:B].astype(np.int32)
    q = e._query_rows(e._dev_i32(uid)).cpu().numpy()
    e.step(0, uid)
    h2 = e.step_hidden(B).cpu().numpy()
    assert (_bits(q) == _bits(h2)).all()
    want = vo.encode(p, [rows[u] for u in uid])['h2']
    assert np.max(np.abs(q[:, :H] - want)) <= 1e-5 and not q[:, H:].any()


@pytest.mark.parametrize('dropout', [0.0, 0.5])
def test_noise_matches_the_restatement(dropout):
    N, L, B = 300, 17, 33
    rows = _data(N, B)
    p = vo.init_params(np.random.default_rng(7), N, 8, L)
    e = _engine(rows, N, 8, L, p, dropout=dropout)
    uid = np.arange(B, dtype=np.int32)
    for seed in (0, 0xFEDCBA9876543210, 12345 * 1000003 + 7):
        eps, keep, words = e.noise(seed, uid, want_words=True)
        want_words = vo.noise_words(seed, B, L)
        assert (words == want_words.astype(np.int64)).all()
        assert (keep.cpu().numpy().astype(bool) == vo.keep_bits(seed, [len(rows[u]) for u in uid], dropout)).all()
        if dropout == 0.0:
            assert keep.cpu().numpy().all()
        e64, e32 = vo.noise_of(want_words, np.float64), vo.noise_of(want_words, np.float32)
        bound = max(1e-6, 4.0 * float(np.max(np.abs(e32 - e64))))
        err = float(np.max(np.abs(eps.cpu().numpy() - e64)))
        print(f'eps seed {seed}: GPU error {err:.3e}, float32 NumPy error {bound / 4:.3e}')
        assert err <= bound


def test_refusals_return_the_codes_and_touch_nothing():
    from drecpy_amd import _lib
    from drecpy_amd._lib import lib, ptr
    import torch
    N, H, L, B = 17, 7, 3, 5
    rows = _data(N, B)
    p = vo.init_params(np.random.default_rng(8), N, H, L)
    e = _engine(rows, N, H, L, p)
    uid, keep, eps = _batch(rows, B, 1, DROPOUT, L, True)
    e.step(0, uid, eps=eps, keep=keep)                      # (allocates the scratch)
    before = {n: t.clone() for n, t in e.tensors().items()}
    uid_d, boff, B_, T, max_len = e._frame(uid)
    alphas, slots, _ = e._step_args(1, (3, 0, 1, 2), False)

    def dims(**kw):
        d = _lib.VaeDims()
        C.pointer(d)[0] = e.dims
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(d, B=B_, T=T, nbytes=None):
        return lib().drx_vae_step(C.byref(d), ptr(e.W_in), ptr(e.sw), ptr(e.W_out), ptr(e.b_out), *slots, C.byref(e._H), ptr(uid_d),
                                  ptr(boff), B, T, max_len, None, None, 0.5, 0.2, C.byref(e._rule()), alphas, 1e-3, None,
                                  ptr(e._scratch), e._scratch.numel() if nbytes is None else nbytes, None)

    for bad in (dims(h=0), dims(h=129), dims(latent=65), dims(ldh=12), dims(n_small=e.dims.n_small + 1)):
        assert lib().drx_vae_step_scratch_bytes(C.byref(bad), B_, T, max_len) == 0
        assert call(bad) == EINVAL
    assert lib().drx_vae_step_scratch_bytes(C.byref(e.dims), 0, T, max_len) == 0
    assert call(e.dims, B=0) == EINVAL
    assert call(e.dims, T=0) == EINVAL
    assert call(e.dims, nbytes=1024) == ESCRATCH
    out = torch.zeros(4, e.ldh, device='cuda:0')
    assert lib().drx_vae_query_rows(ptr(e.W_in), ptr(e.sw), C.byref(dims(h=129)), C.byref(e._H), ptr(uid_d), 4, ptr(out), None) == EINVAL
    assert lib().drx_vae_noise(1, ptr(boff), B_, T, 65, 0.5, None, None, None, None) == EINVAL
    torch.cuda.synchronize()
    for n, t in e.tensors().items():
        assert torch.equal(t, before[n]), n
    with pytest.raises(_lib.DrxError, match='hidden'):
        from drecpy_amd.engine_vae import VaeEngine
        VaeEngine(3, 3, 129, 4)
    with pytest.raises(_lib.DrxError, match='latent'):
        VaeEngine(3, 3, 8, 65)
