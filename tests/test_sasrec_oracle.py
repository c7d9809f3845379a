"""tests/sasrec_oracle.py without a GPU: its forward pass, loss and hand-written backward pass against torch.autograd in float64 on
torch.nn.functional.layer_norm / softmax, causality and the masks, its step against tests/optim_oracle.py; and what
Baseline.SASRec shows before an engine exists — the refusals word for word, the draw seeds, the batch loss, initial_weights — and
that include/drx.h, the bindings and the public package agree on the SASRec entry points."""
import os
import re

import numpy as np
import pytest

import bpr_oracle as bo
import optim_oracle as oo
import sasrec_oracle as so
from test_baseline_bases import SERVING, X5, _NotDense, _model, _refusal
from test_gru_oracle import hand_made_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (7, 3, 2), (17, 16, 1)]              # (H, L, blocks)
N_ITEMS = 9


def _torch_params(p):
    import torch
    return {k: torch.tensor(v, requires_grad=True) for k, v in p.items()}


def _torch_forward(t, ids):
    """h [B, H] of left-aligned ids [B, L] (-1 = absent) from torch tensors t: one sequence at a time, on its m present positions
    L - m .. L - 1 alone, with torch's own layer_norm and softmax"""
    import torch
    import torch.nn.functional as F
    L, H = t['Pos'].shape
    blocks = so.n_blocks(t)
    rows = []
    for row in np.asarray(ids):
        items = [int(x) for x in row if x >= 0]
        m = len(items)
        if m == 0:
            rows.append(torch.zeros(H, dtype=torch.float64))
            continue
        x = t['E'][torch.as_tensor(items)] + t['Pos'][L - m:]
        causal = torch.tril(torch.ones(m, m, dtype=torch.bool))
        for b in range(blocks):
            a = F.layer_norm(x, (H,), t[f'ln1_g{b}'], t[f'ln1_b{b}'], 1e-5)
            s = (a @ t[f'Wq{b}']) @ (a @ t[f'Wk{b}']).T / np.sqrt(H)
            x = x + F.softmax(s.masked_fill(~causal, -np.inf), dim=1) @ (a @ t[f'Wv{b}'])
            f = F.layer_norm(x, (H,), t[f'ln2_g{b}'], t[f'ln2_b{b}'], 1e-5)
            x = x + F.relu(f @ t[f'W1{b}'] + t[f'b1{b}']) @ t[f'W2{b}'] + t[f'b2{b}']
        rows.append(F.layer_norm(x[m - 1], (H,), t['lnf_g'], t['lnf_b'], 1e-5))
    return torch.stack(rows)


def every_length_baskets(L, seed=0):
    """L + 1 left-aligned baskets: lengths 0, 1, .., L"""
    rng = np.random.default_rng(seed)
    out = np.full((L + 1, L), -1)
    for m in range(L + 1):
        out[m, :m] = rng.integers(0, N_ITEMS, size=m)
    return out


@pytest.mark.parametrize('H,L,blocks', SHAPES)
def test_forward_equals_torch_for_baskets_of_every_length(H, L, blocks):
    import torch
    p = so.init_params(np.random.default_rng(H + L), N_ITEMS, H, L, blocks)
    baskets = every_length_baskets(L)
    with torch.no_grad():
        want = _torch_forward(_torch_params(p), baskets).numpy()
    got = so.query_rows(p, baskets)
    assert got.shape == (L + 1, H) and np.max(np.abs(got - want)) <= 1e-12
    assert not got[0].any() and np.array_equal(so.scores(p, baskets)[0], p['b'])          # an empty basket: h = 0 exactly, the score b[i]
    assert H == 1 or np.abs(got[1:]).max() > 1e-3


def _batches(L):
    """the hand-made batch with a repeated item (item 2: an input, a target and a negative), and a window of one item repeated"""
    uid, before, after = hand_made_batch(L)
    one = (np.zeros(2), np.full((2, L), 6), np.array([[6, 2, 3], [1, 6, 0]]))
    return {'repeated item': (uid, before, after), 'one item repeated': one}


@pytest.mark.parametrize('which', ['repeated item', 'one item repeated'])
@pytest.mark.parametrize('H,L,blocks', SHAPES)
def test_loss_and_gradients_equal_autograd(H, L, blocks, which):
    import torch
    p = so.init_params(np.random.default_rng(10 + H), N_ITEMS, H, L, blocks)
    _, before, after = _batches(L)[which]
    want_loss, g, h = so.gradients(p, before, after)
    t = _torch_params(p)
    ht = _torch_forward(t, before)
    x = torch.einsum('wh,wjh->wj', ht, t['Q'][torch.as_tensor(after)]) + t['b'][torch.as_tensor(after)]
    loss = torch.nn.functional.softplus(-(x[:, :1] - x[:, 1:])).mean()
    loss.backward()
    assert np.max(np.abs(h - ht.detach().numpy())) <= 1e-12
    assert abs(want_loss - float(loss.detach())) <= 1e-14 and abs(want_loss - so.loss(p, before, after)) <= 1e-15
    assert list(g) == so.names(blocks) == list(p)
    for name in so.names(blocks):
        auto = np.zeros_like(p[name]) if t[name].grad is None else t[name].grad.numpy()
        scale = float(np.max(np.abs(auto)))
        # LN of one column is its offset whatever the input: at H = 1 nothing before the last LN has a gradient, nor has any gain.
        # Either side may leave the rounding of dy - mean(dy) times rstd = 1 / sqrt(1e-5) = 316 there: a few times 316 * 2.2e-16 per
        # LN, far below the forward pass's absolute bound 1e-12
        dead = H == 1 and name not in ('lnf_b', 'Q', 'b')
        if dead:
            assert scale <= 1e-12 and np.max(np.abs(g[name])) <= 1e-12, name
            continue
        assert scale > 1e-6, name
        assert np.max(np.abs(g[name] - auto)) <= 1e-10 * scale, name


def test_changing_an_item_changes_no_earlier_position():
    H, L = 7, 5
    p = so.init_params(np.random.default_rng(5), N_ITEMS, H, L, 2)
    ids = np.array([[1, 2, 3, 4, 5]])
    base = so.forward(p, ids)[1]
    for t in range(L):
        other = ids.copy()
        other[0, t] = 8
        tape = so.forward(p, other)[1]
        for name in ('x', 'a', 'q', 'k', 'v', 'x1', 'f', 'r'):              # the inputs and every intermediate of block 1 (the second)
            a, b = base['blocks'][1][name][0], tape['blocks'][1][name][0]
            assert np.array_equal(a[:t], b[:t]) and not np.array_equal(a[t], b[t]), (t, name)
        assert np.array_equal(base['x'][0, :t], tape['x'][0, :t]) and not np.array_equal(base['x'][0, t:], tape['x'][0, t:])


def test_a_masked_position_changes_nothing():
    """a basket of m items is the model on those m items at the positions L - m .. L - 1: what stands for an absent entry is never read"""
    H, L = 7, 4
    p = so.init_params(np.random.default_rng(6), N_ITEMS, H, L, 2)
    want = so.query_rows(p, np.array([[3, 8, -1, -1]]))
    q = {k: v.copy() for k, v in p.items()}
    q['Pos'][:2] += 1.0                                     # the positions the basket does not fill
    q['E'][0] += 1.0                                        # an item the basket does not hold (an absent id must not read row 0 either)
    assert np.array_equal(so.query_rows(q, np.array([[3, 8, -1, -1]])), want)
    assert np.array_equal(so.shift(np.array([[3, 8, -1, -1], [-1, -1, -1, -1], [1, 2, 3, 4]])),
                          np.array([[-1, -1, 3, 8], [-1, -1, -1, -1], [1, 2, 3, 4]]))
    # the gradient of a serving-shaped batch leaves the absent positions alone
    _, g, _ = so.gradients(p, np.array([[3, 8, -1, -1], [5, -1, -1, -1]]), np.array([[1, 2], [0, 4]]))
    assert not g['Pos'][:2].any() and g['Pos'][2:].any() and not g['E'][[0, 1, 2, 4, 6, 7]].any()


@pytest.mark.parametrize('kind', ['adam', 'adagrad', 'sgd', 'momentum', 'nesterov', 'rmsprop', 'rmsprop_momentum'])
def test_step_is_the_rule_of_the_optim_oracle_on_the_gradients(kind):
    H, L, blocks = 7, 3, 2
    p = so.init_params(np.random.default_rng(2), N_ITEMS, H, L, blocks)
    st = so.init_state(p, kind)
    uid, before, after = hand_made_batch(L)
    for s in range(2):
        start = {k: v.copy() for k, v in p.items()}
        slots = {k: [None if a is None else a.copy() for a in v] for k, v in st.items()}
        _, g, _ = so.gradients(p, before, after)
        alphas = so.step_sizes(p, s, kind)
        so.step(p, st, s, uid, before, after, kind)
        for name in so.names(blocks):
            reg = name in ('E', 'Q', 'Pos') or name[:2] in ('Wq', 'Wk', 'Wv', 'W1', 'W2')
            assert reg == so.regularised(name) and not (reg and (name.startswith('b') or name.startswith('ln')))
            l2c = so.HP['reg'] if reg else 0.0
            if kind == 'adam':
                assert alphas[name] == bo.adam_alpha(so.HP['lr'], 3 * s + {'E': 0, 'Q': 2, 'b': 2}.get(name, 1) + 1, so.HP['b1'], so.HP['b2'])
                want = bo.du.adam_flat(start[name], slots[name][0], slots[name][1], g[name], alphas[name], l2c, so.HP['b1'], so.HP['b2'],
                                       so.HP['eps'])
                want = (want.p, want.m, want.v)
            else:
                assert alphas[name] == so.HP['lr']
                r = oo.rule_flat(kind, start[name], slots[name][0], slots[name][1], g[name], so.HP['lr'], l2c, mu=so.HP['mu'],
                                 rho=so.HP['rho'], eps=so.HP['eps'])
                want = (r.p, r.s1, r.s2)
            for a, b in zip((p[name], st[name][0], st[name][1]), want):
                assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), (kind, name)
            assert (p[name] != start[name]).any(), name


def test_replay32_runs_the_same_step_in_float32():
    H, L, blocks = 7, 3, 2
    p = so.init_params(np.random.default_rng(3), N_ITEMS, H, L, blocks)
    p32 = so.replay32(p)
    st, st32 = so.init_state(p, 'adam'), so.init_state(p32, 'adam')
    uid, before, after = hand_made_batch(L)
    for s in range(3):
        a, b = so.step(p, st, s, uid, before, after), so.step(p32, st32, s, uid, before, after)
        assert a == pytest.approx(b, abs=1e-5)
    assert all(v.dtype == np.float32 for v in p32.values()) and all(s.dtype == np.float32 for v in st32.values() for s in v)
    baskets = every_length_baskets(L)
    assert so.scores(p32, baskets).dtype == np.float32
    assert 0 < np.max(np.abs(so.scores(p32, baskets) - so.scores(p, baskets))) < 1e-4


# ---- header, bindings, exports -----------------------------------------------------------------------------------------------------------
def _declaration(name):
    with open(os.path.join(ROOT, 'include', 'drx.h')) as f:
        h = f.read()
    m = re.search(r'\b' + name + r'\s*\(([^;]*?)\)\s*;', h, re.S)
    assert m, f'{name} is not declared in include/drx.h'
    return [a for a in m.group(1).split(',') if a.strip()]


@pytest.mark.parametrize('name', ['drx_sas_grid', 'drx_sas_step_scratch_bytes', 'drx_sas_step', 'drx_sas_query_rows'])
def test_header_and_bindings_agree(name):
    from drecpy_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_declaration(name)) == len(_lib.SIGNATURES[name][1])


def dims_of(H, L, blocks, n_items=10):
    """include/drx.h DrxSasDims in its stated layout, built here from the header's words alone"""
    from drecpy_amd._lib import SasDims
    off_blk = L * H
    off_vec = off_blk + 5 * H * H * blocks
    off_lnf = off_vec + 6 * H * blocks
    return SasDims(n_items=n_items, h=H, ldh=(H + 3) // 4 * 4, L=L, blocks=blocks, off_pos=0, off_blk=off_blk, off_vec=off_vec,
                   off_lnf=off_lnf, n_small=off_lnf + 2 * H)


def test_the_library_exports_the_calls_and_refuses_outside_the_domain():
    """host-side checks only: nothing here touches a device"""
    import ctypes as C
    from drecpy_amd._lib import lib
    f = lambda d, *a: lib().drx_sas_step_scratch_bytes(C.byref(d), *a)
    assert f(dims_of(1, 1, 1), 1, 1) > 0 and f(dims_of(64, 16, 2), 64, 16) > f(dims_of(1, 1, 1), 64, 1)
    for H, L, blocks in ((0, 4, 1), (65, 4, 1), (4, 0, 1), (4, 17, 1), (4, 4, 0), (4, 4, 3)):
        assert f(dims_of(H, L, blocks), 64, 1) == 0, (H, L, blocks)
    for B, r in ((0, 1), (-3, 1), (1 << 24, 1), (64, 0), (64, 17)):
        assert f(dims_of(7, 3, 2), B, r) == 0, (B, r)
    for field in ('ldh', 'off_pos', 'off_blk', 'off_vec', 'off_lnf', 'n_small', 'n_items'):
        d = dims_of(7, 3, 2)
        setattr(d, field, 0 if field == 'n_items' else getattr(d, field) + 4)
        assert f(d, 64, 1) == 0, field
    assert [lib().drx_sas_grid(B) for B in (1, 16, 17, 256, 257, 1 << 20)] == [1, 16, 17, 256, 256, 256]
    assert lib().drx_sas_step(None, *([None] * 14), 64, 1, None, None, 0.0, None, None, 0, None) == -1
    assert lib().drx_sas_query_rows(None, None, None, None, None, 1, None, None) == -1


# ---- the class before an engine exists ---------------------------------------------------------------------------------------------------
def test_refusals_word_for_word():
    for r in (0, 1.5, 17):
        assert _refusal('SASRec', {}, dict(neg_ratio=r)) == \
            f'SASRec.fit(neg_ratio={r!r}): neg_ratio must be an integer in 1..16 (negatives drawn per window).'
    assert _refusal('SASRec', dict(L=17), {}) == 'SASRec(L=17): L must be an integer in 1..16.'
    assert _refusal('SASRec', dict(L=0), {}) == 'SASRec(L=0): L must be an integer in 1..16.'
    assert _refusal('SASRec', dict(hidden=65), {}) == 'SASRec(hidden=65): hidden must be an integer in 1..64.'
    assert _refusal('SASRec', dict(hidden=2.5), {}) == 'SASRec(hidden=2.5): hidden must be an integer in 1..64.'
    assert _refusal('SASRec', dict(blocks=3), {}) == 'SASRec(blocks=3): blocks must be an integer in 1..2.'
    assert _refusal('SASRec', dict(blocks=True), {}) == 'SASRec(blocks=True): blocks must be an integer in 1..2.'
    model = _model('SASRec')
    model.optimizer = _NotDense()
    with pytest.raises(Exception) as e:
        model._configure_optimizer()
    assert str(e.value) == ('SASRec trains with the dense rules adam, adagrad, sgd, rmsprop (dense update of both item tables and the '
                            'attention weights); got <not a dense rule>')


def test_process_group_refusal(tmp_path):
    """single GPU only: refused in _pre_fit, before any device work (gloo over a file: no peer, no socket to anywhere)"""
    import torch.distributed as dist
    dist.init_process_group('gloo', init_method=f'file://{tmp_path}/rdzv', rank=0, world_size=1)
    try:
        assert _refusal('SASRec', {}, {}) == 'SASRec.fit under a torch.distributed process group: SASRec trains on a single GPU only.'
    finally:
        dist.destroy_process_group()


def test_draw_seed_and_batch_loss():
    for seed, base in ((None, 0), (0, 0), (10, 10000030)):
        model = _model('SASRec', seed=seed)
        assert [model._draw_seed(k) for k in (1, 7)] == [base + 1, base + 7]
        assert all(type(model._draw_seed(k)) is int for k in (1, 7))
    softplus = float(np.mean(np.log1p(np.exp(-np.abs(X5).astype(np.float64))) + np.maximum(-X5.astype(np.float64), 0.0)))
    assert _model('SASRec')._compute_batch_loss(X5.astype(np.float32), np.ones(5)) == pytest.approx(softplus, rel=1e-15, abs=0)


def test_one_definition_of_serving_and_fit_helpers():
    from drecpy_amd.Recommender import Baseline
    from drecpy_amd.Recommender.Baseline import SASRec, _base, sasrec
    assert 'SASRec' in Baseline.__all__ and issubclass(SASRec, _base.SampledDenseFit)
    for name in SERVING:
        assert name not in SASRec.__dict__, f'SASRec defines {name} itself'
        assert getattr(SASRec, name) is _base.FactorServing.__dict__[name]
    for name in ('_draw_seed', '_configure_optimizer', '_do_batch', '_next_draw_seed', '_start_sampled_fit', '_positives_frame',
                 '_compute_batch_loss'):
        assert name not in SASRec.__dict__, f'SASRec defines {name} itself'
        assert getattr(SASRec, name) is _base.SampledDenseFit.__dict__[name]
    assert '_DENSE_KINDS' not in vars(sasrec) and sasrec.last_items_baskets is _base.last_items_baskets
    assert (SASRec.MODEL, SASRec.NEGATIVES_PER, SASRec.DENSE_UPDATE_OF) == ('SASRec', 'negatives drawn per window',
                                                                          'both item tables and the attention weights')
    assert (SASRec.MAX_HIDDEN, SASRec.MAX_L, SASRec.MAX_BLOCKS, SASRec.MAX_NEG_RATIO) == (64, 16, 2, 16)
    from drecpy_amd.engine_dense import DenseEngine
    from drecpy_amd.engine_rows import RowsRecommender
    from drecpy_amd.engine_sas import SasEngine
    assert 'score_matrix' not in SasEngine.__dict__ and SasEngine.score_matrix is RowsRecommender.__dict__['score_matrix']
    assert '_step_sizes' not in SasEngine.__dict__ and SasEngine._step_sizes is DenseEngine.__dict__['_step_sizes']
    assert SasEngine.ALPHA_OF == (0, 1, 2)


def test_public_names_and_initial_weights():
    from drecpy_amd.Recommender.Baseline import SASRec
    d = SASRec(verbose=False)
    assert (d.hidden, d.L, d.blocks, d.init_std, d.sort_column, d.device) == (64, 10, 2, 0.01, 'timestamp', 'cuda:0')
    H, L, N = 5, 3, 7
    m = SASRec(hidden=H, L=L, blocks=2, seed=11, verbose=False)
    m.n_items = N
    w = m.initial_weights()
    assert list(w) == so.names(2)                           # the order of the flat array, E first, Q and b last
    shapes = {'E': (N, H), 'Pos': (L, H), 'Q': (N, H), 'b': (N,)}
    assert {k: v.shape for k, v in w.items()} == {k: shapes.get(k, (H, H) if k[:2] in ('Wq', 'Wk', 'Wv', 'W1', 'W2') else (H,)) for k in w}
    bound = 1 / np.sqrt(H)
    rng = np.random.default_rng(11)                         # the documented order of the draws
    assert np.array_equal(w['E'], rng.normal(0.0, 0.01, size=(N, H)))
    assert np.array_equal(w['Pos'], rng.normal(0.0, 0.01, size=(L, H)))
    for b in range(2):
        for name in ('Wq', 'Wk', 'Wv', 'W1', 'W2'):
            assert np.array_equal(w[f'{name}{b}'], rng.uniform(-bound, bound, size=(H, H))), (name, b)
    assert np.array_equal(w['Q'], rng.normal(0.0, 0.01, size=(N, H)))
    for k, v in w.items():
        if k.endswith('_g') or k[:-1].endswith('_g'):
            assert (v == 1).all(), k
        elif k == 'b' or k[:2] in ('b1', 'b2') or k.startswith('ln'):
            assert not v.any(), k
    one = SASRec(hidden=H, L=L, blocks=1, seed=11, verbose=False)
    one.n_items = N
    assert list(one.initial_weights()) == so.names(1)
