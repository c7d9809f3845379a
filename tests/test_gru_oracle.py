"""tests/gru_oracle.py without a GPU: its forward pass against torch.nn.GRU in float64, its hand-written backward pass through time
against torch.autograd, its step against tests/optim_oracle.py, short baskets, the window stream, and that include/drx.h, the bindings
and the public package agree on the GRU4Rec entry points."""
import os
import re

import numpy as np
import pytest

import bpr_oracle as bo
import gru_oracle as go
import optim_oracle as oo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (5, 7, 3), (16, 17, 8)]              # (K, H, L)
N_ITEMS = 9


def hand_made_batch(L, n_pool=N_ITEMS):
    """5 windows over 9 items, r = 2: item 4 fills all L inputs of window 0; item 2 is an input of window 1, the target of window 2 and
    a negative of window 3"""
    rng = np.random.default_rng(7 + L)
    before = rng.integers(0, n_pool, size=(5, L))
    before[0, :] = 4
    before[1, 0] = 2
    after = np.array([[5, 0, 7], [3, 8, 0], [2, 4, 6], [1, 2, 7], [8, 3, 0]])
    return np.arange(5), before, after


def _torch_gru(p, K, H):
    """torch.nn.GRU (one layer, float64, CPU) holding the oracle's weights: gates reordered z | r | n -> r | z | n, b_ih = bx,
    b_hh = [0, 0, bhn]"""
    import torch
    order = np.concatenate([np.arange(H, 2 * H), np.arange(0, H), np.arange(2 * H, 3 * H)])
    gru = torch.nn.GRU(K, H, num_layers=1, batch_first=True).double()
    with torch.no_grad():
        gru.weight_ih_l0.copy_(torch.as_tensor(p['Wx'][:, order].T.copy()))
        gru.weight_hh_l0.copy_(torch.as_tensor(p['Wh'][:, order].T.copy()))
        gru.bias_ih_l0.copy_(torch.as_tensor(p['bx'][order].copy()))
        gru.bias_hh_l0.copy_(torch.as_tensor(np.concatenate([np.zeros(2 * H), p['bhn']])))
    return gru, order


@pytest.mark.parametrize('K,H,L', SHAPES)
def test_forward_equals_torch_gru(K, H, L):
    import torch
    p = go.init_params(np.random.default_rng(K + H), N_ITEMS, K, H)
    gru, _ = _torch_gru(p, K, H)
    ids = np.random.default_rng(L).integers(0, N_ITEMS, size=(6, L))
    with torch.no_grad():
        out, hn = gru(torch.as_tensor(p['E'][ids]))
    got, steps = go.run_cell(p, ids)
    assert np.max(np.abs(got - hn[0].numpy())) <= 1e-12
    for t in range(1, L):                                   # every intermediate state too
        assert np.max(np.abs(steps[t][1] - out[:, t - 1].numpy())) <= 1e-12
    assert np.abs(got).max() > 1e-3


@pytest.mark.parametrize('K,H,L', SHAPES)
def test_gradients_equal_autograd(K, H, L):
    import torch
    p = go.init_params(np.random.default_rng(10 + K), N_ITEMS, K, H)
    _, before, after = hand_made_batch(L)
    want_loss, g = go.gradients(p, before, after)
    gru, order = _torch_gru(p, K, H)
    E, Q, b = (torch.tensor(p[n], requires_grad=True) for n in ('E', 'Q', 'b'))
    _, hn = gru(E[torch.as_tensor(before)])
    x = torch.einsum('wh,wjh->wj', hn[0], Q[torch.as_tensor(after)]) + b[torch.as_tensor(after)]
    loss = torch.nn.functional.softplus(-(x[:, :1] - x[:, 1:])).mean()
    loss.backward()
    inv = np.argsort(order)
    auto = {'E': E.grad.numpy(), 'Q': Q.grad.numpy(), 'b': b.grad.numpy(), 'Wx': gru.weight_ih_l0.grad.numpy().T[:, inv],
            'Wh': gru.weight_hh_l0.grad.numpy().T[:, inv], 'bx': gru.bias_ih_l0.grad.numpy()[inv], 'bhn': gru.bias_hh_l0.grad.numpy()[2 * H:]}
    assert abs(want_loss - float(loss.detach())) <= 1e-14 and abs(want_loss - go.loss(p, before, after)) <= 1e-15
    for name in go.NAMES:
        scale = float(np.max(np.abs(auto[name])))
        if name == 'Wh' and L == 1:                         # h_0 = 0: one step has no gradient of Wh
            assert scale == 0.0 and not g[name].any()
            continue
        assert scale > 1e-6, name
        assert np.max(np.abs(g[name] - auto[name])) <= 1e-10 * scale, name


@pytest.mark.parametrize('kind', ['adam', 'adagrad', 'sgd', 'momentum', 'nesterov', 'rmsprop', 'rmsprop_momentum'])
def test_step_is_the_rule_of_the_optim_oracle_on_the_gradients(kind):
    K, H, L = 5, 7, 3
    p = go.init_params(np.random.default_rng(2), N_ITEMS, K, H)
    st = go.init_state(p, kind)
    uid, before, after = hand_made_batch(L)
    for s in range(2):
        start = {k: v.copy() for k, v in p.items()}
        slots = {k: [None if a is None else a.copy() for a in v] for k, v in st.items()}
        _, g = go.gradients(p, before, after)
        alphas = go.step_sizes(s, kind)
        go.step(p, st, s, uid, before, after, kind)
        for name in go.NAMES:
            l2c = go.HP['reg'] if name in ('E', 'Wx', 'Wh', 'Q') else 0.0
            if kind == 'adam':
                assert alphas[name] == bo.adam_alpha(go.HP['lr'], 3 * s + {'E': 0, 'Q': 2, 'b': 2}.get(name, 1) + 1, go.HP['b1'], go.HP['b2'])
                want = bo.du.adam_flat(start[name], slots[name][0], slots[name][1], g[name], alphas[name], l2c, go.HP['b1'], go.HP['b2'],
                                       go.HP['eps'])
                want = (want.p, want.m, want.v)
            else:
                assert alphas[name] == go.HP['lr']
                r = oo.rule_flat(kind, start[name], slots[name][0], slots[name][1], g[name], go.HP['lr'], l2c, mu=go.HP['mu'],
                                 rho=go.HP['rho'], eps=go.HP['eps'])
                want = (r.p, r.s1, r.s2)
            for a, b in zip((p[name], st[name][0], st[name][1]), want):
                assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), (kind, name)
            assert (p[name] != start[name]).any(), name


def test_replay32_runs_the_same_step_in_float32():
    K, H, L = 5, 7, 3
    p = go.init_params(np.random.default_rng(3), N_ITEMS, K, H)
    p32 = go.replay32(p)
    st, st32 = go.init_state(p, 'adam'), go.init_state(p32, 'adam')
    uid, before, after = hand_made_batch(L)
    for s in range(3):
        a, b = go.step(p, st, s, uid, before, after), go.step(p32, st32, s, uid, before, after)
        assert a == pytest.approx(b, abs=1e-5)
    assert all(v.dtype == np.float32 for v in p32.values()) and all(s.dtype == np.float32 for v in st32.values() for s in v)
    baskets = before[:, :L]
    assert go.scores(p32, baskets).dtype == np.float32
    assert 0 < np.max(np.abs(go.scores(p32, baskets) - go.scores(p, baskets))) < 1e-4


def test_a_short_basket_is_a_shorter_model():
    K, H, L = 5, 7, 4
    p = go.init_params(np.random.default_rng(4), N_ITEMS, K, H)
    for m in range(L):
        items = [3, 8, 3][:m]
        basket = np.array([items + [-1] * (L - m)])
        short = go.hidden(p, np.array([items]).reshape(1, m)) if m else np.zeros((1, H))
        assert np.array_equal(go.query_rows(p, basket), short), m
    x = go.scores(p, np.full((2, L), -1))
    assert np.array_equal(x[0], p['b'])                     # an empty basket scores b[i]


def test_windows_are_the_list_samplers_at_one_target():
    """go.windows IS oracle.data_oracle.list_sample_counter at n_targets = 1 and this class's sampler arguments (min = max = L): what is
    checked here is what the model relies on — the structure of its windows and the baskets.  That the device draws this stream is
    tests/test_gpu_gru_api.py's check."""
    L, r = 2, 3
    seqs = [[1, 2, 3, 4, 5], [5], [], [6, 7, 8], [0, 2, 4, 6, 8, 1, 3]]
    twin = go.twin_of(seqs, 12, L, r)
    assert twin['eligible'].tolist() == [0, 3, 4]
    for n, seed in ((1, 0), (64, 1000003 * 3 + 1), (300, 0xFEDCBA9876543210)):
        uid, before, after = go.windows(twin, n, L, r, seed & ((1 << 64) - 1))
        assert set(uid.tolist()) <= {0, 3, 4} and (n < 64 or set(uid.tolist()) == {0, 3, 4})
        assert before.shape == (n, L) and after.shape == (n, 1 + r)
        for u, bf, af in zip(uid, before, after):           # L consecutive items, the next one, r items the sequence does not hold
            s = seqs[int(u)]
            assert any(s[k:k + L + 1] == bf.tolist() + [int(af[0])] for k in range(len(s) - L))
            assert not set(af[1:].tolist()) & set(s) and len(set(af[1:].tolist())) == r
    assert go.baskets_of(twin, 5, L).tolist() == [[4, 5], [5, -1], [-1, -1], [7, 8], [1, 3]]


# ---- header, bindings, exports -----------------------------------------------------------------------------------------------------------
def _declaration(name):
    with open(os.path.join(ROOT, 'include', 'drx.h')) as f:
        h = f.read()
    m = re.search(r'\b' + name + r'\s*\(([^;]*?)\)\s*;', h, re.S)
    assert m, f'{name} is not declared in include/drx.h'
    return [a for a in m.group(1).split(',') if a.strip()]


@pytest.mark.parametrize('name', ['drx_gru_grid', 'drx_gru_step_scratch_bytes', 'drx_gru_step', 'drx_gru_query_rows'])
def test_header_and_bindings_agree(name):
    from drecpy_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_declaration(name)) == len(_lib.SIGNATURES[name][1])


def dims_of(K, H, n_items=10):
    """include/drx.h DrxGruDims in its stated layout, built here from the header's words alone"""
    from drecpy_amd._lib import GruDims
    r4 = lambda x: (x + 3) // 4 * 4
    return GruDims(n_items=n_items, k=K, h=H, ldk=r4(K), ldh=r4(H), off_wx=0, off_wh=3 * K * H, off_bx=3 * (K + H) * H,
                   off_bhn=3 * (K + H) * H + 3 * H, n_small=3 * (K + H) * H + 4 * H)


def test_the_library_exports_the_calls_and_refuses_outside_the_domain():
    """host-side checks only: nothing here touches a device"""
    import ctypes as C
    from drecpy_amd._lib import lib
    f = lambda d, *a: lib().drx_gru_step_scratch_bytes(C.byref(d), *a)
    assert f(dims_of(1, 1), 1, 1, 1) > 0 and f(dims_of(64, 64), 64, 8, 16) > f(dims_of(1, 1), 64, 1, 1)
    for K, H in ((0, 4), (65, 4), (4, 0), (4, 65)):
        assert f(dims_of(K, H), 64, 1, 1) == 0, (K, H)
    for B, L, r in ((0, 1, 1), (64, 0, 1), (64, 9, 1), (64, 1, 0), (64, 1, 17)):
        assert f(dims_of(5, 7), B, L, r) == 0, (B, L, r)
    for field in ('ldk', 'ldh', 'off_wx', 'off_wh', 'off_bx', 'off_bhn', 'n_small', 'n_items'):
        d = dims_of(5, 7)
        setattr(d, field, 0 if field == 'n_items' else getattr(d, field) + 4)
        assert f(d, 64, 1, 1) == 0, field
    assert [lib().drx_gru_grid(B) for B in (1, 16, 17, 4096, 1 << 20)] == [1, 1, 2, 256, 256]
    assert lib().drx_gru_step(None, *([None] * 14), 64, 1, 1, None, None, 0.0, None, None, 0, None) == -1
    assert lib().drx_gru_query_rows(None, None, None, None, 1, None, 1, None, None) == -1


def test_fit_under_a_process_group_raises_by_name(tmp_path):
    """single GPU only: refused in _pre_fit, before any device work"""
    import torch.distributed as dist
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender.Baseline import GRU4Rec
    ds = InteractionDataset.from_arrays(np.array([0, 0, 1]), np.array([0, 1, 1]), np.array([2.0, 3.0, 2.0]), timestamp=np.arange(3))
    dist.init_process_group('gloo', init_method=f'file://{tmp_path}/rendezvous', rank=0, world_size=1)
    try:
        with pytest.raises(Exception, match='single GPU'):
            GRU4Rec(factors=4, hidden=4, verbose=False).fit(ds, epochs=1, batch_size=4)
    finally:
        dist.destroy_process_group()


def test_public_names_and_initial_weights():
    from drecpy_amd.Recommender.Baseline import FPMC, GRU4Rec
    from drecpy_amd.Recommender.Baseline._base import SampledDenseFit
    assert issubclass(GRU4Rec, SampledDenseFit)
    d = GRU4Rec(verbose=False)
    assert (d.factors, d.hidden, d.L, d.init_std, d.sort_column) == (64, 64, 5, 0.01, 'timestamp')
    from drecpy_amd.Recommender.Baseline import _base
    assert callable(_base.last_items_baskets) and issubclass(FPMC, SampledDenseFit)      # (the ONE basket helper of FPMC and GRU4Rec)
    m = GRU4Rec(factors=3, hidden=5, L=2, seed=11, verbose=False)
    m.n_items = 7
    w = m.initial_weights()
    assert {k: v.shape for k, v in w.items()} == {'E': (7, 3), 'Wx': (3, 15), 'Wh': (5, 15), 'bx': (15,), 'bhn': (5,), 'Q': (7, 5), 'b': (7,)}
    assert not w['bx'].any() and not w['bhn'].any() and not w['b'].any()
    assert np.abs(w['Wx']).max() <= 1 / np.sqrt(5) and np.abs(w['Wh']).max() <= 1 / np.sqrt(5) and np.abs(w['Wh']).max() > 0.3
    # the documented order of the draws: E, Wx, Wh, Q
    rng = np.random.default_rng(11)
    assert np.array_equal(w['E'], rng.normal(0.0, 0.01, size=(7, 3)))
    assert np.array_equal(w['Wx'], rng.uniform(-1 / np.sqrt(5), 1 / np.sqrt(5), size=(3, 15)))
    assert np.array_equal(w['Wh'], rng.uniform(-1 / np.sqrt(5), 1 / np.sqrt(5), size=(5, 15)))
    assert np.array_equal(w['Q'], rng.normal(0.0, 0.01, size=(7, 5)))
    for bad in (dict(hidden=2.5), dict(hidden=0), dict(hidden=65), dict(factors=65), dict(L=9)):
        with pytest.raises(Exception, match=list(bad)[0] if list(bad)[0] != 'L' else 'L must'):
            GRU4Rec(verbose=False, **bad)._check_shape()
