"""tests/vae_oracle.py (the definition of record of Mult-VAE) held to torch.autograd in float64 on the same formula, its restatement of
the generator held to its own properties, and the ctypes declarations of drx_vae_* held to include/drx.h.  No GPU, no library load."""
import os
import re

import numpy as np
import pytest

import bpr_oracle as bo
import optim_oracle as oo
import vae_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1e-10
N, H, L, B = 23, 7, 3, 9


def _rows(rng):
    """row 0 holds the whole catalogue, row 1 one item, the others random subsets"""
    return [np.arange(N), np.array([4])] + [np.sort(rng.choice(N, size=int(rng.integers(1, 9)), replace=False)) for _ in range(B - 2)]


def _torch_loss(p, rows, keep, eps, dropout, klw):
    """(loss, {name: gradient}) by torch.autograd, float64, the formulas of the module docstring written with torch operations"""
    import torch
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    latent = p['W_d'].shape[0]
    total = 0.0
    for b, row in enumerate(rows):
        idx = torch.tensor(np.asarray(row, np.int64))
        kept = idx if keep is None else idx[torch.tensor(np.asarray(keep[b], bool))]
        c = 1.0 / (np.sqrt(len(row)) * (1.0 - dropout))
        x1 = c * t['W_in'][kept].sum(dim=0) + t['b_in']
        ml = torch.tanh(x1) @ t['W_e'] + t['b_e']
        mu = ml[:latent]
        z = mu
        if vo.is_variational(p):
            lv = ml[latent:]
            if eps is not None:
                z = mu + torch.tensor(eps[b], dtype=torch.float64) * torch.exp(lv / 2)
            total = total + klw * (-0.5 * (1 + lv - mu * mu - torch.exp(lv)).sum())
        logit = torch.tanh(z @ t['W_d'] + t['b_d']) @ t['W_out'].T + t['b_out']
        total = total - torch.log_softmax(logit, dim=0)[idx].sum()
    loss = total / len(rows)
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in t.items()}


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) / max(1.0, float(np.max(np.abs(b))))


@pytest.mark.parametrize('anneal,step', [(0, 0), (4, 0), (4, 3), (4, 10)])
@pytest.mark.parametrize('dropout', [0.0, 0.5])
@pytest.mark.parametrize('variational', [True, False])
def test_loss_and_gradients_are_torch_autograds(variational, dropout, anneal, step):
    rng = np.random.default_rng(7 + step)
    rows = _rows(rng)
    p = vo.init_params(rng, N, H, L, variational)
    lens = [len(r) for r in rows]
    keep = vo.split(vo.keep_bits(3, lens, dropout), lens) if dropout else None
    if keep is not None:
        keep[2][:] = False                                  # a row with every lookup dropped: x1 = b_in
    eps = vo.noise_of(vo.noise_words(3, B, L))
    klw = vo.beta_t(0.2, anneal, step)
    assert klw == {(0, 0): 0.2, (4, 0): 0.05, (4, 3): 0.2, (4, 10): 0.2}[(anneal, step)]
    loss, g, _ = vo.gradients(p, rows, keep, eps, dropout, klw)
    want, wg = _torch_loss(p, rows, keep, eps, dropout, klw)
    assert abs(loss - want) <= GATE * max(1.0, abs(want))
    for name in vo.NAMES:
        assert _rel(g[name], wg[name]) <= GATE, name


@pytest.mark.parametrize('kind', ('adam',) + oo.KINDS)
def test_a_step_under_every_dense_rule_is_the_rule_on_the_gradients(kind):
    rng = np.random.default_rng(11)
    rows = _rows(rng)
    p = vo.init_params(rng, N, H, L)
    p0 = {k: v.copy() for k, v in p.items()}
    eps = vo.noise_of(vo.noise_words(5, B, L))
    _, g, _ = vo.gradients(p, rows, None, eps, 0.0, 0.2)
    st = vo.init_state(p, kind)
    vo.step(p, st, 2, rows, None, eps, 0.0, 0.2, kind)
    alphas = vo.step_sizes(p0, 2, kind)
    for name in vo.NAMES:
        s1, s2 = vo.init_state(p0, kind)[name]
        want = bo.apply_rule(kind, p0[name], s1, s2, g[name], alphas[name], vo.l2_of(name), vo.HP)
        assert _rel(p[name], want[0]) <= GATE, name
        assert (p[name] != p0[name]).any(), f'{name} did not move under {kind}'
    assert vo.l2_of('b_in') == vo.l2_of('b_out') == 0.0 and vo.l2_of('W_e') == vo.l2_of('W_in') == vo.HP['reg']
    assert alphas['W_in'] != alphas['W_out'] or kind != 'adam'


def test_one_item_gives_a_zero_output_gradient():
    p = vo.init_params(np.random.default_rng(1), 1, 1, 1)
    _, g, _ = vo.gradients(p, [np.array([0])], None, None, 0.0, 0.2)
    assert not g['W_out'].any() and not g['b_out'].any()


def test_scores_use_the_mean_and_no_dropout():
    rng = np.random.default_rng(2)
    rows = _rows(rng) + [np.array([], np.int64)]
    p = vo.init_params(rng, N, H, L)
    x = vo.scores(p, rows)
    t = vo.encode(p, rows)
    assert x.shape == (B + 1, N) and np.array_equal(t['z'], t['mu'])
    assert np.allclose(t['h1'][-1], np.tanh(p['b_in']))    # a user without positives


# ---- the generator ----------------------------------------------------------------------------------------------------------------------
def test_hash_is_the_projects():
    for seed, a, b in ((0, 0, 0), (123, 7, 9), (0xFEDCBA9876543210, 0xFFFFFFFF, 12345)):
        assert int(vo.hash_u32(seed, [a], [b])[0]) == bo.hash_u32(seed, a, b)
    assert vo.q_threshold(0.0) == 0 and vo.q_threshold(0.5) == 1 << 31 and vo.q_threshold(1.0) == 0xFFFFFFFF


def test_keep_bits():
    lens = np.full(1000, 100)
    a, b = vo.keep_bits(9, lens, 0.5), vo.keep_bits(9, lens, 0.5)
    assert a.dtype == bool and len(a) == 100000 and np.array_equal(a, b)
    assert not np.array_equal(a, vo.keep_bits(10, lens, 0.5))
    assert vo.keep_bits(9, lens, 0.0).all()
    for q in (0.5, 0.2, 0.9):
        k = vo.keep_bits(9, lens, q)
        sd = np.sqrt(q * (1 - q) / len(k))
        assert abs(k.mean() - (1 - q)) <= 4 * sd, (q, k.mean())
    # lookup j of row b, whatever the other rows hold
    assert np.array_equal(vo.keep_bits(9, [3, 5], 0.5)[3:], vo.keep_bits(9, [0, 5], 0.5))


def test_noise():
    w = vo.noise_words(4, 2000, 50)
    assert w.shape == (2000, 50, 2) and w.dtype == np.uint32 and np.array_equal(w, vo.noise_words(4, 2000, 50))
    assert np.array_equal(vo.noise_words(4, 10, 50), w[:10]) and not np.array_equal(vo.noise_words(5, 10, 50), w[:10])
    e = vo.noise_of(w)
    n = e.size
    assert np.isfinite(e).all()
    assert abs(e.mean()) <= 4 / np.sqrt(n)
    assert abs(e.var() - 1.0) <= 4 * np.sqrt(2.0 / n)
    assert np.max(np.abs(vo.noise_of(w, np.float32) - e)) < 1e-3


def test_batch_users():
    elig = np.arange(3, 50)
    a = vo.draw_users(6, elig, 16)
    assert len(a) == 16 and len(set(a.tolist())) == 16 and set(a.tolist()) <= set(elig.tolist())
    assert np.array_equal(a, vo.draw_users(6, elig, 16)) and sorted(vo.draw_users(6, elig, 100).tolist()) == elig.tolist()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, 'include', 'drx.h')) as f:
        return re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)


def _n_args(header, name):
    m = re.search(r'\b' + name + r'\s*\(([^;]*?)\)\s*;', header, flags=re.S)
    assert m, f'{name} is not declared in include/drx.h'
    return len([a for a in m.group(1).split(',') if a.strip()])


def test_header_and_bindings_agree():
    import ctypes as C
    from drecpy_amd import _lib
    header = _header()
    for name, n in (('drx_vae_step_scratch_bytes', 4), ('drx_vae_step', 30), ('drx_vae_noise', 10), ('drx_vae_query_rows', 8)):
        assert name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert _n_args(header, name) == len(args) == n, name
        assert res is (C.c_size_t if name.endswith('bytes') else C.c_int)
    assert _lib.SIGNATURES['drx_vae_noise'][1][0] is C.c_uint64
    m = re.search(r'typedef struct DrxVaeDims \{(.*?)\} DrxVaeDims;', header, flags=re.S)
    fields = [f.strip() for part in re.findall(r'int32_t([^;]*);', m.group(1)) for f in part.split(',')]
    assert fields == [f for f, _ in _lib.VaeDims._fields_] and all(t is C.c_int32 for _, t in _lib.VaeDims._fields_)
    with open(os.path.join(ROOT, 'drecpy_amd', 'build.py')) as f:
        assert "'drx_vae.hip'" in f.read()


def test_the_class_is_exported_and_sits_on_the_bases():
    from drecpy_amd.Recommender import Baseline
    from drecpy_amd.Recommender.Baseline import MultVAE, _base
    assert 'MultVAE' in Baseline.__all__ and issubclass(MultVAE, _base.SampledDenseFit)
    for name in ('_draw_seed', '_configure_optimizer', '_do_batch', '_next_draw_seed'):
        assert name not in MultVAE.__dict__ and getattr(MultVAE, name) is _base.SampledDenseFit.__dict__[name]
    for name in ('_predict', '_rank', '_rank_rows', '_recommend_batch', '_catalogue_ranks', '_predict_pairs'):
        assert getattr(MultVAE, name) is _base.FactorServing.__dict__[name]
    m = MultVAE(seed=10, verbose=False)
    assert [m._draw_seed(k) for k in (1, 7)] == [10000031, 10000037]
