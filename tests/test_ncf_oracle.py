"""tests/ncf_oracle.py against itself (CPU): its gradients against central finite differences at points that keep a margin from relu's
kink, the split first layer against the concatenated one, its float32 replay, and twenty Adam steps on a planted frame; and that
include/drx.h, the bindings and the public names agree (host-side checks only)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import ncf_oracle as no

U, N = 9, 14


def _batch(rng, B):
    return rng.integers(0, U, size=B), rng.integers(0, N, size=B), rng.integers(0, 2, size=B).astype(np.float64)


@pytest.mark.parametrize('Kg,Km,layers', [(1, 1, (1,)), (3, 5, (7,)), (4, 6, (8, 5)), (8, 32, (32, 16, 8)), (5, 4, (6, 6, 6, 6))])
def test_gradients_match_central_finite_differences(Kg, Km, layers):
    rng = np.random.default_rng(7 + Kg)
    p = no.init_params(rng, U, N, Kg, Km, layers)
    uid, iid, y = _batch(rng, 12)
    no.reset_seen()
    L, g = no.gradients(p, uid, iid, y)
    h = 1e-6
    assert no.seen['min_abs_z'] > 10 * h, 'a pre-activation sits at the kink: choose another seed'
    assert L == pytest.approx(no.loss(p, uid, iid, y), rel=1e-15)
    for name in no.names(p):
        flat = p[name].reshape(-1)
        for at in rng.choice(flat.size, size=min(flat.size, 6), replace=False):
            keep = flat[at]
            flat[at] = keep + h
            up = no.loss(p, uid, iid, y)
            flat[at] = keep - h
            down = no.loss(p, uid, iid, y)
            flat[at] = keep
            assert g[name].reshape(-1)[at] == pytest.approx((up - down) / (2 * h), rel=1e-5, abs=1e-9), (name, at)
    assert not g['Pg'][np.setdiff1d(np.arange(U), uid)].any() and not g['Qm'][np.setdiff1d(np.arange(N), iid)].any()


@pytest.mark.parametrize('Kg,Km,layers', [(1, 1, (1,)), (5, 5, (17, 16)), (8, 32, (32, 16, 8))])
def test_the_split_first_layer_equals_the_concatenated_one(Kg, Km, layers):
    p = no.init_params(np.random.default_rng(3), U, N, Kg, Km, layers)
    a, b = no.logits(p), no.logits_split(p)
    assert a.shape == (U, N) and np.max(np.abs(a - b)) <= 1e-13 * max(1.0, np.abs(a).max())
    hu, hi = no.half_rows(p)
    assert hu.shape == (U, layers[0] + Kg) and hi.shape == (N, layers[0] + Kg)


def test_the_float32_replay_stays_float32_and_close():
    p = no.init_params(np.random.default_rng(5), U, N, 4, 6, (8, 5))
    p32 = no.replay32(p)
    st, st32 = no.init_state(p, 'adam'), no.init_state(p32, 'adam')
    rng = np.random.default_rng(1)
    for s in range(3):
        uid, iid, y = _batch(rng, 20)
        a, b = no.step(p, st, s, uid, iid, y), no.step(p32, st32, s, uid, iid, y)
        assert a == pytest.approx(b, abs=1e-5)
    assert all(v.dtype == np.float32 for v in p32.values()) and all(s.dtype == np.float32 for v in st32.values() for s in v)
    assert no.logits(p32).dtype == np.float32
    assert 0 < np.max(np.abs(no.logits(p32) - no.logits(p))) < 1e-4


@pytest.mark.parametrize('kind', ['adagrad', 'sgd', 'momentum', 'nesterov', 'rmsprop'])
def test_one_step_under_every_rule_moves_every_group_but_not_the_idle_rows_data_gradient(kind):
    p = no.init_params(np.random.default_rng(11), U, N, 3, 5, (7, 4))
    start = {k: v.copy() for k, v in p.items()}
    st = no.init_state(p, kind)
    uid, iid, y = np.array([0, 1, 1]), np.array([2, 2, 3]), np.array([1.0, 0.0, 1.0])
    no.step(p, st, 0, uid, iid, y, kind)
    for name in no.names(p):
        assert (p[name] != start[name]).any(), name
    hp = no.HP
    if kind == 'sgd':                                     # an idle row moves by its regularisation alone
        assert np.allclose(p['Pm'][5], start['Pm'][5] * (1 - hp['lr'] * hp['reg']), rtol=1e-12, atol=0)


def test_twenty_adam_steps_on_a_planted_frame_lower_the_loss_and_rank_the_planted_items_first():
    """every user holds the five planted items 1, 4, 7, 10, 13 of fifteen: every positive is planted, every other pair unrecorded"""
    Un, Nn = 12, 15
    rows = [[1, 4, 7, 10, 13] for u in range(Un)]
    indptr = np.zeros(Un + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    frame = (indptr, np.array([i for r in rows for i in r], np.int32), None, None, Un, Nn)
    p = no.init_params(np.random.default_rng(0), Un, Nn, 4, 8, (16, 8), bias_scale=0.05)
    hp = dict(no.HP, lr=5e-2)
    losses = no.fit(p, frame, 20, 256, 2, lambda k: 1000003 * 5 + k, hp=hp)
    assert losses[-1] < 0.9 * losses[0], losses
    x = no.logits(p)
    for u in range(Un):
        top = np.argsort(-x[u])[:len(rows[u])]
        assert sorted(top.tolist()) == rows[u], (u, top)


# ---- header, bindings, exports -----------------------------------------------------------------------------------------------------------
def _declaration(name):
    with open(os.path.join(ROOT, 'include', 'drx.h')) as f:
        h = f.read()
    m = re.search(r'\b' + name + r'\s*\(([^;]*?)\)\s*;', h, re.S)
    assert m, f'{name} is not declared in include/drx.h'
    return [a for a in m.group(1).split(',') if a.strip()]


@pytest.mark.parametrize('name', ['drx_ncf_grid', 'drx_ncf_step_scratch_bytes', 'drx_ncf_step', 'drx_ncf_half_width', 'drx_ncf_half_rows',
                                  'drx_ncf_score_rows', 'drx_ncf_pair_scores'])
def test_header_and_bindings_agree(name):
    from drecpy_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_declaration(name)) == len(_lib.SIGNATURES[name][1])


def _dims(Kg, Km, layers, n_users=10, n_items=10):
    """include/drx.h DrxNcfDims in its stated layout, built here from the header's words alone"""
    from drecpy_amd._lib import NcfDims
    d = NcfDims(n_users=n_users, n_items=n_items, kg=Kg, km=Km, ldg=(Kg + 3) // 4 * 4, ldm=(Km + 3) // 4 * 4, n_layers=len(layers))
    off, fin = 0, 2 * Km
    for l, fo in enumerate(layers):
        d.f[l], d.off_w[l], d.off_b[l] = fo, off, off + fin * fo
        off, fin = off + fin * fo + fo, fo
    d.off_h, d.off_b0, d.n_small = off, off + Kg + fin, off + Kg + fin + 1
    return d


def test_the_library_exports_the_calls_and_refuses_outside_the_domain():
    """host-side checks only: nothing here touches a device"""
    from drecpy_amd._lib import NcfDims, lib
    L = lib()
    assert C.sizeof(NcfDims) == 22 * 4
    assert [L.drx_ncf_grid(b) for b in (1, 16, 17, 4096, 4097, 1 << 20)] == [1, 1, 2, 256, 256, 256]
    small, large = _dims(1, 1, (1,)), _dims(64, 64, (64, 64, 64, 64))
    assert large.n_small == 128 * 64 + 64 + 3 * (64 * 64 + 64) + 128 + 1
    f = L.drx_ncf_step_scratch_bytes
    assert 0 < f(C.byref(small), 64) < f(C.byref(large), 64) < f(C.byref(large), 4096)
    assert L.drx_ncf_half_width(C.byref(small)) == 8 and L.drx_ncf_half_width(C.byref(_dims(8, 32, (32, 16, 8)))) == 40
    assert L.drx_ncf_half_width(C.byref(_dims(5, 5, (17, 16)))) == 28
    for bad in (_dims(0, 1, (1,)), _dims(65, 1, (1,)), _dims(1, 0, (1,)), _dims(1, 65, (1,)), _dims(4, 4, ()), _dims(4, 4, (65,)),
                _dims(4, 4, (4, 0)), _dims(4, 4, (4,), n_users=0), _dims(4, 4, (4,), n_items=0)):
        assert f(C.byref(bad), 64) == 0
    for b in (0, -1, 1 << 24):
        assert f(C.byref(small), b) == 0
    assert L.drx_ncf_step(*([None] * 13), 64, None, None, 0.0, None, None, 0, None) == -1
    assert L.drx_ncf_half_rows(None, None, None, None, 1, 0, None, None) == -1
    assert L.drx_ncf_score_rows(None, None, None, None, 1, None, None) == -1
    assert L.drx_ncf_pair_scores(None, None, None, None, None, None, 1, None, None) == -1


def test_fit_refuses_before_any_device_work(tmp_path):
    """a process group (single GPU only), neg_ratio < 1 and shapes outside the domain are refused in _pre_fit, by name"""
    import torch.distributed as dist
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender.Baseline import NeuMF
    ds = InteractionDataset.from_arrays(np.array([0, 0, 1]), np.array([0, 1, 1]), np.array([2.0, 3.0, 2.0]))
    kw = dict(epochs=1, batch_size=4)
    for bad, match in ((dict(factors=0), 'NeuMF: factors must'), (dict(factors=65), 'NeuMF: factors must'), (dict(mlp_factors=0), 'mlp_factors must'),
                       (dict(mlp_factors=2.5), 'mlp_factors must'), (dict(layers=()), 'layers must'), (dict(layers=(8,) * 5), 'layers must'),
                       (dict(layers=(8, 65)), 'layers must')):
        with pytest.raises(Exception, match=match):
            NeuMF(verbose=False, **bad).fit(ds, **kw)
    for r in (0, -1, 2.5):
        with pytest.raises(Exception, match='neg_ratio'):
            NeuMF(verbose=False).fit(ds, neg_ratio=r, **kw)
    dist.init_process_group('gloo', init_method=f'file://{tmp_path}/rendezvous', rank=0, world_size=1)
    try:
        with pytest.raises(Exception, match='single GPU'):
            NeuMF(verbose=False).fit(ds, **kw)
    finally:
        dist.destroy_process_group()


def test_public_names():
    from drecpy_amd.Recommender import Baseline
    from drecpy_amd.Recommender.recommender_abc import RecommenderABC
    assert 'NeuMF' in Baseline.__all__ and issubclass(Baseline.NeuMF, RecommenderABC)
    d = Baseline.NeuMF(verbose=False)
    assert (d.factors, d.mlp_factors, tuple(d.layers), d.init_std) == (8, 32, (32, 16, 8), 0.01)
    m = Baseline.NeuMF(factors=4, mlp_factors=6, layers=(12,), init_std=0.1, verbose=False)
    assert (m.factors, m.mlp_factors, tuple(m.layers), m.init_std) == (4, 6, (12,), 0.1)
