"""tests/bpr_oracle.py without a GPU: its gradients against central finite differences in float64, the properties of its triple stream on
a frame with every kind of edge user, twenty Adam steps on a planted frame, and that include/drx.h, the bindings and the public package
agree on the BPR entry points."""
import os
import re

import numpy as np
import pytest

import bpr_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# 7 users x 9 items, threshold 1.0: user 0 ordinary, 1 without positives (two low pairs), 2 with all 9 items recorded, 3 with 8 recorded
# (complement of one: item 4), 4 whose only recorded pair lies below the threshold, 5 with one positive and one low pair, 6 records nothing
def edge_frame():
    pairs = [(0, 1, 3.0), (0, 5, 2.0), (0, 7, 0.5)]
    pairs += [(1, 2, 0.5), (1, 3, 0.25)]
    pairs += [(2, i, 2.0) for i in range(9)]
    pairs += [(3, i, 1.0 + i) for i in range(9) if i != 4]
    pairs += [(4, 6, 0.5)]
    pairs += [(5, 8, 4.0), (5, 0, 0.1)]
    return bo.Frame(7, 9, pairs, 1.0)


def test_edge_frame_eligibility():
    f = edge_frame()
    assert f.eligible == [0, 3, 5]
    assert f.positives[1] == [] and f.recorded[1] == [2, 3]
    assert len(f.recorded[2]) == 9 and len(f.positives[2]) == 9
    assert f.recorded[3] == [0, 1, 2, 3, 5, 6, 7, 8]
    assert f.positives[4] == [] and f.recorded[4] == [6]
    assert f.positives[0] == [1, 5] and f.recorded[0] == [1, 5, 7]


def test_hash_matches_recorded_values():
    """drx_hash_u32 restated: splitmix64 constants, the top 32 bits — values worked out by hand from the definition"""
    x = (5 + 1 * 0x9E3779B97F4A7C15 + 2 * 0xD1B54A32D192ED03) % (1 << 64)
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 % (1 << 64)
    x ^= x >> 27
    x = x * 0x94D049BB133111EB % (1 << 64)
    x ^= x >> 31
    assert bo.hash_u32(5, 1, 2) == x >> 32 and 0 <= bo.hash_u32(5, 1, 2) < (1 << 32)
    assert bo.hash_u32((1 << 64) - 1, (1 << 32) - 1, (1 << 32) - 1) < (1 << 32)


@pytest.mark.parametrize('held', [[], [0], [8], [0, 1, 2], [1, 3, 5, 7], [0, 1, 2, 3, 5, 6, 7, 8]])
def test_complement_at(held):
    rest = [v for v in range(9) if v not in held]
    assert [bo.complement_at(held, j) for j in range(len(rest))] == rest


@pytest.mark.parametrize('seed', [0, 12345678901234567])
@pytest.mark.parametrize('r', [1, 3])
def test_sampler_properties(seed, r):
    f = edge_frame()
    T = 4096
    uid, pos, neg = bo.sample(f, T, r, seed)
    assert set(uid.tolist()) == set(f.eligible)                       # only the eligible users, and all of them
    for u, i, j in zip(uid.tolist(), pos.tolist(), neg.tolist()):
        assert i in f.positives[u] and j not in f.recorded[u] and 0 <= j < 9
    assert set(neg[uid == 3].tolist()) == {4}                        # a complement of one
    assert set(neg[uid == 0].tolist()) == {0, 2, 3, 4, 6, 8}           # the whole complement, nothing else
    assert set(pos[uid == 0].tolist()) == {1, 5}
    for t in range(T):                                                # consecutive groups of r triples share (u, i)
        assert uid[t] == uid[t - t % r] and pos[t] == pos[t - t % r]
    if r > 1:                                                         # ... and draw their negatives separately
        assert any(neg[t] != neg[t + 1] for t in range(0, T - r, r))
    u2, p2, n2 = bo.sample(f, 100, r, seed)                           # a prefix of the same stream
    assert (u2 == uid[:100]).all() and (p2 == pos[:100]).all() and (n2 == neg[:100]).all()
    assert not (bo.sample(f, T, r, seed + 1)[0] == uid).all()


@pytest.mark.parametrize('K', [1, 5])
def test_gradients_against_central_differences(K):
    rng = np.random.default_rng(3)
    p = bo.init_params(rng, 6, 8, K)
    # users repeat; item 2 is a positive in one triple and a negative in another; item 3 collects both signs twice
    uid = np.array([0, 0, 1, 2, 2, 5, 0])
    pos = np.array([2, 3, 3, 1, 7, 2, 4])
    neg = np.array([3, 2, 0, 3, 3, 6, 2])
    L, g = bo.gradients(p, uid, pos, neg)
    assert abs(L - bo.loss(p, uid, pos, neg)) < 1e-15
    h = 1e-6
    for name in bo.NAMES:
        num = np.zeros_like(p[name])
        it = np.nditer(p[name], flags=['multi_index'])
        for _ in it:
            ix = it.multi_index
            keep = p[name][ix]
            p[name][ix] = keep + h
            up = bo.loss(p, uid, pos, neg)
            p[name][ix] = keep - h
            dn = bo.loss(p, uid, pos, neg)
            p[name][ix] = keep
            num[ix] = (up - dn) / (2 * h)
        assert np.max(np.abs(num - g[name])) < 1e-9, name
        assert np.abs(g[name]).max() > 1e-3, name


def planted_frame():
    """12 users x 16 items in two clusters: users 0..5 record items 0..7, users 6..11 items 8..15 (five of the eight each)"""
    rng = np.random.default_rng(11)
    pairs = []
    for u in range(12):
        base = 0 if u < 6 else 8
        pairs += [(u, base + int(i), 1.0) for i in rng.choice(8, size=5, replace=False)]
    return bo.Frame(12, 16, pairs, 1.0)


def test_twenty_adam_steps_lower_the_loss():
    f = planted_frame()
    assert len(f.eligible) == 12
    p = bo.init_params(np.random.default_rng(5), 12, 16, 8)
    st = bo.init_state(p, 'adam')
    hp = dict(bo.HP, lr=0.05)
    losses = [bo.step(p, st, s, *bo.sample(f, 64, 2, 1000 + s), kind='adam', hp=hp) for s in range(20)]
    assert losses[19] < losses[0] and losses[19] < 0.95 * losses[0], losses
    # the planted structure is found: a user's own cluster outranks the other one on average
    x = bo.scores(p)
    own = np.mean([x[u, (0 if u < 6 else 8):(8 if u < 6 else 16)].mean() - x[u, (8 if u < 6 else 0):(16 if u < 6 else 8)].mean() for u in range(12)])
    assert own > 0


@pytest.mark.parametrize('kind', ['adam', 'adagrad', 'sgd', 'momentum', 'nesterov', 'rmsprop'])
def test_every_rule_steps_and_keeps_its_slots(kind):
    f = planted_frame()
    p = bo.init_params(np.random.default_rng(6), 12, 16, 4)
    p0 = {k: v.copy() for k, v in p.items()}
    st = bo.init_state(p, kind)
    bo.step(p, st, 0, *bo.sample(f, 32, 1, 7), kind=kind)
    n = 2 if kind == 'adam' else bo.oo.N_SLOTS[kind]
    for name in bo.NAMES:
        assert (p[name] != p0[name]).any()
        assert [s is not None for s in st[name]] == [s < n for s in range(2)]


def _declaration(name):
    with open(os.path.join(ROOT, 'include', 'drx.h')) as f:
        h = f.read()
    m = re.search(r'\b' + name + r'\s*\(([^;]*?)\)\s*;', h, re.S)
    assert m, f'{name} is not declared in include/drx.h'
    return [a for a in m.group(1).split(',') if a.strip()]


@pytest.mark.parametrize('name', ['drx_bpr_sample', 'drx_bpr_gather_rows', 'drx_bpr_step_scratch_bytes', 'drx_bpr_step'])
def test_header_and_bindings_agree(name):
    from drecpy_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_declaration(name)) == len(_lib.SIGNATURES[name][1])


def test_fit_under_a_process_group_raises_by_name(tmp_path):
    """single GPU only: refused in _pre_fit, before any device work"""
    import torch.distributed as dist
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender.Baseline import BPR
    ds = InteractionDataset.from_arrays(np.array([0, 0, 1]), np.array([0, 1, 1]), np.array([2.0, 3.0, 2.0]))
    dist.init_process_group('gloo', init_method=f'file://{tmp_path}/rendezvous', rank=0, world_size=1)
    try:
        with pytest.raises(Exception, match='single GPU'):
            BPR(factors=4, verbose=False).fit(ds, epochs=1, batch_size=4)
    finally:
        dist.destroy_process_group()


def test_public_names():
    from drecpy_amd.Recommender.Baseline import BPR
    from drecpy_amd.Recommender.recommender_abc import RecommenderABC
    assert issubclass(BPR, RecommenderABC)
    m = BPR(factors=8, verbose=False)
    assert (m.factors, m.init_std) == (8, 0.01)
    assert BPR(verbose=False).factors == 64
