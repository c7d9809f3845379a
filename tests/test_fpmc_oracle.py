"""tests/fpmc_oracle.py without a GPU: its gradients against central finite differences in float64, its restriction to M = N = 0 against
tests/bpr_oracle.py, that it learns ORDER where the MF-only restriction cannot, and that include/drx.h, the bindings and the public
package agree on the FPMC entry points."""
import os
import re

import numpy as np
import pytest

import bpr_oracle as bo
import fpmc_oracle as fo
from oracle.data_oracle import list_sample_counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# 5 users x 9 items, L = 3, r = 2: window 0 holds item 4 twice; item 2 is a previous item in window 1, the target of window 2 and a
# negative of window 3; users repeat
UID = np.array([0, 1, 1, 3, 0])
BEFORE = np.array([[4, 1, 4], [2, 5, 6], [0, 7, 8], [3, 3, 5], [6, 2, 1]])
AFTER = np.array([[5, 0, 7], [3, 8, 0], [2, 4, 6], [1, 2, 7], [8, 3, 0]])


@pytest.mark.parametrize('K', [1, 5])
def test_gradients_against_central_differences(K):
    p = fo.init_params(np.random.default_rng(3), 5, 9, K)
    L, g = fo.gradients(p, UID, BEFORE, AFTER)
    assert abs(L - fo.loss(p, UID, BEFORE, AFTER)) < 1e-15
    h = 1e-6
    for name in fo.NAMES:
        num = np.zeros_like(p[name])
        it = np.nditer(p[name], flags=['multi_index'])
        for _ in it:
            ix = it.multi_index
            keep = p[name][ix]
            p[name][ix] = keep + h
            up = fo.loss(p, UID, BEFORE, AFTER)
            p[name][ix] = keep - h
            dn = fo.loss(p, UID, BEFORE, AFTER)
            p[name][ix] = keep
            num[ix] = (up - dn) / (2 * h)
        assert np.max(np.abs(num - g[name])) < 1e-9, name
        assert np.abs(g[name]).max() > 1e-3, name


def test_a_repeated_item_counts_twice():
    p = fo.init_params(np.random.default_rng(4), 5, 9, 3)
    assert np.allclose(fo.context(p, [[4, 1, 4]])[0], (2 * p['M'][4] + p['M'][1]) / 3, rtol=0, atol=1e-16)


@pytest.mark.parametrize('kind', ['adam', 'sgd', 'rmsprop'])
def test_with_M_and_N_held_at_zero_the_step_is_bpr_on_the_windows_triples(kind):
    K, r = 4, AFTER.shape[1] - 1
    p = fo.init_params(np.random.default_rng(5), 5, 9, K)
    p['M'][:], p['N'][:] = 0.0, 0.0
    q = {'P': p['P'].copy(), 'Q': p['Q'].copy(), 'bq': p['b'].copy()}
    st, sq = fo.init_state(p, kind), bo.init_state(q, kind)
    # triple w r + k = (u_w, i_w, j_wk)
    tu, ti, tj = np.repeat(UID, r), np.repeat(AFTER[:, 0], r), AFTER[:, 1:].reshape(-1)
    for s in range(5):
        # (2, 0, 0, 1): the step sizes of BPR's two applies
        a = fo.step(p, st, s, UID, BEFORE, AFTER, kind, applies=(2, 0, 0, 1), hold=('M', 'N'))
        b = bo.step(q, sq, s, tu, ti, tj, kind)
        assert abs(a - b) < 1e-14
    for x, y in (('P', 'P'), ('Q', 'Q'), ('b', 'bq')):
        assert np.max(np.abs(p[x] - q[y])) < 1e-13, x
        assert np.max(np.abs(p[x] - fo.init_params(np.random.default_rng(5), 5, 9, K)[x])) > 1e-4
    assert not p['M'].any() and not p['N'].any()


def test_query_rows_and_baskets():
    p = fo.init_params(np.random.default_rng(6), 3, 7, 2)
    twin = fo.twin_of([[1, 2, 3, 4], [5], []], 7, 3, 2)
    baskets = fo.baskets_of(twin, 3, 3)
    assert baskets.tolist() == [[2, 3, 4], [5, -1, -1], [-1, -1, -1]]
    q = fo.query_rows(p, baskets)
    assert np.allclose(q[0, 2:], p['M'][[2, 3, 4]].mean(axis=0)) and np.array_equal(q[1, 2:], p['M'][5]) and not q[2, 2:].any()
    assert np.array_equal(q[:, :2], p['P'])
    x = fo.scores(p, baskets)
    assert x[2, 3] == pytest.approx(p['P'][2] @ p['Q'][3] + p['b'][3], abs=1e-15)


# ---- order -----------------------------------------------------------------------------------------------------------------------------
def _cycle_frame():
    """40 users x 30 items: every sequence is 10 consecutive items of one random single-cycle permutation; the last one is held out"""
    rng = np.random.default_rng(17)
    cycle = rng.permutation(30)
    seqs = [[int(cycle[(s + t) % 30]) for t in range(10)] for s in rng.integers(0, 30, size=40)]
    return [s[:-1] for s in seqs], [s[-1] for s in seqs]


def _mean_rank(p, baskets, train, held_out):
    x = fo.scores(p, baskets)
    ranks = []
    for u, (seen, i) in enumerate(zip(train, held_out)):
        allowed = np.setdiff1d(np.arange(x.shape[1]), seen)                # novelty on
        ranks.append(int((x[u, allowed] > x[u, i]).sum()))
    return float(np.mean(ranks))


def test_the_oracle_learns_order_where_the_mf_restriction_does_not():
    train, held_out = _cycle_frame()
    L, K, r = 1, 8, 3
    twin = fo.twin_of(train, 30, L, r)
    assert len(twin['eligible']) == 40
    baskets = fo.baskets_of(twin, 40, L)
    draws = [list_sample_counter(twin, 64, L, 1, r, 1000003 + s) for s in range(300)]
    hp = dict(fo.HP, lr=0.05)
    result = {}
    for hold in ((), ('M', 'N')):
        p = fo.init_params(np.random.default_rng(23), 40, 30, K)
        if hold:
            p['M'][:], p['N'][:] = 0.0, 0.0
        st = fo.init_state(p, 'adam')
        for s, (uid, before, after) in enumerate(draws):
            fo.step(p, st, s, uid, before, after, 'adam', hp=hp, hold=hold)
        result[hold] = _mean_rank(p, baskets, train, held_out)
    print('mean catalogue rank of the held-out item: FPMC', result[()], ' MF only', result[('M', 'N')])
    assert result[()] < result[('M', 'N')], result


# ---- header, bindings, exports -----------------------------------------------------------------------------------------------------------
def _declaration(name):
    with open(os.path.join(ROOT, 'include', 'drx.h')) as f:
        h = f.read()
    m = re.search(r'\b' + name + r'\s*\(([^;]*?)\)\s*;', h, re.S)
    assert m, f'{name} is not declared in include/drx.h'
    return [a for a in m.group(1).split(',') if a.strip()]


@pytest.mark.parametrize('name', ['drx_fpmc_step_scratch_bytes', 'drx_fpmc_step', 'drx_fpmc_query_rows'])
def test_header_and_bindings_agree(name):
    from drecpy_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_declaration(name)) == len(_lib.SIGNATURES[name][1])


def test_the_library_exports_the_calls_and_refuses_outside_the_domain():
    """host-side checks only: nothing here touches a device"""
    from drecpy_amd._lib import lib
    f = lib().drx_fpmc_step_scratch_bytes
    assert f(64, 1, 1, 4, 10, 10) > 0 and f(64, 8, 16, 128, 10, 10) > f(64, 1, 1, 4, 10, 10)
    for bad in ((0, 1, 1, 4, 10, 10), (64, 0, 1, 4, 10, 10), (64, 9, 1, 4, 10, 10), (64, 1, 0, 4, 10, 10), (64, 1, 17, 4, 10, 10),
                (64, 1, 1, 0, 10, 10), (64, 1, 1, 6, 10, 10), (64, 1, 1, 132, 10, 10), (64, 1, 1, 4, 0, 10), (64, 1, 1, 4, 10, 0)):
        assert f(*bad) == 0, bad
    assert lib().drx_fpmc_step(*([None] * 12), 4, 10, 10, None, None, None, 64, 1, 1, None, None, 0.0, None, None, 0, None) == -1
    assert lib().drx_fpmc_query_rows(None, None, 4, None, 1, None, 1, None, None) == -1


def test_fit_under_a_process_group_raises_by_name(tmp_path):
    """single GPU only: refused in _pre_fit, before any device work"""
    import torch.distributed as dist
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender.Baseline import FPMC
    ds = InteractionDataset.from_arrays(np.array([0, 0, 1]), np.array([0, 1, 1]), np.array([2.0, 3.0, 2.0]), timestamp=np.arange(3))
    dist.init_process_group('gloo', init_method=f'file://{tmp_path}/rendezvous', rank=0, world_size=1)
    try:
        with pytest.raises(Exception, match='single GPU'):
            FPMC(factors=4, verbose=False).fit(ds, epochs=1, batch_size=4)
    finally:
        dist.destroy_process_group()


def test_public_names():
    from drecpy_amd.Recommender.Baseline import FPMC
    from drecpy_amd.Recommender.recommender_abc import RecommenderABC
    assert issubclass(FPMC, RecommenderABC)
    m = FPMC(factors=8, L=3, verbose=False)
    assert (m.factors, m.L, m.init_std, m.sort_column) == (8, 3, 0.01, 'timestamp')
    d = FPMC(verbose=False)
    assert (d.factors, d.L) == (64, 1)
