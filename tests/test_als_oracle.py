"""tests/als_oracle.py against itself and first principles, without a GPU: the half-step against a direct solve per row, the gradient
of L at a solved row by finite differences, the sparse loss against the dense sum, L non-increasing over sweeps, exact zeros for rows
and columns without positives — and the CPU half of the binding (header, ctypes signatures, the exported class)."""
import os
import re

import numpy as np
import pytest

import als_oracle as ao

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = 0.1


@pytest.fixture(scope='module')
def planted():
    """a 37 x 53 frame whose positives follow a rank-3 pattern; user 4 and item 9 have none, user 2 has every other item"""
    rng = np.random.default_rng(11)
    a, b = rng.normal(size=(37, 3)), rng.normal(size=(53, 3))
    R = ((a @ b.T) > 0.8) * rng.integers(1, 6, size=(37, 53))
    R[2] = rng.integers(1, 6, size=53)
    R[4] = 0
    R[:, 9] = 0
    return ao.Frame(40.0 * R)


def test_half_step_is_the_direct_solve_per_row(planted):
    p = ao.init_params(np.random.default_rng(1), 37, 53, 5, std=0.3)
    X = ao.half_step(p['Y'], planted.csr, LAM)
    Y = p['Y']
    for u in range(37):
        w = planted.W[u]
        A = Y.T @ Y + (Y * w[:, None]).T @ Y + LAM * np.eye(5)        # over ALL items: w = 0 off the positives
        b = ((1.0 + w) * (w > 0)) @ Y
        assert np.allclose(X[u], np.linalg.solve(A, b), rtol=1e-11, atol=1e-13), u


def test_the_gradient_vanishes_at_a_solved_row(planted):
    p = ao.init_params(np.random.default_rng(2), 37, 53, 4, std=0.3)
    p['X'] = ao.half_step(p['Y'], planted.csr, LAM)
    base = ao.loss_dense(p, planted, LAM)
    h = 1e-5
    for u in (0, 2, 4, 36):
        for k in range(4):
            up, dn = ({'X': p['X'].copy(), 'Y': p['Y']} for _ in range(2))
            up['X'][u, k] += h
            dn['X'][u, k] -= h
            g = (ao.loss_dense(up, planted, LAM) - ao.loss_dense(dn, planted, LAM)) / (2 * h)
            assert abs(g) <= 1e-6 * max(1.0, base), (u, k, g)
    # and it does not vanish at a row that was not solved
    q = {'X': p['X'] + 0.01, 'Y': p['Y']}
    up, dn = ({'X': q['X'].copy(), 'Y': q['Y']} for _ in range(2))
    up['X'][0, 0] += h
    dn['X'][0, 0] -= h
    assert abs(ao.loss_dense(up, planted, LAM) - ao.loss_dense(dn, planted, LAM)) / (2 * h) > 1e-3


def test_the_sparse_loss_is_the_dense_sum(planted):
    for K, seed in ((1, 3), (5, 4), (16, 5)):
        p = ao.init_params(np.random.default_rng(seed), 37, 53, K, std=0.3)
        a, b = ao.loss(p, planted, LAM), ao.loss_dense(p, planted, LAM)
        assert abs(a - b) <= 1e-12 * abs(b), (K, a, b)


def test_the_loss_never_rises_over_six_sweeps(planted):
    p = ao.init_params(np.random.default_rng(6), 37, 53, 5)
    before = ao.loss(p, planted, LAM)
    _, losses = ao.fit(p, planted, LAM, 6)
    assert losses[0] < before
    assert all(b <= a * (1 + 1e-12) for a, b in zip(losses, losses[1:])), losses


def test_rows_and_columns_without_positives_are_exact_zeros(planted):
    p, _ = ao.fit(ao.init_params(np.random.default_rng(7), 37, 53, 5), planted, LAM, 2)
    assert not p['X'][4].any() and not p['Y'][9].any()
    assert p['X'][3].any() and p['Y'][8].any()
    p32, _ = ao.fit(ao.init_params(np.random.default_rng(7), 37, 53, 5), planted, LAM, 2, dtype=np.float32)
    assert p32['X'].dtype == np.float32 and not p32['X'][4].any() and not p32['Y'][9].any()
    assert np.max(np.abs(p32['X'] - p['X'])) < 1e-3


# ---- the CPU half of the binding ---------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, 'include', 'drx.h')) as f:
        return re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)


def _n_args(header, name):
    m = re.search(r'\b' + name + r'\s*\(([^;]*?)\)\s*;', header, flags=re.S)
    assert m, f'{name} is not declared in include/drx.h'
    return len([a for a in m.group(1).split(',') if a.strip()])


@pytest.mark.parametrize('name, n', [('drx_als_gram_scratch_bytes', 2), ('drx_als_gram', 7), ('drx_als_solve_rows_scratch_bytes', 3),
                                     ('drx_als_solve_rows', 15), ('drx_als_loss_scratch_bytes', 2),
                                     ('drx_als_loss', 15)])
def test_header_and_bindings_agree(name, n):
    import ctypes as C
    from drecpy_amd import _lib
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert _n_args(_header(), name) == len(args) == n
    assert res is (C.c_size_t if name.endswith('scratch_bytes') else C.c_int)
    if name == 'drx_als_solve_rows':
        assert args[10] is C.c_float and args[13] is C.c_size_t and [j for j, a in enumerate(args) if a is C.c_int32] == [7, 8, 9]


def test_the_class_is_exported_and_the_source_is_built():
    from drecpy_amd import build
    from drecpy_amd.Recommender import Baseline
    assert 'ALS' in Baseline.__all__ and Baseline.ALS.__name__ == 'ALS' and Baseline.ALS.MAX_FACTORS == 128
    assert 'drx_als.hip' in build.SOURCES


def test_the_bench_only_switch_is_not_in_the_public_abi():
    from drecpy_amd import _lib
    assert 'parts' not in ' '.join(n for n in _lib.SIGNATURES if n.startswith('drx_als'))
    assert 'solve_rows_parts' not in _header()


def test_the_engine_scratch_holds_every_call_for_any_pair_of_table_sizes():
    """drx_als_gram_scratch_bytes is not monotone in n_rows (strips of ceil(n / 256) rows, at least 64, a multiple of 4: 16 384 rows
    are 256 strips, 20 000 rows 250), so the engine may not size its scratch from the larger table alone.  Host calls only."""
    from drecpy_amd._lib import lib
    from drecpy_amd.engine_als import AlsEngine
    L_ = lib()
    assert L_.drx_als_gram_scratch_bytes(20000, 64) < L_.drx_als_gram_scratch_bytes(16384, 64)
    sizes = (1, 63, 64, 65, 4099, 16383, 16384, 16385, 16640, 20000, 65536, 70000, 1000000)
    for ld in (4, 64, 128):
        for nu in sizes:
            for ni in sizes:
                have = AlsEngine.scratch_need(nu, ni, ld)
                need = [L_.drx_als_gram_scratch_bytes(nu, ld), L_.drx_als_gram_scratch_bytes(ni, ld), L_.drx_als_solve_rows_scratch_bytes(nu, ni, ld),
                        L_.drx_als_solve_rows_scratch_bytes(ni, nu, ld), L_.drx_als_loss_scratch_bytes(nu, ld)]
                assert all(0 < n <= have for n in need), (nu, ni, ld, have, need)
