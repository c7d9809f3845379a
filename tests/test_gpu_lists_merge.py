"""The split-list merge both selectors end in (k_lists_merge, csrc/drx_keys.hpp) at the borders of its padding: a row's 2 x splits
lists of n keys are ordered in LDS over the next power of two.  Every expected value is exact, from the oracles of the neighbouring
tests: the integer problems of tests/test_gpu_rank_items.py for drx_rows_recommend (the score IS the integer sum under DRX_REC_BIAS),
tests/knn_oracle.py for drx_knn_neighbours.

  scorer   n_items = 1000 = 8 item blocks -> 8 splits (asserted through the scratch size), R = 3, ld = 8:
           n = 4    2 * 8 * 4 = 64 keys: a power of two, no padding slot
           n = 5    80 keys in 128
           n = 128  2048 keys; user 1 keeps 3 eligible items: 3 entries, then -1 / -inf
  table    C = 12, forced splits = 4, one row with 2 positive similarities (entries, then -1 / 0.0):
           R = 40   (2 tiles of 32 rows J, so 2 splits are launched)   k = 8: 32 keys exactly, k = 5: 20 in 32
           R = 100  (4 tiles: the 4 splits asked for)                  k = 8: 64 keys exactly, k = 5: 40 in 64
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, U, LD, SPLITS = 1000, 3, 8, 8
KEPT = (17, 500, 999)                     # what user 1 does not exclude


@functools.lru_cache(maxsize=None)
def _scorer_problem():
    import test_gpu_rank_items as tr
    rng = np.random.default_rng(77)
    table, bias, q = tr._integer_parts(rng, N, U, LD, LD, True)
    z = q.astype(np.float64) @ table.astype(np.float64).T + bias.astype(np.float64)
    rows = [np.zeros(0, np.int64), np.setdiff1d(np.arange(N), KEPT), np.sort(rng.choice(N, N // 3, replace=False))]
    return tr._Problem(table, bias, q, rows, tr.BIAS), z, rows


@pytest.mark.parametrize('n', [4, 5, 128])
def test_scorer_lists_at_the_padding_borders(n):
    from drecpy_amd import _lib
    pb, z, rows = _scorer_problem()
    # 8 splits: 2 * 8 * 128 lists of max(32, 2 n) keys and a count each (+ the size function's alignment slack)
    assert int(_lib.lib().drx_rows_recommend_scratch_bytes(U, N, LD, n)) == 2 * SPLITS * 128 * (max(32, 2 * n) * 8 + 4) + 256
    idx, val = pb.lists(np.arange(U, dtype=np.int32), n)
    for u in range(U):
        elig = np.setdiff1d(np.arange(N), rows[u])
        order = elig[np.lexsort((-elig, -z[u, elig]))][:n]          # descending score, ties to the larger item
        want_idx = np.full(n, -1, np.int32)
        want_val = np.full(n, -np.inf, np.float32)
        want_idx[:len(order)], want_val[:len(order)] = order, z[u, order]
        assert np.array_equal(idx[u], want_idx) and np.array_equal(val[u], want_val), (u, n)
    assert (idx[1, :3] >= 0).all() and (idx[1, 3:] == -1).all() and sorted(idx[1, :3].tolist()) == sorted(KEPT)


@functools.lru_cache(maxsize=None)
def _table_problem(R):
    """random integer ratings in columns 0 .. 10; column 11 belongs to rows 7, 20 and 33, and row 7 has nothing else"""
    import knn_oracle as ko
    rng = np.random.default_rng(R)
    mask = rng.random((R, 12)) < 0.4
    mask[:, 11] = False
    mask[7] = False
    mask[[7, 20, 33], 11] = True
    r, c = np.nonzero(mask)
    return ko.csr_of(r, c, rng.integers(1, 6, len(r)).astype(np.float32), R)


@pytest.mark.parametrize('k', [8, 5])
@pytest.mark.parametrize('R', [40, 100])
def test_neighbour_lists_at_the_padding_borders(R, k):
    import test_gpu_knn as tk
    idx, sim = tk.assert_bit_equal(_table_problem(R), R, 12, 'cosine', k, 0, None, splits=4)
    assert sorted(idx[7, :2].tolist()) == [20, 33] and (idx[7, 2:] == -1).all() and (sim[7, 2:] == 0.0).all() and (sim[7, :2] > 0).all()
    assert (idx[:, k - 1] >= 0).sum() >= R // 2                    # most lists are full: the merge really cuts at k
