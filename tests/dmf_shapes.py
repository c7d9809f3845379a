"""Interaction matrices and batches at the limits of the DMF segmented gather (255 segments per id, _ORDER_EXTRA spare list entries
and partial rows, a gather grid of 8192 workgroups, the segment number in bits 24..31 of an int32), shared by the host tests of the
work list (test_dmf_work_list.py) and the GPU tests against the oracle (test_gpu_dmf.py).  NumPy only."""
import functools

import numpy as np

from oracle import data_oracle as do

SEG = 8                      # the segment length these shapes are made for (DmfEngine._seg_len overridden)
ORDER_EXTRA = 4096           # DmfEngine._ORDER_EXTRA (the tests assert that the two agree)
GATHER_GRID = 8192           # k_dmf_gather's largest grid: more work items take its grid-stride loop


def _matrix(u, i, rng, U, N):
    """values as test_gpu_dmf._problem: integers 1..5"""
    u, i = np.asarray(u, np.int64), np.asarray(i, np.int64)
    v = rng.integers(1, 6, size=len(u)).astype(np.float64)
    return {'U': U, 'N': N, 'u': u, 'i': i, 'v': v, 'csr': do.interaction_csr(u, i, v, U, N), 'csc': do.interaction_csr(i, u, v, N, U)}


def dense(m):
    d = np.zeros((m['U'], m['N']))
    d[m['u'], m['i']] = m['v']
    return d


@functools.lru_cache(maxsize=None)
def blocks():
    """48 users x 1200 items: users 0..39 hold 1100 consecutive items each (138 segments of 8: segment numbers up to 137 set the sign
    bit of an entry), every item below 1194 a column of up to 40 non-zeros (5 segments); users 40..44 hold 6 of the last 100 items,
    users 45..47 nothing, items 1194.. at most those few."""
    rng = np.random.default_rng(101)
    U, N = 48, 1200
    u, i = [], []
    for a in range(40):
        s = (5 * a) % 101
        u.append(np.full(1100, a)); i.append(np.arange(s, s + 1100))
    for a in range(40, 45):
        u.append(np.full(6, a)); i.append(rng.choice(np.arange(1100, N), size=6, replace=False))
    return _matrix(np.concatenate(u), np.concatenate(i), rng, U, N)


def blocks_batch(B, seed):
    """users among the 40 long rows, items among the 1100 every one of them could hold"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 40, size=B).astype(np.int32), rng.integers(0, 1100, size=B).astype(np.int32), rng.random(B).astype(np.float32)


@functools.lru_cache(maxsize=None)
def wide():
    """3000 users x 3000 items for a batch of MORE THAN 4096 distinct ids whose partial rows still fit: user 0 holds items 0..1099 (138
    segments of 8), users 1..800 hold 24 random items (3 segments), the others 3; columns come out at about 9 non-zeros (1 or 2
    segments)."""
    rng = np.random.default_rng(102)
    U = N = 3000
    u, i = [np.zeros(1100, np.int64)], [np.arange(1100)]
    for a in range(1, U):
        n = 24 if a <= 800 else 3
        u.append(np.full(n, a)); i.append(rng.choice(N, size=n, replace=False))
    return _matrix(np.concatenate(u), np.concatenate(i), rng, U, N)


def wide_batch(seed):
    """B = 6000: every user and every item exactly twice"""
    rng = np.random.default_rng(seed)
    U = N = 3000
    uids = np.concatenate([rng.permutation(U), rng.permutation(U)]).astype(np.int32)
    iids = np.concatenate([rng.permutation(N), rng.permutation(N)]).astype(np.int32)
    return uids, iids, rng.random(len(uids)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def one_long_row():
    """4 users x 2100 items: user 0 holds every item — 263 segments of 8, more than the 255 an id may have —, users 1..3 five each"""
    rng = np.random.default_rng(103)
    U, N = 4, 2100
    u, i = [np.zeros(N, np.int64)], [np.arange(N)]
    for a in range(1, U):
        u.append(np.full(5, a)); i.append(rng.choice(N, size=5, replace=False))
    return _matrix(np.concatenate(u), np.concatenate(i), rng, U, N)


def one_long_row_batch(B, seed):
    rng = np.random.default_rng(seed)
    uids = rng.choice(np.array([0, 0, 0, 1, 2, 3], np.int32), size=B)          # the long row in every batch, half of its samples
    return uids.astype(np.int32), rng.integers(0, 2100, size=B).astype(np.int32), rng.random(B).astype(np.float32)


@functools.lru_cache(maxsize=None)
def plain():
    """120 users x 80 items, 2500 random cells (the matrix of the seg_len = 8 bit-for-bit tests): 2..5 segments of 8 per id"""
    rng = np.random.default_rng(104)
    U, N = 120, 80
    cell = rng.choice(U * N, size=2500, replace=False)
    return _matrix(cell // N, cell % N, rng, U, N)


def plain_batch(B, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 120, size=B).astype(np.int32), rng.integers(0, 20, size=B).astype(np.int32), rng.random(B).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tall():
    """1100 users x 30 items, nothing overridden: item 0 is rated by everyone — a column of 1100 > 1024 non-zeros, 2 segments at the
    default length, and a row of K0u that the first-layer update walks with a workgroup —, user 7 rates every item, the others two
    more items each (the ml-1m situation at a size that runs in a second)"""
    rng = np.random.default_rng(105)
    U, N = 1100, 30
    cells = {(a, 0) for a in range(U)} | {(7, b) for b in range(N)}
    for a in range(U):
        cells |= {(a, int(b)) for b in rng.choice(np.arange(1, N), size=2, replace=False)}
    cells = np.array(sorted(cells), np.int64)
    return _matrix(cells[:, 0], cells[:, 1], rng, U, N)


def tall_batch(B, seed):
    rng = np.random.default_rng(seed)
    iids = np.where(rng.random(B) < 0.75, 0, rng.integers(0, 30, size=B))
    uids = rng.integers(0, 1100, size=B)
    uids[0] = 7
    return uids.astype(np.int32), iids.astype(np.int32), rng.random(B).astype(np.float32)


def batch_offsets(m, uids, iids):
    """(off_u, off_i) as drx_batch_distinct leaves them: prefix sums of the degrees of the batch's distinct users / items, ascending"""
    out = []
    for ids, (indptr, _, _) in ((uids, m['csr']), (iids, m['csc'])):
        d = np.unique(np.asarray(ids, np.int64))
        out.append(np.concatenate([[0], np.cumsum(indptr[d + 1] - indptr[d])]).astype(np.int32))
    return out


def rules(off_u, off_i, B, seg_len):
    """What the work list of a host-prepared batch must be, from the rules alone (engine_dmf.DmfEngine.host_work_list):
    cut into segments of seg_len unless an id needs more than 255, the entries exceed 2 B + ORDER_EXTRA, or the partial rows exceed
    ORDER_EXTRA.  Returns (n_work, seg_len in use, n_part, segments per work index), and the same for the rule WITHOUT its last
    clause — the list a batch was given before partial rows were counted."""
    deg = np.concatenate([np.diff(off_u), np.diff(off_i)]).astype(np.int64)
    ns = np.where(deg > seg_len, -(-deg // max(seg_len, 1)), 1) if seg_len > 0 else np.ones(len(deg), np.int64)
    cut = (int(ns.sum()), seg_len, int((ns - 1).sum()), ns)
    uncut = (len(deg), 0, 0, np.ones(len(deg), np.int64))
    fits_list = ns.max(initial=1) <= 255 and ns.sum() <= 2 * B + ORDER_EXTRA
    return (cut if fits_list and cut[2] <= ORDER_EXTRA else uncut), (cut if fits_list else uncut)
