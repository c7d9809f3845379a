"""The counts that ride in the sampled step's touch kernel (csrc/drx_prep.hpp k_sparse_touches_rounds) and the fold that replaces the
sort's counting launch (csrc/drx_sort.hip k_fold_counts), read through drx_debug_prep_counts (include/drx.h) BEFORE a sort trusts them:
the first digit's histogram, the 256 degree-bucket counts, the raw keys / vals, the hot mask and the row-sharded caller's presence
marks, all compared EXACTLY with a NumPy restatement (integer counts: nothing to tolerate).

Shapes, where the round logic can go wrong: batches of less than / exactly / just over one and two rounds of 16 samples; fewer rounds
than the launch has workgroups and more; an odd number of rounds (the mask's tail half-word); users without history (also as the
batch's last sample, whose lanes pad the list) and one longer than 16 lanes x 8; catalogues of 3 items and of 255 / 256 / 257; explicit
keep bytes; heads of 0 / 32 / 64 rows; key widths whose first digit is 8 bits (the fold) and 11 bits (the counting launch stays)."""
import ctypes as C

import numpy as np
import pytest
import torch

from prep_oracle import _expect, _wire      # (the statement of the unsorted list: shared with tests/test_gpu_prep_list.py)

NONE = 0xFFFFFFFF
_cache = {}


def _history(U, N, mean_deg, seed):
    """CSR of unique ascending items per user; users 0 and 2 and the LAST user have none, user 1 has min(N, 300) (> 16 x 8)."""
    key = (U, N, mean_deg, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        pop = 1.0 / np.arange(1, N + 1) ** 1.05
        d = np.minimum(rng.poisson(mean_deg, size=U), N)
        d[[0, 2, U - 1]] = 0
        d[1] = 0
        rows = np.repeat(np.arange(U), d)
        cols = rng.choice(N, size=rows.size, p=pop / pop.sum())
        long_ = rng.permutation(N)[:min(N, 300)]
        pairs = np.unique(np.concatenate([rows * N + cols, 1 * N + long_]))
        rows, cols = pairs // N, pairs % N
        indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=U))]).astype(np.int64)
        _cache[key] = (indptr, cols.astype(np.int32))
    return _cache[key]


def _engine(U, N, mean_deg, seed=0):
    key = ('eng', U, N, mean_deg, seed)
    if key not in _cache:
        from drecpy_amd.engine import CdaeEngine
        indptr, indices = _history(U, N, mean_deg, seed)
        eng = CdaeEngine(U, N, 16)
        eng.set_history(indptr, indices, with_transpose=False)
        _cache[key] = eng
    return _cache[key]


def _check(U, N, B, mean_deg=12, H=0, explicit_keep=False, presence=None, q=0.2, seed=77, slack=37, uid_fix=True):
    from drecpy_amd import _lib
    L = _lib.lib()
    eng = _engine(U, N, mean_deg)
    indptr, indices = _history(U, N, mean_deg, 0)
    rng = np.random.default_rng(1000 + B + 7 * H)
    uid = rng.integers(0, U, size=B)
    if uid_fix:                                       # the long user, users without history, one of them as the batch's last sample
        for at, u in ((0, 1), (1, 0), (B // 2, 2), (B - 1, U - 1)):
            if at < B:
                uid[at] = u
    iid = rng.integers(0, N, size=B)
    deg = indptr[uid + 1] - indptr[uid]
    tot = int(deg.sum())
    keep = (rng.random(max(tot, 1)) >= 0.35).astype(np.uint8) if explicit_keep else None
    eng.set_hot_rows(H, min_batch=0)
    slot_of = eng._hot_slot.cpu().numpy().astype(np.int64) if H else None
    want = _expect(indptr, indices, N, uid, iid, seed, q, keep, slot_of, H, slack)
    keep_off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    bt, alive = eng.make_batch(uid.astype(np.int32), iid.astype(np.int32), np.zeros(B, np.float32), keep_off=keep_off, keep=keep, q=q,
                               mask_seed=seed, n_touch_slots=tot + slack)
    dev = eng.device
    nbytes = int(L.drx_cdae_prep_bytes_hot(C.byref(eng._params), B, bt.n_touch_slots, H))
    buf = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=dev)     # (every word that is read was written by the launch)
    T = want['T']
    hist_o = torch.full((2048,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    buck_o = torch.zeros(256, dtype=torch.int32, device=dev)
    keys_o = torch.zeros(T, dtype=torch.int32, device=dev)
    vals_o = torch.zeros(T, dtype=torch.int32, device=dev)
    Bw = (B + 31) // 32
    mask_o = torch.full((max(H, 1) * Bw,), -1, dtype=torch.int32, device=dev)
    present = None
    if presence:
        ipr, cshift, world = presence
        size = int(_wire(np.repeat(np.arange(N), 2), np.tile([0, 1], N), ipr, cshift, world).max()) + 1
        present = torch.zeros(size, dtype=torch.uint8, device=dev)
    info = (C.c_int32 * 4)()
    hot = eng._hot_head(H)
    rc = L.drx_debug_prep_counts(C.byref(eng._params), C.byref(eng._hist), C.byref(bt), C.byref(hot) if H else None,
                                 _lib.ptr(present) if presence else None, *(presence or (0, 0, 0)), _lib.ptr(buf), buf.numel(),
                                 _lib.ptr(hist_o), _lib.ptr(buck_o), _lib.ptr(keys_o), _lib.ptr(vals_o), _lib.ptr(mask_o), info,
                                 _lib.stream_ptr(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    dbits, folded, slots, grid = info[0], info[1], info[2], info[3]
    assert slots == T
    assert folded in (0, grid) and (dbits == 8 or folded == 0)      # (counts are never handed to a plan of another width)
    keys = keys_o.cpu().numpy().view(np.uint32)
    vals = vals_o.cpu().numpy().view(np.uint32)
    assert np.array_equal(keys, want['keys'])
    assert np.array_equal(vals, want['vals'])
    radix = 1 << dbits
    live = want['keys'][want['keys'] != NONE]
    assert np.array_equal(hist_o.cpu().numpy().view(np.uint32)[:radix], np.bincount(live & (radix - 1), minlength=radix))
    assert np.array_equal(buck_o.cpu().numpy().view(np.uint32), want['buckets'])
    if H:
        assert np.array_equal(mask_o.cpu().numpy().view(np.uint32).reshape(H, Bw), want['mask'])
    if presence:
        exp = np.zeros(present.numel(), dtype=np.uint8)
        exp[_wire(want['kept_items'], 0, *presence)] = 1
        exp[_wire(iid, 1, *presence)] = 1
        assert np.array_equal(present.cpu().numpy(), exp)
    return dict(dbits=dbits, folded=folded, grid=grid, want=want)


def _grid():
    """Workgroups of the touch kernel's launch at a batch of many rounds (2500)."""
    if 'grid' not in _cache:
        _cache['grid'] = _check(60000, 1100, 40000)['grid']
        assert _cache['grid'] < 2500
    return _cache['grid']


# 2 N + U + 1 = 6501: 13-bit keys, two 8-bit digits (the fold); = 1701: 11 bits, one 11-bit digit (the counting launch stays)
@pytest.mark.gpu
@pytest.mark.parametrize('U,N,dbits', [(500, 3000, 8), (300, 700, 11)])
@pytest.mark.parametrize('B', [1, 15, 16, 17, 31, 33, 1000])
def test_counts_keys_and_buckets_at_the_round_edges(B, U, N, dbits):
    got = _check(U, N, B)
    assert got['dbits'] == dbits
    assert got['grid'] == (B + 15) // 16                  # fewer rounds than the launch would have workgroups: one workgroup a round
    if B >= 15:
        assert got['want']['deg'].max() > 128 and got['want']['deg'].min() == 0      # (the long user and the empty ones are in the batch)


@pytest.mark.gpu
@pytest.mark.parametrize('B', [33, 1000])
def test_counts_with_explicit_keep_bytes(B):
    _check(500, 3000, B, explicit_keep=True)


@pytest.mark.gpu
@pytest.mark.parametrize('N', [3, 255, 256, 257])
def test_counts_at_tiny_catalogues_and_around_256_items(N):
    """N = 3: the W keys' first digit takes three values (all of a wave's adds on three counters); 255 / 256 / 257: the W2T keys
    N + iid start just below / at / just above a digit's wrap."""
    got = _check(3000, N, 1000, mean_deg=3 if N == 3 else 12)
    assert got['dbits'] == 8


@pytest.mark.gpu
@pytest.mark.parametrize('H', [0, 32, 64])
@pytest.mark.parametrize('extra', [40, 64])
def test_counts_and_mask_with_more_rounds_than_workgroups(H, extra):
    """B = 16 x workgroups + 40 / + 64 (>= 8192, n_items >= 16 H: the head's own gates): every workgroup strides over several rounds,
    the table is built once and the mask words per round; + 40: an odd number of rounds — the last one writes the zero half-word
    behind the batch — and a last round of 8 samples; + 64: an even number."""
    G = _grid()
    B = max(16 * G, 8192) + extra
    got = _check(60000, 1100, B, H=H)       # (2 N + U + 1 = 62 201: 16-bit keys, 8-bit digits; T <= 8 (2 N + U): a head fits)
    assert got['dbits'] == 8 and got['grid'] == G and (B + 15) // 16 > G
    assert ((B + 15) // 16) % 2 == (1 if extra == 40 else 0)


@pytest.mark.gpu
def test_presence_marks_of_the_row_sharded_caller():
    _check(500, 3000, 1000, presence=(1000, 2, 3))


@pytest.mark.gpu
@pytest.mark.parametrize('H', [0, 64])
def test_two_prepared_runs_are_bit_equal(H):
    """Two preparations of the same batches give the same sorted keys, samples, marks and masks — compared through the step: three
    prepared steps from equal tables end bit-equal (B = 2000: an odd number of rounds)."""
    from test_gpu_hot_head import _run
    _, _, _, a = _run(128, H, True, oracle=False, B=2000)
    _, _, _, b = _run(128, H, True, oracle=False, B=2000)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
