"""The device point sampler and the offset scan, through the C ABI (include/drx.h), against their CPU statements:
drx_point_sample* bit for bit against oracle/data_oracle.py::point_sample_counter — uid, iid and the float32 bit patterns of y —,
keep_off and drx_batch_offsets exactly against numpy's prefix sums, the mailbox word as the header states it.  One synthetic frame
(helpers.point_sampler_frame): users who record nothing, users who record everything, users recorded without a positive."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import point_sampler_frame
from oracle import data_oracle as do

pytestmark = pytest.mark.gpu

EINVAL, ESCRATCH = -1, -2                  # include/drx.h
TAG = 0x80000001                           # (the top bit set: the word read back as int64 would be negative)
POISON = -7


@functools.lru_cache(maxsize=None)
def _frame():
    return point_sampler_frame()


@functools.lru_cache(maxsize=None)
def _device_frame():
    import torch
    from drecpy_amd._lib import History, ptr
    f = _frame()
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
         (('pi', f['pos'][0]), ('px', f['pos'][1]), ('pv', f['pos'][2]), ('ri', f['rec'][0]), ('rx', f['rec'][1]))}
    return t, History(ptr(t['pi']), ptr(t['px'])), History(ptr(t['ri']), ptr(t['rx']))


@functools.lru_cache(maxsize=None)
def _oracle(B, neg_ratio, seed, recorded, valued=False, vmin=0.0, vrange=0.0):
    f = _frame()
    rec = f['rec'] if recorded else (None, None)
    out = do.point_sample_counter(f['pos'][0], f['pos'][1], rec[0], rec[1], f['U'], f['N'], B, neg_ratio, seed,
                                  values=f['pos'][2] if valued else None, vmin=vmin, vrange=vrange)
    assert not out[4].any()                # (the inputs never reach the 4096-attempt fallback)
    for a in out:
        a.setflags(write=False)
    return out


def _outputs(B):
    import torch
    return (torch.full((B,), POISON, dtype=torch.int32, device='cuda'), torch.full((B,), POISON, dtype=torch.int32, device='cuda'),
            torch.full((B,), float(POISON), dtype=torch.float32, device='cuda'), torch.full((B + 1,), POISON, dtype=torch.int32, device='cuda'))


def _untouched(outs):
    import torch
    torch.cuda.synchronize()
    return all(bool((t == POISON).all()) for t in outs)


def _call(name, B, neg_ratio, seed, recorded, mailbox=False, short=0, n_items=None, rec_struct=None, outs=None):
    """One call of drx_point_sample / _recorded / _by_user on the frame.  Returns (rc, (uid, iid, y, keep_off) tensors, mailbox word)."""
    import torch
    from drecpy_amd import _lib
    L = _lib.lib()
    f = _frame()
    _, H, R = _device_frame()
    need = int(L.drx_point_sample_by_user_scratch_bytes(max(B, 1), f['U']) if name == 'drx_point_sample_by_user'
               else L.drx_point_sample_scratch_bytes(max(B, 1)))
    assert need > 0
    scratch = torch.empty(need, dtype=torch.uint8, device='cuda')
    outs = outs or _outputs(max(B, 1))
    mb = torch.zeros(1, dtype=torch.int64).pin_memory() if mailbox else None
    rec = rec_struct if rec_struct is not None else (R if recorded else None)
    args = [C.byref(H)] + ([] if name == 'drx_point_sample' else [C.byref(rec) if rec is not None else None]) + \
           [f['U'], f['N'] if n_items is None else n_items, B, neg_ratio, seed & (2 ** 64 - 1)] + [_lib.ptr(t) for t in outs] + \
           [_lib.ptr(scratch), need - short, _lib.ptr(mb), TAG if mailbox else 0, _lib.stream_ptr(torch.device('cuda'))]
    rc = getattr(L, name)(*args)
    torch.cuda.synchronize()
    return rc, outs, (int(mb.numpy().view(np.uint64)[0]) if mailbox else None)


def _bits(y):
    return np.ascontiguousarray(y, np.float32).view(np.uint32)


def _assert_batch(outs, word, uid, iid, y):
    """the triples bit for bit, keep_off = the prefix sums of the drawn users' row lengths in hist (keep_off[0] included), the
    mailbox word = (tag << 32) | keep_off[B]"""
    gu, gi, gy, gk = [t.cpu().numpy() for t in outs]
    assert np.array_equal(gu, uid) and gu.dtype == uid.dtype
    assert np.array_equal(gi, iid) and gi.dtype == iid.dtype
    assert np.array_equal(_bits(gy), _bits(y))
    deg_pos = np.diff(_frame()['pos'][0])
    want = np.concatenate([[0], np.cumsum(deg_pos[uid])])
    assert np.array_equal(gk, want)
    assert word == (TAG << 32) | int(want[-1])


RECORDED_CASES = [(B, 3, 0, True) for B in (1, 255, 256, 257, 1023, 1024, 1025, 4096, 4097, 70_001)] + \
                 [(1025, r, 0, True) for r in (0, 1, 7)] + \
                 [(1025, 3, 0, False)] + \
                 [(B, 3, 2 ** 64 - 3, True) for B in (1025, 4097)]


@pytest.mark.parametrize('B,neg_ratio,seed,recorded', RECORDED_CASES)
def test_point_sample_recorded_equals_the_cpu_statement(B, neg_ratio, seed, recorded):
    """drx_point_sample_recorded: batch sizes around the sampler's workgroup (256) and the scan's tile (1024), 70 001 = 274 sampler
    workgroups and 69 scan tiles with the last of each partial; recorded = NULL draws the negatives against the positives."""
    uid, iid, y, _, _ = _oracle(B, neg_ratio, seed, recorded)
    rc, outs, word = _call('drx_point_sample_recorded', B, neg_ratio, seed, recorded, mailbox=True)
    assert rc == 0
    _assert_batch(outs, word, uid, iid, y)
    if neg_ratio == 0:
        assert (y == 1).all()


def test_point_sample_is_point_sample_recorded_without_a_recorded_csr():
    B = 1025
    rc, a, wa = _call('drx_point_sample', B, 3, 0, False, mailbox=True)
    rc2, b, wb = _call('drx_point_sample_recorded', B, 3, 0, False, mailbox=True)
    assert rc == 0 and rc2 == 0 and wa == wb
    for x, z in zip(a, b):
        assert np.array_equal(x.cpu().numpy().view(np.uint32), z.cpu().numpy().view(np.uint32))
    uid, iid, y, _, _ = _oracle(B, 3, 0, False)
    _assert_batch(a, wa, uid, iid, y)


@pytest.mark.parametrize('B', [257, 4097])
def test_point_sample_by_user_is_the_cpu_statement_in_stable_user_order(B):
    """drx_point_sample_by_user: the oracle's draws under a stable sort by user, keep_off and the mailbox for the sorted users; its
    scratch is drx_point_sample_by_user_scratch_bytes, and one byte less is refused before anything is launched."""
    uid, iid, y, _, _ = _oracle(B, 3, 0, True)
    order = np.argsort(uid, kind='stable')
    rc, outs, word = _call('drx_point_sample_by_user', B, 3, 0, True, mailbox=True)
    assert rc == 0
    _assert_batch(outs, word, uid[order], iid[order], y[order])
    rc, outs, word = _call('drx_point_sample_by_user', B, 3, 0, True, mailbox=True, short=1)
    assert rc == ESCRATCH and word == 0 and _untouched(outs)


@pytest.mark.parametrize('recorded', [True, False])
@pytest.mark.parametrize('vmin,vrange', [(1.0, 4.0), (2.0, 5.0), (0.0, 0.0)])
def test_point_sample_valued_targets_value_by_value(vmin, vrange, recorded):
    """drx_point_sample_valued: a positive's target is its pair's value — standardised in float32 when vrange > 0, raw otherwise —, a
    negative's (0 - vmin) / vrange (-0.4 for (2, 5)) or 0."""
    import torch
    from drecpy_amd import _lib
    B, f = 4097, _frame()
    uid, iid, y, _, _ = _oracle(B, 3, 0, recorded, True, vmin, vrange)
    t, H, R = _device_frame()
    gu, gi, gy, _ = _outputs(B)
    rc = _lib.lib().drx_point_sample_valued(C.byref(H), C.byref(R) if recorded else None, _lib.ptr(t['pv']), vmin, vrange, f['U'], f['N'],
                                            B, 3, 0, _lib.ptr(gu), _lib.ptr(gi), _lib.ptr(gy), _lib.stream_ptr(torch.device('cuda')))
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(gu.cpu().numpy(), uid) and np.array_equal(gi.cpu().numpy(), iid)
    assert np.array_equal(_bits(gy.cpu().numpy()), _bits(y))
    # the same pairs as the unvalued draw; the targets' values are the ones the setting names
    plain = _oracle(B, 3, 0, recorded)
    assert np.array_equal(plain[0], uid) and np.array_equal(plain[1], iid)
    neg = plain[2] == 0
    want_neg = {(1.0, 4.0): np.float32(-0.25), (2.0, 5.0): np.float32(-0.4), (0.0, 0.0): np.float32(0)}[(vmin, vrange)]
    assert neg.any() and (y[neg] == want_neg).all()
    want_pos = {(1.0, 4.0): [0.5, 0.75, 1.0], (2.0, 5.0): [np.float32(v) / np.float32(5) for v in (1, 2, 3)], (0.0, 0.0): [3.0, 4.0, 5.0]}
    assert set(y[~neg].tolist()) == set(float(np.float32(v)) for v in want_pos[(vmin, vrange)])


@pytest.mark.parametrize('name', ['drx_point_sample_recorded', 'drx_point_sample_by_user', 'drx_point_sample_valued'])
def test_point_sampler_refusals_launch_nothing(name):
    """B = 0, n_items = 0, neg_ratio = -1 and a recorded CSR without indices are DRX_EINVAL, too little scratch DRX_ESCRATCH; the
    poisoned outputs and the mailbox stay as they were."""
    import torch
    from drecpy_amd import _lib
    f = _frame()
    t, H, R = _device_frame()
    broken = _lib.History(_lib.ptr(t['ri']), None)
    B = 300
    cases = [dict(B=0), dict(n_items=0), dict(neg_ratio=-1), dict(rec_struct=broken)]
    if name == 'drx_point_sample_valued':
        for kw in cases:
            outs = _outputs(B)
            rec = kw.get('rec_struct', R)
            rc = _lib.lib().drx_point_sample_valued(C.byref(H), C.byref(rec), _lib.ptr(t['pv']), 1.0, 4.0, f['U'], kw.get('n_items', f['N']),
                                                    kw.get('B', B), kw.get('neg_ratio', 3), 0, _lib.ptr(outs[0]), _lib.ptr(outs[1]),
                                                    _lib.ptr(outs[2]), _lib.stream_ptr(torch.device('cuda')))
            assert rc == EINVAL and _untouched(outs), kw
        return
    for kw in cases + [dict(short=1)]:
        outs = _outputs(B)
        rc, outs, word = _call(name, kw.get('B', B), kw.get('neg_ratio', 3), 0, True, mailbox=True, short=kw.get('short', 0),
                               n_items=kw.get('n_items'), rec_struct=kw.get('rec_struct'), outs=outs)
        assert rc == (ESCRATCH if 'short' in kw else EINVAL) and word == 0 and _untouched(outs), kw


# ---- drx_batch_offsets --------------------------------------------------------------------------------------------------------------
N_ROWS = 5000


@functools.lru_cache(maxsize=None)
def _rows():
    import torch
    rng = np.random.default_rng(2)
    lengths = np.where(rng.random(N_ROWS) < 1 / 3, 0, rng.integers(1, 10, N_ROWS))
    lengths[0], lengths[-1] = 9, 7                     # (the two rows every batch names count)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indptr.setflags(write=False)
    return indptr, torch.from_numpy(indptr.copy()).cuda()


@pytest.mark.parametrize('B', [1, 1023, 4096, 4097, 262_144, 262_145, 300_001])
def test_batch_offsets_equals_numpy_cumsum(B):
    """drx_batch_offsets: 4096 = one tile and 4097 = two, 262 144 = 64 tiles (the last shape of the tiled path, a full spine), 262 145
    and 300 001 the one-workgroup path with its slab carry (33 and 37 slabs of 8192, the last partial).  Ids repeat and always name
    row 0 and the last row (B = 1: the last row alone).  One byte of scratch less: DRX_ESCRATCH, nothing written."""
    import torch
    from drecpy_amd import _lib
    L = _lib.lib()
    indptr, d_indptr = _rows()
    rng = np.random.default_rng(B)
    ids = rng.integers(0, N_ROWS, B).astype(np.int32)
    if B == 1:
        ids[0] = N_ROWS - 1
    else:
        ids[rng.choice(B, 2, replace=False)] = [0, N_ROWS - 1]
    want = np.concatenate([[0], np.cumsum(np.diff(indptr)[ids])])
    assert want[-1] < 2 ** 31 // 100
    d_ids = torch.from_numpy(ids).cuda()
    need = int(L.drx_point_sample_scratch_bytes(B))
    scratch = torch.empty(need, dtype=torch.uint8, device='cuda')
    st = _lib.stream_ptr(torch.device('cuda'))
    off = torch.full((B + 1,), POISON, dtype=torch.int32, device='cuda')
    assert L.drx_batch_offsets(_lib.ptr(d_indptr), _lib.ptr(d_ids), B, _lib.ptr(off), _lib.ptr(scratch), need - 1, st) == ESCRATCH
    assert _untouched([off])
    assert L.drx_batch_offsets(_lib.ptr(d_indptr), _lib.ptr(d_ids), B, _lib.ptr(off), _lib.ptr(scratch), need, st) == 0
    torch.cuda.synchronize()
    got = off.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(_lib.batch_offsets(d_indptr, d_ids).cpu().numpy(), want)          # the wrapper the engines call
