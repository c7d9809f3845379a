"""The PREPARED touch list — what drx_cdae_sparse_prepare / _hot leave for a step: the sorted (key, sample) pairs, the sole-toucher
marks, the blanked keys and the forward kernel's launch order — read back through drx_debug_prep_result (include/drx.h) and compared
EXACTLY with tests/prep_oracle.py.  The buffer is written by the library's real preparation (engine.prepare_sparse: touch kernel with
its fold rider, the sort in drop mode on a temp the touch kernel zeroed, plan-and-mark launch); the unsorted list it starts from is the
one tests/test_gpu_prep_counts.py compares with the touch kernel (prep_oracle._expect), on that file's histories: users without
history (one of them the batch's last sample), one user of min(N, 300) items.

A slip this catches and a training step's float results would not: two samples changing places inside a run of equal keys (only the
summation order changes), a mark or a blanked key on the wrong sample where the row's gradient is tiny, an order that loses a sample
whose twin computes the same triple."""
import ctypes as C

import numpy as np
import pytest
import torch

import prep_oracle as po
from prep_oracle import NONE, _expect
from test_gpu_prep_counts import _cache, _grid, _history

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A


def _engine(U, N, K, mean_deg, transpose=False):
    key = ('list-eng', U, N, K, mean_deg, transpose)
    if key not in _cache:
        from drecpy_amd.engine import CdaeEngine
        indptr, indices = _history(U, N, mean_deg, 0)
        eng = CdaeEngine(U, N, K)
        eng.share_users = False                           # the plain list: one touch per kept (sample, item), never the shared-user form
        eng.set_history(indptr, indices, with_transpose=transpose)
        eng.init_optimizer('adagrad', 0.05, 1e-3)         # (a head is granted to the streamed Adagrad step only: _hot_for)
        _cache[key] = eng
    return _cache[key]


def _prepare(U, N, B, K=64, mean_deg=12, H=0, via_hot=False, explicit_keep=False, transpose=False, crowd=False, q=0.2, seed=77, slack=37):
    """Prepares one batch with the engine and reads the result back; returns (device copies, the unsorted list's statement, inputs)."""
    from drecpy_amd import _lib
    L = _lib.lib()
    eng = _engine(U, N, K, mean_deg, transpose)
    indptr, indices = _history(U, N, mean_deg, 0)
    rng = np.random.default_rng(1000 + B + 7 * H)
    uid = rng.integers(0, U, size=B)
    for at, u in ((0, 1), (1, 0), (B // 2, 2), (B - 1, U - 1)):      # the long user, users without history, one as the last sample
        if at < B:
            uid[at] = u
    if crowd:                                             # one user with more than 64 samples of the batch, scattered over it
        uid[rng.permutation(B)[:100]] = 5
    iid = rng.integers(0, N, size=B)
    deg = indptr[uid + 1] - indptr[uid]
    tot = int(deg.sum())
    keep = (rng.random(max(tot, 1)) >= 0.35).astype(np.uint8) if explicit_keep else None
    eng.set_hot_rows(H, min_batch=0)
    keep_off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    bt, alive = eng.make_batch(uid.astype(np.int32), iid.astype(np.int32), np.zeros(B, np.float32), keep_off=keep_off, keep=keep, q=q,
                               mask_seed=seed, n_touch_slots=tot + slack)
    need = int(L.drx_cdae_prep_bytes_hot(C.byref(eng._params), B, bt.n_touch_slots, H))
    buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=eng.device)      # (every word that is read was written by the preparation)
    prep = eng.prepare_sparse(bt, out=buf, hot=via_hot or H > 0)      # (hot=True without hot rows: the plain preparation)
    assert prep is buf
    granted = int(prep._drx_hot)
    assert granted == H                                   # rows of 64 floats, Adagrad, short segments: the head is granted whole
    slot_of = eng._hot_slot.cpu().numpy().astype(np.int64) if granted else None
    unsorted = _expect(indptr, indices, N, uid, iid, seed, q, keep, slot_of, granted, slack)
    T = unsorted['T']
    dev = eng.device
    keys_o = torch.full((T,), SENT, dtype=torch.int32, device=dev)
    vals_o = torch.full((T,), SENT, dtype=torch.int32, device=dev)
    sv_o = torch.full((B,), 0x77, dtype=torch.uint8, device=dev)
    so_o = torch.full((B,), 0x77, dtype=torch.uint8, device=dev)
    order_o = torch.full((B,), -1, dtype=torch.int32, device=dev)
    rc = L.drx_debug_prep_result(C.byref(eng._params), B, bt.n_touch_slots, granted, _lib.ptr(prep), prep.numel(), _lib.ptr(keys_o),
                                 _lib.ptr(vals_o), _lib.ptr(sv_o), _lib.ptr(so_o), _lib.ptr(order_o), _lib.stream_ptr(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = dict(keys=keys_o.cpu().numpy().view(np.uint32), vals=vals_o.cpu().numpy().view(np.uint32), solo_v=sv_o.cpu().numpy(),
               solo_o=so_o.cpu().numpy(), order=order_o.cpu().numpy())
    return got, unsorted, dict(uid=uid, iid=iid, keep_off=keep_off, ld=eng.ld, N=N, B=B, T=T)


def _check_sorted_road(U, N, B, **kw):
    got, unsorted, x = _prepare(U, N, B, **kw)
    want = po.prepared(unsorted['keys'], unsorted['vals'], N, B, x['keep_off'], x['ld'])
    po.check_prepared(got['keys'], got['vals'], got['solo_v'], got['solo_o'], got['order'], want)
    return got, want, x


# 2 N + U + 1 = 6501: 13-bit keys, the fold, two 8-bit passes; = 1701: 11 bits, the counting launch, one 11-bit pass
@pytest.mark.parametrize('U,N', [(500, 3000), (300, 700)], ids=['13bit-fold-2x8', '11bit-counted-1x11'])
@pytest.mark.parametrize('B', [1, 15, 17, 1000])
def test_prepared_list_marks_and_order(B, U, N):
    """K = 64 (rows of 64 floats: marks are made).  B = 1000: a list of more than one tile of the sort."""
    got, want, x = _check_sorted_road(U, N, B)
    assert want['n'] == x['T'] and 2 * B <= want['n_valid'] < x['T']           # (dropped entries and the slack: padding behind the list)
    if B == 1000:
        assert want['n_valid'] > po.SORT_TILE
        # sole touchers and shared rows of both kinds are in the batch, and the long user's bucket beside the empty users'
        assert 0 < want['solo_v'].sum() < B and 0 < want['solo_o'].sum() < B and len(set(want['bucket'].tolist())) > 3
    else:
        assert want['blank'].sum() == want['solo_v'].sum() + want['solo_o'].sum() > 0


def test_prepared_list_with_explicit_keep_bytes():
    _check_sorted_road(500, 3000, 1000, explicit_keep=True)


@pytest.mark.parametrize('B', [17, 1000])
def test_rows_of_16_floats_get_no_marks(B):
    """K = 16 (ld <= 16): nothing is marked, no key is blanked, and the launch order comes from order_by_degree's two launches, not
    from the plan-and-mark launch."""
    got, want, x = _check_sorted_road(500, 3000, B, K=16)
    assert x['ld'] == 16 and not want['blank'].any() and not got['solo_v'].any() and not got['solo_o'].any()
    assert np.array_equal(got['keys'][:want['n_valid']], want['live_keys'])


@pytest.mark.parametrize('H', [0, 64])
def test_prepared_list_with_more_rounds_than_workgroups_and_a_hot_head(H):
    """B = 16 x the touch kernel's workgroups + 40 (test_gpu_prep_counts.py's shape) through prepare_sparse(bt, hot=True) after
    set_hot_rows(H, min_batch=0): drx_cdae_sparse_prepare_hot.  The kept entries of hot items are absent from the list (_expect); the
    engine grants the whole head at K = 64 with Adagrad (asserted in _prepare through the buffer's _drx_hot)."""
    G = _grid()
    B = max(16 * G, 8192) + 40
    got, want, x = _check_sorted_road(60000, 1100, B, H=H, via_hot=True)
    if H:
        eng = _engine(60000, 1100, 64, 12)
        hot = set(eng._hot_item.cpu().numpy().tolist())
        assert len(hot) == H and not hot & set(want['live_keys'][want['live_keys'] < 1100].tolist())


# ---- lists of long segments: T > 8 (2 N + U) -----------------------------------------------------------------------------------------------
LONG = dict(U=2000, N=100, B=4096, mean_deg=24)


def test_long_segments_on_the_sorted_road():
    """No transpose given: the list is sorted as any other (the span plan works in chunks of 64 and places its blocks — not read here)."""
    got, want, x = _check_sorted_road(LONG['U'], LONG['N'], LONG['B'], mean_deg=LONG['mean_deg'], crowd=True)
    assert x['T'] > 8 * (2 * LONG['N'] + LONG['U'])


def test_long_segments_through_the_transpose():
    """prepare_transposed (csrc/drx_prep.hpp) sorts only the batch's 2B (user | item, sample) pairs and expands the history's static
    item-major order.  What its kernels guarantee:
      k_tp_count / k_tp_write   the W part, compact from slot 0: every history entry, in ITEM-MAJOR order (items ascending, users
                                ascending inside an item: DrxHistory::t_users / t_items), writes key = its item once per sample of its
                                user that keeps the entry, in the order of the sorted batch pairs: samples ascending inside the user;
      k_tp_tail                 behind the Tw touches of the W part: the W2T part (N + item, the sorted item pairs: samples ascending inside
                                an item), then the V part (2N + user, likewise); plan.cnt[20] = Tw + 2B says where the list ends, and
                                DRX_KEY_NONE follows for at least a long chunk of 64 slots (or up to T) — slots further behind are
                                never written, and nobody reads them.
    So: the key sequence is the sorted road's; inside a W segment the touches come user by user, samples ascending inside a user
    (prep_oracle.prepared_transposed); the marks and blanked keys follow from the keys alone and are the sorted road's.
    That the road was taken (and did not answer kTpFallback, after which prepare_impl sorts): the two roads' sample orders differ for
    this batch (asserted below), so a buffer equal to the transposed statement was not sorted.  The shape is chosen so that the road's
    work areas fit into the big sort's scratch: 13-bit keys give that sort two passes, hence ping-pong buffers of 8 T bytes; T = 70 000
    slots -> about 618 KB against 494 KB of work areas (U = 200, N = 40 has 9-bit keys, a one-pass sort without those buffers: 58 KB
    against 182 KB — it falls back)."""
    U, N, B = LONG['U'], LONG['N'], LONG['B']
    got, unsorted, x = _prepare(U, N, B, mean_deg=LONG['mean_deg'], transpose=True, crowd=True)
    assert x['T'] > 8 * (2 * N + U)
    assert np.bincount(x['uid']).max() > 64               # (a user whose samples exceed the 64 keep bits the count pass hands on)
    want = po.prepared_transposed(unsorted['keys'], unsorted['vals'], x['uid'], N, B, x['keep_off'], x['ld'])
    sorted_want = po.prepared(unsorted['keys'], unsorted['vals'], N, B, x['keep_off'], x['ld'])
    assert not np.array_equal(want['vals'], sorted_want['vals'])
    nv = want['n_valid']
    # the live keys (blanked ones included) and where the list ends
    po._first_diff(got['keys'][:nv], want['keys'][:nv], 'keys of the compact list')
    assert (got['keys'][nv:min(x['T'], nv + 64)] == NONE).all()
    # the multiset of samples of every key
    by_key = lambda v: v[np.lexsort((v, want['live_keys']))]
    po._first_diff(by_key(got['vals'][:nv]), by_key(want['vals']), 'samples per key (sorted inside a key)')
    # inside a segment: user by user, samples ascending inside a user; W2T / V rows: samples ascending
    po._first_diff(got['vals'][:nv], want['vals'], 'samples in the road\'s order')
    # marks, order
    po.check_prepared(got['keys'], got['vals'], got['solo_v'], got['solo_o'], got['order'], want, behind=64)
    assert 0 < want['solo_v'].sum() < B                   # (users drawn once and users drawn often are both in the batch)
