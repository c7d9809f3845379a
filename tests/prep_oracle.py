"""NumPy statement of the two integer products every sparse step stands on, and the comparison functions the GPU tests call:

  the stable radix sort (csrc/drx_sort.hip)      sort_plan, sorted_pairs, check_sorted
  the unsorted touch list (csrc/drx_prep.hpp)    _wire, _expect (what k_sparse_touches_rounds writes, in batch order)
  the prepared touch list (prepare_impl)         prepared, prepared_transposed, check_prepared

Everything here is exact: integer keys, samples, bytes and permutations — nothing is compared under a tolerance.  No GPU, no torch,
no libdrx (tests/test_prep_oracle.py checks this file against plain Python `sorted` and feeds the comparison functions wrong outputs)."""
import numpy as np

from helpers import hash_u32, q_threshold

NONE = 0xFFFFFFFF                  # DRX_KEY_NONE
SORT_TILE = 8192                   # kSortThreads * kSortIPT: pairs of a tile of the sort
SORT_GRID = 512                    # workgroups of a pass at most: lists of more tiles make a workgroup take a second one


def sort_plan(bits):
    """(passes, digit bits) of a sort on `bits` key bits: the fewest launches with equal digits of 8, 10 or 11 bits."""
    if not 1 <= bits <= 32:
        raise ValueError(bits)
    for hi, plan in ((8, (1, 8)), (10, (1, 10)), (11, (1, 11)), (16, (2, 8)), (20, (2, 10)), (22, (2, 11)), (24, (3, 8)), (30, (3, 10)),
                     (32, (3, 11))):
        if bits <= hi:
            return plan


def sort_temp_bytes(n, bits):
    """drx_sort_pairs_temp_bytes restated (sort_layout: allocations on 256-byte borders): the ping-pong buffers of a plan of two or
    more passes, four histograms of 2048 words, 64 ticket words, a word per (pass, tile, digit value)."""
    up = lambda x: (x + 255) // 256 * 256
    passes, digit = sort_plan(bits)
    n = max(int(n), 1)
    tiles = (n + SORT_TILE - 1) // SORT_TILE
    off = 0
    if passes >= 2:
        off = up(up(4 * n) + 4 * n)
    off = up(off) + 4 * 4 * 2048
    off = up(off) + 4 * 64
    off = up(off) + 4 * passes * (tiles << digit)
    return up(off) + 512


def _first_diff(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        raise AssertionError(f'{what}: {got.shape[0] if got.ndim else got.shape} entries, expected {want.shape[0] if want.ndim else want.shape}')
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f'{what}: first difference at position {i}: got {int(got[i])} (0x{int(got[i]):X}), expected {int(want[i])} '
                             f'(0x{int(want[i]):X}); {bad.size} positions differ')


# ---- the sort ----------------------------------------------------------------------------------------------------------------------
def sorted_pairs(keys, vals, bits, drop_none):
    """What the sort must leave: the pairs in a STABLE order on the key.  The device orders on the low passes * digit bits of the
    key; for every key a test may use — below 2^bits, or DRX_KEY_NONE on the plain path (all ones: the largest under any mask) — that is
    the order on the whole key, and keys for which it is not are refused here (ValueError) rather than sorted some third way.
    drop_none: pairs whose key is DRX_KEY_NONE take no part; keys = the sorted others, then DRX_KEY_NONE up to n; vals = the sorted
    others' only (n_valid entries: the device does not write behind them)."""
    keys = np.asarray(keys, dtype=np.uint32)
    vals = np.asarray(vals, dtype=np.uint32)
    assert keys.shape == vals.shape and keys.ndim == 1
    passes, digit = sort_plan(bits)
    mask = np.uint32((1 << min(passes * digit, 32)) - 1)
    live = keys != NONE if drop_none else np.ones(keys.size, dtype=bool)
    k, v = keys[live], vals[live]
    order = np.argsort(k & mask, kind='stable')
    if not np.array_equal(order, np.argsort(k, kind='stable')):
        raise ValueError(f'keys that the low {passes * digit} bits order differently from the whole key: not a case of a {bits}-bit sort')
    n_valid = int(k.size)
    out_k = np.full(keys.size, NONE, dtype=np.uint32)
    out_k[:n_valid] = k[order]
    return dict(keys=out_k, vals=v[order], n_valid=n_valid, n=int(keys.size))


def check_sorted(got_keys, got_vals, want, sentinel=None):
    """Device output against sorted_pairs(): keys and vals equal up to n_valid, DRX_KEY_NONE keys behind, and — sentinel given: what
    vals_out was filled with before the call — vals behind n_valid still holding it.  AssertionError names the first differing position."""
    got_keys = np.asarray(got_keys).view(np.uint32) if np.asarray(got_keys).dtype == np.int32 else np.asarray(got_keys, dtype=np.uint32)
    got_vals = np.asarray(got_vals).view(np.uint32) if np.asarray(got_vals).dtype == np.int32 else np.asarray(got_vals, dtype=np.uint32)
    n, nv = want['n'], want['n_valid']
    if got_keys.shape != (n,) or got_vals.shape != (n,):
        raise AssertionError(f'outputs of {got_keys.shape} / {got_vals.shape} entries, expected {n}')
    _first_diff(got_keys[:nv], want['keys'][:nv], 'sorted keys')
    _first_diff(got_vals[:nv], want['vals'][:nv], 'sorted vals')
    pad = np.flatnonzero(got_keys[nv:] != NONE)
    if pad.size:
        i = nv + int(pad[0])
        raise AssertionError(f'padding keys: position {i} behind n_valid = {nv} holds 0x{int(got_keys[i]):X}, not DRX_KEY_NONE')
    if sentinel is not None:
        wr = np.flatnonzero(got_vals[nv:] != np.uint32(sentinel))
        if wr.size:
            i = nv + int(wr[0])
            raise AssertionError(f'padding vals: position {i} behind n_valid = {nv} was written ({int(got_vals[i])})')


# ---- the unsorted list (tests/test_gpu_prep_counts.py compares it with the touch kernel's output) ---------------------------------------
def _wire(item, is_out, ipr, cshift, world):
    o = item // ipr
    l = 2 * (item - o * ipr) + is_out
    return (((l >> cshift) * world + o) << cshift) | (l & ((1 << cshift) - 1))


def _expect(indptr, indices, N, uid, iid, seed, q, keep, slot_of, H, slack):
    B = len(uid)
    deg = (indptr[uid + 1] - indptr[uid]).astype(np.int64)
    keep_off = np.concatenate([[0], np.cumsum(deg)])
    tot = int(keep_off[-1])
    T = tot + slack + 2 * B
    row = np.repeat(np.arange(B), deg)
    j = np.arange(tot) - keep_off[row]
    items = indices[indptr[uid][row] + j].astype(np.int64)
    kf = (keep[:tot] != 0) if keep is not None else (hash_u32(seed, row, j) >= q_threshold(q))
    slot = slot_of[items] if H else np.full(tot, -1)
    listed = kf & (slot < 0)
    keys = np.full(T, NONE, dtype=np.uint32)
    vals = np.zeros(T, dtype=np.uint32)
    pos = keep_off[row] + 2 * row + j
    keys[pos] = np.where(listed, items, NONE)
    vals[pos] = row
    b = np.arange(B)
    at = keep_off[:-1] + 2 * b + deg
    keys[at], vals[at] = N + iid, b
    keys[at + 1], vals[at + 1] = 2 * N + uid, b
    Bw = (B + 31) // 32
    mask = np.zeros((max(H, 1), Bw), dtype=np.uint32)
    hot = kf & (slot >= 0)
    np.bitwise_or.at(mask, (slot[hot], row[hot] // 32), (np.uint32(1) << (row[hot] % 32).astype(np.uint32)))
    buckets = np.bincount(255 - np.minimum(deg >> 2, 255), minlength=256)
    return dict(T=T, keys=keys, vals=vals, mask=mask[:H], buckets=buckets, kept_items=items[kf], deg=deg)


# ---- the prepared list -------------------------------------------------------------------------------------------------------------------
def _finish(k, v, T, n_items, B, keep_off, ld):
    """Marks, blanked keys and degree buckets of the live pairs (k, v) in their final order."""
    k, v = np.asarray(k, dtype=np.uint32), np.asarray(v, dtype=np.uint32)
    n_valid = int(k.size)
    first = np.ones(n_valid, dtype=bool)
    last = np.ones(n_valid, dtype=bool)
    first[1:] = k[1:] != k[:-1]
    last[:-1] = k[:-1] != k[1:]
    alone = first & last
    solo_v, solo_o = np.zeros(B, dtype=np.uint8), np.zeros(B, dtype=np.uint8)
    blank = np.zeros(n_valid, dtype=bool)
    if ld > 16:                    # rows of <= 16 floats: no marks (the forward kernel's read-modify-write costs more than it saves)
        out = alone & (k >= n_items) & (k < 2 * n_items)
        usr = alone & (k >= 2 * n_items)
        solo_o[v[out]] = 1
        solo_v[v[usr]] = 1
        blank = out | usr
    keys = np.full(T, NONE, dtype=np.uint32)
    keys[:n_valid] = np.where(blank, np.uint32(NONE), k)
    keep_off = np.asarray(keep_off, dtype=np.int64)
    bucket = 255 - np.minimum((keep_off[1:] - keep_off[:-1]) >> 2, 255)
    assert bucket.shape == (B,)
    return dict(keys=keys, vals=v, n_valid=n_valid, n=int(T), live_keys=k, blank=blank, solo_v=solo_v, solo_o=solo_o, bucket=bucket)


def prepared(keys, vals, n_items, B, keep_off, ld):
    """What a preparation must leave, from the unsorted list (_expect's keys / vals: DRX_KEY_NONE for dropped, hot and padding slots):
      keys / vals   the live pairs in stable key order (the touches of a row in sample order), DRX_KEY_NONE keys behind n_valid;
      solo_o[b]     1 where sample b's key in [N, 2N) — its W2T row — has a run of length 1; solo_v[b]: the same for its key >= 2N;
      keys of those positions blanked to DRX_KEY_NONE, their vals kept (blank: which; live_keys: the keys before blanking);
      nothing marked or blanked when ld <= 16;
      bucket[b]     255 - min((keep_off[b + 1] - keep_off[b]) >> 2, 255): the launch order's degree bucket of sample b."""
    sp = sorted_pairs(keys, vals, 32, True)
    return _finish(sp['keys'][:sp['n_valid']], sp['vals'], len(keys), n_items, B, keep_off, ld)


def prepared_transposed(keys, vals, uid, n_items, B, keep_off, ld):
    """The same list as the preparation through the history's transpose lays it down: the same key sequence, but inside a W row's
    segment (key < N) the touches come user by user (users ascending: the transpose's order), samples ascending inside a user; W2T and V
    rows: samples ascending, as sorted."""
    keys, vals = np.asarray(keys, dtype=np.uint32), np.asarray(vals, dtype=np.uint32)
    live = keys != NONE
    k, v = keys[live], vals[live]
    user = np.where(k < n_items, np.asarray(uid, dtype=np.int64)[v], 0)
    order = np.lexsort((v, user, k))
    return _finish(k[order], v[order], len(keys), n_items, B, keep_off, ld)


def check_order(got_order, bucket):
    """order must be a permutation of 0 .. B-1 whose degree buckets never decrease (equal bucket populations follow)."""
    got_order = np.asarray(got_order)
    B = int(bucket.shape[0])
    if got_order.shape != (B,):
        raise AssertionError(f'order: {got_order.shape} entries, expected {B}')
    out = np.flatnonzero((got_order < 0) | (got_order >= B))
    if out.size:
        raise AssertionError(f'order: position {int(out[0])} holds {int(got_order[out[0]])}, no sample of 0 .. {B - 1}')
    times = np.bincount(got_order, minlength=B)
    if (times != 1).any():
        twice, never = np.flatnonzero(times > 1), np.flatnonzero(times == 0)
        at = int(np.flatnonzero(got_order == twice[0])[1])
        raise AssertionError(f'order: no permutation: sample {int(twice[0])} again at position {at}, sample {int(never[0])} missing')
    seq = bucket[got_order]
    down = np.flatnonzero(seq[1:] < seq[:-1])
    if down.size:
        i = int(down[0]) + 1
        raise AssertionError(f'order: position {i} (sample {int(got_order[i])}, bucket {int(seq[i])}) follows bucket {int(seq[i - 1])}')


def check_prepared(got_keys, got_vals, got_solo_v, got_solo_o, got_order, want, behind=None):
    """Device copies of a prepared list (drx_debug_prep_result) against prepared() / prepared_transposed(): keys — blanked ones
    included — and vals equal up to n_valid, DRX_KEY_NONE keys behind (behind: how many slots behind n_valid the road writes; None: all),
    the marks equal byte for byte, order a permutation grouped by ascending degree bucket."""
    got_keys = np.asarray(got_keys).view(np.uint32) if np.asarray(got_keys).dtype == np.int32 else np.asarray(got_keys, dtype=np.uint32)
    got_vals = np.asarray(got_vals).view(np.uint32) if np.asarray(got_vals).dtype == np.int32 else np.asarray(got_vals, dtype=np.uint32)
    n, nv = want['n'], want['n_valid']
    end = n if behind is None else min(n, nv + behind)
    if got_keys.shape != (n,) or got_vals.shape != (n,):
        raise AssertionError(f'lists of {got_keys.shape} / {got_vals.shape} slots, expected {n}')
    check_sorted(got_keys[:end], got_vals[:end], dict(keys=want['keys'][:end], vals=want['vals'], n_valid=nv, n=end))
    _first_diff(np.asarray(got_solo_o, dtype=np.uint8), want['solo_o'], 'solo_o (sole toucher of its W2T row)')
    _first_diff(np.asarray(got_solo_v, dtype=np.uint8), want['solo_v'], 'solo_v (sole toucher of its V row)')
    check_order(got_order, want['bucket'])
