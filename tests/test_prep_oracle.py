"""tests/prep_oracle.py against plain Python — `sorted` with a key function, loops over runs — on small inputs, and its comparison
functions against deliberately wrong "device outputs": every slip the GPU tests (test_gpu_sort.py, test_gpu_prep_list.py) are there to
catch is injected into a correct output here and must be refused, with the position named.  CPU only: no kernel is mutated to see a
test fail (a wrong offset there is a store out of bounds)."""
import numpy as np
import pytest

import prep_oracle as po
from prep_oracle import NONE

SENT = 0xDEADBEEF


def _pairs(n, bits, seed, pad=0.0):
    rng = np.random.default_rng(seed)
    hi = (1 << bits) - 1
    keys = (rng.random(n) ** 6 * hi).astype(np.uint64).astype(np.uint32)
    if pad:
        keys[rng.random(n) < pad] = NONE
    return keys, np.arange(n, dtype=np.uint32)


# ---- the oracle says what plain Python says ------------------------------------------------------------------------------------------
def test_plan_table_covers_the_nine_plans():
    got = {b: po.sort_plan(b) for b in range(1, 33)}
    assert [got[b] for b in (1, 8, 9, 10, 11, 12, 16, 17, 20, 21, 22, 23, 24, 25, 30, 31, 32)] == \
        [(1, 8), (1, 8), (1, 10), (1, 10), (1, 11), (2, 8), (2, 8), (2, 10), (2, 10), (2, 11), (2, 11), (3, 8), (3, 8), (3, 10), (3, 10),
         (3, 11), (3, 11)]
    assert len(set(got.values())) == 9
    for b, (p, d) in got.items():
        assert p * d >= b and ((p - 1) * d < b or d == 8)          # enough bits, and no launch to spare
    assert {po.sort_plan(b) for b in (1, 8, 9, 11, 12, 16, 20, 22, 24, 30, 32)} == set(got.values())      # (test_gpu_sort.py's widths)


@pytest.mark.parametrize('bits', [1, 9, 11, 13, 24, 32])
@pytest.mark.parametrize('drop', [False, True])
def test_sorted_pairs_is_pythons_stable_sort(bits, drop):
    keys, vals = _pairs(700, bits, bits, pad=0.2)
    if bits == 32 and drop:
        keys[5] = 0xFFFFFFFE                                       # the largest real key of the drop path
    want = po.sorted_pairs(keys, vals, bits, drop)
    pairs = [(int(k), int(v)) for k, v in zip(keys, vals) if not (drop and k == NONE)]
    ref = sorted(pairs, key=lambda kv: kv[0])                      # (list.sort is stable)
    assert want['n_valid'] == len(ref) and want['n'] == 700
    assert want['keys'][:len(ref)].tolist() == [k for k, _ in ref]
    assert want['vals'].tolist() == [v for _, v in ref]
    assert (want['keys'][len(ref):] == NONE).all()
    if drop:
        assert 0 < want['n_valid'] < 700
    po.check_sorted(want['keys'], np.concatenate([want['vals'], np.full(700 - len(ref), SENT, np.uint32)]), want, SENT)


def test_sorted_pairs_refuses_keys_the_digits_would_order_differently():
    keys = np.array([5, 1 << 20, 3], dtype=np.uint32)              # 16 bits: the device orders on the low 16 only
    with pytest.raises(ValueError):
        po.sorted_pairs(keys, np.arange(3, dtype=np.uint32), 16, False)


def test_temp_bytes_restatement():
    # one pass: no ping-pong buffers; 4 x 2048 histogram words, 64 ticket words, tiles << digit tile words, + 512
    assert po.sort_temp_bytes(1, 8) == 32768 + 256 + 1024 + 512
    assert po.sort_temp_bytes(8193, 11) == 32768 + 256 + 2 * 8192 + 512
    assert po.sort_temp_bytes(8192, 24) == 2 * 32768 + 32768 + 256 + 3 * 1024 + 512
    assert po.sort_temp_bytes(0, 8) == po.sort_temp_bytes(1, 8)


def _toy_list(seed=3, ld=64, B=40, N=11, U=9):
    """A small unsorted list in the touch kernel's layout: histories with drops, one output row and one user row per sample."""
    rng = np.random.default_rng(seed)
    uid = rng.integers(0, U, size=B)
    uid[7] = U - 1 if (uid != U - 1).all() else uid[7]
    iid = rng.integers(0, N, size=B)
    deg = rng.integers(0, 9, size=B)
    deg[3] = 0
    keep_off = np.concatenate([[0], np.cumsum(deg)])
    keys, vals = [], []
    for b in range(B):
        for j in range(deg[b]):
            keys.append(int(rng.integers(0, N)) if rng.random() > 0.3 else NONE)
            vals.append(b)
        keys += [N + int(iid[b]), 2 * N + int(uid[b])]
        vals += [b, b]
    keys += [NONE] * 5
    vals += [0] * 5
    return dict(keys=np.array(keys, np.uint32), vals=np.array(vals, np.uint32), uid=uid, iid=iid, keep_off=keep_off, N=N, B=B, U=U, ld=ld)


def _python_prepared(L, ld, transposed=False):
    N, B = L['N'], L['B']
    pairs = [(int(k), int(v)) for k, v in zip(L['keys'], L['vals']) if k != NONE]
    if transposed:
        ref = sorted(pairs, key=lambda kv: (kv[0], int(L['uid'][kv[1]]) if kv[0] < N else 0, kv[1]))
    else:
        ref = sorted(pairs, key=lambda kv: kv[0])
    count = {}
    for k, _ in ref:
        count[k] = count.get(k, 0) + 1
    solo_v, solo_o, keys = [0] * B, [0] * B, []
    for k, v in ref:
        if ld > 16 and k >= N and count[k] == 1:
            (solo_o if k < 2 * N else solo_v)[v] = 1
            keys.append(NONE)
        else:
            keys.append(k)
    bucket = [255 - min((int(L['keep_off'][b + 1]) - int(L['keep_off'][b])) >> 2, 255) for b in range(B)]
    return keys, [v for _, v in ref], solo_v, solo_o, bucket


@pytest.mark.parametrize('ld', [16, 64])
@pytest.mark.parametrize('transposed', [False, True])
def test_prepared_is_the_python_restatement(ld, transposed):
    L = _toy_list(ld=ld)
    want = po.prepared_transposed(L['keys'], L['vals'], L['uid'], L['N'], L['B'], L['keep_off'], ld) if transposed else \
        po.prepared(L['keys'], L['vals'], L['N'], L['B'], L['keep_off'], ld)
    keys, vals, solo_v, solo_o, bucket = _python_prepared(L, ld, transposed)
    nv = len(keys)
    assert want['n_valid'] == nv and want['n'] == len(L['keys'])
    assert want['keys'][:nv].tolist() == keys and (want['keys'][nv:] == NONE).all()
    assert want['vals'].tolist() == vals
    assert want['solo_v'].tolist() == solo_v and want['solo_o'].tolist() == solo_o
    assert want['bucket'].tolist() == bucket
    if ld > 16:
        assert 0 < sum(solo_v) < L['B'] and 0 < sum(solo_o) < L['B']      # (both kinds of row occur: sole touchers and shared rows)
        assert int(want['blank'].sum()) == sum(solo_v) + sum(solo_o)
    else:
        assert sum(solo_v) == sum(solo_o) == 0 and not want['blank'].any()


def test_the_two_roads_differ_only_inside_w_segments():
    L = _toy_list()
    a = po.prepared(L['keys'], L['vals'], L['N'], L['B'], L['keep_off'], 64)
    b = po.prepared_transposed(L['keys'], L['vals'], L['uid'], L['N'], L['B'], L['keep_off'], 64)
    assert np.array_equal(a['keys'], b['keys']) and np.array_equal(a['solo_v'], b['solo_v']) and np.array_equal(a['solo_o'], b['solo_o'])
    assert not np.array_equal(a['vals'], b['vals'])
    w = a['live_keys'] >= L['N']
    assert np.array_equal(a['vals'][w], b['vals'][w])


# ---- the comparison functions refuse wrong outputs ---------------------------------------------------------------------------------------
def _sorted_case(n, bits, drop, pad):
    keys, vals = _pairs(n, bits, n + bits, pad=pad)
    want = po.sorted_pairs(keys, vals, bits, drop)
    got_k = want['keys'].copy()
    got_v = np.full(n, SENT, dtype=np.uint32)
    got_v[:want['n_valid']] = want['vals']
    po.check_sorted(got_k, got_v, want, SENT if drop else None)              # (the correct output passes)
    return want, got_k, got_v


def test_check_sorted_catches_two_vals_swapped_inside_a_run():
    want, k, v = _sorted_case(3000, 6, False, 0.0)
    i = int(np.flatnonzero(k[1:] == k[:-1])[40])                   # positions i, i + 1 hold the same key: only stability tells them apart
    v[[i, i + 1]] = v[[i + 1, i]]
    with pytest.raises(AssertionError, match=f'sorted vals: first difference at position {i}:'):
        po.check_sorted(k, v, want)


def test_check_sorted_catches_a_pair_moved_across_a_tile_border():
    t, n = po.SORT_TILE, 3 * po.SORT_TILE + 5
    keys = (n - 1 - np.arange(n)).astype(np.uint32)                # distinct keys: every slot has one rightful pair
    want = po.sorted_pairs(keys, np.arange(n, dtype=np.uint32), 20, False)
    k, v = want['keys'].copy(), want['vals'].copy()
    for a in (k, v):                                               # the pair at the last slot of tile 0 lands one slot into tile 1
        a[t - 1:t + 2] = a[[t, t + 1, t - 1]]
    with pytest.raises(AssertionError, match=f'first difference at position {t - 1}:'):
        po.check_sorted(k, v, want)


def test_check_sorted_catches_a_missing_padding_key():
    want, k, v = _sorted_case(5000, 12, True, 0.15)
    nv = want['n_valid']
    k[nv + 3] = SENT                                               # (what keys_out held before the call)
    with pytest.raises(AssertionError, match=f'padding keys: position {nv + 3} '):
        po.check_sorted(k, v, want, SENT)


def test_check_sorted_catches_a_val_written_behind_n_valid():
    want, k, v = _sorted_case(5000, 12, True, 0.15)
    nv = want['n_valid']
    v[nv] = 0
    with pytest.raises(AssertionError, match=f'padding vals: position {nv} '):
        po.check_sorted(k, v, want, SENT)
    po.check_sorted(k, v, want)                                    # (without a sentinel the vals behind n_valid are nobody's business)


def _prepared_case():
    L = _toy_list()
    want = po.prepared(L['keys'], L['vals'], L['N'], L['B'], L['keep_off'], 64)
    order = np.argsort(want['bucket'], kind='stable').astype(np.int32)
    got = dict(k=want['keys'].copy(), v=np.concatenate([want['vals'], np.zeros(want['n'] - want['n_valid'], np.uint32)]),
               sv=want['solo_v'].copy(), so=want['solo_o'].copy(), order=order)
    po.check_prepared(got['k'], got['v'], got['sv'], got['so'], got['order'], want)
    # any order inside a bucket will do
    rev = order[np.lexsort((-np.arange(L['B']), want['bucket'][order]))]
    po.check_prepared(got['k'], got['v'], got['sv'], got['so'], rev, want)
    return L, want, got


def test_check_prepared_catches_a_mark_for_a_key_with_two_touches():
    L, want, g = _prepared_case()
    k = want['live_keys']
    i = int(np.flatnonzero((k[1:] == k[:-1]) & (k[1:] >= 2 * L['N']))[0])          # a V row two samples touch
    b = int(want['vals'][i])
    assert g['sv'][b] == 0
    g['sv'][b] = 1
    with pytest.raises(AssertionError, match=rf'solo_v .*first difference at position {b}:'):
        po.check_prepared(g['k'], g['v'], g['sv'], g['so'], g['order'], want)


def test_check_prepared_catches_a_sole_toucher_left_unblanked():
    L, want, g = _prepared_case()
    i = int(np.flatnonzero(want['blank'])[2])
    g['k'][i] = want['live_keys'][i]                               # marked, but the reduction would still see the touch
    with pytest.raises(AssertionError, match=f'sorted keys: first difference at position {i}:'):
        po.check_prepared(g['k'], g['v'], g['sv'], g['so'], g['order'], want)


def test_check_prepared_catches_an_order_with_a_sample_twice():
    L, want, g = _prepared_case()
    lost, dup = int(g['order'][10]), int(g['order'][4])
    g['order'][10] = dup
    with pytest.raises(AssertionError, match=f'sample {dup} again at position 10, sample {lost} missing'):
        po.check_prepared(g['k'], g['v'], g['sv'], g['so'], g['order'], want)


def test_check_prepared_catches_two_buckets_interleaved():
    L, want, g = _prepared_case()
    seq = want['bucket'][g['order']]
    i = int(np.flatnonzero(seq[1:] != seq[:-1])[0]) + 1            # the first sample of the second bucket ...
    g['order'][[i - 1, i]] = g['order'][[i, i - 1]]                # ... changes places with the last of the first
    with pytest.raises(AssertionError, match=rf'order: position {i} \(sample \d+, bucket {int(seq[i - 1])}\) follows bucket {int(seq[i])}'):
        po.check_prepared(g['k'], g['v'], g['sv'], g['so'], g['order'], want)


def test_check_prepared_on_the_transposed_road_looks_only_as_far_as_that_road_writes():
    L = _toy_list()
    want = po.prepared_transposed(L['keys'], L['vals'], L['uid'], L['N'], L['B'], L['keep_off'], 64)
    nv, n = want['n_valid'], want['n']
    k = want['keys'].copy()
    v = np.concatenate([want['vals'], np.zeros(n - nv, np.uint32)])
    order = np.argsort(want['bucket'], kind='stable')
    k[nv + 2:] = 12345                                             # slots the road never wrote
    po.check_prepared(k, v, want['solo_v'], want['solo_o'], order, want, behind=2)
    with pytest.raises(AssertionError, match=f'padding keys: position {nv + 2} '):
        po.check_prepared(k, v, want['solo_v'], want['solo_o'], order, want, behind=3)
    sorted_want = po.prepared(L['keys'], L['vals'], L['N'], L['B'], L['keep_off'], 64)
    with pytest.raises(AssertionError, match='sorted vals: first difference'):      # the sorted road's order is not this road's
        po.check_prepared(k, v, want['solo_v'], want['solo_o'], order, sorted_want, behind=2)
