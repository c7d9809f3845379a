"""tests/seg_oracle.py on hand-written key lists (CPU): the structure statements against values worked out by hand from
csrc/drx_segreduce.hpp, and the designed lists against the cases they are designed for."""
import numpy as np
import pytest

import prep_oracle as po
import seg_oracle as so
from seg_oracle import NONE


def _keys(*runs, pad=0):
    """runs of (key, length) -> the sorted list, `pad` DRX_KEY_NONE slots behind"""
    k = np.concatenate([np.full(n, key, dtype=np.uint32) for key, n in runs])
    assert (np.diff(k.astype(np.int64)) >= 0).all()
    return np.concatenate([k, np.full(pad, NONE, dtype=np.uint32)])


def test_span_shape_by_hand():
    # cpb = 4, first chunk 5: the span's partials begin at chunk 6, two chunks before the boundary at 8
    assert so.span_shape(5, 1, 0, 4) == (1, 0, 0)
    assert so.span_shape(5, 2, 1, 4) == (2, 0, 1)
    assert so.span_shape(5, 6, 0, 4) == (2, 1, 0)
    assert so.span_shape(5, 13, 1, 4) == (2, 2, 4)
    # first chunk 3: the partials begin on a boundary
    assert so.span_shape(3, 3, 0, 4) == (0, 0, 3)
    assert so.span_shape(3, 4, 0, 4) == (0, 1, 0)
    assert so.span_shape(3, 9, 1, 4) == (0, 2, 2)


def test_span_structure_by_hand():
    """chunks of 4, workgroups of 2 chunks:
       pos   0 1 2 3 | 4 5 6 7 | 8 9 10 11 | 12 13 14 15 | 16 17 18 19 | 20 21 22 23 | 24 25 26 27 | 28 ..
       key   1 1 1 2 | 2 3 3 3 | 3 3  3  3 |  3  3  3  3 |  3  4  5  5 |  5  5  5  5 |  6  7  7  7 |  7 N N N
    key 2 starts at chunk 0's last slot and ends in chunk 1: ext[0] = 1.  Key 3 starts in chunk 1, fills chunks 2 and 3 and ends one touch
    into chunk 4: a span (1, 2, 1); chunks 2 and 3 are inner and are workgroup 1: all-inner.  Key 5 starts in chunk 4 and ends exactly
    with chunk 5: a span (4, 1, 0); chunk 5 is inner, workgroup 2 (chunks 4, 5) is not all-inner.  Key 7 ends in chunk 7: ext[6] = 1."""
    keys = _keys((1, 3), (2, 2), (3, 12), (4, 1), (5, 6), (6, 1), (7, 4), pad=3)
    st = so.span_structure(keys, 4, 2)
    assert st['n_chunks'] == 8
    assert st['ext'].tolist() == [1, 0, 0, 0, 0, 0, 1, 0]
    assert st['short'] == {(1, 2, 1), (4, 1, 0)} and st['long'] == set()
    assert st['shape'] == {(1, 2, 1): (0, 1, 1), (4, 1, 0): (1, 0, 0)}
    assert st['inner'].tolist() == [False, False, True, True, False, True, False, False]
    assert st['all_inner'].tolist() == [False, True, False, False]
    c = so.case_counts(keys, 4, 2)
    assert c['b_ext_1'] == 2 and c['b_last_slot_alone'] == 1 and c['c_blk_1'] == 1 and c['c_has_end_0'] == 1 and c['c_has_end_1'] == 1
    assert c['d_all_inner_next_to_end'] == 1 and c['d_two_all_inner_in_a_row'] == 0 and c['e_slack_behind'] == 3
    assert c['a_ends_on_border'] == 1 and c['a_starts_on_border'] == 1 and c['e_last_partial_chunk'] == 1 and c['e_last_crosses_to_end'] == 1


def test_span_structure_long_and_short_sides_of_the_limit():
    # chunks of 2, workgroups of 2 chunks, a run from the last slot of chunk 0: 16 partials is short, 17 long
    for n_partials, where in ((16, 'short'), (17, 'long')):
        # first = 1: one lead chunk, then whole workgroups: total = 1 + n_blk
        n_blk = n_partials - 1
        keys = _keys((1, 1), (2, 1 + 2 * (1 + 2 * n_blk)), (3, 3))
        st = so.span_structure(keys, 2, 2)
        d = (0, 1 + 2 * n_blk, 0)
        assert st[where] == {d} and st['short' if where == 'long' else 'long'] == set() and st['shape'][d] == (1, n_blk, 0)
        assert int(st['all_inner'].sum()) == n_blk


def test_blanked_keys_and_padding_take_no_part():
    keys = _keys((1, 5), pad=11)
    st = so.span_structure(keys, 4, 2)
    assert st['ext'].tolist() == [1, 0, 0, 0] and not st['short'] and not st['long'] and not st['inner'].any()


def test_plan_sets_unpacks_front_and_back():
    desc = np.zeros((6, 2), dtype=np.uint32)
    desc[0] = (3, 2 | (1 << 31))
    desc[1] = (9, 1)
    desc[5] = (20, 40 | (1 << 31))
    s, l = so.plan_sets(desc.ravel(), (2, 1), 6)
    assert s == {(3, 2, 1), (9, 1, 0)} and l == {(20, 40, 1)}


def test_unplanned_structure_by_hand():
    """chunks of 4: key 3 from position 5 to 16 — chunk 1 keeps its tail, chunks 2 and 3 are whole and go on (flag 2), chunk 4 starts with
    its end (flag 1); key 5 ends exactly with chunk 5, which is therefore no middle chunk but an end chunk (flag 1)."""
    keys = _keys((1, 3), (2, 2), (3, 12), (4, 1), (5, 6), (6, 1), (7, 4), pad=3)
    st = so.unplanned_structure(keys, 4)
    assert st['flag'].tolist() == [0, 1, 2, 2, 1, 1, 0, 1]
    assert st['short'] == {(0, 0, 1), (1, 2, 1), (4, 0, 1), (6, 0, 1)} and st['long'] == set()


def test_unplanned_design_holds_both_sides_of_the_short_span_limit():
    runs = so.design_unplanned()
    for n in (31, 32, 33, 1, 63, 64, 65):
        assert n in runs
    keys = so.keys_of_runs(runs, np.arange(len(runs)))
    st = so.unplanned_structure(keys)
    start, end, _ = so._runs(keys)
    crossing = {(m, e) for _, m, e in st['short'] | st['long']}
    # m following chunks, m = 62 .. 65: mids = m - 1 and an end chunk, whole or partial — two runs each
    following = sorted(m + e for _, m, e in st['short'] | st['long'] if m >= 60 and m < 100)
    assert following == [62, 62, 63, 63, 64, 64, 65, 65]
    assert {m + e for _, m, e in st['long']} == {65, 204} and max(m + e for _, m, e in st['short']) == 64
    assert (0, 1) in crossing                           # a tail and an end chunk with no middle
    assert ((end % 32 == 0) & (end - start < 32)).any() and ((start % 32 == 0) & (start > 0)).any()
    assert ((start % 32 == 31) & (end - start > 1)).any()
    whole = (start % 32 == 0) & (end - start == 32)
    assert whole.any()


@pytest.mark.parametrize('ld,long_list,hot', [(64, False, 0), (128, False, 0), (256, False, 0), (52, False, 0), (16, False, 0), (64, True, 0),
                                              (128, True, 0), (128, False, 64)])
def test_cdae_designs_hold_every_case(ld, long_list, hot):
    """the list prep_oracle states for a designed batch has the designed run lengths, the intended kind of segments (long / short) and
    every case; rows of 16 floats carry no marks, so nothing is blanked there"""
    d = so.cdae_design(ld, long_list, hot=hot)
    N, U, B, uid, iid = d['N'], d['U'], d['B'], d['uid'], d['iid']
    deg = d['indptr'][uid + 1] - d['indptr'][uid]
    keep_off = np.concatenate([[0], np.cumsum(deg)])
    slot_of = None
    if hot:
        slot_of = np.full(N, -1)
        slot_of[:hot] = np.arange(hot)
        assert (np.bincount(d['indices'], minlength=N)[:hot] == 2).all() and np.bincount(d['indices'], minlength=N)[hot:].max() == 1
    un = po._expect(d['indptr'], d['indices'], N, uid, iid, 0, 0.5, np.ones(max(int(deg.sum()), 1), np.uint8), slot_of, hot, 37)
    want = po.prepared(un['keys'], un['vals'], N, B, keep_off, ld)
    start, end, _ = so._runs(want['live_keys'])
    assert (end - start).tolist() == [n for r in d['runs'] for n in r]
    assert (un['T'] > 8 * (2 * N + U)) == long_list
    live = np.full(un['T'], NONE, dtype=np.uint32)
    live[:want['n_valid']] = want['live_keys']
    c = so.case_counts(live, d['chunk'], d['cpb'], N, U, want['blank'])
    missing = [k for k, v in c.items() if v == 0 and not (ld <= 16 and k.startswith('g_'))]
    assert not missing, missing
    assert c['f_border_keys'] == (5 if hot else 6)      # (item 0 is hot: its touches are not in the list)
