"""The DMF gather's work list for host-prepared batches (DmfEngine.host_work_list over drx_dmf_work_order) at its limits: which list
a batch gets — cut into segments, or uncut — and what the list holds.  Host code only: no GPU needed."""
import numpy as np
import pytest

import dmf_shapes as ds


def _case(name):
    """(off_u, off_i, B) of the batches the GPU tests of test_gpu_dmf.py run"""
    if name == 'blocks-4096':             # many ids of 138 segments, few distinct ids: more partial rows than _zpart has
        m, (u, i, _) = ds.blocks(), ds.blocks_batch(4096, 1)
    elif name == 'blocks-256':            # the same rows in a small batch: more entries than its list has
        m, (u, i, _) = ds.blocks(), ds.blocks_batch(256, 2)
    elif name == 'one-long-row':          # an id of 263 segments
        m, (u, i, _) = ds.one_long_row(), ds.one_long_row_batch(64, 3)
    elif name == 'wide':                  # segments in use next to every limit
        m, (u, i, _) = ds.wide(), ds.wide_batch(4)
    else:
        m, (u, i, _) = ds.plain(), ds.plain_batch(200, 5)
    return ds.batch_offsets(m, u, i) + [len(u)]


# (name, the list is cut, why not)
CASES = [('blocks-4096', False, 'parts'), ('blocks-256', False, 'entries'), ('one-long-row', False, 'segments'), ('wide', True, None),
         ('plain', True, None)]


@pytest.mark.parametrize('name,cut,why', CASES)
def test_a_host_batch_never_brings_more_partial_rows_than_the_buffer_holds(name, cut, why):
    """DmfEngine.host_work_list against the rules restated in NumPy (dmf_shapes.rules): the list is cut exactly when no id needs more
    than 255 segments, the entries fit 2 B + _ORDER_EXTRA AND the partial rows fit _zpart's _ORDER_EXTRA (+ 8) rows; n_work and n_part
    are the sums of the segment counts; an uncut list has one entry per id, seg_len 0 and no partial row.  Every case is one of the
    reasons, checked to be THAT reason — 'parts' is the batch that, judged by its entries alone (the rule before partial rows were
    counted), was handed to the gather with more partial rows than the buffer has."""
    from drecpy_amd.engine_dmf import DmfEngine
    assert DmfEngine._ORDER_EXTRA == ds.ORDER_EXTRA
    off_u, off_i, B = _case(name)
    want, by_entries_alone = ds.rules(off_u, off_i, B, ds.SEG)
    n_work, seg, n_part, order, zseg = DmfEngine.host_work_list(off_u, off_i, B, ds.SEG)
    assert (n_work, seg, n_part) == want[:3]
    assert n_part <= DmfEngine._ORDER_EXTRA and n_work <= 2 * B + DmfEngine._ORDER_EXTRA
    assert (seg == ds.SEG) == cut and (seg > 0 or n_part == 0)
    n = len(off_u) + len(off_i) - 2
    deg = np.concatenate([np.diff(off_u), np.diff(off_i)])
    ns = -(-deg // ds.SEG)
    if why == 'parts':
        assert ns.max() <= 255 and ns.sum() <= 2 * B + ds.ORDER_EXTRA
        assert by_entries_alone[1] == ds.SEG and by_entries_alone[2] > ds.ORDER_EXTRA + 8           # what overflowed _zpart
    elif why == 'entries':
        assert ns.max() <= 255 and ns.sum() > 2 * B + ds.ORDER_EXTRA
    elif why == 'segments':
        assert ns.max() > 255
    else:
        assert n_part > 0 and by_entries_alone[:3] == want[:3]
    if not cut:
        assert n_work == n and not zseg[:n].any()
        assert sorted((order[:n_work].view(np.uint32) & 0xFFFFFF).tolist()) == list(range(n)) and not (order[:n_work].view(np.uint32) >> 24).any()
    # the arrays a caller passes are the ones filled
    o2, z2 = np.full(2 * B + ds.ORDER_EXTRA, -1, np.int32), np.full(2 * B, -1, np.int32)
    r = DmfEngine.host_work_list(off_u, off_i, B, ds.SEG, o2, z2)
    assert r[:3] == (n_work, seg, n_part) and r[3] is o2 and r[4] is z2
    assert np.array_equal(o2[:n_work], order[:n_work]) and np.array_equal(z2[:n], zseg[:n])
    # seg_len 0 asks for the uncut list
    assert DmfEngine.host_work_list(off_u, off_i, B, 0)[:3] == (n, 0, 0)


@pytest.mark.parametrize('name', ['wide', 'plain'])
def test_the_cut_list_decodes_to_every_segment_once(name):
    """The list host_work_list returns, decoded as k_dmf_gather decodes it — in UNSIGNED arithmetic: work index = enc & 0xFFFFFF,
    segment = uint32(enc) >> 24, so that segment numbers >= 128, which set the sign bit of the int32 entry, stay positive ('wide' has
    an id of 138 segments).  Every id's segments are 0 .. ns - 1, consecutive in the list; the segment counts sum to n_work; the
    ranges of partial rows (zseg = first << 8 | count) are disjoint, of ns - 1 rows each, and fill 0 .. n_part - 1."""
    from drecpy_amd.engine_dmf import DmfEngine
    off_u, off_i, B = _case(name)
    n_work, seg, n_part, order, zseg = DmfEngine.host_work_list(off_u, off_i, B, ds.SEG)
    assert seg == ds.SEG
    n = len(off_u) + len(off_i) - 2
    enc = order[:n_work].view(np.uint32)
    ids, segs = (enc & 0xFFFFFF).astype(np.int64), (enc >> 24).astype(np.int64)
    deg = np.concatenate([np.diff(off_u), np.diff(off_i)]).astype(np.int64)
    ns = np.maximum(-(-deg // ds.SEG), 1)
    if name == 'wide':
        assert ns.max() >= 128 and segs.max() == ns.max() - 1 and (order[:n_work] < 0).any()
    assert ids.max() < n and ns.sum() == n_work
    first = np.flatnonzero(np.concatenate([[True], ids[1:] != ids[:-1]]))            # runs of one id
    assert len(first) == n and len(np.unique(ids[first])) == n                       # each id one run: its segments are adjacent
    run_len = np.diff(np.concatenate([first, [n_work]]))
    assert np.array_equal(run_len, ns[ids[first]])
    assert np.array_equal(segs, np.arange(n_work) - np.repeat(first, run_len))       # 0 .. ns - 1 inside a run
    z = zseg[:n].view(np.uint32)
    lo, cnt = (z >> 8).astype(np.int64), (z & 255).astype(np.int64)
    assert np.array_equal(cnt, ns - 1) and cnt.sum() == n_part
    taken = np.zeros(n_part, np.int64)
    for a in np.flatnonzero(cnt):
        taken[lo[a]:lo[a] + cnt[a]] += 1
    assert np.all(taken == 1)
    assert not z[cnt == 0].any()
