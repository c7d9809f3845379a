"""The stable radix sort (csrc/drx_sort.hip) compared EXACTLY with tests/prep_oracle.py, on its two paths — drx_sort_pairs, and the
drop-padding mode a preparation uses (drx_debug_sort_pairs_drop: DRX_KEY_NONE pairs left out, with the sort's own zeroing and with the
caller's) — where it can go wrong:

  plans       key widths 1, 8, 9, 11, 12, 16, 20, 22, 24, 30, 32 = all nine (passes, digit) plans:
              1-8 (1, 8) | 9-10 (1, 10) | 11 (1, 11) | 12-16 (2, 8) | 17-20 (2, 10) | 21-22 (2, 11) | 23-24 (3, 8) | 25-30 (3, 10) | 31-32 (3, 11)
              (asserted through drx_sort_pairs_temp_bytes, which differs for every plan at a given n);
  sizes       1, 63, 64, 65 (a wave's row), 8191, 8192, 8193 (a tile = 512 threads x 16 pairs), 16385, 73 729 (nine tiles + 1: the last
              tile's look-back reads a second group of eight predecessors), 4 202 497 (514 tiles for 512 workgroups: two of them take
              a second tile, with live LDS);
  keys        skewed (u^6: long runs of small keys), all equal (one bin holds a whole tile), n - 1 - i (every digit value, short runs),
              differing in the top digit only;
  padding     none, all (n_valid = 0), only element 0, only element n - 1, all but one, 15 % at random, and of 20 000 pairs exactly 8192 /
              8193 live (only the passes after the first see that tile edge);
  edges       0xFFFFFFFF as an ordinary largest key of the plain path, 0xFFFFFFFE as the largest real key of the drop path; the refusals.

Every call: temp filled with 0xA5 (a word the sort needs zero and nobody cleared shows as a wrong result), outputs filled with a
sentinel (the vals behind n_valid must still hold it), vals = the input positions (stability is visible)."""
import numpy as np
import pytest

import prep_oracle as po
from prep_oracle import NONE

pytestmark = pytest.mark.gpu

SENT = 0xDEADBEEF
PATHS = ['plain', 'drop-prezeroed0', 'drop-prezeroed1']
BITS = [1, 8, 9, 11, 12, 16, 20, 22, 24, 30, 32]
BIG = 513 * po.SORT_TILE + 1                          # 4 202 497


@pytest.mark.parametrize('n,bits', [(1, 1), (63, 9), (64, 10), (4096, 18), (4097, 18), (100_003, 25), (1_440_000, 25), (300_000, 27), (70_000, 32),
                                    (200_000, 12), (500_000, 16), (33_000, 8),      # narrow keys over many tiles: one- and two-pass plans
                                    # around the tile of 8192 pairs; the plans (1, 11), (2, 11), (3, 8)
                                    (8191, 18), (8192, 18), (8193, 18), (20_000, 11), (100_003, 22), (100_003, 24)])
def test_sort_pairs_is_a_stable_sort(n, bits):
    """drx_sort_pairs (the inverted-index builder of the sparse steps) against torch's stable sort: heavy duplicates (Zipf-like
    keys), padding keys 0xFFFFFFFF, sizes around tile and wave borders, only the low `bits` bits order the pairs."""
    import ctypes as C
    import torch
    from drecpy_amd import _lib
    L = _lib.lib()
    g = torch.Generator(device='cuda'); g.manual_seed(n + bits)
    hi = (1 << bits) - 1
    u = torch.rand(n, generator=g, device='cuda', dtype=torch.float64)
    keys64 = (u ** 6 * hi).to(torch.int64)                                 # skewed: many duplicates of small keys
    if bits == 25 or bits == 32:
        pad = torch.rand(n, generator=g, device='cuda') < 0.15
        keys64 = torch.where(pad, torch.full_like(keys64, 0xFFFFFFFF), keys64)
    keys64 = keys64 & 0xFFFFFFFF
    keys = (keys64 - ((keys64 >> 31) << 32)).to(torch.int32)               # uint32 bit pattern in an int32 tensor
    vals = torch.arange(n, device='cuda', dtype=torch.int32)
    ko, vo = torch.empty_like(keys), torch.empty_like(vals)
    need = L.drx_sort_pairs_temp_bytes(n, bits)
    tmp = torch.empty(need, dtype=torch.uint8, device='cuda')
    _lib.check(L.drx_sort_pairs(_lib.ptr(keys), _lib.ptr(ko), _lib.ptr(vals), _lib.ptr(vo), n, bits, _lib.ptr(tmp), need,
                                _lib.stream_ptr(torch.device('cuda'))), 'drx_sort_pairs')
    torch.cuda.synchronize()
    low = keys64 & hi                                                       # only the low `bits` bits order the pairs
    want = torch.sort(low, stable=True)
    assert torch.equal(vo.long(), want.indices)
    assert torch.equal(ko.long() & 0xFFFFFFFF, keys64[want.indices])


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _skew(n, bits, seed):
    rng = np.random.default_rng(seed)
    hi = (1 << bits) - (2 if bits == 32 else 1)       # (32 bits: 0xFFFFFFFF is the drop path's padding; see the edge tests)
    return np.minimum(rng.random(n) ** 6 * (hi + 1), hi).astype(np.uint64).astype(np.uint32)      # (1 bit: a ninth of the keys are 1)


def _pad(keys, pattern, seed=0):
    """keys with DRX_KEY_NONE where `pattern` says; returns (keys, n_valid)"""
    n = keys.size
    pad = np.zeros(n, dtype=bool)
    if pattern == 'all':
        pad[:] = True
    elif pattern == 'first':
        pad[0] = True
    elif pattern == 'last':
        pad[n - 1] = True
    elif pattern == 'allbutone':
        pad[:] = True
        pad[n // 3] = False
    elif pattern == 'random15':
        pad = np.random.default_rng(seed + 1).random(n) < 0.15
    elif isinstance(pattern, int):                    # exactly `pattern` live pairs, spread over the list
        pad[:] = True
        pad[np.random.default_rng(seed + 2).permutation(n)[:pattern]] = False
    else:
        assert pattern == 'none'
    out = keys.copy()
    out[pad] = NONE
    return out, int(n - pad.sum())


def _sort(keys, bits, path, plan=None):
    """One call on `path`, compared with the oracle; returns the oracle's statement."""
    import torch
    from drecpy_amd import _lib
    L = _lib.lib()
    dev = torch.device('cuda')
    n = int(keys.size)
    drop = path != 'plain'
    vals = np.arange(n, dtype=np.uint32)
    want = po.sorted_pairs(keys, vals, bits, drop)
    d_k = torch.as_tensor(keys.view(np.int32)).to(dev)
    d_v = torch.arange(n, dtype=torch.int32, device=dev)
    sent = int(np.array([SENT], np.uint32).view(np.int32)[0])
    ko = torch.full((n,), sent, dtype=torch.int32, device=dev)
    vo = torch.full((n,), sent, dtype=torch.int32, device=dev)
    need = int(L.drx_sort_pairs_temp_bytes(n, bits))
    assert need == po.sort_temp_bytes(n, bits)        # the plan the table states: its scratch differs from every other plan's
    if plan is not None:
        assert po.sort_plan(bits) == plan
    tmp = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    if drop:
        rc = L.drx_debug_sort_pairs_drop(_lib.ptr(d_k), _lib.ptr(ko), _lib.ptr(d_v), _lib.ptr(vo), n, bits, int(path[-1]), _lib.ptr(tmp), need,
                                         _lib.stream_ptr(dev))
    else:
        rc = L.drx_sort_pairs(_lib.ptr(d_k), _lib.ptr(ko), _lib.ptr(d_v), _lib.ptr(vo), n, bits, _lib.ptr(tmp), need, _lib.stream_ptr(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    po.check_sorted(ko.cpu().numpy(), vo.cpu().numpy(), want, SENT if drop else None)
    assert torch.equal(d_v, torch.arange(n, dtype=torch.int32, device=dev))      # (the inputs are inputs)
    return want


# ---- plans, sizes, key shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('bits', BITS, ids=lambda b: 'bits%d-plan%dx%d' % ((b,) + po.sort_plan(b)))
def test_every_plan_on_both_paths(bits, path):
    """73 729 pairs = nine tiles + one pair, skewed keys, 15 % padding on the drop path (bits = 1: keys 0 and 1, two bins hold it all)."""
    n = 9 * po.SORT_TILE + 1
    keys = _skew(n, bits, bits)
    if path != 'plain':
        keys, _ = _pad(keys, 'random15', bits)
    want = _sort(keys, bits, path)
    assert want['n_valid'] == (n if path == 'plain' else int((keys != NONE).sum()))


@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('bits', [11, 20], ids=['bits11-plan1x11', 'bits20-plan2x10'])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 8191, 8192, 8193, 16385, 73729])
def test_sizes_at_wave_and_tile_borders(n, bits, path):
    keys = _skew(n, bits, n)
    if path != 'plain' and n > 1:
        keys, _ = _pad(keys, 'random15', n)
    _sort(keys, bits, path)


@pytest.mark.parametrize('bits,path', [(24, 'plain'), (32, 'drop-prezeroed1'), (8, 'plain'), (8, 'drop-prezeroed0')],
                         ids=['bits24-plan3x8-plain', 'bits32-plan3x11-drop-prezeroed1', 'bits8-plan1x8-plain', 'bits8-plan1x8-drop-prezeroed0'])
def test_a_workgroup_takes_a_second_tile_n4202497(bits, path):
    """514 tiles for a grid of 512 workgroups: the ticket loop is re-entered with the previous tile's counters, next-digit histogram
    and tile count still in LDS — on a one-pass plan and on three-pass plans (every pass re-enters it)."""
    assert BIG == 4_202_497 and (BIG + po.SORT_TILE - 1) // po.SORT_TILE == po.SORT_GRID + 2      # 513 full tiles and one pair
    keys = _skew(BIG, bits, bits)
    if path != 'plain':
        keys, _ = _pad(keys, 'random15', bits)
    _sort(keys, bits, path)


def _shape(shape, n, bits):
    passes, digit = po.sort_plan(bits)
    if shape == 'equal':
        return np.full(n, 5 % (1 << bits), dtype=np.uint32)
    if shape == 'reversed':
        assert n <= 1 << bits
        return (n - 1 - np.arange(n)).astype(np.uint32)
    assert shape == 'topdigit'
    top = bits - (passes - 1) * digit                 # bits of the key inside the last pass's digit
    return (np.random.default_rng(n).integers(0, 1 << top, size=n).astype(np.uint32) << np.uint32((passes - 1) * digit))


@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('shape,n,bits', [('equal', 16385, 20), ('equal', 8192, 11), ('reversed', 73729, 20), ('reversed', 2048, 11),
                                          ('topdigit', 73729, 20), ('topdigit', 16385, 30), ('topdigit', 16385, 24)])
def test_key_shapes(shape, n, bits, path):
    """All keys equal: one bin holds a whole tile and every earlier pass is the identity; n - 1 - i: every digit value, runs of one
    (the input reversed); keys that differ in the top digit only: all passes but the last move nothing, the last one everything."""
    keys = _shape(shape, n, bits)
    if path != 'plain':
        keys, _ = _pad(keys, 'random15', n)
    _sort(keys, bits, path)


# ---- the drop path's padding -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pre_zeroed', [0, 1], ids=['prezeroed0', 'prezeroed1'])
@pytest.mark.parametrize('pattern,n_valid', [('none', 20000), ('all', 0), ('first', 19999), ('last', 19999), ('allbutone', 1), ('random15', None),
                                             (8192, 8192), (8193, 8193)],
                         ids=['none-nvalid20000', 'all-nvalid0', 'first-nvalid19999', 'last-nvalid19999', 'allbutone-nvalid1', 'random15',
                              'live-nvalid8192', 'live-nvalid8193'])
@pytest.mark.parametrize('bits', [16, 22], ids=['bits16-plan2x8', 'bits22-plan2x11'])
def test_drop_path_padding_patterns(bits, pattern, n_valid, pre_zeroed):
    """20 000 pairs (three tiles for the first pass).  keys_out = the oracle's up to n_valid and DRX_KEY_NONE behind; vals_out = the
    oracle's up to n_valid and the sentinel behind ("their vals are not written": drx_common.hpp).  n_valid = 8192 / 8193: the passes
    after the first — sized from the histogram's sum — have exactly one tile / one tile and one pair."""
    keys, nv = _pad(_skew(20000, bits, 7), pattern, 7)
    if n_valid is not None:
        assert nv == n_valid
    want = _sort(keys, bits, 'drop-prezeroed%d' % pre_zeroed)
    assert want['n_valid'] == nv


# ---- edge values -------------------------------------------------------------------------------------------------------------------------
def test_all_ones_is_an_ordinary_largest_key_of_the_plain_path():
    keys = np.random.default_rng(5).integers(0, 1 << 32, size=30000, dtype=np.uint64).astype(np.uint32)
    keys[[0, 77, 8191, 8192, 29999]] = 0xFFFFFFFF
    keys[[1, 8193]] = 0xFFFFFFFE
    want = _sort(keys, 32, 'plain', plan=(3, 11))
    assert want['n_valid'] == 30000 and want['keys'][-5:].tolist() == [0xFFFFFFFF] * 5 and want['vals'][-5:].tolist() == [0, 77, 8191, 8192, 29999]


@pytest.mark.parametrize('path', PATHS[1:])
def test_the_largest_real_key_of_the_drop_path(path):
    keys = np.random.default_rng(6).integers(0, 1 << 32, size=30000, dtype=np.uint64).astype(np.uint32)
    keys[keys == NONE] = 0
    keys[[3, 8191, 20000]] = 0xFFFFFFFE
    keys[[0, 77, 8192, 29999]] = NONE
    want = _sort(keys, 32, path, plan=(3, 11))
    nv = want['n_valid']
    assert nv == 29996 and want['keys'][nv - 3:nv].tolist() == [0xFFFFFFFE] * 3 and want['vals'][nv - 3:].tolist() == [3, 8191, 20000]


# ---- refusals: each returns before any launch -------------------------------------------------------------------------------------------
def _entry(path):
    from drecpy_amd import _lib
    L = _lib.lib()
    if path == 'plain':
        return lambda ki, ko, vi, vo, n, bits, tmp, nbytes, st: L.drx_sort_pairs(ki, ko, vi, vo, n, bits, tmp, nbytes, st)
    pz = int(path[-1])
    return lambda ki, ko, vi, vo, n, bits, tmp, nbytes, st: L.drx_debug_sort_pairs_drop(ki, ko, vi, vo, n, bits, pz, tmp, nbytes, st)


@pytest.mark.parametrize('path', PATHS)
def test_refusals(path):
    import torch
    from drecpy_amd import _lib
    L = _lib.lib()
    EINVAL, ESCRATCH = -1, -2
    dev = torch.device('cuda')
    call = _entry(path)
    n, bits = 1000, 20
    sent = int(np.array([SENT], np.uint32).view(np.int32)[0])
    ki = torch.arange(n, dtype=torch.int32, device=dev)
    vi = torch.arange(n, dtype=torch.int32, device=dev)
    ko = torch.full((n,), sent, dtype=torch.int32, device=dev)
    vo = torch.full((n,), sent, dtype=torch.int32, device=dev)
    need = int(L.drx_sort_pairs_temp_bytes(n, bits))
    tmp = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)
    p = _lib.ptr
    args = [p(ki), p(ko), p(vi), p(vo), n, bits, p(tmp), need, st]

    def with_(**kw):
        a = list(args)
        for k, v in kw.items():
            a[dict(ki=0, ko=1, vi=2, vo=3, n=4, bits=5, tmp=6, nbytes=7)[k]] = v
        return call(*a)

    assert with_(n=2 ** 30) == EINVAL                               # tile words carry 30-bit counts
    assert with_(nbytes=need - 1024) == ESCRATCH
    for name in ('ki', 'ko', 'vi', 'vo', 'tmp'):
        assert with_(**{name: None}) == EINVAL, name
    assert with_(bits=0) == EINVAL and with_(bits=33) == EINVAL
    assert with_(n=-1) == EINVAL
    assert L.drx_sort_pairs_temp_bytes(n, 0) == 0 and L.drx_sort_pairs_temp_bytes(n, 33) == 0 and L.drx_sort_pairs_temp_bytes(-1, 20) == 0
    assert with_(n=0) == 0                                          # nothing to sort: nothing is launched ...
    assert with_(n=0, ki=None, ko=None, vi=None, vo=None, tmp=None, nbytes=0) == 0
    torch.cuda.synchronize()
    for t in (ko, vo):                                              # ... and no refusal wrote anything
        assert bool((t == sent).all())
    assert bool((tmp == 0xA5).all())
