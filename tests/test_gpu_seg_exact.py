"""The segmented reduction over the sorted touch list, EXACTLY: integer-valued gradient rows through lists whose run lengths are designed
(tests/seg_oracle.py) so that every branch of the fold and of the span plan is taken on purpose.

Every partial sum of integers of this size is an exact float32 whatever the order of the additions, so the expected row sum is exact:
a touch that is lost, folded twice or credited to its neighbour changes a sum by at least 1, and — CDAE lists — the Adagrad accumulator
acc0 + g^2 (|g| <= 4096: g^2 exact, ONE rounding) is compared bit for bit.

  unplanned kernels (k_seg_reduce, k_span_short, k_span_long)     drx_scatter_rows on its sort path, np.array_equal
  planned and streamed forms (k_seg_reduce_planned, k_span_planned, k_seg_reduce_stream; k_plan_spans)
                                                                 drx_debug_cdae_reduce on designed CDAE batches, the plan a preparation
                                                                 left (drx_debug_span_plan) against seg_oracle.span_structure

The cases a designed CDAE list holds (seg_oracle.case_counts counts them; each test asserts that none is missing):
  (a) a segment ending exactly on a chunk border, and one starting there;
  (b) ext = 1 and ext = chunk - 1; two consecutive chunks both extended; an extended chunk whose crossing segment is its last slot alone;
  (c) spans of 16 and of 17 partials (short | long); n_lead = 0 and cpb - 1; n_blk = 0, 1, >= 2; n_trail = 0 and cpb; has_end 0 and 1;
  (d) all-inner workgroups: two in a row, and one next to the workgroup that holds the segment's end;
  (e) the first segment at position 0, the last crossing into a last partial chunk, DRX_KEY_NONE slack behind (one list: none);
  (f) keys N - 1, N, 2N - 1, 2N, 2N + U - 1 (and 0), a crossing segment in each array, a W2T span (b2's sum rides through it);
  (g) prepared lists of rows wider than 16 floats: blanked sole-toucher keys at a chunk's first and last slot and inside an ext window."""
import ctypes as C
import functools

import numpy as np
import pytest

import dense_update_oracle as du
import optim_oracle as oo
import prep_oracle as po
import seg_oracle as so
from seg_oracle import NONE
from test_gpu_optim_rules import _inside

pytestmark = pytest.mark.gpu

F = np.float32
MASK_BUDGET = 8 << 20                     # kMaskBudget (csrc/drx_generic.hip): above it drx_scatter_rows sorts


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


# ---- 1. the unplanned kernels through drx_scatter_rows --------------------------------------------------------------------------------
def _scatter(keys, ld, n_rows, indexed, seed):
    """drx_scatter_rows on integer data against int64 sums; returns nothing, asserts equality of every float"""
    import torch
    from drecpy_amd import _lib
    L = _lib.lib()
    T = int(keys.size)
    rng = np.random.default_rng(seed)
    n_src = max(T // 3, 1) if indexed else T
    src = rng.integers(-2, 3, size=(n_src, ld)).astype(np.int8)
    src_s = rng.integers(-2, 3, size=n_src).astype(np.int8)
    idx = rng.integers(0, n_src, size=T) if indexed else np.arange(T)
    coef = rng.integers(-2, 3, size=T).astype(np.int64) if indexed else np.ones(T, np.int64)
    live = keys != NONE
    order = np.flatnonzero(live)[np.argsort(keys[live], kind='stable')]
    want, want_s = np.full((n_rows, ld), 7.0), np.full(n_rows, 7.0)             # 7 = "kept what it held"
    if order.size:
        ks = keys[order].astype(np.int64)
        first = np.concatenate([[0], np.flatnonzero(ks[1:] != ks[:-1]) + 1])
        want[ks[first]] = np.add.reduceat(coef[order, None].astype(np.int32) * src[idx[order]].astype(np.int32), first, axis=0)
        want_s[ks[first]] = np.add.reduceat(coef[order] * src_s[idx[order]].astype(np.int64), first)
    assert np.abs(want).max() < 2 ** 24 and np.abs(want_s).max() < 2 ** 24
    dev = torch.device('cuda')
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    d_keys, d_src, d_ss = t(keys.view(np.int32)), t(src.astype(F)), t(src_s.astype(F))
    d_idx = t(idx.astype(np.int32)) if indexed else None
    d_coef = t(coef.astype(F)) if indexed else None
    out = torch.full((n_rows, ld), 7.0, dtype=torch.float32, device=dev)
    out_s = torch.full((n_rows,), 7.0, dtype=torch.float32, device=dev)
    need = L.drx_scatter_scratch_bytes(ld, T, n_rows)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    _lib.check(L.drx_scatter_rows(_lib.ptr(d_keys), T, _lib.ptr(d_src), _lib.ptr(d_idx), _lib.ptr(d_coef), _lib.ptr(d_ss), ld, n_rows,
                                  _lib.ptr(out), _lib.ptr(out_s), _lib.ptr(scratch), need, _lib.stream_ptr(dev)), 'drx_scatter_rows')
    torch.cuda.synchronize()
    got, got_s = out.cpu().numpy(), out_s.cpu().numpy()
    bad = np.argwhere(got != want.astype(F))
    assert bad.size == 0, f'{bad.shape[0]} elements differ, first: row {bad[0][0]} column {bad[0][1]}: got {got[tuple(bad[0])]}, ' \
                          f'expected {want[tuple(bad[0])]}'
    assert np.array_equal(got_s, want_s.astype(F))
    named = np.zeros(n_rows, dtype=bool)
    named[keys[live].astype(np.int64)] = True
    assert (_bits(got[~named]) == _bits(F(7.0))).all() and (_bits(got_s[~named]) == _bits(F(7.0))).all()


def _sorts(T, n_rows):
    return n_rows * ((T + 31) // 32) * 4 > MASK_BUDGET


@functools.lru_cache(maxsize=None)
def _unplanned_list(pad):
    """(shuffled keys with `pad` padding keys among them, n_rows): design_unplanned's runs over row ids spread over [0, n_rows)"""
    runs = so.design_unplanned()
    T = sum(runs) + pad
    n_rows = MASK_BUDGET // (4 * ((T + 31) // 32)) + 64
    ids = so.spread_ids(len(runs), n_rows)
    sorted_keys = np.concatenate([so.keys_of_runs(runs, ids), np.full(pad, NONE, dtype=np.uint32)])
    st = so.unplanned_structure(sorted_keys)
    m = sorted(mm + e for _, mm, e in st['short'] | st['long'])
    assert [x for x in m if 60 <= x < 100] == [62, 62, 63, 63, 64, 64, 65, 65]
    assert {mm + e for _, mm, e in st['long']} == {65, 204} and max(mm + e for _, mm, e in st['short']) == 64
    keys = sorted_keys[np.random.default_rng(3).permutation(T)]          # (the library sorts them; padding scattered)
    return keys, n_rows


@pytest.mark.parametrize('indexed', [False, True], ids=['plain', 'indexed'])
@pytest.mark.parametrize('ld', [4, 32, 64, 128, 256, 300, 1024])
def test_scatter_rows_designed_runs_exact(ld, indexed):
    """one width per geometry of pick_geom (300: J = 2; DRX_MAX_K = 1024: J = 4); T no multiple of 32, padding keys scattered"""
    keys, n_rows = _unplanned_list(pad=45)
    assert keys.size % 32 != 0 and _sorts(keys.size, n_rows)
    _scatter(keys, ld, n_rows, indexed, seed=ld)


@pytest.mark.parametrize('indexed', [False, True], ids=['plain', 'indexed'])
def test_scatter_rows_last_run_reaches_the_end_of_a_whole_number_of_chunks(indexed):
    """no padding, T a multiple of 32, the last run crossing into the last chunk and reaching T exactly"""
    runs = so.design_unplanned(tail_pad=0)
    runs.append(32 + 32 - sum(runs) % 32)
    T = sum(runs)
    n_rows = MASK_BUDGET // (4 * (T // 32)) + 64
    keys = so.keys_of_runs(runs, so.spread_ids(len(runs), n_rows))
    assert T % 32 == 0 and _sorts(T, n_rows) and keys[-1] == n_rows - 1 and keys[0] == 0
    _scatter(keys[np.random.default_rng(4).permutation(T)], 64, n_rows, indexed, seed=11)


@pytest.mark.parametrize('case', ['one-touch', 'one-key', 'padding-at-the-end'])
def test_scatter_rows_degenerate_lists_exact(case):
    T, ld = 4096 + 5, 64
    n_rows = MASK_BUDGET // (4 * ((T + 31) // 32)) + 64
    assert _sorts(T, n_rows)
    if case == 'one-touch':                             # all padding but one touch
        keys = np.full(T, NONE, dtype=np.uint32)
        keys[1234] = n_rows - 1
    elif case == 'one-key':                             # one segment over 129 chunks: k_span_long
        keys = np.full(T, 17, dtype=np.uint32)
    else:                                               # sorted input, a block of padding behind it
        keys = np.sort(np.random.default_rng(8).integers(0, 50, size=T).astype(np.uint32))
        keys[-700:] = NONE
    _scatter(keys, ld, n_rows, True, seed=21)


def test_scatter_rows_single_touch():
    """T = 1 (the bit-mask path: no list of this size sorts)"""
    assert not _sorts(1, 30000)
    _scatter(np.array([29999], dtype=np.uint32), 64, 30000, False, seed=1)


# ---- 2. the planned and the streamed form on designed CDAE lists ----------------------------------------------------------------------
LR, ACC0 = 0.05, 0.1
_cache = {}


def _engine(K, d, opt, hot):
    from drecpy_amd.engine import CdaeEngine
    eng = CdaeEngine(d['U'], d['N'], K)
    eng.share_users = False
    eng.set_history(d['indptr'], d['indices'], with_transpose=False)
    eng.init_glorot(7)
    eng.init_optimizer(opt, LR, 0.0)                    # reg_rate 0: a row's own value adds nothing to its gradient
    eng.set_hot_rows(hot, min_batch=0)
    return eng


def _case(K, long_list, opt='adagrad', hot=0, slack=37):
    """A designed batch, its engine, the list prep_oracle expects and the integer gradient rows — made once per shape."""
    key = (K, long_list, opt, hot, slack)
    if key in _cache:
        return _cache[key]
    import torch
    ld = (K + 3) // 4 * 4
    d = so.cdae_design(ld, long_list, hot=hot)
    eng = _engine(K, d, opt, hot)
    assert eng.ld == ld
    N, U, B, uid, iid = d['N'], d['U'], d['B'], d['uid'], d['iid']
    deg = d['indptr'][uid + 1] - d['indptr'][uid]
    keep_off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    keep = np.ones(max(int(deg.sum()), 1), dtype=np.uint8)
    bt, alive = eng.make_batch(uid.astype(np.int32), iid.astype(np.int32), np.zeros(B, F), keep_off=keep_off, keep=keep, q=0.5,
                               mask_seed=0, n_touch_slots=int(deg.sum()) + slack)
    slot_of = None
    if hot:
        slot_of = eng._hot_slot.cpu().numpy().astype(np.int64)
        assert sorted(eng._hot_item.cpu().numpy().tolist()) == list(range(hot))
    un = po._expect(d['indptr'], d['indices'], N, uid, iid, 0, 0.5, keep, slot_of, hot, slack)
    want = po.prepared(un['keys'], un['vals'], N, B, keep_off, ld)
    T = un['T']
    assert (T > 8 * (2 * N + U)) == long_list
    live = np.full(T, NONE, dtype=np.uint32)
    live[:want['n_valid']] = want['live_keys']
    counts = so.case_counts(live, d['chunk'], d['cpb'], N, U, want['blank'])
    missing = [k for k, v in counts.items() if v == 0 and not (ld <= 16 and k.startswith('g_')) and not (slack == 0 and k == 'e_slack_behind')]
    assert not missing, missing
    print(f'[cases] K={K} ld={ld} chunk={d["chunk"]} cpb={d["cpb"]} {"long" if long_list else "short"} hot={hot} T={T}: '
          + ' '.join(f'{k}={v}' for k, v in counts.items()))
    rng = np.random.default_rng(100 + K)
    grads = dict(dz1=rng.integers(-1, 2, size=(B, ld)).astype(F), g2=rng.integers(-1, 2, size=(B, ld)).astype(F),
                 dz2=rng.integers(-1, 2, size=B).astype(F))
    dev = {k: torch.as_tensor(v).to(eng.device) for k, v in grads.items()}
    state0 = [t.clone() for t in eng.tables()], [t.clone() for t in eng.s1], [t.clone() for t in eng.s2] if eng.s2 is not None else None
    c = dict(d=d, eng=eng, bt=bt, alive=alive, want=want, live=live, T=T, ld=ld, grads=grads, dev=dev, state0=state0, uid=uid, hot=hot,
             structure=so.span_structure(live, d['chunk'], d['cpb']), prepared=None, n_touch_slots=int(deg.sum()) + slack, counts=counts)
    _cache[key] = c
    return c


def _prepared(c):
    """the list prepared ahead (once per case), compared with prep_oracle's statement; its plan compared with span_structure"""
    import torch
    from drecpy_amd import _lib
    if c['prepared'] is not None:
        return c['prepared']
    L, eng, bt, B, T = _lib.lib(), c['eng'], c['bt'], c['d']['B'], c['T']
    prep = eng.prepare_sparse(bt, hot=c['hot'] > 0)
    assert int(prep._drx_hot) == c['hot']
    dev = eng.device
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)
    keys_o, vals_o, sv, so_, order = i32(T), i32(T), u8(B), u8(B), i32(B)
    P = C.byref(eng._params)
    assert L.drx_debug_prep_result(P, B, bt.n_touch_slots, c['hot'], _lib.ptr(prep), prep.numel(), _lib.ptr(keys_o), _lib.ptr(vals_o),
                                   _lib.ptr(sv), _lib.ptr(so_), _lib.ptr(order), _lib.stream_ptr(dev)) == 0
    st = c['structure']
    nc = st['n_chunks']
    ext_o, desc_o, cnt_o = u8(nc), i32(2 * nc), i32(2)
    assert L.drx_debug_span_plan(P, B, bt.n_touch_slots, c['hot'], _lib.ptr(prep), prep.numel(), _lib.ptr(ext_o), _lib.ptr(desc_o),
                                 _lib.ptr(cnt_o), _lib.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    po.check_prepared(keys_o.cpu().numpy(), vals_o.cpu().numpy(), sv.cpu().numpy(), so_.cpu().numpy(), order.cpu().numpy(), c['want'])
    cnt = cnt_o.cpu().numpy().view(np.uint32)
    assert (int(cnt[0]), int(cnt[1])) == (len(st['short']), len(st['long'])), (cnt, len(st['short']), len(st['long']))
    po._first_diff(ext_o.cpu().numpy(), st['ext'], 'ext')
    short, long_ = so.plan_sets(desc_o.cpu().numpy().view(np.uint32), cnt, nc)
    assert short == st['short'] and long_ == st['long']
    c['prepared'] = prep
    return prep


def _restore(c):
    eng = c['eng']
    p0, s10, s20 = c['state0']
    for dst, src in zip(eng.tables(), p0):
        dst.copy_(src)
    for dst, src in zip(eng.s1, s10):
        dst.copy_(src)
    if s20 is not None:
        for dst, src in zip(eng.s2, s20):
            dst.copy_(src)


def _reduce(c, prepared, form, grads=None):
    """drx_debug_cdae_reduce from the case's initial state; returns (tables, s1, s2) as numpy arrays"""
    import torch
    from drecpy_amd import _lib
    L, eng, bt = _lib.lib(), c['eng'], c['bt']
    _restore(c)
    g = grads if grads is not None else c['dev']
    o = eng._optim([eng.adam_alpha(eng.lr, 1, eng.beta1, eng.beta2)] * 5)
    sc = eng._ensure_scratch(bt.B, bt.n_touch_slots, hot=c['hot'])
    hot = C.byref(eng._hot_head(c['hot'])) if c['hot'] else None
    rc = L.drx_debug_cdae_reduce(C.byref(eng._params), C.byref(o), C.byref(eng._hist), C.byref(bt), hot,
                                 _lib.ptr(prepared) if prepared is not None else None, prepared.numel() if prepared is not None else 0,
                                 _lib.ptr(g['dz1']), _lib.ptr(g['g2']), _lib.ptr(g['dz2']), form, _lib.ptr(sc), sc.numel(),
                                 _lib.stream_ptr(eng.device))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return [t.clone() for t in eng.tables()], [t.clone() for t in eng.s1], [t.clone() for t in eng.s2] if eng.s2 is not None else None


def _expected_sums(c, blanked):
    """exact gradient of every row the list names: {table index: (rows, g [rows, ld], scalar sums or None)}, hot rows included.
    blanked: the list was prepared ahead — rows whose sole touch was blanked are nobody's here."""
    d, want, gr = c['d'], c['want'], c['grads']
    N, ld = d['N'], c['ld']
    k, v = want['live_keys'].astype(np.int64), want['vals'].astype(np.int64)
    if blanked:
        keep = ~want['blank']
        k, v = k[keep], v[keep]
    dz1, g2, dz2 = (gr[n].astype(np.int64) for n in ('dz1', 'g2', 'dz2'))
    first = np.concatenate([[0], np.flatnonzero(k[1:] != k[:-1]) + 1])
    rows = np.where((k < N)[:, None], 2 * dz1[v], np.where((k < 2 * N)[:, None], g2[v], dz1[v]))      # scale = 1 / (1 - 0.5f) = 2
    sums = np.add.reduceat(rows, first, axis=0)
    ssum = np.add.reduceat(np.where((k >= N) & (k < 2 * N), dz2[v], 0), first)
    kk = k[first]
    out = {}
    for var, lo, hi in ((0, 0, N), (1, N, 2 * N), (2, 2 * N, 2 * N + d['U'])):
        m = (kk >= lo) & (kk < hi)
        out[var] = (kk[m] - lo, sums[m], ssum[m] if var == 1 else None)
    if c['hot']:
        item_of = np.where(d['indptr'][c['uid'] + 1] > d['indptr'][c['uid']], d['indices'][np.minimum(d['indptr'][c['uid']], d['indices'].size - 1)], -1)
        hot_rows = np.flatnonzero(np.bincount(item_of[(item_of >= 0) & (item_of < c['hot'])], minlength=c['hot']))
        assert 0 < hot_rows.size < c['hot']             # (hot items the batch does not keep are among them)
        g_hot = np.stack([2 * dz1[item_of == h].sum(axis=0) for h in hot_rows])
        assert not np.isin(hot_rows, out[0][0]).any()
        out[0] = (np.concatenate([hot_rows, out[0][0]]), np.concatenate([g_hot, out[0][1]]), None)
    return out


def _check_rule(kind, eng, p0, s10, s20, g, p1, s11, s21, what):
    """rows p0 .. under the optimizer's rule on the exact gradient g: Adagrad's accumulator bit for bit, the parameters (Adam: and the
    moments) inside the bound of tests/optim_oracle.py / dense_update_oracle.py for exact sums, as tests/test_gpu_optim_rules.py uses it"""
    assert np.abs(g).max() <= 4096
    g = g.astype(np.float64)
    if kind == 'adagrad':
        acc = (s10.astype(np.float64) + g * g).astype(F)                  # g^2 exact, acc0 + g^2 exact in float64: one rounding
        bad = np.argwhere(_bits(s11) != _bits(acc))
        assert bad.size == 0, f'{what}: {bad.shape[0]} accumulators differ, first at {bad[0].tolist()}: got {s11[tuple(bad[0])]!r}, ' \
                              f'expected {acc[tuple(bad[0])]!r} (g = {g[tuple(bad[0])]})'
        r = oo.apply('adagrad', p0.astype(np.float64), s10.astype(np.float64), None, g, np.abs(g), 1.0, eng.lr, 0.0, eps=eng.opt_eps,
                     exact_sums=True)
        _inside(p1, r.p, r.dp, f'{what} p')
    else:
        a = du._adam(p0.astype(np.float64), s10.astype(np.float64), s20.astype(np.float64), g, np.abs(g), 1.0,
                     eng.adam_alpha(eng.lr, 1, eng.beta1, eng.beta2), 0.0, eng.beta1, eng.beta2, eng.opt_eps, exact_sums=True)
        np.testing.assert_allclose(s11, a.m, rtol=1e-6, atol=0, err_msg=f'{what} m')
        np.testing.assert_allclose(s21, a.v, rtol=1e-6, atol=0, err_msg=f'{what} v')
        _inside(p1, a.p, a.dp, f'{what} p')


def _check_against_exact(c, got, blanked):
    eng, kind = c['eng'], ('adam' if c['eng'].s2 is not None else 'adagrad')
    p0, s10, s20 = c['state0']
    p1, s11, s21 = got
    h = lambda t: t.cpu().numpy()
    sums = _expected_sums(c, blanked)
    for var, name in ((0, 'W'), (1, 'W2T'), (2, 'V')):
        rows, g, gs = sums[var]
        assert np.unique(rows).size == rows.size
        P0, S10, P1, S11 = h(p0[var]), h(s10[var]), h(p1[var]), h(s11[var])
        S20, S21 = (h(s20[var]), h(s21[var])) if s20 is not None else (None, None)
        sel = lambda a: None if a is None else a[rows]
        _check_rule(kind, eng, P0[rows], S10[rows], sel(S20), g, P1[rows], S11[rows], sel(S21), name)
        rest = np.ones(P0.shape[0], dtype=bool)
        rest[rows] = False
        for before, after, what in ((P0, P1, 'table'), (S10, S11, 's1'), (S20, S21, 's2')):
            if before is not None:
                assert np.array_equal(_bits(before[rest]), _bits(after[rest])), f'{name}: a row the list does not name changed ({what})'
        if var == 1:                                    # the output bias rides with the W2T rows
            B0, A0, B1, A1 = h(p0[4]), h(s10[4]), h(p1[4]), h(s11[4])
            C0, C1 = (h(s20[4]), h(s21[4])) if s20 is not None else (None, None)
            _check_rule(kind, eng, B0[rows], A0[rows], sel(C0), gs, B1[rows], A1[rows], sel(C1), 'b2')
            for before, after in ((B0, B1), (A0, A1), (C0, C1)):
                if before is not None:
                    assert np.array_equal(_bits(before[rest]), _bits(after[rest])), 'b2: an entry the list does not name changed'
    gb = c['grads']['dz1'].astype(np.int64).sum(axis=0)                # the hidden bias: column sums over the whole batch
    _check_rule(kind, eng, h(p0[3]), h(s10[3]), h(s20[3]) if s20 is not None else None, gb, h(p1[3]), h(s11[3]),
                h(s21[3]) if s21 is not None else None, 'b')


SHAPES = [  # K, long list, optimizer, form, the form this is
    (64, False, 'adagrad', 0, 'streamed'), (128, False, 'adagrad', 0, 'streamed'), (256, False, 'adagrad', 0, 'streamed'),
    (64, False, 'adagrad', 1, 'planned-short'), (128, False, 'adagrad', 1, 'planned-short'), (256, False, 'adagrad', 1, 'planned-short'),
    (50, False, 'adagrad', 0, 'planned-short'), (128, False, 'adam', 0, 'planned-short'), (16, False, 'adagrad', 0, 'planned-short'),
    (64, True, 'adagrad', 0, 'planned-long'), (128, True, 'adagrad', 0, 'planned-long')]


@pytest.mark.parametrize('ahead', [True, False], ids=['prepared', 'inline'])
@pytest.mark.parametrize('K,long_list,opt,form,which', SHAPES, ids=[f'{s[4]}-K{s[0]}-{s[2]}' for s in SHAPES])
def test_designed_list_reduces_exactly(K, long_list, opt, form, which, ahead):
    """every row's accumulator equals float32(acc0 + g^2) bit for bit (Adam: moments within rtol 1e-6), parameters follow the rule on the
    exact g, rows nobody names — and rows whose sole touch a preparation blanked — keep every bit"""
    c = _case(K, long_list, opt)
    prep = _prepared(c) if ahead else None
    got = _reduce(c, prep, form)
    _check_against_exact(c, got, blanked=ahead and c['ld'] > 16)


def test_designed_list_without_slack_behind():
    """n_touch_slots = the touches exactly: the last segment reaches the list's last slot, in a partial chunk"""
    c = _case(64, False, slack=0)
    assert c['T'] == c['want']['n_valid'] and c['T'] % 32 != 0
    for prep in (_prepared(c), None):
        for form in (0, 1):
            _check_against_exact(c, _reduce(c, prep, form), blanked=prep is not None)


@pytest.mark.parametrize('K', [64, 128, 256])
def test_streamed_equals_planned_bit_for_bit(K):
    """drx_segstream.hpp: the streamed kernel's sums are those of k_seg_reduce_planned, in the same order — with integer rows (any order
    gives the same bits) and with normal ones (the order shows)"""
    import torch
    c = _case(K, False)
    prep = _prepared(c)
    gen = torch.Generator(device=c['eng'].device)
    gen.manual_seed(K)
    normal = {k: torch.randn(v.shape, generator=gen, device=v.device, dtype=torch.float32) for k, v in c['dev'].items()}
    for grads in (None, normal):
        for p in (prep, None):
            a, b = _reduce(c, p, 0, grads), _reduce(c, p, 1, grads)
            names = [f'{kind} {n}' for kind in ('table', 'slot') for n in ('W', 'W2T', 'V', 'b', 'b2')]
            for name, x, y in zip(names, a[0] + a[1], b[0] + b[1]):
                assert torch.equal(x, y), f'{name} differs in {int((x != y).sum())} of {x.numel()} floats ' \
                                          f'({"integer" if grads is None else "normal"} rows, {"prepared" if p is not None else "inline"} list)'
            assert not torch.equal(a[0][0], c['state0'][0][0])


def test_hot_head_sums_exactly():
    """H = 64, K = 128, Adagrad, prepared through prepare_sparse(hot=True): a hot item's sum is 2 * sum of dz1_in over the samples that
    keep it (on the matrix cores: exact for integers), its accumulator compared bit for bit; hot items no sample keeps stay untouched"""
    c = _case(128, False, hot=64)
    got = _reduce(c, _prepared(c), 0)
    _check_against_exact(c, got, blanked=True)


def test_planned_form_is_refused_with_a_head_and_on_long_lists():
    from drecpy_amd import _lib
    L = _lib.lib()
    for c in (_case(128, False, hot=64), _case(64, True)):
        eng, bt, g = c['eng'], c['bt'], c['dev']
        prep = _prepared(c)
        o = eng._optim([eng.lr] * 5)
        sc = eng._ensure_scratch(bt.B, bt.n_touch_slots, hot=c['hot'])
        hot = C.byref(eng._hot_head(c['hot'])) if c['hot'] else None
        rc = L.drx_debug_cdae_reduce(C.byref(eng._params), C.byref(o), C.byref(eng._hist), C.byref(bt), hot, _lib.ptr(prep), prep.numel(),
                                     _lib.ptr(g['dz1']), _lib.ptr(g['g2']), _lib.ptr(g['dz2']), 1, _lib.ptr(sc), sc.numel(),
                                     _lib.stream_ptr(eng.device))
        assert rc == -1                                 # DRX_EINVAL
