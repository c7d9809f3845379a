"""The hot head of the sampled Adagrad step (include/drx.h DrxHotHead): the W rows of the H items of highest training-set degree get
their gradients from the transposed kept-mask times dz1 on the matrix cores instead of the touch list.  Same oracle, same gates as the
plain step (tests/test_gpu_cdae.py); bit-reproducible; rows no sample keeps untouched; refused where it does not apply."""
import numpy as np
import pytest
import torch

from oracle import cdae_oracle as co
from helpers import batch_rows, hash_u32, q_threshold, synth_history


def _engine(U, N, K, seed=0):
    from drecpy_amd.engine import CdaeEngine
    rng = np.random.default_rng(seed)
    p = co.init_params(rng, U, N, K, np.float64)
    eng = CdaeEngine(U, N, K)
    eng.set_params(**{k: v for k, v in p.items()})
    return eng, p, rng


def _kept(indptr, indices, uids, N, seed, q):
    _, keep_off, _ = batch_rows(indptr, indices, uids, N)
    B = len(uids)
    keep = np.concatenate([hash_u32(seed, np.full(keep_off[b + 1] - keep_off[b], b), np.arange(keep_off[b + 1] - keep_off[b])) >= q_threshold(q)
                           for b in range(B)]).astype(np.uint8)
    return batch_rows(indptr, indices, uids, N, keep)[2]


def _hot_rows_for(eng, opt_kind, bt, H):
    import ctypes as C
    from drecpy_amd import _lib
    return _lib.lib().drx_cdae_hot_rows_for(C.byref(eng._params), opt_kind, bt.B, bt.n_touch_slots, H)


def _run(K, H, prepared, steps=3, U=30000, N=400, B=2048, seed=21, oracle=True, poison=None, uids_of=None):
    eng, p, rng = _engine(U, N, K, seed=seed)
    indptr, indices = synth_history(rng, U, N, 12, zipf=1.05)
    eng.set_history(indptr, indices)
    eng.set_hot_rows(H, min_batch=0)
    eng.init_optimizer('adagrad', 0.05, 1e-3)
    st = co.sparse_state(p, 'adagrad')
    q = 0.2
    qf = float(np.float32(q))
    buf = None
    for step in range(steps):
        uids = rng.integers(0, U, size=B) if uids_of is None else uids_of(eng, indptr, indices, rng, B)
        iids = rng.integers(0, N, size=B)
        y = (rng.random(B) < 0.3).astype(np.float32)
        seed_m = 5100 + step
        bt, alive = eng.make_batch(uids, iids, y, q=q, mask_seed=seed_m)
        assert bt.n_touch_slots + 2 * B <= 8 * (2 * N + U)                  # short segments: the streamed path
        if prepared:
            buf = eng.prep_buffer(bt, buf, eng._hot_for(bt))
            if poison is not None:
                buf.fill_(poison)
            pb = eng.prepare_sparse(bt, buf, hot=True)
            assert pb._drx_hot == H
            lg = eng.step_sparse(step, bt, 'bce', want_loss=True, prepared=pb)
        else:
            lg = eng.step_sparse(step, bt, 'bce', want_loss=True, hot=True)
        if oracle:
            kept = _kept(indptr, indices, uids, N, seed_m, q)
            lo, _ = co.sparse_step(p, st, step, uids, iids, y, kept, qf, 0.05, 1e-3, 'bce', 'adagrad')
            lg = lg.cpu().numpy()
            assert abs(lg[0] - lo) / abs(lo) < 1e-4, (step, lg, lo)
    torch.cuda.synchronize()
    return eng, p, eng.get_params(), [t.clone() for t in eng.tables()] + [s.clone() for s in eng.s1]


@pytest.mark.gpu
@pytest.mark.parametrize('prepared', [False, True])
@pytest.mark.parametrize('K,H,B', [(64, 32, 2048), (128, 32, 2048), (128, 64, 2048), (128, 64, 2000), (64, 32, 1000), (125, 64, 1000)])
def test_hot_head_steps_match_oracle(K, H, B, prepared):
    """B = 2000 / 1000: an odd number of 16-sample halves of mask words (the last workgroup zeroes the half behind the batch), a last
    slice of 464 / 488 samples and k-steps that run past the batch.  K = 125: rows padded to 128 floats."""
    eng, p, g, _ = _run(K, H, prepared, B=B)
    for k in p:
        np.testing.assert_allclose(g[k], p[k], rtol=0, atol=3e-5, err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize('K', [64, 128])
def test_hot_head_on_and_off_agree_and_runs_are_bit_equal(K):
    _, _, g_off, _ = _run(K, 0, True, oracle=False)
    _, _, g_on, t_on = _run(K, 64, True, oracle=False)
    _, _, _, t_on2 = _run(K, 64, True, oracle=False)
    for k in g_off:
        np.testing.assert_allclose(g_on[k], g_off[k], rtol=0, atol=3e-5, err_msg=k)
    for a, b in zip(t_on, t_on2):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_hot_head_prepared_matches_inline():
    _, _, g_in, _ = _run(128, 64, False, oracle=False)
    _, _, g_pr, _ = _run(128, 64, True, oracle=False)
    for k in g_in:
        np.testing.assert_allclose(g_pr[k], g_in[k], rtol=0, atol=3e-5, err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize('B', [2048, 2000, 1000])
@pytest.mark.parametrize('fill', [0, 0x11, 0xFF])
def test_hot_head_poisoned_prepared_buffer_gives_the_clean_result(fill, B):
    """The mask words live behind the list in the prepared buffer: the preparation writes every one of them itself (B = 2000 / 1000:
    also the half-word behind the batch's last sixteen samples)."""
    _, _, _, clean = _run(128, 64, True, oracle=False, B=B)
    _, _, _, dirty = _run(128, 64, True, oracle=False, poison=fill, B=B)
    for a, b in zip(clean, dirty):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_hot_row_no_sample_keeps_stays_bit_equal():
    """A hot item none of the batch's users has: its W row and accumulator are not written at all."""
    state = {}

    def users_without(eng, indptr, indices, rng, B):
        x = int(eng._hot_item[-1].item())
        state['x'] = x
        ok = np.array([x not in indices[indptr[u]:indptr[u + 1]] for u in range(len(indptr) - 1)])
        return rng.choice(np.flatnonzero(ok), size=B)

    eng0, _, _, _ = _run(128, 64, True, steps=0, oracle=False)
    w0, a0 = eng0.W.clone(), eng0.s1[0].clone()
    eng, _, _, _ = _run(128, 64, True, steps=2, oracle=False, uids_of=users_without)
    x = state['x']
    assert torch.equal(eng.W[x], w0[x])
    assert torch.equal(eng.s1[0][x], a0[x])
    assert not torch.equal(eng.W, w0)


@pytest.mark.gpu
def test_hot_head_on_an_unsupported_path_is_refused():
    """A head-bearing list handed to Adam (or any path but the streamed Adagrad one) is DRX_EINVAL, not a silent wrong answer."""
    from drecpy_amd import _lib
    U, N, K, B = 30000, 400, 128, 2048
    eng, p, rng = _engine(U, N, K, seed=3)
    indptr, indices = synth_history(rng, U, N, 12, zipf=1.05)
    eng.set_history(indptr, indices)
    eng.set_hot_rows(64, min_batch=0)
    eng.init_optimizer('adagrad', 0.05, 1e-3)
    bt, alive = eng.make_batch(rng.integers(0, U, size=B), rng.integers(0, N, size=B), (rng.random(B) < 0.3).astype(np.float32),
                               q=0.2, mask_seed=1)
    pb = eng.prepare_sparse(bt, hot=True)
    assert pb._drx_hot == 64
    eng.init_optimizer('adam', 1e-3, 1e-3)
    w = eng.W.clone()
    with pytest.raises(_lib.DrxError):
        eng.step_sparse(0, bt, 'bce', prepared=pb)
    torch.cuda.synchronize()
    assert torch.equal(eng.W, w)
    # the library's own answer (drx_cdae_hot_rows_for, what _hot_for asks) is 0 exactly where the step refuses and H where it runs
    assert _hot_rows_for(eng, _lib.OPT_ADAM, bt, 64) == 0 and eng._hot_for(bt) == 0
    assert _hot_rows_for(eng, _lib.OPT_ROWWISE_ADAGRAD, bt, 64) == 0
    eng.init_optimizer('rowwise_adagrad', 0.05, 1e-3)
    with pytest.raises(_lib.DrxError):
        eng.step_sparse(0, bt, 'bce', prepared=pb)
    torch.cuda.synchronize()
    assert torch.equal(eng.W, w)
    eng.init_optimizer('adagrad', 0.05, 1e-3)
    assert _hot_rows_for(eng, _lib.OPT_ADAGRAD, bt, 64) == 64 and eng._hot_for(bt) == 64
    eng.step_sparse(0, bt, 'bce', prepared=pb)
    torch.cuda.synchronize()
    assert not torch.equal(eng.W, w)


@pytest.mark.gpu
def test_a_list_is_only_trained_with_the_head_it_was_prepared_with():
    """The library records every prepared buffer's H (include/drx.h): a head-bearing list handed to the plain prepared step or to the
    column-sharded step, and a plain list handed to the step with a head, are DRX_EINVAL — checked in the library, whatever the caller
    says (a view of the buffer carries none of the engine's attributes)."""
    from drecpy_amd import _lib
    U, N, K, B = 30000, 400, 128, 2048
    eng, p, rng = _engine(U, N, K, seed=4)
    indptr, indices = synth_history(rng, U, N, 12, zipf=1.05)
    eng.set_history(indptr, indices)
    eng.set_hot_rows(64, min_batch=0)
    eng.init_optimizer('adagrad', 0.05, 1e-3)
    bt, alive = eng.make_batch(rng.integers(0, U, size=B), rng.integers(0, N, size=B), (rng.random(B) < 0.3).astype(np.float32),
                               q=0.2, mask_seed=2)
    tabs = [t.clone() for t in eng.tables()]
    pb = eng.prepare_sparse(bt, hot=True)
    assert pb._drx_hot == 64
    with pytest.raises(_lib.DrxError):
        eng.step_sparse(0, bt, 'bce', prepared=pb[:])                      # the plain prepared step
    h, d = eng.kshard_forward(bt, pb[:])
    with pytest.raises(_lib.DrxError):
        eng.step_sparse(0, bt, 'bce', prepared=pb[:], kshard=(h, d))       # the column-sharded step
    plain = eng.prepare_sparse(bt)
    assert plain._drx_hot == 0
    view = plain[:]
    view._drx_hot = 64
    with pytest.raises(_lib.DrxError):
        eng.step_sparse(0, bt, 'bce', prepared=view)                       # a plain list and the step with a head
    torch.cuda.synchronize()
    for a, b in zip(tabs, eng.tables()):
        assert torch.equal(a, b)
    eng.step_sparse(0, bt, 'bce', prepared=eng.prepare_sparse(bt, pb, hot=True))     # the matching pair trains
    torch.cuda.synchronize()
    assert not torch.equal(tabs[0], eng.W)


@pytest.mark.gpu
def test_no_head_at_rows_of_256_floats():
    """ld = 256 takes no head: the engine does not ask for one and the library refuses one."""
    from drecpy_amd import _lib
    import ctypes as C
    U, N, K, B = 30000, 400, 256, 2048
    eng, p, rng = _engine(U, N, K, seed=6)
    indptr, indices = synth_history(rng, U, N, 12, zipf=1.05)
    eng.set_history(indptr, indices)
    eng.set_hot_rows(64, min_batch=0)
    eng.init_optimizer('adagrad', 0.05, 1e-3)
    bt, alive = eng.make_batch(rng.integers(0, U, size=B), rng.integers(0, N, size=B), (rng.random(B) < 0.3).astype(np.float32),
                               q=0.2, mask_seed=3)
    assert eng._hot_for(bt) == 0 and eng.prepare_sparse(bt, hot=True)._drx_hot == 0
    assert _hot_rows_for(eng, _lib.OPT_ADAGRAD, bt, 64) == 0              # the library's answer, and its step's:
    w = eng.W.clone()
    eng._hot_for = lambda bt: 64                                            # (an engine that asked for a head all the same)
    with pytest.raises(_lib.DrxError):
        eng.step_sparse(0, bt, 'bce', hot=True)
    torch.cuda.synchronize()
    assert torch.equal(eng.W, w)
    del eng._hot_for
    eng.step_sparse(0, bt, 'bce', hot=True)                                # H = 0: the plain step runs
    torch.cuda.synchronize()
    assert not torch.equal(eng.W, w)
    buf = torch.empty(int(_lib.lib().drx_cdae_prep_bytes_hot(C.byref(eng._params), bt.B, bt.n_touch_slots, 64)), dtype=torch.uint8,
                      device=eng.device)
    rc = _lib.lib().drx_cdae_sparse_prepare_hot(C.byref(eng._params), C.byref(eng._hist), C.byref(bt), C.byref(eng._hot_head(64)),
                                                _lib.ptr(buf), buf.numel(), _lib.stream_ptr(eng.device))
    assert rc != 0


@pytest.mark.gpu
def test_column_sharded_pipeline_takes_no_head():
    """ColumnShardedCdae.pipeline with prepare='local' prepares through the engine with its own step_fn: the lists carry no head even
    when the head's conditions hold, and the pipeline equals the same seeds stepped inline."""
    from drecpy_amd.dist import ColumnShardedCdae
    U, N, K, q = 30000, 400, 64, 0.2
    rng = np.random.default_rng(8)
    indptr, indices = synth_history(rng, U, N, 12, zipf=1.05)
    outs = []
    for piped in (True, False):
        m = ColumnShardedCdae(U, N, K, 0, 1, 'cuda:0', indptr, indices, q=q, prepare='local')
        m.engine.set_hot_rows(64, min_batch=0)
        if piped:
            pipe = m.pipeline(2048, 5, lambda s: 77 + s, lambda s: 1000 + s)
            for _ in range(4):
                pipe.run_step()
            assert all(getattr(b, '_drx_hot', 0) == 0 for b in pipe.prep if b is not None)
        else:
            for s in range(4):
                uid, iid, y, ko = m.engine.sample_device(2048, 5, 77 + s)
                bt, alive = m.engine.make_batch(uid, iid, y, keep_off=ko, q=q, mask_seed=1000 + s)
                m.step(s, bt)
        torch.cuda.synchronize()
        outs.append([t.clone() for t in m.engine.tables()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_one_full_size_step_with_the_default_head_matches_the_oracle_on_compacted_tables():
    """The headline shape with the engine's DEFAULT head (64 rows, 128 slices of 512 samples, nearly dense mask columns): one step
    prepared as the bench's pipeline prepares it, against the fp64 oracle on tables compacted to the rows the batch names (as
    tests/test_gpu_fullsize.py does for the plain step); rows the batch does not name keep their bits."""
    from test_gpu_fullsize import _setup
    B, K, q, lr, reg, seed = 65536, 128, 0.2, 0.05, 1e-3, 4242
    eng, U, N, ip, idx = _setup('synth-10m')
    assert eng.hot_rows == 64
    uid, iid, y, ko = eng.sample_device(B, 5, seed, n_items=N)
    torch.cuda.synchronize()
    ul_, deg = uid.long(), (ip[uid.long() + 1] - ip[uid.long()])
    T = int(deg.sum())
    row = torch.repeat_interleave(torch.arange(B, device='cuda'), deg)
    j = torch.arange(T, device='cuda') - torch.repeat_interleave(torch.cumsum(deg, 0) - deg, deg)
    items = idx[(ip[ul_][row] + j)].long()
    keep = torch.as_tensor(co.drx_hash_u32(seed, row.cpu().numpy(), j.cpu().numpy()) >= co.q_threshold(q)).cuda()
    il = torch.unique(torch.cat([items, iid.long()]))
    uu = torch.unique(ul_)
    imap = torch.full((N,), -1, dtype=torch.long, device='cuda'); imap[il] = torch.arange(il.numel(), device='cuda')
    umap = torch.full((U,), -1, dtype=torch.long, device='cuda'); umap[uu] = torch.arange(uu.numel(), device='cuda')
    f64 = lambda t: t.double().cpu().numpy()
    p = {'W': f64(eng.W[il, :K]), 'W_': np.ascontiguousarray(f64(eng.W2T[il, :K]).T), 'V': f64(eng.V[uu, :K]), 'b': f64(eng.b[:K]),
         'b_': f64(eng.b2[il])}
    before = [t.clone() for t in eng.tables()]
    kept_flat = imap[items[keep]].cpu().numpy()
    kept_len = torch.zeros(B, dtype=torch.long, device='cuda').index_add_(0, row[keep], torch.ones(int(keep.sum()), dtype=torch.long, device='cuda'))
    kept = np.split(kept_flat, np.cumsum(kept_len.cpu().numpy())[:-1])
    cu, ci, yy = umap[ul_].cpu().numpy(), imap[iid.long()].cpu().numpy(), y.cpu().numpy().astype(np.float64)
    bt, alive = eng.make_batch(uid, iid, y, keep_off=ko, q=q, mask_seed=seed)
    prep = eng.prepare_sparse(bt, hot=True)
    assert prep._drx_hot == 64
    eng.step_sparse(0, bt, prepared=prep)
    torch.cuda.synchronize()
    st = co.sparse_state(p, 'adagrad')
    co.sparse_step(p, st, 0, cu, ci, yy, kept, float(np.float32(q)), lr, reg, 'bce', 'adagrad', accumulate='matrix')
    got = {'W': f64(eng.W[il, :K]), 'W_': f64(eng.W2T[il, :K]).T, 'V': f64(eng.V[uu, :K]), 'b': f64(eng.b[:K]), 'b_': f64(eng.b2[il])}
    for k_ in p:
        np.testing.assert_allclose(got[k_], p[k_], rtol=0, atol=2e-5, err_msg=k_)
    hot = eng._hot_item.long()
    assert bool(torch.isin(hot, items[keep]).all())                       # (every hot row was trained through the head)
    tw = torch.zeros(N, dtype=torch.bool, device='cuda'); tw[items[keep]] = True
    to = torch.zeros(N, dtype=torch.bool, device='cuda'); to[iid.long()] = True
    tu = torch.zeros(U, dtype=torch.bool, device='cuda'); tu[uu] = True
    assert torch.equal(before[0][~tw], eng.W[~tw]) and torch.equal(before[1][~to], eng.W2T[~to])
    assert torch.equal(before[2][~tu], eng.V[~tu]) and torch.equal(before[4][~to], eng.b2[~to])


def test_hot_set_is_the_highest_degrees_ties_to_the_lower_id():
    """CPU: the hot set is the H items of highest degree in the training history; equal degrees go to the lower item id."""
    from drecpy_amd.engine import CdaeEngine
    idx = torch.tensor([5, 5, 5, 2, 2, 7, 7, 1, 9, 9, 3, 3, 0], dtype=torch.int32)
    # degrees: 5:3, 2:2, 7:2, 9:2, 3:2, 1:1, 0:1
    assert CdaeEngine.hot_set(idx, 12, 4).tolist() == [5, 2, 3, 7]
    assert CdaeEngine.hot_set(idx, 12, 7).tolist() == [5, 2, 3, 7, 9, 0, 1]
    assert CdaeEngine.hot_set(torch.zeros(0, dtype=torch.int32), 4, 2).tolist() == [0, 1]


def test_the_hot_rows_override_is_checked(monkeypatch):
    """CPU: DRX_HOT_ROWS must be 0 or a multiple of 32 up to 1024."""
    from drecpy_amd import _lib
    from drecpy_amd.engine import CdaeEngine
    monkeypatch.delenv('DRX_HOT_ROWS', raising=False)
    assert CdaeEngine.default_hot_rows() == CdaeEngine.HOT_ROWS
    for ok in ('0', '32', '128'):
        monkeypatch.setenv('DRX_HOT_ROWS', ok)
        assert CdaeEngine.default_hot_rows() == int(ok)
    for bad in ('48', '-32', '2048'):
        monkeypatch.setenv('DRX_HOT_ROWS', bad)
        with pytest.raises(_lib.DrxError):
            CdaeEngine.default_hot_rows()
