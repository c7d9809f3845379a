"""Where the dense-only update rules (DRX_OPT_SGD .. DRX_OPT_RMSPROP_MOMENTUM) must be refused, and the rule-taking entry points of the
DMF / Caser steps at their edges.  The sparse and sharded entry points are called from inside a real step — every other argument valid,
only DrxOptim.kind changed — and must answer DRX_EINVAL without launching anything: the step that follows is bit-equal to an undisturbed
one.  A sharded CDAE.fit() (two gloo processes sharing the GPU, rows and columns layout) raises the documented message for a forced
optimizer= of the new kinds."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from helpers import new_rendezvous, retry_infra  # noqa: E402

pytestmark = pytest.mark.gpu
DRX_EINVAL = -1
NEW_KINDS = (3, 4, 5, 6, 7)


def _probe_kinds(monkeypatch, name, seen, field='kind', arg=1, codes=NEW_KINDS):
    """wrap lib.<name>: its FIRST call is preceded by one call per code with the struct behind argument `arg` given that code in
    `field` (everything else as the caller passed it); the return codes go to seen[name]"""
    from drecpy_amd import _lib
    lib = _lib.lib()
    real = getattr(lib, name)

    def wrapper(*args):
        if name not in seen:
            o = args[arg]._obj
            keep = getattr(o, field)
            seen[name] = []
            for code in codes:
                setattr(o, field, code)
                seen[name].append(real(*args))
            setattr(o, field, keep)
        return real(*args)
    monkeypatch.setattr(lib, name, wrapper)


def test_row_sharded_entry_points_refuse_the_dense_kinds(monkeypatch):
    """drx_shard_step_local and drx_shard_apply (the call-by-call step), drx_shard_phase_local and drx_shard_phase_tail (the exchanges
    issued by the library; the tail refuses before anything is sent) at world 1"""
    import test_gpu_shard as ts
    base = ts._run_rank(0, 1, False)
    seen = {}
    for name in ('drx_shard_step_local', 'drx_shard_apply'):
        _probe_kinds(monkeypatch, name, seen)
    got = ts._run_rank(0, 1, False)
    assert seen == {'drx_shard_step_local': [DRX_EINVAL] * 5, 'drx_shard_apply': [DRX_EINVAL] * 5}
    assert all(np.array_equal(base[0][k], got[0][k]) for k in base[0]) and base[1] == got[1]
    monkeypatch.undo()
    ts._chunked(monkeypatch, 9000, 1)
    base = ts._run_rank(0, 1, False, force=True, pipelined=True, bypass=False, transport='rccl', phases=True)
    seen = {}
    _probe_kinds(monkeypatch, 'drx_shard_phase_tail', seen)
    got = ts._run_rank(0, 1, False, force=True, pipelined=True, bypass=False, transport='rccl', phases=True)
    assert seen == {'drx_shard_phase_tail': [DRX_EINVAL] * 5}
    assert all(np.array_equal(base[0][k], got[0][k]) for k in base[0]) and base[1] == got[1]


def test_column_sharded_and_sparse_steps_refuse_the_dense_kinds(monkeypatch):
    """drx_cdae_kshard_step inside ColumnShardedCdae.step, drx_cdae_step_sparse and drx_cdae_step_sparse_prepared inside CdaeEngine.step_sparse"""
    import test_gpu_kshard as tk
    from drecpy_amd.dist import ColumnShardedCdae
    from drecpy_amd.engine import CdaeEngine
    p, indptr, indices, batches = tk._problem(64)

    def run_columns():
        m = ColumnShardedCdae(tk.U, tk.N, 64, 0, 1, 'cuda:0', indptr, indices, q=tk.Q)
        m.set_params_global(**p)
        for s in range(2):
            uid, iid, y, ko = m.engine.sample_device(512, 5, 77 + s)
            bt, alive = m.engine.make_batch(uid, iid, y, keep_off=ko, q=tk.Q, mask_seed=1000 + s)
            m.step(s, bt)
        torch.cuda.synchronize()
        return [t.clone() for t in m.engine.tables() + m.engine.s1]

    def run_sparse(prepared):
        e = CdaeEngine(tk.U, tk.N, 64)
        e.set_params(**p); e.set_history(indptr, indices); e.init_optimizer('adagrad', 0.05, 1e-3)
        for s, (uid, iid, y, seed) in enumerate(batches[:2]):
            bt, alive = e.make_batch(uid, iid, y, q=tk.Q, mask_seed=seed)
            e.step_sparse(s, bt, prepared=e.prepare_sparse(bt) if prepared else None)
        torch.cuda.synchronize()
        return [t.clone() for t in e.tables() + e.s1]
    base = run_columns(), run_sparse(False), run_sparse(True)
    seen = {}
    for name in ('drx_cdae_kshard_step', 'drx_cdae_step_sparse', 'drx_cdae_step_sparse_prepared'):
        _probe_kinds(monkeypatch, name, seen)
    got = run_columns(), run_sparse(False), run_sparse(True)
    assert seen == {n: [DRX_EINVAL] * 5 for n in ('drx_cdae_kshard_step', 'drx_cdae_step_sparse', 'drx_cdae_step_sparse_prepared')}
    for a, b in zip(base, got):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- the rule-taking entry points of the DMF / Caser steps ---------------------------------------------------------------------------
def _dmf_engine():
    import test_gpu_optim_models as tm
    from drecpy_amd.engine_dmf import DmfEngine
    U, N, csr, csc, dense, p0, batches, probe = tm._dmf_problem()
    eng = DmfEngine(U, N, (16,), (24, 16), True)
    eng.set_interactions(csr, csc)
    eng.set_params(p0)
    eng.reg = 1e-3
    return eng, batches


def _caser_engine():
    import test_gpu_optim_models as tm
    from drecpy_amd.engine_caser import CaserEngine
    (U, N, L, T, neg, d, n_v, n_h), p0, batches, probe = tm._caser_problem()
    eng = CaserEngine(U, N, L, T, neg, d, n_v, n_h)
    eng.set_params(p0)
    eng.reg = 1e-4
    return eng, batches


def _steps(eng, batches, n=3):
    for s, b in enumerate(batches[:n]):
        eng.step(s, *b) if len(b) == 3 else eng.step(s, b[0], b[1], b[2], b[3], 0.5)
    torch.cuda.synchronize()
    return {k: v.copy() for k, v in eng.get_params().items()}, {n_: tuple(None if t is None else t.clone() for t in st) for n_, st in eng.state.items()}


@pytest.mark.parametrize('rule', ['momentum', 'rmsprop_momentum'])
def test_dmf_and_caser_step_entry_points_refuse_unknown_kinds_and_missing_slots(monkeypatch, rule):
    """drx_dmf_step_small_opt, drx_dmf_k0_update (opt_kind), drx_caser_step_small_opt, drx_rows_csr_opt_multi inside real steps: an unknown
    kind and the row-wise Adagrad are DRX_EINVAL; so is a required slot passed as NULL; the steps around them are undisturbed"""
    import test_gpu_optim_models as tm
    from drecpy_amd import _lib
    lib = _lib.lib()
    bad = (2, 8, -1)
    runs = []
    for probed in (False, True):
        seen = {}
        if probed:
            raw_k0, raw_small = lib.drx_dmf_k0_update, lib.drx_dmf_step_small_opt
            _probe_kinds(monkeypatch, 'drx_dmf_step_small_opt', seen, arg=7, codes=bad)
            _probe_kinds(monkeypatch, 'drx_dmf_k0_update', seen, field='opt_kind', arg=2, codes=bad)
            _probe_kinds(monkeypatch, 'drx_caser_step_small_opt', seen, arg=7, codes=bad)
            _probe_kinds(monkeypatch, 'drx_rows_csr_opt_multi', seen, arg=2, codes=bad)
            real_k0, real_small = lib.drx_dmf_k0_update, lib.drx_dmf_step_small_opt

            def k0_without_s1(*args):                       # the rule's first slot of K0u missing, once
                if 'k0 slot' not in seen:
                    up = args[2]._obj
                    keep, up.m_u = up.m_u, None
                    seen['k0 slot'] = raw_k0(*args)
                    up.m_u = keep
                return real_k0(*args)

            def small_without_s1(*args):
                if 'small slot' not in seen:
                    seen['small slot'] = raw_small(*args[:4], None, *args[5:])
                return real_small(*args)
            monkeypatch.setattr(lib, 'drx_dmf_k0_update', k0_without_s1)
            monkeypatch.setattr(lib, 'drx_dmf_step_small_opt', small_without_s1)
        out = []
        for make in (_dmf_engine, _caser_engine):
            eng, batches = make()
            eng.set_optimizer(tm._engine_optimizer(rule, 2e-3))
            out.append(_steps(eng, batches))
        runs.append(out)
        if probed:
            assert seen == {'drx_dmf_step_small_opt': [DRX_EINVAL] * 3, 'drx_dmf_k0_update': [DRX_EINVAL] * 3, 'drx_caser_step_small_opt': [DRX_EINVAL] * 3,
                            'drx_rows_csr_opt_multi': [DRX_EINVAL] * 3, 'k0 slot': DRX_EINVAL, 'small slot': DRX_EINVAL}
    for (pa, sa), (pb, sb) in zip(*runs):
        assert all(np.array_equal(pa[k], pb[k]) for k in pa)
        assert all((x is None and y is None) or torch.equal(x, y) for n in sa for x, y in zip(sa[n], sb[n]))


def test_step_small_adam_entries_equal_their_twins_bit_for_bit(monkeypatch):
    """drx_dmf_step_small / drx_caser_step_small against drx_dmf_step_small_opt / drx_caser_step_small_opt with the Adam rule: the engines
    call the twins; here the same steps go through the `_adam` entries instead"""
    from drecpy_amd import _lib
    lib = _lib.lib()
    runs = []
    for old_entry in (False, True):
        if old_entry:
            for name in ('drx_dmf_step_small', 'drx_caser_step_small'):
                real = getattr(lib, name)
                calls = []

                def through_adam(*args, real=real, calls=calls):
                    r = args[7]._obj
                    assert r.kind == 0
                    calls.append(1)
                    return real(*args[:7], r.mu, r.mu2, r.eps, args[8])
                monkeypatch.setattr(lib, name + '_opt', through_adam)
                runs.append(calls)
        out = []
        for make in (_dmf_engine, _caser_engine):
            eng, batches = make()
            eng.lr = 2e-3
            out.append(_steps(eng, batches))
        runs.append(out)
    first, dmf_calls, caser_calls, second = runs
    assert len(dmf_calls) == 3 and len(caser_calls) == 3
    for (pa, sa), (pb, sb) in zip(first, second):
        assert all(np.array_equal(pa[k], pb[k]) for k in pa)
        assert all(torch.equal(x, y) for n in sa for x, y in zip(sa[n], sb[n]))


def test_dmf_and_caser_snapshots_carry_the_slots():
    """snapshot / restore(with_optimizer=True) of DmfEngine and CaserEngine with zero, one and two slots"""
    import test_gpu_optim_models as tm
    for make in (_dmf_engine, _caser_engine):
        for rule in ('sgd', 'momentum', 'rmsprop_momentum'):
            eng, batches = make()
            eng.set_optimizer(tm._engine_optimizer(rule, 2e-3))
            _steps(eng, batches, 2)
            snap = eng.snapshot()
            p2, s2 = _steps(eng, batches[2:], 1)
            eng.restore(snap, with_optimizer=True)
            for n, t in eng.tensors().items():
                assert torch.equal(t, snap['p'][n])
            for n, st in eng.state.items():
                assert sum(t is not None for t in st) == {'sgd': 0, 'momentum': 1, 'rmsprop_momentum': 2}[rule]
                assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(st, snap['s'][n]))
            p3, s3 = _steps(eng, batches[2:], 1)               # the same step again from the restored state: the same bits
            assert all(np.array_equal(p2[k], p3[k]) for k in p2)


# ---- a sharded fit() -----------------------------------------------------------------------------------------------------------------
def _fit_refused_worker(rank, world, rdzv, out, layout, forced):
    dist.init_process_group('gloo', init_method=rdzv, rank=rank, world_size=world)
    from drecpy_amd import optimizers as op
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender import CDAE
    if layout == 'rows':
        from test_gpu_shard import _rows_frame as frame
    else:
        from test_gpu_fit import _frame as frame
    ds = InteractionDataset.read_df(frame(), verbose=False)
    optimizer = {'sgd': 'sgd', 'SGD': op.SGD(0.05, momentum=0.9), 'RMSprop': op.RMSprop(0.01)}[forced]
    model = CDAE(hidden_factors=18, mode='sampled', device_sampler=True, seed=3, verbose=False, layout=layout)
    msg = None
    try:
        model.fit(ds, epochs=2, batch_size=256, learning_rate=0.05, reg_rate=1e-3, neg_ratio=5, optimizer=optimizer)
    except Exception as e:                                  # noqa: BLE001
        msg = str(e)
    torch.cuda.synchronize()
    torch.save({'msg': msg, 'sharded': getattr(model, '_dist_model', None) is not None}, f'{out}.{rank}')
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('layout,forced', [('rows', 'sgd'), ('rows', 'SGD'), ('columns', 'sgd'), ('columns', 'RMSprop')])
@retry_infra
def test_a_sharded_fit_refuses_a_forced_optimizer(tmp_path, layout, forced):
    """CDAE(mode='sampled', device_sampler=True, layout=...).fit(optimizer=...) as two processes of one job: every rank raises, after the
    sharded model was built, with the message that names sparse_optimizer="""
    out = str(tmp_path / 'refused')
    rdzv = new_rendezvous(tmp_path)
    mp.spawn(_fit_refused_worker, args=(2, rdzv, out, layout, forced), nprocs=2, join=True)
    for r in range(2):
        res = torch.load(f'{out}.{r}', weights_only=False)
        assert res['sharded'], res
        assert res['msg'] is not None and 'cannot be forced on a sharded fit()' in res['msg'] and 'sparse_optimizer' in res['msg'], res
