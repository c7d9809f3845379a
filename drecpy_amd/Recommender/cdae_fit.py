"""How CDAE.fit() trains: one class per mode (ReferenceTrainer, SampledTrainer, ShardedTrainer), chosen once in CDAE._pre_fit, each
holding the whole state of its mode from its constructor to close().  The three share their method names (configure_optimizer, sample,
step, run_steps, close) and the attributes `engine` and `sampler` because CDAE's hooks call them; there is no fourth kind to plug in."""
import weakref

import numpy as np

from .. import _lib
from ..Sampler import PointSampler


class CorruptionStream:
    """The corruption draws of cdae.py:63 — N uniform draws per batch row, so a batch always consumes 2·N·B words — from the MT19937
    stream of `random.Random(seed)` (RecommenderABC._rng), generated in C++ (drx_rng_corruption_keep).  TWO generators on the one stream:
    inside fit() two worker threads draw batches t+1 and t+2 at once, each from its own generator advanced to where its batch begins, so
    the stream is still consumed strictly batch by batch.  close() destroys both — after the draw-ahead handle that points at them."""

    def __init__(self, seed, hist_indptr, hist_indices, n_items, q):
        L = self._L = _lib.lib()                        # (looked up once: lib() costs more than a microsecond per call)
        self.gens = [L.drx_rng_create(int(seed)), L.drx_rng_create(int(seed))]
        # at: words each generator has consumed; pos: where the next batch begins; ticket: batches handed to the draw-ahead workers
        self.at, self.pos, self.ticket = [0, 0], 0, 0
        self.indptr, self.indices, self.n_items, self.q = hist_indptr, hist_indices, int(n_items), float(q)
        self.drain = None                               # waits for the draws in flight (set by who runs them)

    def place(self):
        """(ticket, generator, words that generator has to skip) of the next batch"""
        # (claim() only once the batch is really queued: a ticket that was handed out but never submitted would stall both workers)
        gen = self.ticket % 2
        return self.ticket, gen, self.pos - self.at[gen]

    def claim(self, gen, B):
        self.ticket += 1
        self.pos = self.at[gen] = self.pos + 2 * self.n_items * B

    def cursor(self):
        """int64 [4]: ticket, position, words consumed per generator — what CdaeEngine.fit_dense reads and updates in place"""
        return np.array([self.ticket, self.pos, self.at[0], self.at[1]], dtype=np.int64)

    def set_cursor(self, cursor):
        self.ticket, self.pos, self.at = int(cursor[0]), int(cursor[1]), [int(cursor[2]), int(cursor[3])]

    def keep(self, uid, gen=0, at=None, out=None):
        """(keep_off int32 [B+1], keep uint8) of the batch rows `uid`, in batch order.  gen / at: which generator draws and the word of
        the stream where this batch begins (default: the next unclaimed one, after whatever is in flight)."""
        L, B = self._L, len(uid)
        if at is None:
            if self.drain is not None:
                self.drain()
            at, self.pos = self.pos, self.pos + 2 * self.n_items * B
        assert at >= self.at[gen], 'corruption stream claimed out of order'
        if at > self.at[gen]:
            L.drx_rng_discard(self.gens[gen], at - self.at[gen])
        self.at[gen] = at + 2 * self.n_items * B
        uid32 = np.ascontiguousarray(uid, dtype=np.int32)
        if out is not None:                               # caller's buffers (a pinned staging slot): keep holds B * max degree
            keep_off, keep = out
        else:
            u64 = uid32.astype(np.int64)
            keep_off = np.zeros(B + 1, dtype=np.int32)
            keep = np.zeros(max(int((self.indptr[u64 + 1] - self.indptr[u64]).sum()), 1), dtype=np.uint8)
        _lib.check(L.drx_rng_corruption_keep(self.gens[gen], self.indptr.ctypes.data, self.indices.ctypes.data, self.n_items,
                                             uid32.ctypes.data, B, self.q, keep_off.ctypes.data, keep.ctypes.data, len(keep)),
                   'drx_rng_corruption_keep')
        return keep_off, (keep if out is None else keep[:max(int(keep_off[B]), 1)])

    def close(self):
        gens, self.gens = self.gens, []
        for g in gens:
            self._L.drx_rng_destroy(g)


def _recorded_pairs(ds, n_positives):
    """The CSR of every recorded pair where the frame records pairs below the threshold too, else (None, None): the device PointSampler
    draws negatives among the pairs ABSENT from the frame (point_sampler.py:56)."""
    all_ip, all_cols, _ = ds.interaction_csr()
    return (all_ip, all_cols) if len(all_cols) != n_positives else (None, None)


def _single_gpu(model, rule, learning_rate, neg_ratio, reg_rate, kwds):
    """cdae.py:34-45 for the two single-GPU trainers: (engine with weights, history, recorded pairs and the slots of `rule`; host
    sampler; corruption stream).  Leaves _hist_indptr / _hist_indices / _mask_seed on the model."""
    from ..engine import CdaeEngine
    ds = model.interaction_dataset
    eng = CdaeEngine(model.n_users, model.n_items, model.hidden_factors, device=model.device)
    weights = kwds.get('initial_weights')
    if weights is not None:                      # injected weights (TF's GlorotUniform stream is not reproducible)
        eng.set_params(**weights)
    else:
        seed = model.seed if model.seed is not None else np.random.SeedSequence().entropy % (2 ** 32)
        n_params = (2 * model.n_items + model.n_users) * model.hidden_factors
        # large tables are drawn on the device (same distribution, torch's generator instead of numpy's)
        (eng.init_glorot_device if n_params > (1 << 26) else eng.init_glorot)(seed)
    ip, idx = model._hist_indptr, model._hist_indices = ds.positives_csr(model.interaction_threshold)
    eng.set_history(ip, idx)
    eng.set_recorded_pairs(*_recorded_pairs(ds, len(idx)))
    eng.init_optimizer(rule, learning_rate, reg_rate)
    sampler = PointSampler(ds, neg_ratio, model.interaction_threshold, model.seed)
    seed = model.seed if model.seed is not None else model._rng.getrandbits(62)
    model._mask_seed = int(seed)
    return eng, sampler, CorruptionStream(seed, ip, idx, model.n_items, model.corruption_level)


def _push_optimizer(e, o):
    """The registered optimizer's kind and hyper-parameters into the engine (the slots _pre_fit allocated are kept when nothing differs)"""
    kind = o.kind
    if kind == 'adam':
        same = e.s2 is not None and e.opt_kind == 0 and (e.lr, e.beta1, e.beta2, e.opt_eps) == (o.learning_rate, o.beta_1, o.beta_2, o.epsilon)
        if not same:
            e.init_optimizer('adam', o.learning_rate, e.reg_rate, o.beta_1, o.beta_2, o.epsilon)
    elif kind in ('adagrad', 'rowwise_adagrad'):
        e.init_optimizer(kind, o.learning_rate, e.reg_rate, eps=o.epsilon, initial_accumulator=o.initial_accumulator_value)
    else:
        e.init_optimizer(kind, o.learning_rate, e.reg_rate, eps=getattr(o, 'epsilon', None), momentum=o.momentum, rho=getattr(o, 'rho', 0.9))


def _pipeline_token(trainer, batch_size, build):
    """The device sampler runs ahead of the training stream inside the pipeline; sample() only makes sure that `trainer.pipeline` exists
    for this batch size — build(first step) makes one, continuing where the last one stood — and hands step() a token."""
    pipe = trainer.pipeline
    if pipe is None or pipe.B != batch_size:
        pipe = trainer.pipeline = build(0 if pipe is None else pipe.next)
    return ('device-batch', pipe.next)


def _pipeline_step(pipe, want_loss):
    loss = pipe.run_step(want_loss=want_loss)
    return None if not want_loss else float(loss) if isinstance(loss, float) else float(loss[0].item())


class _Batch:
    """What ReferenceTrainer.sample hands step: the reference's list of (uid, iid, value) triples — built from the (uid, iid, value,
    is_negative) arrays only if somebody looks at it (len / iteration / indexing) — carrying what the fused step needs: the users and
    the corruption stream's keep flags, already in a pinned staging slot of the engine."""

    def __init__(self, arrays, val_type, slot, keep_off, keep):
        self._arrays, self._val_type, self._list = arrays, val_type, None
        self.uid, self.slot, self.keep_off, self.keep = arrays[0], slot, keep_off, keep

    def _triples(self):
        if self._list is None:
            vt = self._val_type
            self._list = [(a, b, 0) if ng else (a, b, vt(c)) for a, b, c, ng in zip(*(x.tolist() for x in self._arrays))]
        return self._list

    def __len__(self):
        return len(self._arrays[0])

    def __iter__(self):
        return iter(self._triples())

    def __getitem__(self, k):
        return self._triples()[k]


class ReferenceTrainer:
    """mode='reference'.  Inside fit() the host work of the next batches (sampler triples, N uniform draws per row) runs on the two native
    draw-ahead threads of libdrx while batch t trains; the streams are still consumed strictly batch by batch, and nothing is drawn
    beyond the last epoch."""

    DRAW_AHEAD = 4         # batches in flight: two per worker

    def __init__(self, model, learning_rate, neg_ratio, reg_rate, kwds):
        self.m = weakref.proxy(model)                   # (read at every step: corruption_level, _loss_name, loss_targets)
        self.engine, self.sampler, self.stream = _single_gpu(model, 'adam', learning_rate, neg_ratio, reg_rate, kwds)
        ip, idx = self.stream.indptr, self.stream.indices
        self.max_degree = int(np.diff(ip).max()) if len(ip) > 1 else 0
        self._L = self.stream._L
        self.drawahead = self._L.drx_drawahead_create(self.sampler._host._h, self.stream.gens[0], self.stream.gens[1], ip.ctypes.data, idx.ctypes.data,
                                                      model.n_items)
        self.pending = []                               # draws in flight: what _submit_draw returned, in ticket order
        self.stream.drain = self._drain_draws

    def configure_optimizer(self, optimizer, forced):
        from ..optimizers import N_SLOTS                # (the dense rule of Keras Adam, or of the Adam / Adagrad / SGD / RMSprop passed as `optimizer=`)
        if getattr(optimizer, 'kind', None) not in N_SLOTS or optimizer.kind == 'rowwise_adagrad':
            raise Exception(f'CDAE mode="reference" trains with the dense rules adam, adagrad, sgd, rmsprop (got {optimizer!r}); '
                            f'rowwise_adagrad exists in mode="sampled"')
        _push_optimizer(self.engine, optimizer)

    def _submit_draw(self, B):
        """Claims the next batch's place in both streams (sampler ticket, corruption words) and its buffers — a pinned staging slot of the
        engine for users / offsets / keep flags — and hands the job to its generator's draw-ahead worker.  Returns what _finish_draw needs."""
        eng = self.engine
        ticket, gen, discard = self.stream.place()
        cap = max(B * self.max_degree, 1)
        if eng.device.type == 'cuda':
            stage = eng.stage_acquire(B, cap)
            extra, ptrs = eng.stage_extra(stage[0]), eng.stage_pointers(stage[0])
        else:
            stage = (None, np.empty(B, np.int32), np.empty(B + 1, np.int32), np.empty(cap, np.uint8))
            extra = (np.empty(B, np.int32), np.empty(B, np.float64), np.empty(B, np.uint8))
            ptrs = (stage[1].ctypes.data, extra[0].ctypes.data, extra[1].ctypes.data, extra[2].ctypes.data, stage[2].ctypes.data,
                    stage[3].ctypes.data, len(stage[3]))
        job = self._L.drx_drawahead_submit(self.drawahead, gen, ticket, discard, B, self.stream.q, *ptrs)
        if job < 0:
            _lib.check(int(job), 'drx_drawahead_submit')
        self.stream.claim(gen, B)
        return B, gen, int(job), stage, extra

    def _finish_draw(self, entry):
        B, gen, job, (slot, uid_v, ko_v, kp_v), extra = entry
        rc = self._L.drx_drawahead_wait(self.drawahead, gen, job)
        if rc:
            _lib.check(rc, 'drx_cdae_reference_draw')
        return _Batch((uid_v,) + extra, self.sampler._val_type, slot, ko_v, kp_v[:max(int(ko_v[B]), 1)])

    def _drain_draws(self):
        """Waits for (does not consume) the draws in flight: whoever touches the sampler or a generator directly comes after."""
        for B, gen, job, _, _ in self.pending:
            self._L.drx_drawahead_wait(self.drawahead, gen, job)

    def sample(self, batch_size, **kwds):
        batches_after = kwds.get('batches_after', 1 if kwds.get('more_to_come', False) else 0)
        pending, self.pending = self.pending, []
        if pending and pending[0][0] == batch_size:
            batch = self._finish_draw(pending.pop(0))
        else:
            for entry in pending:                                  # (batches of another size were drawn: consumed, like draws)
                self._finish_draw(entry)
            pending = []
            batch = self._finish_draw(self._submit_draw(int(batch_size)))
        while len(pending) < min(self.DRAW_AHEAD, batches_after):
            pending.append(self._submit_draw(int(batch_size)))
        self.pending = pending
        return batch

    def step(self, batch, step, want_loss):
        """One dense step on whatever sample() — CDAE's or a replaced _sample_batch — returned: a _Batch in a pinned slot, a _Batch
        with keep arrays (no GPU), four numpy arrays, or the reference's list of triples (their flags are drawn here)."""
        m, eng = self.m, self.engine
        slot = getattr(batch, 'slot', None)
        if slot is not None:                                       # already in pinned memory: no copy
            bt = eng.batch_in_slot(slot, len(batch.uid), int(batch.keep_off[-1]), m.corruption_level)
        else:
            if getattr(batch, 'keep', None) is not None:
                uid, keep_off, keep = batch.uid, batch.keep_off, batch.keep
            else:
                uid = m._batch_arrays(batch)[0]
                keep_off, keep = self.stream.keep(uid)
            bt, alive = eng.make_batch(uid, keep_off=keep_off, keep=keep, q=m.corruption_level, n_touch_slots=int(keep_off[-1]))
        loss = eng.step_dense(step, bt, m._loss_name, m.loss_targets, want_loss=want_loss)
        if slot is not None:
            eng.stage_release(slot)
        return float(loss.sum().item()) if want_loss else None

    def run_steps(self, first_step, n_steps, batch_size):
        """fit()'s quiet path: the whole sample -> step loop of the remaining epochs in one library call (drx_cdae_fit_dense).  Same
        streams, same arithmetic, same launches as the per-step loop; returns the steps done."""
        B, m = int(batch_size), self.m
        cap = max(B * self.max_degree, 1)
        # (no GPU; draws in flight; the loop's pinned staging ring would exceed 1 GB)
        if self.engine.device.type != 'cuda' or self.pending or cap * self.engine._FIT_SLOTS > (1 << 30):
            return 0
        cursor = self.stream.cursor()
        try:
            self.engine.fit_dense(self.drawahead, cursor, B, m.corruption_level, cap, first_step, n_steps, m._loss_name, m.loss_targets)
        finally:                                        # (what the call consumed of the streams, also when it raised)
            self.stream.set_cursor(cursor)
        return n_steps

    def close(self):            # (draws an early-stopped fit() left in flight included; the handle points at the generators: it goes first)
        if self.drawahead:
            self._drain_draws()
            self._L.drx_drawahead_destroy(self.drawahead)
        self.drawahead, self.pending = None, []
        self.stream.close()


class SampledTrainer:
    """mode='sampled' on one GPU: the sampled (uid, iid, value) triple selects ONE output unit; the constructor's sparse rule touches
    only the rows involved; corruption comes from a counter-based mask evaluated on the device (the MT19937 stream serves the
    _predict_batch compatibility hook alone)."""

    def __init__(self, model, learning_rate, neg_ratio, reg_rate, kwds):
        self.m = weakref.proxy(model)
        self.engine, self.sampler, self.stream = _single_gpu(model, model.sparse_optimizer, learning_rate, neg_ratio, reg_rate, kwds)
        self.on_device = bool(model.device_sampler)     # draw the triples on the GPU (counter-based stream), inside SampledPipeline
        self.pipeline = None

    def configure_optimizer(self, optimizer, forced):
        kind = getattr(optimizer, 'kind', None)
        if not forced:                                  # (the constructor's `sparse_optimizer` unless `optimizer=` forces another of ITS kinds)
            return
        if kind not in ('adam', 'adagrad', 'rowwise_adagrad'):
            raise Exception(f'CDAE mode="sampled" has no sparse {kind} step (got {optimizer!r}): choose CDAE(sparse_optimizer=...) among '
                            f"'adagrad', 'adam', 'rowwise_adagrad', or train with mode=\"reference\", whose dense step takes sgd and rmsprop")
        _push_optimizer(self.engine, optimizer)

    def sample(self, batch_size, **kwds):
        if self.on_device:
            from ..engine import SampledPipeline
            m = self.m
            return _pipeline_token(self, batch_size, lambda first: SampledPipeline(
                self.engine, batch_size, self.sampler.neg_ratio, m.corruption_level, *m.row_seeds(m._mask_seed, 0, 1, first), loss=m._loss_name))
        # (uid, iid, value, is_negative) numpy arrays, or the list of (uid, iid, value) like the reference
        return self.sampler.sample_arrays(batch_size) if kwds.get('as_arrays', True) else self.sampler.sample(batch_size)

    def step(self, batch, step, want_loss):
        if self.on_device:                                      # batch drawn and indexed ahead of time on the device
            return _pipeline_step(self.pipeline, want_loss)
        m = self.m
        uid, iid, val = m._batch_arrays(batch)
        y = (val >= m.interaction_threshold).astype(np.float32)
        bt, alive = self.engine.make_batch(uid, iid, y, q=m.corruption_level, mask_seed=m._mask_seed + 0x9E3779B9 * (step + 1))
        loss = self.engine.step_sparse(step, bt, m._loss_name, want_loss=want_loss)
        return float(loss[0].item()) if want_loss else None

    def run_steps(self, first_step, n_steps, batch_size):
        return 0

    def close(self):
        self.pipeline = None
        self.stream.close()


class ShardedTrainer:
    """mode='sampled' with the device sampler as one process of a multi-GPU job.  layout='rows': this rank keeps the V rows, histories
    and recorded pairs of its user range and the item rows of its item range, and draws `batch_size` triples of ITS users per step;
    'columns': every rank all rows x K / world columns and the same global batch.  No corruption stream: the mask is counter-based."""

    def __init__(self, model, rank, world, learning_rate, neg_ratio, reg_rate, kwds):
        import torch.distributed as dist
        from ..dist import ColumnShardedCdae, ShardedCdae
        if kwds.get('epoch_callback_fn') is not None or kwds.get('early_stopping_rule') is not None:
            raise Exception('epoch callbacks / early stopping need the whole model at every call: not available while it is sharded')
        self.m, self.rows = weakref.proxy(model), model.layout == 'rows'
        ds, U, N, K = model.interaction_dataset, model.n_users, model.n_items, model.hidden_factors
        ip, idx = model._hist_indptr, model._hist_indices = ds.positives_csr(model.interaction_threshold)
        seed = model.seed if model.seed is not None else 0
        lo, hi = U * rank // world, U * (rank + 1) // world

        def mine(indptr, cols):                         # rows: the CSR of users [lo, hi)
            if indptr is None or not self.rows:
                return indptr, cols
            indptr = np.asarray(indptr, np.int64)
            return indptr[lo:hi + 1] - indptr[lo], cols[indptr[lo]:indptr[hi]]
        how = dict(chunks=model.exchange_chunks, transport='rccl' if (model.exchange_transport == 'rccl' and dist.get_backend() == 'nccl') else None) \
            if self.rows else dict(prepare=kwds.get('prepare', 'turns' if world >= 4 else 'local'))     # who sorts the touch lists: dist.py
        self.model = (ShardedCdae if self.rows else ColumnShardedCdae)(
            U, N, K, rank, world, model.device, *mine(ip, idx), seed=seed, lr=learning_rate, reg=reg_rate, optimizer=model.sparse_optimizer,
            loss=model._loss_name, q=model.corruption_level, cpu_staging=(dist.get_backend() == 'gloo'), **how)
        weights = kwds.get('initial_weights')
        if weights is None and (2 * N + U) * K <= (1 << 26):          # the single-GPU initialisation, sliced (larger: drawn per shard on the device)
            weights = _glorot_like_single_gpu(seed, U, N, K)
        if weights is not None:
            self.model.set_params_global(**weights)
        self.engine = self.model.engine
        self.engine.set_recorded_pairs(*mine(*_recorded_pairs(ds, len(idx))))
        self.sampler = PointSampler(ds, neg_ratio, model.interaction_threshold, model.seed)
        model._mask_seed = int(seed)
        self.pipeline = None

    def configure_optimizer(self, optimizer, forced):
        if forced:
            raise Exception('optimizer= cannot be forced on a sharded fit() (layout="rows" or "columns"): choose the sparse rule with '
                            'CDAE(sparse_optimizer=...) — adagrad, adam or rowwise_adagrad')

    def sample(self, batch_size, **kwds):
        m, dm, neg = self.m, self.model, self.sampler.neg_ratio
        if self.rows:       # seeds that differ by rank (tests replay CDAE.row_seeds); exchanges are issued for steps to come: up to the last one
            return _pipeline_token(self, batch_size, lambda first: dm.pipeline(
                batch_size, neg, *m.row_seeds(m._mask_seed, dm.rank, dm.world, first), n_steps=kwds.get('batches_after', 0) + 1))
        return _pipeline_token(self, batch_size, lambda first: dm.pipeline(batch_size, neg, *m.row_seeds(m._mask_seed, 0, 1, first)))

    def step(self, batch, step, want_loss):
        return _pipeline_step(self.pipeline, want_loss)

    def run_steps(self, first_step, n_steps, batch_size):
        return 0

    def full_params(self):
        return self.model.gather_params_global()

    def close(self):
        self.pipeline = self.model = self.engine = None


def _glorot_like_single_gpu(seed, n_users, n_items, k):       # (CdaeEngine.init_glorot's draws, as host arrays to slice)
    rng = np.random.default_rng(seed)

    def glorot(shape):
        lim = np.sqrt(6.0 / (shape[0] + shape[-1]))       # (fan in + fan out; a bias counts its length twice)
        return rng.uniform(-lim, lim, size=shape).astype(np.float32)
    return dict(W=glorot((n_items, k)), W_=glorot((k, n_items)), V=glorot((n_users, k)), b=glorot((k,)), b_=glorot((n_items,)))
