"""CDAE (Collaborative Denoising Auto-Encoder) on the MI355X engine — constructor, hooks and semantics of the reference
model (DRecPy/Recommender/cdae.py), arithmetic in hand-written HIP kernels behind the C ABI of include/drx.h.

mode='reference' (default) reproduces the reference step exactly: every sampled triple contributes its USER only
(cdae.py:52), the loss runs over ALL output units against the batch-mean target ((B,B,N) Keras broadcast,
cdae.py:78-79), L2/B over the full W, W_, V (cdae.py:81-82), dense Keras Adam with one apply per variable
(recommender_abc.py:328-334), corruption drawn from MT19937 seeded like RecommenderABC._rng, N draws per row
(cdae.py:63) — the stream is generated in C++ (drx_rng_corruption_keep) and is bit-identical to `random.Random(seed)`.

mode='sampled' is the engine's throughput mode (CDAE paper's negative sampling, which the reference skips, cdae.py:5):
the sampled (uid, iid, value) triple selects ONE output unit with target 1[value >= threshold]; sparse Adagrad (or lazy
Adam) touches only the rows involved; corruption comes from a counter-based mask evaluated on the device.

How either mode trains, alone or sharded over several GPUs, and the state that takes, is in cdae_fit.py: _pre_fit picks one trainer.
"""
import numpy as np

from . import cdae_fit
from .recommender_abc import RecommenderABC


class CDAE(RecommenderABC):
    fused_fit = True      # reference mode: fit() runs its quiet loop inside the library (_run_steps); False = always step by step

    def __init__(self, hidden_factors=50, corruption_level=0.2, loss='bce', mode='reference', loss_targets='reference',
                 sparse_optimizer='adagrad', device_sampler=False, device='cuda:0', layout='rows', exchange_chunks=2, exchange_transport='rccl', **kwds):
        super().__init__(**kwds)
        if layout not in ('rows', 'columns'):
            raise Exception(f'Unknown multi-GPU layout "{layout}" (supported: "rows", "columns").')
        # how a sampled, device-sampled fit() under a torch.distributed process group shards the model (drecpy_amd/dist.py):
        #   'rows'    north_star / BASELINE configuration 4 — V rows, histories and samples by user range, item rows by item range, the
        #             rows a batch needs and their merged gradients exchanged by all-to-all(v) in `exchange_chunks` pipelined chunks;
        #             every rank draws `batch_size` triples of ITS users per step (global batch = world x batch_size);
        #   'columns' every rank all rows x K / world columns, the same global batch on every rank, one all-reduce of B floats.
        # exchange_transport (rows): 'rccl' = the library's own RCCL communicator, the exchanges of a step issued from C
        #             (include/drx.h drx_comm_*, drx_shard_phase_*) — under an "nccl" process group, where librccl opens on every rank;
        #             'torch' = torch.distributed.all_to_all_single call by call (always under gloo).
        if exchange_transport not in ('rccl', 'torch'):
            raise Exception(f'Unknown exchange transport "{exchange_transport}" (supported: "rccl", "torch").')
        self.layout, self.exchange_chunks, self.exchange_transport = layout, int(exchange_chunks), exchange_transport
        self.hidden_factors = hidden_factors
        self.corruption_level = corruption_level
        if loss not in ('mse', 'bce'):
            raise Exception(f'Loss function "{loss}" is not supported. Supported losses: "mse", "bce".')
        if mode not in ('reference', 'sampled'):
            raise Exception(f'Unknown mode "{mode}" (supported: "reference", "sampled").')
        self._loss_name = loss
        self.mode = mode
        self.loss_targets = loss_targets
        self.sparse_optimizer = sparse_optimizer
        self.device_sampler = device_sampler      # sampled mode: draw the triples on the GPU (counter-based stream)
        self.device = device

    # ---- multi-GPU: the same fit() under an initialised torch.distributed process group ------------------------------------
    def _world(self):
        """(rank, world) when this fit() is one process of a multi-GPU job, else None.  Sampled mode with the device sampler
        trains sharded (drecpy_amd/dist.py: ShardedCdae for layout='rows', ColumnShardedCdae for 'columns'): every process is given
        the SAME dataset and seed; afterwards every process assembles the whole model and predicts / ranks on its own like a
        single-GPU model."""
        import torch.distributed as dist
        if not (self.mode == 'sampled' and self.device_sampler and dist.is_available() and dist.is_initialized()):
            return None
        return (dist.get_rank(), dist.get_world_size()) if dist.get_world_size() > 1 else None

    def fit(self, interaction_dataset, epochs=50, batch_size=32, learning_rate=0.001, neg_ratio=5, reg_rate=0.001,
            copy_dataset=False, **kwds):
        out = super().fit(interaction_dataset, epochs=epochs, batch_size=batch_size, learning_rate=learning_rate, neg_ratio=neg_ratio,
                          reg_rate=reg_rate, copy_dataset=copy_dataset, **kwds)
        if isinstance(self._trainer, cdae_fit.ShardedTrainer):      # training is over: every rank keeps the whole model
            full = self._trainer.full_params()
            self._close_trainer()
            self._restore_engine(full)
        return out

    # ---- cdae.py:34-45 ---------------------------------------------------------------------------
    _trainer = None       # how this fit() trains, and all the state of that: one of cdae_fit's three trainers

    def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
        self._close_trainer()                                        # (the previous fit()'s: draws an early stop left in flight included)
        world = self._world()
        if world is not None:
            t = cdae_fit.ShardedTrainer(self, world[0], world[1], learning_rate, neg_ratio, reg_rate, kwds)
        elif self.mode == 'reference':
            t = cdae_fit.ReferenceTrainer(self, learning_rate, neg_ratio, reg_rate, kwds)
        else:
            t = cdae_fit.SampledTrainer(self, learning_rate, neg_ratio, reg_rate, kwds)
        self._trainer, self._engine, self._sampler = t, t.engine, t.sampler
        self._register_tables()

    @property
    def _dist_model(self):      # the sharded model while a sharded fit() trains, else None (tests ask whether one was built)
        return getattr(self._trainer, 'model', None)

    def _close_trainer(self):
        t, self._trainer = self._trainer, None
        if t is not None:
            t.close()

    def __del__(self):
        try:
            self._close_trainer()
        except Exception:
            pass

    def _register_tables(self):
        """cdae.py:35-43: the five variables, registered in the order W, W_, V, b, b_ (their Adam counters: t = 5*step + j + 1).
        The handles are views over the engine's tables (W_ is stored transposed, one output unit per row)."""
        from .trainables import Variable
        e = self._engine
        self.W, self.W_, self.V, self.b, self.b_ = (Variable.over(t, n) for t, n in zip(e.tables(), ('W', 'W_', 'V', 'b', 'b_')))
        self._register_trainables([self.W, self.W_, self.V, self.b, self.b_])

    def _fused_trainables(self):
        return [self.W, self.W_, self.V, self.b, self.b_]

    # ---- the reference's training hooks: methods here because subclasses override them, work in the trainer (cdae_fit.py) --------
    def _configure_optimizer(self):
        self._trainer.configure_optimizer(self.optimizer, self._optimizer_forced)

    def _sample_batch(self, batch_size, **kwds):       # cdae.py:47
        return self._trainer.sample(batch_size, **kwds)

    def _do_batch(self, batch_samples, step=0, want_loss=False, **kwds):
        return self._trainer.step(batch_samples, step, want_loss)

    def _run_steps(self, first_step, n_steps, batch_size, **kwds):
        """fit()'s quiet path: the trainer's own loop over the remaining epochs (ReferenceTrainer.run_steps: one library call), when these
        very hooks would have run — a subclass or an instance that replaces _sample_batch or _do_batch gets the per-step loop.
        Returns the steps done."""
        if not getattr(self, 'fused_fit', True) or n_steps < 1:
            return 0
        for hook in ('_sample_batch', '_do_batch'):
            if hook in self.__dict__ or getattr(type(self), hook) is not getattr(CDAE, hook):
                return 0
        with self._device_lock:
            return self._trainer.run_steps(first_step, n_steps, batch_size)

    def _restore_engine(self, params):
        from ..engine import CdaeEngine
        self._engine = CdaeEngine(self.n_users, self.n_items, self.hidden_factors, device=self.device)
        self._engine.set_params(**params)
        ip, idx = self.interaction_dataset.positives_csr(self.interaction_threshold)
        self._hist_indptr, self._hist_indices = ip, idx
        self._engine.set_history(ip, idx)

    @staticmethod
    def row_seeds(mask_seed, rank, world, first=0):
        """(sample seed, corruption-mask seed) of step s on rank `rank` of a row-sharded fit"""
        return (lambda s: (mask_seed * 7919 + first + s + 1) * world + rank,
                lambda s: (mask_seed + 0x9E3779B9 * (first + s + 1)) * world + rank)

    # ---- what the trainers' steps and the compatibility hooks share -----------------------------------------------------
    def _batch_arrays(self, batch_samples):
        if isinstance(batch_samples, tuple) and len(batch_samples) == 4 and hasattr(batch_samples[0], 'dtype'):
            return batch_samples[0], batch_samples[1], batch_samples[2]
        u = np.array([s[0] for s in batch_samples], dtype=np.int32)
        i = np.array([s[1] for s in batch_samples], dtype=np.int32)
        v = np.array([float(s[2]) for s in batch_samples], dtype=np.float64)
        return u, i, v

    def _corruption_keep(self, uid, gen=0, at=None, out=None):
        """MT19937 corruption stream of cdae.py:63 for the batch rows: cdae_fit.CorruptionStream.keep"""
        return self._trainer.stream.keep(uid, gen, at, out)

    # ---- hooks kept for API compatibility (cdae.py:50-82) ---------------------------------------------------
    def _predict_batch(self, batch_samples, **kwds):
        """Training-mode reconstructions of the batch users: (predictions [B,N] device tensor, desired [B,N] uint8)."""
        uid, _, _ = self._batch_arrays(batch_samples)
        keep_off, keep = self._corruption_keep(uid)
        with self._device_lock:
            _, pred = self._engine.forward(uid, keep_off=keep_off, keep=keep, q=self.corruption_level)
        desired = np.zeros((len(uid), self.n_items), dtype=np.uint8)
        for b, u in enumerate(uid):
            desired[b, self._hist_indices[self._hist_indptr[u]:self._hist_indptr[u + 1]]] = 1
        return pred, desired

    def _compute_batch_loss(self, predictions, desired_values, **kwds):
        """Keras BCE / MSE of the reference on the (B,B,N) broadcast == against the batch-mean target (cdae.py:78-79)."""
        # (an API-compatibility hook — the fused step computes the training loss itself: host numpy, no device arithmetic in torch)
        p = np.asarray(predictions.cpu().numpy() if hasattr(predictions, 'cpu') else predictions, dtype=np.float64)
        t = np.asarray(desired_values, dtype=np.float64)
        tbar = t.mean(axis=0, keepdims=True)
        if self._loss_name == 'bce':
            eps = 1e-7
            pc = np.clip(p, eps, 1 - eps)
            return float((-(tbar * np.log(pc + eps) + (1 - tbar) * np.log(1 - pc + eps))).mean())
        return float((((p - tbar) ** 2) + tbar * (1 - tbar)).mean())

    def _compute_reg_loss(self, reg_rate, batch_size, trainable_models=None, trainable_layers=None, trainable_weights=None, **kwds):
        e = self._engine                                   # cdae.py:81-82
        from .. import _lib
        return _lib.sumsq([e.W, e.W2T, e.V]) * 0.5 * reg_rate / batch_size

    # ---- inference (cdae.py:67-71, 84-103) -----------------------------------------------------------------
    def _predict(self, uid, iid=None, **kwds):
        if uid is None:
            return None
        with self._device_lock:
            _, pred = self._engine.forward(np.array([uid], dtype=np.int32))
            row = pred[0].cpu().numpy()
        return row if iid is None else row[iid]

    def _rank(self, uid, iids, n, novelty):
        """Top-n of the candidates by (prediction, iid) — heapq.nlargest order (cdae.py:90-103) — on the device."""
        return self._rank_rows([uid], [iids], n, novelty)[0]

    def _rank_rows(self, uids, iid_lists, n, novelty):
        """_rank for many users in one engine call: row r holds the top-n of the candidates iid_lists[r] for the internal user uids[r]."""
        cand = self._candidate_rows(iid_lists)
        if novelty:
            for r, uid in enumerate(uids):
                cand[r, self._all_user_items(uid)] = False        # every (uid, iid) row of the frame, whatever its value
        return self._topk_of_candidates(cand, n, lambda: self._engine.forward(np.asarray(uids, dtype=np.int32))[1])

    def _recommend_batch(self, uids, n, novelty):
        """Top-n of the whole catalogue for many users in one engine call (CdaeEngine.recommend: scores and selection fused on the
        device, no score matrix).  Excluded under novelty: every (uid, iid) row of the frame whatever its value — the set
        _all_user_items gives _rank."""
        return self._recommend_batch_fused(uids, n, novelty)

    def _catalogue_ranks(self, uids, iids, novelty):
        """Catalogue ranks of many (user, item) pairs in one engine call (CdaeEngine.rank_items: scores and counting fused on the
        device), on _recommend_batch's arithmetic and exclusions.  Rows wider than the fused domain: one _recommend per user."""
        if not self._engine.rank_is_fused(self._engine.ld):
            return super()._catalogue_ranks(uids, iids, novelty)
        return self._catalogue_ranks_fused(uids, iids, novelty)

    def _predict_pairs(self, uids, iids):
        """Predictions of many (user, item) pairs in one engine call (CdaeEngine.pair_scores: the hidden row of every distinct user
        once, then two rows per pair — no forward over the catalogue, no [n_items] row downloaded per pair), on _recommend_batch's
        arithmetic: a value may differ from predict()'s in the last ulp.  Any K (the pair scorer has no 256-float limit).  A subclass
        with its own _predict keeps its arithmetic — one _predict per pair."""
        if type(self)._predict is not CDAE._predict:
            return super()._predict_pairs(uids, iids)
        return self._predict_pairs_fused(uids, iids)

    def _all_user_items(self, uid):
        if not hasattr(self, '_user_items'):
            ds = self.interaction_dataset
            order = np.argsort(ds._cols['uid'], kind='stable')
            self._ui_sorted = ds._cols['iid'][order].astype(np.int64)
            self._ui_ptr = np.searchsorted(ds._cols['uid'][order], np.arange(self.n_users + 1))
            self._user_items = True
        return self._ui_sorted[self._ui_ptr[uid]:self._ui_ptr[uid + 1]]
