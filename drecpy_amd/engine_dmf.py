"""Device-side state of one DMF model and the calls into libdrx.so (drx_dmf_*, drx_scatter_rows, drx_adam_*,
drx_score_pairs_bf16).

One training step = the body of the reference fit() loop for DMF (recommender_abc.py:190-204 over dmf.py:64-99):
  drx_dmf_fwd_bwd       both towers, cosine, clip, Keras BCE, backward -> dz0 row per distinct id + small grads
  drx_dmf_k0_update     first-layer kernel gradients (embedding-bag backward) + Keras l2 + dense Adam on both kernels in one walk
                        over the interaction matrix (user_nn t = 2s+1, item_nn t = 2s+2), deterministic
  drx_adam_segments     deeper kernels and all biases
(first_layer_update == 'scatter', for matrices too large to walk every step: touches from drx_dmf_fwd_bwd -> drx_scatter_rows x2
-> drx_adam_dense x2 instead of drx_dmf_k0_update)

`bind_prediction_scale(variable)` adds the ModifiedDMF extension of examples/extending_recommender_dmf.py:9-18 to the fused
step: one registered scalar multiplies every prediction, the loss becomes Keras' (B,B) broadcast (= BCE against the batch-mean
target) and the step makes three Adam applies, the scalar first (recommender_abc.py:194-196,328-334).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import AdamSegments, DmfArgs, DmfDims, DmfK0Update, check, lib, ptr, stream_ptr
from ._staging import StagedUpload
from .engine_dense import DenseEngine, aligned_offsets
from .engine_rows import _round_up


class DmfEngine(DenseEngine):
    def __init__(self, n_users, n_items, user_factors=(64, 32), item_factors=(64, 32), l2_norm_vectors=True, device='cuda:0'):
        if not torch.cuda.is_available():
            raise _lib.DrxError('drecpy_amd needs a ROCm GPU (MI355X); there is no CPU fallback.')
        lib()
        self.device = torch.device(device)
        self.U, self.N = n_users, n_items
        self.n_users, self.n_items = int(n_users), int(n_items)      # (RowsRecommender's names)
        self.factors = [list(user_factors), list(item_factors)]
        if not all(1 <= len(f) <= 4 and 1 <= min(f) and max(f) <= 128 for f in self.factors):
            raise _lib.DrxError(f'DMF engine: towers of 1..4 layers of width 1..128 are supported (a lane of one wavefront holds hidden units '
                                f'k and k + 64), got user_factors={self.factors[0]}, item_factors={self.factors[1]}')
        # floats per row of the per-sample work rows and of the representations predict() hands out: 64 per unit slot of a lane
        self.W = 128 if max(max(f) for f in self.factors) > 64 else 64
        D = DmfDims()
        self.seg = []                      # (name, start, len, regularised, tower)
        off = 0
        for tw, pre in ((0, 'u'), (1, 'i')):
            f = self.factors[tw]
            D.n_layers[tw] = len(f)
            D.ld0[tw] = _round_up(f[0], 4)
            for l, fl in enumerate(f):
                D.f[tw][l] = fl
                if l >= 1:
                    D.off_k[tw][l] = off
                    self.seg.append((f'{pre}{l}_k', off, f[l - 1] * fl, True, tw)); off += _round_up(f[l - 1] * fl, 4)
                D.off_b[tw][l] = off
                self.seg.append((f'{pre}{l}_b', off, fl, False, tw)); off += _round_up(fl, 4)
        self._scale_slot = off                 # reserved for a registered prediction scale (bind_prediction_scale); unused: 1.0, no gradient
        off += 4
        D.n_small = off
        D.l2_norm_vectors = 1 if l2_norm_vectors else 0
        D.off_scale = -1
        self.D = D
        self.scale_var = None
        self.broadcast_targets = False
        z = dict(dtype=torch.float32, device=self.device)
        self.K0u = torch.zeros(n_items, D.ld0[0], **z)
        self.K0i = torch.zeros(n_users, D.ld0[1], **z)
        self.sw = torch.zeros(off, **z)
        self._init_optimizer_state()
        nu, ni = self.K0u.numel(), self.K0i.numel()
        self._g_arena = torch.zeros(nu + ni, **z)            # both dense gradient tables: one buffer, one fill per step
        self._g = {'K0u': self._g_arena[:nu].view(self.K0u.shape), 'K0i': self._g_arena[nu:].view(self.K0i.shape)}
        self._scratch = None
        self.lr, self.reg = 1e-3, 1e-3
        # how the first-layer kernels are updated (set_interactions decides): 'scan' = drx_dmf_k0_update, one walk over all non-zeros
        # per step; 'scatter' = touches -> drx_scatter_rows -> drx_adam_dense, for matrices too large to walk every step
        self.first_layer_update = 'scan'
        self._maps = (torch.zeros(n_users, dtype=torch.int64, device=self.device), torch.zeros(n_items, dtype=torch.int64, device=self.device))
        self._stamp = 0
        self._stage = StagedUpload(self.device)             # host-prepared batches: one upload each, into device buffers the ring keeps
        self._dev_ring, self._dev_i = {}, 0                 # device-prepared batches: (B, k) -> ring slot (prepare_batch_device)
        from .Recommender.trainables import TrainableModel
        # what DMF._pre_fit registers (dmf.py:60): the two Sequential towers, each one apply_gradients per step
        self.user_nn = TrainableModel('user_nn', lambda: self._tower_weights(0))
        self.item_nn = TrainableModel('item_nn', lambda: self._tower_weights(1))

    def _tower_weights(self, tw):
        out = [(self.K0u, self.K0i)[tw][:, :self.factors[tw][0]]]
        for name, start, n, _, t in self.seg:
            if t == tw:
                out.append(self.sw[start:start + n])
        return out

    def bind_prediction_scale(self, variable, broadcast_targets=True):
        """Every prediction of the fused step (and of predict / score_matrix_bf16) is multiplied by `variable` (a registered scalar
        Variable), whose gradient and Adam update the step then also computes.  broadcast_targets: the loss is Keras' (B,B)
        broadcast of (B,) targets against (B,1) predictions — what ModifiedDMF's list of (1,)-tensors produces."""
        if variable.tensor.numel() != 1:
            raise _lib.DrxError('the prediction scale is one scalar')
        self.sw[self._scale_slot:self._scale_slot + 4].zero_()
        variable._rebind(self.sw[self._scale_slot:self._scale_slot + 1])
        variable._consumed_by = self
        self.D.off_scale = self._scale_slot
        self.scale_var = variable
        self.broadcast_targets = bool(broadcast_targets)
        for slot in self.state['sw']:
            if slot is not None:
                slot.fill_(self._slot_init)

    def tensors(self):
        return {'K0u': self.K0u, 'K0i': self.K0i, 'sw': self.sw}

    def set_interactions(self, csr, csc):
        """csr / csc = (indptr int64, indices, values) of the [U,N] interaction matrix and of its transpose, raw values."""
        d = self.device
        mk = lambda t: (torch.as_tensor(np.asarray(t[0], np.int64)).to(d), torch.as_tensor(np.asarray(t[1], np.int32)).to(d),
                        torch.as_tensor(np.asarray(t[2], np.float32)).to(d))
        self.csr, self.csc = mk(csr), mk(csc)
        self._h_indptr = (np.asarray(csr[0], np.int64).copy(), np.asarray(csc[0], np.int64).copy())   # host copies: batch offsets
        # (the scan update gives a quarter-wave to a first-layer gradient row: rows of up to 64 floats)
        self.first_layer_update = 'scan' if len(csr[1]) <= self.SCAN_MAX_NNZ and max(self.D.ld0[0], self.D.ld0[1]) <= 64 else 'scatter'
        # the l2 normaliser of every row / column depends on the dataset alone: once here, not per batch id and step
        self._rho = (torch.empty(self.U, dtype=torch.float32, device=d), torch.empty(self.N, dtype=torch.float32, device=d))
        for (ip, _, vals), n, out in ((self.csr, self.U, self._rho[0]), (self.csc, self.N, self._rho[1])):
            check(lib().drx_dmf_norms(C.byref(self.D), ptr(ip), ptr(vals), n, ptr(out), stream_ptr(self.device)), 'drx_dmf_norms')

        # drx_dmf_k0_update: row n of K0u (an item) walks COLUMN n of the matrix, row u of K0i (a user) walks ROW u; the longest walks
        # first (include/drx.h DrxDmfK0Update::row_order) — static per dataset
        walk = np.concatenate([np.diff(self._h_indptr[1]), np.diff(self._h_indptr[0])])
        # segment length of the gather's work items: 1024 non-zeros, more where the longest row / column would need over 255 segments
        self._seg_len = max(1024, -(-int(walk.max() if len(walk) else 0) // 255))
        self._k0_order = torch.as_tensor(np.argsort(-walk, kind='stable').astype(np.int32)).to(d)
        self._k0_long = int((walk > 1024).sum())            # (csrc/drx_dmf.hip kK0WaveMax: longer walks take a workgroup, the others a wave)

    SCAN_MAX_NNZ = 1 << 25      # 32 M non-zeros = 0.5 GB walked per step: beyond that the touches of a batch are the smaller job

    def set_params(self, p):
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(self.device)
        keep_scale = float(self.sw[self._scale_slot].item()) if self.scale_var is not None else None
        for x in self.tensors().values():
            x.zero_()
        if self.scale_var is not None:        # ('extra_w' before a scale is bound is left to the binder: ModifiedDMF assigns it afterwards)
            self.sw[self._scale_slot] = float(np.asarray(p['extra_w']).reshape(-1)[0]) if 'extra_w' in p else keep_scale
        self.K0u[:, :self.factors[0][0]] = t(p['u0_k'])
        self.K0i[:, :self.factors[1][0]] = t(p['i0_k'])
        for name, start, n, _, _ in self.seg:
            self.sw[start:start + n] = t(p[name]).reshape(-1)

    def get_params(self):
        c = lambda x: x.detach().cpu().numpy().copy()
        p = {'u0_k': c(self.K0u[:, :self.factors[0][0]]), 'i0_k': c(self.K0i[:, :self.factors[1][0]])}
        for name, start, n, _, tw in self.seg:
            v = c(self.sw[start:start + n])
            if name.endswith('_k'):
                l = int(name[1])
                v = v.reshape(self.factors[tw][l - 1], self.factors[tw][l])
            p[name] = v
        if self.scale_var is not None:
            p['extra_w'] = c(self.sw[self._scale_slot:self._scale_slot + 1])
        return p

    def _step_sizes(self, step_idx, applies):
        """the step size of each apply of step `step_idx`: Keras Adam's lr_t of its counter; the learning rate under every other rule"""
        if self.opt_kind != 'adam':
            return [self.lr if j is not None else 0.0 for j in applies[1:]]
        return [self.adam_alpha(self.lr, applies[0] * step_idx + j + 1, self.beta1, self.beta2) if j is not None else 0.0 for j in applies[1:]]

    def _base_args(self, uid, iid, B):
        """DrxDmfArgs with the parameters, both orientations of the matrix and the B (user, item) ids at the addresses uid / iid"""
        A = DmfArgs()
        A.K0u, A.K0i, A.sw = self.K0u.data_ptr(), self.K0i.data_ptr(), self.sw.data_ptr()
        A.u_indptr, A.u_indices, A.u_values = (t.data_ptr() for t in self.csr)
        A.i_indptr, A.i_indices, A.i_values = (t.data_ptr() for t in self.csc)
        A.uid, A.iid, A.B = uid, iid, int(B)
        return A

    def _scatter(self, keys, T, src, src_index, coef, ld, n_rows, out):
        """`out` must already be zero (step() clears the gradient arena once)."""
        if T == 0:
            return
        need = lib().drx_scatter_scratch_bytes(ld, T, n_rows)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(int(need * 1.2) + 1024, dtype=torch.uint8, device=self.device)
        check(lib().drx_scatter_rows(ptr(keys), T, ptr(src), ptr(src_index), ptr(coef), None, ld, n_rows, ptr(out), None,
                                     ptr(self._scratch), self._scratch.numel(), stream_ptr(self.device)), 'drx_scatter_rows')

    # what a step uploads, in this order, each array 16-byte aligned at a byte offset that depends on the batch size alone
    _BATCH_ARRAYS = ('du', 'di', 'y', 'off_u', 'off_i', 'inv_u', 'inv_i', 'gptr_u', 'gptr_i', 'grows_u', 'grows_i', 'order', 'zseg')
    _ORDER_EXTRA = 4096        # work items beyond one per distinct id (segments of long rows / columns): drx_dmf_work_order's order_cap

    @staticmethod
    def _batch_layout(B):
        lens = (B, B, B, B + 1, B + 1, B, B, B + 1, B + 1, B, B, 2 * B + DmfEngine._ORDER_EXTRA, 2 * B)
        offs, total = aligned_offsets([4 * n for n in lens])
        return offs, lens, total

    @staticmethod
    def host_work_list(off_u, off_i, B, seg_len, order=None, zseg=None):
        """The gather's work list of a host-prepared batch of B samples (host code only: no device, no instance): off_u / off_i =
        int32 prefix sums of the degrees of the batch's distinct users / items (drx_batch_distinct), seg_len = the engine's segment
        length.  The list is CUT (drx_dmf_work_order with seg_len) when all three hold: no id needs more than 255 segments, the
        entries fit the list (2 B + _ORDER_EXTRA), and the partial rows fit _zpart (at most _ORDER_EXTRA: a batch of few distinct
        ids leaves room in the list for more partial rows than that — the entries alone do not bound them).  Otherwise UNCUT (seg_len
        0, one entry per distinct id, no partial row): rare, slower on the long rows, correct all the same.
        Returns (n_work, seg_len in use, n_part, order, zseg); order [2 B + _ORDER_EXTRA] / zseg [2 B] int32 are filled in place when
        given."""
        off_u, off_i = np.ascontiguousarray(off_u, np.int32), np.ascontiguousarray(off_i, np.int32)
        cap = 2 * B + DmfEngine._ORDER_EXTRA
        order = np.empty(cap, np.int32) if order is None else order
        zseg = np.empty(2 * B, np.int32) if zseg is None else zseg
        n_part = C.c_int32(0)
        build = lambda seg: int(lib().drx_dmf_work_order(off_u.ctypes.data, len(off_u) - 1, off_i.ctypes.data, len(off_i) - 1, seg,
                                                         order.ctypes.data, cap, zseg.ctypes.data, C.byref(n_part)))
        seg = int(seg_len)
        n_work = build(seg)
        if seg > 0 and (n_work < 0 or n_part.value > DmfEngine._ORDER_EXTRA):
            seg = 0
            n_work = build(0)
        if n_work < 0:
            check(n_work, 'drx_dmf_work_order')
        return n_work, seg, int(n_part.value), order, zseg

    def prepare_batch(self, uids, iids, y):
        """Host half of a step, free of device work (DMF.fit() runs it on the sampler's worker thread): the distinct users / items of
        the batch (ascending), every sample's index among them, the samples per distinct id as a CSR (samples ascending: the order of
        the gradient sums) and the touch offsets of the distinct ids — drx_batch_distinct, counting through an id -> rank scratch
        instead of a sort — written into ONE host buffer at fixed offsets for ONE asynchronous upload."""
        B = len(uids)
        offs, lens, total = self._batch_layout(B)
        buf = np.empty(total, np.uint8)
        base = buf.ctypes.data
        at = dict(zip(self._BATCH_ARRAYS, offs))
        sc = self.__dict__.setdefault('_distinct_scratch', (np.full(self.U, -1, np.int32), np.full(self.N, -1, np.int32)))
        L_ = lib()
        nd = []
        for t, (ids, n, sfx) in enumerate(((uids, self.U, '_u'), (iids, self.N, '_i'))):
            ids32 = np.ascontiguousarray(ids, dtype=np.int32)
            r = L_.drx_batch_distinct(ids32.ctypes.data, B, n, self._h_indptr[t].ctypes.data, sc[t].ctypes.data, base + at['du' if t == 0 else 'di'],
                                      base + at['inv' + sfx], base + at['gptr' + sfx], base + at['grows' + sfx], base + at['off' + sfx])
            if r < 0:
                check(int(r), 'drx_batch_distinct')
            nd.append(int(r))
        y32 = buf[at['y']:at['y'] + 4 * B].view(np.float32)
        y32[:] = y
        off_u = buf[at['off_u']:at['off_u'] + 4 * (nd[0] + 1)].view(np.int32)
        off_i = buf[at['off_i']:at['off_i'] + 4 * (nd[1] + 1)].view(np.int32)
        # the gather's work items: longest rows / columns first, long ones cut into segments of _seg_len non-zeros (include/drx.h
        # DrxDmfArgs::work_order; uncut when the segments would not fit the list or their partial rows _zpart: host_work_list)
        i32 = lambda name: buf[at[name]:at[name] + 4 * lens[self._BATCH_ARRAYS.index(name)]].view(np.int32)
        n_work, seg, n_part, _, _ = self.host_work_list(off_u, off_i, B, self._seg_len, i32('order'), i32('zseg'))
        return {'buf': buf, 'offs': offs, 'B': B, 'n_du': nd[0], 'n_di': nd[1], 'Tu': int(off_u[-1]), 'Ti': int(off_i[-1]),
                'n_work': n_work, 'seg_len': seg, 'n_part': n_part,
                'y_mean': float(y32.astype(np.float64).mean())}

    # ---- batches drawn and prepared ON THE DEVICE (DMF.fit(device_sampler=True): throughput mode) --------------------------------
    def set_sampler_frame(self, positives, recorded, vmin, vrange):
        """positives = (indptr, indices, values) of the pairs a positive draw may return (interaction >= threshold) with their
        values; recorded = (indptr, indices) of every pair the frame holds (a negative is a pair absent from it) or None when all
        recorded pairs are positives; vmin / vrange: the standardisation of recommender_abc.py:463-465 (vrange 0 = raw values)."""
        d = self.device
        ip, idx, val = positives
        self._pos = (torch.as_tensor(np.asarray(ip, np.int64)).to(d), torch.as_tensor(np.asarray(idx, np.int32)).to(d),
                     torch.as_tensor(np.asarray(val, np.float32)).to(d))
        self._rec = None
        if recorded is not None:
            self._rec = (torch.as_tensor(np.asarray(recorded[0], np.int64)).to(d), torch.as_tensor(np.asarray(recorded[1], np.int32)).to(d))
        self._vstd = (float(vmin), float(vrange))
        self._dev_ring, self._dev_i = {}, 0

    # host-prepared batches: the argument structs of a step cached per slot of the upload ring (False: built anew every step — A/B, tests)
    host_step_cache = True

    # device-prepared batches: the gather's work list (longest rows first, long ones cut into segments) built on the device too — False:
    # one work item per distinct id in their own order (52.6 against 28 us for the gather at B = 4096)
    device_work_order = True

    def _device_seg_len(self):
        """segment length of device-built work lists: the host's, raised until the list cannot overflow its _ORDER_EXTRA spare entries —
        every distinct id brings its own row or column once, so the extra entries are at most 2 nnz / seg_len"""
        nnz2 = int(self.csr[1].numel()) + int(self.csc[1].numel())
        return max(int(self._seg_len), -(-nnz2 // self._ORDER_EXTRA))

    def prepare_batch_device(self, B, neg_ratio, seed, triples=None):
        """One batch drawn by the device PointSampler (drx_point_sample_valued: the reference sampler's distribution, a counter-based
        stream) and prepared there (drx_dmf_batch_distinct_device) on the CURRENT stream — DMF.fit() runs it one step ahead on a side
        stream.  Returns what step() takes in place of prepare_batch()'s host arrays.  A ring of 3 slots per batch size: the stream
        first waits for the step that last read the slot (the slot's `free` event, recorded by step() on ITS stream).  triples: (uid, iid, y) device tensors to prepare INSTEAD of drawing (tests)."""
        from ._lib import History
        L_ = lib()
        k = self._dev_i % 3
        self._dev_i += 1
        slot = self._dev_ring.get((B, k))
        if slot is None:
            i32 = dict(dtype=torch.int32, device=self.device)
            need = int(L_.drx_dmf_distinct_scratch_bytes(B, self.U, self.N))
            slot = self._dev_ring[(B, k)] = {
                'ids': torch.empty(2, B, **i32), 'y': torch.empty(B, dtype=torch.float32, device=self.device),
                'arr': torch.empty(8, B + 4, **i32),          # du, di, inv_u, inv_i, gptr_u, gptr_i, grows_u, grows_i
                'nd': torch.empty(2, **i32), 'y_mean': torch.empty(1, dtype=torch.float32, device=self.device),
                'scratch': torch.empty(need, dtype=torch.uint8, device=self.device),
                # the gather's work list built on the device (drx_dmf_work_order_device): entries, zseg per work index, {entries, partial rows}
                'order': torch.empty(2 * B + self._ORDER_EXTRA, **i32), 'zseg': torch.empty(2 * B, **i32), 'nw': torch.zeros(2, **i32),
                'free': None}
        if slot['free'] is not None:
            torch.cuda.current_stream(self.device).wait_event(slot['free'])
            slot['free'] = None
        st = stream_ptr(self.device)
        uid, iid = slot['ids'][0], slot['ids'][1]
        # everything but the seed and the stream is the same from call to call on a slot: the arguments are built once (at B = 256 the
        # host, not the device, bounds fit(device_sampler=True): profiles/r06_dmf_host_profile_B256.txt)
        call = slot.get('call')
        pos, rec = getattr(self, '_pos', None), getattr(self, '_rec', None)          # (set_sampler_frame; absent when only `triples` are prepared)
        if call is None or call['pos'] is not pos or call['rec'] is not rec:
            a = slot['arr']
            call = slot['call'] = {
                'pos': pos, 'rec': rec, 'draw_out': (ptr(uid), ptr(iid), ptr(slot['y'])),
                'distinct': (ptr(uid), ptr(iid), ptr(slot['y']), B, self.U, self.N, *[ptr(a[r]) for r in range(8)], ptr(slot['nd']),
                             ptr(slot['y_mean']), ptr(slot['scratch']), slot['scratch'].numel())}
            if pos is not None:
                H = History(ptr(pos[0]), ptr(pos[1]))
                R = History(ptr(rec[0]), ptr(rec[1])) if rec is not None else None
                call.update({'H': H, 'R': R, 'draw': (C.byref(H), C.byref(R) if R is not None else None, ptr(pos[2]), self._vstd[0], self._vstd[1],
                                                      self.U, self.N, B)})
        if triples is not None:
            uid.copy_(triples[0]); iid.copy_(triples[1]); slot['y'].copy_(triples[2])
        else:
            check(L_.drx_point_sample_valued(*call['draw'], int(neg_ratio), int(seed) & ((1 << 64) - 1), *call['draw_out'], st),
                  'drx_point_sample_valued')
        check(L_.drx_dmf_batch_distinct_device(*call['distinct'], st), 'drx_dmf_batch_distinct_device')
        if self.device_work_order:
            wo = call.get('order')
            if wo is None or wo[0] != self.csr[0].data_ptr():
                a = slot['arr']
                wo = call['order'] = (self.csr[0].data_ptr(), (ptr(self.csr[0]), ptr(self.csc[0]), ptr(a[0]), ptr(a[1]), ptr(slot['nd']),
                                                                  self._device_seg_len(), ptr(slot['order']), slot['order'].numel(), ptr(slot['zseg']),
                                                                  ptr(slot['nw'])))
            check(L_.drx_dmf_work_order_device(*wo[1], st), 'drx_dmf_work_order_device')
        return {'device': slot, 'B': B}

    def _zpart_ptr(self):
        """the partial rows of the work items of cut rows / columns: one buffer, steps run in order on one stream"""
        zp = getattr(self, '_zpart', None)
        if zp is None:
            zp = self._zpart = torch.empty(self._ORDER_EXTRA + 8, self.W, dtype=torch.float32, device=self.device)
        return zp.data_ptr()

    def _where(self, prep, slot):
        """Where the batch of a step is: the DrxDmfArgs fields that name it, the touches of both sides (scatter update) and whether its
        counts come from the host with every batch.  slot: the ring slot it lies in — of the upload ring (13 arrays in the slot's
        device buffer; n_du, n_di, n_work, seg_len and y_mean are this batch's: _launch sets them) or of the device ring (8 rows,
        the counts, the batch mean and the work list are read on the device; the host's n_du / n_di only size the launches)."""
        B = prep['B']
        if prep.get('device') is None:
            base = slot['dev'].data_ptr()
            f = dict(zip(self._BATCH_ARRAYS, (base + o for o in prep['offs'])))
            f['uid'], f['iid'], f['work_order'], f['zpart'] = f.pop('du'), f.pop('di'), f.pop('order'), self._zpart_ptr()
            return {'B': B, 'host': True, 'fields': f, 'touches': (prep['Tu'], prep['Ti'])}
        a = slot['arr']
        f = dict(zip(('uid', 'iid', 'inv_u', 'inv_i', 'gptr_u', 'gptr_i', 'grows_u', 'grows_i'), (a[r].data_ptr() for r in range(8))))
        f.update(y=slot['y'].data_ptr(), n_du=B, n_di=B, nd_dev=slot['nd'].data_ptr(), y_mean_dev=slot['y_mean'].data_ptr())
        if self.device_work_order and 'order' in slot:
            f.update(work_order=slot['order'].data_ptr(), n_work=slot['order'].numel(), seg_len=self._device_seg_len(),
                     zseg=slot['zseg'].data_ptr(), zpart=self._zpart_ptr(), n_work_dev=slot['nw'].data_ptr())
        return {'B': B, 'host': False, 'fields': f, 'touches': (0, 0)}

    def _build_call(self, where, applies):
        """Everything the library calls of one step take, for a batch at `where`: the argument structs, the work buffers and what keeps
        them alive.  What changes from step to step (the stamp, the step sizes, a host batch's counts) is left to _launch."""
        L_ = lib()
        B, (Tu, Ti) = where['B'], where['touches']
        z = dict(dtype=torch.float32, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        ld0u, ld0i = self.D.ld0[0], self.D.ld0[1]
        # device work buffers of a batch size: steps run in order on one stream, so they are reused from step to step
        wk = getattr(self, '_step_bufs', None)
        if wk is None or wk[0] != B:
            grid = L_.drx_dmf_grid(B)
            wk = self._step_bufs = (B, torch.empty(B, ld0u, **z), torch.empty(B, ld0i, **z), torch.empty(grid, self.D.n_small, **z),
                                    torch.empty(grid, **z), torch.empty(self.D.n_small + 1, **z))
        _, dz0u, dz0i, gpart, lpart, gsw = wk
        f = where['fields']
        A = self._base_args(f['uid'], f['iid'], B)
        for name, value in f.items():
            setattr(A, name, value)
        if self.broadcast_targets and self.scale_var is not None:
            A.target_mode = 1                               # (y_mean: a host batch's from _launch, a device batch's at y_mean_dev)
        A.dz0u, A.dz0i = dz0u.data_ptr(), dz0i.data_ptr()
        A.rho_u, A.rho_i = self._rho[0].data_ptr(), self._rho[1].data_ptr()
        A.gsw_part, A.loss_part = gpart.data_ptr(), lpart.data_ptr()
        need = L_.drx_dmf_work_bytes(B)
        if getattr(self, '_work', None) is None or self._work.numel() < need:
            self._work = torch.empty(int(need) + 1024, dtype=torch.uint8, device=self.device)
        A.work = self._work.data_ptr()
        l2c = 2.0 * self.reg
        sg = AdamSegments()
        sg.n = len(self.seg)
        sg_tw = []                                          # (segment, index of its step size): _launch fills sg.alpha
        for i, (_, start, n, regd, tw) in enumerate(self.seg):
            sg.start[i], sg.len[i], sg.l2_coef[i] = start, n, (l2c if regd else 0.0)
            sg_tw.append((i, tw))
        if self.scale_var is not None:                     # the registered scalar: its own lr_t, no regulariser
            i = sg.n
            sg.n += 1
            sg.start[i], sg.len[i], sg.l2_coef[i] = self._scale_slot, 1, 0.0
            sg_tw.append((i, 2))
        m, v = self.state['sw']
        rule = self._rule()
        up = scatter = None
        if self.first_layer_update == 'scan':
            up = DmfK0Update()
            (mu, vu), (mi, vi) = self.state['K0u'], self.state['K0i']
            up.K0u, up.m_u, up.v_u, up.K0i, up.m_i, up.v_i = (t.data_ptr() if t is not None else None for t in (self.K0u, mu, vu, self.K0i, mi, vi))
            up.opt_kind = rule.kind
            up.n_items, up.n_users = self.N, self.U
            up.row_order, up.n_long = self._k0_order.data_ptr(), self._k0_long
            up.l2_coef, up.beta1, up.beta2, up.eps = l2c, self.beta1, self.beta2, self.eps
            A.map_u, A.map_i = self._maps[0].data_ptr(), self._maps[1].data_ptr()
        else:
            tk_u, ts_u, tc_u = torch.empty(max(Tu, 1), **i32), torch.empty(max(Tu, 1), **i32), torch.empty(max(Tu, 1), **z)
            tk_i, ts_i, tc_i = torch.empty(max(Ti, 1), **i32), torch.empty(max(Ti, 1), **i32), torch.empty(max(Ti, 1), **z)
            A.tkeys_u, A.tsrc_u, A.tcoef_u = tk_u.data_ptr(), ts_u.data_ptr(), tc_u.data_ptr()
            A.tkeys_i, A.tsrc_i, A.tcoef_i = tk_i.data_ptr(), ts_i.data_ptr(), tc_i.data_ptr()
            scatter = ((tk_u, Tu, dz0u, ts_u, tc_u, ld0u, self.N, 'K0u'), (tk_i, Ti, dz0i, ts_i, tc_i, ld0i, self.U, 'K0i'))
        return {'B': B, 'applies': applies, 'host': where['host'], 'A': A, 'up': up, 'sg': sg, 'sg_tw': sg_tw,
                'rule': rule, 'l2c': l2c, 'scatter': scatter, 'gsw': gsw, 'upref': C.byref(up) if up is not None else None,
                'small': (C.byref(self.D), C.byref(A), ptr(gsw), ptr(self.sw), ptr(m), ptr(v), C.byref(sg), C.byref(rule)),
                'keep': (gpart, lpart, dz0u, dz0i)}

    def _cached_call(self, slot, B, applies):
        """the call an earlier step built for the ring slot, if it still holds (fit() at B = 256 is bound by the host's Python, not by the
        75 us of kernels: the structs are built once per slot); else None"""
        c = slot.get('step')
        if c is None or c['B'] != B or c['applies'] != applies or c['key'] != self._step_cache_key():
            return None
        return c

    def _launch(self, c, step_idx, prep):
        """The library calls of one step from a built call: stamp and step sizes refreshed, and a host batch's own counts."""
        L_ = lib()
        A, up, sg = c['A'], c['up'], c['sg']
        stream = stream_ptr(self.device)
        if c['host']:
            A.n_du, A.n_di, A.n_work, A.seg_len = prep['n_du'], prep['n_di'], prep['n_work'], prep['seg_len']
            if A.target_mode == 1:
                A.y_mean = prep['y_mean']
        alpha = self._step_sizes(step_idx, c['applies'])
        for i, tw in c['sg_tw']:
            sg.alpha[i] = alpha[tw]
        if up is not None:
            self._stamp += 1
            A.stamp = self._stamp
        # forward / backward with the small weights' update in the launch that sums their partial gradients (one launch less than
        # drx_dmf_fwd_bwd + drx_adam_segments, the same bits; gsw still holds the gradient and, last, the loss sum; the first-layer
        # update below reads none of the small weights)
        check(L_.drx_dmf_step_small_opt(*c['small'], stream), 'drx_dmf_step_small_opt')
        if up is not None:
            up.alpha_u, up.alpha_i = alpha[0], alpha[1]
            check(L_.drx_dmf_k0_update(c['small'][0], c['small'][1], c['upref'], stream), 'drx_dmf_k0_update')
            return
        self._g_arena.zero_()
        for keys, T, src, src_index, coef, ld, n_rows, name in c['scatter']:
            self._scatter(keys, T, src, src_index, coef, ld, n_rows, self._g[name])
        for tw, name in enumerate(('K0u', 'K0i')):
            p = self.tensors()[name]
            m, v = self.state[name]
            check(L_.drx_opt_dense(ptr(p), ptr(m), ptr(v), ptr(self._g[name]), p.numel(), C.byref(self._rule(alpha[tw])), c['l2c'], stream),
                  'drx_opt_dense')

    def step(self, step_idx, uids, iids=None, y=None, want_loss=False, applies=None):
        """uids, iids, y: the batch (arrays or tensors) — or `uids` = what prepare_batch / prepare_batch_device returned for it.
        applies = (n, j_user, j_item, j_scale): number of apply_gradients calls per step and the positions of user_nn, item_nn
        and the prediction scale among them (the registration order, recommender_abc.py:194-196); default: the reference DMF's
        (2, 0, 1), or (3, 1, 2, 0) with a bound scale."""
        applies = tuple(applies) if applies is not None else (3, 1, 2, 0) if self.scale_var is not None else (2, 0, 1, None)
        if not isinstance(uids, dict):
            if torch.is_tensor(uids) or torch.is_tensor(iids) or torch.is_tensor(y):
                c = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
                uids, iids, y = c(uids), c(iids), c(y)
            uids = self.prepare_batch(uids, iids, y)
        prep = uids
        scan = self.first_layer_update == 'scan'
        dev_slot = prep.get('device')
        if dev_slot is not None:            # drawn and prepared on the device: the distinct counts and the batch mean live there
            if not scan:
                raise _lib.DrxError('device-prepared DMF batches need the scan update of the first-layer kernels (set_interactions chose '
                                    '"scatter": more than SCAN_MAX_NNZ interactions)')
            slot, cached = dev_slot, not want_loss
        else:                               # one asynchronous copy into the device buffer of a slot of the upload ring
            slot, cached = self._stage.upload_kept(prep['buf']), not want_loss and scan and self.host_step_cache
        call = self._cached_call(slot, prep['B'], applies) if cached else None
        if call is None:
            call = self._build_call(self._where(prep, slot), applies)
            if cached:
                call['key'] = self._step_cache_key()        # (now: it names the work buffers _build_call may have made)
                slot['step'] = call
        reg_loss = None
        if want_loss:                       # Keras l2(reg) on the pre-update weights
            reg_loss = self.reg * _lib.sumsq([self.K0u, self.K0i] + [self.sw[start:start + n] for _, start, n, regd, _ in self.seg if regd])
        self._launch(call, step_idx, prep)
        if dev_slot is not None:            # (the ring slot may be drawn into again behind this point: prepare_batch_device waits for it)
            dev_slot['free'] = torch.cuda.Event()
            dev_slot['free'].record(torch.cuda.current_stream(self.device))
        if want_loss:
            return float((call['gsw'][-1] + reg_loss).item())
        return None

    def _step_cache_key(self):
        """what a cached argument struct depends on besides its ring slot: the tensors a set_params / set_interactions / optimizer change
        would replace, and the scalars baked into the structs"""
        w = getattr(self, '_work', None)
        return (self.K0u.data_ptr(), self.sw.data_ptr(), self._maps[0].data_ptr(), self._rho[0].data_ptr(), self.csr[0].data_ptr(),
                self.opt_kind, tuple(s.data_ptr() if s is not None else 0 for n in ('sw', 'K0u') for s in self.state[n]), self._k0_order.data_ptr(),
                self._k0_long,
                w.data_ptr() if w is not None else 0, id(self.D), self.D.off_scale, self.first_layer_update, self.reg, self.beta1, self.beta2,
                self.eps, self.broadcast_targets, self.scale_var is not None, getattr(self, '_step_bufs', (None,))[0])

    def predict(self, uids, iids, want_reps=False, scaled=True):
        """max(1e-6, cosine) for each (uid, iid) pair (dmf.py:88-96) — times the bound prediction scale unless scaled=False;
        optionally the normalised tower outputs [B, self.W]."""
        uid, iid = self._dev_i32(uids), self._dev_i32(iids)
        B = uid.numel()
        pred = torch.empty(B, dtype=torch.float32, device=self.device)
        A = self._base_args(uid.data_ptr(), iid.data_ptr(), B)
        A.pred_out = pred.data_ptr()
        ru = ri = None
        if want_reps:
            ru = torch.empty(B, self.W, dtype=torch.float32, device=self.device)
            ri = torch.empty(B, self.W, dtype=torch.float32, device=self.device)
            A.rep_u_out, A.rep_i_out = ru.data_ptr(), ri.data_ptr()
        D = self.D
        if not scaled and self.D.off_scale >= 0:
            D = DmfDims.from_buffer_copy(self.D)
            D.off_scale = -1
        check(lib().drx_dmf_predict(C.byref(D), C.byref(A), stream_ptr(self.device)), 'drx_dmf_predict')
        return (pred, ru, ri) if want_reps else pred

    def score_matrix_bf16(self, uids):
        """[len(uids), N] cosine scores of the given users against ALL items on the matrix cores (bf16 operands)."""
        uid = self._dev_i32(uids)
        n_u = uid.numel()
        ri = self._representations(1, torch.arange(self.N, dtype=torch.int32, device=self.device))
        ru = self._representations(0, uid)
        pitch = _round_up(self.N, 32)                  # rows of 128-byte lines: a line then belongs to ONE tile of the scorer
        out = torch.empty(n_u, pitch, dtype=torch.float32, device=self.device)
        kdim = _round_up(self.factors[0][-1], 16)
        if kdim > 64:
            raise _lib.DrxError(f'score_matrix_bf16: representations of up to 64 factors (the scorer stages 64-wide bf16 tiles), got {self.factors[0][-1]}')
        scale = ptr(self.sw[self._scale_slot:]) if self.scale_var is not None else None
        check(lib().drx_score_pairs_bf16(ptr(ru), n_u, ptr(ri), self.N, self.W, kdim, scale, ptr(out), pitch, stream_ptr(self.device)),
              'drx_score_pairs_bf16')
        return out[:, :self.N]

    # ---- batched top-n recommendation (include/drx.h drx_rows_recommend, DRX_REC_CLIP) ----------------
    def _representations(self, tower, ids):
        """[len(ids), self.W] l2-normalised outputs of one tower (0 = users, 1 = items) for the device ids `ids`: k_dmf_predict writes
        whole rows, zero beyond the last factor (the scorer multiplies those columns)."""
        B = int(ids.numel())
        other = torch.zeros(B, dtype=torch.int32, device=self.device)       # (a pair needs a partner: id 0 of the other side, unused)
        rep = torch.empty(B, self.W, dtype=torch.float32, device=self.device)
        A = self._base_args(ids.data_ptr(), other.data_ptr(), B) if tower == 0 else self._base_args(other.data_ptr(), ids.data_ptr(), B)
        if tower == 0:
            A.rep_u_out = rep.data_ptr()
        else:
            A.rep_i_out = rep.data_ptr()
        check(lib().drx_dmf_predict(C.byref(self.D), C.byref(A), stream_ptr(self.device)), 'drx_dmf_predict')
        return rep

    # what the four calls of RowsRecommender score against: max(1e-6, cosine) of the towers' outputs — WITHOUT a bound prediction
    # scale.  The item tower is the table: computed when a call asks (nothing is cached across calls: the parameters may have moved),
    # once per call — over the catalogue, in pair_scores over the request's distinct items only; the user tower once per distinct user
    # of a chunk.  Outside the fused domain (n > 128): DrxError — DMF._recommend_batch asks recommend_is_fused first.
    EPILOGUE = _lib.DRX_REC_CLIP
    TABLE_IS_COMPUTED = True

    def rank_ld(self):
        return self.W

    def _score_table(self, items=None):
        return self._representations(1, torch.arange(self.N, dtype=torch.int32, device=self.device) if items is None else items), None

    def _query_rows(self, uid):
        return self._representations(0, uid)
