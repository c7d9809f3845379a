"""Device-side state of one Caser model and the calls into libdrx.so (drx_caser_*, drx_scatter_rows, drx_adam_*).

One training step = the body of the reference fit() loop for Caser (recommender_abc.py:190-204 over caser.py:86-120), three launches:
  drx_caser_step_small      forward, Keras BCE, backward (k_caser_tile: tiles of 16 samples on the matrix cores) -> one gradient row per
                            item / user lookup, the score gradients and hidden rows of the dense_1 lookups, the workgroups' partial sums of
                            the small-weight gradients; then those sums and the conv / dense_0 kernels' and biases' l2 + Keras Adam
  drx_rows_csr_adam_multi   the lookups' rows -> gradient + L2 (Keras l2(reg): 2*reg*w) + Keras Adam of item_emb, user_emb and dense_1_W
                            (+ dense_1_b; its rows formed as score gradient x hidden row where they are summed) in one pass per table, from
                            the lookups grouped by row on the host (drx_batch_csr); one lr_t per registered layer
(table_update == 'scatter', for batches already on the device: drx_scatter_rows x3 into a zeroed gradient arena + drx_adam_dense x4)
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import AdamSegments, CaserArgs, CaserDims, check, lib, ptr, stream_ptr
from ._staging import StagedUpload
from .engine_dense import DenseEngine, aligned_offsets
from .engine_rows import _round_up


class CaserEngine(DenseEngine):
    ACTIVATIONS = {'relu': 0, 'tanh': 1, 'sigmoid': 2, 'linear': 3, None: 3}

    def __init__(self, n_users, n_items, L=5, T=3, neg_ratio=3, d=50, n_v=4, n_h=16, device='cuda:0', act_h='relu', act_mlp='relu'):
        if not torch.cuda.is_available():
            raise _lib.DrxError('drecpy_amd needs a ROCm GPU (MI355X); there is no CPU fallback.')
        lib()
        if not (1 <= L <= 8 and 1 <= d <= 64):
            raise _lib.DrxError(f'Caser engine: 1 <= L <= 8 and 1 <= d <= 64 are supported (lane = embedding channel of one wavefront), got L={L}, d={d}')
        if act_h not in self.ACTIVATIONS or act_mlp not in self.ACTIVATIONS:
            raise _lib.DrxError(f'Caser engine: activations {sorted(k for k in self.ACTIVATIONS if k)} are supported, got act_h={act_h!r}, act_mlp={act_mlp!r}')
        self.device = torch.device(device)
        self.U, self.N, self.L, self.T, self.d, self.n_v, self.n_h = n_users, n_items, L, T, d, n_v, n_h
        self.n_users, self.n_items = int(n_users), int(n_items)      # (RowsRecommender's names)
        self.Tp = T + T * neg_ratio
        self.ld, self.ld2 = _round_up(d, 4), _round_up(2 * d, 4)
        self.nx = n_v + L * n_h
        ld = self.ld
        off = 0
        D = CaserDims()
        D.L, D.T, D.Tp, D.d, D.ld, D.ld2, D.n_v, D.n_h = L, T, self.Tp, d, ld, self.ld2, n_v, n_h
        self.seg = []                    # (name, start, len, regularised, layer index)
        D.off_kv = off; self.seg.append(('conv_v_k', off, L * n_v * ld, True, 2)); off += L * n_v * ld
        D.off_bv = off; self.seg.append(('conv_v_b', off, n_v, False, 2)); off += _round_up(n_v, 4)
        for i in range(L):
            D.off_kh[i] = off; self.seg.append((f'conv_h{i}_k', off, (i + 1) * n_h * ld, True, 3 + i)); off += (i + 1) * n_h * ld
            D.off_bh[i] = off; self.seg.append((f'conv_h{i}_b', off, n_h, False, 3 + i)); off += _round_up(n_h, 4)
        D.off_wd = off; self.seg.append(('dense0_k', off, self.nx * ld, True, 3 + L)); off += self.nx * ld
        D.off_bd = off; self.seg.append(('dense0_b', off, ld, False, 3 + L)); off += ld
        D.n_small = off
        D.act_h, D.act_mlp = self.ACTIVATIONS[act_h], self.ACTIVATIONS[act_mlp]
        self.D = D
        # (the kernels keep a tile's scratch and, where they fit, the small weights in a workgroup's LDS: drx_caser_grid answers 0 when
        #  n_v + L * n_h is too large for that — Recommender/caser.py then takes the generic engine)
        if int(lib().drx_caser_grid(C.byref(D), 16)) < 1:
            raise _lib.DrxError(f'Caser engine: n_v + L * n_h = {self.nx} units (n_v={n_v}, n_h={n_h}, L={L}, d={d}) do not fit the kernels\' LDS tiles')
        self.n_layers = 6 + L
        z = dict(dtype=torch.float32, device=self.device)
        self.item_emb = torch.zeros(n_items, ld, **z)
        self.user_emb = torch.zeros(n_users, ld, **z)
        self.W1 = torch.zeros(n_items, self.ld2, **z)
        self.b1 = torch.zeros(n_items, **z)
        self.sw = torch.zeros(off, **z)
        self._init_optimizer_state()
        # the dense gradient tables of the scatters live in ONE buffer, zeroed by one kernel per step
        scat = [n for n in ('item_emb', 'W1', 'b1', 'user_emb') if n in self.tensors()]
        sizes = [(self.tensors()[n].numel() + 63) // 64 * 64 for n in scat]
        self._grad_arena = torch.zeros(sum(sizes), dtype=torch.float32, device=self.device)
        self._grads, o = {}, 0
        for n, sz in zip(scat, sizes):
            self._grads[n] = self._grad_arena[o:o + self.tensors()[n].numel()].view(self.tensors()[n].shape)
            o += sz
        for n, t in self.tensors().items():
            if n not in self._grads:
                self._grads[n] = torch.zeros_like(t)
        self._scratch = None
        self.lr, self.reg = 1e-3, 1e-3
        self._stage = StagedUpload(self.device)             # host batches: one asynchronous upload each
        self._seg_layers = [layer for (_, _, _, _, layer) in self.seg]      # (whose step size a segment of the small weights takes)
        from .Recommender.trainables import TrainableLayer
        # the 6 + L Keras layers caser.py:47-70 registers, in that order (= the order of the per-step Adam applies)
        seg_views = lambda j: [self.sw[st:st + n] for _, st, n, _, layer in self.seg if layer == j]
        self.layers = [TrainableLayer('user_embeddings', lambda: [self.user_emb]), TrainableLayer('item_embeddings', lambda: [self.item_emb]),
                       TrainableLayer('conv_v', lambda: seg_views(2))]
        self.layers += [TrainableLayer(f'convs_h[{i}]', (lambda i=i: seg_views(3 + i))) for i in range(L)]
        self.layers += [TrainableLayer('dense_0', lambda: seg_views(3 + L)), TrainableLayer('dense_1_W', lambda: [self.W1]),
                        TrainableLayer('dense_1_b', lambda: [self.b1])]

    def tensors(self):
        return {'user_emb': self.user_emb, 'item_emb': self.item_emb, 'W1': self.W1, 'b1': self.b1, 'sw': self.sw}

    # ---- parameters in the reference's layout (oracle/caser_oracle.py:init_params) -----------------------------
    def set_params(self, p):
        d, ld = self.d, self.ld
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(self.device)
        for x in self.tensors().values():
            x.zero_()
        self.user_emb[:, :d] = t(p['user_emb'])
        self.item_emb[:, :d] = t(p['item_emb'])
        self.W1[:, :2 * d] = t(p['W1'])
        self.b1.copy_(t(p['b1']).reshape(-1))
        for name, start, n, _, _ in self.seg:
            if name.endswith('_k') and name.startswith('conv'):
                k = t(p[name]).permute(0, 2, 1).contiguous()            # [s, d, f] -> [s, f, d]
                view = self.sw[start:start + n].view(k.shape[0], k.shape[1], ld)
                view[:, :, :d] = k
            elif name == 'dense0_k':
                self.sw[start:start + n].view(self.nx, ld)[:, :d] = t(p[name])
            elif name == 'dense0_b':
                self.sw[start:start + d] = t(p[name])
            else:
                self.sw[start:start + n] = t(p[name])

    def get_params(self):
        d, ld = self.d, self.ld
        c = lambda x: x.detach().cpu().numpy().copy()
        p = {'user_emb': c(self.user_emb[:, :d]), 'item_emb': c(self.item_emb[:, :d]), 'W1': c(self.W1[:, :2 * d]),
             'b1': c(self.b1).reshape(-1, 1)}
        for name, start, n, _, _ in self.seg:
            if name.endswith('_k') and name.startswith('conv'):
                s_ = n // (ld * (self.n_v if name == 'conv_v_k' else self.n_h))
                f = self.n_v if name == 'conv_v_k' else self.n_h
                p[name] = c(self.sw[start:start + n].view(s_, f, ld)[:, :, :d].permute(0, 2, 1))
            elif name == 'dense0_k':
                p[name] = c(self.sw[start:start + n].view(self.nx, ld)[:, :d])
            elif name == 'dense0_b':
                p[name] = c(self.sw[start:start + d])
            else:
                p[name] = c(self.sw[start:start + n])
        return p

    # ---- helpers --------------------------------------------------------------------------------------------------
    def _scatter(self, keys, T, src, ld, n_rows, out, src_s=None, out_s=None, stream=None):
        """keys / src / src_s / out / out_s: device addresses.  `out` (and `out_s`) must already be zero: step() clears the whole
        gradient arena once."""
        sb = self.__dict__.setdefault('_scatter_need', {})
        need = sb.get((ld, T, n_rows))
        if need is None:
            need = sb[(ld, T, n_rows)] = lib().drx_scatter_scratch_bytes(ld, T, n_rows)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(int(need * 1.2) + 1024, dtype=torch.uint8, device=self.device)
        check(lib().drx_scatter_rows(keys, T, src, None, None, src_s, ld, n_rows, out, out_s, self._scratch.data_ptr(),
                                     self._scratch.numel(), stream if stream is not None else stream_ptr(self.device)), 'drx_scatter_rows')

    def _adam(self, name, grad, alpha, l2c, stream=None):
        p = getattr(self, name)
        m, v = self.state[name]
        check(lib().drx_opt_dense(p.data_ptr(), _lib.ptr(m), _lib.ptr(v), grad.data_ptr(), p.numel(), C.byref(self._rule(alpha)), l2c,
                                  stream if stream is not None else stream_ptr(self.device)), 'drx_opt_dense')

    def _alphas(self, step_idx):
        """Keras-Adam lr_t of the n_layers applies of step `step_idx` (t = n_layers * step + j + 1), fp32 like optimizer_v2/adam.py."""
        f = np.float32
        if self.opt_kind != 'adam':                       # no bias correction: every apply steps by the learning rate
            return [float(self.lr)] * self.n_layers
        t = (self.n_layers * step_idx + 1 + np.arange(self.n_layers)).astype(np.float32)
        return (f(self.lr) * np.sqrt(f(1.0) - np.power(f(self.beta2), t)) / (f(1.0) - np.power(f(self.beta1), t))).astype(np.float32).tolist()

    def _args(self, uid, before, B, after=None):
        """DrxCaserArgs with the parameters and the B windows' ids at the device addresses uid / before / after"""
        A = CaserArgs()
        A.item_emb, A.user_emb, A.W1, A.b1, A.sw = (t.data_ptr() for t in (self.item_emb, self.user_emb, self.W1, self.b1, self.sw))
        A.uid, A.before, A.after, A.B = uid, before, after, int(B)
        return A

    # how the four lookup tables (user / item embeddings, dense_1_W + dense_1_b) are updated: 'csr' = drx_rows_csr_adam, gradient and
    # dense Adam in one pass per table from the lookups grouped by row on the host (prepare_batch); 'scatter' = drx_scatter_rows into
    # a zeroed gradient arena + drx_adam_dense (the only way for batches that are already on the device)
    table_update = 'csr'

    # batches already on the device: group their lookups by table row on the device (True) or take the scatter + dense-Adam update
    device_csr = True

    # ---- batches that are already on the device: rings of three slots ---------------------------------------------------------------
    # A slot holds the lookups of one batch grouped by table row (drx_batch_csr_device: row_ptr / order of the three lists in one buffer)
    # and the event `free` of the step that last read it, recorded by that step on ITS stream: the slot is filled again only behind it.
    # Ring '_dev_csr' (prepare_device_batch) is handed the id tensors of every batch; ring '_dev_slots' (device_slot / group_slot:
    # Caser.fit(device_sampler=True), the sampler writes into them) OWNS them — everything a draw and a step hand to the library is
    # then the same from visit to visit of a slot, and the step's call is built once per slot (at 4096 windows the host's Python, not
    # the 79 us of training kernels, bounded the step: profiles/r06_caser_host_profile.txt).
    def _ring_slot(self, ring, B, ids=None):
        """The next slot of `ring` for a batch of B windows, on the CURRENT stream (which may be a run-ahead stream: nothing here depends
        on the parameters).  ids: the batch's (uid, before, after) int32 device tensors, or None for a ring that owns them."""
        st = self.__dict__.setdefault(ring, {})
        if st.get('B') != B:
            i32 = dict(dtype=torch.int32, device=self.device)
            offs, total = aligned_offsets([4 * n for n in (self.N + 1, B * self.L, self.N + 1, B * self.Tp, self.U + 1, B)])
            st.clear()
            st.update({'B': B, 'i': 0, 'scratch': None, 'slots': []})
            for k in range(3):
                sl = {'k': k, 'B': B, 'buf': torch.empty(total, dtype=torch.uint8, device=self.device), 'free': None, 'own_ids': ids is None}
                sl['csr_dev'] = [sl['buf'].data_ptr() + o for o in offs]                   # ptrE, ordE, ptrW, ordW, ptrU, ordU
                if ids is None:
                    self._slot_ids(sl, torch.empty(B, **i32), torch.empty(B, self.L, **i32), torch.empty(B, self.Tp, **i32))
                st['slots'].append(sl)
        sl = st['slots'][st['i'] % 3]
        st['i'] += 1
        if sl['free'] is not None:
            torch.cuda.current_stream(self.device).wait_event(sl['free'])
            sl['free'] = None
        if ids is not None:
            self._slot_ids(sl, *ids)               # (the tensors stay alive with the slot: beyond the step that reads them)
        return sl

    def _slot_ids(self, sl, uid, bef, aft):
        """the id tensors of the slot's batch and the three lists drx_batch_csr_device groups: item lookups, target lookups, users"""
        B = sl['B']
        ptrE, ordE, ptrW, ordW, ptrU, ordU = sl['csr_dev']
        ls = (_lib.CsrList * 3)()
        for l, (keys, T, n_rows, rp, od) in zip(ls, ((bef, B * self.L, self.N, ptrE, ordE), (aft, B * self.Tp, self.N, ptrW, ordW),
                                                    (uid, B, self.U, ptrU, ordU))):
            l.keys, l.T, l.n_rows, l.row_ptr, l.order = keys.data_ptr(), T, n_rows, rp, od
        sl.update(uid=uid, before=bef, after=aft, lists=ls)

    def _group(self, ring, sl):
        """the lookups of a filled slot grouped by table row (drx_batch_csr_device: one stable sort for the three lists) on the current
        stream; returns the slot: what step() takes"""
        st = self.__dict__[ring]
        if st['scratch'] is None:
            need = int(lib().drx_batch_csr_device_bytes(sl['lists'], 3))
            if need <= 0:
                raise _lib.DrxError('drx_batch_csr_device_bytes: invalid lists')
            st['scratch'] = torch.empty(need, dtype=torch.uint8, device=self.device)
            st['scratch_args'] = (st['scratch'].data_ptr(), st['scratch'].numel())
        check(lib().drx_batch_csr_device(sl['lists'], 3, *st['scratch_args'], stream_ptr(self.device)), 'drx_batch_csr_device')
        return sl

    def prepare_device_batch(self, uid, bef, aft):
        """A batch that is already on the device, its lookups grouped by table row on the CURRENT stream — what step() takes in place of
        (uids, before, after)."""
        uid, bef, aft = self._dev_i32(uid), self._dev_i32(bef), self._dev_i32(aft)
        return self._group('_dev_csr', self._ring_slot('_dev_csr', uid.numel(), (uid, bef, aft)))

    def device_slot(self, B):
        """The next ring slot for a batch of B windows drawn on the device: {'uid', 'before', 'after'} int32 tensors to fill on the CURRENT
        stream (which has been made to wait for the step that last read the slot), then group_slot(slot)."""
        return self._ring_slot('_dev_slots', B)

    def group_slot(self, sl):
        return self._group('_dev_slots', sl)

    def prepare_batch(self, uids, before, after):
        """Host half of a step (Caser.fit() runs it on the sampler's worker thread): the batch as int32 arrays plus, for each of the
        three lookup lists, the lookups grouped by the table row they name (drx_batch_csr) — one host buffer for one upload."""
        B = len(uids)
        L_ = lib()
        sizes = (B, B * self.L, B * self.Tp, self.N + 1, B * self.L, self.N + 1, B * self.Tp, self.U + 1, B)
        offs, total = aligned_offsets([4 * n for n in sizes])
        buf = np.empty(total, np.uint8)
        view = lambda k: buf[offs[k]:offs[k] + 4 * sizes[k]].view(np.int32)
        view(0)[:] = uids
        view(1)[:] = np.asarray(before).reshape(-1)
        view(2)[:] = np.asarray(after).reshape(-1)
        base = buf.ctypes.data
        for keys, T, n_rows, kp, ko in ((1, B * self.L, self.N, 3, 4), (2, B * self.Tp, self.N, 5, 6), (0, B, self.U, 7, 8)):
            check(L_.drx_batch_csr(base + offs[keys], T, n_rows, base + offs[kp], base + offs[ko]), 'drx_batch_csr')
        return {'buf': buf, 'offs': offs, 'B': B}

    # ---- one training step ---------------------------------------------------------------------------------------
    def _call_key(self):
        """what the cached call of a ring slot depends on besides the slot: the tensors a set_params / optimizer change would replace,
        the scalars baked into the structs and the work buffers"""
        return (self.item_emb.data_ptr(), self.sw.data_ptr(), self.opt_kind,
                tuple(s.data_ptr() if s is not None else 0 for n in ('sw', 'W1') for s in self.state[n]), self.reg, self.beta1,
                self.beta2, self.eps, id(self.D), id(self.__dict__.get('_step_bufs')))

    def _build_call(self, ids, csr, B):
        """Everything the library calls of one step take, for B windows whose (uid, before, after) ids lie at the device addresses `ids`:
        the argument structs and the work buffers.  csr: the six addresses of the lookups grouped by table row (ptrE, ordE, ptrW, ordW,
        ptrU, ordU) for the 'csr' update of the tables, None for the 'scatter' update.  What changes from step to step (the dropout
        mask, the step sizes) is left to _launch."""
        z = dict(dtype=torch.float32, device=self.device)
        # dense_1's gradient rows are outer products, score gradient x [dense_0 output | user row]: with the 'csr' update the kernel writes
        # the B hidden rows and drx_rows_csr_adam_outer forms the B * Tp rows where it sums them (19.7 MB less to write and to read back
        # per step of 4096); the 'scatter' update takes them written out
        outer = csr is not None
        n_dE, n_dW1, n_dPu = B * self.L * self.ld, (B if outer else B * self.Tp) * self.ld2, B * self.ld
        # device work buffers of a batch size: steps run in order on one stream, so they are reused from step to step
        wk = getattr(self, '_step_bufs', None)
        if wk is None or wk[0] != (B, outer):
            grid = lib().drx_caser_grid(C.byref(self.D), B)
            rows = torch.zeros(n_dE + n_dW1 + n_dPu, **z)    # the padding columns of the gradient rows stay zero: the kernel never writes them
            wk = self._step_bufs = ((B, outer), rows, torch.empty(B * self.Tp, **z), torch.empty(grid, self.D.n_small, **z), torch.empty(grid, **z),
                                    torch.empty(self.D.n_small + 1, **z))
        _, rows, db1, gpart, lpart, gsw = wk
        base = rows.data_ptr()
        p_dE, p_dW1, p_dPu = base, base + 4 * n_dE, base + 4 * (n_dE + n_dW1)       # (p_dW1: the rows, or the B hidden rows)
        A = self._args(*ids[:2], B, ids[2])
        A.dE, A.db1, A.dPu, A.gsw_part, A.loss_part = p_dE, db1.data_ptr(), p_dPu, gpart.data_ptr(), lpart.data_ptr()
        A.dW1, A.cat_out = (None, p_dW1) if outer else (p_dW1, None)
        l2c = 2.0 * self.reg
        sg = AdamSegments()
        sg.n = len(self.seg)
        for i, (_, start, n, regd, _) in enumerate(self.seg):
            sg.start[i], sg.len[i], sg.l2_coef[i] = start, n, (l2c if regd else 0.0)
        tabs = None
        if outer:
            # the three lookup tables (+ dense_1_b) in one launch: gradient rows summed per table row, l2, the update rule
            ptrE, ordE, ptrW, ordW, ptrU, ordU = csr
            tabs = (_lib.CsrAdamTable * 3)()
            for t, (rp, od, src, scale, group, ld, n_rows, name, sname) in zip(tabs, (
                    (ptrU, ordU, p_dPu, None, 0, self.ld, self.U, 'user_emb', None),
                    (ptrE, ordE, p_dE, None, 0, self.ld, self.N, 'item_emb', None),
                    (ptrW, ordW, p_dW1, db1.data_ptr(), self.Tp, self.ld2, self.N, 'W1', 'b1'))):
                t.row_ptr, t.order, t.src, t.scale, t.group, t.ld, t.n_rows = rp, od, src, scale, group, ld, n_rows
                t.p, (t.m, t.v) = getattr(self, name).data_ptr(), (x.data_ptr() if x is not None else None for x in self.state[name])
                if sname is not None:
                    t.p_s, (t.m_s, t.v_s) = getattr(self, sname).data_ptr(), (x.data_ptr() if x is not None else None for x in self.state[sname])
                t.l2_coef = l2c
        m, v = self.state['sw']
        rule = self._rule()
        return {'A': A, 'sg': sg, 'tabs': tabs, 'bufs': wk, 'rule': rule,
                'small': (C.byref(self.D), C.byref(A), gsw.data_ptr(), self.sw.data_ptr(), ptr(m), ptr(v), C.byref(sg), C.byref(rule)),
                'scatter': None if outer else (ids, (p_dE, p_dW1, p_dPu, db1.data_ptr()), l2c)}

    def _launch(self, c, step_idx, kp, rate, mask_seed, want_loss, slot=None):
        """The library calls of one step from a built call, with this step's dropout (kp: uint8 device keep mask or None), step sizes
        and, if wanted, loss.  slot: the ring slot the batch lies in — its `free` event is recorded behind the step's last launch."""
        L_ = lib()
        A, sg, tabs = c['A'], c['sg'], c['tabs']
        A.keep = kp.data_ptr() if kp is not None else None
        A.rate = float(rate)
        A.mask_seed = int(mask_seed) & (2 ** 64 - 1)
        reg_loss = None
        if want_loss:                                   # Keras l2(reg) on the pre-update weights
            sq = _lib.sumsq([self.user_emb, self.item_emb, self.W1] + [self.sw[start:start + n] for _, start, n, regd, _ in self.seg if regd])
            reg_loss = self.reg * sq
        alpha = self._alphas(step_idx)
        for i, layer in enumerate(self._seg_layers):
            sg.alpha[i] = alpha[layer]
        stream = stream_ptr(self.device)
        # forward / backward, then the small weights' update in the launch that sums the workgroups' partial gradients
        check(L_.drx_caser_step_small_opt(*c['small'], stream), 'drx_caser_step_small_opt')
        if tabs is not None:
            tabs[0].alpha, tabs[1].alpha, tabs[2].alpha, tabs[2].alpha_s = alpha[0], alpha[1], alpha[4 + self.L], alpha[5 + self.L]
            check(L_.drx_rows_csr_opt_multi(tabs, 3, c['small'][7], stream), 'drx_rows_csr_opt_multi')
        else:
            B, g = A.B, self._grads
            (uid_p, bef_p, aft_p), (p_dE, p_dW1, p_dPu, p_db1), l2c = c['scatter']
            self._grad_arena.zero_()
            self._scatter(bef_p, B * self.L, p_dE, self.ld, self.N, g['item_emb'].data_ptr(), stream=stream)
            self._scatter(aft_p, B * self.Tp, p_dW1, self.ld2, self.N, g['W1'].data_ptr(), src_s=p_db1, out_s=g['b1'].data_ptr(), stream=stream)
            self._scatter(uid_p, B, p_dPu, self.ld, self.U, g['user_emb'].data_ptr(), stream=stream)
            self._adam('user_emb', g['user_emb'], alpha[0], l2c, stream)
            self._adam('item_emb', g['item_emb'], alpha[1], l2c, stream)
            self._adam('W1', g['W1'], alpha[4 + self.L], l2c, stream)
            self._adam('b1', g['b1'], alpha[5 + self.L], 0.0, stream)
        if slot is not None:                            # (the ring slot may be filled again behind this point: _ring_slot waits for it)
            slot['free'] = torch.cuda.Event()
            slot['free'].record(torch.cuda.current_stream(self.device))
        if want_loss:
            return float((c['bufs'][5][-1] + reg_loss).item())
        return None

    def _step_slot(self, step_idx, sl, keep, rate, mask_seed, want_loss):
        """step() on a ring slot.  A slot that owns its id tensors keeps the call of its earlier visit (the 'csr' update, no loss
        wanted): only this step's scalars are set."""
        csr = sl['csr_dev'] if self.table_update == 'csr' else None
        cached = sl['own_ids'] and csr is not None and not want_loss
        c = sl.get('step') if cached else None
        if c is None or c['key'] != self._call_key():
            c = self._build_call((sl['uid'].data_ptr(), sl['before'].data_ptr(), sl['after'].data_ptr()), csr, sl['B'])
            if cached:
                c['key'] = self._call_key()                 # (now: it names the work buffers _build_call may have made)
                sl['step'] = c
        return self._launch(c, step_idx, self._keep_mask(keep), rate, mask_seed, want_loss, sl)

    def step(self, step_idx, uids, before=None, after=None, keep=None, rate=0.0, want_loss=False, mask_seed=0):
        """uids, before, after: the batch (arrays or device tensors) — or `uids` = what prepare_batch, prepare_device_batch or group_slot
        returned for it.
        keep: explicit dropout keep mask [B, n_v + L*n_h] or None; with None and rate > 0 the kernel evaluates the counter-based
        mask drx_hash_u32(mask_seed, b, j) >= rate * 2^32 itself (no 344 K host random numbers per batch of 4096)."""
        if isinstance(uids, dict) and 'csr_dev' in uids:           # a ring slot: ids and grouped lookups already on the device
            return self._step_slot(step_idx, uids, keep, rate, mask_seed, want_loss)
        tensors = not isinstance(uids, dict) and any(torch.is_tensor(a) for a in (uids, before, after))
        if isinstance(uids, dict) or (self.table_update == 'csr' and not tensors):
            # a host batch with its lookups grouped by row on the host: one asynchronous copy for all of it
            prep = uids if isinstance(uids, dict) else self.prepare_batch(uids, before, after)
            alive = self._stage.upload(prep['buf'])
            B = prep['B']
            pb = [alive.data_ptr() + o for o in prep['offs']]
            ids, csr, kp = pb[:3], pb[3:], self._keep_mask(keep, non_blocking=True)
        elif tensors or torch.is_tensor(keep):
            uid, bef, aft = self._dev_i32(uids), self._dev_i32(before), self._dev_i32(after)
            B = uid.numel()
            assert bef.shape == (B, self.L) and aft.shape == (B, self.Tp)
            if self.table_update == 'csr' and self.device_csr:
                # a batch that is already on the device (Caser.fit(device_sampler=True)): the lookups are grouped by table row THERE
                # and the step takes the same two launches as a host batch
                return self._step_slot(step_idx, self.prepare_device_batch(uid, bef, aft), keep, rate, mask_seed, want_loss)
            ids, csr, kp = (uid.data_ptr(), bef.data_ptr(), aft.data_ptr()), None, self._keep_mask(keep)
        else:                                              # host arrays, 'scatter' update: one asynchronous copy for all of them
            arrays = [np.ascontiguousarray(uids, dtype=np.int32), np.ascontiguousarray(before, dtype=np.int32),
                      np.ascontiguousarray(after, dtype=np.int32)]
            if keep is not None:
                arrays.append(np.ascontiguousarray(keep, dtype=np.uint8))
            alive, views = self._stage(arrays)
            uid, bef, aft = views[:3]
            B = uid.numel()
            assert bef.shape == (B, self.L) and aft.shape == (B, self.Tp)
            ids, csr, kp = (uid.data_ptr(), bef.data_ptr(), aft.data_ptr()), None, views[3] if keep is not None else None
        return self._launch(self._build_call(ids, csr, B), step_idx, kp, rate, mask_seed, want_loss)

    # ---- inference: scores of ALL items for each (user, last-L-items) row (caser.py:128-137) --------------------
    def scores_all(self, uids, before):
        uid, bef = self._dev_i32(uids), self._dev_i32(before)
        B = uid.numel()
        cat = self._hidden_rows(uid, bef)
        out = torch.empty(B, self.N, dtype=torch.float32, device=self.device)
        check(lib().drx_rows_dot(ptr(cat), B, ptr(self.W1), self.N, self.ld2, ptr(self.b1), ptr(out),
                                 stream_ptr(self.device)), 'drx_rows_dot')
        return out

    # ---- batched top-n recommendation (include/drx.h drx_rows_recommend, DRX_REC_BIAS) ----------------
    def _hidden_rows(self, uid, bef):
        """[B, ld2] rows [dense_0 output | user row] of drx_caser_hidden; zeros (not torch.empty) behind 2 d: the scorer multiplies them"""
        cat = torch.zeros(int(uid.numel()), self.ld2, dtype=torch.float32, device=self.device)
        A = self._args(uid.data_ptr(), bef.data_ptr(), uid.numel())
        A.cat_out = cat.data_ptr()
        check(lib().drx_caser_hidden(C.byref(self.D), C.byref(A), stream_ptr(self.device)), 'drx_caser_hidden')
        return cat

    # what the four calls of RowsRecommender score against: the logit hidden row . W1 row + b1 — the values scores_all / _rank give.
    # A hidden row belongs to the request row (user, last L items): ONE per row, from one drx_caser_hidden per chunk (a user with T
    # rows has its hidden row computed T times: cheap beside the catalogue walk).  The calls take `before` [R, L] behind the users.
    # Outside the fused domain (n > 128): DrxError — Caser._recommend_batch asks recommend_is_fused first.
    EPILOGUE = _lib.DRX_REC_BIAS
    QUERY_BY_ROW = True

    def rank_ld(self):
        return self.ld2

    def _score_table(self, items=None):
        return self.W1, self.b1

    def _query_rows(self, uid, bef):
        return self._hidden_rows(uid, bef.reshape(int(uid.numel()), self.L))
