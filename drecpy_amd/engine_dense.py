"""What the engines of the dense models (DMF, Caser, BPR, FPMC, NeuMF, GRU4Rec, SASRec, Mult-VAE, LightGCN) share: the update rule of optimizers.py with its slots, the
snapshot of parameters and slots, the layout of several arrays in one buffer and the keep mask of a step as device bytes; for the fused
steps of the sampled baselines (drx_bpr_step, drx_fpmc_step, drx_ncf_step, drx_gru_step, drx_sas_step, drx_vae_step, drx_lgcn_step) also the host frame of a step — scratch, step sizes, slot
pointers, loss — and the sampler's frame on the device.  (KnnEngine has no optimizer and stays a plain RowsRecommender.)"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import History, ptr
from .engine_rows import ADAM_B1, ADAM_B2, ADAM_EPS, RowsRecommender


def aligned_offsets(nbytes):
    """(byte offset of every array, total bytes) of arrays of `nbytes` bytes each laid out one behind the other, every one at a
    16-byte aligned offset — an empty array takes no room."""
    offs, total = [], 0
    for n in nbytes:
        offs.append(total)
        total += (n + 15) & ~15
    return offs, total


class DenseEngine(RowsRecommender):
    """An engine whose parameters are `tensors()` (name -> device tensor), each updated by one dense rule with up to two slots."""

    def _init_optimizer_state(self):
        """Keras Adam at its defaults, slots at zero, for every tensor of tensors() (call once they exist)."""
        self.beta1, self.beta2, self.eps = ADAM_B1, ADAM_B2, ADAM_EPS
        self.opt_kind, self._slot_init = 'adam', 0.0        # (set_optimizer: another dense rule of optimizers.py)
        self.state = {n: (torch.zeros_like(t), torch.zeros_like(t)) for n, t in self.tensors().items()}

    # ---- the host frame of one fused step: C ABI (tensors, their slots s1 s2 in tensors() order, ..., rule, alphas, reg, loss, scratch) ----
    ALPHA_OF = ()       # per tensor of tensors(): which handle of applies[1:] it is updated with, hence whose step size it takes

    def _init_step_state(self):
        """once the tensors exist: the optimizer state, the defaults of lr / reg, no scratch yet, the loss cell"""
        self._init_optimizer_state()
        self.lr, self.reg = 1e-3, 1e-3
        self._scratch = None
        self._loss = torch.zeros(1, dtype=torch.float64, device=self.device)

    def _step_sizes(self, step_idx, applies):
        """One step size per tensor of tensors(): Keras Adam's lr_t of its apply's counter; the learning rate under every other rule.
        applies = (n, j_0, j_1, ...): the number of apply_gradients calls per step and the position of every handle among them."""
        n, positions = applies[0], applies[1:]
        if self.opt_kind != 'adam':
            return (self.lr,) * len(self.ALPHA_OF)
        a = [self.adam_alpha(self.lr, n * step_idx + j + 1, self.beta1, self.beta2) for j in positions]
        return tuple([a[k] for k in self.ALPHA_OF])

    def _step_scratch(self, need, refusal):
        """the kept scratch of the step at `need` bytes or more (what its *_step_scratch_bytes answers); 0: outside the domain, refused in
        the words of refusal() (made only then: a step pays for no message)"""
        if need == 0:
            raise _lib.DrxError(refusal())
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = None
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._scratch

    def _step_args(self, step_idx, applies, want_loss):
        """(the step sizes as a C array, the slot pointers of every tensor, the loss pointer or None when no loss is wanted)"""
        alphas = (C.c_float * len(self.ALPHA_OF))(*self._step_sizes(step_idx, applies))
        return alphas, [ptr(s) for st in self.state.values() for s in st], ptr(self._loss) if want_loss else None

    def _read_loss(self, want_loss):
        return float(self._loss.cpu().numpy()[0]) if want_loss else None

    def _upload_frame(self, positives, recorded):
        """The sampler's frame on the device: positives = (indptr, indices) of the pairs with interaction >= threshold; recorded =
        (indptr, indices) of every pair of the frame, or None where all of them are positives.  _H / _R: their History structs."""
        d = self.device
        up = lambda csr: (torch.as_tensor(np.asarray(csr[0], np.int64)).to(d),
                          torch.as_tensor(np.asarray(csr[1], np.int32) if len(csr[1]) else np.zeros(1, np.int32)).to(d))
        self._pos = up(positives)
        self._rec = up(recorded) if recorded is not None else None
        self._H = History(ptr(self._pos[0]), ptr(self._pos[1]))
        self._R = History(ptr(self._rec[0]), ptr(self._rec[1])) if self._rec is not None else None

    def set_optimizer(self, opt):
        """The update rule of every dense step from a drecpy_amd.optimizers object (Adam, Adagrad, SGD, RMSprop): its kind and
        hyper-parameters, and slots of that rule alone — none for plain SGD, s1 for all but Adam and RMSprop with momentum (Adagrad's at
        its accumulator value).  beta1 / beta2 carry include/drx.h DrxOptRule's mu / mu2.  Slots that already fit the rule are kept."""
        from .optimizers import KINDS, N_SLOTS
        kind = opt.kind
        if kind not in KINDS or kind == 'rowwise_adagrad':
            raise _lib.DrxError(f'no dense update rule "{kind}"')
        mu, mu2 = opt._mus()
        self.lr, self.beta1, self.beta2, self.eps = opt.learning_rate, mu, mu2, getattr(opt, 'epsilon', 0.0)
        if kind == self.opt_kind and getattr(opt, 'slot_init', 0.0) == self._slot_init:
            return
        self.opt_kind, self._slot_init = kind, float(getattr(opt, 'slot_init', 0.0))
        n = N_SLOTS[kind]
        self.state = {name: tuple(torch.full_like(t, self._slot_init) if i < n else None for i in range(2)) for name, t in self.tensors().items()}

    def _rule(self, step_size=0.0):
        """include/drx.h DrxOptRule of the engine's rule (step_size: where the entry point has none per variable)"""
        key = (self.opt_kind, step_size, self.beta1, self.beta2, self.eps)
        c = self.__dict__.get('_rule_cache')
        if c is None or c[0] != key:                     # (one struct per setting: the steps pass it by reference)
            from .optimizers import KINDS
            c = self._rule_cache = (key, _lib.OptRule(KINDS[self.opt_kind], step_size, self.beta1, self.beta2, self.eps))
        return c[1]

    def snapshot(self):
        """Device copies of the parameters and of the slots the rule has (used by _store_epoch_weights / _revert_weights)."""
        return {'p': {n: t.clone() for n, t in self.tensors().items()},
                's': {n: tuple(None if t is None else t.clone() for t in st) for n, st in self.state.items()}}

    def restore(self, snap, with_optimizer=False):
        for n, t in self.tensors().items():
            t.copy_(snap['p'][n])
        if with_optimizer and 's' in snap:
            for n, st in self.state.items():
                for dst, src in zip(st, snap['s'][n]):
                    if dst is not None and src is not None:
                        dst.copy_(src)

    def _keep_mask(self, keep, non_blocking=False):
        """an explicit dropout keep mask (array or tensor, or None) as a uint8 device tensor"""
        if keep is None:
            return None
        if torch.is_tensor(keep):
            return keep.to(self.device, torch.uint8).contiguous()
        return torch.as_tensor(np.ascontiguousarray(keep, dtype=np.uint8)).to(self.device, non_blocking=non_blocking)
