"""Device-side state of one Mult-VAE / Mult-DAE model (Liang et al. 2018) and the calls into libdrx.so (drx_vae_*; include/drx.h
"Mult-VAE").

Score x(u, i) = h2(u) . W_out[i] + b_out[i] — DRX_REC_BIAS of the fused scorer at rows of ldh floats, with W_out as the table, b_out as
the bias and h2 of the user's positives at z = mu (drx_vae_query_rows) as the query row: recommend / rank_items / rank_lists /
pair_scores are RowsRecommender's.  There is no user table.  One training step = drx_vae_step on B users.  torch is the allocator /
stream provider only.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .engine_dense import DenseEngine
from .engine_rows import _round_up

MAX_HIDDEN = 128
MAX_LATENT = 64
MAX_BATCH = 65536
SMALL = ('W_e', 'W_d', 'b_in', 'b_e', 'b_d')


def check_shape(hidden, latent, who='Mult-VAE engine'):
    """the domain of csrc/drx_vae.hip, refused by name"""
    integer = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, bool)
    if not (integer(hidden) and 1 <= hidden <= MAX_HIDDEN):
        raise _lib.DrxError(f'{who}: hidden must be an integer in 1..{MAX_HIDDEN}, got hidden={hidden!r}')
    if not (integer(latent) and 1 <= latent <= MAX_LATENT):
        raise _lib.DrxError(f'{who}: latent must be an integer in 1..{MAX_LATENT}, got latent={latent!r}')
    return int(hidden), int(latent)


class VaeEngine(DenseEngine):
    EPILOGUE = _lib.DRX_REC_BIAS
    ALPHA_OF = (0, 1, 2)                   # W_in, the small weights, W_out with b_out: a handle each

    def __init__(self, n_users, n_items, hidden=128, latent=64, variational=True, device='cuda:0'):
        self._require_gpu()
        self.H, self.latent = check_shape(hidden, latent)
        self.variational = bool(variational)
        z = self._open(n_users, n_items, device)
        H, L = self.H, self.latent
        E = self.E = 2 * L if self.variational else L
        self.ldh = _round_up(H, 4)
        # the flat array of small weights, no padding, the regularised entries first (include/drx.h DrxVaeDims)
        off_wd = H * E
        off_vec = off_wd + L * H
        self.dims = _lib.VaeDims(n_items=self.n_items, h=H, ldh=self.ldh, latent=L, variational=int(self.variational), e=E, off_we=0,
                                 off_wd=off_wd, off_vec=off_vec, n_small=off_vec + 2 * H + E)
        self.slices = {'W_e': (0, (H, E)), 'W_d': (off_wd, (L, H)), 'b_in': (off_vec, (H,)), 'b_e': (off_vec + H, (E,)),
                       'b_d': (off_vec + H + E, (H,))}
        self.n_small = int(self.dims.n_small)
        self.W_in = torch.zeros(self.n_items, self.ldh, **z)
        self.sw = torch.zeros(self.n_small, **z)
        self.W_out = torch.zeros(self.n_items, self.ldh, **z)
        self.b_out = torch.zeros(self.n_items, **z)
        self._init_step_state()
        self.dropout, self.beta, self.anneal_steps = 0.0, 0.0, 0
        self._indptr = None
        # what MultVAE._pre_fit registers, in this order: one apply_gradients per handle and step
        self.input_emb = self._handle('input_weights', 'W_in')
        self.small = self._handle('small_weights', *self.slices)
        self.item_emb = self._handle('output_weights', 'W_out', 'b_out')

    def tensors(self):
        return {'W_in': self.W_in, 'sw': self.sw, 'W_out': self.W_out, 'b_out': self.b_out}

    def _small(self, name):
        off, shape = self.slices[name]
        return self.sw[off:off + int(np.prod(shape))].view(*shape)

    def views(self):
        """{'W_in': [n_items, H], 'W_e': [H, E], 'W_d': [latent, H], 'b_in': [H], 'b_e': [E], 'b_d': [H], 'W_out': [n_items, H],
        'b_out': [n_items]}: the small weights in the order of the flat array"""
        v = {'W_in': self.W_in[:, :self.H]}
        v.update({name: self._small(name) for name in self.slices})
        v.update({'W_out': self.W_out[:, :self.H], 'b_out': self.b_out})
        return v

    def set_positives(self, positives):
        """positives = (indptr [n_users + 1], indices): every user's items with interaction >= threshold, ascending — the input bag
        of the encoder and the target of the softmax, on the device through DenseEngine._upload_frame"""
        indptr = np.asarray(positives[0], np.int64)
        if len(indptr) != self.n_users + 1:
            raise _lib.DrxError(f'Mult-VAE engine: the positives CSR must have {self.n_users} rows')
        self._upload_frame((indptr, positives[1]), None)
        self._indptr = indptr

    def beta_t(self, step_idx):
        """the KL weight of step `step_idx` (0-based): beta min(1, (step + 1) / anneal_steps), beta where anneal_steps == 0"""
        return self.beta if not self.anneal_steps else self.beta * min(1.0, (int(step_idx) + 1) / self.anneal_steps)

    def _frame(self, uid):
        """(uid on the device, boff [B + 1] on the device, B, T, max_len) of a batch of users (a host array)"""
        uid = np.ascontiguousarray(uid, dtype=np.int32).reshape(-1)
        lens = self._indptr[uid.astype(np.int64) + 1] - self._indptr[uid]
        boff = np.zeros(len(uid) + 1, np.int32)
        boff[1:] = np.cumsum(lens)
        to = lambda a: torch.as_tensor(a).to(self.device)
        return to(uid), to(boff), len(uid), int(boff[-1]), int(lens.max(initial=0))

    def noise(self, seed, uid, want_words=False):
        """(eps [B, latent] float32, keep [T] uint8(, words [B, latent, 2] as int64)) of draw `seed` for the batch uid: drx_vae_noise"""
        uid_d, boff, B, T, _ = self._frame(uid)
        eps = torch.empty(B, self.latent, dtype=torch.float32, device=self.device)
        keep = torch.empty(max(T, 1), dtype=torch.uint8, device=self.device)
        words = torch.empty(B, self.latent, 2, dtype=torch.int32, device=self.device) if want_words else None
        check(lib().drx_vae_noise(int(seed) & (2 ** 64 - 1), ptr(boff), B, T, self.latent, float(self.dropout), ptr(eps), ptr(keep),
                                  ptr(words), stream_ptr(self.device)), 'drx_vae_noise')
        keep = keep[:T]
        return (eps, keep, words.cpu().numpy().astype(np.int64) & 0xFFFFFFFF) if want_words else (eps, keep)

    # ---- the step (include/drx.h drx_vae_step) ---------------------------------------------------------------------------------------
    def step(self, step_idx, uid, seed=None, _unused=None, want_loss=False, applies=None, eps=None, keep=None):
        """One step on the B users uid (a host array).  seed: the draw seed the noise and the keep bits are functions of (drx_vae_noise);
        eps [B, latent] / keep [T] (flat, the rows one behind the other): explicit arrays in their place — with neither a seed nor
        an array, z = mu and every lookup is kept.  applies = (n, j_input, j_small, j_output): the number of apply_gradients calls per
        step and the positions of the three handles among them; default (3, 0, 1, 2).  Returns the batch's mean loss (the data term
        plus beta_t KL) before the update when want_loss, else None."""
        applies = tuple(applies) if applies is not None else (3, 0, 1, 2)
        uid_d, boff, B, T, max_len = self._frame(uid)
        if seed is not None and (eps is None or keep is None):
            n_eps, n_keep = self.noise(seed, uid)
            eps = n_eps if eps is None and self.variational else eps
            keep = n_keep if keep is None and self.dropout > 0 else keep
        if eps is not None:
            eps = torch.as_tensor(np.ascontiguousarray(eps, dtype=np.float32)).to(self.device) if not torch.is_tensor(eps) else eps.contiguous()
            assert tuple(eps.shape) == (B, self.latent), f'eps must be [{B}, {self.latent}]'
        keep = self._keep_mask(keep)
        assert keep is None or keep.numel() == T, f'keep must hold the {T} lookups of the batch'
        L_ = lib()
        scratch = self._step_scratch(int(L_.drx_vae_step_scratch_bytes(C.byref(self.dims), B, T, max_len)),
                                     lambda: f'drx_vae_step: a batch of {B} users with {T} positives is outside its domain '
                                     f'(1..{MAX_BATCH} users, at least one positive)')
        alphas, slots, loss = self._step_args(step_idx, applies, want_loss)
        check(L_.drx_vae_step(C.byref(self.dims), ptr(self.W_in), ptr(self.sw), ptr(self.W_out), ptr(self.b_out), *slots, C.byref(self._H),
                              ptr(uid_d), ptr(boff), B, T, max_len, ptr(eps), ptr(keep), float(self.dropout), float(self.beta_t(step_idx)),
                              C.byref(self._rule()), alphas, float(self.reg), loss, ptr(scratch), scratch.numel(),
                              stream_ptr(self.device)), 'drx_vae_step')
        return self._read_loss(want_loss)

    def step_hidden(self, B):
        """[B, ldh]: the h2 the last step wrote for its B rows — the first array of its scratch (drx_vae_step's carve, from the first
        256-byte boundary).  For tests: serving's rows are held to these bits."""
        base = (-self._scratch.data_ptr()) % 256
        return self._scratch[base:base + 4 * B * self.ldh].view(torch.float32).view(B, self.ldh).clone()

    # what the four calls of RowsRecommender and its score_matrix score against: W_out and b_out themselves, and h2 of the users
    def rank_ld(self):
        return self.ldh

    def _score_table(self, items=None):
        return self.W_out, self.b_out

    def _query_rows(self, uid):
        """[len(uid), ldh] rows h2(u) (drx_vae_query_rows): they depend on the user alone"""
        n = int(uid.numel())
        out = torch.empty(n, self.ldh, dtype=torch.float32, device=self.device)
        if n:
            check(lib().drx_vae_query_rows(ptr(self.W_in), ptr(self.sw), C.byref(self.dims), C.byref(self._H), ptr(uid), n, ptr(out),
                                           stream_ptr(self.device)), 'drx_vae_query_rows')
        return out
