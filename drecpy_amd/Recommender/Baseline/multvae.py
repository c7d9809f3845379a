"""Mult-VAE / Mult-DAE (Liang, Krishnan, Hoffman, Jebara: "Variational Autoencoders for Collaborative Filtering", WWW 2018) on the MI355X
engine — the autoencoder that superseded CDAE, beside it on the same splits and evaluation processes.  The reference has no such
model; the definition of record is tests/vae_oracle.py, the arithmetic csrc/drx_vae.hip behind include/drx.h ("Mult-VAE"; DESIGN.md
section 3.13).

    forward  P_u: the user's items with interaction >= interaction_threshold (all recorded items where it is None), N_u = |P_u|;
             x1 = c sum_{kept i in P_u} W_in[i] + b_in, c = 1 / (sqrt(N_u) (1 - dropout)); h1 = tanh(x1); [mu | logvar] = h1 W_e + b_e
             (no logvar where variational=False); z = mu + eps exp(logvar / 2) in training, z = mu in serving and where
             variational=False; h2 = tanh(z W_d + b_d); logit_i = h2 . W_out[i] + b_out[i] for every item
    score    x(u, i) = logit_i at z = mu, every positive kept (`_predict(u, i)` returns the logit: softmax is monotone, so every
             ranking is the logits' ranking).  There is no user table.
    batch    np.random.default_rng(seed_k).choice(eligible, size=min(batch_size, len(eligible)), replace=False) with the eligible
             users those with N_u >= 1 and seed_k = `_draw_seed(k)` of draw k of a fit(); one "epoch" is one batch.  The keep bit of
             lookup j of batch row b and the noise of (b, column) are functions of seed_k alone (drx_vae_noise: hash_u32 against
             q_threshold(dropout); Box-Muller on two hash_u32 words).
    step     loss = mean_b [-sum_{i in P_u} log softmax(logit)_i + beta_t KL_b] — the target is the whole of P_u, not its kept part —,
             KL_b = -1/2 sum (1 + logvar - mu^2 - exp(logvar)), beta_t = beta min(1, (step + 1) / anneal_steps) (beta where
             anneal_steps == 0); reg_rate * value added to the gradient of EVERY row of W_in and W_out and every entry of W_e and W_d
             (dense; the biases are not regularised); one of the dense rules of fit(optimizer=...), Adam by default, W_in registered
             first, then the small weights, then W_out with b_out.
    weights  initial_weights(): from np.random.default_rng(seed), in this order: W_in ~ N(0, init_std) [n_items, hidden], W_e ~
             U(-1/sqrt(hidden), 1/sqrt(hidden)) [hidden, 2 latent or latent], W_d ~ U(-1/sqrt(latent), 1/sqrt(latent)) [latent, hidden],
             W_out ~ N(0, init_std) [n_items, hidden]; the biases zero.

Deviations from Liang et al.: widths up to 128 / 64 instead of 600 / 200; one hidden layer on each side; the logit is the reported
value; a batch is drawn without replacement from the eligible users by a seeded generator instead of walking a shuffled epoch; the
input bag is scaled by 1 / sqrt(N_u) (their L2 normalisation of a binary row) before dropout's 1 / (1 - p); the logged loss has no L2 term.

fit() accepts neg_ratio and ignores it: a full softmax has no sampled negatives.  Prediction and serving run through the fused hooks of
RecommenderABC (recommend_batch, catalogue_ranks, predict_pairs) on the engine's DRX_REC_BIAS scorer at rows of `hidden` floats; rank() /
ranking_evaluation select on a score matrix: FactorServing's (_base.py), as the draw seeds, _configure_optimizer and _do_batch are
SampledDenseFit's.  Single GPU only.
"""
import numpy as np

from ._base import SampledDenseFit


class MultVAE(SampledDenseFit):
    """MultVAE(hidden=128, latent=64, variational=True, beta=0.2, anneal_steps=0, dropout=0.5, init_std=0.01, device='cuda:0'): the
    multinomial-likelihood variational autoencoder (Mult-DAE where variational=False) with a full softmax over the catalogue;
    1 <= hidden <= 128, 1 <= latent <= 64, 0 <= dropout < 1, beta >= 0, anneal_steps >= 0, single GPU.

    Deviations from Liang et al. 2018: widths up to 128 / 64 instead of 600 / 200; one hidden layer on each side; the logit is the
    reported value; a batch is drawn without replacement from the users with a positive by a seeded generator, one batch an "epoch"."""
    MODEL, NEGATIVES_PER, DENSE_UPDATE_OF = 'MultVAE', 'ignored: a full softmax has no negatives', 'both item tables and the small weights'
    MAX_HIDDEN = 128
    MAX_LATENT = 64

    def __init__(self, hidden=128, latent=64, variational=True, beta=0.2, anneal_steps=0, dropout=0.5, init_std=0.01, device='cuda:0',
                 **kwds):
        super().__init__(**kwds)
        self.hidden = hidden
        self.latent = latent
        self.variational = variational
        self.beta = beta
        self.anneal_steps = anneal_steps
        self.dropout = dropout
        self.init_std = init_std
        self.device = device

    # ---- fit -----------------------------------------------------------------------------------------------------------------------
    def _check_shape(self):
        integer = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, bool)
        real = lambda x: isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)
        if not (integer(self.hidden) and 1 <= self.hidden <= self.MAX_HIDDEN):
            raise Exception(f'MultVAE(hidden={self.hidden!r}): hidden must be an integer in 1..{self.MAX_HIDDEN}.')
        if not (integer(self.latent) and 1 <= self.latent <= self.MAX_LATENT):
            raise Exception(f'MultVAE(latent={self.latent!r}): latent must be an integer in 1..{self.MAX_LATENT}.')
        if not (real(self.dropout) and 0 <= self.dropout < 1):
            raise Exception(f'MultVAE(dropout={self.dropout!r}): dropout must be a number in [0, 1).')
        if not (real(self.beta) and self.beta >= 0):
            raise Exception(f'MultVAE(beta={self.beta!r}): beta must be a number >= 0.')
        if not (integer(self.anneal_steps) and self.anneal_steps >= 0):
            raise Exception(f'MultVAE(anneal_steps={self.anneal_steps!r}): anneal_steps must be an integer >= 0.')

    def initial_weights(self):
        """the arrays of a fresh model, drawn in the order of the module docstring"""
        H, L, N = int(self.hidden), int(self.latent), int(self.n_items)
        E = 2 * L if self.variational else L
        rng = np.random.default_rng(self.seed)
        w = {'W_in': rng.normal(0.0, self.init_std, size=(N, H))}
        w['W_e'] = rng.uniform(-1.0 / np.sqrt(H), 1.0 / np.sqrt(H), size=(H, E))
        w['W_d'] = rng.uniform(-1.0 / np.sqrt(L), 1.0 / np.sqrt(L), size=(L, H))
        w.update({'b_in': np.zeros(H), 'b_e': np.zeros(E), 'b_d': np.zeros(H), 'W_out': rng.normal(0.0, self.init_std, size=(N, H)),
                  'b_out': np.zeros(N)})
        return w

    def _new_engine(self):
        from ...engine_vae import VaeEngine
        e = VaeEngine(self.n_users, self.n_items, int(self.hidden), int(self.latent), bool(self.variational), device=self.device)
        e.dropout, e.beta, e.anneal_steps = float(self.dropout), float(self.beta), int(self.anneal_steps)
        positives, _, _ = self._positives_frame()
        e.set_positives(positives)
        self._positives = (np.asarray(positives[0], np.int64), np.asarray(positives[1], np.int64))
        self._eligible = np.flatnonzero(np.diff(self._positives[0]) >= 1).astype(np.int32)
        return e

    def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
        self._start_sampled_fit(1)                     # (neg_ratio is accepted and ignored, as in ALS)
        self._check_shape()
        self._engine = self._new_engine()
        if len(self._eligible) == 0:
            raise Exception('MultVAE.fit: the dataset has no user with an interaction >= interaction_threshold.')
        self._engine.lr, self._engine.reg = float(learning_rate), float(reg_rate)
        weights = kwds.get('initial_weights')
        self._engine.set_params(weights if weights is not None else self.initial_weights())
        self._register_trainables(self._fused_trainables())

    def _restore_engine(self, params):
        """RecommenderABC.load: the engine rebuilt from the saved weights, the positives from the bound dataset"""
        self._engine = self._new_engine()
        self._engine.set_params(params)

    def _fused_trainables(self):
        e = self._engine
        return [e.input_emb, e.small, e.item_emb]

    def _sample_batch(self, batch_size, **kwds):
        """(uid [B], the draw seed, None): the step derives its keep bits and its noise from the seed on the device"""
        seed = self._next_draw_seed()
        uid = np.random.default_rng(seed).choice(self._eligible, size=min(int(batch_size), len(self._eligible)), replace=False)
        return uid.astype(np.int32), seed, None

    def _predict_batch(self, batch_samples, **kwds):
        """-sum_{i in P_u} log softmax(logit)_i of the batch's users at z = mu, every positive kept (numpy float64 [B]) against the
        target 0 — the reference's training hook, kept for callers, never on the training path (the fused step computes its loss
        itself): the definition on the host, from a copy of the parameters."""
        uid = np.asarray(batch_samples[0], np.int64)
        with self._device_lock:
            p = {k: v.astype(np.float64) for k, v in self._engine.get_params().items()}
        indptr, cols = self._positives
        L = p['W_d'].shape[0]
        out = np.zeros(len(uid))
        for b, u in enumerate(uid):
            row = cols[indptr[u]:indptr[u + 1]]
            x1 = p['W_in'][row].sum(axis=0) / np.sqrt(max(len(row), 1)) + p['b_in']
            mu = (np.tanh(x1) @ p['W_e'] + p['b_e'])[:L]
            logit = np.tanh(mu @ p['W_d'] + p['b_d']) @ p['W_out'].T + p['b_out']
            top = logit.max()
            out[b] = -np.sum(logit[row] - top - np.log(np.sum(np.exp(logit - top))))
        return out, np.zeros(len(uid))

    def _compute_batch_loss(self, predictions, desired_values, **kwds):
        """the mean of the rows' negative log-likelihoods"""
        return float(np.mean(np.asarray(predictions, dtype=np.float64)))
