"""Time of one Mult-VAE training step at the ml-1m shape (6040 x 3706 synthetic, about 10^6 positives, B = 512 users, Adam, dropout 0.5)
for hidden 128 / latent 64 and hidden 64 / latent 32, in one process, and of serving 1024 users:

    fused   MultVAE._do_batch: drx_vae_step (the noise launch, k_vae_encode, the two catalogue passes, k_vae_back, the small-weight
            launch, the grouping of the batch's lookups, one update launch over W_in)
    tape    the same model written with hooks only — its registered Variables, torch operations in _predict_batch /
            _compute_batch_loss / _compute_reg_loss — on RecommenderABC's generic tape step (a [B, n_items] multi-hot input and target,
            made before the clock starts; log_softmax over a [B, n_items] matrix; one drx_opt_dense per variable)
    serve   drx_vae_query_rows for 1024 users, and MultVAE.recommend_batch (n = 10) for them

    python scripts/vae_bench.py [--batch 512] [--reps 30] [--out profiles/vae_step.json]

The forms train on the same pre-drawn users, keep bits and noise.  Timed by HIP events on the step's stream and by the host's wall clock
around the step with a synchronisation, the forms in turns after warm-up steps; median (min - max).  Nothing here fixes a ratio: the
file records what was measured, and per point whether the fused step's slowest run is faster than the tape step's fastest."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bpr_bench import timed_in_turns  # noqa: E402

REGULARISED = ('W_in', 'W_e', 'W_d', 'W_out')


def tape_model(weights, dropout, beta, device='cuda:0'):
    import torch
    from drecpy_amd.Recommender import RecommenderABC
    from drecpy_amd.Recommender.trainables import Variable

    class TapeMultVAE(RecommenderABC):
        """Mult-VAE with the reference's hooks only: no _do_batch"""

        def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
            self.vars = {n: Variable(w, name=n, device=device) for n, w in weights.items()}
            self._register_trainables(list(self.vars.values()))

        def _sample_batch(self, batch_size, **kwds):
            return self._batches[0]

        def _predict_batch(self, batch_samples, **kwds):
            target, kept, scale, eps = batch_samples                  # [B, N] multi-hot, [B, N] kept multi-hot, c_b [B, 1], [B, latent]
            v = {n: x.tensor for n, x in self.vars.items()}
            latent = v['W_d'].shape[0]
            ml = torch.tanh(scale * (kept @ v['W_in']) + v['b_in']) @ v['W_e'] + v['b_e']
            mu, lv = ml[:, :latent], ml[:, latent:]
            z = mu + eps * torch.exp(lv / 2)
            logit = torch.tanh(z @ v['W_d'] + v['b_d']) @ v['W_out'].T + v['b_out']
            nll = -(torch.log_softmax(logit, dim=1) * target).sum(dim=1)
            kl = -0.5 * (1 + lv - mu * mu - torch.exp(lv)).sum(dim=1)
            return nll + beta * kl, None

        def _compute_batch_loss(self, predictions, desired_values, **kwds):
            return predictions.mean()

        def _compute_reg_loss(self, reg_rate, batch_size, trainable_models, trainable_layers, trainable_weights, **kwds):
            return 0.5 * reg_rate * sum((x.tensor ** 2).sum() for n, x in self.vars.items() if n in REGULARISED)

        def _predict(self, uid, iid, **kwds):
            return None

    return TapeMultVAE(verbose=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--widths', type=str, nargs='+', default=['128x64', '64x32'])
    ap.add_argument('--dropout', type=float, default=0.5)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--serve-users', type=int, default=1024)
    ap.add_argument('--only', choices=['fused'], default=None, help='run the fused steps alone and write no file (for a kernel trace)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vae_step.json'))
    a = ap.parse_args()

    import torch
    from drecpy_amd import synth
    from drecpy_amd.Recommender.Baseline import MultVAE
    ds = synth.dataset('ml-1m')
    B = a.batch
    res = {'shape': 'ml-1m (synthetic)', 'batch_users': B, 'dropout': a.dropout, 'optimizer': 'adam', 'device': torch.cuda.get_device_name(0),
           'reps': a.reps, 'warmup': a.warmup,
           'timed': 'HIP events on the stream and host wall clock around one step with a synchronisation; the forms in turns in one process',
           'by_width': {}}
    fit = dict(epochs=1, batch_size=B, learning_rate=1e-3, reg_rate=1e-3)
    n_steps = a.warmup + a.reps
    for width in a.widths:
        H, L = (int(x) for x in width.split('x'))
        fused = MultVAE(hidden=H, latent=L, dropout=a.dropout, beta=0.2, seed=0, verbose=False)
        fused.fit(ds, **fit)
        eng = fused._engine
        weights = eng.get_params()
        eng.set_params(weights)                               # (every form starts from the weights after the fused model's first step)
        for st in eng.state.values():
            for s in st:
                s.zero_()
        indptr, cols = fused._positives
        N = eng.n_items
        draws = [fused._sample_batch(B) for _ in range(n_steps)]
        res['positives'] = int(indptr[-1])
        res['lookups_per_batch_mean'] = float(np.mean([int((indptr[u.astype(np.int64) + 1] - indptr[u]).sum()) for u, _, _ in draws]))
        if a.only == 'fused':
            for k, (uid, seed, _) in enumerate(draws):
                eng.step(k, uid, seed)
            torch.cuda.synchronize()
            continue
        batches = []
        for uid, seed, _ in draws:                            # the tape's inputs, made before the clock starts
            eps, keep = eng.noise(seed, uid)
            lens = (indptr[uid.astype(np.int64) + 1] - indptr[uid]).astype(np.int64)
            rows = np.repeat(np.arange(len(uid)), lens)
            items = np.concatenate([cols[indptr[u]:indptr[u + 1]] for u in uid])
            target = torch.zeros(len(uid), N, device=eng.device)
            target[torch.as_tensor(rows).to(eng.device), torch.as_tensor(items).to(eng.device)] = 1.0
            kept = torch.zeros_like(target)
            kept[torch.as_tensor(rows).to(eng.device), torch.as_tensor(items).to(eng.device)] = keep.float()
            scale = torch.as_tensor((1.0 / (np.sqrt(np.maximum(lens, 1)) * (1.0 - a.dropout))).astype(np.float32)).to(eng.device)[:, None]
            batches.append((target, kept, scale, eps))
        tape = tape_model(weights, a.dropout, 0.2)
        tape._batches = batches
        tape.fit(ds, **dict(fit, epochs=0))                   # registers the variables and the optimizer; no step
        forms = {'fused': lambda k: eng.step(k, draws[k][0], draws[k][1]), 'tape': lambda k: tape._tape_do_batch(batches[k], step=k)}
        t, done = timed_in_turns(forms, a.warmup, a.reps)
        for name, v in t.items():
            v['users_per_s_at_median_device'] = B / (v['device_ms']['median'] * 1e-3)
        out = dict(t)
        out['fused_over_tape_device'] = t['fused']['device_ms']['median'] / t['tape']['device_ms']['median']
        # beyond the recorded spread: the fused step's slowest run against the tape step's fastest
        out['fused_beats_tape_beyond_the_spread'] = bool(t['fused']['device_ms']['max'] < t['tape']['device_ms']['min'])
        # the step's necessary HBM traffic: the gathered W_in rows, W_out read twice and written once with its slots (read and written)
        ldh = eng.ldh
        need = 4 * ldh * (res['lookups_per_batch_mean'] * (1.0 - a.dropout) + N * (2 + 1 + 2 * 2))
        out['necessary_hbm_bytes'] = need
        out['steps_compared'] = done
        users = torch.arange(a.serve_users, dtype=torch.int32, device=eng.device) % eng.n_users
        raw = ds.unique('user').values_list('user', to_list=True)[:a.serve_users]
        out['serve'] = timed_in_turns({'query_rows': lambda k: eng._query_rows(users),
                                       'recommend_batch_n10': lambda k: fused.recommend_batch(raw, n=10)}, 2, max(5, a.reps // 3))[0]
        out['serve']['users'] = int(users.numel())
        res['by_width'][f'hidden{H}_latent{L}'] = out
        res['n_users'], res['n_items'] = eng.n_users, eng.n_items
    if a.only:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(json.dumps(res, sort_keys=True, indent=1) + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
