"""Time of one SASRec training step at the ml-1m shape (6040 x 3706 synthetic sequences, 4096 windows, r = 4, H = 64, Adam) for
L = 5, 10 and 16 and blocks = 1 and 2, in one process, and of serving 1024 users:

    fused   SASRec._do_batch: drx_sas_step (k_sas_tile, the small-weight launch, the grouping of the two key lists, one update launch
            over E and Q with b)
    tape    the same model written with hooks only — its registered Variables, torch operations in _predict_batch /
            _compute_batch_loss / _compute_reg_loss — on RecommenderABC's generic tape step (torch.autograd through the blocks,
            index_add with atomics, one drx_opt_dense per variable)
    gru     drx_gru_step on the same windows at K = H, L <= 8 only: the recurrent model's step
    serve   drx_sas_query_rows for 1024 users, and SASRec.recommend_batch (n = 10) for them

    python scripts/sasrec_bench.py [--batch 4096] [--hidden 64] [--reps 30] [--out profiles/sasrec_step.json]

The forms train on the same pre-drawn windows (drx_list_sample_device).  Timed by HIP events on the step's stream and by the host's wall
clock around the step with a synchronisation, the forms in turns after warm-up steps; median (min - max).  Nothing here fixes a ratio:
the file records what was measured, and per point whether the fused step's slowest run is faster than the tape step's fastest."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bpr_bench import timed_in_turns  # noqa: E402

REGULARISED = ('E', 'Q', 'Pos', 'Wq', 'Wk', 'Wv', 'W1', 'W2')


def tape_model(weights, blocks, device='cuda:0'):
    import torch
    import torch.nn.functional as F
    from drecpy_amd.Recommender import RecommenderABC
    from drecpy_amd.Recommender.trainables import Variable

    class TapeSASRec(RecommenderABC):
        """SASRec with the reference's hooks only: no _do_batch"""

        def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
            self.vars = {n: Variable(w, name=n, device=device) for n, w in weights.items()}
            self._register_trainables(list(self.vars.values()))

        def _sample_batch(self, batch_size, **kwds):
            return self._batches[0]

        def _predict_batch(self, batch_samples, **kwds):
            _, s, a = (t.long() for t in batch_samples[:3])
            v = {n: x.tensor for n, x in self.vars.items()}
            L, H = v['Pos'].shape
            x = v['E'][s] + v['Pos'][None]
            causal = torch.tril(torch.ones(L, L, dtype=torch.bool, device=x.device))
            for b in range(blocks):
                y = F.layer_norm(x, (H,), v[f'ln1_g{b}'], v[f'ln1_b{b}'], 1e-5)
                sc = (y @ v[f'Wq{b}']) @ (y @ v[f'Wk{b}']).transpose(1, 2) / float(np.sqrt(H))
                x = x + torch.softmax(sc.masked_fill(~causal, float('-inf')), dim=2) @ (y @ v[f'Wv{b}'])
                f = F.layer_norm(x, (H,), v[f'ln2_g{b}'], v[f'ln2_b{b}'], 1e-5)
                x = x + torch.relu(f @ v[f'W1{b}'] + v[f'b1{b}']) @ v[f'W2{b}'] + v[f'b2{b}']
            h = F.layer_norm(x[:, L - 1], (H,), v['lnf_g'], v['lnf_b'], 1e-5)
            out = (h[:, None, :] * v['Q'][a]).sum(dim=2) + v['b'][a]
            return (out[:, :1] - out[:, 1:]).reshape(-1), None

        def _compute_batch_loss(self, predictions, desired_values, **kwds):
            return torch.nn.functional.softplus(-predictions).mean()

        def _compute_reg_loss(self, reg_rate, batch_size, trainable_models, trainable_layers, trainable_weights, **kwds):
            return 0.5 * reg_rate * sum((x.tensor ** 2).sum() for n, x in self.vars.items() if n in REGULARISED or n[:2] in REGULARISED)

        def _predict(self, uid, iid, **kwds):
            return None

    return TapeSASRec(verbose=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--hidden', type=int, default=64)
    ap.add_argument('--neg-ratio', type=int, default=4)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--serve-users', type=int, default=1024)
    ap.add_argument('--windows', type=int, nargs='+', default=[5, 10, 16])
    ap.add_argument('--blocks', type=int, nargs='+', default=[1, 2])
    ap.add_argument('--only', choices=['fused'], default=None, help='run the fused steps alone and write no file (for a kernel trace)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sasrec_step.json'))
    a = ap.parse_args()

    import torch
    from drecpy_amd import synth
    from drecpy_amd.engine_gru import GruEngine
    from drecpy_amd.optimizers import Adam
    from drecpy_amd.Recommender.Baseline import SASRec
    ds = synth.dataset('ml-1m', with_timestamp=True)
    B, r, H = a.batch, a.neg_ratio, a.hidden
    res = {'shape': 'ml-1m (synthetic sequences)', 'batch_windows': B, 'hidden': H, 'neg_ratio': r, 'optimizer': 'adam',
           'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup,
           'timed': 'HIP events on the stream and host wall clock around one step with a synchronisation; the forms in turns in one process',
           'by_L_blocks': {}}
    fit = dict(epochs=1, batch_size=B, learning_rate=1e-3, neg_ratio=r, reg_rate=1e-3)
    n_steps = a.warmup + a.reps
    for L in a.windows:
        for nb in a.blocks:
            fused = SASRec(hidden=H, L=L, blocks=nb, seed=0, verbose=False)
            fused.fit(ds, **fit)
            eng = fused._engine
            weights = eng.get_params()
            eng.set_params(weights)                           # (every form starts from the weights after the fused model's first step)
            for st in eng.state.values():
                for s in st:
                    s.zero_()
            batches = [tuple(t.clone() for t in fused._sampler.sample_device(B, 1000 + k)) for k in range(n_steps)]
            if a.only == 'fused':
                for k in range(n_steps):
                    eng.step(k, *batches[k])
                torch.cuda.synchronize()
                continue
            tape = tape_model(weights, nb)
            tape._batches = batches
            tape.fit(ds, **dict(fit, epochs=0))               # registers the variables and the optimizer; no step
            forms = {'fused': lambda k: eng.step(k, *batches[k]), 'tape': lambda k: tape._tape_do_batch(batches[k], step=k)}
            if L <= 8:
                gru = GruEngine(eng.n_users, eng.n_items, H, H, L)
                rng = np.random.default_rng(0)
                gru.set_params({'E': rng.normal(0.0, 0.01, size=(eng.n_items, H)), 'Wx': rng.uniform(-0.125, 0.125, size=(H, 3 * H)),
                                'Wh': rng.uniform(-0.125, 0.125, size=(H, 3 * H)), 'bx': np.zeros(3 * H), 'bhn': np.zeros(H),
                                'Q': rng.normal(0.0, 0.01, size=(eng.n_items, H)), 'b': np.zeros(eng.n_items)})
                gru.set_optimizer(Adam(1e-3))
                forms['gru'] = lambda k: gru.step(k, *batches[k])
            t, done = timed_in_turns(forms, a.warmup, a.reps)
            for name, v in t.items():
                v['windows_per_s_at_median_device'] = B / (v['device_ms']['median'] * 1e-3)
            out = dict(t)
            out['fused_over_tape_device'] = t['fused']['device_ms']['median'] / t['tape']['device_ms']['median']
            # beyond the recorded spread: the fused step's slowest run against the tape step's fastest
            out['fused_beats_tape_beyond_the_spread'] = bool(t['fused']['device_ms']['max'] < t['tape']['device_ms']['min'])
            # the two forms after the same steps on the same windows: the tape's sums run in another order and its Adam counters
            # differ (one apply per variable against three), so the parameters agree only roughly; recorded, not asserted
            v = {n: tape.vars[n].tensor.detach().cpu().numpy().astype(np.float64) for n in tape.vars}
            mine = {n: x.astype(np.float64) for n, x in eng.get_params().items()}
            out['max_parameter_difference_fused_tape_after_steps'] = {n: float(np.max(np.abs(v[n] - mine[n]))) for n in mine}
            out['steps_compared'] = done
            users = torch.arange(a.serve_users, dtype=torch.int32, device=eng.device) % eng.n_users
            raw = ds.unique('user').values_list('user', to_list=True)[:a.serve_users]
            out['serve'] = timed_in_turns({'query_rows': lambda k: eng._query_rows(users),
                                           'recommend_batch_n10': lambda k: fused.recommend_batch(raw, n=10)}, 2, max(5, a.reps // 3))[0]
            out['serve']['users'] = int(users.numel())
            res['by_L_blocks'][f'L{L}_blocks{nb}'] = out
            res['n_users'], res['n_items'] = eng.n_users, eng.n_items
    if a.only:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(json.dumps(res, sort_keys=True, indent=1) + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
