"""Time of one GRU4Rec training step at the ml-1m shape (6040 x 3706 synthetic sequences, 4096 windows, r = 4, K = H = 64, Adam) for
L = 1, 5 and 8, three ways in one process, and of serving 1024 users:

    fused   GRU4Rec._do_batch: drx_gru_step (k_gru_tile, the small-weight launch, the grouping of the two key lists, one update launch
            over E and Q with b)
    tape    the same model written with hooks only — seven registered Variables, torch operations in _predict_batch /
            _compute_batch_loss / _compute_reg_loss — on RecommenderABC's generic tape step (torch.autograd through the L cells,
            index_add with atomics, one drx_opt_dense per variable)
    fpmc    drx_fpmc_step on the same windows at the same K: what the table-update half costs without a recurrence
    serve   drx_gru_query_rows for 1024 users, and GRU4Rec.recommend_batch (n = 10) for them

    python scripts/gru_bench.py [--batch 4096] [--factors 64] [--hidden 64] [--reps 30] [--out profiles/gru_step.json]

The forms train on the same pre-drawn windows (drx_list_sample_device).  Timed by HIP events on the step's stream and by the host's wall
clock around the step with a synchronisation, the forms in turns after warm-up steps; median (min - max).  Nothing here fixes a ratio:
the file records what was measured.  (The tile kernel's share of the step comes from a kernel trace of this script's fused steps,
`--only fused`; DESIGN.md section 3.11 quotes it.)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bpr_bench import timed_in_turns  # noqa: E402

NAMES = ('E', 'Wx', 'Wh', 'bx', 'bhn', 'Q', 'b')


def tape_model(weights, device='cuda:0'):
    import torch
    from drecpy_amd.Recommender import RecommenderABC
    from drecpy_amd.Recommender.trainables import Variable

    class TapeGRU4Rec(RecommenderABC):
        """GRU4Rec with the reference's hooks only: no _do_batch"""

        def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
            self.vars = {n: Variable(weights[n], name=n, device=device) for n in NAMES}
            self._register_trainables(list(self.vars.values()))

        def _sample_batch(self, batch_size, **kwds):
            return self._batches[0]

        def _predict_batch(self, batch_samples, **kwds):
            _, s, a = (t.long() for t in batch_samples[:3])
            v = {n: x.tensor for n, x in self.vars.items()}
            H = v['Wh'].shape[0]
            h = torch.zeros(s.shape[0], H, dtype=v['E'].dtype, device=v['E'].device)
            for t in range(s.shape[1]):
                px, ph = v['E'][s[:, t]] @ v['Wx'] + v['bx'], h @ v['Wh']
                z, r = torch.sigmoid(px[:, :H] + ph[:, :H]), torch.sigmoid(px[:, H:2 * H] + ph[:, H:2 * H])
                n = torch.tanh(px[:, 2 * H:] + r * (ph[:, 2 * H:] + v['bhn']))
                h = (1.0 - z) * n + z * h
            x = (h[:, None, :] * v['Q'][a]).sum(dim=2) + v['b'][a]
            return (x[:, :1] - x[:, 1:]).reshape(-1), None

        def _compute_batch_loss(self, predictions, desired_values, **kwds):
            return torch.nn.functional.softplus(-predictions).mean()

        def _compute_reg_loss(self, reg_rate, batch_size, trainable_models, trainable_layers, trainable_weights, **kwds):
            return 0.5 * reg_rate * sum((self.vars[n].tensor ** 2).sum() for n in ('E', 'Wx', 'Wh', 'Q'))

        def _predict(self, uid, iid, **kwds):
            return None

    return TapeGRU4Rec(verbose=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--factors', type=int, default=64)
    ap.add_argument('--hidden', type=int, default=64)
    ap.add_argument('--neg-ratio', type=int, default=4)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--serve-users', type=int, default=1024)
    ap.add_argument('--windows', type=int, nargs='+', default=[1, 5, 8])
    ap.add_argument('--only', choices=['fused'], default=None, help='run the fused steps alone and write no file (for a kernel trace)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gru_step.json'))
    a = ap.parse_args()

    import torch
    from drecpy_amd import synth
    from drecpy_amd.engine_fpmc import FpmcEngine
    from drecpy_amd.optimizers import Adam
    from drecpy_amd.Recommender.Baseline import GRU4Rec
    ds = synth.dataset('ml-1m', with_timestamp=True)
    B, r = a.batch, a.neg_ratio
    res = {'shape': 'ml-1m (synthetic sequences)', 'batch_windows': B, 'factors': a.factors, 'hidden': a.hidden, 'neg_ratio': r,
           'optimizer': 'adam', 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup,
           'timed': 'HIP events on the stream and host wall clock around one step with a synchronisation; the forms in turns in one process',
           'by_L': {}}
    fit = dict(epochs=1, batch_size=B, learning_rate=1e-3, neg_ratio=r, reg_rate=1e-3)
    n_steps = a.warmup + a.reps
    for L in a.windows:
        fused = GRU4Rec(factors=a.factors, hidden=a.hidden, L=L, seed=0, verbose=False)
        fused.fit(ds, **fit)
        eng = fused._engine
        weights = eng.get_params()
        eng.set_params(weights)                               # (every form starts from the weights after the fused model's first step)
        for st in eng.state.values():
            for s in st:
                s.zero_()
        batches = [tuple(t.clone() for t in fused._sampler.sample_device(B, 1000 + k)) for k in range(n_steps)]
        if a.only == 'fused':
            for k in range(n_steps):
                eng.step(k, *batches[k])
            torch.cuda.synchronize()
            continue
        tape = tape_model(weights)
        tape._batches = batches
        tape.fit(ds, **dict(fit, epochs=0))                   # registers the variables and the optimizer; no step
        fp = FpmcEngine(eng.n_users, eng.n_items, a.factors, L)
        rng = np.random.default_rng(0)
        draw = lambda n: rng.normal(0.0, 0.01, size=(n, a.factors))
        fp.set_params({'P': draw(eng.n_users), 'Q': draw(eng.n_items), 'M': draw(eng.n_items), 'N': draw(eng.n_items),
                       'b': np.zeros(eng.n_items)})
        fp.set_optimizer(Adam(1e-3))

        t, done = timed_in_turns({'fused': lambda k: eng.step(k, *batches[k]),
                                  'tape': lambda k: tape._tape_do_batch(batches[k], step=k),
                                  'fpmc': lambda k: fp.step(k, *batches[k])}, a.warmup, a.reps)
        for name, v in t.items():
            v['windows_per_s_at_median_device'] = B / (v['device_ms']['median'] * 1e-3)
        out = dict(t)
        out['fused_over_tape_device'] = t['fused']['device_ms']['median'] / t['tape']['device_ms']['median']
        out['sampler'] = timed_in_turns({'s': lambda k: fused._sampler.sample_device(B, 5000 + k)}, 2, a.reps)[0]['s']
        # the fused and the tape form after the same steps on the same windows: the tape's sums run in another order and its Adam
        # counters differ (seven applies per step against three), so the scores agree only roughly; recorded, not asserted
        v = {n: tape.vars[n].tensor.detach().cpu().numpy().astype(np.float64) for n in tape.vars}
        mine = {n: x.astype(np.float64) for n, x in eng.get_params().items()}
        out['max_parameter_difference_fused_tape_after_steps'] = {n: float(np.max(np.abs(v[n] - mine[n]))) for n in NAMES}
        out['steps_compared'] = done
        # serving
        users = torch.arange(a.serve_users, dtype=torch.int32, device=eng.device) % eng.n_users
        raw = ds.unique('user').values_list('user', to_list=True)[:a.serve_users]
        out['serve'] = timed_in_turns({'query_rows': lambda k: eng._query_rows(users),
                                       'recommend_batch_n10': lambda k: fused.recommend_batch(raw, n=10)}, 2, max(5, a.reps // 3))[0]
        out['serve']['users'] = int(users.numel())
        res['by_L'][str(L)] = out
        res['n_users'], res['n_items'] = eng.n_users, eng.n_items
    if a.only:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(json.dumps(res, sort_keys=True, indent=1) + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
