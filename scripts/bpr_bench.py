"""Time of one BPR training step at the ml-1m shape (6040 x 3706, batch 4096, K = 64, Adam), two ways in one process:

    fused   BPR._do_batch: drx_bpr_step (k_bpr_fwd_bwd, the grouping of the keys, one update launch over both tables)
    tape    the same model written with hooks only — three registered Variables, torch operations in _predict_batch /
            _compute_batch_loss / _compute_reg_loss — on RecommenderABC's generic tape step (torch.autograd, index_add with atomics,
            one drx_opt_dense per variable)

    python scripts/bpr_bench.py [--shape ml-1m] [--batch 4096] [--factors 64] [--reps 30] [--out profiles/bpr_step.json]

Both train on the same pre-drawn batches (drx_bpr_sample, timed on its own), from the same weights; after --reps steps their scores
are compared.  Timed by HIP events on the step's stream and by the host's wall clock around the step with a synchronisation, the two
forms in turns after warm-up steps; median (min - max).  Nothing here fixes a ratio: the file records what was measured."""
import argparse
import json
import os
import sys
import time
from statistics import median

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tape_model(factors, weights, device='cuda:0'):
    import torch
    from drecpy_amd.Recommender import RecommenderABC
    from drecpy_amd.Recommender.trainables import Variable

    class TapeBPR(RecommenderABC):
        """BPR-MF with the reference's hooks only: no _do_batch"""

        def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
            self.P, self.Q, self.bq = (Variable(weights[n], name=n, device=device) for n in ('P', 'Q', 'bq'))
            self._register_trainables([self.P, self.Q, self.bq])

        def _sample_batch(self, batch_size, **kwds):
            return self._batches[0]

        def _predict_batch(self, batch_samples, **kwds):
            u, i, j = (t.long() for t in batch_samples[:3])
            P, Q, b = self.P.tensor, self.Q.tensor, self.bq.tensor
            return (P[u] * (Q[i] - Q[j])).sum(dim=1) + b[i] - b[j], None

        def _compute_batch_loss(self, predictions, desired_values, **kwds):
            return torch.nn.functional.softplus(-predictions).mean()

        def _compute_reg_loss(self, reg_rate, batch_size, trainable_models, trainable_layers, trainable_weights, **kwds):
            return 0.5 * reg_rate * ((self.P.tensor ** 2).sum() + (self.Q.tensor ** 2).sum())

        def _predict(self, uid, iid, **kwds):
            return float((self.P.tensor[uid] * self.Q.tensor[iid]).sum() + self.bq.tensor[iid])

    return TapeBPR(verbose=False)


def timed_in_turns(steps, warmup, reps):
    """{name: device / wall ms} of the callables step(k), taken in turns: step k of every form, then step k + 1"""
    import torch
    k = 0
    for _ in range(warmup):
        for fn in steps.values():
            fn(k)
        k += 1
    dev, wall = {n: [] for n in steps}, {n: [] for n in steps}
    for _ in range(reps):
        for name, fn in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn(k)
            e1.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            dev[name].append(e0.elapsed_time(e1))
        k += 1
    stat = lambda v: {'median': median(v), 'min': min(v), 'max': max(v)}
    return {n: {'device_ms': stat(dev[n]), 'wall_ms': stat(wall[n])} for n in steps}, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=['ml-100k', 'ml-1m'], default='ml-1m')
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--factors', type=int, default=64)
    ap.add_argument('--neg-ratio', type=int, default=4)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bpr_step.json'))
    a = ap.parse_args()

    import torch
    from drecpy_amd import synth
    from drecpy_amd.Recommender.Baseline import BPR
    ds = synth.dataset(a.shape, with_timestamp=False)
    fit = dict(epochs=1, batch_size=a.batch, learning_rate=1e-3, neg_ratio=a.neg_ratio, reg_rate=1e-3)
    fused = BPR(factors=a.factors, seed=0, verbose=False)
    fused.fit(ds, **fit)
    eng = fused._engine
    weights = eng.get_params()
    eng.set_params(weights)                                   # (both forms start from the weights after the fused model's first step)
    eng.set_optimizer(fused.optimizer)
    for st in eng.state.values():
        for s in st:
            s.zero_()
    tape = tape_model(a.factors, weights)
    n_steps = a.warmup + a.reps
    batches = [tuple(t.clone() for t in eng.sample(a.batch, a.neg_ratio, 1000 + k)) for k in range(n_steps)]
    tape._batches = batches
    tape.fit(ds, **dict(fit, epochs=0))                       # registers the variables and the optimizer; no step
    applies = (2, 0, 1)

    def sample(k):
        eng.sample(a.batch, a.neg_ratio, 5000 + k)
    res = {'shape': a.shape, 'n_users': eng.n_users, 'n_items': eng.n_items, 'batch': a.batch, 'factors': a.factors, 'neg_ratio': a.neg_ratio,
           'optimizer': 'adam', 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup,
           'timed': 'HIP events on the stream and host wall clock around one step with a synchronisation; the forms in turns in one process'}
    t, done = timed_in_turns({'fused': lambda k: eng.step(k, *batches[k], applies=applies),
                              'tape': lambda k: tape._tape_do_batch(batches[k], step=k)}, a.warmup, a.reps)
    for name, r in t.items():
        r['triples_per_s_at_median_wall'] = a.batch / (r['wall_ms']['median'] * 1e-3)
        r['triples_per_s_at_median_device'] = a.batch / (r['device_ms']['median'] * 1e-3)
    res.update(t)
    res['sampler'] = timed_in_turns({'drx_bpr_sample': sample}, 2, a.reps)[0]['drx_bpr_sample']
    # the two forms after the same steps on the same batches: the tape's sums run in another order and its Adam counters differ (three
    # applies per step against two), so the scores agree only roughly; recorded, not asserted
    x = eng.score_matrix(np.arange(64, dtype=np.int32)).cpu().numpy()
    y = (tape.P.tensor[:64] @ tape.Q.tensor.T + tape.bq.tensor[None, :]).cpu().numpy()
    res['max_score_difference_after_steps'] = float(np.max(np.abs(x - y)))
    res['steps_compared'] = done
    # bytes k_bpr_fwd_bwd moves per triple: 3 rows read, 2 rows written, ids, biases, scalars and keys
    ld = eng.ld
    res['fwd_bwd_bytes_per_triple'] = 3 * ld * 4 + 2 * ld * 4 + 3 * 4 + 2 * 4 + 2 * 4 + 2 * 4
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(json.dumps(res, sort_keys=True, indent=1) + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
