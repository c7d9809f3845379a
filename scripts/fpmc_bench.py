"""Time of one FPMC training step at the ml-1m shape (6040 x 3706 synthetic sequences, 4096 windows, r = 4, K = 64, Adam) for L = 1 and
L = 5, three ways in one process:

    fused   FPMC._do_batch: drx_fpmc_step (k_fpmc_fwd_bwd, the grouping of the three key lists, one update launch over three tables)
    tape    the same model written with hooks only — five registered Variables, torch operations in _predict_batch /
            _compute_batch_loss / _compute_reg_loss — on RecommenderABC's generic tape step (torch.autograd, index_add with atomics,
            one drx_opt_dense per variable)
    bpr     drx_bpr_step on the same number of triples (B r: the windows' (u, i, j_k)) at the same K: the step without the
            transition term

    python scripts/fpmc_bench.py [--batch 4096] [--factors 64] [--reps 30] [--out profiles/fpmc_step.json]

The forms train on the same pre-drawn windows (drx_list_sample_device, timed on its own).  Timed by HIP events on the step's stream and
by the host's wall clock around the step with a synchronisation, the forms in turns after warm-up steps; median (min - max).  Nothing
here fixes a ratio: the file records what was measured, next to the bytes the step has to move."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bpr_bench import timed_in_turns  # noqa: E402


def tape_model(weights, device='cuda:0'):
    import torch
    from drecpy_amd.Recommender import RecommenderABC
    from drecpy_amd.Recommender.trainables import Variable

    class TapeFPMC(RecommenderABC):
        """FPMC with the reference's hooks only: no _do_batch"""

        def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
            self.vars = {n: Variable(weights[n], name=n, device=device) for n in ('P', 'M', 'Q', 'N', 'b')}
            self._register_trainables(list(self.vars.values()))

        def _sample_batch(self, batch_size, **kwds):
            return self._batches[0]

        def _predict_batch(self, batch_samples, **kwds):
            u, s, a = (t.long() for t in batch_samples[:3])
            v = {n: x.tensor for n, x in self.vars.items()}
            x = (v['P'][u][:, None, :] * v['Q'][a]).sum(dim=2) + (v['M'][s].mean(dim=1)[:, None, :] * v['N'][a]).sum(dim=2) + v['b'][a]
            return (x[:, :1] - x[:, 1:]).reshape(-1), None

        def _compute_batch_loss(self, predictions, desired_values, **kwds):
            return torch.nn.functional.softplus(-predictions).mean()

        def _compute_reg_loss(self, reg_rate, batch_size, trainable_models, trainable_layers, trainable_weights, **kwds):
            return 0.5 * reg_rate * sum((self.vars[n].tensor ** 2).sum() for n in ('P', 'M', 'Q', 'N'))

        def _predict(self, uid, iid, **kwds):
            return None

    return TapeFPMC(verbose=False)


def necessary_bytes(n_users, n_items, ld, B, L, r, slots=2):
    """bytes one step cannot avoid moving, every row counted once where it is used"""
    row = 4 * ld
    fwd_read = B * ((1 + L) * row + (1 + r) * (2 * row + 4) + (1 + L + 1 + r) * 4)
    fwd_write = B * (2 * row + row + L * row + (1 + r) * 4)
    upd_read_src = B * (row + L * row + 2 * row + (1 + r) * 4)           # (the context row once per window, not once per lookup)
    sweep = (1 + slots) * 2 * (n_users * row + n_items * row + n_items * (2 * row + 4))
    keys = 2 * 4 * B * (1 + L + 1 + r)                                    # the order lists written by the grouping, read by the update
    return {'fwd_bwd_read': fwd_read, 'fwd_bwd_write': fwd_write, 'of_which_copies_for_M': B * L * row, 'update_gradient_rows_read': upd_read_src,
            'update_table_sweep': sweep, 'key_orders': keys, 'total': fwd_read + fwd_write + upd_read_src + sweep + keys}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--factors', type=int, default=64)
    ap.add_argument('--neg-ratio', type=int, default=4)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--hbm-gbps', type=float, default=6300.0,
                    help='the HBM rate the byte share is stated against (MI355X: about 6.3 TB/s achievable of 8 TB/s nominal)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fpmc_step.json'))
    a = ap.parse_args()

    import torch
    from drecpy_amd import synth
    from drecpy_amd.engine_bpr import BprEngine
    from drecpy_amd.optimizers import Adam
    from drecpy_amd.Recommender.Baseline import FPMC
    ds = synth.dataset('ml-1m', with_timestamp=True)
    B, r = a.batch, a.neg_ratio
    res = {'shape': 'ml-1m (synthetic sequences)', 'batch_windows': B, 'factors': a.factors, 'neg_ratio': r, 'optimizer': 'adam',
           'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup, 'hbm_gbps_assumed': a.hbm_gbps,
           'timed': 'HIP events on the stream and host wall clock around one step with a synchronisation; the forms in turns in one process',
           'by_L': {}}
    fit = dict(epochs=1, batch_size=B, learning_rate=1e-3, neg_ratio=r, reg_rate=1e-3)
    n_steps = a.warmup + a.reps
    for L in (1, 5):
        fused = FPMC(factors=a.factors, L=L, seed=0, verbose=False)
        fused.fit(ds, **fit)
        eng = fused._engine
        weights = eng.get_params()
        eng.set_params(weights)                               # (every form starts from the weights after the fused model's first step)
        for st in eng.state.values():
            for s in st:
                s.zero_()
        batches = [tuple(t.clone() for t in fused._sampler.sample_device(B, 1000 + k)) for k in range(n_steps)]
        tape = tape_model(weights)
        tape._batches = batches
        tape.fit(ds, **dict(fit, epochs=0))                   # registers the variables and the optimizer; no step
        bpr = BprEngine(eng.n_users, eng.n_items, a.factors)
        bpr.set_params({'P': weights['P'], 'Q': weights['Q'], 'bq': weights['b']})
        bpr.set_optimizer(Adam(1e-3))
        triples = [(u.repeat_interleave(r), af[:, 0].repeat_interleave(r).contiguous(), af[:, 1:].reshape(-1).contiguous()) for u, _, af in batches]

        t, done = timed_in_turns({'fused': lambda k: eng.step(k, *batches[k]),
                                  'tape': lambda k: tape._tape_do_batch(batches[k], step=k),
                                  'bpr': lambda k: bpr.step(k, *triples[k])}, a.warmup, a.reps)
        for name, v in t.items():
            v['windows_per_s_at_median_device'] = B / (v['device_ms']['median'] * 1e-3)
        out = dict(t)
        out['sampler'] = timed_in_turns({'s': lambda k: fused._sampler.sample_device(B, 5000 + k)}, 2, a.reps)[0]['s']
        # the fused and the tape form after the same steps on the same windows: the tape's sums run in another order and its Adam
        # counters differ (five applies per step against three), so the scores agree only roughly; recorded, not asserted
        x = eng.score_matrix(np.arange(64, dtype=np.int32)).cpu().numpy()
        v = {n: tape.vars[n].tensor for n in tape.vars}
        q = torch.as_tensor(eng.baskets[:64].cpu().numpy().astype(np.int64), device=v['M'].device)
        m = (v['M'][q.clamp(min=0)] * (q >= 0)[:, :, None]).sum(dim=1) / (q >= 0).sum(dim=1).clamp(min=1)[:, None]
        y = (v['P'][:64] @ v['Q'].T + m @ v['N'].T + v['b'][None, :]).cpu().numpy()
        out['max_score_difference_fused_tape_after_steps'] = float(np.max(np.abs(x - y)))
        out['steps_compared'] = done
        nb = necessary_bytes(eng.n_users, eng.n_items, eng.ld, B, L, r)
        out['necessary_bytes'] = nb
        us = out['fused']['device_ms']['median'] * 1e3
        out['necessary_bytes_time_at_hbm_rate_us'] = nb['total'] / (a.hbm_gbps * 1e3)
        out['share_of_hbm_rate'] = nb['total'] / (a.hbm_gbps * 1e3) / us
        res['by_L'][str(L)] = out
        res['n_users'], res['n_items'] = eng.n_users, eng.n_items
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(json.dumps(res, sort_keys=True, indent=1) + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
