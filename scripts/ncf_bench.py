"""Times of NeuMF at the ml-1m shape (6040 x 3706) with the defaults (factors 8, mlp_factors 32, layers 32-16-8), in one process:

  the step (profiles/ncf_step.json), batch 4096, Adam, two ways:
    fused   NeuMF._do_batch: drx_ncf_step (k_ncf_tile, the small weights' launch, the grouping of the keys, one update launch)
    tape    the same model written with hooks only — registered Variables, torch operations in _predict_batch / _compute_batch_loss /
            _compute_reg_loss — on RecommenderABC's generic tape step (torch.autograd, index_add with atomics, one drx_opt_dense per
            array, the same three apply_gradients per step)
  the scorer (profiles/ncf_scores.json), the logits of 1024 users against all items, two ways:
    fused   NcfEngine.score_matrix: the item half rows, the users' half rows, drx_ncf_score_rows
    torch   the same split formula written with torch operations on the same weights (a [users, items, f_1] tensor, then matmuls)

    python scripts/ncf_bench.py [--shape ml-1m] [--batch 4096] [--users 1024] [--reps 30] [--what step|scores|both]

Both steps train on the same pre-drawn batches (drx_point_sample_recorded, timed on its own), from the same weights; after the steps
their logits are compared.  Timed by HIP events on the stream and by the host's wall clock around one call with a synchronisation, the
two forms in turns after warm-up calls; median (min - max).  Nothing here fixes a ratio: the files record what was measured."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bpr_bench import timed_in_turns                                # noqa: E402


def tape_model(weights, n_layers, device='cuda:0'):
    import torch
    from drecpy_amd.Recommender import RecommenderABC
    from drecpy_amd.Recommender.trainables import TrainableModel, Variable

    class TapeNeuMF(RecommenderABC):
        """NeuMF with the reference's hooks only: no _do_batch"""

        def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
            self.v = {n: Variable(w, name=n, device=device) for n, w in weights.items()}
            # the three registrations of NeuMF: one apply_gradients each, so both forms run on the same Adam counters
            groups = [[self.v[n].tensor for n in self.v if n[0] == c] for c in 'PQ'] + [[self.v[n].tensor for n in self.v if n[0] not in 'PQ']]
            self._register_trainables([TrainableModel(name, lambda g=g: g) for name, g in zip(('user', 'item', 'small'), groups)])

        def _sample_batch(self, batch_size, **kwds):
            return self._batches[0]

        def logits(self, u, i):
            t = {n: v.tensor for n, v in self.v.items()}
            a = torch.cat([t['Pm'][u], t['Qm'][i]], dim=1)
            for l in range(1, n_layers + 1):
                a = torch.relu(a @ t[f'W{l}'] + t[f'b{l}'])
            return (t['Pg'][u] * t['Qg'][i]) @ t['hg'] + a @ t['hm'] + t['b0'][0]

        def _predict_batch(self, batch_samples, **kwds):
            u, i, y = batch_samples[:3]
            return self.logits(u.long(), i.long()), y

        def _compute_batch_loss(self, predictions, desired_values, **kwds):
            return torch.nn.functional.binary_cross_entropy_with_logits(predictions, desired_values)

        def _compute_reg_loss(self, reg_rate, batch_size, trainable_models, trainable_layers, trainable_weights, **kwds):
            return 0.5 * reg_rate * sum((v.tensor ** 2).sum() for n, v in self.v.items() if not n.startswith('b'))

        def _predict(self, uid, iid, **kwds):
            return float(self.logits(torch.tensor([uid], device=device), torch.tensor([iid], device=device))[0])

    return TapeNeuMF(verbose=False)


def torch_scores(eng, uid):
    """the split formula of drx_ncf_score_rows in torch operations: [R, n_items] logits"""
    import torch
    p = {n: torch.as_tensor(v).to(eng.device) for n, v in eng.get_params().items()}
    Km, n = eng.Km, len(eng.layers)

    def run():
        a_u = p['Pm'][uid] @ p['W1'][:Km] + p['b1']
        b_i = p['Qm'] @ p['W1'][Km:]
        a = torch.relu(a_u[:, None, :] + b_i[None, :, :])
        for l in range(2, n + 1):
            a = torch.relu(a @ p[f'W{l}'] + p[f'b{l}'])
        return a @ p['hm'] + (p['Pg'][uid] * p['hg']) @ p['Qg'].T + p['b0'][0]
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=['ml-100k', 'ml-1m'], default='ml-1m')
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--users', type=int, default=1024)
    ap.add_argument('--neg-ratio', type=int, default=4)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--what', choices=['step', 'scores', 'both'], default='both')
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'profiles'))
    a = ap.parse_args()

    import ctypes as C

    import torch
    from drecpy_amd import synth
    from drecpy_amd._lib import check, lib, ptr, stream_ptr
    from drecpy_amd.Recommender.Baseline import NeuMF
    ds = synth.dataset(a.shape, with_timestamp=False)
    fit = dict(epochs=1, batch_size=a.batch, learning_rate=1e-3, neg_ratio=a.neg_ratio, reg_rate=1e-3)
    fused = NeuMF(seed=0, verbose=False)
    fused.fit(ds, **fit)
    eng = fused._engine
    head = {'shape': a.shape, 'n_users': eng.n_users, 'n_items': eng.n_items, 'factors': eng.Kg, 'mlp_factors': eng.Km,
            'layers': list(eng.layers), 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup,
            'timed': 'HIP events on the stream and host wall clock around one call with a synchronisation; the forms in turns in one process'}
    os.makedirs(a.out_dir, exist_ok=True)

    def write(name, res):
        with open(os.path.join(a.out_dir, name), 'w') as f:
            f.write(json.dumps(res, sort_keys=True, indent=1) + '\n')
        print(json.dumps(res))

    if a.what in ('step', 'both'):
        weights = eng.get_params()
        eng.set_params(weights)                               # (both forms start from the weights after the fused model's first step)
        eng.set_optimizer(fused.optimizer)
        for st in eng.state.values():
            for s in st:
                s.zero_()
        tape = tape_model(weights, len(eng.layers))
        n_steps = a.warmup + a.reps
        batches = [tuple(t.clone() for t in eng.sample(a.batch, a.neg_ratio, 1000 + k)) for k in range(n_steps)]
        tape._batches = batches
        tape.fit(ds, **dict(fit, epochs=0))                   # registers the variables and the optimizer; no step
        res = dict(head, batch=a.batch, neg_ratio=a.neg_ratio, optimizer='adam')
        t, done = timed_in_turns({'fused': lambda k: eng.step(k, *batches[k], applies=(3, 0, 1, 2)),
                                  'tape': lambda k: tape._tape_do_batch(batches[k], step=k)}, a.warmup, a.reps)
        for name, r in t.items():
            r['samples_per_s_at_median_wall'] = a.batch / (r['wall_ms']['median'] * 1e-3)
            r['samples_per_s_at_median_device'] = a.batch / (r['device_ms']['median'] * 1e-3)
        res.update(t)
        res['sampler'] = timed_in_turns({'s': lambda k: eng.sample(a.batch, a.neg_ratio, 5000 + k)}, 2, a.reps)[0]['s']
        # the two forms after the same steps on the same batches and the same Adam counters: the tape's sums run in another order (and a
        # pre-activation next to zero may fall on the other side of relu), so the logits agree only roughly; recorded, not asserted
        u = torch.arange(64, device=eng.device)
        x = eng.score_matrix(np.arange(64, dtype=np.int32)).cpu().numpy()
        y = tape.logits(u.repeat_interleave(eng.n_items), torch.arange(eng.n_items, device=eng.device).repeat(64)).reshape(64, -1).cpu().numpy()
        res['max_logit_difference_after_steps'] = float(np.max(np.abs(x - y)))
        res['steps_compared'] = done
        # per sample: 2 table rows read and 2 gradient rows written by k_ncf_tile; 2 (sum of fin * fo) multiply-adds forward, twice that backward
        mults = sum(fi * fo for fi, fo in zip((2 * eng.Km,) + eng.layers[:-1], eng.layers))
        res['tile_bytes_per_sample'] = 4 * eng.ld * 4 + 3 * 4
        res['tile_flop_per_sample'] = 6 * mults
        res['n_small'] = eng.n_small
        res['grid'] = int(lib().drx_ncf_grid(a.batch))
        write('ncf_step.json', res)

    if a.what in ('scores', 'both'):
        R = min(a.users, eng.n_users)
        uid = np.arange(R, dtype=np.int32)
        d_uid = torch.as_tensor(uid.astype(np.int64)).to(eng.device)
        by_torch = torch_scores(eng, d_uid)
        res = dict(head, users=R)
        t, _ = timed_in_turns({'fused': lambda k: eng.score_matrix(uid), 'torch': lambda k: by_torch()}, a.warmup, a.reps)
        ih = eng.half_rows(1)
        uh = eng.half_rows(0, eng._dev_i32(uid))
        out = torch.empty(R, eng.n_items, dtype=torch.float32, device=eng.device)
        def kernel_only(k):
            check(lib().drx_ncf_score_rows(C.byref(eng.dims), ptr(eng.sw), ptr(uh), ptr(ih), R, ptr(out), stream_ptr(eng.device)),
                  'drx_ncf_score_rows')
        t.update(timed_in_turns({'drx_ncf_score_rows': kernel_only}, a.warmup, a.reps)[0])
        pairs = R * eng.n_items
        mults = sum(fi * fo for fi, fo in zip(eng.layers[:-1], eng.layers[1:])) + eng.layers[-1] + eng.Kg + eng.layers[0]
        for name, r in t.items():
            r['pairs_per_s_at_median_device'] = pairs / (r['device_ms']['median'] * 1e-3)
            r['gflop_per_s_at_median_device'] = 2 * mults * pairs / (r['device_ms']['median'] * 1e-3) / 1e9
        res.update(t)
        res['multiply_adds_per_pair'] = mults
        res['out_bytes'] = pairs * 4
        res['max_logit_difference'] = float((eng.score_matrix(uid) - by_torch()).abs().max())
        write('ncf_scores.json', res)


if __name__ == '__main__':
    main()
