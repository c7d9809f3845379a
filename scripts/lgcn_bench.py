"""Time of one LightGCN training step at the ml-1m shape (6040 x 3706 synthetic, about 10^6 edges, K = 64, 4096 pairs x 4 negatives, Adam)
for 1, 2 and 3 layers, in one process, of the propagation kernel alone and of serving 1024 users:

    fused      LgcnEngine.step: drx_lgcn_step (2 x layers propagations over the whole graph, the triple kernel, the grouping of the 3 T
               node keys, the dense gradient, drx_opt_dense on both halves)
    tape       the same model written with hooks only — two registered Variables, torch.sparse.mm over a coalesced adjacency in
               _predict_batch — on RecommenderABC's generic tape step (torch.autograd, one drx_opt_dense per variable)
    bpr        drx_bpr_step on the same triples: what a step without propagation costs
    propagate  drx_lgcn_propagate alone: time per call and gathered bytes per second (entries x ld x 4 B over the time)
    serve      drx_lgcn_final, and LightGCN.recommend_batch (n = 10) for 1024 users with and without the cached final embeddings

    python scripts/lgcn_bench.py [--reps 30] [--out profiles/lgcn_step.json]

The forms train on the same pre-drawn triples.  Timed by HIP events on the step's stream and by the host's wall clock around the step with
a synchronisation, the forms in turns after warm-up steps; median (min - max).  Nothing here fixes a ratio: the file records what was
measured, and per point whether the fused step's slowest run is faster than the tape step's fastest."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bpr_bench import timed_in_turns  # noqa: E402


def tape_model(weights, adjacency, n_users, layers, device='cuda:0'):
    import torch
    from drecpy_amd.Recommender import RecommenderABC
    from drecpy_amd.Recommender.trainables import Variable

    class TapeLightGCN(RecommenderABC):
        """LightGCN with the reference's hooks only: no _do_batch"""

        def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
            self.P, self.Q = (Variable(weights[n], name=n, device=device) for n in ('P', 'Q'))
            self._register_trainables([self.P, self.Q])

        def _sample_batch(self, batch_size, **kwds):
            return self._batches[0]

        def final(self):
            total = term = torch.cat([self.P.tensor, self.Q.tensor])
            for _ in range(layers):
                term = torch.sparse.mm(adjacency, term)
                total = total + term
            return total / (layers + 1)

        def _predict_batch(self, batch_samples, **kwds):
            u, i, j = (t.long() for t in batch_samples[:3])
            E = self.final()
            return (E[u] * (E[n_users + i] - E[n_users + j])).sum(dim=1), None

        def _compute_batch_loss(self, predictions, desired_values, **kwds):
            return torch.nn.functional.softplus(-predictions).mean()

        def _compute_reg_loss(self, reg_rate, batch_size, trainable_models, trainable_layers, trainable_weights, **kwds):
            return 0.5 * reg_rate * ((self.P.tensor ** 2).sum() + (self.Q.tensor ** 2).sum())

        def _predict(self, uid, iid, **kwds):
            return None

    return TapeLightGCN(verbose=False)


def coalesced_adjacency(graph, device):
    """the engine's graph as a coalesced torch sparse matrix [N, N] of w[r] w[c]"""
    import torch
    indptr, indices, w = (a.cpu() for a in graph._arrays[:3])
    rows = torch.repeat_interleave(torch.arange(graph.N), indptr[1:] - indptr[:-1])
    cols = indices[:graph.nnz2].long()
    return torch.sparse_coo_tensor(torch.stack([rows, cols]), w[rows] * w[cols], (graph.N, graph.N)).coalesce().to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16384, help='triples per step: 4096 drawn pairs x 4 negatives')
    ap.add_argument('--factors', type=int, default=64)
    ap.add_argument('--neg-ratio', type=int, default=4)
    ap.add_argument('--layers', type=int, nargs='+', default=[1, 2, 3])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--serve-users', type=int, default=1024)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lgcn_step.json'))
    a = ap.parse_args()

    import torch
    from drecpy_amd import synth
    from drecpy_amd._lib import check, lib, ptr, stream_ptr
    from drecpy_amd.Recommender.Baseline import LightGCN
    from drecpy_amd.engine_bpr import BprEngine
    ds = synth.dataset('ml-1m', with_timestamp=False)
    fit = dict(epochs=1, batch_size=a.batch, learning_rate=1e-3, neg_ratio=a.neg_ratio, reg_rate=1e-3)
    n_steps = a.warmup + a.reps
    res = {'shape': 'ml-1m (synthetic)', 'triples': a.batch, 'pairs': a.batch // a.neg_ratio, 'neg_ratio': a.neg_ratio, 'factors': a.factors,
           'optimizer': 'adam', 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup,
           'row_split': int(lib().drx_lgcn_row_split()),
           'timed': 'HIP events on the stream and host wall clock around one step with a synchronisation; the forms in turns in one process',
           'by_layers': {}}
    for layers in a.layers:
        fused = LightGCN(factors=a.factors, layers=layers, seed=0, verbose=False)
        fused.fit(ds, **fit)
        eng = fused._engine
        g = eng._graph
        weights = eng.get_params()
        eng.set_params(weights)                               # (every form starts from the weights after the fused model's first step)
        eng.set_optimizer(fused.optimizer)
        for st in eng.state.values():
            for s in st:
                s.zero_()
        deg = np.diff(g._arrays[0].cpu().numpy())
        res.update(n_users=eng.n_users, n_items=eng.n_items, edges=g.nnz2 // 2, segments=g.n_seg, cut_rows=g.n_cut,
                   longest_user_row=int(deg[:eng.n_users].max()), longest_item_row=int(deg[eng.n_users:].max()),
                   mean_user_row=float(deg[:eng.n_users].mean()), mean_item_row=float(deg[eng.n_users:].mean()))
        batches = [tuple(t.clone() for t in eng.sample(a.batch, a.neg_ratio, 1000 + k)) for k in range(n_steps)]
        bpr = BprEngine(eng.n_users, eng.n_items, a.factors)
        bpr.set_params(dict(weights, bq=np.zeros(eng.n_items)))
        bpr.set_optimizer(fused.optimizer)
        bpr.lr, bpr.reg = eng.lr, eng.reg
        forms = {'fused': lambda k: eng.step(k, *batches[k]), 'bpr': lambda k: bpr.step(k, *batches[k])}
        out = {}
        try:
            tape = tape_model(weights, coalesced_adjacency(g, eng.device), eng.n_users, layers)
            tape._batches = batches
            tape.fit(ds, **dict(fit, epochs=0))               # registers the variables and the optimizer; no step
            tape._tape_do_batch(batches[0], step=0)        # (one step outside the clock: a failure here is recorded below)
            tape.P.assign(weights['P'])
            tape.Q.assign(weights['Q'])
            forms['tape'] = lambda k: tape._tape_do_batch(batches[k], step=k)
        except Exception as err:                              # recorded, never hidden: the comparison is then absent from the file
            out['tape_error'] = f'{type(err).__name__}: {err}'
        t, done = timed_in_turns(forms, a.warmup, a.reps)
        for v in t.values():
            v['triples_per_s_at_median_device'] = a.batch / (v['device_ms']['median'] * 1e-3)
        out.update(t)
        out['steps_compared'] = done
        out['fused_over_bpr_device'] = t['fused']['device_ms']['median'] / t['bpr']['device_ms']['median']
        if 'tape' in t:
            out['fused_over_tape_device'] = t['fused']['device_ms']['median'] / t['tape']['device_ms']['median']
            # beyond the recorded spread: the fused step's slowest run against the tape step's fastest
            out['fused_beats_tape_beyond_the_spread'] = bool(t['fused']['device_ms']['max'] < t['tape']['device_ms']['min'])
            x = eng.score_matrix(np.arange(64, dtype=np.int32)).cpu().numpy()
            E = tape.final()
            out['max_score_difference_after_steps'] = float(np.max(np.abs(x - (E[:64] @ E[eng.n_users:].T).detach().cpu().numpy())))
        res['by_layers'][str(layers)] = out
    # the propagation alone, on the last engine's graph and table
    part_bytes = int(lib().drx_lgcn_part_bytes(C.byref(g.struct), eng.ld))
    part = torch.empty(part_bytes, dtype=torch.uint8, device=eng.device)
    dst = torch.empty_like(eng.E0)

    def propagate(k):
        check(lib().drx_lgcn_propagate(C.byref(g.struct), ptr(eng.E0), ptr(eng.E0), ptr(dst), eng.ld, 1.0, ptr(part), part_bytes,
                                       stream_ptr(eng.device)), 'drx_lgcn_propagate')
    p = timed_in_turns({'propagate': propagate}, a.warmup, a.reps)[0]['propagate']
    p['gathered_bytes'] = g.nnz2 * eng.ld * 4
    p['gathered_bytes_per_s_at_median_device'] = p['gathered_bytes'] / (p['device_ms']['median'] * 1e-3)
    p['gathered_bytes_per_s_at_min_device'] = p['gathered_bytes'] / (p['device_ms']['min'] * 1e-3)
    res['propagate'] = p
    raw = ds.unique('user').values_list('user', to_list=True)[:a.serve_users]

    def final(k):
        eng._ebar = None
        eng.final_embeddings()

    def served_fresh(k):
        eng._ebar = None
        fused.recommend_batch(raw, n=10)
    res['serve'] = timed_in_turns({'final': final, 'final_and_recommend_batch_n10': served_fresh,
                                   'recommend_batch_n10_cached': lambda k: fused.recommend_batch(raw, n=10)}, 2, max(5, a.reps // 3))[0]
    res['serve'].update(users=len(raw), layers=eng.layers)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(json.dumps(res, sort_keys=True, indent=1) + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
