"""CDAE.fit() of the parent commit's Python package against the tree's, in one job on one libdrx.so (the library is the same for both):
every table bit for bit, the sampler and corruption streams where fit() leaves them, save / load across the two, and wall time of fit().

    python scripts/cdae_fit_ab.py --parent DIR_WITH_PARENTS_drecpy_amd --out profiles/cdae_fit_ab.json      # the whole comparison
    python scripts/cdae_fit_ab.py --side tree --pkg . --what digests --out one_side.json                        # what the driver starts

Uses public calls plus _corruption_keep, _sampler and _engine, so one file drives both packages; each side runs in processes of its own
(the two packages have one name), the sides alternating.  Digest cases: 64 users x 40 items, K = 24, seed 21, injected weights
(tests/test_gpu_fit.py's quiet-fit case).  Speed: time.perf_counter around fit() ending in a device synchronise, ROUNDS rounds per side of
one warm-up fit + REPS timed ones per configuration; a tree median passes if it is at most the parent's median plus the two series'
min-to-median distances (the rule of scripts/keys_merge_ab.py)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time
from statistics import median

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, REPS = 3, 2
SPEED = ('reference_quiet', 'reference_stepwise', 'sampled_device')
SPEED_NOTE = {'reference_quiet': "bench.hr_at_10's fit: synthetic ml-100k shape, leave-10-out train part, K = 50, 5000 one-batch epochs of 64, the library loop",
              'reference_stepwise': 'the same with fused_fit = False: the Python per-step loop',
              'sampled_device': "mode='sampled', device_sampler=True, K = 128, batch 4096, 2000 epochs on synth.dataset('ml-1m') (6040 x 3706, ~940k rows)"}


def sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def tables(m):
    import torch
    torch.cuda.synchronize()
    return {n: sha(t.cpu().numpy()) for n, t in zip(('W', 'W2T', 'V', 'b', 'b2'), m._engine.tables())}


def streams(m):
    """where the sampler and the corruption stream stand"""
    import numpy as np
    keep_off, keep = m._corruption_keep(np.array([1, 2, 3], np.int32))       # (first: it waits for draws an early stop left in flight)
    nxt = [[int(a), int(b), float(c)] for a, b, c in m._sampler.sample(5)]
    return {'next_samples': nxt, 'keep_off': np.asarray(keep_off).tolist(), 'keep': np.asarray(keep).tolist()}


def digests(side, tmp):
    import numpy as np
    sys.path.insert(1, os.path.join(ROOT, 'tests'))
    from helpers import load_frames
    from oracle import cdae_oracle as co
    from drecpy_amd import optimizers as op
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender import CDAE, MaxValidationValueRule, RecommenderABC
    frame = {k: v.copy() for k, v in load_frames()['pt_int_dense'].items()}
    ds = InteractionDataset.read_df(frame, verbose=False)
    w = co.init_params(np.random.default_rng(5), 64, 40, 24, np.float32)
    out = {}

    def ref(**kw):
        return CDAE(hidden_factors=24, corruption_level=0.3, seed=21, verbose=False, **kw)

    def fit(m, epochs, B=16, **kw):
        m.fit(ds, epochs=epochs, batch_size=B, learning_rate=2e-3, reg_rate=1e-3, neg_ratio=3, initial_weights=w, **kw)
        return m

    def record(name, m, with_streams=True):
        out[name] = {'tables': tables(m)}
        if with_streams:
            out[name]['streams'] = streams(m)

    for epochs in (1, 3, 57):
        record(f'reference_quiet_{epochs}', fit(ref(), epochs))
    m = ref()
    m.fused_fit = False
    record('reference_fused_fit_false', fit(m, 57))
    m = ref()
    m._sample_batch = lambda B, **k: m._sampler.sample(B)            # the reference's plain list of triples: flags drawn in the step
    record('reference_plain_list_batches', fit(m, 9))
    for name, o in (('adagrad', op.Adagrad(0.01)), ('sgd', op.SGD(0.05, momentum=0.9)), ('rmsprop', op.RMSprop(0.01))):
        record(f'reference_optimizer_{name}', fit(ref(), 11, optimizer=o))

    class StopsAtSix(MaxValidationValueRule):
        def stop_training(self, current_epoch, best_computed_epoch, target_epoch, **kwds):
            return current_epoch >= 6
    seen = []
    m = fit(ref(), 20, epoch_callback_fn=lambda model: (seen.append(1), {'val': -abs(len(seen) - 2)})[1], epoch_callback_freq=2,
            early_stopping_rule=StopsAtSix('val'), early_stopping_freq=2)
    record('reference_callback_and_early_stop', m)
    out['reference_callback_and_early_stop']['losses'] = [float(x) for x in m._loss_tracker.epoch_losses]
    m = fit(fit(ref(), 5), 7, B=24)
    record('reference_second_fit_other_batch_size', m)

    def sampled(**kw):
        return CDAE(hidden_factors=24, mode='sampled', seed=21, verbose=False, **kw)
    record('sampled_host_arrays', fit(sampled(), 20, B=256))
    for rule in ('adagrad', 'adam', 'rowwise_adagrad'):
        record(f'sampled_device_{rule}', fit(sampled(device_sampler=True, sparse_optimizer=rule), 20, B=256), with_streams=False)
    record('sampled_device_second_fit_other_batch_size', fit(fit(sampled(device_sampler=True), 6, B=64), 6, B=96), with_streams=False)

    # save here, load on the other side (the driver runs `--what load` there)
    m = fit(ref(), 5)
    users = [ds.uid_to_user(u) for u in range(0, 64, 7)]
    m.save(os.path.join(tmp, f'saved_by_{side}.bin'))
    out['recommend_after_fit'] = [[[float(s), int(i)] for s, i in row] for row in m.recommend_batch(users, n=6)]
    with open(os.path.join(tmp, 'users.json'), 'w') as f:
        json.dump([int(u) for u in users], f)
    again = RecommenderABC.load(os.path.join(tmp, f'saved_by_{side}.bin'))
    out['recommend_after_own_load'] = [[[float(s), int(i)] for s, i in row] for row in again.recommend_batch(users, n=6)]
    return out


def load_other(side, tmp):
    from drecpy_amd.Recommender import RecommenderABC
    other = 'parent' if side == 'tree' else 'tree'
    users = json.load(open(os.path.join(tmp, 'users.json')))
    m = RecommenderABC.load(os.path.join(tmp, f'saved_by_{other}.bin'))
    return {f'recommend_after_load_of_{other}s_file': [[[float(s), int(i)] for s, i in row] for row in m.recommend_batch(users, n=6)]}


def speed(config):
    import numpy as np
    import torch
    from drecpy_amd import synth
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Evaluation import leave_k_out
    from drecpy_amd.Recommender import CDAE
    if config == 'sampled_device':
        ds = synth.dataset('ml-1m', with_timestamp=False)
        make = lambda: CDAE(hidden_factors=128, mode='sampled', device_sampler=True, seed=10, verbose=False)
        kw = dict(epochs=2000, batch_size=4096, learning_rate=0.05, reg_rate=1e-3, neg_ratio=5)
    else:                                                                      # bench.hr_at_10's data set and configuration
        U, N, md, mn, a = synth.SHAPES['ml-100k']
        ip, idx = synth.synth_history(U, N, md + 12, mn, a, seed=0)
        ip, idx = ip.numpy(), idx.numpy()
        rng = np.random.RandomState(0)
        user = np.repeat(np.arange(U), np.diff(ip)) + 1
        perm = rng.permutation(len(user))
        full = InteractionDataset.read_df({'user': user[perm], 'item': (idx.astype(np.int64) + 1)[perm],
                                           'interaction': rng.randint(1, 6, size=len(user))[perm]}, verbose=False)
        ds, _ = leave_k_out(full, k=10, min_user_interactions=10, seed=10, verbose=False)

        def make():
            m = CDAE(hidden_factors=50, corruption_level=0.2, loss='bce', seed=10, verbose=False)
            m.fused_fit = config == 'reference_quiet'
            return m
        kw = dict(epochs=5000, batch_size=64, learning_rate=1e-3, reg_rate=1e-3, neg_ratio=5)
    secs = []
    for rep in range(REPS + 1):                                                # the first is the warm-up
        m = make()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.fit(ds, **kw)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
        del m
    return {'warm_up_s': secs[0], 'fit_s': secs[1:]}


def child(a):
    sys.path.insert(0, os.path.abspath(a.pkg))
    sys.path.insert(1, ROOT)
    import drecpy_amd
    from drecpy_amd import _lib
    assert os.path.dirname(os.path.dirname(os.path.abspath(drecpy_amd.__file__))) == os.path.abspath(a.pkg), drecpy_amd.__file__
    _lib.LIB_PATH = os.path.join(ROOT, 'drecpy_amd', 'libdrx.so')
    doc = digests(a.side, a.tmp) if a.what == 'digests' else load_other(a.side, a.tmp) if a.what == 'load' else speed(a.what)
    with open(a.out, 'w') as f:
        json.dump(doc, f)


def driver(a):
    tmp = os.path.join(os.path.dirname(os.path.abspath(a.out)), 'cdae_fit_ab_parts')
    os.makedirs(tmp, exist_ok=True)
    pkg = {'parent': os.path.abspath(a.parent), 'tree': ROOT}

    def run(side, what, limit):
        part = os.path.join(tmp, f'{side}_{what}_{run.n}.json')
        run.n += 1
        subprocess.run([sys.executable, os.path.abspath(__file__), '--side', side, '--pkg', pkg[side], '--what', what, '--out', part,
                        '--tmp', tmp], check=True, timeout=limit)               # (a side that fails or hangs ends the job: nothing follows it)
        print(side, what, 'done', flush=True)
        return json.load(open(part))
    run.n = 0
    got = {side: run(side, 'digests', 240) for side in ('parent', 'tree')}
    for side in ('parent', 'tree'):
        got[side].update(run(side, 'load', 120))
    p, t = got['parent'], got['tree']
    same = {name: p[name] == t[name] for name in p if not name.startswith('recommend_')}
    same['save_load_parent_file_into_tree'] = t['recommend_after_load_of_parents_file'] == p['recommend_after_fit'] == t['recommend_after_fit']
    same['save_load_tree_file_into_parent'] = p['recommend_after_load_of_trees_file'] == t['recommend_after_fit']
    same['save_load_own_file'] = p['recommend_after_own_load'] == p['recommend_after_fit'] and t['recommend_after_own_load'] == t['recommend_after_fit']
    doc = {'compared': 'sha256 of the five tables per case; for single-GPU cases with a host sampler also the next _sampler.sample(5) and the '
                       'flags of _corruption_keep([1, 2, 3]); recommend_batch lists across save / load',
           'cases_equal': same, 'all_equal': all(same.values()), 'tree': {k: v for k, v in t.items() if not k.startswith('recommend_')}}
    series = {c: {'parent': [], 'tree': []} for c in SPEED}
    for config in SPEED:
        for _ in range(ROUNDS):
            for side in ('parent', 'tree'):
                series[config][side] += run(side, config, 600)['fit_s']
    doc['speed'] = {'timed': f'wall seconds of fit() ending in a device synchronise; {ROUNDS} rounds per side, alternating, of one warm-up fit and '
                             f'{REPS} timed fits in a fresh process', 'rule': 'tree median <= parent median + (parent median - parent min) + (tree median - tree min)'}
    for config, s in series.items():
        mp, mt = median(s['parent']), median(s['tree'])
        limit = mp + (mp - min(s['parent'])) + (mt - min(s['tree']))
        doc['speed'][config] = {'what': SPEED_NOTE[config], 'parent_s': s['parent'], 'tree_s': s['tree'], 'parent_median_s': mp, 'tree_median_s': mt,
                                'limit_s': limit, 'passes': mt <= limit}
    import torch
    doc['device'] = torch.cuda.get_device_name(0)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps({'all_equal': doc['all_equal'], 'unequal': [k for k, v in same.items() if not v],
                      'speed': {c: [doc['speed'][c]['parent_median_s'], doc['speed'][c]['tree_median_s'], doc['speed'][c]['passes']] for c in SPEED}}))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', help="directory that holds the parent commit's drecpy_amd/ (driver)")
    ap.add_argument('--side', choices=('parent', 'tree'))
    ap.add_argument('--pkg')
    ap.add_argument('--what', help='digests | load | ' + ' | '.join(SPEED))
    ap.add_argument('--tmp')
    ap.add_argument('--out', required=True)
    a = ap.parse_args()
    child(a) if a.side else driver(a)
