"""Batched top-n recommendation for CDAE at the headline catalogue: the fused path (CdaeEngine.recommend: drx_cdae_forward for the
hidden rows + drx_cdae_recommend) against the score-matrix path every caller took before it (forward writes [R, N] fp32 predictions,
a host-built [R, N] candidate mask is packed and uploaded, drx_topk reads the matrix back; chunks of 256 users as
ranking_evaluation sizes them) — on the SAME tables, in the same run.  (CdaeEngine.recommend plus the copy of its two result arrays to the
host is what CDAE.recommend_batch runs; the public method adds the raw-id mapping of the returned items on the host.)

    python scripts/recommend_bench.py [--out profiles/recommend_batch.json] [--items 1000000] [--k 128] [--n 10] [--quick]

N = 1 000 000 items, K = 128, n = 10, novelty on (the exclusion CSR = the users' histories of the bench's synthetic set,
drecpy_amd/synth.py); parameters with the spread of a trained model (logit std ~ 1.1).  Fused: R in {1, 64, 1024, 16384}, >= 20
repetitions after warm-up; score-matrix path: R in {1, 64, 1024}, >= 5 at R = 1024 (its host-built masks make 16384 users a matter of
minutes).  Per call: device time (events around the kernels alone, host work between them excluded) and end-to-end wall time
(results on the host).  One process; every timed step runs under a watchdog of its own (faulthandler: the process exits if a step
overruns).  Writes both series, their ratios, the achieved TFLOP/s of the fused path and its fraction of the fp32 matrix peak.

    python scripts/recommend_bench.py --model dmf|caser [--out profiles/recommend_batch_<model>.json] [--n 10] [--quick]

The other two models at the shapes the repository trains (bench_configs.py configuration 3: ml-1m-shaped DMF [64, 32]; configuration 5:
ml-1m-shaped Caser), a fitted model, n = 10, novelty on, R in {1, 64, 1024, all users}: the fused path (DMF / Caser._recommend_batch:
towers / hidden rows once per call + drx_rows_recommend) against the per-user default every caller took before it
(RecommenderABC._recommend_batch: one _recommend per user) on the same model in the same run.  The per-user path is timed on at most 64
users and extrapolated per user beyond that (the JSON says where).  What is timed is the hook — internal user ids in, numpy arrays out —,
which is what recommend_batch runs before it maps items back to raw ids.  Device ms = events around the call on the current stream
(for the per-user path that span includes the host's work between its launches).

    python scripts/recommend_bench.py --ranks [--model dmf|caser] [--out profiles/rank_items.json] [--quick]

Catalogue ranks of given (user, item) pairs (rank_items: drx_rows_rank_items, counting instead of selecting) beside recommend (n = 10)
at the same R from the same run: R = 1 / 64 / 1024 / 16 384 pairs of distinct users at N = 1 M, K = 128, novelty on (CDAE; the engine
calls with the hidden rows, and the two library calls alone on the same rows: k_rank_keys + k_rank_count + k_rank_finish against
k_recommend + k_lists_merge); with --model the hooks _catalogue_ranks / _recommend_batch of the fitted ml-1m-shaped model.

    python scripts/recommend_bench.py --ranks --targets 1,2,4,10,16 [--model dmf|caser] [--out profiles/rank_lists.json] [--quick]

The SAME P = R x T pairs (R users with T ascending items each) through the pair form (rank_items: one query row and one catalogue walk
per pair) and through the list form (rank_lists: one row per user): the library calls alone on the same hidden rows (the pair form in
the engine's chunks of 16 384 rows) and the engine calls, median and min of >= 20 calls each, and whether the two answers are equal.
CDAE, K = 128, at N = 1 M items / R = 16 384 users and at the ml-1m shape (N = 3706, R = 6040); with --model the hook
_catalogue_ranks of the fitted ml-1m-shaped model with the routing forced either way.  Writes the smallest T from which on the list
form is faster at both shapes by more than the spread of the two series (RowsRecommender.RANK_LISTS_MIN_MEAN).

    python scripts/recommend_bench.py --pairs [--model dmf] [--out profiles/pair_scores.json] [--items 1000000] [--quick]

Scores of given (user, item) pairs and nothing else (pair_scores: drx_rows_pair_scores, two rows per pair) beside the only batched route
to the same scores there was before it, rank_items(..., exclude=False) on the same pairs (a 128-item block per target and a counting
walk of the catalogue per pair), and beside one prediction per call on 64 pairs (CDAE: the work of CDAE._predict, a forward over the
catalogue and the row copied to the host; --model dmf: DMF._predict of the fitted model).  CDAE, K = 128, at the ml-1m shape (6040 x
3706) and at --items; P = 4096, 65 536 and 1 048 576 pairs sorted by user, about 160 per user.  Warm-up, then repeated timed calls:
median and min (the spread) of each series; the kernel alone (events around the library call on prepared query rows) with its
achieved GB/s against P x (ld x 4 + 12) bytes plus the distinct query rows.  Writes where pair_scores is slower than rank_items
(nowhere is the gate) and where it is closer than 10x.
"""
import argparse
import faulthandler
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drecpy_amd import synth                                     # noqa: E402
from drecpy_amd.engine import CdaeEngine, pack_mask_bits        # noqa: E402

FP32_MATRIX_PEAK_TF = 155.0          # measured v_mfma_f32_32x32x2_f32 rate of the chip
PARENT_CHUNK = 256                   # ranking_evaluation's chunk at N = 1 M (_RANK_CHUNK_BYTES)


class step:
    """a timed step under its own watchdog"""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *a):
        faulthandler.cancel_dump_traceback_later()


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def fused_call(eng, uid, n):
    """-> (device ms, wall ms)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    idx, val = eng.recommend(uid, n)
    e1.record()
    idx, val = idx.cpu(), val.cpu()
    wall = (time.perf_counter() - t0) * 1e3
    return e0.elapsed_time(e1), wall, idx, val


def matrix_call(eng, uid_host, n, ip, ix):
    """the path before the fused one: per chunk forward -> host mask -> upload -> drx_topk.  Device time = the kernels' events summed."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev_ms = 0.0
    out_i, out_v = [], []
    N = eng.n_items
    for lo in range(0, len(uid_host), PARENT_CHUNK):
        u = uid_host[lo:lo + PARENT_CHUNK]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        _, pred = eng.forward(u)
        ev[1].record()
        cand = np.ones((len(u), N), dtype=bool)
        for j, x in enumerate(u):
            cand[j, ix[ip[x]:ip[x + 1]]] = False
        mask = torch.as_tensor(pack_mask_bits(cand).view(np.int32)).to(eng.device)
        ev[2].record()
        idx, val = eng.topk(pred, n, mask)
        ev[3].record()
        out_i.append(idx.cpu())
        out_v.append(val.cpu())
        dev_ms += ev[0].elapsed_time(ev[1]) + ev[2].elapsed_time(ev[3])
        del pred, mask
    wall = (time.perf_counter() - t0) * 1e3
    return dev_ms, wall, torch.cat(out_i), torch.cat(out_v)


def hook_call(fn, uids, n):
    """-> (device ms, wall ms, idx, val) of one _recommend_batch-shaped call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    idx, val = fn(uids, n, True)
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return e0.elapsed_time(e1), wall, idx, val


def events_ms(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return median(ms)


def dmf_parts(eng, uid, n, reps):
    """where a fused DMF call spends its device time: the item tower over the catalogue, the user tower, the scorer-selector on rows of
    eng.W floats — and the scorer on rows cut to the last factor (what a row stride separate from the row width would save)"""
    from drecpy_amd import _lib
    L = _lib.lib()
    d_uid = torch.as_tensor(uid).to(eng.device)
    all_items = torch.arange(eng.N, dtype=torch.int32, device=eng.device)
    out = {'item_tower_ms': events_ms(lambda: eng._representations(1, all_items), reps),
           'user_tower_ms': events_ms(lambda: eng._representations(0, d_uid), reps)}
    ri, ru = eng._representations(1, all_items), eng._representations(0, d_uid)
    R = int(d_uid.numel())
    oi = torch.empty(R, n, dtype=torch.int32, device=eng.device)
    ov = torch.empty(R, n, dtype=torch.float32, device=eng.device)
    x = eng._excl
    for name, ld in (('scorer_ms_rows_of_W', eng.W), ('scorer_ms_rows_of_last_factor', (eng.factors[0][-1] + 3) // 4 * 4)):
        t, q = ri[:, :ld].contiguous(), ru[:, :ld].contiguous()
        sb = int(L.drx_rows_recommend_scratch_bytes(R, eng.N, ld, n))
        sc = torch.empty(sb, dtype=torch.uint8, device=eng.device)
        out[name] = events_ms(lambda: _lib.check(L.drx_rows_recommend(_lib.ptr(t), None, eng.N, ld, _lib.DRX_REC_CLIP, _lib.ptr(q), _lib.ptr(d_uid), R, n,
                                                                      _lib.ptr(x[0]), _lib.ptr(x[1]), _lib.ptr(oi), _lib.ptr(ov), _lib.ptr(sc), sb,
                                                                      _lib.stream_ptr(eng.device)), 'drx_rows_recommend'), reps)
    out['row_width'], out['last_factor'] = eng.W, eng.factors[0][-1]
    return out


def model_main(a):
    """--model dmf | caser"""
    from bench_configs import frame_of
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender import DMF, Caser
    from drecpy_amd.Recommender.recommender_abc import RecommenderABC
    n = a.n
    with step(600):
        ds = InteractionDataset.read_df(frame_of('ml-1m'), verbose=False)
        if a.model == 'dmf':
            m = DMF(user_factors=[64, 32], item_factors=[64, 32], seed=10, verbose=False)
            m.fit(ds, epochs=2, batch_size=256, learning_rate=1e-3, reg_rate=1e-4, neg_ratio=5)
            config = 'bench_configs.py configuration 3: DMF [64, 32] / [64, 32], ml-1m shape'
        else:
            m = Caser(L=5, T=3, d=50, n_v=4, n_h=16, dropout_rate=0.5, seed=10, verbose=False)
            m.fit(ds, epochs=2, batch_size=4096, learning_rate=5e-3, reg_rate=1e-6, neg_ratio=3)
            config = 'bench_configs.py configuration 5: Caser L = 5, d = 50, ml-1m shape'
        torch.cuda.synchronize()
    crossover = type(m).RECOMMEND_MIN_FUSED_USERS
    m.RECOMMEND_MIN_FUSED_USERS = 1                              # this run measures the fused path at every R
    users = np.arange(m.n_users, dtype=np.int64)
    if a.model == 'caser':
        users = np.array([u for u in users if len(m._user_sequence(int(u))) >= m.L], dtype=np.int64)
    rng = np.random.default_rng(0)
    order = rng.permutation(users)
    fused_fn = m._recommend_batch
    per_user_fn = lambda uids, nn, nov: RecommenderABC._recommend_batch(m, uids, nn, nov)
    res = {'model': a.model, 'config': config, 'n_users': int(m.n_users), 'n_items': int(m.n_items), 'n': n, 'novelty': True,
           'timed': '_recommend_batch(internal user ids, n, novelty) -> numpy arrays; device_ms = events around the call',
           'fused': {}, 'per_user': {}, 'ratio': {}}
    PER_USER_MAX = 64
    keep = {}
    for R in [1, 64, 1024, len(order)]:
        uids = order[:R]
        reps = 5 if a.quick else 20
        with step(240):
            for _ in range(3):
                hook_call(fused_fn, uids, n)
            runs = [hook_call(fused_fn, uids, n) for _ in range(reps)]
        d, w = median([r[0] for r in runs]), median([r[1] for r in runs])
        res['fused'][str(R)] = {'device_ms': d, 'wall_ms': w, 'reps': reps, 'device_ms_min': min(r[0] for r in runs), 'users_per_s': R / (w * 1e-3)}
        keep[R] = runs[-1][2]
        print('fused', R, res['fused'][str(R)], flush=True)
    for R in [1, 64, 1024, len(order)]:
        timed = min(R, PER_USER_MAX)
        uids = order[:timed]
        reps = 2 if a.quick else (3 if timed > 1 else 10)
        with step(500):
            hook_call(per_user_fn, uids[:2], n)
            runs = [hook_call(per_user_fn, uids, n) for _ in range(reps)]
        d, w = median([r[0] for r in runs]) * R / timed, median([r[1] for r in runs]) * R / timed
        res['per_user'][str(R)] = {'device_ms': d, 'wall_ms': w, 'reps': reps, 'users_timed': timed, 'extrapolated_per_user': R > timed,
                                   'users_per_s': R / (w * 1e-3)}
        f = res['fused'][str(R)]
        same = float(np.mean([set(x.tolist()) == set(y.tolist()) for x, y in zip(runs[-1][2], keep[R][:timed])]))
        res['ratio'][str(R)] = {'device': d / f['device_ms'], 'wall': w / f['wall_ms'], 'share_of_users_with_the_same_item_set': same}
        print('per user', R, res['per_user'][str(R)], res['ratio'][str(R)], flush=True)
    res['fused_slower_at'] = [int(R) for R, r in res['ratio'].items() if r['wall'] < 1.0]
    res['min_fused_users'] = crossover
    if a.model == 'dmf':
        with step(240):
            res['parts_at_all_users'] = dmf_parts(m._engine, order.astype(np.int32), n, 5 if a.quick else 20)
    write_result(res, a.out)


def write_result(res, out):
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(text + '\n')


def pair_call(fn):
    """-> (device ms, wall ms) of one engine call whose two result tensors are copied to the host"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    a, b = fn()
    e1.record()
    a, b = a.cpu(), b.cpu()
    wall = (time.perf_counter() - t0) * 1e3
    return e0.elapsed_time(e1), wall


def timed_pair(fn, reps):
    for _ in range(3):
        pair_call(fn)
    runs = [pair_call(fn) for _ in range(reps)]
    return {'device_ms': median([r[0] for r in runs]), 'wall_ms': median([r[1] for r in runs]), 'device_ms_min': min(r[0] for r in runs),
            'reps': reps}


def cdae_engine(U, N, K):
    """the headline catalogue: parameters with the spread of a trained model, the synthetic set's histories as exclusions"""
    dev = torch.device('cuda:0')
    eng = CdaeEngine(U, N, K)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for t, std in ((eng.W, 0.05), (eng.W2T, 2.0 / np.sqrt(K)), (eng.V, 0.5)):
        t[:, :K].copy_(torch.randn(t.shape[0], K, generator=g, device=dev) * std)
    eng.b[:K].copy_(torch.randn(K, generator=g, device=dev) * 0.1)
    eng.b2.copy_(torch.randn(N, generator=g, device=dev) * 0.3)
    ip, ix = synth.synth_history(10_000_000, N, 23.4, 5, 1.05, seed=0, device='cpu', user_hi=U)
    ip, ix = ip.numpy(), ix.numpy()
    eng.set_history(ip, ix, with_transpose=False)
    eng.set_exclusions(ip, ix)
    eng.RECOMMEND_MIN_FUSED_USERS = 1                            # this run measures the fused path at every R
    torch.cuda.synchronize()
    return eng, ip, ix


def ranks_main(a):
    """--ranks: rank_items beside recommend(n) at the same R, CDAE at the headline catalogue"""
    from drecpy_amd import _lib
    L = _lib.lib()
    N, K, n, U = a.items, a.k, a.n, a.users
    with step(300):
        eng, ip, ix = cdae_engine(U, N, K)
    dev = eng.device
    rng = np.random.default_rng(0)
    res = {'n_items': N, 'k': K, 'n': n, 'novelty': True, 'mean_history': float(len(ix) / U),
           'timed': 'engine: CdaeEngine.rank_items / recommend (hidden rows included), results copied to the host; kernels: the library call alone '
                    'on the same hidden rows (drx_rows_rank_items: k_rank_keys + k_rank_count + k_rank_finish; drx_rows_recommend: k_recommend + '
                    'k_lists_merge), events around it',
           'rank_items': {}, 'recommend': {}, 'rank_over_recommend': {}}
    for R in [1, 64, 1024] + ([] if a.quick else [16384]):
        reps = 5 if a.quick else (20 if R >= 16384 else 30)
        uid = torch.as_tensor(rng.choice(U, size=R, replace=False).astype(np.int32)).to(dev)
        items = torch.as_tensor(rng.integers(0, N, R).astype(np.int32)).to(dev)
        with step(400):
            rk = timed_pair(lambda: eng.rank_items(uid, items), reps)
            rc = timed_pair(lambda: eng.recommend(uid, n), reps)
            h = eng._hidden_rows(uid)
            x = eng._excl
            orank, oscore = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.float32, device=dev)
            oidx, oval = torch.empty(R, n, dtype=torch.int32, device=dev), torch.empty(R, n, dtype=torch.float32, device=dev)
            sb = max(int(L.drx_rows_rank_items_scratch_bytes(R, N, eng.ld)), int(L.drx_rows_recommend_scratch_bytes(R, N, eng.ld, n)))
            sc = torch.empty(sb, dtype=torch.uint8, device=dev)
            rk['kernels_ms'] = events_ms(lambda: _lib.check(L.drx_rows_rank_items(
                _lib.ptr(eng.W2T), _lib.ptr(eng.b2), N, eng.ld, _lib.DRX_REC_SIGMOID_BIAS, _lib.ptr(h), _lib.ptr(uid), _lib.ptr(items), R, _lib.ptr(x[0]),
                _lib.ptr(x[1]), _lib.ptr(orank), _lib.ptr(oscore), _lib.ptr(sc), sb, _lib.stream_ptr(dev)), 'drx_rows_rank_items'), reps)
            rc['kernels_ms'] = events_ms(lambda: _lib.check(L.drx_rows_recommend(
                _lib.ptr(eng.W2T), _lib.ptr(eng.b2), N, eng.ld, _lib.DRX_REC_SIGMOID_BIAS, _lib.ptr(h), _lib.ptr(uid), R, n, _lib.ptr(x[0]),
                _lib.ptr(x[1]), _lib.ptr(oidx), _lib.ptr(oval), _lib.ptr(sc), sb, _lib.stream_ptr(dev)), 'drx_rows_recommend'), reps)
            # the two answers agree: the rank of a list's entry is its position
            got, _ = eng.rank_items(uid.repeat_interleave(n)[:4096], oidx.reshape(-1)[:4096])
            same = bool((got.cpu().numpy() == np.tile(np.arange(n), R)[:4096]).all())
        res['rank_items'][str(R)], res['recommend'][str(R)] = rk, rc
        res['rank_over_recommend'][str(R)] = {'kernels': rk['kernels_ms'] / rc['kernels_ms'], 'device': rk['device_ms'] / rc['device_ms'],
                                              'wall': rk['wall_ms'] / rc['wall_ms'], 'rank_of_a_listed_item_is_its_position': same}
        print(R, 'rank_items', rk, 'recommend', rc, res['rank_over_recommend'][str(R)], flush=True)
    res['slower_than_1.25x_recommend_at'] = [int(R) for R, r in res['rank_over_recommend'].items() if r['kernels'] > 1.25]
    write_result(res, a.out)


def spread_ms(fn, reps):
    """events around fn() alone -> {median, min, reps}"""
    fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {'median_ms': median(ms), 'min_ms': min(ms), 'reps': reps}


def faster_beyond_spread(pair, lists, key='median_ms', low='min_ms'):
    """median against median, the min - median distance of both series as the spread"""
    return pair[key] - lists[key] > (pair[key] - pair[low]) + (lists[key] - lists[low])


def smallest_winning_t(shapes, targets, series):
    """the smallest T from which on the list form is faster at every shape, by more than the spread (None: at no measured T)"""
    best = None
    for T in sorted(targets, reverse=True):
        if all(faster_beyond_spread(s[str(T)]['pair'][series], s[str(T)]['lists'][series]) for s in shapes):
            best = T
        else:
            break
    return best


def rank_lists_main(a):
    """--ranks --targets: the same pairs through rank_items and through rank_lists, CDAE at two catalogues"""
    from drecpy_amd import _lib
    L = _lib.lib()
    K = a.k
    targets = [int(t) for t in a.targets.split(',')]
    reps = 5 if a.quick else 20
    res = {'k': K, 'novelty': True, 'targets': targets, 'group': int(L.drx_rows_rank_lists_group(K)),
           'timed': 'kernels: the library calls alone on the same hidden rows, events around them (pair form: drx_rows_rank_items in chunks of '
                    '16 384 rows: k_rank_keys + k_rank_count + k_rank_finish; list form: ONE drx_rows_rank_lists: k_rankl_keys + k_rankl_count + '
                    'k_rankl_finish); engine: CdaeEngine.rank_items / rank_lists (hidden rows included), device = events around the call, wall = '
                    'results on the host.  median / min of `reps` calls after warm-up', 'shapes': {}}
    for name, N, U in (('headline', a.items, a.users), ('ml-1m', 3706, 6040)):
        with step(300):
            eng, ip, ix = cdae_engine(U, N, K)
        dev = eng.device
        rng = np.random.default_rng(0)
        x = eng._excl
        users = torch.as_tensor(np.arange(U, dtype=np.int32)).to(dev)
        h = eng._hidden_rows(users)
        out = {}
        for T in targets:
            lists = np.sort(np.stack([rng.choice(N, size=T, replace=False) for _ in range(U)]), axis=1).astype(np.int32)
            indptr = np.arange(U + 1, dtype=np.int64) * T
            P = U * T
            d_items, d_ip = torch.as_tensor(lists.reshape(-1)).to(dev), torch.as_tensor(indptr).to(dev)
            d_pu = users.repeat_interleave(T).contiguous()
            hp = h.repeat_interleave(T, dim=0).contiguous()
            r1, s1 = torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.float32, device=dev)
            r2, s2 = torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.float32, device=dev)
            chunk = eng.RECOMMEND_CHUNK_USERS
            sb = max(int(L.drx_rows_rank_items_scratch_bytes(min(P, chunk), N, eng.ld)), int(L.drx_rows_rank_lists_scratch_bytes(U, P, N, eng.ld)))
            sc = torch.empty(sb, dtype=torch.uint8, device=dev)

            def pair_kernels():
                for lo in range(0, P, chunk):
                    r = min(chunk, P - lo)
                    _lib.check(L.drx_rows_rank_items(_lib.ptr(eng.W2T), _lib.ptr(eng.b2), N, eng.ld, _lib.DRX_REC_SIGMOID_BIAS, _lib.ptr(hp[lo:]),
                                                     _lib.ptr(d_pu[lo:]), _lib.ptr(d_items[lo:]), r, _lib.ptr(x[0]), _lib.ptr(x[1]), _lib.ptr(r1[lo:]),
                                                     _lib.ptr(s1[lo:]), _lib.ptr(sc), sb, _lib.stream_ptr(dev)), 'drx_rows_rank_items')

            def list_kernels():
                _lib.check(L.drx_rows_rank_lists(_lib.ptr(eng.W2T), _lib.ptr(eng.b2), N, eng.ld, _lib.DRX_REC_SIGMOID_BIAS, _lib.ptr(h), _lib.ptr(users), U,
                                                 _lib.ptr(d_ip), _lib.ptr(d_items), _lib.ptr(x[0]), _lib.ptr(x[1]), _lib.ptr(r2), _lib.ptr(s2), _lib.ptr(sc),
                                                 sb, _lib.stream_ptr(dev)), 'drx_rows_rank_lists')
            with step(600):
                row = {'pairs': P, 'pair': {'kernels': spread_ms(pair_kernels, reps)}, 'lists': {'kernels': spread_ms(list_kernels, reps)}}
                row['equal'] = bool(torch.equal(r1, r2) and torch.equal(s1, s2))
                for form, fn in (('pair', lambda: eng.rank_items(d_pu, d_items)), ('lists', lambda: eng.rank_lists(users, indptr, d_items))):
                    for _ in range(2):
                        pair_call(fn)
                    runs = [pair_call(fn) for _ in range(reps)]
                    row[form]['device'] = {'median_ms': median([r[0] for r in runs]), 'min_ms': min(r[0] for r in runs), 'reps': reps}
                    row[form]['wall'] = {'median_ms': median([r[1] for r in runs]), 'min_ms': min(r[1] for r in runs), 'reps': reps}
            row['pair_over_lists'] = {k: row['pair'][k]['median_ms'] / row['lists'][k]['median_ms'] for k in ('kernels', 'device', 'wall')}
            row['lists_faster_beyond_spread'] = {k: bool(faster_beyond_spread(row['pair'][k], row['lists'][k])) for k in ('kernels', 'device', 'wall')}
            out[str(T)] = row
            print(name, 'T', T, json.dumps(row), flush=True)
        res['shapes'][name] = {'n_items': N, 'users': U, 'mean_history': float(len(ix) / U), 'by_targets': out}
        del eng, h
        torch.cuda.empty_cache()
    by = [s['by_targets'] for s in res['shapes'].values()]
    res['smallest_T_faster_at_both_shapes'] = {k: smallest_winning_t(by, targets, k) for k in ('kernels', 'device', 'wall')}
    res['all_equal'] = all(r['equal'] for s in by for r in s.values())
    res['rank_lists_min_mean_in_the_engine'] = CdaeEngine.RANK_LISTS_MIN_MEAN
    write_result(res, a.out)


def rank_lists_model_main(a):
    """--ranks --targets --model dmf | caser: the hook _catalogue_ranks of a fitted ml-1m-shaped model, the routing forced either way"""
    from drecpy_amd.engine import RowsRecommender
    m, users = fitted_ml1m(a.model)
    rng = np.random.default_rng(0)
    targets = [int(t) for t in a.targets.split(',')]
    reps = 5 if a.quick else 20
    R = min(1024, len(users))
    uids = rng.permutation(users)[:R]
    res = {'model': a.model, 'n_users': int(m.n_users), 'n_items': int(m.n_items), 'users': R, 'novelty': True, 'targets': targets,
           'timed': '_catalogue_ranks(internal user ids, internal item ids, novelty) -> numpy arrays with RANK_LISTS_MIN_MEAN = inf (pair) and 0 '
                    '(lists); device = events around the call', 'by_targets': {}}
    keep = RowsRecommender.RANK_LISTS_MIN_MEAN
    for T in targets:
        pu = np.repeat(uids, T)
        pi = np.concatenate([rng.choice(m.n_items, size=T, replace=False) for _ in uids])
        row, got = {}, {}
        with step(600):
            for form, mean in (('pair', float('inf')), ('lists', 0.0)):
                RowsRecommender.RANK_LISTS_MIN_MEAN = mean
                for _ in range(2):
                    got[form] = m._catalogue_ranks(pu, pi, True)
                runs = [hook_call(lambda *_: m._catalogue_ranks(pu, pi, True), None, None)[:2] for _ in range(reps)]
                row[form] = {'device': {'median_ms': median([r[0] for r in runs]), 'min_ms': min(r[0] for r in runs), 'reps': reps},
                             'wall': {'median_ms': median([r[1] for r in runs]), 'min_ms': min(r[1] for r in runs), 'reps': reps}}
            RowsRecommender.RANK_LISTS_MIN_MEAN = keep
        row['equal'] = bool(np.array_equal(got['pair'][0], got['lists'][0]) and np.array_equal(got['pair'][1], got['lists'][1]))
        row['pair_over_lists'] = {k: row['pair'][k]['median_ms'] / row['lists'][k]['median_ms'] for k in ('device', 'wall')}
        res['by_targets'][str(T)] = row
        print('T', T, json.dumps(row), flush=True)
    write_result(res, a.out)


def fitted_ml1m(model):
    """a fitted ml-1m-shaped DMF / Caser (bench_configs.py configurations 3 / 5) and the internal users the fused hooks answer"""
    from bench_configs import frame_of
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender import DMF, Caser
    with step(600):
        ds = InteractionDataset.read_df(frame_of('ml-1m'), verbose=False)
        if model == 'dmf':
            m = DMF(user_factors=[64, 32], item_factors=[64, 32], seed=10, verbose=False)
            m.fit(ds, epochs=2, batch_size=256, learning_rate=1e-3, reg_rate=1e-4, neg_ratio=5)
        else:
            m = Caser(L=5, T=3, d=50, n_v=4, n_h=16, dropout_rate=0.5, seed=10, verbose=False)
            m.fit(ds, epochs=2, batch_size=4096, learning_rate=5e-3, reg_rate=1e-6, neg_ratio=3)
        torch.cuda.synchronize()
    m.RECOMMEND_MIN_FUSED_USERS = 1
    users = np.arange(m.n_users, dtype=np.int64)
    if model == 'caser':
        users = np.array([u for u in users if len(m._user_sequence(int(u))) >= m.L], dtype=np.int64)
    return m, users


def ranks_model_main(a):
    """--ranks --model dmf | caser: the hooks _catalogue_ranks / _recommend_batch of a fitted ml-1m-shaped model"""
    n = a.n
    m, users = fitted_ml1m(a.model)
    rng = np.random.default_rng(0)
    order = rng.permutation(users)
    res = {'model': a.model, 'n_users': int(m.n_users), 'n_items': int(m.n_items), 'n': n, 'novelty': True,
           'timed': '_catalogue_ranks(internal user ids, internal item ids, novelty) and _recommend_batch(internal user ids, n, novelty) -> numpy '
                    'arrays; device_ms = events around the call', 'rank_items': {}, 'recommend': {}, 'rank_over_recommend': {}}
    for R in [1, 64, 1024, len(order)]:
        uids, iids = order[:R], rng.integers(0, m.n_items, R)
        reps = 5 if a.quick else 20
        with step(400):
            for name, fn in (('rank_items', lambda: m._catalogue_ranks(uids, iids, True)), ('recommend', lambda: m._recommend_batch(uids, n, True))):
                for _ in range(3):
                    fn()
                runs = [hook_call(lambda *_: fn(), None, None)[:2] for _ in range(reps)]
                res[name][str(R)] = {'device_ms': median([r[0] for r in runs]), 'wall_ms': median([r[1] for r in runs]), 'reps': reps}
        res['rank_over_recommend'][str(R)] = {k: res['rank_items'][str(R)][k + '_ms'] / res['recommend'][str(R)][k + '_ms'] for k in ('device', 'wall')}
        print(R, res['rank_items'][str(R)], res['recommend'][str(R)], res['rank_over_recommend'][str(R)], flush=True)
    write_result(res, a.out)


def series_ms(fn, reps, warm=2):
    """-> {device / wall: median_ms, min_ms, max_ms} of fn() -> a device tensor (or a tuple of them), the last one copied to the host"""
    runs = []
    for j in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        (out[-1] if isinstance(out, tuple) else out).cpu()
        wall = (time.perf_counter() - t0) * 1e3
        if j >= warm:
            runs.append((e0.elapsed_time(e1), wall))
    return {name: {'median_ms': median([r[j] for r in runs]), 'min_ms': min(r[j] for r in runs), 'max_ms': max(r[j] for r in runs)}
            for j, name in enumerate(('device', 'wall'))} | {'reps': reps}


def pairs_of(rng, users, n_items, P, per_user=160):
    """P pairs sorted by user (as predict_pairs hands them over): about `per_user` random items for each of P / per_user users"""
    n_u = min(len(users), max(1, P // per_user))
    uid = np.sort(rng.choice(users, size=n_u, replace=False)[rng.integers(0, n_u, P)])
    return uid.astype(np.int32), rng.integers(0, n_items, P).astype(np.int32)


def pairs_shape(a, eng, pair_scores, rank_items, kernel_of, one_prediction, users, n_items, ld):
    """one shape: the three routes at every P; kernel_of(uid, items) -> (a function launching the library call alone, distinct query rows)"""
    dev = eng.device
    rng = np.random.default_rng(0)
    out = {}
    for P in (4096, 65536) + (() if a.quick else (1 << 20,)):
        uid, items = pairs_of(rng, users, n_items, P)
        d_uid, d_items = torch.as_tensor(uid).to(dev), torch.as_tensor(items).to(dev)
        row = {'pairs': P, 'distinct_users': int(len(np.unique(uid))), 'distinct_items': int(len(np.unique(items)))}
        with step(900):
            row['pair_scores'] = series_ms(lambda: pair_scores(d_uid, d_items), 5 if a.quick else 20)
            row['rank_items'] = series_ms(lambda: rank_items(d_uid, d_items), 2 if a.quick else (3 if P > 65536 else 10), warm=1)
            row['equal_scores'] = bool(torch.equal(pair_scores(d_uid, d_items), rank_items(d_uid, d_items)[1]))
            launch, n_q = kernel_of(d_uid, d_items)
            burst = max(1, (1 << 20) // P)                             # back-to-back launches per event pair: a short kernel is not timed alone

            def launches():
                for _ in range(burst):
                    launch()
            k = spread_ms(launches, 5 if a.quick else 30)
            k = {'median_ms': k['median_ms'] / burst, 'min_ms': k['min_ms'] / burst, 'reps': k['reps'], 'launches_per_timing': burst}
            nbytes = P * (ld * 4 + 12) + n_q * ld * 4
            row['kernel'] = k | {'bytes': nbytes, 'gb_per_s': nbytes / (k['median_ms'] * 1e-3) / 1e9,
                                 'bytes_are': 'P x (ld x 4 + 12) + distinct query rows x ld x 4: a table row, two indices and a score per pair, '
                                              'whether or not the row was already in a cache'}
        row['rank_items_over_pair_scores'] = {s: row['rank_items'][s]['median_ms'] / row['pair_scores'][s]['median_ms'] for s in ('device', 'wall')}
        out[str(P)] = row
        print(P, json.dumps(row), flush=True)
    sel = rng.integers(0, len(uid), 64)
    with step(600):
        for j in sel[:3]:
            one_prediction(int(uid[j]), int(items[j]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in sel:
            one_prediction(int(uid[j]), int(items[j]))
        out['one_prediction_per_call'] = {'pairs': 64, 'wall_ms_per_pair': (time.perf_counter() - t0) * 1e3 / 64}
    return out


def pairs_main(a):
    """--pairs: pair_scores beside rank_items(exclude=False) on the same pairs and beside one prediction per call"""
    from drecpy_amd import _lib
    L = _lib.lib()
    res = {'k': a.k, 'model': a.model, 'pairs_per_user': 160,
           'timed': 'engine.pair_scores(uids, items) and engine.rank_items(uids, items, exclude=False) on the same device ids, sorted by user, '
                    'the scores copied to the host: device = events around the call, wall = host clock to the copy; kernel = events around '
                    'drx_rows_pair_scores alone on prepared query rows; median, min and max over the repetitions after warm-up',
           'shapes': {}}
    if a.model == 'cdae':
        for name, U, N in (('ml-1m', 6040, 3706), (f'{a.items} items', a.users, a.items)):
            with step(300):
                eng, _, _ = cdae_engine(U, N, a.k)

            def kernel_of(d_uid, d_items, eng=eng):
                distinct, inverse = torch.unique(d_uid, return_inverse=True)
                q, q_row = eng._hidden_rows(distinct.to(torch.int32).contiguous()), inverse.to(torch.int32).contiguous()
                out = torch.empty(d_uid.numel(), dtype=torch.float32, device=eng.device)
                return (lambda: _lib.check(L.drx_rows_pair_scores(
                    _lib.ptr(eng.W2T), _lib.ptr(eng.b2), eng.n_items, eng.ld, _lib.DRX_REC_SIGMOID_BIAS, _lib.ptr(q), int(q.shape[0]), _lib.ptr(q_row),
                    _lib.ptr(d_items), int(d_uid.numel()), _lib.ptr(out), _lib.stream_ptr(eng.device)), 'drx_rows_pair_scores')), int(q.shape[0])

            def one_prediction(uid, iid, eng=eng):                    # what CDAE._predict runs for one pair
                return eng.forward(np.array([uid], dtype=np.int32))[1][0].cpu().numpy()[iid]
            res['shapes'][name] = {'n_users': U, 'n_items': N} | pairs_shape(
                a, eng, eng.pair_scores, lambda u, i, eng=eng: eng.rank_items(u, i, exclude=False), kernel_of, one_prediction, np.arange(U), N, eng.ld)
            del eng
            torch.cuda.empty_cache()
    else:
        assert a.model == 'dmf', '--pairs: cdae or dmf (Caser has no point predictions)'
        m, users = fitted_ml1m('dmf')
        eng = m._engine

        def kernel_of(d_uid, d_items):
            distinct, inverse = torch.unique(d_uid, return_inverse=True)
            d_it, t_row = torch.unique(d_items, return_inverse=True)
            q, table = eng._representations(0, distinct.to(torch.int32).contiguous()), eng._representations(1, d_it.to(torch.int32).contiguous())
            q_row, t_row = inverse.to(torch.int32).contiguous(), t_row.to(torch.int32).contiguous()
            out = torch.empty(d_uid.numel(), dtype=torch.float32, device=eng.device)
            return (lambda: _lib.check(L.drx_rows_pair_scores(
                _lib.ptr(table), None, int(table.shape[0]), eng.W, _lib.DRX_REC_CLIP, _lib.ptr(q), int(q.shape[0]), _lib.ptr(q_row), _lib.ptr(t_row),
                int(d_uid.numel()), _lib.ptr(out), _lib.stream_ptr(eng.device)), 'drx_rows_pair_scores')), int(q.shape[0])
        res['shapes']['ml-1m'] = {'n_users': int(m.n_users), 'n_items': int(m.n_items)} | pairs_shape(
            a, eng, eng.pair_scores, lambda u, i: eng.rank_items(u, i, exclude=False), kernel_of, m._predict, users, int(m.n_items), eng.W)
    rows = [(name, P, r) for name, s in res['shapes'].items() for P, r in s.items() if isinstance(r, dict) and 'pair_scores' in r]
    res['pair_scores_slower_than_rank_items_at'] = [[name, int(P)] for name, P, r in rows if min(r['rank_items_over_pair_scores'].values()) < 1.0]
    res['closer_than_10x_at'] = [[name, int(P), r['rank_items_over_pair_scores']] for name, P, r in rows
                                 if min(r['rank_items_over_pair_scores'].values()) < 10.0]
    res['all_equal_scores'] = all(r['equal_scores'] for _, _, r in rows)
    write_result(res, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--model', choices=('cdae', 'dmf', 'caser'), default='cdae')
    ap.add_argument('--items', type=int, default=1_000_000)
    ap.add_argument('--k', type=int, default=128)
    ap.add_argument('--n', type=int, default=10)
    ap.add_argument('--users', type=int, default=16384)
    ap.add_argument('--quick', action='store_true', help='fewer repetitions, no R = 16384')
    ap.add_argument('--ranks', action='store_true', help='rank_items beside recommend at the same R (default --out profiles/rank_items.json)')
    ap.add_argument('--targets', default=None, help='with --ranks: T1,T2,...: the same R x T pairs through rank_items and rank_lists '
                                                    '(default --out profiles/rank_lists.json)')
    ap.add_argument('--pairs', action='store_true', help='pair_scores beside rank_items on the same pairs (default --out profiles/pair_scores.json)')
    a = ap.parse_args()
    if a.pairs:
        a.out = a.out or os.path.join('profiles', 'pair_scores.json' if a.model == 'cdae' else f'pair_scores_{a.model}.json')
        return pairs_main(a)
    if a.ranks and a.targets:
        a.out = a.out or os.path.join('profiles', 'rank_lists.json' if a.model == 'cdae' else f'rank_lists_{a.model}.json')
        return rank_lists_main(a) if a.model == 'cdae' else rank_lists_model_main(a)
    if a.ranks:
        a.out = a.out or os.path.join('profiles', 'rank_items.json' if a.model == 'cdae' else f'rank_items_{a.model}.json')
        return ranks_main(a) if a.model == 'cdae' else ranks_model_main(a)
    if a.model != 'cdae':
        return model_main(a)
    N, K, n, U = a.items, a.k, a.n, a.users
    dev = torch.device('cuda:0')
    with step(300):
        eng, ip, ix = cdae_engine(U, N, K)
    rng = np.random.default_rng(0)
    res = {'n_items': N, 'k': K, 'n': n, 'novelty': True, 'mean_history': float(len(ix) / U), 'fused': {}, 'score_matrix': {}, 'ratio': {}}
    fused_rs = [1, 64, 1024] + ([] if a.quick else [16384])
    keep = {}
    for R in fused_rs:
        uid = rng.choice(U, size=R, replace=False).astype(np.int32)
        reps = 5 if a.quick else (20 if R >= 16384 else 30)
        with step(240):
            d_uid = torch.as_tensor(uid).to(dev)
            for _ in range(3):
                fused_call(eng, d_uid, n)
            runs = [fused_call(eng, d_uid, n) for _ in range(reps)]
        d, w = median([r[0] for r in runs]), median([r[1] for r in runs])
        tf = 2.0 * R * N * K / (d * 1e-3) / 1e12
        res['fused'][str(R)] = {'device_ms': d, 'wall_ms': w, 'reps': reps, 'device_ms_min': min(r[0] for r in runs),
                                'tflops': tf, 'fraction_of_fp32_matrix_peak': tf / FP32_MATRIX_PEAK_TF,
                                'users_per_s': R / (w * 1e-3)}
        keep[R] = (uid, runs[-1][2], runs[-1][3])
        print('fused', R, res['fused'][str(R)], flush=True)
    for R in (1, 64, 1024):
        uid = keep[R][0]
        reps = 2 if a.quick else (5 if R == 1024 else 10)
        with step(500):
            matrix_call(eng, uid, n, ip, ix)
            runs = [matrix_call(eng, uid, n, ip, ix) for _ in range(reps)]
        d, w = median([r[0] for r in runs]), median([r[1] for r in runs])
        res['score_matrix'][str(R)] = {'device_ms': d, 'wall_ms': w, 'reps': reps, 'chunk_users': PARENT_CHUNK}
        f = res['fused'][str(R)]
        same = bool(torch.equal(runs[-1][2], keep[R][1]))
        res['ratio'][str(R)] = {'device': d / f['device_ms'], 'wall': w / f['wall_ms'], 'same_items': same}
        print('score matrix', R, res['score_matrix'][str(R)], res['ratio'][str(R)], flush=True)
    slower = [int(R) for R, r in res['ratio'].items() if r['device'] < 1.0 or r['wall'] < 1.0]
    res['fused_slower_at'] = slower
    res['min_fused_users'] = CdaeEngine.RECOMMEND_MIN_FUSED_USERS
    write_result(res, a.out)


if __name__ == '__main__':
    main()
