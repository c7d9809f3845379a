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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--items', type=int, default=1_000_000)
    ap.add_argument('--k', type=int, default=128)
    ap.add_argument('--n', type=int, default=10)
    ap.add_argument('--users', type=int, default=16384)
    ap.add_argument('--quick', action='store_true', help='fewer repetitions, no R = 16384')
    a = ap.parse_args()
    N, K, n, U = a.items, a.k, a.n, a.users
    dev = torch.device('cuda:0')
    with step(300):
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
        eng.RECOMMEND_MIN_FUSED_USERS = 1                        # this run measures the fused path at every R
        torch.cuda.synchronize()
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
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
