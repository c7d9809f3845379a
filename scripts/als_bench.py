"""Time of one ALS sweep at the ml-1m shape (6040 x 3706 at its density, alpha = 40, lambda = 0.1), K = 64 and 128, two ways in one
process:

    fused   AlsEngine.sweep: drx_als_gram, drx_als_solve_rows (users), drx_als_gram, drx_als_solve_rows (items); each kernel also timed
            on its own, and drx_als_loss with its extra Gram
    torch   the same sweep as a user would write it with torch on the same GPU: users in batches by descending degree, padded gathers
            and einsum for A and b, torch.linalg.cholesky and cholesky_solve (the index tensors built once, outside the timing)

    python scripts/als_bench.py [--shape ml-1m] [--factors 64 128] [--reps 30] [--out profiles/als_sweep.json]

Timed by HIP events on the stream, the two forms in turns after warm-up sweeps; median (min - max).  The solve kernel is also run with
its accumulation alone and with its factorisation alone, which gives the share of each; neither runs the refinement step.  Those two forms are no part of libdrx.so: this script compiles csrc/drx_als.hip alone with
-DDRX_ALS_BENCH_PARTS into csrc/build/libdrx_als_bench.so (--build-only: that and nothing else; it needs no GPU) and loads it.  The file also holds
the two floors of a half-sweep: the fp32 MFMA time of sum_u n_u Kp^2 multiply-adds at 155 TFLOP/s, and the gathered bytes at 17 TB/s
(rows shared in L2) and 6 TB/s (HBM).  Nothing here fixes a time or a ratio: the file records what was measured."""
import argparse
import json
import os
import subprocess
import sys
from statistics import median

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_F32_FLOPS, L2_BPS, HBM_BPS = 155e12, 17e12, 6.0e12


def bench_lib(build_only=False):
    """csrc/drx_als.hip with the kernel's PARTS template flag exposed (drx_als_bench_solve_rows_parts), built once"""
    import ctypes as C
    from drecpy_amd import build as b
    out = os.path.join(b.OBJ, 'libdrx_als_bench.so')
    if build_only or not os.path.exists(out):
        os.makedirs(b.OBJ, exist_ok=True)
        subprocess.check_call([b.HIPCC, f'--offload-arch={b.ARCH}'] + b.COMMON + ['-DDRX_ALS_BENCH_PARTS', '-shared', os.path.join(b.CSRC, 'drx_als.hip'),
                               '-o', out])
    if build_only:
        return out
    import torch  # noqa: F401  (the HIP runtime of torch first, as drecpy_amd._lib.lib does)
    L = C.CDLL(out)
    L.drx_als_bench_solve_rows_parts.restype = C.c_int
    L.drx_als_bench_solve_rows_parts.argtypes = [C.c_void_p] * 7 + [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int32, C.c_void_p,
                                                 C.c_size_t, C.c_void_p]
    return L


def stat(v):
    return {'median': median(v), 'min': min(v), 'max': max(v)}


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


class TorchSweep:
    """padded batches of each orientation, built once"""

    def __init__(self, eng, batch):
        import torch
        self.eng, self.halves = eng, []
        for indptr, indices, w, order in eng._frame:
            ip, order = indptr.cpu().numpy(), order.cpu().numpy().astype(np.int64)
            deg = np.diff(ip)
            batches = []
            for lo in range(0, len(order), batch):
                rows = order[lo:lo + batch]
                rows = rows[deg[rows] > 0]
                if len(rows) == 0:
                    continue
                width = int(deg[rows].max())
                at = ip[rows][:, None] + np.arange(width)[None, :]
                live = np.arange(width)[None, :] < deg[rows][:, None]
                at = torch.as_tensor(np.where(live, at, 0)).to(eng.device)
                live = torch.as_tensor(live).to(eng.device)
                batches.append((torch.as_tensor(rows).to(eng.device), indices.long()[at], torch.where(live, w[at], torch.zeros_like(w[at])),
                                live.float()))
            self.halves.append(batches)
        self.X, self.Y = eng.X[:, :eng.K].clone(), eng.Y[:, :eng.K].clone()

    def half(self, out, other, batches, lam):
        import torch
        G = other.T @ other + lam * torch.eye(other.shape[1], device=other.device)
        out.zero_()
        for rows, idx, w, live in batches:
            Yg = other[idx]                                               # [B, D, K]
            A = G + torch.einsum('bd,bdk,bdl->bkl', w, Yg, Yg)
            b = torch.einsum('bd,bdk->bk', (1.0 + w) * live, Yg)
            L, info = torch.linalg.cholesky_ex(A)
            if int(info.max()):                                           # (what was wrong with the system, for the record)
                k = int(torch.nonzero(info)[0])
                d = torch.diagonal(A[k])
                raise RuntimeError(f'cholesky failed: batch of {len(rows)} rows x {idx.shape[1]} entries, element {k} info {int(info[k])}, '
                                   f'NaN in other {bool(torch.isnan(other).any())}, in gathered rows {bool(torch.isnan(Yg[k]).any())}, '
                                   f'in A {bool(torch.isnan(A[k]).any())}, diagonal min {float(d.min()):.4g} max {float(d.max()):.4g}, '
                                   f'G diagonal min {float(torch.diagonal(G).min()):.4g}')
            out[rows] = torch.cholesky_solve(b[:, :, None], L)[:, :, 0]

    def sweep(self, lam):
        """one sweep from the engine's current factors (both forms then solve the same systems)"""
        self.X.copy_(self.eng.X[:, :self.eng.K])
        self.Y.copy_(self.eng.Y[:, :self.eng.K])
        self.half(self.X, self.Y, self.halves[0], lam)
        self.half(self.Y, self.X, self.halves[1], lam)


def bench(ds, K, a):
    import torch
    from drecpy_amd._lib import check, ptr, stream_ptr
    from drecpy_amd.Recommender.Baseline import ALS
    model = ALS(factors=K, alpha=40.0, seed=0, verbose=False)
    model.fit(ds, epochs=1, reg_rate=0.1)
    e = model._engine
    L_, sc, st = bench_lib(), e._als_scratch, stream_ptr(e.device)
    fail = torch.zeros(1, dtype=torch.int32, device=e.device)

    def solve(half, parts=3):
        out, other, G = (e.X, e.Y, e.Gy) if half == 0 else (e.Y, e.X, e.Gx)
        ip, ix, w, order = e._frame[half]
        check(L_.drx_als_bench_solve_rows_parts(ptr(out), ptr(other), ptr(G), ptr(ip), ptr(ix), ptr(w), ptr(order), out.shape[0], other.shape[0],
                                          e.ld, e.reg, ptr(fail), parts, ptr(sc), sc.numel(), st), 'drx_als_bench_solve_rows_parts')
    res = {'factors': K, 'ld': e.ld}
    try:
        tsw = TorchSweep(e, a.torch_batch)
        tsw.sweep(e.reg)
        torch.cuda.synchronize()
    except Exception as err:                                               # (recorded: the comparison is then missing from the file)
        tsw, res['torch_error'] = None, f'before the loop: {type(err).__name__}: {err}'[:600]
    t = {k: [] for k in ('sweep', 'gram_items', 'solve_users', 'gram_users', 'solve_items', 'loss', 'torch_sweep')}
    for r in range(a.warmup + a.reps):
        keep = r >= a.warmup
        row = {'sweep': timed(lambda: e.sweep())}
        if tsw is not None:
            try:
                row['torch_sweep'] = timed(lambda: tsw.sweep(e.reg))
            except Exception as err:                                       # (recorded with what the torch form saw)
                tsw, res['torch_error'] = None, f'in sweep {r} of the loop ({a.warmup} warm-up): {type(err).__name__}: {err}'[:600]
                torch.cuda.synchronize()
        row['gram_items'] = timed(lambda: e.gram(e.Y, e.Gy))
        row['solve_users'] = timed(lambda: solve(0))
        row['gram_users'] = timed(lambda: e.gram(e.X, e.Gx))
        row['solve_items'] = timed(lambda: solve(1))
        row['loss'] = timed(lambda: e.loss())
        if keep:
            for k, v in row.items():
                t[k].append(v)
    res['device_ms'] = {k: stat(v) for k, v in t.items() if v}
    assert int(fail.cpu().numpy()[0]) == 0
    # the two parts of the solve kernel, on copies of the state a full half leaves (parts 1 and 2 do not give factors)
    keepX, keepY = e.X.clone(), e.Y.clone()
    parts = {}
    for half, name in ((0, 'users'), (1, 'items')):
        for p, what in ((3, 'whole'), (1, 'accumulate_only'), (2, 'factorise_only')):
            v = []
            for r in range(3 + a.reps):
                e.X.copy_(keepX)
                e.Y.copy_(keepY)
                ms = timed(lambda: solve(half, p))
                if r >= 3:
                    v.append(ms)
            parts[f'{name}_{what}'] = stat(v)
    e.X.copy_(keepX)
    e.Y.copy_(keepY)
    res['solve_parts_device_ms'] = parts
    # floors of each half: Kp = the tile-rounded width the kernel is built for
    nt = next(n for n in (1, 2, 3, 4, 6, 8) if 16 * n >= e.ld)
    Kp = 16 * nt
    floors = {}
    for half, name in ((0, 'users'), (1, 'items')):
        n_entries = int(e._frame[half][0][-1].item())
        floors[name] = {'entries': n_entries, 'Kp': Kp,
                        'mfma_ms_square': 2.0 * n_entries * Kp * Kp / MFMA_F32_FLOPS * 1e3,
                        'mfma_ms_lower_triangle_tiles': 2.0 * n_entries * 256 * (nt * (nt + 1) // 2) / MFMA_F32_FLOPS * 1e3,
                        'gather_ms_l2': n_entries * e.ld * 4 / L2_BPS * 1e3, 'gather_ms_hbm': n_entries * e.ld * 4 / HBM_BPS * 1e3}
    res['floors'] = floors
    if tsw is not None:
        tsw.sweep(e.reg)
        e.sweep()
        x = e.score_matrix(np.arange(64, dtype=np.int32)).cpu().numpy()
        y = (tsw.X[:64] @ tsw.Y.T).cpu().numpy()
        res['max_score_difference_fused_torch'] = float(np.max(np.abs(x - y)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=['ml-100k', 'ml-1m'], default='ml-1m')
    ap.add_argument('--factors', type=int, nargs='+', default=[64, 128])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch-batch', type=int, default=256)
    ap.add_argument('--build-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'als_sweep.json'))
    a = ap.parse_args()
    if a.build_only:
        print(bench_lib(build_only=True))
        return
    import torch
    from drecpy_amd import synth
    ds = synth.dataset(a.shape, with_timestamp=False)
    res = {'shape': a.shape, 'alpha': 40.0, 'lambda': 0.1, 'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'warmup': a.warmup,
           'torch_batch_users': a.torch_batch,
           'timed': 'HIP events on the stream around each call; the fused sweep, the torch sweep and the single kernels in turns in one process',
           'rates_for_floors': {'mfma_f32_flops': MFMA_F32_FLOPS, 'l2_bytes_per_s': L2_BPS, 'hbm_bytes_per_s': HBM_BPS},
           'runs': [bench(ds, K, a) for K in a.factors]}
    res['n_users'], res['n_items'] = ds.count_unique('user'), ds.count_unique('item')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(json.dumps(res, sort_keys=True, indent=1) + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
