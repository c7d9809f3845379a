"""The sampled forward kernel's load rounds (csrc/drx_rows.hpp gather_bag: a round's rows in flight are the next eight KEPT entries of
the history): one prepared and one inline step on tiny tables against oracle/cdae_oracle.py:sparse_step on float64, at the history
lengths, kept counts and batch sizes where a round or a fetch of 32 entries begins or ends.

Gates: those of tests/test_gpu_cdae.py::test_sparse_steps_match_oracle (every parameter within 2e-5 absolute of the oracle, the loss
within 1e-4 relative), applied to the optimizer slots as well; prepared against inline as tests/test_gpu_hot_head.py compares them
(3e-5 absolute); rows the batch does not name keep their bits; the same step twice is bit-equal."""
import numpy as np
import pytest
import torch

from oracle import cdae_oracle as co
from helpers import batch_rows, hash_u32, q_threshold

pytestmark = pytest.mark.gpu

U, N = 64, 300
# users 0..10: the borders of a round of 8 rows and of the 32 entries a group fetches at once; the other users: short histories
EDGE_LENGTHS = [0, 1, 7, 8, 9, 16, 17, 31, 32, 33, 70]
ATOL, ATOL_PREPARED_INLINE, LOSS_REL = 2e-5, 3e-5, 1e-4


def _history(rng):
    lens = EDGE_LENGTHS + [int(x) for x in rng.integers(0, 13, size=U - len(EDGE_LENGTHS))]
    rows = [np.sort(rng.choice(N, size=d, replace=False)) for d in lens]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32), np.asarray(lens)


def _batch_ids(rng, B, users):
    """users: 'unique' (every user and item once: every V / W2T row is updated in place by the forward kernel), 'repeated' (users and
    items several times: those rows go through the list), 'long' (histories of 31 .. 70 only: one workgroup per triple)."""
    if users == 'long':
        return np.resize(np.array([7, 8, 9, 10]), B), rng.integers(0, N, size=B)
    if users == 'unique':
        assert B <= U
        first = [4] if B == 1 else list(range(min(B, len(EDGE_LENGTHS))))          # B = 1: the history of 9
        rest = rng.permutation(np.arange(len(EDGE_LENGTHS), U))[:B - len(first)]
        return np.concatenate([first, rest]).astype(np.int64), rng.choice(N, size=B, replace=False)
    uids = np.concatenate([np.arange(len(EDGE_LENGTHS)), rng.integers(0, U, size=max(0, B - len(EDGE_LENGTHS)))])[:B]
    iids = rng.integers(0, N // 4, size=B)
    if B > 1:
        uids[-1], iids[-1] = uids[0], iids[0]
    return uids.astype(np.int64), iids


def _keep_flags(rng, corrupt, keep_off, seed, q):
    """-> (keep bytes of the whole batch, explicit?).  'explicit': a fifth dropped at random, and every history of 16 or more entries
    keeps exactly 8 or exactly 9 (in turn)."""
    B = len(keep_off) - 1
    if corrupt in ('none', 'hash'):
        thr = q_threshold(q)
        keep = [hash_u32(seed, np.full(keep_off[b + 1] - keep_off[b], b), np.arange(keep_off[b + 1] - keep_off[b])) >= thr for b in range(B)]
        return np.concatenate(keep + [np.zeros(0, bool)]).astype(np.uint8), False
    if corrupt == 'all':
        return np.zeros(keep_off[-1], np.uint8), True
    keep = (rng.random(keep_off[-1]) >= q).astype(np.uint8)
    turn = 0
    for b in range(B):
        d = keep_off[b + 1] - keep_off[b]
        if d >= 16:
            row = np.zeros(d, np.uint8)
            row[rng.choice(d, size=8 + turn % 2, replace=False)] = 1
            keep[keep_off[b]:keep_off[b + 1]] = row
            turn += 1
    return keep, True


def _slots(eng, K, opt):
    f = lambda s: {'W': s[0][:, :K], 'W_': s[1][:, :K].t(), 'V': s[2][:, :K], 'b': s[3][:K], 'b_': s[4]}
    c = lambda d: {k: v.detach().cpu().numpy().copy() for k, v in d.items()}
    return [c(f(eng.s1))] + ([c(f(eng.s2))] if opt == 'adam' else [])


CASES = [  # K, optimizer, B, users, corruption
    (128, 'adagrad', 1, 'unique', 'hash'),
    (128, 'adagrad', 7, 'unique', 'none'),
    (128, 'adagrad', 8, 'unique', 'explicit'),
    (128, 'adagrad', 9, 'unique', 'all'),
    (128, 'adagrad', 9, 'repeated', 'hash'),
    (128, 'adagrad', 33, 'unique', 'explicit'),
    (128, 'adagrad', 257, 'repeated', 'hash'),
    (128, 'adagrad', 257, 'repeated', 'explicit'),
    (128, 'adagrad', 257, 'repeated', 'none'),
    (128, 'adagrad', 257, 'repeated', 'all'),
    (100, 'adagrad', 9, 'unique', 'explicit'),           # padding columns
    (100, 'adagrad', 257, 'repeated', 'hash'),
    (256, 'adagrad', 257, 'repeated', 'explicit'),       # groups of 64 lanes: rounds of consecutive entries
    (50, 'adam', 9, 'unique', 'hash'),                   # the optimizer decided at run time, two slots
    (128, 'adagrad', 9, 'long', 'explicit'),             # one workgroup per triple: its groups split the history
]


@pytest.mark.parametrize('K,opt,B,users,corrupt', CASES)
def test_one_step_prepared_and_inline_match_the_oracle(K, opt, B, users, corrupt):
    rng = np.random.default_rng(1000 + 7 * B + K)
    indptr, indices, lens = _history(rng)
    p0 = co.init_params(rng, U, N, K, np.float64)
    uids, iids = _batch_ids(rng, B, users)
    y = (rng.random(B) < 0.3).astype(np.float32)
    q = 0.0 if corrupt == 'none' else 0.2
    qf, lr, seed = float(np.float32(q)), (1e-3 if opt == 'adam' else 0.05), 4100 + B
    _, keep_off, _ = batch_rows(indptr, indices, uids, N)
    keep, explicit = _keep_flags(rng, corrupt, keep_off, seed, q)
    _, _, kept = batch_rows(indptr, indices, uids, N, keep)
    per_workgroup = keep_off[-1] // B > 64 or (B <= 8192 and keep_off[-1] // B > 16)      # csrc/drx_prep.hpp forward_per_workgroup
    assert per_workgroup == (users == 'long')
    if corrupt == 'explicit' and B >= 7:
        assert {8, 9} <= {len(k) for k in kept}
    if corrupt == 'all':
        assert not any(len(k) for k in kept)

    # the reference, once for both forms of the step
    p = {k: v.copy() for k, v in p0.items()}
    st = co.sparse_state(p, opt)
    lo, _ = co.sparse_step(p, st, 0, uids, iids, y, kept, qf, lr, 1e-3, 'bce', opt)
    want_slots = [st] if opt != 'adam' else [{k: v[0] for k, v in st.items()}, {k: v[1] for k, v in st.items()}]

    def run(prepared):
        from drecpy_amd.engine import CdaeEngine
        eng = CdaeEngine(U, N, K)
        eng.set_params(**p0)
        eng.set_history(indptr, indices)
        eng.init_optimizer(opt, lr, 1e-3)
        before = [t.clone() for t in eng.tables()] + [s.clone() for s in eng.s1]
        if explicit:
            bt, alive = eng.make_batch(uids, iids, y, keep_off=keep_off, keep=keep, q=q)
        else:
            bt, alive = eng.make_batch(uids, iids, y, q=q, mask_seed=seed)
        lg = eng.step_sparse(0, bt, 'bce', want_loss=True, prepared=eng.prepare_sparse(bt) if prepared else None).cpu().numpy()
        torch.cuda.synchronize()
        return eng, before, lg

    touched_w = np.zeros(N, bool); touched_w[[n for k in kept for n in k]] = True
    touched_o = np.zeros(N, bool); touched_o[iids] = True
    touched_u = np.zeros(U, bool); touched_u[uids] = True
    got = {}
    for prepared in (True, False):
        eng, before, lg = run(prepared)
        eng2, _, lg2 = run(prepared)
        after = [t.clone() for t in eng.tables()] + [s.clone() for s in eng.s1]
        for a, b in zip(after, [t for t in eng2.tables()] + list(eng2.s1)):
            assert torch.equal(a, b), prepared                                       # the same step twice
        assert np.array_equal(lg, lg2)
        print(f'prepared={prepared} loss {lg[0]:.9g} oracle {lo:.9g}')
        assert abs(lg[0] - lo) / abs(lo) < LOSS_REL, (prepared, lg, lo)
        g = eng.get_params()
        for k in p:
            print(f'prepared={prepared} {k}: max abs error {np.max(np.abs(g[k] - p[k])):.3g}')
            np.testing.assert_allclose(g[k], p[k], rtol=0, atol=ATOL, err_msg=f'prepared={prepared} {k}')
        for have, want in zip(_slots(eng, K, opt), want_slots):
            for k in want:
                np.testing.assert_allclose(have[k], want[k], rtol=0, atol=ATOL, err_msg=f'prepared={prepared} slot {k}')
        # rows the batch does not name: not written at all (tables W, W2T, V, b2 and their first slots)
        for t, mask in ((0, touched_w), (1, touched_o), (2, touched_u), (4, touched_o)):
            m = torch.as_tensor(~mask, device=after[t].device)
            assert torch.equal(after[t][m], before[t][m]), (prepared, t)
            assert torch.equal(after[5 + t][m], before[5 + t][m]), (prepared, t)
        got[prepared] = g
    for k in p:
        np.testing.assert_allclose(got[True][k], got[False][k], rtol=0, atol=ATOL_PREPARED_INLINE, err_msg=k)
