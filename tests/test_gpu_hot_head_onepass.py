"""The hot head's partial products in one pass over dz1: a wave takes a strip of 16 columns and up to 64 hot
rows (four 16 x 16 MFMA tiles), the waves of the first row group also leave the hidden bias's column sums and the loss partials, and the
touch kernel looks hot items up in a table in LDS.  Shapes, oracle and gates are tests/test_gpu_hot_head.py's: U = 30 000, N = 400
unless said otherwise, 3 steps, oracle.cdae_oracle.sparse_step, atol 3e-5 on every parameter (b included), loss relative 1e-4 (asserted
inside _run at every step)."""
import numpy as np
import pytest
import torch

import test_gpu_hot_head as hh
from test_gpu_hot_head import _run

ATOL = 3e-5


def _assert_oracle(g, p):
    for k in p:
        np.testing.assert_allclose(g[k], p[k], rtol=0, atol=ATOL, err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize('prepared', [False, True])
@pytest.mark.parametrize('K,H,B', [(64, 32, 1000), (128, 32, 2048), (128, 64, 1000), (125, 64, 2000), (128, 128, 1000), (64, 128, 2048)])
def test_one_pass_partials_match_oracle(K, H, B, prepared):
    """H = 32: two row tiles instead of four.  B = 1000 / 2000: a last slice of 488 / 464 samples and k-steps that run past the batch.
    K = 125: columns padded to 128.  H = 128: two row groups, each a pass of its own over dz1 — the bias's column sums (and the loss
    partials) must come from the first alone.  K = 64: four column strips and eight waves per workgroup."""
    _, p, g, _ = _run(K, H, prepared, B=B)
    _assert_oracle(g, p)


@pytest.mark.gpu
def test_no_hot_row_kept_bias_and_loss_still_come_from_the_pass():
    """Every user of the batch has a history without a hot item: all mask words are zero, the k-steps still run (their dz1 values are the
    bias's), b, the loss and every table match the oracle, and no hot row or accumulator row is written."""
    def users_without_hot(eng, indptr, indices, rng, B):
        hot = np.zeros(eng.n_items, dtype=bool)
        hot[eng._hot_item.cpu().numpy()] = True
        has = np.zeros(len(indptr) - 1, dtype=np.int64)
        np.add.at(has, np.repeat(np.arange(len(indptr) - 1), np.diff(indptr)), hot[indices])
        ok = np.flatnonzero((has == 0) & (np.diff(indptr) > 0))
        assert len(ok) > 0
        return rng.choice(ok, size=B)

    eng0, _, _, _ = _run(128, 64, True, steps=0, oracle=False, B=1000)
    w0, a0 = eng0.W.clone(), eng0.s1[0].clone()
    eng, p, g, _ = _run(128, 64, True, B=1000, uids_of=users_without_hot)
    _assert_oracle(g, p)
    hot = eng._hot_item.long()
    assert torch.equal(eng.W[hot], w0[hot])
    assert torch.equal(eng.s1[0][hot], a0[hot])
    assert not torch.equal(eng.W, w0)


@pytest.mark.gpu
@pytest.mark.parametrize('prepared', [False, True])
def test_nearly_every_item_hot(prepared):
    """N = 1100, H = 1024: sixteen row groups, the largest lookup table (4096 entries) and a nearly empty touch list."""
    eng, p, g, _ = _run(128, 1024, prepared, N=1100, B=1000)
    assert eng.hot_rows == 1024
    _assert_oracle(g, p)


@pytest.mark.gpu
def test_hot_ids_at_both_ends_of_the_catalogue(monkeypatch):
    """Items 0 and N - 1 among the hot ones: the ids at both ends of the key range are found in the lookup table."""
    N = 400
    synth = hh.synth_history

    def ends_hot(rng, n_users, n_items, mean_deg, **kw):
        indptr, indices = synth(rng, n_users, n_items, mean_deg, **kw)
        deg = np.bincount(indices, minlength=n_items)
        top = np.argsort(-deg, kind='stable')
        new_id = np.arange(n_items)
        for item, end in ((int(top[0]), 0), (int(top[1]), n_items - 1)):       # the two most frequent items trade ids with the ends
            other = int(np.flatnonzero(new_id == end)[0])
            new_id[other], new_id[item] = new_id[item], end
        new = new_id[indices]
        for u in range(n_users):                                               # (sorted columns per row, as synth_history leaves them)
            new[indptr[u]:indptr[u + 1]].sort()
        return indptr, new.astype(np.int32)

    monkeypatch.setattr(hh, 'synth_history', ends_hot)
    eng, p, g, _ = _run(128, 64, True, N=N, B=1000)
    hot = set(eng._hot_item.cpu().numpy().tolist())
    assert 0 in hot and N - 1 in hot
    _assert_oracle(g, p)


@pytest.fixture(scope='module')
def head_on_prepared():
    return _run(128, 64, True, oracle=False, B=2000)


@pytest.mark.gpu
def test_two_runs_are_bit_equal(head_on_prepared):
    _, _, _, t1 = head_on_prepared
    _, _, _, t2 = _run(128, 64, True, oracle=False, B=2000)
    for a, b in zip(t1, t2):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_head_on_off_and_prepared_inline_agree(head_on_prepared):
    _, _, g_on, _ = head_on_prepared
    _, _, g_off, _ = _run(128, 0, True, oracle=False, B=2000)
    _, _, g_in, _ = _run(128, 64, False, oracle=False, B=2000)
    for k in g_on:
        np.testing.assert_allclose(g_on[k], g_off[k], rtol=0, atol=ATOL, err_msg='head off: ' + k)
        np.testing.assert_allclose(g_in[k], g_on[k], rtol=0, atol=ATOL, err_msg='inline: ' + k)
