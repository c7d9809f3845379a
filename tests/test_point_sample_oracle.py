"""oracle/data_oracle.py::point_sample_counter — the CPU statement of the device point sampler's stream (include/drx.h) — checked for
what a point sampler has to deliver, on the frame the GPU tests compare it with the kernels on (helpers.point_sampler_frame).  It is
written from the header's text and calls nothing of libdrx.so; these properties keep it from being a mere transliteration."""
import time

import numpy as np
import pytest

from helpers import point_sampler_frame
from oracle import data_oracle as do


@pytest.fixture(scope='module')
def frame():
    return point_sampler_frame()


def _draw(f, B, neg_ratio, seed, recorded=True, **kw):
    rec = f['rec'] if recorded else (None, None)
    return do.point_sample_counter(f['pos'][0], f['pos'][1], rec[0], rec[1], f['U'], f['N'], B, neg_ratio, seed, **kw)


def _pairs(indptr, indices, N):
    return np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr)) * N + indices


def test_the_frame_has_every_class_of_user():
    f = point_sampler_frame()
    U, N = f['U'], f['N']
    dr, dp = np.diff(f['rec'][0]), np.diff(f['pos'][0])
    assert (U, N) == (203, 37) and len(dr) == U and len(dp) == U
    assert (dr == 0).sum() == U // 4 and (dr == N).sum() == U // 8
    assert dr[0] == 0 and dr[-1] == N                                  # the first and the last user: not of one class
    assert ((dr > 0) & (dp == 0)).sum() >= 2                           # recorded, yet without a positive
    for u in range(U):
        row = f['rec'][1][f['rec'][0][u]:f['rec'][0][u + 1]]
        assert (np.diff(row) > 0).all()
    assert set(_pairs(*f['pos'][:2], N).tolist()) < set(_pairs(*f['rec'], N).tolist())
    assert f['pos'][2].dtype == np.float32 and set(f['pos'][2].tolist()) == {3.0, 4.0, 5.0}


def test_point_sample_counter_draws_valid_triples(frame):
    """B = 60 000, neg_ratio = 3: no negative is a recorded pair, every positive is a pair of pos and carries that pair's value
    standardised in float32, the negatives' share is neg_ratio / (neg_ratio + 1), nothing runs out of attempts and the retry path of
    both kinds is exercised (a positive attempt is rejected with probability ~0.26, a negative one with ~0.31)."""
    f, B, vmin, vrange = frame, 60_000, 1.0, 4.0
    t0 = time.perf_counter()
    uid, iid, y, attempts, exhausted = _draw(f, B, 3, 12345, values=f['pos'][2], vmin=vmin, vrange=vrange)
    took = time.perf_counter() - t0
    assert uid.dtype == np.int32 and iid.dtype == np.int32 and y.dtype == np.float32 and attempts.dtype == np.int32 and exhausted.dtype == bool
    assert not exhausted.any()
    key = uid.astype(np.int64) * f['N'] + iid
    rec_keys, pos_keys = _pairs(*f['rec'], f['N']), _pairs(*f['pos'][:2], f['N'])
    neg = y == np.float32(-0.25)                                       # (0 - 1) / 4; a positive's target is 0.5, 0.75 or 1
    assert not np.isin(key[neg], rec_keys).any()
    assert np.isin(key[~neg], pos_keys).all()
    value_of = dict(zip(pos_keys.tolist(), f['pos'][2].tolist()))
    want = np.array([(np.float32(value_of[k]) - np.float32(vmin)) / np.float32(vrange) for k in key[~neg].tolist()], np.float32)
    assert np.array_equal(y[~neg], want)
    assert abs(neg.mean() - 0.75) < 0.01
    assert (attempts[~neg] > 1).mean() >= 0.10 and (attempts[neg] > 1).mean() >= 0.10
    assert attempts.min() >= 1 and attempts.max() < 4096
    # users are drawn uniformly among the eligible: every user with a positive appears among the positives
    assert set(uid[~neg].tolist()) == set(np.flatnonzero(np.diff(f['pos'][0]) > 0).tolist())
    assert took < 1.0, took                                            # vectorised by attempt round


def test_point_sample_counter_unvalued_and_raw_targets(frame):
    f = frame
    u1, i1, y1, a1, e1 = _draw(f, 5000, 3, 9)
    assert set(y1.tolist()) == {0.0, 1.0} and not e1.any()
    u2, i2, y2, a2, e2 = _draw(f, 5000, 3, 9, values=f['pos'][2])      # vrange = 0: raw values, negatives 0
    assert np.array_equal(u1, u2) and np.array_equal(i1, i2) and np.array_equal(a1, a2)
    assert np.array_equal(y2 == 0, y1 == 0) and set(y2[y2 != 0].tolist()) == {3.0, 4.0, 5.0}
    u3, i3, y3, _, _ = _draw(f, 5000, 3, 9, values=f['pos'][2], vmin=2.0, vrange=5.0)
    assert np.array_equal(u1, u3) and np.array_equal(i1, i3)
    assert np.array_equal(y3[y1 == 0], np.full((y1 == 0).sum(), np.float32(-2.0) / np.float32(5.0), np.float32))


def test_point_sample_counter_without_a_recorded_csr_draws_negatives_against_the_positives(frame):
    f = frame
    uid, iid, y, attempts, exhausted = _draw(f, 20_000, 3, 4, recorded=False)
    key = uid.astype(np.int64) * f['N'] + iid
    pos_keys, rec_keys = _pairs(*f['pos'][:2], f['N']), _pairs(*f['rec'], f['N'])
    assert not exhausted.any() and not np.isin(key[y == 0], pos_keys).any() and np.isin(key[y == 1], pos_keys).all()
    assert np.isin(key[y == 0], rec_keys).any()                        # (recorded non-positives are negatives here)


def test_point_sample_counter_neg_ratio_zero_gives_no_negative(frame):
    uid, iid, y, attempts, exhausted = _draw(frame, 8000, 0, 77)
    assert (y == 1).all() and not exhausted.any()
    key = uid.astype(np.int64) * frame['N'] + iid
    assert np.isin(key, _pairs(*frame['pos'][:2], frame['N'])).all()


def test_point_sample_counter_takes_the_seed_modulo_two_to_the_64(frame):
    a = _draw(frame, 3000, 3, 2 ** 64 - 3)
    b = _draw(frame, 3000, 3, 2 ** 64 - 3 + 2 ** 64)
    c = _draw(frame, 3000, 3, 2 ** 64 - 2)
    assert all(np.array_equal(x, z) for x, z in zip(a, b))
    assert not np.array_equal(a[0], c[0])


def test_point_sample_counter_reports_the_draws_that_run_out():
    """What the header documents for a draw whose attempts run out, on a frame built for it (one user, who records every item and has
    no positive): a negative keeps the last rejected pair, a positive the last user, item 0 and y = 1."""
    N = 5
    pos = (np.zeros(2, np.int64), np.zeros(0, np.int32))
    rec = (np.array([0, N], np.int64), np.arange(N, dtype=np.int32))
    uid, iid, y, attempts, exhausted = do.point_sample_counter(pos[0], pos[1], rec[0], rec[1], 1, N, 64, 1, 3, max_tries=7)
    assert exhausted.all() and (attempts == 7).all() and (uid == 0).all()
    assert set(y.tolist()) == {0.0, 1.0} and (iid[y == 1] == 0).all() and len(set(iid[y == 0].tolist())) > 1
