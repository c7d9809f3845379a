"""NumPy statement of the STRUCTURE of the segmented reduction over a key-sorted touch list (csrc/drx_segreduce.hpp) — who finishes which
segment — and builders of lists whose run lengths are designed so that every branch of that structure is taken on purpose:

  the planned reduction (k_plan_spans / plan_chunk, SpanShape, k_seg_reduce_planned, k_span_planned)   span_structure, case_counts
  the unplanned one (k_seg_reduce's chunk flags, k_span_short's probe, k_span_long)                     unplanned_structure
  run-length designs                                                                                   Runs, design_planned, design_unplanned

Everything here is integer and exact; no GPU, no torch, no libdrx (tests/test_seg_oracle.py checks it on hand-written lists).  The GPU
tests (tests/test_gpu_seg_exact.py) compare span_structure with the plan a preparation left (drx_debug_span_plan) and assert through
case_counts / unplanned_structure that a designed list really contains the cases it was designed for."""
import numpy as np

NONE = 0xFFFFFFFF                  # DRX_KEY_NONE
CHUNK, CHUNK_LONG = 32, 64         # kChunk, kChunkLong
SEG_BLOCK = 128                    # kSegBlock: threads of a workgroup of the planned reduction; cpb = SEG_BLOCK / G chunks per workgroup
PLAN_SHORT = 16                    # kPlanShort: spans of up to this many partial rows are combined by one group
SHORT_SPAN = 64                    # kShortSpan (unplanned): chunk borders a segment may cross and still be combined by one group


def geom_g(ld):
    """G of pick_geom(ld) (csrc/drx_common.hpp)"""
    for top, g in ((16, 4), (32, 8), (64, 16), (128, 32)):
        if ld <= top:
            return g
    return 64


def cpb_of(ld):
    return SEG_BLOCK // geom_g(ld)


def span_shape(g0, m_in, has_end, cpb):
    """SpanShape: the partials of a span behind its first chunk — (n_lead, n_blk, n_trail): lead chunks up to the next workgroup
    boundary, whole all-inner workgroups, trailing chunks (the chunk holding the segment's end among them)."""
    first = g0 + 1
    to_boundary = (cpb - first % cpb) % cpb
    n_lead = min(m_in, to_boundary)
    n_blk = (m_in - n_lead) // cpb
    n_trail = m_in - n_lead - n_blk * cpb + has_end
    return n_lead, n_blk, n_trail


def _runs(keys):
    """(start, end, key) of every maximal run of equal keys"""
    keys = np.asarray(keys, dtype=np.uint32)
    if keys.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), keys
    cut = np.flatnonzero(keys[1:] != keys[:-1]) + 1
    start = np.concatenate([[0], cut])
    end = np.concatenate([cut, [keys.size]])
    return start, end, keys[start]


def span_structure(keys_sorted, chunk, cpb):
    """The planned reduction's structure of a sorted list (DRX_KEY_NONE behind the touches; the PRISTINE list: before any sole toucher's
    key is blanked), after plan_chunk: chunk g STARTS a crossing when the run at its end goes on behind it and did not already fill it
    from before its start.  With seg_end the first position behind that run:
      the run ends inside chunk g + 1     ext[g] = seg_end - (g + 1) chunk: chunk g's window takes those touches, no span;
      else                                 a span (g0 = g, m_in = chunks wholly inside the run behind g, has_end = a partial chunk follows
                                           them): short when SpanShape's total <= PLAN_SHORT, else long.
    inner[g]: chunk g is one whole run of a segment that began before it; all_inner[blk]: every chunk of workgroup blk is (it leaves
    ONE block partial).  Returns dict(ext, short, long, shape, inner, all_inner, n_chunks)."""
    keys = np.asarray(keys_sorted, dtype=np.uint32)
    T = int(keys.size)
    n_chunks = (T + chunk - 1) // chunk
    ext = np.zeros(n_chunks, dtype=np.uint8)
    short, long_, shape = set(), set(), {}
    start, end, key = _runs(keys)
    for s, e, k in zip(start.tolist(), end.tolist(), key.tolist()):
        if k == NONE:
            continue
        g = s // chunk                                  # the chunk the run starts in
        c_end = min(T, (g + 1) * chunk)
        if e <= c_end:
            continue                                    # inside one chunk
        m_in = e // chunk - (g + 1)
        has_end = 1 if e % chunk else 0
        if m_in == 0:
            ext[g] = e - c_end
            continue
        d = (g, m_in, has_end)
        sh = span_shape(g, m_in, has_end, cpb)
        shape[d] = sh
        (short if sum(sh) <= PLAN_SHORT else long_).add(d)
    inner = np.zeros(n_chunks, dtype=bool)
    for g in range(1, n_chunks):
        if (g + 1) * chunk <= T:
            f = keys[g * chunk]
            inner[g] = f != NONE and keys[g * chunk - 1] == f and keys[(g + 1) * chunk - 1] == f
    n_blocks = (n_chunks + cpb - 1) // cpb
    pad = np.zeros(n_blocks * cpb, dtype=bool)
    pad[:n_chunks] = inner
    return dict(ext=ext, short=short, long=long_, shape=shape, inner=inner, all_inner=pad.reshape(n_blocks, cpb).all(axis=1),
                n_chunks=n_chunks)


def plan_sets(desc, cnt, n_chunks):
    """The two descriptor sets of a device plan: desc [n_chunks, 2] words (x = g0, y = m_in | has_end << 31), short spans from the front,
    long ones from the back; cnt = (short, long)."""
    desc = np.asarray(desc, dtype=np.uint32).reshape(n_chunks, 2)
    unpack = lambda d: (int(d[0]), int(d[1] & 0x7FFFFFFF), int(d[1] >> 31))
    n_s, n_l = int(cnt[0]), int(cnt[1])
    assert n_s + n_l <= n_chunks
    return {unpack(desc[i]) for i in range(n_s)}, {unpack(desc[n_chunks - 1 - i]) for i in range(n_l)}


CASES = ('a_ends_on_border', 'a_starts_on_border', 'b_ext_1', 'b_ext_max', 'b_two_extended_in_a_row', 'b_last_slot_alone',
         'c_total_16', 'c_total_17', 'c_lead_0', 'c_lead_max', 'c_blk_0', 'c_blk_1', 'c_blk_2plus', 'c_trail_0', 'c_trail_max',
         'c_has_end_0', 'c_has_end_1', 'd_two_all_inner_in_a_row', 'd_all_inner_next_to_end', 'e_first_at_0', 'e_last_partial_chunk',
         'e_last_crosses_to_end', 'e_slack_behind', 'f_border_keys', 'f_crossing_W', 'f_crossing_W2T', 'f_crossing_V', 'f_W2T_span',
         'g_blank_first_slot', 'g_blank_last_slot', 'g_blank_in_ext_window')


def case_counts(keys_sorted, chunk, cpb, n_items=None, n_users=None, blank=None):
    """How often a list holds each case the designed lists are made for (CASES; the letters are those of the designs' description in
    tests/test_gpu_seg_exact.py).  keys_sorted: the pristine list; blank [n_valid]: which keys a preparation blanks (None: none);
    n_items / n_users: the CDAE key space (None: the f_ cases are not counted)."""
    keys = np.asarray(keys_sorted, dtype=np.uint32)
    T = int(keys.size)
    st = span_structure(keys, chunk, cpb)
    start, end, key = _runs(keys)
    live = key != NONE
    start, end, key = start[live], end[live], key[live]
    n_valid = int(end[-1]) if end.size else 0
    c = dict.fromkeys(CASES, 0)
    c['a_ends_on_border'] = int(((end % chunk == 0) & (end < n_valid)).sum())
    c['a_starts_on_border'] = int(((start % chunk == 0) & (start > 0)).sum())
    ext = st['ext'].astype(np.int64)
    c['b_ext_1'] = int((ext == 1).sum())
    c['b_ext_max'] = int((ext == chunk - 1).sum())
    c['b_two_extended_in_a_row'] = int(((ext[:-1] > 0) & (ext[1:] > 0)).sum())
    crossing_from_last = (start % chunk == chunk - 1) & (end > start + 1)
    c['b_last_slot_alone'] = int((crossing_from_last & (ext[start // chunk] > 0)).sum())
    shapes = [st['shape'][d] + (d[2],) for d in sorted(st['short'] | st['long'])]
    tot = [l + b + t for l, b, t, _ in shapes]
    c['c_total_16'], c['c_total_17'] = tot.count(PLAN_SHORT), tot.count(PLAN_SHORT + 1)
    c['c_lead_0'] = sum(1 for s in shapes if s[0] == 0)
    c['c_lead_max'] = sum(1 for s in shapes if s[0] == cpb - 1)
    c['c_blk_0'] = sum(1 for s in shapes if s[1] == 0)
    c['c_blk_1'] = sum(1 for s in shapes if s[1] == 1)
    c['c_blk_2plus'] = sum(1 for s in shapes if s[1] >= 2)
    c['c_trail_0'] = sum(1 for s in shapes if s[2] == 0)
    c['c_trail_max'] = sum(1 for s in shapes if s[2] == cpb)
    c['c_has_end_0'] = sum(1 for s in shapes if s[3] == 0)
    c['c_has_end_1'] = sum(1 for s in shapes if s[3] == 1)
    ai = st['all_inner']
    c['d_two_all_inner_in_a_row'] = int((ai[:-1] & ai[1:]).sum())
    # an all-inner workgroup whose right neighbour holds the end of the same segment
    bs = chunk * cpb
    for b in np.flatnonzero(ai).tolist():
        at = (b + 1) * bs                               # the right neighbour's first touch
        if at < n_valid and keys[at] == keys[at - 1]:
            e = int(end[np.searchsorted(start, at, side='right') - 1])
            c['d_all_inner_next_to_end'] += int(e <= at + bs)
    c['e_first_at_0'] = int(start.size > 0 and start[0] == 0)
    c['e_last_partial_chunk'] = int(n_valid % chunk != 0)
    c['e_last_crosses_to_end'] = int(end.size > 0 and start[-1] // chunk < (n_valid - 1) // chunk)
    c['e_slack_behind'] = T - n_valid
    if n_items is not None:
        N, U = n_items, n_users
        present = set(key.tolist())
        c['f_border_keys'] = sum(1 for k in (0, N - 1, N, 2 * N - 1, 2 * N, 2 * N + U - 1) if k in present)
        cross = (start // chunk) < ((end - 1) // chunk)
        c['f_crossing_W'] = int((cross & (key < N)).sum())
        c['f_crossing_W2T'] = int((cross & (key >= N) & (key < 2 * N)).sum())
        c['f_crossing_V'] = int((cross & (key >= 2 * N)).sum())
        c['f_W2T_span'] = sum(1 for d in st['short'] | st['long'] if N <= int(keys[(d[0] + 1) * chunk - 1]) < 2 * N)
    if blank is not None:
        at = np.flatnonzero(np.asarray(blank, dtype=bool))
        g = at // chunk
        c['g_blank_first_slot'] = int((at % chunk == 0).sum())
        c['g_blank_last_slot'] = int((at % chunk == chunk - 1).sum())
        left = np.where(g > 0, ext[np.maximum(g - 1, 0)], 0)
        c['g_blank_in_ext_window'] = int(((ext[g] > 0) | (left > 0)).sum())
    return c


def unplanned_structure(keys_sorted, chunk=CHUNK):
    """The unplanned reduction's structure (k_seg_reduce + k_span_short + k_span_long): per chunk the flag k_seg_reduce leaves (0: its
    first segment starts here; 2: the whole chunk is the middle of a crossing segment; 1: it starts with the end of one), and per
    crossing segment (g0, mids, end): the chunk it starts in, the middle chunks behind it, whether a chunk holding its end closes them.
    short / long: which tier finishes it — k_span_short's groups probe G flags at a time and hand a segment over as soon as they have
    counted SHORT_SPAN middle chunks (every G of pick_geom divides 64: at exactly 64 of them, whatever follows), else when mids + end
    exceeds SHORT_SPAN."""
    keys = np.asarray(keys_sorted, dtype=np.uint32)
    T = int(keys.size)
    n_chunks = (T + chunk - 1) // chunk
    flag = np.zeros(n_chunks, dtype=np.uint8)
    for g in range(n_chunks):
        s, e = g * chunk, min(T, (g + 1) * chunk)
        first, last = keys[s], keys[e - 1]
        prev = keys[s - 1] if s > 0 else NONE
        nxt = keys[e] if e < T else NONE
        cont = first != NONE and first == prev
        flag[g] = 2 if (cont and last == first and nxt == first) else (1 if cont else 0)
    short, long_ = set(), set()
    start, end, key = _runs(keys)
    for s, e, k in zip(start.tolist(), end.tolist(), key.tolist()):
        g0 = s // chunk
        if k == NONE or e <= min(T, (g0 + 1) * chunk):
            continue
        mids = 0
        while g0 + 1 + mids < n_chunks and flag[g0 + 1 + mids] == 2:
            mids += 1
        has_end = int(g0 + 1 + mids < n_chunks and flag[g0 + 1 + mids] == 1)
        assert (g0 + mids + has_end) * chunk < e <= (g0 + 1 + mids + has_end) * chunk
        (long_ if (mids >= SHORT_SPAN or mids + has_end > SHORT_SPAN) else short).add((g0, mids, has_end))
    return dict(flag=flag, short=short, long=long_, n_chunks=n_chunks)


# ---- run-length designs -----------------------------------------------------------------------------------------------------------------
class Runs:
    """Run lengths laid down from list position pos0 on: run(n) appends a run; to(p) fills up to list position p with runs that cross no
    chunk border (filler: `small` — singles and pairs — or as long as the chunk allows)."""

    def __init__(self, pos0, chunk, small=True):
        self.pos, self.chunk, self.small, self.runs = int(pos0), chunk, small, []

    def run(self, n):
        assert n >= 1
        self.runs.append(int(n))
        self.pos += int(n)

    def to(self, target):
        assert target >= self.pos, (target, self.pos)
        i = 0
        while self.pos < target:
            room = min(target - self.pos, self.chunk - self.pos % self.chunk)
            self.run(min(room, (1, 2, 1, 3)[i % 4]) if self.small else room)
            i += 1

    def to_slot(self, slot):
        """fill up to the next position whose slot in its chunk is `slot`"""
        self.to(self.pos + (slot - self.pos) % self.chunk)

    def span(self, cpb, n_lead, n_blk, trail_chunks, has_end, tail=5, end_touches=7):
        """a run that starts `tail` touches before the end of a chunk g0 with (g0 + 1) % cpb == (cpb - n_lead) % cpb, fills n_lead +
        n_blk cpb + trail_chunks whole chunks and (has_end) end_touches of the next: SpanShape (n_lead, n_blk, trail_chunks + has_end)"""
        assert 0 <= n_lead < cpb and 0 <= trail_chunks < cpb and 1 <= tail <= self.chunk and 1 <= end_touches < self.chunk
        assert n_lead + n_blk * cpb + trail_chunks >= 1
        g0 = self.pos // self.chunk                               # the first chunk whose last `tail` slots are still free
        if (g0 + 1) * self.chunk - tail < self.pos:
            g0 += 1
        while (g0 + 1) % cpb != (cpb - n_lead) % cpb:
            g0 += 1
        self.to((g0 + 1) * self.chunk - tail)
        m_in = n_lead + n_blk * cpb + trail_chunks
        self.run(tail + m_in * self.chunk + (end_touches if has_end else 0))
        return g0, m_in, int(bool(has_end))


def total_16(cpb):
    """(n_lead, n_blk, trail_chunks) of a span of PLAN_SHORT partials over as few chunks as the workgroup size allows"""
    n_lead = min(cpb - 1, PLAN_SHORT // 2)
    trail = min(cpb - 1, PLAN_SHORT - n_lead)
    return n_lead, PLAN_SHORT - n_lead - trail, trail


def design_planned(pos0, chunk, cpb, spans, small=True, total=None, closing=0):
    """Run lengths from list position pos0 on that hold, whatever pos0 is: a whole-chunk run between two others (a segment ending on a
    chunk border, the next starting there); three chunks extended in a row (ext = 1, chunk - 1, 1: the second starts behind the first's
    extension and reaches into the third, whose crossing segment is its last slot alone) with filler runs inside their windows; single
    runs at a chunk's first and last slot; the spans of `spans` — (n_lead, n_blk, trail_chunks, has_end) each — and, total given, filler
    up to that many touches closed by a run of `closing` touches (0: none)."""
    r = Runs(pos0, chunk, small)
    r.to_slot(0)
    r.run(1)                                            # a single at a chunk's first slot
    r.to_slot(chunk - 1)
    r.run(1)                                            # ... and at its last
    r.run(chunk)                                        # a whole chunk
    r.to_slot(chunk - 3)
    r.run(4)                                            # ext = 1
    r.run(1)                                            # a single inside the next window, which starts behind that extension
    r.to_slot(chunk - 2)
    r.run(2 + chunk - 1)                                # ext = chunk - 1, from behind the left neighbour's extension
    r.run(2)                                            # the last slot alone, ext = 1
    for s in spans:
        r.span(cpb, *s)
    if total is not None:
        used = r.pos - pos0
        assert used + closing <= total, f'the design takes {used} + {closing} touches, {total} are there'
        r.to(pos0 + total - closing)
        if closing:
            r.run(closing)
    return r.runs


def design_unplanned(tail_pad=11):
    """Run lengths for the unplanned kernels (chunks of 32, from position 0): runs of 31, 32, 33, 1, 63, 64, 65 placed so that runs end on
    a chunk border, start on one and start at a chunk's last slot; a whole-chunk run between two others; crossing runs of a first-chunk
    tail + 62 .. 65 following chunks, the last of them whole or partial (both sides of k_span_short's limit and of its early
    exit); one run over 200 middle chunks (k_span_long's strided groups)."""
    r = Runs(0, CHUNK, True)
    r.run(31); r.run(1)                                 # ends on a border; a single at a chunk's last slot
    r.run(32)                                           # a whole chunk between two others
    r.run(33)                                           # starts on a border, one touch into the next chunk
    r.run(31)                                           # ... ends on a border
    r.run(63); r.run(1)
    r.run(64)                                           # two whole chunks: a tail partial and an end chunk, no middle
    r.run(65)
    r.to_slot(CHUNK - 1)
    r.run(33)                                           # starts at a chunk's last slot, ends on the next border
    r.to_slot(CHUNK - 1)
    r.run(2)                                            # starts at a chunk's last slot, ends at the next chunk's first
    for m in (62, 63, 64, 65):                          # m following chunks: all of them whole, or the last one partial
        r.span(1, 0, m, 0, 0)
        r.span(1, 0, m - 1, 0, 1)
    r.span(1, 0, 203, 0, 1, tail=3, end_touches=9)
    r.to(r.pos + tail_pad)
    return r.runs


def keys_of_runs(runs, ids):
    """the sorted key list of runs with ascending ids"""
    ids = np.asarray(ids, dtype=np.int64)
    assert ids.size == len(runs) and (np.diff(ids) > 0).all()
    return np.repeat(ids, runs).astype(np.uint32)


def spread_ids(n, n_rows):
    """n distinct ascending ids over [0, n_rows), 0 and n_rows - 1 among them"""
    assert 2 <= n <= n_rows
    ids = np.unique(np.round(np.linspace(0, n_rows - 1, n)).astype(np.int64))
    assert ids.size == n and ids[0] == 0 and ids[-1] == n_rows - 1
    return ids


# ---- a CDAE batch whose sorted touch list has designed run lengths ---------------------------------------------------------------------
def cdae_design(ld, long_list, B=8192, hot=0, seed=5):
    """A history and a batch of B samples whose sorted touch list is three designed arrays.  Every user holds at most one item, so a
    sample gives one W touch (its user's item, if the user holds one), one W2T touch (N + iid) and one V touch (2N + uid), and the run
    lengths of the three arrays are the multiplicities of held item, iid and uid in the batch; a run's position is the sum of the runs
    before it.  Users 0 .. : one HOLDER per W run (the samples of W run j are that user's: the V array begins with a copy of the W
    array's runs, at another position), then users without history whose multiplicities are the V array's own design.
    hot: the first `hot` items get TWO holders each (the highest degrees of the history: engine.hot_set makes them the hot head) and runs
    of their own, one in four of them no sample at all; their W touches are absent from the list, the W design starts at item `hot`.
    long_list: chunks of 64 and filler runs as long as a chunk allows (few distinct keys: T > 8 (2N + U)); else chunks of 32 and small
    filler runs.  Returns dict(indptr, indices, uid, iid, N, U, chunk, cpb, runs=(W, W2T, V run lengths in list order), hot_runs)."""
    chunk = CHUNK_LONG if long_list else CHUNK
    cpb = cpb_of(ld)
    small = not long_list
    t16 = total_16(cpb)
    rng = np.random.default_rng(seed + ld)
    w_runs = design_planned(0, chunk, cpb, [(0, 0, 1, 0), (cpb - 1, 0, 0, 0), t16 + (0,)], small)
    w_runs.append(chunk + 7 - (sum(w_runs) % chunk) if sum(w_runs) % chunk != 7 else chunk)       # the W array ends 7 touches into a chunk
    n_w = sum(w_runs)
    hot_runs = [0 if h % 4 == 3 else int(rng.integers(1, 40)) + (300 if h == 1 else 0) for h in range(hot)]
    n_hot = sum(hot_runs)
    assert n_w + n_hot < B
    o_runs = design_planned(n_w, chunk, cpb, [(0, 1, cpb - 1, 1), t16 + (1,)], small, total=B, closing=chunk + 3)
    # holders: two per hot item (its run split between them), one per W run
    holder_item, holder_runs = [], []
    for h, n in enumerate(hot_runs):
        holder_item += [h, h]
        holder_runs += [n - n // 2, n // 2]
    w_items = hot + spread_ids(len(w_runs), max(len(w_runs), len(o_runs)) + 3)
    N = int(w_items[-1]) + 1
    holder_item += w_items.tolist()
    holder_runs += w_runs
    n_held = n_w + n_hot
    v_own = design_planned(n_w + B + n_held, chunk, cpb, [(min(1, cpb - 1), 2, 0, 1)], small, total=B - n_held, closing=chunk + 5)
    U = len(holder_runs) + len(v_own)
    deg = np.zeros(U, dtype=np.int64)
    deg[:len(holder_item)] = 1
    indptr = np.concatenate([[0], np.cumsum(deg)])
    indices = np.asarray(holder_item, dtype=np.int32)
    per_user = np.asarray(holder_runs + v_own, dtype=np.int64)
    assert per_user.sum() == B and sum(o_runs) == B
    uid = np.repeat(np.arange(U), per_user)[rng.permutation(B)]
    o_items = spread_ids(len(o_runs), N)
    iid = np.repeat(o_items, o_runs)[rng.permutation(B)]
    v_runs = [n for n in holder_runs + v_own if n > 0]
    return dict(indptr=indptr, indices=indices, uid=uid.astype(np.int64), iid=iid.astype(np.int64), N=N, U=U, chunk=chunk, cpb=cpb,
                runs=(w_runs, o_runs, v_runs), hot_runs=hot_runs, B=B)
