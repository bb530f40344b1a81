"""The pump's burst ticks (vad_pump_set_burst + vad_pump_submit_burst, csrc/pump.hip + kernel_present.hip assemble_burst): a stream may
have several rows in one tick and a row may be longer than a chunk (a 60 ms Opus frame, what a jitter buffer releases after a stall), so
a stream may complete up to max_burst chunks in a tick and is stepped that many times inside it.  The reference's VADIterator is simply
called once per chunk, as fast as the chunks are there (src/silero_vad/utils_vad.py:507-549), so the route is defined by reduction:
every result here is compared, bit for bit, with a second pump WITHOUT bursts that is fed the same concatenated audio, cut into chunks,
through vad_pump_submit_rows -- one chunk per stream and tick, a burst tick's sub-steps spread over as many ticks there.
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import SRS

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
CHUNK_ROUTES = ("rows", "compact", "masked", "full")


@pytest.fixture(scope="module")
def model(built):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback to silently pass on)")
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    assert m.engine._h, "native engine not created"
    return m


def chunk_of(sr):
    return 512 if sr == 16000 else 256


def encode(pcm, law):
    """int16 -> G.711 codes: the code whose expansion is nearest (ties to the lower value); "s16" is the identity."""
    from silero_vad_amd import g711_expand
    if law == "s16":
        return pcm
    codes = np.arange(256, dtype=np.uint8)
    lin = g711_expand(codes, law).astype(np.int32)
    order = np.argsort(lin, kind="stable")
    v = lin[order]
    x = pcm.astype(np.int32)
    j = np.clip(np.searchsorted(v, x), 1, len(v) - 1)
    j -= (x - v[j - 1]) <= (v[j] - x)
    return codes[order[j]]


def through_codecs(pcm_of_stream, ops):
    """What each stream's audio is after its rows went through their codecs (G.711 is lossy): row (s, a, ln, codec) carries
    encode(audio[s][a:a + ln], codec), and encode is the identity on what it produced."""
    from silero_vad_amd import g711_expand
    out = [x.copy() for x in pcm_of_stream]
    for op in ops:
        if op[0] in ("open", "close"):
            continue
        for s, a, ln, codec in op[1]:
            if codec != "s16":
                out[s][a:a + ln] = g711_expand(encode(pcm_of_stream[s][a:a + ln], codec), codec)
    return out


# ---- a run is a list of operations -----------------------------------------------------------------------------------------------------
#   (route, rows)   one tick: rows = [(stream, first sample, length, codec), ...] in arrival order.  route "burst" / "coded" / "packets":
#                   as the entry point takes them; a chunk route ("rows", "compact", "masked", "full"): one whole chunk per listed stream
#   ("open", s) / ("close", s)
# plan() works out, from the lengths alone, which chunks every tick completes: per tick a list of sub-steps, each [(stream, first sample
# of the chunk), ...] in stream order -- what the reference pump steps, one submit_rows tick per sub-step.

def plan(ops, cap, n):
    base = np.zeros(cap, np.int64)               # where the stream's chunking (re)started: open / close drop what is pending
    have = np.zeros(cap, np.int64)               # samples submitted since
    out = []
    for op in ops:
        if op[0] in ("open", "close"):
            s = op[1]
            base[s] += have[s]
            have[s] = 0
            out.append(None)
            continue
        before = have // n
        for s, a, ln, _ in op[1]:
            assert a == base[s] + have[s], "a stream's rows continue its audio"
            have[s] += ln
        k = have // n - before
        out.append([[(int(s), int(base[s] + (before[s] + j) * n)) for s in np.flatnonzero(k > j)] for j in range(max(1, int(k.max())))])
    return out, (have % n).astype(int)


class Record:
    def __init__(self, cap):
        self.probs = {s: [] for s in range(cap)}     # per stream, in the order its chunks were stepped
        self.events = {s: [] for s in range(cap)}
        self.polls = []                              # per tick: the events as polled


def submit(pump, r, op, audio, n):
    route, rows = op
    if route == "burst":
        pump.write_burst(r, [(s, encode(audio[s][a:a + ln], c), c) for s, a, ln, c in rows])
    elif route == "coded":
        pump.write_coded_packets(r, [(s, encode(audio[s][a:a + ln], c), c) for s, a, ln, c in rows])
    elif route == "packets":
        pump.write_packets(r, [(s, audio[s][a:a + ln]) for s, a, ln, _ in rows])
    else:
        assert route in CHUNK_ROUTES and all(ln == n for _, _, ln, _ in rows)
        order = sorted(rows) if route == "compact" else rows
        slot = pump.slot(r)
        fl = np.zeros(pump.streams, np.uint8)
        for i, (s, a, ln, _) in enumerate(order):
            slot[s if route in ("masked", "full") else i] = audio[s][a:a + n]
            fl[s] = 1
        if route == "full":
            assert fl.all()
            pump.submit(r)
        elif route == "rows":
            pump.submit_rows(r, [s for s, _, _, _ in rows])
        else:
            pump.submit(r, present=fl, compact=route == "compact")


def run_pump(pump, ops, subs, audio, n, depth=1, hooks=None):
    """The pump under test: every tick by its own route, `depth` ticks in flight.  hooks[i](pump, r) runs before operation i is
    submitted, on the ring slot it will use (refusals: they must leave the slot free)."""
    rec = Record(pump.streams)
    flying = []
    R = pump.ring_slots
    t = 0

    def retire():
        sub = flying.pop(0)
        ev, r = pump.poll()
        assert pump.burst_steps(r) == len(sub)
        bp = pump.burst_probs(r)
        assert bp.shape == (len(sub), pump.streams) and np.array_equal(bp[0], pump.probs(r))
        for j, step in enumerate(sub):
            on = np.zeros(pump.streams, bool)
            for s, _ in step:
                rec.probs[s].append(bp[j][s])
                on[s] = True
            assert (bp[j][on] >= 0).all() and (bp[j][~on] == -1.0).all()        # VAD_PROB_ABSENT wherever k <= j
        for s, e in ev:
            rec.events[s].append(e)
        rec.polls.append(ev)

    for i, op in enumerate(ops):
        if hooks and i in hooks:
            while flying:
                retire()
            hooks[i](pump, t % R)
        if op[0] == "open":
            pump.open_stream(op[1])
        elif op[0] == "close":
            pump.close_stream(op[1])
        else:
            while len(flying) >= depth:
                retire()
            submit(pump, t % R, op, audio, n)
            flying.append(subs[i])
            t += 1
    while flying:
        retire()
    assert pump.poll() == (None, None)
    return rec


def run_reference(pump, ops, subs, audio, n):
    """The pump without bursts: one submit_rows tick per sub-step, one chunk per stream and tick."""
    rec = Record(pump.streams)
    for op, sub in zip(ops, subs):
        if op[0] == "open":
            pump.open_stream(op[1])
        elif op[0] == "close":
            pump.close_stream(op[1])
        else:
            polled = []
            for step in sub:
                slot = pump.slot(0)
                for i, (s, a) in enumerate(step):
                    slot[i] = audio[s][a:a + n]
                pump.submit_rows(0, [s for s, _ in step])
                ev, r = pump.poll()
                p = pump.probs(r)
                for s, _ in step:
                    rec.probs[s].append(p[s])
                for s, e in ev:
                    rec.events[s].append(e)
                polled += ev
            rec.polls.append(polled)
    return rec


def assert_same(got, want, a, b, residue):
    for s in got.probs:
        assert np.array_equal(np.array(got.probs[s], np.float32), np.array(want.probs[s], np.float32)), s
    assert got.events == want.events
    assert got.polls == want.polls               # sub-step 0's events in stream order, then sub-step 1's, ...
    for s in got.probs:
        for x, y in zip(a.state(s), b.state(s)):
            assert np.array_equal(x, y), s
        assert a.pending(s) == residue[s], s


def check(model, sr, ops, audio, cap, max_burst, depth=1, hooks=None, **kw):
    from silero_vad_amd import StreamPump
    n = chunk_of(sr)
    subs, residue = plan(ops, cap, n)
    pump = StreamPump(model.engine, sr, streams=cap, max_burst=max_burst, **kw)
    got = run_pump(pump, ops, subs, audio, n, depth=depth, hooks=hooks)
    ref = StreamPump(model.engine, sr, streams=cap, **kw)
    want = run_reference(ref, ops, subs, audio, n)
    assert_same(got, want, pump, ref, residue)
    pump.close()
    ref.close()
    return got, subs


def burst_schedule(totals, n, sr, rng, max_burst=8, rate=0.6, empty_every=41, codecs=("s16",)):
    """Burst ticks that play totals[s] samples of every stream.  A packet of stream s arrives at a tick with probability `rate` (stream
    0: always) -- 10 / 20 / 30 / 60 ms, or uniform in [1, 3N]; a stream goes silent for 1 ... 6 ticks now and then and delivers what it
    withheld as several rows of one tick.  A tick holds no more than `cap` rows and no more than the slot's bytes, and no stream more than
    max_burst chunks: what does not fit waits.  Rows are shuffled across streams (a stream's own rows keep their order); every
    `empty_every`-th tick is empty."""
    cap, ms10 = len(totals), sr // 100
    sent, due, quiet = [0] * cap, [[] for _ in range(cap)], [0] * cap
    made = [0] * cap                             # samples cut into packets so far
    ops = []
    while any(sent[s] < totals[s] for s in range(cap)):
        for s in range(cap):                     # arrivals
            if made[s] < totals[s] and (s == 0 or rng.random() < rate):
                ln = int(rng.choice([ms10, 2 * ms10, 3 * ms10, 6 * ms10])) if rng.random() < 0.7 else int(rng.integers(1, 3 * n + 1))
                ln = min(ln, totals[s] - made[s])
                due[s].append(ln)
                made[s] += ln
        per = []
        if len(ops) % empty_every != empty_every - 1:
            n_rows, n_bytes = 0, 0
            for s in [0] + [int(x) for x in 1 + rng.permutation(cap - 1)]:
                if quiet[s] > 0:
                    quiet[s] -= 1
                    continue
                mine, room = [], (max_burst + 1) * n - 1 - sent[s] % n
                while due[s] and due[s][0] <= room and n_rows < cap:
                    codec = codecs[int(rng.integers(len(codecs)))]
                    size = (due[s][0] * 2 + 15) // 16 * 16          # (as int16, whatever the codec: the same rows must fit expanded)
                    if n_bytes + size > cap * n * 2:
                        break
                    ln = due[s].pop(0)
                    mine.append((s, sent[s], ln, codec))
                    sent[s] += ln
                    room -= ln
                    n_rows += 1
                    n_bytes += size
                if mine:
                    per.append(mine)
                if rng.random() < 0.08:
                    quiet[s] = int(rng.integers(1, 7))
        who = rng.permutation([i for i, mine in enumerate(per) for _ in mine])
        at = [0] * len(per)
        rows = []
        for i in who:
            rows.append(per[i][at[i]])
            at[i] += 1
        ops.append(("burst", rows))
    return ops


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_bursts_equal_the_rechunked_stream(model, golden, tag):
    """100 streams (not a multiple of 16), parts=3, ring_slots=3, max_burst=8: packets of 10 / 20 / 30 / 60 ms and uniform lengths in
    [1, 3N], streams that go silent for 1 ... 6 ticks and then deliver everything withheld as several rows of one tick, rows shuffled
    across streams, some ticks empty.  Probability of every (stream, chunk), each stream's events and their order in every poll, final
    (h, c, context), pending residue, burst_steps and VAD_PROB_ABSENT wherever k <= j equal the submit_rows pump; stream 0 plays the
    whole fixture and gives the reference VADIterator's own events."""
    sr, g = SRS[tag], golden[tag]
    n = chunk_of(sr)
    pcm = g["pcm_i16"]
    T = len(pcm) // n
    cap = 100
    rng = np.random.default_rng(17)
    totals = [T * n] + [int(rng.integers(150, 250)) * n - int(rng.integers(0, n)) for _ in range(cap - 1)]
    audio = [np.roll(pcm, -s * 7919)[:totals[s]].copy() for s in range(cap)]
    ops = burst_schedule(totals, n, sr, rng)
    rec = golden["segments"][tag]["iterator"]["default"]
    got, subs = check(model, sr, ops, audio, cap, 8, depth=2, parts=3, ring_slots=3, **rec["init"])
    rows_of = [np.bincount([s for s, _, _, _ in op[1]], minlength=cap) for op in ops]
    assert sum(1 for op in ops if not op[1]) >= 2                   # ticks in which nobody delivers
    assert max(int(c.max()) for c in rows_of) >= 3                  # several rows of one stream in one tick
    assert any(ln > n for op in ops for _, _, ln, _ in op[1])       # rows longer than a chunk
    assert max(len(sub) for sub in subs) >= 4                       # deep bursts
    for s in range(cap):                                            # every whole chunk of every stream was stepped, once
        assert len(got.probs[s]) == totals[s] // n, s
    assert got.events[0] == rec["events"], tag                      # the reference's own iterator events (39 / 92)
    assert np.abs(np.array(got.probs[0]) - np.asarray(g["probs_wav"]).reshape(-1)[:T]).max() < TIGHT


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_burst_boundaries(model, golden, tag):
    """c = 0, L = 8N; c = N - 1, L = 7N + 1 (eight chunks, residue 0); L = 8N + N - 1 - c (eight chunks, residue N - 1), where one more
    sample is refused; a row of length 1 between two long rows."""
    from silero_vad_amd import _lib
    sr, n = SRS[tag], chunk_of(SRS[tag])
    pcm = golden[tag]["pcm_i16"]
    cap = 32                                                         # (the slot holds `cap` chunks of int16: the second tick needs 23)
    audio = [np.roll(pcm, -(40 * n + s * 7919))[:40 * n].copy() for s in range(cap)]
    c = 37
    ops = [("burst", [(1, 0, 8 * n, "s16"), (2, 0, n - 1, "s16"), (3, 0, c, "s16"), (4, 0, 5, "s16")]),
           ("burst", [(2, n - 1, 7 * n + 1, "s16"), (3, c, 8 * n + n - 1 - c, "s16"),
                      (4, 5, 2 * n + 3, "s16"), (5, 0, 3 * n, "s16"), (4, 2 * n + 8, 1, "s16"), (4, 2 * n + 9, n + 5, "s16")]),
           ("burst", [(3, 9 * n - 1, 1, "s16"), (1, 8 * n, n, "s16")]),
           ("burst", [])]

    def one_too_many(pump, r):                                      # stream 3 has c pending: 8N + N - c samples would be a ninth chunk
        assert pump.pending(3) == c and pump.pending(2) == n - 1
        with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
            pump.write_burst(r, [(3, np.zeros(9 * n - c, np.int16))])
        with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):     # ... and so would the same over two rows
            pump.write_burst(r, [(3, np.zeros(8 * n, np.int16)), (0, np.zeros(8, np.int16)), (3, np.zeros(n - c, np.int16))])
        assert pump.pending(3) == c and pump.pending(0) == 0 and pump.poll() == (None, None)

    got, subs = check(model, sr, ops, audio, cap, 8, hooks={1: one_too_many}, parts=2, ring_slots=2)
    assert [len(sub) for sub in subs] == [8, 8, 1, 1]
    assert [len(got.probs[s]) for s in range(1, 6)] == [9, 8, 9, 3, 3]


def test_g711_bursts(model, golden):
    """mu-law and A-law rows in bursts at 8 kHz, and two rows of one stream in one tick with different codecs: the coded burst equals
    the int16 burst of the expanded samples, and both equal the submit_rows pump on that audio."""
    from silero_vad_amd import StreamPump
    sr, n, cap = 8000, 256, 40
    pcm = golden["8k"]["pcm_i16"]
    rng = np.random.default_rng(23)
    totals = [int(rng.integers(60, 90)) * n - int(rng.integers(0, n)) for _ in range(cap)]
    raw = [np.roll(pcm, -(40 * n + s * 7919))[:totals[s]].copy() for s in range(cap)]
    ops = burst_schedule(totals, n, sr, rng, codecs=("s16", "ulaw", "alaw"), empty_every=19)
    # two rows of one stream in one tick with different codecs, whatever the schedule drew
    ops.append(("burst", []))
    raw[7] = np.concatenate([raw[7], np.roll(pcm, -99991)[:3 * n]])
    ops.append(("burst", [(7, totals[7], n + 40, "ulaw"), (7, totals[7] + n + 40, n + 9, "alaw"), (7, totals[7] + 2 * n + 49, 100, "s16")]))
    mixed = [len({c for s, _, _, c in op[1] if s == b}) for op in ops for b in {s for s, _, _, _ in op[1]}]
    assert max(mixed) >= 2
    audio = through_codecs(raw, ops)
    assert any(not np.array_equal(a, b) for a, b in zip(audio, raw))
    got, subs = check(model, sr, ops, audio, cap, 8, depth=2, parts=2, ring_slots=3)
    # the same bursts as int16 rows of the expanded samples
    plain = [(route, [(s, a, ln, "s16") for s, a, ln, _ in rows]) for route, rows in ops]
    pump = StreamPump(model.engine, sr, streams=cap, max_burst=8, parts=2, ring_slots=3)
    also = run_pump(pump, plain, subs, audio, n, depth=2)
    assert also.polls == got.polls
    for s in range(cap):
        assert np.array_equal(np.array(also.probs[s]), np.array(got.probs[s])), s
    pump.close()
    assert max(len(sub) for sub in subs) >= 3


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_burst_without_repeats_is_a_coded_packet_tick(model, golden, tag):
    """A burst tick in which no stream is listed twice and no row is longer than N gives exactly what vad_pump_submit_coded_packets gives
    for the same rows: probabilities of every tick, state, pending, and burst_steps == 1."""
    from silero_vad_amd import StreamPump
    sr, n, cap, K = SRS[tag], chunk_of(SRS[tag]), 40, 70
    pcm = golden[tag]["pcm_i16"]
    rng = np.random.default_rng(5)
    ms10 = sr // 100
    raw = [np.roll(pcm, -(40 * n + s * 7919))[:K * n].copy() for s in range(cap)]
    codecs = ("s16", "ulaw", "alaw") if sr == 8000 else ("s16",)
    sent = [0] * cap
    ops = []
    for t in range(K):
        rows = []
        for s in rng.permutation(cap):
            if t % 13 != 12 and rng.random() < 0.85:
                ln = int(rng.choice([ms10, 2 * ms10, 3 * ms10])) if rng.random() < 0.7 else int(rng.integers(1, n + 1))
                rows.append((int(s), sent[s], ln, codecs[int(rng.integers(len(codecs)))]))
                sent[s] += ln
        ops.append(("burst", rows))
    audio = through_codecs(raw, ops)
    a = StreamPump(model.engine, sr, streams=cap, max_burst=8, parts=2, ring_slots=2)
    b = StreamPump(model.engine, sr, streams=cap, parts=2, ring_slots=2)
    stepped = 0
    for route, rows in ops:
        submit(a, 0, ("burst", rows), audio, n)
        submit(b, 0, ("coded", rows), audio, n)
        ev_a, ev_b = a.poll()[0], b.poll()[0]
        assert ev_a == ev_b and np.array_equal(a.probs(0), b.probs(0))
        assert a.burst_steps(0) == 1 and b.burst_steps(0) == 1 and a.burst_probs(0).shape == (1, cap)
        stepped += int((a.probs(0) >= 0).sum())
    assert stepped > cap * K // 3
    for s in range(cap):
        assert a.pending(s) == b.pending(s) == sent[s] % n
        for x, y in zip(a.state(s), b.state(s)):
            assert np.array_equal(x, y), s
    a.close()
    b.close()


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_burst_ticks_mix_with_every_other_route(model, golden, tag):
    """Burst, packet, coded, rows, compact, masked and full ticks interleaved on one pump with two ticks in flight; streams reopened and
    closed with samples pending and with ticks in flight; a chunk route is refused for a stream a burst left pending."""
    from silero_vad_amd import _lib
    sr, n = SRS[tag], chunk_of(SRS[tag])
    pcm = golden[tag]["pcm_i16"]
    cap = 24
    rng = np.random.default_rng(29)
    audio = [np.roll(pcm, -(30 * n + s * 7919))[:600 * n].copy() for s in range(cap)]
    sent, pend = [0] * cap, [0] * cap
    ops, hooks = [], {}

    def row(s, ln):
        r = (s, sent[s], ln, "s16")
        sent[s] += ln
        pend[s] = (pend[s] + ln) % n
        return r

    def drop(s):
        pend[s] = 0

    def refused_for(s0):
        def hook(pump, r):
            assert pump.pending(s0) > 0
            fl = np.zeros(cap, np.uint8)
            fl[s0] = 1
            for bad in (lambda: pump.submit(r), lambda: pump.submit(r, present=fl), lambda: pump.submit(r, present=fl, compact=True),
                        lambda: pump.submit_rows(r, [s0])):
                with pytest.raises(_lib.VadError, match="pending"):
                    bad()
                assert pump.poll() == (None, None)
        return hook

    for cycle in range(14):
        # a burst that leaves most streams with samples pending: several rows, long rows, up to four chunks
        rows, used = [], 0                                           # (the slot holds `cap` rows and `cap` chunks of int16)
        room = {s: 5 * n - 1 - pend[s] for s in range(cap)}
        for s in [int(x) for x in rng.choice(cap, 3 * cap, replace=True)]:
            ln = int(min(rng.integers(1, 3 * n), room[s], cap * n - used - 8))
            if ln >= 1 and len(rows) < cap:
                rows.append(row(s, ln))
                room[s] -= ln
                used += (ln + 7) // 8 * 8
        ops.append(("burst", rows))
        busy = [s for s in range(cap) if pend[s]]
        if busy and cycle % 3 == 0:
            hooks[len(ops)] = refused_for(busy[0])
        # packets / coded packets for some (rows up to N)
        route = "packets" if cycle % 2 else "coded"
        ops.append((route, [row(int(s), int(rng.integers(1, n + 1))) for s in rng.permutation(cap) if rng.random() < 0.6]))
        # open / close with samples pending, behind ticks that are still in flight
        if cycle % 4 == 1:
            s = next(s for s in range(cap) if pend[s])
            ops.append(("open", s))
            drop(s)
        if cycle == 6:
            closed = next(s for s in range(cap) if pend[s] and s != 0)
            ops.append(("close", closed))
            drop(closed)
        if cycle == 9:
            ops.append(("open", closed))
            drop(closed)
        # a burst that brings every stream to a chunk boundary, then the chunk routes
        ops.append(("burst", [row(s, n - pend[s]) for s in rng.permutation(cap) if pend[s]]))
        assert not any(pend)
        for route in CHUNK_ROUTES:
            on = range(cap) if route == "full" else [int(s) for s in rng.permutation(cap) if rng.random() < 0.7]
            ops.append((route, [row(s, n) for s in on]))
    assert hooks
    got, subs = check(model, sr, ops, audio, cap, 4, depth=2, hooks=hooks, parts=2, ring_slots=3)
    assert max(len(sub) for sub in subs if sub) == 4 and sum(len(v) for v in got.events.values()) > 20


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_start_and_end_in_one_poll(model, golden, tag):
    """With min_silence_duration_ms=0 the fixture has an end and the next start a few chunks apart: a burst of eight chunks over them
    returns both events of that stream in ONE poll, in sub-step order; a `cap` smaller than the number of events writes `cap` of them
    and still returns the full count."""
    from silero_vad_amd import StreamPump, _lib
    sr, n, cap, K = SRS[tag], chunk_of(SRS[tag]), 20, 400
    pcm = golden[tag]["pcm_i16"]
    live = 2                                                         # (the slot holds `cap` chunks: two streams can burst eight at once)
    audio = [pcm[:(K + 8) * n].copy() for s in range(cap)]           # every stream plays the start of the fixture
    kw = dict(parts=1, ring_slots=2, min_silence_duration_ms=0)
    ref = StreamPump(model.engine, sr, streams=cap, **kw)
    at = {}                                                          # chunk index -> kind, stream 0
    for t in range(K + 8):
        ref.slot(0)[:] = np.stack([a[t * n:(t + 1) * n] for a in audio])
        ref.submit(0)
        for s, e in ref.poll()[0]:
            if s == 0:
                at[t] = e
    ticks = sorted(at)
    first = next(i for i, j in zip(ticks, ticks[1:]) if j - i <= 6 and i >= 1)
    want = [at[t] for t in range(first, first + 8) if t in at]
    assert len(want) >= 2 and {"start", "end"} <= {k for e in want for k in e}
    pump = StreamPump(model.engine, sr, streams=cap, max_burst=8, **kw)
    done = 0
    while done < first:                                              # up to the chunk in front of the pair, in bursts of up to 8 chunks
        k = min(8, first - done)
        pump.write_burst(0, [(s, audio[s][done * n:(done + k) * n]) for s in range(live)])
        pump.poll()
        done += k
    pump.write_burst(1, [(s, audio[s][first * n:(first + 8) * n]) for s in range(live)])
    buf = (_lib.IterEvent * 1)()
    r = ctypes.c_int(-1)
    m = pump._L.vad_pump_poll(pump._h, 1, buf, 1, ctypes.byref(r))   # cap = 1: the full count comes back, one event is written
    assert r.value == 1 and pump.burst_steps(1) == 8
    assert m == live * len(want) and m > 1
    assert (buf[0].slot, {"end" if buf[0].kind else "start": buf[0].sample}) == (0, want[0])
    # the same tick on a second pump, polled whole: per sub-step, stream order
    again = StreamPump(model.engine, sr, streams=cap, max_burst=8, **kw)
    for lo in list(range(0, first, 8)):
        again.write_burst(0, [(s, audio[s][lo * n:min(lo + 8, first) * n]) for s in range(live)])
        again.poll()
    again.write_burst(1, [(s, audio[s][first * n:(first + 8) * n]) for s in range(live)])
    ev, _ = again.poll()
    assert ev == [(s, e) for e in want for s in range(live)]
    assert np.array_equal(again.burst_probs(1), pump.burst_probs(1))
    for p in (ref, pump, again):
        p.close()


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_burst_refusals_queue_nothing(model, golden, tag):
    """Bursts not enabled, a stream that would complete more than max_chunks chunks, more rows than streams, a bad codec, a stream out of
    range, a length below 1, a misaligned or negative offset, a row past the slot: VAD_ERR_ARG, the pending counts unchanged, the slot
    still free, and the next valid tick gives the reference's bits."""
    from silero_vad_amd import StreamPump, _lib
    sr, n, cap = SRS[tag], chunk_of(SRS[tag]), 20
    pcm = golden[tag]["pcm_i16"][40 * n:]
    area = cap * n * 2
    off = StreamPump(model.engine, sr, streams=cap, parts=1, ring_slots=2)
    with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
        off.submit_burst(0, [0], [n])
    with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
        off.write_burst(0, [(0, pcm[:n])])
    assert off.poll() == (None, None) and off.pending(0) == 0 and off.burst_steps(0) == 1
    assert off._L.vad_pump_burst_probs(off._h, 0, 1) is None and off._L.vad_pump_burst_probs(off._h, 0, 0) is not None
    pump = StreamPump(model.engine, sr, streams=cap, parts=1, ring_slots=2, max_burst=3)
    pump.write_burst(0, [(2, pcm[:100])])
    assert pump.poll()[0] == [] and (pump.probs(0) == -1.0).all() and pump.burst_steps(0) == 1
    held = [pump.pending(s) for s in range(cap)]
    assert held[2] == 100 and sum(held) == 100
    L, h = pump._L, pump._h
    assert L.vad_pump_set_burst(h, 0) == 1 and L.vad_pump_set_burst(h, 9) == 1
    assert L.vad_pump_burst_steps(h, 2) < 0 and L.vad_pump_burst_steps(h, -1) < 0
    assert L.vad_pump_burst_probs(h, 0, 3) is None and L.vad_pump_burst_probs(h, 2, 0) is None and L.vad_pump_burst_probs(h, 0, -1) is None
    bad = [([2], [4 * n - 100], None, None),                         # 100 pending + 4N - 100: a fourth chunk with max_burst = 3
           ([2, 5, 2], [2 * n, 8, 2 * n - 100], None, None),         # ... over two rows
           (list(range(cap)) + [0], [8] * (cap + 1), None, None),    # more rows than streams
           ([0], [8], [3], None), ([0, 1], [8, 8], [0, 255], None),  # codecs
           ([cap], [8], None, None), ([-1], [8], None, None), ([0], [0], None, None), ([0, 1], [8, -5], None, None),
           ([0], [8], None, [8]), ([0], [8], None, [-16]), ([0], [16], None, [area - 16]), ([0], [17], [1], [area - 16]),
           ([0, 3, 0], [8, 8, 2 ** 31 - 1], None, None)]
    for streams, lengths, codecs, offsets in bad:
        with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
            pump.submit_burst(1, streams, lengths, codecs, offsets)
        assert pump.poll() == (None, None)
        assert [pump.pending(s) for s in range(cap)] == held
    assert L.vad_pump_submit_burst(h, 1, None, None, None, None, 1) == 1 and L.vad_pump_submit_burst(h, 2, None, None, None, None, 0) == 1
    for wrong in (lambda: pump.write_burst(1, [(0, np.zeros(0, np.int16))]), lambda: pump.write_burst(1, [(0, np.zeros(8, np.float32))]),
                  lambda: pump.write_burst(1, [(0, np.zeros(8, np.int16), "ulaw")]), lambda: pump.submit_burst(1, [0, 1], [8]),
                  lambda: pump.write_burst(1, [(0, np.zeros(cap * n + 8, np.int16))])):
        with pytest.raises(ValueError):
            wrong()
    pump.write_burst(0, [(0, pcm[:8])])                              # a tick in flight: the burst depth cannot change
    assert L.vad_pump_set_burst(h, 4) == 1
    pump.poll()
    held[0] = 8
    # the next valid tick on the slot the refusals named: the largest rows that fit, at the end of the slot; stream 2 completes 3 chunks
    a16 = pump.packet_area(1)
    a16[cap * n - 3 * n:] = pcm[100:100 + 3 * n]
    pump.submit_burst(1, [2], [3 * n], None, [area - 6 * n])
    ev, r = pump.poll()
    bp = pump.burst_probs(r)
    assert r == 1 and pump.burst_steps(1) == 3 and pump.pending(2) == 100 and pump.pending(0) == 8
    assert (bp[:, 2] >= 0).all() and (np.delete(bp, 2, axis=1) == -1.0).all()
    ref = StreamPump(model.engine, sr, streams=cap, parts=1, ring_slots=2)
    for j in range(3):
        ref.slot(0)[0] = pcm[j * n:(j + 1) * n]
        ref.submit_rows(0, [2])
        ref.poll()
        assert ref.probs(0)[2] == bp[j, 2]
    for x, y in zip(pump.state(2), ref.state(2)):
        assert np.array_equal(x, y)
    for p in (off, pump, ref):
        p.close()


def test_bursts_at_full_capacity(model, oracle, golden):
    """8 192 streams at 16 kHz, 20 ms packets, 44 ticks: streams stall for 1 ... 11 ticks and then deliver what they withheld as one long
    row in front of the tick's packet, so that in any tick about a tenth of the streams complete 2 ... 8 chunks; rows in a shuffled
    arrival order (a stream's long row in front of its packet).  Every stream equals the submit_rows route bit for bit; stream 0, which
    never stalls, agrees with the CPU oracle."""
    from silero_vad_amd import StreamPump
    sr, n, S, P, TT = 16000, 512, 8192, 320, 44
    pcm = golden["16k"]["pcm_i16"]
    origin = (np.arange(S, dtype=np.int64) * 7919) % (len(pcm) - (TT + 14) * P)
    rng = np.random.default_rng(31)
    pump = StreamPump(model.engine, sr, streams=S, parts=2, ring_slots=3, max_burst=8)
    ref = StreamPump(model.engine, sr, streams=S, parts=2, ring_slots=3)
    sent = np.zeros(S, np.int64)
    owed = np.zeros(S, np.int64)                                     # packets withheld so far
    quiet = np.zeros(S, np.int64)                                    # ticks the stream stays silent
    mid = (rng.random(S) < 0.6) & (np.arange(S) > 0)                 # the run starts in mid-traffic: stalls of every age, not a wave of them
    quiet[mid] = rng.integers(1, 12, int(mid.sum()))
    owed[mid] = rng.integers(0, 12, int(mid.sum())) % (12 - quiet[mid])
    nchunks = ((TT + 12) * P) // n + 1
    got = np.full((S, nchunks), np.nan, np.float32)
    want = np.full((S, nchunks), np.nan, np.float32)
    got_ev, want_ev = [], []
    deep, bursting = 0, []
    for t in range(TT):
        stall = (quiet == 0) & (owed == 0) & (rng.random(S) < 0.25) & (np.arange(S) > 0)     # (stream 0 never stalls)
        quiet[stall] = rng.integers(1, 12, int(stall.sum()))
        silent = quiet > 0
        owed[silent] += 1
        quiet[silent] -= 1
        on = np.flatnonzero(~silent)
        # a delivering stream's rows: what it withheld as ONE long row (owed x 20 ms), then this tick's packet
        long_ = on[owed[on] > 0]
        st = np.concatenate([long_, on])
        ln = np.concatenate([owed[long_] * P, np.full(len(on), P)])
        a = np.concatenate([sent[long_], sent[on] + owed[on] * P])
        key = np.concatenate([rng.random(len(long_)), rng.random(len(on))])
        first = key[:len(long_)].copy()
        second = key[len(long_):][np.searchsorted(on, long_)]
        key[:len(long_)] = np.minimum(first, second)                 # (a stream's long row stays in front of its packet)
        key[len(long_) + np.searchsorted(on, long_)] = np.maximum(first, second)
        order = np.argsort(key, kind="stable")
        st, ln, a = st[order], ln[order], a[order]
        off = np.zeros(len(st), np.int64)
        off[1:] = np.cumsum((ln[:-1] + 7) // 8 * 8)
        total = int(ln.sum())
        assert len(st) <= S and int(off[-1] + ln[-1]) <= S * n
        excl = np.cumsum(ln) - ln
        within = np.arange(total) - np.repeat(excl, ln)
        pump.packet_area(t % 3)[np.repeat(off, ln) + within] = pcm[np.repeat(origin[st] + a, ln) + within]
        pump.submit_burst(t % 3, st, ln, None, off * 2)
        before = sent // n
        sent[on] += (owed[on] + 1) * P
        owed[on] = 0
        k = sent // n - before
        steps = max(1, int(k.max()))
        deep = max(deep, steps)
        bursting.append(int((k >= 2).sum()))
        ev, r = pump.poll()
        assert pump.burst_steps(r) == steps
        bp = pump.burst_probs(r)
        polled = []
        for j in range(steps):
            done = np.flatnonzero(k > j)
            got[done, before[done] + j] = bp[j][done]
            assert (bp[j][k <= j] == -1.0).all()
            ref.slot(0)[:len(done)] = pcm[(origin[done] + (before[done] + j) * n)[:, None] + np.arange(n)[None, :]]
            ref.submit_rows(0, done)
            e2, _ = ref.poll()
            want[done, before[done] + j] = ref.probs(0)[done]
            polled += e2
        got_ev.append(ev)
        want_ev.append(polled)
    assert deep == 8 and 0.05 * S < np.mean(bursting[12:TT - 12]) < 0.2 * S
    assert not np.isnan(got[:, :int(sent.min()) // n]).any()
    assert np.array_equal(got, want, equal_nan=True)
    assert got_ev == want_ev
    for s in range(S):
        assert pump.pending(s) == sent[s] % n
    for s in list(range(0, S, 61)) + [S - 1]:
        for x, y in zip(pump.state(s), ref.state(s)):
            assert np.array_equal(x, y), s
    m = int(sent[0]) // n
    x = pcm[origin[0]:origin[0] + m * n][None, :].astype(np.float32) / 32768.0
    assert np.abs(got[0, :m] - oracle.audio_forward(x, sr)[0]).max() < TIGHT
    pump.close()
    ref.close()
