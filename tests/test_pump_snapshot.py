"""Snapshot and restore of the pump's live streams (vad_pump_export_streams / vad_pump_import_streams, csrc/pump.hip +
kernel_snapshot.hip): a stream leaves one pump as bytes and goes on in any slot of another, bit for bit.  The reference treats
(_state, _context) plus the VADIterator's triggered / temp_end / current_sample as the resumable unit (src/silero_vad/utils_vad.py:
500-549), so "bit for bit" is measured twice: against the same streams run without interruption on one pump, and -- stream 0, which
plays the whole fixture -- against the reference's own iterator events and probabilities.
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import collections

import numpy as np
import pytest
import torch

from conftest import SRS
from test_pump_packets import chunk_of, packet_plan, schedule
from test_pump_wide import widen

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
MOVED = {0: 23, 15: 0, 16: 16, 27: 15, 39: 7}                   # stream of pump A -> slot of pump B
DIRTY = 7                                                       # ticks B runs before the import: odd


@pytest.fixture(scope="module")
def model(built):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback to silently pass on)")
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    assert m.engine._h, "native engine not created"
    return m


class Out:
    """Probabilities by (stream name, chunk index) and events by stream name, collected over any number of pumps."""

    def __init__(self, nchunks):
        self.probs = collections.defaultdict(lambda: np.full(nchunks, np.nan, np.float32))
        self.events = collections.defaultdict(list)


def drive(pump, ticks, t0, t1, audio, slot_of, out):
    """Ticks t0 ... t1 - 1 of `ticks` ([(stream name, first sample, length), ...] per tick) through the packet route, one tick in flight;
    only the packets of the names in slot_of are fed, name s into slot slot_of[s].  Everything is retired on return."""
    n, R = pump.n, pump.ring_slots
    name = {slot: s for s, slot in slot_of.items()}
    prev = None
    for t in range(t0, t1 + 1):
        if t < t1:
            pk = [(s, a, ln) for s, a, ln in ticks[t] if s in slot_of]
            pump.write_packets(t % R, [(slot_of[s], audio[s][a:a + ln]) for s, a, ln in pk])
            cur = [(s, (a + ln) // n - 1) for s, a, ln in pk if (a + ln) // n > a // n]
        if t > t0:
            ev, r = pump.poll()
            p = pump.probs(r)
            on = np.zeros(pump.streams, bool)
            for s, k in prev:
                out.probs[s][k] = p[slot_of[s]]
                on[slot_of[s]] = True
            assert (p[~on] == -1.0).all()                       # VAD_PROB_ABSENT: no chunk completed
            for slot, e in ev:
                assert on[slot], "a stream without a completed chunk emitted an event"
                out.events[name[slot]].append(e)
        prev = cur
    assert pump.poll() == (None, None)


def final(pump, slot_of):
    return {s: (pump.state(slot), pump.pending(slot)) for s, slot in slot_of.items()}


def same_final(a, b, names):
    for s in names:
        assert a[s][1] == b[s][1], s
        for x, y in zip(a[s][0], b[s][0]):
            assert np.array_equal(x, y), s


def same_out(a, b, names):
    for s in names:
        assert np.array_equal(a.probs[s], b.probs[s], equal_nan=True), s
        assert a.events[s] == b.events[s], s


def plan_migration(golden, tag):
    """The audio and the tick lists of `migration` (host only)."""
    sr, g = SRS[tag], golden[tag]
    n = chunk_of(sr)
    pcm = g["pcm_i16"]
    T = len(pcm) // n
    rec = golden["segments"][tag]["iterator"]["default"]
    start, end = rec["events"][0]["start"], rec["events"][1]["end"]
    cut_sample = -(-(start + (end - start) // 4) // n) * n       # a chunk boundary a quarter into the first segment
    assert start + 2 * n < cut_sample < end - 2 * n
    rng = np.random.default_rng(23)
    capA, capB = 40, 24
    audio = {s: np.roll(pcm, -s * 7919)[:T * n if s == 0 else cut_sample + 40 * n - int(rng.integers(0, n))].copy() for s in range(capA)}
    ticks = schedule([packet_plan(len(audio[s]), n, sr, rng) for s in range(capA)], rng, always=(0,))
    sent0 = np.cumsum([sum(ln for s, a, ln in pk if s == 0) for pk in ticks])
    cut = int(np.argmax(sent0 >= cut_sample)) + 1                # ticks A runs before the export
    if (cut - DIRTY) % 2 == 0:                                   # B's context parity must differ from A's: one more (empty) tick for A
        ticks.insert(0, [])
        cut += 1
    assert sum(1 for pk in ticks[:cut] for s, _, _ in pk if s == 15) < cut - 1                                                    # missed ticks
    # the other audio of B's slots: names 100 + slot
    other = {100 + j: np.roll(pcm, -(50 * n + j * 4513))[:30 * n - int(rng.integers(0, n))].copy() for j in range(capB)}
    oticks = schedule([packet_plan(len(other[100 + j]), n, sr, rng) for j in range(capB)], rng, empty_every=10 ** 9)
    oticks = [[(100 + j, a, ln) for j, a, ln in pk] for pk in oticks]
    assert len(oticks) > DIRTY + 20
    ticksB = [oticks[u] if u < DIRTY else (oticks[u] if u < len(oticks) else []) + [p for p in ticks[cut + u - DIRTY] if p[0] in MOVED]
              for u in range(DIRTY + len(ticks) - cut)]
    stop = max(t for t, pk in enumerate(ticks) if any(s for s, _, _ in pk)) + 3        # every stream but 0 has played its audio by then
    assert cut + 40 < stop < len(ticks)
    return dict(tag=tag, sr=sr, n=n, T=T, rec=rec, cut_sample=cut_sample, audio=audio, other=other, ticks=ticks, oticks=oticks, ticksB=ticksB, cut=cut,
                stop=stop)


_scenes = {}


def migration(model, golden, tag):
    """The scenario of the first two tests, run once per sample rate.  Pump A: 40 streams, parts=3, ring_slots=3, the packet plan of
    test_pump_packets.py; stream 0 plays the whole fixture with a packet every tick.  A0 runs uninterrupted.  A1 stops at the cut, a
    tick strictly inside stream 0's first speech segment (from the reference's iterator events), exports MOVED's streams and goes on to
    the end (an export changes nothing); both are also read at tick `stop`, by which every stream but 0 has played all its audio.
    B (24 streams, parts=1, ring_slots=4) and its twin B' run DIRTY ticks of other audio in every slot; B imports the records into MOVED's slots and is fed the rest of those streams' packets beside the other audio of its other
    19 slots; B' runs the other audio alone."""
    if tag in _scenes:
        return _scenes[tag]
    from silero_vad_amd import StreamPump, snapshot_info
    sc = plan_migration(golden, tag)
    sr, n, T, rec, audio, other, ticks, oticks, ticksB, cut, stop = (sc[k] for k in ("sr", "n", "T", "rec", "audio", "other", "ticks", "oticks", "ticksB", "cut",
                                                                                       "stop"))
    capA, capB = 40, 24
    kw = dict(**rec["init"])
    allA = {s: s for s in range(capA)}

    a0 = StreamPump(model.engine, sr, streams=capA, parts=3, ring_slots=3, **kw)
    sc["A0"] = Out(T)
    drive(a0, ticks, 0, stop, audio, allA, sc["A0"])
    sc["A0_at_stop"] = (final(a0, allA), {s: sc["A0"].probs[s].copy() for s in allA}, {s: list(sc["A0"].events[s]) for s in allA})
    drive(a0, ticks, stop, len(ticks), audio, allA, sc["A0"])
    sc["A0_final"] = final(a0, allA)
    a0.close()

    a1 = StreamPump(model.engine, sr, streams=capA, parts=3, ring_slots=3, **kw)
    sc["A1"], sc["moved"] = Out(T), Out(T)
    drive(a1, ticks, 0, cut, audio, allA, sc["A1"])
    for s in MOVED:                                              # what the moved streams did on A
        sc["moved"].probs[s][:] = sc["A1"].probs[s]
        sc["moved"].events[s] = list(sc["A1"].events[s])
    blob = a1.export_streams(list(MOVED))
    sc["info"] = snapshot_info(blob)
    sc["pending_at_cut"] = [a1.pending(s) for s in MOVED]
    sc["parity"] = (cut, DIRTY)
    drive(a1, ticks, cut, stop, audio, allA, sc["A1"])
    sc["A1_final"] = final(a1, allA)
    sc["A1_at_stop"] = ({s: sc["A1"].probs[s].copy() for s in allA}, {s: list(sc["A1"].events[s]) for s in allA})
    drive(a1, ticks, stop, len(ticks), audio, allA, sc["A1"])
    sc["A1_end"] = final(a1, allA)
    a1.close()

    othersB = {100 + j: j for j in range(capB)}
    keepB = {s: j for s, j in othersB.items() if j not in MOVED.values()}
    b = StreamPump(model.engine, sr, streams=capB, parts=1, ring_slots=4, **kw)
    sc["B"] = Out(T)
    drive(b, ticksB, 0, DIRTY, other, othersB, sc["B"])
    sc["dirty_pending"] = [b.pending(j) for j in MOVED.values()]
    b.import_streams(blob, list(MOVED.values()))
    both = {**keepB, **MOVED}
    drive(b, ticksB, DIRTY, len(ticksB), {**other, **audio}, both, sc["B"])
    for s in MOVED:
        later = ~np.isnan(sc["B"].probs[s])
        assert np.isnan(sc["moved"].probs[s][later]).all()       # no chunk was stepped on both pumps
        sc["moved"].probs[s][later] = sc["B"].probs[s][later]
        sc["moved"].events[s] += sc["B"].events[s]
    sc["B_final"] = final(b, both)
    b.close()

    b2 = StreamPump(model.engine, sr, streams=capB, parts=1, ring_slots=4, **kw)
    sc["B2"] = Out(T)
    drive(b2, ticksB, 0, DIRTY, other, othersB, sc["B2"])
    drive(b2, ticksB, DIRTY, len(oticks), other, keepB, sc["B2"])
    sc["B2_final"] = final(b2, keepB)
    b2.close()
    sc["keepB"] = keepB
    _scenes[tag] = sc
    return sc


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_a_migrated_stream_continues_bit_for_bit(model, golden, tag):
    """Streams {0, 15, 16, 27, 39} of A (40 streams, three uneven parts) move, at a tick inside stream 0's first speech segment and with
    samples pending, into slots {23, 0, 16, 15, 7} of B (24 streams, one part, dirty slots, the other context parity): every later
    probability, event, the final (h, c, context) and the pending count are those of the uninterrupted run; stream 0, A's part and
    B's part joined, gives the reference VADIterator's own events and stays within TIGHT of its probabilities."""
    sc = migration(model, golden, tag)
    g, T, n = golden[tag], sc["T"], sc["n"]
    info = sc["info"]
    assert len(info) == len(MOVED)
    assert info[0]["triggered"] == 1 and info[0]["current_sample"] == sc["cut_sample"] and info[0]["active"] == 1
    assert [f["pending"] for f in info] == sc["pending_at_cut"]
    assert sum(f["pending"] > 0 for f in info) >= 3              # the carries are not empty
    for f, s in zip(info, MOVED):
        assert (f["pending_samples"][f["pending"]:] == 0).all()
        sent = f["current_sample"] + f["pending"]
        assert np.array_equal(f["pending_samples"][:f["pending"]], sc["audio"][s][f["current_sample"]:sent]), s
        assert f["wide_step"] == 0 and f["wide_phase"] == 0
    assert (sc["parity"][0] - sc["parity"][1]) % 2 == 1 and sc["parity"][1] % 2 == 1
    assert any(sc["dirty_pending"])                              # the slots the records went into were dirty
    same_out(sc["moved"], sc["A0"], MOVED)
    for s in MOVED:
        k = len(sc["audio"][s]) // n
        assert not np.isnan(sc["moved"].probs[s][:k]).any() and np.isnan(sc["moved"].probs[s][k:]).all(), s
    same_final(sc["B_final"], sc["A0_final"], MOVED)
    assert sc["moved"].events[0] == sc["rec"]["events"], tag   # the reference's own iterator events (39 / 92)
    assert len(sc["B"].events[0]) > 30
    assert np.abs(sc["moved"].probs[0] - np.asarray(g["probs_wav"]).reshape(-1)[:T]).max() < TIGHT


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_nobody_else_notices(model, golden, tag):
    """B's other 19 slots equal a pump B' that ran the same audio with no import -- probabilities, events, state, pending -- and A,
    continued after the export, equals the uninterrupted A on all 40 streams: at the tick by which every stream but 0 has played all its
    audio, and at the end of the fixture."""
    sc = migration(model, golden, tag)
    assert len(sc["keepB"]) == 19
    same_out(sc["B"], sc["B2"], sc["keepB"])
    assert all(not np.isnan(sc["B"].probs[s][:25]).any() for s in sc["keepB"])
    same_final(sc["B_final"], sc["B2_final"], sc["keepB"])
    want_final, want_probs, want_events = sc["A0_at_stop"]
    for s in range(40):
        assert np.array_equal(sc["A1_at_stop"][0][s], want_probs[s], equal_nan=True), s
        assert sc["A1_at_stop"][1][s] == want_events[s], s
    same_final(sc["A1_final"], want_final, range(40))
    same_out(sc["A1"], sc["A0"], range(40))                      # ... and to the end of the fixture
    same_final(sc["A1_end"], sc["A0_final"], range(40))
    assert (~np.isnan(want_probs[0])).sum() > (~np.isnan(want_probs[15])).sum() > sc["cut_sample"] // sc["n"] + 30


def raw_import(pump, blob, slots, records=None):
    """vad_pump_import_streams as it is: the Python wrapper's own checks are not in the way."""
    sl = np.asarray(slots, np.int32)
    rc = None if records is None else np.asarray(records, np.int32)
    return pump._L.vad_pump_import_streams(pump._h, blob.ctypes.data, blob.size, None if rc is None else rc.ctypes.data, sl.ctypes.data, len(sl))


def chunk_tick(pump, r, rows):
    pump.slot(r)[:] = rows
    pump.submit(r)
    ev, rr = pump.poll()
    assert rr == r
    return pump.probs(r).copy(), ev


def twin_ticks_agree(a, b, rows):
    """The next tick of both pumps: same probabilities, events, state and pending counts in every slot."""
    (p, ev), (q, ev2) = chunk_tick(a, 0, rows), chunk_tick(b, 0, rows)
    assert np.array_equal(p, q) and ev == ev2
    for s in range(a.streams):
        assert a.pending(s) == b.pending(s)
        for x, y in zip(a.state(s), b.state(s)):
            assert np.array_equal(x, y), s


def test_wide_streams_keep_their_comb(model, golden):
    """Two 16 kHz pumps with set_wideband(3).  At the cut stream 3 is at step 3 with phase 2, stream 16 at step 2 with phase 1, stream 19
    at step 1 and stream 8 never had a wide row; rows are zero-stuffed, so a wrong phase keeps the stuffing.  In other slots of the second
    pump they continue bit for bit and wide_phase() agrees.  The same blob into a pump without wideband: VAD_ERR_ARG, nothing changed."""
    from silero_vad_amd import StreamPump, _lib, snapshot_info
    sr, n, cap = 16000, 512, 20
    pcm = golden["16k"]["pcm_i16"]
    step = {3: 3, 16: 2, 19: 1}
    per_tick = {3: 3 * 480 + 1, 16: 2 * 480 + 1, 19: 480, 8: 333}
    dest = {3: 17, 16: 3, 19: 0, 8: 16}
    cut, total = 5, 17
    src = {s: np.roll(pcm, -(30 * n + s * 7919)) for s in per_tick}
    wide = {s: widen(src[s][:total * 481], k, hold=False) for s, k in step.items()}

    def feed(pump, t, slot_of):
        """tick t: one wide tick for the comb streams, one packet tick for stream 8 -> [(name, probability), ...], events by name"""
        got, evs = [], []
        rows = [(s, wide[s][t * per_tick[s]:(t + 1) * per_tick[s]]) for s in step]
        at, offs = 0, []
        for s, x in rows:
            pump.wide_slot(0)[at:at + 2 * len(x)] = x.view(np.uint8)
            offs.append(at)
            at += (2 * len(x) + 15) // 16 * 16
        pump.submit_wide_packets(0, [slot_of[s] for s, _ in rows], [len(x) for _, x in rows], [step[s] for s, _ in rows], offs)
        pump.write_packets(1, [(slot_of[8], src[8][t * 333:(t + 1) * 333])])
        name = {v: k for k, v in slot_of.items()}
        for _ in range(2):
            ev, r = pump.poll()
            p = pump.probs(r)
            got += sorted((name[j], float(p[j])) for j in np.flatnonzero(p >= 0))        # (by name: the slots differ from pump to pump)
            evs += sorted(((name[j], e) for j, e in ev), key=lambda x: x[0])
        return got, evs

    def run(pump, t0, t1, slot_of):
        got, evs = [], []
        for t in range(t0, t1):
            a, b = feed(pump, t, slot_of)
            got += a
            evs += b
        return got, evs

    same = {s: s for s in per_tick}
    u = StreamPump(model.engine, sr, streams=cap, parts=2, ring_slots=2)
    u.set_wideband(3)
    want = run(u, 0, total, same)
    assert len(want[0]) > 40 and want[1]
    a = StreamPump(model.engine, sr, streams=cap, parts=2, ring_slots=2)
    a.set_wideband(3)
    head = run(a, 0, cut, same)
    assert [a.wide_phase(s) for s in (3, 16, 19, 8)] == [2, 1, 0, 0]
    blob = a.export_streams(list(per_tick))
    info = dict(zip(per_tick, snapshot_info(blob)))
    assert [(info[s]["wide_step"], info[s]["wide_phase"]) for s in (3, 16, 19, 8)] == [(3, 2), (2, 1), (1, 0), (0, 0)]
    assert all(info[s]["pending"] > 0 for s in per_tick)
    b = StreamPump(model.engine, sr, streams=cap, parts=1, ring_slots=2)
    b.set_wideband(3)
    chunk_tick(b, 0, np.stack([np.roll(pcm, -(90 * n + j * 4513))[:n] for j in range(cap)]))       # dirty slots, the other context parity
    b.import_streams(blob, [dest[s] for s in per_tick])
    assert [b.wide_phase(dest[s]) for s in (3, 16, 19, 8)] == [2, 1, 0, 0]
    tail = run(b, cut, total, dest)
    assert (head[0] + tail[0], head[1] + tail[1]) == want
    for s in per_tick:
        assert b.pending(dest[s]) == u.pending(s) and b.wide_phase(dest[s]) == u.wide_phase(s), s
        for x, y in zip(b.state(dest[s]), u.state(s)):
            assert np.array_equal(x, y), s
    # a pump without wideband, and one whose max_step is smaller: refused, nothing changes; their twins never see the call
    rows = np.stack([np.roll(pcm, -(60 * n + j * 4513))[:2 * n] for j in range(cap)])
    for max_step, bad, fine in ((0, [0, 1], [2, 3]), (2, [0], [1, 2, 3])):
        c, c2 = (StreamPump(model.engine, sr, streams=cap, parts=2, ring_slots=2) for _ in range(2))
        for p in (c, c2):
            if max_step:
                p.set_wideband(max_step)
            chunk_tick(p, 0, rows[:, :n])
            p.write_packets(1, [(j, rows[j, n:n + 100 + j]) for j in range(cap)])
            p.poll()
        before = [(c.state(j), c.pending(j)) for j in range(cap)]
        for records in (None, bad, bad + fine, fine + bad[:1]):
            k = 4 if records is None else len(records)
            assert raw_import(c, blob, list(range(5, 5 + k)), records) == 1
            with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
                c.import_streams(blob, list(range(5, 5 + k)), records)
        for j in range(cap):
            assert c.pending(j) == before[j][1] == 100 + j
            for x, y in zip(c.state(j), before[j][0]):
                assert np.array_equal(x, y), j
        c.write_packets(0, [(j, rows[j, n + 100 + j:2 * n]) for j in range(cap)])       # the next tick completes every slot's chunk
        c2.write_packets(0, [(j, rows[j, n + 100 + j:2 * n]) for j in range(cap)])
        (ev, r), (ev2, r2) = c.poll(), c2.poll()
        assert np.array_equal(c.probs(r), c2.probs(r2)) and (c.probs(r) >= 0).all() and ev == ev2
        c.import_streams(blob, [6, 5], fine[:2])                # the records it can take go in
        assert c.pending(6) == info[list(per_tick)[fine[0]]]["pending"]
        c.close()
        c2.close()
    for p in (u, a, b):
        p.close()


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_exports_are_deterministic_and_round_trip(model, golden, tag):
    """Two exports with no tick between them are byte-identical; streams exported, imported into other slots of the same pump and
    exported from there give byte-identical records; a subset export holds the records of the whole-pump export."""
    from silero_vad_amd import StreamPump, _lib
    sr = SRS[tag]
    n = chunk_of(sr)
    pcm = golden[tag]["pcm_i16"]
    cap = 37
    pump = StreamPump(model.engine, sr, streams=cap, parts=3, ring_slots=2)
    rng = np.random.default_rng(5)
    for t in range(9):                                           # packets of every length: carries of every length, stale tails behind them
        pump.write_packets(t % 2, [(s, np.roll(pcm, -(30 * n + s * 7919 + t * n))[:int(rng.integers(1, n + 1))]) for s in range(cap) if rng.random() < 0.8])
        pump.poll()
    pump.close_stream(4)
    src, dst = [36, 0, 4, 17, 16], [1, 35, 20, 15, 31]
    one, two = pump.export_streams(src), pump.export_streams(src)
    assert one.dtype == np.uint8 and one.shape == (int(_lib.lib().vad_pump_snapshot_bytes(sr, len(src))),)
    assert np.array_equal(one, two)
    whole = pump.export_streams()
    assert np.array_equal(whole, pump.export_streams(list(range(cap))))
    stride = (len(whole) - 64) // cap
    for i, s in enumerate(src):
        assert np.array_equal(one[64 + i * stride:64 + (i + 1) * stride], whole[64 + s * stride:64 + (s + 1) * stride]), s
    assert sum(pump.pending(s) > 0 for s in src) >= 3
    pump.import_streams(one, dst)
    assert np.array_equal(pump.export_streams(dst), one)
    assert np.array_equal(pump.export_streams(src), one)          # the sources are as they were
    pump.import_streams(whole, dst, records=src)                  # one blob dealt out by record index
    assert np.array_equal(pump.export_streams(dst), one)
    empty = pump.export_streams([])
    assert len(empty) == 64
    pump.import_streams(empty, [])
    pump.close()


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_a_whole_pump_moves(model, golden, tag):
    """100 streams run the first 300 ticks of the fixture; export_streams(None), imported in reversed slot order into a fresh pump with
    another `parts`; the next 300 ticks equal the uninterrupted pump's under the renaming."""
    from silero_vad_amd import StreamPump
    sr = SRS[tag]
    n = chunk_of(sr)
    pcm = golden[tag]["pcm_i16"]
    cap, K = 100, 300
    rows = np.ascontiguousarray(np.stack([np.roll(pcm, -s * 7919)[:2 * K * n] for s in range(cap)]))
    a = StreamPump(model.engine, sr, streams=cap, parts=3, ring_slots=2)
    for t in range(K):
        chunk_tick(a, t % 2, rows[:, t * n:(t + 1) * n])
    blob = a.export_streams()
    b = StreamPump(model.engine, sr, streams=cap, parts=7, ring_slots=3)
    b.import_streams(blob, list(range(cap))[::-1])
    n_events = 0
    for t in range(K, 2 * K):
        p, ev = chunk_tick(a, t % 2, rows[:, t * n:(t + 1) * n])
        q, ev2 = chunk_tick(b, t % 3, rows[::-1, t * n:(t + 1) * n])
        assert np.array_equal(p, q[::-1]), t
        assert ev == sorted(((cap - 1 - s, e) for s, e in ev2), key=lambda x: x[0]), t
        n_events += len(ev)
    assert n_events > 100
    for s in range(cap):
        for x, y in zip(a.state(s), b.state(cap - 1 - s)):
            assert np.array_equal(x, y), s
    a.close()
    b.close()


def test_a_closed_stream_travels_closed(model, golden):
    """A closed stream's record says so; in its new slot it emits no event although its probabilities cross the threshold, and
    open_stream then starts it from zero."""
    from silero_vad_amd import StreamPump, snapshot_info
    sr, n, cap = 16000, 512, 20
    pcm = golden["16k"]["pcm_i16"]
    rows = np.ascontiguousarray(np.stack([pcm[:80 * n]] * cap))     # (the fixture starts with speech: 'start' at sample 32)
    a = StreamPump(model.engine, sr, streams=cap, parts=2, ring_slots=2)
    a.close_stream(9)
    for t in range(10):
        p, ev = chunk_tick(a, 0, rows[:, t * n:(t + 1) * n])
        assert 9 not in [s for s, _ in ev]
    assert p[9] > 0.5
    blob = a.export_streams([9, 10])
    info = snapshot_info(blob)
    assert (info[0]["active"], info[1]["active"]) == (0, 1) and info[1]["triggered"] == 1
    b = StreamPump(model.engine, sr, streams=cap, parts=1, ring_slots=2)
    b.import_streams(blob, [2, 3])
    high = 0
    for t in range(10, 40):
        p, ev = chunk_tick(b, 0, rows[:, t * n:(t + 1) * n])
        q, ev_a = chunk_tick(a, 0, rows[:, t * n:(t + 1) * n])
        assert p[2] == q[9] and p[3] == q[10]
        assert [e for s, e in ev if s == 3] == [e for s, e in ev_a if s == 10]
        assert 2 not in [s for s, _ in ev]
        high += p[2] > 0.5
    assert high > 10
    b.open_stream(2)
    b.open_stream(5)                                             # a fresh slot beside it: the same audio, from zero
    events = {2: [], 5: []}
    for t in range(40):
        p, ev = chunk_tick(b, 0, rows[:, t * n:(t + 1) * n])
        assert p[2] == p[5]
        for s, e in ev:
            if s in events:
                events[s].append(e)
    assert events[2] == events[5] and events[2][0] == {"start": 32}
    a.close()
    b.close()


def test_refusals_on_a_live_pump_change_nothing(model, golden):
    """A tick in flight: VAD_ERR_ARG from both calls and the output buffer untouched.  An 8 kHz blob into a 16 kHz pump:
    VAD_ERR_SAMPLE_RATE.  A slot listed twice or out of range, a record index too large or negative, a truncated or corrupted blob:
    VAD_ERR_ARG.  After each refusal the pump's next tick equals that of a twin that never saw the call."""
    from silero_vad_amd import StreamPump, _lib
    n, cap = 512, 20
    pcm = golden["16k"]["pcm_i16"]
    rows = np.ascontiguousarray(np.stack([np.roll(pcm, -(30 * n + s * 7919))[:40 * n] for s in range(cap)]))
    pump, twin = (StreamPump(model.engine, 16000, streams=cap, parts=2, ring_slots=3) for _ in range(2))
    t = [0]

    def step():
        twin_ticks_agree(pump, twin, rows[:, t[0] * n:(t[0] + 1) * n])
        t[0] += 1

    for _ in range(3):
        step()
    blob = pump.export_streams([1, 2, 3])
    small = StreamPump(model.engine, 8000, streams=4, ring_slots=2)
    blob8 = small.export_streams([0, 1, 2])
    small.close()
    # a tick in flight
    pump.slot(1)[:] = rows[:, t[0] * n:(t[0] + 1) * n]
    pump.submit(1)
    out = np.full(len(blob), 0x5A, np.uint8)
    sl = np.array([1, 2, 3], np.int32)
    assert pump._L.vad_pump_export_streams(pump._h, sl.ctypes.data, 3, out.ctypes.data, len(out)) == 1
    assert (out == 0x5A).all()
    assert raw_import(pump, blob, [4, 5, 6]) == 1
    with pytest.raises(_lib.VadError, match="in flight"):
        pump.export_streams([1])
    with pytest.raises(_lib.VadError, match="in flight"):
        pump.import_streams(blob, [4, 5, 6])
    pump.poll()
    chunk_tick(twin, 1, rows[:, t[0] * n:(t[0] + 1) * n])
    t[0] += 1
    step()
    # export: a slot out of range or twice, a buffer too small
    for slots, size in (([1, cap], len(out)), ([-1], len(out)), ([1, 1], len(out)), ([1, 2, 3], len(out) - 1)):
        sl = np.array(slots, np.int32)
        assert pump._L.vad_pump_export_streams(pump._h, sl.ctypes.data, len(sl), out.ctypes.data, size) == 1
        assert (out == 0x5A).all()
    assert pump._L.vad_pump_export_streams(pump._h, None, 3, out.ctypes.data, len(out)) == 1        # NULL = every slot: n is the stream count
    step()
    # import
    assert raw_import(pump, blob8, [4, 5, 6]) == 2                # VAD_ERR_SAMPLE_RATE
    with pytest.raises(_lib.VadError, match="VAD_ERR_SAMPLE_RATE"):
        pump.import_streams(blob8, [4, 5, 6])
    step()
    bad_field = blob.copy()
    bad_field[64 + 16:64 + 20].view("<i4")[:] = n               # record 0: pending = N
    magic = blob.copy()
    magic[0] ^= 1
    for b, slots, records in ((blob, [4, 4, 5], None), (blob, [4, 5, cap], None), (blob, [4, -1], None), (blob, [4, 5, 6, 7], None),
                              (blob, [4, 5], [0, 3]), (blob, [4, 5], [-1, 0]), (blob[:-1].copy(), [4, 5, 6], None), (blob[:63].copy(), [4], None),
                              (bad_field, [4], [1]), (magic, [4], None)):
        assert raw_import(pump, b, slots, records) == 1, (slots, records)
        step()
    pump.import_streams(blob, [4, 5, 6])                          # ... and the call that is right goes through
    twin.import_streams(blob, [4, 5, 6])
    step()
    pump.close()
    twin.close()
