"""Blob version 2 of the pump's snapshots (vad_pump_export_streams_v2 / vad_pump_import_streams, kernel_snapshot.hip, the records with a tail):
streams that are BOUND to a resampled rate leave a pump as bytes and enter another.  The yardstick is the UNINTERRUPTED pump, not an
oracle: pump A runs every tick; pump B runs the first k ticks, exports version 2 and is closed; pump C imports -- into other slots, in
the other part -- and runs the rest on the same packets.  C must equal A bit for bit in every later tick's probabilities and events and,
after every tick, in state() (h, c, context), pending() and resample_state() of every stream.
The pumps have 32 slots in two parts of one 16-stream tile each and carry ten live streams, five in each part, one tick at a time over
ring_slots=2.  A tick is a resampled tick or, every third, an int16 packet tick for the streams that are bound to no rate.
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest
import torch

from test_pump_resample_gpu import model, speech  # noqa: F401  (the module fixtures)

pytestmark = pytest.mark.gpu

CAP = 32
SLOTS_A = [1, 3, 6, 9, 15, 16, 20, 22, 27, 31]          # live stream i of pumps A and B; five in each part
SLOTS_C = [18, 30, 16, 25, 21, 0, 14, 7, 2, 11]         # ... of pump C: other numbers, and every stream in the other part
SCENARIOS = {                                            # sample rate, the enabled rates, the rate of live stream i (0: bound to none)
    "16k": (16000, (44100, 24000), [44100, 24000, 44100, 0, 24000, 44100, 0, 24000, 44100, 44100]),
    "8k": (8000, (44100,), [44100, 44100, 44100, 0, 44100, 44100, 0, 44100, 44100, 44100]),
    "up": (16000, (11025, 44100), [11025, 11025, 44100, 0, 11025, 11025, 0, 11025, 44100, 11025]),
}
LATE_INPUTS = 5
EXACT, CLOSED, LATE = 2, 8, 9                            # roles: c = 0 right after a step at the cut; closed (and bound again); first row just before the cut


def chunk_of(sr):
    return 512 if sr == 16000 else 256


def row_capacity(rates, sr):
    from silero_vad_amd import resample_geometry
    n = chunk_of(sr)
    return (max(-(-n * resample_geometry(r, sr)[0] // resample_geometry(r, sr)[1]) for r in rates) + 7) // 8 * 8


class Plan:
    """The packets of every tick, made once per (scenario, k) on the host and played into every pump: ticks[t] = (kind, [(live stream,
    int16 samples)], [live streams closed in front of the tick]).  Per stream it keeps what the test later holds the blob against: the
    input since the stream was (last) bound, cut[i] = its length at the cut."""

    def __init__(self, name, k, ticks, golden, speech):
        from silero_vad_amd import resample_stream_ready
        self.sr, self.rates, self.rate = SCENARIOS[name]
        self.k, self.N = k, chunk_of(self.sr)
        self.A = row_capacity(self.rates, self.sr)
        N, sr = self.N, self.sr
        rng = np.random.default_rng(1000 * k + len(name))
        pcm = golden["16k" if sr == 16000 else "8k"]["pcm_i16"]
        audio = [np.roll(pcm, -(30 * N + 7919 * i)) if r == 0 else np.roll(speech(r, sr), -977 * i) for i, r in enumerate(self.rate)]
        pos, g, done = [0] * 10, [0] * 10, [0] * 10                # position in the audio; inputs since bound; chunks stepped since bound
        self.sent = [[] for _ in range(10)]                        # the rows since the stream was (last) bound
        self.ticks, self.cut, self.pending_at_cut = [], None, None
        assert (k - 1) % 3 != 1 and k >= 3                         # the tick in front of the cut is a resampled one

        def have(i, extra=0):                                      # outputs ready beyond the stepped chunks
            return resample_stream_ready(self.rate[i], sr, g[i] + extra) - done[i] * N

        def length_for(i, outputs):                                # the shortest row after which exactly `outputs` are pending
            n = 1
            while have(i, n) < outputs:
                n += 1
            assert have(i, n) == outputs and n <= self.A
            return n

        def at_the_cut():
            self.cut = [int(sum(len(x) for x in s)) for s in self.sent]
            self.pending_at_cut = [have(i) if self.rate[i] and g[i] else None for i in range(10)]

        for t in range(ticks):
            kind, rows, closes = ("pkt" if t % 3 == 1 else "res"), [], []
            if t == k:
                at_the_cut()
            if t == 2:                                             # the closed stream: unbound, its pending outputs dropped; its next row binds it again
                closes.append(CLOSED)
                g[CLOSED] = done[CLOSED] = 0
                self.sent[CLOSED] = []
            for i in rng.permutation(10):
                i = int(i)
                if self.rate[i] == 0:
                    if kind == "pkt":
                        n = int(rng.choice([80, 160, 240])) if sr == 8000 else int(rng.choice([160, 320, 480]))
                        rows.append((i, audio[i][pos[i]:pos[i] + n]))
                        pos[i] += n
                    continue
                if kind != "res" or (i == LATE and t < k - 1):
                    continue
                if i == LATE and t == k - 1:
                    n = LATE_INPUTS                                # fewer than H inputs at the cut
                elif i == EXACT and t <= k - 1:                    # half a chunk, then rows without an output, then exactly the chunk
                    n = length_for(i, N) if t == k - 1 else length_for(i, N // 2) if have(i) < N // 2 else 1
                elif rng.random() < 0.12:
                    continue                                       # a missed tick
                else:
                    ms10 = self.rate[i] / 100.0
                    own = row_capacity((self.rate[i],), sr)         # (a chunk's input at the stream's own rate: longer rows only fill up to 2 N - 1)
                    n = int(round(ms10 * int(rng.integers(1, 4)))) if rng.random() < 0.6 else int(rng.integers(1, own + 1))
                    n = min(n, self.A)
                    while have(i, n) >= 2 * N:
                        n -= 1
                rows.append((i, audio[i][pos[i]:pos[i] + n]))
                self.sent[i].append(rows[-1][1])
                pos[i] += n
                g[i] += n
                if have(i) >= N:
                    done[i] += 1
            self.ticks.append((kind, rows, closes))
        if ticks == k:
            at_the_cut()
        self.sent_at_cut = [np.concatenate(s + [np.zeros(0, np.int16)])[:c] for s, c in zip(self.sent, self.cut)]


class Run:
    """One pump and where the ten live streams sit in it."""

    def __init__(self, model, plan, slots, rates=None):
        from silero_vad_amd import StreamPump
        self.plan, self.slots = plan, list(slots)
        self.pump = StreamPump(model.engine, plan.sr, streams=CAP, parts=2, ring_slots=2)
        assert self.pump.parts == 2
        self.route = (rates if rates is not None else plan.rates)
        if self.route:
            self.pump.set_resample(self.route)
        self.live = {s: i for i, s in enumerate(self.slots)}

    def tick(self, t, only=None):
        """-> (the live streams' probabilities as bits, their events, what they carry afterwards); only: the live streams whose rows are
        played (a pump that holds a part of them)"""
        kind, rows, closes = self.plan.ticks[t]
        rows = [(i, x) for i, x in rows if only is None or i in only]
        for i in closes:
            self.pump.close_stream(self.slots[i])
        if kind == "res":
            self.pump.write_resampled_packets(t % 2, [(self.slots[i], x, self.plan.rate[i]) for i, x in rows])
        else:
            self.pump.write_packets(t % 2, [(self.slots[i], x) for i, x in rows])
        ev, r = self.pump.poll()
        assert self.pump.poll() == (None, None)
        probs = self.pump.probs(r)[self.slots].copy()
        events = sorted((self.live[s], tuple(e.items())) for s, e in ev if s in self.live)
        assert len(events) == len(ev)
        return probs.view(np.uint32).tolist(), events, self.carried()

    def carried(self):
        out = []
        for s in self.slots:
            out.append((self.pump.pending(s), self.pump.resample_state(s) if self.route else None, tuple(a.tobytes() for a in self.pump.state(s))))
        return out

    def close(self):
        self.pump.close()


def uninterrupted(model, plan):
    a = Run(model, plan, SLOTS_A)
    out = [a.tick(t) for t in range(len(plan.ticks))]
    a.close()
    assert sum(p != np.float32(-1.0).view(np.uint32) for probs, _, _ in out for p in probs) >= 20       # chunks were stepped ...
    return out


def first_k(model, plan, k, want):
    b = Run(model, plan, SLOTS_A)
    for t in range(k):
        assert b.tick(t) == want[t]
    return b


def continue_on(c, plan, k, want, only=None):
    for t in range(k, len(plan.ticks)):
        got = c.tick(t, only)
        for i in (range(10) if only is None else only):
            assert got[0][i] == want[t][0][i], ("probability", t, i)
            assert got[2][i] == want[t][2][i], ("pending / resample_state / state", t, i)
        assert [e for e in got[1] if only is None or e[0] in only] == [e for e in want[t][1] if only is None or e[0] in only], ("events", t)


@pytest.mark.parametrize("name,k", [("16k", 3), ("16k", 6), ("16k", 10), ("8k", 6), ("up", 6)])
def test_a_migrated_stream_continues_bit_for_bit(model, golden, speech, name, k):
    from silero_vad_amd import resample_stream_history, resample_stream_ready, snapshot_info
    plan = Plan(name, k, k + 7, golden, speech)
    want = uninterrupted(model, plan)
    b = first_k(model, plan, k, want)
    # what migrates: a stream younger than its history, one with c = 0 right after a step, streams mid-chunk, an unbound stream with
    # int16 samples pending, a closed stream
    H = resample_stream_history(plan.rate[LATE], plan.sr)
    assert LATE_INPUTS < H
    assert b.pump.resample_state(SLOTS_A[LATE]) == (plan.rate[LATE], LATE_INPUTS, resample_stream_ready(plan.rate[LATE], plan.sr, LATE_INPUTS))
    assert b.pump.pending(SLOTS_A[EXACT]) == 0 and b.pump.resample_state(SLOTS_A[EXACT])[0] == plan.rate[EXACT]
    assert want[k - 1][0][EXACT] != np.float32(-1.0).view(np.uint32)            # (stepped by the tick in front of the cut)
    mid = [i for i in range(10) if plan.rate[i] and 0 < b.pump.pending(SLOTS_A[i]) < plan.N]
    assert len(mid) >= 4 and len({b.pump.pending(SLOTS_A[i]) for i in mid}) >= 4
    assert any(plan.rate[i] == 0 and b.pump.pending(SLOTS_A[i]) > 0 for i in range(10))
    blob = b.pump.export_streams(SLOTS_A, version=2)
    info = snapshot_info(blob)
    assert info[CLOSED]["active"] == 0 and all(info[i]["active"] == 1 for i in range(10) if i != CLOSED)
    late = info[LATE]["resample"]["history"]
    assert not late[:H - LATE_INPUTS].any() and np.array_equal(late[H - LATE_INPUTS:], plan.sent_at_cut[LATE]) and late.any()
    b.close()
    c = Run(model, plan, SLOTS_C)
    c.pump.import_streams(blob, SLOTS_C)
    assert c.carried() == want[k - 1][2]
    continue_on(c, plan, k, want)
    c.close()


@pytest.mark.parametrize("name,k,extra", [("16k", 6, 96000), ("8k", 6, 96000)])
def test_the_destination_differs_from_the_source(model, golden, speech, name, k, extra):
    """C has one more rate, with a longer history, in front of the others: every rate index and the pitch of the history rows differ.
    The target slots were bound to that rate just before and hold its history and its pending outputs."""
    from silero_vad_amd import resample_stream_history
    plan = Plan(name, k, k + 7, golden, speech)
    want = uninterrupted(model, plan)
    b = first_k(model, plan, k, want)
    blob = b.pump.export_streams(SLOTS_A, version=2)
    b.close()
    rates_c = (extra,) + plan.rates
    pitch = lambda rates: (max(resample_stream_history(r, plan.sr) for r in rates) + 7) // 8 * 8
    assert pitch(rates_c) > pitch(plan.rates) and all(rates_c.index(r) != plan.rates.index(r) for r in plan.rates)
    c = Run(model, plan, SLOTS_C, rates=rates_c)
    foreign = speech(44100, plan.sr)                               # (any samples: played at the extra rate)
    for t in range(2):
        c.pump.write_resampled_packets(t, [(s, foreign[3000 * t + 100 * s:3000 * t + 100 * s + 1200], extra) for s in SLOTS_C])
        c.pump.poll()
    assert all(c.pump.resample_state(s)[0] == extra and c.pump.pending(s) > 0 for s in SLOTS_C)
    c.pump.import_streams(blob, SLOTS_C)
    assert c.carried() == want[k - 1][2]
    continue_on(c, plan, k, want)
    c.close()


@pytest.mark.parametrize("name", ["16k", "8k", "up"])
def test_the_blob_says_what_the_stream_holds(model, golden, speech, name):
    from silero_vad_amd import resample_device, resample_stream_history, resample_stream_ready, snapshot_info
    k = 6
    plan = Plan(name, k, k, golden, speech)
    b = Run(model, plan, SLOTS_A)
    for t in range(k):
        b.tick(t)
    info = snapshot_info(b.pump.export_streams(SLOTS_A, version=2))
    bound = 0
    for i, rec in enumerate(info):
        rs, s = rec["resample"], SLOTS_A[i]
        state = b.pump.resample_state(s)
        assert (rs["src_rate"], rs["inputs_mod"], rs["pending_out"]) == state and rec["pending"] == (0 if state[0] else b.pump.pending(s))
        if not state[0]:
            assert len(rs["carry"]) == len(rs["history"]) == 0 and rs["outputs_mod"] == 0
            continue
        bound += 1
        x = plan.sent_at_cut[i]
        H = resample_stream_history(plan.rate[i], plan.sr)
        assert np.array_equal(rs["history"], np.concatenate([np.zeros(H, np.int16), x])[-H:]), i
        ready, c = resample_stream_ready(plan.rate[i], plan.sr, len(x)), rs["pending_out"]
        assert c == ready % plan.N == plan.pending_at_cut[i] and len(rs["carry"]) == c
        if c:
            y = resample_device(model.engine, torch.from_numpy(x).to(model.device), None, plan.rate[i], plan.sr).cpu().numpy()
            assert rs["carry"].tobytes() == y[ready - c:ready].tobytes(), i
        O, Nr = _pair(plan.rate[i], plan.sr)
        assert rs["outputs_mod"] == ready % Nr and rs["inputs_mod"] == len(x) - ready // Nr * O
    assert bound == 8 and sum(len(r["resample"]["carry"]) > 0 for r in info) >= 5
    b.close()


def _pair(rate, sr):
    from silero_vad_amd import resample_geometry
    return resample_geometry(rate, sr)[:2]


# The edges of the kernels' record walk: 1, 4 and 5 records (a workgroup moves four, a wave each: one live wave, a full workgroup, a full
# one and one live wave), slots of every part of a pump of 37 streams in three parts (16 + 16 + 5), and pending counts on both sides of the
# edge of a 16-byte vector of the carry (8 samples).  A record is 146 or 106 vectors: a lane's last pass over it is ragged.
EDGE_LISTS = ([33], [2, 17, 33, 36], [36, 1, 20, 33, 16])
EDGE_PENDING = {33: 7, 17: 8, 36: 9, 2: 0, 1: 3, 20: 255, 16: 1}


def edge_pump(model, golden, sr, **kw):
    """-> the pump, every stream of EDGE_PENDING stepped on two chunks of speech and holding that many samples, and {stream: what it was fed}"""
    from silero_vad_amd import StreamPump
    n = chunk_of(sr)
    pump = StreamPump(model.engine, sr, streams=37, parts=3, ring_slots=2, **kw)
    assert pump.parts == 3
    pcm = golden["16k" if sr == 16000 else "8k"]["pcm_i16"]
    fed = {s: np.ascontiguousarray(np.roll(pcm, -(30 * n + 7919 * s))[:2 * n + c]) for s, c in EDGE_PENDING.items()}
    for t in range(3):
        pump.write_packets(t % 2, [(s, x[t * n:(t + 1) * n]) for s, x in fed.items() if len(x) > t * n])
        pump.poll()
    assert all(pump.pending(s) == c for s, c in EDGE_PENDING.items())
    return pump, fed


def edge_records_hold(pump, fed, slots, info):
    """the records of `slots` say what the pump's own accessors say of those streams, and what they were fed"""
    n = pump.n
    assert len(info) == len(slots)
    for s, rec in zip(slots, info):
        c = EDGE_PENDING[s]
        assert (rec["pending"], rec["current_sample"], rec["active"]) == (c, 2 * n, 1)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(pump.state(s), (rec["h"], rec["c"], rec["ctx"]))) and rec["h"].any() and rec["ctx"].any()
        assert np.array_equal(rec["pending_samples"][:c], fed[s][2 * n:]) and not rec["pending_samples"][c:].any()


def version_1_is_a_prefix_of_version_2_at_the_edges(model, golden, sr):
    from silero_vad_amd import snapshot_info
    n = chunk_of(sr)
    s1 = 32 + 4 * (256 + n // 8) + 2 * n
    s2 = s1 + 32 + 4 * n + 320
    pump, fed = edge_pump(model, golden, sr)
    twin, _ = edge_pump(model, golden, sr)
    for slots in EDGE_LISTS:
        v1, v2 = pump.export_streams(slots), pump.export_streams(slots, version=2)
        assert len(v1) == 64 + len(slots) * s1 and len(v2) == 96 + len(slots) * s2
        r1, r2 = v1[64:].reshape(-1, s1), v2[96:].reshape(-1, s2)
        assert np.array_equal(r2[:, :s1], r1) and not r2[:, s1:].any()
        edge_records_hold(pump, fed, slots, snapshot_info(v1))
        edge_records_hold(pump, fed, slots, snapshot_info(v2))
        # ... and enter other slots of another pump, in other parts, over what those held
        dst = [(s + 16) % 37 for s in slots]
        for blob in (v1, v2):
            twin.import_streams(blob, dst)
            assert all(twin.pending(d) == pump.pending(s) and all(a.tobytes() == b.tobytes() for a, b in zip(twin.state(d), pump.state(s)))
                       for s, d in zip(slots, dst))
            assert np.array_equal(twin.export_streams(dst, version=int(blob[8])), blob)
    pump.close()
    twin.close()


def test_version_1_is_a_prefix_of_version_2(model, golden, speech):
    from silero_vad_amd import StreamPump, snapshot_info
    k = 6
    plan = Plan("16k", k, k + 7, golden, speech)
    want = uninterrupted(model, plan)
    b = first_k(model, plan, k, want)
    unbound = [s for s in range(CAP) if b.pump.resample_state(s)[0] == 0]
    assert len(unbound) == CAP - 8 and any(b.pump.pending(s) > 0 for s in unbound)
    v1, v2 = b.pump.export_streams(unbound), b.pump.export_streams(unbound, version=2)
    s1, s2 = (len(v1) - 64) // len(unbound), (len(v2) - 96) // len(unbound)
    assert (s1, s2) == (2336, 4736) and np.array_equal(v2[:8], v1[:8]) and np.array_equal(v2[16:28], v1[16:28]) and np.array_equal(v2[32:64], v1[32:64])
    assert v2[8:16].view("<u4").tolist() == [2, 96] and v2[28:32].view("<u4")[0] == s2 and not v2[64:96].any()
    r1, r2 = v1[64:].reshape(-1, s1), v2[96:].reshape(-1, s2)
    assert np.array_equal(r2[:, :s1], r1) and not r2[:, s1:].any()
    # a pump without the route writes the same records for the same streams
    plain = StreamPump(model.engine, 16000, streams=CAP, parts=2, ring_slots=2)
    plain.import_streams(v1, unbound)
    assert np.array_equal(plain.export_streams(unbound, version=2), v2)
    plain.close()
    # two exports with no tick between them; a whole pump moves with streams=None
    whole = b.pump.export_streams(None, version=2)
    assert np.array_equal(whole, b.pump.export_streams(version=2)) and np.array_equal(whole, b.pump.export_streams(list(range(CAP)), version=2))
    assert len(whole) == 96 + CAP * s2 and len(snapshot_info(whole)) == CAP
    b.close()
    c = Run(model, plan, SLOTS_A)
    c.pump.import_streams(whole, list(range(CAP)))
    assert c.carried() == want[k - 1][2] and np.array_equal(c.pump.export_streams(version=2), whole)
    continue_on(c, plan, k, want)
    c.close()
    for sr in (16000, 8000):
        version_1_is_a_prefix_of_version_2_at_the_edges(model, golden, sr)


def test_refusals_change_nothing(model, golden, speech):
    from silero_vad_amd import StreamPump, _lib
    k = 6
    plan = Plan("16k", k, k + 4, golden, speech)
    want = uninterrupted(model, plan)
    b = first_k(model, plan, k, want)
    blob = b.pump.export_streams(SLOTS_A, version=2)
    refused = lambda: pytest.raises(_lib.VadError, match="VAD_ERR_ARG")
    # version 1 still refuses a bound stream, alone, among others and in the whole pump
    for streams in ([SLOTS_A[0]], [SLOTS_A[3], SLOTS_A[1]], None):
        with refused():
            b.pump.export_streams(streams)
        with refused():
            b.pump.export_streams(streams, version=1)
    for bad in (0, 3, "2"):
        with pytest.raises(ValueError):
            b.pump.export_streams(SLOTS_A, version=bad)
    # a tick in flight: no export, no import
    c = Run(model, plan, SLOTS_C)
    c.pump.import_streams(blob, SLOTS_C)
    before = c.carried()
    kind, rows, _ = plan.ticks[k]
    assert kind == "res"
    c.pump.write_resampled_packets(k % 2, [(c.slots[i], x, plan.rate[i]) for i, x in rows])
    for call in (lambda: c.pump.export_streams(SLOTS_C, version=2), lambda: c.pump.export_streams(version=2), lambda: c.pump.import_streams(blob, SLOTS_C)):
        with refused():
            call()
    ev, r = c.pump.poll()
    probs = c.pump.probs(r)[SLOTS_C].view(np.uint32).tolist()
    assert probs == want[k][0] and c.carried() == want[k][2]       # the tick was not disturbed
    c.close()
    # a pump without the route, and one whose rates lack the record's: nothing changes, and the next valid import and tick give A's bits
    for rates in ((), (24000, 22050)):
        c = Run(model, plan, SLOTS_C, rates=rates)
        bare = c.carried()
        bound_24k = [i for i in range(10) if plan.rate[i] == 24000]
        for recs in (list(range(10)), [3, 0], [0]) + (() if rates else ([bound_24k[0]],)):
            with refused():
                c.pump.import_streams(blob, [SLOTS_C[i] for i in recs], records=recs)
            assert c.pump.poll() == (None, None) and c.carried() == bare
        ok = [i for i in range(10) if plan.rate[i] in (0,) + tuple(rates)]      # the records this pump can take, it takes
        c.pump.import_streams(blob, [SLOTS_C[i] for i in ok], records=ok)
        got = c.carried()
        assert all(got[i] == (before[i] if rates else (before[i][0], None, before[i][2])) for i in ok)
        assert all(got[i] == bare[i] for i in range(10) if i not in ok)
        if rates:                                                  # ... and their next ticks are A's, bit for bit
            assert {plan.rate[i] for i in ok} == {0, 24000}
            continue_on(c, plan, k, want, only=ok)
        c.close()
    c = Run(model, plan, SLOTS_C)
    c.pump.import_streams(blob, SLOTS_C)
    continue_on(c, plan, k, want)
    # a version 2 record of a stream that is bound to no rate leaves a bound slot unbound, like a version 1 record
    i0 = plan.rate.index(0)
    target = SLOTS_C[0]
    assert c.pump.resample_state(target)[0] == plan.rate[0] != 0
    for version in (2, 1):
        unbound_blob = b.pump.export_streams([SLOTS_A[i0]], version=version)
        c.pump.import_streams(unbound_blob, [target])
        assert c.pump.resample_state(target) == (0, 0, 0) and c.pump.pending(target) == b.pump.pending(SLOTS_A[i0]) > 0
        for x, y in zip(c.pump.state(target), b.pump.state(SLOTS_A[i0])):
            assert np.array_equal(x, y)
        c.pump.import_streams(blob, [target], records=[0])         # ... and a bound record binds it again
        assert c.pump.resample_state(target) == b.pump.resample_state(SLOTS_A[0])
    b.close()
    c.close()
