"""Silent rows of the pump (VAD_ROW_SILENT, csrc/pump.hip + kernel_present.hip): a row that stands for `len` samples of digital silence
and occupies no bytes of the slot -- a lost packet, a DTX / comfort-noise period -- on the packet, coded, burst and wide routes.  The
feature is defined by reduction to behaviour the pump already has: every result here is compared, bit for bit, with a second pump fed,
through the SAME route and in the same row position, a payload row of int16 zeros.  Before every tick of the pump under test its whole
sample area is filled with 0x5A5A: a silent row that read the slot cannot pass.
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
CAP = 40                                                        # two full 16-stream tiles and a half tile
S16, ULAW, ALAW = 0, 1, 2


@pytest.fixture(scope="module")
def model(built):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback to silently pass on)")
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    assert m.engine._h, "native engine not created"
    return m


def encode(pcm, law):
    """int16 -> G.711 codes: the code whose expansion is nearest (ties to the lower value)."""
    from silero_vad_amd import g711_expand
    codes = np.arange(256, dtype=np.uint8)
    lin = g711_expand(codes, law).astype(np.int32)
    order = np.argsort(lin, kind="stable")
    v = lin[order]
    x = pcm.astype(np.int32)
    j = np.clip(np.searchsorted(v, x), 1, len(v) - 1)
    j -= (x - v[j - 1]) <= (v[j] - x)
    return codes[order[j]]


def feed(pump, route, r, rows, zeros):
    """One tick of `route` over slot r.  rows: [(stream, x, aux), ...] in row order; x = a sample array (int16, or uint8 G.711 codes),
    or an int = that many samples of silence; aux = the row's codec number (coded, burst) or step (wide), unused on the packet route.
    zeros=False: the pump under test -- the area is filled with 0x5A5A, payload rows are packed back to back, silent rows get the
    offset ROW_SILENT and keep their aux (the pump must not look at a silent row's codec).  zeros=True: the reference -- a silent row is
    a payload row of int16 zeros in the same position (codec S16), which existing code handles."""
    from silero_vad_amd import ROW_SILENT
    area = pump.wide_slot(r) if route == "wide" else pump.packet_bytes(r)
    if not zeros:
        area.view(np.int16)[:] = 0x5A5A
    st, ln, aux, off, at = [], [], [], [], 0
    for s, x, a in rows:
        quiet = isinstance(x, int)
        st.append(s)
        ln.append(x if quiet else len(x))
        if quiet and not zeros:
            off.append(ROW_SILENT)
            aux.append(a)
            continue
        if quiet:
            x = np.zeros(x, np.int16)
            a = S16 if route in ("coded", "burst") else a
        assert at + x.nbytes <= len(area)
        area[at:at + x.nbytes] = x.view(np.uint8)
        off.append(at)
        aux.append(a)
        at += (x.nbytes + 15) // 16 * 16
    if route == "packets":
        pump.submit_packets(r, st, ln, [o // 2 if o >= 0 else o for o in off])
    elif route == "coded":
        pump.submit_coded_packets(r, st, ln, np.array(aux, np.uint8), off)
    elif route == "burst":
        pump.submit_burst(r, st, ln, np.array(aux, np.uint8), off)
    else:
        pump.submit_wide_packets(r, st, ln, aux, off)


class Pair:
    """The pump under test (`got`: silent rows) and its reference (`ref`: rows of int16 zeros), cloned from one engine and driven in
    lock step; every retired tick's probabilities, events and sub-steps must be equal."""

    def __init__(self, model, sr, cap=CAP, wide=0, **kw):
        from silero_vad_amd import StreamPump
        self.got = StreamPump(model.engine, sr, streams=cap, **kw)
        self.ref = StreamPump(model.engine, sr, streams=cap, **kw)
        if wide:
            self.got.set_wideband(wide)
            self.ref.set_wideband(wide)
        self.cap, self.n, self.wide = cap, self.got.n, wide
        self.events, self.stepped = [], 0
        self.probs = [[] for _ in range(cap)]

    def tick(self, route, r, rows):
        feed(self.got, route, r, rows, zeros=False)
        feed(self.ref, route, r, rows, zeros=True)

    def retire(self):
        (ev, r), (ev_ref, r_ref) = self.got.poll(), self.ref.poll()
        assert r == r_ref and r is not None
        p, q = self.got.probs(r), self.ref.probs(r)
        assert np.array_equal(p, q)
        assert ev == ev_ref
        assert self.got.burst_steps(r) == self.ref.burst_steps(r)
        bp = self.got.burst_probs(r)
        assert np.array_equal(bp, self.ref.burst_probs(r))
        self.events += ev
        self.stepped += int((bp >= 0).sum())
        for s in np.flatnonzero(p >= 0):
            self.probs[s].append(float(p[s]))
        return bp, ev

    def counts(self):
        out = [self.got.pending(s) for s in range(self.cap)]
        assert out == [self.ref.pending(s) for s in range(self.cap)]
        if self.wide:
            ph = [self.got.wide_phase(s) for s in range(self.cap)]
            assert ph == [self.ref.wide_phase(s) for s in range(self.cap)]
            out += ph
        return out

    def finish(self):
        assert self.got.poll() == (None, None) and self.ref.poll() == (None, None)
        self.counts()
        for s in range(self.cap):
            for x, y in zip(self.got.state(s), self.ref.state(s)):
                assert np.array_equal(x, y), s

    def close(self):
        self.got.close()
        self.ref.close()


# ------------------------------------------------------------------------------------------------------------ 1, 5: the packet route

_PACKET_RUN = {}


def packet_run(model, golden):
    """The scenario of tests 1 and 5, run once: 40 streams at 16 kHz (N = 512), 40 ticks, speech in 10 / 20 / 30 ms packets (and odd
    lengths), two or three gaps of 3 ... 25 packets per stream as silent rows, ~10 % of rows missing (absent), two ticks without rows,
    two ticks whose rows are all silent, two ticks in flight.  Streams 0 ... 3 open with scripted rows that hit the listed alignments."""
    if _PACKET_RUN:
        return _PACKET_RUN
    SR, N, T = 16000, 512, 40
    pcm = golden["16k"]["pcm_i16"]
    rng = np.random.default_rng(61)
    src = [np.roll(pcm, -(30 * N + s * 7919)) for s in range(CAP)]
    at, total = [0] * CAP, [0] * CAP
    audio = [[] for _ in range(CAP)]
    script = {0: [("P", 160), ("S", 351), ("S", 1), ("S", N), ("P", 160)],           # c + len = N - 1; c = 511, len 1 -> N; len = N at c = 0
              1: [("P", 161), ("S", 352), ("P", 160), ("S", 191), ("S", N)],         # c = 161 -> N + 1; a payload behind the residue; -> N; len N
              2: [("P", 511), ("S", N), ("P", 320), ("S", 1)],                       # c = 511, c + len = 2N - 1; a payload behind 511 zeros
              3: [("S", 7), ("S", 1), ("P", 503), ("S", N - 1), ("P", 2)]}           # silent rows at c = 0 and 7; the reverse orders
    gaps = {}
    for s in range(CAP):
        starts = sorted(int(t) for t in rng.choice(np.arange(6, T - 4), 2 + s % 2, replace=False))
        gaps[s] = {t: (25 if s % 10 == 3 and k == 0 else int(rng.integers(3, 9))) for k, t in enumerate(starts)}
    left = [0] * CAP
    empty, hush = {9, 27}, {15, 16}
    seen = {"c%8": set(), "c+len": set(), "len": set(), "P after S": 0, "S after P": 0, "all silent": 0, "absent": 0, "rows": 0}
    last = [None] * CAP                                         # the kind of the row that left the stream's residue
    pair = Pair(model, SR, parts=3, ring_slots=3)
    for t in range(T + 2):
        if t < T:
            rows = []
            for s in range(CAP) if t not in empty else ():
                left[s] += gaps[s].get(t, 0)
                if script.get(s):
                    kind, ln = script[s].pop(0)
                elif t in hush or left[s] > 0:
                    kind, ln = "S", int(rng.choice([160, 320, 480]))
                    left[s] = max(0, left[s] - 1)
                elif rng.random() < 0.1:
                    seen["absent"] += 1
                    continue
                else:
                    kind, ln = "P", int(rng.choice([160, 320, 480])) if rng.random() < 0.7 else int(rng.integers(1, N + 1))
                c = total[s] % N
                if kind == "S":
                    seen["c%8"].add(c % 8), seen["c+len"].add(c + ln), seen["len"].add(ln)
                    audio[s].append(np.zeros(ln, np.int16))
                    rows.append((s, ln, 0))
                else:
                    x = np.ascontiguousarray(src[s][at[s]:at[s] + ln])
                    at[s] += ln
                    audio[s].append(x)
                    rows.append((s, x, 0))
                if c > 0 and last[s] is not None and last[s] != kind:
                    seen["P after S" if kind == "P" else "S after P"] += 1
                total[s] += ln
                last[s] = kind
            rows = [rows[i] for i in rng.permutation(len(rows))]
            seen["rows"] += len(rows)
            seen["all silent"] += bool(rows) and all(isinstance(x, int) for _, x, _ in rows)
            pair.tick("packets", t % 3, rows)
            for s in range(CAP):
                assert pair.got.pending(s) == total[s] % N, (t, s)
        if t >= 2:
            pair.retire()
    pair.finish()
    _PACKET_RUN.update(pair=pair, seen=seen, audio=[np.concatenate(a) for a in audio], total=total, N=N, SR=SR)
    return _PACKET_RUN


def test_packet_route_silent_rows_equal_rows_of_zeros(model, golden):
    """Test 1 of the issue: every tick of `got` (silent rows) equals `ref` (int16 zeros through vad_pump_submit_packets), and the
    population met every listed alignment."""
    run = packet_run(model, golden)
    seen, N, pair = run["seen"], run["N"], run["pair"]
    assert {0, 1, 7} <= seen["c%8"], seen["c%8"]
    assert {N - 1, N, N + 1, 2 * N - 1} <= seen["c+len"], sorted(seen["c+len"])
    assert {1, N} <= seen["len"]
    assert seen["P after S"] >= 4 and seen["S after P"] >= 4
    assert seen["all silent"] == 2
    assert 0.05 * seen["rows"] < seen["absent"] < 0.2 * seen["rows"]
    assert pair.stepped == sum(t // N for t in run["total"]) and len(pair.events) > 0


def test_packet_route_agrees_with_the_oracle(model, golden, oracle):
    """Test 5: four streams of test 1, spread over the three tiles, against the CPU oracle on their concatenated audio with zeros in
    the gaps."""
    run = packet_run(model, golden)
    N, pair = run["N"], run["pair"]
    pick = [1, 13, 22, 38]
    m = min(run["total"][s] // N for s in pick)
    assert m >= 12
    x = np.stack([run["audio"][s][:m * N] for s in pick]).astype(np.float32) / 32768.0
    assert all((run["audio"][s][:m * N] == 0).sum() > 3 * 160 for s in pick)
    want = oracle.audio_forward(x, run["SR"])
    got = np.array([pair.probs[s][:m] for s in pick], np.float32)
    assert np.abs(got - want).max() < TIGHT
    pair.close()
    _PACKET_RUN.clear()


# ------------------------------------------------------------------------------------------------------------ 2: the coded route, DTX

def test_coded_route_dtx_gaps_end_the_segment_during_the_gap(model, golden):
    """8 kHz, N = 256, streams in int16, mu-law and A-law.  Speech for 16 ticks, then the streams with s % 2 == 0 fall silent for 20
    ticks of 20 ms (400 ms > min_silence_duration_ms = 100) while the others talk on, then everybody talks again.  Every fifth tick
    lists the G.711 streams' payload rows not at all (absent): those ticks hold int16 and silent rows only and take the int16 kernel,
    the others take the coded kernel.  Silent rows carry the codec entry 2, in one tick 200.  `got` emits the 'end' of at least four
    streams during the gap; a third pump fed the payload rows alone (the gap rows absent) has emitted none of them by then."""
    from silero_vad_amd import StreamPump
    SR, N, PK, GAP = 8000, 256, 160, 20
    pcm = golden["8k"]["pcm_i16"]
    rng = np.random.default_rng(67)
    law = [("s16", "ulaw", "alaw")[s % 3] for s in range(CAP)]
    at = [(80 + s) * N for s in range(CAP)]                     # (the fixture's first long speech run: chunks 78 ... 189)
    pair = Pair(model, SR, parts=3, ring_slots=3)
    idle = StreamPump(model.engine, SR, streams=CAP, parts=3, ring_slots=3)
    idle_events, mixed, plain, flying = [], 0, 0, 0

    def payload(s, ln):
        x = np.ascontiguousarray(pcm[at[s]:at[s] + ln])
        at[s] += ln
        return (s, x, S16) if law[s] == "s16" else (s, encode(x, law[s]), (ULAW, ALAW)[law[s] == "alaw"])

    def run(t, rows):
        nonlocal mixed, plain, flying
        rows = [rows[i] for i in rng.permutation(len(rows))]
        g711 = any(not isinstance(x, int) and a != S16 for _, x, a in rows)
        quiet = any(isinstance(x, int) for _, x, _ in rows)
        mixed += g711 and quiet and {ULAW, ALAW} <= {a for _, x, a in rows if not isinstance(x, int)}
        plain += quiet and not g711
        pair.tick("coded", t % 3, rows)
        feed(idle, "coded", t % 3, [row for row in rows if not isinstance(row[1], int)], zeros=True)
        flying += 1
        if flying == 2:                                         # (two ticks in flight)
            retire()

    def retire():
        nonlocal flying
        pair.retire()
        idle_events.extend(idle.poll()[0])
        flying -= 1

    def drain():
        while flying:
            retire()
        assert idle.poll() == (None, None)

    t = 0
    for k in range(16):                                         # speech; the first row of odd length, so that c is unaligned from then on
        rows = [payload(s, 1 + (37 * s) % N if k == 0 else PK) for s in range(CAP) if k % 5 != 4 or law[s] == "s16"]
        run(t, rows)
        t += 1
    drain()
    talking = {s for s in range(CAP) if sum(1 if "start" in e else -1 for b, e in pair.events if b == s) == 1}
    dtx = sorted(s for s in talking if s % 2 == 0)
    assert len(dtx) >= 4 and {law[s] for s in dtx} == {"s16", "ulaw", "alaw"}
    before = len(pair.events)
    for k in range(GAP):                                        # the gap: silent rows with a codec entry the pump must not look at
        rows = [(s, PK, 200 if k == 3 else ALAW) if s % 2 == 0 else payload(s, PK) for s in range(CAP)
                if s % 2 == 0 or k % 5 != 4 or law[s] == "s16"]
        run(t, rows)
        t += 1
    drain()                                                     # (every gap tick retired; the next payload rows are not yet submitted)
    ended = sorted({b for b, e in pair.events[before:] if "end" in e} & set(dtx))
    assert len(ended) >= 4 and {law[s] for s in ended} == {"s16", "ulaw", "alaw"}, (dtx, ended)
    assert not any("end" in e and b in dtx for b, e in idle_events)
    for s in dtx:                                               # the clock ran: GAP x 160 samples beyond the absent pump's
        assert pair.got.pending(s) == (idle.pending(s) + GAP * PK) % N
    for k in range(10):                                         # everybody talks again
        run(t, [payload(s, PK) for s in range(CAP)])
        t += 1
    drain()
    assert mixed >= 8 and plain >= 2
    dtx = ended
    starts = [e["start"] for b, e in pair.events[before:] if "start" in e and b in dtx]
    assert starts and all(x > 16 * PK for x in starts)          # event samples count the gap
    pair.finish()
    pair.close()
    idle.close()


# ------------------------------------------------------------------------------------------------------------ 3: the burst route

def test_burst_route_silent_rows_of_several_chunks(model, golden):
    """max_burst = 4.  One tick holds: stream 0's payload, a silent row of 2N + 5, payload; stream 1 completing exactly 4 chunks from one
    silent row of 4N; stream 2 doing so from four silent rows of N (c = 0); G.711 rows beside them.  A tick in which stream 3 would
    complete 5 chunks from a silent row is refused with nothing queued.  Then ten random burst ticks with silent rows of 1 ... 2N."""
    from silero_vad_amd import _lib
    SR, N = 16000, 512
    pcm = golden["16k"]["pcm_i16"]
    rng = np.random.default_rng(71)
    cur = [40 * N]

    def take(n):
        cur[0] += n
        return np.ascontiguousarray(pcm[cur[0] - n:cur[0]])

    pair = Pair(model, SR, parts=3, ring_slots=3, max_burst=4)
    pair.tick("burst", 0, [(3, take(100), S16), (0, 9, ALAW), (5, 2 * N - 1, ULAW)])
    pair.retire()
    before = pair.counts()
    assert before[0] == 9 and before[3] == 100 and before[5] == N - 1
    for rows in ([(0, take(8), S16), (4, 5 * N, S16)],                               # 5 chunks from c = 0
                 [(3, 4 * N, S16), (3, take(8), S16), (3, N - 108, ULAW)],           # c = 100: 100 + 4N + 8 + N - 108 = 5N
                 [(5, 2 * N, S16), (5, 2 * N, S16), (5, 1, 77)]):                    # c = N - 1: ... + 4N + 1 = 5N
        for pump in (pair.got, pair.ref):
            with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
                feed(pump, "burst", 1, rows, zeros=pump is pair.ref)
            assert pump.poll() == (None, None)
        assert pair.counts() == before
    big = [(0, take(200), S16), (1, 4 * N, ALAW), (2, N, S16), (0, 2 * N + 5, 200), (7, encode(take(300), "ulaw"), ULAW),
           (2, N, ULAW), (0, take(300), S16), (2, N, S16), (8, 30, ALAW), (8, encode(take(130), "alaw"), ALAW), (2, N, S16),
           (3, 4 * N - 1, S16), (5, take(3 * N + 1), S16)]
    pair.tick("burst", 1, big)
    bp, _ = pair.retire()
    assert pair.got.burst_steps(1) == 4 and (bp[:, 1] >= 0).all() and (bp[:, 2] >= 0).all()
    assert (bp[:, 0] >= 0).sum() == 3 and (bp[:, 3] >= 0).sum() == 4 and (bp[:, 5] >= 0).sum() == 4
    assert pair.counts()[:9] == [(9 + 200 + 2 * N + 5 + 300) % N, 0, 0, 99, 0, 0, 0, 300, 160]
    for t in range(10):
        rows, area = [], CAP * N * 2 - 64                       # (the reference's rows of zeros must fit its sample area)
        for s in rng.permutation(CAP)[:18]:
            room = 5 * N - 1 - pair.got.pending(int(s))
            for _ in range(int(rng.integers(1, 3))):
                ln = min(int(rng.integers(1, 2 * N + 1)) if rng.random() < 0.3 else int(rng.integers(1, 300)), room, area // 2 - 8)
                if ln < 1:
                    break
                room -= ln
                area -= (2 * ln + 15) // 16 * 16
                rows.append((int(s), ln, int(rng.integers(0, 256))) if rng.random() < 0.5 or ln > 400 else (int(s), take(ln), S16))
        pair.tick("burst", (2 + t) % 3, rows)
        if t >= 1:
            pair.retire()
    pair.retire()
    assert pair.stepped > 60
    pair.finish()
    pair.close()


# ------------------------------------------------------------------------------------------------------------ 4: the wide route

def test_wide_route_silent_rows_advance_the_comb(model, golden):
    """max_step = 3, streams at steps 1, 2 and 3 side by side, 32 ticks: silent rows at every phase, of len = 1 (keeping nothing at a
    phase other than 0), of step * N, and at a change of the stream's step (the phase restarts).  The phase tracked here equals
    wide_phase after every tick."""
    SR, N, T = 16000, 512, 32
    pcm = golden["16k"]["pcm_i16"]
    rng = np.random.default_rng(73)
    cur = [35 * N]

    def take(n):
        cur[0] += n
        return np.ascontiguousarray(pcm[cur[0] - n:cur[0]])

    step, phase, held = [0] * CAP, [0] * CAP, [0] * CAP
    at_phase, kept_none, full, changed = set(), 0, set(), 0
    script = {0: [(1, 3, "S"), (1, 3, "S"), (1, 3, "S"), (3 * N, 3, "S"), (100, 2, "S"), (7, 2, "S"), (2 * N, 2, "S")],
              1: [(1, 2, "S"), (1, 2, "S"), (2 * N, 2, "S"), (101, 3, "P"), (50, 3, "S"), (N, 1, "S")],
              2: [(500, 3, "P"), (1, 3, "S"), (3 * N, 3, "S"), (1, 3, "S"), (3 * N - 1, 3, "S")]}
    pair = Pair(model, SR, wide=3, parts=3, ring_slots=3)
    for t in range(T + 2):
        if t < T:
            rows = []
            for s in range(CAP) if t % 13 != 12 else ():
                if script.get(s):
                    ln, k, kind = script[s].pop(0)
                elif rng.random() < 0.1:
                    continue
                else:
                    k = 1 + s % 3
                    ln = int(rng.choice([160, 320, 480])) * k if rng.random() < 0.6 else int(rng.integers(1, k * N + 1))
                    kind = "S" if rng.random() < 0.45 else "P"
                ph = phase[s] if k == step[s] else 0
                kept = len(range((-ph) % k, ln, k))
                if kind == "S":
                    at_phase.add((k, ph))
                    kept_none += kept == 0
                    full |= {k} if ln == k * N else set()
                    changed += k != step[s] and step[s] != 0
                step[s], phase[s], held[s] = k, (ph + ln) % k, (held[s] + kept) % N
                rows.append((s, ln if kind == "S" else take(ln), k))
            rows = [rows[i] for i in rng.permutation(len(rows))]
            pair.tick("wide", t % 3, rows)
            assert pair.counts() == held + phase, t
        if t >= 2:
            pair.retire()
    assert at_phase == {(k, ph) for k in (1, 2, 3) for ph in range(k)}
    assert kept_none >= 4 and full == {1, 2, 3} and changed >= 2
    assert pair.stepped > 4 * CAP
    pair.finish()
    pair.close()


# ------------------------------------------------------------------------------------------------------------ 6: refusals

def test_refusals_queue_nothing(model, golden):
    """On every route offsets -2 and -16 are VAD_ERR_ARG, and so are silent rows of length 0, of N + 1 (packet, coded) and of
    step * N + 1 (wide), and a silent row for a stream listed twice (packet, coded, wide).  Pending counts and phases stay, nothing is
    queued, the chunk routes still refuse a stream with a silent residue pending, and the next valid tick of every route -- through the
    write_* helpers where there is one -- equals the reference."""
    from silero_vad_amd import _lib
    SR, N = 16000, 512
    pcm = golden["16k"]["pcm_i16"][45 * N:]
    pair = Pair(model, SR, wide=3, parts=1, ring_slots=2, max_burst=4)
    pump = pair.got
    pair.tick("packets", 0, [(1, 100, 0), (2, pcm[:77], 0)])
    pair.retire()
    pair.tick("wide", 1, [(6, 100, 3), (9, 101, 2)])
    pair.retire()
    before = pair.counts()
    assert [before[s] for s in (1, 2, 6, 9)] == [100, 77, 34, 51] and before[CAP + 6] == 1 and before[CAP + 9] == 1
    none = None
    cases = {
        "packets": [([0], [8], none, [-2]), ([0], [8], none, [-16]), ([0], [0], none, [-1]), ([0], [N + 1], none, [-1]),
                    ([4, 4], [8, 8], none, [-1, -1]), ([4, 4], [8, 8], none, [0, -1]), ([4, 0, 4], [8, 8, 8], none, [-1, 0, 8]),
                    ([3, 0], [8, 8], none, [-1, -3])],
        "coded": [([0], [8], [0], [-2]), ([0], [8], [1], [-16]), ([0], [0], [0], [-1]), ([0], [N + 1], [2], [-1]),
                  ([4, 4], [8, 8], [0, 0], [-1, -1]), ([4, 4], [8, 8], [1, 9], [0, -1]), ([3, 0], [8, 8], [9, 9], [-1, 0])],
        "burst": [([0], [8], [0], [-2]), ([0], [8], [1], [-16]), ([0], [0], [0], [-1]), ([3, 0], [8, -5], [0, 0], [-1, -1]),
                  ([3, 0], [8, 8], [9, 9], [-1, 0])],
        "wide": [([0], [8], [3], [-2]), ([0], [8], [3], [-16]), ([0], [0], [3], [-1]), ([0], [3 * N + 1], [3], [-1]),
                 ([0], [2 * N + 1], [2], [-1]), ([0], [N + 1], [1], [-1]), ([4, 4], [8, 8], [3, 3], [-1, -1]),
                 ([4, 4], [8, 8], [3, 2], [0, -1]), ([0], [8], [0], [-1]), ([0], [8], [4], [-1])]}
    call = {"packets": lambda st, ln, aux, off: pump.submit_packets(1, st, ln, off),
            "coded": lambda st, ln, aux, off: pump.submit_coded_packets(1, st, ln, aux, off),
            "burst": lambda st, ln, aux, off: pump.submit_burst(1, st, ln, aux, off),
            "wide": lambda st, ln, aux, off: pump.submit_wide_packets(1, st, ln, aux, off)}
    for route, rows in cases.items():
        for case in rows:
            with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
                call[route](*case)
            assert pump.poll() == (None, None), (route, case)
            assert pair.counts() == before, (route, case)
    # a silent residue is pending like any other: the chunk routes refuse the stream
    for bad in (lambda: pump.submit_rows(1, [1]), lambda: pump.submit(1)):
        with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
            bad()
    assert pump.poll() == (None, None) and pair.counts() == before
    # the next valid tick of every route
    pump.packet_area(0)[:] = 0x5A5A
    pump.write_packets(0, [(1, N - 100), (2, pcm[100:300]), (4, 8)])
    pair.ref.write_packets(0, [(1, np.zeros(N - 100, np.int16)), (2, pcm[100:300]), (4, np.zeros(8, np.int16))])
    p = pair.retire()[0][0]
    assert p[1] >= 0 and pump.pending(1) == 0 and pump.pending(4) == 8
    pump.packet_area(1)[:] = 0x5A5A
    pump.write_coded_packets(1, [(4, N, "alaw"), (2, encode(pcm[300:500], "ulaw"), "ulaw")])
    pair.ref.write_coded_packets(1, [(4, np.zeros(N, np.int16), "s16"), (2, encode(pcm[300:500], "ulaw"), "ulaw")])
    p = pair.retire()[0][0]
    assert p[4] >= 0 and pump.pending(4) == 8
    pump.packet_area(0)[:] = 0x5A5A
    pump.write_burst(0, [(4, 3 * N + 5), (2, pcm[500:600]), (4, 2, "ulaw")])
    pair.ref.write_burst(0, [(4, np.zeros(3 * N + 5, np.int16)), (2, pcm[500:600]), (4, np.zeros(2, np.int16))])
    bp, _ = pair.retire()
    assert (bp[:, 4] >= 0).sum() == 3 and pump.pending(4) == 15
    pair.tick("wide", 1, [(6, 3 * N, 3), (9, pcm[600:700], 2), (0, 1, 3)])
    p = pair.retire()[0][0]
    assert p[6] >= 0 and pump.wide_phase(6) == 1 and pump.pending(6) == 34 and pump.pending(0) == 1
    pair.finish()
    pair.close()
