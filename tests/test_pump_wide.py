"""The pump's wide packet route (vad_pump_set_wideband + vad_pump_submit_wide_packets, csrc/pump.hip + kernel_present.hip
assemble_wide_packets): WebRTC / Opus clients deliver 32 / 48 kHz int16, and the device keeps every step-th sample (the reference's
x[::step], src/silero_vad/utils_vad.py:39-42) on the way into the chunk, with the comb's phase carried per stream.  The route is defined
by reduction to the int16 packet route: every result here is compared, bit for bit, with a second pump fed each tick's rows decimated on
the host (numpy slicing at the phase tracked HERE; rows that keep no sample are not listed) through vad_pump_submit_packets.
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
SR, N, CAP, MAX_STEP = 16000, 512, 48, 3                        # three 16-stream tiles
AREA = CAP * N * MAX_STEP * 2                                   # bytes of a wide slot's sample area


@pytest.fixture(scope="module")
def model(built):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback to silently pass on)")
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    assert m.engine._h, "native engine not created"
    return m


def widen(x, step, hold):
    """x at 16 kHz -> step x 16 kHz whose comb [::step] is x: sample-and-hold, or zero-stuffing (other values between the kept ones)."""
    if hold:
        return np.repeat(x, step)
    w = np.full(len(x) * step, -77, np.int16)
    w[::step] = x
    return w


class Pair:
    """The pump under test (wideband enabled) and its reference (never enabled), driven in lock step: a wide tick goes to the first as
    it is and to the second decimated on the host, through write_packets; every other call goes to both.  Each retired tick's
    probabilities and events must be equal.  The comb rule is restated here: phase = input samples so far, modulo step, counted from
    open or from the row at which the stream's step changed."""

    def __init__(self, model, cap=CAP, max_step=MAX_STEP, **kw):
        from silero_vad_amd import StreamPump
        self.got = StreamPump(model.engine, SR, streams=cap, **kw)
        self.got.set_wideband(max_step)
        self.ref = StreamPump(model.engine, SR, streams=cap, **kw)
        self.cap = cap
        self.step, self.phase = [0] * cap, [0] * cap
        self.events = self.stepped = self.empty_rows = 0
        self.probs = [[] for _ in range(cap)]

    def wide(self, r, packets, offsets=None, steps_arg=True):
        """packets: [(stream, int16 samples, step), ...]; offsets: byte offsets into the wide slot, or None = back to back"""
        area = self.got.wide_slot(r)
        offs, at, rows = [], 0, []
        for i, (s, x, step) in enumerate(packets):
            o = at if offsets is None else offsets[i]
            area[o:o + 2 * len(x)] = x.view(np.uint8)
            offs.append(o)
            at = o + (2 * len(x) + 15) // 16 * 16
            ph = self.phase[s] if step == self.step[s] else 0
            kept = x[(-ph) % step::step]
            self.step[s], self.phase[s] = step, (ph + len(x)) % step
            self.empty_rows += len(kept) == 0
            if len(kept):
                rows.append((s, kept))
        self.got.submit_wide_packets(r, [s for s, _, _ in packets], [len(x) for _, x, _ in packets],
                                     [k for _, _, k in packets] if steps_arg else None, None if offsets is None else offs)
        self.ref.write_packets(r, rows)
        for s, _, _ in packets:
            assert self.got.wide_phase(s) == self.phase[s], s

    def both(self, fn):
        fn(self.got)
        fn(self.ref)

    def open_stream(self, s):
        self.both(lambda p: p.open_stream(s))
        self.step[s] = self.phase[s] = 0
        assert self.got.wide_phase(s) == 0 and self.got.pending(s) == 0

    def retire(self):
        (ev, r), (ev_ref, r_ref) = self.got.poll(), self.ref.poll()
        assert r == r_ref
        p, q = self.got.probs(r), self.ref.probs(r)
        assert np.array_equal(p, q)
        assert ev == ev_ref
        self.events += len(ev)
        self.stepped += int((p >= 0).sum())
        for s in np.flatnonzero(p >= 0):
            self.probs[s].append(float(p[s]))
        return p, ev

    def finish(self):
        assert self.got.poll() == (None, None) and self.ref.poll() == (None, None)
        for s in range(self.cap):
            assert self.got.pending(s) == self.ref.pending(s), s
            for x, y in zip(self.got.state(s), self.ref.state(s)):
                assert np.array_equal(x, y), s

    def close(self):
        self.got.close()
        self.ref.close()


def test_wide_packets_equal_the_host_decimated_packet_route(model, oracle, golden):
    """48 streams (three tiles) at 16 / 32 / 48 kHz side by side in every tick, ~50 ticks: 10 / 20 / 30 ms frames and uniform lengths in
    [1, step * N], ~10 % of ticks missed, empty ticks, rows in random arrival order, two ticks in flight.  Probabilities, events, the
    pending residue and the final (h, c, context) equal the packet route fed the host-decimated rows; the kept comb is the speech fixture,
    and four streams' probabilities agree with the CPU oracle on it."""
    pcm = golden["16k"]["pcm_i16"]
    rng = np.random.default_rng(31)
    steps = [1 + s % 3 for s in range(CAP)]
    base = [np.roll(pcm, -(30 * N + s * 7919))[:18 * N - int(rng.integers(0, N))] for s in range(CAP)]
    audio = [widen(base[s], steps[s], hold=s % 2 == 0) for s in range(CAP)]
    plans = []
    for s in range(CAP):
        lens, left, k = [], len(audio[s]), steps[s]
        while left > 0:
            ln = int(rng.choice([160, 320, 480])) * k if rng.random() < 0.7 else int(rng.integers(1, k * N + 1))
            lens.append(min(ln, left))
            left -= lens[-1]
        plans.append(lens)
    nxt, start, ticks = [0] * CAP, [0] * CAP, []
    while any(nxt[s] < len(plans[s]) for s in range(CAP)):
        pk = []
        if len(ticks) % 11 != 10:                               # (every 11th tick carries no row at all)
            for s in range(CAP):
                if nxt[s] < len(plans[s]) and rng.random() >= 0.1:
                    pk.append((s, audio[s][start[s]:start[s] + plans[s][nxt[s]]], steps[s]))
                    start[s] += plans[s][nxt[s]]
                    nxt[s] += 1
        ticks.append([pk[i] for i in rng.permutation(len(pk))])
    assert 25 <= len(ticks) <= 90 and sum(1 for pk in ticks if not pk) >= 2
    assert all(len({k for _, _, k in pk}) == 3 for pk in ticks[:5])
    pair = Pair(model, parts=3, ring_slots=3)
    for t in range(len(ticks) + 1):
        if t < len(ticks):
            pair.wide(t % 3, ticks[t])
        if t > 0:
            pair.retire()
    pair.finish()
    assert pair.stepped == sum(len(b) // N for b in base) and pair.events > 0
    for s in range(CAP):
        assert pair.got.pending(s) == len(base[s]) % N, s
        assert pair.got.wide_phase(s) == len(audio[s]) % steps[s], s
    pick = [0, 17, 31, 47]                                      # steps 1, 3, 2, 3
    m = min(len(base[s]) // N for s in pick)
    x = np.stack([base[s][:m * N] for s in pick]).astype(np.float32) / 32768.0
    want = oracle.audio_forward(x, SR)
    got = np.array([pair.probs[s][:m] for s in pick], np.float32)
    assert np.abs(got - want).max() < TIGHT
    pair.close()


def test_edge_rows(model, golden):
    """Hand-built rows: len = 1 at every phase (rows that keep nothing included), len = step * N at phase 0 and beyond, pending + kept
    equal to N - 1, N and N + 1, lengths of 8 k +- 1, a row that ends at the last byte of the area, steps=None (every row at max_step),
    a stream that changes its step mid-stream (the phase restarts), open / close with samples pending and a phase other than 0."""
    pcm = golden["16k"]["pcm_i16"][40 * N:]
    cur = [0]

    def take(n):
        cur[0] += n
        return np.ascontiguousarray(pcm[cur[0] - n:cur[0]])

    pair = Pair(model, parts=2, ring_slots=2)
    got = pair.got

    def tick(r, packets, **kw):
        pair.wide(r, packets, **kw)
        return pair.retire()[0]

    # len = 1 at each phase: step 3 keeps 1, 0, 0, 1 samples, step 2 keeps 1, 0, 1, step 1 always 1
    for i in range(4):
        tick(i % 2, [(0, take(1), 3), (1, take(1), 2), (2, take(1), 1)])
        assert [got.pending(s) for s in (0, 1, 2)] == [1 + i // 3, 1 + i // 2, 1 + i]
        assert [got.wide_phase(s) for s in (0, 1, 2)] == [(i + 1) % 3, (i + 1) % 2, 0]
    assert pair.empty_rows == 4
    # a tick whose only row keeps nothing: the reference's tick is empty
    p = tick(0, [(0, take(1), 3)])
    assert (p == -1.0).all() and got.wide_phase(0) == 2 and got.pending(0) == 2
    # len = step * N: at phase 0 on a fresh stream, and behind pending samples at phases 2 (stream 0) and 0 (streams 1, 2)
    p = tick(1, [(3, take(3 * N), 3), (4, take(2 * N), 2), (5, take(N), 1), (0, take(3 * N), 3), (1, take(2 * N), 2), (2, take(N), 1)])
    assert (p[:6] >= 0).all() and [got.pending(s) for s in range(6)] == [2, 2, 4, 0, 0, 0]
    # pending + kept = N - 1, N, N + 1: at phase 0 (streams 6 ... 8) and at phase 1 behind a row of 301 samples (streams 9 ... 11)
    tick(0, [(s, take(300), 3) for s in (6, 7, 8)] + [(s, take(301), 3) for s in (9, 10, 11)])
    assert [got.pending(s) for s in range(6, 12)] == [100] * 3 + [101] * 3 and got.wide_phase(9) == 1
    p = tick(1, [(6, take(3 * (N - 101)), 3), (7, take(3 * (N - 100)), 3), (8, take(3 * (N - 99)), 3),
                 (9, take(3 * (N - 102) + 2), 3), (10, take(3 * (N - 101) + 2), 3), (11, take(3 * (N - 100) + 2), 3)])
    assert [got.pending(s) for s in range(6, 12)] == [N - 1, 0, 1] * 2
    assert (p[[7, 8, 10, 11]] >= 0).all() and (p[[6, 9]] == -1.0).all()
    # lengths of 8 k +- 1 input samples and of 8 k +- 1 kept samples, every step; steps=None on a tick of max_step rows
    lens = [7, 9, 23, 25, 24 * 5 - 1, 24 * 5 + 1, 3 * 63, 3 * 65, 1535, 1529]
    tick(0, [(12 + i, take(ln), 3) for i, ln in enumerate(lens)], steps_arg=False)
    assert [got.pending(12 + i) for i in range(len(lens))] == [(ln + 2) // 3 % N for ln in lens]
    tick(1, [(12 + i, take(ln), 2) for i, ln in enumerate([15, 17, 1023, 1009, 127, 129])] +
            [(20 + i, take(ln), 1) for i, ln in enumerate([7, 9, 511])])
    # a row that ends at the last byte of the area, behind rows at bytes 16 and 48
    tick(0, [(24, take(3 * N), 3), (25, take(9), 3), (26, take(40), 2)], offsets=[AREA - 6 * N, 16, 48])
    assert got.pending(24) == 0 and got.pending(25) == 3 and got.pending(26) == 20
    # a stream that changes its step: 100 samples at step 3 leave phase 1; step 2 restarts at 0 and 101 samples leave 1; step 3 restarts
    for ln, k, ph in ((100, 3, 1), (101, 2, 1), (50, 3, 2), (50, 3, 1), (33, 1, 0), (4, 2, 0)):
        tick(1, [(27, take(ln), k)])
        assert got.wide_phase(27) == ph
    assert got.pending(27) == 34 + 51 + 17 + 17 + 33 + 2
    # open / close with samples pending at a phase other than 0: both drop the samples, open zeroes the phase
    tick(0, [(28, take(100), 3), (29, take(100), 3)])
    assert got.pending(28) == got.pending(29) == 34 and got.wide_phase(28) == 1
    pair.open_stream(28)
    pair.both(lambda q: q.close_stream(29))
    assert got.pending(29) == 0
    p = tick(1, [(28, take(3 * N), 3), (29, take(3 * N - 1), 3)])
    assert p[28] >= 0 and p[29] == -1.0 and got.pending(28) == 0 and got.pending(29) == N - 1     # (29's phase was kept: 1)
    pair.finish()
    pair.close()


def test_a_stream_moves_between_the_routes(model, golden):
    """Every stream alternates between wide ticks (48 kHz, lengths that leave every phase), int16 packet ticks, coded ticks (int16 and
    G.711 rows) and burst ticks (two rows of a stream, a row longer than N): the pending samples are decimated int16 whatever route
    they came by, and every tick equals the reference pump fed int16 (the wide rows decimated, the G.711 rows expanded)."""
    from silero_vad_amd import g711_expand
    pcm = golden["16k"]["pcm_i16"]
    cap = CAP
    rng = np.random.default_rng(37)
    src = [np.roll(pcm, -(30 * N + s * 7919)) for s in range(cap)]
    at = [0] * cap

    def take(s, n):
        at[s] += n
        return np.ascontiguousarray(src[s][at[s] - n:at[s]])

    pair = Pair(model, parts=3, ring_slots=2, max_burst=2)
    for t in range(24):
        who = [int(s) for s in rng.permutation(cap) if rng.random() < 0.85]
        if t % 4 == 0:                                         # wide: the stream's 48 kHz audio is its fixture, held
            pair.wide(0, [(s, widen(take(s, 200), 3, True)[:int(rng.integers(1, 601))], 3) for s in who])
        elif t % 4 == 1:
            pk = [(s, take(s, int(rng.integers(1, N + 1)))) for s in who]
            pair.both(lambda q: q.write_packets(1, pk))
        elif t % 4 == 2:
            pk = [(s, rng.integers(0, 256, int(rng.integers(1, N + 1))).astype(np.uint8), "ulaw") if s % 2 else
                  (s, take(s, int(rng.integers(1, N + 1))), "s16") for s in who]
            pair.got.write_coded_packets(0, pk)
            pair.ref.write_packets(0, [(s, g711_expand(x, c)) for s, x, c in pk])
        else:
            pk, spare = [], cap - len(who)                      # (a burst tick holds at most `streams` rows: `spare` second rows)
            for s in who:
                room = 3 * N - 1 - pair.got.pending(s)         # (at most max_burst = 2 chunks complete)
                assert room >= 2 * N
                if s % 4 == 0:
                    pk.append((s, take(s, int(rng.integers(N, N + 200)))))
                else:
                    rows = 2 if spare > 0 else 1
                    spare -= rows - 1
                    pk += [(s, take(s, int(rng.integers(1, 200)))) for _ in range(rows)]
            assert len(pk) <= cap and len(pk) > len(who)
            pair.both(lambda q: q.write_burst(1, pk))
        (ev, r), (ev_ref, r_ref) = pair.got.poll(), pair.ref.poll()
        assert r == r_ref and ev == ev_ref
        assert np.array_equal(pair.got.burst_probs(r), pair.ref.burst_probs(r))
        pair.stepped += int((pair.got.burst_probs(r) >= 0).sum())
    assert pair.stepped > 6 * cap and len({pair.got.wide_phase(s) for s in range(cap)}) == 3
    pair.finish()
    pair.close()


def test_refusals_queue_nothing(model, golden):
    """Every refusal of vad_pump_submit_wide_packets is VAD_ERR_ARG with nothing queued; phases and pending counts stay, and the next
    tick still equals the reference.  vad_pump_set_wideband refuses max_step 1 and 4, an 8 kHz pump (VAD_ERR_SAMPLE_RATE) and a call
    with a tick in flight; a pump without wideband refuses the route."""
    from silero_vad_amd import StreamPump, _lib
    pcm = golden["16k"]["pcm_i16"][40 * N:]
    pair = Pair(model, parts=1, ring_slots=2)
    pump = pair.got
    pair.wide(0, [(2, pcm[:100], 3), (5, pcm[100:201], 2)])
    pair.retire()
    before = ([pump.pending(s) for s in range(CAP)], [pump.wide_phase(s) for s in range(CAP)])
    assert before[0][2] == 34 and before[0][5] == 51 and before[1][2] == 1 and before[1][5] == 1
    many = list(range(CAP)) + [0]
    for streams, lengths, steps, offsets in (
            ([0], [8], [0], [0]), ([0], [8], [4], [0]), ([0], [8], [255], [0]),                     # a step of 0, above max_step
            ([CAP], [8], [3], [0]), ([-1], [8], [3], [0]), ([1, 1], [8, 8], [3, 2], [0, 16]),       # out of range, listed twice
            ([0, 3, 0], [8, 8, 8], [1, 2, 3], [0, 16, 32]),
            ([0], [0], [3], [0]), ([0], [3 * N + 1], [3], [0]), ([0], [2 * N + 1], [2], [0]), ([0], [N + 1], [1], [0]),
            ([0], [8], [3], [8]), ([0], [8], [3], [-16]),                                           # misaligned, in front of the area
            ([0], [9], [3], [AREA - 16]), ([0], [8], [3], [AREA]),                                  # runs past the area
            ([2, 0], [8, 3 * N + 1], [3, 3], [0, 16]),                                              # a good row in front of a bad one
            (many, [8] * len(many), [3] * len(many), [16 * i for i in range(len(many))])):          # more rows than streams
        with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
            pump.submit_wide_packets(1, streams, lengths, steps, offsets)
        assert pump.poll() == (None, None)
        assert ([pump.pending(s) for s in range(CAP)], [pump.wide_phase(s) for s in range(CAP)]) == before
    for bad in (lambda: pump.submit_wide_packets(1, [0, 1], [8, 8], [3]), lambda: pump.submit_wide_packets(1, [0], [8], [3], [0, 16]),
                lambda: pump.submit_wide_packets(1, [0], [8], [300]), lambda: pump.submit_wide_packets(1, [0], [8.0], [3])):
        with pytest.raises(ValueError):
            bad()
    assert pump.poll() == (None, None)
    # set_wideband: a bad max_step; the same one again is a no-op; refused with a tick in flight
    for m in (1, 0, 4, -3):
        with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
            pump.set_wideband(m)
    pump.set_wideband(MAX_STEP)
    assert ([pump.pending(s) for s in range(CAP)], [pump.wide_phase(s) for s in range(CAP)]) == before
    # the next tick: stream 2 at phase 1, stream 5 at phase 1, stream 7 new
    pair.wide(1, [(5, pcm[201:300], 2), (7, pcm[300:1836], 3), (2, pcm[1836:1836 + 3 * N - 1], 3)])
    with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
        pump.set_wideband(2)
    p, _ = pair.retire()
    assert p[7] >= 0 and p[2] >= 0 and p[5] == -1.0 and pump.pending(2) == 33 and pump.pending(5) == 100
    pair.finish()
    # a pump on which the enabling call was never made, and an 8 kHz pump
    plain = pair.ref
    assert plain._L.vad_pump_wide_slot(plain._h, 0) is None and plain._L.vad_pump_wide_phase(plain._h, 0) < 0
    with pytest.raises(ValueError):
        plain.wide_slot(0)
    with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
        plain.submit_wide_packets(0, [0], [8], [1], [0])
    assert plain.poll() == (None, None) and plain.pending(0) == 0
    pair.close()
    narrow = StreamPump(model.engine, 8000, streams=16)
    with pytest.raises(_lib.VadError, match="VAD_ERR_SAMPLE_RATE"):
        narrow.set_wideband(2)
    narrow.close()


def test_max_step_2_and_reallocation(model, golden):
    """A 32 kHz pump (max_step = 2): its area is streams * N * 2 * 2 bytes, step 3 is refused; set_wideband(3) then reallocates, zeroes
    the phases and keeps the pending samples (they are 16 kHz samples), and the pump goes on equal to the reference."""
    from silero_vad_amd import _lib
    pcm = golden["16k"]["pcm_i16"][50 * N:]
    pair = Pair(model, cap=20, max_step=2, parts=1, ring_slots=2)
    pump = pair.got
    assert len(pump.wide_slot(0)) == 20 * N * 2 * 2
    with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
        pump.submit_wide_packets(0, [0], [8], [3])
    pair.wide(0, [(0, pcm[:2 * N], 2), (19, pcm[2 * N:2 * N + 641], 2), (3, pcm[3000:3100], 1)], offsets=[20 * N * 4 - 4 * N, 0, 1296])
    p, _ = pair.retire()
    assert p[0] >= 0 and pump.pending(19) == 321 and pump.wide_phase(19) == 1
    pump.set_wideband(3)
    pair.step, pair.phase = [0] * 20, [0] * 20
    assert len(pump.wide_slot(1)) == 20 * N * 3 * 2 and pump.wide_phase(19) == 0 and pump.pending(19) == 321
    pair.wide(1, [(19, pcm[4000:4000 + 3 * N], 3), (0, pcm[6000:6007], 2)])
    p, _ = pair.retire()
    assert p[19] >= 0 and pump.pending(19) == 321 and pump.pending(0) == 4
    pair.finish()
    pair.close()


def test_a_pump_without_wideband_runs_as_before(model, golden):
    """The plain packet route on two pumps that never enabled wideband and on one that did: the same probabilities, events, pending
    counts and states, bit for bit -- enabling allocates beside the other routes and changes none of them."""
    from silero_vad_amd import StreamPump
    pcm = golden["16k"]["pcm_i16"]
    rng = np.random.default_rng(41)
    pumps = [StreamPump(model.engine, SR, streams=CAP, parts=3, ring_slots=2) for _ in range(3)]
    pumps[2].set_wideband(3)
    assert all(p._L.vad_pump_wide_slot(p._h, 0) is None for p in pumps[:2])
    src = [np.roll(pcm, -(30 * N + s * 7919)) for s in range(CAP)]
    at = np.zeros(CAP, np.int64)
    for t in range(20):
        pk = []
        for s in rng.permutation(CAP):
            if rng.random() < 0.9:
                ln = int(rng.choice([160, 320, 480])) if rng.random() < 0.7 else int(rng.integers(1, N + 1))
                pk.append((int(s), src[s][at[s]:at[s] + ln]))
                at[s] += ln
        out = []
        for p in pumps:
            p.write_packets(t % 2, pk)
            ev, r = p.poll()
            out.append((ev, r, p.probs(r).copy()))
        for ev, r, probs in out[1:]:
            assert ev == out[0][0] and r == out[0][1] and np.array_equal(probs, out[0][2])
    for s in range(CAP):
        assert pumps[0].pending(s) == pumps[1].pending(s) == pumps[2].pending(s) == at[s] % N
        st = [p.state(s) for p in pumps]
        for other in st[1:]:
            for x, y in zip(st[0], other):
                assert np.array_equal(x, y), s
    for p in pumps:
        p.close()
