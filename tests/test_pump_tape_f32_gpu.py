"""The pump's fp32 tape (vad_pump_set_tape_f32 / vad_pump_fetch_audio_f32 / vad_pump_tape_format, csrc/pump.hip + kernel_tape.hip): every
live stream's recent audio kept on the device as the float32 the net read, on every route -- the resampled one included, which has no
other tape.  Expected contents, compared as uint32 views, bit for bit, no tolerance anywhere:
    a resampled stream   ref.y[s] = resample_device of the stream's whole audio (`Ref` of tests/test_pump_resample_gpu.py), the fp32
                         sequence the pump steps
    every int16 route    fed[b].astype(float32) / 32768 of what the stream was fed after expansion / decimation (`Rig` of
                         tests/test_pump_tape_gpu.py), which is load_pcm's value and exact
Small pumps: at most 48 streams and about 120 ticks a test.
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import ctypes

import numpy as np
import pytest
import torch

import test_pump_tape_gpu as tape_gpu
from test_pump_resample_gpu import RATES, Ref, frames, speech  # noqa: F401  (speech: a fixture)
from test_pump_tape_gpu import FAR, PARTS, Rig, S, TAPE, model, packet_len  # noqa: F401  (model: a fixture)

pytestmark = pytest.mark.gpu

SENTINEL = 0xFFC0DE57                                            # a NaN's bits: no sample of any tape has them


def bits(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool((a == b).all())


def sentinel(size, device):
    raw = np.full(size, SENTINEL, np.uint32).view(np.float32)
    if not device:
        return raw
    out = torch.from_numpy(raw.copy()).to("cuda:0")
    torch.cuda.synchronize()
    return out


def loud(rng, n):
    """int16 over the whole range, both ends of it in every row of two samples or more"""
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    if n >= 2:
        x[0], x[-1] = -32768, 32767
    return x


class F32Rig(Rig):
    """`Rig` with an fp32 tape: what a stream was fed, as the net read it."""

    def __init__(self, model, sr, tape=TAPE, streams=S, **kw):
        super().__init__(model, sr, tape=tape, streams=streams, tape_dtype="float32", **kw)
        assert self.pump.tape_dtype == np.dtype("float32") and self.pump._L.vad_pump_tape_format(self.pump._h) == 4

    def samples(self, b, first, count):
        return super().samples(b, first, count).astype(np.float32) / np.float32(32768)

    def check(self):
        from silero_vad_amd import tape_window
        p = self.pump
        want = [tape_window(self.count(b), self.floor[b], self.tape, self.n, -FAR, FAR) for b in range(self.streams)]
        for b in range(self.streams):
            assert p.tape_state(b) == (self.count(b), self.floor[b]), b
        audios, first = p.fetch_audio(np.arange(self.streams), [-FAR] * self.streams, [FAR] * self.streams)
        for b in range(self.streams):
            assert audios[b].dtype == np.float32 and (int(first[b]), len(audios[b])) == want[b], b
            assert same_bits(audios[b], self.samples(b, *want[b])), b


class Taped:
    """The tape of a `Ref`'s pump against ref.y, stream by stream."""

    def __init__(self, ref):
        self.ref, self.y = ref, {}

    def expected(self, s, first, n):
        ref = self.ref
        if ref.y[s] is None:
            return np.zeros(0, np.float32)
        if self.y.get(s, (None,))[0] is not ref.y[s]:
            self.y[s] = (ref.y[s], ref.y[s].cpu().numpy())
        return self.y[s][1][first:first + n]

    def check(self, floor=None):
        from silero_vad_amd import tape_window
        ref, p = self.ref, self.ref.pump
        cap, floor = ref.cap, floor or {}
        for s in range(cap):
            assert p.tape_state(s) == (ref.done[s], floor.get(s, 0)), s
        audios, first = p.fetch_audio(np.arange(cap), [-FAR] * cap, [FAR] * cap)
        held = 0
        for s in range(cap):
            want = tape_window(ref.done[s], floor.get(s, 0), p.tape_chunks, ref.N, -FAR, FAR)
            assert audios[s].dtype == np.float32 and (int(first[s]), len(audios[s])) == want, s
            assert same_bits(audios[s], self.expected(s, *want)), s
            held += want[1]
        return held


def give_audio(ref, speech, rng, part):
    """every stream its rate (round robin) and `part` of the fixture speech, rolled"""
    for s in range(ref.cap):
        rate = ref.rates[s % len(ref.rates)]
        x = speech(rate, ref.sr)
        ref.audio(s, rate, np.ascontiguousarray(np.roll(x, -s * 977)[:int(len(x) * part) - int(rng.integers(0, 500))]))


def random_ticks(ref, rng, ticks=None, every=0, check=None):
    """`Ref`'s random ticks: 10 / 20 / 30 ms frames and uniform lengths in random arrival order, ~10 % of deliveries missed, every 11th
    tick empty, two ticks in flight; until the audio ends or `ticks` were made.  -> the ticks made."""
    slots, t = ref.pump.ring_slots, 0
    while any(ref.g[s] < len(ref.x[s]) for s in range(ref.cap)) and (ticks is None or t < ticks):
        rows = []
        if t % 11 != 10:
            for s in rng.permutation(ref.cap):
                if ref.g[s] < len(ref.x[s]) and rng.random() >= 0.1:
                    rows.append((int(s), frames(ref, s, rng)))
        before = [ref.done[s] for s in range(ref.cap)]
        ref.tick(t % slots, rows)
        if t > 0:
            ref.retire()
        if check is not None and every and t % every == every - 1:
            absent = [s for s in range(ref.cap) if ref.done[s] == before[s]]
            assert absent                                        # (streams this tick did not step: their counters stand still)
            check.check()
        t += 1
    ref.retire()
    return t


@pytest.mark.parametrize("sr,rates,cap", [(16000, RATES, 48), (8000, (44100, 16000), 32)])
def test_the_resampled_route_fills_the_tape(model, speech, sr, rates, cap):
    """Three / two rates side by side, 3 / 2 parts, a tape of 3 chunks, two ticks in flight: after every fifth tick and at the end every
    stream's counters are (chunks completed, 0) and its whole window is ref.y's bits; a stream absent from a tick keeps both."""
    rng = np.random.default_rng(71)
    ref = Ref(model, rates, sr=sr, cap=cap, parts=len(rates), ring_slots=3, tape_chunks=3, tape_dtype="float32")
    assert ref.pump.tape_dtype == np.dtype("float32") and ref.pump.resample_rates == tuple(rates)
    give_audio(ref, speech, rng, 0.4 if sr == 16000 else 0.25)
    taped = Taped(ref)
    t = random_ticks(ref, rng, every=5, check=taped)
    assert 20 <= t <= 125
    ref.finish()
    assert taped.check() == cap * 3 * ref.N and min(ref.done) > 2 * 3         # every ring full, and wrapped twice
    ref.close()


def run_pair(model, speech, ticks=40):
    """the same resampled ticks into a pump with the fp32 tape and into one without a tape"""
    out = []
    for kw in ({"tape_chunks": 3, "tape_dtype": "float32"}, {}):
        rng = np.random.default_rng(73)
        ref = Ref(model, RATES, cap=19, parts=2, ring_slots=3, **kw)
        give_audio(ref, speech, rng, 0.4)
        assert random_ticks(ref, rng, ticks=ticks) == ticks
        out.append(ref)
    return out


def test_the_tape_changes_no_result(model, speech):
    """Probabilities, events, pending counts, resample_state and the final (h, c, context) of the two pumps: each equals `Ref`'s restated
    reference bit for bit (its own checks), and so each other -- compared here once more, directly."""
    a, b = run_pair(model, speech)
    assert a.pump.tape_dtype == np.dtype("float32") and b.pump.tape_dtype is None and b.pump.tape_chunks == 0
    assert a.probs == b.probs and a.events == b.events > 0 and a.stepped == b.stepped > 5 * 19
    a.finish()
    b.finish()
    for s in range(19):
        assert a.pump.pending(s) == b.pump.pending(s) and a.pump.resample_state(s) == b.pump.resample_state(s), s
        for x, y in zip(a.pump.state(s), b.pump.state(s)):
            assert same_bits(x, y), s
    Taped(a).check()
    a.close()
    b.close()


def chunk_ticks(rig, rng):
    for t, route in enumerate(("full", "masked", "compact", "rows") * 3):
        rig.chunks(route, rng)
        if t % 4 == 3:
            rig.check()


def packet_ticks(rig, rng, coded):
    from silero_vad_amd import g711_expand
    laws = set()
    for t in range(12):
        r, pk = rig.slot(), []
        quiet = int(rng.integers(0, S))
        for b in rng.permutation(S):
            b = int(b)
            ln = packet_len(rng, rig.n, rig.pump.sr)
            if b == quiet:
                pk.append((b, ln, "ulaw") if coded else (b, ln))
                rig.feed(b, np.zeros(ln, np.int16))
            elif rng.random() >= 0.3:
                law = ("s16", "ulaw", "alaw")[(b + t) % 3] if coded else "s16"
                laws.add(law)
                x = loud(rng, ln) if law == "s16" else rng.integers(0, 256, ln).astype(np.uint8)
                pk.append((b, x, law) if coded else (b, x))
                rig.feed(b, g711_expand(x, law))
        if coded:
            rig.pump.write_coded_packets(r, pk)
        else:
            rig.pump.write_packets(r, pk)
        rig.t += 1
        if t % 4 == 3:
            rig.check()
    assert laws == ({"s16", "ulaw", "alaw"} if coded else {"s16"})


def burst_ticks(rig, rng):
    """stream 0 completes exactly 3 chunks in every tick (3 sub-steps), stream 1 dribbles, stream 2 sends more than a chunk"""
    from silero_vad_amd import g711_expand
    n, steps = rig.n, set()
    for t in range(8):
        r, pk = rig.slot(), []

        def add(b, x, law="s16"):
            pk.append((b, x, law))
            rig.feed(b, np.zeros(x, np.int16) if isinstance(x, int) else g711_expand(x, law))

        before = rig.count(0)
        add(0, loud(rng, 3 * n - len(rig.fed[0]) % n + int(rng.integers(0, n - len(rig.fed[0]) % n))))
        add(1, loud(rng, 7))
        add(2, loud(rng, n + 100))
        for b in range(3, 9):
            room = 4 * n - 1 - len(rig.fed[b]) % n
            if b == 3 + t % 6:
                add(b, int(rng.integers(n + 1, room)))           # silent, longer than a chunk
            elif rng.random() >= 0.3:
                add(b, rng.integers(0, 256, int(rng.integers(1, room // 2))).astype(np.uint8), ("ulaw", "alaw")[b % 2])
                add(b, loud(rng, int(rng.integers(1, room // 2))))
        rig.pump.write_burst(r, pk)
        rig.t += 1
        steps.add(rig.count(0) - before)
        assert rig.pump.burst_steps(r) >= 3
        if t % 3 == 2:
            rig.check()
    assert steps == {3}


def wide_ticks(rig, rng):
    """48 and 32 kHz rows beside 16 kHz ones, zero-stuffed so that the comb phase matters, a silent row in every tick"""
    from silero_vad_amd import ROW_SILENT, decimate
    rig.pump.set_wideband(3)
    n, phase = rig.n, [0] * S
    for t in range(10):
        r = rig.slot()
        area = rig.pump.wide_slot(r)
        st, ln, sp, off, at = [], [], [], [], 0
        quiet = int(rng.integers(0, S))
        for b in rng.permutation(S):
            b = int(b)
            step = 3 - b % 3
            if b != quiet and rng.random() < 0.3:
                continue
            length = int(rng.integers(1, step * n + 1)) if rng.random() < 0.5 else step * int(rng.choice([160, 320, 480]))
            x = np.full(length, -77, np.int16)
            first = (-phase[b]) % step
            x[first::step] = loud(rng, len(x[first::step]))
            if b == quiet:
                x[:] = 0
                off.append(ROW_SILENT)
            else:
                area[at:at + 2 * length] = x.view(np.uint8)
                off.append(at)
                at += (2 * length + 15) // 16 * 16
            rig.feed(b, decimate(x, step, phase[b]))
            phase[b] = (phase[b] + length) % step
            st.append(b), ln.append(length), sp.append(step)
        assert 3 in sp
        rig.pump.submit_wide_packets(r, st, ln, sp, off)
        rig.t += 1
        if t % 3 == 2:
            rig.check()


@pytest.mark.parametrize("sr,route", [(sr, route) for sr in (16000, 8000) for route in ("chunks", "packets", "coded", "burst")] + [(16000, "wide")])
def test_int16_routes_on_an_fp32_tape(model, monkeypatch, sr, route):
    """Full, masked, compact and rows ticks; int16 packets; mu-law and A-law packets beside int16 ones; burst ticks of 3 sub-steps; wide
    ticks with 48 kHz rows (a 16 kHz pump only: an 8 kHz pump takes no wide rows): the tape is x / 32768 of what was fed, -32768 and 32767
    among it."""
    monkeypatch.setattr(tape_gpu, "noise", loud)                 # (what `Rig.chunks` draws its rows with)
    rig = F32Rig(model, sr, **({"max_burst": 3} if route == "burst" else {}))
    rng = np.random.default_rng(79)
    if route == "chunks":
        chunk_ticks(rig, rng)
    elif route == "burst":
        burst_ticks(rig, rng)
    elif route == "wide":
        wide_ticks(rig, rng)
    else:
        packet_ticks(rig, rng, route == "coded")
    rig.drain()
    rig.check()
    every = np.concatenate(rig.fed)
    assert every.min() == -32768 and every.max() == 32767
    assert max(rig.count(b) for b in range(S)) > TAPE            # the ring has wrapped
    rig.close()


def test_one_pump_both_kinds(model, speech):
    """Streams bound to 44.1 and 24 kHz beside unbound streams fed int16 packets, resampled ticks and packet ticks in turn: one tape
    holds both, every stream's window is exact."""
    from silero_vad_amd import tape_window
    rng = np.random.default_rng(83)
    cap, K = 24, 4
    ref = Ref(model, (44100, 24000), cap=cap, parts=2, ring_slots=2, tape_chunks=K, tape_dtype="float32")
    unbound = [s for s in range(cap) if s % 3 == 2]
    bound = [s for s in range(cap) if s % 3 != 2]
    for s in bound:
        rate = (44100, 24000)[s % 3]
        x = speech(rate)
        ref.audio(s, rate, np.ascontiguousarray(np.roll(x, -s * 977)[:len(x) // 3]))
    taped = Taped(ref)
    fed = {b: np.zeros(0, np.int16) for b in unbound}

    def check():
        for b in unbound:
            assert ref.done[b] == 0
            ref.done[b] = len(fed[b]) // ref.N                   # (the clock of an unbound stream: the chunks its packets completed)
        try:
            taped.check()
        finally:
            for b in unbound:
                ref.done[b] = 0

    taped.expected_bound = taped.expected
    taped.expected = lambda s, first, n: (fed[s].astype(np.float32) / np.float32(32768))[first:first + n] if s in fed else taped.expected_bound(s, first, n)
    for t in range(60):
        if t % 2 == 0:
            rows = [(int(s), frames(ref, s, rng)) for s in rng.permutation(bound) if ref.g[s] < len(ref.x[s]) and rng.random() >= 0.1]
            ref.tick(t % 2, rows)
            ref.retire()
        else:
            pk = []
            for b in rng.permutation(unbound):
                if rng.random() >= 0.2:
                    x = loud(rng, packet_len(rng, ref.N, 16000))
                    pk.append((int(b), x))
                    fed[int(b)] = np.concatenate([fed[int(b)], x])
            ref.pump.write_packets(t % 2, pk)
            ev, r = ref.pump.poll()
            assert r == t % 2 and all(b in unbound for b, _ in ev)
            probs = ref.pump.probs(r)
            assert (probs[bound] == -1.0).all()                  # (a packet tick steps no bound stream)
        if t % 6 == 5:
            check()
    check()
    assert min(ref.done[s] for s in bound) > K and min(len(fed[b]) // ref.N for b in unbound) > K
    for s in range(cap):
        assert ref.pump.resample_state(s)[0] == (0 if s in fed else ref.rate[s])
    assert tape_window(ref.done[0], 0, K, ref.N, -FAR, FAR)[1] == K * ref.N
    ref.close()


def fetch_checked(rig, streams, starts, ends, offsets_of, device):
    """One fetch of the requests into a sentinel-filled buffer, at the offsets offsets_of(counts) gives: first / count are the rule's,
    the bits are fed's, everything else is still the sentinel.  -> the buffer's bits."""
    from silero_vad_amd import tape_window
    p = rig.pump
    first, count = p.tape_windows(streams, starts, ends)
    for i, b in enumerate(streams):
        assert (int(first[i]), int(count[i])) == tape_window(rig.count(b), rig.floor[b], rig.tape, rig.n, starts[i], ends[i]), i
    offsets = offsets_of(count)
    size = int(max([0] + [o + c for o, c in zip(offsets, count)])) + 40
    out = sentinel(size, device)
    p.fetch_audio_into(streams, first, count, out, offsets)
    got = bits(out)
    want = np.full(size, SENTINEL, np.uint32)
    for i, b in enumerate(streams):
        want[offsets[i]:offsets[i] + count[i]] = bits(rig.samples(b, int(first[i]), int(count[i])))
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    return got, first, count


def offsets_off(k):
    """every request on a multiple of 4 floats (16 bytes), plus k"""
    def of(count):
        off = np.zeros(len(count), np.int64)
        if len(count):
            off[1:] = np.cumsum((np.asarray(count)[:-1] + 3 + k) // 4 * 4)
        return off + k
    return of


@pytest.mark.parametrize("sr", [16000, 8000])
def test_gather_corners(model, sr):
    """A tape of 9 chunks (4608 / 2304 floats: more than one 2048-float tile), wrapped twice and more: requests at every source
    misalignment, across the wrap, of 1 / 3 / 4 / 5 / 2047 / 2048 / 2049 floats and of none, one stream in many requests, to host and
    device destinations at aligned offsets and 1, 2 and 3 floats off; nothing outside the requested runs is written."""
    K = 9
    rig = F32Rig(model, sr, tape=K)
    rng = np.random.default_rng(89)
    for _ in range(2 * K + 2):
        rig.chunks("full", rng)
    rig.chunks("masked", rng, present=np.arange(S) % 2 == 0)     # (the streams' wrap points differ from here on)
    rig.chunks("masked", rng, present=(np.arange(S) % 4 == 0) | (np.arange(S) == 18))
    rig.drain()
    n = rig.n
    assert (rig.count(4), rig.count(5), rig.count(18)) == (2 * K + 4, 2 * K + 2, 2 * K + 4) and 9 * n > 2049 + 70
    req = []
    for b in (4, 5, 18):
        lo, hi = (rig.count(b) - K) * n, rig.count(b) * n
        wrap = ((rig.count(b) - 1) // K) * K * n                 # chunk k * K lies in slot 0: the ring's end is in front of it
        assert lo < wrap < hi and wrap >= 2 * K * n              # (the ring has wrapped twice)
        req += [(b, wrap - 100, wrap + 100), (b, wrap - 3, wrap + 5), (b, wrap - 4, wrap + 4), (b, wrap - 1, wrap + 1), (b, wrap - 2, wrap + 1),
                (b, wrap - 1, wrap + 3), (b, lo, hi), (b, -FAR, FAR), (b, lo + 1, hi - 1),                      # across the wrap
                (b, 0, lo + 10), (b, lo - 1, lo + 64), (b, hi - 10, hi + n), (b, hi, hi + 5),                    # clamped
                (b, lo + 17, lo + 17), (b, 5, 5), (b, hi + 9, hi + 9)]                                           # empty
        for k in range(4):                                       # every source misalignment inside a 16-byte granule
            assert (lo + 64 + k) % 4 == k
            req += [(b, lo + 64 + k, lo + 64 + k + c) for c in (1, 3, 4, 5, 2047, 2048, 2049)]
    streams, starts, ends = [q[0] for q in req], [q[1] for q in req], [q[2] for q in req]
    host, first, count = fetch_checked(rig, streams, starts, ends, offsets_off(0), device=False)
    assert any(f > s for f, s in zip(first, starts)) and any(c == 0 for c in count) and int(count.max()) == K * n
    assert {1, 3, 4, 5, 2047, 2048, 2049} <= set(count.tolist())
    dev, _, _ = fetch_checked(rig, streams, starts, ends, offsets_off(0), device=True)
    assert np.array_equal(host, dev)
    for k in (1, 2, 3):                                          # destinations off the 16-byte grid: element by element
        fetch_checked(rig, streams, starts, ends, offsets_off(k), device=True)
        fetch_checked(rig, streams, starts, ends, offsets_off(k), device=False)
    fetch_checked(rig, [], [], [], offsets_off(0), device=False)                # n = 0
    fetch_checked(rig, [], [], [], offsets_off(0), device=True)
    # fetch_audio: the same through the public call, host and device
    audios, f1 = rig.pump.fetch_audio(streams, starts, ends)
    (packed, offsets, counts), f2 = rig.pump.fetch_audio(streams, starts, ends, device=True)
    assert packed.device.type == "cuda" and packed.dtype == torch.float32 and np.array_equal(f1, first) and np.array_equal(f2, first)
    packed = packed.cpu().numpy()
    for i, b in enumerate(streams):
        assert audios[i].dtype == np.float32 and same_bits(audios[i], rig.samples(b, int(first[i]), int(count[i]))), i
        assert offsets[i] % 8 == 0 and same_bits(packed[offsets[i]:offsets[i] + counts[i]], audios[i]), i
    rig.check()
    rig.close()


def test_a_stale_range_is_refused_and_nothing_is_written(model):
    from silero_vad_amd._lib import VadError
    rig = F32Rig(model, 16000)
    rng = np.random.default_rng(97)
    for _ in range(4):
        rig.chunks("full", rng)
    first, count = rig.pump.tape_windows([2, 9], [-FAR, 600], [FAR, 700])
    assert count.tolist() == [TAPE * rig.n, 100]
    rig.chunks("full", rng)                                      # the intervening tick: still in flight when the fetch is made
    for device in (False, True):
        out = sentinel(4 * TAPE * rig.n, device)
        with pytest.raises(VadError, match="no longer held"):
            rig.pump.fetch_audio_into([2, 9], first, count, out, [0, TAPE * rig.n])
        assert (bits(out) == SENTINEL).all()
    rig.drain()
    rig.check()                                                  # the next fetch is right
    rig.close()


def test_open_with_ticks_in_flight_restarts_a_bound_streams_clock_and_tape(model, speech):
    """Two resampled ticks in flight, then open_stream(3): the slot's earlier chunks do not count, the new stream binds to another rate
    and its window starts at sample 0 of ITS clock; a closed stream keeps its counters."""
    K = 6
    ref = Ref(model, (44100, 24000), cap=16, parts=1, ring_slots=3, tape_chunks=K, tape_dtype="float32")
    taped = Taped(ref)
    x44, x24 = speech(44100), speech(24000)
    ref.audio(3, 44100, x44[:5000])
    ref.audio(4, 44100, x44[2000:7000])
    ref.tick(0, [(3, 1416), (4, 1000)])
    ref.tick(1, [(3, 1300), (4, 1416)])                          # (two ticks in flight at the open)
    assert ref.done[3] == 1 and ref.done[4] == 1
    ref.open_stream(3)
    ref.pump.close_stream(4)
    ref.retire()
    ref.retire()
    assert ref.pump.tape_state(3) == (0, 0) and ref.pump.tape_state(4) == (1, 0)
    ref.audio(3, 24000, x24[:4000])
    for t in range(4):
        ref.tick(t % 3, [(3, 760)])
        ref.retire()
    assert ref.pump.resample_state(3)[0] == 24000 and 2 <= ref.done[3] <= K
    assert ref.pump.tape_state(3) == (ref.done[3], 0)
    audios, first = ref.pump.fetch_audio([3, 4], [-FAR, -FAR], [FAR, FAR])
    assert first.tolist() == [0, 0] and len(audios[0]) == ref.done[3] * 512 and len(audios[1]) == 512
    assert same_bits(audios[0], ref.y[3][:len(audios[0])]) and same_bits(audios[1], ref.y[4][:512])
    taped.check()
    ref.close()


def test_snapshots_ignore_the_tape_and_an_import_restarts_it(model, speech):
    """A version 2 export of a resampling pump with an fp32 tape is the export of an untaped one fed the same ticks; imported into another
    fp32-taped resampling pump (enabled in the other order: set_resample, then set_tape) every record's clock continues with nothing
    held, later chunks are fetchable and exact, a request reaching before the import comes back with first > start."""
    from silero_vad_amd import StreamPump, snapshot_info
    a, b = run_pair(model, speech, ticks=24)                     # (at most 0.72 s of every stream's 1 s)
    a.finish()
    blob = a.pump.export_streams(version=2)
    assert np.array_equal(blob, b.pump.export_streams(version=2))
    b.close()
    Taped(a).check()
    K, N = 3, 512
    dst = StreamPump(model.engine, 16000, streams=19, parts=2, ring_slots=2)
    dst.set_resample(RATES)
    dst.set_tape(K, "float32")
    assert dst.tape_dtype == np.dtype("float32") and dst._L.vad_pump_tape_format(dst._h) == 4
    info = snapshot_info(blob)
    src_of = {7: 2, 0: 18, 18: 11}
    dst.import_streams(blob, list(src_of), [src_of[s] for s in src_of])
    for s, r in src_of.items():
        k = info[r]["current_sample"] // N
        assert k == a.done[r] > 0 and dst.tape_state(s) == (k, k), s
        assert dst.resample_state(s) == a.pump.resample_state(r)
    assert dst.tape_state(1) == (0, 0)
    audios, first = dst.fetch_audio(list(src_of), [0] * 3, [FAR] * 3)
    assert [len(x) for x in audios] == [0, 0, 0] and first.tolist() == [a.done[r] * N for r in src_of.values()]
    for t in range(12):                                          # the streams go on in 10 ms frames of their remaining audio
        pk = []
        for s, r in src_of.items():
            n = min(a.rate[r] // 100, len(a.x[r]) - a.g[r])      # (160 outputs a row: never two chunks in a tick)
            if n > 0:
                pk.append((s, a.x[r][a.g[r]:a.g[r] + n], a.rate[r]))
                a.g[r] += n
        dst.write_resampled_packets(t % 2, pk)
        assert dst.poll()[1] == t % 2
    for s, r in src_of.items():
        k, now = info[r]["current_sample"] // N, a.ready(r) // N
        assert now >= k + 2 and dst.tape_state(s) == (now, k), s
        audios, first = dst.fetch_audio([s], [0], [FAR])
        lo = max(k, now - K) * N
        assert first[0] == lo > 0 and len(audios[0]) == now * N - lo > 0
        assert same_bits(audios[0], a.y[r][lo:now * N]), s
    dst.close()
    a.close()


def test_refusals_leave_the_pump_usable(model, monkeypatch):
    from silero_vad_amd import StreamPump
    from silero_vad_amd._lib import VadError
    rng = np.random.default_rng(101)
    f32 = np.dtype("float32")

    def fmt(p):
        return p._L.vad_pump_tape_format(p._h)

    # chunks < 2; after the first tick
    p = StreamPump(model.engine, 16000, streams=S, parts=PARTS)
    assert fmt(p) == 0 and p.tape_dtype is None
    with pytest.raises(VadError, match="at least 2"):
        p.set_tape(1, "float32")
    assert p._L.vad_pump_set_tape_f32(p._h, -3) == 1 and fmt(p) == 0 and p.tape_chunks == 0 and p.tape_dtype is None
    with pytest.raises(VadError, match="no tape"):
        p.fetch_audio_into([0], [0], [10], np.zeros(16, np.int16), [0])
    assert p._L.vad_pump_fetch_audio_f32(p._h, None, None, None, 0, None, None, 0) == 1 and "no tape" in p._L.vad_pump_last_error(p._h).decode()
    p.slot(0)[:] = loud(rng, S * p.n).reshape(S, p.n)
    p.submit(0)
    assert p.poll()[1] == 0
    with pytest.raises(VadError, match="first tick"):
        p.set_tape(4, "float32")
    p.submit(1)
    assert p.poll()[1] == 1 and fmt(p) == 0                      # still usable, still untaped
    p.close()
    # one tape a pump: either call after either tape
    for have in ("float32", "int16"):
        p = StreamPump(model.engine, 16000, streams=S, parts=PARTS, tape_chunks=4, tape_dtype=have)
        assert fmt(p) == np.dtype(have).itemsize and p.tape_dtype == np.dtype(have)
        for again in ("float32", "int16"):
            with pytest.raises(VadError, match="already"):
                p.set_tape(5, again)
        assert fmt(p) == np.dtype(have).itemsize and p.tape_dtype == np.dtype(have) and p.tape_chunks == 4
        p.close()
    # the wrong fetch for the tape: nothing written, and the next tick is bit-right
    monkeypatch.setattr(tape_gpu, "noise", loud)
    for rig, wrong, right, out in ((F32Rig(model, 16000), "vad_pump_fetch_audio", "vad_pump_fetch_audio_f32", np.full(64, -23131, np.int16)),
                                   (Rig(model, 16000), "vad_pump_fetch_audio_f32", "vad_pump_fetch_audio", sentinel(64, False))):
        rig.chunks("full", rng)
        rig.drain()
        L, h = rig.pump._L, rig.pump._h
        st, fi, ct, of = np.array([3], np.int32), np.array([100], np.int64), np.array([40], np.int64), np.array([8], np.int64)
        before = out.copy()
        rc = getattr(L, wrong)(h, st.ctypes.data, fi.ctypes.data, ct.ctypes.data, 1, of.ctypes.data, out.ctypes.data, 0)
        msg = L.vad_pump_last_error(h).decode()
        assert rc == 1 and msg.endswith("fetch it with " + right), msg
        assert out.tobytes() == before.tobytes()
        with pytest.raises(ValueError, match="out must be"):     # (the Python layer refuses the wrong dtype before the call)
            rig.pump.fetch_audio_into([3], [100], [40], out, [8])
        wrong_dev = torch.zeros(64, dtype=torch.int16 if rig.pump.tape_dtype == f32 else torch.float32, device="cuda:0")
        with pytest.raises(ValueError, match="out must be"):
            rig.pump.fetch_audio_into([3], [100], [40], wrong_dev, [8])
        rig.chunks("masked", rng)
        rig.drain()
        rig.check()
        rig.close()
    # set_resample on an fp32-taped pump, with chunks already on the tape: it and a second call with other rates leave tape and clocks alone
    rig = F32Rig(model, 16000)
    for _ in range(4):
        rig.chunks("full", rng)
    rig.drain()
    rig.pump.set_resample((44100,))
    rig.check()
    rig.pump.set_resample((24000, 22050))
    assert fmt(rig.pump) == 4 and rig.pump.resample_rates == (24000, 22050)
    rig.check()
    rig.chunks("rows", rng)
    rig.drain()
    rig.check()
    rig.close()
    # the int16 tape and the resampled route still refuse each other (tests/test_pump_tape_gpu.py pins the messages)
    p = StreamPump(model.engine, 16000, streams=S, parts=PARTS, tape_chunks=4)
    with pytest.raises(VadError, match="does not hold the resampled route's fp32 chunks"):
        p.set_resample((44100,))
    p.close()


def test_utterances_end_to_end(model, speech):
    """The fixture speech at 44.1 kHz, then silence, as 30 ms packets on three streams at different offsets into it: every utterance the
    collector returns is float32 and ref.y[s][start:end] bit for bit, with first == start (the tape holds the longest of them)."""
    from silero_vad_amd import UtteranceCollector
    x44 = speech(44100)
    pkt, tail = 1323, 20 * 1323
    K = -(-(len(x44) + tail) * 16000 // 44100 // 512) + 4
    ref = Ref(model, (44100,), cap=16, parts=2, ring_slots=2, tape_chunks=K, tape_dtype="float32")
    collector = UtteranceCollector(ref.pump)
    on = (1, 8, 15)
    for i, s in enumerate(on):
        ref.audio(s, 44100, np.concatenate([np.roll(x44, -i * 30000), np.zeros(tail, np.int16)]))
    utterances, t = [], 0
    while any(ref.g[s] < len(ref.x[s]) for s in on):
        ref.tick(t % 2, [(s, min(pkt, len(ref.x[s]) - ref.g[s])) for s in on if ref.g[s] < len(ref.x[s])])
        events = ref.expect[0][1]                                # (`retire` asserts that the pump's events are these)
        ref.retire()
        utterances += collector.feed(events)
        t += 1
    assert t <= 125 and len(utterances) >= 1 and ref.events >= 2 * len(utterances)
    for s, start, end, first, audio in utterances:
        assert start is not None and first == start and audio.dtype == np.float32 and len(audio) == end - start > 0
        assert same_bits(audio, ref.y[s][start:end]), (s, start, end)
    ref.finish()
    ref.close()
