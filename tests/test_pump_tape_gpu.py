"""The pump's tape (vad_pump_set_tape / vad_pump_tape_window / vad_pump_fetch_audio, csrc/pump.hip + kernel_tape.hip): every live
stream's recent net-rate int16 audio kept on the device, fetched by sample range.  Expected audio is computed HERE from what was fed:
per stream the concatenation `fed[b]` of its net-rate samples in order (g711_expand for coded rows, decimate at the phase tracked here
for wide rows, zeros for silent rows, nothing for absent ticks).  After any number of ticks tape_state(b) == (len(fed[b]) // N, floor),
every fetch equals fed[b][first : first + count] bit for bit, and (first, count) equal tape_window(...).  No tolerance anywhere: this
is byte copying.  Shapes: 19 streams (one 16-stream tile + 3), 2 uneven parts, a tape of 3 chunks (no power of two, wraps within four
ticks), both sample rates.
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S, PARTS, TAPE = 19, 2, 3
FAR = 2 ** 62
SENTINEL = -23131


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


def noise(rng, n):
    return rng.integers(-9000, 9000, n).astype(np.int16)


class Rig:
    """A taped pump and what its streams were fed.  fed[b][i] is sample base[b] + i of stream b's clock."""

    def __init__(self, model, sr, tape=TAPE, streams=S, **kw):
        from silero_vad_amd import StreamPump
        self.pump = StreamPump(model.engine, sr, streams=streams, parts=PARTS, tape_chunks=tape, **kw)
        self.n, self.tape, self.streams = self.pump.n, tape, streams
        self.fed = [np.zeros(0, np.int16) for _ in range(streams)]
        self.base = [0] * streams
        self.floor = [0] * streams
        self.t = 0
        self.events = []

    def feed(self, b, x):
        self.fed[b] = np.concatenate([self.fed[b], np.asarray(x, np.int16)])

    def reopen(self, b):
        self.fed[b], self.base[b], self.floor[b] = np.zeros(0, np.int16), 0, 0

    def count(self, b):
        return (self.base[b] + len(self.fed[b])) // self.n

    def samples(self, b, first, count):
        return self.fed[b][first - self.base[b]:first - self.base[b] + count]

    def slot(self):
        """The next tick's ring slot; at most two ticks stay in flight."""
        while self.t - self.retired >= 2:
            self.poll()
        return self.t % self.pump.ring_slots

    retired = 0

    def poll(self):
        ev, r = self.pump.poll()
        assert r is not None
        self.events += ev
        self.retired += 1
        return ev

    def drain(self):
        while self.retired < self.t:
            self.poll()

    def check(self):
        """Counters, and the whole window of every stream in one fetch."""
        from silero_vad_amd import tape_window
        p = self.pump
        want = [tape_window(self.count(b), self.floor[b], self.tape, self.n, -FAR, FAR) for b in range(self.streams)]
        for b in range(self.streams):
            assert p.tape_state(b) == (self.count(b), self.floor[b]), b
        audios, first = p.fetch_audio(np.arange(self.streams), [-FAR] * self.streams, [FAR] * self.streams)
        for b in range(self.streams):
            assert (int(first[b]), len(audios[b])) == want[b], b
            assert np.array_equal(audios[b], self.samples(b, *want[b])), b

    # the chunk routes: every listed stream delivers one chunk
    def chunks(self, route, rng, present=None):
        p, n, r = self.pump, self.n, self.slot()
        if route == "full":
            present = np.ones(self.streams, bool)
        elif present is None:
            present = rng.random(self.streams) >= 0.3
        who = np.flatnonzero(present)
        rows = {int(b): noise(rng, n) for b in who}
        if route == "full":
            for b in who:
                p.slot(r)[b] = rows[b]
            p.submit(r)
        elif route == "masked":
            for b in who:
                p.slot(r)[b] = rows[b]
            p.submit(r, present)
        elif route == "compact":
            for i, b in enumerate(who):
                p.slot(r)[i] = rows[b]
            p.submit(r, present, compact=True)
        else:                                                    # rows: arrival order
            who = rng.permutation(who)
            for i, b in enumerate(who):
                p.slot(r)[i] = rows[int(b)]
            p.submit_rows(r, who)
        for b in who:
            self.feed(int(b), rows[int(b)])
        self.t += 1

    def close(self):
        self.pump.close()


def packet_len(rng, n, sr):
    ms10 = sr // 100
    return int(rng.choice([ms10, 2 * ms10, 3 * ms10])) if rng.random() < 0.6 else int(rng.integers(1, n + 1))


@pytest.mark.parametrize("sr", [16000, 8000])
def test_the_tape_changes_no_result(model, golden, sr):
    """Tape on and tape off, the same masked ticks of speech: probabilities, events and (h, c, context) equal bit for bit at every tick."""
    from silero_vad_amd import StreamPump
    pcm = golden["16k" if sr == 16000 else "8k"]["pcm_i16"]
    rig = Rig(model, sr)
    ref = StreamPump(model.engine, sr, streams=S, parts=PARTS)
    rng = np.random.default_rng(5)
    n, at, events = rig.n, [(b % 4) * 3 * rig.n for b in range(S)], 0
    for t in range(12):
        present = rng.random(S) >= 0.3
        for b in np.flatnonzero(present):
            row = pcm[at[b]:at[b] + n]
            rig.pump.slot(0)[b] = row
            ref.slot(0)[b] = row
            rig.feed(b, row)
            at[b] += n
        rig.pump.submit(0, present)
        ref.submit(0, present)
        (ev, _), (ev_ref, _) = rig.pump.poll(), ref.poll()
        assert ev == ev_ref, t
        events += len(ev)
        assert np.array_equal(rig.pump.probs(0), ref.probs(0)), t
        for b in range(S):
            for x, y in zip(rig.pump.state(b), ref.state(b)):
                assert np.array_equal(x, y), (t, b)
    assert events >= 1
    rig.check()
    rig.close()
    ref.close()


@pytest.mark.parametrize("sr,route", [(sr, route) for sr in (16000, 8000) for route in ("full", "masked", "compact", "rows")])
def test_every_chunk_route_fills_the_tape(model, sr, route):
    rig = Rig(model, sr)
    rng = np.random.default_rng(11)
    for t in range(12):
        rig.chunks(route, rng)
        if t % 3 == 2:
            rig.check()
    rig.drain()
    rig.check()
    assert max(rig.count(b) for b in range(S)) > TAPE            # the ring has wrapped
    rig.close()


@pytest.mark.parametrize("sr,coded", [(16000, False), (8000, False), (16000, True), (8000, True)])
def test_the_packet_routes_fill_the_tape(model, sr, coded):
    """int16 packets (10 / 20 / 30 ms and odd lengths) and coded packets (mu-law and A-law beside s16), ~30 % of the streams absent per
    tick, a silent row in every tick."""
    from silero_vad_amd import g711_expand
    rig = Rig(model, sr)
    rng = np.random.default_rng(13 + coded)
    laws = set()
    for t in range(14):
        r, pk = rig.slot(), []
        quiet = int(rng.integers(0, S))
        for b in rng.permutation(S):
            b = int(b)
            ln = packet_len(rng, rig.n, sr)
            if b == quiet:
                pk.append((b, ln, "ulaw") if coded else (b, ln))
                rig.feed(b, np.zeros(ln, np.int16))
            elif rng.random() >= 0.3:
                law = ("s16", "ulaw", "alaw")[(b + t) % 3] if coded else "s16"
                laws.add(law)
                x = noise(rng, ln) if law == "s16" else rng.integers(0, 256, ln).astype(np.uint8)
                pk.append((b, x, law) if coded else (b, x))
                rig.feed(b, g711_expand(x, law))
        if coded:
            rig.pump.write_coded_packets(r, pk)
        else:
            rig.pump.write_packets(r, pk)
        rig.t += 1
        if t % 3 == 2:
            rig.check()
    rig.drain()
    rig.check()
    assert laws == ({"s16", "ulaw", "alaw"} if coded else {"s16"})
    assert max(rig.count(b) for b in range(S)) > TAPE
    for b in range(S):
        assert rig.pump.pending(b) == len(rig.fed[b]) % rig.n
    rig.close()


@pytest.mark.parametrize("sr", [16000, 8000])
def test_burst_ticks_fill_the_tape(model, sr):
    """max_burst = 3: stream 0 completes exactly 3 chunks in a tick, stream 1 dribbles (0 chunks in most ticks), stream 2 sends packets
    longer than a chunk, a silent row longer than a chunk, G.711 rows beside int16, several rows of one stream in a tick."""
    from silero_vad_amd import g711_expand
    rig = Rig(model, sr, max_burst=3)
    n = rig.n
    rng = np.random.default_rng(17)
    done = {0: set(), 1: set(), 2: set()}
    for t in range(12):
        r, pk = rig.slot(), []

        def add(b, x, law="s16"):
            pk.append((b, x, law))
            rig.feed(b, np.zeros(x, np.int16) if isinstance(x, int) else g711_expand(x, law))

        before = [rig.count(b) for b in range(S)]
        add(0, noise(rng, 3 * n - len(rig.fed[0]) % n + int(rng.integers(0, n - len(rig.fed[0]) % n))))      # 3 chunks, whatever was pending
        add(1, noise(rng, 7))
        add(2, noise(rng, n + 100))
        for b in range(3, 9):                                    # (a tick holds at most `streams` rows)
            room = 4 * n - 1 - len(rig.fed[b]) % n
            if b == 3 + t % 6:
                add(b, int(rng.integers(n + 1, room)))           # silent, longer than a chunk
            elif rng.random() >= 0.3:
                a = int(rng.integers(1, room // 2))
                add(b, rng.integers(0, 256, a).astype(np.uint8), ("ulaw", "alaw")[b % 2])
                add(b, noise(rng, int(rng.integers(1, room // 2))))
        assert len(pk) <= S
        rig.pump.write_burst(r, pk)
        rig.t += 1
        for b in done:
            done[b].add(rig.count(b) - before[b])
        if t % 3 == 2:
            rig.check()
    rig.drain()
    rig.check()
    assert done[0] == {3} and 0 in done[1] and done[2] <= {1, 2}
    rig.close()


def test_wide_ticks_fill_the_tape(model):
    """32 / 48 kHz rows beside 16 kHz ones (steps 1 / 2 / 3 side by side), zero-stuffed so that the comb phase matters, odd row lengths,
    a silent row in every tick: the tape holds what the comb kept."""
    from silero_vad_amd import ROW_SILENT, decimate
    rig = Rig(model, 16000)
    rig.pump.set_wideband(3)
    n = rig.n
    rng = np.random.default_rng(19)
    phase = [0] * S
    for t in range(14):
        r = rig.slot()
        area = rig.pump.wide_slot(r)
        st, ln, sp, off, at = [], [], [], [], 0
        quiet = int(rng.integers(0, S))
        for b in rng.permutation(S):
            b = int(b)
            step = 1 + b % 3
            if b != quiet and rng.random() < 0.3:
                continue
            length = int(rng.integers(1, step * n + 1)) if rng.random() < 0.5 else step * int(rng.choice([160, 320, 480]))
            x = np.full(length, -77, np.int16)
            first = (-phase[b]) % step
            x[first::step] = noise(rng, len(x[first::step]))
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
        rig.pump.submit_wide_packets(r, st, ln, sp, off)
        rig.t += 1
        for b in st:
            assert rig.pump.wide_phase(b) == phase[b]
        if t % 3 == 2:
            rig.check()
    rig.drain()
    rig.check()
    assert max(rig.count(b) for b in range(S)) > TAPE
    rig.close()


def fetch_checked(rig, streams, starts, ends, offsets_of, device):
    """One fetch of the requests into a sentinel-filled buffer, at the offsets offsets_of(counts) gives: first / count are the rule's,
    the bytes are fed's, everything else is still the sentinel.  -> the buffer as numpy."""
    from silero_vad_amd import tape_window
    p = rig.pump
    first, count = p.tape_windows(streams, starts, ends)
    for i, b in enumerate(streams):
        assert (int(first[i]), int(count[i])) == tape_window(rig.count(b), rig.floor[b], rig.tape, rig.n, starts[i], ends[i]), i
    offsets = offsets_of(count)
    size = int(max([0] + [o + c for o, c in zip(offsets, count)])) + 40
    if device:
        out = torch.full((size,), SENTINEL, dtype=torch.int16, device="cuda:0")
        torch.cuda.synchronize()
        p.fetch_audio_into(streams, first, count, out, offsets)
        got = out.cpu().numpy()
    else:
        got = np.full(size, SENTINEL, np.int16)
        p.fetch_audio_into(streams, first, count, got, offsets)
    want = np.full(size, SENTINEL, np.int16)
    for i, b in enumerate(streams):
        want[offsets[i]:offsets[i] + count[i]] = rig.samples(b, int(first[i]), int(count[i]))
    assert np.array_equal(got, want)
    return got, first, count


def aligned(count):
    off = np.zeros(len(count), np.int64)
    if len(count):
        off[1:] = np.cumsum((np.asarray(count)[:-1] + 7) // 8 * 8)
    return off


def ragged(count):
    """Back to back with 1 ... 5 samples between the requests: mostly not 16-byte aligned."""
    off, at = [], 3
    for i, c in enumerate(count):
        off.append(at)
        at += int(c) + 1 + i % 5
    return np.array(off, np.int64)


@pytest.mark.parametrize("sr", [16000, 8000])
def test_ranges_after_the_ring_has_wrapped(model, sr):
    rig = Rig(model, sr)
    rng = np.random.default_rng(23)
    for _ in range(5):
        rig.chunks("full", rng)
    rig.chunks("masked", rng, present=np.arange(S) % 2 == 0)     # (the streams' wrap points differ from here on)
    rig.chunks("masked", rng, present=(np.arange(S) % 4 == 0) | (np.arange(S) == 18))
    rig.drain()
    n = rig.n
    assert (rig.count(4), rig.count(5), rig.count(18), rig.count(7)) == (7, 5, 7, 5)
    req = []
    for b in (4, 5, 18):
        lo, hi = (rig.count(b) - TAPE) * n, rig.count(b) * n
        wrap = ((rig.count(b) - 1) // TAPE) * TAPE * n           # chunk k * TAPE lies in slot 0: the ring's end is in front of it
        assert lo < wrap < hi
        req += [(b, wrap - 100, wrap + 100), (b, wrap - 3, wrap + 5), (b, wrap - 8, wrap + 8), (b, wrap - 1, wrap + 1),      # across the wrap
                (b, 0, lo + 10), (b, lo - 1, lo + 64), (b, -FAR, lo + 1),                                                  # clamped: first > start
                (b, hi - 10, hi + n), (b, hi - 1, FAR), (b, hi, hi + 5),                                                   # beyond held_hi
                (b, lo + 17, lo + 17), (b, 5, 5), (b, hi + 9, hi + 9),                                                     # empty
                (b, lo, hi), (b, lo + 1, hi - 1), (b, -FAR, FAR)]
        req += [(b, lo + 40 + k, lo + 41 + k) for k in range(8)]                # one sample at every position mod 8
        req += [(b, lo + 64 + k, lo + 64 + k + 72) for k in range(8)]           # ... and the funnel at every misalignment
    req += [(7, 3 * n + 5, 4 * n), (7, 3 * n + 5, 4 * n), (7, 2 * n, 5 * n)]    # one stream three times
    streams, starts, ends = [q[0] for q in req], [q[1] for q in req], [q[2] for q in req]
    host, first, count = fetch_checked(rig, streams, starts, ends, aligned, device=False)
    assert any(f > s for f, s in zip(first, starts)) and any(c == 0 for c in count) and int(count.max()) == TAPE * n
    dev, _, _ = fetch_checked(rig, streams, starts, ends, aligned, device=True)
    assert np.array_equal(host, dev)
    fetch_checked(rig, streams, starts, ends, ragged, device=True)              # unaligned destinations: element by element
    fetch_checked(rig, streams, starts, ends, ragged, device=False)
    fetch_checked(rig, [], [], [], aligned, device=False)                       # n = 0
    fetch_checked(rig, [], [], [], aligned, device=True)
    # fetch_audio: the same through the public call, host and device
    audios, f1 = rig.pump.fetch_audio(streams, starts, ends)
    (packed, offsets, counts), f2 = rig.pump.fetch_audio(streams, starts, ends, device=True)
    assert packed.device.type == "cuda" and packed.dtype == torch.int16 and np.array_equal(f1, first) and np.array_equal(f2, first)
    packed = packed.cpu().numpy()
    for i, b in enumerate(streams):
        assert np.array_equal(audios[i], rig.samples(b, int(first[i]), int(count[i]))), i
        assert offsets[i] % 8 == 0 and np.array_equal(packed[offsets[i]:offsets[i] + counts[i]], audios[i]), i
    assert rig.pump.fetch_audio([], [], [])[0] == []
    rig.check()
    rig.close()


def test_a_stale_range_is_refused_and_nothing_is_written(model):
    from silero_vad_amd._lib import VadError
    rig = Rig(model, 16000)
    rng = np.random.default_rng(29)
    for _ in range(4):
        rig.chunks("full", rng)
    first, count = rig.pump.tape_windows([2, 9], [-FAR, 600], [FAR, 700])
    assert count.tolist() == [TAPE * rig.n, 100]
    for _ in range(TAPE):
        rig.chunks("full", rng)                                  # (still in flight when the fetch is made: it synchronises)
    for out in (np.full(4 * TAPE * rig.n, SENTINEL, np.int16), torch.full((4 * TAPE * rig.n,), SENTINEL, dtype=torch.int16, device="cuda:0")):
        with pytest.raises(VadError, match="no longer held"):
            rig.pump.fetch_audio_into([2, 9], first, count, out, [0, TAPE * rig.n])
        assert bool((out == SENTINEL).all())
    # half stale: the tail of the old range is still held, the call is refused as a whole
    rig.drain()
    f2, c2 = rig.pump.tape_windows([2], [-FAR], [FAR])
    rig.chunks("full", rng)
    out = np.full(TAPE * rig.n, SENTINEL, np.int16)
    with pytest.raises(VadError, match="no longer held"):
        rig.pump.fetch_audio_into([2], f2, c2, out, [0])
    assert (out == SENTINEL).all()
    rig.drain()
    rig.check()
    rig.close()


def test_open_with_ticks_in_flight_restarts_clock_and_tape(model, golden):
    """Two ticks in flight, then open_stream(3): the earlier ticks' chunks of the slot do not count -- the clock and the tape restart at
    0, in step with the sample numbers of the new stream's events and with the iterator's current_sample."""
    from silero_vad_amd import snapshot_info
    pcm = golden["16k"]["pcm_i16"]
    rig = Rig(model, 16000)
    rng = np.random.default_rng(31)
    rig.chunks("full", rng)
    rig.drain()
    rig.chunks("full", rng)
    rig.chunks("full", rng)                                      # two ticks in flight
    rig.pump.open_stream(3)
    rig.reopen(3)
    n, speech = rig.n, []
    for t in range(4):                                           # the new stream speaks from its first chunk on
        r = rig.slot()
        for b in range(S):
            row = pcm[t * n:(t + 1) * n] if b == 3 else noise(rng, n)
            rig.pump.slot(r)[b] = row
            rig.feed(b, row)
        rig.pump.submit(r)
        rig.t += 1
    rig.drain()
    assert rig.pump.tape_state(3) == (4, 0) and rig.pump.tape_state(2) == (7, 0)
    rig.check()
    starts = [e["start"] for b, e in rig.events if b == 3 and "start" in e]
    assert starts and starts[-1] < 4 * n                         # counted on the new stream's clock ...
    audios, first = rig.pump.fetch_audio([3], [starts[-1]], [4 * n])
    assert first[0] == max(starts[-1], n) and np.array_equal(audios[0], pcm[first[0]:4 * n])      # ... which is the tape's
    info = snapshot_info(rig.pump.export_streams())
    for b in range(S):
        assert info[b]["current_sample"] == rig.pump.tape_state(b)[0] * n, b
    rig.close()


def test_an_absent_stream_keeps_its_tape(model):
    rig = Rig(model, 8000)
    rng = np.random.default_rng(37)
    for _ in range(4):
        rig.chunks("full", rng)
    present = np.ones(S, bool)
    present[[5, 16]] = False
    for route in ("masked", "compact", "rows", "masked", "compact"):           # more ticks than the tape has chunks
        rig.chunks(route, rng, present=present)
    rig.drain()
    assert rig.pump.tape_state(5) == (4, 0) and rig.pump.tape_state(16) == (4, 0) and rig.pump.tape_state(6) == (9, 0)
    rig.check()
    rig.close()


@pytest.mark.parametrize("sr", [16000, 8000])
def test_export_ignores_the_tape_and_import_restarts_it(model, sr):
    from silero_vad_amd import StreamPump, snapshot_info
    rig = Rig(model, sr)
    plain = StreamPump(model.engine, sr, streams=S, parts=PARTS)
    rng = np.random.default_rng(41)
    for t in range(5):
        rows = noise(rng, S * rig.n).reshape(S, rig.n)
        present = rng.random(S) >= 0.3
        for p in (rig.pump, plain):
            p.slot(0)[:] = rows
            p.submit(0, present)
            p.poll()
        for b in np.flatnonzero(present):
            rig.feed(b, rows[b])
    blob = rig.pump.export_streams()
    assert np.array_equal(blob, plain.export_streams())          # the blob of a taped pump is the blob of an untaped one
    assert np.array_equal(rig.pump.export_streams(version=2), plain.export_streams(version=2))
    rig.check()
    # into another taped pump's slots, which have a history of their own
    dst = Rig(model, sr)
    dst.chunks("full", rng)
    dst.drain()
    info = snapshot_info(blob)
    src_of = {7: 2, 0: 18, 18: 11}
    dst.pump.import_streams(blob, list(src_of), [src_of[b] for b in src_of])
    for b, a in src_of.items():
        k = info[a]["current_sample"] // dst.n
        assert k == rig.count(a) and dst.pump.tape_state(b) == (k, k)
        dst.fed[b], dst.base[b], dst.floor[b] = np.zeros(0, np.int16), k * dst.n, k
    assert dst.pump.tape_state(1) == (1, 0)
    dst.check()                                                  # nothing before the import is held; the other slots are untouched
    for route in ("full", "masked", "rows", "full"):
        dst.chunks(route, rng)
    dst.drain()
    dst.check()                                                  # ... and later ticks are fetchable at the continued sample numbers
    b, k = 7, info[2]["current_sample"] // dst.n
    audios, first = dst.pump.fetch_audio([b], [0], [FAR])
    assert first[0] == max(k, dst.count(b) - TAPE) * dst.n and len(audios[0]) == dst.count(b) * dst.n - first[0] > 0
    # into an untaped pump: as ever
    plain.import_streams(blob, [3], [2])
    for p in (rig, dst):
        p.close()
    plain.close()


def test_refusals_leave_the_pump_usable(model):
    from silero_vad_amd import StreamPump
    from silero_vad_amd._lib import VadError
    rng = np.random.default_rng(43)
    # set_tape: with 1, twice, after a tick
    p = StreamPump(model.engine, 16000, streams=S, parts=PARTS)
    with pytest.raises(VadError, match="at least 2"):
        p.set_tape(1)
    assert p.tape_chunks == 0
    with pytest.raises(VadError, match="no tape"):
        p.fetch_audio([0], [0], [10])
    with pytest.raises(VadError, match="no tape"):
        p.tape_state(0)
    with pytest.raises(VadError, match="no tape"):
        p.fetch_audio_into([0], [0], [10], np.zeros(16, np.int16), [0])
    p.slot(0)[:] = noise(rng, S * p.n).reshape(S, p.n)
    p.submit(0)
    assert p.poll()[1] == 0
    with pytest.raises(VadError, match="first tick"):
        p.set_tape(4)
    p.submit(1)
    assert p.poll()[1] == 1                                      # still usable, still untaped
    p.close()
    p = StreamPump(model.engine, 16000, streams=S, parts=PARTS)
    p.set_tape(4)
    with pytest.raises(VadError, match="already"):
        p.set_tape(4)
    assert p.tape_chunks == 4
    # tape and the resampled route, in both orders
    with pytest.raises(VadError, match="tape"):
        p.set_resample((44100,))
    p.close()
    p = StreamPump(model.engine, 16000, streams=S, parts=PARTS)
    p.set_resample((44100,))
    with pytest.raises(VadError, match="resample"):
        p.set_tape(4)
    assert p.tape_chunks == 0
    p.slot(0)[:] = noise(rng, S * p.n).reshape(S, p.n)
    p.submit(0)
    assert p.poll()[1] == 0
    p.close()
    with pytest.raises(VadError, match="resample"):
        q = StreamPump(model.engine, 16000, streams=S, parts=PARTS)
        q.set_resample((24000,))
        try:
            q.set_tape(8)
        finally:
            q.close()
    # a stream out of range, start > end: nothing queued, the next tick shows the pump is whole
    rig = Rig(model, 16000)
    rig.chunks("full", rng)
    for bad in (([S], [0], [10]), ([-1], [0], [10]), ([0, 3], [0, 11], [10, 10])):
        with pytest.raises(VadError):
            rig.pump.fetch_audio(*bad)
        with pytest.raises(VadError):
            rig.pump.tape_windows(*bad)
    out = np.full(64, SENTINEL, np.int16)
    for bad in (([S], [0], [10], [0]), ([0], [0], [-1], [0]), ([0], [100], [rig.n], [0])):
        with pytest.raises((VadError, ValueError)):
            rig.pump.fetch_audio_into(bad[0], bad[1], bad[2], out, bad[3])
    with pytest.raises(ValueError):
        rig.pump.fetch_audio_into([0], [0], [100], out, [0])     # does not fit into out
    assert (out == SENTINEL).all()
    rig.chunks("masked", rng)
    rig.drain()
    rig.check()
    rig.close()


def test_utterances_end_to_end(model, golden):
    """The 16 kHz speech fixture as mu-law 20 ms packets on three streams at different offsets into the recording: every utterance the
    collector returns is g711_expand(encoded)[start:end], the events are those of an untaped pump, and with a short tape a long
    utterance comes back with first > start and an exact tail."""
    from silero_vad_amd import StreamPump, UtteranceCollector, g711_expand
    pcm = golden["16k"]["pcm_i16"]
    total, pkt = 115200, 320
    sent = {b: encode(pcm[off:off + total], "ulaw") for b, off in ((1, 0), (8, 40000), (17, 78000))}
    heard = {b: g711_expand(x, "ulaw") for b, x in sent.items()}
    long_tape, short_tape = 160, 24
    pumps = [StreamPump(model.engine, 16000, streams=S, parts=PARTS, tape_chunks=long_tape),
             StreamPump(model.engine, 16000, streams=S, parts=PARTS, tape_chunks=short_tape),
             StreamPump(model.engine, 16000, streams=S, parts=PARTS)]
    collectors = [UtteranceCollector(pumps[0]), UtteranceCollector(pumps[1])]
    events, utterances = [[], [], []], [[], []]
    for t in range(total // pkt):
        pk = [(b, x[t * pkt:(t + 1) * pkt], "ulaw") for b, x in sent.items()]
        for i, p in enumerate(pumps):
            p.write_coded_packets(0, pk)
            ev, _ = p.poll()
            events[i] += ev
            if i < 2:
                utterances[i] += collectors[i].feed(ev)
    assert events[0] == events[2] and events[1] == events[2]
    ends = [(b, e["end"]) for b, e in events[2] if "end" in e]
    assert len(ends) >= 5 and [(u[0], u[2]) for u in utterances[0]] == ends and [(u[0], u[2]) for u in utterances[1]] == ends
    longest = 0
    for b, start, end, first, audio in utterances[0]:
        assert start is not None and first == start and np.array_equal(audio, heard[b][start:end]), (b, start, end)
        longest = max(longest, end - start)
    assert short_tape * 512 < longest < long_tape * 512
    cut = 0
    for b, start, end, first, audio in utterances[1]:
        assert start <= first <= end and np.array_equal(audio, heard[b][first:end]), (b, start, end)
        cut += first > start
    assert cut >= 1
    # an END whose START was never fed
    assert UtteranceCollector(pumps[0]).feed([(4, {"end": 999})]) == [(4, None, 999, None, None)]
    c = UtteranceCollector(pumps[0])
    c.feed([(1, {"start": 5})])
    c.forget(1)
    assert c.feed([(1, {"end": 900})]) == [(1, None, 900, None, None)]
    for p in pumps:
        p.close()
