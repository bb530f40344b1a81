"""The pump's resampled packet route (vad_pump_set_resample + vad_pump_submit_resampled_packets, csrc/pump.hip + kernel_present.hip
assemble_resampled_packets): 44.1 / 24 / 22.05 / 11.025 kHz int16 rows, brought to the net's rate on the device per stream by the streaming
form of the resampler.  The route is defined by reduction, and the reference is restated here (`Ref`), per stream:
    y = resample_device(engine, the stream's whole int16 audio)              -- the batch kernel on the concatenated rows
    a stream that has received g input samples has emitted resample_stream_ready(g) outputs
    chunk k, y[k N : (k + 1) N], is stepped at the tick its last sample became ready, through Engine.step_present on an fp32 [streams][N]
    device batch with the tick's flags; the events come from BatchVADIterator on the recorded probabilities.
Probabilities, events, pending counts, `resample_state` and the final (h, c, context) must equal it bit for bit.
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest
import torch

from test_resample import as_float, dense_resample

pytestmark = pytest.mark.gpu

TIGHT = 2e-5        # tests/test_gpu_parity.py: the GPU's probabilities against the oracle's on the same float32 samples
CAP = 48            # three 16-stream tiles
RATES = (44100, 24000, 22050)


@pytest.fixture(scope="module")
def model(built):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback to silently pass on)")
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    assert m.engine._h, "native engine not created"
    return m


@pytest.fixture(scope="module")
def speech(golden):
    """rate -> 2.5 s of the fixture speech at that rate, int16 (the formula of tests/test_resample.py: `resample` serves the net's rates only)"""
    out = {}

    def at(rate, sr=16000):
        if (rate, sr) not in out:
            src = golden["16k" if sr == 16000 else "8k"]["pcm_i16"]
            x = src[30 * sr // 1000 * 32:30 * sr // 1000 * 32 + 5 * sr // 2]
            out[rate, sr] = np.clip(np.rint(dense_resample(as_float(x), sr, rate) * 32768.0), -32768, 32767).astype(np.int16)
        return out[rate, sr]
    return at


class Ref:
    """The reference restated (module docstring) beside the pump under test, driven in lock step.  `audio(s, rate, x)` gives stream s its
    whole input; a tick is a list of rows (stream, n) or (stream, n, True) -- the stream's next n input samples, as a payload or (they
    must be zeros) as a silent row.  Expected results are queued at submit and compared when the tick is retired."""

    def __init__(self, model, rates, sr=16000, cap=CAP, **kw):
        from silero_vad_amd import BatchVADIterator, StreamPump, resample_geometry
        self.model, self.sr, self.cap, self.rates = model, sr, cap, tuple(rates)
        self.N = 512 if sr == 16000 else 256
        self.pump = StreamPump(model.engine, sr, streams=cap, **kw)
        self.pump.set_resample(rates)
        self.A = max(-(-self.N * resample_geometry(r, sr)[0] // resample_geometry(r, sr)[1]) for r in rates)
        self.A = (self.A + 7) // 8 * 8
        assert self.pump.resample_row == self.A and len(self.pump.resample_slot(0)) == cap * self.A * 2
        dev = model.device
        self.ctx = torch.zeros((cap, self.N // 8), device=dev)
        self.state = torch.zeros((2, cap, 128), device=dev)
        self.batch = torch.full((cap, self.N), 0.25, device=dev)
        self.it = BatchVADIterator(cap, sampling_rate=sr)
        self.x, self.y, self.rate = [None] * cap, [None] * cap, [0] * cap
        self.g, self.done = [0] * cap, [0] * cap
        self.expect, self.probs, self.events, self.stepped = [], [[] for _ in range(cap)], 0, 0

    def audio(self, s, rate, x):
        from silero_vad_amd import resample_device
        assert self.g[s] == 0 and x.dtype == np.int16
        self.x[s], self.rate[s] = x, rate
        self.y[s] = resample_device(self.model.engine, torch.from_numpy(x).to(self.model.device), None, rate, self.sr)

    def ready(self, s, extra=0):
        from silero_vad_amd import resample_stream_ready
        return resample_stream_ready(self.rate[s], self.sr, self.g[s] + extra)

    def room(self, s):
        """the longest row stream s may submit now: at most A samples, pending + new outputs below 2 N"""
        n = min(self.A, len(self.x[s]) - self.g[s])
        while n > 0 and self.ready(s, n) - self.done[s] * self.N >= 2 * self.N:
            n -= 1
        return n

    def length_for(self, s, outputs, exact=True):
        """the shortest row after which stream s has `outputs` outputs ready beyond its stepped chunks (exact: not one more -- a pair that
        downsamples passes every count)"""
        n = 1
        while self.ready(s, n) - self.done[s] * self.N < outputs:
            n += 1
        assert not exact or self.ready(s, n) - self.done[s] * self.N == outputs
        return n

    def state_of(self, s):
        from silero_vad_amd import resample_geometry
        if self.g[s] == 0:
            return 0, 0, 0
        O, Nr = resample_geometry(self.rate[s], self.sr)[:2]
        m = self.ready(s)
        return self.rate[s], self.g[s] - (m // Nr) * O, m - self.done[s] * self.N

    def tick(self, r, rows, offsets=None, rates_arg=True):
        area = self.pump.resample_slot(r)
        st, ln, rt, off, at = [], [], [], [], 0
        flags = np.zeros(self.cap, np.uint8)
        for i, row in enumerate(rows):
            s, n, silent = row if len(row) == 3 else (row[0], row[1], False)
            x = self.x[s][self.g[s]:self.g[s] + n]
            assert len(x) == n >= 1
            if silent:
                assert not x.any()
                off.append(-1)
            else:
                o = at if offsets is None else offsets[i]
                area[o:o + 2 * n] = x.view(np.uint8)
                off.append(o)
                at = o + (2 * n + 15) // 16 * 16
            st.append(s), ln.append(n), rt.append(self.rates.index(self.rate[s]))
            self.g[s] += n
            have = self.ready(s) - self.done[s] * self.N
            assert have < 2 * self.N
            if have >= self.N:
                self.batch[s] = self.y[s][self.done[s] * self.N:(self.done[s] + 1) * self.N]
                self.done[s] += 1
                flags[s] = 1
        self.pump.submit_resampled_packets(r, st, ln, rt if rates_arg else None, off)
        for s in st:
            assert self.pump.resample_state(s) == self.state_of(s), s
            assert self.pump.pending(s) == self.state_of(s)[2], s
        if flags.any():
            p = torch.empty((self.cap,), device=self.model.device)
            self.model.engine.step_present(self.batch, self.sr, self.ctx, self.state, p, torch.from_numpy(flags).to(self.model.device))
            p = p.cpu().numpy()
        else:
            p = np.full(self.cap, -1.0, np.float32)
        assert ((p >= 0) == (flags != 0)).all()
        self.expect.append((p, self.it.feed(np.where(flags != 0, p, 0.0), active=flags != 0)))

    def open_stream(self, s):
        self.pump.open_stream(s)
        self.ctx[s] = 0
        self.state[:, s] = 0
        self.it.reset(s)
        self.g[s] = self.done[s] = 0
        self.x[s] = self.y[s] = None

    def retire(self):
        ev, r = self.pump.poll()
        p, ev_ref = self.expect.pop(0)
        got = self.pump.probs(r)
        assert np.array_equal(got.view(np.uint32), p.view(np.uint32)), np.flatnonzero(got != p)
        assert ev == ev_ref
        self.events += len(ev)
        self.stepped += int((p >= 0).sum())
        for s in np.flatnonzero(p >= 0):
            self.probs[s].append(float(got[s]))
        return got

    def finish(self):
        assert self.pump.poll() == (None, None) and not self.expect
        ctx, state = self.ctx.cpu().numpy(), self.state.cpu().numpy()
        for s in range(self.cap):
            assert self.pump.pending(s) == self.state_of(s)[2] and self.pump.resample_state(s) == self.state_of(s), s
            h, c, x = self.pump.state(s)
            assert np.array_equal(h, state[0, s]) and np.array_equal(c, state[1, s]) and np.array_equal(x, ctx[s]), s

    def close(self):
        self.pump.close()


def frames(ref, s, rng):
    """the next row length of stream s: a 10 / 20 / 30 ms frame, or a uniform length, within what the stream may submit"""
    ms10 = ref.rate[s] / 100.0
    n = int(round(ms10 * int(rng.integers(1, 4)))) if rng.random() < 0.7 else int(rng.integers(1, ref.A + 1))
    return min(n, ref.room(s))


def test_resampled_packets_equal_the_batch_resampler_and_the_masked_step(model, oracle, speech):
    """48 streams (three tiles) at 44.1 / 24 / 22.05 kHz side by side in every tick: 10 / 20 / 30 ms frames and uniform lengths, ~10 % of
    ticks missed, empty ticks, rows in random arrival order, two ticks in flight.  Four streams also against the CPU oracle on the same
    device-resampled floats."""
    rng = np.random.default_rng(53)
    ref = Ref(model, RATES, parts=3, ring_slots=3)
    for s in range(CAP):
        rate = RATES[s % 3]
        x = speech(rate)
        ref.audio(s, rate, np.ascontiguousarray(np.roll(x, -s * 977)[:len(x) * 2 // 5 - int(rng.integers(0, 900))]))      # ~1 s: 31 chunks
    t = 0
    while any(ref.g[s] < len(ref.x[s]) for s in range(CAP)):
        rows = []
        if t % 11 != 10:                                         # (every 11th tick carries no row at all)
            for s in rng.permutation(CAP):
                if ref.g[s] < len(ref.x[s]) and rng.random() >= 0.1:
                    rows.append((int(s), frames(ref, s, rng)))
        ref.tick(t % 3, rows)
        if t > 0:
            ref.retire()
        if t < 5:
            assert {ref.rate[s] for s, _ in rows} == set(RATES)
        t += 1
    ref.retire()
    assert 30 <= t <= 120
    ref.finish()
    assert ref.stepped == sum(ref.ready(s) // 512 for s in range(CAP)) >= 28 * CAP and ref.events > 0
    pick = [0, 16, 32, 47]                                      # rates 44.1, 24, 22.05, 22.05 kHz; one stream of every tile
    m = min(len(ref.probs[s]) for s in pick)
    x = np.stack([ref.y[s][:m * 512].cpu().numpy() for s in pick])
    want = oracle.audio_forward(x, 16000)
    got = np.array([ref.probs[s][:m] for s in pick], np.float32)
    err = float(np.abs(got - want).max())
    print(f"max |dp| against the oracle over {m} chunks of 4 streams: {err:.3e}")
    assert err < TIGHT
    ref.close()


def test_packetisation_independence(model, speech):
    """The same audio on two streams, one in 10 ms frames from offset 0, the other in random rows at other slot offsets: identical
    probability sequences, bit for bit (both also equal the reference)."""
    rng = np.random.default_rng(59)
    ref = Ref(model, (44100,), cap=16, parts=1, ring_slots=2)
    x = speech(44100)[:25000]
    ref.audio(0, 44100, x)
    ref.audio(9, 44100, x.copy())
    t = 0
    while ref.g[0] < len(x) or ref.g[9] < len(x):
        rows, offs = [], []
        if ref.g[9] < len(x):
            rows.append((9, min(int(rng.integers(1, ref.A + 1)), ref.room(9))))
            offs.append(16 * int(rng.integers(200, 400)))
        if ref.g[0] < len(x):
            rows.append((0, min(441, ref.room(0))))
            offs.append(16 * int(rng.integers(0, 100)))
        ref.tick(t % 2, rows, offsets=offs, rates_arg=t % 2 == 0)
        ref.retire()
        t += 1
    ref.finish()
    assert len(ref.probs[0]) == len(ref.probs[9]) == ref.ready(0) // 512 >= 17 and ref.probs[0] == ref.probs[9]
    ref.close()


def test_edge_rows(model, speech):
    """Hand-built rows (the list of the issue): a first row shorter than the latency; len = 1 rows in sequence, also on an upsampling pair
    where one input may yield two outputs; rows that yield exactly N - c - 1, N - c and N - c + 1 outputs behind c pending; the longest
    accepted row, which leaves N - 1 pending; a row that ends at the last byte of the area; silent rows, alone and between payload rows,
    equal to payload rows of zeros; rates=None."""
    from silero_vad_amd import _lib
    N = 512
    ref = Ref(model, (44100, 11025), cap=32, parts=2, ring_slots=2)
    pump, A = ref.pump, ref.A
    x44, x11 = speech(44100), speech(11025)

    def tick(r, rows, **kw):
        ref.tick(r, rows, **kw)
        return ref.retire()

    # a first row one sample shorter than what the first output needs: no output; then len = 1 rows, the first outputs among them
    ref.audio(0, 44100, x44[:6000])
    ref.audio(1, 11025, x11[:3000])
    n0, n1 = ref.length_for(0, 1) - 1, ref.length_for(1, 1, exact=False) - 1
    assert n0 >= 10 and n1 >= 4
    p = tick(0, [(0, n0), (1, n1)])
    assert (p == -1.0).all() and pump.resample_state(0) == (44100, n0, 0) and pump.resample_state(1) == (11025, n1, 0)
    seen = [(0, 0)]
    for i in range(12):
        tick(i % 2, [(1, 1), (0, 1)])
        seen.append((pump.pending(0), pump.pending(1)))
    assert seen[1][0] == 1 and seen[1][1] >= 1                  # (the next input completes each stream's first output)
    assert {b[0] - a[0] for a, b in zip(seen, seen[1:])} == {0, 1}             # 44.1 k: an output every second or third input
    assert {b[1] - a[1] for a, b in zip(seen, seen[1:])} == {1, 2}             # 11.025 k: one or two outputs an input
    # N - c - 1, N - c, N - c + 1 outputs behind c pending (streams 2, 3, 4: c = 100; 5, 6, 7: c = 37)
    for s in range(2, 8):
        ref.audio(s, 44100, np.ascontiguousarray(np.roll(x44, -1000 * s)[:6000]))
    ref.audio(8, 44100, x44[3000:3000 + A + 40])
    tick(0, [(s, ref.length_for(s, 100)) for s in (2, 3, 4)] + [(s, ref.length_for(s, 37)) for s in (5, 6, 7)] + [(8, 40)])
    assert [pump.pending(s) for s in range(2, 8)] == [100] * 3 + [37] * 3
    p = tick(1, [(2, ref.length_for(2, N - 1)), (3, ref.length_for(3, N)), (4, ref.length_for(4, N + 1)),
                 (5, ref.length_for(5, N - 1)), (6, ref.length_for(6, N)), (7, ref.length_for(7, N + 1))])
    assert [pump.pending(s) for s in range(2, 8)] == [N - 1, 0, 1] * 2
    assert (p[[3, 4, 6, 7]] >= 0).all() and (p[[2, 5]] == -1.0).all()
    # the longest accepted row: behind N - 1 pending it brings N outputs and leaves N - 1; one sample more is refused
    for s in (2, 5):
        n = ref.room(s)
        assert ref.ready(s, n) - ref.done[s] * N == 2 * N - 1 and n < A
        with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
            pump.submit_resampled_packets(0, [s], [n + 1], [ref.rates.index(ref.rate[s])], [0])
        assert pump.poll() == (None, None) and pump.pending(s) == N - 1
        p = tick(0, [(s, n)])
        assert p[s] >= 0 and pump.pending(s) == N - 1
    # a row of A samples (the whole of a stream's share of the area) that ends at the last byte of the area, behind rows at bytes 16 and 4096
    area = len(pump.resample_slot(0))
    p = tick(1, [(8, A), (0, 9), (1, 33)], offsets=[area - 2 * A, 16, 4096])
    assert p[8] >= 0 and pump.pending(8) == ref.ready(8) - N
    # silent rows, alone and between payload rows: stream 10 takes them as silent rows, stream 11 as payload rows of zeros
    z = np.ascontiguousarray(x44[9000:9000 + 5000])
    z[700:1100] = 0
    z[1100 + 900:1100 + 900 + 1416 + 300] = 0
    for s in (10, 11):
        ref.audio(s, 44100, z.copy())
    for n, quiet, alone in ((700, False, False), (400, True, False), (900, False, False), (1416, True, True), (300, True, False),
                            (984, False, False)):
        if alone:                                                # (a tick whose only row is silent: not one byte of the area is copied)
            tick(0, [(10, n, True)])
            tick(1, [(11, n)])
        else:
            p = tick(0, [(10, n, quiet), (11, n)])
            assert p[10] == p[11]
    assert ref.probs[10] == ref.probs[11] and len(ref.probs[10]) == 3
    # rates=None: every row at rate index 0
    ref.audio(12, 44100, x44[12000:14000])
    ref.audio(13, 44100, x44[13000:15000])
    tick(0, [(12, 1416), (13, 1400)], rates_arg=False)
    p = tick(1, [(12, 300), (13, 8)], rates_arg=False)
    assert p[12] >= 0 and p[13] == -1.0 and pump.resample_state(13)[0] == 44100
    ref.finish()
    ref.close()


def test_an_8_khz_pump(model, speech):
    """44.1 kHz and 16 kHz rows into an 8 kHz pump (N = 256), random rows, two ticks in flight."""
    rng = np.random.default_rng(61)
    ref = Ref(model, (44100, 16000), sr=8000, cap=32, parts=2, ring_slots=3)
    assert ref.A == 1416
    for s in range(32):
        rate = (44100, 16000)[s % 2]
        x = speech(rate, 8000)
        ref.audio(s, rate, np.ascontiguousarray(np.roll(x, -s * 977)[:len(x) // 4 - int(rng.integers(0, 500))]))
    t = 0
    while any(ref.g[s] < len(ref.x[s]) for s in range(32)):
        rows = [(int(s), frames(ref, s, rng)) for s in rng.permutation(32) if ref.g[s] < len(ref.x[s]) and rng.random() >= 0.1]
        ref.tick(t % 3, rows)
        if t > 0:
            ref.retire()
        t += 1
    ref.retire()
    ref.finish()
    assert ref.stepped == sum(ref.ready(s) // 256 for s in range(32)) >= 15 * 32
    ref.close()


def test_refusals_queue_nothing(model, golden, speech):
    """Every refusal is VAD_ERR_ARG with nothing queued and no count touched, and the next valid tick gives the reference's bits; the
    binding rules against the other routes; export_streams refuses a bound stream and exports the others byte-identically to a pump
    without the route; open_stream unbinds."""
    from silero_vad_amd import StreamPump, _lib
    N = 512
    pcm = golden["16k"]["pcm_i16"][40 * N:]
    x44, x24 = speech(44100), speech(24000)
    ref = Ref(model, (44100, 24000), parts=1, ring_slots=2)
    plain = StreamPump(model.engine, 16000, streams=CAP, parts=1, ring_slots=2)
    pump, A = ref.pump, ref.A
    pump.set_wideband(2)
    area = CAP * A * 2
    ref.audio(2, 44100, x44[:4000])
    ref.audio(5, 24000, x24[:4000])
    ref.tick(0, [(2, 1000), (5, 301)])
    ref.retire()
    for q in (pump, plain):                                     # stream 7 has int16 samples pending from the packet route, on both pumps
        q.write_packets(1, [(7, pcm[:100])])
        q.poll()

    def snapshot():
        return [(pump.pending(s), pump.resample_state(s)) for s in range(CAP)]

    before = snapshot()
    assert before[2] == (ref.ready(2), ref.state_of(2)) and before[5][1][0] == 24000 and before[7] == (100, (0, 0, 0))
    many = list(range(CAP)) + [0]
    for streams, lengths, rates, offsets in (
            ([0], [8], [2], [0]), ([0], [8], [255], [0]),                                           # a rate index out of range
            ([CAP], [8], [0], [0]), ([-1], [8], [0], [0]), ([1, 1], [8, 8], [0, 1], [0, 16]),       # out of range, listed twice
            ([0, 3, 0], [8, 8, 8], [0, 1, 0], [0, 16, 32]),
            ([0], [0], [0], [0]), ([0], [-5], [0], [0]), ([0], [A + 1], [0], [0]), ([0], [A + 1], [1], [-1]),      # len < 1, longer than A
            ([0], [8], [0], [8]), ([0], [8], [0], [-16]),                                           # misaligned, in front of the area
            ([0], [9], [0], [area - 16]), ([0], [8], [0], [area]),                                  # runs past the area
            ([2], [8], [1], [0]), ([5], [8], [0], [0]), ([5], [8], None, [0]),                      # a row at another rate than the stream's
            ([7], [8], [0], [0]),                                                                   # int16 samples pending
            ([2], [ref.room(2) + 1], [0], [0]),                                                     # would complete two chunks
            ([0, 2], [8, ref.room(2) + 1], [0, 0], [0, 16]), ([3, 0], [8, A + 1], [1, 0], [0, 16]), # a good row in front of a bad one
            (many, [8] * len(many), [0] * len(many), [16 * i for i in range(len(many))])):          # more rows than streams
        with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
            pump.submit_resampled_packets(1, streams, lengths, rates, offsets)
        assert pump.poll() == (None, None) and snapshot() == before
    for bad in (lambda: pump.submit_resampled_packets(1, [0, 1], [8, 8], [0]), lambda: pump.submit_resampled_packets(1, [0], [8], [0], [0, 16]),
                lambda: pump.submit_resampled_packets(1, [0], [8], [300]), lambda: pump.submit_resampled_packets(1, [0], [8.0], [0]),
                lambda: pump.write_resampled_packets(1, [(0, pcm[:8], 48000)]), lambda: pump.write_resampled_packets(1, [(0, A + 1, 44100)])):
        with pytest.raises(ValueError):
            bad()
    # a bound stream on the other submit routes
    slot_of_2 = np.zeros(CAP, np.uint8)
    slot_of_2[2] = 1
    for bad in (lambda: pump.write_packets(1, [(2, pcm[:160])]), lambda: pump.write_packets(1, [(0, pcm[:160]), (5, 160)]),
                lambda: pump.write_coded_packets(1, [(2, pcm[:160], "s16")]), lambda: pump.submit_rows(1, [0, 2]),
                lambda: pump.submit(1), lambda: pump.submit(1, slot_of_2), lambda: pump.submit(1, slot_of_2, compact=True),
                lambda: pump.submit_wide_packets(1, [2], [320], [2])):
        with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
            bad()
        assert pump.poll() == (None, None) and snapshot() == before
    # set_resample: bad lists, an unserved rate; the same rates again are a no-op; refused with a tick in flight
    for rates in ((), (44100, 24000, 22050, 11025, 48000), (44100, 44100)):
        with pytest.raises((ValueError, _lib.VadError)):
            pump.set_resample(rates)
    for rates in ((16000,), (44100, 12345)):
        with pytest.raises(_lib.VadError, match="VAD_ERR_SAMPLE_RATE"):
            pump.set_resample(rates)
    pump.set_resample((44100, 24000))
    assert snapshot() == before
    # export: the bound streams are refused, the others leave byte-identically to the pump without the route (stream 7's pending samples too)
    for streams in ([2], [0, 5], None):
        with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
            pump.export_streams(streams)
    others = [s for s in range(CAP) if s not in (2, 5)]
    assert np.array_equal(pump.export_streams(others), plain.export_streams(others))
    # the next valid tick: the reference's bits (stream 0 binds to 24 kHz here)
    ref.audio(0, 24000, x24[500:3000])
    ref.tick(1, [(5, 444), (0, 700), (2, ref.length_for(2, N))])
    with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
        pump.set_resample((44100,))
    p = ref.retire()
    assert p[2] >= 0 and p[5] == -1.0 and pump.resample_state(0)[0] == 24000
    # open_stream unbinds: stream 2 then runs the int16 packet route as on the plain pump; import into a bound slot leaves it unbound
    ref.open_stream(2)
    plain.open_stream(2)
    assert pump.resample_state(2) == (0, 0, 0) and pump.pending(2) == 0
    blob = plain.export_streams([7])
    pump.import_streams(blob, [5])
    plain.import_streams(blob, [5])
    ref.g[5] = ref.done[5] = 0
    assert pump.resample_state(5) == (0, 0, 0) and pump.pending(5) == 100
    for t in range(3):
        rows = [(2, pcm[1000 + 400 * t:1400 + 400 * t]), (5, pcm[200 + 300 * t:500 + 300 * t])]
        out = []
        for q in (pump, plain):
            q.write_packets(t % 2, rows)
            ev, r = q.poll()
            out.append((ev, q.probs(r)[[2, 5]].copy(), q.pending(2), q.pending(5)))
        assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]) and out[0][2:] == out[1][2:]
    assert (out[0][1] >= 0).any()
    for s in (2, 5):
        for a, b in zip(pump.state(s), plain.state(s)):
            assert np.array_equal(a, b), s
    ref.close()
    plain.close()
    # a pump on which the enabling call was never made
    bare = StreamPump(model.engine, 16000, streams=16)
    assert bare._L.vad_pump_resample_slot(bare._h, 0) is None and bare._L.vad_pump_resample_state(bare._h, 0, None, None, None) == 1
    with pytest.raises(ValueError):
        bare.resample_slot(0)
    with pytest.raises(ValueError):
        bare.resample_state(0)
    with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
        bare.submit_resampled_packets(0, [0], [8], [0], [0])
    assert bare.poll() == (None, None) and bare.pending(0) == 0
    bare.close()


def test_open_rebinds_from_zero_history(model, speech):
    """A stream that is opened again binds to another rate and starts from zero history, pending outputs and counters, on the device too:
    its results are those of a fresh stream (the reference restarts with it), also with a tick in flight at the open."""
    ref = Ref(model, (44100, 24000), cap=16, parts=1, ring_slots=3)
    x44, x24 = speech(44100), speech(24000)
    ref.audio(3, 44100, x44[:5000])
    ref.audio(4, 44100, x44[2000:7000])
    ref.tick(0, [(3, 1416), (4, 1000)])
    ref.tick(1, [(3, 1300), (4, 1416)])                          # (two ticks in flight at the open)
    ref.open_stream(3)
    ref.pump.close_stream(4)
    assert ref.pump.resample_state(3) == (0, 0, 0) and ref.pump.resample_state(4) == (0, 0, 0) and ref.pump.pending(4) == 0
    ref.retire()
    ref.retire()
    ref.audio(3, 24000, x24[:4000])
    for t in range(4):
        ref.tick(t % 3, [(3, 760)])
        ref.retire()
    assert len(ref.probs[3]) == 1 + 3 and ref.pump.resample_state(3)[0] == 24000
    ref.g[4] = ref.done[4] = 0                                   # (closed: unbound, its pending outputs dropped; its (h, c, context) stay)
    ref.finish()
    ref.close()


def test_a_pump_without_the_route_runs_as_before(model, golden):
    """The packet and wide routes on a pump that never called set_resample and on one that enabled it and never used it: the same
    probabilities, events, pending counts and states, bit for bit; the first allocates nothing of the route."""
    from silero_vad_amd import StreamPump
    N = 512
    pcm = golden["16k"]["pcm_i16"]
    rng = np.random.default_rng(67)
    pumps = [StreamPump(model.engine, 16000, streams=CAP, parts=3, ring_slots=2) for _ in range(2)]
    for p in pumps:
        p.set_wideband(2)
    pumps[1].set_resample((44100, 24000, 22050, 11025))
    assert pumps[0]._L.vad_pump_resample_slot(pumps[0]._h, 0) is None
    assert len(pumps[1].resample_slot(1)) == CAP * 1416 * 2 and pumps[1].resample_rates == (44100, 24000, 22050, 11025)
    src = [np.roll(pcm, -(30 * N + s * 7919)) for s in range(CAP)]
    at = np.zeros(CAP, np.int64)
    stepped = 0
    for t in range(16):
        rows = []
        for s in rng.permutation(CAP):
            if rng.random() < 0.9:
                ln = int(rng.choice([160, 320, 480])) if rng.random() < 0.7 else int(rng.integers(1, N + 1))
                rows.append((int(s), src[s][at[s]:at[s] + ln]))
                at[s] += ln
        out = []
        for p in pumps:
            if t % 4 == 3:                                       # a wide tick: the same samples held at 32 kHz
                wide = [np.repeat(x, 2) for _, x in rows]
                area, o, offs = p.wide_slot(t % 2), 0, []
                for w in wide:
                    area[o:o + 2 * len(w)] = w.view(np.uint8)
                    offs.append(o)
                    o += (2 * len(w) + 15) // 16 * 16
                p.submit_wide_packets(t % 2, [s for s, _ in rows], [len(w) for w in wide], [2] * len(rows), offs)
            else:
                p.write_packets(t % 2, rows)
            ev, r = p.poll()
            out.append((ev, r, p.probs(r).copy()))
        assert out[0][0] == out[1][0] and out[0][1] == out[1][1] and np.array_equal(out[0][2], out[1][2])
        stepped += int((out[0][2] >= 0).sum())
    assert stepped > 6 * CAP                                     # (16 ticks of ~0.9 x 290 samples a stream: about 8 chunks each)
    for s in range(CAP):
        assert pumps[0].pending(s) == pumps[1].pending(s) == at[s] % N
        assert pumps[1].resample_state(s) == (0, 0, 0)
        for a, b in zip(pumps[0].state(s), pumps[1].state(s)):
            assert np.array_equal(a, b), s
    assert np.array_equal(pumps[0].export_streams(), pumps[1].export_streams())
    for p in pumps:
        p.close()
