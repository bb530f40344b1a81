"""The pump's packet route (vad_pump_submit_packets, csrc/pump.hip + kernel_present.hip assemble_packets): live streams that deliver
10 / 20 / 30 ms frames (and odd lengths after a loss) instead of 32 ms chunks.  The reference's VADIterator takes one chunk per call
(src/silero_vad/utils_vad.py:507-549), so a packet stream means "the concatenation of its packets, cut into chunks": every result here
is compared, bit for bit, with the same pump fed those chunks through vad_pump_submit_rows at the tick their last sample arrived.
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest
import torch

from conftest import SRS

pytestmark = pytest.mark.gpu

TIGHT = 2e-5


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


def packet_plan(total, n, sr, rng):
    """Packet lengths that cover `total` samples: mostly 10 / 20 / 30 ms frames, the rest uniform in [1, n] (a jitter buffer after a
    loss); the last one is cut at the end of the audio."""
    ms10 = sr // 100
    lens, left = [], total
    while left > 0:
        ln = int(rng.choice([ms10, 2 * ms10, 3 * ms10])) if rng.random() < 0.7 else int(rng.integers(1, n + 1))
        ln = min(ln, left)
        lens.append(ln)
        left -= ln
    return lens


def schedule(plans, rng, miss=0.1, always=(), empty_every=97):
    """Ticks of (stream, first sample, length) packets in ARRIVAL order: each stream sends its next packet at a tick with probability
    1 - miss (streams in `always`: every tick), and every `empty_every`-th tick carries no packet at all."""
    cap = len(plans)
    nxt, start = [0] * cap, [0] * cap
    ticks = []
    while any(nxt[s] < len(plans[s]) for s in range(cap)):
        pk = []
        if len(ticks) % empty_every != empty_every - 1:
            for s in range(cap):
                if nxt[s] < len(plans[s]) and (s in always or rng.random() >= miss):
                    ln = plans[s][nxt[s]]
                    pk.append((s, start[s], ln))
                    start[s] += ln
                    nxt[s] += 1
        ticks.append([pk[i] for i in rng.permutation(len(pk))])
    return ticks


def completions(ticks, n):
    """Per tick: (stream, chunk index) of every chunk whose last sample arrives in it, in the tick's arrival order."""
    return [[(s, (a + ln) // n - 1) for s, a, ln in pk if (a + ln) // n > a // n] for pk in ticks]


def drive(pump, n_ticks, done, feed, nchunks):
    """Submit tick t, retire tick t - 1.  -> (probabilities [streams, nchunks] by chunk index, events per stream)."""
    cap, R = pump.streams, pump.ring_slots
    probs = np.full((cap, nchunks), np.nan, np.float32)
    events = {s: [] for s in range(cap)}
    for t in range(n_ticks + 1):
        if t < n_ticks:
            feed(t % R, t)
        if t > 0:
            ev, r = pump.poll()
            p = pump.probs(r)
            on = np.zeros(cap, bool)
            for s, k in done[t - 1]:
                probs[s, k] = p[s]
                on[s] = True
            assert (p[~on] == -1.0).all()                       # VAD_PROB_ABSENT: no chunk completed
            for s, e in ev:
                assert on[s], "a stream without a completed chunk emitted an event"
                events[s].append(e)
    assert pump.poll() == (None, None)
    return probs, events


def feed_packets(pump, audio, ticks):
    return lambda r, t: pump.write_packets(r, [(s, audio[s][a:a + ln]) for s, a, ln in ticks[t]])


def feed_rows(pump, audio, done, n):
    def feed(r, t):
        slot = pump.slot(r)
        for i, (s, k) in enumerate(done[t]):
            slot[i] = audio[s][k * n:(k + 1) * n]
        pump.submit_rows(r, [s for s, _ in done[t]])
    return feed


def assert_same_state(a, b, streams):
    for s in streams:
        for x, y in zip(a.state(s), b.state(s)):
            assert np.array_equal(x, y), s


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_packets_equal_the_rechunked_stream(model, golden, tag):
    """100 streams (not a multiple of 16), packets of 10 / 20 / 30 ms and uniform lengths in [1, N], ~10 % of ticks without a packet,
    rows in random arrival order: probabilities, events, final (h, c, context) and the pending residue equal the submit_rows pump fed
    the re-chunked streams; stream 0 (the whole fixture, a packet every tick) gives the reference VADIterator's own events."""
    from silero_vad_amd import StreamPump
    sr, g = SRS[tag], golden[tag]
    n = chunk_of(sr)
    pcm = g["pcm_i16"]
    T = len(pcm) // n
    cap = 100
    rng = np.random.default_rng(11)
    audio = [np.roll(pcm, -s * 7919)[:T * n - (0 if s == 0 else int(rng.integers(0, n)))].copy() for s in range(cap)]
    ticks = schedule([packet_plan(len(a), n, sr, rng) for a in audio], rng, always=(0,))
    done = completions(ticks, n)
    assert sum(1 for pk in ticks if not pk) >= 2                # ticks in which nobody delivers
    rec = golden["segments"][tag]["iterator"]["default"]
    pk_pump = StreamPump(model.engine, sr, streams=cap, parts=3, ring_slots=3, **rec["init"])
    got, got_ev = drive(pk_pump, len(ticks), done, feed_packets(pk_pump, audio, ticks), T)
    ref_pump = StreamPump(model.engine, sr, streams=cap, parts=3, ring_slots=3, **rec["init"])
    want, want_ev = drive(ref_pump, len(ticks), done, feed_rows(ref_pump, audio, done, n), T)
    for s in range(cap):                                        # every whole chunk of every stream was stepped, once
        assert not np.isnan(got[s, :len(audio[s]) // n]).any() and np.isnan(got[s, len(audio[s]) // n:]).all(), s
    assert np.array_equal(got, want, equal_nan=True)
    assert got_ev == want_ev and sum(len(v) for v in got_ev.values()) > 100
    assert_same_state(pk_pump, ref_pump, range(cap))
    for s in range(cap):
        assert pk_pump.pending(s) == len(audio[s]) % n, s
    assert got_ev[0] == rec["events"], tag                      # the reference's own iterator events (39 / 92)
    assert np.abs(got[0] - np.asarray(g["probs_wav"]).reshape(-1)[:T]).max() < TIGHT
    h, c, x = pk_pump.state(0)                                  # context: the last C samples of the last completed chunk
    assert np.array_equal(x, audio[0][T * n - n // 8:T * n].astype(np.float32) / 32768.0)
    pk_pump.close()
    ref_pump.close()


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_packet_and_chunk_ticks_mix(model, golden, tag):
    """Packet ticks and chunk ticks (full, masked, compact, arrival-order rows) interleaved for streams with nothing pending give the
    all-chunk run's bits; a chunk tick that delivers to a stream with samples pending is refused, queues nothing and does not poison
    the pump."""
    from silero_vad_amd import StreamPump, _lib
    sr, g = SRS[tag], golden[tag]
    n = chunk_of(sr)
    pcm = g["pcm_i16"]
    cap, K = 40, 45
    rows = np.ascontiguousarray(np.stack([np.roll(pcm, -(30 * n + s * 7919))[:K * n] for s in range(cap)]))
    rng = np.random.default_rng(3)
    # the all-chunk run
    ref = StreamPump(model.engine, sr, streams=cap, parts=2, ring_slots=2)
    want = np.zeros((cap, K), np.float32)
    want_ev = {s: [] for s in range(cap)}
    for t in range(K):
        ref.slot(0)[:] = rows[:, t * n:(t + 1) * n]
        ref.submit(0)
        ev, r = ref.poll()
        want[:, t] = ref.probs(r)
        for s, e in ev:
            want_ev[s].append(e)
    pump = StreamPump(model.engine, sr, streams=cap, parts=2, ring_slots=2)
    got = np.full((cap, K), np.nan, np.float32)
    got_ev = {s: [] for s in range(cap)}
    k = np.zeros(cap, np.int64)                                 # chunks each stream has had stepped

    def retire(stepped):
        ev, r = pump.poll()
        p = pump.probs(r)
        for s in stepped:
            got[s, k[s]] = p[s]
            k[s] += 1
        for s, e in ev:
            got_ev[s].append(e)

    cycle, refused = 0, False
    while (k < K).any():
        # a packet tick: a whole chunk as ONE packet (completes at once), or its first part (the rest follows in the next packet tick)
        split = {}
        pk, stepped = [], []
        for s in rng.permutation(cap):
            if k[s] >= K or rng.random() < 0.2:
                continue
            chunk = rows[s, k[s] * n:(k[s] + 1) * n]
            if rng.random() < 0.4:
                pk.append((s, chunk))
                stepped.append(s)
            else:
                a = int(rng.integers(1, n))
                pk.append((s, chunk[:a]))
                split[s] = chunk[a:]
        pump.write_packets(0, pk)
        retire(stepped)
        if split and not refused:                               # chunks for streams with samples pending: refused, nothing queued
            s0 = next(iter(split))
            assert pump.pending(s0) > 0
            fl = np.zeros(cap, np.uint8)
            fl[s0] = 1
            for bad in (lambda: pump.submit(1), lambda: pump.submit(1, present=fl), lambda: pump.submit(1, present=fl, compact=True),
                        lambda: pump.submit_rows(1, [s0])):
                with pytest.raises(_lib.VadError, match="pending"):
                    bad()
                assert pump.poll() == (None, None)
            refused = True
        if split:
            pump.write_packets(1, list(split.items()))
            retire(list(split))
        assert all(pump.pending(s) == 0 for s in range(cap))
        # a chunk tick, by a route that changes from cycle to cycle
        route = cycle % 4
        on = np.flatnonzero(k < K) if route == 0 else np.flatnonzero((k < K) & (rng.random(cap) < 0.7))
        if route == 0 and len(on) < cap:                        # (a full tick needs a chunk of every stream)
            route = 1
        if route == 3:
            on = rng.permutation(on)
        slot = pump.slot(0)
        for i, s in enumerate(on):
            slot[i if route >= 2 else s] = rows[s, k[s] * n:(k[s] + 1) * n]
        fl = np.zeros(cap, np.uint8)
        fl[on] = 1
        if route == 0:
            pump.submit(0)
        elif route == 3:
            pump.submit_rows(0, on)
        else:
            pump.submit(0, present=fl, compact=route == 2)
        retire(sorted(on) if route != 3 else on)
        cycle += 1
    assert refused
    assert np.array_equal(got, want)
    assert got_ev == want_ev
    assert_same_state(pump, ref, range(cap))
    pump.close()
    ref.close()


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_packet_refusals_queue_nothing(model, golden, tag):
    """Length 0 or N + 1, a stream listed twice, a stream out of range, an offset that is misaligned, negative or runs past the slot:
    VAD_ERR_ARG, nothing queued, the pending counts unchanged; the next valid tick goes through."""
    from silero_vad_amd import StreamPump, _lib
    sr, g = SRS[tag], golden[tag]
    n = chunk_of(sr)
    pcm = g["pcm_i16"][40 * n:]
    cap = 20
    pump = StreamPump(model.engine, sr, streams=cap, parts=1, ring_slots=2)
    pump.write_packets(0, [(2, pcm[:100])])
    assert pump.poll()[0] == [] and (pump.probs(0) == -1.0).all()
    assert pump.pending(2) == 100 and pump.pending(0) == 0
    for streams, lengths, offsets in (([0], [0], [0]), ([0], [n + 1], [0]), ([1, 1], [8, 8], [0, 8]), ([cap], [8], [0]), ([-1], [8], [0]),
                                      ([0], [8], [4]), ([0], [16], [cap * n - 8]), ([0], [8], [-8]), ([0, 3, 0], [8, 8, 8], [0, 8, 16])):
        with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
            pump.submit_packets(1, streams, lengths, offsets)
        assert pump.poll() == (None, None)
        assert pump.pending(2) == 100 and pump.pending(0) == pump.pending(1) == pump.pending(3) == 0
    # Python-side validation
    for bad in (lambda: pump.write_packets(1, [(0, np.zeros(0, np.int16))]), lambda: pump.write_packets(1, [(0, np.zeros(n + 1, np.int16))]),
                lambda: pump.write_packets(1, [(0, np.zeros(8, np.float32))]), lambda: pump.submit_packets(1, [0, 1], [8]),
                lambda: pump.submit_packets(1, [0.5], [8]), lambda: pump.pending(cap)):
        with pytest.raises(ValueError):
            bad()
    assert pump.poll() == (None, None)
    # the largest valid packet, at the last offset of the slot, completes stream 2's chunk
    area = pump.packet_area(1)
    area[cap * n - n:] = pcm[100:100 + n]
    pump.submit_packets(1, [2], [n], [cap * n - n])
    ev, r = pump.poll()
    p = pump.probs(r)
    assert r == 1 and p[2] >= 0 and (np.delete(p, 2) == -1.0).all() and pump.pending(2) == 100
    ref = StreamPump(model.engine, sr, streams=cap, parts=1, ring_slots=2)
    ref.slot(0)[0] = pcm[:n]
    ref.submit_rows(0, [2])
    ref.poll()
    assert ref.probs(0)[2] == p[2]
    pump.close()
    ref.close()


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_packet_stream_reopened_with_samples_pending_starts_fresh(model, golden, tag):
    """vad_pump_open drops a stream's pending samples: reopened mid-run with samples pending, it gives a fresh stream's probabilities and
    events on the same packets; vad_pump_close drops them too."""
    from silero_vad_amd import StreamPump
    sr, g = SRS[tag], golden[tag]
    n = chunk_of(sr)
    pcm = g["pcm_i16"]
    cap, s0 = 20, 3
    rng = np.random.default_rng(7)
    L = 80 * n
    audio = [np.roll(pcm, -s * 7919)[:L].copy() for s in range(cap)]
    fresh = np.roll(pcm, -123457)[:L].copy()
    plans = [packet_plan(L, n, sr, rng) for _ in range(cap)]
    plan_new = packet_plan(L, n, sr, rng)
    K1 = next(t for t in range(20, len(plans[s0])) if sum(plans[s0][:t]) % n)     # the switch comes with samples pending

    def run(switch):
        pump = StreamPump(model.engine, sr, streams=cap, parts=2, ring_slots=2)
        pos, nxt, probs, events = [0] * cap, [0] * cap, [], []
        for t in range(K1 + len(plan_new) if switch else len(plan_new)):
            if switch and t == K1:
                assert pump.pending(s0) > 0
                pump.open_stream(s0)
                assert pump.pending(s0) == 0
            new = not switch or t >= K1
            pk = []
            done = False
            for s in range(cap):
                if s == s0 and new:
                    i = t - K1 if switch else t
                    a, ln = sum(plan_new[:i]), plan_new[i]
                    pk.append((s, fresh[a:a + ln]))
                    done = (a + ln) // n > a // n
                elif nxt[s] < len(plans[s]):
                    ln = plans[s][nxt[s]]
                    pk.append((s, audio[s][pos[s]:pos[s] + ln]))
                    pos[s] += ln
                    nxt[s] += 1
            pump.write_packets(t % 2, pk)
            ev, r = pump.poll()
            if new and done:
                probs.append(pump.probs(r)[s0])
            if new:
                events += [e for s, e in ev if s == s0]
        pump.close_stream(5)
        assert pump.pending(5) == 0
        pump.close()
        return np.array(probs), events

    got, got_ev = run(True)
    want, want_ev = run(False)
    assert len(got) == L // n and np.array_equal(got, want)
    assert got_ev == want_ev


def test_packets_at_full_capacity(model, oracle, golden):
    """8 192 streams at 16 kHz, 20 ms packets, 64 ticks, each stream on its own phase, rows in random arrival order: every stream equals
    the submit_rows route bit for bit, and eight sampled streams agree with the CPU oracle on their own concatenated audio."""
    from silero_vad_amd import StreamPump
    sr, n, S, P, TT = 16000, 512, 8192, 320, 64
    pcm = golden["16k"]["pcm_i16"]
    origin = (np.arange(S, dtype=np.int64) * 7919) % (len(pcm) - TT * P)
    first = 1 + (np.arange(S) * 37) % P                        # the first packet's length: the streams complete on different ticks
    total = first + (TT - 1) * P
    nchunks = int(total.max()) // n
    rng = np.random.default_rng(13)
    pk_pump = StreamPump(model.engine, sr, streams=S, parts=2, ring_slots=3)
    ref_pump = StreamPump(model.engine, sr, streams=S, parts=2, ring_slots=3)
    got = np.full((S, nchunks), np.nan, np.float32)
    want = np.full((S, nchunks), np.nan, np.float32)
    got_ev, want_ev = [], []
    sent = np.zeros(S, np.int64)
    col = np.arange(P)
    for t in range(TT + 1):
        if t < TT:
            r = t % 3
            ln = first if t == 0 else np.full(S, P)
            order = rng.permutation(S)
            area = pk_pump.packet_area(r)[:S * P].reshape(S, P)
            area[:] = pcm[(origin + sent)[order][:, None] + col[None, :]]
            pk_pump.submit_packets(r, order, ln[order], np.arange(S) * P)
            done = np.flatnonzero((sent + ln) // n > sent // n)
            done = done[rng.permutation(len(done))]
            k = (sent + ln)[done] // n - 1
            slot = ref_pump.slot(r)
            slot[:len(done)] = pcm[(origin[done] + k * n)[:, None] + np.arange(n)[None, :]]
            ref_pump.submit_rows(r, done)
            sent += ln
            batch = (done, k)
        if t > 0:
            for pump, probs, evs in ((pk_pump, got, got_ev), (ref_pump, want, want_ev)):
                ev, rr = pump.poll()
                probs[prev[0], prev[1]] = pump.probs(rr)[prev[0]]
                evs.append(ev)
        if t < TT:
            prev = batch
    assert (sent == total).all()
    for s in range(S):
        assert pk_pump.pending(s) == total[s] % n
    assert not np.isnan(got[:, :int(total.min()) // n]).any()
    assert np.array_equal(got, want, equal_nan=True)
    assert got_ev == want_ev
    assert_same_state(pk_pump, ref_pump, range(S))
    pick = [0, 1, 15, 16, 1000, 4097, 8000, S - 1]
    m = int(total.min()) // n
    x = np.stack([pcm[origin[s]:origin[s] + m * n] for s in pick]).astype(np.float32) / 32768.0
    ref = oracle.audio_forward(x, sr)
    assert np.abs(got[pick, :m] - ref).max() < TIGHT
    pk_pump.close()
    ref_pump.close()
