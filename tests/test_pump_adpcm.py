"""The pump's DVI4 rows (VAD_PCM_DVI4 on vad_pump_submit_coded_packets and vad_pump_submit_burst; csrc/pump.hip + kernel_present.hip
assemble_adpcm_packets and the ADPCM form of assemble_burst): RFC 3551 4-bit IMA ADPCM payloads, header included, decoded on the device
by two wave scans.  The routes are defined by reduction: every result here is compared, bit for bit, with a second pump that is fed
`adpcm_expand` of each payload as int16 on the same schedule (bursts: with the chunk route fed the concatenated audio), and the decoded
samples themselves are read back from the tape and from a snapshot's pending samples.
Speech comes from the golden recordings -- 16 kHz [0, 6 s), 8 kHz [20 s, 26 s), further streams a little later -- through the plain IMA
encoder of tests/adpcm_codec.py, whose state in front of a packet is that packet's header.
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest
import torch

import adpcm_codec as ima
from conftest import SRS

pytestmark = pytest.mark.gpu

CODECS = ("s16", "ulaw", "alaw", "dvi4")
FIRST = {"16k": 0, "8k": 20 * 8000}                      # where the stretch starts in the golden recording
LAG = 1237                                               # stream s starts s * LAG samples into the stretch
MAX_STREAMS = 9


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
    """tag -> (pcm, Encoded) of the stretch, encoded once and never changed; stream s of a test reads it from s * LAG on."""
    made = {}

    def of(tag):
        if tag not in made:
            sr = SRS[tag]
            pcm = np.ascontiguousarray(golden[tag]["pcm_i16"][FIRST[tag]:FIRST[tag] + 6 * sr + MAX_STREAMS * LAG])
            assert len(pcm) == 6 * sr + MAX_STREAMS * LAG
            made[tag] = (pcm, ima.Encoded(pcm))
        return made[tag]
    return of


def chunk_of(sr):
    return 512 if sr == 16000 else 256


def g711_encode(pcm, law):
    """int16 -> the G.711 code whose expansion is nearest (ties to the lower value)."""
    from silero_vad_amd import g711_expand
    codes = np.arange(256, dtype=np.uint8)
    lin = g711_expand(codes, law).astype(np.int32)
    order = np.argsort(lin, kind="stable")
    v = lin[order]
    x = pcm.astype(np.int32)
    j = np.clip(np.searchsorted(v, x), 1, len(v) - 1)
    j -= (x - v[j - 1]) <= (v[j] - x)
    return codes[order[j]]


def row_of(speech_tag, s, a, ln, codec):
    """Samples [a, a + ln) of stream s in format `codec`, as the coded routes take them."""
    pcm, enc = speech_tag
    at = s * LAG + a
    if codec == "dvi4":
        return enc.packet(at, ln)
    return pcm[at:at + ln] if codec == "s16" else g711_encode(pcm[at:at + ln], codec)


def expanded(x, codec):
    """What the reference pump is fed for a row: int16, by the host twins."""
    from silero_vad_amd import adpcm_expand, g711_expand
    if isinstance(x, (int, np.integer)):
        return x                                            # a silent row
    return adpcm_expand(x) if codec == "dvi4" else x if codec == "s16" else g711_expand(x, codec)


def kinds(events):
    return {k for _, e in events for k in e}


class Pair:
    """The pump under test and its reference in lock step: a coded tick goes to the first as it is and to the second expanded,
    through write_packets.  Each retired tick's probabilities and events, and every stream's (h, c, context) and pending count after
    it, must be equal."""

    def __init__(self, model, sr, cap, **kw):
        from silero_vad_amd import StreamPump
        self.got = StreamPump(model.engine, sr, streams=cap, **kw)
        self.ref = StreamPump(model.engine, sr, streams=cap, **kw)
        self.n, self.cap = self.got.n, cap
        self.ref_events = []
        self.stepped = 0

    def coded(self, r, packets):
        self.got.write_coded_packets(r, packets)
        self.ref.write_packets(r, [(s, expanded(x, c)) for s, x, c in packets])

    def retire(self):
        (ev, r), (ev_ref, r_ref) = self.got.poll(), self.ref.poll()
        assert r == r_ref
        p, q = self.got.probs(r), self.ref.probs(r)
        assert np.array_equal(p, q)
        assert ev == ev_ref
        self.ref_events += ev_ref
        self.stepped += int((q >= 0).sum())
        self.same_streams()
        return p

    def same_streams(self):
        for s in range(self.cap):
            assert self.got.pending(s) == self.ref.pending(s), s
            for x, y in zip(self.got.state(s), self.ref.state(s)):
                assert np.array_equal(x, y), s

    def close(self):
        assert self.got.poll() == (None, None) and self.ref.poll() == (None, None)
        self.got.close()
        self.ref.close()


def mixed_schedule(sr, n, cap, rng):
    """-> (ticks of (stream, first sample, length, codec, silent) rows in arrival order, each stream's samples): a stream sends its next
    packet at a tick with probability 0.9, every 53rd tick is empty, every length is even."""
    ms10 = sr // 100
    nxt, ticks = [0] * cap, []
    total = [6 * sr - 2 * int(rng.integers(0, n // 2)) for _ in range(cap)]
    while any(nxt[s] < total[s] for s in range(cap)):
        rows = []
        if len(ticks) % 53 != 52:
            for s in rng.permutation(cap).tolist():
                if nxt[s] >= total[s] or rng.random() < 0.1:
                    continue
                ln = int(rng.choice([ms10, 2 * ms10, 3 * ms10])) if rng.random() < 0.7 else 2 * int(rng.integers(1, n // 2 + 1))
                ln = min(ln, total[s] - nxt[s])
                rows.append((s, nxt[s], ln, CODECS[int(rng.integers(0, 4))], bool(rng.random() < 0.04)))
                nxt[s] += ln
        ticks.append(rows)
    return ticks, total


def burst_schedule(sr, n, cap, M, rng):
    """-> ticks of (stream, first sample, length, codec) rows: up to four rows of a stream in a tick -- DVI4 rows of 60 ms, of 2 N + 6
    samples and of a short even length, S16 / G.711 rows below N / 2 --, as long as the stream completes at most M chunks, the rows fit
    the slot and the stream has audio left."""
    area, sent, ticks = cap * n * 2, [0] * cap, []
    while min(sent) < 6 * sr - 5 * n and len(ticks) < 400:
        rows, room = [], area
        for s in rng.permutation(cap).tolist():
            if rng.random() < 0.15:
                continue
            c = sent[s] % n
            for _ in range(int(rng.integers(1, 5))):
                kind = int(rng.integers(0, 6))
                codec = "dvi4" if kind < 3 else CODECS[kind - 3]
                ln = (sr * 60 // 1000, 2 * n + 6, 2 * int(rng.integers(1, n // 2 + 1)))[kind] if kind < 3 else int(rng.integers(1, n // 2))
                size = (4 + ln // 2 if codec == "dvi4" else 2 * ln if codec == "s16" else ln) + 15 & ~15
                if c + ln >= (M + 1) * n or size > room or sent[s] + ln > 6 * sr or len(rows) == cap:      # (a tick holds `streams` rows)
                    break
                rows.append((s, sent[s], ln, codec))
                sent[s] += ln
                c += ln
                room -= size
        ticks.append(rows)
    return ticks


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_mixed_schedule_equals_the_expanded_int16_route(model, speech, tag):
    """7 streams of 6 s each: packets of 10 / 20 / 30 ms or of a random even length 2 ... N, each in a format drawn afresh from s16 /
    ulaw / alaw / dvi4 (a stream changes format from packet to packet, inside a pending carry too), ~10 % of the packets a tick late,
    empty ticks, ~4 % of the rows silent, rows in random arrival order, two ticks in flight."""
    sr = SRS[tag]
    n = chunk_of(sr)
    sp = speech(tag)
    cap = 7
    plan, total = mixed_schedule(sr, n, cap, np.random.default_rng(351))
    ticks = [[(s, ln if quiet else row_of(sp, s, a, ln, codec), codec) for s, a, ln, codec, quiet in rows] for rows in plan]
    used = {c: sum(codec == c and not quiet for rows in plan for _, _, _, codec, quiet in rows) for c in CODECS}
    assert min(used.values()) > 50 and sum(quiet for rows in plan for *_, quiet in rows) > 10 and sum(1 for rows in plan if not rows) >= 2
    assert any(len({codec for _, _, _, codec, quiet in rows if not quiet}) == 4 for rows in plan)
    pair = Pair(model, sr, cap, parts=2, ring_slots=3, adpcm=True)
    for t in range(len(ticks) + 1):
        if t < len(ticks):
            pair.coded(t % 3, ticks[t])
        if t > 0:
            pair.retire()
    assert pair.stepped == sum(x // n for x in total)
    assert {"start", "end"} <= kinds(pair.ref_events)
    for s in range(cap):
        assert pair.got.pending(s) == total[s] % n, s
    pair.close()


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_decoded_samples_on_the_tape(model, tag):
    """8 streams fed DVI4 only, behind one S16 packet of 1 ... 8 samples that leaves each with another pending count mod 8 (odd ones
    included): lengths 2, 6, 8, 10, 14, 16, 18, 62, 64, 66, N - 2 and N with random codes and headers, then the saturating, index-floor
    and header-index payloads at N and at 66 samples.  The tape's audio is the concatenated `adpcm_expand` of the payloads, sample for
    sample; the residue below a chunk is read from a snapshot."""
    from silero_vad_amd import StreamPump, adpcm_expand, snapshot_info
    sr = SRS[tag]
    n = chunk_of(sr)
    S, K = 8, 32
    rng = np.random.default_rng(45)
    pump = StreamPump(model.engine, sr, streams=S, parts=1, ring_slots=2, tape_chunks=K, adpcm=True)
    want = [np.zeros(0, np.int16) for _ in range(S)]
    residues, t = set(), 0

    def tick(rows):
        nonlocal t
        for s, x, c in rows:
            if c == "dvi4":
                residues.add(pump.pending(s) % 8)
            want[s] = np.concatenate([want[s], expanded(x, c)])
        pump.write_coded_packets(t % 2, rows)
        _, r = pump.poll()
        assert r == t % 2
        t += 1

    tick([(s, rng.integers(-32768, 32768, s + 1).astype(np.int16), "s16") for s in range(S)])
    lens = [2, 6, 8, 10, 14, 16, 18, 62, 64, 66, n - 2, n]
    for i in range(len(lens)):
        rows = []
        for s in range(S):
            ln = lens[(i + s) % len(lens)]
            rows.append((s, ima.payload(int(rng.integers(-32768, 32768)), int(rng.integers(0, 89)), rng.integers(0, 16, ln)), "dvi4"))
        tick(rows[::-1])
    for n_codes in (n, 66):
        special = list(ima.special_payloads(n_codes).values())
        for i in range(len(special)):
            tick([(s, special[(i + s) % len(special)], "dvi4") for s in range(S)])
    assert residues == set(range(8))
    assert pump.poll() == (None, None)
    done = [len(w) // n for w in want]
    assert max(done) < K and min(done) > 12
    audios, first = pump.fetch_audio(list(range(S)), [0] * S, [d * n for d in done])
    assert first.tolist() == [0] * S
    info = snapshot_info(pump.export_streams(list(range(S))))
    for s in range(S):
        assert pump.tape_state(s) == (done[s], 0)
        assert np.array_equal(audios[s], want[s][:done[s] * n]), s
        left = len(want[s]) - done[s] * n
        assert info[s]["pending"] == pump.pending(s) == left
        assert np.array_equal(info[s]["pending_samples"][:left], want[s][done[s] * n:]), s
    assert sum(len(w) % n > 0 for w in want) >= 6 and {len(w) % 2 for w in want} == {0, 1}
    pump.close()


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_bursts_equal_the_chunk_route(model, speech, tag):
    """max_burst = 4: DVI4 rows of 60 ms (960 samples at 16 kHz), of 2 N + 6 samples and of short even lengths, up to four rows of a
    stream in a tick beside S16 and G.711 rows.  A row longer than N is decoded in pieces, the decoder's state carried across the piece
    boundary.  Compared with a pump without bursts that is fed the same audio -- every row through its host twin -- chunk by chunk
    through submit_rows, one tick per sub-step, and with the tape."""
    from silero_vad_amd import StreamPump
    sr = SRS[tag]
    n = chunk_of(sr)
    sp = speech(tag)
    cap, M = 6, 4
    plan = burst_schedule(sr, n, cap, M, np.random.default_rng(77))
    got = StreamPump(model.engine, sr, streams=cap, parts=1, ring_slots=2, max_burst=M, tape_chunks=6 * sr // n + 2, adpcm=True)
    ref = StreamPump(model.engine, sr, streams=cap, parts=1, ring_slots=2)
    sent = np.zeros(cap, np.int64)                        # samples of each stream submitted so far
    audio = [np.zeros(0, np.int16) for _ in range(cap)]
    long_rows = mixed_ticks = deepest = 0
    got_events, ref_events = [], []
    for t, listed in enumerate(plan):
        rows, new = [(s, row_of(sp, s, a, ln, codec), codec) for s, a, ln, codec in listed], np.zeros(cap, np.int64)
        for s, _, ln, codec in listed:
            new[s] += ln
            long_rows += codec == "dvi4" and ln > n
        mixed_ticks += len({c for _, _, c in rows}) >= 3 and any(sum(1 for q, _, _ in rows if q == s) >= 2 for s in range(cap))
        got.write_burst(t % 2, rows)
        for s, x, c in rows:
            audio[s] = np.concatenate([audio[s], expanded(x, c)])
        k = (sent % n + new) // n
        ev, r = got.poll()
        steps = max(1, int(k.max()))
        deepest = max(deepest, steps)
        assert r == t % 2 and got.burst_steps(r) == steps
        bp = got.burst_probs(r)
        got_events += ev
        for j in range(steps):                              # the reference: sub-step j is one chunk tick of the streams with k > j
            on = np.flatnonzero(k > j)
            for i, s in enumerate(on):
                a = (sent[s] // n + j) * n
                ref.slot(0)[i] = audio[s][a:a + n]
            ref.submit_rows(0, on)
            ev_ref, _ = ref.poll()
            ref_events += ev_ref
            assert np.array_equal(bp[j][on], ref.probs(0)[on]) and (np.delete(bp[j], on) == -1.0).all(), (t, j)
        sent += new
        assert got_events == ref_events
        for s in range(cap):
            assert got.pending(s) == sent[s] % n
            for x, y in zip(got.state(s), ref.state(s)):
                assert np.array_equal(x, y), (t, s)
    assert long_rows > 20 and mixed_ticks > 5 and deepest == M
    assert {"start", "end"} <= kinds(ref_events)
    done = [int(x // n) for x in sent]
    audios, first = got.fetch_audio(list(range(cap)), [0] * cap, [d * n for d in done])
    for s in range(cap):
        assert first[s] == 0 and done[s] > 20 and np.array_equal(audios[s], audio[s][:done[s] * n]), s
    got.close()
    ref.close()


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_refusals_queue_nothing(model, speech, tag):
    """An odd length, length 0, a length above N on the packet route, a row whose 4 + len / 2 bytes run past the slot, codec 4 -- on the
    packet route and in a burst --, and codec 3 while DVI4 rows are switched off: VAD_ERR_ARG, nothing queued, the pending counts
    unchanged; the valid tick behind them, with a row that ends on the slot's last byte, matches the reference."""
    from silero_vad_amd import _lib
    sr = SRS[tag]
    n = chunk_of(sr)
    sp = speech(tag)
    cap = 8
    end = cap * n * 2
    pair = Pair(model, sr, cap, parts=1, ring_slots=2, max_burst=4, adpcm=True)
    pair.coded(0, [(2, row_of(sp, 2, 0, 100, "dvi4"), "dvi4"), (5, row_of(sp, 5, 0, 7, "s16"), "s16")])
    pair.retire()
    pump = pair.got
    held = [pump.pending(s) for s in range(cap)]
    assert held[2] == 100 and held[5] == 7 and sum(held) == 107
    bad = [([0], [7], [3], [0]), ([0], [0], [3], [0]), ([0], [n + 2], [3], [0]), ([0], [32], [3], [end - 16]), ([0], [8], [4], [0]),
           ([1, 0], [8, 9], [3, 3], [0, 16]), ([0], [2 * n], [3], [end - n])]
    for streams, lengths, codecs, offsets in bad:
        with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
            pump.submit_coded_packets(1, streams, lengths, np.array(codecs, np.uint8), offsets)
        assert pump.poll() == (None, None) and [pump.pending(s) for s in range(cap)] == held
    burst_bad = [([0], [7], [3], [0]), ([0], [0], [3], [0]), ([0], [32], [3], [end - 16]), ([0], [8], [4], [0]),
                 ([0, 0], [2 * n, 2 * n + 1], [3, 3], [0, 512]), ([0], [5 * n], [3], [0])]
    for streams, lengths, codecs, offsets in burst_bad:
        with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
            pump.submit_burst(1, streams, lengths, np.array(codecs, np.uint8), offsets)
        assert pump.poll() == (None, None) and [pump.pending(s) for s in range(cap)] == held
    for wrong in (lambda: pump.write_coded_packets(1, [(0, np.zeros(4, np.uint8), "dvi4")]),
                  lambda: pump.write_coded_packets(1, [(0, np.zeros(4 + n // 2 + 1, np.uint8), "dvi4")]),
                  lambda: pump.write_coded_packets(1, [(0, np.zeros(8, np.int16), "dvi4")]),
                  lambda: pump.write_burst(1, [(0, np.zeros(3, np.uint8), "dvi4")])):
        with pytest.raises(ValueError):
            wrong()
    assert pump.poll() == (None, None) and [pump.pending(s) for s in range(cap)] == held
    # DVI4 rows are an opt-in: switched off, the same pump refuses a valid row as a bad codec, on both routes, and so does the packer
    pump.set_adpcm(False)
    for submit in (pump.submit_coded_packets, pump.submit_burst):
        with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
            submit(1, [0], [24], np.array([3], np.uint8), [0])
        assert pump.poll() == (None, None) and [pump.pending(s) for s in range(cap)] == held
    with pytest.raises(ValueError):
        pump.write_coded_packets(1, [(0, row_of(sp, 0, 0, 24, "dvi4"), "dvi4")])
    pump.set_adpcm(True)
    # the valid tick on the slot the refusals named: stream 2 completes its chunk, stream 0's 24 samples (16 bytes) end on the slot's
    # last byte, stream 5 (7 pending, an odd carry) gets a DVI4 row behind its S16 samples
    rest, tail, odd = row_of(sp, 2, 100, n - 100, "dvi4"), row_of(sp, 0, 0, 24, "dvi4"), row_of(sp, 5, 7, 66, "dvi4")
    area = pump.packet_bytes(1)
    area[:len(rest)] = rest
    area[end - 16:] = tail
    area[1024:1024 + len(odd)] = odd
    pump.submit_coded_packets(1, [0, 2, 5], [24, n - 100, 66], ["dvi4", "dvi4", "dvi4"], [end - 16, 0, 1024])
    pair.ref.write_packets(1, [(0, expanded(tail, "dvi4")), (2, expanded(rest, "dvi4")), (5, expanded(odd, "dvi4"))])
    p = pair.retire()
    assert p[2] >= 0 and (np.delete(p, 2) == -1.0).all()
    assert pump.pending(0) == 24 and pump.pending(2) == 0 and pump.pending(5) == 73
    pair.close()


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_snapshot_mid_chunk_continues_elsewhere(model, speech, tag):
    """6 streams fed 20 ms DVI4 packets for 3 s, exported with samples pending, imported into other slots of a second pump: both pumps
    then take the next 3 s and agree on every probability, event, (h, c, context) and pending count."""
    from silero_vad_amd import StreamPump
    sr = SRS[tag]
    n = chunk_of(sr)
    sp = speech(tag)
    cap, P = 6, sr // 50
    a = StreamPump(model.engine, sr, streams=cap, parts=1, ring_slots=2, adpcm=True)
    b = StreamPump(model.engine, sr, streams=cap + 2, parts=2, ring_slots=2, adpcm=True)
    dest = [7, 0, 3, 5, 2, 6]
    half = 3 * sr // P

    def rows(t, slots):
        return [(slots[s], row_of(sp, s, t * P, P, "dvi4"), "dvi4") for s in range(cap) if (t + s) % 11]

    for t in range(half):
        a.write_coded_packets(t % 2, rows(t, list(range(cap))))
        a.poll()
    pending = [a.pending(s) for s in range(cap)]
    assert sum(x > 0 for x in pending) >= 4 and len(set(pending)) > 1
    b.import_streams(a.export_streams(list(range(cap))), dest)
    back = {d: s for s, d in enumerate(dest)}
    events = []
    for t in range(half, 2 * half):
        a.write_coded_packets(t % 2, rows(t, list(range(cap))))
        b.write_coded_packets(t % 2, rows(t, dest))
        (ev_a, r), (ev_b, _) = a.poll(), b.poll()
        assert np.array_equal(a.probs(r), b.probs(r)[dest])
        assert ev_a == sorted((back[d], e) for d, e in ev_b)
        events += ev_a
    assert {"start", "end"} <= kinds(events)
    for s in range(cap):
        assert a.pending(s) == b.pending(dest[s])
        for x, y in zip(a.state(s), b.state(dest[s])):
            assert np.array_equal(x, y), s
    a.close()
    b.close()
