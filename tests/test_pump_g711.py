"""The pump's G.711 packet route (vad_pump_submit_coded_packets, csrc/pump.hip + kernel_present.hip assemble_coded_packets): telephony
streams deliver mu-law (PCMU) / A-law (PCMA) payloads, 1 byte a sample, and the device expands them to int16 on their way into the
chunk.  The route is defined by reduction to the int16 packet route: every result here is compared, bit for bit, with a second pump fed
the EXPANDED packets (g711_expand) through vad_pump_submit_packets on the same schedule.
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest
import torch

from conftest import SRS

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
CODECS = ("s16", "ulaw", "alaw")


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


def decode(data, law):
    from silero_vad_amd import g711_expand
    return g711_expand(data, law)


def packet_plan(total, n, sr, rng):
    """Packet lengths that cover `total` samples: mostly 10 / 20 / 30 ms frames, the rest uniform in [1, n]."""
    ms10 = sr // 100
    lens, left = [], total
    while left > 0:
        ln = int(rng.choice([ms10, 2 * ms10, 3 * ms10])) if rng.random() < 0.7 else int(rng.integers(1, n + 1))
        ln = min(ln, left)
        lens.append(ln)
        left -= ln
    return lens


def schedule(plans, rng, miss=0.1, empty_every=53):
    """Ticks of (stream, first sample, length) packets in ARRIVAL order: a stream sends its next packet at a tick with probability
    1 - miss, and every `empty_every`-th tick carries no packet at all."""
    cap = len(plans)
    nxt, start = [0] * cap, [0] * cap
    ticks = []
    while any(nxt[s] < len(plans[s]) for s in range(cap)):
        pk = []
        if len(ticks) % empty_every != empty_every - 1:
            for s in range(cap):
                if nxt[s] < len(plans[s]) and rng.random() >= miss:
                    ln = plans[s][nxt[s]]
                    pk.append((s, start[s], ln))
                    start[s] += ln
                    nxt[s] += 1
        ticks.append([pk[i] for i in rng.permutation(len(pk))])
    return ticks


class Pair:
    """The pump under test and its reference, driven in lock step: a coded tick goes to the first as it is and to the second
    expanded, through write_packets; every other call goes to both.  Each retired tick's probabilities and events must be equal."""

    def __init__(self, model, sr, cap, **kw):
        from silero_vad_amd import StreamPump
        self.got = StreamPump(model.engine, sr, streams=cap, **kw)
        self.ref = StreamPump(model.engine, sr, streams=cap, **kw)
        self.n, self.cap = self.got.n, cap
        self.events = 0
        self.stepped = 0

    def coded(self, r, packets):
        """packets: [(stream, codes or int16, codec), ...]"""
        self.got.write_coded_packets(r, packets)
        self.ref.write_packets(r, [(s, decode(x, c)) for s, x, c in packets])

    def both(self, fn):
        fn(self.got)
        fn(self.ref)

    def retire(self):
        (ev, r), (ev_ref, r_ref) = self.got.poll(), self.ref.poll()
        assert r == r_ref
        p, q = self.got.probs(r), self.ref.probs(r)
        assert np.array_equal(p, q)
        assert ev == ev_ref
        self.events += len(ev)
        self.stepped += int((p >= 0).sum())
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


@pytest.mark.parametrize("law", ["ulaw", "alaw"])
@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_coded_packets_equal_the_expanded_int16_route(model, golden, tag, law):
    """100 streams of G.711-encoded speech (~20 s each), packets of 10 / 20 / 30 ms and uniform lengths in [1, N], ~10 % of ticks
    without a packet, empty ticks, rows in random arrival order, two ticks in flight: probabilities, events, final (h, c, context) and
    the pending residue equal the int16 packet route fed the expanded packets."""
    sr = SRS[tag]
    n = chunk_of(sr)
    pcm = golden[tag]["pcm_i16"]
    cap, L = 100, 20 * sr
    rng = np.random.default_rng(17)
    audio = [encode(np.roll(pcm, -s * 7919)[:L - int(rng.integers(0, n))], law) for s in range(cap)]
    ticks = schedule([packet_plan(len(a), n, sr, rng) for a in audio], rng)
    assert sum(1 for pk in ticks if not pk) >= 2
    pair = Pair(model, sr, cap, parts=3, ring_slots=3)
    for t in range(len(ticks) + 1):
        if t < len(ticks):
            pair.coded(t % 3, [(s, audio[s][a:a + ln], law) for s, a, ln in ticks[t]])
        if t > 0:
            pair.retire()
    pair.finish()
    assert pair.stepped == sum(len(a) // n for a in audio) and pair.events > 100
    for s in range(cap):
        assert pair.got.pending(s) == len(audio[s]) % n, s
    pair.close()


@pytest.mark.parametrize("law", ["ulaw", "alaw"])
def test_every_code_through_the_device(model, law):
    """8 kHz (N = 256, C = 32): 8 streams each send one 256-byte packet whose last 32 codes together cover all 256 codes of the law;
    each stream's carried context (the chunk's last C samples, read as int16 / 32768) is exactly the expansion of its codes."""
    from silero_vad_amd import StreamPump, g711_expand
    n, C, S = 256, 32, 8
    rng = np.random.default_rng(5)
    codes = rng.permutation(256).astype(np.uint8)
    pump = StreamPump(model.engine, 8000, streams=S, parts=1, ring_slots=2)
    packets = []
    for s in range(S):
        x = rng.integers(0, 256, n).astype(np.uint8)
        x[n - C:] = codes[s * C:(s + 1) * C]
        packets.append((s, x, law))
    pump.write_coded_packets(0, packets[::-1])
    _, r = pump.poll()
    assert (pump.probs(r) >= 0).all()
    for s in range(S):
        assert pump.pending(s) == 0
        ctx = pump.state(s)[2]
        want = g711_expand(codes[s * C:(s + 1) * C], law).astype(np.float32) / np.float32(32768.0)
        assert np.array_equal(ctx, want), s
    pump.close()


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_codecs_mix(model, golden, tag):
    """Rows of all three formats in one tick; streams that change format mid-chunk, with the change inside a pending carry; coded
    ticks interleaved with int16 submit_packets ticks and with chunk ticks (submit_rows, masked, compact, full) for streams with
    nothing pending; open / close of streams with samples pending.  Every tick equals the reference pump fed expanded int16."""
    sr = SRS[tag]
    n = chunk_of(sr)
    pcm = golden[tag]["pcm_i16"]
    cap, K = 40, 36
    rows = np.ascontiguousarray(np.stack([np.roll(pcm, -(30 * n + s * 7919))[:K * n] for s in range(cap)]))
    rng = np.random.default_rng(23)
    pair = Pair(model, sr, cap, parts=2, ring_slots=2)
    k = np.zeros(cap, np.int64)
    mixed = switched = reopened = 0
    for cycle in range(K):
        # a coded tick: each stream sends its next chunk whole, or its first part (the rest follows next tick), in a random format
        split, pk = {}, []
        for s in rng.permutation(cap):
            if k[s] >= K or rng.random() < 0.15:
                continue
            chunk = rows[s, k[s] * n:(k[s] + 1) * n]
            c = CODECS[int(rng.integers(0, 3))]
            if rng.random() < 0.4:
                pk.append((s, encode(chunk, c), c))
                k[s] += 1
            else:
                a = int(rng.integers(1, n))
                pk.append((s, encode(chunk[:a], c), c))
                split[s] = (chunk[a:], c)
                k[s] += 1
        mixed += len({c for _, _, c in pk}) == 3
        pair.coded(0, pk)
        pair.retire()
        if cycle == 5 and len(split) >= 2:                     # open / close with samples pending: both drop them
            s0, s1 = list(split)[:2]
            assert pair.got.pending(s0) > 0 and pair.got.pending(s1) > 0
            pair.both(lambda p: p.open_stream(s0))
            pair.both(lambda p: p.close_stream(s1))
            assert pair.got.pending(s0) == pair.got.pending(s1) == 0
            del split[s0], split[s1]
            reopened += 1
        # the rest: in another format (the change lands in the pending carry), as a coded tick or as an int16 submit_packets tick
        if split:
            if cycle % 3 == 2:
                pair.both(lambda p: p.write_packets(1, [(s, x) for s, (x, _) in split.items()]))
            else:
                rest = []
                for s, (x, c0) in split.items():
                    c = CODECS[(CODECS.index(c0) + 1 + int(rng.integers(0, 2))) % 3]
                    rest.append((s, encode(x, c), c))
                    switched += 1
                pair.coded(1, rest)
            pair.retire()
        assert all(pair.got.pending(s) == 0 for s in range(cap))
        # a chunk tick for streams with nothing pending, by a route that changes from cycle to cycle
        route = cycle % 4
        on = np.flatnonzero(k < K) if route == 0 else np.flatnonzero((k < K) & (rng.random(cap) < 0.6))
        if route == 0 and len(on) < cap:
            route = 1
        if route == 3:
            on = rng.permutation(on)
        for p in (pair.got, pair.ref):
            slot = p.slot(0)
            for i, s in enumerate(on):
                slot[i if route >= 2 else s] = rows[s, k[s] * n:(k[s] + 1) * n]
        k[on] += 1
        fl = np.zeros(cap, np.uint8)
        fl[on] = 1
        if route == 0:
            pair.both(lambda p: p.submit(0))
        elif route == 3:
            pair.both(lambda p: p.submit_rows(0, on))
        else:
            pair.both(lambda p: p.submit(0, present=fl, compact=route == 2))
        pair.retire()
    assert mixed > 0 and switched > 20 and reopened == 1
    pair.finish()
    assert pair.events > 10
    pair.close()


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_coded_refusals_queue_nothing(model, golden, tag):
    """A bad codec, a byte offset of 8, a G.711 or S16 row one byte / one sample past the slot, a stream listed twice, length 0 or
    N + 1: VAD_ERR_ARG, nothing queued, the pending counts unchanged.  An S16 row at a 16-byte offset that is not a multiple of 16
    samples and a G.711 row ending exactly at the slot's last byte are accepted; the pump then equals the reference."""
    from silero_vad_amd import _lib
    sr = SRS[tag]
    n = chunk_of(sr)
    pcm = golden[tag]["pcm_i16"][40 * n:]
    cap = 20
    end = cap * n * 2                                           # bytes in a slot's sample area
    pair = Pair(model, sr, cap, parts=1, ring_slots=2)
    ul = encode(pcm[:4 * n], "ulaw")
    pair.coded(0, [(2, ul[:100], "ulaw")])
    pair.retire()
    assert pair.got.pending(2) == 100 and pair.got.pending(0) == 0
    pump = pair.got
    for streams, lengths, codecs, offsets in (([0], [8], [3], [0]), ([0], [8], [1], [8]), ([0], [17], [1], [end - 16]),
                                              ([0], [9], [0], [end - 16]), ([1, 1], [8, 8], [1, 2], [0, 16]), ([0], [0], [1], [0]),
                                              ([0], [n + 1], [1], [0]), ([cap], [8], [1], [0]), ([0], [8], [1], [-16]),
                                              ([0, 3, 0], [8, 8, 8], [0, 1, 2], [0, 16, 32])):
        with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
            pump.submit_coded_packets(1, streams, lengths, np.array(codecs, np.uint8), offsets)
        assert pump.poll() == (None, None)
        assert pump.pending(2) == 100 and pump.pending(0) == pump.pending(1) == pump.pending(3) == 0
    for bad in (lambda: pump.write_coded_packets(1, [(0, np.zeros(8, np.int16), "ulaw")]),
                lambda: pump.write_coded_packets(1, [(0, np.zeros(8, np.uint8), "s16")]),
                lambda: pump.write_coded_packets(1, [(0, np.zeros(8, np.uint8), "pcmu")]),
                lambda: pump.write_coded_packets(1, [(0, np.zeros(0, np.uint8), "alaw")]),
                lambda: pump.write_coded_packets(1, [(0, np.zeros(n + 1, np.uint8), "alaw")]),
                lambda: pump.submit_coded_packets(1, [0, 1], [8, 8], ["ulaw"]),
                lambda: pump.submit_coded_packets(1, [0], [8], ["mp3"])):
        with pytest.raises(ValueError):
            bad()
    assert pump.poll() == (None, None)
    # accepted: stream 2's rest of a chunk as ONE G.711 row ending at the slot's last byte, stream 3 S16 at byte 48 (sample 24),
    # stream 5 A-law at byte 144
    rest = ul[100:100 + n]
    s16 = pcm[7 * n:7 * n + 40]
    al = encode(pcm[9 * n:9 * n + 33], "alaw")
    area = pump.packet_bytes(1)
    area[end - n:] = rest
    area[48:48 + 80] = s16.view(np.uint8)
    area[144:144 + 33] = al
    pump.submit_coded_packets(1, [3, 2, 5], [40, n, 33], ["s16", "ulaw", "alaw"], [48, end - n, 144])
    pair.ref.write_packets(1, [(3, s16), (2, decode(rest, "ulaw")), (5, decode(al, "alaw"))])
    p, _ = pair.retire()
    assert p[2] >= 0 and (np.delete(p, 2) == -1.0).all()
    assert pump.pending(2) == 100 and pump.pending(3) == 40 and pump.pending(5) == 33
    # codecs=None: every row S16 (== submit_packets with the offsets in bytes)
    pump.packet_bytes(0)[32:32 + 2 * (n - 40)] = pcm[11 * n:12 * n - 40].view(np.uint8)
    pump.submit_coded_packets(0, [3], [n - 40], None, [32])
    pair.ref.write_packets(0, [(3, pcm[11 * n:12 * n - 40])])
    p, _ = pair.retire()
    assert p[3] >= 0 and pump.pending(3) == 0
    pair.finish()
    pair.close()


def test_coded_packets_at_full_capacity(model, oracle, golden):
    """8 192 streams at 8 kHz, 20 ms PCMU packets (160 bytes), 64 ticks, each stream on its own phase, rows in random arrival order:
    bit-equal to the int16 packet route fed the expanded packets, and eight sampled streams agree with the CPU oracle on their
    expanded audio."""
    from silero_vad_amd import StreamPump
    sr, n, S, P, TT = 8000, 256, 8192, 160, 64
    codes = encode(golden["8k"]["pcm_i16"], "ulaw")
    lin = decode(codes, "ulaw")
    origin = (np.arange(S, dtype=np.int64) * 7919) % (len(codes) - TT * P)
    first = 1 + (np.arange(S) * 37) % P                        # the first packet's length: the streams complete on different ticks
    total = first + (TT - 1) * P
    nchunks = int(total.max()) // n
    rng = np.random.default_rng(29)
    got_pump = StreamPump(model.engine, sr, streams=S, parts=2, ring_slots=3)
    ref_pump = StreamPump(model.engine, sr, streams=S, parts=2, ring_slots=3)
    got = np.full((S, nchunks), np.nan, np.float32)
    want = np.full((S, nchunks), np.nan, np.float32)
    got_ev, want_ev = [], []
    sent = np.zeros(S, np.int64)
    col = np.arange(P)
    offsets = (np.arange(S) * P).astype(np.int32)              # P bytes of codes / P samples of int16: both 16-byte aligned
    for t in range(TT + 1):
        if t < TT:
            r = t % 3
            ln = first if t == 0 else np.full(S, P)
            order = rng.permutation(S)
            idx = (origin + sent)[order][:, None] + col[None, :]
            got_pump.packet_bytes(r)[:S * P].reshape(S, P)[:] = codes[idx]
            got_pump.submit_coded_packets(r, order, ln[order], np.ones(S, np.uint8), offsets)
            ref_pump.packet_area(r)[:S * P].reshape(S, P)[:] = lin[idx]
            ref_pump.submit_packets(r, order, ln[order], offsets)
            done = np.flatnonzero((sent + ln) // n > sent // n)
            batch = (done, (sent + ln)[done] // n - 1)
            sent += ln
        if t > 0:
            for pump, probs, evs in ((got_pump, got, got_ev), (ref_pump, want, want_ev)):
                ev, rr = pump.poll()
                probs[prev[0], prev[1]] = pump.probs(rr)[prev[0]]
                evs.append(ev)
        if t < TT:
            prev = batch
    assert (sent == total).all()
    for s in range(S):
        assert got_pump.pending(s) == ref_pump.pending(s) == total[s] % n
    assert not np.isnan(got[:, :int(total.min()) // n]).any()
    assert np.array_equal(got, want, equal_nan=True)
    assert got_ev == want_ev
    for s in range(S):
        for x, y in zip(got_pump.state(s), ref_pump.state(s)):
            assert np.array_equal(x, y), s
    pick = [0, 1, 15, 16, 1000, 4097, 8000, S - 1]
    m = int(total.min()) // n
    x = np.stack([lin[origin[s]:origin[s] + m * n] for s in pick]).astype(np.float32) / 32768.0
    ref = oracle.audio_forward(x, sr)
    assert np.abs(got[pick, :m] - ref).max() < TIGHT
    got_pump.close()
    ref_pump.close()
