"""Blob version 3 of the pump's snapshots (vad_pump_export_streams_v3 / vad_pump_import_streams, kernel_snapshot.hip
snapshot_tape_gather / snapshot_tape_scatter): a stream that migrates takes the audio of the utterance it is in along, so the tape of
the destination answers for sample numbers from before the move.  The yardsticks are the audio that was fed -- the int16 samples, or
(float)x / 32768 of them, exact -- and an UNINTERRUPTED twin pump; everything is compared bit for bit, floats as uint32 views.
The pumps have 32 slots in two parts of one 16-stream tile each (a part is whole tiles, so two parts need more than 16 slots) and carry
six live streams, three in each part, one tick at a time over ring_slots=2; at most 12 ticks a pump, but for the utterance test, which
plays the speech fixture through.
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import numpy as np
import pytest

from test_pump_resample_gpu import model, speech  # noqa: F401  (the module fixtures)
from test_pump_snapshot_v2 import EDGE_LISTS, edge_pump, edge_records_hold

pytestmark = pytest.mark.gpu

CAP = 32
SRC = [1, 3, 6, 17, 20, 30]                              # live stream i of the source and of the twin; three in each part
DST = [18, 30, 16, 2, 0, 11]                             # ... of a destination: other numbers, every stream in the other part
TICKS, CUT = 12, 8
FAR = 2 ** 62
HEADER3 = 128


def chunk_of(sr):
    return 512 if sr == 16000 else 256


def strides(sr):
    n = chunk_of(sr)
    s2 = 32 + 4 * (256 + n // 8) + 2 * n + 32 + 4 * n + 320
    return s2, s2 + 32


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def same(a, b):
    a, b = bits(a), bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool((a == b).all())


def heard(x, dtype):
    """what the tape holds of the int16 samples x"""
    return x if dtype == "int16" else x.astype(np.float32) / np.float32(32768)


def audio_for(golden, sr):
    """per live stream TICKS chunks of the fixture speech, each from another place of the recording"""
    n = chunk_of(sr)
    pcm = golden["16k" if sr == 16000 else "8k"]["pcm_i16"]
    return [np.ascontiguousarray(np.roll(pcm, -(30 * n + 7919 * i))[:TICKS * n]) for i in range(len(SRC))]


class Run:
    """One pump, where the live streams sit in it, and their chunks: tick t steps every live stream on its chunk t (a masked tick)."""

    def __init__(self, model, sr, slots, audio, tape=0, dtype="int16"):
        from silero_vad_amd import StreamPump
        self.pump = StreamPump(model.engine, sr, streams=CAP, parts=2, ring_slots=2, tape_chunks=tape, tape_dtype=dtype)
        assert self.pump.parts == 2
        self.slots, self.audio, self.n = list(slots), audio, self.pump.n
        self.live = {s: i for i, s in enumerate(self.slots)}
        self.present = np.zeros(CAP, bool)
        self.present[self.slots] = True

    def submit(self, t):
        r = t % 2
        for i, s in enumerate(self.slots):
            self.pump.slot(r)[s] = self.audio[i][t * self.n:(t + 1) * self.n]
        self.pump.submit(r, self.present)

    def tick(self, t):
        """-> (the live streams' probabilities as bits, their events, what they carry afterwards)"""
        self.submit(t)
        ev, r = self.pump.poll()
        assert self.pump.poll() == (None, None)
        probs = self.pump.probs(r)[self.slots].copy()
        events = sorted((self.live[s], tuple(e.items())) for s, e in ev)
        return probs.view(np.uint32).tolist(), events, self.carried()

    def carried(self):
        return [(self.pump.pending(s), tuple(a.tobytes() for a in self.pump.state(s))) for s in self.slots]

    def dirty(self, ticks, seed):
        """full ticks of noise on every slot: a ring that holds something else, at another phase"""
        rng = np.random.default_rng(seed)
        for t in range(ticks):
            self.pump.slot(t % 2)[:] = rng.integers(-9000, 9000, (CAP, self.n)).astype(np.int16)
            self.pump.submit(t % 2)
            self.pump.poll()

    def close(self):
        self.pump.close()


def twin_run(model, sr, audio, dtype):
    """the uninterrupted pump: every tick's results, and the pump itself (it holds the last 5 chunks)"""
    a = Run(model, sr, SRC, audio, tape=5, dtype=dtype)
    return a, [a.tick(t) for t in range(TICKS)]


def source_at_the_cut(model, sr, audio, dtype, want, tape=5):
    b = Run(model, sr, SRC, audio, tape=tape, dtype=dtype)
    for t in range(CUT):
        assert b.tick(t) == want[t]
    return b


def continue_on(c, want, first=CUT):
    for t in range(first, TICKS):
        got = c.tick(t)
        assert got[0] == want[t][0], ("probability", t)
        assert got[1] == want[t][1], ("events", t)
        assert got[2] == want[t][2], ("pending / state", t)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("sr", [16000, 8000])
def test_a_migrated_stream_keeps_its_audio(model, golden, sr, dtype):
    from silero_vad_amd import snapshot_info, snapshot_tape, _lib
    n, elem = chunk_of(sr), 2 if dtype == "int16" else 4
    s2, s3 = strides(sr)
    audio = audio_for(golden, sr)
    twin, want = twin_run(model, sr, audio, dtype)
    assert sum(len(w[1]) for w in want) >= 1                       # (the streams are inside speech: events happen)
    b = source_at_the_cut(model, sr, audio, dtype, want)
    assert all(b.pump.tape_state(s) == (CUT, 0) for s in SRC)       # the ring of 5 has wrapped: held_lo = 3
    tape_from = [0, 4 * n + 17, 8 * n, -5, 7 * n, 2 ** 62]
    runs = [(3, 5), (4, 4), (0, 0), (3, 5), (7, 1), (0, 0)]        # (first_chunk, n_chunks): chunks 3..7, 4..7, none, 3..7, 7, none
    blob = b.pump.export_streams_v3(SRC, tape_from=tape_from)
    assert np.array_equal(blob, b.pump.export_streams_v3(SRC, tape_from=tape_from))         # no tick between them: the same bytes
    total = sum(k for _, k in runs)
    assert len(blob) == HEADER3 + 6 * s3 + total * n * elem == _lib.lib().vad_snapshot_bytes_v3(sr, 6, elem, total)
    assert blob[8:16].view("<u4").tolist() == [3, HEADER3] and blob[28:32].view("<u4")[0] == s3
    assert blob[64:72].view("<i4").tolist() == [elem, 0] and blob[72:80].view("<i8")[0] == total * n * elem and not blob[80:128].any()
    v2 = b.pump.export_streams(SRC, version=2)
    r3, r2 = blob[HEADER3:HEADER3 + 6 * s3].reshape(6, s3), v2[96:].reshape(6, s2)
    assert np.array_equal(r3[:, :s2], r2)                          # the version 2 record, byte for byte
    info = snapshot_info(blob)
    at = 0
    for i, (first, k) in enumerate(runs):
        t = info[i]["tape"]
        assert (t["first_chunk"], t["n_chunks"], t["offset"], t["elem"]) == (first, k, at if k else 0, elem), i
        assert same(t["audio"], heard(audio[i][first * n:(first + k) * n], dtype)), i
        assert same(snapshot_tape(blob, i), t["audio"]) or k == 0
        assert info[i]["current_sample"] == CUT * n
        at += k * n * elem
    # tape_from as a dict: the streams it names from there, the others nothing; None: everything held
    named = b.pump.export_streams_v3(SRC, tape_from={SRC[0]: 0, SRC[1]: 4 * n + 17, SRC[3]: -5, SRC[4]: 7 * n})
    assert np.array_equal(named, blob)
    held = snapshot_info(b.pump.export_streams_v3(SRC))
    assert all((g["tape"]["first_chunk"], g["tape"]["n_chunks"]) == (3, 5) for g in held)
    whole = snapshot_info(b.pump.export_streams_v3(tape_from=np.zeros(CAP, np.int64)))
    assert len(whole) == CAP and all(whole[s]["tape"]["n_chunks"] == 5 for s in SRC)
    assert all(whole[s]["tape"]["n_chunks"] == 0 for s in range(CAP) if s not in SRC)               # never stepped: count = 0
    b.close()
    # into other slots of three destinations
    for chunks, dirty in ((7, 0), (5, 3), (3, 0)):
        c = Run(model, sr, DST, audio, tape=chunks, dtype=dtype)
        c.dirty(dirty, seed=chunks)
        c.pump.import_streams(blob, DST)
        assert c.carried() == want[CUT - 1][2]
        kept = [min(k, chunks) for _, k in runs]
        for i, s in enumerate(DST):
            assert c.pump.tape_state(s) == (CUT, CUT - kept[i]), (chunks, i)
        audios, first = c.pump.fetch_audio(DST, [0] * 6, [CUT * n] * 6)
        for i in range(6):
            assert int(first[i]) == (CUT - kept[i]) * n and same(audios[i], heard(audio[i][(CUT - kept[i]) * n:CUT * n], dtype)), (chunks, i)
        other = [s for s in range(CAP) if s not in DST]
        assert all(c.pump.tape_state(s) == (dirty, 0) for s in other)                               # no other slot's counters moved
        continue_on(c, want)
        # a range that spans the migration point: what the destination holds of it is the audio fed, and the twin's where both hold it
        lo = [max(CUT - kept[i], TICKS - chunks) for i in range(6)]
        audios, first = c.pump.fetch_audio(DST, [0] * 6, [FAR] * 6)
        theirs, their_first = twin.pump.fetch_audio(SRC, [0] * 6, [FAR] * 6)
        for i, s in enumerate(DST):
            assert c.pump.tape_state(s) == (TICKS, CUT - kept[i])
            assert int(first[i]) == lo[i] * n and same(audios[i], heard(audio[i][lo[i] * n:], dtype)), (chunks, i)
            both = max(int(first[i]), int(their_first[i]))
            assert same(audios[i][both - int(first[i]):], theirs[i][both - int(their_first[i]):]) and both < TICKS * n
        assert chunks == 3 or any(lo[i] < CUT for i in range(6))                                    # (... and did span it)
        c.close()
    twin.close()


def test_a_resampled_stream_keeps_its_audio(model, speech):
    """44.1 -> 16 kHz, bound, fp32 tape: after the move the destination's tape returns the bits the source's returns for the same range,
    before and after further ticks on both."""
    from silero_vad_amd import StreamPump, snapshot_info
    x = speech(44100, 16000)
    row, src_slot, dst_slot = 1411, 3, 21                          # 32 ms of input a tick
    pumps = []
    for chunks in (9, 6):
        p = StreamPump(model.engine, 16000, streams=CAP, parts=2, ring_slots=2, tape_chunks=chunks, tape_dtype="float32")
        p.set_resample((44100,))
        pumps.append(p)
    a, c = pumps

    def tick(p, slot, t):
        p.write_resampled_packets(t % 2, [(slot, x[t * row:(t + 1) * row], 44100)])
        ev, r = p.poll()
        return p.probs(r)[slot].view(np.uint32).item(), ev

    for t in range(8):
        tick(a, src_slot, t)
    count, floor = a.tape_state(src_slot)
    assert floor == 0 and 6 <= count <= 8 and a.pending(src_slot) > 0
    blob = a.export_streams_v3([src_slot], tape_from=[2 * 512 + 100])
    rec = snapshot_info(blob)[0]
    assert rec["resample"]["src_rate"] == 44100 and (rec["tape"]["first_chunk"], rec["tape"]["n_chunks"], rec["tape"]["elem"]) == (2, count - 2, 4)
    c.import_streams(blob, [dst_slot])
    kept = min(count - 2, 6)
    assert c.tape_state(dst_slot) == (count, count - kept) and c.resample_state(dst_slot) == a.resample_state(src_slot)
    ours, first = c.fetch_audio([dst_slot], [0], [FAR])
    theirs, _ = a.fetch_audio([src_slot], [int(first[0])], [FAR])
    assert int(first[0]) == (count - kept) * 512 and len(ours[0]) == kept * 512 and same(ours[0], theirs[0]) and ours[0].any()
    for t in range(8, 11):
        got, want = tick(c, dst_slot, t), tick(a, src_slot, t)
        assert got[0] == want[0] and [e for _, e in got[1]] == [e for _, e in want[1]]
    assert c.tape_state(dst_slot)[0] == a.tape_state(src_slot)[0] > count
    ours, first = c.fetch_audio([dst_slot], [0], [FAR])
    theirs, _ = a.fetch_audio([src_slot], [int(first[0])], [FAR])
    assert int(first[0]) < count * 512 and same(ours[0], theirs[0])                                 # a range that spans the migration point
    for p in pumps:
        p.close()


def test_the_utterance_a_stream_migrates_in_comes_back_whole(model, golden):
    """One stream plays the speech fixture and is moved while it is inside an utterance.  With version 3 and the collector's open START
    the END on the destination returns first == start and the audio the uninterrupted pump's collector returns; a version 2 move of
    the same stream at the same tick, START adopted all the same, returns the utterance with its head cut off: first > start."""
    from silero_vad_amd import StreamPump, UtteranceCollector, snapshot_info
    pcm = golden["16k"]["pcm_i16"]
    n, src, dst = 512, 5, 19
    ticks = 115200 // n
    make = lambda: StreamPump(model.engine, 16000, streams=CAP, parts=2, ring_slots=2, tape_chunks=160)

    def play(p, col, slot, t0, t1):
        present = np.zeros(CAP, bool)
        present[slot] = True
        out = []
        for t in range(t0, t1):
            p.slot(t % 2)[slot] = pcm[t * n:(t + 1) * n]
            p.submit(t % 2, present)
            ev, _ = p.poll()
            out += col.feed(ev)
        return out

    a = make()
    whole = play(a, UtteranceCollector(a), src, 0, ticks)
    a.close()
    assert len(whole) >= 2 and all(u[1] == u[3] for u in whole)
    # cut in the middle of the longest utterance
    _, start, end, _, speech_audio = max(whole, key=lambda u: u[2] - u[1])
    assert end - start >= 8 * n and np.array_equal(speech_audio, pcm[start:end])
    cut = (start + end) // 2 // n
    b = make()
    col_b = UtteranceCollector(b)
    before = play(b, col_b, src, 0, cut)
    assert len(before) < len(whole) and all(g[:4] == r[:4] and np.array_equal(g[4], r[4]) for g, r in zip(before, whole))
    starts = col_b.open_starts([src])
    assert starts == {src: start}
    blob3 = b.export_streams_v3([src], tape_from=starts)
    blob2 = b.export_streams([src], version=2)
    b.close()
    rec = snapshot_info(blob3)[0]
    assert rec["triggered"] == 1 and rec["current_sample"] == cut * n
    assert (rec["tape"]["first_chunk"], rec["tape"]["n_chunks"]) == (start // n, cut - start // n)  # from the chunk that holds START, no more
    after = {}
    for version, blob in ((3, blob3), (2, blob2)):
        c = make()
        col_c = UtteranceCollector(c)
        c.import_streams(blob, [dst])
        col_c.adopt(dst, starts[src])
        after[version] = play(c, col_c, dst, cut, ticks)
        c.close()
    want = whole[len(before):]
    assert [u[1:3] for u in after[3]] == [u[1:3] for u in want] == [u[1:3] for u in after[2]] and after[3][0][1:3] == (start, end)
    for got, ref in zip(after[3], want):                           # the assertion the feature exists for
        assert got[0] == dst and got[3] == got[1] == ref[3] and np.array_equal(got[4], ref[4])
    _, s2, e2, first2, audio2 = after[2][0]                        # the contrast: nothing before the import is held
    assert first2 == cut * n > s2 and np.array_equal(audio2, pcm[first2:e2])
    assert all(np.array_equal(g[4], r[4]) and g[3] == r[3] for g, r in zip(after[2][1:], want[1:]))


@pytest.mark.parametrize("sr", [16000, 8000])
def test_a_pump_without_a_tape_writes_version_2_records_and_no_audio(model, golden, sr):
    from silero_vad_amd import snapshot_info
    s2, s3 = strides(sr)
    audio = audio_for(golden, sr)
    b = Run(model, sr, SRC, audio)
    for t in range(3):
        b.tick(t)
    blob = b.pump.export_streams_v3(SRC, tape_from=[0] * 6)
    assert np.array_equal(blob, b.pump.export_streams_v3(SRC))
    assert len(blob) == HEADER3 + 6 * s3 and blob[64:68].view("<i4")[0] == 0 and not blob[64:128].any()
    v2 = b.pump.export_streams(SRC, version=2)
    r3, r2 = blob[HEADER3:].reshape(6, s3), v2[96:].reshape(6, s2)
    assert np.array_equal(r3[:, :s2], r2) and not r3[:, s2:].any()
    assert all(g["tape"]["n_chunks"] == 0 and g["tape"]["elem"] == 0 for g in snapshot_info(blob))
    # ... and it enters a pump with a tape like a version 2 blob: count = floor
    c = Run(model, sr, DST, audio, tape=4)
    c.pump.import_streams(blob, DST)
    assert all(c.pump.tape_state(s) == (3, 3) for s in DST) and c.carried() == b.carried()
    for p in (b, c):
        p.close()
    # the edges of the record walk (test_pump_snapshot_v2.py): 1, 4 and 5 records of a pump of 37 streams in three parts
    pump, fed = edge_pump(model, golden, sr)
    twin, _ = edge_pump(model, golden, sr, tape_chunks=4)
    for slots in EDGE_LISTS:
        blob, v2 = pump.export_streams_v3(slots), pump.export_streams(slots, version=2)
        assert len(blob) == HEADER3 + len(slots) * s3 and not blob[64:128].any()
        r3, r2 = blob[HEADER3:].reshape(-1, s3), v2[96:].reshape(-1, s2)
        assert np.array_equal(r3[:, :s2], r2) and not r3[:, s2:].any()
        info = snapshot_info(blob)
        edge_records_hold(pump, fed, slots, info)
        assert all(g["tape"]["n_chunks"] == 0 and g["resample"]["src_rate"] == 0 for g in info)
        dst = [(s + 16) % 37 for s in slots]
        twin.import_streams(blob, dst)
        assert all(twin.tape_state(d) == (2, 2) and twin.pending(d) == pump.pending(s) and
                   all(x.tobytes() == y.tobytes() for x, y in zip(twin.state(d), pump.state(s))) for s, d in zip(slots, dst))
        assert np.array_equal(twin.export_streams(dst, version=2), v2)
    pump.close()
    twin.close()


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_a_taped_blob_enters_a_pump_without_a_tape(model, golden, dtype):
    audio = audio_for(golden, 16000)
    twin, want = twin_run(model, 16000, audio, dtype)
    twin.close()
    b = source_at_the_cut(model, 16000, audio, dtype, want)
    blob = b.pump.export_streams_v3(SRC)
    b.close()
    c = Run(model, 16000, DST, audio)
    c.pump.import_streams(blob, DST)
    assert c.carried() == want[CUT - 1][2]
    continue_on(c, want)                                           # the stream itself continues bit for bit
    c.close()


def test_refusals_leave_the_pump_as_it_was(model, golden):
    from silero_vad_amd import _lib
    sr, n = 16000, 512
    audio = audio_for(golden, sr)
    twin, want = twin_run(model, sr, audio, "int16")
    twin.close()
    b = source_at_the_cut(model, sr, audio, "int16", want)
    blob = b.pump.export_streams_v3(SRC, tape_from=[0] * 6)
    refused = lambda: pytest.raises(_lib.VadError, match="VAD_ERR_ARG")
    # an int16 blob into a pump with an fp32 tape (and the reverse)
    f = source_at_the_cut(model, sr, audio, "float32", want)
    before, clocks = f.carried(), [f.pump.tape_state(s) for s in range(CAP)]
    for recs in (list(range(6)), [2]):                              # (also a record whose run is empty: the blob's element is what counts)
        with refused():
            f.pump.import_streams(blob, [SRC[i] for i in recs], records=recs)
    assert f.carried() == before and [f.pump.tape_state(s) for s in range(CAP)] == clocks and f.pump.poll() == (None, None)
    with refused():
        b.pump.import_streams(f.pump.export_streams_v3(SRC), SRC)
    audios, first = f.pump.fetch_audio(SRC, [0] * 6, [FAR] * 6)
    assert all(int(first[i]) == 3 * n and same(audios[i], heard(audio[i][3 * n:CUT * n], "float32")) for i in range(6))
    continue_on(f, want)                                           # the refused pump's next ticks are the twin's
    f.close()
    # a tick in flight: no plan-and-export, no import; the tick is not disturbed
    c = Run(model, sr, DST, audio, tape=5)
    c.pump.import_streams(blob, DST)
    c.submit(CUT)
    for call in (lambda: c.pump.export_streams_v3(DST), lambda: c.pump.export_streams_v3(tape_from={}),
                 lambda: c.pump.import_streams(blob, DST)):
        with refused():
            call()
    ev, r = c.pump.poll()
    assert c.pump.probs(r)[DST].view(np.uint32).tolist() == want[CUT][0] and c.carried() == want[CUT][2]
    continue_on(c, want, first=CUT + 1)
    c.close()
    # cap too small: nothing written, and the source goes on as the twin
    L, h = b.pump._L, b.pump._h
    slots = np.array(SRC, np.int32)
    tf = np.zeros(6, np.int64)
    need = L.vad_pump_snapshot_plan_v3(h, slots.ctypes.data, 6, tf.ctypes.data)
    assert need == len(blob)
    small = np.full(need, 0x5a, np.uint8)
    assert L.vad_pump_export_streams_v3(h, slots.ctypes.data, 6, tf.ctypes.data, small.ctypes.data, need - 1) == 1 and (small == 0x5a).all()
    assert b"plan_v3" in L.vad_pump_last_error(h)
    assert L.vad_pump_export_streams_v3(h, slots.ctypes.data, 6, tf.ctypes.data, small.ctypes.data, need) == 0 and np.array_equal(small, blob)
    for bad in ([SRC[0], SRC[0]], [CAP], [-1]):                     # a slot twice or out of range: no plan, no export
        s = np.array(bad, np.int32)
        assert L.vad_pump_snapshot_plan_v3(h, s.ctypes.data, len(bad), None) == 0
        assert L.vad_pump_export_streams_v3(h, s.ctypes.data, len(bad), None, small.ctypes.data, need) == 1
    continue_on(b, want)
    b.close()
