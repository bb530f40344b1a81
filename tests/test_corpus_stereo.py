"""Interleaved stereo recordings on the corpus side (`channels=` of the ragged_* / refill_* calls and batch_speech_timestamps,
`deinterleave` / vad_deinterleave, `channel_rows`, `read_wav_raw`, vad_upload_rows_channels' first checks), without a GPU.  The route is
defined by reduction, like `codec=` (tests/test_corpus_g711.py): every result of a call with `channels` is, bit for bit, that of the same
call on the flat list [deinterleave(a_i, C_i, c) for i in recordings for c in range(C_i)].  Here the engine is the CPU stand-in
(tests/replay_engine.py), which cannot split: the recordings are de-interleaved on the host and take the mono path.  The device routes
are held to the same reduction in tests/test_corpus_stereo_gpu.py."""
import ctypes
import struct
import wave

import numpy as np
import pytest
import torch

from conftest import GOLD, SRS
from test_corpus_g711 import LAWS, arena_of, encode

CODEC_ID = {None: 0, "s16": 0, "ulaw": 1, "alaw": 2}


@pytest.fixture(scope="module")
def model(oracle):
    from replay_engine import ReplayEngine
    from silero_vad_amd.engine import HipSileroVAD
    return HipSileroVAD(engine=ReplayEngine(oracle))


def interleave(chans):
    out = np.empty(len(chans) * len(chans[0]), dtype=chans[0].dtype)
    for c, x in enumerate(chans):
        out[c::len(chans)] = x
    return out


def stereo_recordings(tag, law, count=9, lo=1, hi=24, seed=11, per=1, single_frame=True):
    """`count` recordings cut from the fixture audio, every third one mono, the others two DIFFERENT cuts interleaved; lo ... hi chunks
    (of `per` samples a net sample) with odd tails, the first a single frame.  law "s16": int16 samples, "ulaw" / "alaw": uint8 codes,
    "g711": the two laws alternating.  -> (interleaved recordings, channel counts, law per recording, the flat int16 twin list)"""
    from silero_vad_amd import g711_expand
    n = (512 if tag == "16k" else 256) * per
    pcm = np.load(GOLD / f"audio_{tag}.npz")["pcm"]
    pcm = np.repeat(pcm, per) if per > 1 else pcm
    rng = np.random.default_rng(seed)
    frames = [max(1, int(c) * n - int(t)) for c, t in zip(rng.integers(lo, hi + 1, size=count), rng.integers(0, n, size=count))]
    if single_frame:
        frames[0] = 1
    chans = [1 if i % 3 == 2 else 2 for i in range(count)]
    laws = [law if law != "g711" else LAWS[(i + i // 4) % 2] for i in range(count)]
    recs, twins = [], []
    for m, C, lw in zip(frames, chans, laws):
        cuts = [encode(pcm[a:a + m], lw) for a in rng.integers(0, len(pcm) - hi * n, size=C)]
        assert C == 1 or m < 64 or not np.array_equal(cuts[0], cuts[1])
        recs.append(interleave(cuts))
        twins += [c if lw == "s16" else g711_expand(c, lw) for c in cuts]
    return recs, chans, laws, twins


def containers(recs, twins):
    """(interleaved recordings, flat int16 twins) as lists and as PackedRecordings over one arena each"""
    from silero_vad_amd import PackedRecordings
    out = {"list": ([torch.from_numpy(r) for r in recs], [torch.from_numpy(x) for x in twins])}
    packed = []
    for group in (recs, twins):
        lens = np.array([len(x) for x in group], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        base = torch.from_numpy(np.concatenate(group + [np.zeros(16, dtype=group[0].dtype)]))
        packed.append(PackedRecordings(base, offs, lens))
    out["packed"] = tuple(packed)
    return out


# ---- 1. the host twin ----------------------------------------------------------------------------------
def _raw_deinterleave(codec, channels, channel, buf_ptr, frames, out):
    from silero_vad_amd import _lib
    return _lib.lib().vad_deinterleave(codec, channels, channel, buf_ptr, frames, out.ctypes.data if out is not None else None)


@pytest.mark.parametrize("law", ["s16", "ulaw", "alaw"])
def test_deinterleave_against_numpy(built, law):
    from silero_vad_amd import deinterleave, g711_expand
    rng = np.random.default_rng(2)
    esz = 2 if law == "s16" else 1
    for C in (1, 2):
        for frames in (0, 1, 2, 255, 256, 4097):
            x = rng.integers(0, 256, size=frames * C * esz, dtype=np.uint8)
            if law != "s16" and frames >= 256:                         # all 256 codes in each channel
                for c in range(C):
                    x[c:256 * C:C] = np.roll(np.arange(256, dtype=np.uint8), 31 * c)
            x = x.view(np.int16) if law == "s16" else x
            for c in range(C):
                want = x[c::C] if law == "s16" else g711_expand(np.ascontiguousarray(x[c::C]), law)
                if law != "s16" and frames >= 256:
                    assert len(set(x[c::C][:256].tolist())) == 256
                got = deinterleave(x, C, c, None if law == "s16" else law)
                assert got.dtype == np.int16 and np.array_equal(got, want), (C, frames, c)
                if law == "s16":
                    assert np.array_equal(deinterleave(x, C, c, "s16"), want)
                # the C entry point at every byte misalignment (G.711) / every even one (S16) of the source
                raw = x.view(np.uint8)
                for mis in range(0, 16, esz):
                    buf = np.zeros(len(raw) + 32, dtype=np.uint8)
                    at = (-buf.ctypes.data) % 16 + mis
                    buf[at:at + len(raw)] = raw
                    out = np.full(frames + 1, 0x5A5A, dtype=np.int16)
                    assert _raw_deinterleave(CODEC_ID[law], C, c, buf.ctypes.data + at, frames, out) == frames
                    assert np.array_equal(out[:frames], want) and out[frames] == 0x5A5A, (C, frames, c, mis)


def test_deinterleave_refusals(built):
    from silero_vad_amd import deinterleave
    x = np.arange(8, dtype=np.int16)
    out = np.full(8, 0x5A5A, dtype=np.int16)
    p = x.ctypes.data
    for codec, C, c, ptr, frames, o in ((3, 2, 0, p, 4, out), (-1, 2, 0, p, 4, out), (0, 0, 0, p, 4, out), (0, 3, 0, p, 2, out), (0, 2, 2, p, 4, out),
                                        (0, 2, -1, p, 4, out), (0, 1, 1, p, 4, out), (0, 2, 0, p, -1, out), (0, 2, 0, None, 4, out), (0, 2, 0, p, 4, None)):
        assert _raw_deinterleave(codec, C, c, ptr, frames, o) == -1, (codec, C, c, frames)      # -VAD_ERR_ARG
        assert bool((out == 0x5A5A).all())
    assert _raw_deinterleave(0, 2, 1, None, 0, None) == 0                # nothing to do
    for args in ((x, 3, 0), (x, 2, 2), (x, 0, 0), (x[:7], 2, 0), (x.astype(np.float32), 2, 0), (x, 2, 0, "ulaw"), (x.astype(np.uint8), 2, 0),
                 (x.reshape(2, 4), 2, 0), (x, 2, 0, "g729")):
        with pytest.raises(ValueError):
            deinterleave(*args)


def test_channel_rows():
    from silero_vad_amd import channel_rows
    assert channel_rows([2, 1, 2]) == [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1)]
    assert channel_rows(2, 2) == [(0, 0), (0, 1), (1, 0), (1, 1)] and channel_rows(1, 3) == [(0, 0), (1, 0), (2, 0)]
    for bad in (([3, 1],), ([0],), ([1, 2], 3), (2,), (True, 2), ([True, True],), ([1.0, 2.0],)):
        with pytest.raises(ValueError):
            channel_rows(*bad)


# ---- 2. the corpus calls equal their twins ----------------------------------------------------------------
@pytest.mark.parametrize("law", ["s16", "g711"])
@pytest.mark.parametrize("tag", ["8k", "16k"])
def test_corpus_calls_equal_their_twins(built, model, tag, law):
    from silero_vad_amd import batch_speech_timestamps, channel_rows, ragged_probs, refill_probs
    sr = SRS[tag]
    recs, chans, laws, twins = stereo_recordings(tag, law)
    assert set(chans) == {1, 2} and len(twins[0]) == 1 and len(twins) == sum(chans) == len(channel_rows(chans))
    assert law == "s16" or set(laws) == set(LAWS)
    codec = None if law == "s16" else laws
    for kind, (inter, twin) in containers(recs, twins).items():
        for call in (lambda a, **kw: ragged_probs(a, model, sr, **kw), lambda a, **kw: refill_probs(a, model, sr, slots=3, slab_chunks=4, **kw)):
            got, want = call(inter, codec=codec, channels=chans), call(twin)
            assert len(got) == len(want) == len(twins)
            for i, (p, q) in enumerate(zip(got, want)):
                assert torch.equal(p, q), (kind, i)
    for kind, (inter, twin) in containers(recs, twins).items():
        for scheduler in ("buckets", "refill"):
            kw = dict(sampling_rate=sr, scheduler=scheduler, threshold=0.3, min_speech_duration_ms=64)
            got, want = batch_speech_timestamps(inter, model, codec=codec, channels=chans, **kw), batch_speech_timestamps(twin, model, **kw)
            assert got == want and any(want), (kind, scheduler)
    inter, twin = containers(recs, twins)["list"]
    # the per-recording path (a progress callback rules the schedulers out)
    kw = dict(sampling_rate=sr, threshold=0.3, min_speech_duration_ms=64, progress_tracking_callback=lambda pct: None)
    assert batch_speech_timestamps(inter, model, codec=codec, channels=chans, **kw) == batch_speech_timestamps(twin, model, **kw)
    # one channel count for all: an int instead of a sequence; channels=1 is today's call
    two = [r for r, C in zip(inter, chans) if C == 2]
    two_twin = [x for (i, c), x in zip(channel_rows(chans), twin) if chans[i] == 2]
    one_codec = None if codec is None else [lw for lw, C in zip(laws, chans) if C == 2]
    for p, q in zip(ragged_probs(two, model, sr, codec=one_codec, channels=2), ragged_probs(two_twin, model, sr)):
        assert torch.equal(p, q)
    if law == "s16":
        for p, q in zip(ragged_probs(twin, model, sr, channels=1), ragged_probs(twin, model, sr)):
            assert torch.equal(p, q)


def test_segment_calls_and_streams_equal_their_twins(built, model):
    from silero_vad_amd import ragged_buckets, ragged_speech_segments, refill_segments_stream, refill_speech_segments
    recs, chans, laws, twins = stereo_recordings("8k", "g711", count=7, hi=16)
    inter, twin = containers(recs, twins)["list"]
    scan = dict(threshold=0.3, min_speech_duration_ms=64)
    for call in (lambda a, **kw: ragged_speech_segments(a, model, 8000, **scan, **kw),
                 lambda a, **kw: refill_speech_segments(a, model, 8000, slots=3, slab_chunks=4, **scan, **kw)):
        got, want = call(inter, codec=laws, channels=chans), call(twin)
        assert got == want and any(want)
    # the indices that the generators yield are indices into the flat list
    got = {int(i): p[r] for idxs, p in ragged_buckets(inter, model, 8000, codec=laws, channels=chans) for r, i in enumerate(idxs)}
    want = {int(i): p[r] for idxs, p in ragged_buckets(twin, model, 8000) for r, i in enumerate(idxs)}
    assert sorted(got) == sorted(want) == list(range(len(twins)))
    for i in want:
        m = (len(twins[i]) + 255) // 256
        assert torch.equal(got[i][:m], want[i][:m])
    got = sorted(int(i) for idx, _, _ in refill_segments_stream(inter, model, 8000, slots=3, slab_chunks=4, codec=laws, channels=chans, **scan) for i in idx)
    assert got == list(range(len(twins)))


def test_raw_48k_stereo(built, model):
    """a multiple of 16 kHz: the interleaved recordings stay at their raw rate, like their mono twins"""
    import warnings
    from silero_vad_amd import ragged_probs, refill_probs
    recs, chans, laws, twins = stereo_recordings("16k", "s16", count=5, hi=6, per=3)
    inter, twin = containers(recs, twins)["list"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for call in (lambda a, **kw: ragged_probs(a, model, 48000, **kw), lambda a, **kw: refill_probs(a, model, 48000, slots=3, slab_chunks=4, **kw)):
            got, want = call(inter, channels=chans), call(twin)
            assert len(got) == len(want) == len(twins)
            for p, q in zip(got, want):
                assert torch.equal(p, q)


# ---- 3. refusals ----------------------------------------------------------------------------------------
def test_refusals(built, model):
    import silero_vad_amd as sv
    from silero_vad_amd import PackedRecordings
    recs, chans, laws, twins = stereo_recordings("8k", "ulaw", count=4, hi=6)
    coded = [torch.from_numpy(r) for r in recs]
    pcm = [torch.from_numpy(np.repeat(x, 2)) for x in twins[:4]]             # int16, even lengths
    calls = [lambda a, **kw: list(sv.ragged_buckets(a, model, 8000, **kw)), lambda a, **kw: sv.ragged_reserve(a, model, 8000, **kw),
             lambda a, **kw: sv.ragged_probs(a, model, 8000, **kw), lambda a, **kw: sv.ragged_speech_segments(a, model, 8000, **kw),
             lambda a, **kw: sv.refill_reserve(a, model, 8000, slots=2, slab_chunks=4, **kw),
             lambda a, **kw: sv.refill_probs(a, model, 8000, slots=2, slab_chunks=4, **kw),
             lambda a, **kw: list(sv.refill_segments_stream(a, model, 8000, slots=2, slab_chunks=4, **kw)),
             lambda a, **kw: sv.refill_speech_segments(a, model, 8000, slots=2, slab_chunks=4, **kw),
             lambda a, **kw: sv.batch_speech_timestamps(a, model, 8000, **kw)]
    assert len(calls) == 9
    base, offs, lens = arena_of(recs)
    odd = [pcm[0], pcm[1][:-1], pcm[2], pcm[3]]
    for call in calls:
        with pytest.raises(TypeError, match="int16"):                          # float32 with 2 channels: the device batch is int16
            call([x.float() / 32768.0 for x in pcm], channels=2)
        with pytest.raises(ValueError, match="even"):                          # an odd length
            call(odd, channels=2)
        with pytest.raises(ValueError, match="channels"):
            call(pcm, channels=3)
        with pytest.raises(ValueError, match="channels"):
            call(pcm, channels=0)
        with pytest.raises(ValueError, match="one entry per recording"):      # a sequence of the wrong length
            call(pcm, channels=[2, 2, 1])
        for audios in (coded, PackedRecordings(base, offs, lens)):
            with pytest.raises(TypeError, match="never guessed"):              # uint8 without a codec
                call(audios, channels=chans)


# ---- 4. vad_upload_rows_channels before any device work --------------------------------------------------------
def test_upload_rows_channels_needs_a_device(built):
    """The checks that come before any device work, in vad_upload_rows' order: no engine is an argument error, a host-only engine
    refuses device work before it looks at the table."""
    from silero_vad_amd import _lib
    L = _lib.lib()
    good = _lib.WEIGHTS_PATH.read_bytes()
    h = ctypes.c_void_p()
    assert L.vad_create_host_only(good, len(good), ctypes.byref(h)) == 0
    buf = np.zeros(64, dtype=np.uint8)
    rows = (ctypes.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data + 7)
    frames = (ctypes.c_long * 2)(8, 8)
    cd = np.array([1, 2], dtype=np.uint8)
    ch = np.array([2, 1], dtype=np.uint8)
    to = np.array([[0, 2], [1, -1]], dtype=np.int32)
    dst = np.zeros((3, 8), dtype=np.int16)

    def call(e, cd_, ch_, to_, how):
        return L.vad_upload_rows_channels(e, rows, frames, cd_, ch_, to_.ctypes.data, 2, 3, 8, dst.ctypes.data, how, None)

    for how in (0, 1, 2):
        assert call(None, cd.ctypes.data, ch.ctypes.data, to, how) == 1      # VAD_ERR_ARG
        assert call(h, cd.ctypes.data, ch.ctypes.data, to, how) == 4         # VAD_ERR_NO_DEVICE
        assert b"host-only" in L.vad_last_error(h)
        # ... also with a bad table: an unknown codec, three channels, a row named twice, a row out of range
        assert call(h, np.array([1, 3], dtype=np.uint8).ctypes.data, ch.ctypes.data, to, how) == 4
        assert call(h, cd.ctypes.data, np.array([3, 1], dtype=np.uint8).ctypes.data, to, how) == 4
        assert call(h, cd.ctypes.data, ch.ctypes.data, np.array([[0, 0], [7, -2]], dtype=np.int32), how) == 4
        assert call(h, None, None, to, how) == 4
    assert not dst.any()
    L.vad_destroy(h)


# ---- 5. read_wav_raw ------------------------------------------------------------------------------------------
def riff(tag, channels, rate, bits, data, extra=b""):
    fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + extra + b"data" + struct.pack("<I", len(data)) + data + (b"\x00" if len(data) & 1 else b"")
    return b"RIFF" + struct.pack("<I", len(body)) + body


def test_read_wav_raw(built, model, tmp_path):
    from silero_vad_amd import ragged_probs, read_wav_raw
    recs, chans, laws, twins = stereo_recordings("8k", "s16", count=2, lo=3, hi=8)
    stereo = recs[1] if chans[1] == 2 else recs[0]
    path = tmp_path / "call.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(8000)
        w.writeframes(stereo.tobytes())
    x, rate, C, codec = read_wav_raw(path)
    assert (rate, C, codec) == (8000, 2, None) and x.dtype == torch.int16 and x.dim() == 1 and np.array_equal(x.numpy(), stereo)
    # G.711 files, which `wave` refuses: mono and stereo, both laws, a LIST chunk in front of the data and an odd data size
    rng = np.random.default_rng(4)
    junk = b"LIST" + struct.pack("<I", 5) + b"hello" + b"\x00"
    for tag, law in ((7, "ulaw"), (6, "alaw")):
        for C_ in (1, 2):
            data = rng.integers(0, 256, size=(4001 if C_ == 1 else 4002), dtype=np.uint8)
            p = tmp_path / f"{law}{C_}.wav"
            p.write_bytes(riff(tag, C_, 8000, 8, data.tobytes(), extra=junk))
            x, rate, C, codec = read_wav_raw(p)
            assert (rate, C, codec) == (8000, C_, law) and x.dtype == torch.uint8 and np.array_equal(x.numpy(), data)
    for name, blob in (("pcm24", riff(1, 2, 8000, 24, bytes(12))), ("float", riff(3, 1, 8000, 32, bytes(16))), ("six", riff(1, 6, 8000, 16, bytes(24)))):
        p = tmp_path / f"{name}.wav"
        p.write_bytes(blob)
        with pytest.raises(ValueError, match="format tag"):
            read_wav_raw(p)
    (tmp_path / "not.wav").write_bytes(b"OggS" + bytes(40))
    with pytest.raises(ValueError):
        read_wav_raw(tmp_path / "not.wav")
    # straight into the corpus calls
    from silero_vad_amd import deinterleave
    cuts = np.load(GOLD / "audio_8k.npz")["pcm"]
    calls = interleave([encode(cuts[1000:1000 + 5000], "ulaw"), encode(cuts[30000:30000 + 5000], "ulaw")])
    p = tmp_path / "ulaw_call.wav"
    p.write_bytes(riff(7, 2, 8000, 8, calls.tobytes()))
    x, rate, C, codec = read_wav_raw(p)
    got = ragged_probs([x], model, rate, codec=codec, channels=C)
    want = ragged_probs([torch.from_numpy(deinterleave(calls, 2, c, "ulaw")) for c in range(2)], model, rate)
    assert len(got) == 2 and all(torch.equal(a, b) for a, b in zip(got, want)) and not torch.equal(got[0], got[1])
