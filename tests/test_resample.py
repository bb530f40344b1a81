"""Recordings at 44.1 kHz and other odd rates, resampled to the net's rate (`resample` / vad_resample_*, `read_audio`, `source_rate=` of the
ragged_* corpus calls), without a GPU.

The function is torchaudio's default Resample (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) as arithmetic; torchaudio is not
in the image, so the reference here is the formula written out in numpy below (`dense_kernel`, `dense_resample`: the dense [N][2 W + O]
kernel and a padded strided convolution in double), independently of the library's table.  The corpus route is defined by reduction,
like `codec=` and `channels=`: a call with `source_rate` is the same call on [resample(a) for a in audios] -- bit for bit on the CPU
stand-in (tests/replay_engine.py), which resamples on the host; the device route is held to `resample` within the derived bound in
tests/test_resample_gpu.py.

Source material: the fixture speech of tests/golden/audio_16k.npz brought to 44.1 kHz and rounded to int16.  `resample` itself serves
the net's rates only (8000 / 16000 as the target), so the upsampling is done by `dense_resample`, the same formula."""
import ctypes
import wave
from math import gcd

import numpy as np
import pytest
import torch

from conftest import GOLD

# src, dst -> O, N, W, K (include/silero_vad_hip.h "resampling"; the values were checked in numpy from the formula)
PAIRS = {(44100, 16000): (441, 160, 17, 34), (22050, 16000): (441, 320, 9, 17), (11025, 16000): (441, 640, 7, 13),
         (24000, 16000): (3, 2, 10, 19), (48000, 16000): (3, 1, 19, 37), (44100, 8000): (441, 80, 34, 67), (88200, 8000): (441, 40, 67, 134)}


def dense_kernel(src, dst):
    """-> (h float32 [N][2 W + O], O, N, W): every tap of every phase, in double, rounded to float32"""
    g = gcd(src, dst)
    O, N = src // g, dst // g
    base = min(O, N) * 0.99
    W = int(np.ceil(6 * O / base))
    i = np.arange(2 * W + O, dtype=np.float64)[None, :]
    j = np.arange(N, dtype=np.float64)[:, None]
    t = np.clip((-j / N + (i - W) / O) * base, -6.0, 6.0)
    win = np.cos(t * np.pi / 12) ** 2
    pt = np.pi * t
    sinc = np.where(pt == 0, 1.0, np.sin(pt) / np.where(pt == 0, 1.0, pt))
    return (sinc * win * base / O).astype(np.float32), O, N, W


def dense_resample(x, src, dst, absolute=False):
    """the padded strided convolution in double -> float64 [ceil(N L / O)]; absolute: sum |h x| instead"""
    h, O, N, W = dense_kernel(src, dst)
    x = np.asarray(x, dtype=np.float64)
    L = len(x)
    n_out = -(-N * L // O)
    Q = -(-n_out // N)
    xp = np.concatenate([np.zeros(W), x, np.zeros(Q * O + W + O)])
    win = np.lib.stride_tricks.sliding_window_view(xp, 2 * W + O)[::O][:Q]          # [Q][2 W + O]: x[q O + i - W]
    h = h.astype(np.float64)
    out = (np.abs(win) @ np.abs(h).T) if absolute else (win @ h.T)
    return out.reshape(-1)[:n_out]


def as_float(x):
    x = np.asarray(x)
    return x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)


@pytest.fixture(scope="module")
def speech_44k():
    """8 s of the fixture speech at 44.1 kHz, int16"""
    x = np.load(GOLD / "audio_16k.npz")["pcm"][:128000]
    y = dense_resample(as_float(x), 16000, 44100)
    assert len(y) == 352800
    return np.clip(np.rint(y * 32768.0), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def model(oracle):
    from replay_engine import ReplayEngine
    from silero_vad_amd.engine import HipSileroVAD
    return HipSileroVAD(engine=ReplayEngine(oracle))


# ---- 1. the table --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", list(PAIRS))
def test_table_and_geometry_against_the_formula(built, pair):
    from silero_vad_amd import resample_geometry, resample_table
    assert resample_geometry(*pair) == PAIRS[pair]
    h, O, N, W = dense_kernel(*pair)
    assert (O, N, W) == PAIRS[pair][:3]
    taps, first = resample_table(*pair)
    K = PAIRS[pair][3]
    assert taps.shape == (N, K) and taps.dtype == np.float32 and first.shape == (N,)
    live = h != 0
    for j in range(N):
        idx = np.flatnonzero(live[j])
        a, b = int(idx[0]), int(idx[-1])
        assert live[j, a:b + 1].all(), f"a zero inside the run of phase {j}"
        assert first[j] == a and b - a + 1 <= K
        run = h[j, a:b + 1]
        assert (np.abs(taps[j, :len(run)] - run) <= np.spacing(np.abs(run))).all(), j      # one float32 ulp: libm against numpy
        assert (taps[j, len(run):] == 0).all()
    assert max(int(np.flatnonzero(r)[-1] - np.flatnonzero(r)[0]) + 1 for r in live) == K
    if pair == (44100, 16000):
        sums = taps.astype(np.float64).sum(axis=1)
        assert 1.0004 <= sums.min() and sums.max() <= 1.0005
        assert taps.nbytes + first.nbytes < 24 * 1024


def test_geometry_refusals(built):
    from silero_vad_amd import _lib, resample, resample_geometry
    L = _lib.lib()
    for src, dst in ((16000, 16000), (8000, 8000), (44100, 44100), (16000, 44100), (44100, 22050), (44101, 16000), (192000, 8000), (0, 16000),
                     (-44100, 16000)):
        assert L.vad_resample_geometry(src, dst, None, None, None, None) == 2, (src, dst)          # VAD_ERR_SAMPLE_RATE
        assert L.vad_resample_length(src, dst, 100) == -2
        assert L.vad_resample_table(src, dst, None, None) == 2 and L.vad_resample_host(src, dst, None, 2, 0, None) == 2
        with pytest.raises(ValueError, match="not served"):
            resample_geometry(src, dst)
    assert L.vad_resample_geometry(44100, 16000, None, None, None, None) == 0
    assert L.vad_resample_table(44100, 16000, None, None) == 1 and L.vad_resample_length(44100, 16000, -1) == -1
    x = np.zeros(8, np.int16)
    out = np.zeros(8, np.float32)
    assert L.vad_resample_host(44100, 16000, x.ctypes.data, 1, 8, out.ctypes.data) == 1              # elem_size
    assert L.vad_resample_host(44100, 16000, None, 2, 8, out.ctypes.data) == 1
    assert L.vad_resample_host(44100, 16000, None, 2, 0, None) == 0
    assert L.vad_resample_reserve(None, 44100, 16000) == 1
    assert L.vad_resample_rows_device(None, 44100, 16000, None, 2, 0, None, 0, 0, None, 0, None) == 1
    h = ctypes.c_void_p()
    good = _lib.WEIGHTS_PATH.read_bytes()
    assert L.vad_create_host_only(good, len(good), ctypes.byref(h)) == 0
    assert L.vad_resample_reserve(h, 44100, 16000) == 4 and L.vad_resample_reserve(h, 44100, 44100) == 2      # NO_DEVICE; the pair first
    assert L.vad_resample_rows_device(h, 44100, 16000, None, 2, 0, None, 0, 0, None, 0, None) == 4
    assert L.vad_resample_rows_device(h, 44100, 16000, None, 3, 0, None, 0, 0, None, 0, None) == 1
    L.vad_destroy(h)
    with pytest.raises(ValueError, match="1-D"):
        resample(np.zeros((2, 8), np.float32), 44100, 16000)
    assert resample(np.zeros(0, np.int16), 44100, 16000).shape == (0,)


@pytest.mark.parametrize("n", [1, 16, 17, 18, 440, 441, 442, 100001])
def test_lengths(built, n):
    from silero_vad_amd import _lib, resample
    want = -(-160 * n // 441)
    assert _lib.lib().vad_resample_length(44100, 16000, n) == want
    assert len(resample(np.ones(n, np.int16), 44100, 16000)) == want
    if n == 100001:
        assert want == 36282


# ---- 2. the CPU twin -----------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("kind", ["int16", "float32"])
def test_twin_against_the_dense_convolution(built, pair, kind):
    """`resample` accumulates the stored run in double and rounds ONCE to float32: its double sum lies within 1e-13 sum |h x| of the
    dense convolution in double (the order of the sums; the taps are the formula's), so the float32 it returns lies within that plus
    half a float32 ulp -- the one rounding -- of the dense value."""
    from silero_vad_amd import resample
    rng = np.random.default_rng(5)
    O, N, W, K = PAIRS[pair]
    for L in (1, W - 1, W, W + 1, O - 1, O, O + 1, 5 * O + 3, 7001):
        x = (rng.standard_normal(L) * 0.3).clip(-1, 1)
        x = np.rint(x * 32767).astype(np.int16) if kind == "int16" else x.astype(np.float32)
        got = resample(x, *pair)
        want, mag = dense_resample(as_float(x), *pair), dense_resample(as_float(x), *pair, absolute=True)
        assert got.dtype == np.float32 and got.shape == want.shape
        half_ulp = 0.5 * np.maximum(np.spacing(np.abs(got)), np.spacing(np.abs(want).astype(np.float32))).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want) <= 1e-13 * mag + half_ulp).all(), L


@pytest.mark.parametrize("pair", [(44100, 16000), (11025, 16000), (24000, 16000), (44100, 8000)])
def test_impulses_reproduce_the_table(built, pair):
    """A unit impulse at sample p puts tap p - (q O + first[j] - W) of phase j into output q N + j: at p = 0 and p = L - 1, both edges."""
    from silero_vad_amd import resample, resample_table
    O, N, W, K = PAIRS[pair]
    taps, first = resample_table(*pair)
    L = 3 * O + 5
    for p in (0, L - 1):
        x = np.zeros(L, np.float32)
        x[p] = 1.0
        got = resample(x, *pair)
        m = np.arange(len(got))
        k = p - ((m // N) * O + first[m % N] - W)
        want = np.where((k >= 0) & (k < K), taps[m % N, np.clip(k, 0, K - 1)], 0.0).astype(np.float32)
        assert np.array_equal(got, want), p
        assert np.count_nonzero(got) > 0


# ---- 3. the front door ---------------------------------------------------------------------------------
def write_wav(path, pcm, rate, channels):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm).tobytes())


def test_read_audio_resamples_a_44k_file(built, speech_44k, tmp_path):
    from silero_vad_amd import read_audio, resample
    mono = speech_44k[:50001]
    write_wav(tmp_path / "mono.wav", mono, 44100, 1)
    got = read_audio(tmp_path / "mono.wav", 16000)
    want = resample(mono.astype(np.float32) / 32768.0, 44100, 16000)
    assert got.dtype == torch.float32 and got.shape == (-(-160 * 50001 // 441),) and np.array_equal(got.numpy(), want)
    right = speech_44k[100000:150001]
    stereo = np.stack([mono, right], axis=1)
    write_wav(tmp_path / "stereo.wav", stereo, 44100, 2)
    got = read_audio(tmp_path / "stereo.wav", 16000)
    want = resample(stereo.astype(np.float32).mean(axis=1) / 32768.0, 44100, 16000)
    assert np.array_equal(got.numpy(), want) and not np.array_equal(got.numpy(), read_audio(tmp_path / "mono.wav", 16000).numpy())
    assert len(read_audio(tmp_path / "mono.wav", 8000)) == -(-80 * 50001 // 441)
    assert np.array_equal(read_audio(tmp_path / "mono.wav", 44100).numpy(), mono.astype(np.float32) / 32768.0)       # the file's own rate: as before
    with pytest.raises(ValueError, match="44100 Hz, asked for 22050"):
        read_audio(tmp_path / "mono.wav", 22050)


# ---- 4. the corpus route on the CPU stand-in -----------------------------------------------------------
def recordings(speech_44k, seed=3):
    rng = np.random.default_rng(seed)
    lens = [1, 17, 441, 1412, 30000, 52345, 97001, 141120]
    return [speech_44k[a:a + m].copy() for a, m in zip(rng.integers(0, len(speech_44k) - max(lens), size=len(lens)), lens)]


def packed(recs):
    from silero_vad_amd import PackedRecordings
    lens = np.array([len(x) for x in recs], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return PackedRecordings(torch.from_numpy(np.concatenate(recs)), offs, lens)


@pytest.mark.parametrize("container", ["list", "packed"])
def test_ragged_probs_with_source_rate_is_the_call_on_resampled_recordings(built, model, speech_44k, container):
    from silero_vad_amd import ragged_probs, resample
    recs = recordings(speech_44k)
    twins = [torch.from_numpy(resample(a, 44100, 16000)) for a in recs]
    audios = [torch.from_numpy(a) for a in recs] if container == "list" else packed(recs)
    got = ragged_probs(audios, model, 16000, source_rate=44100)
    want = ragged_probs(twins, model, 16000)
    assert len(got) == len(want) == len(recs)
    for a, g, w in zip(recs, got, want):
        assert len(g) == -(-(-(-160 * len(a) // 441)) // 512) and torch.equal(g, w)
    # the 8 kHz net, and a source rate equal to the net's: the plain call
    got8 = ragged_probs(audios, model, 8000, source_rate=44100)
    want8 = ragged_probs([torch.from_numpy(resample(a, 44100, 8000)) for a in recs], model, 8000)
    assert all(torch.equal(g, w) for g, w in zip(got8, want8))
    same = ragged_probs(twins, model, 16000, source_rate=16000)
    assert all(torch.equal(g, w) for g, w in zip(same, want))


def test_ragged_probs_with_source_rate_and_channels(built, model, speech_44k):
    from silero_vad_amd import deinterleave, ragged_probs, resample
    recs = recordings(speech_44k)
    inter, flat, ch = [], [], []
    for i, a in enumerate(recs):
        if i % 3 == 2:
            inter.append(a)
            flat.append(a)
            ch.append(1)
        else:
            b = np.roll(a, 7)[::-1].copy()
            st = np.empty(2 * len(a), np.int16)
            st[0::2], st[1::2] = a, b
            inter.append(st)
            flat += [deinterleave(st, 2, 0), deinterleave(st, 2, 1)]
            ch.append(2)
    got = ragged_probs([torch.from_numpy(a) for a in inter], model, 16000, channels=ch, source_rate=44100)
    want = ragged_probs([torch.from_numpy(resample(a, 44100, 16000)) for a in flat], model, 16000)
    assert len(got) == len(flat) and all(torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("container", ["list", "packed"])
def test_ragged_speech_segments_with_source_rate(built, model, speech_44k, container):
    from silero_vad_amd import ragged_speech_segments, resample
    recs = recordings(speech_44k)
    twins = [torch.from_numpy(resample(a, 44100, 16000)) for a in recs]
    audios = [torch.from_numpy(a) for a in recs] if container == "list" else packed(recs)
    got = ragged_speech_segments(audios, model, 16000, source_rate=44100)
    want = ragged_speech_segments(twins, model, 16000)
    assert got == want
    assert sum(len(s) for s in got) >= 1, "the fixture speech must give at least one segment"
    for a, segs in zip(recs, got):
        n_out = -(-160 * len(a) // 441)
        assert all(0 <= s["start"] < s["end"] <= n_out for s in segs)                  # samples of the RESAMPLED signal, clipped to it
    cnt, flat = ragged_speech_segments(audios, model, 16000, source_rate=44100, as_arrays=True)
    assert cnt.tolist() == [len(s) for s in want] and flat.tolist() == [[s["start"], s["end"]] for sg in want for s in sg]


def test_source_rate_refusals(built, model, speech_44k):
    import silero_vad_amd as sv
    recs = [torch.from_numpy(a) for a in recordings(speech_44k)[:3]]
    for call in (lambda: sv.ragged_speech_audio(recs, model, 16000, source_rate=44100),
                 lambda: sv.refill_reserve(recs, model, 16000, source_rate=44100),
                 lambda: sv.refill_probs(recs, model, 16000, source_rate=44100),
                 lambda: next(sv.refill_segments_stream(recs, model, 16000, source_rate=44100)),
                 lambda: sv.refill_speech_segments(recs, model, 16000, source_rate=44100),
                 lambda: sv.batch_speech_timestamps(recs, model, 16000, source_rate=44100),
                 lambda: sv.StreamPump(None, 16000, streams=4, source_rate=44100)):
        with pytest.raises(ValueError, match="source_rate"):
            call()
    # pairs and net rates the route does not serve name the argument too
    for kw in (dict(sampling_rate=16000, source_rate=44101), dict(sampling_rate=48000, source_rate=44100), dict(sampling_rate=44100, source_rate=16000),
               dict(sampling_rate=16000, source_rate=0)):
        with pytest.raises(ValueError, match="source_rate"):
            sv.ragged_probs(recs, model, **kw)
        with pytest.raises(ValueError, match="source_rate"):
            sv.ragged_speech_segments(recs, model, **kw)
        with pytest.raises(ValueError, match="source_rate"):
            sv.ragged_reserve(recs, model, **kw)
    # ... and sampling_rate=44100 alone raises what it raised before
    with pytest.raises(ValueError, match="Supported sampling rates"):
        sv.ragged_probs(recs, model, 44100)
