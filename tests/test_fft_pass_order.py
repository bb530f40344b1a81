"""The FFT pass of the frontends issues its LDS traffic in batches (csrc/fft_wave.hpp fft_math: window taps, twiddle rows and the
partner fetches of the real-FFT unpack are requested ahead and waited for once per batch; the bins of the unpack go in mirrored
groups).  Only the ORDER of issue changed, so at the shapes where framing can go wrong -- one stream, one short of / exactly / one
past a 16-stream tile; one, two, five chunks; a partial last chunk; a carried context; both rates, float and int16 PCM, the 32 / 48 kHz
front door, rows with a stride of their own -- the throughput frontend (kernel_front_f43.hip) and the latency frontend
(kernel_front_lat.hip), which share that code, must give the same bits, and both sit inside the suite's bounds against the oracle."""
import numpy as np
import pytest
import torch

from conftest import SRS, state_err

pytestmark = pytest.mark.gpu

TOL = 1e-4          # relative, on the final (h, c)
TIGHT = 2e-5        # on probabilities


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


def rolled_rows(wav, B, L, stride):
    return np.stack([np.roll(wav, -b * stride)[:L] for b in range(B)])


def as_pcm(rows, pcm):
    """(what the engine reads, the float signal that stands for)"""
    if pcm == "float":
        return rows, rows
    i16 = (rows * 32768.0).clip(-32768, 32767).astype(np.int16)
    return i16, i16.astype(np.float32) / 32768.0


def run_forms(model, x, sr, ctx0, st0):
    """x [B, L] (a cuda tensor, any row stride) through the throughput and the latency frontend: [(probs, ctx, state)] * 2."""
    eng, out = model.engine, []
    for form in ("throughput", "latency"):
        ctx = torch.as_tensor(ctx0).to(model.device).clone()
        st = torch.as_tensor(st0).to(model.device).clone()
        eng.set_option("front", form)
        try:
            p = eng.forward_audio(x, sr, ctx, st)
            torch.cuda.synchronize()
        finally:
            eng.set_option("front", "auto")
        out.append((p.cpu().numpy(), ctx.cpu().numpy(), st.cpu().numpy()))
    return out


def check(model, oracle, x, sr, ref_rows, net_sr, ctx0, st0, what):
    (p1, c1, s1), (p2, c2, s2) = run_forms(model, x, sr, ctx0, st0)
    assert np.array_equal(p1, p2) and np.array_equal(c1, c2) and np.array_equal(s1, s2), what
    want, wctx, wst = oracle.forward_audio(ref_rows, net_sr, ctx=ctx0, state=st0)
    ep, es = float(np.abs(p1 - want).max()), state_err(s1, wst)
    print(f"{what}: max|dp| {ep:.3e}  state {es:.3e}")
    assert ep < TIGHT and es < TOL, (what, ep, es)
    assert np.array_equal(c1, wctx), what
    return p1


def carried(B, n, seed):
    rng = np.random.default_rng(seed)
    return (0.1 * rng.standard_normal((B, n // 8))).astype(np.float32), (0.3 * rng.standard_normal((2, B, 128))).astype(np.float32)


@pytest.mark.parametrize("pcm", ["float", "int16"])
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("B", [1, 15, 16, 17])
@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_tile_and_chunk_edges(model, oracle, golden, tag, B, T, pcm):
    """Whole chunks and a partial last one (the zero-padded `tail` copy), each with a carried non-zero context and state."""
    sr = SRS[tag]
    n = chunk_of(sr)
    ctx0, st0 = carried(B, n, 1000 * B + T)
    for cut in (0, 37):
        rows = rolled_rows(golden[tag]["wav"], B, T * n - cut, 4001)
        data, ref = as_pcm(rows, pcm)
        check(model, oracle, torch.from_numpy(data).to(model.device), sr, ref, sr, ctx0, st0, (tag, B, T, pcm, cut))


@pytest.mark.parametrize("pcm", ["float", "int16"])
@pytest.mark.parametrize("k", [2, 3])
def test_front_door_decimation(model, oracle, golden, k, pcm):
    """32 / 48 kHz input: the decimation is folded into the pass's sample loads; the reference is the oracle on x[:, ::k]."""
    n = 512
    for B, T, cut in ((1, 1, 0), (17, 2, 0), (17, 5, 77)):
        L16 = T * n - cut
        ctx0, st0 = carried(B, n, 77 * k + B + T)
        sig, ref = as_pcm(rolled_rows(golden["16k"]["wav"], B, L16, 313), pcm)
        raw = np.zeros((B, L16 * k - (k - 1)), sig.dtype)
        raw[:, ::k] = sig
        check(model, oracle, torch.from_numpy(raw).to(model.device), 16000 * k, ref, 16000, ctx0, st0, (k, pcm, B, T, cut))


@pytest.mark.parametrize("pad", [8, 3])
@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_rows_with_a_stride_of_their_own(model, oracle, golden, tag, pad):
    """B = 17 rows cut out of a wider buffer: the row stride is no multiple of the row length (pad 3: rows not 16-byte aligned either)."""
    sr = SRS[tag]
    n = chunk_of(sr)
    B, T = 17, 5
    L = T * n - 37
    rows = rolled_rows(golden[tag]["wav"], B, L, 1237)
    big = torch.full((B, L + pad), 0.25, device=model.device)      # (what lies between the rows must not be read as signal)
    view = big[:, :L]
    view.copy_(torch.from_numpy(rows))
    assert view.stride(0) == L + pad
    ctx0, st0 = carried(B, n, 5 + pad)
    check(model, oracle, view, sr, rows, sr, ctx0, st0, (tag, "stride", pad))


def test_speech_fixture_probabilities_are_not_saturated(model, oracle, golden):
    """The speech recording itself (tests/golden/audio_16k.npz), from its start: probabilities across the whole range, where an error
    in a magnitude is not hidden behind a flat sigmoid."""
    n, B, T = 512, 17, 40
    rows = rolled_rows(golden["16k"]["wav"], B, T * n, 7919)
    ctx0, st0 = np.zeros((B, n // 8), np.float32), np.zeros((2, B, 128), np.float32)
    p = check(model, oracle, torch.from_numpy(rows).to(model.device), 16000, rows, 16000, ctx0, st0, "speech")
    mid = (p > 0.1) & (p < 0.9)
    assert mid.sum() >= 20 and (p > 0.9).any() and (p < 0.1).any(), (int(mid.sum()), float(p.min()), float(p.max()))


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_silent_frame_beside_a_non_silent_one(model, oracle, golden, tag):
    """Exactly silent frames beside frames that are not (a run of zeros that begins and ends inside chunks): the pass's magnitudes
    decide which chunks go on the exact-fix list (csrc/exact_front.hpp), a silent frame's must be exactly zero in either form."""
    sr = SRS[tag]
    n = chunk_of(sr)
    B, T = 17, 5
    rows = rolled_rows(golden[tag]["wav"], B, T * n, 3001)
    for b in range(B):
        s0 = n + (b * 53) % (2 * n)
        rows[b, s0:s0 + n + n // 3] = 0.0
    rows[5] = 0.0                                                  # silent throughout
    rows[6, :2 * n] = 0.0                                          # starts silent
    ctx0, st0 = np.zeros((B, n // 8), np.float32), np.zeros((2, B, 128), np.float32)
    x = torch.from_numpy(rows).to(model.device)
    check(model, oracle, x, sr, rows, sr, ctx0, st0, (tag, "silent frames"))
    # the gate pre-activations too, and the list really was used: switched off, some chunk's bits differ
    eng, gx = model.engine, {}
    for form in ("throughput", "latency"):
        eng.set_option("front", form)
        try:
            gx[form] = eng.debug_frontend(x, sr, torch.zeros((B, n // 8), device=model.device)).cpu().numpy()
        finally:
            eng.set_option("front", "auto")
    assert np.array_equal(gx["throughput"], gx["latency"])
    eng.set_option("exact_transitions", "0")
    try:
        off = eng.debug_frontend(x, sr, torch.zeros((B, n // 8), device=model.device)).cpu().numpy()
    finally:
        eng.set_option("exact_transitions", "1")
    taken = (off.reshape(B, T, 512) != gx["throughput"].reshape(B, T, 512)).any(-1)
    assert taken.sum() >= B and not taken.all()
