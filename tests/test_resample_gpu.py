"""The device resampler (csrc/kernel_resample.hip, vad_resample_rows_device, `resample_device`) and the corpus route built on it
(`source_rate=` of ragged_probs / ragged_speech_segments / ragged_reserve), on the GPU.

Error bound.  An output is a K-tap sum in fp32; against the CPU twin `resample` -- the same table, accumulated in double, rounded once
-- it may differ by |d| <= (K + 1) 2^-24 sum_k |h_k x_k|: K roundings in any order, fused or not, plus the twin's final rounding; the
int16 scaling is exact.  Derived, not measured; computed per output sample below (`bound`).

Tile edge.  A workgroup of the kernel makes TILE = 1024 consecutive outputs of one row (kResampleTile, csrc/device_api.hpp) and stages
the input span they read in LDS: the shortest row that fills the first tile, the shortest that puts an output into the second, the row
one sample shorter than each, and the same at the end of the second tile sit either side of it."""
import numpy as np
import pytest
import torch

from test_resample import PAIRS, packed, recordings, speech_44k  # noqa: F401  (speech_44k: the module fixture)

pytestmark = pytest.mark.gpu
TIGHT = 2e-5        # tests/test_gpu_parity.py: the GPU's probabilities against the oracle's on the same float32 samples
TILE = 1024
GPU_PAIRS = [(44100, 16000), (22050, 16000), (11025, 16000), (24000, 16000), (48000, 16000), (44100, 8000)]


@pytest.fixture(scope="module")
def model(built):
    from silero_vad_amd import load_silero_vad
    return load_silero_vad(device=0)


def min_len_for(n_out, O, N):
    """the shortest recording with ceil(N L / O) >= n_out"""
    return (n_out - 1) * O // N + 1


def row_lengths(pair, group):
    O, N, W, K = PAIRS[pair]
    if group == "short":
        return [1, W - 1, W, W + 1, O - 1, O, O + 1]
    # (when the pair upsamples not every output count is some row's: the edge is named by the shortest row that reaches it)
    fill, spill = min_len_for(TILE, O, N), min_len_for(TILE + 1, O, N)           # the first tile full; the first output of the second tile
    fill2, spill2 = min_len_for(2 * TILE, O, N), min_len_for(2 * TILE + 1, O, N)
    out = lambda m: -(-N * m // O)
    assert out(fill - 1) < TILE <= out(fill) and out(spill - 1) <= TILE < out(spill) and out(spill2 - 1) <= 2 * TILE < out(spill2)
    return [fill - 1, fill, spill - 1, spill, fill2 - 1, fill2, spill2, min_len_for(2 * TILE + TILE // 2, O, N)]


def bound(x, pair):
    """(K + 1) 2^-24 sum_k |h_k x_k| of every output of the float64 recording x, from the table"""
    from silero_vad_amd import resample_table
    O, N, W, K = PAIRS[pair]
    taps, first = resample_table(*pair)
    m = np.arange(-(-N * len(x) // O))
    p = ((m // N) * O + first[m % N] - W)[:, None] + np.arange(K)[None, :]
    xs = np.where((p >= 0) & (p < len(x)), np.abs(x)[np.clip(p, 0, len(x) - 1)], 0.0)
    return (K + 1) * 2.0 ** -24 * (np.abs(taps[m % N].astype(np.float64)) * xs).sum(axis=1)


@pytest.mark.parametrize("group", ["short", "tile"])
@pytest.mark.parametrize("kind", ["int16", "float32"])
@pytest.mark.parametrize("pair", GPU_PAIRS)
def test_kernel_against_the_twin(model, pair, kind, group):
    from silero_vad_amd import resample, resample_device
    O, N, W, K = PAIRS[pair]
    lens = row_lengths(pair, group)
    assert len(lens) <= 8
    rng = np.random.default_rng(7)
    L = max(lens) + 13
    if kind == "int16":
        batch = np.full((len(lens), L), 30000, np.int16)                 # behind every row's length: a large value the kernel must not read
        rows = [rng.integers(-20000, 20000, size=m).astype(np.int16) for m in lens]
    else:
        batch = np.full((len(lens), L), 1.0e6, np.float32)
        rows = [(rng.standard_normal(m) * 0.3).astype(np.float32) for m in lens]
    for r, x in enumerate(rows):
        batch[r, :len(x)] = x
    width = -(-N * L // O) + 5
    big = torch.full((len(lens), width + 3), float("nan"), dtype=torch.float32, device=model.device)
    out = resample_device(model.engine, torch.from_numpy(batch).to(model.device), lens, *pair, out=big[:, :width])
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert out.data_ptr() == big.data_ptr()
    assert np.isnan(got[:, width:]).all(), "written past width_out"
    assert not np.isnan(got[:, :width]).any(), "an output in [0, width_out) was left unwritten"
    for r, x in enumerate(rows):
        cut = -(-N * len(x) // O)
        assert (got[r, cut:width] == 0).all() and not np.signbit(got[r, cut:width]).any(), (r, "zeros from the cut to width_out")
        want = resample(x, *pair)
        xf = x.astype(np.float64) / 32768.0 if kind == "int16" else x.astype(np.float64)
        d = np.abs(got[r, :cut].astype(np.float64) - want.astype(np.float64))
        lim = bound(xf, pair)
        print(f"{pair} {kind} len {len(x)}: max |d| {d.max():.3e}, max |d| / bound {np.max(d / np.maximum(lim, 1e-300)):.3f}")
        assert (d <= lim).all(), (r, len(x), float(d.max()))


def test_position_independence(model, speech_44k):
    """The same recording alone, and as row 5 of a batch of another pitch among rows of other lengths: identical bits."""
    from silero_vad_amd import resample_device
    a = speech_44k[20000:20000 + 7001]
    dev = model.device
    alone = resample_device(model.engine, torch.from_numpy(a).to(dev), None, 44100, 16000)
    rng = np.random.default_rng(1)
    lens = [9000, 100, 4410, 8191, 3, 7001, 7002, 5000]
    batch = rng.integers(-30000, 30000, size=(8, 9011)).astype(np.int16)
    batch[5, :7001] = a
    rows = resample_device(model.engine, torch.from_numpy(batch).to(dev), lens, 44100, 16000)
    n_out = -(-160 * 7001 // 441)
    assert alone.shape == (n_out,) and torch.equal(rows[5, :n_out], alone) and bool((rows[5, n_out:] == 0).all())
    af = torch.from_numpy(a.astype(np.float32) / 32768.0).to(dev)           # int16 / 32768 is exact: the float recording gives the same bits
    assert torch.equal(resample_device(model.engine, af, None, 44100, 16000), alone)


def solo_probs(model, a, src=44100, dst=16000):
    """model.audio_forward on the recording's own resampled audio (zero padded to one chunk where it is shorter: the corpus pads so)"""
    from silero_vad_amd import resample_device
    r = resample_device(model.engine, torch.from_numpy(a).to(model.device), None, src, dst)
    n = 512 if dst == 16000 else 256
    if len(r) < n:
        r = torch.nn.functional.pad(r, (0, n - len(r)))
    return model.audio_forward(r[None], dst)[0], r


def containers(recs, kind):
    if kind == "pinned":
        return [torch.from_numpy(a).pin_memory() for a in recs]
    if kind == "pageable":
        return [torch.from_numpy(a) for a in recs]
    p = packed(recs)
    p.base = p.base.pin_memory()
    return p


@pytest.mark.parametrize("kind", ["pinned", "pageable", "arena"])
def test_ragged_probs_with_source_rate_on_the_device(model, speech_44k, kind, monkeypatch):
    """Every ingest route: the gather over the link, pageable staging, an arena window (so few recordings do not pass the window route's
    density rule on their own: the arena runs under SILERO_VAD_AMD_UPLOAD=window)."""
    from silero_vad_amd import ragged_probs
    monkeypatch.delenv("SILERO_VAD_AMD_UPLOAD", raising=False)
    if kind == "arena":
        monkeypatch.setenv("SILERO_VAD_AMD_UPLOAD", "window")
    recs = recordings(speech_44k)
    got = ragged_probs(containers(recs, kind), model, 16000, source_rate=44100)
    assert len(got) == len(recs)
    for a, g in zip(recs, got):
        want = solo_probs(model, a)[0]
        assert len(g) == -(-(-(-160 * len(a) // 441)) // 512) and torch.equal(g, want[:len(g)]), len(a)


def test_ragged_speech_segments_and_reserve_with_source_rate(model, speech_44k):
    from silero_vad_amd import ragged_probs, ragged_reserve, ragged_speech_segments
    from silero_vad_amd.streams import STATS, _compute_lanes
    recs = recordings(speech_44k)
    audios = containers(recs, "pinned")
    on_dev = ragged_speech_segments(audios, model, 16000, source_rate=44100, device_scan=True)
    on_host = ragged_speech_segments(audios, model, 16000, source_rate=44100, device_scan=False)
    assert on_dev == on_host and sum(len(s) for s in on_dev) >= 1
    for a, segs in zip(recs, on_dev):
        assert all(0 <= s["start"] < s["end"] <= -(-160 * len(a) // 441) for s in segs)
    # a fresh model: ragged_reserve alone sizes the lanes' scratch, the staging slots, the resampling table and the lanes' buffers
    from silero_vad_amd import load_silero_vad
    fresh = load_silero_vad(device=0)
    ragged_reserve(audios, fresh, 16000, source_rate=44100)
    lanes = _compute_lanes(fresh, 2)
    gens = [lm.engine.scratch_generation() for lm, _ in lanes]
    allocs = STATS["resample_allocs"]
    assert allocs >= len(lanes)
    again = ragged_probs(audios, fresh, 16000, source_rate=44100)
    assert [lm.engine.scratch_generation() for lm, _ in lanes] == gens and STATS["resample_allocs"] == allocs
    assert all(torch.equal(g, solo_probs(model, a)[0][:len(g)]) for a, g in zip(recs, again))


def test_parity_against_the_oracle_on_the_resampled_audio(model, oracle, speech_44k):
    """The project's contract: the GPU's probabilities against the oracle's at TIGHT.  Both sides read the SAME float32 samples -- the
    GPU's own resampled audio -- so the resampler adds nothing to it."""
    from silero_vad_amd import ragged_probs
    recs = [a for a in recordings(speech_44k) if len(a) > 20000]
    got = ragged_probs([torch.from_numpy(a) for a in recs], model, 16000, source_rate=44100)
    for a, g in zip(recs, got):
        r = solo_probs(model, a)[1].cpu().numpy()
        want = oracle.forward_audio(r[None], 16000)[0][0]
        err = float(np.abs(g.numpy() - want).max())
        print(f"len {len(a)}: max |dp| {err:.3e}")
        assert err < TIGHT
