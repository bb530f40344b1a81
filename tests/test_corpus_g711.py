"""G.711 recordings on the corpus side (`codec=` of ragged_probs / refill_probs / batch_speech_timestamps, a uint8 PackedRecordings,
vad_stage_rows(elem_size = 1), vad_upload_rows_coded's refusals), without a GPU.  The route is defined by reduction, like the pump's
(tests/test_pump_g711.py): every result of a G.711 call is, bit for bit, that of the same call on the recordings expanded by
`g711_expand` as int16.  Here the engine is the CPU stand-in (tests/replay_engine.py), which has no device expansion: the codes are
expanded on the host and take the int16 path.  The device routes are held to the same reduction in tests/test_corpus_g711_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import GOLD, SRS

LAWS = ("ulaw", "alaw")


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


def recordings(tag, count=12, lo=1, hi=40, seed=5):
    """`count` recordings cut from the fixture audio: lo ... hi chunks with odd tails, mu-law and A-law alternating with a few repeats.
    -> (codes per recording, law per recording, the expanded int16 recordings)"""
    from silero_vad_amd import g711_expand
    n = 512 if tag == "16k" else 256
    pcm = np.load(GOLD / f"audio_{tag}.npz")["pcm"]
    rng = np.random.default_rng(seed)
    chunks = [lo, hi] + [int(v) for v in rng.integers(lo, hi + 1, size=count - 2)]
    lens = [max(1, c * n - int(t)) for c, t in zip(chunks, rng.integers(0, n, size=count))]
    lens[0], lens[1] = 1 if lo == 1 else lo * n - 3, hi * n          # the shortest there is, and a whole number of chunks
    laws = [LAWS[(i + i // 5) % 2] for i in range(count)]
    at = rng.integers(0, len(pcm) - hi * n, size=count)
    codes = [encode(pcm[a:a + m], law) for a, m, law in zip(at, lens, laws)]
    return codes, laws, [g711_expand(c, law) for c, law in zip(codes, laws)]


def arena_of(codes, pin=False, align=1):
    """The recordings back to back (or at multiples of `align` bytes) in one uint8 tensor -> (base, offsets, lengths)"""
    lens = np.array([len(c) for c in codes], dtype=np.int64)
    step = (lens + align - 1) // align * align
    offs = np.concatenate([[0], np.cumsum(step)[:-1]]).astype(np.int64)
    base = torch.zeros(int(step.sum()) + 16, dtype=torch.uint8)
    if pin:
        base = base.pin_memory()
    for o, c in zip(offs, codes):
        base[o:o + len(c)] = torch.from_numpy(c)
    return base, offs, lens


@pytest.fixture(scope="module")
def model(oracle):
    from replay_engine import ReplayEngine
    from silero_vad_amd.engine import HipSileroVAD
    return HipSileroVAD(engine=ReplayEngine(oracle))


def containers(codes, laws, pcm):
    """(coded recordings, their int16 twins) as a list and as a PackedRecordings over one arena"""
    from silero_vad_amd import PackedRecordings
    base, offs, lens = arena_of(codes)
    base16 = torch.zeros(base.numel(), dtype=torch.int16)
    for o, x in zip(offs, pcm):
        base16[o:o + len(x)] = torch.from_numpy(x)
    return {"list": ([torch.from_numpy(c) for c in codes], [torch.from_numpy(x) for x in pcm]),
            "packed": (PackedRecordings(base, offs, lens), PackedRecordings(base16, offs, lens))}


@pytest.mark.parametrize("tag", ["8k", "16k"])
def test_corpus_calls_equal_their_expanded_twins(built, model, tag):
    from silero_vad_amd import batch_speech_timestamps, ragged_probs, refill_probs
    sr = SRS[tag]
    codes, laws, pcm = recordings(tag)
    assert set(laws) == set(LAWS) and len(codes[0]) == 1
    for kind, (coded, twin) in containers(codes, laws, pcm).items():
        for call in (lambda a, **kw: ragged_probs(a, model, sr, **kw), lambda a, **kw: refill_probs(a, model, sr, slots=3, slab_chunks=4, **kw)):
            got, want = call(coded, codec=laws), call(twin)
            assert len(got) == len(want) == len(codes)
            for i, (p, q) in enumerate(zip(got, want)):
                assert torch.equal(p, q), (kind, i)
    coded, twin = containers(codes, laws, pcm)["list"]
    for scheduler in ("buckets", "refill"):
        kw = dict(sampling_rate=sr, scheduler=scheduler, threshold=0.3, min_speech_duration_ms=64)
        got, want = batch_speech_timestamps(coded, model, codec=laws, **kw), batch_speech_timestamps(twin, model, **kw)
        assert got == want and any(want), scheduler
    # the per-recording path (a progress callback rules the schedulers out): codes expanded one recording at a time, also from an arena
    kw = dict(sampling_rate=sr, threshold=0.3, min_speech_duration_ms=64, progress_tracking_callback=lambda pct: None)
    want = batch_speech_timestamps(twin, model, **kw)
    assert any(want)
    for audios in (coded, containers(codes, laws, pcm)["packed"][0]):
        assert batch_speech_timestamps(audios, model, codec=laws, **kw) == want
    # one law for all: a name instead of a sequence
    one = [c for c, law in zip(coded, laws) if law == "alaw"]
    one_twin = [x for x, law in zip(twin, laws) if law == "alaw"]
    for p, q in zip(ragged_probs(one, model, sr, codec="alaw"), ragged_probs(one_twin, model, sr)):
        assert torch.equal(p, q)


def test_bytes_are_never_guessed_at(built, model):
    from silero_vad_amd import PackedRecordings, batch_speech_timestamps, ragged_probs, ragged_speech_segments, refill_probs, refill_speech_segments
    codes, laws, pcm = recordings("8k", count=4, hi=6)
    coded = [torch.from_numpy(c) for c in codes]
    base, offs, lens = arena_of(codes)
    for audios in (coded, PackedRecordings(base, offs, lens)):
        for call in (ragged_probs, refill_probs, ragged_speech_segments, refill_speech_segments, batch_speech_timestamps):
            with pytest.raises(TypeError, match="never guessed"):
                call(audios, model, 8000)
    mixed = [coded[0], torch.from_numpy(pcm[1]), coded[2], torch.from_numpy(pcm[3]).float() / 32768.0]
    for call in (ragged_probs, refill_probs, batch_speech_timestamps):
        with pytest.raises(TypeError, match="mixed"):
            call(mixed, model, 8000, codec=laws)
        with pytest.raises(TypeError, match="mixed"):
            call(mixed[:2], model, 8000, codec="ulaw")
    with pytest.raises(ValueError):
        ragged_probs(coded, model, 8000, codec=laws[:2])                   # one codec per recording
    with pytest.raises(ValueError):
        ragged_probs(coded, model, 8000, codec="s16")                      # uint8 is never linear PCM
    with pytest.raises(ValueError):
        ragged_probs(coded, model, 8000, codec="g729")


def test_stage_rows_packs_bytes(built):
    """vad_stage_rows(elem_size = 1): a plain byte packing, rows at any address, zero BYTES behind each row."""
    from silero_vad_amd import _lib
    rng = np.random.default_rng(8)
    arena = rng.integers(0, 256, size=70_000, dtype=np.uint8)
    width = 4099
    lens = np.array([0, 1, 15, 16, 17, width - 1, width] + [int(v) for v in rng.integers(0, width + 1, size=25)], dtype=np.int64)
    offs = rng.integers(0, len(arena) - width, size=len(lens))
    offs[:16] = offs[:16] // 16 * 16 + np.arange(16)                      # every byte misalignment
    rows = (ctypes.c_void_p * len(lens))(*[arena.ctypes.data + int(o) if m else None for o, m in zip(offs, lens)])
    clens = lens.ctypes.data_as(ctypes.POINTER(ctypes.c_long))
    want = np.zeros((len(lens), width), dtype=np.uint8)
    for i, (o, m) in enumerate(zip(offs, lens)):
        want[i, :m] = arena[o:o + m]
    for threads in (1, 3):
        got = np.full((len(lens), width), 0x5A, dtype=np.uint8)
        assert _lib.lib().vad_stage_rows(rows, clens, len(lens), width, 1, got.ctypes.data, threads) == 0
        assert np.array_equal(got, want)
    assert _lib.lib().vad_stage_rows(rows, clens, len(lens), width, 3, got.ctypes.data, 1) == 1          # VAD_ERR_ARG
    assert _lib.lib().vad_stage_rows(rows, clens, len(lens), width - 1, 1, got.ctypes.data, 1) == 1      # a row longer than the width


def test_upload_rows_coded_needs_a_device(built):
    """The checks that come before any device work, in vad_upload_rows' order: no engine is an argument error, a host-only engine
    refuses device work before it looks at the rows."""
    from silero_vad_amd import _lib
    L = _lib.lib()
    good = _lib.WEIGHTS_PATH.read_bytes()
    h = ctypes.c_void_p()
    assert L.vad_create_host_only(good, len(good), ctypes.byref(h)) == 0
    buf = np.zeros(64, dtype=np.uint8)
    rows = (ctypes.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data + 7)
    lens = (ctypes.c_long * 2)(8, 8)
    cd = np.array([1, 2], dtype=np.uint8)
    dst = np.zeros((2, 8), dtype=np.int16)
    for how in (0, 1, 2):
        assert L.vad_upload_rows_coded(None, rows, lens, cd.ctypes.data, 2, 8, dst.ctypes.data, how, None) == 1      # VAD_ERR_ARG
        assert L.vad_upload_rows_coded(h, rows, lens, cd.ctypes.data, 2, 8, dst.ctypes.data, how, None) == 4         # VAD_ERR_NO_DEVICE
        assert b"host-only" in L.vad_last_error(h)
        assert L.vad_upload_rows(h, rows, lens, 2, 8, 2, dst.ctypes.data, how, None) == 4                            # (the same order)
    bad = np.array([1, 3], dtype=np.uint8)
    assert L.vad_upload_rows_coded(h, rows, lens, bad.ctypes.data, 2, 8, dst.ctypes.data, 1, None) == 4
    assert L.vad_upload_rows_coded(h, rows, lens, None, 2, 8, dst.ctypes.data, 1, None) == 4
    L.vad_destroy(h)
