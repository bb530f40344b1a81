"""G.711 recordings on the corpus side, on the device: the gather-and-expand kernel (vad_upload_rows_coded, csrc/kernel_ingest.hip
gather_expand_rows_kernel) against numpy, and every ingest route of the corpus schedulers -- arena windows, scattered pinned
recordings, pageable recordings -- against the same call on the `g711_expand`ed int16 recordings, bit for bit (the definition by
reduction of tests/test_corpus_g711.py and tests/test_pump_g711.py).  The expected values come from `g711_expand`, which shares its
one definition (csrc/device_api.hpp g711_to_s16) with the device code: what makes them a reference is that tests/test_pump_g711.py
holds `g711_expand` to the standard's own values, code by code.
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import SRS
from test_corpus_g711 import arena_of, recordings

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
S16, ULAW, ALAW = 0, 1, 2
LAW_NAME = {ULAW: "ulaw", ALAW: "alaw"}
# the kernel's units, in samples: a lane's vector is 16 source bytes, a wave-load 64 of them, a segment 8 wave-loads (8 KiB of source)
VEC = {S16: 8, ULAW: 16, ALAW: 16}
SEG = {S16: 4096, ULAW: 8192, ALAW: 8192}
WIDTH = 2 * 8192 + 1000          # two G.711 segments (four S16 ones) and a tail; a multiple of 8 and not of 16


@pytest.fixture(scope="module")
def model(built):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback to silently pass on)")
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    assert m.engine._h, "native engine not created"
    return m


def kernel_rows():
    """[(codec, length in samples, byte misalignment of the source)]: every length at which the kernel takes another path, every byte
    misalignment of a G.711 row, every even one of an S16 row."""
    assert WIDTH % 8 == 0 and WIDTH % 16 and WIDTH > 2 * SEG[ULAW]
    rows = []
    g_lens = [0, 1, 15, 16, 17, 64 * 16 - 1, 64 * 16, 64 * 16 + 1, SEG[ULAW] - 1, SEG[ULAW], SEG[ULAW] + 1, 2 * SEG[ULAW] - 1, 2 * SEG[ULAW],
              2 * SEG[ULAW] + 1, WIDTH - 1, WIDTH, WIDTH - 8, WIDTH - 9, SEG[ULAW] + 16, SEG[ULAW] - 15, 2 * SEG[ULAW] + 17, WIDTH, WIDTH - 1, WIDTH,
              SEG[ULAW], 2 * SEG[ULAW], 1, 17, SEG[ULAW] + 1, WIDTH - 7, 15, WIDTH]
    for i, m in enumerate(g_lens):                              # 32 rows: both laws at every misalignment 0 ... 15
        rows.append((ULAW if (i // 16 + i) % 2 else ALAW, m, i % 16))
    s_lens = [0, 1, 7, 8, 9, 64 * 8 - 1, 64 * 8, 64 * 8 + 1, SEG[S16] - 1, SEG[S16], SEG[S16] + 1, 3 * SEG[S16] + 1, 4 * SEG[S16], WIDTH - 1, WIDTH, WIDTH]
    for i, m in enumerate(s_lens):                              # 16 rows: every even misalignment, twice
        rows.append((S16, m, 2 * (i % 8)))
    return rows


def lay_out(rows, all_codes_at=(6, 7)):
    """The rows cut from one arena of random bytes -> (arena uint8, offsets, expected int16 [n, WIDTH]).  Rows `all_codes_at` (one of
    each law) hold all 256 codes."""
    from silero_vad_amd import g711_expand
    rng = np.random.default_rng(31)
    offs, at = [], 0
    for codec, m, mis in rows:
        at = (at + 15) // 16 * 16 + mis
        offs.append(at)
        at += m * (2 if codec == S16 else 1) + int(rng.integers(0, 40))
    arena = rng.integers(0, 256, size=at + 64, dtype=np.uint8)
    for r in all_codes_at:
        assert rows[r][0] != S16 and rows[r][1] >= 256
        arena[offs[r]:offs[r] + 256] = np.arange(256, dtype=np.uint8)
    assert {rows[r][0] for r in all_codes_at} == {ULAW, ALAW}
    want = np.zeros((len(rows), WIDTH), dtype=np.int16)
    for i, ((codec, m, _), o) in enumerate(zip(rows, offs)):
        if codec == S16:
            want[i, :m] = arena[o:o + 2 * m].copy().view(np.int16)
        else:
            want[i, :m] = g711_expand(arena[o:o + m], LAW_NAME[codec])
    return arena, np.asarray(offs, dtype=np.int64), want


def tables(base_ptr, offs, lens):
    n = len(lens)
    rows = (ctypes.c_void_p * n)(*[base_ptr + int(o) if m else None for o, m in zip(offs, lens)])
    return rows, (ctypes.c_long * n)(*[int(m) for m in lens])


@pytest.mark.parametrize("how", [1, 2])
def test_gather_expand_kernel(model, how):
    from silero_vad_amd import _lib
    eng = model.engine
    rows = kernel_rows()
    assert len(rows) == 48
    assert {mis for c, m, mis in rows if c != S16 and m} == set(range(16))
    arena, offs, want = lay_out(rows)
    host = torch.from_numpy(arena).pin_memory()
    src = host if how == 1 else host.cuda()
    assert src.data_ptr() % 16 == 0
    lens = [m for _, m, _ in rows]
    codecs = np.array([c for c, _, _ in rows], dtype=np.uint8)
    rp, lp = tables(src.data_ptr(), offs, lens)
    dst = torch.full((len(rows), WIDTH), 0x5A5A, dtype=torch.int16, device="cuda")
    eng.upload_rows_coded(rp, lp, codecs, len(rows), WIDTH, dst, how)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    for i, (c, m, mis) in enumerate(rows):                      # row by row first: a failure names the row
        assert np.array_equal(got[i], want[i]), (i, c, m, mis, int(np.flatnonzero(got[i] != want[i])[0]))
    assert np.array_equal(got, want)

    # a table without an int16 row
    g = [i for i, (c, _, _) in enumerate(rows) if c != S16]
    rp, lp = tables(src.data_ptr(), offs[g], [lens[i] for i in g])
    dst.fill_(0x5A5A)
    eng.upload_rows_coded(rp, lp, np.ascontiguousarray(codecs[g]), len(g), WIDTH, dst[:len(g)], how)
    torch.cuda.synchronize()
    assert np.array_equal(dst[:len(g)].cpu().numpy(), want[g])
    assert bool((dst[len(g):] == 0x5A5A).all())

    # codec_of_row = NULL: every row is int16 -- the batch of vad_upload_rows(elem_size = 2), and of a table of zeros
    even = offs // 2 * 2
    half = [min(m, WIDTH) if c == S16 else m // 2 for c, m, _ in rows]
    rp, lp = tables(src.data_ptr(), even, half)
    plain = torch.full((len(rows), WIDTH), 0x5A5A, dtype=torch.int16, device="cuda")
    eng.upload_rows(rp, lp, len(rows), WIDTH, 2, plain, how)
    for cd in (None, np.zeros(len(rows), dtype=np.uint8)):
        dst.fill_(0x5A5A)
        eng.upload_rows_coded(rp, lp, cd, len(rows), WIDTH, dst, how)
        torch.cuda.synchronize()
        assert torch.equal(dst, plain)
    # ... and an int16 row inside a G.711 table gives what gather_rows_kernel gives for it (rows 32 ... 47 above are such rows)
    s16 = [i for i, (c, _, _) in enumerate(rows) if c == S16]
    rp, lp = tables(src.data_ptr(), offs[s16], [lens[i] for i in s16])
    eng.upload_rows(rp, lp, len(s16), WIDTH, 2, plain[:len(s16)], how)
    torch.cuda.synchronize()
    assert np.array_equal(plain[:len(s16)].cpu().numpy(), got[s16])

    # refusals: nothing is queued, dst keeps its bytes
    dst.fill_(0x5A5A)
    rp, lp = tables(src.data_ptr(), offs, lens)
    bad_codec = codecs.copy()
    bad_codec[5] = 3
    too_long = (ctypes.c_long * len(rows))(*[WIDTH + 1 if i == 7 else m for i, m in enumerate(lens)])
    odd = np.zeros(len(rows), dtype=np.uint8)                  # row 1 sits at misalignment 1: not an int16 row
    for args in ((rp, lp, codecs, 0), (rp, lp, bad_codec, how), (rp, too_long, codecs, how), (rp, lp, odd, how)):
        with pytest.raises(_lib.VadError) as err:
            eng.upload_rows_coded(args[0], args[1], args[2], len(rows), WIDTH, dst, args[3])
        assert err.value.status == 1                           # VAD_ERR_ARG
    with pytest.raises(_lib.VadError):
        eng.upload_rows_coded(rp, lp, codecs, len(rows), WIDTH - 4, dst, how)      # a pitch that is not 16-byte aligned
    torch.cuda.synchronize()
    assert bool((dst == 0x5A5A).all())


def make_containers(kind, codes, pcm):
    """(coded recordings, their expanded int16 twins) in one kind of container"""
    from silero_vad_amd import PackedRecordings
    if kind == "arena":                                        # a pinned arena, packed back to back: the window route
        base, offs, lens = arena_of(codes, pin=True)
        base16 = torch.zeros(base.numel(), dtype=torch.int16).pin_memory()
        for o, x in zip(offs, pcm):
            base16[o:o + len(x)] = torch.from_numpy(x)
        assert len({int(o) % 16 for o in offs}) > 8            # most recordings start at a misaligned byte
        return PackedRecordings(base, offs, lens), PackedRecordings(base16, offs, lens)
    if kind == "pinned":                                       # separately pinned tensors: the gather over PCIe (how = 1)
        return [torch.from_numpy(c).pin_memory() for c in codes], [torch.from_numpy(x).pin_memory() for x in pcm]
    return [torch.from_numpy(c) for c in codes], [torch.from_numpy(x) for x in pcm]      # pageable: staged


@pytest.mark.parametrize("kind", ["arena", "pinned", "pageable"])
@pytest.mark.parametrize("tag", ["8k", "16k"])
def test_corpus_routes_equal_their_expanded_twins(model, oracle, tag, kind):
    from silero_vad_amd import ragged_probs, ragged_speech_segments, refill_probs, refill_speech_segments, streams
    sr = SRS[tag]
    n = 512 if sr == 16000 else 256
    codes, laws, pcm = recordings(tag, count=24, lo=3, hi=40, seed=9)
    assert set(laws) == {"ulaw", "alaw"}
    coded, twin = make_containers(kind, codes, pcm)
    scan = dict(threshold=0.3, min_speech_duration_ms=64)
    link = {}
    for name, call in (("ragged_probs", lambda a, **kw: ragged_probs(a, model, sr, **kw)),
                       ("refill_probs", lambda a, **kw: refill_probs(a, model, sr, slots=8, slab_chunks=4, **kw)),
                       ("ragged_speech_segments", lambda a, **kw: ragged_speech_segments(a, model, sr, **scan, **kw)),
                       ("refill_speech_segments", lambda a, **kw: refill_speech_segments(a, model, sr, slots=8, slab_chunks=4, **scan, **kw))):
        streams.STATS.clear()
        got = call(coded, codec=laws)
        link[name] = [streams.STATS["h2d_bytes"], streams.STATS["refill_window_feed"]]
        streams.STATS.clear()
        want = call(twin)
        link[name] += [streams.STATS["h2d_bytes"], streams.STATS["refill_window_feed"]]
        assert len(got) == len(want) == len(codes)
        if name.endswith("probs"):
            for i, (p, q) in enumerate(zip(got, want)):
                assert p.shape == ((len(codes[i]) + n - 1) // n,) and torch.equal(p, q), (name, i)
            if name == "ragged_probs":
                probs = got
        else:
            assert got == want and any(want), name
    # the routes taken: the codes cross the link at one byte a sample, on the route of the int16 twin
    for name, (b8, feed8, b16, feed16) in link.items():
        assert b8 > 0 and 2 * b8 == b16 and feed8 == feed16, (name, link[name])
        if kind == "arena" and name.startswith("refill"):
            assert feed8 == 1, name
    # three recordings against the CPU oracle on the expanded audio
    for i in (0, 7, 23):
        x = pcm[i].astype(np.float32) / 32768.0
        want = oracle.audio_forward(np.pad(x, (0, -len(x) % n))[None], sr)[0]
        assert np.abs(probs[i].numpy() - want).max() < TIGHT, i
