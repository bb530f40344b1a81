"""Interleaved stereo recordings on the corpus side, on the device: the gather-expand-and-split kernel (vad_upload_rows_channels,
csrc/kernel_ingest.hip gather_channels_kernel) against the host twin `deinterleave` (vad_deinterleave, held to numpy in
tests/test_corpus_stereo.py), and every ingest route of the corpus schedulers -- arena windows, scattered pinned recordings, pageable
recordings -- against the same call on the de-interleaved, expanded int16 twin recordings, bit for bit (the definition by reduction
of tests/test_corpus_stereo.py).
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import SRS
from test_corpus_stereo import stereo_recordings

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
S16, ULAW, ALAW = 0, 1, 2
LAW_NAME = {S16: None, ULAW: "ulaw", ALAW: "alaw"}
# the kernel's units for a STEREO source, in frames: a lane's vector is 16 source bytes (a stereo frame: 4 bytes of S16, 2 of G.711),
# a wave-load 64 vectors, a segment 8 wave-loads (8 KiB of source)
VEC = {S16: 4, ULAW: 8, ALAW: 8}
LOAD = {c: 64 * v for c, v in VEC.items()}
SEG = {c: 8 * v for c, v in LOAD.items()}
WIDTH = 2 * SEG[ULAW] + 1000     # two stereo G.711 segments (four stereo S16 ones) and a tail; a multiple of 8 and not of 16
FILL = 0x5A5A


@pytest.fixture(scope="module")
def model(built):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback to silently pass on)")
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    assert m.engine._h, "native engine not created"
    return m


def kernel_sources():
    """[(codec, channels, frames, byte misalignment of the source, wanted channels)]: for stereo sources of each codec every frame count
    at which the kernel takes another path, at every byte misalignment (G.711) / every even one (S16); mono sources in between."""
    assert WIDTH % 8 == 0 and WIDTH % 16 and 2 * SEG[ULAW] < WIDTH < 3 * SEG[ULAW]
    out = []
    for codec in (ULAW, S16, ALAW):
        lens = [0, 1]
        for unit in (VEC[codec], LOAD[codec], SEG[codec], 2 * SEG[codec]):
            lens += [unit - 1, unit, unit + 1]
        lens += [WIDTH - 9, WIDTH - 8, WIDTH - 1, WIDTH]
        for i, m in enumerate(lens):                            # 18 sources a codec
            mis = 2 * (i % 8) if codec == S16 else (i + (5 if codec == ALAW else 0)) % 16
            want = (0,) if i % 7 == 3 else (1,) if i % 7 == 5 else (0, 1)
            out.append((codec, 2, m, mis, want))
            if i % 6 == 2:                                      # a mono source of the codec behind every sixth
                out.append((codec, 1, [WIDTH - 1, SEG[ULAW] + 1, 17][i // 6], 2 * (i % 8) if codec == S16 else (3 * i + 2) % 16, (0,)))
    return out


def lay_out(sources):
    """The sources cut from one arena of random bytes -> (arena uint8, offsets).  The first long enough stereo source of each law holds
    all 256 codes in each channel."""
    rng = np.random.default_rng(47)
    offs, at = [], 0
    for codec, ch, m, mis, _ in sources:
        at = (at + 15) // 16 * 16 + mis
        offs.append(at)
        at += m * ch * (2 if codec == S16 else 1) + int(rng.integers(0, 40))
    arena = rng.integers(0, 256, size=at + 64, dtype=np.uint8)
    for law in (ULAW, ALAW):
        r = next(i for i, (c, ch, m, _, w) in enumerate(sources) if c == law and ch == 2 and m >= 256 and w == (0, 1))
        arena[offs[r]:offs[r] + 512:2] = np.arange(256, dtype=np.uint8)
        arena[offs[r] + 1:offs[r] + 512:2] = np.arange(256, dtype=np.uint8)[::-1]
    return arena, np.asarray(offs, dtype=np.int64)


def expected(sources, arena, offs, dst_row, n_dst):
    from silero_vad_amd import deinterleave
    want = np.full((n_dst, WIDTH), FILL, dtype=np.int16)
    named = {}
    for i, ((codec, ch, m, _, _), o) in enumerate(zip(sources, offs)):
        raw = arena[o:o + m * ch * (2 if codec == S16 else 1)].copy()
        raw = raw.view(np.int16) if codec == S16 else raw
        for c in range(ch):
            r = int(dst_row[i, c])
            if r >= 0:
                want[r] = 0
                want[r, :m] = deinterleave(raw, ch, c, LAW_NAME[codec])
                named[r] = (i, c)
    return want, named


def tables(base_ptr, offs, lens):
    n = len(lens)
    rows = (ctypes.c_void_p * n)(*[base_ptr + int(o) if m else None for o, m in zip(offs, lens)])
    return rows, (ctypes.c_long * n)(*[int(m) for m in lens])


@pytest.mark.parametrize("how", [1, 2])
def test_gather_channels_kernel(model, how):
    from silero_vad_amd import _lib
    eng = model.engine
    sources = kernel_sources()
    n = len(sources)
    assert 55 <= n <= 70
    assert {mis for c, ch, m, mis, _ in sources if c != S16 and ch == 2 and m} == set(range(16))
    assert {mis for c, ch, m, mis, _ in sources if c == S16 and ch == 2 and m} == set(range(0, 16, 2))
    assert sum(s[4] == (0,) and s[1] == 2 for s in sources) >= 3 and sum(s[4] == (1,) for s in sources) >= 3
    arena, offs = lay_out(sources)
    # the destination rows: a permutation of the wanted channels over a batch with a few rows that nobody names
    wanted = [(i, c) for i, s in enumerate(sources) for c in s[4]]
    n_dst = len(wanted) + 5
    perm = np.random.default_rng(3).permutation(n_dst)[:len(wanted)]
    assert not np.array_equal(perm, np.arange(len(wanted)))
    dst_row = np.full((n, 2), -1, dtype=np.int32)
    for (i, c), r in zip(wanted, perm):
        dst_row[i, c] = r
    want, named = expected(sources, arena, offs, dst_row, n_dst)
    host = torch.from_numpy(arena).pin_memory()
    src = host if how == 1 else host.cuda()
    assert src.data_ptr() % 16 == 0
    frames = [m for _, _, m, _, _ in sources]
    codecs = np.array([s[0] for s in sources], dtype=np.uint8)
    chans = np.array([s[1] for s in sources], dtype=np.uint8)
    rp, lp = tables(src.data_ptr(), offs, frames)
    dst = torch.full((n_dst, WIDTH), FILL, dtype=torch.int16, device="cuda")
    eng.upload_rows_channels(rp, lp, codecs, chans, dst_row, n, n_dst, WIDTH, dst, how)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    for r, (i, c) in sorted(named.items()):                     # row by row first: a failure names the row
        codec, ch, m, mis, _ = sources[i]
        assert np.array_equal(got[r], want[r]), (r, i, c, codec, ch, m, mis, int(np.flatnonzero(got[r] != want[r])[0]))
    assert np.array_equal(got, want)
    spare = [r for r in range(n_dst) if r not in named]
    assert len(spare) == 5 and bool((got[spare] == FILL).all())

    # every source mono, dst_row the identity: the batch of upload_rows_coded
    mono = [i for i, s in enumerate(sources) if s[1] == 1] + [i for i, s in enumerate(sources) if s[1] == 2]
    m_offs = offs[mono]
    m_len = [min(sources[i][2] * sources[i][1], WIDTH) for i in mono]
    m_cd = np.ascontiguousarray(codecs[mono])
    rp, lp = tables(src.data_ptr(), m_offs, m_len)
    plain = torch.full((len(mono), WIDTH), FILL, dtype=torch.int16, device="cuda")
    eng.upload_rows_coded(rp, lp, m_cd, len(mono), WIDTH, plain, how)
    ident = np.stack([np.arange(len(mono)), np.full(len(mono), -1)], axis=1).astype(np.int32)
    for ch_arg in (None, np.ones(len(mono), dtype=np.uint8)):
        split = torch.full((len(mono), WIDTH), FILL, dtype=torch.int16, device="cuda")
        eng.upload_rows_channels(rp, lp, m_cd, ch_arg, ident, len(mono), len(mono), WIDTH, split, how)
        torch.cuda.synchronize()
        assert torch.equal(split, plain)

    # refusals: status 1, nothing is queued, dst keeps its bytes
    dst.fill_(FILL)
    rp, lp = tables(src.data_ptr(), offs, frames)
    st = next(i for i, s in enumerate(sources) if s[1] == 2 and s[4] == (0, 1) and s[2] > 0)
    mo = next(i for i, s in enumerate(sources) if s[1] == 1)
    odd_s16 = next(i for i, s in enumerate(sources) if s[0] != S16 and s[3] % 2 == 1 and s[2] > 0)

    def changed(a, i, v):
        b = a.copy()
        b.reshape(-1)[i] = v
        return b

    too_long = (ctypes.c_long * n)(*[WIDTH + 1 if i == st else m for i, m in enumerate(frames)])
    null_row = (ctypes.c_void_p * n)(*[None if i == st else rp[i] for i in range(n)])
    twice = changed(dst_row, 2 * st + 1, dst_row[st, 0])
    cases = {"how 0": (rp, lp, codecs, chans, dst_row, 0),
             "codec 3": (rp, lp, changed(codecs, st, 3), chans, dst_row, how),
             "channels 0": (rp, lp, codecs, changed(chans, st, 0), dst_row, how),
             "channels 3": (rp, lp, codecs, changed(chans, st, 3), dst_row, how),
             "row -2": (rp, lp, codecs, chans, changed(dst_row, 2 * st, -2), how),
             "row n_dst": (rp, lp, codecs, chans, changed(dst_row, 2 * st, n_dst), how),
             "row twice": (rp, lp, codecs, chans, twice, how),
             "absent channel": (rp, lp, codecs, chans, changed(dst_row, 2 * mo + 1, spare[0]), how),
             "frames > width": (rp, too_long, codecs, chans, dst_row, how),
             "null row": (null_row, lp, codecs, chans, dst_row, how),
             "odd int16": (rp, lp, changed(codecs, odd_s16, S16), chans, dst_row, how)}
    for name, (a_rows, a_len, a_cd, a_ch, a_dst, a_how) in cases.items():
        with pytest.raises(_lib.VadError) as err:
            eng.upload_rows_channels(a_rows, a_len, a_cd, a_ch, a_dst, n, n_dst, WIDTH, dst, a_how)
        assert err.value.status == 1, name                     # VAD_ERR_ARG
    for a_width, a_dst in ((WIDTH - 4, dst), (WIDTH, dst.reshape(-1)[1:])):      # a pitch / a dst that is not 16-byte aligned
        with pytest.raises(_lib.VadError) as err:
            short = (ctypes.c_long * n)(*[min(m, 8) for m in frames])
            eng.upload_rows_channels(rp, short, codecs, chans, dst_row, n, n_dst - 1, a_width, a_dst, how)
        assert err.value.status == 1
    torch.cuda.synchronize()
    assert bool((dst == FILL).all())


def make_containers(kind, recs, chans, twins):
    """(interleaved recordings, their de-interleaved int16 twins) in one kind of container"""
    from silero_vad_amd import PackedRecordings
    if kind == "arena":                                        # a pinned arena, packed back to back: the window route
        lens = np.array([len(r) for r in recs], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        base = torch.zeros(int(lens.sum()) + 16, dtype=torch.from_numpy(recs[0]).dtype).pin_memory()
        # the twin: an int16 arena in which the channels of a recording occupy, back to back, the range its frames occupy
        base16 = torch.zeros(base.numel(), dtype=torch.int16).pin_memory()
        t_offs, t_lens, k = [], [], 0
        for o, r, C in zip(offs, recs, chans):
            base[o:o + len(r)] = torch.from_numpy(r)
            for c in range(C):
                x = twins[k]
                base16[o + c * len(x):o + (c + 1) * len(x)] = torch.from_numpy(x)
                t_offs.append(int(o) + c * len(x))
                t_lens.append(len(x))
                k += 1
        assert len({int(o) * base.element_size() % 16 for o in offs}) > 4      # most recordings start at a misaligned byte
        return PackedRecordings(base, offs, lens), PackedRecordings(base16, np.array(t_offs), np.array(t_lens))
    if kind == "pinned":                                       # separately pinned tensors: the gather over PCIe (how = 1)
        return [torch.from_numpy(r).pin_memory() for r in recs], [torch.from_numpy(x).pin_memory() for x in twins]
    return [torch.from_numpy(r) for r in recs], [torch.from_numpy(x) for x in twins]      # pageable: staged


@pytest.mark.parametrize("kind", ["arena", "pinned", "pageable"])
@pytest.mark.parametrize("tag", ["8k", "16k"])
def test_corpus_routes_equal_their_twins(model, oracle, tag, kind):
    """24 recordings of 3 ... 40 chunks with odd tails: 12 of int16 samples and 12 of G.711 codes (both laws), in each group two of
    three stereo.  One call holds one kind of sample (uint8 codes and int16 samples in one call are refused as "mixed"), so each group
    is a call of its own."""
    from silero_vad_amd import ragged_probs, ragged_speech_segments, refill_probs, refill_speech_segments, streams
    sr = SRS[tag]
    n = 512 if sr == 16000 else 256
    scan = dict(threshold=0.3, min_speech_duration_ms=64)
    for law in ("s16", "g711"):
        recs, chans, laws, twins = stereo_recordings(tag, law, count=12, lo=3, hi=40, seed=13, single_frame=False)
        assert chans.count(2) == 8 and (law == "s16" or set(laws) == {"ulaw", "alaw"})
        codec = None if law == "s16" else laws
        inter, twin = make_containers(kind, recs, chans, twins)
        link = {}
        for name, call in (("ragged_probs", lambda a, **kw: ragged_probs(a, model, sr, **kw)),
                           ("refill_probs", lambda a, **kw: refill_probs(a, model, sr, slots=8, slab_chunks=4, **kw)),
                           ("ragged_speech_segments", lambda a, **kw: ragged_speech_segments(a, model, sr, **scan, **kw)),
                           ("refill_speech_segments", lambda a, **kw: refill_speech_segments(a, model, sr, slots=8, slab_chunks=4, **scan, **kw))):
            streams.STATS.clear()
            got = call(inter, codec=codec, channels=chans)
            link[name] = [streams.STATS["h2d_bytes"], streams.STATS["refill_window_feed"]]
            streams.STATS.clear()
            want = call(twin)
            link[name] += [streams.STATS["h2d_bytes"], streams.STATS["refill_window_feed"]]
            assert len(got) == len(want) == len(twins)
            if name.endswith("probs"):
                for i, (p, q) in enumerate(zip(got, want)):
                    assert p.shape == ((len(twins[i]) + n - 1) // n,) and torch.equal(p, q), (law, name, i)
                if name == "ragged_probs":
                    probs = got
            else:
                assert got == want and any(want), (law, name)
        # the routes taken: the interleaved bytes cross the link once, on the route of the twin
        for name, (b, feed, b_twin, feed_twin) in link.items():
            assert 0 < b <= b_twin and feed == feed_twin, (law, name, link[name])
            if law == "g711":
                assert 2 * b <= b_twin, (name, link[name])                  # one byte a sample
            if kind == "arena" and name.startswith("refill"):
                assert feed == 1, name
        if law == "g711":
            # three channels, among them both channels of one stereo recording, against the CPU oracle on the expanded audio
            assert chans[0] == 2 and chans[2] == 1
            for i in (0, 1, 4):
                x = twins[i].astype(np.float32) / 32768.0
                want = oracle.audio_forward(np.pad(x, (0, -len(x) % n))[None], sr)[0]
                assert np.abs(probs[i].numpy() - want).max() < TIGHT, i


def route_corpora():
    """Six recordings of 2 ... 6 chunks with odd tails at 16 kHz, three times over: as plain int16, as G.711 codes of both laws, as
    interleaved int16 (every third one mono) -> {format: (recordings, codec, channels, int16 twins)}.  (The seed: packed back to back,
    most recordings of every format start at a misaligned byte, which make_containers asserts.)"""
    from silero_vad_amd import g711_expand
    from test_corpus_g711 import LAWS, encode
    recs, chans, _, twins = stereo_recordings("16k", "s16", count=6, lo=2, hi=6, seed=23, single_frame=False)
    plain = [twins[sum(chans[:i])] for i in range(6)]           # (a recording's first channel)
    assert chans.count(2) == 4 and all(512 < len(x) <= 6 * 512 and len(x) % 512 for x in plain)
    laws = [LAWS[i % 2] for i in range(6)]
    codes = [encode(x, lw) for x, lw in zip(plain, laws)]
    expanded = [g711_expand(c, lw) for c, lw in zip(codes, laws)]
    return {"plain": (plain, None, None, plain), "g711": (codes, laws, None, expanded), "stereo": (recs, None, chans, twins)}


# which engine method carries a batch, and with which `how` (0 one DMA per row, 1 the gather kernel over the link, 2 the gather kernel
# over device memory): by sample format and by where the bytes lie.  None: no upload call at all -- ONE copy straight into the batch.
METHOD = {"plain": "upload_rows", "g711": "upload_rows_coded", "stereo": "upload_rows_channels"}
HOW = {"arena": {"plain": 2, "g711": 2, "stereo": 2},           # cut from an arena window's device copy
       "pinned": {"plain": 1, "g711": 1, "stereo": 1},          # scattered page-locked recordings
       "pageable": {"plain": None, "g711": 2, "stereo": 2},     # staged: the codes / the interleaved bytes into a block behind the batch
       "dma": {"plain": 0, "g711": 1, "stereo": 1}}             # SILERO_VAD_AMD_UPLOAD=dma: a DMA neither expands nor splits


@pytest.mark.parametrize("kind", ["arena", "pinned", "pageable", "dma"])
def test_every_route_calls_its_upload(model, monkeypatch, kind):
    """Each cell of the ingest matrix -- plain int16 / G.711 / interleaved recordings x arena windows / scattered pinned / pageable --
    reaches HBM through the engine method and the `how` that the matrix names, in the bucket scheduler and in the refill scheduler.
    So few recordings do not pass the window routes' density rule on their own: the arena runs under SILERO_VAD_AMD_UPLOAD=window.
    Under SILERO_VAD_AMD_UPLOAD=dma plain pinned recordings take one DMA per row; coded and interleaved ones cannot, say so in a
    warning, take the gather kernel and give the gather run's probabilities."""
    import warnings
    from silero_vad_amd import ragged_probs, refill_probs
    calls = []
    for name in METHOD.values():
        def counting(*a, _name=name, _real=getattr(model.engine, name), **kw):
            calls.append((_name, kw["how"] if "how" in kw else a[-1]))
            return _real(*a, **kw)
        monkeypatch.setattr(model.engine, name, counting)
    schedulers = {"ragged_probs": lambda a, **kw: ragged_probs(a, model, 16000, **kw),
                  "refill_probs": lambda a, **kw: refill_probs(a, model, 16000, slots=4, slab_chunks=2, **kw)}
    for fmt, (recs, codec, chans, twins) in route_corpora().items():
        n_rows = len(twins)
        inter, _ = make_containers("pinned" if kind == "dma" else kind, recs, chans or [1] * 6, twins)
        results = {}
        for name, call in schedulers.items():
            monkeypatch.delenv("SILERO_VAD_AMD_UPLOAD", raising=False)
            if kind == "dma":
                results["gather"] = call(inter, codec=codec, channels=chans)
            if kind in ("arena", "dma"):
                monkeypatch.setenv("SILERO_VAD_AMD_UPLOAD", "window" if kind == "arena" else "dma")
            del calls[:]
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                results[name] = got = call(inter, codec=codec, channels=chans)
            want = HOW[kind][fmt]
            assert len(got) == n_rows
            assert set(calls) == (set() if want is None else {(METHOD[fmt], want)}), (fmt, name, sorted(set(calls)))
            downgraded = [w for w in caught if "SILERO_VAD_AMD_UPLOAD=dma" in str(w.message)]
            assert len(downgraded) == (1 if kind == "dma" and fmt != "plain" else 0), (fmt, name, [str(w.message) for w in caught])
            for i, (p, q) in enumerate(zip(got, results.get("gather", got))):
                assert torch.equal(p, q), (fmt, name, i)
        for i, (p, q) in enumerate(zip(results["ragged_probs"], results["refill_probs"])):      # (both are the single call's bits)
            assert p.numel() > 1 and torch.equal(p, q), (fmt, i)


def test_raw_48k_stereo_arena(model):
    import warnings
    from silero_vad_amd import ragged_probs
    recs, chans, laws, twins = stereo_recordings("16k", "s16", count=12, lo=2, hi=8, seed=17, per=3, single_frame=False)
    inter, twin = make_containers("arena", recs, chans, twins)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got, want = ragged_probs(inter, model, 48000, channels=chans), ragged_probs(twin, model, 48000)
    assert len(got) == len(want) == len(twins)
    for i, (p, q) in enumerate(zip(got, want)):
        assert p.shape == ((len(twins[i]) + 1535) // 1536,) and torch.equal(p, q), i
