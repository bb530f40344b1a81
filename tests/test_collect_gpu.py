"""The audio the segments keep, collected on the device: the segment-driven gather (vad_collect_segments_device,
csrc/kernel_collect.hip) with hand-made segment tables against numpy slices, and `ragged_speech_audio` on every ingest form against
`ragged_speech_segments` of the same call plus `collect_chunks` / `drop_chunks` on the host twin.  Everything is a copy: all comparisons
are bit for bit.
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import GOLD
from test_corpus_g711 import encode
from test_corpus_stereo import stereo_recordings

pytestmark = pytest.mark.gpu

CAP = 24
ROOM = 13000                     # 16 kHz samples of a batch row: a little over three output tiles of int16 (4 096 samples each)
TILE_BYTES = 8192
FILL16, FILL32 = 0x5A5A, 0x5A5A5A5A


@pytest.fixture(scope="module")
def model(built):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback to silently pass on)")
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    assert m.engine._h, "native engine not created"
    return m


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def kernel_rows(esz):
    """[(name, audio_len, segments, count the table claims)]: the rows of the kernel test, in 16 kHz samples.  V: elements of a lane's
    16 bytes, T: elements of an 8 KiB output tile."""
    V, T = 16 // esz, TILE_BYTES // esz
    rng = np.random.default_rng(100 + esz)
    rows = []
    for m in range(V):                                         # a long first segment at every element offset modulo 16 bytes
        rows.append((f"start{m}", ROOM, [(40 * V + m, 40 * V + m + 300), (500 * V + (m + 3) % V, 500 * V + (m + 3) % V + 5 * V + 1)], None))
    rows.append(("tiny", ROOM, [(10, 10), (20, 21), (40, 47), (60, 68), (80, 89), (200, 200 + 2 * V)], None))     # lengths 0, 1, 7, 8, 9
    for k, n in enumerate((T - 1, T, T + 1)):                  # one less than, equal to, one more than a tile
        rows.append((f"tile{n - T:+d}", ROOM, [(3 + k, 3 + k + n)], None))
    rows.append(("three_tiles", ROOM, [(77, 77 + 2 * T + 500)], None))
    short, at = [], 5
    for k in range(CAP):                                       # many short segments in one tile: lanes straddle two and three of them
        n = (5, 6, 3, 2, 3, 1, 2, 7)[k % 8]
        short.append((at, at + n))
        at += n + (1, 5, 2, 9, 4)[k % 5]
    rows.append(("short", ROOM, short, None))                  # ... and counts == cap
    rows.append(("none", ROOM, [], None))
    rows.append(("over_cap", ROOM, [(10 * k, 10 * k + 4) for k in range(CAP)], CAP + 3))
    rows.append(("no_audio", 0, [(0, 100), (200, 300)], None))
    rows.append(("clamped", 9000, [(100, 1100), (8000, 12000)], None))
    rows.append(("at_zero_to_end", ROOM - 5, [(0, 64), (ROOM - 100, ROOM - 5)], None))
    rows.append(("whole", ROOM, [(0, ROOM)], None))
    while len(rows) < 40:                                      # random ordered, disjoint lists
        n = int(rng.integers(1, CAP + 1))
        alen = int(rng.integers(ROOM // 2, ROOM + 1))
        cuts = np.sort(rng.choice(alen + 1, size=2 * n, replace=False))
        rows.append((f"random{len(rows)}", alen, [(int(cuts[2 * k]), int(cuts[2 * k + 1])) for k in range(n)], None))
    return rows


def keeps(x, segs, invert):
    """collect_chunks / drop_chunks on a numpy signal"""
    if not invert:
        parts = [x[a:b] for a, b in segs]
    else:
        parts, cur = [], 0
        for a, b in segs:
            parts.append(x[cur:a])
            cur = b
        parts.append(x[cur:])
    return np.concatenate(parts) if parts else x[:0]


def part_runs(alen, segs, invert):
    """the non-empty runs [a, b) of a row's output, in output order (for the coverage assertions only)"""
    runs, cur = [], 0
    for a, b in segs:
        a, b = min(a, alen), min(b, alen)
        runs.append((cur, a) if invert else (a, b))
        cur = b
    if invert:
        runs.append((cur, alen))
    return [(a, b) for a, b in runs if b > a]


def check_coverage(rows, esz, invert, counts, alens, want_kept):
    """the kernel test's own coverage: what its rows are there for does occur"""
    V, T = 16 // esz, TILE_BYTES // esz
    live = {i: part_runs(r[1], r[2], invert) for i, r in enumerate(rows) if r[3] is None}
    mis = set()
    for runs in live.values():
        before = 0
        for a, b in runs:
            mis.add((a - before) % V)                          # where in its 16-byte granule a lane's source starts (step 1)
            before += b - a
    assert mis == set(range(V)), mis                           # every source misalignment: eight for int16, four for float32
    name_of = {r[0]: i for i, r in enumerate(rows)}
    ends = np.cumsum([b - a for a, b in live[name_of["short"]]])
    spans = set()
    for o in range(0, int(ends[-1]) - V + 1, V):               # parts that a lane's vector touches in the row of short segments
        spans.add(int(np.searchsorted(ends, o + V - 1, side="right") - np.searchsorted(ends, o, side="right")) + 1)
    assert {2, 3} <= spans, spans
    lens = {b - a for r in rows if r[3] is None for a, b in r[2]}
    assert {0, 1, 7, 8, 9, T - 1, T, T + 1} <= lens and max(lens) >= 2 * T + 500, lens
    assert counts[name_of["short"]] == CAP and counts[name_of["over_cap"]] > CAP and counts[name_of["none"]] == 0
    assert alens[name_of["no_audio"]] == 0 and rows[name_of["clamped"]][2][-1][1] > alens[name_of["clamped"]]
    assert (want_kept > 2 * T).sum() >= 2 and (want_kept == 0).sum() >= 1 and (want_kept == -1).sum() == 1


def fill(shape, esz, seed):
    """random samples, every one distinguishable enough: int16 values, or float32 built from distinct bit patterns; as integer bits"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if esz == 2:
        return rng.integers(-32768, 32768, size=n).astype(np.int16).reshape(shape)
    bits = (rng.permutation(n).astype(np.uint32) * np.uint32(2654435761)).view(np.int32)
    assert len(np.unique(bits)) == n
    return bits.reshape(shape)


def launch(L, eng, x, esz, ld, step, alen, segs, counts, invert, kept, offs, out):
    from silero_vad_amd import _lib
    _lib.check(eng._h, L.vad_collect_segments_device(
        eng._h, x.data_ptr(), esz, ld, step, len(alen), alen.data_ptr(), segs.data_ptr(), segs.shape[1], counts.data_ptr(), invert,
        kept.data_ptr(), offs.data_ptr() if offs is not None else None, out.data_ptr() if out is not None else None,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


@pytest.mark.parametrize("invert", [0, 1], ids=["collect", "drop"])
@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("esz", [2, 4], ids=["i16", "f32"])
def test_collect_segments_kernel(model, esz, step, invert):
    from silero_vad_amd import _lib
    L, eng = _lib.lib(), model.engine
    V, T = 16 // esz, TILE_BYTES // esz
    rows = kernel_rows(esz)
    B = len(rows)
    assert B == 40 and 3 * T < ROOM
    ld = (ROOM * step + 7) // 8 * 8 + 8                        # raw-rate elements of a row: a multiple of 16 bytes, a few tiles wide
    bits = np.int16 if esz == 2 else np.int32
    pcm = fill((B, ld), esz, 7 * esz + step)
    seg_tab = np.full((B, CAP, 2), -12345, dtype=np.int64)     # (entries behind a row's count are never read)
    counts = np.zeros(B, dtype=np.int64)
    alens = np.asarray([r[1] for r in rows], dtype=np.int64)
    want = []
    for i, (name, alen, segs, claimed) in enumerate(rows):
        seg_tab[i, :len(segs)] = np.asarray(segs, dtype=np.int64).reshape(-1, 2)
        counts[i] = len(segs) if claimed is None else claimed
        want.append(None if claimed is not None else keeps(pcm[i, ::step][:alen], segs, invert))
    want_kept = np.asarray([-1 if w is None else len(w) for w in want], dtype=np.int64)

    check_coverage(rows, esz, invert, counts, alens, want_kept)

    # offsets: every row on a 16-byte boundary, with gaps of different sizes between the rows
    padded = (np.maximum(want_kept, 0) + V - 1) // V * V
    gaps = V * (np.arange(B) % 3)
    offs = np.concatenate([[2 * V], 2 * V + np.cumsum(padded + gaps)[:-1]]).astype(np.int64)
    assert (offs * esz % 16 == 0).all() and len(np.unique(offs * esz % 64)) > 1
    total = int(offs[-1] + padded[-1]) + 5 * V
    fillv = FILL16 if esz == 2 else FILL32

    dev = model.device
    x = torch.from_numpy(pcm).to(dev)
    d_seg, d_cnt, d_len, d_off = (torch.from_numpy(a).to(dev) for a in (seg_tab, counts, alens, offs))
    kept = torch.full((B,), -777, dtype=torch.int64, device=dev)
    out = torch.full((total,), fillv, dtype=torch.int16 if esz == 2 else torch.int32, device=dev)
    launch(L, eng, x, esz, ld, step, d_len, d_seg, d_cnt, invert, kept, None, None)                  # count
    torch.cuda.synchronize()
    got_kept = kept.cpu().numpy()
    assert np.array_equal(got_kept, want_kept), np.flatnonzero(got_kept != want_kept)
    assert (out.cpu().numpy() == fillv).all()                                                         # (the count phase writes no audio)
    launch(L, eng, x, esz, ld, step, d_len, d_seg, d_cnt, invert, kept, d_off, out)                   # gather
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(bits)
    untouched = np.ones(total, dtype=bool)
    for i, w in enumerate(want):
        if w is None or not len(w):
            continue
        o = int(offs[i])
        bad = np.flatnonzero(got[o:o + len(w)] != w.view(bits))
        assert not len(bad), (rows[i][0], len(w), bad[:8])
        untouched[o:o + len(w)] = False
    assert (got[untouched] == np.array(fillv).astype(bits)).all(), np.flatnonzero(untouched & (got != np.array(fillv).astype(bits)))[:8]


@pytest.mark.parametrize("step,invert", [(1, False), (3, True)])
def test_collect_chunks_device(model, step, invert):
    """the Python form of the two phases: its own offsets, rows over the cap handed back as -1"""
    from silero_vad_amd import collect_chunks_device
    rows = kernel_rows(2)
    B, ld = len(rows), ROOM * step
    pcm = fill((B, ld + 8), 2, 31)
    seg_tab = np.zeros((B, CAP, 2), dtype=np.int64)
    counts = np.zeros(B, dtype=np.int64)
    for i, (_, _, segs, claimed) in enumerate(rows):
        seg_tab[i, :len(segs)] = np.asarray(segs, dtype=np.int64).reshape(-1, 2)
        counts[i] = len(segs) if claimed is None else claimed
    alens = np.asarray([r[1] for r in rows], dtype=np.int64)
    dev = model.device
    x = torch.from_numpy(pcm).to(dev)[:, :ld]                   # (a view: the rows' pitch is not their width)
    out, offs, kept = collect_chunks_device(model.engine, x, torch.from_numpy(seg_tab).to(dev), torch.from_numpy(counts).to(dev),
                                            torch.from_numpy(alens).to(dev), step=step, invert=invert)
    out, offs, kept = out.cpu().numpy(), offs.cpu().numpy(), kept.cpu().numpy()
    assert (offs % 8 == 0).all()
    for i, (name, alen, segs, claimed) in enumerate(rows):
        if claimed is not None:
            assert kept[i] == -1
            continue
        w = keeps(pcm[i, :ld:step][:alen], segs, invert)
        assert kept[i] == len(w), name
        assert np.array_equal(out[offs[i]:offs[i] + kept[i]], w), name


# ---- end to end --------------------------------------------------------------------------------------------------------------------
SHRED = dict(min_speech_duration_ms=0, min_silence_duration_ms=0, speech_pad_ms=0, max_speech_duration_s=0.1)


def cuts():
    """a dozen recordings of 1 ... 6 s cut from the fixture at odd offsets, odd lengths, one of them all zeros -> int16 arrays"""
    pcm = np.load(GOLD / "audio_16k.npz")["pcm"]
    rng = np.random.default_rng(23)
    out = []
    for k in range(12):
        n = int(rng.integers(16000, 96001)) | 1
        a = int(rng.integers(0, len(pcm) - n)) | 1
        out.append(pcm[a:a + n].copy())
    out[0] = pcm[100001:100001 + 96001].copy()                 # a full 6 s
    out[1] = pcm[200001:200001 + 20001].copy()                 # ... and a short one
    out[5] = np.zeros(30001, dtype=np.int16)
    return out


def forms():
    """name -> (recordings as the call takes them, call arguments, the flat list of 16 kHz twins)"""
    from silero_vad_amd import PackedRecordings, g711_expand
    base = cuts()
    lens = np.asarray([len(x) for x in base], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens + 3)[:-1]]).astype(np.int64)      # back to back with odd gaps: misaligned rows
    arena = torch.zeros(int(offs[-1] + lens[-1]), dtype=torch.int16).pin_memory()
    for o, x in zip(offs, base):
        arena[int(o):int(o) + len(x)] = torch.from_numpy(x)
    out = {"i16_arena": (PackedRecordings(arena, offs, lens), {}, base),
           "i16_pageable": ([torch.from_numpy(x) for x in base], {}, base),
           "f32": ([torch.from_numpy(x.astype(np.float32) / 32768.0) for x in base], {}, [x.astype(np.float32) / 32768.0 for x in base])}
    codes = [encode(x, "ulaw") for x in base]
    out["ulaw"] = ([torch.from_numpy(c) for c in codes], {"codec": "ulaw"}, [g711_expand(c, "ulaw") for c in codes])
    recs, chans, _, twins = stereo_recordings("16k", "s16", count=6, lo=30, hi=120, seed=29, single_frame=False)
    out["stereo"] = ([torch.from_numpy(r) for r in recs], {"channels": chans}, twins)
    out["48k"] = ([torch.from_numpy(np.repeat(x, 3)) for x in base[:6]], {"sampling_rate": 48000}, base[:6])
    return out


@pytest.fixture(scope="module")
def corpus(model):
    return forms()


def twin_keeps(segments, twins, nonspeech):
    return [keeps(np.asarray(t), [(d["start"], d["end"]) for d in sg], nonspeech) for sg, t in zip(segments, twins)]


def same_audio(audio, want):
    assert len(audio) == len(want)
    for i, (a, w) in enumerate(zip(audio, want)):
        a = a.cpu()
        assert a.dim() == 1 and a.dtype == (torch.int16 if w.dtype == np.int16 else torch.float32), i
        view = np.int16 if w.dtype == np.int16 else np.int32
        assert np.array_equal(a.numpy().view(view), np.ascontiguousarray(w).view(view)), i


@pytest.mark.parametrize("form", ["i16_arena", "i16_pageable", "f32", "ulaw", "stereo", "48k"])
def test_ragged_speech_audio(model, corpus, form):
    from silero_vad_amd import ragged_probs, ragged_speech_audio, ragged_speech_segments
    recs, kw, twins = corpus[form]
    # what the unchanged calls return, before any call of the new one ...
    seg_before = ragged_speech_segments(recs, model, **kw)
    probs_before = ragged_probs(recs, model, **kw)
    segments, audio = ragged_speech_audio(recs, model, **kw)
    assert segments == seg_before
    assert sum(len(s) for s in segments) >= 3
    same_audio(audio, twin_keeps(segments, twins, False))
    if form != "stereo":
        assert not segments[5] and audio[5].numel() == 0                    # the all-zero recording: an empty tensor, no exception
    # ... on the device: the same bytes, left there
    seg_dev, audio_dev = ragged_speech_audio(recs, model, on_device=True, **kw)
    assert seg_dev == seg_before and all(a.is_cuda for a in audio_dev)
    same_audio(audio_dev, twin_keeps(segments, twins, False))
    # ... everything but the speech
    seg_non, audio_non = ragged_speech_audio(recs, model, keep="nonspeech", **kw)
    assert seg_non == seg_before
    same_audio(audio_non, twin_keeps(segments, twins, True))
    for a, b, t in zip(audio, audio_non, twins):
        assert a.numel() + b.numel() == len(t)
    # ... as arrays
    (cnt, flat), audio_arr = ragged_speech_audio(recs, model, as_arrays=True, **kw)
    c2, f2 = ragged_speech_segments(recs, model, as_arrays=True, **kw)
    assert np.array_equal(cnt, c2) and np.array_equal(flat, f2)
    same_audio(audio_arr, twin_keeps(segments, twins, False))
    # ... and the unchanged calls again, after
    assert ragged_speech_segments(recs, model, **kw) == seg_before
    probs_after = ragged_probs(recs, model, **kw)
    assert len(probs_after) == len(probs_before) and all(torch.equal(a, b) for a, b in zip(probs_after, probs_before))


@pytest.mark.parametrize("form", ["i16_arena", "ulaw", "stereo", "48k"])
def test_rows_over_the_cap_are_collected_on_the_host(model, corpus, form):
    """Scan arguments that shred the speech -- no minimum durations, no padding, and a maximum speech duration of 0.1 s, which cuts
    every stretch of speech into pieces of two or three chunks (on this fixture no threshold alone gives a recording more than a
    handful of segments) -- so that one bucket holds recordings over the scan's optimistic room of 24 segments, which the device
    leaves to the host, beside recordings under it."""
    from silero_vad_amd import ragged_speech_audio, ragged_speech_segments
    from silero_vad_amd.streams import STATS
    recs, kw, twins = corpus[form]
    want_seg = ragged_speech_segments(recs, model, **kw, **SHRED)
    n = [len(s) for s in want_seg]
    assert max(n) > 24 and min(n) < 24 and sum(0 < k <= 24 for k in n) >= 1, n             # the precondition
    for nonspeech in (False, True):
        before = STATS["collect_host_rows"]
        segments, audio = ragged_speech_audio(recs, model, keep="nonspeech" if nonspeech else "speech", **kw, **SHRED)
        assert segments == want_seg
        assert STATS["collect_host_rows"] - before == sum(k > 24 for k in n)
        same_audio(audio, twin_keeps(segments, twins, nonspeech))
    segments, audio = ragged_speech_audio(recs, model, on_device=True, **kw, **SHRED)
    assert segments == want_seg and all(a.is_cuda for a in audio)
    same_audio(audio, twin_keeps(segments, twins, False))
