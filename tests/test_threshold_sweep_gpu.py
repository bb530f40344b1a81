"""The enter / exit threshold sweep on the device: the kernel (vad_threshold_counts_device, csrc/kernel_sweep.hip) against the host
twin on the shape list of tests/test_threshold_sweep.py, all four outputs as integers; the reference's recorded triples through
`threshold_counts_device`; and `ragged_threshold_counts` on every ingest form against `threshold_counts` on `ragged_probs` of the same
call, bit for bit.
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import GOLD
from test_corpus_g711 import encode
from test_corpus_stereo import stereo_recordings
from test_threshold_sweep import (IGNORE, PAIR_COUNTS, TILE, as_batch, fixture_sets, host_counts, kernel_layout, kernel_pairs, kernel_rows,
                                  same_counts)

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
GUARD = 64


@pytest.fixture(scope="module")
def model(built):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback to silently pass on)")
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    assert m.engine._h, "native engine not created"
    return m


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def device_counts(model, flat, ldp, offs, nck, lab, l_off, pairs):
    """one launch -> (tp, tn, n_pos, n_valid) as numpy; every output sits between guard words that must come back untouched"""
    from silero_vad_amd import _lib
    L, dev = _lib.lib(), model.device
    B, P = len(nck), len(pairs.enter)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (flat, nck, lab, l_off, pairs.enter_f32, pairs.exit_f32)]
    d_off = torch.from_numpy(offs).to(dev) if offs is not None else None
    sizes = (B * P, B * P, B, B)
    outs = [torch.full((n + 2 * GUARD,), FILL, dtype=torch.int32, device=dev) for n in sizes]
    _lib.check(model.engine._h, L.vad_threshold_counts_device(
        model.engine._h, d[0].data_ptr(), ldp, d_off.data_ptr() if d_off is not None else None, B, d[1].data_ptr(), d[2].data_ptr(),
        d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), P, *(o.data_ptr() + 4 * GUARD for o in outs),
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize()
    res = []
    for o, n in zip(outs, sizes):
        a = o.cpu().numpy()
        assert (a[:GUARD] == FILL).all() and (a[GUARD + n:] == FILL).all()         # nothing outside the rows x pairs rectangle
        assert (a[GUARD:GUARD + n] != FILL).all()                                   # ... and every cell of it written
        res.append(a[GUARD:GUARD + n])
    return res[0].reshape(B, P), res[1].reshape(B, P), res[2], res[3]


@pytest.mark.parametrize("P", PAIR_COUNTS)
def test_sweep_kernel_against_the_host_twin(model, P):
    from silero_vad_amd import _lib
    L, rows, pairs = _lib.lib(), kernel_rows(), kernel_pairs(P)
    names = [r[0] for r in rows]
    assert {len(r[2]) for r in rows} >= {0, 1, 3, TILE - 1, TILE, TILE + 1, 3 * TILE + 5}
    assert {(len(r[2]), r[1]) for r in rows} >= {(n, m) for n in (1, TILE, 3 * TILE + 5) for m in range(4)}
    assert any(np.isnan(r[2]).any() for r in rows) and "all_ignored@1" in names and "band@1" in names
    # rows at their start offsets modulo 16 bytes in one flat buffer, NaN and 1.0 in the gaps between them
    flat, offs, nck, lab, l_off = kernel_layout(rows)
    assert {int(o) % 4 for o in offs} == {0, 1, 2, 3}
    want = host_counts(L, flat, 0, offs, nck, lab, l_off, pairs)
    got = device_counts(model, flat, 0, offs, nck, lab, l_off, pairs)
    for g, w, what in zip(got, want, ("tp", "tn", "n_pos", "n_valid")):
        assert g.dtype == np.int32 and np.array_equal(g, w), (what, [names[i] for i in np.unique(np.argwhere(g != w)[:, 0])][:8])
    assert got[3][names.index("all_ignored@1")] == 0 and not got[0][names.index("all_ignored@1")].any()
    # the ldp form: rows shorter than the batch is wide (an odd width: the row starts walk through the offsets), NaN and 1.0 behind them
    x, _ = as_batch([r[2] for r in rows])
    x = np.concatenate([x, np.zeros((len(rows), (-x.shape[1]) % 2 + 1), np.float32)], axis=1)      # an odd row pitch
    for i, r in enumerate(rows):
        tail = x[i, len(r[2]):]
        tail[0::2], tail[1::2] = np.nan, 1.0
    assert x.shape[1] % 2 == 1
    got = device_counts(model, x, x.shape[1], None, nck, lab, l_off, pairs)
    for g, w, what in zip(got, want, ("tp", "tn", "n_pos", "n_valid")):
        assert np.array_equal(g, w), (what, [names[i] for i in np.unique(np.argwhere(g != w)[:, 0])][:8])


# ---- the reference's triples -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wav_16k", "wav_8k", "planted", "tiny", "round4", "tie", "random12"])
def test_reference_triples_on_the_device(model, name):
    from silero_vad_amd import threshold_counts, threshold_counts_device
    probs, labels, triple = fixture_sets()[0][name]
    x, lens = as_batch(probs)
    c = threshold_counts_device(model.engine, torch.from_numpy(x).to(model.device), lens, labels)
    assert c.best() == triple
    h = threshold_counts(x, lens, labels)
    same_counts(c, (h.tp, h.tn, h.n_pos, h.n_valid))


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def cuts(tag):
    """a dozen recordings of 0.3 ... 4 s cut from the fixture at odd offsets, odd lengths -> int16 arrays"""
    sr = 16000 if tag == "16k" else 8000
    pcm = np.load(GOLD / f"audio_{tag}.npz")["pcm"]
    rng = np.random.default_rng(41 + sr)
    out = []
    for k in range(12):
        n = int(rng.integers(int(0.3 * sr), 4 * sr + 1)) | 1
        a = int(rng.integers(0, len(pcm) - n)) | 1
        out.append(pcm[a:a + n].copy())
    return out


def form(tag, kind):
    """(recordings as the call takes them, call arguments, chunk count per result row)"""
    from silero_vad_amd import PackedRecordings
    n = 512 if tag == "16k" else 256
    base = cuts(tag)
    kw = {}
    if kind == "i16":
        recs = [torch.from_numpy(x) for x in base]
    elif kind == "arena":
        lens = np.asarray([len(x) for x in base], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(lens + 3)[:-1]]).astype(np.int64)
        arena = torch.zeros(int(offs[-1] + lens[-1]), dtype=torch.int16).pin_memory()
        for o, x in zip(offs, base):
            arena[int(o):int(o) + len(x)] = torch.from_numpy(x)
        recs = PackedRecordings(arena, offs, lens)
    elif kind == "f32":
        recs = [torch.from_numpy(x.astype(np.float32) / 32768.0) for x in base]
    elif kind == "ulaw":
        recs, kw = [torch.from_numpy(encode(x, "ulaw")) for x in base], {"codec": "ulaw"}
    else:
        r, chans, _, twins = stereo_recordings(tag, "s16", count=8, lo=10, hi=125, seed=37, single_frame=False)
        recs, kw, base = [torch.from_numpy(x) for x in r], {"channels": chans}, twins
    return recs, kw, [-(-len(x) // n) for x in base]


@pytest.mark.parametrize("kind", ["i16", "arena", "f32", "ulaw", "stereo"])
@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_ragged_threshold_counts(model, tag, kind):
    from silero_vad_amd import ragged_probs, ragged_threshold_counts, search_thresholds, threshold_counts
    from silero_vad_amd.streams import STATS
    sr = 16000 if tag == "16k" else 8000
    recs, kw, chunks = form(tag, kind)
    rng = np.random.default_rng(5)
    labels = []
    for m in chunks:                                            # runs of speech / silence, a few ignored chunks
        lab = (np.sin(np.arange(m) / rng.uniform(2, 9) + rng.uniform(0, 6)) > 0).astype(np.uint8)
        lab[rng.random(m) < 0.05] = IGNORE
        lab[int(rng.integers(m))] = 1
        labels.append(lab)
    kw = dict(kw, max_bytes=(300_000 if tag == "16k" else 150_000) * (2 if kind == "f32" else 1))
    before = STATS["buckets"]
    got = ragged_threshold_counts(recs, labels, model, sr, **kw)
    assert STATS["buckets"] - before >= 3
    probs = ragged_probs(recs, model, sr, **kw)                 # the same call's probabilities: never across arithmetic
    assert [len(p) for p in probs] == chunks
    x, lens = as_batch([p.numpy() for p in probs])
    want = threshold_counts(x, lens, labels)
    same_counts(got, (want.tp, want.tn, want.n_pos, want.n_valid))            # ... row by row: the caller's order
    assert len({tuple(r) for r in np.concatenate([got.tp, got.tn], axis=1).tolist()}) == len(chunks)    # (no two rows alike: an order mix-up cannot hide)
    assert search_thresholds(recs, labels, model, sr, **kw) == got.best() == want.best()


def test_fixture_speech_gives_the_reference_triple(model):
    """the engine's probabilities of the fixture speech, labels from the reference's own segments: the triple the reference returns on
    ITS probabilities -- which keep 2e-5, the engine-vs-reference bound, away from every inner grid value (checked when the fixture
    was made: min_inner_grid_distance), so every chunk is decided alike at every pair that can come near the best"""
    import json
    from silero_vad_amd import chunk_labels, search_thresholds
    e2e = fixture_sets()[1]
    assert e2e["min_inner_grid_distance"] > 2e-5 and e2e["best_outer_pair_accuracy"] < e2e["triple"][2] - 0.05
    sr = 16000
    pcm = np.load(GOLD / f"audio_{e2e['tag']}.npz")["pcm"][:e2e["n_samples"]]
    seg = json.loads((GOLD / "golden_segments.json").read_text())[e2e["tag"]]["timestamps"]["default"]["out"]
    lab = chunk_labels([{"start": s["start"] / sr, "end": s["end"] / sr} for s in seg], len(pcm), sr)
    assert search_thresholds([torch.from_numpy(pcm)], [lab], model, sr) == tuple(e2e["triple"])
