"""The enter / exit threshold sweep on the host: vad_threshold_counts_host (the twin of the device kernel, csrc/sweeper.hpp) against a
brute-force loop written here that compares like the reference (a Python float with the float64 threshold), `ThresholdCounts.best()`
against the triples the reference's calculate_best_thresholds returned (tests/golden/make_threshold_golden.py), the grid and its
directed float32 roundings, `chunk_labels` against a dense per-sample expression, ignore labels, argument errors.  No GPU."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from conftest import GOLD

TILE = 1024                      # chunks per LDS tile of the device kernel (csrc/kernel_sweep.hip): the shapes below straddle it
IGNORE = 255
PAIR_COUNTS = (1, 63, 64, 65, 190, 257)


# ---- the reference's comparison, in the open --------------------------------------------------------------------------------------
def brute(p, lab, enter64, exit64):
    """tp[P], tn[P], n_pos, n_valid of one row: a plain loop over the chunks, float(p) against the float64 thresholds, the order of
    the two tests as in tuning/utils.py:338-346 (vectorised over the pairs only)"""
    s = np.zeros(len(enter64), dtype=bool)
    tp, tn = np.zeros(len(enter64), dtype=np.int64), np.zeros(len(enter64), dtype=np.int64)
    n_pos = n_valid = 0
    for v, l in zip(p.tolist(), lab.tolist()):
        if l > 1:
            continue
        v = float(v)
        s = np.where(v >= enter64, True, np.where(v <= exit64, False, s))
        n_valid += 1
        if l == 1:
            n_pos += 1
            tp += s
        else:
            tn += ~s
    return tp, tn, n_pos, n_valid


def brute_rows(rows, labels, pairs):
    out = [brute(p, l, pairs.enter, pairs.exit) for p, l in zip(rows, labels)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.asarray([o[2] for o in out]), np.asarray([o[3] for o in out]))


def same_counts(c, want):
    for got, w, name in zip((c.tp, c.tn, c.n_pos, c.n_valid), want, ("tp", "tn", "n_pos", "n_valid")):
        assert got.dtype == np.int32
        assert np.array_equal(got, w), (name, np.argwhere(got != w)[:6])


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_sets():
    """name -> (probabilities per recording, labels per recording, the reference's triple); plus the end-to-end choice"""
    z = np.load(GOLD / "golden_thresholds.npz")
    meta = json.loads((GOLD / "golden_thresholds.json").read_text())
    sets = {}
    for name, info in meta["datasets"].items():
        cuts = np.cumsum(z[f"{name}_lens"])[:-1]
        sets[name] = (np.split(z[f"{name}_probs"], cuts), np.split(z[f"{name}_labels"], cuts), tuple(info["triple"]))
    return sets, meta["e2e"]


def as_batch(rows, fill=np.nan):
    """rows of different lengths -> [B, T] with `fill` behind every row's live part, and their lengths"""
    T = max(1, max(len(r) for r in rows))
    x = np.full((len(rows), T), fill, dtype=np.float32)
    for i, r in enumerate(rows):
        x[i, :len(r)] = r
    return x, [len(r) for r in rows]


@functools.lru_cache(maxsize=None)
def grid_f32():
    g = np.linspace(0, 1, 20)
    f = g.astype(np.float32)
    return np.unique(np.concatenate([f, np.nextafter(f, np.float32(2)), np.nextafter(f, np.float32(-1))]).clip(0, 1))


def random_row(rng, n):
    """probabilities that hit the thresholds: half of them float32 neighbours of grid values, a NaN now and then"""
    p = rng.random(n, dtype=np.float32)
    on = rng.random(n) < 0.5
    p[on] = rng.choice(grid_f32(), size=int(on.sum()))
    p[rng.random(n) < 0.01] = np.nan
    lab = (rng.random(n) < 0.5).astype(np.uint8)
    lab[rng.random(n) < 0.05] = rng.choice(np.asarray([2, 7, IGNORE], dtype=np.uint8))
    return p, lab


@functools.lru_cache(maxsize=None)
def kernel_rows():
    """[(name, start offset in floats modulo 4, probabilities, labels)]: the shape list of the kernel test"""
    rng = np.random.default_rng(404)
    rows = []
    for n in (0, 1, 3, TILE - 1, TILE, TILE + 1, 3 * TILE + 5):
        for m in range(4):                                     # every row start modulo 16 bytes
            rows.append((f"len{n}@{m}", m) + random_row(rng, n))
    for m in (1, 3):
        # one enter, then held in the band between the thresholds across the tile edge: the decision is carried
        n = TILE + 200
        p = np.full(n, 0.30, dtype=np.float32)
        p[5] = 0.99
        rows.append((f"band@{m}", m, p, np.ones(n, dtype=np.uint8)))
    for m in (0, 2):
        # ignore labels on both sides of the first and the second tile edge (the edge is at chunk TILE - m: tiles lie on the address grid)
        p, lab = random_row(rng, 2 * TILE + 100)
        for edge in (TILE - m, 2 * TILE - m):
            lab[edge - 9:edge + 9:2] = IGNORE
            lab[edge - 1:edge + 1] = IGNORE
        rows.append((f"ignore_edge@{m}", m, p, lab))
    p, lab = random_row(rng, TILE + 7)
    p[TILE - 3:TILE + 3] = np.nan                               # NaNs over a tile edge
    rows.append(("nan@0", 0, p, lab))
    rows.append(("all_ignored@1", 1, random_row(rng, 300)[0], np.full(300, IGNORE, dtype=np.uint8)))
    return rows


@functools.lru_cache(maxsize=None)
def kernel_pairs(P):
    """P pairs, among them pairs with exit >= enter and thresholds no float32 holds"""
    from silero_vad_amd import streams, threshold_pairs
    if P == 190:
        return threshold_pairs()
    rng = np.random.default_rng(P)
    g = np.linspace(0, 1, 20)
    e, x = rng.choice(g, size=P), rng.choice(g, size=P)
    e[::7] = rng.random(len(e[::7]))
    assert P < 8 or ((x >= e).any() and (x < e).any())
    return streams._as_pairs(np.stack([e, x], axis=1))


def kernel_layout(rows, fill_a=np.nan, fill_b=1.0):
    """the rows in one flat buffer, each at its start offset modulo 4 floats with a gap in front of it, NaN and 1.0 in every gap ->
    (flat float32, row_offsets, n_chunks, packed labels, label_offsets)"""
    offs, at = [], 8
    for _, m, p, _ in rows:
        at = (at + 3) // 4 * 4 + 4 + m
        offs.append(at)
        at += len(p)
    flat = np.empty(at + 8, dtype=np.float32)
    flat[0::2], flat[1::2] = fill_a, fill_b
    for o, (_, _, p, _) in zip(offs, rows):
        flat[o:o + len(p)] = p
    lab = np.concatenate([r[3] for r in rows])
    l_off = np.concatenate([[0], np.cumsum([len(r[3]) for r in rows])[:-1]]).astype(np.int64)
    return flat, np.asarray(offs, dtype=np.int64), np.asarray([len(r[2]) for r in rows], dtype=np.int64), lab, l_off


@functools.lru_cache(maxsize=None)
def kernel_want(P):
    """the brute-force counts of the kernel rows for the P-pair list: computed once, shared, never written to"""
    rows = kernel_rows()
    want = brute_rows([r[2] for r in rows], [r[3] for r in rows], kernel_pairs(P))
    for w in want:
        w.setflags(write=False)
    return want


def host_counts(L, flat, ldp, offs, nck, lab, l_off, pairs, threads=0):
    B, P = len(nck), len(pairs.enter)
    tp, tn = np.full((B, P), -7, dtype=np.int32), np.full((B, P), -7, dtype=np.int32)
    n_pos, n_valid = np.full(B, -7, dtype=np.int32), np.full(B, -7, dtype=np.int32)
    rc = L.vad_threshold_counts_host(flat.ctypes.data, ldp, None if offs is None else offs.ctypes.data, B, nck.ctypes.data, lab.ctypes.data,
                                     l_off.ctypes.data, pairs.enter_f32.ctypes.data, pairs.exit_f32.ctypes.data, P, tp.ctypes.data,
                                     tn.ctypes.data, n_pos.ctypes.data, n_valid.ctypes.data, threads)
    assert rc == 0, rc
    return tp, tn, n_pos, n_valid


# ---- tests ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(oracle):
    from replay_engine import ReplayEngine
    from silero_vad_amd.engine import HipSileroVAD
    return HipSileroVAD(engine=ReplayEngine(oracle))


def test_threshold_pairs_grid_and_roundings(built):
    from silero_vad_amd import threshold_pairs
    pr = threshold_pairs()
    g = np.linspace(0, 1, 20)
    want = [(e, x) for e in g for x in g if not x >= e]         # the reference's two loops and its `continue`
    assert len(pr.enter) == 190 and list(zip(pr.enter.tolist(), pr.exit.tolist())) == want
    assert pr.enter.dtype == pr.exit.dtype == np.float64 and pr.enter_f32.dtype == pr.exit_f32.dtype == np.float32
    for e, up in zip(pr.enter.tolist(), pr.enter_f32):
        assert float(up) >= e > float(np.nextafter(up, np.float32(-1)))
    for x, dn in zip(pr.exit.tolist(), pr.exit_f32):
        assert float(dn) <= x < float(np.nextafter(dn, np.float32(2)))
    assert (pr.enter_f32 != pr.enter.astype(np.float32)).any() and (pr.exit_f32 != pr.exit.astype(np.float32)).any()   # nearest is not it
    own = threshold_pairs([0.5, 0.7], [0.1, 0.6, 0.9])
    assert list(zip(own.enter.tolist(), own.exit.tolist())) == [(0.5, 0.1), (0.7, 0.1), (0.7, 0.6)]


@pytest.mark.parametrize("name", ["wav_16k", "wav_8k", "planted", "tiny", "round4", "tie", "random12"])
def test_host_twin_and_best_on_the_reference_fixtures(built, name):
    from silero_vad_amd import threshold_counts, threshold_pairs
    sets, _ = fixture_sets()
    assert len(sets) >= 6 and all(1 <= len(s[0]) <= 12 for s in sets.values())
    probs, labels, triple = sets[name]
    pr = threshold_pairs()
    x, lens = as_batch(probs)
    c = threshold_counts(x, lens, labels, pr)
    same_counts(c, brute_rows(probs, labels, pr))
    assert c.best() == triple                                   # the reference's returned (enter, exit, accuracy), exactly
    acc = c.accuracy()
    assert acc.dtype == np.float64 and acc.shape == (len(probs), 190)
    assert np.array_equal(acc, (c.tp.astype(np.float64) + c.tn) / c.n_valid[:, None])
    fp, fn = c.n_valid[:, None] - c.n_pos[:, None] - c.tn, c.n_pos[:, None] - c.tp
    den = 2.0 * c.tp + fp + fn
    assert np.array_equal(c.f1(), np.where(den > 0, 2.0 * c.tp / np.maximum(den, 1), 0.0))


def test_fixture_properties():
    """what the datasets are there for does occur in them"""
    sets, e2e = fixture_sets()
    assert sorted(len(p) for p in sets["tiny"][0])[0] == 1 and max(len(p) for p in sets["tiny"][0]) == 3
    assert [len(p) for p in sets["round4"][0]] == [20000]
    on_grid = np.isin(np.concatenate(sets["planted"][0]), grid_f32())
    assert on_grid.sum() >= 100
    assert e2e["min_inner_grid_distance"] > 2e-5 and e2e["triple"] == list(sets["wav_16k"][2])


def test_round4_and_tie_are_decided_by_the_roundings_and_the_order(built):
    from silero_vad_amd import threshold_counts
    sets, _ = fixture_sets()
    probs, labels, triple = sets["round4"]
    c = threshold_counts(*as_batch(probs), labels)
    correct = (c.tp + c.tn)[0]
    first = int(np.argmax(correct >= 19989))
    assert correct[first] == 19989 and correct.max() == 19992   # 0.99945 first, three more correct chunks at later pairs
    assert (round(c.pairs.enter[first], 2), round(c.pairs.exit[first], 2)) != triple[:2]    # round(0.99945, 4) = 0.9994 -> 0.999 < 1.0
    assert round(round(19989 / 20000, 4), 3) < round(round(19992 / 20000, 4), 3) == triple[2]
    probs, labels, triple = sets["tie"]
    c = threshold_counts(*as_batch(probs), labels)
    top = np.flatnonzero((c.accuracy() == 1.0).all(axis=0))
    assert len(top) > 1 and (round(c.pairs.enter[top[0]], 2), round(c.pairs.exit[top[0]], 2), 1.0) == triple


@pytest.mark.parametrize("P", PAIR_COUNTS)
def test_host_twin_on_the_kernel_shapes(built, P):
    """both addressing forms of the C entry point, single-threaded and on the pool"""
    from silero_vad_amd import _lib
    L, rows, pairs = _lib.lib(), kernel_rows(), kernel_pairs(P)
    want = kernel_want(P)
    flat, offs, nck, lab, l_off = kernel_layout(rows)
    for threads in (1, 4):
        got = host_counts(L, flat, 0, offs, nck, lab, l_off, pairs, threads)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    x, lens = as_batch([r[2] for r in rows])
    got = host_counts(L, x, x.shape[1], None, nck, lab, l_off, pairs)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert want[3][[r[0] for r in rows].index("all_ignored@1")] == 0 and want[3][0] == 0       # no valid chunk: zero counts


def test_band_row_carries_the_decision(built):
    rows = kernel_rows()
    i = [r[0] for r in rows].index("band@1")
    tp = kernel_want(190)[0][i]
    pr = kernel_pairs(190)
    held = (pr.enter > 0.30) & (pr.exit < 0.30) & (pr.enter <= 0.99)
    n = len(rows[i][2])
    assert held.sum() > 20 and (tp[held] == n - 5).all()        # speech from the one loud chunk to the end, over the tile edge


def test_ignored_chunks_are_chunks_that_are_not_there(built):
    from silero_vad_amd import threshold_counts
    rng = np.random.default_rng(9)
    pr = kernel_pairs(65)
    for trial in range(6):
        n = int(rng.integers(5, 400))
        p, lab = random_row(rng, n)
        lab = (lab == 1).astype(np.uint8)
        gone = rng.random(n) < (0.0, 0.1, 0.5, 0.9, 0.3, 1.0)[trial]
        masked = lab.copy()
        masked[gone] = IGNORE
        a = threshold_counts(p[None], [n], [masked], pr)
        m = int((~gone).sum())
        b = threshold_counts(np.concatenate([p[~gone], np.zeros(1, np.float32)])[None], [m], [lab[~gone]], pr)
        same_counts(a, (b.tp, b.tn, b.n_pos, b.n_valid))
        assert a.n_valid[0] == m


def test_chunk_labels():
    from silero_vad_amd import chunk_labels

    def dense(ts, n_samples, sr, N):
        gt = np.zeros(-(-n_samples // N) * N)
        for d in ts:
            gt[int(d["start"] * sr): int(d["end"] * sr)] = 1
        return (np.average(gt.reshape(-1, N), axis=1) > 0.5).astype(np.uint8)

    for sr, N in ((16000, 512), (8000, 256)):
        s = 1.0 / sr
        ts = [{"start": 100 * s, "end": (N + 300) * s},                  # edges inside chunks
              {"start": 3 * N * s, "end": (3 * N + N // 2) * s},         # exactly half a chunk: not speech
              {"start": 5 * N * s, "end": (5 * N + N // 2 + 1) * s},     # one sample more: speech
              {"start": 7.25 * N * s, "end": 9.75 * N * s},
              {"start": 11 * N * s, "end": 40 * N * s}]                  # past the end
        for n_samples in (12 * N, 12 * N + 1, 13 * N - 1, 11 * N + N // 2 + 1):
            got = chunk_labels(ts, n_samples, sr)
            assert got.dtype == np.uint8 and len(got) == -(-n_samples // N)
            assert np.array_equal(got, dense(ts, n_samples, sr, N)), (sr, n_samples)
        got = chunk_labels(ts, 12 * N, sr)
        assert got[3] == 0 and got[5] == 1 and got[0] == 1 and got[11] == 1 and got[10] == 0
    assert len(chunk_labels([], 0)) == 0


def test_argument_errors(built, model):
    from silero_vad_amd import _lib, ragged_threshold_counts, threshold_counts
    from silero_vad_amd.streams import _as_pairs
    L = _lib.lib()
    p = np.full((2, 4), 0.5, dtype=np.float32)
    ok = [np.ones(4, np.uint8), np.zeros(3, np.uint8)]
    assert threshold_counts(p, [4, 3], ok).tp.shape == (2, 190)
    with pytest.raises(ValueError, match="3 chunks and 4 labels"):
        threshold_counts(p, [4, 3], [ok[0], np.zeros(4, np.uint8)])
    with pytest.raises(ValueError):
        threshold_counts(p, [4, 5], [ok[0], np.zeros(5, np.uint8)])            # more chunks than the row holds
    with pytest.raises(ValueError, match="uint8"):
        threshold_counts(p, [4, 3], [ok[0], np.zeros(3, np.int64)])
    none_valid = threshold_counts(p, [4, 3], [ok[0], np.full(3, IGNORE, np.uint8)])
    assert none_valid.n_valid.tolist() == [4, 0]
    with pytest.raises(ValueError, match="without a valid chunk"):
        none_valid.best()
    recs = [torch.zeros(2048), torch.zeros(1000)]
    with pytest.raises(ValueError, match="row 1 has 2 chunks and 3 labels"):
        ragged_threshold_counts(recs, [np.ones(4, np.uint8), np.ones(3, np.uint8)], model)
    with pytest.raises(ValueError, match="row 1 has no valid chunk"):
        ragged_threshold_counts(recs, [np.ones(4, np.uint8), np.full(2, IGNORE, np.uint8)], model)
    with pytest.raises(ValueError, match="2 rows and 1 label arrays"):
        ragged_threshold_counts(recs, [np.ones(4, np.uint8)], model)

    # the C entry points
    pr = _as_pairs(np.asarray([[0.5, 0.35]]))
    flat, nck, lab, off = p.ravel().copy(), np.asarray([4, 3], np.int64), np.ones(7, np.uint8), np.asarray([0, 4], np.int64)
    out = [np.zeros((2, 1), np.int32), np.zeros((2, 1), np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)]

    def host(**bad):
        a = dict(probs=flat.ctypes.data, ldp=4, rows=None, B=2, nck=nck.ctypes.data, lab=lab.ctypes.data, off=off.ctypes.data,
                 en=pr.enter_f32.ctypes.data, ex=pr.exit_f32.ctypes.data, P=1, tp=out[0].ctypes.data, tn=out[1].ctypes.data,
                 n_pos=out[2].ctypes.data, n_valid=out[3].ctypes.data)
        a.update(bad)
        return a

    def call_host(**bad):
        return L.vad_threshold_counts_host(*host(**bad).values(), 1)

    assert call_host() == 0 and out[0].ravel().tolist() == [4, 3]
    for bad in (dict(P=0), dict(P=-1), dict(B=-1), dict(ldp=-1), dict(ldp=3), dict(probs=None), dict(nck=None), dict(lab=None), dict(off=None),
                dict(en=None), dict(ex=None), dict(tp=None), dict(tn=None), dict(n_pos=None), dict(n_valid=None)):
        assert call_host(**bad) == 1, bad                                        # VAD_ERR_ARG
    neg = np.asarray([4, -1], np.int64)
    assert call_host(nck=neg.ctypes.data) == 1

    good = _lib.WEIGHTS_PATH.read_bytes()
    h = ctypes.c_void_p()
    assert L.vad_create_host_only(good, len(good), ctypes.byref(h)) == 0
    try:
        def call_dev(**bad):
            return L.vad_threshold_counts_device(h, *host(**bad).values(), None)
        assert call_dev() == 4 and b"host-only" in L.vad_last_error(h)           # VAD_ERR_NO_DEVICE
        for bad in (dict(P=0), dict(B=-1), dict(probs=None), dict(en=None), dict(n_valid=None)):
            assert call_dev(**bad) == 1, bad
            assert b"vad_threshold_counts_device" in L.vad_last_error(h)
        assert L.vad_threshold_counts_device(None, *host().values(), None) == 1
    finally:
        L.vad_destroy(h)


def test_cpu_standin_takes_the_host_twin(built, model):
    """a model without the device route: the bucket route's probabilities through the host twin, in the caller's order"""
    from silero_vad_amd import ragged_probs, ragged_threshold_counts, search_thresholds, threshold_counts
    pcm = np.load(GOLD / "audio_16k.npz")["pcm"]
    recs = [torch.from_numpy(pcm[a:a + n].copy()) for a, n in ((1001, 9001), (40001, 3000), (90001, 16001), (200001, 5121))]
    rng = np.random.default_rng(3)
    labels = [(rng.random(-(-len(r) // 512)) < 0.5).astype(np.uint8) for r in recs]
    got = ragged_threshold_counts(recs, labels, model, max_bytes=40000)
    probs = ragged_probs(recs, model, max_bytes=40000)
    x, lens = as_batch([q.numpy() for q in probs])
    same_counts(got, [getattr(threshold_counts(x, lens, labels), k) for k in ("tp", "tn", "n_pos", "n_valid")])
    assert search_thresholds(recs, labels, model, max_bytes=40000) == got.best()
