"""Validation loss and ROC-AUC on the host: vad_chunk_scores_host / vad_auc_counts_host (the twins of the device kernels,
csrc/scorer.hpp) against a brute-force numpy count, against the AUCs sklearn gave and the BCE sums BCELoss gave when the fixture was
made (tests/golden/make_validation_golden.py), `ValidationScores.reference()` against the pair the reference's validate() returned,
the key rule at its edges, argument errors, and `ragged_validation` on the CPU stand-in model.  No GPU."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from conftest import GOLD
from test_threshold_sweep import as_batch

IGNORE = 255
KEY_NONE = 0xFFFFFFFF
SETS = ["e2e_16k", "e2e_8k", "ties", "one_ulp", "tiny", "saturated", "random12"]


# ---- fixtures and references ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_sets():
    """name -> (probabilities per recording, labels per recording, recorded BCE sums by label [R] x 2, what the maker recorded)"""
    z = np.load(GOLD / "golden_validation.npz")
    meta = json.loads((GOLD / "golden_validation.json").read_text())["datasets"]
    sets = {}
    for name, info in meta.items():
        cuts = np.cumsum(z[f"{name}_lens"])[:-1]
        sets[name] = (np.split(z[f"{name}_probs"], cuts), np.split(z[f"{name}_labels"], cuts), z[f"{name}_bce_pos"], z[f"{name}_bce_neg"], info)
    return sets


def brute_auc(keys):
    """(U2, n_pos, n_neg) of uint32 keys, KEY_NONE skipped: searchsorted of the sorted negatives, left + right per positive"""
    keys = np.asarray(keys, dtype=np.uint32)
    keys = keys[keys != KEY_NONE]
    v = (keys >> 1).astype(np.int64)
    neg, pos = np.sort(v[(keys & 1) == 0]), v[(keys & 1) == 1]
    u2 = int(np.searchsorted(neg, pos, side="left").sum(dtype=np.int64)) + int(np.searchsorted(neg, pos, side="right").sum(dtype=np.int64))
    return u2, len(pos), len(neg)


def host_auc(keys):
    from silero_vad_amd import _lib
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    out = np.full(3, 7, dtype=np.uint64)
    assert _lib.lib().vad_auc_counts_host(keys.ctypes.data if len(keys) else None, len(keys), out.ctypes.data) == 0
    return tuple(int(x) for x in out)


def keys_of(p, lab):
    """the key rule in numpy, for probabilities in [0, 1] and labels 0 / 1"""
    return ((np.abs(np.asarray(p, dtype=np.float32)).view(np.uint32) << 1) | np.asarray(lab, dtype=np.uint32)).astype(np.uint32)


def numel_of(lens, batch):
    lens = np.asarray(lens)
    return sum(len(lens[a:a + batch]) * int(lens[a:a + batch].max()) for a in range(0, len(lens), batch))


def same_scores(a, b, sums_exact=True):
    for k in ("n_pos", "n_neg", "n_bad", "n_chunks"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert (a.u2, a.total_pos, a.total_neg) == (b.u2, b.total_pos, b.total_neg)
    if sums_exact:
        assert np.array_equal(a.bce_pos, b.bce_pos) and np.array_equal(a.bce_neg, b.bce_neg)


@pytest.fixture(scope="module")
def model(oracle):
    from replay_engine import ReplayEngine
    from silero_vad_amd.engine import HipSileroVAD
    return HipSileroVAD(engine=ReplayEngine(oracle))


# ---- the host twins ---------------------------------------------------------------------------------------------------------------
def test_auc_counts_host_against_brute_force(built):
    rng = np.random.default_rng(11)
    cases = {"empty": np.zeros(0, np.uint32), "one": keys_of([0.5], [1]), "all_none": np.full(40, KEY_NONE, np.uint32),
             "equal": keys_of(np.full(301, 0.25), rng.integers(0, 2, 301)), "one_class": keys_of(rng.random(100), np.ones(100)),
             "uniform": keys_of(rng.random(5000, dtype=np.float32), rng.integers(0, 2, 5000)),
             "ends": keys_of([0.0, 1.0, 0.0, 1.0, -0.0], [1, 0, 0, 1, 0]),
             "any_uint32": rng.integers(0, 1 << 32, 3000, dtype=np.uint64).astype(np.uint32)}
    holes = cases["uniform"].copy()
    holes[rng.random(len(holes)) < 0.3] = KEY_NONE
    cases["holes"] = holes
    for name, keys in cases.items():
        assert host_auc(keys) == brute_auc(keys), name
    assert host_auc(cases["equal"])[0] == host_auc(cases["equal"])[1] * host_auc(cases["equal"])[2]      # all ties: AUC one half
    assert host_auc(cases["ends"]) == (2 * 2 + 1 + 2, 2, 3)       # 1.0 above three negatives; 0.0 ties two (0.0, -0.0), below 1.0
    from silero_vad_amd import _lib
    L, out = _lib.lib(), np.zeros(3, np.uint64)
    assert L.vad_auc_counts_host(None, 1, out.ctypes.data) == 1 and L.vad_auc_counts_host(holes.ctypes.data, -1, out.ctypes.data) == 1
    assert L.vad_auc_counts_host(holes.ctypes.data, 4, None) == 1 and L.vad_auc_counts_host(holes.ctypes.data, 1 << 31, out.ctypes.data) == 1
    assert L.vad_auc_workspace_bytes(-1) == 0 and L.vad_auc_workspace_bytes(1 << 31) == 0
    assert L.vad_auc_workspace_bytes(1000) - L.vad_auc_workspace_bytes(0) == 4000


@pytest.mark.parametrize("name", SETS)
def test_host_twins_on_the_recorded_sets(built, name):
    from silero_vad_amd import chunk_scores
    probs, labels, rp, rn, info = fixture_sets()[name]
    s = chunk_scores(*as_batch(probs), labels)
    y, x = np.concatenate(labels), np.concatenate(probs)
    assert np.array_equal(s.keys[y <= 1], keys_of(x[y <= 1], y[y <= 1])) and (s.keys[y > 1] == KEY_NONE).all()
    assert (s.u2, s.total_pos, s.total_neg) == brute_auc(s.keys) == host_auc(s.keys)
    assert (s.total_pos, s.total_neg) == (info["n_pos"], info["n_neg"]) and not s.n_bad.any()
    assert np.array_equal(s.n_pos, [int((l == 1).sum()) for l in labels]) and np.array_equal(s.n_neg, [int((l == 0).sum()) for l in labels])
    assert abs(s.roc_auc() - info["auc"]) <= 2.0 ** -50 * info["auc"]                  # sklearn's roc_auc_score, unrounded
    tol = min(8 * info["twin_sum_distance"], 1e-6)                                     # (1e-6 is a cap, not the tolerance)
    print(name, "sum distance", np.abs(s.bce_pos - rp).max(), np.abs(s.bce_neg - rn).max(), "tol", tol)
    assert s.bce_pos.dtype == np.float64 and (np.abs(s.bce_pos - rp) <= tol * rp).all() and (np.abs(s.bce_neg - rn) <= tol * rn).all()


# ---- ValidationScores ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_reference_pair_on_the_reference_predictions(built, name):
    from silero_vad_amd import chunk_scores
    probs, labels, rp, rn, info = fixture_sets()[name]
    s = chunk_scores(*as_batch(probs), labels)
    lens = [len(p) for p in probs]
    assert info["batch_size"] == 3 and info["noise_loss"] == 0.5 and numel_of(lens, 3) > sum(lens)       # padding enters numel
    loss, auc = s.reference(0.5, 3)
    tol = min(8 * info["twin_loss_distance"], 1e-6 * info["pair"][0])
    print(name, "loss", loss, "recorded", info["pair"][0], "tol", tol)
    assert auc == info["pair"][1] and abs(loss - info["pair"][0]) <= tol
    total = float(s.bce_pos.sum() + 0.5 * s.bce_neg.sum())
    assert loss == pytest.approx(total / numel_of(lens, 3), rel=1e-14)
    # another batch size pads differently; None divides by the chunks there are
    assert s.loss(0.5, 2) == pytest.approx(total / numel_of(lens, 2), rel=1e-14) and numel_of(lens, 2) != numel_of(lens, 3)
    assert s.loss(0.5, 2) != loss
    assert s.loss(0.5, None) == s.loss(0.5, 1) == pytest.approx(total / sum(lens), rel=1e-14)
    assert s.loss(1.0) == pytest.approx(float(s.bce_pos.sum() + s.bce_neg.sum()) / sum(lens), rel=1e-14)
    assert s.loss(0.5, len(lens) + 5) == pytest.approx(total / (len(lens) * max(lens)), rel=1e-14)


def test_fixture_properties():
    sets = fixture_sets()
    assert sorted(sets) == sorted(SETS)
    for tag in ("e2e_16k", "e2e_8k"):
        info = sets[tag][4]
        assert info["recordings"] == 7 and len(set(info["samples"])) == 7 and any(m % (512 if tag == "e2e_16k" else 256) for m in info["samples"])
        assert info["ignored"] <= 0.01 * sum(len(p) for p in sets[tag][0])
        edge = abs(info["auc"] * 1000 - np.floor(info["auc"] * 1000) - 0.5) / 1000
        assert info["auc_bound"] == info["close_pairs"] / (info["n_pos"] * info["n_neg"]) < edge
        assert 0 < info["loss_bound"] < 1e-3 * info["pair"][0]
    ties = np.concatenate(sets["ties"][0])
    assert len(np.unique(ties)) == 9 and (ties == 0).any() and (ties == 1).any()
    v = np.concatenate(sets["one_ulp"][0]).view(np.uint32)
    assert (v % (1 << 14) == 0).sum() >= 8 and (v % (1 << 14) == (1 << 14) - 1).sum() >= 4 and (v == 0x3F000000).any() and (v == 0x3EFFFFFF).any()
    assert {len(p) for p in sets["tiny"][0]} == {1, 2, 3}
    sat = np.concatenate(sets["saturated"][0])
    assert (sat > 1 - 1e-6).any() and (sat < 1e-30).any()


# ---- the key rule -------------------------------------------------------------------------------------------------------------------
def test_key_rule_at_its_edges(built):
    from silero_vad_amd import chunk_scores
    f = np.float32
    good = np.asarray([-0.0, 0.0, 1.0, 1e-42, 0.5], dtype=f)
    bad = np.asarray([np.nan, np.inf, -1e-3, np.nextafter(f(1), f(2)), -np.inf], dtype=f)
    for lab in (0, 1):
        s = chunk_scores(good[None], [5], [np.full(5, lab, np.uint8)])
        assert s.n_bad[0] == 0 and (s.n_pos[0], s.n_neg[0]) == ((5, 0) if lab else (0, 5))
        assert s.keys.tolist() == [lab, lab, (0x3F800000 << 1) | lab, (int(good[3:4].view(np.uint32)[0]) << 1) | lab, (0x3F000000 << 1) | lab]
        want = [100.0, 100.0, 0.0, -np.log(float(f(1e-42))), np.log(2.0)] if lab else [0.0, 0.0, 100.0, 0.0, np.log(2.0)]
        got = float(s.bce_pos[0] if lab else s.bce_neg[0])
        assert got == pytest.approx(sum(want), rel=1e-12)                              # the log is clamped at -100; -0.0 is +0.0
        s = chunk_scores(bad[None], [5], [np.full(5, lab, np.uint8)])
        assert s.n_bad[0] == 5 and s.n_pos[0] == s.n_neg[0] == 0 and (s.keys == KEY_NONE).all() and s.bce_pos[0] == s.bce_neg[0] == 0.0
    # one bad chunk among good ones: counted, and every figure refuses
    p = np.asarray([[0.2, np.nan, 0.9, 0.4]], dtype=f)
    s = chunk_scores(p, [4], [np.asarray([0, 1, 1, 0], np.uint8)])
    assert s.n_bad.tolist() == [1] and (s.total_pos, s.total_neg) == (1, 2) and s.keys[1] == KEY_NONE
    for call in (s.roc_auc, s.loss, s.reference):
        with pytest.raises(ValueError, match="between 0 and 1"):
            call()
    # label 255 (and any label above 1) is silently skipped, whatever its probability
    s = chunk_scores(p, [4], [np.asarray([0, IGNORE, 1, 2], np.uint8)])
    assert s.n_bad.tolist() == [0] and (s.total_pos, s.total_neg, s.u2) == (1, 1, 2) and s.roc_auc() == 1.0
    assert s.keys.tolist() == [int(keys_of([0.2], [0])[0]), KEY_NONE, int(keys_of([0.9], [1])[0]), KEY_NONE]
    assert s.loss() == pytest.approx((-np.log(float(f(0.9))) - 0.5 * np.log(float(f(1) - f(0.2)))) / 4, rel=1e-14)


def test_rows_keep_their_bits_anywhere(built):
    """a row's sums and keys do not depend on where the row lies: another batch position, pitch and neighbours"""
    from silero_vad_amd import chunk_scores
    rng = np.random.default_rng(8)
    p, lab = rng.random(1500, dtype=np.float32), rng.integers(0, 2, 1500).astype(np.uint8)
    a = chunk_scores(p[None], [1500], [lab])
    x = rng.random((19, 1601), dtype=np.float32)
    x[17, :1500] = p
    x[17, 1500:] = np.nan
    b = chunk_scores(x, [1601] * 17 + [1500, 7], [np.ones(1601, np.uint8)] * 17 + [lab, np.zeros(7, np.uint8)], threads=3)
    assert a.bce_pos[0] == b.bce_pos[17] and a.bce_neg[0] == b.bce_neg[17] and b.n_bad[17] == 0
    assert np.array_equal(a.keys, b.keys[17 * 1601:17 * 1601 + 1500])


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(built, model):
    from silero_vad_amd import _lib, chunk_scores, ragged_validation
    L = _lib.lib()
    p = np.full((2, 4), 0.5, dtype=np.float32)
    one = chunk_scores(p, [4, 3], [np.ones(4, np.uint8), np.ones(3, np.uint8)])
    with pytest.raises(ValueError, match="Only one class present"):
        one.roc_auc()
    assert one.loss() == pytest.approx(np.log(2.0))
    with pytest.raises(ValueError, match="3 chunks and 4 labels"):
        chunk_scores(p, [4, 3], [np.ones(4, np.uint8), np.zeros(4, np.uint8)])
    with pytest.raises(ValueError):
        chunk_scores(p, [4, 5], [np.ones(4, np.uint8), np.zeros(5, np.uint8)])
    with pytest.raises(ValueError, match="uint8"):
        chunk_scores(p, [4, 3], [np.ones(4, np.uint8), np.zeros(3, np.int64)])
    none = chunk_scores(p, [4, 3], [np.full(4, IGNORE, np.uint8), np.full(3, IGNORE, np.uint8)])
    assert (none.total_pos, none.total_neg, none.u2) == (0, 0, 0) and none.loss() == 0.0
    with pytest.raises(ValueError, match="Only one class present"):
        none.roc_auc()
    empty = chunk_scores(np.zeros((0, 0), np.float32), [], [])
    with pytest.raises(ValueError, match="no chunk"):
        empty.loss()
    recs = [torch.zeros(2048), torch.zeros(1000)]
    with pytest.raises(ValueError, match="row 1 has 2 chunks and 3 labels"):
        ragged_validation(recs, [np.ones(4, np.uint8), np.ones(3, np.uint8)], model)
    with pytest.raises(ValueError, match="2 rows and 1 label arrays"):
        ragged_validation(recs, [np.ones(4, np.uint8)], model)

    # the C entry points
    flat, nck, lab, off = p.ravel().copy(), np.asarray([4, 3], np.int64), np.ones(7, np.uint8), np.asarray([0, 4], np.int64)
    keys = np.zeros(7, np.uint32)
    d, i = [np.zeros(2, np.float64) for _ in range(2)], [np.zeros(2, np.int32) for _ in range(3)]

    def host(**bad):
        a = dict(probs=flat.ctypes.data, ldp=4, rows=None, B=2, nck=nck.ctypes.data, lab=lab.ctypes.data, off=off.ctypes.data, koff=off.ctypes.data,
                 keys=keys.ctypes.data, bp=d[0].ctypes.data, bn=d[1].ctypes.data, n_pos=i[0].ctypes.data, n_neg=i[1].ctypes.data, n_bad=i[2].ctypes.data)
        a.update(bad)
        return a

    assert L.vad_chunk_scores_host(*host().values(), 1) == 0 and i[0].tolist() == [4, 3]
    neg = np.asarray([4, -1], np.int64)
    for bad in (dict(B=-1), dict(ldp=-1), dict(ldp=3), dict(probs=None), dict(nck=None), dict(lab=None), dict(off=None), dict(koff=None), dict(keys=None),
                dict(bp=None), dict(bn=None), dict(n_pos=None), dict(n_neg=None), dict(n_bad=None), dict(nck=neg.ctypes.data), dict(koff=neg.ctypes.data)):
        assert L.vad_chunk_scores_host(*host(**bad).values(), 1) == 1, bad              # VAD_ERR_ARG

    good = _lib.WEIGHTS_PATH.read_bytes()
    h = ctypes.c_void_p()
    assert L.vad_create_host_only(good, len(good), ctypes.byref(h)) == 0
    try:
        assert L.vad_chunk_scores_device(h, *host().values(), None) == 4 and b"host-only" in L.vad_last_error(h)      # VAD_ERR_NO_DEVICE
        for bad in (dict(B=-1), dict(probs=None), dict(koff=None), dict(n_bad=None), dict(probs=flat.ctypes.data + 2)):
            assert L.vad_chunk_scores_device(h, *host(**bad).values(), None) == 1, bad
            assert b"vad_chunk_scores_device" in L.vad_last_error(h)
        assert L.vad_chunk_scores_device(None, *host().values(), None) == 1
        out, ws = np.zeros(3, np.uint64), np.zeros(16, np.uint64)
        need = L.vad_auc_workspace_bytes(7)
        assert L.vad_auc_counts_device(h, keys.ctypes.data, 7, ws.ctypes.data, need, out.ctypes.data, None) == 4
        assert L.vad_auc_counts_device(h, keys.ctypes.data, 7, ws.ctypes.data, need - 1, out.ctypes.data, None) == 1
        assert b"workspace" in L.vad_last_error(h)
        assert L.vad_auc_counts_device(h, keys.ctypes.data, -1, ws.ctypes.data, need, out.ctypes.data, None) == 1
        assert L.vad_auc_counts_device(h, keys.ctypes.data, 7, None, need, out.ctypes.data, None) == 1
        assert L.vad_auc_counts_device(None, keys.ctypes.data, 7, ws.ctypes.data, need, out.ctypes.data, None) == 1
    finally:
        L.vad_destroy(h)


# ---- the corpus route on the CPU stand-in --------------------------------------------------------------------------------------------
def test_cpu_standin_takes_the_host_twins(built, model):
    """a model without the device route: the bucket route's probabilities through the host twins, in the caller's order"""
    from silero_vad_amd import chunk_scores, ragged_probs, ragged_validation, validate
    pcm = np.load(GOLD / "audio_16k.npz")["pcm"]
    recs = [torch.from_numpy(pcm[a:a + n].copy()) for a, n in ((1001, 9001), (40001, 3000), (90001, 16001), (200001, 5121))]
    rng = np.random.default_rng(3)
    labels = [(rng.random(-(-len(r) // 512)) < 0.5).astype(np.uint8) for r in recs]
    labels[2][3] = IGNORE
    got = ragged_validation(recs, labels, model, max_bytes=40000, keep_keys=True)
    probs = ragged_probs(recs, model, max_bytes=40000)
    want = chunk_scores(*as_batch([q.numpy() for q in probs]), labels)
    same_scores(got, want)
    assert np.array_equal(got.keys, want.keys) and len(np.unique(got.bce_pos)) == len(recs)
    assert ragged_validation(recs, labels, model, max_bytes=40000).keys is None
    assert validate(recs, labels, model, noise_loss=0.25, batch_size=3, max_bytes=40000) == want.reference(0.25, 3)
