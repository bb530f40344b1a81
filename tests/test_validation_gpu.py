"""Validation loss and ROC-AUC on the device: the score kernel (vad_chunk_scores_device, csrc/kernel_score.hip) against the host twin on
the row list of tests/test_threshold_sweep.py plus the key rule's special values; the AUC kernels (vad_auc_counts_device) against the
host twin and a brute-force count, as integers; the recorded sets through `chunk_scores_device`; `ragged_validation` on every ingest
form against `chunk_scores` on `ragged_probs` of the same call; and `validate()` with the real engine against the pair the
reference's validate() returned (tests/golden/make_validation_golden.py).
Everything here needs a real MI355X:  python -m pytest tests -m gpu
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import GOLD
from test_corpus_g711 import encode
from test_corpus_stereo import stereo_recordings
from test_threshold_sweep import TILE, as_batch, kernel_layout, kernel_rows
from test_validation import IGNORE, KEY_NONE, SETS, brute_auc, fixture_sets, host_auc, keys_of, same_scores

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
FILL64 = 0x5A5A5A5A5A5A5A5A
GUARD = 64


@pytest.fixture(scope="module")
def model(built):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback to silently pass on)")
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    assert m.engine._h, "native engine not created"
    return m


def stream_of(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def sum_bound(n, want):
    """two logs of at most 2 ulp each and two summations of n non-negative terms: (2 n + 8) 2^-53 of the sum"""
    return (2 * np.asarray(n, dtype=np.float64) + 8) * 2.0 ** -53 * want


# ---- the score kernel ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def score_rows():
    """the sweep tests' rows (lengths 0 ... 3 TILE + 5 at all four alignments, NaN, an all-ignored row) and the key rule's specials"""
    f = np.float32
    special = np.asarray([-0.0, 0.0, 1.0, 1e-42, np.nan, np.inf, -1e-3, np.nextafter(f(1), f(2)), 0.5, -np.inf, 1.0 - 2.0 ** -24, 2.0 ** -120], dtype=f)
    rows = list(kernel_rows())
    for m, lab in ((0, 0), (1, 1), (2, IGNORE), (3, None)):
        l = np.full(len(special), lab, np.uint8) if lab is not None else (np.arange(len(special)) % 2).astype(np.uint8)
        rows.append((f"special{lab}@{m}", m, special, l))
    return rows


def host_scores(flat, ldp, offs, nck, lab, l_off, k_off, total):
    from silero_vad_amd import _lib
    B = len(nck)
    keys = np.full(total, FILL, dtype=np.uint32)
    bp, bn = np.zeros(B, np.float64), np.zeros(B, np.float64)
    ints = [np.zeros(B, np.int32) for _ in range(3)]
    rc = _lib.lib().vad_chunk_scores_host(flat.ctypes.data, ldp, None if offs is None else offs.ctypes.data, B, nck.ctypes.data, lab.ctypes.data,
                                          l_off.ctypes.data, k_off.ctypes.data, keys.ctypes.data, bp.ctypes.data, bn.ctypes.data,
                                          *(a.ctypes.data for a in ints), 0)
    assert rc == 0, rc
    return keys, bp, bn, ints


def device_scores(model, flat, ldp, offs, nck, lab, l_off, k_off, total):
    """one launch -> (keys, bce_pos, bce_neg, [n_pos, n_neg, n_bad]) as numpy; every output sits between guard words that must come
    back untouched; key cells no row owns keep the fill"""
    from silero_vad_amd import _lib
    L, dev = _lib.lib(), model.device
    B = len(nck)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (flat, nck, lab, l_off, k_off)]
    d_off = torch.from_numpy(offs).to(dev) if offs is not None else None
    keys = torch.full((total + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)
    sums = [torch.full((B + 2 * GUARD,), FILL64, dtype=torch.int64, device=dev) for _ in range(2)]
    ints = [torch.full((B + 2 * GUARD,), FILL, dtype=torch.int32, device=dev) for _ in range(3)]
    _lib.check(model.engine._h, L.vad_chunk_scores_device(
        model.engine._h, d[0].data_ptr(), ldp, d_off.data_ptr() if d_off is not None else None, B, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
        d[4].data_ptr(), keys.data_ptr() + 4 * GUARD, *(s.data_ptr() + 8 * GUARD for s in sums), *(o.data_ptr() + 4 * GUARD for o in ints), stream_of(dev)))
    torch.cuda.synchronize()
    k = keys.cpu().numpy().view(np.uint32)
    assert (k[:GUARD] == FILL).all() and (k[GUARD + total:] == FILL).all()
    out = []
    for o, fill in zip(sums + ints, (FILL64, FILL64, FILL, FILL, FILL)):
        a = o.cpu().numpy()
        assert (a[:GUARD] == fill).all() and (a[GUARD + B:] == fill).all() and (a[GUARD:GUARD + B] != fill).all()
        out.append(a[GUARD:GUARD + B])
    return k[GUARD:GUARD + total], out[0].view(np.float64), out[1].view(np.float64), out[2:]


def test_score_kernel_against_the_host_twin(model):
    rows = score_rows()
    names = [r[0] for r in rows]
    assert {len(r[2]) for r in rows} >= {0, 1, 3, TILE - 1, TILE, TILE + 1, 3 * TILE + 5}
    flat, offs, nck, lab, l_off = kernel_layout(rows)
    assert {int(o) % 4 for o in offs} == {0, 1, 2, 3}
    k_off = l_off + 3 * np.arange(len(rows), dtype=np.int64)        # three cells between two rows' keys that nobody owns
    total = int(k_off[-1] + nck[-1]) + 3
    owned = np.zeros(total, dtype=bool)
    for o, n in zip(k_off, nck):
        owned[o:o + n] = True
    want = host_scores(flat, 0, offs, nck, lab, l_off, k_off, total)
    got = device_scores(model, flat, 0, offs, nck, lab, l_off, k_off, total)
    assert (got[0][~owned] == FILL).all() and (want[0][~owned] == FILL).all() and (got[0][owned] != FILL).all()
    assert np.array_equal(got[0], want[0])
    for g, w, what in zip(got[3], want[3], ("n_pos", "n_neg", "n_bad")):
        assert g.dtype == np.int32 and np.array_equal(g, w), (what, [names[i] for i in np.flatnonzero(g != w)][:8])
    assert want[3][2].sum() > 20 and want[3][0].sum() > 1000 and want[3][1].sum() > 1000
    for g, w, what in zip(got[1:3], want[1:3], ("bce_pos", "bce_neg")):
        err = np.abs(g - w)
        print(what, "largest error / bound", float((err / np.maximum(sum_bound(nck, w), 1e-300)).max()))
        assert (err <= sum_bound(nck, w)).all(), (what, [names[i] for i in np.flatnonzero(err > sum_bound(nck, w))][:8])
    i = names.index("special1@1")
    assert got[3][0][i] == 7 and got[3][2][i] == 5 and got[3][1][i] == 0
    i = names.index(f"special{IGNORE}@2")
    assert [int(o[i]) for o in got[3]] == [0, 0, 0] and got[1][i] == 0.0 and got[2][i] == 0.0
    # the same rows at another offset, pitch and batch position (reversed, an odd row pitch, NaN and 1.0 behind them): the same BITS
    back = rows[::-1]
    x, _ = as_batch([r[2] for r in back])
    x = np.concatenate([x, np.zeros((len(back), (-x.shape[1]) % 2 + 1), np.float32)], axis=1)
    for j, r in enumerate(back):
        tail = x[j, len(r[2]):]
        tail[0::2], tail[1::2] = np.nan, 1.0
    assert x.shape[1] % 2 == 1
    nck_b = np.ascontiguousarray(nck[::-1])
    lab_b = np.concatenate([r[3] for r in back])
    l_off_b = np.concatenate([[0], np.cumsum(nck_b)[:-1]]).astype(np.int64)
    again = device_scores(model, x, x.shape[1], None, nck_b, lab_b, l_off_b, l_off_b, int(nck_b.sum()))
    assert np.array_equal(again[1][::-1].view(np.uint64), got[1].view(np.uint64)) and np.array_equal(again[2][::-1].view(np.uint64), got[2].view(np.uint64))
    for g, a in zip(got[3], again[3]):
        assert np.array_equal(g, a[::-1])
    for j, (o, n) in enumerate(zip(l_off_b, nck_b)):
        i = len(rows) - 1 - j
        assert np.array_equal(again[0][o:o + n], got[0][k_off[i]:k_off[i] + n])


# ---- the AUC kernels ----------------------------------------------------------------------------------------------------------------
def device_auc(model, keys, short=0):
    """vad_auc_counts_device -> (rc, the three integers); workspace and out between guard words that must come back untouched"""
    from silero_vad_amd import _lib
    L, dev = _lib.lib(), model.device
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    n = len(keys)
    need = int(L.vad_auc_workspace_bytes(n))
    assert need % 4 == 0
    k_dev = torch.from_numpy(keys.view(np.int32)).to(dev) if n else torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.full((need // 4 + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)
    out = torch.full((3 + 2 * GUARD,), FILL64, dtype=torch.int64, device=dev)
    rc = L.vad_auc_counts_device(model.engine._h, k_dev.data_ptr(), n, ws.data_ptr() + 4 * GUARD, need - short, out.data_ptr() + 8 * GUARD, stream_of(dev))
    torch.cuda.synchronize()
    w, o = ws.cpu().numpy(), out.cpu().numpy()
    assert (w[:GUARD] == FILL).all() and (w[GUARD + need // 4:] == FILL).all()
    assert (o[:GUARD] == FILL64).all() and (o[GUARD + 3:] == FILL64).all()
    if rc != 0:
        assert (w == FILL).all() and (o == FILL64).all()                            # refused: nothing written
    return rc, tuple(int(v) for v in o[GUARD:GUARD + 3].view(np.uint64))


def check_auc(model, keys, what):
    want = brute_auc(keys)
    assert host_auc(keys) == want, what
    rc, got = device_auc(model, keys)
    assert rc == 0 and got == want, (what, got, want)
    return got


BLOCK = 256           # keys per workgroup and pass of the histogram / scatter kernels; also the largest bin compared all against all
SIZES = (0, 1, 2, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 5)


@pytest.mark.parametrize("n", SIZES)
def test_auc_kernels_at_every_size(model, n):
    rng = np.random.default_rng(100 + n)
    lab = rng.integers(0, 2, n)
    uniform = keys_of(rng.random(n, dtype=np.float32), lab)
    check_auc(model, uniform, "uniform")
    got = check_auc(model, keys_of(np.full(n, 0.75, np.float32), lab), "equal")            # one bin: all against all up to BLOCK keys, LDS histograms above
    assert got[0] == got[1] * got[2]
    near = (np.uint32(0x3F000000 << 1) + (rng.integers(0, 40, n).astype(np.uint32) << 1)) | lab.astype(np.uint32)
    check_auc(model, near, "one bin, 40 values")
    holes = uniform.copy()
    holes[rng.random(n) < 0.4] = KEY_NONE
    check_auc(model, holes, "holes")
    assert check_auc(model, np.full(n, KEY_NONE, np.uint32), "all none") == (0, 0, 0)
    one = check_auc(model, uniform | np.uint32(1), "one class")
    assert one == (0, n, 0)


def test_auc_kernels_contents(model):
    rng = np.random.default_rng(77)
    n = 3 * BLOCK + 5
    lab = rng.integers(0, 2, n).astype(np.uint32)
    for step in (1 << 14, 1 << 12):                              # v = k step - 1 against k step: neighbours in different bins
        k = rng.integers(1, 0x3F800000 // step, n).astype(np.uint32)
        v = k * np.uint32(step) - (rng.integers(0, 2, n).astype(np.uint32))
        check_auc(model, (v << 1) | lab, f"bin edges {step}")
        k[:] = k[0]                                              # ... one edge, many keys on both sides of it
        v = k * np.uint32(step) - (rng.integers(0, 2, n).astype(np.uint32))
        check_auc(model, (v << 1) | lab, f"one bin edge {step}")
    ends = np.where(rng.integers(0, 2, n) == 1, np.uint32(0x3F800000), np.uint32(0))
    check_auc(model, (ends << 1) | lab, "v = 0 and v = 0x3F800000")
    check_auc(model, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), "any uint32 is a key")
    for name in ("ties", "saturated", "one_ulp"):
        probs, labels = fixture_sets()[name][:2]
        got = check_auc(model, keys_of(np.concatenate(probs), np.concatenate(labels)), name)
        info = fixture_sets()[name][4]
        assert got[1:] == (info["n_pos"], info["n_neg"]) and abs(got[0] / (2 * got[1] * got[2]) - info["auc"]) <= 2.0 ** -50


def test_auc_kernels_many_workgroups_and_bins(model):
    rng = np.random.default_rng(78)
    n = 200_003
    lab = rng.integers(0, 2, n)
    u = rng.random(n, dtype=np.float32)
    check_auc(model, keys_of(u, lab), "uniform: next to no two keys in one bin")
    # probabilities on a grid of 400 / 1000 values with a few thousand ulps of jitter: bins of ~500 keys (LDS histograms) and of ~200
    # (all against all), equal keys among them
    grid = np.where(np.arange(n) % 2 == 0, np.round(u * 400) / 400, np.round(u * 1000) / 1000).astype(np.float32).clip(0.001, 0.999)
    v = grid.view(np.uint32) + rng.integers(0, 3000, n).astype(np.uint32)
    keys = (v << 1) | lab.astype(np.uint32)
    keys[rng.random(n) < 0.02] = KEY_NONE
    check_auc(model, keys, "gridded")
    # more keys than one pass of the grid holds (2 048 workgroups x 256): the second trip of the grid-stride loops
    m = 2048 * BLOCK + 77
    big = keys_of(rng.random(m, dtype=np.float32) ** 8, rng.integers(0, 2, m))
    check_auc(model, big, "two passes")


def test_auc_workspace_too_small_is_refused(model):
    keys = keys_of(np.linspace(0, 1, 500, dtype=np.float32), np.arange(500) % 2)
    rc, _ = device_auc(model, keys, short=1)
    from silero_vad_amd import _lib
    assert rc == 1 and b"workspace" in _lib.lib().vad_last_error(model.engine._h)
    assert device_auc(model, keys)[1] == brute_auc(keys)


# ---- the recorded sets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_recorded_sets_on_the_device(model, name):
    from silero_vad_amd import chunk_scores, chunk_scores_device
    probs, labels, _, _, info = fixture_sets()[name]
    x, lens = as_batch(probs)
    d = chunk_scores_device(model.engine, torch.from_numpy(x).to(model.device), lens, labels, keep_keys=True)
    h = chunk_scores(x, lens, labels)
    same_scores(d, h, sums_exact=False)
    assert np.array_equal(d.keys, h.keys)
    assert (np.abs(d.bce_pos - h.bce_pos) <= sum_bound(lens, h.bce_pos)).all() and (np.abs(d.bce_neg - h.bce_neg) <= sum_bound(lens, h.bce_neg)).all()
    loss, auc = d.reference(info["noise_loss"], info["batch_size"])
    assert auc == info["pair"][1] and abs(loss - info["pair"][0]) <= min(8 * info["twin_loss_distance"], 1e-6 * info["pair"][0])


# ---- the corpus route -----------------------------------------------------------------------------------------------------------------
def cuts(sr, seed, count=9):
    """recordings of 0.3 ... 4 s cut from the fixture at odd offsets, odd lengths -> int16 arrays"""
    pcm = np.load(GOLD / f"audio_{'16k' if sr == 16000 else '8k'}.npz")["pcm"]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(int(0.3 * sr), 4 * sr + 1)) | 1
        a = int(rng.integers(0, len(pcm) - n)) | 1
        out.append(pcm[a:a + n].copy())
    return out


@pytest.mark.parametrize("kind", ["i16", "ulaw", "stereo", "44100"])
def test_ragged_validation(model, kind):
    from silero_vad_amd import chunk_scores, ragged_probs, ragged_validation
    from silero_vad_amd.streams import STATS
    sr = 16000
    if kind == "stereo":
        r, chans, _, _ = stereo_recordings("16k", "s16", count=8, lo=10, hi=125, seed=37, single_frame=False)
        recs, kw = [torch.from_numpy(x) for x in r], {"channels": chans}
    elif kind == "ulaw":
        recs, kw = [torch.from_numpy(encode(x, "ulaw")) for x in cuts(sr, 51)], {"codec": "ulaw"}
    elif kind == "44100":
        # (the fixture's samples played as 44.1 kHz material: what matters is that it is resampled on the way in)
        recs, kw = [torch.from_numpy(x) for x in cuts(sr, 52)], {"source_rate": 44100}
    else:
        recs, kw = [torch.from_numpy(x) for x in cuts(sr, 53)], {}
    kw = dict(kw, max_bytes=200_000)
    probs = ragged_probs(recs, model, sr, **kw)                 # the same call's probabilities: never across arithmetic
    chunks = [len(p) for p in probs]
    rng = np.random.default_rng(5)
    labels = []
    for m in chunks:                                            # runs of speech / silence, a few ignored chunks
        lab = (np.sin(np.arange(m) / rng.uniform(2, 9) + rng.uniform(0, 6)) > 0).astype(np.uint8)
        lab[rng.random(m) < 0.05] = IGNORE
        lab[int(rng.integers(m))] = 1
        labels.append(lab)
    before = STATS["buckets"]
    got = ragged_validation(recs, labels, model, sr, keep_keys=True, **kw)
    assert STATS["buckets"] - before >= 3
    want = chunk_scores(*as_batch([p.numpy() for p in probs]), labels)
    same_scores(got, want, sums_exact=False)
    assert np.array_equal(got.keys, want.keys)                  # every bucket's keys at its recordings' corpus offsets
    assert (np.abs(got.bce_pos - want.bce_pos) <= sum_bound(chunks, want.bce_pos)).all()
    assert (np.abs(got.bce_neg - want.bce_neg) <= sum_bound(chunks, want.bce_neg)).all()
    assert len(np.unique(got.bce_pos)) == len(chunks) and got.total_pos > 0 and got.total_neg > 0
    assert got.roc_auc() == want.roc_auc()


@pytest.mark.parametrize("tag", ["e2e_16k", "e2e_8k"])
def test_validate_gives_the_reference_pair(model, tag):
    """the real engine on the recordings the reference's validate() ran on: the pair it returned, within what an engine 2e-5 away from
    the reference's probabilities can move -- every bound is the fixture's"""
    from silero_vad_amd import ragged_validation, validate
    _, labels, _, _, info = fixture_sets()[tag]
    sr = info["sampling_rate"]
    pcm = np.load(GOLD / f"audio_{info['tag']}.npz")["pcm"]
    recs = [torch.from_numpy(pcm[a:a + m].copy()) for a, m in zip(info["starts"], info["samples"])]
    s = ragged_validation(recs, labels, model, sr)
    loss, auc = s.reference(info["noise_loss"], info["batch_size"])
    print(tag, "auc", s.roc_auc(), "recorded", info["auc"], "bound", info["auc_bound"], "loss", loss, "recorded", info["pair"][0], "bound", info["loss_bound"])
    assert (s.total_pos, s.total_neg) == (info["n_pos"], info["n_neg"]) and not s.n_bad.any()
    assert abs(s.roc_auc() - info["auc"]) <= info["auc_bound"]
    assert auc == info["pair"][1]
    assert abs(loss - info["pair"][0]) <= info["loss_bound"]
    assert validate(recs, labels, model, sr, noise_loss=info["noise_loss"], batch_size=info["batch_size"]) == (loss, auc)
