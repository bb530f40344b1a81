"""Audio augmentations of decoder fine-tuning without a GPU: the filter design (vad_biquad_design) against scipy.signal and the identities
of the Audio-EQ-cookbook forms, the host twin (vad_augment_rows_host) op by op against scipy / numpy, the composition rules, the recipe
check, and `Augmenter`'s draw.

Yardsticks.  audiomentations is not available, so nothing here is pinned to it: BIQUADS is scipy.signal.sosfilt in double rounded once
(1 float32 ulp: both compute in double and round once, a difference in the double result can only move a value across a rounding
boundary); CLIP is np.clip at np.percentile's default method, bit for bit; NOISE is Box-Muller in double over the test's own numpy
Philox4x32-10 (checked against Random123's known answers), 4 float32 ulp.

np.percentile interpolates in the precision of its input: on a float32 array a Python-float percentile is divided by np.float32(100)
and the virtual index and the weight are float32 as well.  The rule here interpolates in double, so the reference is np.percentile of
the same values as float64 -- the same order statistics, numpy's own formula -- rounded to float32.
"""
import ctypes

import numpy as np
import pytest
import scipy.signal as sig

from conftest import GOLD, SRS

SQ = 1.0 / np.sqrt(2.0)


@pytest.fixture(scope="module")
def aug(built):
    from silero_vad_amd import augment
    return augment


def speech(tag, n, start=40000):
    return np.load(GOLD / f"audio_{tag}.npz")["pcm"][start:start + n]


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32)))


def sos6(coef):
    c = np.atleast_2d(coef)
    return np.concatenate([c[:, :3], np.ones((c.shape[0], 1)), c[:, 3:]], axis=1)


def mag(coef, f, sr):
    _, h = sig.sosfreqz(sos6(coef), worN=np.atleast_1d(np.asarray(f, dtype=np.float64)), fs=sr)
    return np.abs(h)


# ---- filter design -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [16000, 8000])
@pytest.mark.parametrize("f0", [20.0, 150.0, 1000.0, 3500.0])
def test_butterworth_sections_equal_scipy(aug, sr, f0):
    for kind, btype in (("lowpass", "low"), ("highpass", "high")):
        got = aug.biquad_design(kind, sr, f0, SQ)
        want = sig.butter(2, f0, btype, fs=sr, output="sos")[0]
        assert np.abs(sos6(got)[0] - want).max() <= 1e-12, (kind, got, want)
        # 24 dB/oct: the pairing of numerator and denominator factors may differ, so compare as responses
        two = aug.butterworth(kind, sr, f0, 24)
        assert two.shape == (2, 5)
        f = np.geomspace(10.0, 0.499 * sr, 64)
        _, h = sig.sosfreqz(sos6(two), worN=f, fs=sr)
        _, hw = sig.sosfreqz(sig.butter(4, f0, btype, fs=sr, output="sos"), worN=f, fs=sr)
        assert (np.abs(h - hw) / np.abs(hw)).max() <= 1e-10, kind


@pytest.mark.parametrize("sr,f0,q,gain", [(16000, 50.0, 5.0, 24.0), (16000, 1000.0, 0.5, -24.0), (8000, 3000.0, 2.0, 7.5), (16000, 7000.0, 1.0, -3.0)])
def test_cookbook_identities(aug, sr, f0, q, gain):
    lin, ny = 10.0 ** (gain / 20.0), sr / 2.0
    pk = aug.biquad_design("peaking", sr, f0, q, gain)
    assert abs(mag(pk, f0, sr)[0] - lin) <= 1e-9 * lin
    assert np.abs(mag(pk, [0.0, ny], sr) - 1.0).max() <= 1e-9
    lo = aug.biquad_design("lowshelf", sr, f0, min(q, 0.999), gain)
    assert np.abs(mag(lo, [0.0, ny], sr) - [lin, 1.0]).max() <= 1e-9 * max(lin, 1.0)
    hi = aug.biquad_design("highshelf", sr, f0, min(q, 0.999), gain)
    assert np.abs(mag(hi, [0.0, ny], sr) - [1.0, lin]).max() <= 1e-9 * max(lin, 1.0)
    assert mag(aug.biquad_design("notch", sr, f0, q), f0, sr)[0] < 1e-9
    bp = aug.biquad_design("bandpass", sr, f0, q)
    assert abs(mag(bp, f0, sr)[0] - 1.0) <= 1e-9 and mag(bp, [0.0, ny], sr).max() <= 1e-9


def test_design_refuses_bad_arguments(aug):
    from silero_vad_amd._lib import VadError
    for args in (("lowpass", 16000, 0.0), ("lowpass", 16000, 8000.0), ("lowpass", 0, 100.0), ("peaking", 16000, 100.0, 0.0),
                 ("peaking", 16000, 100.0, 1.0, float("nan")), (7, 16000, 100.0), (-1, 16000, 100.0)):
        with pytest.raises(VadError, match="VAD_ERR_ARG"):
            aug.biquad_design(*args)


# ---- BIQUADS twin ------------------------------------------------------------------------------------------------------------------
def biquad_cases(aug, sr):
    ny = 0.45 * sr
    eq = np.stack([aug.biquad_design(k, sr, min(f, ny), q, g) for k, f, q, g in
                   (("lowshelf", 100, SQ, 9.0), ("peaking", 200, 1.0, -12.0), ("peaking", 400, 1.0, 12.0), ("peaking", 800, 2.0, -6.0),
                    ("peaking", 1600, 1.0, 5.0), ("peaking", 3200, 0.7, -11.0), ("highshelf", 6400, SQ, 12.0), ("notch", 1000, 1.5, 0.0))])
    return {"one section": aug.biquad_design("highshelf", sr, 3000.0, 0.5, -18.0)[None], "eight sections": eq,
            "peaking 50 Hz q 5 +24 dB": aug.biquad_design("peaking", sr, 50.0, 5.0, 24.0)[None],
            "24 dB/oct low-pass 150 Hz": aug.butterworth("lowpass", sr, 150.0, 24)}


@pytest.mark.parametrize("tag", list(SRS))
@pytest.mark.parametrize("as_int16", [True, False])
def test_biquads_twin_is_sosfilt(aug, tag, as_int16):
    pcm = speech(tag, 48000)
    x = pcm if as_int16 else (pcm.astype(np.float32) / 32768.0)
    x64 = pcm.astype(np.float64) / 32768.0
    for name, coef in biquad_cases(aug, SRS[tag]).items():
        got = aug.augment_host(x[None], [x.size], aug.make_recipes([[("biquads", coef)]]))[0]
        want = sig.sosfilt(sos6(coef), x64).astype(np.float32)
        worst = float((np.abs(got.astype(np.float64) - want) / ulp32(want)).max())
        print(tag, name, "worst difference", worst, "ulp; peak", float(np.abs(want).max()))
        assert worst <= 1.0, name


# ---- CLIP twin ---------------------------------------------------------------------------------------------------------------------
def clip_reference(x, q_lo, q_hi):
    x64 = x.astype(np.float64)
    return np.clip(x, np.float32(np.percentile(x64, 100 * q_lo)), np.float32(np.percentile(x64, 100 * q_hi)))


def clip_rows():
    rng = np.random.default_rng(5)
    sp = speech("16k", 30001).astype(np.float32) / 32768.0
    ties = (rng.integers(-3, 4, 5000).astype(np.float32) / 32768.0)
    return {"speech": sp, "ties": ties, "constant": np.full(777, 0.25, np.float32), "len 1": sp[100:101].copy(), "len 2": sp[100:102].copy(),
            "normal": rng.standard_normal(4099).astype(np.float32)}


QUANTILES = [(0.0, 1.0), (0.1, 0.9), (0.2, 0.8), (0.5, 0.5)]


@pytest.mark.parametrize("q", QUANTILES)
def test_clip_twin_is_numpy(aug, q):
    for name, x in clip_rows().items():
        got = aug.augment_host(x[None], [x.size], aug.make_recipes([[("clip", *q)]]))[0]
        want = clip_reference(x, *q)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, q)


def test_clip_other_quantiles(aug):
    """the interpolation weight between two order statistics, away from the four pairs above"""
    rng = np.random.default_rng(6)
    done = 0
    while done < 40:
        lo = float(rng.uniform(0, 0.5))
        q = (lo, float(rng.uniform(lo, 1.0)))
        if (100 * q[0]) / 100 != q[0] or (100 * q[1]) / 100 != q[1]:
            continue                                           # (np.percentile takes 100 q and divides by 100 again: keep the q that survive)
        done += 1
        x = rng.standard_normal(int(rng.integers(1, 700))).astype(np.float32)
        got = aug.augment_host(x[None], [x.size], aug.make_recipes([[("clip", *q)]]))[0]
        assert np.array_equal(got.view(np.uint32), clip_reference(x, *q).view(np.uint32)), q


# ---- NOISE twin --------------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """numpy Philox4x32-10: counter [n, 4] uint32, key [2] uint32 -> [n, 4] uint32"""
    c = [counter[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, axis=1).astype(np.uint32)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 10"""
    z = philox4x32_10(np.zeros((1, 4), np.uint32), np.zeros(2, np.uint32))[0]
    assert [hex(v) for v in z] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    f = philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), np.full(2, 0xFFFFFFFF, np.uint32))[0]
    assert [hex(v) for v in f] == ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]


def gauss_reference(seed, row_key, n):
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), np.full_like(q, row_key & 0xFFFFFFFF), np.full_like(q, row_key >> 32)], axis=1)
    w = philox4x32_10(ctr.astype(np.uint32), np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)).astype(np.float64)
    u = (w + 0.5) / 4294967296.0
    out = np.empty((q.size, 4))
    for h in (0, 1):
        r, a = np.sqrt(-2.0 * np.log(u[:, 2 * h])), 2.0 * np.pi * u[:, 2 * h + 1]
        out[:, 2 * h], out[:, 2 * h + 1] = r * np.cos(a), r * np.sin(a)
    return out.reshape(-1)[:n]


def twin_noise(aug, n, seed, row_key, amplitude=2.0 ** -7):
    """(y - x) / amplitude of the twin at x = 0 with a power-of-two amplitude: the generator's float32 values themselves"""
    y = aug.augment_host(np.zeros((1, n), np.float32), [n], aug.make_recipes([[("noise", amplitude, seed)]], row_keys=[row_key]))[0]
    return y / np.float32(amplitude)


def test_noise_twin_is_box_muller_of_philox(aug):
    for seed, key, n in ((0, 0, 4099), (0x123456789ABCDEF, 7, 1001), (5, 0xFEDCBA9876543210, 1 << 16)):
        g = twin_noise(aug, n, seed, key)
        want = gauss_reference(seed, key, n)
        worst = float((np.abs(g.astype(np.float64) - want) / ulp32(want)).max())
        print("noise twin against numpy:", worst, "ulp")
        assert worst <= 4.0


def test_noise_is_added_in_double_and_rounded_once(aug):
    x = speech("16k", 5000).astype(np.float32) / 32768.0
    amp = 0.0123
    g = twin_noise(aug, x.size, 11, 3)
    y = aug.augment_host(x[None], [x.size], aug.make_recipes([[("noise", amp, 11)]], row_keys=[3]))[0]
    want = (x.astype(np.float64) + np.float64(np.float32(amp)) * g.astype(np.float64)).astype(np.float32)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))


def test_noise_statistics_and_independence(aug):
    n = 1 << 20
    a = twin_noise(aug, n, 1, 0).astype(np.float64)
    assert abs(a.mean()) <= 5 / np.sqrt(n) and abs(a.var() - 1.0) <= 5 * np.sqrt(2.0 / n)
    for seed, key in ((1, 1), (2, 0)):
        b = twin_noise(aug, n, seed, key).astype(np.float64)
        assert abs(np.corrcoef(a, b)[0, 1]) <= 5 / np.sqrt(n), (seed, key)
    # a sample's noise depends on (seed, row_key, n) alone: not on the row's place, the batch or the length
    y = aug.augment_host(np.zeros((3, 1000), np.float32), [10, 1000, 999], aug.make_recipes([[("noise", 2.0 ** -7, 1)]] * 3, row_keys=[5, 0, 0]))
    assert np.array_equal(y[1] / np.float32(2.0 ** -7), a[:1000].astype(np.float32)) and np.array_equal(y[2, :999], y[1, :999])


# ---- composition and rules ---------------------------------------------------------------------------------------------------------
def test_composition_and_rules(aug):
    sr = 16000
    x = speech("16k", 3000)
    ops = [("noise", 0.01, 9), ("clip", 0.05, 0.95), ("biquads", aug.butterworth("highpass", sr, 300.0, 24))]
    width, ln = 3100, 2999
    xin = np.zeros((1, width), np.int16)
    xin[0, :3000] = x
    got = aug.augment_host(xin, [ln], aug.make_recipes([ops], row_keys=[4]))
    y = xin
    for op in ops:
        y = aug.augment_host(y, [ln], aug.make_recipes([[op]], row_keys=[4]))
    assert np.array_equal(got.view(np.uint32), y.view(np.uint32))
    assert np.all(got[0, ln:] == 0.0) and np.any(got[0, :ln] != 0.0)
    # an empty recipe: the input's float32 bits, int16 as x / 32768, zero behind len
    e = aug.augment_host(xin, [ln], aug.make_recipes([[]]))
    want = np.zeros(width, np.float32)
    want[:ln] = xin[0, :ln].astype(np.float32) / np.float32(32768.0)
    assert np.array_equal(e[0].view(np.uint32), want.view(np.uint32))
    f = np.float32(np.random.default_rng(0).standard_normal((2, 50)))
    f[0, 3] = -0.0
    e = aug.augment_host(f, [50, 20], aug.make_recipes([[], []]))
    assert np.array_equal(e[0].view(np.uint32), f[0].view(np.uint32)) and np.array_equal(e[1, :20], f[1, :20]) and np.all(e[1, 20:] == 0)
    # the reference's NaN rule: a non-finite result gives the row back as it came; its neighbour is filtered
    f = np.float32(np.random.default_rng(1).standard_normal((2, 400)))
    f[0, 100] = np.inf
    rec = aug.make_recipes([[("biquads", aug.biquad_design("lowpass", sr, 1000.0)[None])]] * 2)
    e = aug.augment_host(f, [400, 400], rec)
    assert np.array_equal(e[0].view(np.uint32), f[0].view(np.uint32))
    assert not np.array_equal(e[1], f[1]) and np.all(np.isfinite(e[1]))
    # rows do not see each other, and the thread count does not matter
    many = np.float32(np.random.default_rng(2).standard_normal((5, 700)))
    recs = aug.make_recipes([[("noise", 0.1, 1)], [], ops, [ops[1]], [ops[2], ops[0]]])
    lens = [700, 300, 699, 1, 0]
    all_ = aug.augment_host(many, lens, recs, threads=3)
    for i in range(5):
        solo = aug.augment_host(many[i:i + 1], lens[i:i + 1], recs[i:i + 1], threads=1)
        assert np.array_equal(all_[i].view(np.uint32), solo[0].view(np.uint32)), i


def test_bad_arguments(aug, built):
    from silero_vad_amd import _lib
    from silero_vad_amd._lib import VadError
    x = np.zeros((1, 64), np.float32)
    good = aug.make_recipes([[("biquads", aug.biquad_design("lowpass", 16000, 1000.0)[None]), ("clip", 0.1, 0.9), ("noise", 0.01, 1)]])
    aug.check_recipes(good)

    def broken(edit):
        r = good.copy()
        edit(r[0])
        return r

    def set_n_ops(r): r["n_ops"] = 4
    def set_sections(r): r["ops"][0]["n_sections"] = 9
    def set_no_sections(r): r["ops"][0]["n_sections"] = 0
    def set_coef(r): r["ops"][0]["coef"][0, 3] = np.nan
    def set_q_low(r): r["ops"][1]["a"] = -0.01
    def set_q_high(r): r["ops"][1]["b"] = 1.01
    def set_q_order(r): r["ops"][1]["a"], r["ops"][1]["b"] = 0.6, 0.4
    def set_kind(r): r["ops"][2]["kind"] = 9
    for edit, text in ((set_n_ops, "n_ops"), (set_sections, "n_sections"), (set_no_sections, "n_sections"), (set_coef, "non-finite"),
                       (set_q_low, "quantiles"), (set_q_high, "quantiles"), (set_q_order, "quantiles"), (set_kind, "kind")):
        with pytest.raises(VadError, match=text) as err:
            aug.augment_host(x, [64], broken(edit))
        assert err.value.status == 1
        # the C call itself refuses too, not only the wrapper's check
        r, out, ln = broken(edit), np.zeros((1, 64), np.float32), np.array([64], np.int64)
        assert _lib.lib().vad_augment_rows_host(x.ctypes.data, 4, 64, ln.ctypes.data, 1, r.ctypes.data, out.ctypes.data, 64, 1) == 1
    L, ln, out = _lib.lib(), np.array([65], np.int64), np.zeros((1, 64), np.float32)
    assert L.vad_augment_rows_host(x.ctypes.data, 4, 64, ln.ctypes.data, 1, good.ctypes.data, out.ctypes.data, 64, 1) == 1     # len > ld
    ln[0] = 64
    assert L.vad_augment_rows_host(x.ctypes.data, 3, 64, ln.ctypes.data, 1, good.ctypes.data, out.ctypes.data, 64, 1) == 1     # elem_size
    assert L.vad_augment_rows_host(None, 4, 64, ln.ctypes.data, 1, good.ctypes.data, out.ctypes.data, 64, 1) == 1
    assert L.vad_augment_rows_host(x.ctypes.data, 4, 64, ln.ctypes.data, 1, good.ctypes.data, out.ctypes.data, 64, 1) == 0
    assert L.vad_augment_workspace_bytes(0, 10) == 0 and L.vad_augment_workspace_bytes(128, 128000) >= 128 * 500 * 128
    # a host-only engine refuses the device call loudly
    blob = _lib.WEIGHTS_PATH.read_bytes()
    h = ctypes.c_void_p()
    assert L.vad_create_host_only(blob, len(blob), ctypes.byref(h)) == 0
    assert L.vad_augment_rows_device(h, None, 4, 64, None, 1, None, None, 64, None, 0, None) == 4 and b"host-only" in L.vad_last_error(h)
    assert L.vad_augment_rows_device(None, None, 4, 64, None, 1, None, None, 64, None, 0, None) == 1
    L.vad_destroy(h)


# ---- Augmenter ---------------------------------------------------------------------------------------------------------------------
def test_augmenter_draws(aug):
    a, b = aug.Augmenter(p=0.5, seed=3), aug.Augmenter(p=0.5, seed=3)
    ra, rb = a.draw(64), b.draw(64)
    assert ra.tobytes() == rb.tobytes() and a.draw(64).tobytes() != ra.tobytes()
    assert aug.Augmenter(p=0.5, seed=4).draw(64).tobytes() != ra.tobytes()
    assert 0 < (ra["n_ops"] == 0).sum() < 64
    assert np.all(aug.Augmenter(p=0.0).draw(50)["n_ops"] == 0)
    assert list(ra["row_key"]) == list(range(64)) and list(a.draw(3, row_keys=[9, 2, 5])["row_key"]) == [9, 2, 5]
    order = {t: i for i, t in enumerate(aug.TRANSFORMS)}
    for sr in (16000, 8000):
        g = aug.Augmenter(p=1.0, sampling_rate=sr, seed=1)
        rec = g.draw(400)
        aug.check_recipes(rec)
        assert np.all((rec["n_ops"] >= 1) & (rec["n_ops"] <= 3)) and set(rec["n_ops"]) == {1, 2, 3}
        seen = set()
        for r, prms in zip(rec, g.last_params):
            names = [n for n, _ in prms]
            assert len(names) == r["n_ops"] and len(set(names)) == len(names) and names == sorted(names, key=order.get)
            seen.update(names)
            for (name, prm), op in zip(prms, r["ops"]):
                for f in np.atleast_1d(prm.get("f0", [])):
                    assert 0.0 < f < 0.45 * sr, (name, f)
                if op["kind"] == aug.BIQUADS:
                    for c in op["coef"][:op["n_sections"]]:
                        assert np.abs(np.roots([1.0, c[3], c[4]])).max() < 1.0, (name, prm)      # poles inside the unit circle
                elif op["kind"] == aug.CLIP:
                    assert 0.0 <= op["a"] <= 0.2 and 0.8 <= op["b"] <= 1.0 and abs(op["a"] + op["b"] - 1.0) < 1e-12
                else:
                    assert op["kind"] == aug.NOISE and 0.001 <= op["a"] <= 0.015
        assert seen == set(aug.TRANSFORMS)
    only = aug.Augmenter(p=1.0, seed=2, transforms=["noise"], noise_amplitude=(0.5, 0.5))
    rec = only.draw(20)
    assert np.all(rec["n_ops"] == 1) and np.all(rec["ops"][:, 0]["kind"] == aug.NOISE) and np.all(rec["ops"][:, 0]["a"] == 0.5)
    assert len(set(rec["ops"][:, 0]["seed"].tolist())) == 20
    with pytest.raises(ValueError):
        aug.Augmenter(transforms=["reverb"])
    with pytest.raises(TypeError):
        aug.Augmenter(no_such_range=(0, 1))


def test_exported_from_the_package(built):
    import silero_vad_amd
    for name in ("Augmenter", "augment_device", "augment_host", "biquad_design", "make_recipes", "RECIPE_DTYPE"):
        assert hasattr(silero_vad_amd, name), name
