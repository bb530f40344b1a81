"""Room reverb (FIR) and aliasing (ALIAS) of decoder fine-tuning without a GPU: the host twin (vad_augment_rows_host_x) against numpy,
the shoebox room response (vad_rir_shoebox) against a numpy restatement of its rule, the recipe check with a bank, `fir_bank`, and the
`Augmenter` with the twelve transforms.

Yardsticks.  ALIAS is audiomentations' Aliasing written out as two np.interp calls on np.linspace grids: bit for bit.  FIR is
np.convolve of the float64 values cut to len and rounded to float32: both sides sum exact products in double and round once, numpy in
another order, so a difference of the double sums (about K 2^-53 of the sum of magnitudes) can only move a value across a rounding
boundary, or show where the sum cancels far below its terms: the bound is 1 float32 ulp of the value plus 2^-40 of sum |h||x|
(K 2^-53 <= 2^-40 at K = 8192).  Measured here: 0 of the values differ at every K.  rir_shoebox: 2^-22 absolute, one float32 rounding
of values below 2.
"""
import ctypes

import numpy as np
import pytest

from conftest import GOLD

ALIAS_LENS = [1, 2, 3, 255, 256, 257, 773, 10247]
ALIAS_RATES = [4000, 8000, 11025, 15999, 16000]
FIR_TAPS = [1, 2, 3, 4, 5, 16, 17, 255, 8192]


@pytest.fixture(scope="module")
def aug(built):
    from silero_vad_amd import augment
    return augment


def speech(n, start=40000):
    return np.load(GOLD / "audio_16k.npz")["pcm"][start:start + n]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def batch_of(lens, kind="float32", start=30000):
    x = np.zeros((len(lens), max(lens)), np.int16)
    for i, n in enumerate(lens):
        x[i, :n] = speech(n, start + 9000 * i)
    return x if kind == "int16" else x.astype(np.float32) / np.float32(32768.0)


def alias_numpy(samples, a, b):
    """audiomentations' Aliasing as remembered: down to the new rate and back by linear interpolation, without a filter"""
    n = len(samples)
    m = round(n * float(a) / b)
    if n < 2 or m < 2:
        return np.asarray(samples, np.float32).copy()
    x = np.linspace(0, n, num=n)
    dx = np.linspace(0, n, num=m)
    return np.interp(x, dx, np.interp(dx, x, samples)).astype(np.float32)


# ---- ALIAS ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int16", "float32"])
@pytest.mark.parametrize("rate", ALIAS_RATES)
def test_alias_twin_is_numpy_bit_for_bit(aug, rate, kind):
    x = batch_of(ALIAS_LENS, kind)
    xf = x.astype(np.float32) / np.float32(32768.0) if kind == "int16" else x
    rec = aug.make_recipes([[("alias", rate, 16000)]] * len(ALIAS_LENS))
    got = aug.augment_host(x, ALIAS_LENS, rec, bank=np.zeros(0, np.float32))
    differ = 0
    for i, n in enumerate(ALIAS_LENS):
        want = alias_numpy(xf[i, :n], rate, 16000)
        differ += int((bits(got[i, :n]) != bits(want)).sum())
        assert np.all(got[i, n:] == 0.0)
        if rate == 16000 or n < 2 or round(n * rate / 16000) < 2:
            assert np.array_equal(bits(got[i, :n]), bits(xf[i, :n])), (rate, n)      # a == b, or too short: the input
    print(f"alias {rate}/16000 {kind}: {differ} of {sum(ALIAS_LENS)} samples differ from numpy")
    assert differ == 0
    if rate == 4000:
        assert not np.array_equal(got[7], xf[7])                                     # (something was aliased)


def test_alias_short_rows_and_threads(aug):
    x = batch_of([1, 2, 3, 5, 773])
    lens = [1, 2, 3, 5, 773]
    rec = aug.make_recipes([[("alias", 3000, 16000)]] * 5)                           # m = 0, 0, 1, 1, 145
    got = aug.augment_host(x, lens, rec, bank=[])
    for i in range(4):
        assert np.array_equal(bits(got[i]), bits(x[i])), i
    assert np.array_equal(bits(got[4, :773]), bits(alias_numpy(x[4, :773], 3000, 16000)))
    for threads in (1, 3, 8):
        assert np.array_equal(bits(aug.augment_host(x, lens, rec, threads=threads, bank=[])), bits(got))


# ---- FIR -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fir_case(aug):
    """a bank of random responses of every K at odd offsets, and rows shorter and longer than K"""
    rng = np.random.default_rng(11)
    responses = [np.ones(1, np.float32) * 7]                                         # (one tap of padding: every offset below is odd or shifted)
    for K in FIR_TAPS:
        h = (rng.standard_normal(K) * np.exp(-np.arange(K) / max(K / 4.0, 1.0))).astype(np.float32)
        responses += [h, np.zeros(2 - K % 2, np.float32)]                            # the next response starts at an odd offset
    bank, offs, lens = aug.fir_bank(responses)
    return bank, offs[1::2], lens[1::2]


@pytest.mark.parametrize("kind", ["int16", "float32"])
def test_fir_twin_against_numpy_convolve(aug, fir_case, kind):
    bank, offs, taps = fir_case
    assert list(taps) == FIR_TAPS and all(int(o) % 2 == 1 for o in offs)
    lens = [1, 3, 100, 257, 9000]
    x = batch_of(lens, kind)
    xf = x.astype(np.float32) / np.float32(32768.0) if kind == "int16" else x
    worst, differ, total = 0.0, 0, 0
    for o, K in zip(offs, taps):
        rec = aug.make_recipes([[("fir", int(o), int(K))]] * len(lens))
        got = aug.augment_host(x, lens, rec, bank=bank)
        h = bank[o:o + K].astype(np.float64)
        for i, n in enumerate(lens):
            full = np.convolve(xf[i, :n].astype(np.float64), h)[:n]
            want = full.astype(np.float32)
            S = np.convolve(np.abs(xf[i, :n].astype(np.float64)), np.abs(h))[:n]
            d = np.abs(got[i, :n].astype(np.float64) - want.astype(np.float64))
            bound = np.spacing(np.abs(want)).astype(np.float64) + 2.0 ** -40 * S
            worst = max(worst, float((d / np.maximum(bound, 1e-300)).max()))
            differ += int((bits(got[i, :n]) != bits(want)).sum())
            total += n
            assert np.all(d <= bound), (K, n)
            assert np.all(got[i, n:] == 0.0)
    print(f"fir twin {kind}: {differ} of {total} values differ from np.convolve, worst {worst} x the bound")


def test_fir_identities(aug):
    """K = 1 is one rounded product; a single 1.0 at tap d is a delay; silence longer than K stays exactly zero behind the tail"""
    lens = [1, 17, 300, 9000]
    x = batch_of(lens)
    bank = np.zeros(1 + 8192, np.float32)
    bank[0] = np.float32(0.37)
    got = aug.augment_host(x, lens, aug.make_recipes([[("fir", 0, 1)]] * 4), bank=bank)
    assert np.array_equal(bits(got), bits(x * np.float32(0.37)))
    for d in (0, 1, 15, 16, 17, 255, 8191):
        bank[1:] = 0.0
        bank[1 + d] = 1.0
        got = aug.augment_host(x, lens, aug.make_recipes([[("fir", 1, d + 1)]] * 4), bank=bank)
        for i, n in enumerate(lens):
            want = np.zeros(x.shape[1], np.float32)
            if n > d:
                want[d:n] = x[i, :n - d]
            assert np.array_equal(bits(got[i] + 0.0), bits(want)), (d, n)
    rng = np.random.default_rng(5)
    h = rng.standard_normal(255).astype(np.float32)
    y = x[3:4].copy()
    y[0, 2000:4000] = 0.0
    got = aug.augment_host(y, [9000], aug.make_recipes([[("fir", 0, 255)]]), bank=h)
    assert np.all(got[0, 2000 + 254:4000] == 0.0) and np.any(got[0, 2000:2000 + 254] != 0.0)


def test_new_ops_compose_with_the_old_ones(aug):
    """each op reads the float32 output of the op before it; a non-finite result gives the row back"""
    lens = [773, 2049]
    x = batch_of(lens)
    rng = np.random.default_rng(2)
    bank = rng.standard_normal(40).astype(np.float32)
    lp = aug.butterworth("lowpass", 16000, 2000.0, 12)
    ops = [("alias", 9000, 16000), ("biquads", lp), ("fir", 3, 37)]
    rec = aug.make_recipes([ops, ops[::-1]])
    got = aug.augment_host(x, lens, rec, bank=bank)
    for i, order in enumerate((ops, ops[::-1])):
        y = x[i:i + 1]
        for op in order:
            y = aug.augment_host(y, lens[i:i + 1], aug.make_recipes([[op]]), bank=bank)
        assert np.array_equal(bits(got[i]), bits(y[0])), i
    bad = x.copy()
    bad[1, 100] = np.inf
    got = aug.augment_host(bad, lens, aug.make_recipes([[("fir", 0, 5)]] * 2), bank=bank)
    assert np.array_equal(bits(got[1]), bits(bad[1])) and not np.array_equal(got[0], x[0])


# ---- the shoebox room ----------------------------------------------------------------------------------------------------------------
def shoebox_numpy(sr, room, src, mic, absorption, max_order, n_taps):
    beta, c = np.sqrt(1.0 - absorption), 343.0
    room, src, mic = (np.asarray(v, np.float64) for v in (room, src, mic))
    d0 = np.sqrt(((src - mic) ** 2).sum())
    h = np.zeros(n_taps + 1)
    rng = range(-max_order, max_order + 1)
    for nx in rng:
        for ny in rng:
            for nz in rng:
                for px in (0, 1):
                    for py in (0, 1):
                        for pz in (0, 1):
                            n, p = np.array([nx, ny, nz]), np.array([px, py, pz])
                            R = int((np.abs(n - p) + np.abs(n)).sum())
                            if R > max_order:
                                continue
                            image = 2 * n * room + (1 - 2 * p) * src
                            d = np.sqrt(((image - mic) ** 2).sum())
                            A = (1.0 if R == 0 else beta ** R) * d0 / d
                            t = (d - d0) * sr / c
                            j = int(np.floor(t))
                            f = t - j
                            if j < n_taps:
                                h[j] += A * (1 - f)
                                h[j + 1] += A * f
    return h[:n_taps]


ROOM = dict(room=[4.7, 3.8, 2.6], source=[1.1, 2.9, 1.5], microphone=[3.2, 0.9, 1.2])


@pytest.mark.parametrize("absorption,max_order,n_taps", [(0.25, 3, 2048), (0.075, 5, 1000), (0.4, 0, 64), (0.3, 4, 1)])
def test_rir_shoebox_against_the_rule_in_numpy(aug, absorption, max_order, n_taps):
    got = aug.rir_shoebox(16000, ROOM["room"], ROOM["source"], ROOM["microphone"], absorption, max_order, n_taps)
    want = shoebox_numpy(16000, ROOM["room"], ROOM["source"], ROOM["microphone"], absorption, max_order, n_taps)
    assert got.dtype == np.float32 and got.shape == (n_taps,)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"shoebox absorption {absorption} order {max_order}: max error {err:.3e}, peak {np.abs(want).max():.3f}, {np.count_nonzero(want)} taps set")
    assert np.abs(want).max() < 2.0 and err <= 2.0 ** -22
    assert got[0] >= 1.0 or n_taps == 1 or max_order == 0                            # the direct sound at tap 0 with gain 1


def test_rir_shoebox_properties_and_refusals(aug):
    from silero_vad_amd._lib import VadError
    dead = aug.rir_shoebox(16000, ROOM["room"], ROOM["source"], ROOM["microphone"], 1.0, 12, 4096)
    want = np.zeros(4096, np.float32)
    want[0] = 1.0
    assert np.array_equal(bits(dead), bits(want))
    tail = []
    for absorption in (0.1, 0.4):
        h = aug.rir_shoebox(16000, ROOM["room"], ROOM["source"], ROOM["microphone"], absorption, 12, 8192).astype(np.float64)
        assert h[0] == pytest.approx(1.0, abs=1e-6) or h[0] > 1.0
        tail.append(float((h[800:] ** 2).sum()))
    print("energy behind 50 ms at absorption 0.1, 0.4:", tail)
    assert tail[0] > tail[1] > 0.0
    ok = dict(sampling_rate=16000, room=ROOM["room"], source=ROOM["source"], microphone=ROOM["microphone"], absorption=0.3, max_order=2, n_taps=64)
    aug.rir_shoebox(**ok)
    refused = [dict(source=[4.8, 1.0, 1.0]), dict(microphone=[1.0, 1.0, 2.6]), dict(source=[0.0, 1.0, 1.0]), dict(microphone=ROOM["source"]),
               dict(room=[4.7, np.inf, 2.6]), dict(room=[4.7, 0.0, 2.6]), dict(room=[-4.7, 3.8, 2.6]), dict(room=[4.7, np.nan, 2.6]),
               dict(n_taps=0), dict(n_taps=8193), dict(absorption=0.0), dict(absorption=1.5), dict(max_order=-1), dict(sampling_rate=0.0)]
    for change in refused:
        with pytest.raises(VadError, match="VAD_ERR_ARG"):
            aug.rir_shoebox(**dict(ok, **change))


# ---- the check, the bank -------------------------------------------------------------------------------------------------------------
def test_check_recipes_with_a_bank(aug):
    from silero_vad_amd._lib import VadError, lib
    good = aug.make_recipes([[("fir", 3, 17), ("alias", 8000, 16000)], [("alias", 16000, 16000)], [("fir", 0, 20)]])
    aug.check_recipes(good, bank_len=20)
    aug.check_recipes(aug.make_recipes([[("noise", 0.01, 1)]]), bank_len=0)
    cases = [([("fir", 0, 0)], 20, "fir taps outside 1 .. 8192"), ([("fir", 0, 8193)], 9000, "fir taps outside 1 .. 8192"),
             ([("fir", 4, 17)], 20, "fir taps outside the bank"), ([("fir", 21, 1)], 20, "fir taps outside the bank"),
             ([("fir", 2 ** 63, 1)], 20, "fir taps outside the bank"), ([("fir", 0, 1)], 0, "fir taps outside the bank"),
             ([("alias", 0, 16000)], 0, "aliasing rates must satisfy 0 < new rate <= rate"), ([("alias", 16001, 16000)], 0, "aliasing rates"),
             ([("alias", np.nan, 16000)], 0, "aliasing rates"), ([("alias", 8000, np.inf)], 0, "aliasing rates"),
             ([("noise", 0.1, 1), ("clip", 0.5, 0.4)], 5, "quantiles")]
    for ops, bank_len, why in cases:
        with pytest.raises(VadError, match=why):
            aug.check_recipes(aug.make_recipes([[], ops]), bank_len=bank_len)
    # without a bank both kinds are unknown, as they were; the entry point without a bank refuses them
    for ops in ([("fir", 0, 1)], [("alias", 8000, 16000)]):
        with pytest.raises(VadError, match="unknown op kind"):
            aug.check_recipes(aug.make_recipes([ops]))
        with pytest.raises(VadError, match="unknown op kind"):
            aug.augment_host(np.zeros((1, 8), np.float32), [8], aug.make_recipes([ops]))
    x, ln, out = np.zeros((1, 8), np.float32), np.array([8], np.int64), np.zeros((1, 8), np.float32)
    bank = np.ones(4, np.float32)
    for ops, inside in (([("fir", 0, 4)], True), ([("fir", 1, 4)], False)):
        rec = aug.make_recipes([ops])
        rc_old = lib().vad_augment_rows_host(x.ctypes.data, 4, 8, ln.ctypes.data, 1, rec.ctypes.data, out.ctypes.data, 8, 1)
        rc_new = lib().vad_augment_rows_host_x(x.ctypes.data, 4, 8, ln.ctypes.data, 1, rec.ctypes.data, out.ctypes.data, 8, bank.ctypes.data, 4, 1)
        assert rc_old != 0 and (rc_new == 0) == inside, ops                          # a range outside the bank is refused
    assert lib().vad_augment_rows_host_x(x.ctypes.data, 4, 8, ln.ctypes.data, 1, rec.ctypes.data, out.ctypes.data, 8, None, 4, 1) != 0
    assert lib().vad_augment_check_recipes_bank(good.ctypes.data, 3, -1, None) != 0
    # the structs keep their sizes, the workspace its values
    assert aug.OP_DTYPE.itemsize == 352 and aug.RECIPE_DTYPE.itemsize == 1072
    assert aug.augment_scratch_bytes(3, 1001) == (3 * 1001 * 4 + 255) // 256 * 256 and aug.augment_scratch_bytes(0, 4) == 0


def test_fir_bank_packs_and_refuses(aug):
    bank, offs, lens = aug.fir_bank([[1.0, 2.0], np.arange(5.0), [3.0]])
    assert bank.dtype == np.float32 and list(bank) == [1, 2, 0, 1, 2, 3, 4, 3] and list(offs) == [0, 2, 7] and list(lens) == [2, 5, 1]
    for bad in ([[1.0, np.nan]], [[np.inf]], [[]], [np.zeros((2, 2))], [np.zeros(8193)]):
        with pytest.raises(ValueError):
            aug.fir_bank(bad)
    with pytest.raises(ValueError):
        aug.make_recipes([[("fir", -1, 2)]])


# ---- the Augmenter -------------------------------------------------------------------------------------------------------------------
def test_augmenter_with_the_twelve(aug):
    assert aug.ALL_TRANSFORMS == ("aliasing", "noise", "band_pass", "band_stop", "clipping", "high_pass", "high_shelf", "low_pass", "low_shelf",
                                  "peaking", "room", "seven_band_eq")
    assert len(aug.TRANSFORMS) == 10 and set(aug.TRANSFORMS) == set(aug.ALL_TRANSFORMS) - {"aliasing", "room"}
    # the default is the ten it was, and carries no bank
    d = aug.Augmenter(p=1.0, seed=1)
    assert d.transforms == aug.TRANSFORMS and d.bank is None and not d.needs_bank
    d.draw(200)
    assert {name for row in d.last_params for name, _ in row} == set(aug.TRANSFORMS)
    aug.check_recipes(aug.Augmenter(p=1.0, seed=1).draw(50))                         # (no new kind among them)
    a = aug.Augmenter(p=1.0, seed=4, transforms=aug.ALL_TRANSFORMS, rooms=5)
    assert a.needs_bank and a.bank.dtype == np.float32 and len(a.offsets) == 5 and len(a.rooms) == 5
    assert all(1 <= n <= 8192 for n in a.lengths) and a.bank.size == int(a.lengths.sum())
    for i, room in enumerate(a.rooms):
        assert 3.6 <= room["size"][0] <= 5.6 and 3.6 <= room["size"][1] <= 3.9 and 2.4 <= room["size"][2] <= 3.0 and 0.075 <= room["absorption"] <= 0.4
        for pos in (room["source"], room["microphone"]):
            assert all(0.3 <= v <= s - 0.3 for v, s in zip(pos, room["size"]))
        assert a.bank[a.offsets[i]] >= 1.0                                           # the direct sound
    rec = a.draw(400)
    aug.check_recipes(rec, bank_len=a.bank.size)
    order = {t: i for i, t in enumerate(aug.ALL_TRANSFORMS)}
    seen = set()
    for row, r in zip(a.last_params, rec):
        names = [name for name, _ in row]
        assert 1 <= len(names) <= 3 and len(set(names)) == len(names) and names == sorted(names, key=order.get)
        seen |= set(names)
        for (name, prm), op in zip(row, r["ops"]):
            if name == "room":
                assert op["kind"] == aug.FIR and 0 <= op["seed"] and op["seed"] + op["n_sections"] <= a.bank.size
                assert (int(op["seed"]), int(op["n_sections"])) == (int(a.offsets[prm["response"]]), int(a.lengths[prm["response"]]))
            elif name == "aliasing":
                assert op["kind"] == aug.ALIAS and op["b"] == 16000 and 8000 <= op["a"] <= 16000 and op["a"] == int(op["a"])
            else:
                assert op["kind"] in (aug.NOISE, aug.BIQUADS, aug.CLIP)
    assert seen == set(aug.ALL_TRANSFORMS)
    b = aug.Augmenter(p=1.0, seed=4, transforms=aug.ALL_TRANSFORMS, rooms=5)
    assert np.array_equal(b.draw(400).view(np.uint8), rec.view(np.uint8)) and np.array_equal(bits(b.bank), bits(a.bank))
    # measured responses instead of rooms, cut to 8192 taps; an aliasing range of the caller's
    m = aug.Augmenter(p=1.0, seed=0, transforms=["room", "aliasing"], rirs=[np.ones(3), np.ones(9000)], aliasing_rate=(4000, 5000))
    assert list(m.lengths) == [3, 8192] and m.bank.size == 8195
    rec = m.draw(50)
    aug.check_recipes(rec, bank_len=8195)
    rates = [prm["rate"] for row in m.last_params for name, prm in row if name == "aliasing"]
    assert rates and all(4000 <= r <= 5000 for r in rates)
    with pytest.raises(ValueError):
        aug.Augmenter(transforms=["reverb"])
    with pytest.raises(ValueError):
        aug.Augmenter(transforms=["room"], rirs=[[1.0, np.nan]])
    # the recipes run on the twin
    x = batch_of([3000] * 8)
    out = aug.augment_host(x, [3000] * 8, a.draw(8), bank=a.bank)
    assert np.all(np.isfinite(out))


def test_the_new_names_are_exported(built):
    import silero_vad_amd as pkg
    for name in ("ALL_TRANSFORMS", "fir_bank", "rir_shoebox", "augment_scratch_bytes", "Augmenter", "augment_host", "augment_device", "check_recipes"):
        assert hasattr(pkg, name), name
    for name in ("FIR", "ALIAS", "MAX_TAPS"):
        assert hasattr(pkg.augment, name), name
    assert pkg.augment.MAX_TAPS == 8192 and (pkg.augment.FIR, pkg.augment.ALIAS) == (4, 5)
    for sym in ("vad_augment_scratch_bytes", "vad_augment_check_recipes_bank", "vad_augment_rows_device_x", "vad_augment_rows_host_x", "vad_rir_shoebox"):
        assert getattr(pkg._lib.lib(), sym) is not None, sym
    assert ctypes.sizeof(pkg.augment._Extra) == 32
