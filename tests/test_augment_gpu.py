"""Audio augmentations on the device (vad_augment_rows_device, csrc/kernel_augment.hip) against the host twin on identical inputs, at the
smallest shapes at which the kernels can still go wrong: with S the block of the three-pass cascade as built, rows of 1, S - 1, S,
S + 1, 3 S + 5 and 40 S + 7 samples (the last makes the state scan cross forty blocks, more than the eight it requests at a time, and
the clip's workgroup go round its row more than once), an odd width, an input leading dimension larger than the width.
Everything here needs a real MI355X:  python -m pytest tests -m gpu

Bounds, per op (the measured worst case is printed in front of every assertion; profiles/augment.md holds a run's):
  BIQUADS  |device - twin| <= 2^-22 x the twin's row peak.  Both run the recursion in double; the device contracts a x + b into
           fused multiply-adds and hands the state over between blocks through M, which reorders the sums: about kappa 2^-53 with
           kappa <= 1e6 for these filters, below 1e-10 of the peak.  What remains is two independent roundings to float32, half an ulp
           each, at most at the peak's magnitude: one ulp of the peak, and a factor 2 of margin.
  CLIP     bit-equal: the order statistics are exact and the interpolation is the same double expression, compiled without contraction.
  NOISE    the generator's value within 4 float32 ulp of the twin's (only the double log / cos / sin of the two libraries differ, and
           the result is rounded to float32 once; bit-equality is counted and printed, not promised); the sum x + a g is formed in
           double from exact products, so y differs by that times a plus one rounding of y.
Three-op recipes are compared stage by stage, by calling with prefixes of the recipe: stage k of the device against the twin's op k on
the device's own stage k - 1, so that each stage has its op's bound and a difference is seen where it arises.
"""
import numpy as np
import pytest
import torch

from conftest import GOLD
from test_augment import QUANTILES, SQ, biquad_cases, ulp32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(built):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback to silently pass on)")
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    assert m.engine._h, "native engine not created"
    return m


@pytest.fixture(scope="module")
def aug(built):
    from silero_vad_amd import augment
    return augment


@pytest.fixture(scope="module")
def shapes(aug):
    S = aug.block_size()
    lens = [1, S - 1, S, S + 1, 3 * S + 5, 40 * S + 7]
    return S, lens, 40 * S + 7


@pytest.fixture(scope="module")
def batch(shapes):
    """six rows of speech (int16), every row from another place of the fixture"""
    _, lens, W = shapes
    pcm = np.load(GOLD / "audio_16k.npz")["pcm"]
    x = np.zeros((len(lens), W), np.int16)
    for i, n in enumerate(lens):
        x[i, :n] = pcm[30000 + 9000 * i:30000 + 9000 * i + n]
    return x


def as_input(batch, kind):
    return batch if kind == "int16" else (batch.astype(np.float32) / np.float32(32768.0))


def on_device(model, x, extra=9):
    """x on the device as a view of a wider buffer: ld = W + extra, the slack filled with a value that must never be read"""
    n, W = x.shape
    buf = np.full((n, W + extra), 12345 if x.dtype == np.int16 else np.float32(np.nan), x.dtype)
    buf[:, :W] = x
    return torch.from_numpy(buf).to(model.device)[:, :W]


def run(model, aug, x, lens, recipes, **kw):
    out = aug.augment_device(model.engine, on_device(model, x), lens, recipes, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_biquads(got, want, what):
    worst = 0.0
    for i in range(want.shape[0]):
        peak = float(np.abs(want[i]).max())
        d = float(np.abs(got[i].astype(np.float64) - want[i]).max())
        if peak == 0.0:
            assert d == 0.0, (what, i)
            continue
        worst = max(worst, d / (2.0 ** -22 * peak))
    print(what, "worst |device - twin| =", worst, "x the bound")
    assert worst <= 1.0, what
    return worst


def check_noise(got, want, amp, what):
    """rows of y = x + amp g: 4 ulp of g times amp, plus one rounding of y"""
    g_bound = 4.0 * np.spacing(np.float32(6.0)) * float(np.float32(amp))            # |g| < 6.66 by construction: u >= 2^-33
    bound = g_bound + ulp32(want)
    d = np.abs(got.astype(np.float64) - want)
    print(what, "noise: worst", float((d / bound).max()), "x the bound;", int((bits(got) != bits(want)).sum()), "of", got.size, "values differ")
    assert np.all(d <= bound), what


# ---- device against twin, op by op ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int16", "float32"])
def test_biquads_against_twin(model, aug, shapes, batch, kind):
    _, lens, W = shapes
    x = as_input(batch, kind)
    for name, coef in biquad_cases(aug, 16000).items():
        rec = aug.make_recipes([[("biquads", coef)]] * len(lens))
        got, want = run(model, aug, x, lens, rec), aug.augment_host(x, lens, rec)
        assert got.shape == (len(lens), W)
        for i, n in enumerate(lens):
            assert np.all(got[i, n:] == 0.0), (name, i)
        check_biquads(got, want, f"{kind} {name}")


@pytest.mark.parametrize("q", QUANTILES)
def test_clip_bit_equal(model, aug, shapes, batch, q):
    S, lens, W = shapes
    rng = np.random.default_rng(7)
    x = as_input(batch, "int16").copy()
    x[4, :lens[4]] = rng.integers(-3, 4, lens[4])                                    # many ties
    x[2, :lens[2]] = 1234                                                            # a constant row
    for data in (x, as_input(x, "float32")):
        rec = aug.make_recipes([[("clip", *q)]] * len(lens))
        got, want = run(model, aug, data, lens, rec), aug.augment_host(data, lens, rec)
        assert np.array_equal(bits(got), bits(want)), q
    if q == (0.1, 0.9):
        assert not np.array_equal(want[5], as_input(x, "float32")[5])                # (something was clipped)


def test_noise_against_twin(model, aug, shapes, batch):
    _, lens, W = shapes
    zero = np.zeros((len(lens), W), np.float32)
    amp = 2.0 ** -7
    rec = aug.make_recipes([[("noise", amp, 77 + i)] for i in range(len(lens))], row_keys=[3, 1, 4, 1, 5, 9])
    g_dev, g_twin = run(model, aug, zero, lens, rec) / np.float32(amp), aug.augment_host(zero, lens, rec) / np.float32(amp)
    d = np.abs(g_dev.astype(np.float64) - g_twin) / ulp32(g_twin)
    print("generator: worst", float(d.max()), "ulp;", int((bits(g_dev) != bits(g_twin)).sum()), "of", sum(lens), "values differ from the twin's")
    assert d.max() <= 4.0
    assert abs(float(g_twin[5, :lens[5]].std()) - 1.0) < 0.05
    x = as_input(batch, "float32")
    rec = aug.make_recipes([[("noise", 0.015, 5)]] * len(lens))
    check_noise(run(model, aug, x, lens, rec), aug.augment_host(x, lens, rec), 0.015, "speech")


def mixed_recipes(aug):
    cases = biquad_cases(aug, 16000)
    peak, eq = ("biquads", cases["peaking 50 Hz q 5 +24 dB"]), ("biquads", cases["eight sections"])
    return [[("clip", 0.0, 1.0)], [("noise", 0.01, 1), eq], [], [peak, ("clip", 0.02, 0.98), ("noise", 0.005, 2)],
            [("biquads", cases["24 dB/oct low-pass 150 Hz"]), ("biquads", cases["one section"])], [("noise", 0.015, 3), ("clip", 0.1, 0.9), peak]]


@pytest.mark.parametrize("kind", ["int16", "float32"])
def test_mixed_batch_stage_by_stage(model, aug, shapes, batch, kind):
    _, lens, W = shapes
    x = as_input(batch, kind)
    rows = mixed_recipes(aug)
    keys = [10, 11, 12, 13, 14, 15]
    prev = run(model, aug, x, lens, aug.make_recipes([[]] * len(rows), keys))
    want0 = aug.augment_host(x, lens, aug.make_recipes([[]] * len(rows), keys))
    assert np.array_equal(bits(prev), bits(want0))
    for k in (1, 2, 3):
        got = run(model, aug, x, lens, aug.make_recipes([r[:k] for r in rows], keys))
        step = aug.augment_host(prev, lens, aug.make_recipes([r[k - 1:k] for r in rows], keys))
        for i, r in enumerate(rows):
            what = f"{kind} row {i} stage {k}"
            if len(r) < k:
                assert np.array_equal(bits(got[i]), bits(prev[i])), what
            elif r[k - 1][0] == "clip":
                assert np.array_equal(bits(got[i]), bits(step[i])), what
            elif r[k - 1][0] == "noise":
                check_noise(got[i], step[i], r[k - 1][1], what)
            else:
                check_biquads(got[i:i + 1], step[i:i + 1], what)
        prev = got
    # the whole recipe in one call, in one go, is what the stages arrived at; the empty row is its input, bit for bit
    assert np.array_equal(bits(prev[2]), bits(want0[2]))
    for i, n in enumerate(lens):
        assert np.all(prev[i, n:] == 0.0)


# ---- batch independence, determinism, the rules ---------------------------------------------------------------------------------------
def test_rows_do_not_see_each_other_and_calls_repeat(model, aug, shapes, batch):
    _, lens, W = shapes
    x = as_input(batch, "int16")
    rows = mixed_recipes(aug)
    rec = aug.make_recipes(rows, [10, 11, 12, 13, 14, 15])
    a, b = run(model, aug, x, lens, rec), run(model, aug, x, lens, rec)
    assert np.array_equal(bits(a), bits(b))
    for i in (5, 3, 1):
        solo = run(model, aug, x[i:i + 1], lens[i:i + 1], rec[i:i + 1])
        assert np.array_equal(bits(solo[0]), bits(a[i])), i
        sel = [0, 4, i]
        third = run(model, aug, x[sel], [lens[j] for j in sel], rec[sel])
        assert np.array_equal(bits(third[2]), bits(a[i])), i
    # a workspace and an output of the caller's, both dirty: the same bits, the padding columns written as zero
    Wp = (W + 3) // 4 * 4
    out = torch.full((len(lens), Wp), float("nan"), device=model.device)
    ws = torch.full((aug.augment_workspace_bytes(len(lens), Wp),), 0xFF, dtype=torch.uint8, device=model.device)
    c = aug.augment_device(model.engine, on_device(model, x), lens, rec, out=out, workspace=ws)
    torch.cuda.synchronize()
    assert c.data_ptr() == out.data_ptr() and np.array_equal(bits(c.cpu().numpy()), bits(a)) and bool((out[:, W:] == 0).all())


def test_nonfinite_rows_come_back_as_their_input(model, aug, shapes, batch):
    S, lens, W = shapes
    x = as_input(batch, "float32").copy()
    x[5, 17 * S + 3] = np.inf
    x[4, 2] = np.nan
    cases = biquad_cases(aug, 16000)
    rec = aug.make_recipes([[("biquads", cases["eight sections"])]] * 4 + [[("noise", 0.01, 1)], [("noise", 0.01, 2), ("biquads", cases["one section"])]])
    got, want = run(model, aug, x, lens, rec), aug.augment_host(x, lens, rec)
    for i in (4, 5):
        assert np.array_equal(bits(got[i]), bits(x[i])) and np.array_equal(bits(want[i]), bits(x[i])), i
    check_biquads(got[:4], want[:4], "the finite rows beside them")
    assert not np.array_equal(got[3], x[3])
    # the rule reads the FINAL result: an infinite sample that the clip brings back into range is no reason to return the input
    rec = aug.make_recipes([[("clip", 0.1, 0.9)]] * len(lens))
    got, want = run(model, aug, x[[0, 1, 2, 3, 5]], lens[:4] + lens[5:], rec[:5]), aug.augment_host(x[[0, 1, 2, 3, 5]], lens[:4] + lens[5:], rec[:5])
    assert np.array_equal(bits(got), bits(want)) and np.all(np.isfinite(got[4])) and not np.array_equal(bits(got[4]), bits(x[5]))


def test_a_bad_recipe_on_the_device_gives_the_row_back(model, aug, shapes, batch):
    _, lens, W = shapes
    x = as_input(batch, "int16")
    rec = aug.make_recipes(mixed_recipes(aug))
    good = run(model, aug, x, lens, rec)
    bad = rec.copy()
    bad[1]["n_ops"] = 4
    bad[3]["ops"][0]["n_sections"] = 9
    bad[5]["ops"][1]["a"] = 2.0
    with pytest.raises(Exception, match="VAD_ERR_ARG"):
        run(model, aug, x, lens, bad)
    got = run(model, aug, x, lens, torch.from_numpy(bad.view(np.uint8).copy()).to(model.device))
    plain = aug.augment_host(x, lens, aug.make_recipes([[]] * 6))
    for i in range(6):
        assert np.array_equal(bits(got[i]), bits(plain[i] if i in (1, 3, 5) else good[i])), i
    # arguments the call can see are refused with the library's text
    from silero_vad_amd._lib import VadError
    xd = on_device(model, x)
    with pytest.raises(VadError, match="workspace smaller"):
        aug.augment_device(model.engine, xd, lens, rec, workspace=torch.empty(256, dtype=torch.uint8, device=model.device))
    with pytest.raises(ValueError):
        aug.augment_device(model.engine, xd, lens, rec, out=torch.empty((6, W), device=model.device))          # an odd row length


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------
def recordings():
    pcm = np.load(GOLD / "audio_16k.npz")["pcm"]
    rng = np.random.default_rng(3)
    audios = [pcm[40000:45000], pcm[80000:88192], pcm[120000:123000]]
    labels = [rng.integers(0, 2, (a.size + 511) // 512).astype(np.uint8) for a in audios]
    return audios, labels


def test_trainer_step_with_recipes(model, aug):
    from silero_vad_amd import DecoderTrainer, decoder_grad
    from silero_vad_amd.tuning import DECODER_NAMES, H
    audios, labels = recordings()
    rec = aug.Augmenter(p=1.0, seed=1).draw(3)
    tr = DecoderTrainer(model, seed=5)
    before = {n: tr.params[n].clone() for n in DECODER_NAMES}
    loss = tr.step(audios, labels, recipes=rec)
    assert np.isfinite(loss)
    pcm, nck, lab, T = tr._batch(audios, labels)
    want = aug.augment_device(model.engine, torch.from_numpy(pcm).to(model.device), [a.size for a in audios], rec)
    assert tuple(tr.last_augmented.shape) == pcm.shape and tr.last_augmented.is_contiguous()
    assert torch.equal(tr.last_augmented.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(want, torch.from_numpy(pcm.astype(np.float32) / np.float32(32768.0)).to(model.device))
    assert any(not torch.equal(before[n], tr.params[n]) for n in DECODER_NAMES)
    # without recipes: the path as it was -- encode the uploaded batch, the mask from the trainer's generator, the gradient call
    plain = DecoderTrainer(model, seed=5)
    got = plain.step(audios, labels)
    assert plain.last_augmented is None
    ref = DecoderTrainer(model, seed=5)
    x = torch.from_numpy(pcm).to(model.device)
    feat = model.encode(x, 16000)
    keep = (torch.rand((3, T, H), device=model.device, generator=ref.generator) >= ref.dropout).to(torch.uint8)
    by_hand, _, _ = decoder_grad(model.engine, ref.params, feat, nck, lab, keep, 1.0 / (1.0 - ref.dropout), ref.noise_loss, float(3 * T), want_probs=False)
    assert np.float64(got).tobytes() == np.float64(by_hand.item()).tobytes()
    # empty recipes change nothing either
    empty = DecoderTrainer(model, seed=5)
    assert np.float64(empty.step(audios, labels, recipes=aug.Augmenter(p=0.0).draw(3))).tobytes() == np.float64(got).tobytes()
    assert got != loss


def test_trainer_epoch_with_an_augmenter(model, aug):
    from silero_vad_amd import DecoderTrainer
    audios, labels = recordings()
    losses = []
    for _ in range(2):
        tr = DecoderTrainer(model, seed=2)
        losses.append([tr.epoch(audios, labels, batch_size=2, augment=aug.Augmenter(p=1.0, seed=1)) for _ in range(2)])
        assert tr.last_augmented is not None
    assert losses[0] == losses[1] and all(np.isfinite(l) for l in losses[0])
    # a callable still runs on the host, per recording
    seen = []
    tr = DecoderTrainer(model, seed=2)
    tr.epoch(audios, labels, batch_size=2, augment=lambda w: (seen.append(len(w)), w)[1])
    assert sorted(seen) == sorted(a.size for a in audios) and tr.last_augmented is None
