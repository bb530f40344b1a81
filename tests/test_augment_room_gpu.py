"""Room reverb (FIR) and aliasing (ALIAS) on the device (vad_augment_rows_device_x, csrc/kernel_augment_x.hip) against the host twin on
identical inputs: rows of 1, 15, 16, 17, 255, 256, 257, 773 and 10 247 samples in one batch (below, at and above the 16 outputs of an
MFMA column, the 256 of an accumulator, the 1024 of a wave and the 4096 of a workgroup), int16 and float32 input, an odd width and an
input leading dimension larger than the width.
Everything here needs a real MI355X:  python -m pytest tests -m gpu

Bounds (the measured worst case is printed in front of every assertion; profiles/augment_room.md holds a run's):
  ALIAS  bit-equal: the same statements in double, compiled without contraction on both sides.
  FIR    |device - twin| <= (K + 2) 2^-24 S[n], S[n] = sum |h[k]| |x[n - k]| in double: the device runs K fused multiply-adds in
         float32, each within 2^-24 relative, the twin rounds an exact double sum once; where S[n] is 0 the device value is 0.
         K = 1 and a response that is a single 1.0 are bit-equal by construction, and pin the indexing.
         Measured on the MI355X: at most 5.53 x 2^-24 S on the responses of 2 .. 8192 taps and the mixed recipes, 13.0 on the trainer's
         drawn recipes, where K + 2 are allowed.
Recipes of several ops are compared stage by stage, by calling with prefixes of the recipe: stage k of the device against the twin's op
k on the device's own stage k - 1, so that each stage has its op's bound (test_augment_gpu.py has those of the first three kinds).
"""
import numpy as np
import pytest
import torch

from conftest import GOLD
from test_augment_gpu import bits, check_biquads, check_noise, on_device

pytestmark = pytest.mark.gpu

LENS = [1, 15, 16, 17, 255, 256, 257, 773, 10247]
W = 10247
RATES = [4000, 8000, 11025, 15999, 16000]


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
def batch():
    """nine rows of speech (int16), every row from another place of the fixture"""
    pcm = np.load(GOLD / "audio_16k.npz")["pcm"]
    x = np.zeros((len(LENS), W), np.int16)
    for i, n in enumerate(LENS):
        x[i, :n] = pcm[30000 + 9000 * i:30000 + 9000 * i + n]
    return x


def as_input(x, kind):
    return x if kind == "int16" else (x.astype(np.float32) / np.float32(32768.0))


def run(model, aug, x, lens, recipes, bank, **kw):
    out = aug.augment_device(model.engine, on_device(model, x), lens, recipes, bank=bank, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_fir(got, want, prev, h, n, what):
    """one row: the device's got[0 .. n) against the twin's want, prev the row both filtered; -> the worst error / (2^-24 S)"""
    K = len(h)
    S = np.convolve(np.abs(prev[:n].astype(np.float64)), np.abs(np.asarray(h, np.float64)))[:n]
    d = np.abs(got[:n].astype(np.float64) - want[:n].astype(np.float64))
    assert np.all(d <= (K + 2) * 2.0 ** -24 * S), (what, float((d / np.maximum((K + 2) * 2.0 ** -24 * S, 1e-300)).max()))
    assert np.all(got[n:] == 0.0), what
    return float((d[S > 0] / (2.0 ** -24 * S[S > 0])).max()) if np.any(S > 0) else 0.0


# ---- ALIAS ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int16", "float32"])
def test_alias_bit_equal(model, aug, batch, kind):
    x = as_input(batch, kind)
    plain = as_input(batch, "float32")
    for rate in RATES:
        rec = aug.make_recipes([[("alias", rate, 16000)]] * len(LENS))
        got, want = run(model, aug, x, LENS, rec, []), aug.augment_host(x, LENS, rec, bank=[])
        assert got.shape == (len(LENS), W)
        assert np.array_equal(bits(got), bits(want)), rate
        assert np.array_equal(bits(got), bits(plain)) == (rate == 16000)             # a == b is the input; anything else aliases


# ---- FIR -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int16", "float32"])
def test_fir_bit_equal_where_the_sum_is_one_term(model, aug, batch, kind):
    x = as_input(batch, kind)
    plain = as_input(batch, "float32")
    bank = np.zeros(3 + 8192, np.float32)
    bank[1] = np.float32(-0.37)
    rec = aug.make_recipes([[("fir", 1, 1)]] * len(LENS))
    got = run(model, aug, x, LENS, rec, bank)
    assert np.array_equal(bits(got), bits(aug.augment_host(x, LENS, rec, bank=bank))) and np.array_equal(bits(got), bits(plain * np.float32(-0.37) + np.float32(0.0)))     # (the sum starts at +0)
    for d in (0, 1, 15, 16, 17, 255, 8191):
        bank[:] = 0.0
        bank[3 + d] = 1.0
        rec = aug.make_recipes([[("fir", 3, d + 1)]] * len(LENS))
        got, want = run(model, aug, x, LENS, rec, bank), aug.augment_host(x, LENS, rec, bank=bank)
        assert np.array_equal(bits(got), bits(want)), d
        for i, n in enumerate(LENS):
            assert np.array_equal(got[i, d:n], plain[i, :max(n - d, 0)]) and np.all(got[i, :min(d, n)] == 0.0), (d, n)


@pytest.fixture(scope="module")
def responses(aug):
    """random responses of 2 .. 8192 taps and one shoebox room, packed so that every one starts at an odd offset"""
    rng = np.random.default_rng(21)
    hs = [(rng.standard_normal(K) * np.exp(-np.arange(K) / max(K / 5.0, 1.0))).astype(np.float32) for K in (2, 3, 5, 17, 255, 1024, 8192)]
    room = aug.rir_shoebox(16000, [4.7, 3.8, 2.6], [1.1, 2.9, 1.5], [3.2, 0.9, 1.2], 0.2, 12, 8192)
    hs.append(room[:int(np.flatnonzero(room)[-1]) + 1])
    packed = [np.zeros(1, np.float32)]
    for h in hs:
        packed += [h, np.zeros(2 - h.size % 2, np.float32)]
    bank, offs, lens = aug.fir_bank(packed)
    assert all(int(o) % 2 == 1 for o in offs[1::2])
    return bank, offs[1::2], lens[1::2]


@pytest.mark.parametrize("kind", ["int16", "float32"])
def test_fir_within_its_bound_on_speech(model, aug, batch, responses, kind):
    bank, offs, taps = responses
    pcm = np.load(GOLD / "audio_16k.npz")["pcm"]
    silent = np.zeros((1, W), np.int16)                                              # speech, 8500 samples of digital silence, speech
    silent[0, :1000], silent[0, 9500:] = pcm[50000:51000], pcm[60000:60000 + W - 9500]
    x = as_input(np.concatenate([batch, silent]), kind)
    lens = LENS + [W]
    plain = as_input(np.concatenate([batch, silent]), "float32")
    worst = 0.0
    for o, K in zip(offs, taps):
        rec = aug.make_recipes([[("fir", int(o), int(K))]] * len(lens))
        got = run(model, aug, x, lens, rec, bank)
        twin = aug.augment_host(x, lens, rec, bank=bank)
        h = bank[o:o + K]
        for i, n in enumerate(lens):
            worst = max(worst, check_fir(got[i], twin[i], plain[i], h, n, f"{kind} K {K} row {i}"))
        assert np.all(got[-1, 1000 + K - 1:9500] == 0.0) and np.any(got[-1, 9500:] != 0.0), K        # silence behind the tail stays silence
    print(f"fir {kind}: worst |device - twin| = {worst} x 2^-24 S (the bound is K + 2)")


# ---- the new ops beside the old ones --------------------------------------------------------------------------------------------------
def stage(rec, k):
    """the recipes cut to their first k ops, and the recipes that hold op k alone"""
    head, one = rec.copy(), rec.copy()
    head["n_ops"] = np.minimum(rec["n_ops"], k)
    one["n_ops"] = (rec["n_ops"] >= k).astype(np.int32)
    one["ops"][:, 0] = rec["ops"][:, k - 1]
    return head, one


def stages_against_twin(model, aug, x, lens, rec, bank, what):
    """-> the device's result of the whole recipes, each stage checked against the twin's op on the stage before"""
    empty = rec.copy()
    empty["n_ops"] = 0
    prev = run(model, aug, x, lens, empty, bank)
    assert np.array_equal(bits(prev), bits(aug.augment_host(x, lens, empty, bank=bank)))
    worst = 0.0
    for k in (1, 2, 3):
        head, one = stage(rec, k)
        got = run(model, aug, x, lens, head, bank)
        step = aug.augment_host(prev, lens, one, bank=bank)
        for i, r in enumerate(rec):
            tag = f"{what} row {i} stage {k}"
            if r["n_ops"] < k:
                assert np.array_equal(bits(got[i]), bits(prev[i])), tag
                continue
            op = r["ops"][k - 1]
            if op["kind"] in (aug.CLIP, aug.ALIAS):
                assert np.array_equal(bits(got[i]), bits(step[i])), tag
            elif op["kind"] == aug.NOISE:
                check_noise(got[i], step[i], float(op["a"]), tag)
            elif op["kind"] == aug.BIQUADS:
                check_biquads(got[i:i + 1], step[i:i + 1], tag)
            else:
                h = bank[int(op["seed"]):int(op["seed"]) + int(op["n_sections"])]
                worst = max(worst, check_fir(got[i], step[i], prev[i], h, lens[i], tag))
        prev = got
    print(f"{what}: worst fir stage {worst} x 2^-24 S")
    return prev


def mixed_rows(aug, offs, taps):
    lp = ("biquads", aug.butterworth("lowpass", 16000, 3000.0, 24))
    peak = ("biquads", aug.biquad_design("peaking", 16000, 900.0, 2.0, 9.0)[None])
    fir = [("fir", int(o), int(K)) for o, K in zip(offs, taps)]
    return [[("alias", 9000, 16000), lp, fir[4]], [fir[0]], [fir[7], ("clip", 0.02, 0.98), ("alias", 12000, 16000)], [],
            [("noise", 0.01, 3), fir[3], peak], [fir[1], fir[2], ("alias", 8000, 16000)], [("alias", 15999, 16000), ("alias", 4000, 16000)],
            [("clip", 0.1, 0.9), ("alias", 11025, 16000), fir[5]], [lp, ("noise", 0.005, 9), fir[6]]]


@pytest.mark.parametrize("kind", ["int16", "float32"])
def test_mixed_recipes_stage_by_stage(model, aug, batch, responses, kind):
    bank, offs, taps = responses
    x = as_input(batch, kind)
    rec = aug.make_recipes(mixed_rows(aug, offs, taps), row_keys=range(20, 29))
    whole = stages_against_twin(model, aug, x, LENS, rec, bank, kind)
    assert np.array_equal(bits(whole[3]), bits(as_input(batch, "float32")[3]))
    for i, n in enumerate(LENS):
        assert np.all(whole[i, n:] == 0.0)


def test_calls_repeat_and_rows_do_not_see_each_other(model, aug, batch, responses):
    bank, offs, taps = responses
    x = as_input(batch, "int16")
    rec = aug.make_recipes(mixed_rows(aug, offs, taps), row_keys=range(20, 29))
    a, b = run(model, aug, x, LENS, rec, bank), run(model, aug, x, LENS, rec, bank)
    assert np.array_equal(bits(a), bits(b))
    for i in (8, 7, 2, 0):
        solo = run(model, aug, x[i:i + 1], LENS[i:i + 1], rec[i:i + 1], bank)
        assert np.array_equal(bits(solo[0]), bits(a[i])), i
        sel = [j % 9 for j in range(16)] + [i]                                       # the row at position 16 of 17
        far = run(model, aug, x[sel], [LENS[j] for j in sel], rec[sel], bank)
        assert np.array_equal(bits(far[16]), bits(a[i])) and np.array_equal(bits(far[:9]), bits(a)), i
    # a workspace, a scratch and an output of the caller's, all dirty; the bank already on the device
    Wp = (W + 3) // 4 * 4
    out = torch.full((9, Wp), float("nan"), device=model.device)
    ws = torch.full((aug.augment_workspace_bytes(9, Wp),), 0xFF, dtype=torch.uint8, device=model.device)
    sc = torch.full((aug.augment_scratch_bytes(9, Wp),), 0xFF, dtype=torch.uint8, device=model.device)
    c = aug.augment_device(model.engine, on_device(model, x), LENS, rec, out=out, workspace=ws, bank=torch.from_numpy(bank).to(model.device), scratch=sc)
    torch.cuda.synchronize()
    assert c.data_ptr() == out.data_ptr() and np.array_equal(bits(c.cpu().numpy()), bits(a)) and bool((out[:, W:] == 0).all())


# ---- the rules -----------------------------------------------------------------------------------------------------------------------
def test_rows_that_come_back_as_their_input(model, aug, batch, responses):
    from silero_vad_amd._lib import VadError
    bank, offs, taps = responses
    x = as_input(batch, "float32").copy()
    x[8, 5000] = np.inf
    x[7, 3] = np.nan
    fir = ("fir", int(offs[4]), int(taps[4]))
    rec = aug.make_recipes([[fir]] * 9)
    got, want = run(model, aug, x, LENS, rec, bank), aug.augment_host(x, LENS, rec, bank=bank)
    for i in (7, 8):
        assert np.array_equal(bits(got[i]), bits(x[i])) and np.array_equal(bits(want[i]), bits(x[i])), i
    assert not np.array_equal(got[6], x[6]) and np.all(np.isfinite(got[:7]))
    for i in range(7):
        check_fir(got[i], want[i], x[i], bank[offs[4]:offs[4] + taps[4]], LENS[i], f"the finite row {i}")
    # a range outside the bank: refused on the host, the row's input from the device
    x = as_input(batch, "int16")
    plain = as_input(batch, "float32")
    out_of_bank = aug.make_recipes([[fir]] * 8 + [[("fir", bank.size - 3, 4)]])
    with pytest.raises(VadError, match="fir taps outside the bank"):
        run(model, aug, x, LENS, out_of_bank, bank)
    got = run(model, aug, x, LENS, torch.from_numpy(out_of_bank.view(np.uint8).copy()).to(model.device), bank)
    assert np.array_equal(bits(got[8]), bits(plain[8])) and not np.array_equal(got[5], plain[5])
    # the entry point without a bank does not know the two kinds
    for ops in ([fir], [("alias", 8000, 16000)]):
        rec = aug.make_recipes([ops] * 9)
        with pytest.raises(VadError, match="unknown op kind"):
            aug.augment_device(model.engine, on_device(model, x), LENS, rec)
        got = aug.augment_device(model.engine, on_device(model, x), LENS, torch.from_numpy(rec.view(np.uint8).copy()).to(model.device))
        torch.cuda.synchronize()
        assert np.array_equal(bits(got.cpu().numpy()), bits(plain))
    # arguments the call can see are refused with the library's text
    with pytest.raises(VadError, match="scratch smaller"):
        aug.augment_device(model.engine, on_device(model, x), LENS, aug.make_recipes([[fir]] * 9), bank=bank,
                           scratch=torch.empty(aug.augment_scratch_bytes(9, W + 1) - 256, dtype=torch.uint8, device=model.device))
    with pytest.raises(VadError, match="misaligned"):
        aug.augment_device(model.engine, on_device(model, x), LENS, aug.make_recipes([[fir]] * 9), bank=bank,
                           scratch=torch.empty(aug.augment_scratch_bytes(9, W + 1) + 16, dtype=torch.uint8, device=model.device)[4:])


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------
def test_trainer_with_the_twelve_transforms(model, aug):
    from silero_vad_amd import DecoderTrainer, TrainingSet
    from silero_vad_amd.tuning import DECODER_NAMES
    pcm = np.load(GOLD / "audio_16k.npz")["pcm"]
    rng = np.random.default_rng(3)
    audios = [pcm[40000:45000], pcm[80000:88192], pcm[120000:123000], pcm[20000:29001], pcm[100000:100700]]
    labels = [rng.integers(0, 2, (a.size + 511) // 512).astype(np.uint8) for a in audios]
    idx = [0, 1, 2, 3, 4, 1, 3, 0]
    a = aug.Augmenter(p=1.0, seed=9, transforms=aug.ALL_TRANSFORMS, rooms=6)
    rec = a.draw(len(idx), row_keys=idx)
    kinds = {int(op["kind"]) for r in rec for op in r["ops"][:r["n_ops"]]}
    assert aug.FIR in kinds and aug.ALIAS in kinds, a.last_params                    # (the seed's draw holds both new ops)
    ts = TrainingSet(audios, labels, model)
    res, host = (DecoderTrainer(model, seed=5) for _ in range(2))
    loss_r = res.step_resident(ts, idx, recipes=rec, bank=a.bank_on(model.device))
    loss_h = host.step([audios[i] for i in idx], [labels[i] for i in idx], recipes=rec, bank=a.bank)
    assert np.isfinite(loss_h) and float(loss_r.item()) == loss_h
    assert torch.equal(host.last_augmented.view(torch.int32), res.last_augmented.view(torch.int32))
    assert all(torch.equal(host.last_grads[n], res.last_grads[n]) for n in DECODER_NAMES)
    # what the trainer encoded is what the device call gives, and that agrees with the twin stage by stage
    x, nck, lab, T = host._batch([audios[i] for i in idx], [labels[i] for i in idx])
    lens = [audios[i].size for i in idx]
    whole = stages_against_twin(model, aug, x, lens, rec, a.bank, "trainer")
    assert np.array_equal(bits(res.last_augmented.cpu().numpy()), bits(whole))
    assert not np.array_equal(whole, x.astype(np.float32) / np.float32(32768.0))
    # an epoch over the resident set takes the augmenter's bank by itself
    tr = DecoderTrainer(model, seed=2)
    assert np.isfinite(tr.epoch(ts, batch_size=3, augment=aug.Augmenter(p=1.0, seed=1, transforms=aug.ALL_TRANSFORMS, rooms=3)))
    assert tr._aug_scratch is not None
