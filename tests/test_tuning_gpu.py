"""Decoder fine-tuning on the device: the encoder's features (vad_encode_audio) against the oracle's encoder and against the engine's own
gate pre-activations; the gradient call (vad_decoder_grad_device, csrc/kernel_train.hip) against its host twin on identical inputs;
bit reproducibility; `DecoderTrainer` end to end against the reference's recorded fp32 trajectory (tests/golden/make_tuning_golden.py)
and the way back into the engine.
Everything here needs a real MI355X:  python -m pytest tests -m gpu

Bounds.  Device against twin, per tensor, relative to the Frobenius norm: 8 x the largest ref_fp32_distance the fixture records for
that tensor (what the reference's own fp32 arithmetic is away from float64); the device's sigmoid and tanh are v_exp / v_rcp compositions
good to 1.1e-7 / 2.2e-7 absolute where torch's are good to an ulp, they enter every step twice, and the B T sums run in another order.
End to end, against the reference's fp32 values: 2 x feature_sensitivity + ref_fp32_distance, over the fixture's recorded coordinates.
The measured ratios are printed in front of every assertion (profiles/decoder_training.md holds a run's).
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import SRS
from test_gpu_parity import TIGHT, chunk_of, rolled_rows
from test_tuning import H, NAMES, batch_of, fixture, grad_cases, published, recorded

pytestmark = pytest.mark.gpu

FILL = 0x5A


@pytest.fixture(scope="module")
def model(built):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback to silently pass on)")
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    assert m.engine._h, "native engine not created"
    return m


def factor8(kind, name):
    """8 x the largest ref_fp32_distance of the fixture for a gradient tensor (kind 'grad') or the loss (kind 'loss')"""
    sets = fixture()[1]["datasets"].values()
    return 8.0 * max(max(d["ref_fp32_distance"]["loss"]) if kind == "loss" else d["ref_fp32_distance"]["grad"][name] for d in sets)


def dev_params(params, dev):
    return {n: torch.from_numpy(np.ascontiguousarray(params[n], dtype=np.float32)).to(dev) for n in NAMES}


def device_grad(model, params32, feat, nck, lab, keep=None, scale=1.0, denom=None, **kw):
    from silero_vad_amd import decoder_grad
    dev = model.device
    loss, grads, probs = decoder_grad(model.engine, dev_params(params32, dev), torch.from_numpy(feat).to(dev), nck, lab,
                                      None if keep is None else torch.from_numpy(keep).to(dev), scale, 0.5, denom, **kw)
    torch.cuda.synchronize()
    return float(loss.item()), {n: g.cpu().numpy() for n, g in grads.items()}, None if probs is None else probs.cpu().numpy()


def against_twin(model, params, feat, nck, lab, keep, scale, what):
    """the device call and the host twin on the same float32 parameters and features"""
    from silero_vad_amd import decoder_grad_host
    p32 = {n: np.asarray(params[n], dtype=np.float32) for n in NAMES}
    want_loss, want, want_p = decoder_grad_host(p32, feat, nck, lab, keep=keep, keep_scale=scale)
    loss, got, probs = device_grad(model, p32, feat, nck, lab, keep, scale)
    live = np.arange(feat.shape[1])[None, :] < np.asarray(nck)[:, None]
    assert np.all(probs[~live] == 0.0)
    if live.any():
        assert np.abs(probs[live] - want_p[live]).max() < TIGHT
    ratio = abs(loss - want_loss) / abs(want_loss) if want_loss else abs(loss)
    print(what, "loss", ratio / (factor8("loss", None) / 8), "x the recorded distance")
    assert ratio <= factor8("loss", None), (loss, want_loss)
    for n in NAMES:
        nw = float(np.linalg.norm(want[n]))
        d = float(np.linalg.norm(got[n].astype(np.float64) - want[n]))
        if nw == 0.0:
            assert d == 0.0, n
            continue
        print(what, n, d / nw / (factor8("grad", n) / 8), "x the recorded distance")
        assert d <= factor8("grad", n) * nw, (n, d / nw)
    return got, want


# ---- encode ----------------------------------------------------------------------------------------------------------------------------
def oracle_features(oracle, rows, sr):
    n, B = chunk_of(sr), rows.shape[0]
    C, T = n // 8, rows.shape[1] // n
    out = np.empty((B, T, H), np.float32)
    for t in range(T):
        prev = rows[:, t * n - C: t * n] if t else np.zeros((B, C), np.float32)
        _, _, st = oracle.step(np.concatenate([prev, rows[:, t * n:(t + 1) * n]], 1), np.zeros((2, B, H), np.float32), sr, stages=True)
        out[:, t] = st["enc3"][:, :, 0]
    return out


@pytest.mark.parametrize("dtype", ["f32", "i16"])
@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_encode_against_oracle_and_gates(model, oracle, golden, tag, dtype):
    sr, g = SRS[tag], golden[tag]
    n, B, T = chunk_of(sr), 19, 5
    if dtype == "i16":
        rows_i = rolled_rows(g["pcm_i16"], B, T * n, 5003)
        rows, x = rows_i.astype(np.float32) / 32768.0, torch.from_numpy(rows_i)
    else:
        rows = rolled_rows(g["wav"], B, T * n, 5003)
        x = torch.from_numpy(rows)
    feat = model.encode(x, sr)
    assert feat.is_cuda and tuple(feat.shape) == (B, T, H)
    got = feat.cpu().numpy()
    want = oracle_features(oracle, rows, sr)
    err = np.abs(got - want).max()
    print(tag, dtype, "max |feat - oracle enc3|", err, "of", np.abs(want).max())
    assert err < 1e-4 * max(1.0, np.abs(want).max())
    assert got.min() >= 0.0
    # the unchanged engine's gate pre-activations are W_ih feat + b in fp32: a 128-term dot product and the bias add
    p = published(sr)
    w_ih, b = p["rnn.weight_ih"], p["rnn.bias_ih"] + p["rnn.bias_hh"]
    xd = torch.from_numpy(rows).to(model.device)
    gx = model.engine.debug_frontend(xd, sr, torch.zeros((B, n // 8), device=model.device)).cpu().numpy().astype(np.float64)
    f64 = got.astype(np.float64)
    bound = 130 * 2.0 ** -24 * (f64 @ np.abs(w_ih).T + np.abs(b))
    assert np.all(np.abs(f64 @ w_ih.T + b - gx) <= bound), float((np.abs(f64 @ w_ih.T + b - gx) / bound).max())


@pytest.mark.parametrize("B", [1, 1025])
def test_encode_both_frontend_forms(model, oracle, golden, B):
    """B = 1: the latency form; B = 1025 x 12 chunks: the throughput form and its fix-up pass.  The same rows give the same bits."""
    sr, n, T = 16000, 512, 12 if B > 1 else 3
    rows = rolled_rows(golden["16k"]["wav"], min(B, 8), T * n, 4001)
    rows = rows[np.arange(B) % len(rows)]
    got = model.encode(torch.from_numpy(rows), sr).cpu().numpy()
    again = model.encode(torch.from_numpy(rows), sr).cpu().numpy()
    assert np.array_equal(got, again)
    want = oracle_features(oracle, rows[:min(B, 8)], sr)
    assert np.abs(got[:min(B, 8)] - want).max() < 1e-4 * max(1.0, np.abs(want).max())
    if B > 8:
        assert np.array_equal(got[8:16], got[:8])                  # the same audio in another tile


def test_encode_silence_then_speech_and_48k(model, oracle, golden):
    sr, n, T = 16000, 512, 6
    wav = golden["16k"]["wav"]
    rows = rolled_rows(wav, 3, T * n, 6007)
    rows[1, :3 * n] = 0.0                                          # digital silence, then speech: the exact-fix path
    rows[2, :] = 0.0
    got = model.encode(torch.from_numpy(rows), sr).cpu().numpy()
    want = oracle_features(oracle, rows, sr)
    assert np.abs(got - want).max() < 1e-4 * max(1.0, np.abs(want).max())
    # a 48 kHz row is its every third sample at 16 kHz
    wide = np.repeat(rows, 3, axis=1)
    wide[:, 1::3] += 0.25
    got48 = model.encode(torch.from_numpy(wide), 48000).cpu().numpy()
    assert np.abs(got48 - want).max() < 1e-4 * max(1.0, np.abs(want).max())
    # a non-finite sample poisons its chunk's whole vector
    bad = rows.copy()
    bad[0, 2 * n + 17] = np.nan
    nan = model.encode(torch.from_numpy(bad), sr).cpu().numpy()
    assert np.isnan(nan[0, 2]).all() and not np.isnan(nan[0, :2]).any() and not np.isnan(nan[1:]).any()


def test_encode_leaves_the_engine_alone(built, golden):
    """audio_forward on a fresh model before and after its first encode call (which builds the second image set): identical bits"""
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    for tag, sr in SRS.items():
        rows = torch.from_numpy(rolled_rows(golden[tag]["wav"], 5, 9 * chunk_of(sr), 3001))
        before = m.audio_forward(rows, sr)
        m.encode(rows, sr)
        assert torch.equal(before, m.audio_forward(rows, sr))
    with pytest.raises(Exception):
        m.encode(torch.zeros((1, 100)), 16000)                      # the front door's own rule: too short


# ---- gradients: device against the host twin -----------------------------------------------------------------------------------------------
def ragged_problem(rng, B, T, noisy):
    feat0 = fixture()[0]["e2e_16k_feat0"].reshape(-1, H)
    feat = feat0[rng.integers(0, len(feat0), size=(B, T))] * rng.uniform(0.8, 1.2, size=(B, T, H)).astype(np.float32)
    params = published()
    if noisy:
        params = {n: v + 0.02 * rng.standard_normal(v.shape) for n, v in params.items()}
    nck = rng.integers(0, T + 1, size=B).astype(np.int64)
    nck[0] = T
    if B > 1:
        nck[1] = 0
    if B > 2:
        nck[2] = 1
    lab = rng.integers(0, 2, size=(B, T)).astype(np.uint8)
    lab[rng.random((B, T)) < 0.1] = 255
    keep = (rng.random((B, T, H)) >= 0.1).astype(np.uint8)
    return params, feat.astype(np.float32), nck, lab, keep


@pytest.mark.parametrize("with_keep", [False, True], ids=["nokeep", "keep"])
@pytest.mark.parametrize("B,T", [(1, 1), (1, 37), (16, 2), (17, 5), (19, 37)])
def test_gradients_against_twin(model, B, T, with_keep):
    rng = np.random.default_rng(100 * B + T)
    for noisy in (False, True):
        params, feat, nck, lab, keep = ragged_problem(rng, B, T, noisy)
        against_twin(model, params, feat, nck, lab, keep if with_keep else None, 1.0 / 0.9 if with_keep else 1.0, f"{B}x{T} noisy={noisy}")


def test_gradients_against_twin_130x64(model):
    """more rows than CUs per XCD, several split-K slabs, a partial last GEMM tile"""
    params, feat, nck, lab, keep = ragged_problem(np.random.default_rng(13064), 130, 64, True)
    against_twin(model, params, feat, nck, lab, keep, 1.0 / 0.9, "130x64")


@pytest.mark.parametrize("case", list(grad_cases()), ids=lambda c: c[0])
def test_fixture_sets_on_device(model, case):
    """every recorded set (drop_16k with its recorded masks) against the twin; the saturated set's zeros are zeros on the device"""
    z, meta = fixture()
    name, params, feat, nck, lab, keep, scale = case
    against_twin(model, params, feat, nck, lab, keep, scale, name)
    if name == "saturated":
        p32 = {n: np.asarray(params[n], dtype=np.float32) for n in NAMES}
        _, _, probs = device_grad(model, p32, feat, nck, lab)
        ones = (probs == 1.0) & (lab <= 1)
        assert np.array_equal(ones, (z["saturated_probs32"] == 1.0) & (lab <= 1))
        loss, g, _ = device_grad(model, p32, feat, nck, np.where(ones, lab, 255).astype(np.uint8))
        assert loss > 0 and all(not np.any(g[n]) for n in NAMES)


def test_bit_reproducible(model):
    from silero_vad_amd import _lib
    params, feat, nck, lab, keep = ragged_problem(np.random.default_rng(77), 19, 37, True)
    p32 = {n: np.asarray(params[n], dtype=np.float32) for n in NAMES}
    a = device_grad(model, p32, feat, nck, lab, keep, 1.25)
    b = device_grad(model, p32, feat, nck, lab, keep, 1.25)
    side = torch.cuda.Stream(model.device)
    _lib.check(model.engine._h, _lib.lib().vad_debug_foreign_load(model.engine._h, 0, 512, 200000, side.cuda_stream))
    c = device_grad(model, p32, feat, nck, lab, keep, 1.25)
    torch.cuda.synchronize()
    for other in (b, c):
        assert a[0] == other[0] and all(np.array_equal(a[1][n], other[1][n]) for n in NAMES) and np.array_equal(a[2], other[2])
    # a row's probabilities are the same bits at another batch position
    order = np.roll(np.arange(19), 5)
    d = device_grad(model, p32, feat[order], nck[order], lab[order], keep[order], 1.25)
    assert np.array_equal(d[2], a[2][order])


# ---- the trainer -----------------------------------------------------------------------------------------------------------------------
def fixture_recordings(golden, name):
    d = fixture()[1]["datasets"][name]
    tag = "16k" if d["sampling_rate"] == 16000 else "8k"
    wav = golden[tag]["wav"]
    return [wav[a:a + m] for a, m in zip(d["starts"], d["samples"])], d


@pytest.mark.parametrize("name", ["e2e_16k", "e2e_8k"])
def test_trainer_against_reference_trajectory(model, oracle, golden, name, tmp_path):
    from oracle import Oracle
    from silero_vad_amd import DecoderTrainer
    z, _ = fixture()
    wavs, d = fixture_recordings(golden, name)
    sr, bs, dist, sens = d["sampling_rate"], d["batch_size"], d["ref_fp32_distance"], d["feature_sensitivity"]
    labels = [z[f"{name}_labels{k // bs}"][k % bs][:c] for k, c in enumerate(d["chunks"])]
    trainer = DecoderTrainer(model, sampling_rate=sr, dropout=0.0, optimizer=lambda p: torch.optim.SGD(p, lr=d["lr"]))
    first = None
    for s in range(d["steps"]):
        a = (s % 2) * bs
        loss = trainer.step(wavs[a:a + bs], labels[a:a + bs])
        want = float(z[f"{name}_loss32"][s])
        print(name, "step", s, "loss", loss, want, abs(loss - want) / want, "bound", 2 * sens["loss"][s] + dist["loss"][s])
        assert abs(loss - want) <= (2 * sens["loss"][s] + dist["loss"][s]) * want
        first = first or {n: g.cpu().numpy() for n, g in trainer.last_grads.items()}
    sd = trainer.state_dict()
    assert list(sd) == list(NAMES) and tuple(sd["decoder.2.weight"].shape) == (1, H, 1)
    for kind, got_all in (("grad", recorded(first)), ("final", recorded({n: v.numpy() for n, v in sd.items()}))):
        for n in NAMES:
            w32 = z[f"{name}_{kind}32_{n}"].astype(np.float64)
            r = float(np.linalg.norm(got_all[n] - w32) / np.linalg.norm(z[f"{name}_{kind}64_{n}"]))
            print(name, kind, n, r, "bound", 2 * sens[kind][n] + dist[kind][n])
            assert r <= 2 * sens[kind][n] + dist[kind][n]
    # the way back in: the tuned container in the engine and in the oracle
    blob = trainer.weights()
    path = tmp_path / "tuned.weights"
    path.write_bytes(blob)
    tuned = trainer.model()
    n = chunk_of(sr)
    rows = rolled_rows(golden["16k" if sr == 16000 else "8k"]["wav"], 4, 6 * n, 7001)
    got = tuned.audio_forward(torch.from_numpy(rows), sr).numpy()
    assert np.abs(got - Oracle(weights_path=str(path)).audio_forward(rows, sr)).max() < TIGHT
    assert np.abs(got - oracle.audio_forward(rows, sr)).max() > TIGHT


def test_mask_of_ones_is_no_mask(model):
    case = [c for c in grad_cases() if c[0] == "e2e_16k"][0]
    _, params, feat, nck, lab, _, _ = case
    p32 = {n: np.asarray(params[n], dtype=np.float32) for n in NAMES}
    a = device_grad(model, p32, feat, nck, lab)
    b = device_grad(model, p32, feat, nck, lab, np.ones(feat.shape, np.uint8), 1.0)
    assert a[0] == b[0] and all(np.array_equal(a[1][n], b[1][n]) for n in NAMES)


def test_default_training_lowers_validation_loss(model, golden):
    """20 default steps (Adam 5e-4, dropout 0.1, seeded) on the fixture's recordings with their unflipped labels"""
    from silero_vad_amd import DecoderTrainer, validate
    z, _ = fixture()
    wavs, d = fixture_recordings(golden, "e2e_16k")
    labels = np.split(z["e2e_16k_clean_labels"], np.cumsum(d["chunks"])[:-1])
    base_loss, _ = validate(wavs, labels, model, 16000)
    out = []
    for _ in range(2):
        t = DecoderTrainer(model, seed=3)
        losses = [t.step(wavs, labels) for _ in range(20)]
        out.append((losses, t.state_dict()))
    assert out[0][0] == out[1][0] and all(torch.equal(out[0][1][n], out[1][1][n]) for n in NAMES)
    tuned_loss, _ = validate(wavs, labels, t.model(), 16000)
    print("validate loss", base_loss, "->", tuned_loss)
    assert tuned_loss < base_loss


def test_device_argument_errors(model):
    from silero_vad_amd import _lib, decoder_grad_workspace_bytes
    from silero_vad_amd.tuning import _Params
    L, e, dev = _lib.lib(), model.engine._h, model.device
    B, T = 2, 3
    params = dev_params(published(), dev)
    grads = {n: torch.full_like(params[n], 7.0) for n in NAMES}
    feat = torch.rand((B, T, H), device=dev)
    nck = torch.tensor([3, 2], device=dev)
    lab = torch.zeros((B, T), dtype=torch.uint8, device=dev)
    loss = torch.full((), 7.0, dtype=torch.float64, device=dev)
    probs = torch.full((B, T), 7.0, device=dev)
    need = decoder_grad_workspace_bytes(B, T)
    ws = torch.full((need + 256,), FILL, dtype=torch.uint8, device=dev)
    cp, cg = _Params(*[params[n].data_ptr() for n in NAMES]), _Params(*[grads[n].data_ptr() for n in NAMES])

    def call(p=cp, f=feat.data_ptr(), B=B, T=T, ldl=T, denom=6.0, g=cg, w=ws.data_ptr(), wb=need, h=e):
        return L.vad_decoder_grad_device(h, ctypes.byref(p) if p else None, f, B, T, nck.data_ptr(), lab.data_ptr(), ldl, None, 1.0, 0.5, denom,
                                         ctypes.byref(g) if g else None, loss.data_ptr(), probs.data_ptr(), w, wb, None)

    assert call(h=None) == 1 and call(p=None) == 1 and call(g=None) == 1 and call(f=None) == 1 and call(w=None) == 1
    assert call(B=0) == 1 and call(T=0) == 1 and call(ldl=2) == 1 and call(denom=0.0) == 1 and call(denom=float("nan")) == 1
    assert call(f=feat.data_ptr() + 4) == 1 and call(w=ws.data_ptr() + 16) == 1
    assert call(wb=need - 1) == 1                                   # a short workspace: nothing is written
    assert b"workspace" in L.vad_last_error(e)
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and torch.all(probs == 7.0) and all(torch.all(grads[n] == 7.0) for n in NAMES) and torch.all(ws == FILL)
    assert call() == 0
    torch.cuda.synchronize()
    assert float(loss) != 7.0 and torch.all(ws[need:] == FILL)
    blob = open(_lib.WEIGHTS_PATH, "rb").read()
    host = ctypes.c_void_p()
    assert L.vad_create_host_only(blob, len(blob), ctypes.byref(host)) == 0
    assert call(h=host) == 4
    assert L.vad_encode_audio(host, 16000, 1, 512, feat.data_ptr(), 4, 512, feat.data_ptr(), feat.data_ptr(), None) == 4
    L.vad_destroy(host)
    assert L.vad_encode_audio(e, 16000, 0, 512, feat.data_ptr(), 4, 512, feat.data_ptr(), feat.data_ptr(), None) == 1
    assert L.vad_encode_audio(e, 16000, 1, 512, feat.data_ptr(), 3, 512, feat.data_ptr(), feat.data_ptr(), None) == 1
    assert L.vad_encode_audio(e, 44100, 1, 512, feat.data_ptr(), 4, 512, feat.data_ptr(), feat.data_ptr(), None) == 2
