"""Decoder fine-tuning without a GPU: the host twin of the gradient call (vad_decoder_grad_host, csrc/trainer.cpp; the rule is
csrc/trainer.hpp) against the float64 gradients and the reference's own fp32 gradients recorded by tests/golden/make_tuning_golden.py
from the real reference's train(); a finite-difference check of the twin's loss; the rule's properties; the container that carries a
tuned decoder back into the engine and the oracle.

The 128 x 512 matrices are recorded at the 2048 coordinates `idx`; distances are over the recorded coordinates (the maker's docstring).
"""
import ctypes
import functools
import json

import numpy as np
import pytest

from conftest import GOLD

H, G = 128, 512
NAMES = ("rnn.weight_ih", "rnn.weight_hh", "rnn.bias_ih", "rnn.bias_hh", "decoder.2.weight", "decoder.2.bias")
SHAPES = ((G, H), (G, H), (G,), (G,), (1, H, 1), (1,))


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLD / "golden_tuning.npz")), json.loads((GOLD / "golden_tuning.json").read_text())


def published(sr=16000):
    from silero_vad_amd import decoder_state_dict
    return {k: v.astype(np.float64) for k, v in decoder_state_dict(None, sr).items()}


def recorded(grads):
    """the fixture's coordinates of six tensors"""
    idx = fixture()[0]["idx"]
    return {n: np.asarray(grads[n]).reshape(-1)[idx] if k < 2 else np.asarray(grads[n]).reshape(-1) for k, n in enumerate(NAMES)}


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def batch_of(name, k):
    """(feat, n_chunks, labels) of batch k of an e2e set"""
    z, meta = fixture()
    chunks = meta["datasets"][name]["chunks"]
    bs = meta["datasets"][name]["batch_size"]
    return z[f"{name}_feat{k}"], np.asarray(chunks[k * bs:(k + 1) * bs], dtype=np.int64), z[f"{name}_labels{k}"]


def grad_cases():
    """(set, params, feat, n_chunks, labels, keep, keep_scale): the first step of every recorded set"""
    z, meta = fixture()
    for tag, sr in (("e2e_16k", 16000), ("e2e_8k", 8000)):
        yield (tag, published(sr)) + batch_of(tag, 0) + (None, 1.0)
    d = meta["datasets"]["drop_16k"]
    keep = np.unpackbits(z["drop_16k_keep"])[:3 * 12 * H].reshape(3, 12, H)
    yield ("drop_16k", published()) + batch_of("e2e_16k", 0) + (keep, d["keep_scale"])
    p = published()
    s = np.float32(meta["datasets"]["saturated"]["head_scale"])
    p["decoder.2.weight"] = (p["decoder.2.weight"].astype(np.float32) * s).astype(np.float64)
    p["decoder.2.bias"] = (p["decoder.2.bias"].astype(np.float32) * s).astype(np.float64)
    feat, nck, _ = batch_of("e2e_16k", 0)
    yield ("saturated", p, feat, nck, z["saturated_labels"], None, 1.0)


@pytest.mark.parametrize("case", list(grad_cases()), ids=lambda c: c[0])
def test_host_twin_against_recorded_gradients(built, case):
    from silero_vad_amd import decoder_grad_host
    z, meta = fixture()
    name, params, feat, nck, lab, keep, scale = case
    loss, grads, _ = decoder_grad_host(params, feat, nck, lab, keep=keep, keep_scale=scale, noise_loss=0.5)
    got = recorded(grads)
    dist = meta["datasets"][name]["ref_fp32_distance"]
    want_loss = float(z[f"{name}_loss64"][0])
    print(name, "loss", loss, want_loss)
    assert abs(loss - want_loss) <= 1e-9 * abs(want_loss)
    assert abs(loss - float(z[f"{name}_loss32"][0])) <= (dist["loss"][0] + 1e-9) * abs(want_loss)
    for n in NAMES:
        w64, w32 = z[f"{name}_grad64_{n}"], z[f"{name}_grad32_{n}"]
        err = float(np.abs(got[n] - w64).max())
        print(name, n, "max |twin - float64|", err, "of", float(np.abs(w64).max()), "twin to the reference's fp32", rel(w32, got[n]))
        assert err <= 1e-9 * np.abs(w64).max()
        # the triangle inequality: |fp32 - twin| <= |fp32 - float64| + |float64 - twin|
        assert np.linalg.norm(w32.astype(np.float64) - got[n]) <= (dist["grad"][n] + 1e-9) * np.linalg.norm(w64)


@pytest.mark.parametrize("name", ["e2e_16k", "e2e_8k"])
def test_host_twin_follows_the_recorded_trajectory(built, name):
    """SGD in float64 with the twin's gradients over the four recorded batches: every loss and the final parameters"""
    from silero_vad_amd import decoder_grad_host
    z, meta = fixture()
    d = meta["datasets"][name]
    params = published(d["sampling_rate"])
    for s in range(d["steps"]):
        feat, nck, lab = batch_of(name, s % 2)
        loss, grads, _ = decoder_grad_host(params, feat, nck, lab)
        want = float(z[f"{name}_loss64"][s])
        assert abs(loss - want) <= 1e-9 * abs(want), (s, loss, want)
        params = {n: params[n] - d["lr"] * grads[n] for n in NAMES}
    got = recorded(params)
    for n in NAMES:
        w64 = z[f"{name}_final64_{n}"]
        assert np.abs(got[n] - w64).max() <= 1e-9 * np.abs(w64).max()
        assert np.linalg.norm(z[f"{name}_final32_{n}"].astype(np.float64) - got[n]) <= (d["ref_fp32_distance"]["final"][n] + 1e-9) * np.linalg.norm(w64)


def test_saturated_chunks_hand_back_nothing(built):
    """A batch whose only labelled chunks have fp32 p == 1 has exactly zero gradients, right or wrong labels alike (torch: p (1 - p) is 0);
    the chunks at p of 1e-9 hand back their full share."""
    from silero_vad_amd import decoder_grad_host
    z, _ = fixture()
    case = [c for c in grad_cases() if c[0] == "saturated"][0]
    _, params, feat, nck, lab, _, _ = case
    _, _, probs = decoder_grad_host(params, feat, nck, lab)
    ones = (probs == 1.0) & (lab <= 1)
    assert ones.sum() >= 2 and np.array_equal(ones, (z["saturated_probs32"] == 1.0) & (lab <= 1))       # torch's fp32 sigmoid agrees on which
    only = np.where(ones, lab, 255).astype(np.uint8)
    loss, grads, _ = decoder_grad_host(params, feat, nck, only)
    assert loss > 0 and all(not np.any(grads[n]) for n in NAMES)
    rest = np.where(~ones, lab, 255).astype(np.uint8)
    _, g_rest, _ = decoder_grad_host(params, feat, nck, rest)
    _, g_all, _ = decoder_grad_host(params, feat, nck, lab)
    assert all(np.array_equal(g_rest[n], g_all[n]) for n in NAMES) and np.any(g_all["rnn.weight_hh"])


def random_problem(rng, B=3, T=5, scale=0.3):
    params = {n: rng.standard_normal(s) * scale for n, s in zip(NAMES, SHAPES)}
    feat = np.abs(rng.standard_normal((B, T, H))).astype(np.float32)
    nck = np.asarray([T, 2, T - 1][:B], dtype=np.int64)
    lab = rng.integers(0, 2, size=(B, T)).astype(np.uint8)
    keep = (rng.random((B, T, H)) >= 0.1).astype(np.uint8)
    return params, feat, nck, lab, keep


def test_finite_differences(built):
    """12 random coordinates per tensor, B = 3, T = 5, denom = 1, central differences at h and h / 2 extrapolated (error O(h^4)).  The
    twin's loss is not smooth below 2^-24: p is rounded to float32, which moves a chunk's term by at most 2^-24 (1 + p / (1 - p)); with
    |logit| < 8 here that is at most 2^-24 * 3000 per chunk in the worst case and 2^-23 typically.  The tolerance is the sum of that
    over the 11 live chunks at the typical size, doubled, over the smallest step (4 values enter each quotient): 11 * 2^-23 * 2 * 4 /
    h, plus 1e-4 of the tensor's largest gradient for the truncation."""
    from silero_vad_amd import decoder_grad_host
    rng = np.random.default_rng(5)
    params, feat, nck, lab, keep = random_problem(rng)
    kw = dict(keep=keep, keep_scale=1.0 / 0.9, noise_loss=0.5, denom=1.0)
    _, grads, probs = decoder_grad_host(params, feat, nck, lab, **kw)
    live = np.arange(5)[None, :] < nck[:, None]
    assert 3e-4 < probs[live].min() and probs[live].max() < 1 - 3e-4
    h = 1e-2
    tol_noise = 11 * 2.0 ** -23 * 2 * 4 / (h / 2)

    def loss_at(name, at, delta):
        p = {n: v.copy() for n, v in params.items()}
        p[name].reshape(-1)[at] += delta
        return decoder_grad_host(p, feat, nck, lab, **kw)[0]

    for name in NAMES:
        flat = grads[name].reshape(-1)
        for at in rng.choice(flat.size, size=min(12, flat.size), replace=False):
            d1 = (loss_at(name, at, h) - loss_at(name, at, -h)) / (2 * h)
            d2 = (loss_at(name, at, h / 2) - loss_at(name, at, -h / 2)) / h
            fd = (4 * d2 - d1) / 3
            assert abs(fd - flat[at]) <= tol_noise + 1e-4 * np.abs(flat).max(), (name, at, fd, flat[at])


def test_ignored_chunks_change_nothing(built):
    from silero_vad_amd import decoder_grad_host
    rng = np.random.default_rng(6)
    params, feat, nck, lab, keep = random_problem(rng, B=3, T=5)
    nck[1] = 0
    base = decoder_grad_host(params, feat, nck, lab, keep=keep, keep_scale=1.25)
    # what lies behind n_chunks: NaN features, other labels, another mask
    feat2, lab2, keep2 = feat.copy(), lab.copy(), keep.copy()
    for b in range(3):
        feat2[b, nck[b]:] = np.nan
        lab2[b, nck[b]:] ^= 1
        keep2[b, nck[b]:] ^= 1
    other = decoder_grad_host(params, feat2, nck, lab2, keep=keep2, keep_scale=1.25)
    assert base[0] == other[0] and all(np.array_equal(base[1][n], other[1][n]) for n in NAMES)
    # a row without chunks contributes nothing: the batch without it, at the same denominator
    rows = [0, 2]
    less = decoder_grad_host(params, feat[rows], nck[rows], lab[rows], keep=keep[rows], keep_scale=1.25, denom=15.0)
    assert base[0] == less[0] and all(np.array_equal(base[1][n], less[1][n]) for n in NAMES)
    # label 255 = weight 0: the loss loses the chunk's term and the gradient its share, as with noise_loss = 0 on a label-0 chunk
    lab3 = lab.copy()
    lab3[0, 1], lab3[2, 3] = 0, 0
    lab4 = lab3.copy()
    lab4[0, 1], lab4[2, 3] = 255, 7
    a = decoder_grad_host(params, feat, nck, np.where(lab3 == 1, 255, lab3).astype(np.uint8), noise_loss=0.0)
    assert a[0] == 0.0 and all(not np.any(a[1][n]) for n in NAMES)
    only_pos = decoder_grad_host(params, feat, nck, lab3, noise_loss=0.0)
    masked = decoder_grad_host(params, feat, nck, np.where(lab3 == 0, 255, lab3).astype(np.uint8), noise_loss=0.5)
    assert only_pos[0] == masked[0] and all(np.array_equal(only_pos[1][n], masked[1][n]) for n in NAMES)
    assert decoder_grad_host(params, feat, nck, lab4)[0] < decoder_grad_host(params, feat, nck, lab3)[0]


def test_result_does_not_depend_on_threads(built):
    from silero_vad_amd import decoder_grad_host
    params, feat, nck, lab, keep = random_problem(np.random.default_rng(7), B=3, T=5)
    a = decoder_grad_host(params, feat, nck, lab, threads=1)
    b = decoder_grad_host(params, feat, nck, lab, threads=7)
    assert a[0] == b[0] and all(np.array_equal(a[1][n], b[1][n]) for n in NAMES) and np.array_equal(a[2], b[2])


def test_host_argument_errors(built):
    from silero_vad_amd import _lib, decoder_grad_host
    from silero_vad_amd.tuning import _Params
    L = _lib.lib()
    params, feat, nck, lab, _ = random_problem(np.random.default_rng(8), B=2, T=3)
    for bad in ([4, 1], [-1, 1]):
        with pytest.raises(_lib.VadError) as e:
            decoder_grad_host(params, feat, np.asarray(bad), lab)
        assert e.value.status == 1
    for denom in (0.0, -1.0, float("nan")):
        with pytest.raises(_lib.VadError):
            decoder_grad_host(params, feat, nck, lab, denom=denom)
    with pytest.raises(ValueError):
        decoder_grad_host(params, feat[:, :, :64], nck, lab)
    with pytest.raises(ValueError):
        decoder_grad_host({**params, "rnn.bias_ih": np.zeros(3)}, feat, nck, lab)
    # the C call itself: NULL pointers, empty shapes, a label pitch below T, a misaligned tensor
    p64 = {n: np.ascontiguousarray(v, dtype=np.float64) for n, v in params.items()}
    g64 = {n: np.zeros_like(v) for n, v in p64.items()}
    cp, cg = _Params(*[p64[n].ctypes.data for n in NAMES]), _Params(*[g64[n].ctypes.data for n in NAMES])
    loss, probs = ctypes.c_double(), np.zeros((2, 3), np.float32)

    def call(p=cp, f=feat.ctypes.data, B=2, T=3, n=nck.ctypes.data, l=lab.ctypes.data, ldl=3, g=cg, out=ctypes.byref(loss)):
        return L.vad_decoder_grad_host(ctypes.byref(p) if p else None, f, B, T, n, l, ldl, None, 1.0, 0.5, 6.0, ctypes.byref(g) if g else None, out,
                                       probs.ctypes.data, 1)

    assert call() == 0
    assert call(p=None) == 1 and call(f=None) == 1 and call(n=None) == 1 and call(l=None) == 1 and call(g=None) == 1 and call(out=None) == 1
    assert call(B=0) == 1 and call(T=0) == 1 and call(ldl=2) == 1
    assert call(p=_Params(p64[NAMES[0]].ctypes.data + 4, *[p64[n].ctypes.data for n in NAMES[1:]])) == 1
    assert call(g=_Params(*[g64[n].ctypes.data for n in NAMES[:5]], None)) == 1


def test_workspace_formula(built):
    from silero_vad_amd import decoder_grad_workspace_bytes
    assert decoder_grad_workspace_bytes(0, 5) == 0 and decoder_grad_workspace_bytes(5, 0) == 0
    for B, T in ((1, 1), (19, 37), (128, 250)):
        n = B * T
        got = decoder_grad_workspace_bytes(B, T)
        assert n * (512 * 2 + 7 * 128) * 4 <= got <= n * (512 * 2 + 7 * 128 + 2) * 4 + 8 * B + 35 * 2 ** 20


# ---- the way back in: containers ------------------------------------------------------------------------------------------------------
def tuned_state(rng, sr=16000):
    from silero_vad_amd import decoder_state_dict
    sd = decoder_state_dict(None, sr)
    return {n: (v + 0.05 * rng.standard_normal(v.shape)).astype(np.float32) for n, v in sd.items()}


def test_state_dict_names_and_shapes(built):
    from silero_vad_amd import DECODER_NAMES, decoder_state_dict
    assert tuple(DECODER_NAMES) == NAMES
    for sr in (16000, 8000):
        sd = decoder_state_dict(None, sr)
        assert list(sd) == list(NAMES) and [v.shape for v in sd.values()] == list(SHAPES) and all(v.dtype == np.float32 for v in sd.values())


def test_tuned_container(built, tmp_path, golden):
    from oracle import Oracle
    from oracle.weights import read_container
    from silero_vad_amd import _lib, replace_decoder
    base = open(_lib.WEIGHTS_PATH, "rb").read()
    sd = tuned_state(np.random.default_rng(9))
    blob = replace_decoder(base, sd, 16000)
    assert len(blob) == len(base) and blob[:80] == base[:80]                     # magic, count, the sha field
    a, b = read_container(base), read_container(blob)
    assert list(a) == list(b)
    for name in a:
        if name.startswith("_model.decoder."):
            assert np.array_equal(b[name], sd[name[len("_model.decoder."):]].reshape(b[name].shape)) and not np.array_equal(a[name], b[name])
        else:
            assert a[name].tobytes() == b[name].tobytes(), name              # the encoders and the 8 kHz decoder
    changed = np.flatnonzero(np.frombuffer(base, np.uint8) != np.frombuffer(blob, np.uint8))
    spans = [(a[n].ctypes.data, a[n].nbytes) for n in a if n.startswith("_model.decoder.")]
    origin = np.frombuffer(base, np.uint8).ctypes.data
    assert len(changed) and all(any(s - origin <= c < s - origin + m for s, m in spans) for c in changed[[0, -1]])
    h = ctypes.c_void_p()
    assert _lib.lib().vad_create_host_only(blob, len(blob), ctypes.byref(h)) == 0
    _lib.lib().vad_destroy(h)
    with pytest.raises(ValueError):
        replace_decoder(base, {**sd, "rnn.bias_hh": np.zeros(7, np.float32)}, 16000)
    path = tmp_path / "tuned.weights"
    path.write_bytes(blob)
    wav = golden["16k"]["wav"][:512 * 24]
    p0, p1 = Oracle().audio_forward(wav[None], 16000), Oracle(weights_path=str(path)).audio_forward(wav[None], 16000)
    assert np.abs(p0 - p1).max() > 1e-3
    # the 8 kHz net of the tuned container is the published one
    wav8 = golden["8k"]["wav"][:256 * 24]
    assert np.array_equal(Oracle().audio_forward(wav8[None], 8000), Oracle(weights_path=str(path)).audio_forward(wav8[None], 8000))
