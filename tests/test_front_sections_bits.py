"""The vector sections between the GEMMs of the throughput frontend (csrc/kernel_front_f43.hip: the epilogue of an encoder-0 row part
-- Nyquist rank-1 updates, bias, ReLU -- and the bias / initial-value sections of encoders 1-3) read every table vector from LDS once,
ahead of use, and run from registers (front_common.hpp tab_rows / rank1 / add_rows).  Value and order of every floating-point
operation of every accumulator are what they were, so the outputs must be the SAME BITS as the build before that change gave on the
GPU (tests/golden/front_sections_parent.npz: this project's own outputs, recorded with `python tests/test_front_sections_bits.py
record OUT.npz` while the parent commit's library was loaded) -- and, as everywhere, inside the suite's bound against the CPU oracle.
Shapes: B = 17, T = 5 (two stream tiles, the second ragged, the last workgroup with invalid tiles) and B = 16, T = 1 with a partial
last chunk; 16 kHz, 8 kHz, 32 / 48 kHz input; float and int16 PCM; real speech (tests/golden/audio_*.npz)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

GOLD = Path(__file__).resolve().parent / "golden"
FIXTURE = GOLD / "front_sections_parent.npz"
TOL = 1e-4          # relative, on the final (h, c)
TIGHT = 2e-5        # on probabilities

# (tag, input rate, net rate, chunk samples at the net rate)
RATES = {"16k": (16000, 16000, 512), "8k": (8000, 8000, 256), "32k": (32000, 16000, 512), "48k": (48000, 16000, 512)}
SHAPES = {"B17_T5": (17, 5, 0), "B16_T1_partial": (16, 1, 37)}
CASES = [(r, s, p) for r in RATES for s in SHAPES for p in ("float", "int16")]


def case_id(rate, shape, pcm):
    return f"{rate}-{shape}-{pcm}"


def make_input(wavs, rate, shape, pcm):
    """(what the engine reads [B, L at the input rate], the float signal at the net rate that stands for, ctx0, state0)"""
    sr, net, n = RATES[rate]
    B, T, cut = SHAPES[shape]
    k = sr // net
    wav = wavs["8k" if net == 8000 else "16k"]
    L = T * n - cut
    rows = np.stack([np.roll(wav, -b * 4001)[:L] for b in range(B)])
    if pcm == "int16":
        sig = (rows * 32768.0).clip(-32768, 32767).astype(np.int16)
        ref = sig.astype(np.float32) / 32768.0
    else:
        sig = ref = rows
    raw = sig
    if k > 1:                                                   # the reference decimates with x[:, ::k]
        raw = np.zeros((B, L * k - (k - 1)), sig.dtype)
        raw[:, ::k] = sig
    rng = np.random.default_rng(1000 * B + T + k)
    ctx0 = (0.1 * rng.standard_normal((B, n // 8))).astype(np.float32)
    st0 = (0.3 * rng.standard_normal((2, B, 128))).astype(np.float32)
    return raw, ref, ctx0, st0


def run_throughput(model, raw, sr, ctx0, st0):
    eng = model.engine
    ctx = torch.from_numpy(ctx0).to(model.device)
    st = torch.from_numpy(st0).to(model.device)
    eng.set_option("front", "throughput")                       # (these shapes would take the latency kernel otherwise)
    try:
        p = eng.forward_audio(torch.from_numpy(raw).to(model.device), sr, ctx, st)
        torch.cuda.synchronize()
    finally:
        eng.set_option("front", "auto")
    return p.cpu().numpy(), ctx.cpu().numpy(), st.cpu().numpy()


def load_wavs():
    return {tag: np.load(GOLD / f"audio_{tag}.npz")["pcm"].astype(np.float32) / 32768.0 for tag in ("16k", "8k")}


@pytest.fixture(scope="module")
def model(built):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback to silently pass on)")
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    assert m.engine._h, "native engine not created"
    return m


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(FIXTURE))


@pytest.mark.gpu
@pytest.mark.parametrize("rate,shape,pcm", CASES, ids=[case_id(*c) for c in CASES])
def test_same_bits_as_before_and_inside_the_oracle_bound(model, oracle, golden, recorded, rate, shape, pcm):
    from conftest import state_err
    sr, net, _ = RATES[rate]
    raw, ref, ctx0, st0 = make_input({"16k": golden["16k"]["wav"], "8k": golden["8k"]["wav"]}, rate, shape, pcm)
    p, ctx, st = run_throughput(model, raw, sr, ctx0, st0)
    want, wctx, wst = oracle.forward_audio(ref, net, ctx=ctx0, state=st0)
    ep, es = float(np.abs(p - want).max()), state_err(st, wst)
    print(f"{case_id(rate, shape, pcm)}: max|dp| {ep:.3e}  state {es:.3e}")
    assert ep < TIGHT and es < TOL, (ep, es)
    assert np.array_equal(ctx, wctx)
    cid = case_id(rate, shape, pcm)
    for name, got in (("probs", p), ("ctx", ctx), ("state", st)):
        old = recorded[f"{cid}/{name}"]
        assert old.shape == got.shape and old.dtype == got.dtype
        assert np.array_equal(old.view(np.uint32), got.view(np.uint32)), (cid, name, int((old.view(np.uint32) != got.view(np.uint32)).sum()))


def test_fixture_holds_every_case():
    """(no GPU) the recorded outputs cover exactly the cases of this file, finite and small enough to be a fixture"""
    rec = dict(np.load(FIXTURE))
    assert sorted(rec) == sorted(f"{case_id(*c)}/{n}" for c in CASES for n in ("probs", "ctx", "state"))
    for c in CASES:
        B, T, _ = SHAPES[c[1]]
        assert rec[f"{case_id(*c)}/probs"].shape == (B, T) and rec[f"{case_id(*c)}/state"].shape == (2, B, 128)
        assert all(np.isfinite(rec[f"{case_id(*c)}/{n}"]).all() for n in ("probs", "ctx", "state"))
    assert FIXTURE.stat().st_size < 400 * 1024


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "record":
    # the parent commit's outputs: run on the GPU with the parent commit's library loaded
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    from silero_vad_amd import load_silero_vad
    m, wavs, out = load_silero_vad(device=0), load_wavs(), {}
    for c in CASES:
        raw, _, ctx0, st0 = make_input(wavs, *c)
        p, ctx, st = run_throughput(m, raw, RATES[c[0]][0], ctx0, st0)
        out.update({f"{case_id(*c)}/probs": p, f"{case_id(*c)}/ctx": ctx, f"{case_id(*c)}/state": st})
    np.savez_compressed(sys.argv[2], **out)
    print("recorded", len(CASES), "cases ->", sys.argv[2])
