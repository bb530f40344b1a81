"""The reference's OWN, unmodified callers over the drop-in model object:

    src/silero_vad/utils_vad.py:314,328   get_speech_timestamps -> model.reset_states(), model(chunk, sr).item()
    src/silero_vad/utils_vad.py:501,528   VADIterator           -> model.reset_states(), model(x, sr).item()

were run from the reference checkout with a `HipSileroVAD` whose engine is the CPU replay engine (tests/replay_engine.py: the
oracle behind the engine's Python surface), i.e. everything of the drop-in except the kernels.  What they did is stored in
tests/golden/golden_callers.json (tests/golden/make_caller_golden.py): every call they made on the model object -- reset_states(),
model(x, sr) with the fixture samples x held -- what the model returned, and what the caller returned.  These tests replay those call
transcripts on a fresh model object (protocol, validation, state ownership, shapes and dtypes the reference code relies on), require
the same probabilities, and hold the callers' results against what the reference produced with its own model
(tests/golden/golden_segments.json) and against silero_vad_amd's own callers and native scanner on the same probabilities."""
import json
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLD, SRS

PROB_TOL = 1e-6          # the replay engine is the CPU oracle both times: the same probabilities up to the oracle's own round-off


@pytest.fixture(scope="module")
def callers():
    return json.loads((GOLD / "golden_callers.json").read_text())


def replay(model, wav, rec):
    """Make exactly the calls a reference caller made on its model object (rec["calls"]) on `model`; the model must answer
    each one the way the caller uses it (a [1, 1] float32 tensor, `.item()` a float) with the recorded probability."""
    got = []
    for c in rec["calls"]:
        if c[0] == "reset":
            model.reset_states()
            continue
        _, start, n, sr = c
        out = model(wav[start:start + n], sr)
        assert out.shape == (1, 1) and out.dtype == torch.float32
        p = out.item()
        assert isinstance(p, float)
        got.append(p)
    got = np.asarray(got, dtype=np.float32)
    assert len(got) == len(rec["probs"]) and np.abs(got - np.asarray(rec["probs"], dtype=np.float32)).max() <= PROB_TOL
    return got


@pytest.fixture()
def model(oracle):
    from replay_engine import ReplayEngine
    from silero_vad_amd.engine import HipSileroVAD
    return HipSileroVAD(engine=ReplayEngine(oracle))


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_reference_get_speech_timestamps_accepts_the_model(callers, model, golden, tag):
    from silero_vad_amd import get_speech_timestamps
    from silero_vad_amd.timestamps import segment_probs
    sr, info, rec = SRS[tag], golden["segments"][tag], callers["get_speech_timestamps"][tag]
    n_use = 400 * (512 if sr == 16000 else 256)               # 400 chunks: the per-chunk Python loop is slow
    assert rec["n_use"] == n_use
    wav = torch.from_numpy(golden[tag]["wav"])
    probs = replay(model, wav, rec["default"])
    assert rec["default"]["calls"][0] == ["reset"] and len(probs) == 400
    assert model.engine.calls["step"] == 400 and model.engine.calls["forward_audio"] == 0   # the per-chunk protocol
    # the same call through the reference's own model produced info["timestamps"]["default"] for the WHOLE file;
    # every segment that closes well inside the prefix must be identical
    got = rec["default"]["out"]
    want = [s for s in info["timestamps"]["default"]["out"] if s["end"] < n_use - 16000]
    assert len(want) >= 1 and got[:len(want)] == want
    # the reference's scan over these probabilities is the native scanner's
    assert segment_probs(probs, n_use, sr) == got
    # seconds / other kwargs take the same code path in the caller; one more variant for the argument plumbing
    v = rec["variant"]
    replay(model, wav, v)
    assert all(isinstance(s["start"], float) for s in v["out"]) and len(v["out"]) >= 1
    assert get_speech_timestamps(wav[:n_use], model, sampling_rate=sr, **v["kwargs"]) == v["out"]


@pytest.mark.parametrize("tag", ["16k", "8k"])
def test_reference_vad_iterator_accepts_the_model(callers, model, golden, tag):
    from silero_vad_amd import VADIterator
    sr, info, rec = SRS[tag], golden["segments"][tag], callers["vad_iterator"][tag]
    n = 512 if sr == 16000 else 256
    wav = torch.from_numpy(golden[tag]["wav"])
    assert [c[1] for c in rec["calls"] if c[0] == "call"] == list(range(0, 500 * n, n))
    replay(model, wav, rec)
    assert rec["calls"][-1] == ["reset"] and len(model._state) == 0      # the iterator's reset_states() reached the model object
    events = [ev for _, ev in rec["events"]]
    want = info["iterator"]["default"]["events"]
    assert len(events) >= 4 and events == want[:len(events)]
    # silero_vad_amd's own iterator emits the same events at the same chunks
    it = VADIterator(model, sampling_rate=sr)
    ours = []
    for i, s in enumerate(range(0, 500 * n, n)):
        ev = it(wav[s:s + n])
        if ev:
            ours.append([i, ev])
    assert ours == rec["events"]


def test_reference_caller_and_own_caller_agree(callers, model, golden):
    """silero_vad_amd.get_speech_timestamps (one audio_forward + native scan) == the reference's caller
    (per-chunk loop + Python scan) on the same model object."""
    from silero_vad_amd import get_speech_timestamps
    rec = callers["caller_agree"]
    wav = torch.from_numpy(golden["16k"]["wav"][:rec["n_use"]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        b = get_speech_timestamps(wav, model, sampling_rate=rec["sr"], **rec["kwargs"])
    assert len(rec["out"]) >= 1 and b == rec["out"] and model.engine.calls["forward_audio"] == 1


def test_model_protocol_details_the_reference_relies_on(model):
    out = model(torch.zeros(512), 16000)
    assert out.shape == (1, 1) and out.dtype == torch.float32 and isinstance(out.item(), float)
    assert model.sample_rates == [8000, 16000]
    assert model._state.shape == (2, 1, 128) and model._context.shape == (1, 64)
    model(torch.zeros(3, 256), 8000)                             # sr / batch change: auto reset (vad_annotator.py:37-57)
    assert model._state.shape == (2, 3, 128) and model._context.shape == (3, 32)
    p = model.audio_forward(torch.zeros(2, 1000), 16000)
    assert p.shape == (2, 2) and p.device.type == "cpu"


def fuzz_cases():
    """Random-walk probabilities and random argument sets (seeded): (sr, probs, audio length, kwargs) per case."""
    rng = np.random.default_rng(2024)
    for case in range(160):
        sr = 16000 if case % 2 == 0 else 8000
        n = 512 if sr == 16000 else 256
        T = int(rng.integers(1, 400))
        walk = np.cumsum(rng.standard_normal(T) * rng.uniform(0.1, 0.8))
        probs = (1.0 / (1.0 + np.exp(-walk + rng.standard_normal()))).astype(np.float32)
        if case % 7 == 0:
            probs[rng.integers(0, T, size=T // 3)] = 0.0                      # many short drop-outs
        audio_len = T * n - int(rng.integers(0, n))
        kw = dict(threshold=float(rng.choice([0.3, 0.5, 0.7, 0.9])),
                  min_speech_duration_ms=int(rng.choice([0, 100, 250, 1000])),
                  min_silence_duration_ms=int(rng.choice([0, 32, 100, 300, 700])),
                  speech_pad_ms=int(rng.choice([0, 30, 100, 400])),
                  max_speech_duration_s=float(rng.choice([0.3, 0.6, 1.0, 2.5, float("inf")])),
                  min_silence_at_max_speech=int(rng.choice([0, 40, 98, 200])),
                  use_max_poss_sil_at_max_speech=bool(rng.integers(0, 2)))
        if rng.random() < 0.3:
            kw["neg_threshold"] = float(rng.choice([0.05, 0.2, 0.45, 0.8]))
        yield sr, probs, audio_len, kw


def test_native_scanner_equals_reference_scan_fuzz(callers, built):
    """The native segmenter (csrc/scanner.hpp: O(1) state instead of the reference's `possible_ends` list) against the
    reference's own Python scan (utils_vad.py:338-450, its results on these cases stored in golden_callers.json) on random-walk
    probabilities and random argument sets, with the emphasis on the max_speech_duration_s branches that the speech fixtures barely reach."""
    from silero_vad_amd.timestamps import segment_probs
    wants = callers["scanner_fuzz"]
    checked = with_cut = 0
    for case, (sr, probs, audio_len, kw) in enumerate(fuzz_cases()):
        want = wants[case]
        got = segment_probs(probs, audio_len, sr, **kw)
        assert got == want, (case, sr, kw, want[:3], got[:3])
        checked += 1
        with_cut += int(np.isfinite(kw["max_speech_duration_s"]) and len(want) > 1)
    assert checked == len(wants) == 160 and with_cut > 30
