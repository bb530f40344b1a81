#!/usr/bin/env python3
"""Record what the reference's OWN callers do with the drop-in model object -> tests/golden/golden_callers.json.

    python tests/golden/make_caller_golden.py <reference checkout>      (after `python __graft_entry__.py`)

The reference's unmodified src/silero_vad/utils_vad.py (get_speech_timestamps, VADIterator, the Python segment scan) is imported
from the checkout (the absent ``torchaudio`` is stubbed, as in make_golden.py) and run over a `HipSileroVAD` whose engine is the CPU
replay engine (tests/replay_engine.py).  A recording wrapper logs every call the caller makes on the model -- reset_states(), and
model(x, sr) with the sample range of the fixture x is a view of -- and what the model returned.  Stored per protocol: that call
transcript, the probabilities and the caller's return value; and, for the scanner fuzz of tests/test_reference_callers.py, the
reference scan's result for each of its seeded cases.  tests/test_reference_callers.py replays all of it without the checkout."""
import json
import sys
import types
import warnings
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

from conftest import SRS                               # noqa: E402
from test_reference_callers import fuzz_cases          # noqa: E402


class Recorder:
    """Forwards reset_states() / __call__ to the model and logs them (the caller sees the model's own return values)."""

    def __init__(self, model, wav):
        self.model, self.wav, self.log, self.probs = model, wav, [], []

    def reset_states(self):
        self.log.append(["reset"])
        self.model.reset_states()

    def __call__(self, x, sr):
        start, n = x.storage_offset(), x.shape[-1]
        assert x.dim() == 1 and x.untyped_storage().data_ptr() == self.wav.untyped_storage().data_ptr()
        assert torch.equal(x, self.wav[start:start + n])
        self.log.append(["call", int(start), int(n), int(sr)])
        out = self.model(x, sr)
        self.probs.append(float(out.item()))
        return out


def main(ref_checkout):
    src = Path(ref_checkout).resolve() / "src"
    if "torchaudio" not in sys.modules:
        stub = types.ModuleType("torchaudio")
        stub.__version__ = "2.8.0"
        sys.modules["torchaudio"] = stub
    sys.path.insert(0, str(src))
    import silero_vad.utils_vad as uv
    sys.path.remove(str(src))
    assert Path(uv.__file__).resolve().is_relative_to(src)

    import __graft_entry__ as ge
    ge.build()
    from oracle import Oracle
    from replay_engine import ReplayEngine
    from silero_vad_amd.engine import HipSileroVAD
    oracle = Oracle()
    wavs = {tag: np.load(HERE / f"audio_{tag}.npz")["pcm"].astype(np.float32) / 32768.0 for tag in SRS}   # (conftest.py's golden[tag]["wav"])

    def model():
        return HipSileroVAD(engine=ReplayEngine(oracle))

    out = {"get_speech_timestamps": {}, "vad_iterator": {}}
    for tag, sr in SRS.items():
        n = 512 if sr == 16000 else 256
        wav = torch.from_numpy(wavs[tag])
        # (1) get_speech_timestamps over the first 400 chunks, default arguments and one variant
        rec = Recorder(model(), wav)
        n_use = 400 * n
        default = uv.get_speech_timestamps(wav[:n_use], rec, sampling_rate=sr)
        first = {"calls": rec.log, "probs": rec.probs, "out": default}
        rec = Recorder(model(), wav)
        variant = uv.get_speech_timestamps(wav[:n_use], rec, sampling_rate=sr, threshold=0.3, return_seconds=True, time_resolution=3)
        out["get_speech_timestamps"][tag] = {"n_use": n_use, "default": first,
                                             "variant": {"kwargs": {"threshold": 0.3, "return_seconds": True, "time_resolution": 3},
                                                         "calls": rec.log, "probs": rec.probs, "out": variant}}
        # (2) VADIterator over the first 500 chunks, then its reset_states()
        rec = Recorder(model(), wav)
        it = uv.VADIterator(rec, sampling_rate=sr)
        events = []
        for s in range(0, 500 * n, n):
            ev = it(wav[s:s + n])
            if ev:
                events.append([len(rec.probs) - 1, ev])
        it.reset_states()
        out["vad_iterator"][tag] = {"calls": rec.log, "probs": rec.probs, "events": events}
    # (3) the reference's caller with non-default arguments, for the comparison with silero_vad_amd.get_speech_timestamps
    kw = {"min_silence_duration_ms": 300, "speech_pad_ms": 100}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        agree = uv.get_speech_timestamps(torch.from_numpy(wavs["16k"][:300 * 512]), model(), sampling_rate=16000, **kw)
    out["caller_agree"] = {"sr": 16000, "n_use": 300 * 512, "kwargs": kw, "out": agree}
    # (4) the reference's Python scan over replayed probabilities (utils_vad.py:338-450), every fuzz case
    fuzz = []
    for sr, probs, audio_len, kw in fuzz_cases():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fuzz.append(uv.get_speech_timestamps(torch.zeros(audio_len), _Replay(probs), sampling_rate=sr, **kw))
    out["scanner_fuzz"] = fuzz
    (HERE / "golden_callers.json").write_text(json.dumps(out, separators=(",", ":")) + "\n")


class _Replay:
    """Model object that replays given probabilities (protocol: utils_vad.py:57-92)."""

    def __init__(self, probs):
        self.probs, self.i = [float(p) for p in probs], 0

    def reset_states(self):
        self.i = 0

    def __call__(self, x, sr):
        p = self.probs[self.i]
        self.i += 1
        return torch.tensor([[p]], dtype=torch.float32)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
