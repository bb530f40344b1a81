"""The pump's fp32 tape without a GPU: the new entry points (vad_pump_set_tape_f32 / vad_pump_fetch_audio_f32 / vad_pump_tape_format)
refuse a NULL pump, and StreamPump(tape_dtype=...) / UtteranceCollector check their arguments before any native call."""
import numpy as np
import pytest


def test_fp32_tape_entry_points_refuse_a_null_pump(built):
    from silero_vad_amd import _lib
    L = _lib.lib()
    assert L.vad_pump_set_tape_f32(None, 4) == 1                 # VAD_ERR_ARG
    assert L.vad_pump_fetch_audio_f32(None, None, None, None, 0, None, None, 0) == 1
    assert L.vad_pump_fetch_audio_f32(None, None, None, None, 0, None, None, 1) == 1
    assert L.vad_pump_tape_format(None) == -1                    # -VAD_ERR_ARG


class _NoEngine:
    """An engine whose library must not be reached: the argument checks come first."""

    @property
    def _L(self):
        raise AssertionError("a native call was made before the arguments were checked")


@pytest.mark.parametrize("bad", ["int32", "float64", np.float16, "uint16", "bogus", None, 4, 2.0, object, np.dtype([("a", np.int16)])])
@pytest.mark.parametrize("chunks", [0, 8])
def test_stream_pump_checks_tape_dtype_before_any_native_call(built, bad, chunks):
    """Also with tape_chunks == 0, where the dtype is only validated."""
    from silero_vad_amd import StreamPump
    with pytest.raises(ValueError, match="tape_dtype"):
        StreamPump(_NoEngine(), 16000, streams=4, tape_chunks=chunks, tape_dtype=bad)


@pytest.mark.parametrize("good", ["int16", "float32", np.int16, np.float32, np.dtype("float32"), "<f4", "i2", "single"])
def test_a_good_tape_dtype_passes_the_argument_checks(built, good):
    """... and the next thing the constructor does is reach for the engine's library."""
    from silero_vad_amd import StreamPump
    with pytest.raises(AssertionError, match="native call"):
        StreamPump(_NoEngine(), 16000, streams=4, tape_chunks=8, tape_dtype=good)
    with pytest.raises(ValueError, match="tape_chunks"):          # (the chunk count is still checked, and first)
        StreamPump(_NoEngine(), 16000, streams=4, tape_chunks=1, tape_dtype=good)


def test_utterance_collector_still_needs_a_taped_pump(built):
    from silero_vad_amd import UtteranceCollector

    class Untaped:
        tape_chunks = 0
        tape_dtype = None

    with pytest.raises(ValueError, match="tape"):
        UtteranceCollector(Untaped())
