"""The pump's tape without a GPU: the window rule (csrc/tape.hpp through vad_tape_window / silero_vad_amd.tape_window) against a
brute-force restatement -- the tape's held samples listed one by one and intersected with the request -- and the argument checks of
StreamPump(tape_chunks=...) that fail before any native call."""
import ctypes
import itertools

import pytest


def brute(count, floor, chunks, n, start, end):
    """The rule, sample by sample: chunk k (0 <= ... < count as far as it matters) is held iff k >= floor and k >= count - chunks; the
    answer is the held samples inside [start, end) -- they are one run -- and, where there is none, `start` confined to the window."""
    held = [k * n + i for k in range(max(floor, count - chunks), count) for i in range(n)]
    lo = max(floor, count - chunks) * n
    hi = count * n
    want = [s for s in held if start <= s < end]
    if want:
        assert want == list(range(want[0], want[0] + len(want)))
        return want[0], len(want)
    return min(max(start, lo), hi), 0


def cases():
    for chunks, n in itertools.product((2, 3, 8), (256, 512)):
        for count in (0, 1, chunks - 1, chunks, chunks + 1, 5 * chunks + 2):
            for floor in sorted({0, count - 1, count}):
                lo, hi = max(floor, count - chunks) * n, count * n
                mid = (lo + hi) // 2
                ranges = [(lo - 900, lo - 900), (mid, mid), (hi + 5, hi + 5), (lo, lo), (hi, hi),      # empty
                          (lo - 2 * n, lo - 3), (lo - 2 * n, lo),                                  # wholly before the window
                          (lo - 7, lo + 9), (lo - 1, mid), (lo - n - 1, lo + 1),                   # straddling its start
                          (lo, hi), (lo + 1, hi - 1), (mid, mid + 1), (lo + 3, mid + 5),           # inside it
                          (hi - 9, hi + 7), (mid, hi + n), (hi - 1, hi + 1),                       # straddling its end
                          (hi, hi + n), (hi + 3, hi + 2 * n),                                      # wholly after it
                          (lo - 5, hi + 5), (-2 ** 62, 2 ** 62), (-2 ** 62, mid), (mid, 2 ** 62),
                          (-2 ** 63, 2 ** 63 - 1), (2 ** 63 - 1, 2 ** 63 - 1), (-2 ** 63, -2 ** 63)]
                for a, b in ranges:
                    if a <= b:
                        yield count, floor, chunks, n, a, b


def test_tape_window_equals_the_brute_force_rule(built):
    from silero_vad_amd import tape_window
    seen = 0
    for count, floor, chunks, n, a, b in cases():
        want = brute(count, floor, chunks, n, a, b)
        got = tape_window(count, floor, chunks, n, a, b)
        assert got == want, (count, floor, chunks, n, a, b)
        lo, hi = max(floor, count - chunks) * n, count * n
        if lo <= hi:                                             # the rule as the header states it, clamp by clamp
            first = min(max(a, lo), hi)
            assert got == (first, min(max(b, first), hi) - first)
        seen += 1
    assert seen > 1500


def test_tape_window_refuses_bad_arguments(built):
    from silero_vad_amd import _lib, tape_window
    with pytest.raises(ValueError, match="behind end"):
        tape_window(4, 0, 3, 512, 10, 9)
    for bad in ((4, 0, 1, 512, 0, 1), (4, 0, 3, 0, 0, 1), (-1, 0, 3, 512, 0, 1), (2 ** 62, 0, 3, 512, 0, 1), (4, 2 ** 62, 3, 512, 0, 1)):
        with pytest.raises(ValueError):
            tape_window(*bad)
    for bad in ((4.0, 0, 3, 512, 0, 1), (4, 0, 3, 512, 0, 2 ** 63), (True, 0, 3, 512, 0, 1)):
        with pytest.raises(ValueError):
            tape_window(*bad)
    L = _lib.lib()
    first, n = ctypes.c_int64(7), ctypes.c_int64(7)
    assert L.vad_tape_window(4, 0, 3, 512, 10, 9, ctypes.byref(first), ctypes.byref(n)) == 1           # VAD_ERR_ARG, nothing written
    assert (first.value, n.value) == (7, 7)
    assert L.vad_tape_window(4, 0, 3, 512, 0, 1, None, ctypes.byref(n)) == 1
    assert L.vad_tape_window(4, 0, 3, 512, 600, 5000, ctypes.byref(first), ctypes.byref(n)) == 0
    assert (first.value, n.value) == (600, 4 * 512 - 600)


def test_tape_entry_points_refuse_a_null_pump(built):
    from silero_vad_amd import _lib
    L = _lib.lib()
    assert L.vad_pump_set_tape(None, 4) == 1
    assert L.vad_pump_tape_state(None, 0, None, None) == 1
    assert L.vad_pump_tape_window(None, None, None, None, 0, None, None) == -1
    assert L.vad_pump_fetch_audio(None, None, None, None, 0, None, None, 0) == 1


class _NoEngine:
    """An engine whose library must not be reached: the argument checks come first."""

    @property
    def _L(self):
        raise AssertionError("a native call was made before the arguments were checked")


@pytest.mark.parametrize("bad", [1, -1, -512, 2.0, "8", True, None, 2 ** 31])
def test_stream_pump_checks_tape_chunks_before_any_native_call(built, bad):
    from silero_vad_amd import StreamPump
    with pytest.raises(ValueError, match="tape_chunks"):
        StreamPump(_NoEngine(), 16000, streams=4, tape_chunks=bad)


def test_utterance_collector_needs_a_taped_pump(built):
    from silero_vad_amd import UtteranceCollector

    class Untaped:
        tape_chunks = 0

    with pytest.raises(ValueError, match="tape"):
        UtteranceCollector(Untaped())
