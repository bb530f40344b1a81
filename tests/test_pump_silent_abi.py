"""Silent rows of the pump (VAD_ROW_SILENT, include/silero_vad_hip.h) on a machine WITHOUT a GPU: the marker's value in the header and
in the package, the four packet entry points called with a null pump and a silent row (a status, never a crash), and the argument checks
of the write_* helpers for int rows, driven on a StreamPump whose submit_* are stubbed (no pump behind it)."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
N, CAP = 512, 4


def test_the_marker_is_minus_one(built):
    import silero_vad_amd
    text = (ROOT / "include" / "silero_vad_hip.h").read_text()
    assert re.search(r"^#define\s+VAD_ROW_SILENT\s+\(-1\)\s*$", text, re.M)
    assert silero_vad_amd.ROW_SILENT == -1
    assert silero_vad_amd.streams.ROW_SILENT == -1


def test_a_null_pump_and_a_silent_row_return_a_status(built):
    from silero_vad_amd import _lib
    L = _lib.lib()
    st, off, ln = (np.array(v, np.int32) for v in ([0], [-1], [160]))
    one = np.array([2], np.uint8)
    args = (st.ctypes.data, off.ctypes.data, ln.ctypes.data)
    assert L.vad_pump_submit_packets(None, 0, *args, 1) == 1
    assert L.vad_pump_submit_coded_packets(None, 0, *args, one.ctypes.data, 1) == 1
    assert L.vad_pump_submit_coded_packets(None, 0, *args, None, 1) == 1
    assert L.vad_pump_submit_burst(None, 0, *args, one.ctypes.data, 1) == 1
    assert L.vad_pump_submit_wide_packets(None, 0, *args, one.ctypes.data, 1) == 1


class Stub:
    """A StreamPump with no pump behind it: the slot is plain memory, submit_* record what they were handed."""

    def __init__(self):
        from silero_vad_amd import StreamPump
        self.calls = []
        p = StreamPump.__new__(StreamPump)
        p.n, p.streams = N, CAP
        p._slots = [np.full((CAP, N), 0x5A5A, np.int16)]
        p.submit_packets = lambda r, st, ln, off=None: self.calls.append(("packets", list(st), list(ln), list(off)))
        p.submit_coded_packets = lambda r, st, ln, cd, off=None: self.calls.append(("coded", list(st), list(ln), list(cd), list(off)))
        p.submit_burst = lambda r, st, ln, cd=None, off=None: self.calls.append(("burst", list(st), list(ln), list(cd), list(off)))
        self.pump = p

    def untouched(self):
        return not self.calls and (self.pump._slots[0] == 0x5A5A).all()


@pytest.mark.parametrize("bad", [True, False, 0, -3, 2.0, np.float32(160), np.bool_(True), np.int64(0)])
def test_what_is_neither_samples_nor_a_length_raises_before_anything_is_written(built, bad):
    x = np.arange(100, dtype=np.int16)
    for call in (lambda p: p.write_packets(0, [(0, x), (1, bad)]),
                 lambda p: p.write_coded_packets(0, [(0, x, "s16"), (1, bad, "ulaw")]),
                 lambda p: p.write_burst(0, [(0, x), (1, bad)]),
                 lambda p: p.write_burst(0, [(0, x, "s16"), (1, bad, "alaw")])):
        stub = Stub()
        with pytest.raises(ValueError):
            call(stub.pump)
        assert stub.untouched()


def test_the_length_limits_of_the_routes_hold_for_silent_rows(built):
    x = np.arange(100, dtype=np.int16)
    for call in (lambda p: p.write_packets(0, [(0, x), (1, N + 1)]),
                 lambda p: p.write_coded_packets(0, [(0, x, "s16"), (1, N + 1, "s16")])):
        stub = Stub()
        with pytest.raises(ValueError):
            call(stub.pump)
        assert stub.untouched()
    stub = Stub()
    stub.pump.write_packets(0, [(1, N), (0, 1)])
    stub.pump.write_coded_packets(0, [(1, N, "ulaw")])
    stub.pump.write_burst(0, [(1, 3 * N + 5), (1, np.int32(7), "alaw")])           # (a burst row may be longer than N)
    assert stub.calls == [("packets", [1, 0], [N, 1], [-1, -1]), ("coded", [1], [N], [1], [-1]),
                          ("burst", [1, 1], [3 * N + 5, 7], [0, 2], [-1, -1])]
    assert (stub.pump._slots[0] == 0x5A5A).all()                                    # silent rows write nothing


def test_a_silent_row_consumes_no_offset(built):
    x, y = np.arange(100, dtype=np.int16), np.arange(7, dtype=np.int16) - 3
    up = (len(x) + 7) // 8 * 8
    stub = Stub()
    stub.pump.write_packets(0, [(0, x), (1, 160), (2, y)])
    assert stub.calls == [("packets", [0, 1, 2], [100, 160, 7], [0, -1, up])]
    area = stub.pump._slots[0].reshape(-1)
    assert np.array_equal(area[:100], x) and np.array_equal(area[up:up + 7], y)
    assert (area[100:up] == 0x5A5A).all() and (area[up + 7:] == 0x5A5A).all()
    # the coded and burst helpers: byte offsets, rows rounded up to 16 bytes; a G.711 row takes 1 byte a sample
    u = np.arange(50, dtype=np.uint8)
    rows = [(0, x, "s16"), (1, 160, "alaw"), (2, u, "ulaw")]
    stub = Stub()
    stub.pump.write_coded_packets(0, rows)
    assert stub.calls == [("coded", [0, 1, 2], [100, 160, 50], [0, 2, 1], [0, -1, 208])]
    assert np.array_equal(stub.pump._slots[0].reshape(-1).view(np.uint8)[208:258], u)
    stub = Stub()
    stub.pump.write_burst(0, rows + [(3, 33), (1, y)])
    assert stub.calls == [("burst", [0, 1, 2, 3, 1], [100, 160, 50, 33, 7], [0, 2, 1, 0, 0], [0, -1, 208, -1, 272])]
    assert np.array_equal(stub.pump._slots[0].reshape(-1).view(np.uint8)[272:286], y.view(np.uint8))
