"""The pump's packet route (vad_pump_submit_packets / vad_pump_pending) on a machine WITHOUT a GPU: both symbols are exported and
bound, and a null pump is refused with a status, never a crash."""
import ctypes

import numpy as np


def test_packet_symbols_exported_and_bound(built):
    from silero_vad_amd import _lib
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("vad_pump_submit_packets", "vad_pump_pending"):
        assert hasattr(handle, name), name
        assert name in _lib.SYMBOLS, name
        assert getattr(_lib.lib(), name).restype is _lib.SYMBOLS[name][0]


def test_packet_route_refuses_a_null_pump(built):
    from silero_vad_amd import _lib
    L = _lib.lib()
    st, off, ln = (np.array(v, np.int32) for v in ([0], [0], [320]))
    assert L.vad_pump_submit_packets(None, 0, st.ctypes.data, off.ctypes.data, ln.ctypes.data, 1) == 1       # VAD_ERR_ARG
    assert L.vad_pump_submit_packets(None, 0, None, None, None, 0) == 1
    assert L.vad_pump_pending(None, 0) < 0
    assert L.vad_pump_pending(None, -1) < 0
