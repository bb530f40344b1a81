"""Burst ticks of the pump (vad_pump_set_burst, vad_pump_submit_burst, vad_pump_burst_steps, vad_pump_burst_probs) on a machine WITHOUT
a GPU: the four symbols are exported, listed in the binding with the right result types, and a NULL pump comes back as a status / NULL,
never a crash."""
import ctypes
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
NAMES = {"vad_pump_set_burst": ctypes.c_int, "vad_pump_submit_burst": ctypes.c_int, "vad_pump_burst_steps": ctypes.c_int,
         "vad_pump_burst_probs": ctypes.c_void_p}


def test_burst_symbols_exported_and_bound(built):
    from silero_vad_amd import _lib
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name, restype in NAMES.items():
        assert hasattr(handle, name), name
        assert name in _lib.SYMBOLS, name
        assert _lib.SYMBOLS[name][0] is restype, name
        assert getattr(_lib.lib(), name).restype is restype, name
    assert len(_lib.SYMBOLS["vad_pump_submit_burst"][1]) == 7 and len(_lib.SYMBOLS["vad_pump_burst_probs"][1]) == 3


def test_header_states_the_burst_limit():
    text = (ROOT / "include" / "silero_vad_hip.h").read_text()
    m = re.search(r"^#define\s+VAD_PUMP_MAX_BURST\s+(\d+)\s*$", text, flags=re.M)
    assert m and int(m.group(1)) == 8


def test_null_pump_is_refused(built):
    from silero_vad_amd import _lib
    L = _lib.lib()
    st, off, ln = (np.array(v, np.int32) for v in ([0, 0], [0, 2048], [960, 960]))
    cd = np.array([0, 1], np.uint8)
    assert L.vad_pump_set_burst(None, 8) == 1                                                          # VAD_ERR_ARG
    assert L.vad_pump_set_burst(None, 0) == 1
    assert L.vad_pump_submit_burst(None, 0, st.ctypes.data, off.ctypes.data, ln.ctypes.data, cd.ctypes.data, 2) == 1
    assert L.vad_pump_submit_burst(None, 0, None, None, None, None, 0) == 1
    assert L.vad_pump_burst_steps(None, 0) < 0
    assert L.vad_pump_burst_probs(None, 0, 0) is None and L.vad_pump_burst_probs(None, 0, 1) is None


def test_python_refuses_a_bad_max_burst(built):
    """The argument is checked before anything touches a device."""
    import pytest
    from silero_vad_amd import StreamPump
    for bad in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match="max_burst"):
            StreamPump(None, 16000, streams=16, max_burst=bad)
