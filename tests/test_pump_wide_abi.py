"""32 / 48 kHz packets for the pump (vad_pump_set_wideband, vad_pump_wide_slot, vad_pump_submit_wide_packets, vad_pump_wide_phase,
vad_decimate) on a machine WITHOUT a GPU: the five symbols are exported and bound, the host decimation is the reference's x[::step]
(src/silero_vad/utils_vad.py:39-42) carried across pieces by its phase, and bad arguments come back as a status, never a crash."""
import ctypes

import numpy as np
import pytest

WIDE = {"vad_pump_set_wideband": ctypes.c_int, "vad_pump_wide_slot": ctypes.c_void_p, "vad_pump_submit_wide_packets": ctypes.c_int,
        "vad_pump_wide_phase": ctypes.c_int, "vad_decimate": ctypes.c_long}


def raw_decimate(L, step, phase, x, n=None):
    out = np.full(len(x) + 1, 12345, np.int16)
    m = L.vad_decimate(step, phase, x.ctypes.data, len(x) if n is None else n, out.ctypes.data)
    return m, out


def test_wide_symbols_exported_and_bound(built):
    from silero_vad_amd import _lib
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name, restype in WIDE.items():
        assert hasattr(handle, name), name
        assert name in _lib.SYMBOLS, name
        assert _lib.SYMBOLS[name][0] is restype, name
        assert getattr(_lib.lib(), name).restype is restype, name


@pytest.mark.parametrize("step", [1, 2, 3])
def test_decimate_is_the_reference_comb(built, step):
    from silero_vad_amd import _lib, decimate
    L = _lib.lib()
    rng = np.random.default_rng(step)
    for phase in range(step):
        for n in (0, 1, 2, 3, 7, 8, 9, 1535, 1536):
            x = rng.integers(-32768, 32768, n).astype(np.int16)
            want = x[(-phase) % step::step]
            m, out = raw_decimate(L, step, phase, x)
            assert m == len(want), (phase, n)
            assert np.array_equal(out[:m], want) and (out[m:] == 12345).all(), (phase, n)
            got = decimate(x, step, phase)
            assert got.dtype == np.int16 and np.array_equal(got, want), (phase, n)


@pytest.mark.parametrize("step", [1, 2, 3])
def test_pieces_with_the_carried_phase_equal_the_whole(built, step):
    from silero_vad_amd import decimate
    rng = np.random.default_rng(40 + step)
    x = rng.integers(-32768, 32768, 20011).astype(np.int16)
    parts, at, phase = [], 0, 0
    while at < len(x):
        n = int(rng.integers(1, 1537)) if rng.random() < 0.8 else int(rng.integers(1, 4))
        piece = x[at:at + n]
        parts.append(decimate(piece, step, phase))
        phase = (phase + len(piece)) % step
        at += len(piece)
    assert np.array_equal(np.concatenate(parts), x[::step])


def test_bad_arguments_return_a_status(built):
    from silero_vad_amd import _lib, decimate
    L = _lib.lib()
    x = np.arange(16, dtype=np.int16)
    for step, phase in ((0, 0), (-1, 0), (3, 3), (3, -1), (1, 1)):
        m, out = raw_decimate(L, step, phase, x)
        assert m < 0 and (out == 12345).all(), (step, phase)                           # nothing written
    assert raw_decimate(L, 3, 0, x, n=-1)[0] < 0
    assert L.vad_decimate(3, 0, None, 4, None) < 0
    assert L.vad_decimate(3, 0, x.ctypes.data, 4, None) < 0
    assert L.vad_decimate(3, 1, None, 0, None) == 0                                    # nothing to do
    st, off, ln = (np.array(v, np.int32) for v in ([0], [0], [480]))
    sp = np.array([3], np.uint8)
    assert L.vad_pump_submit_wide_packets(None, 0, st.ctypes.data, off.ctypes.data, ln.ctypes.data, sp.ctypes.data, 1) == 1
    assert L.vad_pump_submit_wide_packets(None, 0, None, None, None, None, 0) == 1
    assert L.vad_pump_set_wideband(None, 3) == 1
    assert L.vad_pump_wide_slot(None, 0) is None
    assert L.vad_pump_wide_phase(None, 0) < 0
    for bad in (lambda: decimate(x, 0), lambda: decimate(x, 3, 3), lambda: decimate(x, 2, -1), lambda: decimate(x.astype(np.int32), 3),
                lambda: decimate(x.reshape(4, 4), 2), lambda: decimate(x, 2.0)):
        with pytest.raises(ValueError):
            bad()
