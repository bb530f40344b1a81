"""G.711 packets for the pump (vad_pump_submit_coded_packets, vad_g711_expand) on a machine WITHOUT a GPU: both symbols are exported and
bound, the host expansion gives the ITU-T G.711 values (those of Python's audioop, and an independent formula written here) for all 256
codes of each law, S16 is the identity, and bad arguments come back as a status, never a crash."""
import ctypes
import warnings

import numpy as np
import pytest

CODES = np.arange(256, dtype=np.uint8)


def ulaw_formula(code):
    """G.711 mu-law: the code is sent inverted; |x| = (2 m + 33) * 2^(e + 2) - 132, negative when the sign bit is set."""
    c = ~int(code) & 0xFF
    e, m = (c >> 4) & 7, c & 0xF
    mag = (2 * m + 33) * 2 ** (e + 2) - 132
    return -mag if c & 0x80 else mag


def alaw_formula(code):
    """G.711 A-law: the even bits are sent inverted; |x| = (2 m + 1) * 8 in segment 0, else (2 m + 33) * 2^(e + 2); positive when the
    sign bit is set."""
    c = int(code) ^ 0x55
    e, m = (c >> 4) & 7, c & 0xF
    mag = (2 * m + 1) * 8 if e == 0 else (2 * m + 33) * 2 ** (e + 2)
    return mag if c & 0x80 else -mag


def expand(L, codec, data, n=None):
    out = np.full(len(data) if n is None else max(n, 1), 12345, np.int16)
    rc = L.vad_g711_expand(codec, data.ctypes.data, len(data) if n is None else n, out.ctypes.data)
    return rc, out


def test_g711_symbols_exported_and_bound(built):
    from silero_vad_amd import _lib
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("vad_pump_submit_coded_packets", "vad_g711_expand"):
        assert hasattr(handle, name), name
        assert name in _lib.SYMBOLS, name
        assert getattr(_lib.lib(), name).restype is ctypes.c_int, name


@pytest.mark.parametrize("law", ["ulaw", "alaw"])
def test_g711_expand_all_codes(built, law):
    from silero_vad_amd import _lib, g711_expand
    codec, formula = {"ulaw": (1, ulaw_formula), "alaw": (2, alaw_formula)}[law]
    rc, got = expand(_lib.lib(), codec, CODES)
    assert rc == 0
    want = np.array([formula(c) for c in CODES], np.int16)
    assert np.array_equal(got, want)
    assert np.array_equal(g711_expand(CODES, law), want) and np.array_equal(g711_expand(CODES.reshape(16, 16), codec), want.reshape(16, 16))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            import audioop
    except ImportError:
        return
    ref = np.frombuffer((audioop.ulaw2lin if law == "ulaw" else audioop.alaw2lin)(CODES.tobytes(), 2), np.int16)
    assert np.array_equal(got, ref)


def test_g711_anchors(built):
    from silero_vad_amd import g711_expand
    assert g711_expand(np.array([0, 1, 2, 3], np.uint8), "ulaw").tolist() == [-32124, -31100, -30076, -29052]
    assert g711_expand(np.array([0xFC, 0xFD, 0xFE, 0xFF], np.uint8), "ulaw").tolist() == [24, 16, 8, 0]
    assert g711_expand(np.array([0, 1, 2, 3], np.uint8), "alaw").tolist() == [-5504, -5248, -6016, -5760]
    assert g711_expand(np.array([0xD5], np.uint8), "alaw").tolist() == [8]


def test_s16_is_identity(built):
    from silero_vad_amd import _lib, g711_expand
    x = np.random.default_rng(0).integers(-32768, 32768, 1001).astype(np.int16)
    out = np.zeros_like(x)
    assert _lib.lib().vad_g711_expand(0, x.ctypes.data, len(x), out.ctypes.data) == 0
    assert np.array_equal(out, x)
    y = g711_expand(x, "s16")
    assert np.array_equal(y, x) and y.ctypes.data != x.ctypes.data


def test_bad_arguments_return_a_status(built):
    from silero_vad_amd import _lib, g711_expand
    L = _lib.lib()
    for codec in (3, -1, 255):
        rc, out = expand(L, codec, CODES)
        assert rc == 1 and (out == 12345).all(), codec                                 # VAD_ERR_ARG, nothing written
    assert expand(L, 1, CODES, n=-1)[0] == 1
    assert L.vad_g711_expand(1, None, 4, None) == 1
    assert L.vad_g711_expand(1, None, 0, None) == 0                                    # nothing to do
    st, off, ln = (np.array(v, np.int32) for v in ([0], [0], [160]))
    cd = np.array([1], np.uint8)
    assert L.vad_pump_submit_coded_packets(None, 0, st.ctypes.data, off.ctypes.data, ln.ctypes.data, cd.ctypes.data, 1) == 1
    assert L.vad_pump_submit_coded_packets(None, 0, None, None, None, None, 0) == 1
    for bad in (lambda: g711_expand(CODES, "pcmu"), lambda: g711_expand(CODES, 3), lambda: g711_expand(CODES.astype(np.int16), "ulaw"),
                lambda: g711_expand(CODES, "s16")):
        with pytest.raises(ValueError):
            bad()
