"""DVI4 packets for the pump (VAD_PCM_DVI4, vad_adpcm_expand) on a machine WITHOUT a GPU: the symbol is exported and bound, the host
decode gives the values of the recurrence written out in tests/adpcm_codec.py (and of Python's audioop, where it imports) on every
first step, random payloads, both saturations of the predictor, the index floor, header indices above 88 and a nonzero reserved byte;
bad arguments come back as a status, never a crash; and the Python packers know the row's size, 4 + len / 2 bytes.
(The host decode's sanitizer run is tools/adpcm_asan.cpp, a stand-alone program; it is not run from here.)"""
import ctypes
import warnings

import numpy as np
import pytest

import adpcm_codec as ima


def raw_expand(L, p, nbytes=None, room=None):
    n = len(p) if nbytes is None else nbytes
    out = np.full(max(2 * (len(p) - 4), 2) if room is None else room, 12345, np.int16)
    return L.vad_adpcm_expand(p.ctypes.data, n, out.ctypes.data), out


def audioop_or_none():
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            import audioop
        return audioop
    except ImportError:
        return None


def by_audioop(audioop, p):
    predict = int(p[:2].view(">i2")[0])
    return np.frombuffer(audioop.adpcm2lin(p[4:].tobytes(), 2, (predict, min(int(p[2]), 88)))[0], np.int16)


def test_adpcm_symbol_exported_and_bound(built):
    import silero_vad_amd
    from silero_vad_amd import _lib
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("vad_adpcm_expand", "vad_pump_set_adpcm"):
        assert hasattr(handle, name) and name in _lib.SYMBOLS, name
    assert _lib.lib().vad_adpcm_expand.restype is ctypes.c_long and _lib.lib().vad_pump_set_adpcm.restype is ctypes.c_int
    assert _lib.lib().vad_pump_set_adpcm(None, 1) == 1          # VAD_ERR_ARG: no pump
    assert silero_vad_amd.adpcm_expand is silero_vad_amd.streams.adpcm_expand and silero_vad_amd.streams._PCM["dvi4"] == 3
    header_text = (_lib.LIB_PATH.parents[1] / "include" / "silero_vad_hip.h").read_text()
    assert "VAD_PCM_DVI4 = 3" in header_text and "long vad_adpcm_expand(const uint8_t *payload, long nbytes, int16_t *out);" in header_text


def test_every_first_step(built):
    """Every (index 0 ... 88) x (code 0 ... 15) from predictors in the middle and next to both ends: the first sample and, through the
    second code, the index the first one left behind."""
    from silero_vad_amd import adpcm_expand
    for predict in (0, -3, 32760, -32760):
        for index in range(89):
            for d in range(16):
                p = ima.payload(predict, index, [d, 5])
                first, idx = ima.step_once(d, predict, index)
                second, _ = ima.step_once(5, first, idx)
                assert adpcm_expand(p).tolist() == [first, second], (predict, index, d)


def test_random_payloads(built):
    from silero_vad_amd import _lib, adpcm_expand
    rng = np.random.default_rng(3551)
    audioop = audioop_or_none()
    L = _lib.lib()
    for nbytes in list(range(5, 40)) + [84, 164, 259, 260] + rng.integers(5, 261, 60).tolist():
        p = rng.integers(0, 256, nbytes).astype(np.uint8)
        want = ima.decode(p)
        got = adpcm_expand(p)
        assert got.dtype == np.int16 and np.array_equal(got, want), nbytes
        rc, out = raw_expand(L, p, room=len(want) + 4)
        assert rc == len(want) == 2 * (nbytes - 4) and np.array_equal(out[:rc], want) and (out[rc:] == 12345).all()
        if audioop is not None:
            assert np.array_equal(got, by_audioop(audioop, p)), nbytes


@pytest.mark.parametrize("n_codes", [2, 160, 512])
def test_saturation_index_floor_and_header_fields(built, n_codes):
    from silero_vad_amd import adpcm_expand
    audioop = audioop_or_none()
    sp = ima.special_payloads(n_codes)
    got = {k: adpcm_expand(p) for k, p in sp.items()}
    for k, p in sp.items():
        assert np.array_equal(got[k], ima.decode(p)), k
        if audioop is not None:
            assert np.array_equal(got[k], by_audioop(audioop, p)), k
    assert (got["saturate_up"] == 32767).all() and (got["saturate_down"] == -32768).all()
    assert np.array_equal(got["index_89"], got["index_88"]) and np.array_equal(got["index_255"], got["index_88"])
    assert np.array_equal(got["reserved"], got["index_0"])
    if n_codes >= 160:                                      # index 5 is on the floor after 5 codes: every later step adds 7 >> 3 = 0
        assert (np.diff(got["floor_up"][5:]) == 0).all() and (np.diff(got["floor_down"][5:]) == 0).all()
        assert got["cross_up"][-1] == 32767 and got["cross_down"][-1] == -32768


def test_empty_payload_and_bad_arguments(built):
    from silero_vad_amd import _lib, adpcm_expand
    L = _lib.lib()
    p = np.array([0, 0, 0, 0, 0x17, 0x00], np.uint8)
    assert adpcm_expand(p[:4]).shape == (0,) and adpcm_expand(p[:4]).dtype == np.int16
    assert L.vad_adpcm_expand(p.ctypes.data, 4, None) == 0 and L.vad_adpcm_expand(None, 4, None) == 0
    assert adpcm_expand(p[:5]).tolist() == [1, 12]             # step 7: code 1 adds 0 + 1, code 7 adds 0 + 7 + 3 + 1
    for nbytes in (3, 0, -1, -2 ** 40):
        rc, out = raw_expand(L, p, nbytes=nbytes)
        assert rc == -1 and (out == 12345).all(), nbytes        # -VAD_ERR_ARG, nothing written
    out = np.full(4, 12345, np.int16)
    assert L.vad_adpcm_expand(None, 6, out.ctypes.data) == -1 and L.vad_adpcm_expand(p.ctypes.data, 6, None) == -1
    assert L.vad_adpcm_expand(None, 5, None) == -1 and (out == 12345).all()
    for bad in (lambda: adpcm_expand(p[:3]), lambda: adpcm_expand(p.astype(np.int16)), lambda: adpcm_expand(p.reshape(2, 3)),
                lambda: adpcm_expand(np.zeros(0, np.uint8))):
        with pytest.raises(ValueError):
            bad()


def test_the_other_expanders_refuse_dvi4(built):
    """g711_expand, deinterleave and the corpus codec go on taking G.711 only; vad_g711_expand still answers codec 3 with a status."""
    from silero_vad_amd import _lib, deinterleave, g711_expand
    from silero_vad_amd.streams import _codec_of
    p = np.zeros(8, np.uint8)
    out = np.full(8, 12345, np.int16)
    assert _lib.lib().vad_g711_expand(3, p.ctypes.data, 8, out.ctypes.data) == 1 and (out == 12345).all()
    for bad in (lambda: g711_expand(p, "dvi4"), lambda: g711_expand(p, 3), lambda: deinterleave(p, 2, 0, "dvi4"),
                lambda: _codec_of([p], "dvi4")):
        with pytest.raises(ValueError):
            bad()


class Recorder:
    """In place of the library behind a StreamPump: the columns of every submit call, copied while the call is in progress."""

    def __init__(self):
        self.made = []
        self.vad_pump_last_error = lambda h: b""
        for name in ("coded_packets", "burst"):
            setattr(self, "vad_pump_submit_" + name, self.entry(name))

    def entry(self, name):
        def call(h, r, st, off, ln, cd, n):
            col = lambda ptr, ct: None if ptr is None else np.ctypeslib.as_array((ct * n).from_address(ptr)).tolist()      # noqa: E731
            self.made.append((name, r, col(st, ctypes.c_int32), col(off, ctypes.c_int32), col(ln, ctypes.c_int32), col(cd, ctypes.c_uint8)))
            return 0
        return call


@pytest.fixture(params=[512, 256])
def stub(built, request):
    from silero_vad_amd import StreamPump
    n = request.param
    p = StreamPump.__new__(StreamPump)
    p.n, p.streams, p.sr, p.ring_slots, p._L, p._h, p.max_burst = n, 8, {512: 16000, 256: 8000}[n], 2, Recorder(), None, 4
    p._slots = [np.full((8, n), 0x5A5A, np.int16) for _ in range(2)]
    p.adpcm = True
    return p


def test_a_pump_without_adpcm_knows_three_codecs(stub):
    """DVI4 rows are an opt-in of the pump (adpcm=True / set_adpcm): without it the packers and the row builder refuse "dvi4" and 3 in
    the words they always used, and nothing is written or called."""
    stub.adpcm = False
    names = "codec must be one of ['alaw', 's16', 'ulaw']"
    payload = np.zeros(84, np.uint8)
    for call, text in ((lambda: stub.write_coded_packets(0, [(1, payload, "dvi4")]), names + ", got 'dvi4'"),
                       (lambda: stub.write_burst(0, [(1, payload, 3)]), names + " or [0, 1, 2], got 3"),
                       (lambda: stub.submit_coded_packets(0, [1], [160], ["dvi4"]), names + ", got 'dvi4'"),
                       (lambda: stub.submit_burst(0, [1], [160], ["dvi4"]), names + ", got 'dvi4'")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text and stub._L.made == []
    assert (stub.packet_bytes(0) == 0x5A).all()
    stub.adpcm = True
    with pytest.raises(ValueError) as e:
        stub.write_coded_packets(0, [(1, payload, "g722")])
    assert str(e.value) == "codec must be one of ['alaw', 'dvi4', 's16', 'ulaw'], got 'g722'"


def test_packers_know_the_dvi4_row(stub):
    """write_coded_packets / write_burst take the payload with its header, derive the length 2 * (size - 4), place the rows at multiples
    of 16 bytes by their size 4 + len / 2, and refuse a payload without codes or above the route's cap; the default offsets of
    submit_coded_packets / submit_burst use the same size."""
    n = stub.n
    rng = np.random.default_rng(9)
    a, b, c, d = (rng.integers(0, 256, k).astype(np.uint8) for k in (84, 5, 4 + n // 2, 21))
    s16 = rng.integers(-9, 9, 7).astype(np.int16)
    stub.write_coded_packets(0, [(3, a, "dvi4"), (1, b, 3), (0, s16, "s16"), (5, c, "dvi4"), (2, 11, "dvi4"), (4, d, "ulaw")])
    at = [0, 96, 112, 128, -1, 128 + (4 + n // 2 + 15) // 16 * 16]
    assert stub._L.made.pop() == ("coded_packets", 0, [3, 1, 0, 5, 2, 4], at, [160, 2, 7, n, 11, 21], [3, 3, 0, 3, 3, 1])
    area = stub.packet_bytes(0)
    assert np.array_equal(area[0:84], a) and np.array_equal(area[96:101], b) and np.array_equal(area[128:128 + len(c)], c)
    assert (area[84:96] == 0x5A).all() and (area[101:112] == 0x5A).all()
    long_row = rng.integers(0, 256, 4 + n + 3).astype(np.uint8)          # 2 N + 6 samples
    stub.write_burst(1, [(6, long_row, "dvi4"), (6, s16), (6, b, "dvi4")])
    up = (len(long_row) + 15) // 16 * 16
    assert stub._L.made.pop() == ("burst", 1, [6, 6, 6], [0, up, up + 16], [2 * n + 6, 7, 2], [3, 0, 3])
    for writer, row, text in (("write_coded_packets", (1, a[:4], "dvi4"), "a 'dvi4' packet is its 4 header bytes and at least 1 byte of codes, got 4 bytes"),
                              ("write_burst", (1, a[:0], "dvi4"), "a 'dvi4' packet is its 4 header bytes and at least 1 byte of codes, got 0 bytes"),
                              ("write_coded_packets", (1, long_row[:4 + n // 2 + 1], "dvi4"),
                               f"a packet holds 1 ... {n} samples, got {n + 2} (submit a longer one over two ticks)"),
                              ("write_coded_packets", (1, s16, "dvi4"), "a 'dvi4' packet must be a 1-D uint8 array, got int16 of shape (7,)")):
        with pytest.raises(ValueError) as e:
            getattr(stub, writer)(0, [row])
        assert str(e.value) == text and stub._L.made == []
    stub.submit_coded_packets(0, [0, 1, 2, 3], [160, 2, 30, 8], ["dvi4", "dvi4", "s16", "alaw"])      # bytes 84 -> 96, 5 -> 16, 60 -> 64
    assert stub._L.made.pop() == ("coded_packets", 0, [0, 1, 2, 3], [0, 96, 112, 176], [160, 2, 30, 8], [3, 3, 0, 2])
    stub.submit_burst(0, [0, 0], [2 * n + 6, 8], [3, 3])
    assert stub._L.made.pop() == ("burst", 0, [0, 0], [0, up], [2 * n + 6, 8], [3, 3])
