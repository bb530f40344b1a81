"""Snapshot and restore of the pump's streams (include/silero_vad_hip.h "SNAPSHOT AND RESTORE") on a machine WITHOUT a GPU: the entry
points in the header and in the library, the blob's size, the null-pump calls (a status, never a crash), the host-only readers on a
blob built here in numpy from the DOCUMENTED layout (so the header text, not the library, is what the test reads), each single
corruption of it, and the argument checks of the Python wrappers on a StreamPump with no pump behind it."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = ("vad_pump_snapshot_bytes", "vad_pump_export_streams", "vad_pump_import_streams", "vad_snapshot_inspect", "vad_snapshot_stream")
HEADER = 64
GEOMETRY = {16000: (512, 64), 8000: (256, 32)}          # sr -> (N, C)
FIELDS = ("active", "triggered", "temp_end", "current_sample", "pending", "wide_step", "wide_phase")


def stride_of(sr):
    n, c = GEOMETRY[sr]
    return 32 + 4 * (128 + 128 + c) + 2 * n


def make_blob(sr, records, version=1):
    """The documented layout, little-endian, written field by field."""
    n, c = GEOMETRY[sr]
    stride = stride_of(sr)
    blob = np.zeros(HEADER + len(records) * stride, np.uint8)
    blob[0:8] = np.frombuffer(b"SVADSNAP", np.uint8)
    blob[8:16].view("<u4")[:] = (version, HEADER)
    blob[16:28].view("<i4")[:] = (sr, n, c)
    blob[28:32].view("<u4")[:] = stride
    blob[32:40].view("<i8")[:] = len(records)
    blob[40:64].view("<f8")[:] = (0.5, sr * 100 / 1000.0, sr * 30 / 1000.0)
    for i, r in enumerate(records):
        rec = blob[HEADER + i * stride:HEADER + (i + 1) * stride]
        rec[0:16].view("<i8")[:] = (r["current_sample"], r["temp_end"])
        rec[16:20].view("<i4")[:] = r["pending"]
        rec[20:24] = (r["active"], r["triggered"], r["wide_step"], r["wide_phase"])
        rec[32:544].view("<f4")[:] = r["h"]
        rec[544:1056].view("<f4")[:] = r["c"]
        rec[1056:1056 + 4 * c].view("<f4")[:] = r["ctx"]
        rec[1056 + 4 * c:].view("<i2")[:] = r["pending_samples"]
    return blob


def two_records(sr):
    n, c = GEOMETRY[sr]
    rng = np.random.default_rng(sr)
    out = []
    for k, (act, trig, step, phase, pend) in enumerate(((1, 1, 3, 2, n - 1), (0, 0, 0, 0, 5))):
        samples = np.zeros(n, np.int16)
        samples[:pend] = rng.integers(-30000, 30000, pend)
        out.append(dict(active=act, triggered=trig, temp_end=(7 + k) * n, current_sample=(2 ** 33 + 9 + k) * n, pending=pend, wide_step=step,
                        wide_phase=phase, h=rng.standard_normal(128).astype(np.float32), c=(40 * rng.standard_normal(128)).astype(np.float32),
                        ctx=rng.standard_normal(c).astype(np.float32), pending_samples=samples))
    return out


def inspect(L, blob, nbytes=None):
    n, sr = ctypes.c_long(-7), ctypes.c_int(-7)
    rc = L.vad_snapshot_inspect(blob.ctypes.data, len(blob) if nbytes is None else nbytes, ctypes.byref(n), ctypes.byref(sr))
    return rc, n.value, sr.value


def test_the_header_declares_and_the_library_exports_the_entry_points(built):
    from silero_vad_amd import _lib
    text = (ROOT / "include" / "silero_vad_hip.h").read_text()
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"^(int|size_t)\s+" + name + r"\(", text, re.M), name
        assert name in _lib.SYMBOLS and getattr(L, name)
    assert re.search(r"typedef struct vad_stream_info \{", text) and ctypes.sizeof(_lib.StreamInfo) == 32


def test_blob_size(built):
    from silero_vad_amd import _lib
    L = _lib.lib()
    for sr in GEOMETRY:
        assert stride_of(sr) % 16 == 0
        for n in (0, 1, 5, 8192):
            assert L.vad_pump_snapshot_bytes(sr, n) == HEADER + n * stride_of(sr)
    assert stride_of(8000) < stride_of(16000)
    assert L.vad_pump_snapshot_bytes(44100, 1) == 0 and L.vad_pump_snapshot_bytes(16000, -1) == 0


def test_a_null_pump_returns_a_status(built):
    from silero_vad_amd import _lib
    L = _lib.lib()
    blob = make_blob(16000, two_records(16000))
    slots = np.array([0, 1], np.int32)
    assert L.vad_pump_export_streams(None, slots.ctypes.data, 2, blob.ctypes.data, len(blob)) == 1
    assert L.vad_pump_export_streams(None, None, 0, None, 0) == 1
    assert L.vad_pump_import_streams(None, blob.ctypes.data, len(blob), None, slots.ctypes.data, 2) == 1
    assert L.vad_pump_import_streams(None, None, 0, None, None, 0) == 1


@pytest.mark.parametrize("sr", [16000, 8000])
def test_the_readers_return_what_the_documented_layout_holds(built, sr):
    from silero_vad_amd import _lib, snapshot_info
    L = _lib.lib()
    n, c = GEOMETRY[sr]
    recs = two_records(sr)
    blob = make_blob(sr, recs)
    assert inspect(L, blob) == (0, 2, sr)
    assert L.vad_snapshot_inspect(blob.ctypes.data, len(blob), None, None) == 0
    odd = np.zeros(len(blob) + 1, np.uint8)[1:]                    # a blob need not be aligned, and may be longer than its records
    odd[:] = blob
    assert inspect(L, np.concatenate([blob, np.zeros(3, np.uint8)])) == (0, 2, sr)
    for src in (blob, odd):
        for i, want in enumerate(recs):
            f = _lib.StreamInfo()
            h, cc, x, pend = np.empty(128, np.float32), np.empty(128, np.float32), np.empty(c, np.float32), np.empty(n, np.int16)
            assert L.vad_snapshot_stream(src.ctypes.data, len(src), i, ctypes.byref(f), h.ctypes.data, cc.ctypes.data, x.ctypes.data, pend.ctypes.data) == 0
            assert {k: getattr(f, k) for k in FIELDS} == {k: want[k] for k in FIELDS}
            for a, b in ((h, "h"), (cc, "c"), (x, "ctx"), (pend, "pending_samples")):
                assert np.array_equal(a, want[b]), b
            assert L.vad_snapshot_stream(src.ctypes.data, len(src), i, None, None, None, None, None) == 0
    assert L.vad_snapshot_stream(blob.ctypes.data, len(blob), 2, None, None, None, None, None) == 1
    assert L.vad_snapshot_stream(blob.ctypes.data, len(blob), -1, None, None, None, None, None) == 1
    got = snapshot_info(blob)
    assert len(got) == 2
    for g, want in zip(got, recs):
        assert set(g) == set(want)
        for k in want:
            assert np.array_equal(g[k], want[k]), k
    assert snapshot_info(make_blob(sr, [])) == []


def corrupt(sr, what):
    n, _ = GEOMETRY[sr]
    recs = two_records(sr)
    blob = make_blob(sr, recs)
    rec1 = HEADER + stride_of(sr)                                  # the second record
    if what == "magic":
        blob[3] ^= 0x20
    elif what == "version":
        blob = make_blob(sr, recs, version=2)
    elif what == "one byte short":
        blob = blob[:-1].copy()
    elif what == "record count":
        blob[32:40].view("<i8")[:] = 3
    elif what == "pending = N":
        blob[rec1 + 16:rec1 + 20].view("<i4")[:] = n
    elif what == "pending < 0":
        blob[rec1 + 16:rec1 + 20].view("<i4")[:] = -1
    elif what == "wide_step = 4":
        blob[HEADER + 22] = 4
    elif what == "wide_phase = wide_step":
        blob[HEADER + 23] = 3
    elif what == "wide_phase without a step":
        blob[rec1 + 23] = 1
    elif what == "triggered = 2":
        blob[rec1 + 21] = 2
    elif what == "active = 2":
        blob[rec1 + 20] = 2
    elif what == "a reserved byte":
        blob[rec1 + 27] = 1
    elif what == "negative clock":
        blob[rec1:rec1 + 8].view("<i8")[:] = -1
    elif what == "another geometry":
        blob[20:24].view("<i4")[:] = n // 2
    elif what == "record count < 0":
        blob[32:40].view("<i8")[:] = -1
    return blob


@pytest.mark.parametrize("sr", [16000, 8000])
@pytest.mark.parametrize("what", ["magic", "version", "one byte short", "record count", "pending = N", "pending < 0", "wide_step = 4",
                                  "wide_phase = wide_step", "wide_phase without a step", "triggered = 2", "active = 2", "a reserved byte",
                                  "negative clock", "another geometry", "record count < 0"])
def test_each_single_corruption_is_refused(built, sr, what):
    from silero_vad_amd import _lib, snapshot_info
    L = _lib.lib()
    good = make_blob(sr, two_records(sr))
    blob = corrupt(sr, what)
    assert len(blob) != len(good) or (blob != good).sum() in range(1, 9)     # one field
    assert inspect(L, blob) == (1, -7, -7)
    assert L.vad_snapshot_stream(blob.ctypes.data, len(blob), 0, None, None, None, None, None) == 1
    with pytest.raises(_lib.VadError, match="VAD_ERR_ARG"):
        snapshot_info(blob)


def test_short_buffers_are_refused_without_being_read_past(built):
    from silero_vad_amd import _lib
    L = _lib.lib()
    blob = make_blob(16000, two_records(16000))
    for nbytes in (0, 1, HEADER - 1, HEADER, HEADER + stride_of(16000), len(blob) - 1):
        assert inspect(L, blob, nbytes)[0] == 1
    assert L.vad_snapshot_inspect(None, 0, None, None) == 1 and L.vad_snapshot_inspect(None, 4096, None, None) == 1


class Stub:
    """A StreamPump with no pump behind it: the library calls are recorded instead of made."""

    def __init__(self, sr=16000, cap=8):
        from silero_vad_amd import StreamPump, _lib

        class Calls:
            def __init__(s):
                s.made = []
                s.vad_pump_snapshot_bytes = _lib.lib().vad_pump_snapshot_bytes
                s.vad_pump_last_error = lambda h: b""

            def vad_pump_export_streams(s, h, st, n, blob, cap):
                s.made.append(("export", n))
                return 0

            def vad_pump_import_streams(s, h, blob, nbytes, rec, st, n):
                s.made.append(("import", nbytes, n, rec is not None))
                return 0
        self.L = Calls()
        p = StreamPump.__new__(StreamPump)
        p.n, p.streams, p.sr, p._L, p._h = GEOMETRY[sr][0], cap, sr, self.L, None
        self.pump = p


def test_the_python_wrappers_check_their_arguments_before_the_library_is_called(built):
    blob = make_blob(16000, two_records(16000))
    bad_calls = (lambda p: p.export_streams([0, 3, 0]),                                 # a slot twice
                 lambda p: p.export_streams([0.5]), lambda p: p.export_streams([[0, 1]]), lambda p: p.export_streams([2 ** 31]),
                 lambda p: p.import_streams(blob, [1, 1]),
                 lambda p: p.import_streams(blob, [0, 1], records=[0]),                 # lengths
                 lambda p: p.import_streams(blob, [0], records=[0, 1]),
                 lambda p: p.import_streams(blob, [0.0, 1.0]), lambda p: p.import_streams(blob, [0, 1], records=[0.0, 1.0]),
                 lambda p: p.import_streams(blob.astype(np.int8), [0, 1]),              # a blob is uint8 bytes
                 lambda p: p.import_streams(blob.reshape(2, -1), [0, 1]), lambda p: p.import_streams(list(range(4)), [0]))
    for call in bad_calls:
        stub = Stub()
        with pytest.raises(ValueError):
            call(stub.pump)
        assert stub.L.made == []
    stub = Stub()
    out = stub.pump.export_streams([5, 2])
    assert out.dtype == np.uint8 and out.shape == (HEADER + 2 * stride_of(16000),)
    assert stub.pump.export_streams().shape == (HEADER + 8 * stride_of(16000),)
    stub.pump.import_streams(blob, [3, 0])
    stub.pump.import_streams(blob, np.array([3, 0, 4]), records=[1, 1, 0])             # records may repeat: one blob, many slots
    assert stub.L.made == [("export", 2), ("export", 8), ("import", len(blob), 2, False), ("import", len(blob), 3, True)]
