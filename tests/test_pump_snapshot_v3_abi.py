"""Blob version 3 of the pump's snapshots (include/silero_vad_hip.h "THE BLOB (version 3)": each record carries a run of its stream's
tape) on a machine WITHOUT a GPU: the new entry points in the header and in the library, the blob's size, the host-only readers on blobs
built here in numpy from the DOCUMENTED layout, each single corruption of such a blob, blobs of versions 1 and 2 through the new code,
the run rule vad_tape_run against a statement of it in Python integers, and the argument checks of StreamPump.export_streams_v3 and
of the collector's open_starts / adopt on a pump with no pump behind it."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from test_pump_snapshot_abi import FIELDS, GEOMETRY, make_blob, stride_of, two_records
from test_pump_snapshot_v2_abi import HEADER2, TAIL_FIELDS, inspect, make_blob2, read_tail, stride2_of, three_records

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = ("vad_tape_run", "vad_snapshot_bytes_v3", "vad_pump_snapshot_plan_v3", "vad_pump_export_streams_v3", "vad_snapshot_tape")
HEADER3 = 128
STRIDE3 = {16000: 4768, 8000: 3104}                       # the figures the header states
RUNS = (3, 0, 1)                                          # chunks the three records of a test blob carry
DTYPE = {2: "<i2", 4: "<f4"}
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def _lib():
    from silero_vad_amd import _lib as m
    return m


def stride3_of(sr):
    return stride2_of(sr) + 32


def records_with_runs(L, sr, elem, runs=RUNS):
    """three_records, each ending at a chunk boundary of its clock, with `runs[i]` chunks of audio behind it"""
    n, _ = GEOMETRY[sr]
    rng = np.random.default_rng(sr + elem)
    out = []
    for r, k in zip(three_records(L, sr), runs):
        r = dict(r)
        assert r["current_sample"] % n == 0
        r["n_chunks"], r["first_chunk"] = k, (r["current_sample"] // n - k if k else 0)
        x = rng.integers(-32768, 32768, k * n)
        r["audio"] = x.astype(np.int16) if elem == 2 else (x / 32768.0).astype(np.float32)
        out.append(r)
    return out


def make_blob3(sr, records, elem):
    """The documented version 3 layout, little-endian, written field by field: the version 2 blob's records, each followed by its
    vad_tape_info, then the runs in record order."""
    n, _ = GEOMETRY[sr]
    s2, s3 = stride2_of(sr), stride3_of(sr)
    v2 = make_blob2(sr, records)
    tape_bytes = sum(r["n_chunks"] for r in records) * n * elem
    blob = np.zeros(HEADER3 + len(records) * s3 + tape_bytes, np.uint8)
    blob[:64] = v2[:64]
    blob[8:16].view("<u4")[:] = (3, HEADER3)
    blob[28:32].view("<u4")[:] = s3
    blob[64:68].view("<i4")[:] = elem
    blob[72:80].view("<i8")[:] = tape_bytes
    section, at = HEADER3 + len(records) * s3, 0
    for i, r in enumerate(records):
        rec = blob[HEADER3 + i * s3:HEADER3 + (i + 1) * s3]
        rec[:s2] = v2[HEADER2 + i * s2:HEADER2 + (i + 1) * s2]
        if r["n_chunks"]:
            rec[s2:s2 + 24].view("<i8")[:] = (r["first_chunk"], r["n_chunks"], at)
            size = r["n_chunks"] * n * elem
            blob[section + at:section + at + size] = r["audio"].astype(DTYPE[elem]).view(np.uint8)
            at += size
    return blob


def read_run(L, blob, i, cap=None):
    t = _lib().TapeInfo()
    out = np.full(len(blob) if cap is None else cap, 0x5a, np.uint8)
    rc = L.vad_snapshot_tape(blob.ctypes.data, len(blob), i, ctypes.byref(t), out.ctypes.data, len(out))
    return rc, t, out


def test_the_header_declares_and_the_library_exports_the_entry_points(built):
    text = (ROOT / "include" / "silero_vad_hip.h").read_text()
    L = _lib().lib()
    for name in ENTRY_POINTS:
        assert re.search(r"^(int|size_t)\s+" + name + r"\(", text, re.M), name
        assert name in _lib().SYMBOLS and getattr(L, name)
    assert re.search(r"typedef struct vad_tape_info \{", text) and ctypes.sizeof(_lib().TapeInfo) == 32
    for name, value in (("VAD_SNAPSHOT_VERSION_3", 3), ("VAD_SNAPSHOT_HEADER_BYTES_V3", HEADER3)):
        assert re.search(rf"^#define {name} {value}$", text, re.M), name
    # a null pump: a status, never a crash
    assert L.vad_pump_export_streams_v3(None, None, 0, None, None, 0) == 1 and L.vad_pump_snapshot_plan_v3(None, None, 0, None) == 0


def test_blob_size(built):
    L = _lib().lib()
    for sr, (n, _) in GEOMETRY.items():
        assert stride3_of(sr) == STRIDE3[sr] and stride3_of(sr) % 16 == 0
        for records in (0, 1, 5, 8192):
            assert L.vad_snapshot_bytes_v3(sr, records, 0, 0) == HEADER3 + records * stride3_of(sr)
            for elem in (2, 4):
                for chunks in (0, 1, 8192 * 32):
                    assert L.vad_snapshot_bytes_v3(sr, records, elem, chunks) == HEADER3 + records * stride3_of(sr) + chunks * n * elem
            assert L.vad_pump_snapshot_bytes_v2(sr, records) == HEADER2 + records * stride2_of(sr)       # version 2 is what it was
    for bad in ((44100, 1, 2, 1), (16000, -1, 2, 1), (16000, 1, 3, 1), (16000, 1, 0, 1), (16000, 1, 2, -1), (16000, 1, 4, 2 ** 62), (16000, 1, -2, 1)):
        assert L.vad_snapshot_bytes_v3(*bad) == 0, bad


@pytest.mark.parametrize("elem", [2, 4])
@pytest.mark.parametrize("sr", [16000, 8000])
def test_the_readers_return_what_the_documented_layout_holds(built, sr, elem):
    from silero_vad_amd import snapshot_info, snapshot_tape
    L = _lib().lib()
    n, c = GEOMETRY[sr]
    recs = records_with_runs(L, sr, elem)
    blob = make_blob3(sr, recs, elem)
    assert len(blob) == L.vad_snapshot_bytes_v3(sr, 3, elem, sum(RUNS))
    assert inspect(L, blob) == (0, 3, sr)
    odd = np.zeros(len(blob) + 1, np.uint8)[1:]                    # a blob need not be aligned
    odd[:] = blob
    at = 0
    for src in (blob, odd):
        at = 0
        for i, want in enumerate(recs):
            f = _lib().StreamInfo()
            h, cc, x, pend = np.empty(128, np.float32), np.empty(128, np.float32), np.empty(c, np.float32), np.empty(n, np.int16)
            assert L.vad_snapshot_stream(src.ctypes.data, len(src), i, ctypes.byref(f), h.ctypes.data, cc.ctypes.data, x.ctypes.data, pend.ctypes.data) == 0
            assert {k: getattr(f, k) for k in FIELDS} == {k: want[k] for k in FIELDS}
            for a, b in ((h, "h"), (cc, "c"), (x, "ctx"), (pend, "pending_samples")):
                assert np.array_equal(a, want[b]), b
            rc, q, carry, hist = read_tail(L, src, i, sr)
            assert rc == 0 and {k: getattr(q, k) for k in TAIL_FIELDS} == {k: want[k] for k in TAIL_FIELDS}
            assert carry.tobytes() == want["carry"].tobytes() and np.array_equal(hist, want["history"])
            size = want["n_chunks"] * n * elem
            rc, t, out = read_run(L, src, i)
            assert rc == 0 and (t.first_chunk, t.n_chunks, t.offset) == (want["first_chunk"], want["n_chunks"], at if size else 0)
            assert bytes(t.reserved) == bytes(8)
            assert out[:size].tobytes() == want["audio"].tobytes() and (out[size:] == 0x5a).all()          # exactly the run is written
            assert read_run(L, src, i, cap=size)[0] == 0
            if size:
                rc, _, out = read_run(L, src, i, cap=size - 1)
                assert rc == 1 and (out == 0x5a).all()
            assert L.vad_snapshot_tape(src.ctypes.data, len(src), i, None, None, 0) == 0
            got = snapshot_tape(src, i)
            assert got.dtype == (np.dtype(DTYPE[elem]) if size else np.int16) and got.tobytes() == want["audio"].tobytes()
            at += size
    assert L.vad_snapshot_tape(blob.ctypes.data, len(blob), 3, None, None, 0) == 1
    assert L.vad_snapshot_tape(blob.ctypes.data, len(blob), -1, None, None, 0) == 1
    info = snapshot_info(blob)
    assert len(info) == 3
    for g, want in zip(info, recs):
        assert set(g) == set(two_records(sr)[0]) | {"resample", "tape"}
        for k in two_records(sr)[0]:
            assert np.array_equal(g[k], want[k]), k
        assert {k: g["resample"][k] for k in TAIL_FIELDS} == {k: want[k] for k in TAIL_FIELDS}
        t = g["tape"]
        assert (t["first_chunk"], t["n_chunks"], t["elem"]) == (want["first_chunk"], want["n_chunks"], elem)
        assert t["audio"].dtype == np.dtype(DTYPE[elem]) and t["audio"].tobytes() == want["audio"].tobytes()
    assert [g["tape"]["offset"] for g in info] == [0, 0, RUNS[0] * n * elem]
    empty = make_blob3(sr, [], elem)
    assert snapshot_info(empty) == [] and inspect(L, empty) == (0, 0, sr) and len(empty) == HEADER3


@pytest.mark.parametrize("sr", [16000, 8000])
def test_a_blob_of_a_pump_without_a_tape(built, sr):
    from silero_vad_amd import snapshot_info, snapshot_tape
    L = _lib().lib()
    recs = records_with_runs(L, sr, 2, runs=(0, 0, 0))
    blob = make_blob3(sr, recs, 0)
    assert len(blob) == HEADER3 + 3 * stride3_of(sr) and inspect(L, blob) == (0, 3, sr)
    for i in range(3):
        rc, t, out = read_run(L, blob, i)
        assert rc == 0 and (t.first_chunk, t.n_chunks, t.offset) == (0, 0, 0) and (out == 0x5a).all()
        assert snapshot_tape(blob, i).size == 0
    assert all(g["tape"]["elem"] == 0 and g["tape"]["audio"].size == 0 for g in snapshot_info(blob))


@pytest.mark.parametrize("sr", [16000, 8000])
def test_blobs_of_versions_1_and_2_read_as_before(built, sr):
    from silero_vad_amd import snapshot_info, snapshot_tape
    L = _lib().lib()
    v1, v2 = make_blob(sr, two_records(sr)), make_blob2(sr, three_records(L, sr))
    assert inspect(L, v1) == (0, 2, sr) and inspect(L, v2) == (0, 3, sr)
    for blob, count in ((v1, 2), (v2, 3)):
        for i in range(count):
            rc, t, out = read_run(L, blob, i)
            assert rc == 0 and (t.first_chunk, t.n_chunks, t.offset) == (0, 0, 0) and bytes(t.reserved) == bytes(8) and (out == 0x5a).all()
            assert snapshot_tape(blob, i).size == 0
        assert L.vad_snapshot_tape(blob.ctypes.data, len(blob), count, None, None, 0) == 1
        assert all("tape" not in g for g in snapshot_info(blob))
        assert inspect(L, np.concatenate([blob, np.zeros(5, np.uint8)]))[0] == 0          # (they may still lie in a longer buffer)
    assert all("resample" in g for g in snapshot_info(v2)) and all("resample" not in g for g in snapshot_info(v1))
    for i, want in enumerate(three_records(L, sr)):
        rc, q, carry, hist = read_tail(L, v2, i, sr)
        assert rc == 0 and {k: getattr(q, k) for k in TAIL_FIELDS} == {k: want[k] for k in TAIL_FIELDS}


CORRUPTIONS = ["tape_elem 3", "tape_elem 0 with a run", "n_chunks < 0", "n_chunks = 2^62", "first_chunk < 0", "an offset off by 16",
               "tape_bytes one run short", "one byte short", "16 bytes long", "a run that does not end at current_sample",
               "an empty run with a first_chunk", "an empty run with an offset", "a reserved header word", "the last reserved header byte",
               "a reserved info byte", "a v2 header size under version 3", "a v2 stride under version 3", "a v2 layout that says version 3",
               "version 4", "a v1 field: pending = N", "a v2 field: c = N", "tape_bytes < 0", "runs in the wrong order"]


def corrupt(L, sr, elem, what):
    n, _ = GEOMETRY[sr]
    recs = records_with_runs(L, sr, elem)
    blob = make_blob3(sr, recs, elem)
    s1, s2, s3 = stride_of(sr), stride2_of(sr), stride3_of(sr)
    info0, info1, info2 = (HEADER3 + i * s3 + s2 for i in range(3))                 # runs of 3, 0 and 1 chunks
    run = n * elem
    if what == "tape_elem 3":
        blob[64:68].view("<i4")[:] = 3
    elif what == "tape_elem 0 with a run":
        blob[64:68].view("<i4")[:] = 0
    elif what == "n_chunks < 0":
        blob[info1 + 8:info1 + 16].view("<i8")[:] = -1
    elif what == "n_chunks = 2^62":
        blob[info2 + 8:info2 + 16].view("<i8")[:] = 2 ** 62
    elif what == "first_chunk < 0":
        blob[info1:info1 + 8].view("<i8")[:] = -1
    elif what == "an offset off by 16":
        blob[info2 + 16:info2 + 24].view("<i8")[:] += 16
    elif what == "tape_bytes one run short":
        blob[72:80].view("<i8")[:] -= run
    elif what == "one byte short":
        blob = blob[:-1].copy()
    elif what == "16 bytes long":
        blob = np.concatenate([blob, np.zeros(16, np.uint8)])
    elif what == "a run that does not end at current_sample":
        blob[info0:info0 + 8].view("<i8")[:] += 1
    elif what == "an empty run with a first_chunk":
        blob[info1:info1 + 8].view("<i8")[:] = 5
    elif what == "an empty run with an offset":
        blob[info1 + 16:info1 + 24].view("<i8")[:] = 3 * run
    elif what == "a reserved header word":
        blob[68:72].view("<i4")[:] = 1
    elif what == "the last reserved header byte":
        blob[127] = 0x80
    elif what == "a reserved info byte":
        blob[info1 + 24 + 3] = 1
    elif what == "a v2 header size under version 3":
        blob[12:16].view("<u4")[:] = HEADER2
    elif what == "a v2 stride under version 3":
        blob[28:32].view("<u4")[:] = s2
    elif what == "a v2 layout that says version 3":
        blob = make_blob2(sr, recs)
        blob[8:12].view("<u4")[:] = 3
    elif what == "version 4":
        blob[8:12].view("<u4")[:] = 4
    elif what == "a v1 field: pending = N":                       # the version 1 part is held against its ranges as before
        at = HEADER3 + s3 + 16
        blob[at:at + 4].view("<i4")[:] = n
    elif what == "a v2 field: c = N":                             # ... and the version 2 tail against its
        at = HEADER3 + s1 + 4
        blob[at:at + 4].view("<i4")[:] = n
    elif what == "tape_bytes < 0":
        blob[72:80].view("<i8")[:] = -1
    elif what == "runs in the wrong order":                        # both runs lie inside the section, but not one behind the other
        blob[info0 + 16:info0 + 24].view("<i8")[:] = run
        blob[info2 + 16:info2 + 24].view("<i8")[:] = 0
    else:
        raise AssertionError(what)
    return blob


@pytest.mark.parametrize("elem", [2, 4])
@pytest.mark.parametrize("sr", [16000, 8000])
@pytest.mark.parametrize("what", CORRUPTIONS)
def test_each_single_corruption_is_refused(built, sr, elem, what):
    from silero_vad_amd import snapshot_info, snapshot_tape
    L = _lib().lib()
    good = make_blob3(sr, records_with_runs(L, sr, elem), elem)
    assert inspect(L, good) == (0, 3, sr)
    blob = corrupt(L, sr, elem, what)
    assert len(blob) != len(good) or (blob != good).sum() in range(1, 17)     # one field (two for the swapped offsets)
    assert inspect(L, blob) == (1, -7, -7)
    assert L.vad_snapshot_stream(blob.ctypes.data, len(blob), 0, None, None, None, None, None) == 1
    assert L.vad_snapshot_resample(blob.ctypes.data, len(blob), 0, None, None, None) == 1
    rc, _, out = read_run(L, blob, 0)
    assert rc == 1 and (out == 0x5a).all()
    with pytest.raises(_lib().VadError, match="VAD_ERR_ARG"):
        snapshot_info(blob)
    with pytest.raises(_lib().VadError, match="VAD_ERR_ARG"):
        snapshot_tape(blob, 0)


def test_short_buffers_are_refused_without_being_read_past(built):
    L = _lib().lib()
    blob = make_blob3(16000, records_with_runs(L, 16000, 2), 2)
    s3 = stride3_of(16000)
    for nbytes in (0, 1, 63, 64, HEADER2, HEADER3 - 1, HEADER3, HEADER3 + 2 * s3, HEADER3 + 3 * s3, HEADER3 + 3 * s3 + 1024, len(blob) - 1):
        assert inspect(L, blob, nbytes)[0] == 1
    assert inspect(L, blob)[0] == 0


def run_rule(count, floor, chunks, n, start):
    """THE RUN of include/silero_vad_hip.h in Python integers"""
    held_lo = max(floor, count - chunks)
    first = min(max(start // n, held_lo), count)
    return first, count - first


@pytest.mark.parametrize("n", [512, 256])
def test_the_run_rule(built, n):
    from silero_vad_amd import tape_run
    L = _lib().lib()
    cases = [(3, 0, 5), (5, 0, 5),                                # before the ring has wrapped, and exactly full
             (8, 0, 5), (1000, 0, 7),                             # wrapped
             (8, 6, 5), (8, 8, 5), (20, 19, 64),                  # floor > count - chunks: an import in between
             (0, 0, 2), (2 ** 40, 2 ** 40 - 3, 512)]
    for count, floor, chunks in cases:
        held_lo = max(floor, count - chunks)
        starts = [I64_MIN, -5, 0, held_lo * n, held_lo * n + 1, held_lo * n + n - 1, (held_lo + 1) * n, (held_lo + 1) * n + n // 2 + 17,
                  count * n - 1, count * n, count * n + 1, I64_MAX]
        for start in starts:
            first, m = ctypes.c_int64(-7), ctypes.c_int64(-7)
            assert L.vad_tape_run(count, floor, chunks, n, start, ctypes.byref(first), ctypes.byref(m)) == 0
            want = run_rule(count, floor, chunks, n, start)
            assert (first.value, m.value) == want, (count, floor, chunks, start)
            assert tape_run(count, floor, chunks, n, start) == want
            assert held_lo <= first.value <= max(count, held_lo) and 0 <= m.value <= min(chunks, count)
    # a position in the middle of a chunk rounds down to its chunk; everything held; nothing
    assert tape_run(8, 0, 5, n, 4 * n + 17) == (4, 4) and tape_run(8, 0, 5, n, -5) == (3, 5) and tape_run(8, 0, 5, n, 2 ** 62) == (8, 0)
    first, m = ctypes.c_int64(-7), ctypes.c_int64(-7)
    for bad in ((8, 0, 1, n, 0), (8, 0, 5, 0, 0), (-1, 0, 5, n, 0), (8, -1, 5, n, 0), (2 ** 62, 0, 5, n, 0), (8, 2 ** 62, 5, n, 0)):
        assert L.vad_tape_run(*bad, ctypes.byref(first), ctypes.byref(m)) == 1, bad
        assert (first.value, m.value) == (-7, -7)
        with pytest.raises(ValueError):
            tape_run(*bad)
    assert L.vad_tape_run(8, 0, 5, n, 0, None, ctypes.byref(m)) == 1 and L.vad_tape_run(8, 0, 5, n, 0, ctypes.byref(first), None) == 1
    for bad in ((8.0, 0, 5, n, 0), (8, 0, 5, n, True), (8, 0, 5, n, 2 ** 63), (8, 0, 2 ** 31, n, 0)):
        with pytest.raises(ValueError):
            tape_run(*bad)


class Stub:
    """A StreamPump with no pump behind it: the library calls are recorded instead of made."""

    def __init__(self, sr=16000, cap=8, plan=0):
        from silero_vad_amd import StreamPump

        class Calls:
            def __init__(s):
                s.made = []
                s.vad_pump_snapshot_bytes = _lib().lib().vad_pump_snapshot_bytes
                s.vad_pump_snapshot_bytes_v2 = _lib().lib().vad_pump_snapshot_bytes_v2
                s.vad_pump_last_error = lambda h: b"said the stub"

            def vad_pump_export_streams(s, h, st, n, blob, cap):
                s.made.append(("export", n, cap))
                return 0

            def vad_pump_snapshot_plan_v3(s, h, st, n, tf):
                s.made.append(("plan_v3", n, st is not None, None if tf is None else np.ctypeslib.as_array(ctypes.cast(tf, ctypes.POINTER(ctypes.c_int64)), (n,)).tolist()))
                return plan

            def vad_pump_export_streams_v3(s, h, st, n, tf, blob, cap):
                s.made.append(("export_v3", n, tf is not None, cap))
                return 0
        self.L = Calls()
        p = StreamPump.__new__(StreamPump)
        p.n, p.streams, p.sr, p._L, p._h = GEOMETRY[sr][0], cap, sr, self.L, None
        self.pump = p


def test_export_streams_v3_checks_its_arguments_before_the_library_is_called(built):
    for bad in (0, 3, 4, "3", 3.0, None, True):                    # export_streams goes on writing versions 1 and 2 only
        stub = Stub()
        with pytest.raises(ValueError, match="version"):
            stub.pump.export_streams([0, 1], version=bad)
        assert stub.L.made == []
    for args, kw in ((([5, 2],), dict(tape_from=[0])), (([5, 2],), dict(tape_from=[0.5, 1.0])), (([5, 2],), dict(tape_from=[[0, 1]])),
                     (([5, 5],), {}), (([0.5],), {}), (([2 ** 31],), {}), ((), dict(tape_from=[0, 0]))):
        stub = Stub()
        with pytest.raises(ValueError):
            stub.pump.export_streams_v3(*args, **kw)
        assert stub.L.made == []
    stub = Stub()
    with pytest.raises(TypeError):
        stub.pump.export_streams([5, 2], tape_from=[0, 0])         # the tape goes with export_streams_v3
    assert stub.L.made == []
    stub = Stub(plan=4096)
    assert stub.pump.export_streams_v3([5, 2]).shape == (4096,)
    assert stub.pump.export_streams_v3([5, 2], tape_from=[7, -5]).shape == (4096,)
    assert stub.pump.export_streams_v3([5, 2], tape_from={2: 1024}).shape == (4096,)                  # a dict: the others carry nothing
    assert stub.pump.export_streams_v3(tape_from={}).shape == (4096,)
    assert stub.pump.export_streams([5, 2]).shape == (64 + 2 * stride_of(16000),)                     # version 1, as ever
    assert stub.L.made == [("plan_v3", 2, True, None), ("export_v3", 2, False, 4096),
                           ("plan_v3", 2, True, [7, -5]), ("export_v3", 2, True, 4096),
                           ("plan_v3", 2, True, [I64_MAX, 1024]), ("export_v3", 2, True, 4096),
                           ("plan_v3", 8, False, [I64_MAX] * 8), ("export_v3", 8, True, 4096),
                           ("export", 2, 64 + 2 * stride_of(16000))]
    stub = Stub(plan=0)                                            # the plan refused: the library's message, no export
    with pytest.raises(_lib().VadError, match="said the stub"):
        stub.pump.export_streams_v3([5, 2])
    assert [m[0] for m in stub.L.made] == ["plan_v3"]


def test_the_collector_hands_its_open_starts_over():
    from silero_vad_amd import UtteranceCollector

    class Taped:
        tape_chunks = 4

        def fetch_audio(self, streams, starts, ends):
            self.asked = (list(streams), list(starts), list(ends))
            return [np.arange(e - s, dtype=np.int16) for s, e in zip(starts, ends)], np.array(starts, np.int64)

    a, b = UtteranceCollector(Taped()), UtteranceCollector(Taped())
    assert a.open_starts() == {} and a.open_starts([3]) == {}
    a.feed([(3, {"start": 1000}), (5, {"start": 2000}), (6, {"start": 50}), (6, {"end": 900})])
    assert a.open_starts() == {3: 1000, 5: 2000} and a.open_starts([5, 6, 7]) == {5: 2000} and a.open_starts(np.array([3], np.int32)) == {3: 1000}
    a.open_starts()[9] = 1                                         # a copy
    assert 9 not in a.open_starts()
    b.adopt(0, a.open_starts()[3])
    a.forget(3)
    assert a.open_starts() == {5: 2000} and b.open_starts() == {0: 1000}
    out = b.feed([(0, {"end": 1512})])
    assert b.pump.asked == ([0], [1000], [1512]) and out[0][:4] == (0, 1000, 1512, 1000) and len(out[0][4]) == 512
    assert b.open_starts() == {}
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError):
            b.adopt(0, bad)
