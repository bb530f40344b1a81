"""Blob version 2 of the pump's snapshots (include/silero_vad_hip.h "THE BLOB (version 2)": the record of a stream that is bound to a
resampled rate) on a machine WITHOUT a GPU: the new entry points in the header and in the library, the blob's size, the host-only
readers on blobs built here in numpy from the DOCUMENTED layout, each single corruption of such a blob, a version 1 blob through the
new reader, the counters the submit path's period reduction can produce against the ranges the readers demand, and the `version=`
argument of StreamPump.export_streams on a pump with no pump behind it."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from test_pump_snapshot_abi import FIELDS, GEOMETRY, make_blob, stride_of, two_records

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = ("vad_pump_snapshot_bytes_v2", "vad_pump_export_streams_v2", "vad_snapshot_resample")
HEADER2, HISTORY = 96, 160
STRIDE2 = {16000: 4736, 8000: 3072}                       # the figures the header states
RATES = {16000: (44100, 11025), 8000: (44100, 24000)}     # the two bound records of a test blob, per sample rate
TAIL_FIELDS = ("src_rate", "pending_out", "inputs_mod", "outputs_mod")


def stride2_of(sr):
    n, _ = GEOMETRY[sr]
    return stride_of(sr) + 32 + 4 * n + 2 * HISTORY


def pair(L, rate, sr):
    O, N = ctypes.c_int(), ctypes.c_int()
    assert L.vad_resample_geometry(rate, sr, ctypes.byref(O), ctypes.byref(N), None, None) == 0
    return O.value, N.value, L.vad_resample_stream_history(rate, sr)


def reduced(L, rate, sr, received):
    """(g, m) of a stream that has received `received` inputs: both less the whole periods its emitted outputs hold."""
    O, Nr, _ = pair(L, rate, sr)
    m1 = L.vad_resample_stream_ready(rate, sr, received)
    return received - m1 // Nr * O, m1 % Nr


def make_blob2(sr, records):
    """The documented version 2 layout, little-endian, written field by field: the version 1 blob's records, each followed by its tail."""
    n, _ = GEOMETRY[sr]
    s1, s2 = stride_of(sr), stride2_of(sr)
    v1 = make_blob(sr, records)
    blob = np.zeros(HEADER2 + len(records) * s2, np.uint8)
    blob[:64] = v1[:64]
    blob[8:16].view("<u4")[:] = (2, HEADER2)
    blob[28:32].view("<u4")[:] = s2
    for i, r in enumerate(records):
        rec = blob[HEADER2 + i * s2:HEADER2 + (i + 1) * s2]
        rec[:s1] = v1[64 + i * s1:64 + (i + 1) * s1]
        rec[s1:s1 + 8].view("<i4")[:] = (r["src_rate"], r["pending_out"])
        rec[s1 + 8:s1 + 24].view("<i8")[:] = (r["inputs_mod"], r["outputs_mod"])
        rec[s1 + 32:s1 + 32 + 4 * n].view("<f4")[:] = r["carry"]
        rec[s1 + 32 + 4 * n:].view("<i2")[:] = r["history"]
    return blob


def three_records(L, sr):
    """bound to RATES[sr][0] mid-chunk, unbound with int16 samples pending, bound to RATES[sr][1] with nothing pending"""
    n, _ = GEOMETRY[sr]
    rng = np.random.default_rng(sr + 2)
    base = two_records(sr)
    out = []
    for k, (rate, c, received) in enumerate(((RATES[sr][0], n - 1, 12345), (0, 0, 0), (RATES[sr][1], 0, 7))):
        r = dict(base[k % 2])
        carry, hist = np.zeros(n, np.float32), np.zeros(HISTORY, np.int16)
        g = m = 0
        if rate:
            r["pending"], r["pending_samples"] = 0, np.zeros(n, np.int16)       # a bound stream has no int16 samples pending
            H = pair(L, rate, sr)[2]
            g, m = reduced(L, rate, sr, received)
            carry[:c] = rng.standard_normal(c).astype(np.float32)
            hist[:H] = rng.integers(-30000, 30000, H)
        r.update(src_rate=rate, pending_out=c, inputs_mod=g, outputs_mod=m, carry=carry, history=hist)
        out.append(r)
    return out


def inspect(L, blob, nbytes=None):
    n, sr = ctypes.c_long(-7), ctypes.c_int(-7)
    rc = L.vad_snapshot_inspect(blob.ctypes.data, len(blob) if nbytes is None else nbytes, ctypes.byref(n), ctypes.byref(sr))
    return rc, n.value, sr.value


def read_tail(L, blob, i, sr):
    q = _lib().ResampleInfo()
    carry, hist = np.full(GEOMETRY[sr][0], 7, np.float32), np.full(HISTORY, 7, np.int16)
    rc = L.vad_snapshot_resample(blob.ctypes.data, len(blob), i, ctypes.byref(q), carry.ctypes.data, hist.ctypes.data)
    return rc, q, carry, hist


def _lib():
    from silero_vad_amd import _lib as m
    return m


def test_the_header_declares_and_the_library_exports_the_entry_points(built):
    text = (ROOT / "include" / "silero_vad_hip.h").read_text()
    L = _lib().lib()
    for name in ENTRY_POINTS:
        assert re.search(r"^(int|size_t)\s+" + name + r"\(", text, re.M), name
        assert name in _lib().SYMBOLS and getattr(L, name)
    assert re.search(r"typedef struct vad_resample_info \{", text) and ctypes.sizeof(_lib().ResampleInfo) == 32
    for name, value in (("VAD_SNAPSHOT_VERSION", 1), ("VAD_SNAPSHOT_VERSION_2", 2), ("VAD_SNAPSHOT_HEADER_BYTES_V2", HEADER2), ("VAD_SNAPSHOT_HISTORY", HISTORY)):
        assert re.search(rf"^#define {name} {value}$", text, re.M), name


def test_blob_size(built):
    L = _lib().lib()
    for sr in GEOMETRY:
        assert stride2_of(sr) == STRIDE2[sr] and stride2_of(sr) % 16 == 0
        for n in (0, 1, 5, 8192):
            assert L.vad_pump_snapshot_bytes_v2(sr, n) == HEADER2 + n * stride2_of(sr)
            assert L.vad_pump_snapshot_bytes(sr, n) == 64 + n * stride_of(sr)            # version 1 is what it was
    assert L.vad_pump_snapshot_bytes_v2(44100, 1) == 0 and L.vad_pump_snapshot_bytes_v2(16000, -1) == 0
    assert L.vad_pump_export_streams_v2(None, None, 0, None, 0) == 1                      # a null pump: a status, never a crash


def test_the_history_capacity_holds_every_served_pair(built):
    """VAD_SNAPSHOT_HISTORY, as the header states it, against the H of the pairs the library serves."""
    L = _lib().lib()
    text = (ROOT / "include" / "silero_vad_hip.h").read_text()
    capacity = int(re.search(r"^#define VAD_SNAPSHOT_HISTORY (\d+)$", text, re.M).group(1))
    assert capacity == HISTORY
    served = 0
    for sr in GEOMETRY:
        for rate in (11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000):
            H = L.vad_resample_stream_history(rate, sr)
            if H >= 0:
                served += 1
                assert H <= capacity, (rate, sr, H)
    assert served >= 8


@pytest.mark.parametrize("sr", [16000, 8000])
def test_the_readers_return_what_the_documented_layout_holds(built, sr):
    from silero_vad_amd import snapshot_info
    L = _lib().lib()
    n, c = GEOMETRY[sr]
    recs = three_records(L, sr)
    blob = make_blob2(sr, recs)
    assert inspect(L, blob) == (0, 3, sr)
    odd = np.zeros(len(blob) + 1, np.uint8)[1:]                    # a blob need not be aligned, and may be longer than its records
    odd[:] = blob
    assert inspect(L, np.concatenate([blob, np.zeros(5, np.uint8)])) == (0, 3, sr)
    for src in (blob, odd):
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
            assert L.vad_snapshot_resample(src.ctypes.data, len(src), i, None, None, None) == 0
    assert L.vad_snapshot_resample(blob.ctypes.data, len(blob), 3, None, None, None) == 1
    assert L.vad_snapshot_resample(blob.ctypes.data, len(blob), -1, None, None, None) == 1
    got = snapshot_info(blob)
    assert len(got) == 3
    for g, want in zip(got, recs):
        H = pair(L, want["src_rate"], sr)[2] if want["src_rate"] else 0
        assert set(g) == set(two_records(sr)[0]) | {"resample"}
        for k in two_records(sr)[0]:
            assert np.array_equal(g[k], want[k]), k
        rs = g["resample"]
        assert set(rs) == set(TAIL_FIELDS) | {"carry", "history"}
        assert {k: rs[k] for k in TAIL_FIELDS} == {k: want[k] for k in TAIL_FIELDS}
        assert rs["carry"].dtype == np.float32 and rs["carry"].tobytes() == want["carry"][:want["pending_out"]].tobytes()
        assert rs["history"].dtype == np.int16 and np.array_equal(rs["history"], want["history"][:H])
    assert snapshot_info(make_blob2(sr, [])) == [] and inspect(L, make_blob2(sr, [])) == (0, 0, sr)


@pytest.mark.parametrize("sr", [16000, 8000])
def test_a_version_1_blob_has_a_zero_tail_and_its_own_output(built, sr):
    from silero_vad_amd import snapshot_info
    L = _lib().lib()
    blob = make_blob(sr, two_records(sr))
    for i in range(2):
        rc, q, carry, hist = read_tail(L, blob, i, sr)
        assert rc == 0 and all(getattr(q, k) == 0 for k in TAIL_FIELDS) and bytes(q.reserved) == bytes(8)
        assert carry.tobytes() == bytes(carry.nbytes) and not hist.any()
    assert L.vad_snapshot_resample(blob.ctypes.data, len(blob), 2, None, None, None) == 1
    assert all("resample" not in g for g in snapshot_info(blob))


def corrupt(L, sr, what):
    n, _ = GEOMETRY[sr]
    recs = three_records(L, sr)
    blob = make_blob2(sr, recs)
    s1, s2 = stride_of(sr), stride2_of(sr)
    rec0, rec2 = HEADER2, HEADER2 + 2 * s2                         # the two bound records
    tail0, tail2 = rec0 + s1, rec2 + s1
    O, Nr, H = pair(L, RATES[sr][0], sr)
    if what == "a reserved header byte":
        blob[64 + 17] = 1
    elif what == "the last reserved header byte":
        blob[95] = 0x80
    elif what == "a v1 stride under version 2":
        blob[28:32].view("<u4")[:] = s1
    elif what == "a v1 header size under version 2":
        blob[12:16].view("<u4")[:] = 64
    elif what == "version 3":
        blob[8:12].view("<u4")[:] = 3
    elif what == "src_rate not served":
        blob[tail0:tail0 + 4].view("<i4")[:] = 44101
    elif what == "src_rate < 0":
        blob[tail0:tail0 + 4].view("<i4")[:] = -44100
    elif what == "c = N":
        blob[tail0 + 4:tail0 + 8].view("<i4")[:] = n
    elif what == "c < 0":
        blob[tail2 + 4:tail2 + 8].view("<i4")[:] = -1
    elif what == "m = N":                                          # the pair's N: one whole period more than the reduction leaves
        blob[tail0 + 16:tail0 + 24].view("<i8")[:] = Nr
    elif what == "m < 0":
        blob[tail0 + 16:tail0 + 24].view("<i8")[:] = -1
    elif what == "g < 0":
        blob[tail0 + 8:tail0 + 16].view("<i8")[:] = -1
    elif what == "g a period too large":                           # (g + O, m) is what the stream holds BEFORE the reduction
        blob[tail0 + 8:tail0 + 16].view("<i8")[:] += O
    elif what == "g = 2^62":
        blob[tail0 + 8:tail0 + 16].view("<i8")[:] = 2 ** 62
    elif what == "(g, m) inconsistent":
        m = blob[tail0 + 16:tail0 + 24].view("<i8")
        m[:] = (m[0] + 1) % Nr
    elif what == "a bound record with int16 pending":
        blob[rec2 + 16:rec2 + 20].view("<i4")[:] = 1
    elif what == "a sample behind H":
        blob[tail0 + 32 + 4 * n + 2 * H] = 1
    elif what == "the last history sample":
        blob[rec0 + s2 - 1] = 1
    elif what == "a float behind c":
        blob[tail2 + 32:tail2 + 36].view("<f4")[:] = 1.0
    elif what == "-0.0f behind c":
        blob[tail0 + 32 + 4 * n - 1] = 0x80
    elif what == "a reserved info byte":
        blob[tail2 + 24 + 5] = 1
    elif what == "an unbound record with a counter":
        blob[rec0 + s2 + s1 + 8:rec0 + s2 + s1 + 16].view("<i8")[:] = 1
    elif what == "an unbound record with a carry":
        blob[rec0 + s2 + s1 + 32:rec0 + s2 + s1 + 36].view("<f4")[:] = 0.5
    elif what == "an unbound record with a history":
        blob[rec0 + s2 + s1 + 32 + 4 * n] = 1
    elif what == "one byte short":
        blob = blob[:-1].copy()
    elif what == "a v1 field: pending = N":                        # the version 1 part is held against its ranges as before
        blob[rec0 + s2 + 16:rec0 + s2 + 20].view("<i4")[:] = n
    else:
        raise AssertionError(what)
    return blob


@pytest.mark.parametrize("sr", [16000, 8000])
@pytest.mark.parametrize("what", ["a reserved header byte", "the last reserved header byte", "a v1 stride under version 2", "a v1 header size under version 2",
                                  "version 3", "src_rate not served", "src_rate < 0", "c = N", "c < 0", "m = N", "m < 0", "g < 0", "g a period too large",
                                  "g = 2^62", "(g, m) inconsistent", "a bound record with int16 pending", "a sample behind H", "the last history sample",
                                  "a float behind c", "-0.0f behind c", "a reserved info byte", "an unbound record with a counter",
                                  "an unbound record with a carry", "an unbound record with a history", "one byte short", "a v1 field: pending = N"])
def test_each_single_corruption_is_refused(built, sr, what):
    from silero_vad_amd import snapshot_info
    L = _lib().lib()
    good = make_blob2(sr, three_records(L, sr))
    assert inspect(L, good) == (0, 3, sr)
    blob = corrupt(L, sr, what)
    assert len(blob) != len(good) or (blob != good).sum() in range(1, 9)     # one field
    assert inspect(L, blob) == (1, -7, -7)
    assert L.vad_snapshot_stream(blob.ctypes.data, len(blob), 0, None, None, None, None, None) == 1
    assert L.vad_snapshot_resample(blob.ctypes.data, len(blob), 0, None, None, None) == 1
    with pytest.raises(_lib().VadError, match="VAD_ERR_ARG"):
        snapshot_info(blob)


def test_short_buffers_are_refused_without_being_read_past(built):
    L = _lib().lib()
    blob = make_blob2(16000, three_records(L, 16000))
    for nbytes in (0, 1, 63, 64, HEADER2 - 1, HEADER2, HEADER2 + 2 * stride2_of(16000), len(blob) - 1):
        assert inspect(L, blob, nbytes)[0] == 1
    empty = make_blob2(16000, [])
    assert inspect(L, empty) == (0, 0, 16000) and inspect(L, empty, HEADER2 - 1)[0] == 1


@pytest.mark.parametrize("sr,rate", [(16000, 44100), (16000, 24000), (16000, 22050), (16000, 11025), (16000, 48000), (8000, 44100), (8000, 24000),
                                     (8000, 11025)])
def test_what_the_submit_path_can_hold_is_what_the_readers_accept(built, sr, rate):
    """The pump drops the whole periods of the emitted outputs from both counters after every row.  Every (g, m) that leaves is inside
    the documented ranges -- m below the pair's N, ready(g) == m -- and a record that holds it passes; the same inputs one period
    later, unreduced, do not."""
    L = _lib().lib()
    O, Nr, H = pair(L, rate, sr)
    rng = np.random.default_rng(rate)
    g = m = 0
    seen = []
    for _ in range(400):
        length = int(rng.integers(1, 1500))
        m1 = L.vad_resample_stream_ready(rate, sr, g + length)
        assert m1 >= m
        g, m = g + length - m1 // Nr * O, m1 % Nr
        assert 0 <= m < Nr and g >= 0 and L.vad_resample_stream_ready(rate, sr, g) == m
        assert L.vad_resample_stream_ready(rate, sr, g + O) == m + Nr             # the rule is periodic behind the dropped periods
        seen.append((g, m))
    recs = three_records(L, sr)
    recs[0]["history"] = np.concatenate([np.arange(1, H + 1), np.zeros(HISTORY - H)]).astype(np.int16)
    for g, m in seen[::40]:
        recs[0].update(src_rate=rate, inputs_mod=g, outputs_mod=m)
        assert inspect(L, make_blob2(sr, recs))[0] == 0, (g, m)
        recs[0].update(inputs_mod=g + O, outputs_mod=m)               # (ready(g + O) is m + N, asserted above)
        assert inspect(L, make_blob2(sr, recs))[0] == 1, (g, m)
    for g in (0, 1, 2):                                               # a stream younger than the filter's latency: nothing emitted yet
        recs[0].update(src_rate=rate, inputs_mod=g, outputs_mod=L.vad_resample_stream_ready(rate, sr, g))
        assert inspect(L, make_blob2(sr, recs))[0] == 0, g


class Stub:
    """A StreamPump with no pump behind it: the library calls are recorded instead of made."""

    def __init__(self, sr=16000, cap=8):
        from silero_vad_amd import StreamPump

        class Calls:
            def __init__(s):
                s.made = []
                s.vad_pump_snapshot_bytes = _lib().lib().vad_pump_snapshot_bytes
                s.vad_pump_snapshot_bytes_v2 = _lib().lib().vad_pump_snapshot_bytes_v2
                s.vad_pump_last_error = lambda h: b""

            def vad_pump_export_streams(s, h, st, n, blob, cap):
                s.made.append(("export", n, cap))
                return 0

            def vad_pump_export_streams_v2(s, h, st, n, blob, cap):
                s.made.append(("export_v2", n, cap))
                return 0
        self.L = Calls()
        p = StreamPump.__new__(StreamPump)
        p.n, p.streams, p.sr, p._L, p._h = GEOMETRY[sr][0], cap, sr, self.L, None
        self.pump = p


def test_export_streams_takes_a_version(built):
    for bad in (0, 3, "2", 2.0, None, True):
        stub = Stub()
        with pytest.raises(ValueError, match="version"):
            stub.pump.export_streams([0, 1], version=bad)
        assert stub.L.made == []
    stub = Stub()
    with pytest.raises(ValueError):
        stub.pump.export_streams([0, 3, 0], version=2)                                  # a slot twice: as for version 1
    assert stub.L.made == []
    s1, s2 = stride_of(16000), stride2_of(16000)
    assert stub.pump.export_streams([5, 2], version=2).shape == (HEADER2 + 2 * s2,)
    assert stub.pump.export_streams(version=2).shape == (HEADER2 + 8 * s2,)
    assert stub.pump.export_streams([5, 2], version=1).shape == stub.pump.export_streams([5, 2]).shape == (64 + 2 * s1,)
    assert stub.L.made == [("export_v2", 2, HEADER2 + 2 * s2), ("export_v2", 8, HEADER2 + 8 * s2), ("export", 2, 64 + 2 * s1), ("export", 2, 64 + 2 * s1)]


def test_snapshot_info_reads_a_large_blob_as_the_record_readers_do(built):
    """snapshot_info validates a blob once and reads the records itself; the C readers validate the whole blob on every call."""
    from silero_vad_amd import snapshot_info
    L = _lib().lib()
    sr, n = 16000, GEOMETRY[16000][0]
    recs = three_records(L, sr) * 200
    blob = make_blob2(sr, recs)
    got = snapshot_info(blob)
    assert len(got) == 600
    for i in (0, 1, 299, 598, 599):
        f = _lib().StreamInfo()
        h, cc, x, pend = np.empty(128, np.float32), np.empty(128, np.float32), np.empty(n // 8, np.float32), np.empty(n, np.int16)
        assert L.vad_snapshot_stream(blob.ctypes.data, len(blob), i, ctypes.byref(f), h.ctypes.data, cc.ctypes.data, x.ctypes.data, pend.ctypes.data) == 0
        rc, q, carry, hist = read_tail(L, blob, i, sr)
        assert rc == 0 and {k: getattr(f, k) for k in FIELDS} == {k: got[i][k] for k in FIELDS}
        for a, b in ((h, "h"), (cc, "c"), (x, "ctx"), (pend, "pending_samples")):
            assert a.tobytes() == got[i][b].tobytes(), b
        rs = got[i]["resample"]
        assert {k: getattr(q, k) for k in TAIL_FIELDS} == {k: rs[k] for k in TAIL_FIELDS}
        assert carry[:q.pending_out].tobytes() == rs["carry"].tobytes() and np.array_equal(hist[:len(rs["history"])], rs["history"])
        assert not hist[len(rs["history"]):].any()
