"""The Python side of the pump's packet routes on a machine WITHOUT a GPU: the five submit_* methods and the four write_* packers of
StreamPump, driven on a pump with no pump behind it.  The library is a recorder that copies every column out of the pointers it is
handed, the three areas are numpy arrays filled with a sentinel, and every expected column, area image and message below is written
out from the methods' docstrings -- default offsets, silent rows, null pointers, and each refusal with its text."""
import ctypes

import numpy as np
import pytest

SR_OF = {512: 16000, 256: 8000}                          # N -> sample rate
STREAMS, RING, MAX_STEP, RATES = 8, 2, 3, (44100, 24000)
RES_ROW = 1416                                           # ceil(N * 44100 / sr) = ceil(1411.2) = 1412, rounded up to 8: the same at both rates
FILL16, FILL8 = 0x5A5A, 0x5A                             # the sentinel the areas start from
TICK = " (submit a longer one over two ticks)"
ENTRIES = {"vad_pump_submit_packets": False, "vad_pump_submit_coded_packets": True, "vad_pump_submit_burst": True,
           "vad_pump_submit_wide_packets": True, "vad_pump_submit_resampled_packets": True}     # entry -> it takes a fourth column


def column(ptr, n, ctype):
    return None if ptr is None else np.ctypeslib.as_array((ctype * n).from_address(ptr)).copy()


class Recorder:
    """In place of the library: (entry, r, n, (streams, offsets, lengths, fourth column)) of every call, the columns copied while the
    call is in progress -- the arrays behind the pointers are temporaries of the caller."""

    def __init__(self):
        self.made = []
        self.vad_pump_last_error = lambda h: b""
        for name, four in ENTRIES.items():
            setattr(self, name, self.entry(name, four))

    def entry(self, name, four):
        def call(h, r, st, off, ln, *rest):
            c4, n = rest if four else (None,) + rest
            assert h is None and type(r) is int and type(n) is int
            self.made.append((name, r, n, (column(st, n, ctypes.c_int32), column(off, n, ctypes.c_int32), column(ln, n, ctypes.c_int32),
                                           column(c4, n, ctypes.c_uint8))))
            return 0
        return call


class Stub:
    """A StreamPump with no pump behind it, the attributes the packet routes read set by hand."""

    def __init__(self, n):
        from silero_vad_amd import StreamPump
        self.L = Recorder()
        p = StreamPump.__new__(StreamPump)
        p.n, p.streams, p.sr, p.ring_slots, p._L, p._h = n, STREAMS, SR_OF[n], RING, self.L, None
        p.max_burst, p.max_step, p.resample_rates, p.resample_row = 4, MAX_STEP, RATES, RES_ROW
        p._slots = [np.full((STREAMS, n), FILL16, np.int16) for _ in range(RING)]
        p._wide = [np.full(STREAMS * n * MAX_STEP * 2, FILL8, np.uint8) for _ in range(RING)]
        p._res = [np.full(STREAMS * RES_ROW * 2, FILL8, np.uint8) for _ in range(RING)]
        self.pump = p

    def areas(self):
        p = self.pump
        return [a for group in (p._slots, p._wide, p._res) for a in group]

    def untouched(self):
        return all((a.view(np.uint8) == FILL8).all() for a in self.areas())

    def one_call(self, entry, r, streams, offsets, lengths, col4=None):
        """The one recorded call is exactly this one, int32 / uint8 columns included."""
        assert len(self.L.made) == 1
        name, rr, n, cols = self.L.made.pop()
        assert (name, rr, n) == ("vad_pump_submit_" + entry, r, len(streams))
        for got, want, dtype in zip(cols, (streams, offsets, lengths, col4), (np.int32, np.int32, np.int32, np.uint8)):
            if want is None:
                assert got is None
            else:
                assert got.dtype == dtype and got.tolist() == list(want)


@pytest.fixture(params=[512, 256])
def stub(built, request):
    return Stub(request.param)


def samples(k, seed=0):
    return np.random.default_rng(1000 * seed + k).integers(-30000, 30000, k).astype(np.int16)


def codes(k, seed=0):
    return np.random.default_rng(7000 * seed + k).integers(0, 256, k).astype(np.uint8)


def test_the_resample_row_of_the_stub_is_what_set_resample_computes(built):
    from silero_vad_amd import resample_geometry
    for n, sr in SR_OF.items():
        rows = [-(-n * resample_geometry(rate, sr)[0] // resample_geometry(rate, sr)[1]) for rate in RATES]
        assert (max(rows) + 7) // 8 * 8 == RES_ROW


def test_default_offsets(stub):
    p = stub.pump
    st, ln = [0, 1, 2, 3], [160, 1, 512, 7]
    p.submit_packets(0, st, ln)                                       # samples: 160 -> 160, 1 -> 8, 512 -> 512
    stub.one_call("packets", 0, st, [0, 160, 168, 680], ln)
    p.submit_coded_packets(1, st, ln, None)                           # bytes: 320 -> 320, 2 -> 16, 1024 -> 1024
    stub.one_call("coded_packets", 1, st, [0, 320, 336, 1360], ln)
    p.submit_coded_packets(1, st, ln, ["s16"] * 4)
    stub.one_call("coded_packets", 1, st, [0, 320, 336, 1360], ln, [0, 0, 0, 0])
    p.submit_burst(0, st, ln)
    stub.one_call("burst", 0, st, [0, 320, 336, 1360], ln)
    p.submit_burst(0, st, ln, np.zeros(4, np.uint8))
    stub.one_call("burst", 0, st, [0, 320, 336, 1360], ln, [0, 0, 0, 0])
    p.submit_wide_packets(1, st, ln)
    stub.one_call("wide_packets", 1, st, [0, 320, 336, 1360], ln)
    p.submit_wide_packets(1, st, ln, [3, 1, 2, 3])
    stub.one_call("wide_packets", 1, st, [0, 320, 336, 1360], ln, [3, 1, 2, 3])
    p.submit_resampled_packets(0, st, ln)
    stub.one_call("resampled_packets", 0, st, [0, 320, 336, 1360], ln)
    p.submit_resampled_packets(0, st, ln, [1, 0, 0, 1])
    stub.one_call("resampled_packets", 0, st, [0, 320, 336, 1360], ln, [1, 0, 0, 1])
    # G.711 rows take 1 byte a sample, s16 rows 2: 160, 320, 1 -> 16, 16, (34 -> 48)
    st, ln = [4, 5, 6, 7, 0], [160, 160, 1, 16, 17]
    for cd in (["ulaw", "s16", "alaw", "ulaw", "s16"], [1, 0, 2, 1, 0]):
        p.submit_coded_packets(0, st, ln, cd)
        stub.one_call("coded_packets", 0, st, [0, 160, 480, 496, 512], ln, [1, 0, 2, 1, 0])
        p.submit_burst(1, st, ln, cd)
        stub.one_call("burst", 1, st, [0, 160, 480, 496, 512], ln, [1, 0, 2, 1, 0])
    p.submit_packets(0, [5], [9])
    stub.one_call("packets", 0, [5], [0], [9])
    assert stub.untouched()


def test_explicit_offsets_go_to_the_library_as_given(stub):
    p = stub.pump
    p.submit_packets(1, np.array([2, 0, 1], np.int64), (5, 40, 6), [8, -1, 0])
    stub.one_call("packets", 1, [2, 0, 1], [8, -1, 0], [5, 40, 6])
    p.submit_coded_packets(0, [2, 0], [5, 40], ["alaw", "ulaw"], [16, -1])
    stub.one_call("coded_packets", 0, [2, 0], [16, -1], [5, 40], [2, 1])
    p.submit_coded_packets(0, [2], [5], [7], [16])                  # a codec number goes to the pump as it is
    stub.one_call("coded_packets", 0, [2], [16], [5], [7])
    p.submit_burst(1, [1, 1], [700, 3], byte_offsets=[32, 0])
    stub.one_call("burst", 1, [1, 1], [32, 0], [700, 3])
    p.submit_wide_packets(0, [3], [30], [2], [-1])
    stub.one_call("wide_packets", 0, [3], [-1], [30], [2])
    p.submit_resampled_packets(1, [3], [441], None, [160])
    stub.one_call("resampled_packets", 1, [3], [160], [441])


def test_zero_rows_arrive_as_null_pointers(stub):
    p = stub.pump
    e = np.zeros(0, np.int32)
    for call, entry in ((lambda: p.submit_packets(1, [], []), "packets"), (lambda: p.submit_packets(1, e, e, e), "packets"),
                        (lambda: p.submit_coded_packets(1, [], [], None), "coded_packets"),
                        (lambda: p.submit_coded_packets(1, e, e, np.zeros(0, np.uint8), e), "coded_packets"),
                        (lambda: p.submit_burst(1, [], []), "burst"), (lambda: p.submit_burst(1, e, e, e, e), "burst"),
                        (lambda: p.submit_wide_packets(1, [], []), "wide_packets"), (lambda: p.submit_wide_packets(1, e, e, e, e), "wide_packets"),
                        (lambda: p.submit_resampled_packets(1, [], []), "resampled_packets"),
                        (lambda: p.submit_resampled_packets(1, e, e, e, e), "resampled_packets"),
                        (lambda: p.write_packets(1, []), "packets"), (lambda: p.write_coded_packets(1, iter(())), "coded_packets"),
                        (lambda: p.write_burst(1, []), "burst"), (lambda: p.write_resampled_packets(1, []), "resampled_packets")):
        call()
        assert stub.L.made == [("vad_pump_submit_" + entry, 1, 0, (None, None, None, None))]
        stub.L.made.clear()
    assert stub.untouched()


def test_a_left_out_fourth_column_arrives_as_a_null_pointer(stub):
    p = stub.pump
    p.submit_coded_packets(0, [1], [5], None)
    stub.one_call("coded_packets", 0, [1], [0], [5], None)
    p.submit_burst(0, [1, 1], [5, 9], byte_offsets=[0, -1])
    stub.one_call("burst", 0, [1, 1], [0, -1], [5, 9], None)
    p.submit_wide_packets(0, [1], [5])
    stub.one_call("wide_packets", 0, [1], [0], [5], None)
    p.submit_resampled_packets(0, [1], [5], byte_offsets=[16])
    stub.one_call("resampled_packets", 0, [1], [16], [5], None)


def test_write_packets_packs_rows_rounded_up_to_8_samples(stub):
    p, n = stub.pump, stub.pump.n
    a, b, c, d = samples(160), samples(1), samples(n), samples(7)
    p.write_packets(1, [(3, a), (5, 40), (0, b), (7, c), (2, d), (6, n)])
    # a silent row: offset -1, its length in the length column, no room in the area and no move of the cursor
    stub.one_call("packets", 1, [3, 5, 0, 7, 2, 6], [0, -1, 160, 168, 168 + n, -1], [160, 40, 1, n, 7, n])
    want = np.full(STREAMS * n, FILL16, np.int16)
    want[0:160], want[160:161], want[168:168 + n], want[168 + n:175 + n] = a, b, c, d
    assert np.array_equal(p.packet_area(1), want)
    p._slots[1][:] = FILL16
    assert stub.untouched()
    p.write_packets(0, ((s, samples(n, s)) for s in range(STREAMS)))       # the area holds exactly `streams` full packets
    stub.one_call("packets", 0, range(STREAMS), [s * n for s in range(STREAMS)], [n] * STREAMS)
    assert np.array_equal(p.slot(0), np.stack([samples(n, s) for s in range(STREAMS)]))


def test_write_coded_packets_packs_rows_rounded_up_to_16_bytes(stub):
    p, n = stub.pump, stub.pump.n
    a, b, c, d = codes(160), samples(5), codes(3), samples(n)
    p.write_coded_packets(0, [(1, a, "ulaw"), (2, 33, "alaw"), (4, b, "s16"), (6, c, 2), (0, d, 0), (5, n, np.int64(1))])
    # 160 bytes -> 160, 10 -> 16, 3 -> 16; the silent rows keep the codec they were given
    stub.one_call("coded_packets", 0, [1, 2, 4, 6, 0, 5], [0, -1, 160, 176, 192, -1], [160, 33, 5, 3, n, n], [1, 2, 0, 2, 0, 1])
    want = np.full(STREAMS * n * 2, FILL8, np.uint8)
    want[0:160], want[160:170], want[176:179], want[192:192 + 2 * n] = a, b.view(np.uint8), c, d.view(np.uint8)
    assert np.array_equal(p.packet_bytes(0), want)
    p._slots[0][:] = FILL16
    assert stub.untouched()


def test_write_burst_packs_rows_of_any_length(stub):
    p, n = stub.pump, stub.pump.n
    a, b, c = samples(n + 9), codes(17), samples(1)
    p.write_burst(1, [(1, a), (1, 3 * n + 5), (2, b, "ulaw"), (1, c, "s16"), (2, 7, "alaw")])
    at = (2 * (n + 9) + 15) // 16 * 16                                # a row longer than N is accepted; the codec defaults to "s16"
    assert at == {512: 1056, 256: 544}[n]
    stub.one_call("burst", 1, [1, 1, 2, 1, 2], [0, -1, at, at + 32, -1], [n + 9, 3 * n + 5, 17, 1, 7], [0, 0, 1, 0, 2])
    want = np.full(STREAMS * n * 2, FILL8, np.uint8)
    want[0:2 * (n + 9)], want[at:at + 17], want[at + 32:at + 34] = a.view(np.uint8), b, c.view(np.uint8)
    assert np.array_equal(p.packet_bytes(1), want)
    p._slots[1][:] = FILL16
    assert stub.untouched()


def test_write_resampled_packets_packs_rows_rounded_up_to_16_bytes(stub):
    p = stub.pump
    a, b, c = samples(441), samples(240), samples(RES_ROW)
    p.write_resampled_packets(1, [(0, a, 44100), (3, b), (5, 441, 24000), (2, c, 24000), (7, RES_ROW)])
    # 882 bytes -> 896, 480 -> 480; a row without a rate is at resample_rates[0]; the rates go out as indices
    stub.one_call("resampled_packets", 1, [0, 3, 5, 2, 7], [0, 896, -1, 1376, -1], [441, 240, 441, RES_ROW, RES_ROW], [0, 0, 1, 1, 0])
    want = np.full(STREAMS * RES_ROW * 2, FILL8, np.uint8)
    want[0:882], want[896:1376], want[1376:1376 + 2 * RES_ROW] = a.view(np.uint8), b.view(np.uint8), c.view(np.uint8)
    assert np.array_equal(p.resample_slot(1), want)
    p._res[1][:] = FILL8
    assert stub.untouched()


NOT_A_ROW = "a packet is a 1-D sample array, or an int >= 1 for a silent row of that many samples, got {!r}"
NO_SAMPLE = "a silent row holds at least 1 sample, got {!r}"
WRITERS = {"write_packets": lambda s, x: (s, x), "write_coded_packets": lambda s, x: (s, x, "s16"), "write_burst": lambda s, x: (s, x),
           "write_resampled_packets": lambda s, x: (s, x, 24000)}


@pytest.mark.parametrize("writer", sorted(WRITERS))
def test_a_bad_silent_row_is_refused_before_a_byte_is_written(stub, writer):
    p, row = stub.pump, WRITERS[writer]
    for bad, text in ((True, NOT_A_ROW), (np.True_, NOT_A_ROW), (2.0, NOT_A_ROW), (np.float32(3), NOT_A_ROW), (0, NO_SAMPLE), (-3, NO_SAMPLE)):
        with pytest.raises(ValueError) as e:
            getattr(p, writer)(0, [row(1, samples(20)), row(2, bad)])
        assert str(e.value) == text.format(bad)
        assert stub.L.made == [] and stub.untouched()


def test_first_pass_refusals_leave_the_area_untouched(stub):
    p, n = stub.pump, stub.pump.n
    good = samples(20)
    too_long = f"a packet holds 1 ... {n} samples, got {n + 1}" + TICK
    for call, text in ((lambda: p.write_packets(0, [(1, good), (2, n + 1)]), too_long),
                       (lambda: p.write_coded_packets(0, [(1, good, "s16"), (2, n + 1, "ulaw")]), too_long),
                       (lambda: p.write_resampled_packets(0, [(1, good), (2, RES_ROW + 1)]), f"a row holds 1 ... {RES_ROW} samples, got {RES_ROW + 1}" + TICK),
                       (lambda: p.write_resampled_packets(0, [(1, good), (2, good, 48000)]),
                        "rate 48000 is none of the pump's resample_rates (44100, 24000)"),
                       (lambda: p.write_resampled_packets(0, [(1, good), (2, 10, 1)]), "rate 1 is none of the pump's resample_rates (44100, 24000)")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
        assert stub.L.made == [] and stub.untouched()


def test_second_pass_refusals_keep_the_earlier_rows_and_make_no_call(stub):
    p, n = stub.pump, stub.pump.n
    good, good8 = samples(20), codes(20)
    codec_names = "codec must be one of ['alaw', 's16', 'ulaw']"
    cases = (
        ("write_packets", (1, good), (2, samples(6).reshape(2, 3)), "a packet must be a 1-D int16 array"),
        ("write_packets", (1, good), (2, good.astype(np.float32)), "a packet must be a 1-D int16 array"),
        ("write_packets", (1, good), (2, good8), "a packet must be a 1-D int16 array"),
        ("write_packets", (1, good), (2, samples(n + 1)), f"a packet holds 1 ... {n} samples, got {n + 1}" + TICK),
        ("write_packets", (1, good), (2, samples(0)), f"a packet holds 1 ... {n} samples, got 0" + TICK),
        ("write_coded_packets", (1, good, "s16"), (2, codes(6).reshape(2, 3), "ulaw"), "a 'ulaw' packet must be a 1-D uint8 array, got uint8 of shape (2, 3)"),
        ("write_coded_packets", (1, good, "s16"), (2, codes(4), "s16"), "a 's16' packet must be a 1-D int16 array, got uint8 of shape (4,)"),
        ("write_coded_packets", (1, good, "s16"), (2, samples(4), 2), "a 2 packet must be a 1-D uint8 array, got int16 of shape (4,)"),
        ("write_coded_packets", (1, good, "s16"), (2, codes(n + 1), "alaw"), f"a packet holds 1 ... {n} samples, got {n + 1}" + TICK),
        ("write_coded_packets", (1, good, "s16"), (2, codes(0), "alaw"), f"a packet holds 1 ... {n} samples, got 0" + TICK),
        ("write_coded_packets", (1, good, "s16"), (2, codes(4), "opus"), codec_names + ", got 'opus'"),
        ("write_coded_packets", (1, good, "s16"), (2, 30, "opus"), codec_names + ", got 'opus'"),
        ("write_coded_packets", (1, good, "s16"), (2, codes(4), 7), codec_names + " or [0, 1, 2], got 7"),
        ("write_coded_packets", (1, good, "s16"), (2, codes(4), 1.0), codec_names + " or [0, 1, 2], got 1.0"),
        ("write_burst", (1, good), (2, samples(6).reshape(3, 2)), "a 's16' packet must be a 1-D int16 array, got int16 of shape (3, 2)"),
        ("write_burst", (1, good), (2, samples(4), "ulaw"), "a 'ulaw' packet must be a 1-D uint8 array, got int16 of shape (4,)"),
        ("write_burst", (1, good), (2, samples(0)), "a packet holds at least 1 sample"),
        ("write_burst", (1, good), (2, codes(4), "g722"), codec_names + ", got 'g722'"),
        ("write_burst", (1, good), (2, codes(4), 3), codec_names + " or [0, 1, 2], got 3"),
        ("write_resampled_packets", (1, good), (2, samples(6).reshape(2, 3), 24000), "a row must be a 1-D int16 array"),
        ("write_resampled_packets", (1, good), (2, good8, 24000), "a row must be a 1-D int16 array"),
        ("write_resampled_packets", (1, good), (2, samples(RES_ROW + 1)), f"a row holds 1 ... {RES_ROW} samples, got {RES_ROW + 1}" + TICK),
        ("write_resampled_packets", (1, good), (2, samples(0)), f"a row holds 1 ... {RES_ROW} samples, got 0" + TICK),
    )
    for writer, first, bad, text in cases:
        with pytest.raises(ValueError) as e:
            getattr(p, writer)(1, [first, bad])
        assert str(e.value) == text, writer
        assert stub.L.made == []
        area = p.resample_slot(1) if writer == "write_resampled_packets" else p.packet_bytes(1)
        assert np.array_equal(area[:40], good.view(np.uint8)) and (area[40:] == FILL8).all()       # the first row stays where it was put
        area[:40] = FILL8
        assert stub.untouched()


def test_rows_that_do_not_fit_are_refused(stub):
    p, n = stub.pump, stub.pump.n
    full = [(s, samples(n)) for s in range(STREAMS)]
    res_full = [(s, samples(RES_ROW)) for s in range(STREAMS)]
    for call, text in ((lambda: p.write_packets(0, full + [(0, samples(1))]), "the packets do not fit into the slot"),
                       (lambda: p.write_coded_packets(0, [(s, x, "s16") for s, x in full] + [(0, codes(1), "ulaw")]), "the packets do not fit into the slot"),
                       (lambda: p.write_burst(0, [(0, samples(STREAMS * n + 1))]), "the packets do not fit into the slot"),
                       (lambda: p.write_burst(0, [(0, samples(STREAMS * n - 1)), (1, codes(1), "alaw")]), "the packets do not fit into the slot"),
                       (lambda: p.write_resampled_packets(0, res_full + [(0, samples(1))]), "the rows do not fit into the slot")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
        assert stub.L.made == []
    p.write_burst(1, [(0, samples(STREAMS * n))])                     # one row may fill the area, N or not
    stub.one_call("burst", 1, [0], [0], [STREAMS * n], [0])
    p.write_burst(1, full + [(3, 9 * n)])                             # and a silent row needs no room
    stub.one_call("burst", 1, list(range(STREAMS)) + [3], [2 * n * s for s in range(STREAMS)] + [-1], [n] * STREAMS + [9 * n], [0] * (STREAMS + 1))


def submitters(p):
    """(method, the name of its offset argument, its fourth column or None, the word of its count message), streams and lengths bound later."""
    return (("submit_packets", "offsets", None, "packet", lambda st, ln, c4, off: p.submit_packets(0, st, ln, off)),
            ("submit_coded_packets", "byte_offsets", "codecs", "packet", lambda st, ln, c4, off: p.submit_coded_packets(0, st, ln, c4, off)),
            ("submit_burst", "byte_offsets", "codecs", "row", lambda st, ln, c4, off: p.submit_burst(0, st, ln, c4, off)),
            ("submit_wide_packets", "byte_offsets", "steps", "row", lambda st, ln, c4, off: p.submit_wide_packets(0, st, ln, c4, off)),
            ("submit_resampled_packets", "byte_offsets", "rates", "row", lambda st, ln, c4, off: p.submit_resampled_packets(0, st, ln, c4, off)))


def test_columns_of_different_lengths_are_refused(stub):
    for name, off_name, col4, per, call in submitters(stub.pump):
        head = f"streams, lengths, {col4} and {off_name}" if col4 else f"streams, lengths and {off_name}"
        head += f" must have one entry per {per}, got "
        # (streams, lengths, fourth column, offsets) -> the counts in the message: a column left out counts as len(streams)
        cases = [(([0, 1], [5], None, None), (2, 1, 2, 2)), (([0, 1], [5, 5], None, [0, 16, 32]), (2, 2, 2, 3)),
                 (([], [5], None, None), (0, 1, 0, 0)), (([0, 1], [5, 5, 5], None, [0]), (2, 3, 2, 1))]
        if col4:
            cases += [(([0, 1], [5, 5], [1], None), (2, 2, 1, 2)), (([0, 1], [5, 5], [1, 1, 1], [0, 16]), (2, 2, 3, 2)),
                      (([0], [5], [], [0]), (1, 1, 0, 1))]
        for args, counts in cases:
            if not col4:
                counts = counts[:2] + counts[3:]
            with pytest.raises(ValueError) as e:
                call(*args)
            assert str(e.value) == head + ", ".join(map(str, counts)), name
            assert stub.L.made == []
    assert stub.untouched()


def test_columns_that_are_not_int32_or_uint8_rows_are_refused(stub):
    p = stub.pump
    int32 = "{} must be a 1-D sequence of int32 values, got {}"
    for name, off_name, col4, per, call in submitters(p):
        for args, text in ((([2 ** 31], [5], None, None), int32.format("streams", "int64 of shape (1,)")),
                           (([-2 ** 31 - 1], [5], None, None), int32.format("streams", "int64 of shape (1,)")),
                           (([[0]], [5], None, None), int32.format("streams", "int64 of shape (1, 1)")),
                           (([0], [5.0], None, None), int32.format("lengths", "float64 of shape (1,)")),
                           (([0], 5, None, None), int32.format("lengths", "int64 of shape ()")),
                           (([0], [5], None, [2 ** 31]), int32.format(off_name, "int64 of shape (1,)")),
                           (([0], [5], None, [0.0]), int32.format(off_name, "float64 of shape (1,)"))):
            with pytest.raises(ValueError) as e:
                call(*args)
            assert str(e.value) == text, name
            assert stub.L.made == []
        call([2 ** 31 - 1], [-2 ** 31], None, [2 ** 31 - 1])              # the ends of int32 are int32: the pump is the one to refuse them
        stub.one_call(name[len("submit_"):], 0, [2 ** 31 - 1], [2 ** 31 - 1], [-2 ** 31])
    uint8 = {"steps": "steps must be a 1-D sequence of uint8 values, got {}", "rates": "rates must be a 1-D sequence of rate indices (uint8 values), got {}"}
    for col4, method in (("steps", p.submit_wide_packets), ("rates", p.submit_resampled_packets)):
        for bad, got in (([256], "int64 of shape (1,)"), ([-1], "int64 of shape (1,)"), ([1.0], "float64 of shape (1,)"), ([[1]], "int64 of shape (1, 1)")):
            with pytest.raises(ValueError) as e:
                method(0, [0], [5], bad)
            assert str(e.value) == uint8[col4].format(got)
            assert stub.L.made == []
        method(0, [0], [5], [255])
        stub.one_call(method.__name__[len("submit_"):], 0, [0], [0], [5], [255])
    for method in (p.submit_coded_packets, p.submit_burst):
        for bad, text in (([256], "codecs must be names or uint8 values, got int64"), ([0.0], "codecs must be names or uint8 values, got float64"),
                          ([[0]], "codecs must be a 1-D sequence, got shape (1, 1)"), (["s16", "opus"], "codec must be one of ['alaw', 's16', 'ulaw'], got 'opus'")):
            with pytest.raises(ValueError) as e:
                method(0, [0] * len(bad), [5] * len(bad), bad)
            assert str(e.value) == text
            assert stub.L.made == []
    assert stub.untouched()


def test_areas_that_are_not_enabled(stub):
    p = stub.pump
    for absent in (lambda: setattr(p, "_wide", None) or setattr(p, "_res", None), lambda: delattr(p, "_wide") or delattr(p, "_res")):
        absent()
        with pytest.raises(ValueError, match=r"^wideband is not enabled on this pump \(set_wideband\)$"):
            p.wide_slot(0)
        for call in (lambda: p.resample_slot(0), lambda: p.write_resampled_packets(0, [(1, samples(20))])):
            with pytest.raises(ValueError, match=r"^resampled rows are not enabled on this pump \(set_resample\)$"):
                call()
    assert stub.L.made == []
    assert p.packet_area(1).shape == (STREAMS * p.n,) and p.packet_area(1).dtype == np.int16
    assert p.packet_bytes(1).shape == (STREAMS * p.n * 2,) and p.packet_bytes(1).dtype == np.uint8
