"""The audio a segment list keeps, on the host: vad_collect_segments (the host twin of the device gather, csrc/collector.hpp) against
`collect_chunks` / `drop_chunks` on numpy slices, bit for bit, and the argument checks of both entry points -- the device one on a
host-only engine, where no launch can follow.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

N = 1000                                  # 16 kHz samples of the test signal


def signal(dtype, step):
    """N * step raw-rate samples, every one distinguishable: int16 values, or float32 made of distinct bit patterns (NaNs among them:
    a copy must not look at the values)."""
    rng = np.random.default_rng(5 + step)
    if dtype == np.int16:
        return rng.integers(-32768, 32768, size=N * step).astype(np.int16)
    bits = rng.permutation(np.arange(1 << 20, dtype=np.uint32))[:N * step] * np.uint32(4093) + np.uint32(0x7F800000)
    assert len(np.unique(bits)) == N * step
    return bits.view(np.float32)


def numpy_reference(segs, twin, invert):
    from silero_vad_amd import collect_chunks, drop_chunks
    tss = [{"start": int(a), "end": int(b)} for a, b in segs]
    t = torch.from_numpy(twin.view(np.int16 if twin.dtype == np.int16 else np.int32))
    if invert:
        return drop_chunks(tss, t).numpy()
    return collect_chunks(tss, t).numpy() if tss else np.empty(0, t.numpy().dtype)


def call(L, raw, step, alen, segs, invert, out, cap):
    sg = np.ascontiguousarray(segs, dtype=np.int64).reshape(-1, 2)
    return L.vad_collect_segments(raw.ctypes.data if raw.size else None, raw.itemsize, step, alen, sg.ctypes.data if len(sg) else None, len(sg),
                                  invert, out.ctypes.data if out is not None else None, cap)


CASES = {
    "none": [],
    "at_zero": [(0, 130)],
    "to_the_end": [(700, N)],
    "past_the_end": [(10, 20), (900, N + 77)],
    "empty_segment": [(5, 9), (300, 300), (400, 417)],
    "several": [(1, 2), (3, 10), (10, 18), (19, 500), (777, 999)],
    "whole": [(0, N)],
}


@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["i16", "f32"])
@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("invert", [0, 1])
def test_host_twin_against_numpy(built, dtype, step, invert):
    from silero_vad_amd import _lib
    L = _lib.lib()
    raw = signal(dtype, step)
    twin = np.ascontiguousarray(raw[::step])
    bits = np.int16 if dtype == np.int16 else np.int32
    for name, segs in CASES.items():
        want = numpy_reference(segs, twin, invert)
        need = call(L, raw, step, N, segs, invert, None, 0)                     # out == NULL: the size
        assert need == len(want), name
        got = np.full(need + 8, 0x5A, dtype=bits).view(dtype)
        assert call(L, raw, step, N, segs, invert, got, need) == need, name
        assert np.array_equal(got[:need].view(bits), want), name
        assert (got[need:].view(bits) == 0x5A).all(), name                      # nothing behind the kept samples
        if need:                                                                # cap too small: the size, and nothing written
            got = np.full(need, 0x5A, dtype=bits).view(dtype)
            assert call(L, raw, step, N, segs, invert, got, need - 1) == need, name
            assert (got.view(bits) == 0x5A).all(), name
    # audio_len 0: nothing to keep either way, whatever the segments say
    for segs in ([], [(0, 10)]):
        assert call(L, raw, step, 0, segs, invert, None, 0) == 0
    # a shorter audio_len clamps the segments and ends the inverted output
    want = numpy_reference([(10, 20), (400, 600)], twin[:500], invert)
    got = np.empty(len(want), dtype)
    assert call(L, raw, step, 500, [(10, 20), (400, 600)], invert, got, len(got)) == len(want)
    assert np.array_equal(got.view(bits), want)


def test_a_segment_that_ends_before_it_starts_is_empty(built):
    from silero_vad_amd import _lib
    L = _lib.lib()
    raw = signal(np.int16, 1)
    want = numpy_reference([(50, 40), (100, 110)], raw, 0)                       # numpy: x[50:40] is empty
    got = np.empty(len(want), np.int16)
    assert call(L, raw, 1, N, [(50, 40), (100, 110)], 0, got, len(got)) == 10 == len(want)
    assert np.array_equal(got, want)
    # inverted, such a segment ends where it starts: every sample outside the proper segments once
    got = np.empty(N - 10, np.int16)
    assert call(L, raw, 1, N, [(50, 40), (100, 110)], 1, got, len(got)) == N - 10
    assert np.array_equal(got, np.concatenate([raw[:100], raw[110:]]))


def test_host_twin_refuses_bad_arguments(built):
    from silero_vad_amd import _lib
    L = _lib.lib()
    raw = signal(np.int16, 1)
    sg = np.array([[0, 10]], dtype=np.int64)
    out = np.empty(16, np.int16)
    ok = dict(pcm=raw.ctypes.data, esz=2, step=1, alen=N, segs=sg.ctypes.data, n=1, inv=0, out=out.ctypes.data, cap=16)

    def run(**kw):
        a = dict(ok, **kw)
        return L.vad_collect_segments(a["pcm"], a["esz"], a["step"], a["alen"], a["segs"], a["n"], a["inv"], a["out"], a["cap"])

    assert run() == 10
    for bad in (dict(esz=1), dict(esz=3), dict(esz=8), dict(step=0), dict(step=4), dict(step=-1), dict(alen=-1), dict(n=-1), dict(cap=-1),
                dict(inv=2), dict(segs=None), dict(pcm=None)):
        assert run(**bad) == -1, bad                                            # -VAD_ERR_ARG
    assert run(segs=None, n=0) == 0 and run(pcm=None, out=None) == 10           # (nothing to read there)


def test_device_entry_checks_its_arguments_and_needs_a_device(built):
    """On a host-only engine: every malformed call is refused for what is wrong with it (VAD_ERR_ARG and its text), a well-formed one
    because there is no device (VAD_ERR_NO_DEVICE) -- before any launch either way."""
    from silero_vad_amd import _lib
    L = _lib.lib()
    good = _lib.WEIGHTS_PATH.read_bytes()
    h = ctypes.c_void_p()
    assert L.vad_create_host_only(good, len(good), ctypes.byref(h)) == 0
    P = 0x10000                                                                  # stands for device memory: never dereferenced here
    ok = dict(pcm=P, esz=2, ld=512, step=1, n=4, alen=P, segs=P, cap=24, counts=P, inv=0, kept=P, offs=P, out=P)

    def run(**kw):
        a = dict(ok, **kw)
        return L.vad_collect_segments_device(h, a["pcm"], a["esz"], a["ld"], a["step"], a["n"], a["alen"], a["segs"], a["cap"], a["counts"],
                                             a["inv"], a["kept"], a["offs"], a["out"], None)

    for bad, text in ((dict(esz=1), b"elem_size"), (dict(esz=8), b"elem_size"), (dict(step=0), b"step"), (dict(step=4), b"step"),
                      (dict(inv=2), b"invert"), (dict(ld=-1), b"negative"), (dict(n=-1), b"negative"), (dict(cap=-1), b"negative"),
                      (dict(cap=513), b"cap_per_stream"), (dict(alen=None), b"null"), (dict(counts=None), b"null"),
                      (dict(kept=None), b"null"), (dict(segs=None), b"null"), (dict(pcm=None), b"null pcm"), (dict(offs=None), b"out_offset"),
                      (dict(pcm=P + 1), b"aligned"), (dict(esz=4, pcm=P + 2), b"aligned"), (dict(out=P + 8), b"16-byte")):
        assert run(**bad) == 1, bad                                             # VAD_ERR_ARG
        err = L.vad_last_error(h)
        assert b"vad_collect_segments_device" in err and text in err, (bad, err)
    for fine in (dict(), dict(out=None, pcm=None, offs=None), dict(esz=4, step=3, inv=1), dict(n=0, alen=None, counts=None, kept=None)):
        assert run(**fine) == 4, fine                                           # VAD_ERR_NO_DEVICE
        assert b"host-only" in L.vad_last_error(h)
    assert L.vad_collect_segments_device(None, P, 2, 512, 1, 4, P, P, 24, P, 0, P, P, P, None) == 1
    L.vad_destroy(h)


def test_python_surface(built):
    import silero_vad_amd
    assert callable(silero_vad_amd.ragged_speech_audio) and callable(silero_vad_amd.collect_chunks_device)
    with pytest.raises(ValueError, match="keep"):
        silero_vad_amd.ragged_speech_audio([], None, keep="both")
    with pytest.raises(ValueError, match="CUDA"):
        z = torch.zeros(0, dtype=torch.int64)
        silero_vad_amd.collect_chunks_device(None, torch.zeros((2, 8), dtype=torch.int16), z, z, z)
