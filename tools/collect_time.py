#!/usr/bin/env python3
"""What collecting the speech costs (profiles/collect_chunks.md).  One GPU process at a time; three modes:

    python tools/collect_time.py kernel [rows]
        the gather alone (vad_collect_segments_device, csrc/kernel_collect.hip) on a resident int16 batch of about a corpus bucket's
        size -- `rows` (default 256) recordings of 30 s cut from the speech fixture, segment tables from the device scan of the net's
        own probabilities -- beside a plain device-to-device hipMemcpyAsync of the same number of bytes, in bytes read plus bytes
        written per second; the same for a 48 kHz batch (step 3, the element-wise path), as information.
    python tools/collect_time.py corpus audio|segments [recordings] [reps] [--root TREE]
        ONE way in a fresh process: `ragged_speech_audio` (host output) or `ragged_speech_segments` over the same page-locked arena of
        recordings of 20-40 s cut from the fixture, warmed up and reserved first, `reps` timed runs.  --root: import the package from
        another checkout (the parent commit's, for the comparison).  The driver alternates the two.

Each prints one JSON line."""
import ctypes
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if "--root" in sys.argv:
    k = sys.argv.index("--root")
    sys.path.insert(0, str(Path(sys.argv[k + 1]).resolve()))
    del sys.argv[k:k + 2]
else:
    sys.path.insert(0, str(ROOT))
SR, N = 16000, 512


def speech_page():
    import numpy as np
    pcm = np.load(ROOT / "tests" / "golden" / "audio_16k.npz")["pcm"]
    return np.concatenate([pcm, pcm])                                    # 120 s: a 40 s cut fits wherever it starts in the first 60


def timed(fn, reps=6):
    import torch
    ms = []
    for k in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if k:                                                            # (the first launch loads the code object)
            ms.append(e0.elapsed_time(e1))
    return min(ms), sorted(ms)[len(ms) // 2]


def kernel(rows):
    import numpy as np
    import torch
    from silero_vad_amd import _lib, load_silero_vad
    from silero_vad_amd import streams as S
    dev = torch.device("cuda", 0)
    model = load_silero_vad(device=0)
    L, eng = _lib.lib(), model.engine
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    page = speech_page()
    rng = np.random.default_rng(3)
    width = 30 * SR
    host = np.stack([page[a:a + width] for a in rng.integers(0, len(page) - width, size=rows)])
    out = {"rows": rows, "row_samples": width}
    for step in (1, 3):
        x = torch.from_numpy(host if step == 1 else np.repeat(host[:rows // 3], 3, axis=1)).to(dev)
        B = x.shape[0]
        probs = model.audio_forward_device(x, SR * step)
        T = probs.shape[1]
        alen = torch.full((B,), width, dtype=torch.int64, device=dev)
        nck = torch.full((B,), T, dtype=torch.int64, device=dev)
        counts, segs = S._device_scan(eng, probs, nck, alen, S._segment_params(SR), 64)
        assert int(counts.max()) <= 64
        res = {"batch_MB": round(x.numel() * 2 / 1e6, 1), "segments_per_row": round(float(counts.float().mean()), 1)}
        for invert in (0, 1):
            o, offs, kept = S.collect_chunks_device(eng, x, segs, counts, alen, step=step, invert=bool(invert))
            torch.cuda.synchronize()
            nbytes = int(kept.clamp(min=0).sum()) * 2
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

            def phase(out_ptr):
                _lib.check(eng._h, L.vad_collect_segments_device(eng._h, x.data_ptr(), 2, x.stride(0), step, B, alen.data_ptr(), segs.data_ptr(),
                                                                 segs.shape[1], counts.data_ptr(), invert, kept.data_ptr(), offs.data_ptr(),
                                                                 out_ptr, st))

            g_ms, g_med = timed(lambda: phase(o.data_ptr()))
            c_ms, _ = timed(lambda: phase(None))
            src = x.view(-1)[:nbytes // 2]
            dst = torch.empty_like(src)
            m_ms, m_med = timed(lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, st))      # 3: device to device
            res["drop" if invert else "collect"] = {
                "kept_MB": round(nbytes / 1e6, 1), "gather_ms": round(g_ms, 4), "gather_ms_median": round(g_med, 4), "count_ms": round(c_ms, 4),
                "gather_GBps_read_plus_written": round(2 * nbytes / g_ms / 1e6, 1), "memcpy_d2d_ms": round(m_ms, 4),
                "memcpy_d2d_ms_median": round(m_med, 4), "memcpy_GBps_read_plus_written": round(2 * nbytes / m_ms / 1e6, 1),
                "gather_over_memcpy_time": round(g_ms / m_ms, 2)}
            del o, dst
        out[f"step{step}"] = res
        del x, probs
    print(json.dumps(out))


def corpus(way, nrec, reps):
    import numpy as np
    import torch
    import silero_vad_amd
    from silero_vad_amd import PackedRecordings, load_silero_vad, ragged_speech_segments
    from silero_vad_amd import streams as S
    dev = torch.device("cuda", 0)
    model = load_silero_vad(device=0)
    page = speech_page()
    rng = np.random.default_rng(7)
    lens = rng.integers(20 * SR, 40 * SR, size=nrec).astype(np.int64)
    cut = rng.integers(0, len(page) - 40 * SR, size=nrec)
    step = (lens + 7) // 8 * 8
    offs = np.concatenate([[0], np.cumsum(step)[:-1]]).astype(np.int64)
    base = torch.empty(int(step.sum()) + 16, dtype=torch.int16, pin_memory=True)
    b = base.numpy()
    for o, c, m in zip(offs, cut, lens):
        b[o:o + m] = page[c:c + m]
    rec = PackedRecordings(base, offs, lens)
    kw = dict(max_waste=0.1, max_bytes=256 << 20, as_arrays=True)
    call = ragged_speech_segments if way == "segments" else silero_vad_amd.ragged_speech_audio

    def one(m):
        return call(PackedRecordings(base, offs[:m], lens[:m]), model, SR, **kw)

    one(min(nrec, 256))
    S.ragged_reserve(rec, model, SR, max_waste=0.1, max_bytes=256 << 20)
    one(nrec)                                                            # (the allocator's blocks for the packed outputs, the pinned buffers)
    chunks = int(((lens + N - 1) // N).sum())
    runs, res, segments, audio = [], None, None, None
    for _ in range(reps):
        S.STATS.clear()
        trace = None
        if way == "audio":
            trace = S.AUDIO_TRACE = []
        res = segments = audio = None                                    # (its pinned buffers go back to torch's host allocator: a run
        torch.cuda.synchronize()                                         #  beside a live result allocates 1.6 GB of page-locked memory)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        ev0.record()
        res = one(nrec)
        ev1.record()                                                     # behind every lane's kernels (the loop joins its lanes)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        st = dict(S.STATS)
        r = {"wall_ms": round(wall * 1e3, 2), "Mchunks_per_s": round(chunks / wall / 1e6, 2), "h2d_GBps": round(st["h2d_bytes"] / wall / 1e9, 2),
             "kernels_ms": round(ev0.elapsed_time(ev1), 2), "buckets": int(st["buckets"])}
        if way == "audio":
            segments, audio = res
            r.update(audio_d2h_MB=round(st["audio_d2h_bytes"] / 1e6, 1), collect_MB=round(st["collect_bytes"] / 1e6, 1),
                     audio_d2h_ms=round(st["audio_d2h_s"] * 1e3, 2), host_rows=int(st.get("collect_host_rows", 0)),
                     audio_samples=int(sum(a.numel() for a in audio)))
            # where each copy lies on the device's clock, against the end of the last kernel of the run
            ends = [ev0.elapsed_time(e1) for _, e1, _ in trace]
            starts = [ev0.elapsed_time(e0) for e0, _, _ in trace]
            k_end = ev0.elapsed_time(ev1)
            r.update(d2h_copies=len(trace), d2h_copies_done_before_last_kernel=sum(e <= k_end for e in ends),
                     d2h_ms_behind_last_kernel=round(max(0.0, max(ends) - max(k_end, min(starts))) if ends else 0.0, 2),
                     d2h_GBps_while_copying=round(st["audio_d2h_bytes"] / st["audio_d2h_s"] / 1e9, 2) if st.get("audio_d2h_s") else None)
            S.AUDIO_TRACE = None
        runs.append(r)
    print(json.dumps({"way": way, "tree": str(Path(silero_vad_amd.__file__).resolve().parents[1]), "recordings": nrec,
                      "audio_hours": round(float(lens.sum()) / SR / 3600, 2), "chunks": chunks, "runs": runs}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "kernel":
        kernel(int(sys.argv[2]) if len(sys.argv) > 2 else 256)
    elif len(sys.argv) > 2 and sys.argv[1] == "corpus" and sys.argv[2] in ("audio", "segments"):
        corpus(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 2048, int(sys.argv[4]) if len(sys.argv) > 4 else 3)
    else:
        sys.exit(__doc__)
