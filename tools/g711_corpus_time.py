#!/usr/bin/env python3
"""The corpus' arena-window route at 8 kHz on the same recordings three ways: as int16 (`int16`), as G.711 mu-law with every recording
at a 16-byte aligned offset of its arena (`ulaw_aligned`), and as mu-law packed back to back (`ulaw_packed`: 15 of 16 recordings start
at a misaligned byte).  Each way is one `ragged_speech_segments` call over a PackedRecordings in page-locked memory (one DMA per arena
window, batches cut -- and for G.711 expanded -- on the device, scan on the device), warmed up and reserved first; the ways are
alternated `reps` times on one engine.  Prints one JSON line: per way and repetition the delivered chunks/s and the GB/s that crossed
the link, their best and spread, the share of a plain pinned -> HBM copy's rate, the ratios between the ways -- and the gather
kernels' own time on one bucket that already lies in HBM (hipEvents around `upload_rows` / `upload_rows_coded`, how = 2).

    python tools/g711_corpus_time.py [recordings] [reps]

recordings: 20-40 s each (default 8192: 68 h of audio, 3.9 GB as int16, pinned three times over in its three forms); reps: 3."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def g711_encode(pcm, law):
    """int16 -> the G.711 code whose expansion is nearest (what an encoder on the far side of the trunk would have sent)."""
    import numpy as np
    from silero_vad_amd import g711_expand
    codes = np.arange(256, dtype=np.uint8)
    lin = g711_expand(codes, law).astype(np.int32)
    order = np.argsort(lin, kind="stable")
    v = lin[order]
    x = pcm.astype(np.int32)
    j = np.clip(np.searchsorted(v, x), 1, len(v) - 1)
    j -= (x - v[j - 1]) <= (v[j] - x)
    return codes[order[j]]


def main():
    import ctypes

    import numpy as np
    import torch
    import bench
    from silero_vad_amd import PackedRecordings, load_silero_vad, ragged_speech_segments
    from silero_vad_amd import streams as S
    nrec = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    sr, n = 8000, 256
    dev = torch.device("cuda", 0)
    model = load_silero_vad(device=0)
    link = bench.h2d_rate_GBps(dev)
    rng = np.random.default_rng(7)
    page_len = 8 << 20                                                  # the signal every recording is cut from (bench.py run_corpus)
    tt = np.arange(page_len, dtype=np.float32) / sr
    page = ((0.03 * rng.standard_normal(page_len).astype(np.float32)
             + 0.2 * np.sin(2 * np.pi * 170.0 * tt) * (np.sin(2 * np.pi * 0.7 * tt) > 0)) * 32767.0).clip(-32768, 32767).astype(np.int16)
    page_u = g711_encode(page, "ulaw")
    lens = rng.integers(20 * sr, 40 * sr, size=nrec).astype(np.int64)
    cut = rng.integers(0, page_len - 40 * sr, size=nrec)               # where in the page each recording's audio comes from

    def arena(dtype, src, align):
        """the recordings one behind the other at multiples of `align` samples, page-locked"""
        step = (lens + align - 1) // align * align
        offs = np.concatenate([[0], np.cumsum(step)[:-1]]).astype(np.int64)
        base = torch.empty(int(step.sum()) + 16, dtype=dtype, pin_memory=True)
        b = base.numpy()
        for o, c, m in zip(offs, cut, lens):
            b[o:o + m] = src[c:c + m]
        return PackedRecordings(base, offs, lens)

    ways = {"int16": (arena(torch.int16, page, 8), None), "ulaw_aligned": (arena(torch.uint8, page_u, 16), "ulaw"),
            "ulaw_packed": (arena(torch.uint8, page_u, 1), "ulaw")}
    chunks = int(((lens + n - 1) // n).sum())
    kw = dict(max_waste=0.1, max_bytes=1 << 30, as_arrays=True)

    def one(name, m):
        rec, codec = ways[name]
        sub = PackedRecordings(rec.base, rec.offsets[:m], rec.lengths[:m])
        return ragged_speech_segments(sub, model, sr, codec=codec, **kw)

    runs = {name: [] for name in ways}
    counts = {}
    for name, (rec, codec) in ways.items():                             # warm-up and everything the full plan allocates
        one(name, min(nrec, 2048))
        S.ragged_reserve(rec, model, sr, max_waste=0.1, max_bytes=1 << 30, codec=codec)
    for _ in range(reps):                                               # alternating
        for name in ways:
            S.STATS.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            counts[name], _ = one(name, nrec)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            st = dict(S.STATS)
            runs[name].append({"chunks_per_s": chunks / wall, "link_GBps": st["h2d_bytes"] / wall / 1e9,
                               "link_GBps_while_copying": st["h2d_bytes"] / st["h2d_s"] / 1e9 if st.get("h2d_s") else None})
    assert np.array_equal(counts["ulaw_aligned"], counts["ulaw_packed"])

    out = {"sr": sr, "recordings": nrec, "audio_hours": round(float(lens.sum()) / sr / 3600.0, 2), "chunks": chunks, "reps": reps,
           "h2d_GBps": round(link, 2)}
    for name, rr in runs.items():
        v = [r["chunks_per_s"] for r in rr]
        g = [r["link_GBps"] for r in rr]
        out[name] = {"Mchunks_per_s": [round(x / 1e6, 2) for x in v], "best_Mchunks_per_s": round(max(v) / 1e6, 2),
                     "spread": round((max(v) - min(v)) / max(v), 4), "link_GBps": [round(x, 2) for x in g],
                     "best_of_link": round(max(g) / link, 3),
                     "link_GBps_while_copying": [round(r["link_GBps_while_copying"], 2) if r["link_GBps_while_copying"] else None for r in rr]}
    best = {name: max(r["chunks_per_s"] for r in rr) for name, rr in runs.items()}
    out["ulaw_aligned_over_int16"] = round(best["ulaw_aligned"] / best["int16"], 3)
    out["ulaw_packed_over_int16"] = round(best["ulaw_packed"] / best["int16"], 3)
    out["ulaw_packed_over_aligned"] = round(best["ulaw_packed"] / best["ulaw_aligned"], 3)

    # the gather kernels alone: one bucket of 1 024 recordings (padded to the longest) whose bytes already lie in HBM
    m = min(nrec, 1024)
    width = (int(lens[:m].max()) + 7) // 8 * 8
    dst = torch.empty((m, width), dtype=torch.int16, device=dev)
    lp = np.ascontiguousarray(lens[:m]).ctypes.data_as(ctypes.POINTER(ctypes.c_long))
    kern = {}
    for name, (rec, codec) in ways.items():
        esz = rec.base.element_size()
        hi = int(rec.offsets[m - 1] + rec.lengths[m - 1])
        on_dev = rec.base[:hi + 16 // esz].to(dev)
        rows = np.ascontiguousarray(on_dev.data_ptr() + rec.offsets[:m] * esz, dtype=np.uint64)
        rp = rows.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p))
        cd = None if codec is None else np.full(m, 1, np.uint8)
        ms = []
        for k in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if cd is None:
                model.engine.upload_rows(rp, lp, m, width, 2, dst, 2)
            else:
                model.engine.upload_rows_coded(rp, lp, cd, m, width, dst, 2)
            e1.record()
            e1.synchronize()
            if k:                                                       # (the first launch loads the code object)
                ms.append(e0.elapsed_time(e1))
        kern[name] = {"ms": round(min(ms), 3), "Gsamples_per_s": round(float(lens[:m].sum()) / min(ms) / 1e6, 1)}
        del on_dev
    out["gather_kernel_1024_rows_in_hbm"] = kern
    print(json.dumps(out))


if __name__ == "__main__":
    main()
