#!/usr/bin/env python3
"""The corpus' arena-window route at 8 kHz on the same recorded calls three ways: as the de-interleaved mono int16 twin corpus, two
recordings a call (`twin`), as interleaved stereo int16 (`stereo_s16`), and as interleaved stereo G.711 mu-law packed back to back
(`stereo_ulaw`: most calls start at a misaligned byte).  Each way is one `ragged_speech_segments` call over a PackedRecordings in
page-locked memory (one DMA per arena window, batches cut -- and for the stereo ways split, for G.711 expanded -- on the device, scan
on the device), warmed up and reserved first; the ways are alternated `reps` times on one engine.  Prints one JSON line: per way and
repetition the delivered chunks/s and the GB/s that crossed the link, their best and spread, the ratios to the twin way -- and
  * the gather kernels' own time on one bucket that already lies in HBM (hipEvents around `upload_rows_coded` on the twin's rows and
    `upload_rows_channels` on the interleaved sources, how = 2);
  * the host time of de-interleaving the same corpus with `vad_deinterleave` on 16 threads: the pass over the corpus that the device
    split takes off the host.

    python tools/stereo_corpus_time.py [calls] [reps]

calls: 20-40 s each, two channels (default 4096: 68 h of audio in 8192 channels, 3.9 GB as int16, pinned three times over in its three
forms); reps: 3."""
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def main():
    import ctypes

    import numpy as np
    import torch
    import bench
    from g711_corpus_time import g711_encode
    from silero_vad_amd import PackedRecordings, _lib, load_silero_vad, ragged_speech_segments
    from silero_vad_amd import streams as S
    ncall = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    sr, n = 8000, 256
    dev = torch.device("cuda", 0)
    model = load_silero_vad(device=0)
    link = bench.h2d_rate_GBps(dev)
    rng = np.random.default_rng(7)
    page_len = 8 << 20                                                  # the signal every channel is cut from (bench.py run_corpus)
    tt = np.arange(page_len, dtype=np.float32) / sr
    page = ((0.03 * rng.standard_normal(page_len).astype(np.float32)
             + 0.2 * np.sin(2 * np.pi * 170.0 * tt) * (np.sin(2 * np.pi * 0.7 * tt) > 0)) * 32767.0).clip(-32768, 32767).astype(np.int16)
    page_u = g711_encode(page, "ulaw")
    frames = rng.integers(20 * sr, 40 * sr, size=ncall).astype(np.int64)
    cut = rng.integers(0, page_len - 40 * sr, size=(ncall, 2))         # where in the page each channel's audio comes from
    offs = np.concatenate([[0], np.cumsum(2 * frames)[:-1]]).astype(np.int64)       # calls back to back, in samples of both channels

    def stereo_arena(dtype, src):
        base = torch.empty(int(2 * frames.sum()) + 16, dtype=dtype, pin_memory=True)
        b = base.numpy()
        for o, (c0, c1), m in zip(offs, cut, frames):
            b[o:o + 2 * m:2] = src[c0:c0 + m]
            b[o + 1:o + 2 * m:2] = src[c1:c1 + m]
        return PackedRecordings(base, offs, 2 * frames)

    def twin_arena():
        """the two channels of a call back to back in the range its frames occupy in the interleaved int16 arena"""
        base = torch.empty(int(2 * frames.sum()) + 16, dtype=torch.int16, pin_memory=True)
        b = base.numpy()
        t_offs = np.stack([offs, offs + frames], axis=1).reshape(-1)
        t_lens = np.repeat(frames, 2)
        for o, c, m in zip(t_offs, cut.reshape(-1), t_lens):
            b[o:o + m] = page[c:c + m]
        return PackedRecordings(base, t_offs, t_lens)

    ways = {"twin": (twin_arena(), None, None), "stereo_s16": (stereo_arena(torch.int16, page), None, 2),
            "stereo_ulaw": (stereo_arena(torch.uint8, page_u), "ulaw", 2)}
    chunks = int(2 * ((frames + n - 1) // n).sum())
    kw = dict(max_waste=0.1, max_bytes=1 << 30, as_arrays=True)

    def one(name, calls):
        rec, codec, ch = ways[name]
        m = calls * (2 if ch is None else 1)
        sub = PackedRecordings(rec.base, rec.offsets[:m], rec.lengths[:m])
        return ragged_speech_segments(sub, model, sr, codec=codec, channels=ch, **kw)

    runs = {name: [] for name in ways}
    counts = {}
    for name, (rec, codec, ch) in ways.items():                         # warm-up and everything the full plan allocates
        one(name, min(ncall, 1024))
        S.ragged_reserve(rec, model, sr, max_waste=0.1, max_bytes=1 << 30, codec=codec, channels=ch)
    for _ in range(reps):                                               # alternating
        for name in ways:
            S.STATS.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            counts[name], _ = one(name, ncall)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            st = dict(S.STATS)
            runs[name].append({"chunks_per_s": chunks / wall, "link_GBps": st["h2d_bytes"] / wall / 1e9,
                               "link_GBps_while_copying": st["h2d_bytes"] / st["h2d_s"] / 1e9 if st.get("h2d_s") else None})
    assert np.array_equal(counts["twin"], counts["stereo_s16"])        # (the same audio: the same segments)

    out = {"sr": sr, "calls": ncall, "audio_hours": round(float(2 * frames.sum()) / sr / 3600.0, 2), "chunks": chunks, "reps": reps,
           "h2d_GBps": round(link, 2)}
    for name, rr in runs.items():
        v = [r["chunks_per_s"] for r in rr]
        g = [r["link_GBps"] for r in rr]
        out[name] = {"Mchunks_per_s": [round(x / 1e6, 2) for x in v], "best_Mchunks_per_s": round(max(v) / 1e6, 2),
                     "spread": round((max(v) - min(v)) / max(v), 4), "link_GBps": [round(x, 2) for x in g],
                     "best_of_link": round(max(g) / link, 3),
                     "link_GBps_while_copying": [round(r["link_GBps_while_copying"], 2) if r["link_GBps_while_copying"] else None for r in rr]}
    best = {name: max(r["chunks_per_s"] for r in rr) for name, rr in runs.items()}
    worst = {name: min(r["chunks_per_s"] for r in rr) for name, rr in runs.items()}
    out["stereo_s16_over_twin"] = round(best["stereo_s16"] / best["twin"], 3)
    out["stereo_ulaw_over_twin"] = round(best["stereo_ulaw"] / best["twin"], 3)
    out["twin_worst_over_best"] = round(worst["twin"] / best["twin"], 3)

    # the gather kernels alone: one bucket of 1 024 rows (512 calls, padded to the longest) whose bytes already lie in HBM
    m = min(ncall, 512)
    width = (int(frames[:m].max()) + 7) // 8 * 8
    dst = torch.empty((2 * m, width), dtype=torch.int16, device=dev)
    kern = {}
    for name, (rec, codec, ch) in ways.items():
        esz = rec.base.element_size()
        k_src = m if ch else 2 * m
        hi = int(rec.offsets[k_src - 1] + rec.lengths[k_src - 1])
        on_dev = rec.base[:hi + 16 // esz].to(dev)
        rows = np.ascontiguousarray(on_dev.data_ptr() + rec.offsets[:k_src] * esz, dtype=np.uint64)
        rp = rows.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p))
        fr = np.ascontiguousarray(rec.lengths[:k_src] // (ch or 1))
        lp = fr.ctypes.data_as(ctypes.POINTER(ctypes.c_long))
        cd = None if codec is None else np.full(k_src, 1, np.uint8)
        chs = np.full(k_src, 2, np.uint8)
        to = np.arange(2 * m, dtype=np.int32).reshape(m, 2)
        ms = []
        for k in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if ch is None:
                model.engine.upload_rows_coded(rp, lp, cd, k_src, width, dst, 2)
            else:
                model.engine.upload_rows_channels(rp, lp, cd, chs, to, k_src, 2 * m, width, dst, 2)
            e1.record()
            e1.synchronize()
            if k:                                                       # (the first launch loads the code object)
                ms.append(e0.elapsed_time(e1))
        kern[name] = {"ms": round(min(ms), 3), "Gsamples_per_s": round(float(2 * frames[:m].sum()) / min(ms) / 1e6, 1)}
        del on_dev
    out["gather_kernel_1024_rows_in_hbm"] = kern

    # what the feature takes off the host: vad_deinterleave over the whole stereo int16 corpus, 16 threads (the call releases the GIL)
    L = _lib.lib()
    rec = ways["stereo_s16"][0]
    src_ptr = rec.base.data_ptr()
    scratch = np.empty(int(2 * frames.sum()), dtype=np.int16)

    def split(i):
        for c in range(2):
            L.vad_deinterleave(0, 2, c, src_ptr + int(offs[i]) * 2, int(frames[i]), scratch.ctypes.data + (int(offs[i]) + c * int(frames[i])) * 2)

    host = []
    with ThreadPoolExecutor(16) as pool:
        for _ in range(reps):
            t0 = time.perf_counter()
            list(pool.map(split, range(ncall), chunksize=16))
            host.append(time.perf_counter() - t0)
    out["host_deinterleave_16_threads"] = {"s": [round(x, 3) for x in host], "GBps_read": round(float(4 * frames.sum()) / min(host) / 1e9, 2),
                                           "share_of_best_stereo_s16_run": round(min(host) / (chunks / best["stereo_s16"]), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
