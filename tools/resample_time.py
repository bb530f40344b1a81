#!/usr/bin/env python3
"""What resampling on the device costs (profiles/resample.md).  One GPU process; prints one JSON line with two measurements.

  * kernel: the resample kernel alone (vad_resample_rows_device, csrc/kernel_resample.hip) on ONE bucket of the corpus leg's shape
    that already lies in HBM -- `rows` recordings of 20-40 s at 44.1 kHz, int16, padded to the longest --: its time (hipEvents, best
    and median of 6), the bytes it must move (the live int16 samples read, the float32 batch written) and the share of the HBM
    peak that is; beside it the frontend's and the recurrence's time for the resampled bucket (option profile = 1, vad_kernel_times).
  * corpus: the link share of a 44.1 kHz int16 corpus in a page-locked arena through ragged_speech_segments(source_rate=44100)
    against the raw 48 kHz leg (sampling_rate=48000: the same arena route, decimation inside the frontend's loads, no resampler) on
    the same recordings' durations, each warmed up and reserved first, the two alternated `reps` times on one engine: delivered
    chunks/s, GB/s over the link and their share of the pinned H2D rate measured at the start (bench.h2d_rate_GBps).

    python tools/resample_time.py [recordings] [reps] [rows]

recordings: 20-40 s each (default 1536: 12.8 h, 4 GB at 44.1 kHz, pinned once per rate); reps: 3; rows of the kernel's bucket: 96 (a
256 MB bucket of 30 s recordings at 44.1 kHz)."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
HBM_PEAK_GBPS = 8000.0                                                  # MI355X: 8 TB/s


def page_at(sr, seconds, rng):
    """noise and a gated tone, int16, at `sr` (bench.py run_corpus' signal)"""
    import numpy as np
    n = int(seconds * sr)
    tt = np.arange(n, dtype=np.float32) / sr
    return ((0.03 * rng.standard_normal(n).astype(np.float32)
             + 0.2 * np.sin(2 * np.pi * 170.0 * tt) * (np.sin(2 * np.pi * 0.7 * tt) > 0)) * 32767.0).clip(-32768, 32767).astype(np.int16)


def main():
    import numpy as np
    import torch
    import bench
    from silero_vad_amd import PackedRecordings, load_silero_vad, ragged_speech_segments, resample_device, resample_geometry
    from silero_vad_amd import streams as S
    nrec = int(sys.argv[1]) if len(sys.argv) > 1 else 1536
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    rows = int(sys.argv[3]) if len(sys.argv) > 3 else 96
    dev = torch.device("cuda", 0)
    model = load_silero_vad(device=0)
    link = bench.h2d_rate_GBps(dev)
    rng = np.random.default_rng(7)
    secs = rng.uniform(20.0, 40.0, size=nrec)
    start = rng.uniform(0.0, 80.0, size=nrec)
    O, N, W, K = resample_geometry(44100, 16000)
    out = {"recordings": nrec, "audio_hours": round(float(secs.sum()) / 3600.0, 2), "reps": reps, "h2d_GBps": round(link, 2)}

    # ---- the kernel alone ------------------------------------------------------------------------------------------------
    page = page_at(44100, 120, rng)
    lens = (secs[:rows] * 44100).astype(np.int64)
    L = (int(lens.max()) + 7) // 8 * 8
    host = np.zeros((rows, L), np.int16)
    for r in range(rows):
        a = int(start[r] * 44100)
        host[r, :lens[r]] = page[a:a + lens[r]]
    x = torch.from_numpy(host).to(dev)
    lens_dev = torch.from_numpy(lens).to(dev)
    width = (int(lens.max()) * N + O - 1) // O
    y = torch.empty((rows, (width + 3) // 4 * 4), dtype=torch.float32, device=dev)[:, :width]
    ms = []
    for k in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        resample_device(model.engine, x, lens_dev, 44100, 16000, out=y)
        e1.record()
        e1.synchronize()
        if k:                                                           # (the first launch loads the code object and the table)
            ms.append(e0.elapsed_time(e1))
    moved = int(lens.sum()) * 2 + rows * width * 4                      # live int16 read once + every float32 of the batch written
    best = min(ms)
    model.engine.set_option("profile", 1)
    model.audio_forward_device(y, 16000)
    torch.cuda.synchronize()
    model.engine.kernel_times()
    model.audio_forward_device(y, 16000)
    torch.cuda.synchronize()
    f_ms, r_ms, _ = model.engine.kernel_times()
    model.engine.set_option("profile", 0)
    out["kernel"] = {"rows": rows, "raw_samples_per_row": L, "out_samples_per_row": width, "batch_MB_int16": round(rows * L * 2 / 1e6, 1),
                     "ms": round(best, 4), "ms_median": round(sorted(ms)[len(ms) // 2], 4), "MB_moved": round(moved / 1e6, 1),
                     "GBps": round(moved / best / 1e6, 1), "share_of_hbm_peak": round(moved / best / 1e6 / HBM_PEAK_GBPS, 3),
                     "Gfma_per_s": round(float(((lens * N + O - 1) // O).sum()) * K / best / 1e6, 1),
                     "frontend_ms_same_bucket": round(f_ms, 3), "recurrence_ms_same_bucket": round(r_ms, 3),
                     "resample_over_frontend": round(best / f_ms, 4) if f_ms else None}
    del x, y, host

    # ---- the corpus: 44.1 kHz through the resampler against the raw 48 kHz leg ---------------------------------------------------
    ways = {}
    for name, sr in (("src44100", 44100), ("raw48000", 48000)):
        pg = page if sr == 44100 else page_at(48000, 120, rng)
        m = (secs * sr).astype(np.int64)
        step = (m + 7) // 8 * 8
        offs = np.concatenate([[0], np.cumsum(step)[:-1]]).astype(np.int64)
        base = torch.empty(int(step.sum()) + 16, dtype=torch.int16, pin_memory=True)
        b = base.numpy()
        for o, s0, k in zip(offs, start, m):
            a = int(s0 * sr)
            b[o:o + k] = pg[a:a + k]
        rec = PackedRecordings(base, offs, m)
        n_out = (m * N + O - 1) // O if sr == 44100 else (m + 2) // 3
        kw = dict(sampling_rate=16000, source_rate=44100) if sr == 44100 else dict(sampling_rate=48000)
        ways[name] = (rec, kw, int(((n_out + 511) // 512).sum()))
    common = dict(max_waste=0.1, max_bytes=256 << 20, as_arrays=True)

    def one(name, m):
        rec, kw, _ = ways[name]
        return ragged_speech_segments(PackedRecordings(rec.base, rec.offsets[:m], rec.lengths[:m]), model, **kw, **common)

    for name, (rec, kw, _) in ways.items():                             # warm-up and everything the full plan allocates
        one(name, min(nrec, 256))
        S.ragged_reserve(rec, model, max_waste=0.1, max_bytes=256 << 20, **kw)
        one(name, nrec)
    runs = {name: [] for name in ways}
    for _ in range(reps):                                               # alternating
        for name, (rec, kw, chunks) in ways.items():
            S.STATS.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one(name, nrec)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            st = dict(S.STATS)
            runs[name].append({"wall_ms": round(wall * 1e3, 2), "Mchunks_per_s": round(chunks / wall / 1e6, 2),
                               "link_GBps": round(st["h2d_bytes"] / wall / 1e9, 2), "of_link": round(st["h2d_bytes"] / wall / 1e9 / link, 3),
                               "buckets": int(st["buckets"]), "resample_allocs": int(st.get("resample_allocs", 0))})
    for name, rr in runs.items():
        v = [r["of_link"] for r in rr]
        out[name] = {"chunks": ways[name][2], "runs": rr, "best_of_link": max(v), "spread_of_link": round(max(v) - min(v), 3)}
    a, b = [r["of_link"] for r in runs["src44100"]], [r["of_link"] for r in runs["raw48000"]]
    out["src44100_within_raw48000_spread"] = bool(min(b) - (max(b) - min(b)) <= max(a))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
