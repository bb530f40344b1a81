#!/usr/bin/env python3
"""What the enter / exit threshold sweep costs (profiles/threshold_sweep.md).  One GPU process, two parts, one JSON line:

    python tools/threshold_sweep_time.py [rows] [recordings] [reps]

  kernel  sweep_kernel alone (vad_threshold_counts_device, csrc/kernel_sweep.hip): `rows` (default 4 096) rows of 256 chunks -- and, as the
          corpus leg's bucket of its longest recordings, 56 rows of 1 875 chunks (60 s) -- against the 190 pairs of the reference's grid,
          on the probabilities the net itself left in HBM for a batch of speech cut from the fixture; hipEvents around windows of 20 launches after a warm-up, the best and the median window.  Beside it the frontend's and the
          recurrence's time for the SAME batch (option profile = 1, vad_kernel_times) and the instruction-count estimate.
  corpus  `recordings` (default 2 000) recordings of 1 ... 60 s in one page-locked arena: the wall time of `ragged_threshold_counts`
          and of `ragged_probs` on the same recordings, alternating, `reps` (default 3) runs each after a warm-up and a
          ragged_reserve, and the bytes each copies back.
"""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SR, N = 16000, 512
VALU_PER_CHUNK_PAIR = 8           # the estimate: two compares, two selects, and the and / add of each of the two counts
LANES_PER_CLOCK = 256 * 4 * 32    # 256 CUs x 4 SIMDs x 32 lanes: 32-bit VALU results per clock
CLOCK_GHZ = 2.4


def speech_page():
    import numpy as np
    pcm = np.load(ROOT / "tests" / "golden" / "audio_16k.npz")["pcm"]
    return np.concatenate([pcm, pcm])


def run_labels(rng, m):
    """speech / silence in runs of 5 ... 60 chunks, one ignored chunk in fifty"""
    import numpy as np
    lab = np.zeros(m, dtype=np.uint8)
    t, on = 0, False
    while t < m:
        k = int(rng.integers(5, 61))
        lab[t:t + k] = on
        t, on = t + k, not on
    lab[rng.random(m) < 0.02] = 255
    lab[0] = 1
    return lab


def kernel(model, rows, T):
    import numpy as np
    import torch
    from silero_vad_amd import threshold_pairs
    from silero_vad_amd import streams as S
    dev = torch.device("cuda", 0)
    eng = model.engine
    page = speech_page()
    rng = np.random.default_rng(3)
    x = torch.from_numpy(np.stack([page[a:a + T * N] for a in rng.integers(0, len(page) - T * N, size=rows)])).to(dev)
    eng.set_option("profile", 1)
    model.audio_forward_device(x, SR)
    torch.cuda.synchronize()
    eng.kernel_times()
    probs = model.audio_forward_device(x, SR)
    torch.cuda.synchronize()
    f_ms, r_ms, _ = eng.kernel_times()
    eng.set_option("profile", 0)
    assert probs.shape == (rows, T)
    pr = threshold_pairs()
    P = len(pr.enter)
    labels = [run_labels(rng, T) for _ in range(rows)]
    lab, offs = S._pack_labels(labels, [T] * rows, "tool")
    meta = S._label_meta(np.full(rows, T, dtype=np.int64), lab, offs).to(dev)
    thr = torch.from_numpy(np.stack([pr.enter_f32, pr.exit_f32])).to(dev)

    def launch():
        return S._device_sweep(eng, probs, meta[:rows], meta.data_ptr() + 16 * rows, meta[rows:2 * rows], thr[0], thr[1])

    out = launch()
    torch.cuda.synchronize()
    # (the counts are the host twin's: a timing of a wrong kernel is no timing)
    want = S.threshold_counts(probs.cpu(), [T] * rows, labels, pr)
    got = S._split_counts(out.cpu().numpy(), rows, P)
    assert all(np.array_equal(g, w) for g, w in zip(got, (want.tp, want.tn, want.n_pos, want.n_valid)))
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    ms, per = [], 20
    for _ in range(9):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            launch()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / per)
    best = min(ms)
    ops = rows * T * P * VALU_PER_CHUNK_PAIR
    est_ms = ops / (LANES_PER_CLOCK * CLOCK_GHZ * 1e9) * 1e3
    return {"rows": rows, "chunks_per_row": T, "pairs": P, "sweep_ms": round(best, 4), "sweep_ms_median": round(sorted(ms)[len(ms) // 2], 4),
            "launches_per_window": per, "windows": len(ms), "estimate_valu_per_chunk_pair": VALU_PER_CHUNK_PAIR, "estimate_ms": round(est_ms, 4),
            "measured_over_estimate": round(best / est_ms, 2), "G_chunk_pairs_per_s": round(rows * T * P / best / 1e6, 1),
            "frontend_ms_same_batch": round(f_ms, 3), "recurrence_ms_same_batch": round(r_ms, 3),
            "sweep_over_front_plus_rec": round(best / (f_ms + r_ms), 5) if f_ms + r_ms else None,
            "counts_bytes_back": rows * (2 * P + 2) * 4, "probs_bytes_back_otherwise": rows * T * 4}


def corpus(model, nrec, reps):
    import numpy as np
    import torch
    from silero_vad_amd import PackedRecordings, ragged_probs, ragged_threshold_counts
    from silero_vad_amd import streams as S
    page = speech_page()
    rng = np.random.default_rng(7)
    lens = rng.integers(1 * SR, 60 * SR + 1, size=nrec).astype(np.int64)
    cut = rng.integers(0, len(page) - 60 * SR, size=nrec)
    step = (lens + 7) // 8 * 8
    offs = np.concatenate([[0], np.cumsum(step)[:-1]]).astype(np.int64)
    base = torch.empty(int(step.sum()) + 16, dtype=torch.int16, pin_memory=True)
    b = base.numpy()
    for o, c, m in zip(offs, cut, lens):
        b[o:o + m] = page[c:c + m]
    rec = PackedRecordings(base, offs, lens)
    labels = [run_labels(rng, int(m)) for m in (lens + N - 1) // N]
    kw = dict(max_waste=0.1, max_bytes=256 << 20)
    ways = {"ragged_threshold_counts": lambda m: ragged_threshold_counts(PackedRecordings(base, offs[:m], lens[:m]), labels[:m], model, SR, **kw),
            "ragged_probs": lambda m: ragged_probs(PackedRecordings(base, offs[:m], lens[:m]), model, SR, **kw)}
    for one in ways.values():
        one(min(nrec, 256))
    S.ragged_reserve(rec, model, SR, **kw)
    for one in ways.values():
        one(nrec)
    chunks = int(((lens + N - 1) // N).sum())
    runs = {name: [] for name in ways}
    for _ in range(reps):
        for name, one in ways.items():                                   # alternating: the two see the same machine
            S.STATS.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = one(nrec)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            del res
            runs[name].append({"wall_ms": round(wall * 1e3, 2), "Mchunks_per_s": round(chunks / wall / 1e6, 2),
                               "d2h_MB": round(S.STATS["d2h_bytes"] / 1e6, 3), "buckets": int(S.STATS["buckets"]),
                               "setup_ms": round(S.STATS["setup_s"] * 1e3, 2), "result_wait_ms": round(S.STATS["result_wait_s"] * 1e3, 2),
                               "slot_wait_ms": round(S.STATS["slot_wait_s"] * 1e3, 2)})
    best = {name: min(r["wall_ms"] for r in rs) for name, rs in runs.items()}
    return {"recordings": nrec, "audio_hours": round(float(lens.sum()) / SR / 3600, 2), "chunks": chunks, "runs": runs, "best_wall_ms": best,
            "counts_over_probs_wall": round(best["ragged_threshold_counts"] / best["ragged_probs"], 3)}


if __name__ == "__main__":
    if len(sys.argv) > 1 and not sys.argv[1].isdigit():
        sys.exit(__doc__)
    a = [int(v) for v in sys.argv[1:]]
    from silero_vad_amd import load_silero_vad
    model = load_silero_vad(device=0)
    print(json.dumps({"kernel": kernel(model, a[0] if a else 4096, 256), "kernel_bucket_of_60s_rows": kernel(model, 56, 1875),
                      "corpus": corpus(model, a[1] if len(a) > 1 else 2000, a[2] if len(a) > 2 else 3)}))
