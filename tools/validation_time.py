#!/usr/bin/env python3
"""What the validation scores cost (profiles/validation_scores.md).  One GPU process, three parts, one JSON line:

    python tools/validation_time.py [rows] [recordings] [reps] [largest power of ten of keys]

  kernel  score_kernel alone (vad_chunk_scores_device, csrc/kernel_score.hip): `rows` (default 4 096) rows of 256 chunks -- and, as the
          corpus leg's bucket of its longest recordings, 56 rows of 1 875 chunks (60 s) -- on the probabilities the net itself left in
          HBM for a batch of speech cut from the fixture; hipEvents around windows of 20 launches after a warm-up, the best and the
          median window.  Beside it the frontend's and the recurrence's time for the SAME batch (option profile = 1).
  auc     vad_auc_counts_device over 10^6, 10^7 and 10^8 keys made on the device: uniform probabilities, probabilities drawn from the
          reference's predictions on the speech fixture (golden_validation.npz, e2e_16k), and one probability for all.  Beside each
          time the occupancy of the bins the counting scheme forms (bins in use, bins that hold both classes, the largest of those):
          the largest is what the slowest workgroup streams.  Up to 10^7 keys the three integers are checked against the host twin.
  corpus  `recordings` (default 2 000) recordings of 1 ... 60 s in one page-locked arena: the wall time of `ragged_validation`, of
          `ragged_probs`, and of `ragged_probs` followed by the host twins (`chunk_scores`), alternating, `reps` (default 3) runs each
          after a warm-up and a ragged_reserve, and the bytes each copies back.
"""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
SR, N = 16000, 512


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


def windows(launch, per=20, count=9, warm=5):
    import torch
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            launch()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / per)
    return min(ms), sorted(ms)[len(ms) // 2]


def kernel(model, rows, T):
    import numpy as np
    import torch
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
    labels = [run_labels(rng, T) for _ in range(rows)]
    nck = np.full(rows, T, dtype=np.int64)
    lab, offs = S._pack_labels(labels, nck, "tool")
    meta = S._score_meta(nck, lab, offs, offs).to(dev)
    keys = torch.empty(rows * T, dtype=torch.int32, device=dev)

    def launch():
        return S._device_scores(eng, probs, meta, rows, keys)

    out = launch()
    torch.cuda.synchronize()
    # (the counts and keys are the host twin's: a timing of a wrong kernel is no timing)
    want = S.chunk_scores(probs.cpu(), nck, labels)
    got = S._split_scores(out.cpu().numpy(), rows)
    assert all(np.array_equal(g, w) for g, w in zip(got[2:], (want.n_pos, want.n_neg, want.n_bad)))
    assert np.array_equal(keys.cpu().numpy().view(np.uint32), want.keys)
    best, median = windows(launch)
    return {"rows": rows, "chunks_per_row": T, "score_ms": round(best, 4), "score_ms_median": round(median, 4),
            "G_chunks_per_s": round(rows * T / best / 1e6, 2), "GB_per_s_read_and_written": round(rows * T * 9 / best / 1e6, 1),
            "frontend_ms_same_batch": round(f_ms, 3), "recurrence_ms_same_batch": round(r_ms, 3),
            "score_over_front_plus_rec": round(best / (f_ms + r_ms), 5) if f_ms + r_ms else None,
            "bytes_back": rows * 28, "probs_bytes_back_otherwise": rows * T * 4}


def auc(model, n, shape):
    import numpy as np
    import torch
    from silero_vad_amd import _lib
    from silero_vad_amd import streams as S
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(n % 1000 + len(shape))
    lab = torch.randint(0, 2, (n,), device=dev, dtype=torch.int32, generator=g)
    if shape == "uniform":
        p = torch.rand(n, device=dev, generator=g)
    elif shape == "fixture":
        z = np.load(ROOT / "tests" / "golden" / "golden_validation.npz")
        src = torch.from_numpy(z["e2e_16k_probs"]).to(dev)
        pick = torch.randint(0, len(src), (n,), device=dev, generator=g)
        p = src[pick]
        lab = torch.from_numpy(z["e2e_16k_labels"].astype(np.int32)).to(dev)[pick].clamp(max=1)
        del pick
    else:
        p = torch.full((n,), 0.75, device=dev)
    keys = (p.view(torch.int32) << 1) | lab
    del p, lab
    hi = (keys >> 13).to(torch.int64)
    neg = torch.bincount(hi[(keys & 1) == 0], minlength=1 << 19)
    pos = torch.bincount(hi[(keys & 1) == 1], minlength=1 << 19)
    both = (neg > 0) & (pos > 0)
    occupancy = {"bins_in_use": int(((neg + pos) > 0).sum()), "bins_with_both_classes": int(both.sum()),
                 "largest_bin_with_both_classes": int(((neg + pos) * both).max()), "bins_over_256_keys_with_both": int((((neg + pos) > 256) & both).sum())}
    del hi, neg, pos, both
    L = _lib.lib()
    need = int(L.vad_auc_workspace_bytes(n))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    out = torch.zeros(3, dtype=torch.int64, device=dev)
    import ctypes

    def launch():
        _lib.check(model.engine._h, L.vad_auc_counts_device(model.engine._h, keys.data_ptr(), n, ws.data_ptr(), need, out.data_ptr(),
                                                            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

    launch()
    torch.cuda.synchronize()
    got = tuple(int(v) for v in out.cpu().numpy().view(np.uint64))
    checked = n <= 10 ** 7
    if checked:
        assert got == S._auc_counts_host(keys.cpu().numpy().view(np.uint32)), (shape, n)
    best, median = windows(launch, per=2, count=3, warm=1) if n >= 10 ** 7 else windows(launch, per=10, count=5)
    return dict({"keys": n, "shape": shape, "auc_ms": round(best, 4), "auc_ms_median": round(median, 4), "G_keys_per_s": round(n / best / 1e6, 3),
                 "auc": got[0] / (2 * got[1] * got[2]), "checked_against_host_twin": checked, "workspace_MB": round(need / 1e6, 1)}, **occupancy)


def corpus(model, nrec, reps):
    import numpy as np
    import torch
    from silero_vad_amd import PackedRecordings, chunk_scores, ragged_probs, ragged_validation
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
    nck = (lens + N - 1) // N
    labels = [run_labels(rng, int(m)) for m in nck]
    kw = dict(max_waste=0.1, max_bytes=256 << 20)

    def host_way(m):
        probs = ragged_probs(PackedRecordings(base, offs[:m], lens[:m]), model, SR, **kw)
        T = int(nck[:m].max())
        x = np.zeros((m, T), dtype=np.float32)
        for i, p in enumerate(probs):
            x[i, :len(p)] = p.numpy()
        return chunk_scores(x, nck[:m], labels[:m])

    ways = {"ragged_validation": lambda m: ragged_validation(PackedRecordings(base, offs[:m], lens[:m]), labels[:m], model, SR, **kw),
            "ragged_probs": lambda m: ragged_probs(PackedRecordings(base, offs[:m], lens[:m]), model, SR, **kw),
            "ragged_probs_then_host_twins": host_way}
    for one in ways.values():
        one(min(nrec, 256))
    S.ragged_reserve(rec, model, SR, **kw)
    res = {name: one(nrec) for name, one in ways.items()}
    a, h = res["ragged_validation"], res["ragged_probs_then_host_twins"]
    assert (a.u2, a.total_pos, a.total_neg) == (h.u2, h.total_pos, h.total_neg) and np.array_equal(a.n_pos, h.n_pos)
    pair = a.reference(0.5, 8)
    del res
    # the pooled count alone, on this corpus's own keys
    kept = ragged_validation(rec, labels, model, SR, keep_keys=True, **kw).keys
    k_dev = torch.from_numpy(kept.view(np.int32)).to(torch.device("cuda", 0))
    auc_ms = windows(lambda: S._device_auc(model.engine, k_dev, len(kept)), per=5, count=5, warm=2)
    live = kept[kept != S.SCORE_KEY_NONE]
    bins, per_bin = np.unique(live >> 13, return_counts=True)
    own_keys = {"auc_call_ms_with_its_allocations_and_copy_back": round(auc_ms[0], 3), "distinct_keys": int(len(np.unique(live))), "bins_in_use": int(len(bins)),
                "largest_bin": int(per_bin.max()), "keys_in_the_ten_largest_bins": int(np.sort(per_bin)[-10:].sum())}
    del k_dev, kept, live
    chunks = int(nck.sum())
    runs = {name: [] for name in ways}
    for _ in range(reps):
        for name, one in ways.items():                                   # alternating: the three see the same machine
            S.STATS.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = one(nrec)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            del r
            runs[name].append({"wall_ms": round(wall * 1e3, 2), "Mchunks_per_s": round(chunks / wall / 1e6, 2),
                               "d2h_MB": round(S.STATS["d2h_bytes"] / 1e6, 3), "buckets": int(S.STATS["buckets"]),
                               "setup_ms": round(S.STATS["setup_s"] * 1e3, 2), "result_wait_ms": round(S.STATS["result_wait_s"] * 1e3, 2),
                               "slot_wait_ms": round(S.STATS["slot_wait_s"] * 1e3, 2)})
    best = {name: min(r["wall_ms"] for r in rs) for name, rs in runs.items()}
    return {"recordings": nrec, "audio_hours": round(float(lens.sum()) / SR / 3600, 2), "chunks": chunks, "pair_batch_size_8": list(pair), "auc_on_its_keys": own_keys, "runs": runs,
            "best_wall_ms": best, "validation_over_probs_wall": round(best["ragged_validation"] / best["ragged_probs"], 3),
            "host_twins_over_probs_wall": round(best["ragged_probs_then_host_twins"] / best["ragged_probs"], 3)}


if __name__ == "__main__":
    if len(sys.argv) > 1 and not sys.argv[1].isdigit():
        sys.exit(__doc__)
    a = [int(v) for v in sys.argv[1:]]
    from silero_vad_amd import load_silero_vad
    model = load_silero_vad(device=0)
    top = a[3] if len(a) > 3 else 8
    print(json.dumps({"kernel": kernel(model, a[0] if a else 4096, 256), "kernel_bucket_of_60s_rows": kernel(model, 56, 1875),
                      "auc": [auc(model, 10 ** e, shape) for e in range(6, top + 1) for shape in ("uniform", "fixture", "equal")],
                      "corpus": corpus(model, a[1] if len(a) > 1 else 2000, a[2] if len(a) > 2 else 3)}))
