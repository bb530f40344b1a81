#!/usr/bin/env python3
"""Times of the training augmentations on the GPU (silero_vad_amd/augment.py) at the reference's batch, 128 recordings of 250 chunks:
the device call as a whole (recipes as `Augmenter(p=1)` draws them) and per op kind with one-kind recipes, the host twin on 16
threads for the same batch, and the whole `DecoderTrainer.step` with and without recipes.

    python tools/augment_time.py [--shape 128x250] [--reps 10] [--host-threads 16] [--no-step] [--no-host] [--room]
                                 [--out profiles/augment_times.json]

--room adds the two ops of the call with a bank (profiles/augment_room.md): ALIAS on every row, FIR on every row at 512, 2048 and
8192 taps (with the fraction of the 157.3 TFLOP/s fp32 matrix peak the executed multiply-adds amount to), recipes as
`Augmenter(p=1, transforms=ALL_TRANSFORMS)` draws them, the ten old transforms through the call with a bank, and `step_resident` with
the ten and with the twelve transforms.

Device calls are event-timed medians behind warm-up runs, with the recipes already on the device and the workspace and the output
reused; `host` and the steps are wall-clock medians around a synchronisation.  SILERO_VAD_AMD_LIB selects another build of the library
(csrc/augment.hpp: -DVAD_AUG_BLOCK=... for another block of the three-pass cascade); the block as built is in the output line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tools.train_step_time import event_ms, wall_ms  # noqa: E402


def room_times(a, r, model, x, lens, out, ws, wavs, labels):
    """the call with a bank: per new op, as drawn, and the resident step"""
    from silero_vad_amd import ALL_TRANSFORMS, Augmenter, DecoderTrainer, TrainingSet, augment
    dev, (B, W) = model.device, x.shape
    rng = np.random.default_rng(1)
    scratch = torch.empty(augment.augment_scratch_bytes(B, W), dtype=torch.uint8, device=dev)
    all12 = Augmenter(p=1.0, seed=0, transforms=ALL_TRANSFORMS)
    taps = (512, 2048, 8192)
    bank, offs, _ = augment.fir_bank([(rng.standard_normal(K) * np.exp(-np.arange(K) / (K / 6.0)) / np.sqrt(K)).astype(np.float32) for K in taps])
    cases = {"alias": (augment.make_recipes([[("alias", 11025, 16000)]] * B), bank),
             "mixed12_p1": (all12.draw(B), all12.bank), "mixed10_p1_through_x": (Augmenter(p=1.0, seed=0).draw(B), bank)}
    for K, o in zip(taps, offs):
        cases[f"fir_{K}"] = (augment.make_recipes([[("fir", int(o), K)]] * B), bank)
    r["scratch_MB"], r["device_x_ms"], r["fir_fraction_of_fp32_matrix_peak"] = scratch.numel() / 1e6, {}, {}
    for name, (rec, bk) in cases.items():
        rec_dev, bank_dev = torch.from_numpy(rec.view(np.uint8).copy()).to(dev), torch.from_numpy(bk).to(dev)
        ms = event_ms(lambda: augment.augment_device(model.engine, x, lens, rec_dev, out=out, workspace=ws, bank=bank_dev, scratch=scratch), a.reps)
        r["device_x_ms"][name] = ms
    empty = r["device_x_ms"]["mixed10_p1_through_x"] - r["device_ms"]["mixed_p1"]      # (the nine launches that find nothing to do)
    r["device_x_ms"]["nine_idle_launches"] = empty
    for K in taps:
        # executed per workgroup of 4096 outputs: ceil((K' + 15) / 16) groups, K' = min(K, the last output's index + 1), of sixteen
        # instructions in every wave that has outputs (1024 each), 2 x 16 x 16 x 4 flop an instruction
        mfma = sum(-(-(min(K, n0 + 4096, W) + 15) // 16) * 16 * min(4, -(-(W - n0) // 1024)) for n0 in range(0, W, 4096))
        flop = B * mfma * 2048.0
        r["fir_fraction_of_fp32_matrix_peak"][str(K)] = flop / ((r["device_x_ms"][f"fir_{K}"] - r["device_ms"]["empty"]) * 1e-3) / 157.3e12
    if not a.no_step:
        ts = TrainingSet(wavs, labels, model, max_train_length_sec=W / 16000)
        idx = list(range(B))
        for name, aug in (("ten", Augmenter(p=1.0, seed=0)), ("twelve", all12)):
            trainer = DecoderTrainer(model, max_train_length_sec=W / 16000)
            rec = aug.draw(B, row_keys=idx)
            bk = aug.bank_on(dev) if aug.needs_bank else None
            r[f"step_resident_{name}_ms"] = wall_ms(lambda: trainer.step_resident(ts, idx, recipes=rec, bank=bk).item(), a.reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="128x250")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--room", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from silero_vad_amd import Augmenter, DecoderTrainer, augment, load_silero_vad
    model = load_silero_vad(device=0)
    dev = model.device
    rng = np.random.default_rng(0)
    B, T = (int(v) for v in a.shape.split("x"))
    W = T * 512
    wavs = [(0.1 * rng.standard_normal(W)).astype(np.float32) for _ in range(B)]
    labels = [rng.integers(0, 2, size=T).astype(np.uint8) for _ in range(B)]
    x_host = np.stack(wavs)
    x = torch.from_numpy(x_host).to(dev)
    lens = torch.full((B,), W, dtype=torch.int64, device=dev)
    out = torch.empty((B, W), dtype=torch.float32, device=dev)
    ws = torch.empty(augment.augment_workspace_bytes(B, W), dtype=torch.uint8, device=dev)
    eq = np.stack([augment.biquad_design(k, 16000, f, 1.0, g) for k, f, g in
                   (("lowshelf", 100, 6.0), ("peaking", 200, -6.0), ("peaking", 400, 6.0), ("peaking", 800, -6.0), ("peaking", 1600, 6.0),
                    ("peaking", 3200, -6.0), ("highshelf", 6400, 6.0), ("peaking", 50, 24.0))])
    kinds = {"mixed_p1": Augmenter(p=1.0, seed=0).draw(B), "empty": augment.make_recipes([[]] * B),
             "noise": augment.make_recipes([[("noise", 0.01, 1)]] * B), "biquads_1": augment.make_recipes([[("biquads", eq[:1])]] * B),
             "biquads_8": augment.make_recipes([[("biquads", eq)]] * B), "clip": augment.make_recipes([[("clip", 0.1, 0.9)]] * B),
             "three_ops": augment.make_recipes([[("noise", 0.01, 1), ("clip", 0.1, 0.9), ("biquads", eq)]] * B)}
    r = {"B": B, "T": T, "block": augment.block_size(), "workspace_MB": ws.numel() / 1e6, "device_ms": {}}
    for name, rec in kinds.items():
        rec_dev = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
        r["device_ms"][name] = event_ms(lambda: augment.augment_device(model.engine, x, lens, rec_dev, out=out, workspace=ws), a.reps)
    print(json.dumps(r), flush=True)
    if a.room:
        room_times(a, r, model, x, lens, out, ws, wavs, labels)
        print(json.dumps(r), flush=True)
    if not a.no_host:
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            augment.augment_host(x_host, [W] * B, kinds["mixed_p1"], threads=a.host_threads)
            host.append((time.perf_counter() - t0) * 1e3)
        r["host_mixed_p1_ms"], r["host_threads"] = float(np.median(host)), a.host_threads
    if not a.no_step:
        trainer = DecoderTrainer(model, max_train_length_sec=W / 16000)
        r["step_ms"] = wall_ms(lambda: trainer.step(wavs, labels), a.reps)
        r["step_with_recipes_ms"] = wall_ms(lambda: trainer.step(wavs, labels, recipes=kinds["mixed_p1"]), a.reps)
        aug = Augmenter(p=1.0, seed=0)
        r["draw_ms"] = wall_ms(lambda: aug.draw(B), a.reps)
    print(json.dumps(r), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(r, indent=1))


if __name__ == "__main__":
    main()
