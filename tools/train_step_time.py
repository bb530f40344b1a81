#!/usr/bin/env python3
"""Times of one decoder training step on the GPU (silero_vad_amd/tuning.py), per part and whole, beside the same step written with
torch.nn.LSTMCell and autograd on the same GPU -- what the reference's train() costs a user who sets device: 'cuda'.

    python tools/train_step_time.py [--shapes 128x250,1024x250] [--reps 10] [--resident] [--out profiles/decoder_training_times.json]

Every figure is the median of `reps` runs behind warm-up runs.  `encode` and the gradient call (its six kernels together) are
event-timed as calls; the whole `.step` (padding, upload, encode, mask, gradient call, Adam) and the torch step are wall-clock times
around a synchronisation, host time included, as a user sees them.  The torch step starts from features already on the device: it is
the decoder's share alone.

--resident adds, in the same process: the one-time upload of a `TrainingSet` holding the batch's recordings, an epoch of `reps`
`step_resident` calls (optimizer="fused_adam") with ONE synchronisation at its end -- the median per-step time of five such epochs --
its ratio to `.step`, and batch assembly (vad_trainset_batch_device) and the fused Adam step event-timed on their own.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def event_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def wall_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


class TorchDecoder(torch.nn.Module):
    """the reference's decoder, from its description: LSTMCell(128, 128), Dropout(0.1), ReLU, a 128 -> 1 linear map, Sigmoid"""

    def __init__(self):
        super().__init__()
        self.rnn = torch.nn.LSTMCell(128, 128)
        self.drop = torch.nn.Dropout(0.1)
        self.head = torch.nn.Linear(128, 1)

    def forward(self, feat):
        h = c = feat.new_zeros((feat.shape[0], 128))
        out = []
        for t in range(feat.shape[1]):
            h, c = self.rnn(feat[:, t], (h, c))
            out.append(torch.sigmoid(self.head(torch.relu(self.drop(h)))))
        return torch.cat(out, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x250,1024x250")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from silero_vad_amd import DecoderTrainer, TrainingSet, decoder_grad, decoder_grad_workspace_bytes, load_silero_vad
    model = load_silero_vad(device=0)
    dev = model.device
    rng = np.random.default_rng(0)
    rows = []
    for shape in a.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        wavs = [(0.1 * rng.standard_normal(T * 512)).astype(np.float32) for _ in range(B)]
        labels = [rng.integers(0, 2, size=T).astype(np.uint8) for _ in range(B)]
        x = torch.from_numpy(np.stack(wavs)).to(dev)
        trainer = DecoderTrainer(model, max_train_length_sec=T * 512 / 16000)
        feat = model.encode(x, 16000)
        lab = torch.from_numpy(np.stack(labels)).to(dev)
        nck = torch.full((B,), T, dtype=torch.int64, device=dev)
        keep = (torch.rand((B, T, 128), device=dev) >= 0.1).to(torch.uint8)
        ws = torch.empty(decoder_grad_workspace_bytes(B, T), dtype=torch.uint8, device=dev)
        r = {"B": B, "T": T, "workspace_MB": ws.numel() / 1e6}
        r["encode_ms"] = event_ms(lambda: model.encode(x, 16000), a.reps)
        r["grad_call_ms"] = event_ms(lambda: decoder_grad(model.engine, trainer.params, feat, nck, lab, keep, 1 / 0.9, 0.5, None, ws, False), a.reps)
        r["step_ms"] = wall_ms(lambda: trainer.step(wavs, labels), a.reps)
        ref = TorchDecoder().to(dev)
        opt = torch.optim.Adam(ref.parameters(), lr=5e-4)
        target, mask = lab.float(), torch.where(lab == 1, 1.0, 0.5)

        def torch_step():
            loss = (torch.nn.functional.binary_cross_entropy(ref(feat), target, reduction="none") * mask).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss

        r["torch_decoder_step_ms"] = wall_ms(torch_step, max(2, a.reps // 3), warm=1)
        if a.resident:
            del ref, opt, x, feat
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ts = TrainingSet(wavs, labels, model, max_train_length_sec=T * 512 / 16000)
            r["trainset_upload_ms"], r["trainset_MB"] = (time.perf_counter() - t0) * 1e3, ts.nbytes / 1e6
            fused = DecoderTrainer(model, max_train_length_sec=T * 512 / 16000, optimizer="fused_adam")
            idx = list(range(B))

            def resident_epoch():
                for _ in range(a.reps):
                    fused.step_resident(ts, idx)

            r["resident_step_ms"] = wall_ms(resident_epoch, 5, warm=1) / a.reps
            r["resident_over_host"] = r["resident_step_ms"] / r["step_ms"]
            r["batch_ms"] = event_ms(lambda: ts.batch(idx), a.reps)
            r["fused_adam_ms"] = event_ms(fused.optimizer.step, a.reps)
            r["torch_adam_ms"] = event_ms(trainer.optimizer.step, a.reps)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
