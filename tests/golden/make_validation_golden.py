#!/usr/bin/env python3
"""Generate golden_validation.npz / .json: labelled validation sets and what the REAL reference's validate() returns on them.

Runs only in the authoring container: it takes `validate`, `VADDecoderRNNJIT`, `AverageMeter` and `SileroVadPadder` out of the
unmodified reference file /root/reference/tuning/utils.py (their AST alone is executed -- the module's other imports, torchaudio and
pandas, are not installed) and runs them with the reference's real silero_vad.jit (its _model / _model_8k submodules), the decoder's
own state dict, nn.BCELoss(reduction='none') and a plain list of batches as the loader.  Only data goes into the repository.

Audio sets (e2e_16k, e2e_8k): the committed speech fixtures cut into 7 recordings of unequal length, one of them not a whole number
of chunks (zero-padded as load_speech_sample pads); labels from `chunk_labels` of the reference's default segments; batch size 3, noise
loss 0.5.  A chunk whose reference probability leaves q < 1e-3 (q = p for label 1, 1 - p for label 0) gets label 255 and mask 0: an
engine within 2e-5 of the reference has no bounded loss term there.  At most 1 % of a set's chunks may go that way.
Recorded: cut points, labels, batch size, the reference's predictions, the pair validate() returned, sklearn's unrounded AUC,
close_pairs (positive / negative pairs whose reference probabilities differ by at most 4e-5: only those can change sides under an
engine within 2e-5), loss_bound = sum(mask 2e-5 / (q - 2e-5)) / numel, the distance of the host twin on the reference's predictions.
The unrounded AUC must keep close_pairs / (n_pos n_neg) away from a 3-decimal rounding boundary; else a shorter stretch is taken.

Probability-level sets (no audio; references: roc_auc_score, BCELoss and the reference's padder / meter on the probabilities):
  ties      -- values from a 9-value set that includes exact 0.0 and 1.0
  one_ulp   -- positive / negative pairs one ulp apart, on both sides of a binade and of multiples of 2^14 (and 2^12) in the bit pattern
  tiny      -- 1 ... 3 chunks per recording
  saturated -- 1 - 2^-k and 2^-k
  random12  -- the threshold fixture's twelve noisy recordings
"""
import ast
import gc
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn
from sklearn.metrics import roc_auc_score

REF = Path("/root/reference")
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))

from silero_vad_amd import chunk_labels, chunk_scores  # noqa: E402

BATCH, NOISE, IGNORE = 3, 0.5, 255
WANTED = ("validate", "VADDecoderRNNJIT", "AverageMeter", "SileroVadPadder")


def reference_defs():
    tree = ast.parse((REF / "tuning" / "utils.py").read_text())
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in WANTED]
    assert sorted(n.name for n in body) == sorted(WANTED)
    ns = {"np": np, "torch": torch, "nn": nn, "gc": gc, "roc_auc_score": roc_auc_score, "tqdm": lambda x, **kw: x}
    exec(compile(ast.Module(body=body, type_ignores=[]), "tuning/utils.py", "exec"), ns)
    return ns


def as_batch(rows):
    T = max(1, max(len(r) for r in rows))
    x = np.zeros((len(rows), T), dtype=np.float32)
    for i, r in enumerate(rows):
        x[i, :len(r)] = r
    return x, [len(r) for r in rows]


def masks_of(labels):
    return [np.where(l == 1, 1.0, np.where(l == 0, NOISE, 0.0)) for l in labels]


def loader_of(ns, items):
    return [ns["SileroVadPadder"](items[a:a + BATCH]) for a in range(0, len(items), BATCH)]


def reference_loss(ns, probs, labels):
    """the loop body of validate() on given probabilities: BCELoss(reduction='none'), (loss * masks).mean(), the meter"""
    crit, meter = nn.BCELoss(reduction="none"), ns["AverageMeter"]()
    items = [(torch.from_numpy(p), torch.FloatTensor(np.where(l == 1, 1.0, 0.0)), torch.from_numpy(m)) for p, l, m in zip(probs, labels, masks_of(labels))]
    for x, targets, masks in loader_of(ns, items):
        loss = (crit(x, targets) * masks).mean()
        meter.update(loss.item(), masks.numel())
    return float(meter.avg)


def reference_sums(probs, labels):
    """per recording the sums of BCELoss's fp32 terms by label, accumulated in double"""
    crit = nn.BCELoss(reduction="none")
    pos, neg = [], []
    for p, l in zip(probs, labels):
        t = crit(torch.from_numpy(p), torch.FloatTensor(np.where(l == 1, 1.0, 0.0))).double().numpy()
        pos.append(float(t[l == 1].sum()))
        neg.append(float(t[l == 0].sum()))
    return np.asarray(pos), np.asarray(neg)


def close_pairs(p, l, width=4e-5):
    neg = np.sort(p[l == 0].astype(np.float64))
    pos = p[l == 1].astype(np.float64)
    return int((np.searchsorted(neg, pos + width, side="right") - np.searchsorted(neg, pos - width, side="left")).sum())


def describe(ns, probs, labels):
    """what every set records beside its arrays"""
    y = np.concatenate(labels)
    x = np.concatenate(probs)
    ok = y <= 1
    auc = float(roc_auc_score(y[ok], x[ok]))
    loss = reference_loss(ns, probs, labels)
    s = chunk_scores(*as_batch(probs), labels)
    twin = s.loss(NOISE, BATCH)
    rp, rn = reference_sums(probs, labels)
    both = np.concatenate([rp, rn])
    got = np.concatenate([s.bce_pos, s.bce_neg])
    rel = np.abs(got - both)[both > 0] / both[both > 0]
    assert abs(s.roc_auc() - auc) <= 2.0 ** -50 * auc
    return {"recordings": len(probs), "auc": auc, "pair": [loss, round(auc, 3)], "batch_size": BATCH, "noise_loss": NOISE,
            "n_pos": int((y == 1).sum()), "n_neg": int((y == 0).sum()), "twin_loss_distance": abs(twin - loss),
            "twin_sum_distance": float(rel.max()) if len(rel) else 0.0}, rp, rn


def e2e(ns, jit, tag, sr):
    n = 512 if sr == 16000 else 256
    pcm_all = np.load(HERE / f"audio_{tag}.npz")["pcm"]
    seg = json.loads((HERE / "golden_segments.json").read_text())[tag]
    ts = [{"start": s["start"] / sr, "end": s["end"] / sr} for s in seg["timestamps"]["default"]["out"]]
    lab_all = chunk_labels(ts, seg["n_samples"], sr)
    decoder = ns["VADDecoderRNNJIT"]()
    decoder.load_state_dict((jit._model_8k if sr == 8000 else jit._model).decoder.state_dict())
    config = types.SimpleNamespace(tune_8k=sr == 8000)
    crit = nn.BCELoss(reduction="none")
    whole = len(pcm_all) // n
    for chunks in (whole, whole * 3 // 4, whole // 2, whole // 3, whole // 5):
        # 7 recordings of unequal length; the fourth ends a third of a chunk early and is padded
        w = np.asarray([5, 2, 9, 1, 6, 3, 4], dtype=np.float64)
        lens = np.maximum(1, np.floor(w / w.sum() * chunks).astype(np.int64))
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]) * n
        samples = lens * n
        samples[3] -= n // 3
        wavs, labels = [], []
        for a, m, c in zip(starts, samples, lens):
            wav = pcm_all[a:a + m].astype(np.float32) / 32768.0
            if len(wav) % n:
                wav = np.pad(wav, (0, n - len(wav) % n), "constant", constant_values=0)
            assert len(wav) == c * n
            wavs.append(wav)
            labels.append(lab_all[a // n:a // n + c].copy())

        def run(labels_now):
            items = [(torch.FloatTensor(wv), torch.FloatTensor(np.where(l == 1, 1.0, 0.0)), torch.from_numpy(m))
                     for wv, l, m in zip(wavs, labels_now, masks_of(labels_now))]
            return ns["validate"](config, loader_of(ns, items), jit, decoder, crit, torch.device("cpu"))

        # pass 1, every chunk scored: the reference's predictions come back through roc_auc_score's inputs (all masks non-zero)
        seen = {}
        ns["roc_auc_score"] = lambda gts, predicts: seen.update(p=list(predicts)) or roc_auc_score(gts, predicts)
        run(labels)
        ns["roc_auc_score"] = roc_auc_score
        flat = np.asarray(seen["p"], dtype=np.float32)
        assert len(flat) == int(lens.sum()) and np.array_equal(flat.astype(np.float64), np.asarray(seen["p"]))
        probs = np.split(flat, np.cumsum(lens)[:-1])
        ignored = 0
        for p, l in zip(probs, labels):
            q = np.where(l == 1, p.astype(np.float64), 1.0 - p.astype(np.float64))
            ignored += int((q < 1e-3).sum())
            l[q < 1e-3] = IGNORE
        assert ignored <= 0.01 * len(flat), (ignored, len(flat))
        pair = run(labels)                                     # pass 2: the recorded pair, the hard chunks masked out
        info, rp, rn = describe(ns, probs, labels)
        y, x = np.concatenate(labels), flat
        ok = y <= 1
        cp = close_pairs(x[ok], y[ok])
        margin = cp / (info["n_pos"] * info["n_neg"])
        edge = abs(info["auc"] * 1000 - np.floor(info["auc"] * 1000) - 0.5) / 1000
        numel = sum(len(lens[a:a + BATCH]) * int(lens[a:a + BATCH].max()) for a in range(0, len(lens), BATCH))
        q = np.where(y == 1, x.astype(np.float64), 1.0 - x.astype(np.float64))[ok]
        mask = np.where(y == 1, 1.0, NOISE)[ok]
        print(tag, "chunks", chunks, "ignored", ignored, "pair", pair, "auc", info["auc"], "close pairs", cp, "margin", margin, "distance to a rounding boundary", edge)
        if edge <= margin:
            continue
        assert abs(pair[0] - info["pair"][0]) <= 1e-12 and pair[1] == info["pair"][1], (pair, info["pair"])
        info.update(pair=[float(pair[0]), float(pair[1])], tag=tag, sampling_rate=sr, starts=[int(a) for a in starts], samples=[int(m) for m in samples],
                    ignored=ignored, close_pairs=cp, auc_bound=margin, loss_bound=float((mask * 2e-5 / (q - 2e-5)).sum() / numel), numel=int(numel))
        return info, probs, labels, rp, rn
    raise SystemExit(f"{tag}: no stretch keeps its AUC away from a rounding boundary")


def bits(v):
    return np.asarray(v, dtype=np.uint32).view(np.float32)


def prob_sets(rng):
    sets = {}
    vals = np.asarray([0.0, 1.0, 0.5, 0.25, 0.75, 1e-3, 0.999, 0.3, 0.7], dtype=np.float32)
    lens = [40, 7, 111, 64, 65, 300]
    sets["ties"] = ([rng.choice(vals, size=m) for m in lens], [(rng.random(m) < 0.5).astype(np.uint8) for m in lens])
    # one ulp apart: v and v + 1 with the negative below, above and on the positive; v at binade and at 2^14 / 2^12 multiples
    at = [0x3F000000, 0x3E800000, 0x3F7FFFFF] + [k << 14 for k in (1, 2, 40000, 65000)] + [k << 12 for k in (3, 200001)]
    p, l = [], []
    for v in at:
        for a, b in ((v - 1, v), (v, v - 1), (v, v + 1), (v + 1, v), (v, v)):
            p += [a, b]
            l += [1, 0]
    # shuffled over the recordings, so that every recording's sums hold terms of ordinary size: this torch's BCELoss evaluates
    # log1p(-p) where the rule subtracts in fp32 -- up to 2^-24 apart per label-0 chunk, but all there is of a sum of p < 2^-24 alone
    order = rng.permutation(len(p))
    p, l = bits(p)[order], np.asarray(l, dtype=np.uint8)[order]
    cuts = [10, 30, 31, 50]
    sets["one_ulp"] = (np.split(p, cuts), np.split(l, cuts))
    lens = [int(rng.integers(1, 4)) for _ in range(12)]
    sets["tiny"] = ([rng.random(m, dtype=np.float32) for m in lens], [(rng.random(m) < 0.5).astype(np.uint8) for m in lens])
    sets["tiny"][1][0][:] = 1
    sets["tiny"][1][1][:] = 0
    k = np.arange(1, 25)
    sat = np.concatenate([1.0 - 2.0 ** -k, 2.0 ** -k, 2.0 ** -np.arange(25, 120, 7)]).astype(np.float32)
    lens = [30, 90, 200]
    sets["saturated"] = ([rng.choice(sat, size=m) for m in lens], [(rng.random(m) < 0.5).astype(np.uint8) for m in lens])
    z = np.load(HERE / "golden_thresholds.npz")
    cuts = np.cumsum(z["random12_lens"])[:-1]
    sets["random12"] = (np.split(z["random12_probs"], cuts), np.split(z["random12_labels"], cuts))
    return sets


def main():
    ns = reference_defs()
    jit = torch.jit.load(str(REF / "src" / "silero_vad" / "data" / "silero_vad.jit"), map_location="cpu")
    jit.eval()
    torch.set_grad_enabled(False)
    rng = np.random.default_rng(20261)
    arrays, meta = {}, {"datasets": {}}

    def keep(name, info, probs, labels, rp, rn):
        arrays[f"{name}_probs"] = np.concatenate(probs).astype(np.float32)
        arrays[f"{name}_labels"] = np.concatenate(labels).astype(np.uint8)
        arrays[f"{name}_lens"] = np.asarray([len(p) for p in probs], dtype=np.int64)
        arrays[f"{name}_bce_pos"], arrays[f"{name}_bce_neg"] = rp, rn
        meta["datasets"][name] = info
        print(name, info)

    for tag, sr in (("16k", 16000), ("8k", 8000)):
        keep(f"e2e_{tag}", *e2e(ns, jit, tag, sr))
    for name, (probs, labels) in prob_sets(rng).items():
        assert all(p.dtype == np.float32 and l.dtype == np.uint8 and len(p) == len(l) for p, l in zip(probs, labels))
        info, rp, rn = describe(ns, probs, labels)
        keep(name, info, probs, labels, rp, rn)
    np.savez_compressed(HERE / "golden_validation.npz", **arrays)
    (HERE / "golden_validation.json").write_text(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
