#!/usr/bin/env python3
"""Generate golden_thresholds.npz / .json: labelled datasets and what the REAL reference's threshold search returns on them.

Runs only in the authoring container: it takes the one function `calculate_best_thresholds` out of the unmodified reference file
/root/reference/tuning/utils.py (the function's AST alone is executed, with numpy and this machine's sklearn.metrics.accuracy_score
-- the module's other imports, torchaudio and pandas, are not installed) and records its returned (enter, exit, accuracy) for every
dataset.  Only data goes into the repository: probabilities, labels, the returned triples.

Datasets (float32 probabilities, uint8 0 / 1 labels, 1 ... 12 recordings each):
  * wav_16k, wav_8k -- the reference's own per-chunk probabilities of the speech fixtures (golden_{16k,8k}.npz probs_wav), labels
                       from `chunk_labels` of the reference's default get_speech_timestamps segments (golden_segments.json)
  * planted         -- random rows with probabilities planted exactly on, one ulp above and one ulp below the float32 roundings (up
                       and down) of every grid value
  * tiny            -- recordings of 1 ... 3 chunks
  * round4          -- one recording of exactly 20 000 chunks: 19 989 correct (0.99945) at the first good pairs, 3 more at their
                       neighbours with a higher enter threshold -- the 4-digit rounding decides which pair is returned
  * tie             -- clean recordings on which many pairs tie at the rounded mean: the strict > and the iteration order decide
  * random12        -- twelve noisy recordings of 30 ... 300 chunks
`e2e` names the stretch of the 16 kHz fixture whose reference probabilities keep 2e-5 (the engine-vs-reference bound) away from the grid
values named there, so that an engine's probabilities give the same counts and the same triple.
"""
import ast
import json
import sys
from pathlib import Path

import numpy as np
from sklearn.metrics import accuracy_score

REF = Path("/root/reference")
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))

from silero_vad_amd import chunk_labels, threshold_pairs  # noqa: E402


def reference_function():
    tree = ast.parse((REF / "tuning" / "utils.py").read_text())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "calculate_best_thresholds"]
    assert len(fn) == 1
    ns = {"np": np, "accuracy_score": accuracy_score, "tqdm": lambda x, **kw: x}
    exec(compile(ast.Module(body=fn, type_ignores=[]), "tuning/utils.py", "exec"), ns)
    return ns["calculate_best_thresholds"]


def run(fn, probs, labels):
    e, x, a = fn([p.tolist() for p in probs], [l.tolist() for l in labels])
    return [float(e), float(x), float(a)]


def noisy(rng, n, flip=0.05):
    """a plausible recording: runs of speech / silence, probabilities around them, a few chunks mislabelled"""
    lab = np.zeros(n, dtype=np.uint8)
    t, on = 0, bool(rng.integers(2))
    while t < n:
        m = int(rng.integers(1, 25))
        lab[t:t + m] = on
        t, on = t + m, not on
    p = np.where(lab == 1, rng.beta(5, 1.5, n), rng.beta(1.5, 5, n)).astype(np.float32)
    bad = rng.random(n) < flip
    lab[bad] ^= 1
    return p, lab


def planted(rng):
    grid = np.linspace(0, 1, 20)
    vals = []
    for g in grid:
        f = np.float32(g)
        up = f if float(f) >= g else np.nextafter(f, np.float32(np.inf))
        dn = f if float(f) <= g else np.nextafter(f, np.float32(-np.inf))
        for c in (up, dn):
            vals += [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]
    vals = np.clip(np.asarray(vals, dtype=np.float32), 0.0, 1.0)
    probs, labels = [], []
    for r in range(7):
        n = int(rng.integers(60, 400))
        p, lab = noisy(rng, n, 0.1)
        at = rng.choice(n, size=min(n // 2, len(vals)), replace=False)
        p[at] = rng.permutation(vals)[:len(at)]
        probs.append(p)
        labels.append(lab)
    return probs, labels


def round4():
    n = 20000
    lab = np.zeros(n, dtype=np.uint8)
    p = np.full(n, 0.02, dtype=np.float32)
    for a in range(100, n - 100, 400):                      # speech runs of 150 chunks
        lab[a:a + 150] = 1
        p[a:a + 150] = 0.9
        p[a + 150:a + 160] = 0.1                            # leaves only with exit >= 0.1
    wrong = np.arange(8) * 400 + 300                        # loud chunks labelled silence: wrong at every pair that scores at all
    p[wrong] = 0.97
    p[wrong + 1] = 0.0                                      # ... and off again at once
    edge = np.arange(3) * 400 + 8300                        # silence at 0.40: right only where enter > 0.40
    p[edge] = 0.40
    p[edge + 1] = 0.0
    return [p], [lab]


def e2e_choice(probs, segs, sr, fn):
    """the longest leading stretch of the fixture whose reference probabilities stay 2e-5 away from every INNER grid value: an engine
    within 2e-5 of the reference then decides every chunk alike at every pair whose thresholds are inner ones -- the best pair, its
    bracket and all the rest of them.  Speech reaches probabilities within 2e-5 of 1, so the pairs with exit = 0 or enter = 1 (crossed
    only by a probability of exactly 0 or 1) are not covered by that; what is recorded and asserted for them is that in the reference
    their best mean accuracy lies far below the returned one."""
    from silero_vad_amd import threshold_counts
    grid = np.linspace(0, 1, 20)
    pr = threshold_pairs()
    n = 512 if sr == 16000 else 256
    for chunks in (len(probs), 1250, 940, 625, 310):
        p = probs[:chunks]
        d = np.abs(p.astype(np.float64)[:, None] - grid[None, 1:-1]).min()
        lab = chunk_labels([{"start": s["start"] / sr, "end": s["end"] / sr} for s in segs], chunks * n, sr)
        tri = run(fn, [p], [lab])
        acc = threshold_counts(p[None], [chunks], [lab], pr).accuracy()[0]
        outer = float(acc[(pr.exit == 0) | (pr.enter == 1)].max())
        print("e2e", chunks, "min distance to an inner grid value", d, "best accuracy of a pair with exit 0 or enter 1:", outer, tri)
        if d > 2e-5 and outer < tri[2] - 0.05:
            return {"tag": "16k", "n_samples": chunks * n, "triple": tri, "min_inner_grid_distance": float(d), "best_outer_pair_accuracy": outer}
    raise SystemExit("no stretch of the fixture keeps its distance from the grid")


def main():
    fn = reference_function()
    rng = np.random.default_rng(20260)
    seg = json.loads((HERE / "golden_segments.json").read_text())
    sets = {}
    for tag, sr in (("16k", 16000), ("8k", 8000)):
        p = np.load(HERE / f"golden_{tag}.npz")["probs_wav"]
        ts = [{"start": s["start"] / sr, "end": s["end"] / sr} for s in seg[tag]["timestamps"]["default"]["out"]]
        lab = chunk_labels(ts, seg[tag]["n_samples"], sr)
        assert len(lab) == len(p)
        sets[f"wav_{tag}"] = ([p], [lab])
    sets["planted"] = planted(rng)
    tiny = [noisy(rng, int(rng.integers(1, 4)), 0.2) for _ in range(12)]
    sets["tiny"] = ([t[0] for t in tiny], [t[1] for t in tiny])
    sets["round4"] = round4()
    clean = []
    for n in (40, 77, 130):
        p, lab = noisy(rng, n, 0.0)
        clean.append((np.where(lab == 1, 0.8, 0.2).astype(np.float32), lab))
    sets["tie"] = ([c[0] for c in clean], [c[1] for c in clean])
    many = [noisy(rng, int(rng.integers(30, 301))) for _ in range(12)]
    sets["random12"] = ([m[0] for m in many], [m[1] for m in many])

    arrays, meta = {}, {"datasets": {}}
    for name, (probs, labels) in sets.items():
        assert all(p.dtype == np.float32 and l.dtype == np.uint8 and len(p) == len(l) and set(np.unique(l)) <= {0, 1} for p, l in zip(probs, labels))
        tri = run(fn, probs, labels)
        print(name, [len(p) for p in probs], tri)
        arrays[f"{name}_probs"] = np.concatenate(probs)
        arrays[f"{name}_labels"] = np.concatenate(labels)
        arrays[f"{name}_lens"] = np.asarray([len(p) for p in probs], dtype=np.int64)
        meta["datasets"][name] = {"recordings": len(probs), "triple": tri}
    # the tie really is one: more than one pair reaches the returned mean
    from silero_vad_amd import threshold_counts
    pr = threshold_pairs()
    for name in ("tie", "round4"):
        probs, labels = sets[name]
        T = max(len(p) for p in probs)
        batch = np.zeros((len(probs), T), dtype=np.float32)
        for i, p in enumerate(probs):
            batch[i, :len(p)] = p
        acc = threshold_counts(batch, [len(p) for p in probs], labels, pr).accuracy()
        print(name, "pairs at the highest plain mean accuracy:", int((acc.mean(axis=0) == acc.mean(axis=0).max()).sum()),
              "distinct accuracies:", np.unique(acc)[-4:])
    meta["e2e"] = e2e_choice(np.load(HERE / "golden_16k.npz")["probs_wav"], seg["16k"]["timestamps"]["default"]["out"], 16000, fn)
    np.savez_compressed(HERE / "golden_thresholds.npz", **arrays)
    (HERE / "golden_thresholds.json").write_text(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
