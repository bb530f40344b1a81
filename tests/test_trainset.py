"""Resident training without a GPU: `TrainingSet.batch_host` (vad_trainset_batch_host, csrc/trainset.cpp; the rule is
csrc/trainset.hpp) against `DecoderTrainer._batch` bit for bit, the argument errors of the two twins, and the Adam twin
(vad_decoder_adam_host) against a float64 numpy statement of torch.optim.Adam's rule over five consecutive steps.

`adam_reference_distance` is the yardstick of the GPU test (tests/test_trainset_gpu.py): what torch.optim.Adam on the CPU in float32
is away from the float64 rule after one step from the same float32 state.  It is computed live, never stored.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_tuning import NAMES, SHAPES, fixture, published

LENGTHS = (1, 255, 511, 512, 513, 4095, 4096, 4097, 8193)
SEC = 0.256                       # 4 096 samples at 16 kHz: 8 chunks
LR, BETA1, BETA2, EPS = 5e-4, 0.9, 0.999, 1e-8


def corpus(kind, seed=11):
    """recordings of LENGTHS samples: all int16, all float32, or mixed (every third int16, one float64); a label per chunk of the cut"""
    rng = np.random.default_rng(seed)
    audios = []
    for k, n in enumerate(LENGTHS):
        if kind == "int16" or (kind == "mixed" and k % 3 == 0):
            audios.append(rng.integers(-32768, 32768, size=n).astype(np.int16))
        elif kind == "mixed" and k == 4:
            audios.append(rng.uniform(-1, 1, size=n))
        else:
            audios.append(rng.uniform(-1, 1, size=n).astype(np.float32))
    labels = [rng.integers(0, 2, size=(min(n, 4096) + 511) // 512).astype(np.uint8) for n in LENGTHS]
    return audios, labels


def host_trainer(sec=SEC, sr=16000):
    """a DecoderTrainer as far as `_batch` needs one: no model, no device"""
    from silero_vad_amd import DecoderTrainer
    t = DecoderTrainer.__new__(DecoderTrainer)
    t.sampling_rate, t.chunk, t.max_samples = sr, 512 if sr == 16000 else 256, int(sec * sr)
    return t


def raw_batch_host(arena, offs, lens, label_arena, label_offs, idx, max_samples, chunk, ld, ldl, fill=0x5A):
    """vad_trainset_batch_host on plain arrays, outputs pre-filled: (rc, pcm [B, ld], labels [B, ldl], lens [B], n_chunks [B])"""
    from silero_vad_amd import _lib
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    B = len(idx)
    pcm = np.frombuffer(bytes([fill]) * (B * ld * arena.itemsize), dtype=arena.dtype).reshape(B, ld).copy()
    lab = np.full((B, ldl), fill, np.uint8)
    out_lens, out_nck = np.full(B, -7, np.int64), np.full(B, -7, np.int64)
    rc = _lib.lib().vad_trainset_batch_host(arena.ctypes.data, arena.itemsize, offs.ctypes.data, lens.ctypes.data, label_arena.ctypes.data,
                                            label_offs.ctypes.data, len(lens), idx.ctypes.data, B, max_samples, chunk, pcm.ctypes.data, ld,
                                            lab.ctypes.data, ldl, out_lens.ctypes.data, out_nck.ctypes.data)
    return rc, pcm, lab, out_lens, out_nck


INDEX_LISTS = ([0, 1, 2, 3, 4, 5, 6, 7, 8], [8, 3, 3, 0], [5], [0], [0, 0], [7, 6, 5, 4, 3, 2, 1, 0, 8, 8, 1, 2, 3, 4, 5, 6, 7])


@pytest.mark.parametrize("kind", ["int16", "float32", "mixed"])
def test_batch_host_is_the_trainers_batch(built, kind):
    from silero_vad_amd import TrainingSet
    audios, labels = corpus(kind)
    ts = TrainingSet(audios, labels, None, max_train_length_sec=SEC)
    assert len(ts) == len(LENGTHS) and ts.dtype == (np.int16 if kind == "int16" else np.float32)
    assert ts.lens.tolist() == [min(n, 4096) for n in LENGTHS] and ts.n_chunks.tolist() == [(min(n, 4096) + 511) // 512 for n in LENGTHS]
    assert ts.nbytes >= int(ts.lens.sum()) * ts.dtype.itemsize + int(ts.n_chunks.sum())
    trainer = host_trainer()
    for idx in INDEX_LISTS:
        pcm, nck, lab, T = ts.batch_host(idx)
        w_pcm, w_nck, w_lab, w_T = trainer._batch([audios[i] for i in idx], [labels[i] for i in idx])
        if w_pcm.dtype != ts.dtype:
            # `_batch` picks int16 per BATCH, the set per CORPUS: a batch of int16 recordings only, out of a mixed corpus, is the
            # same samples under the rule's own conversion (exact: an int16 over 2^15 is a float32)
            assert kind == "mixed" and all(audios[i].dtype == np.int16 for i in idx)
            w_pcm = w_pcm.astype(np.float32) / 32768.0
        assert T == w_T and pcm.dtype == w_pcm.dtype and pcm.shape == w_pcm.shape
        assert pcm.tobytes() == w_pcm.tobytes() and np.array_equal(nck, w_nck) and np.array_equal(lab, w_lab)
    assert ts.batch_host([0])[3] == 1                                          # the 1-sample recording alone: T = 1
    assert ts.batch_host(torch.tensor([1, 0]))[3] == 1


def test_batch_host_8k_and_tensors(built):
    """the 8 kHz geometry (chunks of 256) and recordings given as tensors"""
    from silero_vad_amd import TrainingSet
    rng = np.random.default_rng(3)
    audios = [torch.from_numpy(rng.uniform(-1, 1, size=n).astype(np.float32)) for n in (1, 256, 257, 2049)]
    labels = [rng.integers(0, 2, size=(min(n, 2048) + 255) // 256).astype(np.uint8) for n in (1, 256, 257, 2049)]
    ts = TrainingSet(audios, labels, None, sampling_rate=8000, max_train_length_sec=SEC)
    got, want = ts.batch_host([3, 1, 0, 2]), host_trainer(sr=8000)._batch([audios[i] for i in (3, 1, 0, 2)], [labels[i] for i in (3, 1, 0, 2)])
    assert got[3] == want[3] == 8 and all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3]))


def test_argument_errors(built):
    from silero_vad_amd import TrainingSet, _lib, decoder_adam_host
    audios, labels = corpus("float32")
    ts = TrainingSet(audios, labels, None, max_train_length_sec=SEC)
    for bad in ([9], [-1], [0, 12]):
        with pytest.raises(IndexError):
            ts.batch_host(bad)
    with pytest.raises(ValueError):
        ts.batch_host([])
    with pytest.raises(ValueError, match="labels for"):
        TrainingSet(audios, [l[:-1] if k == 6 else l for k, l in enumerate(labels)], None, max_train_length_sec=SEC)
    with pytest.raises(ValueError, match="non-empty"):
        TrainingSet(audios + [np.zeros(0, np.float32)], labels + [np.zeros(0, np.uint8)], None, max_train_length_sec=SEC)
    with pytest.raises(ValueError):
        TrainingSet(audios, labels[:-1], None, max_train_length_sec=SEC)
    with pytest.raises(ValueError):
        TrainingSet(audios, labels, None, sampling_rate=44100)
    with pytest.raises(RuntimeError):
        ts.batch([0])                                                           # a set without a model lives on the host
    # the C twin itself: an index out of range, ldl < T, ld < len, empty shapes, NULL -- and nothing written
    arena, lab_arena = ts._arena_host.numpy(), ts._labels_host

    def call(idx=(8, 0), max_samples=4096, chunk=512, ld=4096, ldl=8):
        return raw_batch_host(arena, ts.offs, ts.lens, lab_arena, ts.label_offs, idx, max_samples, chunk, ld, ldl)

    assert call()[0] == 0
    for kw in (dict(idx=(0, 9)), dict(idx=(-1,)), dict(ldl=7), dict(ld=4095), dict(chunk=0), dict(ld=0), dict(ldl=0), dict(max_samples=-1)):
        rc, pcm, lab, ln, nck = call(**kw)
        assert rc == 1, kw
        assert np.all(pcm.view(np.uint8) == 0x5A) and np.all(lab == 0x5A) and np.all(ln == -7) and np.all(nck == -7), kw
    assert call(idx=(0, 1), ldl=1, ld=512)[0] == 0                              # the pitches need only hold the batch's own rows
    L = _lib.lib()
    assert L.vad_trainset_batch_host(None, 4, None, None, None, None, 1, None, 1, 1, 1, None, 1, None, 1, None, None) == 1
    assert L.vad_trainset_batch_device(None, None, 4, None, None, None, None, 1, None, 1, 1, 1, None, 1, None, 1, None, None, None) == 1
    blob = open(_lib.WEIGHTS_PATH, "rb").read()
    host = ctypes.c_void_p()
    assert L.vad_create_host_only(blob, len(blob), ctypes.byref(host)) == 0
    assert L.vad_trainset_batch_device(host, None, 4, None, None, None, None, 1, None, 1, 1, 1, None, 1, None, 1, None, None, None) == 4
    assert L.vad_decoder_adam_device(host, None, None, None, None, 1, LR, BETA1, BETA2, EPS, None) == 4
    assert L.vad_decoder_adam_device(None, None, None, None, None, 1, LR, BETA1, BETA2, EPS, None) == 1
    L.vad_destroy(host)
    # Adam: step counts from 1
    p, g, m, v = adam_problem()[:4]
    before = {n: p[n].copy() for n in NAMES}
    for kw in (dict(step=0), dict(step=-3), dict(step=1, beta1=1.0), dict(step=1, beta2=-0.1), dict(step=1, lr=float("nan")), dict(step=1, eps=-1.0)):
        with pytest.raises(_lib.VadError) as e:
            decoder_adam_host(p, g, m, v, **kw)
        assert e.value.status == 1 and all(np.array_equal(p[n], before[n]) for n in NAMES)
    with pytest.raises(ValueError):
        decoder_adam_host(p, {n: g[n].astype(np.float32) for n in NAMES}, m, v, 1)
    with pytest.raises(ValueError):
        decoder_adam_host(p, g, {**m, NAMES[2]: np.zeros(3)}, v, 1)


# ---- Adam --------------------------------------------------------------------------------------------------------------------------------
def adam_gradients(step, rng):
    """the fixture's recorded float64 gradients where it records them (the matrices at its 2 048 coordinates, the small tensors whole),
    seeded normal gradients of mixed scale elsewhere; then, in every tensor that has room, the elements the rule is probed with: an
    exact zero at [0] (and at [1], where the parameter is 0), 1e-8 at [2], 1e4 at [3]"""
    z, _ = fixture()
    g = {}
    for k, (n, shape) in enumerate(zip(NAMES, SHAPES)):
        a = rng.standard_normal(int(np.prod(shape))) * 10.0 ** rng.integers(-6, 2, size=int(np.prod(shape)))
        rec = z[f"e2e_16k_grad64_{n}"].astype(np.float64).reshape(-1) * (1.0 + 0.25 * step)
        if k < 2:
            a[z["idx"]] = rec
        else:
            a[:] = rec
        if a.size >= 4:
            a[0], a[1], a[2], a[3] = 0.0, 0.0, 1e-8 * rng.standard_normal(), 1e4 * rng.standard_normal()
        g[n] = a.reshape(shape)
    return g


def adam_problem(seed=21):
    """(params, grads of step 1, m, v) as float64 arrays; the parameters are the published decoder with p[1] = 0 in every tensor"""
    rng = np.random.default_rng(seed)
    p = {n: np.ascontiguousarray(v, dtype=np.float64).copy() for n, v in published().items()}
    for n in NAMES:
        if p[n].size >= 4:
            p[n].reshape(-1)[1] = 0.0
    g = adam_gradients(0, rng)
    return p, g, {n: np.zeros_like(p[n]) for n in NAMES}, {n: np.zeros_like(p[n]) for n in NAMES}, rng


def adam_rule64(p, g, m, v, step):
    """torch.optim.Adam's default rule in float64 numpy (no amsgrad, no weight decay, not maximize) -> new (p, m, v)"""
    m = m + (g - m) * (1.0 - BETA1)
    v = BETA2 * v + (1.0 - BETA2) * g * g
    p = p - (LR / (1.0 - BETA1 ** step)) * m / (np.sqrt(v) / np.sqrt(1.0 - BETA2 ** step) + EPS)
    return p, m, v


def torch_adam32(p, g, m, v, step):
    """one step of torch.optim.Adam on the CPU in float32 from the float32 state (p, m, v) with gradient g -> new (p, m, v)"""
    tp = torch.from_numpy(np.array(p, dtype=np.float32)).requires_grad_(False)
    opt = torch.optim.Adam([tp], lr=LR, betas=(BETA1, BETA2), eps=EPS)
    opt.state[tp] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(np.array(m, dtype=np.float32)),
                     "exp_avg_sq": torch.from_numpy(np.array(v, dtype=np.float32))}
    tp.grad = torch.from_numpy(np.array(g, dtype=np.float32))
    opt.step()
    assert float(opt.state[tp]["step"]) == step
    return tp.numpy(), opt.state[tp]["exp_avg"].numpy(), opt.state[tp]["exp_avg_sq"].numpy()


def adam_reference_distance(state32, step):
    """d_ref[tensor][quantity]: the Euclidean distance of torch.optim.Adam (CPU, float32, one step from the float32 state `state32` =
    (p, g, m, v) dicts) from the float64 rule on the same state, per tensor and separately for p, m and v; where torch lands on the
    float64 result exactly, one float32 ulp of the tensor's largest magnitude.  Also returns the float64 result."""
    p, g, m, v = state32
    d, want = {}, {}
    for n in NAMES:
        a64 = [np.asarray(x[n], dtype=np.float64) for x in (p, g, m, v)]
        w = adam_rule64(a64[0], a64[1], a64[2], a64[3], step)
        t = torch_adam32(p[n], g[n], m[n], v[n], step)
        want[n] = dict(zip("pmv", w))
        d[n] = {}
        for q, wq, tq in zip("pmv", w, t):
            dist = float(np.linalg.norm(tq.astype(np.float64) - wq))
            d[n][q] = dist if dist > 0.0 else float(np.spacing(np.float32(np.abs(wq).max())))
    return d, want


def adam_trajectory(steps=5):
    """the twin's run over `steps` steps in double: yields (step, float64 state before the step (p, g, m, v), the twin's state after)"""
    from silero_vad_amd import decoder_adam_host
    p, g, m, v, rng = adam_problem()
    for step in range(1, steps + 1):
        before = tuple({n: x[n].copy() for n in NAMES} for x in (p, g, m, v))
        decoder_adam_host(p, g, m, v, step, LR, BETA1, BETA2, EPS)
        yield step, before, tuple({n: x[n].copy() for n in NAMES} for x in (p, m, v))
        g = adam_gradients(step, rng)


def test_adam_twin_against_the_float64_rule(built):
    """5 consecutive steps of the twin against the numpy rule run beside it (1e-12 relative, per tensor and quantity), and the yardstick
    the GPU test uses: torch's own float32 step is a finite, small distance from the rule"""
    ref = None
    for step, (p, g, m, v), after in adam_trajectory(5):
        if ref is None:
            ref = tuple({n: x[n].copy() for n in NAMES} for x in (p, m, v))
        for n in NAMES:
            ref[0][n], ref[1][n], ref[2][n] = adam_rule64(ref[0][n], g[n], ref[1][n], ref[2][n], step)
            for q, got, want in zip("pmv", (after[0][n], after[1][n], after[2][n]), (ref[0][n], ref[1][n], ref[2][n])):
                err = float(np.linalg.norm(got - want))
                assert err <= 1e-12 * float(np.linalg.norm(want)), (step, n, q, err)
            if p[n].size >= 4:
                flat = lambda a: a[n].reshape(-1)
                assert flat(g)[0] == 0.0 and (step > 1 or flat(after[0])[0] == flat(p)[0])     # a zero gradient at step 1: p stays
                assert flat(after[0])[1] == 0.0 if step == 1 else True                         # ... and a zero parameter stays zero
        s32 = tuple({n: x[n].astype(np.float32) for n in NAMES} for x in (p, g, m, v))
        d_ref, _ = adam_reference_distance(s32, step)
        for n in NAMES:
            for q in "pmv":
                scale = max(float(np.linalg.norm(after["pmv".index(q)][n])), 1e-30)
                print("step", step, n, q, "torch fp32 to the float64 rule, relative:", d_ref[n][q] / scale)
                assert 0.0 < d_ref[n][q] <= 1e-5 * scale + 1e-30
    # step 1 starts the state: whatever m and v held
    from silero_vad_amd import decoder_adam_host
    p, g, m, v, _ = adam_problem()
    dirty_m, dirty_v = {n: np.full_like(m[n], 3.0) for n in NAMES}, {n: np.full_like(v[n], 5.0) for n in NAMES}
    p2 = {n: p[n].copy() for n in NAMES}
    decoder_adam_host(p, g, m, v, 1, LR, BETA1, BETA2, EPS)
    decoder_adam_host(p2, g, dirty_m, dirty_v, 1, LR, BETA1, BETA2, EPS)
    assert all(np.array_equal(p[n], p2[n]) and np.array_equal(m[n], dirty_m[n]) and np.array_equal(v[n], dirty_v[n]) for n in NAMES)


def test_reference_sampling_seed_repeats():
    """the seed tests/test_trainset_gpu.py fixes for sampling='reference': 64 draws from [0, 64) with a repeat among them"""
    g = torch.Generator()
    g.manual_seed(3)
    order = torch.randint(0, 64, (64,), generator=g).tolist()
    assert len(order) == 64 and all(0 <= i < 64 for i in order) and len(set(order)) < 64
