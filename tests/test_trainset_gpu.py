"""Resident training on the GPU: the batch kernel (vad_trainset_batch_device, csrc/kernel_trainset.hip) against its host twin bit for
bit; `step_resident` against `step` bit for bit; the fused Adam (vad_decoder_adam_device) one step at a time against its twin with
torch's own float32 distance from the float64 rule as the yardstick (test_trainset.adam_reference_distance, computed live); `epoch`
over a `TrainingSet`, reference sampling, the tune_8k flow, and twenty fused steps on the tuning fixture.
Everything here needs a real MI355X:  python -m pytest tests -m gpu

Fused Adam, measured on an MI355X (device to twin over torch-CPU-float32 to the float64 rule; the bound is 4): 0.999997 ... 1.000004
over six tensors x (p, m, v) x steps 1, 2, 5.  The ratios are printed in front of the assertion; profiles/decoder_training.md holds a
run's.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_trainset import (BETA1, BETA2, EPS, LENGTHS, LR, SEC, adam_reference_distance, adam_trajectory, corpus, raw_batch_host)
from test_tuning import NAMES, fixture
from test_tuning_gpu import fixture_recordings

pytestmark = pytest.mark.gpu

FILL = 0x5A


@pytest.fixture(scope="module")
def model(built):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback to silently pass on)")
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    assert m.engine._h, "native engine not created"
    return m


def raw_batch_device(model, arena, offs, lens, label_arena, label_offs, idx, max_samples, chunk, ld, ldl, arena_offset=0):
    """vad_trainset_batch_device on device copies of plain arrays, outputs pre-filled with FILL; arena_offset: elements the arena
    pointer is advanced by inside its allocation (the arrays given are already cut there)"""
    from silero_vad_amd import _lib
    dev = model.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pad = np.zeros(arena_offset, arena.dtype)
    d_arena, d_offs, d_lens, d_lab, d_loffs = up(np.concatenate([pad, arena])), up(offs), up(lens), up(label_arena), up(label_offs)
    d_idx = up(np.asarray(idx, dtype=np.int64))
    B = len(idx)
    pcm = torch.full((B, ld * arena.itemsize), FILL, dtype=torch.uint8, device=dev)
    lab = torch.full((B, ldl), FILL, dtype=torch.uint8, device=dev)
    out = torch.full((2, B), -7, dtype=torch.int64, device=dev)
    rc = _lib.lib().vad_trainset_batch_device(model.engine._h, d_arena.data_ptr() + arena_offset * arena.itemsize, arena.itemsize, d_offs.data_ptr(),
                                              d_lens.data_ptr(), d_lab.data_ptr(), d_loffs.data_ptr(), len(lens), d_idx.data_ptr(), B, max_samples,
                                              chunk, pcm.data_ptr(), ld, lab.data_ptr(), ldl, out[0].data_ptr(), out[1].data_ptr(),
                                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return rc, pcm.cpu().numpy().view(arena.dtype).reshape(B, ld), lab.cpu().numpy(), out[0].cpu().numpy(), out[1].cpu().numpy()


def index_list(B):
    return [(5 * b + 3) % len(LENGTHS) for b in range(B)] if B > 1 else [8]


def packed_back_to_back(audios, labels, dtype, max_samples, chunk):
    """the recordings cut and packed with no padding between them: (arena, offs, lens, label arena, label offs)"""
    cut = [np.asarray(a)[:max_samples] for a in audios]
    cut = [a if a.dtype == dtype else (a.astype(np.float32) / (32768.0 if a.dtype == np.int16 else 1.0)).astype(dtype) for a in cut]
    lens = np.asarray([len(a) for a in cut], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    nck = (lens + chunk - 1) // chunk
    return np.concatenate(cut), offs, lens, np.concatenate([l[:n] for l, n in zip(labels, nck)]).astype(np.uint8), \
        np.concatenate([[0], np.cumsum(nck)[:-1]]).astype(np.int64)


@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("kind", ["int16", "float32", "mixed"])
def test_batch_kernel_against_twin(model, kind, B):
    from silero_vad_amd import TrainingSet
    audios, labels = corpus(kind)
    ts = TrainingSet(audios, labels, model, max_train_length_sec=SEC)
    idx = index_list(B)
    T = int(ts.n_chunks[idx].max())
    # the public route
    pcm, lens, nck, lab, T_dev = ts.batch(idx)
    w_pcm, w_nck, w_lab, w_T = ts.batch_host(idx)
    assert T_dev == w_T == T and pcm.is_cuda and lens.dtype == nck.dtype == torch.int64
    assert pcm.cpu().numpy().tobytes() == w_pcm.tobytes() and np.array_equal(nck.cpu().numpy(), w_nck) and np.array_equal(lab.cpu().numpy(), w_lab)
    assert np.array_equal(lens.cpu().numpy(), ts.lens[idx])
    # the raw call: pitches larger than needed over pre-filled outputs -- a vector pitch and one that is no multiple of 16 bytes --
    # on the set's own arena (every recording from a 16-byte boundary) and on recordings packed back to back from an odd sample
    # (sources at 2-byte alignment for int16, at 4- but not 16-byte alignment for float32)
    tight = packed_back_to_back(audios, labels, ts.dtype, ts.max_samples, ts.chunk)
    assert any((o + 1) * ts.dtype.itemsize % 16 for o in tight[1])
    for name, arrays, shift in (("set", (ts._arena_host.numpy(), ts.offs, ts.lens, ts._labels_host, ts.label_offs), 0), ("odd", tight, 1)):
        for ld, ldl in ((T * 512 + 24, T + 5), (T * 512 + 3, T + 1)):
            want = raw_batch_host(*arrays, idx, ts.max_samples, ts.chunk, ld, ldl, fill=FILL)
            got = raw_batch_device(model, *arrays, idx, ts.max_samples, ts.chunk, ld, ldl, arena_offset=shift)
            again = raw_batch_device(model, *arrays, idx, ts.max_samples, ts.chunk, ld, ldl, arena_offset=shift)
            assert want[0] == 0 and got[0] == 0 and again[0] == 0, name
            for w, g, a in zip(want[1:], got[1:], again[1:]):
                assert w.tobytes() == g.tobytes() == a.tobytes(), (name, ld, ldl)
            # whole pitch: nothing of the fill is left, zeros behind the cut, 255 behind the chunks
            for b, r in enumerate(idx):
                assert np.all(got[1][b, ts.lens[r]:] == 0) and np.all(got[2][b, ts.n_chunks[r]:] == 255)
            assert np.array_equal(got[3], ts.lens[idx]) and np.array_equal(got[4], ts.n_chunks[idx])


def test_batch_row_does_not_depend_on_its_place(model):
    from silero_vad_amd import TrainingSet
    for kind in ("int16", "float32"):
        audios, labels = corpus(kind)
        ts = TrainingSet(audios, labels, model, max_train_length_sec=SEC)
        idx17 = index_list(16) + [6]
        one, many = ts.batch([6]), ts.batch(idx17)
        assert one[4] == many[4] == 8
        for a, b in zip(one[:4], many[:4]):
            assert torch.equal(a[0], b[16])
        # an index outside the set cannot be refused by the device: the raw call gives an empty row, and leaves its neighbours alone
        arrays = (ts._arena_host.numpy(), ts.offs, ts.lens, ts._labels_host, ts.label_offs)
        rc, pcm, lab, lens, nck = raw_batch_device(model, *arrays, [6, 9, -1, 5], ts.max_samples, ts.chunk, 4096, 8)
        good = raw_batch_host(*arrays, [6, 5], ts.max_samples, ts.chunk, 4096, 8)
        assert rc == 0 and lens.tolist() == [4096, 0, 0, 4095] and nck.tolist() == [8, 0, 0, 8]
        assert not pcm[1:3].any() and np.all(lab[1:3] == 255)
        assert pcm[[0, 3]].tobytes() == good[1].tobytes() and np.array_equal(lab[[0, 3]], good[2])


def test_batch_device_argument_errors(model):
    from silero_vad_amd import TrainingSet, _lib
    audios, labels = corpus("int16")
    ts = TrainingSet(audios, labels, model, max_train_length_sec=SEC)
    L, e, dev = _lib.lib(), model.engine._h, model.device
    pcm = torch.full((2, 4096), 7, dtype=torch.int16, device=dev)
    lab = torch.full((2, 8), 7, dtype=torch.uint8, device=dev)
    out = torch.full((2, 2), 7, dtype=torch.int64, device=dev)
    idx = torch.tensor([0, 8], device=dev)

    def call(arena=ts._arena.data_ptr(), esz=2, n=len(ts), i=idx.data_ptr(), B=2, mx=4096, chunk=512, p=pcm.data_ptr(), ld=4096, ldl=8):
        return L.vad_trainset_batch_device(e, arena, esz, ts._tables[0].data_ptr(), ts._tables[1].data_ptr(), ts._labels.data_ptr(),
                                           ts._tables[2].data_ptr(), n, i, B, mx, chunk, p, ld, lab.data_ptr(), ldl, out[0].data_ptr(),
                                           out[1].data_ptr(), None)

    for kw in (dict(arena=None), dict(esz=3), dict(n=0), dict(i=None), dict(B=0), dict(mx=-1), dict(chunk=0), dict(p=None), dict(ld=0), dict(ldl=0),
               dict(arena=ts._arena.data_ptr() + 1), dict(p=pcm.data_ptr() + 1), dict(i=idx.data_ptr() + 4)):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert torch.all(pcm == 7) and torch.all(lab == 7) and torch.all(out == 7)       # nothing was queued
    assert call() == 0
    torch.cuda.synchronize()
    assert out.tolist() == [[1, 4096], [1, 8]]


# ---- the routes ---------------------------------------------------------------------------------------------------------------------------
def small_corpus(golden, n=5):
    """float32 recordings cut out of the golden speech, of lengths either side of the chunk and of the 0.256 s cut"""
    wav = golden["16k"]["wav"]
    lens = [4096, 1500, 513, 4097, 8193, 512, 2048][:n]
    rng = np.random.default_rng(4)
    audios = [wav[20000 + 3001 * k: 20000 + 3001 * k + m].copy() for k, m in enumerate(lens)]
    labels = [rng.integers(0, 2, size=(min(m, 4096) + 511) // 512).astype(np.uint8) for m in lens]
    return audios, labels


@pytest.mark.parametrize("augmented", [False, True], ids=["plain", "recipes"])
def test_step_resident_is_step(model, golden, augmented):
    from silero_vad_amd import Augmenter, DecoderTrainer, TrainingSet
    audios, labels = small_corpus(golden)
    ts = TrainingSet(audios, labels, model, max_train_length_sec=SEC)
    host, res = (DecoderTrainer(model, max_train_length_sec=SEC, seed=5) for _ in range(2))
    aug_h, aug_r = (Augmenter(p=1.0, seed=9) for _ in range(2))
    for idx in ([0, 1, 2], [3, 4, 0, 2], [2, 2, 1]):
        loss_h = host.step([audios[i] for i in idx], [labels[i] for i in idx], recipes=aug_h.draw(len(idx), row_keys=idx) if augmented else None)
        loss_r = res.step_resident(ts, idx, recipes=aug_r.draw(len(idx), row_keys=idx) if augmented else None)
        assert torch.is_tensor(loss_r) and loss_r.is_cuda and loss_r.dim() == 0 and loss_r.dtype == torch.float64
        assert float(loss_r.item()) == loss_h
        assert all(torch.equal(host.last_grads[n], res.last_grads[n]) for n in NAMES)
        if augmented:
            assert torch.equal(host.last_augmented, res.last_augmented)
    assert all(torch.equal(host.params[n], res.params[n]) for n in NAMES)


# ---- fused Adam ---------------------------------------------------------------------------------------------------------------------------
def test_fused_adam_one_step_from_identical_state(model):
    """steps 1, 2 and 5 of the twin's trajectory, each from the twin's float32-rounded state: device to twin <= 4 x d_ref"""
    from silero_vad_amd import decoder_adam, decoder_adam_host
    dev = model.device
    for step, before, _ in adam_trajectory(5):
        if step not in (1, 2, 5):
            continue
        s32 = tuple({n: x[n].astype(np.float32) for n in NAMES} for x in before)
        d_ref, _ = adam_reference_distance(s32, step)
        p64, g64, m64, v64 = ({n: x[n].astype(np.float64) for n in NAMES} for x in s32)
        decoder_adam_host(p64, g64, m64, v64, step, LR, BETA1, BETA2, EPS)
        runs = []
        for _ in range(2):
            p, g, m, v = ({n: torch.from_numpy(x[n]).to(dev) for n in NAMES} for x in s32)
            decoder_adam(model.engine, p, g, m, v, step, LR, BETA1, BETA2, EPS)
            torch.cuda.synchronize()
            runs.append({q: {n: t[n].cpu().numpy() for n in NAMES} for q, t in zip("pmv", (p, m, v))})
        for q, want in zip("pmv", (p64, m64, v64)):
            for n in NAMES:
                assert np.array_equal(runs[0][q][n], runs[1][q][n])
                d = float(np.linalg.norm(runs[0][q][n].astype(np.float64) - want[n]))
                print("fused adam step", step, n, q, "device to twin / torch fp32 to the float64 rule:", d / d_ref[n][q])
                assert d <= 4.0 * d_ref[n][q], (step, n, q, d, d_ref[n][q])
        if step == 1:
            for n in NAMES:
                if s32[0][n].size >= 4:
                    assert s32[1][n].reshape(-1)[0] == 0.0 and runs[0]["p"][n].reshape(-1)[0] == s32[0][n].reshape(-1)[0]
    # step 1 starts the state whatever m and v held; a later step uses them
    p, g = ({n: torch.from_numpy(x[n]).to(dev) for n in NAMES} for x in s32[:2])
    dirty = [{n: torch.full_like(p[n], 3.0) for n in NAMES} for _ in range(2)]
    clean = [{n: torch.zeros_like(p[n]) for n in NAMES} for _ in range(2)]
    p2 = {n: p[n].clone() for n in NAMES}
    decoder_adam(model.engine, p, g, dirty[0], dirty[1], 1)
    decoder_adam(model.engine, p2, g, clean[0], clean[1], 1)
    assert all(torch.equal(p[n], p2[n]) and torch.equal(dirty[0][n], clean[0][n]) and torch.equal(dirty[1][n], clean[1][n]) for n in NAMES)
    decoder_adam(model.engine, p, g, dirty[0], dirty[1], 2)
    assert not any(torch.equal(dirty[0][n], clean[0][n]) for n in NAMES)
    from silero_vad_amd import _lib
    with pytest.raises(_lib.VadError):
        decoder_adam(model.engine, p, g, dirty[0], dirty[1], 0)


# ---- epoch --------------------------------------------------------------------------------------------------------------------------------
def test_epoch_over_a_training_set(model, golden):
    from silero_vad_amd import DecoderTrainer, TrainingSet
    audios, labels = small_corpus(golden, 7)
    ts = TrainingSet(audios, labels, model, max_train_length_sec=SEC)
    sgd0 = lambda p: torch.optim.SGD(p, lr=0.0)
    host, res = (DecoderTrainer(model, max_train_length_sec=SEC, dropout=0.0, optimizer=sgd0) for _ in range(2))
    want = host.epoch(audios, labels, batch_size=3, shuffle=False)
    got = res.epoch(ts, batch_size=3, shuffle=False)
    print("epoch losses.avg: host route", want, "resident", got)
    assert abs(got - want) <= 1e-12 * abs(want) and res.last_order == list(range(7))
    with pytest.raises(ValueError):
        res.epoch(ts, labels)
    with pytest.raises(ValueError):
        res.epoch(ts, augment=lambda w: w)
    with pytest.raises(ValueError):
        res.epoch(ts, sampling="bootstrap")
    with pytest.raises(ValueError):
        res.epoch(audios)


def test_reference_sampling_draws_with_replacement(model, golden):
    from silero_vad_amd import DecoderTrainer, TrainingSet
    wav = golden["16k"]["wav"]
    audios = [wav[30000 + 700 * k: 30000 + 700 * k + 512] for k in range(64)]
    labels = [np.asarray([k & 1], np.uint8) for k in range(64)]
    ts = TrainingSet(audios, labels, model, max_train_length_sec=SEC)
    assert len(ts) == 64
    trainer = DecoderTrainer(model, max_train_length_sec=SEC, seed=3)
    loss = trainer.epoch(ts, batch_size=64, sampling="reference")
    order = trainer.last_order
    assert np.isfinite(loss) and len(order) == 64 and all(0 <= i < 64 for i in order) and len(set(order)) < 64
    g = torch.Generator()
    g.manual_seed(3)
    assert order == torch.randint(0, 64, (64,), generator=g).tolist()
    trainer.epoch(ts, batch_size=64)                                            # the default stays a permutation
    assert sorted(trainer.last_order) == list(range(64))


# ---- tune_8k ------------------------------------------------------------------------------------------------------------------------------
def test_tune_8k(model, golden):
    from silero_vad_amd import DecoderTrainer, TrainingSet, resample, resample_device, resample_geometry, resample_table
    audios, labels = small_corpus(golden)
    ts = TrainingSet(audios, labels, model, sampling_rate=16000, max_train_length_sec=SEC)
    trainer = DecoderTrainer(model, sampling_rate=8000, max_train_length_sec=SEC, seed=1)
    idx = [4, 1, 2, 0]
    loss = trainer.step_resident(ts, idx)
    pcm, lens, nck, lab, T = ts.batch(idx)
    x8 = resample_device(model.engine, pcm, lens, 16000, 8000)
    assert tuple(x8.shape) == (4, T * 256)
    assert torch.equal(trainer.last_features, model.encode(x8, 8000)) and np.isfinite(float(loss.item()))
    # live rows against the host `resample` of each recording, within the resampler's documented bound; zeros behind
    O, N, W, K = resample_geometry(16000, 8000)
    taps, first = resample_table(16000, 8000)
    got = x8.cpu().numpy()
    for b, r in enumerate(idx):
        x = audios[r][:ts.max_samples].astype(np.float64)
        want = resample(audios[r][:ts.max_samples], 16000, 8000)
        m = np.arange(len(want))
        assert len(want) == (len(x) + 1) // 2
        p = ((m // N) * O + first[m % N] - W)[:, None] + np.arange(K)[None, :]
        xs = np.where((p >= 0) & (p < len(x)), np.abs(x)[np.clip(p, 0, len(x) - 1)], 0.0)
        bound = (K + 1) * 2.0 ** -24 * (np.abs(taps[m % N].astype(np.float64)) * xs).sum(axis=1)
        assert np.all(np.abs(got[b, :len(want)].astype(np.float64) - want) <= bound) and not got[b, len(want):].any()
    ts8 = TrainingSet([a[::2] for a in audios], labels, model, sampling_rate=8000, max_train_length_sec=SEC)
    with pytest.raises(ValueError):
        DecoderTrainer(model, sampling_rate=16000, max_train_length_sec=SEC).step_resident(ts8, [0])


# ---- twenty steps -------------------------------------------------------------------------------------------------------------------------
def test_fused_training_lowers_validation_loss(model, golden):
    """20 steps (Adam 5e-4, dropout 0.1, seed 3) on the tuning fixture's six 16 kHz recordings, the host route (torch's Adam) and the
    resident route (optimizer='fused_adam') in the same run.  On record (MI355X): host route 0.29908 -> 0.10876367, resident and fused
    0.10876368 (profiles/decoder_training.md); both are printed."""
    from silero_vad_amd import DecoderTrainer, TrainingSet, validate
    z, _ = fixture()
    wavs, d = fixture_recordings(golden, "e2e_16k")
    labels = np.split(z["e2e_16k_clean_labels"], np.cumsum(d["chunks"])[:-1])
    base_loss, _ = validate(wavs, labels, model, 16000)
    host = DecoderTrainer(model, seed=3)
    for _ in range(20):
        host.step(wavs, labels)
    host_loss, _ = validate(wavs, labels, host.model(), 16000)
    ts = TrainingSet(wavs, labels, model)
    res = DecoderTrainer(model, seed=3, optimizer="fused_adam")
    idx = list(range(len(wavs)))
    for _ in range(20):
        res.step_resident(ts, idx)
    res_loss, _ = validate(wavs, labels, res.model(), 16000)
    print("validate loss", base_loss, "-> host route", host_loss, ", resident + fused Adam", res_loss)
    assert res_loss < base_loss and res_loss < 1.5 * host_loss
