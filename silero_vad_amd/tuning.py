"""Decoder fine-tuning on the device: the reference's `tuning/` training loop (`train()`, tuning/utils.py:206-249, driven by tune.py).

The reference trains one module, `VADDecoderRNNJIT` -- LSTMCell(128, 128), Dropout(0.1), ReLU, Conv1d(128, 1, 1), Sigmoid -- on the
output of the frozen STFT and encoder.  Here the frozen part is the engine's frontend (`HipSileroVAD.encode`, vad_encode_audio), the
loss and the six gradients come from HIP kernels (`decoder_grad`, vad_decoder_grad_device; csrc/trainer.hpp is the rule), and torch is
plumbing: device tensors, the optimizer, the dropout mask's generator.

    trainer = DecoderTrainer(model)                      # Adam(5e-4), dropout 0.1, noise loss 0.5, 8 s cuts: tuning/config.yml
    trainer.epoch(audios, labels)                        # labels: `chunk_labels` per recording
    trainer.epoch(audios, labels, augment=Augmenter())   # the reference's augmentations, on the device (augment.py)
    tuned = trainer.model()                              # a HipSileroVAD on trainer.weights()

A corpus that is visited every epoch need not cross the link every epoch: `TrainingSet` uploads it once, and `step_resident` / `epoch(trainset)`
cut every batch out of it on the device (vad_trainset_batch_device), optionally with the Adam step in one launch (`optimizer="fused_adam"`,
vad_decoder_adam_device), without a host synchronisation per step:

    trainset = TrainingSet(audios, labels, model)        # one upload
    trainer = DecoderTrainer(model, optimizer="fused_adam")
    trainer.epoch(trainset, augment=Augmenter(), sampling="reference")
"""
import ctypes
import struct
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import lib

H, G = 128, 512
# the reference's state-dict names of the decoder (model._model.decoder.state_dict()), their shapes, the C structs' field order
DECODER_TENSORS = (("rnn.weight_ih", (G, H)), ("rnn.weight_hh", (G, H)), ("rnn.bias_ih", (G,)), ("rnn.bias_hh", (G,)),
                   ("decoder.2.weight", (1, H, 1)), ("decoder.2.bias", (1,)))
DECODER_NAMES = tuple(n for n, _ in DECODER_TENSORS)


def _prefix(sampling_rate: int) -> str:
    if sampling_rate not in (8000, 16000):
        raise ValueError("Supported sampling rates: [8000, 16000]")
    return "_model.decoder." if sampling_rate == 16000 else "_model_8k.decoder."


def _container_index(blob: bytes) -> dict:
    """name -> (byte offset, float count, shape) of an SVADW001 container (tools/export_weights.py)"""
    if blob[:8] != b"SVADW001":
        raise ValueError("not an SVADW001 weight container")
    (n,) = struct.unpack_from("<I", blob, 8)
    out = {}
    for i in range(n):
        name, ndim, d0, d1, d2, d3, off, cnt = struct.unpack_from("<64sI4IQQ", blob, 80 + 100 * i)
        out[name.rstrip(b"\0").decode()] = (off, cnt, (d0, d1, d2, d3)[:ndim])
    return out


def decoder_state_dict(weights: Optional[bytes] = None, sampling_rate: int = 16000) -> dict:
    """The decoder of one rate out of a container (default: the published one) as float32 numpy arrays under the reference's names."""
    blob = open(_lib.WEIGHTS_PATH, "rb").read() if weights is None else bytes(weights)
    index, pre = _container_index(blob), _prefix(sampling_rate)
    return {name: np.frombuffer(blob, "<f4", index[pre + name][1], index[pre + name][0]).reshape(shape).copy() for name, shape in DECODER_TENSORS}


def replace_decoder(weights: bytes, state_dict: dict, sampling_rate: int = 16000) -> bytes:
    """`weights` with the six decoder tensors of `sampling_rate` replaced by `state_dict`'s; every other byte -- the other rate's decoder,
    the encoders, the header with its sha field -- stays as it is."""
    blob = bytearray(weights)
    index, pre = _container_index(bytes(weights)), _prefix(sampling_rate)
    for name, shape in DECODER_TENSORS:
        off, cnt, _ = index[pre + name]
        v = state_dict[name]
        v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        v = np.ascontiguousarray(v, dtype="<f4")
        if v.size != cnt or v.size != int(np.prod(shape)):
            raise ValueError(f"{name}: {v.shape} does not hold {cnt} values")
        blob[off:off + 4 * cnt] = v.tobytes()
    return bytes(blob)


class _Params(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out")]


def _check_shapes(params: dict, what: str):
    for name, shape in DECODER_TENSORS:
        if name not in params:
            raise KeyError(f"{what}: {name} missing")
        if int(np.prod(tuple(params[name].shape))) != int(np.prod(shape)):
            raise ValueError(f"{what}: {name} has shape {tuple(params[name].shape)}, expected {shape}")


def decoder_grad_workspace_bytes(B: int, T: int) -> int:
    return int(lib().vad_decoder_grad_workspace_bytes(int(B), int(T)))


def decoder_grad(engine, params: dict, feat, n_chunks, labels, keep=None, keep_scale: float = 1.0, noise_loss: float = 0.5,
                 denom: Optional[float] = None, workspace=None, want_probs: bool = True):
    """vad_decoder_grad_device: (loss, grads, probs) of one batch on the GPU.

    params: the six float32 cuda tensors under the reference's names; feat [B, T, 128] float32 cuda; n_chunks [B] (any integer
    sequence or an int64 cuda tensor); labels [B, >= T] uint8 (0, 1, anything else = ignored); keep [B, T, 128] uint8 / bool or None;
    denom: default B * T, the reference's `.mean()` over the padded batch.  Returns the loss as a 0-dim float64 cuda tensor (no host
    synchronisation), the gradients as float32 cuda tensors of the parameters' shapes and probs [B, T] (None without want_probs).
    workspace: a uint8 cuda tensor of at least `decoder_grad_workspace_bytes(B, T)` bytes to reuse, else one is made."""
    _check_shapes(params, "params")
    dev = feat.device
    if not (feat.is_cuda and feat.dtype == torch.float32 and feat.dim() == 3 and feat.shape[2] == H and feat.is_contiguous()):
        raise ValueError("feat must be a contiguous float32 cuda tensor [B, T, 128]")
    B, T = int(feat.shape[0]), int(feat.shape[1])
    for name in DECODER_NAMES:
        p = params[name]
        if not (torch.is_tensor(p) and p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
            raise ValueError(f"params[{name!r}] must be a contiguous float32 cuda tensor")
    nck = n_chunks if torch.is_tensor(n_chunks) else torch.as_tensor(np.asarray(n_chunks, dtype=np.int64))
    nck = nck.to(device=dev, dtype=torch.int64).contiguous()
    lab = labels if torch.is_tensor(labels) else torch.as_tensor(np.ascontiguousarray(labels, dtype=np.uint8))
    lab = lab.to(device=dev, dtype=torch.uint8)
    if nck.numel() != B or lab.dim() != 2 or lab.shape[0] != B or lab.shape[1] < T or lab.stride(1) != 1:
        raise ValueError("n_chunks must hold B values and labels must be [B, >= T]")
    if keep is not None:
        keep = keep.to(device=dev).view(torch.uint8) if keep.dtype == torch.bool else keep.to(device=dev, dtype=torch.uint8)
        if tuple(keep.shape) != (B, T, H) or not keep.is_contiguous():
            raise ValueError("keep must be a contiguous [B, T, 128] byte tensor")
    need = decoder_grad_workspace_bytes(B, T)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    grads = {name: torch.empty_like(params[name]) for name in DECODER_NAMES}
    loss = torch.empty((), dtype=torch.float64, device=dev)
    probs = torch.empty((B, T), dtype=torch.float32, device=dev) if want_probs else None
    cp = _Params(*[params[n].data_ptr() for n in DECODER_NAMES])
    cg = _Params(*[grads[n].data_ptr() for n in DECODER_NAMES])
    with torch.cuda.device(dev):
        engine._check(lib().vad_decoder_grad_device(
            engine._h, ctypes.byref(cp), feat.data_ptr(), B, T, nck.data_ptr(), lab.data_ptr(), lab.stride(0) if B > 1 else lab.shape[1],
            None if keep is None else keep.data_ptr(), float(keep_scale), float(noise_loss), float(B * T if denom is None else denom),
            ctypes.byref(cg), loss.data_ptr(), None if probs is None else probs.data_ptr(), workspace.data_ptr(), workspace.numel(),
            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return loss, grads, probs


def decoder_grad_host(params: dict, feat, n_chunks, labels, keep=None, keep_scale: float = 1.0, noise_loss: float = 0.5,
                      denom: Optional[float] = None, threads: int = 0):
    """vad_decoder_grad_host, the device call's twin in double, no GPU: params (any float arrays under the reference's names; taken as
    float64), feat [B, T, 128] float32 -> (loss float, grads float64 numpy arrays of the reference's shapes, probs float32 [B, T])."""
    _check_shapes(params, "params")
    feat = np.ascontiguousarray(feat, dtype=np.float32)
    if feat.ndim != 3 or feat.shape[2] != H:
        raise ValueError("feat must be [B, T, 128]")
    B, T = feat.shape[:2]
    nck = np.ascontiguousarray(n_chunks, dtype=np.int64)
    lab = np.ascontiguousarray(labels, dtype=np.uint8)
    if nck.size != B or lab.ndim != 2 or lab.shape[0] != B or lab.shape[1] < T:
        raise ValueError("n_chunks must hold B values and labels must be [B, >= T]")
    if keep is not None:
        keep = np.ascontiguousarray(keep).astype(np.uint8)
        if keep.shape != (B, T, H):
            raise ValueError("keep must be [B, T, 128]")
    p64 = {n: np.ascontiguousarray(params[n].detach().cpu().numpy() if torch.is_tensor(params[n]) else params[n], dtype=np.float64)
           for n in DECODER_NAMES}
    grads = {n: np.zeros(shape, dtype=np.float64) for n, shape in DECODER_TENSORS}
    loss = ctypes.c_double()
    probs = np.zeros((B, T), dtype=np.float32)
    cp = _Params(*[p64[n].ctypes.data for n in DECODER_NAMES])
    cg = _Params(*[grads[n].ctypes.data for n in DECODER_NAMES])
    rc = lib().vad_decoder_grad_host(ctypes.byref(cp), feat.ctypes.data, B, T, nck.ctypes.data, lab.ctypes.data, lab.shape[1],
                                     None if keep is None else keep.ctypes.data, float(keep_scale), float(noise_loss),
                                     float(B * T if denom is None else denom), ctypes.byref(cg), ctypes.byref(loss), probs.ctypes.data, int(threads))
    if rc:
        raise _lib.VadError(rc, "vad_decoder_grad_host")
    return loss.value, grads, probs


def _struct64(arrays: dict) -> _Params:
    return _Params(*[arrays[n].ctypes.data for n in DECODER_NAMES])


def decoder_adam_host(params: dict, grads: dict, m: dict, v: dict, step: int, lr: float = 5e-4, beta1: float = 0.9, beta2: float = 0.999,
                      eps: float = 1e-8) -> None:
    """vad_decoder_adam_host: torch.optim.Adam's default step in double, in place on `params`, `m`, `v` -- contiguous float64 numpy
    arrays under the reference's names.  step counts from 1; step 1 starts the state (m and v count as zero)."""
    for what, d in (("params", params), ("grads", grads), ("m", m), ("v", v)):
        _check_shapes(d, what)
        for n in DECODER_NAMES:
            a = d[n]
            if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and (what == "grads" or a.flags.writeable)):
                raise ValueError(f"{what}[{n!r}] must be a contiguous float64 numpy array")
    cp, cg, cm, cv = (_struct64(d) for d in (params, grads, m, v))
    rc = lib().vad_decoder_adam_host(ctypes.byref(cp), ctypes.byref(cg), ctypes.byref(cm), ctypes.byref(cv), int(step), float(lr), float(beta1),
                                     float(beta2), float(eps))
    if rc:
        raise _lib.VadError(rc, "vad_decoder_adam_host")


def decoder_adam(engine, params: dict, grads: dict, m: dict, v: dict, step: int, lr: float = 5e-4, beta1: float = 0.9, beta2: float = 0.999,
                 eps: float = 1e-8) -> None:
    """vad_decoder_adam_device on the current stream: one launch over the six tensors (contiguous float32 cuda tensors under the
    reference's names), in place on `params`, `m`, `v`.  step counts from 1 and is the caller's to count; step 1 zeroes m and v first."""
    for what, d in (("params", params), ("grads", grads), ("m", m), ("v", v)):
        _check_shapes(d, what)
        for n in DECODER_NAMES:
            t = d[n]
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError(f"{what}[{n!r}] must be a contiguous float32 cuda tensor")
    dev = params[DECODER_NAMES[0]].device
    cp, cg, cm, cv = (_Params(*[d[n].data_ptr() for n in DECODER_NAMES]) for d in (params, grads, m, v))
    with torch.cuda.device(dev):
        engine._check(lib().vad_decoder_adam_device(engine._h, ctypes.byref(cp), ctypes.byref(cg), ctypes.byref(cm), ctypes.byref(cv), int(step),
                                                    float(lr), float(beta1), float(beta2), float(eps),
                                                    ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))


class FusedAdam:
    """torch.optim.Adam(lr, betas, eps) over the trainer's six tensors as one launch (`decoder_adam`); `step()` reads each tensor's
    `.grad` as a torch optimizer does.  The step count lives on the host; the state is two tensors per parameter."""

    def __init__(self, engine, params: dict, lr: float = 5e-4, betas=(0.9, 0.999), eps: float = 1e-8):
        self.engine, self.params = engine, params
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.m = {n: torch.empty_like(p) for n, p in params.items()}          # zeroed by step 1
        self.v = {n: torch.empty_like(p) for n, p in params.items()}
        self.steps = 0

    def step(self):
        self.steps += 1
        decoder_adam(self.engine, self.params, {n: self.params[n].grad for n in DECODER_NAMES}, self.m, self.v, self.steps, self.lr, *self.betas,
                     self.eps)


def _pinned_upload(a: np.ndarray, device):
    """a small host table to the device without blocking on the stream: through page-locked memory the host allocator recycles"""
    return torch.from_numpy(a).pin_memory().to(device, non_blocking=True)


class TrainingSet:
    """A tuning corpus resident on the device: uploaded once, visited `num_epochs` times.

    audios: 1-D recordings (numpy arrays or tensors) at `sampling_rate`; labels: one `chunk_labels`-style uint8 sequence per recording,
    a label per chunk of the CUT.  The recordings are cut to `max_train_length_sec` here -- nothing behind the cut is ever trained on
    -- and packed, each from a 16-byte boundary, into one arena: int16 if every recording is int16, otherwise float32 with int16 taken
    as / 32768 (`DecoderTrainer._batch`'s rule).  With a `model` the arena is page-locked and uploaded once; `model=None` keeps the set
    on the host (`batch_host` only).  `lens` and `n_chunks` stay on the host as numpy arrays, so a batch's T is known without asking the
    device."""

    def __init__(self, audios: Sequence, labels: Sequence, model=None, sampling_rate: int = 16000, max_train_length_sec: float = 8):
        _prefix(sampling_rate)
        self.sampling_rate = int(sampling_rate)
        self.chunk = 512 if self.sampling_rate == 16000 else 256
        self.max_samples = int(max_train_length_sec * self.sampling_rate)
        cut = [np.asarray(a.cpu() if torch.is_tensor(a) else a)[:self.max_samples] for a in audios]
        if not cut or len(labels) != len(cut):
            raise ValueError("a training set holds at least one recording and one label sequence per recording")
        if any(a.ndim != 1 or a.size == 0 for a in cut):
            raise ValueError("every recording must be a non-empty 1-D array")
        n = self.chunk
        self.lens = np.asarray([a.size for a in cut], dtype=np.int64)
        self.n_chunks = (self.lens + n - 1) // n
        self.dtype = np.dtype(np.int16 if all(a.dtype == np.int16 for a in cut) else np.float32)
        per16 = 16 // self.dtype.itemsize
        self.offs = np.concatenate([[0], np.cumsum((self.lens + per16 - 1) // per16 * per16)[:-1]]).astype(np.int64)
        total = int(self.offs[-1] + (self.lens[-1] + per16 - 1) // per16 * per16)
        self.label_offs = np.concatenate([[0], np.cumsum(self.n_chunks)[:-1]]).astype(np.int64)
        self.model, self.device = model, None if model is None else model.device
        self._arena_host = torch.zeros(total, dtype=torch.int16 if self.dtype == np.int16 else torch.float32, pin_memory=model is not None)
        arena = self._arena_host.numpy()
        self._labels_host = np.empty(int(self.n_chunks.sum()), dtype=np.uint8)
        for r, (a, l) in enumerate(zip(cut, labels)):
            arena[self.offs[r]:self.offs[r] + a.size] = a if a.dtype == self.dtype else a.astype(np.float32) / (32768.0 if a.dtype == np.int16 else 1.0)
            l = np.asarray(l, dtype=np.uint8)[:self.n_chunks[r]]
            if l.size != self.n_chunks[r]:
                raise ValueError(f"recording {r}: {l.size} labels for {self.n_chunks[r]} chunks")
            self._labels_host[self.label_offs[r]:self.label_offs[r] + l.size] = l
        self._tables_host = np.ascontiguousarray(np.stack([self.offs, self.lens, self.label_offs]))
        if model is not None:
            with torch.cuda.device(self.device):
                self._arena = self._arena_host.to(self.device, non_blocking=True)
                self._labels = torch.from_numpy(self._labels_host).to(self.device)
                self._tables = torch.from_numpy(self._tables_host).to(self.device)
                torch.cuda.current_stream(self.device).synchronize()          # the one upload is over when the constructor returns

    def __len__(self) -> int:
        return len(self.lens)

    @property
    def nbytes(self) -> int:
        """bytes the set occupies (on the device, and as many on the host): samples, labels and the three tables"""
        return int(self._arena_host.numel() * self.dtype.itemsize + self._labels_host.nbytes + self._tables_host.nbytes)

    def _index(self, idx) -> np.ndarray:
        i = np.ascontiguousarray(np.asarray(idx.cpu() if torch.is_tensor(idx) else idx).reshape(-1), dtype=np.int64)
        if i.size == 0:
            raise ValueError("a batch takes at least one index")
        if i.min() < 0 or i.max() >= len(self):
            raise IndexError(f"index outside [0, {len(self)})")
        return i

    def batch_host(self, idx):
        """vad_trainset_batch_host: (pcm [B, T * chunk], n_chunks int64 [B], labels uint8 [B, T], T) as numpy arrays -- what
        `DecoderTrainer._batch` makes of the same recordings, bit for bit.  No GPU."""
        i = self._index(idx)
        B, T = len(i), int(self.n_chunks[i].max())
        pcm, lab = np.empty((B, T * self.chunk), dtype=self.dtype), np.empty((B, T), dtype=np.uint8)
        lens, nck = np.empty(B, dtype=np.int64), np.empty(B, dtype=np.int64)
        rc = lib().vad_trainset_batch_host(self._arena_host.numpy().ctypes.data, self.dtype.itemsize, self.offs.ctypes.data, self.lens.ctypes.data,
                                           self._labels_host.ctypes.data, self.label_offs.ctypes.data, len(self), i.ctypes.data, B, self.max_samples,
                                           self.chunk, pcm.ctypes.data, T * self.chunk, lab.ctypes.data, T, lens.ctypes.data, nck.ctypes.data)
        if rc:
            raise _lib.VadError(rc, "vad_trainset_batch_host")
        return pcm, nck, lab, T

    def batch(self, idx):
        """vad_trainset_batch_device on the current stream: idx (a host integer sequence, uploaded as B integers) ->
        (pcm [B, T * chunk] int16 or float32, lens int64 [B], n_chunks int64 [B], labels uint8 [B, T], T), device tensors but T, which
        comes from the host's copy of `n_chunks`: nothing here waits for the device."""
        if self.model is None:
            raise RuntimeError("a TrainingSet built without a model lives on the host: batch_host")
        i = self._index(idx)
        B, T = len(i), int(self.n_chunks[i].max())
        dev, engine = self.device, self.model.engine
        with torch.cuda.device(dev):
            idx_dev = _pinned_upload(i, dev)
            pcm = torch.empty((B, T * self.chunk), dtype=self._arena.dtype, device=dev)
            lab = torch.empty((B, T), dtype=torch.uint8, device=dev)
            out = torch.empty((2, B), dtype=torch.int64, device=dev)
            engine._check(lib().vad_trainset_batch_device(
                engine._h, self._arena.data_ptr(), self.dtype.itemsize, self._tables[0].data_ptr(), self._tables[1].data_ptr(), self._labels.data_ptr(),
                self._tables[2].data_ptr(), len(self), idx_dev.data_ptr(), B, self.max_samples, self.chunk, pcm.data_ptr(), T * self.chunk,
                lab.data_ptr(), T, out[0].data_ptr(), out[1].data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return pcm, out[0], out[1], lab, T


class DecoderTrainer:
    """The reference's `train()` over one rate's decoder, on the device.  The six parameters are float32 cuda tensors started from the
    model's container; `optimizer`: a callable `params -> torch optimizer`, None for torch.optim.Adam(lr=learning_rate), or
    "fused_adam" for the same rule as one launch of ours (`FusedAdam`, vad_decoder_adam_device) with `learning_rate`."""

    def __init__(self, model, sampling_rate: int = 16000, noise_loss: float = 0.5, dropout: float = 0.1, learning_rate: float = 5e-4,
                 max_train_length_sec: float = 8, optimizer=None, seed: int = 0, weights: Optional[bytes] = None):
        if not 0.0 <= dropout < 1.0:
            raise ValueError("dropout must be in [0, 1)")
        self.base_model = model
        self.sampling_rate = int(sampling_rate)
        self.chunk = 512 if self.sampling_rate == 16000 else 256
        self.noise_loss, self.dropout = float(noise_loss), float(dropout)
        self.max_samples = int(max_train_length_sec * self.sampling_rate)
        self.base_weights = bytes(weights) if weights is not None else _model_weights(model)
        self.device = model.device
        sd = decoder_state_dict(self.base_weights, self.sampling_rate)
        self.params = {n: torch.from_numpy(sd[n]).to(self.device).requires_grad_(False) for n in DECODER_NAMES}
        plist = [self.params[n] for n in DECODER_NAMES]
        if isinstance(optimizer, str):
            if optimizer != "fused_adam":
                raise ValueError(f"optimizer: a callable, None or 'fused_adam', got {optimizer!r}")
            self.optimizer = FusedAdam(model.engine, self.params, lr=learning_rate)
        else:
            self.optimizer = torch.optim.Adam(plist, lr=learning_rate) if optimizer is None else optimizer(plist)
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(int(seed))
        self._workspace = None
        self._aug_workspace = None
        self._aug_scratch = None
        self.last_grads = None
        self.last_augmented = None
        self.last_features = None
        self.last_order = None

    def _batch(self, audios, labels):
        n = self.chunk
        cut = [np.asarray(a.cpu() if torch.is_tensor(a) else a)[:self.max_samples] for a in audios]
        if any(a.ndim != 1 or a.size == 0 for a in cut):
            raise ValueError("every recording must be a non-empty 1-D array")
        nck = np.asarray([(a.size + n - 1) // n for a in cut], dtype=np.int64)
        T = int(nck.max())
        dt = np.int16 if all(a.dtype == np.int16 for a in cut) else np.float32
        pcm = np.zeros((len(cut), T * n), dtype=dt)
        lab = np.full((len(cut), T), 255, dtype=np.uint8)
        for b, (a, l) in enumerate(zip(cut, labels)):
            pcm[b, :a.size] = a if a.dtype == dt else a.astype(np.float32) / (32768.0 if a.dtype == np.int16 else 1.0)
            l = np.asarray(l, dtype=np.uint8)[:nck[b]]
            if l.size != nck[b]:
                raise ValueError(f"recording {b}: {l.size} labels for {nck[b]} chunks")
            lab[b, :nck[b]] = l
        return pcm, nck, lab, T

    def _augment(self, x, lens, recipes, bank):
        """`augment_device` with the trainer's workspace; with a bank (recipes that may hold "fir" and "alias" ops) the call with a
        bank, and the trainer's second row buffer beside the workspace"""
        from .augment import augment_device, augment_scratch_bytes, augment_workspace_bytes
        B = int(x.shape[0])
        need = augment_workspace_bytes(B, x.shape[1])
        if self._aug_workspace is None or self._aug_workspace.numel() < need:
            self._aug_workspace = None
            self._aug_workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        if bank is None:
            return augment_device(self.base_model.engine, x, lens, recipes, workspace=self._aug_workspace)
        need = augment_scratch_bytes(B, (int(x.shape[1]) + 3) // 4 * 4)
        if self._aug_scratch is None or self._aug_scratch.numel() < need:
            self._aug_scratch = None
            self._aug_scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        if not torch.is_tensor(bank):
            bank = torch.from_numpy(np.ascontiguousarray(bank, dtype=np.float32)).to(self.device)
        return augment_device(self.base_model.engine, x, lens, recipes, workspace=self._aug_workspace, bank=bank, scratch=self._aug_scratch)

    def step(self, audios: Sequence, labels: Sequence, recipes=None, bank=None):
        """One optimizer step on one batch; returns the batch's loss (a float: one host synchronisation).  recipes: one augmentation
        recipe per recording (augment.RECIPE_DTYPE, e.g. `Augmenter.draw`): the uploaded padded batch goes through `augment_device`
        on the current stream before `encode` -- the recordings are cut to `max_train_length_sec` first, so the augmentation sees the
        cut -- and the augmented batch stays in `last_augmented`.  None: no augmentation.  bank: the taps the recipes' "fir" ops index
        (a float32 array or cuda tensor, e.g. `Augmenter.bank`); with it "fir" and "alias" ops are admitted, without it the call is
        the one it was."""
        pcm, nck, lab, T = self._batch(audios, labels)
        B = len(nck)
        with torch.cuda.device(self.device):
            x = torch.from_numpy(pcm).to(self.device)
            if recipes is not None:
                lens = [min(len(a), self.max_samples) for a in audios]
                x = self._augment(x, lens, recipes, bank)
                self.last_augmented = x
            return float(self._train_on(x, nck, lab, B, T).item())

    def _train_on(self, x, nck, lab, B, T):
        """encode -> keep mask -> loss and gradients -> optimizer on a padded batch that is on the device; the loss as a 0-dim float64
        device tensor, no synchronisation (n_chunks and labels: host arrays, uploaded, or device tensors)"""
        with torch.cuda.device(self.device):
            feat = self.base_model.encode(x, self.sampling_rate)
            self.last_features = feat
            keep = None
            if self.dropout > 0.0:
                keep = (torch.rand((B, T, H), device=self.device, generator=self.generator) >= self.dropout).to(torch.uint8)
            need = decoder_grad_workspace_bytes(B, T)
            if self._workspace is None or self._workspace.numel() < need:
                self._workspace = None
                self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            # the reference pads labels with 0 and masks with 0: padded chunks weigh nothing but count in the mean (denom = B * T)
            loss, grads, _ = decoder_grad(self.base_model.engine, self.params, feat, nck, lab, keep, 1.0 / (1.0 - self.dropout), self.noise_loss,
                                          float(B * T), self._workspace, want_probs=False)
            for name in DECODER_NAMES:
                self.params[name].grad = grads[name]
            self.optimizer.step()
            self.last_grads = grads
            self.last_numel = B * T
            return loss

    def step_resident(self, trainset: "TrainingSet", idx: Sequence, recipes=None, bank=None):
        """`step` on a batch cut out of a resident `TrainingSet`: recordings `idx` (host integers, repeats allowed), the same padded
        batch, augmentation, mask draw, gradients and optimizer step as `step([audios[i] ...], [labels[i] ...], recipes, bank)` -- but the batch
        is assembled on the device and the loss comes back as the 0-dim float64 DEVICE tensor: nothing here synchronises, so the host
        runs ahead (drawing the next recipes) while the device works.
        tune_8k: a trainer at sampling_rate 8000 on a set at 16000 augments at 16 kHz, then resamples 16000 -> 8000 on the device
        (`resample_device`, live lengths ceil(len / 2)) and encodes at 8000, as the reference's tune_8k flow does with
        Resample(16000, 8000) behind its augmentations; the chunk counts and labels are the set's (ceil(ceil(L / 2) / 256) ==
        ceil(L / 512)).  The resampler's arithmetic is this project's `resample`, not torchaudio's bits.  Any other
        mismatch of rates is a ValueError."""
        down = trainset.sampling_rate != self.sampling_rate
        if down and (trainset.sampling_rate, self.sampling_rate) != (16000, 8000):
            raise ValueError(f"a {trainset.sampling_rate} Hz training set cannot feed a {self.sampling_rate} Hz trainer: the rates match, or "
                             "the set is at 16000 and the trainer at 8000 (tune_8k)")
        if trainset.model is None or trainset.device != self.device:
            raise ValueError("the training set must be resident on the trainer's device")
        with torch.cuda.device(self.device):
            x, lens, nck, lab, T = trainset.batch(idx)
            B = int(x.shape[0])
            if recipes is not None:
                from .augment import _recipes_array, check_recipes
                if not torch.is_tensor(recipes):
                    r = _recipes_array(recipes, B)
                    check_recipes(r, None if bank is None else int(bank.numel() if torch.is_tensor(bank) else np.size(bank)))
                    recipes = _pinned_upload(r.view(np.uint8).reshape(-1), self.device)
                x = self._augment(x, lens, recipes, bank)
                self.last_augmented = x
            if down:
                from .streams import resample_device
                x = resample_device(self.base_model.engine, x, lens, 16000, 8000)
            return self._train_on(x, nck, lab, B, T)

    def epoch(self, audios, labels: Optional[Sequence] = None, batch_size: int = 128, shuffle: bool = True, augment=None,
              sampling: str = "permutation"):
        """One pass over the corpus in batches; returns the reference's `losses.avg` (each batch weighted by its padded size).
        augment: None, a callable `wav -> wav` run on the host per visited recording, or an `Augmenter`: one recipe is drawn per visited
        recording, with the recording's index as row_key (its noise differs from its neighbours' and, the seeds being drawn anew,
        between epochs), and applied on the device inside `step`, with the augmenter's bank of impulse responses when it draws
        "aliasing" or "room".
        audios may be a `TrainingSet` (labels omitted): every batch then goes through `step_resident`, the batches' losses x B T are
        summed on the device and ONE `.item()` at the end gives the average (augment: None or an `Augmenter`).
        sampling: "permutation" visits every recording once (shuffled or in order); "reference" draws len(corpus) indices WITH
        replacement from the trainer's CPU generator, what the reference's `SileroVadDataset.__getitem__` does in train mode, where the
        loader's index is ignored (tuning/utils.py:88, 109-110).  The visited indices stay in `last_order`."""
        from .augment import Augmenter
        on_device = isinstance(augment, Augmenter)
        # an augmenter that draws "aliasing" or "room" goes through the calls with a bank (its own, uploaded once; empty without "room")
        bank = None
        if on_device and augment.needs_bank:
            bank = augment.bank_on(self.device)
            if bank is None:
                bank = torch.zeros(0, dtype=torch.float32, device=self.device)
        resident = isinstance(audios, TrainingSet)
        if resident and (labels is not None or not (augment is None or on_device)):
            raise ValueError("a TrainingSet carries its labels, and takes no host augmentation: augment is None or an Augmenter")
        if not resident and labels is None:
            raise ValueError("labels: one sequence per recording")
        if sampling == "reference":
            order = torch.randint(0, len(audios), (len(audios),), generator=self._cpu_generator()).tolist()
        elif sampling == "permutation":
            order = torch.randperm(len(audios), generator=self._cpu_generator()).tolist() if shuffle else list(range(len(audios)))
        else:
            raise ValueError(f"sampling: 'permutation' or 'reference', got {sampling!r}")
        self.last_order = order
        if resident:
            total, count = torch.zeros((), dtype=torch.float64, device=self.device), 0
            for i in range(0, len(order), batch_size):
                idx = order[i:i + batch_size]
                loss = self.step_resident(audios, idx, recipes=augment.draw(len(idx), row_keys=idx) if on_device else None, bank=bank)
                total = total + loss * self.last_numel
                count += self.last_numel
            return float(total.item()) / max(count, 1)
        total, count = 0.0, 0
        for i in range(0, len(order), batch_size):
            idx = order[i:i + batch_size]
            if on_device:
                loss = self.step([audios[j] for j in idx], [labels[j] for j in idx], recipes=augment.draw(len(idx), row_keys=idx), bank=bank)
            else:
                wavs = [audios[j] if augment is None else augment(audios[j]) for j in idx]
                loss = self.step(wavs, [labels[j] for j in idx])
            total += loss * self.last_numel
            count += self.last_numel
        return total / max(count, 1)

    def _cpu_generator(self):
        if not hasattr(self, "_cpu_gen"):
            self._cpu_gen = torch.Generator()
            self._cpu_gen.manual_seed(self.generator.initial_seed())
        return self._cpu_gen

    def state_dict(self) -> dict:
        """The decoder under the reference's names (CPU tensors): `model._model.decoder.load_state_dict(...)` takes it at a user's site."""
        return {n: self.params[n].detach().cpu().clone() for n in DECODER_NAMES}

    def weights(self) -> bytes:
        return replace_decoder(self.base_weights, self.state_dict(), self.sampling_rate)

    def model(self):
        from .engine import load_silero_vad
        return load_silero_vad(device=self.device.index or 0, weights=self.weights())


def _model_weights(model) -> bytes:
    blob = getattr(getattr(model, "engine", None), "weights", None)
    return bytes(blob) if blob is not None else open(_lib.WEIGHTS_PATH, "rb").read()


def tune(train_audios, train_labels, val_audios, val_labels, model, num_epochs: int = 20, sampling_rate: int = 16000, batch_size: int = 128,
         noise_loss: float = 0.5, trainer: Optional[DecoderTrainer] = None, augment=None, sampling: str = "permutation", **trainer_kw):
    """tune.py's loop: every epoch one `DecoderTrainer.epoch`, then `validate` on the tuned model; the weights of the best rounded ROC-AUC
    are kept.  augment, sampling: as in `DecoderTrainer.epoch`.  train_audios may be a resident `TrainingSet` with train_labels None (a
    16 kHz set with sampling_rate=8000 is the reference's tune_8k flow; the validation recordings are then at 8 kHz).  Returns (container bytes of the best epoch or None if no epoch beat 0, [(train loss, val loss, val ROC-AUC), ...])."""
    from .streams import validate
    trainer = trainer or DecoderTrainer(model, sampling_rate=sampling_rate, noise_loss=noise_loss, **trainer_kw)
    best_auc, best, history = 0.0, None, []
    for _ in range(num_epochs):
        train_loss = trainer.epoch(train_audios, train_labels, batch_size=batch_size, augment=augment, sampling=sampling)
        tuned = trainer.model()
        val_loss, val_auc = validate(val_audios, val_labels, tuned, sampling_rate, noise_loss)
        history.append((train_loss, val_loss, val_auc))
        if val_auc > best_auc:                      # (tune.py: `if val_roc > best_val_roc`, from 0)
            best_auc, best = val_auc, trainer.weights()
    return best, history
