"""Decoder fine-tuning on the device: the reference's `tuning/` training loop (`train()`, tuning/utils.py:206-249, driven by tune.py).

The reference trains one module, `VADDecoderRNNJIT` -- LSTMCell(128, 128), Dropout(0.1), ReLU, Conv1d(128, 1, 1), Sigmoid -- on the
output of the frozen STFT and encoder.  Here the frozen part is the engine's frontend (`HipSileroVAD.encode`, vad_encode_audio), the
loss and the six gradients come from HIP kernels (`decoder_grad`, vad_decoder_grad_device; csrc/trainer.hpp is the rule), and torch is
plumbing: device tensors, the optimizer, the dropout mask's generator.

    trainer = DecoderTrainer(model)                      # Adam(5e-4), dropout 0.1, noise loss 0.5, 8 s cuts: tuning/config.yml
    trainer.epoch(audios, labels)                        # labels: `chunk_labels` per recording
    trainer.epoch(audios, labels, augment=Augmenter())   # the reference's augmentations, on the device (augment.py)
    tuned = trainer.model()                              # a HipSileroVAD on trainer.weights()
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


class DecoderTrainer:
    """The reference's `train()` over one rate's decoder, on the device.  The six parameters are float32 cuda tensors started from the
    model's container; `optimizer`: a callable `params -> torch optimizer` or None for torch.optim.Adam(lr=learning_rate)."""

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
        self.optimizer = torch.optim.Adam(plist, lr=learning_rate) if optimizer is None else optimizer(plist)
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(int(seed))
        self._workspace = None
        self._aug_workspace = None
        self.last_grads = None
        self.last_augmented = None

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

    def step(self, audios: Sequence, labels: Sequence, recipes=None):
        """One optimizer step on one batch; returns the batch's loss (a float: one host synchronisation).  recipes: one augmentation
        recipe per recording (augment.RECIPE_DTYPE, e.g. `Augmenter.draw`): the uploaded padded batch goes through `augment_device`
        on the current stream before `encode` -- the recordings are cut to `max_train_length_sec` first, so the augmentation sees the
        cut -- and the augmented batch stays in `last_augmented`.  None: no augmentation."""
        pcm, nck, lab, T = self._batch(audios, labels)
        B = len(nck)
        with torch.cuda.device(self.device):
            x = torch.from_numpy(pcm).to(self.device)
            if recipes is not None:
                from .augment import augment_device, augment_workspace_bytes
                lens = [min(len(a), self.max_samples) for a in audios]
                need = augment_workspace_bytes(B, x.shape[1])
                if self._aug_workspace is None or self._aug_workspace.numel() < need:
                    self._aug_workspace = None
                    self._aug_workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
                x = augment_device(self.base_model.engine, x, lens, recipes, workspace=self._aug_workspace)
                self.last_augmented = x
            feat = self.base_model.encode(x, self.sampling_rate)
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
            return float(loss.item())

    def epoch(self, audios: Sequence, labels: Sequence, batch_size: int = 128, shuffle: bool = True, augment=None):
        """One pass over the corpus in batches; returns the reference's `losses.avg` (each batch weighted by its padded size).
        augment: None, a callable `wav -> wav` run on the host per visited recording, or an `Augmenter`: one recipe is drawn per visited
        recording, with the recording's index as row_key (its noise differs from its neighbours' and, the seeds being drawn anew,
        between epochs), and applied on the device inside `step`."""
        from .augment import Augmenter
        on_device = isinstance(augment, Augmenter)
        order = torch.randperm(len(audios), generator=self._cpu_generator()).tolist() if shuffle else list(range(len(audios)))
        total, count = 0.0, 0
        for i in range(0, len(order), batch_size):
            idx = order[i:i + batch_size]
            if on_device:
                loss = self.step([audios[j] for j in idx], [labels[j] for j in idx], recipes=augment.draw(len(idx), row_keys=idx))
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
         noise_loss: float = 0.5, trainer: Optional[DecoderTrainer] = None, augment=None, **trainer_kw):
    """tune.py's loop: every epoch one `DecoderTrainer.epoch`, then `validate` on the tuned model; the weights of the best rounded ROC-AUC
    are kept.  augment: as in `DecoderTrainer.epoch` (a callable or an `Augmenter`).  Returns (container bytes of the best epoch or None if no epoch beat 0, [(train loss, val loss, val ROC-AUC), ...])."""
    from .streams import validate
    trainer = trainer or DecoderTrainer(model, sampling_rate=sampling_rate, noise_loss=noise_loss, **trainer_kw)
    best_auc, best, history = 0.0, None, []
    for _ in range(num_epochs):
        train_loss = trainer.epoch(train_audios, train_labels, batch_size=batch_size, augment=augment)
        tuned = trainer.model()
        val_loss, val_auc = validate(val_audios, val_labels, tuned, sampling_rate, noise_loss)
        history.append((train_loss, val_loss, val_auc))
        if val_auc > best_auc:                      # (tune.py: `if val_roc > best_val_roc`, from 0)
            best_auc, best = val_auc, trainer.weights()
    return best, history
