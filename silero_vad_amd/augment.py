"""Audio augmentations of decoder fine-tuning, on the device: the part of the reference's training recipe that runs every recording
through audiomentations (`SileroVadDataset.__getitem__` -> `build_audiomentations_augs(p)`: `SomeOf((1, 3))` of fifteen transforms,
tuning/utils.py:87-143).  Here the twelve transforms with arithmetic that can be stated are five op kinds of a per-row *recipe*
(csrc/augment.hpp is the rule): NOISE (counter-based Gaussian noise), BIQUADS (a cascade of up to eight second-order sections, the
recursion in double), CLIP (clipping at two quantiles of the row), FIR (convolution with a per-row impulse response out of a bank
of taps: room reverb, or audiomentations' ApplyImpulseResponse with measured responses) and ALIAS (audiomentations' Aliasing, two
np.interp calls).  `augment_device` applies recipes to a padded batch on the GPU (vad_augment_rows_device, or
vad_augment_rows_device_x when a bank is given), `augment_host` is its twin in double on the host, `Augmenter` draws recipes with
the reference's rule.  The default `Augmenter()` draws the ten transforms of TRANSFORMS; `transforms=ALL_TRANSFORMS` adds "aliasing"
and "room".

    aug = Augmenter(p=0.5, seed=0)
    trainer.epoch(audios, labels, augment=aug)          # recipes drawn per visited recording, applied between upload and encode

Left out, for want of arithmetic that can be stated and checked without the library:
    AirAbsorption, Mp3Compression, PitchShift -- no definable arithmetic here.
"room" is RoomSimulator in spirit, not in bits: the library takes its impulse response from pyroomacoustics; here it is the stated
image-source rule of `rir_shoebox` (Allen and Berkley, box room, the direct sound at tap 0 with gain 1 so that labels stay aligned).
The parameter ranges below are audiomentations' documented defaults AS REMEMBERED; nothing here verifies them against the library,
which is why each is a constructor argument.

One deliberate difference from the reference: it augments the whole recording and then cuts to `max_train_length_sec`; the trainer
cuts first and the augmentation sees the cut.  For causal filters and counter-based noise that is the same audio; for clipping the
quantiles are those of the cut.
"""
import ctypes
import math
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import lib

NOISE, BIQUADS, CLIP, FIR, ALIAS = 1, 2, 3, 4, 5
MAX_OPS, MAX_SECTIONS, MAX_TAPS = 3, 8, 8192
LOWPASS, HIGHPASS, BANDPASS, NOTCH, PEAKING, LOWSHELF, HIGHSHELF = range(7)
BIQUAD_KINDS = {"lowpass": LOWPASS, "highpass": HIGHPASS, "bandpass": BANDPASS, "notch": NOTCH, "peaking": PEAKING, "lowshelf": LOWSHELF,
                "highshelf": HIGHSHELF}
# vad_augment_op / vad_augment_recipe of include/silero_vad_hip.h
OP_DTYPE = np.dtype([("kind", "<i4"), ("n_sections", "<i4"), ("coef", "<f8", (MAX_SECTIONS, 5)), ("a", "<f8"), ("b", "<f8"), ("seed", "<u8")])
RECIPE_DTYPE = np.dtype([("n_ops", "<i4"), ("reserved", "<i4"), ("ops", OP_DTYPE, (MAX_OPS,)), ("row_key", "<u8")])
assert OP_DTYPE.itemsize == 352 and RECIPE_DTYPE.itemsize == 1072
# 24 dB/oct Butterworth as two sections: q = 1 / (2 cos(pi / 8)), 1 / (2 cos(3 pi / 8)) = 0.54119610, 1.30656296 (the eight digits
# alone leave the response 4e-9 away from scipy's butter(4))
BUTTER4_Q = (0.5 / math.cos(math.pi / 8.0), 0.5 / math.cos(3.0 * math.pi / 8.0))
# the reference's list, in its order (the order ops are applied in)
TRANSFORMS = ("noise", "band_pass", "band_stop", "clipping", "high_pass", "high_shelf", "low_pass", "low_shelf", "peaking", "seven_band_eq")
# the twelve: the reference's list order with Aliasing (its first entry) and RoomSimulator (between PeakingFilter and SevenBandParametricEQ)
ALL_TRANSFORMS = ("aliasing",) + TRANSFORMS[:9] + ("room",) + TRANSFORMS[9:]
DEFAULT_RANGES = dict(
    noise_amplitude=(0.001, 0.015),
    clipping_percentile=(0.0, 40.0),
    low_pass_cutoff=(150.0, 7500.0), high_pass_cutoff=(20.0, 2400.0), rolloffs=(12, 24),
    band_center=(200.0, 4000.0), band_fraction=(0.5, 1.99),
    low_shelf_center=(50.0, 4000.0), high_shelf_center=(300.0, 7500.0), shelf_gain_db=(-18.0, 18.0), shelf_q=(0.1, 0.999),
    peaking_center=(50.0, 7500.0), peaking_gain_db=(-24.0, 24.0), peaking_q=(0.5, 5.0),
    eq_centers=(100.0, 200.0, 400.0, 800.0, 1600.0, 3200.0, 6400.0), eq_gain_db=(-12.0, 12.0), eq_q=1.0, eq_shelf_q=0.7071067811865476,
    aliasing_rate=(8000, None),                                                      # None: the augmenter's sampling rate
    room_size_x=(3.6, 5.6), room_size_y=(3.6, 3.9), room_size_z=(2.4, 3.0), room_absorption=(0.075, 0.4), room_margin=0.3, room_max_order=12,
)


def block_size() -> int:
    """Samples of one block of the device's three-pass cascade (the shapes the GPU tests are built around)."""
    return int(lib().vad_augment_block())


def biquad_design(kind, sampling_rate: float, f0: float, q: float = 0.7071067811865476, gain_db: float = 0.0) -> np.ndarray:
    """vad_biquad_design: one Audio-EQ-cookbook section [b0, b1, b2, a1, a2] (a0 = 1) in double."""
    k = BIQUAD_KINDS[kind] if isinstance(kind, str) else int(kind)
    coef = np.zeros(5, dtype=np.float64)
    rc = lib().vad_biquad_design(k, float(sampling_rate), float(f0), float(q), float(gain_db), coef.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    if rc:
        raise _lib.VadError(rc, f"vad_biquad_design({kind!r}, sr={sampling_rate}, f0={f0}, q={q}, gain_db={gain_db})")
    return coef


def butterworth(kind, sampling_rate: float, f0: float, rolloff_db: int = 12) -> np.ndarray:
    """12 or 24 dB/oct Butterworth low- / high-pass as [1 or 2][5] sections."""
    if rolloff_db == 12:
        return biquad_design(kind, sampling_rate, f0)[None]
    if rolloff_db == 24:
        return np.stack([biquad_design(kind, sampling_rate, f0, q) for q in BUTTER4_Q])
    raise ValueError("rolloff_db must be 12 or 24")


def make_recipes(rows: Sequence, row_keys=None) -> np.ndarray:
    """Recipes from plain Python: one list of ops per row, an op being ("noise", amplitude, seed), ("biquads", sections [S][5] as
    b0 b1 b2 a1 a2 or [S][6] as scipy's sos with a0 = 1), ("clip", q_lo, q_hi), ("fir", first_tap, n_taps): the taps
    bank[first_tap : first_tap + n_taps] of the bank given to the call, or ("alias", new_rate, rate).  row_keys: default the row's
    index."""
    out = np.zeros(len(rows), dtype=RECIPE_DTYPE)
    out["row_key"] = np.arange(len(rows), dtype=np.uint64) if row_keys is None else np.asarray(row_keys, dtype=np.uint64)
    for r, ops in zip(out, rows):
        r["n_ops"] = len(ops)
        if len(ops) > MAX_OPS:
            raise ValueError(f"a recipe holds at most {MAX_OPS} ops")
        for o, op in zip(r["ops"], ops):
            if op[0] == "noise":
                o["kind"], o["a"], o["seed"] = NOISE, float(op[1]), int(op[2])
            elif op[0] == "biquads":
                sos = np.atleast_2d(np.asarray(op[1], dtype=np.float64))
                if sos.shape[1] == 6:
                    if not np.all(sos[:, 3] == 1.0):
                        raise ValueError("sos sections must have a0 = 1")
                    sos = sos[:, (0, 1, 2, 4, 5)]
                if sos.shape[1] != 5 or not 1 <= sos.shape[0] <= MAX_SECTIONS:
                    raise ValueError(f"biquads: [1 .. {MAX_SECTIONS}][5] sections, got {sos.shape}")
                o["kind"], o["n_sections"] = BIQUADS, sos.shape[0]
                o["coef"][:sos.shape[0]] = sos
            elif op[0] == "clip":
                o["kind"], o["a"], o["b"] = CLIP, float(op[1]), float(op[2])
            elif op[0] == "fir":
                if int(op[1]) < 0:
                    raise ValueError("fir: a negative first tap")
                o["kind"], o["seed"], o["n_sections"] = FIR, int(op[1]), int(op[2])
            elif op[0] == "alias":
                o["kind"], o["a"], o["b"] = ALIAS, float(op[1]), float(op[2])
            else:
                raise ValueError(f"unknown op {op[0]!r}")
    return out


def _recipes_array(recipes, n: int) -> np.ndarray:
    r = np.ascontiguousarray(recipes)
    if r.dtype != RECIPE_DTYPE or r.ndim != 1 or r.shape[0] != n:
        raise ValueError(f"recipes must be a 1-D array of RECIPE_DTYPE with one entry per row ({n})")
    return r


def check_recipes(recipes, bank_len: Optional[int] = None) -> None:
    """vad_augment_check_recipes: raises VadError with the library's sentence for the first bad recipe.  bank_len: the length of the
    bank of taps the recipes go with (vad_augment_check_recipes_bank); None: no bank, "fir" and "alias" are unknown kinds."""
    r = np.ascontiguousarray(recipes)
    if r.dtype != RECIPE_DTYPE or r.ndim != 1:
        raise ValueError("recipes must be a 1-D array of RECIPE_DTYPE")
    why = ctypes.c_char_p()
    if bank_len is None:
        rc = lib().vad_augment_check_recipes(r.ctypes.data, r.shape[0], ctypes.byref(why))
    else:
        rc = lib().vad_augment_check_recipes_bank(r.ctypes.data, r.shape[0], int(bank_len), ctypes.byref(why))
    if rc:
        raise _lib.VadError(rc, (why.value or b"").decode())


def augment_workspace_bytes(n_rows: int, width: int) -> int:
    return int(lib().vad_augment_workspace_bytes(int(n_rows), int(width)))


def augment_scratch_bytes(n_rows: int, width: int) -> int:
    """vad_augment_scratch_bytes: the second row buffer of a call with a bank ("fir" and "alias" cannot run in place)."""
    return int(lib().vad_augment_scratch_bytes(int(n_rows), int(width)))


def fir_bank(responses: Sequence):
    """Packs 1-D impulse responses into one float32 bank: (bank, offsets, lengths), response i at bank[offsets[i] : offsets[i] +
    lengths[i]] -- the ("fir", offsets[i], lengths[i]) of `make_recipes`.  Refuses an empty response, one longer than MAX_TAPS and a
    non-finite tap."""
    taps = [np.asarray(h, dtype=np.float32) for h in responses]
    for i, h in enumerate(taps):
        if h.ndim != 1 or not 1 <= h.size <= MAX_TAPS:
            raise ValueError(f"response {i}: a 1-D array of 1 .. {MAX_TAPS} taps, got shape {h.shape}")
        if not np.all(np.isfinite(h)):
            raise ValueError(f"response {i}: a non-finite tap")
    lengths = np.asarray([h.size for h in taps], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64) if taps else np.zeros(0, np.int64)
    bank = np.concatenate(taps) if taps else np.zeros(0, np.float32)
    return bank, offsets, lengths


def rir_shoebox(sampling_rate: float, room, source, microphone, absorption: float, max_order: int = 12, n_taps: int = MAX_TAPS) -> np.ndarray:
    """vad_rir_shoebox: the image-source impulse response (Allen and Berkley) of a box room of size `room` [3] in metres, float32
    [n_taps], the direct sound at tap 0 with gain 1.  A stated rule in the spirit of audiomentations' RoomSimulator; it does not
    reproduce pyroomacoustics' bits."""
    vec = [np.ascontiguousarray(v, dtype=np.float64) for v in (room, source, microphone)]
    if any(v.shape != (3,) for v in vec):
        raise ValueError("room, source and microphone are three coordinates each")
    n_taps = int(n_taps)
    h = np.zeros(max(n_taps, 1), dtype=np.float32)
    ptr = [v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for v in vec]
    rc = lib().vad_rir_shoebox(float(sampling_rate), ptr[0], ptr[1], ptr[2], float(absorption), int(max_order), h.ctypes.data, n_taps)
    if rc:
        raise _lib.VadError(rc, f"vad_rir_shoebox(sr={sampling_rate}, room={vec[0].tolist()}, source={vec[1].tolist()}, "
                                f"microphone={vec[2].tolist()}, absorption={absorption}, max_order={max_order}, n_taps={n_taps})")
    return h


def _bank_array(bank) -> np.ndarray:
    b = np.ascontiguousarray(bank, dtype=np.float32)
    if b.ndim != 1:
        raise ValueError("bank must be a 1-D float32 array of taps")
    return b


def augment_host(x, lens, recipes, threads: int = 0, bank=None) -> np.ndarray:
    """vad_augment_rows_host, the device call's twin, no GPU: x [n, W] int16 or float32 (anything else is taken as float32), lens [n],
    recipes [n] of RECIPE_DTYPE -> float32 [n, W], zero at and behind lens.  bank: the float32 taps that "fir" ops index
    (vad_augment_rows_host_x; also admits "alias"); None: the call without a bank, to which both are unknown kinds."""
    x = np.asarray(x)
    if x.dtype != np.int16:
        x = x.astype(np.float32, copy=False)
    if x.ndim != 2 or x.shape[0] == 0 or x.shape[1] == 0:
        raise ValueError("x must be [n, W]")
    if x.strides[1] != x.itemsize or x.strides[0] % x.itemsize or x.strides[0] < x.shape[1] * x.itemsize:
        x = np.ascontiguousarray(x)
    n, W = x.shape
    ln = np.ascontiguousarray(lens, dtype=np.int64)
    if ln.shape != (n,):
        raise ValueError("lens must hold one value per row")
    r = _recipes_array(recipes, n)
    b = None if bank is None else _bank_array(bank)
    check_recipes(r, None if b is None else b.size)
    out = np.empty((n, W), dtype=np.float32)
    ld = x.strides[0] // x.itemsize if n > 1 else W
    if b is None:
        rc = lib().vad_augment_rows_host(x.ctypes.data, x.itemsize, ld, ln.ctypes.data, n, r.ctypes.data, out.ctypes.data, W, int(threads))
    else:
        rc = lib().vad_augment_rows_host_x(x.ctypes.data, x.itemsize, ld, ln.ctypes.data, n, r.ctypes.data, out.ctypes.data, W,
                                           b.ctypes.data if b.size else None, b.size, int(threads))
    if rc:
        raise _lib.VadError(rc, "vad_augment_rows_host")
    return out


class _Extra(ctypes.Structure):
    """vad_augment_extra"""
    _fields_ = [("fir_bank", ctypes.c_void_p), ("fir_bank_len", ctypes.c_long), ("scratch", ctypes.c_void_p), ("scratch_bytes", ctypes.c_size_t)]


def augment_device(engine, x_dev, lens, recipes, out=None, workspace=None, bank=None, scratch=None):
    """vad_augment_rows_device on the current stream: x_dev [n, W] int16 or float32 cuda tensor (rows may be strided), lens [n] (any
    integer sequence or an int64 cuda tensor), recipes [n] of RECIPE_DTYPE (checked on the host, then uploaded) or a uint8 cuda tensor
    holding them already (not checked: the device returns a row with a bad recipe as its input).  Returns float32 [n, W], zero at and
    behind lens; the storage's rows are padded to a multiple of 4 samples, so the result is contiguous when W is one.
    out: a float32 cuda tensor [n, >= W] to write (row stride a multiple of 4, 16-byte aligned; written over its whole width);
    workspace: a uint8 cuda tensor of at least `augment_workspace_bytes(n, out width)` bytes to reuse.
    bank: the taps "fir" ops index, a 1-D float32 array (uploaded) or cuda tensor; with it the call is vad_augment_rows_device_x,
    which also admits "alias".  None: the call without a bank, to which both are unknown kinds.
    scratch: with a bank, a uint8 cuda tensor of at least `augment_scratch_bytes(n, out width)` bytes to reuse."""
    import torch
    if not (torch.is_tensor(x_dev) and x_dev.is_cuda and x_dev.dim() == 2 and x_dev.dtype in (torch.int16, torch.float32)):
        raise ValueError("x_dev must be an int16 or float32 cuda tensor [n, W]")
    n, W = int(x_dev.shape[0]), int(x_dev.shape[1])
    if n == 0 or W == 0:
        raise ValueError("x_dev must be [n, W] with n, W > 0")
    if x_dev.stride(1) != 1 or (n > 1 and x_dev.stride(0) < W):
        x_dev = x_dev.contiguous()
    dev = x_dev.device
    ln = lens if torch.is_tensor(lens) else torch.as_tensor(np.asarray(lens, dtype=np.int64))
    ln = ln.to(device=dev, dtype=torch.int64).contiguous()
    if ln.numel() != n:
        raise ValueError("lens must hold one value per row")
    if bank is not None:
        if torch.is_tensor(bank):
            if not (bank.is_cuda and bank.dtype == torch.float32 and bank.dim() == 1 and bank.is_contiguous()):
                raise ValueError("bank on the device must be a contiguous 1-D float32 cuda tensor")
        else:
            bank = torch.from_numpy(_bank_array(bank).copy()).to(dev)
    if torch.is_tensor(recipes):
        rec = recipes
        if not (rec.is_cuda and rec.dtype == torch.uint8 and rec.is_contiguous() and rec.numel() == n * RECIPE_DTYPE.itemsize):
            raise ValueError("recipes on the device must be a contiguous uint8 cuda tensor of n * 1072 bytes")
    else:
        r = _recipes_array(recipes, n)
        check_recipes(r, None if bank is None else int(bank.numel()))
        rec = torch.from_numpy(r.view(np.uint8).copy()).to(dev)
    if out is None:
        out = torch.empty((n, (W + 3) // 4 * 4), dtype=torch.float32, device=dev)
    if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == n and out.shape[1] >= W
            and out.stride(1) == 1 and out.shape[1] % 4 == 0 and (n == 1 or out.stride(0) == out.shape[1])):
        raise ValueError("out must be a contiguous float32 cuda tensor [n, W rounded up to a multiple of 4 or more]")
    Wo = int(out.shape[1])
    need = augment_workspace_bytes(n, Wo)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    args = (engine._h, x_dev.data_ptr(), x_dev.element_size(), x_dev.stride(0) if n > 1 else W, ln.data_ptr(), n, rec.data_ptr(), out.data_ptr(),
            Wo, workspace.data_ptr(), workspace.numel())
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if bank is None:
            engine._check(lib().vad_augment_rows_device(*args, stream))
        else:
            if scratch is None:
                scratch = torch.empty(max(augment_scratch_bytes(n, Wo), 1), dtype=torch.uint8, device=dev)
            if not (torch.is_tensor(scratch) and scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous()):
                raise ValueError("scratch must be a contiguous uint8 cuda tensor")
            extra = _Extra(bank.data_ptr() if bank.numel() else None, int(bank.numel()), scratch.data_ptr(), int(scratch.numel()))
            engine._check(lib().vad_augment_rows_device_x(*args, ctypes.byref(extra), stream))
    return out[:, :W]


class Augmenter:
    """Draws recipes with the reference's rule: per row, with probability `p`, 1 to 3 distinct transforms of `transforms` (default
    all ten of TRANSFORMS; names out of the twelve of ALL_TRANSFORMS), applied in the order of the reference's list; otherwise an
    empty recipe.
    With "room" the augmenter carries a bank of impulse responses, `bank` (numpy float32; `offsets`, `lengths` per response), that
    the calls applying its recipes must be given: `rirs`, the caller's measured responses (1-D arrays, cut to 8192 taps), or, when
    `rirs` is None, `rooms` shoebox responses (`rir_shoebox`) drawn once at construction from their own generator (seeded with
    `seed`): room size, absorption, source and microphone uniform inside with a margin -- the room_* keys of DEFAULT_RANGES.  A
    "room" draw picks a response uniformly; an "aliasing" draw picks an integer rate in `aliasing_rate` (None: the sampling rate).
    `bank_on(device)` is the device copy, cached per device.  `ranges`: any key of
    DEFAULT_RANGES -- audiomentations' documented defaults as remembered, UNVERIFIED against the library.  Frequencies are drawn
    log-uniformly and kept below 0.45 * sampling_rate, so the 8 kHz net's trainer can use the same object.  The draws come from one
    numpy Generator seeded with `seed` and continue from call to call; `last_params` holds what the last `draw` drew, per row a list
    of (transform, parameters)."""

    def __init__(self, p: float = 0.5, sampling_rate: int = 16000, seed: int = 0, transforms: Optional[Sequence[str]] = None,
                 rirs: Optional[Sequence] = None, rooms: int = 64, **ranges):
        if not 0.0 <= p <= 1.0:
            raise ValueError("p must be in [0, 1]")
        unknown = set(ranges) - set(DEFAULT_RANGES)
        if unknown:
            raise TypeError(f"unknown ranges: {sorted(unknown)}")
        names = TRANSFORMS if transforms is None else tuple(transforms)
        bad = [t for t in names if t not in ALL_TRANSFORMS]
        if bad or not names or len(set(names)) != len(names):
            raise ValueError(f"transforms must be distinct names out of {ALL_TRANSFORMS}")
        self.p, self.sampling_rate, self.seed = float(p), int(sampling_rate), int(seed)
        self.transforms = tuple(t for t in ALL_TRANSFORMS if t in names)             # the list's order
        self.ranges = dict(DEFAULT_RANGES, **ranges)
        self.rng = np.random.default_rng(self.seed)
        self.last_params = []
        self.bank, self.offsets, self.lengths, self.rooms = None, None, None, []
        self._bank_dev = {}
        if "room" in self.transforms:
            if rirs is not None:
                responses = [np.asarray(h, dtype=np.float32)[:MAX_TAPS] for h in rirs]
                if not responses:
                    raise ValueError("rirs: at least one impulse response")
            else:
                if int(rooms) < 1:
                    raise ValueError("rooms: at least one room")
                responses = self._draw_rooms(int(rooms))
            self.bank, self.offsets, self.lengths = fir_bank(responses)

    def _draw_rooms(self, count):
        """`count` shoebox responses from a generator of their own, so that the recipe draws do not depend on the number of rooms;
        a response is cut behind its last non-zero tap"""
        g, rng = self.ranges, np.random.default_rng([self.seed, 0x726F6F6D])
        out, margin = [], float(g["room_margin"])
        for _ in range(count):
            size = np.array([rng.uniform(*g["room_size_" + a]) for a in "xyz"])
            absorption = float(rng.uniform(*g["room_absorption"]))
            src = rng.uniform(margin, size - margin)
            mic = rng.uniform(margin, size - margin)
            h = rir_shoebox(self.sampling_rate, size, src, mic, absorption, int(g["room_max_order"]), MAX_TAPS)
            self.rooms.append(dict(size=size.tolist(), absorption=absorption, source=src.tolist(), microphone=mic.tolist()))
            out.append(h[:max(int(np.flatnonzero(h)[-1]) + 1, 1)])
        return out

    def bank_on(self, device):
        """The bank as a float32 tensor on `device` (uploaded once per device), or None without "room"."""
        import torch
        if self.bank is None:
            return None
        key = str(torch.device(device))
        if key not in self._bank_dev:
            self._bank_dev[key] = torch.from_numpy(self.bank).to(device)
        return self._bank_dev[key]

    @property
    def needs_bank(self) -> bool:
        """True when the recipes hold ops that only the calls with a bank know ("aliasing", "room")."""
        return "room" in self.transforms or "aliasing" in self.transforms

    # -- draws
    def _uniform(self, key):
        lo, hi = self.ranges[key]
        return float(self.rng.uniform(lo, hi))

    def _clamp(self, f):
        return min(float(f), 0.45 * self.sampling_rate * (1.0 - 1e-6))

    def _freq(self, key):
        lo, hi = self.ranges[key]
        return self._clamp(math.exp(self.rng.uniform(math.log(lo), math.log(hi))))

    def _draw_op(self, name):
        sr, g = self.sampling_rate, self.ranges
        if name == "aliasing":
            lo, hi = g["aliasing_rate"]
            hi = sr if hi is None else int(hi)
            prm = dict(rate=int(self.rng.integers(min(int(lo), hi), hi + 1)))
            return ("alias", prm["rate"], sr), prm
        if name == "room":
            i = int(self.rng.integers(0, len(self.offsets)))
            prm = dict(response=i, first_tap=int(self.offsets[i]), n_taps=int(self.lengths[i]))
            return ("fir", prm["first_tap"], prm["n_taps"]), prm
        if name == "noise":
            prm = dict(amplitude=self._uniform("noise_amplitude"), seed=int(self.rng.integers(0, 2 ** 63)))
            return ("noise", prm["amplitude"], prm["seed"]), prm
        if name == "clipping":
            t = self._uniform("clipping_percentile")
            prm = dict(percentile=t, q_lo=t / 200.0, q_hi=1.0 - t / 200.0)
            return ("clip", prm["q_lo"], prm["q_hi"]), prm
        if name in ("low_pass", "high_pass"):
            prm = dict(f0=self._freq(name + "_cutoff"), rolloff_db=int(self.rng.choice(g["rolloffs"])))
            sos = butterworth("lowpass" if name == "low_pass" else "highpass", sr, prm["f0"], prm["rolloff_db"])
        elif name in ("band_pass", "band_stop"):
            prm = dict(f0=self._freq("band_center"), fraction=self._uniform("band_fraction"))
            prm["q"] = 1.0 / prm["fraction"]                                         # bandwidth = fraction * centre
            sos = biquad_design("bandpass" if name == "band_pass" else "notch", sr, prm["f0"], prm["q"])[None]
        elif name in ("low_shelf", "high_shelf"):
            prm = dict(f0=self._freq(name + "_center"), gain_db=self._uniform("shelf_gain_db"), q=self._uniform("shelf_q"))
            sos = biquad_design("lowshelf" if name == "low_shelf" else "highshelf", sr, prm["f0"], prm["q"], prm["gain_db"])[None]
        elif name == "peaking":
            prm = dict(f0=self._freq("peaking_center"), gain_db=self._uniform("peaking_gain_db"), q=self._uniform("peaking_q"))
            sos = biquad_design("peaking", sr, prm["f0"], prm["q"], prm["gain_db"])[None]
        else:                                                                        # seven_band_eq
            centers = [self._clamp(f) for f in g["eq_centers"]]
            gains = [self._uniform("eq_gain_db") for _ in centers]
            kinds = ["lowshelf"] + ["peaking"] * (len(centers) - 2) + ["highshelf"]
            qs = [g["eq_shelf_q"]] + [g["eq_q"]] * (len(centers) - 2) + [g["eq_shelf_q"]]
            prm = dict(f0=centers, gain_db=gains, q=qs)
            sos = np.stack([biquad_design(k, sr, f, q, db) for k, f, q, db in zip(kinds, centers, qs, gains)])
        return ("biquads", sos), prm

    def draw(self, n_rows: int, row_keys=None) -> np.ndarray:
        """Recipes [n_rows] of RECIPE_DTYPE; row_keys: default 0 .. n_rows - 1."""
        rows, self.last_params = [], []
        for _ in range(int(n_rows)):
            ops, prms = [], []
            if self.rng.random() < self.p:
                k = min(int(self.rng.integers(1, MAX_OPS + 1)), len(self.transforms))
                for i in sorted(self.rng.choice(len(self.transforms), size=k, replace=False).tolist()):
                    op, prm = self._draw_op(self.transforms[i])
                    ops.append(op)
                    prms.append((self.transforms[i], prm))
            rows.append(ops)
            self.last_params.append(prms)
        return make_recipes(rows, row_keys)
