"""Weight containers with a decoder other than the published one (TEST infrastructure; tests/test_decoder_containers.py and
tests/test_decoder_containers_gpu.py): built from the published container with `replace_decoder`, seeded, GPU-free, no fixture files.

    swapped    each rate carries the other rate's published decoder (the six tensors have the same shapes at both rates)
    jitter25   every value x (1 + 0.25 N(0, 1)), the two rates on their own draws
    random     every tensor redrawn N(0, sigma), sigma the published tensor's standard deviation -- rnn.weight_hh at 0.5 sigma (at the
               full sigma the recurrence is no longer contracting: a 1e-6 change of the state grows 263-fold in 32 steps, and two
               correct fp32 evaluations drift apart), decoder.2.bias (one value) drawn at its published magnitude
    only16k    `random`'s decoder at 16 kHz, the published one at 8 kHz
    only8k     the published decoder at 16 kHz, `random`'s at 8 kHz

What makes a variant usable at the suite's bounds is checked by tests/test_decoder_containers.py (the two conditioning tests)."""
import ctypes
import functools

import numpy as np

RATES = (16000, 8000)
VARIANTS = ("swapped", "jitter25", "random", "only16k", "only8k")
BOTH_RATES = ("swapped", "jitter25", "random")           # the variants whose two decoders are both new
WHICH = (0, 1, 2, 5, 6, 7, 8)                            # the images vad_debug_packed_copy hands out
# the longest run of chunks tests/test_decoder_containers_gpu.py carries a state over; the conditioning tests cover it
GPU_MAX_T = 8
_SEED = {"jitter25": 2501, "random": 7703}


def published_blob() -> bytes:
    from silero_vad_amd import _lib
    return _lib.WEIGHTS_PATH.read_bytes()


def _jitter(sd, rng):
    return {k: (v.astype(np.float64) * (1.0 + 0.25 * rng.standard_normal(v.shape))).astype(np.float32) for k, v in sd.items()}


def _random(sd, rng):
    out = {}
    for k, v in sd.items():
        if k == "decoder.2.bias":
            sigma = float(np.abs(v).max())
        else:
            sigma = float(v.astype(np.float64).std()) * (0.5 if k == "rnn.weight_hh" else 1.0)
        out[k] = (sigma * rng.standard_normal(v.shape)).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def variant_tensors(name: str, sr: int):
    """The decoder `name` puts at rate `sr` (float32 arrays under the reference's names), or None where it keeps the published one."""
    from silero_vad_amd.tuning import decoder_state_dict
    pub = published_blob()
    if name == "published":
        return None
    if name == "swapped":
        return decoder_state_dict(pub, 8000 if sr == 16000 else 16000)
    if name in ("only16k", "only8k"):
        return variant_tensors("random", sr) if sr == (16000 if name == "only16k" else 8000) else None
    if name not in _SEED:
        raise KeyError(name)
    rng = np.random.default_rng([_SEED[name], sr])
    return (_jitter if name == "jitter25" else _random)(decoder_state_dict(pub, sr), rng)


def build_variant(name: str) -> bytes:
    """The container of one variant (a fresh build on every call: the tests compare two builds)."""
    from silero_vad_amd.tuning import replace_decoder
    blob = published_blob()
    for sr in RATES:
        sd = variant_tensors(name, sr)
        if sd is not None:
            blob = replace_decoder(blob, sd, sr)
    return blob


@functools.lru_cache(maxsize=None)
def variant_blob(name: str) -> bytes:
    return published_blob() if name == "published" else build_variant(name)


def decoder_of(name: str, sr: int):
    """The six tensors the container `name` holds at `sr`, read back out of its bytes"""
    from silero_vad_amd.tuning import decoder_state_dict
    return decoder_state_dict(variant_blob(name), sr)


@functools.lru_cache(maxsize=None)
def packed_images(name: str):
    """{(sr, which): float32 words} of every image the C++ packer makes of the container, through a host-only engine"""
    from silero_vad_amd import _lib
    L = _lib.lib()
    blob = variant_blob(name)
    h = ctypes.c_void_p()
    assert L.vad_create_host_only(blob, len(blob), ctypes.byref(h)) == 0
    out = {}
    try:
        for sr in RATES:
            for which in WHICH:
                n = L.vad_debug_packed_floats(h, sr, which)
                assert n > 0, (sr, which)
                a = np.empty(n, np.float32)
                assert L.vad_debug_packed_copy(h, sr, which, a.ctypes.data_as(_lib.f32p), n) == 0
                out[sr, which] = a
    finally:
        L.vad_destroy(h)
    return out


def write_variant(name: str, directory):
    """The container as a file (what `Oracle(weights_path=...)` reads)"""
    path = directory / f"decoder_{name}.weights"
    if not path.exists():
        path.write_bytes(variant_blob(name))
    return path


# ---- the decoder in float64 (plain numpy) -------------------------------------------------------------------------------------------------
def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-x))


class Decoder64:
    """LSTMCell(128, 128) -> ReLU -> Conv1d(128, 1, 1) -> Sigmoid in float64 on one decoder's six tensors"""

    def __init__(self, sd):
        f = lambda k: np.asarray(sd[k], np.float64)
        self.w_ih, self.w_hh = f("rnn.weight_ih"), f("rnn.weight_hh")
        self.b = f("rnn.bias_ih") + f("rnn.bias_hh")
        self.w_out, self.b_out = f("decoder.2.weight").reshape(128), float(f("decoder.2.bias").reshape(()))

    def gates(self, feat):
        """feat [B, 128] -> W_ih feat + b_ih + b_hh [B, 512]"""
        return np.asarray(feat, np.float64) @ self.w_ih.T + self.b

    def cell(self, gx, h, c):
        """gate pre-activations [B, 512] without the recurrent term, (h, c) [B, 128] -> (prob [B], h', c')"""
        g = gx + h @ self.w_hh.T
        i, f, gg, o = sigmoid64(g[:, :128]), sigmoid64(g[:, 128:256]), np.tanh(g[:, 256:384]), sigmoid64(g[:, 384:])
        c = f * c + i * gg
        h = o * np.tanh(c)
        return sigmoid64(np.maximum(h, 0.0) @ self.w_out + self.b_out), h, c


def chunk_of(sr):
    return 512 if sr == 16000 else 256


def rolled_rows(wav, B, L, stride=7919):
    return np.stack([np.roll(wav, -b * stride)[:L] for b in range(B)])


def carried(B, T, n):
    """The random carried state and context of test_batch_shapes_vs_oracle"""
    rng = np.random.default_rng(B * 100 + T)
    st0 = (rng.standard_normal((2, B, 128)) * 0.3).astype(np.float32)
    cx0 = (rng.standard_normal((B, n // 8)) * 0.05).astype(np.float32)
    return st0, cx0
