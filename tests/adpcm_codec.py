"""DVI4 (RFC 3551 section 4.5.1, 4-bit IMA ADPCM) for the tests, in plain Python and independent of the library: the decoder the host
twin and the device are compared with, and the encoder that turns the golden audio into payloads (the package has none).  A payload is
{predict: int16 big-endian, index: uint8, reserved, then 4-bit codes, two a byte, the first sample in the high nibble}."""
import numpy as np

STEP = (7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157,
        173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707,
        1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635,
        13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767)
IDX = (-1, -1, -1, -1, 2, 4, 6, 8)
assert len(STEP) == 89


def step_once(d, pred, idx):
    """One code d with the decoder's state (pred, idx) -> the new state; the sample is the new pred."""
    step = STEP[idx]
    v = (step >> 3) + (step if d & 4 else 0) + (step >> 1 if d & 2 else 0) + (step >> 2 if d & 1 else 0)
    pred = max(-32768, min(32767, pred - v if d & 8 else pred + v))
    return pred, max(0, min(88, idx + IDX[d & 7]))


def header(predict, index, reserved=0):
    return np.array([(predict >> 8) & 0xFF, predict & 0xFF, index, reserved], np.uint8)


def payload(predict, index, codes, reserved=0):
    """The payload of an even number of 4-bit codes behind the header (predict, index, reserved)."""
    c = np.asarray(codes, np.uint8)
    assert c.ndim == 1 and len(c) % 2 == 0 and (c < 16).all()
    return np.concatenate([header(predict, index, reserved), (c[0::2] << 4 | c[1::2]).astype(np.uint8)])


def decode(p):
    """A payload -> its int16 samples, one code at a time."""
    p = np.asarray(p, np.uint8)
    pred = int(np.array([p[0], p[1]], np.uint8).view(">i2")[0])
    idx = min(int(p[2]), 88)
    out = np.empty(2 * (len(p) - 4), np.int16)
    for j in range(len(out)):
        b = int(p[4 + j // 2])
        pred, idx = step_once(b & 15 if j & 1 else b >> 4, pred, idx)
        out[j] = pred
    return out


def special_payloads(n_codes):
    """name -> payload: the predictor saturating at both ends from index 88, the index floor, header indices 89 and 255 (used as 88)
    beside 88 itself, and a nonzero reserved byte."""
    rng = np.random.default_rng(88)
    codes = rng.integers(0, 16, n_codes).astype(np.uint8)
    return {"saturate_up": payload(32767, 88, np.full(n_codes, 0x7, np.uint8)),
            "saturate_down": payload(-32767, 88, np.full(n_codes, 0xF, np.uint8)),
            "cross_up": payload(-32768, 88, np.full(n_codes, 0x7, np.uint8)),
            "cross_down": payload(32767, 88, np.full(n_codes, 0xF, np.uint8)),
            "floor_up": payload(1000, 5, np.full(n_codes, 0x0, np.uint8)),
            "floor_down": payload(-1000, 5, np.full(n_codes, 0x8, np.uint8)),
            "index_88": payload(-77, 88, codes), "index_89": payload(-77, 89, codes), "index_255": payload(-77, 255, codes),
            "index_0": payload(123, 0, codes), "reserved": payload(123, 0, codes, reserved=0xC3)}


class Encoded:
    """A stretch of int16 audio through a plain IMA encoder, once: codes[j] and the encoder's state (pred[j], idx[j]) in FRONT of sample
    j.  packet(a, n) is the DVI4 payload of samples [a, a + n): the state before its first sample is its header, whatever was sent
    before it, so streams may start anywhere in the stretch."""

    def __init__(self, pcm):
        x = np.asarray(pcm, np.int16).astype(np.int64).tolist()
        n = len(x)
        self.codes, self.pred, self.idx = np.empty(n, np.uint8), np.empty(n + 1, np.int32), np.empty(n + 1, np.uint8)
        pred, idx = 0, 0
        for j, s in enumerate(x):
            self.pred[j], self.idx[j] = pred, idx
            step, diff = STEP[idx], s - pred
            d = 8 if diff < 0 else 0
            diff = abs(diff)
            if diff >= step:
                d |= 4
                diff -= step
            if diff >= step >> 1:
                d |= 2
                diff -= step >> 1
            if diff >= step >> 2:
                d |= 1
            self.codes[j] = d
            pred, idx = step_once(d, pred, idx)
        self.pred[n], self.idx[n] = pred, idx

    def packet(self, a, n):
        return payload(int(self.pred[a]), int(self.idx[a]), self.codes[a:a + n])
