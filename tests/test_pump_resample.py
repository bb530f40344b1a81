"""The streaming form of the resampler (vad_resample_stream_ready / _history / _host; `resample_stream_ready`, `resample_stream_history`,
`resample_stream`), without a GPU: the rule the pump's resampled rows follow (include/silero_vad_hip.h "THE STREAMING FORM").

Output m = q N + j reads the K inputs from p0 = q O + first[j] - W on; a stream that has received g inputs has emitted exactly the outputs
with p0 + K <= g.  The expected figures are computed HERE from `resample_table` -- the end p0 + K of every output of enough periods, and
for g near 2^40 from the same ends shifted by whole periods -- and the expected samples are `resample` of the whole signal: the streaming
twin must give those bits for every cut of the signal into pieces."""
import numpy as np
import pytest

from test_resample_gpu import GPU_PAIRS

PAIRS = GPU_PAIRS + [(8000, 16000), (16000, 8000)]
# the latency in input samples, max_j (first[j] - floor(j O / N)) - W + K: the figures of the header
ERR_ARG, ERR_SAMPLE_RATE = 1, 2            # include/silero_vad_hip.h vad_status
LATENCY = {(44100, 16000): 19, (24000, 16000): 11, (22050, 16000): 10, (48000, 16000): 19, (44100, 8000): 35}


def rule(pair):
    from silero_vad_amd import resample_geometry, resample_table
    O, N, W, K = resample_geometry(*pair)
    first = resample_table(*pair)[1].astype(np.int64)
    return O, N, W, K, first


def ends(pair, periods):
    """p0 + K of the outputs 0 ... periods * N - 1"""
    O, N, W, K, first = rule(pair)
    m = np.arange(periods * N, dtype=np.int64)
    return (m // N) * O + first[m % N] - W + K


@pytest.mark.parametrize("pair", PAIRS)
def test_ready_is_the_count_of_outputs_whose_inputs_have_arrived(built, pair):
    from silero_vad_amd import resample_stream_ready
    O, N, W, K, first = rule(pair)
    top = 3 * O + 2 * K
    e = ends(pair, top // O + 2 * K + 4)                           # (every output that can be ready at g <= top, and many more)
    assert (np.diff(e) >= 0).all(), "p0 + K falls from one output to the next: ready(g) would not be a count"
    assert e[-1] > top
    got = [resample_stream_ready(*pair, g) for g in range(top + 1)]
    want = [int((e <= g).sum()) for g in range(top + 1)]
    assert got == want
    assert all(a <= b for a, b in zip(got, got[1:])) and all(m <= -(-N * g // O) for g, m in enumerate(got))
    # far out: 2^40 = t O + r.  Output m + t N ends t O later than output m, and every output of the first t periods -- less the few of
    # the last ones, which the shifted table counts -- has ended
    big = 2 ** 40
    t = big // O - (2 * K + 4)
    assert t > 0
    far = [resample_stream_ready(*pair, big + d) for d in range(top + 1)]
    e_far = ends(pair, (big + top - t * O) // O + 2 * K + 8)
    assert e_far[-1] > big + top - t * O
    assert far == [t * N + int((e_far <= big + d - t * O).sum()) for d in range(top + 1)]
    assert all(m <= -(-N * (big + d) // O) for d, m in enumerate(far))


@pytest.mark.parametrize("pair", sorted(LATENCY))
def test_latency_figures(built, pair):
    O, N, W, K, first = rule(pair)
    j = np.arange(N)
    assert int((first - j * O // N).max()) - W + K == LATENCY[pair]


def pieces(x, pair, lengths, keep=None):
    """x cut into rows of the given lengths (the last one repeated to the end) through resample_stream, from zero history; keep: the
    history samples carried from one row to the next (None: all H), the older ones read as zero"""
    from silero_vad_amd import resample_stream, resample_stream_history
    H = resample_stream_history(*pair)
    hist, g, out, i = np.zeros(H, np.int16), 0, [], 0
    while g < len(x):
        n = min(lengths[min(i, len(lengths) - 1)], len(x) - g)
        y, hist = resample_stream(x[g:g + n], *pair, g, hist)
        if keep is not None:
            hist[:H - keep] = 0
        out.append(y)
        g, i = g + n, i + 1
    return np.concatenate(out)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("pair", PAIRS)
def test_every_cut_gives_the_whole_signal_bit_for_bit(built, pair):
    from silero_vad_amd import resample, resample_stream_history, resample_stream_ready, resample_table
    O, N, W, K, first = rule(pair)
    H = resample_stream_history(*pair)
    assert H == K - 1
    rng = np.random.default_rng(5)
    x = rng.integers(-30000, 30000, size=3 * O + 2 * K + 37).astype(np.int16)
    want = resample(x, *pair)[:resample_stream_ready(*pair, len(x))]
    cuts = {"1": [1], "H - 1": [H - 1], "H": [H], "H + 1": [H + 1], "whole": [len(x)],
            "random": [int(v) for v in rng.integers(1, 2 * H + 9, size=4 * len(x) // H + 8)],
            "mixed": [1, H + 1, 1, 1, H - 1, 3 * H, 1, H, 2]}
    for name, lengths in cuts.items():
        assert same_bits(pieces(x, pair, lengths), want), name
    # with one history sample fewer the rows of length 1 -- every output is then made with its oldest input the oldest history sample --
    # do NOT give the signal: H is what the rule needs, not a comfortable bound
    short = pieces(x, pair, [1], keep=H - 1)
    assert short.shape == want.shape and not same_bits(short, want)
    # ... and exactly: a single impulse at the oldest input of an output with a full run of K taps gives that output as tap 0 times the
    # impulse with H samples of history and as zero with H - 1
    taps = resample_table(*pair)[0]
    j = int(np.flatnonzero(taps[:, K - 1] != 0)[0])
    m = (W // O + 2) * N + j
    p0 = (m // N) * O + int(first[j]) - W
    assert p0 >= 0
    imp = np.zeros(p0 + K, np.int16)
    imp[p0] = 16384
    assert pieces(imp, pair, [1])[m] == np.float32(taps[j, 0]) * np.float32(0.5) != 0 and pieces(imp, pair, [1], keep=H - 1)[m] == 0


def test_unserved_pairs_and_bad_arguments_are_refused(built):
    from silero_vad_amd import _lib, resample_stream, resample_stream_history, resample_stream_ready
    L = _lib.lib()
    for pair in ((16000, 16000), (44100, 22050), (12345, 16000), (0, 16000), (-1, 8000)):
        assert L.vad_resample_stream_ready(*pair, 10) == -ERR_SAMPLE_RATE
        assert L.vad_resample_stream_history(*pair) == -ERR_SAMPLE_RATE
        assert L.vad_resample_stream_host(*pair, 0, None, None, 0, None, None) == -ERR_SAMPLE_RATE
        for call in (lambda: resample_stream_ready(*pair, 10), lambda: resample_stream_history(*pair),
                     lambda: resample_stream(np.zeros(4, np.int16), *pair, 0, np.zeros(33, np.int16))):
            with pytest.raises(ValueError):
                call()
    pair = (44100, 16000)
    H = resample_stream_history(*pair)
    hist, x, out = np.zeros(H, np.int16), np.ones(64, np.int16), np.zeros(64, np.float32)
    assert L.vad_resample_stream_ready(*pair, -1) == -ERR_ARG
    args = lambda g, h, a, n, o: (*pair, g, None if h is None else h.ctypes.data, None if a is None else a.ctypes.data, n,
                                  None if o is None else o.ctypes.data, None)
    assert L.vad_resample_stream_host(*args(-1, hist, x, 64, out)) == -ERR_ARG
    assert L.vad_resample_stream_host(*args(0, hist, x, -1, out)) == -ERR_ARG
    assert L.vad_resample_stream_host(*args(0, None, x, 64, out)) == -ERR_ARG
    assert L.vad_resample_stream_host(*args(0, hist, None, 64, out)) == -ERR_ARG
    assert L.vad_resample_stream_host(*args(0, hist, x, 64, None)) == -ERR_ARG          # (outputs are due: 64 > the latency)
    assert L.vad_resample_stream_host(*args(0, hist, x, 5, None)) == 0                            # (none is: no buffer needed)
    assert L.vad_resample_stream_host(*args(0, hist, x, 64, out)) == resample_stream_ready(*pair, 64) > 0
    for call in (lambda: resample_stream_ready(*pair, -1), lambda: resample_stream_ready(*pair, 1.5), lambda: resample_stream_ready(*pair, True),
                 lambda: resample_stream(x.astype(np.float32), *pair, 0, hist), lambda: resample_stream(x, *pair, 0, hist[:-1]),
                 lambda: resample_stream(x, *pair, 0, hist.astype(np.int32)), lambda: resample_stream(x[None], *pair, 0, hist),
                 lambda: resample_stream(x, *pair, -1, hist)):
        with pytest.raises((ValueError, _lib.VadError)):
            call()
