"""The native host helpers called from several host threads at once (no GPU needed).  ctypes releases the GIL around a foreign call,
so the calls below really run beside each other.  include/silero_vad_hip.h states which entry points serialise themselves on the
process-wide helper pool (vad_stage_rows, vad_segment_probs_batch: csrc/host_threads.hpp HostPool, one mutex around a run) and which
are re-entrant (vad_segment_probs, vad_iterator_feed, vad_g711_expand: no shared state); this file holds the library to both.
Every comparison is exact: a thread's result in the crowd must be the result the same call gave alone, before the threads started.
"""
import ctypes
import math
import threading

import numpy as np
import pytest

JOIN_S = 120
ROUNDS = 50


def run_threads(workers, timeout=JOIN_S):
    """One thread per worker, released together; a worker that raises fails the test (its exception is re-raised here, after the joins);
    a thread that has not finished after `timeout` seconds fails it too, at once and without a second try."""
    gate = threading.Barrier(len(workers))
    errors = []

    def body(fn):
        try:
            gate.wait(timeout)
            fn()
        except BaseException as e:       # noqa: BLE001 -- handed to the main thread
            errors.append(e)

    threads = [threading.Thread(target=body, args=(w,), daemon=True) for w in workers]
    for t in threads:
        t.start()
    for i, t in enumerate(threads):
        t.join(timeout)
        if t.is_alive():
            pytest.fail(f"worker {i} did not finish within {timeout} s")
    if errors:
        raise errors[0]


def walk_track(rng, B, T):
    """[B, T] probability tracks: the piecewise-smooth random walk of test_segmenter_matches_python_scan_on_random_probs, folded into
    [0, 1], so that runs of speech and of silence exist."""
    p = np.clip(np.cumsum(rng.normal(0, 0.15, (B, T)), axis=1) % 2.0, 0, 2)
    return np.ascontiguousarray(np.where(p > 1, 2 - p, p).astype(np.float32))


def scan_params(sr, **kw):
    from silero_vad_amd.streams import _segment_params
    return _segment_params(sr, **kw)


def segment_lists(segs, counts):
    return [segs[i, :counts[i]].tolist() for i in range(len(counts))]


class BatchScan:
    """One vad_segment_probs_batch call with everything it needs, ready to be repeated: -> per-stream segment lists."""

    def __init__(self, seed, sr, B, T, threads, **kw):
        rng = np.random.default_rng(seed)
        win = 512 if sr == 16000 else 256
        self.probs = walk_track(rng, B, T)
        self.nck = np.ascontiguousarray(rng.integers(0, T + 1, B), dtype=np.int64)
        self.alen = np.ascontiguousarray(np.maximum(0, self.nck * win - rng.integers(0, win, B)), dtype=np.int64)
        self.params = scan_params(sr, **kw)
        self.B, self.T, self.threads, self.cap = B, T, threads, T // 2 + 2

    def __call__(self):
        from silero_vad_amd import _lib
        lp = ctypes.POINTER(ctypes.c_long)
        segs = np.full((self.B, self.cap, 2), -7, np.int64)
        counts = np.full(self.B, -7, np.int64)
        total = _lib.lib().vad_segment_probs_batch(
            self.probs.ctypes.data_as(_lib.f32p), self.T, self.B, self.nck.ctypes.data_as(lp), self.alen.ctypes.data_as(lp),
            ctypes.byref(self.params), ctypes.cast(segs.ctypes.data, ctypes.POINTER(_lib.Segment)), self.cap, counts.ctypes.data_as(lp),
            self.threads)
        assert total == counts.sum() and counts.min() >= 0 and counts.max() <= self.cap
        return segment_lists(segs, counts)


class Stage:
    """One vad_stage_rows call over ragged rows of one dtype: -> the padded [n, width] batch."""

    def __init__(self, seed, dtype, n, width, threads):
        rng = np.random.default_rng(seed)
        self.base = (rng.integers(-30000, 30000, 1 << 21).astype(np.int16) if dtype == np.int16
                     else rng.standard_normal(1 << 21).astype(np.float32))
        self.lens = rng.integers(0, width + 1, n)
        self.lens[:3] = (0, width, 1)
        self.offs = rng.integers(0, len(self.base) - width, n)
        esz = self.base.itemsize
        self.rows = (ctypes.c_void_p * n)(*[self.base.ctypes.data + esz * int(o) for o in self.offs])
        self.clens = (ctypes.c_long * n)(*[int(v) for v in self.lens])
        self.n, self.width, self.threads, self.fill = n, width, threads, 0

    def __call__(self):
        from silero_vad_amd import _lib
        self.fill += 1                           # whatever the destination held before must be gone, padding included
        dst = np.full((self.n, self.width), self.fill, self.base.dtype)
        assert _lib.lib().vad_stage_rows(self.rows, self.clens, self.n, self.width, self.base.itemsize, dst.ctypes.data, self.threads) == 0
        return dst

    def definition(self):
        want = np.zeros((self.n, self.width), self.base.dtype)
        for i in range(self.n):
            want[i, :self.lens[i]] = self.base[self.offs[i]:self.offs[i] + self.lens[i]]
        return want


def test_pool_backed_helpers_from_four_threads_equal_their_solo_results(built):
    """Two threads in vad_segment_probs_batch (different tracks, parameters, both sample rates, 4 and default-many helper threads) and
    two in vad_stage_rows (int16 on 3 helper threads, float32 alternating between 1 -- the caller alone, no pool -- and 0 = the default)
    share the ONE process-wide HostPool: 50 calls each, all four released together.  The pool holds one job (fn_, next_, pending_ ...)
    and claims to serialise its callers; a job slot two callers wrote at once would hand one caller's items to the other's function,
    return before the own items are done, or never return.  Every call's result equals the one made alone."""
    scans = [BatchScan(21, 16000, 300, 1500, 4, threshold=0.3, min_silence_duration_ms=300, speech_pad_ms=100),
             BatchScan(22, 8000, 257, 1100, 0, max_speech_duration_s=2.0, use_max_poss_sil_at_max_speech=False, min_speech_duration_ms=100)]
    stages = [Stage(23, np.int16, 48, 120_000, 3), Stage(24, np.float32, 37, 70_001, 0)]
    want_scans = [s() for s in scans]
    assert all(sum(len(x) for x in w) > 100 for w in want_scans)
    want_stage = [s() for s in stages]
    for s, w in zip(stages, want_stage):
        assert np.array_equal(w, s.definition())
    # threads=0 takes the default count: below 2 such a caller would run alone, without the pool
    from silero_vad_amd import _lib
    assert _lib.lib().vad_host_threads() >= 2
    done = [0] * 4

    def scan_worker(k):
        def go():
            for _ in range(ROUNDS):
                assert scans[k]() == want_scans[k], f"segment_probs_batch caller {k}"
                done[k] += 1
        return go

    def stage_worker(k):
        def go():
            for r in range(ROUNDS):
                if k == 1:
                    stages[k].threads = (1, 3, 0)[r % 3]
                assert np.array_equal(stages[k](), want_stage[k]), f"stage_rows caller {k}"
                done[2 + k] += 1
        return go

    run_threads([scan_worker(0), scan_worker(1), stage_worker(0), stage_worker(1)])
    assert done == [ROUNDS] * 4


def _g711_codes(rng, n):
    return rng.integers(0, 256, n).astype(np.uint8)


def test_stateless_entry_points_are_reentrant(built):
    """vad_segment_probs, vad_iterator_feed and vad_g711_expand keep no state of their own (the iterator's lives in the caller's
    arrays): four threads, each on its own data, get what the same calls gave one after the other."""
    from silero_vad_amd import _lib, segment_probs
    from silero_vad_amd.streams import BatchVADIterator, g711_expand
    L = _lib.lib()
    jobs = []
    for k in range(4):
        rng = np.random.default_rng(40 + k)
        sr = (16000, 8000)[k % 2]
        win = 512 if sr == 16000 else 256
        tracks = walk_track(rng, 40, 600)
        kw = [dict(threshold=float(rng.choice([0.3, 0.5, 0.7])), min_speech_duration_ms=int(rng.choice([0, 100, 250])),
                   max_speech_duration_s=float(rng.choice([0.5, 1.0, 3.0, math.inf])), min_silence_duration_ms=int(rng.choice([0, 64, 100, 300])),
                   speech_pad_ms=int(rng.choice([0, 30, 100])), use_max_poss_sil_at_max_speech=bool(rng.integers(0, 2))) for _ in range(40)]
        lens = [600 * win - int(rng.integers(0, win)) for _ in range(40)]
        ticks = walk_track(rng, 64, 300).T.copy()                 # [ticks, slots]: 64 live streams over 300 ticks
        active = rng.random((300, 64)) < 0.9
        codes = _g711_codes(rng, 200_000 + k)
        codec = ("ulaw", "alaw")[k // 2]
        jobs.append((sr, tracks, kw, lens, ticks, active, codes, codec))

    def run(job):
        sr, tracks, kw, lens, ticks, active, codes, codec = job
        segs = [segment_probs(tracks[i], lens[i], sr, **kw[i]) for i in range(len(kw))]
        it = BatchVADIterator(64, threshold=0.55, sampling_rate=sr, min_silence_duration_ms=160)
        events = [it.feed(ticks[t], active=active[t]) for t in range(len(ticks))]
        tail = (it.triggered.copy(), it.temp_end.copy(), it.current_sample.copy())
        pcm = [g711_expand(codes, codec) for _ in range(10)]
        # the raw call too, into a buffer of the thread's own
        out = np.empty(len(codes), np.int16)
        assert L.vad_g711_expand(1 if codec == "ulaw" else 2, codes.ctypes.data, len(codes), out.ctypes.data) == 0
        return segs, events, tail, pcm, out

    want = [run(j) for j in jobs]
    assert all(sum(len(s) for s in w[0]) > 20 and sum(len(e) for e in w[1]) > 50 for w in want)
    got = [None] * 4

    def worker(k):
        def go():
            for _ in range(3):
                got[k] = run(jobs[k])
                segs, events, tail, pcm, out = got[k]
                assert segs == want[k][0] and events == want[k][1], k
                assert all(np.array_equal(a, b) for a, b in zip(tail, want[k][2])), k
                assert all(np.array_equal(p, want[k][4]) for p in pcm) and np.array_equal(out, want[k][4]), k
        return go

    run_threads([worker(k) for k in range(4)])
    assert all(g is not None for g in got)
