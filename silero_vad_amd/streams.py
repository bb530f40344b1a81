"""Many streams at once: the two callers BASELINE.json's configs name on top of the engine.

* ``ragged_probs`` / ``RaggedPlan`` -- offline corpora (configs[3]).  ``audio_forward`` assumes
  equal-length rows (JIT!/vad/model/vad_annotator.py:141-148); real corpora are ragged.  The
  network is causal (a chunk's probability depends only on samples up to the end of that chunk,
  and the reference right-pads the last partial chunk with zeros, :141-148), so a recording that
  is right-padded with zeros to its bucket's length yields bit-identical probabilities for its
  own ceil(len / N) chunks.  The plan sorts recordings by length and cuts buckets so that padding
  waste and bytes per GPU call stay bounded; each bucket is one lock-step ``vad_forward_audio``
  call.  Recordings that already sit in PINNED host memory are DMA'd / gathered straight into the device batch
  (vad_upload_rows: no host-side copy at all); pageable ones go through a threaded copy into pinned staging first
  (vad_stage_rows).  int16 halves the PCIe bytes.

* ``StreamPool`` -- live streams (configs[4]).  Per-stream LSTM state and context stay resident
  in HBM (the resumable unit of the reference model object, vad_annotator.py:7-8,72,87); one
  hipGraph-captured ``vad_step`` serves every open stream per 32 ms tick; streams are opened and
  closed by slot, a fresh slot starting from zero state like ``reset_states()`` (:157-162).

* ``BatchVADIterator`` -- the reference's streaming event logic (``VADIterator``,
  src/silero_vad/utils_vad.py:507-549) for all slots of a pool at once, vectorised on the host.
"""
import collections
import contextlib
import ctypes
import math
import os
import time
import types
from typing import List, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import lib


# Cumulative counters of the corpus path since the last STATS.clear() (bench.py --config corpus reads them):
# stage_s host packing into pinned memory, h2d_bytes / h2d_s the H2D copies themselves (hipEvents on the copy
# stream), scan_s the native segmenter, buckets, padded / real samples staged; ragged_speech_audio: collect_bytes the audio kept on the
# device, audio_d2h_bytes / audio_d2h_s what of it was brought home (copy-stream events), collect_host_rows the rows left to the host.
STATS = collections.defaultdict(float)
TRACE = None             # bring-up: set to a list to collect (slab, t before on_slab, t after, t after stage) from the refill loop
AUDIO_TRACE = None       # measurement: set to a list to collect (start event, end event, bytes) of ragged_speech_audio's D2H copies


def chunk_size(sr: int) -> int:
    if sr not in (8000, 16000):
        raise ValueError("Supported sampling rates: [8000, 16000] (or multiply of 16000)")
    return 512 if sr == 16000 else 256


def _rates(sr: int):
    """(rate of the net that serves `sr`, decimation step k, INPUT samples per chunk): a multiple of 16 kHz runs on the 16 kHz net
    over every k-th sample (src/silero_vad/utils_vad.py:301-307, JIT!/vad/model/vad_annotator.py:104-112).  The corpus schedulers
    keep such recordings at their raw rate all the way into HBM -- lengths, buckets, slabs and row pitches count RAW samples, a chunk
    is 512 k of them -- and the frontend's loads take every k-th sample (csrc/fft_wave.hpp load_vec<SL, DEC>): no decimated copy on
    the host, none on the device."""
    if sr > 16000 and sr % 16000 == 0:
        return 16000, sr // 16000, 512 * (sr // 16000)
    return sr, 1, chunk_size(sr)


# ---- offline: ragged corpora ------------------------------------------------------------------------
def _bucket_cuts(L: np.ndarray, max_waste: float, max_bytes: int, itemsize: int, mate=None):
    """The greedy bucketing of RaggedPlan on arrays: -> (order, cuts) with order = the non-empty recordings by descending length (ties in
    index order) and bucket k = order[cuts[k] : cuts[k + 1]].  A bucket takes recordings while the zero padding to its first (longest)
    member wastes at most max_waste of its samples and its padded size stays within max_bytes; the waste grows with every (shorter)
    member, so the first violation ends the bucket -- found block-wise on prefix sums instead of one Python iteration per recording
    (151 552 recordings of a corpus shard: 85 ms of planning in front of the first upload before, ~10 after)."""
    live = np.flatnonzero(L > 0)
    order = live[np.argsort(-L[live], kind="stable")]
    Ls = L[order]
    cs = np.zeros(len(order) + 1, dtype=np.int64)
    np.cumsum(Ls, out=cs[1:])
    cuts = [0]
    s, n = 0, len(order)
    while s < n:
        mx = int(Ls[s])
        hi = min(n - s, max(1, max_bytes // (mx * itemsize)))     # the first member is always taken
        cnt, k0, blk = hi, 2, 256
        while k0 <= hi:
            k = np.arange(k0, min(hi, k0 + blk - 1) + 1, dtype=np.int64)          # members the bucket would have
            waste = 1.0 - (cs[s + k] - cs[s]) / (mx * k)
            bad = np.flatnonzero(waste > max_waste)
            if len(bad):
                cnt = int(k[bad[0]]) - 1
                break
            k0 += blk
            blk *= 2
        # mate[i]: entry i + 1 is the other channel of entry i's recording (equal lengths: neighbours after the sort).  A bucket does not
        # end between them -- the pair opens the next one -- so that one source of the upload serves both rows.
        if mate is not None and cnt > 1 and s + cnt < n and mate[order[s + cnt - 1]] and order[s + cnt] == order[s + cnt - 1] + 1:
            cnt -= 1
        s += cnt
        cuts.append(s)
    return order, cuts


class RaggedPlan:
    """Buckets of recording indices, each processed as one lock-step batch.

    ``lengths`` in samples.  A bucket holds recordings whose zero-padding to the bucket's longest
    member wastes at most ``max_waste`` of the bucket's samples, and at most ``max_bytes`` of
    staged PCM (``itemsize`` bytes per sample)."""

    def __init__(self, lengths: Sequence[int], max_waste: float = 0.15, max_bytes: int = 1 << 30,
                 itemsize: int = 4, mate=None):
        L = np.asarray(lengths, dtype=np.int64).reshape(-1)
        self.lengths = L.tolist()
        self.empty = np.flatnonzero(L <= 0).tolist()
        order, cuts = _bucket_cuts(L, max_waste, max_bytes, itemsize, mate)
        self.buckets: List[List[int]] = [order[cuts[k]:cuts[k + 1]].tolist() for k in range(len(cuts) - 1)]

    def padded_samples(self) -> int:
        return sum(self.lengths[b[0]] * len(b) for b in self.buckets)

    def real_samples(self) -> int:
        return sum(n for n in self.lengths if n > 0)


class _StagePool:
    """Pinned host buffers + device buffers reused for every bucket (pinned allocation is expensive): one more slot
    than there are compute lanes, so that staging + H2D of the next bucket overlap the kernels of the buckets in flight."""

    def __init__(self, device, slots=2):
        self.device = device
        self.slots = slots
        self.host = [None] * slots
        self.dev = [None] * slots
        self.done = [None] * slots          # event: H2D of this slot finished (host buffer reusable)
        self.consumed = [None] * slots      # event: the kernels that read this slot's device buffer finished
        self.meta = [None] * slots          # pinned int64 scratch per slot (refill: scatter indices, resets)
        self.stream = torch.cuda.Stream(device)

    def meta_buffer(self, i, n):
        """Pinned int64[n] owned by slot i (valid until the slot is handed out again): `tensor.pin_memory()` per slab
        costs a pinned allocation each time -- 5.6 ms for 1 MB on the MI355X hosts, more than the slab's kernels."""
        if self.meta[i] is None or self.meta[i].numel() < n:
            self.meta[i] = torch.empty(max(n, 1024), dtype=torch.int64, pin_memory=True)
        return self.meta[i][:n]

    def get(self, k, nbytes, dev_bytes=None):
        """Slot for bucket k with `nbytes` of pinned staging (0: the source is pinned already, no staging) and
        `dev_bytes` (default: nbytes) of device buffer."""
        i = k % self.slots
        dev_bytes = nbytes if dev_bytes is None else dev_bytes
        t0 = time.perf_counter()
        if self.done[i] is not None:
            self.done[i].synchronize()
        STATS["slot_wait_s"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        if nbytes and (self.host[i] is None or self.host[i].numel() < nbytes):
            self.host[i] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
        if self.dev[i] is None or self.dev[i].numel() < dev_bytes:
            cap = max(dev_bytes, 1 << 20)
            # The device buffer is written on self.stream first: allocate it there, so that a block the caching
            # allocator recycles is ordered after its previous use on that stream, and make self.stream wait for
            # whatever the consumer stream still has in flight (the block may come from its pool, e.g. the
            # previous call's probs during their D2H copy).  Consumers call record_stream() on their views.
            cur = torch.cuda.current_stream(self.device)
            self.stream.wait_stream(cur)
            with torch.cuda.stream(self.stream):
                self.dev[i] = torch.empty(cap, dtype=torch.uint8, device=self.device)
            self.consumed[i] = None
            STATS["slot_allocs"] += 1
        STATS["slot_alloc_s"] += time.perf_counter() - t0
        return i


def _distinct_queue_stream(engine, device, others, tries=12, priority=0):
    """A torch stream whose kernels demonstrably run BESIDE those of every stream in `others` (vad_streams_overlap).  torch hands out
    streams from a pool, the HIP runtime maps them onto ~4 hardware queues in the order of their first use, and two streams on one
    queue serialise: an upload kernel that lands on a compute lane's queue alternates with the lane instead of overlapping it -- the
    scattered-pinned routes then read half the link (profiles/r05_ingest_queues.md).  torch's pool hands its streams out round-robin
    whatever is still alive, so the search simply asks for the next one; every candidate, the last one included, is probed, and when
    none of `tries` candidates runs beside all of `others` the best one found is returned and STATS["stream_collisions"] says so (the
    caller's pipeline is then correct but partly serial).  The probe synchronises the streams involved (~1 ms per pair): it is skipped
    -- a plain new stream is returned -- while the current stream is being captured into a graph."""
    st = torch.cuda.Stream(device, priority=priority)
    if engine is None or not hasattr(engine, "streams_overlap") or torch.cuda.is_current_stream_capturing():
        return st
    best, best_hits = st, -1
    for k in range(tries):
        hits = sum(1 for o in others if engine.streams_overlap(o, st))
        if hits > best_hits:
            best, best_hits = st, hits
        if hits == len(others):
            break
        STATS["stream_retries"] += 1
        if k + 1 < tries:
            st = torch.cuda.Stream(device, priority=priority)
    if best_hits < len(others):
        STATS["stream_collisions"] += 1
    return best


def _copy_stream(pool, model, device, others):
    """The staging pool's stream for the arena windows' DMAs, on a hardware queue that carries none of `others` (compute lanes, the
    cut / upload stream): the runtime orders a copy inside its stream's queue, so a 37 ms window DMA on a lane's queue stands in front
    of that lane's kernels (the raw 48 kHz corpus leg read 0.71 instead of 0.96 of the link when an unprobed stream landed there
    after other legs had created streams of their own).  Made once per pool."""
    st = getattr(pool, "copy_stream", None)
    if st is None:
        st = pool.copy_stream = _distinct_queue_stream(getattr(model, "engine", None), device, list(others))
    return st


def _compute_lanes(model, want):
    """[(model, stream)]: lane 0 is the caller's model on the caller's stream; further lanes are CLONES of its engine
    (vad_clone: the same weight images and options, their own scratch -- no second weight copy, no option drift) on
    their own streams.  A bucket's recurrence is latency-bound -- 4.4 us per time step on as few CUs as the bucket has
    stream tiles -- so buckets on different lanes overlap: one lane's recurrence runs beside the other lane's frontend
    instead of in front of it.  Memory: each lane holds its own gx scratch (up to the engine's gx_cap_mib)."""
    cur = torch.cuda.current_stream(model.device)
    lanes = [(model, cur)]
    eng = getattr(model, "engine", None)
    if want > 1 and eng is not None and hasattr(eng, "clone"):
        sibs = getattr(model, "_lane_siblings", None)
        if sibs is None or getattr(model, "_lane_options", None) != dict(eng.options):
            sibs = model._lane_siblings = []             # the primary's options changed: fresh clones carry the new ones
            model._lane_options = dict(eng.options)
        while len(sibs) < want - 1:             # (each lane on a hardware queue of its own: _distinct_queue_stream)
            sibs.append((type(model)(engine=eng.clone()), _distinct_queue_stream(eng, model.device, [cur] + [s for _, s in sibs])))
        lanes.extend(sibs[: want - 1])
    return lanes


class PackedRecordings:
    """Many recordings inside ONE host tensor -- a decoder's output arena, a memory-mapped shard: recording i is
    `base[offsets[i] : offsets[i] + lengths[i]]` (a uint8 base: G.711 codes, 1 byte a sample, packed at any byte offset -- pass
    `codec=` to the corpus function).  Accepted wherever the corpus functions take a list of recordings; it
    spares the per-recording Python work (150 000 tensor views cost more host time than their audio costs GPU time) and,
    when `base` is pinned, the whole set is one page-locked source for `vad_upload_rows`."""

    def __init__(self, base: torch.Tensor, offsets, lengths):
        if base.dim() != 1 or base.is_cuda or not base.is_contiguous() or base.dtype not in (torch.int16, torch.float32, torch.uint8):
            raise ValueError("base must be a contiguous 1-D CPU tensor of int16 or float32 samples, or of uint8 G.711 codes "
                             "(the corpus functions' `codec` says which law)")
        self.base = base
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.lengths = np.ascontiguousarray(lengths, dtype=np.int64)
        if self.offsets.shape != self.lengths.shape or self.offsets.ndim != 1:
            raise ValueError("offsets and lengths need one entry per recording")
        if len(self.offsets) and (self.offsets.min() < 0 or self.lengths.min() < 0
                                  or int((self.offsets + self.lengths).max()) > base.numel()):
            raise ValueError("a recording lies outside base")

    def __len__(self):
        return len(self.offsets)

    def __getitem__(self, i):
        o, m = int(self.offsets[i]), int(self.lengths[i])
        return self.base[o:o + m]

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def windows(self, max_bytes: int):
        """Index ranges [lo, hi) of recordings that lie in arena order without overlap and whose span (first sample of the
        first .. last sample of the last) is at most `max_bytes`: each can be brought to the GPU by ONE copy."""
        esz = self.base.element_size()
        out, n = [], len(self)
        lo = 0
        end = self.offsets + self.lengths
        while lo < n:
            hi = lo + 1
            while hi < n and self.offsets[hi] >= end[hi - 1] and (end[hi] - self.offsets[lo]) * esz <= max_bytes:
                hi += 1
            out.append((lo, hi))
            lo = hi
        return out


def _arena_windows(offs: np.ndarray, lens: np.ndarray, limit: int, lead_limit: int = 0):
    """The arena windows of a PackedRecordings (WindowedPlan's rules; also the refill route's window feed): (order, bounds, o, e) --
    `order` = the live recordings in the order they are walked (by offset when nothing overlaps, else as handed over), `bounds` =
    [(lo, hi)] index ranges of `order`, one per window: runs in which the offsets do not turn back, cut greedily where the span would
    exceed `limit` samples (a window always takes its first recording); o / e = first / one-past-last sample of order's recordings.
    On arrays: one searchsorted per window instead of one iteration per recording.  lead_limit: the FIRST windows are cut at lead_limit,
    2 lead_limit, 4 lead_limit ... samples until `limit` is reached (the refill route's first slabs read little and should not wait
    for a whole window)."""
    live = np.flatnonzero(lens > 0)
    by_offset = live[np.argsort(offs[live], kind="stable")]
    ends = offs[by_offset] + lens[by_offset]
    overlap_free = bool(np.all(offs[by_offset][1:] >= ends[:-1])) if len(by_offset) > 1 else True
    order = by_offset if overlap_free else live
    o, e = offs[order], offs[order] + lens[order]
    turns = np.flatnonzero(o[1:] < e[:-1]) + 1 if len(order) > 1 else np.zeros(0, dtype=np.int64)
    starts = np.concatenate([[0], turns, [len(order)]]).astype(np.int64) if len(order) else np.zeros(1, dtype=np.int64)
    bounds = []
    for r in range(len(starts) - 1):
        lo, hi = int(starts[r]), int(starts[r + 1])
        while lo < hi:
            lim = min(limit, lead_limit << min(len(bounds), 40)) if lead_limit else limit
            nxt = lo + max(1, int(np.searchsorted(e[lo:hi], o[lo] + lim, side="right")))     # (e - a0) > limit ends the window
            bounds.append((lo, nxt))
            lo = nxt
    return order, bounds, o, e


class WindowedPlan:
    """RaggedPlan per arena window.  A window is a set of recordings whose span -- first sample of the first .. last sample
    of the last -- is at most `window_bytes` and which lie in it in arena order without overlap, so that ONE DMA of the span
    brings exactly their bytes to the GPU; the recordings of a window are bucketed among themselves.
      * recordings that do not overlap anywhere are walked in arena order (sorted by offset), whatever order they were handed
        over in;
      * a set with overlaps -- a ring buffer that was refilled: the same offsets mean DIFFERENT audio at different times -- is
        walked in the order it was handed over, and a window ends where the order turns back (the wrap of the ring): a byte is
        never copied once for two recordings.
    `density` = live bytes / copied bytes: a sparse set (recordings scattered over a large arena) is better served by the
    gather kernel (streams.ragged_buckets)."""

    def __init__(self, rec: PackedRecordings, max_waste, max_bytes, itemsize, window_bytes, on_windows=None, src_itemsize=None, fan=None):
        """itemsize: bytes per sample of the DEVICE batch (what the buckets are planned on); src_itemsize (default: the same): bytes per
        sample in the arena, what a window's span is measured in -- 1 for G.711 recordings, whose batch is int16.
        on_windows(plan): called as soon as the windows, their spans and the density are known and BEFORE the buckets are planned --
        the hook for starting the first windows' DMA while the rest of the planning runs.
        fan (_Fanned over rec): the recordings are interleaved -- the windows are those of the recordings, the buckets (and lengths,
        empty, windows) are of the batch ROWS they fan out to, a recording's channels in one bucket."""
        offs, lens = rec.offsets, rec.lengths
        row_lens = lens if fan is None else fan.lengths
        self.lengths = row_lens.tolist()
        self.empty = np.flatnonzero(row_lens <= 0).tolist()
        order, bounds, o, e = _arena_windows(offs, lens, window_bytes // (src_itemsize or itemsize))
        live = order
        rows_in = (lambda r: r) if fan is None else fan.rows_of
        self.windows = [rows_in(order[a:b]).tolist() for a, b in bounds]      # recording (row) indices of each window (arena order)
        self.span = [(int(o[a]), int(e[b - 1])) for a, b in bounds]  # (first, last + 1) sample
        copied = sum(b - a for a, b in self.span)
        self.density = float(lens[live].sum()) / copied if copied else 0.0
        self.buckets, self.window_of = [], []
        if on_windows is not None:
            on_windows(self)
        for w, (a, b) in enumerate(bounds):
            idx = rows_in(order[a:b])
            sub_order, cuts = _bucket_cuts(row_lens[idx], max_waste, max_bytes, itemsize, None if fan is None else fan.mate[idx])
            glob = idx[sub_order]
            for k in range(len(cuts) - 1):
                self.buckets.append(glob[cuts[k]:cuts[k + 1]].tolist())
                self.window_of.append(w)

    def mean_window_fill(self):
        return float(np.mean([len(w) for w in self.windows])) if self.windows else 0.0


def _as_packed(audios):
    """A list of recordings that are all contiguous views of ONE host storage (a decoder's output buffer, sliced) as a
    PackedRecordings over that storage; None if they are not."""
    if isinstance(audios, PackedRecordings) or len(audios) < 2:
        return None
    first = audios[0]
    if not torch.is_tensor(first) or first.is_cuda or first.dtype not in (torch.int16, torch.float32, torch.uint8):
        return None
    st = first.untyped_storage()
    key, dtype, esz = st.data_ptr(), first.dtype, first.element_size()
    offs = np.empty(len(audios), dtype=np.int64)
    lens = np.empty(len(audios), dtype=np.int64)
    for i, a in enumerate(audios):
        if not torch.is_tensor(a) or a.dtype != dtype or a.dim() != 1 or a.is_cuda or (a.numel() > 1 and a.stride(0) != 1) \
                or a.untyped_storage().data_ptr() != key:
            return None
        offs[i] = a.storage_offset()
        lens[i] = a.shape[0]
    base = torch.empty(0, dtype=dtype).set_(st, 0, (st.nbytes() // esz,))
    return PackedRecordings(base, offs, lens)


def _describe(audios):
    """(is int16, lengths as a list of ints) of a list of recordings or a PackedRecordings."""
    if isinstance(audios, PackedRecordings):
        return audios.base.dtype == torch.int16, audios.lengths.tolist()
    if isinstance(audios, _Fanned):
        return True, audios.lengths.tolist()
    as_i16 = len(audios) > 0 and all(torch.is_tensor(a) and a.dtype == torch.int16 for a in audios)
    return as_i16, [int(a.shape[0]) if hasattr(a, "shape") else len(a) for a in audios]


def _sample_kind(dtype):
    """what a recording's samples are: G.711 codes (uint8), int16 PCM, or something that is converted to float32"""
    return 0 if dtype == torch.uint8 else 1 if dtype == torch.int16 else 2


_MIXED_U8 = "mixed uint8 (G.711) / int16 / float recordings in one call"


def _is_u8(a):
    return str(getattr(a, "dtype", "")) in ("torch.uint8", "uint8")


def _codec_of(audios, codec):
    """The `codec` argument of a corpus call, checked against its recordings: -> None (int16 / float recordings, no codec) or the codec
    of every recording as uint8 ids (1 mu-law, 2 A-law).  uint8 recordings without a codec are refused -- bytes are never guessed at --
    and so is uint8 mixed with int16 / float."""
    n = len(audios)
    u8 = [audios.base.dtype == torch.uint8] * n if isinstance(audios, PackedRecordings) else [_is_u8(a) for a in audios]
    if codec is None:
        if any(u8):
            raise TypeError("uint8 recordings need codec='ulaw' | 'alaw' (or one per recording): bytes are never guessed at")
        return None
    cd = np.full(n, _codec_id(codec), np.uint8) if isinstance(codec, (str, int, np.integer)) else _codec_rows(codec)
    if len(cd) != n:
        raise ValueError(f"codec needs one entry per recording: {len(cd)} for {n}")
    if n and (cd.min() < _PCM["ulaw"] or cd.max() > _PCM["alaw"]):
        raise ValueError("a corpus codec is 'ulaw' or 'alaw'")
    if not all(u8):
        raise TypeError(_MIXED_U8 if any(u8) else "codec given, but the recordings are not uint8 G.711 codes")
    return cd


def _coded_input(audios, codec, model):
    """(recordings, codec ids per recording or None) as the schedulers take them.  A model whose engine has the device expansion
    (Engine.upload_rows_coded) gets the G.711 bytes as they are; any other (a CPU stand-in) gets them expanded on the host (g711_expand)
    as int16 recordings -- the definition of what the device route computes."""
    cd = _codec_of(audios, codec)
    if cd is None or hasattr(getattr(model, "engine", None), "upload_rows_coded"):
        return audios, cd
    out = []
    for a, c in zip(audios, cd):
        a = a if torch.is_tensor(a) else torch.as_tensor(a)
        out.append(torch.from_numpy(g711_expand(a.contiguous().numpy(), int(c))))
    return out, None


MAX_CHANNELS = 2         # include/silero_vad_hip.h VAD_MAX_CHANNELS


def _channel_counts(channels, n):
    """`channels` as one int64 count per recording, checked (the one checker of `_channels_of` and `channel_rows`).  n: the number of
    recordings, None if the caller does not know it (a single int then cannot be spread)."""
    if isinstance(channels, (int, np.integer)) and not isinstance(channels, (bool, np.bool_)):
        if n is None:
            raise ValueError("channels as one int needs the number of recordings")
        ch = np.full(int(n), int(channels), np.int64)
    else:
        ch = np.asarray(channels)
        if ch.ndim != 1 or (ch.size and not np.issubdtype(ch.dtype, np.integer)):
            raise ValueError("channels must be an int or one int per recording")
        ch = ch.astype(np.int64)
    if n is not None and len(ch) != n:
        raise ValueError(f"channels needs one entry per recording: {len(ch)} for {n}")
    if ch.size and (ch.min() < 1 or ch.max() > MAX_CHANNELS):
        raise ValueError(f"a recording has 1 ... {MAX_CHANNELS} channels")
    return ch


def _channels_of(audios, channels):
    """The `channels` argument of a corpus call, checked: -> None (every recording is mono: the call is today's) or the channel count
    of every recording as int64."""
    if channels is None:
        return None
    ch = _channel_counts(channels, len(audios))
    return ch if ch.size and ch.max() > 1 else None


def channel_rows(channels, n: int = None) -> list:
    """The (recording, channel) pairs that the flat indices of a `channels=` call stand for, recording-major: entry k of a result -- a
    probability tensor, a segment list, an index that `ragged_buckets` or `refill_segments_stream` yields -- belongs to
    channel_rows(channels, n)[k].  channels: an int (then n recordings) or one int per recording."""
    ch = _channel_counts(channels, n)
    return [(i, c) for i, m in enumerate(ch.tolist()) for c in range(int(m))]


class _Fanned:
    """The recordings of a `channels=` call beside the flat list of batch rows they fan out to: row k is channel ch_of[k] of recording
    rec_of[k], recording-major (channel_rows), `lengths[k]` FRAMES long.  The schedulers plan on the rows -- len(), lengths and every
    index they yield are the rows' -- and read the recordings (`audios`: a list or a PackedRecordings of interleaved int16 samples or
    G.711 codes, `cd` their codec ids or None) only to build the sources of an upload (table)."""

    def __init__(self, audios, ch, cd):
        if isinstance(audios, PackedRecordings):
            kinds, elems = {_sample_kind(audios.base.dtype)}, audios.lengths
        else:
            audios = [a if torch.is_tensor(a) else torch.as_tensor(a) for a in audios]
            if any(a.dim() != 1 for a in audios):
                raise ValueError("a recording with channels is a 1-D tensor of interleaved samples, as in a WAV data chunk")
            kinds, elems = {_sample_kind(a.dtype) for a in audios}, np.asarray([a.shape[0] for a in audios], dtype=np.int64)
        if 2 in kinds:
            raise TypeError("float recordings with more than one channel: the device batch the channels are split into is int16 -- "
                            "hand over int16 samples, or G.711 codes with `codec`")
        if ((elems % ch) != 0).any():
            raise ValueError("an interleaved recording of 2 channels has an even number of samples")
        self.audios, self.C, self.cd = audios, ch, cd
        self.frames = elems // ch
        self.row0 = np.concatenate([[0], np.cumsum(ch)[:-1]]).astype(np.int64)       # a recording's first row
        self.rec_of = np.repeat(np.arange(len(ch), dtype=np.int64), ch)
        self.ch_of = np.arange(len(self.rec_of), dtype=np.int64) - self.row0[self.rec_of]
        self.lengths = self.frames[self.rec_of]
        self.mate = (self.C[self.rec_of] == 2) & (self.ch_of == 0)                   # row k + 1 is row k's sibling channel

    def __len__(self):
        return len(self.rec_of)

    def rows_of(self, recs):
        """the rows of recordings `recs`, in their order"""
        recs = np.asarray(recs, dtype=np.int64)
        reps = self.C[recs]
        first = np.repeat(self.row0[recs], reps)
        within = np.arange(int(reps.sum()), dtype=np.int64) - np.repeat(np.cumsum(reps) - reps, reps)
        return first + within

    def table(self, rows, at=None, batch_rows=None):
        """The sources of an upload whose batch row batch_rows[j] (default: j) is row rows[j], from sample at[j] (default: 0) of its
        channel on: -> (recording of every source, first frame of every source, position in `rows` of every source's first row,
        int32 [n_src, 2] batch row of each channel or -1).  Rows that want the same frames of one recording share ONE source: every
        source byte is read once."""
        rows = np.asarray(rows, dtype=np.int64)
        rec, ch = self.rec_of[rows], self.ch_of[rows]
        at = np.zeros(len(rows), dtype=np.int64) if at is None else np.asarray(at, dtype=np.int64)
        key = rec * (int(self.frames.max()) + 1 if len(self.frames) else 1) + at
        _, first, inv = np.unique(key, return_index=True, return_inverse=True)
        dst = np.full((len(first), MAX_CHANNELS), -1, dtype=np.int32)
        dst[inv.reshape(-1), ch] = np.arange(len(rows)) if batch_rows is None else batch_rows
        return rec[first], at[first], first, dst


def _channel_input(audios, codec, channels, model):
    """(recordings, codec, fan) as the schedulers take them; the public corpus calls resolve `channels=` here, once, and hand `fan` down
    through the schedulers' private `_fan=`.  Mono (channels None or all 1): as handed over, fan None.  Otherwise a model whose engine
    splits on the device (Engine.upload_rows_channels) keeps the interleaved recordings, with fan = the _Fanned over them (it carries
    the codecs: codec None); any other (a CPU stand-in) gets the flat list of de-interleaved int16 recordings, fan None -- the
    definition of what the device route computes."""
    ch = _channels_of(audios, channels)
    if ch is None:
        return audios, codec, None
    cd = _codec_of(audios, codec)
    fan = _Fanned(audios, ch, cd)
    if hasattr(getattr(model, "engine", None), "upload_rows_channels"):
        return fan.audios, None, fan
    out = []
    for i, a in enumerate(fan.audios):
        x = a.contiguous().numpy()
        for c in range(int(ch[i])):
            out.append(torch.from_numpy(deinterleave(x, int(ch[i]), c, None if cd is None else int(cd[i]))))
    return out, None, None


def _corpus_input(audios, model, codec, channels, fan):
    """What both corpus schedulers open with: `channels=` and `codec=` resolved (_channel_input -- unless a public caller did that
    already and hands its `fan` down --, _coded_input) and the sample formats that follow.  -> recs (the recordings to read), lengths
    (of the batch ROWS: the recordings', or with interleaved recordings their channels'), cd (codec ids per recording or None), fan
    (_Fanned or None), coded, and dtype / esz of the DEVICE batch beside src_dtype / src_esz of the source (1 byte a sample for G.711).
    The sources themselves are read later, once the plan is known (_Ingest): a window route swaps a list for its PackedRecordings."""
    if fan is None:
        audios, codec, fan = _channel_input(audios, codec, channels, model)
    if fan is not None:                                   # interleaved recordings: `recs` the sources, lengths / plan / indices the rows'
        recs, cd = fan.audios, fan.cd
    else:
        recs, cd = _coded_input(audios, codec, model)
    as_i16, lengths = _describe(recs if fan is None else fan)
    coded = cd is not None
    dtype, esz = (torch.int16, 2) if as_i16 or coded else (torch.float32, 4)
    src_dtype, src_esz = (torch.uint8, 1) if coded else (dtype, esz)
    return types.SimpleNamespace(recs=recs, lengths=lengths, cd=cd, fan=fan, coded=coded, dtype=dtype, esz=esz, src_dtype=src_dtype, src_esz=src_esz)


def _pack_rows(ptr, lens, pitch, esz, dst_ptr):
    """Rows at host addresses `ptr` (uint64), `lens` elements of `esz` bytes each, into [len(ptr)][pitch] at host address dst_ptr, zero
    padded, with the native threaded copy."""
    ptr, lens = np.ascontiguousarray(ptr, dtype=np.uint64), np.ascontiguousarray(lens, dtype=np.int64)
    rc = lib().vad_stage_rows(ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)), lens.ctypes.data_as(ctypes.POINTER(ctypes.c_long)),
                              len(ptr), pitch, esz, dst_ptr, 0)
    if rc:
        raise _lib.VadError(rc, "vad_stage_rows")


def _stage_sources(ptr, frames, ch, width, src_esz, host):
    """Pageable interleaved sources into the pinned staging block `host` (uint8) as the bytes they are: the one-channel sources at a
    pitch of `width` elements, behind them the two-channel ones at 2 x width (vad_stage_rows, once per pitch) -> byte offset of every
    source in the block.  The block holds what the batch rows of these sources hold, no more."""
    off = np.zeros(len(ptr), dtype=np.int64)
    at = 0
    for c in range(1, MAX_CHANNELS + 1):
        sel = np.flatnonzero(ch == c)
        if not len(sel):
            continue
        _pack_rows(ptr[sel], frames[sel] * c, width * c, src_esz, host.data_ptr() + at)
        off[sel] = at + np.arange(len(sel), dtype=np.int64) * width * c * src_esz
        at += len(sel) * width * c * src_esz
    return off


def _ingest_route(windowed, direct, interleaved, coded, nbytes, staged=0):
    """How a device batch of `nbytes` gets into HBM, and the staging slot it needs: -> (route, (pinned staging bytes, device bytes)).
      "cut"     the sources are device addresses inside an arena window's copy: the gather kernel cuts the batch out of it (how 2);
      "pinned"  the sources sit in page-locked memory: the gather kernel reads them over the link, or one DMA per row (how 1 / 0);
    neither needs staging.  Pageable sources are packed into the slot's pinned staging and cross the link in ONE copy:
      "copy"    plain samples, straight into the batch;
      "codes"   G.711 codes, staged as bytes (half the int16 batch) into a device block BEHIND the batch, which the expansion reads;
      "sources" interleaved sources, whatever their codec (`staged`: their bytes), into such a block, which the split reads."""
    if windowed or direct:
        return "cut" if windowed else "pinned", (0, nbytes)
    if interleaved:
        return "sources", (staged, nbytes + staged)
    if coded:
        return "codes", (nbytes // 2, nbytes + nbytes // 2)
    return "copy", (nbytes, nbytes)


class _Batch:
    """What a scheduler says about one batch of an upload, as plain arrays: `ptr` (uint64) the sources' addresses -- host ones, or
    device ones on the window routes --, `lens` (int64) their samples (frames, where interleaved), `codecs` (uint8 ids) or None,
    `channels` (uint8 counts: the sources are interleaved) or None with `rows_of` the int32 [sources, 2] batch row of each channel
    (-1: not wanted), into a batch of n_rows x pitch samples.  Without channels, source j IS batch row j."""
    __slots__ = ("ptr", "lens", "codecs", "channels", "rows_of", "n_rows", "pitch")

    def __init__(self, ptr, lens, codecs, channels, rows_of, n_rows, pitch):
        def arr(x, dtype):
            return None if x is None else np.ascontiguousarray(x, dtype=dtype)

        self.ptr, self.lens, self.codecs = arr(ptr, np.uint64), arr(lens, np.int64), arr(codecs, np.uint8)
        self.channels, self.rows_of, self.n_rows, self.pitch = arr(channels, np.uint8), arr(rows_of, np.int32), n_rows, pitch


class _Ingest:
    """The one place that knows how a batch of rows gets into HBM (_ingest_route: the matrix of sample format x where the bytes lie);
    the schedulers only say which rows (_Batch).  Made once per corpus call, after the plan: it holds the call's _Sources (`src`) and
    what follows from them -- `direct` (every recording is page-locked: no host copy) and `how` (1 the gather kernel, 0 one DMA per row).
    A scheduler that took a window route sets `windowed`.  Staging a batch has a host half (`host`) and a device half (`device`, inside
    the scheduler's own `with torch.cuda.stream(pool.stream)`); the stream choreography around them is the scheduler's."""

    def __init__(self, inp, recs, pool, engine, on_gpu):
        self.pool, self.engine = pool, engine
        self.dtype, self.esz, self.src_dtype, self.src_esz = inp.dtype, inp.esz, inp.src_dtype, inp.src_esz
        self.coded, self.interleaved = inp.coded, inp.fan is not None
        mode = _upload_mode()
        self.src = _Sources(recs, inp.src_dtype, check_pinned=on_gpu and mode != "stage" and hasattr(engine, "upload_rows"))
        self.direct = self.src.pinned
        self.windowed = False
        self.how = 0 if mode == "dma" else 1
        if (self.coded or self.interleaved) and self.how == 0:
            import warnings
            warnings.warn("SILERO_VAD_AMD_UPLOAD=dma: a DMA cannot expand G.711 -- such recordings take the gather kernel")
            self.how = 1
        self.stage_sync = os.environ.get("SILERO_VAD_AMD_STAGE_SYNC", "1") != "0"   # (0: A/B -- the staged copies wait on the device)

    def reserve(self, nbytes):
        """every staging slot, sized for a batch of nbytes (prepare_only)"""
        for k in range(self.pool.slots):
            self.pool.get(k, *_ingest_route(self.windowed, self.direct, self.interleaved, self.coded, nbytes, nbytes * self.src_esz // self.esz)[1])

    def host(self, k, b, since=None):
        """The host half of staging batch k: its slot, pageable sources packed into the slot's pinned staging, the wait for the slot's
        previous reader.  -> a handle, `d` its device batch [n_rows, pitch] and `slot` the slot's index.  since: where the caller's
        clock for stage_s / upload_call_s started, if before the slot was taken (the refill loop has always counted the wait for the
        slot into them, the bucket loop has not)."""
        pool = self.pool
        nbytes = b.n_rows * b.pitch * self.esz
        staged = int(b.channels.sum()) * b.pitch * self.src_esz if self.interleaved else 0
        route, (host_b, dev_b) = _ingest_route(self.windowed, self.direct, self.interleaved, self.coded, nbytes, staged)
        i = pool.get(k, host_b, dev_b)
        if route != "cut":
            STATS["h2d_bytes"] += nbytes * self.src_esz // self.esz
        STATS["buckets"] += 1
        h = types.SimpleNamespace(slot=i, route=route, nbytes=nbytes, host=None, at=None,
                                  d=pool.dev[i][:nbytes].view(self.dtype).view(b.n_rows, b.pitch))
        # The slot's previous reader is done before anything is written: the cuts and the gather kernels wait for it on the stream.  A
        # DMA -- the staged copy, the per-row copies -- issued behind an OPEN device-side wait leaves the copy engines' fast path (the
        # refill window feed's finding, profiles/r06_refill_window_feed.md); the reader of this slot's previous batch started a few
        # batches ago and is normally done by the time this one is staged, so it is waited for on the HOST, behind the staging, and the
        # copy is issued without a dependency.
        late_wait = None
        if pool.consumed[i] is not None:
            if route == "cut" or (route == "pinned" and self.how != 0) or not self.stage_sync:
                pool.stream.wait_event(pool.consumed[i])
            else:
                late_wait = pool.consumed[i]
        h.t0 = time.perf_counter() if since is None else since
        if host_b:
            h.host = pool.host[i][:host_b]
            if route == "sources":
                h.at = _stage_sources(b.ptr, b.lens, b.channels, b.pitch, self.src_esz, h.host)
            else:
                h.host = h.host.view(self.src_dtype).view(b.n_rows, b.pitch)
                _pack_rows(b.ptr, b.lens, b.pitch, self.src_esz, h.host.data_ptr())
            STATS["stage_s"] += time.perf_counter() - h.t0
        if late_wait is not None:
            late_wait.synchronize()
        return h

    def device(self, h, b):
        """The device half: batch b into h.d -- enqueued on the current stream, the staging pool's."""
        if h.route == "cut":
            self._upload(b, b.ptr, 2, h.d)                # (2: the sources are device addresses)
        elif h.route == "pinned":
            self._upload(b, b.ptr, self.how, h.d)
        elif h.route == "copy":
            h.d.copy_(h.host, non_blocking=True)
            return
        else:
            # the staged bytes cross the link in one copy, into the slot's device block behind the batch; the expansion / the split
            # reads them there, the codes with the recordings' TRUE lengths (the staging's zero bytes are not audio)
            block = self.pool.dev[h.slot][h.nbytes:h.nbytes + h.host.numel()]
            block.view(h.host.shape).copy_(h.host, non_blocking=True)
            at = h.at if h.route == "sources" else np.arange(b.n_rows, dtype=np.int64) * b.pitch
            self._upload(b, block.data_ptr() + at, 2, h.d)
            return
        STATS["upload_call_s"] += time.perf_counter() - h.t0

    def _upload(self, b, ptr, how, d):
        """vad_upload_rows; vad_upload_rows_coded when the rows carry codecs (d is then int16); vad_upload_rows_channels when the
        sources are interleaved"""
        ptr = np.ascontiguousarray(ptr, dtype=np.uint64)
        rows_p, lens_p = ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)), b.lens.ctypes.data_as(ctypes.POINTER(ctypes.c_long))
        if b.channels is not None:
            self.engine.upload_rows_channels(rows_p, lens_p, b.codecs, b.channels, b.rows_of, len(b.channels), b.n_rows, b.pitch, d, how)
        elif b.codecs is not None:
            self.engine.upload_rows_coded(rows_p, lens_p, b.codecs, b.n_rows, b.pitch, d, how)
        else:
            self.engine.upload_rows(rows_p, lens_p, b.n_rows, b.pitch, self.esz, d, how)


class _Sources:
    """The recordings of one call as flat arrays: host address and length of each, made contiguous / of one dtype once,
    and whether ALL of them sit in page-locked memory (then no host-side copy is needed at all)."""

    def __init__(self, audios, dtype, check_pinned):
        n = len(audios)
        if isinstance(audios, PackedRecordings):
            if audios.base.dtype != dtype:
                raise TypeError("mixed int16 / float recordings in one call")
            self.keep = [audios.base]
            self.len = audios.lengths
            self.ptr = (audios.base.data_ptr() + audios.offsets * audios.base.element_size()).astype(np.uint64)
            self.ptr[self.len == 0] = 0
            self.pinned = bool(check_pinned and n > 0 and audios.base.is_pinned())
            return
        self.keep = []
        self.ptr = np.zeros(n, dtype=np.uint64)
        self.len = np.zeros(n, dtype=np.int64)
        pinned_storage = {}
        all_pinned = check_pinned and n > 0
        for i, a in enumerate(audios):
            a = a if torch.is_tensor(a) else torch.as_tensor(a)
            if a.dim() != 1:
                raise ValueError("More than one dimension in audio. Are you trying to process audio with 2 channels?")
            if _sample_kind(a.dtype) != _sample_kind(dtype):
                # (an int16 recording among float ones would be read as floats in [-32768, 32767]: never silently)
                raise TypeError("mixed int16 / float recordings in one call" if torch.uint8 not in (a.dtype, dtype) else _MIXED_U8)
            if a.dtype != dtype or not a.is_contiguous() or a.is_cuda:
                a = a.to("cpu", dtype).contiguous()      # (a strided view of int16 PCM lands here: same dtype, new layout)
            self.keep.append(a)
            self.ptr[i] = a.data_ptr() if a.numel() else 0
            self.len[i] = a.shape[0]
            if all_pinned and a.numel():
                key = a.untyped_storage().data_ptr()
                if key not in pinned_storage:
                    pinned_storage[key] = bool(a.is_pinned())
                all_pinned = pinned_storage[key]
        self.pinned = bool(all_pinned)

    def tables(self, idxs):
        rows = np.ascontiguousarray(self.ptr[idxs])
        lens = np.ascontiguousarray(self.len[idxs])
        return (rows, lens, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)),
                lens.ctypes.data_as(ctypes.POINTER(ctypes.c_long)))


def _resampled_len(L, rs):
    """samples of a recording of L raw samples behind the resampler (rs = (O, N) of _source_rate, or None: no resampler)"""
    return L if rs is None else (L * rs[1] + rs[0] - 1) // rs[0]


def _resample_input(audios, codec, channels, model, source_rate, sampling_rate, fan=None):
    """`source_rate=` resolved, once, where a corpus call opens: -> (audios, codec, channels, rs).  rs = (O, N) and the recordings as
    handed over for a model whose engine resamples on the device (Engine.resample_rows); for any other (a CPU stand-in) the recordings
    come back RESAMPLED on the host -- `channels=` and `codec=` resolved first, then `resample`: float32 at the net's rate, rs None --,
    the definition of what the device route computes."""
    rs = _source_rate(source_rate, sampling_rate)
    if rs is None or hasattr(getattr(model, "engine", None), "resample_rows"):
        return audios, codec, channels, rs
    assert fan is None                                    # (a stand-in never gets interleaved recordings: _channel_input)
    recs, cd = _coded_input(*_channel_input(audios, codec, channels, model)[:2], model)
    return [torch.from_numpy(resample(a, source_rate, sampling_rate)) for a in recs], None, None, None


def _lane_resampled_bytes(rows, width):
    return rows * ((width + 3) // 4 * 4) * 4


def _lane_resampled(lane_model, rows, width):
    """[rows, width] float32 of the lane's buffer of resampled audio, rows 16-byte aligned (the frontend's vector loads); made on the
    current stream, the lane's, which alone uses it: bucket k + lanes resamples into it behind bucket k's kernels in stream order."""
    need = _lane_resampled_bytes(rows, width)
    buf = getattr(lane_model, "_resample_buf", None)
    if buf is None or buf.numel() < need:
        buf = lane_model._resample_buf = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=lane_model.device)
        STATS["resample_allocs"] += 1
    return buf[:need].view(torch.float32).view(rows, -1)[:, :width]


def _upload_mode():
    """How pinned recordings reach the GPU: "window" (a PackedRecordings whose recordings lie back to back: one DMA per arena
    window, batches cut on the device; the default where it applies), "gather" (one kernel that reads host memory; the default
    otherwise), "dma" (copy engines, one copy per row), "stage" (force the pageable path).  SILERO_VAD_AMD_UPLOAD overrides."""
    return os.environ.get("SILERO_VAD_AMD_UPLOAD", "")


def ragged_buckets(audios: Sequence, model, sampling_rate: int = 16000, max_waste: float = 0.15,
                   max_bytes: int = 256 << 20, plan: RaggedPlan = None, post=None, meta=None, lanes: int = 2, prepare_only: bool = False,
                   codec=None, channels=None, _fan=None, post_batch: bool = False, source_rate=None):
    """Generator over the plan's buckets: yields (indices, probs[len(indices), T_bucket] on the CPU).
    Recording i of a bucket owns the first ceil(len_i / N) entries of its row.

    `post` (GPU models only): a function (probs_dev, indices, meta_dev) -> list of device tensors that is enqueued
    right after the bucket's kernels; the generator then yields (indices, [those tensors on the CPU], probs_dev) and
    the probabilities themselves never leave the GPU (ragged_speech_segments scans them there).  `meta` (indices ->
    small CPU int64 tensor) rides to the GPU with the bucket's PCM on the copy stream (pinned, asynchronous), so that
    nothing in the loop blocks the host on the compute stream.  `post_batch`: `post` is called as (probs_dev, indices, meta_dev, x)
    with x the bucket's batch [len(indices), L] as the kernels read it (int16 or float32, raw rate; its rows keep the staging slot's
    pitch) -- valid only for the work `post` enqueues: the slot is handed to a later bucket once that work is done (the slot's
    `consumed` event is recorded behind `post`).  `lanes`: buckets are issued round-robin to this many
    engines on their own streams (_compute_lanes); results are yielded in bucket order.  `prepare_only`: plan the run, create the lanes
    and their streams, size every lane's scratch and the staging slots for the plan's largest bucket -- everything that allocates --
    and stop (ragged_reserve): a run over the same recordings then allocates nothing.

    Ingest: recordings in pinned host memory go straight to the device batch (vad_upload_rows: no host copy);
    pageable ones are packed into pinned staging by the native threaded copy and copied from there.

    `codec` ("ulaw" / "alaw", or one per recording): the recordings are uint8 G.711 codes.  They take the same routes at ONE byte a
    sample -- the arena windows' DMAs, the gather over PCIe, the staging buffers carry the codes -- and the gather kernel expands them
    into the int16 batch (vad_upload_rows_coded); the buckets are planned on the batch's bytes, so the call forms the buckets of its
    int16 twin and every result is that of the same call on the `g711_expand`ed recordings.

    `channels` (1 or 2, or one per recording; with `codec` or with int16 recordings): a recording is INTERLEAVED, as a WAV data chunk
    holds a recorded call, and every channel is a stream of its own.  The interleaved bytes take the same routes, once -- the windows'
    DMAs, the gather over PCIe, the staging buffers carry them as they are -- and the gather kernel writes one batch row per channel
    (vad_upload_rows_channels).  Buckets are planned on the batch rows, a recording's channels in one bucket; every result is that of
    the same call on the flat list [deinterleave(a_i, C_i, c) for i for c in range(C_i)], and the indices yielded are indices into
    that list (channel_rows).

    `source_rate` (44100, 22050, 24000, 11025, ...: resample_geometry): the recordings are at THAT rate and `sampling_rate` is the net's,
    8000 or 16000 -- what a reference user gets from read_audio(path, sampling_rate), channel averaging apart.  Planning and ingest are
    untouched: lengths, buckets, windows, staging and every ingest route count RAW samples, the raw bytes cross the link once, `codec`
    and `channels` compose.  Per bucket ONE resample (vad_resample_rows_device) is enqueued on the lane's stream in front of the
    kernels, from the batch the ingest wrote into the lane's float32 buffer (sized by ragged_reserve); recording i then owns the first
    ceil(ceil(N len_i / O) / chunk) entries of its row, and the x a `post_batch` post sees is the RESAMPLED batch.  Every result is
    that of the same call on [resample(a) for a in audios] up to the kernel's fp32 rounding (resample_device).  A model without the
    device route (a CPU stand-in) gets the recordings resampled on the host by `resample`: exactly that call.
    NOT `sampling_rate=48000`: that is the reference's x[::3] inside the model, no low-pass; `source_rate=48000` is read_audio's
    low-pass resample.  Both exist in the reference."""
    t_setup = time.perf_counter()
    audios, codec, channels, rs = _resample_input(audios, codec, channels, model, source_rate, sampling_rate, _fan)
    n = _rates(sampling_rate)[2]                          # input samples per chunk (512 k for a multiple of 16 kHz)
    inp = _corpus_input(audios, model, codec, channels, _fan)
    audios, lengths, cd, fan = inp.recs, inp.lengths, inp.cd, inp.fan
    dtype, esz, src_dtype, src_esz = inp.dtype, inp.esz, inp.src_dtype, inp.src_esz
    fast = model.audio_forward_device
    dev = getattr(model, "device", None)
    on_gpu = dev is not None and torch.device(dev).type == "cuda"
    mode = _upload_mode()
    lane_list = pool = cur = None
    if on_gpu:                                            # (before the plan: the first windows' DMA starts while the buckets are planned)
        lane_list = _compute_lanes(model, max(1, int(lanes)))
        pool = getattr(model, "_stage_pool", None)
        if pool is None or pool.slots != len(lane_list) + 1:
            pool = model._stage_pool = _StagePool(dev, len(lane_list) + 1)
            # the upload stream beside every compute lane, not in front of one of them
            pool.stream = _distinct_queue_stream(getattr(model, "engine", None), dev, [st for _, st in lane_list])
        cur = torch.cuda.current_stream(dev)
    copies = []                                           # (start event, end event) of every H2D copy, for STATS
    # One large H2D DMA per arena window (copy engines: no CU time, no host time, exactly the live bytes), two windows
    # ahead of the kernels; the padded [rows][pitch] batches are then cut out of the window's device copy at HBM speed.
    win = {"buf": [None, None, None], "free": [None, None, None], "ev": {}, "next": 0, "span": [], "base": None, "stream": None}

    def ensure_window(w):
        while win["next"] <= w and win["next"] < len(win["span"]):
            v = win["next"]
            a, b = win["span"][v]
            j = v % 3
            nb = (b - a) * src_esz
            if win["buf"][j] is None or win["buf"][j].numel() < nb:
                # (the old block goes back to the caching allocator: its cuts on pool.stream were recorded against it
                #  -- record_stream below -- and the copy stream waits for the last of them before anything else)
                if win["free"][j] is not None:
                    win["stream"].wait_event(win["free"][j])
                with torch.cuda.stream(win["stream"]):
                    win["buf"][j] = torch.empty(max(nb, 1 << 20), dtype=torch.uint8, device=dev)
                win["buf"][j].record_stream(pool.stream)  # allocated on the copy stream, read by the cut kernels on pool.stream
                win["free"][j] = None
            if win["free"][j] is not None:                # every bucket cut from the buffer's previous window is done
                win["stream"].wait_event(win["free"][j])
            with torch.cuda.stream(win["stream"]):
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record(win["stream"])
                win["buf"][j][:nb].view(src_dtype).copy_(win["base"][a:b], non_blocking=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record(win["stream"])
            copies.append((e0, e1))
            STATS["h2d_bytes"] += nb
            win["ev"][v] = e1
            win["next"] += 1

    if plan is None and on_gpu and mode in ("", "window") and hasattr(getattr(model, "engine", None), "upload_rows"):
        # recordings that lie in ONE pinned host buffer (a PackedRecordings, or a list of views of one pinned tensor) and cover
        # most of the range they span: one DMA per arena window, batches cut on the device
        packed = audios if isinstance(audios, PackedRecordings) else _as_packed(audios)
        if packed is not None and packed.base.is_pinned():
            wbytes = int(os.environ.get("SILERO_VAD_AMD_WINDOW_BYTES", 0)) or max(2 * max_bytes, 1 << 30)

            def takes_windows(wp_):
                return mode == "window" or (wp_.density >= 0.6 and wp_.mean_window_fill() >= 16)

            def first_windows(wp_):
                # the windows are known, the buckets are not yet: the first three windows' copies start NOW, the bucket planning (tens
                # of ms for a corpus shard) runs beside them
                if prepare_only or not takes_windows(wp_):
                    return
                win["span"], win["base"] = wp_.span, packed.base
                win["stream"] = _copy_stream(pool, model, dev, [st for _, st in lane_list] + [pool.stream])
                win["stream"].wait_stream(cur)            # (the arena was written before this call in stream order, if at all)
                ensure_window(2)

            wp = WindowedPlan(packed, max_waste, max_bytes, esz, window_bytes=wbytes, on_windows=first_windows, src_itemsize=src_esz, fan=fan)
            if takes_windows(wp):
                plan, audios = wp, packed
    plan = plan or RaggedPlan(lengths, max_waste, max_bytes, esz, None if fan is None else fan.mate)
    ing = _Ingest(inp, audios, pool, getattr(model, "engine", None), on_gpu)      # (after the plan: the window route reads the arena)
    src = ing.src
    if not on_gpu:                                        # CPU stand-in models (tests)
        assert fan is None                                # (they were handed the de-interleaved recordings: _channel_input)
        if prepare_only:
            return
        for idxs in plan.buckets:
            width = max(plan.lengths[idxs[0]], n)
            host = torch.empty((len(idxs), width), dtype=dtype)
            _pack_rows(src.ptr[idxs], src.len[idxs], width, host.element_size(), host.data_ptr())
            yield idxs, fast(host, sampling_rate).cpu()
        return
    windowed = ing.windowed = ing.direct and isinstance(plan, WindowedPlan)

    if windowed:
        if win["stream"] is None:                          # (a plan handed in by the caller, or prepare_only: nothing was started early)
            win["span"], win["base"] = plan.span, audios.base
            win["stream"] = _copy_stream(pool, model, dev, [st for _, st in lane_list] + [pool.stream])
        last_bucket_of = {}
        for k, w in enumerate(plan.window_of):
            last_bucket_of[w] = k
    align = 16 // esz                                      # device rows are 16-byte aligned: the kernels' vector loads
    # every lane's scratch is sized up front for the largest bucket it can meet: a growth inside the loop would
    # synchronise the device and stall all lanes (vad_reserve)
    if plan.buckets and hasattr(getattr(model, "engine", None), "reserve"):
        shapes = [(len(b), (max(_resampled_len(plan.lengths[b[0]], rs), n) + n - 1) // n) for b in plan.buckets]
        big = max(shapes, key=lambda bt: ((bt[0] + 15) // 16) * bt[1])
        wide = max(shapes, key=lambda bt: bt[0])
        t_res = time.perf_counter()
        for lane_model, _ in lane_list:
            for bt in {big, wide}:
                lane_model.engine.reserve(sampling_rate, bt[0], bt[1])
        STATS["reserve_s"] += time.perf_counter() - t_res
    if rs is not None and plan.buckets:
        # the pair's table onto the device, and every lane's float32 buffer for the largest resampled bucket it can meet
        rs_bytes = max(_lane_resampled_bytes(len(b), max(_resampled_len(plan.lengths[b[0]], rs), n)) for b in plan.buckets)
        for lane_model, lane_stream in lane_list:
            lane_model.engine.resample_reserve(source_rate, sampling_rate)
            with torch.cuda.stream(lane_stream):
                _lane_resampled(lane_model, 1, rs_bytes // 4)
    if prepare_only:
        if plan.buckets:
            big_b = max(plan.buckets, key=lambda b: len(b) * ((max(plan.lengths[b[0]], n) + align - 1) // align * align))
            nb = len(big_b) * ((max(plan.lengths[big_b[0]], n) + align - 1) // align * align) * esz
            ing.reserve(nb)
            if windowed:                                   # the three window buffers: warm torch's allocator with blocks of the largest window
                wb = max((b - a) * src_esz for a, b in plan.span)
                with torch.cuda.stream(win["stream"]):
                    warm = [torch.empty(max(wb, 1 << 20), dtype=torch.uint8, device=dev) for _ in range(3)]
                del warm
        torch.cuda.synchronize(dev)
        return
    for _, st in lane_list[1:]:
        st.wait_stream(cur)                               # sibling lanes start behind whatever the caller has queued
    # Buckets on different lanes overlap because a bucket's recurrence sits on the few CUs its stream tiles need (16 streams per CU,
    # kernel_rec.hip) beside the other lane's frontend.  The matrix-vector form of the recurrence (kernel_rec_small.hip) finishes a
    # bucket of a few hundred recordings 2-3 x sooner but spreads it over the whole chip, with nothing left to overlap with: the
    # pipelined corpus runs 4 % (window route) to 30 % (gather kernel) slower with it.  Lanes therefore pin the MFMA form.
    lane_form = os.environ.get("SILERO_VAD_AMD_LANE_REC", "mfma")     # (A/B: "auto" lets the lanes take the matrix-vector form)
    lane_engines = []
    if len(lane_list) > 1 and lane_form != "auto":
        lane_engines = [e for e in (getattr(m, "engine", None) for m, _ in lane_list) if e is not None and hasattr(e, "set_transient")]
    pinned = {}                                            # engine -> the value it had when the pin was applied

    def pin_lanes(on):
        """The pin holds only while this generator runs: it is taken back before every `yield` (the caller's own engine is lane 0;
        a consumer that never exhausts the generator must not be left with the slower form) and re-applied on resumption.  The
        value to restore is sampled EVERY time the pin goes on (the consumer may have changed the option between two yields), and
        it is restored only if the option still holds the pinned value (a change made while pinned is the consumer's and stays)."""
        for eng_l in lane_engines:
            if on:
                pinned[id(eng_l)] = eng_l.options.get("rec_form", "auto")
                eng_l.set_transient("rec_form", lane_form)
            elif id(eng_l) in pinned:
                before = pinned.pop(id(eng_l))
                if eng_l.options.get("rec_form", "auto") == before:      # (set_transient does not touch .options)
                    eng_l.set_transient("rec_form", before)

    pin_lanes(True)

    def stage(k):
        idxs = plan.buckets[k]
        # at least one full window: audio_forward rejects shorter inputs (vad_annotator.py:124)
        L = max(plan.lengths[idxs[0]], n)
        width = (L + align - 1) // align * align          # row pitch
        from_, lens, ch_k, rows_of = idxs, src.len, None, None
        if fan is not None:
            # the bucket's sources: one per recording, both channels wanted (a bucket does not end between them: _bucket_cuts)
            from_, _, _, rows_of = fan.table(idxs)
            lens, ch_k = fan.frames, fan.C[from_]
        # (a windowed bucket's sources are device addresses, known once its window is on its way: below)
        b = _Batch(None if windowed else src.ptr[from_], lens[from_], None if cd is None else cd[from_], ch_k, rows_of, len(idxs), width)
        STATS["padded"] += len(idxs) * L
        STATS["real"] += sum(plan.lengths[j] for j in idxs)
        mt = meta(idxs) if meta is not None else None
        h = ing.host(k, b)
        i, d = h.slot, h.d
        if windowed:
            w = plan.window_of[k]
            ensure_window(w + 2)                          # this bucket's window and the two after it are on their way
            pool.stream.wait_event(win["ev"][w])
            b.ptr = np.ascontiguousarray(win["buf"][w % 3].data_ptr() + (audios.offsets[from_] - plan.span[w][0]) * src_esz, dtype=np.uint64)
        with torch.cuda.stream(pool.stream):
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record(pool.stream)
            ing.device(h, b)
            if windowed and last_bucket_of[w] == k:       # the window's buffer may take another window once this cut is done
                win["free"][w % 3] = torch.cuda.Event()
                win["free"][w % 3].record(pool.stream)
            m_dev = m_host = l_dev = None
            mt_n = mt.numel() if mt is not None else 0
            if mt is not None or rs is not None:          # through the slot's own pinned scratch (meta_buffer: why)
                scratch = pool.meta_buffer(i, mt_n + (len(idxs) if rs is not None else 0))
            if mt is not None:
                m_host = scratch[:mt_n].view(mt.shape)
                m_host.copy_(mt)
                m_dev = m_host.to(dev, non_blocking=True)
            if rs is not None:                            # the rows' live lengths, raw samples: where the resampler ends each row
                l_host = scratch[mt_n:]
                l_host.copy_(torch.as_tensor([plan.lengths[j] for j in idxs], dtype=torch.int64))
                l_dev = l_host.to(dev, non_blocking=True)
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(pool.stream)
        if not windowed:
            copies.append((ev0, ev))
        pool.done[i] = ev
        return d[:, :L], ev, i, m_dev, m_host, l_dev

    def finish(done_bucket):
        idxs, outs, _, probs_dev = done_bucket
        if post is None:
            return idxs, outs[0]
        return idxs, outs, probs_dev

    STATS["setup_s"] += time.perf_counter() - t_setup
    try:
        staged = stage(0) if plan.buckets else None
        inflight = []                                     # buckets enqueued and not yet yielded, oldest first
        for k, idxs in enumerate(plan.buckets):
            x, ev, slot, m_dev, _keep, l_dev = staged
            lane_model, lane_stream = lane_list[k % len(lane_list)]
            lane_stream.wait_event(ev)
            with torch.cuda.stream(lane_stream):
                x.record_stream(lane_stream)              # allocated on pool.stream, read on the lane's stream
                if m_dev is not None:
                    m_dev.record_stream(lane_stream)
                if rs is not None:                        # the raw batch -> the lane's float32 buffer at the net's rate
                    l_dev.record_stream(lane_stream)
                    raw, x = x, _lane_resampled(lane_model, len(idxs), max(_resampled_len(plan.lengths[idxs[0]], rs), n))
                    lane_model.engine.resample_rows(source_rate, sampling_rate, raw, l_dev, x.shape[1], x)
                probs = lane_model.audio_forward_device(x, sampling_rate)   # asynchronous
                back = [probs] if post is None else post(probs, idxs, m_dev, x) if post_batch else post(probs, idxs, m_dev)
                pool.consumed[slot] = torch.cuda.Event()      # (behind post: with post_batch it reads x)
                pool.consumed[slot].record(lane_stream)
                outs = []
                for o in back:                            # pinned blocks come from torch's caching host allocator
                    h = torch.empty(o.shape, dtype=o.dtype, pin_memory=True)
                    h.copy_(o, non_blocking=True)
                    STATS["d2h_bytes"] += h.numel() * h.element_size()
                    outs.append(h)
                done = torch.cuda.Event()
                done.record(lane_stream)
            staged = stage(k + 1) if k + 1 < len(plan.buckets) else None   # the next bucket is on its way meanwhile
            inflight.append((idxs, outs, done, probs))
            while len(inflight) > len(lane_list):
                first = inflight.pop(0)
                t_w = time.perf_counter()
                first[2].synchronize()
                STATS["result_wait_s"] += time.perf_counter() - t_w
                pin_lanes(False)
                yield finish(first)
                pin_lanes(True)
        for first in inflight:
            t_w = time.perf_counter()
            first[2].synchronize()
            STATS["result_wait_s"] += time.perf_counter() - t_w
            pin_lanes(False)
            yield finish(first)
            pin_lanes(True)
    finally:
        pin_lanes(False)
        # also when the consumer stops early or an exception propagates: the sibling lanes' work is ordered before
        # whatever the caller enqueues next, and the copy events are drained
        for _, st in lane_list[1:]:
            cur.wait_stream(st)
        cur.wait_stream(pool.stream)
        if windowed:                                      # cuts still pending on pool.stream read the window buffers: the copy
            win["stream"].wait_stream(pool.stream)        # stream (where they were allocated and will be freed) falls in behind them
            cur.wait_stream(win["stream"])
        for a, b in copies:
            b.synchronize()
            STATS["h2d_s"] += a.elapsed_time(b) / 1e3


def ragged_reserve(audios: Sequence, model, sampling_rate: int = 16000, max_waste: float = 0.15, max_bytes: int = 256 << 20,
                   lanes: int = 2, codec=None, channels=None, source_rate=None):
    """Everything a `ragged_probs` / `ragged_speech_segments` run over these recordings would allocate -- the compute lanes and their
    streams, every lane's scratch (vad_reserve: a later growth synchronises the device and, on some boxes, costs 0.1-0.2 s of
    hipFree / hipMalloc for the multi-GB gx scratch: profiles/r05_ingest_routes.md), the staging slots -- sized for the plan's
    largest bucket, up front.  Call it once before a corpus run (or a timed region); the run itself then allocates nothing.  With
    `source_rate` (ragged_buckets) also the pair's resampling table and every lane's buffer of resampled audio."""
    for _ in ragged_buckets(audios, model, sampling_rate, max_waste, max_bytes, lanes=lanes, prepare_only=True, codec=codec, channels=channels,
                            source_rate=source_rate):
        pass


def ragged_probs(audios: Sequence, model, sampling_rate: int = 16000, max_waste: float = 0.15,
                 max_bytes: int = 256 << 20, plan: RaggedPlan = None, codec=None, channels=None, source_rate=None) -> List[torch.Tensor]:
    """Speech probabilities of many recordings of different lengths.

    Returns one 1-D CPU float tensor per recording (ceil(len / N) entries), bit-identical to
    ``model.audio_forward(audio[None], sr)[0]`` on that recording alone.  ``audios`` may be float
    tensors in [-1, 1] or int16 PCM (all of one kind).  `model` needs ``audio_forward_device``
    (HipSileroVAD); staging + H2D of bucket k+1 overlap the kernels of bucket k.  `sampling_rate` may be a multiple of 16000: the
    recordings then stay at their raw rate all the way into HBM (_rates).  `codec` ("ulaw" / "alaw", or one per recording): the
    recordings are uint8 G.711 codes and cross the link as such (ragged_buckets); the result is that of the `g711_expand`ed recordings.
    `channels` (1 or 2, or one per recording): the recordings are interleaved and split on the device (ragged_buckets); the result has
    one entry per (recording, channel), recording-major (channel_rows) -- that of the call on the `deinterleave`d recordings.
    `source_rate`: the recordings are at that rate and are resampled to `sampling_rate`, the net's, on the device (ragged_buckets: what
    read_audio(path, sampling_rate) gives a reference user); recording i has ceil(ceil(N len_i / O) / chunk) probabilities, bit-identical
    to ``model.audio_forward(resample_device(engine, audio_on_the_gpu, None, source_rate, sampling_rate)[None], sampling_rate)[0]``."""
    audios, codec, channels, rs = _resample_input(audios, codec, channels, model, source_rate, sampling_rate)
    n = _rates(sampling_rate)[2]
    audios, codec, fan = _channel_input(audios, codec, channels, model)
    lengths = [_resampled_len(m, rs) for m in _describe(audios if fan is None else fan)[1]]
    out: List[torch.Tensor] = [torch.empty(0)] * len(lengths)
    for idxs, probs in ragged_buckets(audios, model, sampling_rate, max_waste, max_bytes, plan, codec=codec, _fan=fan,
                                      source_rate=source_rate if rs else None):
        for row, i in enumerate(idxs):
            out[i] = probs[row, : (lengths[i] + n - 1) // n].clone()
    return out


def ragged_speech_segments(audios: Sequence, model, sampling_rate: int = 16000, max_waste: float = 0.15,
                           max_bytes: int = 256 << 20, threads: int = 0, device_scan: bool = None,
                           as_arrays: bool = False, codec=None, channels=None, source_rate=None, **scan_kw) -> List[list]:
    """Speech segments (sample indices) of many recordings: bucketed GPU batches, then the segmenter.
    scan_kw: the threshold/duration arguments of get_speech_timestamps.  codec / channels: as in ragged_probs (uint8 G.711 recordings;
    interleaved recordings, one result per channel).  `audios`: a list of 1-D tensors or a
    PackedRecordings.  as_arrays: return (counts int64[n], segments int64[sum(counts), 2]) -- recording i owns rows
    cumsum(counts)[i-1] .. -- instead of a list of lists of dicts (for corpora of 10^5+ recordings the dicts cost more
    host time than the GPU work; the arrays are also what a host-side gather to rank 0 wants).

    device_scan (default: on for a GPU model backed by the native engine): the scan runs on the GPU right behind the
    kernels of its bucket (vad_segment_probs_device, one lane per recording) and only counts + segment lists come
    back over PCIe; otherwise the probabilities are copied to the host and scanned by the native threaded scanner.
    Both give the same segments (one source, csrc/scanner.hpp).  `sampling_rate` may be a multiple of 16000 (raw recordings, _rates):
    the segments are then in samples of the 16 kHz signal x[::k], as the reference's scan sees it (utils_vad.py:301-307).
    `source_rate`: the recordings are at that rate and are resampled to `sampling_rate` on the device (ragged_buckets); the segments are
    in samples of the RESAMPLED signal, clipped to its length ceil(N len / O) -- what get_speech_timestamps gives on read_audio's
    output."""
    return _speech_segments(audios, model, sampling_rate, max_waste, max_bytes, threads, device_scan, as_arrays, codec, channels, None, scan_kw,
                            source_rate)


def _speech_segments(audios, model, sampling_rate, max_waste, max_bytes, threads, device_scan, as_arrays, codec, channels, collector, scan_kw,
                     source_rate=None):
    """ragged_speech_segments; with a `collector` (_AudioCollector: ragged_speech_audio) every bucket's gather is enqueued behind its
    scan and the collector is told each bucket's final segment table.  Without one, the calls are those of ragged_speech_segments."""
    audios, codec, channels, rs = _resample_input(audios, codec, channels, model, source_rate, sampling_rate)
    net_sr, dec, n = _rates(sampling_rate)
    audios, codec, fan = _channel_input(audios, codec, channels, model)
    lengths = [_resampled_len(m, rs) for m in _describe(audios if fan is None else fan)[1]]      # (of what the net and the scan see)
    source_rate = source_rate if rs else None
    dev = getattr(model, "device", None)
    on_gpu = dev is not None and torch.device(dev).type == "cuda"
    if device_scan is None:
        device_scan = on_gpu and hasattr(getattr(model, "engine", None), "_h")
    counts_all = np.zeros(len(lengths), dtype=np.int64)
    parts = []                                                 # (indices, counts, segs[rows, cap, 2]) per bucket
    if device_scan:
        params = _segment_params(net_sr, **scan_kw)
        cap0 = 24                                              # segments per recording copied back optimistically
        lens_t = torch.as_tensor(lengths, dtype=torch.int64)

        def meta(idxs):                                        # [2, n]: chunks and (16 kHz) samples of each recording of the bucket
            lens = lens_t[idxs]
            return torch.stack([(lens + n - 1) // n, (lens + dec - 1) // dec])

        def post(probs_dev, idxs, both, x=None):
            counts, segs = _device_scan(model.engine, probs_dev, both[0], both[1], params, cap0)
            if collector is None:
                return [counts, segs]
            return [counts, segs] + collector.enqueue(x, both[1], counts, segs)

        if collector is not None:
            collector.open(audios, _codec_of(audios, codec) if fan is None else fan.cd, fan, lengths)
        for idxs, outs, probs_dev in ragged_buckets(audios, model, sampling_rate, max_waste, max_bytes, post=post, meta=meta,
                                                    codec=codec, _fan=fan, post_batch=collector is not None, source_rate=source_rate):
            counts, segs = outs[0], outs[1]
            t0 = time.perf_counter()
            cnt = counts.numpy()
            if len(cnt) and int(cnt.max()) > cap0:             # rare: rescan this bucket with room for all
                both = meta(idxs).to(probs_dev.device)
                c2, s2 = _device_scan(model.engine, probs_dev, both[0], both[1], params, int(cnt.max()))
                cnt, segs = c2.cpu().numpy(), s2.cpu()
            parts.append((np.asarray(idxs, dtype=np.int64), cnt.copy(), segs.numpy()))
            STATS["scan_s"] += time.perf_counter() - t0
            if collector is not None:
                collector.bucket(idxs, parts[-1][1], parts[-1][2], outs[2], outs[3])
    else:
        if collector is not None:
            raise RuntimeError("ragged_speech_audio collects on the device, behind the device scan: it needs a GPU model backed by the "
                               "native engine (and device_scan left on); there is no host route")
        for idxs, probs in ragged_buckets(audios, model, sampling_rate, max_waste, max_bytes, codec=codec, _fan=fan, source_rate=source_rate):
            lens = [lengths[i] for i in idxs]
            t0 = time.perf_counter()
            segs = segment_probs_batch(probs, [(m + n - 1) // n for m in lens], [(m + dec - 1) // dec for m in lens], net_sr,
                                       threads=threads, **scan_kw)
            cnt = np.asarray([len(sg) for sg in segs], dtype=np.int64)
            arr = np.zeros((len(segs), max(1, int(cnt.max()) if len(cnt) else 1), 2), dtype=np.int64)
            for r, sg in enumerate(segs):
                for k, d in enumerate(sg):
                    arr[r, k] = (d["start"], d["end"])
            parts.append((np.asarray(idxs, dtype=np.int64), cnt, arr))
            STATS["scan_s"] += time.perf_counter() - t0
    t0 = time.perf_counter()
    for idxs, cnt, _ in parts:
        counts_all[idxs] = cnt
    first = np.concatenate([[0], np.cumsum(counts_all)])
    flat = np.zeros((int(first[-1]), 2), dtype=np.int64)
    for idxs, cnt, sg in parts:                                # scatter every bucket's segments to their recording's rows
        if not len(idxs) or not cnt.any():
            continue
        k = np.arange(sg.shape[1])[None, :]
        mask = k < cnt[:, None]
        flat[(first[idxs][:, None] + k)[mask]] = sg[mask]
    STATS["scan_s"] += time.perf_counter() - t0
    if as_arrays:
        return counts_all, flat
    fl = flat.tolist()
    return [[{"start": a, "end": b} for a, b in fl[first[i]:first[i + 1]]] for i in range(len(lengths))]


def collect_chunks_device(engine, pcm_dev: torch.Tensor, segs_dev: torch.Tensor, counts_dev: torch.Tensor, audio_len_dev: torch.Tensor,
                          step: int = 1, invert: bool = False):
    """`collect_chunks` (invert: `drop_chunks`) for every row of a batch that is on the GPU beside its scan, asynchronous on the current
    stream (vad_collect_segments_device: the count phase, the offsets, the gather) -> (out_dev, offsets, kept), all on the device.

    pcm_dev[B, W]: int16 or float32 rows with unit stride inside a row, as `audio_forward_device` received them; `step` 1, 2 or 3: the
    batch holds raw 16 / 32 / 48 kHz samples, 16 kHz sample s of a row is its element s * step.  segs_dev[B, cap, 2] / counts_dev[B]:
    what the device scan wrote (cap <= 512); audio_len_dev[B]: the 16 kHz lengths the scan was given.  Row i's kept[i] samples are
    out_dev[offsets[i] : offsets[i] + kept[i]]; every offset is a multiple of 16 bytes and the elements between rows are uninitialised.
    kept[i] == -1: the row is left to the caller -- its segment list did not fit `cap` (rescan it), or, for hand-made overlapping
    segments only, it keeps more than out_dev has room for (out_dev is sized like the batch itself, which lists of disjoint segments
    cannot exceed; nothing here waits for the device to learn a size)."""
    if not (torch.is_tensor(pcm_dev) and pcm_dev.is_cuda and pcm_dev.dim() == 2 and pcm_dev.dtype in (torch.int16, torch.float32)):
        raise ValueError("pcm_dev must be a 2-D CUDA tensor of int16 or float32 samples")
    B, W = pcm_dev.shape
    if W > 1 and pcm_dev.stride(1) != 1:
        raise ValueError("pcm_dev: the samples of a row must be contiguous")
    if step not in (1, 2, 3):
        raise ValueError(f"step must be 1, 2 or 3, got {step!r}")
    dev, esz = pcm_dev.device, pcm_dev.element_size()
    if segs_dev.dim() != 3 or segs_dev.shape[0] != B or segs_dev.shape[2] != 2 or counts_dev.shape != (B,) or audio_len_dev.shape != (B,):
        raise ValueError("segs_dev[B, cap, 2], counts_dev[B] and audio_len_dev[B] need one entry per row of pcm_dev")
    for t in (segs_dev, counts_dev, audio_len_dev):
        if t.dtype != torch.int64 or t.device != dev:
            raise ValueError("segs_dev, counts_dev and audio_len_dev must be int64 tensors on pcm_dev's device")
    segs_dev, counts_dev = segs_dev.contiguous(), counts_dev.contiguous()
    per = 16 // esz                                            # elements of a 16-byte granule: every row of out starts on one
    room = (W + step - 1) // step                              # 16 kHz samples a row holds
    alen = audio_len_dev.clamp(max=room).contiguous()
    ld = pcm_dev.stride(0) if B > 1 else W
    capacity = B * ((room + per - 1) // per * per)
    out = torch.empty(capacity, dtype=pcm_dev.dtype, device=dev)
    kept = torch.empty(B, dtype=torch.int64, device=dev)
    offsets = torch.zeros(B, dtype=torch.int64, device=dev)
    if B == 0:
        return out, offsets, kept
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def phase(out_ptr):
        _lib.check(engine._h, lib().vad_collect_segments_device(
            engine._h, pcm_dev.data_ptr(), esz, ld, int(step), B, alen.data_ptr(), segs_dev.data_ptr(), segs_dev.shape[1],
            counts_dev.data_ptr(), 1 if invert else 0, kept.data_ptr(), offsets.data_ptr(), out_ptr, stream))

    phase(None)
    padded = (kept.clamp(min=0) + (per - 1)) // per * per
    ends = torch.cumsum(padded, 0)
    offsets = (ends - padded).contiguous()
    kept = torch.where(ends <= capacity, kept, torch.full_like(kept, -1)).contiguous()
    phase(out.data_ptr())
    return out, offsets, kept


class _AudioCollector:
    """ragged_speech_audio's half of the bucket loop (_speech_segments): `enqueue` puts a bucket's gather behind its scan on the lane's
    stream; `bucket` is told the bucket's final segments once the host has them (and kept[] with them) and brings the kept bytes home
    on a stream of its own -- or leaves them where they are --; rows the device left alone are collected from their recording on the
    host (vad_collect_segments)."""

    def __init__(self, model, step, invert, on_device):
        self.model, self.step, self.invert, self.on_device = model, step, invert, on_device
        self.held = collections.deque()                        # packed outputs of the buckets in flight, oldest first
        self.events = []
        self.audio = self.dtype = self.dev = None
        self.copy_stream = None

    def open(self, audios, cd, fan, lengths):
        self.audios, self.cd, self.fan, self.lengths = audios, cd, fan, lengths
        self.audio = [None] * len(lengths)

    def enqueue(self, x, audio_len_dev, counts, segs):
        out, offsets, kept = collect_chunks_device(self.model.engine, x, segs, counts, audio_len_dev, self.step, self.invert)
        self.dtype, self.dev = out.dtype, out.device
        self.held.append(out)
        return [kept, offsets]

    def _stream(self):
        """where the audio goes home: not a compute lane, and beside the lanes where the hardware queues allow it"""
        if self.copy_stream is None:
            pool = self.model._stage_pool
            st = getattr(pool, "audio_stream", None)
            if st is None:
                lanes = [s for _, s in _compute_lanes(self.model, pool.slots - 1)]
                st = pool.audio_stream = _distinct_queue_stream(getattr(self.model, "engine", None), self.dev, lanes)
            self.copy_stream = st
        return self.copy_stream

    def bucket(self, idxs, cnt, segs, kept, offsets):
        out = self.held.popleft()
        kept, offsets = kept.numpy(), offsets.numpy()
        live = kept > 0
        total = int((offsets[live] + kept[live]).max()) if live.any() else 0
        esz = out.element_size()
        STATS["collect_bytes"] += int(kept[live].sum()) * esz
        if self.on_device:
            buf = out[:total]
            out.record_stream(torch.cuda.current_stream(self.dev))      # (allocated on a lane's stream, read by the caller's)
        else:
            buf = torch.empty(total, dtype=out.dtype, pin_memory=True)
            if total:
                # the bucket is done (the loop waited for it): nothing to wait for on the device, the copy overlaps the later buckets
                st = self._stream()
                with torch.cuda.stream(st):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    buf.copy_(out[:total], non_blocking=True)
                    e1.record(st)
                out.record_stream(st)
                self.events.append((e0, e1))
                if AUDIO_TRACE is not None:
                    AUDIO_TRACE.append((e0, e1, total * esz))
                STATS["audio_d2h_bytes"] += total * esz
        # every row's view in ONE call (a slice per row costs more host time than a bucket's gather costs the device): the cuts are
        # each row's first and one-past-last element, so the odd pieces are the rows and the even ones the padding between them
        cuts = np.stack([offsets, offsets + np.maximum(kept, 0)], axis=1).reshape(-1)
        cuts = np.minimum(np.maximum.accumulate(cuts), total)  # (rows the device left alone own nothing of buf)
        views = torch.tensor_split(buf, cuts.tolist())[1::2]
        for r, i in enumerate(idxs):
            self.audio[i] = views[r] if kept[r] >= 0 else self._on_host(i, segs[r, :int(cnt[r])])

    def _on_host(self, i, segs):
        """row i from its recording: the twin's raw-rate samples (g711_expand / deinterleave), every step-th of them inside the segments"""
        STATS["collect_host_rows"] += 1
        rec, ch, C = (i, 0, 1) if self.fan is None else (int(self.fan.rec_of[i]), int(self.fan.ch_of[i]), int(self.fan.C[self.fan.rec_of[i]]))
        a = self.audios[rec]
        a = a if torch.is_tensor(a) else torch.as_tensor(a)
        raw = a.detach().cpu().contiguous().numpy()
        c = None if self.cd is None else int(self.cd[rec])
        if self.fan is not None:
            raw = deinterleave(raw, C, ch, c)
        elif c is not None:
            raw = g711_expand(raw, c)
        raw = np.ascontiguousarray(raw, dtype=np.int16 if self.dtype == torch.int16 else np.float32)
        alen = (len(raw) + self.step - 1) // self.step
        sg = np.ascontiguousarray(segs, dtype=np.int64).reshape(-1, 2)
        args = (raw.ctypes.data if raw.size else None, raw.itemsize, self.step, alen, sg.ctypes.data if len(sg) else None, len(sg),
                1 if self.invert else 0)
        need = lib().vad_collect_segments(*args, None, 0)
        if need < 0:
            raise _lib.VadError(-need, "vad_collect_segments")
        res = np.empty(need, raw.dtype)
        if lib().vad_collect_segments(*args, res.ctypes.data if need else None, need) != need:
            raise _lib.VadError(1, "vad_collect_segments")
        t = torch.from_numpy(res)
        return t.to(self.dev) if self.on_device else t

    def finish(self):
        for e0, e1 in self.events:
            e1.synchronize()
            STATS["audio_d2h_s"] += e0.elapsed_time(e1) / 1e3
        dtype = self.dtype
        if dtype is None:                                      # no bucket ran: every recording is empty
            dtype = torch.int16
        for i, a in enumerate(self.audio):
            if a is None:                                      # an empty recording is in no bucket
                self.audio[i] = torch.empty(0, dtype=dtype, device=self.dev if self.on_device and self.dev is not None else "cpu")
        return self.audio


def ragged_speech_audio(audios: Sequence, model, sampling_rate: int = 16000, max_waste: float = 0.15, max_bytes: int = 256 << 20,
                        keep: str = "speech", on_device: bool = False, as_arrays: bool = False, codec=None, channels=None, source_rate=None,
                        **scan_kw):
    """`ragged_speech_segments` AND the audio its segments keep -> (segments, audio): the speech of every recording (keep="speech",
    `collect_chunks`) or everything but the speech (keep="nonspeech", `drop_chunks`), collected on the GPU from the batch rows the scan
    ran on (vad_collect_segments_device, csrc/kernel_collect.hip) -- the recordings are not expanded, split, decimated or sliced on the
    host again, and only the kept bytes cross the link back, on a stream of their own while the following buckets compute.

    `segments` is exactly what `ragged_speech_segments` returns for the same arguments (`as_arrays` included).  `audio[i]` is a 1-D tensor
    of the batch's sample type -- int16 for int16 and G.711 recordings, float32 for float ones.  With recording i's TWIN being the
    recording after `g711_expand`, `deinterleave` and the reference's decimation x[::k] for a multiple of 16 kHz (`decimate`), so that
    segments and samples share the 16 kHz axis, audio[i] == collect_chunks(segments[i], twin_i) (drop_chunks for keep="nonspeech"),
    bit for bit.  A recording without segments gives an EMPTY tensor under keep="speech": the reference's `torch.cat([])` raises there,
    this call does not.  With `channels=` there is one entry per (recording, channel), in `channel_rows` order.

    on_device=True leaves the tensors on the GPU, as views of one packed buffer per bucket (for a consumer on the same device: nothing
    crosses the link); otherwise they are views of one pinned host buffer per bucket.  A recording with more segments than the scan's
    optimistic room (24) is collected on the host from its recording (vad_collect_segments) with the same result.  Needs a GPU model
    backed by the native engine.  The continuous-refill route (refill_*) holds a recording only a slab at a time and has no such
    call: out of scope.  STATS: collect_bytes (kept on the device), audio_d2h_bytes / audio_d2h_s (brought home)."""
    _no_source_rate(source_rate, "ragged_speech_audio")
    if keep not in ("speech", "nonspeech"):
        raise ValueError(f"keep must be 'speech' or 'nonspeech', got {keep!r}")
    if "device_scan" in scan_kw or "threads" in scan_kw:
        raise TypeError("ragged_speech_audio always scans on the device: device_scan / threads are not arguments of it")
    col = _AudioCollector(model, _rates(sampling_rate)[1], keep == "nonspeech", bool(on_device))
    segments = _speech_segments(audios, model, sampling_rate, max_waste, max_bytes, 0, None, as_arrays, codec, channels, col, scan_kw)
    return segments, col.finish()


def _segment_params(sampling_rate=16000, threshold=0.5, neg_threshold=None, min_speech_duration_ms=250,
                    max_speech_duration_s=float("inf"), min_silence_duration_ms=100, speech_pad_ms=30,
                    min_silence_at_max_speech=98, use_max_poss_sil_at_max_speech=True):
    p = _lib.SegmentParams()
    lib().vad_segment_params_default(ctypes.byref(p), int(sampling_rate))
    p.threshold = float(threshold)
    p.neg_threshold = -1.0 if neg_threshold is None else float(neg_threshold)
    p.min_speech_duration_ms = int(min_speech_duration_ms)
    p.max_speech_duration_s = float(max_speech_duration_s)
    p.min_silence_duration_ms = int(min_silence_duration_ms)
    p.speech_pad_ms = int(speech_pad_ms)
    p.min_silence_at_max_speech_ms = int(min_silence_at_max_speech)
    p.use_max_poss_sil_at_max_speech = 1 if use_max_poss_sil_at_max_speech else 0
    return p


def _device_scan(engine, probs_dev, n_chunks_dev, audio_len_dev, params, cap, row_offsets=None):
    """Enqueue the GPU scan of probs_dev[B, T] on the current stream -> (counts[B], segs[B, cap, 2]) int64, device.
    With `row_offsets` (device int64[B]) stream i's probabilities start at probs_dev.flatten()[row_offsets[i]]."""
    B, T = probs_dev.shape
    if row_offsets is not None:
        B = row_offsets.shape[0]
    counts = torch.empty((B,), dtype=torch.int64, device=probs_dev.device)
    segs = torch.empty((B, max(cap, 1), 2), dtype=torch.int64, device=probs_dev.device)
    _lib.check(engine._h, lib().vad_segment_probs_device(
        engine._h, probs_dev.data_ptr(), probs_dev.stride(0) if probs_dev.shape[0] > 1 else T,
        row_offsets.data_ptr() if row_offsets is not None else None, B,
        n_chunks_dev.data_ptr() if n_chunks_dev is not None else None, T, audio_len_dev.data_ptr(),
        ctypes.byref(params), segs.data_ptr(), segs.shape[1], counts.data_ptr(),
        ctypes.c_void_p(torch.cuda.current_stream(probs_dev.device).cuda_stream)))
    return counts, segs


def segment_probs_batch_device(engine, probs_dev: torch.Tensor, n_chunks, audio_lengths, sampling_rate=16000,
                               **scan_kw) -> List[list]:
    """`segment_probs_batch` for probabilities that are already on the GPU (probs_dev[B, T], CUDA): the scan runs
    there (vad_segment_probs_device) and only the segment lists are copied back."""
    B, T = probs_dev.shape
    params = _segment_params(sampling_rate, **scan_kw)
    both = torch.stack([torch.as_tensor(n_chunks, dtype=torch.int64), torch.as_tensor(audio_lengths, dtype=torch.int64)])
    if both.shape != (2, B):
        raise ValueError("n_chunks and audio_lengths need one entry per row of probs")
    if int(both[0].max() if B else 0) > T or int(both.min() if B else 0) < 0:
        raise ValueError("n_chunks must lie in [0, T] and audio lengths must not be negative")
    both = both.to(probs_dev.device)
    cap = 24
    while True:
        counts, segs = _device_scan(engine, probs_dev.contiguous(), both[0], both[1], params, cap)
        cnt = counts.cpu().numpy()
        if B == 0 or int(cnt.max()) <= cap:
            break
        cap = int(cnt.max())
    m = int(cnt.max()) if B else 0
    sg = segs[:, :max(m, 1)].cpu().numpy()
    return [[{"start": int(a), "end": int(b)} for a, b in sg[i, : cnt[i]]] for i in range(B)]


def segment_probs_batch(probs: torch.Tensor, n_chunks, audio_lengths, sampling_rate=16000, threshold=0.5,
                        neg_threshold=None, min_speech_duration_ms=250,
                        max_speech_duration_s=float("inf"), min_silence_duration_ms=100,
                        speech_pad_ms=30, min_silence_at_max_speech=98,
                        use_max_poss_sil_at_max_speech=True, threads=0) -> List[list]:
    """`timestamps.segment_probs` for every row of probs[B, T] in one native call (host threads)."""
    probs = torch.as_tensor(probs, dtype=torch.float32).contiguous().cpu()
    B, T = probs.shape
    p = _segment_params(sampling_rate, threshold, neg_threshold, min_speech_duration_ms, max_speech_duration_s,
                        min_silence_duration_ms, speech_pad_ms, min_silence_at_max_speech,
                        use_max_poss_sil_at_max_speech)
    nck = np.ascontiguousarray(n_chunks, dtype=np.int64)
    alen = np.ascontiguousarray(audio_lengths, dtype=np.int64)
    if nck.shape != (B,) or alen.shape != (B,):
        raise ValueError("n_chunks and audio_lengths need one entry per row of probs")
    cap = T // 2 + 2
    lp = ctypes.POINTER(ctypes.c_long)
    while True:     # counts[] may exceed cap (e.g. min_silence 0 with a small max_speech): grow and rescan
        segs = np.zeros((B, cap, 2), dtype=np.int64)
        counts = np.zeros(B, dtype=np.int64)
        rc = lib().vad_segment_probs_batch(
            ctypes.cast(probs.data_ptr(), _lib.f32p) if B * T else None, T, B,
            nck.ctypes.data_as(lp), alen.ctypes.data_as(lp), ctypes.byref(p),
            ctypes.cast(segs.ctypes.data, ctypes.POINTER(_lib.Segment)), cap, counts.ctypes.data_as(lp),
            int(threads))
        if rc < 0:
            from .timestamps import _raise_scan_error
            _raise_scan_error(rc)
        if B == 0 or int(counts.max()) <= cap:
            break
        cap = int(counts.max())
    return [[{"start": int(s), "end": int(e)} for s, e in segs[i, : counts[i]]] for i in range(B)]


# ---- offline: the enter / exit threshold search over a labelled corpus ----------------------------------------------
LABEL_IGNORE = 255        # VAD_LABEL_IGNORE: a chunk that does not exist for the sweep (the reference's masked chunks, tuning/utils.py:317-319)

ThresholdPairs = collections.namedtuple("ThresholdPairs", "enter exit enter_f32 exit_f32")
ThresholdPairs.__doc__ = """(enter, exit) threshold pairs: `enter` / `exit` float64[P] as the caller means them, `enter_f32` / `exit_f32` their directed
float32 roundings, which the sweep compares with (threshold_pairs)."""


def _round_f32(x: np.ndarray, up: bool) -> np.ndarray:
    """the smallest float32 >= x (up) / the largest float32 <= x (down), element by element"""
    f = x.astype(np.float32)
    with np.errstate(over="ignore"):
        if up:
            return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)
        return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def threshold_pairs(enter=None, exit=None) -> ThresholdPairs:
    """The grid of the reference's threshold search (calculate_best_thresholds, tuning/utils.py:328-331): every (enter, exit) with
    exit < enter, enter-major, from `enter` x `exit` (default: np.linspace(0, 1, 20) for both -- 190 pairs).

    The reference compares a float32 probability, widened to double, with these float64 values.  double(p) >= e holds exactly when
    p >= the smallest float32 >= e, and double(p) <= x exactly when p <= the largest float32 <= x: `enter_f32` is `enter` rounded UP
    and `exit_f32` is `exit` rounded DOWN, and the sweep compares in fp32 with the reference's outcome for every float32 probability."""
    en = np.linspace(0, 1, 20) if enter is None else np.asarray(enter, dtype=np.float64).reshape(-1)
    ex = np.linspace(0, 1, 20) if exit is None else np.asarray(exit, dtype=np.float64).reshape(-1)
    keep = ex[None, :] < en[:, None]                          # [enter, exit]: row-major is enter-major
    e = np.ascontiguousarray(np.broadcast_to(en[:, None], keep.shape)[keep])
    x = np.ascontiguousarray(np.broadcast_to(ex[None, :], keep.shape)[keep])
    return ThresholdPairs(e, x, _round_f32(e, True), _round_f32(x, False))


def _as_pairs(pairs) -> ThresholdPairs:
    if pairs is None:
        return threshold_pairs()
    if isinstance(pairs, ThresholdPairs):
        return pairs
    p = np.asarray(pairs, dtype=np.float64)                    # [P, 2]: the pairs as they are, none left out
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError("pairs: a ThresholdPairs (threshold_pairs) or an array [P, 2] of (enter, exit)")
    e, x = np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1])
    return ThresholdPairs(e, x, _round_f32(e, True), _round_f32(x, False))


def chunk_labels(speech_ts, n_samples: int, sampling_rate: int = 16000) -> np.ndarray:
    """Per-chunk 0 / 1 labels (uint8) of a recording of `n_samples` samples from its annotation, a list of {'start': s, 'end': s} in
    SECONDS -- the reference's rule (get_ground_truth_annotated, tuning/utils.py:113-133): samples int(start * sr) ... int(end * sr)
    are speech, the length is padded up to a whole chunk, and a chunk is speech when more than half of its samples are."""
    n = chunk_size(sampling_rate)
    chunks = (int(n_samples) + n - 1) // n
    gt = np.zeros(chunks * n, dtype=np.uint8)
    for seg in speech_ts:
        gt[int(seg["start"] * sampling_rate): int(seg["end"] * sampling_rate)] = 1
    return (gt.reshape(chunks, n).sum(axis=1, dtype=np.int64) * 2 > n).astype(np.uint8)


class ThresholdCounts:
    """The sweep's result: `pairs` (ThresholdPairs, P of them) and, for R recordings in the caller's order, the int32 counts
    tp[R, P], tn[R, P] (chunks decided speech / not speech and labelled so), n_pos[R] (labels equal to 1), n_valid[R] (labels equal
    to 0 or 1).  Everything else is derived from these integers on the host."""

    def __init__(self, pairs: ThresholdPairs, tp, tn, n_pos, n_valid):
        self.pairs = pairs
        self.tp, self.tn = np.asarray(tp, dtype=np.int32), np.asarray(tn, dtype=np.int32)
        self.n_pos, self.n_valid = np.asarray(n_pos, dtype=np.int32), np.asarray(n_valid, dtype=np.int32)

    def _scored(self):
        if len(self.n_valid) == 0 or int(self.n_valid.min()) <= 0:
            raise ValueError("a recording without a valid chunk cannot be scored")

    def accuracy(self) -> np.ndarray:
        """(tp + tn) / n_valid, float64[R, P]"""
        self._scored()
        return (self.tp.astype(np.int64) + self.tn) / self.n_valid.astype(np.int64)[:, None]

    def f1(self) -> np.ndarray:
        """2 tp / (2 tp + fp + fn) with fp = n_valid - n_pos - tn and fn = n_pos - tp, float64[R, P]; 0 where nothing is speech or
        called speech"""
        tp = self.tp.astype(np.int64)
        den = tp + self.n_valid.astype(np.int64)[:, None] - self.tn
        return np.divide(2.0 * tp, den, out=np.zeros(tp.shape, dtype=np.float64), where=den > 0)

    def best(self):
        """(enter, exit, accuracy): what the reference's calculate_best_thresholds returns on these recordings (tuning/utils.py:326-356),
        with its roundings -- per recording round(accuracy, 4) on a Python float, per pair round(np.mean(those), 3), a strict > against
        a running best that starts at 0, pairs in their order (enter-major), thresholds round(., 2)."""
        acc = self.accuracy()
        vals, inv = np.unique(acc, return_inverse=True)        # Python's round, once per distinct value
        acc4 = np.asarray([round(v, 4) for v in vals.tolist()], dtype=np.float64)[inv.reshape(-1)].reshape(acc.shape)
        per_pair = np.ascontiguousarray(acc4.T)                # a contiguous vector per pair: numpy sums it as it sums the reference's list
        best_acc, found = 0, None
        for k in range(per_pair.shape[0]):
            mean_acc = round(np.mean(per_pair[k]), 3)
            if mean_acc > best_acc:
                best_acc, found = mean_acc, k
        if found is None:
            raise ValueError("no threshold pair scores above 0")
        return round(self.pairs.enter[found], 2), round(self.pairs.exit[found], 2), best_acc


def _pack_labels(labels, n_chunks, who):
    """the rows' label arrays back to back -> (uint8[sum], int64 offsets[R]); every row's length is checked against its chunk count"""
    arrs = []
    for i, (lab, m) in enumerate(zip(labels, n_chunks)):
        a = lab.cpu().numpy() if isinstance(lab, torch.Tensor) else np.asarray(lab)
        if a.dtype != np.uint8:
            raise ValueError(f"{who}: labels must be uint8 arrays (0, 1, {LABEL_IGNORE} = ignore)")
        if a.ndim != 1 or len(a) != int(m):
            raise ValueError(f"{who}: row {i} has {int(m)} chunks and {a.size} labels")
        arrs.append(a)
    offs = np.zeros(len(arrs), dtype=np.int64)
    if arrs:
        offs[1:] = np.cumsum([len(a) for a in arrs[:-1]])
    return (np.concatenate(arrs) if arrs else np.zeros(0, np.uint8)), offs


def _sweep_rows(n_chunks, labels, B, T, who):
    nck = np.ascontiguousarray(n_chunks, dtype=np.int64)
    if nck.shape != (B,) or len(labels) != B:
        raise ValueError(f"{who}: n_chunks and labels need one entry per row of probs")
    if B and (int(nck.min()) < 0 or int(nck.max()) > T):
        raise ValueError(f"{who}: n_chunks must lie in [0, T]")
    return nck


def threshold_counts(probs, n_chunks, labels, pairs=None, threads: int = 0) -> ThresholdCounts:
    """The sweep on the host (vad_threshold_counts_host, the twin of the device kernel: one source, csrc/sweeper.hpp): probs[B, T]
    float32 on the CPU, row i's first n_chunks[i] entries against labels[i] (uint8[n_chunks[i]]: 0, 1, anything else = ignore) for
    every pair of `pairs` (threshold_pairs(); or an array [P, 2] of (enter, exit), taken as it is)."""
    pr = _as_pairs(pairs)
    probs = torch.as_tensor(probs, dtype=torch.float32).contiguous().cpu()
    if probs.dim() != 2:
        raise ValueError("threshold_counts: probs[B, T]")
    B, T = probs.shape
    nck = _sweep_rows(n_chunks, labels, B, T, "threshold_counts")
    lab, offs = _pack_labels(labels, nck, "threshold_counts")
    P = len(pr.enter)
    tp, tn = np.zeros((B, P), dtype=np.int32), np.zeros((B, P), dtype=np.int32)
    n_pos, n_valid = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    none = np.zeros(8, dtype=np.uint8)                         # (rows of no chunks: something to point at)
    rc = lib().vad_threshold_counts_host(probs.data_ptr() if B * T else none.ctypes.data, T, None, B, nck.ctypes.data,
                                         lab.ctypes.data if len(lab) else none.ctypes.data, offs.ctypes.data, pr.enter_f32.ctypes.data, pr.exit_f32.ctypes.data, P,
                                         tp.ctypes.data, tn.ctypes.data, n_pos.ctypes.data, n_valid.ctypes.data, int(threads))
    if rc != _lib.VAD_OK:
        raise _lib.VadError(rc, "vad_threshold_counts_host")
    return ThresholdCounts(pr, tp, tn, n_pos, n_valid)


def _device_sweep(engine, probs_dev, n_chunks_dev, labels_ptr, label_offs_dev, enter_dev, exit_dev, row_offsets=None):
    """Enqueue the sweep of probs_dev[B, T] on the current stream -> one int32 device tensor holding tp[B, P], tn[B, P], n_pos[B],
    n_valid[B] back to back (_split_counts), so that one copy brings a bucket's counts home."""
    B, T = probs_dev.shape
    if row_offsets is not None:
        B = row_offsets.shape[0]
    P = enter_dev.shape[0]
    out = torch.empty((B * (2 * P + 2),), dtype=torch.int32, device=probs_dev.device)
    at = out.data_ptr()
    _lib.check(engine._h, lib().vad_threshold_counts_device(
        engine._h, probs_dev.data_ptr(), probs_dev.stride(0) if probs_dev.shape[0] > 1 else T,
        row_offsets.data_ptr() if row_offsets is not None else None, B, n_chunks_dev.data_ptr(), labels_ptr, label_offs_dev.data_ptr(),
        enter_dev.data_ptr(), exit_dev.data_ptr(), P, at, at + 4 * B * P, at + 8 * B * P, at + 8 * B * P + 4 * B,
        ctypes.c_void_p(torch.cuda.current_stream(probs_dev.device).cuda_stream)))
    return out


def _split_counts(flat: np.ndarray, B: int, P: int):
    return flat[:B * P].reshape(B, P), flat[B * P:2 * B * P].reshape(B, P), flat[2 * B * P:2 * B * P + B], flat[2 * B * P + B:]


def _label_meta(nck: np.ndarray, lab: np.ndarray, offs: np.ndarray) -> torch.Tensor:
    """int64[2 R + ceil(bytes / 8)]: the rows' chunk counts, their label offsets, then the label bytes themselves (viewed as int64,
    padded with ignore) -- one small tensor to the device per batch"""
    R = len(nck)
    words = (len(lab) + 7) // 8
    m = np.empty(2 * R + words, dtype=np.int64)
    m[:R], m[R:2 * R] = nck, offs
    tail = m[2 * R:].view(np.uint8)
    tail[:len(lab)] = lab
    tail[len(lab):] = LABEL_IGNORE
    return torch.from_numpy(m)


def threshold_counts_device(engine, probs_dev: torch.Tensor, n_chunks, labels, pairs=None) -> ThresholdCounts:
    """`threshold_counts` for probabilities that are already on the GPU (probs_dev[B, T], CUDA float32, unit stride inside a row): the
    sweep runs there (vad_threshold_counts_device) and only the counts are copied back."""
    pr = _as_pairs(pairs)
    if probs_dev.dim() != 2 or probs_dev.dtype != torch.float32 or (probs_dev.shape[1] > 1 and probs_dev.stride(1) != 1):
        raise ValueError("threshold_counts_device: probs_dev[B, T] float32 with unit stride inside a row")
    B, T = probs_dev.shape
    nck = _sweep_rows(n_chunks, labels, B, T, "threshold_counts_device")
    lab, offs = _pack_labels(labels, nck, "threshold_counts_device")
    P = len(pr.enter)
    dev = probs_dev.device
    meta = _label_meta(nck, lab, offs).to(dev)
    thr = torch.from_numpy(np.stack([pr.enter_f32, pr.exit_f32])).to(dev)
    out = _device_sweep(engine, probs_dev, meta[:B], meta.data_ptr() + 16 * B, meta[B:2 * B], thr[0], thr[1])
    return ThresholdCounts(pr, *_split_counts(out.cpu().numpy(), B, P))


def ragged_threshold_counts(audios: Sequence, labels: Sequence, model, sampling_rate: int = 16000, pairs=None, max_waste: float = 0.15,
                            max_bytes: int = 256 << 20, codec=None, channels=None, source_rate=None, threads: int = 0) -> ThresholdCounts:
    """The threshold sweep over a labelled corpus (what tuning/search_thresholds.py does with model.audio_forward and
    calculate_best_thresholds): the recordings take the bucket route of `ragged_probs` and every bucket's sweep is enqueued right
    behind its kernels (vad_threshold_counts_device, one wave per recording and 64 pairs) -- the probabilities never leave the GPU,
    only the integer counts come back.  The bucket's labels ride to the device with its PCM, one byte per chunk.

    labels[i]: uint8, one entry per chunk of recording i (`chunk_labels`; 0, 1, anything else = ignore); with `channels` one per
    (recording, channel) in `channel_rows` order, with `source_rate` per chunk of the resampled recording.  ValueError if a row's
    label count differs from its chunk count or if it has no valid chunk (the reference's accuracy_score cannot score one either).
    The counts are, as integers, those of `threshold_counts` on `ragged_probs` of the same call.  A model without the device route (a
    CPU stand-in) takes the host twin.  codec / channels / source_rate / max_waste / max_bytes: as in ragged_probs."""
    pr = _as_pairs(pairs)
    audios, codec, channels, rs = _resample_input(audios, codec, channels, model, source_rate, sampling_rate)
    n = _rates(sampling_rate)[2]
    audios, codec, fan = _channel_input(audios, codec, channels, model)
    lengths = [_resampled_len(m, rs) for m in _describe(audios if fan is None else fan)[1]]
    source_rate = source_rate if rs else None
    R, P = len(lengths), len(pr.enter)
    nck = np.asarray([(m + n - 1) // n for m in lengths], dtype=np.int64)
    if len(labels) != R:
        raise ValueError(f"ragged_threshold_counts: {R} rows and {len(labels)} label arrays")
    lab, offs = _pack_labels(labels, nck, "ragged_threshold_counts")
    ignored = np.flatnonzero(lab > 1)                          # (sparse: a running sum over every label costs ten times this)
    valid = nck - (np.searchsorted(ignored, offs + nck) - np.searchsorted(ignored, offs))
    if R and int(valid.min()) == 0:
        raise ValueError(f"ragged_threshold_counts: row {int(np.argmin(valid))} has no valid chunk")
    tp, tn = np.zeros((R, P), dtype=np.int32), np.zeros((R, P), dtype=np.int32)
    n_pos, n_valid = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
    dev = getattr(model, "device", None)
    on_gpu = dev is not None and torch.device(dev).type == "cuda"

    def rows_of(idxs):
        ix = np.asarray(idxs, dtype=np.int64)
        return ix, [lab[offs[i]:offs[i] + nck[i]] for i in ix]

    if on_gpu and hasattr(getattr(model, "engine", None), "_h"):
        thr = torch.from_numpy(np.stack([pr.enter_f32, pr.exit_f32])).to(dev)

        def meta(idxs):
            ix, rows = rows_of(idxs)
            b_off = np.zeros(len(ix), dtype=np.int64)
            b_off[1:] = np.cumsum(nck[ix][:-1])
            return _label_meta(nck[ix], np.concatenate(rows) if rows else lab[:0], b_off)

        def post(probs_dev, idxs, m_dev):
            B = len(idxs)
            return [_device_sweep(model.engine, probs_dev, m_dev[:B], m_dev.data_ptr() + 16 * B, m_dev[B:2 * B], thr[0], thr[1])]

        for idxs, outs, _ in ragged_buckets(audios, model, sampling_rate, max_waste, max_bytes, post=post, meta=meta, codec=codec, _fan=fan,
                                            source_rate=source_rate):
            ix = np.asarray(idxs, dtype=np.int64)
            tp[ix], tn[ix], n_pos[ix], n_valid[ix] = _split_counts(outs[0].numpy(), len(ix), P)
    else:
        for idxs, probs in ragged_buckets(audios, model, sampling_rate, max_waste, max_bytes, codec=codec, _fan=fan, source_rate=source_rate):
            ix, rows = rows_of(idxs)
            c = threshold_counts(probs, nck[ix], rows, pr, threads)
            tp[ix], tn[ix], n_pos[ix], n_valid[ix] = c.tp, c.tn, c.n_pos, c.n_valid
    return ThresholdCounts(pr, tp, tn, n_pos, n_valid)


def search_thresholds(audios: Sequence, labels: Sequence, model, sampling_rate: int = 16000, **kw):
    """(enter, exit, accuracy) of the reference's threshold search (tuning/search_thresholds.py) over a labelled corpus:
    `ragged_threshold_counts(...).best()`."""
    return ragged_threshold_counts(audios, labels, model, sampling_rate, **kw).best()


# ---- offline: validation loss and ROC-AUC of a labelled corpus -------------------------------------------------------
SCORE_KEY_NONE = 0xFFFFFFFF   # VAD_SCORE_KEY_NONE: the key of a chunk that is not valid (csrc/scorer.hpp)


class ValidationScores:
    """What the reference's validate() (tuning/utils.py:252-298) needs of a labelled validation set, for R recordings in the caller's
    order: bce_pos[R], bce_neg[R] (float64: the sums of the BCE terms of the valid label-1 / label-0 chunks), n_pos[R], n_neg[R]
    (int32: valid chunks by label), n_bad[R] (int32: chunks labelled 0 / 1 whose probability is not in [0, 1]), n_chunks[R] (int64),
    and the pooled rank statistic as Python ints: u2 = sum over the positive chunks of 2 #{negatives with a smaller probability} +
    #{negatives with an equal one}, total_pos, total_neg.  `keys` (uint32, one per chunk at the recordings' corpus offsets) is kept
    where the caller asked for it, else None."""

    def __init__(self, bce_pos, bce_neg, n_pos, n_neg, n_bad, n_chunks, u2, total_pos, total_neg, keys=None):
        self.bce_pos, self.bce_neg = np.asarray(bce_pos, dtype=np.float64), np.asarray(bce_neg, dtype=np.float64)
        self.n_pos, self.n_neg, self.n_bad = (np.asarray(a, dtype=np.int32) for a in (n_pos, n_neg, n_bad))
        self.n_chunks = np.asarray(n_chunks, dtype=np.int64)
        self.u2, self.total_pos, self.total_neg = int(u2), int(total_pos), int(total_neg)
        self.keys = keys

    def _no_bad(self):
        bad = int(self.n_bad.astype(np.int64).sum())
        if bad:
            raise ValueError(f"{bad} labelled chunks have a probability outside [0, 1] (a NaN too): all elements of input should be between 0 and 1")

    def roc_auc(self) -> float:
        """u2 / (2 total_pos total_neg): the Mann-Whitney statistic with ties at one half, what roc_auc_score returns on all chunks"""
        self._no_bad()
        if self.total_pos == 0 or self.total_neg == 0:
            raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
        return self.u2 / (2 * self.total_pos * self.total_neg)

    def loss(self, noise_loss: float = 0.5, batch_size=None) -> float:
        """The reference's losses.avg: sum(bce_pos + noise_loss bce_neg) / sum over the batches of numel, a batch being `batch_size`
        consecutive recordings (a DataLoader without shuffling) and numel = len(batch) x its largest chunk count -- the padded count
        (loss * masks).mean() divides by.  batch_size None: every recording is its own batch, nothing padded."""
        self._no_bad()
        nck = self.n_chunks
        if batch_size is None:
            numel = int(nck.sum())
        else:
            b = int(batch_size)
            if b <= 0:
                raise ValueError("batch_size must be positive")
            numel = sum(len(nck[a:a + b]) * int(nck[a:a + b].max()) for a in range(0, len(nck), b))
        if numel == 0:
            raise ValueError("no chunk to average over")
        return float((math.fsum(self.bce_pos.tolist()) + float(noise_loss) * math.fsum(self.bce_neg.tolist())) / numel)

    def reference(self, noise_loss: float = 0.5, batch_size=None):
        """(loss, round(roc_auc, 3)): the pair the reference's validate() returns"""
        return self.loss(noise_loss, batch_size), round(self.roc_auc(), 3)


def _auc_counts_host(keys: np.ndarray):
    out = np.zeros(3, dtype=np.uint64)
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    rc = lib().vad_auc_counts_host(keys.ctypes.data if len(keys) else None, len(keys), out.ctypes.data)
    if rc != _lib.VAD_OK:
        raise _lib.VadError(rc, "vad_auc_counts_host")
    return int(out[0]), int(out[1]), int(out[2])


def _key_offsets(nck: np.ndarray, who):
    offs = np.zeros(len(nck), dtype=np.int64)
    if len(nck):
        offs[1:] = np.cumsum(nck[:-1])
    total = int(nck.sum())
    if total >= 1 << 31:
        raise ValueError(f"{who}: {total} chunks; the pooled ROC-AUC takes fewer than 2^31")
    return offs, total


def _score_rows_host(probs, nck, lab, l_offs, k_offs, keys, threads):
    """vad_chunk_scores_host on probs[B, T] (a CPU float32 tensor) -> (bce_pos, bce_neg, n_pos, n_neg, n_bad); row i's keys are written
    to keys[k_offs[i]:]"""
    B, T = probs.shape
    bp, bn = np.zeros(B, dtype=np.float64), np.zeros(B, dtype=np.float64)
    cp, cn, cb = (np.zeros(B, dtype=np.int32) for _ in range(3))
    none = np.zeros(8, dtype=np.uint8)                         # (rows of no chunks: something to point at)
    rc = lib().vad_chunk_scores_host(probs.data_ptr() if B * T else none.ctypes.data, T, None, B, nck.ctypes.data,
                                     lab.ctypes.data if len(lab) else none.ctypes.data, l_offs.ctypes.data, k_offs.ctypes.data,
                                     keys.ctypes.data if len(keys) else none.ctypes.data, bp.ctypes.data, bn.ctypes.data, cp.ctypes.data,
                                     cn.ctypes.data, cb.ctypes.data, int(threads))
    if rc != _lib.VAD_OK:
        raise _lib.VadError(rc, "vad_chunk_scores_host")
    return bp, bn, cp, cn, cb


def chunk_scores(probs, n_chunks, labels, threads: int = 0) -> ValidationScores:
    """The validation scores on the host (vad_chunk_scores_host + vad_auc_counts_host, the twins of the device kernels: one source,
    csrc/scorer.hpp): probs[B, T] float32 on the CPU, row i's first n_chunks[i] entries against labels[i] (uint8[n_chunks[i]]: 0, 1,
    anything else = ignore)."""
    probs = torch.as_tensor(probs, dtype=torch.float32).contiguous().cpu()
    if probs.dim() != 2:
        raise ValueError("chunk_scores: probs[B, T]")
    B, T = probs.shape
    nck = _sweep_rows(n_chunks, labels, B, T, "chunk_scores")
    lab, offs = _pack_labels(labels, nck, "chunk_scores")
    total = _key_offsets(nck, "chunk_scores")[1]
    keys = np.full(total, SCORE_KEY_NONE, dtype=np.uint32)
    rows = _score_rows_host(probs, nck, lab, offs, offs, keys, threads)
    return ValidationScores(*rows, nck, *_auc_counts_host(keys), keys=keys)


def _score_meta(nck: np.ndarray, lab: np.ndarray, l_offs: np.ndarray, k_offs: np.ndarray) -> torch.Tensor:
    """int64[3 R + ceil(bytes / 8)]: the rows' chunk counts, label offsets and key offsets, then the label bytes (viewed as int64,
    padded with ignore) -- one small tensor to the device per batch"""
    R = len(nck)
    words = (len(lab) + 7) // 8
    m = np.empty(3 * R + words, dtype=np.int64)
    m[:R], m[R:2 * R], m[2 * R:3 * R] = nck, l_offs, k_offs
    tail = m[3 * R:].view(np.uint8)
    tail[:len(lab)] = lab
    tail[len(lab):] = LABEL_IGNORE
    return torch.from_numpy(m)


def _device_scores(engine, probs_dev, m_dev, B, keys_dev):
    """Enqueue the score kernel of probs_dev's first B rows on the current stream; m_dev is the rows' _score_meta on the device.  The
    keys go to keys_dev (int32 storage of the uint32 keys) at the rows' key offsets; returns ONE float64 device tensor holding
    bce_pos[B], bce_neg[B], then n_pos[B], n_neg[B], n_bad[B] as int32 (_split_scores), so that one copy brings a bucket's sums home."""
    out = torch.empty((2 * B + (3 * B + 1) // 2,), dtype=torch.float64, device=probs_dev.device)
    at, mp = out.data_ptr(), m_dev.data_ptr()
    _lib.check(engine._h, lib().vad_chunk_scores_device(
        engine._h, probs_dev.data_ptr(), probs_dev.stride(0) if probs_dev.shape[0] > 1 else probs_dev.shape[1], None, B, mp, mp + 24 * B,
        mp + 8 * B, mp + 16 * B, keys_dev.data_ptr(), at, at + 8 * B, at + 16 * B, at + 20 * B, at + 24 * B,
        ctypes.c_void_p(torch.cuda.current_stream(probs_dev.device).cuda_stream)))
    return out


def _split_scores(flat: np.ndarray, B: int):
    ints = flat[2 * B:].view(np.int32)
    return flat[:B], flat[B:2 * B], ints[:B], ints[B:2 * B], ints[2 * B:3 * B]


def _device_auc(engine, keys_dev, total):
    """vad_auc_counts_device over keys_dev[:total] on the current stream -> (u2, total_pos, total_neg); 24 bytes come home"""
    dev = keys_dev.device
    need = int(lib().vad_auc_workspace_bytes(total))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    out = torch.empty(3, dtype=torch.int64, device=dev)
    _lib.check(engine._h, lib().vad_auc_counts_device(engine._h, keys_dev.data_ptr(), total, ws.data_ptr(), need, out.data_ptr(),
                                                      ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return tuple(int(v) for v in out.cpu().numpy().view(np.uint64))


def chunk_scores_device(engine, probs_dev: torch.Tensor, n_chunks, labels, keep_keys: bool = False) -> ValidationScores:
    """`chunk_scores` for probabilities that are already on the GPU (probs_dev[B, T], CUDA float32, unit stride inside a row): the score
    kernel and the pooled count run there (vad_chunk_scores_device, vad_auc_counts_device); the per-row sums and counts and three
    integers are copied back -- and the keys, with keep_keys."""
    if probs_dev.dim() != 2 or probs_dev.dtype != torch.float32 or (probs_dev.shape[1] > 1 and probs_dev.stride(1) != 1):
        raise ValueError("chunk_scores_device: probs_dev[B, T] float32 with unit stride inside a row")
    B, T = probs_dev.shape
    nck = _sweep_rows(n_chunks, labels, B, T, "chunk_scores_device")
    lab, offs = _pack_labels(labels, nck, "chunk_scores_device")
    total = _key_offsets(nck, "chunk_scores_device")[1]
    dev = probs_dev.device
    keys_dev = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    m_dev = _score_meta(nck, lab, offs, offs).to(dev)
    out = _device_scores(engine, probs_dev, m_dev, B, keys_dev)
    auc = _device_auc(engine, keys_dev, total)
    keys = keys_dev[:total].cpu().numpy().view(np.uint32) if keep_keys else None
    return ValidationScores(*_split_scores(out.cpu().numpy(), B), nck, *auc, keys=keys)


def ragged_validation(audios: Sequence, labels: Sequence, model, sampling_rate: int = 16000, max_waste: float = 0.15,
                      max_bytes: int = 256 << 20, codec=None, channels=None, source_rate=None, threads: int = 0,
                      keep_keys: bool = False) -> ValidationScores:
    """The validation scores of a labelled corpus (the reference's validate(), tuning/utils.py:252-298: masked BCE loss and the ROC-AUC of
    every chunk of the set): the recordings take the bucket route of `ragged_probs` and every bucket's score kernel is enqueued right
    behind its kernels (vad_chunk_scores_device, one wave per recording).  It leaves the per-recording BCE sums and counts, which come
    home in one copy per bucket, and one uint32 key per chunk in ONE device array at the recording's corpus offset; after the last
    bucket vad_auc_counts_device counts the pooled rank statistic over that array and 24 bytes come home.  The probabilities never
    leave the GPU.

    labels: as in ragged_threshold_counts (uint8 per chunk; 0, 1, anything else = ignore; with `channels` one array per (recording,
    channel) in `channel_rows` order, with `source_rate` per chunk of the resampled recording).  ValueError if a row's label count
    differs from its chunk count or the corpus has 2^31 chunks or more.  A model without the device route (a CPU stand-in) takes the
    host twins over the buckets' probabilities.  keep_keys: also bring the keys home (tests).  codec / channels / source_rate /
    max_waste / max_bytes: as in ragged_probs."""
    audios, codec, channels, rs = _resample_input(audios, codec, channels, model, source_rate, sampling_rate)
    n = _rates(sampling_rate)[2]
    audios, codec, fan = _channel_input(audios, codec, channels, model)
    lengths = [_resampled_len(m, rs) for m in _describe(audios if fan is None else fan)[1]]
    source_rate = source_rate if rs else None
    R = len(lengths)
    nck = np.asarray([(m + n - 1) // n for m in lengths], dtype=np.int64)
    if len(labels) != R:
        raise ValueError(f"ragged_validation: {R} rows and {len(labels)} label arrays")
    lab, offs = _pack_labels(labels, nck, "ragged_validation")
    total = _key_offsets(nck, "ragged_validation")[1]
    bp, bn = np.zeros(R, dtype=np.float64), np.zeros(R, dtype=np.float64)
    cp, cn, cb = (np.zeros(R, dtype=np.int32) for _ in range(3))
    dev = getattr(model, "device", None)
    on_gpu = dev is not None and torch.device(dev).type == "cuda"

    def rows_of(idxs):
        ix = np.asarray(idxs, dtype=np.int64)
        return ix, [lab[offs[i]:offs[i] + nck[i]] for i in ix]

    def local_offsets(ix):
        b_off = np.zeros(len(ix), dtype=np.int64)
        b_off[1:] = np.cumsum(nck[ix][:-1])
        return b_off

    if on_gpu and hasattr(getattr(model, "engine", None), "_h"):
        keys_dev = torch.empty(max(total, 1), dtype=torch.int32, device=dev)      # every chunk's key, written bucket by bucket

        def meta(idxs):
            ix, rows = rows_of(idxs)
            return _score_meta(nck[ix], np.concatenate(rows) if rows else lab[:0], local_offsets(ix), offs[ix])

        def post(probs_dev, idxs, m_dev):
            return [_device_scores(model.engine, probs_dev, m_dev, len(idxs), keys_dev)]

        for idxs, outs, _ in ragged_buckets(audios, model, sampling_rate, max_waste, max_bytes, post=post, meta=meta, codec=codec, _fan=fan,
                                            source_rate=source_rate):
            ix = np.asarray(idxs, dtype=np.int64)
            bp[ix], bn[ix], cp[ix], cn[ix], cb[ix] = _split_scores(outs[0].numpy(), len(ix))
        # (the lanes' streams have been joined into the current one: every bucket's keys are in front of this)
        auc = _device_auc(model.engine, keys_dev, total)
        keys = keys_dev[:total].cpu().numpy().view(np.uint32) if keep_keys else None
    else:
        keys = np.full(total, SCORE_KEY_NONE, dtype=np.uint32)
        for idxs, probs in ragged_buckets(audios, model, sampling_rate, max_waste, max_bytes, codec=codec, _fan=fan, source_rate=source_rate):
            ix, rows = rows_of(idxs)
            p = torch.as_tensor(probs, dtype=torch.float32).contiguous()
            bp[ix], bn[ix], cp[ix], cn[ix], cb[ix] = _score_rows_host(p, np.ascontiguousarray(nck[ix]), np.concatenate(rows) if rows else lab[:0],
                                                                      local_offsets(ix), np.ascontiguousarray(offs[ix]), keys, threads)
        auc = _auc_counts_host(keys)
        keys = keys if keep_keys else None
    return ValidationScores(bp, bn, cp, cn, cb, nck, *auc, keys=keys)


def validate(audios: Sequence, labels: Sequence, model, sampling_rate: int = 16000, noise_loss: float = 0.5, batch_size=None, **kw):
    """(loss, ROC-AUC rounded to 3 decimals) of a labelled corpus, the pair the reference's validate() returns (tuning/utils.py:252-298):
    `ragged_validation(...).reference(noise_loss, batch_size)`."""
    return ragged_validation(audios, labels, model, sampling_rate, **kw).reference(noise_loss, batch_size)


# ---- offline: continuous refill ------------------------------------------------------------------------------------
class RefillPlan:
    """A fixed number of stream slots, processed in time slabs of `slab_chunks` chunks; a slot whose recording ends
    inside a slab is handed the next recording at the following slab boundary (state and context reset) instead of
    idling until the longest member of a bucket is done.  This is the reference's padded lock-step batch
    (`SileroVadPadder`, tuning/utils.py:146-160; bounded blocks, examples/onnx_sequence/run.py:34-56) with rows
    retired and re-admitted: the waste per recording is below one slab, whatever the spread of the lengths.

    The schedule depends on the lengths only, so it is computed up front: `slabs` is a list of
    (slot, recording, first_sample, n_samples, reset) tuples per slab.  Recordings are admitted longest first, behind a few of the
    shortest (so that results start to flow at once)."""

    def __init__(self, lengths: Sequence[int], slots: int, slab_chunks: int, chunk: int, order=None, ramp: int = 1):
        """order: the admission order (recording indices; empty recordings are skipped) instead of longest-first -- the window feed
        admits recordings in ARENA order, so that the bytes the slots need next are the bytes the next window DMA brings.
        ramp (with order): the slots START over `ramp` slabs, a 1 / ramp of them per slab, lowest slots first -- the first slab then
        needs the audio of slots / ramp recordings instead of all slots' (2 GiB for 2 048 slots of 30 s recordings: 37 ms of link
        time in front of the first kernel), and the first recordings retire that much earlier."""
        lens = self.lengths = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)     # (an array: a shard has 10^5 recordings)
        self.slots, self.slab_chunks, self.chunk = int(slots), int(slab_chunks), int(chunk)
        if self.slots < 1 or self.slab_chunks < 1:
            raise ValueError("slots and slab_chunks must be positive")
        width = self.slab_chunks * self.chunk
        live = np.flatnonzero(lens > 0)
        if order is not None:
            queue = np.ascontiguousarray(order, dtype=np.int64).reshape(-1)
            queue = queue[lens[queue] > 0]
            if len(queue) != len(live) or len(np.unique(queue)) != len(queue):
                raise ValueError("order must name every non-empty recording once")
        else:
            queue = live[np.argsort(-lens[live], kind="stable")]  # longest first, ties in input order
        # ... except that a sixteenth of the slots START with the shortest recordings: with the longest in every slot nothing retires
        # before the longest recording's last slab (a shard of 30 s recordings: 13 of 580 slabs, 5 % of the run, before the first result
        # reaches the host); the shortest retire after their own few slabs and the results flow from then on.  They are taken from the end
        # of the queue, where they would have filled the last slabs' gaps: a 1 / 16 of the slots' worth of the shortest does not move the
        # makespan of a shard.
        early = min(self.slots // 16, len(queue) - self.slots) if len(queue) > self.slots else 0
        if early > 0 and order is None:
            queue = np.concatenate([queue[len(queue) - early:][::-1], queue[:len(queue) - early]])
        self.empty = np.flatnonzero(lens <= 0).tolist()
        need = np.ascontiguousarray((lens[queue] + width - 1) // width)   # slabs each recording occupies its slot for
        # event-driven form of "at every slab boundary, every free slot (in slot order) takes the next recording": a heap of (slab at
        # which the slot becomes free, slot) -- native (vad_refill_schedule: a corpus shard has 10^5 recordings)
        lp = ctypes.POINTER(ctypes.c_long)
        ramp = int(ramp) if order is not None else 1
        g = self.slots // ramp if ramp > 1 else 0
        if ramp > 1 and g >= 1 and len(queue) > self.slots:
            # the staggered start, expressed in the scheduler's own terms: behind the first g recordings (slots 0 .. g - 1 at slab 0)
            # the queue holds one PLACEHOLDER per remaining slot that keeps it busy for its delay (slot s starts at slab s // g, the
            # last slots at ramp - 1); the recordings behind them take the slots as the placeholders end, in queue order
            delay = np.minimum(np.arange(g, self.slots, dtype=np.int64) // g, ramp - 1)
            need_q = np.ascontiguousarray(np.concatenate([need[:g], delay, need[g:]]))
            start_q = np.zeros(len(need_q), dtype=np.int64)
            slot_q = np.zeros(len(need_q), dtype=np.int64)
            if lib().vad_refill_schedule(need_q.ctypes.data_as(lp), len(need_q), self.slots, start_q.ctypes.data_as(lp), slot_q.ctypes.data_as(lp)):
                raise ValueError("vad_refill_schedule: bad arguments")
            real = np.ones(len(need_q), dtype=bool)
            real[g:g + len(delay)] = False
            start, slot = np.ascontiguousarray(start_q[real]), np.ascontiguousarray(slot_q[real])
        else:
            start = np.zeros(len(queue), dtype=np.int64)
            slot = np.zeros(len(queue), dtype=np.int64)
            if lib().vad_refill_schedule(need.ctypes.data_as(lp), len(queue), self.slots, start.ctypes.data_as(lp), slot.ctypes.data_as(lp)):
                raise ValueError("vad_refill_schedule: bad arguments")
        # one row per (recording, slab it is active in): [slot, recording, first sample, samples, reset], by slab, then by slot (native:
        # 1.3 M rows for a shard -- vad_refill_table)
        n_slabs = int((start + need).max()) if len(queue) else 0
        rows = np.empty((int(need.sum()), 5), dtype=np.int64)
        cuts = np.zeros(n_slabs + 1, dtype=np.int64)
        rec = np.ascontiguousarray(queue, dtype=np.int64)
        qlen = np.ascontiguousarray(lens[queue])
        got = lib().vad_refill_table(need.ctypes.data_as(lp), start.ctypes.data_as(lp), slot.ctypes.data_as(lp), rec.ctypes.data_as(lp),
                                     qlen.ctypes.data_as(lp), len(queue), self.slots, width, n_slabs, rows.ctypes.data_as(lp),
                                     cuts.ctypes.data_as(lp))
        if got != len(rows):
            raise ValueError("vad_refill_table: bad arguments")
        # the schedule as arrays (slot, recording, first sample, samples, reset flag) per slab, for the vectorised stager
        self.slab_arrays = [rows[cuts[k]:cuts[k + 1]] for k in range(n_slabs)]
        # first / last slab each recording is active in (-1: empty recording): what the window feed plans its device buffers on
        self.first_slab = np.full(len(lens), -1, dtype=np.int64)
        self.last_slab = np.full(len(lens), -1, dtype=np.int64)
        self.first_slab[queue] = start
        self.last_slab[queue] = start + need - 1

    @property
    def slabs(self) -> List[list]:
        """The schedule as lists of (slot, recording, first sample, samples, reset) tuples per slab."""
        return [[(int(a), int(b), int(c), int(d), bool(e)) for a, b, c, d, e in arr] for arr in self.slab_arrays]

    def n_chunks(self, i: int) -> int:
        return (int(self.lengths[i]) + self.chunk - 1) // self.chunk

    def padded_chunks(self) -> int:
        return len(self.slab_arrays) * self.slots * self.slab_chunks

    def real_chunks(self) -> int:
        live = self.lengths[self.lengths > 0]
        return int(((live + self.chunk - 1) // self.chunk).sum())


def _assign_window_buffers(first: np.ndarray, last: np.ndarray, ahead: int, slack: int = 1):
    """Device buffers for the refill route's arena windows, planned up front (the schedule is static).  Window w is first read by
    the gather of slab first[w], last by the gather of slab last[w]; its DMA is ISSUED while slab issue[w] = max(0, first[w] - ahead)
    is being staged, before that slab's gather.  A buffer may take window w if the window it held was last read by a slab BEFORE
    issue[w] (its release event exists by then).  Windows are issued in index order (first[] is non-decreasing in arena order).
    `slack`: the previous window must have been last read at least `slack` slabs before the issue slab -- the refill loop knows, when it
    stages slab k, that the uploads of slabs <= k - 2 are COMPLETE (it waited for that staging slot), so with slack 2 a window's DMA never
    carries an open device-side dependency (a copy that does is taken off the copy engines' fast path: 35.6 instead of 19 ms per GiB for
    hundreds of ms, profiles/r06_refill_window_feed.md).
    Returns (buffer index per window, number of buffers, issue slab per window)."""
    first = np.asarray(first, dtype=np.int64)
    last = np.asarray(last, dtype=np.int64)
    issue = np.maximum(first - int(ahead), 0)
    issue = np.maximum.accumulate(issue) if len(issue) else issue      # in-order issue: a window is never issued before its predecessor
    buf = np.zeros(len(first), dtype=np.int64)
    import heapq
    busy = []                                                           # (last slab of the window held, buffer)
    free = []
    n_buf = 0
    for w in range(len(first)):
        while busy and busy[0][0] <= issue[w] - slack:
            heapq.heappush(free, heapq.heappop(busy)[1])
        if free:
            j = heapq.heappop(free)
        else:
            j, n_buf = n_buf, n_buf + 1
        buf[w] = j
        heapq.heappush(busy, (int(last[w]), j))
    return buf, n_buf, issue


def _refill_iter(audios: Sequence, model, sampling_rate: int, slots: int, slab_chunks: int, plan: "RefillPlan" = None, on_slab=None,
                 prepare_only: bool = False, codec=None, channels=None, _fan=None):
    """The continuous-refill loop (RefillPlan) as a generator: stages slab k + 1 while the kernels of slab k run, scatters every slab's
    probabilities into one flat device tensor (recording i owns out_flat[base[i] : base[i + 1]]) and yields k once slab k has been
    ENQUEUED.  `on_slab(k, finished, out_flat, base)` is called right before that, with the recordings whose last chunk lies in slab k
    (np.int64 array, may be empty): the hook for work that follows a recording's retirement in stream order.  The generator's return
    value is (out_flat, base, plan).  `prepare_only`: plan the run and make everything that allocates -- the window buffers, the staging
    slots, the engine's scratch, the flat probability tensor -- then stop (refill_reserve): a run over the same recordings allocates
    nothing (7 GiB of window buffers for a 1 263 h shard are 60 ms when they come fresh from the driver, 0.5 s when an outgrown block
    has to go back first).  `codec`: the recordings are uint8 G.711 codes (ragged_buckets: the same rules -- every route carries
    the codes at one byte a sample and the gather kernel expands them into the int16 slab).  `channels`: the recordings are interleaved
    (ragged_buckets: the same rules).  Every channel is a queue entry of its own, next to its sibling and with the same need, so the
    schedule is that of the flat list of de-interleaved recordings; where a slab's slots want the same frames of both channels of a
    recording that is ONE source of the slab's upload, where the schedule admitted the two at different slabs each slab names the
    channel it wants (_Fanned.table)."""
    t_setup = time.perf_counter()
    net_sr, _, n = _rates(sampling_rate)
    eng = model.engine
    inp = _corpus_input(audios, model, codec, channels, _fan)
    recs, lengths, cd, fan = inp.recs, inp.lengths, inp.cd, inp.fan     # (interleaved: `recs` the sources; lengths, plan, base, results the rows')
    dtype, esz, src_dtype, src_esz = inp.dtype, inp.esz, inp.src_dtype, inp.src_esz
    n_rows = len(lengths)
    dev = torch.device(getattr(eng, "torch_device", None) or torch.device("cuda", eng.device))
    on_gpu = dev.type == "cuda"
    lens_np = np.asarray(lengths, dtype=np.int64).reshape(-1)
    slots = max(1, min(int(slots), int((lens_np > 0).sum())))
    mode = _upload_mode()
    # The window feed (recordings that lie in ONE pinned arena, GPU engine, no plan handed in): recordings are admitted in ARENA order,
    # the arena goes to the GPU by one DMA per window (copy engines: no CU time, exactly the live bytes) a few slabs ahead of the
    # slots that read it, and a slab's rows are cut out of the windows' device copies at HBM speed -- instead of a gather kernel that
    # reads 128 KB row pieces over PCIe beside the frontend (0.90 of the link).  The device buffers are planned up front
    # (_assign_window_buffers: the schedule is static); a corpus whose long recordings would pin more than the budget of window
    # buffers (SILERO_VAD_AMD_REFILL_WINDOW_BUDGET, 16 GiB of the 288) keeps the gather route.
    wf = None
    if plan is None and on_gpu and mode in ("", "window") and hasattr(eng, "upload_rows"):
        packed = recs if isinstance(recs, PackedRecordings) else _as_packed(recs)
        if packed is not None and packed.base.is_pinned() and int((lens_np > 0).sum()):
            slab_bytes = slots * slab_chunks * n * src_esz                                      # (of the arena: what a slab reads of a window)
            wbytes = int(os.environ.get("SILERO_VAD_AMD_REFILL_WINDOW", 0)) or (1 << 30)        # (256 MiB windows: 0.92 of the link, 1 GiB: 0.95)
            # (the slots start over `ramp` slabs and the first windows are small -- 1/8, 1/4, 1/2 of a window: the first kernel runs
            #  after 7 ms of link time instead of 37, the first recordings retire that much earlier)
            ramp = max(1, int(os.environ.get("SILERO_VAD_AMD_REFILL_RAMP", "8")))
            order, bounds, o_, e_ = _arena_windows(packed.offsets, packed.lengths, wbytes // src_esz, lead_limit=(wbytes // src_esz) // 8 if int(os.environ.get("SILERO_VAD_AMD_REFILL_LEAD", ramp > 1)) else 0)
            spans = np.asarray([(o_[a], e_[b - 1]) for a, b in bounds], dtype=np.int64).reshape(-1, 2)
            copied = int((spans[:, 1] - spans[:, 0]).sum())
            dense = mode == "window" or float(packed.lengths[packed.lengths > 0].sum()) >= 0.6 * copied
            if dense:
                rows_in = (lambda r: r) if fan is None else fan.rows_of       # (the rows of recordings, in their order)
                wplan = RefillPlan(lens_np, slots, slab_chunks, n, order=rows_in(order), ramp=ramp)
                win_of = np.full(len(packed), -1, dtype=np.int64)
                for w, (a, b) in enumerate(bounds):
                    win_of[order[a:b]] = w
                w_first = np.asarray([wplan.first_slab[rows_in(order[a:b])].min() for a, b in bounds], dtype=np.int64)
                w_last = np.asarray([wplan.last_slab[rows_in(order[a:b])].max() for a, b in bounds], dtype=np.int64)
                wmax = int((spans[:, 1] - spans[:, 0]).max()) * src_esz
                wmax = (wmax + 255) // 256 * 256
                ahead = max(2, -(-2 * wmax // max(slab_bytes, 1))) + 1          # two windows' worth of slabs in front of the reader
                slack = int(os.environ.get("SILERO_VAD_AMD_REFILL_SLACK", "2"))      # (1: A/B -- the DMAs may then wait on the device)
                buf_of, n_buf, issue = _assign_window_buffers(w_first, w_last, ahead, slack=slack)
                budget = int(os.environ.get("SILERO_VAD_AMD_REFILL_WINDOW_BUDGET", 0))
                if not budget:                                               # 16 GiB of the 288, less on a device that others fill
                    held = getattr(getattr(model, "_stage_pool", None), "refill_windows", None)
                    free = torch.cuda.mem_get_info(dev)[0] + (held.numel() if held is not None else 0)
                    budget = min(16 << 30, free // 4)
                if n_buf * wmax <= budget:
                    plan = wplan
                    wf = {"packed": packed, "spans": spans, "win_of": win_of, "first": w_first, "last": w_last, "buf_of": buf_of,
                          "n_buf": n_buf, "wmax": wmax, "issue": issue, "next": 0, "ev": {}, "release": {}, "holder": {}, "slack": slack}
                    STATS["refill_window_feed"] += 1
                    STATS["refill_window_buffers"] = max(STATS["refill_window_buffers"], n_buf)
    plan = plan or RefillPlan(lens_np, slots, slab_chunks, n)
    B, S, width = plan.slots, plan.slab_chunks, plan.slab_chunks * n
    base = np.zeros(n_rows + 1, dtype=np.int64)   # recording i owns out_flat[base[i] : base[i] + n_chunks(i)]
    np.cumsum(np.where(lens_np > 0, (lens_np + n - 1) // n, 0), out=base[1:])
    total = int(base[-1])
    out_flat = torch.zeros(total + 1, dtype=torch.float32, device=dev)      # [+1]: sink for the padding chunks
    ctx = torch.zeros((B, chunk_size(net_sr) // 8), dtype=torch.float32, device=dev)
    state = torch.zeros((2, B, 128), dtype=torch.float32, device=dev)
    done = np.zeros(n_rows, dtype=np.int64)       # chunks of each recording already produced
    ctxm = contextlib.nullcontext() if not on_gpu else torch.cuda.device(dev)
    pool = None
    with ctxm:
        if on_gpu:
            pool = getattr(model, "_stage_pool", None)
            cur = torch.cuda.current_stream(dev)
            if pool is None:
                pool = model._stage_pool = _StagePool(dev)
                pool.stream = _distinct_queue_stream(getattr(model, "engine", None), dev, [cur],    # the upload beside the slab's kernels
                                                     priority=int(os.environ.get("SILERO_VAD_AMD_UPLOAD_PRIORITY", "0")))
        STATS["padded"] += plan.padded_chunks() * n
        STATS["real"] += int(lens_np[lens_np > 0].sum())

        ing = _Ingest(inp, recs, pool, eng, on_gpu)    # (pinned recordings: one gather kernel per slab, no host copy)
        ing.windowed = wf is not None
        ptr0 = ing.src.ptr
        if on_gpu and hasattr(eng, "reserve"):
            eng.reserve(sampling_rate, B, S)
        if wf is not None:
            # the window buffers: one device block, kept on the staging pool from call to call; written by the copy stream, read by
            # the cut kernels on pool.stream
            need_b = wf["n_buf"] * wf["wmax"]
            blk = getattr(pool, "refill_windows", None)
            if blk is None or blk.numel() < need_b:
                if blk is not None:                        # a larger plan than the last call's: the old block goes back to the DRIVER
                    blk = pool.refill_windows = None       # first (GiBs that torch's cache would keep beside the new one)
                    torch.cuda.synchronize(dev)
                    torch.cuda.empty_cache()
                blk = pool.refill_windows = torch.empty(need_b, dtype=torch.uint8, device=dev)
                STATS["slot_allocs"] += 1
            # (the DMAs on a hardware queue that carries neither the slabs' kernels nor the cuts: a copy queued behind a kernel of
            #  another stream on the same queue waits for it)
            wf["stream"] = _copy_stream(pool, model, dev, [cur, pool.stream])
            blk.record_stream(wf["stream"])
            blk.record_stream(pool.stream)
            wf["stream"].wait_stream(cur)                  # (the block's previous use, the arena's writer: both in front of this call)
            wf["stream"].wait_stream(pool.stream)
            wf["blk"] = blk
            # every recording's device address, once: its window's buffer + its place in the window's span
            w_ = wf["win_of"]
            livem = w_ >= 0
            dptr = np.zeros(len(w_), dtype=np.uint64)
            dptr[livem] = (blk.data_ptr() + wf["buf_of"][w_[livem]] * wf["wmax"]
                           + (wf["packed"].offsets[livem] - wf["spans"][w_[livem], 0]) * src_esz).astype(np.uint64)
            ptr0 = dptr

        def issue_windows(upto):
            """start the DMA of every window whose issue slab is <= upto (in order; a buffer's previous window was released by an
            earlier slab's cuts -- _assign_window_buffers)"""
            while wf["next"] < len(wf["first"]) and wf["issue"][wf["next"]] <= upto:
                v = wf["next"]
                j = int(wf["buf_of"][v])
                a, b = (int(x) for x in wf["spans"][v])
                nb = (b - a) * src_esz
                prev = wf["holder"].get(j)
                if prev is not None:
                    # recorded behind the last cut that read window `prev`, at least two slabs ago: complete by now (stage() has waited
                    # for the upload of slab k - 2), so this returns at once and the DMA below is issued WITHOUT a device-side dependency
                    rel = wf["release"].pop(prev)
                    if wf["slack"] >= 2:
                        rel.synchronize()
                    else:
                        wf["stream"].wait_event(rel)
                with torch.cuda.stream(wf["stream"]):
                    wf["blk"][j * wf["wmax"]: j * wf["wmax"] + nb].view(src_dtype).copy_(wf["packed"].base[a:b], non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(wf["stream"])
                wf["ev"][v] = ev
                wf["holder"][j] = v
                wf["by_first"].setdefault(int(wf["first"][v]), []).append(v)
                STATS["h2d_bytes"] += nb
                wf["next"] += 1

        if wf is not None:
            wf["by_first"] = {}
            wf["by_last"] = {}
            for v, l in enumerate(wf["last"]):
                wf["by_last"].setdefault(int(l), []).append(v)

        # The scatter indices and reset lists of G consecutive slabs cross the link in ONE copy (the schedule is static: a group's are
        # known when its first slab is staged).  A small copy per slab costs the large transfers beside it far more than its bytes:
        # the refill route's window DMAs ran at 0.907 of the link with a 2 MB copy per slab and the scans' three small ones, 0.949
        # without them (profiles/r06_refill_window_feed.md).
        G = max(1, int(os.environ.get("SILERO_VAD_AMD_REFILL_GROUP", "8")))
        n_slabs_all = len(plan.slab_arrays)
        grp = {"g": -1, "host": [None, None], "ev": [None, None], "dev": None, "roff": {}, "next": 0}

        def prepare(j):
            """slab j's scatter description and reset list into its group's page-locked buffer: int64 [per slab: first output index of
            every slot (B) | chunks every slot produces (B)] [resets of every slab] -- 48 KB per slab instead of the B S indices
            themselves (2 MB: 0.75 % of the link's bytes on the gather route); the indices are formed on the device (scatter_index).
            One slab per call: the host work stays spread over the slabs."""
            g = j // G
            lo, cnt = g * G, min(G, n_slabs_all - g * G)
            q, b = j - lo, g % 2
            cap = cnt * 3 * B
            if q == 0:
                if on_gpu and grp["ev"][b] is not None:
                    grp["ev"][b].synchronize()                                 # the copy that last read this buffer (two groups ago)
                if grp["host"][b] is None or grp["host"][b].numel() < cap:
                    grp["host"][b] = torch.empty(max(cap, 1024), dtype=torch.int64, pin_memory=on_gpu)
                grp["roff"][g] = [cnt * 2 * B]
            e = plan.slab_arrays[j]                                        # [entries, 5], vectorised bookkeeping
            sl, rec, take = e[:, 0], e[:, 1], e[:, 3]
            nck = (take + n - 1) // n
            hb = grp["host"][b].numpy()
            v = hb[q * 2 * B:(q + 1) * 2 * B]
            v[:] = 0                                                       # a slot without a recording produces nothing
            v[sl] = base[rec] + done[rec]
            v[B + sl] = nck
            done[rec] += nck
            rs = sl[e[:, 4] != 0]
            r0 = grp["roff"][g][-1]
            hb[r0:r0 + len(rs)] = rs
            grp["roff"][g].append(r0 + len(rs))

        def slab_meta(k):
            """(first index per slot, chunks per slot, resets) of slab k as tensors where the kernels run; a group's ONE copy is issued
            (on pool.stream) with its first slab"""
            while grp["next"] < n_slabs_all and grp["next"] <= k + G:    # this slab's group is complete, the next one grows by a slab
                prepare(grp["next"])
                grp["next"] += 1
            g = k // G
            if g != grp["g"]:
                b, roff = g % 2, grp["roff"][g]
                grp["g"] = g
                grp["roff"].pop(g - 1, None)
                if not on_gpu:
                    grp["dev"] = grp["host"][b][: roff[-1]].clone()
                else:
                    with torch.cuda.stream(pool.stream):
                        grp["dev"] = grp["host"][b][: roff[-1]].to(dev, non_blocking=True)
                        grp["ev"][b] = torch.cuda.Event()
                        grp["ev"][b].record(pool.stream)
            q, roff = k - g * G, grp["roff"][g]
            return grp["dev"][q * 2 * B:(q + 1) * 2 * B], grp["dev"][roff[q]:roff[q + 1]]

        cols_d = torch.arange(S, dtype=torch.int64, device=dev)[None, :]

        def scatter_index(sn):
            """[B S] output positions of a slab: slot b's chunk c goes to first[b] + c while c < chunks[b], to the sink otherwise"""
            first, count = sn[:B, None], sn[B:, None]
            return torch.where(cols_d < count, first + cols_d, total).reshape(-1)

        def stage(k):
            e = plan.slab_arrays[k]                                        # [entries, 5], vectorised bookkeeping
            sl, rec, at, take = e[:, 0], e[:, 1], e[:, 2], e[:, 3]
            if fan is not None:
                # the slab's sources: the slots that read the same frames of one recording -- its two channels, admitted together --
                # share one
                src_k, at_k, _, dst_k = fan.table(rec, at, sl)
                ch_k = fan.C[src_k].astype(np.uint8)
                rows = ptr0[src_k] + (at_k * fan.C[src_k] * src_esz).astype(np.uint64)
                lens = np.minimum(fan.frames[src_k] - at_k, width)
                cd_k = None if cd is None else cd[src_k]
                if len(sl) < B:
                    # a slot without a recording: an empty one-channel source names it, so the row is zeros as on the mono path
                    idle = np.setdiff1d(np.arange(B, dtype=np.int64), sl)
                    ch_k = np.concatenate([ch_k, np.ones(len(idle), dtype=np.uint8)])
                    rows = np.concatenate([rows, np.zeros(len(idle), dtype=np.uint64)])
                    lens = np.concatenate([lens, np.zeros(len(idle), dtype=np.int64)])
                    cd_k = None if cd_k is None else np.concatenate([cd_k, np.zeros(len(idle), dtype=np.uint8)])
                    dst_k = np.concatenate([dst_k, np.stack([idle, np.full(len(idle), -1)], axis=1).astype(np.int32)])
                b = _Batch(rows, lens, cd_k, ch_k, dst_k, B, width)
            else:
                rows = np.zeros(B, dtype=np.uint64)
                lens = np.zeros(B, dtype=np.int64)
                rows[sl] = ptr0[rec] + (at * src_esz).astype(np.uint64)
                lens[sl] = take
                cd_k = None
                if cd is not None:
                    cd_k = np.zeros(B, dtype=np.uint8)                        # (a slot without a recording: an empty row, zeros)
                    cd_k[sl] = cd[rec]
                b = _Batch(rows, lens, cd_k, None, None, B, width)
            t0 = time.perf_counter()
            if not on_gpu:
                assert fan is None                                            # (a CPU stand-in was handed the de-interleaved recordings)
                host = torch.empty((B, width), dtype=dtype)
                _pack_rows(b.ptr, b.lens, width, src_esz, host.data_ptr())
                STATS["stage_s"] += time.perf_counter() - t0
                STATS["buckets"] += 1
                idx_k, rs_k = slab_meta(k)
                return host, None, 0, idx_k, rs_k
            idx_k, rs_k = slab_meta(k)                                      # (the group's one copy goes out with its first slab)
            h = ing.host(k, b, since=t0)
            if wf is not None:
                issue_windows(k)
                for v in wf["by_first"].pop(k, ()):                         # the windows this slab is the first to read
                    pool.stream.wait_event(wf["ev"].pop(v))
            with torch.cuda.stream(pool.stream):
                ing.device(h, b)
                if wf is not None:
                    for v in wf["by_last"].pop(k, ()):                     # the windows this slab is the last to read: released
                        rel = torch.cuda.Event()
                        rel.record(pool.stream)
                        wf["release"][v] = rel
                ev = torch.cuda.Event()
                ev.record(pool.stream)
            pool.done[h.slot] = ev
            return h.d, ev, h.slot, idx_k, rs_k

        n_slabs = len(plan.slab_arrays)
        STATS["setup_s"] += time.perf_counter() - t_setup
        if prepare_only:
            if on_gpu:
                ing.reserve(B * width * esz)
                torch.cuda.synchronize(dev)
            return None, base, plan
        staged = stage(0) if n_slabs else None
        for k in range(n_slabs):
            x, ev, slot, idx, rs = staged
            if on_gpu:
                cur.wait_event(ev)
                for t in (x, idx, rs):
                    t.record_stream(cur)
            if rs.numel():                                                # re-admitted slots start like reset_states()
                ctx.index_fill_(0, rs, 0.0)
                state.index_fill_(1, rs, 0.0)
            probs = eng.forward_audio(x, sampling_rate, ctx, state)     # [B, S], carried ctx/state updated in place
            out_flat.index_put_((scatter_index(idx),), probs.reshape(-1))
            if on_gpu:
                pool.consumed[slot] = torch.cuda.Event()
                pool.consumed[slot].record(cur)
            t_a = time.perf_counter()
            if on_slab is not None:
                e = plan.slab_arrays[k]
                on_slab(k, e[e[:, 2] + e[:, 3] >= lens_np[e[:, 1]], 1], out_flat, base)
            t_b = time.perf_counter()
            staged = stage(k + 1) if k + 1 < n_slabs else None          # CPU packs k+1 meanwhile
            if TRACE is not None:
                TRACE.append((k, t_a, t_b, time.perf_counter()))
            yield k
    return out_flat, base, plan


def _drain(gen):
    """run a generator to its end -> its return value"""
    while True:
        try:
            next(gen)
        except StopIteration as stop:
            return stop.value


def _refill_run(audios, model, sampling_rate, slots, slab_chunks, plan=None, codec=None, _fan=None):
    return _drain(_refill_iter(audios, model, sampling_rate, slots, slab_chunks, plan, codec=codec, _fan=_fan))


def refill_reserve(audios: Sequence, model, sampling_rate: int = 16000, slots: int = 1024, slab_chunks: int = 32, codec=None, channels=None,
                   source_rate=None):
    """Everything a refill run over these recordings allocates, allocated now (`ragged_reserve`'s twin): the arena windows' device
    buffers, the staging slots, the engine's scratch, the block the flat probability tensor will take.  Returns the plan."""
    _no_source_rate(source_rate, "refill_reserve")
    return _drain(_refill_iter(audios, model, sampling_rate, slots, slab_chunks, prepare_only=True, codec=codec, channels=channels))[2]


def refill_probs(audios: Sequence, model, sampling_rate: int = 16000, slots: int = 1024, slab_chunks: int = 32,
                 plan: RefillPlan = None, _keep_on_device: bool = False, codec=None, channels=None, source_rate=None):
    """Speech probabilities of many recordings of different lengths through `slots` persistent stream slots
    (RefillPlan).  Returns one 1-D CPU float tensor per recording, bit-identical to
    ``model.audio_forward(audio[None], sr)[0]``: the state and context a slot carries from slab to slab are exactly
    what a single call carries from chunk to chunk, and a re-admitted slot starts from zeros like `reset_states()`.
    Staging of slab k+1 (native threaded copy into pinned memory + H2D on a side stream) overlaps the kernels of
    slab k.  `audios`: float tensors in [-1, 1] or int16 PCM (all of one kind); `sampling_rate` may be a multiple of 16000 (raw
    recordings, _rates: a slab is slab_chunks x 512 k raw samples, the carried context is the 16 kHz net's).  `codec` ("ulaw" / "alaw",
    or one per recording): uint8 G.711 recordings, as in ragged_probs.  `channels`: interleaved recordings, one result per (recording,
    channel) as in ragged_probs."""
    _no_source_rate(source_rate, "refill_probs")
    audios, codec, fan = _channel_input(audios, codec, channels, model)
    out_flat, base, plan = _refill_run(audios, model, sampling_rate, slots, slab_chunks, plan, codec=codec, _fan=fan)
    if _keep_on_device:
        return out_flat, base, plan
    flat = out_flat.cpu()
    return [flat[base[i]:base[i + 1]].clone() for i in range(len(base) - 1)]


def refill_segments_stream(audios: Sequence, model, sampling_rate: int = 16000, slots: int = 1024, slab_chunks: int = 32, codec=None,
                           channels=None, _fan=None, source_rate=None, **scan_kw):
    """The continuous-refill scheduler with RESULTS AS RECORDINGS RETIRE -- what the reference's worker pool does, each file's
    timestamps handed back when that file is done (examples/parallel_example.ipynb cell 7).  Generator of
    (recording indices int64[m], counts int64[m], segments int64[m, cap, 2]) batches: behind the slab in which a recording's last
    chunk was computed, ONE device scan (vad_segment_probs_device, a lane per recording, over the recording's own row of the flat
    probability tensor) turns the retired recordings into segment lists, which ride back over PCIe asynchronously; a batch is
    yielded as soon as its copy has landed (a slab or two behind the kernels; nothing here blocks the pipeline).  Probabilities
    never leave the GPU.  Segments are in samples of the net's rate (x[::k] for raw 32 / 48 kHz recordings).  codec: as in refill_probs.
    channels: interleaved recordings; the indices yielded are those of channel_rows."""
    _no_source_rate(source_rate, "refill_segments_stream")
    net_sr, dec, _ = _rates(sampling_rate)
    fan = _fan                                                            # (refill_speech_segments resolved `channels=` already)
    if fan is None:
        audios, codec, fan = _channel_input(audios, codec, channels, model)
    lengths = (np.asarray(_describe(audios if fan is None else fan)[1], dtype=np.int64).reshape(-1) + dec - 1) // dec     # samples at the net's rate: the scan's unit
    eng = model.engine
    on_gpu = hasattr(eng, "_h")
    if not on_gpu:                                                        # CPU stand-in engines (tests): scan at the end, on the host
        flat, base, _ = _refill_run(audios, model, sampling_rate, slots, slab_chunks, codec=codec, _fan=fan)
        from .timestamps import segment_probs
        for i in range(len(lengths)):
            sg = segment_probs(flat[base[i]:base[i + 1]], int(lengths[i]), net_sr, **scan_kw) if lengths[i] > 0 else []
            arr = np.asarray([[d["start"], d["end"]] for d in sg], dtype=np.int64).reshape(1, -1, 2)
            yield np.asarray([i], dtype=np.int64), np.asarray([len(sg)], dtype=np.int64), arr
        return
    params = _segment_params(net_sr, **scan_kw)
    cap0 = 32
    pending = collections.deque()                                         # (indices, counts pinned, segs pinned, event, device handles)
    ready = []

    def collect(block):
        while pending and (block or pending[0][3].query()):
            idx, bufs, m, ev, flat_ref, meta_d = pending.popleft()
            ev.synchronize()
            cnt = bufs[1][:m].numpy().copy()
            segs = bufs[2][:m].numpy().copy()
            side["free"].append(bufs)
            if len(cnt) and int(cnt.max()) > cap0:                          # rare: a recording with more segments than were copied back
                with torch.cuda.stream(side["stream"]):
                    c2, s2 = _device_scan(eng, flat_ref[None], meta_d[0], meta_d[1], params, int(cnt.max()), row_offsets=meta_d[2])
                    cnt, segs = c2.cpu().numpy(), s2.cpu().numpy()
            STATS["d2h_bytes"] += segs.nbytes + cnt.nbytes
            ready.append((idx, cnt.copy(), segs))

    side = {"free": []}                                                  # page-locked result buffers, recycled (a pinned allocation per
                                                                          # slab costs milliseconds and can wait for the device)

    def pinned_set(m):
        """(meta int64[3, m], counts int64[m], segs int64[m, cap0, 2]) in page-locked memory, from the free list when one is big enough"""
        for i, bufs in enumerate(side["free"]):
            if bufs[0].shape[1] >= m:
                side["free"].pop(i)
                break
        else:
            cap = max(64, 1 << int(np.ceil(np.log2(max(m, 1)))))
            bufs = (torch.empty((3, cap), dtype=torch.int64, pin_memory=True), torch.empty((cap,), dtype=torch.int64, pin_memory=True),
                    torch.empty((cap, cap0, 2), dtype=torch.int64, pin_memory=True))
        return bufs

    import os as _os
    G = max(1, int(_os.environ.get("SILERO_VAD_AMD_REFILL_GROUP", "8")))
    acc = {"lists": [], "since": 0, "first": True, "args": None}

    def on_slab(k, finished, out_flat, base):
        # the recordings that retire are scanned G slabs at a time (the very first ones at once: results start to flow with the first
        # retirement): a scan is three small copies, and small copies cost the large transfers beside them (see _refill_iter)
        acc["args"] = (out_flat, base)
        if len(finished):
            acc["lists"].append(finished)
        acc["since"] += 1
        if acc["lists"] and (acc["first"] or acc["since"] >= G):
            flush(k)
        collect(False)

    def flush(k):
        out_flat, base = acc["args"]
        finished = np.concatenate(acc["lists"]) if len(acc["lists"]) > 1 else acc["lists"][0]
        acc["lists"], acc["since"], acc["first"] = [], 0, False
        if len(finished):
            # The scan of the recordings that retired in this slab runs on a SIDE stream, behind the slab's kernels by event: one lane per
            # recording walks ~1 000 probabilities one after the other (2-5 ms for the few dozen recordings of a slab) -- on the
            # compute stream that would stand between this slab's kernels and the next slab's (measured: the leg became compute-bound,
            # 0.81 of the link); beside them it is one wave.
            t0 = time.perf_counter()
            dev = out_flat.device
            cur = torch.cuda.current_stream(dev)
            if "stream" not in side:
                # (on a hardware queue of its own: a scan that lands on the upload's or the compute stream's queue serialises with it
                #  -- measured as 3.4 ms holes in the upload stream every time a wave of recordings retires, 0.79 instead of 0.90 of
                #  the link, depending on which streams the process happened to create before)
                pool = getattr(model, "_stage_pool", None)
                others = [cur] + ([pool.stream] if pool is not None else [])
                if getattr(pool, "copy_stream", None) is not None:            # (the window feed's DMA queue)
                    others.append(pool.copy_stream)
                side["stream"] = _distinct_queue_stream(eng, dev, others)
            done_k = torch.cuda.Event()
            done_k.record(cur)
            side["stream"].wait_event(done_k)
            m = len(finished)
            bufs = pinned_set(m)
            bufs[0][0, :m] = torch.from_numpy(base[finished + 1] - base[finished])
            bufs[0][1, :m] = torch.from_numpy(lengths[finished])
            bufs[0][2, :m] = torch.from_numpy(base[finished])
            with torch.cuda.stream(side["stream"]):
                meta = bufs[0][:, :m].to(dev, non_blocking=True)
                counts, segs = _device_scan(eng, out_flat[None], meta[0], meta[1], params, cap0, row_offsets=meta[2])
                bufs[1][:m].copy_(counts, non_blocking=True)
                bufs[2][:m].copy_(segs, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(side["stream"])
            pending.append((finished.copy(), bufs, m, ev, out_flat, meta))
            STATS["scan_s"] += time.perf_counter() - t0

    for _ in _refill_iter(audios, model, sampling_rate, slots, slab_chunks, None, on_slab, codec=codec, _fan=fan):
        while ready:
            yield ready.pop(0)
    if acc["lists"]:
        flush(-1)
    collect(True)
    while ready:
        yield ready.pop(0)
    if "stream" in side:                                                  # later work on the caller's stream is ordered behind the scans
        torch.cuda.current_stream().wait_stream(side["stream"])
    empty = np.flatnonzero(lengths <= 0)
    if len(empty):
        yield empty.astype(np.int64), np.zeros(len(empty), dtype=np.int64), np.zeros((len(empty), 1, 2), dtype=np.int64)


def refill_speech_segments(audios: Sequence, model, sampling_rate: int = 16000, slots: int = 1024,
                           slab_chunks: int = 32, as_arrays: bool = False, codec=None, channels=None, source_rate=None, **scan_kw) -> List[list]:
    """`ragged_speech_segments` over the continuous-refill scheduler (refill_segments_stream: every recording is scanned on the GPU
    behind the slab it retires in, its segment list crosses PCIe while later slabs run).  as_arrays: (counts int64[n], segments
    int64[sum(counts), 2]) like ragged_speech_segments, instead of a list of lists of dicts.  codec / channels: as in refill_probs."""
    _no_source_rate(source_rate, "refill_speech_segments")
    audios, codec, fan = _channel_input(audios, codec, channels, model)
    n_rec = len(audios) if fan is None else len(fan)
    counts_all = np.zeros(n_rec, dtype=np.int64)
    parts = []
    for idx, cnt, segs in refill_segments_stream(audios, model, sampling_rate, slots, slab_chunks, codec=codec, _fan=fan, **scan_kw):
        counts_all[idx] = cnt
        parts.append((idx, cnt, segs))
    t0 = time.perf_counter()
    first = np.concatenate([[0], np.cumsum(counts_all)])
    flat = np.zeros((int(first[-1]), 2), dtype=np.int64)
    for idx, cnt, sg in parts:
        if not len(idx) or not cnt.any():
            continue
        k = np.arange(sg.shape[1])[None, :]
        mask = k < cnt[:, None]
        flat[(first[idx][:, None] + k)[mask]] = sg[mask]
    STATS["scan_s"] += time.perf_counter() - t0
    if as_arrays:
        return counts_all, flat
    fl = flat.tolist()
    return [[{"start": a, "end": b} for a, b in fl[first[i]:first[i + 1]]] for i in range(n_rec)]


# ---- live streams --------------------------------------------------------------------------------------
# Live streams: StreamPool drives the engine directly (no host synchronisation per tick), fp32 like everything else.
class StreamPool:
    """`capacity` concurrently live streams on one GPU, one `tick` per 32 ms chunk.

    tick(chunks[capacity, N]) -> probs[capacity] (a CUDA tensor that is overwritten by the next
    tick).  Rows of closed slots are computed too (lock-step batch) and ignored.  With
    `graph=True` the step is captured once into a hipGraph and replayed; the input is then copied
    into a fixed staging buffer first.

    `tick(chunks, present=flags)`: live streams do not arrive in lock step.  A row whose flag is 0 has NO chunk this tick and is
    not stepped: its (h, c) and context stay bit for bit what they were and its probability slot holds -1.0 (VAD_PROB_ABSENT) --
    what the reference's per-stream callers do by simply not calling the model (src/silero_vad/utils_vad.py:507-549, one
    `__call__` per chunk that arrived).  The other rows' results do not depend on the flags.  Without flags the tick is the
    same launch it always was (a second hipGraph holds the flagged form; it is captured on first use).

    `dtype=torch.int16`: the chunks are 16-bit PCM, scaled by 1/32768 inside the kernel's loads -- what every
    non-Python client of the reference feeds (examples/onnx_sequence/run.py:115-119, examples/cpp/wav.h:113-118) and
    half the PCIe bytes of fp32.

    `host_slots=R` (R >= 1) makes the pool a HOST-TO-HOST server, the shape of the reference's streaming caller (host chunk
    in, probability out: src/silero_vad/utils_vad.py:507-549): a page-locked ingest ring `host_pcm[R, capacity, N]` that the
    audio sources write into directly (no staging copy on the host) and `host_prob[R, capacity]`; slot r has ONE hipGraph =
    H2D of host_pcm[r] -> the fused step -> D2H of the probabilities into host_prob[r], replayed on the pool's own stream.
    `submit(r)` starts a tick and returns, `wait(r)` blocks until its probabilities are readable on the host;
    `tick_host(r)` = both.  Ticks of one pool execute in submission order (the carried state demands it); with R >= 2 the
    next tick may be submitted while the host still reads the previous one, and several pools (each on a clone of the
    engine) overlap one pool's H2D with another's kernel."""

    def __init__(self, engine, sampling_rate: int = 16000, capacity: int = 8192, graph: bool = True,
                 dtype: torch.dtype = torch.float32, host_slots: int = 0):
        if dtype not in (torch.float32, torch.int16):
            raise TypeError(f"StreamPool dtype must be float32 or int16, got {dtype}")
        self.engine = engine
        self.sr = int(sampling_rate)
        self.n = chunk_size(self.sr)
        self.capacity = int(capacity)
        self.dtype = dtype
        self.device = torch.device("cuda", engine.device)
        with torch.cuda.device(self.device):
            self.ctx = torch.zeros((self.capacity, self.n // 8), device=self.device)
            self.state = torch.zeros((2, self.capacity, 128), device=self.device)
            self.pcm = torch.zeros((self.capacity, self.n), dtype=dtype, device=self.device)
            self.prob = torch.zeros((self.capacity,), device=self.device)
            self.host_slots = int(host_slots)
            self.host_pcm = self.host_prob = self.stream = None
            if self.host_slots:
                self.host_pcm = torch.zeros((self.host_slots, self.capacity, self.n), dtype=dtype, pin_memory=True)
                self.host_prob = torch.zeros((self.host_slots, self.capacity), dtype=torch.float32, pin_memory=True)
                self.stream = torch.cuda.Stream(self.device)
                self._done = [torch.cuda.Event() for _ in range(self.host_slots)]
                self.host_present = torch.ones((self.host_slots, self.capacity), dtype=torch.uint8, pin_memory=True)
            self.present = torch.ones((self.capacity,), dtype=torch.uint8, device=self.device)     # flags of the tick (device staging)
        self._graph_present = None
        self._host_graphs_present = None
        self.open_mask = np.zeros(self.capacity, dtype=bool)
        self._free = list(range(self.capacity - 1, -1, -1))
        self._graph = None
        self._host_graphs = None
        self._graph_gen = None
        self._use_graph = bool(graph)
        engine.reserve(self.sr, self.capacity, 1)
        if graph:
            self._capture()

    def _launch(self, masked=False):
        if masked:  # rows with self.present[b] == 0 are not stepped (vad_step_present)
            self.engine.step_present(self.pcm, self.sr, self.ctx, self.state, self.prob, self.present)
        elif self.dtype == torch.float32:
            self.engine.step(self.pcm, self.sr, self.ctx, self.state, self.prob)
        else:       # one chunk of int16 PCM per stream: a ONE-step vad_forward_audio_i16 call (the same fused kernel)
            self.engine.forward_audio(self.pcm, self.sr, self.ctx, self.state, self.prob.view(self.capacity, 1))

    def _host_tick(self, r, stream=None, masked=False):
        """What slot r's graph holds: ingest ring -> HBM, the step, probabilities -> host (one native call: vad_step_host)."""
        # (the kernel stores the probabilities straight into the page-locked host_prob[r]: no device buffer, no D2H operation)
        if masked:
            self.engine.step_host(self.host_pcm[r], self.pcm, self.sr, self.ctx, self.state, None, self.host_prob[r], stream,
                                  host_present=self.host_present[r], dev_present=self.present)
        else:
            self.engine.step_host(self.host_pcm[r], self.pcm, self.sr, self.ctx, self.state, None, self.host_prob[r], stream)

    def _capture(self):
        """Capture one step into a hipGraph.  The graph bakes in the engine's scratch addresses, so it is tied to
        the engine's scratch generation (include/silero_vad_hip.h, vad_scratch_generation) and is captured again,
        with the carried state preserved, when another user of the same engine made the scratch grow."""
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            keep_ctx, keep_state = self.ctx.clone(), self.state.clone()
            self.engine.reserve(self.sr, self.capacity, 1)
            side = torch.cuda.Stream(self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):
                self._launch()                             # warm-up outside capture (lazy module load)
            torch.cuda.current_stream(self.device).wait_stream(side)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._launch()
            self._graph = g
            if self._graph_present is not None:            # (only pools that have ticked with flags hold the flagged graphs)
                with torch.cuda.stream(side):
                    self._launch(masked=True)
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._launch(masked=True)
                self._graph_present = g
            if self.host_slots:
                self._host_graphs = []
                for r in range(self.host_slots):
                    hg = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(hg, stream=self.stream):
                        self._host_tick(r)
                    self._host_graphs.append(hg)
                if self._host_graphs_present is not None:
                    self._host_graphs_present = []
                    for r in range(self.host_slots):
                        hg = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(hg, stream=self.stream):
                            self._host_tick(r, masked=True)
                        self._host_graphs_present.append(hg)
            torch.cuda.synchronize(self.device)
            self.ctx.copy_(keep_ctx)                       # the warm-up step advanced them
            self.state.copy_(keep_state)
            torch.cuda.synchronize(self.device)            # (a host-mode replay on self.stream may follow at once)
            self._graph_gen = self.engine.scratch_generation()

    # -- slots ---------------------------------------------------------------------------------------
    def open(self) -> int:
        """Admit a stream: returns its slot; the slot starts from zero state/context."""
        if not self._free:
            raise RuntimeError("StreamPool is full")
        s = self._free.pop()
        with self._state_stream():
            self.ctx[s].zero_()
            self.state[:, s].zero_()
        self.open_mask[s] = True
        return s

    def open_all(self):
        """Admit `capacity` streams at once (every slot from zero state)."""
        with self._state_stream():
            self.ctx.zero_()
            self.state.zero_()
        self.open_mask[:] = True
        self._free = []

    def close(self, slot: int):
        if not self.open_mask[slot]:
            raise ValueError(f"slot {slot} is not open")
        self.open_mask[slot] = False
        self._free.append(int(slot))

    def reset(self, slot: int):
        with self._state_stream():
            self.ctx[slot].zero_()
            self.state[:, slot].zero_()

    def _state_stream(self):
        """Where writes to the carried state are issued.  A host-mode pool (host_slots > 0) runs its ticks on its own
        non-blocking stream: the zeroing of a slot must be ordered on THAT stream, or a tick submitted right behind
        open()/reset() could read the state before the zeroing has landed.  Device-mode pools tick on torch's current
        stream, where the writes already are.  (tick() and submit() must not be mixed on one pool.)"""
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    # -- the tick --------------------------------------------------------------------------------------
    def tick(self, chunks: torch.Tensor, present=None) -> torch.Tensor:
        if chunks.shape != (self.capacity, self.n):
            raise ValueError(f"expected chunks of shape {(self.capacity, self.n)}, got {tuple(chunks.shape)}")
        if (chunks.dtype == torch.int16) != (self.dtype == torch.int16):
            raise TypeError(f"this pool takes {self.dtype} chunks, got {chunks.dtype}")
        with torch.cuda.device(self.device):
            self.pcm.copy_(chunks, non_blocking=True)
            if present is not None:
                self.present.copy_(self._flags(present), non_blocking=True)
            self.tick_staged(masked=present is not None)
        return self.prob

    def _flags(self, present) -> torch.Tensor:
        f = torch.as_tensor(present)
        if f.shape != (self.capacity,):
            raise ValueError(f"expected {self.capacity} present flags, got shape {tuple(f.shape)}")
        return (f != 0).to(torch.uint8)

    def tick_staged(self, masked: bool = False):
        """One step over whatever `self.pcm` holds (for callers that write the staging buffer
        themselves, e.g. a device-side audio source); masked: only the rows flagged in `self.present`."""
        if self._graph is not None:
            if masked and self._graph_present is None:
                self._graph_present = False                # (asks _capture for the flagged graphs too)
                self._capture()
            elif self.engine.scratch_generation() != self._graph_gen:
                self._capture()                            # the engine's scratch moved: the old graph is stale
            (self._graph_present if masked else self._graph).replay()
        else:
            self._launch(masked)
        return self.prob

    # -- host to host ------------------------------------------------------------------------------------
    def submit(self, r: int = 0, present=None):
        """Start one tick over `host_pcm[r]` on the pool's stream; returns at once (see the class docstring).  present: flags of
        the streams that have a chunk in the slot (None = all; or True = `host_present[r]` as the sources left it)."""
        if not self.host_slots:
            raise RuntimeError("StreamPool was created without host_slots")
        masked = present is not None
        if masked and present is not True:
            self.host_present[r].copy_(self._flags(present))
        if self._use_graph:
            if masked and self._host_graphs_present is None:
                self._host_graphs_present = []
                self._capture()
            elif self.engine.scratch_generation() != self._graph_gen:
                self._capture()
            with torch.cuda.stream(self.stream):             # (replay launches on torch's current stream)
                (self._host_graphs_present if masked else self._host_graphs)[r].replay()
        else:       # one native call on the pool's stream: no stream switch on the host side
            self._host_tick(r, self.stream.cuda_stream, masked)
        self._done[r].record(self.stream)

    def wait(self, r: int = 0) -> torch.Tensor:
        """Block until the tick submitted for slot r has delivered; returns `host_prob[r]` (page-locked, overwritten by the
        slot's next tick)."""
        self._done[r].synchronize()
        return self.host_prob[r]

    def tick_host(self, r: int = 0) -> torch.Tensor:
        self.submit(r)
        return self.wait(r)


class BatchVADIterator:
    """`VADIterator` (src/silero_vad/utils_vad.py:458-549) for every slot of a lock-step batch.

    feed(probs[B]) advances all streams by one chunk and returns the list of events of this tick as
    (slot, {'start': n}) / (slot, {'end': n}) -- the same numbers the reference iterator emits for
    that stream (`current_sample` counts chunk ENDS, exit threshold fixed at threshold - 0.15,
    positions shifted back by one window, :526-547)."""

    def __init__(self, batch: int, threshold: float = 0.5, sampling_rate: int = 16000,
                 min_silence_duration_ms: int = 100, speech_pad_ms: int = 30):
        if sampling_rate not in (8000, 16000):
            raise ValueError("VADIterator does not support sampling rates other than [8000, 16000]")
        self.threshold = threshold
        self.sampling_rate = sampling_rate
        self.window = chunk_size(sampling_rate)
        self.min_silence_samples = sampling_rate * min_silence_duration_ms / 1000
        self.speech_pad_samples = sampling_rate * speech_pad_ms / 1000
        self.triggered = np.zeros(batch, dtype=bool)
        self.temp_end = np.zeros(batch, dtype=np.int64)
        self.current_sample = np.zeros(batch, dtype=np.int64)
        self._events = None

    def reset(self, slot=None):
        sl = slice(None) if slot is None else slot
        self.triggered[sl] = False
        self.temp_end[sl] = 0
        self.current_sample[sl] = 0

    def feed(self, probs, active=None):
        """One tick: probs[B] (host or device tensor / array) -> [(slot, {'start': n} | {'end': n}), ...] in slot order.  The
        per-stream logic runs in the native library (vad_iterator_feed, csrc/segmenter.cpp): one pass over the batch, no
        per-stream Python."""
        if torch.is_tensor(probs):
            probs = probs.detach().cpu().numpy()
        p = np.ascontiguousarray(probs, dtype=np.float32).reshape(-1)
        B = self.triggered.shape[0]
        if p.shape[0] != B:
            raise ValueError(f"expected {B} probabilities, got {p.shape[0]}")
        act = None if active is None else np.ascontiguousarray(active, dtype=np.bool_)
        if act is not None and act.shape[0] != B:
            raise ValueError(f"expected {B} active flags, got {act.shape[0]}")
        if self._events is None or len(self._events) < B:
            self._events = (_lib.IterEvent * B)()
        m = lib().vad_iterator_feed(p.ctypes.data, None if act is None else act.ctypes.data, B, self.window,
                                    float(self.threshold), float(self.min_silence_samples), float(self.speech_pad_samples),
                                    self.triggered.ctypes.data, self.temp_end.ctypes.data, self.current_sample.ctypes.data,
                                    self._events, B)
        if m < 0:
            raise ValueError("vad_iterator_feed: bad arguments")
        ev = self._events
        return [(ev[i].slot, {"end" if ev[i].kind else "start": ev[i].sample}) for i in range(m)]


# sample formats of a packet row (include/silero_vad_hip.h VAD_PCM_*): int16, G.711 mu-law (PCMU), G.711 A-law (PCMA), DVI4 (RFC 3551
# 4-bit IMA ADPCM: a 4-byte header, then two samples a byte -- the pump's coded packet and burst routes only)
_PCM = {"s16": 0, "ulaw": 1, "alaw": 2, "dvi4": 3}
_DVI4_HEADER = 4                                        # bytes in front of a DVI4 payload's codes


def _codec_id(codec, dvi4: bool = False) -> int:
    """A codec's name or number -> its number.  dvi4: "dvi4" / 3 is one of them -- on the packet routes of a pump with `adpcm=True`;
    everywhere else (the corpus routes, g711_expand, deinterleave, a pump without it) the codecs are the three they always were."""
    known = _PCM if dvi4 else {k: v for k, v in _PCM.items() if k != "dvi4"}
    if isinstance(codec, str):
        if codec not in known:
            raise ValueError(f"codec must be one of {sorted(known)}, got {codec!r}")
        return known[codec]
    if not isinstance(codec, (int, np.integer)) or int(codec) not in known.values():
        raise ValueError(f"codec must be one of {sorted(known)} or {sorted(known.values())}, got {codec!r}")
    return int(codec)


def _codec_rows(codecs, dvi4: bool = False) -> np.ndarray:
    """Per-row codecs as uint8: names are mapped here, numbers go to the pump as they are (it refuses a bad one)."""
    a = np.asarray(codecs)
    if a.ndim != 1:
        raise ValueError(f"codecs must be a 1-D sequence, got shape {a.shape}")
    if a.dtype.kind in "US":
        return np.array([_codec_id(str(c), dvi4) for c in a], np.uint8)
    if a.size and (not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() > 255):
        raise ValueError(f"codecs must be names or uint8 values, got {a.dtype}")
    return np.ascontiguousarray(a, dtype=np.uint8)


# the offset entry of a SILENT row (include/silero_vad_hip.h VAD_ROW_SILENT): lengths[i] samples of digital silence, no bytes in the slot
ROW_SILENT = -1


def _silent_len(x):
    """A write_* helper's row payload: None for a sample array, the row's length for an int (a silent row).  bool, 0, negative values
    and floats are refused: they are neither."""
    if isinstance(x, (bool, np.bool_, float, np.floating)):
        raise ValueError(f"a packet is a 1-D sample array, or an int >= 1 for a silent row of that many samples, got {x!r}")
    if not isinstance(x, (int, np.integer)):
        return None
    if x < 1:
        raise ValueError(f"a silent row holds at least 1 sample, got {x!r}")
    return int(x)


def _int32_rows(x, name) -> np.ndarray:
    a = np.asarray(x)
    if a.ndim != 1 or (a.size and (not np.issubdtype(a.dtype, np.integer) or a.min() < -2**31 or a.max() >= 2**31)):
        raise ValueError(f"{name} must be a 1-D sequence of int32 values, got {a.dtype} of shape {a.shape}")
    return np.ascontiguousarray(a, dtype=np.int32)


def _uint8_rows(x, name, what) -> np.ndarray:
    a = np.asarray(x)
    if a.ndim != 1 or (a.size and (not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() > 255)):
        raise ValueError(f"{name} must be a 1-D sequence of {what}, got {a.dtype} of shape {a.shape}")
    return np.ascontiguousarray(a, dtype=np.uint8)


def _coded_sizes(ln, cd):
    """Each row's bytes: 2 a sample (int16), 1 a sample (G.711), or a DVI4 payload's 4 + len / 2."""
    if cd is None:
        return ln * 2
    return np.where(cd == _PCM["dvi4"], _DVI4_HEADER + ln // 2, ln * np.where(cd == _PCM["s16"], 2, 1))


# The pump's packet routes, one row each; `StreamPump._submit_route` is the one builder behind the five submit_* methods.
#   entry    the C entry point: entry(pump, r, streams, offsets, lengths[, fourth column], n)
#   offsets  the name of the offset argument: "offsets" counts samples, "byte_offsets" bytes
#   align    what the default offsets round each row up to, in that unit
#   col4     the fourth column's name (None: the route has none) and `rows4`, its check and conversion to uint8
#   sizes    (lengths as int64, fourth column or None) -> each row's size in the offsets' unit
#   per      the word of the count message: one entry per ...
_Route = collections.namedtuple("_Route", "entry offsets align col4 rows4 sizes per")
_ROUTES = {
    "packets": _Route("vad_pump_submit_packets", "offsets", 8, None, None, lambda ln, _: ln, "packet"),
    "coded": _Route("vad_pump_submit_coded_packets", "byte_offsets", 16, "codecs", _codec_rows, _coded_sizes, "packet"),
    "burst": _Route("vad_pump_submit_burst", "byte_offsets", 16, "codecs", _codec_rows, _coded_sizes, "row"),
    "wide": _Route("vad_pump_submit_wide_packets", "byte_offsets", 16, "steps",
                   lambda x: _uint8_rows(x, "steps", "uint8 values"), lambda ln, _: ln * 2, "row"),
    "resampled": _Route("vad_pump_submit_resampled_packets", "byte_offsets", 16, "rates",
                        lambda x: _uint8_rows(x, "rates", "rate indices (uint8 values)"), lambda ln, _: ln * 2, "row"),
}

# What `StreamPump._pack` needs to know of a route that has a write_* method: the word its messages use for a row, the attribute that
# caps a row's length (None: any length >= 1), and what a row tuple's third element is (None: (stream, x) only; "codec": it picks the
# payload's dtype, int16 or uint8; "rate": one of resample_rates in Hz, refused in the first pass when it is not).
_Packer = collections.namedtuple("_Packer", "noun cap third")
_PACKERS = {
    "packets": _Packer("packet", "n", None),
    "coded": _Packer("packet", "n", "codec"),
    "burst": _Packer("packet", None, "codec"),
    "resampled": _Packer("row", "resample_row", "rate"),
}


def _pinned_view(ptr, ctype, shape) -> np.ndarray:
    """A numpy view of page-locked memory the pump owns: `ptr` as an array of `ctype` elements of `shape`."""
    return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=shape)


def g711_expand(data, codec) -> np.ndarray:
    """ITU-T G.711 codes -> int16 linear PCM (vad_g711_expand: the values of audioop.ulaw2lin / alaw2lin(x, 2), from the definition the
    pump's device expansion uses).  codec "ulaw" / "alaw" takes uint8 codes, "s16" int16 samples (returned as a copy).  Same shape.
    A G.711 stream for `model(chunk, 8000)` or `StreamPump.write_packets`: `g711_expand(payload, "ulaw")`."""
    c = _codec_id(codec)
    x = np.ascontiguousarray(data)
    want = np.int16 if c == _PCM["s16"] else np.uint8
    if x.dtype != want:
        raise ValueError(f"{codec!r} data must be {np.dtype(want).name}, got {x.dtype}")
    out = np.empty(x.shape, np.int16)
    rc = lib().vad_g711_expand(c, x.ctypes.data if x.size else None, x.size, out.ctypes.data if x.size else None)
    if rc:
        raise _lib.VadError(rc, "vad_g711_expand")
    return out


def adpcm_expand(payload) -> np.ndarray:
    """A DVI4 payload (RFC 3551 section 4.5.1, RTP payload types 5 / 6: uint8, the 4 header bytes {predict, index, reserved} included)
    -> its 2 * (len - 4) int16 samples (vad_adpcm_expand: the values of audioop.adpcm2lin(payload[4:], 2, (predict, min(index, 88))),
    from the single-code step the pump's device decoder uses).  A DVI4 stream for `StreamPump.write_packets`: `adpcm_expand(payload)`;
    `write_coded_packets(r, [(stream, payload, "dvi4")])` has the device do it.  There is no encoder in this package."""
    x = np.ascontiguousarray(payload)
    if x.dtype != np.uint8 or x.ndim != 1:
        raise ValueError(f"a DVI4 payload must be a 1-D uint8 array, got {x.dtype} of shape {x.shape}")
    if len(x) < _DVI4_HEADER:
        raise ValueError(f"a DVI4 payload holds at least its {_DVI4_HEADER} header bytes, got {len(x)}")
    out = np.empty(2 * (len(x) - _DVI4_HEADER), np.int16)
    n = lib().vad_adpcm_expand(x.ctypes.data, len(x), out.ctypes.data if out.size else None)
    if n < 0:
        raise _lib.VadError(int(-n), "vad_adpcm_expand")
    return out


def deinterleave(x, channels: int, channel: int, codec=None) -> np.ndarray:
    """Channel `channel` of a 1-D array of interleaved samples, as a WAV data chunk holds them, as int16 (vad_deinterleave, from the
    definition the device split uses): x[channel::channels] for int16 samples (codec None or "s16"), g711_expand(x[channel::channels])
    for uint8 codes with codec "ulaw" / "alaw".  What a corpus call with `channels=` computes is, by definition, what it computes on
    these."""
    c = _PCM["s16"] if codec is None else _codec_id(codec)
    x = np.ascontiguousarray(x)
    want = np.int16 if c == _PCM["s16"] else np.uint8
    if x.ndim != 1 or x.dtype != want:
        raise ValueError(f"{'s16' if codec is None else codec!r} data must be 1-D {np.dtype(want).name}, got {x.dtype} of shape {x.shape}")
    if isinstance(channels, (bool, np.bool_)) or not isinstance(channels, (int, np.integer)) or not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"channels must be 1 ... {MAX_CHANNELS}, got {channels!r}")
    if not 0 <= channel < channels:
        raise ValueError(f"channel must be 0 ... {channels - 1}, got {channel!r}")
    if x.size % channels:
        raise ValueError("an interleaved recording of 2 channels has an even number of samples")
    frames = x.size // channels
    out = np.empty(frames, np.int16)
    rc = lib().vad_deinterleave(c, int(channels), int(channel), x.ctypes.data if frames else None, frames, out.ctypes.data if frames else None)
    if rc != frames:
        raise _lib.VadError(-rc, "vad_deinterleave")
    return out


def decimate(x, step: int, phase: int = 0) -> np.ndarray:
    """The samples of a 1-D int16 piece that the reference's decimation x[::step] keeps (vad_decimate, from the definition the pump's
    device decimation uses): `phase` = the number of the stream's samples in front of x[0], modulo step, so the result is
    x[(-phase) % step::step] and the next piece's phase is (phase + len(x)) % step."""
    x = np.ascontiguousarray(x)
    if x.dtype != np.int16 or x.ndim != 1:
        raise ValueError(f"x must be a 1-D int16 array, got {x.dtype} of shape {x.shape}")
    if not isinstance(step, (int, np.integer)) or step < 1 or not isinstance(phase, (int, np.integer)) or not 0 <= phase < step:
        raise ValueError(f"step must be >= 1 and phase in 0 ... step - 1, got step {step!r}, phase {phase!r}")
    out = np.empty((len(x) + int(step) - 1) // int(step), np.int16)
    m = lib().vad_decimate(int(step), int(phase), x.ctypes.data if x.size else None, x.size, out.ctypes.data if out.size else None)
    if m < 0:
        raise _lib.VadError(-m, "vad_decimate")
    return out[:m]


def resample_geometry(orig_freq: int, new_freq: int):
    """(O, N, W, K) of the pair (vad_resample_geometry: O : N the reduced ratio, W the reference's filter half-width in input samples, K
    the taps of a phase's live run); ValueError for a pair that is not served -- new_freq 8000 or 16000, from another rate, O and N at
    most 1024, K at most 160."""
    v = [ctypes.c_int() for _ in range(4)]
    ok = all(isinstance(f, (int, np.integer)) and not isinstance(f, (bool, np.bool_)) and 0 < f < 2 ** 31 for f in (orig_freq, new_freq))
    if not ok or lib().vad_resample_geometry(int(orig_freq), int(new_freq), *[ctypes.byref(c) for c in v]):
        raise ValueError(f"resampling {orig_freq!r} -> {new_freq!r} Hz is not served: the target is 8000 or 16000, the source another rate "
                         "whose reduced ratio O : N has O, N <= 1024 and at most 160 taps a phase (88200 -> 8000 and 11025 -> 16000 are)")
    return tuple(c.value for c in v)


def resample_table(orig_freq: int, new_freq: int):
    """(taps float32 [N, K], first int32 [N]) of the pair (vad_resample_table): the table the device kernel and `resample` read."""
    _, N, _, K = resample_geometry(orig_freq, new_freq)
    taps, first = np.empty((N, K), np.float32), np.empty(N, np.int32)
    rc = lib().vad_resample_table(int(orig_freq), int(new_freq), taps.ctypes.data, first.ctypes.data)
    if rc:
        raise _lib.VadError(rc, "vad_resample_table")
    return taps, first


def resample(x, orig_freq: int, new_freq: int) -> np.ndarray:
    """A 1-D recording (int16 PCM, taken as x / 32768, or float) at orig_freq -> float32 at new_freq (8000 or 16000): what the reference's
    `read_audio` does to a file of another rate, torchaudio's default Resample (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99),
    as arithmetic: the polyphase table of vad_resample_table, every output accumulated in double and rounded once (vad_resample_host,
    the CPU twin of the device kernel) -- ceil(N len / O) samples.  Not torchaudio's bits: its float32 convolution differs in the
    last places.  The function and the pairs served: include/silero_vad_hip.h "resampling"."""
    resample_geometry(orig_freq, new_freq)
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    if x.ndim != 1:
        raise ValueError(f"x must be 1-D, got shape {x.shape}")
    x = np.ascontiguousarray(x, dtype=np.int16 if x.dtype == np.int16 else np.float32)
    out = np.empty(lib().vad_resample_length(int(orig_freq), int(new_freq), x.size), np.float32)
    rc = lib().vad_resample_host(int(orig_freq), int(new_freq), x.ctypes.data if x.size else None, x.itemsize, x.size,
                                 out.ctypes.data if out.size else None)
    if rc:
        raise _lib.VadError(rc, "vad_resample_host")
    return out


def resample_stream_ready(orig_freq: int, new_freq: int, n_in: int) -> int:
    """ready(n_in) of the streaming resampler (vad_resample_stream_ready): the outputs a stream that has received n_in input samples has
    emitted -- those whose K inputs have all arrived; nothing is zero-extended on the right, so `resample(x)[:ready(len(x))]` is what any
    cut of x into pieces yields.  Exact for any n_in below 2^62."""
    resample_geometry(orig_freq, new_freq)
    if isinstance(n_in, (bool, np.bool_)) or not isinstance(n_in, (int, np.integer)) or not 0 <= n_in < 2 ** 62:
        raise ValueError(f"n_in must be an integer in 0 ... 2^62 - 1, got {n_in!r}")
    m = lib().vad_resample_stream_ready(int(orig_freq), int(new_freq), int(n_in))
    if m < 0:
        raise _lib.VadError(-m, "vad_resample_stream_ready")
    return int(m)


def resample_stream_history(orig_freq: int, new_freq: int) -> int:
    """H of the pair (vad_resample_stream_history): the input samples a stream keeps between pieces, K - 1."""
    resample_geometry(orig_freq, new_freq)
    h = lib().vad_resample_stream_history(int(orig_freq), int(new_freq))
    if h < 0:
        raise _lib.VadError(-h, "vad_resample_stream_history")
    return int(h)


def resample_stream(x_new, orig_freq: int, new_freq: int, n_before: int, history):
    """One piece of a stream through the streaming resampler on the host (vad_resample_stream_host, the CPU twin of the pump's resampled
    rows): x_new = the piece, 1-D int16; n_before = the input samples the stream received before it; history = the last
    `resample_stream_history` of them, oldest first, zeros where the stream has not lived that long (all zeros in front of the first
    piece).  -> (outputs float32, the next piece's history int16): the outputs ready(n_before) ... ready(n_before + len(x_new)) - 1,
    bit for bit those `resample` gives for the whole signal."""
    H = resample_stream_history(orig_freq, new_freq)
    x = np.ascontiguousarray(x_new)
    hist = np.ascontiguousarray(history)
    if x.dtype != np.int16 or x.ndim != 1:
        raise ValueError(f"x_new must be a 1-D int16 array, got {x.dtype} of shape {x.shape}")
    if hist.dtype != np.int16 or hist.shape != (H,):
        raise ValueError(f"history must be an int16 array of {H} samples (resample_stream_history), got {hist.dtype} of shape {hist.shape}")
    n0 = resample_stream_ready(orig_freq, new_freq, n_before)
    out = np.empty(resample_stream_ready(orig_freq, new_freq, int(n_before) + x.size) - n0, np.float32)
    nxt = np.empty(H, np.int16)
    m = lib().vad_resample_stream_host(int(orig_freq), int(new_freq), int(n_before), hist.ctypes.data, x.ctypes.data if x.size else None, x.size,
                                       out.ctypes.data if out.size else None, nxt.ctypes.data)
    if m != out.size:
        raise _lib.VadError(-m if m < 0 else 0, "vad_resample_stream_host")
    return out, nxt


def resample_device(engine, x_dev: torch.Tensor, lens, orig_freq: int, new_freq: int, out: torch.Tensor = None) -> torch.Tensor:
    """`resample` on the device, for a padded batch: x_dev [rows, L] (or 1-D: one row, and a 1-D result) int16 or float32 on the
    engine's GPU at orig_freq; lens: the live samples of each row (a sequence, or an int64 tensor -- on the device or pinned --; None:
    L for every row).  -> float32 [rows, ceil(N L / O)] on the device (or `out`, float32 [rows, width_out] with unit sample stride,
    whatever it held): row r is its recording resampled, ceil(N lens[r] / O) samples, and exact zeros from there on.  The batch behind
    lens[r] is not read.  Enqueued on the current stream (vad_resample_rows_device); fp32 sums in tap order, the same bits for a
    recording in any row of any batch, each within (K + 1) 2^-24 sum |h x| of `resample`."""
    O, N, _, _ = resample_geometry(orig_freq, new_freq)
    x = x_dev if x_dev.dim() == 2 else x_dev.unsqueeze(0)
    if x_dev.dim() not in (1, 2) or not x.is_cuda or x.dtype not in (torch.int16, torch.float32):
        raise ValueError("x_dev must be a 1-D or 2-D int16 / float32 tensor on the GPU")
    if x.stride(1) != 1 and x.shape[1] > 1:
        x = x.contiguous()
    rows, L = x.shape
    if lens is None:
        lens = torch.full((rows,), L, dtype=torch.int64, device=x.device)
    elif not torch.is_tensor(lens):
        host = np.asarray(lens, dtype=np.int64).reshape(-1)
        if len(host) != rows or (len(host) and (host.min() < 0 or host.max() > L)):
            raise ValueError(f"lens needs one entry in 0 ... {L} per row")
        lens = torch.from_numpy(host).to(x.device)
    elif lens.dtype != torch.int64 or lens.numel() != rows or not (lens.is_cuda or lens.is_pinned()):
        raise ValueError("lens as a tensor is int64, one entry per row, on the device or in pinned memory")
    width = (L * N + O - 1) // O
    if out is None:
        out = torch.empty((rows, width), dtype=torch.float32, device=x.device)
    elif not out.is_cuda or out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != rows or (out.shape[1] > 1 and out.stride(1) != 1):
        raise ValueError("out must be a float32 [rows, width_out] tensor on the GPU with unit sample stride")
    if rows and out.shape[1]:
        engine.resample_rows(orig_freq, new_freq, x, lens.contiguous(), out.shape[1], out)
    return out[0] if x_dev.dim() == 1 else out


def _source_rate(source_rate, sampling_rate):
    """The `source_rate=` of a corpus call, checked: -> None (the recordings are at `sampling_rate`: the call is today's) or (O, N), the
    reduced ratio of the resample in front of the net.  With a source rate, `sampling_rate` is the NET's rate, 8000 or 16000."""
    if source_rate is None or source_rate == sampling_rate:
        return None
    if sampling_rate not in (8000, 16000):
        raise ValueError(f"source_rate={source_rate!r}: sampling_rate is then the net's rate, 8000 or 16000, got {sampling_rate!r}")
    try:
        return resample_geometry(source_rate, sampling_rate)[:2]
    except ValueError as e:
        raise ValueError(f"source_rate={source_rate!r}: {e}") from None


def _no_source_rate(source_rate, who):
    """the corpus and stream routes that do not resample say so"""
    if source_rate is not None:
        raise ValueError(f"{who}: source_rate= is not served here -- resampling in front of the net is a route of ragged_buckets / "
                         "ragged_reserve / ragged_probs / ragged_speech_segments (or `resample` the recordings first)")


def _blob_bytes(blob) -> np.ndarray:
    a = np.asarray(blob)
    if a.dtype != np.uint8 or a.ndim != 1:
        raise ValueError(f"a snapshot blob is a 1-D uint8 array, got {a.dtype} of shape {a.shape}")
    return np.ascontiguousarray(a)


def _distinct_slots(x, name) -> np.ndarray:
    a = _int32_rows(x, name)
    if len(np.unique(a)) != len(a):
        raise ValueError(f"{name} lists a slot twice")
    return a


_SNAPSHOT_HISTORY = 160                                    # VAD_SNAPSHOT_HISTORY: the int16 history of a record's tail
_SnapshotLayout = collections.namedtuple("_SnapshotLayout", "version header_bytes sr N C stride n_records tape_elem tape_at "
                                                             "info h c ctx pending resample carry history tape")


def _snapshot_layout(a: np.ndarray) -> _SnapshotLayout:
    """The header of a blob the library HAS validated (include/silero_vad_hip.h "SNAPSHOT AND RESTORE"; the layout is snap_layout's of
    csrc/pump.hip), and the parts of a record as slices of its bytes: `resample`, `carry`, `history` (version 2 on) and `tape` (version 3)
    are None in a blob without them.  tape_elem: the element of the tape section in bytes (0: none); tape_at: where it starts in the blob."""
    version, head = (int(v) for v in a[8:16].view("<u4"))
    sr, N, C = (int(v) for v in a[16:28].view("<i4"))
    stride, n = int(a[28:32].view("<u4")[0]), int(a[32:40].view("<i8")[0])
    cuts = np.cumsum([0, ctypes.sizeof(_lib.StreamInfo), 4 * 128, 4 * 128, 4 * C, 2 * N] +
                     ([ctypes.sizeof(_lib.ResampleInfo), 4 * N, 2 * _SNAPSHOT_HISTORY] if version >= 2 else []) +
                     ([ctypes.sizeof(_lib.TapeInfo)] if version >= 3 else [])).tolist()
    parts = [slice(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    return _SnapshotLayout(version, head, sr, N, C, stride, n, int(a[64:68].view("<i4")[0]) if version >= 3 else 0, head + n * stride,
                           *(parts + [None] * (9 - len(parts))))


def snapshot_info(blob) -> list:
    """The records of a snapshot blob (`StreamPump.export_streams`), host only (vad_snapshot_inspect validates it, once): per record a
    dict of the vad_stream_info fields (`active`, `triggered`, `temp_end`, `current_sample`, `pending`, `wide_step`, `wide_phase`) plus
    `h` [128], `c` [128], `ctx` [C] float32 and `pending_samples` [N] int16 (zeros behind `pending`).  A record of a version 2 blob
    (`export_streams(version=2)`) has a `resample` entry besides (what vad_snapshot_resample reads): a dict of `src_rate` (Hz; 0 = bound to no
    rate), `pending_out`, `inputs_mod`, `outputs_mod`, `carry` (the pending_out fp32 outputs that wait for their chunk) and `history`
    (the last H int16 inputs at src_rate, oldest first).  A record of a version 3 blob (`export_streams_v3`) has that entry and a
    `tape` entry (what vad_snapshot_tape reads): a dict of `first_chunk`, `n_chunks`, `offset` (of the run in the blob's tape section, in
    bytes), `elem` (the tape's element in bytes: 0, 2 or 4) and `audio`, the run's n_chunks * N samples as int16 or float32 (empty int16
    without a run).  A blob the library refuses -- bad magic or version, truncated, a field out of range -- raises."""
    a = _blob_bytes(blob)
    L = lib()
    rc = L.vad_snapshot_inspect(a.ctypes.data if a.size else None, a.size, None, None)
    if rc:
        raise _lib.VadError(rc, "vad_snapshot_inspect: not a valid snapshot blob")
    # The library has validated the WHOLE blob, once; the records are then read here from the documented layout.  (vad_snapshot_stream /
    # vad_snapshot_resample validate the whole blob again on every call, as a C caller that reads one record wants: a loop over them
    # would be quadratic in the blob, and a whole pump's version 2 blob is 39 MB.)
    at = _snapshot_layout(a)
    H_of = {0: 0}
    out = []
    for i in range(at.n_records):
        rec = a[at.header_bytes + i * at.stride:at.header_bytes + (i + 1) * at.stride]
        f = _lib.StreamInfo.from_buffer_copy(rec[at.info].tobytes())
        d = {k: int(getattr(f, k)) for k in ("active", "triggered", "temp_end", "current_sample", "pending", "wide_step", "wide_phase")}
        d.update(h=rec[at.h].view("<f4").copy(), c=rec[at.c].view("<f4").copy(), ctx=rec[at.ctx].view("<f4").copy(),
                 pending_samples=rec[at.pending].view("<i2").copy())
        if at.resample:
            q = _lib.ResampleInfo.from_buffer_copy(rec[at.resample].tobytes())
            if q.src_rate not in H_of:
                H_of[q.src_rate] = L.vad_resample_stream_history(q.src_rate, at.sr)
            d["resample"] = dict(src_rate=int(q.src_rate), pending_out=int(q.pending_out), inputs_mod=int(q.inputs_mod), outputs_mod=int(q.outputs_mod),
                                 carry=rec[at.carry].view("<f4")[:q.pending_out].copy(), history=rec[at.history].view("<i2")[:H_of[q.src_rate]].copy())
        if at.tape:
            t = _lib.TapeInfo.from_buffer_copy(rec[at.tape].tobytes())
            run = a[at.tape_at + int(t.offset):at.tape_at + int(t.offset) + int(t.n_chunks) * at.N * at.tape_elem]
            d["tape"] = dict(first_chunk=int(t.first_chunk), n_chunks=int(t.n_chunks), offset=int(t.offset), elem=at.tape_elem,
                             audio=run.view("<f4" if at.tape_elem == 4 else "<i2").copy())
        out.append(d)
    return out


def snapshot_tape(blob, i: int) -> np.ndarray:
    """The run of the tape that record i of a snapshot blob carries (vad_snapshot_tape; host only): its n_chunks * N samples, oldest first,
    as int16 or float32 -- the element of the tape of the pump that wrote the blob.  Empty (int16) for a record without a run and for a
    blob of version 1 or 2.  The samples are those [first_chunk * N, current_sample) of the stream's clock (`snapshot_info(blob)[i]["tape"]`
    has the numbers).  An invalid blob or i out of range raises."""
    a = _blob_bytes(blob)
    L = lib()
    t = _lib.TapeInfo()
    rc = L.vad_snapshot_tape(a.ctypes.data if a.size else None, a.size, int(i), ctypes.byref(t), None, 0)
    if rc:
        raise _lib.VadError(rc, "vad_snapshot_tape: not a valid snapshot blob, or no such record")
    at = _snapshot_layout(a)
    out = np.empty(int(t.n_chunks) * at.N, np.float32 if t.n_chunks and at.tape_elem == 4 else np.int16)
    if out.size:
        rc = L.vad_snapshot_tape(a.ctypes.data, a.size, int(i), None, out.ctypes.data, out.nbytes)
        if rc:
            raise _lib.VadError(rc, "vad_snapshot_tape")
    return out


def tape_run(count: int, floor: int, chunks: int, n: int, start: int):
    """(first_chunk, n_chunks): the whole chunks a version 3 snapshot carries of a stream whose tape, `chunks` chunks of n samples, has the
    counters (count, floor), when its audio is wanted from sample `start` on -- held_lo = max(floor, count - chunks), first_chunk =
    min(max(start // n, held_lo), count) with `start` clamped into the held window first, n_chunks = count - first_chunk (vad_tape_run:
    the rule `StreamPump.export_streams_v3(tape_from=...)` applies; host only, no GPU).  Any int64 `start` is legal."""
    vals = [count, floor, chunks, n, start]
    if any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in vals):
        raise ValueError(f"tape_run takes integers, got {vals!r}")
    if not all(-2 ** 63 <= int(v) < 2 ** 63 for v in vals) or not all(-2 ** 31 <= int(v) < 2 ** 31 for v in (chunks, n)):
        raise ValueError(f"tape_run: a value out of its integer range in {vals!r}")
    first, m = ctypes.c_int64(), ctypes.c_int64()
    rc = lib().vad_tape_run(int(count), int(floor), int(chunks), int(n), int(start), ctypes.byref(first), ctypes.byref(m))
    if rc:
        raise ValueError(f"tape_run: chunks >= 2, n >= 1, count >= 0, floor >= 0 and counters times n within int64, got {vals!r}")
    return first.value, m.value


def tape_window(count: int, floor: int, chunks: int, n: int, start: int, end: int):
    """(first, samples): the part of the sample range [start, end) that a tape of `chunks` chunks of n samples holds when the stream's
    counters are (count, floor) -- held_lo = max(floor, count - chunks) * n, held_hi = count * n, first = min(max(start, held_lo),
    held_hi), last = min(max(end, first), held_hi) (vad_tape_window: the rule `StreamPump.fetch_audio` applies; host only, no GPU).
    Any int64 start <= end is legal; start > end raises."""
    vals = [count, floor, chunks, n, start, end]
    if any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in vals):
        raise ValueError(f"tape_window takes integers, got {vals!r}")
    if not all(-2 ** 63 <= int(v) < 2 ** 63 for v in vals) or not all(-2 ** 31 <= int(v) < 2 ** 31 for v in (chunks, n)):
        raise ValueError(f"tape_window: a value out of its integer range in {vals!r}")
    if start > end:
        raise ValueError(f"tape_window: start {start} lies behind end {end}")
    first, m = ctypes.c_int64(), ctypes.c_int64()
    rc = lib().vad_tape_window(int(count), int(floor), int(chunks), int(n), int(start), int(end), ctypes.byref(first), ctypes.byref(m))
    if rc:
        raise ValueError(f"tape_window: chunks >= 2, n >= 1, count >= 0 and counters times n within int64, got {vals!r}")
    return first.value, m.value


def _tape_dtype(dtype) -> np.dtype:
    """The tape's element, int16 or float32, from anything np.dtype() takes; anything else raises (before any native call)."""
    try:
        dt = np.dtype(dtype)
    except TypeError:
        dt = None
    if dt is None or dtype is None or dt not in (np.dtype(np.int16), np.dtype(np.float32)):
        raise ValueError(f"tape_dtype must be int16 or float32, got {dtype!r}")
    return dt


class UtteranceCollector:
    """The utterances behind a taped pump's events: `feed(events)` takes what `pump.poll()` returned, remembers each stream's `start`
    and returns, for every `end`, (stream, start, end, first, audio) -- audio the samples [first, end) of the stream as the net heard
    them, in the tape's dtype (int16, or float32 in [-1, 1) with `tape_dtype="float32"`, the only tape of the resampled route),
    first > start where the head of a long utterance had already left the tape.  All ENDs of one `feed` are fetched in
    one `fetch_audio` call.  An END whose START was never fed comes back as (stream, None, end, None, None).  `forget(stream)` drops a
    remembered START: call it with `pump.open_stream(stream)`, the slot's new stream starts a new clock.
    Streams that migrate in the middle of an utterance take their START along: `open_starts(streams)` -> {stream: start} of the streams
    that are inside one, for `export_streams_v3(tape_from=...)` and for the destination's collector, which `adopt(stream, start)`
    tells where the utterance of the stream in ITS slot began (`StreamPump.export_streams_v3` shows the whole move)."""

    def __init__(self, pump):
        if not getattr(pump, "tape_chunks", 0):
            raise ValueError("UtteranceCollector needs a pump with a tape (StreamPump(..., tape_chunks=K))")
        self.pump = pump
        self._start = {}

    def forget(self, stream: int):
        self._start.pop(int(stream), None)

    def open_starts(self, streams=None) -> dict:
        """{stream: start} of the remembered STARTs -- the streams that are inside an utterance -- of `streams` (None: of every stream)."""
        if streams is None:
            return dict(self._start)
        return {int(b): self._start[int(b)] for b in streams if int(b) in self._start}

    def adopt(self, stream: int, start: int):
        """Remember `start` as the START of the utterance the stream in slot `stream` is in, as if its event had been fed here: the stream
        was imported in the middle of that utterance (its clock, and so the sample number, came along)."""
        if isinstance(start, (bool, np.bool_)) or not isinstance(start, (int, np.integer)) or start < 0:
            raise ValueError(f"start is a sample number of the stream's clock, got {start!r}")
        self._start[int(stream)] = int(start)

    def feed(self, events) -> list:
        done = []
        for stream, ev in events or ():
            if "start" in ev:
                self._start[int(stream)] = int(ev["start"])
            else:
                done.append((int(stream), self._start.pop(int(stream), None), int(ev["end"])))
        known = [d for d in done if d[1] is not None]
        audios, first = ([], []) if not known else self.pump.fetch_audio([d[0] for d in known], [d[1] for d in known], [d[2] for d in known])
        got = iter(zip(audios, first))
        out = []
        for stream, start, end in done:
            if start is None:
                out.append((stream, None, end, None, None))
            else:
                audio, f = next(got)
                out.append((stream, start, end, int(f), audio))
        return out


class StreamPump:
    """BASELINE configs[4] through the native pump (include/silero_vad_hip.h "live streams: the pump", csrc/pump.hip): `streams`
    live streams on one GPU, host int16 chunks in, VADIterator events out, with no Python and no torch on the per-tick path
    (the reference's native streaming loop, examples/cpp/silero-vad-onnx.cpp:335-390, for thousands of streams in lock step).

        pump = StreamPump(engine, 16000, streams=8192)
        pump.slot(r)[b] = next int16 chunk of stream b          # numpy view of the page-locked ingest ring, [streams, N]
        pump.submit(r)                                           # asynchronous: H2D -> step kernels -> probabilities on the host
        events, r = pump.poll()                                  # retire the oldest tick: [(stream, {'start' | 'end': sample}), ...]
        pump.probs(r)                                            # its probabilities, [streams] float32 (page-locked)

    Streams that arrive in 10 / 20 / 30 ms packets: `pump.write_packets(r, [(stream, int16 packet), ...])` (or the packets written
    into `packet_area(r)` + `submit_packets(r, streams, lengths, offsets)`); the device cuts each stream's concatenated packets into
    chunks, and `pending(stream)` says how many samples wait for the next one.  Time without a payload (a lost packet, DTX, a
    comfort-noise period) is a SILENT row: `(stream, 160)` in a `write_*` list, or `ROW_SILENT` as the row's offset -- that many zero
    samples of the stream, no bytes written or sent; a stream listed in no row is absent (late) and stands still instead.  G.711 (PCMU / PCMA) packets go in as they came off
    the wire, 1 byte a sample: `pump.write_coded_packets(r, [(stream, packet, "ulaw" | "alaw" | "s16"), ...])` (or `packet_bytes(r)` +
    `submit_coded_packets(...)`); the device expands them.  With `adpcm=True` the same two routes and bursts also take DVI4 payloads
    (RFC 3551 4-bit IMA ADPCM, header included: `(stream, payload, "dvi4")`), decoded on the device.  With `max_burst=M` (2 ... 8) a tick may be a BURST:
    `pump.write_burst(r, [(stream, packet[, codec]), ...])` takes any number of packets of one stream and packets longer than a chunk (a
    60 ms Opus frame, what a jitter buffer releases after a stall); a stream that completes k <= M chunks is stepped k times inside the
    tick, `burst_steps(r)` / `burst_probs(r)` give the sub-steps, and `poll` returns their events one sub-step after the other.

    32 / 48 kHz clients (WebRTC, Opus decoders): after `pump.set_wideband(3)` the rows of `wide_slot(r)` +
    `submit_wide_packets(r, streams, lengths, steps)` are int16 samples at steps[i] x 16 kHz, and the device keeps every steps[i]-th one
    (the reference's `x[::step]`); the pump carries each stream's comb phase (`wide_phase(stream)`), events count 16 kHz samples.

    44.1 / 24 / 22.05 / 11.025 kHz clients (voice-agent and speech-synthesis APIs, desktop and browser capture), or 48 kHz with
    `read_audio`'s low-pass: after `pump.set_resample((44100, 24000))` the rows of `resample_slot(r)` + `submit_resampled_packets(r,
    streams, lengths, rates)` (or `write_resampled_packets(r, [(stream, int16 samples, 44100), ...])`) are int16 samples at those rates
    and the device resamples them per stream -- `resample_device`'s bits for the concatenated rows, whatever the packetisation; the pump
    carries each stream's filter history and fp32 pending outputs (`resample_state(stream)`, `pending(stream)`).

    Moving live streams (a drain, a rebalancing between per-GPU ranks, a restart): with no tick in flight `blob = pump.export_streams([3, 7])`
    packs everything those streams carry into one uint8 array, `other.import_streams(blob, [0, 5])` puts the records into slots of any
    pump of the same sample rate (another GPU, another process), and `snapshot_info(blob)` reads a blob without a pump; the streams go
    on bit for bit.  `export_streams(..., version=2)` also moves streams that are bound to a resampled rate, and
    `export_streams_v3(..., tape_from=...)` also the taped audio of the utterances they are in (below).

    The audio behind the events: with `tape_chunks=K` the pump keeps every stream's last K chunks on the device as the net heard them
    (G.711 expanded, 32 / 48 kHz combed, silent rows as zeros), taped as a side effect of every step of every route but the resampled
    one; the sample numbers of the events are tape positions, `fetch_audio(streams, starts, ends)` copies any still-held ranges out
    (to numpy arrays, or with device=True into one packed tensor on the pump's GPU) and `UtteranceCollector(pump).feed(events)` hands
    back the utterance behind every `end`.  A sample stays fetchable for K chunks of its stream (ticks in flight count):
    K = longest utterance + pad + ring_slots x max_burst; the tape costs streams x K x N x 2 bytes.  With `tape_dtype="float32"` the
    tape holds what the net read, float32 in [-1, 1) (x / 32768 of an int16 sample, exact), at 4 bytes a sample: it also tapes the
    resampled route, bit for bit `resample_device` of what the stream was fed, and goes together with `set_resample`; utterances come
    out as float32, on the device if wanted, the form a model on the same GPU takes.  `tape_dtype` says which tape the pump has.

    `play(rows, ...)` runs the whole loop natively over memory-resident recordings (tests, benchmarks, file-fed servers)."""

    def __init__(self, engine, sampling_rate: int = 16000, streams: int = 8192, parts: int = 0, ring_slots: int = 0,
                 threshold: float = 0.5, min_silence_duration_ms: int = 100, speech_pad_ms: int = 30, max_burst: int = 1, source_rate=None,
                 tape_chunks: int = 0, tape_dtype="int16", adpcm: bool = False):
        _no_source_rate(source_rate, "StreamPump")
        if isinstance(tape_chunks, (bool, np.bool_)) or not isinstance(tape_chunks, (int, np.integer)) or tape_chunks < 0 or tape_chunks == 1 \
                or tape_chunks >= 2 ** 31:
            raise ValueError(f"tape_chunks must be 0 (no tape) or 2 ... 2^31 - 1 chunks a stream, got {tape_chunks!r}")
        tape_dtype = _tape_dtype(tape_dtype)                     # (with tape_chunks == 0 it is only validated)
        if sampling_rate not in (8000, 16000):
            raise ValueError("VADIterator does not support sampling rates other than [8000, 16000]")
        if not isinstance(max_burst, (int, np.integer)) or not 1 <= max_burst <= 8:
            raise ValueError(f"max_burst must be 1 ... 8 (VAD_PUMP_MAX_BURST), got {max_burst!r}")
        self._L = engine._L
        prm = _lib.PumpParams()
        self._L.vad_pump_params_default(ctypes.byref(prm), int(sampling_rate), int(streams))
        prm.parts, prm.ring_slots = int(parts), int(ring_slots)
        prm.threshold, prm.min_silence_duration_ms, prm.speech_pad_ms = float(threshold), int(min_silence_duration_ms), int(speech_pad_ms)
        h = ctypes.c_void_p()
        rc = self._L.vad_pump_create(engine._h, ctypes.byref(prm), ctypes.byref(h))
        if rc:
            raise _lib.VadError(rc, "vad_pump_create")
        self._h = h
        g = [ctypes.c_int() for _ in range(4)]
        self._L.vad_pump_geometry(h, *[ctypes.byref(x) for x in g])
        self.streams, self.n, self.ring_slots, self.parts = (x.value for x in g)
        self.sr = int(sampling_rate)
        self.max_burst = int(max_burst)
        if self.max_burst > 1:                                   # (1: burst ticks stay off, nothing is allocated for them)
            rc = self._L.vad_pump_set_burst(h, self.max_burst)
            if rc:
                msg = self._L.vad_pump_last_error(h).decode()
                self._L.vad_pump_destroy(h)
                self._h = None
                raise _lib.VadError(rc, msg)
        self.adpcm = False
        if adpcm:                                                # (off: codec 3 stays the bad codec it was)
            try:
                self.set_adpcm(True)
            except Exception:
                self._L.vad_pump_destroy(h)
                self._h = None
                raise
        self.tape_chunks = 0
        self.tape_dtype = None
        self.device = getattr(engine, "device", 0)
        if tape_chunks:                                          # (0: no tape, nothing is allocated or launched for it)
            try:
                self.set_tape(int(tape_chunks), tape_dtype)
            except Exception:
                self._L.vad_pump_destroy(h)
                self._h = None
                raise
        self._events = (_lib.IterEvent * (self.streams * self.max_burst))()
        ring = range(self.ring_slots)
        self._slots = [_pinned_view(self._L.vad_pump_slot(h, r), ctypes.c_int16, (self.streams, self.n)) for r in ring]
        self._probs = [_pinned_view(self._L.vad_pump_probs(h, r), ctypes.c_float, (self.streams,)) for r in ring]
        self._present = [_pinned_view(self._L.vad_pump_present(h, r), ctypes.c_uint8, (self.streams,)) for r in ring]
        # sub-steps 1 ... max_burst - 1 of a burst tick: per ring slot [max_burst - 1, streams] (page-locked, one block per slot)
        self._probs_more = [_pinned_view(self._L.vad_pump_burst_probs(h, r, 1), ctypes.c_float, (self.max_burst - 1, self.streams))
                            for r in ring] if self.max_burst > 1 else None

    def close(self):
        if getattr(self, "_h", None):
            self._slots = self._probs = self._present = self._probs_more = self._wide = self._res = None
            self._L.vad_pump_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        if rc:
            raise _lib.VadError(rc, self._L.vad_pump_last_error(self._h).decode())

    def slot(self, r: int) -> np.ndarray:
        return self._slots[r]

    def probs(self, r: int) -> np.ndarray:
        return self._probs[r]

    def present(self, r: int) -> np.ndarray:
        """Slot r's flag row, [streams] uint8 (page-locked, in front of the slot's audio): 0 = the stream has no chunk this tick."""
        return self._present[r]

    def submit(self, r: int, present=None, compact: bool = False):
        """Start the tick over ring slot r.  present: None = every stream has a chunk; True = the flags the sources wrote into
        `present(r)`; an array of `streams` flags = copied there.  A stream whose flag is 0 is not stepped: its (h, c), context and
        iterator counters stay as they are and `probs(r)[b]` reads -1.0 (vad_pump_submit_present).
        compact=True (vad_pump_submit_compact): `slot(r)` holds only the delivering streams' chunks, back to back -- row i is the chunk
        of the i-th stream whose flag is set -- and only those rows cross the link; same results, bit for bit."""
        if compact and present is None:
            raise ValueError("a compact tick needs its present flags")
        if present is None:
            self._check(self._L.vad_pump_submit(self._h, int(r)))
            return
        if present is not True:
            f = np.asarray(present)
            if f.shape != (self.streams,):
                raise ValueError(f"expected {self.streams} present flags, got shape {f.shape}")
            self._present[r][:] = f != 0
        fn = self._L.vad_pump_submit_compact if compact else self._L.vad_pump_submit_present
        self._check(fn(self._h, int(r), self._present[r].ctypes.data))

    def submit_rows(self, r: int, stream_of_row):
        """A compact tick in ARRIVAL order (vad_pump_submit_rows): row i of `slot(r)` holds the chunk of stream `stream_of_row[i]`; every
        other stream is absent this tick.  A stream listed twice, or out of range, raises and queues nothing."""
        rows = np.ascontiguousarray(stream_of_row, dtype=np.int32).reshape(-1)
        self._check(self._L.vad_pump_submit_rows(self._h, int(r), rows.ctypes.data if len(rows) else None, len(rows)))

    def packet_area(self, r: int) -> np.ndarray:
        """Slot r's sample area as one flat int16 array of streams * N samples (page-locked): where a packet tick's packets go."""
        return self._slots[r].reshape(-1)

    def submit_packets(self, r: int, streams, lengths, offsets=None):
        """A PACKET tick (vad_pump_submit_packets): row i of `packet_area(r)` holds lengths[i] samples (1 ... N) of stream streams[i]
        at sample offset offsets[i] (a multiple of 8; None = the rows back to back, each rounded up to 8 samples).  Each stream's
        packets are appended to what it has pending; a stream whose pending samples reach N is stepped on the first N of them, every
        other stream is absent this tick.  A stream listed twice or out of range, a bad length or offset raises and queues nothing.
        offsets[i] == ROW_SILENT (-1): a SILENT row -- lengths[i] samples of digital silence, no bytes of the area, exempt from the
        alignment and fit checks, a row in every other respect; results are those of a row of int16 zeros.  Every other negative
        offset is refused.  With offsets=None every row has a payload."""
        self._submit_route("packets", r, streams, lengths, offsets)

    def _submit_route(self, route, r, streams, lengths, offsets, col4=None):
        """The row columns of a packet tick, for every route of `_ROUTES`: converted and checked, one entry per row, the default
        offsets (the rows back to back, each rounded up to the route's alignment) filled in, and handed to the route's C entry."""
        rt = _ROUTES[route]
        st, ln = _int32_rows(streams, "streams"), _int32_rows(lengths, "lengths")
        off = None if offsets is None else _int32_rows(offsets, rt.offsets)
        c4 = None if col4 is None else _codec_rows(col4, getattr(self, "adpcm", False)) if rt.rows4 is _codec_rows else rt.rows4(col4)
        n = len(st)
        if len(ln) != n or (off is not None and len(off) != n) or (c4 is not None and len(c4) != n):
            names = ["streams", "lengths"] + [rt.col4] * (rt.col4 is not None)
            counts = [n, len(ln)] + [n if c4 is None else len(c4)] * (rt.col4 is not None) + [n if off is None else len(off)]
            raise ValueError(f"{', '.join(names)} and {rt.offsets} must have one entry per {rt.per}, got {', '.join(map(str, counts))}")
        if off is None:
            off = np.zeros(n, np.int32)
            if n:
                sizes = rt.sizes(ln[:-1].astype(np.int64), None if c4 is None else c4[:-1])
                off[1:] = np.cumsum((sizes + (rt.align - 1)) // rt.align * rt.align)
        cols = (st, off, ln) if rt.col4 is None else (st, off, ln, c4)
        ptrs = [x.ctypes.data if n and x is not None else None for x in cols]
        self._check(getattr(self._L, rt.entry)(self._h, int(r), *ptrs, n))

    def _pack(self, route, area, packets, default=None):
        """The rows of a write_* method, for every route of `_PACKERS`: the payloads copied into `area` back to back, each rounded up to
        16 bytes (8 samples of an int16 area), and the columns -> (streams, lengths, codecs or rate indices as uint8 or None, offsets
        in the area's elements).  default: the third element of a row tuple that has none (None: the route's tuples are complete)."""
        pk = _PACKERS[route]
        cap = pk.cap and getattr(self, pk.cap)
        packets = list(packets)

        def rows():
            for row in packets:
                if pk.third is None:
                    s, x = row
                    yield s, x, None
                elif default is None:
                    s, x, t = row
                    yield s, x, t
                else:
                    yield row if len(row) == 3 else (row[0], row[1], default)

        too_long = f"a {pk.noun} holds 1 ... {cap} samples, got {{}} (submit a longer one over two ticks)"
        for _, x, t in rows():                                   # (the rates and the silent rows first: nothing is written when one is bad)
            if pk.third == "rate" and t not in self.resample_rates:
                raise ValueError(f"rate {t!r} is none of the pump's resample_rates {self.resample_rates}")
            n = _silent_len(x)
            if n is not None and cap and n > cap:
                raise ValueError(too_long.format(n))
        align = 16 // area.itemsize
        streams, lengths, thirds, offsets, at = [], [], [], [], 0
        for s, x, t in rows():
            c = _codec_id(t, getattr(self, "adpcm", False)) if pk.third == "codec" else self.resample_rates.index(t) if pk.third == "rate" else None
            streams.append(s)
            thirds.append(c)
            if _silent_len(x) is not None:
                lengths.append(int(x))
                offsets.append(ROW_SILENT)
                continue
            x = np.asarray(x)
            want = np.uint8 if pk.third == "codec" and c != _PCM["s16"] else np.int16
            if x.dtype != want or x.ndim != 1:
                raise ValueError(f"a {t!r} packet must be a 1-D {np.dtype(want).name} array, got {x.dtype} of shape {x.shape}"
                                 if pk.third == "codec" else f"a {pk.noun} must be a 1-D int16 array")
            n = len(x)                                           # the row's samples
            if pk.third == "codec" and c == _PCM["dvi4"]:        # (the payload's header is no sample; two samples a byte behind it)
                if n <= _DVI4_HEADER:
                    raise ValueError(f"a 'dvi4' packet is its {_DVI4_HEADER} header bytes and at least 1 byte of codes, got {n} bytes")
                n = 2 * (n - _DVI4_HEADER)
            if n < 1 or (cap and n > cap):
                raise ValueError(too_long.format(n) if cap else "a packet holds at least 1 sample")
            size = x.nbytes // area.itemsize
            if at + size > len(area):
                raise ValueError(f"the {pk.noun}s do not fit into the slot")
            area[at:at + size] = x.view(area.dtype)
            lengths.append(n)
            offsets.append(at)
            at += (size + align - 1) // align * align
        return streams, lengths, None if pk.third is None else np.array(thirds, np.uint8), offsets

    def write_packets(self, r: int, packets):
        """Pack [(stream, int16 samples), ...] back to back (each rounded up to 8 samples) into `packet_area(r)` and submit the packet
        tick -- the convenience form for tests and small servers.  An int in place of the samples, `(stream, 160)`, is a silent row of
        that many samples (1 ... N): it takes no room in the area and advances no offset."""
        streams, lengths, _, offsets = self._pack("packets", self.packet_area(r), packets)
        self.submit_packets(r, streams, lengths, offsets)

    def packet_bytes(self, r: int) -> np.ndarray:
        """Slot r's sample area as one flat uint8 array of streams * N * 2 bytes (page-locked): where a coded packet tick's rows go."""
        return self._slots[r].reshape(-1).view(np.uint8)

    def submit_coded_packets(self, r: int, streams, lengths, codecs, byte_offsets=None):
        """A packet tick whose rows may be G.711 (vad_pump_submit_coded_packets): row i of `packet_bytes(r)` holds lengths[i] samples
        (1 ... N) of stream streams[i] in format codecs[i] -- "s16" (2 bytes a sample), "ulaw" or "alaw" (1 byte), or the VAD_PCM_*
        numbers; None = every row "s16" -- at byte offset byte_offsets[i] (a multiple of 16; None = the rows back to back, each
        rounded up to 16 bytes).  The device expands G.711 to int16: the same results, bit for bit, as `submit_packets` with the rows
        expanded by `g711_expand`.  A bad codec, stream, length or offset raises and queues nothing.
        byte_offsets[i] == ROW_SILENT (-1): a SILENT row of lengths[i] int16 zeros (see `submit_packets`); its codecs[i] is not looked
        at by the pump.  With byte_offsets=None every row has a payload.
        codecs[i] == "dvi4" (RFC 3551 4-bit IMA ADPCM; on a pump with `adpcm=True` / `set_adpcm()`): the row is the RTP payload, header included -- 4 + lengths[i] / 2 bytes for
        an even lengths[i] of 2 ... N SAMPLES; the device decodes it, with the results of the row `adpcm_expand`ed.  An odd length
        raises."""
        self._submit_route("coded", r, streams, lengths, byte_offsets, codecs)

    def write_coded_packets(self, r: int, packets):
        """Pack [(stream, samples, codec), ...] back to back (each rounded up to 16 bytes) into `packet_bytes(r)` and submit the tick:
        codec "s16" takes an int16 array, "ulaw" / "alaw" a uint8 array of G.711 codes (an RTP payload as it came off the wire).  An int
        in place of the samples, `(stream, 160, codec)`, is a silent row of that many samples (1 ... N), whatever the codec.
        codec "dvi4" (on a pump with `adpcm=True`) takes a uint8 array too: the whole payload, its 4 header bytes included (5 bytes at least); the row's length is
        derived from it, 2 * (size - 4) samples."""
        streams, lengths, codecs, offsets = self._pack("coded", self.packet_bytes(r), packets)
        self.submit_coded_packets(r, streams, lengths, codecs, offsets)

    def submit_burst(self, r: int, streams, lengths, codecs=None, byte_offsets=None):
        """A BURST tick (vad_pump_submit_burst; needs `max_burst` > 1): rows as in `submit_coded_packets`, except that a stream may be
        listed any number of times and a row may be longer than N.  Each stream's rows are appended, in row order, to what it has
        pending; a stream that completes k chunks (k <= max_burst) is stepped k times, in order, inside this tick.  The results are
        those of the same audio fed chunk by chunk, bit for bit.  A stream that would complete more than max_burst chunks, more rows
        than `streams`, a bad codec, stream, length or offset raises and queues nothing.
        byte_offsets[i] == ROW_SILENT (-1): a SILENT row of lengths[i] >= 1 int16 zeros (see `submit_packets`), longer than N if the
        gap was; it counts towards max_burst like any row.  With byte_offsets=None every row has a payload.
        A "dvi4" row: any even length >= 2, 4 + lengths[i] / 2 bytes (see `submit_coded_packets`)."""
        self._submit_route("burst", r, streams, lengths, byte_offsets, codecs)

    def write_burst(self, r: int, packets):
        """Pack [(stream, samples) | (stream, samples, codec), ...] back to back in arrival order (each rounded up to 16 bytes) into
        `packet_bytes(r)` and submit the burst tick: packets of any length, streams repeated as often as they delivered.  codec "s16"
        (the default) takes an int16 array, "ulaw" / "alaw" a uint8 array of G.711 codes, "dvi4" a uint8 DVI4 payload with its header
        (`write_coded_packets`).  An int in place of the samples, `(stream, 3 * N + 5)`, is a silent row of that many samples."""
        streams, lengths, codecs, offsets = self._pack("burst", self.packet_bytes(r), packets, default="s16")
        self.submit_burst(r, streams, lengths, codecs, offsets)

    def set_wideband(self, max_step: int):
        """Enable WIDE packet ticks (vad_pump_set_wideband): rows sampled at up to max_step x 16 kHz -- 2 (32 kHz) or 3 (48 kHz) -- on a
        16 kHz pump with no tick in flight.  Allocates the wide slots ([streams * N * max_step] int16 each) and their device buffers."""
        self._check(self._L.vad_pump_set_wideband(self._h, int(max_step)))
        self.max_step = int(max_step)
        nbytes = self.streams * self.n * self.max_step * 2
        self._wide = [_pinned_view(self._L.vad_pump_wide_slot(self._h, r), ctypes.c_uint8, (nbytes,)) for r in range(self.ring_slots)]

    def wide_slot(self, r: int) -> np.ndarray:
        """Wide slot r's sample area as one flat uint8 array of streams * N * max_step * 2 bytes (page-locked): where a wide tick's rows
        go."""
        if getattr(self, "_wide", None) is None:
            raise ValueError("wideband is not enabled on this pump (set_wideband)")
        return self._wide[r]

    def submit_wide_packets(self, r: int, streams, lengths, steps=None, byte_offsets=None):
        """A WIDE packet tick (vad_pump_submit_wide_packets; needs `set_wideband`): row i of `wide_slot(r)` holds lengths[i] int16
        samples (1 ... steps[i] * N) of stream streams[i], sampled at steps[i] x 16 kHz (1 ... max_step; None = every row at max_step),
        at byte offset byte_offsets[i] (a multiple of 16; None = the rows back to back, each rounded up to 16 bytes).  The device keeps
        the samples of the stream's comb (input sample g iff g % step == 0) and appends them to what the stream has pending: the same
        results, bit for bit, as `submit_packets` with the rows cut by `decimate` at the carried phase.  A bad step, stream, length or
        offset raises and queues nothing.
        byte_offsets[i] == ROW_SILENT (-1): a SILENT row of lengths[i] input samples of silence at steps[i] (see `submit_packets`): the
        phase advances by lengths[i], the stream gains the zeros the comb keeps.  With byte_offsets=None every row has a payload."""
        self._submit_route("wide", r, streams, lengths, byte_offsets, steps)

    def wide_phase(self, stream: int) -> int:
        """The comb phase of `stream`: the input samples it has delivered since its comb started, modulo its step (0 ... step - 1)."""
        v = self._L.vad_pump_wide_phase(self._h, int(stream))
        if v < 0:
            raise ValueError(f"no such stream, or wideband is not enabled: {stream}")
        return int(v)

    def set_resample(self, rates):
        """Enable RESAMPLED packet ticks (vad_pump_set_resample): rows sampled at one of `rates` -- 1 ... 4 distinct source rates that
        `resample_geometry(rate, the pump's rate)` serves, e.g. (44100, 24000, 22050) -- on a pump with no tick in flight.  Allocates the
        resample slots ([streams * A] int16 each, A = the input samples of one chunk at the largest rate, rounded up to 8), their device
        buffers, the fp32 batch and carry and every stream's filter history.  Goes together with a float32 tape (`tape_dtype="float32"`),
        in either order, and leaves that tape and its clocks alone; refused on a pump with the int16 tape, which cannot hold this route's
        fp32 chunks."""
        rt = [r for r in rates]
        if not 1 <= len(rt) <= 4 or not all(isinstance(r, (int, np.integer)) and not isinstance(r, (bool, np.bool_)) and 0 < r < 2 ** 31 for r in rt):
            raise ValueError(f"rates must be 1 ... 4 (VAD_PUMP_MAX_RATES) positive integers, got {rates!r}")
        arr = (ctypes.c_int * len(rt))(*[int(r) for r in rt])
        self._check(self._L.vad_pump_set_resample(self._h, arr, len(rt)))
        self.resample_rates = tuple(int(r) for r in rt)
        self.resample_row = max(-(-self.n * resample_geometry(r, self.sr)[0] // resample_geometry(r, self.sr)[1]) for r in rt)
        self.resample_row = (self.resample_row + 7) // 8 * 8
        nbytes = self.streams * self.resample_row * 2
        self._res = [_pinned_view(self._L.vad_pump_resample_slot(self._h, r), ctypes.c_uint8, (nbytes,)) for r in range(self.ring_slots)]

    def resample_slot(self, r: int) -> np.ndarray:
        """Resample slot r's sample area as one flat uint8 array of streams * resample_row * 2 bytes (page-locked): where a resampled
        tick's rows go."""
        if getattr(self, "_res", None) is None:
            raise ValueError("resampled rows are not enabled on this pump (set_resample)")
        return self._res[r]

    def submit_resampled_packets(self, r: int, streams, lengths, rates=None, byte_offsets=None):
        """A RESAMPLED packet tick (vad_pump_submit_resampled_packets; needs `set_resample`): row i of `resample_slot(r)` holds lengths[i]
        int16 INPUT samples (1 ... resample_row) of stream streams[i], sampled at resample_rates[rates[i]] Hz (rate INDICES; None = every
        row at resample_rates[0]), at byte offset byte_offsets[i] (a multiple of 16; None = the rows back to back, each rounded up to 16
        bytes).  The device runs the streaming resampler (`resample_stream`'s rule, `resample_device`'s bits) and appends the outputs
        that are ready to what the stream has pending; a stream whose pending outputs reach N is stepped on the first N of them.  A
        stream binds to the rate of its first row until `open_stream` / `close_stream`; while bound, every other submit route refuses
        it.  A bad rate index, stream, length or offset, a row at another rate than the stream's, a stream with int16 samples pending,
        or a row that would complete two chunks raises and queues nothing.
        byte_offsets[i] == ROW_SILENT (-1): a SILENT row of lengths[i] input samples of silence (see `submit_packets`): zeros enter the
        filter.  With byte_offsets=None every row has a payload."""
        self._submit_route("resampled", r, streams, lengths, byte_offsets, rates)

    def write_resampled_packets(self, r: int, packets):
        """Pack [(stream, int16 samples, rate) | (stream, int16 samples), ...] back to back (each rounded up to 16 bytes) into
        `resample_slot(r)` and submit the resampled tick, mirroring `write_packets`: `rate` is one of `resample_rates` in Hz (left out:
        resample_rates[0]).  An int in place of the samples, `(stream, 441, 44100)`, is a silent row of that many input samples."""
        streams, lengths, rates, offsets = self._pack("resampled", self.resample_slot(r), packets, default=self.resample_rates[0])
        self.submit_resampled_packets(r, streams, lengths, rates, offsets)

    def resample_state(self, stream: int):
        """(rate the stream is bound to in Hz or 0, its input samples received less O * (outputs emitted // N), its fp32 outputs pending)
        of `stream` (vad_pump_resample_state; host bookkeeping, no synchronisation)."""
        rate, g, c = ctypes.c_int(), ctypes.c_long(), ctypes.c_long()
        if self._L.vad_pump_resample_state(self._h, int(stream), ctypes.byref(rate), ctypes.byref(g), ctypes.byref(c)):
            raise ValueError(f"no such stream, or resampled rows are not enabled: {stream}")
        return rate.value, g.value, c.value

    def burst_steps(self, r: int) -> int:
        """The sub-steps slot r's last tick ran: max(1, the most chunks a stream completed) for a burst tick, 1 for any other."""
        return int(self._L.vad_pump_burst_steps(self._h, int(r)))

    def burst_probs(self, r: int) -> np.ndarray:
        """[burst_steps(r), streams] float32 (a copy): row j = the probabilities of sub-step j of slot r's last tick, -1.0 where the
        stream completed no more than j chunks.  Row 0 is `probs(r)`."""
        k = self.burst_steps(r)
        first = self._probs[r][None, :]
        return first.copy() if k == 1 else np.concatenate([first, self._probs_more[r][:k - 1]])

    def pending(self, stream: int) -> int:
        """Samples of `stream` submitted in packets and not yet stepped (0 ... N - 1)."""
        v = self._L.vad_pump_pending(self._h, int(stream))
        if v < 0:
            raise ValueError(f"no such stream: {stream}")
        return int(v)

    def poll(self, block: bool = True):
        """-> (events, ring slot) of the oldest submitted tick; (None, None) if nothing is in flight or (block=False) it has not finished."""
        r = ctypes.c_int(-1)
        m = self._L.vad_pump_poll(self._h, 1 if block else 0, self._events, len(self._events), ctypes.byref(r))
        if m in (-1, -2):
            return None, None
        if m < 0:
            raise RuntimeError("vad_pump_poll: " + self._L.vad_pump_last_error(self._h).decode())
        ev = self._events
        return [(ev[i].slot, {"end" if ev[i].kind else "start": ev[i].sample}) for i in range(m)], r.value

    def open_stream(self, stream: int):
        self._check(self._L.vad_pump_open(self._h, int(stream)))

    def close_stream(self, stream: int):
        self._check(self._L.vad_pump_close(self._h, int(stream)))

    def state(self, stream: int):
        """(h[128], c[128], ctx[C]) of one stream (synchronises; tests)."""
        h, c, x = np.empty(128, np.float32), np.empty(128, np.float32), np.empty(self.n // 8, np.float32)
        self._check(self._L.vad_pump_state(self._h, int(stream), h.ctypes.data, c.ctypes.data, x.ctypes.data))
        return h, c, x

    def set_adpcm(self, on: bool = True):
        """Enable (or switch off) DVI4 rows, codec "dvi4", on `submit_coded_packets` / `write_coded_packets` / `submit_burst` /
        `write_burst` (vad_pump_set_adpcm; what `StreamPump(..., adpcm=True)` calls): only with no tick in flight; nothing is allocated.
        Without it the pump and its packers know "s16", "ulaw" and "alaw" and refuse codec 3, as they always did."""
        self._check(self._L.vad_pump_set_adpcm(self._h, 1 if on else 0))
        self.adpcm = bool(on)

    def set_tape(self, chunks: int, dtype="int16"):
        """Enable the tape (vad_pump_set_tape / vad_pump_set_tape_f32; what `StreamPump(..., tape_chunks=chunks, tape_dtype=dtype)` calls):
        once, before the first tick, chunks >= 2; a pump has one tape.  dtype "int16": streams x chunks x N int16 samples on the device,
        not together with `set_resample`.  dtype "float32": 4 bytes a sample, every route taped as the net read it -- also the resampled
        one, with `set_resample` before or after this call."""
        dt = _tape_dtype(dtype)
        call = self._L.vad_pump_set_tape_f32 if dt == np.float32 else self._L.vad_pump_set_tape
        self._check(call(self._h, int(chunks)))
        self.tape_chunks = int(chunks)
        self.tape_dtype = dt

    def tape_state(self, stream: int):
        """(count, floor) of `stream`'s tape: the chunks stepped since its clock started (count * N is the iterator's current_sample)
        and the first chunk the tape can hold (vad_pump_tape_state; synchronises; tests)."""
        c, f = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._L.vad_pump_tape_state(self._h, int(stream), ctypes.byref(c), ctypes.byref(f)))
        return c.value, f.value

    @staticmethod
    def _int64_rows(x, name) -> np.ndarray:
        a = np.asarray(x)
        if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise ValueError(f"{name} must be a 1-D sequence of integers, got {a.dtype} of shape {a.shape}")
        return np.ascontiguousarray(a, dtype=np.int64)

    def tape_windows(self, streams, starts, ends):
        """(first, count), two int64 arrays: the part of [starts[i], ends[i]) of streams[i]'s sample clock that the tape still holds,
        as of every tick submitted so far (vad_pump_tape_window; synchronises).  first[i] > starts[i]: the head is no longer held."""
        st, a, b = _int32_rows(streams, "streams"), self._int64_rows(starts, "starts"), self._int64_rows(ends, "ends")
        if not len(st) == len(a) == len(b):
            raise ValueError(f"streams, starts and ends must have one entry per request, got {len(st)}, {len(a)}, {len(b)}")
        first, count = np.zeros(len(st), np.int64), np.zeros(len(st), np.int64)
        n = len(st)
        total = self._L.vad_pump_tape_window(self._h, *[x.ctypes.data if n else None for x in (st, a, b)], n,
                                             first.ctypes.data if n else None, count.ctypes.data if n else None)
        if total < 0:
            raise _lib.VadError(-total, self._L.vad_pump_last_error(self._h).decode())
        return first, count

    def fetch_audio_into(self, streams, first, counts, out, out_offsets):
        """counts[i] samples from sample first[i] of streams[i] to out[out_offsets[i] : ...] (vad_pump_fetch_audio, or vad_pump_fetch_audio_f32
        on a float32 tape): `out` is a flat C-contiguous numpy array of the tape's dtype (`tape_dtype`: int16 or float32), or a flat
        contiguous tensor of that dtype on the pump's GPU.  Exactly those samples are written.  Offsets that are multiples of 16 bytes
        (8 int16 samples, 4 floats; of a 16-byte aligned `out`) take the gather kernel's 16-byte stores.  A range that is not wholly
        inside its stream's window as it is NOW raises ("no longer held") and nothing is written."""
        st, fi, ct, of = (_int32_rows(streams, "streams"), self._int64_rows(first, "first"), self._int64_rows(counts, "counts"),
                          self._int64_rows(out_offsets, "out_offsets"))
        if not len(st) == len(fi) == len(ct) == len(of):
            raise ValueError(f"streams, first, counts and out_offsets must have one entry per request, got {len(st)}, {len(fi)}, {len(ct)}, {len(of)}")
        f32 = self.tape_dtype == np.float32                      # (a pump without a tape: the int16 call refuses it)
        name, np_dt, torch_dt = ("float32", np.float32, torch.float32) if f32 else ("int16", np.int16, torch.int16)
        on_device = isinstance(out, torch.Tensor)
        if on_device:
            if out.dtype != torch_dt or out.dim() != 1 or not out.is_contiguous() or out.device != torch.device("cuda", self.device):
                raise ValueError(f"out must be a flat contiguous {name} tensor on cuda:{self.device}")
            size, ptr = out.numel(), out.data_ptr()
        else:
            if not isinstance(out, np.ndarray) or out.dtype != np_dt or out.ndim != 1 or not out.flags.c_contiguous or not out.flags.writeable:
                raise ValueError(f"out must be a flat, writeable, C-contiguous {name} numpy array (or a {name} tensor on the pump's GPU)")
            size, ptr = out.size, out.ctypes.data
        if len(st) and (ct.min() < 0 or of.min() < 0 or int((of + ct).max()) > size):
            raise ValueError("a request's samples do not fit into out")
        n = len(st)
        fetch = self._L.vad_pump_fetch_audio_f32 if f32 else self._L.vad_pump_fetch_audio
        self._check(fetch(self._h, *[x.ctypes.data if n else None for x in (st, fi, ct)], n, of.ctypes.data if n else None,
                          ptr if size else None, 1 if on_device else 0))

    def fetch_audio(self, streams, starts, ends, device: bool = False):
        """The audio of [starts[i], ends[i]) of streams[i]'s sample clock -- the clock of the events -- as far as the tape still holds
        it: -> (audios, first).  audios[i] is a numpy array of the tape's dtype (int16, or float32 in [-1, 1)) of the samples [first[i],
        first[i] + len(audios[i])); first[i] > starts[i] means the head of the range was no longer held.  device=True: audios is (packed,
        offsets, counts) instead -- ONE tensor of that dtype on the pump's GPU, request i at packed[offsets[i] : offsets[i] + counts[i]]
        (every offset a multiple of 8 samples), for a consumer on the same GPU; nothing crosses the link.  A stream may appear in any
        number of requests.  Raises without a tape, for a stream out of range and for starts[i] > ends[i]."""
        first, count = self.tape_windows(streams, starts, ends)
        offsets = np.zeros(len(count), np.int64)
        if len(count):
            offsets[1:] = np.cumsum((count[:-1] + 7) // 8 * 8)
        total = int(offsets[-1] + count[-1]) if len(count) else 0
        f32 = self.tape_dtype == np.float32
        if device:
            with torch.cuda.device(self.device):
                packed = torch.empty(total, dtype=torch.float32 if f32 else torch.int16, device=torch.device("cuda", self.device))
                torch.cuda.current_stream().synchronize()        # (the pump writes on its own stream: the allocation is settled first)
            self.fetch_audio_into(streams, first, count, packed, offsets)
            return (packed, offsets, count), first
        packed = np.empty(total, np.float32 if f32 else np.int16)
        self.fetch_audio_into(streams, first, count, packed, offsets)
        return [packed[o:o + c] for o, c in zip(offsets.tolist(), count.tolist())], first

    def _export_slots(self, streams):
        """The slot list of an export -> (the distinct slots, int32, or None = every slot; their number; what the library takes for them)."""
        st = None if streams is None else _distinct_slots(streams, "streams")
        n = self.streams if st is None else len(st)
        return st, n, st.ctypes.data if st is not None and n else None

    def export_streams(self, streams=None, version: int = 1) -> np.ndarray:
        """Everything `streams` (distinct slots; None = every slot, ascending) carry, as one self-describing uint8 blob
        (vad_pump_export_streams; layout: include/silero_vad_hip.h): (h, c), the context the next tick reads, the pending samples, the
        comb step and phase, the iterator state and the open / closed flag.  Only with no tick in flight (poll them first).  Read-only:
        the pump and the streams go on as if nothing had happened.
        version=1 refuses a stream that is bound to a resampled rate; version=2 (vad_pump_export_streams_v2) writes the longer record
        that also carries the rate, the resampler's counters, the fp32 pending outputs and the filter history, for bound and unbound
        streams alike.  `import_streams` takes both.  Blob version 3, which also carries the streams' taped audio, is written by
        `export_streams_v3`."""
        if isinstance(version, (bool, np.bool_)) or not isinstance(version, (int, np.integer)) or version not in (1, 2):
            raise ValueError(f"version must be 1 or 2, got {version!r}")
        st, n, st_ptr = self._export_slots(streams)
        size, export = ((self._L.vad_pump_snapshot_bytes, self._L.vad_pump_export_streams) if version == 1 else
                        (self._L.vad_pump_snapshot_bytes_v2, self._L.vad_pump_export_streams_v2))
        blob = np.zeros(int(size(self.sr, n)), np.uint8)
        self._check(export(self._h, st_ptr, n, blob.ctypes.data, blob.size))
        return blob

    def export_streams_v3(self, streams=None, tape_from=None) -> np.ndarray:
        """`export_streams` in blob version 3 (vad_pump_snapshot_plan_v3 + vad_pump_export_streams_v3): the version 2 records and, behind
        them, a run of each stream's tape -- the newest whole chunks from sample tape_from[i] of streams[i]'s clock on, as far as the tape
        holds them (`tape_run`).  tape_from=None: everything held; a {stream: sample} dict: those streams from there, every other stream
        nothing; on a pump without a tape: no audio.  The same rules: no tick in flight, read-only.  `import_streams` takes the blob, and
        a pump whose tape has the same dtype keeps the audio.

        Moving streams in the middle of their utterances, with the audio the END events will ask for:

            col_a, col_b = UtteranceCollector(a), UtteranceCollector(b)
            starts = col_a.open_starts(moving)                   # {stream: START sample} of the streams inside an utterance
            blob = a.export_streams_v3(moving, tape_from=starts)
            b.import_streams(blob, slots)
            for s, d in zip(moving, slots):
                if s in starts:
                    col_b.adopt(d, starts[s])                    # the END on b then returns first == start
                col_a.forget(s)
        """
        st, n, st_ptr = self._export_slots(streams)
        slots = range(self.streams) if st is None else st.tolist()
        if isinstance(tape_from, dict):                          # (behind every int64 sample of a clock: nothing)
            tf = np.array([int(tape_from.get(b, 2 ** 63 - 1)) for b in slots], np.int64)
        else:
            tf = None if tape_from is None else self._int64_rows(tape_from, "tape_from")
        if tf is not None and len(tf) != n:
            raise ValueError(f"tape_from must have one sample position per exported stream, got {len(tf)} for {n}")
        args = (self._h, st_ptr, n, tf.ctypes.data if tf is not None and n else None)
        need = int(self._L.vad_pump_snapshot_plan_v3(*args))
        if need == 0:
            self._check(1)
        blob = np.zeros(need, np.uint8)
        self._check(self._L.vad_pump_export_streams_v3(*args, blob.ctypes.data, blob.size))
        return blob

    def import_streams(self, blob, slots, records=None):
        """Record records[i] of `blob` (None = record i) replaces the whole carried state of slot slots[i] (vad_pump_import_streams); the
        stream continues bit for bit if this pump has the iterator parameters of the pump that wrote the blob.  Only with no tick in
        flight.  A blob of another sample rate, a malformed blob, a bad record index or slot, a 32 / 48 kHz stream for a pump without
        that wideband step, or (version 2) a stream bound to a rate that is none of this pump's `resample_rates` raises, and nothing
        has changed.  A bound record binds its slot; every other record leaves its slot bound to no rate.  The runs of a version 3
        blob enter this pump's tape if it has one of the same dtype -- the newest `tape_chunks` chunks of each, `tape_state(slot)` is
        then (count, count - kept) and `fetch_audio` reaches back across the move; without a tape here they are ignored; a tape of the
        other dtype raises, and nothing has changed."""
        a = _blob_bytes(blob)
        sl = _distinct_slots(slots, "slots")
        rc = None if records is None else _int32_rows(records, "records")
        if rc is not None and len(rc) != len(sl):
            raise ValueError(f"slots and records must have one entry per stream, got {len(sl)} and {len(rc)}")
        n = len(sl)
        self._check(self._L.vad_pump_import_streams(self._h, a.ctypes.data if a.size else None, a.size, rc.ctypes.data if rc is not None and n else None,
                                                    sl.ctypes.data if n else None, n))

    def play(self, rows: np.ndarray, n_ticks: int, first_tick: int = 0, depth: int = 2, fill_threads: int = 0, max_events: int = 0,
             pattern: np.ndarray = None, compact: bool = False):
        """vad_pump_play: stream b plays rows[b] (int16, length a multiple of the chunk) circularly, chunk by chunk.
        pattern [pattern_ticks, streams] uint8 (vad_pump_play_gaps): stream b delivers a chunk at tick t iff pattern[t % pattern_ticks, b];
        its audio advances only when it delivers.  compact=True (vad_pump_play_compact): the sources write compact slots, only the
        delivering streams' rows cross the link.
        -> (events [(stream, {...}), ...] (the first max_events of them), stats dict)."""
        if rows.dtype != np.int16 or rows.ndim != 2 or rows.shape[0] != self.streams or not rows.flags.c_contiguous:
            raise ValueError(f"rows must be C-contiguous int16 [{self.streams}, period]")
        if pattern is not None and (pattern.dtype != np.uint8 or pattern.ndim != 2 or pattern.shape[1] != self.streams or not pattern.flags.c_contiguous):
            raise ValueError(f"pattern must be C-contiguous uint8 [pattern_ticks, {self.streams}]")
        cap = int(max_events)
        buf = (_lib.IterEvent * max(cap, 1))()
        st = _lib.PumpStats()
        fn = self._L.vad_pump_play_compact if compact and pattern is not None else self._L.vad_pump_play_gaps
        m = fn(self._h, rows.ctypes.data, rows.shape[1], rows.shape[1], None if pattern is None else pattern.ctypes.data,
                                       0 if pattern is None else pattern.shape[0], int(first_tick), int(n_ticks), int(depth),
                                       int(fill_threads), buf if cap else None, cap, ctypes.byref(st))
        if m < 0:
            raise RuntimeError("vad_pump_play: " + self._L.vad_pump_last_error(self._h).decode())
        ev = [(buf[i].slot, {"end" if buf[i].kind else "start": buf[i].sample}) for i in range(min(m, cap))]
        return ev, {k: getattr(st, k) for k, _ in _lib.PumpStats._fields_}
