"""Multi-GPU use of the path: streams are independent, so they are sharded across ranks with NO
data-path collective -- one process per GPU, each with its own engine and a
replica of the 1.2 MB weights, the 7 xGMI links idle by design.  This mirrors the reference's only
parallel pattern, process-per-worker over files (examples/parallel_example.ipynb cells 5, 7).  The
only communication is a host-side gather of the (tiny) results to rank 0.
"""
import os
from typing import List, Sequence

import numpy as np
import torch


def world():
    """(rank, world_size, local_rank) from the torchrun environment (1 process = 1 GPU)."""
    return (int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)),
            int(os.environ.get("LOCAL_RANK", 0)))


def shard_range(n_items: int, world_size: int, rank: int) -> range:
    """Contiguous, balanced block of item indices owned by `rank` (first n % W ranks get one more)."""
    if not (0 <= rank < world_size):
        raise ValueError(f"rank {rank} outside world of {world_size}")
    q, r = divmod(n_items, world_size)
    lo = rank * q + min(rank, r)
    return range(lo, lo + q + (1 if rank < r else 0))


def shard_by_duration(lengths: Sequence[int], world_size: int, rank: int) -> List[int]:
    """Indices owned by `rank` when items are dealt out by total duration instead of by count (SURVEY.md 8e:
    "contiguous blocks balanced by total duration"): longest first, each to the rank with the least work so far
    (ties: lowest rank).  Deterministic, so every rank computes the same partition without communicating; the
    returned indices are in input order."""
    if not (0 <= rank < world_size):
        raise ValueError(f"rank {rank} outside world of {world_size}")
    import heapq
    load = [(0, r) for r in range(world_size)]
    mine = []
    for i in sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i)):
        total, r = heapq.heappop(load)
        if r == rank:
            mine.append(i)
        heapq.heappush(load, (total + int(lengths[i]), r))
    return sorted(mine)


def gather_to_rank0(obj, group=None):
    """Host-side gather of a picklable per-rank result; returns the list on rank 0, None elsewhere.
    Works without an initialised process group (single process)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return [obj]
    ws, rk = dist.get_world_size(group), dist.get_rank(group)
    out = [None] * ws if rk == 0 else None
    dist.gather_object(obj, out, dst=0, group=group)
    return out


def batch_speech_timestamps(audios: Sequence[torch.Tensor], model, sampling_rate: int = 16000,
                            rank: int = 0, world_size: int = 1, balance: str = "duration",
                            scheduler: str = "buckets", codec=None, channels=None, source_rate=None, **kwargs) -> List[list]:
    """`get_speech_timestamps` over many recordings (the reference's pattern is one worker process
    per file, examples/parallel_example.ipynb cells 5, 7): this rank processes its shard --
    `balance="duration"` (default) deals recordings out by total audio length, `"count"` by contiguous
    index blocks; recordings of any lengths go through `scheduler="buckets"` (length-sorted lock-step
    batches, `streams.ragged_speech_segments`) or `"refill"` (persistent slots, continuous refill,
    `streams.refill_speech_segments`), both scanned on the GPU -- and rank 0 receives every result in
    input order (other ranks get None).  kwargs are those of get_speech_timestamps.  `codec` ("ulaw" / "alaw", or one per
    recording): the recordings are uint8 G.711 codes; they go to the scheduler as they are (one byte a sample over the link, expanded on
    the device) and the result is that of the `g711_expand`ed recordings.  `channels` (1 or 2, or one per recording): the recordings
    are interleaved int16 samples or G.711 codes, as a WAV data chunk holds a recorded call; a recording goes to one rank whole, is
    split on the device, and the result has one entry per (recording, channel), recording-major (`streams.channel_rows`): that of the
    call on the `deinterleave`d recordings."""
    from .streams import _no_source_rate
    _no_source_rate(source_rate, "batch_speech_timestamps")
    import warnings

    from .streams import _Fanned, _channels_of, _codec_of, deinterleave, g711_expand, ragged_speech_segments, refill_speech_segments
    from .timestamps import get_speech_timestamps

    if balance not in ("duration", "count") or scheduler not in ("buckets", "refill"):
        raise ValueError("balance must be duration|count and scheduler buckets|refill")
    if balance == "duration":
        mine = shard_by_duration([int(a.shape[-1]) if hasattr(a, "shape") else len(a) for a in audios], world_size, rank)
    else:
        mine = list(shard_range(len(audios), world_size, rank))
    cd = _codec_of(audios, codec)                          # (uint8 without a codec, uint8 among int16 / float: refused here)
    ch = _channels_of(audios, channels)                    # (None: every recording is mono)
    if ch is not None:
        _Fanned(audios, ch, cd)                            # (float recordings, an odd length: refused here)
    n_ch = np.ones(len(audios), dtype=np.int64) if ch is None else ch
    row0 = np.concatenate([[0], np.cumsum(n_ch)]).astype(np.int64)      # recording i owns results row0[i] ... row0[i + 1] - 1
    results = {}
    scan_kw = {k: kwargs[k] for k in kwargs if k not in ("return_seconds", "time_resolution",
                                                         "visualize_probs", "progress_tracking_callback",
                                                         "window_size_samples")}
    fast = getattr(model, "audio_forward_device", None)
    if fast is None or kwargs.get("visualize_probs") or kwargs.get("progress_tracking_callback"):
        for i in mine:
            a = audios[i]                                  # (a list's entry, or a PackedRecordings' view of its arena)
            if ch is not None:                             # interleaved: split (and expanded) here, one channel at a time
                for c in range(int(n_ch[i])):
                    x = torch.from_numpy(deinterleave(np.ascontiguousarray(a), int(n_ch[i]), c, None if cd is None else int(cd[i])))
                    results[int(row0[i]) + c] = get_speech_timestamps(x, model, sampling_rate=sampling_rate, **kwargs)
                continue
            if cd is not None:                             # G.711 codes: expanded here, the per-recording path has no device batch
                a = torch.from_numpy(g711_expand(np.ascontiguousarray(a), int(cd[i])))
            results[i] = get_speech_timestamps(a, model, sampling_rate=sampling_rate, **kwargs)
    elif mine:
        step, sr = 1, sampling_rate
        if sr > 16000 and sr % 16000 == 0:                 # utils_vad.py:301-307
            step, sr = sr // 16000, 16000
            warnings.warn('Sampling rate is a multiply of 16000, casting to 16000 manually!')
        local = []
        for i in mine:
            a = audios[i] if torch.is_tensor(audios[i]) else torch.as_tensor(audios[i])
            while a.dim() > 1 and a.shape[0] == 1:
                a = a.squeeze(0)
            local.append(a)
        # The recordings go to the scheduler AS THEY ARE, with the raw rate: every zero-copy route stays open (pinned 48 kHz
        # recordings are read by the DMA / the gather kernel where they lie) and the frontend's loads take every step-th sample
        # (streams._rates) -- the reference's x[::step] (utils_vad.py:301-307) without the copy.  Segments come back in samples of
        # the 16 kHz signal, like the reference's before its final `* step`.
        flat = [(i, c) for i in mine for c in range(int(n_ch[i]))]      # the scheduler's results: one per (recording, channel)
        lens = [(int(local[r].shape[0]) // int(n_ch[i]) + step - 1) // step for r, i in enumerate(mine) for _ in range(int(n_ch[i]))]
        segs = (ragged_speech_segments if scheduler == "buckets" else refill_speech_segments)(
            local, model, sampling_rate, codec=None if cd is None else cd[mine], channels=None if ch is None else ch[mine], **scan_kw)
        seconds, res = kwargs.get("return_seconds", False), kwargs.get("time_resolution", 1)
        for r, (rec_i, c) in enumerate(flat):
            i = int(row0[rec_i]) + c
            out = segs[r]
            if seconds:                                    # utils_vad.py:442-446
                total = lens[r] / sr
                for seg in out:
                    seg["start"] = max(round(seg["start"] / sr, res), 0)
                    seg["end"] = min(round(seg["end"] / sr, res), total)
            elif step > 1:                                 # utils_vad.py:447-450
                for seg in out:
                    seg["start"] *= step
                    seg["end"] *= step
            results[i] = out
    gathered = gather_to_rank0(results)
    if gathered is None:
        return None
    merged = {}
    for part in gathered:
        merged.update(part)
    return [merged[i] for i in range(int(row0[-1]))]
