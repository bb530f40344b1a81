#!/usr/bin/env python3
"""What the pump's tape costs: `StreamPump.play` at 8 192 streams x 16 kHz in lock step on two pumps of ONE process -- tape_chunks = 0
and tape_chunks = 512 (16.4 s a stream, 4.3 GB) -- alternated, every repetition after a warm-up, and the time of one `fetch_audio` of
256 requests of 2 s each (a host clock around the blocking call).  The untaped pump launches nothing for the tape: its figures are the
baseline, and their run-to-run spread is what a difference has to be read against.  Prints a markdown note (profiles/pump_tape.md) and
writes it to the path given as the last argument, if any.

    python tools/pump_tape_time.py [reps] [ticks] [out.md]"""
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def spread(xs):
    return f"{statistics.median(xs):.4f} ({min(xs):.4f} ... {max(xs):.4f})"


def main():
    import numpy as np
    from silero_vad_amd import Engine, StreamPump
    args = sys.argv[1:]
    out_path = args.pop() if args and args[-1].endswith(".md") else None
    reps = max(5, int(args[0])) if args else 7
    ticks = int(args[1]) if len(args) > 1 else 1500
    sr, n, cap, chunks, warm = 16000, 512, 8192, 512, 200
    eng = Engine(device=0)
    pumps = {0: StreamPump(eng, sr, streams=cap), chunks: StreamPump(eng, sr, streams=cap, tape_chunks=chunks)}
    rng = np.random.default_rng(1)
    rows = rng.integers(-8000, 8000, (cap, 8 * n), dtype=np.int16)
    keys = ("tick_ms_p50", "tick_ms_p95", "wall_ms")
    got = {k: {key: [] for key in keys} for k in pumps}
    at = {k: 0 for k in pumps}
    for rep in range(reps):
        for k in (pumps if rep % 2 == 0 else reversed(list(pumps))):       # alternated, and in alternating order
            p = pumps[k]
            p.play(rows, warm, first_tick=at[k])
            _, st = p.play(rows, ticks, first_tick=at[k] + warm)
            at[k] += warm + ticks
            for key in keys:
                got[k][key].append(st[key])
    # the fetch: 256 utterances of 2 s, each of another stream, ending at the stream's newest sample
    p = pumps[chunks]
    count, _ = p.tape_state(0)
    assert count == at[chunks] and count >= chunks
    who, hi, two_s = np.arange(0, cap, cap // 256)[:256], count * n, 2 * sr
    fetch_host, fetch_dev = [], []
    for rep in range(reps + 1):                                  # (the first call allocates the staging buffers: not counted)
        t0 = time.perf_counter()
        audios, first = p.fetch_audio(who, [hi - two_s] * 256, [hi] * 256)
        t1 = time.perf_counter()
        (packed, offsets, counts), _ = p.fetch_audio(who, [hi - two_s] * 256, [hi] * 256, device=True)
        t2 = time.perf_counter()
        if rep:
            fetch_host.append((t1 - t0) * 1e3)
            fetch_dev.append((t2 - t1) * 1e3)
    assert all(len(a) == two_s for a in audios) and int(first[0]) == hi - two_s
    period = rows.shape[1]
    for i in (0, 100, 255):                                      # (what was played: stream b's chunk at tick t is rows[b, (t * n) % period ...])
        want = np.concatenate([rows[who[i], (t * n) % period:(t * n) % period + n] for t in range(count - 63, count)])[-two_s:]
        assert np.array_equal(audios[i], want), i
        assert np.array_equal(packed[offsets[i]:offsets[i] + counts[i]].cpu().numpy(), want), i
    mb = 256 * two_s * 2 / 1e6
    lines = [f"# The pump's tape: {cap} streams, {sr // 1000} kHz, tape_chunks = {chunks} ({cap * chunks * n * 2 / 1e9:.1f} GB)",
             "",
             f"`python tools/pump_tape_time.py {reps} {ticks}`: `StreamPump.play` in lock step, two pumps of one process alternated, {reps} repetitions of",
             f"{ticks} ticks each after {warm} warm-up ticks; median (min ... max) over the repetitions.  The untaped pump launches nothing for the",
             "tape, so its rows are the baseline and their spread is the run-to-run spread.  The tape adds one launch per step that reads and",
             f"writes {cap * n * 2 / 1e6:.1f} MB of HBM.",
             "",
             "| pump | tick_ms_p50 | tick_ms_p95 | wall_ms |",
             "|---|---|---|---|"]
    for k in pumps:
        lines.append(f"| tape_chunks = {k} | " + " | ".join(spread(got[k][key]) for key in keys) + " |")
    d = {key: statistics.median(got[chunks][key]) - statistics.median(got[0][key]) for key in keys}
    lines += ["",
              f"Difference of the medians, taped less untaped: tick_ms_p50 {d['tick_ms_p50']:+.4f}, tick_ms_p95 {d['tick_ms_p95']:+.4f}, wall_ms {d['wall_ms']:+.2f}"
              f" ({d['wall_ms'] / ticks * 1e3:+.2f} us a tick).",
              "",
              f"`fetch_audio` of 256 requests of 2 s each ({mb:.1f} MB), 256 streams, a host clock around the blocking call, {reps} calls:",
              "",
              "| destination | ms |",
              "|---|---|",
              f"| host: numpy arrays (gather, one D2H copy, dealt out on the host) | {spread(fetch_host)} |",
              f"| device: one packed tensor on the pump's GPU | {spread(fetch_dev)} |",
              ""]
    text = "\n".join(lines)
    print(text)
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(text)
    for p in pumps.values():
        p.close()


if __name__ == "__main__":
    main()
