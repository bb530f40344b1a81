#!/usr/bin/env python3
"""What the pump's fp32 tape costs, measured the way tools/pump_tape_time.py measured the int16 tape: pumps of ONE process alternated, every
repetition after a warm-up, median (min ... max) over the repetitions, the untaped pump as the baseline whose own spread a difference is
read against.  Two tables at 8 192 streams x 16 kHz, tape_chunks = 512 (16.4 s a stream: 8.6 GB of float32, 4.3 GB of int16):

    the resampled 44.1 kHz tick of tools/pump_resample_time.py (every stream 1 411 / 1 412 samples a tick: a chunk per tick, two ticks in
    flight), without a tape and with tape_dtype="float32" -- the route no other tape holds;
    the lock-step `StreamPump.play` tick of tools/pump_tape_time.py, with no tape, the int16 tape and the fp32 tape;

and `fetch_audio` of 256 requests of 2 s each from the fp32 tape, into numpy arrays and into one device tensor (a host clock around the
blocking call).  Prints a markdown note (profiles/pump_tape_f32.md) and writes it to the path given as the last argument, if any.

    python tools/pump_tape_f32_time.py [reps] [ticks] [out.md]"""
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def spread(xs, digits=4):
    return f"{statistics.median(xs):.{digits}f} ({min(xs):.{digits}f} ... {max(xs):.{digits}f})"


def outside(taped, plain):
    """whether the taped median lies outside the untaped repetitions' min ... max"""
    m = statistics.median(taped)
    return not min(plain) <= m <= max(plain)


def main():
    import numpy as np
    import bench
    from silero_vad_amd import Engine, StreamPump
    args = sys.argv[1:]
    out_path = args.pop() if args and args[-1].endswith(".md") else None
    reps = max(5, int(args[0])) if args else 7
    ticks = int(args[1]) if len(args) > 1 else 1500
    sr, n, cap, chunks, warm, R = 16000, 512, 8192, 512, 200, 4
    eng = Engine(device=0)
    rng = np.random.default_rng(1)

    # 1. the resampled 44.1 kHz tick
    res_ticks = min(ticks, 1000)
    order = rng.permutation(cap).astype(np.int32)
    lens, room = [1411, 1411, 1411, 1411, 1412], 1416
    held = np.repeat(bench.fixture_rows_i16(sr, cap, n)[order], 3, axis=1)[:, :room]
    offsets = (np.arange(cap) * room * 2).astype(np.int32)
    res = {}
    for name, kw in (("no tape", {}), ("tape_dtype = float32", {"tape_chunks": chunks, "tape_dtype": "float32"})):
        p = StreamPump(eng, sr, streams=cap, parts=1, ring_slots=R, **kw)
        p.set_resample((44100,))
        for r in range(R):
            p.resample_slot(r)[:cap * room * 2].view(np.int16).reshape(cap, room)[:] = held
        res[name] = p
    clock = {name: 0 for name in res}

    def run(name, count):
        p, inflight = res[name], 0
        t0 = time.perf_counter()
        for _ in range(count):
            t = clock[name]
            p.submit_resampled_packets(t % R, order, np.full(cap, lens[t % len(lens)], np.int32), None, offsets)
            clock[name] += 1
            inflight += 1
            if inflight >= 2:
                p.poll()
                inflight -= 1
        while inflight:
            p.poll()
            inflight -= 1
        return (time.perf_counter() - t0) / count * 1e6

    res_us = {name: [] for name in res}
    for rep in range(reps):
        for name in (res if rep % 2 == 0 else reversed(list(res))):         # alternated, and in alternating order
            run(name, warm)
            res_us[name].append(run(name, res_ticks))
    taped = res["tape_dtype = float32"]
    count, _ = taped.tape_state(0)
    assert taped.tape_state(cap - 1)[0] == count and count >= reps * res_ticks     # (a chunk a tick but for the filter's latency)
    for p in res.values():
        p.close()

    # 2. the lock-step play tick
    pumps = {"no tape": StreamPump(eng, sr, streams=cap), "tape_dtype = int16": StreamPump(eng, sr, streams=cap, tape_chunks=chunks),
             "tape_dtype = float32": StreamPump(eng, sr, streams=cap, tape_chunks=chunks, tape_dtype="float32")}
    rows = rng.integers(-8000, 8000, (cap, 8 * n), dtype=np.int16)
    keys = ("tick_ms_p50", "tick_ms_p95", "wall_ms")
    got = {k: {key: [] for key in keys} for k in pumps}
    at = {k: 0 for k in pumps}
    names = list(pumps)
    for rep in range(reps):
        for k in names[rep % 3:] + names[:rep % 3]:                          # alternated, the order rotated
            p = pumps[k]
            p.play(rows, warm, first_tick=at[k])
            _, st = p.play(rows, ticks, first_tick=at[k] + warm)
            at[k] += warm + ticks
            for key in keys:
                got[k][key].append(st[key])

    # 3. the fetch: 256 utterances of 2 s, each of another stream, ending at the stream's newest sample
    p = pumps["tape_dtype = float32"]
    count, _ = p.tape_state(0)
    assert count == at["tape_dtype = float32"] and count >= chunks
    who, hi, two_s = np.arange(0, cap, cap // 256)[:256], count * n, 2 * sr
    fetch_host, fetch_dev = [], []
    for rep in range(reps + 1):                                  # (the first call allocates the staging buffers: not counted)
        t0 = time.perf_counter()
        audios, first = p.fetch_audio(who, [hi - two_s] * 256, [hi] * 256)
        t1 = time.perf_counter()
        (packed, offs, counts), _ = p.fetch_audio(who, [hi - two_s] * 256, [hi] * 256, device=True)
        t2 = time.perf_counter()
        if rep:
            fetch_host.append((t1 - t0) * 1e3)
            fetch_dev.append((t2 - t1) * 1e3)
    assert all(len(a) == two_s and a.dtype == np.float32 for a in audios) and int(first[0]) == hi - two_s
    period = rows.shape[1]
    for i in (0, 100, 255):                                      # (what was played: stream b's chunk at tick t is rows[b, (t * n) % period ...])
        want = np.concatenate([rows[who[i], (t * n) % period:(t * n) % period + n] for t in range(count - 63, count)])[-two_s:]
        want = (want.astype(np.float32) / np.float32(32768)).view(np.uint32)
        assert np.array_equal(audios[i].view(np.uint32), want), i
        assert np.array_equal(packed[offs[i]:offs[i] + counts[i]].cpu().numpy().view(np.uint32), want), i
    mb = 256 * two_s * 4 / 1e6

    d_res = statistics.median(res_us["tape_dtype = float32"]) - statistics.median(res_us["no tape"])
    lines = [f"# The pump's fp32 tape: {cap} streams, {sr // 1000} kHz, tape_chunks = {chunks} ({cap * chunks * n * 4 / 1e9:.1f} GB of float32)",
             "",
             f"`python tools/pump_tape_f32_time.py {reps} {ticks}`: the pumps of one process alternated, {reps} repetitions after {warm} warm-up ticks each;",
             "median (min ... max) over the repetitions.  The untaped pump launches nothing for the tape, so its rows are the baseline and their",
             "spread is the run-to-run spread a difference is read against.",
             "",
             f"## The resampled 44.1 kHz tick ({res_ticks} ticks a repetition, two ticks in flight, every stream a chunk per tick)",
             "",
             f"The tape adds one launch per tick that reads {cap * n * 4 / 1e6:.1f} MB of the fp32 batch and writes {cap * n * 4 / 1e6:.1f} MB of HBM.",
             "",
             "| pump | tick_us |",
             "|---|---|"]
    for name in res_us:
        lines.append(f"| {name} | {spread(res_us[name], 1)} |")
    lines += ["",
              f"Difference of the medians, taped less untaped: {d_res:+.1f} us a tick; the taped median lies "
              f"{'OUTSIDE' if outside(res_us['tape_dtype = float32'], res_us['no tape']) else 'inside'} the untaped repetitions' min ... max.",
              "",
              f"## The lock-step `StreamPump.play` tick ({ticks} ticks a repetition)",
              "",
              f"The int16 tape reads and writes {cap * n * 2 / 1e6:.1f} MB a tick; the fp32 tape reads {cap * n * 2 / 1e6:.1f} MB of int16 and writes"
              f" {cap * n * 4 / 1e6:.1f} MB of float32.",
              "",
              "| pump | tick_ms_p50 | tick_ms_p95 | wall_ms |",
              "|---|---|---|---|"]
    for k in pumps:
        lines.append(f"| {k} | " + " | ".join(spread(got[k][key]) for key in keys) + " |")
    lines.append("")
    for k in names[1:]:
        d = {key: statistics.median(got[k][key]) - statistics.median(got["no tape"][key]) for key in keys}
        where = "OUTSIDE" if outside(got[k]["wall_ms"], got["no tape"]["wall_ms"]) else "inside"
        lines.append(f"Difference of the medians, {k} less no tape: tick_ms_p50 {d['tick_ms_p50']:+.4f}, tick_ms_p95 {d['tick_ms_p95']:+.4f}, wall_ms "
                     f"{d['wall_ms']:+.2f} ({d['wall_ms'] / ticks * 1e3:+.2f} us a tick); the taped wall_ms median lies {where} the untaped min ... max.")
        lines.append("")
    lines += [f"## `fetch_audio` of 256 requests of 2 s each ({mb:.1f} MB of float32), 256 streams, a host clock around the blocking call, {reps} calls",
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
