#!/usr/bin/env python3
"""The pump's resampled packet route (vad_pump_set_resample + vad_pump_submit_resampled_packets) at full capacity, beside the wide route
at 48 kHz as the yardstick: 8 192 streams, every stream delivering 32 ms of int16 per tick -- 1 411 / 1 412 samples at 44.1 kHz (1 411.2
on average: a chunk per tick), 768 at 24 kHz, 1 536 at 48 kHz through vad_pump_submit_wide_packets --, rows in a shuffled arrival order.
The slots are written once before the timed window: this times the device side and the link, not a receive path's host writes.  Prints
one JSON line: per route the per-tick time with two ticks in flight ("tick_us", best of `reps`), the bytes the tick's one copy carries,
the share of a plain pinned -> HBM copy's rate that reaches, and the median time of ONE tick alone, submission to events
("tick_ms_p50_depth1").

    python tools/pump_resample_time.py [ticks] [reps]

The content of the rows is the benchmark's fixture speech, sample-and-held to the row length: plausible audio for the step kernels, not a
faithful 44.1 kHz recording (the route's results are the business of tests/test_pump_resample_gpu.py).

assemble_resampled_packets_kernel's own time (and assemble_wide_packets_kernel's beside it): run it under
`rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python tools/pump_resample_time.py 300 1` (in a run of its own) and read the
kernels' lines of the stats file."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    import numpy as np
    import torch
    import bench
    from silero_vad_amd import Engine, StreamPump
    ticks = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    S, R, N, sr = 8192, 4, 512, 16000
    dev = torch.device("cuda", 0)
    eng = Engine(device=0)
    link = bench.h2d_rate_GBps(dev)
    rows = bench.fixture_rows_i16(sr, S, N)
    rng = np.random.default_rng(0)
    order = rng.permutation(S).astype(np.int32)
    page = lambda b: (b + 4095) // 4096 * 4096                          # noqa: E731  (the slot's header areas, csrc/pump.hip)
    # route -> (source rate, the row lengths of consecutive ticks, samples a row is given room for)
    plan = {"resampled_44100": (44100, [1411, 1411, 1411, 1411, 1412], 1416), "resampled_24000": (24000, [768], 768),
            "wide_48000": (48000, [1536], 1536)}
    pumps, offsets = {}, {}
    for name, (rate, lens, room) in plan.items():
        pump = StreamPump(eng, sr, streams=S, parts=1, ring_slots=R)
        held = np.repeat(rows[order], 3, axis=1)[:, :room]              # [S][room] int16
        if name.startswith("wide"):
            pump.set_wideband(3)
            areas = [pump.wide_slot(r) for r in range(R)]
        else:
            pump.set_resample((rate,))
            areas = [pump.resample_slot(r) for r in range(R)]
        for a in areas:
            a[:S * room * 2].view(np.int16).reshape(S, room)[:] = held
        pumps[name] = pump
        offsets[name] = (np.arange(S) * room * 2).astype(np.int32)

    def submit(name, t):
        rate, lens, _ = plan[name]
        ln = np.full(S, lens[t % len(lens)], np.int32)
        if name.startswith("wide"):
            pumps[name].submit_wide_packets(t % R, order, ln, None, offsets[name])
        else:
            pumps[name].submit_resampled_packets(t % R, order, ln, None, offsets[name])

    clock = {name: 0 for name in plan}                                  # ticks submitted so far: the 44.1 kHz lengths follow it

    def run(name, n, depth):
        pump, inflight, sent, lat = pumps[name], 0, [], []
        t0 = time.perf_counter()
        for _ in range(n):
            sent.append(time.perf_counter())
            submit(name, clock[name])
            clock[name] += 1
            inflight += 1
            if inflight >= depth:
                pump.poll()
                lat.append(time.perf_counter() - sent[len(lat)])
                inflight -= 1
        while inflight:
            pump.poll()
            lat.append(time.perf_counter() - sent[len(lat)])
            inflight -= 1
        return time.perf_counter() - t0, lat

    for name in plan:                                                   # warm-up: code objects, the carries' first fill
        run(name, 200, 2)
    best = {name: float("inf") for name in plan}
    alone = {}
    for _ in range(reps):                                               # alternating, best of `reps`
        for name in plan:
            best[name] = min(best[name], run(name, ticks, 2)[0])
    for name in plan:
        alone[name] = run(name, min(ticks, 500), 1)[1]
    out = {"streams": S, "sr": sr, "ticks": ticks, "reps": reps, "h2d_GBps": round(link, 2)}
    for name, (rate, lens, room) in plan.items():
        tick_s = best[name] / ticks
        row_bytes = (2 * max(lens) + 15) // 16 * 16
        nbytes = (16 if name.startswith("wide") else 32) * S + page(S) + (S - 1) * room * 2 + row_bytes      # table + flags + the rows where they lie
        out[name] = {"tick_us": round(tick_s * 1e6, 1), "link_bytes_per_tick": nbytes, "link_us_at_h2d_rate": round(nbytes / link / 1e3, 1),
                     "link_GBps": round(nbytes / tick_s / 1e9, 2), "of_link": round(nbytes / tick_s / 1e9 / link, 3),
                     "tick_ms_p50_depth1": round(float(np.median(alone[name])) * 1e3, 4),
                     "tick_ms_p95_depth1": round(float(np.percentile(alone[name], 95)) * 1e3, 4)}
    for name in plan:
        if name != "wide_48000":
            out[f"{name}_over_wide_48000"] = round(out[name]["tick_us"] / out["wide_48000"]["tick_us"], 3)
    for pump in pumps.values():
        pump.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
