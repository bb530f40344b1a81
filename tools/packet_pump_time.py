#!/usr/bin/env python3
"""The pump's packet route (vad_pump_submit_packets) against its chunk route (vad_pump_submit_rows) at full capacity: 8 192 streams at
16 kHz, every stream delivering a 20 ms packet (320 samples) per packet tick against a 32 ms chunk (512 samples) per chunk tick, rows
in a shuffled arrival order, two ticks in flight.  The ring slots are written once before the timed window: this times the device
side and the link, not a receive path's host writes.  Prints one JSON line: per-tick time, link bytes per tick, the share of a plain
pinned -> HBM copy's rate that reaches, and the time per second of audio of both routes (equal audio throughput).

    python tools/packet_pump_time.py [ticks] [reps]

assemble_packets_kernel's own time: run it under `rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python tools/packet_pump_time.py`
(in a run of its own) and read the kernel's line of the stats file."""
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
    ticks = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    S, sr, N, P, R = 8192, 16000, 512, 320, 4
    dev = torch.device("cuda", 0)
    eng = Engine(device=0)
    link = bench.h2d_rate_GBps(dev)
    rows = bench.fixture_rows_i16(sr, S, N)
    rng = np.random.default_rng(0)
    order = rng.permutation(S).astype(np.int32)
    page = lambda b: (b + 4095) // 4096 * 4096                          # noqa: E731  (the slot's header areas, csrc/pump.hip)
    routes = {
        # row table (16 bytes a row) + flags + the packets
        "packets": {"bytes": 16 * S + page(S) + S * P * 2, "ms_audio": 1000.0 * P / sr},
        # position table + flags + the chunks
        "chunks": {"bytes": page(4 * S) + page(S) + S * N * 2, "ms_audio": 1000.0 * N / sr},
    }
    pumps = {}
    for name in routes:
        pump = StreamPump(eng, sr, streams=S, parts=1, ring_slots=R)
        for r in range(R):
            if name == "packets":
                pump.packet_area(r)[:S * P].reshape(S, P)[:] = rows[order, :P]
            else:
                pump.slot(r)[:] = rows[order]
        pumps[name] = pump
    lengths, offsets = np.full(S, P, np.int32), (np.arange(S) * P).astype(np.int32)

    def run(name, n):
        pump = pumps[name]
        inflight = 0
        t0 = time.perf_counter()
        for t in range(n):
            if name == "packets":
                pump.submit_packets(t % R, order, lengths, offsets)
            else:
                pump.submit_rows(t % R, order)
            inflight += 1
            if inflight >= 2:
                pump.poll()
                inflight -= 1
        while inflight:
            pump.poll()
            inflight -= 1
        return time.perf_counter() - t0

    for name in routes:                                                 # warm-up: code objects, the carry's first fill
        run(name, 200)
    best = {name: float("inf") for name in routes}
    for _ in range(reps):                                               # alternating, best of `reps`
        for name in routes:
            best[name] = min(best[name], run(name, ticks))
    out = {"streams": S, "sr": sr, "packet_samples": P, "ticks": ticks, "reps": reps, "h2d_GBps": round(link, 2)}
    for name, info in routes.items():
        tick_s = best[name] / ticks
        out[name] = {"tick_us": round(tick_s * 1e6, 1), "link_bytes_per_tick": info["bytes"],
                     "link_GBps": round(info["bytes"] / tick_s / 1e9, 2), "of_link": round(info["bytes"] / tick_s / 1e9 / link, 3),
                     "ms_per_s_audio": round(tick_s * 1e3 / (info["ms_audio"] / 1000.0), 2)}
    out["packets_over_chunks_per_s_audio"] = round(out["packets"]["ms_per_s_audio"] / out["chunks"]["ms_per_s_audio"], 3)
    for pump in pumps.values():
        pump.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
