#!/usr/bin/env python3
"""Moving ALL streams of a full pump (8 192 streams, 16 kHz by default) in blob version 2 (vad_pump_export_streams_v2, which also carries
streams that are bound to a resampled rate) against the version 1 calls on the same pump in the same run.  Two states of the pump: every
stream bound to no rate with int16 samples pending (both versions can move it), then every stream bound to 44.1 or 24 kHz with fp32
outputs pending (version 2 only).  Prints a markdown note (profiles/pump_snapshot_v2.md) and writes it to the path given as the last
argument, if any.

    python tools/pump_snapshot_v2_time.py [reps] [sr] [out.md]"""
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    import numpy as np
    from silero_vad_amd import Engine, StreamPump, snapshot_info
    args = sys.argv[1:]
    out_path = args.pop() if args and args[-1].endswith(".md") else None
    reps = int(args[0]) if args else 20
    sr = int(args[1]) if len(args) > 1 else 16000
    n = 512 if sr == 16000 else 256
    cap, rates = 8192, (44100, 24000)
    eng = Engine(device=0)
    src = StreamPump(eng, sr, streams=cap, parts=2, ring_slots=3)
    dst = StreamPump(eng, sr, streams=cap, parts=1, ring_slots=3)
    src.set_resample(rates)
    dst.set_resample(tuple(reversed(rates)))
    rng = np.random.default_rng(1)
    slots = np.arange(cap)

    def timed(fn):
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), min(ms), max(ms)

    def both_ways(version):
        """(export through the C call into a caller's buffer, StreamPump.import_streams), after one untimed round"""
        L, h = src._L, src._h
        blob = src.export_streams(version=version)
        dst.import_streams(blob, slots)
        assert np.array_equal(dst.export_streams(version=version), blob)
        out = np.zeros(len(blob), np.uint8)
        export = L.vad_pump_export_streams if version == 1 else L.vad_pump_export_streams_v2
        ex = timed(lambda: export(h, None, cap, out.ctypes.data, out.size))
        assert np.array_equal(out, blob)
        return ex, timed(lambda: dst.import_streams(blob, slots)), len(blob) / 1e6

    # every stream bound to no rate: four stepped packets, 256 samples pending (the state of profiles/pump_snapshot.md)
    for t in range(4):
        area = src.packet_area(t % 3)[:cap * 320].reshape(cap, 320)
        area[:] = rng.integers(-8000, 8000, (cap, 320), dtype=np.int16)
        src.submit_packets(t % 3, slots, np.full(cap, 320, np.int32), slots * 320)
        src.poll()
    plain = {v: both_ways(v) for v in (1, 2)}
    # every stream bound: even slots at 44.1 kHz, odd slots at 24 kHz, two rows of 20 ms each behind vad_pump_open
    for s in range(cap):
        src.open_stream(s)
    rate_of = np.tile(np.array([0, 1], np.uint8), cap // 2)
    length = np.where(rate_of == 0, 882, 480).astype(np.int32)
    for t in range(2):
        area = src.resample_slot(t).view(np.int16)[:cap * 888].reshape(cap, 888)
        area[:] = rng.integers(-8000, 8000, (cap, 888), dtype=np.int16)
        src.submit_resampled_packets(t, slots, length, rate_of, slots * 888 * 2)
        src.poll()
    info = snapshot_info(src.export_streams([0, 1, cap - 1], version=2))
    assert [f["resample"]["src_rate"] for f in info] == [44100, 24000, 24000] and all(f["resample"]["pending_out"] > 0 for f in info)
    bound = both_ways(2)

    def row(what, r):
        return f"| {what} | {r[2]:.1f} | {r[0][0]:.2f} ({r[0][1]:.2f} ... {r[0][2]:.2f}) | {r[1][0]:.2f} ({r[1][1]:.2f} ... {r[1][2]:.2f}) | {r[0][0] + r[1][0]:.2f} |"
    worst = max(r[0][0] + r[1][0] for r in (plain[1], plain[2], bound))
    lines = [f"# Moving every stream of a pump in blob version 2: {cap} streams, {sr // 1000} kHz",
             "",
             f"`python tools/pump_snapshot_v2_time.py {reps} {sr}`; median (min ... max) of {reps} calls, wall time of the blocking call: the export",
             "is the C call into a caller's buffer, the import `StreamPump.import_streams`.  The blobs lie in pageable host memory.  A tick of",
             "audio is 32 ms.",
             "",
             "| what | blob, MB | export, ms | import, ms | export + import, ms |",
             "|---|---|---|---|---|",
             row("version 1, every stream bound to no rate (256 samples pending)", plain[1]),
             row("version 2, the same streams", plain[2]),
             row("version 2, every stream bound to 44.1 / 24 kHz (fp32 outputs pending)", bound),
             "",
             f"One MI355X, `parts=2` source pump, `parts=1` destination with its rates in the other order, all three rows in one run.  Version 2",
             f"is {plain[2][0][0] / plain[1][0][0]:.2f} x version 1 on the export and {plain[2][1][0] / plain[1][1][0]:.2f} x on the import for {plain[2][2] / plain[1][2]:.2f} x the bytes; the import also",
             "reads every byte of the blob on the host before anything is queued (the bytes behind `pending_out` and behind H must be zero).",
             f"Draining a whole pump into another costs {worst:.2f} ms at most, {100 * worst / 32:.0f} % of one 32 ms tick" +
             (": it fits between two ticks." if worst < 32 else ": it does NOT fit between two ticks.") + "  No test gates on these figures.",
             ""]
    text = "\n".join(lines)
    print(text)
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(text)
    src.close()
    dst.close()


if __name__ == "__main__":
    main()
