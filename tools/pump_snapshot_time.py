#!/usr/bin/env python3
"""Moving ALL streams of a full pump (8 192 streams, 16 kHz by default): vad_pump_export_streams + vad_pump_import_streams against the
only thing there was before them, a loop of vad_pump_state over the same streams (three blocking copies and a synchronise per stream, and
it reads h, c and the context only -- there never was a way back in).  Prints a markdown note (profiles/pump_snapshot.md) and writes it to
the path given as the last argument, if any.

    python tools/pump_snapshot_time.py [reps] [sr] [out.md]"""
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
    cap = 8192
    eng = Engine(device=0)
    src = StreamPump(eng, sr, streams=cap, parts=2, ring_slots=3)
    dst = StreamPump(eng, sr, streams=cap, parts=1, ring_slots=3)
    rng = np.random.default_rng(1)
    for t in range(4):                                           # every stream has stepped chunks and has samples pending
        ln = np.full(cap, 320, np.int32)
        area = src.packet_area(t % 3)[:cap * 320].reshape(cap, 320)
        area[:] = rng.integers(-8000, 8000, (cap, 320), dtype=np.int16)
        src.submit_packets(t % 3, np.arange(cap), ln, np.arange(cap) * 320)
        src.poll()

    def timed(fn):
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), min(ms), max(ms)

    blob = src.export_streams()                                  # (the first call allocates the staging block: not timed)
    dst.import_streams(blob, np.arange(cap))
    info = snapshot_info(src.export_streams([0, 1, cap // 2, cap - 1]))
    assert all(f["pending"] == 4 * 320 % n for f in info)
    slots = np.arange(cap)
    ex = timed(lambda: src.export_streams())
    L, h = src._L, src._h
    out = np.zeros(len(blob), np.uint8)
    ex_raw = timed(lambda: L.vad_pump_export_streams(h, None, cap, out.ctypes.data, out.size))
    im = timed(lambda: dst.import_streams(blob, slots))
    assert np.array_equal(dst.export_streams(), blob)

    def state_loop():
        for s in range(cap):
            src.state(s)
    hb, cb, xb = (np.empty(k, np.float32) for k in (128, 128, n // 8))

    def state_loop_raw():
        for s in range(cap):
            L.vad_pump_state(h, s, hb.ctypes.data, cb.ctypes.data, xb.ctypes.data)
    old_reps = max(2, reps // 5)
    reps, keep = old_reps, reps
    st = timed(state_loop)
    st_raw = timed(state_loop_raw)
    reps = keep
    mb = len(blob) / 1e6
    lines = [f"# Moving every stream of a pump: {cap} streams, {sr // 1000} kHz",
             "",
             f"`python tools/pump_snapshot_time.py {reps} {sr}`; median (min ... max) of {reps} calls ({old_reps} for the loop), wall time of the",
             f"blocking call.  The blob is {mb:.1f} MB in pageable host memory.  A tick of audio is 32 ms.",
             "",
             "| what | ms |",
             "|---|---|",
             f"| `vad_pump_export_streams`, all streams (C call into a caller's buffer) | {ex_raw[0]:.2f} ({ex_raw[1]:.2f} ... {ex_raw[2]:.2f}) |",
             f"| `StreamPump.export_streams()` (allocates and zeroes the numpy blob as well) | {ex[0]:.2f} ({ex[1]:.2f} ... {ex[2]:.2f}) |",
             f"| `vad_pump_import_streams`, all streams (`StreamPump.import_streams`) | {im[0]:.2f} ({im[1]:.2f} ... {im[2]:.2f}) |",
             f"| export + import | {ex_raw[0] + im[0]:.2f} |",
             f"| before: a loop of `vad_pump_state` over the streams, ctypes calls (h, c, context only; no way back in) | {st_raw[0]:.1f} ({st_raw[1]:.1f} ... {st_raw[2]:.1f}) |",
             f"| ... through `StreamPump.state()` (allocates three arrays per stream) | {st[0]:.1f} ({st[1]:.1f} ... {st[2]:.1f}) |",
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
