#!/usr/bin/env python3
"""Moving ALL streams of a full pump in blob version 3 (vad_pump_export_streams_v3: every record carries a run of its stream's tape)
against version 2 on the same pump in the same run: 8 192 streams at 16 kHz, an int16 tape of 64 chunks, every stream carrying its newest
32 chunks (268 MB of audio).  The two versions alternate, call by call; the yardstick for version 3 is version 2 plus the tape bytes at
the rate of a plain copy between page-locked host memory and the device, which this run measures as well (and, because a blob lies in
pageable memory, the rate of the same copy from and to pageable memory).  Prints a markdown note (profiles/pump_snapshot_v3.md) and
writes it to the path given as the last argument, if any.

    python tools/pump_snapshot_v3_time.py [reps] [out.md]"""
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    import numpy as np
    import torch
    from silero_vad_amd import Engine, StreamPump, snapshot_info
    args = sys.argv[1:]
    out_path = args.pop() if args and args[-1].endswith(".md") else None
    reps = int(args[0]) if args else 7
    sr, n, cap, tape, carried, ticks = 16000, 512, 8192, 64, 32, 72
    eng = Engine(device=0)
    src = StreamPump(eng, sr, streams=cap, parts=2, ring_slots=3, tape_chunks=tape)
    dst = StreamPump(eng, sr, streams=cap, parts=1, ring_slots=3, tape_chunks=tape)
    rng = np.random.default_rng(1)
    slots = np.arange(cap, dtype=np.int32)
    rows = rng.integers(-8000, 8000, (3, cap, n), dtype=np.int16)
    for t in range(ticks):                                         # full ticks: every ring has wrapped
        src.slot(t % 3)[:] = rows[t % 3]
        src.submit(t % 3)
        src.poll()
    assert src.tape_state(cap - 1) == (ticks, 0)
    tape_from = np.full(cap, (ticks - carried) * n, np.int64)
    L, h = src._L, src._h

    def once(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    blob3 = src.export_streams_v3(tape_from=tape_from)
    blob2 = src.export_streams(version=2)
    tape_bytes = int(blob3[72:80].view("<i8")[0])
    assert tape_bytes == cap * carried * n * 2
    out3, out2 = np.zeros(len(blob3), np.uint8), np.zeros(len(blob2), np.uint8)
    calls = {
        "export v3": lambda: L.vad_pump_export_streams_v3(h, None, cap, tape_from.ctypes.data, out3.ctypes.data, out3.size),
        "export v2": lambda: L.vad_pump_export_streams_v2(h, None, cap, out2.ctypes.data, out2.size),
        "import v3": lambda: dst.import_streams(blob3, slots),
        "import v2": lambda: dst.import_streams(blob2, slots),
    }
    ms = {k: [] for k in calls}
    for rep in range(reps + 1):                                    # the first round warms up (staging allocations, page faults of the buffers)
        for k, fn in calls.items():
            x = once(fn)
            if rep:
                ms[k].append(x)
    assert np.array_equal(out3, blob3) and np.array_equal(out2, blob2)
    dst.import_streams(blob3, slots)
    assert dst.tape_state(cap - 1) == (ticks, ticks - carried)
    audio, first = dst.fetch_audio([cap - 1], [0], [2 ** 62])
    assert int(first[0]) == (ticks - carried) * n and np.array_equal(audio[0], snapshot_info(src.export_streams_v3([cap - 1], tape_from=[0]))[0]["tape"]["audio"][-carried * n:])

    # the plain copies of this run: tape_bytes between the device and page-locked / pageable host memory
    dev = torch.empty(tape_bytes, dtype=torch.uint8, device="cuda:0")
    pinned = torch.empty(tape_bytes, dtype=torch.uint8).pin_memory()
    pageable = torch.zeros(tape_bytes, dtype=torch.uint8)
    copies = {}
    for name, host in (("page-locked", pinned), ("pageable", pageable)):
        for way, fn in (("device to host", lambda: host.copy_(dev)), ("host to device", lambda: dev.copy_(host))):
            t = []
            for rep in range(reps + 1):
                torch.cuda.synchronize()
                x = once(lambda: (fn(), torch.cuda.synchronize()))
                if rep:
                    t.append(x)
            copies[name, way] = t

    med = lambda v: statistics.median(v)
    show = lambda v: f"{med(v):.2f} ({min(v):.2f} ... {max(v):.2f})"
    rate = lambda v: tape_bytes / med(v) / 1e6                     # GB/s
    lines = [f"# Moving every stream of a pump with its audio, blob version 3: {cap} streams, {sr // 1000} kHz, {carried} of {tape} taped chunks each",
             "",
             f"`python tools/pump_snapshot_v3_time.py {reps}`; median (min ... max) of {reps} calls after one warm-up round, wall time of the blocking",
             "call; version 3 and version 2 alternate call by call on the same two pumps.  The export is the C call into a caller's buffer, the",
             "import `StreamPump.import_streams`.  The blobs lie in pageable host memory.",
             "",
             "| call | blob, MB | ms |",
             "|---|---|---|",
             f"| export, version 3 | {len(blob3) / 1e6:.1f} | {show(ms['export v3'])} |",
             f"| export, version 2 | {len(blob2) / 1e6:.1f} | {show(ms['export v2'])} |",
             f"| import, version 3 | {len(blob3) / 1e6:.1f} | {show(ms['import v3'])} |",
             f"| import, version 2 | {len(blob2) / 1e6:.1f} | {show(ms['import v2'])} |",
             "",
             f"The tape section is {tape_bytes / 1e6:.1f} MB.  A plain copy of that many bytes in this run:",
             "",
             "| copy | ms | GB/s |",
             "|---|---|---|"]
    for key, t in copies.items():
        lines.append(f"| {key[0]} host memory, {key[1]} | {show(t)} | {rate(t):.1f} |")
    yard = {}
    for way, call in (("device to host", "export"), ("host to device", "import")):
        yard[call] = {name: med(ms[call + " v2"]) + med(copies[name, way]) for name in ("page-locked", "pageable")}
    lines += ["",
              "Against version 2 plus the tape bytes at the plain copy's rate:",
              "",
              "| call | version 3, ms | version 2 + page-locked copy, ms | ratio | version 2 + pageable copy, ms | ratio |",
              "|---|---|---|---|---|---|"]
    for call in ("export", "import"):
        v3 = med(ms[call + " v3"])
        a, b = yard[call]["page-locked"], yard[call]["pageable"]
        lines.append(f"| {call} | {v3:.2f} | {a:.2f} | {v3 / a:.2f} | {b:.2f} | {v3 / b:.2f} |")
    lines += ["",
              "One MI355X, `parts=2` source pump, `parts=1` destination.  The import also reads every byte of the records on the host before anything",
              "is queued; the audio is payload and is not read there.  No test gates on these figures.",
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
