#!/usr/bin/env python3
"""The pump's packet route (vad_pump_submit_packets) against its chunk route (vad_pump_submit_rows) at full capacity: 8 192 streams,
every stream delivering a 20 ms packet per packet tick against a chunk (32 ms) per chunk tick, rows in a shuffled arrival order, two
ticks in flight.  The ring slots are written once before the timed window: this times the device side and the link, not a receive
path's host writes.  Prints one JSON line: per-tick time, link bytes per tick, the share of a plain pinned -> HBM copy's rate that
reaches, and the time per second of audio of every route (equal audio throughput).

    python tools/packet_pump_time.py [ticks] [reps] [sr] [codecs] [burst_share d] [--wide] [--silent SHARE [--zeros]]

sr: 16000 (default) or 8000.  codecs: a comma-separated list of packet formats, timed alternately with the chunk route -- "s16" (the
default: int16 packets through vad_pump_submit_packets), "ulaw" / "alaw" (G.711 packets, 1 byte a sample, through
vad_pump_submit_coded_packets; the device expands them), "dvi4" (RFC 3551 4-bit IMA ADPCM payloads, a 4-byte header and 2 samples a
byte, through the same entry; the device decodes them).  The telephony case: `python tools/packet_pump_time.py 2000 3 8000 s16,ulaw,alaw,dvi4`.
For the routes without gaps the tool asserts what a tick's one copy carries: rows x (16 + the row's bytes rounded up to 16) + streams.

burst_share d (e.g. `0.1 3`): burst mode -- adds the route "burst" (vad_pump_submit_burst on a pump with max_burst = 8).  That share of
the streams is withheld for d ticks at a time (in d + 1 phases, so every tick sees the same load) and then delivers its d + 1 packets
in one tick as one long row; everybody else delivers a packet a tick.  Every tick carries the same audio as a tick of "packets", which
is what the same streams cost an integrator without bursts: the withheld packets trickled in one per tick, the stream's events lagging
d ticks behind.  Share, d and the sub-steps per tick are in the output, and so is
"packets_on_burst_pump": the ordinary packet ticks of a burst-enabled pump, which must cost what "packets" costs.

--wide (16 kHz only): adds the route "wide" -- every stream delivers a 20 ms 48 kHz packet (960 int16 samples) a tick through
vad_pump_submit_wide_packets on a pump with vad_pump_set_wideband(3), the device keeps every third sample -- and "packets_on_wide_pump",
the ordinary 16 kHz packet ticks of that same pump.  A wide tick carries the same audio as a packet tick in 3 x the packet bytes.

--silent SHARE (0 ... 1): that share of the streams (the first of the arrival order) is in a gap -- lost packets, DTX -- in every tick of
the routes "packets" / "packets_ulaw" / "packets_alaw": their rows are SILENT rows (offset ROW_SILENT, no bytes in the slot), the payload
rows lie back to back, and the tick's copy ends behind the last of them.  With --zeros the same streams deliver payload rows of int16
zeros instead, each where its packet would lie: what a caller without silent rows sends (and what a library without them can be timed
with).  Both give the same chunks to the step kernels.  "link_bytes_per_tick" is what the tick's one copy carries either way, and
"tick_ms_p50" the median time from a tick's submission to its retirement, two ticks in flight.

assemble_packets_kernel's / assemble_coded_packets_kernel's / assemble_adpcm_packets_kernel's / assemble_burst_kernel's / assemble_wide_packets_kernel's own time: run it under
`rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python tools/packet_pump_time.py ...` (in a run of its own) and read the
kernels' lines of the stats file."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def g711_encode(pcm, law):
    """int16 -> the G.711 code whose expansion is nearest (what an encoder on the far side of the trunk would have sent)."""
    import numpy as np
    from silero_vad_amd import g711_expand
    codes = np.arange(256, dtype=np.uint8)
    lin = g711_expand(codes, law).astype(np.int32)
    order = np.argsort(lin, kind="stable")
    v = lin[order]
    x = pcm.astype(np.int32)
    j = np.clip(np.searchsorted(v, x), 1, len(v) - 1)
    j -= (x - v[j - 1]) <= (v[j] - x)
    return codes[order[j]]


def dvi4_encode(pcm):
    """int16 [rows, P] (P even) -> DVI4 payloads uint8 [rows, 4 + P / 2]: a plain IMA encoder over all rows at once, each row's header
    {predict = its first sample, index = 30}."""
    import numpy as np
    step_of = np.array([7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118,
                        130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060,
                        1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484,
                        7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767])
    index_add = np.array([-1, -1, -1, -1, 2, 4, 6, 8])
    x = pcm.astype(np.int64)
    rows, P = x.shape
    pred, idx = x[:, 0].copy(), np.full(rows, 30)
    out = np.zeros((rows, 4 + P // 2), np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = (pred >> 8) & 0xFF, pred & 0xFF, idx
    for j in range(P):
        step = step_of[idx]
        diff = x[:, j] - pred
        d = np.where(diff < 0, 8, 0)
        diff = np.abs(diff)
        v = step >> 3
        for bit, sh in ((4, 0), (2, 1), (1, 2)):
            on = diff >= step >> sh
            d |= np.where(on, bit, 0)
            diff -= np.where(on, step >> sh, 0)
            v = v + np.where(on, step >> sh, 0)
        pred = np.clip(np.where(d & 8, pred - v, pred + v), -32768, 32767)
        idx = np.clip(idx + index_add[d & 7], 0, 88)
        out[:, 4 + j // 2] |= (d << (0 if j & 1 else 4)).astype(np.uint8)
    return out


def main():
    import numpy as np
    import torch
    import bench
    from silero_vad_amd import Engine, StreamPump
    wide = "--wide" in sys.argv
    zeros = "--zeros" in sys.argv
    silent = 0.0
    if "--silent" in sys.argv:
        k = sys.argv.index("--silent")
        silent = float(sys.argv[k + 1])
        del sys.argv[k:k + 2]
    if not 0.0 <= silent <= 1.0 or (zeros and not silent):
        raise SystemExit("--silent SHARE: a share of 0 ... 1; --zeros goes with it")
    sys.argv = [a for a in sys.argv if a not in ("--wide", "--zeros")]
    ticks = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    sr = int(sys.argv[3]) if len(sys.argv) > 3 else 16000
    codecs = sys.argv[4].split(",") if len(sys.argv) > 4 else ["s16"]
    share = float(sys.argv[5]) if len(sys.argv) > 6 else 0.0
    d = int(sys.argv[6]) if len(sys.argv) > 6 else 0
    if silent and "dvi4" in codecs:
        raise SystemExit("--silent times the s16 / ulaw / alaw routes")
    if sr not in (8000, 16000) or not set(codecs) <= {"s16", "ulaw", "alaw", "dvi4"} or not 0.0 <= share <= 1.0 or not 0 <= d <= 11 or (wide and sr != 16000):
        raise SystemExit("usage: packet_pump_time.py [ticks] [reps] [8000|16000] [s16,ulaw,alaw,dvi4] [burst_share d (0 ... 11)] [--wide (16000 only)]")
    S, R = 8192, 4
    N, P = (512 if sr == 16000 else 256), sr // 50                     # a chunk, a 20 ms packet (samples)
    dev = torch.device("cuda", 0)
    eng = Engine(device=0)
    link = bench.h2d_rate_GBps(dev)
    rows = bench.fixture_rows_i16(sr, S, N)
    rng = np.random.default_rng(0)
    order = rng.permutation(S).astype(np.int32)
    page = lambda b: (b + 4095) // 4096 * 4096                          # noqa: E731  (the slot's header areas, csrc/pump.hip)
    n_gap = int(S * silent)                                             # rows 0 ... n_gap - 1 of the arrival order are in a gap
    packed = n_gap > 0 and not zeros                                    # silent rows: the payload rows move up, back to back
    # route -> packet format (None: the chunk route)
    names = {"s16": "packets", "ulaw": "packets_ulaw", "alaw": "packets_alaw", "dvi4": "packets_dvi4"}
    row_bytes = {"s16": 2 * P, "ulaw": P, "alaw": P, "dvi4": 4 + P // 2}     # a row in the slot: 320 / 160 / 84 bytes for 20 ms at 8 kHz
    pitch = {c: (b + 15) // 16 * 16 for c, b in row_bytes.items()}           # ... and where the next one starts
    fmt = {names[c]: c for c in codecs}
    fmt["chunks"] = None
    if share > 0:
        fmt["burst"] = "burst"
        fmt["packets_on_burst_pump"] = "s16"                              # ordinary packet ticks of a pump that has bursts enabled
    if wide:
        fmt["wide"] = "wide"
        fmt["packets_on_wide_pump"] = "s16"                               # ordinary packet ticks of the pump that has wideband enabled
    routes = {}
    for name, c in fmt.items():
        if c == "wide":                                                 # row table + flags + the packets at 3 samples for one
            routes[name] = {"bytes": 16 * S + page(S) + S * P * 3 * 2, "ms_audio": 1000.0 * P / sr}
        elif c == "burst":                                                # row table + flags + the same samples as a tick of int16 packets
            routes[name] = {"bytes": 16 * S + page(S) + S * P * 2, "ms_audio": 1000.0 * P / sr}
        elif c is None:                                                 # position table + flags + the chunks
            routes[name] = {"bytes": page(4 * S) + page(S) + S * N * 2, "ms_audio": 1000.0 * N / sr}
        else:                                                           # row table (16 bytes a row) + flags + the packets
            row = row_bytes[c]
            carried = S - n_gap if packed and "_on_" not in name else S
            if zeros and c != "s16":                                    # (the rows of zeros are int16 among 1-byte rows: see below)
                carried = n_gap * 2 + (S - n_gap)
            routes[name] = {"bytes": 16 * S + page(S) + carried * ((row + 15) // 16 * 16), "ms_audio": 1000.0 * P / sr}
            if not n_gap:                                               # what the tick's one copy carries: table + rows, and the flags
                assert routes[name]["bytes"] == S * (16 + pitch[c]) + S, (name, routes[name]["bytes"])
    pumps = {}
    dvi4_payloads = dvi4_encode(rows[order, :P]) if "dvi4" in codecs else None
    for name, c in fmt.items():
        if name == "packets_on_wide_pump":                              # (the same pump object: its ordinary slots)
            pump = pumps["wide"]
        else:
            pump = StreamPump(eng, sr, streams=S, parts=1, ring_slots=R, max_burst=8 if "burst" in name else 1, adpcm=c == "dvi4")
        if c == "wide":
            pump.set_wideband(3)
        for r in range(R):
            if c == "wide":                                             # sample-and-hold: the kept comb is the fixture
                pump.wide_slot(r)[:S * P * 6].view(np.int16).reshape(S, 3 * P)[:] = np.repeat(rows[order, :P], 3, axis=1)
            elif c == "burst":
                pump.packet_area(r)[:S * P].reshape(S, P)[:] = rows[order, :P]
            elif c is None:
                pump.slot(r)[:] = rows[order]
            elif c == "s16":
                pump.packet_area(r)[:S * P].reshape(S, P)[:] = rows[order, :P]
            elif c == "dvi4":
                pump.packet_bytes(r)[:S * pitch[c]].reshape(S, pitch[c])[:, :row_bytes[c]] = dvi4_payloads
            else:
                pump.packet_bytes(r)[:S * P].reshape(S, P)[:] = g711_encode(rows[order, :P], c)
        pumps[name] = pump
    lengths = np.full(S, P, np.int32)
    offsets = (np.arange(S) * P).astype(np.int32)                       # samples (s16) or bytes (G.711): 16-byte aligned either way
    gap_offsets, gap_codecs = {}, {}                                    # per packet format, with `silent`
    if n_gap:
        ROW_SILENT = -1                                                 # (silero_vad_amd.ROW_SILENT, include/silero_vad_hip.h VAD_ROW_SILENT)
        for c in codecs:
            cd = np.full(S, {"s16": 0, "ulaw": 1, "alaw": 2}[c], np.uint8)
            if packed:                                                  # payload row k lies where row k - n_gap lay
                off = np.concatenate([np.full(n_gap, ROW_SILENT), offsets[:S - n_gap]]).astype(np.int32)
                for r in range(R):
                    area = pumps[names[c]].packet_area(r) if c == "s16" else pumps[names[c]].packet_bytes(r)
                    area[:(S - n_gap) * P] = area[n_gap * P:S * P].copy()
            elif c == "s16":
                off = offsets
                for r in range(R):
                    pumps[names[c]].packet_area(r)[:n_gap * P] = 0
            else:                                                       # int16 zeros in front (2 bytes a sample), the G.711 rows behind them
                off = np.concatenate([np.arange(n_gap) * 2 * P, n_gap * 2 * P + np.arange(S - n_gap) * P]).astype(np.int32)
                cd[:n_gap] = 0
                for r in range(R):
                    area = pumps[names[c]].packet_bytes(r)
                    area[n_gap * 2 * P:n_gap * 2 * P + (S - n_gap) * P] = area[n_gap * P:S * P].copy()
                    area[:n_gap * 2 * P] = 0
            gap_offsets[c], gap_codecs[c] = off, cd
    wide_lengths, wide_offsets = np.full(S, 3 * P, np.int32), (np.arange(S) * P * 6).astype(np.int32)
    codec_rows = {"ulaw": np.full(S, 1, np.uint8), "alaw": np.full(S, 2, np.uint8), "dvi4": np.full(S, 3, np.uint8)}
    dvi4_offsets = (np.arange(S) * pitch["dvi4"]).astype(np.int32)      # 96 bytes a row at 8 kHz, 176 at 16 kHz

    # burst mode: the first `share` of the arrival order stalls, in d + 1 phases; phase f delivers (d + 1) packets as ONE row at ticks
    # t = f (mod d + 1), the rest of the group is silent, everybody else delivers a packet (rows back to back: S * P samples a tick)
    phases = []
    if share > 0:
        group = int(S * share) // (d + 1) * (d + 1)
        for f in range(d + 1):
            who = np.concatenate([order[f:group:d + 1], order[group:]])
            ln = np.concatenate([np.full(group // (d + 1), (d + 1) * P), np.full(S - group, P)]).astype(np.int32)
            off = np.zeros(len(ln), np.int64)
            off[1:] = np.cumsum(ln[:-1]) * 2
            phases.append((who.astype(np.int32), ln, off.astype(np.int32)))

    def run(name, n):
        pump, c = pumps[name], fmt[name]
        inflight = 0
        gap = n_gap and name in (names.get(c), ) and c in gap_offsets
        sent, lat = [], lats.setdefault(name, [])
        lat.clear()
        t0 = time.perf_counter()
        for t in range(n):
            sent.append(time.perf_counter())
            if gap and c == "s16":
                pump.submit_packets(t % R, order, lengths, gap_offsets[c])
            elif gap:
                pump.submit_coded_packets(t % R, order, lengths, gap_codecs[c], gap_offsets[c])
            elif c == "wide":
                pump.submit_wide_packets(t % R, order, wide_lengths, None, wide_offsets)
            elif c == "burst":
                pump.submit_burst(t % R, phases[t % (d + 1)][0], phases[t % (d + 1)][1], None, phases[t % (d + 1)][2])
            elif c is None:
                pump.submit_rows(t % R, order)
            elif c == "s16":
                pump.submit_packets(t % R, order, lengths, offsets)
            else:
                pump.submit_coded_packets(t % R, order, lengths, codec_rows[c], dvi4_offsets if c == "dvi4" else offsets)
            inflight += 1
            if inflight >= 2:
                pump.poll()
                lat.append(time.perf_counter() - sent[len(lat)])
                inflight -= 1
        while inflight:
            pump.poll()
            lat.append(time.perf_counter() - sent[len(lat)])
            inflight -= 1
        return time.perf_counter() - t0

    lats = {}

    for name in routes:                                                 # warm-up: code objects, the carry's first fill
        run(name, 200)
    best = {name: float("inf") for name in routes}
    for _ in range(reps):                                               # alternating, best of `reps`
        for name in routes:
            best[name] = min(best[name], run(name, ticks))
    out = {"streams": S, "sr": sr, "packet_samples": P, "ticks": ticks, "reps": reps, "h2d_GBps": round(link, 2)}
    if n_gap:
        out.update({"silent_share": round(n_gap / S, 4), "gap_rows": "int16 zeros" if zeros else "silent"})
    if share > 0:
        out.update({"burst_share": round(group / S, 4), "withheld_ticks": d,
                    "burst_steps_last_ticks": sorted({pumps["burst"].burst_steps(r) for r in range(R)})})
    for name, info in routes.items():
        tick_s = best[name] / ticks
        out[name] = {"tick_us": round(tick_s * 1e6, 1), "link_bytes_per_tick": info["bytes"],
                     "link_GBps": round(info["bytes"] / tick_s / 1e9, 2), "of_link": round(info["bytes"] / tick_s / 1e9 / link, 3),
                     "ms_per_s_audio": round(tick_s * 1e3 / (info["ms_audio"] / 1000.0), 2),
                     "tick_ms_p50": round(float(np.median(lats[name])) * 1e3, 4)}
    for name in routes:
        if name != "chunks":
            out[f"{name}_over_chunks_per_s_audio"] = round(out[name]["ms_per_s_audio"] / out["chunks"]["ms_per_s_audio"], 3)
    for pump in pumps.values():
        pump.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
