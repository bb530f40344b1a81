"""An engine, its clones, pumps and a graph-replaying pool IN FLIGHT TOGETHER, driven from several host threads of one process -- the
deployment the pump routes were built for (a 16 kHz pump, an 8 kHz pump and a few blocking `model(chunk)` callers in one server), and
the sentences of include/silero_vad_hip.h that promise it: "An engine and its clones may have calls in flight on different streams at
the same time" (vad_clone), "The pump works on a clone of `e`: the caller's engine stays free for other calls" (vad_pump_create).
Every path of the engine is bit-stable, so the expected result of a concurrent run is no tolerance: it is the bits the same object
produces alone.  What would break that and pass every single-threaded test: a scratch pointer a clone did not take for itself, a static
buffer in csrc/pump.hip, a remembered host-buffer view that survives another thread's vad_host_unregister, an event recorded on the
wrong stream (a process has fewer hardware queues than these tests have streams: ordering rests on the project's own events).
Selected streams are also held against the CPU oracle / the reference's goldens at the suite's bounds, from the solo results.

One thing is kept out of the crowd on purpose: objects whose construction captures a hipGraph (StreamPool(graph=True)) are built one
after the other, before the threads are released.  A stream capture opened by torch is in HIP's global capture mode, in which an
allocating runtime call from ANY thread is an error for the length of the capture; that is a rule of the runtime's capture mode, not
a property of the engine, and a server captures its pools before it serves.  The replays run in the crowd.
Everything here needs a real MI355X:  python -m pytest tests/test_concurrency.py -m gpu
"""
import json
import os
import threading
import time

import numpy as np
import pytest
import torch

from conftest import ROOT, state_err
from silero_vad_amd.streams import _distinct_queue_stream
from test_gpu_parity import TIGHT, TOL, chunk_of, gap_pattern, rolled_rows

pytestmark = pytest.mark.gpu

JOIN_S = 180
PUMP_STREAMS, PUMP_TICKS, WINDOW = 2048, 1500, 100
PUMP_SAMPLE = list(range(0, PUMP_STREAMS, 61)) + [PUMP_STREAMS - 1]
# (L and D: 30 and 100 repetitions measured 24 ms and 12 ms alone on an MI355X; every participant is to run for 30 ms or more alone,
#  so that the overlap condition of test A is not met by accident: raised to 90 and 400)
M_CALLS, L_REPS, D_REPS, G_TICKS, G_CAP = 1500, 90, 400, 300, 256
L_B, L_T = 1025, 40
D_B, D_LEN = 33, 3 * (25 * 512 - 100) + 1
MAX_EVENTS = 400_000


@pytest.fixture(scope="module")
def model(built):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback to silently pass on)")
    from silero_vad_amd import load_silero_vad
    m = load_silero_vad(device=0)
    assert m.engine._h, "native engine not created"
    return m


# ---- the harness ---------------------------------------------------------------------------------------------------------------------
def run_together(workers, background=()):
    """workers: {name: callable}.  One host thread per worker, all released by one barrier; each records time.monotonic() at its start
    and end.  Workers named in `background` are called with a threading.Event that is set once every other worker has returned.  A
    worker's exception is re-raised here; a thread that has not ended JOIN_S after the release fails the test -- no retry, and the
    caller issues no further GPU work.  -> ({name: result}, {name: (start, end)})"""
    gate = threading.Barrier(len(workers))
    results, spans, errors = {}, {}, {}
    others_done = threading.Event()
    left = [sum(1 for k in workers if k not in background)]
    lock = threading.Lock()

    def body(name, fn):
        try:
            gate.wait(JOIN_S)
            t0 = time.monotonic()
            try:
                results[name] = fn(others_done) if name in background else fn()
            finally:
                spans[name] = (t0, time.monotonic())
        except BaseException as e:       # noqa: BLE001 -- handed to the main thread
            errors[name] = e
        finally:
            if name not in background:
                with lock:
                    left[0] -= 1
                    if left[0] == 0:
                        others_done.set()

    threads = {k: threading.Thread(target=body, args=(k, fn), name=k, daemon=True) for k, fn in workers.items()}
    for t in threads.values():
        t.start()
    for k, t in threads.items():
        t.join(JOIN_S)
        if t.is_alive():
            others_done.set()
            pytest.fail(f"{k} did not finish within {JOIN_S} s: {sorted(n for n, x in threads.items() if x.is_alive())} still running")
    for k, e in errors.items():
        raise AssertionError(f"worker {k} raised {type(e).__name__}: {e}") from e
    return results, spans


def same(a, b):
    """Exact equality of two results: dicts / lists / tuples walked, arrays under np.array_equal, everything else under ==."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    if isinstance(a, list) and a and isinstance(a[0], (np.ndarray, dict)):
        return isinstance(b, list) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b          # event lists, counters


def record(name, fig):
    """Figures that are recorded, not asserted: concurrency.json in the repository's output directory (the one bench.py writes its
    detail record to)."""
    import bench
    out = os.path.join(ROOT, os.path.dirname(bench.DETAIL_FILE))
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "concurrency.json")
    have = {}
    if os.path.exists(path):
        with open(path) as f:
            have = json.load(f)
    have[name] = fig
    with open(path, "w") as f:
        json.dump(have, f, indent=1)


# ---- the participants: each builds fresh objects, runs, and returns plain numpy ---------------------------------------------------------
def window_rows(pcm, n, streams=PUMP_STREAMS):
    """Stream s plays a 100-chunk window of the fixture, np.roll(pcm, -s * 7919), in a circle."""
    return np.ascontiguousarray(np.stack([np.roll(pcm, -s * 7919)[:WINDOW * n] for s in range(streams)]))


def pump_participant(model, sr, rows, ticks=PUMP_TICKS, pattern=None):
    def run():
        from silero_vad_amd import StreamPump
        pump = StreamPump(model.engine, sr, streams=PUMP_STREAMS, parts=2, ring_slots=3)
        try:
            ev, stats = pump.play(rows, ticks, depth=3, fill_threads=2, max_events=MAX_EVENTS, pattern=pattern, compact=pattern is not None)
            assert stats["ticks"] == ticks and len(ev) < MAX_EVENTS
            return {"events": ev, "chunks": int(stats["chunks"]), "probs": np.stack([pump.probs(r).copy() for r in range(3)]),
                    "state": np.stack([np.concatenate(pump.state(s)) for s in PUMP_SAMPLE])}
        finally:
            pump.close()
    return run


def model_participant(model, wav, n):
    """Blocking `model(chunk, sr)` calls on CPU chunks, on the ORIGINAL engine (the one the pumps were cloned from): vad_step_host_sync."""
    chunks = torch.from_numpy(wav[:M_CALLS * n].copy()).view(M_CALLS, n)

    def run():
        stream = torch.cuda.Stream(model.device)
        with torch.cuda.stream(stream):
            model.reset_states()
            probs = np.array([model(chunks[t], 16000).item() for t in range(M_CALLS)], np.float32)
            out = {"probs": probs, "state": model._state.cpu().numpy(), "ctx": model._context.cpu().numpy()}
            stream.synchronize()
        return out
    return run


def lane_participant(model, sr, rows, reps, state=None, ctx=None):
    """A clone on its own stream: `reps` forward_audio calls over the same batch, each from the same initial (state, context)."""
    n = chunk_of(16000 if sr > 16000 else sr)

    def run():
        eng = model.engine.clone()
        stream = torch.cuda.Stream(model.device)
        try:
            with torch.cuda.stream(stream):
                x = torch.from_numpy(rows).to(model.device)
                B = x.shape[0]
                st0 = torch.zeros((2, B, 128), device=model.device) if state is None else torch.from_numpy(state).to(model.device)
                cx0 = torch.zeros((B, n // 8), device=model.device) if ctx is None else torch.from_numpy(ctx).to(model.device)
                probs, states = [], []
                for _ in range(reps):
                    st, cx = st0.clone(), cx0.clone()
                    probs.append(eng.forward_audio(x, sr, cx, st))
                    states.append(st)
                out = {"probs": torch.stack(probs).cpu().numpy(), "state": torch.stack(states).cpu().numpy()}
                stream.synchronize()
            return out
        finally:
            eng.close()
    return run


class PoolParticipant:
    """StreamPool on a clone, one hipGraph per ring slot (H2D, fused step, probabilities to the host), replayed per tick; every third
    tick carries present= flags (the flagged graphs).  Both sets of graphs are captured HERE, before the threads start (module
    docstring); the flagged ones by a tick in which nobody delivers, which leaves every stream's state as it is."""

    def __init__(self, model, rows, n, seed=17):
        from silero_vad_amd import StreamPool
        self.pool = StreamPool(model.engine.clone(), 16000, capacity=G_CAP, graph=True, dtype=torch.int16, host_slots=2)
        self.pool.open_all()
        self.pool.submit(0, present=np.zeros(G_CAP, np.uint8))
        assert (self.pool.wait(0).numpy() == -1.0).all()
        self.rows, self.n = rows[:G_CAP], n
        self.flags = (np.random.default_rng(seed).random((G_TICKS, G_CAP)) < 0.8).astype(np.uint8)
        self.flags[np.arange(G_TICKS) % 3 != 2] = 1
        self.device = model.device

    def __call__(self):
        from silero_vad_amd import BatchVADIterator
        pool, n = self.pool, self.n
        it = BatchVADIterator(G_CAP, sampling_rate=16000)
        ring = pool.host_pcm.numpy()
        pos = np.zeros(G_CAP, np.int64)
        probs, events = np.empty((G_TICKS, G_CAP), np.float32), []
        stream = torch.cuda.Stream(self.device)
        with torch.cuda.stream(stream):
            for t in range(G_TICKS):
                r, fl = t % 2, self.flags[t]
                at = (pos % WINDOW) * n
                ring[r][:] = self.rows[np.arange(G_CAP)[:, None], at[:, None] + np.arange(n)[None, :]]
                pool.submit(r, present=fl if t % 3 == 2 else None)
                probs[t] = pool.wait(r).numpy()
                events += [(t, s, e) for s, e in it.feed(probs[t], active=fl.astype(bool))]
                pos += fl
            stream.wait_stream(pool.stream)
            out = {"probs": probs, "events": events, "state": pool.state.cpu().numpy(), "ctx": pool.ctx.cpu().numpy()}
            stream.synchronize()
        return out


def overlap_of(spans):
    return max(s for s, _ in spans.values()), min(e for _, e in spans.values())


# ---- A: steady state --------------------------------------------------------------------------------------------------------------------
def test_everything_in_flight_together_gives_each_its_solo_bits(model, oracle, golden):
    """Six participants, each first alone and then all at once from six host threads (plus two source threads per pump):
      P16  a 2 048-stream pump at 16 kHz, 1 500 ticks played natively (vad_pump_play, two ticks in flight, three HIP streams of its own)
      P8   the same at 8 kHz with ~10 % of the ticks missed in runs, compact slots (vad_pump_play_compact)
      M    1 500 blocking model(chunk, 16000) calls on CPU chunks on the ORIGINAL engine (vad_step_host_sync: waits on the page-locked slot)
      L    a clone: 90 x forward_audio on [1 025, 40 chunks] from a carried state (throughput frontend, fix-up pass, MFMA recurrence)
      G    a StreamPool on a clone replaying its per-slot hipGraphs over 300 ticks, every third with present= flags
      D    a second clone at 48 kHz: 400 x forward_audio on raw int16 [33, 3 * (25 * 512 - 100) + 1] (folded decimation, ragged tail)
    (1) every participant's concurrent result EQUALS its solo result, every repetition of L and D included; (2) the solo results meet
    independent references at the suite's bounds -- M the reference model's own probabilities, L / D / pump streams the CPU oracle on
    the audio they consumed; (3) the runs overlapped: the latest start lies before the earliest end (a guard against passing vacuously,
    not a performance claim).  Wall times and intervals go to concurrency.json (`record`), unasserted."""
    g16, g8 = golden["16k"], golden["8k"]
    dev = model.device
    rows16, rows8 = window_rows(g16["pcm_i16"], 512), window_rows(g8["pcm_i16"], 256)
    pat8 = gap_pattern(PUMP_STREAMS, PUMP_TICKS, np.random.default_rng(5))[:PUMP_TICKS]
    missed = 1.0 - pat8.mean()
    assert pat8.shape == (PUMP_TICKS, PUMP_STREAMS) and 0.06 < missed < 0.15
    rows_l = rolled_rows(g16["wav"], L_B, L_T * 512, 4001)
    _, ctx_l, st_l = oracle.forward_audio(rolled_rows(g16["wav"], L_B, 12 * 512, 2003)[:, ::-1].copy(), 16000)   # a state the network produced
    rows_d = np.ascontiguousarray(np.stack([np.roll(g16["pcm_i16"], -b * 4001)[:D_LEN] for b in range(D_B)]))
    model.engine.reserve(16000, 16, 1)                        # M's scratch: nothing of the original engine grows in the timed region
    torch.cuda.synchronize()

    def participants():
        return {"P16": pump_participant(model, 16000, rows16),
                "P8": pump_participant(model, 8000, rows8, pattern=pat8),
                "M": model_participant(model, g16["wav"], 512),
                "L": lane_participant(model, 16000, rows_l, L_REPS, state=st_l, ctx=ctx_l),
                "G": PoolParticipant(model, rows16, 512),
                "D": lane_participant(model, 48000, rows_d, D_REPS)}

    solo, solo_s = {}, {}
    for name, fn in participants().items():
        res, spans = run_together({name: fn})
        solo[name], solo_s[name] = res[name], spans[name][1] - spans[name][0]
    torch.cuda.synchronize()
    got, spans = run_together(participants())
    torch.cuda.synchronize()
    latest_start, earliest_end = overlap_of(spans)
    t0 = min(s for s, _ in spans.values())
    record("steady_state", {"solo_s": solo_s, "together_s": {k: e - s for k, (s, e) in spans.items()},
                            "intervals_s": {k: [s - t0, e - t0] for k, (s, e) in spans.items()},
                            "max_start_s": latest_start - t0, "min_end_s": earliest_end - t0, "overlapped": latest_start < earliest_end})
    print("solo", solo_s, "together", {k: e - s for k, (s, e) in spans.items()})
    # (1) the same bits as alone
    for name in solo:
        assert same(got[name], solo[name]), f"{name}: the concurrent run differs from the solo run"
    for name in ("L", "D"):
        for r in range(1, len(solo[name]["probs"])):
            assert np.array_equal(got[name]["probs"][r], got[name]["probs"][0]) and np.array_equal(got[name]["state"][r], got[name]["state"][0]), (name, r)
    assert len(solo["P16"]["events"]) > 10_000 and len(solo["P8"]["events"]) > 10_000 and len(solo["G"]["events"]) > 100
    assert solo["P16"]["chunks"] == PUMP_STREAMS * PUMP_TICKS and solo["P8"]["chunks"] == int(pat8.sum())
    # (2) independent references, from the solo results
    want_m = np.asarray(g16["probs_wav"]).reshape(-1)[:M_CALLS]
    err = float(np.abs(solo["M"]["probs"] - want_m).max())
    print("M vs golden", err)
    assert err < TIGHT and want_m.max() > 0.9
    want, _, wst = oracle.forward_audio(rows_l, 16000, state=st_l, ctx=ctx_l)
    figs = float(np.abs(solo["L"]["probs"][0] - want).max()), state_err(solo["L"]["state"][0], wst)
    print("L vs oracle", figs)
    assert figs[0] < TIGHT and figs[1] < TOL, figs
    want, _, wst = oracle.forward_audio(rows_d[:, ::3].astype(np.float32) / 32768.0, 16000)
    figs = float(np.abs(solo["D"]["probs"][0] - want).max()), state_err(solo["D"]["state"][0], wst)
    print("D vs oracle", figs)
    assert solo["D"]["probs"].shape == (D_REPS, D_B, 25) and figs[0] < TIGHT and figs[1] < TOL, figs
    for name, sr, rows, pat, streams in (("P16", 16000, rows16, None, (0, 61, PUMP_STREAMS - 1)), ("P8", 8000, rows8, pat8, (0, 61))):
        n = chunk_of(sr)
        for s in streams:
            k = PUMP_TICKS if pat is None else int(pat[:, s].sum())                 # chunks the stream actually delivered
            audio = np.tile(rows[s], PUMP_TICKS // WINDOW)[:k * n].astype(np.float32) / 32768.0
            want, wctx, wst = oracle.forward_audio(audio[None], sr)
            h_c_ctx = solo[name]["state"][PUMP_SAMPLE.index(s)]
            figs = [state_err(h_c_ctx[:256].reshape(2, 1, 128), wst)]
            assert np.array_equal(h_c_ctx[256:], wctx[0]), (name, s)
            for t in range(PUMP_TICKS - 3, PUMP_TICKS):                           # the ticks whose slots were retired last
                p = solo[name]["probs"][t % 3][s]
                if pat is not None and not pat[t, s]:
                    assert p == -1.0, (name, s, t)
                    continue
                figs.append(abs(float(p) - float(want[0, t if pat is None else int(pat[:t, s].sum())])))
            print(name, "stream", s, "vs oracle: state, probs", figs)
            assert figs[0] < TOL and max(figs[1:], default=0.0) < TIGHT, (name, s, figs)
    # (3) they did run beside each other
    assert latest_start < earliest_end, spans


# ---- B: growth, teardown and unregister under load ----------------------------------------------------------------------------------
def churn_pass(model, x_dev, packets, L):
    """What a server does beside its running streams: a clone whose scratch grows four times and is torn down, a small pump created,
    ticked once and closed, an unrelated buffer page-locked and released, torch's cache returned."""
    from silero_vad_amd import StreamPump
    out = {}
    eng = model.engine.clone()
    try:
        grew = []
        for B in (16, 257, 1025, 4096):
            gen = eng.scratch_generation()
            st, cx = torch.zeros((2, B, 128), device=model.device), torch.zeros((B, 64), device=model.device)
            p = eng.forward_audio(x_dev[:B], 16000, cx, st)
            out[f"probs{B}"], out[f"state{B}"] = p.cpu().numpy(), st.cpu().numpy()
            grew.append(eng.scratch_generation() != gen)
        assert all(grew), grew                                   # the scratch was reallocated each time
    finally:
        eng.close()
    pump = StreamPump(model.engine, 16000, streams=64, parts=1, ring_slots=2, max_burst=4)
    try:
        pump.write_burst(0, packets)
        ev, r = pump.poll()
        out["burst_events"], out["burst_probs"], out["burst_steps"] = ev, pump.burst_probs(r), pump.burst_steps(r)
    finally:
        pump.close()
    buf = np.zeros(1 << 20, np.int16)
    assert L.vad_host_register(buf.ctypes.data, buf.nbytes) == 0
    assert L.vad_host_unregister(buf.ctypes.data) == 0       # bumps the generation under M's remembered buffer views
    torch.cuda.empty_cache()
    return out


def test_scratch_growth_and_teardown_beside_running_streams(model, golden):
    """P16, M and G as above; beside them a fourth thread that, until they are done, keeps cloning an engine and growing its scratch
    (B = 16, 257, 1 025, 4 096: freed and reallocated each time), destroying it, creating / ticking / closing a small burst pump,
    page-locking and releasing an unrelated host buffer (vad_host_unregister invalidates the host-buffer views the blocking call route
    remembers, process-wide) and returning torch's cache.  The three keep their solo bits, every pass of the fourth equals the same
    pass made alone, and at least 3 passes completed while the others ran."""
    from silero_vad_amd import _lib
    g16 = golden["16k"]
    rows16 = window_rows(g16["pcm_i16"], 512)
    x_dev = torch.from_numpy(rolled_rows(g16["wav"], 4096, 3 * 512, 4001)).to(model.device)
    rng = np.random.default_rng(23)
    pcm = g16["pcm_i16"]
    packets = [(int(s), np.roll(pcm, -(40 * 512 + int(s) * 7919))[k * 700:(k + 1) * 700].copy()) for k in range(2) for s in rng.permutation(20)]      # 2 x 700 samples a stream: two chunks each in the one tick
    model.engine.reserve(16000, 16, 1)
    torch.cuda.synchronize()
    L = _lib.lib()

    def churner(others_done=None):
        stream = torch.cuda.Stream(model.device)
        passes, while_running = [], 0
        with torch.cuda.stream(stream):
            while True:
                passes.append(churn_pass(model, x_dev, packets, L))
                stream.synchronize()
                if others_done is None or others_done.is_set():
                    break
                while_running += 1
        return {"passes": passes, "while_running": while_running}

    def participants():
        return {"P16": pump_participant(model, 16000, rows16), "M": model_participant(model, g16["wav"], 512),
                "G": PoolParticipant(model, rows16, 512)}

    solo, solo_s = {}, {}
    for name, fn in dict(participants(), churner=churner).items():
        res, spans = run_together({name: fn})
        solo[name], solo_s[name] = res[name], spans[name][1] - spans[name][0]
    torch.cuda.synchronize()
    alone = solo["churner"]["passes"][0]
    assert alone["burst_steps"] == 2 and alone["probs4096"].max() > 0.5
    got, spans = run_together(dict(participants(), churner=churner), background=("churner",))
    torch.cuda.synchronize()
    t0 = min(s for s, _ in spans.values())
    record("growth_and_teardown", {"solo_s": solo_s, "together_s": {k: e - s for k, (s, e) in spans.items()},
                                   "intervals_s": {k: [s - t0, e - t0] for k, (s, e) in spans.items()},
                                   "churner_passes": len(got["churner"]["passes"]), "churner_passes_while_running": got["churner"]["while_running"]})
    print("solo", solo_s, "together", {k: e - s for k, (s, e) in spans.items()}, "passes", got["churner"]["while_running"])
    for name in ("P16", "M", "G"):
        assert same(got[name], solo[name]), f"{name}: the run beside the churner differs from the solo run"
    for i, one in enumerate(got["churner"]["passes"]):
        assert same(one, alone), f"churner pass {i} differs from the same pass made alone"
    assert got["churner"]["while_running"] >= 3, got["churner"]["while_running"]


# ---- C: lanes of unlike shape from one host thread -------------------------------------------------------------------------------------
def drive_lanes(lanes, rounds, serial, device):
    """lanes: [(engine, sr, x)] with x [B, L] on the device (float32 or int16), or (engine, sr, x, "step") for a lane that makes ONE
    vad_step per round on chunk `round` of x and carries its state from round to round.  The other lanes start every round from zero
    state.  serial: every call on one stream with a synchronise behind it; otherwise each lane on a torch stream of its own, issued
    round-robin from this thread with nothing between the calls, one device synchronise at the end.
    -> per lane {"probs": [rounds, ...], "state": [rounds, 2, B, 128]} (a step lane: the state after its last round)."""
    bufs = []
    for lane in lanes:
        eng, sr, x = lane[:3]
        n = chunk_of(16000 if sr > 16000 else sr)
        B = x.shape[0]
        if len(lane) == 4:
            bufs.append({"probs": torch.full((rounds, B), -9.0, device=device), "state": torch.zeros((2, B, 128), device=device),
                         "ctx": torch.zeros((B, n // 8), device=device)})
        else:
            step = sr // 16000 if sr > 16000 else 1
            T = ((x.shape[1] + step - 1) // step + n - 1) // n
            bufs.append({"probs": torch.full((rounds, B, T), -9.0, device=device), "state": torch.zeros((rounds, 2, B, 128), device=device),
                         "ctx": torch.zeros((rounds, B, n // 8), device=device)})
    torch.cuda.synchronize()
    one = torch.cuda.Stream(device)
    streams = []
    for lane in lanes:      # each lane on a stream that demonstrably runs beside the lanes before it, as the corpus scheduler picks its lanes
        streams.append(one if serial else _distinct_queue_stream(lanes[0][0], device, list(streams)))
    for r in range(rounds):
        for lane, b, st in zip(lanes, bufs, streams):
            eng, sr, x = lane[:3]
            with torch.cuda.stream(st):
                if len(lane) == 4:
                    n = chunk_of(sr)
                    eng.step(x[:, r * n:(r + 1) * n], sr, b["ctx"], b["state"], b["probs"][r])
                else:
                    eng.forward_audio(x, sr, b["ctx"][r], b["state"][r], b["probs"][r])
            if serial:
                st.synchronize()
    torch.cuda.synchronize()
    return [{"probs": b["probs"].cpu().numpy(), "state": b["state"].cpu().numpy()} for b in bufs], streams


def test_four_lanes_of_unlike_calls_equal_their_serial_runs(model, oracle, golden):
    """The engine and three clones on four streams, 40 rounds issued round-robin from ONE host thread with no synchronisation between
    the calls: 16 kHz float [4 096, 8 chunks]; 8 kHz int16 [17, 300 chunks + 3 samples]; raw 48 kHz float, ragged [33, ...]; one
    vad_step of 64 streams per round (the fused latency kernel) that chains its state.  After one device synchronise every round of
    every lane equals the same sequence issued on one stream with a synchronise after each call, and lanes 0-2 meet the oracle.  (The
    corpus scheduler's test covers lanes of one rate and one kernel form.)"""
    g16, g8 = golden["16k"], golden["8k"]
    dev = model.device
    rounds = 40
    x0 = rolled_rows(g16["wav"], 4096, 8 * 512, 4001)
    x1 = np.ascontiguousarray(np.stack([np.roll(g8["pcm_i16"], -b * 7919)[:300 * 256 + 3] for b in range(17)]))
    x2 = rolled_rows(g16["wav"], D_B, D_LEN, 2003)
    x3 = rolled_rows(g16["wav"], 64, rounds * 512, 977)
    eng = model.engine
    clones = [eng.clone() for _ in range(3)]
    lanes = [(eng, 16000, torch.from_numpy(x0).to(dev)), (clones[0], 8000, torch.from_numpy(x1).to(dev)),
             (clones[1], 48000, torch.from_numpy(x2).to(dev)), (clones[2], 16000, torch.from_numpy(x3).to(dev), "step")]
    want, _ = drive_lanes(lanes, rounds, True, dev)
    got, streams = drive_lanes(lanes, rounds, False, dev)
    for k, (a, b) in enumerate(zip(got, want)):
        assert not (b["probs"] == -9.0).any()
        for r in range(rounds):
            assert np.array_equal(a["probs"][r], b["probs"][r]), (k, r)
        assert np.array_equal(a["state"], b["state"]), k
    for k in range(3):                                          # every round of a stateless lane is the same call
        assert all(np.array_equal(want[k]["probs"][r], want[k]["probs"][0]) for r in range(rounds)), k
    refs = ((x0, 16000), (x1.astype(np.float32) / 32768.0, 8000), (x2[:, ::3], 16000))
    for k, (x, sr) in enumerate(refs):
        ref, _, rst = oracle.forward_audio(x, sr)
        figs = float(np.abs(want[k]["probs"][0] - ref).max()), state_err(want[k]["state"][0], rst)
        print("lane", k, "vs oracle", figs)
        assert figs[0] < TIGHT and figs[1] < TOL and np.ptp(ref) > 0.1, (k, figs)      # (ptp: the reference is no constant)
    chain, _, cst = oracle.forward_audio(x3, 16000)
    assert np.abs(want[3]["probs"].T - chain).max() < TIGHT and state_err(want[3]["state"], cst) < TOL
    # not vacuous: the large lane's stream runs BESIDE another lane's (vad_streams_overlap: a kernel on one finishes while a long one on
    # the other is running), so the runtime was free to execute the lanes' kernels at once
    beside = {f"{a}-{b}": bool(eng.streams_overlap(streams[a], streams[b])) for a in range(4) for b in range(a + 1, 4)}
    record("four_lanes", {"lanes_overlap": beside})
    assert any(beside[f"0-{b}"] for b in range(1, 4)), beside
    for c in clones:
        c.close()
