"""Reconnect-storm timing (tooling): the shared-state SyncStep2 call (Engine.sync_step2_shared_batch: one state per
document, one state vector per ask) against the per-ask call over the same asks with the state repeated per ask
(Engine.sync_step2_batch), in one process, each timed by a pair of HIP events around the host-API call, with the
host API's own split (h2d / kernel / d2h event times from ygm_stats) beside it.

    python tools/step2_storm.py [--out DIR] [--reps N] [--per-ask-only]

Two shapes, built from the fixture states under tests/golden/:
  storm    1 state (the largest step2_v135 state) x 1000 asks (cuts of its own state vector)
  spread   1000 states x 4 asks (the empty vector and three cuts)
Writes DIR/storm.jsonl (one line per shape and path, best of N) and DIR/storm.md (the same as a table); the replies
of the two paths are compared byte for byte, and a difference fails the run.  --per-ask-only: a library without the shared
forms (a parent-commit build), the per-ask path alone."""
import argparse
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def rd_vu(b, p):
    n = s = 0
    while True:
        x = b[p]
        p += 1
        n |= (x & 127) << s
        s += 7
        if x < 128:
            return n, p


def vu(n):
    o = bytearray()
    while n > 127:
        o.append(0x80 | (n & 127))
        n >>= 7
    o.append(n)
    return bytes(o)


def decode_sv(b):
    n, p = rd_vu(b, 0)
    out = []
    for _ in range(n):
        c, p = rd_vu(b, p)
        k, p = rd_vu(b, p)
        out.append((c, k))
    return out


def encode_sv(ents):
    return vu(len(ents)) + b"".join(vu(c) + vu(k) for c, k in ents)


def fixture_states():
    out = {}
    for f in ("step2_v135.json.gz", "step2_pending_v135.json.gz"):
        for u, *_ in json.load(gzip.open(os.path.join(GOLD, f), "rt"))["rows"]:
            out.setdefault(bytes.fromhex(u), None)
    return list(out)


def own_svs(e, states):
    """each state's own state vector, decoded (through the engine: snapshot, then its state vector); None where the
    snapshot refuses the state or leaves it pending"""
    snaps = e.snapshot_batch(states)
    ok = [k for k, (st, _) in enumerate(snaps) if st == 0]
    svs = e.encode_state_vector_from_update_batch([snaps[k][1] for k in ok])
    out = [None] * len(states)
    for k, (st, sv) in zip(ok, svs):
        if st == 0:
            out[k] = decode_sv(sv)
    return out


def shapes(e):
    states = fixture_states()
    big = max(range(len(states)), key=lambda k: len(states[k]))
    own = own_svs(e, states)
    storm_svs = [b"\x00" if i == 0 else encode_sv([(c, k * i // 1000) for c, k in own[big]]) for i in range(1000)]
    good = [k for k in range(len(states)) if own[k] is not None][:1000]
    assert len(good) == 1000, len(good)
    spread_states = [states[k] for k in good]
    spread_ask, spread_svs = [], []
    for s, k in enumerate(good):
        for q in range(4):
            spread_ask.append(s)
            spread_svs.append(b"\x00" if q == 0 else encode_sv([(c, n * q // 4) for c, n in own[k]]))
    return {"storm": ([states[big]], [0] * 1000, storm_svs), "spread": (spread_states, spread_ask, spread_svs)}


def timed(e, fn, reps):
    import torch
    best = None
    for _ in range(reps):
        s0 = e.stats()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        ev0.record()
        res = fn()
        ev1.record()
        ev1.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        s1 = e.stats()
        row = {"event_ms": round(ev0.elapsed_time(ev1), 3), "wall_ms": round(wall, 3), "h2d_ms": round(s1.h2d_ms - s0.h2d_ms, 3),
               "kernel_ms": round(s1.kernel_ms - s0.kernel_ms, 3), "d2h_ms": round(s1.d2h_ms - s0.d2h_ms, 3),
               "host_syncs": s1.host_syncs - s0.host_syncs, "docs_snapshot": getattr(s1, "docs_snapshot", 0) - getattr(s0, "docs_snapshot", 0)}
        if best is None or row["event_ms"] < best["event_ms"]:
            best = row
    return best, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step2_shared"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--per-ask-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from hocuspocus_amd import Engine
    import hocuspocus_amd.engine as eng
    torch.cuda.init()
    os.makedirs(a.out, exist_ok=True)
    rows = []
    with Engine(0, compat135=True) as e:
        for name, (states, ask, svs) in shapes(e).items():
            per = lambda: e.sync_step2_batch([states[s] for s in ask], svs)   # noqa: E731
            paths = [("per_ask", per)]
            if not a.per_ask_only:
                paths.append(("shared", lambda: e.sync_step2_shared_batch(states, ask, svs)))
            replies = {}
            for path, fn in paths:
                fn()   # warm-up: buffers grown, code loaded
                best, replies[path] = timed(e, fn, a.reps)
                rows.append({"shape": name, "path": path, "states": len(states), "asks": len(svs),
                             "state_bytes": sum(len(s) for s in states), "reps": a.reps, **best,
                             "lib": os.path.relpath(eng.LIB_PATH, ROOT)})
                print(json.dumps(rows[-1]), flush=True)
            if "shared" in replies:
                assert replies["shared"] == replies["per_ask"], f"{name}: the two paths' replies differ"
    with open(os.path.join(a.out, "storm.jsonl"), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    with open(os.path.join(a.out, "storm.md"), "w") as f:
        f.write("| shape | path | states | asks | event ms | h2d ms | kernel ms | d2h ms | snapshots |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['shape']} | {r['path']} | {r['states']} | {r['asks']} | {r['event_ms']} | {r['h2d_ms']} | {r['kernel_ms']} | "
                    f"{r['d2h_ms']} | {r['docs_snapshot']} |\n")
        by = {(r["shape"], r["path"]): r for r in rows}
        for shape in ("storm", "spread"):
            if (shape, "shared") in by:
                f.write(f"\n{shape}: per-ask / shared = {by[(shape, 'per_ask')]['event_ms'] / by[(shape, 'shared')]['event_ms']:.2f}x\n")


if __name__ == "__main__":
    main()
