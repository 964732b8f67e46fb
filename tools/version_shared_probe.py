"""Shared version-restore probe (tooling): the host API end to end -- pack, upload, the three stages, download -- for
restoring many versions of few documents, through the pair form (Engine.restore_version_batch: the state once per
version) and the shared form (Engine.restore_version_shared_batch: each state once), with the stage times the engine
prints under YGM_VERSION_TIMES summed over the call's chunks.  Inputs come from tests/golden/version_history_v135.json.gz
(its documents that yjs answers every version of, the ~300 KB one left out), cycled:

    64x32    64 states, 32 versions each (2 048 asks)
    2048x1   2 048 states, one version each (nothing to share)

    python tools/version_shared_probe.py [--reps 15] [--warmup 3] [--forms pair,shared] [--cases 64x32,2048x1]

One JSON line per (case, form): the median, minimum and maximum of the end-to-end wall times, the median stage times,
and the docs_snapshot delta of one call.  A form the engine does not have is skipped (the pair form alone runs on
commits before the shared form)."""
import argparse
import gzip
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("snapshot_nogc_ms", "cut_ms", "snapshot_restored_ms")


def inputs(n_states, per_state):
    docs = json.load(gzip.open(os.path.join(ROOT, "tests", "golden", "version_history_v135.json.gz"), "rt"))["docs"]
    docs = [d for d in docs if d["family"] not in ("large", "empty") and all(v["restored"] != "throws" for v in d["versions"])]
    states, ask_state, versions = [], [], []
    for s in range(n_states):
        d = docs[s % len(docs)]
        states.append(bytes.fromhex(d["state"]))
        for k in range(per_state):
            ask_state.append(s)
            versions.append(bytes.fromhex(d["versions"][(s // len(docs) + k) % len(d["versions"])]["version"]))
    return states, ask_state, versions


def stage_times(text):
    """the stage times of one call: summed over the lines (one per chunk) the engine printed"""
    tot = dict.fromkeys(STAGES, 0.0)
    for line in text.splitlines():
        m = re.search(r"snapshot_nogc_ms ([\d.]+) cut_ms ([\d.]+) snapshot_restored_ms ([\d.]+)", line)
        if m:
            for k, v in zip(STAGES, m.groups()):
                tot[k] += float(v)
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--forms", default="pair,shared")
    ap.add_argument("--cases", default="64x32,2048x1")
    a = ap.parse_args()
    from hocuspocus_amd import Engine
    os.environ["YGM_VERSION_TIMES"] = "1"
    for case in a.cases.split(","):
        n_states, per_state = (int(x) for x in case.split("x"))
        states, ask_state, versions = inputs(n_states, per_state)
        pair_states = [states[s] for s in ask_state]
        for form in a.forms.split(","):
            with Engine(0, compat135=True) as e:
                if form == "shared" and not hasattr(e, "restore_version_shared_batch"):
                    continue
                call = (lambda: e.restore_version_batch(pair_states, versions)) if form == "pair" else \
                       (lambda: e.restore_version_shared_batch(states, ask_state, versions))
                wall, stages, snap = [], [], 0
                for it in range(a.warmup + a.reps):
                    with tempfile.TemporaryFile() as tmp:
                        keep = os.dup(2)
                        os.dup2(tmp.fileno(), 2)   # the engine prints the stage times of each device call on stderr
                        try:
                            s0 = e.stats().docs_snapshot
                            t0 = time.perf_counter()
                            res = call()
                            t1 = time.perf_counter()
                            snap = e.stats().docs_snapshot - s0
                        finally:
                            os.dup2(keep, 2)
                            os.close(keep)
                        tmp.seek(0)
                        st = stage_times(tmp.read().decode())
                    assert len(res) == len(versions) and all(r[0] == 0 for r in res)
                    if it >= a.warmup:
                        wall.append((t1 - t0) * 1e3)
                        stages.append(st)
                out = {"case": case, "form": form, "states": n_states, "asks": len(versions),
                       "state_bytes": sum(len(s) for s in (pair_states if form == "pair" else states)), "docs_snapshot_per_call": snap,
                       "wall_ms_median": round(statistics.median(wall), 3), "wall_ms_min": round(min(wall), 3), "wall_ms_max": round(max(wall), 3),
                       **{k: round(statistics.median(s[k] for s in stages), 3) for k in STAGES}, "reps": a.reps}
                print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
