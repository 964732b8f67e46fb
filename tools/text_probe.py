"""Text probe (tooling, device-resident API): ygm_text_v1_device against ygm_snapshot_v1_device in one process, on
  f1    `n` merged C2 logs (bench.py's f1 shape: single-character updates, 20 % deletions, 1-4 clients; flat text, root
        't' -- the flat tier against k_snap_text)
  live  the LIVE_SPECS documents of tests/test_snapshot.py (Tiptap-style XmlFragment trees and heavily edited Y.Text,
        up to 300 clients), their root deep -- k_text against k_snap
and yjs on one CPU core (a fresh Y.Doc, applyUpdate, getText().toString() / the walker; tools/text_corpus.js --time,
through tools/yjs_bundle.js) when node and the bundle are present.  The two calls alternate, warmed up, `reps` times;
each time is the engine's HIP-event span of the call (stats().kernel_ms), the best and the median of the reps.  One
JSON line per workload, with the call's tier line (YGM_TIER_COUNTS).

    python tools/text_probe.py [n] [reps]"""
import json
import os
import re
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def f1_states(n):
    import numpy as np
    from hocuspocus_amd import Engine
    from tools import synth
    arena, upd_off, doc_upd = synth.text_updates(n, 200, seed=61, del_pct=20)
    upd_doc = np.repeat(np.arange(n, dtype=np.uint32), np.diff(doc_upd.astype(np.int64)))
    with Engine(0, compat135=True) as e:
        st, off, ln, data = e.merge_packed_raw(arena, upd_off, upd_doc, n)
        assert (st == 0).all()
        buf = bytes(data)
        return [buf[int(off[d]):int(off[d]) + int(ln[d])] for d in range(n)]


def root_of(state):
    """The root a probe document keeps its text under: tools/synth_live.c's XmlFragment 'prosemirror', else the Y.Text 't'."""
    return b"prosemirror" if b"\x01\x0bprosemirror" in state else b"t"


def tier_lines(tmp):
    tmp.seek(0)
    txt = tmp.read().decode()
    tmp.seek(0)
    tmp.truncate()
    return re.findall(r"^ygm (?:text|snapshot) tiers: .*$", txt, re.M)


def probe(what, states, names, deep, reps):
    import numpy as np
    import torch
    from hocuspocus_amd import Engine
    dev = torch.device("cuda", 0)

    def to_dev(blobs):
        a = np.frombuffer(b"".join(blobs) + bytes(64), np.uint8)
        off = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
        return torch.from_numpy(a.copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev), len(a) - 64

    n = len(states)
    ts, tso, sb = to_dev(states)
    tn, tno, _ = to_dev(names)
    os.environ["YGM_TIER_COUNTS"] = "1"
    t_text, t_snap = [], []
    with Engine(0, compat135=True) as e, tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            for rep in range(reps + 2):      # two warm-up rounds
                s0 = e.stats().kernel_ms
                r = e.text_device(ts, sb, tso, tn, tno, n, deep=deep)
                torch.cuda.synchronize()
                s1 = e.stats().kernel_ms
                q = e.snapshot_device(ts, sb, tso, n)
                torch.cuda.synchronize()
                s2 = e.stats().kernel_ms
                if rep >= 2:
                    t_text.append(s1 - s0)
                    t_snap.append(s2 - s1)
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        lines = tier_lines(tmp)
    out = {"workload": what, "docs": n, "state_bytes": sb, "text_bytes": int(r.payload_bytes), "snapshot_bytes": int(q.payload_bytes),
           "deep": bool(deep), "reps": reps,
           "text_ms": {"best": round(min(t_text), 3), "median": round(statistics.median(t_text), 3)},
           "snapshot_ms": {"best": round(min(t_snap), 3), "median": round(statistics.median(t_snap), 3)},
           "tiers": sorted(set(lines))}
    node = shutil.which("node")
    if node and os.path.exists("/opt/conda/share/jupyter/lab/static/3502.fbe0c610be82ba1360db.js"):
        k = min(n, 2000)
        with tempfile.NamedTemporaryFile(suffix=".bin") as f:
            f.write(struct.pack("<I", k))
            for st, nm in zip(states[:k], names[:k]):
                f.write(struct.pack("<I", len(st)) + st + struct.pack("<I", len(nm)) + nm + struct.pack("<I", int(deep)))
            f.flush()
            p = subprocess.run([node, os.path.join(ROOT, "tools", "text_corpus.js"), "--time", f.name], capture_output=True, text=True, timeout=600)
        if p.returncode == 0:
            j = json.loads(p.stdout.strip().splitlines()[-1])
            out["yjs_one_core"] = {"asks": j["asks"], "ms": j["yjs_one_core_ms"], "ms_scaled_to_docs": round(j["yjs_one_core_ms"] * n / k, 1)}
    print(json.dumps(out), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    states = f1_states(n)
    probe("f1", states, [b"t"] * n, False, reps)
    from test_snapshot import LIVE_SPECS, _live_batch
    live = _live_batch(LIVE_SPECS)
    probe("live", live, [root_of(s) for s in live], True, reps)


if __name__ == "__main__":
    main()
