"""JSON probe (tooling, device-resident API): ygm_json_v1_device on the serializing roots of two committed fixtures
  subdoc    tests/golden/snapshot_subdoc_v135 (Tiptap-style XmlFragment trees beside sub-documents)
  snapshot  tests/golden/snapshot_v135
replicated to `n` documents each, against yjs on the host's cores in the same run: `procs` node processes, each a fresh
Y.Doc + applyUpdate + the restated y-prosemirror serializer + JSON.stringify per document over its slice of the same
asks (tools/json_corpus.js --time, through tools/yjs_bundle.js), wall time of the slowest.  The GPU time is the engine's
HIP-event span of the call (stats().kernel_ms: count, scan, k_json and, when a document overflows, its second launch),
warmed up, the best and the median of `reps`.  One JSON line per workload; --readme PATH also writes the table
profiles/json/README.md holds.

    python tools/json_probe.py [n] [reps] [procs] [--readme PATH]"""
import json
import os
import re
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# k_json's resources as the compiler reports them (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage
# on ygm_json.hip / ygm_text.hip); the per-document stages both kernels share (parse, integrate_all, apply_ds) set them
RESOURCES = {"k_json": {"vgpr": 248, "agpr": 16, "sgpr": 106, "scratch_bytes_per_lane": 1440, "lds_bytes_per_block": 40976, "waves_per_simd": 1},
             "k_text": {"vgpr": 248, "agpr": 16, "sgpr": 106, "scratch_bytes_per_lane": 1440, "lds_bytes_per_block": 40976, "waves_per_simd": 1}}
LINE = re.compile(r"^ygm json tiers: docs (\d+) general (\d+) overflow (\d+) overflow_bytes (\d+)$", re.M)


def asks_of(set_name, n):
    import json_fixture as jf
    rows = [r for r in jf.expectations(sets=(set_name,), edges=False) if r[3] == 0 and r[6] > 27]   # (not the absent / empty roots)
    return [(rows[i % len(rows)][1], rows[i % len(rows)][2]) for i in range(n)]


def probe(what, asks, reps, procs):
    import numpy as np
    import torch
    from hocuspocus_amd import Engine
    dev = torch.device("cuda", 0)

    def to_dev(blobs):
        a = np.frombuffer(b"".join(blobs) + bytes(64), np.uint8)
        off = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
        return torch.from_numpy(a.copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev), len(a) - 64

    n = len(asks)
    ts, tso, sb = to_dev([a[0] for a in asks])
    tn, tno, _ = to_dev([a[1] for a in asks])
    os.environ["YGM_TIER_COUNTS"] = "1"
    t = []
    with Engine(0, compat135=True) as e, tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            for rep in range(reps + 2):      # two warm-up rounds
                s0 = e.stats().kernel_ms
                r = e.json_device(ts, sb, tso, tn, tno, n)
                torch.cuda.synchronize()
                if rep >= 2:
                    t.append(e.stats().kernel_ms - s0)
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        lines = LINE.findall(tmp.read().decode())
    out = {"workload": what, "docs": n, "state_bytes": sb, "json_bytes": int(r.payload_bytes), "reps": reps,
           "json_ms": {"best": round(min(t), 3), "median": round(statistics.median(t), 3)},
           "overflow_docs": int(lines[-1][2]) if lines else None, "overflow_share": round(int(lines[-1][2]) / n, 5) if lines else None}
    node = shutil.which("node")
    if node and os.path.exists("/opt/conda/share/jupyter/lab/static/3502.fbe0c610be82ba1360db.js"):
        with tempfile.NamedTemporaryFile(suffix=".bin") as f:
            f.write(struct.pack("<I", n))
            for st, nm in asks:
                f.write(struct.pack("<I", len(st)) + st + struct.pack("<I", len(nm)) + nm)
            f.flush()
            per = (n + procs - 1) // procs
            t0 = time.perf_counter()
            ps = [subprocess.Popen([node, os.path.join(ROOT, "tools", "json_corpus.js"), "--time", f.name, str(k * per), str(min(n, (k + 1) * per))],
                                   stdout=subprocess.PIPE, text=True) for k in range(procs) if k * per < n]
            outs = [p.communicate(timeout=900)[0] for p in ps]
            wall = (time.perf_counter() - t0) * 1e3
        if all(p.returncode == 0 for p in ps):
            js = [json.loads(o.strip().splitlines()[-1]) for o in outs]
            # each process reports the best of three passes over its slice (its start-up is not counted): the slowest slice
            out["yjs"] = {"procs": len(ps), "ms_slowest_slice": max(j["yjs_ms"] for j in js), "ms_sum_of_slices": round(sum(j["yjs_ms"] for j in js), 1),
                          "json_bytes": sum(j["json_bytes"] for j in js), "refused": sum(j["refused"] for j in js), "wall_ms_with_startup_x3": round(wall, 1)}
    print(json.dumps(out), flush=True)
    return out


def readme(path, results, n, reps, procs):
    L = ["# ygm_json_v1: measured", "",
         "Written by `python tools/json_probe.py %d %d %d --readme profiles/json/README.md`: `ygm_json_v1_device` on one MI355X" % (n, reps, procs),
         "against yjs 13.5.16 on the host's cores in the",
         "same run.  The documents are the serializing roots of two committed fixtures, replicated.  GPU time is the HIP-event span",
         "of the whole call (count, scan, `k_json`, and `k_json`'s second launch when a document overflows); the yjs time is a fresh",
         "`Y.Doc`, `applyUpdate`, the restated y-prosemirror serializer and `JSON.stringify` per document, the asks split over the",
         "processes, each process's best of three passes, the slowest slice (process start-up not counted).  The parent commit has no",
         "such path, so the comparison is against yjs on the CPU.", "",
         "| workload | documents | state bytes | JSON bytes | GPU ms (best / median) | yjs ms, slowest of N processes | yjs ms, one core (sum) | overflow reruns |",
         "|---|---|---|---|---|---|---|---|"]
    for r in results:
        y = r.get("yjs")
        L.append("| %s | %d | %d | %d | %.3f / %.3f | %s | %s | %d (%.3f %%) |" % (
            r["workload"], r["docs"], r["state_bytes"], r["json_bytes"], r["json_ms"]["best"], r["json_ms"]["median"],
            "%.1f (N = %d)" % (y["ms_slowest_slice"], y["procs"]) if y else "n/a", "%.1f" % y["ms_sum_of_slices"] if y else "n/a",
            r["overflow_docs"], 100.0 * r["overflow_share"]))
    L += ["", "yjs produced the same number of JSON bytes in every row (%s)." % ", ".join(str(r["yjs"]["json_bytes"] == r["json_bytes"]) for r in results if r.get("yjs")),
          "", "## Kernel resources", "",
          "`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage`:", "",
          "| kernel | VGPRs | AGPRs | SGPRs | scratch bytes / lane | LDS bytes / block | waves / SIMD |", "|---|---|---|---|---|---|---|"]
    for k, v in RESOURCES.items():
        L.append("| `%s` | %d | %d | %d | %d | %d | %d |" % (k, v["vgpr"], v["agpr"], v["sgpr"], v["scratch_bytes_per_lane"], v["lds_bytes_per_block"], v["waves_per_simd"]))
    L += ["", "`k_json` reports what `k_text` reports: both are one thread per document over the same non-inlined stages (parse,",
          "integrate_all, apply_ds), whose call tree sets the register and scratch figures; the JSON walk keeps its marks Map and its",
          "attribute ordering in the document's workspace (`Doc::tx`, the free part of `Doc::st`), not in registers or scratch arrays.",
          "The 40 976 bytes of LDS are the staging of a wave's documents.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(L))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if len(args) > 0 else 4000
    reps = int(args[1]) if len(args) > 1 else 7
    procs = int(args[2]) if len(args) > 2 else 16
    res = [probe("snapshot_subdoc_v135", asks_of("snapshot_subdoc_v135", n), reps, procs),
           probe("snapshot_v135", asks_of("snapshot_v135", n), reps, procs)]
    if "--readme" in sys.argv:
        readme(sys.argv[sys.argv.index("--readme") + 1], res, n, reps, procs)


if __name__ == "__main__":
    main()
