"""Version-history probe (tooling): the HIP-event times of the three restore stages -- the no-GC snapshot of the
states, the cut kernel (k_ver_cut), the snapshot of the cut updates -- and of take, for one batch: the rows of
tests/golden/version_v135.json.gz that yjs answers, repeated to about `n` documents.  One JSON line.

    python tools/version_probe.py [n]"""
import gzip
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    from hocuspocus_amd import Engine
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    rows = [r for r in json.load(gzip.open(os.path.join(ROOT, "tests", "golden", "version_v135.json.gz"), "rt"))["rows"] if r["restored"] != "throws"]
    rows = (rows * (n // len(rows) + 1))[:n]
    dev = torch.device("cuda", 0)

    def to_dev(blobs):
        a = np.frombuffer(b"".join(blobs) + bytes(64), np.uint8)
        off = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
        return torch.from_numpy(a.copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev), len(a) - 64

    ts, tso, sb = to_dev([bytes.fromhex(r["state"]) for r in rows])
    tv, tvo, vb = to_dev([bytes.fromhex(r["version"]) for r in rows])
    os.environ["YGM_VERSION_TIMES"] = "1"
    best = {}
    with Engine(0, compat135=True) as e, tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        os.dup2(tmp.fileno(), 2)   # the engine prints the stage times of each restore on stderr
        try:
            for _ in range(3):
                e.version_restore_device(ts, tso, tv, tvo, n)
                s0 = e.stats().kernel_ms
                e.version_take_device(ts, sb, tso, n)
                torch.cuda.synchronize()
                t = e.stats().kernel_ms - s0
                best["take_ms"] = min(best.get("take_ms", t), t)
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        for line in tmp.read().decode().splitlines():
            m = re.search(r"snapshot_nogc_ms ([\d.]+) cut_ms ([\d.]+) snapshot_restored_ms ([\d.]+)", line)
            if m:
                for k, v in zip(("snapshot_nogc_ms", "cut_ms", "snapshot_restored_ms"), m.groups()):
                    best[k] = min(best.get(k, float(v)), float(v))
    print(json.dumps({"docs": n, "state_bytes": sb, "version_bytes": vb, **{k: round(v, 3) for k, v in best.items()}}), flush=True)


if __name__ == "__main__":
    main()
