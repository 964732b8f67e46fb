"""Fields probe (tooling, device-resident API): what one load per document saves.  Over the fixture documents that have
two or more roots (tests/golden/json_fields_v135.json.gz), replicated to `n` documents, it times
  fields     one ygm_json_fields_v1_device call asking all fields of every document
  per_field  the way to the same bytes without it: one ygm_json_v1_device call per field, call k over the documents
             that have a k-th key, each asking that key
and, because most of those documents hold a root that refuses as a fragment (so the all-fields ask stops at it), the
same pair over the listed asks of the roots that do serialize:
  fields_ok / per_field_ok
Both sides run in one process on one GPU, interleaved rep by rep; the time is the engine's HIP-event span of the calls
(stats().kernel_ms), warmed up, best and median of `reps`.  The outputs are compared before anything is timed: a
fields object must be its per-field JSONs joined.  One JSON line per pair.

    python tools/json_fields_probe.py [n] [reps]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def documents(n, ok_only):
    """[(state, keys in output order, encoded list)]: all-fields asks, or the listed asks of serializing roots."""
    import json_fields_fixture as ff
    from hocuspocus_amd.engine import encode_fields
    rows = []
    absent = bytes.fromhex(ff.load()["absent"])      # (the listed ask that names it is not the serializing-roots ask)
    for r in ff.rows(edges=False):
        if ok_only and r.fields and r.status == 0 and absent not in r.fields and len(set(r.fields)) >= 2:
            rows.append((r.state, list(r.fields), encode_fields(r.fields)))
        elif not ok_only and r.fields is None and len(r.keys) >= 2:
            rows.append((r.state, list(r.keys), b""))
    return [rows[i % len(rows)] for i in range(n)]


def probe(what, docs, reps):
    import numpy as np
    import torch
    import bench
    from hocuspocus_amd import Engine
    dev = torch.device("cuda", 0)

    def to_dev(blobs):
        a = np.frombuffer(b"".join(blobs) + bytes(64), np.uint8)
        off = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
        return torch.from_numpy(a.copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev), len(a) - 64

    def fetch(r, n):
        offs = bench._d2h(r.off, n * 8).view(np.uint64)
        lens = bench._d2h(r.len, n * 8).view(np.uint64)
        sts = bench._d2h(r.status, n * 4).view(np.int32)
        data = bench._d2h(r.data, int(r.data_bytes)).tobytes()
        return [(int(sts[d]), data[int(offs[d]):int(offs[d]) + int(lens[d])]) for d in range(n)]

    n = len(docs)
    ts, tso, sb = to_dev([d[0] for d in docs])
    tf, tfo, _ = to_dev([d[2] for d in docs])
    depth = max(len(d[1]) for d in docs)
    calls = []      # per k: the documents with a k-th key, their states again, that key
    for k in range(depth):
        idx = [i for i, d in enumerate(docs) if len(d[1]) > k]
        calls.append((idx, to_dev([docs[i][0] for i in idx]), to_dev([docs[i][1][k] for i in idx])))
    with Engine(0, compat135=True) as e:
        def fields():
            s0 = e.stats().kernel_ms
            r = e.json_fields_device(ts, sb, tso, tf, tfo, n)
            torch.cuda.synchronize()
            return e.stats().kernel_ms - s0, r

        def per_field(keep=None):
            ms = 0.0
            for k, (idx, (a, ao, ab), (b, bo, _)) in enumerate(calls):
                s0 = e.stats().kernel_ms
                r = e.json_device(a, ab, ao, b, bo, len(idx))
                torch.cuda.synchronize()
                ms += e.stats().kernel_ms - s0
                if keep is not None:      # (results are the context's until its next call)
                    for i, x in zip(idx, fetch(r, len(idx))):
                        keep[i].append(x)
            return ms
        # the same bytes both ways, before anything is timed
        got = fetch(fields()[1], n)
        parts = [[] for _ in range(n)]
        per_field(parts)
        same = 0
        for i, d in enumerate(docs):
            bad = [st for st, _ in parts[i] if st]
            want = (bad[0], b"") if bad else (0, b"{" + b",".join(json.dumps(k.decode(), ensure_ascii=False).encode() + b":" + x
                                                                  for k, (_, x) in zip(d[1], parts[i])) + b"}")
            same += got[i] == want
        tf_ms, tp_ms = [], []
        for rep in range(reps + 2):      # two warm-up rounds, the two sides interleaved
            a = fields()[0]
            b = per_field()
            if rep >= 2:
                tf_ms.append(a)
                tp_ms.append(b)
    out = {"workload": what, "docs": n, "state_bytes": sb, "fields_per_doc_max": depth, "single_field_calls": len(calls),
           "single_field_asks": sum(len(c[0]) for c in calls), "ok_docs": sum(st == 0 for st, _ in got),
           "json_bytes": sum(len(b) for _, b in got), "same_bytes": same == n, "reps": reps,
           "fields_ms": {"best": round(min(tf_ms), 3), "median": round(statistics.median(tf_ms), 3)},
           "per_field_ms": {"best": round(min(tp_ms), 3), "median": round(statistics.median(tp_ms), 3)}}
    print(json.dumps(out), flush=True)
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    probe("all fields of the documents with two or more roots", documents(n, False), reps)
    probe("the serializing roots of those documents, listed", documents(n, True), reps)


if __name__ == "__main__":
    main()
