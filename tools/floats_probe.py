"""What the number conversion costs on the GPU (tooling): ygm_tojson_v1_device over N Array documents of 256 float64
values each on a context opened with YGM_F_FLOATS, against the same documents with every value replaced by an integer
of sixteen digits (still a float64 tag: an integer above 2^31 is stored that way) -- on a context without the flag,
where the integer-only branch writes it, and on the flagged context, where the conversion writes it too.  Times are
the HIP-event span of the call (stats().kernel_ms: count, scan, k_tojson and the second launch of the documents whose
JSON outgrew their workspace), the three workloads alternating inside one process after two warm-up rounds.

    python tools/floats_probe.py [docs [reps]] [--out FILE.json]      one JSON line; needs a GPU"""
import json
import os
import random
import re
import statistics
import struct
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LINE = re.compile(r"^ygm tojson tiers: docs (\d+) general (\d+) overflow (\d+) overflow_bytes (\d+)$", re.M)
VALUES = 256


def documents(n, seed=20251):
    """(float documents, integer documents): document d holds 256 seeded random doubles that neither a varInt nor a
    float32 holds / 256 integers in [10^15, 2^53)."""
    from v1util import vu
    rnd = random.Random(seed)

    def doc(d, vals):
        return b"\x01\x01" + vu(1000 + d) + b"\x00" + b"\x08\x01\x01a" + vu(len(vals)) + b"".join(b"\x7b" + struct.pack(">d", x) for x in vals) + b"\x00"
    fl, it = [], []
    for d in range(n):
        xs = []
        while len(xs) < VALUES:
            b = rnd.getrandbits(64)
            x = struct.unpack(">d", struct.pack(">Q", b))[0]
            if (b >> 52) & 0x7FF == 0x7FF or (abs(x) < 3e38 and struct.unpack(">f", struct.pack(">f", x))[0] == x):
                continue
            xs.append(x)
        fl.append(doc(d, xs))
        it.append(doc(d, [float(rnd.randrange(10 ** 15, 2 ** 53)) for _ in range(VALUES)]))
    return fl, it


def main():
    import numpy as np
    import torch
    from hocuspocus_amd import Engine
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path:
        args.remove(out_path)
    n = int(args[0]) if args else 10000
    reps = int(args[1]) if len(args) > 1 else 7
    dev = torch.device("cuda", 0)
    fl, it = documents(n)

    def to_dev(blobs):
        a = np.frombuffer(b"".join(blobs) + bytes(64), np.uint8)
        off = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
        return torch.from_numpy(a.copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev), len(a) - 64
    names = to_dev([b"a"] * n)
    arenas = {"floats": to_dev(fl), "ints": to_dev(it)}
    os.environ["YGM_TIER_COUNTS"] = "1"
    work = (("floats_flag_on", "floats", True), ("ints_flag_off", "ints", False), ("ints_flag_on", "ints", True))
    t = {w[0]: [] for w in work}
    info = {}
    with Engine(0, floats=True) as on, Engine(0) as off, tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            for rep in range(reps + 2):      # two warm-up rounds; the workloads alternate
                for what, arena, flag in work:
                    e = on if flag else off
                    ts, tso, sb = arenas[arena]
                    s0 = e.stats().kernel_ms
                    r = e.tojson_device(ts, sb, tso, names[0], names[1], n, 1)
                    torch.cuda.synchronize()
                    if rep >= 2:
                        t[what].append(e.stats().kernel_ms - s0)
                    if rep == 0:
                        import bench
                        sts = bench._d2h(r.status, n * 4).view(np.int32)
                        info[what] = {"state_bytes": sb, "json_bytes": int(r.payload_bytes), "ok": int((sts == 0).sum())}
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        lines = LINE.findall(tmp.read().decode())
    for k, (what, _, _) in enumerate(work):
        info[what]["overflow_docs"] = int(lines[k][2])
        info[what]["ms"] = {"best": round(min(t[what]), 3), "median": round(statistics.median(t[what]), 3), "worst": round(max(t[what]), 3)}
    out = {"docs": n, "values_per_doc": VALUES, "reps": reps, "device": torch.cuda.get_device_name(0), **info,
           "ratio_floats_on_over_ints_off_median": round(info["floats_flag_on"]["ms"]["median"] / info["ints_flag_off"]["ms"]["median"], 3)}
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
