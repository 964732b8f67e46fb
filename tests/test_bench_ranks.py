"""bench.py's own rank path on CPU: `python bench.py --gpus 2 --dry-run --full` starts two rank processes
through torch.distributed.run (gloo), each takes its fnv1a64(name) mod 2 shard of the named document
sets, the CPU oracle stands in for the engine, and rank 0 prints the node totals."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.timeout(400) if hasattr(pytest.mark, "timeout") else (lambda f: f)
def test_bench_two_ranks_dry_run():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--full", "--docs", "30", "--updates", "12",
                        "--c2big-docs", "20", "--c4-docs", "150", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=380, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout          # rank 0 only
    j = lines[0]
    assert j["n_gpus"] == 2 and j["scaling"] == "weak"
    assert j["config"]["docs_total"] == 60 and j["config"]["docs_per_gpu"] == 30
    assert j["config"]["updates_total"] == 60 * 12
    assert j["c2_100k"]["docs_total"] == 40
    assert j["c4"]["docs_total"] == 150 and set(j["c4"]) >= {"sv", "diff"}
    # single-process totals of the same named document sets
    sys.path.insert(0, ROOT)
    import numpy as np
    from tools import synth
    a, o, d = synth.text_updates_docs(np.arange(60), 12)
    assert j["config"]["bytes_in_total"] == len(a)
    a4, *_ = synth.text_states(150, seed=3)
    assert j["c4"]["bytes_in_total"] == len(a4)


def test_dump_outputs_document_order_and_budget(tmp_path):
    # --dump-outputs: per-document outputs in document order whatever the slots' layout, a failed document
    # contributes no bytes, and past the budget every array is the same seeded sample on every call
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    st = np.array([0, 3, 0, 0], np.int32)
    off = np.array([10, 0, 2, 6], np.uint64)
    ln = np.array([3, 9, 0, 4], np.uint64)
    data = bytes(range(100, 116))
    bench.dump_outputs(str(tmp_path / "a"), st, off, ln, data)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in ("status", "len", "data")}
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["data.npy", "len.npy", "status.npy"]
    assert got["status"].dtype == np.float32 and got["status"].tolist() == [0, 3, 0, 0]
    assert got["len"].dtype == np.float64 and got["len"].tolist() == [3, 0, 0, 4]
    assert got["data"].dtype == np.float32 and got["data"].tolist() == [110, 111, 112, 106, 107, 108, 109]
    n = 5000
    st, ln = np.zeros(n, np.int32), np.full(n, 8, np.uint64)
    off = (np.arange(n, dtype=np.uint64)[::-1] * 8).copy()
    data = np.random.default_rng(1).integers(0, 256, 8 * n, dtype=np.uint8).tobytes()
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), st, off, ln, data, budget=30000)
    total = 0
    for k in ("status", "len", "data"):
        b, c = np.load(tmp_path / "b" / f"{k}.npy"), np.load(tmp_path / "c" / f"{k}.npy")
        assert b.tobytes() == c.tobytes()
        total += b.nbytes
    assert total <= 30000
    assert np.load(tmp_path / "b" / "status.npy").size == 2500   # each array over its 10 000-byte share is cut to it


def test_partition_matches_shard_of():
    import sys
    sys.path.insert(0, ROOT)
    from hocuspocus_amd.shard import shard_of
    from tools import synth
    for world in (2, 3, 8):
        parts = [set(synth.partition("c4-", 500, world, r).tolist()) for r in range(world)]
        assert sum(map(len, parts)) == 500 and set().union(*parts) == set(range(500))
        for r, p in enumerate(parts):
            assert all(shard_of(f"c4-{i}", world) == r for i in p)
