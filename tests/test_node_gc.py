"""Documents created with gc: false through the Node extension (packages/extension-gpu-merge/test/gc.js): GpuMerge stores
the bytes yjs holds for a Y.Doc({gc: false}) -- a snapshot from before a deletion still restores the text after a
reload -- beside a garbage-collected document in the same store window, and SyncResponder answers both with the
reference's own encodeStateAsUpdate(doc, sv)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "packages", "extension-gpu-merge")
BUNDLE = "/opt/conda/share/jupyter/lab/static/3502.fbe0c610be82ba1360db.js"
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(BUNDLE),
                                reason="node or the bundled yjs (test oracle) not present")


def run(mode):
    r = subprocess.run(["node", os.path.join(PKG, "test", "gc.js"), f"--{mode}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "passed" in r.stdout


@needs_node
def test_gc_option_cpu_double():
    run("cpu")


@needs_node
@pytest.mark.gpu
def test_gc_option_gpu_addon():
    assert os.path.exists(os.path.join(PKG, "build", "ygm_napi.node")), "N-API addon not built"
    run("gpu")
