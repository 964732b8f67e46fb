"""Many versions of few documents through the Node extension (packages/extension-gpu-merge/test/version_shared.js): a
live gc: false document with 8 versions and a second with 3, GpuMerge.restoreVersions called with the entries
interleaved -- results in entry order, byte for byte yjs's Y.createDocFromSnapshot path, through one
restoreVersionShared call with 2 states and 11 asks; a version ahead of its state rejects alone; an engine without
restoreVersionShared takes the pair path with the same result."""
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
    r = subprocess.run(["node", os.path.join(PKG, "test", "version_shared.js"), f"--{mode}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "passed" in r.stdout


@needs_node
def test_version_shared_cpu_double():
    run("cpu")


@needs_node
@pytest.mark.gpu
def test_version_shared_gpu_addon():
    assert os.path.exists(os.path.join(PKG, "build", "ygm_napi.node")), "N-API addon not built"
    run("gpu")
