"""Version history through the Node extension (packages/extension-gpu-merge/test/version.js): GpuMerge.takeVersions of two
live gc: false documents between edits, a store and a reload, and GpuMerge.restoreVersions bringing deleted text back,
byte for byte yjs's Y.createDocFromSnapshot path; a gc: true document's entry is rejected with yjs's own message and a
version ahead of its state fails alone."""
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
    r = subprocess.run(["node", os.path.join(PKG, "test", "version.js"), f"--{mode}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "passed" in r.stdout


@needs_node
def test_version_history_cpu_double():
    run("cpu")


@needs_node
@pytest.mark.gpu
def test_version_history_gpu_addon():
    assert os.path.exists(os.path.join(PKG, "build", "ygm_napi.node")), "N-API addon not built"
    run("gpu")
