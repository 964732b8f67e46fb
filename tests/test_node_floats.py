"""Non-integer numbers through the Node extension (packages/extension-gpu-merge/test/floats.js): a whiteboard document
(shapes with x: 103.5, y: 40.25) and a Tiptap document (lineHeight 1.5, a { pt: 10.5 } mark) -- with `floats: true`
GpuMerge.sharedJsonOf, jsonOf and versionSharedJson equal JSON.stringify on yjs's own document, without the option the
documents are left out and named ENONCANON as before; --gpu adds the addon opened with and without the option against
tests/golden/floats_v135.json.gz and V8's strings of tests/golden/dtoa_v8.json.gz."""
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
    r = subprocess.run(["node", os.path.join(PKG, "test", "floats.js"), f"--{mode}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "passed" in r.stdout


@needs_node
def test_floats_cpu_double():
    run("cpu")


@needs_node
@pytest.mark.gpu
def test_floats_gpu_addon():
    assert os.path.exists(os.path.join(PKG, "build", "ygm_napi.node")), "N-API addon not built"
    run("gpu")
