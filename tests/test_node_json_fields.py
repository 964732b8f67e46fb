"""Every field of a document as one object, through the Node extension
(packages/extension-gpu-merge/test/json_fields.js): GpuMerge.jsonOf with field null (the reference webhook's
fromYdoc(document)), with an array of names, and with the untouched string default; GpuMerge.versionJson with field
null; a refused document named in `unserialized`; --gpu adds the addon's `jsonFields` entry and the pool's routing."""
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
    r = subprocess.run(["node", os.path.join(PKG, "test", "json_fields.js"), f"--{mode}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "passed" in r.stdout


@needs_node
def test_json_fields_cpu_double():
    run("cpu")


@needs_node
@pytest.mark.gpu
def test_json_fields_gpu_addon():
    assert os.path.exists(os.path.join(PKG, "build", "ygm_napi.node")), "N-API addon not built"
    run("gpu")
