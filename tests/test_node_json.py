"""What a document is, through the Node extension (packages/extension-gpu-merge/test/json.js): a live Tiptap-shaped
XmlFragment document (headings with a level attr, bold and link marks) -- GpuMerge.jsonOf equals the committed
restatement of y-prosemirror's serializer on the live document, GpuMerge.versionJson over three versions equals it on
Y.createDocFromSnapshot, a Y.Text document asked as a fragment is left out and named; --gpu adds the addon's `json`
entry and the pool's routing."""
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
    r = subprocess.run(["node", os.path.join(PKG, "test", "json.js"), f"--{mode}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "passed" in r.stdout


@needs_node
def test_json_cpu_double():
    run("cpu")


@needs_node
@pytest.mark.gpu
def test_json_gpu_addon():
    assert os.path.exists(os.path.join(PKG, "build", "ygm_napi.node")), "N-API addon not built"
    run("gpu")
