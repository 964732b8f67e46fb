"""What a Map / Array / Text document is, through the Node extension (packages/extension-gpu-merge/test/tojson.js): a
live board document (a Y.Map of cards holding nested maps, arrays, texts and timestamps) -- GpuMerge.sharedJsonOf equals
JSON.stringify(getMap(root).toJSON()) on the live document, with parse, GpuMerge.versionSharedJson on a restored
version equals it on Y.createDocFromSnapshot, a document holding binary content is left out and named in
`unserialized`; --gpu adds the addon's `toJson` entry against the fixture's edge sessions and the pool's routing."""
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
    r = subprocess.run(["node", os.path.join(PKG, "test", "tojson.js"), f"--{mode}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "passed" in r.stdout


@needs_node
def test_tojson_cpu_double():
    run("cpu")


@needs_node
@pytest.mark.gpu
def test_tojson_gpu_addon():
    assert os.path.exists(os.path.join(PKG, "build", "ygm_napi.node")), "N-API addon not built"
    run("gpu")
