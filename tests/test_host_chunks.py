"""The host API's chunk planners (hocuspocus_amd/csrc/ygm_chunks.hpp) on the CPU: tools/hostdev/chunks.cpp, a
stand-alone program built with the address and undefined-behaviour sanitizers, checks a few thousand random offset
tables per planner -- partition in order, the plain planner against a linear scan, the shared planner against the rules
its comment states, the empty cases.  The GPU side of the pipeline is tests/test_host_chunks_gpu.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_chunk_planners_under_sanitizers(tmp_path):
    exe = str(tmp_path / "chunks")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tools", "hostdev", "chunks.cpp")], check=True, timeout=300)
    r = subprocess.run([exe, "4000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"chunks ok: (\d+) plain plans, (\d+) shared plans, (\d+) chunks$", r.stdout.strip())
    assert m and int(m.group(1)) == 8000 and int(m.group(2)) == 4000 and int(m.group(3)) > 30000, r.stdout
