"""The layout of tests/ ("Tests"): what two test files share lives in a plain module, so no file imports a
test module, and devrun.py alone reaches into the private functions of bench.py."""
import glob
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
IMPORTS_A_TEST = re.compile(r"^\s*(?:from\s+test_\w+\s+import|import\s+(?:\w+\s*,\s*)*test_\w+)", re.M)
BENCH_PRIVATE = re.compile(r"\bbench\._\w+")


def sources():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(HERE, "*.py")))}


def test_no_file_imports_a_test_module():
    bad = [name for name, src in sources().items() if IMPORTS_A_TEST.search(src)]
    assert not bad, bad


def test_bench_privates_are_read_in_devrun_alone():
    users = [name for name, src in sources().items() if BENCH_PRIVATE.search(src)]
    assert users == ["devrun.py"], users
