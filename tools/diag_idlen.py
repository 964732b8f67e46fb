"""Documents taking the narrow lean kernel's five-byte-id parse, counted by the diagnostic build (libygm_diag.so;
tooling, not product) and set against the corpus on the CPU: the benchmark's C2 documents and every corpus of
tests/test_lean_idlen.py, on a default context and on one opened under YGM_LN_NO_IDLEN=1 (which must count none).
The CPU side applies the kernel's test to the bytes: a document passes when every update with structs has bytes 2 .. 5
with the top bit and byte 6 without (no update of these corpora is shorter than seven bytes).  Through the device
API, one launch per corpus.  Exit status 1 when a count differs.

    make -C hocuspocus_amd/csrc diag && python tools/diag_idlen.py [n_docs]"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hocuspocus_amd.engine as eng  # noqa: E402

eng.LIB_PATH = os.path.join(ROOT, "hocuspocus_amd", "libygm_diag.so")
from tools import synth  # noqa: E402


def passes(us):
    return all(u[0] == 0 or (len(u) > 6 and all(b & 0x80 for b in u[2:6]) and not u[6] & 0x80) for u in us)


def corpora(n_docs):
    import test_lean_idlen as t
    idx = synth.partition("c2-", n_docs, 1, 0)
    a, o, d = synth.text_updates_docs(idx, 200)
    ups = synth.split(a, o)
    yield "c2 (%d documents)" % n_docs, [ups[d[i]:d[i + 1]] for i in range(n_docs)]
    for name, fn in (("bound", t._boundary_docs), ("foreign", t._one_foreign_docs), ("y70", lambda: t._fifth_byte_docs()[0]),
                     ("clocks", t._clock_docs), ("infos", t._info_docs), ("dsonly", t._ds_docs), ("mixed", t._mixed_row_docs),
                     ("long200", lambda: t._long_docs(200)), ("long255", lambda: t._long_docs(255))):
        yield name, fn()


def main():
    from devrun import run_merge
    n_docs = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    L = eng.lib()
    L.ygm_diag_id5_read.argtypes = [ctypes.c_void_p, ctypes.c_int]
    e = eng.Engine(0)
    os.environ["YGM_LN_NO_IDLEN"] = "1"
    g = eng.Engine(0)
    del os.environ["YGM_LN_NO_IDLEN"]
    buf = np.zeros(2, np.uint64)
    bad = 0
    for name, docs in corpora(n_docs):
        want = sum(passes(us) for us in docs)
        got = []
        for ctx in (e, g):
            L.ygm_diag_id5_read(buf.ctypes.data, 1)
            run_merge(ctx, docs, "lens")
            L.ygm_diag_id5_read(buf.ctypes.data, 0)
            got.append((int(buf[0]), int(buf[1])))
        ok = got[0] == (len(docs), want) and got[1] == (len(docs), 0)
        bad += not ok
        print(json.dumps({"corpus": name, "documents": len(docs), "expected_id5": want, "default_parsed_id5": got[0],
                          "no_idlen_parsed_id5": got[1], "ok": ok}), flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
