"""The stored-document tests' file formats and host twins: the binary files exchanged with the node generators
(tools/snap_corpus.js, tools/snap_expect.js) and with the device code host-compiled under tools/snapdev (snapdev,
snaptext, versiondev), the build and run of those twins, and the steps the engine takes after the kernel (the pending
merge, the SyncStep2 reply from a snapshot's parts), done by the oracle.  A plain module: the CPU tests and the *_gpu.py
files of the snapshot, SyncStep2 and version families import it."""
import os
import shutil
import struct
import subprocess

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
BUNDLE = os.path.exists("/opt/conda/share/jupyter/lab/static/3502.fbe0c610be82ba1360db.js")
NOGC = 32   # snap::F_SNAP_NOGC, the host twins' mode bit


def write_in(path, us):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(us)))
        for u in us:
            f.write(struct.pack("<I", len(u)))
            f.write(u)


def read_res(path):
    b = open(path, "rb").read()
    i, out = 0, []
    while i < len(b):
        st, ln = struct.unpack_from("<iI", b, i)
        i += 8
        out.append((st, b[i:i + ln]))
        i += ln
    return out


def read_in(path):
    b = open(path, "rb").read()
    n = struct.unpack_from("<I", b, 0)[0]
    i, out = 4, []
    for _ in range(n):
        ln = struct.unpack_from("<I", b, i)[0]
        i += 4
        out.append(b[i:i + ln])
        i += ln
    return out


def write_pairs(path, pairs):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(pairs)))
        for s, v in pairs:
            f.write(struct.pack("<I", len(s)) + s + struct.pack("<I", len(v)) + v)


def _resolve_pending(st, body, compat135):
    """A host-compiled kernel result: status 64 (snap::ST_PEND) carries PendHdr + [state, pendingDs, pending structs],
    which the engine merges with the merge kernels -- here the oracle's mergeUpdates does that step."""
    if st != 64:
        return st, body
    ln = struct.unpack_from("<IIII", body, 0)
    assert ln[3] == 0x444E4550
    parts, p = [], 16
    for k in range(3):
        parts.append(body[p:p + ln[k]])
        p += ln[k]
    return oracle.merge_updates(parts, compat135=compat135)


def build_twin(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "snapdev", name + ".cpp")], check=True, timeout=300)
    return exe


def run_snaptext(exe, tmp_path, updates, flags, budget):
    """-> (taken indices, 'equals the general code' per document, the text path's results)"""
    a, b = str(tmp_path / "tin.bin"), str(tmp_path / "tout.bin")
    write_in(a, updates)
    r = subprocess.run([exe, a, str(flags), str(budget), b], check=True, timeout=120, capture_output=True, text=True)
    lines = [tuple(map(int, x.split())) for x in r.stdout.split("\n") if x]
    return [k for k, (t, _, _) in enumerate(lines) if t], [eq for _, _, eq in lines], read_res(b)


def run_twin(tmp_path, pairs, mode):
    """versiondev over (state, version) pairs -> per pair (take, cut, restored, restored_nogc), each (status, bytes)"""
    exe = str(tmp_path / "versiondev")
    if not os.path.exists(exe):
        subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "snapdev", "versiondev.cpp")], check=True, timeout=300)
    a, b = str(tmp_path / "vin.bin"), str(tmp_path / "vout.bin")
    write_pairs(a, pairs)
    subprocess.run([exe, a, b, str(mode)], check=True, timeout=300)
    r = read_res(b)
    assert len(r) == 4 * len(pairs)
    return [tuple(r[4 * k:4 * k + 4]) for k in range(len(pairs))]


def _kernel_outputs(tmp_path, states, mode):
    """snapdev over the states -> (status, bytes) per state"""
    exe = str(tmp_path / "snapdev")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "snapdev", "snapdev.cpp")], check=True, timeout=300)
    a, b = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_in(a, states)
    subprocess.run([exe, a, b, str(mode)], check=True, timeout=120)
    return read_res(b)


def _parts_reply(body, st, sv, compat135):
    """The reply from the kernel code's output: a complete state's snapshot diffed keeping the bit; a pending one's
    three parts (PendHdr) diffed (state: keeping the bit, pending structs: plain) and merged -- the engine's steps."""
    if st == 0:
        return oracle.diff_update(body, sv, compat135=compat135, keep_sub=True)
    assert st == 64
    ln = struct.unpack_from("<IIII", body, 0)
    a, b, c = body[16:16 + ln[0]], body[16 + ln[0]:16 + ln[0] + ln[1]], body[16 + ln[0] + ln[1]:16 + ln[0] + ln[1] + ln[2]]
    sa, da = oracle.diff_update(a, sv, compat135=compat135, keep_sub=True)
    sc, dc = oracle.diff_update(c, sv, compat135=compat135)
    if sa or sc:
        return (sa or sc), None
    return oracle.merge_updates([da, b, dc], compat135=compat135)
