"""The staging and lane prologue that k_snap_count, k_snap, k_text and k_json share (ygm_docstage.hpp), and the host
waits of the workspace batch (ygm_engine.cpp: ws_flat, ws_plan, read_meta).

Every document here is written out by hand, so its outputs are known by construction:
  * a single Y.Text insert of n ASCII characters under root "default": its text is the string (both modes: the root
    holds no nested type) and its normalized snapshot is the input -- one client, one Item, an empty delete set;
  * an XmlFragment "default" holding one <paragraph> with one XmlText of n characters: its ProseMirror JSON is
    {"type":"doc","content":[{"type":"paragraph","content":[{"type":"text","text":"..."}]}]} (no attributes, no marks).

The staging test runs under YGM_SNAP_NOLDS=1 (the general tier takes every document; asserted from the tier line) and
places the documents in the arena byte by byte: a wave whose extent from its 16-aligned start is exactly the 40 960
staged bytes, the same wave one byte longer (unstaged), first documents 1, 15 and 16 bytes past an aligned address, a
last wave with fewer documents than a wave takes, one document alone, 1, 16 and 64 documents per wave (64: the whole
batch is one wave over the staging size, so the same documents run unstaged), and an empty document between valid
neighbours."""
import re

import numpy as np
import pytest

from devrun import engine_fixture, read_results
from v1util import vu

pytestmark = pytest.mark.gpu

STAGE = 40960        # docstage::STAGE
ROOT = b"default"
CLIENT = 7
LINES = {
    "snapshot": re.compile(r"^ygm snapshot tiers: docs (\d+) text_first (\d+) text_second (\d+) general (\d+) pending (\d+)$", re.M),
    "text": re.compile(r"^ygm text tiers: docs (\d+) flat_first (\d+) flat_second (\d+) general (\d+)$", re.M),
    "json": re.compile(r"^ygm json tiers: docs (\d+) general (\d+) overflow (\d+) overflow_bytes (\d+)$", re.M),
}
OPS = ("snapshot", "text_flat", "text_deep", "json")


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("YGM_TIER_COUNTS", "1")
    for k in ("YGM_SNAP_NOLDS", "YGM_SNAP_DPW", "YGM_CHUNK_MB"):
        monkeypatch.delenv(k, raising=False)


eng = engine_fixture(compat135=True)


def letters(n, salt):
    return bytes(97 + (i * 7 + salt) % 26 for i in range(n))


def text_doc(n, salt=0):
    """One client, one Item: ContentString of n characters, parent the root "default", no origins; no deletes."""
    s = letters(n, salt)
    return b"\x01\x01" + vu(CLIENT) + b"\x00" + b"\x04\x01" + vu(len(ROOT)) + ROOT + vu(n) + s + b"\x00"


def para_doc(n, salt=0):
    """Three Items of one client: XmlElement "paragraph" in the root fragment, XmlText in it, n characters in that."""
    s = letters(n, salt)
    el = b"\x07\x01" + vu(len(ROOT)) + ROOT + b"\x03" + vu(9) + b"paragraph"
    tx = b"\x07\x00" + vu(CLIENT) + vu(0) + b"\x06"
    st = b"\x04\x00" + vu(CLIENT) + vu(1) + vu(n) + s
    return b"\x01\x03" + vu(CLIENT) + b"\x00" + el + tx + st + b"\x00"


def expected(op, kind, n, salt):
    s = letters(n, salt)
    if op == "snapshot":
        return (text_doc if kind == "text" else para_doc)(n, salt)
    if op == "json":
        return b'{"type":"doc","content":[{"type":"paragraph","content":[{"type":"text","text":"' + s + b'"}]}]}'
    return s


def make(op):
    return para_doc if op == "json" else text_doc


def fitted(op, count, total):
    """`count` documents of `total` bytes together: equal lengths, the last two adjusted (a document grows by one
    byte per character, by two where the length's varuint grows)."""
    mk = make(op)
    n0 = total // count - len(mk(0)) - 2
    ns = [n0] * count
    for last in range(n0, n0 + 4096):
        for prev in (n0, n0 + 1):
            ns[-2], ns[-1] = prev, last
            if sum(len(mk(n, k)) for k, n in enumerate(ns)) == total:
                return ns
    raise AssertionError("no fit")


def run(eng, capfd, op, specs, lead):
    """One device call over documents specs = [(n characters | None for an empty document)], the first starting `lead`
    bytes into a 16-aligned arena -> [(status, bytes)], general count of the tier line."""
    import torch
    dev = torch.device("cuda", 0)
    mk = make(op)
    docs = [b"" if n is None else mk(n, k) for k, n in enumerate(specs)]
    n = len(docs)
    arena = np.frombuffer(b"\xee" * lead + b"".join(docs) + bytes(64), np.uint8).copy()
    off = (lead + np.cumsum([0] + [len(d) for d in docs])).astype(np.uint64)
    names = np.frombuffer(ROOT * n + bytes(64), np.uint8).copy()
    noff = (len(ROOT) * np.arange(n + 1)).astype(np.uint64)
    ta, to = torch.from_numpy(arena).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev)
    tn, tno = torch.from_numpy(names).to(dev), torch.from_numpy(noff.view(np.int64).copy()).to(dev)
    assert ta.data_ptr() % 16 == 0
    nbytes = int(off[-1])
    capfd.readouterr()
    if op == "snapshot":
        r = eng.snapshot_device(ta, nbytes, to, n)
    elif op == "json":
        r = eng.json_device(ta, nbytes, to, tn, tno, n)
    else:
        r = eng.text_device(ta, nbytes, to, tn, tno, n, deep=op == "text_deep")
    torch.cuda.synchronize()
    line = LINES[op.split("_")[0]].findall(capfd.readouterr().err)
    assert len(line) == 1, line
    general = int(line[0][3 if op != "json" else 1])
    return read_results(r, n, sync=False, every=True), general


def check(op, specs, res, general, what):
    from hocuspocus_amd.engine import EMALFORMED
    kind = "para" if op == "json" else "text"
    assert general == len(specs), (what, general)
    exp = [(EMALFORMED, b"") if n is None else (0, expected(op, kind, n, k)) for k, n in enumerate(specs)]
    bad = [k for k in range(len(specs)) if res[k] != exp[k]]
    assert not bad, (what, bad[:6], res[bad[0]][0], len(res[bad[0]][1]), len(exp[bad[0]][1]))


@pytest.mark.parametrize("op", OPS)
def test_staging_and_lane_prologue(eng, capfd, monkeypatch, op):
    monkeypatch.setenv("YGM_SNAP_NOLDS", "1")
    mk = make(op)
    tail = [40, 3, None, 1, 200]          # a second wave of fewer than 16 documents, an empty one among them
    for lead in (1, 15, 16):
        full = fitted(op, 16, STAGE - lead % 16)   # wave 0: exactly STAGE bytes from its 16-aligned start
        start16 = lead - lead % 16
        assert lead + sum(len(mk(n, k)) for k, n in enumerate(full)) - start16 == STAGE
        specs = full + tail
        per_dpw = {}
        for dpw in ("1", "16", "64"):
            monkeypatch.setenv("YGM_SNAP_DPW", dpw)
            res, general = run(eng, capfd, op, specs, lead)
            check(op, specs, res, general, (op, "lead", lead, "dpw", dpw))
            per_dpw[dpw] = res
        # 16 per wave: wave 0 staged; 64 per wave: the 21 documents are one wave over STAGE, unstaged
        assert per_dpw["16"] == per_dpw["64"] == per_dpw["1"]
    monkeypatch.setenv("YGM_SNAP_DPW", "16")
    # the same documents, one byte later: wave 0 extends STAGE + 1 bytes from its aligned start and runs unstaged
    full = fitted(op, 16, STAGE - 1)
    staged, g1 = run(eng, capfd, op, full + tail, 1)
    unstaged, g2 = run(eng, capfd, op, full + tail, 2)
    check(op, full + tail, staged, g1, (op, "extent", STAGE))
    check(op, full + tail, unstaged, g2, (op, "extent", STAGE + 1))
    assert staged == unstaged
    # one byte more in the wave's last document
    longer = full[:-1] + [full[-1] + 1]
    res, general = run(eng, capfd, op, longer + tail, 1)
    check(op, longer + tail, res, general, (op, "one character more"))
    # one document alone, and the default documents per wave
    monkeypatch.delenv("YGM_SNAP_DPW")
    for lead in (0, 1):
        res, general = run(eng, capfd, op, [33], lead)
        check(op, [33], res, general, (op, "one document", lead))
    res, general = run(eng, capfd, op, full + tail, 15)
    check(op, full + tail, res, general, (op, "default dpw"))


def syncs(eng, call):
    s0 = eng.stats().host_syncs
    res = call()
    return res, eng.stats().host_syncs - s0


@pytest.mark.parametrize("claimed", [True, False])
def test_host_syncs_per_call(eng, capfd, claimed):
    """The host waits of one call, counted in the engine's code (every read-back goes through read_meta or read_u64s,
    which count one wait each):
      ws_flat   one read of the tier's counters after each launch: 1 when the first launch claims every document,
                2 when documents remain after it (the 24 KiB launch runs and is read too)
      ws_plan   1: the scanned workspace total
      read_meta 1 after the general kernel (k_snap, k_text, k_json)
    snapshot, text: all claimed 1 (the general path is skipped); none claimed 2 + 1 + 1 = 4.
    JSON has no flat tier: ws_plan + read_meta = 2 either way.
    contains: 1 (the states' extent) + its snapshot batch (1 or 4) + its own ws_plan (1) = 3 or 6; k_cont is followed by
    no read.
    All claimed: single flat Y.Text inserts.  None claimed: the paragraph documents, whose nested types are outside
    the flat tiers' envelope (asked in the deep mode for the text)."""
    n = 5
    docs = [(text_doc if claimed else para_doc)(10 + k, k) for k in range(n)]
    names = [ROOT] * n
    want = {"snapshot": 1 if claimed else 4, "text": 1 if claimed else 4, "json": 2, "contains": 3 if claimed else 6}

    def tier(op):
        line = LINES[op].findall(capfd.readouterr().err)
        assert len(line) == 1, (op, line)
        return list(map(int, line[0]))

    capfd.readouterr()
    res, got = syncs(eng, lambda: eng.snapshot_batch(docs))
    t = tier("snapshot")
    assert [st for st, _ in res] == [0] * n and (t[1] == n if claimed else t[3] == n)
    assert got == want["snapshot"]

    res, got = syncs(eng, lambda: eng.text_batch(docs, names, deep=not claimed))
    t = tier("text")
    assert all(isinstance(b, bytes) for b in res) and (t[1] == n if claimed else t[3] == n)
    assert got == want["text"]

    res, got = syncs(eng, lambda: eng.json_batch(docs, names))
    t = tier("json")
    assert t[0] == t[1] == n and t[2] == 0
    assert got == want["json"]

    res, got = syncs(eng, lambda: eng.contains_batch(docs, docs))
    t = tier("snapshot")
    assert res == [(0, True)] * n and (t[1] == n if claimed else t[3] == n)
    assert got == want["contains"]
