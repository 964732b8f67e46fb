"""The GPU tests' device harness: the one place under tests/ that uploads inputs from numpy, reads a DeviceResult back,
opens the module-scoped engines and compares a result with an expectation.  A plain module, imported by the *_gpu.py
files (and by the lean test files); torch and the engine are imported when a function runs, so importing it needs no GPU."""
import collections

import numpy as np
import pytest

THROWS = {1, 2, 4, 5}      # EMALFORMED, ERANGE, ESURROGATE, EDEPTH: yjs throws, any of them is an acceptable answer

# read_results(raw=True): status int32, off / len int64, data uint8 -- numpy arrays
Raw = collections.namedtuple("Raw", "status off len data")


def same(expected, got):
    """statuses agree (any throw == any throw) and bytes agree when OK."""
    if expected[0] in THROWS:
        return got[0] in THROWS
    return expected[0] == got[0] and expected[1] == got[1]


def to_device(*arrays):
    """numpy arrays -> torch tensors on cuda:0 (each copied first: np.frombuffer's views are read-only)."""
    import torch
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(a.copy()).to(dev) for a in arrays]


def upload(blobs, lead=0, tail=0x00):
    """The blobs back to back in one device arena, `lead` bytes of 0xEE before them and 64 bytes of `tail` after them
    -> (arena, u64 offsets, the arena's bytes up to the last blob's end)."""
    a = np.frombuffer(b"\xee" * lead + b"".join(blobs) + bytes([tail]) * 64, np.uint8)
    off = (lead + np.cumsum([0] + [len(u) for u in blobs])).astype(np.uint64)
    ta, to = to_device(a, off.view(np.int64))
    return ta, to, len(a) - 64


def read_results(r, n, sync=True, every=False, places=False, raw=False):
    """A DeviceResult of n documents -> [(status, bytes or None)]: a document's bytes where its status is 0.
    sync: wait for the device first (False where the caller has).  every: slice the bytes of every document, whatever its
    status.  places: return (results, offsets, lengths), the two as lists of int.  raw: return the four arrays (Raw)."""
    import bench
    if sync:
        import torch
        torch.cuda.synchronize()
    off = bench._d2h(r.off, n * 8).view(np.uint64)
    ln = bench._d2h(r.len, n * 8).view(np.uint64)
    st = bench._d2h(r.status, n * 4).view(np.int32)
    data = bench._d2h(r.data, int(r.data_bytes))
    if raw:
        return Raw(st, off.astype(np.int64), ln.astype(np.int64), data)
    data = data.tobytes()
    off, ln = [int(x) for x in off], [int(x) for x in ln]
    res = [(int(st[d]), data[off[d]:off[d] + ln[d]] if every or st[d] == 0 else None) for d in range(n)]
    return (res, off, ln) if places else res


def pack_updates(docs):
    """docs (lists of updates) -> blobs, arena (64 spare bytes after it), u16 update lengths (None when an update has
    64 KB or more), u64 update offsets, u32 first update per document, u64 document offsets."""
    blobs = [u for us in docs for u in us]
    a = np.frombuffer(b"".join(blobs) + bytes(64), np.uint8)
    lens = np.array([len(b) for b in blobs], np.uint16) if max(map(len, blobs), default=0) < 0x10000 else None
    off = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
    du = np.cumsum([0] + [len(us) for us in docs]).astype(np.uint32)
    doff = off[du]
    return blobs, a, lens, off, du, doff


def run_merge(eng, docs, form):
    """docs through the u64-offset device API ('off') or the compact one ('lens'): results, documents finished lean."""
    blobs, a, lens, off, du, doff = pack_updates(docs)
    ta, to, td, tdo = to_device(a, off.view(np.int64), du.view(np.int32), doff.view(np.int64))
    lean0 = eng.stats().docs_lean
    if form == "off":
        r = eng.merge_device(ta.data_ptr(), len(a) - 64, to.data_ptr(), td.data_ptr(), len(blobs), len(docs))
    else:
        assert lens is not None, "an update of 64 KB or more: the offset form only"
        tl, = to_device(lens.view(np.int16))
        r = eng.merge_device_lens(ta.data_ptr(), len(a) - 64, tdo.data_ptr(), tl.data_ptr(), td.data_ptr(), len(blobs), len(docs))
    res = read_results(r, len(docs))
    return res, eng.stats().docs_lean - lean0


def engine_fixture(**kw):
    """A module-scoped fixture that opens Engine(0, **kw) and closes it: `eng = engine_fixture()` in a test file."""
    @pytest.fixture(scope="module")
    def fixture():
        from hocuspocus_amd import Engine
        e = Engine(0, **kw)
        yield e
        e.close()
    return fixture


class Memo:
    """What a test module computes once and shares among its tests; every module makes its own (the keys are short and
    repeat from file to file)."""

    def __init__(self):
        self.kept = {}

    def get(self, key, fn):
        if key not in self.kept:
            self.kept[key] = fn()
        return self.kept[key]

    def expect(self, key, docs, compat135=False):
        """The oracle's results of a corpus, computed once and shared."""
        import oracle
        return self.get(("expect", key), lambda: [oracle.merge_updates(us, compat135=True) if compat135 else oracle.merge_updates(us) for us in docs])
