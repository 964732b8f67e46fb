"""ctypes binding of libygm.so (include/ygm.h) -- the MI355X batched Yjs update engine.

Python mirror of the yjs update-level API that Hocuspocus's persistence and
sync path calls, batched over documents:

* ``Engine.merge_updates_batch(docs)``          per document ``Y.mergeUpdates(updates)``
* ``Engine.diff_update_batch(updates, svs)``    per document ``Y.diffUpdate(update, sv)``
* ``Engine.encode_state_vector_from_update_batch(updates)``
                                                 per document ``Y.encodeStateVectorFromUpdate``

Single-document helpers (``merge_updates`` ...) raise :class:`YjsError` where yjs
throws, mirroring the reference's error behaviour.  There is no CPU fallback:
if the HIP library is missing or no GPU is present, construction fails loudly.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("YGM_LIB") or os.path.join(_HERE, "libygm.so")  # YGM_LIB: experiment builds (tooling)

OK, EMALFORMED, ERANGE, ENONCANON, ESURROGATE, EDEPTH, ENOMEM, EDEVICE, EINVAL, EUNSUPPORTED = range(10)
STATUS_NAMES = {0: "OK", 1: "EMALFORMED", 2: "ERANGE", 3: "ENONCANON", 4: "ESURROGATE", 5: "EDEPTH",
                6: "ENOMEM", 7: "EDEVICE", 8: "EINVAL", 9: "EUNSUPPORTED"}
F_COMPAT_135 = 1
F_FORCE_SEQ = 2
F_FLOATS = 8      # YGM_F_FLOATS: the JSON calls write non-integer numbers (off by default: stored expectations do not move)
DOC_NO_GC = 1   # YGM_DOC_NO_GC: a document's option byte, the document is a Y.Doc({gc: false})
TEXT_FLAT, TEXT_DEEP = 0, 1   # YGM_TEXT_FLAT / YGM_TEXT_DEEP: the modes of ygm_text_v1
JSON_PROSEMIRROR = 0          # YGM_JSON_PROSEMIRROR: the one kind of ygm_json_v1
TOJSON_MAP, TOJSON_ARRAY, TOJSON_TEXT = 0, 1, 2   # YGM_TOJSON_MAP / _ARRAY / _TEXT: the kinds of ygm_tojson_v1


class YjsError(Exception):
    """Raised where yjs would throw (or where the engine refuses a document)."""

    def __init__(self, code: int):
        self.code = code
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {strerror(code)}")


class _Result(ctypes.Structure):
    _fields_ = [("data", ctypes.POINTER(ctypes.c_uint8)), ("off", ctypes.POINTER(ctypes.c_uint64)),
                ("len", ctypes.POINTER(ctypes.c_uint64)), ("status", ctypes.POINTER(ctypes.c_int32)),
                ("n_docs", ctypes.c_uint32), ("data_bytes", ctypes.c_uint64)]


class _DevResult(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("off", ctypes.c_void_p), ("len", ctypes.c_void_p),
                ("status", ctypes.c_void_p), ("data_bytes", ctypes.c_uint64), ("payload_bytes", ctypes.c_uint64)]


class Stats(ctypes.Structure):
    _fields_ = [("calls", ctypes.c_uint64), ("docs", ctypes.c_uint64), ("updates", ctypes.c_uint64),
                ("bytes_in", ctypes.c_uint64), ("bytes_out", ctypes.c_uint64), ("docs_fast", ctypes.c_uint64),
                ("docs_seq", ctypes.c_uint64), ("kernel_ms", ctypes.c_double), ("h2d_ms", ctypes.c_double),
                ("d2h_ms", ctypes.c_double),
                ("docs_lean", ctypes.c_uint64), ("lean_ms", ctypes.c_double),
                ("lean_launches", ctypes.c_uint64), ("docs_big", ctypes.c_uint64),
                ("docs_lean_wide", ctypes.c_uint64), ("host_syncs", ctypes.c_uint64),
                ("docs_pending", ctypes.c_uint64), ("docs_snapshot", ctypes.c_uint64)]


_lib = None

# ---- the C boundary: one entry per function include/ygm.h declares, in the header's order.  An entry is its argument
# kinds and its result kind; lib() sets argtypes / restype from it and tests/test_abi.py holds it against the header.
_KIND = {"p": ctypes.c_void_p, "u64": ctypes.c_uint64, "u32": ctypes.c_uint32, "int": ctypes.c_int,
         "res": ctypes.POINTER(_Result), "dres": ctypes.POINTER(_DevResult), "stats": ctypes.POINTER(Stats),
         "ctxp": ctypes.POINTER(ctypes.c_void_p)}
_RET = {"int": ctypes.c_int, "void": None, "str": ctypes.c_char_p}


def _sig(args, ret="int"):
    return tuple(args.split()), ret


def _dev_sig(sig, arena_bytes=True, out=True):
    """The device-resident form of a host shape: the first arena's byte count after it, a stream before the result."""
    args = list(sig[0][:-1])
    if arena_bytes:
        args.insert(2, "u64")
    return tuple(args + ["p"] + (["dres"] if out else [])), sig[1]


# the host shapes (each starts with the context)
UNARY = _sig("p p p u32 res")                  # arena, off, n
UNARY_OPT = _sig("p p p p u32 res")            # arena, off, opt, n
PAIR = _sig("p p p p p u32 res")               # arena, off, second arena, its off, n
PAIR_OPT = _sig("p p p p p p u32 res")         # a pair and one option array (where it stands: the header)
PAIR_U32 = _sig("p p p p p u32 u32 res")       # a pair, a mode / kind, n
MERGE = _sig("p p p p u32 u32 res")            # arena, upd_off, upd_doc, n_upd, n_docs
SHARED = _sig("p p p u32 p p p u32 res")       # states, off, n_states, second arena, its off, ask, n_asks
SHARED_OPT_STATE = _sig("p p p p u32 p p p u32 res")   # ... off, opt, n_states, ...
SHARED_OPT_ASK = _sig("p p p u32 p p p p u32 res")     # ... ask, opt, n_asks
MERGE_LENS = _sig("p p u64 p p p u32 u32 p dres")      # (device only) arena, bytes, doc_off, upd_len, doc_upd, n_upd, n_docs, stream

SIGNATURES = {
    "ygm_open": _sig("int u32 ctxp"),
    "ygm_close": _sig("p", "void"),
    "ygm_merge_v1": MERGE,
    "ygm_diff_v1": PAIR,
    "ygm_sv_from_update_v1": UNARY,
    "ygm_snapshot_v1": UNARY,
    "ygm_snapshot_opts_v1": UNARY_OPT,
    "ygm_contains_v1": PAIR,
    "ygm_text_v1": PAIR_U32,
    "ygm_json_v1": PAIR_U32,
    "ygm_json_fields_v1": PAIR_U32,
    "ygm_tojson_v1": PAIR_U32,
    "ygm_sync_step2_v1": PAIR,
    "ygm_sync_step2_opts_v1": PAIR_OPT,
    "ygm_version_take_v1": UNARY,
    "ygm_version_restore_v1": PAIR_OPT,
    "ygm_diff_shared_v1": SHARED,
    "ygm_sync_step2_shared_v1": SHARED,
    "ygm_sync_step2_shared_opts_v1": SHARED_OPT_STATE,
    "ygm_version_restore_shared_v1": SHARED_OPT_ASK,
    "ygm_merge_v2": MERGE,
    "ygm_diff_v2": PAIR,
    "ygm_sv_from_update_v2": UNARY,
    "ygm_convert_v1_to_v2": UNARY,
    "ygm_convert_v2_to_v1": UNARY,
    "ygm_merge_v1_device": _dev_sig(MERGE),
    "ygm_merge_v1_device_async": _dev_sig(MERGE, out=False),
    "ygm_merge_v1_device_finish": _sig("p dres"),
    "ygm_merge_v1_device_lens": MERGE_LENS,
    "ygm_merge_v1_device_lens_async": (MERGE_LENS[0][:-1], "int"),
    "ygm_diff_v1_device": _dev_sig(PAIR),
    "ygm_sv_from_update_v1_device": _dev_sig(UNARY),
    "ygm_snapshot_v1_device": _dev_sig(UNARY),
    "ygm_snapshot_opts_v1_device": _dev_sig(UNARY_OPT),
    "ygm_contains_v1_device": _dev_sig(PAIR, arena_bytes=False),
    "ygm_text_v1_device": _dev_sig(PAIR_U32),
    "ygm_json_v1_device": _dev_sig(PAIR_U32),
    "ygm_json_fields_v1_device": _dev_sig(PAIR_U32),
    "ygm_tojson_v1_device": _dev_sig(PAIR_U32),
    "ygm_sync_step2_v1_device": _dev_sig(PAIR),
    "ygm_sync_step2_opts_v1_device": _dev_sig(PAIR_OPT),
    "ygm_version_take_v1_device": _dev_sig(UNARY),
    "ygm_version_restore_v1_device": _dev_sig(PAIR_OPT, arena_bytes=False),
    "ygm_diff_shared_v1_device": _dev_sig(SHARED),
    "ygm_sync_step2_shared_v1_device": _dev_sig(SHARED),
    "ygm_sync_step2_shared_opts_v1_device": _dev_sig(SHARED_OPT_STATE),
    "ygm_version_restore_shared_v1_device": _dev_sig(SHARED_OPT_ASK),
    "ygm_merge_v2_device": _dev_sig(MERGE),
    "ygm_diff_v2_device": _dev_sig(PAIR),
    "ygm_sv_from_update_v2_device": _dev_sig(UNARY),
    "ygm_convert_v1_to_v2_device": _dev_sig(UNARY),
    "ygm_convert_v2_to_v1_device": _dev_sig(UNARY),
    "ygm_stats": _sig("p stats"),
    "ygm_strerror": _sig("int", "str"),
    "ygm_version": _sig("", "str"),
}
EXPORTS = tuple(SIGNATURES)   # every symbol include/ygm.h declares


def lib():
    """Loads libygm.so (raises OSError when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} missing: run __graft_entry__.build() (no CPU fallback exists)")
        # One HIP runtime per process: the torch wheel bundles its own libamdhip64.so.7 (same soname as
        # /opt/rocm's).  Whichever loads first serves both, and torch's CUDA init fails ("No HIP GPUs are
        # available") on the system copy -- so when torch is installed it loads first.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (args, ret) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = [_KIND[k] for k in args]
            fn.restype = _RET[ret]
        _lib = L
    return _lib


def strerror(code: int) -> str:
    return lib().ygm_strerror(code).decode()


def _check(st):
    """A batch call's (or one document's) status: anything but OK raises."""
    if st != OK:
        raise YjsError(st)


def _pack(blobs):
    arena = b"".join(blobs)
    off = np.zeros(len(blobs) + 1, dtype=np.uint64)
    if blobs:
        np.cumsum(np.fromiter((len(b) for b in blobs), dtype=np.uint64, count=len(blobs)), out=off[1:])
    return arena, off


def encode_fields(fields) -> bytes:
    """A document's field list for ygm_json_fields_v1: None or an empty list gives no bytes (every key of doc.share),
    names (str or bytes) give their lib0 varStrings back to back -- a varuint byte length, then the UTF-8 bytes."""
    out = bytearray()
    for f in fields or ():
        b = f.encode() if isinstance(f, str) else bytes(f)
        n = len(b)
        while n > 127:
            out.append(0x80 | (n & 127))
            n >>= 7
        out.append(n)
        out += b
    return bytes(out)


def _ptr(a):
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(ctypes.c_void_p)
    return ctypes.c_char_p(a) if a else None


# ---- argument helpers: each gives the C arguments of one logical input, to be spliced into a call
def _packed(blobs):
    """A list of byte strings as (arena or None, offset pointer)."""
    arena, off = _pack([bytes(b) for b in blobs])
    return arena or None, _ptr(off)


def _names(names):
    return _packed([n.encode() if isinstance(n, str) else n for n in names])


def _merge_input(docs):
    """Lists of updates per document in the packed form of a merge: arena, upd_off, upd_doc, n_docs."""
    upd_doc = np.asarray([d for d, ups in enumerate(docs) for _ in ups], dtype=np.uint32)
    return (*_pack([bytes(u) for ups in docs for u in ups]), upd_doc, len(docs))


def _opts(opts, n):
    """Per-document option bytes (YGM_DOC_NO_GC) from a bytes-like or a sequence of bools / ints, as a pointer to n
    bytes; None (no options, or n = 0) is the C API's NULL."""
    if opts is None:
        return None
    if isinstance(opts, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(opts), dtype=np.uint8).copy()
    else:
        a = np.ascontiguousarray(np.asarray([int(x) for x in opts], dtype=np.int64).astype(np.uint8))
    if len(a) != n:
        raise ValueError(f"{len(a)} option bytes for {n} documents")
    return _ptr(a) if n else None


def _asks(ask_state):
    """The ask -> state table of the shared forms as (u32 pointer or None, n_asks)."""
    ask = np.ascontiguousarray(np.asarray(ask_state, dtype=np.int64).astype(np.uint32))
    return _ptr(ask) if len(ask) else None, len(ask)


TAIL_PAD = 64   # readable bytes the kernels need after a device arena (include/ygm.h, "Tail padding")


def _dptr(x, need=0):
    """A device pointer: an int, or a tensor (then its allocation must hold `need` bytes)."""
    if hasattr(x, "data_ptr"):
        nbytes = x.numel() * x.element_size()
        if nbytes < need:
            raise ValueError(f"device buffer of {nbytes} bytes: the engine reads {need} (arena + {TAIL_PAD} bytes of tail padding)")
        return x.data_ptr()
    return int(x)


def _darena(d_arena, arena_bytes):
    """A device arena as (pointer, byte count); a tensor must also hold the tail padding."""
    return _dptr(d_arena, arena_bytes + TAIL_PAD), arena_bytes


def _dopt(d_opt, n):
    """Device-resident option bytes: None / 0 is NULL, a tensor must hold n bytes."""
    if d_opt is None or (not hasattr(d_opt, "data_ptr") and not d_opt):
        return None
    return _dptr(d_opt, n)


@dataclass
class DeviceResult:
    """Outputs left in HBM by a device-resident call (context-owned memory)."""
    data: int
    off: int
    len: int
    status: int
    data_bytes: int      # used extent of `data` (merge outputs sit in per-document slots)
    payload_bytes: int   # sum of the per-document output lengths


class Engine:
    """One engine context on one GPU (not thread-safe; one batch in flight)."""

    def __init__(self, device: int = 0, compat135: bool = False, force_seq: bool = False, floats: bool = False):
        flags = (F_COMPAT_135 if compat135 else 0) | (F_FORCE_SEQ if force_seq else 0) | (F_FLOATS if floats else 0)
        ctx = ctypes.c_void_p()
        _check(lib().ygm_open(device, flags, ctypes.byref(ctx)))
        self._ctx = ctx
        self.device = device

    def close(self):
        if getattr(self, "_ctx", None):
            lib().ygm_close(self._ctx)
            self._ctx = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ------------------------------------------------------------ the two call paths
    def _host(self, fn, *args) -> _Result:
        """A host-memory batch call fn(ctx, *args, &result): the context-owned result, valid until the next call."""
        res = _Result()
        _check(getattr(lib(), fn)(self._ctx, *args, ctypes.byref(res)))
        return res

    def _dev(self, fn, *args) -> DeviceResult:
        """A device-resident call fn(ctx, *args, &result)."""
        r = _DevResult()
        _check(getattr(lib(), fn)(self._ctx, *args, ctypes.byref(r)))
        return DeviceResult(r.data, r.off, r.len, r.status, r.data_bytes, r.payload_bytes)

    # ------------------------------------------------------------ results
    @staticmethod
    def _unpack(res: _Result):
        n = res.n_docs
        if n == 0:
            return []
        off = np.ctypeslib.as_array(res.off, shape=(n,))
        ln = np.ctypeslib.as_array(res.len, shape=(n,))
        status = np.ctypeslib.as_array(res.status, shape=(n,))
        data = ctypes.string_at(res.data, res.data_bytes) if res.data_bytes else b""
        out = []
        for d in range(n):
            st = int(status[d])
            if st == OK:
                o = int(off[d])
                out.append((OK, data[o:o + int(ln[d])]))
            else:
                out.append((st, None))
        return out

    @staticmethod
    def _raw(res: _Result):
        n = res.n_docs
        if n == 0:
            return (np.zeros(0, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint64), b"")
        return (np.ctypeslib.as_array(res.status, shape=(n,)), np.ctypeslib.as_array(res.off, shape=(n,)),
                np.ctypeslib.as_array(res.len, shape=(n,)), (ctypes.c_uint8 * max(res.data_bytes, 1)).from_address(ctypes.cast(res.data, ctypes.c_void_p).value))

    def _or_error(self, res: _Result):
        """Per document its bytes, or the YjsError of its refusal (the text / JSON calls)."""
        return [b if s == OK else YjsError(s) for s, b in self._unpack(res)]

    # ------------------------------------------------------------ batch API
    def merge_updates_batch(self, docs):
        """docs: list of lists of update bytes -> list of (status, merged bytes | None)."""
        return self._unpack(self._merge_packed(*_merge_input(docs)))

    def _merge_packed(self, arena, upd_off, upd_doc, n_docs, fn="ygm_merge_v1") -> _Result:
        return self._host(fn, _ptr(arena), _ptr(upd_off), _ptr(upd_doc), len(upd_doc), n_docs)

    def merge_packed(self, arena: np.ndarray, upd_off: np.ndarray, upd_doc: np.ndarray, n_docs: int):
        """Packed host-array form of merge_updates_batch (arena uint8, upd_off uint64, upd_doc uint32)."""
        return self._unpack(self._merge_packed(arena, upd_off, upd_doc, n_docs))

    def merge_packed_raw(self, arena: np.ndarray, upd_off: np.ndarray, upd_doc: np.ndarray, n_docs: int):
        """merge_packed without the per-document Python unpacking: (status, off, len, data) views of the
        context's pinned result buffers, valid until the next call on this engine."""
        return self._raw(self._merge_packed(arena, upd_off, upd_doc, n_docs))

    def _doc_packed(self, op, arena, doc_off, sv_arena=None, sv_off=None) -> _Result:
        n = len(doc_off) - 1
        if op == "diff":
            return self._host("ygm_diff_v1", _ptr(arena), _ptr(doc_off), _ptr(sv_arena), _ptr(sv_off), n)
        return self._host("ygm_sv_from_update_v1", _ptr(arena), _ptr(doc_off), n)

    def doc_packed_raw(self, op: str, arena: np.ndarray, doc_off: np.ndarray, sv_arena=None, sv_off=None):
        """Host-array SV ("sv") / diff ("diff") batch; result views as merge_packed_raw."""
        return self._raw(self._doc_packed(op, arena, doc_off, sv_arena, sv_off))

    def _unary(self, fn, updates):
        """fn over one list of byte strings -> list of (status, bytes | None)."""
        return self._unpack(self._host(fn, *_packed(updates), len(updates)))

    def _pair(self, fn, first, second):
        """fn over two lists of byte strings, one pair per document -> list of (status, bytes | None)."""
        return self._unpack(self._host(fn, *_packed(first), *_packed(second), len(first)))

    def diff_update_batch(self, updates, svs):
        return self._unpack(self._doc_packed("diff", *_pack([bytes(u) for u in updates]), *_pack([bytes(s) for s in svs])))

    def encode_state_vector_from_update_batch(self, updates):
        return self._unpack(self._doc_packed("sv", *_pack([bytes(u) for u in updates])))

    # ------------------------------------------------------------ update V2
    def merge_updates_v2_batch(self, docs):
        """Y.mergeUpdatesV2 per document: docs = list of lists of V2 updates -> list of (status, V2 bytes | None)."""
        return self._unpack(self._merge_packed(*_merge_input(docs), fn="ygm_merge_v2"))

    def diff_update_v2_batch(self, updates, svs):
        """Y.diffUpdateV2(update, sv) per document (V2 updates, V1-format state vectors)."""
        return self._pair("ygm_diff_v2", updates, svs)

    def _conv_packed(self, fn, arena, doc_off):
        """Packed host-array form of a unary V2 call (ygm_sv_from_update_v2 / ygm_convert_*): the raw _Result."""
        return self._host(fn, _ptr(arena), _ptr(doc_off), len(doc_off) - 1)

    def encode_state_vector_from_update_v2_batch(self, updates):
        """Y.encodeStateVectorFromUpdateV2 per update (the state vector is V1-encoded, as yjs's)."""
        return self._unary("ygm_sv_from_update_v2", updates)

    def convert_update_format_v1_to_v2_batch(self, updates):
        """yjs 13.6 Y.convertUpdateFormatV1ToV2 per update."""
        return self._unary("ygm_convert_v1_to_v2", updates)

    def convert_update_format_v2_to_v1_batch(self, updates):
        """yjs 13.6 Y.convertUpdateFormatV2ToV1 per update."""
        return self._unary("ygm_convert_v2_to_v1", updates)

    def merge_v2_device(self, d_arena, arena_bytes, d_upd_off, d_doc_upd, n_upd, n_docs, stream=0) -> "DeviceResult":
        return self._dev("ygm_merge_v2_device", *_darena(d_arena, arena_bytes), _dptr(d_upd_off), _dptr(d_doc_upd), n_upd, n_docs,
                         stream or None)

    def doc_v2_device(self, op, d_arena, arena_bytes, d_doc_off, n_docs, d_sv=None, d_sv_off=None, stream=0) -> "DeviceResult":
        """op: "diff" (d_sv / d_sv_off), "sv", "v1_to_v2", "v2_to_v1" -- the device-resident V2 calls."""
        a = _darena(d_arena, arena_bytes)
        if op == "diff":
            return self._dev("ygm_diff_v2_device", *a, _dptr(d_doc_off), _dptr(d_sv), _dptr(d_sv_off), n_docs, stream or None)
        fn = {"sv": "ygm_sv_from_update_v2_device", "v1_to_v2": "ygm_convert_v1_to_v2_device",
              "v2_to_v1": "ygm_convert_v2_to_v1_device"}[op]
        return self._dev(fn, *a, _dptr(d_doc_off), n_docs, stream or None)

    # ------------------------------------------------------------ yjs-shaped single calls
    def snapshot_batch(self, updates, opts=None):
        """Doc-normalized snapshots: Y.encodeStateAsUpdate(Y.applyUpdate(new Y.Doc(), u)) per update
        (ygm_snapshot_v1) -> list of (status, bytes | None); UNSUPPORTED marks documents outside the envelope.
        opts: one option per update (bytes-like, or bools / ints): DOC_NO_GC / True marks a document created with
        gc: false, whose snapshot is that of new Y.Doc({gc: false}) -- deleted content kept (ygm_snapshot_opts_v1,
        which without options is ygm_snapshot_v1)."""
        return self._unpack(self._host("ygm_snapshot_opts_v1", *_packed(updates), _opts(opts, len(updates)), len(updates)))

    def sync_step2_batch(self, states, svs, opts=None):
        """SyncStep2 payloads of stored documents: Y.encodeStateAsUpdate(doc, sv) for doc = Y.applyUpdate(new Y.Doc(),
        state) (MessageReceiver.ts:137-138; ygm_sync_step2_v1) -> list of (status, bytes | None); UNSUPPORTED marks
        documents outside the snapshot envelope.  opts as snapshot_batch, one per state (ygm_sync_step2_opts_v1)."""
        return self._unpack(self._host("ygm_sync_step2_opts_v1", *_packed(states), _opts(opts, len(states)), *_packed(svs), len(states)))

    def diff_update_shared_batch(self, updates, ask_doc, svs):
        """Y.diffUpdate(updates[ask_doc[a]], svs[a]) per ask a (ygm_diff_shared_v1): many state vectors answered from
        one update, which is uploaded once and read in place.  ask_doc is non-decreasing, each entry below
        len(updates); anything else raises YjsError(EINVAL).  -> list of (status, bytes | None) per ask."""
        if len(ask_doc) != len(svs):
            raise ValueError("one state index per state vector")
        return self._unpack(self._host("ygm_diff_shared_v1", *_packed(updates), len(updates), *_packed(svs), *_asks(ask_doc)))

    def sync_step2_shared_batch(self, states, ask_state, svs, opts=None):
        """SyncStep2 payloads of a reconnect storm (ygm_sync_step2_shared_v1): ask a is answered from
        states[ask_state[a]] with svs[a], byte for byte what sync_step2_batch gives for that pair, but every state
        is uploaded and snapshotted once however many asks name it.  ask_state as ask_doc in
        diff_update_shared_batch.  opts as snapshot_batch, one per state: a state's asks are all answered from its
        snapshot, so from its option (ygm_sync_step2_shared_opts_v1).  -> list of (status, bytes | None) per ask."""
        if len(ask_state) != len(svs):
            raise ValueError("one state index per state vector")
        return self._unpack(self._host("ygm_sync_step2_shared_opts_v1", *_packed(states), _opts(opts, len(states)), len(states),
                                       *_packed(svs), *_asks(ask_state)))

    def contains_batch(self, states, updates):
        """Read-only SyncStep2: Y.snapshotContainsUpdate(Y.snapshot(doc), update) per pair, `states` being the
        documents' normalized states (snapshot_batch) -> list of (status, bool | None)."""
        return [(s, None if s != OK else b == b"\x01") for s, b in self._pair("ygm_contains_v1", states, updates)]

    # ------------------------------------------------------------ plain text
    def text_batch(self, states, names, deep=False):
        """Plain text of stored documents (ygm_text_v1): for doc = Y.applyUpdate(new Y.Doc(), state), the UTF-8 of
        doc.getText(name).toString(), or with deep=True the walk that also descends into nested types (XmlFragment /
        Tiptap documents; one newline after each nested type) -> list of bytes, or a YjsError for a refused state.
        names: one root name per state (str or bytes).  A name the state has no root for gives b""."""
        if len(states) != len(names):
            raise ValueError("one root name per state")
        return self._or_error(self._host("ygm_text_v1", *_packed(states), *_names(names), TEXT_DEEP if deep else TEXT_FLAT, len(states)))

    def text_device(self, d_states, states_bytes, d_state_off, d_names, d_name_off, n_docs, deep=False, stream=0, mode=None) -> "DeviceResult":
        """Device-resident text batch (ygm_text_v1_device): the states arena followed by TAIL_PAD readable bytes;
        mode overrides deep (the raw YGM_TEXT_* value)."""
        m = (TEXT_DEEP if deep else TEXT_FLAT) if mode is None else int(mode)
        return self._dev("ygm_text_v1_device", *_darena(d_states, states_bytes), _dptr(d_state_off), _dptr(d_names), _dptr(d_name_off), m,
                         n_docs, stream or None)

    # ------------------------------------------------------------ ProseMirror JSON
    def json_batch(self, states, names, kind=JSON_PROSEMIRROR):
        """Stored documents as ProseMirror / Tiptap JSON (ygm_json_v1): for doc = Y.applyUpdate(new Y.Doc(), state),
        the UTF-8 of JSON.stringify(yXmlFragmentToProsemirrorJSON(doc.getXmlFragment(name))) -- what
        TiptapTransformer.fromYdoc(doc, name) returns -> list of bytes, or a YjsError for a refused document (the
        caller keeps its yjs path for it).  names: one root name per state (str or bytes).  A name the state has no
        root for gives b'{"type":"doc","content":[]}'."""
        if len(states) != len(names):
            raise ValueError("one root name per state")
        return self._or_error(self._host("ygm_json_v1", *_packed(states), *_names(names), int(kind), len(states)))

    def json_device(self, d_states, states_bytes, d_state_off, d_names, d_name_off, n_docs, kind=JSON_PROSEMIRROR, stream=0) -> "DeviceResult":
        """Device-resident JSON batch (ygm_json_v1_device): the states arena followed by TAIL_PAD readable bytes."""
        return self._dev("ygm_json_v1_device", *_darena(d_states, states_bytes), _dptr(d_state_off), _dptr(d_names), _dptr(d_name_off),
                         int(kind), n_docs, stream or None)

    def json_fields_batch(self, states, fields, kind=JSON_PROSEMIRROR):
        """Every asked field of stored documents as one JSON object (ygm_json_fields_v1): for
        doc = Y.applyUpdate(new Y.Doc(), state), the UTF-8 of JSON.stringify(TiptapTransformer.fromYdoc(doc, fields))
        -- the body of a change webhook -> list of bytes, or a YjsError for a refused document.  fields: per state
        None or [] (every key of doc.share) or a list of names (str or bytes); see encode_fields."""
        if len(states) != len(fields):
            raise ValueError("one field list per state")
        return self._or_error(self._host("ygm_json_fields_v1", *_packed(states), *_packed([encode_fields(f) for f in fields]), int(kind),
                                         len(states)))

    def json_fields_device(self, d_states, states_bytes, d_state_off, d_fields, d_field_off, n_docs, kind=JSON_PROSEMIRROR,
                           stream=0) -> "DeviceResult":
        """Device-resident form (ygm_json_fields_v1_device): the states arena followed by TAIL_PAD readable bytes; the
        field lists encoded as encode_fields does."""
        return self._dev("ygm_json_fields_v1_device", *_darena(d_states, states_bytes), _dptr(d_state_off), _dptr(d_fields),
                         _dptr(d_field_off), int(kind), n_docs, stream or None)

    # ------------------------------------------------------------ toJSON of Map / Array / Text roots
    def tojson_batch(self, states, names, kind):
        """toJSON of stored documents' Map, Array or Text roots (ygm_tojson_v1): for doc = Y.applyUpdate(new Y.Doc(),
        state), the UTF-8 of JSON.stringify(doc.getMap(name).toJSON()) (kind TOJSON_MAP), of getArray (TOJSON_ARRAY) or
        of getText (TOJSON_TEXT) -> list of bytes, or a YjsError for a refused document (the caller keeps its yjs path
        for it).  names: one root name per state (str or bytes).  A name the state has no root for gives b"{}", b"[]"
        or b'""'."""
        if len(states) != len(names):
            raise ValueError("one root name per state")
        return self._or_error(self._host("ygm_tojson_v1", *_packed(states), *_names(names), int(kind), len(states)))

    def tojson_device(self, d_states, states_bytes, d_state_off, d_names, d_name_off, n_docs, kind, stream=0) -> "DeviceResult":
        """Device-resident toJSON batch (ygm_tojson_v1_device): the states arena followed by TAIL_PAD readable bytes."""
        return self._dev("ygm_tojson_v1_device", *_darena(d_states, states_bytes), _dptr(d_state_off), _dptr(d_names), _dptr(d_name_off),
                         int(kind), n_docs, stream or None)

    # ------------------------------------------------------------ version history
    def take_version_batch(self, states):
        """Versions of stored documents: Y.encodeSnapshot(Y.snapshot(doc)) for doc = Y.applyUpdate(new Y.Doc(), state)
        (ygm_version_take_v1) -> list of (status, bytes | None).  A state with pending parts is seen through its
        integrated part, as Y.snapshot sees the store."""
        return self._unary("ygm_version_take_v1", states)

    def restore_version_batch(self, states, versions, opts=None):
        """Old versions of gc: false documents: Y.encodeStateAsUpdate(Y.createDocFromSnapshot(doc,
        Y.decodeSnapshot(version), newDoc)) for doc = Y.applyUpdate(new Y.Doc({gc: false}), state)
        (ygm_version_restore_v1) -> list of (status, bytes | None).  opts as snapshot_batch, one per pair: DOC_NO_GC /
        True restores into new Y.Doc({gc: false}).  To restore several versions of one document use
        restore_version_shared_batch: here its state is staged and snapshotted once per version."""
        if len(states) != len(versions):
            raise ValueError("one version per state")
        return self._unpack(self._host("ygm_version_restore_v1", *_packed(states), *_packed(versions), _opts(opts, len(states)), len(states)))

    def restore_version_shared_batch(self, states, ask_state, versions, opts=None):
        """Many versions restored from one stored state (ygm_version_restore_shared_v1): ask a restores versions[a] from
        states[ask_state[a]], byte for byte and status for status what restore_version_batch gives for that pair, but
        every state is uploaded and given its no-GC snapshot once however many asks name it.  ask_state as ask_doc in
        diff_update_shared_batch.  opts as snapshot_batch, one per ask: the option belongs to the restored document.
        -> list of (status, bytes | None) per ask."""
        if len(ask_state) != len(versions):
            raise ValueError("one state index per version")
        ask, n_asks = _asks(ask_state)
        return self._unpack(self._host("ygm_version_restore_shared_v1", *_packed(states), len(states), *_packed(versions), ask,
                                       _opts(opts, len(versions)), n_asks))

    def version_take_device(self, d_states, states_bytes, d_state_off, n_docs, stream=0) -> "DeviceResult":
        """Device-resident take batch (ygm_version_take_v1_device)."""
        return self._dev("ygm_version_take_v1_device", *_darena(d_states, states_bytes), _dptr(d_state_off), n_docs, stream or None)

    def version_restore_device(self, d_states, d_state_off, d_versions, d_version_off, n_docs, stream=0, d_restored_opt=0) -> "DeviceResult":
        """Device-resident restore batch (ygm_version_restore_v1_device): both arenas followed by TAIL_PAD readable
        bytes, d_versions 16-byte aligned; d_restored_opt: a device pointer / tensor of n_docs option bytes (0: none)."""
        return self._dev("ygm_version_restore_v1_device", _dptr(d_states), _dptr(d_state_off), _dptr(d_versions), _dptr(d_version_off),
                         _dopt(d_restored_opt, n_docs), n_docs, stream or None)

    def version_restore_shared_device(self, d_states, states_bytes, d_state_off, n_states, d_versions, d_version_off, d_ask_state, n_asks,
                                      stream=0, d_restored_opt=0) -> "DeviceResult":
        """Device-resident shared restore batch (ygm_version_restore_shared_v1_device): n_states states, n_asks versions,
        d_ask_state (u32) naming each ask's state; arenas as version_restore_device; d_restored_opt: a device pointer /
        tensor of n_asks option bytes (0: none).  Results are indexed by ask; an ask whose id is out of range or below
        its predecessor carries EINVAL."""
        return self._dev("ygm_version_restore_shared_v1_device", *_darena(d_states, states_bytes), _dptr(d_state_off), n_states,
                         _dptr(d_versions), _dptr(d_version_off), _dptr(d_ask_state), _dopt(d_restored_opt, n_asks), n_asks, stream or None)

    def snapshot_device(self, d_arena, arena_bytes, d_doc_off, n_docs, stream=0, d_doc_opt=0) -> "DeviceResult":
        """Device-resident snapshot batch; d_doc_opt: a device pointer / tensor of n_docs option bytes (0: none)."""
        return self._dev("ygm_snapshot_opts_v1_device", *_darena(d_arena, arena_bytes), _dptr(d_doc_off), _dopt(d_doc_opt, n_docs), n_docs,
                         stream or None)

    @staticmethod
    def _one(results):
        """The single-document form of a batch: its bytes, or the YjsError yjs would throw."""
        st, out = results[0]
        _check(st)
        return out

    def merge_updates(self, updates):
        return self._one(self.merge_updates_batch([list(updates)]))

    def diff_update(self, update, sv):
        return self._one(self.diff_update_batch([update], [sv]))

    def encode_state_vector_from_update(self, update):
        return self._one(self.encode_state_vector_from_update_batch([update]))

    # ------------------------------------------------------------ device-resident API
    def merge_device(self, d_arena: int, arena_bytes: int, d_upd_off: int, d_doc_upd: int, n_upd: int, n_docs: int,
                     stream: int = 0) -> DeviceResult:
        return self._dev("ygm_merge_v1_device", *_darena(d_arena, arena_bytes), _dptr(d_upd_off), _dptr(d_doc_upd), n_upd, n_docs,
                         stream or None)

    def merge_device_async(self, d_arena: int, arena_bytes: int, d_upd_off: int, d_doc_upd: int, n_upd: int, n_docs: int,
                           stream: int = 0) -> None:
        """Enqueues a device-resident batch merge without waiting (ygm_merge_v1_device_async)."""
        _check(lib().ygm_merge_v1_device_async(self._ctx, *_darena(d_arena, arena_bytes), _dptr(d_upd_off), _dptr(d_doc_upd), n_upd, n_docs,
                                               stream or None))

    def merge_device_lens(self, d_arena: int, arena_bytes: int, d_doc_off: int, d_upd_len: int, d_doc_upd: int, n_upd: int,
                          n_docs: int, stream: int = 0) -> DeviceResult:
        """The compact input form (ygm_merge_v1_device_lens): u64 offset per document, u16 length per update."""
        return self._dev("ygm_merge_v1_device_lens", *_darena(d_arena, arena_bytes), _dptr(d_doc_off), _dptr(d_upd_len), _dptr(d_doc_upd),
                         n_upd, n_docs, stream or None)

    def merge_device_lens_async(self, d_arena: int, arena_bytes: int, d_doc_off: int, d_upd_len: int, d_doc_upd: int, n_upd: int,
                                n_docs: int, stream: int = 0) -> None:
        _check(lib().ygm_merge_v1_device_lens_async(self._ctx, *_darena(d_arena, arena_bytes), _dptr(d_doc_off), _dptr(d_upd_len),
                                                    _dptr(d_doc_upd), n_upd, n_docs, stream or None))

    def merge_device_finish(self) -> DeviceResult:
        """Completes the last enqueued batch (sequential tier, fault check, payload) -- ygm_merge_v1_device_finish."""
        return self._dev("ygm_merge_v1_device_finish")

    def diff_device(self, d_arena, arena_bytes, d_doc_off, d_sv, d_sv_off, n_docs, stream=0) -> DeviceResult:
        return self._dev("ygm_diff_v1_device", *_darena(d_arena, arena_bytes), _dptr(d_doc_off), _dptr(d_sv), _dptr(d_sv_off), n_docs,
                         stream or None)

    def sv_device(self, d_arena, arena_bytes, d_doc_off, n_docs, stream=0) -> DeviceResult:
        return self._dev("ygm_sv_from_update_v1_device", *_darena(d_arena, arena_bytes), _dptr(d_doc_off), n_docs, stream or None)

    def stats(self) -> Stats:
        s = Stats()
        lib().ygm_stats(self._ctx, ctypes.byref(s))
        return s
