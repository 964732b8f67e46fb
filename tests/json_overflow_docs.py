"""Documents around the JSON kernel's overflow rerun (k_json's second launch), written out by hand so that their
ProseMirror JSON and the size of their workspace's output region are known by construction.

marks_doc(K, tail): the fragment `root` holds one <paragraph> with one XmlText; in it K pairs of (ContentFormat
m<i> = true, a one-character ContentString), then the string `tail`.  Every op repeats the marks set so far, so op i
lists m0..mi (the tail follows the last character with no format between them: toDelta joins it to that op's string):
the JSON grows with K^2 while the state grows with K.  One client, no deletes:

    struct        clock       info  origin        content
    XmlElement    0           07    (root name)   03 "paragraph"
    XmlText       1           07    parent 0      06
    format i      2 + 2i      86    1 + 2i        "m<i>" "true"        (i = 0: info 06, parent 1)
    string i      3 + 2i      84    2 + 2i        one character
    tail          2 + 2K      84    1 + 2K        tail                  (K = 0: info 04, parent 1)

caps_out restates the output region of a document's workspace from the documented layout (ygm_snapshot.hpp, caps_of:
n + 48 (3 S + 2 D + 4) + 16 (C + 1) + 64 for n bytes, S structs, D delete ranges, C clients); delta(doc) is
len(JSON) - caps_out: the document runs a second time exactly when delta > 0.  A '"' in the tail is one byte of input
and two of JSON, so quotes move delta by +1 each."""
import collections

from v1util import vu

CLIENT = 7
ROOT = b"default"
ABSENT = b"no-such-root"
EMPTY = b'{"type":"doc","content":[]}'
HASHED_KEY = b"c--AbCd012+"            # a mark name newer y-prosemirror versions rewrite: YGM_EUNSUPPORTED
FLOAT_VAL = b'{"pt":10.5}'             # a number JSON.stringify writes with a fraction: YGM_ENONCANON

# name: what the document is; u: the update; ask: the root name asked; status, json: what ygm_json_v1 gives
# (json b"" when refused); rerun: the document's JSON outgrows its workspace and is not refused before the end;
# delta: len(JSON of the document's own root) - caps_out
Doc = collections.namedtuple("Doc", "name u ask status json rerun delta")


def letters(n, salt):
    return bytes(97 + (i * 7 + salt) % 26 for i in range(n))


def _vs(b):
    return vu(len(b)) + b


def _key(K, i, last_key):
    return last_key if last_key is not None and i == K - 1 else b"m%d" % i


def _val(K, i, val, last_val):
    return last_val if last_val is not None and i == K - 1 else val


def _ch(i):
    return bytes([65 + i % 26])


def marks_doc(K, tail=b"z", val=b"true", root=ROOT, last_key=None, last_val=None):
    """The update.  val: every mark's value (JSON text); last_key / last_val replace the last mark's name / value."""
    el = b"\x07\x01" + _vs(root) + b"\x03" + _vs(b"paragraph")
    tx = b"\x07\x00" + vu(CLIENT) + vu(0) + b"\x06"
    items = []
    for i in range(K):
        head = b"\x06\x00" + vu(CLIENT) + vu(1) if i == 0 else b"\x86" + vu(CLIENT) + vu(1 + 2 * i)
        items.append(head + _vs(_key(K, i, last_key)) + _vs(_val(K, i, val, last_val)))
        items.append(b"\x84" + vu(CLIENT) + vu(2 + 2 * i) + _vs(_ch(i)))
    if tail:
        head = b"\x04\x00" + vu(CLIENT) + vu(1) if K == 0 else b"\x84" + vu(CLIENT) + vu(1 + 2 * K)
        items.append(head + _vs(tail))
    return b"\x01" + vu(2 + len(items)) + vu(CLIENT) + b"\x00" + el + tx + b"".join(items) + b"\x00"


def expect(K, tail=b"z", val=b"true", root=ROOT, last_key=None, last_val=None):
    """The JSON of root `root` (tail: ASCII at or above 0x20; only '"' and '\\' are escaped)."""
    def marks(n):
        return b",".join(b'{"type":"' + _key(K, j, last_key) + b'","attrs":' + _val(K, j, val, last_val) + b"}" for j in range(n))

    def op(text, n):
        return b'{"type":"text","text":"' + text + b'"' + (b',"marks":[' + marks(n) + b"]" if n else b"") + b"}"
    esc = tail.replace(b"\\", b"\\\\").replace(b'"', b'\\"')
    ops = [op(_ch(i) + (esc if i == K - 1 else b""), i + 1) for i in range(K)]      # (no format before the tail: one string)
    if tail and K == 0:
        ops.append(op(esc, 0))
    return b'{"type":"doc","content":[{"type":"paragraph","content":[' + b",".join(ops) + b"]}]}"


def structs(K, tail=b"z"):
    return 2 + 2 * K + (1 if tail else 0)


def caps_out(n, S, D=0, C=1):
    return n + 48 * (3 * S + 2 * D + 4) + 16 * (C + 1) + 64


def al16(x):
    return (x + 15) // 16 * 16


def family(name, K, tail=b"z", root=ROOT, ask=None, status=0, **kw):
    """A Doc of the family.  status != 0: the refusal its last mark earns once the walk reaches it; ask: a root name
    the document does not have (the 27-byte empty document).  delta is that of the document's own root either way."""
    u = marks_doc(K, tail, root=root, **kw)
    js = expect(K, tail, root=root, **kw)
    dl = len(js) - caps_out(len(u), structs(K, tail))
    if ask is not None and ask != root:
        return Doc(name, u, ask, 0, EMPTY, False, dl)
    return Doc(name, u, root, status, js if status == 0 else b"", dl > 0 and status == 0, dl)


def delta(doc):
    """len(JSON of the document's own root) - caps_out."""
    return doc.delta


# ---- the filler: a paragraph of plain text, of a given size in bytes (as tests/test_docstage_gpu.py's para_doc)
def para_doc(n, salt=0, root=ROOT):
    s = letters(n, salt)
    el = b"\x07\x01" + _vs(root) + b"\x03" + _vs(b"paragraph")
    tx = b"\x07\x00" + vu(CLIENT) + vu(0) + b"\x06"
    st = b"\x04\x00" + vu(CLIENT) + vu(1) + vu(n) + s
    return b"\x01\x03" + vu(CLIENT) + b"\x00" + el + tx + st + b"\x00"


def para_json(n, salt=0):
    return b'{"type":"doc","content":[{"type":"paragraph","content":[{"type":"text","text":"' + letters(n, salt) + b'"}]}]}'


def filler(nbytes, salt=0, root=ROOT):
    """A fitting document of exactly nbytes bytes (its JSON is shorter than twice its state)."""
    n = nbytes - len(para_doc(0, salt, root))
    while n > 0 and len(para_doc(n, salt, root)) > nbytes:
        n -= 1
    u = para_doc(n, salt, root)
    if len(u) != nbytes:      # (the length's varuint grew between n and n + 1: no document of that size)
        raise ValueError("no filler of %d bytes" % nbytes)
    js = para_json(n, salt)
    dl = len(js) - caps_out(len(u), 3)
    assert dl <= 0
    return Doc("filler %d bytes salt %d root %d" % (nbytes, salt, len(root)), u, root, 0, js, False, dl)


# ---- the named families
def fit(salt=0, root=ROOT):
    """A small document with marks that fits (K = 3)."""
    return family("fits K 3 salt %d root %d" % (salt, len(root)), 3, b"fit-" + letters(5, salt), root=root)


def sweep():
    """K = 21 with q quotes in the tail, q = 8..31: delta = q - 12, every value from -4 to +19."""
    return [family("sweep K 21 q %d" % q, 21, b'"' * q) for q in range(8, 32)]


def grid(n, root=ROOT):
    """n distinct overflow documents: K cycles 22..40, the tail is salted so that no two JSONs are equal."""
    return [family("grid %d K %d root %d" % (i, 22 + i % 19, len(root)), 22 + i % 19, b"g%d-" % i + letters(3 + i % 5, i), root=root)
            for i in range(n)]


def late_refusals():
    """K = 30: the JSON passes the cap (delta > 0 at K = 22 already), then the last mark is refused: never listed."""
    return [family("late refusal: a hashed last key", 30, last_key=HASHED_KEY, status=9),
            family("late refusal: a float in the last value", 30, last_val=FLOAT_VAL, status=3)]


def no_tail():
    return family("K 30 without a tail", 30, b"")


def absent_ask():
    """The same overflow-capable document asked for a root it does not have: the 27-byte empty document, no rerun."""
    return family("K 30 without a tail, absent root", 30, b"", ask=ABSENT)


def big(salt=0):
    return family("big K 64 salt %d" % salt, 64, b"big-" + letters(2, salt))


def plain():
    return [family("K %d tail z" % k, k) for k in (0, 1, 21, 22, 64)] + [family("K 0 without a tail", 0, b"")]


def named_roots():
    """Overflow and fitting documents under root names of 1, 7 and 130 bytes."""
    out = []
    for root in (b"r", ROOT, b"n" * 130):
        out += grid(3, root) + [fit(1, root)]
    return out


def unique():
    """Every distinct (document, asked root) of the families above, once."""
    docs = (plain() + sweep() + grid(65) + late_refusals() + [no_tail(), absent_ask(), big(0), big(1)] +
            [fit(s) for s in range(4)] + named_roots())
    seen, out = set(), []
    for d in docs:
        if (d.u, d.ask) not in seen:
            seen.add((d.u, d.ask))
            out.append(d)
    return out


# ---- the fixture: yjs's answers (tests/golden/json_overflow_v135.json.gz, tools/json_overflow_fixture.py)
def states():
    """The distinct states of unique(), in order: row i of the fixture's "states" belongs to states()[i]."""
    out = []
    for d in unique():
        if d.u not in out:
            out.append(d.u)
    return out


_cache = {}


def load():
    import gzip
    import json
    import os
    if "fix" not in _cache:
        _cache["fix"] = json.load(gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "json_overflow_v135.json.gz"), "rt"))
    return _cache["fix"]


def built_rows():
    """json_fixture rows (label, state, name, status, bytes | None, sha256, length) of the by-construction states:
    per state its root and the absent name, as yjs answers."""
    import json_fixture as jf
    fix, sts = load(), states()
    assert len(fix["states"]) == len(sts)
    return [jf._row("state %d" % i, sts[i], r) for i, roots in enumerate(fix["states"]) for r in roots]


def session_rows():
    """json_fixture rows of the boundary sessions (yjs-made; each asked by its root and by the absent name)."""
    import json_fixture as jf
    return [jf._row(e["note"], bytes.fromhex(e["state"]), r) for e in load()["sessions"] for r in e["roots"]]
