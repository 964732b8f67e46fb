"""Number::toString on the host (hocuspocus_amd/csrc/ygm_dtoa.hpp through tools/snapdev/dtoadev.cpp -- the arithmetic the
kernels run): against V8's strings (tests/golden/dtoa_v8.json.gz), against an independent reference built on Python's
repr over the edge list and 200 000 seeded random bit patterns, once more under the address and undefined-behaviour
sanitizers, and the generated table against its generator."""
import os
import random
import shutil
import struct
import subprocess
import sys

import pytest

import floats_fixture as ff

ROOT = ff.ROOT
NODE = shutil.which("node")
CSRC = os.path.join(ROOT, "hocuspocus_amd", "csrc")
RANDOM = 200000


def build(tmp_path_factory, name, flags):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", *flags, "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "snapdev", "dtoadev.cpp")], check=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def dtoadev(tmp_path_factory):
    return build(tmp_path_factory, "dtoadev", ["-O1"])


def strings(exe, raw, *args):
    out = subprocess.run([exe, *args], input=raw, stdout=subprocess.PIPE, check=True, timeout=600).stdout.decode().split("\n")
    assert out[-1] == ""
    return out[:-1]


def of_doubles(exe, xs):
    return strings(exe, b"".join(struct.pack("=d", x) for x in xs))


@pytest.fixture(scope="module")
def inputs():
    """The fixture's doubles (the edge list first) and 200 000 uniform random bit patterns, NaN and infinity removed."""
    rnd = random.Random(20251021)
    xs = [x for x, _ in ff.v8_doubles()]
    while len(xs) < len(ff.v8_doubles()) + RANDOM:
        b = rnd.getrandbits(64)
        if (b >> 52) & 0x7FF != 0x7FF:
            xs.append(struct.unpack("=d", struct.pack("=Q", b))[0])
    return xs


def test_fixture_holds_the_edge_list_and_random_patterns():
    fix = dict((s, x) for x, s in ff.v8_doubles())
    for s in ("5e-324", "2.2250738585072014e-308", "2.225073858507201e-308", "1.7976931348623157e+308", "0.1", "0.3", "0.30000000000000004",
              "4.35", "0.000001", "1e-7", "1.5e-7", "123456.789", "1e+21", "999999999999999900000", "1e+22", "1e+23",
              "9007199254740992", "9007199254740994", "1152921504606847000", "9223372036854776000", "18446744073709552000", "-1.5", "100.25",
              "0.5", "0.3333333333333333", "-0.0000027410441684333906", "0.10000000149011612", "3.4028234663852886e+38"):
        assert s in fix, s
    assert fix["2.2250738585072014e-308"] == 2.0 ** -1022 and fix["1152921504606847000"] == 2.0 ** 60
    zeros = [struct.pack(">d", x).hex() for x, s in ff.v8_doubles() if s == "0"]
    assert sorted(zeros) == ["0000000000000000", "8000000000000000"]
    pow2 = [x for x, _ in ff.v8_doubles()[:400] if x > 0 and struct.unpack(">Q", struct.pack(">d", x))[0] & ((1 << 52) - 1) == 0]
    assert len(pow2) > 100                                    # the narrow interval below a power of two
    assert len(ff.v8_doubles()) > 4000 and max(len(s) for _, s in ff.v8_doubles()) == 25
    f = dict((s, b) for b, s in ff.v8_floats())
    assert f["0.10000000149011612"] == 0x3DCCCCCD and f["16777216"] == 0x4B800000 and f["3.4028234663852886e+38"] == 0x7F7FFFFF
    assert f["1.401298464324817e-45"] == 1                   # the smallest subnormal float
    assert os.path.getsize(ff.DTOA_FIX) < (1 << 20)


def test_python_reference_agrees_with_the_whole_v8_fixture():
    bad = [(x.hex(), s, ff.js_number(x)) for x, s in ff.v8_doubles() if ff.js_number(x) != s]
    assert not bad, bad[:5]
    bad = [(hex(b), s) for b, s in ff.v8_floats() if ff.js_number(struct.unpack(">f", struct.pack(">I", b))[0]) != s]
    assert not bad, bad[:5]


def test_dtoadev_vs_v8(dtoadev):
    got = of_doubles(dtoadev, [x for x, _ in ff.v8_doubles()])
    bad = [(x.hex(), s, g) for (x, s), g in zip(ff.v8_doubles(), got) if g != s]
    assert len(got) == len(ff.v8_doubles()) and not bad, bad[:5]
    got = strings(dtoadev, b"".join(struct.pack("=I", b) for b, _ in ff.v8_floats()), "--f32")
    bad = [(hex(b), s, g) for (b, s), g in zip(ff.v8_floats(), got) if g != s]
    assert len(got) == len(ff.v8_floats()) and not bad, bad[:5]


def test_dtoadev_vs_python_reference_over_200000_random_doubles(dtoadev, inputs):
    got = of_doubles(dtoadev, inputs)
    assert len(got) == len(inputs) == len(ff.v8_doubles()) + RANDOM
    bad = [(x.hex(), g, ff.js_number(x)) for x, g in zip(inputs, got) if g != ff.js_number(x)]
    assert not bad, (len(bad), bad[:5])


def test_sanitizer_build_over_the_same_input(tmp_path_factory, inputs):
    """The stand-alone program built with -fsanitize=address,undefined and run directly: the table index, the shifts and
    the writer of exactly 25 bytes."""
    exe = build(tmp_path_factory, "dtoadev_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    got = of_doubles(exe, inputs)
    assert got == [ff.js_number(x) for x in inputs]
    assert strings(exe, b"".join(struct.pack("=I", b) for b, _ in ff.v8_floats()), "--f32") == [s for _, s in ff.v8_floats()]


def test_table_is_what_the_generator_writes():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_pow5.py"), "--stdout"], stdout=subprocess.PIPE, check=True, timeout=120).stdout
    with open(os.path.join(CSRC, "ygm_dtoa_pow5.inc"), "rb") as f:
        committed = f.read()
    assert out == committed
    assert committed.count(b"\n") == 1 + 617 and len(committed) < (1 << 20)


def test_header_uses_integer_arithmetic_only():
    src = open(os.path.join(CSRC, "ygm_dtoa.hpp")).read()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    for word in ("double", "float ", "printf", "long double"):
        assert word not in code, word
    assert "__umul64hi" in code and "unsigned __int128" in code and "__device__ const" in code and "__shared__" not in code


@pytest.mark.skipif(not NODE, reason="node is needed to regenerate")
def test_fixture_regenerates(tmp_path):
    out = str(tmp_path / "d.json.gz")
    subprocess.run([NODE, os.path.join(ROOT, "tools", "dtoa_corpus.js"), out], check=True, timeout=120, stdout=subprocess.DEVNULL)
    import gzip
    import json
    assert json.load(gzip.open(out, "rt")) == ff.load(ff.DTOA_FIX)
