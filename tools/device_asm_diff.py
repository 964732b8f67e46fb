"""Device-code comparison of two csrc directories (tooling for refactors that must leave the kernels alone): compiles
every HIP source of each directory's Makefile SRC line for gfx950, device side only, to assembly; splits the text into
functions by their `.type NAME,@function` symbols (up to the function's `.size` line); strips comments, alignment
directives and the function number in block labels; compares function by function and prints one table row per source
-- functions in A / in B / identical -- and the names that differ.  Exit status 1 when any function differs or is
missing on one side.  Text comparison only: nothing is assembled, loaded or run.

    python tools/device_asm_diff.py A/csrc B/csrc [-DYGM_DIAG ...]"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S"]


def sources(csrc):
    with open(os.path.join(csrc, "Makefile")) as mk:
        return [s for s in re.search(r"^SRC\s*=(.*)$", mk.read(), re.M).group(1).split() if s.endswith(".hip")]


def assembly(job):
    csrc, src, defs, out = job
    r = subprocess.run([HIPCC, *FLAGS, *defs, "-o", out, src], cwd=csrc, capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{csrc}/{src}: {r.stderr}")
    with open(out) as f:
        return f.read()


def functions(text):
    """{name: normalised body} of every `.type NAME,@function` symbol"""
    out, name, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(rf"\s*\.size\s+{re.escape(name)},", line):
            out[name] = "\n".join(body)
            name = None
            continue
        line = line.split(";", 1)[0].rstrip()
        if not line or re.match(r"\s*\.(p2align|align|balign)\b", line):
            continue
        line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)
        body.append(re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line))
    return out


def main():
    dirs = [os.path.abspath(a) for a in sys.argv[1:] if not a.startswith("-")]
    defs = [a for a in sys.argv[1:] if a.startswith("-")]
    if len(dirs) != 2:
        sys.exit(__doc__)
    srcs = [sources(d) for d in dirs]
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(d, s, defs, os.path.join(tmp, f"{i}_{s}.s")) for i, d in enumerate(dirs) for s in srcs[i]]
        with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
            texts = dict(zip(((j[0], j[1]) for j in jobs), ex.map(assembly, jobs)))
    print(f"| source | functions A | functions B | identical |   ({' '.join(FLAGS + defs)})\n|---|---|---|---|")
    bad, tot = [], [0, 0, 0]
    for s in sorted(set(srcs[0]) | set(srcs[1]), key=lambda x: (srcs[1] + srcs[0]).index(x)):
        a, b = (functions(texts.get((d, s), "")) for d in dirs)
        same = [n for n in a if n in b and a[n] == b[n]]
        bad += [f"{s}: {n}" for n in sorted(set(a) | set(b)) if n not in same]
        print(f"| `{s}` | {len(a)} | {len(b)} | {len(same)} |")
        tot = [tot[0] + len(a), tot[1] + len(b), tot[2] + len(same)]
    print(f"| all | {tot[0]} | {tot[1]} | {tot[2]} |")
    for n in bad:
        print("differs:", n)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
