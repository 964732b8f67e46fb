"""Runs the VALU issue-rate microbenchmark (tools/valu_rate.hip; tooling) on GPU 0 and writes its rows, one per
(instruction, waves per SIMD), as a JSON list.  The program is built by `make -C tools valu_rate` when it is missing.

    python tools/valu_rate.py [OUT.json]      (default profiles/lean_diet/valu_rate.json)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lean_diet", "valu_rate.json")
    exe = os.path.join(TOOLS, "valu_rate")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", TOOLS, "valu_rate"])
    text = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    rows = [json.loads(line) for line in text.splitlines() if line.startswith("{")]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    for r in rows:
        print(f"{r['inst']:26s} {r['waves_per_simd']} waves/SIMD: {r['cycles_per_inst_per_simd']:.2f} cycles per wave-instruction")


if __name__ == "__main__":
    main()
