#!/usr/bin/env python3
"""What rust/patches/*.patch and rust/src/eval_hip.rs expect of the reference tree -> tests/golden/reference_patch_targets.json.

    python scripts/gen_reference_patch_targets.py <reference checkout>

For every patch and every hunk: the line of the reference file where the hunk's pre-image (context + removed lines) stands, and the
SHA-256 of those lines of the file; and the parameter list of eval_cpu::eval (src/eval_cpu.rs), which eval_hip::eval repeats.
tests/test_rust_shim.py checks against this fixture, so the checks need no copy of the reference.  A hunk whose pre-image is not in
the file exactly is an error here: the fixture only records patches that apply."""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCHES = os.path.join(ROOT, "rust", "patches")
OUT = os.path.join(ROOT, "tests", "golden", "reference_patch_targets.json")


def hunks(text):
    """-> (path the patch applies to, [(old_start, pre-image lines)]) of a one-file unified diff."""
    rel = re.match(r"--- a/(\S+)", text).group(1)
    out, left = [], 0
    for line in text.split("\n"):
        m = re.match(r"@@ -(\d+)(?:,(\d+))? \+\d+(?:,\d+)? @@", line)
        if m:
            out.append((int(m.group(1)), []))
            left = int(m.group(2) or 1)
        elif left and line[:1] in (" ", "-", ""):                # ("": a blank context line whose space an editor dropped)
            out[-1][1].append(line[1:])
            left -= 1
    return rel, out


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def main():
    ref = sys.argv[1]
    patches = {}
    for f in sorted(os.listdir(PATCHES)):
        if not f.endswith(".patch"):
            continue
        rel, hs = hunks(open(os.path.join(PATCHES, f)).read())
        lines = open(os.path.join(ref, rel)).read().split("\n")
        entry, at = [], 0
        for start, pre in hs:
            found = [i for i in range(at, len(lines) - len(pre) + 1) if lines[i:i + len(pre)] == pre]
            assert found, f"{f}: the hunk at line {start} is not in {rel}"
            i = min(found, key=lambda k: abs(k - (start - 1)))
            entry.append({"line": i + 1, "lines": len(pre), "sha256": digest(lines[i:i + len(pre)])})
            at = i + len(pre)
        patches[f] = {"file": rel, "hunks": entry}
    text = open(os.path.join(ref, "src", "eval_cpu.rs")).read()
    sig = re.search(r"pub fn eval<Fp: GpuFftField<FftField = Fp> \+ FftField, Fq: StarkExtensionOf<Fp>>\((.*?)\) -> Matrix<Fq>", text, re.S).group(1)
    fixture = {"patches": patches, "eval_cpu_eval_params": [p.strip() for p in sig.strip().rstrip(",").split(",\n")]}
    with open(OUT, "w") as fh:
        json.dump(fixture, fh, indent=1)
        fh.write("\n")
    print(OUT)


if __name__ == "__main__":
    main()
