#!/usr/bin/env python3
"""Are the kernels of two builds the same machine code?  Compares two directories of device assembly (one .s per source:
`make -C sais_amd/csrc asm OBJDIR=<dir>`, i.e. the Makefile's flags with -S --cuda-device-only), kernel by kernel, paired by
symbol name wherever the kernel sits in either tree: its instruction stream and its .amdhsa_* descriptor lines (register counts,
LDS size, scratch size, accumulator offset).  Normalised away: comments, and the function number in local labels (.LBB<n>_<m>),
which counts the functions of a translation unit.
    tools/isa_diff.py <dir A> <dir B> [--json table.json --label=<build>] [--by-file]
--by-file pairs <stem>.s with <stem>.s instead of pooling each directory.  Exit status 1 when a kernel differs, is missing on one
side or is defined twice on one side.  A kernel that differs gets, in the table, what a refactor that may move registers and
address arithmetic has to keep: "descriptors_identical" and the counts of both builds per class of tools/asm_count.py (MFMA,
LDS, global memory) plus barriers and atomics."""
import argparse
import glob
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asm_count import classify  # noqa: E402

LABEL_FN = re.compile(r"\.L(BB|JTI|CPI|tmp|func_begin|func_end)\d+(_?)")


def kernels(path):
    """{symbol: (instruction lines, descriptor lines)} of one assembly file."""
    out, body, name, desc = {}, None, None, None
    bodies = {}
    for raw in open(path):
        line = raw.split(";", 1)[0].rstrip()
        s = line.strip()
        if not s:
            continue
        if desc is not None:                                   # inside .amdhsa_kernel ... .end_amdhsa_kernel
            if s == ".end_amdhsa_kernel":
                out[name] = (bodies[name], desc)
                desc = None
            else:
                desc.append(" ".join(s.split()))
            continue
        if s.startswith(".amdhsa_kernel "):
            name, desc = s.split()[1], []
            continue
        if body is not None:
            if s.startswith(".Lfunc_end"):
                body = None
            elif not s.startswith(".") or s.startswith(".L") and s.endswith(":"):
                body.append(LABEL_FN.sub(lambda m: ".L" + m.group(1) + m.group(2), " ".join(s.split())))
            continue
        m = re.match(r"^([A-Za-z_$][\w$.]*):$", s)
        if m and not s.startswith(".L"):
            body = bodies.setdefault(m.group(1), [])
    return out


def mix(body):
    """{class: count} of the instruction classes that a change of register assignment or address arithmetic leaves alone."""
    c = {"mfma": 0, "lds": 0, "vmem": 0, "barrier": 0, "atomic": 0}
    for line in body:
        op = line.split()[0]
        k = classify(op)
        if k in ("mfma", "lds", "vmem"):
            c[k] += 1
        c["barrier"] += op.startswith("s_barrier")
        c["atomic"] += "_atomic_" in op
    return c


def pool(files):
    found, twice = {}, []
    for f in files:
        for k, v in kernels(f).items():
            if k in found:
                twice.append(k)
            found[k] = v + (os.path.basename(f),)
    return found, twice


def compare(a_files, b_files):
    a, a2 = pool(a_files)
    b, b2 = pool(b_files)
    rows = []
    for k in sorted(set(a) | set(b)):
        ia = sum(1 for x in a[k][0] if not x.endswith(":")) if k in a else None
        ib = sum(1 for x in b[k][0] if not x.endswith(":")) if k in b else None
        same = k in a and k in b and a[k][0] == b[k][0] and a[k][1] == b[k][1]
        rows.append({"kernel": k, "file_a": a[k][2] if k in a else None, "file_b": b[k][2] if k in b else None,
                     "instructions_a": ia, "instructions_b": ib, "identical": same})
        if not same and k in a and k in b:
            rows[-1].update(descriptors_identical=a[k][1] == b[k][1], mix_a=mix(a[k][0]), mix_b=mix(b[k][0]))
    return rows, a2, b2


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--json", help="add this run's per-kernel table to a JSON file, under --label")
    ap.add_argument("--label", default="default", help="name of the run in the JSON file, e.g. the build's extra flags")
    ap.add_argument("--by-file", action="store_true")
    ap.add_argument("-q", "--quiet", action="store_true", help="print only the kernels that are not identical")
    args = ap.parse_args()
    fa, fb = sorted(glob.glob(os.path.join(args.dir_a, "*.s"))), sorted(glob.glob(os.path.join(args.dir_b, "*.s")))
    if args.by_file:
        stems = sorted({os.path.basename(f) for f in fa + fb})
        groups = [([f for f in fa if os.path.basename(f) == s], [f for f in fb if os.path.basename(f) == s]) for s in stems]
    else:
        groups = [(fa, fb)]
    rows, twice = [], []
    for ga, gb in groups:
        r, a2, b2 = compare(ga, gb)
        rows += r
        twice += ["A: " + k for k in a2] + ["B: " + k for k in b2]
    bad = [r for r in rows if not r["identical"]]
    for r in rows:
        if not args.quiet or not r["identical"]:
            print(f"{'same' if r['identical'] else 'DIFF':4s} {str(r['instructions_a']):>6s} {str(r['instructions_b']):>6s}  {r['kernel']}")
            if "mix_a" in r:
                print(f"     descriptors {'same' if r['descriptors_identical'] else 'DIFF'}, mix {'same' if r['mix_a'] == r['mix_b'] else 'DIFF'}"
                      f"  {r['mix_a']} / {r['mix_b']}")
    for k in twice:
        print("defined twice in", k)
    print(f"{len(rows)} kernels, {sum(r['instructions_a'] or 0 for r in rows)} / {sum(r['instructions_b'] or 0 for r in rows)} instructions, "
          f"{len(bad)} not identical, {len(twice)} defined twice")
    if args.json:                                              # one file collects several runs, each under its --label
        runs = json.load(open(args.json)) if os.path.exists(args.json) else {}
        runs[args.label] = {"kernels": len(rows), "instructions_a": sum(r["instructions_a"] or 0 for r in rows),
                            "instructions_b": sum(r["instructions_b"] or 0 for r in rows), "not_identical": len(bad),
                            "defined_twice": twice, "table": rows}
        with open(args.json, "w") as fh:
            json.dump(runs, fh, indent=0)
            fh.write("\n")
    sys.exit(1 if bad or twice else 0)


if __name__ == "__main__":
    main()
