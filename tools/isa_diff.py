#!/usr/bin/env python3
"""Compare two AMDGPU assembly files (hipcc --cuda-device-only -S) kernel by kernel.

  python tools/isa_diff.py A.s B.s [--ops K]

For every kernel symbol of either file: the instruction counts, whether the instruction streams are
equal (lines starting with ';' or '.', trailing comments, the __hip_cuid_ symbol and label names
dropped), whether they are equal up to a consistent renaming of registers, the per-opcode count
differences, and .vgpr_count / .agpr_count / .sgpr_spill_count / scratch / LDS of both.  The verdict
of a kernel is one of
  identical                 the same instructions, the same registers
  same up to renaming       the same instructions under one bijection of the v / a / s registers
  same opcodes, other order the same multiset of opcodes, in another order or with other operands
  opcodes differ (n)        n = sum over opcodes of |count A - count B|, each listed (at most K)
A generic diff: it knows no particular instruction.  Exit status 0 if every kernel is identical or
same up to renaming with equal resources, 1 otherwise.
"""
import argparse
import collections
import re
import shutil
import subprocess
import sys

RES_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_spill_count", ".private_segment_fixed_size",
            ".group_segment_fixed_size")
RES_NAMES = ("vgpr", "agpr", "sgpr_spill", "scratch", "lds")
REG = re.compile(r"\b([vas])(?:(\d+)|\[(\d+):(\d+)\])(?![\w\[])")
LABEL = re.compile(r"\.L\w+")


def instructions(body):
    """The instruction lines of a kernel body, comments and label names dropped."""
    out = []
    for raw in body.splitlines():
        s = raw.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":") or "__hip_cuid_" in s:
            continue
        out.append(LABEL.sub(".L", " ".join(s.split())))
    return out


def renamed(ins):
    """The stream with every register replaced by its class and order of first appearance."""
    seen = {}

    def canon(kind, num):
        return seen.setdefault((kind, num), "%s%d" % (kind, sum(1 for k in seen if k[0] == kind)))

    def sub(m):
        kind = m.group(1)
        if m.group(2) is not None:
            return canon(kind, int(m.group(2)))
        return "[" + ",".join(canon(kind, i) for i in range(int(m.group(3)), int(m.group(4)) + 1)) + "]"

    return [REG.sub(sub, x) for x in ins]


def parse(text):
    """{symbol: (instruction list, {resource: value})} of one assembly file."""
    res, cur, in_meta = {}, None, False
    for line in text.splitlines():
        if line.startswith("amdhsa.kernels:"):
            in_meta = True
        elif in_meta:
            m = re.match(r"^  ([- ]) (\.\w+):\s*(\S*)\s*$", line)
            if not m:
                if line and not line.startswith(" "):
                    in_meta = False
                continue
            if m.group(1) == "-":
                cur = {}
            if m.group(2) == ".name":
                res[m.group(3)] = cur
            if cur is not None:
                cur[m.group(2)] = m.group(3)
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        name = m.group(1)
        start = re.search(r"^%s:" % re.escape(name), text, re.M)
        if not start:
            continue
        end = text.find(".Lfunc_end", start.end())
        body = text[start.end():end if end >= 0 else len(text)]
        meta = res.get(name, {})
        out[name] = (instructions(body), {k: meta.get(k, "?") for k in RES_KEYS})
    return out


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool or not names:
        return {n: n for n in names}
    got = subprocess.run([tool, "-p"] + list(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, got)) if len(got) == len(names) else {n: n for n in names}


def compare(a, b, max_ops=40):
    """(report lines, number of kernels that moved) for two parse() results."""
    names = sorted(set(a) | set(b))
    pretty = demangle(names)
    lines, moved = [], 0
    for nm in names:
        if nm not in a or nm not in b:
            lines.append("%-44s only in %s" % (pretty[nm], "A" if nm in a else "B"))
            moved += 1
            continue
        (ia, ra), (ib, rb) = a[nm], b[nm]
        ca, cb = collections.Counter(x.split()[0] for x in ia), collections.Counter(x.split()[0] for x in ib)
        ops = {op: (ca[op], cb[op]) for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op]}
        if ia == ib:
            verdict = "identical"
        elif renamed(ia) == renamed(ib):
            verdict = "same up to renaming"
        elif not ops:
            verdict = "same opcodes, other order"
        else:
            verdict = "opcodes differ (%d)" % sum(abs(x - y) for x, y in ops.values())
        same_res = ra == rb
        if not same_res or verdict not in ("identical", "same up to renaming"):
            moved += 1
        lines.append("%-44s insns %6d/%6d  %s" % (pretty[nm], len(ia), len(ib), verdict))
        for tag, r in (("A", ra), ("B", rb)):
            lines.append("    %s: %s%s" % (tag, " ".join("%s %s" % (n, r[k]) for n, k in zip(RES_NAMES, RES_KEYS)),
                                           "" if same_res or tag == "A" else "   <- resources differ"))
        for op, (x, y) in list(ops.items())[:max_ops]:
            lines.append("    %-28s %6d -> %6d" % (op, x, y))
        if len(ops) > max_ops:
            lines.append("    ... %d more opcodes" % (len(ops) - max_ops))
    return lines, moved


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--ops", type=int, default=40, help="opcode differences listed per kernel")
    args = ap.parse_args()
    lines, moved = compare(parse(open(args.a).read()), parse(open(args.b).read()), args.ops)
    print("\n".join(lines))
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
