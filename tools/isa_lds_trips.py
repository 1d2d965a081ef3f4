#!/usr/bin/env python3
"""Static count of the LDS round trips of wave_kernel<N, KS>: at one wave per SIMD nothing hides an
LDS wait, so what matters is how many times the code drains the LDS queue (s_waitcnt lgkmcnt(0)) for
the sake of one or two reads.  Two compiles of csrc/mpcqp_wave.hip for one horizon, with the
Makefile's code generation flags (in parallel):

  with -DMPCQP_ISA_MARKS   per marked phase (between consecutive WV_MARK ids in program order)
  the product build        the innermost loop that holds the 64 row_newbcast FMAs of q = Q z (the plain
                           ADMM iteration), which the marks would perturb

and for each the four counts
  reads    LDS read instructions (ds_read*)
  waits    s_waitcnt with an lgkmcnt field
  drains   of those, lgkmcnt(0)
  short    drains that close a group of one or two reads: the reads issued since the previous
           lgkmcnt(0) (a batch waited for with counted waits, lgkmcnt(8) .. (0), is one group)
plus the kernel's registers, spills, scratch, LDS size and occupancy.

  python tools/isa_lds_trips.py [--n 10] [--ks 1] [--defs -DFOO] [--src other/mpcqp_wave.hip] [--json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "go1-qp-mpc-controller_amd", "csrc", "mpcqp_wave.hip")
KEYS = ("reads", "waits", "drains", "short")
LGKM = re.compile(r"lgkmcnt\((\d+)\)")
QZ_FMAS = 64  # q = Q z: four mv16 blocks


def compile_asm(n, defs, out, src=SRC, marks=False):
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-strict-aliasing",
           "-mllvm", "-amdgpu-mfma-vgpr-form", f"-DMPCQP_WAVE_FOR_EACH_N(X)=X({n})", "--cuda-device-only", "-S", src,
           "-o", out] + (["-DMPCQP_ISA_MARKS"] if marks else []) + defs
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


def kernel_body(text, n, ks):
    m = re.search(r"^(_ZN5mpcqp2wv11wave_kernelILi%dELi%dEE\S*):" % (n, ks), text, re.M)
    if not m:
        raise SystemExit("wave_kernel<%d, %d> is not in the assembly" % (n, ks))
    end = text.index(".Lfunc_end", m.end())
    return m.group(1), text[m.end():end].splitlines(), text[end:]


class Trips:
    """The four counts of a straight run of instructions."""

    def __init__(self):
        self.c = dict.fromkeys(KEYS, 0)
        self.group = 0  # reads since the last drain

    def feed(self, ins):
        op = ins.split()[0]
        if op.startswith("ds_read"):
            self.c["reads"] += 1
            self.group += 1
        elif op == "s_waitcnt":
            m = LGKM.search(ins)
            if m:
                self.c["waits"] += 1
                if int(m.group(1)) == 0:
                    self.c["drains"] += 1
                    if 1 <= self.group <= 2:
                        self.c["short"] += 1
                    self.group = 0


def lines_of(body):
    """(kind, text) per line: 'mark', 'label' or 'ins'."""
    for raw in body:
        t = raw.strip()
        mm = re.match(r";WV_MARK (\d+)", t)
        if mm:
            yield "mark", mm.group(1)
            continue
        t = t.split(";")[0].strip()
        if not t or t.startswith(("//", ".")) and not t.endswith(":"):
            continue
        if t.endswith(":"):
            yield "label", t[:-1]
        else:
            yield "ins", t


def phases(body):
    """[(segment name, counts)] between consecutive marks in program order."""
    rows, seg, cur = [], "entry", Trips()
    for kind, t in lines_of(body):
        if kind == "mark":
            rows.append((seg + " -> " + t, cur.c))
            seg, cur = t, Trips()
        elif kind == "ins":
            cur.feed(t)
    rows.append((seg + " -> end", cur.c))
    return rows


def qz_loop(body):
    """Counts, instruction count and label of the innermost loop (label .. backward branch to it)
    that holds the Q z block's row_newbcast FMAs."""
    seq = list(lines_of(body))
    at = {t: i for i, (kind, t) in enumerate(seq) if kind == "label"}
    best = None
    for i, (kind, t) in enumerate(seq):
        if kind != "ins" or not t.startswith(("s_cbranch", "s_branch")):
            continue
        lab = t.split()[-1]
        if lab in at and at[lab] < i:
            ins = [x for k, x in seq[at[lab]:i + 1] if k == "ins"]
            fmas = sum(1 for x in ins if x.startswith("v_fmac_f64_dpp") and "row_newbcast" in x)
            if fmas >= QZ_FMAS and (best is None or len(ins) < len(best[1])):
                best = (lab, ins, fmas)
    if best is None:
        raise SystemExit("no loop with the Q z block found")
    tr = Trips()
    for x in best[1]:
        tr.feed(x)
    return dict(tr.c, label=best[0], instructions=len(best[1]), newbcast_fmas=best[2])


def resources(sym, tail):
    """The kernel's metadata entry and the occupancy comment that follows its body."""
    out = {}
    occ = re.search(r";\s*Occupancy:\s*(\d+)", tail)
    out["occupancy"] = int(occ.group(1)) if occ else None
    meta = tail[tail.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in tail else ""
    for blk in re.split(r"^  - ", meta, flags=re.M)[1:]:
        if re.search(r"^\s*\.name:\s*%s\s*$" % re.escape(sym), blk, re.M):
            for key, name in ((".vgpr_count", "vgpr_count"), (".agpr_count", "agpr_count"),
                              (".vgpr_spill_count", "vgpr_spill_count"), (".sgpr_spill_count", "sgpr_spill_count"),
                              (".private_segment_fixed_size", "private_segment"),
                              (".group_segment_fixed_size", "lds_bytes")):
                m = re.search(r"^\s*%s:\s*(\d+)" % re.escape(key), blk, re.M)
                out[name] = int(m.group(1)) if m else None
    return out


def report(n, ks=1, defs=(), src=SRC, keep=None):
    d = keep or tempfile.mkdtemp()
    os.makedirs(d, exist_ok=True)
    marked, plain = os.path.join(d, "w_marks.s"), os.path.join(d, "w.s")
    with ThreadPoolExecutor(2) as ex:
        jobs = [ex.submit(compile_asm, n, list(defs), marked, src, True),
                ex.submit(compile_asm, n, list(defs), plain, src, False)]
        for j in jobs:
            j.result()
    _, body, _ = kernel_body(open(marked).read(), n, ks)
    sym, pbody, tail = kernel_body(open(plain).read(), n, ks)
    return {"kernel": "wave_kernel<%d, %d>" % (n, ks), "phases": [dict(c, segment=s) for s, c in phases(body)],
            "qz_loop": qz_loop(pbody), "resources": resources(sym, tail)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--ks", type=int, default=1)
    ap.add_argument("--defs", nargs="*", default=[])
    ap.add_argument("--src", default=SRC)
    ap.add_argument("--keep", default=None, help="directory that keeps the two assembly files")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    r = report(a.n, a.ks, a.defs, a.src, a.keep)
    if a.json:
        print(json.dumps(r, indent=1))
        return 0
    print(r["kernel"])
    print("%-12s" % "marks" + "".join("%8s" % k for k in KEYS))
    tot = dict.fromkeys(KEYS, 0)
    for row in r["phases"]:
        if any(row[k] for k in KEYS):
            print("%-12s" % row["segment"] + "".join("%8d" % row[k] for k in KEYS))
        for k in KEYS:
            tot[k] += row[k]
    print("%-12s" % "total" + "".join("%8d" % tot[k] for k in KEYS))
    q = r["qz_loop"]
    print("Q z loop (product build, %s, %d instructions, %d row_newbcast FMAs)" % (q["label"], q["instructions"],
                                                                                 q["newbcast_fmas"]))
    print("%-12s" % "" + "".join("%8d" % q[k] for k in KEYS))
    print("resources " + " ".join("%s=%s" % kv for kv in r["resources"].items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
