"""Static check of the Schur factorization's code at every horizon it is compiled for (mpcqp_schur.h
schur_factor, N = 1..10), on the compiler's resource report and instruction counts only: no scratch
and no VGPR spill, the LDS size the parent had (profiles/schur_factor/isa_parent.json: the layout is
unchanged, WSmem<10, 1> = 40,880 B), one wave per SIMD, registers not above the parent's; and at
N = 10 the factorization (marks 25 .. 15 of a -DMPCQP_ISA_MARKS compile, tools/isa_lds_trips.py)
drains the LDS queue no more often than the parent's did.  CPU only (hipcc -S: one compile per
horizon and the marked one, in parallel).

  python tests/test_isa_schur_factor.py [SRC]   prints the record of SRC (default: this tree's source)"""
import json
import os
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_lds_trips as trips  # noqa: E402

HORIZONS = list(range(10, 0, -1))  # the long compiles first
FACTOR_MARKS = ("25", "21", "22", "23", "24", "13", "14")  # segments that start at these marks


def _one(job):
    n, marks, src, d = job
    out = os.path.join(d, f"w{n}{'_marks' if marks else ''}.s")
    trips.compile_asm(n, [], out, src, marks)
    sym, body, tail = trips.kernel_body(open(out).read(), n, 1)
    if not marks:
        return n, "resources", trips.resources(sym, tail)
    seen, total = set(), dict.fromkeys(trips.KEYS, 0)
    for seg, c in trips.phases(body):
        start = seg.split(" -> ")[0]
        if start in FACTOR_MARKS and seg not in seen:  # (the first copy: the code is there once)
            seen.add(seg)
            for k in trips.KEYS:
                total[k] += c[k]
    assert {s.split(" -> ")[0] for s in seen} >= {"25", "21", "14"}, f"factorization marks not found: {sorted(seen)}"
    return n, "factor", total


def record(src=trips.SRC):
    d = tempfile.mkdtemp()
    jobs = [(10, True, src, d)] + [(n, False, src, d) for n in HORIZONS]
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        outs = list(ex.map(_one, jobs))
    rec = {}
    for n, key, val in outs:
        rec.setdefault(str(n), {})[key] = val
    return rec


@pytest.fixture(scope="module")
def result():
    return record()


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(REPO, "profiles", "schur_factor", "isa_parent.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("n", HORIZONS)
def test_resources(result, parent, n):
    r, p = result[str(n)]["resources"], parent[str(n)]["resources"]
    print(f"N={n}: {r} (parent {p})")
    assert r["vgpr_spill_count"] == 0 and r["private_segment"] == 0
    assert r["lds_bytes"] == p["lds_bytes"]
    assert r["occupancy"] == 1 and p["occupancy"] == 1
    assert r["vgpr_count"] <= p["vgpr_count"], "VGPR + AGPR must not grow"


def test_wsmem_n10_size(result):
    assert result["10"]["resources"]["lds_bytes"] == 40880


def test_factorization_drains_n10(result, parent):
    f, p = result["10"]["factor"], parent["10"]["factor"]
    print(f"factorization, N=10: {f} (parent {p})")
    assert f["drains"] <= p["drains"]


if __name__ == "__main__":
    print(json.dumps(record(sys.argv[1] if len(sys.argv) > 1 else trips.SRC), indent=1))
