"""Static check that the plain ADMM iteration of wave_kernel<N, 1> keeps its LDS reads in flight
(tools/isa_lds_trips.py): at one wave per SIMD every lgkmcnt(0) that closes one or two reads is a
full LDS round trip on the iteration's dependency chain.  The innermost loop holding the Q z block
must have none (the u phase of schur_solve had six at N = 10), without a spill, scratch, more LDS or
another occupancy than before (profiles/order_hint/resources.txt at N = 10, the parent's report in
profiles/lds_flight/ at every horizon).  N = 3, 6, 10: one, two and three register rounds.  CPU only
(hipcc -S, two compiles per horizon, the horizons in parallel)."""
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HORIZONS = [10, 6, 3]  # the long compile first


def _report(n):
    cmd = [sys.executable, os.path.join(REPO, "tools", "isa_lds_trips.py"), "--n", str(n), "--json"]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=1200)


@pytest.fixture(scope="module")
def reports():
    with ThreadPoolExecutor(min(3, os.cpu_count() or 1)) as ex:
        outs = list(ex.map(_report, HORIZONS))
    res = {}
    for n, o in zip(HORIZONS, outs):
        assert o.returncode == 0, f"N={n}:\n{o.stdout[-2000:]}{o.stderr[-2000:]}"
        res[n] = json.loads(o.stdout)
    return res


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(REPO, "profiles", "lds_flight", "lds_trips_parent.json")) as f:
        return {int(k): v for k, v in json.load(f).items()}


@pytest.mark.parametrize("n", HORIZONS)
def test_iteration_loop_has_no_short_drain(reports, parent, n):
    q = reports[n]["qz_loop"]
    print(f"N={n}: {q} (parent {parent[n]['qz_loop']})")
    assert q["newbcast_fmas"] == 64, "not the loop of the Q z block"
    assert q["short"] == 0
    assert q["reads"] == parent[n]["qz_loop"]["reads"], "the same reads, in another order"


@pytest.mark.parametrize("n", HORIZONS)
def test_resources_unchanged(reports, parent, n):
    r, p = reports[n]["resources"], parent[n]["resources"]
    assert r["vgpr_spill_count"] == 0 and r["private_segment"] == 0
    assert r["lds_bytes"] == p["lds_bytes"] and r["occupancy"] == p["occupancy"]
    assert r["vgpr_count"] <= p["vgpr_count"], "the register count must not rise"


def test_n10_matches_order_hint_resources(reports):
    txt = open(os.path.join(REPO, "profiles", "order_hint", "resources.txt")).read()
    blk = txt[txt.index("wave_kernelILi10ELi1E"):].split("--")[0]
    lds = int(re.search(r"LDS Size \[bytes/block\]:\s*(\d+)", blk).group(1))
    occ = int(re.search(r"Occupancy \[waves/SIMD\]:\s*(\d+)", blk).group(1))
    scr = int(re.search(r"ScratchSize \[bytes/lane\]:\s*(\d+)", blk).group(1))
    r = reports[10]["resources"]
    assert (r["lds_bytes"], r["occupancy"], r["private_segment"]) == (lds, occ, scr)
