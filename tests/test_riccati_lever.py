"""The gravity-weight lever of tests/test_gpu_riccati_horizons.py, pinned on the CPU oracle.

launch_wave's schur_ok() (csrc/mpcqp_wave.hip) walks all 13 state weights, so a handle with
q_weights[12] < 0 runs wave_kernel<N, 0> (the Riccati form) for the whole batch at N <= 10 too.
State 12 is the constant gravity state: its rows of B_d are zero and x0[12] - x_ref[12] is zero at
every step, so its weight enters neither H nor g, and the kernels read q_weights[0..11] only.  The QP
with q_weights[12] = -1 is therefore the QP of the default weights.  This file pins that claim bitwise
on the oracle (build_qp and the whole solve) at every horizon, which is what lets the GPU tests compare
a lever handle with the oracle's default-weight run.  No device."""
import numpy as np
import pytest

import mpcqp

B = 4


def _lever_q(oracle):
    q = list(oracle.GO1_Q)
    q[12] = -1.0
    return q


def test_lever_weights_are_the_defaults_but_for_gravity(oracle):
    q = _lever_q(oracle)
    assert len(q) == 13 and q[:12] == list(oracle.GO1_Q)[:12] and oracle.GO1_Q[12] == 0.0
    assert list(mpcqp.default_params(10).q_weights) == list(oracle.GO1_Q)
    assert list(oracle.default_params(10, q=q).q_weights) == q


@pytest.mark.parametrize("N", range(1, 21))
def test_gravity_weight_changes_nothing(oracle, N):
    recs = mpcqp.assemble_compute_grf(mpcqp.synthetic_go1(B, seed=500 + N, gait="mixed", mixed_mu=True), N)
    dflt, lever = oracle.default_params(N), oracle.default_params(N, q=_lever_q(oracle))
    assert recs.shape[0] == B
    for b in range(B):
        for name, a, c in zip("PgluA", oracle.build_qp(dflt, recs[b]), oracle.build_qp(lever, recs[b])):
            assert np.array_equal(a.view(np.uint64), c.view(np.uint64)), f"N={N} robot {b}: {name} differs"
    (ra, sa), (rl, sl) = (oracle.solve_batch(p, recs, nthreads=4, want_solution=True) for p in (dflt, lever))
    assert np.all(ra["status"] == 1), "the pin must cover solved QPs"
    assert ra.tobytes() == rl.tobytes(), f"N={N}: results differ"
    assert sa.tobytes() == sl.tobytes(), f"N={N}: solutions differ"
