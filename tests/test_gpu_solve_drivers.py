"""GPU suite (-m gpu): the host drivers of the first-order solve (csrc/solve_plan.hpp, csrc/cfmm_hip.hip: solve_lbfgs) under the
switches that select them.  tests/envelope_worker.py runs once per mode, unchanged; its networks -- C2 (100 tokens, 1e4 pools) and
the mixed one (1000 tokens, 2e4 pools) -- take seconds.

Part A, the one-launch iteration:
    default              drive_eager, sealed envelope
    CFMM_ENVELOPE=classic drive_eager, synchronised envelope
    CFMM_ZERO_COPY=0     drive_eager, synchronised envelope, the result copied back
    CFMM_FUSED_GRAPH=1   drive_chunks replaying the one-launch iterations from a graph
Every mode's records `cold` and `mixed_cold` end with status 1 and a primal value within 2e-6 relative of the default mode's (the
project's tolerance for converged objectives, DESIGN (c)).  Beyond that every pair of modes is compared record by record with
test_gpu_envelope.same (evals, iters and status exactly, the rest to its RTOL) -- where the PARENT of the change that split
solve_lbfgs into drivers agrees under that rule; a refactor cannot be asked to agree where its parent does not.  The parent build
(commit f1f28ba), run once on an MI355X with this worker and these modes, agrees in ALL six pairs and in all eleven records of each:
evals, iters and status are equal everywhere (cold 22 / 21 / 1, at_optimum 1 / 0 / 1, budget_k k / k - 1 / 3, budget_exact 22 / 21 / 1,
mixed_cold 100 / 99 / 1, warm_after_update 93 / 92 / 1, other_utility 141 / 140 / 1), and the largest differences over all pairs and
records were dual value 4.1e-13, primal value 7.1e-13, gap 3.5e-13, infeasibility 2.1e-12, prices 6.2e-14, net trade 1.3e-11, tenders
3.6e-13 -- the arrival-order noise of the accumulators' floating-point atomics that test_gpu_envelope.py's docstring measures, two
orders below RTOL = 1e-9.  So no pair and no record is excepted.

Part B, the two-launch iteration (CFMM_FUSED=0): drive_chunks replaying a graph (CFMM_NO_GRAPH=0) against the same driver enqueuing
its chunks (CFMM_NO_GRAPH=1) -- status 1, equal evals, values to 1e-9, on both networks: the assertions of
test_gpu.py::test_eager_iteration_path_matches_graph_path."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_envelope import same

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

SWITCHES = ("CFMM_ENVELOPE", "CFMM_ZERO_COPY", "CFMM_FUSED_GRAPH", "CFMM_FUSED", "CFMM_NO_GRAPH")
MODES_A = {"default": {}, "classic": {"CFMM_ENVELOPE": "classic"}, "zero_copy_off": {"CFMM_ZERO_COPY": "0"}, "fused_graph": {"CFMM_FUSED_GRAPH": "1"}}
MODES_B = {"two_launch_graph": {"CFMM_FUSED": "0", "CFMM_NO_GRAPH": "0"}, "two_launch_eager": {"CFMM_FUSED": "0", "CFMM_NO_GRAPH": "1"}}
RECORDS = ("cold", "at_optimum", "budget_1", "budget_2", "budget_4", "budget_exact", "mixed_cold", "trades_cp2", "warm_after_update", "other_utility", "closed")
CONVERGED = ("cold", "mixed_cold")


def run_mode(d, name, switches):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    path = str(d / f"{name}.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "envelope_worker.py"), path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-2000:])
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def one_launch(tmp_path_factory):
    d = tmp_path_factory.mktemp("drivers_a")
    return {name: run_mode(d, name, sw) for name, sw in MODES_A.items()}


@pytest.fixture(scope="module")
def two_launch(tmp_path_factory):
    d = tmp_path_factory.mktemp("drivers_b")
    return {name: run_mode(d, name, sw) for name, sw in MODES_B.items()}


@pytest.mark.parametrize("record", CONVERGED)
@pytest.mark.parametrize("mode", list(MODES_A))
def test_one_launch_iteration_converges_under_every_switch(one_launch, mode, record):
    got, ref = one_launch[mode][record], one_launch["default"][record]
    print(mode, record, got[:7], "default", ref[:7])
    assert got[2] == 1.0, (mode, record, got[:7])
    assert abs(got[4] - ref[4]) <= 2e-6 * abs(ref[4]), (mode, record, got[4], ref[4])


@pytest.mark.parametrize("pair", list(itertools.combinations(MODES_A, 2)), ids="-".join)
def test_one_launch_iteration_modes_agree_where_the_parent_build_agrees(one_launch, pair):
    a, b = pair
    assert set(one_launch[a]) == set(one_launch[b]) == set(RECORDS)
    for record in RECORDS:                                   # (every one: the parent build agrees in all of them, module docstring)
        assert same(one_launch[a][record], one_launch[b][record]), (pair, record, one_launch[a][record][:7], one_launch[b][record][:7])


@pytest.mark.parametrize("record", CONVERGED)
def test_two_launch_iteration_replayed_matches_enqueued(two_launch, record):
    g, e = two_launch["two_launch_graph"][record], two_launch["two_launch_eager"][record]
    print(record, g[:7], e[:7])
    assert g[2] == 1.0 and e[2] == 1.0, (g[:7], e[:7])
    assert g[0] == e[0], (g[:7], e[:7])
    assert abs(g[3] - e[3]) <= 1e-9 * abs(g[3]) and abs(g[4] - e[4]) <= 1e-9 * abs(g[4]), (g[:7], e[:7])
