"""Every layout of the projected L-BFGS step against the twin, iterate by iterate (docs/step_parity.md).

One case = one layout on one scenario of tests/step_parity.py: the device solves from the scenario's start with max_evals = k for
k = 1 .. K, each solve from scratch, and every budget's (evals, iters, status) must EQUAL the twin's, its accepted prices and five
values agree within the tolerance measured on the twin (tests/test_step_parity_host.py proves that tolerance stable and three or more
orders of magnitude below what a wrong rule does on the same scenario).

Which layout runs is not reported by the library; `expected_layout` restates the selection of csrc/cfmm_hip.hip (tiny_applies,
fused_applies, launch_update, the update lambda of cfmm_solve_batch) from the same facts -- token count, memory, ties, utility kind,
reproducible mode and the context-level switches CFMM_TINY, CFMM_FUSED, CFMM_UPDATE_GENERIC, CFMM_UPDATE_VARIANT, which cfmm_create
reads: set before the context is built -- and every case asserts that the layout it names is the one that selection gives.
"""
import numpy as np
import pytest

import cfmm
from cfmm._lib import E_HIP
from cfmm.problem import Utility
import step_parity as sp

pytestmark = pytest.mark.gpu

SWITCHES = ("CFMM_TINY", "CFMM_FUSED", "CFMM_UPDATE_GENERIC", "CFMM_UPDATE_VARIANT", "CFMM_DETERMINISTIC", "CFMM_NO_GRAPH", "CFMM_UPD_GRID")
TWO = {"CFMM_FUSED": "0"}                 # the two-launch iteration: evaluation, then launch_update
NOTINY = {"CFMM_TINY": "0"}


def expected_layout(sc, env, det=False, batch=False):
    """csrc/cfmm_hip.hip, in the order plan_first_order (solve_plan.hpp) asks: tiny_applies, fused_applies, launch_update"""
    n, M = sc.n, sc.memory
    table, tied = sc.utility == "table", sc.ties
    generic = env.get("CFMM_UPDATE_GENERIC", "0") != "0"
    if batch:                             # cfmm_solve_batch: launch_update_batch
        if generic or n > 2048 or (n > 1024 and M > 4):
            return "update_kernel"
        if n <= 1024 and M <= 4:          # GRAM_MM
            return "update_gram_kernel<512,2>"
        return "update_reg_kernel<512,8,2>" if n <= 1024 else "update_reg_kernel<512,4,4>"
    # tiny_applies: the switch, no table utility, not the reproducible mode, <= TINY_N tokens (and <= TINY_MAX_TILES wave-tiles: the
    # networks of step_parity.pool_counts hold at most 448 pools there)
    if env.get("CFMM_TINY", "1") != "0" and not table and not det and n <= 64:
        return "WaveUpdate/solve_tiny_kernel"
    # fused_applies: the switch, no table utility, no ties, <= 2 * EVAL_THREADS tokens, memory <= ITER_MM
    if env.get("CFMM_FUSED", "1") != "0" and not table and not tied and n <= 2048 and M <= 3:
        return "iter_kernel<2,det>" if det else "iter_kernel<2>"       # (ITER_E_SMALL = 2: E = 2 on both sides of 1024 tokens)
    # launch_update
    if table and not generic and n <= 1024 and not tied:
        return "update_reg_kernel<512,8,2,false,true>"
    v = 9 if (generic or table) else int(env.get("CFMM_UPDATE_VARIANT", "0"))
    if v == 0 and n <= 1024 and M <= 4:
        return "update_gram_kernel<512,2>"
    if v in (0, 3) and n <= 1024:
        return "update_reg_kernel<512,8,2>"
    if v in (0, 1, 3) and n <= 2048 and M <= 4:
        return "update_reg_kernel<512,4,4>"
    if v == 2 and n <= 1024:
        return "update_reg_kernel<256,8,4>"
    return "update_kernel"


def _name(n, utility="arbitrage", sigma=0.2, memory=3, ties=False, q=0):
    return sp.Scenario(n, utility=utility, sigma=sigma, memory=memory, ties=ties, start_seed=q).name


FAR_ARB = dict(sigma=2.5)
FAR_LIQ = dict(utility="liquidate", sigma=1.0)
CASES = []


def case(layout, scenario, env=None, det=False):
    assert scenario in sp.SCENARIOS, scenario
    CASES.append(pytest.param(layout, scenario, dict(env or {}), det,
                              id=f"{layout}|{scenario}" + "".join(f"|{k[5:]}={v}" for k, v in (env or {}).items()) + ("|det" if det else "")))


# ---- the one-launch solve (tiny.hpp: WaveUpdate<E> in solve_tiny_kernel): 5 .. 64 tokens, memory 1 .. 8, ties, bounds fixed and free
for _s in (_name(5, memory=8), _name(6, "swap", memory=8), _name(7, "liquidate"), _name(20, memory=1), _name(20, ties=True),
           _name(33, memory=4), _name(33, **FAR_ARB), _name(64), _name(64, memory=8), _name(64, "liquidate", ties=True)):
    case("WaveUpdate/solve_tiny_kernel", _s)
# ... and the same instances through the grid-wide layouts
case("update_reg_kernel<512,8,2>", _name(5, memory=8), NOTINY)
case("update_gram_kernel<512,2>", _name(20, ties=True), NOTINY)
case("update_gram_kernel<512,2>", _name(33, memory=4), NOTINY)
case("iter_kernel<2>", _name(33, **FAR_ARB), NOTINY)
case("iter_kernel<2>", _name(64), NOTINY)
case("update_reg_kernel<512,8,2>", _name(64, memory=8), NOTINY)
case("update_gram_kernel<512,2>", _name(64, "liquidate", ties=True), NOTINY)

# ---- the in-launch update of iter_kernel (iterate.hpp): every wave edge up to 2048 tokens, memory 1 and 3, plain and reproducible
for _n in (65, 127, 128, 129, 1024, 1025, 2048):
    case("iter_kernel<2>", _name(_n, memory=3))
    case("iter_kernel<2>", _name(_n, memory=1))
for _n in (65, 129, 1024, 1025, 2048):
    case("iter_kernel<2,det>", _name(_n, memory=3), det=True)
for _s in (_name(70, **FAR_ARB), _name(70, **FAR_LIQ), _name(70, "swap"), _name(70, "liquidate"), _name(129, **FAR_ARB),
           _name(129, **FAR_LIQ), _name(1025, q=3, **FAR_ARB), _name(1024, **FAR_LIQ)):
    case("iter_kernel<2>", _s)
case("iter_kernel<2,det>", _name(70, **FAR_ARB), det=True)
case("iter_kernel<2,det>", _name(1025, q=3, **FAR_ARB), det=True)

# ---- update_gram_kernel<512,2>: <= 1024 tokens, memory <= 4 (memory 4 is beyond ITER_MM: the two-launch iteration without a switch)
for _n in (65, 127, 128, 129, 1024):
    case("update_gram_kernel<512,2>", _name(_n, memory=3), TWO)
    case("update_gram_kernel<512,2>", _name(_n, memory=1), TWO)
for _n in (65, 129, 1024):
    case("update_gram_kernel<512,2>", _name(_n, memory=4))
for _s in (_name(129, ties=True), _name(70, **FAR_ARB), _name(70, **FAR_LIQ), _name(129, **FAR_ARB), _name(1024, **FAR_LIQ), _name(70, "swap")):
    case("update_gram_kernel<512,2>", _s, TWO)
case("update_gram_kernel<512,2>", _name(129), TWO, det=True)

# ---- update_reg_kernel<512,8,2>: <= 1024 tokens, any memory (memory 8 by itself; memory <= 4 through CFMM_UPDATE_VARIANT=3)
V3 = dict(TWO, CFMM_UPDATE_VARIANT="3")
for _n in (65, 129, 1024):
    case("update_reg_kernel<512,8,2>", _name(_n, memory=8))
for _s in (_name(127), _name(128), _name(129), _name(1024), _name(1024, memory=1), _name(129, ties=True), _name(70, **FAR_ARB), _name(70, **FAR_LIQ)):
    case("update_reg_kernel<512,8,2>", _s, V3)

# ---- update_reg_kernel<512,4,4>: 1025 .. 2048 tokens, memory <= 4
for _n in (1025, 2048):
    for _m in (1, 3, 4):
        case("update_reg_kernel<512,4,4>", _name(_n, memory=_m), TWO)
case("update_reg_kernel<512,4,4>", _name(1025, ties=True))            # (ties keep it off the evaluation launch)
case("update_reg_kernel<512,4,4>", _name(1025, q=3, **FAR_ARB), TWO)

# ---- update_reg_kernel<256,8,4> (CFMM_UPDATE_VARIANT=2): <= 1024 tokens, any memory
V2 = dict(TWO, CFMM_UPDATE_VARIANT="2")
for _s in (_name(65), _name(129), _name(129, memory=8), _name(1024), _name(1024, memory=8), _name(1024, memory=1), _name(129, ties=True),
           _name(70, **FAR_ARB), _name(1024, **FAR_LIQ)):
    case("update_reg_kernel<256,8,4>", _s, V2)

# ---- update_generic_body / update_kernel: beyond 2048 tokens, beyond memory 4 above 1024, or CFMM_UPDATE_GENERIC=1
for _s in (_name(2049), _name(2049, memory=1), _name(2049, memory=8), _name(2049, ties=True), _name(2049, q=7, **FAR_ARB), _name(1025, memory=8)):
    case("update_kernel", _s)
GEN = dict(TWO, CFMM_UPDATE_GENERIC="1")
for _s in (_name(65), _name(129), _name(129, memory=8), _name(1024, memory=4), _name(2048), _name(129, ties=True), _name(70, **FAR_ARB), _name(70, **FAR_LIQ),
           _name(70, "swap")):
    case("update_kernel", _s, GEN)

# ---- the utility table (ULOG / UQUAD / linear mix): its register form, and the generic kernel
case("update_reg_kernel<512,8,2,false,true>", _name(129, "table", memory=8))
case("update_reg_kernel<512,8,2,false,true>", _name(1024, "table", memory=3))
case("update_kernel", _name(1025, "table", memory=8))
case("update_kernel", _name(129, "table", memory=8), {"CFMM_UPDATE_GENERIC": "1"})

WORST = {}        # layout -> (fraction of the tolerance, case id): printed by the last test of the file
HIP_ERROR = []    # a HIP error of an earlier case: nothing more is started on the device behind it


class _device:
    """with _device(): ... -- refuses to start behind an earlier HIP error, and remembers one"""

    def __enter__(self):
        if HIP_ERROR:
            pytest.fail(f"not run: an earlier case ended in a HIP error ({HIP_ERROR[0]})")

    def __exit__(self, typ, e, tb):
        if isinstance(e, cfmm.CfmmError) and e.code == E_HIP:
            HIP_ERROR.append(str(e))
        return False


def _clean_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _problem(sc, det=False):
    b = sp.build(sc)
    p = cfmm.Problem.from_network(b.net, utility=Utility(b.c, b.h, b.ctype), deterministic=det)
    ctx = p._ensure_ctx()
    p._send_utility()
    if b.grp is not None:
        ctx.set_ties(b.grp, b.off)
    return b, p, ctx


def _record(st, nu):
    return dict(evals=st["evals"], iters=st["iters"], status=st["status"], nu=np.asarray(nu, dtype=np.float64).copy(),
                dual_value=st["dual_value"], primal_value=st["primal_value"], gap=st["gap"], infeas=st["infeas"], pg=st["pg"])


def _judge(layout, label, sc, recs):
    fails, worst = sp.compare(sc, recs)
    print(f"step parity: {layout} | {label}: worst {worst[0]:.3g} of the tolerance (budget {worst[1]}, {worst[2]})" +
          (f"; {len(fails)} FAILURES" if fails else ""))
    if worst[0] > WORST.get(layout, (0.0, ""))[0]:
        WORST[layout] = (worst[0], label)
    assert not fails, "\n".join([f"{layout} | {label}"] + fails)


@pytest.mark.parametrize("layout,scenario,env,det", CASES)
def test_layout_follows_the_twin_at_every_budget(oracle_lib, monkeypatch, layout, scenario, env, det):
    sc = sp.SCENARIOS[scenario]
    assert expected_layout(sc, env, det) == layout            # the case table against the selection code
    _clean_env(monkeypatch, env)
    recs = []
    with _device():
        b, p, ctx = _problem(sc, det)
        for k in range(1, sc.K + 1):
            st = ctx.solve(b.nu0, tol=sp.TOL, method="lbfgs", max_evals=k, memory=sc.memory)
            nu, _ = ctx.get_solution()
            recs.append(_record(st, nu))
        p.close()
    _judge(layout, scenario + "".join(f" {k}={v}" for k, v in env.items()) + (" det" if det else ""), sc, recs)


def _starts70(memory, size):
    return [_name(70, memory=memory, q=q) for q in range(size)]


# (layout, the scenarios of one call -- one network, one utility, one memory --, switches)
BATCH_CASES = [("update_gram_kernel<512,2>", _starts70(3, 1), {}), ("update_gram_kernel<512,2>", _starts70(3, 8), {}),
               ("update_reg_kernel<512,8,2>", _starts70(8, 8), {}), ("update_kernel", _starts70(3, 8), {"CFMM_UPDATE_GENERIC": "1"}),
               ("update_gram_kernel<512,2>", [_name(70, **FAR_ARB), _name(70)], {}),
               ("update_kernel", [_name(70), _name(70, **FAR_ARB)], {"CFMM_UPDATE_GENERIC": "1"})]


@pytest.mark.parametrize("layout,scenarios,env", BATCH_CASES, ids=["gram-1", "gram-8", "reg-8", "generic-8", "gram-far", "generic-far"])
def test_batched_solve_follows_the_twin_at_every_budget(oracle_lib, monkeypatch, layout, scenarios, env):
    """cfmm_solve_batch's own step -- update_gram_kernel<512,2,true>, update_reg_kernel<512,8,2,true>, update_kernel<true>, one workgroup
    per solve -- with up to eight different starts in one call, each against its own twin run; a far start (rejections, the step cap) in
    lock-step with a tame one"""
    scs = [sp.SCENARIOS[s] for s in scenarios]
    size, memory = len(scs), scs[0].memory
    assert all(sc.n == scs[0].n and sc.memory == memory and sc.utility == "arbitrage" and not sc.ties for sc in scs)
    assert expected_layout(scs[0], env, batch=True) == layout
    _clean_env(monkeypatch, env)
    starts = [sp.build(sc).nu0 for sc in scs]
    recs = [[] for _ in scs]
    with _device():
        b0, p, ctx = _problem(scs[0])
        assert ctx.batch_capacity() >= size
        clones = [ctx.clone() for _ in scs[1:]]
        for c in clones:
            c.set_utility(b0.c, b0.h, b0.ctype)
        for k in range(1, scs[0].K + 1):
            sts = ctx.solve_batch(clones, starts, tol=sp.TOL, max_evals=k, memory=memory)
            for q, c in enumerate([ctx] + clones):
                recs[q].append(_record(sts[q], c.get_solution()[0]))
        for c in clones:
            c.close()
        p.close()
    for q, sc in enumerate(scs):
        _judge(layout + " (batched)", f"{sc.name}, {q + 1} of {size}", sc, recs[q])


@pytest.mark.parametrize("scenarios", [[sc.name for sc in sp.SWEEP_STARTS], [_name(33, **FAR_ARB), _name(33)]], ids=["tame-4", "far"])
def test_swept_solve_follows_the_twin_at_every_budget(oracle_lib, monkeypatch, scenarios):
    """cfmm_solve_sweep: solve_tiny_kernel<true>, one workgroup per point (WaveUpdate<E>); the starts of one call (four tame ones; a far one
    beside a tame one).  Without constant-sum pools a point is one leg of the caller's budget when the kink search starts at its widest
    (kink_tol 0.05: sweep_rules.hpp: round_tail)"""
    _clean_env(monkeypatch, {})
    scs = [sp.SCENARIOS[s] for s in scenarios]
    assert all(sc.n == scs[0].n and sc.memory == scs[0].memory and sc.utility == "arbitrage" and not sc.ties for sc in scs)
    B = len(scs)
    nu0 = np.stack([sp.build(sc).nu0 for sc in scs])
    recs = [[] for _ in scs]
    with _device():
        b0, p, ctx = _problem(scs[0])
        c = np.tile(b0.c, (B, 1)); h = np.tile(b0.h, (B, 1)); ct = np.tile(b0.ctype, (B, 1))
        for k in range(1, scs[0].K + 1):
            nu, psi, theta, tsgn, trades, sts, rounds = ctx.solve_sweep(c, h, ct, nu0, kink_tol=0.05, max_rounds=1, tol=sp.TOL, max_evals=k,
                                                                          memory=scs[0].memory, method="lbfgs")
            assert list(rounds) == [1] * B
            for q in range(B):
                recs[q].append(_record(sts[q], nu[q]))
        p.close()
    for q, sc in enumerate(scs):
        _judge("WaveUpdate/solve_tiny_kernel (swept)", sc.name, sc, recs[q])


def test_the_case_table_names_every_layout():
    """every layout of docs/step_parity.md is a case, at every token count at which its lanes or its selection change; prints, per
    layout, the largest device-to-twin deviation the cases of this session saw, as a fraction of its tolerance"""
    for layout, (frac, label) in sorted(WORST.items()):
        print(f"step parity summary: {layout}: {frac:.3g} of the tolerance ({label})")
    at = {}
    for c in CASES:
        at.setdefault(c.values[0], set()).add(sp.SCENARIOS[c.values[1]].n)
    for b in BATCH_CASES:
        at.setdefault(b[0] + " (batched)", set()).add(sp.SCENARIOS[b[1][0]].n)
    want = {"WaveUpdate/solve_tiny_kernel": {5, 20, 33, 64}, "iter_kernel<2>": {65, 127, 128, 129, 1024, 1025, 2048},
            "iter_kernel<2,det>": {65, 129, 1024, 1025, 2048}, "update_gram_kernel<512,2>": {65, 127, 128, 129, 1024},
            "update_reg_kernel<512,8,2>": {65, 127, 128, 129, 1024}, "update_reg_kernel<512,4,4>": {1025, 2048},
            "update_reg_kernel<256,8,4>": {65, 129, 1024}, "update_reg_kernel<512,8,2,false,true>": {129, 1024},
            "update_kernel": {65, 129, 1025, 2048, 2049}, "update_gram_kernel<512,2> (batched)": {70},
            "update_reg_kernel<512,8,2> (batched)": {70}, "update_kernel (batched)": {70}}
    for layout, ns in want.items():
        assert ns <= at.get(layout, set()), (layout, sorted(ns - at.get(layout, set())))
