"""CPU suite: the host side of auditing a route (docs/audit.md) -- the layouts of cfmm_audit / cfmm_audit_tenders as bound by
cfmm/_lib.py, and the NumPy twin cfmm.problem.audit_trades on the seven shipped instances at the fixture's KKT point and on doctored
routes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cfmm
from cfmm import _lib
from cfmm.problem import audit_trades, audit_buckets, audit_exponent
from helpers import golden, shipped_cases, problem_of, utility_of, exact_floor, limbs_as_integers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = shipped_cases()


def test_audit_structs_match_the_header_layout_and_the_names_exist(tmp_path):
    """cfmm_audit and cfmm_audit_tenders as bound by cfmm/_lib.py have the size and the field offsets the C compiler gives the header's
    structs; the symbol is listed and the Python entry points exist"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cfmm.h"', 'int main(void) {']
    want = []
    for cname, cls in (("cfmm_audit", _lib.Audit), ("cfmm_audit_tenders", _lib.AuditTenders)):
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(ctypes.sizeof(cls))
        for f, _ in cls._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
            want.append(getattr(cls, f).offset)
    lines += ['printf("%d\\n", CFMM_MAX_POOL_SIZE);', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[:-1] == want
    assert out[-1] == _lib.MAX_POOL_SIZE and len(_lib.AuditTenders().sumk_delta) == _lib.MAX_POOL_SIZE + 1
    assert "cfmm_audit_trades" in _lib.SYMBOLS
    assert callable(_lib.Context.audit) and callable(cfmm.Problem.audit)
    rep = _lib.Audit(pools=5, pools_trading=4, pools_violating=1, legs_out_of_range=2, worst_family=2, worst_kind=1, worst_k=3,
                     fixed_exponent=71, worst_pos=9, min_slack=-0.5, min_tender=0.0, min_leg=0.25, value=1.5, infeas=0.0)
    assert rep.asdict() == dict(pools=5, pools_trading=4, pools_violating=1, legs_out_of_range=2, worst_family=2, worst_kind=1, worst_k=3,
                                fixed_exponent=71, worst_pos=9, min_slack=-0.5, min_tender=0.0, min_leg=0.25, value=1.5, infeas=0.0)


def kkt_route(name, inst):
    """the packed network of a shipped instance and the fixture's KKT point as a route: Delta = max(-y, 0), Lambda = max(y, 0)"""
    p = problem_of(inst)
    k = golden()[name]["kkt"]
    tr = {b["key"]: (np.zeros_like(b["R"]), np.zeros_like(b["R"])) for b in audit_buckets(p.net)}
    for (key, pos), y in zip(p.where, k["y"]):
        y = np.asarray(y, dtype=np.float64)
        tr[key][0][:, pos] = np.maximum(-y, 0.0); tr[key][1][:, pos] = np.maximum(y, 0.0)
    return p, k, tr


@pytest.mark.parametrize("name,inst", CASES, ids=[c[0] for c in CASES])
def test_twin_accepts_the_kkt_point_of_every_shipped_instance(name, inst):
    p, k, tr = kkt_route(name, inst)
    rep = audit_trades(p.net, tr, utility_of(inst))
    print(name, "min_slack", rep["min_slack"], "min_leg", rep["min_leg"], "psi err", np.abs(rep["psi"] - np.asarray(k["psi"])).max())
    assert rep["pools"] == len(inst["local_indices"])
    assert rep["min_slack"] >= -1e-14
    assert rep["pools_violating"] == 0 and rep["legs_out_of_range"] == 0 and rep["min_tender"] == 0.0
    if name in ("two_asset_0", "two_asset_1", "two_asset_25", "two_asset_49"):
        assert rep["min_leg"] == 0.0                         # a fully drained constant-sum leg: feasible (arbitrage.py:73-74)
    psi = rep["psi"]
    assert np.abs(psi - np.asarray(k["psi"])).max() <= 1e-12 * max(1.0, float(np.abs(psi).max()))
    # the integer psi against exact floors formed independently, contribution by contribution
    F = rep["fixed_exponent"]
    assert F == audit_exponent(p.net)
    want = [0] * p.n
    for b in audit_buckets(p.net):
        d, l = tr[b["key"]]
        for y, sign in ((l, 1.0), (d, -1.0)):
            sel = y != 0.0
            for tok, v in zip(b["idx"][sel].tolist(), exact_floor(sign * y[sel], F)):
                want[tok] += v
    assert rep["psi_int"] == want
    assert limbs_as_integers(rep["limbs"]) == want
    assert np.array_equal(psi, np.array([float(v) for v in want]) * 2.0 ** -F)
    assert abs(rep["value"] - k["value"]) <= 1e-9 * max(1.0, abs(k["value"]))


def test_twin_catches_doctored_routes():
    """one pool's Lambda times 1 + 1e-6: exactly that pool is the worst and the only violator; a constant-sum pool filled 1.5 times its
    full fill violates through its leg; an entry of 1e300 is counted and stays out of the limbs"""
    p, k, tr = kkt_route("arbitrage", dict(CASES)["arbitrage"])
    base = audit_trades(p.net, tr, None)
    assert base["pools_violating"] == 0 and np.isnan(base["value"]) and np.isnan(base["infeas"])
    buckets = {b["key"]: b for b in audit_buckets(p.net)}
    for key, b in buckets.items():
        for pos in range(b["R"].shape[1]):
            if not tr[key][1][:, pos].any():
                continue
            doc = {q: (d.copy(), l.copy()) for q, (d, l) in tr.items()}
            doc[key][1][:, pos] *= 1.0 + 1e-6
            rep = audit_trades(p.net, doc, None)
            assert rep["pools_violating"] == 1, (key, pos, rep["min_slack"])
            assert (rep["worst_family"], rep["worst_kind"], rep["worst_k"], rep["worst_pos"]) == (b["family"], b["kind"], b["k"], pos)
            assert rep["min_slack"] < -1e-9
    # the constant-sum pool (pool 4 of arbitrage.py: filled 38.6 % at the optimum) filled 1.5 times its FULL fill
    b = buckets["sum2"]
    y = np.asarray(k["y"][4])
    out = int(np.argmax(y))                                  # the leg the pool pays out
    full = b["R"][out, 0]
    doc = {q: (d.copy(), l.copy()) for q, (d, l) in tr.items()}
    doc["sum2"][1][out, 0] = 1.5 * full
    doc["sum2"][0][1 - out, 0] = 1.5 * full / b["fee"][0]
    rep = audit_trades(p.net, doc, None)
    assert rep["pools_violating"] == 1 and rep["min_leg"] < 0.0 and rep["min_slack"] >= -1e-14
    assert (rep["worst_family"], rep["worst_kind"], rep["worst_k"]) != (-1, -1, -1)
    # exactly the full fill: the leg is drained to zero, which a constant-sum pool accepts
    doc["sum2"][1][out, 0] = full
    doc["sum2"][0][1 - out, 0] = full / b["fee"][0]
    rep = audit_trades(p.net, doc, None)
    assert rep["pools_violating"] == 0 and rep["min_leg"] == 0.0
    # a negative tender
    doc = {q: (d.copy(), l.copy()) for q, (d, l) in tr.items()}
    doc["cp2"][0][0, 0] = -1e-3
    rep = audit_trades(p.net, doc, None)
    assert rep["pools_violating"] >= 1 and rep["min_tender"] == -1e-3
    # 1e300: outside the fixed point -- counted, and absent from the limbs
    doc = {q: (d.copy(), l.copy()) for q, (d, l) in tr.items()}
    key = "cp2"
    tok = int(buckets[key]["idx"][0, 0])
    zero = {q: (d.copy(), l.copy()) for q, (d, l) in tr.items()}
    zero[key][1][0, 0] = 0.0
    doc[key][1][0, 0] = 1e300
    rep, ref = audit_trades(p.net, doc, None), audit_trades(p.net, zero, None)
    assert rep["legs_out_of_range"] == 1 and ref["legs_out_of_range"] == 0
    assert np.array_equal(rep["limbs"], ref["limbs"]) and rep["psi_int"][tok] == ref["psi_int"][tok]
    assert rep["pools_violating"] >= 1
