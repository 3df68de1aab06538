"""CPU tests of the host half of the in-place update of fees and weights (include/cfmm.h: cfmm_update_terms2 / N / G):
cfmm.problem.route_terms maps pool-list indices to (bucket, position) with pack()'s normalisation and refuses what the library would
refuse; Problem.update_bucket_terms keeps the host network in step before any device exists; cfmm.problem.shard_terms cuts an update
the way shard_network cuts the pools; csrc/update_rules.hpp (the predicates the uploads and the updates share, the smallest fee after
a scatter, when the compact mirror is reset) through a stand-alone host program."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import cfmm
from cfmm.problem import route_terms, shard_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one pool of every kind: cp2, w2, sum2, curve2, pow2, geo-mean k = 3 and 4, table stableswap k = 3, table constant sum k = 4, cp2, w2
IDX = [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [0, 1, 2], [1, 2, 3, 4], [2, 3, 4], [0, 2, 4, 5], [1, 5], [0, 5]]
RES = [[10, 20], [30, 40], [5, 6], [7, 8], [9, 11], [1, 2, 3], [4, 5, 6, 7], [8, 9, 10], [11, 12, 13, 14], [3, 4], [6, 7]]
KINDS = ["geomean", "geomean", "sum", "curve", "powersum", "geomean", "geomean", "curve", "sum", "geomean", "geomean"]
WEIGHTS = [None, [0.3, 0.7], None, None, None, None, [1, 2, 3, 4], None, None, None, [0.8, 0.2]]
PARAMS = [None, None, None, 50.0, 0.4, None, None, 20.0, None, None, None]
FEES = [0.997, 0.99, 0.999, 0.9996, 0.995, 0.997, 0.998, 0.9994, 0.9999, 0.9970, 0.98]


def mixed():
    return cfmm.pack(6, IDX, RES, FEES, KINDS, WEIGHTS, PARAMS)


# ---------------------------------------------------------------------------------------------------------- the routing helper
def test_route_terms_maps_every_kind_to_its_bucket_and_position():
    net, where = mixed()
    assert where[0] == ("cp2", 0) and where[9] == ("cp2", 1) and where[1] == ("w2", 0) and where[10] == ("w2", 1)
    pools = [9, 0, 10, 1, 2, 3, 4, 5, 6, 7, 8]
    fees = [0.90 + 0.005 * i for i in range(len(pools))]
    out = route_terms(net, where, pools, fees=fees)
    assert set(out) == {"cp2", "w2", "sum2", "curve2", "pow2", 3, 4, ("stable", 3), ("sum", 4)}
    pos, fee, w = out["cp2"]
    assert pos.dtype == np.int32 and pos.tolist() == [0, 1] and fee.tolist() == [fees[1], fees[0]] and w is None    # ascending positions
    pos, fee, w = out["w2"]
    assert pos.tolist() == [0, 1] and fee.tolist() == [fees[3], fees[2]] and w is None
    for key, i in (("sum2", 2), ("curve2", 3), ("pow2", 4), (3, 5), (4, 6), (("stable", 3), 7), (("sum", 4), 8)):
        pos, fee, w = out[key]
        assert pos.tolist() == [0] and fee.tolist() == [fees[pools.index(i)]] and w is None, key
    assert route_terms(net, where, [], fees=[]) == {}
    assert route_terms(net, where, [3, 4], fees=[None, None]) == {}           # nothing to change: no bucket is named


def test_route_terms_normalises_weights_as_pack_does():
    net, where = mixed()
    new = {1: [2.0, 6.0], 10: [5.0, 5.0], 5: [1.0, 2.0, 7.0], 6: [0.1, 0.2, 0.3, 0.9]}
    out = route_terms(net, where, list(new), weights=list(new.values()))
    assert set(out) == {"w2", 3, 4}
    pos, fee, wa = out["w2"]
    assert fee is None and pos.tolist() == [0, 1]
    assert wa.tolist() == [(np.array(new[1]) / np.array(new[1]).sum())[0], 0.5]     # (a w2 pool may take equal weights: it stays in w2)
    for k, i in ((3, 5), (4, 6)):
        pos, fee, w = out[k]
        assert fee is None and pos.tolist() == [0] and w.shape == (k, 1)                # slot-major [k][count]
        assert np.array_equal(w[:, 0], np.array(new[i]) / np.array(new[i]).sum())
    # the packed network of the changed lists holds exactly these columns (pool 10 left out: pack() would file its equal weights under cp2)
    W2 = list(WEIGHTS)
    for i, w in new.items():
        if i != 10:
            W2[i] = w
    net2, _ = cfmm.pack(6, IDX, RES, FEES, KINDS, W2, PARAMS)
    assert net2["w2"]["wa"][0] == out["w2"][2][0] and np.array_equal(net2["gn"][3]["w"], out[3][2]) and np.array_equal(net2["gn"][4]["w"], out[4][2])


def test_route_terms_keeps_the_current_column_of_entries_without_a_value():
    net, where = mixed()
    out = route_terms(net, where, [1, 10], fees=[0.9, None], weights=[None, [1.0, 3.0]])
    pos, fee, wa = out["w2"]
    assert pos.tolist() == [0, 1] and fee.tolist() == [0.9, 0.98] and wa.tolist() == [0.3 / (0.3 + 0.7), 0.25]


def test_route_terms_refusals_carry_messages():
    net, where = mixed()
    with pytest.raises(ValueError, match="2 pools but 1 fees"):
        route_terms(net, where, [0, 1], fees=[0.9])
    with pytest.raises(ValueError, match="1 pools but 2 weight vectors"):
        route_terms(net, where, [1], weights=[[1, 2], [1, 2]])
    for bad in (0.0, 1.5, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"fee must be in \(0, 1\]"):
            route_terms(net, where, [0, 2], fees=[0.99, bad])
    for bad in ([0.0, 1.0], [-1.0, 2.0], [float("nan"), 1.0], [1.0, 2.0, 3.0], [float("inf"), 1.0]):
        with pytest.raises(ValueError, match="bad weights"):
            route_terms(net, where, [1], weights=[bad])
    with pytest.raises(ValueError, match="bad weights"):
        route_terms(net, where, [1], weights=[[1.0, 1e-300]])                 # normalises to a weight of exactly 1
    with pytest.raises(ValueError, match="unequal weights is a re-upload"):
        route_terms(net, where, [0], weights=[[0.3, 0.7]])                    # a pool pack() put into cp2
    for i in (2, 3, 4, 7, 8):
        with pytest.raises(ValueError, match="no weights to update"):
            route_terms(net, where, [i], weights=[[1.0] * len(IDX[i])])
    with pytest.raises(ValueError, match="twice"):
        route_terms(net, where, [0, 0], fees=[0.9, 0.9])
    with pytest.raises(ValueError, match="outside"):
        route_terms(net, where, [len(IDX)], fees=[0.9])
    with pytest.raises(ValueError, match="outside"):
        route_terms(net, where, [-1], fees=[0.9])


# ---------------------------------------------------------------------------------------------------------- before upload
def problem():
    return cfmm.Problem(6, IDX, RES, FEES, KINDS, WEIGHTS, PARAMS, utility=cfmm.Arbitrage(np.ones(6)))


def test_update_bucket_terms_before_upload_changes_only_the_host_network():
    p = problem()
    q = cfmm.Problem(6, network=p.net, utility=p.utility)          # shares the network, as a clone does
    q.where = p.where
    g0 = p.net.get("_generation", 0)
    R0 = {k: p.net[k]["Ra"].copy() for k in ("cp2", "w2", "sum2")}
    p.update_fees([2, 7, 0], [0.9, 0.95, 0.5])
    assert p.ctx is None and q.ctx is None                         # no device was touched
    assert p.net["_generation"] == g0 + 3                          # one bucket call each
    assert q.net["sum2"]["fee"].tolist() == [0.9] and q.net["gk"][("stable", 3)]["fee"].tolist() == [0.95] and q.net["cp2"]["fee"].tolist() == [0.5, 0.997]
    p.update_weights([1, 6], [[1.0, 1.0], [4, 3, 2, 1]])
    assert q.net["w2"]["wa"].tolist() == [0.5, 0.8] and np.array_equal(q.net["gn"][4]["w"][:, 0], np.array([4, 3, 2, 1]) / 10.0)
    assert q.net["gn"][4]["fee"].tolist() == [0.998]
    for k, R in R0.items():
        assert np.array_equal(p.net[k]["Ra"], R)
    p.update_bucket_terms(3, [0], fee=[0.9], w=[[0.2], [0.3], [0.5]])
    assert p.net["gn"][3]["fee"].tolist() == [0.9] and p.net["gn"][3]["w"][:, 0].tolist() == [0.2, 0.3, 0.5]
    p.update_bucket_terms("cp2", [], fee=[])                        # an empty part (a rank whose slice is untouched) is legal
    # the Problem that shares the network drops what it derived from the old terms
    q._theta = {"x": 1}; q._trade_cache = object()
    p.update_fees([0], [0.9])
    q._pools_seen()
    assert q._theta == {} and q._trade_cache is None


def test_update_bucket_terms_refusals():
    p = problem()
    net0 = {k: p.net[k]["fee"].copy() for k in ("cp2", "w2")}
    cases = [
        ("outside", lambda: p.update_bucket_terms("cp2", [2], fee=[0.9])),
        ("outside", lambda: p.update_bucket_terms("cp2", [-1], fee=[0.9])),
        ("twice", lambda: p.update_bucket_terms("cp2", [0, 0], fee=[0.9, 0.9])),
        ("neither fees nor weights", lambda: p.update_bucket_terms("cp2", [0])),
        ("2 positions but 1 fees", lambda: p.update_bucket_terms("cp2", [0, 1], fee=[0.9])),
        ("fee must be in", lambda: p.update_bucket_terms("cp2", [0, 1], fee=[0.9, 0.0])),
        ("fee must be in", lambda: p.update_bucket_terms("cp2", [0], fee=[float("nan")])),
        ("fee must be in", lambda: p.update_bucket_terms("cp2", [0], fee=[1.5])),
        ("re-upload", lambda: p.update_bucket_terms("cp2", [0], w=[0.3])),
        ("no weights", lambda: p.update_bucket_terms("curve2", [0], w=[0.3])),
        ("no weights", lambda: p.update_bucket_terms(("stable", 3), [0], w=np.full((3, 1), 1 / 3))),
        ("weights of shape", lambda: p.update_bucket_terms("w2", [0], w=[[0.3], [0.7]])),
        ("weights of shape", lambda: p.update_bucket_terms(3, [0], w=[0.2, 0.3, 0.5])),
        (r"weights must be in \(0, 1\)", lambda: p.update_bucket_terms("w2", [0], w=[1.0])),
        (r"weights must be in \(0, 1\)", lambda: p.update_bucket_terms("w2", [0, 1], w=[0.5, 0.0])),
        (r"weights must be in \(0, 1\)", lambda: p.update_bucket_terms(3, [0], w=[[0.5], [float("nan")], [0.5]])),
        ("no bucket", lambda: p.update_bucket_terms(5, [0], fee=[0.9])),
    ]
    for msg, call in cases:
        with pytest.raises(ValueError, match=msg):
            call()
    for k, f in net0.items():
        assert np.array_equal(p.net[k]["fee"], f)
    q = cfmm.Problem.from_network(p.net)
    with pytest.raises(cfmm.CfmmError, match="update_bucket_terms"):
        q.update_fees([0], [0.9])                                   # no pool list
    with pytest.raises(cfmm.CfmmError, match="update_bucket_terms"):
        q.update_weights([1], [[1, 2]])


def test_a_context_without_the_new_calls_says_so():
    from oracle_ctx import OracleContext
    p = problem()
    p.ctx = OracleContext(6); p._uploaded = True
    assert not hasattr(p.ctx, "update_terms2")
    fee0 = p.net["cp2"]["fee"].copy()
    with pytest.raises(cfmm.CfmmError, match="no in-place update of fees and weights"):
        p.update_fees([0], [0.9])
    with pytest.raises(cfmm.CfmmError, match="no in-place update of fees and weights"):
        p.update_bucket_terms(3, [0], fee=[0.9])
    assert np.array_equal(p.net["cp2"]["fee"], fee0)                 # refused before the host network moved


# ---------------------------------------------------------------------------------------------------------- sharding
def test_shard_terms_picks_each_ranks_slice_in_local_positions():
    m, world = 10, 3                                                       # slices [0, 3), [3, 6), [6, 10) as shard_network cuts them
    pos = np.array([9, 0, 4, 3, 6])
    fee = 0.9 + pos / 100.0
    w = np.vstack([pos + 100.0, pos + 200.0, pos + 300.0])
    parts = [shard_terms(m, r, world, pos, fee, w) for r in range(world)]
    assert [p[0].tolist() for p in parts] == [[0], [1, 0], [3, 0]]
    assert parts[1][1].tolist() == [fee[2], fee[3]] and parts[2][1].tolist() == [fee[0], fee[4]]
    assert parts[1][2][:, 0].tolist() == [104.0, 204.0, 304.0] and parts[2][2].shape == (3, 2)
    wa = shard_terms(m, 2, world, pos, None, pos * 1.0)                    # the two-asset weighted bucket's one column
    assert wa[1] is None and wa[2].tolist() == [9.0, 6.0]
    empty = shard_terms(m, 0, world, [7], [0.9])
    assert len(empty[0]) == 0 and len(empty[1]) == 0 and empty[2] is None
    # the cut is shard_network's: an update of the whole network through the parts is the shards of the updated network
    from cfmm import synthetic
    net = synthetic.config("C3", scale=0.001)
    mk = len(net["cp2"]["fee"])
    gpos = np.arange(0, mk, 3)
    newfee = np.linspace(0.5, 0.9, len(gpos))
    upd = synthetic.copy_network(net)
    upd["cp2"]["fee"][gpos] = newfee
    for r in range(world):
        sh = cfmm.shard_network(net, r, world)
        lp, lf, _ = shard_terms(mk, r, world, gpos, newfee)
        f = sh["cp2"]["fee"].copy(); f[lp] = lf
        assert np.array_equal(f, cfmm.shard_network(upd, r, world)["cp2"]["fee"])


# ---------------------------------------------------------------------------------------------------------- csrc/update_rules.hpp
def _rules_program(tmp_path, name, body, sanitize=False):
    """a stand-alone HOST program over csrc/update_rules.hpp (nothing of HIP in it): compiled -Wall -Werror, run, its output lines"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc missing")
    src = tmp_path / f"{name}.cpp"
    src.write_text('#include "update_rules.hpp"\n#include <cstdio>\n#include <cmath>\n#include <limits>\n#include <initializer_list>\nusing namespace terms;\n'
                   "int main()\n{\n" + body + "\n    return 0;\n}\n")
    exe = tmp_path / name
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []      # (host code only: the program has no device code)
    r = subprocess.run([hipcc, "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "cfmm-routing-code_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r.stdout.strip().splitlines()


_EDGES = [("zero", "0.0"), ("negzero", "-0.0"), ("denormal", "4.9406564584124654e-324"), ("tiny", "2.2250738585072014e-308"), ("half", "0.5"),
          ("below1", "std::nextafter(1.0, 0.0)"), ("one", "1.0"), ("above1", "std::nextafter(1.0, 2.0)"), ("neg", "-0.5"),
          ("nan", "std::numeric_limits<double>::quiet_NaN()"), ("inf", "std::numeric_limits<double>::infinity()"),
          ("neginf", "-std::numeric_limits<double>::infinity()")]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_update_rules_predicates_at_their_edges(tmp_path, sanitize):
    """a fee is in (0, 1], a weight in (0, 1): the smallest denormal is in, 0 and -0 are out, 1 is a fee and no weight, the next double
    above 1, NaN and the infinities are neither.  first_bad names the first offender and reports the smallest entry in front of it."""
    body = "".join(f'    printf("{nm} %d %d\\n", (int)fee_ok({x}), (int)weight_ok({x}));\n' for nm, x in _EDGES)
    body += r'''
    const double good[] = {0.997, 0.4, 1.0, 0.9}, bad[] = {0.997, 0.3, std::nan(""), 0.1};
    double mn = 1.0;
    printf("first_good %lld %.17g\n", (long long)first_bad(good, 4, fee_ok, &mn), mn);
    mn = 1.0;
    printf("first_nan %lld %.17g\n", (long long)first_bad(bad, 4, fee_ok, &mn), mn);
    printf("first_weight %lld\n", (long long)first_bad(good, 4, weight_ok));
    printf("first_empty %lld\n", (long long)first_bad(good, 0, weight_ok));
'''
    got = {l.split()[0]: l.split()[1:] for l in _rules_program(tmp_path, "pred", body, sanitize)}
    want_fee = dict(zero=0, negzero=0, denormal=1, tiny=1, half=1, below1=1, one=1, above1=0, neg=0, nan=0, inf=0, neginf=0)
    want_w = dict(want_fee, one=0)
    for nm, _ in _EDGES:
        assert [int(x) for x in got[nm]] == [want_fee[nm], want_w[nm]], nm
    assert (int(got["first_good"][0]), float(got["first_good"][1])) == (-1, 0.4) and (int(got["first_nan"][0]), float(got["first_nan"][1])) == (2, 0.3)
    assert got["first_weight"] == ["2"] and got["first_empty"] == ["-1"]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_update_rules_smallest_fee_after_a_scatter(tmp_path, sanitize):
    """min_fee_after against the minimum of the column itself, on hand-made buckets: the scatter's flag is formed as the kernel forms it
    (a fee EQUAL to the recorded minimum overwritten with a larger one), the reduction is the column's minimum through the complemented
    bit pattern the device leaves.  Cases: the minimum raised (alone, and with a twin left behind), lowered, untouched, rewritten with
    itself, every pool updated, nothing updated; and mirror_reset over its three facts."""
    cases = [
        ("raised", [0.5, 0.9, 0.7], [0], [0.8]),
        ("raised_twin", [0.5, 0.9, 0.5], [0], [0.8]),
        ("raised_below_new", [0.5, 0.9, 0.7], [0, 1], [0.95, 0.6]),
        ("lowered", [0.5, 0.9, 0.7], [1], [0.4]),
        ("min_lowered", [0.5, 0.9, 0.7], [0], [0.25]),
        ("untouched", [0.5, 0.9, 0.7], [2], [0.99]),
        ("same", [0.5, 0.9, 0.7], [0], [0.5]),
        ("all", [0.5, 0.9, 0.7], [0, 1, 2], [0.8, 1.0, 0.9]),
        ("all_down", [0.5, 0.9, 0.7], [2, 1, 0], [0.1, 0.2, 0.3]),
        ("none", [0.5, 0.9, 0.7], [], []),
        ("ones", [1.0, 1.0], [1], [1.0]),
    ]
    body = r'''
    auto run = [](const char *name, std::initializer_list<double> col0, std::initializer_list<int> pos, std::initializer_list<double> fee) {
        double col[8]; int n = 0;
        for (double x : col0) col[n++] = x;
        double mn_old = 1.0;
        for (int i = 0; i < n; ++i) mn_old = col[i] < mn_old ? col[i] : mn_old;
        bool raised = false;
        double mn_new = 1.0;
        auto f = fee.begin();
        for (int p : pos) { const double v = *f++; if (col[p] == mn_old && v > col[p]) raised = true; col[p] = v; mn_new = v < mn_new ? v : mn_new; }
        unsigned long long word = 0ull;                       // what upd_min_kernel leaves: the largest complement
        for (int i = 0; i < n; ++i) { unsigned long long b; std::memcpy(&b, &col[i], 8); b = ~b; word = b > word ? b : word; }
        double truth = 1.0;
        for (int i = 0; i < n; ++i) truth = col[i] < truth ? col[i] : truth;
        printf("%s %d %.17g %.17g\n", name, (int)raised, min_fee_after(mn_old, raised, mn_new, raised ? fee_from_reduced(word) : 1.0), truth);
    };
'''
    for nm, col, pos, fee in cases:
        body += '    run("%s", {%s}, {%s}, {%s});\n' % (nm, ", ".join(map(repr, col)), ", ".join(map(str, pos)), ", ".join(map(repr, fee)))
    body += '    for (int t = 0; t < 2; ++t) for (int f = 0; f < 2; ++f) for (int c = 0; c < 2; ++c) printf("reset_%d%d%d %d\\n", t, f, c, (int)mirror_reset(t, f, c));\n'
    body += '    const double x = 0.3; unsigned long long b; std::memcpy(&b, &x, 8); printf("roundtrip %.17g\\n", fee_from_reduced(~b));\n'
    got = {l.split()[0]: l.split()[1:] for l in _rules_program(tmp_path, "minfee", body, sanitize)}
    want_raised = dict(raised=1, raised_twin=1, raised_below_new=1, lowered=0, min_lowered=0, untouched=0, same=0, all=1, all_down=0, none=0, ones=0)
    want_min = dict(raised=0.7, raised_twin=0.5, raised_below_new=0.6, lowered=0.4, min_lowered=0.25, untouched=0.5, same=0.5, all=0.8, all_down=0.1,
                    none=0.5, ones=1.0)
    for nm, *_ in cases:
        raised, mn, truth = int(got[nm][0]), float(got[nm][1]), float(got[nm][2])
        assert raised == want_raised[nm] and mn == truth == want_min[nm], (nm, got[nm])
    for t in (0, 1):
        for f in (0, 1):
            for c in (0, 1):
                assert int(got[f"reset_{t}{f}{c}"][0]) == int(t and f and c)      # tried, fees written, at least one pool
    assert float(got["roundtrip"][0]) == 0.3 and math.isfinite(float(got["roundtrip"][0]))
