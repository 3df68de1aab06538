"""CPU suite, part 2: host logic of the product (packing, start prices, kink ties + fill recovery,
sharding) with the C oracle standing in for the device (tests/oracle_ctx.py), and the C-ABI
library itself: it must load and export every symbol include/cfmm.h declares, and must refuse to
run without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import cfmm
from cfmm import _lib, synthetic
from oracle import instances as I
from oracle.primal_scipy import solve_primal
from helpers import golden, shipped_cases, problem_of, random_instance, normalise_with_params
from oracle_ctx import OracleContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cabi_library_exports_header_symbols():
    """two-sided: every entry point include/cfmm.h declares is exported, and the library exports no cfmm_* symbol
    the header does not declare (tuning-build-only entry points sit behind #ifdef in both places)"""
    import subprocess
    _lib.build()
    L = ctypes.CDLL(_lib._SO)
    header = open(os.path.join(ROOT, "include", "cfmm.h")).read()
    header = re.sub(r"#ifdef CFMM_SMOOTH_HIST.*?#endif", "", header, flags=re.S)       # (not part of the shipped build)
    names = set(re.findall(r"\b(cfmm_[a-z_0-9A-Z]+)\s*\(", header))
    assert len(names) >= 20
    for nm in names:
        assert hasattr(L, nm), f"libcfmm_hip.so lacks {nm}"
    assert names == set(_lib.SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib._SO]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("cfmm_")}
    assert exported == names, f"undeclared exports: {sorted(exported - names)}; missing: {sorted(names - exported)}"


def test_ctypes_structs_match_the_header_layout(tmp_path):
    """cfmm_opts / cfmm_stats as bound by cfmm/_lib.py AND by the verbatim stub in INTEGRATION.md have the size and
    field offsets the C compiler gives the header's structs (a mismatch corrupts memory silently)"""
    import subprocess
    src = tmp_path / "layout.c"
    fields_o = [f for f, _ in _lib.Opts._fields_]
    fields_s = [f for f, _ in _lib.Stats._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cfmm.h"', 'int main(void) {',
             'printf("%zu %zu\\n", sizeof(cfmm_opts), sizeof(cfmm_stats));']
    lines += [f'printf("%zu\\n", offsetof(cfmm_opts, {f}));' for f in fields_o]
    lines += [f'printf("%zu\\n", offsetof(cfmm_stats, {f}));' for f in fields_s]
    lines += ['return 0; }']
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert int(out[0]) == ctypes.sizeof(_lib.Opts) and int(out[1]) == ctypes.sizeof(_lib.Stats)
    offs = [int(x) for x in out[2:]]
    assert offs[:len(fields_o)] == [getattr(_lib.Opts, f).offset for f in fields_o]
    assert offs[len(fields_o):] == [getattr(_lib.Stats, f).offset for f in fields_s]
    # the stub in INTEGRATION.md declares the same two structs by hand
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    stub = md[md.index("import ctypes as C, numpy as np"):]
    stub = stub[:stub.index("```")]
    decl = stub[stub.index("class Opts"):stub.index("L.cfmm_last_error.restype")]
    ns = {"C": ctypes}
    exec(decl, ns)
    assert [f for f, _ in ns["Opts"]._fields_] == fields_o and ctypes.sizeof(ns["Opts"]) == ctypes.sizeof(_lib.Opts)
    assert [f for f, _ in ns["Stats"]._fields_] == fields_s and ctypes.sizeof(ns["Stats"]) == ctypes.sizeof(_lib.Stats)


def test_ctypes_plumbing_shortcuts_agree_with_the_plain_forms():
    """the per-solve shortcuts of cfmm/_lib.py (round 4: 34 -> ~20 us of Python per solve): the statistics record unpacked in one
    struct.unpack equals the field-by-field read; a float64 array passed as a zero-length ctypes array over its buffer is the
    same address as ndarray.ctypes.data_as gives (read-only arrays take the slow way); the options record is rebuilt when an
    argument changes and only then"""
    st = _lib.Stats()
    vals = dict(evals=22, iters=21, status=1, n_ranks=1, dual_value=1.5, primal_value=1.25, gap=1e-7, infeas=2e-7, wall_seconds=5e-4,
                device_seconds=4.5e-4, pg=0.125, pool_subproblems=22_000_000, barrier_mu=1e-9, newton_steps=8, method=2)
    for k, v in vals.items():
        setattr(st, k, v)
    assert st.asdict() == {k: getattr(st, k) for k, _ in _lib.Stats._fields_} == vals
    dp = ctypes.POINTER(ctypes.c_double)
    a = np.arange(7.0)
    for arr in (a, a[:0].copy(), np.zeros((3, 4))):
        assert ctypes.addressof(_lib._d(arr)) == arr.ctypes.data or arr.size == 0
    ro = np.arange(5.0); ro.flags.writeable = False
    assert ctypes.cast(_lib._d(ro), ctypes.c_void_p).value == ro.ctypes.data and isinstance(_lib._d(ro), dp)
    assert _lib._d(None) is None

    class Ctx(_lib.Context):                  # (the options logic alone: no library behind it)
        def __init__(self):
            self.calls = 0
        def default_opts(self):
            self.calls += 1
            o = _lib.Opts(); o.tol_gap = o.tol_infeas = 1e-6; o.max_evals = 2000
            return o
        def __del__(self):
            pass
    c = Ctx()
    o1 = c._opts(dict(tol=1e-6, max_evals=100, method="lbfgs"))
    assert c._opts(dict(tol=1e-6, max_evals=100, method="lbfgs")) is o1 and c.calls == 1
    o2 = c._opts(dict(tol=1e-8, max_evals=100, method="lbfgs"))
    assert o2 is not o1 and o2.tol_gap == 1e-8 and o1.tol_gap == 1e-6 and o2.max_evals == 100 and o2.method == _lib.METHODS["lbfgs"]
    with pytest.raises(TypeError):
        c._opts(dict(no_such_option=1))


def test_no_kernel_of_the_library_carries_a_private_segment(tmp_path):
    """`table_newton_kernel<true>` had picked up a 16-byte private segment (three spilled dwords) behind the builder's
    last resource check -- a tool, not a test.  Here the check reads the code object the built library CARRIES (no recompilation): the
    .hip_fatbin section -> the gfx950 bundle -> its AMDGPU metadata note; every kernel must report .private_segment_fixed_size 0, and
    the register-bound kernels must stay inside the budget their launch geometry assumes."""
    import shutil, subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("the ROCm LLVM binutils are not installed")
    so = _lib.build()
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "co.elf")
    subprocess.check_call([tools[0], f"--dump-section=.hip_fatbin={fat}", so, str(tmp_path / "rest.so")])
    subprocess.check_call([tools[1], "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    notes = subprocess.run([tools[2], "--notes", co], capture_output=True, text=True, check=True).stdout
    rows = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", notes, re.S):
        g = lambda k: int((re.search(r"\.%s:\s+(\d+)" % k, m.group(2)) or [0, 0])[1])
        rows[m.group(1)] = dict(scratch=g("private_segment_fixed_size"), vgpr=g("vgpr_count"), agpr=g("agpr_count"))
    assert len(rows) >= 140, len(rows)                 # (every device kernel of the library: 145 at the time of writing)
    spilled = {k: v for k, v in rows.items() if v["scratch"]}
    assert not spilled, spilled
    for k, v in rows.items():
        if "iter_kernel" in k or ("eval_kernel" in k and "table" not in k) or "eval_batch_kernel" in k:
            assert v["vgpr"] + v["agpr"] <= 128, (k, v)     # 16 waves of 1024 threads per CU: 4 per SIMD
        if "table_eval_kernel" in k or "table_newton_kernel" in k:
            assert v["vgpr"] + v["agpr"] <= 256, (k, v)     # 8 waves of 512 threads: 2 per SIMD


def test_product_fails_loudly_without_gpu():
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is visible")
    except ImportError:
        pass
    with pytest.raises(cfmm.CfmmError, match="no HIP device|no CPU"):
        _lib.Context(4)
    inst = I.arbitrage()
    p = problem_of(inst)
    with pytest.raises(cfmm.CfmmError):
        p.solve()


def test_bench_dump_outputs_samples_large_trade_sets(tmp_path):
    """bench.py --dump-outputs: float64 files; trade sets past the budget keep the same fraction of every bucket's pools, a seeded
    sample in pool order that two dumps share; trade sets inside the budget are written whole"""
    import types
    import bench
    rng = np.random.default_rng(5)
    trades = {"cp2": (rng.random((2, 300_000)), rng.random((2, 300_000))), 3: (rng.random((3, 50_000)), rng.random((3, 50_000))),
              ("sum", 4): (rng.random((4, 20_000)), rng.random((4, 20_000)))}
    prob = types.SimpleNamespace(value=2.5, dual_value=2.5000001, nu=rng.random(7), psi=rng.random(7).astype(np.float32), _trades=lambda: trades)
    budget = 4 << 20
    got = []
    for run in ("a", "b"):
        names = bench.dump_outputs(prob, str(tmp_path / run), budget=budget)
        got.append({k: np.load(tmp_path / run / (k + ".npy")) for k in names})
    assert set(got[0]) == {"objective", "nu", "psi"} | {f"trades_{b}_{w}" for b in ("cp2", "gn3", "gk_sum4") for w in ("delta", "lambda")}
    assert all(a.dtype == np.float64 for a in got[0].values())
    assert all(np.array_equal(got[0][k], got[1][k]) for k in got[0])
    assert got[0]["objective"].tolist() == [2.5, 2.5000001] and np.array_equal(got[0]["psi"], prob.psi.astype(np.float64))
    assert sum(a.nbytes for k, a in got[0].items() if k.startswith("trades_")) <= budget
    frac = budget / sum(d.nbytes + l.nbytes for d, l in trades.values())
    for key, name in (("cp2", "cp2"), (3, "gn3"), (("sum", 4), "gk_sum4")):
        d, l = trades[key]
        sd, sl = got[0][f"trades_{name}_delta"], got[0][f"trades_{name}_lambda"]
        assert sd.shape == sl.shape == (d.shape[0], int(frac * d.shape[1]))
        pos = np.searchsorted(d[0], sd[0], sorter=np.argsort(d[0]))
        idx = np.argsort(d[0])[pos]                     # (random columns: row 0 identifies a pool)
        assert np.all(np.diff(idx) > 0) and np.array_equal(d[:, idx], sd) and np.array_equal(l[:, idx], sl)
    whole = bench.dump_outputs(prob, str(tmp_path / "c"))
    assert all(np.array_equal(np.load(tmp_path / "c" / f"trades_cp2_{w}.npy"), a) for w, a in zip(("delta", "lambda"), trades["cp2"]))
    assert len(whole) == len(got[0])


def test_bench_self_launches_one_rank_per_gpu(tmp_path):
    """`python bench.py --gpus N` (the driver's command, no launcher around it) must start N ranks itself; without
    GPUs every rank then refuses loudly instead of falling back to anything"""
    import subprocess
    import sys
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is visible")
    except ImportError:
        pytest.skip("torch missing")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    # (the launcher stops the surviving rank as soon as one has failed: one or both get to print)
    assert re.search(r"rank [01] of 2: --gpus 2 but only 0 GPU\(s\) are visible", r.stderr), r.stderr[-2000:]


@pytest.mark.parametrize("cfg", ["C2", "C3", "C4", "C5", "C4x4", "C3zipf"])
def test_committed_bench_lines_keep_the_contract(cfg):
    """profiles/r06_bench_*.json: the round's driver-reproducible line of every BASELINE.json configuration that fits one GPU
    (`python bench.py --config Cx` on MI355X, tools/gpu_profile.sh), plus the two lines SURVEY 8(d) asks for beside them (C4x4:
    a pool set that MUST stream from HBM; C3zipf: hub-weighted token pairs) -- BASELINE's metric and unit, whole-job value
    consistent with evaluations x pools / time, BOTH ceilings in the roofline object with `bound` naming the binding one, the
    CPU baseline beside it"""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "profiles", "r06_bench_%s.json" % cfg)
    d = json.loads([l for l in open(path).read().splitlines() if l.startswith("{")][-1])
    base = json.load(open(os.path.join(root, "BASELINE.json")))
    assert d["metric"] == base["metric"] and d["unit"] == "pool-subproblems/s" and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["n_gpus"] == 1 and d["dtype"] == "f64" and d["data"] == "synthetic"
    assert d["config"]["workload"].startswith(("C3" if cfg == "C3zipf" else cfg) + ":")
    assert "model" not in d["config"] and d["scaling"] == ("strong" if cfg in ("C4", "C4x4") else "weak")
    work = d["evals_per_solve"] * d["config"]["pools_total"]
    assert abs(d["ms_per_step"] * 1e-3 * d["value"] - work) <= 1e-6 * work
    assert d["gap"] <= 1e-6 and d["infeas"] <= 1e-6
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "valu") and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and rf["avg_launch_us"] > 0
    # round 6: the line explains itself -- blocks of the timed steps, the shader clock measured live (a pass of its own
    # behind the timed region) beside the idle clock, the line's kernel times against profiles/budget.json
    blocks = d["ms_per_step_blocks"]
    assert len(blocks) == 5 and abs(sum(blocks) / 5 - d["ms_per_step"]) <= 0.02 * d["ms_per_step"] and max(blocks) <= 1.12 * min(blocks)
    assert min(blocks) <= d["ms_per_step_median_block"] <= max(blocks) and d["extra_warmup_steps"] >= 100
    assert 1.5 < rf["effective_clock_ghz_live"] <= 2.5 and 2.2 < rf["clock_ghz_idle"] <= 2.5 and rf["clock_pass"]["solves"] >= 20
    assert 5.5 < rf["clock_probe_fma_chain"]["cycles_per_dependent_v_fma_f64"] < 8.0
    if cfg != "C3zipf":
        assert d["budget_ok"] is True and d["budget"]["over"] == {} and d["budget"]["checked"]
    if cfg == "C5":                                   # second-order path: the dense factorisation against the fp64 vector peak
        assert rf["unit"] == "TFLOP/s" and rf["peak"] == 78.6 and rf["bound"] == "valu" and d["newton_steps_per_solve"] >= 3
        assert set(rf["newton_step_us"]) == {"smoothed_evaluation_with_hessian", "smoothed_evaluation", "factorisation", "back_substitution"}
        assert rf["flop_frac"] == rf["frac"] and rf["valu_frac"] is None       # a flop rate, NOT the PMC issue fraction
        # round 5: the kernel the rocprof summary lists, its launch count, the issued and the useful flop fractions
        assert rf["kernel"].startswith("chol_step2_kernel") and rf["launches_per_factorisation"] == 17
        assert abs(rf["useful_flop_frac"] * 3.0 - rf["flop_frac"]) <= 1e-12 and "useful_flop_frac" in rf["flop_frac_note"]
        assert rf["rocprof_source"].endswith("kernel_stats_C5newton.csv") and 10.0 < rf["rocprof_avg_per_launch_us"] < 25.0
        assert abs(rf["rocprof_avg_launch_us"] - rf["avg_launch_us"]) <= 0.12 * rf["avg_launch_us"]     # the chain: trace x launches against HIP events
        assert d["ms_per_step"] <= 4.6                # (round 2: 13.6, round 3: 6.6, round 4: 4.1-4.2)
        sp = d["start_prices"]                        # memoised start prices said out loud, with the un-memoised time beside it
        assert sp["ms_per_step_memoised"] == d["ms_per_step"] and sp["ms_per_step_recomputed"] >= 0.93 * sp["ms_per_step_memoised"]      # (O(n) extra: within the run-to-run noise of two 10-step timings)
        assert "EVALUATIONS only" in d["cpu_baseline"]["measures"]
    else:
        # `frac` prices the algorithmic bytes (the contract), `hbm_frac` the bytes as stored: equal unless a compact mirror exists
        # (round 5: the K-asset buckets' log(R/w) column is counted as stored -- more than the algorithm names where such pools exist)
        assert rf["unit"] == "GB/s" and rf["peak"] == 8000.0
        ratio = rf["bytes_as_stored_per_launch"] / rf["algorithmic_bytes_per_launch"]
        assert abs(rf["hbm_frac"] - rf["frac"] * ratio) <= 1e-9
        mirrored = ratio < 1.0
        assert mirrored == (cfg in ("C4", "C4x4")) and (ratio == 1.0) == (cfg == "C2") and ratio <= 1.15
        assert rf["traffic"] is None or abs(rf["traffic"] - rf["bytes_as_stored_per_launch"]) <= (0.12 if cfg != "C2" else 3.0) * rf["bytes_as_stored_per_launch"]
        assert rf["bound"] == ("valu" if (rf["valu_frac"] or 0.0) > rf["hbm_frac"] else "hbm")
        assert rf["evaluation_only"]["bound"] in ("hbm", "valu") and 0.0 < rf["evaluation_only"]["hbm_frac"] < 1.0
    if cfg != "C3zipf":                               # (the stress variant is timed without the CPU leg)
        cb = d["cpu_baseline"]
        assert cb["kind"] == "port" and cb["unit"] == "pool-subproblems/s" and cb["cores"] >= 1 and cb["value"] > 0 and cb["sample"]
        # BASELINE.md section 4's baseline B beside A: vectorised NumPy on one thread, where the restatement covers the pool kinds and
        # the pool set fits the host's memory several times over
        if cfg in ("C2", "C3", "C4"):
            nb = cb["numpy_one_thread"]
            assert nb["cores"] == 1 and nb["kind"] == "port" and 1e6 < nb["value"] < cb["value"] and "one thread" in nb["sample"]
        else:
            assert "numpy_one_thread" not in cb
    if cfg == "C3":
        assert d["ms_per_step"] <= 0.52 and d["value"] >= 4.2e10      # (round 2: 0.594 ms, 3.70e10; round 5's driver line: 0.574)
        assert rf["avg_launch_us"] <= 20.6 and rf["frac"] >= 0.26     # (rounds 4-5: 20.0-20.9 us)
        # the live clock accounts for the launch: duration x clock in shader cycles, live against the profiled pass
        cc = rf["clock_check"]
        assert 0.9 < cc["time_ratio_live_over_profiled"] < 1.1 and cc["launch_shader_cycles_live"] > 0
    if cfg == "C4":
        assert rf["avg_launch_us"] <= 52.0 and rf["frac"] >= 0.78  # (round 2: 68-69 us, 0.58; round 3: 59.4; before the mirror: 58.1)
        assert rf["bytes_as_stored_per_launch"] == 210_000_000 and rf["hbm_frac"] >= 0.5
        assert "PARTLY CACHE-SERVED" in rf["note"]    # 210 MB as stored against a 256 MiB Infinity Cache is not an HBM figure
    if cfg == "C4x4":                                 # 1.28 GB of algorithmic columns per launch, 0.84 GB as stored: the HBM-streaming figure
        assert rf["algorithmic_bytes_per_launch"] == 1_280_000_000 and rf["bytes_as_stored_per_launch"] == 840_000_000 and rf["bound"] == "hbm"
        assert rf["avg_launch_us"] <= 172.0           # (before the mirror and the wide tiles: 198-208)
        assert rf["hbm_frac"] >= 0.62 and rf["evaluation_only"]["hbm_frac"] >= 0.70 and rf["frac"] >= 0.93
    if cfg == "C3zipf":
        assert "Zipf(1.1)" in d["config"]["workload"] and rf["avg_launch_us"] <= 24.0


def test_product_never_imports_oracle():
    """the oracle is test infrastructure: no import, include, link or dlopen of it in the product"""
    pkg = os.path.join(ROOT, "cfmm-routing-code_amd")
    pat = re.compile(r"^\s*(import\s+oracle|from\s+oracle|#\s*include.*oracle)|dlopen\(.*oracle|libcfmm_oracle|c_oracle", re.M)
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")) or f == "Makefile":
                src = open(os.path.join(dirpath, f)).read()
                assert not pat.search(src), f"{f} uses the oracle"


def test_pack_roundtrip_and_validation():
    inst = I.arbitrage()
    net, where = cfmm.pack(inst["n_tokens"], inst["local_indices"], inst["reserves"], inst["fees"], inst["kinds"], inst["weights"])
    assert where == [(4, 0), ("cp2", 0), ("cp2", 1), ("cp2", 2), ("sum2", 0)]
    assert net["gn"][4]["idx"].shape == (4, 1) and np.allclose(net["gn"][4]["w"][:, 0], [.4, .3, .2, .1])
    with pytest.raises(ValueError):
        cfmm.pack(3, [[0, 0]], [[1, 1]], [0.99])
    with pytest.raises(ValueError):
        cfmm.pack(3, [[0, 5]], [[1, 1]], [0.99])
    with pytest.raises(ValueError):
        cfmm.pack(3, [[0, 1]], [[1, -1]], [0.99])
    # three-token constant-sum / stableswap pools: the K-asset table's buckets (round 4; they were refused before)
    net3, where3 = cfmm.pack(3, [[0, 1, 2], [2, 0, 1]], [[1, 1, 1], [2, 3, 4]], [0.99, 0.999], kinds=["sum", "curve"], params=[None, 5.0])
    assert where3 == [(("sum", 3), 0), (("stable", 3), 0)] and cfmm.problem.network_pool_count(net3) == 2
    assert net3["gk"][("stable", 3)]["idx"][:, 0].tolist() == [2, 0, 1] and net3["gk"][("stable", 3)]["param"][0] == 5.0
    with pytest.raises(ValueError):
        cfmm.pack(3, [[0, 1, 2]], [[1, 1, 1]], [0.99], kinds=["curve"])              # alpha missing
    with pytest.raises(ValueError):
        cfmm.pack(12, [list(range(9))], [[1.0] * 9], [0.99], kinds=["sum"])          # more than 8 tokens
    # empty problem object
    net, where = cfmm.pack(3, [], [], [])
    assert where == [] and cfmm.problem.network_pool_count(net) == 0


def test_shard_network_partitions_every_bucket():
    net = synthetic.config("C3", scale=0.001)
    parts = [cfmm.shard_network(net, r, 3) for r in range(3)]
    for key in ("cp2", "w2"):
        assert np.array_equal(np.concatenate([p[key]["Ra"] for p in parts]), net[key]["Ra"])
    for k in net["gn"]:
        assert np.array_equal(np.concatenate([p["gn"][k]["R"] for p in parts], axis=1), net["gn"][k]["R"])
    netk = synthetic.config("GK", scale=0.02)
    parts = [cfmm.shard_network(netk, r, 3) for r in range(3)]
    for key in netk["gk"]:
        assert np.array_equal(np.concatenate([p["gk"][key]["R"] for p in parts], axis=1), netk["gk"][key]["R"])
        assert np.array_equal(np.concatenate([p["gk"][key]["param"] for p in parts]), netk["gk"][key]["param"])
    assert sum(cfmm.problem.network_pool_count(p) for p in parts) == cfmm.problem.network_pool_count(netk)


def test_start_prices_propagate_through_pools():
    inst = I.liquidation()
    p = problem_of(inst)
    nu0 = cfmm.start_prices(p.net, p.utility)
    assert nu0[4] == 1.0 and np.all(nu0 > 0) and np.all(np.isfinite(nu0))
    # a consistent network gives back its latent prices exactly
    net = synthetic.make_network(50, m_cp2=400, seed=1, mispricing=0.0)
    c = np.zeros(50); c[7] = net["prices"][7]
    nu0 = cfmm.start_prices(net, cfmm.Utility(c))
    assert np.abs(nu0 / net["prices"] - 1).max() < 1e-9


def test_start_prices_from_network_potentials():
    """cfmm.problem._potentials: one least-squares fit per network (cached in the network dict, not inherited by shards), O(n)
    per utility -- several priced tokens shift it by their mean, a component the utility prices nowhere gets 1, another utility
    on the same network costs no new fit"""
    net = synthetic.make_network(60, m_cp2=600, m_w2=100, m_gn=60, seed=3, mispricing=0.0)
    pi = net["prices"]
    c = np.zeros(60); c[[3, 17, 40]] = pi[[3, 17, 40]] * np.array([1.0, 1.02, 0.98])       # inconsistent by +-2 %: the fit takes their mean
    nu0 = cfmm.start_prices(net, cfmm.Utility(c))
    assert np.array_equal(nu0[[3, 17, 40]], c[[3, 17, 40]])                                  # priced tokens keep their price
    free = np.setdiff1d(np.arange(60), [3, 17, 40])
    shift = np.exp(np.mean(np.log([1.0, 1.02, 0.98])))
    assert np.abs(nu0[free] / (pi[free] * shift) - 1).max() < 1e-9
    fit = net["_potentials"]
    c2 = np.zeros(60); c2[5] = 2.0 * pi[5]
    nu1 = cfmm.start_prices(net, cfmm.Utility(c2))
    assert net["_potentials"] is fit and np.abs(nu1 / (2.0 * pi) - 1).max() < 1e-9          # the same fit, another anchor
    assert "_potentials" not in cfmm.shard_network(net, 0, 2) and "_price_relations" not in cfmm.shard_network(net, 0, 2)
    # two components: tokens 0-29 and 30-59 never share a pool; the utility prices only the first
    a = synthetic.make_network(30, m_cp2=300, seed=4, mispricing=0.0)
    two = dict(n_tokens=60, prices=np.concatenate([a["prices"], a["prices"]]), c=np.concatenate([a["c"], a["c"]]), seed=0,
               cp2={k: np.concatenate([a["cp2"][k], a["cp2"][k] + (30 if k in ("ia", "ib") else 0)]) for k in a["cp2"]})
    c3 = np.zeros(60); c3[7] = a["prices"][7]
    nu2 = cfmm.start_prices(two, cfmm.Utility(c3))
    assert np.abs(nu2[:30] / a["prices"] - 1).max() < 1e-9 and np.all(nu2[30:] == 1.0)


@pytest.mark.parametrize("name,inst", shipped_cases())
def test_host_logic_reproduces_shipped_instances(oracle_lib, name, inst):
    """objective, psi and every pool's tenders, incl. the partially filled constant-sum pool"""
    g = golden()[name]
    p = problem_of(inst, OracleContext(inst["n_tokens"]))
    v = p.solve(tol=1e-10)
    assert p.status == "optimal"
    assert abs(v - g["survey"]["value"]) <= 1e-8 * max(1, abs(v))
    assert abs(v - g["kkt"]["value"]) <= 1e-9 * max(1, abs(v))
    assert p.gap <= 1e-10 and p.infeas <= 1e-10
    # psi and every pool's tenders against the 50-digit KKT solution: 1e-6 absolute is the bar,
    # 2e-8 is what a solve to 1e-10 certificates reaches
    assert np.abs(p.psi - np.asarray(g["kkt"]["psi"])).max() <= 2e-8
    for d, l, y in zip(p.deltas, p.lambdas, g["kkt"]["y"]):
        assert np.all(d >= 0) and np.all(l >= 0) and np.all(d * l == 0)
        assert np.abs((l - d) - np.asarray(y)).max() <= 1e-6
        assert np.abs((l - d) - np.asarray(y)).max() <= 2e-8
    if "nu" in g["survey"] and not name.startswith("two_asset"):   # (token 1's price is not unique there)
        assert np.abs(p.nu / np.asarray(g["survey"]["nu"]) - 1).max() <= 1e-5


def test_two_asset_full_sweep_monotone(oracle_lib):
    """two-asset.py:40-100: u(t) over the 50-point sweep is increasing and concave"""
    vals = []
    nu = None
    for t in I.two_asset_sweep():
        p = problem_of(I.two_asset(t), OracleContext(3))
        vals.append(p.solve(tol=1e-9, nu0=nu)); nu = p.nu
        assert p.status == "optimal"
    vals = np.array(vals)
    assert np.all(np.diff(vals) > 0) and np.all(np.diff(vals, 2) < 1e-7)
    assert abs(vals[0] - 6.2330001314) < 1e-7 and abs(vals[-1] - 44.1820204014) < 1e-7


@pytest.mark.parametrize("seed", range(24))
def test_random_instances_with_constant_sum_pools(oracle_lib, seed):
    util = ["arbitrage", "swap", "liquidate"][seed % 3]
    inst = random_instance(100 + seed, n_tokens=5 + seed % 3, n_pools=10 + seed % 5, with_sum=True,
                           with_curve=(seed % 2 == 1), utility=util)
    p = problem_of(inst, OracleContext(inst["n_tokens"]))
    v = p.solve(tol=1e-9)
    r = solve_primal(normalise_with_params(inst))
    if p.status == "infeasible":          # a token to sell that no pool lists: SLSQP fails on it too
        assert not r["success"]
        return
    assert p.status == "optimal" and p.gap <= 1e-8 and p.infeas <= 1e-8
    assert r["value"] <= v + 2e-6 * max(1, abs(v))
    if r["success"]:
        assert abs(v - r["value"]) <= 2e-6 * max(1, abs(v)), (v, r["value"], p._theta)


def test_barrier_smoothed_constant_sum_pool_against_finite_differences(tmp_path):
    """csrc/phik.hpp: sum_smooth_k -- the K-asset constant-sum pool (arbitrage.py:73-74 over K tokens) with the second-order path's log
    barrier on its sign constraints -- is __host__ __device__: compiled for the HOST here and checked without a GPU.  The pool's
    constraint holds to rounding, the value tends to the LP's as the weight shrinks, its gradient is L - D and its Hessian the closed
    form, both against central differences."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc missing")
    src = tmp_path / "t.hip"
    src.write_text(r'''
#include "phik.hpp"
#include <cstdio>
#include <cmath>
using namespace cfmm;
int main()
{
    constexpr int K = 4;
    double R[K] = {31.5, 29.4, 27.2, 15.5}, p[K] = {1.005, 1.007, 1.0, 1.0153};
    const double g = 0.99;
    for (double mu : {1e-1, 1e-3, 1e-6, 1e-10}) {
        SumSmooth<K> o; sum_smooth_k<K>(R, p, g, mu, o);
        double bal = 0, minslack = 1e300;
        for (int j = 0; j < K; ++j) { bal += g * o.D[j] - o.L[j]; minslack = std::fmin(minslack, std::fmin(std::fmin(o.L[j], R[j] - o.L[j]), o.D[j])); }
        double maxg = 0, maxh = 0;
        for (int k = 0; k < K; ++k) {
            const double e = 1e-6 * std::fmax(mu, 1e-4);
            double pp[K], pm[K]; for (int j = 0; j < K; ++j) { pp[j] = pm[j] = p[j]; } pp[k] += e; pm[k] -= e;
            SumSmooth<K> a, b; sum_smooth_k<K>(R, pp, g, mu, a); sum_smooth_k<K>(R, pm, g, mu, b);
            maxg = std::fmax(maxg, std::fabs((a.val - b.val) / (2 * e) - (o.L[k] - o.D[k])));
            for (int j = 0; j < K; ++j) {
                const double fh = ((a.L[j] - a.D[j]) - (b.L[j] - b.D[j])) / (2 * e);
                maxh = std::fmax(maxh, std::fabs(fh - sum_smooth_hess<K>(o, g, j, k)) / (1.0 + std::fabs(fh)));
            }
        }
        printf("%.0e %.12g %.12g %.3e %.3e %.3e %.3e\n", mu, o.val, o.trade, bal, minslack, maxg, maxh);
    }
    return 0;
}
''')
    exe = tmp_path / "t"
    inc = os.path.join(ROOT, "cfmm-routing-code_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I", inc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.strip().splitlines()
    rows = [[float(x) for x in l.split()] for l in out]
    assert [r[0] for r in rows] == [1e-1, 1e-3, 1e-6, 1e-10]
    # the LP's value at these prices: token 5 (price 1.0) pays for the whole of token 2 (price 1.0153): R (p - 1 / gamma)
    lp = 15.5 * (1.0153 - 1.0 / 0.99)
    for mu, val, trade, bal, minslack, maxg, maxh in rows:
        assert abs(bal) <= 1e-12 * 100.0 and minslack > 0.0                      # feasible, strictly inside
        assert lp - 1e-12 <= trade + 12 * mu and trade <= lp + 1e-9              # p'y within 3 K mu of the LP's value, never above it
        assert maxg <= 1e-4 and maxh <= 2e-3                                     # (central differences at step 1e-6 max(mu, 1e-4))
    assert abs(rows[-1][2] - lp) <= 1e-8


def test_first_order_plan_over_every_combination_of_its_facts(tmp_path):
    """csrc/solve_plan.hpp: plan_first_order -- which host driver runs a first-order solve, and under which envelope -- is a pure host
    function of eleven booleans and three integers: compiled for the HOST here and run over every combination of the booleans, crossed
    with one and two ranks, four chunk lengths and the evaluation budgets around the 24 bits the sealed envelope's words carry.  Every
    line against the rules restated below (from the design, not from the header)."""
    import itertools
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc missing")
    bools = ["tiny_applies", "fused_applies", "sharded", "oneshot_runahead", "multi_graph", "os_ready", "no_graph", "det",
             "fused_graph", "zero_copy_off", "envelope_classic"]
    ranks, chunk, budget = (1, 2), (1, 3, 4, 256), (1, 0xfffffe, 0xffffff)
    src = tmp_path / "plan.cpp"
    src.write_text(r'''
#include "solve_plan.hpp"
#include <cstdio>
int main()
{
    const int ranks[] = {%s}, chunk[] = {%s}, budget[] = {%s};
    for (unsigned m = 0; m < (1u << %d); ++m)
        for (int nr : ranks) for (int ipg : chunk) for (int me : budget) {
            PlanFacts f;
%s
            f.n_ranks = nr; f.iters_per_graph = ipg; f.max_evals = me;
            const FirstOrderPlan p = plan_first_order(f);
            const char *d = p.drive == Drive::Tiny ? "Tiny" : p.drive == Drive::Eager ? "Eager" : p.drive == Drive::RingChunks ? "RingChunks" : "Chunks";
            printf("%%u %%d %%d %%d %%s %%d %%d %%d %%d %%d\n", m, nr, ipg, me, d, (int)p.fused, (int)p.use_graph, (int)p.zero_copy, (int)p.sealed, p.iters_per_graph);
        }
    return 0;
}
''' % (", ".join(map(str, ranks)), ", ".join(map(str, chunk)), ", ".join(map(str, budget)), len(bools),
       "\n".join(f"            f.{b} = (m >> {i}) & 1u;" for i, b in enumerate(bools))))
    exe = tmp_path / "plan"
    r = subprocess.run([hipcc, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "cfmm-routing-code_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.strip().splitlines()

    def plan(f):
        tiny = f["tiny_applies"]
        fused = not tiny and f["fused_applies"]
        ipg = f["iters_per_graph"]
        if fused:
            ipg = -(-ipg // 3) * 3
        if f["sharded"] and f["n_ranks"] > 1 and not f["oneshot_runahead"] and not f["multi_graph"]:
            ipg = 3
        graph_opt = fused and not f["sharded"] and f["fused_graph"]
        use_graph = (not tiny and (not f["sharded"] or (f["multi_graph"] and not f["os_ready"])) and not f["no_graph"]
                     and (not fused or f["sharded"] or f["fused_graph"]))
        zero_copy = fused and not f["sharded"] and not graph_opt and not f["det"] and not f["zero_copy_off"]
        sealed = zero_copy and not f["envelope_classic"] and f["max_evals"] < 0xffffff
        if tiny:
            drive = "Tiny"
        elif fused and (not f["sharded"] or f["oneshot_runahead"]) and not graph_opt:
            drive = "Eager"
        elif fused and f["sharded"] and not use_graph:
            drive = "RingChunks"
        else:
            drive = "Chunks"
        return drive, int(fused), int(use_graph), int(zero_copy), int(sealed), ipg

    want = []
    for m in range(1 << len(bools)):
        for nr, ipg, me in itertools.product(ranks, chunk, budget):
            f = {b: bool((m >> i) & 1) for i, b in enumerate(bools)}
            f.update(n_ranks=nr, iters_per_graph=ipg, max_evals=me)
            want.append("%d %d %d %d %s %d %d %d %d %d" % ((m, nr, ipg, me) + plan(f)))
    assert len(got) == len(want) == (1 << len(bools)) * len(ranks) * len(chunk) * len(budget)
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, (len(bad), bad[:5])
    assert {l.split()[4] for l in got} == {"Tiny", "Eager", "RingChunks", "Chunks"}


def _newton_rules_program(tmp_path, name, body):
    """a stand-alone HOST program over csrc/newton_rules.hpp (nothing of HIP in it): compiled -Wall -Werror, run, its output lines"""
    return _rules_program(tmp_path, "newton_rules.hpp", "newton", name, body)


def _rules_program(tmp_path, header, namespace, name, body, helpers=""):
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc missing")
    src = tmp_path / f"{name}.cpp"
    src.write_text(f'#include "{header}"\n#include <cstdio>\n#include <vector>\nusing namespace {namespace};\n'
                   'inline void row(const char *k, const double *v, int n) { printf("%s", k); for (int i = 0; i < n; ++i) printf(" %.17g", v[i]); printf("\\n"); }\n'
                   + helpers + "int main()\n{\n" + body + "\n    return 0;\n}\n")
    exe = tmp_path / name
    r = subprocess.run([hipcc, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "cfmm-routing-code_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.strip().splitlines()


def _same_numbers(got, want, rel=1e-15):
    got = [float(x) for x in got]
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        assert g == w or abs(g - w) <= rel * abs(w), (g, w, got, want)


def test_second_order_chord_rule_over_every_combination_of_its_facts(tmp_path):
    """csrc/newton_rules.hpp: chord_allowed -- may a step reuse the factor the device holds.  One rule for "this step" and for "the step
    behind this trial": every combination of its boolean facts, the run of chord steps at 0, one under and at its cap, the move either
    side of 1e-10.  Against the rule restated from the design: a valid factor, made at this weight, behind a full step, outside the
    low-order regime, a move above 1e-10, not refused since, the run under its cap, no diagonal shift, the inverse factor kept."""
    import itertools
    bools = ["fac_valid", "same_weight", "full_step", "slo", "chord_bad", "shifted", "inverse_factor"]
    chord_max, runs, moves = 3, (0, 2, 3), (0.99e-10, 1.01e-10)
    got = _newton_rules_program(tmp_path, "chord", r'''
    const int runs[] = {%s}; const double moves[] = {%s};
    for (unsigned m = 0; m < (1u << %d); ++m) for (int run : runs) for (double mv : moves) {
        ChordFacts f;
        f.fac_valid = m & 1u; f.fac_mu = 1e-5; f.mu = (m >> 1) & 1u ? 1e-5 : 1e-6; f.full_step = (m >> 2) & 1u; f.slo = (m >> 3) & 1u;
        f.chord_bad = (m >> 4) & 1u; f.reg = (m >> 5) & 1u ? 1e-12 : 0.0; f.inverse_factor = (m >> 6) & 1u;
        f.chord_run = run; f.chord_max = %d; f.move = mv;
        printf("%%u %%d %%.17g %%d\n", m, run, mv, (int)chord_allowed(f));
    }''' % (", ".join(map(str, runs)), ", ".join(repr(x) for x in moves), len(bools), chord_max))
    want = []
    for m in range(1 << len(bools)):
        for run, mv in itertools.product(runs, moves):
            f = {b: bool((m >> i) & 1) for i, b in enumerate(bools)}
            ok = (f["fac_valid"] and f["same_weight"] and f["full_step"] and not f["slo"] and mv > 1e-10 and not f["chord_bad"]
                  and run < chord_max and not f["shifted"] and f["inverse_factor"])
            want.append((m, run, mv, int(ok)))
    assert len(got) == len(want) == (1 << len(bools)) * 6
    for g, w in zip(got, want):
        g = g.split()
        assert (int(g[0]), int(g[1]), float(g[2]), int(g[3])) == w, (g, w)
    assert sum(w[3] for w in want) == 2          # (one combination of the booleans, the two runs under the cap, the larger move)


def test_second_order_schedule_rules_either_side_of_their_thresholds(tmp_path):
    """csrc/newton_rules.hpp: the barrier schedule (first weight, when the exact evaluation is due, the final weight, "the weight stays",
    the shrink behind an accepted step, the stall counter with its forced shrinks, the diagonal shift), the chord direction's test and
    the line search's acceptance -- each at values either side of its threshold, against the rules restated from the design."""
    lo, hi = 1.0 - 1e-9, 1.0 + 1e-9
    tol = 1e-7
    calls, want = [], []

    def call(expr, value):
        calls.append(f'    {{ const double v[] = {{(double)({expr})}}; row("r", v, 1); }}')
        want.append(float(value))
    # the first weight: 0.1 |dual| / nbar, no barrier terms counting as one; a warm start caps it at a multiple of the last weight
    for dual, nbar, warm in ((-40.0, 8, 0.0), (0.0, 8, 0.0), (3.0, 0, 0.0), (3.0, 8, 1e-6), (3.0, 8, 1.0)):
        mu = 0.1 * max(abs(dual), 1e-300) / max(nbar, 1)
        call(f"first_weight(0.1, {dual!r}, {nbar}, {warm!r}, 1e3)", min(mu, 1e3 * warm) if warm > 0 else mu)
    for dual in (0.3, -40.0):
        s = max(1.0, abs(dual))
        for f in (lo, hi):
            call(f"weight_is_final({0.5 * tol * s * f!r}, {dual!r}, {tol!r})", 0.5 * tol * s * f <= 0.5 * tol * s)
            for steps in (0, 1):
                call(f"exact_due({steps}, {10 * tol * s * f!r}, {dual!r}, 0.0, {tol!r}, {tol!r})", steps == 0 or 10 * tol * s * f <= 10 * tol * s)
                call(f"exact_due({steps}, 0.0, {dual!r}, {10 * tol * f!r}, {tol!r}, {tol!r})", steps == 0 or 10 * tol * f <= 10 * tol)
    mu, nbar = 3e-6, 7
    for final in (False, True):
        for dec in (10 * mu * nbar * lo, 10 * mu * nbar * hi, 1e-3 * mu * nbar * lo, 1e-3 * mu * nbar * hi):
            stays = final or not dec < 10 * mu * nbar
            call(f"weight_stays({int(final)}, {dec!r}, {mu!r}, {nbar})", stays)
            for full in (False, True):
                call(f"weight_shrinks({int(final)}, {dec!r}, {mu!r}, {nbar}, {int(full)})", not stays and (full or dec < 1e-3 * mu * nbar))
    # the stall counter at the final weight: (best infeasibility, stalled, forced shrinks) before -> after, the forced shrink, "stalled"
    gmu = -25.0
    for best, stalled, forced, infeas, dec, gap in (
            (1e-3, 2, 0, 0.5e-3 * lo, 1.0, 1.0), (1e-3, 2, 0, 0.5e-3 * hi, 1.0, 1.0),                       # halves the best: counter reset
            (1e-9, 1, 0, 1e-9, 25e-13 * hi, 2 * tol), (1e-9, 1, 0, 1e-9, 25e-13 * lo, 2 * tol),            # decrement at rounding level or not
            (1e-9, 1, 2, 1e-9, 1e-14, tol * hi), (1e-9, 1, 2, 1e-9, 1e-14, tol * lo), (1e-9, 1, 3, 1e-9, 1e-14, 2 * tol),
            (2 * tol, 1, 0, tol * hi, 1e-14, 2 * tol), (2 * tol, 1, 0, tol * lo, 1e-14, 2 * tol), (1e-9, 3, 3, 1e-9, 1e-14, -2 * tol)):
        calls.append(f"    {{ Schedule sc; sc.best_infeas = {best!r}; sc.stalled = {stalled}; sc.forced_shrinks = {forced};\n"
                     f"      const bool end = final_weight_stalls(sc, {infeas!r}, {dec!r}, {gmu!r}, {gap!r}, {tol!r}, {tol!r});\n"
                     f'      const double v[] = {{(double)end, sc.best_infeas, (double)sc.stalled, (double)sc.forced_shrinks, (double)sc.shrink_now}}; row("s", v, 5); }}')
        shrink = False
        if infeas < 0.5 * best:
            best, stalled = infeas, 0
        elif dec <= 1e-13 * max(1.0, abs(gmu)):
            if infeas <= tol and abs(gap) > tol and forced < 3:
                shrink, forced = True, forced + 1
            else:
                stalled += 1
        want.append((float(stalled >= 4), best, float(stalled), float(forced), float(shrink)))
    # the diagonal shift: 1e-12 of the largest entry at first, x 100 per further refusal, out of range at 1e300; x 0.1 per step taken
    for reg, md in ((0.0, 5.0), (0.0, 0.0), (1e-6, 5.0), (1e299, 5.0)):
        calls.append(f'    {{ Schedule sc; sc.reg = {reg!r}; const bool ok = raise_shift(sc, {md!r}); const double v[] = {{(double)ok, sc.reg}}; row("s", v, 2); }}')
        new = 1e-12 * max(md, 1e-300) if reg == 0.0 else reg * 100.0
        want.append((float(new < 1e300), new))
    for reg in (1e-4, 0.0):
        calls.append(f'    {{ Schedule sc; sc.reg = {reg!r}; relax_shift(sc); const double v[] = {{sc.reg}}; row("s", v, 1); }}')
        want.append((0.1 * reg if reg > 0 else 0.0,))
    dec_prev = 4e-3
    for fin, dc in ((1, 1e-2 * dec_prev * lo), (1, 1e-2 * dec_prev * hi), (1, 0.0), (1, -1e-9), (0, 1e-2 * dec_prev * lo), (1, float("nan"))):
        call(f"chord_direction_serves({fin}, {'NAN' if dc != dc else repr(dc)}, {dec_prev!r})", bool(fin) and dc > 0.0 and dc <= 1e-2 * dec_prev)
    armijo, gd = 1e-4, -2.0
    bound = gmu + armijo * gd + 2e-15 * abs(gmu)
    for g2, dec in ((bound, 1.0), (bound + 1e-14, 1.0), (bound + 1.0, 1e-13 * abs(gmu) * lo), (bound + 1.0, 1e-13 * abs(gmu) * hi)):
        call(f"trial_accepted({g2!r}, {gmu!r}, {armijo!r}, {gd!r}, {dec!r})", g2 <= bound or dec <= 1e-13 * abs(gmu))
    for max_step, dmax in ((2.0, 1.0), (2.0, 8.0), (2.0, 0.0)):
        call(f"first_step_length({max_step!r}, {dmax!r})", min(1.0, max_step / max(dmax, 1e-300)))
    got = _newton_rules_program(tmp_path, "schedule", "\n".join(calls))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        _same_numbers(g.split()[1:], w if isinstance(w, tuple) else (w,))


def test_second_order_token_rules_on_one_token_of_each_kind(tmp_path):
    """csrc/newton_rules.hpp on a 7-token vector -- GE with c > 0, GE with c = 0 that a pool lists (a barrier token), the same unlisted
    with h = 0 (flat: pinned, no barrier term), EQ, FREE, ULOG, UQUAD: the prologue's token pass, the start dual (the pools' value plus
    the terms in token order), assemble, the certificate sums (1e-15 relative against the same sums restated here, in token order), the
    exact certificate (refused because of the table entries, accepted with them replaced), and the line search's trial point in both
    regimes with token 0 on its lower bound."""
    import math
    GE, EQ, FREE, ULOG, UQUAD = 0, 1, 2, 3, 4
    ct = [GE, GE, GE, EQ, FREE, ULOG, UQUAD]
    c = [1.2, 0.0, 0.0, 0.9, 1.1, 0.8, 1.3]
    h = [0.3, 0.5, 0.0, 0.4, 0.1, 2.0, 5.0]
    pools = [1, 1, 0, 1, 1, 1, 1]
    nu0 = [1.0, 0.7, 0.6, 0.95, 3.0, 0.5, 1.25]            # (token 0 starts under its bound c: projected; the FREE token goes to c)
    psi = [-0.2, -0.45, 0.0, -0.41, 0.3, -1.5, 0.2]
    n, mu, value, arb, floor = 7, 3e-3, 0.37, 0.41, 1e-12 * 5e4
    d = [-0.3, 0.2, 0.5, -0.1, 0.4, 0.05, -0.25]
    vec = lambda name, a, t="double": f"    const {t} {name}[] = {{{', '.join(repr(x) for x in a)}}};"
    body = "\n".join([vec("ct", ct, "int"), vec("c", c), vec("h", h), vec("pools", pools, "char"), vec("psi", psi), vec("d", d), vec("nu0", nu0)]) + r'''
    const int n = 7; const double mu = %r, value = %r, arb = %r;
    std::vector<double> nu(nu0, nu0 + n), lob(n), s(n), G(n), Hd(n), rhs(n), slo(n, 0.0), s2(n), nu2(n), slo2(n);
    std::vector<int> mask(n), pin(n); std::vector<char> listed(n);
    long long nb = 0;
    double v[8];
    v[0] = token_pass(n, c, h, ct, pools, nu.data(), listed.data(), mask.data(), lob.data(), s.data(), &nb); v[1] = (double)nb; row("pass", v, 2);
    for (int j = 0; j < n; ++j) v[j] = listed[j]; row("listed", v, n);
    for (int j = 0; j < n; ++j) v[j] = mask[j]; row("mask", v, n);
    row("lob", lob.data(), n); row("s", s.data(), n); row("nu", nu.data(), n);
    { double cz[] = {1.2, 0.0, 0.0, 0.9, 0.0, 0.8, 1.3}; std::vector<double> p(nu0, nu0 + n);
      v[0] = token_pass(n, cz, h, ct, pools, p.data(), listed.data(), mask.data(), lob.data(), s.data(), &nb); row("unbounded", v, 1);
      token_pass(n, c, h, ct, pools, p.data(), listed.data(), mask.data(), lob.data(), s.data(), &nb); }
    Tokens tk; tk.n = n; tk.c = c; tk.h = h; tk.ctype = ct; tk.listed = listed.data(); tk.mask = mask.data(); tk.lob = lob.data(); tk.nbar = 4 + nb; tk.infeas_floor = %r;
    for (int j = 0; j < n; ++j) v[j] = tk.barrier_token(j); row("barrier", v, n);
    v[0] = start_dual(tk, nu.data(), arb); row("start_dual", v, 1);
    v[0] = assemble(tk, nu.data(), psi, value, mu, G.data(), Hd.data()); row("g", v, 1); row("G", G.data(), n); row("Hd", Hd.data(), n);
    v[0] = assemble(tk, nu.data(), psi, value, mu, nullptr, nullptr); row("g_only", v, 1);
    { const Certificate k = certificate(tk, nu.data(), psi); const double w[] = {k.lin, k.primal, k.cs, k.viol, k.scale, k.infeas(tk)}; row("cert", w, 6); }
    { const ExactCertificate x = exact_certificate(tk, nu.data(), psi, arb, 1e-6, 1e-6); v[0] = x.holds; row("exact_table", v, 1); }
    { const int ct2[] = {0, 0, 0, 1, 2, 0, 0}; Tokens t2 = tk; t2.ctype = ct2;
      double px[7]; for (int j = 0; j < n; ++j) px[j] = -h[j];
      ExactCertificate x = exact_certificate(t2, nu.data(), px, arb, 1e-6, 1e-6); const double w[] = {(double)x.holds, x.dual, x.gap, x.infeas, x.primal}; row("exact_holds", w, 5);
      x = exact_certificate(t2, nu.data(), psi, arb, 1e-6, 1e-6); const double w2[] = {(double)x.holds, x.dual, x.gap, x.infeas, x.primal}; row("exact_fails", w2, 5);
      t2.ctype = ct; x = exact_certificate(t2, nu.data(), px, arb, 1e-6, 1e-6); v[0] = x.holds; row("exact_table_feasible", v, 1); }
    G[0] = 0.25;                                   // (pushing token 0, on its bound, further down: pinned by the projection)
    pin_and_right_hand_side(tk, s.data(), slo.data(), 1e-9, G.data(), Hd.data(), pin.data(), rhs.data());
    for (int j = 0; j < n; ++j) v[j] = pin[j]; row("pin", v, n); row("rhs", rhs.data(), n); row("Hd_shifted", Hd.data(), n);
    G[0] = 0.25;
    for (int pass = 0; pass < 3; ++pass) {
        if (pass == 2) slo[1] = 2e-10;             // (a low-order part already too large for the regime)
        const Trial tr = trial_point(tk, s.data(), nu.data(), slo.data(), d, G.data(), pass == 0 ? 0.5 : 1e-13, 0.5, pass != 0, s2.data(), nu2.data(), slo2.data());
        v[0] = tr.small; v[1] = tr.gd; row("trial", v, 2); row("s2", s2.data(), n); row("nu2", nu2.data(), n); row("slo2", slo2.data(), n);
    }
    { std::vector<double> st(s); v[0] = price_collapsed(tk, s.data(), st.data()); st[1] = s[1] + 60.5; v[1] = price_collapsed(tk, s.data(), st.data());
      st[1] = s[1]; st[2] = s[2] + 61.0; v[2] = price_collapsed(tk, s.data(), st.data()); row("collapsed", v, 3); }''' % (mu, value, arb, floor)
    got = {}
    for line in _newton_rules_program(tmp_path, "tokens", body):
        k, *vals = line.split()
        got.setdefault(k, []).append(vals)

    # ---- the same, restated
    listed = [not (ct[j] < ULOG and not pools[j] and h[j] == 0.0) for j in range(n)]
    mask = [ct[j] == FREE or not listed[j] for j in range(n)]
    lob = [math.log(c[j]) if ct[j] == GE and c[j] > 0 else -math.inf for j in range(n)]
    barrier = [ct[j] == GE and not c[j] > 0 and listed[j] for j in range(n)]
    s = [math.log(c[j]) if ct[j] == FREE else max(math.log(nu0[j]), lob[j]) for j in range(n)]
    nu = [math.exp(x) for x in s]
    assert [float(x) for x in got["pass"][0]] == [-1.0, 1.0] and [float(x) for x in got["unbounded"][0]] == [4.0]
    assert [float(x) for x in got["listed"][0]] == [1, 1, 0, 1, 1, 1, 1] == [float(x) for x in listed]
    assert [float(x) for x in got["mask"][0]] == [0, 0, 1, 0, 1, 0, 0] == [float(x) for x in mask]
    assert [float(x) for x in got["barrier"][0]] == [0, 1, 0, 0, 0, 0, 0] == [float(x) for x in barrier]
    _same_numbers(got["lob"][0], lob); _same_numbers(got["s"][0], s); _same_numbers(got["nu"][0], nu)
    assert s[0] == lob[0] and nu[4] == math.exp(math.log(c[4]))

    def table(j, p, q):                  # (P*, conjugate, utility of q, violation, nu^2 ubar'')
        if ct[j] == ULOG:
            return c[j] / p - h[j], c[j] * math.log(c[j] / p) - c[j] + p * h[j], c[j] * math.log(max(q + h[j], 1e-300)), max(-(q + h[j]), 0.0), c[j]
        return h[j] * (c[j] - p), 0.5 * h[j] * (c[j] - p) * (c[j] - p), c[j] * q - 0.5 * q * q / h[j], 0.0, h[j] * p * p
    dual = arb
    for j in range(n):
        dual += table(j, nu[j], 0.0)[1] if ct[j] >= ULOG else (nu[j] - c[j]) * h[j]
    _same_numbers(got["start_dual"][0], [dual])
    g, G, Hd = value, [0.0] * n, [0.0] * n
    for j in range(n):
        if ct[j] >= ULOG:
            pstar, ubar, _, _, d2 = table(j, nu[j], psi[j])
            g += ubar; Gj = nu[j] * (psi[j] - pstar); hj = d2
        else:
            g += (nu[j] - c[j]) * h[j]; Gj = nu[j] * (psi[j] + h[j]); hj = 0.0
        Hd[j] = max(Gj, 0.0) + hj
        if barrier[j]:
            g -= mu * math.log(nu[j]); Gj -= mu
        G[j] = 0.0 if mask[j] else Gj
    _same_numbers(got["g"][0], [g]); _same_numbers(got["g_only"][0], [g]); _same_numbers(got["G"][0], G); _same_numbers(got["Hd"][0], Hd)

    def sums(kinds, q):
        lin = primal = cs = viol = scale = 0.0
        for j in range(n):
            if kinds[j] >= ULOG:
                pstar, ubar, uval, vio, _ = table(j, nu[j], q[j])
                lin += ubar; primal += uval; cs += ubar + nu[j] * q[j] - uval
                viol = max(viol, vio); scale = max(scale, abs(q[j]), abs(pstar))
                continue
            r = q[j] + h[j]
            lin += (nu[j] - c[j]) * h[j]; primal += c[j] * q[j]; cs += (nu[j] - c[j]) * r
            viol = max(viol, max(-r, 0.0) if kinds[j] == GE else (abs(r) if kinds[j] == EQ else 0.0))
            scale = max(scale, abs(q[j]), abs(h[j]))
        return lin, primal, cs, viol, scale, viol / max(scale, floor, 1e-300)
    _same_numbers(got["cert"][0], sums(ct, psi))
    assert float(got["exact_table"][0][0]) == 0.0 and float(got["exact_table_feasible"][0][0]) == 0.0     # (the table entries alone refuse it)
    ct2, px = [GE, GE, GE, EQ, FREE, GE, GE], [-x for x in h]
    for key, q in (("exact_holds", px), ("exact_fails", psi)):
        lin, primal, cs, viol, scale, infeas = sums(ct2, q)
        d0 = lin + arb
        gap0 = abs(cs) / max(1.0, abs(d0))
        _same_numbers(got[key][0], [float(gap0 <= 1e-6 and infeas <= 1e-6), d0, gap0, infeas, primal])
    assert float(got["exact_holds"][0][0]) == 1.0 and float(got["exact_fails"][0][0]) == 0.0
    # pinned: the masked tokens, and token 0 -- on its bound, the gradient pushing it down
    G[0] = 0.25
    pin = [bool(mask[j] or (s[j] <= lob[j] + 1e-13 * max(1.0, abs(lob[j])) and G[j] > 0.0)) for j in range(n)]
    assert pin == [True, False, True, False, True, False, False]
    Gp = [0.0 if pin[j] else G[j] for j in range(n)]
    _same_numbers(got["pin"][0], [float(x) for x in pin]); _same_numbers(got["rhs"][0], [-x for x in Gp]); _same_numbers(got["Hd_shifted"][0], [x + 1e-9 for x in Hd])
    Gt = list(Gp); Gt[0] = 0.25
    slo = [0.0] * n
    for i, (t, final_mu, want_small) in enumerate(((0.5, False, False), (1e-13, True, True), (1e-13, True, False))):
        if i == 2:
            slo[1] = 2e-10
        small = final_mu and t * 0.5 < 1e-11 and max(abs(slo[j] + t * d[j]) for j in range(n)) < 1e-10
        assert small == want_small
        s2, nu2, slo2, gd = [0.0] * n, [0.0] * n, [0.0] * n, 0.0
        for j in range(n):
            if small:
                s2[j], nu2[j], slo2[j] = s[j], nu[j], (0.0 if mask[j] else max(slo[j] + t * d[j], lob[j] - s[j]))
            else:
                s2[j] = max(s[j] + slo[j] + t * d[j], lob[j]); nu2[j] = nu[j] if mask[j] else math.exp(s2[j]); slo2[j] = 0.0
            gd += Gt[j] * ((s2[j] + slo2[j]) - (s[j] + slo[j]))
        _same_numbers(got["trial"][i], [float(small), gd])
        _same_numbers(got["s2"][i], s2); _same_numbers(got["nu2"][i], nu2); _same_numbers(got["slo2"][i], slo2)
        assert (s2[0] + slo2[0]) == lob[0] and nu2[2] == nu[2] and nu2[4] == nu[4]      # (the bound holds token 0; pinned prices stay)
    assert [float(x) for x in got["collapsed"][0]] == [0.0, 1.0, 0.0]                  # (60 e-foldings under the start; a pinned token does not count)


_SWEEP_HELPERS = r'''
#include <cstdint>
inline void rowi(const char *k, const int *v, int n) { printf("%s", k); for (int i = 0; i < n; ++i) printf(" %d", v[i]); printf("\n"); }
// a point's state on one line: done fills_ok status evals iters rounds budget kink_tol | tied: i sgn loose ... | banned: i sgn ... | theta ...
inline void show(const char *k, const PointState &S)
{
    printf("%s %d %d %d %d %d %d %d %.17g |", k, (int)S.done, (int)S.fills_ok, S.st.status, S.evals, S.iters, S.rounds, S.budget, S.kink_tol);
    for (auto &kv : S.tied) printf(" %d %d %d", kv.first, kv.second.sgn, (int)kv.second.loose);
    printf(" |");
    for (auto &b : S.banned) printf(" %d %d", b.first, b.second);
    printf(" |");
    for (double t : S.theta) printf(" %.17g", t);
    printf("\n");
}
'''


def _sweep_rules_program(tmp_path, name, body):
    """a stand-alone HOST program over csrc/sweep_rules.hpp (nothing of HIP in it): compiled -Wall -Werror, run, its output lines"""
    return _rules_program(tmp_path, "sweep_rules.hpp", "sweep", name, body, _SWEEP_HELPERS)


def _keyed(lines):
    out = {}
    for l in lines:
        k, _, rest = l.partition(" ")
        out.setdefault(k, []).append(rest)
    return out


def _cvec(name, v, typ="double"):
    return "const %s %s[] = {%s};" % (typ, name, ", ".join(repr(float(x)) if typ == "double" else str(int(x)) for x in v))


def test_swept_solve_ties_are_the_weighted_union_find_of_the_python_loop(tmp_path):
    """csrc/sweep_rules.hpp: Ties.  A chain 0-1-2 with offsets d01, d12 gives off[0] - off[2] = d01 + d12; tying 0-2 again with that sum
    is accepted, with the sum + 1e-6 refused; groups() numbers the groups in the order of their roots.  Then the same list of ties
    (a refused one among them) through cfmm.problem._Ties: the tie results and group ids equal, the offsets to 1e-15 relative -- both
    add the same doubles in the same order (find compresses from the top of the path down in both)."""
    from cfmm.problem import _Ties
    d01, d12 = 0.25, -0.6
    pairs = [(3, 1, 0.11), (1, 6, -0.07), (0, 7, 0.3), (7, 3, 0.02), (0, 6, 0.5), (4, 5, -0.2), (5, 4, 0.2), (2, 5, 0.013)]
    got = _keyed(_sweep_rules_program(tmp_path, "ties", r'''
    { Ties t; t.init(6);
      const int a = t.tie(0, 1, %r), b = t.tie(1, 2, %r);
      t.find(0); t.find(2);
      const double v[] = {(double)a, (double)b, t.off[0] - t.off[2], (double)t.tie(0, 2, %r + %r), (double)t.tie(0, 2, %r + %r + 1e-6), (double)t.tie(4, 5, 0.1)};
      row("chain", v, 6);
      int grp[6]; const int ng = t.groups(grp); rowi("chain_grp", grp, 6); printf("chain_ng %%d\n", ng); }
    { Ties t; t.init(8);
      const int a[] = {%s}, b[] = {%s}; const double d[] = {%s};
      int ok[%d];
      for (int q = 0; q < %d; ++q) ok[q] = t.tie(a[q], b[q], d[q]);
      rowi("ok", ok, %d);
      int grp[8]; const int ng = t.groups(grp); rowi("grp", grp, 8); printf("ng %%d\n", ng); row("off", t.off, 8); }
    ''' % (d01, d12, d01, d12, d01, d12, ", ".join(str(p[0]) for p in pairs), ", ".join(str(p[1]) for p in pairs),
           ", ".join(repr(p[2]) for p in pairs), len(pairs), len(pairs), len(pairs))))
    assert [float(x) for x in got["chain"][0].split()] == [1.0, 1.0, d01 + d12, 1.0, 0.0, 1.0]
    # roots: tokens 0, 1, 2 hang under 2, token 3 is its own, 4 hangs under 5 -- numbered in the order of the roots 2 < 3 < 5
    assert got["chain_grp"][0].split() == ["0", "0", "0", "1", "2", "2"] and got["chain_ng"] == ["3"]
    t = _Ties(8)
    ok = [int(t.tie(a, b, d)) for a, b, d in pairs]
    grp, off, ng = t.groups()
    assert ok == [1, 1, 1, 1, 0, 1, 1, 1]                       # (0-6 is already fixed at 0.3 + 0.02 + 0.11 - 0.07; 5-4 repeats 4-5)
    assert [int(x) for x in got["ok"][0].split()] == ok
    assert [int(x) for x in got["grp"][0].split()] == list(grp) and int(got["ng"][0]) == ng == 2
    _same_numbers(got["off"][0].split(), list(off))


def test_swept_solve_box_least_squares_against_the_enumerated_faces(tmp_path):
    """csrc/sweep_rules.hpp: box_lsq.  K = 2 with A = I: the solution is b clipped to the box, coordinate by coordinate (inside, one
    coordinate over 1, one under 0 and one over 1).  A coupled 3 x 2 system whose free solution lies outside: the optimum among the nine
    face assignments {free, 0, 1}^2, enumerated here with NumPy, to 1e-9.  K = 8 with the free solution outside: the clipped free
    solution (no enumeration beyond 7 unknowns).  Two equal columns: finite values inside [0, 1]."""
    import itertools
    rng = np.random.default_rng(5)
    cases = [("i0", np.eye(2), [0.3, 0.6]), ("i1", np.eye(2), [1.4, 0.5]), ("i2", np.eye(2), [-0.2, 1.7])]
    A3 = np.array([[1.0, 0.5], [0.2, 1.0], [0.7, -0.3]])
    cases.append(("c3", A3, A3 @ np.array([1.3, 0.4]) + np.array([0.02, -0.01, 0.03])))
    A8 = np.eye(8) + 0.25 * (np.abs(np.subtract.outer(np.arange(8), np.arange(8))) == 1)
    cases.append(("k8", A8, A8 @ np.array([1.5, -0.4, 0.3, 0.6, 0.2, 1.2, 0.5, 0.1]) + 0.01 * rng.standard_normal(8)))
    cases.append(("rd", np.array([[1.0, 1.0], [2.0, 2.0], [0.5, 0.5]]), [0.6, 1.2, 0.3]))
    body = ""
    for nm, A, b in cases:
        A = np.asarray(A, float)
        body += ("    { std::vector<double> A = {%s}, b = {%s}, th; box_lsq(A, b, %d, %d, th); row(\"%s\", th.data(), (int)th.size()); }\n"
                 % (", ".join(repr(float(x)) for x in A.ravel()), ", ".join(repr(float(x)) for x in b), A.shape[0], A.shape[1], nm))
    got = {k: [float(x) for x in v[0].split()] for k, v in _keyed(_sweep_rules_program(tmp_path, "lsq", body)).items()}
    for nm, want in (("i0", (0.3, 0.6)), ("i1", (1.0, 0.5)), ("i2", (0.0, 1.0))):
        assert np.abs(np.array(got[nm]) - want).max() <= 1e-12, (nm, got[nm])       # (the ridge is 1e-14 relative)
    _, A, b = cases[3]
    assert not np.all((np.linalg.lstsq(A, b, rcond=None)[0] >= 0) & (np.linalg.lstsq(A, b, rcond=None)[0] <= 1))
    best = None
    for faces in itertools.product((None, 0.0, 1.0), repeat=2):
        th = np.array([0.0 if f is None else f for f in faces])
        free = [k for k, f in enumerate(faces) if f is None]
        if free:
            th[free] = np.linalg.lstsq(A[:, free], b - A @ th, rcond=None)[0]
            if not np.all((th[free] >= 0) & (th[free] <= 1)):
                continue
        r = float(np.sum((A @ th - b) ** 2))
        if best is None or r < best[0]:
            best = (r, th)
    assert np.abs(np.array(got["c3"]) - best[1]).max() <= 1e-9, (got["c3"], best)
    _, A, b = cases[4]
    free = np.linalg.solve(A, b)
    assert free.max() > 1 and free.min() < 0
    assert np.abs(np.array(got["k8"]) - np.clip(free, 0, 1)).max() <= 1e-9, (got["k8"], free)
    assert len(got["rd"]) == 2 and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in got["rd"]), got["rd"]


# a 3-token point with ONE constant-sum pool (tokens 0 -> 1, fee g, reserves Ra, Rb) tied on its a->b kink: the full fill tenders
# Rb / g of token 0 and drains Rb of token 1.  Tokens 0 and 1 are equalities, token 2 a GE token sitting ON its bound nu = c
_FILL = dict(g=0.997, Ra=7.0, Rb=10.0, nu=[0.997 * 2.0, 2.0, 3.0], c=[0.0, 0.0, 3.0], ctype=[1, 1, 0], surplus=0.7)


def _fill_psi(theta):
    """net trade of the rest of the network that a fill of theta balances exactly on tokens 0 and 1"""
    f = _FILL
    return [theta * f["Rb"] / f["g"], -theta * f["Rb"], f["surplus"]]


_FILL_DECL = (_cvec("ia", [0], "int32_t") + _cvec("ib", [1], "int32_t") + _cvec("fee", [_FILL["g"]]) + _cvec("Ra", [_FILL["Ra"]]) + _cvec("Rb", [_FILL["Rb"]])
              + " const SumCols sc{1, ia, ib, fee, Ra, Rb};" + _cvec("nu", _FILL["nu"]) + _cvec("c", _FILL["c"]) + _cvec("h", [0, 0, 0]) + _cvec("ct", _FILL["ctype"], "int32_t"))


def test_swept_solve_recovers_the_fill_that_balances_the_tied_pool(tmp_path):
    """csrc/sweep_rules.hpp: recover_fills on a 3-token point built by hand (above) so that theta = 0.386 balances the two EQ tokens
    exactly: accepted, theta to 1e-12.  A perturbation of psi orthogonal to the pool's direction (it moves no theta, all of it is
    residual) of 100 x tol x scale is refused, of 1 x tol x scale accepted (the bar is 10 x tol).  The GE token at its bound carries a
    positive surplus throughout and does not count; the same surplus on a GE token OFF its bound must balance, and is refused."""
    f, tol, theta = _FILL, 1e-6, 0.386
    psi = np.array(_fill_psi(theta))
    nu = np.array(f["nu"])
    Acol = np.array([-f["Rb"] / f["g"] * nu[0], f["Rb"] * nu[1]])          # the pool's column on the two tokens that must balance
    v = np.array([Acol[1], -Acol[0]]); v /= np.abs(v).sum()               # orthogonal to it, |v|_1 = 1
    scale = max(1.0, float(np.sum(np.abs(nu * np.abs(psi)))))
    body = "    " + _FILL_DECL + " (void)c;\n    std::map<int, Tie> tied; tied[0] = Tie{1, false}; std::vector<double> th;\n"
    runs = [("exact", psi, f["c"])]
    for nm, mult in (("far", 100.0), ("near", 1.0)):
        p = psi.copy(); p[:2] += mult * tol * scale * v / nu[:2]
        runs.append((nm, p, f["c"]))
    runs.append(("offbound", psi, [0.0, 0.0, 1.0]))
    for nm, p, c in runs:
        body += ("    { %s %s const int ok = recover_fills(3, nu, psi, c2, h, ct, sc, tied, %r, th); const double o[] = {(double)ok, th[0]}; row(\"%s\", o, 2); }\n"
                 % (_cvec("psi", p), _cvec("c2", c), tol, nm))
    got = {k: [float(x) for x in r[0].split()] for k, r in _keyed(_sweep_rules_program(tmp_path, "fills", body)).items()}
    assert got["exact"][0] == 1.0 and abs(got["exact"][1] - theta) <= 1e-12, got["exact"]
    assert got["far"][0] == 0.0 and abs(got["far"][1] - theta) <= 1e-9, got["far"]
    assert got["near"][0] == 1.0, got["near"]
    assert got["offbound"][0] == 0.0, got["offbound"]


def test_swept_solve_finds_the_pools_that_sit_on_a_kink(tmp_path):
    """csrc/sweep_rules.hpp: kink_candidates, one pool over tokens (0, 1), log-price ratio r, lg = log fee, tolerance 1e-3.
    r = lg + 0.5e-3: found, sgn +1 (the a->b kink); r = -lg - 0.5e-3: found, sgn -1.  A banned (pool, sgn) and an already tied pool are
    skipped.  A fee band narrower than twice the distance (|lg| < 2 dist) is ambiguous: found only by a loose search, and marked loose.
    lg = 0 (no fee: the two kinks coincide): found."""
    import math
    lg = math.log(0.99)
    cases = [("plus", 0.99, lg + 0.5e-3, "", "", 0), ("minus", 0.99, -lg - 0.5e-3, "", "", 0),
             ("banned", 0.99, lg + 0.5e-3, "banned.insert({0, 1});", "", 0), ("othersign", 0.99, lg + 0.5e-3, "banned.insert({0, -1});", "", 0),
             ("tied", 0.99, lg + 0.5e-3, "", "tied[0] = Tie{1, false};", 0),
             ("narrow", math.exp(-0.8e-3), -0.8e-3 + 0.5e-3, "", "", 0), ("narrow_loose", math.exp(-0.8e-3), -0.8e-3 + 0.5e-3, "", "", 1),
             ("nofee", 1.0, -0.5e-3, "", "", 0), ("far", 0.99, lg + 1.5e-3, "", "", 1)]
    body = "    const int32_t ia[] = {0}, ib[] = {1}; const double Ra[] = {1.0}, Rb[] = {1.0};\n"
    for nm, fee, r, ban, tie, loose in cases:
        body += ("    { const double fee[] = {%r}, nu[] = {std::exp(%r), 1.0}; const SumCols sc{1, ia, ib, fee, Ra, Rb};\n"
                 "      std::set<std::pair<int, int>> banned; std::map<int, Tie> tied, out; out[5] = Tie{1, true}; %s %s\n"
                 "      kink_candidates(nu, sc, 1e-3, banned, tied, %d, out);\n"
                 "      printf(\"%s %%d\", (int)out.size()); for (auto &kv : out) printf(\" %%d %%d %%d\", kv.first, kv.second.sgn, (int)kv.second.loose); printf(\"\\n\"); }\n"
                 % (fee, r, ban, tie, loose, nm))
    got = {k: [int(x) for x in v[0].split()] for k, v in _keyed(_sweep_rules_program(tmp_path, "kinks", body)).items()}
    assert got == {"plus": [1, 0, 1, 0], "minus": [1, 0, -1, 0], "banned": [0], "othersign": [1, 0, 1, 0], "tied": [0], "narrow": [0],
                   "narrow_loose": [1, 0, 1, 1], "nofee": [1, 0, 1, 0], "far": [0]}, got


def test_swept_solve_round_tail_takes_each_branch_of_the_active_set_loop(tmp_path):
    """csrc/sweep_rules.hpp: round_tail, one case per branch, in the order the loop tries them (the point of the fills test above, and a
    second pool over tokens (1, 2) with fee 0.99; tolerance 1e-6, max_evals 300; every leg reports 7 evaluations and 5 iterations):
    a non-finite dual value ends the point with the numeric status; status 1 without ties ends it; status 1 with a fill inside (0, 1) ends
    it with fills_ok and the fill; a fill at 1 (the balance asks for 1.7) is released and banned, the point goes on; a LOOSE tie with
    fill 0 is re-tied on the pool's other kink, no longer loose -- unless that sign is banned too; a new candidate joins the ties and
    clears the bans that do not concern it; status 3 with no candidate within 0.1 doubles a leg budget below max_evals (capped at it);
    with the budget at max_evals the kink tolerance goes up tenfold; at 0.05 the point is given up."""
    import math
    f = _FILL
    lg0 = math.log(f["g"])
    far = [1.0, 2.0, 4.0]                                     # log-price ratios -0.69: no kink within the widest search (0.1)
    on0 = [math.exp(lg0 + 0.5e-3) * 2.0, 2.0, 2.0]            # pool 0 on its a->b kink; pool 1 at ratio 0, 0.01 from either of its kinks
    decl = ("    " + _cvec("ia", [0, 1], "int32_t") + _cvec("ib", [1, 2], "int32_t") + _cvec("fee", [f["g"], 0.99]) + _cvec("Ra", [f["Ra"], 5.0])
            + _cvec("Rb", [f["Rb"], 5.0]) + " const SumCols sc{2, ia, ib, fee, Ra, Rb};" + _cvec("c", f["c"]) + _cvec("h", [0, 0, 0]) + _cvec("ct", f["ctype"], "int32_t")
            + "\n    const double INF = INFINITY; (void)INF;\n")
    cases = [   # name, leg status, dual value, prices, psi, set-up of the state
        ("nonfinite", 1, "INF", f["nu"], _fill_psi(0.3), ""),
        ("plain", 1, "-3.5", f["nu"], _fill_psi(0.3), ""),
        ("filled", 1, "-3.5", f["nu"], _fill_psi(0.386), "S.tied[0] = Tie{1, false};"),
        ("full", 1, "-3.5", f["nu"], _fill_psi(1.7), "S.tied[0] = Tie{1, false};"),
        ("flip", 1, "-3.5", f["nu"], _fill_psi(-0.5), "S.tied[0] = Tie{1, true};"),
        ("noflip", 1, "-3.5", f["nu"], _fill_psi(-0.5), "S.tied[0] = Tie{1, true}; S.banned.insert({0, -1});"),
        ("fresh", 3, "-3.5", on0, _fill_psi(0.3), "S.banned.insert({0, -1}); S.banned.insert({1, 1});"),
        ("longer", 3, "-3.5", far, _fill_psi(0.3), "S.budget = 40;"),
        ("capped", 0, "-3.5", far, _fill_psi(0.3), "S.budget = 200;"),
        ("wider", 3, "-3.5", far, _fill_psi(0.3), "S.budget = 300;"),
        ("wider2", 2, "-3.5", far, _fill_psi(0.3), "S.budget = 40;"),
        ("giveup", 3, "-3.5", far, _fill_psi(0.3), "S.budget = 300; S.kink_tol = 0.05;"),
    ]
    body = decl
    for nm, status, fval, nu, psi, setup in cases:
        body += ("    { PointState S; S.budget = 40; S.evals = 10; S.iters = 8; S.rounds = 2; %s\n"
                 "      %s %s const LegResult leg = {%d, 7, 5, %s, 1.0, 2e-7, 3e-7, 4e-7};\n"
                 "      round_tail(S, leg, 3, nu, psi, c, h, ct, sc, 1e-6, 300); show(\"%s\", S); }\n" % (setup, _cvec("nu", nu), _cvec("psi", psi), status, fval, nm))
    got = {}
    for k, v in _keyed(_sweep_rules_program(tmp_path, "tail", body)).items():
        head, tied, banned, theta = [p.split() for p in v[0].split("|")]
        got[k] = dict(done=int(head[0]), fills_ok=int(head[1]), status=int(head[2]), counts=[int(x) for x in head[3:6]], budget=int(head[6]), kink_tol=float(head[7]),
                      tied=[int(x) for x in tied], banned=[int(x) for x in banned], theta=[float(x) for x in theta])
    assert len(got) == len(cases)
    for k, g in got.items():
        assert g["counts"] == [17, 13, 3], (k, g)              # (the leg's evaluations and iterations are added, the round counted)
    E_NUMERIC = int(re.search(r"CFMM_E_NUMERIC\s*=\s*(-?\d+)", open(os.path.join(ROOT, "include", "cfmm.h")).read()).group(1))

    def check(k, **want):
        base = dict(done=0, fills_ok=0, budget=40, kink_tol=1e-3, tied=[], banned=[], theta=[])
        base.update(want)
        for key, w in base.items():
            assert got[k][key] == w, (k, key, got[k], w)
    check("nonfinite", done=1, status=E_NUMERIC)
    check("plain", done=1, status=1)
    check("filled", done=1, fills_ok=1, status=1, tied=[0, 1, 0], theta=got["filled"]["theta"])
    assert len(got["filled"]["theta"]) == 1 and abs(got["filled"]["theta"][0] - 0.386) <= 1e-12
    check("full", status=1, banned=[0, 1])
    check("flip", status=1, tied=[0, -1, 0], banned=[0, 1])
    check("noflip", status=1, banned=[0, -1, 0, 1])
    check("fresh", status=3, tied=[0, 1, 0], banned=[0, -1])
    check("longer", status=3, budget=80)
    check("capped", status=0, budget=300)
    check("wider", status=3, budget=300, kink_tol=1e-3 * 10.0)
    check("wider2", status=2, kink_tol=1e-3 * 10.0)
    check("giveup", done=1, status=3, budget=300, kink_tol=0.05)


def test_swept_solve_round_head_bounds_and_schedule(tmp_path):
    """csrc/sweep_rules.hpp: round_head, group_bounds, first_budget, exhausted.
    round_head: two records over the same token pair with different fees contradict -- the first stays tied and flagged, the second is
    dropped and banned; the tied pair is one group numbered before token 2, token 0 carries the offset log fee; the tolerance factor is
    0.01 and pg_rule 1; the group's lower bound is the larger of the members' (log c - off), and the slot past ng is unbounded.  An
    untied point: identity groups, zero offsets, the full tolerance, pg_rule 0.
    group_bounds, one token each of GE with c > 0, GE with c = 0, EQ, FREE and a CFMM_ULOG entry: [log c, inf), [mid - 100, inf),
    mid +- 100, log c twice, unbounded -- with mid = log of the largest c over the NON-table tokens.  Two tokens of one group with
    offsets: the intersection.  A FREE token with c = 0: its index.
    The schedule: legs of 40 evaluations up to 1000 pools and 100 beyond, never more than max_evals, and one leg of max_evals without
    constant-sum pools; a point is exhausted at 4 x max_evals."""
    import math
    inf = float("inf")
    ULOG = int(re.search(r"CFMM_ULOG\s*=\s*(-?\d+)", open(os.path.join(ROOT, "include", "cfmm.h")).read()).group(1))
    f0, f1 = 0.997, 0.99
    got = _keyed(_sweep_rules_program(tmp_path, "head", r'''
    { const int32_t ia[] = {0, 0}, ib[] = {1, 1}; const double fee[] = {%r, %r}, Ra[] = {1.0, 1.0}, Rb[] = {1.0, 1.0}; const SumCols sc{2, ia, ib, fee, Ra, Rb};
      const double c[] = {1.5, 10.0, 2.0}; const int ct[] = {0, 0, 0};
      int flags[2] = {7, 7}, grp[3]; double off[3], glo[3], ghi[3];
      PointState S; S.tied[0] = Tie{1, false}; S.tied[1] = Tie{1, false};
      const RoundHead r = round_head(S, sc, 3, c, ct, flags, grp, off, glo, ghi);
      show("h1", S); rowi("h1_flags", flags, 2); rowi("h1_grp", grp, 3); row("h1_off", off, 3); row("h1_lo", glo, 3); row("h1_hi", ghi, 3);
      printf("h1_r %%d %%d %%.17g %%d\n", r.ng, (int)r.tied, r.tol_factor, r.pg_rule);
      PointState U; int fl2[2] = {7, 7};
      const RoundHead u = round_head(U, sc, 3, c, ct, fl2, grp, off, glo, ghi);
      rowi("h2_flags", fl2, 2); rowi("h2_grp", grp, 3); row("h2_off", off, 3); row("h2_lo", glo, 3); row("h2_hi", ghi, 3);
      printf("h2_r %%d %%d %%.17g %%d\n", u.ng, (int)u.tied, u.tol_factor, u.pg_rule); }
    { const double c[] = {2.0, 0.0, 5.0, 3.0, 1000.0}; const int ct[] = {CFMM_GE, CFMM_GE, CFMM_EQ, CFMM_FREE, CFMM_ULOG}, grp[] = {0, 1, 2, 3, 4};
      const double off[5] = {}; double lo[5], hi[5];
      printf("b1_rc %%d\n", group_bounds(5, c, ct, grp, off, 5, lo, hi)); row("b1_lo", lo, 5); row("b1_hi", hi, 5); }
    { const double c[] = {2.0, 4.0, 0.0}; const int ct[] = {CFMM_GE, CFMM_EQ, CFMM_FREE}, grp[] = {0, 0, 1};
      const double off[] = {0.1, -0.2, 0.0}; double lo[2], hi[2];
      printf("b2_rc %%d\n", group_bounds(2, c, ct, grp, off, 1, lo, hi)); row("b2_lo", lo, 1); row("b2_hi", hi, 1);
      printf("b3_rc %%d\n", group_bounds(3, c, ct, grp, off, 2, lo, hi)); }
    printf("budget %%d %%d %%d %%d %%d\n", first_budget(0, 5, 300), first_budget(1, 5, 300), first_budget(3, 1000, 300), first_budget(3, 1001, 300), first_budget(1, 5, 30));
    { PointState S; S.evals = 1199; const int a = exhausted(S, 300); S.evals = 1200; printf("exhausted %%d %%d\n", a, (int)exhausted(S, 300)); }
    ''' % (f0, f1)))
    one = lambda k: got[k][0].split()
    head, tied, banned, theta = [p.split() for p in got["h1"][0].split("|")]
    assert tied == ["0", "1", "0"] and banned == ["1", "1"] and theta == []
    assert one("h1_flags") == ["1", "0"] and one("h1_grp") == ["0", "0", "1"]
    _same_numbers(one("h1_off"), [math.log(f0), 0.0, 0.0])
    _same_numbers(one("h1_lo"), [max(math.log(1.5) - math.log(f0), math.log(10.0)), math.log(2.0), -inf])
    assert [float(x) for x in one("h1_hi")] == [inf, inf, inf]
    assert [float(x) for x in one("h1_r")] == [2.0, 1.0, 0.01, 1.0]
    assert one("h2_flags") == ["0", "0"] and one("h2_grp") == ["0", "1", "2"] and [float(x) for x in one("h2_off")] == [0.0, 0.0, 0.0]
    _same_numbers(one("h2_lo"), [math.log(1.5), math.log(10.0), math.log(2.0)])
    assert [float(x) for x in one("h2_hi")] == [inf, inf, inf]
    assert one("h2_r") == ["3", "0", "1", "0"]
    mid = math.log(5.0)                                       # (the table entry's c = 1000 does not count)
    assert ULOG >= 3 and one("b1_rc") == ["-1"]
    _same_numbers(one("b1_lo"), [math.log(2.0), mid - 100.0, mid - 100.0, math.log(3.0), -inf])
    _same_numbers(one("b1_hi"), [inf, inf, mid + 100.0, math.log(3.0), inf])
    assert one("b2_rc") == ["-1"]
    _same_numbers(one("b2_lo"), [max(math.log(2.0) - 0.1, math.log(4.0) - 100.0 + 0.2)])
    _same_numbers(one("b2_hi"), [math.log(4.0) + 100.0 + 0.2])
    assert one("b3_rc") == ["2"]
    assert one("budget") == ["300", "40", "40", "100", "30"] and one("exhausted") == ["0", "1"]


def test_swept_solve_folds_the_arbitrage_fill_and_certifies_the_point(tmp_path):
    """csrc/sweep_rules.hpp: fold_fills and point_certificates on the shipped arbitrage instance, numbers from the 50-digit KKT record of
    tests/golden: pool 4 (constant-sum, tokens 2 and 3) is partially filled -- theta and the sign read from its y.  psi of the four other
    pools + the folded fill reproduces the record's psi to 5e-8 (the bound of the GPU test), the pool's tenders its y; value and dual
    agree with the record's value to 1e-9.  Gap and infeasibility: the record satisfies the KKT system to 1e-49, folding in doubles adds
    a few ulp of trades of size ~5, so both must come out under 1e-12."""
    inst, k = I.normalise(I.arbitrage()), golden()["arbitrage"]["kkt"]
    n, idx, R, fee = inst["n_tokens"], inst["local_indices"][4], inst["reserves"][4], inst["fees"][4]
    assert inst["kinds"][4] == "sum" and list(k["theta"]) == ["4"]
    y4 = k["y"][4]
    sgn = 1 if y4[0] < 0 else -1                              # sgn +1 tenders the pool's first token
    theta = float(y4[1] / R[1] if sgn > 0 else y4[0] / R[0])
    assert abs(theta - k["theta"]["4"]) <= 1e-12 and 0.0 < theta < 1.0
    psi = np.zeros(n)
    for p in range(4):
        psi[np.asarray(inst["local_indices"][p])] += np.asarray(k["y"][p])
    got = _keyed(_sweep_rules_program(tmp_path, "fold", "    " + _cvec("ia", [idx[0], 0], "int32_t") + _cvec("ib", [idx[1], 1], "int32_t") + _cvec("fee", [fee, 0.99])
                                      + _cvec("Ra", [R[0], 1.0]) + _cvec("Rb", [R[1], 1.0]) + " const SumCols sc{2, ia, ib, fee, Ra, Rb};\n    "
                                      + _cvec("nu", k["nu"]) + _cvec("c", inst["c"]) + _cvec("h", inst["h"]) + _cvec("ct", inst["ctype"], "int32_t") + r'''
    double psi[] = {%s}, tr[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    const double theta[] = {%r, NAN}; const int32_t tsgn[] = {%d, 0};
    fold_fills(sc, theta, tsgn, psi, tr, tr + 4);
    row("psi", psi, %d); row("tr", tr, 8);
    const PointCertificates k = point_certificates(%d, nu, psi, c, h, ct, 50.0);
    const double v[] = {k.value, k.dual, k.gap, k.infeas}; row("cert", v, 4);''' % (", ".join(repr(float(x)) for x in psi), theta, sgn, n, n)))
    gpsi = np.array([float(x) for x in got["psi"][0].split()])
    assert np.abs(gpsi - np.asarray(k["psi"])).max() <= 5e-8
    tr = [float(x) for x in got["tr"][0].split()]
    assert tr[1] == tr[3] == tr[5] == tr[7] == 9.0           # (the untied second pool's tenders are left alone)
    delta, lam = np.array([tr[0], tr[2]]), np.array([tr[4], tr[6]])
    assert np.abs((lam - delta) - np.asarray(y4)).max() <= 5e-8 and min(delta.min(), lam.min()) >= 0.0 and float(delta @ lam) == 0.0
    value, dual, gap, infeas = [float(x) for x in got["cert"][0].split()]
    assert abs(value - k["value"]) <= 1e-9 and abs(dual - k["value"]) <= 1e-9
    assert 0.0 <= gap <= 1e-12 and 0.0 <= infeas <= 1e-12, (gap, infeas)


# ---------------------------------------------------------------------------------------------------------------
# csrc/route_rules.hpp: the bucket order and its slots, the layouts of host-held tenders, the folds of the apply's and the audit's
# records, the audited psi from its limbs and its worth under a utility
# ---------------------------------------------------------------------------------------------------------------
_ROUTE_HELPERS = r'''
#include <cstdint>
#include <cstring>
inline void rowi(const char *k, const long long *v, int n) { printf("%s", k); for (int i = 0; i < n; ++i) printf(" %lld", v[i]); printf("\n"); }
inline unsigned long long bits(double x) { unsigned long long b; std::memcpy(&b, &x, sizeof b); return b; }
// pools per slot of the tests' store: two-asset kinds 3 0 5 0 2, geo-mean sizes 3: 4, 5: 1, the table's stableswap 3: 7, constant sum 3: 6, 5: 2
inline Counts some_counts()
{
    Counts c = {};
    c.m[slot2(0)] = 3; c.m[slot2(2)] = 5; c.m[slot2(4)] = 2; c.m[slotN(3)] = 4; c.m[slotN(5)] = 1;
    c.m[slotG(CFMM_POOLK_STABLE, 3)] = 7; c.m[slotG(CFMM_POOLK_SUM, 3)] = 6; c.m[slotG(CFMM_POOLK_SUM, 5)] = 2;
    return c;
}
'''
_KINDS2, _KS, _POOLK = _lib.POOL_POW2 + 1, _lib.MAX_POOL_SIZE + 1, dict(stable=0, sum=1)
_slot2 = lambda kind: kind
_slotN = lambda k: _KINDS2 + k
_slotG = lambda kind, k: _KINDS2 + _KS * (1 + kind) + k


def _route_rules_program(tmp_path, name, body):
    """a stand-alone HOST program over csrc/route_rules.hpp (nothing of HIP in it): compiled -Wall -Werror, run, its output lines"""
    return _rules_program(tmp_path, "route_rules.hpp", "route", name, body, _ROUTE_HELPERS)


def _ints(line):
    return [int(x) for x in line.split()]


def test_route_slots_round_trip_and_ascend_in_the_documented_bucket_order(tmp_path):
    """csrc/route_rules.hpp: slot2 / slotN / slotG, slot_name, each_slot.  The documented bucket order (include/cfmm.h: cfmm_apply_info) --
    two-asset kinds 0.., geo-mean sizes 3..8, the table's kinds each by size 2..8 -- written out here: slot_name inverts the slot of every
    bucket with the family / kind / k the header documents, no slot is hit twice, the slots ascend along that order and stay below SLOTS,
    and each_slot enumerates exactly that order.  No slot: -1 each."""
    assert (_KINDS2, _KS, _lib.POOLK) == (5, 9, _POOLK)
    order = [(0, kind, 2) for kind in range(_KINDS2)] + [(1, 0, k) for k in range(3, _KS)] + [(2, kind, k) for kind in range(2) for k in range(2, _KS)]
    got = _keyed(_route_rules_program(tmp_path, "slots", r'''
    for (int kind = 0; kind < CFMM_POOL_KINDS2; ++kind) { const SlotName s = slot_name(slot2(kind)); printf("slot %d %d %d %d\n", slot2(kind), s.family, s.kind, s.k); }
    for (int k = 3; k <= CFMM_MAX_POOL_SIZE; ++k) { const SlotName s = slot_name(slotN(k)); printf("slot %d %d %d %d\n", slotN(k), s.family, s.kind, s.k); }
    for (int kind = 0; kind < CFMM_POOLK_KINDS; ++kind) for (int k = 2; k <= CFMM_MAX_POOL_SIZE; ++k) { const SlotName s = slot_name(slotG(kind, k)); printf("slot %d %d %d %d\n", slotG(kind, k), s.family, s.kind, s.k); }
    each_slot([](int q, int family, int kind, int k) { printf("each %d %d %d %d\n", q, family, kind, k); });
    const SlotName none = slot_name(-1);
    printf("none %d %d %d\nslots %d\n", none.family, none.kind, none.k, SLOTS);'''))
    rows = [_ints(l) for l in got["slot"]]
    assert [tuple(r[1:]) for r in rows] == order                         # the round trip, in the order written out above
    slots = [r[0] for r in rows]
    assert slots == sorted(set(slots)) and 0 <= slots[0] and slots[-1] < int(got["slots"][0])      # distinct, ascending, in range
    assert slots == [_slot2(k) for k in range(_KINDS2)] + [_slotN(k) for k in range(3, _KS)] + [_slotG(kind, k) for kind in range(2) for k in range(2, _KS)]
    assert [_ints(l) for l in got["each"]] == rows
    assert _ints(got["none"][0]) == [-1, -1, -1]


def test_route_layouts_of_swept_tenders_and_of_the_audits_staged_tenders(tmp_path):
    """csrc/route_rules.hpp: trade_layout, audit_stage, audit_span, fixed_exponent, point_view on hand-set counts with empty buckets in the middle
    (_ROUTE_HELPERS: some_counts).  The sums are written out here.  The staging layout: without and with the kink loop's block, the caller's
    two-asset block, two k-asset blocks, all three; each way of naming one array of a bucket without the other gives that bucket's slot
    (the first in the order two-asset, then k ascending); arrays named for an empty bucket are ignored."""
    got = _keyed(_route_rules_program(tmp_path, "layouts", r'''
    const Counts c = some_counts();
    const TradeLayout t = trade_layout(c);
    { long long v[CFMM_POOL_KINDS2]; for (int k = 0; k < CFMM_POOL_KINDS2; ++k) v[k] = (long long)t.off2[k]; rowi("off2", v, CFMM_POOL_KINDS2); }
    { long long v[KS] = {}; for (int k = 3; k < KS; ++k) v[k] = (long long)t.offn[k]; rowi("offn", v, KS); }
    printf("stride %zu %zu\n", t.stride, t.two_asset());
    const double x = 0.0, *p = &x;
    auto show = [&](const char *key, const Counts &cc, bool kink, const cfmm_audit_tenders *own) {
        const AuditStage s = audit_stage(cc, kink, own);
        printf("%s %zu %d %d %zu |", key, s.len, s.half, (int)s.own2, s.off_own2);
        for (int k = 2; k < KS; ++k) printf(" %d:%zu", (int)s.ownk[k], s.off_ownk[k]);
        printf("\n");
    };
    cfmm_audit_tenders own = {};
    show("none", c, false, nullptr); show("kink", c, true, nullptr); show("blank", c, true, &own);
    own.sum2_delta = own.sum2_lambda = p;                               show("own2", c, true, &own);
    own.sumk_delta[3] = own.sumk_lambda[3] = p;                         show("all", c, true, &own);
    own.sumk_delta[4] = p;                                              show("empty4", c, true, &own);      // (no 4-asset bucket: ignored)
    own.sum2_delta = own.sum2_lambda = nullptr; own.sumk_delta[5] = own.sumk_lambda[5] = p; show("ownk", c, false, &own);
    own.sumk_lambda[5] = nullptr;                                       show("half5d", c, false, &own);
    own.sumk_lambda[5] = p; own.sumk_delta[3] = nullptr;                show("half3l", c, false, &own);
    own.sum2_delta = p;                                                 show("half2d", c, true, &own);      // (the two-asset bucket is met first)
    own.sum2_delta = nullptr; own.sum2_lambda = p;                      show("half2l", c, true, &own);
    Counts e = c; e.m[slot2(CFMM_POOL_SUM2)] = 0;                       show("empty2", e, false, &own);      // (no constant-sum pairs: ignored, bucket 3 is half)
    const AuditSpan sp = audit_span(10, 2048);
    printf("span %zu %zu %zu %zu %zu\n", sp.recs, sp.limbs, sp.parts, sp.total, sizeof(cfmm::AuditRec));
    printf("exp %d %d %d\n", fixed_exponent(0x1p71), fixed_exponent(0x1p-3), fixed_exponent(1.0));
    for (double mu : {0.0, 1e-6, -1.0}) for (int slo = 0; slo < 2; ++slo) { const PointView v = point_view(mu, slo != 0); printf("view %.17g %d\n", v.mu, (int)v.use_slo); }'''))
    # which point the tenders are of: the barrier weight only while positive, the low-order log-prices only with it
    assert [(float(l.split()[0]), int(l.split()[1])) for l in got["view"]] == [(0.0, 0), (0.0, 0), (1e-6, 0), (1e-6, 1), (0.0, 0), (0.0, 0)]
    # two-asset kinds 3 0 5 0 2 pools of 4 doubles; geo-mean 3: 4 pools of 6, 5: 1 pool of 10
    assert _ints(got["off2"][0]) == [0, 12, 12, 32, 32]
    assert _ints(got["offn"][0])[3:] == [40, 64, 64, 74, 74, 74]
    assert got["stride"] == ["74 40"]
    two, s2, s3, s5 = 40, 4 * 5, 2 * 3 * 6, 2 * 5 * 2
    no = " ".join(["0:0"] * 7)
    ks = lambda d: " ".join("1:%d" % d[k] if k in d else "0:0" for k in range(2, _KS))
    assert got["none"] == ["0 -1 0 0 | " + no] and got["kink"] == ["%d -1 0 0 | %s" % (two, no)] and got["blank"] == got["kink"]
    assert got["own2"] == ["%d -1 1 %d | %s" % (two + s2, two, no)]
    assert got["all"] == ["%d -1 1 %d | %s" % (two + s2 + s3, two, ks({3: two + s2}))] and got["empty4"] == got["all"]
    assert got["ownk"] == ["%d -1 0 0 | %s" % (s3 + s5, ks({3: 0, 5: s3}))]
    assert _ints(got["half5d"][0].split("|")[0])[1] == _slotG(_POOLK["sum"], 5)
    assert _ints(got["half3l"][0].split("|")[0])[1] == _slotG(_POOLK["sum"], 3)
    assert _ints(got["half2d"][0].split("|")[0])[1] == _slot2(_lib.POOL_SUM2) and _ints(got["half2l"][0].split("|")[0])[1] == _slot2(_lib.POOL_SUM2)
    assert _ints(got["empty2"][0].split("|")[0])[1] == _slotG(_POOLK["sum"], 3)
    # one 64-byte record per slot | 3 n limbs, rounded up to 256 bytes | 2048 partial records per slot
    slots = _KINDS2 + 3 * _KS
    parts = -(-(slots * 64 + 3 * 10 * 8) // 256) * 256
    assert got["span"] == ["0 %d %d %d 64" % (slots * 64, parts, parts + slots * 2048 * 64)]
    assert got["exp"] == ["71 -3 0"]


def test_route_fold_of_the_apply_records(tmp_path):
    """csrc/route_rules.hpp: fold_apply.  Refusals in a later slot (the table's 3-asset constant-sum bucket) and an earlier one (the
    3-asset geo-mean bucket): the earlier one is named, with ITS position; the totals add over the resident buckets; each largest reserve
    is the double whose bit pattern the record holds (one ulp under 2048 survives); empty slots holding stale records -- a refusal in
    front of every other, a larger maximum -- are ignored.  Without a refusal: -1 / -1."""
    got = _keyed(_route_rules_program(tmp_path, "fold_apply", r'''
    const Counts c = some_counts();
    cfmm::ApplyRec r[SLOTS];
    for (auto &q : r) q = cfmm::ApplyRec{0ull, 0ull, ~0ull, 0ull};
    r[slot2(0)] = {3, 0, ~0ull, bits(2.0)};
    r[slot2(1)] = {100, 5, 0, bits(1e308)};                                 // (stale: no pool of kind 1)
    r[slot2(2)] = {4, 0, ~0ull, bits(0x1.fffffffffffffp+10)};
    r[slotN(3)] = {4, 2, 11, bits(1e300)};
    r[slotN(4)] = {9, 9, 1, bits(1e301)};                                   // (stale)
    r[slotG(CFMM_POOLK_SUM, 3)] = {1, 1, 7, bits(3.0)};
    auto show = [&](const char *key) {
        const ApplyFold f = fold_apply(r, c);
        printf("%s %lld %lld %d %lld\n", key, (long long)f.moved, (long long)f.refused, f.first, (long long)f.first_pos);
        const double v[] = {f.mx[slot2(0)], f.mx[slot2(1)], f.mx[slot2(2)], f.mx[slotN(3)], f.mx[slotN(4)], f.mx[slotG(CFMM_POOLK_SUM, 3)], f.mx_all};
        row(key, v, 7);
    };
    show("two");
    r[slotN(3)].refused = 0; r[slotN(3)].first = ~0ull; show("later");
    r[slotG(CFMM_POOLK_SUM, 3)].refused = 0; show("clean");'''))
    top = float.fromhex("0x1.fffffffffffffp+10")
    assert got["two"][0] == "12 3 %d 11" % _slotN(3) and [float(x) for x in got["two"][1].split()] == [2.0, 0.0, top, 1e300, 0.0, 3.0, 1e300]
    assert got["later"][0] == "12 1 %d 7" % _slotG(_POOLK["sum"], 3)
    assert got["clean"][0] == "12 0 -1 -1"


def test_route_fold_of_the_audit_records_and_the_order_preserving_images(tmp_path):
    """csrc/route_rules.hpp: fold_audit, audit_ord / audit_unord.  The same smallest slack in two buckets names the first in bucket
    order; a strictly smaller one in a later bucket wins; a stale record in an empty slot does not count; the counts add and the
    minima come back as doubles.  An empty network: -1 / -1 / -1 / -1 and +inf three times.  audit_unord(audit_ord(x)) is x bit for bit
    for +-0, denormals, +-inf and ordinary values, NaN counts as -inf, and the images ascend with the doubles."""
    import struct
    xs = [float("-inf"), -2.25, -5e-324, -0.0, 0.0, 5e-324, 2.2250738585072014e-308 / 4, 1.5, float("inf")]
    got = _keyed(_route_rules_program(tmp_path, "fold_audit", r'''
    using cfmm::audit_ord; using cfmm::audit_unord;
    const Counts c = some_counts();
    cfmm::AuditRec r[SLOTS];
    for (auto &q : r) q = cfmm::AuditRec{0ull, 0ull, 0ull, ~0ull, ~0ull, ~0ull, ~0ull, 0ull};
    r[slot2(0)] = {2, 1, 0, audit_ord(-0.5), 3, audit_ord(0.0), audit_ord(0.25), 1};
    r[slot2(1)] = {50, 50, 50, audit_ord(-100.0), 0, audit_ord(-7.0), audit_ord(-7.0), 1};      // (stale: no pool of kind 1)
    r[slot2(2)] = {5, 0, 1, audit_ord(0.0), 0, audit_ord(1.0), audit_ord(0.0), 1};
    r[slot2(4)] = {0, 0, 0, audit_ord(1e-3), 1, audit_ord(2.0), audit_ord(0.5), 1};
    r[slotN(3)] = {4, 1, 0, audit_ord(-0.5), 1, audit_ord(-1e-9), audit_ord(0.5), 1};
    r[slotN(5)] = {1, 0, 0, audit_ord(0.125), 0, audit_ord(0.0), audit_ord(0.75), 1};
    r[slotG(CFMM_POOLK_STABLE, 3)] = {7, 0, 2, audit_ord(1e-12), 6, audit_ord(0.0), audit_ord(0.9), 1};
    r[slotG(CFMM_POOLK_SUM, 3)] = {3, 0, 0, audit_ord(-0.25), 5, audit_ord(0.0), audit_ord(0.125), 1};
    r[slotG(CFMM_POOLK_SUM, 5)] = {2, 0, 0, audit_ord(0.0), 0, audit_ord(0.0), audit_ord(1.0), 1};
    auto show = [&](const char *key, const Counts &cc) {
        const AuditFold f = fold_audit(r, cc);
        const SlotName s = slot_name(f.worst);
        printf("%s %lld %lld %lld %lld %d %d %d %d %lld\n", key, (long long)f.pools, (long long)f.trading, (long long)f.violating, (long long)f.oor, f.worst, s.family, s.kind, s.k, (long long)f.worst_pos);
        const double v[] = {f.min_slack, f.min_tender, f.min_leg}; row(key, v, 3);
    };
    show("tie", c);
    r[slotG(CFMM_POOLK_SUM, 3)].slack = audit_ord(-0.75); show("later", c);
    r[slotG(CFMM_POOLK_SUM, 3)].slack = audit_ord(NAN); show("nan", c);
    const Counts none = {}; show("empty", none);
    const double xs[] = {@XS@, NAN};
    for (double x : xs) printf("ord %llu %llu %llu\n", bits(x), audit_ord(x), bits(audit_unord(audit_ord(x))));'''.replace("@XS@", ", ".join(
        "-INFINITY" if x == float("-inf") else "INFINITY" if x == float("inf") else x.hex() for x in xs))))
    head = "30 24 2 3"                                                  # pools 3 + 5 + 2 + 4 + 1 + 7 + 6 + 2; trading, violating, out of range added up
    assert got["tie"][0] == "%s %d 0 0 2 3" % (head, _slot2(0)) and [float(x) for x in got["tie"][1].split()] == [-0.5, -1e-9, 0.0]
    assert got["later"][0] == "%s %d 2 %d 3 5" % (head, _slotG(_POOLK["sum"], 3), _POOLK["sum"]) and float(got["later"][1].split()[0]) == -0.75
    assert got["nan"][0] == got["later"][0] and float(got["nan"][1].split()[0]) == float("-inf")      # (what cannot be computed is the worst)
    assert got["empty"][0] == "0 0 0 0 -1 -1 -1 -1 -1" and [float(x) for x in got["empty"][1].split()] == [float("inf")] * 3
    rows = [_ints(l) for l in got["ord"]]
    as_bits = lambda x: struct.unpack("<Q", struct.pack("<d", x))[0]
    assert [r[0] for r in rows[:-1]] == [as_bits(x) for x in xs]
    assert all(r[2] == r[0] for r in rows[:-1])                          # the round trip, bit for bit (-0 stays -0)
    assert rows[-1][2] == as_bits(float("-inf")) and rows[-1][1] == rows[0][1]
    assert [r[1] for r in rows[:-1]] == sorted(set(r[1] for r in rows[:-1]))      # strictly ascending with the doubles


def _limb_sums(contribs):
    """[3][n] uint64 limb sums of per-token lists of integers, each split as fixed_split does (a0, a1 in [0, 2^32), a2 = v >> 64 signed),
    the sums wrapped to 64 bits"""
    M32, M64 = (1 << 32) - 1, (1 << 64) - 1
    out = np.zeros((3, len(contribs)), dtype=np.uint64)
    for j, vs in enumerate(contribs):
        out[0, j] = sum(v & M32 for v in vs) & M64
        out[1, j] = sum((v >> 32) & M32 for v in vs) & M64
        out[2, j] = sum(v >> 64 for v in vs) & M64
    return out


def test_route_psi_from_limbs_against_python_integers(tmp_path):
    """csrc/route_rules.hpp: psi_from_limbs = fixed_combine, ONE correctly rounded conversion, one exact scaling.  Limb sums of exact
    floors (helpers.exact_floor) for a negative sum, a sum whose low limbs carry (5000 contributions with full low limbs: l0, l1 beyond
    2^32), sums beyond 2^64 in magnitude of both signs, more than 53 significant bits (the conversion must round, once), zero: the
    result equals math.ldexp(float(v), -F) exactly, v the Python integer the limbs stand for (helpers.limbs_as_integers)."""
    import math
    from helpers import exact_floor, limbs_as_integers
    F = 40
    ys = [[-3.75, 1.5, -2.0 ** -45],                                     # negative, with a fraction that floors away
          [(2.0 ** 32 - 1) * 2.0 ** -F] * 5000 + [(2.0 ** 32 - 1) * 2.0 ** (32 - F)] * 5000,       # a0 = 2^32 - 1, then a1 = 2^32 - 1, 5000 times each: both low sums carry
          [2.0 ** 30, 2.0 ** 41 + 1.0, 3.0 * 2.0 ** 40],                 # 2^F y beyond 2^64
          [-2.0 ** 41 - 2.0 ** -11, -7.0 * 2.0 ** 39, -2.0 ** -45],      # ... and negative
          [2.0 ** 30 + 2.0 ** -22, 2.0 ** -40, 2.0 ** -40, 1.0 + 2.0 ** -39],      # 71 significant bits: rounded once
          [0.0]]
    ints = [exact_floor(np.array(y), F) for y in ys]
    limbs = _limb_sums(ints)
    want = [sum(v) for v in ints]
    assert limbs_as_integers(limbs) == want
    assert want[0] < 0 and int(limbs[0, 1]) >= 2 ** 32 and int(limbs[1, 1]) >= 2 ** 32 and want[2] > 2 ** 64 and want[3] < -2 ** 64 and want[4].bit_length() > 53
    n = len(ys)
    got = _route_rules_program(tmp_path, "psi", "    const unsigned long long hl[] = {%s};\n    double psi[%d];\n    psi_from_limbs(hl, %d, %d, psi);\n    row(\"psi\", psi, %d);"
                               % (", ".join("%dull" % int(x) for x in limbs.reshape(-1)), n, n, F, n))
    assert [float(x) for x in got[0].split()[1:]] == [math.ldexp(float(v), -F) for v in want]


def test_route_value_and_infeasibility_of_the_audited_psi_against_the_numpy_twin(tmp_path):
    """csrc/route_rules.hpp: psi_worth against cfmm.problem.audit_trades on the SAME psi (the twin's own): the shipped arbitrage instance
    at the fixture's KKT point with its utility, and hand-made tenders on a random six-token network under a hand-made utility with one
    token of every kind (GE, EQ, FREE, ULOG, UQUAD, and a second GE with h < 0 that is violated).  Both add the tokens' terms in token
    order in doubles and take the same maxima: infeas must be EQUAL, value within one ulp of the twin's (both cases gave equal bits; the
    ulp is for the ULOG term, which goes through the C library's log here and NumPy's there)."""
    import math
    from cfmm.problem import Utility, audit_trades, audit_buckets
    from test_audit_host import kkt_route
    cases = []
    p, _, tr = kkt_route("arbitrage", dict(shipped_cases())["arbitrage"])
    cases.append(("shipped", p.net, tr, p.utility))
    q = problem_of(random_instance(5, n_tokens=6, n_pools=10))
    tr = {}
    for b in audit_buckets(q.net):
        d, l = np.zeros_like(b["R"]), np.zeros_like(b["R"])
        d[0] = 0.0625 * b["R"][0]; l[1] = 0.03125 * b["R"][1]
        tr[b["key"]] = (d, l)
    ct = np.array([_lib.GE, _lib.EQ, _lib.FREE, _lib.ULOG, _lib.UQUAD, _lib.GE], dtype=np.int32)
    cases.append(("hand", q.net, tr, Utility(np.array([1.0, 0.9, 1.1, 2.5, 1.2, 0.8]), np.array([0.5, 0.25, 3.0, 1e3, 40.0, -1e3]), ct)))
    body, want = "", {}
    for name, net, tr, util in cases:
        rep = audit_trades(net, tr, util)
        mr = max(float(b["R"].max()) for b in audit_buckets(net))
        want[name] = (rep, util)
        body += ("    { " + _cvec("psi", rep["psi"]) + _cvec("c", util.c) + _cvec("h", util.h) + _cvec("ct", util.ctype, "int")
                 + " const PsiWorth w = psi_worth(psi, %d, c, h, ct, %r); const double v[] = {w.value, w.infeas}; row(\"%s\", v, 2); }\n" % (len(rep["psi"]), mr, name))
    got = _keyed(_route_rules_program(tmp_path, "worth", body))
    for name, (rep, util) in want.items():
        value, infeas = [float(x) for x in got[name][0].split()]
        print(name, "value", value, rep["value"], "infeas", infeas, rep["infeas"])
        assert infeas == rep["infeas"], (name, infeas, rep["infeas"])
        assert abs(value - rep["value"]) <= math.ulp(rep["value"]), (name, value, rep["value"])
    assert want["hand"][0]["infeas"] > 0.0 and np.isfinite(want["hand"][0]["value"]) and want["shipped"][0]["infeas"] <= 1e-12


def test_switch_records_of_a_k_asset_constant_sum_pool_are_rooted_at_the_paying_leg():
    """cfmm/problem.py: _canonical_switches, _split_payers (round 6, pure functions of the records: every rank of a pool-sharded solve
    computes the same).  Three tokens tied for cheapest, found pair by pair in rounds whose cheapest token differed -- records (0, 3) and
    (2, 3) -- become (0, 2) and (0, 3): rooted at the leg the device makes pay (the lowest of the tied legs), same union of tied tokens.
    A partly drained leg of such a pool gets one record per cheapest token that could pay for it."""
    from cfmm.problem import Problem, _drain_leg
    pidx, pR = [10, 11, 12, 13], [5.0, 6.0, 7.0, 8.0]
    sw = lambda a, b: dict(sgn=0, ia=pidx[a], ib=pidx[b], fee=0.99, Ra=0.0, Rb=0.0, loose=False, leg_a=a, leg_b=b, pool=7, k=4, pidx=pidx, pR=pR)
    tied = {(0, 4, 7, 103): sw(0, 3), (0, 4, 7, 123): sw(2, 3)}
    out = Problem._canonical_switches(tied, set())
    assert sorted(out) == [(0, 4, 7, 102), (0, 4, 7, 103)]
    assert [(r["leg_a"], r["leg_b"], r["ia"], r["ib"]) for r in out.values()] == [(0, 2, 10, 12), (0, 3, 10, 13)]
    assert Problem._canonical_switches(out, set()) == out                                   # (a fixed point)
    assert sorted(Problem._canonical_switches(tied, {((0, 4, 7, 102), 0)})) == [(0, 4, 7, 103)]      # (a banned record is not re-created)
    # a drain record of leg 1 paid for by leg 0, with legs 0, 2, 3 tied for cheapest: one more record per other payer
    drain = dict(sgn=1, ia=pidx[0], ib=pidx[1], fee=0.99, Ra=pR[0], Rb=pR[1], loose=False, leg_lo=0, pidx=pidx, pR=pR)
    both = dict(out); both[(0, 4, 7, 1)] = drain
    sp = Problem._split_payers(dict(sorted(both.items())), set())
    assert sorted(k[3] for k in sp) == [1, 102, 103, 221, 231]
    assert (sp[(0, 4, 7, 221)]["ia"], sp[(0, 4, 7, 221)]["leg_lo"], sp[(0, 4, 7, 221)]["Ra"], sp[(0, 4, 7, 221)]["ib"]) == (12, 2, 7.0, 11)
    assert [_drain_leg(c) for c in (1, 221, 231)] == [1, 1, 1]
    assert Problem._split_payers(sp, set()) == sp
    # a pool without tied payers, and a payer that is not among the tied tokens: nothing to split
    assert Problem._split_payers({(0, 4, 7, 1): drain}, set()) == {(0, 4, 7, 1): drain}
    other = dict(drain, leg_lo=1, ia=pidx[1], ib=pidx[2], Ra=pR[1], Rb=pR[2])
    lone = {(0, 4, 7, 2): other, (0, 4, 7, 103): sw(0, 3)}
    assert Problem._split_payers(dict(sorted(lone.items())), set()) == dict(sorted(lone.items()))
