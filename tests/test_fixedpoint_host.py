"""CPU suite: the reproducible mode's fixed-point arithmetic (csrc/fixedpoint.hpp) against exact integers.  The header is the code
Scatter<true>::add and det_fold_kernel run on the device; here the host compiler builds it into a stand-alone program, and every
limb it produces is compared with Python integers: equality, no tolerance, no input left out."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np

from helpers import FIXED_EDGES, fixed_scale_exponent, fixed_random_scaled, exact_floor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cfmm-routing-code_amd", "csrc")

PROBE = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "fixedpoint.hpp"
// split F:   doubles y on stdin -> (a0, a1, a2) of fixed_split(y * 2^F) as three 32-bit words each on stdout
// combine:   (l0, l1, l2) 64-bit limb sums on stdin -> (hi, lo) of fixed_combine on stdout
int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "split")) {
        const double sc = ldexp(1.0, atoi(argv[2]));
        double y;
        while (fread(&y, sizeof y, 1, stdin) == 1) {
            const cfmm::FixedLimbs a = cfmm::fixed_split(y * sc);
            const unsigned out[3] = {a.a0, a.a1, (unsigned)a.a2};
            if (fwrite(out, sizeof out, 1, stdout) != 1) return 3;
        }
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "combine")) {
        unsigned long long l[3];
        while (fread(l, sizeof l, 1, stdin) == 1) {
            const cfmm::Fixed128 t = cfmm::fixed_combine(l[0], l[1], l[2]);
            const unsigned long long out[2] = {(unsigned long long)t.hi, t.lo};
            if (fwrite(out, sizeof out, 1, stdout) != 1) return 3;
        }
        return 0;
    }
    return 2;
}
"""
UBSAN = ["-fsanitize=undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all"]

EDGES = FIXED_EDGES + [2.0 ** 95 - 2.0 ** 42]            # ... and the last double inside the split's own range
REF_RESERVES = (1e-3, 1.0, 1e6, 1e12)
REF_FEES = (0.997, 1e-3)


def scaled_inputs(n_random=1_000_000, seed=20260419):
    """the edge list with both signs, then `n_random` seeded values"""
    edges = np.array(EDGES)
    return np.concatenate([edges, -edges, fixed_random_scaled(n_random, seed)])


def build_probe(tmp_path, name, flags=(), include=CSRC):
    src = tmp_path / "fixedpoint_probe.cpp"
    src.write_text(PROBE)
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O2", *flags, "-I", include, str(src), "-o", str(exe)])
    return str(exe)


def run_split(exe, y, F):
    """the program's limbs as Python integers a2 2^64 + a1 2^32 + a0 (0 <= a0, a1 < 2^32 by their type; a2 a signed 32-bit word)"""
    r = subprocess.run([exe, "split", str(F)], input=np.ascontiguousarray(y, dtype="<f8").tobytes(), stdout=subprocess.PIPE, check=True)
    w = np.frombuffer(r.stdout, dtype="<u4").reshape(-1, 3)
    assert len(w) == len(y)
    a0, a1, a2 = w[:, 0].tolist(), w[:, 1].tolist(), w[:, 2].view(np.int32).tolist()
    return [(c << 64) + (b << 32) + a for a, b, c in zip(a0, a1, a2)]


def split_mismatches(exe, yf, F):
    """indices at which the program's limbs differ from floor(Fraction(y) 2^F)"""
    y = yf * 2.0 ** -F
    assert np.array_equal(y * 2.0 ** F, yf)                                     # the way back to scaled units is exact
    want = exact_floor(y, F)
    # the shift form above IS floor(Fraction(y) * 2**F): literally so on the edges and on a sample of the rest
    lit = np.r_[0:2 * len(EDGES), np.random.default_rng(F).integers(0, len(y), 2000)]
    assert all(want[i] == math.floor(Fraction(float(y[i])) * Fraction(2) ** F) for i in lit.tolist())
    got = run_split(exe, y, F)
    return [i for i, (g, w) in enumerate(zip(got, want)) if g != w]


def test_fixed_split_is_the_exact_floor_for_both_signs(tmp_path):
    """fixed_split(y 2^F) == floor(Fraction(y) 2^F) as a2 2^64 + a1 2^32 + a0 with 0 <= a0, a1 < 2^32, for the edge list in both
    signs and 1e6 seeded values, at every exponent det_scales derives from reference reserves 1e-3 .. 1e12 and fees 0.997, 1e-3.
    The same inputs through a build with the undefined-behaviour sanitizer (float-to-integer range included) exit clean and
    give the same bytes.  (The top-limb-first split this replaces, restated for the host with saturating conversions, fails here on
    394 238 of the 1 000 034 inputs at every exponent: 79 % of the negative ones, none of the positive.)"""
    exe = build_probe(tmp_path, "probe")
    exe_ub = build_probe(tmp_path, "probe_ubsan", UBSAN)
    yf = scaled_inputs()
    assert len(yf) >= 1_000_000 and (yf < 0).sum() > 400_000 and np.abs(yf).max() < 2.0 ** 95
    exps = sorted({fixed_scale_exponent(mr, mf) for mr in REF_RESERVES for mf in REF_FEES})
    assert exps[0] == 84 - 50 and exps[-1] == 84 + 9 and len(exps) >= 6
    for F in exps:
        bad = split_mismatches(exe, yf, F)
        assert not bad, f"F = {F}: {len(bad)} of {len(yf)} inputs differ from the exact floor, first yf = {[float(yf[i]).hex() for i in bad[:5]]}"
        y = np.ascontiguousarray(yf * 2.0 ** -F, dtype="<f8").tobytes()
        plain = subprocess.run([exe, "split", str(F)], input=y, stdout=subprocess.PIPE, check=True)
        ub = subprocess.run([exe_ub, "split", str(F)], input=y, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert ub.returncode == 0 and ub.stderr == b"", ub.stderr.decode()[:2000]
        assert ub.stdout == plain.stdout


def test_fixed_combine_is_exact_on_wrapped_limb_sums(tmp_path):
    """fixed_combine(l0, l1, l2) == l2 2^64 + l1 2^32 + l0 in Python integers, with l2 a wrapped signed 64-bit sum and l0, l1 unsigned:
    negative l2 (a net tender), l0 and l1 carrying up to 2^32 contributions of 2^32 - 1, and the corners of every limb's range"""
    exe = build_probe(tmp_path, "probe")
    exe_ub = build_probe(tmp_path, "probe_ubsan", UBSAN)
    top = 2 ** 32 * (2 ** 32 - 1)
    rng = np.random.default_rng(7)
    cases = [(0, 0, 0), (top, top, 0), (top, top, -1), (top, top, -2 ** 41), (0, 0, -2 ** 41), (1, 0, -1), (0, top, 2 ** 41 - 1),
             (2 ** 32 - 1, 2 ** 32 - 1, -2 ** 31), (top, 0, -2 ** 62), (2 ** 64 - 1, 2 ** 64 - 1, -1), (2 ** 64 - 1, 2 ** 64 - 1, -2 ** 62),
             (2 ** 63, 2 ** 63, 2 ** 62 - 1), (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 62 - 1)]
    u64 = dict(dtype=np.uint64, endpoint=True)
    cases += [(int(a), int(b), int(c)) for a, b, c in zip(rng.integers(0, top, 1000, **u64), rng.integers(0, top, 1000, **u64), rng.integers(-2 ** 41, 2 ** 41, 1000))]
    cases += [(int(a), int(b), int(c)) for a, b, c in zip(rng.integers(0, 2 ** 64 - 1, 200, **u64), rng.integers(0, 2 ** 64 - 1, 200, **u64),
                                                          rng.integers(-2 ** 62, 2 ** 62, 200))]
    raw = np.array([[v % 2 ** 64 for v in c] for c in cases], dtype=np.uint64).astype("<u8").tobytes()
    outs = []
    for e in (exe, exe_ub):
        r = subprocess.run([e, "combine"], input=raw, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()[:2000]
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    w = np.frombuffer(outs[0], dtype="<u8").reshape(-1, 2)
    assert len(w) == len(cases)
    for (l0, l1, l2), hi, lo in zip(cases, w[:, 0].view(np.int64).tolist(), w[:, 1].tolist()):
        value = l2 * 2 ** 64 + l1 * 2 ** 32 + l0
        assert -2 ** 127 <= value < 2 ** 127
        assert hi * 2 ** 64 + lo == value, (l0, l1, l2)
