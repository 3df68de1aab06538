"""CPU suite: the host side of applying a solve's trades to the pools (docs/apply_trades.md) -- the reserve expression in both fee
conventions, the layout of cfmm_apply_info as bound by cfmm/_lib.py, and the choice between the device pass and the host path."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cfmm
from cfmm import _lib, synthetic
from cfmm.problem import post_trade_reserves, apply_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_post_trade_reserves_by_hand_in_both_fee_modes():
    """three two-asset pools, hand-computed: a plain swap, a pool that does not trade, and GROSS tenders (leg a both receives 2 and
    pays 1, as after a second-order solve) -- binary fractions, so every figure is exact"""
    R = np.array([[100.0, 50.0, 8.0], [200.0, 60.0, 16.0]])
    delta = np.array([[4.0, 0.0, 2.0], [0.0, 0.0, 0.5]])
    lam = np.array([[0.0, 0.0, 1.0], [7.5, 0.0, 4.0]])
    fee = np.array([0.75, 0.5, 0.5])
    pool = post_trade_reserves(R, delta, lam, fee, "pool")
    assert np.array_equal(pool, np.array([[104.0, 50.0, 9.0], [192.5, 60.0, 12.5]]))
    aside = post_trade_reserves(R, delta, lam, fee, "aside")
    assert np.array_equal(aside, np.array([[103.0, 50.0, 8.0], [192.5, 60.0, 12.25]]))
    assert np.array_equal(post_trade_reserves(R, delta, lam, fee), pool)                    # "pool" is the default
    # a single column of a bucket, and k-asset shapes, broadcast the per-pool fee the same way
    assert np.array_equal(post_trade_reserves(R[0], delta[0], lam[0], fee, "aside"), aside[0])
    R3 = np.arange(1.0, 7.0).reshape(3, 2) * 8.0
    d3 = np.array([[1.0, 0.0], [0.0, 2.0], [0.0, 0.0]]); l3 = np.array([[0.0, 4.0], [2.0, 0.0], [0.0, 0.0]])
    assert np.array_equal(post_trade_reserves(R3, d3, l3, np.array([0.5, 0.25]), "aside"),
                          np.array([[8.5, 12.0], [22.0, 32.5], [40.0, 48.0]]))
    # the order of the operations is (R + g delta) - lam, each rounded on its own
    big, one = np.array([2.0 ** 53]), np.array([1.0])
    assert post_trade_reserves(big, one, big, one, "pool")[0] == 0.0
    with pytest.raises(ValueError):
        post_trade_reserves(R, delta, lam, fee, "burn")


def test_apply_info_matches_the_header_layout(tmp_path):
    """cfmm_apply_info as bound by cfmm/_lib.py has the size and the field offsets the C compiler gives the header's struct"""
    fields = [f for f, _ in _lib.ApplyInfo._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cfmm.h"', 'int main(void) {',
             'printf("%zu\\n", sizeof(cfmm_apply_info));']
    lines += [f'printf("%zu\\n", offsetof(cfmm_apply_info, {f}));' for f in fields]
    lines += ['printf("%d %d\\n", CFMM_FEES_TO_POOL, CFMM_FEES_ASIDE);', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert int(out[0]) == ctypes.sizeof(_lib.ApplyInfo)
    assert [int(x) for x in out[1:1 + len(fields)]] == [getattr(_lib.ApplyInfo, f).offset for f in fields]
    assert [int(x) for x in out[1 + len(fields):]] == [_lib.FEE_MODES["pool"], _lib.FEE_MODES["aside"]]
    info = _lib.ApplyInfo(pools_moved=3, pools_refused=1, first_family=0, first_kind=2, first_k=2, first_pos=137, max_reserve=2.5)
    assert info.asdict() == dict(pools_moved=3, pools_refused=1, first_family=0, first_kind=2, first_k=2, first_pos=137, max_reserve=2.5)


def test_apply_takes_the_device_pass_unless_fills_ties_or_shards_say_otherwise():
    assert apply_path({}, False, False) == "device"
    assert apply_path({(0, 2, 4, 0): (dict(), 0.386)}, False, False) == "host"        # fills held on the host
    assert apply_path({}, True, False) == "host"                                      # price ties / tie flags on the device
    assert apply_path({}, False, True) == "host"                                      # pool-sharded
    # ... as a Problem's state drives it (no context is made: the predicate reads host state only)
    net = synthetic.make_network(16, m_cp2=20, seed=1)
    p = cfmm.Problem.from_network(net, utility=cfmm.Arbitrage(net["c"]))
    assert p._apply_path() == "device" and p.ctx is None
    p._theta = {(0, 2, 1, 0): (dict(), 0.5)}
    assert p._apply_path() == "host"
    p._theta = {}; p._dev_ties = True
    assert p._apply_path() == "host"
    p._dev_ties = False; p._comm = (2, 0)
    assert p._apply_path() == "host"
    p._comm = None
    assert p._apply_path() == "device"
    with pytest.raises(ValueError):
        p.apply_trades(fees="burn")
    assert p.ctx is None
