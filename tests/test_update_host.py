"""CPU tests of the in-place reserve update's host half: cfmm.problem.route_updates maps pool-list indices to (bucket,
position) with slot-major reserve columns and refuses what the library would refuse; Problem.update_bucket keeps the host copy
of the network in step before any device exists."""
import numpy as np
import pytest

import cfmm
from cfmm.problem import route_updates

# one pool of every kind: cp2, w2, sum2, curve2, pow2, geo-mean k = 3 and 4, table stableswap k = 3, table constant sum k = 4
IDX = [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [0, 1, 2], [1, 2, 3, 4], [2, 3, 4], [0, 2, 4, 5], [1, 5]]
RES = [[10, 20], [30, 40], [5, 6], [7, 8], [9, 11], [1, 2, 3], [4, 5, 6, 7], [8, 9, 10], [11, 12, 13, 14], [3, 4]]
KINDS = ["geomean", "geomean", "sum", "curve", "powersum", "geomean", "geomean", "curve", "sum", "geomean"]
WEIGHTS = [None, [0.3, 0.7], None, None, None, None, None, None, None, None]
PARAMS = [None, None, None, 50.0, 0.4, None, None, 20.0, None, None]


def mixed():
    return cfmm.pack(6, IDX, RES, [0.997] * len(IDX), KINDS, WEIGHTS, PARAMS)


def test_route_updates_maps_every_kind_to_its_bucket_and_position():
    net, where = mixed()
    assert where[0] == ("cp2", 0) and where[9] == ("cp2", 1)
    pools = [9, 0, 1, 2, 3, 4, 5, 6, 7, 8]
    new = [np.asarray(RES[i], dtype=float) * (1.5 + i) for i in pools]
    params = [None, None, None, None, 60.0, None, None, None, 25.0, None]
    out = route_updates(net, where, pools, new, params)
    assert set(out) == {"cp2", "w2", "sum2", "curve2", "pow2", 3, 4, ("stable", 3), ("sum", 4)}
    pos, R, prm = out["cp2"]
    assert pos.dtype == np.int32 and pos.tolist() == [0, 1]                 # ascending positions, whatever order they came in
    assert R.shape == (2, 2) and R[:, 0].tolist() == new[1].tolist() and R[:, 1].tolist() == new[0].tolist()
    assert prm is None
    pos, R, prm = out["curve2"]
    assert pos.tolist() == [0] and R[:, 0].tolist() == new[4].tolist() and prm.tolist() == [60.0]
    pos, R, prm = out["pow2"]
    assert prm is None                                                      # (its parameter not given: unchanged, no column)
    for key, i in ((3, 5), (4, 6), (("stable", 3), 7), (("sum", 4), 8)):
        pos, R, prm = out[key]
        k = key if isinstance(key, int) else key[1]
        assert pos.tolist() == [0] and R.shape == (k, 1)                    # slot-major [k][count]
        assert R[:, 0].tolist() == new[pools.index(i)].tolist()
    assert out[("stable", 3)][2].tolist() == [25.0]
    assert out[("sum", 4)][2] is None


def test_route_updates_keeps_the_current_parameter_of_entries_without_one():
    net, where = cfmm.pack(4, [[0, 1], [1, 2], [2, 3]], [[1, 2], [3, 4], [5, 6]], [0.99] * 3, ["curve"] * 3, params=[5.0, 6.0, 7.0])
    out = route_updates(net, where, [2, 0], [[1, 1], [2, 2]], [None, 9.0])
    pos, R, prm = out["curve2"]
    assert pos.tolist() == [0, 2] and prm.tolist() == [9.0, 7.0]


def test_route_updates_rejects_length_mismatches():
    net, where = mixed()
    with pytest.raises(ValueError, match="2 pools but 1 reserve vectors"):
        route_updates(net, where, [0, 1], [[1, 2]])
    with pytest.raises(ValueError, match="1 pools but 2 parameters"):
        route_updates(net, where, [0], [[1, 2]], [None, None])
    with pytest.raises(ValueError, match="3 indices but 4 reserves"):           # a three-asset pool given four reserves
        route_updates(net, where, [5], [[1, 2, 3, 4]])


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_route_updates_rejects_reserves_that_are_not_positive_and_finite(bad):
    net, where = mixed()
    with pytest.raises(ValueError, match="reserves must be > 0"):
        route_updates(net, where, [0], [[1.0, bad]])


def test_route_updates_rejects_out_of_range_duplicates_and_bad_parameters():
    net, where = mixed()
    with pytest.raises(ValueError, match="outside"):
        route_updates(net, where, [10], [[1, 2]])
    with pytest.raises(ValueError, match="outside"):
        route_updates(net, where, [-1], [[1, 2]])
    with pytest.raises(ValueError, match="twice"):
        route_updates(net, where, [0, 0], [[1, 2], [3, 4]])
    with pytest.raises(ValueError, match="alpha > 0"):
        route_updates(net, where, [3], [[1, 2]], [-5.0])
    with pytest.raises(ValueError, match="t in"):
        route_updates(net, where, [4], [[1, 2]], [1.5])
    with pytest.raises(ValueError, match="no parameter"):
        route_updates(net, where, [0], [[1, 2]], [0.5])


def test_update_before_upload_changes_only_the_host_network():
    """no device needed: a Problem that never uploaded keeps its host network in step (the upload later takes the new values)"""
    net, where = mixed()
    p = cfmm.Problem(6, IDX, RES, [0.997] * len(IDX), KINDS, WEIGHTS, PARAMS)
    p.update_reserves([3, 7, 6], [[70, 80], [80, 90, 100], [40, 50, 60, 70]], [55.0, 21.0, None])
    assert p.net["curve2"]["Ra"][0] == 70 and p.net["curve2"]["alpha"][0] == 55.0
    assert p.net["gk"][("stable", 3)]["R"][:, 0].tolist() == [80, 90, 100] and p.net["gk"][("stable", 3)]["param"][0] == 21.0
    assert p.net["gn"][4]["R"][:, 0].tolist() == [40, 50, 60, 70]
    assert p.net["cp2"]["Ra"].tolist() == [10, 3]                            # untouched
    with pytest.raises(ValueError):
        p.update_bucket("cp2", [0], [[1.0], [0.0]])
    with pytest.raises(ValueError):
        p.update_bucket(5, [0], np.ones((5, 1)))                             # no bucket of five-asset pools
    q = cfmm.Problem.from_network(net)
    with pytest.raises(cfmm.CfmmError):
        q.update_reserves([0], [[1, 2]])                                    # no pool list: update_bucket instead


def test_shard_updates_picks_each_ranks_slice_in_local_positions():
    m, world = 10, 3                                                       # slices [0, 3), [3, 6), [6, 10) as shard_network cuts them
    pos = np.array([9, 0, 4, 3, 6])
    R = np.vstack([pos + 100.0, pos + 200.0])
    parts = [cfmm.problem.shard_updates(m, r, world, pos, R, pos * 1.0) for r in range(world)]
    assert [p[0].tolist() for p in parts] == [[0], [1, 0], [3, 0]]
    assert parts[1][1][:, 0].tolist() == [104.0, 204.0] and parts[2][2].tolist() == [9.0, 6.0]
    from cfmm import synthetic
    net = synthetic.config("C3", scale=0.001)
    for key in ("cp2", "w2"):                                              # the same cut as shard_network
        mk = len(net[key]["Ra"])
        for r in range(world):
            lo, hi = cfmm.problem.shard_range(mk, r, world)
            assert np.array_equal(cfmm.shard_network(net, r, world)[key]["Ra"], net[key]["Ra"][lo:hi])
    empty = cfmm.problem.shard_updates(m, 0, world, [7], [[1.0], [2.0]])
    assert len(empty[0]) == 0 and empty[1].shape == (2, 0)


def test_an_update_through_one_problem_reaches_problems_sharing_its_network():
    """clones share the host network: the largest reserve and the start prices they cached follow an update made through another"""
    net, where = mixed()
    a = cfmm.Problem(6, IDX, RES, [0.997] * len(IDX), KINDS, WEIGHTS, PARAMS, utility=cfmm.Arbitrage(np.ones(6)))
    b = cfmm.Problem(6, network=a.net, utility=a.utility)
    b.where = a.where
    assert a._max_reserve() == 40.0 and b._max_reserve() == 40.0
    s0 = cfmm.start_prices(a.net, a.utility)
    b.update_reserves([1], [[300.0, 40.0]])
    assert a._max_reserve() == 300.0 and b._max_reserve() == 300.0
    assert a.net["w2"]["Ra"][0] == 300.0
    # start prices memoised on the utility are propagated through the reserves: an update through b re-derives a's
    u = cfmm.Arbitrage(np.array([1.0, 0, 0, 0, 0, 0]))
    s0 = cfmm.start_prices(a.net, u)
    assert np.array_equal(cfmm.start_prices(a.net, u), s0)                # (memoised)
    b.update_reserves([0], [[10.0, 80.0]])                                # pool 0: tokens 0, 1
    s1 = cfmm.start_prices(a.net, u)
    assert s1[1] != s0[1]
