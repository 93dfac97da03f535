"""CPU suite: the C restatement's matchers (oracle/slam_oracle.c: orc_process_scan over the BF / HC / MC enumerators) on the
DESIGNED score landscapes of tests/landscape_cases.py, against
  * tests/golden/landscapes.npz -- the compiled reference's decisions on the same tables
    (tests/golden/make_golden_landscapes.py), bit for bit, for every case the reference did not refuse (its obstacle
    OOPE asserts on a NaN impact: the NaN cases are the oracle's alone);
  * the author's expected decision for every BF and HC case, NaN cases included: the accepted calls, the winner and the
    number of calls that landscape_cases.accept_loop derives from the designed score sequence.
tests/test_gpu_landscapes.py holds the device to the same two references."""
import numpy as np
import pyoracle as po
import pytest
from landscape_cases import (BF_SIZES, DRAWN_MARGIN, POSITIONS, accept_loop, all_cases, assert_equals_row, bf_case, bits,
                             cases_of, golden_rows, load_golden, margin_holds, oracle_matches)

CASES = all_cases()
DESIGNED = [c for c in CASES if c.expect is not None]


def ids(cases):
    return ["%s-%s" % (c.kind, c.name) for c in cases]


@pytest.fixture(scope="module")
def g():
    return load_golden()


def test_the_golden_holds_every_case_and_only_nan_cases_are_refused(g):
    names = [c.kind + ":" + c.name for c in CASES]
    assert len(set(names)) == len(names) == 194
    nan_cases = {n for n, c in zip(names, CASES) if np.any(np.isnan(c.payload))}
    assert g["refused"] <= nan_cases and len(nan_cases) == 39
    assert sum(len(c.inits) for c in CASES if c.kind + ":" + c.name not in g["refused"]) == len(g["rows"])
    for c in CASES:
        rows = golden_rows(g, c)
        assert rows is None or len(rows) == len(c.inits)
    # every boundary size of the device arg-max and every listed position is a case of its own
    bf = [c.name for c in cases_of("BF")]
    for n in [nx * ny for nx, ny, _ in BF_SIZES] + [40401]:
        assert any(name.startswith("n%d-" % n) for name in bf), n
    for p in POSITIONS:
        assert any(name.endswith("-max_at_%d" % p) for name in bf), p
    for pair in ("63_64", "64_65", "1023_1024", "1024_1025"):
        assert any(name.endswith("-tie_" + pair) for name in bf), pair
    assert len(cases_of("HC")) == 16 and len(cases_of("MC")) == 4


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_oracle_equals_the_reference(oracle, g, c):
    rows = golden_rows(g, c)
    if rows is None:  # refused by the reference: the author's decision below is the bar (BF, HC)
        assert np.any(np.isnan(c.payload))
        return
    for t, row in zip(oracle_matches(c, oracle, po), rows):
        assert_equals_row(t, row)


@pytest.mark.parametrize("c", DESIGNED, ids=ids(DESIGNED))
def test_oracle_equals_the_authors_decision(oracle, c):
    for t, want, init in zip(oracle_matches(c, oracle, po), c.expect, c.inits):
        assert t["n_calls"] == want["n_calls"] == len(t["scores"])
        assert np.nonzero(t["accepted"])[0].tolist() == want["accepted"]
        win = want["win"]
        assert accept_loop(t["scores"]) == (want["accepted"], win)
        assert bits(t["prob"]) == bits(t["scores"][win])
        assert np.array_equal(t["delta"], t["poses"][win] - init)
        if win == 0:
            assert np.array_equal(t["delta"], [0.0, 0.0, 0.0])
        if c.kind == "BF":
            assert t["n_calls"] == 1 + c.shape[0] * c.shape[1] * c.shape[2]
            assert tuple(len(np.unique(t["poses"][1:, d])) for d in range(3)) == c.shape


def test_hill_climbing_plateaus_cost_the_calls_the_reference_makes(oracle):
    """nothing accepted: six candidates per failed round, and the one the enumerator hands out while it counts the last
    failed round (FailedRoundsLimitedPoseEnumerator::next, hill_climbing_scan_matcher.h:87-96)"""
    for c in cases_of("HC"):
        if c.name.startswith(("plateau", "nan_initial")):
            assert c.expect[0] == dict(n_calls=1 + 6 * c.params[0] + 1, accepted=[0], win=0)


def transposed(c):
    """the case's table walked y first: the same cells, x and y exchanged"""
    nx, ny, nt = c.shape
    cand = c.payload[1:1 + ny, 2:2 + nx]
    return bf_case(c.name + "-transposed", (ny, nx, nt), c.payload[1, 1], cand.T.ravel())


def test_the_golden_pins_the_order_of_the_walk(oracle, g):
    """x fastest, then y: walked y first, the tables with one maximum, two maxima and the staircases accept other calls
    (where only the first or the last candidate is accepted nothing can tell: the corners of a table stay where they are)"""
    n = 0
    for c in cases_of("BF"):
        kind = c.name.split("-", 1)[1]
        if not kind.startswith(("max_at_", "tie_", "staircase")) or min(c.shape[:2]) < 2 or c.shape == (201, 201, 1):
            continue
        if set(golden_rows(g, c)[0]["accepted"]) <= {0, 1, c.shape[0] * c.shape[1]}:
            continue
        t = oracle_matches(transposed(c), oracle, po)[0]
        assert t["n_calls"] == golden_rows(g, c)[0]["n_calls"]
        assert np.nonzero(t["accepted"])[0].tolist() != golden_rows(g, c)[0]["accepted"], c.name
        n += 1
    assert n >= 60


def test_drawn_poses_keep_clear_of_cell_edges(oracle):
    """The Monte-Carlo poses are drawn, not placed: none lies within 1e-7 m of a cell edge across which the value
    changes, so the cell under a pose does not depend on how its index is computed."""
    for c in cases_of("MC"):
        for t in oracle_matches(c, oracle, po):
            assert margin_holds(c.payload, c.origin, t["poses"], c.rng, DRAWN_MARGIN), c.name
            assert t["n_calls"] > 20
