"""CPU: the SRS v1-V reference (tests/values_ref.py).  With x_i = i and no weights it is the plain
reference bit for bit, on all four topologies with and without faults; every admissibility rule
refuses its counter-example and accepts the value just inside."""
import math
import struct

import pytest

from oracle.srs_py import PySim
from tests import values_ref as V
from tests.faults_ref import FaultSim

TOPOS = ("line", "full", "3D", "Imp3D")
FAULTS = (0.1, 0.05, 3)


def bits(v):
    return [struct.pack("<d", x) for x in v]


@pytest.mark.parametrize("topo", TOPOS)
def test_ids_as_values_equal_the_plain_reference(topo):
    n, seed = 60, 5
    ref = PySim(n, topo, "push-sum", seed)
    sim = V.ValueSim(n, topo, [float(i) for i in range(ref.P)], seed=seed, max_rounds=10 ** 6)
    assert sim.mean == (ref.P - 1) / 2
    for _ in range(60):
        assert sim.step(7) == ref.step(7)
        assert bits(sim.s) == bits(ref.s) and bits(sim.w) == bits(ref.w) and sim.flags() == ref.flags()
        if ref.done:
            break
    assert sim.round == ref.round and sim.alerts_total == ref.alerts_total


@pytest.mark.parametrize("topo", TOPOS)
def test_ids_as_values_equal_the_fault_reference(topo):
    n, seed = 60, 9
    ref = FaultSim(n, topo, "push-sum", seed, *FAULTS, max_rounds=300)
    sim = V.ValueSim(n, topo, [float(i) for i in range(ref.P)], [1.0] * ref.P, seed, None, *FAULTS, max_rounds=300)
    while not ref.done:
        assert sim.step(11) == ref.step(11)
        assert bits(sim.s) == bits(ref.s) and bits(sim.w) == bits(ref.w) and sim.flags() == ref.flags()
    assert sim.done and sim.stats() == ref.stats() and sim.status == ref.status


def test_values_change_the_run():
    a = V.ValueSim(26, "3D", [0.1 * (i + 1) for i in range(27)], seed=3)
    b = V.ValueSim(26, "3D", [float(i) for i in range(27)], seed=3)
    a.step(20)
    b.step(20)
    assert bits(a.s) != bits(b.s) and bits(a.w) == bits(b.w)


up, down = (lambda v: math.nextafter(v, math.inf)), (lambda v: math.nextafter(v, 0.0))


@pytest.mark.parametrize("x,w,want", [
    (-0.0, 1.0, V.X_SIGN), (math.inf, 1.0, V.X_SIGN), (math.nan, 1.0, V.X_SIGN), (-1.0, 1.0, V.X_SIGN),
    (1.0, -0.0, V.W_SIGN), (1.0, math.inf, V.W_SIGN), (1.0, math.nan, V.W_SIGN),
    (5e-324, 1.0, V.X_TINY), (2.0 ** -1023, 1.0, V.X_TINY), (down(2.0 ** -64), 1.0, V.X_TINY),
    (1.0, 2.0 ** -33, V.W_RANGE), (0.0, down(2.0 ** -32), V.W_RANGE), (1.0, up(2.0 ** 32), V.W_RANGE), (1.0, 0.0, V.W_RANGE),
    (2.0 ** 32, 1.0, V.RATIO), (2.0 ** 32 * 3.0, 3.0, V.RATIO), (1.0, 2.0 ** -32, V.RATIO), (2.0 ** 64, 2.0 ** 32, V.RATIO),
])
def test_rule_refuses_its_counter_example(x, w, want):
    assert V.rule(x, w) == want


@pytest.mark.parametrize("x,w", [
    (0.0, 1.0), (0.0, 2.0 ** -32), (0.0, 2.0 ** 32), (2.0 ** -64, 1.0), (2.0 ** -64, 2.0 ** 32),
    (down(2.0 ** 32), 1.0), (down(2.0 ** 32 * 3.0), 3.0), (down(1.0), 2.0 ** -32), (down(2.0 ** 64), 2.0 ** 32),
    (1.0, up(2.0 ** -32)), (2.0 ** 63, 2.0 ** 32), (0.1, 1.0),
])
def test_rule_accepts_the_value_just_inside(x, w):
    assert V.rule(x, w) == V.OK


def test_first_offender_is_the_lowest_id():
    x = [0.1, 0.2, -0.0, 0.4, math.nan]
    assert V.first_offender(x) == (2, V.X_SIGN)
    assert V.first_offender(x[:2]) is None
    assert V.first_offender([1.0, 1.0], [1.0, 2.0 ** -33]) == (1, V.W_RANGE)
    with pytest.raises(ValueError):
        V.ValueSim(4, "line", x)


def test_mean():
    x, w = [0.1 * (i + 1) for i in range(61)], [1.0 + (i % 3) for i in range(61)]
    assert V.default_mean(x) == math.fsum(x) / 61
    assert V.default_mean(x, w) == math.fsum(x) / math.fsum(w)
    assert V.ValueSim(60, "full", x, w).mean == V.default_mean(x, w)
    assert V.mean_ok(0.0) and V.mean_ok(down(2.0 ** 32))
    assert not any(V.mean_ok(m) for m in (-1e-300, 2.0 ** 32, math.inf, math.nan))
