"""GPU: the on-device state summary (gp_summary_take / gp_ensemble_summary, gp_summary.hip;
DESIGN.md section 10) against the numpy reference (tests/summary_ref.py) applied to the oracle's
state at the same round.

Comparison rules (summary_ref.py): integer fields, est / w min and max, err_max, err_max_node
and within_tol are bit-equal; the double-double sums meet two derived bounds (hi within 1 ulp
of math.fsum; hi + lo within 2^-70 relative of the exact rational sum).

Sizes are the smallest at which the kernel can go wrong: a partial wave, a partial 4-node flag
word, a partial 256-node segment, fewer nodes than the grid has lanes, more than one workgroup,
slabs whose arrays start at a halo (base != lo, also odd offsets), the LDS-resident 3D kernel
between step calls that end mid-epoch, and full push-sum (flags in nb[0]) at both parities.
"""
import ctypes as C
import math

import numpy as np
import pytest

from tests.summary_ref import assert_matches, assert_same_exact, field, raw, ref_summary

pytestmark = pytest.mark.gpu

TOLS = (0.0, 1e-10, 1e300)
ALGS = ("gossip", "push-sum")
ALG_ID = {"gossip": 0, "push-sum": 1}

SIZES = ([("line", a, n) for a in ALGS for n in (1, 2, 63, 64, 65, 255, 1023, 1024, 1025, 4099)] +
         [("full", a, n) for a in ALGS for n in (1, 255, 4099, 131071)] +
         [(t, a, n) for t in ("3D", "Imp3D") for a in ALGS for n in (8, 27, 1000, 8000)])


def check(sim, orc, what, tols=TOLS):
    """sim.summary() at every tol equals the reference over the oracle's state at the same round;
    two consecutive summaries are byte-identical."""
    from gossipprotocol_amd import _lib as L
    assert sim.rounds == orc.rounds
    st = orc.state()
    out = None
    for tol in tols:
        ref = ref_summary(st, 0, orc.P, orc.rounds, ALG_ID[sim.algorithm], orc.seed_node, tol)
        m = sim.summary(tol)
        assert_matches(m, ref, f"{what} round {orc.rounds} tol {tol}")
        assert raw(sim.summary(tol)) == raw(m), f"{what}: two summaries of one state differ"
        g = sim.summary(tol, scope="global")  # not an RCCL handle: equals local
        assert raw(g) == raw(m)
        out = m
    assert isinstance(out, L.GpSummary)
    return out


def both_step(sim, orc, k, what):
    a, b = sim.step(k), orc.step(k)
    assert a == b, f"{what}: per-round alerts differ from the oracle after a summary"


@pytest.mark.parametrize("topo,alg,n", SIZES)
def test_summary_matches_oracle(topo, alg, n, oracle):
    """Round 0, an odd round, and round 70 (3D push-sum at 8000: mid-epoch of the LDS-resident kernel)."""
    from gossipprotocol_amd import Simulation
    what = f"{topo} {alg} n={n}"
    with Simulation(n, topo, alg, seed=3) as sim:
        orc = oracle(n, topo, alg, 3)
        m0 = check(sim, orc, what)
        assert m0.rounds == 0 and m0.count == m0.population == sim.population
        if alg == "push-sum":
            assert field(m0, "sum_w") == [float(m0.count), 0.0]  # w = 1 everywhere, s = id
            assert m0.sum_s[0] == m0.count * (m0.count - 1) / 2 and m0.mean_estimate == (m0.count - 1) / 2
        else:
            assert m0.active == 1 and m0.c_hist[0] == m0.count
        both_step(sim, orc, 1, what)
        check(sim, orc, what)
        both_step(sim, orc, 69, what)
        check(sim, orc, what)
        both_step(sim, orc, 3, what)
        check(sim, orc, what, tols=(1e-10,))
        gs, os_ = sim.state(), orc.state()
        for k in ("c", "s", "w", "flags"):
            assert np.array_equal(gs[k], os_[k]), f"{what}: state '{k}' differs from the oracle after summaries"
        orc.close()


def test_summary_block_kernel_million(oracle):
    """3D push-sum at 10^6 runs on the LDS-resident block kernel: summaries between step calls that
    end mid-epoch (70 rounds, not 64), at an even and an odd round."""
    from gossipprotocol_amd import Simulation
    n, what = 10**6, "3D push-sum n=1e6"
    with Simulation(n, "3D", "push-sum", seed=2) as sim:
        orc = oracle(n, "3D", "push-sum", 2)
        both_step(sim, orc, 70, what)
        check(sim, orc, what, tols=(1e-10,))
        both_step(sim, orc, 71, what)
        check(sim, orc, what, tols=(0.0,))
        orc.close()


@pytest.mark.parametrize("topo,alg,n", [("3D", "push-sum", 1000), ("full", "push-sum", 255), ("line", "gossip", 255),
                                        ("Imp3D", "gossip", 1000)])
def test_summary_after_convergence(topo, alg, n, oracle):
    from gossipprotocol_amd import Simulation
    what = f"{topo} {alg} n={n} converged"
    with Simulation(n, topo, alg, seed=5) as sim:
        orc = oracle(n, topo, alg, 5)
        both_step(sim, orc, 20000, what)
        assert sim.alerts_total >= sim.threshold, "did not converge"
        m = check(sim, orc, what)
        assert m.converged > 0
        if alg == "push-sum":
            assert m.rms_error <= m.err_max * (1 + 1e-12) and m.est_min <= m.mean_estimate <= m.est_max
        orc.close()


def test_summary_argument_checks():
    from gossipprotocol_amd import Simulation
    from gossipprotocol_amd import _lib as L
    with Simulation(100, "line", "push-sum") as sim:
        out = L.GpSummary()
        take = sim._L.gp_summary_take
        assert take(sim._h, 1e-10, L.GP_SCOPE_LOCAL, C.byref(out)) == 0
        for tol in (-1e-300, -1.0, math.nan, math.inf, -math.inf):
            assert take(sim._h, tol, L.GP_SCOPE_LOCAL, C.byref(out)) == -1, tol
            assert b"tol" in sim._L.gp_last_error()
        for scope in (-1, 2, 7):
            assert take(sim._h, 1e-10, scope, C.byref(out)) == -1, scope
        assert take(sim._h, 1e-10, L.GP_SCOPE_LOCAL, None) == -1
        with pytest.raises(L.GossipError):
            sim.summary(tol=-1.0)
        with pytest.raises(ValueError):
            sim.summary(scope="world")
        assert sim.step(3) is not None and sim.summary().rounds == 3  # the handle is still good


# ---- halos and slab offsets: the arrays of a slab start at base = lo - halo

@pytest.fixture(scope="module")
def single_slab(oracle):
    """Per (n, topology): the single-slab summary and the oracle reference after 41 rounds, shared by
    the virtual-rank cases."""
    from gossipprotocol_amd import Simulation
    cache = {}

    def get(n, topo):
        if (n, topo) not in cache:
            orc = oracle(n, topo, "push-sum", 4)
            want = orc.step(41)
            ref = ref_summary(orc.state(), 0, orc.P, orc.rounds, 1, orc.seed_node, 1e-10)
            orc.close()
            with Simulation(n, topo, "push-sum", seed=4) as sim:
                assert sim.step(41) == want
                one = sim.summary(1e-10)
            assert_matches(one, ref, f"{topo} n={n} single slab")
            cache[(n, topo)] = (want, ref, one)
        return cache[(n, topo)]
    return get


@pytest.mark.parametrize("n,topo,vr", [(32768, "Imp3D", 2), (32768, "Imp3D", 3), (32768, "Imp3D", 8),
                                       (10**6, "Imp3D", 2), (10**6, "Imp3D", 3), (10**6, "Imp3D", 8),
                                       (4099, "line", 3)])
def test_summary_virtual_ranks(n, topo, vr, single_slab):
    from gossipprotocol_amd import Simulation
    want, ref, one = single_slab(n, topo)
    what = f"{topo} push-sum n={n} virtual_ranks={vr}"
    with Simulation(n, topo, "push-sum", seed=4, virtual_ranks=vr) as sim:
        m0 = sim.summary(1e-10)
        assert m0.rounds == 0 and field(m0, "sum_w") == [float(m0.count), 0.0]
        assert sim.step(41) == want
        m = sim.summary(1e-10)
        assert (m.first, m.count) == (0, sim.population)  # a virtual-rank handle owns every slab
        assert_same_exact(m, one, what)
        assert_matches(m, ref, what)
        assert raw(sim.summary(1e-10)) == raw(m)


def test_summary_does_not_disturb_the_run(oracle):
    """Summaries between every step: the following per-round alerts and the final state still equal the oracle's."""
    from gossipprotocol_amd import Simulation
    for n, topo, alg, vr in ((8000, "3D", "push-sum", 1), (4099, "full", "push-sum", 1), (27000, "Imp3D", "gossip", 1),
                             (32768, "Imp3D", "push-sum", 3)):
        with Simulation(n, topo, alg, seed=6, virtual_ranks=vr) as sim:
            orc = oracle(n, topo, alg, 6)
            for k in (1, 2, 5, 64, 7, 70):
                a, b = sim.summary(), sim.summary()
                assert raw(a) == raw(b)
                assert sim.step(k) == orc.step(k), f"{topo} {alg}: alerts differ after a summary"
            gs, os_ = sim.state(), orc.state()
            for k in ("c", "s", "w", "flags"):
                assert np.array_equal(gs[k], os_[k]), f"{topo} {alg}: state '{k}' differs after summaries"
            ref = ref_summary(os_, 0, orc.P, orc.rounds, ALG_ID[alg], orc.seed_node, 1e-10)
            assert_matches(sim.summary(), ref, f"{topo} {alg} n={n}")
            orc.close()


# ---- ensembles

def ensemble_case(n, topo, alg, seeds, oracle):
    from gossipprotocol_amd import Ensemble, Simulation
    what = f"ensemble {topo} {alg} n={n}"
    with Ensemble(n, topo, alg, seeds, max_rounds=200000) as ens:
        for phase in ("step", "run"):
            if phase == "step":
                ens.step(7)
            else:
                ens.run()
            recs = ens.members()
            sums = ens.summary(1e-10)
            assert len(sums) == len(seeds)
            again = ens.summary(1e-10)
            for m, (rec, got) in enumerate(zip(recs, sums)):
                assert raw(again[m]) == raw(got)
                assert (got.first, got.count, got.rounds) == (0, ens.population, rec.rounds)
                orc = oracle(n, topo, alg, seeds[m])
                orc.step(int(rec.rounds))
                ref = ref_summary(orc.state(), 0, orc.P, orc.rounds, ALG_ID[alg], orc.seed_node, 1e-10)
                orc.close()
                assert_matches(got, ref, f"{what} member {m} {phase}")
                with Simulation(n, topo, alg, seed=seeds[m]) as sim:
                    sim.step(int(rec.rounds))
                    one = sim.summary(1e-10)
                assert_same_exact(got, one, f"{what} member {m} {phase} vs Simulation")
                assert_matches(one, ref, f"{what} member {m} {phase} Simulation")
            dup = seeds.index(seeds[-1])
            assert raw(sums[dup]) == raw(sums[-1]), "duplicate seeds give identical summaries"


@pytest.mark.parametrize("n", [100, 1000])
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("topo", ["line", "full", "3D", "Imp3D"])
def test_ensemble_summary(topo, alg, n, oracle):
    ensemble_case(n, topo, alg, [11, 12, 13, 14, 15, 16, 17, 18, 12], oracle)


def test_ensemble_summary_at_the_cap(oracle):
    from gossipprotocol_amd import ensemble_max_nodes
    n = ensemble_max_nodes("Imp3D", "push-sum")
    assert n == 5832
    ensemble_case(n, "Imp3D", "push-sum", [21, 22, 21], oracle)
