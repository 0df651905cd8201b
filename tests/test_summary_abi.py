"""CPU tests of the state-summary boundary (include/gossip_hip.h: gp_summary, gp_summary_take,
gp_summary_merge, gp_ensemble_summary): the struct's layout, the argument checks that need no
GPU, and the join of two summaries against the numpy reference over oracle states.  The kernel
itself is tested on the GPU (tests/test_gpu_summary.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gossipprotocol_amd import _lib as L
from tests.summary_ref import (SUM_FIELDS, assert_matches, dd_of, exact_sum, field, ref_summary)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10

SCALARS = ("first", "count", "population", "rounds", "algorithm", "reserved", "active", "converged", "c_max",
           "reserved2", "est_min", "est_max", "w_min", "w_max", "err_max", "err_max_node", "within_tol", "tol")
ARRAYS = ("c_hist", "cnt_hist", "sum_s", "sum_w", "sum_sqerr")


def test_struct_layout_matches_c(tmp_path):
    """GpSummary is blittable and matches the C layout: size and the offset of every field."""
    names = [n for n, _ in L.GpSummary._fields_]
    assert sorted(names) == sorted(SCALARS + ARRAYS)
    fmt = " ".join(["%zu"] * (len(names) + 1))
    args = ", ".join(["sizeof(gp_summary)"] + [f"offsetof(gp_summary, {n})" for n in names])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gossip_hip.h"\n'
                   f'int main(void){{printf("{fmt}\\n", {args});return 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    assert got == [C.sizeof(L.GpSummary)] + [getattr(L.GpSummary, n).offset for n in names]
    assert got[0] == 304
    assert (L.GP_SCOPE_LOCAL, L.GP_SCOPE_GLOBAL) == (0, 1)


def test_null_arguments_are_einval():
    lib = L.lib()
    out = L.GpSummary()
    assert lib.gp_summary_take(None, TOL, L.GP_SCOPE_LOCAL, C.byref(out)) == -1
    assert b"gp_summary_take" in lib.gp_last_error()
    fake = C.c_void_p(1)  # never dereferenced: the null output is refused first
    assert lib.gp_summary_take(fake, TOL, L.GP_SCOPE_LOCAL, None) == -1
    assert lib.gp_ensemble_summary(None, TOL, C.byref(out)) == -1
    assert lib.gp_ensemble_summary(fake, TOL, None) == -1
    assert lib.gp_summary_merge(None, C.byref(out), C.byref(out)) == -1
    assert lib.gp_summary_merge(C.byref(out), None, C.byref(out)) == -1
    assert lib.gp_summary_merge(C.byref(out), C.byref(out), None) == -1
    assert b"gp_summary_merge" in lib.gp_last_error()


def to_struct(ref) -> L.GpSummary:
    """The reference as a GpSummary, its sums as the double-doubles nearest the exact sums."""
    m = L.GpSummary()
    for k in SCALARS:
        if k in ref:
            setattr(m, k, ref[k])
    for k in ("c_hist", "cnt_hist"):
        for i, v in enumerate(ref[k]):
            getattr(m, k)[i] = v
    for k in SUM_FIELDS:
        hi, lo = dd_of(exact_sum(ref["terms"][k]))
        getattr(m, k)[0], getattr(m, k)[1] = hi, lo
    return m


def part(state, a, b):
    return {k: v[a:b] for k, v in state.items()}


@pytest.fixture(scope="module")
def oracle_states(oracle):
    """(state, P, rounds, algorithm, seed_node) of the two oracle runs the merge cases share."""
    out = {}
    for name, (n, topo, alg, rounds) in {"push-sum": (1000, "line", "push-sum", 50),
                                         "gossip": (1000, "Imp3D", "gossip", 200)}.items():
        o = oracle(n, topo, alg, 1)
        o.step(rounds)
        out[name] = (o.state(), o.P, o.rounds, 1 if alg == "push-sum" else 0, o.seed_node)
        o.close()
    return out


@pytest.mark.parametrize("name", ["push-sum", "gossip"])
@pytest.mark.parametrize("cut", [1, 333, -1])
def test_merge_of_halves_matches_reference(oracle_states, name, cut):
    state, P, rounds, alg, seed = oracle_states[name]
    cut = cut % P
    a = to_struct(ref_summary(part(state, 0, cut), 0, P, rounds, alg, seed, TOL))
    b = to_struct(ref_summary(part(state, cut, P), cut, P, rounds, alg, seed, TOL))
    whole = ref_summary(state, 0, P, rounds, alg, seed, TOL)
    if alg == 1:
        assert whole["active"] > 0 and whole["err_max"] > 0  # the state is a run's, not the initial one
    else:
        assert whole["c_hist"][0] < P and whole["c_max"] >= 1
    out = L.GpSummary()
    assert L.lib().gp_summary_merge(C.byref(a), C.byref(b), C.byref(out)) == 0
    assert_matches(out, whole, f"{name} cut at {cut}")
    assert_matches(a.merge(b), whole, "GpSummary.merge")
    # three pieces, joined left to right
    if 1 < cut < P - 1:
        mid = (cut + P) // 2
        b1 = to_struct(ref_summary(part(state, cut, mid), cut, P, rounds, alg, seed, TOL))
        b2 = to_struct(ref_summary(part(state, mid, P), mid, P, rounds, alg, seed, TOL))
        assert_matches(a.merge(b1).merge(b2), whole, "three pieces")


def test_merge_refuses_what_does_not_join(oracle_states):
    state, P, rounds, alg, seed = oracle_states["push-sum"]
    lib = L.lib()
    a = to_struct(ref_summary(part(state, 0, 400), 0, P, rounds, alg, seed, TOL))
    b = to_struct(ref_summary(part(state, 400, P), 400, P, rounds, alg, seed, TOL))
    out = L.GpSummary()
    assert lib.gp_summary_merge(C.byref(a), C.byref(b), C.byref(out)) == 0
    assert lib.gp_summary_merge(C.byref(b), C.byref(a), C.byref(out)) == -1  # the wrong order
    gap = to_struct(ref_summary(part(state, 401, P), 401, P, rounds, alg, seed, TOL))
    assert lib.gp_summary_merge(C.byref(a), C.byref(gap), C.byref(out)) == -1
    assert b"adjacent" in lib.gp_last_error()
    lap = to_struct(ref_summary(part(state, 399, P), 399, P, rounds, alg, seed, TOL))
    assert lib.gp_summary_merge(C.byref(a), C.byref(lap), C.byref(out)) == -1
    for k, v in (("population", P + 1), ("rounds", rounds + 1), ("algorithm", 0), ("tol", 2 * TOL)):
        bad = to_struct(ref_summary(part(state, 400, P), 400, P, rounds, alg, seed, TOL))
        setattr(bad, k, v)
        assert lib.gp_summary_merge(C.byref(a), C.byref(bad), C.byref(out)) == -1, k
    with pytest.raises(L.GossipError):
        b.merge(a)


@pytest.mark.parametrize("lo_id,hi_id", [(3, 60), (0, 99), (39, 40)])
def test_merge_tie_goes_to_the_lower_id(lo_id, hi_id):
    """Two nodes with the same |e|, one in each half (one above the average, one below): the lower id."""
    P, cut = 100, 40
    mu = (P - 1) / 2
    for sign in (1.0, -1.0):
        s = np.full(P, mu)
        s[lo_id] = mu + sign * 2.0
        s[hi_id] = mu - sign * 2.0
        state = {"c": np.zeros(P, np.int32), "s": s, "w": np.ones(P), "flags": np.full(P, 1 | (2 << 2), np.uint8)}
        a = to_struct(ref_summary(part(state, 0, cut), 0, P, 9, 1, 0, TOL))
        b = to_struct(ref_summary(part(state, cut, P), cut, P, 9, 1, 0, TOL))
        assert (a.err_max, a.err_max_node, b.err_max, b.err_max_node) == (2.0, lo_id, 2.0, hi_id)
        out = a.merge(b)
        assert (out.err_max, out.err_max_node) == (2.0, lo_id)
        assert_matches(out, ref_summary(state, 0, P, 9, 1, 0, TOL), "tie")
        assert field(out, "cnt_hist") == [0, 0, P, 0] and out.within_tol == P - 2


def test_standalone_host_program_under_sanitizers(tmp_path):
    """gp_summary.hpp is host-only C++: a program with its own main includes it, is built with
    AddressSanitizer and UBSan, and runs directly (no library, no Python, nothing preloaded)."""
    exe = tmp_path / "summary_merge_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "helpers", "summary_merge_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "summary_merge_check ok" in r.stdout
