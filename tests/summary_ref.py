"""Numpy reference of gp_summary (include/gossip_hip.h) and the comparison rules of the summary
tests (tests/test_summary_abi.py, tests/test_gpu_summary*.py).

ref_summary() restates every field from a node state as gp_read_state / the oracle report it.
Integer fields, min / max, err_max, err_max_node and within_tol are order-independent and
IEEE-exact, so they are compared for equality.  The three sums are double-doubles (hi, lo) of
non-negative terms:

  bound 1: hi is within 1 ulp of math.fsum of the same terms;
  bound 2: Fraction(hi) + Fraction(lo) is within 2^-70 (relative) of the exact rational sum.

Both are derived, not measured: without cancellation the double-double error is at most
n * 2^-105 of the total, i.e. 2^-73 for n <= 2^32; hi is the rounding of a value that close to the
exact sum (bound 1), and bound 2 keeps a factor of eight over it.
"""
import math
from fractions import Fraction

import numpy as np

EXACT_FIELDS = ("first", "count", "population", "rounds", "algorithm", "active", "converged", "c_hist", "c_max",
                "cnt_hist", "est_min", "est_max", "w_min", "w_max", "err_max", "err_max_node", "within_tol", "tol")
SUM_FIELDS = ("sum_s", "sum_w", "sum_sqerr")


def exact_sum(terms) -> Fraction:
    """The exact rational sum of an array of finite, non-negative doubles."""
    t = np.ascontiguousarray(terms, np.float64)
    if t.size == 0:
        return Fraction(0)
    assert np.all(np.isfinite(t)) and np.all(t >= 0)
    m, e = np.frexp(t)
    mi = np.ldexp(m, 53).astype(np.int64)  # exact: |m| < 1 has 53 bits
    e = e.astype(np.int64) - 53
    emin = int(e.min())
    total = 0
    for ue in np.unique(e):
        sel = mi[e == ue]
        part = (int((sel >> 26).sum()) << 26) + int((sel & ((1 << 26) - 1)).sum())
        total += part << (int(ue) - emin)
    return Fraction(total) * (Fraction(2) ** emin)


def dd_of(x: Fraction):
    """The double-double nearest the rational x."""
    hi = float(x)
    return hi, float(x - Fraction(hi))


def ref_summary(state, first, P, rounds, alg, seed_node, tol):
    """gp_summary of the ids [first, first + len) from their state {c, s, w, flags}.  Returns a dict of
    the exact fields plus 'terms': the three arrays the sums run over."""
    c, s, w, f = (np.asarray(state[k]) for k in ("c", "s", "w", "flags"))
    n = len(f)
    r = {"first": first, "count": n, "population": P, "rounds": rounds, "algorithm": alg,
         "active": int((f & 1).sum()), "converged": int(((f >> 1) & 1).sum()), "tol": tol,
         "c_hist": [0] * 12, "c_max": 0, "cnt_hist": [0] * 4, "est_min": 0.0, "est_max": 0.0, "w_min": 0.0,
         "w_max": 0.0, "err_max": 0.0, "err_max_node": 0, "within_tol": 0}
    zero = np.zeros(0)
    terms = {"sum_s": zero, "sum_w": zero, "sum_sqerr": zero}
    if alg == 0:
        r["c_hist"] = [int(v) for v in np.bincount(np.minimum(c, 11), minlength=12)]
        r["c_max"] = max(0, int(c.max()))
        if 0 <= seed_node - first < n and c[seed_node - first] <= 10:
            assert f[seed_node - first] & 1, "the seed node is active until it has heard the rumour 11 times"
    else:
        mu = (P - 1) / 2
        est = s / w
        e = est - mu
        ae = np.abs(e)
        r["cnt_hist"] = [int(v) for v in np.bincount((f >> 2) & 3, minlength=4)]
        r["est_min"], r["est_max"] = float(est.min()), float(est.max())
        r["w_min"], r["w_max"] = float(w.min()), float(w.max())
        r["err_max"] = float(ae.max())
        r["err_max_node"] = first + int(np.argmax(ae))  # first occurrence: the lowest id
        r["within_tol"] = int((ae <= tol).sum())
        terms = {"sum_s": s.astype(np.float64), "sum_w": w.astype(np.float64), "sum_sqerr": e * e}
    r["terms"] = terms
    return r


def field(m, k):
    v = getattr(m, k)
    return list(v) if hasattr(v, "__len__") else v


def bits(x):
    return np.float64(x).tobytes()


def assert_exact(got, ref, what=""):
    """Every exact field of the GpSummary `got` equals the reference's (doubles: the same bits)."""
    for k in EXACT_FIELDS:
        g, w = field(got, k), ref[k]
        if isinstance(w, float):
            assert bits(g) == bits(w), f"{what}: {k} = {g!r}, reference {w!r}"
        else:
            assert g == w, f"{what}: {k} = {g!r}, reference {w!r}"
    assert got.reserved == 0 and got.reserved2 == 0


def assert_sums(got, ref, what=""):
    """The two derived bounds on every double-double sum."""
    for k in SUM_FIELDS:
        hi, lo = field(got, k)
        t = ref["terms"][k]
        if t.size == 0:
            assert hi == 0.0 and lo == 0.0, f"{what}: {k} of a gossip summary is zero"
            continue
        fs = math.fsum(t.tolist())
        assert abs(hi - fs) <= math.ulp(fs), f"{what}: {k} hi = {hi!r}, fsum {fs!r}"
        exact = exact_sum(t)
        err = abs(Fraction(hi) + Fraction(lo) - exact)
        assert err <= exact / 2 ** 70, f"{what}: {k} (hi, lo) off by {float(err / exact) if exact else 0:.3e} relative"


def assert_matches(got, ref, what=""):
    assert_exact(got, ref, what)
    assert_sums(got, ref, what)


def assert_same_exact(a, b, what=""):
    """Two GpSummary records agree in every exact field."""
    for k in EXACT_FIELDS:
        x, y = field(a, k), field(b, k)
        if isinstance(x, float):
            assert bits(x) == bits(y), f"{what}: {k} {x!r} != {y!r}"
        else:
            assert x == y, f"{what}: {k} {x!r} != {y!r}"


def raw(m) -> bytes:
    import ctypes as C
    return C.string_at(C.addressof(m), C.sizeof(m))
