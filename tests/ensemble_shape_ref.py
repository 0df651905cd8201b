"""Python mirror of the ensemble launch shape (gossipprotocol_amd/csrc/gp_ensemble_shape.hpp).

TEST INFRASTRUCTURE: the GPU tests derive from it which push-sum instantiation a population
reaches (npt node slots per thread), the workgroup size and the slot a node sits in, so that they
can assert from the reference alone that a case touches every slot and every slot boundary.
tests/test_ensemble_shape.py holds it against the header itself, compiled with the host compiler,
for every population up to the largest one.
"""
from __future__ import annotations

ENS_THREADS = 1024
ENS_NPT_MAX = 8
ENS_LDS_MAX = 150 * 1024
ENS_LDS_HDR = 16
ENS_LDS_TRACE = 32
TOPO = {"line": 0, "full": 1, "3D": 2, "Imp3D": 3}
ALG = {"gossip": 0, "push-sum": 1}


def up8(b):
    return (b + 7) & ~7


def up64(p):
    return (p + 63) & ~63


def npt(P):
    """Push-sum: node slots per thread, the smallest power of two with npt * 1024 >= P."""
    k = 1
    while k * ENS_THREADS < P:
        k *= 2
    return k


def threads(alg, P):
    """The workgroup: whole waves for one node a thread per slot (push-sum) or per pass (gossip)."""
    per = -(-P // npt(P)) if alg == "push-sum" else P
    return min(ENS_THREADS, up64(per))


def slots(alg, P):
    """Push-sum: the slots a thread keeps; gossip: the passes of the strided loops."""
    return npt(P) if alg == "push-sum" else -(-P // threads(alg, P))


def slot_of(node, alg, P):
    """Thread t keeps (or, gossip, visits in pass q) node t + q * threads: the q of a node."""
    return node // threads(alg, P)


def boundaries(alg, P):
    """The first node of every slot but slot 0: b = q * threads < P."""
    t = threads(alg, P)
    return list(range(t, P, t))


def lds_bytes(topo, alg, P, faults=False, trace=False):
    b = ENS_LDS_HDR
    if alg == "gossip":
        b += up8(4 * P) * 2
        if topo == "Imp3D":
            b += up8(2 * P)
        if topo != "full":
            b += up8(4 * ((P + 31) // 32))
    else:
        b += 8 * P * 2
        if topo in ("full", "Imp3D"):
            b += up8(4 * P) + up8(2 * P)
        if topo == "Imp3D":
            b += up8(2 * P)
        if topo != "full":
            b += up8(P)
    if faults:
        b += up8(4 * ((P + 31) // 32))
    if trace:
        b += ENS_LDS_TRACE
    return b


def max_population(topo, alg, faults=False, trace=False):
    P = ENS_THREADS * ENS_NPT_MAX
    while P > 2 and lds_bytes(topo, alg, P, faults, trace) > ENS_LDS_MAX:
        P -= 1
    return P


def inject_words(T):
    """Gossip, not full: (nwords, W) -- the injector's live bitmap words and the words a lane of wave 0 counts."""
    nwords = (T + 31) // 32
    return nwords, (nwords + 63) // 64
