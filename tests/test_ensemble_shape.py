"""The ensemble launch shape (gossipprotocol_amd/csrc/gp_ensemble_shape.hpp), evaluated on the host,
against its Python mirror (tests/ensemble_shape_ref.py).

tests/test_gpu_ensemble_slots.py derives from the mirror which push-sum instantiation a population
reaches, the workgroup size and the slot of a node, and asserts from the oracle that every slot and
slot boundary is touched.  Here the header itself, compiled with the host compiler into
tests/helpers/ensemble_shape_check.cpp, gets every population from 2 to 8192 and must give what the
mirror gives; and the shapes the GPU module is built around are stated literally.  CPU-only:
compiles a small host program.
"""
import os
import shutil
import subprocess

import pytest

from tests import ensemble_shape_ref as sh

HERE = os.path.dirname(os.path.abspath(__file__))
PMAX = sh.ENS_THREADS * sh.ENS_NPT_MAX
VARIANTS = [(f, t) for f in (False, True) for t in (False, True)]


@pytest.fixture(scope="module")
def shape(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path_factory.mktemp("ens_shape") / "ensemble_shape_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-o", exe,
                           os.path.join(HERE, "helpers", "ensemble_shape_check.cpp")])

    def ask(queries):
        """One list of integers per query."""
        text = "".join(" ".join([q[0]] + [str(int(x)) for x in q[1:]]) + "\n" for q in queries)
        out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(queries)
        res = []
        for q, line in zip(queries, out):
            name, _, rest = line.partition(" ")
            assert name == q[0] and rest.strip() != "?", line
            res.append([int(x) for x in rest.split()])
        return res
    return ask


def test_constants(shape):
    assert shape([("K",)]) == [[sh.ENS_THREADS, sh.ENS_NPT_MAX, sh.ENS_LDS_MAX, sh.ENS_LDS_HDR, sh.ENS_LDS_TRACE]]
    assert (sh.ENS_THREADS, sh.ENS_NPT_MAX) == (1024, 8)


@pytest.mark.parametrize("alg", ("gossip", "push-sum"))
def test_npt_and_threads_of_every_population(shape, alg):
    (got,) = shape([("range", sh.ALG[alg], 2, PMAX)])
    want = []
    for P in range(2, PMAX + 1):
        want += [sh.npt(P) if alg == "push-sum" else 1, sh.threads(alg, P)]
    assert got == want
    for P in range(2, PMAX + 1):  # what the kernels rely on: whole waves, a slot or a pass for every node
        t = sh.threads(alg, P)
        assert t % 64 == 0 and 64 <= t <= sh.ENS_THREADS
        assert sh.slots(alg, P) * t >= P > (sh.slots(alg, P) - 1) * t
        assert sh.slot_of(P - 1, alg, P) == sh.slots(alg, P) - 1 and sh.slot_of(0, alg, P) == 0
        if alg == "push-sum":
            assert sh.npt(P) in (1, 2, 4, 8)


# P, push-sum npt, push-sum threads: the sizes the GPU module is built around
TABLE = [(1024, 1, 1024),  # last single-slot size
         (1025, 2, 576),   # slot 1 holds 449 nodes
         (2048, 2, 1024),
         (2049, 4, 576),
         (4096, 4, 1024),
         (4097, 8, 576),
         (1331, 2, 704),   # g = 11
         (2197, 4, 576),   # g = 13
         (4096, 4, 1024),  # g = 16: every slot full
         (4913, 8, 640)]   # g = 17


@pytest.mark.parametrize("P,npt,threads", TABLE)
def test_push_sum_table(shape, P, npt, threads):
    assert (sh.npt(P), sh.threads("push-sum", P)) == (npt, threads)
    for topo in sh.TOPO:
        for f, t in VARIANTS:
            (got,) = shape([("shape", sh.TOPO[topo], sh.ALG["push-sum"], P, f, t)])
            assert got == [npt, threads, sh.lds_bytes(topo, "push-sum", P, f, t)]
    assert sh.boundaries("push-sum", P) == list(range(threads, P, threads)) and len(sh.boundaries("push-sum", P)) == npt - 1


def test_slot_1_of_1025_holds_449_nodes():
    assert sum(sh.slot_of(i, "push-sum", 1025) == 1 for i in range(1025)) == 449
    assert sh.slot_of(575, "push-sum", 1025) == 0 and sh.slot_of(576, "push-sum", 1025) == 1


def test_gossip_threads(shape):
    for P in (2, 64, 65, 1000, 1024, 1025, 2048, 2049, 2050, 2197, 4913, PMAX):
        want = min(1024, sh.up64(P))
        assert sh.threads("gossip", P) == want
        (got,) = shape([("shape", sh.TOPO["line"], sh.ALG["gossip"], P, 0, 0)])
        assert got[:2] == [1, want]
    # P = 1025: the second pass of the strided loops has thread 0 only
    assert [i for i in range(1025) if sh.slot_of(i, "gossip", 1025) == 1] == [1024]


def test_lds_bytes_and_caps(shape):
    q, want = [], []
    for topo in sh.TOPO:
        for alg in sh.ALG:
            for f, t in VARIANTS:
                q.append(("cap", sh.TOPO[topo], sh.ALG[alg], f, t))
                P = sh.max_population(topo, alg, f, t)
                g = round(P ** (1 / 3))
                g = g if g ** 3 <= P else g - 1
                want.append([P, P - 1 if topo in ("line", "full") else g ** 3])
                for P in (2, 31, 32, 33, 1025, 2049, 2050, 2197, P):
                    q.append(("shape", sh.TOPO[topo], sh.ALG[alg], P, f, t))
                    want.append([sh.npt(P) if alg == "push-sum" else 1, sh.threads(alg, P),
                                 sh.lds_bytes(topo, alg, P, f, t)])
    assert shape(q) == want
    assert sh.max_population("Imp3D", "push-sum") >= 4913  # Imp3D push-sum's cap admits g = 11, 13, 16, 17


def test_injector_words():
    # the rank-select of the injector: W words per lane of wave 0, 1 -> 2 at T = 2048 -> 2049
    assert [sh.inject_words(T) for T in (2047, 2048, 2049, 2197)] == [(64, 1), (64, 1), (65, 2), (69, 2)]
    assert 2047 % 32 == 31  # the last word of T = 2047 has 31 bits
