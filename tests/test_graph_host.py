"""CPU: gp_graph.hpp, the host-only graph code of SRS v1-G, through tests/helpers/graph_check.cpp.

The admissibility check (every rule refused with its node and its words, the lowest node first,
nothing read outside the arrays) and the transposed, deduplicated in-CSR (ascending, each sender
once, the right entry counts) on a star, a directed cycle, a graph with self-loops and duplicates
and the largest population.  A stand-alone program with its own main, built with the host compiler
and AddressSanitizer + UBSan where they link (plain otherwise): the arrays are exact-size heap
blocks, so a read past an end aborts the program.  No Python code runs under a sanitizer.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "helpers", "graph_check.cpp")


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path_factory.mktemp("graph_check") / "graph_check")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC]
    # (the runtimes linked statically, as tests/test_summary_abi.py does: the program runs directly)
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                                 "-fno-sanitize-recover=all"], capture_output=True)
    if san.returncode != 0:  # the sanitizer runtimes do not link here
        subprocess.check_call(base)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines(), san.returncode == 0


def test_every_check_passes(output):
    lines, sanitized = output
    print("sanitized" if sanitized else "plain build")
    last = lines[-1].split()
    assert last[:2] == ["graph_check", "ok"] and int(last[2]) > 50


def test_transposes_and_their_entry_counts(output):
    lines, _ = output
    t = [l for l in lines if l.startswith("transpose ")]
    assert t == ["transpose star(65): 128 out, 128 in", "transpose cycle(40): 40 out, 40 in",
                 "transpose loops and duplicates: 10 out, 7 in", "transpose reversal(8192): 8192 out, 8192 in"]


def test_every_rule_is_refused_once_at_least(output):
    lines, _ = output
    rules = {int(l.split("(")[1].split(")")[0]) for l in lines if l.startswith("refused (")}
    assert rules == {1, 2, 3, 4, 5, 6, 7}
