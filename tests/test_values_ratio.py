"""CPU: ratio_moved on the states a value run can reach (SRS v1-V).

The division-free branch of ratio_moved (gp_device.hpp) was proved on the premise that every ratio
s / w stays below 2^32.  gp_set_values admits exactly the inputs that keep the premise
(x * 2^-32 < omega, omega in [2^-32, 2^32], x = 0 or >= 2^-64), so on every state reachable from
them the function must decide like the exact two-division test.  4.2e6 cases: nonnegative
combinations of admissible pairs halved 0..200 times, with ratios just below 2^32, weights at
both ends of their range, x at 2^-64 and 0, and moves around the 1e-10 edge.  A mismatch means the
admissible set is wrong -- the function is not to be touched.  Compiles a tiny host program with
hipcc, like tests/test_device_math.py."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def line(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("vr") / "values_ratio_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                           os.path.join(HERE, "helpers", "values_ratio_check.cpp")])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    print("\n".join(out))
    return [l for l in out if l.startswith("values_ratio")][0].split()


def test_ratio_moved_matches_the_exact_test_on_reachable_states(line):
    cases, fast, bad, refused = int(line[1]), int(line[3]), int(line[5]), int(line[7])
    assert cases >= 4000000
    assert refused == 0  # every pair the cases are built from passes the library's own rule
    assert bad == 0
    assert fast > cases // 10  # the shortcut does decide a share of them
