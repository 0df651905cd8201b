"""The box grid of the LDS-resident push-sum kernel (gp_block_plan.hpp), evaluated on the host.

block_plan is the one place that decides how k_ps_block (gp_block.hip) cuts a g^3 lattice into
boxes; the kernel then trusts its vmax / fmax / lds for every LDS and face-buffer index.  For
cus in {8, 64, 256, 304} and every g in 2..130 the plan's own invariants are checked against the
kernel's arithmetic restated here (floor splits g * i / n, the LDS layout), and for 256 CUs the
table of box-shape classes that tests/test_gpu_block_kernel.py runs on the GPU is pinned, so that
table cannot drift from the code.  CPU-only: compiles a tiny host program.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

CUS = (8, 64, 256, 304)
SIDES = range(2, 131)

# g -> (nbx, nby, nbz) on 256 CUs, None: no plan (the tile kernel runs).  The sides stand for the
# box-shape classes listed in DESIGN.md §3.5; tests/test_gpu_block_kernel.py imports this table.
PLANS_256 = {
    2: (1, 1, 1), 3: (1, 1, 1),   # one box: degree-3 corners only / one interior node
    16: (1, 1, 1),                # the largest single box: 4096 nodes, four full node slots
    17: (1, 1, 6),                # dz 2 and 3, uneven
    21: (1, 1, 11),               # dz 1 and 2 mixed (the one-node slab is the bottom layer, z = 0)
    29: (3, 3, 3),                # uneven on all three axes
    32: (1, 1, 32),               # dz = 1, fmax = 1024 = the workgroup, 32 boxes
    43: (1, 2, 43),               # dz = 1 with a y cut
    64: (1, 4, 64),               # dz = 1, fmax = 1024, 256 boxes: one per CU
    69: (1, 5, 35),               # dz 1 (z = 0 only) and 2, fmax 966, two node slots
    78: (1, 6, 39),               # dz = 2, fmax 1014, LDS 148 128 B
    104: (4, 7, 8),               # fifth node slot, LDS 151 404 B
    105: (5, 7, 7),               # the last planned side
    106: None,
}
DZ1_256 = (21, 31, 32, 37, 39, 43, 44, 49, 53, 54, 61, 62, 63, 64, 69)  # slabs one node thick
DZ2_256 = (17, 22, 25, 26, 38, 50, 52, 56, 70, 71, 76, 78)              # thinnest box two nodes


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None) \
        or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path_factory.mktemp("bp") / "block_plan_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "helpers", "block_plan_check.cpp")])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    table, consts = {}, None
    for line in out:
        f = line.split()
        if f[0] == "P":
            table[(int(f[1]), int(f[2]))] = None if f[3] == "none" else tuple(map(int, f[3:]))
        elif f[0] == "K":
            consts = tuple(map(int, f[1:]))
    assert consts is not None and len(table) == len(CUS) * len(SIDES)
    return table, consts


def extents(g, n):
    """The kernel's cut of [0, g) into n boxes: box i is [g * i // n, g * (i + 1) // n)."""
    cuts = [g * i // n for i in range(n + 1)]
    return cuts, [b - a for a, b in zip(cuts, cuts[1:])]


def align4(x):
    return (x + 3) & ~3


def test_constants(plans):
    threads, npt, lds_max = plans[1]
    assert (threads, npt, lds_max) == (1024, 5, 150 * 1024)


@pytest.mark.parametrize("cus", CUS)
def test_plan_invariants(plans, cus):
    table, (threads, npt, lds_max) = plans
    planned = 0
    for g in SIDES:
        p = table[(cus, g)]
        if p is None:
            continue
        planned += 1
        nbx, nby, nbz, vmax, fmax, lds = p
        assert nbx * nby * nbz <= cus, (g, p)
        assert 1 <= nbx <= g and 1 <= nby <= g and 1 <= nbz <= g, (g, p)
        d = []
        for n in (nbx, nby, nbz):
            cuts, ext = extents(g, n)
            assert cuts[0] == 0 and cuts[-1] == g and min(ext) >= 1 and sum(ext) == g, (g, n)
            assert max(ext) <= 1023  # box coordinates are packed in 10 bits each
            d.append(max(ext))
        assert vmax == d[0] * d[1] * d[2], (g, p)
        assert fmax == max(d[1] * d[2], d[0] * d[2], d[0] * d[1]), (g, p)
        assert vmax <= npt * threads == 5 * 1024, (g, p)
        ns = vmax + 6 * fmax
        assert lds == 16 * (ns + 1) + align4(ns + 1) + align4(vmax) + 4 * vmax + 64, (g, p)
        assert lds <= lds_max == 150 * 1024, (g, p)
    assert planned >= 7  # g = 2..8 fit one box on any device


def thinnest(g, p):
    return min(min(extents(g, n)[1]) for n in p[:3])


def test_shape_classes_on_256_cus(plans):
    """The table the GPU test runs, and the classes its sides stand for."""
    table, _ = plans
    for g, want in PLANS_256.items():
        p = table[(256, g)]
        assert (None if p is None else p[:3]) == want, (g, p)
    assert table[(256, 105)] is not None and table[(256, 106)] is None
    assert all(table[(256, g)] is None for g in range(106, 131))
    assert all(table[(256, g)] is not None for g in range(2, 106))
    assert [g for g in range(2, 106) if table[(256, g)][:3] == (1, 1, 1)] == list(range(2, 17))
    # every side whose thinnest box is one / two nodes thick
    assert tuple(g for g in range(2, 106) if table[(256, g)][:3] != (1, 1, 1) and thinnest(g, table[(256, g)]) == 1) == DZ1_256
    assert tuple(g for g in range(2, 106) if table[(256, g)][:3] != (1, 1, 1) and thinnest(g, table[(256, g)]) == 2) == DZ2_256
    # where the one-node slabs lie: at 21 and 69 only the layer z = 0 (no z - 1 neighbour there),
    # at 32, 43 and 64 every slab (interior nodes with both z neighbours in halos)
    for g in (21, 69):
        ext = extents(g, table[(256, g)][2])[1]
        assert ext[0] == 1 and set(ext[1:]) == {2}, (g, ext)
    for g in (32, 43, 64):
        assert set(extents(g, table[(256, g)][2])[1]) == {1}
    # a face exactly as large as the workgroup; faces above 960 entries with two node slots
    assert table[(256, 32)][3:5] == (1024, 1024) and table[(256, 64)][3:5] == (1024, 1024)
    assert [table[(256, g)][4] for g in (69, 70, 76, 78)] == [966, 980, 988, 1014]
    assert all(1024 < table[(256, g)][3] <= 2048 for g in (69, 70, 76, 78))
    # LDS next to the limit, the fifth node slot
    assert table[(256, 78)][5] == 148128
    assert table[(256, 103)] == table[(256, 104)] == (4, 7, 8, 5070, 390, 151404)
    assert table[(256, 16)][3] == 4096 and table[(256, 104)][3] > 4096
