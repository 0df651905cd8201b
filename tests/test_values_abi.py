"""CPU tests of the values boundary (gp_set_values, gp_set_mean, gp_ensemble_create_values;
include/gossip_hip.h, SRS v1-V): the symbols exist, gp_values matches its C layout, the version did
not move, and every host-only refusal answers before any HIP call (so it works without a GPU)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from gossipprotocol_amd import Values, default_mean
from gossipprotocol_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gp_set_values", "gp_set_mean", "gp_ensemble_create_values")
GP_EINVAL, GP_ENODEV = -1, -6


def test_library_exports_the_symbols():
    raw = C.CDLL(L.LIB_PATH)
    bound = {n for n, _, _ in L.SIGNATURES}
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in bound, n
    assert L.lib().gp_version() == 10100  # the ABI grew, the version did not move


def test_struct_layout_matches_c(tmp_path):
    src = tmp_path / "values.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gossip_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(gp_values), offsetof(gp_values, x), offsetof(gp_values, w),'
                   'offsetof(gp_values, count), offsetof(gp_values, mean), offsetof(gp_values, reserved));'
                   'printf("%d\\n", (int)GP_VERSION);return 0;}\n')
    exe = tmp_path / "values"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    V = L.GpValues
    assert got == [C.sizeof(V), V.x.offset, V.w.offset, V.count.offset, V.mean.offset, V.reserved.offset, 10100]
    assert C.sizeof(V) == 40


def _create(n=100, topo=L.GP_3D, alg=L.GP_PUSHSUM, values="default", count=None, mean=62.0, reserved=0, x_null=False,
            faults=None, trace=None, seeds=(1, 2), max_rounds=1000):
    cfg = L.GpConfig()
    cfg.num_nodes, cfg.topology, cfg.algorithm = n, topo, alg
    cfg.num_gpus, cfg.device, cfg.max_rounds = 1, 0, max_rounds
    P = C.c_int64()
    T, g = C.c_int64(), C.c_int64()
    L.lib().gp_resolve(max(1, n), topo if 0 <= topo <= 3 else 0, C.byref(P), C.byref(T), C.byref(g))
    x = np.arange(P.value, dtype=np.float64) * 0.1
    dp = C.POINTER(C.c_double)
    v = None
    if values is not None:
        v = C.byref(L.GpValues(None if x_null else x.ctypes.data_as(dp), None, P.value if count is None else count,
                               mean, reserved))
    arr = (C.c_uint64 * len(seeds))(*seeds)
    f = None if faults is None else C.byref(L.GpFaults(*faults))
    t = None if trace is None else C.byref(L.GpTraceCfg(*trace))
    h = C.c_void_p()
    rc = L.lib().gp_ensemble_create_values(C.byref(cfg), v, f, t, arr, len(seeds), C.byref(h))
    if rc == 0:  # (a GPU is present and the arguments were fine)
        L.lib().gp_ensemble_destroy(h)
    return rc, L.lib().gp_last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(values=None), b"values is null"),
    (dict(x_null=True), b"values.x"),
    (dict(count=124), b"count"),
    (dict(count=126), b"count"),
    (dict(count=0), b"count"),
    (dict(reserved=1), b"reserved"),
    (dict(mean=math.nan), b"mean"),
    (dict(mean=math.inf), b"mean"),
    (dict(mean=-1.0), b"mean"),
    (dict(mean=2.0 ** 32), b"mean"),
    (dict(alg=L.GP_GOSSIP), b"gossip"),
    # every check of the other create calls still applies
    (dict(faults=(1.5, 0.0, 0, 0)), b"node_fail"),
    (dict(trace=(0, 0)), b"stride"),
    (dict(max_rounds=0), b"max_rounds"),
    (dict(topo=7), b"topology"),
    (dict(n=10 ** 6, count=10 ** 6), b"cap"),
])
def test_create_refuses_bad_arguments_on_the_host(kw, word):
    rc, msg = _create(**kw)
    assert rc == GP_EINVAL, (kw, rc, msg)
    assert word in msg, msg


def test_create_accepts_good_arguments():
    for kw in (dict(), dict(mean=0.0), dict(mean=math.nextafter(2.0 ** 32, 0.0)), dict(faults=(0.1, 0.05, 3, 0), trace=(1, 0))):
        rc, msg = _create(**kw)
        assert rc in (0, GP_ENODEV), (kw, rc, msg)  # refused, if at all, for the missing GPU


def test_null_handles():
    lib = L.lib()
    x = (C.c_double * 1)(1.0)
    assert lib.gp_set_values(None, 0, 1, x, None) == GP_EINVAL
    assert lib.gp_set_mean(None, 1.0) == GP_EINVAL


def test_python_values():
    x, w = [0.1 * (i + 1) for i in range(9)], [1.0 + i for i in range(9)]
    v = Values(x)
    assert v.w is None and v.mean == math.fsum(x) / 9 == default_mean(x)
    v = Values(x, w)
    assert v.mean == math.fsum(x) / math.fsum(w) and "weighted" in repr(v)
    assert Values(x, mean=3.0).mean == 3.0
    with pytest.raises(ValueError):
        Values(x, w[:3])
