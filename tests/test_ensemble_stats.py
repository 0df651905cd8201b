"""CPU: tools/ensemble_stats.py -- its quantiles and its command line (no GPU needed)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ensemble_stats  # noqa: E402


def test_quantile_is_nearest_rank():
    vals = list(range(1, 102))  # 1..101
    assert ensemble_stats.quantile(vals, 0.5) == 51
    assert ensemble_stats.quantile(vals, 0.05) == 6
    assert ensemble_stats.quantile(vals, 0.95) == 96
    assert ensemble_stats.quantile([7], 0.95) == 7
    assert ensemble_stats.quantile([1, 9], 0.0) == 1 and ensemble_stats.quantile([1, 9], 1.0) == 9


def test_command_line_lists_its_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ensemble_stats.py"), "--help"],
                         capture_output=True, text=True)
    assert out.returncode == 0
    for opt in ("--nodes", "--seeds", "--sequential", "--out"):
        assert opt in out.stdout
