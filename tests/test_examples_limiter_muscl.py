"""examples/sod_tube_limited_second_order.py at its tiny size: both modes run, the second-order update gives the smaller error."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sod_tube_limited_second_order.py"), "16", "4", "2"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    l1 = {m.group(1): float(m.group(2)) for m in re.finditer(r"^(\w+)\s.*L1\(rho\) = ([0-9.e+-]+)$", r.stdout, re.M)}
    assert set(l1) == {"rusanov", "muscl_hancock"}, r.stdout
    assert 0 < l1["muscl_hancock"] < l1["rusanov"] < 0.03, l1
