"""examples/sod_tube_fv_second_order.py runs at a tiny size and does what it prints."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_sod_tube_fv_second_order_example():
    spec = importlib.util.spec_from_file_location("sod_tube_fv_second_order", os.path.join(ROOT, "examples", "sod_tube_fv_second_order.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(16, 4, 0.05)
    first, second = out["rusanov"], out["muscl_hancock"]
    assert second["min_rho"] >= 0.125 - 1e-12 and second["min_p"] >= 0.1 - 1e-12
    assert 0 < second["l1"] < first["l1"]
