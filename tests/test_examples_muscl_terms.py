"""examples/advection_reaction_fv_second_order.py runs at a tiny size and does what it prints."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_advection_reaction_fv_second_order_example():
    spec = importlib.util.spec_from_file_location("advection_reaction_fv_second_order", os.path.join(ROOT, "examples", "advection_reaction_fv_second_order.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(4, 4, 0.1)
    for form in mod.FORMS:
        first, second = out[form, "rusanov"], out[form, "muscl_hancock"]
        assert first["steps"] == second["steps"] > 0
        assert 0 < second["l1"] < first["l1"]
    assert abs(out["flux", "muscl_hancock"]["l1"] / out["ncp", "muscl_hancock"]["l1"] - 1) < 1e-10
