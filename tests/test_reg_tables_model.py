"""CPU: the lane-table model of the register-resident stage A (scripts/reg_tables.py) under the primitive image.

The table the library ships (dg_inst.hip fill_reg_tables, restated by reg_tables.library_table) is the parent's: the primitive image moves
every array of the sums by the same amount and takes one of the reads every lane makes at the same slot away, so what the table was built for
can only get cheaper.  New is the second read of the normal component, whose slot depends on the lane's direction: its modelled conflict cycles
are counted on their own, printed, and are all the step may cost more than the parent's.
"""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_model():
    spec = importlib.util.spec_from_file_location("reg_tables", os.path.join(ROOT, "scripts", "reg_tables.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_shipped_table_costs_no_more_than_the_parents_plus_the_normal_velocity_read():
    R = load_model()
    tab = R.library_table(2)
    assert sorted(t for t in tab if t is not None) == sorted((d, ls, t) for d in range(3) for ls in range(2) for t in range(36))
    parent, put = R.step_cost(tab, put=False), R.step_cost(tab, put=True)
    print("modelled extra LDS cycles per two-level step: parent image %s, primitive image %s; groups that mix directions %s"
          % (parent, put, R.mixed_groups(tab)))
    assert parent["vn"] == 0 and parent["total"] == parent["same"] + parent["wr"]
    assert put["total"] == put["same"] + put["wr"] + put["vn"]
    assert put["same"] + put["wr"] <= parent["total"]
    assert put["total"] <= parent["total"] + put["vn"]
    # the second read can only conflict where a 32-lane group holds pencils of several directions
    pure_only = [t if (k // 32) not in R.mixed_groups(tab) else None for k, t in enumerate(tab)]
    assert R.step_cost(pure_only, put=True)["vn"] == 0


def test_iteration_zero_table_holds_every_pencil_of_one_level_once():
    R = load_model()
    tab = R.library_table(1)
    assert sorted(t for t in tab if t is not None) == sorted((d, 0, t) for d in range(3) for t in range(36))
