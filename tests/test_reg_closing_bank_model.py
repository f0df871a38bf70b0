"""CPU: the bank model of the closing phases' volume rounds (scripts/reg_tables.py volume_cost) for the two array strides of the closing image.

The closing image of the register-resident stage A moved into the arrays of the sums, whose stride is the odd level stride 217 instead of the 216
nodes of a cell: a volume task (v, t) starts v * 217 doubles into its array group instead of v * 216, one double-bank further per variable.  The
model must not charge the new stride more than the old one; both counts are printed (profiles/reg_kernel_closing_schedule.txt records them).
"""
from tests.test_reg_tables_model import load_model


def test_volume_rounds_cost_no_more_at_the_stride_of_the_sums():
    R = load_model()
    PY, PX, SL = R.library_geometry()
    assert (R.NN, SL) == (216, 217)
    old, new = R.volume_cost(R.NN), R.volume_cost(SL)
    print("modelled extra LDS cycles of the volume rounds per cell: stride %d %s, stride %d %s" % (R.NN, old, SL, new))
    for c in (old, new):
        assert c["total"] == c["rd"] + c["wr"] and c["rd"] >= 0 and c["wr"] >= 0
    assert new["total"] <= old["total"]
    # the figures DESIGN.md 4.1c and profiles/reg_kernel_closing_schedule.txt quote
    assert old == dict(rd=192, wr=60, total=252) and new == dict(rd=180, wr=54, total=234)


def test_volume_model_sees_a_stride_that_puts_every_variable_on_one_bank():
    """a stride of a multiple of 32 doubles stacks the five variables of a pencil position on one bank: the model must charge it"""
    R = load_model()
    assert R.volume_cost(224)["rd"] > R.volume_cost(217)["rd"]
