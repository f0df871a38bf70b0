"""The register-resident stage A (3-D, N = 6, built-in Euler) with the PRIMITIVE image: the node owners put the momenta, 1/rho, E + p and p into LDS (six values per node and level instead of seven), a pencil
task reads the normal component a second time from the slot of its own direction (exa_dg_reg.hpp StageAReg::PUT, exa_pde.hpp Euler::put_fast /
flux_scaled_put).  Everything through AderDgSolver(stage_a="reg") against oracle/exa_oracle.c, measure tests/util.py dg_err, bound 1e-10, on u*, the
traces and the stepped u.

Cases (cells):  (1, 1, 3)  one half of a workgroup idles through its last trip
                (2, 2, 3)  both halves, periodic wrap on every axis
                (3, 2, 2)  the same with another axis order
                (2, 2, 3)  as a box inside a (4, 3, 3) block: the box path (the rest of the block follows in three more box launches)
each with n_picard 6, 2 and 0 and anisotropic cells (the per-direction scale is a lane property).  (2, 2, 3) also runs the hard states of
tests/test_dg_hard_states.py, the step as one kernel (the FUSE instantiation shares the template) and a comparison with stage_a="lds".
"""
import functools

import numpy as np
import pytest

from tests import dg_cases as C
from tests.dg_cases import DgRef
from tests.util import cfl_dt, dg_err, euler_dg_state, rel_err

pytestmark = pytest.mark.gpu
N = 6
BOUND = 1e-10
WHOLE = [(1, 1, 3), (2, 2, 3), (3, 2, 2)]
BLOCK, BOX_LO, BOX_HI = (4, 3, 3), (1, 1, 0), (3, 3, 3)               # the (2, 2, 3) box
N_PICARD = [6, 2, 0]


@pytest.fixture(scope="module")
def exa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from exahype_amd import solvers
    return solvers


def dx_of(nc):
    return [1.0 / nc[0], 0.8 / nc[1], 1.3 / nc[2]]


@functools.lru_cache(maxsize=None)
def reference(nc, n_it):
    """input and oracle of a block (computed once, shared, never written)"""
    u = euler_dg_state(tuple(nc) + (N,) * 3, seed=6100 + 10 * sum(nc) + n_it)
    dx = dx_of(nc)
    dt = cfl_dt(u, dx, 3, N)
    return u, dx, dt, DgRef(u, dt, dx, 3, N, nc, n_it)


def errors(r, ustar, trace, unew, label):
    """dg_err of u*, traces (against their n_it = 0 part as DgRef.check_traces takes it) and the stepped u; printed before anything is asserted"""
    want_us, want_tr = r.stage_a()
    base_tr = r.stage_a(0)[1] if r.n_it > 0 else None
    e = {"u*": dg_err(np.asarray(ustar).reshape(-1, 5), want_us.reshape(-1, 5), r.u.reshape(-1, 5)),
         "traces": dg_err(np.asarray(trace).reshape(want_tr.shape), want_tr, base_tr, var_axis=4),
         "step": dg_err(np.asarray(unew).reshape(-1, 5), r.steps(1).reshape(-1, 5), r.u.reshape(-1, 5))}
    print("primitive put %s: " % (label,) + ", ".join("%s %.3e" % kv for kv in e.items()))
    return e


def run_whole(exa, r, u, dx, dt, nc, n_picard, **kw):
    s = exa.AderDgSolver(3, N, nc, n_picard=n_picard, dx=dx, stage_a="reg", **kw)
    s.upload(u)
    s.predictor_volume(dt)
    ustar, trace = s.download().copy(), s.trace.cpu().numpy().copy()
    s.upload(u)
    s.step(dt)
    return s, ustar, trace, s.download()


@pytest.mark.parametrize("n_picard", N_PICARD)
@pytest.mark.parametrize("nc", WHOLE)
def test_primitive_put_vs_oracle(exa, nc, n_picard):
    u, dx, dt, r = reference(nc, n_picard)
    s, ustar, trace, unew = run_whole(exa, r, u, dx, dt, nc, n_picard)
    if n_picard > 0:
        assert "reg" in s.stage_a_kernel_name()
    e = errors(r, ustar, trace, unew, (nc, n_picard))
    assert max(e.values()) < BOUND, e


@pytest.mark.parametrize("n_picard", N_PICARD)
def test_primitive_put_box_inside_a_block_vs_oracle(exa, n_picard):
    u, dx, dt, r = reference(BLOCK, n_picard)
    s = exa.AderDgSolver(3, N, BLOCK, n_picard=n_picard, dx=dx, stage_a="reg")
    s.upload(u)
    s.predictor_volume(dt, BOX_LO, BOX_HI)
    us = s.download().reshape(BLOCK + (N ** 3, 5))
    want = r.stage_a()[0].reshape(BLOCK + (N ** 3, 5))
    inside = np.zeros(BLOCK, dtype=bool)
    inside[tuple(slice(l, h) for l, h in zip(BOX_LO, BOX_HI))] = True
    assert inside.sum() == 12
    assert np.array_equal(us[~inside], u.reshape(us.shape)[~inside]), "the box launch wrote outside its box"
    e_box = dg_err(us[inside].reshape(-1, 5), want[inside].reshape(-1, 5), u.reshape(us.shape)[inside].reshape(-1, 5))
    print("primitive put box %s: u* inside the box %.3e" % (n_picard, e_box))
    # the rest of the block, box by box: then the traces are complete and stage B can run
    for lo, hi in (((0, 0, 0), (1, 3, 3)), ((3, 0, 0), (4, 3, 3)), ((1, 0, 0), (3, 1, 3))):
        s.predictor_volume(dt, lo, hi)
    ustar, trace = s.download().copy(), s.trace.cpu().numpy().copy()
    s.riemann_corrector(dt)
    e = errors(r, ustar, trace, s.download(), ("box", n_picard))
    assert e_box < BOUND, e_box
    assert max(e.values()) < BOUND, e


@pytest.mark.parametrize("family", ["supersonic", "tiny", "huge"])
def test_primitive_put_hard_states_vs_oracle(exa, family):
    from tests.test_dg_hard_states import hard_dt, hard_input
    nc = (2, 2, 3)
    u, dx = hard_input(3, N, nc, family)
    dt = hard_dt(u, dx, 3, N, family)
    r = DgRef(u, dt, dx, 3, N, nc, N)
    _, ustar, trace, unew = run_whole(exa, r, u, dx, dt, nc, N)
    e = errors(r, ustar, trace, unew, (family,))
    assert max(e.values()) < BOUND, e


@pytest.mark.parametrize("n_picard", [6, 2])
def test_primitive_put_one_kernel_step_vs_oracle(exa, n_picard):
    """[A] [B o A] B: the second step's launch is the FUSE instantiation"""
    nc = (2, 2, 3)
    u, dx, dt0, r = reference(nc, n_picard)
    dts = [C.steps_dt(dt0), 0.7 * C.steps_dt(dt0)]
    s = exa.AderDgSolver(3, N, nc, n_picard=n_picard, dx=dx, stage_a="reg", one_kernel_step=True)
    assert s._one_kernel
    s.upload(u)
    for d in dts:
        s.step(d)
    got = s.download()
    e = dg_err(got.reshape(-1, 5), r.steps(2, dts=dts).reshape(-1, 5), u.reshape(-1, 5))
    print("primitive put one-kernel step %s: 2 steps %.3e" % (n_picard, e))
    assert e < BOUND, e


def test_primitive_put_agrees_with_the_lds_kernel(exa):
    nc = (2, 2, 3)
    u, dx, dt, r = reference(nc, 6)
    out = {}
    for variant in ("reg", "lds"):
        s = exa.AderDgSolver(3, N, nc, n_picard=6, dx=dx, stage_a=variant)
        s.upload(u)
        s.predictor_volume(dt)
        out[variant] = (s.download().copy(), s.trace.cpu().numpy().copy())
    e_u, e_t = rel_err(out["reg"][0], out["lds"][0]), rel_err(out["reg"][1], out["lds"][1])
    print("primitive put reg against lds: u* %.3e, traces %.3e" % (e_u, e_t))
    assert e_u < 1e-12 and e_t < 1e-12, (e_u, e_t)
    assert not np.array_equal(out["reg"][0], u)
