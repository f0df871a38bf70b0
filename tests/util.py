"""Shared input generators for the parity tests (seeded, admissible Euler states)."""
import json
import os

import numpy as np


def euler_dg_state(shape, seed, amp=0.2):
    """u[..., 5]: smooth-ish random admissible state (rho, m0, m1, m2, E)."""
    rng = np.random.default_rng(seed)
    u = np.zeros(tuple(shape) + (5,))
    rho = 1.0 + amp * rng.random(shape)
    u[..., 0] = rho
    vel = [0.4 * rng.random(shape) - 0.2 for _ in range(3)]
    for a in range(3):
        u[..., 1 + a] = rho * vel[a]
    p = 1.0 + amp * rng.random(shape)
    u[..., 4] = p / 0.4 + 0.5 * rho * sum(v * v for v in vel)
    return u


def euler_ref2d_patches(n_patches, S, V, seed):
    """Q[n_patches, S, S, V] with (rho, rho u, rho v, E) in vars 0..3, noise elsewhere."""
    rng = np.random.default_rng(seed)
    sh = (n_patches, S, S)
    Q = rng.uniform(-1, 1, sh + (V,))
    rho = rng.uniform(0.5, 2.0, sh); u = rng.uniform(-1, 1, sh); v = rng.uniform(-1, 1, sh); p = rng.uniform(0.5, 2.0, sh)
    Q[..., 0] = rho; Q[..., 1] = rho * u; Q[..., 2] = rho * v; Q[..., 3] = p / 0.4 + 0.5 * rho * (u * u + v * v)
    return Q


def euler_patches(n_patches, dim, S, V, seed):
    rng = np.random.default_rng(seed)
    sh = (n_patches,) + (S,) * dim
    Q = rng.uniform(-1, 1, sh + (V,))
    Q[..., :5] = euler_dg_state(sh, seed + 1, amp=0.5)
    return Q


def rel_err(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


# ---- ADER-DG oracle comparisons: one step size, one error measure ----------------------------------------------------------------------------
# Every ADER-DG result is compared with its oracle at the step run() would take at CFL 0.9, per variable, relative to how far the oracle's
# result moved from its starting point (the increment).  At that step the last Picard iteration changes the result by far more than DG_TOL of
# the increment; a test that uses a smaller step, or divides by the whole state, cannot tell the last iterations apart (max|u| ~ 1 hides them).
DG_TOL = 1e-11
ADV_A = (1.0, 0.5, -0.75)                        # oracle/exa_oracle.c ADV_A: the built-in advection's velocity


def dg_max_eigenvalue(u, dim, pde=1, m=5):
    """max over nodes and directions of the PDE's eigenvalue bound (oracle.PDE_EULER = 1, PDE_ADVECTION = 2, or an object with maxeig(q, d))."""
    from oracle import aderdg_numpy as A
    if pde == 2:
        return max(abs(ADV_A[d]) for d in range(dim))
    p = A.Euler() if pde == 1 else pde
    q = np.asarray(u).reshape(-1, m)
    return float(max(np.max(p.maxeig(q, d)) for d in range(dim)))


def cfl_dt(u, dx, dim, N, cfl=0.9, pde=1, m=5, lam=None):
    """The step AderDgSolver.run takes at `cfl`: cfl * min(dx) / ((2N - 1) * dim * lambda_max)."""
    if lam is None:
        lam = dg_max_eigenvalue(u, dim, pde, m)
    return cfl * min(dx) / ((2 * N - 1) * dim * lam)


def dg_err(got, want, base, var_axis=-1):
    """max_v max|got_v - want_v| / inc_v with inc_v = max|want_v - base_v| (base None: max|want_v|), floored at 1e-3 of the largest inc_v."""
    got, want = np.moveaxis(np.asarray(got), var_axis, 0), np.moveaxis(np.asarray(want), var_axis, 0)
    m = want.shape[0]
    got, want = got.reshape(m, -1), want.reshape(m, -1)
    ref = np.zeros_like(want) if base is None else np.moveaxis(np.asarray(base), var_axis, 0).reshape(m, -1)
    inc = np.max(np.abs(want - ref), axis=1)
    inc = np.maximum(inc, 1e-3 * inc.max())
    assert inc.max() > 0, "dg_err: the oracle's result does not move"
    return float(np.max(np.max(np.abs(got - want), axis=1) / inc))


def assert_dg_parity(got, want, base, mutant=None, tol=DG_TOL, var_axis=-1, what=""):
    """got == want to `tol` of the per-variable increment, and to the old relative 1e-10 of max|want|; with a `mutant` (the oracle run with one
    Picard iteration less) the case must be able to see that iteration: dg_err(mutant) >= 100 * tol."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape or got.size == want.size, (what, got.shape, want.shape)
    got = got.reshape(want.shape)
    e = dg_err(got, want, base, var_axis)
    em = None if mutant is None else dg_err(np.asarray(mutant).reshape(want.shape), want, base, var_axis)
    msg = "%s: dg_err %.3e (tol %.0e), mutant %s" % (what, e, tol, "n/a" if em is None else "%.3e" % em)
    if os.environ.get("EXA_DG_ERR_LOG"):                    # measurement aid: one JSON line per comparison
        with open(os.environ["EXA_DG_ERR_LOG"], "a") as f:
            f.write(json.dumps(dict(test=os.environ.get("PYTEST_CURRENT_TEST", ""), what=what, err=e, mutant=em)) + "\n")
    assert e <= tol, msg
    assert rel_err(got, want) < 1e-10, msg + ", rel_err %.3e" % rel_err(got, want)
    assert em is None or em >= 100 * tol, msg + ": the case is blind to the last Picard iteration"
    return e, em


def assert_shard_equals_whole_block(got, whole, base, shard, block, what=""):
    """A shard's cells against the same cells of the un-sharded block stepped on the same GPU (`shard`, `block`: the two AderDgSolvers).  Stage A
    is per cell and stage B's arithmetic does not depend on where a neighbour's trace is read from (tests/test_stage_b_chain.py
    test_traversal_does_not_change_a_bit), so where the same stage-A kernel serves both the results are equal bit for bit; where the
    selector picks different kernels they agree to DG_TOL of the increment."""
    a, b = shard.stage_a_kernel_name(), block.stage_a_kernel_name()
    got, whole = np.asarray(got), np.asarray(whole)
    same = bool(np.array_equal(got, whole))
    if os.environ.get("EXA_DG_ERR_LOG"):
        with open(os.environ["EXA_DG_ERR_LOG"], "a") as f:
            f.write(json.dumps(dict(test=os.environ.get("PYTEST_CURRENT_TEST", ""), what=what + " == whole block", bit_equal=same,
                                    err=dg_err(got, whole, base), kernels=[a, b])) + "\n")
    if a == b:
        assert same, "%s: shard != whole block, dg_err %.3e (stage A %s)" % (what, dg_err(got, whole, base), a)
    else:
        print("%s: stage A of the shard is %s, of the whole block %s" % (what, a, b))
        assert_dg_parity(got, whole, base, what=what + " against the whole block")


def euler_supersonic_state(shape, seed):
    """Admissible Euler state with velocities up to +-2 and sound speed ~1.2: sub- and supersonic nodes, both flow directions, both
    eigenvalue branches |u_n - c| and |u_n + c| as the maximum."""
    rng = np.random.default_rng(seed)
    u = np.zeros(tuple(shape) + (5,))
    rho = 1.0 + 0.2 * rng.random(shape)
    vel = [4.0 * rng.random(shape) - 2.0 for _ in range(3)]
    p = 1.0 + 0.2 * rng.random(shape)                       # c = sqrt(1.4 p / rho) in [1.08, 1.30]
    u[..., 0] = rho
    for a in range(3):
        u[..., 1 + a] = rho * vel[a]
    u[..., 4] = p / 0.4 + 0.5 * rho * sum(v * v for v in vel)
    return u


def euler_scaled_state(shape, seed, scale):
    """euler_dg_state times `scale` (2^-20, 2^20): the same flow (Euler is homogeneous of degree 1), every conserved variable far from 1 --
    the device's fast reciprocal of rho sees values it was never measured on."""
    return euler_dg_state(shape, seed) * scale


def log_limiter_measurement(kind, **fields):
    """Measurement aid of tests/test_limiter_kernels.py, like EXA_DG_ERR_LOG above: with EXA_LIM_ERR_LOG=<file> every comparison appends one JSON line
    (kind: operators | projection | ghost | face_layers | reconstruction | round_trip; the largest error / bound ratio it saw)."""
    if os.environ.get("EXA_LIM_ERR_LOG"):
        with open(os.environ["EXA_LIM_ERR_LOG"], "a") as f:
            f.write(json.dumps(dict(kind=kind, test=os.environ.get("PYTEST_CURRENT_TEST", ""), **fields)) + "\n")


def log_fv_measurement(**fields):
    """Measurement aid of tests/test_fv_kernels_hp.py, like EXA_LIM_ERR_LOG above: with EXA_FV_ERR_LOG=<file> every comparison appends one JSON line
    (row, family, entry, the largest error / bound ratio it saw)."""
    if os.environ.get("EXA_FV_ERR_LOG"):
        with open(os.environ["EXA_FV_ERR_LOG"], "a") as f:
            f.write(json.dumps(dict(test=os.environ.get("PYTEST_CURRENT_TEST", ""), **fields)) + "\n")
