"""ADER-DG case tables and input builders shared by the GPU parity tests and their CPU check (tests/test_dg_reference_hp.py).

Every case runs at the CFL-0.9 step (tests/util.py cfl_dt; runs of several steps at STEPS_CFL below) and is compared with
oracle/exa_oracle.c through `DgRef`, which also runs the oracle with one Picard iteration less (the mutant): a case whose mutant does not differ by 100 * DG_TOL cannot see the last iteration, and
its check fails -- on the CPU, for every table here, without a GPU.
"""
import numpy as np

from tests.util import assert_dg_parity, cfl_dt, euler_dg_state

PDE_EULER, PDE_ADVECTION = 1, 2          # oracle.PDE_*
# Runs of several steps take the CFL-0.6 step: at CFL 0.9 the node-wise random states of these tables blow up by the third step (max|u| ~ 1e38
# in the oracle itself; a 1e-15 perturbation of u grows to 1e-4 of the increment), so two correct fp64 runs no longer agree.  One step (u*,
# traces, stage B, one full step) stays at CFL 0.9.  The single-stage scheme (no predictor: forward Euler in time) runs several steps at CFL
# 0.3: at 0.6 a 1e-16 perturbation of u grows to 1.6e-11 of the increment in three steps on the 100 x 91 grid at N = 8.
STEPS_CFL, SINGLE_STAGE_STEPS_CFL = 0.6, 0.3


def steps_dt(dt, single_stage=False):
    """The step for runs of several steps, from the CFL-0.9 one (same maximum eigenvalue)."""
    return dt * (SINGLE_STAGE_STEPS_CFL if single_stage else STEPS_CFL) / 0.9

# (dim, N, nc), each with n_picard -1 (N iterations) and 0 (single stage): tests/test_gpu_parity.py
DG_CASES = [(2, 4, (5, 3)), (2, 2, (4, 4)), (2, 8, (2, 3)), (2, 5, (3, 2)), (2, 3, (2, 4)), (2, 7, (2, 2)), (3, 3, (3, 2, 2)), (3, 4, (2, 2, 3)), (3, 5, (2, 1, 3)), (3, 6, (2, 2, 2)),
            (3, 7, (2, 1, 2)), (3, 8, (1, 2, 2)),       # N = 7, 8 in 3-D (cfg 4's p = 7): level-streamed stage A (exa_dg_stream.hpp)
            (3, 2, (2, 2, 2)), (2, 6, (3, 2)), (3, 6, (1, 1, 1)), (2, 4, (1, 1))]     # lowest order; a single periodic cell (its own neighbour everywhere)
TILE_ORDER_CASES = [(3, (8, 16, 8), None), (6, (8, 8, 8), None), (4, (16, 8, 24), ((8, 0, 8), (16, 8, 24))), (8, (8, 8, 8), None)]
MULTIPASS_CASES = [(6, (12, 10, 9)), (8, (7, 7, 6)), (4, (13, 11, 9)), (5, (9, 8, 8))]
BOX_MULTIPASS_CASE = (6, (9, 8, 7))
FUSED_CASES = [(4, (5, 3)), (2, (4, 4)), (8, (2, 3)), (6, (7, 4)), (3, (1, 9)), (4, (130, 127)), (3, (190, 130)), (8, (100, 91))]
# tests/test_stage_a_variants.py: (nc, n_picard) at N = 6 and N = 8
VARIANT_N6_CASES = [((2, 2, 2), -1), ((1, 1, 1), -1), ((3, 2, 1), 1), ((2, 1, 2), 2), ((2, 3, 2), 3), ((12, 10, 9), -1)]
VARIANT_N8_CASES = [((1, 2, 2), -1), ((2, 1, 1), 1), ((2, 2, 1), 3), ((7, 7, 6), -1)]
# tests/test_one_kernel_step.py (N = 6): (nc, n_picard), four steps of different size
ONE_KERNEL_CASES = [((2, 2, 2), -1), ((1, 1, 1), 2), ((3, 2, 1), 1), ((1, 3, 2), 3), ((9, 8, 8), -1)]
ONE_KERNEL_DT_FACTORS = (1.0, 0.7, 1.2, 0.9)     # of the CFL-0.6 step (STEPS_CFL)
# tests/test_limiter.py::test_limited_step_vs_oracle
LIMITER_CASES = [(2, 4, (4, 3)), (3, 3, (2, 2, 3)), (2, 2, (3, 3)), (3, 8, (2, 1, 2)), (3, 7, (1, 2, 2)),
                 (2, 5, (3, 2)), (3, 5, (2, 1, 2)), (2, 6, (2, 3)), (3, 6, (1, 2, 2))]      # N = 5, 6: limited steps at the orders no other case launches
# tests/test_dg_hard_states.py: one case per stage-A kernel (label, dim, N, nc, stage_a, fused 2-D single stage)
HARD_KERNELS = [("lds_n4", 3, 4, (2, 2, 3), "auto", False), ("reg_n6", 3, 6, (2, 2, 2), "reg", False), ("stream_n7", 3, 7, (2, 1, 2), "auto", False),
                ("m8_n8", 3, 8, (1, 2, 2), "reg", False), ("fused_2d_n4", 2, 4, (5, 3), "auto", True)]


def parity_input(dim, N, nc):
    u = euler_dg_state(tuple(nc) + (N,) * dim, seed=dim * 100 + N)
    dx = [1.0 / c for c in nc]
    return u, dx, cfl_dt(u, dx, dim, N)


def tile_order_input(N, nc):
    u = euler_dg_state(tuple(nc) + (N,) * 3, seed=900 + N)
    dx = [1.0 / c for c in nc]
    return u, dx, cfl_dt(u, dx, 3, N)


def multipass_input(N, nc, seed=None):
    u = euler_dg_state(tuple(nc) + (N,) * 3, seed=500 + N if seed is None else seed)
    dx = [1.0 / c for c in nc]
    return u, dx, cfl_dt(u, dx, 3, N)


def fused_input(N, nc):
    u = euler_dg_state(tuple(nc) + (N, N), seed=900 + N)
    dx = [1.0 / c for c in nc]
    return u, dx, cfl_dt(u, dx, 2, N)


def variant_n6_input(nc, n_it):
    N = 6
    u = euler_dg_state(tuple(nc) + (N,) * 3, seed=9000 + sum(nc) + max(n_it, 0))
    dx = [1.0 / nc[0], 0.8 / nc[1], 1.3 / nc[2]]                       # anisotropic: the per-direction scale is a lane property in the reg kernel
    return u, dx, cfl_dt(u, dx, 3, N)


def variant_n8_input(nc, n_it):
    N = 8
    u = euler_dg_state(tuple(nc) + (N,) * 3, seed=800 + sum(nc))
    dx = [1.0 / nc[0], 0.9 / nc[1], 1.2 / nc[2]]
    return u, dx, cfl_dt(u, dx, 3, N)


def one_kernel_input(nc):
    N = 6
    u = euler_dg_state(tuple(nc) + (N,) * 3, seed=77 + sum(nc))
    dx = [1.0 / nc[0], 0.8 / nc[1], 1.3 / nc[2]]
    dt = steps_dt(cfl_dt(u, dx, 3, N))
    return u, dx, [dt * f for f in ONE_KERNEL_DT_FACTORS]


def limiter_input(dim, N, nc):
    u = euler_dg_state(tuple(nc) + (N,) * dim, seed=31 + N)
    dx = [1.0 / nc[0]] * dim                                    # uniform cells (the FV patch has one h)
    rng = np.random.default_rng(5)
    mask = rng.random(nc) < 0.35
    mask.flat[0] = True
    return u, dx, cfl_dt(u, dx, dim, N), mask


def n_it_of(N, n_picard):
    return N if n_picard < 0 else n_picard


class DgRef:
    """The C oracle's stage A, stage B and steps for one input, with the bases and mutants assert_dg_parity needs.

    n_it is the oracle's Picard count (0: single stage).  Bases: u for u* and for states after k steps; the oracle's n_it = 0 stage A for
    traces (for an n_it = 0 run the traces have no dynamic part and are measured against max|want|).  Mutant: the same with n_it - 1."""

    def __init__(self, u, dt, dx, dim, N, nc, n_it, pde=PDE_EULER, m=5):
        import oracle
        from oracle.dg_operators import operators
        self.orc, self.ops = oracle, operators(N)
        self.u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        self.dt, self.dx, self.dim, self.N, self.nc, self.n_it, self.pde, self.m = dt, list(dx), dim, N, tuple(nc), n_it, pde, m
        self._a, self._s = {}, {}

    def stage_a(self, n_it=None):
        n_it = self.n_it if n_it is None else n_it
        if n_it not in self._a:
            self._a[n_it] = self.orc.aderdg_stage_a(self.u, self.dt, self.dx, self.ops, self.dim, self.N, self.m, self.pde, n_it)
        return self._a[n_it]

    def stage_b(self, n_it=None):
        us, tr = self.stage_a(n_it)
        return self.orc.aderdg_stage_b(us, tr, self.dt, self.dx, self.ops, self.dim, self.N, self.m, self.pde, self.nc)

    def steps(self, k, n_it=None, dts=None):
        """u after k steps (of dt, or of dts[0..k-1])."""
        n_it = self.n_it if n_it is None else n_it
        dts = [self.dt] * k if dts is None else list(dts)[:k]
        key = (n_it, tuple(dts))
        if key not in self._s:
            uo = self.u.copy()
            for dt in dts:
                uo = self.orc.aderdg_step(uo, dt, self.dx, self.ops, self.dim, self.N, self.m, self.pde, n_it, self.nc)
            self._s[key] = uo
        return self._s[key]

    @property
    def has_mutant(self):
        return self.n_it > 0

    def check_ustar(self, got, tol=None, what="u*"):
        kw = {} if tol is None else dict(tol=tol)
        return assert_dg_parity(np.asarray(got).reshape(-1, self.m), self.stage_a()[0].reshape(-1, self.m), self.u.reshape(-1, self.m),
                                None if not self.has_mutant else self.stage_a(self.n_it - 1)[0].reshape(-1, self.m), what=what, **kw)

    def check_traces(self, got, tol=None, what="traces"):
        kw = {} if tol is None else dict(tol=tol)
        want = self.stage_a()[1]
        base = self.stage_a(0)[1] if self.n_it > 0 else None
        mut = None if not self.has_mutant else self.stage_a(self.n_it - 1)[1]
        return assert_dg_parity(np.asarray(got).reshape(want.shape), want, base, mut, var_axis=4, what=what, **kw)

    def check_stage_b(self, got, tol=None, what="stage B"):
        kw = {} if tol is None else dict(tol=tol)
        return assert_dg_parity(np.asarray(got).reshape(-1, self.m), self.stage_b().reshape(-1, self.m), self.u.reshape(-1, self.m),
                                None if not self.has_mutant else self.stage_b(self.n_it - 1).reshape(-1, self.m), what=what, **kw)

    def check_steps(self, got, k, dts=None, tol=None, what=None):
        kw = {} if tol is None else dict(tol=tol)
        return assert_dg_parity(np.asarray(got).reshape(-1, self.m), self.steps(k, dts=dts).reshape(-1, self.m), self.u.reshape(-1, self.m),
                                None if not self.has_mutant else self.steps(k, self.n_it - 1, dts).reshape(-1, self.m),
                                what=what or "%d steps" % k, **kw)
