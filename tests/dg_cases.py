"""ADER-DG case tables and input builders shared by the GPU parity tests and their CPU check (tests/test_dg_reference_hp.py).

Every case runs at the CFL-0.9 step (tests/util.py cfl_dt; runs of several steps at STEPS_CFL below) and is compared with
oracle/exa_oracle.c through `DgRef`, which also runs the oracle with one Picard iteration less (the mutant): a case whose mutant does not differ by 100 * DG_TOL cannot see the last iteration, and
its check fails -- on the CPU, for every table here, without a GPU.  The sharded cases (tests/test_gpu_distributed.py) follow the single-block ones below:
their CPU check holds on every rank's cells, and also sees a block that ignores its ghosts (check_rank_slices).
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


# ---- the sharded step (tests/test_gpu_distributed.py; CPU half in tests/test_dg_reference_hp.py and tests/test_limiter.py) --------------------
# nc is ONE rank's block, pdims the process grid; the global grid is nc * pdims.  Runs of several steps at the CFL-0.6 step (steps_dt): at
# CFL 0.9 the unlimited N = 8 reference on (4, 1, 2) reaches 6e26 in two steps, the limited one 5e24.
# (N, nc, pdims, one_kernel): three steps of SHARDED_DT_FACTORS times that step (the one-kernel step sees dt_prev != dt)
SHARDED_CASES = [(3, (2, 3, 2), [2, 1, 1], False), (4, (3, 2, 2), [1, 2, 1], False), (3, (1, 2, 3), [2, 1, 1], False),
                 (6, (2, 2, 2), [2, 1, 1], False),      # cfg 3's order, one partitioned direction
                 (6, (2, 2, 2), [2, 2, 1], False),      # cfg 3's order, 4 ranks: ghosts in two directions
                 (6, (3, 2, 2), [1, 2, 2], False),      # 4 ranks, the other two directions; interior box non-empty in x
                 (6, (2, 2, 2), [2, 1, 1], True), (6, (3, 3, 2), [1, 2, 2], True)]       # the step as one kernel on shards, 2 and 4 ranks
SHARDED_DT_FACTORS = (1.0, 0.9, 0.8)
# (dim, N, nc, pdims): two limited steps, two ranks
SHARDED_LIMITER_CASES = [(2, 3, (2, 3), [2, 1]), (3, 3, (2, 2, 1), [1, 2, 1]), (2, 4, (3, 1), [1, 2]),
                         (3, 8, (2, 1, 2), [2, 1, 1])]      # cfg 4's order: p = 7, 17^3 patches
# (N, nc, limited): one rank, its own neighbour in every direction (RCCL send / recv to self), two steps
SHARDED_SELF_CASES = [(6, (3, 2, 2), False), (8, (2, 1, 2), True)]
EIGHT_SHARD_CASES = [(3, (2, 2, 2)), (6, (2, 1, 2))]       # (N, nc): 2 x 2 x 2 shards in one process, two steps
SHARDED_XT_CASE = (2, 3, (2, 3), [2, 1])                   # (dim, N, nc, pdims): term set with x, t and an ncp; three steps from t = 0.4
XT_ORIGIN, XT_T0 = [0.25, -0.5], 0.4
# (N, nc, pdims): AderDgSolver.run on two shards; the largest eigenvalue lies in rank 1's half (RUN_VELOCITY_SCALE on its x velocity)
SHARDED_RUN_CASES = [(3, (2, 2, 2), [2, 1, 1]), (6, (2, 2, 2), [2, 1, 1])]
RUN_CFL, RUN_CFL_STEPS, RUN_VELOCITY_SCALE = 0.6, 2.5, 5.5


def global_grid(nc, pdims):
    return tuple(int(c) * int(p) for c, p in zip(nc, pdims))


def rank_slices(nc, pdims):
    """Every rank's cells of the global grid (exahype_amd.solvers.CartesianPartition: rank = row-major index of its coordinates)."""
    dim = len(nc)
    pd = list(pdims) + [1] * (3 - len(pdims))
    out = []
    for r in range(int(np.prod(pd))):
        co = [r // (pd[1] * pd[2]), (r // pd[2]) % pd[1], r % pd[2]]
        out.append(tuple(slice(co[a] * nc[a], (co[a] + 1) * nc[a]) for a in range(dim)))
    return out


def sharded_input(N, nc, pdims, seed=42, factors=SHARDED_DT_FACTORS):
    G = global_grid(nc, pdims)
    u = euler_dg_state(G + (N,) * 3, seed=seed)
    dx = [1.0 / g for g in G]
    dt = steps_dt(cfl_dt(u, dx, 3, N))
    return G, u, dx, [dt * f for f in factors]


def sharded_self_input(N, nc, limited):
    u = euler_dg_state(tuple(nc) + (N,) * 3, seed=7 if limited else 9)
    dx = [1.0 / nc[0]] * 3 if limited else [1.0 / c for c in nc]
    return tuple(nc), u, dx, [steps_dt(cfl_dt(u, dx, 3, N))] * 2


def eight_shard_input(N, nc):
    return sharded_input(N, nc, [2, 2, 2], seed=88, factors=(1.0, 1.0))


def limiter_mask(G):
    dim = len(G)
    mask = np.random.default_rng(11).random(G) < 0.4
    mask[(0,) * dim] = True                                     # a troubled cell in the corner: every face is a block or wrap face
    return mask


def sharded_limiter_input(dim, N, nc, pdims):
    G = global_grid(nc, pdims)
    u = euler_dg_state(G + (N,) * dim, seed=7)
    dx = [1.0 / G[0]] * dim                                     # uniform cells (the FV patch has one h)
    return G, u, dx, steps_dt(cfl_dt(u, dx, dim, N)), limiter_mask(G)


def steps_ref(u, dx, N, G, dts, n_it=None):
    """u, the oracle after the steps dts, the same with one Picard iteration less; all in u's shape"""
    r = DgRef(u, dts[0], dx, len(G), N, G, N if n_it is None else n_it)
    return u, r.steps(len(dts), dts=dts).reshape(u.shape), r.steps(len(dts), r.n_it - 1, dts=dts).reshape(u.shape)


def limited_ref(u, mask, dt, dx, N, steps=2):
    import oracle
    from oracle import aderdg_numpy as A
    from oracle.dg_operators import operators
    from oracle.limiter_numpy import limited_step
    dim = len(dx)

    def fv(patch, dt, h):
        return oracle.fv_corrected(patch[None], dt, h, dim, patch.shape[0] - 2, 1, 5, 0, 1, oracle.PDE_EULER)[0]
    out = []
    for n_it in (N, N - 1):
        ref = u.copy()
        for _ in range(steps):
            ref = limited_step(ref, mask, dt, dx, operators(N), A.Euler(), fv, n_it)
        out.append(ref)
    return u, out[0], out[1]


def sharded_xt_input():
    """(term set, its numpy restatement, G, u, dx, dt): lam from the restatement's maxeig at the nodes (tests/test_dg_reference_hp.py
    test_numpy_step_xt_vs_long_double_reference)"""
    from oracle import aderdg_numpy as A
    from oracle.dg_operators import operators
    from tests.test_user_pde import OracleXtPDE, coupled_xt_ncp_system
    dim, N, nc, pdims = SHARDED_XT_CASE
    G = global_grid(nc, pdims)
    p = coupled_xt_ncp_system(max_dim=dim)
    o = OracleXtPDE(p)
    u = 1.0 + 0.3 * np.random.default_rng(5).random(G + (N,) * dim + (3,))
    dx = [0.9 / G[0], 1.1 / G[1]]
    x3 = A._coords(G, N, operators(N), dx, XT_ORIGIN)
    lam = max(float(np.max(o.maxeig(u, x3, XT_T0, a) * np.ones(u.shape[:-1]))) for a in range(dim))
    return p, o, G, u, dx, steps_dt(cfl_dt(u, dx, dim, N, lam=lam))


def xt_ref(o, u, dx, dt, N, origin=XT_ORIGIN, steps=3):
    from oracle import aderdg_numpy as A
    from oracle.dg_operators import operators
    out = []
    for n_it in (N, N - 1):
        ref, t = u.copy(), XT_T0
        for _ in range(steps):
            ref = A.step_xt(ref, dt, dx, operators(N), o, t=t, origin=origin, n_it=n_it)
            t += dt
        out.append(ref)
    return u, out[0], out[1]


def sharded_run_input(N, nc, pdims):
    """(G, u, dx, t_end): sharded_input's state with the x velocity of rank 1's half (pdims [2, 1, 1]) times RUN_VELOCITY_SCALE at the same
    density and pressure; t_end = RUN_CFL_STEPS steps of the first CFL step of the whole grid.  (x alone: with all three components scaled
    the node-wise random N = 6 state leaves the admissible set within three steps at CFL 0.6, lambda 2.3 -> 3e3; with one it stays put,
    2.4 -> 2.6 -> 2.5, and a 1e-15 perturbation of u moves the end state by 1e-14 of the increment.)"""
    G, u, dx, _ = sharded_input(N, nc, pdims, seed=300 + N)
    half = u[nc[0]:]
    kinetic = 0.5 * half[..., 1] ** 2 / half[..., 0]
    half[..., 1] *= RUN_VELOCITY_SCALE
    half[..., 4] += (RUN_VELOCITY_SCALE ** 2 - 1.0) * kinetic
    return G, u, dx, RUN_CFL_STEPS * cfl_dt(u, dx, 3, N, cfl=RUN_CFL)


def run_replay(u, dx, N, G, t_end, n_it=None, lam_of=None, max_steps=20):
    """AderDgSolver.run(t_end, cfl=RUN_CFL) on the oracle, the loop of tests/test_host_driver.py test_dg_cfl_time_loop: (steps, time, state).
    lam_of(state) replaces the scan over the whole grid (a rank that forgets the reduction scans its own cells only)."""
    import oracle
    from oracle.dg_operators import operators
    from tests.util import dg_max_eigenvalue
    dim = len(G)
    ref, t, steps = np.ascontiguousarray(u, dtype=np.float64).reshape(-1).copy(), 0.0, 0
    while t < t_end * (1 - 1e-14) and steps < max_steps:
        state = ref.reshape(u.shape)
        lam = dg_max_eigenvalue(state, dim) if lam_of is None else lam_of(state)
        dt = min(RUN_CFL * min(dx) / ((2 * N - 1) * dim * lam), t_end - t)
        ref = oracle.aderdg_step(ref, dt, dx, operators(N), dim, N, 5, oracle.PDE_EULER, N if n_it is None else n_it, G)
        t += dt
        steps += 1
    return steps, t, ref.reshape(u.shape)


def check_rank_slices(u, want, mutant, slices, alone=None, what=""):
    """CPU half of a sharded case, the oracle as `got`, on EVERY rank's cells: the run is finite, the mutant with one Picard iteration less is
    seen (>= 100 * DG_TOL of that rank's increment), and so is `alone(rank, slice)`: the rank's block stepped as a periodic block of its own,
    i.e. a shard that never read a ghost."""
    from tests.util import DG_TOL, dg_err
    assert np.isfinite(want).all() and np.isfinite(mutant).all(), what
    out = []
    for r, sl in enumerate(slices):
        _, em = assert_dg_parity(want[sl], want[sl], u[sl], mutant[sl], what="%s rank %d" % (what, r))
        ea = None
        if alone is not None:
            ea = dg_err(alone(r, sl), want[sl], u[sl])
            assert ea >= 100 * DG_TOL, "%s rank %d: a block that ignores its neighbours differs by %.3e only" % (what, r, ea)
        out.append((em, ea))
    return out
