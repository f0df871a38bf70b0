"""Case tables, inputs and references of the ADER-DG domain-boundary tests, shared by the GPU tests (tests/test_gpu_dg_boundary.py) and their
CPU check (tests/test_dg_boundary_reference.py), as tests/dg_cases.py is for the periodic and sharded paths.

A `Case` is one row with one kind set.  Its reference is the restatement tests/dg_boundary_numpy.py (fp64, or np.longdouble on operators_hp: the
anchor); `Case.run(mutant=...)` runs the restatement with ONE thing wrong -- a mistake the boundary path could make -- and every case must see
each mutant that applies to it at 100 * DG_TOL of the increment (MUTANTS_OF names them per kind set; DIM / row rules below)."""
import numpy as np

from oracle import aderdg_numpy as A
from oracle.dg_operators import operators, operators_hp
from tests import dg_boundary_numpy as B
from tests.dg_cases import steps_dt
from tests.util import cfl_dt, dg_max_eigenvalue, euler_dg_state

ORIGIN, T0 = [0.25, -0.5, 1.0], 0.4                # every row: a box away from the origin, a start time away from 0
EULER_SIGN = {a: np.where(np.arange(5) == 1 + a, -1.0, 1.0) for a in range(3)}
Q_IN = np.array([1.3, 0.4, -0.2, 0.1, 3.1])        # a constant Dirichlet state (Euler)
XT_SIGN = np.array([1.0, -1.0, 1.0])               # the wall of the three-field system
# a constant Dirichlet state of the three-field system: its eigenvalue |vel(x, t)| + |q0| / 5 at the face nodes exceeds every interior one
# (q0 <= 1.3 inside), so run() takes ITS step -- and one evaluated without position and time (vel = 1: 1.5) would not
XT_Q_IN = np.array([2.5, 0.9, 1.1])
STEP_FACTORS = (1.0, 0.9)                          # runs of two steps: the second sees advanced level times and another dt

KIND_SETS = {
    "outflow": lambda dim: {(a, s): "outflow" for a in range(dim) for s in range(2)},
    "wall": lambda dim: {(a, s): "wall" for a in range(dim) for s in range(2)},
    "const": lambda dim: {(a, s): "const" for a in range(dim) for s in range(2)},
    "func": lambda dim: {(a, s): "func" for a in range(dim) for s in range(2)},
    "mixed": lambda dim: {(0, 0): "func", (0, 1): "outflow", (1, 0): "wall", (1, 1): "const"},     # (axis 2, if any: periodic)
    "all_faces": lambda dim: dict([((0, 0), "func"), ((0, 1), "outflow"), ((1, 0), "wall"), ((1, 1), "const")]
                                  + ([((2, 0), "wall"), ((2, 1), "func")] if dim == 3 else [])),
    "all_faces_swapped": lambda dim: dict([((0, 1), "func"), ((0, 0), "outflow"), ((1, 1), "wall"), ((1, 0), "const")]
                                          + ([((2, 1), "wall"), ((2, 0), "func")] if dim == 3 else [])),
}
# the mutants a kind set can see (an outflow-only set has no wall to get wrong, ...).  By row: `picard` needs a Picard loop, `swap_node_axes` two
# transverse axes (3-D), `const_midpoint` / `flux_x0` a flux that sees x and t, `no_domain_jump` an ncp (Case.mutants).  An outflow ghost has no
# jump (q+ = q-), so an outflow-only set cannot see `no_domain_jump`.
_FUNC = ("func_midpoint", "opposite_side", "swap_node_axes", "no_origin")
MUTANTS_OF = {
    "outflow": ("picard", "periodic"),
    "wall": ("picard", "periodic", "wall_flux", "no_domain_jump"),
    "const": ("picard", "periodic", "const_midpoint", "flux_x0", "no_domain_jump"),
    "func": ("picard", "periodic", "flux_x0", "no_domain_jump") + _FUNC,
    "mixed": ("picard", "periodic", "wall_flux", "const_midpoint", "flux_x0", "no_domain_jump") + _FUNC,
    "all_faces": ("picard", "periodic", "wall_flux", "const_midpoint", "flux_x0", "no_domain_jump") + _FUNC,
    "all_faces_swapped": ("picard", "periodic", "wall_flux", "const_midpoint", "flux_x0", "no_domain_jump") + _FUNC,
}
ALL_MUTANTS = ("picard", "periodic", "wall_flux", "func_midpoint", "opposite_side", "swap_node_axes", "no_origin", "const_midpoint", "flux_x0",
               "no_domain_jump")
OLD_KINDS, NEW_KINDS = ("const", "func", "mixed", "outflow", "wall"), ("all_faces", "all_faces_swapped")

# (dim, N, nc, stage_a, n_picard)
PARITY_CASES = [(2, 4, (4, 3), "auto"), (3, 3, (3, 2, 2), "auto"), (3, 6, (2, 3, 2), "lds"), (3, 6, (2, 3, 2), "reg"), (3, 8, (2, 2, 2), "auto")]
NEW_EULER_ROWS = [(3, 2, (2, 2, 2), "auto", -1),
                  (3, 4, (2, 1, 2), "auto", -1),        # one cell along the bounded axis 1: the same cell feeds both ghosts
                  (3, 5, (1, 2, 2), "auto", -1),
                  (3, 7, (2, 1, 2), "auto", -1),        # level-streamed stage A
                  (2, 3, (2, 3), "auto", -1),           # dense stage B, an odd face
                  (2, 8, (2, 1), "auto", -1),
                  (3, 4, (2, 2, 2), "auto", 0),         # the single-stage scheme
                  (2, 4, (4, 3), "auto", 0)]
EULER_ROWS = [r + (-1,) for r in PARITY_CASES] + NEW_EULER_ROWS
EULER_CASES = [(r, k) for r in EULER_ROWS[:len(PARITY_CASES)] for k in OLD_KINDS] + [(r, k) for r in NEW_EULER_ROWS for k in NEW_KINDS]
# (dim, N, nc, with_ncp, with_xt) on tests/test_user_pde.py coupled_xt_ncp_system (the names of that file: one JIT library serves both)
XT_ROWS = [(2, 3, (3, 2), False, True), (2, 4, (2, 3), True, True), (3, 3, (2, 2, 2), True, True), (3, 6, (2, 1, 2), True, True),
           (3, 8, (1, 2, 1), True, True), (3, 4, (1, 2, 2), True, False)]
XT_CASES = [(r, k) for r in XT_ROWS for k in NEW_KINDS]
# AderDgSolver.run on a bounded box: (table, row, kind set); RUN_CFL_STEPS steps of the first CFL step at RUN_CFL
RUN_CASES = [("euler", (3, 4, (2, 2, 2), "auto", -1), "all_faces"), ("xt", (2, 4, (2, 3), True, True), "all_faces")]
RUN_CFL, RUN_CFL_STEPS = 0.6, 2.5
# two ranks, the x/t + ncp set: (dim, N, nc of ONE rank, pdims), three steps; the Dirichlet function on (0, 0), (0, 1), (1, 0), the constant on (2, 1)
SHARDED_XT_BC_CASE = (3, 3, (2, 2, 2), [2, 1, 1])
SHARDED_XT_BC_KINDS = {(0, 0): "func", (0, 1): "func", (1, 0): "func", (2, 1): "const"}
SHARDED_DT_FACTORS = (1.0, 0.9, 0.8)


def case_id(case):
    row, kind = case
    return "%dd-N%d-%s-%s-%s" % (row[0], row[1], "x".join(map(str, row[2])), "-".join(str(x) for x in row[3:]), kind)


def _lib(X):
    try:
        import torch
        if isinstance(X, torch.Tensor):
            return torch
    except ImportError:
        pass
    return np


def smooth_state(X, t):
    """An admissible Euler state that varies in space and time; numpy arrays or device tensors [..., 3] -> [..., 5]."""
    lib = _lib(X)
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    rho = 1.0 + 0.2 * lib.sin(2.0 * x + y - 0.5 * z + 3.0 * t)
    vx, vy, vz = 0.3 * lib.cos(x - y + t), 0.2 * lib.sin(y + z - t), -0.1 + 0.05 * x
    p = 1.0 + 0.1 * lib.cos(x + z + 2.0 * t)
    return lib.stack([rho, rho * vx, rho * vy, rho * vz, p / 0.4 + 0.5 * rho * (vx * vx + vy * vy + vz * vz)], -1)


def xt_state(X, t):
    """Three smooth fields of all three coordinates and t, not symmetric in any two axes: low-degree polynomials and one sine of a small argument
    (numpy and torch evaluate it alike to rounding); numpy arrays or device tensors [..., 3] -> [..., 3]."""
    lib = _lib(X)
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    q0 = 1.2 + 0.1 * x - 0.05 * y + 0.08 * z * x + 0.3 * t + 0.1 * lib.sin(0.3 * x + 0.2 * y - 0.1 * z + 0.5 * t)
    q1 = 0.9 + 0.07 * y * y - 0.04 * x * z + 0.2 * t * x + 0.03 * z
    q2 = 1.1 - 0.06 * z + 0.05 * x * y + 0.1 * t * t + 0.02 * y
    return lib.stack([q0, q1, q2], -1)


def coupled_system(dim, with_ncp=True, with_xt=True):
    """(the SympyPDE, its numpy restatement) of tests/test_user_pde.py's three-field system"""
    from tests.test_user_pde import OracleXtPDE, coupled_xt_ncp_system
    p = coupled_xt_ncp_system(max_dim=dim, with_ncp=with_ncp, with_xt=with_xt)
    return p, OracleXtPDE(p)


class Case:
    """One row with one kind set: input, step sizes and the restatement's runs (cached per mutant and dtype)."""

    def __init__(self, table, row, kind, kinds=None, nc=None, factors=STEP_FACTORS):
        self.table, self.row, self.kind = table, row, kind
        self.dim, self.N = row[0], row[1]
        self.nc = tuple(row[2] if nc is None else nc)
        dim, N, nc = self.dim, self.N, self.nc
        self.kinds = KIND_SETS[kind](dim) if kinds is None else dict(kinds)
        self.origin, self.t0 = ORIGIN[:dim], T0
        shape = nc + (N,) * dim
        if table == "euler":
            self.stage_a, self.n_picard = row[3], row[4]
            self.m, self.sympy_pde, self.pde = 5, None, A.Euler()
            self.with_ncp = self.with_xt = False
            self.u = euler_dg_state(shape, seed=5)
            self.dx = [0.7 / c for c in nc]
            self.func, self.const, self.sign = smooth_state, Q_IN, lambda a: EULER_SIGN[a]
            lam = dg_max_eigenvalue(self.u, dim)
        else:
            self.stage_a, self.n_picard = "auto", -1
            self.with_ncp, self.with_xt = row[3], row[4]
            self.m = 3
            self.sympy_pde, self.pde = coupled_system(dim, self.with_ncp, self.with_xt)
            self.u = 1.0 + 0.3 * np.random.default_rng(100 * dim + N).random(shape + (3,))
            self.dx = [(0.9, 1.1, 0.7)[a] / nc[a] for a in range(dim)]
            self.func, self.const, self.sign = xt_state, XT_Q_IN, lambda a: XT_SIGN
            lam = self.state_eigenvalue(self.u, self.t0)
        self.n_it = N if self.n_picard < 0 else self.n_picard
        self.dt = cfl_dt(self.u, self.dx, dim, N, lam=lam)                  # one step: CFL 0.9
        self.dts = [steps_dt(self.dt, single_stage=self.n_it == 0) * f for f in factors]      # a run of several steps
        self._runs = {}

    # -- what applies -------------------------------------------------------------------------------------------------------------------------
    def mutants(self):
        out = []
        has_func = "func" in self.kinds.values()
        for m in MUTANTS_OF[self.kind]:
            if m == "picard" and self.n_it == 0:
                continue
            if m == "swap_node_axes" and self.dim < 3:
                continue
            if m in ("const_midpoint", "flux_x0") and not self.with_xt:
                continue
            if m == "no_domain_jump" and not self.with_ncp:
                continue
            if m in _FUNC and not has_func:
                continue
            out.append(m)
        return out

    # -- the restatement ----------------------------------------------------------------------------------------------------------------------
    def state_eigenvalue(self, u, t, origin=None):
        """max over nodes and directions of the eigenvalue bound of a block's state at time t (AderDgSolver.max_eigenvalue)"""
        if self.table == "euler":
            return dg_max_eigenvalue(u, self.dim)
        nc = u.shape[:self.dim]
        x3 = A._coords(nc, self.N, operators(self.N), self.dx, self.origin if origin is None else origin)
        return max(float(np.max(self.pde.maxeig(u, x3, t, a) * np.ones(u.shape[:-1]))) for a in range(self.dim))

    def dirichlet_faces(self):
        return [(key, k) for key, k in sorted(self.kinds.items()) if k in ("func", "const")]

    def bcs(self, t, dt, ops, mutant=None, nc=None, origin=None, own=None):
        """the restatement's bcs of the step [t, t + dt]; nc / origin / own: of one shard (own: the faces that are domain faces of it)"""
        nc = self.nc if nc is None else nc
        origin = self.origin if origin is None else origin
        out = {}
        left_periodic = max(self.kinds) if mutant == "periodic" else None
        for (a, side), k in self.kinds.items():
            if (a, side) == left_periodic or (own is not None and (a, side) not in own):
                continue
            if k == "outflow":
                out[(a, side)] = ("outflow",)
            elif k == "wall":
                s = self.sign(a)
                out[(a, side)] = ("wall", s, s) if mutant == "wall_flux" else ("wall", s)
            else:
                X = B.face_positions(nc, self.N, ops, self.dx, a, 1 - side if mutant == "opposite_side" else side,
                                     None if mutant == "no_origin" else origin)
                if mutant == "swap_node_axes" and self.dim == 3:
                    X = np.swapaxes(X, 2, 3).copy()
                const = k == "const"
                mid = (mutant == "const_midpoint" and const) or (mutant == "func_midpoint" and not const)
                gh = B.dirichlet_ghost(self.const if const else self.func, self.pde, X, a, t, dt, ops, constant=const, midpoint=mid,
                                       flux_X=0 * X if mutant == "flux_x0" else None)
                out[(a, side)] = ("dirichlet", gh)
        return out

    def one_step(self, u, t, dt, ops, mutant=None, stages=False):
        n_it = self.n_it - 1 if mutant == "picard" else self.n_it
        bcs = self.bcs(t, dt, ops, mutant)
        if self.table == "euler":
            return B.step(u, dt, self.dx, ops, self.pde, bcs, n_it=n_it, stages=stages)
        return B.step_xt(u, dt, self.dx, ops, self.pde, bcs, t=t, origin=self.origin, n_it=n_it, stages=stages, domain_jump=mutant != "no_domain_jump")

    def run(self, mutant=None, hp=False, dts=None):
        """[stages of step 1, stages of step 2, ...] (dicts with ustar, unew) of the steps dts from t0; default: the one CFL-0.9 step"""
        dts = [self.dt] if dts is None else list(dts)
        key = (mutant, hp, tuple(dts))
        if key not in self._runs:
            ops = operators_hp(self.N) if hp else operators(self.N)
            u, t, out = (self.u.astype(np.longdouble) if hp else self.u), self.t0, []
            for dt in dts:
                out.append(self.one_step(u, t, dt, ops, mutant, stages=True))
                u, t = out[-1]["unew"], t + dt
            self._runs[key] = out
        return self._runs[key]

    def state(self, mutant=None, hp=False, dts=None):
        return self.run(mutant, hp, dts)[-1]["unew"]

    def dirichlet_eigenvalue(self, t, dt=None, kinds=("func",)):
        """max eigenvalue of the Dirichlet data of `kinds`: over the Gauss levels of the step [t, t + dt] (what the boundary kernel leaves in its
        scalar), or with dt None at time t (what run() evaluates before its first step).  0.0 without such a face."""
        ops = operators(self.N)
        times = [t] if dt is None else B.dirichlet_levels(t, dt, ops)[1]
        best = 0.0
        for (a, side), k in self.dirichlet_faces():
            if k in kinds:
                X = B.face_positions(self.nc, self.N, ops, self.dx, a, side, self.origin)
                best = max(best, B.dirichlet_max_eigenvalue(self.const if k == "const" else self.func, self.pde, X, times, self.dim, constant=k == "const"))
        return best

    def const_eigenvalue_without_xt(self):
        """the constant state's eigenvalue evaluated at x = 0, t = 0: what a point-wise evaluation without position and time hands a term set"""
        q, X = np.asarray(self.const, dtype=float)[None], np.zeros((1, 3))
        return max(float(np.max(B.maxeig_at(self.pde, q, X, 0.0, a))) for a in range(self.dim))

    # -- AderDgSolver.run(t_end, cfl) on the restatement -----------------------------------------------------------------------------------------
    def t_end(self):
        lam = max(self.state_eigenvalue(self.u, self.t0), self.dirichlet_eigenvalue(self.t0, kinds=("func", "const")))
        return self.t0 + RUN_CFL_STEPS * cfl_dt(self.u, self.dx, self.dim, self.N, cfl=RUN_CFL, lam=lam)

    def replay(self, t_end, mutant=None, max_steps=20):
        """(steps, time, state): the loop of AderDgSolver.run -- the eigenvalue of the state at the current time and of the Dirichlet data, then the
        step.  The Dirichlet data enter as the solver takes them in: a constant state of a term set without x / t by its eigenvalue; everything else
        at the face nodes, before the first step at the current time, afterwards over the levels of the step before (the scalar the boundary kernel
        left).  Mutants: picard, and `const_lambda_x0` -- the constant state's eigenvalue taken without position and time."""
        ops = operators(self.N)
        u, t, steps, last = self.u, self.t0, 0, None
        while t < t_end * (1 - 1e-14) and steps < max_steps:
            lam = self.state_eigenvalue(u, t)
            if self.with_xt:
                if mutant == "const_lambda_x0":
                    lam = max(lam, self.const_eigenvalue_without_xt())
                    lam = max(lam, self.dirichlet_eigenvalue(t, kinds=("func",)) if last is None else self.dirichlet_eigenvalue(*last, kinds=("func",)))
                else:
                    lam = max(lam, self.dirichlet_eigenvalue(t, kinds=("func", "const")) if last is None
                              else self.dirichlet_eigenvalue(*last, kinds=("func", "const")))
            else:
                lam = max(lam, self.dirichlet_eigenvalue(t, kinds=("const",)))
                lam = max(lam, self.dirichlet_eigenvalue(t, kinds=("func",)) if last is None else self.dirichlet_eigenvalue(*last, kinds=("func",)))
            dt = min(RUN_CFL * min(self.dx) / ((2 * self.N - 1) * self.dim * lam), t_end - t)
            u = self.one_step(u, t, dt, ops, "picard" if mutant == "picard" else None)
            last, t, steps = (t, dt), t + dt, steps + 1
        return steps, t, u


_CACHE = {}


def get_case(table, row, kind):
    """one Case per (table, row, kind set) and process: the tests that need its reference share it"""
    key = (table, row, kind)
    if key not in _CACHE:
        _CACHE[key] = Case(table, row, kind)
    return _CACHE[key]


# ---- the sharded case -------------------------------------------------------------------------------------------------------------------------
def sharded_xt_bc_case():
    """the WHOLE block of SHARDED_XT_BC_CASE as a Case (three steps of SHARDED_DT_FACTORS times the CFL-0.6 step)"""
    dim, N, nc, pdims = SHARDED_XT_BC_CASE
    G = tuple(c * p for c, p in zip(nc, pdims))
    key = ("sharded",)
    if key not in _CACHE:
        _CACHE[key] = Case("xt", (dim, N, G, True, True), "sharded", kinds=SHARDED_XT_BC_KINDS, factors=SHARDED_DT_FACTORS)
    return _CACHE[key]


MUTANTS_OF["sharded"] = ("picard", "periodic", "const_midpoint", "flux_x0", "no_domain_jump") + _FUNC


def rank_without_its_offset(case, rank_slice, dts):
    """Rank 1 of the sharded case evaluating its transverse Dirichlet faces WITHOUT its offset: the whole block with the ghosts of those faces
    replaced, on that rank's cells, by ghosts evaluated at the positions of a block that starts at the global origin.  Returns the end state."""
    ops = operators(case.N)
    nc = tuple(s.stop - s.start for s in rank_slice)
    own = [(a, side) for (a, side) in case.kinds if (side == 0 and rank_slice[a].start == 0) or (side == 1 and rank_slice[a].stop == case.nc[a])]
    u, t = case.u, case.t0
    for dt in dts:
        bcs = case.bcs(t, dt, ops)
        wrong = case.bcs(t, dt, ops, nc=nc, origin=case.origin, own=own)          # (origin: the global one, the shard's offset left out)
        for (a, side), bc in wrong.items():
            if bc[0] != "dirichlet":
                continue
            qg, Fg = (x.copy() for x in bcs[(a, side)][1])
            sl = tuple(rank_slice[b] for b in range(case.dim) if b != a)
            qg[sl], Fg[sl] = bc[1][0], bc[1][1]
            bcs[(a, side)] = ("dirichlet", (qg, Fg))
        u = B.step_xt(u, dt, case.dx, ops, case.pde, bcs, t=t, origin=case.origin, n_it=case.n_it)
        t += dt
    return u
