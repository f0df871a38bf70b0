"""Case tables of the halo-2 limiter tests, shared by the GPU tests (tests/test_limiter_muscl.py) and the CPU check of their bound
(tests/test_limiter_muscl_reference.py).

Grids: three or more cells on two axes make all four diagonal neighbours of a cell distinct; one and two cells exercise the wrap onto the
cell itself and onto one neighbour from both sides.  States: tests/limiter_cases.state (node-wise random, a different magnitude per variable).
Faces with conditions: one grid per dimension, with
  "wall_outflow_state"   a wall at the low and an outflow at the high face of axis 0, constant Dirichlet states on both faces of the last axis
                         (the later axis: its state wins in the corner entries, and a wrong axis order shows in the normal momentum);
  "walls"                walls on both faces of axes 0 and 1: wall-wall corners (3-D: the last axis stays periodic);
  "state_walls"          constant Dirichlet states on both faces of axis 0 (the EARLIER axis) and walls on axis 1: the corner entries are the
                         wall's signs times the state; in 3-D the last axis stays periodic, so the edges of axes (0, 2) carry the bare state.
"""
import numpy as np

from exahype_amd.boundary import Dirichlet, Outflow, Wall
from tests import limiter_cases as K

GRIDS = {2: [(3, 4), (2, 3), (1, 3), (4, 1)], 3: [(3, 4, 2), (2, 3, 4), (1, 3, 2)]}
ORDERS = {2: tuple(range(2, 9)), 3: tuple(range(2, 6))}
KERNEL_CASES = [(dim, N) for dim in (2, 3) for N in ORDERS[dim]]
OTHER_NV_CASES = [(2, 3), (2, 8), (3, 2), (3, 5)]              # nv = 1, 2
BC_GRID = {2: (3, 4), 3: (2, 3, 4)}
BC_KINDS = ("wall_outflow_state", "walls", "state_walls")
STATE_LO = np.array([1.3, 0.45, -0.2, 0.1, 2.9])
STATE_HI = np.array([0.7, -0.35, 0.25, -0.15, 2.1])


def wall_sign(dim, axis, nv=5):
    s = np.ones(nv)
    s[1 + axis] = -1.0
    return s


def conditions(dim, kind):
    """{(axis, side): condition} with every wall's sign resolved"""
    last = dim - 1
    if kind == "wall_outflow_state":
        return {(0, 0): Wall(wall_sign(dim, 0)), (0, 1): Outflow(), (last, 0): Dirichlet(STATE_LO), (last, 1): Dirichlet(STATE_HI)}
    if kind == "state_walls":
        return {(0, 0): Dirichlet(STATE_LO), (0, 1): Dirichlet(STATE_HI), (1, 0): Wall(wall_sign(dim, 1)), (1, 1): Wall(wall_sign(dim, 1))}
    assert kind == "walls", kind
    return {(a, side): Wall(wall_sign(dim, a)) for a in (0, 1) for side in (0, 1)}


def inputs(dim, N, nv=5):
    """[(nc, u)] for every grid of GRIDS[dim]"""
    return [(nc, K.state(dim, N, nc, nv, i)) for i, nc in enumerate(GRIDS[dim])]


def bc_inputs(dim, N):
    """[(kind, conditions, nc, u)]"""
    nc = BC_GRID[dim]
    return [(kind, conditions(dim, kind), nc, K.state(dim, N, nc, 5, 7 + i)) for i, kind in enumerate(BC_KINDS)]


def repad(patches, dim, halo=2, fill=1e30):
    """limiter_cases.random_patches (halo 1) with the same interiors and `halo` layers of +-fill around them"""
    core = patches[(slice(None),) + (slice(1, -1),) * dim]
    rng = np.random.default_rng(core.shape[1] + 17 * dim)
    shape = (core.shape[0],) + tuple(n + 2 * halo for n in core.shape[1:1 + dim]) + (core.shape[-1],)
    out = np.where(rng.random(shape) < 0.5, -fill, fill)
    out[(slice(None),) + (slice(halo, -halo),) * dim] = core
    return out
