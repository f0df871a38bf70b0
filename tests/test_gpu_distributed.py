"""The sharded ADER-DG step (boundary shell first, face-trace exchange on a second stream, interior overlapped) on real kernels, held to the
rule of tests/util.py: CFL-sized steps, the error per variable against the increment (dg_err <= DG_TOL), every case able to see its last
Picard iteration.

2 or 4 ranks share cuda:0 and exchange over gloo (host-staged).  (RCCL between ranks needs one GPU per rank; what one GPU can do over the real
transport is a rank that is its own periodic neighbour -- the *_over_rccl_send_recv_to_self tests.)  The cases and their inputs are the tables
of tests/dg_cases.py (SHARDED_*, EIGHT_SHARD_CASES); their CPU half -- on every rank's cells the oracle sees the Picard iteration less, a
block that ignores its ghosts, a shard that forgets its offset, a rank that skips the CFL reduction -- is in tests/test_dg_reference_hp.py and
tests/test_limiter.py.

The parent test computes the oracle's run of the whole grid once (result, the mutant with one Picard iteration less, the start state) and
hands it to the ranks as an .npz.  Every rank compares its cells
  * with the oracle's: assert_dg_parity at DG_TOL, the bound the same kernels meet un-sharded (tests/test_gpu_parity.py check_steps), and
  * with the same cells of the un-sharded block stepped on the same GPU, bit for bit (tests/util.py assert_shard_equals_whole_block): stage A is
    per cell, stage B does not care where a neighbour's trace lies.  The stage-A kernel's name depends on (N, n_picard, variant) only, so shard
    and block always run the same one and the DG_TOL branch of that helper is not taken by any case here.
Further: AderDgSolver.run on two shards (the CFL scan riding in stage B on ghost pointers, reduced with all_reduce(MAX)) and exa_dg_pack_face
against the slice of the trace array it copies.  Measured errors: profiles/dg_sharded_err.txt."""
import ctypes as CT
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import dg_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _run_ranks(tmp_path, text, world, timeout=600):
    script = tmp_path / "worker.py"
    script.write_text(text)
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout)[0])
    finally:
        for p in procs:                                   # exactly the processes started here
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, o[-3000:])


def _handover(tmp_path, u, want, mutant, **more):
    """the oracle's run of the whole grid, computed once by the parent, for the ranks to load"""
    path = str(tmp_path / "ref.npz")
    np.savez(path, u=u, want=want, mutant=mutant, **{k: np.asarray(v) for k, v in more.items()})
    return path


# Every worker: load the reference, run, collect the first failed check, leave the process group together and only then fail -- a rank that
# raised in front of the barrier would leave the others waiting in it for the time limit.
HEAD = r'''
import os, sys, traceback
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from exahype_amd import solvers as exa
from tests.util import assert_dg_parity, assert_shard_equals_whole_block
ref = np.load(%(ref)r)
u, want, mutant, dx = ref["u"], ref["want"], ref["mutant"], [float(x) for x in ref["dx"]]
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group(%(backend)r, rank=rank, world_size=world)

def leave(checks):
    failed = None
    try:
        checks()
    except BaseException:
        failed = traceback.format_exc()
    torch.cuda.synchronize()
    dist.barrier(); dist.destroy_process_group()
    if failed:
        print(failed)
        sys.exit(1)
'''

WORKER = HEAD + r'''
dim, N, nc, pdims, one = 3, %(N)d, %(nc)r, %(pdims)r, %(one)r
dts = [float(x) for x in ref["dts"]]
part = exa.CartesianPartition(world, rank, dim, pdims)
G = tuple(nc[a] * part.pdims[a] for a in range(3))
s = exa.AderDgSolver(dim, N, nc, dx=dx, part=part, backend_is_gloo=True, one_kernel_step=one)
whole = exa.AderDgSolver(dim, N, G, dx=dx, one_kernel_step=one)
sl = tuple(slice(part.coords[a] * nc[a], (part.coords[a] + 1) * nc[a]) for a in range(3))
s.upload(u[sl])
whole.upload(u)
def checks():
    for dt in dts:
        s.step(dt)
        whole.step(dt)
        assert (s._pending_dt is not None) == bool(one)
    torch.cuda.synchronize()
    got = s.download()
    what = "sharded N %%d %%s on %%s%%s, rank %%d" %% (N, nc, pdims, " one kernel" if one else "", rank)
    assert_dg_parity(got, want[sl], u[sl], mutant[sl], what=what)
    assert_shard_equals_whole_block(got, whole.download()[sl], u[sl], s, whole, what)
leave(checks)
'''


def _sharded(tmp_path, N, nc, pdims, one):
    G, u, dx, dts = C.sharded_input(N, nc, pdims)
    ref = _handover(tmp_path, *C.steps_ref(u, dx, N, G, dts), dx=dx, dts=dts)
    _run_ranks(tmp_path, WORKER % dict(root=ROOT, ref=ref, backend="gloo", N=N, nc=nc, pdims=pdims, one=one), int(np.prod(pdims)))


@pytest.mark.parametrize("N,nc,pdims", [c[:3] for c in C.SHARDED_CASES if not c[3]])
def test_sharded_step_equals_global_oracle(tmp_path, N, nc, pdims):
    _sharded(tmp_path, N, nc, pdims, False)


@pytest.mark.parametrize("nc,pdims", [c[1:3] for c in C.SHARDED_CASES if c[3]])
def test_sharded_one_kernel_step_equals_global_oracle(tmp_path, nc, pdims):
    """the step as one kernel on shards (exa_dg_corrector_predictor): the shell cells' kernel takes the previous step's ghosts, the new traces
    travel while the interior cells run; 2 and 4 ranks, N = 6, a different dt every step"""
    _sharded(tmp_path, 6, nc, pdims, True)


XT_WORKER = HEAD + r'''
from tests.test_user_pde import coupled_xt_ncp_system
dim, N, nc, pdims = %(case)r
origin, t0, dt = %(origin)r, %(t0)r, float(ref["dt"])
part = exa.CartesianPartition(world, rank, dim, pdims)
G = tuple(nc[a] * part.pdims[a] for a in range(dim))
pid = coupled_xt_ncp_system(max_dim=dim).register()
s = exa.AderDgSolver(dim, N, nc, pde=pid, n_vars=3, dx=dx, part=part, backend_is_gloo=True, origin=origin, time=t0)
whole = exa.AderDgSolver(dim, N, G, pde=pid, n_vars=3, dx=dx, origin=origin, time=t0)
sl = tuple(slice(part.coords[a] * nc[a], (part.coords[a] + 1) * nc[a]) for a in range(dim))
s.upload(u[sl])
whole.upload(u)
def checks():
    for _ in range(3):
        s.step(dt)
        whole.step(dt)
    torch.cuda.synchronize()
    got = s.download()
    what = "sharded x/t + ncp, rank %%d" %% rank
    assert_dg_parity(got, want[sl], u[sl], mutant[sl], what=what)
    # (the shard's nodes lie at (origin + offset) + (c + xi) dx, the block's at origin + (c_global + xi) dx: on this grid both round to the same
    # positions, so the terms see the same x and the equality holds here too)
    assert_shard_equals_whole_block(got, whole.download()[sl], u[sl], s, whole, what)
leave(checks)
'''


def test_sharded_step_with_position_dependent_terms_and_ncp(tmp_path):
    """two shards of a 2-D grid, term set with node coordinates, level times and a non-conservative product: every shard evaluates the terms at
    ITS coordinates (origin + shard offset), the ncp jump term crosses the shard boundary through the ghost traces"""
    p, o, G, u, dx, dt = C.sharded_xt_input()
    ref = _handover(tmp_path, *C.xt_ref(o, u, dx, dt, C.SHARDED_XT_CASE[1]), dx=dx, dt=dt)
    _run_ranks(tmp_path, XT_WORKER % dict(root=ROOT, ref=ref, backend="gloo", case=C.SHARDED_XT_CASE, origin=C.XT_ORIGIN, t0=C.XT_T0), 2)


RCCL_SELF_WORKER = HEAD + r'''
dim, N, nc = 3, %(N)d, %(nc)r                                    # RCCL, one rank: its own neighbour in every direction
dts = [float(x) for x in ref["dts"]]
part = exa.CartesianPartition(1, 0, dim, exchange_self=(0, 1, 2))
s = exa.AderDgSolver(dim, N, nc, dx=dx, part=part)               # device buffers go to ncclSend / ncclRecv as they are
assert s.halo is not None and all(g is not None and g.is_cuda for g in s.halo.ghost)
s.exchange_events = []
s.upload(u)
plain = exa.AderDgSolver(dim, N, nc, dx=dx)
plain.upload(u)
def checks():
    for dt in dts:
        s.step(dt)
        plain.step(dt)
    torch.cuda.synchronize()
    got = s.download()
    what = "rccl to self N %%d %%s" %% (N, nc)
    assert_dg_parity(got, want, u, mutant, what=what)
    assert np.array_equal(got, plain.download())                 # shell + interior + ghost buffers == one periodic block, bit for bit
    assert_shard_equals_whole_block(got, plain.download(), u, s, plain, what)
    assert len(s.exchange_events) == 2
leave(checks)
'''


def test_sharded_step_over_rccl_send_recv_to_self(tmp_path):
    """The one exchange a single GPU allows over the real transport: a process group of ONE rank on the nccl (= RCCL) backend,
    every direction wrapped through HaloExchange (ncclSend / ncclRecv to self inside one group call).  cfg 3's order; the result must equal
    both the oracle and the un-sharded periodic block."""
    (N, nc, _), = [c for c in C.SHARDED_SELF_CASES if not c[2]]
    G, u, dx, dts = C.sharded_self_input(N, nc, False)
    ref = _handover(tmp_path, *C.steps_ref(u, dx, N, G, dts), dx=dx, dts=dts)
    _run_ranks(tmp_path, RCCL_SELF_WORKER % dict(root=ROOT, ref=ref, backend="nccl", N=N, nc=nc), 1)


LIM_WORKER = HEAD + r'''
dim, N, nc, pdims, self_exchange = %(dim)d, %(N)d, %(nc)r, %(pdims)r, %(selfx)r
dt, mask = float(ref["dt"]), ref["mask"]
part = exa.CartesianPartition(world, rank, dim, pdims, exchange_self=self_exchange)
G = tuple(nc[a] * part.pdims[a] for a in range(dim))
s = exa.AderDgSolver(dim, N, nc, dx=dx, part=part, backend_is_gloo=not self_exchange)
lim = exa.SubcellLimiter(s)
if self_exchange:
    assert lim.hx_layer is not None and not lim.hx_layer.stage      # subcell layers travel as device buffers
whole = exa.AderDgSolver(dim, N, G, dx=dx)
lim_whole = exa.SubcellLimiter(whole)
sl = tuple(slice(part.coords[a] * nc[a], (part.coords[a] + 1) * nc[a]) for a in range(dim))
s.upload(u[sl])
whole.upload(u)
def checks():
    for _ in range(2):
        n = lim.step(dt, mask[sl])
        assert n == int(mask[sl].sum())
        assert lim_whole.step(dt, mask) == int(mask.sum())
    torch.cuda.synchronize()
    got = s.download()
    what = "sharded limited %%d-D N %%d %%s on %%s%%s, rank %%d" %% (dim, N, nc, pdims, " rccl to self" if self_exchange else "", rank)
    assert_dg_parity(got, want[sl], u[sl], mutant[sl], what=what)
    assert_shard_equals_whole_block(got, whole.download()[sl], u[sl], s, whole, what)
leave(checks)
'''


@pytest.mark.parametrize("dim,N,nc,pdims", C.SHARDED_LIMITER_CASES)
def test_sharded_limited_step_equals_global_oracle(tmp_path, dim, N, nc, pdims):
    """cfg 4 across ranks: troubled cells at a block face take their FV halo from the neighbour block's subcell layer."""
    G, u, dx, dt, mask = C.sharded_limiter_input(dim, N, nc, pdims)
    ref = _handover(tmp_path, *C.limited_ref(u, mask, dt, dx, N), dx=dx, dt=dt, mask=mask)
    _run_ranks(tmp_path, LIM_WORKER % dict(root=ROOT, ref=ref, backend="gloo", dim=dim, N=N, nc=nc, pdims=pdims, selfx=()), 2)


def test_sharded_limited_step_over_rccl_send_recv_to_self(tmp_path):
    """cfg 4's order (p = 7, 17^3 FV patches) with both limiter exchanges (troubled flags, subcell layers) and the trace exchange over RCCL
    send/recv to self."""
    (N, nc, _), = [c for c in C.SHARDED_SELF_CASES if c[2]]
    G, u, dx, dts = C.sharded_self_input(N, nc, True)
    mask = C.limiter_mask(G)
    ref = _handover(tmp_path, *C.limited_ref(u, mask, dts[0], dx, N), dx=dx, dt=dts[0], mask=mask)
    _run_ranks(tmp_path, LIM_WORKER % dict(root=ROOT, ref=ref, backend="nccl", dim=3, N=N, nc=nc, pdims=[1, 1, 1], selfx=(0, 1, 2)), 1)


RUN_WORKER = HEAD + r'''
dim, N, nc, pdims, cfl = 3, %(N)d, %(nc)r, %(pdims)r, %(cfl)r
t_end = float(ref["t_end"])
part = exa.CartesianPartition(world, rank, dim, pdims)
G = tuple(nc[a] * part.pdims[a] for a in range(3))
sl = tuple(slice(part.coords[a] * nc[a], (part.coords[a] + 1) * nc[a]) for a in range(3))
shard = lambda: exa.AderDgSolver(dim, N, nc, dx=dx, part=part, backend_is_gloo=True)
s, whole = shard(), exa.AderDgSolver(dim, N, G, dx=dx)
s.upload(u[sl])
whole.upload(u)
def checks():
    assert s.can_fuse_cfl_scan()                                 # the scan of step n + 1 rides in stage B of step n, on ghost pointers
    steps = s.run(t_end, cfl=cfl)
    seen = [None] * world
    dist.all_gather_object(seen, (steps, s.time))
    assert all(x == (3, s.time) for x in seen), seen
    assert whole.run(t_end, cfl=cfl) == 3 and abs(whole.time - s.time) <= 1e-15 * t_end
    torch.cuda.synchronize()
    got = s.download()
    what = "sharded run N %%d %%s on %%s, rank %%d" %% (N, nc, pdims, rank)
    assert_dg_parity(got, want[sl], u[sl], mutant[sl], what=what)
    assert_shard_equals_whole_block(got, whole.download()[sl], u[sl], s, whole, what)
    # one step on the shard: stage B on the ghosts with the scan == the plain launch, its eigenvalue == the separate scan of the same u
    a, b = shard(), shard()
    a.upload(u[sl])
    b.upload(u[sl])
    dt = t_end / %(cfl_steps)r
    a.step(dt)
    lam = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    for lo, hi in b.shell:
        b.predictor_volume(dt, lo, hi)
    b._pack_faces()
    b.halo.start()
    b.halo.finish()
    lo, hi = b.interior
    if all(h > l for l, h in zip(lo, hi)):
        b.predictor_volume(dt, lo, hi)
    assert b.ghost_ptrs()[0] and b.ghost_ptrs()[1]
    b.riemann_corrector(dt, lam_out=lam)
    torch.cuda.synchronize()
    assert torch.equal(a.u, b.u)
    assert float(lam[0]) == float(a.max_eigenvalue()[0]) > 0.0
leave(checks)
'''


@pytest.mark.parametrize("N,nc,pdims", C.SHARDED_RUN_CASES)
def test_sharded_run_reduces_the_cfl_step_over_the_ranks(tmp_path, N, nc, pdims):
    """AderDgSolver.run on two shards whose largest eigenvalue lies in rank 1 and is 1.6 times rank 0's own: both ranks take the same three steps,
    and end where the un-sharded run and the oracle's replay of the adaptive rule end."""
    G, u, dx, t_end = C.sharded_run_input(N, nc, pdims)
    steps, _, want = C.run_replay(u, dx, N, G, t_end)
    assert steps == 3
    ref = _handover(tmp_path, u, want, C.run_replay(u, dx, N, G, t_end, n_it=N - 1)[2], dx=dx, t_end=t_end)
    _run_ranks(tmp_path, RUN_WORKER % dict(root=ROOT, ref=ref, backend="gloo", N=N, nc=nc, pdims=pdims, cfl=C.RUN_CFL, cfl_steps=C.RUN_CFL_STEPS), 2)


@pytest.mark.parametrize("N,nc", C.EIGHT_SHARD_CASES)
def test_full_2x2x2_layout_eight_shards_in_one_process(N, nc):
    """configs[3]'s process grid at kernel level: EIGHT shards of a periodic grid -- all three directions partitioned, every shard with
    ghosts on all six faces -- each with its own plan, boundary shell, packed faces (exa_dg_pack_face), ghost buffers and stage B on
    ghosts; the exchange itself is a device copy between the shards' buffers (eight processes cannot share the box's one GPU: at most six
    may, and RCCL needs a GPU per rank; the transport is covered by the gloo runs above, by tests/test_partition_halo.py with world 8
    and by the RCCL-to-self test).  Every shard must equal the oracle's cells of the whole 2 nc grid, and the un-sharded block's bit for bit."""
    import torch
    from exahype_amd import solvers as exa
    from tests.util import assert_dg_parity, assert_shard_equals_whole_block
    dim = 3
    G, u, dx, dts = C.eight_shard_input(N, nc)
    u, want, mutant = C.steps_ref(u, dx, N, G, dts)
    parts = [exa.CartesianPartition(8, r, dim) for r in range(8)]
    assert parts[0].pdims == [2, 2, 2]
    shards = [exa.AderDgSolver(dim, N, nc, dx=dx, part=p, backend_is_gloo=True) for p in parts]
    sl = [tuple(slice(p.coords[a] * nc[a], (p.coords[a] + 1) * nc[a]) for a in range(3)) for p in parts]
    assert sl == C.rank_slices(nc, [2, 2, 2])
    for s, w in zip(shards, sl):
        s.upload(u[w])
    whole = exa.AderDgSolver(dim, N, G, dx=dx)
    whole.upload(u)
    for dt in dts:
        for s in shards:                                          # stage A on the boundary shell, faces packed
            for lo, hi in s.shell:
                s.predictor_volume(dt, lo, hi)
            s._pack_faces()
        for r, s in enumerate(shards):                            # "exchange": my ghost pair of direction d = the peer's send pair
            for d in range(3):
                peer = parts[r].neighbour(d, +1)
                assert peer == parts[r].neighbour(d, -1) and peer != r
                s.halo._ghost_pair[d].copy_(shards[peer].halo._send_pair[d])
        for s in shards:                                          # interior cells, then Riemann + corrector on the ghosts
            lo, hi = s.interior
            if all(h > l for l, h in zip(lo, hi)):
                s.predictor_volume(dt, lo, hi)
            s.riemann_corrector(dt)
        whole.step(dt)
    torch.cuda.synchronize()
    block = whole.download()
    for r, (s, w) in enumerate(zip(shards, sl)):
        what = "eight shards N %d %s, shard %d" % (N, nc, r)
        got = s.download()
        assert_dg_parity(got, want[w], u[w], mutant[w], what=what)
        assert_shard_equals_whole_block(got, block[w], u[w], s, whole, what)


@pytest.mark.parametrize("dim,N,nc", [(2, 4, (3, 2)), (3, 3, (2, 3, 4)), (3, 3, (1, 2, 3)),      # (1, 2, 3): one cell along x, both layers are the same cell
                                       (3, 6, (2, 1, 2))])
def test_packed_face_is_the_slice_of_the_trace_array(dim, N, nc):
    """exa_dg_pack_face(d, side) == trace[d, side] at the layer c_d = 0 (side 0: the L traces) / nc_d - 1 (side 1: the R traces), the expression of
    HaloExchange.pack; the destination starts as NaN, so every entry must have been written."""
    import torch
    from exahype_amd import solvers as exa
    from exahype_amd._lib import check
    u, dx, dt = C.parity_input(dim, N, nc)
    s = exa.AderDgSolver(dim, N, nc, dx=dx)
    s.upload(u)
    s.predictor_volume(dt)
    nc3 = list(nc) + [1] * (3 - dim)
    assert bool(torch.isfinite(s.trace).all())
    for d in range(dim):
        for side in range(2):
            want = s.trace[d, side].select(d, 0 if side == 0 else nc3[d] - 1).reshape(-1, s.ts)
            assert want.shape[0] == int(np.prod(nc3)) // nc3[d] and bool((want != 0).any())
            packed = torch.full(tuple(want.shape), float("nan"), dtype=torch.float64, device="cuda")
            check(s.lib.exa_dg_pack_face(s._plan, CT.c_void_p(s.trace.data_ptr()), d, side, CT.c_void_p(packed.data_ptr()), None))
            torch.cuda.synchronize()
            assert torch.equal(packed, want), (d, side)
            other = s.trace[d, 1 - side].select(d, 0 if side == 0 else nc3[d] - 1).reshape(-1, s.ts)
            assert not torch.equal(packed, other), (d, side)     # (the other side's traces of the same layer differ: the side is seen)
