"""Numpy restatement of one ADER-DG step on a NON-periodic box: the local stages of oracle/aderdg_numpy.py (predictor, time averages,
volume, traces) unchanged, then a Riemann solve that takes the state beyond a domain face from a ghost trace, and the corrector.  `step` for
term sets of the state alone, `step_xt` for terms that see x and t and a non-conservative product (the bounded form of aderdg_numpy.step_xt).

bcs: {(axis, side): ("outflow",) | ("wall", s[V]) | ("dirichlet", (qg, Fg))} with qg, Fg the ghost's time-averaged state and normal flux,
shaped like one face slice of the traces (grid without `axis`, face nodes, var).  A face not named is periodic.  The ghost rules are those of
include/exahype_hip.h exa_dg_boundary_ghost: outflow (q_in, F_in), wall (s q_in, -s F_in), Dirichlet sum_l w_l (q_l, F_d(q_l, x_y, t_l)) over the
Gauss levels, for a function and for a constant state alike (a constant state's average is the state itself; its flux is averaged where the
term set sees x or t).  Everything runs in the dtype of `u` and `ops` (np.longdouble on oracle.dg_operators.operators_hp: the anchor of
tests/test_dg_boundary_reference.py).  ("wall", s, fs) with a third entry is a wall whose flux factor is fs instead of -s: a mutant."""
import inspect

import numpy as np

from oracle import aderdg_numpy as A


def ghost(tr, axis, side, bc):
    """(q, F) beyond the face (axis, side) of the domain; tr = traces(...)[axis] = (qL, qR, FL, FR)."""
    qL, qR, FL, FR = tr
    n = qL.shape[axis]
    q_in = np.take(qL, 0, axis=axis) if side == 0 else np.take(qR, n - 1, axis=axis)
    F_in = np.take(FL, 0, axis=axis) if side == 0 else np.take(FR, n - 1, axis=axis)
    kind = bc[0]
    if kind == "outflow":
        return q_in, F_in
    if kind == "wall":
        s = np.asarray(bc[1])
        return s * q_in, (-s if len(bc) < 3 else np.asarray(bc[2])) * F_in
    if kind == "dirichlet":
        return bc[1]
    raise ValueError(kind)


def riemann_faces(tr, pde, axis, dim, bcs):
    """Rusanov flux on the n + 1 faces along `axis` (face f between cell f - 1 and cell f): [.., n + 1 along axis, .., face nodes, var]."""
    qL, qR, FL, FR = tr
    n = qL.shape[axis]
    lo, hi = bcs.get((axis, 0)), bcs.get((axis, 1))
    gq_lo, gF_lo = ghost(tr, axis, 0, lo) if lo else (np.take(qR, n - 1, axis=axis), np.take(FR, n - 1, axis=axis))
    gq_hi, gF_hi = ghost(tr, axis, 1, hi) if hi else (np.take(qL, 0, axis=axis), np.take(FL, 0, axis=axis))
    qm = np.concatenate([np.expand_dims(gq_lo, axis), qR], axis=axis)
    Fm = np.concatenate([np.expand_dims(gF_lo, axis), FR], axis=axis)
    qp = np.concatenate([qL, np.expand_dims(gq_hi, axis)], axis=axis)
    Fp = np.concatenate([FL, np.expand_dims(gF_hi, axis)], axis=axis)
    lam = np.maximum(pde.maxeig(qm, axis), pde.maxeig(qp, axis))
    s = lam.max(axis=tuple(range(dim, 2 * dim - 1)), keepdims=True) if dim > 1 else lam
    return 0.5 * (Fm + Fp) - 0.5 * s[..., None] * (qp - qm)


def corrector(us, Ff, dt, dx, ops):
    d = A._dim(us)
    N = ops['N']
    w, phiL, phiR = ops['w'], ops['phiL'], ops['phiR']
    un = us.copy()
    for a in range(d):
        n = us.shape[a]
        FR = np.expand_dims(np.take(Ff[a], np.arange(1, n + 1), axis=a), d + a)
        FLf = np.expand_dims(np.take(Ff[a], np.arange(0, n), axis=a), d + a)
        sh = [1] * us.ndim
        sh[d + a] = N
        un -= dt / dx[a] * (phiR.reshape(sh) * FR - phiL.reshape(sh) * FLf) / w.reshape(sh)
    return un


def step(u, dt, dx, ops, pde, bcs, n_it=None, stages=False):
    """One step with boundary ghosts.  n_it = 0 is the single-stage scheme: qbar := u, Fbar := f(u) (aderdg_numpy.step_single_stage)."""
    d = A._dim(u)
    if n_it == 0:
        qbar, Fbar = u, [pde.flux(u, a) for a in range(d)]
    else:
        q = A.predictor(u, dt, dx, ops, pde, n_it)
        qbar, Fbar = A.time_averages(q, ops, pde)
    us = A.volume(u, Fbar, dt, dx, ops)
    tr = A.traces(qbar, Fbar, ops)
    Ff = [riemann_faces(tr[a], pde, a, d, bcs) for a in range(d)]
    un = corrector(us, Ff, dt, dx, ops)
    if stages:
        return dict(traces=tr, Ffaces=Ff, ustar=us, unew=un)
    return un


def _put(arr, index, axis, value):
    """arr[.., index along axis, ..] = value, in place (arr: a fresh array)"""
    arr[(slice(None),) * axis + (index,)] = value
    return arr


def step_xt(u, dt, dx, ops, pde, bcs, t=0.0, origin=None, n_it=None, stages=False, domain_jump=True):
    """The bounded form of aderdg_numpy.step_xt: its local stages (predictor with x and t, source, ncp, volume, traces) as they are; in the
    Riemann solve the plus state of the last cell's high face and the minus state of cell 0's low face, with their fluxes, come from the ghost of
    a named domain face.  Eigenvalue and ncp jump term at the face's own coordinates and t + dt / 2 (dg_stage_b_dense_kernel).  With no face
    named every operation is step_xt's, in its order: the results are equal bit for bit.  domain_jump=False leaves the ncp jump term out at
    the named domain faces (a mutant)."""
    d = A._dim(u)
    N = ops['N']
    grid = u.shape[:d]
    origin = [0.0] * d if origin is None else origin
    st = A.step_xt(u, dt, dx, ops, pde, t=t, origin=origin, n_it=n_it, stages=True)
    us, tr, w = st['ustar'], st['traces'], ops['w']
    has_ncp = hasattr(pde, "ncp")
    x3 = A._coords(grid, N, ops, dx, origin)
    tf = t + 0.5 * dt
    un = us.copy()
    for a in range(d):
        qL, qR, FL, FR = tr[a]
        n = grid[a]
        lo, hi = bcs.get((a, 0)), bcs.get((a, 1))
        xf = []
        for b in range(3):
            if b >= d:
                xf.append(np.zeros([1] * (2 * d - 1)))
            elif b == a:
                sh = [1] * (2 * d - 1)
                sh[a] = n
                xf.append((origin[a] + (np.arange(n, dtype=u.dtype) + 1) * dx[a]).reshape(sh))
            else:
                xf.append(np.squeeze(x3[b], axis=d + a))
        # high face of every cell: minus = own R, plus = right neighbour's L -- beyond the last cell the ghost of (a, 1)
        qm, Fm = qR, FR
        qp, Fp = np.roll(qL, -1, axis=a), np.roll(FL, -1, axis=a)
        if hi:
            gq, gF = ghost(tr[a], a, 1, hi)
            qp, Fp = _put(qp, n - 1, a, gq), _put(Fp, n - 1, a, gF)
        lam = np.maximum(pde.maxeig(qm, xf, tf, a) * np.ones(qm.shape[:-1]), pde.maxeig(qp, xf, tf, a) * np.ones(qm.shape[:-1]))
        s = lam.max(axis=tuple(range(d, d + d - 1)), keepdims=True) if d > 1 else lam
        Fs = 0.5 * (Fm + Fp) - 0.5 * s[..., None] * (qp - qm)
        Dj = pde.ncp(0.5 * (qm + qp), qp - qm, xf, tf, a) if has_ncp else np.zeros_like(Fs)
        if hi and has_ncp and not domain_jump:
            Dj = _put(Dj.copy(), n - 1, a, 0.0)
        # low face of every cell, at ITS coordinates: minus = left neighbour's R -- before cell 0 the ghost of (a, 0) --, plus = own L
        xlo = list(xf)
        sh = [1] * (2 * d - 1)
        sh[a] = n
        xlo[a] = (origin[a] + np.arange(n, dtype=u.dtype) * dx[a]).reshape(sh)
        qm_l, Fm_l, qp_l = np.roll(qR, 1, axis=a), np.roll(FR, 1, axis=a), qL
        if lo:
            gq, gF = ghost(tr[a], a, 0, lo)
            qm_l, Fm_l = _put(qm_l, 0, a, gq), _put(Fm_l, 0, a, gF)
        lam_l = np.maximum(pde.maxeig(qm_l, xlo, tf, a) * np.ones(qL.shape[:-1]), pde.maxeig(qp_l, xlo, tf, a) * np.ones(qL.shape[:-1]))
        s_l = lam_l.max(axis=tuple(range(d, d + d - 1)), keepdims=True) if d > 1 else lam_l
        Flo = 0.5 * (Fm_l + FL) - 0.5 * s_l[..., None] * (qp_l - qm_l)
        if has_ncp:
            Dl = pde.ncp(0.5 * (qm_l + qp_l), qp_l - qm_l, xlo, tf, a)
            if lo and not domain_jump:
                Dl = _put(Dl.copy(), 0, a, 0.0)
            Flo = Flo - 0.5 * Dl
        Fhi = Fs + 0.5 * Dj
        sh = [1] * us.ndim
        sh[d + a] = N
        un -= dt / dx[a] * (ops['phiR'].reshape(sh) * np.expand_dims(Fhi, d + a) - ops['phiL'].reshape(sh) * np.expand_dims(Flo, d + a)) / w.reshape(sh)
    if stages:
        return dict(ustar=us, traces=tr, unew=un)
    return un


def face_positions(nc, N, ops, dx, axis, side, origin=None):
    """[grid without axis, face nodes (dim - 1 axes), 3]: the face nodes of the domain face (axis, side); `origin`: of the block (a shard's
    includes its offset)."""
    dim = len(nc)
    origin = np.zeros(dim) if origin is None else np.asarray(origin)
    others = [a for a in range(dim) if a != axis]
    k = len(others)
    X = np.zeros(tuple(nc[a] for a in others) + (N,) * k + (3,), dtype=ops['xi'].dtype)
    for j, a in enumerate(others):
        cs, ns = [1] * (2 * k), [1] * (2 * k)
        cs[j], ns[k + j] = nc[a], N
        X[..., a] = origin[a] + (np.arange(nc[a]).reshape(cs) + ops['xi'].reshape(ns)) * dx[a]
    X[..., axis] = origin[axis] + (nc[axis] if side else 0) * dx[axis]
    return X


def sees_xt(pde):
    """True for a term set with flux(q, x, t, a) (aderdg_numpy.step_xt's interface), False for flux(q, a)"""
    return len(inspect.signature(pde.flux).parameters) == 4


def _flux(pde, q, X, t, axis):
    return pde.flux(q, [X[..., 0], X[..., 1], X[..., 2]], t, axis) if sees_xt(pde) else pde.flux(q, axis)


def maxeig_at(pde, q, X, t, axis):
    """the eigenvalue bound of states q at the positions X[..., 3] and time t, for either interface"""
    if sees_xt(pde):
        return pde.maxeig(q, [X[..., 0], X[..., 1], X[..., 2]], t, axis) * np.ones(q.shape[:-1], dtype=q.dtype)
    return pde.maxeig(q, axis)


def dirichlet_levels(t, dt, ops, midpoint=False):
    """(weights, times) of the average: the Gauss levels t + xi_l dt, or (a mutant / a constant state without x, t) one level at t + dt / 2"""
    if midpoint:
        return [1.0], [t + 0.5 * dt]
    return list(ops['w']), [t + xl * dt for xl in ops['xi']]


def dirichlet_ghost(f, pde, X, axis, t, dt, ops, constant=False, midpoint=False, flux_X=None):
    """(qg, Fg) = sum_l w_l (q_l, F_axis(q_l, X, t_l)) over the Gauss levels t_l = t + xi_l dt, q_l = f(X, t_l); constant: f is the state, qg
    the state itself and Fg the average of ITS flux (one evaluation for a term set that sees neither x nor t).  X: face_positions(...), the
    origin included.  Mutants: midpoint (one level at t + dt / 2), flux_X (the flux evaluated at other positions than f)."""
    FX = X if flux_X is None else flux_X
    if constant:
        q = np.broadcast_to(np.asarray(f, dtype=X.dtype), X.shape[:-1] + (len(f),)).copy()
        if not sees_xt(pde):
            return q, pde.flux(q.copy(), axis)
        Fg = 0.0
        for wl, tl in zip(*dirichlet_levels(t, dt, ops, midpoint)):
            Fg = Fg + wl * _flux(pde, q, FX, tl, axis)
        return q, Fg
    qg, Fg = 0.0, 0.0
    for wl, tl in zip(*dirichlet_levels(t, dt, ops, midpoint)):
        q = f(X, tl)
        qg = qg + wl * q
        Fg = Fg + wl * _flux(pde, q, FX, tl, axis)
    return qg, Fg


def dirichlet_max_eigenvalue(f, pde, X, times, dim, constant=False):
    """max over the times, the face nodes X and the directions of the eigenvalue of f(X, t) (constant: of the state f): what the boundary
    kernel folds into its scalar over a step's levels, and what AderDgSolver.run evaluates at the current time before its first step."""
    best = 0.0
    for tl in times:
        q = np.broadcast_to(np.asarray(f, dtype=X.dtype), X.shape[:-1] + (len(f),)) if constant else f(X, tl)
        best = max([best] + [float(np.max(maxeig_at(pde, q, X, tl, a))) for a in range(dim)])
    return best


def mirror_x(u, momentum=1):
    """The mirror image of a DG state across its low x face: cells and nodes reversed along x, the x momentum negated."""
    d = A._dim(u)
    m = np.flip(np.flip(u, axis=0), axis=d).copy()
    m[..., momentum] *= -1.0
    return m
