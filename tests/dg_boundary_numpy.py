"""Numpy restatement of one ADER-DG step on a NON-periodic box: the local stages of oracle/aderdg_numpy.py (predictor, time averages,
volume, traces) unchanged, then a Riemann solve that takes the state beyond a domain face from a ghost trace, and the corrector.

bcs: {(axis, side): ("outflow",) | ("wall", s[V]) | ("dirichlet", (qg, Fg))} with qg, Fg the ghost's time-averaged state and normal flux,
shaped like one face slice of the traces (grid without `axis`, face nodes, var).  A face not named is periodic."""
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
        return s * q_in, -s * F_in
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
    """One step with boundary ghosts; bcs values may also be callables (traces) -> bc, for ghosts that need the step's traces."""
    d = A._dim(u)
    q = A.predictor(u, dt, dx, ops, pde, n_it)
    qbar, Fbar = A.time_averages(q, ops, pde)
    us = A.volume(u, Fbar, dt, dx, ops)
    tr = A.traces(qbar, Fbar, ops)
    Ff = [riemann_faces(tr[a], pde, a, d, bcs) for a in range(d)]
    un = corrector(us, Ff, dt, dx, ops)
    if stages:
        return dict(traces=tr, Ffaces=Ff, ustar=us, unew=un)
    return un


def face_positions(nc, N, ops, dx, axis, side, origin=None):
    """[grid without axis, face nodes (dim - 1 axes), 3]: the face nodes of the domain face (axis, side)."""
    dim = len(nc)
    origin = np.zeros(dim) if origin is None else np.asarray(origin)
    others = [a for a in range(dim) if a != axis]
    k = len(others)
    X = np.zeros(tuple(nc[a] for a in others) + (N,) * k + (3,))
    for j, a in enumerate(others):
        cs, ns = [1] * (2 * k), [1] * (2 * k)
        cs[j], ns[k + j] = nc[a], N
        X[..., a] = origin[a] + (np.arange(nc[a]).reshape(cs) + ops['xi'].reshape(ns)) * dx[a]
    X[..., axis] = origin[axis] + (nc[axis] if side else 0) * dx[axis]
    return X


def dirichlet_ghost(f, pde, X, axis, t, dt, ops, constant=False):
    """(qg, Fg): the time average over the Gauss levels t + xi_l dt of f(X, t_l) and of its flux along axis (constant: f is the state)."""
    if constant:
        q = np.broadcast_to(np.asarray(f, dtype=float), X.shape[:-1] + (len(f),))
        return q.copy(), pde.flux(q.copy(), axis)
    qg, Fg = 0.0, 0.0
    for wl, xl in zip(ops['w'], ops['xi']):
        q = f(X, t + xl * dt)
        qg = qg + wl * q
        Fg = Fg + wl * pde.flux(q, axis)
    return qg, Fg


def mirror_x(u, momentum=1):
    """The mirror image of a DG state across its low x face: cells and nodes reversed along x, the x momentum negated."""
    d = A._dim(u)
    m = np.flip(np.flip(u, axis=0), axis=d).copy()
    m[..., momentum] *= -1.0
    return m
