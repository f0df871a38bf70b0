"""ORACLE (test infrastructure only -- never imported by the product path).

One-dimensional ADER-DG reference-element operators on Gauss-Legendre nodes.

Reference anchor: none.  /root/reference contains no ADER-DG code at all
(SURVEY.md F2); these follow SURVEY.md Appendix A.1 (standard nodal ADER-DG,
Dumbser et al. 2008).  "parity unpinned" against the reference; pinned instead
by the operator identities of SURVEY.md A.5 (tests/test_dg_operators.py).
"""
import numpy as np


def gauss_legendre_01(N):
    """Nodes/weights on [0,1] (sum w = 1)."""
    x, w = np.polynomial.legendre.leggauss(N)
    return 0.5 * (x + 1.0), 0.5 * w


def lagrange_eval(nodes, x):
    """phi_j(x) for all j (1-D array)."""
    N = len(nodes)
    out = np.ones(N)
    for j in range(N):
        for k in range(N):
            if k != j:
                out[j] *= (x - nodes[k]) / (nodes[j] - nodes[k])
    return out


def derivative_matrix(nodes):
    """D[i][j] = phi_j'(xi_i) via barycentric weights."""
    N = len(nodes)
    bw = np.ones(N)
    for j in range(N):
        for k in range(N):
            if k != j:
                bw[j] /= (nodes[j] - nodes[k])
    D = np.zeros((N, N))
    for i in range(N):
        for j in range(N):
            if i != j:
                D[i, j] = (bw[j] / bw[i]) / (nodes[i] - nodes[j])
        D[i, i] = -np.sum(D[i, :])
    return D


def operators(N):
    """Return dict of the A.1 operators for polynomial order p = N-1."""
    xi, w = gauss_legendre_01(N)
    D = derivative_matrix(xi)
    Kxi = D.T * w[None, :]          # Kxi[i][j] = w_j * D[j][i]
    phiL = lagrange_eval(xi, 0.0)
    phiR = lagrange_eval(xi, 1.0)
    K1 = np.outer(phiR, phiR) - Kxi
    iK1 = np.linalg.inv(K1)
    return dict(N=N, xi=xi, w=w, D=D, Kxi=Kxi, phiL=phiL, phiR=phiR,
                F0=phiL.copy(), K1=K1, iK1=iK1)


def gauss_legendre_mp(N, dps):
    """Gauss-Legendre nodes and weights on [0, 1] as mpmath numbers (call inside mpmath.workdps(dps)): Newton on P_N (three-term recurrence)
    from the fp64 nodes; w_i = 1 / ((1 - x_i^2) P_N'(x_i)^2) (half the [-1, 1] weight 2 / (...))."""
    import mpmath
    mp = mpmath.mpf

    def legendre(x):
        p0, p1 = mp(1), x
        if N == 0:
            return p0, mp(0)
        for k in range(2, N + 1):
            p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
        return p1, N * (x * p1 - p0) / (x * x - 1)           # P_N, P_N'

    x0, _ = np.polynomial.legendre.leggauss(N)
    xs, ws = [], []
    for g in x0:
        x = mp(float(g))
        for _ in range(100):
            p, dp = legendre(x)
            dx = p / dp
            x -= dx
            if abs(dx) < mp(10) ** (-dps - 2):
                break
        p, dp = legendre(x)
        xs.append((x + 1) / 2)
        ws.append(1 / ((1 - x * x) * dp * dp))
    return xs, ws


_HP_CACHE = {}


def operators_hp(N, dps=40):
    """The operators of `operators(N)` built in mpmath at `dps` digits from closed forms and returned as np.longdouble
    (cached per N): the high-precision reference the fp64 oracles are pinned against (tests/test_dg_reference_hp.py).

    Nodes and weights: gauss_legendre_mp; D from barycentric weights; iK1 by an mpmath inverse."""
    if N in _HP_CACHE:
        return _HP_CACHE[N]
    import mpmath
    with mpmath.workdps(dps):
        mp = mpmath.mpf
        xs, ws = gauss_legendre_mp(N, dps)
        bw = [mp(1)] * N
        for j in range(N):
            for k in range(N):
                if k != j:
                    bw[j] /= xs[j] - xs[k]
        D = mpmath.matrix(N, N)
        for i in range(N):
            for j in range(N):
                if i != j:
                    D[i, j] = (bw[j] / bw[i]) / (xs[i] - xs[j])
            D[i, i] = -sum(D[i, j] for j in range(N) if j != i)

        def lagrange(t):
            out = []
            for j in range(N):
                v = mp(1)
                for k in range(N):
                    if k != j:
                        v *= (t - xs[k]) / (xs[j] - xs[k])
                out.append(v)
            return out
        phiL, phiR = lagrange(mp(0)), lagrange(mp(1))
        Kxi = mpmath.matrix(N, N)
        K1 = mpmath.matrix(N, N)
        for i in range(N):
            for j in range(N):
                Kxi[i, j] = ws[j] * D[j, i]
                K1[i, j] = phiR[i] * phiR[j] - Kxi[i, j]
        iK1 = K1 ** -1

        def ld(v):
            return np.longdouble(mpmath.nstr(v, dps + 5))           # decimal string -> correctly rounded long double

        vec = lambda a: np.array([ld(v) for v in a], dtype=np.longdouble)
        mat = lambda M: np.array([[ld(M[i, j]) for j in range(N)] for i in range(N)], dtype=np.longdouble)
        ops = dict(N=N, xi=vec(xs), w=vec(ws), D=mat(D), Kxi=mat(Kxi), phiL=vec(phiL), phiR=vec(phiR),
                   F0=vec(phiL), K1=mat(K1), iK1=mat(iK1))
    _HP_CACHE[N] = ops
    return ops
