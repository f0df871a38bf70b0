"""Term sets given as SymPy expressions, shared by tests/test_user_pde.py (their first home: names and expressions are unchanged, so the
content-addressed side libraries are the same ones), the case table tests/fv_user_cases.py and the tests built on it."""
import sympy

G = 9.81


def swe():
    from exahype_amd.pde_codegen import SympyPDE

    def flux(q, d):
        h, hu, hv = q
        un = (hu, hv)[d] / h if d < 2 else 0
        p = sympy.Rational(1, 2) * G * h * h
        f = [h * un, hu * un, hv * un]
        if d < 2:
            f[1 + d] = f[1 + d] + p
        return f

    def eig(q, d):
        h, hu, hv = q
        un = (hu, hv)[d] / h if d < 2 else 0
        return sympy.Abs(un) + sympy.sqrt(G * h)
    return SympyPDE(3, flux, eig, max_dim=2, name="shallow_water")


def euler_sympy():
    from exahype_amd.pde_codegen import SympyPDE

    def prim(q):
        irho = 1 / q[0]
        p = sympy.Float(0.4) * (q[4] - sympy.Rational(1, 2) * irho * (q[1] ** 2 + q[2] ** 2 + q[3] ** 2))
        return irho, p

    def flux(q, d):
        irho, p = prim(q)
        c = irho * q[d + 1]
        f = [c * q[0], c * q[1], c * q[2], c * q[3], c * q[4] + c * p]
        f[d + 1] = f[d + 1] + p
        return f

    def eig(q, d):
        irho, p = prim(q)
        return sympy.Abs(q[d + 1] * irho) + sympy.sqrt(sympy.Float(1.4) * p * irho)
    return SympyPDE(5, flux, eig, max_dim=3, name="euler_from_sympy")


def euler_gravity(g=(0.3, -0.5, 0.8)):
    """Compressible Euler with a constant body force: a NONLINEAR five-variable system with a source, S = (0, rho g, m . g)."""
    from exahype_amd.pde_codegen import SympyPDE
    base = euler_sympy()
    q = base.q
    return SympyPDE(5, flux=lambda qq, d: [e.subs(dict(zip(q, qq))) for e in base.flux_exprs[d]],
                    max_eigenvalue=lambda qq, d: base.eig_exprs[d].subs(dict(zip(q, qq))),
                    source=lambda qq: [0, qq[0] * g[0], qq[0] * g[1], qq[0] * g[2], qq[1] * g[0] + qq[2] * g[1] + qq[3] * g[2]],
                    max_dim=3, name="euler_gravity")


def two_layer_like(max_dim=2):
    """A system with a flux AND a non-conservative product (the shape of two-layer shallow water: the coupling of the layers is B(q) grad q):
    q0_t + div(a q0) + k q1 grad q0 = 0,  q1_t + div(b q1) + k q0 grad q1 = 0."""
    from exahype_amd.pde_codegen import SympyPDE
    a, b, k = (1.0, 0.5, -0.25), (0.75, -0.5, 0.5), 0.3
    return SympyPDE(2, flux=lambda q, d: [a[d] * q[0], b[d] * q[1]], max_eigenvalue=lambda q, d: sympy.Float(1.5),
                    ncp=lambda q, dq, d: [k * q[1] * dq[0], k * q[0] * dq[1]], max_dim=max_dim, name="two_layer_like")


def coupled_rational(max_dim=3):
    """The three fields of tests/test_user_pde.py's coupled_xt_ncp_system with polynomial / rational dependence on position and time in place of
    sin and cos (no libm call: every operation of the device code is an IEEE +, *, /, whose rounding the reference counts).  Flux, eigenvalue,
    source and ncp all see x and t, with coefficients of order 0.1 to 1; the advection velocity along d depends on x[d] itself, so the terms of
    the neighbours along d (at x_c +- h e_d) and of the faces (x_c +- h/2 e_d) differ from those at x_c in the second digit."""
    from exahype_amd.pde_codegen import SympyPDE
    R = sympy.Rational

    def vel(x, t, d):
        o = x[(d + 1) % max_dim]
        return (1, R(-1, 2), R(3, 4))[d] + R(3, 10) * x[d] - R(1, 5) * o * t + R(1, 4) * t / (1 + x[d] ** 2)
    flux = lambda q, x, t, d: [vel(x, t, d) * q[0], R(3, 4) * vel(x, t, d) * q[1] + R(1, 5) * q[0] * q[2], R(1, 2) * vel(x, t, d) * q[2]]
    eig = lambda q, x, t, d: sympy.Abs(vel(x, t, d)) + R(1, 5) * sympy.Abs(q[0])
    source = lambda q, x, t: [x[0] * (1 - R(1, 2) * t ** 2) - q[0] * x[1], q[0] - 2 * q[1] + t, R(1, 2) * q[1] * x[0] + R(1, 5) * q[2] * x[max_dim - 1] * t]
    ncp = lambda q, dq, x, t, d: [R(3, 10) * (1 + R(1, 2) * x[d]) * q[1] * dq[0], (R(1, 5) + R(1, 10) * x[d]) * q[0] * dq[2], R(1, 4) * dq[1] * (1 + t)]
    return SympyPDE(3, flux=flux, max_eigenvalue=eig, source=source, ncp=ncp, max_dim=max_dim, name="coupled_rational")
