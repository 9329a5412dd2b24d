"""Reverse mode of the Navier-Stokes side: the solver's transposed Jacobian apply (_get_dresiduals_T), the adjoint
Schur operator (_SchurComplementT) and the adjoint update (_get_update_T), and the component's opt-in mode='rev',
against SciPy on the pinned oracle's matrices and against the forward methods (dot-product identities).

The reference matrix is the block form of the operator A of _get_dresiduals at dT = 0, assembled from the oracle,

    A = [ J  B ]    J = NSOracle.Jvelo,  B = (1 - m) [G_x; G_y],  C = (1 - m_c) [G_x, G_y],  E = diag(m_b) K + e_pin e_pin^T
        [ C  E ]    (m = mask_bound, pin = int(N / 2), m_c = m + pin, m_b = m - pin)

and checked against NSOracle.dresiduals on a random vector to 1e-13.  The meshes have odd element counts in both
directions on purpose: with an even nex or ney the equal-order Jacobian with the pin at int(N / 2) is singular
(cond 1e17 - 1e19), a random right-hand side is then inconsistent for the forward and the transposed system alike and
the mass-preconditioned GMRES stalls in both directions; on the six meshes below cond(A) is 5e4 - 2e7.  Every case
asserts cond(A) <= 1e9, so a change of fixture cannot quietly move onto a singular case.

Bars: the applies 1e-12 (the CD adjoint test's), the Schur operator 1e-10 against SciPy (the velocity solve's forward-
error bar in test_gpu_nd_transpose.py) and 1e-11 against the composed matvec (test_nd_gemv_forms_agree's bar for another
summation order carried through the solve), the solve's pressure rows 1.01 mtol sqrt(N) (the CD adjoint test's factor)
and its velocity rows 1e-13 normwise backward error (_solve_T_checks' measure)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

from velocity_blocks import oracle_velocity_jacobian

pytestmark = pytest.mark.gpu
MTOL = 1e-10
GR = 30.0
MESHES = [(2, 3, 3, 100.0), (4, 3, 3, 100.0), (4, 5, 3, 200.0), (6, 3, 5, 100.0), (8, 3, 3, 100.0), (12, 3, 3, 100.0)]


def rel(a, b):
    return np.abs(np.asarray(a) - b).max() / max(np.abs(b).max(), 1e-300)


def close_dot(lhs, rhs, tol):
    print(f"lhs {lhs:.15e} rhs {rhs:.15e} diff {abs(lhs - rhs):.3e}")
    return abs(lhs - rhs) <= tol * max(abs(lhs), abs(rhs))


class _Blocks:
    """The block form of A from the oracle at its linearisation."""

    def __init__(self, ref):
        N = ref.N
        m = ref.mask_bound
        pin = int(N / 2)
        e = np.zeros(N, dtype=bool)
        e[pin] = True
        free, m_c, m_b = (~m).astype(float), m | e, m & ~e
        G = sp.vstack([ref.Gx, ref.Gy]).tocsr()                       # 2N x N
        self.J = ref.Jvelo.tocsr()
        self.B = sp.diags(np.hstack((free, free))) @ G
        self.C = sp.diags((~m_c).astype(float)) @ sp.hstack([ref.Gx, ref.Gy]).tocsr()
        self.E = (sp.diags(m_b.astype(float)) @ ref.K + sp.diags(e.astype(float))).tocsr()
        self.A = sp.bmat([[self.J, self.B], [self.C, self.E]], format="csr")
        self.N, self.pin, self.mask = N, pin, m
        r = np.random.default_rng(99)
        d = r.uniform(-1, 1, 3 * N)
        want = np.hstack(ref.dresiduals(d[:N], d[N:2 * N], d[2 * N:]))
        assert rel(self.A @ d, want) <= 1e-13
        s = np.linalg.svd(self.A.toarray(), compute_uv=False)
        self.cond = s[0] / s[-1]


@functools.lru_cache(maxsize=None)
def case(P, nex, ney, Re):
    """(oracle, its block matrix, the device solver) linearised at the same smooth seeded state."""
    ref, u, v = oracle_velocity_jacobian(P, nex, ney, Re, seed=P + nex, smooth=0.3)
    blk = _Blocks(ref)
    blk.state = (u, v)
    print(f"cond(A) = {blk.cond:.3e}")
    assert blk.cond <= 1e9
    return ref, blk, _solver(P, nex, ney, Re, u, v)


def _solver(P, nex, ney, Re, u, v, **kw):
    """A device solver linearised at (u, v)."""
    from sem_amd.solvers import NavierStokesSolver
    s = NavierStokesSolver(1.0, 1.0, Re, GR, P, nex, ney, u_N=1.0, iprint=[], mtol=MTOL, **kw)
    s._get_residuals(u, v, np.zeros(s.N), np.zeros(s.N))
    s._calc_jacobians(u, v)
    return s


@pytest.mark.parametrize("P,nex,ney,Re", MESHES)
def test_get_dresiduals_T(gpu, P, nex, ney, Re):
    ref, blk, s = case(P, nex, ney, Re)
    assert blk.cond <= 1e9
    N = s.N
    rng = np.random.default_rng(22)
    w = rng.uniform(-1, 1, 3 * N)
    bars = s._get_dresiduals_T(w[:N], w[N:2 * N], w[2 * N:], want_T=True)
    assert len(bars) == 4 and all(isinstance(b, np.ndarray) for b in bars)
    want = blk.A.T @ w
    for k, name in enumerate(("du_bar", "dv_bar", "dp_bar")):
        err = rel(bars[k], want[k * N:(k + 1) * N])
        print(f"{name}: {err:.3e}")
        assert err <= 1e-12, name
    dT_ref = -(GR / Re) * (ref.M @ ((~blk.mask) * w[N:2 * N]))
    err = rel(bars[3], dT_ref)
    print(f"dT_bar: {err:.3e}")
    assert err <= 1e-12
    assert len(s._get_dresiduals_T(w[:N], w[N:2 * N], w[2 * N:])) == 3
    # the dot identity, the dT path included
    d = rng.uniform(-1, 1, 4 * N)
    fwd = np.hstack(s._get_dresiduals(d[:N], d[N:2 * N], d[2 * N:3 * N], d[3 * N:]))
    assert close_dot(np.dot(fwd, w), np.dot(d, np.hstack(bars)), 1e-12)
    # tensor in -> tensors out
    outs = s._get_dresiduals_T(*(s._dev(w[k * N:(k + 1) * N]) for k in range(3)))
    assert all(isinstance(t, torch.Tensor) and t.device == s._mesh.device for t in outs)
    assert rel(outs[2].cpu().numpy(), want[2 * N:]) <= 1e-12


@pytest.mark.parametrize("P,nex,ney,Re", MESHES)
def test_schur_operator_T(gpu, P, nex, ney, Re):
    import importlib.util
    import os
    from sem_amd.solvers.navier_stokes import _SchurComplementT
    spec = importlib.util.spec_from_file_location("ns_adjoint_composed", os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "ns_adjoint_composed.py"))
    composed = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(composed)
    ref, blk, s = case(P, nex, ney, Re)
    assert blk.cond <= 1e9
    vs = s._velocity_solver_T()
    q = np.random.default_rng(7).uniform(-1, 1, s.N)
    want = blk.E.T @ q - blk.B.T @ spla.spsolve(blk.J.T.tocsc(), blk.C.T @ q)
    op = _SchurComplementT(s, vs, graph=True)
    assert op._graph is not None
    tq = s._dev(q)
    got = op(tq)
    err = rel(got.cpu().numpy(), want)
    print(f"S^T q against SciPy: {err:.3e}")
    assert err <= 1e-10
    eager = op._body(tq)
    assert torch.equal(got, eager) and torch.equal(op(tq), eager)
    comp = composed.ComposedSchurT(s, vs)(tq)
    err = float((eager - comp).abs().max() / comp.abs().max())
    print(f"fused against composed: {err:.3e}")
    assert err <= 1e-11


def _forward_update(s, rhs):
    return [np.asarray(a) for a in s._get_update(*rhs)]


@pytest.mark.parametrize("P,nex,ney,Re", MESHES)
def test_get_update_T(gpu, P, nex, ney, Re):
    ref, blk, _ = case(P, nex, ney, Re)
    assert blk.cond <= 1e9
    # a solver of its own (the test switches its graphs off and on): one factor throughout, first without graphs
    s = _solver(P, nex, ney, Re, *blk.state, velocity_graph=False)
    N = s.N
    rng = np.random.default_rng(23)
    b = rng.uniform(-1, 1, 3 * N)
    rhs = [rng.uniform(-1, 1, N) for _ in range(3)]
    f_eager = _forward_update(s, rhs)           # the forward update before any adjoint call
    lam = s._get_update_T(b[:N], b[N:2 * N], b[2 * N:])
    assert all(isinstance(a, np.ndarray) for a in lam)
    first = s.schur_matvecs
    assert first > 0
    x = np.hstack(lam)
    res = blk.A.T @ x - b
    res_p = np.linalg.norm(res[2 * N:])
    print(f"adjoint GMRES: {first} matvecs, pressure-row residual {res_p:.3e}, bound {1.01 * MTOL * np.sqrt(N):.3e}")
    assert res_p <= 1.01 * MTOL * np.sqrt(N)
    # velocity rows: J^T lam_uv = b_uv - C^T lam_c, normwise backward error in _solve_T_checks' measure
    JT = blk.J.T.tocsr()
    bv = b[:2 * N] - blk.C.T @ x[2 * N:]
    eta = np.abs(JT @ x[:2 * N] - bv).max() / (abs(JT).sum(axis=1).max() * np.abs(x[:2 * N]).max() + np.abs(bv).max())
    print(f"velocity rows: backward error {eta:.3e}")
    assert eta <= 1e-13
    for a, w in zip(_forward_update(s, rhs), f_eager):      # the forward update is bit for bit what it was
        assert np.array_equal(a, w)
    # the same with every graph captured (both solves, both Schur operators)
    s._velocity_graph = True
    s._schur = s._schur_T = None
    vs = s._velocity_solver()
    assert vs.capture() and vs.capture_T()
    f_graph = _forward_update(s, rhs)
    # restarted from its own solution the adjoint solve needs no more matvecs
    s._get_update_T(b[:N], b[N:2 * N], b[2 * N:], dres_c0=lam[2])
    print(f"second call from lam_c: {s.schur_matvecs} matvecs")
    assert s.schur_matvecs <= first
    assert s._schur_T._graph is not None
    for a, w in zip(_forward_update(s, rhs), f_graph):
        assert np.array_equal(a, w)


def test_refusals(gpu):
    from sem_amd.solvers import NavierStokesSolver
    ref, u, v = oracle_velocity_jacobian(4, 3, 3, 100.0, seed=1, smooth=0.3)
    z = np.zeros(ref.N)

    def solver(**kw):
        s = NavierStokesSolver(1.0, 1.0, 100.0, 0.0, 4, 3, 3, u_N=1.0, iprint=[], **kw)
        s._get_residuals(u, v, z, z)
        return s

    s = solver()
    with pytest.raises(RuntimeError, match="_calc_jacobians must run before"):     # before the linearisation
        s._get_dresiduals_T(z, z, z)
    with pytest.raises(RuntimeError, match="_calc_jacobians must run before"):
        s._get_update_T(z, z, z)
    s = solver(velocity_interior="nested")                  # the line condensation: no transposed solve
    s._calc_jacobians(u, v)
    with pytest.raises(ValueError, match="nested-dissection"):
        s._get_update_T(z, z, z)
    s = solver(schur_precond="pcd")                         # no transposed A_p solve; no silent switch
    s._calc_jacobians(u, v)
    with pytest.raises(ValueError, match="schur_precond='mass'"):
        s._get_update_T(z, z, z)
    s = solver()
    s._calc_jacobians(u, v)
    s._part = object()                                      # a partitioned solver refuses before anything else
    for call in (lambda: s._get_update_T(z, z, z), lambda: s._get_dresiduals_T(z, z, z)):
        with pytest.raises(ValueError, match="whole-mesh"):
            call()


@functools.lru_cache(maxsize=None)
def component_pair():
    """An NS solver on 3 x 3 elements of P = 4 (odd x odd: the system is regular) and a CD solver on the mismatched
    2 x 3 elements of P = 3, as test_gpu_adjoint_solver.transfer_pair."""
    from sem_amd.solvers import ConvectionDiffusionSolver, NavierStokesSolver
    ns = NavierStokesSolver(1.0, 1.0, 100.0, GR, 4, 3, 3, u_N=1.0, iprint=[], mtol=MTOL)
    cd = ConvectionDiffusionSolver(1, 1, 40, 3, 2, 3, T_W=0.5, T_E=-0.5, mtol=MTOL)
    return ns, cd


def _component(adjoint):
    from sem_amd.solvers.components import NavierStokes_Component
    ns, cd = component_pair()
    c = NavierStokes_Component(solver_NS=ns, solver_CD=cd, **({"adjoint": True} if adjoint else {}))
    c.setup()
    ref, u, v = oracle_velocity_jacobian(4, 3, 3, 100.0, seed=7, smooth=0.3)
    rng = np.random.default_rng(41)
    inp = {"T_cd": rng.uniform(-1, 1, cd.N)}
    out = {"u_ns": u, "v_ns": v, "p_ns": rng.uniform(-1, 1, ns.N)}
    c.apply_nonlinear(inp, out, {})
    c.linearize(inp, out, None)
    return c, ns, cd, ref, inp, out, rng


def test_component_reverse_mode(gpu):
    from sem_amd.solvers.components import transfer_T
    c, ns, cd, ref, inp, out, rng = _component(True)
    blk = _Blocks(ref)
    print(f"cond(A) = {blk.cond:.3e}")
    assert blk.cond <= 1e9
    N = ns.N
    names = ("u_ns", "v_ns", "p_ns")
    w = {n: rng.uniform(-1, 1, N) for n in names}
    bars = ns._get_dresiduals_T(*(w[n] for n in names), want_T=True)
    want = dict(zip(names, bars[:3]), T_cd=transfer_T(bars[3], cd, ns))
    pre = {n: rng.uniform(-1, 1, N) for n in names}
    pre["T_cd"] = rng.uniform(-1, 1, cd.N)
    dout, din = {n: pre[n].copy() for n in names}, {"T_cd": pre["T_cd"].copy()}
    c.apply_linear(inp, out, din, dout, dict(w), "rev")
    for n in names:
        assert np.array_equal(dout[n], pre[n] + want[n]), n
    assert np.array_equal(din["T_cd"], pre["T_cd"] + want["T_cd"])
    # absent entries are skipped; an absent d_residuals entry counts as zero
    dout, din = {"v_ns": pre["v_ns"].copy()}, {}
    c.apply_linear(inp, out, din, dout, {"u_ns": w["u_ns"], "p_ns": w["p_ns"]}, "rev")
    assert din == {} and list(dout) == ["v_ns"]
    part = ns._get_dresiduals_T(w["u_ns"], np.zeros(N), w["p_ns"])
    assert np.array_equal(dout["v_ns"], pre["v_ns"] + part[1])
    # dot identity against forward mode
    d = {n: rng.uniform(-1, 1, N) for n in names}
    dT = rng.uniform(-1, 1, cd.N)
    dres = {}
    c.apply_linear(inp, out, {"T_cd": dT}, dict(d), dres, "fwd")
    lhs = sum(np.dot(dres[n], w[n]) for n in names)
    rhs = sum(np.dot(d[n], want[n]) for n in names) + np.dot(dT, want["T_cd"])
    assert close_dot(lhs, rhs, 1e-12)
    # adjoint solve
    b = {n: rng.uniform(-1, 1, N) for n in names}
    dres = {n: np.zeros(N) for n in names}
    before = c.iter_count_solve
    c.solve_linear(dict(b), dres, "rev")
    assert c.iter_count_solve == before + 1
    x, bb = np.hstack([dres[n] for n in names]), np.hstack([b[n] for n in names])
    res = blk.A.T @ x - bb
    res_p = np.linalg.norm(res[2 * N:])
    print(f"component adjoint solve: pressure-row residual {res_p:.3e}, bound {1.01 * MTOL * np.sqrt(N):.3e}")
    assert res_p <= 1.01 * MTOL * np.sqrt(N)
    JT = blk.J.T.tocsr()
    bv = bb[:2 * N] - blk.C.T @ x[2 * N:]
    eta = np.abs(JT @ x[:2 * N] - bv).max() / (abs(JT).sum(axis=1).max() * np.abs(x[:2 * N]).max() + np.abs(bv).max())
    print(f"velocity rows: backward error {eta:.3e}")
    assert eta <= 1e-13
    dres2 = {"u_ns": np.zeros(N), "v_ns": np.zeros(N)}      # no initial guess for the Schur solve
    c.solve_linear(dict(b), dres2, "rev")
    assert set(dres2) == set(names) and c.iter_count_solve == before + 2


def test_component_default_stays_forward_only(gpu):
    c, ns, cd, ref, inp, out, rng = _component(False)
    assert c.options["adjoint"] is False
    z = {n: np.zeros(ns.N) for n in ("u_ns", "v_ns", "p_ns")}
    with pytest.raises(ValueError, match="only forward mode implemented"):
        c.apply_linear({}, {}, {"T_cd": np.zeros(cd.N)}, dict(z), dict(z), "rev")
    with pytest.raises(ValueError, match="only forward mode implemented"):
        c.solve_linear(dict(z), dict(z), "rev")
