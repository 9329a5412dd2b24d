"""Reverse mode of the convection-diffusion side: the solver's transposed Jacobian apply and adjoint
solve, the transposed grid transfer and the component's opt-in mode='rev', against SciPy transposes
of the pinned oracle's matrices and against the forward methods (dot-product identities).

Solver-level applies are held to 1e-12 (the component tests' bar), the transfer to 1e-13.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import sem_oracle as O

pytestmark = pytest.mark.gpu
MTOL = 1e-10


def rel(a, b):
    return np.abs(np.asarray(a) - b).max() / max(np.abs(b).max(), 1e-300)


def close_dot(lhs, rhs, tol):
    print(f"lhs {lhs:.15e} rhs {rhs:.15e} diff {abs(lhs - rhs):.3e}")
    return abs(lhs - rhs) <= tol * max(abs(lhs), abs(rhs))


def identity_rows(A, mask):
    L = sp.lil_matrix(A)
    for p in np.flatnonzero(mask):
        L.rows[p], L.data[p] = [int(p)], [1.0]
    return L.tocsr()


@functools.lru_cache(maxsize=None)
def cd_case():
    """The 4x4, P = 4 solver after _get_residuals and _calc_jacobians, and its oracle."""
    from sem_amd.solvers import ConvectionDiffusionSolver
    s = ConvectionDiffusionSolver(1, 1, 40, 4, 4, 4, T_W=0.5, T_E=-0.5, mtol=MTOL)
    o = O.CDOracle(1, 1, 40, 4, 4, 4, T_W=0.5, T_E=-0.5)
    rng = np.random.default_rng(21)
    T, u, v = (rng.uniform(-1, 1, s.N) for _ in range(3))
    s._get_residuals(T, u, v)
    s._calc_jacobians(T)
    o.residuals(T, u, v)
    o.calc_jacobians(T)
    AD = identity_rows(o.Sys, o.mask)
    return s, o, AD


def test_get_dresiduals_T(gpu):
    s, o, AD = cd_case()
    rng = np.random.default_rng(22)
    w, dT, du, dv = (rng.uniform(-1, 1, s.N) for _ in range(4))
    dT_bar, du_bar, dv_bar = s._get_dresiduals_T(w)
    free = ~o.mask
    refs = (AD.T @ w, o.JTu.diagonal() * free * w, o.JTv.diagonal() * free * w)
    for name, got, ref in zip(("dT_bar", "du_bar", "dv_bar"), (dT_bar, du_bar, dv_bar), refs):
        assert isinstance(got, np.ndarray)
        err = rel(got, ref)
        print(f"{name}: {err:.3e}")
        assert err <= 1e-12, name
    lhs = np.dot(s._get_dresiduals(dT, du, dv), w)
    rhs = np.dot(dT, dT_bar) + np.dot(du, du_bar) + np.dot(dv, dv_bar)
    assert close_dot(lhs, rhs, 1e-12)
    # tensor in -> tensors out
    outs = s._get_dresiduals_T(s._dev(w))
    assert all(hasattr(t, "device") and t.device == s._mesh.device for t in outs)
    assert rel(outs[0].cpu().numpy(), refs[0]) <= 1e-12


def test_get_update_T(gpu):
    from sem_amd.solvers import ConvectionDiffusionSolver
    s, o, AD = cd_case()
    rng = np.random.default_rng(23)
    b, r = rng.uniform(-1, 1, s.N), rng.uniform(-1, 1, s.N)
    lam = s._get_update_T(b)
    res = np.linalg.norm(AD.T @ lam - b)
    print(f"adjoint GMRES: {s.matvecs} matvecs, residual {res:.3e}, bound {1.01 * MTOL * np.sqrt(s.N):.3e}")
    assert s.matvecs > 0
    assert res <= 1.01 * MTOL * np.sqrt(s.N)
    assert close_dot(np.dot(lam, r), np.dot(b, s._get_update(r)), 1e-7)
    # a partitioned solver has no transposed strip apply: the methods' guard raises
    part = object.__new__(ConvectionDiffusionSolver)
    part._part = object()
    with pytest.raises(ValueError, match="whole-mesh"):
        part._get_update_T(b)
    with pytest.raises(ValueError, match="whole-mesh"):
        part._get_dresiduals_T(b)


@functools.lru_cache(maxsize=None)
def transfer_pair():
    """Source P = 3 on 2x3 elements (N = 70), destination P = 4 on 3x2 elements: the meshes do not
    match, so destination nodes fall inside source elements and on their edges."""
    from sem_amd.solvers import ConvectionDiffusionSolver
    src = ConvectionDiffusionSolver(1, 1, 40, 3, 2, 3, T_W=0.5, T_E=-0.5, mtol=MTOL)
    dst = ConvectionDiffusionSolver(1, 1, 40, 4, 3, 2, T_W=0.5, T_E=-0.5, mtol=MTOL)
    return src, dst


def test_transfer_T(gpu):
    from sem_amd import SEM
    from sem_amd.interp import eval_interpolation_adjoint
    from sem_amd.solvers.components import transfer, transfer_T
    src, dst = transfer_pair()
    assert src.N == 70
    Mat = np.stack([transfer(e, src, dst) for e in np.eye(src.N)], axis=1)
    assert Mat.shape == (dst.N, src.N)
    g = np.random.default_rng(31).uniform(-1, 1, dst.N)
    got = transfer_T(g, src, dst)
    assert got.shape == (src.N,)
    err = rel(got, Mat.T @ g)
    print(f"transfer_T: {err:.3e}")
    assert err <= 1e-13
    # plot points outside the domain (x > L_x) contribute nothing
    grid = np.array(np.meshgrid([0.05, 0.5, 0.77, 1.2, 1.4], [0.0, 0.31, 1.0], indexing="ij"))
    ob = np.random.default_rng(32).uniform(-1, 1, grid.shape[1:])
    ueb = eval_interpolation_adjoint(ob, src.points_e, grid)
    ue = np.random.default_rng(33).uniform(-1, 1, ueb.shape)
    fwd = SEM.eval_interpolation(ue, src.points_e, grid)
    assert np.all(fwd[3:] == 0.0)
    assert close_dot(np.sum(fwd * ob), np.sum(ue * ueb), 1e-13)
    ob2 = ob.copy()
    ob2[3:] += 5.0
    assert np.array_equal(eval_interpolation_adjoint(ob2, src.points_e, grid), ueb)
    assert np.all(eval_interpolation_adjoint(ob[3:], src.points_e, grid[:, 3:]) == 0.0)


def test_component_reverse_mode(gpu):
    from sem_amd.solvers.components import ConvectionDiffusion_Component, transfer_T
    ns, cd = transfer_pair()
    c = ConvectionDiffusion_Component(solver_CD=cd, solver_NS=ns, adjoint=True)
    c.setup()
    rng = np.random.default_rng(41)
    inp = {"u_ns": rng.uniform(-1, 1, ns.N), "v_ns": rng.uniform(-1, 1, ns.N)}
    out = {"T_cd": rng.uniform(-1, 1, cd.N)}
    c.apply_nonlinear(inp, out, {})
    c.linearize(inp, out, None)
    w = rng.uniform(-1, 1, cd.N)
    dT_bar, du_bar, dv_bar = cd._get_dresiduals_T(w)
    want = {"T_cd": dT_bar, "u_ns": transfer_T(du_bar, ns, cd), "v_ns": transfer_T(dv_bar, ns, cd)}
    pre = {"T_cd": rng.uniform(-1, 1, cd.N), "u_ns": rng.uniform(-1, 1, ns.N), "v_ns": rng.uniform(-1, 1, ns.N)}
    dout, din = {"T_cd": pre["T_cd"].copy()}, {"u_ns": pre["u_ns"].copy(), "v_ns": pre["v_ns"].copy()}
    c.apply_linear(inp, out, din, dout, {"T_cd": w}, "rev")
    assert np.array_equal(dout["T_cd"], pre["T_cd"] + want["T_cd"])
    assert np.array_equal(din["u_ns"], pre["u_ns"] + want["u_ns"])
    assert np.array_equal(din["v_ns"], pre["v_ns"] + want["v_ns"])
    # absent entries are skipped
    dout, din = {}, {"v_ns": pre["v_ns"].copy()}
    c.apply_linear(inp, out, din, dout, {"T_cd": w}, "rev")
    assert dout == {} and list(din) == ["v_ns"]
    assert np.array_equal(din["v_ns"], pre["v_ns"] + want["v_ns"])
    # dot identity against forward mode
    dT, du, dv = rng.uniform(-1, 1, cd.N), rng.uniform(-1, 1, ns.N), rng.uniform(-1, 1, ns.N)
    dres = {}
    c.apply_linear(inp, out, {"u_ns": du, "v_ns": dv}, {"T_cd": dT}, dres, "fwd")
    rhs = np.dot(dT, want["T_cd"]) + np.dot(du, want["u_ns"]) + np.dot(dv, want["v_ns"])
    assert close_dot(np.dot(dres["T_cd"], w), rhs, 1e-12)
    # adjoint solve
    o = O.CDOracle(1, 1, 40, 4, 3, 2, T_W=0.5, T_E=-0.5)
    o.residuals(out["T_cd"], *c.change_inputs(inp["u_ns"], inp["v_ns"]))
    AD = identity_rows(o.Sys, o.mask)
    b = rng.uniform(-1, 1, cd.N)
    dres = {"T_cd": np.zeros(cd.N)}
    before = c.iter_count_solve
    c.solve_linear({"T_cd": b}, dres, "rev")
    assert c.iter_count_solve == before + 1
    res = np.linalg.norm(AD.T @ dres["T_cd"] - b)
    print(f"component adjoint solve: residual {res:.3e}, bound {1.01 * MTOL * np.sqrt(cd.N):.3e}")
    assert res <= 1.01 * MTOL * np.sqrt(cd.N)


def test_component_default_stays_forward_only(gpu):
    from sem_amd.solvers.components import ConvectionDiffusion_Component
    ns, cd = transfer_pair()
    c = ConvectionDiffusion_Component(solver_CD=cd, solver_NS=ns)
    c.setup()
    assert c.options["adjoint"] is False
    z = np.zeros(cd.N)
    with pytest.raises(ValueError, match="only forward mode implemented"):
        c.apply_linear({}, {}, {}, {"T_cd": z}, {"T_cd": z}, "rev")
    with pytest.raises(ValueError, match="only forward mode implemented"):
        c.solve_linear({"T_cd": z}, {"T_cd": z}, "rev")
