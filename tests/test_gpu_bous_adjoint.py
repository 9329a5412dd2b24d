"""Reverse mode of the Boussinesq coupler on the device solvers: jacobian_apply_T, block_jacobi_T, solve_adjoint,
residual_partials and total_derivatives, against the coupled sparse Jacobian assembled from the oracle's blocks
(tests/adjoint_doubles.py), against the coupler's own forward maps (dot identity) and against finite differences of
its own converged forward solves.

Whatever solves uses odd element counts and even P (J regular); every such case prints cond(J) and asserts it is at
most 1e9, the guard of test_gpu_ns_adjoint.py.  The states of the oracle comparisons are the oracle coupler's converged
solutions (a CPU solve of a second or two), so the device couplers there are linearised without a forward solve.

Bounds: the dot identity 1e-12 (close_dot of test_gpu_ns_adjoint.py); the transposed apply 1e-12 per block; a block's
transposed solve 1.01 mtol sqrt(N) of its solver; the adjoint solve's true residual 1.01 atol_gmres; a total derivative
against the sparse direct -g^T J^-1 dR/dp within 1.01 atol_gmres ||J^-1 dR/dp||_2 + 1e-12 |reference| (its error is
r_adj^T dx/dp); the finite-difference bound is derived in test_finite_difference."""
import functools

import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

import adjoint_doubles as AD
from conftest import golden

pytestmark = pytest.mark.gpu
BASE = dict(Re=1e3, Ra=1e3, Pr=0.71)
PARAMS = ("Ra", "Re", "Pr")
MESHES = [(4, 3, 3), (2, 5, 3)]


def rel(a, b):
    return np.abs(np.asarray(a) - b).max() / max(np.abs(b).max(), 1e-300)


def close_dot(lhs, rhs, tol):
    print(f"lhs {lhs:.15e} rhs {rhs:.15e} diff {abs(lhs - rhs):.3e}")
    return abs(lhs - rhs) <= tol * max(abs(lhs), abs(rhs))


def _functionals():
    from sem_amd.solvers.functionals import KineticEnergy, WallNusselt
    return [WallNusselt("W"), KineticEnergy()]


def _device_coupler(P, nex, ney, **kw):
    from sem_amd.solvers.boussinesq import BoussinesqCoupler
    args = dict(BASE, **{k: kw.pop(k) for k in tuple(kw) if k in BASE})
    return BoussinesqCoupler(1.0, 1.0, args["Re"], args["Ra"], args["Pr"], P, nex, ney, P, nex, ney, **kw)


@functools.lru_cache(maxsize=None)
def oracle_case(P, nex, ney):
    """The oracle coupler converged and linearised at its solution x, the assembled J and cond(J)."""
    ref = AD.coupler(P, nex, ney, **BASE)
    x = np.concatenate(ref.solve())
    ref.residuals(x)
    ref.linearize(x)
    J = AD.coupled_jacobian(ref.cd, ref.ns)
    k = AD.cond(J)
    print(f"cond(J) = {k:.3e}")
    assert k <= 1e9
    return ref, x, J, k


@functools.lru_cache(maxsize=None)
def device_case(P, nex, ney):
    """A device coupler linearised at the oracle's converged state."""
    ref, x, J, k = oracle_case(P, nex, ney)
    c = _device_coupler(P, nex, ney)
    assert c._device
    assert np.linalg.norm(c.residuals(x)) <= c.atol_nonlin
    c.linearize(x)
    return c


# ------------------------------------------------------------------ no solve: the golden seeded states
def _golden_coupler(g, key):
    from sem_amd.solvers.boussinesq import BoussinesqCoupler
    Pc, nxc, nyc, Pn, nxn, nyn = (int(a) for a in g[key + "_cfg"])
    c = BoussinesqCoupler(1.0, 1.0, 1e3, 1e3, 0.71, Pc, nxc, nyc, Pn, nxn, nyn, mode=str(g[key + "_mode"]))
    c.residuals(g[key + "_x"])
    c.linearize(g[key + "_x"])
    return c


@pytest.mark.parametrize("key", ["a", "b"])
def test_dot_identity_golden(gpu, key):
    """<J dx, w> = <dx, J^T w> at the golden seeded states: "a" the same mesh (device mode), "b" CD 4 x 4, P = 4
    against NS 3 x 3, P = 6 (host mode, both transposed mesh transfers).  NumPy in, and in device mode, where the
    working form is a tensor, tensors in; a second call is bitwise the first."""
    g = golden("bous.npz")
    c = _golden_coupler(g, key)
    assert c._device == (key == "a")
    dx = g[key + "_dx"]
    w = np.random.default_rng(17).uniform(-1, 1, c.DOF)
    Jdx = c.jacobian_apply(dx)
    assert np.abs(Jdx - g[key + "_JR"]).max() <= 1e-12 * np.abs(g[key + "_JR"]).max()
    JTw = c.jacobian_apply_T(w)
    assert isinstance(JTw, np.ndarray) and JTw.shape == (c.DOF,)
    assert close_dot(np.dot(Jdx, w), np.dot(dx, JTw), 1e-12)
    assert np.array_equal(c.jacobian_apply_T(w), JTw)
    if c._device:
        tw, tdx = c.to_local(w), c.to_local(dx)
        t = c.jacobian_apply_T(tw)
        assert isinstance(t, torch.Tensor) and t.device == c.cd._mesh.device
        assert close_dot(torch.dot(c.jacobian_apply(tdx), tw).item(), torch.dot(tdx, t).item(), 1e-12)
        assert torch.equal(c.jacobian_apply_T(tw), t)
        assert np.array_equal(t.cpu().numpy(), JTw)
    assert c.calls["jacobian_apply_T"] >= 2 and c.timing["jacobian_apply_T"] > 0.0


# ------------------------------------------------------------------ against the assembled oracle Jacobian
def test_jacobian_apply_T_oracle(gpu):
    ref, x, J, k = oracle_case(4, 3, 3)
    assert k <= 1e9
    c = device_case(4, 3, 3)
    w = np.random.default_rng(5).uniform(-1, 1, c.DOF)
    got, want = c.jacobian_apply_T(w), J.T @ w
    for name, a, b in zip(("dT_bar", "du_bar", "dv_bar", "dp_bar"), np.split(got, 4), np.split(want, 4)):
        print(f"{name}: {rel(a, b):.3e}")
        assert rel(a, b) <= 1e-12, name


def test_block_jacobi_T(gpu):
    """Each block of block_jacobi_T(r) solves its solver's transposed system: residual (against the oracle's
    assembled blocks) at most 1.01 mtol sqrt(N) of that solver."""
    ref, x, J, k = oracle_case(4, 3, 3)
    assert k <= 1e9
    c = device_case(4, 3, 3)
    r = np.random.default_rng(8).uniform(-1, 1, c.DOF)
    z = c.block_jacobi_T(r)
    n = c.Ncd
    res_cd = np.linalg.norm(ref.cd.matrix()[0].T @ z[:n] - r[:n])
    res_ns = np.linalg.norm(ref.ns.matrix()[0].T @ z[n:] - r[n:])
    b_cd, b_ns = 1.01 * c.cd._mtol * np.sqrt(c.Ncd), 1.01 * c.ns._mtol * np.sqrt(c.Nns)
    print(f"CD block: residual {res_cd:.3e} bound {b_cd:.3e}; NS block: residual {res_ns:.3e} bound {b_ns:.3e}")
    assert c.calls["cd_update_T"] >= 1 and c.calls["ns_update_T"] >= 1
    assert res_cd <= b_cd
    assert res_ns <= b_ns


def _reference_derivatives(ref, x, J, functionals):
    lu = spla.splu(J.tocsc())
    out, scale = {}, {}
    for p in PARAMS:
        dxdp = lu.solve(ref.residual_partials(x, p))
        scale[p] = np.linalg.norm(dxdp)
        for F in functionals:
            out[(F.name, p)] = -float(np.dot(F.gradient(ref, x), dxdp))
    return out, scale


@pytest.mark.parametrize("P,nex,ney", MESHES)
def test_solve_adjoint_and_derivatives(gpu, P, nex, ney):
    """solve_adjoint's true residual and total_derivatives for Ra, Re, Pr on the device solvers; the reference (J,
    the functionals' gradients, dR/dp) is the oracle's throughout.  3 x 3, P = 4 goes in as global NumPy vectors,
    5 x 3, P = 2 as device tensors."""
    ref, x, J, k = oracle_case(P, nex, ney)
    assert k <= 1e9
    c = device_case(P, nex, ney)
    Fs = _functionals()
    tensors = P == 2
    xin = c.to_local(x) if tensors else x
    for p in PARAMS:     # the hand-written partials and the gradients: the oracle's to the apply bar
        assert rel(c.residual_partials(x, p), ref.residual_partials(x, p)) <= 1e-12, p
    for F in Fs:
        g = F.gradient(c, xin)
        assert isinstance(g, torch.Tensor) == tensors
        assert rel(c.to_global(g) if tensors else g, F.gradient(ref, x)) <= 1e-12, F.name
        assert abs(F.value(c, xin) - F.value(ref, x)) <= 1e-12 * abs(F.value(ref, x)), F.name
        lam = c.solve_adjoint(g)
        assert isinstance(lam, torch.Tensor) == tensors
        lam = c.to_global(lam) if tensors else lam
        res = np.linalg.norm(J.T @ lam - F.gradient(ref, x))
        print(f"{F.name}: {c.adjoint_iterations} GMRES iterations, true residual {res:.3e}, "
              f"bound {1.01 * c.atol_gmres:.3e}, |lam| {np.linalg.norm(lam):.3e}")
        assert res <= 1.01 * c.atol_gmres, F.name
    mtols = (c.cd._mtol, c.ns._mtol)
    got = c.total_derivatives(xin, Fs, PARAMS)
    assert (c.cd._mtol, c.ns._mtol) == mtols
    want, scale = _reference_derivatives(ref, x, J, Fs)
    assert set(got) == set(want)
    for (name, p), r in want.items():
        bound = 1.01 * c.atol_gmres * scale[p] + 1e-12 * abs(r)
        print(f"d{name}/d{p}: {got[(name, p)]:.9e} reference {r:.9e} diff {abs(got[(name, p)] - r):.3e} "
              f"bound {bound:.3e}")
        assert abs(got[(name, p)] - r) <= bound, (name, p)
    for F in Fs:
        assert isinstance(c.adjoints[F.name], torch.Tensor) == tensors
        assert c.adjoint_norms[F.name] > 0.0


def test_finite_difference(gpu):
    """dNu_W/dRa and dKE/dRa by the adjoint against central differences FD(h), FD(h / 2), h = 20, of the coupler's
    own converged forward solves at 3 x 3, P = 2, each warm-started from the base state.

    Bound: |FD(h) - FD(h/2)| + 2 ||lam||_2 atol_nonlin / h.  The first term is three times the Richardson estimate
    of FD(h/2)'s truncation error (FD(h) - FD(h/2) = 3 e(h/2) for an h^2 error); the second bounds the noise of the
    two solves of a difference, each stopped at ||R|| <= atol_nonlin, through dF = lam^T R.  The check is vacuous
    unless the bound is below 1e-3 |FD(h/2)|, which is asserted; mtol_nonlin = 1e-11 and mtol_gmres = 1e-12 meet it.
    Measured on the MI355X: Nu_W difference 3.8e-9, terms 1.150e-8 + 9.82e-9, bar 2.08e-7;
    KE difference 1.7e-13, terms 5.145e-13 + 4.88e-14, bar 1.33e-11."""
    P, nex, ney, h = 2, 3, 3, 20.0
    kw = dict(mtol_nonlin=1e-11, mtol_gmres=1e-12)
    Fs = _functionals()
    c = _device_coupler(P, nex, ney, **kw)
    x = np.concatenate(c.solve())
    ref = AD.coupler(P, nex, ney, **BASE)
    ref.residuals(x)
    ref.linearize(x)
    J = AD.coupled_jacobian(ref.cd, ref.ns)
    k = AD.cond(J)
    print(f"cond(J) = {k:.3e}")
    assert k <= 1e9
    adj = c.total_derivatives(x, Fs, ("Ra",))
    vals = {}
    for dRa in (h, -h, h / 2, -h / 2):
        cp = _device_coupler(P, nex, ney, Ra=BASE["Ra"] + dRa, **kw)
        xp = np.concatenate(cp.solve(x))
        vals[dRa] = {F.name: F.value(cp, xp) for F in Fs}
    for F in Fs:
        fd = {s: (vals[s][F.name] - vals[-s][F.name]) / (2 * s) for s in (h, h / 2)}
        rich = abs(fd[h] - fd[h / 2])
        noise = 2.0 * c.adjoint_norms[F.name] * c.atol_nonlin / h
        tol = rich + noise
        a = adj[(F.name, "Ra")]
        print(f"d{F.name}/dRa: adjoint {a:.9e} FD(h) {fd[h]:.9e} FD(h/2) {fd[h / 2]:.9e} |adjoint - FD(h/2)| "
              f"{abs(a - fd[h / 2]):.3e}; Richardson term {rich:.3e} noise term {noise:.3e} "
              f"(|lam| {c.adjoint_norms[F.name]:.3e}) vacuity bar {1e-3 * abs(fd[h / 2]):.3e}")
        assert tol < 1e-3 * abs(fd[h / 2]), F.name
        assert abs(a - fd[h / 2]) <= tol, F.name


def test_refusals(gpu):
    from sem_amd.solvers.functionals import KineticEnergy
    ref, x, J, _ = oracle_case(4, 3, 3)
    c = _device_coupler(4, 3, 3)
    g = KineticEnergy().gradient(ref, x)
    with pytest.raises(RuntimeError, match="linearize must run before solve_adjoint"):
        c.solve_adjoint(g)
    c.residuals(x)
    with pytest.raises(RuntimeError, match="linearize must run before solve_adjoint"):
        c.solve_adjoint(g)
    c = _device_coupler(4, 3, 3, schur_precond="pcd")              # the NS solver's own refusal, no silent switch
    c.residuals(x)
    c.linearize(x)
    with pytest.raises(ValueError, match="schur_precond='mass'"):
        c.solve_adjoint(g)
    c = _device_coupler(4, 3, 3, mtol_gmres=1e-20)                 # a solvable case, out of reach of one cycle
    c.residuals(x)
    c.linearize(x)
    mtols = (c.cd._mtol, c.ns._mtol)
    with pytest.raises(RuntimeError, match="adjoint GMRES failed to converge in 1 restarts"):
        c.solve_adjoint(g, maxiter=1)
    assert (c.cd._mtol, c.ns._mtol) == mtols
    c.cd._part = object()                                          # a partitioned coupler refuses before anything else
    for call in (lambda: c.jacobian_apply_T(g), lambda: c.block_jacobi_T(g), lambda: c.solve_adjoint(g)):
        with pytest.raises(ValueError, match="whole-mesh solvers only"):
            call()
    c.cd._part = None
