"""GPU tests of the transposed line condensation (VelocityJacobianSolver(transpose=True): sem_nested_solve_t,
sem_interface_rhs with the permuted couplings, the transposed cyclic reduction on sem_block_gemv_t) on device factors,
and of the adjoint convection-diffusion solve it preconditions.  The checks are those of _solve_T_checks in
tests/test_gpu_nd_transpose.py: J^T x = b against SciPy's sparse solve of the transposed oracle matrix (forward error
1e-10), backward error 1e-13 after check_refinement_T (the project's refinement gate), the HIP path against the torch
path of the same factor (1e-10), eager solves bitwise repeatable, graph replay bitwise equal to the eager solve, the
forward solve's bits untouched.  The kernels are tested one launch at a time in
test_gpu_condense_transpose_launches.py."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

from oracle import sem_oracle as O
from velocity_blocks import oracle_cd_jacobian, oracle_velocity_jacobian

pytestmark = pytest.mark.gpu


def _eta(JT, x, b):
    return float(np.abs(JT @ x - b).max() / (abs(JT).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))


def _to_lines(z, NX, nc):
    """x-major component vectors [c0 | c1] -> the (NX, nc NY) line array."""
    return np.ascontiguousarray(z.reshape(nc, NX, -1).transpose(1, 0, 2)).reshape(NX, -1)


def _from_lines(X, NX, nc):
    return np.ascontiguousarray(X.reshape(NX, nc, -1).transpose(1, 0, 2)).reshape(-1)


def _host_apply(M, NX, nc, dev):
    """X -> M X on line arrays through the oracle's assembled matrix (the tests' operator of check_refinement_T)."""
    def f(X):
        y = M @ _from_lines(X.cpu().numpy(), NX, nc)
        return torch.as_tensor(_to_lines(y, NX, nc), device=dev)
    return f


def _checks(vs, J, dev):
    nc, NX, N = vs.ncomp, vs.NX, J.shape[0] // vs.ncomp
    JT = J.T.tocsc()
    r = np.random.default_rng(5)
    b, c = r.uniform(-1, 1, nc * N), r.uniform(-1, 1, nc * N)
    B = torch.as_tensor(_to_lines(b, NX, nc), device=dev)

    def solve_T(z):
        t = [torch.as_tensor(p, device=dev) for p in z.reshape(nc, N)]
        out = vs.solve_T(*t) if nc == 2 else (vs.solve1_T(t[0]),)
        return np.hstack([o.cpu().numpy() for o in out])

    def solve(z):
        t = [torch.as_tensor(p, device=dev) for p in z.reshape(nc, N)]
        out = vs.solve(*t) if nc == 2 else (vs.solve1(t[0]),)
        return np.hstack([o.cpu().numpy() for o in out])

    assert vs._edge_thomas and vs.sweep == "cr" and vs._graph_T is None
    x_fwd0 = solve(c)                                   # the forward solve before any transposed call
    got = solve_T(b)
    want = spla.spsolve(JT, b)
    fwd = np.abs(got - want).max() / np.abs(want).max()
    print(f"forward error {fwd:.3e}  backward error {_eta(JT, got, b):.3e}")
    assert fwd <= 1e-10
    assert np.array_equal(solve(c), x_fwd0)
    # <solve(c), b> = <c, solve_T(b)>
    lhs, rhs = x_fwd0 @ b, c @ got
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), np.linalg.norm(x_fwd0) * np.linalg.norm(b))
    # the HIP path against the torch path of the same device factor; two eager solves
    x_hip = vs._solve_lines_once_T(B.clone())
    assert torch.equal(vs._solve_lines_once_T(B.clone()), x_hip)
    vs.hip_nested = False
    x_t = vs._solve_lines_once_T(B.clone())
    vs.hip_nested = True
    assert (x_hip - x_t).abs().max() <= 1e-10 * x_t.abs().max()
    # the refinement gate, then the backward error of the gated solve
    vs.set_operator(_host_apply(J.tocsr(), NX, nc, dev), apply_lines_T=_host_apply(J.T.tocsr(), NX, nc, dev))
    eta_probe = vs.check_refinement_T()
    got = solve_T(b)
    eta = _eta(JT, got, b)
    print(f"probe eta {eta_probe:.3e} refine_T {vs.refine_T}  backward error {eta:.3e}")
    assert eta <= 1e-13
    # graph replay = eager, bit for bit; the forward solve as it was
    x_eager = vs._solve_lines_T(B.clone())
    assert vs.capture_T()
    assert vs._graph_T is not None
    g1, g2 = solve_T(b), solve_T(b)
    assert np.array_equal(g1, _from_lines(x_eager.cpu().numpy(), NX, nc)) and np.array_equal(g1, g2)
    assert np.array_equal(solve(c), x_fwd0)


@pytest.mark.parametrize("P,nex,ney,Pe", [(4, 4, 4, 40.0), (5, 3, 5, 100.0), (2, 2, 2, 5.0)])
def test_cd_factor_solves_the_transpose(P, nex, ney, Pe):
    """One component: the CD solver's own factor (west and east Dirichlet sides only)."""
    from sem_amd.solvers import ConvectionDiffusionSolver
    _, A, u, v = oracle_cd_jacobian(P, nex, ney, Pe, seed=P + nex)
    cd = ConvectionDiffusionSolver(1.0, 1.0, Pe, P, nex, ney, T_W=0.5, T_E=-0.5)
    cd._get_residuals(np.zeros(cd.N), u, v)
    vs = cd._jacobian_solver()
    assert vs.transpose and vs.ncomp == 1
    _checks(vs, A, cd._mesh.device)


def _ns_partial(P, nex, ney, Re, seed):
    """A two-component line-condensation factor on the device with Dirichlet rows on the west, east and south sides
    only, and the oracle's velocity Jacobian with the same rows replaced."""
    from sem_amd import _lib
    from sem_amd.solvers import NavierStokesSolver
    from sem_amd.solvers.convection_diffusion import geometric_mask
    from sem_amd.solvers.velocity_solve import VelocityJacobianSolver
    ref, u, v = oracle_velocity_jacobian(P, nex, ney, Re, seed=seed, smooth=0.3)
    ns = NavierStokesSolver(1.0, 1.0, Re, 0.0, P, nex, ney, u_N=1.0, iprint=[], velocity_interior="nested")
    ns._get_residuals(u, v, np.zeros(ns.N), np.zeros(ns.N))
    ns._calc_jacobians(u, v)
    sides = _lib.SIDE_W | _lib.SIDE_E | _lib.SIDE_S
    mask1 = geometric_mask(nex * P + 1, ney * P + 1, sides)
    assert 0 < mask1.sum() < ref.mask_bound.sum()
    mask = np.hstack((mask1, mask1))
    J = sp.bmat([[ref.Juu, ref.Juv], [ref.Jvu, ref.Jvv]], format="lil")
    J[mask, :] = 0
    J[mask, mask] = 1
    dev = ns._mesh.device
    vs = VelocityJacobianSolver(P, nex, ney, dev, transpose=True)
    vs.factor_mesh(ns._mesh, juu=ns._Jac_u_u._coeffs()[4], juv=ns._Jac_u_v._coeffs()[4], jvu=ns._Jac_v_u._coeffs()[4],
                   jvv=ns._Jac_v_v._coeffs()[4], dir_mask=None, dir_sides=sides, **ns._sys_kw(ns._Sys))
    return vs, J.tocsr(), dev


@pytest.mark.parametrize("P,nex,ney,Re", [(4, 3, 2, 100.0), (7, 2, 3, 100.0)])
def test_ns_factor_with_a_partial_dirichlet_set(P, nex, ney, Re):
    vs, J, dev = _ns_partial(P, nex, ney, Re, seed=P + nex)
    _checks(vs, J, dev)


def test_torch_fallback_on_a_dense_edge_factor():
    """A device factor forced to the dense edge inverse has no transposed HIP nested solve: the torch path runs on
    the device and solves J^T x = b."""
    from sem_amd.solvers.velocity_solve import VelocityJacobianSolver
    P, nex, ney = 4, 3, 2
    orig = VelocityJacobianSolver.__init__

    def dense_init(self, *a, **k):
        orig(self, *a, **k)
        self.edge_solve = "dense"

    VelocityJacobianSolver.__init__ = dense_init
    try:
        vs, J, dev = _ns_partial(P, nex, ney, 100.0, seed=3)
    finally:
        VelocityJacobianSolver.__init__ = orig
    assert not vs._edge_thomas and vs._Se_inv is not None
    N = J.shape[0] // 2
    r = np.random.default_rng(8)
    b = r.uniform(-1, 1, 2 * N)
    xu, xv = vs.solve_T(torch.as_tensor(b[:N], device=dev), torch.as_tensor(b[N:], device=dev))
    assert xu.device == dev
    got = np.hstack((xu.cpu().numpy(), xv.cpu().numpy()))
    want = spla.spsolve(J.T.tocsc(), b)
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    assert vs.capture_T()
    gu, gv = vs.solve_T(torch.as_tensor(b[:N], device=dev), torch.as_tensor(b[N:], device=dev))
    assert np.abs(np.hstack((gu.cpu().numpy(), gv.cpu().numpy())) - want).max() <= 1e-10 * np.abs(want).max()


def test_device_refusals():
    from sem_amd.solvers.velocity_solve import VelocityJacobianSolver
    dev = torch.device("cuda", 0)
    for interior in ("lu", "inverse"):
        with pytest.raises(NotImplementedError, match="nested"):
            VelocityJacobianSolver(4, 2, 2, dev, interior=interior, transpose=True)
    z = torch.zeros(81, dtype=torch.float64, device=dev)
    with pytest.raises(NotImplementedError, match="condensation"):
        VelocityJacobianSolver(4, 2, 2, dev, ncomp=1).solve1_T(z)
    with pytest.raises(RuntimeError, match="factor"):
        VelocityJacobianSolver(4, 2, 2, dev, ncomp=1, transpose=True).solve1_T(z)


# ---- the adjoint convection-diffusion solve ------------------------------------------------------------------------------

MTOL = 1e-10


def _cd(precond):
    from sem_amd.solvers import ConvectionDiffusionSolver
    s = ConvectionDiffusionSolver(1, 1, 40, 4, 4, 4, T_W=0.5, T_E=-0.5, mtol=MTOL, precond=precond)
    rng = np.random.default_rng(21)
    T, u, v = (rng.uniform(-1, 1, s.N) for _ in range(3))
    s._get_residuals(T, u, v)
    s._calc_jacobians(T)
    return s, T, u, v


def test_get_update_T_is_preconditioned_by_the_transposed_factor():
    """The 4 x 4, P = 4 solver of tests/test_gpu_adjoint_solver.py: the adjoint solve converges on the true residual,
    satisfies the dot-product identity against _get_update, takes no more than the forward solve's matvecs + 2 on the
    same right-hand side (the forward path is the reference for the count; the margin is for the different residual
    history) and strictly fewer than the unpreconditioned solve of a second solver."""
    s, T, u, v = _cd("condensed")
    o = O.CDOracle(1, 1, 40, 4, 4, 4, T_W=0.5, T_E=-0.5)
    o.residuals(T, u, v)
    L = sp.lil_matrix(o.Sys)
    for p in np.flatnonzero(o.mask):
        L.rows[p], L.data[p] = [int(p)], [1.0]
    AD = L.tocsr()
    rng = np.random.default_rng(23)
    b, r = rng.uniform(-1, 1, s.N), rng.uniform(-1, 1, s.N)
    lam = s._get_update_T(b)
    mv_T = s.matvecs
    vs = s._jacobian_solver()
    assert vs.transpose and vs._graph_T is not None            # the transposed graph was captured on first use
    res = np.linalg.norm(AD.T @ lam - b)
    s._get_update(b)
    f = s.matvecs
    print(f"adjoint GMRES: {mv_T} matvecs (forward: {f}), residual {res:.3e}, bound {1.01 * MTOL * np.sqrt(s.N):.3e}")
    assert res <= 1.01 * MTOL * np.sqrt(s.N)
    assert 0 < mv_T <= f + 2
    lhs, rhs = np.dot(lam, r), np.dot(b, s._get_update(r))
    assert abs(lhs - rhs) <= 1e-7 * max(abs(lhs), abs(rhs))
    s2, *_ = _cd(None)
    lam2 = s2._get_update_T(b)
    print(f"unpreconditioned adjoint GMRES: {s2.matvecs} matvecs")
    assert mv_T < s2.matvecs
    assert np.linalg.norm(AD.T @ lam2 - b) <= 1.01 * MTOL * np.sqrt(s.N)
    assert s2._factor is None                                    # precond=None: no factor is built
