"""CPU tests of the transposed nested-dissection velocity solve (NestedDissectionSolver.solve_T,
sem_amd/solvers/nested_dissection.py _build_steps_T / _run_T): the torch path over the forward factor's own tables
against SciPy's sparse solve of the transposed Dirichlet-row-replaced Jacobian (the reference factors J with `splu`,
NavierStokes_Solver.py:176-192; its transposed solve is splu's trans='T'), duality with the forward solve, the
transposed lift on the Dirichlet rows, the refinement gate's twin, the refusals and the lazy plan."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

from velocity_blocks import oracle_velocity_jacobian
from sem_amd.solvers.nested_dissection import NestedDissectionSolver, StripNDSolver, _gll_tables, element_matrices
from sem_amd.solvers.velocity_solve import VelocityJacobianSolver

# the CASES of test_nested_dissection.py (random fields) and the six cases of its test_nd_split_leaves
CASES = [(4, 3, 2, 100.0), (2, 2, 3, 400.0), (6, 2, 2, 1000.0), (3, 1, 1, 1.0), (2, 7, 2, 300.0), (3, 6, 5, 50.0),
         (4, 1, 3, 20.0), (5, 3, 7, 150.0)]
SPLIT_CASES = [(4, 3, 2, 100.0, 0.3, True), (8, 2, 3, 1000.0, 0.3, True), (10, 2, 2, 1000.0, 0.3, True),
               (12, 2, 2, 1000.0, 0.3, True), (5, 3, 7, 150.0, 0.0, False), (12, 2, 3, 200.0, 0.0, False)]
FWD_TOL, ETA_TOL = 1e-10, 1e-13


def _kw(ns, u, v, Re):
    t = torch.as_tensor
    return dict(c_stiff=1.0, c_gradx=Re, cu=t(u), c_grady=Re, cv=t(v), juu=t(Re * (ns.Gx @ u)),
                jvv=t(Re * (ns.Gy @ v)), juv=t(Re * (ns.Gy @ u)), jvu=t(Re * (ns.Gx @ v)))


@pytest.fixture(scope="module")
def factored():
    """(ns, solver, J^T as CSC) per case, factored once and shared (the tests do not change the factor)."""
    cache = {}

    def get(P, nex, ney, Re, smooth=0.0):
        key = (P, nex, ney, Re, smooth)
        if key not in cache:
            ns, u, v = oracle_velocity_jacobian(P, nex, ney, Re, seed=P * 10 + nex, smooth=smooth)
            vs = NestedDissectionSolver(P, nex, ney, "cpu")
            vs.factor_coeffs(1.0 / nex, 1.0 / ney, **_kw(ns, u, v, Re))
            cache[key] = (ns, vs, ns.Jvelo.T.tocsc())
        return cache[key]
    return get


def _check_against_scipy(vs, JT, N, solve=None):
    r = np.random.default_rng(5)
    bu, bv = r.uniform(-1, 1, N), r.uniform(-1, 1, N)
    xu, xv = (solve or vs.solve_T)(torch.as_tensor(bu), torch.as_tensor(bv))
    b = np.hstack((bu, bv))
    want = spla.spsolve(JT, b)
    got = np.hstack((xu.numpy(), xv.numpy()))
    fwd = np.abs(got - want).max() / np.abs(want).max()
    eta = np.abs(JT @ got - b).max() / (abs(JT).sum(axis=1).max() * np.abs(got).max() + np.abs(b).max())
    print(f"forward error {fwd:.3e}  backward error {eta:.3e}")
    assert fwd <= FWD_TOL
    assert eta <= ETA_TOL
    return got


@pytest.mark.parametrize("P,nex,ney,Re", CASES)
def test_solve_T_matches_sparse_lu(factored, P, nex, ney, Re):
    ns, vs, JT = factored(P, nex, ney, Re)
    _check_against_scipy(vs, JT, ns.N)


@pytest.mark.parametrize("P,nex,ney,Re,smooth,split", SPLIT_CASES)
def test_solve_T_both_leaf_kinds(factored, P, nex, ney, Re, smooth, split):
    ns, vs, JT = factored(P, nex, ney, Re, smooth)
    assert vs.split == split and (vs._leafB is not None) == split and (vs._leafF is None) == split
    _check_against_scipy(vs, JT, ns.N)
    kinds = [st[0] for st in vs._steps_T]
    assert kinds.count("leafT") == int(split) and kinds.count("sparseT") == int(not split)


@pytest.mark.parametrize("P,nex,ney,Re,smooth", [(4, 3, 2, 100.0, 0.0), (6, 2, 2, 1000.0, 0.0), (8, 2, 3, 1000.0, 0.3),
                                                 (5, 3, 7, 150.0, 0.0)])
def test_duality_with_the_forward_solve(factored, P, nex, ney, Re, smooth):
    """<J^-T c, b> = <c, J^-1 b>: each side carries its solve's 1e-10 relative error, so the two differ by at most
    1e-10 (|x_T|_inf |b|_1 + |c|_1 |x|_inf)."""
    ns, vs, _ = factored(P, nex, ney, Re, smooth)
    r = np.random.default_rng(8)
    b, c = (torch.as_tensor(r.uniform(-1, 1, 2 * ns.N)) for _ in range(2))
    x = torch.cat(vs.solve(b[:ns.N], b[ns.N:]))
    xT = torch.cat(vs.solve_T(c[:ns.N], c[ns.N:]))
    gap = abs(float(xT @ b) - float(c @ x))
    bound = 1e-10 * (float(xT.abs().max() * b.abs().sum()) + float(c.abs().sum() * x.abs().max()))
    print(f"duality gap {gap:.3e}  bound {bound:.3e}")
    assert gap <= bound


def test_dirichlet_entries(factored):
    """x_D = b_D - A_ND^T x_N: the transposed lift changes the Dirichlet entries (the forward solve keeps them)."""
    ns, vs, _ = factored(4, 3, 2, 100.0)
    r = np.random.default_rng(3)
    bu, bv = torch.as_tensor(r.uniform(-1, 1, ns.N)), torch.as_tensor(r.uniform(-1, 1, ns.N))
    D = torch.as_tensor(np.asarray(ns.mask_bound, dtype=bool))
    xu, xv = vs.solve_T(bu, bv)
    assert (xu[D] != bu[D]).any() and (xv[D] != bv[D]).any()
    yu, yv = vs.solve(bu, bv)
    assert torch.equal(yu[D], bu[D]) and torch.equal(yv[D], bv[D])


def test_singular_component_block():
    """The case of test_nd_split_refused_when_a_component_block_is_singular (juv = jvu = 1: dense leaves): J swaps
    u and v off the Dirichlet rows and has no Dirichlet columns, so J^T = J there and the solve is SciPy's."""
    P, nex, ney = 3, 3, 2
    vs = NestedDissectionSolver(P, nex, ney, "cpu")
    NY = ney * P + 1
    N = vs.NX * NY
    one = torch.ones(N, dtype=torch.float64)
    vs.factor_coeffs(1.0 / nex, 1.0 / ney, juv=one, jvu=one)
    assert not vs.split and vs._leafF is not None
    x, y = np.divmod(np.arange(N), NY)
    Dn = (x == 0) | (x == vs.NX - 1) | (y == 0) | (y == NY - 1)
    D = np.concatenate((Dn, Dn))
    import scipy.sparse as sp
    swap = sp.bmat([[None, sp.identity(N)], [sp.identity(N), None]]).tocsr()
    keep = sp.diags((~D).astype(float))
    J = (keep @ swap @ keep + sp.diags(D.astype(float))).tocsc()
    _check_against_scipy(vs, J.T.tocsc(), N)


def _scipy_apply_T(JT, vs):
    N = JT.shape[0] // 2

    def apply(X):
        x = torch.cat((X.view(vs.NX, 2, -1)[:, 0].reshape(-1), X.view(vs.NX, 2, -1)[:, 1].reshape(-1))).numpy()
        y = torch.as_tensor(JT @ x)
        return torch.stack((y[:N].view(vs.NX, -1), y[N:].view(vs.NX, -1)), 1).reshape(vs.NX, -1)
    return apply


def test_refinement_gate(factored):
    ns, vs, JT = factored(6, 2, 2, 1000.0)
    zero = torch.zeros(ns.N, dtype=torch.float64)
    try:
        with pytest.raises(RuntimeError):
            vs.check_refinement_T()                      # no transposed operator yet
        vs.set_operator(None, apply_lines_T=_scipy_apply_T(JT.tocsr(), vs))
        eta = vs.check_refinement_T()
        assert np.isfinite(eta) and eta < 1e-12 and vs.refine_T == (eta > 1e-13) and vs.refine_eta_T == eta
        assert vs.check_refinement_T(tau=0.0) == eta and vs.refine_T    # tau = 0: refine always
        _check_against_scipy(vs, JT, ns.N)
        vs.set_operator(None, apply_lines_T=lambda X: X * float("nan"))
        with pytest.raises(RuntimeError):                # a non-finite eta does not pass as "no refinement needed"
            vs.check_refinement_T()
        vs.set_operator(None)                            # refine_T forced on, the operator gone
        vs.refine_T = True
        with pytest.raises(RuntimeError):
            vs.solve_T(zero, zero)
    finally:
        vs.set_operator(None)
        vs.refine_T = False


def test_refusals():
    """No transposed condensation (line condensation) and no transposed reduced system (strips)."""
    with pytest.raises(NotImplementedError, match="condensation"):
        VelocityJacobianSolver(3, 2, 2, "cpu").solve_T(None, None)
    with pytest.raises(NotImplementedError, match="reduced system"):
        StripNDSolver.solve_T(object(), None, None)
    assert StripNDSolver.solve_T is not NestedDissectionSolver.solve_T


def test_plan_is_lazy_and_leaves_the_forward_plan_alone():
    P, nex, ney, Re = 4, 3, 2, 100.0
    ns, u, v = oracle_velocity_jacobian(P, nex, ney, Re, seed=P * 10 + nex, smooth=0.3)
    vs = NestedDissectionSolver(P, nex, ney, "cpu")
    vs.factor_coeffs(1.0 / nex, 1.0 / ney, **_kw(ns, u, v, Re))
    assert vs._steps_T is None
    steps, nbytes = vs._steps, vs.bytes_per_solve()
    ids = [id(st) for st in steps]
    b = torch.ones(ns.N, dtype=torch.float64)
    x0 = vs.solve(b, b)
    vs.solve_T(b, b)
    assert vs._steps_T is not None
    assert vs._steps is steps and [id(st) for st in vs._steps] == ids and vs.bytes_per_solve() == nbytes
    x1 = vs.solve(b, b)
    assert torch.equal(x0[0], x1[0]) and torch.equal(x0[1], x1[1])
    # the transposed plan reads the stored operators: every operand tensor of its GEMVs is a forward-plan tensor
    stored = {id(t) for t in (vs._leafV, vs._leafF, vs._lift) if t is not None}
    stored |= {id(g[0]) for g in vs._fw + vs._fv if g is not None}
    assert all(id(it[0]) in stored for st in vs._steps_T if st[0] == "gemvT" for it in st[1])
    vs.factor_coeffs(1.0 / nex, 1.0 / ney, **_kw(ns, u, v, Re))     # a new factor drops the transposed plan
    assert vs._steps_T is None


def test_transposed_launch_policy():
    """The transposed planner's per-launch choices: the column form of sem_front_gemv for short operand columns and for
    full column workgroups that fill the device, sem_front_gemv_t elsewhere; its lanes from the median column-pair
    count, its row split only below 256 workgroups."""
    S = NestedDissectionSolver
    vs = S.__new__(S)
    a = np.array
    assert vs._launch_form_T(a([46] * 16384), a([22] * 16384)) == "cols"        # the deepest forward level
    assert vs._launch_form_T(a([94] * 4096), a([46] * 4096)) == "cols"
    assert vs._launch_form_T(a([142] * 2048), a([94] * 2048)) == "t"
    assert vs._launch_form_T(a([574] * 128), a([382] * 128)) == "cols"          # 384 full column workgroups
    assert vs._launch_form_T(a([766] * 64), a([382] * 64)) == "t"               # 192
    assert vs._launch_form_T(a([190] * 256), a([768] * 256)) == "t"             # 190 of 256 threads busy
    assert vs._launch_form_T(a([3070]), a([3070])) == "t"
    vs.forms_T = "cols"
    assert vs._launch_form_T(a([3070]), a([3070])) == "cols"
    vs.forms_T = "t"
    assert vs._launch_form_T(a([46] * 16384), a([22] * 16384)) == "t"
    assert S._launch_shape_T(a([3070]), a([3070])) == (64, 16)                        # the root: 24 tiles x 16 parts
    assert S._launch_shape_T(a([96] * 16384), a([242] * 16384)) == (64, 1)            # the leaves' V_e^T
    assert S._launch_shape_T(a([22] * 8192), a([144] * 8192)) == (16, 1)
    assert S._launch_shape_T(a([8] * 128), a([56] * 128)) == (4, 1)                   # parts keep >= 64 rows
    assert S._launch_shape_T(a([1534] * 4), a([3070] * 4)) == (64, 11)                # 48 tiles -> ceil(512 / 48) parts


def one_component_case(P, nex, ney, device="cpu"):
    """A one-component convection-diffusion-like operator with the whole perimeter Dirichlet: (solver, dense J in the
    x-major numbering), J assembled from the element shares the factor itself eliminates (the shares are pinned to
    the oracle's Jacobian by test_element_shares_sum_to_the_jacobian) with identity Dirichlet rows."""
    r = np.random.default_rng(P + nex)
    vs = NestedDissectionSolver(P, nex, ney, device, ncomp=1)
    N = vs.NX * vs.NY
    kw = dict(c_stiff=1.0, c_mass=0.3, c_gradx=40.0, cu=torch.as_tensor(r.uniform(-1, 1, N), device=device),
              c_grady=40.0, cv=torch.as_tensor(r.uniform(-1, 1, N), device=device))
    vs.factor_coeffs(1.0 / nex, 1.0 / ney, **kw)
    t = vs.tree
    A = element_matrices(t, np.arange(nex * ney), 1.0 / nex, 1.0 / ney, *_gll_tables(P), device=device, **kw)
    A = A.cpu().numpy()
    J = np.zeros((N, N))
    for e in range(nex * ney):
        J[np.ix_(t.eflat[e], t.eflat[e])] += A[e]       # one component: the line-array index is the x-major node
    D = np.zeros(N, dtype=bool)
    D[t.eflat.reshape(-1)] = t.eD.reshape(-1)
    assert not J[D].any()
    J[D, D] = 1.0
    return vs, J


@pytest.mark.parametrize("P,nex,ney", [(3, 3, 2), (4, 2, 3), (2, 5, 4)])
def test_solve1_T_one_component(P, nex, ney):
    vs, J = one_component_case(P, nex, ney)
    b = np.random.default_rng(1).uniform(-1, 1, J.shape[0])
    x = vs.solve1(torch.as_tensor(b)).numpy()
    xT = vs.solve1_T(torch.as_tensor(b)).numpy()
    want, wantT = np.linalg.solve(J, b), np.linalg.solve(J.T, b)
    assert np.abs(x - want).max() <= FWD_TOL * np.abs(want).max()
    assert np.abs(xT - wantT).max() <= FWD_TOL * np.abs(wantT).max()
    eta = np.abs(J.T @ xT - b).max() / (np.abs(J.T).sum(1).max() * np.abs(xT).max() + np.abs(b).max())
    assert eta <= ETA_TOL
    with pytest.raises(ValueError):
        vs.solve_T(torch.as_tensor(b), torch.as_tensor(b))
