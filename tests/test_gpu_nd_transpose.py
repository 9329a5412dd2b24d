"""GPU tests of the transposed nested-dissection velocity solve (NestedDissectionSolver.solve_T; HIP steps
sem_front_gemv_t / sem_leaf_transpose / sem_leaf_sparse_t / sem_front_scatter, sem_amd/csrc/front_transpose.hip):
J^T x = b of the oracle's Dirichlet-row-replaced velocity Jacobian (NavierStokes_Solver.py:176-192) against SciPy's
sparse solve of the transposed matrix, agreement with the torch path of the same device factor, bitwise graph replay
and repeatability, the forward solve left bit for bit as it was, every form and shape of the transposed planner,
and the Navier-Stokes solver's transposed velocity apply and solve.  The kernels themselves are tested one launch
at a time in test_gpu_front_transpose_kernels.py."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

from velocity_blocks import oracle_velocity_jacobian

pytestmark = pytest.mark.gpu

# the CASES of test_gpu_nd.py (random fields: dense leaves mostly) and the split-leaf list of its
# test_nd_split_leaf_kernel (smooth fields, every register tile)
CASES = [(4, 3, 2, 100.0), (2, 2, 3, 400.0), (6, 2, 2, 1000.0), (3, 1, 1, 1.0), (2, 7, 2, 300.0), (3, 6, 5, 50.0),
         (8, 5, 4, 1000.0), (12, 4, 6, 200.0), (16, 2, 3, 300.0)]
SPLIT_CASES = [(2, 3, 2, 300.0), (3, 2, 3, 100.0), (4, 3, 2, 100.0), (8, 3, 4, 1000.0), (10, 2, 3, 500.0),
               (12, 4, 3, 1000.0)]


def _kw(ns, u, v, Re, dev):
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)  # noqa: E731
    return dict(c_stiff=1.0, c_gradx=Re, cu=t(u), c_grady=Re, cv=t(v), juu=t(Re * (ns.Gx @ u)),
                jvv=t(Re * (ns.Gy @ v)), juv=t(Re * (ns.Gy @ u)), jvu=t(Re * (ns.Gx @ v)))


def _factor(P, nex, ney, Re, seed, smooth=0.0):
    from sem_amd.solvers.nested_dissection import NestedDissectionSolver
    dev = torch.device("cuda", 0)
    ns, u, v = oracle_velocity_jacobian(P, nex, ney, Re, seed=seed, smooth=smooth)
    vs = NestedDissectionSolver(P, nex, ney, dev)
    vs.factor_coeffs(1.0 / nex, 1.0 / ney, **_kw(ns, u, v, Re, dev))
    return ns, vs, dev


def _lines(vs, bu, bv, dev):
    tu, tv = (torch.as_tensor(b, device=dev).view(vs.NX, -1) for b in (bu, bv))
    return torch.stack((tu, tv), 1).reshape(vs.NX, -1)


def _torch_path(vs, B):
    """The torch loop over the same device factor and tables (the CPU tests' path)."""
    Wz = torch.cat((B.reshape(-1), B.new_zeros(1)))
    vs._run_T(Wz)
    return Wz[:-1].view(vs.NX, vs.m)


def _solve_T_checks(ns, vs, dev):
    """solve_T against SciPy (forward error 1e-10, backward error 1e-13), against the torch path (1e-10: another
    summation order in every product, carried through the dependent levels -- test_nd_split_leaf_kernel's bar), two
    eager solves bitwise equal, graph replay bitwise equal to the eager solve."""
    r = np.random.default_rng(5)
    bu, bv = r.uniform(-1, 1, ns.N), r.uniform(-1, 1, ns.N)
    tu, tv = torch.as_tensor(bu, device=dev), torch.as_tensor(bv, device=dev)
    xu, xv = vs.solve_T(tu, tv)
    JT = ns.Jvelo.T.tocsc()
    b = np.hstack((bu, bv))
    want = spla.spsolve(JT, b)
    got = np.hstack((xu.cpu().numpy(), xv.cpu().numpy()))
    fwd = np.abs(got - want).max() / np.abs(want).max()
    eta = np.abs(JT @ got - b).max() / (abs(JT).sum(axis=1).max() * np.abs(got).max() + np.abs(b).max())
    print(f"forward error {fwd:.3e}  backward error {eta:.3e}")
    assert fwd <= 1e-10
    assert eta <= 1e-13
    B = _lines(vs, bu, bv, dev)
    x_hip = vs._solve_lines_once_T(B.clone())
    x_t = _torch_path(vs, B.clone())
    assert (x_hip - x_t).abs().max() <= 1e-10 * x_t.abs().max()
    assert torch.equal(vs._solve_lines_once_T(B.clone()), x_hip)
    assert vs.capture_T()
    gu, gv = vs.solve_T(tu, tv)
    assert torch.equal(gu, x_hip.view(vs.NX, 2, -1)[:, 0].reshape(-1))
    assert torch.equal(gv, x_hip.view(vs.NX, 2, -1)[:, 1].reshape(-1))
    gu2, gv2 = vs.solve_T(tu, tv)
    assert torch.equal(gu2, gu) and torch.equal(gv2, gv)


@pytest.mark.parametrize("P,nex,ney,Re", CASES)
def test_solve_T_matches_sparse_lu(P, nex, ney, Re):
    ns, vs, dev = _factor(P, nex, ney, Re, seed=P * 10 + nex)
    _solve_T_checks(ns, vs, dev)


@pytest.mark.parametrize("P,nex,ney,Re", SPLIT_CASES)
def test_solve_T_split_leaves(P, nex, ney, Re):
    ns, vs, dev = _factor(P, nex, ney, Re, seed=P + nex, smooth=0.3)
    assert vs.split, vs.split_eta
    _solve_T_checks(ns, vs, dev)
    assert sum(k == "leafT" for k, *_ in vs._hip_T) == 1


def test_forward_solve_untouched():
    """solve(b) before any transposed call, after solve_T, and after capture_T() plus a replay: bitwise equal, eager
    and replayed; operator bytes and the forward plan as they were."""
    ns, vs, dev = _factor(6, 4, 3, 400.0, seed=9, smooth=0.3)
    r = np.random.default_rng(1)
    bu, bv = (torch.as_tensor(r.uniform(-1, 1, ns.N), device=dev) for _ in range(2))
    steps, hip, nbytes = vs._steps, vs._hip, vs.bytes_per_solve()
    x0 = vs.solve(bu, bv)
    vs.solve_T(bu, bv)
    x1 = vs.solve(bu, bv)
    assert vs.capture_T()
    vs.solve_T(bu, bv)
    x2 = vs.solve(bu, bv)
    assert vs.capture()
    x3 = vs.solve(bu, bv)           # the forward graph
    vs.solve_T(bu, bv)              # the transposed graph
    x4 = vs.solve(bu, bv)
    for x in (x1, x2, x3, x4):
        assert torch.equal(x[0], x0[0]) and torch.equal(x[1], x0[1])
    assert vs._steps is steps and vs._hip is hip and vs.bytes_per_solve() == nbytes


# (mesh, smooth, the (form, lanes, split?) launches it is here for)
PLAN_CASES = [((2, 40, 40, 100.0), 0.0, {("t", 4, False), ("t", 16, False), ("t", 32, False), ("t", 64, False),
                                          ("t", 32, True), ("t", 64, True), ("cols", 1, False)}),
              ((8, 12, 12, 100.0), 0.3, {("t", 8, False), ("t", 16, False), ("t", 32, False), ("t", 64, False),
                                         ("t", 32, True), ("t", 64, True), ("cols", 1, False)})]


def _planned(vs):
    from sem_amd import _lib
    out = set()
    for kind, d, *_ in vs._hip_T:
        if kind == "gemvT":
            if isinstance(d, _lib.SemFrontTLaunch):
                out.add(("t", d.lanes, d.nparts > 1))
            else:
                out.add(("cols", 1, False))
    return out


@pytest.mark.parametrize("case,smooth,shapes", PLAN_CASES, ids=["P2-40x40", "P8-12x12"])
def test_transposed_plan_coverage(case, smooth, shapes):
    """Two mid-size meshes (the ones of test_nd_solve_wide_tiles) whose transposed plans hold every lane count of
    sem_front_gemv_t, with and without the row split; the same solve with the new form switched off (the column form
    of sem_front_gemv on the untransposed storage everywhere) agrees to 1e-11 (another summation order carried
    through the levels: test_nd_gemv_forms_agree's bar).  If the planner's rule changes and a shape below leaves
    the plans, pick meshes that bring it back."""
    P, nex, ney, Re = case
    ns, vs, dev = _factor(P, nex, ney, Re, seed=P * 10 + nex, smooth=smooth)
    _solve_T_checks(ns, vs, dev)
    planned = _planned(vs)
    assert shapes <= planned, (sorted(shapes - planned), sorted(planned))
    B = torch.rand((vs.NX, vs.m), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    x_auto = vs._solve_lines_once_T(B.clone())
    vs.forms_T = "cols"
    vs._graph_T = None              # the captured graph holds the automatic plan's tables
    vs._hip_T = vs._hip_plan_T()
    assert _planned(vs) == {("cols", 1, False)}
    x_cols = vs._solve_lines_once_T(B.clone())
    assert torch.equal(vs._solve_lines_once_T(B.clone()), x_cols)
    assert (x_auto - x_cols).abs().max() <= 1e-11 * x_cols.abs().max()


def test_all_lane_counts_are_planned():
    """Between them the plan-coverage meshes hold every lane count the library dispatches."""
    lanes = {s[1] for _, _, shapes in PLAN_CASES for s in shapes if s[0] == "t"}
    assert lanes == {4, 8, 16, 32, 64}
    assert {s[2] for _, _, shapes in PLAN_CASES for s in shapes} == {True, False}
    assert {s[0] for _, _, shapes in PLAN_CASES for s in shapes} == {"t", "cols"}


# ---- the Navier-Stokes solver ----------------------------------------------------------------------------------------

def _ns_solver(P, nex, ney, Re, seed, interior="auto", smooth=0.3):
    """(oracle, device solver) linearised at the same seeded smooth state (the oracle of test_gpu_ns_velocity.py)."""
    from sem_amd.solvers import NavierStokesSolver
    ref, u, v = oracle_velocity_jacobian(P, nex, ney, Re, seed=seed, smooth=smooth)
    s = NavierStokesSolver(1.0, 1.0, Re, 0.0, P, nex, ney, u_N=1.0, iprint=[], velocity_interior=interior)
    s._get_residuals(u, v, np.zeros(s.N), np.zeros(s.N))
    s._calc_jacobians(u, v)
    return ref, s


@pytest.mark.parametrize("P,nex,ney", [(4, 3, 2), (8, 3, 3)])
def test_ns_velocity_apply_and_solve_T(P, nex, ney):
    ref, s = _ns_solver(P, nex, ney, 100.0, seed=P + nex)
    JT = ref.Jvelo.T.tocsr()
    N, NY = s.N, s._mesh.NY
    r = np.random.default_rng(3)
    z = r.uniform(-1, 1, 2 * N)
    X = _lines_np(z, N, NY)
    Y = s._velocity_apply_lines_T(torch.as_tensor(X, device=s._mesh.device))
    y = _unlines(Y.cpu().numpy(), NY)
    y_ref = JT @ z
    assert np.abs(y - y_ref).max() <= 1e-13 * np.abs(y_ref).max()
    bu, bv = r.uniform(-1, 1, N), r.uniform(-1, 1, N)
    xu, xv = s.velocity_solve_T(bu, bv)
    assert isinstance(xu, np.ndarray)
    b = np.hstack((bu, bv))
    want = spla.spsolve(JT.tocsc(), b)
    got = np.hstack((xu, xv))
    eta = np.abs(JT @ got - b).max() / (abs(JT).sum(axis=1).max() * np.abs(got).max() + np.abs(b).max())
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    assert eta <= 1e-13
    vs = s._velocity_solver()
    assert vs._graph_T is not None and vs.refine_eta_T is not None and vs.refine_eta_T < 1e-12
    dev = s._mesh.device
    tu, tv = s.velocity_solve_T(torch.as_tensor(bu, device=dev), torch.as_tensor(bv, device=dev))
    assert isinstance(tu, torch.Tensor) and tu.device == dev
    assert np.array_equal(tu.cpu().numpy(), xu) and np.array_equal(tv.cpu().numpy(), xv)


def _lines_np(z, N, NY):
    return np.stack((z[:N].reshape(-1, NY), z[N:].reshape(-1, NY)), 1).reshape(-1, 2 * NY)


def _unlines(Y, NY):
    Y3 = Y.reshape(-1, 2, NY)
    return np.concatenate((Y3[:, 0].reshape(-1), Y3[:, 1].reshape(-1)))


def test_ns_velocity_solve_T_refusals():
    _, s = _ns_solver(4, 3, 2, 100.0, seed=1, interior="nested")     # the line condensation: no transposed solve
    z = np.zeros(s.N)
    with pytest.raises(ValueError, match="nested-dissection"):
        s.velocity_solve_T(z, z)
    s._part = object()                                        # a partitioned solver refuses before anything else
    with pytest.raises(ValueError, match="whole-mesh"):
        s.velocity_solve_T(z, z)
    with pytest.raises(ValueError, match="whole-mesh"):
        s._velocity_apply_lines_T(None)
