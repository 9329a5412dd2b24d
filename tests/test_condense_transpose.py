"""CPU tests of the transposed line condensation (VelocityJacobianSolver(transpose=True), sem_amd/solvers/
velocity_solve.py): J^T x = b from the forward factor against SciPy's sparse solve of the transposed oracle Jacobian,
the identity <solve(b), c> = <b, solve_T(c)>, every transposed interface sweep against the dense S^T solve, the
long-double references of tests/condense_reference_T.py against the torch path and against mutants, and the refusals.

The CD solver itself needs the device (its mesh and apply are HIP): _get_update_T is left to
tests/test_gpu_condense_transpose.py."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

import condense_reference as cr
import condense_reference_T as crt
from velocity_blocks import extract, oracle_cd_jacobian, oracle_velocity_jacobian
from sem_amd.solvers import velocity_solve as V
from sem_amd.solvers.velocity_solve import VelocityJacobianSolver

# (P, nex, ney, Re): P = 2, odd P, nex != ney both ways, P = 1 (no interiors)
NS_CASES = [(2, 2, 3, 400.0), (5, 3, 2, 100.0), (4, 2, 4, 250.0), (3, 6, 2, 50.0), (1, 4, 3, 10.0)]
FORMS = [("cr", "dense"), ("cr", "thomas"), ("thomas", "dense"), ("thomas", "thomas")]


def _factor(pcs, P, nex, ney, sweep, edge, ncomp=2, transpose=True):
    vs = VelocityJacobianSolver(P, nex, ney, "cpu", sweep=sweep, ncomp=ncomp, transpose=transpose)
    if edge == "thomas":
        vs.edge_dense_max, vs.edge_solve = 0, "thomas"
    else:
        vs.edge_solve = "dense"
    vs.factor(pcs.get("AII"), pcs["D"], pcs.get("aIB"), pcs.get("aBI"), pcs["E"], pcs["F"])
    assert P == 1 or vs._edge_thomas == (edge == "thomas")
    return vs


def _ns(P, nex, ney, Re):
    ns, _, _ = oracle_velocity_jacobian(P, nex, ney, Re, seed=P * 10 + nex)
    return ns, {k: torch.as_tensor(v) for k, v in extract(ns.Jvelo.toarray(), P, nex, ney).items()}


@pytest.mark.parametrize("P,nex,ney,Re", NS_CASES)
@pytest.mark.parametrize("sweep,edge", FORMS)
def test_solve_T_matches_sparse_lu_of_the_transpose(P, nex, ney, Re, sweep, edge):
    ns, pcs = _ns(P, nex, ney, Re)
    vs = _factor(pcs, P, nex, ney, sweep, edge)
    r = np.random.default_rng(5)
    bu, bv = r.uniform(-1, 1, ns.N), r.uniform(-1, 1, ns.N)
    JT = ns.Jvelo.T.tocsc()
    want = spla.spsolve(JT, np.hstack((bu, bv)))
    got = np.hstack([t.numpy() for t in vs.solve_T(torch.as_tensor(bu), torch.as_tensor(bv))])
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    res = JT @ got - np.hstack((bu, bv))
    assert np.abs(res).max() <= 1e-11 * (abs(JT).max() * np.abs(got).max())
    # <solve(b), c> = <b, solve_T(c)>
    cu, cv = r.uniform(-1, 1, ns.N), r.uniform(-1, 1, ns.N)
    x = np.hstack([t.numpy() for t in vs.solve(torch.as_tensor(bu), torch.as_tensor(bv))])
    y = np.hstack([t.numpy() for t in vs.solve_T(torch.as_tensor(cu), torch.as_tensor(cv))])
    lhs, rhs = x @ np.hstack((cu, cv)), np.hstack((bu, bv)) @ y
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs), np.linalg.norm(x) * np.linalg.norm(np.hstack((cu, cv))))
    with pytest.raises(ValueError):
        vs.solve1_T(torch.as_tensor(bu))


CD_CASES = [(4, 3, 2, 40.0), (8, 2, 3, 710.0), (1, 4, 3, 10.0), (3, 1, 1, 1.0), (2, 2, 2, 5.0), (5, 3, 5, 200.0)]


@pytest.mark.parametrize("P,nex,ney,Pe,sweep,edge", [c + f for c in CD_CASES for f in FORMS
                                                     if not (c[3] == 710.0 and f[1] == "thomas")])
def test_solve1_T_solves_the_transposed_cd_jacobian(P, nex, ney, Pe, sweep, edge):
    """ncomp = 1 on the oracle CD operator, whose Dirichlet set is the west and east sides only (not the whole
    perimeter).  The cases are tests/test_velocity_solve.py's and three more.  Its P = 8, Pe = 710 case runs on the
    dense edge inverse only, as it does there: on the block-Thomas edge factors (no pivoting across the edge blocks)
    the FORWARD solve of that factor is itself 1.9e-10 from SciPy at cond(A) = 2.7e4 (backward error 1.1e-12), and
    the transposed solve 3.1e-10 (backward error 2.5e-13): the factor's accuracy, which the refinement gate
    (check_refinement / check_refinement_T) exists for, not the transposition's."""
    cd, A, _, _ = oracle_cd_jacobian(P, nex, ney, Pe, seed=P + nex)
    assert not cd.mask.all() and cd.mask.sum() == 2 * (ney * P + 1)
    pcs = {k: torch.as_tensor(v) for k, v in extract(A.toarray(), P, nex, ney, ncomp=1).items()}
    vs = _factor(pcs, P, nex, ney, sweep, edge, ncomp=1)
    r = np.random.default_rng(7)
    b, c = r.uniform(-1, 1, cd.N), r.uniform(-1, 1, cd.N)
    got = vs.solve1_T(torch.as_tensor(b)).numpy()
    want = spla.spsolve(A.T.tocsc(), b)
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    x = vs.solve1(torch.as_tensor(c)).numpy()
    assert abs(x @ b - c @ got) <= 1e-10 * max(abs(x @ b), np.linalg.norm(x) * np.linalg.norm(b))
    with pytest.raises(ValueError):
        vs.solve_T(torch.as_tensor(b), torch.as_tensor(b))


def test_the_forward_solve_is_bitwise_the_same_with_the_flag():
    """transpose=True changes nothing the forward solve reads: same bits before and after transposed solves."""
    P, nex, ney = 4, 3, 2
    ns, pcs = _ns(P, nex, ney, 100.0)
    a = _factor(pcs, P, nex, ney, "cr", "thomas", transpose=False)
    b = _factor(pcs, P, nex, ney, "cr", "thomas", transpose=True)
    r = np.random.default_rng(1)
    bu, bv = (torch.as_tensor(r.uniform(-1, 1, ns.N)) for _ in range(2))
    want = a.solve(bu, bv)
    for _ in range(2):
        got = b.solve(bu, bv)
        assert all(torch.equal(g, w) for g, w in zip(got, want))
        b.solve_T(bu, bv)


def _tridiag(n, m, seed):
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    Sd = torch.rand((n, m, m), dtype=f64, generator=g) - 0.5 + 3 * m * torch.eye(m, dtype=f64)
    Su = torch.rand((max(n - 1, 0), m, m), dtype=f64, generator=g) - 0.5
    Sl = torch.rand((max(n - 1, 0), m, m), dtype=f64, generator=g) - 0.5
    A = torch.zeros((n * m, n * m), dtype=f64)
    for L in range(n):
        A[L * m:(L + 1) * m, L * m:(L + 1) * m] = Sd[L]
        if L < n - 1:
            A[L * m:(L + 1) * m, (L + 1) * m:(L + 2) * m] = Su[L]
            A[(L + 1) * m:(L + 2) * m, L * m:(L + 1) * m] = Sl[L]
    return Sd, Su, Sl, A, torch.rand((n, m), dtype=f64, generator=g) - 0.5


def _plain_factors(Sd, Su, Sl):
    n = Sd.shape[0]
    Dinv, Uh = torch.empty_like(Sd), torch.empty_like(Su)
    Dt = Sd[0]
    for L in range(n):
        if L > 0:
            Dt = Sd[L] - Sl[L - 1] @ Uh[L - 1]
        Dinv[L] = torch.linalg.inv(Dt)
        if L < n - 1:
            Uh[L] = Dinv[L] @ Su[L]
    return Dinv, Uh


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7])
@pytest.mark.parametrize("m", [1, 5])
def test_transposed_sweeps_match_the_dense_transposed_solve(n, m):
    """Cyclic reduction and the plain, fused and twisted (n >= 3) block-Thomas sweeps, each transposed from its own
    stored operators, against a dense solve with S^T; the right-hand side is left alone."""
    Sd, Su, Sl, A, b = _tridiag(n, m, 100 * n + m)
    keep = b.clone()
    want = torch.linalg.solve(A.T, b.reshape(-1)).reshape(n, m)
    tol = 1e-12 * want.abs().max().item()
    vs = VelocityJacobianSolver(1, max(n - 1, 1), 1, "cpu", sweep="cr", ncomp=1, transpose=True)
    vs.nex, vs.m = n - 1, m
    vs._cr_factor(Sd, Su, Sl)
    assert (vs._cr_solve_T(b) - want).abs().max().item() <= tol
    fwd = vs._cr_solve(b.clone())
    assert (fwd - torch.linalg.solve(A, b.reshape(-1)).reshape(n, m)).abs().max().item() <= tol * 10
    Dinv, Uh = _plain_factors(Sd, Su, Sl)
    assert (V.plain_thomas_solve_T(Dinv, Sl, Uh, b) - want).abs().max().item() <= tol
    th = V.fused_thomas_operators(Dinv, Sl, Uh)
    assert (V.fused_thomas_solve_T(*th, b) - want).abs().max().item() <= tol
    if n >= 3:
        tw = V.twisted_thomas_operators(Sd, Su, Sl, inv=torch.linalg.inv)
        assert (V.twisted_thomas_solve_T(tw, b) - want).abs().max().item() <= tol
    assert torch.equal(b, keep)


def test_cr_levels_in_the_forward_order_fail():
    """Mutant: the transposed cyclic reduction with its levels in the forward solve's order is not S^-T."""
    n, m = 7, 4
    Sd, Su, Sl, A, b = _tridiag(n, m, 3)
    want = torch.linalg.solve(A.T, b.reshape(-1)).reshape(n, m)
    vs = VelocityJacobianSolver(1, n - 1, 1, "cpu", sweep="cr", ncomp=1, transpose=True)
    vs.m = m
    vs._cr_factor(Sd, Su, Sl)
    assert (vs._cr_solve_T(b) - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    vs._cr.reverse()
    vs._cr_T = None
    assert (vs._cr_solve_T(b) - want).abs().max().item() > 1e-3 * want.abs().max().item()


def test_roles_of_aIB_and_aBI_not_swapped_fail():
    """Mutant: the transposed solve with aIB and aBI in their forward places misses SciPy's solve of J^T."""
    P, nex, ney = 4, 3, 2
    ns, pcs = _ns(P, nex, ney, 100.0)
    vs = _factor(pcs, P, nex, ney, "cr", "thomas")
    r = np.random.default_rng(5)
    b = np.hstack((r.uniform(-1, 1, ns.N), r.uniform(-1, 1, ns.N)))
    want = spla.spsolve(ns.Jvelo.T.tocsc(), b)
    bu, bv = torch.as_tensor(b[:ns.N]), torch.as_tensor(b[ns.N:])
    got = np.hstack([t.numpy() for t in vs.solve_T(bu, bv)])
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    vs.aIB, vs.aBI = vs.aBI.permute(0, 2, 1, 3).contiguous(), vs.aIB.permute(0, 2, 1, 3).contiguous()
    bad = np.hstack([t.numpy() for t in vs.solve_T(bu, bv)])
    assert np.abs(bad - want).max() > 1e-6 * np.abs(want).max()


def test_check_refinement_T_gates_on_the_transposed_operator():
    P, nex, ney = 4, 3, 2
    ns, pcs = _ns(P, nex, ney, 100.0)
    J, NX = ns.Jvelo, nex * P + 1

    def lines(M):
        def f(X):
            X3 = X.view(NX, 2, -1)
            y = M @ np.hstack((X3[:, 0].reshape(-1).numpy(), X3[:, 1].reshape(-1).numpy()))
            Y = torch.as_tensor(y).view(2, NX, -1)
            return torch.stack((Y[0], Y[1]), dim=1).reshape(X.shape)
        return f

    vs = _factor(pcs, P, nex, ney, "cr", "thomas")
    with pytest.raises(RuntimeError, match="apply_lines_T"):
        vs.check_refinement_T()
    vs.set_operator(lines(J), apply_lines_T=lines(J.T.tocsr()))
    assert vs.check_refinement_T() <= 1e-13 and not vs.refine_T
    assert vs.check_refinement_T(tau=0.0) <= 1e-13 and vs.refine_T     # tau = 0: always refine
    r = np.random.default_rng(3)
    b = np.hstack((r.uniform(-1, 1, ns.N), r.uniform(-1, 1, ns.N)))
    got = np.hstack([t.numpy() for t in vs.solve_T(torch.as_tensor(b[:ns.N]), torch.as_tensor(b[ns.N:]))])
    res = J.T @ got - b
    assert np.abs(res).max() <= 1e-14 * (abs(J).max() * np.abs(got).max() + 1)
    assert vs.capture_T() is False                                      # no device: the solve stays eager


def test_refusals():
    P, nex, ney = 3, 2, 2
    ns, pcs = _ns(P, nex, ney, 50.0)
    b = torch.zeros(ns.N, dtype=torch.float64)
    vs = _factor(pcs, P, nex, ney, "cr", "dense", transpose=False)            # default-constructed
    for call in (lambda: vs.solve_T(b, b), lambda: vs.solve1_T(b), lambda: vs._solve_lines_T(b),
                 lambda: vs.check_refinement_T(), lambda: vs.capture_T()):
        with pytest.raises(NotImplementedError, match="condensation"):
            call()
    for interior in ("lu", "inverse"):
        with pytest.raises(NotImplementedError, match="nested"):
            VelocityJacobianSolver(P, nex, ney, "cpu", interior=interior, transpose=True)
    with pytest.raises(RuntimeError, match="factor"):                         # unfactored
        VelocityJacobianSolver(P, nex, ney, "cpu", transpose=True).solve_T(b, b)
    from sem_amd.solvers.strip_solve import StripLineSolver
    import inspect
    assert "transpose" not in inspect.signature(StripLineSolver.__init__).parameters
    strip = StripLineSolver.__new__(StripLineSolver)
    VelocityJacobianSolver.__init__(strip, P, nex, ney, "cpu", ncomp=2)
    with pytest.raises(NotImplementedError, match="condensation"):
        strip.solve_T(b, b)


# ---- the long-double references of the transposed launches (tests/condense_reference_T.py) --------------------------

@pytest.mark.parametrize("nc,P,nex,ney", [(1, 4, 2, 3), (2, 3, 3, 2), (2, 5, 1, 1)])
def test_references_reproduce_the_torch_path(nc, P, nex, ney):
    """chain_solve_t on a real factor's blocks equals VelocityJacobianSolver._nested_solve_T, with and without the
    interface correction."""
    if nc == 2:
        ns, pcs = _ns(P, nex, ney, 100.0)
    else:
        _, A, _, _ = oracle_cd_jacobian(P, nex, ney, 40.0, seed=P + nex)
        pcs = {k: torch.as_tensor(v) for k, v in extract(A.toarray(), P, nex, ney, ncomp=1).items()}
    vs = _factor(pcs, P, nex, ney, "cr", "thomas", ncomp=nc)
    c = crt.case_from_solver(vs, seed=nc * 10 + P)
    for coupled in (False, True):
        ref = crt.chain_solve_t(c, coupled)
        R = torch.as_tensor(c.R[:, :c.nI].copy())
        if coupled:
            aBIt, xB = torch.as_tensor(c.aBIt), torch.as_tensor(c.xB)
            R = (R.view(nex, P - 1, c.m) - (aBIt[:, :, 0] * xB[:-1, None] + aBIt[:, :, 1] * xB[1:, None])).reshape(nex, -1)
        want = vs._nested_solve_T(R[..., None])[..., 0].numpy()
        got = np.asarray(ref["Y"], dtype=np.float64)
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()


def _verdicts(mutant):
    """Per launch: does a float64 evaluation of the (possibly mutated) formulas stay within SLACK x bound of the
    long-double reference."""
    out = {}
    for nc, P, nex, ney in ((1, 5, 2, 3), (2, 4, 2, 2)):
        for coupled in (False, True):
            c = crt.synthetic_t(P, nex, ney, nc, coupled)
            ref = crt.chain_solve_t(c, coupled)
            got = crt.chain_solve_t(c, coupled, dt=np.float64, mutant=mutant)
            for k in ("C", "re", "ye", "Yi"):
                out[(nc, coupled, k)] = cr.within(got[k], ref[k], ref["b" + k])
    return out


def test_float64_evaluation_passes_every_bound():
    v = _verdicts(None)
    assert all(v.values()), v


@pytest.mark.parametrize("mutant,launch", [("swap_EuEl", "ye"), ("Ed_not_transposed", "ye"), ("swap_C", "re"),
                                           ("drop_coupling", "re"), ("Xi_not_transposed", "Yi")])
def test_mutant_fails_its_bound(mutant, launch):
    assert mutant in crt.MUTANTS_T
    v = _verdicts(mutant)
    hit = [k for k, ok in v.items() if k[2] == launch and not ok and (mutant != "drop_coupling" or k[1])]
    assert hit, v


@pytest.mark.parametrize("P,nex,ney,nc", crt.solve_cases_t())
def test_every_bound_is_capped(P, nex, ney, nc):
    """SLACK x bound <= CAP at every shape the GPU tests run, ni = 1024 included: no bound is vacuous."""
    for coupled in (False, True):
        c = crt.synthetic_t(P, nex, ney, nc, coupled)
        ref = crt.chain_solve_t(c, coupled)
        for k in ("bC", "bre", "bye", "bYi"):
            assert cr.SLACK * float(np.max(ref[k])) <= cr.CAP, (k, float(np.max(ref[k])))


@pytest.mark.parametrize("m,nb,S,W", crt.GEMV_T_CASES)
def test_block_gemv_t_reference(m, nb, S, W):
    """The reference of sem_block_gemv_t: float64 within the bound, capped; an untransposed slice is not."""
    g = crt.gemv_t_case(m, nb, S, W, seed=m + nb)
    ref, bound = crt.ref_block_gemv_t(g)
    assert cr.SLACK * float(np.max(bound)) <= cr.CAP
    got, _ = crt.ref_block_gemv_t(g, dt=np.float64)
    assert cr.within(got, ref, bound)
    if m > 1:
        bad, _ = crt.ref_block_gemv_t(g, dt=np.float64, mutant="not_transposed")
        assert not cr.within(bad, ref, bound)
