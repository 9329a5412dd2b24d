"""Reverse mode of the Boussinesq couplers on the CPU: jacobian_apply_T, block_jacobi_T, solve_adjoint,
residual_partials and total_derivatives of BoussinesqCoupler and ParallelBoussinesqCoupler (gloo, world 2) on the
oracle-backed doubles of tests/adjoint_doubles.py, against the coupled sparse Jacobian assembled from the oracle's
blocks (itself checked against the oracle's dresiduals to 1e-13).

Everything that solves runs at 3 x 3 elements, P = 4 (odd counts, even P: J is regular; every case prints cond(J)
and asserts it is at most 1e9, the guard of test_gpu_ns_adjoint.py).

Bounds: the applies 1e-13 per block; the adjoint solve's true residual 1.01 atol_gmres (gmres_left tests the true
residual at each restart; 1.01 is the CD adjoint test's factor); a total derivative against the sparse direct
-g^T J^-1 dR/dp within 1.01 atol_gmres ||J^-1 dR/dp||_2 + 1e-12 |reference|, because its error is r_adj^T dx/dp for
the adjoint residual r_adj."""
import functools
import os
import socket

import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch.distributed as dist
import torch.multiprocessing as mp

import adjoint_doubles as AD

P, NE = 4, 3
PARAMS = ("Ra", "Re", "Pr")
BASE = dict(Re=1e3, Ra=1e3, Pr=0.71)


def rel(a, b):
    return np.abs(np.asarray(a) - b).max() / max(np.abs(b).max(), 1e-300)


def _functionals():
    from sem_amd.solvers.functionals import KineticEnergy, WallNusselt
    return [WallNusselt("W"), KineticEnergy()]


@functools.lru_cache(maxsize=None)
def case():
    """The sequential coupler on the doubles, converged and linearised at its solution, with the assembled J."""
    c = AD.coupler(P, NE, NE, **BASE)
    x = np.concatenate(c.solve())
    x.setflags(write=False)
    c.residuals(x)
    c.linearize(x)
    J = AD.coupled_jacobian(c.cd, c.ns)
    k = AD.cond(J)
    print(f"cond(J) = {k:.3e}")
    assert k <= 1e9
    return c, x, J, k


def test_jacobian_apply_T_and_dot_identity():
    c, x, J, k = case()
    assert k <= 1e9
    rng = np.random.default_rng(5)
    w, d = rng.uniform(-1, 1, c.DOF), rng.uniform(-1, 1, c.DOF)
    got, want = c.jacobian_apply_T(w), J.T @ w
    for name, a, b in zip(("dT_bar", "du_bar", "dv_bar", "dp_bar"), c._split(got), c._split(want)):
        print(f"{name}: {rel(a, b):.3e}")
        assert rel(a, b) <= 1e-13, name
    lhs, rhs = np.dot(c.jacobian_apply(d), w), np.dot(d, got)
    print(f"dot identity: {lhs:.15e} {rhs:.15e}")
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    assert c.calls["jacobian_apply_T"] >= 1 and c.timing["jacobian_apply_T"] > 0.0
    # the block-Jacobi transpose solves each block's transposed system
    z = c.block_jacobi_T(w)
    back = np.hstack((c.cd._get_dresiduals_T(z[:c.Ncd])[0],) + tuple(c.ns._get_dresiduals_T(*c._split(z)[1:])))
    assert rel(back, w) <= 1e-9
    assert c.calls["cd_update_T"] >= 1 and c.calls["ns_update_T"] >= 1


def test_functional_values():
    """WallNusselt is 1 for pure conduction at either wall; KineticEnergy and Linear against their definitions."""
    from sem_amd.solvers.functionals import KineticEnergy, Linear, WallNusselt
    c, x, J, _ = case()
    xs = np.asarray(c.cd.points[0])
    cond_state = np.concatenate((0.5 - xs, np.zeros(3 * c.Nns)))
    for side in "WE":
        assert abs(WallNusselt(side).value(c, cond_state) - 1.0) <= 1e-12
    _, u, v, _ = c._split(x)
    M = c.ns.o.M
    assert abs(KineticEnergy().value(c, x) - 0.5 * (u @ (M @ u) + v @ (M @ v))) <= 1e-15
    coef = np.random.default_rng(3).uniform(-1, 1, c.DOF)
    lin = Linear(coef)
    assert lin.value(c, x) == float(np.dot(coef, x)) and np.array_equal(lin.gradient(c, x), coef)
    # every gradient is the derivative of its value (both are linear or quadratic: a unit step is exact), and its
    # pressure block is zero
    d = np.random.default_rng(4).uniform(-1, 1, c.DOF)
    for F in (WallNusselt("W"), WallNusselt("E"), KineticEnergy()):
        g = F.gradient(c, x)
        fd = 0.5 * (F.value(c, x + d) - F.value(c, x - d))
        assert abs(np.dot(g, d) - fd) <= 1e-12 * max(abs(fd), 1e-3), F.name
        assert not g[c.Ncd + 2 * c.Nns:].any(), F.name
        assert F.partial(c, x, "Ra") == 0.0


def test_solve_adjoint():
    c, x, J, k = case()
    assert k <= 1e9
    for F in _functionals():
        g = F.gradient(c, x)
        lam = c.solve_adjoint(g)
        res = np.linalg.norm(J.T @ lam - g)
        print(f"{F.name}: {c.adjoint_iterations} GMRES iterations, true residual {res:.3e}, "
              f"bound {1.01 * c.atol_gmres:.3e}, |lam| {np.linalg.norm(lam):.3e}")
        assert res <= 1.01 * c.atol_gmres, F.name
        # restarted from its own solution it is done at once
        again = c.solve_adjoint(g, lam0=lam)
        assert c.adjoint_iterations == 0 and np.array_equal(again, lam)


def _reference_derivatives(c, x, J, functionals):
    lu = spla.splu(J.tocsc())
    out, scale = {}, {}
    for p in PARAMS:
        dxdp = lu.solve(c.residual_partials(x, p))
        scale[p] = np.linalg.norm(dxdp)
        for F in functionals:
            out[(F.name, p)] = -float(np.dot(F.gradient(c, x), dxdp))
    return out, scale


def _check_derivatives(got, want, scale, atol_gmres):
    for (name, p), ref in want.items():
        bound = 1.01 * atol_gmres * scale[p] + 1e-12 * abs(ref)
        print(f"d{name}/d{p}: {got[(name, p)]:.9e} reference {ref:.9e} diff {abs(got[(name, p)] - ref):.3e} "
              f"bound {bound:.3e}")
        assert abs(got[(name, p)] - ref) <= bound, (name, p)


def test_total_derivatives():
    c, x, J, k = case()
    assert k <= 1e9
    Fs = _functionals()
    got = c.total_derivatives(x, Fs, PARAMS)
    want, scale = _reference_derivatives(c, x, J, Fs)
    assert set(got) == set(want)
    _check_derivatives(got, want, scale, c.atol_gmres)
    assert set(c.adjoints) == set(c.adjoint_norms) == {F.name for F in Fs}
    for F in Fs:
        assert c.adjoint_norms[F.name] == np.linalg.norm(c.adjoints[F.name])
    # the issue's oracle figure for this mesh: dNu_W/dRa = 1.931887e-4 (all printed digits)
    assert abs(got[("Nu_W", "Ra")] - 1.931887e-4) <= 5e-11


@pytest.mark.parametrize("name", PARAMS)
def test_residual_partials(name):
    """The hand-written partials against a symmetric difference of the coupler's own residuals in the parameter.
    Each residual is a + b p + c / p in each parameter p (the buoyancy coefficient is Ra / (Pr Re)), so the
    geometric symmetric difference (R(2 p) - R(p / 2)) / (3 p / 2) is exact to rounding -- for a p, for a 1 / p,
    and for a constant -- where an arithmetic unit step is exact only for the first: 1e-10 relative."""
    c, x, _, _ = case()
    got = c.residual_partials(x, name)
    R = {}
    for s in (2.0, 0.5):
        kw = dict(BASE)
        kw[name] *= s
        R[s] = AD.coupler(P, NE, NE, **kw).residuals(x)
    fd = (R[2.0] - R[0.5]) / (1.5 * BASE[name])
    err = np.abs(got - fd).max() / np.abs(fd).max()
    print(f"dR/d{name}: {err:.3e}")
    assert err <= 1e-10
    assert not got[c.Ncd + 2 * c.Nns:].any()                      # pressure rows and the pin
    assert not got[:c.Ncd][c.cd.o.mask].any()                    # Dirichlet rows
    for blk in c._split(got)[1:3]:
        assert not blk[c.ns.o.mask_bound].any()
    with pytest.raises(ValueError, match="'Ra', 'Re' or 'Pr'"):
        c.residual_partials(x, "Gr")


def test_refusals():
    from sem_amd.solvers.functionals import KineticEnergy
    c = AD.coupler(P, NE, NE, **BASE)
    g = np.ones(c.DOF)
    with pytest.raises(RuntimeError):                              # before linearize
        c.solve_adjoint(g)
    _, x, _, _ = case()
    c = AD.coupler(P, NE, NE, mtol_gmres=1e-30, **BASE)            # out of reach: maxiter runs out
    c.residuals(x)
    c.linearize(x)
    mtols = (c.cd._mtol, c.ns._mtol)
    with pytest.raises(RuntimeError, match="adjoint GMRES failed to converge in 1 restarts"):
        c.solve_adjoint(KineticEnergy().gradient(c, x), maxiter=1)
    assert (c.cd._mtol, c.ns._mtol) == mtols

    class Part:
        _part = object()

        def _whole_mesh_only(self, what):
            raise ValueError(f"{what} is implemented for whole-mesh solvers only")

    c.cd = Part()
    for call in (lambda: c.jacobian_apply_T(g), lambda: c.block_jacobi_T(g), lambda: c.solve_adjoint(g)):
        with pytest.raises(ValueError, match="whole-mesh solvers only"):
            call()


# ------------------------------------------------------------------ the parallel coupler over gloo, world 2
def _worker(rank, port, x, w, q):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    import torch as _torch
    from threadpoolctl import threadpool_limits
    threadpool_limits(1)   # ranks share the host: no BLAS / OpenMP oversubscription
    _torch.set_num_threads(1)
    try:
        import adjoint_doubles
        from sem_amd.solvers.boussinesq import ParallelBoussinesqCoupler
        c = adjoint_doubles.coupler(P, NE, NE, cls=ParallelBoussinesqCoupler, dist=dist, **BASE)
        c.residuals(x)
        c.linearize(x)
        JTw = c.jacobian_apply_T(w)
        d = c.total_derivatives(x, _functionals(), PARAMS)
        q.put((rank, JTw, d, c.calls))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_parallel_coupler_adjoint():
    c, x, J, k = case()
    assert k <= 1e9
    w = np.random.default_rng(6).uniform(-1, 1, c.DOF)
    seq = c.jacobian_apply_T(w)
    Fs = _functionals()
    want, scale = _reference_derivatives(c, x, J, Fs)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, np.array(x), w, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = dict((o[0], o[1:]) for o in (q.get(timeout=600) for _ in range(2)))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (J0, d0, calls0), (J1, d1, calls1) = out[0], out[1]
    assert np.array_equal(J0, J1)
    print(f"parallel against sequential J^T w: {rel(J0, seq):.3e}")
    assert rel(J0, seq) <= 1e-14
    assert d0 == d1
    _check_derivatives(d0, want, scale, c.atol_gmres)
    # each rank ran only its own block solves, and only its own transposed map
    assert calls0["ns_update_T"] == 0 and calls1["cd_update_T"] == 0
    assert calls0["cd_update_T"] == calls1["ns_update_T"] > 0
    assert calls0["jacobian_apply_T"] == calls1["jacobian_apply_T"] > 0
