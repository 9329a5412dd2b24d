"""World-size 2/3 gloo tests (CPU) of the DISTRIBUTED adjoint update of the partitioned Navier-Stokes solver
(NavierStokesSolver(partition=..., partition_adjoint="distributed")), against SciPy on the pinned oracle's matrices
(the block form A = [J B; C E] of tests/test_gpu_ns_adjoint._Blocks, cond(A) <= 1e9 asserted: odd element counts):

* velocity_solve_T (the transposed strip nested-dissection solve) against spsolve(Jvelo^T), 1e-9 of max|x|, in both
  I/O conventions;
* _velocity_apply_lines_T on the strips -- ONE transposed strip launch on line views and the line-layout interface
  assembly -- against Jvelo^T x, 1e-12: the launch with z_c = None is the operator the whole-mesh method applies;
* the _StripSchurT operator against the dense S^T q = E^T q - B^T J^-T C^T q, at test_schur_operator_T's 1e-10;
* _get_update_T on a consistent right-hand side b = A^T lam0: ||A^T lam - b||_2 <= 1.01 mtol sqrt(N), schur_matvecs > 0
  and rank 0's whole-mesh counterpart never built (_central_solver raises);
* the inner-product identity <lam, r> = <b, _get_update(r)> at close_dot's 1e-7;
* partition_adjoint=True on the same mesh still refuses velocity_solve_T ("whole-mesh"); an unknown string is a
  ValueError.

The HIP kernels cannot run here: each rank's strip mesh is tests/cpu_mesh_lines.CPUStripMeshLines.  The product's
partition, exchanges, strip solver and solver logic run unchanged."""
import numpy as np
import pytest
import torch.distributed as dist

from test_dist_ns_adjoint_gloo import _run, _setup

MTOL = 1e-10


def _worker(rank, world, port, case, q):
    _setup(rank, world, port)
    try:
        import scipy.sparse.linalg as spla
        import torch
        from cpu_mesh_lines import CPUStripMeshLines
        from sem_amd.parallel import Partition
        from sem_amd.solvers import NavierStokesSolver
        from sem_amd.solvers.navier_stokes import _StripSchurT
        from sem_amd.solvers.nested_dissection import StripNDSolver
        from test_gpu_ns_adjoint import _Blocks
        from velocity_blocks import oracle_velocity_jacobian
        P, nex, ney, kind = case
        Re, Gr = 100.0, 30.0
        ref, u, v = oracle_velocity_jacobian(P, nex, ney, Re, seed=P + nex, smooth=0.3)
        blk = _Blocks(ref)
        N = blk.N
        z = np.zeros(N)

        def solver(mode):
            s = NavierStokesSolver(1.0, 1.0, Re, Gr, P, nex, ney, u_N=1.0, mtol=MTOL, iprint=[],
                                   partition=Partition(dist, exchange=kind, mesh_factory=CPUStripMeshLines),
                                   partition_adjoint=mode)
            s._get_residuals(u, v, z, z)
            s._calc_jacobians(u, v)
            return s

        ns = solver("distributed")
        part, mesh = ns._part, ns._mesh

        def no_twin():
            raise AssertionError("the distributed adjoint update must not build the whole-mesh counterpart")

        ns._central_solver = no_twin
        rel = lambda a, c: float(np.abs(np.asarray(a) - c).max() / np.abs(c).max())   # noqa: E731
        r = np.random.default_rng(41)
        e = dict(cond=blk.cond, widths=[part.part.bounds[k + 1] - part.part.bounds[k] for k in range(world)])
        # velocity_solve_T
        b2 = r.uniform(-1, 1, 2 * N)
        want = spla.spsolve(blk.J.T.tocsc(), b2)
        xu, xv = ns.velocity_solve_T(b2[:N], b2[N:])
        e["solve_T"] = float(np.abs(np.hstack((xu, xv)) - want).max() / np.abs(want).max())
        e["solve_T_numpy"] = all(isinstance(a, np.ndarray) and a.shape == (N,) for a in (xu, xv))
        lu, lv = ns.velocity_solve_T(ns._dev(b2[:N]), ns._dev(b2[N:]))
        e["solve_T_local"] = all(isinstance(a, torch.Tensor) and a.numel() == mesh.n_local for a in (lu, lv))
        e["solve_T_tensor"] = max(float(np.abs(part.gather(a).numpy() - c).max()) for a, c in ((lu, xu), (lv, xv)))
        vs = ns._velo
        e["factor"] = isinstance(vs, StripNDSolver) and vs.adjoint and vs._apply_T is not None
        # _velocity_apply_lines_T: one transposed strip launch, one line-layout assembly
        x2 = r.uniform(-1, 1, 2 * N)
        NY = mesh.NY
        X = torch.stack((ns._dev(x2[:N]).view(-1, NY), ns._dev(x2[N:]).view(-1, NY)), dim=1).reshape(-1, 2 * NY)
        mesh.launches_nsT.clear()
        mesh.launches_lines.clear()
        Y = ns._velocity_apply_lines_T(X)
        e["apply_T_launches"] = (list(mesh.launches_nsT), list(mesh.launches_lines))
        got = np.hstack([part.gather(Y[:, c * NY:(c + 1) * NY].reshape(-1).contiguous()).numpy() for c in range(2)])
        e["apply_T"] = rel(got, blk.J.T @ x2)
        # the adjoint Schur operator on the strips
        qv = r.uniform(-1, 1, N)
        want = blk.E.T @ qv - blk.B.T @ spla.spsolve(blk.J.T.tocsc(), blk.C.T @ qv)
        op = _StripSchurT(ns, ns._strip_velocity_solver_T(), graph=True)
        e["schur_graph"] = op._graph is None        # gloo: the matvec stays eager
        e["schur_T"] = rel(part.gather(op(ns._dev(qv))).numpy(), want)
        # the distributed adjoint update on a consistent right-hand side
        AT = blk.A.T.tocsr()
        b = AT @ r.uniform(-1, 1, 3 * N)
        lam = ns._get_update_T(b[:N], b[N:2 * N], b[2 * N:])
        e["update_T_numpy"] = all(isinstance(a, np.ndarray) and a.shape == (N,) for a in lam)
        e["update_T_res"] = float(np.linalg.norm(AT @ np.hstack(lam) - b))
        e["matvecs_T"] = ns.schur_matvecs
        e["twin"] = ns._twin is None
        llam = ns._get_update_T(*(ns._dev(b[k * N:(k + 1) * N]) for k in range(3)))
        e["update_T_local"] = all(isinstance(a, torch.Tensor) and a.numel() == mesh.n_local for a in llam)
        e["update_T_tensor"] = float(np.linalg.norm(AT @ np.hstack([part.gather(a).numpy() for a in llam]) - b))
        # <lam, r> = <b, _get_update(r)>.  The two sides differ by <lam, r - A x> - <A^T lam - b, x>, at most
        # 1.01 mtol sqrt(N) (|lam|_2 + |x|_2) by the two stopping rules; r = A x0 is consistent like b = A^T lam0, so
        # both solutions are O(1) per entry (not amplified by cond(A) ~ 1e7) and the products O(|A|): the gap is far
        # inside close_dot's relative 1e-7
        rr = blk.A @ r.uniform(-1, 1, 3 * N)
        x = np.hstack(ns._get_update(rr[:N], rr[N:2 * N], rr[2 * N:]))
        e["dot"] = (float(np.hstack(lam) @ rr), float(b @ x))
        # partition_adjoint=True keeps the whole-mesh refusals; an unknown mode is refused at construction
        plain = solver(True)
        kept = 0
        for call in (lambda: plain.velocity_solve_T(b2[:N], b2[N:]), lambda: plain._velocity_apply_lines_T(None)):
            try:
                call()
            except ValueError as err:
                kept += "whole-mesh" in str(err)
        e["kept_refusals"] = kept
        try:
            NavierStokesSolver(1.0, 1.0, Re, Gr, P, nex, ney, iprint=[], partition_adjoint="scattered",
                               partition=Partition(dist, exchange=kind, mesh_factory=CPUStripMeshLines))
            e["unknown_mode"] = False
        except ValueError:
            e["unknown_mode"] = True
        q.put((rank, e))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,case", [
    (2, (4, 5, 3, "allreduce")),      # strips of 3 and 2 columns
    (2, (4, 5, 3, "p2p")),
    (3, (4, 5, 3, "allreduce")),      # strips of 2, 2, 1 columns
    (3, (4, 5, 3, "p2p")),
    (3, (2, 3, 3, "allreduce")),      # one column per strip
    (3, (2, 3, 3, "p2p")),
])
def test_partitioned_ns_distributed_adjoint_gloo(world, case):
    from test_gpu_ns_adjoint import close_dot
    res = _run(_worker, world, (case,), limit=600)
    P, nex, ney, _ = case
    N = (nex * P + 1) * (ney * P + 1)
    bound = 1.01 * MTOL * np.sqrt(N)
    for rank, e in sorted(res.items()):
        print(rank, e)
        assert e["cond"] <= 1e9
        assert e["solve_T"] <= 1e-9 and e["solve_T_numpy"] and e["solve_T_local"] and e["solve_T_tensor"] == 0.0
        assert e["factor"], (rank, e)
        # one transposed launch writing (yu, yv); one pack and one unpack of whole [u | v] lines
        NY = ney * P + 1
        assert e["apply_T_launches"] == ([("yu", "yv")], [("pack", 2 * NY), ("unpack", 2 * NY)] if case[3] == "allreduce"
                                         else []), (rank, e["apply_T_launches"])
        assert e["apply_T"] <= 1e-12, (rank, e["apply_T"])
        assert e["schur_graph"] and e["schur_T"] <= 1e-10, (rank, e["schur_T"])
        assert e["update_T_numpy"] and e["update_T_local"] and e["twin"], (rank, e)
        assert e["update_T_res"] <= bound and e["update_T_tensor"] <= bound, (rank, e["update_T_res"], bound)
        assert e["matvecs_T"] > 0
        assert close_dot(*e["dot"], 1e-7), (rank, e["dot"])
        assert e["kept_refusals"] == 2 and e["unknown_mode"], (rank, e)
