"""World-size 2/3 gloo tests (CPU) of reverse mode on the partitioned Navier-Stokes solver
(NavierStokesSolver(partition=..., partition_adjoint=True)):

* _get_dresiduals_T, gathered, equals the transpose of the dense matrix of NSOracle.dresiduals at dT = 0 (built from
  identity columns), and with want_T the transpose of the oracle's dT column block, on uneven strips that include a
  one-column strip, for both exchange protocols; tolerance 1e-12 of max|ref|, as the CD twin test uses;
* the inner-product identity <_get_dresiduals(d), w> = <d, _get_dresiduals_T(w)>, shared lines counted once;
* both I/O conventions (global NumPy in, gathered NumPy out; local tensors in, local tensors out), exactly one
  transposed launch per call, one collective for all outputs;
* _get_update_T: rank 0's whole-mesh counterpart (replaced by an oracle-backed twin whose _get_update_T solves the
  dense A^T) gets the gathered linearisation and right-hand sides, the result is broadcast and satisfies
  ||A^T lam - b|| within the bound the twin itself reaches; a twin that raises makes every rank raise;
* without partition_adjoint both methods still raise the "whole-mesh" ValueError.

The HIP kernels cannot run here: each rank's strip mesh is tests/cpu_mesh_nsT.CPUStripMeshNST, whose transposed apply
is the dense transpose of its own forward strip matrix.  The product's partition, exchanges and solver logic run
unchanged."""
import os
import queue
import socket
import time

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _setup(rank, world, port):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import torch
    from threadpoolctl import threadpool_limits
    threadpool_limits(1)   # ranks share the host: no BLAS / OpenMP oversubscription
    torch.set_num_threads(1)


def _dense(ref, N):
    """(A, A_T): the 3N x 3N matrix of NSOracle.dresiduals at dT = 0 and its 3N x N dT column block."""
    A, AT = np.empty((3 * N, 3 * N)), np.empty((3 * N, N))
    Z = np.zeros(N)
    for j in range(3 * N):
        ops = [Z, Z, Z]
        e = np.zeros(N)
        e[j % N] = 1.0
        ops[j // N] = e
        A[:, j] = np.concatenate(ref.dresiduals(*ops))
    for j in range(N):
        e = np.zeros(N)
        e[j] = 1.0
        AT[:, j] = np.concatenate(ref.dresiduals(Z, Z, Z, e))
    return A, AT


def _twin_class():
    from oracle_solvers import OracleNS

    class OracleNST(OracleNS):
        """The oracle solver double with an adjoint update: the dense A^T of its own dresiduals, solved by least
        squares (on a mesh with an even element count the equal-order Jacobian is singular up to rounding)."""

        def _get_update_T(self, du_bar, dv_bar, dp_bar, dres_c0=None):
            A, _ = _dense(self.o, self.N)
            b = np.concatenate([np.asarray(a) for a in (du_bar, dv_bar, dp_bar)])
            lam = np.linalg.lstsq(A.T, b, rcond=None)[0]
            self.reached = float(np.linalg.norm(A.T @ lam - b))
            self.schur_matvecs = 0
            return tuple(np.split(lam, 3))

    return OracleNST


def _worker(rank, world, port, case, q):
    _setup(rank, world, port)
    try:
        import torch
        from cpu_mesh_nsT import CPUStripMeshNST
        from oracle import sem_oracle as O
        from sem_amd.parallel import Partition
        from sem_amd.solvers import NavierStokesSolver
        P, nex, ney, kind = case
        Re, Gr = 60.0, 25.0
        part = Partition(dist, exchange=kind, mesh_factory=CPUStripMeshNST)
        mk = lambda p, **kw: NavierStokesSolver(1.0, 1.0, Re, Gr, P, nex, ney, u_N=1.0, mtol=1e-11, iprint=[],  # noqa: E731
                                                partition=p, **kw)
        ns = mk(part, partition_adjoint=True)
        twin = _twin_class()(1.0, 1.0, Re, Gr, P, nex, ney)
        ns._central_solver = lambda: twin
        ref = O.NSOracle(1.0, 1.0, Re, Gr, P, nex, ney, u_N=1.0)
        N = ns.N
        r = np.random.default_rng(31)
        u, v, p, T = (r.uniform(-1, 1, N) for _ in range(4))
        w = [r.uniform(-1, 1, N) for _ in range(3)]
        d = [r.uniform(-1, 1, N) for _ in range(3)]
        ns._get_residuals(u, v, p, T)
        ns._calc_jacobians(u, v)
        ref.residuals(u, v, p, T)
        ref.calc_jacobians(u, v)
        A, AT = _dense(ref, N)
        wz = np.concatenate(w)
        want = np.split(A.T @ wz, 3) + [AT.T @ wz]
        rel = lambda a, c: float(np.abs(np.asarray(a) - c).max() / np.abs(c).max())   # noqa: E731
        mesh = ns._mesh
        errs = {"widths": [part.part.bounds[k + 1] - part.part.bounds[k] for k in range(world)]}
        # global NumPy in, gathered NumPy out
        mesh.launches_nsT.clear()
        outs = ns._get_dresiduals_T(*w)
        errs["launches"] = list(mesh.launches_nsT)
        errs["dres_T"] = max(rel(g, c) for g, c in zip(outs, want))
        errs["dres_T_numpy"] = len(outs) == 3 and all(isinstance(g, np.ndarray) and g.shape == (N,) for g in outs)
        mesh.launches_nsT.clear()
        outs = ns._get_dresiduals_T(*w, want_T=True)
        errs["launches_T"] = list(mesh.launches_nsT)
        errs["dres_T_wantT"] = max(rel(g, c) for g, c in zip(outs, want))
        errs["wantT_len"] = len(outs)
        # local tensors in, local tensors out
        louts = ns._get_dresiduals_T(*(ns._dev(a) for a in w), want_T=True)
        errs["dres_T_local"] = all(isinstance(g, torch.Tensor) and g.numel() == mesh.n_local for g in louts)
        errs["dres_T_tensor"] = max(rel(part.gather(g).numpy(), c) for g, c in zip(louts, want))
        # the inner-product identity on gathered vectors (a shared line counted once)
        fwd = ns._get_dresiduals(*d)
        lhs = sum(float(a @ b) for a, b in zip(fwd, w))
        adj = ns._get_dresiduals_T(*w)
        rhs = sum(float(a @ b) for a, b in zip(d, adj))
        # the two applies are right to 1e-13 max|fwd| (test_dist_ns_gloo) and 1e-12 max|adj| (above) per entry, so
        # the two inner products differ by at most that times the 1-norm of the other factor
        bound = (1e-13 * max(np.abs(a).max() for a in fwd) * sum(np.abs(a).sum() for a in w)
                 + 1e-12 * max(np.abs(a).max() for a in adj) * sum(np.abs(a).sum() for a in d))
        errs["dot"] = abs(lhs - rhs) / bound
        # the central adjoint update: consistent right-hand side b = A^T lam0
        b = np.split(A.T @ np.concatenate([r.uniform(-1, 1, N) for _ in range(3)]), 3)
        lam = ns._get_update_T(*b)
        errs["update_T_numpy"] = all(isinstance(g, np.ndarray) and g.shape == (N,) for g in lam)
        errs["update_T_res"] = float(np.linalg.norm(A.T @ np.concatenate(lam) - np.concatenate(b)))
        errs["twin_reached"] = getattr(twin, "reached", None) if rank == 0 else None
        errs["twin_unused"] = rank == 0 or not hasattr(twin, "reached")
        errs["b_norm"] = float(np.linalg.norm(np.concatenate(b)))
        llam = ns._get_update_T(*(ns._dev(a) for a in b))
        errs["update_T_local"] = all(isinstance(g, torch.Tensor) and g.numel() == mesh.n_local for g in llam)
        errs["update_T_tensor"] = max(float(np.abs(part.gather(g).numpy() - c).max()) for g, c in zip(llam, lam))
        # without the opt-in a partitioned solver refuses both methods
        plain = mk(Partition(dist, exchange=kind, mesh_factory=CPUStripMeshNST))
        plain._get_residuals(u, v, p, T)
        plain._calc_jacobians(u, v)
        raised = 0
        for call in (lambda: plain._get_dresiduals_T(*w), lambda: plain._get_update_T(*b)):
            try:
                call()
            except ValueError as e:
                raised += "whole-mesh" in str(e)
        errs["refused"] = raised
        # the solves that stay whole-mesh only refuse with the option too
        kept = 0
        for call in (lambda: ns.velocity_solve_T(w[0], w[1]), lambda: ns._velocity_apply_lines_T(None)):
            try:
                call()
            except ValueError as e:
                kept += "whole-mesh" in str(e)
        errs["kept_refusals"] = kept
        q.put((rank, errs))
    finally:
        dist.destroy_process_group()


def _run(target, world, args, limit=300):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + args + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    res, t0 = {}, time.time()
    while len(res) < world:     # fail fast when a rank dies instead of waiting out the queue
        try:
            k, v = q.get(timeout=2)
            res[k] = v
        except queue.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            assert not dead and time.time() - t0 < limit, f"rank failed or hung (exit codes {dead})"
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("world,case", [
    (2, (3, 3, 3, "allreduce")),      # strips of 2 and 1 columns
    (2, (3, 3, 3, "p2p")),
    (3, (2, 4, 3, "allreduce")),      # strips of 2, 1, 1 columns; the pin lies on the first interface line
    (3, (2, 4, 3, "p2p")),
])
def test_partitioned_ns_adjoint_gloo(world, case):
    res = _run(_worker, world, (case,))
    for rank, e in sorted(res.items()):
        print(rank, e)
        assert 1 in e["widths"] and len(set(e["widths"])) > 1, e["widths"]
        assert e["dres_T"] <= 1e-12 and e["dres_T_wantT"] <= 1e-12 and e["dres_T_tensor"] <= 1e-12, (rank, e)
        assert e["dres_T_numpy"] and e["dres_T_local"] and e["wantT_len"] == 4, (rank, e)
        assert e["launches"] == [("yu", "yv", "yp")] and e["launches_T"] == [("yu", "yv", "yp", "yT")], (rank, e)
        assert e["dot"] <= 1.0, (rank, e)
        assert e["update_T_numpy"] and e["update_T_local"] and e["update_T_tensor"] == 0.0, (rank, e)
        assert e["twin_unused"], (rank, e)
        assert e["update_T_res"] <= res[0]["twin_reached"], (rank, e)
        assert res[0]["twin_reached"] <= 1e-9 * e["b_norm"], (rank, e)     # the twin did solve the system
        assert e["refused"] == 2 and e["kept_refusals"] == 2, (rank, e)


def _fail_worker(rank, world, port, q):
    """Rank 0's whole-mesh adjoint update raises; every rank must raise, none may stay blocked in the broadcast."""
    _setup(rank, world, port)
    try:
        from cpu_mesh_nsT import CPUStripMeshNST
        from sem_amd.parallel import Partition
        from sem_amd.solvers import NavierStokesSolver
        P, nex, ney = 2, 3, 2
        s = NavierStokesSolver(1.0, 1.0, 100.0, 0.0, P, nex, ney, u_N=1.0, iprint=[],
                               partition=Partition(dist, mesh_factory=CPUStripMeshNST), partition_adjoint=True)
        twin = _twin_class()(1.0, 1.0, 100.0, 0.0, P, nex, ney)
        z = np.zeros(s.N)
        s._get_residuals(z, z, z, z)
        s._calc_jacobians(z, z)

        def boom(*a, **k):
            raise RuntimeError("adjoint GMRES: Failed to converge in 1 iterations")

        twin._get_update_T = boom
        s._central_solver = lambda: twin
        try:
            s._get_update_T(z, z, z)
            q.put((rank, "no error"))
        except RuntimeError as e:
            q.put((rank, str(e)))
    finally:
        dist.destroy_process_group()


def _stale_worker(rank, world, port, q):
    """A forward and an adjoint central update on one linearisation, then an adjoint update on the next: how often
    the whole-mesh counterpart is handed the linearisation."""
    _setup(rank, world, port)
    try:
        from cpu_mesh_nsT import CPUStripMeshNST
        from sem_amd.parallel import Partition
        from sem_amd.solvers import NavierStokesSolver
        P, nex, ney = 4, 3, 3
        calls = {"residuals": 0, "jacobians": 0}

        class Counting(_twin_class()):
            def _get_residuals(self, *a):
                calls["residuals"] += 1
                return super()._get_residuals(*a)

            def _calc_jacobians(self, *a):
                calls["jacobians"] += 1
                return super()._calc_jacobians(*a)

        ns = NavierStokesSolver(1.0, 1.0, 60.0, 0.0, P, nex, ney, u_N=1.0, mtol=1e-9, iprint=[],
                                partition=Partition(dist, mesh_factory=CPUStripMeshNST), partition_update="central",
                                partition_adjoint=True)
        twin = Counting(1.0, 1.0, 60.0, 0.0, P, nex, ney, mtol=1e-9)
        ns._central_solver = lambda: twin
        r = np.random.default_rng(5)
        u, v, p, T = (0.1 * r.uniform(-1, 1, ns.N) for _ in range(4))
        b = [r.uniform(-1, 1, ns.N) for _ in range(3)]
        ns._get_residuals(u, v, p, T)
        ns._calc_jacobians(u, v)
        ns._get_update(*b)
        ns._get_update_T(*b)
        first = dict(calls)
        ns._calc_jacobians(v, u)
        ns._get_update_T(*b)
        q.put((rank, (first, dict(calls))))
    finally:
        dist.destroy_process_group()


def test_forward_and_adjoint_central_updates_share_one_refresh():
    """_get_update then _get_update_T on one linearisation hand it to rank 0's counterpart once (one staleness record
    for both); the next _calc_jacobians makes it stale again.  The other rank never touches its counterpart."""
    res = _run(_stale_worker, 2, ())
    assert res[0] == ({"residuals": 1, "jacobians": 1}, {"residuals": 2, "jacobians": 2})
    assert res[1] == ({"residuals": 0, "jacobians": 0}, {"residuals": 0, "jacobians": 0})


def test_rank0_adjoint_update_failure_reaches_every_rank():
    res = _run(_fail_worker, 2, (), limit=120)
    assert "Failed to converge" in res[0]
    assert "failed on rank 0" in res[1]
