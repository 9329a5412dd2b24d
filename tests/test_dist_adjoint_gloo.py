"""World-size 2/3 gloo tests (CPU) of reverse mode on the partitioned convection-diffusion solver
(ConvectionDiffusionSolver(partition=..., partition_adjoint=True), sem_amd.parallel.StripApplyT):

* the transposed strip apply with the interface exchange, gathered, equals the oracle's A_D^T w, for both
  exchange protocols, with and without overlap, on uneven strips that include a one-column strip;
* _get_dresiduals_T (global NumPy in, gathered NumPy out; local tensors in, local tensors out) equals the
  whole-mesh oracle's transposes;
* _get_update_T (the unpreconditioned distributed GMRES) meets the stopping rule of the forward solve at
  4 x 4, P = 4;
* without partition_adjoint both methods still raise.

The HIP kernels cannot run here: each rank's strip mesh is tests/cpu_mesh_T.CPUStripMeshT, whose transposed
apply is the dense transpose of its own forward strip matrix.  The product's partition, launch schedule,
exchanges, distributed inner products and solver logic run unchanged."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

MTOL = 1e-10


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, case, q):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import torch as _torch
    from threadpoolctl import threadpool_limits
    threadpool_limits(1)   # ranks share the host: no BLAS / OpenMP oversubscription
    _torch.set_num_threads(1)
    try:
        import scipy.sparse as sp
        from cpu_mesh_T import CPUStripMeshT
        from oracle import sem_oracle as O
        from sem_amd.parallel import Partition, StripApplyT
        from sem_amd.solvers import ConvectionDiffusionSolver
        P, nex, ney, kind, overlap = case
        Pe = 40.0
        part = Partition(dist, exchange=kind, overlap=overlap, mesh_factory=CPUStripMeshT)
        cd = ConvectionDiffusionSolver(1.0, 1.0, Pe, P, nex, ney, T_W=0.5, T_E=-0.5, mtol=MTOL, partition=part,
                                       partition_adjoint=True)
        ref = O.CDOracle(1.0, 1.0, Pe, P, nex, ney, T_W=0.5, T_E=-0.5)
        r = np.random.default_rng(29)
        T, u, v, w, b = (r.uniform(-1, 1, cd.N) for _ in range(5))
        cd._get_residuals(T, u, v)
        cd._calc_jacobians(T)
        ref.residuals(T, u, v)
        ref.calc_jacobians(T)
        AD = sp.lil_matrix(ref.Sys)
        for p in np.flatnonzero(ref.mask):
            AD.rows[p], AD.data[p] = [int(p)], [1.0]
        AD = AD.tocsr()
        rel = lambda a, c: np.abs(np.asarray(a) - c).max() / np.abs(c).max()   # noqa: E731
        errs = {"widths": [part.part.bounds[k + 1] - part.part.bounds[k] for k in range(world)]}
        # the transposed strip step itself
        assert isinstance(part.step_T, StripApplyT)
        mesh = cd._mesh
        mesh.launches_T.clear()
        y = cd._apply_T(cd._dev(w))
        errs["launches_T"] = list(mesh.launches_T)
        errs["step_T"] = rel(part.gather(y).numpy(), AD.T @ w)
        # _get_dresiduals_T: NumPy in, gathered NumPy out
        free = ~ref.mask
        refs = (AD.T @ w, ref.JTu.diagonal() * free * w, ref.JTv.diagonal() * free * w)
        outs = cd._get_dresiduals_T(w)
        errs["dres_T"] = max(rel(g, c) for g, c in zip(outs, refs))
        errs["dres_T_numpy"] = all(isinstance(g, np.ndarray) and g.shape == (cd.N,) for g in outs)
        # local tensors in, local tensors out
        louts = cd._get_dresiduals_T(cd._dev(w))
        errs["dres_T_local"] = all(isinstance(g, _torch.Tensor) and g.numel() == mesh.n_local for g in louts)
        errs["dres_T_tensor"] = max(rel(part.gather(g).numpy(), c) for g, c in zip(louts, refs))
        if (P, nex, ney) == (4, 4, 4):
            lam = cd._get_update_T(b)
            errs["update_T"] = float(np.linalg.norm(AD.T @ lam - b))
            errs["bound"] = 1.01 * MTOL * np.sqrt(cd.N)
            errs["matvecs"] = cd.matvecs
        # without the opt-in a partitioned solver refuses both methods
        plain = ConvectionDiffusionSolver(1.0, 1.0, Pe, P, nex, ney, T_W=0.5, T_E=-0.5, mtol=MTOL,
                                          partition=Partition(dist, exchange=kind, overlap=overlap,
                                                              mesh_factory=CPUStripMeshT))
        plain._get_residuals(T, u, v)
        plain._calc_jacobians(T)
        raised = 0
        for call in (lambda: plain._get_dresiduals_T(w), lambda: plain._get_update_T(b)):
            try:
                call()
            except ValueError as e:
                raised += "whole-mesh" in str(e)
        errs["refused"] = raised
        q.put((rank, errs))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,case", [
    (2, (4, 3, 3, "allreduce", True)),      # strips of 2 and 1 columns
    (2, (3, 3, 2, "p2p", False)),
    (2, (4, 4, 4, "p2p", True)),            # the adjoint solve
    (3, (4, 4, 4, "allreduce", True)),      # strips of 2, 1, 1 columns; the adjoint solve
    (3, (2, 5, 3, "p2p", True)),            # strips of 2, 2, 1
    (3, (3, 4, 2, "allreduce", False)),
])
def test_partitioned_cd_adjoint_gloo(world, case):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, case, q)) for r in range(world)]
    for p in procs:
        p.start()
    import queue
    import time
    res, t0 = {}, time.time()
    while len(res) < world:     # fail fast when a rank dies instead of waiting out the queue
        try:
            k, v = q.get(timeout=2)
            res[k] = v
        except queue.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            assert not dead and time.time() - t0 < 300, f"rank failed (exit codes {dead})"
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    P, nex, ney, kind, overlap = case
    for rank, e in sorted(res.items()):
        print(rank, e)
        n = e["widths"][rank]
        if (P, nex, ney) != (4, 4, 4) or world == 3:
            assert 1 in e["widths"] and len(set(e["widths"])) > 1, e["widths"]
        assert e["step_T"] <= 1e-13, (rank, e)
        assert e["dres_T"] <= 1e-12 and e["dres_T_tensor"] <= 1e-12, (rank, e)
        assert e["dres_T_numpy"] and e["dres_T_local"], (rank, e)
        want = [(0, 1), (n, n + 1)] + ([(1, n)] if n > 1 else []) if overlap else [None]
        assert e["launches_T"] == want, (rank, e)
        if (P, nex, ney) == (4, 4, 4):
            assert e["matvecs"] > 0 and e["update_T"] <= e["bound"], (rank, e)
        assert e["refused"] == 2, (rank, e)
