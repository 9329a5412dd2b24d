"""World-size 2/3 gloo tests (CPU) of the PRECONDITIONED adjoint update of the partitioned convection-diffusion solver
(ConvectionDiffusionSolver(partition=..., partition_adjoint="condensed")): the worker setting of
tests/test_dist_adjoint_gloo.py (tests/cpu_mesh_T.CPUStripMeshT strips) on its two (4, 4, 4) cases.  _get_update_T,
right-preconditioned by StripLineSolver(adjoint=True).solve1_T, meets the forward solve's stopping rule on the true
residual in at most 3 matvecs (the whole-mesh preconditioned solve takes 2; one more for a second iteration when the
first lands just above atol), strictly fewer than the unpreconditioned partition_adjoint=True solver in the same
worker; a string other than "condensed" raises ValueError."""
import os
import queue
import time

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from test_dist_adjoint_gloo import MTOL, _free_port


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
        from sem_amd.parallel import Partition
        from sem_amd.solvers import ConvectionDiffusionSolver
        from sem_amd.solvers.strip_solve import StripLineSolver
        P, nex, ney, kind, overlap = case
        Pe = 40.0
        ref = O.CDOracle(1.0, 1.0, Pe, P, nex, ney, T_W=0.5, T_E=-0.5)
        r = np.random.default_rng(29)
        T, u, v, w, b = (r.uniform(-1, 1, ref.N) for _ in range(5))
        ref.residuals(T, u, v)
        ref.calc_jacobians(T)
        AD = sp.lil_matrix(ref.Sys)
        for p in np.flatnonzero(ref.mask):
            AD.rows[p], AD.data[p] = [int(p)], [1.0]
        AD = AD.tocsr()

        def solver(mode):
            cd = ConvectionDiffusionSolver(1.0, 1.0, Pe, P, nex, ney, T_W=0.5, T_E=-0.5, mtol=MTOL,
                                           partition=Partition(dist, exchange=kind, overlap=overlap,
                                                               mesh_factory=CPUStripMeshT), partition_adjoint=mode)
            cd._get_residuals(T, u, v)
            cd._calc_jacobians(T)
            return cd

        out = {}
        for name, mode in (("condensed", "condensed"), ("plain", True)):
            cd = solver(mode)
            lam = cd._get_update_T(b)
            out[name] = dict(res=float(np.linalg.norm(AD.T @ lam - b)), matvecs=cd.matvecs)
            if name == "condensed":
                vs = cd._jacobian_solver()
                out["solver"] = isinstance(vs, StripLineSolver) and vs.transpose
        out["bound"] = 1.01 * MTOL * np.sqrt(ref.N)
        try:
            ConvectionDiffusionSolver(1.0, 1.0, Pe, P, nex, ney, T_W=0.5, T_E=-0.5, mtol=MTOL,
                                      partition=Partition(dist, exchange=kind, overlap=overlap,
                                                          mesh_factory=CPUStripMeshT), partition_adjoint="dense")
            out["bad_string"] = False
        except ValueError as e:
            out["bad_string"] = "partition_adjoint" in str(e)
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,case", [
    (2, (4, 4, 4, "p2p", True)),
    (3, (4, 4, 4, "allreduce", True)),      # strips of 2, 1, 1 columns
])
def test_partitioned_cd_adjoint_preconditioned_gloo(world, case):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, case, q)) for r in range(world)]
    for p in procs:
        p.start()
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
    for rank, e in sorted(res.items()):
        print(rank, "matvecs: condensed", e["condensed"]["matvecs"], "unpreconditioned", e["plain"]["matvecs"],
              "residual", e["condensed"]["res"], "bound", e["bound"])
        assert e["solver"], rank
        assert e["condensed"]["res"] <= e["bound"], (rank, e)
        assert e["plain"]["res"] <= e["bound"], (rank, e)
        assert 0 < e["condensed"]["matvecs"] <= 3, (rank, e)
        assert e["condensed"]["matvecs"] < e["plain"]["matvecs"], (rank, e)
        assert e["bad_string"], rank
