"""The transposed element-partitioned line solve on real strip handles (StripLineSolver(adjoint=True) over gloo, the
ranks sharing the GPU, the collectives through the host -- the setting of
tests/test_gpu_dist.py::test_strip_velocity_solve_real_kernels): sem_condensed_blocks writes each strip's pieces,
sem_nested_solve_t, sem_gemv_rows_t / sem_gemv_rows2_t and the all-reduce of the transposed reduced system carry
solve_T.  Against SciPy's sparse solve of the whole transposed Jacobian at that test's tolerance; shared lines bitwise
equal; the backward error of the assembled solution no worse than 4x the forward solve's on the same factor (the
yardstick is existing code; the factor covers the transposed sweeps' different summation order), floor 1e-13.
And the partitioned convection-diffusion adjoint update preconditioned by it (partition_adjoint="condensed")."""
import os
import queue
import socket
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(worker, world, *args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    res, t0 = {}, time.time()
    while len(res) < world:     # fail fast when a rank dies instead of waiting out the queue
        try:
            k, v = q.get(timeout=2)
            res[k] = v
        except queue.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            assert not dead and time.time() - t0 < 240, f"rank failed (exit codes {dead})"
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return [res[r] for r in range(world)]


def _init(rank, world, port, env=None):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), **(env or {}))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(max(1, 16 // world))   # ranks share the box's CPU share: no OpenMP oversubscription


def _worker_strip_T(rank, world, port, q, case, env):
    _init(rank, world, port, env)
    try:
        from velocity_blocks import oracle_velocity_jacobian
        import scipy.sparse.linalg as spla
        from sem_amd import _lib
        from sem_amd.device import get_mesh
        from sem_amd.parallel import StripPartition
        from sem_amd.solvers.strip_solve import StripLineSolver
        P, nex, ney, Re = case
        ref, u, v = oracle_velocity_jacobian(P, nex, ney, Re, seed=P * 10 + nex)
        part = StripPartition(nex, world)
        eb, ee = part.local_range(rank)
        mesh = get_mesh(P, nex, ney, 1.0 / nex, 1.0 / ney, eb, ee, 0)
        sl = slice(mesh.dof_begin, mesh.dof_begin + mesh.n_local)
        d = lambda a: mesh.to_device(np.asarray(a)[sl])  # noqa: E731
        kw = dict(c_stiff=1.0, c_gradx=Re, cu=d(u), c_grady=Re, cv=d(v), juu=d(Re * (ref.Gx @ u)),
                  jvv=d(Re * (ref.Gy @ v)), juv=d(Re * (ref.Gy @ u)), jvu=d(Re * (ref.Gx @ v)),
                  dir_sides=_lib.SIDE_W | _lib.SIDE_E | _lib.SIDE_S | _lib.SIDE_N)
        vs = StripLineSolver(P, nex, ney, mesh.device, part.bounds, rank, dist, gather_device="cpu", adjoint=True)
        vs.factor_mesh(mesh, budget_bytes=1, **kw)     # one column per chunk
        assert not vs.capture_T()                      # the collective goes through the host: declined
        r = np.random.default_rng(3)
        bu, bv = r.uniform(-1, 1, ref.N), r.uniform(-1, 1, ref.N)
        want = spla.spsolve(ref.Jvelo.T.tocsc(), np.hstack((bu, bv)))
        dbu, dbv = d(bu), d(bv)
        xu, xv = vs.solve_T(dbu, dbv)
        assert torch.equal(dbu, d(bu)) and torch.equal(dbv, d(bv))
        fu, fv = vs.solve(dbu, dbv)
        err = max(np.abs(xu.cpu().numpy() - want[:ref.N][sl]).max(), np.abs(xv.cpu().numpy() - want[ref.N:][sl]).max())
        form = vs._T[0][0] if vs._T is not None else None
        q.put((rank, (err / np.abs(want).max(), sl.start, xu.cpu().numpy(), xv.cpu().numpy(), fu.cpu().numpy(),
                      fv.cpu().numpy(), form)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,case,env,form", [
    (2, (4, 4, 3, 300.0), None, "single"),               # one interior line per strip: both boundary products on it
    (3, (6, 7, 2, 1000.0), None, "single"),              # strips of 3, 2, 2 columns
    (2, (3, 9, 2, 300.0), None, "twisted"),              # strips of 5 and 4 columns: the two-ended sweep
    (2, (3, 9, 2, 300.0), {"SEM_SWEEP_FORM": "single"}, "single"),
])
def test_strip_line_solve_T_real_kernels(gpu, world, case, env, form):
    out = _run(_worker_strip_T, world, case, env)
    from velocity_blocks import oracle_velocity_jacobian
    P, nex, ney, Re = case
    ref, _, _ = oracle_velocity_jacobian(P, nex, ney, Re, seed=P * 10 + nex)
    NY = ney * P + 1
    for rank, (err, *_, f) in enumerate(out):
        assert err <= 1e-9, (rank, err)
        assert f == form, (rank, f)
    r = np.random.default_rng(3)
    b = np.hstack((r.uniform(-1, 1, ref.N), r.uniform(-1, 1, ref.N)))
    eta = {}
    for name, J, iu, iv in (("transposed", ref.Jvelo.T.tocsr(), 2, 3), ("forward", ref.Jvelo.tocsr(), 4, 5)):
        xu, xv = np.zeros(ref.N), np.zeros(ref.N)
        for rank, o in enumerate(out):
            start, lu, lv = o[1], o[iu], o[iv]
            if rank and name == "transposed":     # the shared line: bitwise equal on both ranks (one reduced buffer)
                assert np.array_equal(xu[start:start + NY], lu[:NY]) and np.array_equal(xv[start:start + NY], lv[:NY])
            xu[start:start + lu.size], xv[start:start + lv.size] = lu, lv
        x = np.hstack((xu, xv))
        eta[name] = np.abs(J @ x - b).max() / (abs(J).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())
    print(f"strip solve over {world} ranks, {case}, {form}: backward error transposed {eta['transposed']:.1e}, "
          f"forward {eta['forward']:.1e}")
    assert eta["transposed"] <= max(1e-13, 4 * eta["forward"]), eta


MTOL = 1e-10


def _worker_cd(rank, world, port, q):
    _init(rank, world, port)
    try:
        import scipy.sparse as sp
        from oracle import sem_oracle as O
        from sem_amd.parallel import Partition
        from sem_amd.solvers import ConvectionDiffusionSolver
        P, ne, Pe = 4, 4, 40.0
        cd = ConvectionDiffusionSolver(1.0, 1.0, Pe, P, ne, ne, T_W=0.5, T_E=-0.5, mtol=MTOL, partition=Partition(dist),
                                       partition_adjoint="condensed")
        ref = O.CDOracle(1.0, 1.0, Pe, P, ne, ne, T_W=0.5, T_E=-0.5)
        r = np.random.default_rng(29)
        T, u, v, w, b = (r.uniform(-1, 1, cd.N) for _ in range(5))
        cd._get_residuals(T, u, v)
        cd._calc_jacobians(T)
        ref.residuals(T, u, v)
        AD = sp.lil_matrix(ref.Sys)
        for p in np.flatnonzero(ref.mask):
            AD.rows[p], AD.data[p] = [int(p)], [1.0]
        lam = cd._get_update_T(b)
        q.put((rank, (float(np.linalg.norm(AD.tocsr().T @ lam - b)), 1.01 * MTOL * np.sqrt(cd.N), cd.matvecs)))
    finally:
        dist.destroy_process_group()


def test_partitioned_cd_adjoint_preconditioned(gpu):
    for rank, (res, bound, matvecs) in enumerate(_run(_worker_cd, 2)):
        print(rank, "residual", res, "bound", bound, "matvecs", matvecs)
        assert res <= bound and 0 < matvecs <= 3, (rank, res, bound, matvecs)
