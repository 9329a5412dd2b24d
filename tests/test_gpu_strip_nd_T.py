"""The transposed element-partitioned nested-dissection solve on real strip handles (StripNDSolver(adjoint=True) over
gloo, the ranks sharing the GPU, the collectives through the host -- the setting of tests/test_gpu_strip_solve_T.py):
the front / leaf kernels of csrc/front_transpose.hip run each strip's two halves of the transposed steps, sem_gemv_rows_t
and the all-reduce carry the transposed reduced system.  Against SciPy's sparse solve of the whole transposed Jacobian
at 1e-9; shared lines bitwise equal; capture_T() declined while the collectives go through the host; the backward error
of the assembled solution no worse than 4x the forward solve's on the same factor (the rule of
test_strip_line_solve_T_real_kernels: the yardstick is existing code), floor 1e-13.  (12, 3, 3) is the split-leaf limit
n = (P - 1)^2 = 121 on a smooth state.
And the partitioned Navier-Stokes solver's distributed adjoint update (partition_adjoint="distributed") on real
kernels: the residual of A^T lam = b within 1.01 mtol sqrt(N); its Schur matvec count is printed beside the whole-mesh
solver's on the same linearisation (recorded, not asserted equal: the all-reduced inner products round differently)."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from test_gpu_strip_solve_T import _init, _run

pytestmark = pytest.mark.gpu


def _worker_strip_nd_T(rank, world, port, q, case, smooth):
    _init(rank, world, port)
    try:
        from velocity_blocks import oracle_velocity_jacobian
        import scipy.sparse.linalg as spla
        from sem_amd import _lib
        from sem_amd.device import get_mesh
        from sem_amd.parallel import StripPartition
        from sem_amd.solvers.nested_dissection import StripNDSolver
        P, nex, ney, Re = case
        ref, u, v = oracle_velocity_jacobian(P, nex, ney, Re, seed=P * 10 + nex, smooth=smooth)
        part = StripPartition(nex, world)
        eb, ee = part.local_range(rank)
        mesh = get_mesh(P, nex, ney, 1.0 / nex, 1.0 / ney, eb, ee, 0)
        sl = slice(mesh.dof_begin, mesh.dof_begin + mesh.n_local)
        d = lambda a: mesh.to_device(np.asarray(a)[sl])  # noqa: E731
        kw = dict(c_stiff=1.0, c_gradx=Re, cu=d(u), c_grady=Re, cv=d(v), juu=d(Re * (ref.Gx @ u)),
                  jvv=d(Re * (ref.Gy @ v)), juv=d(Re * (ref.Gy @ u)), jvu=d(Re * (ref.Gx @ v)),
                  dir_sides=_lib.SIDE_W | _lib.SIDE_E | _lib.SIDE_S | _lib.SIDE_N)
        vs = StripNDSolver(P, nex, ney, mesh.device, part.bounds, rank, dist, gather_device="cpu", adjoint=True)
        vs.factor_mesh(mesh, **kw)
        assert not vs.capture_T()                      # the collectives go through the host: declined
        r = np.random.default_rng(3)
        bu, bv = r.uniform(-1, 1, ref.N), r.uniform(-1, 1, ref.N)
        want = spla.spsolve(ref.Jvelo.T.tocsc(), np.hstack((bu, bv)))
        dbu, dbv = d(bu), d(bv)
        xu, xv = vs.solve_T(dbu, dbv)
        assert torch.equal(dbu, d(bu)) and torch.equal(dbv, d(bv))
        fu, fv = vs.solve(dbu, dbv)
        torch.cuda.synchronize()
        err = max(np.abs(xu.cpu().numpy() - want[:ref.N][sl]).max(), np.abs(xv.cpu().numpy() - want[ref.N:][sl]).max())
        q.put((rank, (err / np.abs(want).max(), sl.start, xu.cpu().numpy(), xv.cpu().numpy(), fu.cpu().numpy(),
                      fv.cpu().numpy(), bool(vs.split))))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,case,smooth", [
    (2, (4, 4, 3, 300.0), 0.0),
    (3, (6, 7, 2, 1000.0), 0.0),               # strips of 3, 2, 2 columns
    (2, (3, 2, 4, 100.0), 0.0),                # one column per strip
    (2, (12, 3, 3, 100.0), 0.3),               # the split-leaf limit n = 121 (smooth state: the split leaves)
])
def test_strip_nd_solve_T_real_kernels(gpu, world, case, smooth):
    out = _run(_worker_strip_nd_T, world, case, smooth)
    from velocity_blocks import oracle_velocity_jacobian
    P, nex, ney, Re = case
    ref, _, _ = oracle_velocity_jacobian(P, nex, ney, Re, seed=P * 10 + nex, smooth=smooth)
    NY = ney * P + 1
    for rank, (err, *_, split) in enumerate(out):
        print(f"rank {rank}: forward error {err:.3e}, split leaves {split}")
        assert err <= 1e-9, (rank, err)
        assert split or P < 12, "the n = 121 case must run the split leaves"
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
    print(f"strip ND solve over {world} ranks, {case}: backward error transposed {eta['transposed']:.1e}, "
          f"forward {eta['forward']:.1e}")
    assert eta["transposed"] <= max(1e-13, 4 * eta["forward"]), eta


MTOL = 1e-10


def _worker_ns(rank, world, port, q):
    _init(rank, world, port)
    try:
        from sem_amd.parallel import Partition
        from sem_amd.solvers import NavierStokesSolver
        from test_gpu_ns_adjoint import _Blocks
        from velocity_blocks import oracle_velocity_jacobian
        P, nex, ney, Re = 4, 5, 3, 100.0
        ref, u, v = oracle_velocity_jacobian(P, nex, ney, Re, seed=P + nex, smooth=0.3)
        blk = _Blocks(ref)
        N = blk.N
        z = np.zeros(N)

        def linearised(**kw):
            s = NavierStokesSolver(1.0, 1.0, Re, 30.0, P, nex, ney, u_N=1.0, mtol=MTOL, iprint=[], **kw)
            s._get_residuals(u, v, z, z)
            s._calc_jacobians(u, v)
            return s

        ns = linearised(partition=Partition(dist), partition_adjoint="distributed")

        def no_twin():
            raise AssertionError("the distributed adjoint update must not build the whole-mesh counterpart")

        ns._central_solver = no_twin
        AT = blk.A.T.tocsr()
        b = AT @ np.random.default_rng(43).uniform(-1, 1, 3 * N)
        lam = ns._get_update_T(b[:N], b[N:2 * N], b[2 * N:])
        res = float(np.linalg.norm(AT @ np.hstack(lam) - b))
        whole = None
        if rank == 0:      # the whole-mesh solver on the same linearisation and right-hand side, for the record
            w = linearised()
            w._get_update_T(b[:N], b[N:2 * N], b[2 * N:])
            whole = w.schur_matvecs
        torch.cuda.synchronize()
        dist.barrier()     # rank 1 leaves the group only after rank 0's extra solve
        q.put((rank, (res, 1.01 * MTOL * np.sqrt(N), ns.schur_matvecs, whole, float(blk.cond))))
    finally:
        dist.destroy_process_group()


def test_partitioned_ns_distributed_adjoint_real_kernels(gpu):
    out = _run(_worker_ns, 2)
    for rank, (res, bound, matvecs, whole, cond) in enumerate(out):
        print(f"rank {rank}: residual {res:.3e} bound {bound:.3e} Schur matvecs {matvecs} (whole mesh: {whole}) "
              f"cond(A) {cond:.2e}")
        assert cond <= 1e9
        assert res <= bound and matvecs > 0, (rank, res, bound, matvecs)
