"""The device-collective branch of the distributed Navier-Stokes adjoint, on one GPU (the pattern of
tests/test_gpu_rccl_strip_T.py): ONE spawned process holds a real one-rank RCCL group and takes the G = 2 branches as
rank r of 2 through tests/rank_view.RankView.  A partitioned NavierStokesSolver(partition_adjoint="distributed") builds
its StripNDSolver(adjoint=True); its capture_T() must agree and a replay equal the eager _solve_lines_T to 1e-12; the
adjoint Schur operator _StripSchurT must capture its whole matvec -- the transposed launches, the line-layout interface
assembly (sem_interface_pack_lines / unpack_lines around an RCCL all-reduce), the transposed strip solve with its two
collectives, the plain assembly -- in one hipGraph whose replay equals the eager matvec to 1e-12; an eager transposed
solve issues two all-reduces and no all-gather.  Only rank-independent properties are checkable under the view (a
one-rank sum is the local tensor); the gloo tests carry correctness across ranks."""
import os
import socket
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

NS_CASE = dict(P=4, nex=5, ney=3, Re=100.0, Gr=30.0)


def sc_strip_nd_T_view(dist, dev):
    from rank_view import RankView
    from sem_amd.parallel import Partition
    from sem_amd.solvers import NavierStokesSolver
    from sem_amd.solvers.navier_stokes import _StripSchurT
    from sem_amd.solvers.nested_dissection import StripNDSolver
    c = NS_CASE
    out = {}
    for r in (0, 1):
        view = RankView(dist, 2, r)
        ns = NavierStokesSolver(1.0, 1.0, c["Re"], c["Gr"], c["P"], c["nex"], c["ney"], u_N=1.0, mtol=1e-10, iprint=[],
                                partition=Partition(view), partition_adjoint="distributed")
        rng = np.random.default_rng(41)
        u, v, p, T = (0.3 * rng.uniform(-1, 1, ns.N) for _ in range(4))
        ns._get_residuals(u, v, p, T)
        ns._calc_jacobians(u, v)
        vs = ns._strip_velocity_solver_T()      # registers the operator, gates, attempts capture_T
        vs.refine = vs.refine_T = False         # the stand-in reduced blocks make the refinement probes meaningless
        cap = vs.capture_T()
        n1 = dict(view.calls)
        B = torch.rand((vs.NX, vs.m), dtype=torch.float64, device=dev)
        keep = B.clone()
        want = vs._solve_lines_T(B)
        n2 = dict(view.calls)
        err = None
        if cap:
            vs._bin_T.copy_(B)
            vs._graph_T.replay()
            err = float((vs._xout_T - want).abs().max() / want.abs().max())
        sch = _StripSchurT(ns, vs, graph=True)
        q = torch.rand(ns._mesh.n_local, dtype=torch.float64, device=dev)
        qk = q.clone()
        eager = sch._body(q)
        sch_err = float((sch(q) - eager).abs().max() / eager.abs().max()) if sch._graph is not None else None
        torch.cuda.synchronize(dev)
        count = lambda a, b, k: b.get(k, 0) - a.get(k, 0)   # noqa: E731
        out[f"r{r}"] = dict(kind=isinstance(vs, StripNDSolver) and vs.adjoint and vs.G == 2,
                            gather_device=str(vs.gather_device), captured=bool(cap), replay_vs_eager=err,
                            b_kept=bool(torch.equal(B, keep)), finite=bool(want.isfinite().all()),
                            solve_reduces=count(n1, n2, "all_reduce"), solve_gathers=count(n1, n2, "all_gather"),
                            schur_graph=sch._graph is not None, schur_graph_vs_eager=sch_err,
                            q_kept=bool(torch.equal(q, qk)), schur_finite=bool(eager.isfinite().all()))
    return out


def _worker(port, q):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.set_num_threads(8)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        try:
            res = ("ok", sc_strip_nd_T_view(dist, dev))
        except Exception:
            res = ("error", traceback.format_exc())
    finally:
        q.put(res)
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_strip_schur_T_capture_over_rccl(gpu):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(_free_port(), q))
    p.start()
    status, out = q.get(timeout=240)
    p.join(timeout=60)
    assert p.exitcode == 0, p.exitcode
    assert status == "ok", out
    print(out)
    for key, r in out.items():
        assert r["kind"] and r["gather_device"].startswith("cuda"), (key, r)
        assert r["captured"], (key, r)
        assert r["replay_vs_eager"] <= 1e-12, (key, r)
        assert r["b_kept"] and r["finite"], (key, r)
        # an eager transposed solve: the reduced system's all-reduce and the Dirichlet end nodes', no all-gather
        assert r["solve_reduces"] == 2 and r["solve_gathers"] == 0, (key, r)
        assert r["schur_graph"], (key, r)
        assert r["schur_graph_vs_eager"] <= 1e-12, (key, r)
        assert r["q_kept"] and r["schur_finite"], (key, r)
