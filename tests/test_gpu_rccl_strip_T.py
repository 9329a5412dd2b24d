"""The device-collective branch of the transposed strip line solve, on one GPU (the pattern of
tests/test_gpu_rccl.py::sc_strip_view): ONE spawned process holds a real one-rank RCCL group and takes the G = 2
branches as rank r of 2 through tests/rank_view.RankView.  A partitioned convection-diffusion solver with
partition_adjoint="condensed" builds its StripLineSolver(adjoint=True); capture_T() must agree (its all-reduce inside
the hipGraph, the agreement reduces around it), a replay must equal the eager _solve_lines_T to 1e-12, and an eager
transposed solve must issue exactly one all-reduce and no all-gather.  Only rank-independent properties are checkable
under the view (a one-rank sum is the local tensor); the gloo tests carry correctness across ranks."""
import os
import socket
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

CD_CASE = dict(P=6, nex=12, ney=7, Pe=40.0)


def sc_strip_T_view(dist, dev):
    from rank_view import RankView
    from sem_amd.parallel import Partition
    from sem_amd.solvers import ConvectionDiffusionSolver
    from sem_amd.solvers.strip_solve import StripLineSolver
    c = CD_CASE
    out = {}
    for r in (0, 1):
        view = RankView(dist, 2, r)
        cd = ConvectionDiffusionSolver(1.0, 1.0, c["Pe"], c["P"], c["nex"], c["ney"], T_W=0.5, T_E=-0.5, mtol=1e-10,
                                       partition=Partition(view), partition_adjoint="condensed")
        rng = np.random.default_rng(5)
        T, u, v = (rng.uniform(-1, 1, cd.N) for _ in range(3))
        cd._get_residuals(T, u, v)
        vs = cd._jacobian_solver()
        n0 = dict(view.calls)
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
        count = lambda a, b, k: b.get(k, 0) - a.get(k, 0)   # noqa: E731
        out[f"r{r}"] = dict(kind=isinstance(vs, StripLineSolver) and vs.transpose and vs.G == 2,
                            gather_device=str(vs.gather_device), captured=bool(cap), replay_vs_eager=err,
                            b_kept=bool(torch.equal(B, keep)), finite=bool(want.isfinite().all()),
                            capture_reduces=count(n0, n1, "all_reduce"), capture_gathers=count(n0, n1, "all_gather"),
                            solve_reduces=count(n1, n2, "all_reduce"), solve_gathers=count(n1, n2, "all_gather"))
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
            res = ("ok", sc_strip_T_view(dist, dev))
        except Exception:
            res = ("error", traceback.format_exc())
    finally:
        q.put(res)
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_strip_line_solve_T_capture_over_rccl(gpu):
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
        assert r["captured"], (key, r)                      # both agreement reduces said yes
        assert r["replay_vs_eager"] <= 1e-12, (key, r)
        assert r["b_kept"] and r["finite"], (key, r)
        # capture_T: the all-reduce of the warm-up solve (the eager reference of the check) and of the captured solve,
        # and the two agreement reduces
        assert r["capture_reduces"] == 4 and r["capture_gathers"] == 0, (key, r)
        assert r["solve_reduces"] == 1 and r["solve_gathers"] == 0, (key, r)
