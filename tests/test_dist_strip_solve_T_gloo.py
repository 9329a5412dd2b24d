"""World-size 1/2/3/8 gloo tests (CPU) of the TRANSPOSED element-partitioned condensed direct solve
(sem_amd/solvers/strip_solve.py, StripLineSolver(adjoint=True)): the worker of tests/test_dist_strip_solve_gloo.py
with solve_T / solve1_T against SciPy's sparse solve of the whole transposed Jacobian, at that test's tolerance on
the same matrices (cond(J^T) = cond(J)).  Also: shared lines come out bitwise equal on the two neighbours, the
forward solve of an adjoint=True solver is bitwise the adjoint=False one's, and adjoint=False refuses."""
import os
import queue
import time

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from test_dist_strip_solve_gloo import _free_port, strip_pieces


def _worker(rank, world, port, case, reduced, q):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if reduced:
        os.environ["SEM_STRIP_REDUCED"] = reduced
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import torch as _torch
    from threadpoolctl import threadpool_limits
    threadpool_limits(1)   # ranks share the host: no BLAS / OpenMP oversubscription
    _torch.set_num_threads(1)
    try:
        import scipy.sparse.linalg as spla
        import torch
        from velocity_blocks import extract, oracle_cd_jacobian, oracle_velocity_jacobian
        from sem_amd.parallel import StripPartition
        from sem_amd.solvers.strip_solve import StripLineSolver
        P, nex, ney, Re, ncomp, blocklu = case
        if ncomp == 2:
            ref, _, _ = oracle_velocity_jacobian(P, nex, ney, Re, seed=P * 10 + nex)
            J = ref.Jvelo
        else:
            ref, J, _, _ = oracle_cd_jacobian(P, nex, ney, Re, seed=P + nex)
        pcs = extract(J.toarray(), P, nex, ney, ncomp=ncomp)
        part = StripPartition(nex, world)

        def factored(adjoint):
            vs = StripLineSolver(P, nex, ney, "cpu", part.bounds, rank, dist, ncomp=ncomp, adjoint=adjoint)
            if blocklu:
                vs.edge_dense_max = 0
            sp_ = {k: torch.as_tensor(v) for k, v in strip_pieces(pcs, P, part.bounds, rank).items()}
            vs.factor_condensed(None, pieces=vs.condense_dense(sp_.pop("AII")), line=sp_)
            return vs

        vs, plain = factored(True), factored(False)
        NY, N = ney * P + 1, (nex * P + 1) * (ney * P + 1)
        r = np.random.default_rng(17)
        b = r.uniform(-1, 1, ncomp * N)
        want = spla.spsolve(J.T.tocsc(), b)
        eb, ee = part.bounds[rank], part.bounds[rank + 1]
        sl = slice(eb * P * NY, (ee * P + 1) * NY)
        comps = [torch.as_tensor(b[c * N:(c + 1) * N][sl]) for c in range(ncomp)]
        keep = [c.clone() for c in comps]
        if ncomp == 2:
            got, fwd, fwd_plain = vs.solve_T(*comps), vs.solve(*comps), plain.solve(*comps)
            refuse = lambda: plain.solve_T(*comps)      # noqa: E731
        else:
            got, fwd, fwd_plain = (vs.solve1_T(comps[0]),), (vs.solve1(comps[0]),), (plain.solve1(comps[0]),)
            refuse = lambda: plain.solve1_T(comps[0])   # noqa: E731
        err = max(np.abs(g.numpy() - want[c * N:(c + 1) * N][sl]).max() for c, g in enumerate(got))
        try:
            refuse()
            refused = False
        except NotImplementedError as e:
            refused = "condensation" in str(e)
        q.put((rank, dict(err=err / np.abs(want).max(), refused=refused,
                          same_fwd=all(torch.equal(a, c) for a, c in zip(fwd, fwd_plain)),
                          b_kept=all(torch.equal(a, c) for a, c in zip(comps, keep)),
                          first=[g.numpy()[:NY].copy() for g in got], last=[g.numpy()[-NY:].copy() for g in got])))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,case,reduced", [
    (1, (4, 3, 2, 300.0, 2, False), None),
    (2, (4, 4, 3, 300.0, 2, False), None),    # one interior line per strip: both boundary products land on it
    (2, (3, 2, 4, 100.0, 2, True), None),     # no interior line
    (3, (4, 7, 2, 700.0, 2, False), None),    # uneven strips (3, 2, 2 columns)
    (2, (3, 9, 2, 300.0, 2, False), None),    # strips of 5 and 4 columns: the twisted interior sweep
    (3, (5, 6, 3, 40.0, 1, False), None),     # the one-component (CD) operator
    (8, (3, 9, 3, 40.0, 1, True), None),      # cfg5's world size
    (2, (4, 4, 3, 300.0, 2, False), "cr"),    # the replicated transposed cyclic reduction of the reduced system
])
def test_strip_line_solver_T_gloo(world, case, reduced):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, case, reduced, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, t0 = {}, time.time()
    while len(res) < world:
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
        print(rank, e["err"])
        assert e["err"] < 1e-10, (rank, e["err"])
        assert e["refused"] and e["same_fwd"] and e["b_kept"], (rank, e["refused"], e["same_fwd"], e["b_kept"])
    for rank in range(world - 1):     # the shared line: bitwise equal on its two neighbours
        for a, c in zip(res[rank]["last"], res[rank + 1]["first"]):
            assert np.array_equal(a, c), rank
