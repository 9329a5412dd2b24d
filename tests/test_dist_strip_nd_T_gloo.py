"""World-size 1/2/3/8 gloo tests (CPU) of the TRANSPOSED element-partitioned nested-dissection velocity solve
(sem_amd/solvers/nested_dissection.py, StripNDSolver(adjoint=True)): the worker of tests/test_dist_strip_nd_gloo.py
with solve_T against SciPy's sparse solve of the whole transposed Jacobian (cond(J^T) = cond(J); odd element counts
in both directions wherever the world size allows it, cond(J) <= 1e9 asserted).  Also: shared lines, their Dirichlet
end nodes included, come out bitwise equal on the two neighbours; b is not modified; the forward solve of an
adjoint=True solver is bitwise a default-constructed one's, which refuses solve_T; one strip equals
NestedDissectionSolver.solve_T bitwise; a transposed solve issues at most two collectives; both leaf forms."""
import os
import queue
import time

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from test_dist_strip_nd_gloo import _free_port

TOL = 1e-9      # relative to max |x|: the forward strip solves' tolerance


class CountingDist:
    """torch.distributed with its collectives counted (the solvers call them on the `dist` object they are given)."""

    def __init__(self):
        self.calls = 0
        self.ReduceOp = dist.ReduceOp

    def all_reduce(self, *a, **kw):
        self.calls += 1
        return dist.all_reduce(*a, **kw)

    def all_gather(self, *a, **kw):
        self.calls += 1
        return dist.all_gather(*a, **kw)


def _worker(rank, world, port, case, reduced, smooth, split, q):
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
        from velocity_blocks import oracle_velocity_jacobian
        from sem_amd.parallel import StripPartition
        from sem_amd.solvers.nested_dissection import NestedDissectionSolver, StripNDSolver
        P, nex, ney, Re = case
        ref, u, v = oracle_velocity_jacobian(P, nex, ney, Re, seed=P * 10 + nex, smooth=smooth)
        J = ref.Jvelo
        part = StripPartition(nex, world)
        eb, ee = part.bounds[rank], part.bounds[rank + 1]
        NY, N = ney * P + 1, (nex * P + 1) * (ney * P + 1)
        sl = slice(eb * P * NY, (ee * P + 1) * NY)
        t = lambda a: torch.as_tensor(np.asarray(a)[sl].copy())  # noqa: E731
        kw = dict(c_stiff=1.0, c_gradx=Re, cu=t(u), c_grady=Re, cv=t(v), juu=t(Re * (ref.Gx @ u)),
                  jvv=t(Re * (ref.Gy @ v)), juv=t(Re * (ref.Gy @ u)), jvu=t(Re * (ref.Gx @ v)))
        cd = CountingDist()

        def factored(**extra):
            vs = StripNDSolver(P, nex, ney, "cpu", part.bounds, rank, cd, **extra)
            vs.factor_coeffs(1.0 / nex, 1.0 / ney, **kw)
            return vs

        vs, plain = factored(adjoint=True), factored()
        assert vs._steps_T is None       # the transposed plan is lazy
        r = np.random.default_rng(17)
        b = r.uniform(-1, 1, 2 * N)
        want = spla.spsolve(J.T.tocsc(), b)
        comps = [torch.as_tensor(b[c * N:(c + 1) * N][sl].copy()) for c in range(2)]
        keep = [c.clone() for c in comps]
        vs.solve_T(*comps)                       # builds the plan
        n0 = cd.calls
        got = vs.solve_T(*comps)
        ncoll = cd.calls - n0
        fwd, fwd_plain = vs.solve(*comps), plain.solve(*comps)
        try:
            plain.solve_T(*comps)
            refused = False
        except NotImplementedError as e:
            refused = "reduced system" in str(e)
        err = max(np.abs(g.numpy() - want[c * N:(c + 1) * N][sl]).max() for c, g in enumerate(got))
        same_whole = None
        if world == 1:
            whole = NestedDissectionSolver(P, nex, ney, "cpu")
            whole.factor_coeffs(1.0 / nex, 1.0 / ney, **kw)
            same_whole = all(torch.equal(a, c) for a, c in zip(got, whole.solve_T(*comps)))
        kinds = [st[0] for st in vs._steps_T]
        q.put((rank, dict(err=err / np.abs(want).max(), refused=refused, ncoll=ncoll, same_whole=same_whole, split=vs.split,
                          cond=float(np.linalg.cond(J.toarray())) if rank == 0 else None,
                          leaf_kinds=(kinds.count("leafT"), kinds.count("sparseT")),
                          same_fwd=all(torch.equal(a, c) for a, c in zip(fwd, fwd_plain)),
                          b_kept=all(torch.equal(a, c) for a, c in zip(comps, keep)),
                          first=[g.numpy()[:NY].copy() for g in got], last=[g.numpy()[-NY:].copy() for g in got])))
    finally:
        dist.destroy_process_group()


# smooth = 0: random velocity fields, whose split-leaf probe may exceed SPLIT_ETA (the dense Xi leaves: sparseT + X_i^T;
# each strip decides for its own elements, so `split` is pinned only where it is known: None = either);
# smooth = 0.3: smooth fields, the split leaves (leafT) -- as SPLIT_CASES of tests/test_nd_transpose.py
@pytest.mark.parametrize("world,case,reduced,smooth,split", [
    (1, (4, 3, 2, 300.0), None, 0.0, False),
    (2, (4, 4, 3, 300.0), None, 0.0, None),     # two columns per strip
    (2, (3, 2, 4, 100.0), None, 0.0, None),     # one column per strip: the root is a horizontal cut of a 1 x 4 piece
    (3, (4, 7, 2, 700.0), None, 0.0, None),     # uneven strips (3, 2, 2 columns)
    (8, (3, 9, 3, 100.0), None, 0.0, None),     # cfg5's world size over 9 columns (2, 1, 1, 1, 1, 1, 1, 1)
    (2, (4, 4, 3, 300.0), "cr", 0.0, None),     # the replicated transposed cyclic reduction of the reduced system
    (1, (4, 3, 2, 100.0), None, 0.3, True),      # the split leaves, one strip
    (3, (4, 7, 3, 100.0), None, 0.3, True),      # the split leaves across strips
    (2, (3, 3, 1, 100.0), None, 0.0, None),     # strips of 2 and 1 columns, ney = 1: rank 1's root is one element
])
def test_strip_nd_solver_T_gloo(world, case, reduced, smooth, split):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, case, reduced, smooth, split, q)) for r in range(world)]
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
    print("cond(J)", res[0]["cond"])
    assert res[0]["cond"] <= 1e9
    for rank, e in sorted(res.items()):
        print(rank, e["err"], e["ncoll"])
        assert e["err"] <= TOL, (rank, e["err"])
        assert e["refused"] and e["same_fwd"] and e["b_kept"], (rank, e["refused"], e["same_fwd"], e["b_kept"])
        assert e["ncoll"] <= 2 and (world > 1 or e["ncoll"] == 0), (rank, e["ncoll"])
        assert e["leaf_kinds"] == ((1, 0) if e["split"] else (0, 1)), e["leaf_kinds"]
        assert split is None or e["split"] == split, (rank, e["split"])
        assert e["same_whole"] in (None, True)
    assert world > 1 or res[0]["same_whole"] is True
    for rank in range(world - 1):     # the shared line: bitwise equal on its two neighbours, end nodes included
        for a, c in zip(res[rank]["last"], res[rank + 1]["first"]):
            assert np.array_equal(a, c), rank
