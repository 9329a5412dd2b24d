"""Record what the solvers' Python drivers compute, so that a change of the drivers alone can be compared
run against run (profiles/solver_drivers/).

python tools/solver_drivers.py --out digests.json             iteration counts and SHA-256 digests (GPU)
python tools/solver_drivers.py --time 20 --out times.json     wall time of NavierStokesSolver._get_update (GPU)
python tools/solver_drivers.py --gloo --out gloo.json         the partitioned paths at world 2 (CPU, gloo)

--root DIR imports sem_amd from another checkout (the library is taken from SEM_LIBDIR when set).

Digest cases: the lid-driven Navier-Stokes _get_solution at P = 4, 5 x 5 elements, Re = 100 under both Schur
preconditioners and _get_update_T on the solution's linearisation; the convection-diffusion _get_solution and
_get_update_T at P = 4, 4 x 3 elements, Pe = 40 with and without the condensed preconditioner.  --gloo: the same
solvers on two strips of tests/cpu_mesh*.py (deterministic), distributed and central updates.
"""
import argparse
import hashlib
import json
import os
import queue
import statistics
import sys
import time

import numpy as np


def sha(a):
    import torch
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def ns_cases(mk_ns, rec):
    for pc in ("mass", "pcd"):
        ns = mk_ns(schur_precond=pc)
        N = ns.N
        u, v, p = ns._get_solution(np.zeros(N))
        rec[f"ns_{pc}"] = {"newton_history": [[float(a), int(b)] for a, b in ns.newton_history],
                           "schur_matvecs": int(ns.schur_matvecs), "sha": [sha(a) for a in (u, v, p)]}
        if pc == "mass":
            ns._get_residuals(u, v, p, np.zeros(N))
            ns._calc_jacobians(u, v)
            r = np.random.default_rng(7)
            lam = ns._get_update_T(*(r.uniform(-1, 1, N) for _ in range(3)))
            rec["ns_mass_update_T"] = {"schur_matvecs": int(ns.schur_matvecs), "sha": [sha(a) for a in lam]}


def cd_cases(mk_cd, rec):
    for pc in ("condensed", None):
        cd = mk_cd(precond=pc)
        x, y = cd.points
        u, v = np.sin(np.pi * x) * np.cos(np.pi * y), -np.cos(np.pi * x) * np.sin(np.pi * y)
        T = cd._get_solution(u, v)
        e = {"matvecs": int(cd.matvecs), "sha": [sha(T)]}
        lam = cd._get_update_T(np.random.default_rng(11).uniform(-1, 1, cd.N))
        e["update_T"] = {"matvecs": int(cd.matvecs), "sha": [sha(lam)]}
        rec[f"cd_{pc}"] = e


def digests():
    from sem_amd.solvers import ConvectionDiffusionSolver, NavierStokesSolver
    rec = {}
    ns_cases(lambda **kw: NavierStokesSolver(1.0, 1.0, 100.0, 0.0, 4, 5, 5, u_N=1.0, iprint=[], **kw), rec)
    cd_cases(lambda **kw: ConvectionDiffusionSolver(1.0, 1.0, 40.0, 4, 4, 3, T_W=1.0, T_E=0.0, **kw), rec)
    return rec


def timings(n):
    """Median wall time of one _get_update (factor and graphs warm) at the first Newton step of the lid-driven
    cavity, Re = 100: the 5 x 5, P = 4 case and a mid-size 15 x 15, P = 8 one."""
    import torch
    from sem_amd.solvers import NavierStokesSolver
    rec = {}
    for name, P, ne in (("ns_5x5_P4", 4, 5), ("ns_15x15_P8", 8, 15)):
        ns = NavierStokesSolver(1.0, 1.0, 100.0, 0.0, P, ne, ne, u_N=1.0, iprint=[])
        z = torch.zeros(ns.N, dtype=torch.float64, device=ns._mesh.device)
        res = ns._get_residuals(z, z, z, z)
        ns._calc_jacobians(z, z)
        rhs = [-a for a in res]
        ns._get_update(*rhs)
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ns._get_update(*rhs)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        rec[name] = {"schur_matvecs": int(ns.schur_matvecs), "calls": n, "median_ms": 1e3 * statistics.median(ts),
                     "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}
    return rec


def _gloo_worker(rank, world, port, root, q):
    sys.path[:0] = [root, os.path.join(REPO, "tests"), REPO]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        from cpu_mesh_nsT import CPUStripMeshNST
        from cpu_mesh_T import CPUStripMeshT
        from oracle_solvers import OracleCD, OracleNS
        from sem_amd.parallel import Partition
        from sem_amd.solvers import ConvectionDiffusionSolver, NavierStokesSolver
        rec = {}
        P, nex, ney = 4, 3, 3
        N = (P * nex + 1) * (P * ney + 1)
        r = np.random.default_rng(3)
        u, v, p, T = (0.1 * r.uniform(-1, 1, N) for _ in range(4))
        rhs = [r.uniform(-1, 1, N) for _ in range(3)]
        for mode in ("distributed", "central"):
            ns = NavierStokesSolver(1.0, 1.0, 50.0, 0.0, P, nex, ney, u_N=1.0, iprint=[], mtol=1e-9,
                                    partition=Partition(dist, mesh_factory=CPUStripMeshNST), partition_update=mode)
            ns._central_solver = lambda: OracleNS(1.0, 1.0, 50.0, 0.0, P, nex, ney, mtol=1e-9)
            res = ns._get_residuals(u, v, p, T)
            ns._calc_jacobians(u, v)
            dr = ns._get_dresiduals(*rhs)
            d = ns._get_update(*rhs)
            rec[f"ns_{mode}"] = {"schur_matvecs": int(ns.schur_matvecs),
                                 "sha": [sha(a) for a in tuple(res) + tuple(dr) + tuple(d)]}
        x0 = r.uniform(-1, 1, N)
        for mode in ("distributed", "central"):
            cd = ConvectionDiffusionSolver(1.0, 1.0, 40.0, P, nex, ney, T_W=1.0, T_E=0.0, partition_update=mode,
                                           partition=Partition(dist, mesh_factory=CPUStripMeshT),
                                           partition_adjoint=True)
            cd._central_solver = lambda: OracleCD(1.0, 1.0, 40.0, P, nex, ney, T_W=1.0, T_E=0.0)
            Ts = cd._get_solution(u, v)
            e = {"matvecs": int(cd.matvecs), "sha": [sha(Ts)]}
            lam = cd._get_update_T(x0)
            e["update_T"] = {"matvecs": int(cd.matvecs), "sha": [sha(lam)]}
            rec[f"cd_{mode}"] = e
        q.put((rank, rec))
    finally:
        dist.destroy_process_group()


def gloo(root):
    import socket

    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, root, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    while len(res) < len(procs):     # stop when a rank dies instead of waiting out the queue
        try:
            k, v = q.get(timeout=2)
            res[k] = v
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):
                for p in procs:
                    p.terminate()
                raise SystemExit("a rank failed")
    for p in procs:
        p.join(timeout=60)
    return {f"rank{k}": res[k] for k in sorted(res)}


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--root", default=REPO, help="checkout whose sem_amd is measured")
    ap.add_argument("--time", type=int, default=0, help="time _get_update over this many calls per case")
    ap.add_argument("--gloo", action="store_true", help="the partitioned paths at world 2 on the CPU strip meshes")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    if args.gloo:
        rec = gloo(root)
    else:
        sys.path.insert(0, root)
        rec = timings(args.time) if args.time else digests()
    rec["label"] = args.label
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
