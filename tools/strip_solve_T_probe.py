"""What the transposed strip line solve costs, on one MI355X (in the style of tools/cond_transpose_probe.py and of
tools/strip_profile.py's loopback group).

  kernel  -- sem_gemv_rows_t at the cfg5 shapes (m = 3,074: the m x m and m x 2m sweep operators, X01 = 7m x 2m,
             Z = 2m x 9m), both lane forms, against sem_gemv_rows on the same operator (the same bytes, the forward
             product) and against torch's A.mT @ x, alternated in one process.  Operators below 1 GB are cycled over
             enough copies that no call finds its operator in the 256 MB MALL.  GB/s = operator bytes / time.
  solve   -- ONE process as rank r of G (strip_profile.LoopbackDist: the collectives are local no-ops with the real
             shapes): the partitioned convection-diffusion solver's StripLineSolver(adjoint=True), its forward and
             its transposed line solve on the same factor, eager and graph-captured.  Values from "other ranks" are
             stand-ins: timing only.  A multi-GPU timing needs an RCCL run over real ranks and is not made here.

Writes JSON to --out (default profiles/strip_solve_T/)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def timed_ms(fns, dev, reps, rounds):
    """Median over `rounds` of the device time of `reps` back-to-back calls of each fn, the fns alternated."""
    out = {k: [] for k in fns}
    for k, f in fns.items():
        f(0)
    torch.cuda.synchronize(dev)
    for _ in range(rounds):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(reps):
                f(i)
            b.record()
            torch.cuda.synchronize(dev)
            out[k].append(a.elapsed_time(b) / reps)
    return {k: float(np.median(v)) for k, v in out.items()}


def kernel_rates(args, dev):
    from sem_amd import _lib
    lib = _lib.load()
    v = C.c_void_p
    m = args.m
    shapes = {"m x m": (m, m), "m x 2m": (m, 2 * m), "X01 7m x 2m": (7 * m, 2 * m), "Z 2m x 9m": (2 * m, 9 * m)}
    recs = []
    for name, (M, K) in shapes.items():
        nbytes = M * K * 8
        copies = max(1, min(8, int(np.ceil(1.2e9 / nbytes))))
        A = torch.rand((copies, M, K), dtype=torch.float64, device=dev) - 0.5
        xr, yc = (torch.rand(M, dtype=torch.float64, device=dev) for _ in range(2))
        xc, yr = torch.rand(K, dtype=torch.float64, device=dev), torch.empty(K, dtype=torch.float64, device=dev)
        st = v(torch.cuda.current_stream(dev).cuda_stream)

        def fwd(i):
            _lib.check(lib.sem_gemv_rows(M, K, 1.0, v(A[i % copies].data_ptr()), K, v(xc.data_ptr()), 0.0,
                                         v(yc.data_ptr()), st))

        def tr(form):
            return lambda i: _lib.check(lib.sem_gemv_rows_t(M, K, 1.0, v(A[i % copies].data_ptr()), K,
                                                            v(xr.data_ptr()), 0.0, v(yr.data_ptr()), form, st))

        def tor(i):
            torch.mv(A[i % copies].mT, xr, out=yr)

        ms = timed_ms({"sem_gemv_rows": fwd, "rows_t wide": tr(1), "rows_t narrow": tr(2), "rows_t by size": tr(0),
                       "torch A.mT @ x": tor}, dev, args.reps, args.rounds)
        want = A[0].mT @ xr
        tr(1)(0)
        err = float((yr - want).abs().max() / want.abs().max())
        rec = dict(shape=name, M=M, K=K, MB=nbytes / 1e6, copies=copies, rel_err_vs_torch=err,
                   us={k: 1e3 * t for k, t in ms.items()}, GBps={k: nbytes / 1e9 / (t / 1e3) for k, t in ms.items()})
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del A
    return recs


def solve_times(args, dev):
    from strip_profile import LoopbackDist, loopback_gather
    from sem_amd.parallel import Partition
    from sem_amd.solvers import ConvectionDiffusionSolver
    from sem_amd.solvers.strip_solve import _StripReduced
    fake = LoopbackDist(args.G, args.rank)
    _StripReduced._all_gather = loopback_gather(fake)
    cd = ConvectionDiffusionSolver(1.0, 1.0, 40.0, args.P, args.ne, args.ne, T_W=0.5, T_E=-0.5, mtol=1e-10,
                                   partition=Partition(fake), partition_adjoint="condensed")
    r = np.random.default_rng(1)
    T, u, v = (r.uniform(-1, 1, cd.N) for _ in range(3))
    cd._get_residuals(T, u, v)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    vs = cd._jacobian_solver()
    torch.cuda.synchronize(dev)
    rec = dict(G=args.G, rank=args.rank, P=args.P, ne=args.ne, m=vs.m, lines=vs.nex + 1, factor_s=time.perf_counter() - t0,
               interior_sweep=vs._T[0][0] if vs._T is not None else None, forward_graph=vs._graph is not None)
    rec["transposed_graph"] = bool(vs.capture_T())
    B = torch.rand((vs.NX, vs.m), dtype=torch.float64, device=dev)

    def replay(s):
        g, b = getattr(vs, "_graph" + s), getattr(vs, "_bin" + s)
        b.copy_(B)
        return lambda i: g.replay()

    fns = {"forward eager": lambda i: vs._solve_lines_once(B), "transposed eager": lambda i: vs._solve_lines_once_T(B)}
    if vs._graph is not None and vs._graph_T is not None:
        fns.update({"forward graph": replay(""), "transposed graph": replay("_T")})
    rec["ms"] = timed_ms(fns, dev, max(1, args.reps // 4), args.rounds)
    rec["collectives"] = {k: c[0] for k, c in fake.calls.items()}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=3074)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--P", type=int, default=12)
    ap.add_argument("--ne", type=int, default=128)
    ap.add_argument("--G", type=int, default=8)
    ap.add_argument("--rank", type=int, default=3)
    ap.add_argument("--skip", default="", help="'kernel' or 'solve'")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strip_solve_T"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.makedirs(args.out, exist_ok=True)
    rec = dict(device=torch.cuda.get_device_name(0), args=vars(args))
    if args.skip != "kernel":
        rec["kernel"] = kernel_rates(args, dev)
        with open(os.path.join(args.out, "gemv_rows_t_rates.json"), "w") as f:
            json.dump(dict(device=rec["device"], m=args.m, reps=args.reps, rounds=args.rounds, shapes=rec["kernel"]), f,
                      indent=1)
    if args.skip != "solve":
        rec["solve"] = solve_times(args, dev)
        with open(os.path.join(args.out, f"strip_solve_T_P{args.P}_ne{args.ne}_G{args.G}.json"), "w") as f:
            json.dump(dict(device=rec["device"], **rec["solve"]), f, indent=1)


if __name__ == "__main__":
    main()
