"""What the transposed strip nested-dissection solve and the adjoint strip Schur matvec cost, on one MI355X (in the
style of tools/strip_solve_T_probe.py and of tools/strip_profile.py's loopback group).

ONE process as rank r of G (strip_profile.LoopbackDist: the collectives are local no-ops with the real shapes): the
partitioned Navier-Stokes solver with partition_adjoint="distributed" on a cfg5 strip (default: 16 of 128 element
columns, P = 12), its StripNDSolver(adjoint=True).  Timed, alternated in one process, warm, the median of --rounds
(>= 20) repeats:

  solve  -- the forward and the transposed line solve on the same factor, eager and graph-captured;
  schur  -- the body of _StripSchur (gradient launch, two plain assemblies, stack into the line layout, solve,
            divergence launch, assembly) against the body of _StripSchurT (transposed launch into the line buffer,
            one line-layout assembly, transposed solve, transposed launch, assembly), eager and graph-captured.

Values from "other ranks" are stand-ins: timing only (the refinement gates are switched off, as strip_profile does).
A multi-GPU timing needs an RCCL run over real ranks and is not made here.  Writes JSON to --out (default
profiles/strip_nd_T/)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def timed_ms(fns, dev, reps, rounds):
    """Median (and min, max) over `rounds` of the device time of `reps` back-to-back calls of each fn, alternated."""
    out = {k: [] for k in fns}
    for f in fns.values():
        f()
    torch.cuda.synchronize(dev)
    for _ in range(rounds):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _i in range(reps):
                f()
            b.record()
            torch.cuda.synchronize(dev)
            out[k].append(a.elapsed_time(b) / reps)
    return {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=12)
    ap.add_argument("--ne", type=int, default=128)
    ap.add_argument("--G", type=int, default=8)
    ap.add_argument("--rank", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strip_nd_T"))
    args = ap.parse_args()
    if args.rounds < 20:
        ap.error("--rounds must be at least 20 (the medians that go into profiles/)")
    from strip_profile import LoopbackDist, loopback_gather, smooth_step
    from sem_amd.parallel import Partition
    from sem_amd.solvers import NavierStokesSolver
    from sem_amd.solvers.navier_stokes import _StripSchur, _StripSchurT
    from sem_amd.solvers.strip_solve import _StripReduced
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    fake = LoopbackDist(args.G, args.rank)
    _StripReduced._all_gather = loopback_gather(fake)
    ns = NavierStokesSolver(1.0, 1.0, 1e3, 1e6 / 0.71, args.P, args.ne, args.ne, mtol=1e-13, mtol_newton=1e-13,
                            iprint=[], partition=Partition(fake), partition_adjoint="distributed")
    x, y = ns.points
    u0, v0, _ = smooth_step(x, y)
    ns._get_residuals(10 * u0, 10 * v0, np.zeros(ns.N), 0.5 - x)
    ns._calc_jacobians(10 * u0, 10 * v0)
    m = ns._mesh
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    vs = ns._strip_velocity_solver_T()
    torch.cuda.synchronize(dev)
    rec = dict(device=torch.cuda.get_device_name(0), args=vars(args), strip=[m.ex_begin, m.ex_end], n_local=m.n_local,
               factor_and_gates_s=time.perf_counter() - t0, split_leaves=bool(vs.split),
               refine_eta_loopback=[vs.refine_eta, vs.refine_eta_T])
    vs.refine = vs.refine_T = False      # the stand-in reduced blocks make the gates' probes meaningless
    rec["forward_graph"], rec["transposed_graph"] = bool(vs.capture()), bool(vs.capture_T())
    B = torch.rand((vs.NX, vs.m), dtype=torch.float64, device=dev)

    def replay(s):
        g, b = getattr(vs, "_graph" + s), getattr(vs, "_bin" + s)
        b.copy_(B)
        return g.replay

    fns = {"forward eager": lambda: vs._solve_lines_once(B), "transposed eager": lambda: vs._solve_lines_once_T(B)}
    if rec["forward_graph"] and rec["transposed_graph"]:
        fns.update({"forward graph": replay(""), "transposed graph": replay("_T")})
    rec["solve_ms"] = timed_ms(fns, dev, args.reps, args.rounds)
    # the Schur bodies: the solves inside them are the eager line solves (the captured body is one graph)
    fwd, adj = _StripSchur(ns, vs, graph=True), _StripSchurT(ns, vs, graph=True)
    rec["schur_graphs"] = [fwd._graph is not None, adj._graph is not None]
    q = torch.rand(m.n_local, dtype=torch.float64, device=dev)
    fns = {"_StripSchur body eager": lambda: fwd._body(q), "_StripSchurT body eager": lambda: adj._body(q)}
    if all(rec["schur_graphs"]):
        fns.update({"_StripSchur graph": lambda: fwd(q), "_StripSchurT graph": lambda: adj(q)})
    rec["schur_ms"] = timed_ms(fns, dev, args.reps, args.rounds)
    s = rec["solve_ms"]
    rec["ratio_transposed_over_forward"] = {
        k: s[f"transposed {k}"]["median"] / s[f"forward {k}"]["median"] for k in ("eager", "graph")
        if f"forward {k}" in s}
    c = rec["schur_ms"]
    rec["ratio_schur_T_over_schur"] = {
        k: c[f"_StripSchurT {k}"]["median"] / c[f"_StripSchur {k}"]["median"] for k in ("body eager", "graph")
        if f"_StripSchur {k}" in c}
    rec["collectives"] = {k: v[0] for k, v in fake.calls.items()}
    rec["not_measured"] = "real multi-rank RCCL runs (the collectives here are local no-ops of the real shapes)"
    print(json.dumps(rec, indent=1), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"strip_nd_T_P{args.P}_ne{args.ne}_G{args.G}.json"), "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
