"""The adjoint Navier-Stokes launches and matvecs against their forward counterparts, variants alternated in one
process (median and range of --trials rounds), at cfg4 (48^2, P = 8) and cfg5 (128^2, P = 12):

  * kernels: the forward Schur gradient / divergence forms of sem_ns_apply (band form; the LDS-tile form too, whose
    layout sem_ns_apply_transpose shares) against the transposed gradient / divergence forms, and the full transposed
    apply against the forward differential -- graph-replayed launches timed with HIP events (tools/nsbench.py's timer);
  * Schur matvecs on one linearisation: the forward _SchurComplement and the adjoint _SchurComplementT under graph
    replay, the adjoint matvec eager, and the adjoint matvec composed from Mesh.apply_transpose / Mesh.apply / torch
    pointwise operations (tools/ns_adjoint_composed.py, eager: five operator launches and the masks, the A/B baseline of
    the two fused launches);
  * --solve 1: one adjoint update (_get_update_T) beside the forward _get_update on a right-hand side of the same
    norm, linearised at the lid-driven state _get_solution reaches (Re = --Re): matvec counts and times; each of the
    two Krylov solves stops after --maxiter iterations (default 5000) and is then reported as not converged.

python tools/ns_adjoint_probe.py [--meshes 8:48,12:128] [--reps 200] [--trials 5] [--solve 0] [--Re 400] [--maxiter 5000]
                                    [--out DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nsbench import timed  # noqa: E402


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "trials": [float(x) for x in v]}


def kernel_report(m, reps, trials):
    """us per launch of the forward and transposed forms on random fields (the solvers' descriptors)."""
    from sem_amd import _lib
    lib = _lib.load()
    dev = m.device
    N, NX, NY = m.n_local, m.NX, m.NY
    sides = _lib.SIDE_W | _lib.SIDE_E | _lib.SIDE_S | _lib.SIDE_N
    vec = lambda: torch.rand(N, dtype=torch.float64, device=dev) * 2 - 1  # noqa: E731
    p, rc, cu, cv = vec(), vec(), vec(), vec()
    du, dv, ru, rv = vec(), vec(), vec(), vec()
    jac = dict(juu=vec(), juv=vec(), jvu=vec(), jvv=vec())
    B = torch.rand((NX, 2 * NY), dtype=torch.float64, device=dev)
    Y = torch.empty_like(B)
    rows = dict(dir_sides=sides, pin=N // 2)
    sysk = dict(c_stiff=1.0, c_gradx=1e3, cu=cu, c_grady=1e3, cv=cv)
    bu, bv, xu, xv = B[:, :NY], B[:, NY:], Y[:, :NY], Y[:, NY:]
    forms = {
        "gradient": lambda: m.ns_apply(None, None, p, bu, bv, **rows),
        "gradient_T": lambda: m.ns_apply_transpose(None, None, p, bu, bv, c_div=-1.0, **rows),
        "divergence": lambda: m.ns_apply(bu, bv, p, rc=rc, c_div=-1.0, **rows),
        "divergence_T": lambda: m.ns_apply_transpose(bu, bv, p, yp=rc, **rows),
        "velocity_rows": lambda: m.ns_apply(bu, bv, None, xu, xv, **sysk, **jac, **rows),
        "velocity_rows_T": lambda: m.ns_apply_transpose(bu, bv, None, xu, xv, **sysk, **jac, **rows),
        "dresidual": lambda: m.ns_apply(du, dv, p, ru, rv, rc, **sysk, **jac, **rows),
        "dresidual_T": lambda: m.ns_apply_transpose(du, dv, p, ru, rv, rc, **sysk, **jac, **rows),
    }
    tile = {k: forms[k] for k in ("gradient", "divergence", "velocity_rows", "dresidual")}
    us = {k: [] for k in forms}
    us.update({k + "_tile": [] for k in tile})
    for _ in range(trials):
        for k, fn in forms.items():
            us[k].append(timed(fn, reps))
        _lib.check(lib.sem_set_tuning(_lib.TUNE_NS_APPLY, 1))      # the forward LDS-tile form
        for k, fn in tile.items():
            us[k + "_tile"].append(timed(fn, reps))
        _lib.check(lib.sem_set_tuning(_lib.TUNE_NS_APPLY, 0))
    out = {k: stats(v) for k, v in us.items()}
    for k in tile:
        out[f"ratio_{k}_T_over_forward"] = out[k + "_T"]["median"] / out[k]["median"]
        out[f"ratio_{k}_T_over_forward_tile"] = out[k + "_T"]["median"] / out[k + "_tile"]["median"]
    return out


def event_ms(fn, n):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def linearised(P, ne, Re, solve):
    """A solver linearised at a smooth cell (tools/nd_probe.py's state), or, for --solve, at the lid-driven solution."""
    from sem_amd.solvers import NavierStokesSolver
    ns = NavierStokesSolver(1.0, 1.0, Re, 0.0, P, ne, ne, u_N=1.0, mtol=1e-10, mtol_newton=1e-8, iprint=[])
    N = ns.N
    x, y = ns.points
    if solve:
        u, v, p = ns._get_solution(np.zeros(N))
        ns._get_residuals(u, v, p, np.zeros(N))
    else:
        u = 1e-2 * np.sin(np.pi * x) * np.sin(2 * np.pi * y)
        v = -1e-2 * np.sin(2 * np.pi * x) * np.sin(np.pi * y)
        ns._get_residuals(u, v, np.zeros(N), np.zeros(N))
    ns._calc_jacobians(u, v)
    return ns


def matvec_report(ns, solves, trials):
    """ms per Schur matvec: forward and adjoint under graph replay, the adjoint eager, the composed adjoint (eager)."""
    from ns_adjoint_composed import ComposedSchurT
    from sem_amd.solvers.navier_stokes import _SchurComplement, _SchurComplementT
    vs = ns._velocity_solver_T()
    q = torch.rand(ns.N, dtype=torch.float64, device=ns._mesh.device) * 2 - 1
    fwd = _SchurComplement(ns, vs, graph=True)
    adj = _SchurComplementT(ns, vs, graph=True)
    comp = ComposedSchurT(ns, vs)
    variants = {"forward_graph": lambda: fwd(q), "adjoint_graph": lambda: adj(q), "adjoint_eager": lambda: adj._body(q),
                "adjoint_composed_eager": lambda: comp(q)}
    ms = {k: [] for k in variants}
    for _ in range(trials):
        for k, fn in variants.items():
            ms[k].append(event_ms(fn, solves))
    out = {k: stats(v) for k, v in ms.items()}
    out["graphs"] = {"forward": fwd._graph is not None, "adjoint": adj._graph is not None}
    out["ratio_adjoint_over_forward_graph"] = out["adjoint_graph"]["median"] / out["forward_graph"]["median"]
    out["ratio_fused_over_composed_eager"] = out["adjoint_eager"]["median"] / out["adjoint_composed_eager"]["median"]
    a, c = adj._body(q), comp(q)
    out["fused_vs_composed_rel_diff"] = float((a - c).abs().max() / c.abs().max())
    out["refine_T"], out["refine"] = bool(vs.refine_T), bool(vs.refine)
    return out


def solve_report(ns, maxiter):
    """One adjoint update beside one forward update on right-hand sides of the same norm, each in the range of its
    operator (b = A d and b = A^T w for random d, w: on a mesh with an even element count the equal-order Jacobian is
    singular up to rounding and a random right-hand side would be inconsistent for either system).  maxiter caps both
    Krylov solves; a solve that does not get there is reported, not waited for."""
    dev = ns._mesh.device
    g = torch.Generator(device=dev).manual_seed(3)
    d = [torch.rand(ns.N, dtype=torch.float64, device=dev, generator=g) * 2 - 1 for _ in range(3)]
    norm = lambda vs: float(torch.sqrt(sum(v.square().sum() for v in vs)))   # noqa: E731
    b_f = list(ns._get_dresiduals(*d))
    b_a = list(ns._get_dresiduals_T(*d))
    scale = norm(b_f) / norm(b_a)
    b_a = [v * scale for v in b_a]
    out = {"rhs_2norm": norm(b_f), "atol": ns._mtol * np.sqrt(ns.N), "maxiter": maxiter}
    saved, ns._schur_maxiter = ns._schur_maxiter, maxiter
    try:
        for name, fn, b, apply in (("forward", ns._get_update, b_f, ns._get_dresiduals),
                                   ("adjoint", ns._get_update_T, b_a, ns._get_dresiduals_T)):
            try:
                fn(*b)                            # the first call builds the factor's plan and the Schur graph
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                x = fn(*b)
                torch.cuda.synchronize(dev)
                out[name] = {"seconds": time.perf_counter() - t0, "schur_matvecs": ns.schur_matvecs,
                             "discarded": ns.schur_discarded,
                             "residual_2norm": norm([ri - bi for ri, bi in zip(apply(*x), b)])}
            except RuntimeError as e:
                out[name] = {"error": str(e)}
    finally:
        ns._schur_maxiter = saved
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="8:48,12:128")
    ap.add_argument("--reps", type=int, default=200, help="launches per graph replay of the kernel timings")
    ap.add_argument("--solves", type=int, default=10, help="matvecs per trial")
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--matvec", type=int, default=1, help="time the Schur matvecs (factors the velocity Jacobian)")
    ap.add_argument("--solve", type=int, default=0, help="also one adjoint and one forward update at the lid-driven state")
    ap.add_argument("--Re", type=float, default=400.0)
    ap.add_argument("--maxiter", type=int, default=5000, help="cap of the two Krylov solves of --solve")
    ap.add_argument("--out", default="", help="directory for ns_adjoint_P<P>_ne<ne>.json")
    a = ap.parse_args()
    from sem_amd.device import get_mesh
    for spec in a.meshes.split(","):
        P, ne = map(int, spec.split(":"))
        m = get_mesh(P, ne, ne, 1.0 / ne, 1.0 / ne)
        rep = {"config": f"{ne}x{ne} P={P}", "N": m.n_local, "device": torch.cuda.get_device_name(0)}
        reps = a.reps if m.n_local < 1e6 else max(20, a.reps // 10)
        rep["kernels_us"] = kernel_report(m, reps, a.trials)
        if a.matvec or a.solve:
            ns = linearised(P, ne, a.Re, a.solve)
            if a.matvec:
                rep["schur_matvec_ms"] = matvec_report(ns, a.solves, a.trials)
            if a.solve:
                rep["update"] = solve_report(ns, a.maxiter)
                rep["update"]["Re"] = a.Re
        print(json.dumps(rep), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"ns_adjoint_P{P}_ne{ne}.json"), "w") as f:
                json.dump(rep, f, indent=1)


if __name__ == "__main__":
    main()
