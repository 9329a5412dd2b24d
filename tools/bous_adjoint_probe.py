"""The coupled adjoint solve of the Boussinesq coupler beside the forward linear solve of one Newton step, on one
linearisation, in one process:

  * regular cases (odd element counts, even P; default 15 x 15, P = 8 at Ra = 1e3 and, by continuation, 1e4): the
    coupler is converged and linearised there; solve_adjoint (right-hand side: the gradient of WallNusselt("W"))
    against _linear_jnk (right-hand side: -dR/dRa, the tangent system of the same derivative).  Both are warmed once
    (factors, graphs), then timed --trials times, alternated, with a host clock around a device synchronise: median
    and range.  Reported per solve: coupled GMRES iterations, block-solve counts, Schur matvecs of the last NS block
    solve, the true residual gmres_left ended on, and dNu_W/dRa from either side (adjoint: -lam^T dR/dRa; tangent:
    g^T dx/dRa).  One more adjoint solve runs with a synchronise on either side of every jacobian_apply_T for the
    share of the solve's wall time spent there (the coupler's own timing keys are host clocks around asynchronous
    launches);
  * the even case (default 8 x 8, P = 4): the equal-order Jacobian is singular there, and solve_adjoint must end with
    a RuntimeError -- its own after --even-maxiter restarts, or before that the NS block's, whose adjoint Schur solve
    meets the same singular system: the outcome, the block solves completed, the residual it stopped on (if it got
    that far) and the time are recorded for WallNusselt and KineticEnergy.

Writes bous_adjoint_<nex>x<ney>_P<P>.json per mesh under --out.  No threshold: the numbers go to DESIGN.md.

python tools/bous_adjoint_probe.py [--mesh 8:15:15] [--Ra 1e3,1e4] [--even 4:8:8] [--even-maxiter 5]
                                   [--even-schur-maxiter 0] [--trials 5] [--out profiles/bous_adjoint]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RE, PR = 1e3, 0.71


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "trials": [float(x) for x in v]}


def coupler(P, nex, ney, Ra):
    from sem_amd.solvers.boussinesq import BoussinesqCoupler
    return BoussinesqCoupler(1.0, 1.0, RE, Ra, PR, P, nex, ney, P, nex, ney, mode="JNK")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def counted(c, fn, keys):
    """fn() with the coupler's call counters of `keys` over it."""
    before = {k: c.calls[k] for k in keys}
    out, dt = wall(fn)
    return out, dt, {k: c.calls[k] - before[k] for k in keys}


def regular_case(c, x, trials):
    """solve_adjoint against _linear_jnk at the state x (working form) of the converged coupler c."""
    from sem_amd.solvers.functionals import WallNusselt
    F = WallNusselt("W")
    rnorm = c._norm(c.residuals(x))
    c.linearize(x)
    g = F.gradient(c, x)
    dRdRa = c.residual_partials(x, "Ra")
    adj_keys = ("jacobian_apply_T", "cd_update_T", "ns_update_T")
    fwd_keys = ("jacobian_apply", "cd_update", "ns_update")
    adjoint = lambda: c.solve_adjoint(g)            # noqa: E731
    forward = lambda: c._linear_jnk(-dRdRa)         # noqa: E731
    lam, _, n_adj = counted(c, adjoint, adj_keys)   # warm-up: transposed factor plan, graphs
    adj_info = {"gmres_iterations": c.adjoint_iterations, "true_residual": c.adjoint_res_norm, "calls": n_adj,
                "last_ns_schur_matvecs": c.ns.schur_matvecs, "last_cd_matvecs": c.cd.matvecs}
    its = [0]
    # _linear_jnk logs one line per iteration
    c._log = lambda msg: its.__setitem__(0, its[0] + msg.startswith("  GMRES "))
    try:
        dx, _, n_fwd = counted(c, forward, fwd_keys)
    finally:
        del c._log
    fwd_info = {"calls": n_fwd, "gmres_iterations": its[0], "last_ns_schur_matvecs": c.ns.schur_matvecs,
                "last_cd_matvecs": c.cd.matvecs,
                "true_residual": c._norm(c.jacobian_apply(dx) + dRdRa)}
    t_adj, t_fwd = [], []
    for _ in range(trials):
        t_adj.append(wall(adjoint)[1])
        t_fwd.append(wall(forward)[1])
    # the share of jacobian_apply_T: one more solve, a synchronise on either side of every transposed apply
    spent = [0.0]
    plain = c.jacobian_apply_T

    def synced(w):
        out, dt = wall(lambda: plain(w))
        spent[0] += dt
        return out

    c.jacobian_apply_T = synced
    try:
        _, t_total = wall(adjoint)
    finally:
        del c.jacobian_apply_T
    return {"residual_norm_at_x": rnorm, "atol_nonlin": c.atol_nonlin, "atol_gmres": c.atol_gmres,
            "restart": c.restart, "adjoint": adj_info, "forward": fwd_info,
            "adjoint_seconds": stats(t_adj), "forward_seconds": stats(t_fwd),
            "ratio_adjoint_over_forward": float(np.median(t_adj) / np.median(t_fwd)),
            "jacobian_apply_T_share": {"apply_seconds": spent[0], "solve_seconds": t_total,
                                       "share": spent[0] / t_total},
            "Nu_W": F.value(c, x), "lam_2norm": c._norm(lam),
            "dNu_W_dRa_adjoint": -torch.dot(lam, dRdRa).item(), "dNu_W_dRa_tangent": torch.dot(g, dx).item()}


def even_case(P, nex, ney, maxiter, schur_maxiter):
    from sem_amd.solvers.functionals import KineticEnergy, WallNusselt
    c = coupler(P, nex, ney, 1e3)
    rep = {"config": f"{nex}x{ney} P={P}", "Ra": 1e3, "maxiter": maxiter, "restart": c.restart,
           "atol_gmres": c.atol_gmres}
    (sol, t_solve) = wall(c.solve)
    x = c.to_local(np.concatenate(sol))
    rep["forward_solve"] = {"seconds": t_solve, "newton_iterations": c.iterations}
    c.residuals(x)
    c.linearize(x)
    # --even-schur-maxiter: a cap on the NS block's inner Schur solves (0: the solver's own, 10 N iterations)
    rep["ns_schur_maxiter"] = schur_maxiter or None
    c.ns._schur_maxiter = schur_maxiter or None
    for F in (WallNusselt("W"), KineticEnergy()):
        g = F.gradient(c, x)
        c.adjoint_iterations = c.adjoint_res_norm = None
        c.restart_jumps = 0
        before = dict(c.calls)
        t0 = time.perf_counter()
        try:
            c.solve_adjoint(g, maxiter=maxiter)
            outcome = "converged"
        except RuntimeError as e:
            outcome = f"RuntimeError: {e}"
        torch.cuda.synchronize()
        rep[F.name] = {"outcome": outcome, "seconds": time.perf_counter() - t0, "rhs_2norm": c._norm(g),
                       "gmres_iterations": c.adjoint_iterations, "true_residual": c.adjoint_res_norm,
                       "restart_jumps": c.restart_jumps,
                       "calls": {k: c.calls[k] - before[k] for k in ("jacobian_apply_T", "cd_update_T", "ns_update_T")}}
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="8:15:15", help="P:nex:ney of the regular cases ('' to skip)")
    ap.add_argument("--Ra", default="1e3,1e4", help="Rayleigh numbers, reached by continuation in this order")
    ap.add_argument("--even", default="4:8:8", help="P:nex:ney of the even case ('' to skip)")
    ap.add_argument("--even-maxiter", type=int, default=5)
    ap.add_argument("--even-schur-maxiter", type=int, default=0)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "bous_adjoint"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    dev = torch.cuda.get_device_name(0)

    def write(rep, P, nex, ney):
        rep["device"] = dev
        print(json.dumps(rep), flush=True)
        with open(os.path.join(a.out, f"bous_adjoint_{nex}x{ney}_P{P}.json"), "w") as f:
            json.dump(rep, f, indent=1)

    if a.mesh:
        P, nex, ney = map(int, a.mesh.split(":"))
        rep = {"config": f"{nex}x{ney} P={P}", "Re": RE, "Pr": PR, "trials": a.trials, "cases": []}
        x = None
        for Ra in map(float, a.Ra.split(",")):
            c = coupler(P, nex, ney, Ra)
            sol, t_solve = wall(lambda: c.solve(x))
            x = np.concatenate(sol)
            case = {"Ra": Ra, "DOF": c.DOF, "forward_solve": {"seconds": t_solve, "newton_iterations": c.iterations}}
            case.update(regular_case(c, c.to_local(x), a.trials))
            rep["cases"].append(case)
            write(rep, P, nex, ney)       # after every case: a later failure keeps the earlier numbers
    if a.even:
        P, nex, ney = map(int, a.even.split(":"))
        write(even_case(P, nex, ney, a.even_maxiter, a.even_schur_maxiter), P, nex, ney)


if __name__ == "__main__":
    main()
