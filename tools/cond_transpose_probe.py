"""Probe of the transposed line condensation on one GPU process (not a benchmark gate; bench.py is untouched).

  python tools/cond_transpose_probe.py --case cfg2      # CD, 64 x 64, P = 8: one component, m = 513
  python tools/cond_transpose_probe.py --case ns48      # NS velocity pair, 48 x 48, P = 8: two components, m = 770

Reports, as JSON under profiles/cond_transpose/:
* solve / solve_T of the SAME factor under graph replay, alternated, median of 5 windows, with the factor bytes each
  reads computed from the shapes (vectors and index tables are left out: under 1 % of the operators), and the forward
  solve's "full" path (SEM_NESTED_BACK=full: two nested solves through Xi, the bytes the transposed solve reads) from a
  second factor of the same operator;
* the transposed solve's parts timed eagerly (the nested solve, the interface right-hand side, the transposed cyclic
  reduction), to name the launch that dominates;
* the transposed solve with sem_block_gemv_t's form forced wide, forced narrow and chosen by size (alternated A/B);
* (cfg2) the adjoint CD GMRES, matvecs and seconds, with the transposed preconditioner and with precond=None.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sem_amd import _lib  # noqa: E402
from sem_amd.solvers.velocity_solve import VelocityJacobianSolver  # noqa: E402

PE = 40.0


def factor_bytes(vs):
    """Bytes of stored operators one solve reads: forward "coupled" (the default), forward "full", transposed."""
    nel, ncol, ney, B = vs.nex * vs.ney, vs.nex, vs.ney, vs._ne1
    ni, G, m = vs._pi.shape[1], 2 * vs._ne1, vs.m
    Xi, Aei, Yie, XiB, AXB, ABY = ni * ni, G * ni, ni * G, ni * G, G * G, G * G
    E = (3 * ney + 1) * B * B
    cr = sum(lev[1].numel() + lev[4].numel() for lev in vs._cr) + vs._cr_top[1].numel()
    full = 2 * (nel * (Xi + Aei + Yie) + ncol * E) + cr
    coupled = nel * (Xi + Aei + ABY) + ncol * E + nel * (XiB + AXB + Yie) + ncol * E + cr
    return dict(coupled=8 * coupled, full=8 * full, transposed=8 * full, cr=8 * cr, m=m, ni=ni, ne1=B)


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def alternated(fns, reps=20, rounds=5):
    """Median over `rounds` of each function's window, the functions taking turns inside every round."""
    for fn in fns.values():
        window(fn, 3)
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(window(fn, reps))
    return {k: statistics.median(v) for k, v in t.items()}, {k: [min(v), max(v)] for k, v in t.items()}


def parts_T(vs, B):
    """The transposed solve's parts, eager, each timed on its own (median of 5 windows of 20)."""
    lib = _lib.load()
    P, nex, m = vs.P, vs.nex, vs.m
    vs._require_T()
    d = vs._hip_nested()
    _, _, _, yI, g, _ = vs._work
    st = C.c_void_p(torch.cuda.current_stream(vs.device).cuda_stream)
    v = C.c_void_p
    b1 = B.data_ptr() + 8 * m
    xB = vs._iface_solve_T(g)
    out = torch.empty_like(B)
    fns = {
        "nested_solve_t": lambda: _lib.check(lib.sem_nested_solve_t(C.byref(d), v(b1), P * m, None, None,
                                                                    v(yI.data_ptr()), vs.nI, st)),
        "nested_solve_t_coupled": lambda: _lib.check(lib.sem_nested_solve_t(
            C.byref(d), v(b1), P * m, v(vs._aBIp.data_ptr()), v(xB.data_ptr()), v(out.data_ptr() + 8 * m), P * m, st)),
        "interface_rhs": lambda: _lib.check(lib.sem_interface_rhs(P, nex, m, v(B.data_ptr()), m,
                                                                  v(vs._aIBp.data_ptr()), v(yI.data_ptr()), vs.nI,
                                                                  v(g.data_ptr()), st)),
        "cr_solve_T": lambda: vs._iface_solve_T(g),
        "cr_solve (forward)": lambda: vs._iface_solve(g.clone()),
    }
    med, _ = alternated(fns)
    return med


def solve_fns(vs, b):
    if vs.ncomp == 1:
        return (lambda: vs.solve1(b)), (lambda: vs.solve1_T(b))
    return (lambda: vs.solve(b, b)), (lambda: vs.solve_T(b, b))


def probe_factor(vs, vs_full, res):
    dev = vs.device
    g = torch.Generator(device=dev).manual_seed(3)
    b = torch.rand(vs.NX * vs.NY, dtype=torch.float64, device=dev, generator=g) * 2 - 1
    assert vs._edge_thomas and vs.sweep == "cr"
    res["bytes"] = factor_bytes(vs)
    assert vs.capture() or vs._graph is not None
    assert vs.capture_T()
    vs_full.nested_back = "full"
    assert vs_full.capture()
    fwd, tr = solve_fns(vs, b)
    full, _ = solve_fns(vs_full, b)
    med, spread = alternated({"solve": fwd, "solve_T": tr, "solve_full": full})
    res["graph_replay_s"] = med
    res["graph_replay_min_max_s"] = spread
    res["ratio_T_over_solve"] = med["solve_T"] / med["solve"]
    res["ratio_T_over_full"] = med["solve_T"] / med["solve_full"]
    res["TBps"] = {"solve": res["bytes"]["coupled"] / med["solve"] / 1e12,
                   "solve_T": res["bytes"]["transposed"] / med["solve_T"] / 1e12,
                   "solve_full": res["bytes"]["full"] / med["solve_full"] / 1e12}
    # the block GEMV's form: by size (0), wide (1), narrow (2); each with its own captured graph
    B = torch.rand((vs.NX, vs.m), dtype=torch.float64, device=dev, generator=g) * 2 - 1
    rhs = B[0::vs.P].contiguous()

    def cr_with(form):
        def f():
            vs.gemv_t_form = form
            vs._iface_solve_T(rhs)
        return f

    ab, ab_spread = alternated({"by_size": cr_with(0), "wide": cr_with(1), "narrow": cr_with(2)})
    vs.gemv_t_form = 0
    res["cr_solve_T_form_ab_s"] = ab
    res["cr_solve_T_form_ab_min_max_s"] = ab_spread
    res["cr_levels_blocks"] = [int(lev[3].numel()) for lev in vs._cr]
    res["parts_eager_s"] = parts_T(vs, B)


def cd_solver(precond, P, ne, mtol=1e-7):
    from sem_amd.solvers import ConvectionDiffusionSolver
    s = ConvectionDiffusionSolver(1, 1, PE, P, ne, ne, T_W=0.5, T_E=-0.5, mtol=mtol, precond=precond)
    rng = np.random.default_rng(21)
    T, u, v = (rng.uniform(-1, 1, s.N) for _ in range(3))
    s._get_residuals(T, u, v)
    s._calc_jacobians(T)
    return s


def second_cd_factor(s):
    vs = VelocityJacobianSolver(s._P, s._N_ex, s._N_ey, s._mesh.device, ncomp=1)
    cX, cu, cY, cv, d = s._Sys._coeffs()
    vs.factor_mesh(s._mesh, c_mass=s._Sys.cM, c_stiff=s._Sys.cK, c_gradx=cX, cu=cu, c_grady=cY, cv=cv, juu=d,
                   **s._dir.kw())
    return vs


def run_cfg2(res, P=8, ne=64):
    s = cd_solver("condensed", P, ne)
    vs = s._jacobian_solver()
    probe_factor(vs, second_cd_factor(s), res)
    b = np.random.default_rng(23).uniform(-1, 1, s.N)
    adj = {}
    for rep in ("first", "second"):                      # the first call captured nothing new: capture_T ran above
        t0 = time.perf_counter()
        lam = s._get_update_T(b)
        adj[rep] = dict(matvecs=int(s.matvecs), seconds=time.perf_counter() - t0)
    res_T = float(np.linalg.norm(np.asarray(s._get_dresiduals_T(lam)[0]) - b))
    t0 = time.perf_counter()
    s._get_update(b)
    fwd = dict(matvecs=int(s.matvecs), seconds=time.perf_counter() - t0)
    s2 = cd_solver(None, P, ne)
    t0 = time.perf_counter()
    lam2 = s2._get_update_T(b)
    none = dict(matvecs=int(s2.matvecs), seconds=time.perf_counter() - t0)
    res_none = float(np.linalg.norm(np.asarray(s2._get_dresiduals_T(lam2)[0]) - b))
    res["adjoint_cd"] = dict(N=int(s.N), atol=float(s._mtol * np.sqrt(s.N)), preconditioned=adj["second"],
                             preconditioned_first_call=adj["first"], residual_preconditioned=res_T,
                             forward_same_rhs=fwd, unpreconditioned=none, residual_unpreconditioned=res_none)


def run_ns48(res, P=8, ne=48, Re=100.0):
    from sem_amd.solvers import NavierStokesSolver
    ns = NavierStokesSolver(1.0, 1.0, Re, 0.0, P, ne, ne, u_N=1.0, iprint=[], velocity_interior="nested")
    rng = np.random.default_rng(5)
    x, y = (np.asarray(a) for a in ns.points)
    u = 0.3 * (np.sin(np.pi * x) * np.sin(2 * np.pi * y) + 0.01 * rng.uniform(-1, 1, ns.N))
    v = -0.3 * (np.sin(2 * np.pi * x) * np.sin(np.pi * y) + 0.01 * rng.uniform(-1, 1, ns.N))
    ns._get_residuals(u, v, np.zeros(ns.N), np.zeros(ns.N))
    ns._calc_jacobians(u, v)
    kw = dict(juu=ns._Jac_u_u._coeffs()[4], juv=ns._Jac_u_v._coeffs()[4], jvu=ns._Jac_v_u._coeffs()[4],
              jvv=ns._Jac_v_v._coeffs()[4], dir_mask=ns._dir.mask, dir_sides=ns._dir.sides, **ns._sys_kw(ns._Sys))
    pair = []
    for transpose in (True, False):
        vs = VelocityJacobianSolver(P, ne, ne, ns._mesh.device, transpose=transpose)
        vs.factor_mesh(ns._mesh, **kw)
        pair.append(vs)
    probe_factor(pair[0], pair[1], res)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=("cfg2", "ns48", "tiny"), default="cfg2")
    ap.add_argument("--out", default=os.path.join("profiles", "cond_transpose"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cond_transpose_probe: needs the GPU (no CPU timing stands in for it)")
    res = {"tool": "cond_transpose_probe", "case": a.case, "device": torch.cuda.get_device_name(0)}
    if a.case == "cfg2":
        res.update(P=8, nex=64, ney=64, ncomp=1, Pe=PE)
        run_cfg2(res)
    elif a.case == "tiny":                                # a rehearsal size: every path, meaningless times
        res.update(P=4, nex=6, ney=6, ncomp=1, Pe=PE)
        run_cfg2(res, P=4, ne=6)
    else:
        res.update(P=8, nex=48, ney=48, ncomp=2, Re=100.0)
        run_ns48(res)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "cond_transpose_%s.json" % a.case)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
