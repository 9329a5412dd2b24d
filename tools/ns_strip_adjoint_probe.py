#!/usr/bin/env python
"""Launch times of the transposed Navier-Stokes strip apply (sem_ns_apply_transpose_part) on ONE GPU.

Per mesh (default: 1024x1024 P=8 and cfg5's 128x128 P=12; the solvers' descriptors -- K + 1e3 (cu G_x + cv G_y) with
the four j** diagonals, the whole perimeter Dirichlet, the pin at N / 2; seeded U(-1,1) inputs), each of the G strips
of a G-way element-strip partition (default 8) ALONE on this GPU, one handle per strip, in the four forms the kernel
specialises, each beside the forward sem_ns_apply launch of the same shape on the same handle:
  gradient_T       zc -> yu, yv            (forward: p -> ru, rv)
  divergence_T     zu, zv, zc -> yp        (forward: u, v, p -> rc)
  velocity_rows_T  zu, zv -> yu, yv        (forward: u, v -> ru, rv)
  dresidual_T      zu, zv, zc -> yu, yv, yp    (forward: u, v, p -> ru, rv, rc)
Each launch is captured as one graph of `reps` back-to-back launches, replayed once untimed, then timed with device
events; the eight launches alternate within each trial and the median is reported.  Before timing the strips'
dresidual_T results are assembled on the host side of the exchange (sum over the shared lines) and must equal the
whole-mesh sem_ns_apply_transpose to 1e-13, or the tool fails.

This measures the KERNELS a rank launches.  The multi-GPU step itself -- the interface exchange over RCCL -- is NOT
measured here.

The driver starts one child process per mesh, each under its own time limit, one after the other, and stops at the
first one that fails; only a child opens the GPU.  Writes one JSON line per mesh to --out (default
profiles/ns_strip_adjoint/strip_probe.jsonl) and prints it.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from strip_adjoint_probe import parse_sizes, timed_pair  # noqa: E402

DEFAULT_SIZES = "1024x1024x8:20,128x128x12:200"
FORMS = ("gradient", "divergence", "velocity_rows", "dresidual")


def run_size(nex, ney, P, reps, trials, G):
    import torch

    from sem_amd import _lib
    from sem_amd.device import get_mesh, no_gc
    from sem_amd.parallel import StripPartition
    dx, dy = 1.0 / nex, 1.0 / ney
    full = get_mesh(P, nex, ney, dx, dy)
    dev, n = full.device, full.n_local
    gen = torch.Generator(device=dev)
    gen.manual_seed(2024 + P + nex)
    names = ("zu", "zv", "zc", "cu", "cv", "juu", "juv", "jvu", "jvv")
    f = {k: torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * 2 - 1 for k in names}
    rows = dict(dir_sides=_lib.SIDE_W | _lib.SIDE_E | _lib.SIDE_S | _lib.SIDE_N, pin=n // 2)
    coef = ("cu", "cv", "juu", "juv", "jvu", "jvv")
    want = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3)]
    full.ns_apply_transpose(f["zu"], f["zv"], f["zc"], *want, c_stiff=1.0, c_gradx=1e3, c_grady=1e3,
                            **{k: f[k] for k in coef}, **rows)
    out = {"mesh": f"{nex}x{ney}", "P": P, "N": n, "G": G, "reps": reps, "trials": trials,
           "device": torch.cuda.get_device_name(0), "strips": []}
    part = StripPartition(nex, G)
    total = [torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(3)]
    for r in range(G):
        eb, ee = part.local_range(r)
        m = get_mesh(P, nex, ney, dx, dy, eb, ee)
        sl = slice(m.dof_begin, m.dof_begin + m.n_local)
        s = {k: v[sl].contiguous() for k, v in f.items()}
        sysk = dict(c_stiff=1.0, c_gradx=1e3, c_grady=1e3, **{k: s[k] for k in coef})
        zu, zv, zc = s["zu"], s["zv"], s["zc"]
        ya, yb, yc = (torch.empty_like(zu) for _ in range(3))
        m.ns_apply_transpose_part(zu, zv, zc, ya, yb, yc, **sysk, **rows)
        for t, y in zip(total, (ya, yb, yc)):
            t[sl] += y                            # the exchange's sum over shared lines
        T, F = m.ns_apply_transpose_part, m.ns_apply
        launches = {
            "gradient_T": lambda: T(None, None, zc, ya, yb, c_div=-1.0, **rows),
            "gradient": lambda: F(None, None, zc, ya, yb, **rows),
            "divergence_T": lambda: T(zu, zv, zc, yp=yc, **rows),
            "divergence": lambda: F(zu, zv, zc, rc=yc, c_div=-1.0, **rows),
            "velocity_rows_T": lambda: T(zu, zv, None, ya, yb, **sysk, **rows),
            "velocity_rows": lambda: F(zu, zv, None, ya, yb, **sysk, **rows),
            "dresidual_T": lambda: T(zu, zv, zc, ya, yb, yc, **sysk, **rows),
            "dresidual": lambda: F(zu, zv, zc, ya, yb, yc, **sysk, **rows),
        }
        t = timed_pair(torch, no_gc, dev, launches, reps, trials)
        rec = {"rank": r, "columns": [eb, ee], "n_local": m.n_local, "us": {k: statistics.median(v) for k, v in t.items()},
               "us_all": t}
        rec["ratio_T_over_forward"] = {k: rec["us"][k + "_T"] / rec["us"][k] for k in FORMS}
        out["strips"].append(rec)
    worst = 0.0
    for t, w in zip(total, want):
        scale = w.abs().max().item()
        diff = (t - w).abs().max().item()
        worst = max(worst, diff / scale)
        if not diff <= 1e-13 * scale:
            raise SystemExit(f"{nex}x{ney} P={P}: assembled strips differ from the whole-mesh transposed apply: "
                             f"{diff:.3e} of {scale:.3e}")
    out["rel_diff_assembled_vs_whole"] = worst
    out["us_strip_max"] = {k: max(s["us"][k] for s in out["strips"]) for k in out["strips"][0]["us"]}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default=DEFAULT_SIZES, help="comma list of NEXxNEYxP[:reps] (default %(default)s)")
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--parts", type=int, default=8, help="strips of the partition (default %(default)s)")
    ap.add_argument("--limit", type=int, default=240, help="time limit of one mesh's child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ns_strip_adjoint", "strip_probe.jsonl"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        from sem_amd.device import require_gpu
        require_gpu()
        (size,) = parse_sizes(args.child)
        print(json.dumps(run_size(*size, args.trials, args.parts)))
        return 0
    lines = []
    for item in args.sizes.split(","):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", item,
               "--trials", str(args.trials), "--parts", str(args.parts)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:   # a failed or hung step ends the probe: nothing more is started on the GPU
            sys.stderr.write(r.stdout + r.stderr)
            print(f"ns_strip_adjoint_probe: {item} ended with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
