#!/usr/bin/env python
"""Launch times of the transposed strip apply (sem_apply_transpose_part) on ONE GPU.

Per mesh (default: 1024x1024 P=8 and cfg5's 128x128 P=12; the convection-diffusion operator K + Pe (cu G_x +
cv G_y), Pe = 40, identity Dirichlet rows on W and E; seeded U(-1,1) inputs):
  whole     the whole-mesh transposed launch (sem_apply_transpose) and the forward one (sem_apply)
  strips    each of the G strips of a G-way element-strip partition (default 8) ALONE on this GPU, one handle
            per strip: the transposed launch (sem_apply_transpose_part, all positions) and, beside it, the
            forward strip launch (sem_apply) on the same handle.
Each launch is captured as one graph of `reps` back-to-back applies, replayed once untimed, then timed with
device events; transposed and forward alternate within each trial and the median is reported.  Before timing
the strips' results are assembled on the host side of the exchange (sum over the shared lines) and must equal
the whole-mesh transposed apply to 1e-13, or the tool fails.

This measures the KERNELS a rank launches.  The multi-GPU step itself -- the interface exchange over RCCL and
its overlap with the interior launch -- is NOT measured here.

The driver starts one child process per mesh, each under its own time limit, one after the other, and stops
at the first one that fails; only a child opens the GPU.  Writes one JSON line per mesh to --out (default
profiles/strip_adjoint/strip_probe.jsonl) and prints it.  Needs a GPU: there is no fallback.
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

DEFAULT_SIZES = "1024x1024x8:20,128x128x12:200"
PE = 40.0


def parse_sizes(text):
    out = []
    for item in text.split(","):
        dims, _, reps = item.partition(":")
        nex, ney, P = (int(v) for v in dims.split("x"))
        out.append((nex, ney, P, int(reps or 200)))
    return out


def timed_pair(torch, no_gc, dev, launches, reps, trials):
    """{name: [us per apply, ...]} of graph-captured back-to-back launches, alternated within each trial."""
    graphs = {}
    side = torch.cuda.Stream(dev)
    for name, f in launches.items():
        f()
        g = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), no_gc(), torch.cuda.graph(g, stream=side):
            for _ in range(reps):
                f()
        torch.cuda.current_stream(dev).wait_stream(side)
        g.replay()   # untimed
        graphs[name] = g
    torch.cuda.synchronize(dev)
    times = {name: [] for name in launches}
    for _ in range(trials):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    return times


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
    z, cu, cv = (torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * 2 - 1 for _ in range(3))
    dkw = dict(c_stiff=1.0, c_gradx=PE, c_grady=PE, dir_mode=_lib.DIR_IDENTITY, dir_sides=_lib.SIDE_W | _lib.SIDE_E)
    want = full.apply_transpose(z, cu=cu, cv=cv, **dkw)
    y = torch.empty_like(z)
    t = timed_pair(torch, no_gc, dev, {"transposed": lambda: full.apply_transpose(z, y, cu=cu, cv=cv, **dkw),
                                       "forward": lambda: full.apply(z, y, cu=cu, cv=cv, **dkw)}, reps, trials)
    out = {"mesh": f"{nex}x{ney}", "P": P, "N": n, "G": G, "reps": reps, "trials": trials,
           "device": torch.cuda.get_device_name(0), "kernel_transposed": full.transpose_kernel_name(),
           "whole": {"us_transposed": statistics.median(t["transposed"]), "us_forward": statistics.median(t["forward"]),
                     "us_all": t}, "strips": []}
    part = StripPartition(nex, G)
    total = torch.zeros_like(z)
    for r in range(G):
        eb, ee = part.local_range(r)
        m = get_mesh(P, nex, ney, dx, dy, eb, ee)
        sl = slice(m.dof_begin, m.dof_begin + m.n_local)
        zs, us, vs = (v[sl].contiguous() for v in (z, cu, cv))
        ys = torch.empty_like(zs)
        total[sl] += m.apply_transpose_part(zs, cu=us, cv=vs, **dkw)   # the exchange's sum over shared lines
        t = timed_pair(torch, no_gc, dev, {"transposed": lambda: m.apply_transpose_part(zs, ys, cu=us, cv=vs, **dkw),
                                           "forward": lambda: m.apply(zs, ys, cu=us, cv=vs, **dkw)}, reps, trials)
        out["strips"].append({"rank": r, "columns": [eb, ee], "n_local": m.n_local,
                              "us_transposed": statistics.median(t["transposed"]),
                              "us_forward": statistics.median(t["forward"]), "us_all": t})
    scale = want.abs().max().item()
    diff = (total - want).abs().max().item()
    out["rel_diff_assembled_vs_whole"] = diff / scale
    if not diff <= 1e-13 * scale:
        raise SystemExit(f"{nex}x{ney} P={P}: assembled strips differ from the whole-mesh transposed apply: "
                         f"{diff:.3e} of {scale:.3e}")
    out["us_strip_transposed_max"] = max(s["us_transposed"] for s in out["strips"])
    out["us_strip_forward_max"] = max(s["us_forward"] for s in out["strips"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default=DEFAULT_SIZES, help="comma list of NEXxNEYxP[:reps] (default %(default)s)")
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--parts", type=int, default=8, help="strips of the partition (default %(default)s)")
    ap.add_argument("--limit", type=int, default=240, help="time limit of one mesh's child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strip_adjoint", "strip_probe.jsonl"))
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
            print(f"strip_adjoint_probe: {item} ended with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
