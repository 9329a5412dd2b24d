#!/usr/bin/env python
"""Timing of the fused transposed apply (sem_apply_transpose) against the forward apply and against
the composition of A^T z from forward launches -- the only device route without the fused kernel.

In ONE process, per mesh (default: 64x64 P=8, 128x128 P=12, 1024x1024 P=8; the convection-diffusion
operator K + Pe (cu G_x + cv G_y), Pe = 40, identity Dirichlet rows on W and E; seeded U(-1,1) inputs):
  (a) forward      y = A_D z              one sem_apply launch
  (b) transposed   y = A_D^T z            one sem_apply_transpose launch
  (c) composed     y = A_D^T z            three sem_apply launches + torch pointwise products:
                   z' = (1-m) z;  y = K z';  y -= Pe G_x (cu z');  y -= Pe G_y (cv z');
                   y += Pe (b_x cu z' + b_y cv z') + m z     (G^T = -G + boundary term)
Each is captured as one graph of `reps` back-to-back applies (1000, 20 on the largest mesh), replayed
once untimed, then timed with device events; the three are alternated within each of 5 trials and
the median is reported.  (b) and (c) must agree to 1e-13 on the timed inputs or the tool fails.
Prints one JSON line and writes it to profiles/adjoint/bench.json.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT_SIZES = "64x64x8:1000,128x128x12:1000,1024x1024x8:20"
PE = 40.0


def parse_sizes(text):
    out = []
    for item in text.split(","):
        dims, _, reps = item.partition(":")
        nex, ney, P = (int(v) for v in dims.split("x"))
        out.append((nex, ney, P, int(reps or 1000)))
    return out


def run_size(nex, ney, P, reps, trials):
    import torch

    from sem_amd import _lib
    from sem_amd.device import get_mesh, no_gc
    mesh = get_mesh(P, nex, ney, 1.0 / nex, 1.0 / ney)
    dev, n, NX, NY = mesh.device, mesh.n_local, mesh.NX, mesh.NY
    gen = torch.Generator(device=dev)
    gen.manual_seed(2024 + P + nex)
    z, cu, cv = (torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * 2 - 1 for _ in range(3))
    sides = _lib.SIDE_W | _lib.SIDE_E
    kw = dict(c_stiff=1.0, c_gradx=PE, cu=cu, c_grady=PE, cv=cv, dir_mode=_lib.DIR_IDENTITY, dir_sides=sides)

    # the composition's constant vectors: 1 - m, m, and Pe times the boundary terms of G_x^T, G_y^T
    mx, my = (torch.as_tensor(w, device=dev) for w in mesh.weights_1d())
    m = torch.zeros(NX, NY, dtype=torch.float64, device=dev)
    m[0, :] = 1.0
    m[-1, :] = 1.0
    bx = torch.zeros(NX, NY, dtype=torch.float64, device=dev)
    bx[0, :] = -PE * (mesh.dy / 2) * my
    bx[-1, :] = PE * (mesh.dy / 2) * my
    by = torch.zeros(NX, NY, dtype=torch.float64, device=dev)
    by[:, 0] = -PE * (mesh.dx / 2) * mx
    by[:, -1] = PE * (mesh.dx / 2) * mx
    m, bx, by = m.reshape(-1), bx.reshape(-1), by.reshape(-1)
    free = 1.0 - m
    ya, yb, yc, zp, w1, w2 = (torch.empty_like(z) for _ in range(6))

    def forward():
        mesh.apply(z, ya, **kw)

    def fused():
        mesh.apply_transpose(z, yb, **kw)

    def composed():
        torch.mul(free, z, out=zp)
        torch.mul(cu, zp, out=w1)
        torch.mul(cv, zp, out=w2)
        mesh.apply(zp, yc, c_stiff=1.0)
        mesh.apply(w1, yc, c_gradx=-PE, c_acc=1.0)
        mesh.apply(w2, yc, c_grady=-PE, c_acc=1.0)
        yc.addcmul_(bx, w1).addcmul_(by, w2).addcmul_(m, z)

    steps = {"forward": forward, "transposed": fused, "composed": composed}
    for f in steps.values():   # warm up (module load, allocator)
        f()
    torch.cuda.synchronize(dev)
    scale = yc.abs().max().item()
    diff = (yb - yc).abs().max().item()
    if not diff <= 1e-13 * scale:
        raise SystemExit(f"{nex}x{ney} P={P}: fused and composed transposed applies differ: "
                         f"max|b - c| = {diff:.3e}, max|c| = {scale:.3e}")
    graphs = {}
    side = torch.cuda.Stream(dev)
    for name, f in steps.items():
        g = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), no_gc(), torch.cuda.graph(g, stream=side):
            for _ in range(reps):
                f()
        torch.cuda.current_stream(dev).wait_stream(side)
        g.replay()   # untimed
        graphs[name] = g
    torch.cuda.synchronize(dev)
    times = {name: [] for name in steps}
    for _ in range(trials):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / reps)   # us per apply
    med = {name: statistics.median(t) for name, t in times.items()}
    return {
        "mesh": f"{nex}x{ney}", "P": P, "N": n, "reps": reps, "trials": trials,
        "kernel_forward": mesh.kernel_name(), "kernel_transposed": mesh.transpose_kernel_name(),
        "us_forward": med["forward"], "us_transposed": med["transposed"], "us_composed": med["composed"],
        "us_all": times,
        "transposed_over_forward": med["transposed"] / med["forward"],
        "composed_over_transposed": med["composed"] / med["transposed"],
        "GBps_transposed": 32.0 * n / (med["transposed"] * 1e-6) / 1e9,
        "GBps_forward": 32.0 * n / (med["forward"] * 1e-6) / 1e9,
        "rel_diff_fused_vs_composed": diff / scale,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default=DEFAULT_SIZES, help="comma list of NEXxNEYxP[:reps] (default %(default)s)")
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adjoint", "bench.json"))
    args = ap.parse_args()
    from sem_amd.device import require_gpu
    require_gpu()
    import torch
    result = {"tool": "adjoint_bench", "device": torch.cuda.get_device_name(0), "Pe": PE,
              "sizes": [run_size(*s, args.trials) for s in parse_sizes(args.sizes)]}
    result["transposed_beats_composed"] = all(s["us_transposed"] < s["us_composed"] for s in result["sizes"])
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0 if result["transposed_beats_composed"] else 1


if __name__ == "__main__":
    sys.exit(main())
