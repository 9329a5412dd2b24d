"""Benchmark: DOF-updates/s of the SEM Laplacian+convection matvec on MI355X.

One step = one application of the convection-diffusion system operator with
Dirichlet identity rows -- the LGMRES matvec of ConvectionDiffusion_Solver
(`_get_dresiduals`, ConvectionDiffusion_Solver.py:104-121):

    y = K T + Pe (u . G_x T + v . G_y T),   y[W/E boundary rows] = T

on a synthetic 64 x 64-element, P = 8 mesh per GPU (BASELINE.json configs[1];
Pe = 40, T, u, v ~ U(-1, 1) from default_rng(2024)).  N = 263,169 DOFs per
GPU; inputs resident in HBM before the timed region.  With --gpus N > 1 each
rank holds one element-column strip and every step assembles the interface lines
(RCCL all-reduce of the shared-edge partial sums, or --exchange p2p: send/recv
with the two neighbours), overlapped with the interior apply (--overlap 1: the
strip's two interface positions are applied first, the exchange is started, the
interior positions are applied while it runs).
  --scaling strong (default) the --ne x --ne mesh (64 x 64: BASELINE configs[1]) split into N strips -- north_star's
                   "Ne x Ne, P=8 mesh at 1, 2, 4 and 8 GPUs" and BASELINE.md's strong-scaling plan; at N > 1 the
                   line also carries `strong_hbm` (the 1024 x 1024 mesh split into N strips: the HBM regime) and
                   `weak` (a 64-element-column strip per rank of a (64 N) x 64 mesh)
  --scaling weak   the weak-scaling mesh as the headline instead

A plain run sets up, warms up, times the --steps steps and prints the result line: the headline
(`value`, `ms_per_step`) and what follows from it without another run.  --full adds everything that takes
runs of its own: the 1000-launch graph timing, `laplacian_only`, `mfma_variant`, `roofline_hbm`, the other
meshes (`strong_hbm`, `weak`, `weak_hbm`), `velocity_solve`, `cpu_baseline` and, at N > 1, the roofline of the
apply alone.  --dump-outputs DIR writes the y of the last timed step as DIR/y.npy (float64; N > 1:
DIR/y_rank<r>.npy), so that two builds can be compared output for output: the inputs are seeded.

Run:  python bench.py [--gpus N --steps K --warmup W] [--full] [--dump-outputs DIR]
      torchrun --nproc-per-node N bench.py --gpus N ...
Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BASELINE_METRIC = "DOF-updates/sec, SEM Laplacian matvec, P=8, at 1/2/4/8 MI355X"   # BASELINE.json "metric"
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E peak (MI355X_MICROARCH.md, chip table)
FP64_PEAK_TFLOPS = 78.6        # MI355X FP64 vector / matrix dense peak (datasheet)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--ne", type=int, default=64, help="elements per direction per GPU")
    ap.add_argument("--P", type=int, default=8)
    ap.add_argument("--Pe", type=float, default=40.0)
    ap.add_argument("--graph", type=int, default=1,
                    help="capture steps in hipGraphs (N=1, and N>1 over RCCL: apply + pack + all-reduce + unpack)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="CPU baseline budget (0 = skip)")
    ap.add_argument("--hbm-ne", type=int, default=1024, help="HBM-regime mesh size (0 = skip)")
    ap.add_argument("--weak-ne", type=int, default=512,
                    help="HBM-regime weak scaling: (weak_ne N) x weak_ne elements over N GPUs, SURVEY 8(d) (0 = skip)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl (= RCCL, the measured path); gloo only to rehearse N > 1 on a 1-GPU box")
    ap.add_argument("--scaling", default="strong", choices=["weak", "strong"],
                    help="strong: --ne x --ne elements over all GPUs; weak: --ne x --ne elements per GPU")
    ap.add_argument("--extra-steps", type=int, default=100,
                    help="N > 1: steps timed for the strong_hbm and weak extra keys (0 = skip them)")
    ap.add_argument("--overlap", type=int, default=-1,
                    help="N > 1: overlap the interface exchange with the interior apply (1), or not (0); -1 (default): "
                         "overlap only strips of >= 2^20 local DOFs -- the overlapped step's two extra position-ranged "
                         "launches and cross-stream waits cost ~6 us per step (measured over a one-rank RCCL group, "
                         "profiles/r06/rccl/), more than a small strip's interior apply it could hide")
    ap.add_argument("--vsolve-ne", type=int, default=128,
                    help="N = 1: also time the NS velocity solve (nested dissection) on this mesh at --vsolve-P "
                         "(BASELINE cfg5: 128, P = 12; 0 = skip)")
    ap.add_argument("--vsolve-P", type=int, default=12)
    ap.add_argument("--exchange", default="allreduce", choices=["allreduce", "p2p"],
                    help="interface assembly for N > 1: one RCCL all-reduce, or send/recv with the two neighbours")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline (1000-launch graph timing, Laplacian-only and "
                         "MFMA variants, HBM-regime and other meshes, velocity solve, CPU baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the output of the last one as DIR/y.npy (N > 1: y_rank<r>.npy)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_LIMIT_BYTES = 64 << 20   # --dump-outputs: all ranks' files together


def dump_outputs(path, y, world, rank):
    """The timed path's output (y of the last timed step, as a caller of mesh.apply / StripApply receives it)
    as float64 .npy.  An output beyond this rank's share of DUMP_LIMIT_BYTES is sampled at fixed, seeded
    positions (the same ones for every run of the same size)."""
    os.makedirs(path, exist_ok=True)
    a = y.detach().cpu().numpy().astype(np.float64, copy=False)
    cap = DUMP_LIMIT_BYTES // world // 8 - 16   # entries; 128 bytes left for the .npy header
    if a.size > cap:
        a = a[np.sort(np.random.default_rng(977).choice(a.size, size=cap, replace=False))]
    np.save(os.path.join(path, "y.npy" if world == 1 else f"y_rank{rank}.npy"), a)


def algorithmic(P, nex, ney):
    n = P + 1
    N = (nex * P + 1) * (ney * P + 1)
    return N, 32.0 * N, 8.0 * n ** 3 * nex * ney   # DOFs, bytes (T,u,v read + y write), flops


def make_inputs(mesh, seed=2024):
    r = np.random.default_rng(seed)
    N = mesh.n_local
    return [mesh.to_device(r.uniform(-1, 1, N)) for _ in range(3)]


GRAPH_BATCH = 100   # steps per captured hipGraph


def capture(step, count, dev):
    """One hipGraph holding `count` back-to-back steps (captured on a side stream)."""
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        # thread-local capture mode: the process group's watchdog thread keeps querying its
        # events while this thread captures; global mode would invalidate the capture
        pg = torch.distributed.is_available() and torch.distributed.is_initialized()
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local" if pg else "global"):
            for _ in range(count):
                step()
    torch.cuda.current_stream(dev).wait_stream(s)
    return g


def time_steps(step, steps, warmup, dev, use_graph, dist=None):
    """Time exactly `steps` steps between barrier + synchronize on both sides.

    With graphs, all steps are captured up front: one graph of min(steps, 100) steps replayed
    steps // 100 times, plus one graph for the remainder, so a short run (the driver's
    --steps 20) is ONE graph replay of 20 back-to-back applies, not 20 single-launch replays.
    Every graph is replayed once untimed before the timed region."""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    plan = []
    if use_graph and steps > 0:
        batch = min(steps, GRAPH_BATCH)
        reps, rem = divmod(steps, batch)
        try:
            plan.append((capture(step, batch, dev), reps))
            if rem:
                plan.append((capture(step, rem, dev), 1))
        except RuntimeError as exc:   # capture refused (a collective the library cannot capture): eager steps
            if dist is None:
                raise
            print(f"[bench] hipGraph capture failed ({exc}); timing eagerly", file=sys.stderr, flush=True)
            plan = []
        if dist is not None:
            # a capture executes no collective, so a rank whose capture failed would otherwise run a different
            # number of collectives than the others: every rank replays only if every rank captured
            ok = torch.tensor([1.0 if plan else 0.0], device=dev)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if ok.item() < 1.0:
                plan = []
        for g, _ in plan:
            g.replay()
        torch.cuda.synchronize(dev)
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    if plan:
        for g, reps in plan:
            for _ in range(reps):
                g.replay()
    else:
        for _ in range(steps):
            step()
    e1.record()
    torch.cuda.synchronize(dev)
    wall = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
    return e0.elapsed_time(e1) / 1e3, bool(plan)


def graph_kernel_us(fn, dev, launches=1000, trials=5):
    """Per-launch device time of `fn` from `launches` back-to-back launches captured in ONE graph,
    HIP events on the launch stream; median of `trials` replays.  Graph-launch overhead is
    amortised over 1000 launches, so this is the kernel's average duration (plus the in-graph
    dispatch gap), the number a rocprofv3 kernel trace of the same launches averages to."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize(dev)
    g = capture(fn, launches, dev)
    g.replay()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(trials):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize(dev)
        ts.append(a.elapsed_time(b) * 1e3 / launches)
    del g
    return float(np.median(ts))


def build_strip_step(P, nex, ney, d, Pe, parts, rank, dev, dist, exchange="allreduce", overlap=True, seed=2024):
    """This rank's strip (element columns of StripPartition(nex, parts)) and its bench step: the fused apply of the
    CD system operator plus, with parts > 1, the interface assembly (StripApply: the interface positions first, the
    RCCL all-reduce or send/recv started, the interior applied while it runs).  Returns (step, mesh, (T, y, kw),
    (eb, ee)).  tests/test_gpu_rccl.py drives this with a real one-rank RCCL group and parts = 2."""
    from sem_amd import _lib
    from sem_amd.device import get_mesh
    from sem_amd.parallel import StripApply, StripPartition
    part = StripPartition(nex, parts)
    eb, ee = part.bounds[rank], part.bounds[rank + 1]
    mesh = get_mesh(P, nex, ney, d, d, eb, ee, dev.index)
    T, u, v = make_inputs(mesh, seed=seed)
    y = torch.empty_like(T)
    kw = dict(c_stiff=1.0, c_gradx=Pe, cu=u, c_grady=Pe, cv=v, dir_mode=_lib.DIR_IDENTITY,
              dir_sides=_lib.SIDE_W | _lib.SIDE_E)
    strip = StripApply(part, mesh, dist, kind=exchange, overlap=overlap) if parts > 1 else None

    def step():
        if strip is None:
            mesh.apply(T, y, **kw)
        else:
            strip(T, y, **kw)
    return step, mesh, (T, y, kw), (eb, ee)


def cpu_baseline(P, ne, Pe, seconds):
    """Oracle (CPU restatement of the reference path): SciPy CSR `Sys @ T` + Dirichlet rows,
    single core, cfg2.  Sys assembled once as the reference does (SEM.py:186-223)."""
    from oracle import sem_oracle as O
    d = 1.0 / ne
    K = O.global_stiffness_matrix(P, ne, ne, d, d)
    Gx, Gy = O.global_gradient_matrices(P, ne, ne, d, d)
    N = K.shape[0]
    r = np.random.default_rng(2024)
    T, u, v = r.uniform(-1, 1, N), r.uniform(-1, 1, N), r.uniform(-1, 1, N)
    Sys = (Pe * (O.conv_left(Gx, u) + O.conv_left(Gy, v)) + K).tocsr()
    NY = ne * P + 1
    mask = np.zeros(N, dtype=bool)
    mask[:NY] = True
    mask[-NY:] = True
    try:
        aff = os.sched_getaffinity(0)
        os.sched_setaffinity(0, {min(aff)})
    except (AttributeError, OSError):
        aff = None
    try:  # one thread (SciPy's CSR SpMV is single-threaded; this pins any BLAS pool too)
        from threadpoolctl import threadpool_limits
        limiter = threadpool_limits(1)
    except ImportError:
        limiter = None
    # median of 50 reps (after 3 warm-up reps), inside the time budget
    for _ in range(3):
        y = Sys @ T
    ts, t_start = [], time.perf_counter()
    while len(ts) < 50 and time.perf_counter() - t_start < seconds:
        t0 = time.perf_counter()
        y = Sys @ T
        y[mask] = T[mask]
        ts.append(time.perf_counter() - t0)
    if limiter is not None:
        limiter.unregister()
    if aff is not None:
        os.sched_setaffinity(0, aff)
    med = float(np.median(ts))
    return {"value": N / med, "unit": "DOF-updates/s", "cores": 1, "kind": "port",
            "sample": f"cfg2 64x64 P=8 (N={N}): median of {len(ts)} reps of (SciPy CSR Sys@T + Dirichlet "
                      f"rows) = {med * 1e3:.3f} ms, 1 thread pinned to 1 core of {os.cpu_count()} host threads "
                      f"(oracle/sem_oracle.py restatement of ConvectionDiffusion_Solver.py:85-87,112-119)"}


def velocity_solve_line(ne, P, dev, solves=20):
    """The inner solve of every NS Schur-complement matvec (NavierStokes_Solver.py:189-203): the velocity Jacobian of a
    smooth linearisation (Re = 1e3, Ra = 1e6, cfg5's mesh by default) factored by nested dissection
    (solvers/nested_dissection.py), then `solves` graph-replayed solves timed with HIP events; bytes = the operators
    one solve streams (bytes_per_solve)."""
    import time
    import numpy as np
    from sem_amd.solvers import NavierStokesSolver
    ns = NavierStokesSolver(1.0, 1.0, 1e3, 1e6 / 0.71, P, ne, ne, mtol=1e-10, mtol_newton=1e-10, iprint=[])
    x, y = ns.points
    u0 = 1e-2 * np.sin(np.pi * x) * np.sin(2 * np.pi * y)
    v0 = -1e-2 * np.sin(2 * np.pi * x) * np.sin(np.pi * y)
    ns._get_residuals(u0, v0, np.zeros(ns.N), 0.5 - x)
    ns._calc_jacobians(u0, v0)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    vs = ns._velocity_solver()
    torch.cuda.synchronize(dev)
    factor_s = time.perf_counter() - t0
    r = np.random.default_rng(5)
    bu, bv = (ns._dev(r.uniform(-1, 1, ns.N)) for _ in range(2))
    for _ in range(3):
        vs.solve(bu, bv)
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(solves):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        vs.solve(bu, bv)
        b.record()
        torch.cuda.synchronize(dev)
        ts.append(a.elapsed_time(b) * 1e-3)
    t = float(np.median(ts))
    nbytes = vs.bytes_per_solve() if vs.interior == "nd" else None
    return {"workload": f"ns_velocity_solve_{ne}x{ne}_P{P}", "factorisation": vs.interior, "unknowns": 2 * ns.N,
            "ms_per_solve": t * 1e3, "factor_s": factor_s, "backward_error": vs.refine_eta,
            "graph": getattr(vs, "_graph", None) is not None, "bytes_per_solve": nbytes,
            "achieved_GBs": nbytes / t / 1e9 if nbytes else None,
            "frac_hbm": nbytes / t / 1e9 / HBM_PEAK_GBS if nbytes else None}


def load_pmc(workload, kernel):
    """HBM traffic per launch measured with rocprofv3 PMC passes (profiles/pmc_traffic.json, written by
    tools/pmc_traffic.py), and the exact kernel instantiation it was measured on; only an entry measured
    on the kernel family this run launches (kernel_name() plus its template flags) is used."""
    p = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        with open(p) as f:
            e = json.load(f).get("workloads", {}).get(workload, {})
    except (OSError, ValueError):
        return None, None
    k = e.get("kernel", "")
    # kernel_name() spells the coefficient mode as a suffix (", dpp" = CM 1, ", smem" = CM 2, none = CM 0); the
    # PMC entry records the full instantiation <P, TXE, TYE, NS, FULL, CM, GRAD>: the families must match
    cm, fam = "0", kernel[:-1] if kernel.endswith(">") else kernel
    for suffix, mode in ((", dpp", "1"), (", smem", "2")):
        if fam.endswith(suffix):
            cm, fam = mode, fam[:-len(suffix)]
    rest = k[len(fam) + 1:].rstrip(">").split(",") if k.startswith(fam + ",") else []
    if not (k == kernel or (len(rest) >= 2 and rest[1].strip() == cm)):
        return None, None
    return e.get("hbm_bytes_per_launch"), k


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        local = local % max(1, torch.cuda.device_count())   # rehearsal: several ranks may share one GPU
        torch.cuda.set_device(local)
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo")
    dev = torch.device("cuda", local if world > 1 else 0)
    torch.cuda.set_device(dev)

    from sem_amd import _lib
    from sem_amd.device import get_mesh
    from sem_amd.parallel import StripPartition

    P, ne, Pe = args.P, args.ne, args.Pe

    def strip_case(nex, ney, d, steps, warmup, seed):
        """Build this rank's strip of an nex x ney mesh and time `steps` partitioned applies (apply + interface
        exchange).  Returns (seconds max-reduced over ranks, graph used, mesh, operands)."""
        part_cols = StripPartition(nex, world).bounds
        local = (part_cols[rank + 1] - part_cols[rank]) * P * (ney * P + 1)
        overlap = bool(args.overlap) if args.overlap >= 0 else local >= (1 << 20)
        step, mesh, (T, y, kw), (eb, ee) = build_strip_step(P, nex, ney, d, Pe, world, rank, dev, dist,
                                                            args.exchange, overlap, seed)

        # N > 1 over RCCL: the whole step (apply, pack, RCCL all-reduce or send/recv, unpack) is captured
        # too -- RCCL collectives are stream-capturable -- so the per-step host cost (four launches and a
        # collective call from Python) leaves the timed loop; gloo collectives are host-side and cannot be.
        use_graph = bool(args.graph) and (world == 1 or args.dist_backend == "nccl")
        # a refused capture (every rank agrees first) times the same steps eagerly
        secs, use_graph = time_steps(step, steps, warmup, dev, use_graph=use_graph, dist=dist)
        if dist is not None:
            t = torch.tensor([secs], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            secs = float(t.item())
        return secs, use_graph, mesh, (T, y, kw), (eb, ee)

    nex, ney = (ne * world, ne) if args.scaling == "weak" else (ne, ne)
    d = 1.0 / ne
    secs, use_graph, mesh, (T, y, kw), (eb, ee) = strip_case(nex, ney, d, args.steps, args.warmup, 2024 + rank)
    N_glob = (nex * P + 1) * (ney * P + 1)
    value = N_glob * args.steps / secs
    ms = secs / args.steps * 1e3
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, y, world, rank)

    # roofline of the dominant kernel (the fused apply) on this rank
    n_loc = mesh.n_local
    bytes_launch, flops_launch = 32.0 * n_loc, 8.0 * (P + 1) ** 3 * (ee - eb) * ney
    apply_only = (lambda: mesh.apply(T, y, **kw))
    # the kernel's average launch duration, measured live: the timed region (HIP events on the launch
    # stream) / launches at N = 1; at N > 1 the step also holds the exchange, so the apply alone is
    # timed the same way (all launches of one graph; a run of its own: --full).  graph1000_us (--full):
    # 1000 back-to-back launches in one graph, where the graph-launch cost is fully amortised.
    if world == 1:
        kern_s = secs / args.steps
    elif args.full:
        k_secs, _ = time_steps(apply_only, args.steps, args.warmup, dev, use_graph=True)
        kern_s = k_secs / args.steps
    else:
        kern_s = None
    workload = f"cd_matvec_{nex}x{ney}_P{P}"

    def regime(n_rank, latency=False):
        mb = 32.0 * n_rank / 1e6
        r = (f"HBM ({mb:.0f} MB moved per apply per GPU, beyond the 256 MB MALL)" if mb > 256 else
             f"L2/MALL-resident ({mb:.1f} MB working set per GPU)")
        if latency:
            r += ("; latency-bound: the per-rank apply (a few us) is shorter than the interface exchange "
                  "(small-message collective latency), so strong scaling of this mesh cannot be linear")
        return r
    out = {
        "metric": BASELINE_METRIC,
        "work": "y = K T + Pe (u.Gx T + v.Gy T), Dirichlet identity rows on x=0,1: the Laplacian+convection "
                "matvec north_star targets (ConvectionDiffusion_Solver.py:104-121); the Laplacian-only K T "
                "is reported under laplacian_only (--full)",
        "value": value, "unit": "DOF-updates/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "f64",
        "data": "synthetic (T,u,v ~ U(-1,1), default_rng(2024+rank); Pe=40; Dirichlet W/E rows)",
        "config": {"workload": workload,
                   "mesh_per_gpu": f"{ee - eb}x{ney} elements" + (" (rank 0)" if args.scaling == "strong" else ""),
                   "P": P,
                   "global_mesh": f"{nex}x{ney}", "dofs_global": N_glob, "dofs_per_gpu": n_loc,
                   "partition": f"element-column strips x{world}" + (
                       {"allreduce": ", all-reduce of interface lines",
                        "p2p": ", send/recv of interface lines with neighbours"}[args.exchange]
                       + (", overlapped with the interior apply" if (args.overlap > 0 or (args.overlap < 0 and n_loc >= (1 << 20)))
                          else "")
                       + (" (RCCL)" if args.dist_backend == "nccl" else " (gloo rehearsal)")
                       if world > 1 else ""),
                   "regime": regime(n_loc, latency=world > 1 and 32.0 * n_loc < 256e6), "hipgraph": use_graph},
    }
    if kern_s is not None:
        achieved = bytes_launch / kern_s / 1e9
        # PMC traffic was measured on the whole-mesh kernel: a strip launch is another workload
        traffic, traffic_kernel = load_pmc(workload, mesh.kernel_name()) if world == 1 else (None, None)
        out["roofline"] = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_kernel": traffic_kernel,
                           "kernel": mesh.kernel_name(), "bytes_per_launch": bytes_launch,
                           "flops_per_launch": flops_launch, "kernel_us": kern_s * 1e6,
                           "kernel_us_from": "timed region / launches (HIP events on the launch stream)",
                           "fp64_tflops": flops_launch / kern_s / 1e12, "fp64_peak_tflops": FP64_PEAK_TFLOPS}
        if args.full:
            g1000_us = graph_kernel_us(apply_only, dev)
            out["roofline"].update(graph1000_us=g1000_us,
                                   frac_graph1000=bytes_launch / (g1000_us * 1e3) / HBM_PEAK_GBS)

    if world > 1:
        # the N > 1 headline changed definition in round 5 (rounds 1-4: weak scaling, 64 x 64 elements per
        # GPU); that quantity is still reported, under "weak" (or "strong" with --scaling weak)
        out["headline_definition"] = (f"{args.scaling} scaling of the {nex}x{ney} mesh over {world} GPUs (round 5 on; "
                                      "rounds 1-4 reported weak scaling, 64x64 elements per GPU, as the headline: "
                                      "that is the 'weak' key here)")
    if args.full and world == 1:
        # BASELINE.json's metric read literally: the Laplacian-only y = K T (16 B/DOF: read T, write y)
        kwl = dict(c_stiff=1.0)
        kl = graph_kernel_us(lambda: mesh.apply(T, y, **kwl), dev) * 1e-6
        out["laplacian_only"] = {"value": N_glob / kl, "unit": "DOF-updates/s", "ms_per_step": kl * 1e3,
                                 "kernel": mesh.kernel_name(), "bytes_per_launch": 16.0 * n_loc,
                                 "achieved": 16.0 * n_loc / kl / 1e9, "unit_bw": "GB/s",
                                 "frac": 16.0 * n_loc / kl / 1e9 / HBM_PEAK_GBS}
        # north_star's MFMA form of the same apply (element-block contractions on
        # v_mfma_f64_16x16x4_f64, SEM_ALGO_MFMA): its fraction of the fp64 MFMA peak, beside the
        # default VALU band kernel that beats it
        kwm = dict(kw, algo=_lib.ALGO_MFMA)
        km = graph_kernel_us(lambda: mesh.apply(T, y, **kwm), dev) * 1e-6
        out["mfma_variant"] = {"kernel": mesh.kernel_name(_lib.ALGO_MFMA), "kernel_us": km * 1e6,
                               "value": N_glob / km, "unit": "DOF-updates/s",
                               "fp64_tflops": flops_launch / km / 1e12, "mfma_peak_tflops": FP64_PEAK_TFLOPS,
                               "frac_mfma_peak": flops_launch / km / 1e12 / FP64_PEAK_TFLOPS,
                               "flops_per_launch": flops_launch, "speedup_band_over_mfma": km / kern_s}

    if args.full and rank == 0 and world == 1 and args.hbm_ne > 0:
        # HBM regime: 1024^2 elements, P=8 (N = 67.1 M, 2.15 GB moved per apply > 256 MB MALL)
        big = get_mesh(P, args.hbm_ne, args.hbm_ne, 1.0 / args.hbm_ne, 1.0 / args.hbm_ne)
        Tb, ub, vb = (torch.rand(big.n_local, dtype=torch.float64, device=dev) * 2 - 1 for _ in range(3))
        yb = torch.empty_like(Tb)
        kwb = dict(kw, cu=ub, cv=vb)
        kb = graph_kernel_us(lambda: big.apply(Tb, yb, **kwb), dev, launches=50, trials=3) * 1e-6
        bb = 32.0 * big.n_local
        wl = f"cd_matvec_{args.hbm_ne}x{args.hbm_ne}_P{P}"
        tb, tbk = load_pmc(wl, big.kernel_name())
        out["roofline_hbm"] = {"workload": wl, "kernel": big.kernel_name(), "dofs": big.n_local,
                               "value": big.n_local / kb, "unit": "DOF-updates/s",
                               "bound": "hbm", "achieved": bb / kb / 1e9, "peak": HBM_PEAK_GBS, "unit_bw": "GB/s",
                               "frac": bb / kb / 1e9 / HBM_PEAK_GBS, "traffic": tb, "traffic_kernel": tbk,
                               "kernel_us": kb * 1e6}
        # BASELINE.json's metric read literally (the Laplacian-only y = K T, 16 B/DOF) in the HBM regime
        kbl = graph_kernel_us(lambda: big.apply(Tb, yb, c_stiff=1.0), dev, launches=50, trials=3) * 1e-6
        bl = 16.0 * big.n_local
        out["roofline_hbm"]["laplacian_only"] = {
            "kernel": big.kernel_name(), "value": big.n_local / kbl, "unit": "DOF-updates/s", "kernel_us": kbl * 1e6,
            "bytes_per_launch": bl, "achieved": bl / kbl / 1e9, "unit_bw": "GB/s", "frac": bl / kbl / 1e9 / HBM_PEAK_GBS}
        del Tb, ub, vb, yb

    if args.full and args.extra_steps > 0:
        # the other meshes per rank count (north_star: absolute numbers at 1, 2, 4 and 8 GPUs): the HBM-regime mesh
        # split into N strips, the weak-scaling mesh (or, with --scaling weak, the strong one), and the HBM-regime
        # weak-scaling mesh of SURVEY 8(d) (weak_ne^2 elements per GPU; at N = 1 its baseline)
        def extra(nex_, ney_, d_, seed, latency):
            es, eg, em, _, (eb_, ee_) = strip_case(nex_, ney_, d_, args.extra_steps, min(args.warmup, 10), seed)
            Ng = (nex_ * P + 1) * (ney_ * P + 1)
            r = {"global_mesh": f"{nex_}x{ney_}", "mesh_per_gpu": f"{ee_ - eb_}x{ney_} elements (rank 0)",
                 "dofs_global": Ng, "value": Ng * args.extra_steps / es, "unit": "DOF-updates/s",
                 "ms_per_step": es / args.extra_steps * 1e3, "steps": args.extra_steps, "hipgraph": eg,
                 "regime": regime(em.n_local, latency),
                 "rank0_bw_GBs": 32.0 * em.n_local / (es / args.extra_steps) / 1e9}
            return r
        if world > 1 and args.hbm_ne > 0:
            out["strong_hbm"] = dict(extra(args.hbm_ne, args.hbm_ne, 1.0 / args.hbm_ne, 4048 + rank, False),
                                     scaling="strong")
            torch.cuda.empty_cache()
        if world > 1 and args.scaling == "strong":
            out["weak"] = dict(extra(ne * world, ne, d, 2024 + rank, True), scaling="weak")
        elif world > 1:
            out["strong"] = dict(extra(ne, ne, d, 2024 + rank, True), scaling="strong")
        if args.weak_ne > 0:
            wn = args.weak_ne
            out["weak_hbm"] = dict(extra(wn * world, wn, 1.0 / wn, 6072 + rank, False), scaling="weak")
            torch.cuda.empty_cache()

    if args.full and rank == 0 and world == 1 and args.vsolve_ne > 0:
        try:
            out["velocity_solve"] = velocity_solve_line(args.vsolve_ne, args.vsolve_P, dev)
        except (RuntimeError, ValueError) as e:   # an extra key: it never fails the headline line
            out["velocity_solve"] = {"error": str(e)[:300]}
        torch.cuda.empty_cache()

    if args.full and rank == 0 and world == 1 and args.cpu_seconds > 0:
        out["cpu_baseline"] = cpu_baseline(P, ne, Pe, args.cpu_seconds)
        out["speedup_vs_cpu"] = value / out["cpu_baseline"]["value"]
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
