"""Static instruction budget and dependent-chain report of a kernel, read from its gfx950 assembly.

Compiles one HIP source of sem_amd/csrc (default apply_band.hip, with the flags of sem_amd/build.py) to assembly,
device only, into a temporary directory -- nothing is written inside the source tree -- and cuts the chosen kernel
at its first and last s_barrier:
  prologue (tile map, staging, pointwise loads) | roles (the contractions; a wave runs one role path) | epilogue.

Default report: VALU (fp64 FMA / add / mul separately), SALU, LDS, VMEM and waitcnt counts per section, and the
even-odd plan's fp64 operation count per wave beside them, so the overhead is explicit.

--chain: what sits on a workgroup's dependent chain without the source asking for it:
  * every s_waitcnt with a vmcnt field between the first and the last barrier (a role path that waits for global
    loads serialises a memory round trip behind barrier 1),
  * every scalar (kernarg) load after the first barrier,
  * the LDS wait points of the epilogue: s_waitcnt instructions with an lgkmcnt field that follow at least one LDS read
    since the previous one (a static count over all epilogue paths, the off-path Dirichlet / mass blocks included).

--entry: the instruction index of the first load through the x buffer resource (what a workgroup executes before its
longest latency starts) and the number of instructions from the last barrier to the last buffer_store.

    python tools/isa_budget.py [--order 8] [--cm 0] [--grad 1] [--chain | --entry]
    python tools/isa_budget.py --source ns_apply.hip --symbol 'ns_apply_band.*Li8E' --chain
    python tools/isa_budget.py --asm FILE ...        # an assembly file made earlier (compile() below)
"""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sem_amd", "csrc")


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def band_shape(P):
    """BandShape<P> of apply_select.h: (TXE, TYE, NS)."""
    return (min(4, max(1, 8 // P)), max(1, 64 // P), 2 if P >= 2 else 1)


def mangle(P, full, cm, grad, shape=None):
    """Symbol of apply_band_kp<P, TXE, TYE, NS, full, cm, grad>."""
    TXE, TYE, NS = shape or band_shape(P)
    b = lambda v: "Lb1E" if v else "Lb0E"  # noqa: E731
    return (f"_ZN3sem13apply_band_kpILi{P}ELi{TXE}ELi{TYE}ELi{NS}E{b(full)}Li{cm}E{b(grad)}EEvPKdS2_S2_"
            "iiiiiiiiNS_8BandArgsE")


def compile(source, out, remarks=None):
    """source (a file name of sem_amd/csrc) -> assembly file `out`, every instantiation, compiled in place with the
    library's flags; `remarks`: a file for the compiler's kernel-resource-usage remarks."""
    sys.path.insert(0, ROOT)
    from sem_amd import build as B
    cmd = [hipcc(), "-O3", "-std=c++17", f"--offload-arch={B.ARCH}", "-I", os.path.join(ROOT, "include"),
           "-DSEM_DIAGNOSTICS=0"] + B.EXTRA_FLAGS.get(source, []) + ["--cuda-device-only", "-S", "-o", out,
                                                                     os.path.join(CSRC, source)]
    if remarks:
        cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + r.stderr[-2000:])
    if remarks:
        with open(remarks, "w") as f:
            f.write(r.stderr)
    return out


def kernel_body(asm_lines, symbol):
    """Instruction lines of the kernel whose symbol matches the regex `symbol` (exactly one must)."""
    rx = re.compile(symbol)
    label = lambda l: l.split(":")[0]  # noqa: E731   ("symbol: ; @symbol")
    starts = [i for i, l in enumerate(asm_lines) if l.startswith("_Z") and ":" in l and rx.search(label(l))]
    if len(starts) != 1:
        names = [label(asm_lines[i]) for i in starts]
        raise KeyError(f"{len(starts)} kernels match {symbol!r}: {names[:8]}")
    st = en = starts[0]
    while not asm_lines[en].startswith(".Lfunc_end"):
        en += 1
    body = []
    for l in asm_lines[st + 1:en]:
        t = l.split(";")[0].strip()
        if t and not t.startswith(".") or t.endswith(":"):
            body.append(t)
    return label(asm_lines[st]), body


def category(op):
    if op.startswith("v_") and "f64" in op:
        if "fma" in op or "fmac" in op:
            return "VALU fp64 fma"
        return "VALU fp64 add/mul"
    if op.startswith("v_cmp") or op.startswith("v_cndmask"):
        return "VALU cmp/select"
    if op.startswith("v_"):
        return "VALU int/move"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "SMEM"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "SALU branch"
    if op.startswith("s_mov") or op.startswith("s_movk"):
        return "SALU move"
    if op.startswith("s_"):
        return "SALU other"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("buffer_") or op.startswith("global_"):
        return "VMEM"
    return None


def barriers(body):
    bars = [i for i, t in enumerate(body) if t.startswith("s_barrier")]
    if not bars:
        raise ValueError("the kernel has no s_barrier")
    return bars


def budget(body):
    bars = barriers(body)
    cuts = [("prologue (tile map, staging loads -> LDS, pointwise loads)", 0, bars[0]),
            ("roles (X and Y contractions; a wave runs one of the role paths)", bars[0], bars[-1]),
            ("epilogue (X + Y + u, v terms, Dirichlet path, stores)", bars[-1], len(body))]
    out = []
    for label, a, b in cuts:
        c = collections.Counter()
        for t in body[a:b]:
            if t.endswith(":"):
                continue
            k = category(t.split()[0])
            if k:
                c[k] += 1
        out.append((label, c))
    return out


def chain(body):
    """The chain report of one kernel body: a dict of
    role_vmcnt_waits   [(instruction index, text)]: s_waitcnt with a vmcnt field, first barrier .. last barrier
    late_scalar_loads  [(index, text)]: s_load* / s_buffer_load* after the first barrier
    epilogue_lds_waits [(index, text, LDS reads since the previous wait)]
    barriers           indices of the s_barrier instructions."""
    bars = barriers(body)
    first, last = bars[0], bars[-1]
    role_vm = [(i, t) for i, t in enumerate(body[first:last], first) if t.startswith("s_waitcnt") and "vmcnt(" in t]
    late = [(i, t) for i, t in enumerate(body[first:], first)
            if t.startswith("s_load") or t.startswith("s_buffer_load")]
    waits, pending = [], 0
    for i, t in enumerate(body[last:], last):
        if t.startswith("ds_read") or t.startswith("ds_load"):
            pending += 1
        elif t.startswith("s_waitcnt") and "lgkmcnt(" in t and pending:
            waits.append((i, t, pending))
            pending = 0
    return {"role_vmcnt_waits": role_vm, "late_scalar_loads": late, "epilogue_lds_waits": waits, "barriers": bars}


def chain_text(name, body):
    c = chain(body)
    b = c["barriers"]
    lines = [f"kernel {name}", f"  instructions {len(body)}, s_barrier at {b}"]
    lines.append(f"  s_waitcnt with vmcnt between the first and last barrier: {len(c['role_vmcnt_waits'])}")
    lines += [f"    [{i}] {t}" for i, t in c["role_vmcnt_waits"]]
    lines.append(f"  scalar loads after the first barrier: {len(c['late_scalar_loads'])}")
    lines += [f"    [{i}] {t}" for i, t in c["late_scalar_loads"]]
    lines.append(f"  epilogue LDS wait points: {len(c['epilogue_lds_waits'])}")
    lines += [f"    [{i}] {t}   <- {n} LDS read(s)" for i, t, n in c["epilogue_lds_waits"]]
    ep_vm = [(i, t) for i, t in enumerate(body[b[-1]:], b[-1]) if t.startswith("s_waitcnt") and "vmcnt(" in t]
    lines.append(f"  epilogue s_waitcnt with vmcnt: {', '.join(t for _, t in ep_vm) or 'none'}")
    return "\n".join(lines)


def entry(body):
    """The two ends of a workgroup's chain that tile-uniform bookkeeping can lengthen: a dict of
    first_x_load   instruction index of the first buffer_load (the staging loads go through x's buffer resource and
                   are the kernel's first buffer loads; the weight / coefficient tables before them are global_load)
    tail           instructions after the last s_barrier up to and including the last buffer_store (labels not
                   counted): a static count over every epilogue path
    rcp_before_barrier  v_rcp* instructions in front of the first barrier (a runtime integer division)
    waits_before_load   s_waitcnt instructions in front of the first buffer load: one belongs to the fallback
                        prologue of the preloaded arguments; any other puts a kernarg or table fetch in front of
                        the staging loads."""
    bars = barriers(body)
    loads = [i for i, t in enumerate(body) if t.startswith("buffer_load")]
    stores = [i for i, t in enumerate(body) if t.startswith("buffer_store")]
    if not loads or not stores:
        raise ValueError("the kernel has no buffer load or no buffer store")
    tail = sum(1 for t in body[bars[-1] + 1:stores[-1] + 1] if not t.endswith(":"))
    rcp = [(i, t) for i, t in enumerate(body[:bars[0]]) if t.startswith("v_rcp")]
    waits = [(i, t) for i, t in enumerate(body[:loads[0]]) if t.startswith("s_waitcnt")]
    return {"first_x_load": loads[0], "tail": tail, "rcp_before_barrier": rcp, "waits_before_load": waits,
            "barriers": bars}


def entry_text(name, body):
    e = entry(body)
    return "\n".join([f"kernel {name}", f"  instructions {len(body)}, s_barrier at {e['barriers']}",
                      f"  first load through the x buffer resource: instruction {e['first_x_load']}",
                      f"  instructions from the last barrier to the last buffer_store: {e['tail']}",
                      f"  v_rcp in front of the first barrier: {len(e['rcp_before_barrier'])}",
                      f"  s_waitcnt in front of the first buffer load: {[i for i, _ in e['waits_before_load']]}"])


def resources(remarks_text, symbol):
    """{kernel symbol: {field: int}} from the compiler's kernel-resource-usage remarks, kernels matching `symbol`."""
    rx, out, cur = re.compile(symbol), {}, None
    for l in remarks_text.split("\n"):
        m = re.search(r"remark:\s+Function Name: (\S+)", l)
        if m:
            cur = out.setdefault(m.group(1), {}) if rx.search(m.group(1)) else None
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", l)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


def resources_text(remarks_text):
    """Band-kernel table, every order and both coefficient modes (apply_band_kp<P, ..., false, CM, true>):
    workgroups per CU = min(LDS: 160 KiB / LDS bytes, registers: 4 SIMDs x occupancy / waves, 32 waves / waves)."""
    rows = ["  P CM  waves  VGPRs  scratch  occ/SIMD  LDS bytes  WG/CU by LDS  by regs  by waves"]
    for P in range(1, 17):
        for cm in (0, 1):
            r = resources(remarks_text, re.escape(mangle(P, False, cm, True)) + "$")
            if len(r) != 1:
                rows.append(f"{P:3d} {cm:2d}  (not compiled)")
                continue
            v = next(iter(r.values()))
            TXE, TYE, NS = band_shape(P)
            xw = (TYE * P + 63) // 64
            waves = TXE * NS * xw + NS * ((TXE * P * TYE + 63) // 64)
            rows.append(f"{P:3d} {cm:2d} {waves:6d} {v['VGPRs']:6d} {v['ScratchSize']:8d} {v['Occupancy']:9d} "
                        f"{v['LDS Size']:10d} {160 * 1024 // v['LDS Size']:13d} {4 * v['Occupancy'] // waves:8d} "
                        f"{32 // waves:9d}")
    return "\n".join(rows)


def eo_plan_ops(P=8, NS=2, grad=True):
    """fp64 operations per element line of rows in the even-odd band plan (both K and G rows)."""
    H = (P + 1) // 2
    row0 = (2 * P if grad else P) + 2 * P + 2          # K, G FMAs; t[P+m] +- t[P-m]; the fold multiplies
    pair = (4 * H if grad else 2 * H) + (2 if P % 2 == 0 else 0) * (2 if grad else 1) + 4
    centre = (2 * H + 2) if P % 2 == 0 else 0
    eo = 2 * H
    npairs = (P - 1) // 2
    per_element_line = row0 + npairs * pair + centre + eo * (NS)     # e/o formed once per split that needs it
    return per_element_line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", default="", help="an assembly file made earlier instead of compiling")
    ap.add_argument("--source", default="apply_band.hip", help="file of sem_amd/csrc to compile")
    ap.add_argument("--symbol", default="", help="regex on the mangled kernel name (default: apply_band_kp of --order)")
    ap.add_argument("--order", type=int, default=8)
    ap.add_argument("--cm", type=int, default=0)
    ap.add_argument("--grad", type=int, default=1)
    ap.add_argument("--full", type=int, default=0)
    ap.add_argument("--chain", action="store_true")
    ap.add_argument("--entry", action="store_true", help="first staging load and the tail behind the last barrier")
    ap.add_argument("--resources", action="store_true", help="registers, LDS, occupancy of the band kernel per order")
    ap.add_argument("--remarks", default="", help="with --resources: a remarks file made earlier")
    a = ap.parse_args()
    if a.resources:
        with tempfile.TemporaryDirectory() as tmp:
            rem = a.remarks or os.path.join(tmp, "remarks.txt")
            if not a.remarks:
                compile("apply_band.hip", os.path.join(tmp, "kernel.s"), rem)
            print(resources_text(open(rem).read()))
        return 0
    with tempfile.TemporaryDirectory() as tmp:
        asm = a.asm or compile(a.source, os.path.join(tmp, "kernel.s"))
        lines = open(asm).read().split("\n")
    symbol = a.symbol or re.escape(mangle(a.order, bool(a.full), a.cm, bool(a.grad)))
    name, body = kernel_body(lines, symbol)
    if a.chain:
        print(chain_text(name, body))
        return 0
    if a.entry:
        print(entry_text(name, body))
        return 0
    print(f"kernel {name}")
    total = collections.Counter()
    for label, c in budget(body):
        total.update(c)
        valu = sum(v for k, v in c.items() if k.startswith("VALU"))
        salu = sum(v for k, v in c.items() if k.startswith("SALU"))
        print(f"{label}: VALU {valu}, SALU {salu}, " + ", ".join(f"{k} {v}" for k, v in sorted(c.items())))
    if not a.symbol:
        P, (TXE, TYE, NS) = a.order, band_shape(a.order)
        per_line = eo_plan_ops(P, NS, bool(a.grad))
        # X: one lane per tile column, Y: one lane per (line, element position); each carries one element line of rows
        nodes = TXE * P * TYE * P
        tile = 2 * TYE * P * TXE * per_line
        print(f"even-odd plan: {per_line} fp64 ops per element line of rows (both directions' K{'+G' if a.grad else ''});"
              f" per tile of {nodes} nodes {tile} lane-ops = {tile / nodes:.1f} per node"
              f" -- the epilogue's combination adds ~4 per node")
    print("static totals: " + ", ".join(f"{k} {v}" for k, v in sorted(total.items())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
