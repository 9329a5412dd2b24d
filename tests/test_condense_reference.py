"""CPU tests of tests/condense_reference.py, the long-double references the GPU tests of the line-condensation kernels
(tests/test_gpu_condense_launches.py) compare with.

Layout tie: on a real factor of a CPU VelocityJacobianSolver the references, chained launch after launch, reproduce the
solver's torch formulation (_nested_solve, _edge_thomas_solve, and the interface right-hand side and back substitution
of _solve_lines) within the chained bounds -- the references read pi, pe, the blocks, aIB, aBI and x_B|n the way the
solver writes them.  The chained bound of an output is the single-launch bound of condense_reference's docstring plus
|M| x (the bound of the launch's input); torch's products are sums in some order, which the bound covers.  The
references that go through XiB, AXB and ABY (rounded once from long double) are compared with the same torch values
under the sum of the two paths' chained bounds: each path's bound already allows n u |M| |x| >= u |M| |x|, the effect
of that rounding.

Sensitivity: the same operations in plain float64 pass every bound, and each mutant -- a dropped El term, Eu[k-1] for
Eu[k], the halves of C swapped, the aIB / xB correction dropped, x_B|n read (component, side, height), the closing
edge of Pw omitted, pi's heights shifted by one -- fails the bound of the first output it reaches.

Cap: SLACK x bound <= 1e-12 for every single-launch bound at every shape the GPU tests run."""
import functools

import numpy as np
import pytest
import torch

import condense_reference as cr
from condense_reference import LD, SLACK, Case
from sem_amd.solvers.velocity_solve import VelocityJacobianSolver
from velocity_blocks import extract, oracle_cd_jacobian, oracle_velocity_jacobian

F64 = np.float64


# ---- layout tie ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _factor(nc, P, nex, ney, edge):
    if nc == 2:
        ns, _, _ = oracle_velocity_jacobian(P, nex, ney, 100.0, seed=P * 10 + nex)
        pcs = extract(ns.Jvelo.toarray(), P, nex, ney)
    else:
        _, A, _, _ = oracle_cd_jacobian(P, nex, ney, 40.0, seed=P + nex)
        pcs = extract(A.toarray(), P, nex, ney, ncomp=1)
    pcs = {k: torch.as_tensor(v) for k, v in pcs.items()}
    vs = VelocityJacobianSolver(P, nex, ney, "cpu", sweep="thomas", ncomp=nc)
    if edge == "thomas":
        vs.edge_dense_max, vs.edge_solve = 0, "thomas"
    else:
        vs.edge_solve = "dense"
    vs.factor(pcs["AII"], pcs["D"], pcs["aIB"], pcs["aBI"], pcs["E"], pcs["F"])
    assert vs._edge_thomas == (edge == "thomas")
    return vs


def _tie_case(vs, B):
    """The Case over the solver's factor and the line array B (NX, m)."""
    c = Case(vs.P, vs.nex, vs.ney, vs.ncomp)
    assert np.array_equal(c.pi, vs._pi.numpy()) and np.array_equal(c.pe, vs._pe.numpy())
    assert (c.m, c.nI, c.ne1) == (vs.m, vs.nI, vs._ne1)
    c.Xi, c.Aei, c.Yie = vs._Xi.numpy(), vs._Aei.numpy(), vs._Yie.numpy()
    if vs._edge_thomas:
        c.Ed, c.El, c.Eu = vs._Ed.numpy(), vs._El.numpy(), vs._Eu.numpy()
    else:
        c.Se = vs._Se_inv.numpy()
    c.aIB, c.aBI = vs.aIB.numpy(), vs.aBI.numpy()
    c.ld_r = c.ld_b = c.P * c.m
    c.R = B[1:].reshape(c.nex, c.P * c.m)       # column e: lines e P + 1 .. e P + P (the last one is the interface)
    c.Bl = B.reshape(-1, c.m)
    c.xB = np.zeros((c.nex + 1, c.m))
    c.XiB, c.AXB, c.ABY = cr.coupling_blocks(c)
    return c


@pytest.mark.parametrize("edge", ["dense", "thomas"])
@pytest.mark.parametrize("nc,P,nex,ney", [(2, 4, 3, 2), (1, 5, 2, 3)])
def test_references_reproduce_the_torch_solver(nc, P, nex, ney, edge):
    vs = _factor(nc, P, nex, ney, edge)
    m, nI = vs.m, vs.nI
    B = np.random.default_rng(11 * P + nc).uniform(-1, 1, (vs.NX, m))
    c = _tie_case(vs, B)
    # the torch path of _solve_lines_once, step by step
    Bt = torch.as_tensor(B)
    bI = Bt[:-1].reshape(nex, P, m)[:, 1:, :].reshape(nex, nI, 1)
    yI = vs._nested_solve(bI)
    g = Bt[0::P].clone()
    yIr = yI.view(nex, P - 1, m)
    g[:-1] -= (vs.aBI[:, 0] * yIr).sum(1)
    g[1:] -= (vs.aBI[:, 1] * yIr).sum(1)
    xB = vs._iface_solve(g.clone())
    rI = bI.view(nex, P - 1, m) - (vs.aIB[:, :, 0, :] * xB[:-1, None, :] + vs.aIB[:, :, 1, :] * xB[1:, None, :])
    xI = vs._nested_solve(rI.reshape(nex, nI, 1))
    out = torch.empty((vs.NX, m), dtype=torch.float64)
    out[0::P] = xB
    out[:-1].view(nex, P, m)[:, 1:, :] = xI.view(nex, P - 1, m)
    assert torch.equal(out, vs._solve_lines(Bt))

    # forward: K1 -> K2 -> K3
    ch = cr.chain_solve(c, False)
    assert cr.within(yI.numpy()[..., 0], ch["Y"], ch["bY"]), cr.worst(yI.numpy()[..., 0], ch["Y"], ch["bY"])
    # the edge solve alone, on a float64 right-hand side
    re64 = ch["re"].astype(F64)
    Re = torch.as_tensor(re64).reshape(nex, c.n_e, 1)
    ye_t = (vs._edge_thomas_solve(Re) if edge == "thomas" else vs._Se_inv @ Re).numpy().reshape(re64.shape)
    ye, bye = cr.ref_edge(c, re64.astype(LD))
    assert cr.within(ye_t, ye, bye), cr.worst(ye_t, ye, bye)
    # interface right-hand side: from y_I, and from T and the edge values through ABY
    g1, b1 = cr.ref_interface_rhs(P, nex, m, B[::P], c.aBI, ch["Y"], ch["bY"])
    assert cr.within(g.numpy(), g1, b1), cr.worst(g.numpy(), g1, b1)
    ci = cr.chain_iface_rhs(c)
    assert np.all(np.isfinite(ci["Pw"].astype(F64)))
    assert cr.within(g.numpy(), ci["g"], ci["bg"] + b1), cr.worst(g.numpy(), ci["g"], ci["bg"] + b1)
    # back substitution: through Xi with the corrected right-hand side, and from T, C through XiB and AXB
    c.xB = xB.numpy()
    cb = cr.chain_solve(c, True)
    assert cr.within(xI.numpy()[..., 0], cb["Y"], cb["bY"]), cr.worst(xI.numpy()[..., 0], cb["Y"], cb["bY"])
    c2 = cr.chain_back_solve(c, ch["T"], ch["C"], ch["bT"], ch["bC"])
    assert cr.within(xI.numpy()[..., 0], c2["Y"], c2["bY"] + cb["bY"]), \
        cr.worst(xI.numpy()[..., 0], c2["Y"], c2["bY"] + cb["bY"])
    # none of this is vacuous: every bound is far below the values
    for ref, b in ((ch["Y"], ch["bY"]), (g1, b1), (cb["Y"], cb["bY"]), (c2["Y"], c2["bY"])):
        assert float(b.max()) <= 1e-9 * float(np.abs(ref).max())


# ---- sensitivity ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sens_case(edge):
    c = Case.synthetic(4, 2, 3, 2, edge, True, seed=3)
    return c, cr.chain_solve(c, True), cr.chain_back_solve(c, c.T0, c.C0), cr.chain_iface_rhs(c)


def _verdicts(edge, mutant):
    """name -> whether the float64 evaluation (with the mutant) of each output is within its bound."""
    c, rs, rb, ri = _sens_case(edge)
    ms = cr.chain_solve(c, True, F64, mutant)
    mb = cr.chain_back_solve(c, c.T0, c.C0, dt=F64, mutant=mutant)
    mi = cr.chain_iface_rhs(c, F64, mutant)
    out = {}
    for tag, m, r, keys in (("solve", ms, rs, ("T", "C", "ye", "Y")), ("back", mb, rb, ("T", "C", "ye", "Y")),
                            ("iface", mi, ri, ("T", "C", "ye", "Pw", "g"))):
        for k in keys:
            out[tag + "." + k] = cr.within(m[k], r[k], r["bY" if k == "Y" else "b" + k])
    return out


@pytest.mark.parametrize("edge", ["dense", "thomas"])
def test_float64_evaluation_passes_every_bound(edge):
    v = _verdicts(edge, None)
    assert len(v) == 13 and all(v.values()), v


# the first outputs each mutant must break, and outputs upstream of it that must still pass
_MUTANTS = {
    "drop_El": ("thomas", ["solve.ye", "solve.Y", "back.ye", "iface.ye", "iface.Pw", "iface.g"],
                ["solve.T", "solve.C"]),
    "shift_Eu": ("thomas", ["solve.ye", "solve.Y", "back.ye", "iface.ye", "iface.g"], ["solve.T", "solve.C"]),
    "swap_C": ("both", ["solve.ye", "solve.Y", "back.ye", "iface.ye", "iface.g"], ["solve.T", "solve.C", "back.T"]),
    "drop_coupling": ("both", ["solve.T", "solve.C", "solve.ye", "solve.Y", "back.ye"], ["iface.T", "iface.g"]),
    "xB_order": ("both", ["back.T", "back.C", "back.ye", "back.Y"], ["solve.Y", "iface.g"]),
    "no_closing_edge": ("both", ["iface.Pw", "iface.g"], ["iface.T", "iface.C", "iface.ye", "solve.Y"]),
    "shift_pi": ("both", ["solve.T", "solve.C", "solve.Y", "back.Y", "iface.T", "iface.g"], ["back.T", "back.C"]),
}


@pytest.mark.parametrize("mutant", cr.MUTANTS)
def test_mutant_fails_its_bound(mutant):
    assert set(_MUTANTS) == set(cr.MUTANTS)
    edges, broken, intact = _MUTANTS[mutant]
    for edge in (("dense", "thomas") if edges == "both" else (edges,)):
        v = _verdicts(edge, mutant)
        assert not any(v[k] for k in broken), (edge, {k: v[k] for k in broken})
        assert all(v[k] for k in intact), (edge, {k: v[k] for k in intact})


def test_thomas_mutants_land_far_outside_the_bound():
    """A dropped El term is not a near miss: it lands more than 1e9 bounds away."""
    c, rs, _, _ = _sens_case("thomas")
    m = cr.chain_solve(c, True, F64, "drop_El")
    assert cr.worst(m["ye"], rs["ye"], rs["bye"]) > 1e9


# ---- the cap on every bound the GPU tests use ------------------------------------------------------------------------

def single_launch_bounds(c, coupled):
    """name -> largest single-launch bound of sem_nested_solve (coupled or not), sem_nested_back_solve and
    sem_nested_iface_rhs at this case, every launch fed the reference's values (the GPU tests feed the device's,
    which differ from them by less than these bounds)."""
    out = {}
    T, bT = cr.ref_T(c, coupled)
    C, bC = cr.ref_C(c, T)
    re, dre = cr.ref_re(c, coupled, C)
    ye, bye = cr.ref_edge(c, re, dre)
    _, bYi = cr.ref_Yi(c, T, ye)
    out.update(T=bT, C=bC, ye=bye, Yi=bYi)
    if coupled:
        T2, C2, bT2, bC2 = cr.ref_coupled(c, c.T0, c.C0)
        re2, dre2 = cr.ref_re(c, True, C2)
        ye2, bye2 = cr.ref_edge(c, re2, dre2)
        _, bYi2 = cr.ref_Yi(c, T2, ye2)
        out.update(backT=bT2, backC=bC2, backye=bye2, backYi=bYi2)
    else:
        Pw, bPw = cr.ref_Pw(c, T, ye)
        _, bg = cr.ref_g_sum(c, Pw)
        out.update(Pw=bPw, g=bg)
    return {k: float(np.max(v)) for k, v in out.items()}


def _all_cases():
    cases = set(cr.solve_cases()) | set(cr.back_cases())
    cases |= {(P, nex, ney, nc, edge) for nc, P, nex, ney, edge in cr.IFACE}
    return sorted(cases)


@pytest.mark.parametrize("P,nex,ney,nc,edge", _all_cases())
def test_every_bound_is_capped(P, nex, ney, nc, edge):
    for coupled in (False, True):
        c = Case.synthetic(P, nex, ney, nc, edge, coupled)
        for k, b in single_launch_bounds(c, coupled).items():
            assert 0.0 < SLACK * b <= cr.CAP, (k, b)


@pytest.mark.parametrize("P,nex,m", cr.INTERFACE)
def test_interface_rhs_bound_is_capped(P, nex, m):
    r = np.random.default_rng(m)
    args = (r.uniform(-1, 1, (nex + 1, m)), r.uniform(-1, 1, (nex, 2, P - 1, m)), r.uniform(-1, 1, (nex, (P - 1) * m)))
    g, b = cr.ref_interface_rhs(P, nex, m, *args)
    assert 0.0 < SLACK * float(b.max()) <= cr.CAP
    g64, _ = cr.ref_interface_rhs(P, nex, m, *args, dt=F64)
    assert cr.within(g64, g, b)
    bad = g64.copy()
    bad[1:] += (args[1][:, 1, 0] * args[2][:, :m])          # the first line's term of the left column dropped
    assert not cr.within(bad, g, b)


def test_thomas_bound_against_float64_over_widths_and_lengths():
    """The running bound of the block-Thomas recurrence over widths and chain lengths: float64 stays within it, a
    dropped El term does not."""
    for nc, P, ney in [(1, 2, 1), (1, 4, 2), (1, 6, 4), (2, 5, 6), (1, 16, 3), (2, 16, 8), (1, 32, 2), (1, 33, 4)]:
        c = Case(P, 1, ney, nc)
        r = np.random.default_rng(P + ney)
        B = c.ne1
        c.Ed, c.El, c.Eu = (r.uniform(-1, 1, (1, n, B, B)) / B for n in (ney + 1, ney, ney))
        re = r.uniform(-1, 1, (1, ney + 1, B))
        ye, bye = cr.ref_edge(c, re.astype(LD))
        assert SLACK * float(bye.max()) <= cr.CAP
        y64, _ = cr.ref_edge(c, re, dt=F64)
        assert cr.within(y64, ye, bye)
        bad, _ = cr.ref_edge(c, re, dt=F64, mutant="drop_El")
        assert not cr.within(bad, ye, bye) and cr.worst(bad, ye, bye) > 1e9
