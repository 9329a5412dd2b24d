"""CPU tests of tests/velocity_reference.py, the long-double reference the GPU tests of velocity_blocks_kernel
(tests/test_gpu_velocity_blocks_launches.py) compare with.

Oracle tie: on whole meshes the reference's pieces are the pieces of the oracle's assembled float64 Jacobians
(NSOracle.Jvelo, the CD oracle's Sys with identity rows) within the entry bound, T = 0: the same tables on both sides.

Operator tie: the dense matrix times [u; v] is (ru, rv) of ns_reference -- sem_ns_apply's reference -- to long-double
rounding, on whole meshes and on first, middle and last strips with the irregular mask: the assembled Jacobian and the
applied operator are one operator, the strips' ownership rule included.

Layout tie: the pieces name every non-zero of the matrix once; the condensed pieces are
VelocityJacobianSolver.condense_dense of the dense ones and name every non-zero of A_II once; a strip's pieces are those
of tests/cpu_mesh.py's condensed_blocks, which gives a shared line's D block whole to its right-hand owner where the
kernel gives each side its partial sum: there the two strips' reference blocks add up to it.

Sensitivity: the kernel's formulas in plain float64 (kernel_f64) stay inside the bound at every shape the GPU tests
run, on the oracle's tables with T = 0 and on the library's host tables with the table allowance, and write every
entry; each of the ten mutants fails."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import velocity_reference as vr
from cpu_mesh import CPUStripMesh
from ns_reference import LD, ns_reference
from velocity_blocks import extract, oracle_cd_jacobian, oracle_velocity_jacobian
from velocity_reference import Case

WHOLE = [(4, 3, 2), (2, 2, 3), (1, 4, 3), (3, 1, 2), (6, 2, 2)]
STRIPS = [(3, 4, 2, 0, 4), (3, 4, 2, 0, 2), (3, 4, 2, 1, 3), (3, 4, 2, 2, 4), (1, 4, 3, 1, 3), (2, 3, 1, 1, 2),
          (5, 2, 2, 0, 1)]


def _ok(got, ref, P, **kw):
    worst, fails = vr.compare(got, ref, P, **kw)
    assert not fails, fails
    return worst


# ---- the oracle ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,nex,ney", WHOLE)
def test_reference_matches_the_oracle_velocity_jacobian(P, nex, ney):
    Re = 100.0
    ns, u, v = oracle_velocity_jacobian(P, nex, ney, Re, seed=P * 10 + nex)
    c = Case(P, nex, ney, 0, nex, nc=2, dx=1.0 / nex, dy=1.0 / ney).with_operands(
        dict(c_mass=0.0, c_stiff=1.0, c_gradx=Re, c_grady=Re),
        dict(cu=u, cv=v, juu=Re * (ns.Gx @ u), juv=Re * (ns.Gy @ u), jvu=Re * (ns.Gx @ v), jvv=Re * (ns.Gy @ v)),
        None, 15)
    got = extract(ns.Jvelo.toarray(), P, nex, ney)
    assert _ok(got, vr.reference(c), P, tables_differ=False) <= vr.SLACK


@pytest.mark.parametrize("P,nex,ney", WHOLE)
def test_reference_matches_the_oracle_cd_jacobian(P, nex, ney):
    Pe = 40.0
    _, A, u, v = oracle_cd_jacobian(P, nex, ney, Pe, seed=P + nex)
    c = Case(P, nex, ney, 0, nex, nc=1, dx=1.0 / nex, dy=1.0 / ney).with_operands(
        dict(c_mass=0.0, c_stiff=1.0, c_gradx=Pe, c_grady=Pe), dict(cu=u, cv=v), None, 3)
    got = extract(A.toarray(), P, nex, ney, ncomp=1)
    assert _ok(got, vr.reference(c), P, tables_differ=False) <= vr.SLACK


# ---- the applied operator ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("mask", ["irregular", "sides15", "sides9"])
@pytest.mark.parametrize("P,nex,ney,eb,ee", STRIPS)
def test_dense_matrix_is_the_operator_ns_reference_applies(P, nex, ney, eb, ee, mask, nc):
    c = Case(P, nex, ney, eb, ee, nc=nc, desc="full", mask=mask)
    J, mag = vr.dense_jacobian(c)[:2]
    r = np.random.default_rng(P + 7 * eb)
    u = r.uniform(-1, 1, c.n)
    v = r.uniform(-1, 1, c.n) if nc == 2 else None
    x = np.concatenate((u, v) if nc == 2 else (u,)).astype(LD)
    kw = dict(c.coef, dir_mask=c.dir_mask, dir_sides=c.dir_sides, **c.f)
    want = ns_reference(P, nex, ney, c.dx, c.dy, eb, ee, u, v, None, **kw)[:nc]
    scale = ns_reference(P, nex, ney, c.dx, c.dy, eb, ee, u, v, None, absval=True, **kw)[:nc]
    got, amag = J @ x, mag @ np.abs(x)
    eps = LD(np.finfo(LD).eps)
    terms = 4 * (P + 1) + 8
    for k in range(nc):
        g, w, s = got[k * c.n:(k + 1) * c.n], want[k], scale[k]
        dirichlet = s == np.abs(x[k * c.n:(k + 1) * c.n])      # identity rows (and the all-zero non-owned ones)
        assert np.all(np.abs(g - w) <= terms * eps * s), float(np.max(np.abs(g - w) / np.maximum(s, LD(1e-300))) / eps)
        # the per-entry sums of absolute terms add up to ns_reference's per-row ones
        assert np.all(np.abs(amag[k * c.n:(k + 1) * c.n] - s)[~dirichlet] <= terms * eps * s[~dirichlet])


def test_perimeter_mask_is_dir_sides_15():
    for P, nex, ney, eb, ee in STRIPS:
        a = Case(P, nex, ney, eb, ee, mask="sides15")
        b = Case(P, nex, ney, eb, ee, mask="perimeter")
        assert b.dir_mask is not None and a.dir_mask is None
        for x, y in zip(vr.dense_jacobian(a), vr.dense_jacobian(b)):
            assert np.array_equal(x, y)
        for lay in ("dense", "condensed") if P > 1 else ("dense",):
            ka, kb = vr.kernel_f64(a, lay), vr.kernel_f64(b, lay)
            assert all(np.array_equal(ka[k].view(np.int64), kb[k].view(np.int64)) for k in ka)


@pytest.mark.parametrize("P,nex,ney,eb,ee", vr.SHAPES)
def test_irregular_mask_holds_every_node_class(P, nex, ney, eb, ee):
    c = Case(P, nex, ney, eb, ee, mask="irregular")
    cl = vr.mask_classes(P, ney, c.dir_mask, c.lines)
    assert cl["corner"] and cl["first"] and cl["last"] and not np.all(c.dir_mask)
    if P > 1:
        assert cl["interior"] and cl["interface"] and {0, ney, ney // 2} <= cl["edge_k"]
    # and dir_sides, which the mask overrides, would give another set
    assert c.dir_sides == 10


# ---- the layouts ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("P,nex,ney,eb,ee", STRIPS)
def test_pieces_name_every_nonzero_once_and_the_layouts_agree(P, nex, ney, eb, ee, nc):
    from sem_amd.solvers.velocity_solve import VelocityJacobianSolver
    c = Case(P, nex, ney, eb, ee, nc=nc, desc="full", mask="irregular")
    J = vr.dense_jacobian(c)[0].astype(np.float64)
    dense = vr.pieces(c, J, "dense")
    assert np.count_nonzero(J) == sum(np.count_nonzero(a) for a in dense.values())
    if P == 1:
        return
    cond = vr.pieces(c, J, "condensed")
    for k in vr.IFACE:
        assert np.array_equal(dense[k], cond[k])
    assert np.count_nonzero(dense["AII"]) == sum(np.count_nonzero(cond[k]) for k in vr.COND)
    vs = VelocityJacobianSolver(P, c.ne, ney, "cpu", ncomp=nc)
    want = vs.condense_dense(torch.as_tensor(dense["AII"]))
    for k in vr.COND:
        assert np.array_equal(want[k].numpy(), cond[k]), k
    # a column range: the blocks of those columns, counted from the first of them
    for name, cols in vr.column_ranges(eb, ee).items():
        cc = Case(P, nex, ney, eb, ee, nc=nc, desc="full", mask="irregular", cols=cols)
        lo, hi = cols[0] - eb, cols[1] - eb
        sub_d, sub_c = vr.pieces(cc, J, "dense"), vr.pieces(cc, J, "condensed")
        assert np.array_equal(sub_d["AII"], dense["AII"][lo:hi])
        for k in vr.COND:
            assert np.array_equal(sub_c[k], cond[k][lo:hi]), (k, name)
        for k in vr.IFACE:
            assert np.array_equal(sub_d[k], dense[k])


def _global_fields(P, nex, ney, seed):
    r = np.random.default_rng(seed)
    N = (nex * P + 1) * (ney * P + 1)
    return {k: r.uniform(-1, 1, N) for k in vr.FIELDS}, (r.random(N) < 0.2).astype(np.uint8)


@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("P,nex,ney,bounds", [(3, 4, 2, (0, 1, 3, 4)), (2, 3, 3, (0, 2, 3)), (4, 2, 1, (0, 1, 2))])
def test_strip_pieces_match_the_cpu_mesh(P, nex, ney, bounds, nc):
    """Every piece but the D blocks of shared lines equals CPUStripMesh.condensed_blocks (the oracle's float64
    operators: entry bound, T = 0); the two strips' blocks of a shared line add up to the block the CPU mesh gives
    the right-hand strip."""
    gf, gmask = _global_fields(P, nex, ney, 5 * P + nex)
    NY = ney * P + 1
    refs, cpu = [], []
    for eb, ee in zip(bounds[:-1], bounds[1:]):
        sl = slice(eb * P * NY, (ee * P + 1) * NY)
        names = vr.FIELDS if nc == 2 else ("cu", "cv", "juu")
        c = Case(P, nex, ney, eb, ee, nc=nc).with_operands(vr.COEF, {k: gf[k][sl] for k in names}, gmask[sl], 0)
        ref = vr.reference(c, "condensed")
        blocks = {k: torch.zeros(s, dtype=torch.float64) for k, s in c.shapes("condensed").items()}
        CPUStripMesh(P, nex, ney, c.dx, c.dy, eb, ee).condensed_blocks(
            blocks, dir_mask=torch.as_tensor(gmask[sl]), ncomp=nc, **vr.COEF,
            **{k: torch.as_tensor(gf[k][sl]) for k in names})
        got = {k: b.numpy() for k, b in blocks.items()}
        refs.append(ref)
        cpu.append(got)
        shared = [L for L, on in ((0, eb > 0), (c.ne, ee < nex)) if on]
        keep = [L for L in range(c.ne + 1) if L not in shared]
        cut = lambda a, k: a[keep] if k == "D" else a     # noqa: E731
        _ok({k: cut(a, k) for k, a in got.items()}, {k: tuple(cut(a, k) for a in t) for k, t in ref.items()}, P,
            tables_differ=False)
    for left, right, whole in zip(refs[:-1], refs[1:], cpu[1:]):
        (a, ma, ka, ta), (b, mb, kb, tb) = (tuple(x[-1] for x in left["D"]), tuple(x[0] for x in right["D"]))
        total, mag = a + b, ma + mb
        kind = np.where((ka == vr.EXACT) | (kb == vr.EXACT), vr.EXACT, np.where(mag == 0, vr.ZERO, vr.BOUND))
        assert np.all(a[(kb == vr.EXACT) & (total == 1)] == 0)       # the identity diagonal is the owner's alone
        _ok({"D": whole["D"][0]}, {"D": (total, mag, kind.astype(np.int8), ta + tb)}, P, tables_differ=False)


# ---- the bound can fail --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _library_tables(P):
    """(w, K_s, G_s) of the library's host functions: what sem_create uploads for the kernels."""
    from sem_amd import _lib
    lib = _lib.load()
    n = P + 1
    x, w, K, G = np.zeros(n), np.zeros(n), np.zeros((n, n)), np.zeros((n, n))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    _lib.check(lib.sem_gll_nodes(P, dp(x), dp(w), None))
    _lib.check(lib.sem_gll_stiffness(P, dp(K)))
    _lib.check(lib.sem_gll_gradient(P, dp(G)))
    return w, K, G


@pytest.mark.parametrize("P", sorted({s[0] for s in vr.SHAPES}))
def test_library_tables_against_the_oracles(P):
    """What the bound assumes of the tables: w and G_s agree with the oracle's to the last place and have the same
    zeros (the entries compared == 0); K_s agrees within the two evaluations' rounding (T of the docstring)."""
    from oracle import sem_oracle as O
    w, K, G = _library_tables(P)
    ow, oK, oG = O.gll_nodes(P)[1], O.gll_K(P), O.gll_G(P)
    assert np.array_equal(G == 0, oG == 0) and not np.any(K == 0) and not np.any(oK == 0) and not np.any(w == 0)
    assert np.all(np.abs(w - ow) <= np.spacing(ow)) and np.all(np.abs(G - oG) <= np.spacing(np.abs(oG)))
    aK = np.abs(O.gll_D(P)).T @ (ow[:, None] * np.abs(O.gll_D(P)))
    assert np.all(np.abs(K - oK) <= vr.table_roundings(P) * vr.U53 * aK)


@pytest.mark.parametrize("P,nex,ney,eb,ee", vr.SHAPES)
def test_float64_evaluation_is_inside_the_bound(P, nex, ney, eb, ee):
    """kernel_f64 on the oracle's tables (T = 0) and on the library's (T = 2 (P + 2)), both layouts, ncomp 1 and 2,
    the full descriptor and the stiffness alone, the irregular mask and the sides: every entry finite (so written),
    exact where it must be, inside the bound elsewhere."""
    worst = 0.0
    for nc in (1, 2):
        for desc, mask in (("full", "irregular"), ("stiff", "sides15"), ("null", "sides9"), ("jac", "irregular")):
            for name, cols in vr.column_ranges(eb, ee).items():
                if name not in ("all", "middle" if ee - eb >= 3 else "last"):
                    continue
                c = Case(P, nex, ney, eb, ee, nc=nc, desc=desc, mask=mask, cols=cols)
                for lay in ("dense", "condensed") if P > 1 else ("dense",):
                    ref = vr.reference(c, lay)
                    worst = max(worst, _ok(vr.kernel_f64(c, lay), ref, P, tables_differ=False),
                                _ok(vr.kernel_f64(c, lay, tabs=_library_tables(P)), ref, P))
    assert worst <= vr.SLACK


MUTANT_CASE = (4, 5, 2, 1, 4)      # a middle strip: a first line with a left neighbour, a non-owned right line


@pytest.mark.parametrize("mutant", vr.MUTANTS)
def test_mutants_fail_the_bound(mutant):
    lay = "condensed" if mutant == "swap_Aeu_Ael" else "dense"
    c = Case(*MUTANT_CASE, nc=2, desc="full", mask="irregular")
    ref = vr.reference(c, lay)
    assert not vr.compare(vr.kernel_f64(c, lay), ref, c.P, tables_differ=False)[1]
    _, fails = vr.compare(vr.kernel_f64(c, lay, mutant=mutant), ref, c.P)
    assert fails, mutant


def test_mutants_are_the_ten_of_the_list():
    assert len(vr.MUTANTS) == len(set(vr.MUTANTS)) == 10


def test_launch_selection_covers_every_value_with_every_handle_kind():
    """tests/test_gpu_velocity_blocks_launches.py runs launches(shape) for every shape: each value of each factor
    with each handle kind (the middle column range needs three columns: whole and middle-strip handles have them)."""
    seen = {}
    for P, nex, ney, eb, ee in vr.SHAPES:
        s = seen.setdefault(vr.handle_kind(nex, eb, ee), [set() for _ in range(5)])
        for launch in vr.launches(P, nex, ney, eb, ee):
            for f, v in zip(s, launch):
                f.add(v)
    assert set(seen) == {"whole", "first", "middle", "last"}
    for kind, (ncs, lays, masks, descs, cols) in seen.items():
        assert ncs == {0, 1, 2} and lays == {"dense", "condensed"}
        assert masks == set(vr.MASKS) and descs == set(vr.DESCS)
        assert cols >= {"all", "first", "last"} and (("middle" in cols) == (kind in ("whole", "middle")))
    # one thread per row: row counts below, above and not a multiple of the 256-thread block, none above 1500
    rows = [2 * ((ee - eb) * P + 1) * (ney * P + 1) for P, nex, ney, eb, ee in vr.SHAPES]
    assert min(rows) < 256 < max(rows) <= 1500 and any(r % 256 for r in rows if r > 256)
