"""GPU tests of velocity_blocks_kernel (sem_amd/csrc/ns_velocity.hip), the assembly every device direct solve starts
from, one launch at a time through the C ABI (sem_velocity_blocks, sem_condensed_blocks and the three size functions)
on handles from sem_amd.device.get_mesh, entry by entry against tests/velocity_reference.py (np.longdouble, pinned to
the oracle, to ns_reference and to the CPU mesh by tests/test_velocity_reference.py; the bound is derived in its
docstring: L = 13 roundings on the sum of absolute terms, T = 2 (P + 2) more on the stiffness terms for the two
evaluations of the K_s table, SLACK = 2).

Every piece lies in a buffer full of a sentinel with guard bands before and after it, A_II and the condensed pieces
with room for one element column more than the call writes.  Per launch: the status; every entry of every piece
finite and inside its bound, or == 0 / 1 / the operand's bits where the reference says exact; guard bands and the
spare column bit for bit untouched; a second call into fresh sentinels gives the same bits; the interface pieces D,
aIB, aBI, E, F agree bit for bit between the dense and the condensed call and between column ranges, as do the
blocks of one element column written under different ranges, and ncomp = 0 gives the bits of ncomp = 2.

Shapes (velocity_reference.SHAPES) are the smallest at which each path exists; velocity_reference.launches picks, per
shape, every value of every factor -- ncomp 0 / 1 / 2, dense / condensed, the seven masks, the seven descriptors, the
column ranges -- from a base launch and 14 rotated combinations.  The operands are all-distinct uniform(-1, 1) fields,
dx != dy, four coefficients of different size and sign with c_mass != 0.  Each shape prints its largest ratio to the
first-order bound on a VBRATIO line and beside it, for the record and never asserted, the ratio to L mag alone: what
the comparison would give without the allowance for the two evaluations of the K_s table."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import velocity_reference as vr
from condense_reference import Arrays
from velocity_reference import COND, DENSE, DX, DY, FIELDS, IFACE, SENTINEL, SLACK, Case

pytestmark = pytest.mark.gpu


def _lib():
    from sem_amd import _lib as L
    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _handle(P, nex, ney, eb, ee):
    from sem_amd.device import get_mesh
    mesh = get_mesh(P, nex, ney, DX, DY, eb, ee)
    assert (mesh.n_local, mesh.NY, mesh.ex_begin, mesh.ex_end) == ((ee - eb) * P * (ney * P + 1) + ney * P + 1,
                                                                 ney * P + 1, eb, ee)
    return mesh


class _Shape:
    """One handle, its operand fields and masks on the device, and what earlier launches wrote (for the bitwise
    agreement between layouts, column ranges and ncomp 0 / 2)."""

    def __init__(self, P, nex, ney, eb, ee):
        self.geo = (P, nex, ney, eb, ee)
        self.mesh = _handle(*self.geo)
        base = Case(*self.geo)
        self.ops = Arrays()
        for k in FIELDS:
            self.ops.put(k, base.fields[k])
        for k in ("perimeter", "irregular"):
            self.ops.put(k, vr.mask_of(k, *self.geo)[0], guard=1)
        self.cases, self.iface, self.blocks, self.partners = {}, {}, {}, {}
        self.worst, self.plain, self.count = 0.0, 0.0, 0

    def case(self, nc, desc, mask, cols):
        key = (nc, desc, mask)
        if key not in self.cases:
            self.cases[key] = Case(*self.geo, nc=nc, desc=desc, mask=mask)
            vr.dense_jacobian(self.cases[key])
        c = copy.copy(self.cases[key])          # shares the dense reference
        c.cols = cols
        return c

    def descriptor(self, c, ncomp, whole=False):
        L, _ = _lib()
        p = lambda k: self.ops.ptr(k) if c.f[k] is not None else None   # noqa: E731
        mask = self.ops.ptr(c.mask) if c.dir_mask is not None else None
        cb, ce = (0, 0) if whole else c.cols     # (0, 0): the handle's whole strip
        return L.SemVelocityDesc(c.coef["c_mass"], c.coef["c_stiff"], c.coef["c_gradx"], c.coef["c_grady"],
                                 *(p(k) for k in FIELDS), mask, c.dir_sides, ncomp, cb, ce)


def _outputs(c, layout):
    """Sentinel-filled device buffers of every piece; A_II and the condensed pieces with one spare column."""
    out = Arrays()
    used = c.shapes(layout)
    for k, s in c.shapes(layout, ncols=c.cols[1] - c.cols[0] + 1).items():
        out.put(k, np.full(s, SENTINEL), guard=SENTINEL)
    return out, used


def _call(sh, c, layout, ncomp, out, whole=False):
    L, lib = _lib()
    d = sh.descriptor(c, ncomp, whole)
    q = lambda k: out.ptr(k) if out.host[k][0].size > 2 * vr.GUARD else None   # noqa: E731  P = 1: no such piece
    if layout == "dense":
        st = lib.sem_velocity_blocks(sh.mesh._h, C.byref(d), *(q(k) for k in DENSE), _stream())
    else:
        st = lib.sem_condensed_blocks(sh.mesh._h, C.byref(d), *(q(k) for k in COND + IFACE), _stream())
    torch.cuda.synchronize()
    assert st == L.SEM_OK, lib.sem_last_error().decode(errors="replace")
    return {k: out.raw(k) for k in out.bufs}


def check_launch(sh, ncomp, layout, mask, desc, colname):
    P, nex, ney, eb, ee = sh.geo
    nc = ncomp or 2
    cols = vr.column_ranges(eb, ee)[colname]
    c = sh.case(nc, desc, mask, cols)
    tag = (ncomp, layout, mask, desc, colname)
    out, used = _outputs(c, layout)
    whole = colname == "all"                # col_begin = col_end = 0; the other ranges are given explicitly
    raw = _call(sh, c, layout, ncomp, out, whole)
    got = {}
    sent = _bits(np.array([SENTINEL]))[0]
    for k, s in used.items():
        n = int(np.prod(s))
        r = raw[k]
        got[k] = r[vr.GUARD:vr.GUARD + n].reshape(s)
        rest = np.concatenate((r[:vr.GUARD], r[vr.GUARD + n:]))
        assert rest.size >= 2 * vr.GUARD and np.all(_bits(rest) == sent), (tag, k, "written outside the piece")
    if P > 1:
        spare = DENSE[:1] if layout == "dense" else COND
        assert all(raw[k].size - 2 * vr.GUARD > got[k].size for k in spare)
    ref = vr.reference(c, layout)
    worst, fails = vr.compare(got, ref, P)
    assert not fails, (tag, fails)
    assert worst <= SLACK
    sh.worst, sh.count = max(sh.worst, worst), sh.count + 1
    sh.plain = max(sh.plain, vr.plain_ratio(got, ref))
    # a second call into fresh sentinels
    out.reset(*out.bufs)
    again = _call(sh, c, layout, ncomp, out, whole)
    for k in raw:
        assert np.array_equal(_bits(raw[k]), _bits(again[k])), (tag, k, "not reproducible")
    # the same bits whatever the layout, the column range and ncomp 0 or 2, and for the perimeter as a mask or as sides
    mask = "sides15" if mask == "perimeter" else mask
    sh.partners.setdefault((nc, mask, desc), set()).add(tag)
    seen = sh.iface.setdefault((nc, mask, desc), {})
    for k in IFACE:
        if k in seen:
            assert np.array_equal(_bits(got[k]), seen[k][1]), (tag, k, "differs from launch", seen[k][0])
        else:
            seen[k] = (tag, _bits(got[k]).copy())
    for k in (DENSE[:1] if layout == "dense" else COND):
        for i, col in enumerate(range(*cols)):
            key = (nc, mask, desc, k, col)
            b = _bits(got[k][i])
            if key in sh.blocks:
                assert np.array_equal(b, sh.blocks[key][1]), (tag, k, col, "differs from launch", sh.blocks[key][0])
            else:
                sh.blocks[key] = (tag, b.copy())
    return worst


@pytest.mark.parametrize("P,nex,ney,eb,ee", vr.SHAPES)
def test_every_entry_of_every_piece(gpu, P, nex, ney, eb, ee):
    sh = _Shape(P, nex, ney, eb, ee)
    todo = vr.launches(P, nex, ney, eb, ee)
    for launch in todo:
        check_launch(sh, *launch)
    assert sh.count == len(todo)
    # the bitwise agreement met its partners: the base operands under ncomp 0 and 2, every layout and every column
    # range; the perimeter as dir_sides = 15 and as a mask
    base = sh.partners[(2, "irregular", "full")]
    assert {t[0] for t in base} == {0, 2} and {t[4] for t in base} == set(vr.column_ranges(eb, ee))
    assert {t[1] for t in base} == ({"dense", "condensed"} if P > 1 else {"dense"})
    assert {t[2] for t in sh.partners[(2, "sides15", "full")]} == {"sides15", "perimeter"}
    print("VBRATIO", f"P={P} nex={nex} ney={ney} strip=[{eb},{ee}) {vr.handle_kind(nex, eb, ee)}",
          f"launches={sh.count} worst={sh.worst:.3f} without-table-allowance={sh.plain:.3f}")


# ---- the size functions --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,nex,ney,eb,ee", vr.SHAPES)
def test_size_functions_equal_the_header_formulas(gpu, P, nex, ney, eb, ee):
    L, lib = _lib()
    h = _handle(P, nex, ney, eb, ee)._h
    ne, NY = ee - eb, ney * P + 1
    for nc in (1, 2):
        m = nc * NY
        nI = (P - 1) * m
        s = (C.c_int64 * 6)(*[-1] * 6)
        assert lib.sem_line_block_sizes(h, nc, s) == L.SEM_OK
        assert list(s) == [ne * nI * nI, (ne + 1) * m * m, ne * (P - 1) * 2 * m, ne * 2 * (P - 1) * m, ne * m, ne * m]
        assert list(s) == [int(np.prod(x)) for x in Case(P, nex, ney, eb, ee, nc=nc).shapes("dense").values()]
        if nc == 2:
            s2 = (C.c_int64 * 6)(*[-1] * 6)
            assert lib.sem_velocity_block_sizes(h, s2) == L.SEM_OK and list(s2) == list(s)
        cs = (C.c_int64 * 6)(*[-1] * 6)
        if P == 1:
            assert lib.sem_condensed_block_sizes(h, nc, cs) == L.SEM_EINVAL and list(cs) == [-1] * 6
            continue
        ne1 = nc * (P - 1)
        ni = ne1 * (P - 1)
        assert lib.sem_condensed_block_sizes(h, nc, cs) == L.SEM_OK
        assert list(cs) == [ney * ni * ni, ney * ni * 2 * ne1, ney * 2 * ne1 * ni, (ney + 1) * ne1 * ne1,
                            ney * ne1 * ne1, ney * ne1 * ne1]
        per_column = list(Case(P, nex, ney, eb, ee, nc=nc).shapes("condensed", ncols=1).values())[:6]
        assert list(cs) == [int(np.prod(x)) for x in per_column]


# ---- refusals ------------------------------------------------------------------------------------------------------

def _refusal_setup(geo, nc=2):
    sh = _Shape(*geo)
    c = sh.case(nc, "full", "irregular", (geo[3], geo[4]))
    outs = {}
    for layout in ("dense", "condensed") if geo[0] > 1 else ("dense",):
        outs[layout] = _outputs(c, layout)[0]
    return sh, c, outs


def _refused(sh, c, out, layout, drop=(), h="handle", desc="desc", **fields):
    """The call with the arguments in `drop` null and the descriptor fields replaced returns SEM_EINVAL with a
    message, before any write."""
    L, lib = _lib()
    d = sh.descriptor(c, c.nc)
    for k, v in fields.items():
        setattr(d, k, sh.ops.ptr(v) if isinstance(v, str) else v)
    q = lambda k: None if k in drop or out.host[k][0].size <= 2 * vr.GUARD else out.ptr(k)   # noqa: E731
    hh = sh.mesh._h if h == "handle" else None
    dd = C.byref(d) if desc == "desc" else None
    if layout == "dense":
        st = lib.sem_velocity_blocks(hh, dd, *(q(k) for k in DENSE), _stream())
    else:
        st = lib.sem_condensed_blocks(hh, dd, *(q(k) for k in COND + IFACE), _stream())
    torch.cuda.synchronize()
    assert st == L.SEM_EINVAL, (layout, drop, fields, st)
    assert lib.sem_last_error().decode(errors="replace") != ""
    with pytest.raises(ValueError):
        L.check(st)
    for k in out.bufs:
        assert np.array_equal(_bits(out.raw(k)), _bits(out.initial(k))), (layout, drop, fields, k)


def test_refusals_write_nothing(gpu):
    L, lib = _lib()
    sh, c, outs = _refusal_setup((2, 3, 2, 1, 2))        # a one-column strip of a three-column mesh
    for layout, out in outs.items():
        _refused(sh, c, out, layout, h=None)
        _refused(sh, c, out, layout, desc=None)
        for k in ("D", "E", "F", "aIB", "aBI") + (("AII",) if layout == "dense" else COND):
            _refused(sh, c, out, layout, drop=(k,))
        _refused(sh, c, out, layout, ncomp=3)
        _refused(sh, c, out, layout, ncomp=-1)
        for cb, ce in ((0, 2), (1, 3), (1, 1), (2, 1), (2, 2), (0, 1)):
            _refused(sh, c, out, layout, col_begin=cb, col_end=ce)
    sh1, c1, outs1 = _refusal_setup((2, 3, 2, 1, 2), nc=1)
    for layout, out in outs1.items():
        for k in ("juv", "jvu", "jvv"):
            _refused(sh1, c1, out, layout, ncomp=1, **{k: k})
    # P = 1: D, E, F are still required; the condensed layout does not exist
    shp, cp, outp = _refusal_setup((1, 3, 2, 0, 3))
    for k in ("D", "E", "F"):
        _refused(shp, cp, outp["dense"], "dense", drop=(k,))
    d = shp.descriptor(cp, 2)
    a = outp["dense"]
    st = lib.sem_condensed_blocks(shp.mesh._h, C.byref(d), *[a.ptr("D")] * 6, a.ptr("D"), None, None, a.ptr("E"),
                                  a.ptr("F"), _stream())
    torch.cuda.synchronize()
    assert st == L.SEM_EINVAL and lib.sem_last_error().decode(errors="replace") != ""
    for k in a.bufs:
        assert np.array_equal(_bits(a.raw(k)), _bits(a.initial(k)))
    # the size functions
    s = (C.c_int64 * 6)(*[-1] * 6)
    assert lib.sem_condensed_block_sizes(shp.mesh._h, 2, s) == L.SEM_EINVAL
    for h in (sh.mesh._h, None):
        for sizes in ((None,) if h is not None else (None, s)):
            assert lib.sem_line_block_sizes(h, 2, sizes) == L.SEM_EINVAL
            assert lib.sem_velocity_block_sizes(h, sizes) == L.SEM_EINVAL
            assert lib.sem_condensed_block_sizes(h, 2, sizes) == L.SEM_EINVAL
            assert lib.sem_last_error().decode(errors="replace") != ""
    assert list(s) == [-1] * 6
