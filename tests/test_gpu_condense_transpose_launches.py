"""GPU tests of the transposed line-condensation kernels, one launch at a time through the C ABI on synthetic device
arrays: sem_nested_solve_t (sem_amd/csrc/ns_condense_transpose.hip) and sem_block_gemv_t (sem_amd/csrc/block_gemv.hip),
each launch against the same operation in np.longdouble (tests/condense_reference_T.py, which derives the bounds).

sem_nested_solve_t's three launches are checked as tests/test_gpu_condense_launches.py checks the forward ones: C
against the reference, the edge values against the reference sweep run on the reduced right-hand side formed from
the device's C, y_i against the reference evaluated on the device's edge values, so every bound is a single-launch
bound; each check asserts SLACK x bound <= 1e-12.  Guard bands and everything a call must not write (the gaps of Y,
the work array T, the inputs) are compared bit for bit, and a second call must give the same bits.

Which kernel and regime each parameter set reaches:
  REGIMES (nc, P) -> ni, 2 ne1   cond_fwd_t_kernel and cond_back_t_kernel through rows_dot_l, L lanes per stored row:
      (1, 2) -> 1, 2             L = 4, one element per row (idle lanes), odd ni: the 8-byte loads
      (1, 9) -> 64, 16           rows of 64 at L = 16, of 16 at L = 4; even ni: the 16-byte loads
      (2, 7) -> 72, 24           L = 32 and 8;   (2, 9) -> 128, 32: L = 32 (the last) and 8 (the last)
      (1, 13) -> 144, 24         L = 64: more than two elements per lane;   (2, 10) -> 162, 36: L = 16 for Aei
      (2, 13) -> 288, 48         more rows than one pass of 256 / L;   (2, 16) -> 450, 60
  WIDTHS B = 1..32               cond_edge_thomas_t_kernel<B>, every instantiation (ni = 1024 at B = 32, nc = 1: the
                                 longest rows, odd and even ni)
  CHAINS ney = 1..8              the sweep's ring of depth 3 at B = 1, 2, 7, 8, 30: chains of 2..9 edges
Both values of `coupled` run in every case (rhs() with aBIt in K1t, K2t and K3t)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import condense_reference as cr
import condense_reference_T as crt
from condense_reference import CAP, GUARD, SENTINEL, SLACK, Arrays, Device

pytestmark = pytest.mark.gpu


def _lib():
    from sem_amd import _lib as L
    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _last_error(lib):
    return lib.sem_last_error().decode(errors="replace")


_WORST = {}


def _close(name, got, ref, bound):
    """got within SLACK x bound of ref everywhere, and the bound is not vacuous."""
    assert np.all(np.isfinite(got)), name
    assert SLACK * float(np.max(bound)) <= CAP, (name, float(np.max(bound)))
    ratio = cr.worst(got, ref, bound)
    _WORST[name] = max(_WORST.get(name, 0.0), ratio)
    assert cr.within(got, ref, bound), (name, ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    """With -s: the largest |got - ref| / bound of every output over the module (allowed: SLACK)."""
    yield
    print("\nlargest |got - ref| / bound, allowed %g: " % SLACK
          + ", ".join("%s %.3f" % kv for kv in sorted(_WORST.items())))


def _unchanged(dv, *names):
    for k in names:
        assert np.array_equal(_bits(dv.raw(k)), _bits(dv.initial(k))), k


def _only_written(dv, name, rows, ld, offsets):
    raw = dv.raw(name)
    mask = np.zeros(raw.size, dtype=bool)
    for e in range(rows):
        mask[GUARD + e * ld + np.asarray(offsets)] = True
    assert np.array_equal(_bits(raw[~mask]), _bits(dv.initial(name)[~mask])), name


INPUTS = ("Xi", "Aei", "Yie", "Ed", "El", "Eu", "pi", "pe", "aIB", "xB", "R")
OUTPUTS = ("T", "C", "Ye", "Pw", "Y", "g")


@functools.lru_cache(maxsize=4)
def _device(P, nex, ney, nc):
    L, _ = _lib()
    return Device(crt.synthetic_t(P, nex, ney, nc, True), L)     # its "aIB" array is aBIt


def _start(dv):
    dv.reset(*OUTPUTS)


def _call(dv, coupled):
    L, lib = _lib()
    c = dv.c
    st = lib.sem_nested_solve_t(C.byref(dv.d), dv.ptr("R"), c.ld_r, dv.ptr("aIB") if coupled else None,
                                dv.ptr("xB") if coupled else None, dv.ptr("Y"), c.ld_y, _stream())
    torch.cuda.synchronize()
    assert st == L.SEM_OK, _last_error(lib)
    return {k: dv.get(k) for k in ("C", "Ye")} | {"Y": dv.raw("Y"), "Yv": dv.get("Y")}


def check_solve_t(dv, coupled):
    c = dv.c
    _start(dv)
    o = _call(dv, coupled)
    Cw, Ye, Yv = o["C"], o["Ye"], o["Yv"]
    rC, bC = crt.ref_Ct(c, coupled)
    _close("C", Cw, rC, bC)
    re, dre = cr.ref_re(c, coupled, Cw)
    rye, bye = crt.ref_edge_t(c, re, dre)
    _close("Ye", Ye, rye, bye)
    rYi, bYi = crt.ref_Yi_t(c, coupled, Ye)
    _close("Y", Yv[:, c.pi.reshape(-1)], rYi.reshape(c.nex, -1), bYi.reshape(c.nex, -1))
    assert np.array_equal(_bits(Yv[:, c.pe]), _bits(Ye.reshape(c.nex, -1)))
    _only_written(dv, "Y", c.nex, c.ld_y, np.concatenate((c.pi.reshape(-1), c.pe)))
    _unchanged(dv, *INPUTS)
    _unchanged(dv, "T", "Pw", "g")                    # T is not a work array of the transposed solve
    _start(dv)
    o2 = _call(dv, coupled)
    for k in ("C", "Ye", "Y"):
        assert np.array_equal(_bits(o2[k]), _bits(o[k])), k


@pytest.mark.parametrize("coupled", [False, True], ids=["plain", "coupled"])
@pytest.mark.parametrize("nc,P", cr.REGIMES)
def test_nested_solve_t_element_regimes(nc, P, coupled):
    check_solve_t(_device(P, 2, 2, nc), coupled)


@pytest.mark.parametrize("nc,P", cr.WIDTHS)
def test_nested_solve_t_thomas_widths(nc, P):
    nex, ney = cr.width_nex_ney(nc, P)
    dv = _device(P, nex, ney, nc)
    for coupled in (False, True):
        check_solve_t(dv, coupled)


@pytest.mark.parametrize("nc,P,ney", cr.CHAINS)
def test_nested_solve_t_thomas_chain_lengths(nc, P, ney):
    dv = _device(P, 2, ney, nc)
    for coupled in (False, True):
        check_solve_t(dv, coupled)


def test_shapes_are_the_ones_the_bounds_were_capped_at():
    run = {(P, 2, 2, nc) for nc, P in cr.REGIMES} | {(P,) + cr.width_nex_ney(nc, P) + (nc,) for nc, P in cr.WIDTHS} \
        | {(P, 2, ney, nc) for nc, P, ney in cr.CHAINS}
    assert run == set(crt.solve_cases_t())
    assert max(nc * (P - 1) ** 2 for P, _, _, nc in run) == 1024


def _copy_desc(L, d, **fields):
    n = L.SemNestedDesc()
    C.memmove(C.byref(n), C.byref(d), C.sizeof(d))
    for k, v in fields.items():
        setattr(n, k, v)
    return n


def _refused(dv, want, drop=(), **fields):
    """The call with the descriptor fields replaced and the arguments in `drop` null returns `want` with a message
    and writes nothing."""
    L, lib = _lib()
    c = dv.c
    _start(dv)
    d = fields.pop("desc", "copy")
    dref = None if d is None else C.byref(_copy_desc(L, dv.d, **fields))
    a = {k: (None if k in drop else dv.ptr(k)) for k in ("R", "aIB", "xB", "Y")}
    st = lib.sem_nested_solve_t(dref, a["R"], c.ld_r, a["aIB"], a["xB"], a["Y"], c.ld_y, _stream())
    torch.cuda.synchronize()
    assert st == want, (drop, fields, st)
    assert _last_error(lib) != ""
    with pytest.raises(ValueError if want == L.SEM_EINVAL else RuntimeError):
        L.check(st)
    _unchanged(dv, *OUTPUTS)


def test_nested_solve_t_refusals():
    """Every refusal of the header, each before any launch (nothing is written): the dense edge inverse, ne1 > 32,
    null pointers and bad sizes."""
    L, _ = _lib()
    E, U = L.SEM_EINVAL, L.SEM_EUNSUPPORTED
    dv = _device(3, 2, 2, 2)
    plain = ("aIB", "xB")
    for base in (plain, ()):
        _refused(dv, U, base, Se=dv.ptr("Ed"))                              # a dense edge inverse: the torch path
        _refused(dv, U, base, P=34, nc=1, NY=2 * 34 + 1)                    # ne1 = 33
        _refused(dv, U, base, P=18, nc=2, NY=2 * 18 + 1)                    # ne1 = 34
        _refused(dv, E, base, desc=None)
        _refused(dv, E, base + ("R",))
        _refused(dv, E, base + ("Y",))
        _refused(dv, E, base, P=1, NY=dv.c.ney + 1)
        _refused(dv, E, base, nc=3)
        _refused(dv, E, base, NY=dv.c.NY + 1)
        _refused(dv, E, base, nex=0)
        _refused(dv, E, base, ney=0, NY=1)
        for k in ("Xi", "Aei", "Yie", "pi", "pe", "T", "C", "Ye", "Ed", "El", "Eu"):
            _refused(dv, E, base, **{k: None})
    _refused(dv, E, ("xB",))                                                # aBIt without xB
    _refused(dv, E, ("aIB",))


# ---- sem_block_gemv_t ----------------------------------------------------------------------------------------------------

class GemvDevice(Arrays):
    def __init__(self, g):
        super().__init__()
        self.g = g
        self.put("M", g.M)
        for s in range(g.S):
            self.put("src%d" % s, g.src[s])
        self.put("mblk", g.mblk, guard=-1), self.put("xrow", g.xrow, guard=-1), self.put("yrow", g.yrow, guard=0)
        y0 = np.full((g.ny, g.ld_y), SENTINEL)
        y0[:, :] = g.y0
        y0[:, g.m:] = SENTINEL                       # the gap between output rows
        self.put("y", y0, guard=SENTINEL)

    def call(self, form=0, **over):
        L, lib = _lib()
        g = self.g
        P = C.c_void_p
        a = dict(nb=g.nb, m=g.m, S=g.S, W=g.W, M=self.ptr("M"), mcol=(C.c_int * g.S)(*g.mcol), mblk=self.ptr("mblk"),
                 src=(P * g.S)(*(P(self.ptr("src%d" % s)) for s in range(g.S))),
                 ld=(C.c_int64 * g.S)(*g.ld_src), xrow=self.ptr("xrow"), y=self.ptr("y"), ld_y=g.ld_y,
                 yrow=self.ptr("yrow"), acc=g.accumulate, form=form)
        a.update(over)
        st = lib.sem_block_gemv_t(a["nb"], a["m"], a["S"], a["W"], a["M"], a["mcol"], a["mblk"], a["src"], a["ld"],
                                  a["xrow"], a["y"], a["ld_y"], a["yrow"], a["acc"], a["form"], _stream())
        torch.cuda.synchronize()
        return st


def check_gemv_t(g, form):
    L, lib = _lib()
    dv = GemvDevice(g)
    ref, bound = crt.ref_block_gemv_t(g)
    outs = []
    for _ in range(2):
        dv.reset("y")
        assert dv.call(form) == L.SEM_OK, _last_error(lib)
        outs.append(dv.raw("y"))
    y = dv.get("y")
    _close("gemv_t form %d" % form, y[g.yrow, :g.m], ref, bound)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    _only_written(dv, "y", 1, 0, (g.yrow[:, None] * g.ld_y + np.arange(g.m)[None, :]).reshape(-1))
    _unchanged(dv, "M", "mblk", "xrow", "yrow", *("src%d" % s for s in range(g.S)))


@pytest.mark.parametrize("form", [1, 2], ids=["wide", "narrow"])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, 513])
def test_block_gemv_t(m, accumulate, form):
    """Every S and W at one block and at three (with absent terms either way: mblk = -1, xrow = -1), both kernel
    forms, ld_y > m and operand rows with their own leading dimensions."""
    for nb, S, W in ((1, 1, 1), (3, 2, 2), (3, 3, 3), (1, 2, 3), (3, 1, 2), (3, 3, 1)):
        check_gemv_t(crt.GemvTCase(m, nb, S, W, seed=7, accumulate=accumulate), form)


def test_block_gemv_t_by_size_takes_both_forms():
    """form = 0 picks the wide form from ceil(m / 64) nb >= 256 on: its bits are the wide form's there and the narrow
    form's below."""
    L, lib = _lib()
    for nb, want in ((128, 1), (127, 2)):                       # m = 65: two 64-column tiles per block
        g = crt.GemvTCase(65, nb, 2, 3, seed=nb, accumulate=1)
        ref, bound = crt.ref_block_gemv_t(g)
        dv = GemvDevice(g)
        bits = {}
        for form in (0, 1, 2):
            dv.reset("y")
            assert dv.call(form) == L.SEM_OK, _last_error(lib)
            bits[form] = dv.raw("y")
            _close("gemv_t by size", dv.get("y")[g.yrow, :g.m], ref, bound)
        assert np.array_equal(_bits(bits[0]), _bits(bits[want]))


def test_block_gemv_t_argument_checks():
    L, lib = _lib()
    E, U = L.SEM_EINVAL, L.SEM_EUNSUPPORTED
    g = crt.GemvTCase(5, 2, 2, 3, seed=1)
    dv = GemvDevice(g)
    dv.reset("y")
    bad = [dict(nb=-1), dict(m=0), dict(S=0), dict(S=4), dict(W=0), dict(W=4), dict(form=3), dict(form=-1),
           dict(M=None), dict(mcol=None), dict(mblk=None), dict(src=None), dict(ld=None), dict(xrow=None), dict(y=None),
           dict(yrow=None), dict(mcol=(C.c_int * 2)(0, 3)), dict(mcol=(C.c_int * 2)(-1, 0)),
           dict(src=(C.c_void_p * 2)(C.c_void_p(dv.ptr("src0")), None))]
    for over in bad:
        assert dv.call(**over) == E, over
        assert _last_error(lib) != ""
    assert dv.call(0, m=4097) == U                              # S m = 8194 > 8192: the caller's batched product
    assert dv.call(0, S=1, m=8193) == U
    assert dv.call(0, nb=0) == L.SEM_OK
    _unchanged(dv, "y")
