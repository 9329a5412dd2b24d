"""GPU tests of the line-condensation kernels (sem_amd/csrc/ns_condense.hip), one launch at a time through the C ABI on
synthetic device arrays (tests/condense_reference.py: random blocks in the documented layouts, NaN in every gap and
guard band, the results' arrays full of a sentinel), each launch against the same operation in np.longdouble.

Every launch that consumes an earlier launch's output is checked against the reference evaluated on the values the
device produced (C from the read-back T, the edge values from the read-back C, y_i and Pw from the read-back T and Ye,
g from the read-back Pw), so every bound is a single-launch bound; the derivation is condense_reference's docstring.
Each check asserts SLACK x bound <= 1e-12.  What a call must not write is compared bit for bit, and a second call
must give the same bits.

Which kernel and regime each parameter set reaches:
  REGIMES (nc, P) -> ni       cond_fwd_kernel, cond_fwd_coupled_kernel, cond_back_kernel through colmajor_gemv:
      (1, 2) -> 1             one row, fewer columns than the 4 column splits (empty splits)
      (1, 9) -> 64            the last size of RP = 64 (4 splits)
      (2, 7) -> 72            RP = 128 (2 splits); 2 ne1 = 24
      (2, 9) -> 128           the last size with column splits; 2 ne1 = 32
      (1, 13) -> 144, (2, 10) -> 162    the row loop, one pass
      (2, 13) -> 288, (2, 16) -> 450    the row loop past 256: a thread owns two rows; 2 ne1 = 48, 60 for the second
                              product (Aei, AXB, ABY rows <= 64)
  DENSE_EDGES n_e             cond_edge_kernel: 2 (one partly filled tile), 63, 64, 65 (the tile boundary: a second
                              workgroup of one row), 128, 129
  WIDTHS B = 1..32            cond_edge_thomas_kernel<B>, every instantiation: nc = 1 at P = B + 1 and, for even B,
                              nc = 2 at P = B / 2 + 1 (the edge offsets' (l, c) split); odd B the scalar half-row
                              loads, even B the 16-byte ones; B = 1 (H = 2 > B), the lanes past 2 H that leave early
  CHAINS ney = 1..8           the sweep's ring of depth D = 3 at B = 1, 2, 7, 8, 30: nb = 2 (shorter than the ring:
                              no whole round), every remainder of nb mod 3 and of (nb - 1) mod 3 up to nb = 9
  RT_SWEEP                    cond_edge_thomas_rt_kernel (SEM_TUNE_EDGE_THOMAS = 1) at B = 1, 5, 7, 8, 30, 32
  back_cases()                cond_fwd_coupled_kernel's two products at every regime, then the edge and back kernels
                              with the interface correction of rhs(); nex >= 2 so x_B[e] and x_B[e+1] differ
  IFACE                       cond_iface_part_kernel (interior heights, edge heights, the closing edge; ney = 1: the
                              first element is the last) and cond_iface_sum_kernel (nex = 1: both lines one-sided)
  INTERFACE                   cond_iface_rhs_kernel: m around the 256-thread workgroup, the one-sided lines 0 and nex
Both values of `coupled` run in every sem_nested_solve case (the rhs() correction in K1 and in each edge kernel)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import condense_reference as cr
from condense_reference import CAP, GUARD, SENTINEL, SLACK, Arrays, Case, Device

pytestmark = pytest.mark.gpu


def _lib():
    from sem_amd import _lib as L
    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64)


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
    """Outside `offsets` of each of the `rows` rows (ld apart) the allocation still holds what it started with."""
    raw = dv.raw(name)
    mask = np.zeros(raw.size, dtype=bool)
    for e in range(rows):
        mask[GUARD + e * ld + np.asarray(offsets)] = True
    assert np.array_equal(_bits(raw[~mask]), _bits(dv.initial(name)[~mask])), name


INPUTS = ("Xi", "Aei", "Yie", "XiB", "AXB", "ABY", "pi", "pe", "aIB", "aBI", "xB", "R", "Bl")


def _inputs_unchanged(dv):
    _unchanged(dv, *INPUTS, *(("Ed", "El", "Eu") if dv.c.thomas else ("Se",)))


@functools.lru_cache(maxsize=4)
def _device(P, nex, ney, nc, edge):
    L, _ = _lib()
    return Device(Case.synthetic(P, nex, ney, nc, edge, True), L)


def _call_solve(dv, coupled, back=False):
    L, lib = _lib()
    c = dv.c
    fn = lib.sem_nested_back_solve if back else lib.sem_nested_solve
    st = fn(C.byref(dv.d), dv.ptr("R"), c.ld_r, dv.ptr("aIB") if coupled else None, dv.ptr("xB") if coupled else None,
            dv.ptr("Y"), c.ld_y, _stream())
    torch.cuda.synchronize()
    assert st == L.SEM_OK, _last_error(lib)
    return {k: dv.get(k) for k in ("T", "C", "Ye")} | {k: dv.raw(k) for k in ("Y",)} | {"Yv": dv.get("Y")}


def _start(dv, back):
    c = dv.c
    dv.set("T", c.T0 if back else np.full(c.T0.shape, np.nan))
    dv.set("C", c.C0 if back else np.full(c.C0.shape, np.nan))
    dv.reset("Ye", "Pw", "Y", "g")


def check_solve(dv, coupled, back=False):
    """One sem_nested_solve (or sem_nested_back_solve) call: T, C, Ye and Y launch by launch, what must stay, and a
    second call's bits."""
    c = dv.c
    _start(dv, back)
    o = _call_solve(dv, coupled, back)
    T, Cw, Ye = o["T"], o["C"], o["Ye"]
    if back:
        rT, rC, bT, bC = cr.ref_coupled(c, c.T0, c.C0)
    else:
        rT, bT = cr.ref_T(c, coupled)
        rC, bC = cr.ref_C(c, T)
    _close("T", T, rT, bT)
    _close("C", Cw, rC, bC)
    re, dre = cr.ref_re(c, coupled, Cw)
    rye, bye = cr.ref_edge(c, re, dre)
    _close("Ye", Ye, rye, bye)
    rYi, bYi = cr.ref_Yi(c, T, Ye)
    Yv = o["Yv"]
    _close("Y", Yv[:, c.pi.reshape(-1)], rYi.reshape(c.nex, -1), bYi.reshape(c.nex, -1))
    assert np.array_equal(_bits(Yv[:, c.pe]), _bits(Ye.reshape(c.nex, -1)))
    _only_written(dv, "Y", c.nex, c.ld_y, np.concatenate((c.pi.reshape(-1), c.pe)))
    _inputs_unchanged(dv)
    _unchanged(dv, "Pw", "g")
    _start(dv, back)
    o2 = _call_solve(dv, coupled, back)
    for k in ("T", "C", "Ye", "Y"):
        assert np.array_equal(_bits(o2[k]), _bits(o[k])), k


# ---- sem_nested_solve ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("coupled", [False, True], ids=["plain", "coupled"])
@pytest.mark.parametrize("nc,P", cr.REGIMES)
def test_nested_solve_element_regimes(nc, P, coupled):
    check_solve(_device(P, 2, 2, nc, "thomas"), coupled)


@pytest.mark.parametrize("coupled", [False, True], ids=["plain", "coupled"])
@pytest.mark.parametrize("nc,P,ney", cr.DENSE_EDGES)
def test_nested_solve_dense_edge(nc, P, ney, coupled):
    dv = _device(P, 2, ney, nc, "dense")
    assert dv.c.n_e in (2, 63, 64, 65, 128, 129)
    check_solve(dv, coupled)


@pytest.mark.parametrize("nc,P", cr.WIDTHS)
def test_nested_solve_thomas_widths(nc, P):
    nex, ney = cr.width_nex_ney(nc, P)
    dv = _device(P, nex, ney, nc, "thomas")
    for coupled in (False, True):
        check_solve(dv, coupled)


def test_thomas_widths_are_every_instantiation():
    assert sorted({nc * (P - 1) for nc, P in cr.WIDTHS}) == list(range(1, 33))
    assert sorted(nc * (P - 1) for nc, P in cr.WIDTHS if nc == 2) == list(range(2, 33, 2))


@pytest.mark.parametrize("nc,P,ney", cr.CHAINS)
def test_nested_solve_thomas_chain_lengths(nc, P, ney):
    dv = _device(P, 2, ney, nc, "thomas")
    for coupled in (False, True):
        check_solve(dv, coupled)


@pytest.mark.parametrize("nc,P,ney", cr.RT_SWEEP)
def test_nested_solve_runtime_width_sweep(nc, P, ney):
    """The runtime-width sweep meets the same reference bound as the templated one."""
    L, lib = _lib()
    dv = _device(P, 1 if P > 16 else 2, ney, nc, "thomas")
    L.check(lib.sem_set_tuning(L.TUNE_EDGE_THOMAS, 1))
    try:
        for coupled in (False, True):
            check_solve(dv, coupled)
    finally:
        L.check(lib.sem_set_tuning(L.TUNE_EDGE_THOMAS, 0))
    check_solve(dv, True)


# ---- sem_nested_back_solve -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,nex,ney,nc,edge", cr.back_cases())
def test_nested_back_solve(P, nex, ney, nc, edge):
    assert nex >= 2
    check_solve(_device(P, nex, ney, nc, edge), True, back=True)


# ---- sem_nested_iface_rhs ------------------------------------------------------------------------------------------

def _call_iface(dv):
    L, lib = _lib()
    c = dv.c
    st = lib.sem_nested_iface_rhs(C.byref(dv.d), dv.ptr("R"), c.ld_r, dv.ptr("Bl"), c.ld_b, dv.ptr("aBI"), dv.ptr("Y"),
                                  c.ld_y, dv.ptr("g"), _stream())
    torch.cuda.synchronize()
    assert st == L.SEM_OK, _last_error(lib)
    return {k: dv.get(k) for k in ("T", "C", "Ye", "Pw", "g")} | {"Y": dv.raw("Y"), "Yv": dv.get("Y")}


@pytest.mark.parametrize("nc,P,nex,ney,edge", cr.IFACE)
def test_nested_iface_rhs(nc, P, nex, ney, edge):
    dv = _device(P, nex, ney, nc, edge)
    c = dv.c
    _start(dv, False)
    assert np.all(np.isnan(dv.get("Pw")))
    o = _call_iface(dv)
    T, Cw, Ye, Pw, g = (o[k] for k in ("T", "C", "Ye", "Pw", "g"))
    rT, bT = cr.ref_T(c, False)
    _close("T", T, rT, bT)
    rC, bC = cr.ref_C(c, T)
    _close("C", Cw, rC, bC)
    re, dre = cr.ref_re(c, False, Cw)
    rye, bye = cr.ref_edge(c, re, dre)
    _close("Ye", Ye, rye, bye)
    # Y: the edge offsets only
    assert np.array_equal(_bits(o["Yv"][:, c.pe]), _bits(Ye.reshape(c.nex, -1)))
    _only_written(dv, "Y", c.nex, c.ld_y, c.pe)
    # every entry of Pw: the interior heights, the edge heights and the closing edge tile the line
    rPw, bPw = cr.ref_Pw(c, T, Ye)
    assert rPw.shape == Pw.shape == (c.nex, 2, c.m) and np.all(np.isfinite(rPw.astype(np.float64)))
    _close("Pw", Pw, rPw, bPw)
    rg, bg = cr.ref_g_sum(c, Pw)
    _close("g", g, rg, bg)
    _only_written(dv, "g", 1, 0, np.arange((c.nex + 1) * c.m))
    _inputs_unchanged(dv)
    _start(dv, False)
    o2 = _call_iface(dv)
    for k in ("T", "C", "Ye", "Pw", "g", "Y"):
        assert np.array_equal(_bits(o2[k]), _bits(o[k])), k


# ---- sem_interface_rhs ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,nex,m", cr.INTERFACE)
def test_interface_rhs(P, nex, m):
    L, lib = _lib()
    r = np.random.default_rng(1000 * P + 10 * m + nex)
    nI, ld_b, ld_yI = (P - 1) * m, m + 3, (P - 1) * m + 5
    Bl = np.full((nex * P + 1, ld_b), np.nan)
    Bl[::P, :m] = r.uniform(-1, 1, (nex + 1, m))
    yI = np.full((nex, ld_yI), np.nan)
    yI[:, :nI] = r.uniform(-1, 1, (nex, nI))
    aBI = r.uniform(-1, 1, (nex, 2, P - 1, m))
    dv = Arrays()
    dv.put("Bl", Bl), dv.put("yI", yI), dv.put("aBI", aBI)
    dv.put("g", np.full((nex + 1, m), SENTINEL), guard=SENTINEL)
    ref, bound = cr.ref_interface_rhs(P, nex, m, Bl[::P, :m], aBI, yI[:, :nI])
    outs = []
    for _ in range(2):
        dv.reset("g")
        st = lib.sem_interface_rhs(P, nex, m, dv.ptr("Bl"), ld_b, dv.ptr("aBI"), dv.ptr("yI"), ld_yI, dv.ptr("g"),
                                   _stream())
        torch.cuda.synchronize()
        assert st == L.SEM_OK, _last_error(lib)
        outs.append(dv.raw("g"))
    _close("g", dv.get("g"), ref, bound)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    assert np.array_equal(_bits(outs[0][:GUARD]), _bits(np.full(GUARD, SENTINEL)))
    assert np.array_equal(_bits(outs[0][-GUARD:]), _bits(np.full(GUARD, SENTINEL)))
    _unchanged(dv, "Bl", "yI", "aBI")


# ---- status codes --------------------------------------------------------------------------------------------------

OUTPUTS = ("T", "C", "Ye", "Pw", "Y", "g")


def _copy_desc(L, d, **fields):
    n = L.SemNestedDesc()
    C.memmove(C.byref(n), C.byref(d), C.sizeof(d))
    for k, v in fields.items():
        setattr(n, k, v)
    return n


def _refused(dv, entry, want, drop=(), **fields):
    """The call with the descriptor fields replaced and the arguments in `drop` null returns `want` with a message
    and writes nothing."""
    L, lib = _lib()
    c = dv.c
    _start(dv, False)
    d = fields.pop("desc", "copy")
    dref = None if d is None else C.byref(_copy_desc(L, dv.d, **fields))
    a = {k: (None if k in drop else dv.ptr(k)) for k in ("R", "aIB", "xB", "Y", "Bl", "aBI", "g")}
    if entry == "iface":
        st = lib.sem_nested_iface_rhs(dref, a["R"], c.ld_r, a["Bl"], c.ld_b, a["aBI"], a["Y"], c.ld_y, a["g"],
                                      _stream())
    else:
        fn = lib.sem_nested_back_solve if entry == "back" else lib.sem_nested_solve
        st = fn(dref, a["R"], c.ld_r, a["aIB"], a["xB"], a["Y"], c.ld_y, _stream())
    torch.cuda.synchronize()
    assert st == want, (entry, drop, fields, st)
    assert _last_error(lib) != ""
    with pytest.raises(ValueError if want == L.SEM_EINVAL else RuntimeError):
        L.check(st)
    _unchanged(dv, *OUTPUTS)


def test_argument_checks():
    """Every bad call returns SEM_EINVAL with a message, before any launch: nothing is written."""
    L, _ = _lib()
    E = L.SEM_EINVAL
    th, de = _device(3, 2, 2, 2, "thomas"), _device(3, 2, 2, 2, "dense")
    plain = ("aIB", "xB")                       # sem_nested_solve without the interface correction
    for dv in (th, de):
        for entry, base in (("solve", plain), ("solve", ()), ("back", ()), ("iface", ())):
            _refused(dv, entry, E, base, desc=None)
            _refused(dv, entry, E, base + ("R",))
            _refused(dv, entry, E, base + ("Y",))
            _refused(dv, entry, E, base, P=1, NY=dv.c.ney + 1)
            _refused(dv, entry, E, base, nc=3)
            _refused(dv, entry, E, base, NY=dv.c.NY + 1)
            _refused(dv, entry, E, base, nex=0)
            _refused(dv, entry, E, base, ney=0, NY=1)
            for k in ("Xi", "Aei", "Yie", "pi", "pe", "T", "C", "Ye"):
                _refused(dv, entry, E, base, **{k: None})
        _refused(dv, "solve", E, ("xB",))        # aIB without xB
        _refused(dv, "solve", E, ("aIB",))
        _refused(dv, "back", E, ("aIB", "xB"))
        _refused(dv, "back", E, ("aIB",))
        _refused(dv, "back", E, ("xB",))
        _refused(dv, "back", E, XiB=None)
        _refused(dv, "back", E, AXB=None)
        _refused(dv, "iface", E, ABY=None)
        _refused(dv, "iface", E, Pw=None)
        for k in ("Bl", "aBI", "g"):
            _refused(dv, "iface", E, (k,))
    _refused(de, "solve", E, plain, Se=None)     # neither Se nor Ed
    _refused(th, "solve", E, plain, Ed=None)
    _refused(th, "solve", E, plain, El=None)
    _refused(th, "solve", E, plain, Eu=None)


def test_unsupported_sizes_are_refused_before_any_launch():
    """ne1 = 33 in the block-Thomas form and a dense Se whose n_e + 256 doubles exceed 64 KiB of LDS: both refused by
    the shared argument check, so the small allocations are never read."""
    L, _ = _lib()
    U = L.SEM_EUNSUPPORTED
    th, de = _device(3, 2, 2, 2, "thomas"), _device(3, 2, 2, 2, "dense")
    for entry, base in (("solve", ("aIB", "xB")), ("solve", ()), ("back", ()), ("iface", ())):
        _refused(th, entry, U, base, P=34, nc=1, NY=2 * 34 + 1)              # ne1 = 33
        _refused(th, entry, U, base, P=18, nc=2, NY=2 * 18 + 1)              # ne1 = 34
        # n_e = (ney + 1) 32 = 7968: (7968 + 256) 8 bytes = 65792 > 65536
        _refused(de, entry, U, base, P=17, nc=2, ney=248, NY=248 * 17 + 1)


def test_interface_rhs_argument_checks():
    L, lib = _lib()
    dv = Arrays()
    dv.put("a", np.ones(64))
    dv.put("g", np.full(64, SENTINEL), guard=SENTINEL)
    a, g = dv.ptr("a"), dv.ptr("g")
    for args in ((1, 2, 4, a, 4, a, a, 4, g), (2, 0, 4, a, 4, a, a, 4, g), (2, 2, 0, a, 4, a, a, 4, g),
                 (2, 2, -1, a, 4, a, a, 4, g), (2, 2, 4, None, 4, a, a, 4, g), (2, 2, 4, a, 4, None, a, 4, g),
                 (2, 2, 4, a, 4, a, None, 4, g), (2, 2, 4, a, 4, a, a, 4, None)):
        assert lib.sem_interface_rhs(*args, _stream()) == L.SEM_EINVAL, args
        assert _last_error(lib) != ""
    torch.cuda.synchronize()
    _unchanged(dv, "g", "a")
