"""GPU tests of sem_ns_apply_transpose (sem_amd/csrc/ns_apply_transpose.hip) one launch at a time through
Mesh.ns_apply_transpose on synthetic device arrays, against tests/ns_reference_T.py (np.longdouble, pinned to
ns_reference by tests/test_ns_reference_T.py): every order P = 1..16 at the three y tilings around a tile edge and on
a 1 x 1 mesh, the forms the solvers launch, and the descriptor's contract (Dirichlet sides and masks, pins, line
views, absent inputs and outputs), plus the refusals the header lists.

Bound per row, derived from the kernel's code, not measured:  |got_r - ref_r| <= SLACK L 2^-53 (|A^T| |z|)_r  with
(|A^T| |z|)_r from ns_reference_T(absval=True) -- the absolute terms in the kernel's form G^T = -G + b -- and L the
longest chain of roundings a term of a row goes through.  The longest is a stiffness term of yu (yv alike) at an
element corner:

  * 4 for its Sys coefficient: c_stiff (dy / dx) on the host (2), fKx K (1), fma(-fX cu, G, fKx K) (1)  (the convection
    part has 3: c_gradx (dy / 2), -fX cu, the fma);
  * 2 (P + 1) for the sum: the x rows of a node run the left element's P + 1 fused multiply-adds and then the right
    element's into one accumulator; the y rows have an accumulator of their own (the same length);
  * 3 to join the directions: the assembled weight My = w_P + w_0, Mx Suy, fma(My, Sux, Mx Suy);
  * 5 to finish the row: fma(pm, z'_u, .) (mass and boundary-line coefficient), juu, jvu, the G_x^T w term, + m zu;
  * 2 because the kernel's compile-time GLL constants may differ from the oracle's tables in the last place (one
    unit in the last place of a coefficient is up to 2^-52 of it);
  * 2 because the forward row entry -G[r, q] stands in for the transpose's G[q, r] (K[r, q] for K[q, r]): equal in
    exact arithmetic, up to one unit in the last place apart in the float64 tables.

So L = 2 (P + 1) + 16.  The other rows are shorter: a G^T w term of yu has 1 (c_div zc) + 2 (P + 1) + 5 (bx w - sum,
My, (dy / 2) My, its fma, + m zu) + 4; a term of yp 2 (P + 1) + 8 + 4 (bx z' - sum, My, (dy / 2) My, the product, the y
part's fma, the two K k fmas, + zc[pin]); yT = ((fT Mx) My) z'_v has 7.  SLACK = 2 covers the second-order terms, as
in test_gpu_ns_apply_launches.py.  Rows that are a single copy are exact: yu = zu, yv = zv when every node is a
Dirichlet node, yp[pin] = zc[pin] when there is no Dirichlet node and no velocity input.  Everything a launch must not
write starts as a sentinel and is compared bit for bit; every launch runs twice and must reproduce its bits.  Each test
prints its largest ratio to the first-order bound (L 2^-53 (|A^T| |z|)_r) per form."""
import ctypes as C

import numpy as np
import pytest
import torch

from ns_reference import LD, dirichlet_rows, uv_index
from ns_reference_T import ns_reference_T

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
SLACK = 2.0
SENTINEL = -7.25e77
GUARD = 37                       # sentinel entries before and after every plain output
DX, DY = 0.37, 0.23
COEF = dict(c_mass=0.75, c_stiff=1.0, c_gradx=310.0, c_grady=-270.0)
NAMES = ("zu", "zv", "zc", "cu", "cv", "juu", "juv", "jvu", "jvv")
OUTS = ("yu", "yv", "yp", "yT")


def _tye(P):
    """The kernel's y tile in elements (NsTTile::TYE)."""
    return max(32 // P, 1)


def _chain(P):
    return 2 * (P + 1) + 16


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


class _Case:
    """One whole-mesh handle and one set of random fields (uniform in (-1, 1), fixed seed) on its nodes."""

    def __init__(self, P, nex, ney, seed):
        from sem_amd.device import Mesh
        self.geo = (P, nex, ney, DX, DY, 0, nex)
        self.P, self.nex, self.ney = P, nex, ney
        self.mesh = Mesh(*self.geo)
        self.lines, self.NY = nex * P + 1, ney * P + 1
        self.n = self.lines * self.NY
        assert self.mesh.n_local == self.n and self.mesh.NY == self.NY
        r = np.random.default_rng(seed)
        self.f = {k: r.uniform(-1, 1, self.n) for k in NAMES}

    def form(self, name):
        """(ins, outs, descriptor) of the forms the solvers launch."""
        f = self.f
        jac = dict(COEF, cu=f["cu"], cv=f["cv"], juu=f["juu"], juv=f["juv"], jvu=f["jvu"], jvv=f["jvv"])
        rows = dict(dir_sides=15, pin=int(self.n / 2), pin_first=False)
        if name == "full":      # _get_dresiduals_T with the temperature bar
            return ("zu", "zv", "zc"), OUTS, dict(jac, c_T=-0.4, c_div=1.0, **rows)
        if name == "noT":       # _get_dresiduals_T without it
            return ("zu", "zv", "zc"), OUTS[:3], dict(jac, c_div=1.0, **rows)
        if name == "grad":      # the transposed gradient of the adjoint Schur matvec (-C^T q)
            return ("zc",), ("yu", "yv"), dict(rows, c_div=-1.0)
        if name == "div":       # its transposed divergence (B^T x + E^T q)
            return ("zu", "zv", "zc"), ("yp",), dict(rows)
        if name == "vel":       # the velocity rows alone (J^T x)
            return ("zu", "zv"), ("yu", "yv"), dict(jac, **rows)
        raise KeyError(name)

    def check(self, ins, outs, kw, L, pitch=0):
        """Launches twice, checks sentinels, reproducibility and the per-row bound; returns (the largest ratio to the
        first-order bound, the outputs)."""
        n, NY, lines = self.n, self.NY, self.lines
        host = {k: (self.f[k] if k in ins else None) for k in ("zu", "zv", "zc")}
        idx = uv_index(lines, NY, pitch)
        span = lines * (pitch or NY)
        if pitch:
            assert pitch >= 2 * NY
            B = np.full(span, np.nan)
            for k, o in (("zu", 0), ("zv", NY)):
                if host[k] is not None:
                    B[o + idx] = host[k]
            dB = _dev(B)
            view = lambda t, o: torch.as_strided(t, (lines, NY), (pitch, 1), o)   # noqa: E731
            d_in = {k: (view(dB, o) if host[k] is not None else None) for k, o in (("zu", 0), ("zv", NY))}
        else:
            d_in = {k: (_dev(host[k]) if host[k] is not None else None) for k in ("zu", "zv")}
        d_in["zc"] = _dev(host["zc"]) if host["zc"] is not None else None
        dkw = {k: (_dev(x) if isinstance(x, np.ndarray) else x) for k, x in kw.items()}
        sent = _bits(np.array([SENTINEL]))[0]

        def launch():
            res = {}
            if pitch:
                R = torch.full((span + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
                d_out = {k: (view(R, GUARD + o) if k in outs else None) for k, o in (("yu", 0), ("yv", NY))}
                bufs = {}
            else:
                bufs = {k: torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
                        for k in ("yu", "yv") if k in outs}
                d_out = {k: (bufs[k][GUARD:GUARD + n] if k in bufs else None) for k in ("yu", "yv")}
            # the plain outputs; one that is not requested is not passed, and a buffer the launch must not touch
            # (yT of a launch without it) stays whole
            plain = {k: torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda") for k in ("yp", "yT")}
            self.mesh.ns_apply_transpose(d_in["zu"], d_in["zv"], d_in["zc"], d_out["yu"], d_out["yv"],
                                         plain["yp"][GUARD:GUARD + n] if "yp" in outs else None,
                                         plain["yT"][GUARD:GUARD + n] if "yT" in outs else None, **dkw)
            torch.cuda.synchronize()
            if pitch:
                h = R.cpu().numpy()
                keep = np.ones(h.size, dtype=bool)
                for k, o in (("yu", 0), ("yv", NY)):
                    if k in outs:
                        res[k] = h[GUARD + o + idx].copy()
                        keep[GUARD + o + idx] = False
                assert np.all(_bits(h)[keep] == sent), "a line view's padding, guard or unrequested half was written"
            for k, b in list(bufs.items()) + list(plain.items()):
                h = b.cpu().numpy()
                if k in outs:
                    res[k] = h[GUARD:GUARD + n].copy()
                    assert np.all(_bits(h[:GUARD]) == sent) and np.all(_bits(h[GUARD + n:]) == sent), f"{k} guard"
                else:
                    assert np.all(_bits(h) == sent), f"{k} was written though not requested"
            return res

        got, again = launch(), launch()
        for k in outs:
            assert np.array_equal(_bits(got[k]), _bits(again[k])), f"{k} is not reproducible"
        ref = dict(zip(OUTS, ns_reference_T(*self.geo, host["zu"], host["zv"], host["zc"], **kw)))
        bnd = dict(zip(OUTS, ns_reference_T(*self.geo, host["zu"], host["zv"], host["zc"], absval=True, **kw)))
        worst = 0.0
        for k in outs:
            g = got[k]
            assert np.all(np.isfinite(g)), f"{k}: a non-finite value (NaN padding read?)"
            err = np.abs(g.astype(LD) - ref[k])
            b = bnd[k]
            assert np.all(err[b == 0] == 0), f"{k}: a row with no terms is not zero"
            ratio = float((err[b > 0] / (L * LD(U53) * b[b > 0])).max()) if (b > 0).any() else 0.0
            assert ratio <= SLACK, f"{k}: {ratio:.3f} of the first-order bound (L = {L})"
            worst = max(worst, ratio)
        return worst, got


def _report(P, ratios):
    print("NSTRATIO", f"P={P}", " ".join(f"{k}={v:.3f}" for k, v in sorted(ratios.items())))


def _two_launch_velocity(s, kw, zu, zv):
    """NavierStokesSolver._velocity_apply_lines_T (two sem_apply_transpose launches) on the case's mesh and fields."""
    from sem_amd.solvers.convection_diffusion import DirichletRows
    from sem_amd.solvers.navier_stokes import NavierStokesSolver
    ns = object.__new__(NavierStokesSolver)
    ns._part, ns._mesh, ns._free = None, s.mesh, None
    ns._jac_kw = {k: (_dev(x) if isinstance(x, np.ndarray) else x) for k, x in kw.items()
                  if k in ("c_stiff", "c_mass", "c_gradx", "cu", "c_grady", "cv", "juu", "juv", "jvu", "jvv")}
    dm = dirichlet_rows(s.P, s.nex, s.ney, 0, s.nex, kw.get("dir_mask"), kw.get("dir_sides", 0))[0].reshape(-1)
    ns._dir = DirichletRows(s.mesh, dm, 15)
    X = torch.stack((_dev(zu).view(-1, s.NY), _dev(zv).view(-1, s.NY)), dim=1).reshape(-1, 2 * s.NY)
    Y = ns._velocity_apply_lines_T(X).view(-1, 2, s.NY)
    return Y[:, 0].reshape(-1).cpu().numpy(), Y[:, 1].reshape(-1).cpu().numpy()


@pytest.mark.parametrize("P", range(1, 17))
def test_shape_sweep(gpu, P):
    """Every order at the y tilings around a tile edge -- the ghost column inside a partial tile (ney = TYE - 1),
    alone in its own tile (TYE), and after a second tile of one element (TYE + 1) -- on two element columns, and on a
    1 x 1 mesh, in the forms the solvers launch.  The velocity rows also against the two-launch transposed apply."""
    T, L = _tye(P), _chain(P)
    ratios = {}
    for nex, ney in ((2, T - 1), (2, T), (2, T + 1), (1, 1)):
        if ney < 1:
            continue
        s = _Case(P, nex, ney, seed=1000 * P + 10 * ney + nex)
        for name in ("full", "noT", "grad", "div", "vel"):
            ins, outs, kw = s.form(name)
            r, got = s.check(ins, outs, kw, L)
            ratios[name] = max(ratios.get(name, 0.0), r)
            if name == "vel":
                two = _two_launch_velocity(s, kw, s.f["zu"], s.f["zv"])
                bnd = ns_reference_T(*s.geo, s.f["zu"], s.f["zv"], None, absval=True, **kw)
                for k, t, b in zip(("yu", "yv"), two, bnd):
                    # the same bound as against the reference
                    d = np.abs(got[k].astype(LD) - t.astype(LD))
                    assert np.all(d[b == 0] == 0)
                    r2 = float((d[b > 0] / (L * LD(U53) * b[b > 0])).max())
                    assert r2 <= SLACK, f"{k}: the fused and the two-launch velocity rows differ by {r2:.3f}"
                    ratios["vel-2launch"] = max(ratios.get("vel-2launch", 0.0), r2)
    _report(P, ratios)


def _contract_cases(P):
    """(tag, base form, descriptor changes, operands / outputs dropped, pitch) on nex = 3, ney = 2."""
    NY = 2 * P + 1
    n = (3 * P + 1) * NY
    cases = []
    add = lambda tag, base, kw=None, drop=(), pitch=0: cases.append((tag, base, kw or {}, drop, pitch))   # noqa: E731
    for sides in (0, 1, 2, 4, 8, 15):       # W, E, S, N: which bit is which side; 0: no Dirichlet set
        add(f"sides{sides}", "full", dict(dir_sides=sides))
    for base in ("full", "grad", "div"):    # a mask with interior nodes; dir_sides must be ignored
        add("mask", base, dict(dir_mask="random", dir_sides=10))
    pins = [("none", -1), ("interior", (P + 1) * NY + 1 if P > 1 else P * NY + 1), ("boundary", P * NY),
            ("corner", 0), ("last", n - 1)]
    for tag, pin in pins:
        for first in (True, False):
            for base in ("full", "grad", "div"):
                add(f"pin-{tag}", base, dict(pin=pin, pin_first=first))
    add("pin-masked-interior", "full", dict(dir_mask="random+pin", pin=(P + 1) * NY + 1 if P > 1 else P * NY + 1,
                                           pin_first=True))
    for pitch in (0, 2 * NY, 2 * NY + 3):   # line views
        for base in ("full", "grad", "div", "vel"):
            add(f"pitch{pitch}", base, pitch=pitch)
        add(f"pitch{pitch}", "full", drop=("yu",), pitch=pitch)
    add("ones", "full", dict(cu=None, cv=None))
    for j in ("juu", "juv", "jvu", "jvv"):
        add(f"no-{j}", "full", {j: None})
    for k in ("zu", "zv", "zc", "yu", "yv", "yp", "yT"):
        add(f"no-{k}", "full", drop=(k,))
    add("no-zc", "div", drop=("zc",))       # B^T f of the adjoint update
    add("yT-only", "full", drop=("yu", "yv", "yp"))
    add("cT-zero", "full", dict(c_T=0.0))
    return cases


@pytest.mark.parametrize("P", [1, 3, 4, 7, 12, 16])
def test_descriptor_contract(gpu, P):
    """The descriptor's paths, each varied from one of the solver forms on nex = 3, ney = 2."""
    L = _chain(P)
    s = _Case(P, 3, 2, seed=77 * P + 21)
    ratios = {}
    for tag, base, dkw, drop, pitch in _contract_cases(P):
        ins, outs, kw = s.form(base)
        kw = dict(kw)
        kw.update(dkw)
        if isinstance(kw.get("dir_mask"), str):
            mask = (np.random.default_rng(P).random(s.n) < 0.25).astype(np.uint8)
            if kw["dir_mask"].endswith("+pin"):
                mask[kw["pin"]] = 1
            kw["dir_mask"] = mask
        ins = tuple(k for k in ins if k not in drop)
        outs = tuple(k for k in outs if k not in drop)
        try:
            r, _ = s.check(ins, outs, kw, L, pitch)
        except AssertionError as e:
            raise AssertionError(f"{tag} form {base} (P = {P}): {e}") from e
        ratios[base] = max(ratios.get(base, 0.0), r)
    _report(P, ratios)


@pytest.mark.parametrize("P", [1, 2, 5, 12])
def test_single_copy_rows_are_exact(gpu, P):
    """Every node a Dirichlet node: z' = 0 and w = 0, so yu = zu and yv = zv bit for bit.  No Dirichlet node and no
    velocity input: k = 0, so yp is zc[pin] on the pinned row, bit for bit, and zero elsewhere."""
    s = _Case(P, 2, 2, seed=5 * P)
    ins, outs, kw = s.form("full")
    _, got = s.check(ins, outs, dict(kw, dir_mask=np.ones(s.n, dtype=np.uint8)), _chain(P))
    assert np.array_equal(_bits(got["yu"]), _bits(s.f["zu"]))
    assert np.array_equal(_bits(got["yv"]), _bits(s.f["zv"]))
    pin = kw["pin"]
    _, got = s.check(("zc",), ("yp",), dict(kw, dir_sides=0), _chain(P))
    assert _bits(got["yp"][pin:pin + 1])[0] == _bits(s.f["zc"][pin:pin + 1])[0]
    ins, outs, kw = s.form("div")            # the same through the transposed-divergence kernel
    _, got = s.check(("zc",), ("yp",), dict(kw, dir_sides=0, c_div=0.0), _chain(P))
    want = np.zeros(s.n)
    want[pin] = s.f["zc"][pin]
    assert np.array_equal(got["yp"], want)


def test_argument_checks(gpu):
    """The raw ABI's refusals, by status and message; a call without outputs is SEM_OK and touches nothing."""
    from sem_amd import _lib as Lb
    from sem_amd.device import Mesh
    lib = Lb.load()
    mesh = Mesh(2, 2, 2, DX, DY)
    n, NY = mesh.n_local, mesh.NY
    r = np.random.default_rng(2)
    zu, zv, zc, aux = (_dev(r.uniform(-1, 1, n)) for _ in range(4))
    yu, yv, yp, yT = (torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(4))
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    stream = mesh.stream_ptr()

    def call(h, d, ins=(zu, zv, zc), outs=(yu, yv, yp, yT)):
        st = lib.sem_ns_apply_transpose(h, None if d is None else C.byref(d), *(ptr(t) for t in ins),
                                        *(ptr(t) for t in outs), stream)
        return st, lib.sem_last_error().decode(errors="replace")

    def desc(**kw):
        d = Lb.SemNsDesc()
        d.c_stiff, d.c_div, d.pin = 1.0, 1.0, -1
        for k, x in kw.items():
            setattr(d, k, x)
        return d

    inval = [(None, desc(), {}, "null argument"), (mesh._h, None, {}, "null argument"),
             (mesh._h, desc(uv_pitch=NY - 1), {}, "uv_pitch below the line length"),
             (mesh._h, desc(uv_pitch=1), {}, "uv_pitch below the line length"),
             (mesh._h, desc(pin=-2), {}, "pinned node out of range"),
             (mesh._h, desc(pin=mesh.NX * NY), {}, "pinned node out of range"),
             (mesh._h, desc(T=aux.data_ptr()), {}, "T, dval_u, dval_v must be NULL"),
             (mesh._h, desc(dval_u=aux.data_ptr()), {}, "T, dval_u, dval_v must be NULL"),
             (mesh._h, desc(dval_v=aux.data_ptr()), {}, "T, dval_u, dval_v must be NULL"),
             (mesh._h, desc(pin_val=0.5), {}, "pin_val 0")]
    for i, src in enumerate((zu, zv, zc)):          # every output against every input
        for j in range(4):
            outs = [yu, yv, yp, yT]
            outs[j] = src
            inval.append((mesh._h, desc(), dict(outs=tuple(outs)), "an output aliases an input"))
    big = _dev(r.uniform(-1, 1, mesh.NX * 2 * NY))
    for k in ("cu", "cv"):                           # cu / cv by pointer on a line view names other nodes
        for pitch in (2 * NY, NY + 1):
            inval.append((mesh._h, desc(uv_pitch=pitch, **{k: big.data_ptr()}), dict(ins=(big, zv, zc)),
                          f"{k} aliases zu or zv"))
            inval.append((mesh._h, desc(uv_pitch=pitch, **{k: big.data_ptr()}), dict(ins=(zu, big, zc)),
                          f"{k} aliases zu or zv"))
    for h, d, kw, text in inval:
        st, msg = call(h, d, **kw)
        assert st == Lb.SEM_EINVAL and text in msg, (text, st, msg)
    # ... and cu = zu, cv = zv are accepted for plain vectors, whichever way the pitch says so
    for pitch in (0, NY):
        st, _ = call(mesh._h, desc(uv_pitch=pitch, cu=zu.data_ptr(), cv=zv.data_ptr()))
        assert st == Lb.SEM_OK
    torch.cuda.synchronize()
    sent = _bits(np.array([SENTINEL]))[0]
    assert not np.any(_bits(yu.cpu().numpy()) == sent)
    # SEM_EUNSUPPORTED: a strip handle; offsets past 32 bits (refused before any pointer is used)
    strip = Mesh(2, 3, 2, DX, DY, 1, 2)
    st, msg = call(strip._h, desc())
    assert st == Lb.SEM_EUNSUPPORTED and "whole-mesh handles only" in msg
    st, msg = call(mesh._h, desc(uv_pitch=2 ** 30))
    assert (mesh.NX - 1) * 2 ** 30 + NY > 2 ** 31 - 1
    assert st == Lb.SEM_EUNSUPPORTED and "32-bit node-offset limit" in msg
    # a handle of another device than the current one, and an order without a compiled kernel: no valid handle has
    # either on a one-GPU box (sem_create refuses P = 17), so the handle's fields are overwritten and put back
    # (struct sem_handle, sem_internal.h: int P, nex, ney, ex_begin, ex_end, device; test_gpu_abi.py's way)
    for o in (yu, yv, yp, yT):
        o.fill_(SENTINEL)
    field = C.cast(mesh._h, C.POINTER(C.c_int))
    for at, value, status, text in ((5, 7, Lb.SEM_EINVAL, "handle belongs to device 7"),
                                    (0, 17, Lb.SEM_EUNSUPPORTED, "polynomial order outside compiled range")):
        old = field[at]
        field[at] = value
        try:
            st, msg = call(mesh._h, desc())
        finally:
            field[at] = old
        assert st == status and text in msg, (text, st, msg)
    torch.cuda.synchronize()
    for o in (yu, yv, yp, yT):
        assert np.all(_bits(o.cpu().numpy()) == sent)
    st, _ = call(mesh._h, desc())            # the handle is whole again
    assert st == Lb.SEM_OK
    # no output at all: SEM_OK, nothing launched, nothing written
    keep = [t.clone() for t in (zu, zv, zc)]
    for o in (yu, yv, yp, yT):
        o.fill_(SENTINEL)
    st, _ = call(mesh._h, desc(), outs=(None, None, None, None))
    torch.cuda.synchronize()
    assert st == Lb.SEM_OK
    for t, k in zip((zu, zv, zc), keep):
        assert torch.equal(t, k)
    for o in (yu, yv, yp, yT):
        assert np.all(_bits(o.cpu().numpy()) == sent)
