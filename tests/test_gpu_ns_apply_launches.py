"""GPU tests of sem_ns_apply (sem_amd/csrc/ns_apply.hip) one launch at a time through Mesh.ns_apply on synthetic
device arrays, against tests/ns_reference.py (np.longdouble, pinned to the oracle by tests/test_ns_reference.py):
every order P = 1..16 in the band and the LDS-tile form, the three y tilings around a tile edge, whole meshes and
strips, the six forms the solvers launch, and the descriptor's contract (Dirichlet sides and masks, pins, line views,
aliasing, absent operands and outputs), plus the band form's 32-bit offset boundary and the argument checks.

Bound per row, derived from the kernels' code, not measured:  |got_r - ref_r| <= SLACK L 2^-53 (|A| |x|)_r  with
(|A| |x|)_r from ns_reference(absval=True) and L the longest chain of roundings a term of the row goes through:

  * the sums.  A node on an element corner sums two elements of P + 1 fused multiply-adds in each direction.  The
    band form keeps the y sums and the x sums in separate accumulators (2 (P + 1) each, the longer path), the tile
    form runs x then y into one accumulator (4 (P + 1));
  * 6 to finish the longest row, rv: band fma(hx mx, G_y p, Sys v), the add of the x sums, the mass term, jvu, jvv, T
    (tile: mass, jvu, jvv, G_y p, T: 5);
  * 6 for the Sys coefficient of a term: c_stiff (dx / dy) on the host (2), the assembled weight mx = w_P + w_0 (1),
    fKy mx (1), fy K (1), fma(gyc, G, fy K) (1)  (the convection part fY cv mx has 5);
  * 1 because the kernels' compile-time GLL constants may differ from the oracle's tables in the last place.

So L = 2 (P + 1) + 13 for the band form and 4 (P + 1) + 13 for the tile form (one more than its count, to keep one
constant).  SLACK = 2 covers the second-order terms, as in test_gpu_front_kernels.py.  Rows replaced by a single
subtraction (u - dval, p - pin_val) must be exact and rows written as 0 must be +0.0, bit for bit.  Everything a
launch must not write starts as a sentinel and is compared bit for bit; every launch runs twice and must reproduce
its bits.  Each test prints its largest ratio to the first-order bound (L 2^-53 (|A| |x|)_r) per form."""
import ctypes as C

import numpy as np
import pytest
import torch

from ns_reference import LD, dirichlet_rows, ns_reference, pin_row, strip_shape, uv_index

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
SLACK = 2.0
SENTINEL = -7.25e77
GUARD = 37                       # sentinel entries before and after every plain output
DX, DY = 0.37, 0.23
COEF = dict(c_mass=0.75, c_stiff=1.0, c_gradx=310.0, c_grady=-270.0)
NAMES = ("u", "v", "p", "T", "cu", "cv", "juu", "juv", "jvu", "jvv", "dval_u", "dval_v")
KINDS = ("band", "tile")


def _tye(P, kind):
    return max((64 if kind == "band" else 32) // P, 1)


def _chain(P, kind):
    return (2 if kind == "band" else 4) * (P + 1) + 13


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


class _Strip:
    """One handle and one set of random fields (uniform in (-1, 1), fixed seed) on its n_local nodes."""

    def __init__(self, P, nex, ney, eb, ee, seed):
        from sem_amd.device import Mesh
        self.geo = (P, nex, ney, DX, DY, eb, ee)
        self.P, self.nex, self.ney, self.eb, self.ee = P, nex, ney, eb, ee
        self.mesh = Mesh(*self.geo)
        self.lines, self.NY, self.l0 = strip_shape(P, nex, ney, eb, ee)
        self.n = self.lines * self.NY
        assert self.mesh.n_local == self.n and self.mesh.NY == self.NY
        r = np.random.default_rng(seed)
        self.f = {k: r.uniform(-1, 1, self.n) for k in NAMES}
        self.N = (nex * P + 1) * self.NY

    def boundary_mask(self):
        return dirichlet_rows(*self._g(), None, 15)[0].reshape(-1).astype(np.uint8)

    def _g(self):
        return self.P, self.nex, self.ney, self.eb, self.ee

    # ---- the forms of the shape sweep
    def form(self, name):
        """(ins, outs, kw, alias): operands present, outputs written, descriptor (numpy values), and which of
        cu, cv are passed as the very tensors of u, v."""
        f = self.f
        pin = int(self.N / 2)
        if name == "a":     # the residual
            return ("u", "v", "p"), ("ru", "rv", "rc"), dict(
                COEF, cu=f["u"], cv=f["v"], c_T=-0.4, T=f["T"], c_div=-1.0, dval_u=f["dval_u"], dval_v=f["dval_v"],
                dir_mask=self.boundary_mask(), pin=pin, pin_val=0.3, pin_first=True), ("cu", "cv")
        jac = dict(COEF, cu=f["cu"], cv=f["cv"], juu=f["juu"], juv=f["juv"], jvu=f["jvu"], jvv=f["jvv"])
        rows = dict(dir_sides=15, pin=pin, pin_val=0.0, pin_first=False)
        if name == "b":     # the Jacobian: distinct cu, cv (the staged-cv variant of the band form)
            return ("u", "v", "p"), ("ru", "rv", "rc"), dict(jac, c_T=-0.4, T=f["T"], c_div=-1.0, **rows), ()
        if name == "c":     # the Schur gradient
            return ("p",), ("ru", "rv"), dict(rows), ()
        if name == "d":     # the Schur divergence
            return ("u", "v", "p"), ("rc",), dict(rows, c_div=-1.0), ()
        if name == "e":     # the velocity rows alone (the refinement step's operator)
            return ("u", "v"), ("ru", "rv"), dict(jac, **rows), ()
        if name == "f":     # the divergence of a velocity alone
            return ("u", "v"), ("rc",), dict(rows, c_div=-1.0), ()
        raise KeyError(name)

    # ---- one checked launch
    def check(self, ins, outs, kw, alias, L, pitch=0):
        """Launches twice, checks sentinels, reproducibility, the exact rows and the per-row bound; returns the
        largest ratio to the first-order bound."""
        n, NY, lines = self.n, self.NY, self.lines
        f = self.f
        host = {k: (f[k] if k in ins else None) for k in ("u", "v", "p")}
        for k in alias:
            assert kw[k] is f[k[1]] and k[1] in ins and pitch in (0, NY)
        idx = uv_index(lines, NY, pitch)
        span = lines * (pitch or NY)

        # operands
        if pitch:
            assert pitch >= 2 * NY
            B = np.full(span, np.nan)
            for k, o in (("u", 0), ("v", NY)):
                if host[k] is not None:
                    B[o + idx] = host[k]
            dB = _dev(B)
            view = lambda t, o: torch.as_strided(t, (lines, NY), (pitch, 1), o)   # noqa: E731
            d_in = {k: (view(dB, o) if host[k] is not None else None) for k, o in (("u", 0), ("v", NY))}
        else:
            d_in = {k: (_dev(host[k]) if host[k] is not None else None) for k in ("u", "v")}
        d_in["p"] = _dev(host["p"]) if host["p"] is not None else None
        dkw = {}
        for k, x in kw.items():
            if k in alias:
                dkw[k] = d_in[k[1]]
            elif isinstance(x, np.ndarray):
                dkw[k] = _dev(x)
            else:
                dkw[k] = x

        def launch():
            res = {}
            if pitch:
                R = torch.full((span + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
                d_out = {k: (view(R, GUARD + o) if k in outs else None) for k, o in (("ru", 0), ("rv", NY))}
            else:
                bufs = {k: torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
                        for k in ("ru", "rv") if k in outs}
                d_out = {k: (bufs[k][GUARD:GUARD + n] if k in bufs else None) for k in ("ru", "rv")}
            rcb = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda") if "rc" in outs else None
            self.mesh.ns_apply(d_in["u"], d_in["v"], d_in["p"], d_out["ru"], d_out["rv"],
                               None if rcb is None else rcb[GUARD:GUARD + n], **dkw)
            torch.cuda.synchronize()
            sent = _bits(np.array([SENTINEL]))[0]
            if pitch:
                h = R.cpu().numpy()
                keep = np.ones(h.size, dtype=bool)
                for k, o in (("ru", 0), ("rv", NY)):
                    if k in outs:
                        res[k] = h[GUARD + o + idx].copy()
                        keep[GUARD + o + idx] = False
                assert np.all(_bits(h)[keep] == sent), "a line view's padding or guard was written"
            else:
                for k, b in bufs.items():
                    h = b.cpu().numpy()
                    res[k] = h[GUARD:GUARD + n].copy()
                    assert np.all(_bits(h[:GUARD]) == sent) and np.all(_bits(h[GUARD + n:]) == sent), f"{k} guard"
            if rcb is not None:
                h = rcb.cpu().numpy()
                res["rc"] = h[GUARD:GUARD + n].copy()
                assert np.all(_bits(h[:GUARD]) == sent) and np.all(_bits(h[GUARD + n:]) == sent), "rc guard"
            return res

        got, again = launch(), launch()
        for k in outs:
            assert np.array_equal(_bits(got[k]), _bits(again[k])), f"{k} is not reproducible"

        ref = dict(zip(("ru", "rv", "rc"), ns_reference(*self.geo, host["u"], host["v"], host["p"], **kw)))
        bnd = dict(zip(("ru", "rv", "rc"), ns_reference(*self.geo, host["u"], host["v"], host["p"], absval=True, **kw)))
        dm, own = dirichlet_rows(*self._g(), kw.get("dir_mask"), kw.get("dir_sides", 0))
        dm, own = dm.reshape(-1), own.reshape(-1)
        zero = lambda a: np.zeros(n) if a is None else a   # noqa: E731
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
            if k in ("ru", "rv"):
                x, dval = zero(host["u" if k == "ru" else "v"]), zero(kw.get("dval_u" if k == "ru" else "dval_v"))
                sel = dm & own
                assert np.array_equal(_bits(g[sel]), _bits((x - dval)[sel])), f"{k}: a Dirichlet row is not exact"
                assert np.all(_bits(g[dm & ~own]) == 0), f"{k}: an unowned Dirichlet row is not +0.0"
        if "rc" in outs:
            at = pin_row(*self._g(), int(kw.get("pin", -1)), bool(kw.get("pin_first", False)), dm.reshape(lines, NY))
            if at is not None:
                q = at[0] * NY + at[1]
                want = (zero(host["p"])[q] - kw.get("pin_val", 0.0)) if own[q] else 0.0
                assert _bits(got["rc"][q:q + 1])[0] == _bits(np.array([want]))[0], "rc: the pinned row is not exact"
        return worst


def _report(kind, P, ratios):
    print("NSRATIO", kind, f"P={P}", " ".join(f"{k}={v:.3f}" for k, v in sorted(ratios.items())))


@pytest.mark.parametrize("P", range(1, 17))
@pytest.mark.parametrize("kind", KINDS)
def test_shape_sweep(gpu, tuning, kind, P):
    """Every order in both forms at the y tilings around a tile edge -- the ghost column inside a partial tile
    (ney = TYE - 1), alone in its own tile (TYE), and after a second tile of one element (TYE + 1) -- on a whole
    mesh (nex = 2) and on the strip [1, 2) of nex = 3 (both interface lines), in the six forms the solvers launch."""
    from sem_amd import _lib
    tuning(_lib.TUNE_NS_APPLY, 1 if kind == "tile" else 0)
    T, L = _tye(P, kind), _chain(P, kind)
    ratios = {}
    for ney in (T - 1, T, T + 1):
        if ney < 1:
            continue
        for nex, eb, ee in ((2, 0, 2), (3, 1, 2)):
            s = _Strip(P, nex, ney, eb, ee, seed=1000 * P + 10 * ney + nex)
            for name in "abcdef":
                r = s.check(*s.form(name), L)
                ratios[name] = max(ratios.get(name, 0.0), r)
    _report(kind, P, ratios)


def _contract_cases(P):
    """(tag, (nex, eb, ee), base form, descriptor changes, operand / output changes, pitch factor, alias) on ney = 2."""
    NY = 2 * P + 1
    cases = []
    add = lambda tag, x, base, kw=None, io=None, pitch=0, alias=None: cases.append(   # noqa: E731
        (tag, x, base, kw or {}, io or {}, pitch, alias))
    whole = (3, 0, 3)
    for x in ((3, 0, 1), (3, 0, 2), (3, 1, 3), (3, 2, 3), whole, (1, 0, 1)):
        for base in "ab":
            add(f"strip{x}", x, base)
    for sides in (0, 1, 2, 4, 8, 15):       # W, E, S, N: which bit is which side
        add(f"sides{sides}", whole, "b", dict(dir_sides=sides))
        add(f"sides{sides}", (3, 1, 2), "b", dict(dir_sides=sides))
    for x in (whole, (3, 0, 2)):            # a mask with interior nodes; dir_sides must be ignored
        for base in "ab":
            add("mask", x, base, dict(dir_mask="random", dir_sides=10))
    mid = (3, 1, 2)                          # lines P .. 2 P: both interface lines
    pins = [("none", -1), ("interior", (P + 1) * NY + 1 if P > 1 else P * NY + 1), ("left-line", P * NY + 1),
            ("right-line", 2 * P * NY + 1), ("not-held", 0), ("dirichlet", P * NY), ("right-dirichlet", 2 * P * NY)]
    for tag, pin in pins:
        for x in (whole, mid):
            for first in (True, False):
                add(f"pin-{tag}", x, "b", dict(pin=pin, pin_val=0.3, pin_first=first))
            add(f"pin-{tag}", x, "a", dict(pin=pin))
    for pitch in (0, 2 * NY, 2 * NY + 3):   # line views: cu, cv must then be tensors of their own
        add(f"pitch{pitch}", whole, "a", pitch=pitch, alias=())
        add(f"pitch{pitch}", whole, "b", pitch=pitch)
        add(f"pitch{pitch}", whole, "b", io=dict(ru=None), pitch=pitch)
    add("alias-cu", whole, "a", alias=("cu",))
    add("alias-cv", whole, "a", alias=("cv",))
    add("alias-cu", mid, "a", alias=("cu",))
    add("alias-cv", mid, "a", alias=("cv",))
    for x in (whole, mid):
        add("ones", x, "b", dict(cu=None, cv=None))
        for j in ("juu", "juv", "jvu", "jvv"):
            add(f"no-{j}", x, "b", {j: None})
        add("no-T", x, "a", dict(T=None))
        add("no-dval", x, "a", dict(dval_u=None, dval_v=None))
        for k in ("u", "v", "ru", "rv"):
            add(f"no-{k}", x, "b", io={k: None})
    return cases


@pytest.mark.parametrize("P", [1, 3, 4, 7, 12, 16])
@pytest.mark.parametrize("kind", KINDS)
def test_descriptor_contract(gpu, tuning, kind, P):
    """The descriptor's paths, each varied from the residual (a) or the Jacobian (b) form on nex = 3, ney = 2: both
    Y-phase lane orders (P = 3, 7 against 1, 4, 12, 16), orders with idle waves (P < 4) and the largest order."""
    from sem_amd import _lib
    tuning(_lib.TUNE_NS_APPLY, 1 if kind == "tile" else 0)
    L = _chain(P, kind)
    strips, ratios = {}, {}
    for tag, x, base, dkw, io, pitch, alias in _contract_cases(P):
        if x not in strips:
            strips[x] = _Strip(P, x[0], 2, x[1], x[2], seed=77 * P + 7 * x[0] + 3 * x[1] + x[2])
        s = strips[x]
        ins, outs, kw, base_alias = s.form(base)
        alias = base_alias if alias is None else alias
        kw = dict(kw)
        for k in ("cu", "cv"):                # cu = u by value but not by pointer: a tensor of its own
            if k in base_alias and k not in alias:
                kw[k] = s.f[k[1]].copy()
        for k, val in dkw.items():
            kw[k] = val
        if isinstance(kw.get("dir_mask"), str):
            kw["dir_mask"] = (np.random.default_rng(P + x[1]).random(s.n) < 0.25).astype(np.uint8)
        ins = tuple(k for k in ins if k not in io)
        outs = tuple(k for k in outs if k not in io)
        try:
            r = s.check(ins, outs, kw, alias, L, pitch)
        except AssertionError as e:
            raise AssertionError(f"{tag} {x} form {base} ({kind}, P = {P}): {e}") from e
        ratios[base] = max(ratios.get(base, 0.0), r)
    _report(kind, P, ratios)


def test_band_offset_boundary(gpu, tuning):
    """The band form addresses u, v through 32-bit buffer offsets and takes operands below 2 GB: line views of pitch
    2^28 - 3 on two lines of two nodes (P = 1, one element) span 2^31 - 8 bytes, the last size it takes; pitch
    2^28 - 2 spans 2^31 and falls back to the tile form.  Both against the reference under the band form's bound."""
    from sem_amd import _lib
    from sem_amd.device import Mesh
    tuning(_lib.TUNE_NS_APPLY, 0)
    geo = (1, 1, 1, DX, DY, 0, 1)
    mesh = Mesh(*geo)
    r = np.random.default_rng(31)
    f = {k: r.uniform(-1, 1, 4) for k in NAMES}
    kw = dict(COEF, cu=f["cu"], cv=f["cv"], juu=f["juu"], juv=f["juv"], jvu=f["jvu"], jvv=f["jvv"], c_T=-0.4, T=f["T"],
              c_div=-1.0, dir_sides=4, pin=3, pin_val=0.3, pin_first=False)
    dkw = {k: (_dev(x) if isinstance(x, np.ndarray) else x) for k, x in kw.items()}
    ref = ns_reference(*geo, f["u"], f["v"], f["p"], **kw)
    bnd = ns_reference(*geo, f["u"], f["v"], f["p"], absval=True, **kw)
    L = _chain(1, "band")
    big = 2 ** 28 + 16
    buf = torch.empty(big, dtype=torch.float64, device="cuda")   # about 2 GiB; a failed allocation fails the test
    try:
        for pitch in (2 ** 28 - 3, 2 ** 28 - 2):
            span = (pitch + 2) * 8
            assert (span < 2 ** 31) == (pitch == 2 ** 28 - 3)
            view = lambda o: torch.as_strided(buf, (2, 2), (pitch, 1), o)   # noqa: E731
            u, v, ru, rv = (view(o) for o in (0, 2, 4, 6))
            near = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, 8, 9], device="cuda")
            for base in (0, pitch):               # the used doubles and sentinels beside the outputs
                buf[base + near] = SENTINEL
            u.copy_(_dev(f["u"].reshape(2, 2)))
            v.copy_(_dev(f["v"].reshape(2, 2)))
            rc = torch.full((4 + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
            mesh.ns_apply(u, v, _dev(f["p"]), ru, rv, rc[GUARD:GUARD + 4], **dkw)
            torch.cuda.synchronize()
            got = (ru.cpu().numpy().reshape(-1), rv.cpu().numpy().reshape(-1), rc[GUARD:GUARD + 4].cpu().numpy())
            edge = torch.stack((buf[8:10], buf[pitch + 8:pitch + 10])).cpu().numpy()
            sent = _bits(np.array([SENTINEL]))[0]
            assert np.all(_bits(edge) == sent) and np.all(_bits(rc[:GUARD].cpu().numpy()) == sent) \
                and np.all(_bits(rc[GUARD + 4:].cpu().numpy()) == sent)
            assert np.array_equal(_bits(u.cpu().numpy()), _bits(f["u"].reshape(2, 2)))
            worst = 0.0
            for g, w, b in zip(got, ref, bnd):
                err = np.abs(g.astype(LD) - w)
                assert np.all(err[b == 0] == 0)
                worst = max(worst, float((err[b > 0] / (L * LD(U53) * b[b > 0])).max()))
            print("NSRATIO offset-boundary", f"pitch={pitch}", f"{worst:.3f}")
            assert worst <= SLACK
    finally:
        del buf
        torch.cuda.empty_cache()


def test_argument_checks(gpu):
    """The raw ABI's refusals, by status and message; a call without outputs is SEM_OK and touches nothing."""
    from sem_amd import _lib as Lb
    from sem_amd.device import Mesh
    lib = Lb.load()
    mesh = Mesh(2, 2, 2, DX, DY)
    n, NY = mesh.n_local, mesh.NY
    r = np.random.default_rng(2)
    u, v, p = (_dev(r.uniform(-1, 1, n)) for _ in range(3))
    ru, rv, rc = (torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(3))
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    stream = mesh.stream_ptr()

    def call(h, d, u_=u, v_=v, outs=(ru, rv, rc)):
        st = lib.sem_ns_apply(h, None if d is None else C.byref(d), ptr(u_), ptr(v_), ptr(p),
                              *(None if o is None else ptr(o) for o in outs), stream)
        return st, lib.sem_last_error().decode(errors="replace")

    def desc(**kw):
        d = Lb.SemNsDesc()
        d.c_stiff, d.c_div, d.pin = 1.0, 1.0, -1
        for k, x in kw.items():
            setattr(d, k, x)
        return d

    for h, d, text in ((None, desc(), "null argument"), (mesh._h, None, "null argument"),
                       (mesh._h, desc(uv_pitch=NY - 1), "uv_pitch below the line length"),
                       (mesh._h, desc(uv_pitch=1), "uv_pitch below the line length"),
                       (mesh._h, desc(pin=-2), "pinned node out of range"),
                       (mesh._h, desc(pin=mesh.NX * NY), "pinned node out of range")):
        st, msg = call(h, d)
        assert st == Lb.SEM_EINVAL and text in msg
    # cu == u / cv == v by pointer with a line view: the two forms would read different nodes -- refused
    big = _dev(r.uniform(-1, 1, mesh.NX * 2 * NY))
    for k, operand in (("cu", "u"), ("cv", "v")):
        for pitch in (2 * NY, NY + 1):
            st, msg = call(mesh._h, desc(uv_pitch=pitch, **{k: big.data_ptr()}), **{operand + "_": big})
            assert st == Lb.SEM_EINVAL and f"{k} aliases {operand}" in msg
    # ... and accepted for plain vectors, whichever way the pitch says so
    for pitch in (0, NY):
        st, _ = call(mesh._h, desc(uv_pitch=pitch, cu=u.data_ptr(), cv=v.data_ptr()))
        assert st == Lb.SEM_OK
    torch.cuda.synchronize()
    assert not np.any(_bits(ru.cpu().numpy()) == _bits(np.array([SENTINEL]))[0])
    # no output at all: SEM_OK, nothing launched, nothing written
    keep = [t.clone() for t in (u, v, p)]
    for o in (ru, rv, rc):
        o.fill_(SENTINEL)
    st, _ = call(mesh._h, desc(), outs=(None, None, None))
    torch.cuda.synchronize()
    assert st == Lb.SEM_OK
    for t, k in zip((u, v, p), keep):
        assert torch.equal(t, k)
    for o in (ru, rv, rc):
        assert np.all(_bits(o.cpu().numpy()) == _bits(np.array([SENTINEL]))[0])
