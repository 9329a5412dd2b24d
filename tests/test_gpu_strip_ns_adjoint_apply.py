"""GPU tests of sem_ns_apply_transpose_part (sem_amd/csrc/ns_apply_transpose.hip) through Mesh.ns_apply_transpose_part:
the transposed Navier-Stokes apply of a handle's own matrix A_s, every strip its own handle on one GPU.

1. against tests/ns_reference_T_strip.py (np.longdouble, pinned to ns_reference by tests/test_ns_reference_T_strip.py):
   P = 1..16, the strips (0,2), (2,3), (3,5) of nex = 5, ney = TYE + {-1, 0, 1}, the four forms plus yT, uv_pitch NY
   and 2 NY with gaps and guards against sentinels bit for bit, the Dirichlet and pin variants of
   ns_reference_T_strip.strip_variants;
2. against the strip's own forward operator: A_s dense from Mesh.ns_apply on the identity columns of the same handle;
3. assembled (pack, sum, unpack over bounds [0, 2, 3, 5]) against Mesh.ns_apply_transpose on the whole mesh;
4. the dot identity <A_s x, z> = <x, A_s^T z> on a one-column middle strip and a three-column one;
5. a whole-mesh handle: bitwise Mesh.ns_apply_transpose in every form;
6. repeatability and graph replay;  7. the argument checks of the header, outputs untouched.

Tolerances.  Against the long-double helper: the per-row first-order bound of test_gpu_ns_apply_transpose_launches.py,
unchanged -- |got_r - ref_r| <= SLACK L 2^-53 (|A_s^T| |z|)_r with L = 2 (P + 1) + 16 (derived there from the kernel's
code; a strip runs the same chains or, on a right interface line, shorter ones), SLACK = 2 and (|A_s^T| |z|)_r the
helper's absval in the strip form.  Against float64 references (the forward kernel, the whole-mesh kernel): 1e-13 of
max|ref|.  Every sweep prints its largest ratio / error."""
import ctypes as C

import numpy as np
import pytest
import torch

from ns_reference import LD, strip_shape, uv_index
from ns_reference_T_strip import ns_reference_T_strip, strip_variants

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
SLACK = 2.0
TOL = 1e-13
SENTINEL = -7.25e77
GUARD = 37                       # sentinel entries before and after every output
DX, DY = 0.37, 0.23
COEF = dict(c_mass=0.75, c_stiff=1.0, c_gradx=310.0, c_grady=-270.0)
NAMES = ("zu", "zv", "zc", "cu", "cv", "juu", "juv", "jvu", "jvv")
OUTS = ("yu", "yv", "yp", "yT")
FORMS = ("full", "grad", "div", "vel")
NEX = 5
STRIPS = [(0, 2), (2, 3), (3, 5)]   # a left strip, a one-column middle strip, a right strip


def _tye(P):
    """The kernel's y tile in elements (NsTTile::TYE)."""
    return max(32 // P, 1)


def _chain(P):
    return 2 * (P + 1) + 16


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _rel(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


class _Handle:
    """One handle (a strip or a whole mesh) and one set of random fields (uniform in (-1, 1), fixed seed) on its nodes."""

    def __init__(self, P, nex, ney, eb, ee, seed):
        from sem_amd.device import Mesh
        self.geo = (P, nex, ney, DX, DY, eb, ee)
        self.P, self.nex, self.ney = P, nex, ney
        self.mesh = Mesh(*self.geo)
        self.lines, self.NY, _ = strip_shape(P, nex, ney, eb, ee)
        self.n = self.lines * self.NY
        assert self.mesh.n_local == self.n and self.mesh.NY == self.NY
        r = np.random.default_rng(seed)
        self.f = {k: r.uniform(-1, 1, self.n) for k in NAMES}
        self.d = {k: _dev(v) for k, v in self.f.items()}

    def form(self, name, rows):
        """(ins, outs, host descriptor) of the four specialised forms; `rows`: dir_sides, dir_mask, pin, pin_first."""
        f = self.f
        jac = dict(COEF, cu=f["cu"], cv=f["cv"], juu=f["juu"], juv=f["juv"], jvu=f["jvu"], jvv=f["jvv"])
        if name == "full":      # everything, with the temperature bar
            return ("zu", "zv", "zc"), OUTS, dict(jac, c_T=-0.4, c_div=1.0, **rows)
        if name == "grad":      # the transposed gradient (-C^T q)
            return ("zc",), ("yu", "yv"), dict(rows, c_div=-1.0)
        if name == "div":       # the transposed divergence (B^T x + E^T q)
            return ("zu", "zv", "zc"), ("yp",), dict(rows)
        if name == "vel":       # the velocity rows alone (J^T x)
            return ("zu", "zv"), ("yu", "yv"), dict(jac, **rows)
        raise KeyError(name)

    def dkw(self, kw):
        """The descriptor with its arrays on the device (the fields' copies are kept)."""
        out = {}
        for k, x in kw.items():
            if isinstance(x, np.ndarray):
                x = self.d[k] if k in self.d and x is self.f[k] else _dev(x)
            out[k] = x
        return out

    def launch(self, ins, outs, kw, pitch=0, entry=None):
        """One launch into sentinel-filled buffers; returns the outputs on the host after checking that nothing else
        was written (guards, the gaps of a line view, outputs that were not requested)."""
        n, NY, lines = self.n, self.NY, self.lines
        entry = entry or self.mesh.ns_apply_transpose_part
        idx = uv_index(lines, NY, pitch)
        span = lines * (pitch or NY)
        sent = _bits(np.array([SENTINEL]))[0]
        if pitch:
            assert pitch >= 2 * NY
            B = np.full(span, np.nan)
            for k, o in (("zu", 0), ("zv", NY)):
                if k in ins:
                    B[o + idx] = self.f[k]
            dB = _dev(B)
            view = lambda t, o: torch.as_strided(t, (lines, NY), (pitch, 1), o)   # noqa: E731
            d_in = {k: (view(dB, o) if k in ins else None) for k, o in (("zu", 0), ("zv", NY))}
            R = torch.full((span + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
            d_out = {k: (view(R, GUARD + o) if k in outs else None) for k, o in (("yu", 0), ("yv", NY))}
            bufs = {}
        else:
            d_in = {k: (self.d[k] if k in ins else None) for k in ("zu", "zv")}
            bufs = {k: torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
                    for k in ("yu", "yv") if k in outs}
            d_out = {k: (bufs[k][GUARD:GUARD + n] if k in bufs else None) for k in ("yu", "yv")}
        plain = {k: torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda") for k in ("yp", "yT")}
        entry(d_in["zu"], d_in["zv"], self.d["zc"] if "zc" in ins else None, d_out["yu"], d_out["yv"],
              plain["yp"][GUARD:GUARD + n] if "yp" in outs else None,
              plain["yT"][GUARD:GUARD + n] if "yT" in outs else None, **self.dkw(kw))
        torch.cuda.synchronize()
        res = {}
        if pitch:
            h = R.cpu().numpy()
            keep = np.ones(h.size, dtype=bool)
            for k, o in (("yu", 0), ("yv", NY)):
                if k in outs:
                    res[k] = h[GUARD + o + idx].copy()
                    keep[GUARD + o + idx] = False
            assert np.all(_bits(h)[keep] == sent), "a line view's gap, guard or unrequested half was written"
        for k, b in list(bufs.items()) + list(plain.items()):
            h = b.cpu().numpy()
            if k in outs:
                res[k] = h[GUARD:GUARD + n].copy()
                assert np.all(_bits(h[:GUARD]) == sent) and np.all(_bits(h[GUARD + n:]) == sent), f"{k} guard"
            else:
                assert np.all(_bits(h) == sent), f"{k} was written though not requested"
        return res

    def check(self, ins, outs, kw, pitch=0):
        """One launch against the long-double helper; returns the largest ratio to the first-order bound."""
        L = _chain(self.P)
        got = self.launch(ins, outs, kw, pitch)
        host = [self.f[k] if k in ins else None for k in ("zu", "zv", "zc")]
        ref = dict(zip(OUTS, ns_reference_T_strip(*self.geo, *host, **kw)))
        bnd = dict(zip(OUTS, ns_reference_T_strip(*self.geo, *host, absval=True, **kw)))
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
        return worst


# ------------------------------------------------------------------ 1. against the long-double helper
@pytest.mark.parametrize("P", range(1, 17))
def test_against_long_double_reference(gpu, P):
    """Every (strip, ney) runs every Dirichlet x pin variant in all four forms (the full one with yT); the pitch (NY or
    2 NY) alternates with the variant, the form, the strip and ney, so that over the nine (strip, ney) pairs every
    variant meets every form at both pitches."""
    T = _tye(P)
    ratios = {}
    for si, (eb, ee) in enumerate(STRIPS):
        for ki, ney in enumerate((T - 1, T, T + 1)):
            s = _Handle(P, NEX, ney, eb, ee, seed=1000 * P + 10 * ney + eb)
            for i, rows in enumerate(strip_variants(P, NEX, ney, eb, ee)):
                t = i + si + ki
                for fi, name in enumerate(FORMS):
                    pitch = ((t + fi) % 2) * 2 * s.NY
                    ins, outs, kw = s.form(name, rows)
                    try:
                        r = s.check(ins, outs, kw, pitch)
                    except AssertionError as e:
                        tag = {k: v for k, v in rows.items() if k != "dir_mask"}
                        raise AssertionError(f"strip [{eb},{ee}) ney={ney} {name} pitch={pitch} "
                                             f"{'mask' if rows['dir_mask'] is not None else 'sides'} {tag}: {e}") from e
                    ratios[name] = max(ratios.get(name, 0.0), r)
    print("NSTSTRIPRATIO", f"P={P}", " ".join(f"{k}={v:.3f}" for k, v in sorted(ratios.items())))


# ------------------------------------------------------------------ 2. the strip's own forward operator
def _dense_forward_T(s, kw, c_T):
    """(A_s^T, the transpose of its T column block) dense: row j = A_s e_j, from Mesh.ns_apply on the identity columns
    of the same handle."""
    n, m = s.n, s.mesh
    eye = torch.eye(n, dtype=torch.float64, device="cuda")
    AT = torch.empty(3 * n, 3 * n, dtype=torch.float64, device="cuda")
    TT = torch.empty(n, n, dtype=torch.float64, device="cuda")
    for j in range(3 * n):
        ops = [None, None, None]
        ops[j // n] = eye[j % n]
        m.ns_apply(*ops, AT[j, :n], AT[j, n:2 * n], AT[j, 2 * n:], **kw)
    for j in range(n):
        m.ns_apply(None, None, None, None, TT[j], None, c_T=c_T, T=eye[j], **kw)
    return AT, TT


@pytest.mark.parametrize("eb,ee", STRIPS)
@pytest.mark.parametrize("P", [1, 3, 4, 8, 12, 16])
def test_against_own_forward_operator(gpu, P, eb, ee):
    s = _Handle(P, NEX, 2, eb, ee, seed=31 * P + eb)
    var = strip_variants(P, NEX, 2, eb, ee)
    z = torch.cat([s.d[k] for k in ("zu", "zv", "zc")])
    for name, rows in (("sides, pin on the last line", var[2]), ("mask, Dirichlet pin on the last line", var[16])):
        ins, outs, kw = s.form("full", rows)
        dkw = s.dkw(kw)
        c_T = dkw.pop("c_T")
        AT, TT = _dense_forward_T(s, dkw, c_T)
        want = torch.cat([AT @ z, TT @ s.d["zv"]]).cpu().numpy()
        got = s.launch(ins, outs, kw)
        err = max(_rel(got[k], want[i * s.n:(i + 1) * s.n]) for i, k in enumerate(OUTS))
        print(f"P={P} strip [{eb},{ee}) {name}: {err:.3e}")
        assert err <= TOL, name


# ------------------------------------------------------------------ 3. assembled against the whole mesh
def _assemble(bounds, strips, ys):
    """Pack, sum over strips, unpack: what the forward exchange does with every output."""
    G = len(bounds) - 1
    for k in ys[0]:
        bufs = []
        for s, y in zip(strips, ys):
            buf = torch.empty((G - 1) * s.mesh.NY, dtype=torch.float64, device="cuda")
            s.mesh.interface_pack(y[k], bounds, buf)
            bufs.append(buf)
        total = torch.stack(bufs).sum(0)
        for s, y in zip(strips, ys):
            s.mesh.interface_unpack(total, bounds, y[k])


@pytest.mark.parametrize("dney", [-1, 0, 1])
@pytest.mark.parametrize("P", range(1, 17))
def test_assembled_against_whole_mesh(gpu, P, dney):
    ney = _tye(P) + dney             # >= 1: TYE >= 2 for P <= 16
    bounds = [0, 2, 3, 5]
    full = _Handle(P, NEX, ney, 0, NEX, seed=7 * P + ney)
    NY = full.NY
    # the pin: the reference solver's N / 2; a node of the first interface line; a Dirichlet node of the second one
    pin = {-1: full.n // 2, 0: 2 * P * NY + 1, 1: 3 * P * NY}[dney]
    rows = dict(dir_sides=15, dir_mask=None, pin=pin, pin_first=False)
    ins, outs, kw = full.form("full", rows)
    want = full.mesh.ns_apply_transpose(*(full.d[k] for k in ins),
                                        *(torch.empty(full.n, dtype=torch.float64, device="cuda") for _ in outs),
                                        **full.dkw(kw))
    strips, ys = [], []
    for eb, ee in zip(bounds[:-1], bounds[1:]):
        s = _Handle(P, NEX, ney, eb, ee, seed=0)
        sl = slice(s.mesh.dof_begin, s.mesh.dof_begin + s.n)
        loc = {k: (full.d[k][sl].contiguous() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        y = {k: torch.empty(s.n, dtype=torch.float64, device="cuda") for k in outs}
        s.mesh.ns_apply_transpose_part(*(full.d[k][sl].contiguous() for k in ins), *(y[k] for k in outs), **loc)
        strips.append((s, sl))
        ys.append(y)
    _assemble(bounds, [s for s, _ in strips], ys)
    err = max(_rel(y[k], want[i][sl]) for (s, sl), y in zip(strips, ys) for i, k in enumerate(outs))
    print(f"P={P} 5x{ney} pin={pin} assembled vs whole-mesh kernel: {err:.3e}")
    assert err <= TOL


# ------------------------------------------------------------------ 4. the dot identity
@pytest.mark.parametrize("P", [2, 5, 8])
def test_dot_identity(gpu, P):
    """<A_s x, z> = <x, A_s^T z> on a one-column middle strip and on a three-column one (both end lines interfaces).
    Both applies are right to 1e-13 of their largest entry per row, so the two inner products
    differ by at most 1e-13 (max|A_s x| |z|_1 + max|A_s^T z| |x|_1)."""
    ney = _tye(P) + 1
    for eb, ee in ((3, 4), (2, 5)):
        s = _Handle(P, 7, ney, eb, ee, seed=13 * P + eb)
        var = strip_variants(P, 7, ney, eb, ee)
        for rows in (var[2], var[11]):      # sides with a pin on the right interface line; a mask with a free pin there
            _, _, kw = s.form("full", rows)
            dkw = s.dkw(kw)
            dkw.pop("c_T")
            x = [s.d[k] for k in ("cu", "juu", "jvv")]      # any three fields serve as (u, v, p)
            z = [s.d[k] for k in ("zu", "zv", "zc")]
            Ax = [torch.empty_like(x[0]) for _ in range(3)]
            ATz = [torch.empty_like(x[0]) for _ in range(3)]
            s.mesh.ns_apply(*x, *Ax, **dkw)
            s.mesh.ns_apply_transpose_part(*z, *ATz, **dkw)
            lhs = sum(torch.dot(a, b).item() for a, b in zip(Ax, z))
            rhs = sum(torch.dot(a, b).item() for a, b in zip(x, ATz))
            bound = TOL * (max(a.abs().max().item() for a in Ax) * sum(b.abs().sum().item() for b in z)
                           + max(a.abs().max().item() for a in ATz) * sum(b.abs().sum().item() for b in x))
            print(f"P={P} strip [{eb},{ee}): lhs {lhs:.15e} rhs {rhs:.15e} diff {abs(lhs - rhs):.3e} bound {bound:.3e}")
            assert abs(lhs - rhs) <= bound


# ------------------------------------------------------------------ 5. a whole-mesh handle
@pytest.mark.parametrize("P", [1, 4, 7, 12, 16])
def test_whole_mesh_handle_is_bitwise_the_old_entry_point(gpu, P):
    s = _Handle(P, 3, _tye(P) + 1, 0, 3, seed=3 * P)
    for rows in strip_variants(P, 3, s.ney, 0, 3)[1::4]:
        for name in FORMS:
            for pitch in (0, 2 * s.NY):
                ins, outs, kw = s.form(name, rows)
                new = s.launch(ins, outs, kw, pitch)
                old = s.launch(ins, outs, kw, pitch, entry=s.mesh.ns_apply_transpose)
                for k in outs:
                    assert np.array_equal(_bits(new[k]), _bits(old[k])), (name, pitch, k)


# ------------------------------------------------------------------ 6. repeatability
@pytest.mark.parametrize("P,nex,eb,ee", [(8, 5, 2, 3), (4, 7, 1, 6), (12, 5, 3, 5)])
def test_repeatable_and_graph_replay(gpu, P, nex, eb, ee):
    from sem_amd.device import no_gc
    s = _Handle(P, nex, _tye(P) + 1, eb, ee, seed=P + nex)
    rows = strip_variants(P, nex, s.ney, eb, ee)[2]
    ins, outs, kw = s.form("full", rows)
    dkw = s.dkw(kw)
    z = [s.d[k] for k in ins]
    new = lambda: [torch.zeros(s.n, dtype=torch.float64, device="cuda") for _ in outs]   # noqa: E731
    eager, again, y = new(), new(), new()
    s.mesh.ns_apply_transpose_part(*z, *eager, **dkw)
    s.mesh.ns_apply_transpose_part(*z, *again, **dkw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with no_gc(), torch.cuda.graph(g):
        s.mesh.ns_apply_transpose_part(*z, *y, **dkw)
    for t in y:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b, c in zip(eager, again, y):
        assert a.abs().max().item() > 0
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        assert torch.equal(a.view(torch.int64), c.view(torch.int64))


# ------------------------------------------------------------------ 7. argument checks
def test_argument_checks(gpu):
    """The raw ABI's refusals on a strip handle, by status and message, each leaving the sentinel-filled outputs
    untouched; what the whole-mesh entry point refuses for being a strip is accepted here."""
    from sem_amd import _lib as Lb
    from sem_amd.device import Mesh
    lib = Lb.load()
    mesh = Mesh(2, 3, 2, DX, DY, 1, 2)       # a one-column middle strip: 3 lines
    n, NY, lines = mesh.n_local, mesh.NY, 3
    r = np.random.default_rng(2)
    zu, zv, zc, aux = (_dev(r.uniform(-1, 1, n)) for _ in range(4))
    yu, yv, yp, yT = (torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(4))
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    stream = mesh.stream_ptr()
    sent = _bits(np.array([SENTINEL]))[0]

    def call(h, d, ins=(zu, zv, zc), outs=(yu, yv, yp, yT)):
        st = lib.sem_ns_apply_transpose_part(h, None if d is None else C.byref(d), *(ptr(t) for t in ins),
                                             *(ptr(t) for t in outs), stream)
        return st, lib.sem_last_error().decode(errors="replace")

    def desc(**kw):
        d = Lb.SemNsDesc()
        d.c_stiff, d.c_div, d.pin = 1.0, 1.0, -1
        for k, x in kw.items():
            setattr(d, k, x)
        return d

    def untouched():
        torch.cuda.synchronize()
        return all(np.all(_bits(o.cpu().numpy()) == sent) for o in (yu, yv, yp, yT))

    inval = [(None, desc(), {}, "null argument"), (mesh._h, None, {}, "null argument"),
             (mesh._h, desc(uv_pitch=NY - 1), {}, "uv_pitch below the line length"),
             (mesh._h, desc(pin=-2), {}, "pinned node out of range"),
             (mesh._h, desc(pin=mesh.NX * NY), {}, "pinned node out of range"),      # N of the whole mesh
             (mesh._h, desc(T=aux.data_ptr()), {}, "T, dval_u, dval_v must be NULL"),
             (mesh._h, desc(dval_u=aux.data_ptr()), {}, "T, dval_u, dval_v must be NULL"),
             (mesh._h, desc(dval_v=aux.data_ptr()), {}, "T, dval_u, dval_v must be NULL"),
             (mesh._h, desc(pin_val=0.5), {}, "pin_val 0")]
    for src in (zu, zv, zc):                          # every output against every input
        for j in range(4):
            outs = [yu, yv, yp, yT]
            outs[j] = src
            inval.append((mesh._h, desc(), dict(outs=tuple(outs)), "an output aliases an input"))
    big = _dev(r.uniform(-1, 1, lines * 2 * NY))
    for k in ("cu", "cv"):                            # cu / cv by pointer on a line view names other nodes
        for pitch in (2 * NY, NY + 1):
            inval.append((mesh._h, desc(uv_pitch=pitch, **{k: big.data_ptr()}), dict(ins=(big, zv, zc)),
                          f"{k} aliases zu or zv"))
            inval.append((mesh._h, desc(uv_pitch=pitch, **{k: big.data_ptr()}), dict(ins=(zu, big, zc)),
                          f"{k} aliases zu or zv"))
    keep = [t.clone() for t in (zu, zv, zc)]
    for h, d, kw, text in inval:
        st, msg = call(h, d, **kw)
        assert st == Lb.SEM_EINVAL and text in msg, (text, st, msg)
    assert untouched()
    for t, k in zip((zu, zv, zc), keep):              # an aliased "output" was not written either
        assert torch.equal(t, k)
    # SEM_EUNSUPPORTED: offsets past 32 bits on the strip's own lines (refused before any pointer is used)
    st, msg = call(mesh._h, desc(uv_pitch=2 ** 30))
    assert (lines - 1) * 2 ** 30 + NY > 2 ** 31 - 1
    assert st == Lb.SEM_EUNSUPPORTED and "32-bit node-offset limit" in msg and "sem_ns_apply_transpose_part" in msg
    # a handle of another device than the current one, and an order without a compiled kernel: the handle's fields are
    # overwritten and put back (struct sem_handle, sem_internal.h: int P, nex, ney, ex_begin, ex_end, device)
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
    assert untouched()
    # no output at all: SEM_OK, nothing launched, nothing written
    st, _ = call(mesh._h, desc(), outs=(None, None, None, None))
    assert st == Lb.SEM_OK and untouched()
    for t, k in zip((zu, zv, zc), keep):
        assert torch.equal(t, k)
    # the strip itself is no refusal, and a pin of the mesh outside the strip is accepted (no pin)
    for pin in (-1, 0, mesh.NX * NY - 1):
        st, msg = call(mesh._h, desc(pin=pin))
        assert st == Lb.SEM_OK, msg
    torch.cuda.synchronize()
    assert not any(np.any(_bits(o.cpu().numpy()) == sent) for o in (yu, yv, yp))
