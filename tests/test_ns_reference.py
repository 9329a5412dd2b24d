"""Pins tests/ns_reference.py (the np.longdouble restatement of sem_ns_apply that the GPU launch tests compare the
kernels with) to the golden-pinned oracle, so that it cannot drift on its own: the whole mesh against
NSOracle.residuals / dresiduals with the descriptor NavierStokesSolver passes, strips against the float64 oracle
composition CPUStripMesh.ns_apply, and the strips' interface lines summed against the whole mesh.

Bound per row: |oracle - ref| <= 2 L 2^-53 (|A| |x|)_r, with (|A| |x|)_r from ns_reference(absval=True) and L the
chain length of the float64 composition it is compared with:
  * CPUStripMesh.ns_apply sums a row from sum-factorised element applies: P + 1 products for the derivative, P + 1
    for its transpose, and about 8 more roundings (the weights and metric factors, the direct-stiffness sum, the
    coefficient, the sums of the operators and pointwise terms): L = 2 (P + 1) + 8;
  * NSOracle multiplies assembled CSR rows: at an element corner Sys has the 2 (2 P + 1) - 1 entries of its two
    lines, each entry carrying the roundings of its own assembly (tensor product, duplicate sum, Re diag(u) G, the
    sum with K: about 6), then the G p row and b are added: L = 4 (P + 1) + 8."""
import numpy as np
import pytest
import torch

from ns_reference import LD, ns_reference, strip_shape

U53 = 2.0 ** -53
DX, DY = 0.37, 0.23
COEF = dict(c_mass=0.75, c_stiff=1.0, c_gradx=310.0, c_grady=-270.0, c_T=-0.4)


def _within(got, ref, bound, L):
    """max over rows of |got - ref| / (2 L 2^-53 bound_r); rows with a zero bound must agree exactly."""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref)
    lim = 2 * L * LD(U53) * bound
    assert np.all(err[bound == 0] == 0)
    nz = bound > 0
    return float((err[nz] / lim[nz]).max()) if nz.any() else 0.0


def _fields(n, seed, names):
    r = np.random.default_rng(seed)
    return {k: r.uniform(-1, 1, n) for k in names}


@pytest.mark.parametrize("P,nex,ney", [(1, 4, 3), (2, 3, 2), (3, 3, 3), (5, 2, 3), (8, 2, 2)])
def test_whole_mesh_matches_ns_oracle(P, nex, ney):
    """(3, 3, 3) has NX = NY = 10: the pin int(N / 2) = 50 lies on y = 0, where the two statement orders differ."""
    from oracle import sem_oracle as O
    Re, Gr = 400.0, 30.0
    ref = O.NSOracle(nex * DX, ney * DY, Re, Gr, P, nex, ney, u_N=1.0, v_W=0.25)
    N = ref.N
    f = _fields(N, 11 * P + nex, ("u", "v", "p", "T", "du", "dv", "dp", "dT"))
    geo = (P, nex, ney, DX, DY, 0, nex)
    mask = ref.mask_bound.astype(np.uint8)
    pin = int(N / 2)
    L = 4 * (P + 1) + 8

    kw = dict(c_stiff=1.0, c_gradx=Re, c_grady=Re, cu=f["u"], cv=f["v"], c_T=-ref.GoR, T=f["T"],
              dval_u=np.nan_to_num(ref.dir_u), dval_v=np.nan_to_num(ref.dir_v), dir_mask=mask, pin=pin, pin_val=0.0,
              pin_first=True)
    got = ref.residuals(f["u"], f["v"], f["p"], f["T"])
    want = ns_reference(*geo, f["u"], f["v"], f["p"], **kw)
    bound = ns_reference(*geo, f["u"], f["v"], f["p"], absval=True, **kw)
    for g, w, b in zip(got, want, bound):
        assert _within(g, w, b, L) <= 1.0

    ref.calc_jacobians(f["u"], f["v"])
    jac = dict(juu=(ref.Juu - ref.Sys).diagonal(), jvv=(ref.Jvv - ref.Sys).diagonal(), juv=ref.Juv.diagonal(),
               jvu=ref.Jvu.diagonal())
    for dT in (f["dT"], None):
        kw = dict(c_stiff=1.0, c_gradx=Re, c_grady=Re, cu=f["u"], cv=f["v"], c_T=-ref.GoR if dT is not None else 0.0,
                  T=dT, dir_mask=mask, pin=pin, pin_val=0.0, pin_first=False, **jac)
        got = ref.dresiduals(f["du"], f["dv"], f["dp"], dT)
        want = ns_reference(*geo, f["du"], f["dv"], f["dp"], **kw)
        bound = ns_reference(*geo, f["du"], f["dv"], f["dp"], absval=True, **kw)
        for g, w, b in zip(got, want, bound):
            assert _within(g, w, b, L) <= 1.0


NAMES = ("u", "v", "p", "T", "cu", "cv", "juu", "juv", "jvu", "jvv", "dval_u", "dval_v")
NEX, NEY = 4, 2
STRIPS = [(0, 4), (0, 1), (1, 3), (3, 4)]     # whole mesh, left, middle (two interface lines), right


def _strip(P, eb, ee, g):
    """The strip's lines of the whole-mesh fields g."""
    lines, NY, l0 = strip_shape(P, NEX, NEY, eb, ee)
    return {k: (a[l0 * NY:(l0 + lines) * NY].copy() if a is not None else None) for k, a in g.items()}


def _pins(P):
    NY = NEY * P + 1
    # on the boundary (y = 0) and inside, each on a line inside strip (1, 3) and on the line strips (0, 1), (1, 3) share
    return [("boundary", 2 * P * NY), ("interior", 2 * P * NY + 1), ("shared-boundary", P * NY),
            ("shared-interior", P * NY + 1)]


@pytest.mark.parametrize("pin_first", [True, False])
@pytest.mark.parametrize("P", [1, 2, 5, 8])
def test_strips_match_the_float64_composition(P, pin_first):
    from cpu_mesh import CPUStripMesh
    NX, NY = NEX * P + 1, NEY * P + 1
    g = _fields(NX * NY, 5 * P + pin_first, NAMES)
    L = 2 * (P + 1) + 8
    worst = 0.0
    for _, pin in _pins(P):
        whole = None
        total = [np.zeros(NX * NY, dtype=LD) for _ in range(3)]
        for eb, ee in STRIPS:
            s = _strip(P, eb, ee, g)
            kw = dict(COEF, c_div=-1.0, dir_sides=15, pin=pin, pin_val=0.3, pin_first=pin_first,
                      **{k: s[k] for k in NAMES[3:]})
            geo = (P, NEX, NEY, DX, DY, eb, ee)
            want = ns_reference(*geo, s["u"], s["v"], s["p"], **kw)
            bound = ns_reference(*geo, s["u"], s["v"], s["p"], absval=True, **kw)
            m = CPUStripMesh(*geo)
            t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
            outs = [torch.full((m.n_local,), np.nan, dtype=torch.float64) for _ in range(3)]
            tk = {k: (t(x) if isinstance(x, np.ndarray) else x) for k, x in kw.items()}
            m.ns_apply(t(s["u"]), t(s["v"]), t(s["p"]), *outs, **tk)
            for o, w, b in zip(outs, want, bound):
                worst = max(worst, _within(o.numpy(), w, b, L))
            if (eb, ee) == (0, NEX):
                whole = want
            else:   # the interface exchange: shared lines summed
                l0 = eb * P * NY
                for acc, w in zip(total, want):
                    acc[l0:l0 + w.size] += w
        # strips (0,1), (1,3), (3,4) tile the mesh: their sum over the shared lines is the whole-mesh reference
        # (to the rounding of adding two partial sums in long double)
        bound = ns_reference(P, NEX, NEY, DX, DY, 0, NEX, g["u"], g["v"], g["p"], absval=True,
                             **dict(COEF, c_div=-1.0, dir_sides=15, pin=pin, pin_val=0.3, pin_first=pin_first,
                                    **{k: g[k] for k in NAMES[3:]}))
        for acc, w, b in zip(total, whole, bound):
            assert np.all(np.abs(acc - w) <= 8 * np.finfo(LD).eps * b)
    assert worst <= 1.0


def test_absent_operands_and_mask():
    """NULL operands are zeros (cu, cv ones), a mask (interior nodes included) wins over dir_sides: against the
    float64 composition on a middle strip."""
    from cpu_mesh import CPUStripMesh
    P, eb, ee = 3, 1, 3
    geo = (P, NEX, NEY, DX, DY, eb, ee)
    m = CPUStripMesh(*geo)
    n = m.n_local
    s = _fields(n, 3, NAMES)
    mask = (np.random.default_rng(4).random(n) < 0.25).astype(np.uint8)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    base = dict(COEF, c_div=-1.0, dir_mask=mask, dir_sides=5, pin=(eb * P + 1) * m.NY + 2, pin_val=0.3,
                **{k: s[k] for k in NAMES[3:]})
    for drop in (("cu", "cv"), ("juu", "jvv"), ("juv", "jvu"), ("T",), ("dval_u", "dval_v"), ("u",), ("v",), ("p",)):
        kw = dict(base)
        ops = {k: s[k] for k in ("u", "v", "p")}
        for k in drop:
            if k in ops:
                ops[k] = None
            else:
                kw[k] = None
        want = ns_reference(*geo, ops["u"], ops["v"], ops["p"], **kw)
        bound = ns_reference(*geo, ops["u"], ops["v"], ops["p"], absval=True, **kw)
        outs = [torch.full((n,), np.nan, dtype=torch.float64) for _ in range(3)]
        tk = {k: (t(x) if isinstance(x, np.ndarray) else x) for k, x in kw.items()}
        m.ns_apply(t(ops["u"]), t(ops["v"]), t(ops["p"]), *outs, **tk)
        for o, w, b in zip(outs, want, bound):
            assert _within(o.numpy(), w, b, 2 * (P + 1) + 8) <= 1.0
