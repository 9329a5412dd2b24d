"""Test helper (not a test module): the Jacobian pieces sem_velocity_blocks and sem_condensed_blocks write
(sem_amd/csrc/ns_velocity.hip, include/sem_ops.h sem_velocity_desc) restated in np.longdouble, entry by entry, on a
whole mesh or an element-column strip [ex_begin, ex_end), with a derived bound per entry.

Reference.  The dense nc n x nc n Jacobian (n = n_local nodes, unknown c n + lx N_y + gy) from Kronecker products of
the assembled 1-D operators of tests/ns_reference.py (ops_1d: the oracle's GLL tables widened, never the library's;
the x operators over the strip's own columns):

    A = cM mx (x) my + cK (Kx (x) diag(my) + diag(mx) (x) Ky)
        + cX diag(cu) (Gx (x) diag(my)) + cY diag(cv) (diag(mx) (x) Gy)
    J = [[A + diag(own juu), diag(own juv)], [diag(own jvu), A + diag(own jvv)]]      (nc = 1: A + diag(own juu))

Rows of the Dirichlet set (ns_reference.dirichlet_rows: dir_mask wins over dir_sides) are identity rows where the
strip owns them and all zero on the non-owned right interface line of a strip with ex_end < nex, where `own` also
removes the pointwise j** terms.  The pieces are cut out of J by index (pieces()): nothing in this module follows the
kernel's row-by-row formulas except kernel_f64, the float64 evaluator the CPU tests use to show that the bound can
fail.

Bound.  |got - ref| <= SLACK L 2^-53 mag per entry, mag the sum of the absolute values of the terms that enter the
entry (a shared node's two element contributions counted separately, as ns_reference(absval=True) does per row).
L is the longest chain of roundings a term goes through, read off ns_velocity.hip:

  * forming a term, 6 roundings at the most.
      mass        fM = c_mass ((dx/2) (dy/2)) in the launcher: 2 (the halvings are exact); the assembled weights
                  mx = w[P] + w[0] and my = w[P] + w[0]: 1 each; fM mx, (fM mx) my: 2.
      stiffness   fKx = c_stiff (dy / dx) in the launcher: 2; my: 1; fx = fKx my: 1; fx Ks: 1; the addition of the
                  convection product in xk(): 1.  The y direction is the same with fKy, mx, fy.
      convection  fX = c_gradx (dy / 2): 1; fX cu: 1; my: 1; (fX cu) my: 1; gxc Gs: 1; the addition in xk(): 1.
  * accumulating the diagonal of a node that is an element corner on an interface line (the longest): dg starts as
    the mass term and takes juu, xk(P, P), xk(0, 0), yk(P, P), yk(0, 0); then row[self] += dg: 6 additions, all of
    which the mass term goes through (every other term fewer; an off-diagonal entry is one term added to zero).
  * 1 because the library's compile-time GLL constants may differ from the oracle's tables in the last place.

So L = 6 + 6 + 1 = 13 for every entry (a contraction into fused multiply-adds only removes roundings).  SLACK = 2
covers the second-order terms, as in the other launch tests.

The tables' own error.  "In the last place" holds for w and G_s = W D, single products, but not for K_s = D^T W D
(GLL.py:73-81): each entry is a float64 sum of P + 1 products w_q D_qi D_qk that cancel, and two float64 evaluations
of it (the oracle's matrix product, the library's loop) agree only to the rounding error of such a sum -- two
roundings per product and P additions, (P + 2) 2^-53 sum_q |w_q D_qi D_qk| each -- which is many units in the last
place of a small entry.  That is the reference's error, not the kernel's, and L does not cover it.  So the stiffness
terms get a second allowance, derived the same way and not measured: T = 2 (P + 2) roundings on tab, the sum of the
absolute stiffness terms with sum_q |w_q D_qi D_qk| in place of |K_s[i][k]|:

    |got - ref| <= SLACK 2^-53 (L mag + T tab).

tab is zero wherever no stiffness term enters, so every entry of the mass, convection and j** terms keeps the plain
bound, and the ratios the tests print are to L mag + T tab.

Exact entries.  Where no term enters (mag = 0: structural zeros, the couplings of a Dirichlet row, everything of a
non-owned Dirichlet row) the entry must compare == 0 (so -0.0 passes); the identity diagonal must be 1 and the
off-component entries, a single operand copied (juv[node], jvu[node]), must have the operand's bits."""
import numpy as np

from condense_reference import nested_index
from ns_reference import LD, dirichlet_rows, ops_1d, strip_shape, tables

U53 = 2.0 ** -53
SLACK = 2.0
L_ROUNDINGS = 13
SENTINEL = -7.25e77
GUARD = 32                      # doubles of guard band on either side of a device array
DX, DY = 0.37, 0.23             # dx != dy, neither a power of two
COEF = dict(c_mass=-0.75, c_stiff=1.7, c_gradx=310.0, c_grady=-27.0)
FIELDS = ("cu", "cv", "juu", "juv", "jvu", "jvv")
DENSE = ("AII", "D", "aIB", "aBI", "E", "F")
IFACE = DENSE[1:]
COND = ("Aii", "Aie", "Aei", "Aed", "Aeu", "Ael")
BOUND, ZERO, EXACT = 0, 1, 2    # how an entry is compared

MASKS = ("sides0", "sides3", "sides4", "sides9", "sides15", "perimeter", "irregular")
DESCS = ("full", "null", "mass", "stiff", "gradx", "grady", "jac")
MUTANTS = ("drop_mass", "swap_dydx", "swap_EF", "swap_aIB_sides", "swap_juv_jvu", "cu_for_y", "first_line_weight",
           "ignore_own", "dir_keeps_aIB", "swap_Aeu_Ael")

# (P, nex, ney, ex_begin, ex_end) the GPU tests run: P = 1 (no interior pieces), P = 2 (one interior line), ney = 1
# (only the two end edges), nex = 1, a one-column strip, first / middle / last strips, and nc (lines) N_y rows below
# (18 at (1, 3, 2)), above and not a multiple of the 256-thread block (578 at P = 16, 650 at P = 12)
SHAPES = [(1, 3, 2, 0, 3), (1, 4, 3, 1, 3), (2, 2, 1, 0, 2), (2, 3, 2, 1, 2), (3, 1, 1, 0, 1), (4, 3, 2, 0, 3),
          (4, 4, 3, 0, 2), (4, 4, 3, 2, 4), (4, 5, 2, 1, 4), (5, 2, 3, 0, 2), (8, 2, 2, 0, 2), (8, 3, 1, 1, 2),
          (12, 1, 2, 0, 1), (16, 1, 1, 0, 1), (16, 2, 1, 1, 2)]


def table_roundings(P):
    """T of the module docstring: two float64 evaluations of K_s = D^T W D."""
    return 2 * (P + 2)


_ABS_K = {}


def abs_stiffness_1d(P, ne, d):
    """sum_q |w_q D_qi D_qk| of the oracle's tables, assembled over ne elements of width d like ops_1d's |K|."""
    key = (P, ne, float(d))
    if key not in _ABS_K:
        from oracle import sem_oracle as O
        w, D = O.gll_nodes(P)[1].astype(LD), np.abs(np.asarray(O.gll_D(P), dtype=np.float64).astype(LD))
        Ks = D.T @ (w[:, None] * D)
        K = np.zeros((ne * P + 1,) * 2, dtype=LD)
        for e in range(ne):
            s = slice(e * P, e * P + P + 1)
            K[s, s] += Ks
        _ABS_K[key] = K * (2 / LD(d))
    return _ABS_K[key]


def handle_kind(nex, eb, ee):
    return "whole" if (eb, ee) == (0, nex) else "first" if eb == 0 else "last" if ee == nex else "middle"


# ---- masks ---------------------------------------------------------------------------------------------------------

def irregular_mask(P, nex, ney, eb, ee, seed=0):
    """A seeded random Dirichlet mask (uint8, n_local) that holds at least: an element-interior node, horizontal-edge
    nodes of an interior line at k = 0, k = ney and (ney > 1) in between, an interface-line node between two edges, an
    element corner, and on strips a node of the first line and a node of the right interface line."""
    lines, NY, _ = strip_shape(P, nex, ney, eb, ee)
    r = np.random.default_rng([seed, P, nex, ney, eb, ee])
    dm = r.random((lines, NY)) < 0.15
    if P > 1:
        dm[1, 1] = True                              # an element interior
        for k in {0, ney, ney // 2}:                 # horizontal edges of the last interior line
            dm[lines - 2, k * P] = True
        dm[P if lines > P + 1 else 0, P - 1] = True  # an interface line between two edges
    dm[(lines - 1) // P // 2 * P, (ney + 1) // 2 * P] = True    # an element corner
    dm[0, NY - 1] = True                             # the first line (a corner of the strip)
    dm[lines - 1, NY // 2] = True                    # the right interface line (not owned when ee < nex)
    return dm.reshape(-1).astype(np.uint8)


def mask_classes(P, ney, dir_mask, lines):
    """Which node classes a mask holds: (element interior, interior-line edge heights k, interface line off the
    edges, element corner, first line, last line)."""
    dm = np.asarray(dir_mask).reshape(lines, -1) != 0
    lx, gy = np.nonzero(dm)
    l, j = lx % P, gy % P
    return dict(interior=bool(np.any((l != 0) & (j != 0))), edge_k=set((gy[(l != 0) & (j == 0)] // P).tolist()),
                interface=bool(np.any((l == 0) & (j != 0))), corner=bool(np.any((l == 0) & (j == 0))),
                first=bool(dm[0].any()), last=bool(dm[-1].any()))


def mask_of(kind, P, nex, ney, eb, ee):
    """(dir_mask or None, dir_sides) of a mask generator's name; a mask comes with dir_sides it must override."""
    if kind.startswith("sides"):
        return None, int(kind[5:])
    if kind == "perimeter":
        return dirichlet_rows(P, nex, ney, eb, ee, None, 15)[0].reshape(-1).astype(np.uint8), 0
    if kind == "irregular":
        return irregular_mask(P, nex, ney, eb, ee), 10
    raise KeyError(kind)


# ---- cases ---------------------------------------------------------------------------------------------------------

def descriptor(kind, nc, f):
    """(coefficients, operand fields) of a descriptor's name from the all-distinct fields f."""
    none = dict.fromkeys(FIELDS)
    zero = dict.fromkeys(COEF, 0.0)
    js = ("juu",) if nc == 1 else ("juu", "juv", "jvu", "jvv")
    pick = lambda *ks: dict(none, **{k: f[k] for k in ks})   # noqa: E731
    if kind == "full":
        return dict(COEF), pick("cu", "cv", *js)
    if kind == "null":
        return dict(COEF), none
    if kind == "mass":
        return dict(zero, c_mass=COEF["c_mass"]), none
    if kind == "stiff":
        return dict(zero, c_stiff=COEF["c_stiff"]), none
    if kind == "gradx":
        return dict(zero, c_gradx=COEF["c_gradx"]), pick("cu")
    if kind == "grady":
        return dict(zero, c_grady=COEF["c_grady"]), pick("cv")
    if kind == "jac":
        return zero, pick(*js)
    raise KeyError(kind)


class Case:
    """One launch: the handle's geometry, ncomp, the descriptor and the column range (global element columns)."""

    def __init__(self, P, nex, ney, eb, ee, nc=2, desc="full", mask="irregular", cols=None, dx=DX, dy=DY, seed=0):
        self.P, self.nex, self.ney, self.eb, self.ee, self.nc = P, nex, ney, eb, ee, nc
        self.dx, self.dy = dx, dy
        self.lines, self.NY, self.l0 = strip_shape(P, nex, ney, eb, ee)
        self.n, self.ne, self.m = self.lines * self.NY, ee - eb, nc * self.NY
        self.nI = (P - 1) * self.m
        self.ne1 = nc * (P - 1)
        self.ni = self.ne1 * (P - 1)
        self.cols = (eb, ee) if cols is None else tuple(cols)
        r = np.random.default_rng([seed, P, nex, ney, eb, ee])
        self.fields = {k: r.uniform(-1, 1, self.n) for k in FIELDS}
        self.desc, self.mask = desc, mask
        self.coef, self.f = descriptor(desc, nc, self.fields)
        self.dir_mask, self.dir_sides = mask_of(mask, P, nex, ney, eb, ee) if isinstance(mask, str) else mask
        self._ref = None

    def geo(self):
        return self.P, self.nex, self.ney, self.eb, self.ee

    def with_operands(self, coef, f, dir_mask, dir_sides):
        """The case with operands given directly (the ties to the oracle)."""
        self.coef, self.f = dict(coef), dict(dict.fromkeys(FIELDS), **f)
        self.dir_mask, self.dir_sides, self._ref = dir_mask, dir_sides, None
        return self

    def shapes(self, layout, ncols=None):
        """Logical shape of every piece of the layout; AII and the condensed pieces for ncols columns."""
        P, m, ne, nI, ney, ne1, ni = self.P, self.m, self.ne, self.nI, self.ney, self.ne1, self.ni
        k = self.cols[1] - self.cols[0] if ncols is None else ncols
        s = dict(D=(ne + 1, m, m), aIB=(ne, P - 1, 2, m), aBI=(ne, 2, P - 1, m), E=(ne, m), F=(ne, m))
        if layout == "dense":
            return dict(AII=(k, nI, nI), **s)
        return dict(Aii=(k, ney, ni, ni), Aie=(k, ney, ni, 2 * ne1), Aei=(k, ney, 2 * ne1, ni),
                    Aed=(k, ney + 1, ne1, ne1), Aeu=(k, ney, ne1, ne1), Ael=(k, ney, ne1, ne1), **s)


# ---- the dense reference -------------------------------------------------------------------------------------------

def dense_jacobian(c):
    """(J, mag, kind): the nc n x nc n Jacobian in np.longdouble, the per-entry sums of absolute terms, and how each
    entry is compared (BOUND, ZERO, EXACT)."""
    if c._ref is not None:
        return c._ref
    P, n, nc = c.P, c.n, c.nc
    mx, Kx, Gx, aKx, aGx = ops_1d(P, c.ne, c.dx)
    my, Ky, Gy, aKy, aGy = ops_1d(P, c.ney, c.dy)
    dmx, dmy = np.diag(mx), np.diag(my)

    def fld(k, fill, a):
        x = c.f[k]
        x = np.full(n, fill, dtype=LD) if x is None else np.asarray(x, dtype=np.float64).astype(LD)
        return np.abs(x) if a else x

    def system(a):
        co = (lambda k: abs(LD(c.coef[k]))) if a else (lambda k: LD(c.coef[k]))
        kx, ky, gx, gy = (aKx, aKy, aGx, aGy) if a else (Kx, Ky, Gx, Gy)
        return (co("c_mass") * np.diag(np.kron(mx, my)) + co("c_stiff") * (np.kron(kx, dmy) + np.kron(dmx, ky))
                + co("c_gradx") * fld("cu", 1.0, a)[:, None] * np.kron(gx, dmy)
                + co("c_grady") * fld("cv", 1.0, a)[:, None] * np.kron(dmx, gy))

    dm, own = dirichlet_rows(*c.geo(), c.dir_mask, c.dir_sides)
    dm, own = dm.reshape(-1), own.reshape(-1)
    ownf = own.astype(LD)
    out = []
    for a in (False, True):
        A = system(a)
        if nc == 1:
            J = A + np.diag(ownf * fld("juu", 0.0, a))
        else:
            J = np.zeros((2 * n, 2 * n), dtype=LD)
            J[:n, :n] = A + np.diag(ownf * fld("juu", 0.0, a))
            J[n:, n:] = A + np.diag(ownf * fld("jvv", 0.0, a))
            J[:n, n:] = np.diag(ownf * fld("juv", 0.0, a))
            J[n:, :n] = np.diag(ownf * fld("jvu", 0.0, a))
        out.append(J)
    J, mag = out
    tabA = abs(LD(c.coef["c_stiff"])) * (np.kron(abs_stiffness_1d(P, c.ne, c.dx), dmy)
                                         + np.kron(dmx, abs_stiffness_1d(P, c.ney, c.dy)))
    tab = np.zeros_like(mag)
    for comp in range(nc):
        tab[comp * n:(comp + 1) * n, comp * n:(comp + 1) * n] = tabA
    kind = np.where(mag == 0, ZERO, BOUND).astype(np.int8)
    q = np.arange(n)
    if nc == 2:
        for k, (r0, c0) in (("juv", (0, n)), ("jvu", (n, 0))):
            if c.f[k] is not None:
                kind[r0 + q[own], c0 + q[own]] = EXACT
    for comp in range(nc):
        rows = comp * n + q[dm]
        J[rows, :] = 0
        mag[rows, :] = 0
        tab[rows, :] = 0
        kind[rows, :] = ZERO
        ro = comp * n + q[dm & own]
        J[ro, ro] = 1
        kind[ro, ro] = EXACT
    c._ref = (J, mag, kind, tab)
    return c._ref


def line_index(c, lx):
    """Rows of J of the m unknowns (component, gy) of local line lx."""
    cg = np.arange(c.m)
    return (cg // c.NY) * c.n + lx * c.NY + cg % c.NY


def column_index(c, e):
    """Rows of J of the nI interior unknowns of local element column e, in column-interior order."""
    return np.concatenate([line_index(c, e * c.P + l) for l in range(1, c.P)]) if c.P > 1 else np.zeros(0, np.int64)


def pieces(c, M, layout="dense"):
    """The pieces of the nc n x nc n matrix M (any dtype) in the layout's logical shapes: the generalisation of
    tests/velocity_blocks.extract to ncomp 1 or 2, to strips, to a column range and to the condensed layout."""
    P, ne, m = c.P, c.ne, c.m
    sh = c.shapes(layout)
    out = {k: np.zeros(s, dtype=M.dtype) for k, s in sh.items()}
    for L in range(ne + 1):
        r = line_index(c, L * P)
        out["D"][L] = M[np.ix_(r, r)]
        if L < ne:
            r2 = line_index(c, (L + 1) * P)
            out["E"][L] = M[r, r2]
            out["F"][L] = M[r2, r]
    for e in range(ne):
        for li, l in enumerate(range(1, P)):
            ri = line_index(c, e * P + l)
            for s in range(2):
                rb = line_index(c, (e + s) * P)
                out["aIB"][e, li, s] = M[ri, rb]
                out["aBI"][e, s, li] = M[rb, ri]
    if P == 1:
        return out
    c0, c1 = c.cols[0] - c.eb, c.cols[1] - c.eb
    if layout == "dense":
        for e in range(c0, c1):
            rows = column_index(c, e)
            out["AII"][e - c0] = M[np.ix_(rows, rows)]
        return out
    pi, pe = nested_index(P, c.ney, c.nc)
    pe = pe.reshape(c.ney + 1, c.ne1)
    for e in range(c0, c1):
        rows = column_index(c, e)
        for n in range(c.ney):
            i, g = rows[pi[n]], rows[np.concatenate((pe[n], pe[n + 1]))]
            out["Aii"][e - c0, n] = M[np.ix_(i, i)]
            out["Aie"][e - c0, n] = M[np.ix_(i, g)]
            out["Aei"][e - c0, n] = M[np.ix_(g, i)]
            out["Aeu"][e - c0, n] = M[np.ix_(rows[pe[n]], rows[pe[n + 1]])]
            out["Ael"][e - c0, n] = M[np.ix_(rows[pe[n + 1]], rows[pe[n]])]
        for k in range(c.ney + 1):
            out["Aed"][e - c0, k] = M[np.ix_(rows[pe[k]], rows[pe[k]])]
    return out


def reference(c, layout="dense"):
    """{piece: (ref, mag, kind, tab)} of the case in the layout."""
    parts = [pieces(c, M, layout) for M in dense_jacobian(c)]
    return {name: tuple(p[name] for p in parts) for name in parts[0]}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def compare(got, ref, P, tables_differ=True):
    """(worst, failures): the largest |got - ref| / (2^-53 (L mag + T tab)) over the entries compared by the bound,
    and what failed -- a non-finite entry, an exact entry that differs, an entry further than SLACK bounds away.
    Every entry of every piece of `ref` is compared; a piece of size 0 may be absent from `got`.  tables_differ
    False: `got` was computed from the oracle's own tables, so T = 0."""
    worst, fails = 0.0, []
    T = table_roundings(P) if tables_differ else 0
    for name, (r, mag, kind, tab) in ref.items():
        if r.size == 0:
            continue
        g = np.asarray(got[name], dtype=np.float64).reshape(r.shape)
        if not np.all(np.isfinite(g)):
            fails.append(f"{name}: {int(np.sum(~np.isfinite(g)))} non-finite entries")
            continue
        z, x, b = kind == ZERO, kind == EXACT, kind == BOUND
        assert np.all(mag[b] > 0) and z.sum() + x.sum() + b.sum() == g.size
        if not np.all(g[z] == 0):
            fails.append(f"{name}: {int(np.sum(g[z] != 0))} entries without a term are not zero")
        if not np.array_equal(_bits(g[x]), _bits(r[x].astype(np.float64))):
            fails.append(f"{name}: an identity diagonal or a copied operand differs")
        if b.any():
            ratio = float((np.abs(g[b].astype(LD) - r[b]) / (LD(U53) * (L_ROUNDINGS * mag[b] + T * tab[b]))).max())
            worst = max(worst, ratio)
            if ratio > SLACK:
                fails.append(f"{name}: {ratio:.3g} of the first-order bound (L = {L_ROUNDINGS})")
    return worst, fails


def plain_ratio(got, ref):
    """The largest |got - ref| / (L 2^-53 mag) over the entries compared by the bound: what the comparison would
    be without the table allowance.  Reported, never asserted (module docstring: the tables' own error)."""
    worst = 0.0
    for name, (r, mag, kind, _) in ref.items():
        b = kind == BOUND
        if b.any():
            g = np.asarray(got[name], dtype=np.float64).reshape(r.shape)
            worst = max(worst, float((np.abs(g[b].astype(LD) - r[b]) / (LD(U53) * L_ROUNDINGS * mag[b])).max()))
    return worst


# ---- the kernel's formulas in float64, with mutants ----------------------------------------------------------------

def kernel_f64(c, layout="dense", mutant=None, tabs=None):
    """velocity_blocks_kernel and its launcher evaluated row by row in float64 on the oracle's tables (or the tables
    tabs = (w, K_s, G_s)): D, A_II and the condensed pieces start as zeros (the launcher's memsets), every other
    piece as NaN (callers hand in uninitialised storage).  mutant: one of MUTANTS, a plausible slip of the kernel."""
    assert mutant is None or mutant in MUTANTS
    P, ney, NY, nc, m, nex, eb, ee = c.P, c.ney, c.NY, c.nc, c.m, c.nex, c.eb, c.ee
    w, Ks, Gs = (np.asarray(t, dtype=np.float64) for t in (tables(P) if tabs is None else tabs))
    dx, dy, cf = c.dx, c.dy, c.coef
    fKx, fKy = cf["c_stiff"] * (dy / dx), cf["c_stiff"] * (dx / dy)
    if mutant == "swap_dydx":
        fKx, fKy = fKy, fKx
    fM = 0.0 if mutant == "drop_mass" else cf["c_mass"] * ((dx / 2.0) * (dy / 2.0))
    fX, fY = cf["c_gradx"] * (dy / 2.0), cf["c_grady"] * (dx / 2.0)
    f = dict(c.f)
    if mutant == "swap_juv_jvu":
        f["juv"], f["jvu"] = f["jvu"], f["juv"]
    c0, c1 = c.cols
    lb0, lb1, NX = eb * P, ee * P, nex * P + 1
    cond = layout == "condensed"
    ne1, ni = c.ne1, c.ni
    o = {k: (np.zeros(s) if k in ("AII", "D") + COND else np.full(s, np.nan)) for k, s in c.shapes(layout).items()}
    dmask = None if c.dir_mask is None else np.asarray(c.dir_mask).reshape(c.lines, NY)
    sides = c.dir_sides

    def is_dir(gx, gy):
        if dmask is not None:
            return dmask[gx - lb0, gy] != 0
        return bool((sides & 1 and gx == 0) or (sides & 2 and gx == NX - 1) or (sides & 4 and gy == 0)
                    or (sides & 8 and gy == NY - 1))

    at = lambda k, node, fill: fill if f[k] is None else f[k][node]   # noqa: E731

    for lx in range(c.lines):
        gx = lb0 + lx
        L, l = divmod(gx, P)
        Ll = L - eb
        own = not (gx == lb1 and ee < nex)
        own_j = own or mutant == "ignore_own"
        for r in range(m):
            comp, gy = divmod(r, NY)
            node = lx * NY + gy
            dirn = is_dir(gx, gy)
            ey, j = divmod(gy, P)
            my = w[j] if j != 0 else (w[P] if ey > 0 else 0.0) + (w[0] if ey < ney else 0.0)
            left = L > (0 if mutant == "first_line_weight" else eb)
            mx = w[l] if l != 0 else (w[P] if left else 0.0) + (w[0] if L < ee else 0.0)
            cu, cv = at("cu", node, 1.0), at("cv", node, 1.0)
            fx, gxc = fKx * my, fX * cu * my
            fy, gyc = fKy * mx, fY * (cu if mutant == "cu_for_y" else cv) * mx
            xk = lambda i, k: fx * Ks[i, k] + gxc * Gs[i, k]      # noqa: E731
            yk = lambda i, k: fy * Ks[i, k] + gyc * Gs[i, k]      # noqa: E731
            jd = at("juu" if comp == 0 else "jvv", node, 0.0)
            jc = f["juv" if comp == 0 else "jvu"] if nc == 2 else None
            if l != 0:
                ib = o["aIB"][Ll, l - 1]
                if dirn and mutant != "dir_keeps_aIB":
                    ib[0, r] = ib[1, r] = 0.0
                else:
                    ib[0, r], ib[1, r] = xk(l, 0), xk(l, P)
                if L < c0 or L >= c1:
                    continue
                col = L - c0
                if cond:
                    lc = (l - 1) * nc + comp
                    oc = (l - 1) * nc + 1 - comp
                    if j != 0:
                        ri = lc * (P - 1) + j - 1
                        Ar, Er = o["Aii"][col, ey, ri], o["Aie"][col, ey, ri]
                        if dirn:
                            Ar[ri] = 1.0
                            continue
                        dg = fM * mx * my + jd + xk(l, l)
                        for k in range(1, P):
                            if k != l:
                                Ar[((k - 1) * nc + comp) * (P - 1) + j - 1] = xk(l, k)
                        for q in range(P + 1):
                            v = yk(j, q)
                            if q == j:
                                dg += v
                            elif q == 0:
                                Er[lc] = v
                            elif q == P:
                                Er[ne1 + lc] = v
                            else:
                                Ar[lc * (P - 1) + q - 1] = v
                        if jc is not None:
                            Ar[oc * (P - 1) + j - 1] = jc[node]
                        Ar[ri] = dg
                        continue
                    k = ey
                    Dr = o["Aed"][col, k, lc]
                    if dirn:
                        Dr[lc] = 1.0
                        continue
                    dg = fM * mx * my + jd + xk(l, l)
                    for kk in range(1, P):
                        if kk != l:
                            Dr[(kk - 1) * nc + comp] = xk(l, kk)
                    if k > 0:
                        Fr = o["Aei"][col, k - 1, ne1 + lc]
                        for q in range(P + 1):
                            v = yk(P, q)
                            if q == P:
                                dg += v
                            elif q == 0:
                                o["Ael"][col, k - 1, lc, lc] = v
                            else:
                                Fr[lc * (P - 1) + q - 1] = v
                    if k < ney:
                        Fr = o["Aei"][col, k, lc]
                        for q in range(P + 1):
                            v = yk(0, q)
                            if q == 0:
                                dg += v
                            elif q == P:
                                o["Aeu"][col, k, lc, lc] = v
                            else:
                                Fr[lc * (P - 1) + q - 1] = v
                    if jc is not None:
                        Dr[oc] = jc[node]
                    Dr[lc] = dg
                    continue
                row, col0 = o["AII"][col, (l - 1) * m + r], (l - 1) * m
            else:
                row, col0 = o["D"][Ll, r], 0
            self_ = col0 + r
            if dirn:
                if own:
                    row[self_] = 1.0
                if l == 0:
                    if L < ee:
                        o["E"][Ll, r] = 0.0
                        o["aBI"][Ll, 0, :, r] = 0.0
                    if L > eb:
                        o["F"][Ll - 1, r] = 0.0
                        o["aBI"][Ll - 1, 1, :, r] = 0.0
                continue
            dg = fM * mx * my
            if own_j:
                dg += jd
            if l != 0:
                dg += xk(l, l)
            else:
                if L > eb:
                    dg += xk(P, P)
                if L < ee:
                    dg += xk(0, 0)
            yb = col0 + comp * NY
            for i, el in ((j, ey),) if j != 0 else ((P, ey - 1), (0, ey)):
                if el < 0 or el >= ney:
                    continue
                for k in range(P + 1):
                    v = yk(i, k)
                    if k == i:
                        dg += v
                    else:
                        row[yb + el * P + k] += v
            row[self_] += dg
            if jc is not None and own_j:
                row[col0 + (1 - comp) * NY + gy] = jc[node]
            if l != 0:
                for k in range(1, P):
                    if k != l:
                        row[(k - 1) * m + r] = xk(l, k)
            else:
                if L < ee:
                    for k in range(1, P):
                        o["aBI"][Ll, 0, k - 1, r] = xk(0, k)
                    o["E"][Ll, r] = xk(0, P)
                if L > eb:
                    for k in range(1, P):
                        o["aBI"][Ll - 1, 1, k - 1, r] = xk(P, k)
                    o["F"][Ll - 1, r] = xk(P, 0)
    if mutant == "swap_EF":
        o["E"], o["F"] = o["F"], o["E"]
    if mutant == "swap_aIB_sides":
        o["aIB"] = o["aIB"][:, :, ::-1].copy()
    if mutant == "swap_Aeu_Ael":
        o["Aeu"], o["Ael"] = o["Ael"], o["Aeu"]
    return o


# ---- the launches the GPU tests make ---------------------------------------------------------------------------------

def column_ranges(eb, ee):
    """{name: cols}: all, the first column, the last column and, on three columns or more, a middle range."""
    out = {"all": (eb, ee), "first": (eb, eb + 1), "last": (ee - 1, ee)}
    if ee - eb >= 3:
        out["middle"] = (eb + 1, ee - 1)
    return out


def launches(P, nex, ney, eb, ee):
    """The covering selection of one shape: (ncomp, layout, mask, desc, cols name).  From the base launch
    (2, dense, irregular, full, all) every factor alone takes each of its values; then 14 launches rotate all the
    factors together at different strides, so that every value also meets other partners."""
    layouts = ("dense", "condensed") if P > 1 else ("dense",)
    ranges = tuple(column_ranges(eb, ee))
    base = (2, "dense", "irregular", "full", "all")
    out = [base]
    out += [(nc,) + base[1:] for nc in (0, 1)]
    out += [base[:1] + (lay,) + base[2:4] + (cr,) for lay in layouts for cr in ranges]
    out += [base[:2] + (mk,) + base[3:] for mk in MASKS]
    out += [base[:3] + (ds,) + base[4:] for ds in DESCS]
    for t in range(14):
        out.append(((2, 1, 0)[t % 3], layouts[(t // 2) % len(layouts)], MASKS[t % 7], DESCS[(3 * t + t // 7) % 7],
                    ranges[(t + t // 4) % len(ranges)]))
    seen, uniq = set(), []
    for x in out:
        if x not in seen:
            seen.add(x)
            uniq.append(x)
    return uniq
