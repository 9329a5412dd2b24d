"""Test helper (not a test module): sem_ns_apply_transpose_part's documented semantics (include/sem_ops.h) restated in
np.longdouble -- A_s^T z for the matrix A_s of ns_reference.ns_reference on ANY handle: a whole mesh or the
element-column strip [ex_begin, ex_end).  ns_reference_T generalised by the strip rules of the header:

  * x direction: the assembled 1-D operators are those of a mesh of the strip's own ncols = ex_end - ex_begin
    columns (ns_reference.ops_1d(P, ncols, dx)), so both interface lines carry partial sums and, in the kernel's
    form G_x^T = -G_x + b, the boundary term sits on the strip's first and last line; y is unchanged;
  * the Dirichlet set (ns_reference.dirichlet_rows): W / E bits only on the mesh boundary, an explicit mask and
    every operand indexed from the strip's first line;
  * the pin (ns_reference.pin_row): a global node, held by the strip or not a pin;
  * the right interface line (own == False): z', w, k are formed as everywhere (a kept pin gives w = k = 0), and
    m zu, m zv, the j** terms and the pinned entry are its right-hand owner's -- not added.

On a whole mesh every `own` is True and the expressions below are ns_reference_T's, term for term.
absval=True: the per-row sums of the absolute terms in the form the kernel computes them, as ns_reference_T has."""
import numpy as np

from ns_reference import LD, dirichlet_rows, ops_1d, pin_row, strip_shape


def ns_reference_T_strip(P, nex, ney, dx, dy, ex_begin=0, ex_end=None, zu=None, zv=None, zc=None, *, c_mass=0.0,
                         c_stiff=0.0, c_gradx=0.0, c_grady=0.0, cu=None, cv=None, juu=None, juv=None, jvu=None, jvv=None,
                         c_T=0.0, T=None, c_div=1.0, dval_u=None, dval_v=None, dir_mask=None, dir_sides=0, pin=-1,
                         pin_val=0.0, pin_first=False, absval=False):
    """(yu, yv, yp, yT) of sem_ns_apply_transpose_part as np.longdouble vectors of the strip's n_local rows; every
    operand a plain float64 vector of n_local entries or None (zeros; cu, cv: ones); pin a global node index."""
    ex_end = nex if ex_end is None else ex_end
    if T is not None or dval_u is not None or dval_v is not None or pin_val != 0.0:
        raise ValueError("the transpose of the linear part takes no T, dval_u, dval_v, pin_val")
    lines, NY, _ = strip_shape(P, nex, ney, ex_begin, ex_end)
    mx, Kx, Gx, aKx, aGx = ops_1d(P, ex_end - ex_begin, dx)
    my, Ky, Gy, aKy, aGy = ops_1d(P, ney, dy)
    A = np.abs if absval else (lambda a: a)

    def fld(a, fill=0.0):
        if a is None:
            return np.full((lines, NY), fill, dtype=LD)
        return A(np.asarray(a, dtype=np.float64).reshape(lines, NY).astype(LD))

    def co(c):
        return A(LD(c))

    mxc, myr = mx[:, None], my[None, :]
    mass = lambda X: mxc * myr * X                                    # noqa: E731
    if absval:
        # the kernel's form: forward rows of |K|, |G| and the boundary-line term of G^T = -G + b on the STRIP's ends
        bx = np.zeros((lines, 1), dtype=LD)
        by = np.zeros((1, NY), dtype=LD)
        bx[0, 0] = bx[-1, 0] = by[0, 0] = by[0, -1] = 1
        stiffT = lambda X: (aKx @ X) * myr + mxc * (X @ aKy.T)        # noqa: E731
        gradxT = lambda X: (aGx @ X) * myr + bx * myr * X             # noqa: E731
        gradyT = lambda X: mxc * (X @ aGy.T) + mxc * by * X           # noqa: E731
    else:
        stiffT = lambda X: Kx.T @ (X * myr) + (mxc * X) @ Ky          # noqa: E731
        gradxT = lambda X: Gx.T @ (X * myr)                           # noqa: E731
        gradyT = lambda X: (mxc * X) @ Gy                             # noqa: E731
    CU, CV = fld(cu, 1.0), fld(cv, 1.0)
    sysT = lambda X: (co(c_mass) * mass(X) + co(c_stiff) * stiffT(X) + co(c_gradx) * gradxT(CU * X)   # noqa: E731
                      + co(c_grady) * gradyT(CV * X))
    dm, own = dirichlet_rows(P, nex, ney, ex_begin, ex_end, dir_mask, dir_sides)
    at = pin_row(P, nex, ney, ex_begin, ex_end, int(pin), bool(pin_first), dm)
    pinned = np.zeros((lines, NY), dtype=bool)
    if at is not None:
        pinned[at] = True
    zero = np.zeros((lines, NY), dtype=LD)
    owned = lambda X: np.where(own, X, zero)                          # noqa: E731
    Zu, Zv, Zc = fld(zu), fld(zv), fld(zc)
    Zup, Zvp = np.where(dm, zero, Zu), np.where(dm, zero, Zv)
    W = co(c_div) * np.where(dm | pinned, zero, Zc)
    Kk = np.where(dm & ~pinned, Zc, zero)

    yu = sysT(Zup) + owned(fld(juu) * Zup) + owned(fld(jvu) * Zvp) + gradxT(W) + np.where(dm & own, Zu, zero)
    yv = sysT(Zvp) + owned(fld(jvv) * Zvp) + owned(fld(juv) * Zup) + gradyT(W) + np.where(dm & own, Zv, zero)
    yp = gradxT(Zup) + gradyT(Zvp) + stiffT(Kk) + np.where(pinned & own, Zc, zero)
    yT = co(c_T) * mass(Zvp)
    return yu.reshape(-1), yv.reshape(-1), yp.reshape(-1), yT.reshape(-1)


def strip_variants(P, nex, ney, ex_begin, ex_end, seed=0):
    """The Dirichlet x pin variants the strip tests run: dicts of dir_sides, dir_mask, pin (global), pin_first.

    Dirichlet: all four side bits; an explicit mask (random, with nodes forced in on the strip's first line, its
    last line and an inner line, and their neighbours forced out).  Pin: none; an owned inner node; a node on the
    strip's last line (its right interface line when ex_end < nex); a node on its first line; a Dirichlet node on
    the inner line and one on the last line, each with both values of pin_first; a node outside the strip."""
    lines, NY, l0 = strip_shape(P, nex, ney, ex_begin, ex_end)
    assert NY >= 3
    inner = 1 if lines > 2 else 0                 # P = 1 on one column: the first line is the only owned one
    last = lines - 1
    mask = (np.random.default_rng(seed + 31 * P + ex_begin).random((lines, NY)) < 0.25).astype(np.uint8)
    mask[[0, inner, last], 2] = 1
    mask[[0, inner, last], 1] = 0
    outside = 1 if ex_begin > 0 else (nex * P + 1) * NY - 2      # a node of the mesh's first / last line
    glob = lambda lx, gy: (l0 + lx) * NY + gy                    # noqa: E731
    out = []
    for sides, dmask, dcol in ((15, None, 0), (0, mask.reshape(-1), 2)):
        pins = [(-1, False), (glob(inner, 1), False), (glob(last, 1), False), (glob(0, 1), False), (outside, False)]
        pins += [(glob(lx, dcol), first) for lx in (inner, last) for first in (False, True)]
        out += [dict(dir_sides=sides, dir_mask=dmask, pin=int(pin), pin_first=first) for pin, first in pins]
    return out
