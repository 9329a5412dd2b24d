"""Test helper (not a test module): sem_ns_apply_transpose's documented semantics (include/sem_ops.h) restated in
np.longdouble -- the transpose of the linear part of ns_reference.ns_reference (T, dval_u, dval_v absent, pin_val 0),
from the same assembled 1-D operators (ns_reference.ops_1d) and the same Dirichlet / pin rules
(ns_reference.dirichlet_rows, pin_row).  Whole meshes only, as the entry point.

With the notation of ns_reference (U of shape (lines, NY)) the transposes are

    M^T U = M U       K^T U = Kx^T (U . my) + (mx . U) Ky       G_x^T U = Gx^T (U . my)       G_y^T U = (mx . U) Gy

and, with m the Dirichlet set, at the pinned row that rc keeps, z' = (1 - m) z, w = c_div (1 - m - at) zc,
k = (m - at) zc:

    yu = Sys^T z'_u + juu z'_u + jvu z'_v + G_x^T w + m zu          Sys^T X = cM M X + cK K^T X + cX G_x^T (cu X)
    yv = Sys^T z'_v + jvv z'_v + juv z'_u + G_y^T w + m zv                    + cY G_y^T (cv X)
    yp = G_x^T z'_u + G_y^T z'_v + K^T k + at zc
    yT = c_T M z'_v

The values use the true transposes of the oracle's tables.  ns_reference_T(..., absval=True) returns, for every row,
the sum of the absolute values of the terms IN THE FORM THE KERNEL COMPUTES THEM (ns_apply_transpose.hip): the
transposed gradient as forward rows plus a boundary-line term, G^T a = -G a + b a, so a row sums |G| |a| over the
forward element rows (a shared node's two elements counted separately) and |b| |a| as a term of its own; K through its
forward rows."""
import numpy as np

from ns_reference import LD, dirichlet_rows, ops_1d, pin_row, strip_shape


def ns_reference_T(P, nex, ney, dx, dy, ex_begin=0, ex_end=None, zu=None, zv=None, zc=None, *, c_mass=0.0, c_stiff=0.0,
                   c_gradx=0.0, c_grady=0.0, cu=None, cv=None, juu=None, juv=None, jvu=None, jvv=None, c_T=0.0, T=None,
                   c_div=1.0, dval_u=None, dval_v=None, dir_mask=None, dir_sides=0, pin=-1, pin_val=0.0, pin_first=False,
                   absval=False):
    """(yu, yv, yp, yT) of sem_ns_apply_transpose as np.longdouble vectors of N rows; every operand a plain float64
    vector of N entries or None (zeros; cu, cv: ones).  absval: the per-row sums of absolute terms."""
    ex_end = nex if ex_end is None else ex_end
    if ex_begin != 0 or ex_end != nex:
        raise ValueError("the transposed apply is a whole-mesh operation")
    if T is not None or dval_u is not None or dval_v is not None or pin_val != 0.0:
        raise ValueError("the transpose of the linear part takes no T, dval_u, dval_v, pin_val")
    lines, NY, _ = strip_shape(P, nex, ney, 0, nex)
    mx, Kx, Gx, aKx, aGx = ops_1d(P, nex, dx)
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
        # the kernel's form: forward rows of |K|, |G| and the boundary-line term of G^T = -G + b
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
    dm, _ = dirichlet_rows(P, nex, ney, 0, nex, dir_mask, dir_sides)
    at = pin_row(P, nex, ney, 0, nex, int(pin), bool(pin_first), dm)
    pinned = np.zeros((lines, NY), dtype=bool)
    if at is not None:
        pinned[at] = True
    zero = np.zeros((lines, NY), dtype=LD)
    Zu, Zv, Zc = fld(zu), fld(zv), fld(zc)
    Zup, Zvp = np.where(dm, zero, Zu), np.where(dm, zero, Zv)
    W = co(c_div) * np.where(dm | pinned, zero, Zc)
    Kk = np.where(dm & ~pinned, Zc, zero)

    yu = sysT(Zup) + fld(juu) * Zup + fld(jvu) * Zvp + gradxT(W) + np.where(dm, Zu, zero)
    yv = sysT(Zvp) + fld(jvv) * Zvp + fld(juv) * Zup + gradyT(W) + np.where(dm, Zv, zero)
    yp = gradxT(Zup) + gradyT(Zvp) + stiffT(Kk) + np.where(pinned, Zc, zero)
    yT = co(c_T) * mass(Zvp)
    return yu.reshape(-1), yv.reshape(-1), yp.reshape(-1), yT.reshape(-1)
