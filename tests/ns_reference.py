"""Test helper (not a test module): sem_ns_apply's documented semantics (include/sem_ops.h, the comment above
sem_ns_desc) restated in np.longdouble, on a whole mesh or an element-column strip [ex_begin, ex_end).

Tensor-product form.  The 1-D tables w, K_s, G_s are the oracle's (oracle.sem_oracle gll_nodes / gll_K / gll_G,
float64, widened), never the library's.  Assembled over the strip's own element columns in x and over all element
rows in y:  mx, my (diagonal mass, with the d/2 factor), Kx, Ky (with the 2/d factor), Gx, Gy.  For U of shape
(lines, NY):

    M U   = mx (x) my . U                 K U   = (Kx U) . my + mx . (U Ky^T)
    G_x U = (Gx U) . my                   G_y U = mx . (U Gy^T)

ns_reference(..., absval=True) returns, for every row, the sum of the absolute values of all the terms that enter
it -- (|A| |x|)_r with the element contributions of a shared node counted separately, as the kernels sum them --
which is what a first-order rounding bound of the row multiplies."""
import numpy as np

LD = np.longdouble

_TABLES = {}
_OPS = {}


def tables(P):
    """w, K_s, G_s of order P: the oracle's float64 tables, widened."""
    if P not in _TABLES:
        from oracle import sem_oracle as O
        _TABLES[P] = tuple(np.asarray(a, dtype=np.float64).astype(LD)
                           for a in (O.gll_nodes(P)[1], O.gll_K(P), O.gll_G(P)))
    return _TABLES[P]


def ops_1d(P, ne, d):
    """The assembled 1-D operators over ne elements of width d: (m, K, G, |K|, |G|); the absolute ones sum the
    absolute element entries (a shared node's two contributions do not cancel in them)."""
    key = (P, ne, float(d))
    if key not in _OPS:
        w, Ks, Gs = tables(P)
        L = ne * P + 1
        m = np.zeros(L, dtype=LD)
        K, G, aK, aG = (np.zeros((L, L), dtype=LD) for _ in range(4))
        for e in range(ne):
            s = slice(e * P, e * P + P + 1)
            m[s] += w
            K[s, s] += Ks
            G[s, s] += Gs
            aK[s, s] += np.abs(Ks)
            aG[s, s] += np.abs(Gs)
        half, inv = LD(d) / 2, 2 / LD(d)
        _OPS[key] = (m * half, K * inv, G, aK * inv, aG)
    return _OPS[key]


def strip_shape(P, nex, ney, ex_begin=0, ex_end=None):
    """(lines, NY, first global line) of the strip."""
    ex_end = nex if ex_end is None else ex_end
    return (ex_end - ex_begin) * P + 1, ney * P + 1, ex_begin * P


def dirichlet_rows(P, nex, ney, ex_begin, ex_end, dir_mask=None, dir_sides=0):
    """(dir, own) of shape (lines, NY): the Dirichlet set (dir_mask wins over dir_sides; bits W = 1, E = 2, S = 4,
    N = 8) and the rows this strip owns (all but the right interface line of a strip with ex_end < nex)."""
    lines, NY, l0 = strip_shape(P, nex, ney, ex_begin, ex_end)
    gx = (l0 + np.arange(lines))[:, None] + np.zeros((1, NY), dtype=np.int64)
    gy = np.arange(NY)[None, :] + np.zeros((lines, 1), dtype=np.int64)
    if dir_mask is not None:
        dm = np.asarray(dir_mask).reshape(lines, NY) != 0
    else:
        dm = (((dir_sides & 1) != 0) & (gx == 0)) | (((dir_sides & 2) != 0) & (gx == nex * P)) | \
             (((dir_sides & 4) != 0) & (gy == 0)) | (((dir_sides & 8) != 0) & (gy == NY - 1))
    own = ~((gx == ex_end * P) & (ex_end < nex))
    return dm, own


def pin_row(P, nex, ney, ex_begin, ex_end, pin, pin_first, dm):
    """Local (line, column) of the pinned row if this strip holds it and the pin is what rc keeps there (it
    goes before the Dirichlet rows when pin_first and after them otherwise), else None."""
    lines, NY, l0 = strip_shape(P, nex, ney, ex_begin, ex_end)
    if pin < 0:
        return None
    lx, gy = pin // NY - l0, pin % NY
    if not 0 <= lx < lines:
        return None
    if pin_first and dm[lx, gy]:
        return None
    return int(lx), int(gy)


def uv_index(lines, NY, pitch):
    """Flat position of node (lx, gy) of u, v, ru, rv in a buffer of line pitch `pitch` (0: NY)."""
    pitch = pitch or NY
    return (np.arange(lines)[:, None] * pitch + np.arange(NY)[None, :]).reshape(-1)


def ns_reference(P, nex, ney, dx, dy, ex_begin=0, ex_end=None, u=None, v=None, p=None, *, c_mass=0.0, c_stiff=0.0,
                 c_gradx=0.0, c_grady=0.0, cu=None, cv=None, juu=None, juv=None, jvu=None, jvv=None, c_T=0.0, T=None,
                 c_div=1.0, dval_u=None, dval_v=None, dir_mask=None, dir_sides=0, pin=-1, pin_val=0.0, pin_first=False,
                 absval=False):
    """(ru, rv, rc) of sem_ns_apply as np.longdouble vectors of the strip's n_local rows; every operand a plain
    float64 vector of n_local entries or None (zeros; cu, cv: ones).  absval: the per-row sums of absolute terms."""
    ex_end = nex if ex_end is None else ex_end
    lines, NY, _ = strip_shape(P, nex, ney, ex_begin, ex_end)
    mx, Kx, Gx, aKx, aGx = ops_1d(P, ex_end - ex_begin, dx)
    my, Ky, Gy, aKy, aGy = ops_1d(P, ney, dy)
    if absval:
        Kx, Gx, Ky, Gy = aKx, aGx, aKy, aGy
    A = np.abs if absval else (lambda a: a)
    minus = 1 if absval else -1

    def fld(a, fill=0.0):
        if a is None:
            return np.full((lines, NY), fill, dtype=LD)
        return A(np.asarray(a, dtype=np.float64).reshape(lines, NY).astype(LD))

    def co(c):
        return A(LD(c))

    U, V, Pp, Tt = fld(u), fld(v), fld(p), fld(T)
    CU, CV = fld(cu, 1.0), fld(cv, 1.0)
    mxc, myr = mx[:, None], my[None, :]
    mass = lambda X: mxc * myr * X                                   # noqa: E731
    stiff = lambda X: (Kx @ X) * myr + mxc * (X @ Ky.T)              # noqa: E731
    gradx = lambda X: (Gx @ X) * myr                                 # noqa: E731
    grady = lambda X: mxc * (X @ Gy.T)                               # noqa: E731
    sys = lambda X: (co(c_mass) * mass(X) + co(c_stiff) * stiff(X) + co(c_gradx) * CU * gradx(X)   # noqa: E731
                     + co(c_grady) * CV * grady(X))
    dm, own = dirichlet_rows(P, nex, ney, ex_begin, ex_end, dir_mask, dir_sides)
    ownf = own.astype(LD)
    zero = np.zeros((lines, NY), dtype=LD)

    ru = sys(U) + ownf * (fld(juu) * U + fld(juv) * V) + gradx(Pp)
    rv = sys(V) + ownf * (fld(jvu) * U + fld(jvv) * V) + grady(Pp) + co(c_T) * mass(Tt)
    ru = np.where(dm, np.where(own, U + minus * fld(dval_u), zero), ru)
    rv = np.where(dm, np.where(own, V + minus * fld(dval_v), zero), rv)

    rc = co(c_div) * (gradx(U) + grady(V))
    rc = np.where(dm, stiff(Pp), rc)
    at = pin_row(P, nex, ney, ex_begin, ex_end, int(pin), bool(pin_first), dm)
    if at is not None:
        rc[at] = (Pp[at] + minus * co(pin_val)) if own[at] else LD(0)
    return ru.reshape(-1), rv.reshape(-1), rc.reshape(-1)
