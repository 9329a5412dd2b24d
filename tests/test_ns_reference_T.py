"""Pins tests/ns_reference_T.py (the np.longdouble restatement of sem_ns_apply_transpose that the GPU launch tests
compare the kernel with) to tests/ns_reference.py, which tests/test_ns_reference.py pins to the oracle: on meshes of
at most ~150 nodes the matrix of ns_reference is built column by column from unit vectors -- 3N rows (ru, rv, rc), 4N
columns (u, v, p and the temperature T of the c_T M T term) -- and ns_reference_T(z) must be Matrix^T z.

Bound per row: 1e-17 (|A|^T |z|)_r with |A| the entrywise absolute matrix: both sides are long-double sums
(eps = 1.1e-19) of the same products in different orders, at most 2 (2 P + 1) + 4 terms of a few roundings each."""
import numpy as np
import pytest

from ns_reference import LD, ns_reference
from ns_reference_T import ns_reference_T

DX, DY = 0.37, 0.23
COEF = dict(c_mass=0.75, c_stiff=1.0, c_gradx=310.0, c_grady=-270.0)
NAMES = ("cu", "cv", "juu", "juv", "jvu", "jvv")
MESHES = {1: (4, 3), 2: (3, 2), 3: (3, 3), 5: (2, 2)}


def _matrix(geo, N, kw, c_T):
    """The 3N x 4N matrix of ns_reference: columns u, v, p, T."""
    A = np.zeros((3 * N, 4 * N), dtype=LD)
    for j in range(4 * N):
        e = np.zeros(N)
        e[j % N] = 1.0
        ops = [None, None, None]
        T = None
        if j < 3 * N:
            ops[j // N] = e
        else:
            T = e
        A[:, j] = np.concatenate(ns_reference(*geo, *ops, c_T=c_T, T=T, **kw))
    return A


def _variants(P, nex, ney):
    NY = ney * P + 1
    N = (nex * P + 1) * NY
    interior = NY + 1 if P > 1 or (nex > 1 and ney > 1) else -1
    boundary = 2 * NY                     # gy = 0: Dirichlet under sides 15 and 4
    rnd = (np.random.default_rng(P).random(N) < 0.3).astype(np.uint8)
    rnd[NY + 1] = 1                       # an interior node in the mask: a pin there is a pin on a Dirichlet node
    out = []
    for sides, mask in ((15, None), (5, None), (0, None), (10, rnd)):
        for pin in (-1, interior, boundary):
            for first in ((False, True) if pin >= 0 else (False,)):
                out.append(dict(dir_sides=sides, dir_mask=mask, pin=pin, pin_first=first))
    return out


@pytest.mark.parametrize("P", sorted(MESHES))
def test_transpose_is_the_matrix_transpose(P):
    nex, ney = MESHES[P]
    geo = (P, nex, ney, DX, DY, 0, nex)
    N = (nex * P + 1) * (ney * P + 1)
    assert N <= 150
    r = np.random.default_rng(100 + P)
    f = {k: r.uniform(-1, 1, N) for k in NAMES}
    z = r.uniform(-1, 1, 3 * N)
    worst = 0.0
    for i, var in enumerate(_variants(P, nex, ney)):
        c_T = -0.4 if i % 2 == 0 else 0.0
        kw = dict(COEF, c_div=-1.0 if i % 3 else 0.7, **f, **var)
        if i % 5 == 4:                    # absent coefficients: cu, cv ones, j** zeros
            kw.update(cu=None, juv=None)
        A = _matrix(geo, N, kw, c_T)
        want = A.T @ z.astype(LD)
        bound = np.abs(A).T @ np.abs(z).astype(LD)
        got = np.concatenate(ns_reference_T(*geo, z[:N], z[N:2 * N], z[2 * N:], c_T=c_T, **kw))
        err = np.abs(got - want)
        assert np.all(err[bound == 0] == 0), var
        nz = bound > 0
        ratio = float((err[nz] / (LD(1e-17) * bound[nz])).max())
        assert ratio <= 1.0, (var, ratio)
        worst = max(worst, ratio)
        # absent inputs are zeros
        only_c = np.concatenate(ns_reference_T(*geo, None, None, z[2 * N:], c_T=c_T, **kw))
        w2 = A[2 * N:].T @ z[2 * N:].astype(LD)
        b2 = np.abs(A[2 * N:]).T @ np.abs(z[2 * N:]).astype(LD)
        assert np.all(np.abs(only_c - w2) <= LD(1e-17) * b2)
    print("NSTREF", f"P={P}", f"{worst:.3f}")


@pytest.mark.parametrize("P", [2, 3])
def test_absval_bounds_the_terms(P):
    """absval sums the absolute terms of the kernel's form G^T = -G + b, in which the boundary-line term and a shared
    node's two element rows do not cancel: it is never below the entrywise |A|^T |z|, so a bound built on it holds for
    the exact transpose too."""
    nex, ney = MESHES[P]
    geo = (P, nex, ney, DX, DY, 0, nex)
    NY = ney * P + 1
    N = (nex * P + 1) * NY
    r = np.random.default_rng(7 + P)
    f = {k: r.uniform(-1, 1, N) for k in NAMES}
    z = r.uniform(-1, 1, 3 * N)
    kw = dict(COEF, c_div=-1.0, dir_sides=15, pin=NY + 1, pin_first=False, **f)
    A = _matrix(geo, N, kw, -0.4)
    low = np.abs(A).T @ np.abs(z).astype(LD)
    got = np.concatenate(ns_reference_T(*geo, z[:N], z[N:2 * N], z[2 * N:], c_T=-0.4, absval=True, **kw))
    # |G[r, q]| of the forward rows against |G[q, r]| of the transpose: the float64 tables differ in the last place
    assert np.all(got >= low * (1 - LD(1e-15)))


@pytest.mark.parametrize("P", [1, 2, 3])
def test_absval_is_exactly_the_kernels_terms(P):
    """Pins absval from above as well, on operators without cancellation between terms.  Mass and stiffness alone
    (positive diagonals, K symmetric): absval is the entrywise |A|^T |z|.  The transposed gradients alone: the form
    G^T = -G + b counts, on every line that ends an element, the two halves +-1/2 a of a shared node (exact entry 0)
    or 1/2 a and the boundary-line term a (exact entry -+1/2 a) separately -- one weighted |a| more than the entrywise
    sum there, and nothing more anywhere."""
    from ns_reference import ops_1d
    nex, ney = MESHES[P]
    geo = (P, nex, ney, DX, DY, 0, nex)
    lines, NY = nex * P + 1, ney * P + 1
    N = lines * NY
    r = np.random.default_rng(17 + P)
    z = r.uniform(-1, 1, 3 * N)
    zero = np.zeros(N)
    tol = LD(1e-15)             # |K[r, q]| against |K[q, r]|, |G[r, q]| against |G[q, r]| of the float64 tables

    kw = dict(c_mass=0.75, c_stiff=1.3, dir_sides=0, pin=-1)
    A = _matrix(geo, N, kw, 0.0)[:2 * N, :2 * N]
    low = np.abs(A).T @ np.abs(z[:2 * N]).astype(LD)
    got = np.concatenate(ns_reference_T(*geo, z[:N], z[N:2 * N], None, absval=True, **kw)[:2])
    assert np.all(np.abs(got - low) <= tol * low)

    kw = dict(dir_sides=0, pin=-1)
    A = _matrix(geo, N, kw, 0.0)
    mx = ops_1d(P, nex, DX)[0][:, None]
    my = ops_1d(P, ney, DY)[0][None, :]
    endx = (np.arange(lines) % P == 0).astype(LD)[:, None]
    endy = (np.arange(NY) % P == 0).astype(LD)[None, :]
    for k, (w, end) in enumerate(((my, endx), (mx, endy))):        # zu alone, then zv alone: yp = G^T z
        zz = [None, None, None]
        zz[k] = z[k * N:(k + 1) * N]
        low = np.abs(A[k * N:(k + 1) * N, 2 * N:3 * N]).T @ np.abs(zz[k]).astype(LD)
        extra = (end * w * np.abs(zz[k]).reshape(lines, NY).astype(LD)).reshape(-1)
        got = ns_reference_T(*geo, *zz, absval=True, **kw)[2]
        assert np.all(np.abs(got - (low + extra)) <= tol * (low + extra))
        assert np.all(zero == ns_reference_T(*geo, *zz, absval=True, **kw)[3])
