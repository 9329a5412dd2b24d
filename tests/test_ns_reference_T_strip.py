"""Pins tests/ns_reference_T_strip.py (the np.longdouble restatement of sem_ns_apply_transpose_part that the GPU strip
test compares the kernel with) to tests/ns_reference.py on strips: the matrix A_s of ns_reference on the strip is built
column by column from unit vectors -- 3 n_local rows (ru, rv, rc), 4 n_local columns (u, v, p and the temperature T of
the c_T M T term) -- and ns_reference_T_strip(z) must be A_s^T z.  That is independent of the identity G^T = -G + b.
On a whole mesh the helper must be ns_reference_T itself.

Bound per row: 1e-17 (|A_s|^T |z|)_r, as tests/test_ns_reference_T.py: both sides are long-double sums (eps = 1.1e-19)
of the same products in different orders, at most 2 (2 P + 1) + 4 terms of a few roundings each."""
import numpy as np
import pytest

from ns_reference import LD, ns_reference
from ns_reference_T import ns_reference_T
from ns_reference_T_strip import ns_reference_T_strip, strip_variants

DX, DY = 0.37, 0.23
COEF = dict(c_mass=0.75, c_stiff=1.0, c_gradx=310.0, c_grady=-270.0)
NAMES = ("cu", "cv", "juu", "juv", "jvu", "jvv")
NEX, NEY = 5, 2
STRIPS = [(0, 2), (2, 3), (3, 5)]


def _matrix(geo, n, kw, c_T):
    """The 3n x 4n matrix of ns_reference on the strip: columns u, v, p, T."""
    A = np.zeros((3 * n, 4 * n), dtype=LD)
    for j in range(4 * n):
        e = np.zeros(n)
        e[j % n] = 1.0
        ops = [None, None, None]
        T = None
        if j < 3 * n:
            ops[j // n] = e
        else:
            T = e
        A[:, j] = np.concatenate(ns_reference(*geo, *ops, c_T=c_T, T=T, **kw))
    return A


@pytest.mark.parametrize("strip", STRIPS)
@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_strip_transpose_is_the_matrix_transpose(P, strip):
    eb, ee = strip
    geo = (P, NEX, NEY, DX, DY, eb, ee)
    n = ((ee - eb) * P + 1) * (NEY * P + 1)
    r = np.random.default_rng(100 + 7 * P + eb)
    f = {k: r.uniform(-1, 1, n) for k in NAMES}
    z = r.uniform(-1, 1, 3 * n)
    worst = 0.0
    for i, var in enumerate(strip_variants(P, NEX, NEY, eb, ee)):
        c_T = -0.4 if i % 2 == 0 else 0.0
        kw = dict(COEF, c_div=-1.0 if i % 3 else 0.7, **f, **var)
        if i % 5 == 4:                    # absent coefficients: cu, cv ones, j** zeros
            kw.update(cu=None, juv=None)
        A = _matrix(geo, n, kw, c_T)
        want = A.T @ z.astype(LD)
        bound = np.abs(A).T @ np.abs(z).astype(LD)
        got = np.concatenate(ns_reference_T_strip(*geo, z[:n], z[n:2 * n], z[2 * n:], c_T=c_T, **kw))
        err = np.abs(got - want)
        assert np.all(err[bound == 0] == 0), var
        nz = bound > 0
        ratio = float((err[nz] / (LD(1e-17) * bound[nz])).max())
        assert ratio <= 1.0, (var, ratio)
        worst = max(worst, ratio)
        # absval is never below the entrywise |A_s|^T |z| (the tables' |G[r, q]| against |G[q, r]|: last place)
        av = np.concatenate(ns_reference_T_strip(*geo, z[:n], z[n:2 * n], z[2 * n:], c_T=c_T, absval=True, **kw))
        assert np.all(av >= bound * (1 - LD(1e-15))), var
    print("NSTSTRIPREF", f"P={P}", strip, f"{worst:.3f}")


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_whole_mesh_is_ns_reference_T(P):
    nex, ney = 3, 2
    geo = (P, nex, ney, DX, DY, 0, nex)
    n = (nex * P + 1) * (ney * P + 1)
    r = np.random.default_rng(5 + P)
    f = {k: r.uniform(-1, 1, n) for k in NAMES}
    z = [r.uniform(-1, 1, n) for _ in range(3)]
    for var in strip_variants(P, nex, ney, 0, nex):
        for absval in (False, True):
            kw = dict(COEF, c_div=0.7, c_T=-0.4, absval=absval, **f, **var)
            for a, b in zip(ns_reference_T_strip(*geo, *z, **kw), ns_reference_T(*geo, *z, **kw)):
                assert np.array_equal(a, b), (var, absval)
