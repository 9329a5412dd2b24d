"""Test helper (not a test module): the oracle-backed solver doubles of tests/oracle_solvers.py with the
reverse-mode interface the coupled adjoint needs (_get_dresiduals_T, _get_update_T, _operator), from SciPy
transposes and sparse LU of the oracle's own matrices, and the coupled sparse Jacobian assembled from the same
blocks -- the reference of the coupler's transposed maps on the CPU and on the GPU.

Block solves are exact (splu) in both directions, so Krylov counts of the coupled solves are those of an exact
block-Jacobi preconditioner."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle_solvers import OracleCD, OracleNS


def _operator(o, M, x, c_mass, c_stiff, cu, cv, free, mask):
    x = np.asarray(x, dtype=np.float64)
    y = c_mass * (M @ x) + c_stiff * (o.K @ x)
    if cu is not None:
        y = y + np.asarray(cu) * (o.Gx @ x)
    if cv is not None:
        y = y + np.asarray(cv) * (o.Gy @ x)
    return np.where(mask, 0.0, y) if free else y


def _identity_rows(A, mask):
    """A with the rows of mask replaced by identity rows (CSR)."""
    keep = sp.diags((~mask).astype(np.float64))
    return (keep @ A + sp.diags(mask.astype(np.float64))).tocsr()


class AdjointCD(OracleCD):
    def _calc_jacobians(self, T):
        super()._calc_jacobians(T)
        self._lu = self._lu_T = None

    def matrix(self):
        """d rT / d (T, u_cd, v_cd) at the linearisation: A_D and the two free-row diagonals."""
        if not hasattr(self.o, "Sys") or not hasattr(self.o, "JTu"):
            raise RuntimeError("AdjointCD: residuals and linearize first")
        free = sp.diags((~self.o.mask).astype(np.float64))
        return _identity_rows(self.o.Sys, self.o.mask), (free @ self.o.JTu).tocsr(), (free @ self.o.JTv).tocsr()

    def _get_dresiduals_T(self, w):
        A, Ju, Jv = self.matrix()
        w = np.asarray(w, dtype=np.float64)
        return A.T @ w, Ju.T @ w, Jv.T @ w

    def _get_update(self, dres, dT0=None):
        if getattr(self, "_lu", None) is None:
            self._lu = spla.splu(_identity_rows(self.o.Sys, self.o.mask).tocsc())
        return self._lu.solve(np.asarray(dres, dtype=np.float64))

    def _get_residuals(self, T, u, v):
        self._lu = self._lu_T = None
        return super()._get_residuals(T, u, v)

    def _get_update_T(self, b, dres0=None):
        if getattr(self, "_lu_T", None) is None:
            self._lu_T = spla.splu(self.matrix()[0].T.tocsc())
        return self._lu_T.solve(np.asarray(b, dtype=np.float64))

    def _operator(self, x, c_mass=0.0, c_stiff=0.0, cu=None, cv=None, free=False):
        if c_mass:
            raise ValueError("the CD oracle holds no mass matrix")
        return _operator(self.o, sp.csr_matrix((self.N, self.N)), x, 0.0, c_stiff, cu, cv, free, self.o.mask)


class AdjointNS(OracleNS):
    def _calc_jacobians(self, u, v):
        super()._calc_jacobians(u, v)
        self._A = self._lu = self._lu_T = None

    def matrix(self):
        """(A, t): the 3N x 3N operator of dresiduals at dT = 0 (the block form of tests/test_gpu_ns_adjoint.py)
        and the N x N temperature column of the rv rows, -Gr/Re (1 - m) M."""
        if getattr(self, "_A", None) is None:
            o = self.o
            if not hasattr(o, "Juu"):
                raise RuntimeError("AdjointNS: residuals and linearize first")
            N, m = o.N, o.mask_bound
            e = o.mask_p
            m_c, m_b = m | e, m & ~e
            free = sp.diags((~m).astype(np.float64))
            J = _identity_rows(sp.bmat([[o.Juu, o.Juv], [o.Jvu, o.Jvv]], format="csr"), np.hstack((m, m)))
            B = sp.vstack([free @ o.Gx, free @ o.Gy])
            C = sp.diags((~m_c).astype(np.float64)) @ sp.hstack([o.Gx, o.Gy])
            E = sp.diags(m_b.astype(np.float64)) @ o.K + sp.diags(e.astype(np.float64))
            self._A = sp.bmat([[J, B], [C, E]], format="csr")
            self._t = (-o.GoR * (free @ o.M)).tocsr()
            assert self._A.shape == (3 * N, 3 * N)
        return self._A, self._t

    def _get_dresiduals_T(self, wu, wv, wc, want_T=False):
        A, t = self.matrix()
        N = self.N
        y = A.T @ np.hstack((wu, wv, wc))
        out = (y[:N], y[N:2 * N], y[2 * N:])
        return out + ((t.T @ np.asarray(wv, dtype=np.float64),) if want_T else ())

    def _get_update(self, ru, rv, rc, du0=None, dv0=None, dp0=None):
        if getattr(self, "_lu", None) is None:
            self._lu = spla.splu(self.matrix()[0].tocsc())
        return tuple(np.split(self._lu.solve(np.hstack((ru, rv, rc))), 3))

    def _get_update_T(self, bu, bv, bp, dres_c0=None):
        if getattr(self, "_lu_T", None) is None:
            self._lu_T = spla.splu(self.matrix()[0].T.tocsc())
        return tuple(np.split(self._lu_T.solve(np.hstack((bu, bv, bp))), 3))

    def _operator(self, x, c_mass=0.0, c_stiff=0.0, cu=None, cv=None, free=False):
        return _operator(self.o, self.o.M, x, c_mass, c_stiff, cu, cv, free, self.o.mask_bound)


def solvers(P, nex, ney, Re=1e3, Ra=1e3, Pr=0.71, mtol=1e-13):
    cd = AdjointCD(1.0, 1.0, Re * Pr, P, nex, ney, T_W=0.5, T_E=-0.5, mtol=mtol)
    ns = AdjointNS(1.0, 1.0, Re, Ra / Pr, P, nex, ney, mtol=mtol, mtol_newton=mtol)
    return cd, ns


def coupler(P, nex, ney, Re=1e3, Ra=1e3, Pr=0.71, cls=None, **kw):
    """A same-mesh coupler on the doubles (cls: BoussinesqCoupler by default)."""
    from sem_amd.solvers.boussinesq import BoussinesqCoupler
    cd, ns = solvers(P, nex, ney, Re, Ra, Pr)
    return (cls or BoussinesqCoupler)(1.0, 1.0, Re, Ra, Pr, P, nex, ney, P, nex, ney, cd=cd, ns=ns, **kw)


def coupled_jacobian(cd, ns):
    """The coupled sparse Jacobian of a same-mesh coupler from the doubles' blocks at their linearisation, rows
    [rT | ru | rv | rp], columns [T | u | v | p]; checked against the oracle's own dresiduals on a random vector
    to 1e-13 before it is returned."""
    Acd, Ju, Jv = cd.matrix()
    Ans, t = ns.matrix()
    N = ns.N
    assert cd.N == N
    Z = sp.csr_matrix((N, N))
    top = sp.hstack([Acd, Ju, Jv, Z])
    left = sp.vstack([Z, t, Z])
    J = sp.vstack([top, sp.hstack([left, Ans])]).tocsr()
    d = np.random.default_rng(99).uniform(-1, 1, 4 * N)
    dT, du, dv, dp = np.split(d, 4)
    want = np.hstack((cd.o.dresiduals(dT, du, dv),) + tuple(ns.o.dresiduals(du, dv, dp, dT)))
    assert np.abs(J @ d - want).max() <= 1e-13 * np.abs(want).max()
    return J


def cond(J):
    s = np.linalg.svd(J.toarray(), compute_uv=False)
    return s[0] / s[-1]
