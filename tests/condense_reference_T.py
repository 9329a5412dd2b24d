"""Test helper (not a test module): np.longdouble references, with derived first-order bounds, for the launches of the
transposed line condensation -- sem_nested_solve_t (sem_amd/csrc/ns_condense_transpose.hip) and sem_block_gemv_t
(sem_amd/csrc/block_gemv.hip).  The cases, the shape lists, SLACK, CAP, `within` and `worst` are those of
tests/condense_reference.py; so are the layouts, the bound's form (|err| <= n u sum |a_i b_i| for a sum of n products
in any order, u = 2^-53) and the way the tests use it (every launch's reference is fed the device's output of the
launch before it, so every GPU bound is a single-launch bound).

The transposed solve reads the forward factor.  A case here is a `Case` of the block-Thomas edge form whose `aIB`
field holds aBIt -- aBI permuted into aIB's layout, what sem_nested_solve_t takes -- so rhs() (r = R - aBIt xB) and the
reduced edge right-hand side are the forward module's references unchanged.

Term counts n, read off the kernels:
  rows_dot_l           a stored row of `len` elements, L = dot_lanes(len) lanes: each lane's elements in two
                       accumulators (1 addition), a butterfly of log2(L) additions: len + 1 + log2(L)
  K1t  C = Yie^T r_i   rows of ni; r_i carries rhs()'s error
  reduced edge rhs     as the forward sweep (EdgeRhs::value): rhs()'s terms and the one or two C terms
  K3t  s = r_i - Aei^T [y_e(n); y_e(n+1)]   rows of 2 ne1, one subtraction more;  y_i = Xi^T s: rows of ni
  block_gemv_t         S m products; a lane's eight sums meet in 3 additions, the 256 / LANES <= 16 row groups in at most
                       15, one more when accumulating: S m + 19
Where an input x of y = M^T x carries an error dx, |M|^T dx is added.

The transposed block-Thomas sweep is the forward sweep's machinery with the lane on an output column (half_dot over
half a column, the pair sums of the operand, the two accumulators, the two halves, the subtraction): w = B + 4 as there,
  dw_k = dr_k + w u |r_k| + |Eu_{k-1}|^T dw_{k-1} + w u |Eu_{k-1}|^T |w_{k-1}|
  dt_k = dw_k + w u |w_k| + |El_k|^T dy_{k+1} + w u |El_k|^T |y_{k+1}|          (no El term at the last edge)
  dy_k = |Ed_k|^T dt_k + w u |Ed_k|^T |t_k|.

Scaling.  Ed, El, Eu are uniform(-1, 1) / B (absolute column sums <= 1 as well as row sums), every other block is
uniform(-1, 1).  The forward scaling does not fit the last product: Xi^T s has ni terms with s = r_i - Aei^T y_e, so the
bound of y_i is about ni u sum |Xi| |s| ~ ni^2 u |s| / 2, and y_e (through C = Yie^T r_i, ni terms of size |r_i|) is of
order sqrt(ni) |r_i|.  On a copy of the case the entries of R at the element-interior offsets and aBIt are therefore
uniform(-1, 1) / ni^2.5, those of R at the edge offsets uniform(-1, 1) / ni^2 and xB is uniform(-1, 1): y_e is of order
ni^-2 and s of order sqrt(2 ne1) ni^-2.  The chained bound of y_i is led by the sweep's running bound carried through
|Xi|^T |Aei|^T (a factor ne1 ni / 2): 3e-14 at ni = 1024, where the single-launch bound the GPU tests use (the device's
y_e fed in) is 2e-17 for values of 2e-5.  With vectors sqrt(ni) larger the chained bound was 6.7e-13 at ni = 1024,
above CAP / SLACK.  Every bound is relative to sum |a_i b_i|, so the scaling takes nothing from a test's power.  tests/test_condense_transpose.py asserts
SLACK x bound <= CAP at every shape the GPU tests run."""
import numpy as np

import condense_reference as cr
from condense_reference import (CAP, CHAINS, LD, REGIMES, SLACK, U53, WIDTHS, Case, ref_re, ref_rhs, within,  # noqa: F401
                                width_nex_ney, worst)

MUTANTS_T = ("swap_EuEl", "Ed_not_transposed", "swap_C", "drop_coupling", "Xi_not_transposed")


def dot_lanes(n):
    """Lanes per stored row of rows_dot_l."""
    return 4 if n <= 16 else 8 if n <= 32 else 16 if n <= 64 else 32 if n <= 128 else 64


def rowdot_terms(n):
    """n of one rows_dot_l row sum."""
    return n + 1 + int(np.log2(dot_lanes(n)))


def _mvT(M, x):
    """M^T x over the leading (batch) axes."""
    return np.matmul(np.swapaxes(M, -1, -2), x[..., None])[..., 0]


def _zero(a):
    return np.zeros(a.shape, dtype=LD)


def synthetic_t(P, nex, ney, nc, coupled, seed=0):
    """A synthetic block-Thomas case rescaled for the transposed solve (module docstring: Scaling); c.aIB is aBIt."""
    c = Case.synthetic(P, nex, ney, nc, "thomas", coupled, seed)
    r = np.random.default_rng([seed, P, nex, ney, nc, 77, int(coupled)])
    u = lambda *s: r.uniform(-1, 1, s)  # noqa: E731
    ni = c.ni
    c.aIB = u(nex, P - 1, 2, c.m) / ni ** 2.5
    c.aBIt = c.aIB
    c.xB = u(nex + 1, c.m)
    c.R[:, :c.nI] = u(nex, c.nI)
    c.R[:, c.pi.reshape(-1)] /= ni ** 2.5
    c.R[:, c.pe] /= ni ** 2
    return c


def case_from_solver(vs, seed=0):
    """The blocks of a factored VelocityJacobianSolver (CPU, block-Thomas edge form) as a Case, with a seeded
    right-hand side; c.aIB is aBIt = aBI permuted into aIB's layout."""
    assert vs._edge_thomas
    c = Case(vs.P, vs.nex, vs.ney, vs.ncomp)
    c.edge, c.coupled = "thomas", True
    for k in ("Xi", "Aei", "Yie", "Ed", "El", "Eu"):
        setattr(c, k, np.ascontiguousarray(getattr(vs, "_" + k).numpy()))
    assert np.array_equal(c.pi, vs._pi.numpy()) and np.array_equal(c.pe, vs._pe.numpy())
    c.aIB = np.ascontiguousarray(vs.aBI.permute(0, 2, 1, 3).numpy())
    c.aBIt = c.aIB
    r = np.random.default_rng(seed)
    c.xB = r.uniform(-1, 1, (c.nex + 1, c.m))
    c.ld_r = c.P * c.m
    c.R = np.full((c.nex, c.ld_r), np.nan)
    c.R[:, :c.nI] = r.uniform(-1, 1, (c.nex, c.nI))
    c.ld_y = c.nI + 5
    return c


# ---- K1t -----------------------------------------------------------------------------------------------------------

def ref_Ct(c, coupled, dt=LD, mutant=None):
    """cond_fwd_t_kernel: C = Yie^T r_i (nex, ney, 2 ne1) and its bound."""
    r, dr, _ = ref_rhs(c, coupled, dt, mutant)
    x, dx = r[:, c.pi], dr[:, c.pi]
    Yie = c.Yie.astype(dt)
    C = _mvT(Yie, x)
    if dt is not LD:
        return C, None
    aY = np.abs(Yie)
    return C, rowdot_terms(c.ni) * U53 * _mvT(aY, np.abs(x)) + _mvT(aY, dx)


# ---- K2t: the reduced right-hand side is condense_reference.ref_re; the sweep -------------------------------------------

def ref_edge_t(c, re, dre=None, dt=LD, mutant=None):
    """cond_edge_thomas_t_kernel<B>: y_e = S_e^-T r_e (nex, ney+1, ne1) by the transposed recurrence, with the running
    componentwise bound of the module docstring; also returns the forward half w (what the kernel parks in Ye)."""
    bound = dt is LD
    re = re.astype(dt)
    if bound and dre is None:
        dre = _zero(re)
    Ed, El, Eu = c.Ed.astype(dt), c.El.astype(dt), c.Eu.astype(dt)
    if mutant == "swap_EuEl":
        El, Eu = Eu, El
    nb, wu = c.ney + 1, (c.ne1 + 4) * U53
    w, dw = [None] * nb, [None] * nb
    for k in range(nb):
        t = re[:, k]
        d = dre[:, k] + wu * np.abs(t) if bound else None
        if k > 0:
            t = t - _mvT(Eu[:, k - 1], w[k - 1])
            if bound:
                aU = np.abs(Eu[:, k - 1])
                d = d + _mvT(aU, dw[k - 1]) + wu * _mvT(aU, np.abs(w[k - 1]))
        w[k], dw[k] = t, d
    y, dy = [None] * nb, [None] * nb
    apply_Ed = (lambda M, v: cr._mv(M, v)) if mutant == "Ed_not_transposed" else _mvT
    for k in range(nb - 1, -1, -1):
        t = w[k]
        d = dw[k] + wu * np.abs(t) if bound else None
        if k < nb - 1:
            t = t - _mvT(El[:, k], y[k + 1])
            if bound:
                aL = np.abs(El[:, k])
                d = d + _mvT(aL, dy[k + 1]) + wu * _mvT(aL, np.abs(y[k + 1]))
        y[k] = apply_Ed(Ed[:, k], t)
        if bound:
            aD = np.abs(Ed[:, k])
            dy[k] = _mvT(aD, d) + wu * _mvT(aD, np.abs(t))
    return np.stack(y, axis=1), (np.stack(dy, axis=1) if bound else None)


# ---- K3t -----------------------------------------------------------------------------------------------------------

def ref_Yi_t(c, coupled, ye, dye=None, dt=LD, mutant=None):
    """cond_back_t_kernel: y_i = Xi^T (r_i - Aei^T [y_e(n); y_e(n+1)]) (nex, ney, ni) from the given edge values."""
    r, dr, _ = ref_rhs(c, coupled, dt, "drop_coupling" if mutant == "drop_coupling" else None)
    ri, dri = r[:, c.pi], dr[:, c.pi]
    Aei, Xi, x = c.Aei.astype(dt), c.Xi.astype(dt), cr._ye_pair(c, ye.astype(dt))
    v = _mvT(Aei, x)
    s = ri - v
    Yi = cr._mv(Xi, s) if mutant == "Xi_not_transposed" else _mvT(Xi, s)
    if dt is not LD:
        return Yi, None
    aA, aX = np.abs(Aei), np.abs(Xi)
    ds = dri + (rowdot_terms(c.G) + 1) * U53 * (np.abs(ri) + _mvT(aA, np.abs(x)))
    if dye is not None:
        ds = ds + _mvT(aA, cr._ye_pair(c, dye))
    return Yi, rowdot_terms(c.ni) * U53 * _mvT(aX, np.abs(s)) + _mvT(aX, ds)


def chain_solve_t(c, coupled, dt=LD, mutant=None):
    """sem_nested_solve_t, every launch fed the launch before it: C, re, ye, Yi, Y and (dt = LD) their chained
    bounds bC, bre, bye, bYi, bY."""
    C, bC = ref_Ct(c, coupled, dt, mutant)
    re, bre = ref_re(c, coupled, C, bC, dt, mutant)
    ye, bye = ref_edge_t(c, re, bre, dt, mutant)
    Yi, bYi = ref_Yi_t(c, coupled, ye, bye, dt, mutant)
    out = dict(C=C, re=re, ye=ye, Yi=Yi, Y=c.scatter(Yi, ye), bC=bC, bre=bre, bye=bye, bYi=bYi)
    if dt is LD:
        out["bY"] = c.scatter(bYi, bye)
    return out


def solve_cases_t():
    """Every (P, nex, ney, nc) sem_nested_solve_t is run at: the element-kernel regimes, all 32 block widths (ni = 1024
    among them), chains of 2..9 edges against the ring depth."""
    out = [(P, 2, 2, nc) for nc, P in REGIMES]
    out += [(P,) + width_nex_ney(nc, P) + (nc,) for nc, P in WIDTHS]
    out += [(P, 1 if P > 16 else 2, ney, nc) for nc, P, ney in CHAINS]
    return sorted(set(out))


# ---- sem_block_gemv_t ----------------------------------------------------------------------------------------------------

# (m, nb, S, W): the widths around the 64- and 16-column tiles, one block and three, every S and W
GEMV_T_CASES = [(m, nb, S, W) for m in (1, 63, 64, 65, 257, 513) for nb, S, W in ((1, 1, 1), (3, 2, 2), (3, 3, 3), (1, 2, 3))]
GEMV_T_GROUPS = 16          # the most row groups of either form


class GemvTCase:
    """One sem_block_gemv_t call: M (nblk, m, W m), S source arrays with their own leading dimensions, tables with
    absent terms (-1 in mblk or in xrow), an output array whose rows are ld_y > m apart."""

    def __init__(self, m, nb, S, W, seed=0, accumulate=1, nblk=None):
        r = np.random.default_rng([seed, m, nb, S, W, accumulate])
        self.m, self.nb, self.S, self.W, self.accumulate = m, nb, S, W, accumulate
        self.nblk = nblk or nb + 2
        self.M = r.uniform(-1, 1, (self.nblk, m, W * m))
        self.mcol = [int(v) for v in r.permutation(W)[:S]] if S <= W else [int(v) for v in r.integers(0, W, S)]
        self.nrow = nb + 3
        scale = 1.0 / (S * m) ** 1.5
        self.ld_src = [m + s for s in range(S)]
        self.src = [np.full((self.nrow, m + s), np.nan) for s in range(S)]
        for s in range(S):
            self.src[s][:, :m] = r.uniform(-1, 1, (self.nrow, m)) * scale
        self.mblk = r.integers(0, self.nblk, (S, nb)).astype(np.int64)
        self.xrow = r.integers(0, self.nrow, (S, nb)).astype(np.int64)
        if nb > 1:                      # absent terms, either way
            self.mblk[0, 1] = -1
            self.xrow[S - 1, nb - 1] = -1
        self.ld_y = m + 3
        self.ny = nb + 2
        self.yrow = r.permutation(self.ny)[:nb].astype(np.int64)
        self.y0 = r.uniform(-1, 1, (self.ny, self.ld_y)) * scale


def gemv_t_case(m, nb, S, W, seed=0, accumulate=1):
    return GemvTCase(m, nb, S, W, seed, accumulate)


def ref_block_gemv_t(g, dt=LD, mutant=None):
    """(y rows (nb, m), bound): y0[yrow[b]] (when accumulating) + sum_s M[mblk][:, slice]^T src_s[xrow]."""
    m = g.m
    out = np.zeros((g.nb, m), dtype=dt)
    mag = np.zeros((g.nb, m), dtype=LD)
    if g.accumulate:
        out += g.y0[g.yrow, :m].astype(dt)
        mag += np.abs(g.y0[g.yrow, :m])
    for s in range(g.S):
        for b in range(g.nb):
            blk, row = g.mblk[s, b], g.xrow[s, b]
            if blk < 0 or row < 0:
                continue
            A = g.M[blk][:, g.mcol[s] * m:(g.mcol[s] + 1) * m].astype(dt)
            x = g.src[s][row, :m].astype(dt)
            out[b] += (A @ x) if mutant == "not_transposed" else (A.T @ x)
            mag[b] += np.abs(A).T.astype(LD) @ np.abs(x).astype(LD)
    return out, (g.S * m + 3 + (GEMV_T_GROUPS - 1) + 1) * U53 * mag
