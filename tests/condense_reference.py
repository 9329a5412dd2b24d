"""Test helper (not a test module): synthetic cases and np.longdouble references for the line-condensation kernels of
sem_amd/csrc/ns_condense.hip, one reference per launch, with derived error bounds.

Layouts (ns_condense.hip lines 1-26, include/sem_ops.h sem_nested_desc).  m = nc N_y, N_y = ney P + 1, column-interior
offset o = (l-1) m + c N_y + gy.  Element-interior unknown ((l-1) nc + c)(P-1) + j-1 of element n sits at gy = n P + j
(pi), edge unknown (l-1) nc + c of edge k at gy = k P (pe).  Here every block is held as its logical [row, col] array;
`Device` stores Xi, Aei, Yie, XiB, AXB, ABY and Se column-major (the transpose) and Ed, El, Eu row-major.

Inputs.  Ed, El, Eu are uniform(-1, 1) / B, so every block has absolute row sums <= 1 and the sweep neither grows its
values nor its running bound; every other block is uniform(-1, 1).  The vectors are scaled so that the absolute
bounds stay far below 1e-12 at every shape.  A row of Xi or Aei has up to ni = 1024 terms: with r_i of order s, T is
of order s sqrt(ni), a row of |Aei| |T| of order s ni^1.5 and C's bound of order s ni^2.5 2^-53, so the entries of R
at the element-interior offsets, and aIB (which is added to them), are uniform(-1, 1) / ni^1.5: C's bound is then
about 0.13 ni 2^-53.  A row of the dense Se has n_e terms, so everything that enters the reduced edge
right-hand side is of order 1 / n_e: the entries of R at the edge offsets, xB (through AXB in the back solve) and
the back solve's starting C0 are uniform(-1, 1) / n_e; its starting T0 is uniform(-1, 1).  Every bound is relative to
sum |a_i b_i|, so the scaling changes no test's power: a lost term is as many bounds away as with vectors of order
one.

Bounds (derived, not measured).  u = 2^-53.  A sum of n products evaluated in any order, with or without fused
multiply-adds, satisfies |err| <= n u sum |a_i b_i| to first order: every term passes through at most one rounding of
its product and n - 1 of additions.  n is read off the kernel: the number of terms in the row plus the combining
additions --
  colmajor_gemv        cols terms, 3 additions of the four accumulators, splits - 1 of the column splits
                       (splits = 256 / RP for rows <= 128, RP = rows rounded up to 64; 1 above)
  T -= v, T - v        one more (K1 coupled, K3)
  rhs()                R, aIB0 xB0, aIB1 xB1: 3 terms
  reduced edge rhs     rhs()'s terms and the one or two C terms
  cond_edge_kernel     n_e terms, 3 + 3 additions (four accumulators, four splits)
  Pw, interior heights P-1 terms of aBI T, the ABY row as colmajor_gemv, one subtraction
  Pw, edge heights     P-1 terms
  g (iface_sum)        B, Pw[L][0], Pw[L-1][1]: 3 terms
  g (interface_rhs)    two sums of P-1 terms and two subtractions: P + 1 over all terms
Where an input x of y = M x carries an error dx (it was formed earlier in the same kernel, or the caller chains
launches), |M| dx is added.  The tests feed every launch's reference the values the device produced for the launch
before it, so each GPU bound is a single-launch bound.

The block-Thomas sweep overwrites its intermediate z, so its bound is carried through the recurrence componentwise, on
the reference's values, with w = B + 4 (a half-row of at most B/2 + 2 fused multiply-adds per accumulator, the pair sum
of the operand, the two accumulators, the two halves, the subtraction):
  dt_k = |El_{k-1}| dz_{k-1} + w u (|r_k| + |El_{k-1}| |z_{k-1}|) + dr_k
  dz_k = |Ed_k| dt_k + w u |Ed_k| |t_k|
  dy_k = dz_k + |Eu_k| dy_{k+1} + w u (|z_k| + |Eu_k| |y_{k+1}|),   dy_{nb-1} = dz_{nb-1}.
The runtime-width sweep (B fused multiply-adds in one chain and a subtraction) is inside the same w.

The tests allow SLACK = 2 over these first-order bounds (the project's factor for the second-order terms) and assert
that SLACK x bound <= CAP = 1e-12 at every shape they run, so that no bound is vacuous."""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
SLACK = 2.0
CAP = 1e-12
SENTINEL = -7.25e77             # what a launch must leave alone
GUARD = 32                      # doubles of guard band on either side of a device array (keeps 256-byte alignment)

MUTANTS = ("drop_El", "shift_Eu", "swap_C", "drop_coupling", "xB_order", "no_closing_edge", "shift_pi")


def nested_index(P, ney, nc):
    """pi (ney, ni) and pe (n_e) as VelocityJacobianSolver._nested_index builds them."""
    NY = ney * P + 1
    m = nc * NY
    l = np.arange(1, P)
    c = np.arange(nc)
    n = np.arange(ney)
    j = np.arange(1, P)
    k = np.arange(ney + 1)
    col = lambda ll, cc, gy: (ll - 1) * m + cc * NY + gy  # noqa: E731
    pi = col(l[None, :, None, None], c[None, None, :, None], n[:, None, None, None] * P + j[None, None, None, :])
    pe = col(l[None, :, None], c[None, None, :], k[:, None, None] * P)
    return pi.reshape(ney, -1).astype(np.int64), pe.reshape(-1).astype(np.int64)


def gemv_terms(rows, cols):
    """n of colmajor_gemv's row sum."""
    splits = 1 if rows > 128 else 256 // ((rows + 63) // 64 * 64)
    return cols + 3 + (splits - 1)


class Case:
    """Sizes and host arrays of one nested-condensation problem.  Blocks are logical [row, col] float64 arrays."""

    def __init__(self, P, nex, ney, nc):
        self.P, self.nex, self.ney, self.nc = P, nex, ney, nc
        self.NY = ney * P + 1
        self.m = nc * self.NY
        self.pm1 = P - 1
        self.nI = (P - 1) * self.m
        self.ne1 = nc * (P - 1)
        self.ni = self.ne1 * (P - 1)
        self.G = 2 * self.ne1
        self.n_e = (ney + 1) * self.ne1
        self.pi, self.pe = nested_index(P, ney, nc)
        self.Se = self.Ed = self.El = self.Eu = None
        self.XiB = self.AXB = self.ABY = None

    @property
    def thomas(self):
        return self.Se is None

    @classmethod
    def synthetic(cls, P, nex, ney, nc, edge, coupled, seed=0):
        """Random blocks that need not come from any factor (module docstring: Inputs)."""
        assert edge in ("dense", "thomas")
        c = cls(P, nex, ney, nc)
        c.edge, c.coupled = edge, coupled
        r = np.random.default_rng([seed, P, nex, ney, nc, int(edge == "thomas"), int(coupled)])
        u = lambda *s: r.uniform(-1, 1, s)  # noqa: E731
        ni, G, B, m = c.ni, c.G, c.ne1, c.m
        c.Xi, c.Aei, c.Yie = u(nex, ney, ni, ni), u(nex, ney, G, ni), u(nex, ney, ni, G)
        c.XiB, c.AXB, c.ABY = u(nex, ney, ni, G), u(nex, ney, G, G), u(nex, ney, G, G)
        if edge == "dense":
            c.Se = u(nex, c.n_e, c.n_e)
        else:
            c.Ed, c.El, c.Eu = u(nex, ney + 1, B, B) / B, u(nex, ney, B, B) / B, u(nex, ney, B, B) / B
        c.aIB, c.aBI, c.xB = u(nex, P - 1, 2, m) / ni ** 1.5, u(nex, 2, P - 1, m), u(nex + 1, m) / c.n_e
        # R: one interface line between the columns' interiors (production's ld_r = P m), NaN there
        c.ld_r = P * m
        c.R = np.full((nex, c.ld_r), np.nan)
        c.R[:, :c.nI] = u(nex, c.nI)
        c.R[:, c.pi.reshape(-1)] /= ni ** 1.5
        c.R[:, c.pe] /= c.n_e
        c.ld_y = c.nI + (5 if m != 5 else 6)
        assert c.ld_y != c.ld_r and c.ld_y > c.nI
        # interface lines of the line array B: rows L P of (nex P + 1) rows ld_b > m apart, NaN everywhere else
        c.ld_b = m + 3
        c.Bl = np.full((nex * P + 1, c.ld_b), np.nan)
        c.Bl[::P, :m] = u(nex + 1, m)
        # what sem_nested_back_solve starts from
        c.T0, c.C0 = u(nex, ney, ni), u(nex, ney, G) / c.n_e
        return c

    def scatter(self, Yi, ye, fill=np.nan):
        """The (nex, nI) column interiors holding element values Yi (nex, ney, ni) and edge values ye (nex, n_e)."""
        Y = np.full((self.nex, self.nI), fill, dtype=np.result_type(Yi, ye))
        Y[:, self.pi.reshape(-1)] = Yi.reshape(self.nex, -1)
        Y[:, self.pe] = ye.reshape(self.nex, -1)
        return Y


def _mv(M, x):
    return np.matmul(M, x[..., None])[..., 0]


def _zero(a):
    return np.zeros(a.shape, dtype=LD)


# ---- rhs(): r = R - aIB xB ---------------------------------------------------------------------------------------

def ref_rhs(c, coupled, dt=LD, mutant=None):
    """(r, dr, mag): the column interiors' right-hand side (nex, nI), its bound and sum of |terms|."""
    R = c.R[:, :c.nI].astype(dt)
    if not coupled or mutant == "drop_coupling":
        return R, _zero(R), np.abs(R)
    a, x = c.aIB.astype(dt), c.xB.astype(dt)
    t0, t1 = a[:, :, 0, :] * x[:-1, None, :], a[:, :, 1, :] * x[1:, None, :]
    r = R.reshape(c.nex, c.pm1, c.m) - (t0 + t1)
    mag = (np.abs(R.reshape(r.shape)) + np.abs(t0) + np.abs(t1)).reshape(c.nex, c.nI)
    return r.reshape(c.nex, c.nI), 3 * U53 * mag, mag


def _pi(c, mutant):
    return c.pi + 1 if mutant == "shift_pi" else c.pi


# ---- K1 ----------------------------------------------------------------------------------------------------------

def ref_T(c, coupled, dt=LD, mutant=None):
    """cond_fwd_kernel, first product: T = Xi r_i (nex, ney, ni) and its bound."""
    r, dr, _ = ref_rhs(c, coupled, dt, mutant)
    x, dx = r[:, _pi(c, mutant)], dr[:, _pi(c, mutant)]
    Xi = c.Xi.astype(dt)
    T = _mv(Xi, x)
    if dt is not LD:
        return T, None
    aX = np.abs(Xi)
    return T, gemv_terms(c.ni, c.ni) * U53 * _mv(aX, np.abs(x)) + _mv(aX, dx)


def ref_C(c, T, dT=None, dt=LD):
    """cond_fwd_kernel, second product: C = Aei T (nex, ney, 2 ne1) from the given T."""
    A, T = c.Aei.astype(dt), T.astype(dt)
    C = _mv(A, T)
    if dt is not LD:
        return C, None
    b = gemv_terms(c.G, c.ni) * U53 * _mv(np.abs(A), np.abs(T))
    return C, b if dT is None else b + _mv(np.abs(A), dT)


def xB_elem(c, dt=LD, mutant=None):
    """x_B|n (nex, ney, 2 ne1) in the order (side, component, height)."""
    x = c.xB.astype(dt).reshape(c.nex + 1, c.nc, c.NY)
    gy = (np.arange(c.ney)[:, None] * c.P + np.arange(1, c.P)[None, :])            # (ney, P-1)
    xs = np.stack((x[:-1], x[1:]), axis=1)[..., gy]                                 # (nex, s, c, ney, j)
    order = (0, 3, 2, 1, 4) if mutant == "xB_order" else (0, 3, 1, 2, 4)
    return xs.transpose(order).reshape(c.nex, c.ney, c.G)


def ref_coupled(c, T0, C0, dT0=None, dC0=None, dt=LD, mutant=None):
    """cond_fwd_coupled_kernel: T = T0 - XiB x_B|n, C = C0 - AXB x_B|n, and their bounds."""
    x = xB_elem(c, dt, mutant)
    XiB, AXB, T0, C0 = c.XiB.astype(dt), c.AXB.astype(dt), T0.astype(dt), C0.astype(dt)
    T, C = T0 - _mv(XiB, x), C0 - _mv(AXB, x)
    if dt is not LD:
        return T, C, None, None
    bT = (gemv_terms(c.ni, c.G) + 1) * U53 * (np.abs(T0) + _mv(np.abs(XiB), np.abs(x)))
    bC = (gemv_terms(c.G, c.G) + 1) * U53 * (np.abs(C0) + _mv(np.abs(AXB), np.abs(x)))
    return T, C, bT if dT0 is None else bT + dT0, bC if dC0 is None else bC + dC0


# ---- K2 ----------------------------------------------------------------------------------------------------------

def ref_re(c, coupled, C, dC=None, dt=LD, mutant=None):
    """The reduced edge right-hand side r_e[k] - C[n=k][:ne1] - C[n=k-1][ne1:], (nex, ney+1, ne1), and its bound."""
    r, dr, mag = ref_rhs(c, coupled, dt, mutant)
    B = c.ne1
    re = r[:, c.pe].reshape(c.nex, c.ney + 1, B).copy()
    C = C.astype(dt)
    lo, hi = (C[:, :, B:], C[:, :, :B]) if mutant == "swap_C" else (C[:, :, :B], C[:, :, B:])
    re[:, :-1] -= lo
    re[:, 1:] -= hi
    if dt is not LD:
        return re, None
    mg = mag[:, c.pe].reshape(re.shape).copy()
    mg[:, :-1] += np.abs(lo)
    mg[:, 1:] += np.abs(hi)
    d = ((5 if coupled else 3) * U53) * mg
    if dC is not None:
        d[:, :-1] += dC[:, :, :B]
        d[:, 1:] += dC[:, :, B:]
    return re, d


def ref_edge(c, re, dre=None, dt=LD, mutant=None):
    """y_e (nex, ney+1, ne1) from the reduced right-hand side: Se r_e (cond_edge_kernel) or the block-Thomas
    recurrence (cond_edge_thomas_kernel<B>, cond_edge_thomas_rt_kernel), with the bound of the module docstring."""
    bound = dt is LD
    re = re.astype(dt)
    if bound and dre is None:
        dre = _zero(re)
    if not c.thomas:
        Se = c.Se.astype(dt)
        x = re.reshape(c.nex, c.n_e)
        y = _mv(Se, x).reshape(re.shape)
        if not bound:
            return y, None
        aS = np.abs(Se)
        b = (c.n_e + 6) * U53 * _mv(aS, np.abs(x)) + _mv(aS, dre.reshape(x.shape))
        return y, b.reshape(re.shape)
    Ed, El, Eu = c.Ed.astype(dt), c.El.astype(dt), c.Eu.astype(dt)
    nb, w = c.ney + 1, (c.ne1 + 4) * U53
    z, dz = [None] * nb, [None] * nb
    for k in range(nb):
        t, d = re[:, k], dre[:, k] if bound else None
        if bound:
            d = d + w * np.abs(t)
        if k > 0:
            if mutant != "drop_El":
                t = t - _mv(El[:, k - 1], z[k - 1])
            if bound:
                aL = np.abs(El[:, k - 1])
                d = d + _mv(aL, dz[k - 1]) + w * _mv(aL, np.abs(z[k - 1]))
        z[k] = _mv(Ed[:, k], t)
        if bound:
            aD = np.abs(Ed[:, k])
            dz[k] = _mv(aD, d) + w * _mv(aD, np.abs(t))
    y, dy = list(z), list(dz)
    for k in range(nb - 2, -1, -1):
        E = Eu[:, max(k - 1, 0)] if mutant == "shift_Eu" else Eu[:, k]
        y[k] = z[k] - _mv(E, y[k + 1])
        if bound:
            aU = np.abs(E)
            dy[k] = dz[k] + _mv(aU, dy[k + 1]) + w * (np.abs(z[k]) + _mv(aU, np.abs(y[k + 1])))
    return np.stack(y, axis=1), np.stack(dy, axis=1) if bound else None


def _ye_pair(c, ye):
    """[y_e(n); y_e(n+1)] per element, (nex, ney, 2 ne1)."""
    ye = ye.reshape(c.nex, c.ney + 1, c.ne1)
    return np.concatenate((ye[:, :-1], ye[:, 1:]), axis=2)


# ---- K3 ----------------------------------------------------------------------------------------------------------

def ref_Yi(c, T, ye, dT=None, dye=None, dt=LD):
    """cond_back_kernel: y_i = T - Yie [y_e(n); y_e(n+1)] (nex, ney, ni); scatter with Case.scatter."""
    Yie, T, x = c.Yie.astype(dt), T.astype(dt), _ye_pair(c, ye.astype(dt))
    Yi = T - _mv(Yie, x)
    if dt is not LD:
        return Yi, None
    aY = np.abs(Yie)
    b = (gemv_terms(c.ni, c.G) + 1) * U53 * (np.abs(T) + _mv(aY, np.abs(x)))
    if dT is not None:
        b = b + dT
    if dye is not None:
        b = b + _mv(aY, _ye_pair(c, dye))
    return Yi, b


def scatter_Y(c, Yi, ye, mutant=None, fill=np.nan):
    """Case.scatter, through the mutant's pi."""
    Y = np.full((c.nex, c.nI + 1), fill, dtype=np.result_type(Yi, ye))
    Y[:, _pi(c, mutant).reshape(-1)] = Yi.reshape(c.nex, -1)
    Y[:, c.pe] = ye.reshape(c.nex, -1)
    return Y[:, :c.nI]


# ---- interface partial sums ------------------------------------------------------------------------------------------

def ref_Pw(c, T, ye, dT=None, dye=None, dt=LD, mutant=None):
    """cond_iface_part_kernel: Pw (nex, 2, m).  At element n's interior heights sum_l aBI T - ABY [y_e(n); y_e(n+1)],
    at the edge heights k = n, and k = ney on the last element, sum_l aBI y_e(k).  Entries nothing writes are NaN."""
    nex, ney, nc, pm1, P, NY = c.nex, c.ney, c.nc, c.pm1, c.P, c.NY
    bound = dt is LD
    a5 = c.aBI.astype(dt).reshape(nex, 2, pm1, nc, NY)
    T5 = T.astype(dt).reshape(nex, ney, pm1, nc, pm1)
    ye = ye.astype(dt).reshape(nex, ney + 1, c.ne1)
    gy = np.arange(ney)[:, None] * P + np.arange(1, P)[None, :]
    ai = a5[..., gy]                                                        # (nex, s, l, c, ney, j)
    acc = np.einsum("eslcnj,enlcj->enscj", ai, T5)
    ABY, x = c.ABY.astype(dt), _ye_pair(c, ye)
    v = _mv(ABY, x).reshape(nex, ney, 2, nc, pm1)
    Pw = np.full((nex, 2, nc, NY), np.nan, dtype=dt)
    bP = np.full((nex, 2, nc, NY), np.nan, dtype=LD) if bound else None
    val = acc - v
    if bound:
        nt = gemv_terms(c.G, c.G) + pm1 + 1
        aA = np.abs(ABY)
        b = nt * U53 * (np.einsum("eslcnj,enlcj->enscj", np.abs(ai), np.abs(T5))
                        + _mv(aA, np.abs(x)).reshape(v.shape))
        if dT is not None:
            b = b + np.einsum("eslcnj,enlcj->enscj", np.abs(ai), dT.reshape(T5.shape))
        if dye is not None:
            b = b + _mv(aA, _ye_pair(c, dye)).reshape(v.shape)
    for n in range(ney):
        Pw[..., n * P + 1:(n + 1) * P] = val[:, n]
        if bound:
            bP[..., n * P + 1:(n + 1) * P] = b[:, n]
    ae = a5[..., ::P]                                                       # (nex, s, l, c, ney+1)
    y4 = ye.reshape(nex, ney + 1, pm1, nc)
    ve = np.einsum("eslck,eklc->esck", ae, y4)
    last = ney if mutant == "no_closing_edge" else ney + 1
    Pw[..., 0:last * P:P] = ve[..., :last]
    if bound:
        be = pm1 * U53 * np.einsum("eslck,eklc->esck", np.abs(ae), np.abs(y4))
        if dye is not None:
            be = be + np.einsum("eslck,eklc->esck", np.abs(ae), dye.reshape(y4.shape))
        bP[..., ::P] = be
    return Pw.reshape(nex, 2, c.m), bP.reshape(nex, 2, c.m) if bound else None


def ref_g_sum(c, Pw, dPw=None, dt=LD):
    """cond_iface_sum_kernel: g[L] = B[L P] - Pw[L][0] - Pw[L-1][1], (nex+1, m)."""
    g = c.Bl[::c.P, :c.m].astype(dt)
    Pw = Pw.astype(dt)
    mag = np.abs(g)
    g[:-1] -= Pw[:, 0]
    g[1:] -= Pw[:, 1]
    if dt is not LD:
        return g, None
    mag[:-1] += np.abs(Pw[:, 0])
    mag[1:] += np.abs(Pw[:, 1])
    b = 3 * U53 * mag
    if dPw is not None:
        b[:-1] += dPw[:, 0]
        b[1:] += dPw[:, 1]
    return g, b


def ref_interface_rhs(P, nex, m, Bi, aBI, yI, dyI=None, dt=LD):
    """sem_interface_rhs: g[L] = Bi[L] - sum_l aBI[L][0][l] yI[L][l] - sum_l aBI[L-1][1][l] yI[L-1][l] for the
    interface lines Bi (nex+1, m), aBI (nex, 2, P-1, m) and the column interiors yI (nex, (P-1) m)."""
    a, y = aBI.astype(dt), yI.astype(dt).reshape(nex, 1, P - 1, m)
    s = (a * y).sum(2)                                                      # (nex, 2, m)
    g = Bi.astype(dt).copy()
    mag = np.abs(g)
    g[:-1] -= s[:, 0]
    g[1:] -= s[:, 1]
    if dt is not LD:
        return g, None
    sa = (np.abs(a) * np.abs(y)).sum(2)
    mag[:-1] += sa[:, 0]
    mag[1:] += sa[:, 1]
    b = (P + 1) * U53 * mag
    if dyI is not None:
        sd = (np.abs(a) * dyI.reshape(y.shape)).sum(2)
        b[:-1] += sd[:, 0]
        b[1:] += sd[:, 1]
    return g, b


# ---- whole entry points, launch after launch (chained bounds) ------------------------------------------------------

def chain_solve(c, coupled, dt=LD, mutant=None):
    """sem_nested_solve, every launch fed the launch before it: dict of T, C, re, ye, Yi, Y and (dt = LD) their chained
    bounds bT, bC, bre, bye, bYi, bY."""
    T, bT = ref_T(c, coupled, dt, mutant)
    C, bC = ref_C(c, T, bT, dt)
    return _chain_tail(c, coupled, T, C, bT, bC, dt, mutant)


def chain_back_solve(c, T0, C0, dT0=None, dC0=None, dt=LD, mutant=None):
    """sem_nested_back_solve from the work arrays T0, C0."""
    T, C, bT, bC = ref_coupled(c, T0, C0, dT0, dC0, dt, mutant)
    return _chain_tail(c, True, T, C, bT, bC, dt, mutant)


def _chain_tail(c, coupled, T, C, bT, bC, dt, mutant):
    re, bre = ref_re(c, coupled, C, bC, dt, mutant)
    ye, bye = ref_edge(c, re, bre, dt, mutant)
    Yi, bYi = ref_Yi(c, T, ye, bT, bye, dt)
    out = dict(T=T, C=C, re=re, ye=ye, Yi=Yi, Y=scatter_Y(c, Yi, ye, mutant), bT=bT, bC=bC, bre=bre, bye=bye, bYi=bYi)
    if dt is LD:
        out["bY"] = c.scatter(bYi, bye)
    return out


def chain_iface_rhs(c, dt=LD, mutant=None):
    """sem_nested_iface_rhs: T, C, ye, Pw, g and their chained bounds."""
    T, bT = ref_T(c, False, dt, mutant)
    C, bC = ref_C(c, T, bT, dt)
    re, bre = ref_re(c, False, C, bC, dt, mutant)
    ye, bye = ref_edge(c, re, bre, dt, mutant)
    Pw, bPw = ref_Pw(c, T, ye, bT, bye, dt, mutant)
    g, bg = ref_g_sum(c, Pw, bPw, dt)
    return dict(T=T, C=C, ye=ye, Pw=Pw, g=g, bT=bT, bC=bC, bye=bye, bPw=bPw, bg=bg)


def within(got, ref, bound):
    """got is finite and within SLACK x bound of ref, entry by entry."""
    got = np.asarray(got)
    if not np.all(np.isfinite(got)):
        return False
    return bool(np.all(np.abs(got.astype(LD) - ref) <= SLACK * bound))


def worst(got, ref, bound):
    """max |got - ref| / bound, for messages."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.abs(np.asarray(got).astype(LD) - ref) / np.maximum(bound, LD(1e-300))))


# ---- device side ---------------------------------------------------------------------------------------------------

class Arrays:
    """Device arrays, each inside a larger allocation with guard bands of GUARD entries before and after it, so that
    a used out-of-range read poisons the output and an out-of-range write shows.  A guard band is a multiple of
    256 bytes, so every array keeps its allocation's alignment."""

    def __init__(self):
        import torch
        self.torch = torch
        self.bufs, self.host = {}, {}

    def put(self, name, a, guard=np.nan):
        a = np.ascontiguousarray(a)
        full = np.full(a.size + 2 * GUARD, guard, dtype=a.dtype)
        full[GUARD:GUARD + a.size] = a.reshape(-1)
        self.host[name] = (full, a.shape)
        self.bufs[name] = self.torch.as_tensor(full, device="cuda")

    def set(self, name, a):
        """Overwrite the array (not its guard bands), on the host copy and on the device."""
        full, _ = self.host[name]
        full[GUARD:full.size - GUARD] = np.ascontiguousarray(a).reshape(-1)
        self.reset(name)

    def reset(self, *names):
        for k in names:
            self.bufs[k].copy_(self.torch.as_tensor(self.host[k][0]))

    def ptr(self, name):
        b = self.bufs[name]
        return b.data_ptr() + GUARD * b.element_size()

    def get(self, name):
        """The array as the device holds it (without the guard bands)."""
        full, shape = self.host[name]
        return self.bufs[name].cpu().numpy()[GUARD:full.size - GUARD].reshape(shape)

    def raw(self, name):
        """The whole allocation as the device holds it, guard bands included."""
        return self.bufs[name].cpu().numpy()

    def initial(self, name):
        """The whole allocation as it was put (or last set)."""
        return self.host[name][0]


class Device(Arrays):
    """The case's arrays on the GPU and the sem_nested_desc over them.  Guard bands: NaN; the sentinel around Y and
    g; the offset nI -- a NaN gap of R, a sentinel gap of Y -- around pi and pe.  The work arrays T, C, Ye, Pw start
    as NaN.  Ed, El and Eu keep the 16-byte alignment the templated sweep's vector loads rely on."""

    def __init__(self, c, L):
        super().__init__()
        self.c = c
        T = lambda a: np.swapaxes(a, -1, -2)  # noqa: E731  column-major storage
        put = self.put
        for k in ("Xi", "Aei", "Yie", "XiB", "AXB", "ABY"):
            put(k, T(getattr(c, k)))
        if c.thomas:
            for k in ("Ed", "El", "Eu"):
                put(k, getattr(c, k))
                assert self.ptr(k) % 16 == 0
        else:
            put("Se", T(c.Se))
        put("pi", c.pi, guard=c.nI), put("pe", c.pe, guard=c.nI)
        put("aIB", c.aIB), put("aBI", c.aBI), put("xB", c.xB), put("R", c.R), put("Bl", c.Bl)
        put("Y", np.full((c.nex, c.ld_y), SENTINEL), guard=SENTINEL)
        put("g", np.full((c.nex + 1, c.m), SENTINEL), guard=SENTINEL)
        put("T", np.full((c.nex, c.ney, c.ni), np.nan)), put("C", np.full((c.nex, c.ney, c.G), np.nan))
        put("Ye", np.full((c.nex, c.ney + 1, c.ne1), np.nan)), put("Pw", np.full((c.nex, 2, c.m), np.nan))
        q = lambda k: self.ptr(k) if k in self.bufs else None  # noqa: E731
        self.d = L.SemNestedDesc(c.P, c.nex, c.ney, c.nc, c.NY, q("Xi"), q("Aei"), q("Yie"), q("Se"), q("pi"),
                                 q("pe"), q("T"), q("C"), q("Ye"), q("Ed"), q("El"), q("Eu"), q("XiB"), q("AXB"),
                                 q("ABY"), q("Pw"))


# ---- a real factor's coupling blocks -------------------------------------------------------------------------------

def coupling_blocks(c):
    """XiB = Xi A_iB, AXB = A_ei Xi A_iB and ABY = A_Bi Xi A_ie = A_Bi Yie of the case's Xi, Aei, Yie, aIB and aBI (what
    VelocityJacobianSolver._condense_chunk keeps for the GPU), formed in long double and rounded once.  A_iB couples
    element n's interior unknown (l, c, j) to the interface unknown (s, c, j) of the same component and height with
    aIB[e, l-1, s, c N_y + n P + j]; A_Bi the other way with aBI[e, s, l-1, .]."""
    nex, ney, nc, pm1, NY = c.nex, c.ney, c.nc, c.pm1, c.NY
    gy = np.arange(ney)[:, None] * c.P + np.arange(1, c.P)[None, :]
    a = c.aIB.astype(LD).reshape(nex, pm1, 2, nc, NY)[..., gy]             # (e, l, s, c, n, j)
    b = c.aBI.astype(LD).reshape(nex, 2, pm1, nc, NY)[..., gy]             # (e, s, l, c, n, j)
    ec, ej = np.eye(nc, dtype=LD), np.eye(pm1, dtype=LD)
    AiB = np.einsum("elscnj,cd,jk->enlcjsdk", a, ec, ej).reshape(nex, ney, c.ni, c.G)
    ABi = np.einsum("eslcnj,cd,jk->enscjldk", b, ec, ej).reshape(nex, ney, c.G, c.ni)
    XiB = np.matmul(c.Xi.astype(LD), AiB)
    AXB = np.matmul(c.Aei.astype(LD), XiB)
    ABY = np.matmul(ABi, c.Yie.astype(LD))
    return XiB.astype(np.float64), AXB.astype(np.float64), ABY.astype(np.float64)


# ---- the shapes the GPU tests run (test_gpu_condense_launches.py; the CPU tests check every bound's cap on them) ----

# (nc, P): ni = 1 (fewer columns than splits), 64, 72, 128 (the last RP = 128), 144, 162 (row loop), 288, 450 (the row
# loop past 256); 2 ne1 crosses 64 between (2, 16) and below
REGIMES = [(1, 2), (1, 9), (2, 7), (2, 9), (1, 13), (2, 10), (2, 13), (2, 16)]
# (nc, P, ney): n_e = 2, 63, 64, 65, 128, 129 across cond_edge_kernel's 64-row tiles
DENSE_EDGES = [(1, 2, 1), (1, 8, 8), (2, 9, 3), (1, 6, 12), (2, 9, 7), (1, 4, 42)]
# (nc, P) of every block width B = nc (P - 1) = 1..32
WIDTHS = [(1, B + 1) for B in range(1, 33)] + [(2, B // 2 + 1) for B in range(2, 33, 2)]
# (nc, P, ney): chains of 2..9 edges against the ring depth D = 3, at B = 1, 2, 7, 8, 30
CHAINS = [(nc, P, ney) for nc, P in ((1, 2), (2, 2), (1, 8), (2, 5), (2, 16)) for ney in range(1, 9)]
# the runtime-width sweep: (nc, P, ney)
RT_SWEEP = [(1, 2, 2), (1, 6, 4), (2, 5, 3), (2, 16, 2), (1, 33, 2), (1, 8, 7)]
# sem_nested_iface_rhs: (nc, P, nex, ney, edge)
IFACE = [(nc, P, nex, ney, edge)
         for nc, P, edge in ((1, 5, "thomas"), (2, 4, "thomas"), (1, 3, "dense"), (2, 6, "dense"))
         for nex in (1, 3) for ney in (1, 3)]
# sem_interface_rhs: (P, nex, m)
INTERFACE = [(P, nex, m) for P in (2, 5, 16) for nex in (1, 3) for m in (1, 255, 256, 257, 770)]


def width_nex_ney(nc, P):
    """Widths the solver cannot reach at the library's largest order (16) run one column of two elements."""
    return (1, 2) if P > 16 else (2, 2)


def solve_cases():
    """Every (P, nex, ney, nc, edge) sem_nested_solve is run at."""
    out = [(P, 2, 2, nc, "thomas") for nc, P in REGIMES]
    out += [(P, 2, ney, nc, "dense") for nc, P, ney in DENSE_EDGES]
    out += [(P,) + width_nex_ney(nc, P) + (nc, "thomas") for nc, P in WIDTHS]
    out += [(P, 1 if P > 16 else 2, ney, nc, "thomas") for nc, P, ney in CHAINS + RT_SWEEP]
    return sorted(set(out))


def back_cases():
    """Every (P, nex, ney, nc, edge) sem_nested_back_solve is run at."""
    return [(P, 2, 2, nc, "thomas") for nc, P in REGIMES] + [(P, 2, 2, nc, "dense") for nc, P in REGIMES[::2]] + \
        [(6, 3, 5, 1, "thomas"), (4, 3, 12, 2, "dense")]
