"""GPU tests of the transposed nested-dissection kernels (sem_amd/csrc/front_transpose.hip), one launch at a time
through the C ABI on synthetic device arrays, as test_gpu_front_kernels.py tests the forward ones: sem_front_gemv_t
(every lane count, forward and back, with and without the cross-workgroup row split), sem_leaf_sparse_t and
sem_leaf_transpose (every register tile, both sides of each tile boundary), each against the same operation in
np.longdouble on the float64 inputs.

The bounds are derived, not measured: an output the kernel sums in chains of at most L roundings satisfies, to first
order, |got - ref| <= L 2^-53 (|A| |x|); the tests compute that bound per output from absolute values and allow a
factor of 2 over it for the second-order terms (SLACK, as the forward kernels' tests).  Everything a launch must not
write starts as a sentinel and is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
SLACK = 2.0
LD = np.longdouble
SENTINEL = -7.25e77
HUGE = 1e30
LANES = [64, 32, 16, 8, 4]
MAX_PARTS = 16


def _lib():
    from sem_amd import _lib as L
    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _last_error(lib):
    return lib.sem_last_error().decode(errors="replace")


# ---- sem_front_gemv_t ----------------------------------------------------------------------------------------------

class _TLaunch:
    """One sem_front_gemv_t launch over `items` = [(R, K, ld)]: random row-major operators with NaN in the row padding
    (columns K .. ld: not read), operands from a shared pool of W with -1 entries, the outputs with gaps between."""

    def __init__(self, items, lanes, nparts, back, seed, kmax=None):
        L, self.lib = _lib()
        r = np.random.default_rng(seed)
        self.items, self.lanes, self.nparts, self.back = items, lanes, nparts, back
        nf = len(items)
        nop = 1500
        sumK = sum(K for _, K, _ in items)
        self.A, self.xidx = [], []
        off, offs, chunks = 0, [], []
        for f, (R, K, ld) in enumerate(items):
            A = r.uniform(-1, 1, (R, K))
            S = np.full((R, ld), np.nan)
            S[:, :K] = A
            xi = r.integers(1, nop, R)
            xi[r.random(R) < 0.1] = -1
            if f % 2:
                xi[0] = -1
            if f % 3 == 0:
                xi[R - 1] = -1
            self.A.append(A)
            self.xidx.append(xi)
            offs.append(off)
            chunks.append(S.reshape(-1))
            off += S.size                                    # ld even: every operator 16-byte aligned
        self.ops = _dev(np.concatenate(chunks))
        assert self.ops.data_ptr() % 16 == 0
        ptr = np.array([self.ops.data_ptr() + 8 * o for o in offs], dtype=np.int64)
        dims = np.zeros((nf, 4), dtype=np.int32)
        dims[:, :3] = items
        xoff = np.concatenate(([0], np.cumsum([R for R, _, _ in items])[:-1])).astype(np.int64)
        nt = [(K + 2 * lanes - 1) // (2 * lanes) for _, K, _ in items]
        tiles = np.array([(f, c * 2 * lanes, p, 0) for f in range(nf) for c in range(nt[f]) for p in range(nparts)],
                         dtype=np.int32)
        poff = np.concatenate(([0], np.cumsum([K * nparts for _, K, _ in items]))).astype(np.int64)
        self.nW = nop + 2 * sumK + 5
        self.W0 = r.uniform(-1, 1, self.nW)
        self.W0[0] = HUGE
        if back:
            self.yidx = nop + r.permutation(2 * sumK)[:sumK]
            self.yoff = np.concatenate(([0], np.cumsum([K for _, K, _ in items])[:-1])).astype(np.int64)
            self.nstage = 0
        else:
            yo, cur = [], 3
            for _, K, _ in items:
                yo.append(cur)
                cur += K + 3
            self.yoff, self.yidx, self.nstage = np.array(yo, dtype=np.int64), None, cur + 4
        self.keep = dict(ptr=_dev(ptr), dims=_dev(dims), xoff=_dev(xoff), yoff=_dev(self.yoff), poff=_dev(poff[:-1]),
                         tiles=_dev(tiles), xidx=_dev(np.concatenate(self.xidx).astype(np.int32)),
                         yidx=_dev(self.yidx.astype(np.int32)) if back else None,
                         partials=_dev(np.full(int(poff[-1]) + 2, SENTINEL)))
        self.buf = _dev(np.concatenate(([HUGE, HUGE], self.W0)))      # two HUGE entries before W: a -1 used as an index
        self.stage = None if back else _dev(np.full(self.nstage, SENTINEL))
        k = self.keep
        self.d = L.SemFrontTLaunch(len(tiles), lanes, nparts, kmax if kmax is not None else max(R for R, _, _ in items),
                                   int(back), k["ptr"].data_ptr(), k["dims"].data_ptr(), k["xoff"].data_ptr(),
                                   k["yoff"].data_ptr(), k["poff"].data_ptr(), k["tiles"].data_ptr(),
                                   k["xidx"].data_ptr(), k["yidx"].data_ptr() if back else None,
                                   self.buf.data_ptr() + 16, None if back else self.stage.data_ptr(),
                                   k["partials"].data_ptr())

    def reset(self):
        self.buf.copy_(_dev(np.concatenate(([HUGE, HUGE], self.W0))))
        self.keep["partials"].fill_(SENTINEL)
        if self.stage is not None:
            self.stage.fill_(SENTINEL)

    def run(self):
        st = self.lib.sem_front_gemv_t(C.byref(self.d), _stream())
        torch.cuda.synchronize()
        return st, self.buf.cpu().numpy(), None if self.stage is None else self.stage.cpu().numpy()

    def chain(self, R):
        """The longest chain of roundings in one output: a row group's ceil(rp / RG) fused multiply-adds (rp rows per
        part, RG = 256 / lanes row groups), RG - 1 additions over the groups, nparts - 1 over the parts."""
        rg = 256 // self.lanes
        rp = -(-R // self.nparts)
        return -(-rp // rg) + (rg - 1) + (self.nparts - 1)

    def check(self):
        st, buf, stage = self.run()
        assert st == 0, _last_error(self.lib)
        W = buf[2:]
        assert np.array_equal(_bits(buf[:2]), _bits([HUGE, HUGE]))
        assert np.array_equal(_bits(self.keep["partials"].cpu().numpy()[-2:]), _bits([SENTINEL, SENTINEL]))
        written = np.zeros(self.nW if self.back else self.nstage, dtype=bool)
        for f, (R, K, _) in enumerate(self.items):
            xi = self.xidx[f]
            x = np.where(xi >= 0, self.W0[np.maximum(xi, 0)], 0.0).astype(LD)
            A = self.A[f].astype(LD)
            ref, mag = A.T @ x, np.abs(A).T @ np.abs(x)
            bound = self.chain(R) * U53 * mag
            if self.back:
                p = self.yidx[self.yoff[f]:self.yoff[f] + K]
                old = self.W0[p].astype(LD)
                got, ref = W[p], old - ref
                bound = bound + U53 * (np.abs(old) + mag)
                written[p] = True
            else:
                got = stage[self.yoff[f]:self.yoff[f] + K]
                written[self.yoff[f]:self.yoff[f] + K] = True
            err = np.abs(got.astype(LD) - ref)
            assert np.all(np.isfinite(got)), (f, R, K)
            assert np.all(err <= SLACK * bound), (f, R, K, int(np.argmax(err - SLACK * bound)),
                                                  float((err / np.maximum(bound, LD(1e-300))).max()))
        if self.back:
            assert np.array_equal(_bits(W[~written]), _bits(self.W0[~written]))
        else:
            assert np.array_equal(_bits(stage[~written]), _bits(np.full((~written).sum(), SENTINEL)))
            assert np.array_equal(_bits(W), _bits(self.W0))
        self.reset()
        st2, buf2, stage2 = self.run()
        assert st2 == 0
        assert np.array_equal(_bits(buf2), _bits(buf))
        if not self.back:
            assert np.array_equal(_bits(stage2), _bits(stage))


def _t_items(lanes):
    """Every R edge with every K edge: R = 1 and around one sweep of the row groups (RG) and around the unrolled
    batch (4 RG); K = 2 and a pair below, at and above the lane tile (2 lanes columns), and three tiles and a bit;
    row padding (ld > K) on two items of three.  Items of unequal size in one launch."""
    rg = 256 // lanes
    Rs = [1, rg - 1, rg, rg + 1, 4 * rg - 1, 4 * rg, 4 * rg + 1, 9 * rg + 3]
    Ks = [2, 2 * lanes - 2, 2 * lanes, 2 * lanes + 2, 6 * lanes + 6]
    return [(R, K, K + 2 * ((i + j) % 3)) for i, K in enumerate(Ks) if K >= 2 for j, R in enumerate(Rs) if R >= 1]


@pytest.mark.parametrize("back", [0, 1], ids=["forward", "back"])
@pytest.mark.parametrize("lanes", LANES)
def test_front_gemv_t(lanes, back):
    _TLaunch(_t_items(lanes), lanes, 1, back, seed=100 * lanes + back).check()


@pytest.mark.parametrize("back", [0, 1], ids=["forward", "back"])
@pytest.mark.parametrize("nparts", [2, 3, MAX_PARTS])
@pytest.mark.parametrize("lanes", [64, 8])
def test_front_gemv_t_row_split(lanes, nparts, back):
    """The operand rows split over 2, 3 and the maximum number of workgroups: R = 1 and R < nparts (empty parts),
    R around nparts and around a whole sweep per part, a long front; the parts' sums added in a fixed order."""
    rg = 256 // lanes
    Rs = [1, nparts - 1, nparts, nparts + 1, nparts * rg - 1, nparts * rg + 1, 1003]
    items = [(R, K, K + 2 * (j % 2)) for j, R in enumerate(Rs) for K in (2, 2 * lanes + 4)]
    _TLaunch(items, lanes, nparts, back, seed=7 * lanes + nparts + back).check()


@pytest.mark.parametrize("lanes,nparts", [(64, 1), (4, 1), (16, 4)])
def test_front_gemv_t_operand_cap(lanes, nparts):
    """8192 operand rows (64 KiB of LDS unsplit) next to a short item launch and meet the bound; 8194 are refused
    before any launch."""
    L, lib = _lib()
    items = [(8192, 6, 8), (3, 10, 10)]
    t = _TLaunch(items, lanes, nparts, 0, seed=lanes)
    assert t.d.kmax == 8192
    t.check()
    t = _TLaunch(items, lanes, nparts, 0, seed=lanes, kmax=8194)
    st, buf, stage = t.run()
    assert st == L.SEM_EUNSUPPORTED and "front_gemv_t" in _last_error(lib)
    assert np.array_equal(_bits(stage), _bits(np.full(t.nstage, SENTINEL)))
    assert np.array_equal(_bits(buf[2:]), _bits(t.W0))


def test_front_gemv_t_argument_checks():
    L, lib = _lib()
    items = [(5, 8, 8), (3, 6, 8)]

    def refused(back=0, nparts=1, **fields):
        t = _TLaunch(items, 16, nparts, back, seed=3)
        for k, v in fields.items():
            setattr(t.d, k, v)
        st, buf, stage = t.run()
        assert st == L.SEM_EINVAL, (fields, st)
        assert "front_gemv_t" in _last_error(lib)
        with pytest.raises(ValueError):
            L.check(st)
        assert np.array_equal(_bits(buf[2:]), _bits(t.W0))
        if stage is not None:
            assert np.array_equal(_bits(stage), _bits(np.full(t.nstage, SENTINEL)))

    for lanes in (1, 2, 48, 128, 0):
        refused(lanes=lanes)
    for name in ("op", "dims", "xoff", "yoff", "tiles", "xidx", "W"):
        refused(**{name: None})
        refused(back=1, **{name: None})
    refused(back=1, yidx=None)
    refused(back=0, stage=None)
    refused(nparts=2, partials=None)
    refused(nparts=2, poff=None)
    refused(nparts=0)
    refused(nparts=MAX_PARTS + 1)
    refused(ntiles=-1)
    refused(kmax=-2)
    assert lib.sem_front_gemv_t(None, _stream()) == L.SEM_EINVAL and "front_gemv_t" in _last_error(lib)
    d = L.SemFrontTLaunch(0, 16, 1, 8, 0, *([None] * 11))          # no tiles: nothing to do
    assert lib.sem_front_gemv_t(C.byref(d), _stream()) == L.SEM_OK
    assert L.FRONT_T_MAX_PARTS == MAX_PARTS


# ---- sem_leaf_sparse_t / sem_leaf_transpose -------------------------------------------------------------------------

LEAF_N = [1, 2, 4, 16, 31, 32, 33, 36, 63, 64, 65, 95, 96, 97, 100, 120, 121]


def _inverse_tables(r, nint, ncoef, nb):
    """(ipat, brow) (4, nint): interior unknown k has k % 5 boundary couplings (0, 1, .., 4) in its first slots."""
    cnt = np.arange(nint) % 5
    cnt[:3] = (4, 0, 1)[:min(3, nint)]
    ipat = np.where(np.arange(4)[:, None] < cnt[None, :], r.integers(0, ncoef, (4, nint)), -1)
    brow = np.where(ipat >= 0, r.integers(0, nb, (4, nint)), 10 ** 6)     # not read where there is no coupling
    return ipat, brow


def _sparse_ref(coef, ipat, brow, xb):
    """(sum_j coef[ipat] x_b[brow], the same in absolute values) per interior unknown, long double."""
    v, mag = np.zeros(ipat.shape[1], dtype=LD), np.zeros(ipat.shape[1], dtype=LD)
    for j in range(4):
        on = ipat[j] >= 0
        term = np.where(on, coef[np.maximum(ipat[j], 0)].astype(LD) * xb[np.where(on, brow[j], 0)], LD(0))
        v, mag = v + term, mag + np.abs(term)
    return v, mag


class _LeafT:
    def __init__(self, n, nelem, nb, nnz, seed):
        L, self.lib = _lib()
        r = np.random.default_rng(seed)
        self.n, self.E, self.nb, self.nnz = n, nelem, nb, nnz
        ld = self.ld = n + (n & 1)
        size = 2 * n * ld + 2 * ld + nnz * nb
        self.stride = size + (size & 1) + 6
        blob = np.full((nelem, self.stride), np.nan)
        self.Au, self.Sv = r.uniform(-1, 1, (nelem, n, n)), r.uniform(-1, 1, (nelem, n, n))
        self.d1, self.d2 = r.uniform(-1, 1, (nelem, n)), r.uniform(-1, 1, (nelem, n))
        self.coef = r.uniform(-1, 1, (nelem, nnz * nb))
        for e in range(nelem):
            M = np.full((2 * n + 2, ld), np.nan)                 # the pad column: loaded, its products discarded
            M[:n, :n], M[n:2 * n, :n], M[2 * n, :n], M[2 * n + 1, :n] = self.Au[e], self.Sv[e], self.d1[e], self.d2[e]
            blob[e, :M.size] = M.reshape(-1)
            blob[e, M.size:M.size + nnz * nb] = self.coef[e]
        self.ipat, self.brow = _inverse_tables(r, 2 * n, nnz * nb, nb)
        nint = nelem * 2 * n
        self.nW = 3 * nint + nb + 7
        perm = r.permutation(self.nW)
        self.iidx = perm[:nint].reshape(nelem, 2 * n)
        pool = perm[nint:]
        self.bidx = pool[r.integers(0, len(pool), (nelem, nb))]       # shared between elements, never an interior
        self.bidx[r.random((nelem, nb)) < 0.25] = -1                  # Dirichlet positions
        self.bidx[:, 0] = -1
        self.W0 = r.uniform(-1, 1, self.nW)
        self.keep = dict(blob=_dev(blob), iidx=_dev(self.iidx.astype(np.int32)), bidx=_dev(self.bidx.astype(np.int32)),
                         ipat=_dev(self.ipat.astype(np.int32)), brow=_dev(self.brow.astype(np.int32)))
        self.buf = _dev(np.concatenate(([HUGE, HUGE], self.W0)))
        k = self.keep
        self.d = L.SemLeafTLaunch(nelem, n, ld, nb, nnz, self.stride, k["blob"].data_ptr(), k["iidx"].data_ptr(),
                                  k["bidx"].data_ptr(), k["ipat"].data_ptr(), k["brow"].data_ptr(),
                                  self.buf.data_ptr() + 16)

    def run(self):
        st = self.lib.sem_leaf_transpose(C.byref(self.d), _stream())
        torch.cuda.synchronize()
        return st, self.buf.cpu().numpy()[2:]

    def reset(self):
        self.buf.copy_(_dev(np.concatenate(([HUGE, HUGE], self.W0))))

    def reference(self, e):
        """[z_u; z_v] and its first-order error bound: r = b - A_bi^T x_b (four products and their sum, one
        subtraction), t = A_u^T r_u, z_v = S_v^T (r_v - D1 t), z_u = t - A_u^T (D2 z_v), the errors carried through
        in absolute values.  Each transposed n x n product sums a column in a chain of RK fused multiply-adds in the
        thread and 31 additions over the row groups (L = RK + 31); the elementwise steps round twice."""
        n = self.n
        Lp = ((n + 32) // 32 + 31) * U53
        Au, Sv, d1, d2 = (a[e].astype(LD) for a in (self.Au, self.Sv, self.d1, self.d2))
        aAu, aSv, ad1, ad2 = (np.abs(a) for a in (Au, Sv, d1, d2))
        xb = np.where(self.bidx[e] >= 0, self.W0[np.maximum(self.bidx[e], 0)], 0.0).astype(LD)
        s, smag = _sparse_ref(self.coef[e], self.ipat, self.brow, xb)
        b = self.W0[self.iidx[e]].astype(LD)
        r = b - s
        e_r = U53 * (4 * smag + np.abs(b) + smag)
        ru, rv, e_ru, e_rv = r[:n], r[n:], e_r[:n], e_r[n:]
        t = Au.T @ ru
        e_t = aAu.T @ e_ru + Lp * (aAu.T @ np.abs(ru))
        w = rv - d1 * t
        e_w = e_rv + ad1 * e_t + 2 * U53 * (np.abs(rv) + ad1 * np.abs(t))
        zv = Sv.T @ w
        e_zv = aSv.T @ e_w + Lp * (aSv.T @ np.abs(w))
        z = d2 * zv
        e_z = ad2 * e_zv + 2 * U53 * np.abs(z)
        q = Au.T @ z
        e_q = aAu.T @ e_z + Lp * (aAu.T @ np.abs(z))
        zu = t - q
        e_zu = e_t + e_q + 2 * U53 * (np.abs(t) + np.abs(q))
        return np.concatenate((zu, zv)), np.concatenate((e_zu, e_zv))

    def check(self):
        st, W = self.run()
        assert st == 0, _last_error(self.lib)
        wW = np.zeros(self.nW, dtype=bool)
        for e in range(self.E):
            ref, bound = self.reference(e)
            got = W[self.iidx[e]]
            err = np.abs(got.astype(LD) - ref)
            assert np.all(np.isfinite(got)), (self.n, e)
            assert np.all(err <= SLACK * bound), (self.n, e, int(np.argmax(err - SLACK * bound)),
                                                  float((err / np.maximum(bound, LD(1e-300))).max()))
            wW[self.iidx[e]] = True
        assert np.array_equal(_bits(W[~wW]), _bits(self.W0[~wW]))
        self.reset()
        st2, W2 = self.run()
        assert st2 == 0 and np.array_equal(_bits(W2), _bits(W))


@pytest.mark.parametrize("n", LEAF_N)
def test_leaf_transpose(n):
    """Every register tile (RK = (n + 32) / 32 = 1..4), both sides of n = 31|32, 63|64, 95|96, odd n for the pad
    column (NaN here: loaded, never used), the ABI's limits 1 and 121; boundary values at Dirichlet positions given
    as -1; interior unknowns with 0, 1, 2, 3 and 4 boundary contributions; [z_u; z_v] into distinct entries of a
    larger W, nothing else written, twice the same bits."""
    i = LEAF_N.index(n)
    nb = {36: 300, 100: 256 + 131, 64: 100}.get(n, 37)
    _LeafT(n, 3 + i % 3, nb, 1 + (5 * i) % 11, seed=900 + n).check()


def test_leaf_transpose_argument_checks():
    L, lib = _lib()

    def status(**fields):
        t = _LeafT(9, 3, 12, 3, seed=1)
        for k, v in fields.items():
            setattr(t.d, k, v)
        st, W = t.run()
        if st != L.SEM_OK:
            assert "leaf_transpose" in _last_error(lib)
            assert np.array_equal(_bits(W), _bits(t.W0))
        return st, t

    st, t = status()
    assert st == L.SEM_OK
    size = 2 * 9 * 10 + 2 * 10 + 3 * 12
    for bad in (dict(n=0), dict(n=122, ld=122), dict(n=-1), dict(ld=9), dict(ld=11), dict(ld=8),
                dict(stride=size - 2), dict(stride=size + 1), dict(nelem=-1), dict(nb=-1), dict(nnz=-1),
                dict(blob=None), dict(iidx=None), dict(bidx=None), dict(ipat=None), dict(brow=None), dict(W=None),
                dict(blob=t.keep["blob"].data_ptr() + 8)):
        st, _ = status(**bad)
        assert st == L.SEM_EINVAL, bad
        with pytest.raises(ValueError):
            L.check(st)
    assert lib.sem_leaf_transpose(None, _stream()) == L.SEM_EINVAL and "leaf_transpose" in _last_error(lib)
    st, t = status(nelem=0)
    assert st == L.SEM_OK and np.array_equal(_bits(t.buf.cpu().numpy()[2:]), _bits(t.W0))


@pytest.mark.parametrize("nelem,ni,nb", [(7, 100, 40), (3, 300, 12), (2, 1, 4)])
def test_leaf_sparse_t(nelem, ni, nb):
    """W[i] -= A_bi^T x_b on the inverse pattern: items x interior unknowns across the 256-thread workgroups,
    0..4 couplings per unknown, -1 boundary positions; a chain of four products and their sum, then the subtraction."""
    L, lib = _lib()
    r = np.random.default_rng(nelem + ni)
    ncoef = 3 * nb
    cstride = ncoef + 5
    coef = np.full((nelem, cstride), np.nan)
    coef[:, :ncoef] = r.uniform(-1, 1, (nelem, ncoef))
    ipat, brow = _inverse_tables(r, ni, ncoef, nb)
    nW = 3 * nelem * ni + nb + 7
    perm = r.permutation(nW)
    iidx, pool = perm[:nelem * ni].reshape(nelem, ni), perm[nelem * ni:]
    bidx = pool[r.integers(0, len(pool), (nelem, nb))]
    bidx[r.random((nelem, nb)) < 0.25] = -1
    W0 = r.uniform(-1, 1, nW)
    keep = [_dev(coef), _dev(ipat.astype(np.int32)), _dev(brow.astype(np.int32)), _dev(iidx.astype(np.int32)),
            _dev(bidx.astype(np.int32))]
    buf = _dev(np.concatenate(([HUGE, HUGE], W0)))

    def run():
        st = lib.sem_leaf_sparse_t(nelem, ni, nb, keep[0].data_ptr(), cstride, keep[1].data_ptr(), keep[2].data_ptr(),
                                   keep[3].data_ptr(), keep[4].data_ptr(), buf.data_ptr() + 16, _stream())
        torch.cuda.synchronize()
        return st, buf.cpu().numpy()[2:]

    st, W = run()
    assert st == 0, _last_error(lib)
    wW = np.zeros(nW, dtype=bool)
    for e in range(nelem):
        xb = np.where(bidx[e] >= 0, W0[np.maximum(bidx[e], 0)], 0.0).astype(LD)
        s, smag = _sparse_ref(coef[e], ipat, brow, xb)
        b = W0[iidx[e]].astype(LD)
        err = np.abs(W[iidx[e]].astype(LD) - (b - s))
        assert np.all(err <= SLACK * U53 * (4 * smag + np.abs(b) + smag)), (e, float(err.max()))
        wW[iidx[e]] = True
    assert np.array_equal(_bits(W[~wW]), _bits(W0[~wW]))
    buf.copy_(_dev(np.concatenate(([HUGE, HUGE], W0))))
    st2, W2 = run()
    assert st2 == 0 and np.array_equal(_bits(W2), _bits(W))
    # argument checks: nothing launched
    buf.copy_(_dev(np.concatenate(([HUGE, HUGE], W0))))
    for args in ((-1, ni, nb, keep[0].data_ptr(), cstride), (nelem, -1, nb, keep[0].data_ptr(), cstride),
                 (nelem, ni, nb, None, cstride), (nelem, ni, nb, keep[0].data_ptr(), -1)):
        st = lib.sem_leaf_sparse_t(*args, keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(),
                                   keep[4].data_ptr(), buf.data_ptr() + 16, _stream())
        assert st == L.SEM_EINVAL and "leaf_sparse_t" in _last_error(lib)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(buf.cpu().numpy()[2:]), _bits(W0))
