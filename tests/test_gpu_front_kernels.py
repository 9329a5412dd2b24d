"""GPU tests of the nested-dissection front kernels (sem_amd/csrc/front_solve.hip), one launch at a time through the
C ABI on synthetic device arrays: sem_front_gemv (every (lanes, rows) of the row form, forward and back, and the
column form), sem_leaf_forward (every register tile and both sides of each tile boundary), sem_front_sparse_rows and
sem_front_scatter, each against the same operation in np.longdouble on the float64 inputs.

The bounds are derived, not measured: a row that the kernel sums in chains of at most L fused multiply-adds and
additions satisfies, to first order, |got_r - ref_r| <= L 2^-53 (|A| |x|)_r; the tests compute that bound per row
from absolute values and allow a factor of 2 over it for the second-order terms.  A missing or extra term, a row
stored past R or a misread -1 operand is of order one against it.  Everything a launch must not write starts as a
sentinel and is compared bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
SLACK = 2.0                     # over the first-order bound: the second-order terms
LD = np.longdouble
SENTINEL = -7.25e77             # what a launch must leave alone
HUGE = 1e30                     # W[0] and the entries before W: a -1 operand read as an index shows

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sem_amd", "csrc", "front_solve.hip")


def _front_cases():
    """(lanes, rows) -> (RW, U) from the library's SEM_FRONT_CASE dispatch list."""
    with open(_SRC) as f:
        text = f.read()
    return {(int(m[1]), int(m[2])): (int(m[3]), int(m[4]))
            for m in re.finditer(r"SEM_FRONT_CASE\((\d+), (\d+), (\d+), (\d+)\)", text)}


def _shapes():
    from sem_amd.solvers.nested_dissection import NestedDissectionSolver
    return [(lanes, rows) for lanes, pair in sorted(NestedDissectionSolver.SHAPES.items()) for rows in pair]


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


def test_dispatch_list_is_the_python_table():
    """The (lanes, rows) pairs the library dispatches are NestedDissectionSolver.SHAPES, and each kernel's rows per
    workgroup are 4 waves x (64 / lanes) groups x RW rows."""
    cases = _front_cases()
    assert sorted(cases) == sorted(_shapes()) and len(cases) == 10
    for (lanes, rows), (rw, u) in cases.items():
        assert rows == 4 * (64 // lanes) * rw and u >= 1


# ---- sem_front_gemv ------------------------------------------------------------------------------------------------

class _FrontLaunch:
    """One sem_front_gemv launch over `fronts` = [(R, K, ld)]: random operators with NaN in the row padding, operands
    drawn from a shared pool of W (so fronts share indices) with -1 entries, the outputs with gaps between them."""

    def __init__(self, fronts, lanes, rows, form, back, seed, kmax=None):
        L, self.lib = _lib()
        r = np.random.default_rng(seed)
        self.fronts, self.lanes, self.rows, self.form, self.back = fronts, lanes, rows, form, back
        nf = len(fronts)
        nop = 1500
        sumR = sum(R for R, _, _ in fronts)
        self.A, self.xidx = [], []
        off, offs, chunks = 0, [], []
        for f, (R, K, ld) in enumerate(fronts):
            A = r.uniform(-1, 1, (R, K))
            if form == 1:       # A^T: K rows of ld >= R doubles
                S = np.full((K, ld), np.nan)
                S[:, :R] = A.T
            else:               # R rows of ld >= K doubles
                S = np.full((R, ld), np.nan)
                S[:, :K] = A
            xi = r.integers(1, nop, K)
            xi[r.random(K) < 0.1] = -1
            if f % 2:
                xi[0] = -1
            if f % 3 == 0:
                xi[K - 1] = -1  # the last column pair: the masked tail
            self.A.append(A)
            self.xidx.append(xi)
            offs.append(off)
            chunks.append(S.reshape(-1))
            off += S.size + (S.size & 1)        # every operator 16-byte aligned
            if S.size & 1:
                chunks.append(np.full(1, np.nan))
        self.ops = _dev(np.concatenate(chunks))
        assert self.ops.data_ptr() % 16 == 0
        ptr = np.array([self.ops.data_ptr() + 8 * o for o in offs], dtype=np.int64)
        dims = np.zeros((nf, 4), dtype=np.int32)
        dims[:, :3] = fronts
        xoff = np.concatenate(([0], np.cumsum([K for _, K, _ in fronts])[:-1])).astype(np.int64)
        nt = [(R + rows - 1) // rows for R, _, _ in fronts]
        tiles = np.stack((np.repeat(np.arange(nf), nt), np.concatenate([np.arange(n) * rows for n in nt])), 1)
        # W: [0] HUGE, operands 1 .. nop - 1, then (back) the targets among twice as many entries
        self.nW = nop + 2 * sumR + 5
        self.W0 = r.uniform(-1, 1, self.nW)
        self.W0[0] = HUGE
        if back:
            tgt = nop + r.permutation(2 * sumR)[:sumR]
            self.yoff = np.concatenate(([0], np.cumsum([R for R, _, _ in fronts])[:-1])).astype(np.int64)
            self.yidx = tgt
            self.nstage = 0
        else:
            yo, cur = [], 3
            for R, _, _ in fronts:
                yo.append(cur)
                cur += R + 3    # a gap after every front's rows
            self.yoff = np.array(yo, dtype=np.int64)
            self.yidx = None
            self.nstage = cur + 4
        self.keep = dict(ptr=_dev(ptr), dims=_dev(dims), xoff=_dev(xoff), yoff=_dev(self.yoff),
                         tiles=_dev(tiles.astype(np.int32)), xidx=_dev(np.concatenate(self.xidx).astype(np.int32)),
                         yidx=_dev(self.yidx.astype(np.int32)) if back else None)
        # two HUGE entries before W: what a -1 used as an index would read
        self.buf = _dev(np.concatenate(([HUGE, HUGE], self.W0)))
        self.stage = None if back else _dev(np.full(self.nstage, SENTINEL))
        k = self.keep
        self.d = L.SemFrontLaunch(len(tiles), rows, lanes, kmax if kmax is not None else max(K for _, K, _ in fronts),
                                  int(back), form, k["ptr"].data_ptr(), k["dims"].data_ptr(), k["xoff"].data_ptr(),
                                  k["yoff"].data_ptr(), k["tiles"].data_ptr(), k["xidx"].data_ptr(),
                                  k["yidx"].data_ptr() if back else None, self.buf.data_ptr() + 16,
                                  None if back else self.stage.data_ptr())

    def reset(self):
        self.buf.copy_(_dev(np.concatenate(([HUGE, HUGE], self.W0))))
        if self.stage is not None:
            self.stage.fill_(SENTINEL)

    def run(self):
        """(status, W with its two guard entries in front, stage)"""
        st = self.lib.sem_front_gemv(C.byref(self.d), _stream())
        torch.cuda.synchronize()
        return st, self.buf.cpu().numpy(), None if self.stage is None else self.stage.cpu().numpy()

    def chain(self, K):
        """The longest chain of roundings in one row's sum."""
        if self.form == 1:
            return -(-K // 2) + 1
        return -(-K // (2 * self.lanes)) + 1 + int(np.log2(self.lanes))

    def reference(self, f):
        """(A x, |A| |x|) of front f in long double."""
        xi = self.xidx[f]
        x = np.where(xi >= 0, self.W0[np.maximum(xi, 0)], 0.0).astype(LD)
        A = self.A[f].astype(LD)
        return A @ x, np.abs(A) @ np.abs(x)

    def check(self):
        st, buf, stage = self.run()
        assert st == 0, _last_error(self.lib)
        W = buf[2:]
        assert np.array_equal(_bits(buf[:2]), _bits([HUGE, HUGE]))
        written = np.zeros(self.nW if self.back else self.nstage, dtype=bool)
        for f, (R, K, _) in enumerate(self.fronts):
            ref, mag = self.reference(f)
            bound = self.chain(K) * U53 * mag
            if self.back:
                p = self.yidx[self.yoff[f]:self.yoff[f] + R]
                old = self.W0[p].astype(LD)
                got, ref = W[p], old - ref
                bound = bound + U53 * (np.abs(old) + mag)       # the rounding of W_old - v
                written[p] = True
            else:
                got = stage[self.yoff[f]:self.yoff[f] + R]
                written[self.yoff[f]:self.yoff[f] + R] = True
            err = np.abs(got.astype(LD) - ref)
            assert np.all(np.isfinite(got)), (f, R, K)
            assert np.all(err <= SLACK * bound), (f, R, K, int(np.argmax(err - SLACK * bound)),
                                                  float((err / np.maximum(bound, LD(1e-300))).max()))
        if self.back:
            assert np.array_equal(_bits(W[~written]), _bits(self.W0[~written]))
        else:
            assert np.array_equal(_bits(stage[~written]), _bits(np.full((~written).sum(), SENTINEL)))
            assert np.array_equal(_bits(W), _bits(self.W0))
        # the same launch again: bitwise equal
        self.reset()
        st2, buf2, stage2 = self.run()
        assert st2 == 0
        assert np.array_equal(_bits(buf2), _bits(buf))
        if not self.back:
            assert np.array_equal(_bits(stage2), _bits(stage))


def _row_fronts(lanes, rows, U):
    """Every K edge with every R edge, the row padding (ld > K, even) on two fronts of three."""
    it = 2 * lanes * U          # the columns of one iteration of the row loop
    Ks = [2, it - 2, it, it + 2, 2 * (2 * lanes * U + lanes + 1)]   # 2 (lanes U - 1) = it - 2; two iterations + a tail
    Rs = [1, rows - 1, rows, rows + 1, 3 * rows + 2]
    return [(R, K, K + 2 * ((i + j) % 3)) for i, K in enumerate(Ks) for j, R in enumerate(Rs)]


@pytest.mark.parametrize("back", [0, 1], ids=["forward", "back"])
@pytest.mark.parametrize("lanes,rows", _shapes())
def test_front_gemv_rows(lanes, rows, back):
    """Form 0, every (lanes, rows) the planner can choose, forward and back: one launch of 25 fronts, K at the
    edges of the unrolled row loop (one iteration of lanes U column pairs, +- a pair, a tail after two iterations,
    K = 2), R at the edges of the tile (1, rows - 1, rows, rows + 1: the clamped rows of a partly filled group and
    whole waves past the front; three tiles and a bit)."""
    _, U = _front_cases()[(lanes, rows)]
    fronts = _row_fronts(lanes, rows, U)
    _FrontLaunch(fronts, lanes, rows, 0, back, seed=1000 * lanes + rows + back).check()


@pytest.mark.parametrize("back", [0, 1], ids=["forward", "back"])
def test_front_gemv_columns(back):
    """Form 1 (operators stored transposed, a thread per row, 256 rows per workgroup): K around the 8-column batch
    and its even / odd accumulators, R around the workgroup, an odd ld > R with NaN padding."""
    fronts = []
    for i, K in enumerate([2, 6, 8, 10, 14, 16, 130]):
        for j, R in enumerate([1, 255, 256, 257, 600]):
            ld = (R, R + 1 + (R & 1), R + 4)[(i + j) % 3]       # R, the next odd number, R + 4
            fronts.append((R, K, ld))
    assert any(ld > R and ld % 2 for R, _, ld in fronts)
    _FrontLaunch(fronts, 1, 256, 1, back, seed=77 + back).check()


@pytest.mark.parametrize("lanes,rows", [(64, 16), (4, 64)])
def test_front_gemv_operand_cap(lanes, rows):
    """8192 operands (exactly 64 KiB of dynamic LDS) next to a short front launch and meet the bound; 8194 are
    refused before any launch."""
    L, lib = _lib()
    fronts = [(5, 8192, 8192), (3, 6, 8)]
    t = _FrontLaunch(fronts, lanes, rows, 0, 0, seed=lanes)
    assert t.d.kmax == 8192
    t.check()
    t = _FrontLaunch(fronts, lanes, rows, 0, 0, seed=lanes, kmax=8194)
    st, buf, stage = t.run()
    assert st == L.SEM_EUNSUPPORTED and "front_gemv" in _last_error(lib)
    assert np.array_equal(_bits(stage), _bits(np.full(t.nstage, SENTINEL)))
    assert np.array_equal(_bits(buf[2:]), _bits(t.W0))


def test_front_gemv_argument_checks():
    """Every bad descriptor returns SEM_EINVAL with a message, and nothing is written."""
    L, lib = _lib()
    fronts = [(5, 8, 8), (3, 6, 8)]

    def refused(back=0, form=0, lanes=16, rows=16, **fields):
        t = _FrontLaunch(fronts, lanes, rows, form, back, seed=3)
        for k, v in fields.items():
            setattr(t.d, k, v)
        st, buf, stage = t.run()
        assert st == L.SEM_EINVAL, (fields, st)
        assert "front_gemv" in _last_error(lib)
        with pytest.raises(ValueError):
            L.check(st)
        assert np.array_equal(_bits(buf[2:]), _bits(t.W0))
        if stage is not None:
            assert np.array_equal(_bits(stage), _bits(np.full(t.nstage, SENTINEL)))

    refused(form=2)
    refused(form=-1)
    refused(form=1, lanes=1, rows=128)
    refused(lanes=64, rows=8)
    refused(lanes=2, rows=256)
    refused(lanes=16, rows=64)
    for name in ("op", "dims", "xoff", "yoff", "tiles", "xidx", "W"):
        refused(**{name: None})
        refused(back=1, **{name: None})
    refused(back=1, yidx=None)
    refused(back=0, stage=None)
    refused(ntiles=-1)
    refused(kmax=-2)
    assert lib.sem_front_gemv(None, _stream()) == L.SEM_EINVAL and "front_gemv" in _last_error(lib)
    # no tiles: nothing to do, whatever the arrays
    d = L.SemFrontLaunch(0, 16, 16, 8, 0, 0, None, None, None, None, None, None, None, None, None)
    assert lib.sem_front_gemv(C.byref(d), _stream()) == L.SEM_OK


# ---- sem_leaf_forward ----------------------------------------------------------------------------------------------

LEAF_N = [1, 2, 4, 16, 31, 32, 33, 36, 63, 64, 65, 95, 96, 97, 100, 120, 121]


class _LeafLaunch:
    def __init__(self, n, nelem, nb, nnz, seed):
        L, self.lib = _lib()
        r = np.random.default_rng(seed)
        self.n, self.E, self.nb, self.nnz = n, nelem, nb, nnz
        ld = self.ld = n + (n & 1)
        size = 2 * n * ld + 2 * ld + nnz * nb
        self.stride = size + (size & 1) + 6                      # even, with slack nothing reads
        blob = np.full((nelem, self.stride), np.nan)
        self.Au, self.Sv = r.uniform(-1, 1, (nelem, n, n)), r.uniform(-1, 1, (nelem, n, n))
        self.d1, self.d2 = r.uniform(-1, 1, (nelem, n)), r.uniform(-1, 1, (nelem, n))
        self.coef = r.uniform(-1, 1, (nelem, nnz, nb))
        for e in range(nelem):
            M = np.zeros((2 * n + 2, ld))                        # pad entries zero
            M[:n, :n], M[n:2 * n, :n], M[2 * n, :n], M[2 * n + 1, :n] = self.Au[e], self.Sv[e], self.d1[e], self.d2[e]
            blob[e, :M.size] = M.reshape(-1)
            blob[e, M.size:M.size + nnz * nb] = self.coef[e].reshape(-1)
        self.pat = r.integers(0, 2 * n, (nnz, nb))
        self.nW = 3 * nelem * 2 * n + 7
        self.iidx = r.permutation(self.nW)[:nelem * 2 * n].reshape(nelem, 2 * n)
        self.W0 = r.uniform(-1, 1, self.nW)
        self.soff = 5
        self.sstride = self.soff + nb + 9
        self.nstage = nelem * self.sstride + 3
        self.keep = dict(blob=_dev(blob), iidx=_dev(self.iidx.astype(np.int32)), pat=_dev(self.pat.astype(np.int32)))
        self.W = _dev(self.W0)
        self.stage = _dev(np.full(self.nstage, SENTINEL))
        k = self.keep
        self.d = L.SemLeafLaunch(nelem, n, ld, nb, nnz, self.stride, k["blob"].data_ptr(), k["iidx"].data_ptr(),
                                 k["pat"].data_ptr(), self.W.data_ptr(), self.stage.data_ptr(), self.sstride,
                                 self.soff)

    def run(self):
        st = self.lib.sem_leaf_forward(C.byref(self.d), _stream())
        torch.cuda.synchronize()
        return st, self.W.cpu().numpy(), self.stage.cpu().numpy()

    def reset(self):
        self.W.copy_(_dev(self.W0))
        self.stage.fill_(SENTINEL)

    def reference(self, e):
        """(y, g) and their first-order error bounds: t = A_u b_u, y_v = S_v (b_v - D2 t), y_u = t - A_u (D1 y_v),
        g = coef . y[pat], the errors carried through in absolute values.  Each n x n product sums a row in chains
        of 2 RK pair products, the pair sum and three shuffle additions (L = 2 RK + 4); the elementwise steps
        round twice."""
        n = self.n
        Lp = (2 * ((n + 32) // 32) + 4) * U53
        Au, Sv, d1, d2 = (a[e].astype(LD) for a in (self.Au, self.Sv, self.d1, self.d2))
        aAu, aSv, ad1, ad2 = (np.abs(a) for a in (Au, Sv, d1, d2))
        bu, bv = self.W0[self.iidx[e, :n]].astype(LD), self.W0[self.iidx[e, n:]].astype(LD)
        t = Au @ bu
        e_t = Lp * (aAu @ np.abs(bu))
        w = bv - d2 * t
        e_w = ad2 * e_t + 2 * U53 * (np.abs(bv) + ad2 * np.abs(t))
        yv = Sv @ w
        e_yv = aSv @ e_w + Lp * (aSv @ np.abs(w))
        z = d1 * yv
        e_z = ad1 * e_yv + 2 * U53 * np.abs(z)
        q = Au @ z
        e_q = aAu @ e_z + Lp * (aAu @ np.abs(z))
        yu = t - q
        e_yu = e_t + e_q + 2 * U53 * (np.abs(t) + np.abs(q))
        y, e_y = np.concatenate((yu, yv)), np.concatenate((e_yu, e_yv))
        c = self.coef[e].astype(LD)
        g = (c * y[self.pat]).sum(0)
        e_g = (np.abs(c) * e_y[self.pat]).sum(0) + self.nnz * U53 * (np.abs(c) * np.abs(y[self.pat])).sum(0)
        return y, e_y, g, e_g

    def check(self):
        st, W, stage = self.run()
        assert st == 0, _last_error(self.lib)
        wW, wS = np.zeros(self.nW, dtype=bool), np.zeros(self.nstage, dtype=bool)
        for e in range(self.E):
            y, e_y, g, e_g = self.reference(e)
            lo = e * self.sstride + self.soff
            for got, ref, bound in ((W[self.iidx[e]], y, e_y), (stage[lo:lo + self.nb], g, e_g)):
                err = np.abs(got.astype(LD) - ref)
                assert np.all(np.isfinite(got)), (self.n, e)
                assert np.all(err <= SLACK * bound), (self.n, e, int(np.argmax(err - SLACK * bound)),
                                                      float((err / np.maximum(bound, LD(1e-300))).max()))
            wW[self.iidx[e]] = True
            wS[lo:lo + self.nb] = True
        assert np.array_equal(_bits(W[~wW]), _bits(self.W0[~wW]))
        assert np.array_equal(_bits(stage[~wS]), _bits(np.full((~wS).sum(), SENTINEL)))
        self.reset()
        st2, W2, stage2 = self.run()
        assert st2 == 0
        assert np.array_equal(_bits(W2), _bits(W)) and np.array_equal(_bits(stage2), _bits(stage))


def _leaf_nnz(n):
    return 1 + (5 * LEAF_N.index(n)) % 11


def _leaf_case(n):
    nb = {36: 300, 100: 256 + 131, 64: 100}.get(n, 37)       # not a multiple of 256; above 256
    return _LeafLaunch(n, 3 + LEAF_N.index(n) % 3, nb, _leaf_nnz(n), seed=500 + n)


@pytest.mark.parametrize("n", LEAF_N)
def test_leaf_forward(n):
    """Every register tile (RK = (n + 32) / 32 = 1..4), both sides of n = 31|32, 63|64, 95|96, the unsplit orders'
    n = 16, 36, 64, 100 and the ABI's limits 1 and 121: y_i into distinct entries of a larger W, the boundary rows
    into each element's window of the stage, nothing else written, twice the same bits.  The cases' pattern lengths
    are every nnz from 1 to 11."""
    assert {_leaf_nnz(m) for m in LEAF_N} == set(range(1, 12))
    _leaf_case(n).check()


def test_leaf_forward_argument_checks():
    L, lib = _lib()

    def status(**fields):
        t = _LeafLaunch(9, 3, 12, 3, seed=1)
        for k, v in fields.items():
            setattr(t.d, k, v)
        st, W, stage = t.run()
        if st != L.SEM_OK:
            assert "leaf_forward" in _last_error(lib)
            assert np.array_equal(_bits(W), _bits(t.W0))
            assert np.array_equal(_bits(stage), _bits(np.full(t.nstage, SENTINEL)))
        return st, t

    st, t = status()
    assert st == L.SEM_OK
    size = 2 * 9 * 10 + 2 * 10 + 3 * 12
    assert t.stride == size + 6
    for bad in (dict(n=0), dict(n=122, ld=122), dict(n=-1), dict(ld=9), dict(ld=11), dict(ld=8),
                dict(stride=size - 2), dict(stride=size + 1), dict(nelem=-1), dict(nb=-1), dict(nnz=-1),
                dict(sstride=-1), dict(soff=-1), dict(blob=None), dict(iidx=None), dict(pat=None), dict(W=None),
                dict(stage=None), dict(blob=t.keep["blob"].data_ptr() + 8)):
        st, _ = status(**bad)
        assert st == L.SEM_EINVAL, bad
        with pytest.raises(ValueError):
            L.check(st)
    assert lib.sem_leaf_forward(None, _stream()) == L.SEM_EINVAL and "leaf_forward" in _last_error(lib)
    st, _ = status(stride=size, nelem=1)          # exactly the blob
    assert st == L.SEM_OK
    st, t = status(nelem=0)
    assert st == L.SEM_OK
    assert np.array_equal(_bits(t.W.cpu().numpy()), _bits(t.W0))


# ---- sem_front_sparse_rows -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nnz", [0, 1, 3, 11, 15])
@pytest.mark.parametrize("nitems,nrows", [(7, 100), (3, 300)])
def test_front_sparse_rows(nitems, nrows, nnz):
    """Items x rows across the 256-thread workgroups, the output range ending exactly at the stride, nnz = 0
    writing zeros; the operands before out_off are untouched."""
    L, lib = _lib()
    r = np.random.default_rng(10 * nrows + nnz)
    out_off = 41
    stride = out_off + nrows
    coef = r.uniform(-1, 1, (nitems, nnz, nrows))
    pat = r.integers(0, out_off, (nnz, nrows))
    stage0 = r.uniform(-1, 1, nitems * stride + 5)
    for i in range(nitems):
        stage0[i * stride + out_off:(i + 1) * stride] = SENTINEL
    stage0[nitems * stride:] = SENTINEL
    dc, dp = _dev(coef.reshape(-1) if nnz else np.zeros(1)), _dev(pat.astype(np.int32).reshape(-1) if nnz else
                                                                  np.zeros(1, dtype=np.int32))
    outs = []
    for _ in range(2):
        ds = _dev(stage0)
        st = lib.sem_front_sparse_rows(nitems, nrows, nnz, dc.data_ptr(), dp.data_ptr(), ds.data_ptr(), stride,
                                       out_off, _stream())
        torch.cuda.synchronize()
        assert st == L.SEM_OK, _last_error(lib)
        outs.append(ds.cpu().numpy())
    got = outs[0]
    assert np.array_equal(_bits(outs[1]), _bits(got))
    written = np.zeros(stage0.size, dtype=bool)
    for i in range(nitems):
        y = stage0[i * stride:i * stride + out_off].astype(LD)
        c = coef[i].astype(LD)
        ref = (c * y[pat]).sum(0)
        bound = nnz * U53 * (np.abs(c) * np.abs(y[pat])).sum(0)
        o = got[i * stride + out_off:(i + 1) * stride]
        assert np.all(np.abs(o.astype(LD) - ref) <= SLACK * bound), (i, nnz)
        if nnz == 0:
            assert np.array_equal(_bits(o), _bits(np.zeros(nrows)))
        written[i * stride + out_off:(i + 1) * stride] = True
    assert np.array_equal(_bits(got[~written]), _bits(stage0[~written]))


def test_front_sparse_rows_argument_checks():
    L, lib = _lib()
    ds, dc, dp = _dev(np.full(64, SENTINEL)), _dev(np.ones(8)), _dev(np.zeros(8, dtype=np.int32))
    s, c, p = ds.data_ptr(), dc.data_ptr(), dp.data_ptr()
    for args in ((-1, 4, 2, c, p, s, 16, 8), (2, -1, 2, c, p, s, 16, 8), (2, 4, -1, c, p, s, 16, 8),
                 (2, 4, 2, c, p, s, -1, 8), (2, 4, 2, c, p, s, 16, -1), (2, 4, 2, c, p, s, 11, 8),
                 (2, 4, 2, None, p, s, 16, 8), (2, 4, 2, c, None, s, 16, 8), (2, 4, 2, c, p, None, 16, 8)):
        assert lib.sem_front_sparse_rows(*args, _stream()) == L.SEM_EINVAL, args
        assert "front_sparse_rows" in _last_error(lib)
    assert lib.sem_front_sparse_rows(0, 4, 2, None, None, None, 16, 8, _stream()) == L.SEM_OK
    assert lib.sem_front_sparse_rows(2, 0, 2, None, None, None, 16, 8, _stream()) == L.SEM_OK
    torch.cuda.synchronize()
    assert np.array_equal(_bits(ds.cpu().numpy()), _bits(np.full(64, SENTINEL)))


# ---- sem_front_scatter ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ncopy,nacc", [(300, 400), (0, 48), (300, 0), (256, 16), (1, 1)])
def test_front_scatter(ncopy, nacc):
    """Copies and accumulations in one launch (ncopy = 300: the second workgroup holds both kinds), all sixteen
    patterns of -1 among the four sources: NumPy's float64 subtractions in the same order, bit for bit."""
    L, lib = _lib()
    r = np.random.default_rng(ncopy + 7 * nacc)
    nstage, nW = 500, 3 * (ncopy + nacc) + 11
    stage = r.uniform(-1, 1, nstage)
    W0 = r.uniform(-1, 1, nW)
    tgt = r.permutation(nW)[:ncopy + nacc]
    ct, at = tgt[:ncopy], tgt[ncopy:]
    cs = r.integers(0, nstage, ncopy)
    a4 = r.integers(0, nstage, (nacc, 4))
    for j in range(nacc):
        for k in range(4):
            if (j >> k) & 1:
                a4[j, k] = -1
    if nacc >= 16:
        assert len({tuple(row < 0) for row in a4}) == 16
    want = W0.copy()
    want[ct] = stage[cs]
    v = W0[at].copy()
    for k in range(4):
        m = a4[:, k] >= 0
        v[m] = v[m] - stage[a4[m, k]]
    want[at] = v
    i32 = lambda a: _dev(np.asarray(a, dtype=np.int32).reshape(-1)) if np.size(a) else None  # noqa: E731
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    dct, dcs, dat, da4, dst = i32(ct), i32(cs), i32(at), i32(a4), _dev(stage)
    outs = []
    for _ in range(2):
        dW = _dev(W0)
        st = lib.sem_front_scatter(ncopy, ptr(dct), ptr(dcs), nacc, ptr(dat), ptr(da4), dst.data_ptr(),
                                   dW.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert st == L.SEM_OK, _last_error(lib)
        outs.append(dW.cpu().numpy())
    assert np.array_equal(_bits(outs[0]), _bits(want))      # the targets exact, every other entry unchanged
    assert np.array_equal(_bits(outs[1]), _bits(want))
    assert np.array_equal(_bits(dst.cpu().numpy()), _bits(stage))


def test_front_scatter_argument_checks():
    L, lib = _lib()
    dW, dst = _dev(np.full(32, SENTINEL)), _dev(np.ones(32))
    idx = _dev(np.arange(16, dtype=np.int32))
    i, W, s = idx.data_ptr(), dW.data_ptr(), dst.data_ptr()
    assert i % 16 == 0
    for args in ((2, i, i, 2, i, i + 4, s, W),      # acc_src4 4 bytes off its alignment
                 (2, i, i, 2, i, i + 8, s, W), (-1, i, i, 2, i, i, s, W), (2, i, i, -1, i, i, s, W),
                 (2, None, i, 0, None, None, s, W), (2, i, None, 0, None, None, s, W),
                 (0, None, None, 2, None, i, s, W), (0, None, None, 2, i, None, s, W),
                 (2, i, i, 2, i, i, None, W), (2, i, i, 2, i, i, s, None)):
        assert lib.sem_front_scatter(*args, _stream()) == L.SEM_EINVAL, args
        assert "front_scatter" in _last_error(lib)
    assert lib.sem_front_scatter(0, None, None, 0, None, None, None, None, _stream()) == L.SEM_OK
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dW.cpu().numpy()), _bits(np.full(32, SENTINEL)))
