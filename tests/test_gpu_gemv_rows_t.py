"""sem_gemv_rows_t / sem_gemv_rows2_t (sem_amd/csrc/block_gemv.hip row_gemv_t_kernel) one launch at a time through the
C ABI, against the product in np.longdouble on the host:

    y[c] = alpha sum_{r<M} A[r lda + c] x[r] + beta y[c]

Per entry |y - ref| <= (M + 4) 2^-53 (|alpha| sum_r |A[r, c] x[r]| + |beta y0[c]|): the standard bound of a dot product
of M terms summed in any order, plus the scalings (nothing measured).  Sizes: fewer rows than row groups, one row over,
a column tile +-1, odd and even K; lda > K; every operand one double off a 16-byte boundary (the 8-byte loads) and
aligned (the 16-byte loads where K and lda are even); both forms.  Bitwise: the two load widths, the two forms and two
repeated calls give equal results.  Guards: entries around y and x, and the lda padding of A, hold NaN or a sentinel and
are neither read into a result nor written.  Also the dual launch, the refusals, graph capture, and the transposed
block-Thomas sweeps on the HIP path against their torch path (tests/test_thomas_T_gemv.py's systems)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_thomas_T_gemv import sweeps_T, thomas_system

pytestmark = pytest.mark.gpu

SENT = 123.25
P = C.c_void_p


def _lib():
    from sem_amd import _lib as L
    return L, L.load()


def _stream(dev):
    return P(torch.cuda.current_stream(dev).cuda_stream)


class Operands:
    """A (M x K, leading dimension lda), x (M) and y (K) inside guarded device buffers, each `off` doubles past a
    512-byte aligned allocation; padding and guards of A and x are NaN, y's guards a sentinel."""

    def __init__(self, dev, M, K, lda, off, seed):
        r = np.random.default_rng(seed)
        self.M, self.K, self.lda, self.off = M, K, lda, off
        self.A = r.uniform(-1, 1, (M, K))
        self.x = r.uniform(-1, 1, M)
        self.y0 = r.uniform(-1, 1, K)
        a = np.full(off + max(M, 1) * lda + 2, np.nan)
        for i in range(M):
            a[off + i * lda: off + i * lda + K] = self.A[i]
        xb = np.full(off + M + 2, np.nan)
        xb[off:off + M] = self.x
        self.dA, self.dx = torch.as_tensor(a, device=dev), torch.as_tensor(xb, device=dev)
        self.dy = torch.empty(off + K + 4, dtype=torch.float64, device=dev)
        self.dev = dev

    def fill_y(self, beta):
        self.dy.fill_(SENT)
        self.dy[self.off:self.off + self.K] = (torch.full((self.K,), float("nan"), dtype=torch.float64) if beta == 0.0
                                               else torch.as_tensor(self.y0)).to(self.dev)

    def args(self):
        return (P(self.dA.data_ptr() + 8 * self.off), self.lda, P(self.dx.data_ptr() + 8 * self.off),
                P(self.dy.data_ptr() + 8 * self.off))

    def run(self, alpha, beta, form):
        L, lib = _lib()
        self.fill_y(beta)
        pA, lda, px, py = self.args()
        L.check(lib.sem_gemv_rows_t(self.M, self.K, alpha, pA, lda, px, beta, py, form, _stream(self.dev)))
        out = self.dy.cpu()
        y = out[self.off:self.off + self.K].clone()
        guards = torch.cat((out[:self.off], out[self.off + self.K:]))
        assert bool((guards == SENT).all()), "entries around y were written"
        return y

    def check(self, y, alpha, beta):
        ld = np.longdouble
        prod = self.A.astype(ld) * self.x.astype(ld)[:, None]
        ref = ld(alpha) * prod.sum(axis=0) + (ld(beta) * self.y0.astype(ld) if beta != 0.0 else 0)
        mag = abs(alpha) * np.abs(prod).sum(axis=0) + (np.abs(ld(beta) * self.y0.astype(ld)) if beta != 0.0 else 0)
        got = y.numpy()
        assert np.isfinite(got).all(), "NaN padding or guards reached a result"
        err = np.abs(got.astype(ld) - ref)
        bound = (self.M + 4) * ld(2.0) ** -53 * mag
        assert (err <= bound).all(), (float((err / np.maximum(bound, ld(1e-300))).max()), self.M, self.K, self.lda)


SCALARS = ((1.0, 0.0), (-1.0, 1.0), (2.0, 0.5))


@pytest.mark.parametrize("M", [1, 7, 16, 17, 257])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 129, 130])
def test_gemv_rows_t_against_longdouble(gpu, M, K):
    for lda in (K, K + 2, K + 3):
        ops = [Operands(gpu, M, K, lda, off, seed=M * 1000 + K) for off in (0, 1)]   # same values, two alignments
        for alpha, beta in SCALARS:
            ys = []
            for op in ops:
                for form in (1, 2):
                    y = op.run(alpha, beta, form)
                    op.check(y, alpha, beta)
                    assert torch.equal(y, op.run(alpha, beta, form)), "not repeatable"
                    ys.append(y)
            y0 = op.run(alpha, beta, 0)      # by size
            for y in ys:    # both load widths (aligned: 16-byte loads when K and lda are even), both forms
                assert torch.equal(y, y0), (M, K, lda, alpha, beta)


@pytest.mark.parametrize("M,K", [(2500, 34), (32 * 512 + 37, 66)])
def test_gemv_rows_t_staged_in_chunks(gpu, M, K):
    """More rows per slice than one LDS stage of x holds (narrow 16-byte form: 64 per group; wide 8-byte form: 512)."""
    ops = [Operands(gpu, M, K, K + 2, off, seed=M) for off in (0, 1)]
    ys = []
    for op in ops:
        for form in (1, 2):
            y = op.run(-1.0, 1.0, form)
            op.check(y, -1.0, 1.0)
            ys.append(y)
    assert all(torch.equal(y, ys[0]) for y in ys)


def test_gemv_rows2_t_equals_two_single_calls(gpu):
    L, lib = _lib()
    M = 17
    for off in (0, 1):
        a, b = Operands(gpu, M, 65 + off, 70, off, seed=1), Operands(gpu, M, 130, 130, off, seed=2)
        for alpha, beta in SCALARS:
            for form in (0, 1, 2):
                want = (a.run(alpha, beta, form), b.run(alpha, beta, form))
                a.fill_y(beta)
                b.fill_y(beta)
                (pA0, l0, px0, py0), (pA1, l1, px1, py1) = a.args(), b.args()
                L.check(lib.sem_gemv_rows2_t(M, alpha, beta, a.K, pA0, l0, px0, py0, b.K, pA1, l1, px1, py1, form,
                                             _stream(gpu)))
                for op, w in zip((a, b), want):
                    out = op.dy.cpu()
                    assert torch.equal(out[op.off:op.off + op.K], w)
                    assert bool((torch.cat((out[:op.off], out[op.off + op.K:])) == SENT).all())
                a.check(want[0], alpha, beta)
    # one empty product: the other still runs
    a.fill_y(0.0)
    pA0, l0, px0, py0 = a.args()
    L.check(lib.sem_gemv_rows2_t(M, 1.0, 0.0, a.K, pA0, l0, px0, py0, 0, None, 0, None, None, 0, _stream(gpu)))
    assert torch.equal(a.dy.cpu()[a.off:a.off + a.K], a.run(1.0, 0.0, 0))


def test_gemv_rows_t_refusals_and_empty_sizes(gpu):
    L, lib = _lib()
    op = Operands(gpu, 7, 9, 10, 0, seed=3)
    op.fill_y(1.0)
    before = op.dy.clone()
    pA, lda, px, py = op.args()
    st = _stream(gpu)
    bad = [((-1, 9, 1.0, pA, lda, px, 1.0, py, 0, st), "bad sizes"), ((7, -1, 1.0, pA, lda, px, 1.0, py, 0, st), "bad sizes"),
           ((7, 9, 1.0, pA, 8, px, 1.0, py, 0, st), "bad sizes"), ((7, 9, 1.0, pA, lda, px, 1.0, py, 3, st), "bad sizes"),
           ((7, 9, 1.0, None, lda, px, 1.0, py, 0, st), "null"), ((7, 9, 1.0, pA, lda, None, 1.0, py, 0, st), "null"),
           ((7, 9, 1.0, pA, lda, px, 1.0, None, 0, st), "null")]
    for args, word in bad:
        status = lib.sem_gemv_rows_t(*args)
        assert status == L.SEM_EINVAL, args
        msg = lib.sem_last_error().decode()
        assert "gemv_rows_t" in msg and word in msg, msg
        with pytest.raises(ValueError, match="gemv_rows_t"):
            L.check(status)
    status = lib.sem_gemv_rows2_t(7, 1.0, 1.0, 9, pA, 8, px, py, 9, pA, lda, px, py, 0, st)
    assert status == L.SEM_EINVAL and "gemv_rows2_t" in lib.sem_last_error().decode()
    status = lib.sem_gemv_rows2_t(7, 1.0, 1.0, 9, pA, lda, px, py, 9, pA, lda, px, None, 0, st)
    assert status == L.SEM_EINVAL and "null" in lib.sem_last_error().decode()
    # K = 0, and M = 0 with beta != 0: nothing to do
    assert lib.sem_gemv_rows_t(7, 0, 1.0, pA, lda, px, 1.0, py, 0, st) == L.SEM_OK
    assert lib.sem_gemv_rows_t(0, 9, 1.0, pA, lda, px, 1.0, py, 0, st) == L.SEM_OK
    torch.cuda.synchronize(gpu)
    assert torch.equal(op.dy, before), "a refused or empty call wrote to y"
    # M = 0, beta = 0: y = 0 (no product, y not read), its guards untouched
    op.fill_y(0.0)
    assert lib.sem_gemv_rows_t(0, 9, 1.0, pA, lda, px, 0.0, py, 0, st) == L.SEM_OK
    out = op.dy.cpu()
    assert bool((out[:9] == 0.0).all()) and bool((out[9:] == SENT).all())


def test_gemv_rows_t_graph_capture(gpu):
    L, lib = _lib()
    op = Operands(gpu, 257, 130, 132, 0, seed=4)
    want = op.run(2.0, 0.0, 0)
    op.fill_y(0.0)
    pA, lda, px, py = op.args()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.check(lib.sem_gemv_rows_t(op.M, op.K, 2.0, pA, lda, px, 0.0, py, 0, _stream(gpu)))
    op.fill_y(0.0)
    g.replay()
    torch.cuda.synchronize(gpu)
    assert torch.equal(op.dy.cpu()[:op.K], want)


@pytest.mark.parametrize("n", [1, 2, 3, 6])
@pytest.mark.parametrize("m", [3, 8])
def test_thomas_T_hip_against_torch(gpu, monkeypatch, n, m):
    """The three transposed sweeps with their products on sem_gemv_rows_t / sem_gemv_rows2_t against the same sweeps
    on torch's A.mT @ x, in one process (the module attribute, not the environment variable)."""
    from sem_amd.solvers import velocity_solve as V
    Sd, Su, Sl, b, _ = thomas_system(n, m, device=gpu)
    keep = b.clone()
    monkeypatch.setattr(V, "_SWEEP_GEMV", "torch")
    want = sweeps_T(Sd, Su, Sl, b)
    monkeypatch.setattr(V, "_SWEEP_GEMV", "hip")
    calls = []
    lib = _lib()[1]
    for name in ("sem_gemv_rows_t", "sem_gemv_rows2_t"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _f=fn, _n=name: (calls.append(_n), _f(*a))[1])
    got = sweeps_T(Sd, Su, Sl, b)
    assert "sem_gemv_rows_t" in calls and (n < 3 or "sem_gemv_rows2_t" in calls), "the HIP products did not run"
    assert set(got) == set(want)
    for name in want:
        err = float((got[name] - want[name]).abs().max() / want[name].abs().max())
        print(name, n, m, err)
        assert err <= 1e-12, (name, err)
    assert torch.equal(b, keep)
