"""The transposed block-Thomas sweeps (velocity_solve.plain_thomas_solve_T, fused_thomas_solve_T,
twisted_thomas_solve_T) on their transposed-GEMV helpers (_gemv_t / _gemv2_t; torch's A.mT @ x on the CPU): random
well-conditioned block-tridiagonal systems against numpy's dense solve of S^T.  tests/test_gpu_gemv_rows_t.py runs the
same systems on the GPU, the HIP path against the torch path."""
import numpy as np
import pytest
import torch

from sem_amd.solvers import velocity_solve as V


def thomas_system(n, m, seed=0, device="cpu"):
    """(S_diag, S_up, S_lo, b, dense S) of a random diagonally dominant block-tridiagonal system (float64)."""
    g = torch.Generator().manual_seed(1000 * n + 10 * m + seed)
    rnd = lambda *s: torch.rand(*s, dtype=torch.float64, generator=g) * 2 - 1   # noqa: E731
    Sd = rnd(n, m, m) + 2.0 * m * torch.eye(m, dtype=torch.float64)
    Su, Sl = rnd(max(n - 1, 0), m, m), rnd(max(n - 1, 0), m, m)
    b = rnd(n, m)
    S = torch.zeros((n * m, n * m), dtype=torch.float64)
    for L in range(n):
        S[L * m:(L + 1) * m, L * m:(L + 1) * m] = Sd[L]
        if L < n - 1:
            S[L * m:(L + 1) * m, (L + 1) * m:(L + 2) * m] = Su[L]
            S[(L + 1) * m:(L + 2) * m, L * m:(L + 1) * m] = Sl[L]
    return tuple(t.to(device) for t in (Sd, Su, Sl, b)) + (S,)


def thomas_factors(Sd, Su, Sl):
    """The one-ended block-Thomas factors (Dinv, Uh) as VelocityJacobianSolver._sweep_factor forms them."""
    n, m = Sd.shape[0], Sd.shape[1]
    Dinv, Uh = torch.empty_like(Sd), torch.empty((max(n - 1, 0), m, m), dtype=Sd.dtype, device=Sd.device)
    Dt = Sd[0]
    for L in range(n):
        if L > 0:
            Dt = Sd[L] - Sl[L - 1] @ Uh[L - 1]
        Dinv[L] = torch.linalg.inv(Dt)
        if L < n - 1:
            Uh[L] = Dinv[L] @ Su[L]
    return Dinv, Uh


def sweeps_T(Sd, Su, Sl, b):
    """{name: x} of every transposed sweep that serves this n."""
    n = Sd.shape[0]
    Dinv, Uh = thomas_factors(Sd, Su, Sl)
    out = {"plain": V.plain_thomas_solve_T(Dinv, Sl, Uh, b),
           "fused": V.fused_thomas_solve_T(*V.fused_thomas_operators(Dinv, Sl, Uh), b)}
    if n >= 3:
        inv = lambda A: torch.linalg.inv(A).contiguous()   # noqa: E731  row-major, as the helpers' HIP path needs
        out["twisted"] = V.twisted_thomas_solve_T(V.twisted_thomas_operators(Sd, Su, Sl, inv=inv), b)
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 6])
@pytest.mark.parametrize("m", [3, 8])
def test_thomas_T_cpu(n, m):
    Sd, Su, Sl, b, S = thomas_system(n, m)
    keep = b.clone()
    want = np.linalg.solve(S.numpy().T, b.reshape(-1).numpy())
    got = sweeps_T(Sd, Su, Sl, b)
    assert set(got) == ({"plain", "fused", "twisted"} if n >= 3 else {"plain", "fused"})
    for name, x in got.items():
        err = np.abs(x.reshape(-1).numpy() - want).max() / np.abs(want).max()
        print(name, n, m, err)
        assert err <= 1e-12, (name, err)
    assert torch.equal(b, keep)


def test_gemv_t_helpers_cpu():
    """The helpers' torch forms: y = alpha A^T x + beta y on views, for the scalars the sweeps use and a general pair."""
    g = torch.Generator().manual_seed(5)
    A = torch.rand((7, 12), dtype=torch.float64, generator=g)[:, 1:10]
    x = torch.rand(7, dtype=torch.float64, generator=g)
    for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (1.0, 1.0), (2.0, 0.5)):
        y0 = torch.rand(9, dtype=torch.float64, generator=g)
        y = (torch.full((9,), float("nan"), dtype=torch.float64) if beta == 0.0 else y0.clone())
        V._gemv_t(A, x, y, alpha=alpha, beta=beta)
        want = alpha * (A.mT @ x) + (beta * y0 if beta else 0.0)
        assert (y - want).abs().max() <= 1e-15 * 16
    y0, y1 = torch.zeros(9, dtype=torch.float64), torch.zeros(5, dtype=torch.float64)
    V._gemv2_t((A, x, y0), (A[:, :5], x, y1))
    assert torch.equal(y0, A.mT @ x) and torch.equal(y1, A[:, :5].mT @ x)
