"""GPU parity of the fused transposed apply (sem_apply_transpose) and of the `.T` / rmatvec operator
layer against SciPy transposes of the pinned oracle's matrices.

Tolerance: max|y - y_ref| <= 1e-13 * max|y_ref|.  The identity the kernel builds on,
G^T = -G + boundary term, holds to 5e-16 on these meshes, so the margin is for summation order only.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import sem_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-13
LX, LY = 1.3, 0.7
W, E, S, N = 1, 2, 4, 8


def rel(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@functools.lru_cache(maxsize=None)
def mats(P, nex, ney):
    dx, dy = LX / nex, LY / ney
    Gx, Gy = O.global_gradient_matrices(P, nex, ney, dx, dy)
    return (sp.csr_matrix(O.global_mass_matrix(P, nex, ney, dx, dy)),
            sp.csr_matrix(O.global_stiffness_matrix(P, nex, ney, dx, dy)), sp.csr_matrix(Gx), sp.csr_matrix(Gy))


def get(P, nex, ney):
    from sem_amd.device import get_mesh
    return get_mesh(P, nex, ney, LX / nex, LY / ney)


def matrix(P, nex, ney, cM=0.0, cK=0.0, cX=0.0, cu=None, cY=0.0, cv=None, d=None):
    M, K, Gx, Gy = mats(P, nex, ney)
    n = M.shape[0]
    A = cM * M + cK * K
    A = A + cX * (Gx if cu is None else sp.diags(cu) @ Gx) + cY * (Gy if cv is None else sp.diags(cv) @ Gy)
    if d is not None:
        A = A + sp.diags(d)
    return sp.csr_matrix(A, shape=(n, n))


def identity_rows(A, mask):
    """A with the rows of `mask` replaced by identity rows."""
    L = sp.lil_matrix(A)
    for p in np.flatnonzero(mask):
        L.rows[p], L.data[p] = [int(p)], [1.0]
    return L.tocsr()


def side_mask(P, nex, ney, sides):
    NX, NY = P * nex + 1, P * ney + 1
    gx, gy = np.divmod(np.arange(NX * NY), NY)
    m = np.zeros(NX * NY, dtype=bool)
    for bit, hit in ((W, gx == 0), (E, gx == NX - 1), (S, gy == 0), (N, gy == NY - 1)):
        if sides & bit:
            m |= hit
    return m


TERM_MESHES = [(1, 3, 2), (2, 5, 3), (3, 4, 7), (4, 1, 1), (5, 2, 9), (7, 4, 2), (8, 8, 8), (8, 1, 13), (8, 17, 5),
               (12, 5, 3), (16, 3, 2)]


@pytest.mark.parametrize("P,nex,ney", TERM_MESHES)
def test_terms_and_fused_apply(gpu, P, nex, ney):
    mesh = get(P, nex, ney)
    n = mesh.n_local
    rng = np.random.default_rng(100 * P + 10 * nex + ney)
    z, cu, cv, ea, y0 = (rng.uniform(-1, 1, n) for _ in range(5))
    dev = mesh.to_device
    zd, cud, cvd = dev(z), dev(cu), dev(cv)
    cases = {
        "M": (dict(c_mass=1.0), dict(cM=1.0)),
        "K": (dict(c_stiff=1.0), dict(cK=1.0)),
        "GxT": (dict(c_gradx=1.0), dict(cX=1.0)),
        "GyT": (dict(c_grady=1.0), dict(cY=1.0)),
        "GxT cu": (dict(c_gradx=1.0, cu=cud), dict(cX=1.0, cu=cu)),
        "GyT cv": (dict(c_grady=1.0, cv=cvd), dict(cY=1.0, cv=cv)),
    }
    for name, (kw, mk) in cases.items():
        ref = matrix(P, nex, ney, **mk).T @ z
        err = rel(mesh.apply_transpose(zd, **kw), ref)
        print(f"P={P} {nex}x{ney} {name}: {err:.3e}")
        assert err <= TOL, name
    # everything at once, accumulating into a random y
    ref = matrix(P, nex, ney, cM=0.5, cK=1.0, cX=40.0, cu=cu, cY=40.0, cv=cv, d=3.0 * ea).T @ z + 2.0 * y0
    y = dev(y0).clone()
    out = mesh.apply_transpose(zd, y, c_mass=0.5, c_stiff=1.0, c_gradx=40.0, cu=cud, c_grady=40.0, cv=cvd,
                               diag=dev(3.0 * ea), c_acc=2.0)
    assert out is y
    err = rel(y, ref)
    print(f"P={P} {nex}x{ney} fused: {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("P,nex,ney", [(4, 4, 4), (8, 6, 5), (12, 3, 4), (8, 40, 33)])
def test_dirichlet(gpu, P, nex, ney):
    from sem_amd import _lib
    mesh = get(P, nex, ney)
    n = mesh.n_local
    rng = np.random.default_rng(7 * P + nex)
    z, cu, cv = (rng.uniform(-1, 1, n) for _ in range(3))
    dev = mesh.to_device
    kw = dict(c_stiff=1.0, c_gradx=40.0, cu=dev(cu), c_grady=40.0, cv=dev(cv), dir_mode=_lib.DIR_IDENTITY)
    A = matrix(P, nex, ney, cK=1.0, cX=40.0, cu=cu, cY=40.0, cv=cv)
    explicit = np.random.default_rng(11).uniform(size=n) < 0.1
    variants = {
        "W|E": (side_mask(P, nex, ney, W | E), dict(dir_sides=W | E)),
        "WESN": (side_mask(P, nex, ney, W | E | S | N), dict(dir_sides=W | E | S | N)),
        "explicit": (explicit, dict(dir_mask=torch.as_tensor(explicit.astype(np.uint8), device=mesh.device))),
    }
    for name, (mask, dkw) in variants.items():
        ref = identity_rows(A, mask).T @ z
        err = rel(mesh.apply_transpose(dev(z), **kw, **dkw), ref)
        print(f"P={P} {nex}x{ney} {name}: {err:.3e}")
        assert err <= TOL, name


@pytest.mark.parametrize("P,nex,ney", [(3, 4, 7), (8, 17, 5), (12, 5, 3)])
def test_dot_product_identity(gpu, P, nex, ney):
    """<A_D x, z> = <x, A_D^T z> with the forward kernel on the left."""
    from sem_amd import _lib
    mesh = get(P, nex, ney)
    n = mesh.n_local
    rng = np.random.default_rng(5)
    x, z, cu, cv = (mesh.to_device(rng.uniform(-1, 1, n)) for _ in range(4))
    kw = dict(c_mass=0.5, c_stiff=1.0, c_gradx=40.0, cu=cu, c_grady=40.0, cv=cv, dir_mode=_lib.DIR_IDENTITY,
              dir_sides=W | E)
    Ax = mesh.apply(x, **kw)
    ATz = mesh.apply_transpose(z, **kw)
    lhs, rhs = torch.dot(Ax, z).item(), torch.dot(x, ATz).item()
    bound = TOL * torch.linalg.vector_norm(Ax).item() * torch.linalg.vector_norm(z).item()
    print(f"P={P} {nex}x{ney}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


def test_graph_capture_and_determinism(gpu):
    from sem_amd import _lib
    from sem_amd.device import no_gc
    mesh = get(8, 8, 8)
    n = mesh.n_local
    rng = np.random.default_rng(9)
    z, cu, cv = (mesh.to_device(rng.uniform(-1, 1, n)) for _ in range(3))
    kw = dict(c_stiff=1.0, c_gradx=40.0, cu=cu, c_grady=40.0, cv=cv, dir_mode=_lib.DIR_IDENTITY, dir_sides=W | E)
    eager = mesh.apply_transpose(z, **kw)
    again = mesh.apply_transpose(z, **kw)
    assert torch.equal(eager, again)
    y = torch.zeros_like(z)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with no_gc(), torch.cuda.graph(g):
        mesh.apply_transpose(z, y, **kw)
    y.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)


def test_errors(gpu):
    from sem_amd import _lib
    from sem_amd.device import get_mesh
    mesh = get(4, 2, 3)
    z = mesh.to_device(np.linspace(-1, 1, mesh.n_local))
    other = torch.ones_like(z)
    with pytest.raises(ValueError):
        mesh.apply_transpose(z, c_stiff=1.0, dir_mode=_lib.DIR_REPLACE, dir_sides=W)
    with pytest.raises(ValueError):
        mesh.apply_transpose(z, c_stiff=1.0, eb=other)
    with pytest.raises(ValueError):
        mesh.apply_transpose(z, z, c_stiff=1.0)
    with pytest.raises(RuntimeError, match="whole-mesh"):
        strip = get_mesh(4, 2, 3, LX / 2, LY / 3, ex_begin=0, ex_end=1)
        zs = torch.ones(strip.n_local, dtype=torch.float64, device=strip.device)
        strip.apply_transpose(zs, c_stiff=1.0)
    with pytest.raises(RuntimeError, match="element-position"):
        mesh.apply_transpose(z, c_stiff=1.0, pos=(0, 1))
    assert mesh.transpose_kernel_name() == "sem::apply_transpose<4>"


def test_operator_layer(gpu):
    from sem_amd import SEM
    P, nex, ney = 4, 3, 2
    dx, dy = LX / nex, LY / ney
    n = (P * nex + 1) * (P * ney + 1)
    rng = np.random.default_rng(4)
    u, v, z = (rng.uniform(-1, 1, n) for _ in range(3))
    K = SEM.global_stiffness_matrix(P, nex, ney, dx, dy)
    Cx, Cy = SEM.global_convection_matrices(P, nex, ney, dx, dy)
    Sys = 40.0 * (SEM.tensordot(Cx, u, (1, 0)) + SEM.tensordot(Cy, v, (1, 0))) + K
    ref = Sys.tocsr().T @ z
    zd = Sys.mesh.to_device(z)
    for name, f in (("T @", lambda x: Sys.T @ x), ("rmatvec", Sys.rmatvec), ("transpose() @", lambda x: Sys.transpose() @ x)):
        out = f(z)
        assert isinstance(out, np.ndarray), name
        assert rel(out, ref) <= TOL, name
        out = f(zd)
        assert isinstance(out, torch.Tensor) and out.device == zd.device, name
        assert rel(out, ref) <= TOL, name
    assert rel(Sys.T.matvec(z[:, None])[:, 0], ref) <= TOL
    assert rel(Sys.T.rmatvec(z), Sys @ z) == 0.0
    assert Sys.T.T is Sys
    assert Sys.T.shape == Sys.shape and Sys.T.dtype == Sys.dtype
    assert rel(Sys.T.diagonal(), Sys.diagonal()) < 1e-14
    assert abs(Sys.T.tocsr() - Sys.tocsr().T).max() == 0.0
