"""The transposed apply of a strip's local operator (sem_apply_transpose_part, Mesh.apply_transpose_part).

A strip handle's `apply` applies A_s: partial sums of the strip's own elements on both interface lines, the
pointwise terms and Dirichlet rows of the right interface line left to its right-hand owner (all-zero Dirichlet
rows there).  The new entry point applies A_s^T, so that A^T z = sum_s R_s^T A_s^T R_s z after the forward
exchange.  Checked here, on one GPU with every strip its own handle:

1. against the strip's OWN forward operator: A_s dense from Mesh.apply on identity columns, transposed on the host;
2. assembled (pack, sum, unpack) against Mesh.apply_transpose on the whole mesh and, for P <= 8, the SciPy
   transpose of the oracle's CSR;
3. the dot identity <A_s x, z> = <x, A_s^T z> on middle strips of widths around the tile;
4. position ranges: composed in every order bitwise the unranged result, nothing outside a range touched;
5. repeatability and graph replay;  6. a whole-mesh handle bitwise Mesh.apply_transpose;
7. the OLD entry point unchanged: SHA-256 digests of Mesh.apply_transpose recorded on the parent commit;
8. argument checks leave y untouched.

Tolerance for applies: max|y - ref| <= 1e-13 max|ref|.  Tile shapes (apply_select.h,
BandShape<P>): TYE = 64 // P element rows, TXE = 4, 4, 2, 2 element columns for P = 1..4 and 1 above.
"""
import functools
import hashlib
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-13
LX, LY = 1.3, 0.7
W, E, S, N = 1, 2, 4, 8
STRIPS = [(0, 2), (2, 3), (3, 5)]   # of nex = 5: a left strip, a one-column middle strip, a right strip


def tye(P):
    return max(64 // P, 1)


def txe(P):
    return {1: 4, 2: 4, 3: 2, 4: 2}.get(P, 1)


def get(P, nex, ney, eb=0, ee=None):
    from sem_amd.device import get_mesh
    return get_mesh(P, nex, ney, LX / nex, LY / ney, eb, nex if ee is None else ee)


def rel(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def bits(t):
    return t.view(torch.int64)


def fields(mesh, seed, names):
    r = np.random.default_rng(seed)
    return {k: mesh.to_device(r.uniform(-1, 1, mesh.n_local)) for k in names}


def strip_mask(mesh, seed):
    """An explicit Dirichlet mask with interior nodes and nodes on the strip's first and last line."""
    r = np.random.default_rng(seed)
    m = r.uniform(size=mesh.n_local) < 0.15
    NY = mesh.NY
    m[[1, NY // 2, NY - 1]] = True                      # first line
    m[[-NY, -NY + NY // 2, -2]] = True                   # last line
    m[NY + 1] = True                                     # an interior node (P = 1: of the second line)
    return torch.as_tensor(m.astype(np.uint8), device=mesh.device)


def owned(mesh):
    """1 on the nodes whose pointwise terms this handle writes (all but a right interface line)."""
    o = torch.ones(mesh.n_local, dtype=torch.float64, device=mesh.device)
    if mesh.ex_end < mesh.nex:
        o[-mesh.NY:] = 0.0
    return o


def cd_form(f):
    """(kw of apply_transpose[_part], kw of apply) of one operator: mass, stiffness, both gradients, a diagonal."""
    sys = dict(c_mass=0.5, c_stiff=1.0, c_gradx=40.0, cu=f["cu"], c_grady=30.0, cv=f["cv"])
    return dict(sys, diag=f["d"]), dict(sys, c_extra=1.0, ea=f["d"])


# ------------------------------------------------------------------ 1. the strip's own forward operator
def dense_forward_T(mesh, fwd_kw):
    """A_s^T dense: row j = A_s e_j, from Mesh.apply on identity columns of the same handle."""
    n = mesh.n_local
    AT = torch.empty(n, n, dtype=torch.float64, device=mesh.device)
    x = torch.zeros(n, dtype=torch.float64, device=mesh.device)
    for j in range(n):
        x[j] = 1.0
        mesh.apply(x, AT[j], eb=x, **fwd_kw)
        x[j] = 0.0
    return AT.cpu().numpy()


@pytest.mark.parametrize("eb,ee", STRIPS)
@pytest.mark.parametrize("P", [1, 3, 4, 8, 12, 16])
def test_against_own_forward_operator(gpu, P, eb, ee):
    from sem_amd import _lib
    mesh = get(P, 5, 2, eb, ee)
    f = fields(mesh, [P, eb, ee], ("z", "cu", "cv", "d", "y0"))
    tkw, fkw = cd_form(f)
    z = f["z"].cpu().numpy()
    own = owned(mesh).cpu().numpy()
    variants = {"W|E|S": dict(dir_sides=W | E | S), "mask": dict(dir_mask=strip_mask(mesh, [P, eb]))}
    for name, dkw in variants.items():
        dkw = dict(dkw, dir_mode=_lib.DIR_IDENTITY)
        AT = dense_forward_T(mesh, dict(fkw, **dkw))
        ref = AT @ z + 2.0 * own * f["y0"].cpu().numpy()
        y = f["y0"].clone()
        out = mesh.apply_transpose_part(f["z"], y, c_acc=2.0, **tkw, **dkw)
        assert out is y
        err = rel(y, ref)
        print(f"P={P} strip [{eb},{ee}) {name}: {err:.3e}")
        assert err <= TOL, name


# ------------------------------------------------------------------ 2. assembled against the whole mesh
@functools.lru_cache(maxsize=4)
def oracle_mats(P, nex, ney):
    from oracle import sem_oracle as O
    dx, dy = LX / nex, LY / ney
    Gx, Gy = O.global_gradient_matrices(P, nex, ney, dx, dy)
    return (sp.csr_matrix(O.global_mass_matrix(P, nex, ney, dx, dy)),
            sp.csr_matrix(O.global_stiffness_matrix(P, nex, ney, dx, dy)), sp.csr_matrix(Gx), sp.csr_matrix(Gy))


def identity_rows(A, mask):
    L = sp.lil_matrix(A)
    for p in np.flatnonzero(mask):
        L.rows[p], L.data[p] = [int(p)], [1.0]
    return L.tocsr()


def assemble(full, bounds, launch):
    """launch(mesh, slice) -> the strip's y; returns [(slice, y)] after pack, sum over strips, unpack."""
    G = len(bounds) - 1
    bufs, outs = [], []
    for r in range(G):
        m = get(full.P, full.nex, full.ney, bounds[r], bounds[r + 1])
        sl = slice(m.dof_begin, m.dof_begin + m.n_local)
        y = launch(m, sl)
        buf = torch.empty((G - 1) * m.NY, dtype=torch.float64, device=m.device)
        m.interface_pack(y, bounds, buf)
        bufs.append(buf)
        outs.append((m, sl, y))
    total = torch.stack(bufs).sum(0)   # what the all-reduce returns on every rank
    for m, sl, y in outs:
        m.interface_unpack(total, bounds, y)
    return [(sl, y) for _, sl, y in outs]


@pytest.mark.parametrize("dney", [-1, 0, 1])
@pytest.mark.parametrize("P", range(1, 17))
def test_assembled_against_whole_mesh(gpu, P, dney):
    from sem_amd import _lib
    nex, ney = 5, tye(P) + dney
    full = get(P, nex, ney)
    f = fields(full, [P, ney], ("z", "cu", "cv", "d", "y0"))
    tkw, _ = cd_form(f)
    dkw = dict(dir_mode=_lib.DIR_IDENTITY, dir_sides=W | E | S, c_acc=2.0)
    want = full.apply_transpose(f["z"], f["y0"].clone(), **tkw, **dkw)

    def launch(m, sl):
        loc = {k: (v[sl].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in tkw.items()}
        return m.apply_transpose_part(f["z"][sl].contiguous(), f["y0"][sl].clone(), **loc, **dkw)

    parts = assemble(full, [0, 2, 3, 5], launch)
    err = max(rel(y, want[sl]) for sl, y in parts)
    print(f"P={P} 5x{ney} assembled vs whole-mesh kernel: {err:.3e}")
    assert err <= TOL
    if P <= 8:
        M, K, Gx, Gy = oracle_mats(P, nex, ney)
        np_ = {k: v.cpu().numpy() for k, v in f.items()}
        A = 0.5 * M + K + 40.0 * sp.diags(np_["cu"]) @ Gx + 30.0 * sp.diags(np_["cv"]) @ Gy + sp.diags(np_["d"])
        NY = full.NY
        gx, gy = np.divmod(np.arange(full.n_local), NY)
        mask = (gx == 0) | (gx == full.NX - 1) | (gy == 0)
        ref = identity_rows(sp.csr_matrix(A), mask).T @ np_["z"] + 2.0 * np_["y0"]
        err = max(rel(y, ref[sl]) for sl, y in parts)
        print(f"P={P} 5x{ney} assembled vs oracle CSR transpose: {err:.3e}")
        assert err <= TOL


# ------------------------------------------------------------------ 3. strip widths around the tile
@pytest.mark.parametrize("P", [2, 4, 8])
def test_dot_identity_strip_widths(gpu, P):
    from sem_amd import _lib
    t = txe(P)
    for ncols in (1, t, t + 1, 2 * t + 1):
        mesh = get(P, ncols + 2, tye(P) + 1, 1, 1 + ncols)   # a middle strip: both edge lines are interfaces
        f = fields(mesh, [P, ncols], ("x", "z", "cu", "cv", "d"))
        tkw, fkw = cd_form(f)
        for dkw in (dict(dir_sides=S | N), dict(dir_mask=strip_mask(mesh, [P, ncols]))):
            dkw = dict(dkw, dir_mode=_lib.DIR_IDENTITY)
            Ax = mesh.apply(f["x"], eb=f["x"], **fkw, **dkw)
            ATz = mesh.apply_transpose_part(f["z"], **tkw, **dkw)
            lhs, rhs = torch.dot(Ax, f["z"]).item(), torch.dot(f["x"], ATz).item()
            print(f"P={P} ncols={ncols}: lhs {lhs:.15e} rhs {rhs:.15e} diff {abs(lhs - rhs):.3e}")
            assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))


# ------------------------------------------------------------------ 4. position ranges
def range_lines(mesh, pos):
    """Boolean mask over the local vector of the nodes positions [pos[0], pos[1]) write."""
    P, n = mesh.P, mesh.ex_end - mesh.ex_begin
    lines = np.zeros(n * P + 1, dtype=bool)
    for p in range(*pos):
        if p < n:
            lines[p * P:(p + 1) * P] = True
        else:
            lines[n * P] = True
    return torch.as_tensor(np.repeat(lines, mesh.NY), device=mesh.device)


RANGE_STRIPS = [(P, 5, eb, ee) for P in (2, 4, 8) for eb, ee in STRIPS] + [(4, 7, 1, 6), (1, 11, 1, 10), (8, 4, 0, 4)]


@pytest.mark.parametrize("P,nex,eb,ee", RANGE_STRIPS)
def test_position_ranges(gpu, P, nex, eb, ee):
    from sem_amd import _lib
    mesh = get(P, nex, tye(P) + 1, eb, ee)
    n = ee - eb
    f = fields(mesh, [P, nex, eb], ("z", "cu", "cv", "d"))
    tkw, _ = cd_form(f)
    for dkw in (dict(dir_sides=W | E | S), dict(dir_mask=strip_mask(mesh, [P, nex]))):
        kw = dict(tkw, dir_mode=_lib.DIR_IDENTITY, **dkw)
        want = mesh.apply_transpose_part(f["z"], **kw)
        assert not torch.isnan(want).any()
        three = [(0, 1), (n, n + 1)] + ([(1, n)] if n > 1 else [])     # n = 1: the interior range is empty
        for order in itertools.permutations(three):
            y = torch.full_like(want, float("nan"))
            for pos in order:
                mesh.apply_transpose_part(f["z"], y, pos=pos, **kw)
            assert torch.equal(bits(y), bits(want)), order
        singles = three + [(0, n + 1)] + ([(1, 2), (n - 1, n + 1)] if n > 2 else [])
        for pos in singles:
            y = torch.full_like(want, float("nan"))
            before = bits(y).clone()
            mesh.apply_transpose_part(f["z"], y, pos=pos, **kw)
            wr = range_lines(mesh, pos)
            assert torch.equal(bits(y)[wr], bits(want)[wr]), pos
            assert torch.equal(bits(y)[~wr], before[~wr]), pos
    y = torch.full_like(want, float("nan"))
    for pos in ((1, 1), (2, 1), (-1, 1), (0, n + 2), (n + 1, n + 2), (1, 0)):
        with pytest.raises(ValueError):
            mesh.apply_transpose_part(f["z"], y, pos=pos, **kw)
    assert torch.isnan(y).all()


# ------------------------------------------------------------------ 5. repeatability
@pytest.mark.parametrize("P,nex,eb,ee", [(8, 5, 2, 3), (4, 7, 1, 6), (12, 5, 3, 5)])
def test_repeatable_and_graph_replay(gpu, P, nex, eb, ee):
    from sem_amd import _lib
    from sem_amd.device import no_gc
    mesh = get(P, nex, tye(P) + 1, eb, ee)
    n = ee - eb
    f = fields(mesh, [P, nex, 5], ("z", "cu", "cv", "d"))
    kw = dict(cd_form(f)[0], dir_mode=_lib.DIR_IDENTITY, dir_sides=W | E | S)
    eager = mesh.apply_transpose_part(f["z"], **kw)
    assert torch.equal(bits(eager), bits(mesh.apply_transpose_part(f["z"], **kw)))
    y, y2 = torch.zeros_like(eager), torch.zeros_like(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with no_gc(), torch.cuda.graph(g):
        mesh.apply_transpose_part(f["z"], y, **kw)
        for pos in [(0, 1), (n, n + 1)] + ([(1, n)] if n > 1 else []):
            mesh.apply_transpose_part(f["z"], y2, pos=pos, **kw)
    y.zero_()
    y2.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(y), bits(eager)) and torch.equal(bits(y2), bits(eager))


# ------------------------------------------------------------------ 6. / 7. whole-mesh handles, old entry point
DIGEST_MESHES = [(4, 4, 3), (8, 9, 7), (12, 5, 4)]
DIGEST_VARIANTS = ("cd", "cd_acc_diag", "mask", "sides_all", "plain")


def whole_case(P, nex, ney, variant):
    """(mesh, z, y0, kw) of one whole-mesh case; the inputs depend on the seed alone."""
    from sem_amd import _lib
    mesh = get(P, nex, ney)
    f = fields(mesh, [P, nex, ney], ("z", "cu", "cv", "d", "y0"))
    cd = dict(c_stiff=1.0, c_gradx=40.0, cu=f["cu"], c_grady=40.0, cv=f["cv"])
    mask = torch.as_tensor((np.random.default_rng([P, nex]).uniform(size=mesh.n_local) < 0.15).astype(np.uint8),
                           device=mesh.device)
    kw = {
        "cd": dict(cd, dir_mode=_lib.DIR_IDENTITY, dir_sides=W | E),
        "cd_acc_diag": dict(cd, c_mass=0.5, diag=f["d"], c_acc=2.0, dir_mode=_lib.DIR_IDENTITY, dir_sides=W | E | S),
        "mask": dict(cd, diag=f["d"], dir_mode=_lib.DIR_IDENTITY, dir_mask=mask),
        "sides_all": dict(cd, dir_mode=_lib.DIR_IDENTITY, dir_sides=W | E | S | N),
        "plain": dict(cd, c_mass=0.25),
    }[variant]
    return mesh, f["z"], f["y0"], kw


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy(), dtype=np.float64).tobytes()).hexdigest()


def old_entry_digests():
    """{case: SHA-256 of Mesh.apply_transpose's y}: what DIGESTS records (run on the parent commit to record)."""
    out = {}
    for P, nex, ney in DIGEST_MESHES:
        for v in DIGEST_VARIANTS:
            mesh, z, y0, kw = whole_case(P, nex, ney, v)
            out[f"P{P}_{nex}x{ney}/{v}"] = sha(mesh.apply_transpose(z, y0.clone(), **kw))
    return out


@pytest.mark.parametrize("P,nex,ney", DIGEST_MESHES + [(1, 9, 65), (16, 2, 5)])
def test_whole_mesh_handle_bitwise_old_entry(gpu, P, nex, ney):
    for v in DIGEST_VARIANTS:
        mesh, z, y0, kw = whole_case(P, nex, ney, v)
        old = mesh.apply_transpose(z, y0.clone(), **kw)
        new = mesh.apply_transpose_part(z, y0.clone(), **kw)
        assert torch.equal(bits(old), bits(new)), v


def test_old_entry_point_digests(gpu):
    """Mesh.apply_transpose computes bit for bit what it computed before the kernel learnt strips and ranges."""
    got = old_entry_digests()
    bad = [f"{k}: {d} != recorded {DIGESTS[k]}" for k, d in got.items() if d != DIGESTS[k]]
    assert not bad and len(got) == len(DIGESTS), "\n".join(bad)


def test_strip_operator_transpose(gpu):
    """`A.T @ x` and rmatvec on a strip operator give the strip's partial sums, as `A @ x` does."""
    from sem_amd.operators import SEMOperator
    mesh = get(4, 5, 3, 2, 4)
    f = fields(mesh, [4, 77], ("x", "z", "cu", "d"))
    A = SEMOperator(mesh, cM=0.5, cK=1.0, gx=[(40.0, f["cu"])], dg=[(1.0, f["d"])])
    want = mesh.apply_transpose_part(f["z"], c_mass=0.5, c_stiff=1.0, c_gradx=1.0, cu=40.0 * f["cu"], diag=f["d"])
    for got in (A.T @ f["z"], A.rmatvec(f["z"]), A.transpose() @ f["z"]):
        assert torch.equal(bits(got), bits(want))
    out = A.T @ f["z"].cpu().numpy()
    assert isinstance(out, np.ndarray) and np.array_equal(out, want.cpu().numpy())
    lhs, rhs = torch.dot(A @ f["x"], f["z"]).item(), torch.dot(f["x"], A.T @ f["z"]).item()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))


# ------------------------------------------------------------------ 8. argument checks
def test_argument_checks_leave_y_untouched(gpu):
    from sem_amd import _lib
    mesh = get(4, 5, 3, 2, 4)
    z = mesh.to_device(np.linspace(-1, 1, mesh.n_local))
    other = torch.ones_like(z)
    y = torch.full_like(z, float("nan"))
    bad = [
        (ValueError, dict(dir_mode=_lib.DIR_REPLACE, dir_sides=W)),
        (ValueError, dict(eb=other)),
        (ValueError, dict(ec=other)),
        (ValueError, dict(ed=other)),
        (ValueError, dict(dir_val=other)),
        (ValueError, dict(pos=(0, 4))),
        (ValueError, dict(pos=(2, 2))),
        (ValueError, dict(pos=(-1, 1))),
    ] + [(RuntimeError, dict(algo=a)) for a in (_lib.ALGO_VALU, _lib.ALGO_MFMA, _lib.ALGO_COLUMN, _lib.ALGO_BAND)]
    for exc, kw in bad:
        with pytest.raises(exc):
            mesh.apply_transpose_part(z, y, c_stiff=1.0, **kw)
    with pytest.raises(ValueError):
        mesh.apply_transpose_part(z, z, c_stiff=1.0)
    assert torch.isnan(y).all()
    assert torch.equal(z, mesh.to_device(np.linspace(-1, 1, mesh.n_local)))
    # the old entry point still refuses what it refused
    with pytest.raises(RuntimeError, match="whole-mesh"):
        mesh.apply_transpose(z, y, c_stiff=1.0)
    assert torch.isnan(y).all()


# Recorded on an MI355X from a build of the parent commit a307f77: old_entry_digests().
DIGESTS = {
    "P4_4x3/cd": "4edcc49d9009e6254a855c28ea3f08a5cb34ec1f1d895a002b6f8a40019f85e1",
    "P4_4x3/cd_acc_diag": "92f9adfed25fd8970011e65ea3d25024c3445d38b0e10a22c7790be2203e2f87",
    "P4_4x3/mask": "087d4bf5c2a3aa54b0d54ad05c42be65cbcfd88015729e32ac0bf611b5a7f7df",
    "P4_4x3/sides_all": "6a1ce8107290c6112fc56ba9da0e9349f6a8b209f6737272b90321bcfc5139fc",
    "P4_4x3/plain": "c92ed2784a09e04a5ff07906a347677c0b73b891edfb325dc5ee1453a5a0abb6",
    "P8_9x7/cd": "569af979f68321095beb1b8559366575311f610d2b6443c4d22a49bfc154d7e0",
    "P8_9x7/cd_acc_diag": "146937cddc336ae483eecb43ae596b7c5abc301d91ad577c74fd1c65c070ad26",
    "P8_9x7/mask": "053a2b3bb6ce21bc275f657c85cdd7fb2191f3288ba3c2d13b0ac3be13887037",
    "P8_9x7/sides_all": "4f3ce133ff4de55cabb0a17fd93fc5186732779d34b50a49af837efd695c4483",
    "P8_9x7/plain": "8af0d19472c955c770acd77800cc083a89a9d1a88508b7a9a60a1bb55ee0cfbd",
    "P12_5x4/cd": "211573f5bd11791c4bab55c2a5dea0e9d4abc4e3cb81ae462223de2562606f97",
    "P12_5x4/cd_acc_diag": "9ebaffc8b5e6dd88abe6172c42c6bb4c9873ae2a10aa60cecf228b4e93438758",
    "P12_5x4/mask": "ded782d67be23c9d21c30b08466f6b5e89c7438a00ae5547cb9a031d6d779e0e",
    "P12_5x4/sides_all": "ab12cab0a338443a9bdf76ae3873079067e94ea5955d91047eba3d1fd80db761",
    "P12_5x4/plain": "cdcebc8c3bf179f912454f7d7d88848ed4802d6312bce3c6a231ac1eb4e5e51b",
}
