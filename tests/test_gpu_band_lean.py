"""The band kernels' division-free tile map and lean epilogue (apply_band.hip, band_tile_map.h) on meshes with
enough tiles to exercise them.

The tile map sends block b to tile L = (run of XCD b % 8) + b / 8 and splits L by a host-computed reciprocal of
tiles_y; the epilogue of an ordinary tile of a form without mass term and with every given coefficient field present
takes a branch that does nothing but combine and store, and its stores are not masked.  A wrong tile or a wrong
branch shows as a node never written or written with another tile's value, so y is prefilled with NaN and compared
with the oracle.  Shapes: tiles_y in {2, 3, 5} x tiles_x in {4, 11} (nblk = 8 .. 55, all but one no multiple of 8)
for P = 8 (ney = 9, 17, 33, nex = 3, 10), P = 2 (TXE = 4) and P = 12, and the middle strip of a 5-column mesh per
order.  Forms: the benchmark's CD operator, the same with only cu or only cv given, with a mass term, with all four
Dirichlet sides, without Dirichlet rows, and the Laplacian -- in both coefficient modes.

Per case, form and mode:
(a) no NaN is left in y;
(b) max|y - y_ref| <= 1e-13 max|y_ref| against the oracle's CSR operators;
(c) the preloaded-argument launch, a repeat, the struct launch and the composed position ranges are bitwise equal.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-13
PE = 40.0
FORMS = ("cd", "cu_only", "cv_only", "mass", "sides4", "no_dir", "lap")

# (P, nex, ney, ex_begin, ex_end); BandShape<P>: P = 8 TXE 1 TYE 8, P = 2 TXE 4 TYE 32, P = 12 TXE 1 TYE 5, so every
# order runs tiles_x = ceil((nex + 1) / TXE) in {4, 11} and tiles_y = ceil((ney + 1) / TYE) in {2, 3, 5}
CASES = ([(8, nex, ney, 0, nex) for nex in (3, 10) for ney in (9, 17, 33)] +
         [(2, nex, ney, 0, nex) for nex in (13, 41) for ney in (33, 65, 129)] +
         [(12, nex, ney, 0, nex) for nex in (3, 10) for ney in (6, 11, 21)] +
         [(8, 5, 17, 1, 4), (2, 5, 65, 1, 4), (12, 5, 11, 1, 4)])


def case_id(c):
    P, nex, ney, eb, ee = c
    return f"P{P}_{nex}x{ney}" + ("" if (eb, ee) == (0, nex) else f"_strip{eb}-{ee}")


def band_tiles(c):
    """(tiles_x, tiles_y) of a whole launch of apply_band.hip's launch_band."""
    P, _, ney, eb, ee = c
    txe, tye = min(4, max(1, 8 // P)), max(1, 64 // P)
    return -(-(ee - eb + 1) // txe), -(-(ney + 1) // tye)


def test_shapes_are_what_the_docstring_says():
    got = {(c[0], c[3] == 0 and c[4] == c[1]): set() for c in CASES}
    for c in CASES:
        got[c[0], c[3] == 0 and c[4] == c[1]].add(band_tiles(c))
    for P in (8, 2, 12):
        assert got[P, True] == {(tx, ty) for tx in (4, 11) for ty in (2, 3, 5)}, (P, got[P, True])
    nblk = sorted({tx * ty for tx, ty in map(band_tiles, CASES[:18])})   # the whole meshes
    assert nblk == [8, 12, 20, 22, 33, 55], nblk


def form_kwargs(form, dev):
    from sem_amd import _lib
    we = dict(dir_mode=_lib.DIR_IDENTITY, dir_sides=_lib.SIDE_W | _lib.SIDE_E)
    conv = dict(c_stiff=1.0, c_gradx=PE, cu=dev["u"], c_grady=PE, cv=dev["v"])
    if form == "cd":
        return dict(**conv, **we)
    if form == "cu_only":   # an absent coefficient field is 1
        return dict(c_stiff=1.0, c_gradx=PE, cu=dev["u"], c_grady=PE, **we)
    if form == "cv_only":
        return dict(c_stiff=1.0, c_gradx=PE, c_grady=PE, cv=dev["v"], **we)
    if form == "mass":
        return dict(c_mass=0.25, **conv, **we)
    if form == "sides4":
        return dict(**conv, dir_mode=_lib.DIR_IDENTITY,
                    dir_sides=_lib.SIDE_W | _lib.SIDE_E | _lib.SIDE_S | _lib.SIDE_N)
    if form == "no_dir":
        return conv
    return dict(c_stiff=1.0)


def references(c, v):
    """{form: y} from the oracle's assembled CSR operators.  A strip's own elements are a (ncols x ney) mesh of the
    same element size; a Dirichlet row on its right interface line belongs to the next strip (this one leaves 0)."""
    from oracle import sem_oracle as O
    P, nex, ney, eb, ee = c
    nc, dx, dy = ee - eb, 1.0 / nex, 1.5 / ney
    NY = ney * P + 1
    x, u, w = v["x"], v["u"], v["v"]
    lap = O.global_stiffness_matrix(P, nc, ney, dx, dy) @ x
    Gx, Gy = O.global_gradient_matrices(P, nc, ney, dx, dy)
    gxx, gyx = Gx @ x, Gy @ x
    gx, gy = np.arange(x.size) // NY + eb * P, np.arange(x.size) % NY
    own = ~((gx == ee * P) & (ee < nex))
    we = (gx == 0) | (gx == nex * P)
    sn = (gy == 0) | (gy == NY - 1)

    def rows(y, r):
        y = y.copy()
        y[r] = np.where(own, x, 0.0)[r]
        return y

    conv = lap + PE * u * gxx + PE * w * gyx
    return {"cd": rows(conv, we), "cu_only": rows(lap + PE * u * gxx + PE * gyx, we),
            "cv_only": rows(lap + PE * gxx + PE * w * gyx, we),
            "mass": rows(conv + 0.25 * (O.global_mass_matrix(P, nc, ney, dx, dy) @ x), we),
            "sides4": rows(conv, we | sn), "no_dir": conv, "lap": lap}


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_band_lean(gpu, c, tuning):
    from sem_amd import _lib
    from sem_amd.device import get_mesh
    P, nex, ney, eb, ee = c
    n = ee - eb
    mesh = get_mesh(P, nex, ney, 1.0 / nex, 1.5 / ney, eb, ee)
    size = (n * P + 1) * (ney * P + 1)
    r = np.random.default_rng([P, nex, ney, eb, ee])
    v = {k: r.uniform(-1, 1, size) for k in ("x", "u", "v")}
    dev = {k: mesh.to_device(t) for k, t in v.items()}
    nan = torch.full_like(dev["x"], float("nan"))
    refs = references(c, v)
    bad = []
    for form in FORMS:
        kw = form_kwargs(form, dev)
        for name, tile in (("dpp", 3), ("imm", 4)):
            tuning(_lib.TUNE_BAND_TILE, tile)
            tuning(_lib.TUNE_BAND_KP, 0)
            ys = [mesh.apply(dev["x"], nan.clone(), algo=_lib.ALGO_BAND, **kw) for _ in range(2)]
            tuning(_lib.TUNE_BAND_KP, -1)
            ys.append(mesh.apply(dev["x"], nan.clone(), algo=_lib.ALGO_BAND, **kw))
            tuning(_lib.TUNE_BAND_KP, 0)
            y = nan.clone()
            for pos in [(0, 1), (n, n + 1), (1, n)]:
                mesh.apply(dev["x"], y, pos=pos, algo=_lib.ALGO_BAND, **kw)
            ys.append(y)
            ys = [t.cpu().numpy() for t in ys]
            key = f"{case_id(c)}/{form}/{name}"
            nans = int(np.isnan(ys[0]).sum())
            err = np.abs(ys[0] - refs[form]).max() / np.abs(refs[form]).max()
            print(f"{key}: NaN {nans}, rel err {err:.3e}")
            if nans:                                                            # (a)
                bad.append(f"{key}: {nans} NaN left in y")
            if not err <= TOL:                                                  # (b)
                bad.append(f"{key}: rel err {err:.3e} > {TOL}")
            for i, t in enumerate(ys[1:], 1):                                   # (c)
                if not np.array_equal(t, ys[0]):
                    bad.append(f"{key}: launch variant {i} differs bitwise ({int((t != ys[0]).sum())} entries)")
    assert not bad, "\n".join(bad)
