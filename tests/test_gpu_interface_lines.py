"""sem_interface_pack_lines / sem_interface_unpack_lines alone, against NumPy, on ONE GPU: every strip of a partition is
its own handle and the all-reduce between pack and unpack is the host-side sum of the ranks' buffers (what the
collective computes).  Line arrays of width 2 N_y (the velocity solve's [u | v] lines) with pitch = width and
pitch = width + 3, and of width N_y; whole lines and the column list of the four Dirichlet end offsets; every rank
position (left end, middle, right end).  The assembled first / last lines must equal the sums of the neighbours'
partial lines EXACTLY (one addition of two doubles either way), everything else -- other lines, entries outside the
column list, the padding behind `width` -- must stay bit for bit; the invalid calls return SEM_EINVAL and touch
nothing; one strip (G = 1) is a no-op."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _strips(P, nex, ney, G):
    from sem_amd.device import get_mesh
    from sem_amd.parallel import StripPartition
    part = StripPartition(nex, G)
    return part, [get_mesh(P, nex, ney, 1.0 / nex, 1.0 / ney, *part.local_range(r)) for r in range(G)]


@pytest.mark.parametrize("cols_kind", ["whole", "ends"])
@pytest.mark.parametrize("layout", ["uv", "uv_padded", "single"])
@pytest.mark.parametrize("P,nex,ney,G", [(2, 3, 2, 3), (4, 5, 3, 2)])
def test_pack_sum_unpack_assembles_lines(gpu, P, nex, ney, G, layout, cols_kind):
    part, meshes = _strips(P, nex, ney, G)
    NY = ney * P + 1
    width = NY if layout == "single" else 2 * NY
    pitch = width + 3 if layout == "uv_padded" else width
    cols = None
    if cols_kind == "ends":
        cols = [0, NY - 1] if layout == "single" else [0, NY - 1, NY, 2 * NY - 1]
    n = width if cols is None else len(cols)
    idx = np.arange(width) if cols is None else np.asarray(cols)
    rng = np.random.default_rng(P * 10 + G)
    base, bufs = [], []
    for m in meshes:
        lines = m.line_end - m.line_begin + 1
        b = torch.as_tensor(rng.uniform(-1, 1, (lines, pitch)), device=m.device)
        base.append(b)
        # pre-filled with a sentinel: pack must write every slot, zeros where this strip has no line
        buf = torch.full(((G - 1) * n,), 7.0, dtype=torch.float64, device=m.device)
        m.interface_pack_lines(b[:, :width], part.bounds, buf, cols=cols)
        bufs.append(buf)
    before = [b.cpu().numpy().copy() for b in base]
    for r, buf in enumerate(bufs):           # the packed buffer: slot r - 1 the first line, slot r the last, else 0
        want = np.zeros((G - 1, n))
        if r > 0:
            want[r - 1] = before[r][0, idx]
        if r < G - 1:
            want[r] = before[r][-1, idx]
        assert np.array_equal(buf.cpu().numpy().reshape(G - 1, n), want), r
    total = torch.stack(bufs).sum(0)
    for r, (m, b) in enumerate(zip(meshes, base)):
        m.interface_unpack_lines(total, part.bounds, b[:, :width], cols=cols)
        want = before[r].copy()
        if r > 0:
            want[0, idx] = before[r][0, idx] + before[r - 1][-1, idx]
        if r < G - 1:
            want[-1, idx] = before[r][-1, idx] + before[r + 1][0, idx]
        assert np.array_equal(b.cpu().numpy(), want), r      # exact; untouched entries bit for bit
    torch.cuda.synchronize()


def test_invalid_calls_return_einval_and_touch_nothing(gpu):
    from sem_amd import _lib
    lib = _lib.load()
    part, meshes = _strips(2, 3, 2, 3)
    m = meshes[1]
    NY, lines = m.NY, m.line_end - m.line_begin + 1
    w = 2 * NY
    Y = torch.rand((lines, w), dtype=torch.float64, device=m.device)
    buf = torch.full((2 * w,), 7.0, dtype=torch.float64, device=m.device)
    cols = torch.tensor([0, NY - 1], dtype=torch.int32, device=m.device)
    keepY, keepB = Y.clone(), buf.clone()
    good = (C.c_int * 4)(*part.bounds)
    st = m.stream_ptr()
    p = lambda t: C.c_void_p(t.data_ptr())    # noqa: E731

    def both(h, y, width, pitch, c, nc, bounds, G, b):
        return (lib.sem_interface_pack_lines(h, y, width, pitch, c, nc, bounds, G, b, st),
                lib.sem_interface_unpack_lines(h, b, width, pitch, c, nc, bounds, G, y, st))

    bad = {
        "null handle": (None, p(Y), w, w, None, 0, good, 3, p(buf)),
        "null Y": (m._h, None, w, w, None, 0, good, 3, p(buf)),
        "null buf": (m._h, p(Y), w, w, None, 0, good, 3, None),
        "width 0": (m._h, p(Y), 0, w, None, 0, good, 3, p(buf)),
        "pitch < width": (m._h, p(Y), w, w - 1, None, 0, good, 3, p(buf)),
        "cols without a count": (m._h, p(Y), w, w, p(cols), 0, good, 3, p(buf)),
        "a count without cols": (m._h, p(Y), w, w, None, 2, good, 3, p(buf)),
        "null bounds": (m._h, p(Y), w, w, None, 0, None, 3, p(buf)),
        "G = 0": (m._h, p(Y), w, w, None, 0, good, 0, p(buf)),
        "bounds do not cover": (m._h, p(Y), w, w, None, 0, (C.c_int * 4)(0, 1, 2, 4), 3, p(buf)),
        "bounds not increasing": (m._h, p(Y), w, w, None, 0, (C.c_int * 4)(0, 2, 2, 3), 3, p(buf)),
        "strip not in the partition": (m._h, p(Y), w, w, None, 0, (C.c_int * 3)(0, 2, 3), 2, p(buf)),
    }
    for name, args in bad.items():
        assert both(*args) == (_lib.SEM_EINVAL, _lib.SEM_EINVAL), name
    torch.cuda.synchronize()
    assert torch.equal(Y, keepY) and torch.equal(buf, keepB)
    # the Python wrapper checks the column offsets on the host (the library cannot: they live on the device)
    for cl in ([w], [-1], []):
        with pytest.raises(ValueError, match="cols"):
            m.interface_pack_lines(Y, part.bounds, buf, cols=cl)
    with pytest.raises(ValueError, match="buf"):
        m.interface_pack_lines(Y, part.bounds, buf[:w])
    with pytest.raises(ValueError, match="line array"):
        m.interface_unpack_lines(buf, part.bounds, Y[1:])
    assert torch.equal(Y, keepY) and torch.equal(buf, keepB)


def test_one_strip_is_a_noop(gpu):
    part, (m,) = _strips(2, 3, 2, 1)
    lines = m.line_end - m.line_begin + 1
    Y = torch.rand((lines, 2 * m.NY), dtype=torch.float64, device=m.device)
    buf = torch.full((4,), 7.0, dtype=torch.float64, device=m.device)
    keepY, keepB = Y.clone(), buf.clone()
    for cols in (None, [0, m.NY - 1]):
        m.interface_pack_lines(Y, part.bounds, buf, cols=cols)
        m.interface_unpack_lines(buf, part.bounds, Y, cols=cols)
    torch.cuda.synchronize()
    assert torch.equal(Y, keepY) and torch.equal(buf, keepB)
