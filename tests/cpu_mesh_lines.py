"""Test helper (not a test module): tests/cpu_mesh_nsT.CPUStripMeshNST with the line-layout interface exchange.

interface_pack_lines / interface_unpack_lines follow the documented semantics of sem_interface_pack_lines /
sem_interface_unpack_lines (include/sem_ops.h) in torch indexing: the first and the last row of a (lines, >= width)
array are this strip's interface lines, slot s of the buffer is partition boundary s (slots of other boundaries are
zero-filled by pack), `cols` restricts the exchange to those in-line offsets.  Every call is recorded in
launches_lines as (name, entries per line)."""
import torch

from cpu_mesh_nsT import CPUStripMeshNST


class CPUStripMeshLines(CPUStripMeshNST):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.launches_lines = []

    def ns_apply_transpose_part(self, zu=None, zv=None, zc=None, yu=None, yv=None, yp=None, yT=None, **kw):
        """The parent's dense transpose, taking zu, zv, yu, yv also as (lines, NY) line views (one row stride, as
        the device entry point does): views are flattened on the way in and written through on the way out."""
        views = [t for t in (zu, zv, yu, yv) if t is not None and t.dim() == 2]
        assert len({t.stride(0) for t in views}) <= 1 and all(t.stride(1) == 1 and t.shape[1] == self.NY for t in views)
        flat = lambda t: t if t is None or t.dim() == 1 else t.reshape(-1).clone()    # noqa: E731
        fu, fv = flat(yu), flat(yv)
        super().ns_apply_transpose_part(flat(zu), flat(zv), zc, fu, fv, yp, yT, **kw)
        for t, f in ((yu, fu), (yv, fv)):
            if t is not None and t.dim() == 2:
                t.copy_(f.view(t.shape))
        return yu, yv, yp, yT

    def _lines_args(self, Y, bounds, cols, width):
        lines = self.n_local // self.NY
        assert Y.dim() == 2 and Y.shape[0] == lines and Y.stride(1) == 1, "Y must be this strip's line array"
        width = Y.shape[1] if width is None else width
        assert 1 <= width <= Y.shape[1]
        idx = torch.arange(width) if cols is None else torch.as_tensor(list(cols))
        assert idx.numel() and int(idx.min()) >= 0 and int(idx.max()) < width
        r = bounds.index(self.ex_begin)
        left, right = (r - 1 if r > 0 else -1), (r if r < len(bounds) - 2 else -1)
        return idx, left, right

    def interface_pack_lines(self, Y, bounds, buf, cols=None, width=None, stream=None):
        idx, left, right = self._lines_args(Y, bounds, cols, width)
        n = idx.numel()
        self.launches_lines.append(("pack", n))
        buf[:(len(bounds) - 2) * n].zero_()
        if left >= 0:
            buf[left * n:(left + 1) * n] = Y[0, idx]
        if right >= 0:
            buf[right * n:(right + 1) * n] = Y[-1, idx]

    def interface_unpack_lines(self, buf, bounds, Y, cols=None, width=None, stream=None):
        idx, left, right = self._lines_args(Y, bounds, cols, width)
        n = idx.numel()
        self.launches_lines.append(("unpack", n))
        if left >= 0:
            Y[0, idx] = buf[left * n:(left + 1) * n]
        if right >= 0:
            Y[-1, idx] = buf[right * n:(right + 1) * n]
