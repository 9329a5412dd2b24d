"""Test helper (not a test module): tests/cpu_mesh.CPUStripMesh with the transposed strip apply.

apply_transpose_part is, by definition, the dense transpose of the strip's OWN forward matrix A_s -- the matrix
CPUStripMesh.apply applies (local elements only, pointwise terms and Dirichlet rows of the right interface
line left to its owner) built column by column from identity vectors -- plus the accumulate term on the owned
lines; a position range writes only the output lines of those element positions.  That is the documented
semantics of sem_apply_transpose_part (include/sem_ops.h), computed without the identity G^T = -G + B the HIP
kernel rests on."""
import numpy as np
import torch

from cpu_mesh import CPUStripMesh


class CPUStripMeshT(CPUStripMesh):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.launches_T = []
        self._dense = {}

    def _forward_matrix(self, key, kw):
        """A_s dense for one descriptor; kept per descriptor content (a Krylov solve applies one operator)."""
        A = self._dense.get(key)
        if A is None:
            n, kept = self.n_local, len(self.launches)
            A = np.empty((n, n))
            x = torch.zeros(n, dtype=torch.float64)
            for j in range(n):
                x[j] = 1.0
                A[:, j] = self.apply(x, eb=x if kw["ea"] is not None else None, **kw).numpy()
                x[j] = 0.0
            del self.launches[kept:]      # the identity columns are no launches of the code under test
            if len(self._dense) >= 8:
                self._dense.clear()
            self._dense[key] = A
        return A

    def apply_transpose_part(self, z, y=None, *, c_mass=0.0, c_stiff=0.0, c_gradx=0.0, c_grady=0.0, cu=None, cv=None,
                             diag=None, c_acc=0.0, dir_mode=0, dir_mask=None, dir_sides=0, pos=None, stream=None):
        if dir_mode not in (0, 1):
            raise ValueError("the transposed apply takes SEM_DIR_NONE or SEM_DIR_IDENTITY")
        ncols = self.ex_end - self.ex_begin
        if pos is not None and not 0 <= pos[0] < pos[1] <= ncols + 1:
            raise ValueError("element-position range outside [0, ex_end - ex_begin + 1)")
        self.launches_T.append(pos)
        tens = (cu, cv, diag, dir_mask)
        key = (c_mass, c_stiff, c_gradx, c_grady, dir_mode, dir_sides) + tuple(
            None if t is None else t.numpy().tobytes() for t in tens)
        A = self._forward_matrix(key, dict(c_mass=c_mass, c_stiff=c_stiff, c_gradx=c_gradx, c_grady=c_grady, cu=cu, cv=cv,
                                           c_extra=1.0 if diag is not None else 0.0, ea=diag, dir_mode=dir_mode,
                                           dir_mask=dir_mask, dir_sides=dir_sides))
        out = A.T @ z.numpy()
        if y is None:
            y = torch.empty_like(z)
        line = np.arange(self.n_local) // self.NY
        if c_acc != 0.0:
            own = ~((line == ncols * self.P) & (self.ex_end < self.nex))
            out = out + np.where(own, c_acc * y.numpy(), 0.0)     # y_in is not read on a line left to its owner
        if pos is None:
            write = np.ones(self.n_local, dtype=bool)
        else:
            lines = np.zeros(ncols * self.P + 1, dtype=bool)
            for p in range(*pos):
                if p < ncols:
                    lines[p * self.P:(p + 1) * self.P] = True
                else:
                    lines[ncols * self.P] = True
            write = lines[line]
        y.numpy()[write] = out[write]
        return y
