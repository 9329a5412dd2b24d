"""Test helper (not a test module): tests/cpu_mesh_T.CPUStripMeshT with the transposed Navier-Stokes strip apply.

ns_apply_transpose_part is, by definition, the dense transpose of the strip's OWN forward matrix A_s -- the 3 n_local x
3 n_local matrix CPUStripMesh.ns_apply applies with T, dval_u, dval_v absent and pin_val 0 (local elements only; the
pointwise terms, Dirichlet rows and pinned row of the right interface line left to its owner), built column by column
from identity vectors -- and yT the transpose of its c_T M T column block.  That is the documented semantics of
sem_ns_apply_transpose_part (include/sem_ops.h), computed without the identity G^T = -G + B the HIP kernel rests on.
Every call is recorded in launches_nsT."""
import numpy as np
import torch

from cpu_mesh_T import CPUStripMeshT


class CPUStripMeshNST(CPUStripMeshT):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.launches_nsT = []
        self._ns_dense = {}

    def _ns_forward_matrix(self, key, kw, c_T):
        """(A_s, its T column block) dense for one descriptor."""
        hit = self._ns_dense.get(key)
        if hit is None:
            n, kept = self.n_local, len(self.launches)
            A, AT = np.empty((3 * n, 3 * n)), np.zeros((n, n))
            e = torch.zeros(n, dtype=torch.float64)
            out = [torch.empty(n, dtype=torch.float64) for _ in range(3)]
            for j in range(3 * n):
                ops = [None, None, None]
                ops[j // n] = e
                e[j % n] = 1.0
                self.ns_apply(*ops, *out, **kw)
                A[:, j] = np.concatenate([o.numpy() for o in out])
                e[j % n] = 0.0
            if c_T != 0.0:
                for j in range(n):       # rv is linear in T: the column is rv(T = e_j) at u = v = p = 0
                    e[j] = 1.0
                    self.ns_apply(None, None, None, None, out[1], None, c_T=c_T, T=e, **kw)
                    AT[:, j] = out[1].numpy()
                    e[j] = 0.0
            del self.launches[kept:]      # the identity columns are no launches of the code under test
            if len(self._ns_dense) >= 4:
                self._ns_dense.clear()
            hit = self._ns_dense[key] = (A, AT)
        return hit

    def ns_apply_transpose_part(self, zu=None, zv=None, zc=None, yu=None, yv=None, yp=None, yT=None, *, c_mass=0.0,
                                c_stiff=0.0, c_gradx=0.0, c_grady=0.0, cu=None, cv=None, juu=None, juv=None, jvu=None,
                                jvv=None, c_T=0.0, T=None, c_div=1.0, dval_u=None, dval_v=None, dir_mask=None,
                                dir_sides=0, pin=-1, pin_val=0.0, pin_first=False, stream=None):
        if T is not None or dval_u is not None or dval_v is not None or pin_val != 0.0:
            raise ValueError("the transposed apply is that of the linear part: T, dval_u, dval_v must be NULL and "
                             "pin_val 0")
        self.launches_nsT.append(tuple(nm for nm, t in (("yu", yu), ("yv", yv), ("yp", yp), ("yT", yT))
                                       if t is not None))
        n = self.n_local
        tens = (cu, cv, juu, juv, jvu, jvv, dir_mask)
        key = (c_mass, c_stiff, c_gradx, c_grady, c_T if yT is not None else 0.0, c_div, dir_sides, pin, pin_first) + \
            tuple(None if t is None else t.numpy().tobytes() for t in tens)
        A, AT = self._ns_forward_matrix(key, dict(c_mass=c_mass, c_stiff=c_stiff, c_gradx=c_gradx, c_grady=c_grady,
                                                  cu=cu, cv=cv, juu=juu, juv=juv, jvu=jvu, jvv=jvv, c_div=c_div,
                                                  dir_mask=dir_mask, dir_sides=dir_sides, pin=pin, pin_first=pin_first),
                                        c_T if yT is not None else 0.0)
        z = np.concatenate([np.zeros(n) if t is None else t.numpy() for t in (zu, zv, zc)])
        y = A.T @ z
        for k, t in enumerate((yu, yv, yp)):
            if t is not None:
                t.copy_(torch.from_numpy(y[k * n:(k + 1) * n].copy()))
        if yT is not None:
            yT.copy_(torch.from_numpy(AT.T @ z[n:2 * n]))
        return yu, yv, yp, yT
