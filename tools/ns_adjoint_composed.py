"""The adjoint Navier-Stokes Schur matvec S^T q = E^T q - B^T J^-T C^T q composed from the general-purpose launches
(Mesh.apply_transpose, Mesh.apply) and torch pointwise operations -- five operator launches and the masks in between,
where the library's _SchurComplementT uses two fused sem_ns_apply_transpose launches.  A second implementation for the
tests (tests/test_gpu_ns_adjoint.py) and the A/B baseline of tools/ns_adjoint_probe.py; the library does not use it."""
import numpy as np
import torch


class ComposedSchurT:
    def __init__(self, ns, vs):
        """ns: a whole-mesh NavierStokesSolver after _calc_jacobians; vs: its factor ready for transposed solves
        (ns._velocity_solver_T())."""
        self.ns, self.vs = ns, vs
        m = ns._mesh
        self.free = m.to_device((~ns._dir.mask_np).astype(np.float64))      # 1 - m
        self.pin = ns._pin

    def grad_T(self, q):
        """(-C^T q) as (bu, bv): w = -(1 - m_c) q, then G_x^T w, G_y^T w."""
        m = self.ns._mesh
        w = -(self.free * q)
        if self.pin >= 0:
            w[self.pin] = 0.0
        return m.apply_transpose(w, c_gradx=1.0), m.apply_transpose(w, c_grady=1.0)

    def div_T(self, xu, xv, q):
        """B^T x + E^T q = G_x^T (1 - m) xu + G_y^T (1 - m) xv + K (m_b q) + e_pin q[pin]."""
        m = self.ns._mesh
        k = (1.0 - self.free) * q
        if self.pin >= 0:
            k[self.pin] = 0.0
        y = m.apply_transpose(self.free * xu, c_gradx=1.0) + m.apply_transpose(self.free * xv, c_grady=1.0)
        y += m.apply(k, c_stiff=1.0)         # K is symmetric
        if self.pin >= 0:
            y[self.pin] += q[self.pin]
        return y

    def __call__(self, q):
        m = self.ns._mesh
        NX, NY = m.NX, m.NY
        bu, bv = self.grad_T(q)
        B = torch.stack((bu.view(NX, NY), bv.view(NX, NY)), dim=1).reshape(NX, 2 * NY)
        X = self.vs._solve_lines_T(B).view(NX, 2, NY)
        return self.div_T(X[:, 0].reshape(-1), X[:, 1].reshape(-1), q)
