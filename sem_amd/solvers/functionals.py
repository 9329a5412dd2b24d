"""Scalar functionals of the coupled Boussinesq state [T | u | v | p] for BoussinesqCoupler.total_derivatives.

Each functional has
    value(coupler, x)      the scalar F(x)
    gradient(coupler, x)   dF/dx as a coupled vector: the right-hand side of the adjoint solve J^T lam = dF/dx
    partial(coupler, x, p) the explicit dF/dp at fixed x (zero for every functional here)
and works on the coupler's working form (device tensors in device mode, global NumPy vectors in host mode) or, in
device mode, on a global NumPy vector (the gradient then is one too).  The operators come from the solvers' one
fused apply (`_operator`): nothing is assembled.

The pressure block of every gradient here is zero, and a functional added to this module should keep it so or
justify its right-hand side: J^T lam = dF/dx is solvable only for dF/dx in range(J^T), the complement of null(J).
On a regular J (odd element counts in both directions, even P) that is every vector, but the directions J nearly
annihilates are the equal-order discretisation's spurious pressure modes, and with an even element count one of
them is an exact null vector: on 4 x 4 elements, P = 4, the null vector of J has 0.999998 of its norm in the
pressure block (2e-3 in T, 3e-4 in u and in v; CPU oracle at a smooth state).  A gradient with a zero pressure
block is orthogonal to all but that remainder -- WallNusselt's has a relative component of 7e-5 along it, which
is what keeps the adjoint GMRES from atol_gmres on such a mesh -- while a functional of the pressure would put
its whole right-hand side there.
"""
import numpy as np
import torch


def _working(coupler, x):
    """x in the coupler's working form, and whether it came as a global NumPy vector in device mode."""
    host = coupler._device and not isinstance(x, torch.Tensor)
    return (coupler.to_local(x) if host else x), host


def _dot(a, b):
    if isinstance(a, torch.Tensor):
        return torch.dot(a, b).item()
    return float(np.dot(a, b))


class Functional:
    name = "F"

    def partial(self, coupler, x, param):
        """The explicit dF/d(param) at fixed x: none of the functionals here depends on Ra, Re or Pr."""
        return 0.0

    def _blocks(self, coupler, x):
        """(gT, gu, gv) of the gradient in the working form; None for a zero block."""
        raise NotImplementedError

    def gradient(self, coupler, x):
        xl, host = _working(coupler, x)
        n_cd, n_ns = getattr(coupler, "_ncd_loc", 0), getattr(coupler, "_nns_loc", 0)
        blocks = list(self._blocks(coupler, xl)) + [None]
        sizes = ((coupler.Ncd, n_cd),) + ((coupler.Nns, n_ns),) * 3
        g = coupler._join(*(coupler._zeros(*s) if b is None else b for b, s in zip(blocks, sizes)))
        return coupler.to_global(g) if host else g


class WallNusselt(Functional):
    """The consistent heat flux through the west ("W") or east ("E") wall, 1_side^T K T counted in the direction
    from the hot to the cold wall: the stiffness rows of the wall nodes summed, i.e. the weak form's boundary term
    of the discrete solution (no differentiation of T at the wall).  1 for pure conduction between T = +-0.5 on the
    unit square at any resolution.  The gradient is K 1_side in the T block (K is symmetric)."""

    def __init__(self, side="W"):
        if side not in ("W", "E"):
            raise ValueError("WallNusselt: side must be 'W' or 'E'")
        self.side, self.name = side, f"Nu_{side}"

    def _wall(self, coupler, like):
        """sign 1_side on the CD nodes, in the form of `like`."""
        xs = np.asarray(coupler.cd.points[0])
        one = np.isclose(xs, xs.min() if self.side == "W" else xs.max()).astype(np.float64)
        if self.side == "E":
            one = -one
        return coupler.cd._dev(one) if isinstance(like, torch.Tensor) else one

    def value(self, coupler, x):
        xl, _ = _working(coupler, x)
        T = coupler._split(xl)[0]
        return _dot(self._wall(coupler, T), coupler.cd._operator(T, c_stiff=1.0))

    def _blocks(self, coupler, xl):
        T = coupler._split(xl)[0]
        return coupler.cd._operator(self._wall(coupler, T), c_stiff=1.0), None, None


class KineticEnergy(Functional):
    """(u^T M u + v^T M v) / 2 with the NS mesh's mass matrix; the gradient is (M u, M v) in the velocity blocks."""
    name = "KE"

    def value(self, coupler, x):
        xl, _ = _working(coupler, x)
        _, u, v, _ = coupler._split(xl)
        ns = coupler.ns
        return 0.5 * (_dot(u, ns._operator(u, c_mass=1.0)) + _dot(v, ns._operator(v, c_mass=1.0)))

    def _blocks(self, coupler, xl):
        _, u, v, _ = coupler._split(xl)
        return None, coupler.ns._operator(u, c_mass=1.0), coupler.ns._operator(v, c_mass=1.0)


class Linear(Functional):
    """<c, x> for a fixed coupled vector c (global NumPy or working form); the gradient is c.  The caller answers
    for c's pressure block (see the module docstring)."""

    def __init__(self, c, name="linear"):
        self.c, self.name = c, name

    def _c(self, coupler):
        return coupler.to_local(self.c)

    def value(self, coupler, x):
        xl, _ = _working(coupler, x)
        return _dot(self._c(coupler), xl)

    def gradient(self, coupler, x):
        _, host = _working(coupler, x)
        c = self._c(coupler)
        return coupler.to_global(c) if host else c
