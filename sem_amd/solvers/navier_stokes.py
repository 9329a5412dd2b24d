"""Navier-Stokes solver counterpart on the device operators.

Mirrors Solvers/NavierStokes_Solver.py:10-306 (same constructor, same private
methods the OpenMDAO component calls, same errors).  The operator applies run on
the GPU as fused launches:

  * `_get_residuals`  (:93-121): res_u = Sys u + G_x p, res_v = Sys v + G_y p - Gr/Re M T,
    res_cont = G_x u + G_y v, with the reference's Dirichlet / pinned-pressure /
    artificial-Neumann (`K[mask,:] @ p`) rows -- one sem_ns_apply launch for all three outputs.
  * `_calc_jacobians` (:123-136): Re diag(G_x u) ... as closed-form operators.
  * `_get_dresiduals` (:138-160): the velocity Jacobian blocks applied matrix-free, one launch.

`_get_update` keeps the reference's algorithm -- a direct velocity solve inside a pressure
Schur-complement Krylov solve with the mass-diagonal preconditioner (NavierStokes_Solver.py:162-236)
-- entirely on the device: the velocity Jacobian is factored by static condensation over node
lines (sem_amd/solvers/velocity_solve.py, blocks written by the sem_velocity_blocks HIP kernel)
instead of host SuperLU, and the Schur system runs the device GMRES.  No CSR matrix is formed.
"""
import gc
import os
import time
import typing

import numpy as np
import torch

from .. import SEM, _lib
from ..device import CapturedOp, get_mesh, mass_diagonal
from ..krylov import Recycle, gcro, gmres
from ..operators import ConvectionTensor, SEMOperator
from ..parallel import all_agree
from ..tracing import phase
from ._base import SolverBase
from .convection_diffusion import DirichletRows
from .nested_dissection import NestedDissectionSolver
from .velocity_solve import VelocityJacobianSolver


_ALL_SIDES = _lib.SIDE_W | _lib.SIDE_E | _lib.SIDE_S | _lib.SIDE_N
_NEEDS_ND = ("NavierStokes: velocity_solve_T needs the nested-dissection factor (P >= 2, the whole perimeter Dirichlet, "
             "velocity_interior 'auto' or 'nd'): the line condensation has no transposed solve")


class _SchurVariant(typing.NamedTuple):
    """What distinguishes the pressure-Schur eliminations that NavierStokesSolver._schur_update runs."""
    name: str                       # the Krylov solve in the progress and success messages
    fail: str                       # ... and in the non-convergence error
    solve: typing.Callable          # (bu, bv) -> (xu, xv): the velocity solve, J^-1 or J^-T
    pressure_rhs: typing.Callable   # (fu, fv, c0): the launch that writes what the Schur right-hand side subtracts
    velocity_rhs: typing.Callable   # (p, bu, bv) -> the final velocity solve's right-hand sides (one launch)
    slot: str                       # the attribute that caches the Schur operator ("_schur" / "_schur_T")
    operator: typing.Callable       # () -> the Schur operator
    precond: typing.Callable        # the right preconditioner
    size: int                       # the vector length that sets the restart (_restart)
    krylov: typing.Callable         # gcro or gmres
    kw: typing.Callable             # restart -> the call's further keywords
    progress: bool                  # honour the _progress hook
    clock: bool                     # progress lines carry the elapsed time
    report: bool                    # print the LGMRES_suc line


class NavierStokesSolver(SolverBase):
    _name, _whole_mesh_note = "NavierStokes", " (no transposed strip solve)"
    _partition_adjoint_modes = ("distributed",)

    def __init__(self, L_x: float, L_y: float, Re: float, Gr: float, P: int, N_ex: int, N_ey: int,
                 v_W: float = 0, v_E: float = 0, u_S: float = 0, u_N: float = 0,
                 mtol=1e-7, mtol_newton=1e-5, iprint: list = ['NEWTON_suc', 'NEWTON_iter'],  # noqa: B006
                 max_basis: int = 3000, velocity_interior: str = "auto", velocity_graph: bool = True,
                 recycle_bytes: float = 0.0, velocity_sweep: str = "auto", schur_precond: str = "mass",
                 partition=None, partition_update: str = "distributed", partition_adjoint: bool = False):
        """partition: a sem_amd.parallel.Partition -- the solver then holds one element-column strip per
        rank: _get_residuals / _calc_jacobians / _get_dresiduals run the fused strip launch and sum the
        interface lines of all three outputs with one collective.  partition_update: "distributed"
        (default) -- _get_update runs on the strips: the velocity Jacobian is factored by the
        element-partitioned condensation (strip_solve.StripLineSolver: each rank its own columns, a
        reduced system over the strip-boundary lines shared by all), and the Schur-complement Krylov
        solve runs over the strips (inner products all-reduced); "central" -- rank 0's whole-mesh
        counterpart (_central_solver) solves and the update is broadcast.  The reference methods take
        and return global NumPy vectors (local strips when given device tensors).
        partition_adjoint: opt-in to reverse mode on a partitioned solver.  _get_dresiduals_T then runs on the
        strips (one Mesh.ns_apply_transpose_part launch per rank, one collective for the interface lines).
        _get_update_T is the FUNCTIONAL path, not the scalable one: whatever partition_update says it runs
        centrally -- the linearisation and the right-hand sides are gathered, rank 0's whole-mesh counterpart
        solves, the result is broadcast; a distributed adjoint Schur solve waits for the transposed strip solvers.
        velocity_solve_T and _velocity_apply_lines_T stay whole-mesh only.  Off by default: a partitioned solver
        refuses every reverse-mode method.
        partition_adjoint="distributed": as True, but _get_update_T runs on the strips -- the strip velocity factor
        is built with its transposed solve (nested_dissection.StripNDSolver(adjoint=True); the nested-dissection
        factor only, schur_precond='mass'), velocity_solve_T and _velocity_apply_lines_T work on the strips, and the
        adjoint Schur system S^T q = E^T q - B^T J^-T C^T q is solved over the strips (_StripSchurT) by the GMRES
        with all-reduced inner products: no whole-mesh vector travels and no rank waits for rank 0.
        recycle_bytes: device memory for a recycled Krylov subspace of the Schur-complement solves
        (sem_amd.krylov.Recycle, GCRO; 0 = off, the default): consecutive _get_update calls with one
        linearisation -- the Boussinesq coupler's block-Jacobi preconditioner -- then start from the
        earlier solves' spaces.  Measured (tools/recycle_probe.py, profiles/r02/bous): 5-8x fewer Schur
        matvecs on consistent right-hand sides, but the Arnoldi-relation error of the recycled space
        puts a floor near 1e-8 relative under the residual, above the couplers' mtol_internal = 1e-13,
        so inside the coupler it stagnates; off by default.
        velocity_interior: the velocity-Jacobian factorisation -- "auto" (default): nested dissection of the element
        grid (solvers/nested_dissection.py; on a partitioned solver each strip's own dissection, StripNDSolver) when
        the Dirichlet rows are the whole perimeter (the reference's velocity mask) and P >= 2, else the line
        condensation; "nd": nested dissection; "nested" / "lu" / "inverse": the line condensation
        (solvers/velocity_solve.py, strip_solve.StripLineSolver) with its interior variants.
        schur_precond: right preconditioner of the Schur-complement Krylov solve.  "mass" (default):
        the reference's mass diagonal (NavierStokes_Solver.py:207-212); "pcd": a
        pressure-convection-diffusion approximation S^-1 ~ A_p^-1 F_p M^-1 on the continuity rows,
        A_p^-1 on the pressure rows the reference replaces (boundary K rows, pinned node), where
        A_p = K with the pinned row (factored once per solver by the one-component line
        condensation) and F_p = Sys of the linearisation.  Right preconditioning keeps the stopping
        test on the true Schur residual, so the reference's rule is unchanged; only the Krylov count
        falls (tools/pcd_probe.py).  It is opt-in because on the smallest meshes (4^2, P=4) the
        equal-order Jacobian is singular or nearly so, and which member of the near-null family of
        solutions a Krylov method returns depends on its preconditioner: the reference's golden
        velocities there are reproduced only by the reference's own preconditioner."""
        if schur_precond not in ("mass", "pcd"):
            raise ValueError("schur_precond must be 'mass' or 'pcd'")
        if velocity_interior not in ("auto", "nd", "nested", "lu", "inverse"):
            raise ValueError("velocity_interior must be 'auto', 'nd', 'nested', 'lu' or 'inverse'")
        super().__init__(partition, partition_update, partition_adjoint)
        if partition is not None and schur_precond != "mass" and partition_update == "distributed":
            raise ValueError("the distributed update uses the mass-diagonal Schur preconditioner")
        self._schur_precond, self._Ap = schur_precond, None
        self._iprint = iprint
        self._recycle_bytes, self._schur_recycle = recycle_bytes, None
        self._velocity_interior, self._velocity_graph = velocity_interior, velocity_graph
        self._velocity_sweep = velocity_sweep
        self._max_basis = max_basis
        self._schur_maxiter = None   # cap of a whole-mesh Schur solve's iterations (None: the Krylov default, 10 N)
        self._velo = None
        self._Re, self._Gr = Re, Gr
        if self._Re == 0 and self._Gr != 0:
            raise ValueError('Cannot have Re == 0 and Gr != 0')
        self._Gr_over_Re = self._Gr / self._Re if self._Re != 0 else 0.
        self._mtol, self._mtol_newton = mtol, mtol_newton
        self._L_x, self._L_y = L_x, L_y
        self._P, self._N_ex, self._N_ey = P, N_ex, N_ey
        dx, dy = L_x / N_ex, L_y / N_ey
        self.points = SEM.global_nodes(P, N_ex, N_ey, L_x / N_ex, L_y / N_ey)
        self.points_e = SEM.element_nodes(P, N_ex, N_ey, dx, dy)
        self.N = (N_ex * P + 1) * (N_ey * P + 1)
        self._args = dict(L_x=L_x, L_y=L_y, Re=Re, Gr=Gr, P=P, N_ex=N_ex, N_ey=N_ey, v_W=v_W, v_E=v_E, u_S=u_S,
                          u_N=u_N, mtol=mtol, mtol_newton=mtol_newton, iprint=iprint, max_basis=max_basis,
                          velocity_interior=velocity_interior, velocity_graph=velocity_graph,
                          recycle_bytes=recycle_bytes, velocity_sweep=velocity_sweep, schur_precond=schur_precond)
        self._lin_sys = None
        if partition is None:
            self._mesh = m = get_mesh(P, N_ex, N_ey, dx, dy)
            self._M = SEM.global_mass_matrix(P, N_ex, N_ey, dx, dy)
            self._K = SEM.global_stiffness_matrix(P, N_ex, N_ey, dx, dy)
            self._C_x, self._C_y = SEM.global_convection_matrices(P, N_ex, N_ey, dx, dy)
        else:   # matrix-free operators on this rank's strip
            self._mesh = m = partition.setup(P, N_ex, N_ey, dx, dy)
            self._M, self._K = SEMOperator(m, cM=1.0), SEMOperator(m, cK=1.0)
            self._C_x, self._C_y = ConvectionTensor(m, "x"), ConvectionTensor(m, "y")
        self._Sys = None
        self._Jac_u_u = self._Jac_u_v = self._Jac_v_u = self._Jac_v_v = None
        self._jac_kw, self._schur, self._schur_T = None, None, None

        # Dirichlet values and masks, exactly as NavierStokes_Solver.py:78-94 builds them
        x, y = self.points
        du, dv, dpp = np.full(self.N, np.nan), np.full(self.N, np.nan), np.full(self.N, np.nan)
        dv[np.isclose(x, 0)] = v_W
        du[np.isclose(x, 0)] = 0
        dv[np.isclose(x, self._L_x)] = v_E
        du[np.isclose(x, self._L_x)] = 0
        du[np.isclose(y, 0)] = u_S
        dv[np.isclose(y, 0)] = 0
        du[np.isclose(y, self._L_y)] = u_N
        dv[np.isclose(y, self._L_y)] = 0
        dpp[int(self.N / 2)] = 0
        self._dirichlet_u, self._dirichlet_v, self._dirichlet_p = du, dv, dpp
        self._mask_bound = ~np.isnan(du)
        self._mask_dir_p = ~np.isnan(dpp)
        all_sides = _lib.SIDE_W | _lib.SIDE_E | _lib.SIDE_S | _lib.SIDE_N
        self._dir = DirichletRows(m, self._mask_bound, all_sides)
        self._dval_u = self._dev(np.where(self._mask_bound, du, 0.0))
        self._dval_v = self._dev(np.where(self._mask_bound, dv, 0.0))
        pins = np.nonzero(self._mask_dir_p)[0]
        if len(pins) > 1:
            raise ValueError("one pinned pressure node is supported")
        self._pin = int(pins[0]) if len(pins) else -1
        self._pin_val = float(dpp[self._pin]) if len(pins) else 0.0
        if partition is not None:
            # the reference's mass diagonal (NavierStokes_Solver.py:207-212) is the assembled one: on a
            # shared line both strips hold the whole-mesh value
            self._Mdiag = m.to_device(partition.local(mass_diagonal(P, N_ex, N_ey, dx, dy)))
            self._pin_local = self._pin - m.dof_begin if 0 <= self._pin - m.dof_begin < m.n_local else -1
            return
        self._pin_local = self._pin
        self._Mdiag = m.to_device(self._M.diagonal())
        # PCD row weights: 1/M on the continuity rows, 0 on the replaced rows (and the reverse)
        repl = self._mask_bound.copy()
        if self._pin >= 0:
            repl[self._pin] = True
        self._pcd_w = m.to_device(np.where(repl, 0.0, 1.0 / self._M.diagonal()))
        self._pcd_b = m.to_device(repl.astype(np.float64))

    # ------------------------------------------------------------------ helpers
    def _norm(self, *ys):
        if self._part is not None:
            return self._part.norm(*ys)
        return torch.sqrt(sum(y.square().sum() for y in ys)).item()

    def _amax(self, *ys):
        if self._part is not None:
            return self._part.amax(*ys)
        return max(y.abs().max().item() for y in ys)

    def _grad(self, x, which):
        """G_x x or G_y x, assembled across strips on a partitioned solver."""
        if self._part is None:
            return self._mesh.apply(x, **{which: 1.0})
        return self._part.step(x, **{which: 1.0})

    def _ns_kw(self, pin_first):
        """Row replacements of sem_ns_apply: Dirichlet rows (mask_bound) and the pinned-pressure row."""
        return dict(pin=self._pin, pin_val=0.0 if not pin_first else self._pin_val, pin_first=pin_first,
                    **self._dir.kw())

    # ------------------------------------------------------------------ reference methods
    def _get_residuals(self, u, v, p, T):
        """NavierStokes_Solver.py:93-121: one fused launch (sem_ns_apply) for res_u, res_v, res_cont."""
        m = self._mesh
        U, V, Pp, Tt = self._dev(u), self._dev(v), self._dev(p), self._dev(T)
        Conv = self._Re * (SEM.tensordot(self._C_x, U, (1, 0)) + SEM.tensordot(self._C_y, V, (1, 0)))
        self._Sys = self._K + Conv
        if self._schur_recycle is not None:   # the Schur operator depends on Sys
            self._schur_recycle.reset()
        ru, rv, rc = (torch.empty_like(U) for _ in range(3))
        m.ns_apply(U, V, Pp, ru, rv, rc, **self._sys_kw(), c_T=-self._Gr_over_Re, T=Tt,
                   dval_u=self._dval_u, dval_v=self._dval_v, **self._ns_kw(pin_first=True))
        if self._part is not None:
            self._part.assemble(ru, rv, rc)
            self._lin_sys = (U, V)   # Sys's velocity: part of the next linearisation
        return self._out(ru, u), self._out(rv, u), self._out(rc, u)

    def _calc_jacobians(self, u, v):
        """NavierStokes_Solver.py:123-136.  The Jacobians keep the Sys of this linearisation, as the
        reference's J_uu = Sys + ... does, even if _get_residuals runs again before they are used."""
        U, V = self._dev(u), self._dev(v)
        Re = self._Re
        if self._part is None:
            self._Jac_u_u = self._Sys + Re * SEM.tensordot(self._C_x, U, (2, 0))
            self._Jac_v_v = self._Sys + Re * SEM.tensordot(self._C_y, V, (2, 0))
            self._Jac_u_v = Re * SEM.tensordot(self._C_y, U, (2, 0))
            self._Jac_v_u = Re * SEM.tensordot(self._C_x, V, (2, 0))
        else:   # G u on a strip needs the interface exchange before it becomes a diagonal
            m = self._mesh
            self._Jac_u_u = self._Sys + SEMOperator(m, dg=[(Re, self._grad(U, "c_gradx"))])
            self._Jac_v_v = self._Sys + SEMOperator(m, dg=[(Re, self._grad(V, "c_grady"))])
            self._Jac_u_v = SEMOperator(m, dg=[(Re, self._grad(U, "c_grady"))])
            self._Jac_v_u = SEMOperator(m, dg=[(Re, self._grad(V, "c_gradx"))])
            self._twin_lin, self._twin_stale = self._lin_sys + (U, V), True
        self._jac_kw = dict(self._sys_kw(), juu=self._Jac_u_u._coeffs()[4], jvv=self._Jac_v_v._coeffs()[4],
                            juv=self._Jac_u_v._coeffs()[4], jvu=self._Jac_v_u._coeffs()[4])
        self._velo = None  # factorised on first use, reused until the next linearisation
        self._schur = self._schur_T = None
        if self._schur_recycle is not None:
            self._schur_recycle.reset()

    def _get_dresiduals(self, du, dv, dp, dT=None):
        """NavierStokes_Solver.py:138-160: one fused launch (sem_ns_apply) for the three differentials."""
        m = self._mesh
        DU, DV, DP = self._dev(du), self._dev(dv), self._dev(dp)
        ru, rv, rc = (torch.empty_like(DU) for _ in range(3))
        m.ns_apply(DU, DV, DP, ru, rv, rc, **self._jac_kw, c_T=-self._Gr_over_Re if dT is not None else 0.0,
                   T=self._dev(dT), **self._ns_kw(pin_first=False))
        if self._part is not None:
            self._part.assemble(ru, rv, rc)
        return self._out(ru, du), self._out(rv, du), self._out(rc, du)

    def _central_solver(self):
        """Rank 0's whole-mesh counterpart that runs the partitioned solver's updates (same arguments,
        no partition)."""
        return NavierStokesSolver(**self._args)

    def _twin_refresh(self, twin, us, vs, uj, vj):
        """The gathered linearisation through the reference interface: _get_residuals sets Sys (the residual's
        u, v), _calc_jacobians the Jacobians."""
        z = np.zeros(self.N)
        twin._get_residuals(us, vs, z, z)
        twin._calc_jacobians(uj, vj)

    def _get_update_partitioned(self, dres_u, dres_v, dres_cont, du0, dv0, dp0):
        """Whole-mesh update for a strip-partitioned solver (SolverBase._central): the linearisation and the
        right-hand sides are gathered, rank 0's whole-mesh counterpart runs _get_update, the update is broadcast."""
        if self._twin_lin is None:
            raise RuntimeError("NavierStokes: _calc_jacobians must run before _get_update")
        return self._central(self._twin_refresh,
                             lambda twin, ru, rv, rc, u0, v0, p0: twin._get_update(ru, rv, rc, du0=u0, dv0=v0, dp0=p0),
                             (dres_u, dres_v, dres_cont, du0, dv0, dp0), 3, "schur_matvecs", "the update")

    def _get_update_T_partitioned(self, du_bar, dv_bar, dp_bar, dres_c0):
        """_get_update_T of a strip-partitioned solver, run centrally whatever partition_update says (the mirror of
        _get_update_partitioned on the same cached twin and the same staleness record).  This is the functional
        path, not the scalable one: every call moves whole-mesh vectors through rank 0.  A distributed adjoint Schur
        solve S^T q = E^T q - B^T J^-T C^T q needs the transposed strip solvers, which do not exist yet."""
        if self._twin_lin is None:
            raise RuntimeError("NavierStokes: _get_residuals and _calc_jacobians must run before _get_update_T")
        return self._central(self._twin_refresh,
                             lambda twin, bu, bv, bp, q0: twin._get_update_T(bu, bv, bp, dres_c0=q0),
                             (du_bar, dv_bar, dp_bar, dres_c0), 3, "schur_matvecs", "the adjoint update")

    def _dist_adjoint(self):
        """True on a partitioned solver built with partition_adjoint='distributed'."""
        return self._part is not None and self._partition_adjoint_mode == "distributed"

    def _use_nd(self):
        """Nested dissection (velocity_interior "auto" / "nd") needs P >= 2 and the whole perimeter Dirichlet."""
        ok = self._P >= 2 and self._dir.mask is None and self._dir.sides == _ALL_SIDES
        if self._velocity_interior == "nd" and not ok:
            raise ValueError("velocity_interior='nd' needs P >= 2 and the whole perimeter Dirichlet")
        return ok and self._velocity_interior in ("auto", "nd")

    def _strip_velocity_solver(self):
        """The element-partitioned velocity factor of this linearisation on this rank's strip handle
        (nested_dissection.StripNDSolver, or strip_solve.StripLineSolver for other Dirichlet sets), kept until
        _calc_jacobians runs again."""
        if self._velo is not None:
            return self._velo
        from .nested_dissection import StripNDSolver
        from .strip_solve import StripLineSolver
        tStart = time.perf_counter()
        m, p = self._mesh, self._part
        # every rank takes the same choice: the Dirichlet set and the option are global
        cls = StripNDSolver if self._use_nd() else StripLineSolver
        # the distributed adjoint update needs the factor's transposed solve (the forward factor is the same)
        extra = dict(adjoint=True) if cls is StripNDSolver and self._dist_adjoint() else {}
        vs = cls(self._P, self._N_ex, self._N_ey, m.device, p.part.bounds, p.rank, p.dist, group=p.group,
                 gather_device=p.backend_device(), **extra)
        vs.factor_mesh(m, dir_mask=self._dir.mask, dir_sides=self._dir.sides, **self._jac_kw)
        vs.set_operator(self._velocity_apply_lines, amax=lambda t: p.amax(t))
        vs.check_refinement()       # every rank takes the same decision (norms max-reduced over the ranks)
        self._velo = vs
        if 'LU_suc' in self._iprint:
            print(f'NavierStokes LU: Succeeded in {time.perf_counter()-tStart:0.2f}sec (element-partitioned)')
        return vs

    def _schur_strips(self, vs, dp):
        """S dp on the strips (NavierStokes_Solver.py:194-203): the gradients of dp (interface lines summed
        across strips), the partitioned velocity solve, the divergence (summed)."""
        m, part, NY = self._mesh, self._part, self._mesh.NY
        kw = self._ns_kw(pin_first=False)
        gu, gv = torch.empty_like(dp), torch.empty_like(dp)
        with phase("schur.grad_apply"):
            m.ns_apply(None, None, dp, gu, gv, **kw)
        with phase("schur.grad_assemble"):
            part.assemble(gu, gv)
        with phase("schur.velocity_solve"):
            X = vs._solve_lines(torch.stack((gu.view(-1, NY), gv.view(-1, NY)), dim=1).reshape(-1, 2 * NY))
        rc = torch.empty_like(dp)
        with phase("schur.div_apply"):
            m.ns_apply(X[:, :NY].reshape(-1), X[:, NY:].reshape(-1), dp, rc=rc, c_div=-1.0, **kw)
        with phase("schur.div_assemble"):
            part.assemble(rc)
        return rc

    def _get_update_strips(self, dres_u, dres_v, dres_cont, du0=None, dv0=None, dp0=None):
        """_get_update (NavierStokes_Solver.py:162-236) on the strips: the element-partitioned velocity
        solve inside the Schur-complement GMRES, whose inner products are all-reduced (a shared line
        counted once); the reference's mass-diagonal preconditioner and stopping rule."""
        return self._schur_update(self._forward_variant(), (dres_u, dres_v, dres_cont), dp0)

    def _velocity_solver(self):
        """Device factorisation of the Dirichlet-row-replaced velocity Jacobian -- the reference's
        `bmat` + `splu` (NavierStokes_Solver.py:176-184) -- by static condensation over node lines
        (sem_amd/solvers/velocity_solve.py).  The reference refactorises on every _get_update call;
        the factor depends only on the Jacobians, so it is kept until _calc_jacobians runs again (the
        Boussinesq coupler's block-Jacobi preconditioner calls _get_update once per Krylov iteration)."""
        if self._velo is not None:
            return self._velo
        tStart = time.perf_counter()
        m = self._mesh
        if self.N > 1_000_000:   # the previous linearisation's factor and graphs go before the next one
            gc.collect()
            torch.cuda.empty_cache()
        interior = self._velocity_interior
        if self._use_nd():
            # nested dissection of the element grid (solvers/nested_dissection.py): cfg5 3.0 ms per solve with the
            # split leaves against the line condensation's 7.8 ms, cfg4 0.34 against 0.56 ms (profiles/r06/velocity/)
            vs = NestedDissectionSolver(self._P, self._N_ex, self._N_ey, m.device)
        else:
            vs = VelocityJacobianSolver(self._P, self._N_ex, self._N_ey, m.device,
                                        interior="nested" if interior == "auto" else interior, sweep=self._velocity_sweep)
        vs.factor_mesh(m, dir_mask=self._dir.mask, dir_sides=self._dir.sides, **self._jac_kw)
        vs.set_operator(self._velocity_apply_lines)
        vs.check_refinement()       # one refinement step per solve if the factor's backward error exceeds 1e-13
        if self._velocity_graph:
            vs.capture()
        self._velo = vs
        if 'LU_suc' in self._iprint:
            torch.cuda.synchronize(m.device)
            kind = ("nested dissection" + (", split leaves" if vs.split else ", A_ii^-1 leaves")
                    if vs.interior == "nd" else "device static condensation")
            print(f'NavierStokes LU: Succeeded in {time.perf_counter()-tStart:0.2f}sec ({kind}, '
                  f'backward error {vs.refine_eta:.1e}{", refined" if vs.refine else ""})')
        return vs

    def _velocity_apply_lines(self, X):
        """J X for the velocity Jacobian of this linearisation on (NX, 2 NY) line arrays: the velocity rows of
        _get_dresiduals at dp = 0 (NavierStokes_Solver.py:138-160; Dirichlet rows identity, as the factored
        Jacobian's), assembled across strips on a partitioned solver.  The refinement step's operator."""
        m, NY = self._mesh, self._mesh.NY
        kw = dict(self._jac_kw, **self._ns_kw(pin_first=False))
        if self._part is None:
            Y = torch.empty_like(X)
            m.ns_apply(X[:, :NY], X[:, NY:], None, Y[:, :NY], Y[:, NY:], None, **kw)
            return Y
        xu, xv = X[:, :NY].reshape(-1), X[:, NY:].reshape(-1)
        ru, rv = torch.empty_like(xu), torch.empty_like(xv)
        m.ns_apply(xu, xv, None, ru, rv, None, **kw)
        self._part.assemble(ru, rv)
        return torch.stack((ru.view(-1, NY), rv.view(-1, NY)), dim=1).reshape(-1, 2 * NY)

    def _velocity_apply_lines_T(self, X):
        """J_D^T X for the velocity Jacobian of this linearisation on (NX, 2 NY) line arrays (the transpose of
        _velocity_apply_lines' operator): with z' = (1 - m) z (m the Dirichlet mask),
            u block: (Sys + diag(juu))_D^T z_u + jvu z'_v,    v block: (Sys + diag(jvv))_D^T z_v + juv z'_u
        -- two fused transposed launches (sem_apply_transpose, identity Dirichlet rows), the cross terms pre-loaded
        into the outputs and added through c_acc = 1.  The operator of check_refinement_T and of the transposed
        velocity solve's refinement step.  sem_apply_transpose refuses what it does not support.
        On the strips (partition_adjoint='distributed'; X this strip's lines, equal on shared lines): ONE
        sem_ns_apply_transpose_part launch on line views of X and of the result -- the velocity block of the strip's
        own A_s^T at z_c = 0, which is the same operator: the Dirichlet rows of [J C] are identity rows, so
        (A^T [z_u; z_v; 0])_{u,v} = J_D^T z, cross terms included -- and the interface lines of the line buffer
        summed across the strips (Partition.assemble_lines).  Otherwise whole mesh only."""
        if self._dist_adjoint():
            m, NY = self._mesh, self._mesh.NY
            Y = torch.empty_like(X)
            m.ns_apply_transpose_part(X[:, :NY], X[:, NY:], None, Y[:, :NY], Y[:, NY:], None, **self._jac_kw,
                                      **self._ns_kw(pin_first=False))
            return self._part.assemble_lines(Y)
        self._whole_mesh_only("_velocity_apply_lines_T")
        m, NY = self._mesh, self._mesh.NY
        kw = self._jac_kw
        sys = {k: kw[k] for k in ("c_stiff", "c_mass", "c_gradx", "cu", "c_grady", "cv")}
        free = self._free_rows()
        zu, zv = X[:, :NY].reshape(-1).contiguous(), X[:, NY:].reshape(-1).contiguous()
        yu, yv = kw["jvu"] * (free * zv), kw["juv"] * (free * zu)
        m.apply_transpose(zu, yu, diag=kw["juu"], c_acc=1.0, dir_mode=_lib.DIR_IDENTITY, **sys, **self._dir.kw())
        m.apply_transpose(zv, yv, diag=kw["jvv"], c_acc=1.0, dir_mode=_lib.DIR_IDENTITY, **sys, **self._dir.kw())
        return torch.stack((yu.view(-1, NY), yv.view(-1, NY)), dim=1).reshape(-1, 2 * NY)

    def velocity_solve_T(self, bu, bv):
        """(J^-T [bu; bv]) split as (xu, xv) from the cached nested-dissection factor of _velocity_solver() -- the
        inner solve of a transposed Schur matvec S_p^T = G^T J^-T D^T.  The first call after a linearisation
        registers _velocity_apply_lines_T, runs check_refinement_T and, with velocity_graph, captures the transposed
        solve.  NumPy in, NumPy out; device tensors in, device tensors out.  Solvers whose factor is nested dissection
        only (there is no transposed line condensation): whole-mesh ones, and partitioned ones built with
        partition_adjoint='distributed' -- the transposed strip solve (StripNDSolver(adjoint=True)): local tensors
        in (equal on shared lines), local tensors out; global NumPy in, gathered NumPy out."""
        if self._dist_adjoint():
            vs = self._strip_velocity_solver_T()
        else:
            self._whole_mesh_only("velocity_solve_T")
            vs = self._velocity_solver_T()
        xu, xv = vs.solve_T(self._dev(bu), self._dev(bv))
        return self._out(xu, bu), self._out(xv, bu)

    def _strip_velocity_solver_T(self):
        """_velocity_solver_T's twin on the strips: _strip_velocity_solver()'s factor made ready for transposed
        solves (the transposed operator registered, check_refinement_T -- every rank the same decision, the norms
        max-reduced --, capture_T attempted: declined while the collectives go through the host).  The same
        ValueError for a factor that is not nested dissection."""
        from .nested_dissection import StripNDSolver
        if self._jac_kw is None:
            raise RuntimeError("NavierStokes: _get_residuals and _calc_jacobians must run before the transposed "
                               "velocity solve")
        if not self._use_nd():
            raise ValueError(_NEEDS_ND)
        vs = self._strip_velocity_solver()
        if not isinstance(vs, StripNDSolver):
            raise ValueError(_NEEDS_ND)
        return self._ready_T(vs, amax=self._part.amax)

    def _velocity_solver_T(self):
        """_velocity_solver()'s factor made ready for transposed solves: the first call after a linearisation
        registers _velocity_apply_lines_T, runs check_refinement_T and, with velocity_graph, captures the transposed
        solve.  ValueError for a factor that is not nested dissection."""
        vs = self._velocity_solver()
        if not isinstance(vs, NestedDissectionSolver):
            raise ValueError(_NEEDS_ND)
        return self._ready_T(vs)

    def _ready_T(self, vs, amax=None):
        """The first call after a linearisation registers the transposed operator on the velocity factor vs (amax:
        set_operator's, the strips' reduced max norm), runs check_refinement_T and, with velocity_graph, attempts
        capture_T; returns vs."""
        if vs._apply_T is None:
            vs.set_operator(self._velocity_apply_lines, amax=amax, apply_lines_T=self._velocity_apply_lines_T)
            vs.check_refinement_T()
            if self._velocity_graph:
                vs.capture_T()
        return vs

    def _pressure_laplacian(self):
        """A_p = K with the pinned pressure row as an identity row (the Neumann pressure Laplacian
        made regular), factored once per solver by the one-component line condensation."""
        if self._Ap is None:
            m = self._mesh
            vs = VelocityJacobianSolver(self._P, self._N_ex, self._N_ey, m.device, ncomp=1)
            mask = torch.zeros(m.n_local, dtype=torch.uint8, device=m.device)
            mask[self._pin if self._pin >= 0 else self.N // 2] = 1
            vs.factor_mesh(m, c_stiff=1.0, dir_mask=mask)
            if self._velocity_graph and m.device.type == "cuda":
                vs.capture()
            self._Ap = vs
        return self._Ap

    def _pcd(self, c):
        """z = A_p^-1 (F_p (w c) + b c): w = 1/M on continuity rows (0 elsewhere), b = 1 on the
        replaced rows (boundary K rows and the pin), F_p = Sys of this linearisation."""
        y = self._mesh.apply(c * self._pcd_w, **{k: self._jac_kw[k] for k in ("c_stiff", "c_mass", "c_gradx", "cu",
                                                                              "c_grady", "cv")},
                             c_extra=1.0, ea=c, eb=self._pcd_b)
        return self._pressure_laplacian().solve1(y)

    def _mass_precond(self, c):
        """The reference's Schur preconditioner (NavierStokes_Solver.py:207-212): the inverse mass diagonal, the
        identity on the pinned row (when this rank holds it).  Diagonal, so it preconditions S and S^T alike."""
        z = c / self._Mdiag
        if self._pin_local >= 0:
            z[self._pin_local] = c[self._pin_local]
        return z

    def _restart(self, size):
        """The basis and its preconditioned images (2 restart N doubles = 16 N bytes per vector) within 32 GB:
        unrestarted up to max_basis on cfg3/cfg4, restarted at 846 vectors on a whole-mesh cfg5 solver (N = 1537^2 =
        2.36 M; 31.9 GB).  The velocity factor, the Schur graph's buffers and the Hessenberg matrix come on top of
        this budget.  Twice that (V only, as krylov.gmres keeps no M^-1 V for the linear mass-diagonal
        preconditioner) measured no faster at cfg5 -- fewer iterations in the long first solves, each dearer
        (profiles/r04/cfg5/cfg5_restart1694.json).  On the strips `size` is the largest strip and N the global
        count, sizes every rank shares: the ranks run the same Arnoldi iterations and so call the same collectives."""
        return max(1, min(self.N, self._max_basis, int(32e9 // (16 * size))))

    def _recycle(self, restart):
        if self._recycle_bytes and self._schur_recycle is None:
            cap = min(self.N, max(restart + 1, int(self._recycle_bytes // (16 * self.N))))
            self._schur_recycle = Recycle(self.N, torch.float64, self._mesh.device, cap)
        return self._schur_recycle

    def _forward_variant(self):
        """_schur_update's record for _get_update: on the whole mesh GCRO (recycling when asked for) over the
        captured _SchurComplement under either preconditioner; on the strips the GMRES with all-reduced inner
        products over _StripSchur, every launch followed by the interface assembly."""
        m, part, kw = self._mesh, self._part, self._ns_kw(pin_first=False)
        assemble = part.assemble if part is not None else (lambda *ys: None)

        def pressure_rhs(fu, fv, c0):    # dres_cont(J^-1 [ru; rv], 0)
            m.ns_apply(fu, fv, None, rc=c0, **kw)
            assemble(c0)

        def velocity_rhs(dp, ru, rv):
            b_u, b_v = torch.empty_like(dp), torch.empty_like(dp)
            m.ns_apply(None, None, dp, b_u, b_v, **kw)
            assemble(b_u, b_v)
            return ru - b_u, rv - b_v

        if part is not None:
            vs = self._strip_velocity_solver()
            return _SchurVariant("GMRES", "LGMRES", vs.solve, pressure_rhs, velocity_rhs, "_schur",
                                 lambda: _StripSchur(self, vs, graph=self._velocity_graph), self._mass_precond,
                                 part.max_local_dofs(), gmres,
                                 lambda restart: dict(maxiter=10 * self.N, inner=part.inner),
                                 progress=True, clock=True, report=False)
        vs = self._velocity_solver()
        return _SchurVariant("GMRES", "LGMRES", vs.solve, pressure_rhs, velocity_rhs, "_schur",
                             lambda: _SchurComplement(self, vs, graph=self._velocity_graph),
                             self._pcd if self._schur_precond == "pcd" else self._mass_precond, self.N, gcro,
                             lambda restart: dict(maxiter=self._schur_maxiter, recycle=self._recycle(restart)),
                             progress=True, clock=False, report=True)

    def _adjoint_variant(self):
        """_schur_update's record for _get_update_T: the transposed solves and launches, plain GMRES over
        _SchurComplementT, no recycling; on the strips (partition_adjoint='distributed') the strip's own transposed
        launches (sem_ns_apply_transpose_part) each followed by the interface assembly, the transposed strip solve,
        and the GMRES with all-reduced inner products over _StripSchurT, sized as the forward strip variant."""
        m, part, kw = self._mesh, self._part, self._ns_kw(pin_first=False)
        if part is not None:
            vs = self._strip_velocity_solver_T()

            def strip_pressure_rhs(fu, fv, c0):    # B^T f
                m.ns_apply_transpose_part(fu, fv, None, yp=c0, **kw)
                part.assemble(c0)

            def strip_velocity_rhs(q, bu, bv):     # [bu; bv] - C^T q
                gu, gv = torch.empty_like(q), torch.empty_like(q)
                m.ns_apply_transpose_part(None, None, q, gu, gv, c_div=-1.0, **kw)
                part.assemble(gu, gv)
                return bu + gu, bv + gv

            return _SchurVariant("adjoint GMRES", "adjoint GMRES", vs.solve_T, strip_pressure_rhs, strip_velocity_rhs,
                                 "_schur_T", lambda: _StripSchurT(self, vs, graph=self._velocity_graph),
                                 self._mass_precond, part.max_local_dofs(), gmres,
                                 lambda restart: dict(maxiter=10 * self.N, inner=part.inner),
                                 progress=False, clock=False, report=False)
        vs = self._velocity_solver_T()

        def pressure_rhs(fu, fv, c0):    # B^T f
            m.ns_apply_transpose(fu, fv, None, yp=c0, **kw)

        def velocity_rhs(q, bu, bv):     # [bu; bv] - C^T q
            gu, gv = torch.empty_like(q), torch.empty_like(q)
            m.ns_apply_transpose(None, None, q, gu, gv, c_div=-1.0, **kw)
            return bu + gu, bv + gv

        return _SchurVariant("adjoint GMRES", "adjoint GMRES", vs.solve_T, pressure_rhs, velocity_rhs, "_schur_T",
                             lambda: _SchurComplementT(self, vs, graph=self._velocity_graph), self._mass_precond,
                             self.N, gmres, lambda restart: dict(maxiter=self._schur_maxiter),
                             progress=False, clock=False, report=True)

    def _schur_update(self, var, rhs, x0):
        """The block elimination of _get_update and _get_update_T, once: with the variant's velocity solve J^-1 (or
        J^-T), launches and Schur operator S (or S^T),
            f = J^-1 [ru; rv],   S dp = rc - (pressure rows of f),   [du; dv] = J^-1 (velocity_rhs(dp, ru, rv)),
        the Schur system by the variant's Krylov function under its right preconditioner with the reference's
        stopping rule ||r||_2 <= mtol sqrt(N) (NavierStokes_Solver.py:222-224).  The Schur operator is built on
        first use and kept in the variant's slot until _calc_jacobians runs again."""
        ru, rv, rc = (self._dev(a) for a in rhs)
        fu, fv = var.solve(ru, rv)
        c0 = torch.empty_like(rc)
        var.pressure_rhs(fu, fv, c0)
        b_schur = rc - c0
        if getattr(self, var.slot) is None:
            setattr(self, var.slot, var.operator())
        count, it = [0], [0]

        def schur_mv(dp):
            count[0] += 1
            return getattr(self, var.slot)(dp)

        prog = self._progress if var.progress else 0
        t_start = time.perf_counter()

        def cb(est):
            it[0] += 1
            if 'LGMRES_iter' in self._iprint or (prog and it[0] % prog == 0):
                took = f'\t{time.perf_counter() - t_start:.1f}s' if var.clock else ''
                print(f'NavierStokes {var.name}: {it[0]}\t{est}{took}', flush=True)

        restart = self._restart(var.size)
        r = var.krylov(schur_mv, b_schur, x0=self._dev(x0), atol=self._mtol * np.sqrt(self.N), rtol=0.0,
                       restart=restart, precond=var.precond, callback=cb, **var.kw(restart))
        if r.info != 0:
            raise RuntimeError(f'NavierStokes {var.fail}: Failed to converge in {r.info} iterations')
        dp = r.x
        self.schur_matvecs = count[0] - r.discarded     # a dropped speculative matvec is not counted
        self.schur_discarded = r.discarded
        if var.report and 'LGMRES_suc' in self._iprint:
            res = (schur_mv(dp) - b_schur).abs().max().item()
            print(f'NavierStokes {var.name}: Converged in {self.schur_matvecs} evaluations with max-norm {res}')
        du, dv = var.solve(*var.velocity_rhs(dp, ru, rv))
        return self._out(du, rhs[0]), self._out(dv, rhs[0]), self._out(dp, rhs[0])

    def _get_update(self, dres_u, dres_v, dres_cont, du0=None, dv0=None, dp0=None):
        """Velocity solve + pressure Schur-complement Krylov solve (NavierStokes_Solver.py:162-236), on
        the device: the velocity Jacobian is factored once per linearisation (_velocity_solver) and the
        Schur system is solved by the device GMRES (sem_amd/krylov.py) with the reference's
        mass-diagonal preconditioner (:208-212) and stopping rule ||r||_2 <= mtol sqrt(N) (:222-224).
        The reference's inner_m = 0.3 N is "not a realistic inner_m" (:224): its LGMRES runs as an
        unrestarted GMRES with outer augmentation.  A plain GMRES restarted at 0.3 N stagnates on small
        meshes (the Schur complement carries the spurious pressure modes of the equal-order
        discretisation), so the device GMRES runs unrestarted up to max_basis vectors."""
        if self._part is not None and self._partition_update == "central":
            return self._get_update_partitioned(dres_u, dres_v, dres_cont, du0, dv0, dp0)
        return self._schur_update(self._forward_variant(), (dres_u, dres_v, dres_cont), dp0)

    # ------------------------------------------------------------------ reverse mode
    def _get_dresiduals_T(self, ru_bar, rv_bar, rc_bar, want_T=False):
        """Transpose of _get_dresiduals(du, dv, dp, dT): (du_bar, dv_bar, dp_bar) = A^T (ru_bar, rv_bar, rc_bar) for
        the operator A of _get_dresiduals at dT = 0, and with want_T also dT_bar = -(Gr/Re) M (1 - m) rv_bar, so that
        <_get_dresiduals(d), w> = <d, _get_dresiduals_T(w)> -- one fused launch (sem_ns_apply_transpose).  NumPy in,
        NumPy out; device tensors in, device tensors out.  Needs _calc_jacobians, like the forward method.
        On a partitioned solver (partition_adjoint=True): each rank's transposed strip launch
        (sem_ns_apply_transpose_part) and one collective that sums the interface lines of all outputs; with shared
        lines counted once the inner-product identity holds.  Global NumPy in, gathered NumPy out; local tensors in
        (equal on shared lines), local tensors out."""
        self._whole_mesh_only("_get_dresiduals_T", adjoint=True)
        if self._jac_kw is None:
            raise RuntimeError("NavierStokes: _get_residuals and _calc_jacobians must run before _get_dresiduals_T")
        m = self._mesh
        zu, zv, zc = self._dev(ru_bar), self._dev(rv_bar), self._dev(rc_bar)
        yu, yv, yp = (torch.empty_like(zu) for _ in range(3))
        yT = torch.empty_like(zu) if want_T else None
        launch = m.ns_apply_transpose if self._part is None else m.ns_apply_transpose_part
        launch(zu, zv, zc, yu, yv, yp, yT, **self._jac_kw, c_T=-self._Gr_over_Re if want_T else 0.0,
               **self._ns_kw(pin_first=False))
        out = (yu, yv, yp) + ((yT,) if want_T else ())
        if self._part is not None:
            self._part.assemble(*out)
        return tuple(self._out(y, ru_bar) for y in out)

    def _get_update_T(self, du_bar, dv_bar, dp_bar, dres_c0=None):
        """Adjoint of _get_update: (lam_u, lam_v, lam_c) with A^T lam = (du_bar, dv_bar, dp_bar), by the block
        elimination of the forward update transposed:
            f = J^-T [du_bar; dv_bar],   S^T q = dp_bar - B^T f,   [lam_u; lam_v] = J^-T ([du_bar; dv_bar] - C^T q),
        lam_c = q, with S^T = E^T - B^T J^-T C^T (_SchurComplementT) solved by the device GMRES under the forward
        update's mass-diagonal right preconditioner, stopping rule (||r||_2 <= mtol sqrt(N)) and restart; dres_c0 is
        the initial guess of q.  No recycling.  Whole-mesh solvers with the nested-dissection factor and
        schur_precond='mass' only: PCD's A_p^-T would need a transposed line condensation, which does not exist.
        On a partitioned solver with partition_adjoint=True the solve runs centrally (_get_update_T_partitioned): the
        functional path, not the scalable one.  With partition_adjoint='distributed' it runs on the strips: the same
        elimination with the transposed strip solve (StripNDSolver(adjoint=True)) and _StripSchurT, the same
        preconditioner (the pinned row on the rank that holds it), stopping rule and restart sizing as the forward
        strip update; global NumPy in, gathered NumPy out; local tensors in, local tensors out."""
        self._whole_mesh_only("_get_update_T", adjoint=True)
        if self._part is not None and not self._dist_adjoint():
            return self._get_update_T_partitioned(du_bar, dv_bar, dp_bar, dres_c0)
        if self._schur_precond == "pcd":
            raise ValueError("NavierStokes: _get_update_T needs schur_precond='mass': the PCD preconditioner's A_p^-T "
                             "would need a transposed line condensation")
        if self._jac_kw is None:
            raise RuntimeError("NavierStokes: _get_residuals and _calc_jacobians must run before _get_update_T")
        return self._schur_update(self._adjoint_variant(), (du_bar, dv_bar, dp_bar), dres_c0)

    def _get_solution(self, T, u0=None, v0=None, p0=None):
        """Newton iteration (NavierStokes_Solver.py:238-270), iterates kept on the device; NumPy in,
        NumPy out (device tensors in, device tensors out)."""
        like = T
        Z = torch.zeros(self._mesh.n_local, dtype=torch.float64, device=self._mesh.device)
        u = self._dev(u0) if u0 is not None else Z.clone()
        v = self._dev(v0) if v0 is not None else Z.clone()
        p = self._dev(p0) if p0 is not None else Z.clone()
        T = self._dev(T)
        self._k = 0
        self.newton_history = []
        while True:
            res_u, res_v, res_cont = self._get_residuals(u, v, p, T)
            norm = self._norm(res_u, res_v, res_cont)
            if 'NEWTON_iter' in self._iprint:
                print(f'NavierStokes NEWTON: {self._k}\t{norm}')
            if norm <= self._mtol_newton * np.sqrt(self.N * 3):
                self.newton_history.append((norm, 0))
                if 'NEWTON_suc' in self._iprint:
                    mx = self._amax(res_u, res_v, res_cont)
                    print(f'NavierStokes NEWTON: Converged in {self._k} iterations with max-norm {mx}')
                break
            self._calc_jacobians(u, v)
            du, dv, dp = self._get_update(-res_u, -res_v, -res_cont)
            self.newton_history.append((norm, self.schur_matvecs))
            u = u + du
            v = v + dv
            p = p + dp
            self._k += 1
        return self._out(u, like), self._out(v, like), self._out(p, like)

    def run(self, T_func, points_plot):
        T = self._get_vector(T_func)
        u, v, p = self._get_solution(T)
        return self._get_interpol(u, points_plot), self._get_interpol(v, points_plot), self._get_interpol(p,
                                                                                                         points_plot)


class _SchurComplement:
    """The pressure Schur-complement operator of _get_update (NavierStokes_Solver.py:194-203):
    S dp = dres_cont(-J^-1 [G_x dp; G_y dp]_D, dp), i.e. two fused sem_ns_apply launches around one
    velocity solve.  The gradients are written straight into the solve's line-interleaved [u | v]
    layout and the divergence reads the solution from it (uv_pitch = 2 N_y), and the whole matvec is
    captured in one hipGraph per linearisation: a Krylov iteration then costs one graph launch.
    The base of the four Schur operators: a subclass gives _body (one matvec, eager) and, where its rules differ,
    _capture_kw; the capture, the eager fallback and the replay are device.CapturedOp's."""

    def __init__(self, ns, vs, graph=True):
        self.ns, self.vs = ns, vs
        m = ns._mesh
        # the [u | v] line buffer the bodies write into (all but _StripSchur's, which stacks plain vectors)
        self._B = torch.zeros((m.n_local // m.NY, 2 * m.NY), dtype=torch.float64, device=m.device)
        self._op = CapturedOp(m.device, self._body, m.n_local, **self._capture_kw(graph))

    _graph = property(lambda self: self._op.graph)
    _x = property(lambda self: self._op.x)
    _out = property(lambda self: self._op.out)

    def _capture_kw(self, graph):
        return dict(capture=graph and (self.vs.P == 1 or self.vs.interior != "lu"))

    def _body(self, dp):
        ns, m, NY = self.ns, self.ns._mesh, self.ns._mesh.NY
        B = self._B
        m.ns_apply(None, None, dp, B[:, :NY], B[:, NY:], **ns._ns_kw(pin_first=False))
        X = self.vs._solve_lines(B)
        rc = torch.empty_like(dp)
        m.ns_apply(X[:, :NY], X[:, NY:], dp, rc=rc, c_div=-1.0, **ns._ns_kw(pin_first=False))
        return rc

    def __call__(self, dp):
        return self._op(dp)


class _StripSchur(_SchurComplement):
    """The strip-partitioned Schur-complement operator (_schur_strips: gradient launch + interface assembly,
    the element-partitioned velocity solve with its all-gather, divergence launch + assembly).  Under RCCL
    every step stays on the device (collectives included), so the whole matvec is captured in one hipGraph
    per linearisation, as the whole-mesh _SchurComplement is; the capture is used only after its replay has
    reproduced the eager matvec on a probe vector, and every rank takes the same decision (CapturedOp's agreed
    capture).  Under gloo (the CPU rehearsal, host-staged collectives) the matvec stays eager."""

    def _capture_kw(self, graph):
        # SEM_STRIP_GRAPH=0 keeps the matvec eager (the capture of RCCL collectives is checked against
        # the eager matvec on a probe vector, but no multi-GPU run has exercised it yet -- DESIGN.md section 7)
        part = self.ns._part
        dev = part.backend_device()
        return dict(capture=graph and dev.type == "cuda" and os.environ.get("SEM_STRIP_GRAPH", "1") != "0",
                    agree=lambda ok: all_agree(part.dist, part.group, dev, ok), seed=5)

    def _body(self, dp):
        return self.ns._schur_strips(self.vs, dp)


class _StripSchurT(_StripSchur):
    """The strip-partitioned adjoint Schur-complement operator S^T q = E^T q - B^T J^-T C^T q: _SchurComplementT's
    body on the strips, under _StripSchur's capture rules (the same code).  The strip's transposed-gradient launch
    (sem_ns_apply_transpose_part, c_div = -1) writes -C^T q straight into the solve's [u | v] line buffer, whose two
    interface lines are summed across the strips in the line layout (Partition.assemble_lines: one pack launch for
    both components of both lines, one collective, one unpack); the transposed strip solve runs on it; the
    transposed-divergence launch reads the solution's line views and writes yp, assembled as a plain vector.  No
    field is stacked into or reshaped out of the line layout."""

    def _body(self, q):
        ns, m, part, NY = self.ns, self.ns._mesh, self.ns._part, self.ns._mesh.NY
        kw = ns._ns_kw(pin_first=False)
        B = self._B
        with phase("schur_T.grad_apply"):
            m.ns_apply_transpose_part(None, None, q, B[:, :NY], B[:, NY:], c_div=-1.0, **kw)
        with phase("schur_T.grad_assemble"):
            part.assemble_lines(B)
        with phase("schur_T.velocity_solve"):
            X = self.vs._solve_lines_T(B)
        yp = torch.empty_like(q)
        with phase("schur_T.div_apply"):
            m.ns_apply_transpose_part(X[:, :NY], X[:, NY:], q, yp=yp, **kw)
        with phase("schur_T.div_assemble"):
            part.assemble(yp)
        return yp


class _SchurComplementT(_SchurComplement):
    """The adjoint Schur-complement operator of _get_update_T, S^T q = E^T q - B^T J^-T C^T q: the transposed-gradient
    launch (-C^T q, written straight into the solve's [u | v] line buffer), the transposed velocity solve on the line
    layout, and the transposed-divergence launch (B^T x + E^T q, reading the solution from it) -- two fused
    sem_ns_apply_transpose launches around one solve, _SchurComplement._body mirrored, captured in one hipGraph per
    linearisation by the same capture / fallback code."""

    def _body(self, q):
        ns, m, NY = self.ns, self.ns._mesh, self.ns._mesh.NY
        B = self._B
        m.ns_apply_transpose(None, None, q, B[:, :NY], B[:, NY:], c_div=-1.0, **ns._ns_kw(pin_first=False))
        X = self.vs._solve_lines_T(B)
        yp = torch.empty_like(q)
        m.ns_apply_transpose(X[:, :NY], X[:, NY:], q, yp=yp, **ns._ns_kw(pin_first=False))
        return yp
