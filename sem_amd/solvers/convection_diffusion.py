"""Convection-diffusion solver counterpart on the device operators.

Mirrors Solvers/ConvectionDiffusion_Solver.py:9-203 (same constructor, same
private methods the OpenMDAO component calls, same error behaviour), with the
operator applies on the GPU:

  * `_get_residuals`  (:73-92)   -> ONE fused launch: Sys T with Dirichlet rows
                                    res = T - T_dir (SEM_DIR_IDENTITY + dir_val)
  * `_calc_jacobians` (:94-102)  -> Pe*G_x T, Pe*G_y T once per linearisation
  * `_get_dresiduals` (:104-121) -> ONE fused launch: Sys dT + (Pe G_x T).du
                                    + (Pe G_y T).dv with Dirichlet rows dres = dT

Vectors may be NumPy arrays (returned as NumPy, like the reference) or float64
device tensors (kept on the device).  The Dirichlet mask is built exactly as the
reference builds it (np.isclose on the node coordinates, :62-71); when it is the
plain boundary-line set the kernel derives it from geometry (no mask traffic).
`_get_update` runs a device-resident GMRES (sem_amd/krylov.py: Krylov basis in
HBM, CGS2 orthogonalisation as GEMVs, same stopping rule atol = mtol*sqrt(N) as
the reference's LGMRES); `krylov="scipy"` keeps the reference's host LGMRES
around device matvecs.  On a whole-mesh solver the GMRES is right-preconditioned
by a direct solve of the Jacobian itself (`precond="condensed"`, the default):
the static condensation over node lines of the NS velocity solve
(velocity_solve.py) with one unknown per node, factored once per Sys.  Right
preconditioning leaves the stopping test on the true residual ||dres_op(dT) -
dres||_2, so the reference's rule is unchanged; the Krylov count drops from
hundreds-thousands of matvecs to one or two.
"""
import numpy as np
import scipy.sparse.linalg as linalg
import torch

from .. import SEM, _lib
from ..device import get_mesh
from ..krylov import Recycle, gcro, gmres
from ..operators import ConvectionTensor, SEMOperator
from ._base import SolverBase
from .velocity_solve import VelocityJacobianSolver


def side_mask(points, L_x, L_y, sides):
    """Boundary-line mask for side bits, from the same np.isclose tests as the reference."""
    m = np.zeros(points.shape[1], dtype=bool)
    if sides & _lib.SIDE_W:
        m |= np.isclose(points[0], 0)
    if sides & _lib.SIDE_E:
        m |= np.isclose(points[0], L_x)
    if sides & _lib.SIDE_S:
        m |= np.isclose(points[1], 0)
    if sides & _lib.SIDE_N:
        m |= np.isclose(points[1], L_y)
    return m


def geometric_mask(NX, NY, sides):
    gx, gy = np.divmod(np.arange(NX * NY), NY)
    m = np.zeros(NX * NY, dtype=bool)
    if sides & _lib.SIDE_W:
        m |= gx == 0
    if sides & _lib.SIDE_E:
        m |= gx == NX - 1
    if sides & _lib.SIDE_S:
        m |= gy == 0
    if sides & _lib.SIDE_N:
        m |= gy == NY - 1
    return m


class DirichletRows:
    """Device form of a reference Dirichlet mask (global, np.isclose-built): side bits when it is
    exactly the boundary lines (the usual case), an explicit uint8 mask otherwise.  On a strip
    mesh the mask is the strip's slice."""

    def __init__(self, mesh, mask, sides):
        sl = slice(mesh.dof_begin, mesh.dof_begin + mesh.n_local)
        full = np.asarray(mask, dtype=bool)
        self.mask_np = full[sl]
        if np.array_equal(full, geometric_mask(mesh.NX, mesh.NY, sides)):
            self.sides, self.mask = sides, None
        else:
            self.sides = 0
            self.mask = torch.as_tensor(self.mask_np.astype(np.uint8), device=mesh.device)

    def kw(self):
        return dict(dir_sides=self.sides, dir_mask=self.mask)


class ConvectionDiffusionSolver(SolverBase):
    _name = "ConvectionDiffusion"
    _partition_adjoint_modes = ("condensed",)

    def __init__(self, L_x: float, L_y: float, Pe: float, P: int, N_ex: int, N_ey: int,
                 T_W: float = None, T_E: float = None, T_S: float = None, T_N: float = None,
                 mtol=1e-7, iprint: list = [], krylov: str = "device", max_basis: int = 2000,  # noqa: B006
                 partition=None, recycle_bytes: float = 0.0, precond: str = "condensed",
                 partition_update: str = "distributed", partition_adjoint: bool = False):
        """partition: a sem_amd.parallel.Partition -- the solver then holds one element-column strip
        per rank, every apply ends with the interface exchange (overlapped with the interior) and
        the Krylov inner products are all-reduced; the reference methods still take and return
        global NumPy vectors (local strips when given device tensors).
        partition_update: how a partitioned solver solves its Newton update -- "distributed": the
        device GMRES over the strips (every matvec a strip apply + exchange, inner products
        all-reduced), right-preconditioned by the element-partitioned condensed direct solve of the
        Jacobian (strip_solve.StripLineSolver: each rank factors its own columns, the ranks share a
        reduced system over the strip-boundary lines); "central": the Sys velocity field and the
        right-hand side are gathered, rank 0's whole-mesh counterpart (_central_solver) solves with
        the condensed direct preconditioner, the update is broadcast.
        partition_adjoint: opt-in to reverse mode on a partitioned solver -- _get_dresiduals_T and
        _get_update_T then run over the strips (parallel.StripApplyT: each rank's transposed strip apply
        + the interface exchange).  True: the adjoint solve is the UNPRECONDITIONED distributed GMRES; "condensed":
        it is right-preconditioned by the element-partitioned condensed direct solve applied transposed
        (StripLineSolver(adjoint=True).solve1_T: the forward update's factor, nothing stored twice).  Any other
        string raises ValueError.  Off by default: a partitioned solver refuses both methods."""
        if krylov not in ("device", "scipy"):
            raise ValueError("krylov must be 'device' or 'scipy'")
        if partition is not None and krylov != "device":
            raise ValueError("a partitioned solver needs krylov='device'")
        if precond not in ("condensed", None):
            raise ValueError("precond must be 'condensed' or None")
        # a partitioned solver preconditions with the element-partitioned condensation (strip_solve.py)
        self._precond = precond
        super().__init__(partition, partition_update, partition_adjoint)
        self._args = dict(L_x=L_x, L_y=L_y, Pe=Pe, P=P, N_ex=N_ex, N_ey=N_ey, T_W=T_W, T_E=T_E, T_S=T_S, T_N=T_N,
                          mtol=mtol, iprint=iprint, max_basis=max_basis, precond=precond)
        self._factor = None     # condensed Jacobian of the current Sys (rebuilt after _get_residuals)
        self._krylov, self._max_basis = krylov, max_basis
        # recycled Krylov subspace across _get_update calls with one operator (sem_amd.krylov.Recycle):
        # the Boussinesq coupler's block-Jacobi preconditioner solves with the same Sys tens of times
        self._recycle_bytes, self._recycle = recycle_bytes, None
        self._iprint = iprint
        self._Pe = Pe
        self._mtol = mtol
        self._L_x, self._L_y = L_x, L_y
        self._P, self._N_ex, self._N_ey = P, N_ex, N_ey
        dx, dy = L_x / N_ex, L_y / N_ey
        self.points = SEM.global_nodes(P, N_ex, N_ey, L_x / N_ex, L_y / N_ey)
        self.points_e = SEM.element_nodes(P, N_ex, N_ey, dx, dy)
        self.N = (N_ex * P + 1) * (N_ey * P + 1)
        if partition is None:
            self._mesh = get_mesh(P, N_ex, N_ey, dx, dy)
            self._apply = self._mesh.apply
        else:
            self._mesh = partition.setup(P, N_ex, N_ey, dx, dy)
            self._apply = partition.step

        # global operators (matrix-free; on a strip mesh when partitioned)
        m = self._mesh
        self._M = SEMOperator(m, cM=1.0)
        self._K = SEMOperator(m, cK=1.0)
        self._C_x, self._C_y = ConvectionTensor(m, "x"), ConvectionTensor(m, "y")
        self._Sys = None
        self._Jac_T_u = None
        self._Jac_T_v = None

        # Dirichlet values and mask (ConvectionDiffusion_Solver.py:62-71)
        self._dirichlet = np.full(self.N, np.nan)
        sides = 0
        for val, coord, target, bit in ((T_W, 0, 0, _lib.SIDE_W), (T_E, 0, L_x, _lib.SIDE_E),
                                        (T_S, 1, 0, _lib.SIDE_S), (T_N, 1, L_y, _lib.SIDE_N)):
            if val is not None:
                self._dirichlet[np.isclose(self.points[coord], target)] = val
                sides |= bit
        self._mask_dir = ~np.isnan(self._dirichlet)
        self._dir = DirichletRows(self._mesh, self._mask_dir, sides)
        self._dir_val = self._dev(np.where(self._mask_dir, self._dirichlet, 0.0))

    # ------------------------------------------------------------------ reference methods
    def _get_residuals(self, T, u, v):
        """res = Sys T, Dirichlet rows T - T_dir (ConvectionDiffusion_Solver.py:73-92)."""
        Conv = self._Pe * (SEM.tensordot(self._C_x, self._dev(u), (1, 0)) + SEM.tensordot(self._C_y, self._dev(v), (1, 0)))
        self._Sys = Conv + self._K
        self._factor = None
        if self._part is not None:
            self._twin_lin, self._twin_stale = (self._dev(u), self._dev(v)), True
        if self._recycle is not None:   # the update operator depends on Sys
            self._recycle.reset()
        y = self._apply(self._dev(T), dir_mode=_lib.DIR_IDENTITY, dir_val=self._dir_val, **self._sys_kw(),
                        **self._dir.kw())
        return self._out(y, T)

    def _calc_jacobians(self, T):
        """Pe diag(G_x T), Pe diag(G_y T) (ConvectionDiffusion_Solver.py:94-102)."""
        if self._part is None:
            self._Jac_T_u = self._Pe * SEM.tensordot(self._C_x, T, (2, 0))
            self._Jac_T_v = self._Pe * SEM.tensordot(self._C_y, T, (2, 0))
        else:  # G_x T on a strip needs the interface exchange before it becomes a diagonal
            Td = self._dev(T)
            self._Jac_T_u = SEMOperator(self._mesh, dg=[(self._Pe, self._apply(Td, c_gradx=1.0))])
            self._Jac_T_v = SEMOperator(self._mesh, dg=[(self._Pe, self._apply(Td, c_grady=1.0))])

    def _get_dresiduals(self, dT, du=None, dv=None):
        """dres = Sys dT + J_u du + J_v dv, Dirichlet rows dT (ConvectionDiffusion_Solver.py:104-121)."""
        kw = {}
        if du is not None or dv is not None:
            ju = self._Jac_T_u._coeffs()[4] if du is not None else None
            jv = self._Jac_T_v._coeffs()[4] if dv is not None else None
            kw = dict(c_extra=1.0, ea=ju, eb=self._dev(du), ec=jv, ed=self._dev(dv))
        y = self._apply(self._dev(dT), dir_mode=_lib.DIR_IDENTITY, **self._sys_kw(), **self._dir.kw(), **kw)
        return self._out(y, dT)

    def _apply_T(self, w, y=None, **kw):
        """A_D^T w: one fused transposed launch of Sys with identity Dirichlet rows; on a partitioned solver
        the transposed strip apply with the interface exchange (partition.step_T; w agrees on shared lines)."""
        launch = self._mesh.apply_transpose if self._part is None else self._part.step_T
        return launch(w, y, dir_mode=_lib.DIR_IDENTITY, **self._sys_kw(), **self._dir.kw(), **kw)

    def _get_dresiduals_T(self, dres_bar):
        """Transpose of _get_dresiduals(dT, du, dv): (dT_bar, du_bar, dv_bar) with
        dT_bar = A_D^T dres_bar, du_bar = (Pe G_x T) (1 - m) dres_bar, dv_bar = (Pe G_y T) (1 - m) dres_bar
        (m = the Dirichlet mask), so that <_get_dresiduals(dT, du, dv), w> = <dT, dT_bar> + <du, du_bar> +
        <dv, dv_bar>.  Needs _get_residuals and _calc_jacobians, like the forward method.  On a partitioned
        solver (partition_adjoint=True) dT_bar is assembled by the interface exchange; the two pointwise
        products are local to every node and need none.  NumPy in, gathered NumPy out; local tensors in (equal
        on shared lines), local tensors out."""
        self._whole_mesh_only("_get_dresiduals_T", adjoint=True)
        if self._Sys is None or self._Jac_T_u is None:
            raise RuntimeError("ConvectionDiffusion: _get_residuals and _calc_jacobians must run before "
                               "_get_dresiduals_T")
        w = self._dev(dres_bar)
        wf = self._free_rows() * w
        out = (self._apply_T(w), self._Jac_T_u._coeffs()[4] * wf, self._Jac_T_v._coeffs()[4] * wf)
        return tuple(self._out(y, dres_bar) for y in out)

    def _get_update_T(self, dT_bar, dres0=None):
        """Adjoint of the Newton update: solve A_D^T lambda = dT_bar with the device GMRES, every
        iteration one fused transposed apply.  Stopping rule and restart are the forward solve's
        (atol = mtol sqrt(N), rtol = 0, restart = min(int(0.3 N), max_basis)).  With precond="condensed"
        (the default) it is right-preconditioned, as the forward solve is, by the condensed direct factor
        applied transposed (VelocityJacobianSolver.solve1_T: the same factor, no second one; restart at most
        100; on the GPU the transposed solve is captured in a graph on its first use); the stopping test stays
        on the true residual.  precond=None: the unpreconditioned solve.
        On a partitioned solver (partition_adjoint=True) every iteration is a transposed strip apply plus the
        interface exchange, the inner products are all-reduced (partition.inner), the restart comes from the
        global N and is the same on every rank.  partition_adjoint=True leaves that solve unpreconditioned whatever
        `precond` says; partition_adjoint="condensed" (with precond="condensed", P > 1) right-preconditions it with
        the strip factor's transposed solve (StripLineSolver.solve1_T: one transposed GEMV and one all-reduce over the
        strip-boundary lines per application; captured in a graph when the collective runs on the device)."""
        self._whole_mesh_only("_get_update_T", adjoint=True)
        if self._Sys is None:
            raise RuntimeError("ConvectionDiffusion: _get_residuals must run before _get_update_T")
        kw, precond = {}, None
        if self._part is not None:
            kw = dict(inner=self._part.inner)
        condensed = self._precond == "condensed" and (
            self._part is None or (self._partition_adjoint_mode == "condensed" and self._P > 1))
        if condensed:
            vs = self._jacobian_solver()
            if vs.device.type == "cuda" and vs._graph_T is None:
                vs.capture_T()
            precond = vs.solve1_T
        x = self._krylov_solve(gmres, lambda v: self._apply_T(v), self._dev(dT_bar), self._dev(dres0), precond,
                               "adjoint GMRES", progress=False, maxiter=10 * self.N, **kw)
        return self._out(x, dT_bar)

    def _get_update(self, dres, dT0=None):
        """Newton update: solve dres_op(dT) = dres (ConvectionDiffusion_Solver.py:123-156)."""
        if self._part is not None and self._partition_update == "central":
            return self._get_update_central(dres, dT0)
        if self._krylov == "device":
            return self._get_update_device(dres, dT0)
        return self._get_update_scipy(dres, dT0)

    def _jacobian_solver(self):
        """Direct solve of dres_op = Sys with Dirichlet identity rows (ConvectionDiffusion_Solver.py:
        104-121 at du = dv = 0): sem_condensed_blocks with one component writes the condensation
        pieces, VelocityJacobianSolver factors them (on a partitioned solver: StripLineSolver, each rank
        its own strip); kept until Sys changes (_get_residuals)."""
        if self._factor is None:
            if self._Sys is None:
                raise RuntimeError("ConvectionDiffusion: _get_residuals must run before _get_update")
            m = self._mesh
            if self._part is not None:
                from .strip_solve import StripLineSolver
                p = self._part
                vs = StripLineSolver(self._P, self._N_ex, self._N_ey, m.device, p.part.bounds, p.rank, p.dist,
                                     group=p.group, ncomp=1, gather_device=p.backend_device(),
                                     adjoint=self._partition_adjoint_mode == "condensed")
            else:
                # transpose=True: the same factor preconditions the adjoint solve (_get_update_T); nothing of the
                # forward solve changes, and what the transposed solve adds is built on its first use
                vs = VelocityJacobianSolver(self._P, self._N_ex, self._N_ey, m.device, ncomp=1, transpose=True)
            cX, cu, cY, cv, d = self._Sys._coeffs()
            vs.factor_mesh(m, c_mass=self._Sys.cM, c_stiff=self._Sys.cK, c_gradx=cX, cu=cu, c_grady=cY, cv=cv, juu=d,
                           **self._dir.kw())
            if m.device.type == "cuda":
                vs.capture()
            self._factor = vs
        return self._factor

    def _restart(self, precond):
        """restart = min(int(0.3 N), max_basis) (the reference's inner_m, capped so the basis fits device memory), at
        most 100 under a preconditioner; from the global N, so the same on every rank."""
        restart = max(1, min(int(self.N * 0.3), self._max_basis))
        return restart if precond is None else min(restart, 100)

    def _krylov_solve(self, krylov, matvec, b, x0, precond, label, progress, **kw):
        """The device Krylov solve of _get_update_device and _get_update_T: `krylov` (gcro or gmres) with the basis in
        HBM, the reference's stopping rule atol = mtol sqrt(N), _restart's restart, the iteration callback (progress:
        honouring the _progress hook), the convergence check, self.matvecs and the LGMRES_suc report."""
        it = [0]
        prog = self._progress if progress else 0

        def cb(est):
            it[0] += 1
            if "LGMRES_iter" in self._iprint or (prog and it[0] % prog == 0):
                print(f"ConvectionDiffusion {label}: {it[0]}\t{est}", flush=True)

        r = krylov(matvec, b, x0=x0, atol=self._mtol * np.sqrt(self.N), rtol=0.0, restart=self._restart(precond),
                   precond=precond, callback=cb, **kw)
        if r.info != 0:
            raise RuntimeError(f"ConvectionDiffusion LGMRES: Failed to converge in {r.info} iterations")
        self.matvecs = r.matvecs
        if "LGMRES_suc" in self._iprint:
            res = (matvec(r.x) - b).abs().max().item()
            print(f"ConvectionDiffusion {label}: Converged in {r.matvecs} evaluations with max-norm {res}")
        return r.x

    def _get_update_device(self, dres, dT0=None):
        """GMRES with the Krylov basis in HBM (_krylov_solve), right-preconditioned by the condensed direct solve
        when precond="condensed": over the strips the GMRES with all-reduced inner products, on the whole mesh GCRO
        (recycling, when asked for, only without the preconditioner)."""
        precond = None
        if self._precond == "condensed" and (self._part is None or self._P > 1):
            precond = self._jacobian_solver().solve1
        if self._part is not None:
            krylov, kw = gmres, dict(maxiter=10 * self.N, inner=self._part.inner)
        else:
            if self._recycle_bytes and self._recycle is None:
                n = self._mesh.n_local
                cap = min(n, max(self._restart(precond) + 1, int(self._recycle_bytes // (16 * n))))
                self._recycle = Recycle(n, torch.float64, self._mesh.device, cap)
            krylov, kw = gcro, dict(recycle=self._recycle if precond is None else None)
        x = self._krylov_solve(krylov, lambda v: self._get_dresiduals(v), self._dev(dres), self._dev(dT0), precond,
                               "GMRES", progress=True, **kw)
        return self._out(x, dres)

    def _central_solver(self):
        """Rank 0's whole-mesh counterpart for partition_update="central" (same arguments, no
        partition)."""
        return ConvectionDiffusionSolver(**self._args)

    def _get_update_central(self, dres, dT0=None):
        """The partitioned solver's update on rank 0's whole-mesh counterpart (SolverBase._central): its Sys is set
        from the gathered velocity field of the last _get_residuals (the reference interface), it solves with the
        condensed direct preconditioner, and the update is broadcast to every rank."""
        if self._twin_lin is None:
            raise RuntimeError("ConvectionDiffusion: _get_residuals must run before _get_update")
        return self._central(lambda twin, u, v: twin._get_residuals(np.zeros(self.N), u, v),
                             lambda twin, b, x0: (twin._get_update(b, dT0=x0),), (dres, dT0), 1, "matvecs",
                             "the update")[0]

    def _get_update_scipy(self, dres, dT0=None):
        """The reference's LGMRES on the host around device matvecs."""

        def lhs_mv(dT):
            lhs_mv.fCount += 1
            return self._get_dresiduals(np.ascontiguousarray(dT, dtype=np.float64).ravel())

        lhs_mv.fCount = 0
        lhs_LO = linalg.LinearOperator((self.N,) * 2, lhs_mv, dtype=float)
        dres = np.asarray(dres.cpu().numpy() if isinstance(dres, torch.Tensor) else dres)

        def print_res(xk):
            print_res.iterCount += 1
            if "LGMRES_iter" in self._iprint:
                print(f"ConvectionDiffusion LGMRES: {print_res.iterCount}\t{np.linalg.norm(lhs_LO.matvec(xk) - dres)}")

        print_res.iterCount = 0
        dT, info = linalg.lgmres(A=lhs_LO, b=dres, M=None, x0=dT0, atol=self._mtol * np.sqrt(self.N), rtol=0,
                                 inner_m=int(self.N * 0.3), callback=print_res)
        if info != 0:
            raise RuntimeError(f"ConvectionDiffusion LGMRES: Failed to converge in {info} iterations")
        if "LGMRES_suc" in self._iprint:
            res = np.linalg.norm(lhs_LO.matvec(dT) - dres, ord=np.inf)
            print(f"ConvectionDiffusion LGMRES: Converged in {lhs_mv.fCount} evaluations with max-norm {res}")
        return dT

    def _get_solution(self, u, v, T0=None):
        """Single Newton step (ConvectionDiffusion_Solver.py:158-170)."""
        if self._part is not None and not isinstance(u, torch.Tensor):   # strips for the whole step
            Tl = self._dev(T0) if T0 is not None else torch.zeros(self._mesh.n_local, dtype=torch.float64,
                                                                   device=self._mesh.device)
            Tl = self._get_solution(self._dev(u), self._dev(v), Tl)
            return self._out(Tl, u)
        T = T0 if T0 is not None else np.zeros(self.N)
        res = self._get_residuals(T, u, v)
        dT = self._get_update(-res)
        return T + dT

    def run(self, u_func, v_func, points_plot):
        u = self._get_vector(u_func)
        v = self._get_vector(v_func)
        T = self._get_solution(u, v)
        return self._get_interpol(T, points_plot)
