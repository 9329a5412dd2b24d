"""What the Navier-Stokes and the convection-diffusion solver share: moving vectors between the reference's global
NumPy interface and this rank's device strip, the whole-mesh guard, the fused `_operator`, and the protocol by which
rank 0's whole-mesh counterpart runs a partitioned solver's update (`_central`)."""
import numpy as np
import torch

from .. import SEM


class SolverBase:
    _name = ""                   # the solver's name in its messages
    _whole_mesh_note = ""        # what _whole_mesh_only adds to a plain refusal
    _partition_adjoint = False   # reverse mode on a partitioned solver is opt-in
    _partition_adjoint_modes = ()   # the strings a solver takes for partition_adjoint besides a bool
    _progress = 0                # print the Krylov estimate every _progress iterations (set by tools)

    def __init__(self, partition, partition_update, partition_adjoint):
        if partition_update not in ("distributed", "central"):
            raise ValueError("partition_update must be 'distributed' or 'central'")
        self._part, self._partition_update = partition, partition_update
        if isinstance(partition_adjoint, str) and partition_adjoint not in self._partition_adjoint_modes:
            raise ValueError(f"partition_adjoint must be a bool" +
                             "".join(f" or '{v}'" for v in self._partition_adjoint_modes))
        # the value beside its truthiness: a string names how the partitioned adjoint update is preconditioned
        self._partition_adjoint, self._partition_adjoint_mode = bool(partition_adjoint), partition_adjoint
        self._free = None        # 1 - Dirichlet mask as a device vector (_free_rows)
        # rank 0's whole-mesh counterpart, the local fields of the linearisation it has to be given, and whether it
        # has them yet: one record for the forward and the adjoint update
        self._twin, self._twin_lin, self._twin_stale = None, None, True

    def _dev(self, a):
        """Device vector of this solver's (local) DOFs; a global NumPy vector is sliced to the strip."""
        if a is None:
            return None
        if self._part is not None and not isinstance(a, torch.Tensor):
            a = self._part.local(np.asarray(a))
        return self._mesh.to_device(a)

    def _out(self, t, like):
        if isinstance(like, torch.Tensor):
            return t
        if self._part is not None:
            t = self._part.gather(t)
        return t.cpu().numpy()

    def _global(self, a):
        """Global NumPy vector from a global NumPy vector or this rank's strip tensor."""
        if isinstance(a, torch.Tensor) and self._part is not None:
            return self._part.gather(a).cpu().numpy()
        return np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)

    def _whole_mesh_only(self, what, adjoint=False):
        """Refuse `what` on a partitioned solver; adjoint=True: unless partition_adjoint opted in."""
        if self._part is not None and not (adjoint and self._partition_adjoint):
            raise ValueError(f"{self._name}: {what} is implemented for whole-mesh solvers only" +
                             (" unless the partitioned solver was built with partition_adjoint=True" if adjoint else
                              self._whole_mesh_note))

    def _free_rows(self):
        """1 - m (m the Dirichlet mask) on the device, built on first use."""
        if self._free is None:
            self._free = self._mesh.to_device((~self._dir.mask_np).astype(np.float64))
        return self._free

    def _sys_kw(self, Sys=None):
        Sys = self._Sys if Sys is None else Sys
        cX, cu, cY, cv, d = Sys._coeffs()
        return dict(c_stiff=Sys.cK, c_mass=Sys.cM, c_gradx=cX, cu=cu, c_grady=cY, cv=cv)

    def _operator(self, x, c_mass=0.0, c_stiff=0.0, cu=None, cv=None, free=False):
        """(c_mass M + c_stiff K + diag(cu) G_x + diag(cv) G_y) x on this solver's mesh in one fused launch, no
        row replaced; free=True zeroes the (velocity) Dirichlet rows.  What the coupler's parameter partials and the
        functionals (solvers/functionals.py) are built from.  NumPy in, NumPy out; device tensors likewise."""
        self._whole_mesh_only("_operator")
        kw = {}
        if cu is not None:
            kw.update(c_gradx=1.0, cu=self._dev(cu))
        if cv is not None:
            kw.update(c_grady=1.0, cv=self._dev(cv))
        y = self._mesh.apply(self._dev(x), c_mass=c_mass, c_stiff=c_stiff, **kw)
        if free:
            y = self._free_rows() * y
        return self._out(y, x)

    def _central(self, refresh, call, args, n_out, count_attr, what):
        """A partitioned solver's update on rank 0's whole-mesh counterpart (the twin, _central_solver()).  Every rank
        gathers the linearisation's fields (_twin_lin, only while the twin does not have them) and then `args` (None
        entries stay None); rank 0 runs refresh(twin, *fields) when stale and call(twin, *args), which returns n_out
        global vectors; they are broadcast with a status word that carries the twin's `count_attr`.  A failure on
        rank 0 (non-convergence, a singular block, out of memory) travels as a NaN status, so every rank raises
        instead of waiting in the collective.  Tensors in `args`: local tensors out; NumPy: global NumPy out."""
        part, N = self._part, self.N
        stale, self._twin_stale = self._twin_stale, False
        lin = [self._global(a) for a in self._twin_lin] if stale else None
        glob = [None if a is None else self._global(a) for a in args]
        out = torch.zeros(n_out * N + 1, dtype=torch.float64)
        err = None
        if part.rank == 0:
            try:
                if stale:
                    if self._twin is None:
                        self._twin = self._central_solver()
                    refresh(self._twin, *lin)
                res = call(self._twin, *glob)
                out[:n_out * N] = torch.from_numpy(np.concatenate([np.asarray(a) for a in res]))
                out[-1] = float(getattr(self._twin, count_attr, -1))
            except (RuntimeError, ValueError) as e:
                err = e
                out[-1] = float("nan")
        out = part.broadcast(out)
        if err is not None:
            raise err
        if torch.isnan(out[-1]):
            raise RuntimeError(f"{self._name}: {what} failed on rank 0 (see its error)")
        setattr(self, count_attr, int(out[-1].item()))
        res = [out[i * N:(i + 1) * N].cpu().numpy() for i in range(n_out)]
        if isinstance(args[0], torch.Tensor):
            return tuple(self._dev(a) for a in res)
        return tuple(res)

    def _get_vector(self, f_func):
        return f_func(self.points[0], self.points[1])

    def _get_interpol(self, f, points_plot):
        f_e = SEM.scatter(f, self._P, self._N_ex, self._N_ey)
        return SEM.eval_interpolation(f_e, self.points_e, points_plot)
