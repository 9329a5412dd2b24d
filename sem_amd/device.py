"""Device-side mesh handle: owns one libsemops handle and launches the kernels.

PyTorch-ROCm is plumbing here: it provides device buffers, the current HIP
stream and (for multi-GPU) torch.distributed/RCCL.  All arithmetic of the
operator layer runs in the HIP kernels of libsemops.
"""
import contextlib
import ctypes as C
import gc

import numpy as np
import torch

from . import _lib


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("the SEM operator layer runs on a ROCm GPU (gfx950); no GPU is visible -- "
                           "there is no CPU fallback")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


_NS_T_NAMES = ("zu", "zv", "zc", "yu", "yv", "yp", "yT")    # the operands of the transposed Navier-Stokes entries


class Mesh:
    """N_ex x N_ey elements of order P with widths dx, dy, holding element columns
    [ex_begin, ex_end) on one GPU (the whole mesh by default)."""

    def __init__(self, P, nex, ney, dx, dy, ex_begin=0, ex_end=None, device=None):
        require_gpu()
        lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        ex_end = nex if ex_end is None else ex_end
        h = C.c_void_p()
        _lib.check(lib.sem_create(int(P), int(nex), int(ney), float(dx), float(dy), int(ex_begin), int(ex_end),
                                  self.device.index, C.byref(h)))
        self._h = h
        self._lib = lib
        info = _lib.SemInfo()
        _lib.check(lib.sem_get_info(h, C.byref(info)))
        self.P, self.nex, self.ney = info.P, info.nex, info.ney
        self.dx, self.dy = info.dx, info.dy
        self.ex_begin, self.ex_end = info.ex_begin, info.ex_end
        self.NX, self.NY, self.N = info.NX, info.NY, info.N
        self.line_begin, self.line_end = info.line_begin, info.line_end
        self.n_local, self.dof_begin = info.n_local, info.dof_begin

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.sem_destroy(h)
            self._h = None

    @property
    def key(self):
        return (self.P, self.nex, self.ney, self.dx, self.dy, self.ex_begin, self.ex_end, self.device.index)

    # ------------------------------------------------------------------ helpers
    def to_device(self, v, dtype=torch.float64):
        if isinstance(v, torch.Tensor):
            t = v.to(device=self.device, dtype=dtype)
        else:
            t = torch.as_tensor(np.ascontiguousarray(v), dtype=dtype, device=self.device)
        return t.contiguous()

    def _vec(self, t, name):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.float64:
            raise ValueError(f"{name} must be a float64 tensor on {self.device}")
        if not t.is_contiguous() or t.numel() != self.n_local:
            raise ValueError(f"{name} must be contiguous with {self.n_local} entries, got {tuple(t.shape)}")
        return t

    def stream_ptr(self, stream=None):
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        return C.c_void_p(s.cuda_stream)

    # ------------------------------------------------------------------ kernels
    def _mask(self, dir_mask):
        """The explicit Dirichlet mask of every entry point: uint8, on the mesh's device, n_local entries."""
        if dir_mask is not None and (dir_mask.dtype != torch.uint8 or dir_mask.device != self.device
                                     or dir_mask.numel() != self.n_local):
            raise ValueError("dir_mask must be a uint8 tensor of n_local entries on the mesh device")
        return dir_mask

    def _apply_launch(self, entry, x, xname, y, c_mass, c_stiff, c_gradx, c_grady, cu, cv, c_extra, ea, ea_name, eb, ec,
                      ed, c_acc, dir_mode, dir_mask, dir_val, dir_sides, algo, pos, stream):
        """The checks, the SemApplyDesc and the launch of sem_apply and its two transposed entry points."""
        x = self._vec(x, xname)
        if y is None:
            y = torch.empty_like(x)
        self._vec(y, "y")
        for nm, t in (("cu", cu), ("cv", cv), (ea_name, ea), ("eb", eb), ("ec", ec), ("ed", ed), ("dir_val", dir_val)):
            self._vec(t, nm)
        self._mask(dir_mask)
        d = _lib.SemApplyDesc(float(c_mass), float(c_stiff), float(c_gradx), float(c_grady), _ptr(cu), _ptr(cv),
                              float(c_extra), _ptr(ea), _ptr(eb), _ptr(ec), _ptr(ed), float(c_acc), int(dir_mode),
                              _ptr(dir_mask), _ptr(dir_val), int(dir_sides), int(algo),
                              *((0, 0) if pos is None else (int(pos[0]), int(pos[1]))))
        _lib.check(entry(self._h, C.byref(d), _ptr(x), _ptr(y), self.stream_ptr(stream)))
        return y

    def apply(self, x, y=None, *, c_mass=0.0, c_stiff=0.0, c_gradx=0.0, c_grady=0.0, cu=None, cv=None, c_extra=0.0,
              ea=None, eb=None, ec=None, ed=None, c_acc=0.0, dir_mode=_lib.DIR_NONE, dir_mask=None, dir_val=None,
              dir_sides=0, algo=_lib.ALGO_AUTO, pos=None, stream=None):
        """Fused operator apply (include/sem_ops.h, sem_apply).  pos = (begin, end): write only the
        output lines of those element positions of the strip (0..ncols, ncols = closing line)."""
        return self._apply_launch(self._lib.sem_apply, x, "x", y, c_mass, c_stiff, c_gradx, c_grady, cu, cv, c_extra,
                                  ea, "ea", eb, ec, ed, c_acc, dir_mode, dir_mask, dir_val, dir_sides, algo, pos,
                                  stream)

    def apply_transpose(self, z, y=None, *, c_mass=0.0, c_stiff=0.0, c_gradx=0.0, c_grady=0.0, cu=None, cv=None,
                        diag=None, c_acc=0.0, dir_mode=_lib.DIR_NONE, dir_mask=None, dir_sides=0, stream=None,
                        eb=None, ec=None, ed=None, dir_val=None, algo=_lib.ALGO_AUTO, pos=None):
        """Fused transposed apply (include/sem_ops.h, sem_apply_transpose): y = A_D^T z + c_acc y for
        A = c_mass M + c_stiff K + c_gradx diag(cu) G_x + c_grady diag(cv) G_y + diag(diag) and identity
        Dirichlet rows.  One launch; whole-mesh handles only.  eb, ec, ed, dir_val, algo and pos are the
        remaining descriptor fields: the transposed apply takes none of them and the library refuses
        them as the header documents (ValueError / RuntimeError)."""
        return self._apply_launch(self._lib.sem_apply_transpose, z, "z", y, c_mass, c_stiff, c_gradx, c_grady, cu, cv,
                                  1.0 if diag is not None else 0.0, diag, "diag", eb, ec, ed, c_acc, dir_mode, dir_mask,
                                  dir_val, dir_sides, algo, pos, stream)

    def apply_transpose_part(self, z, y=None, *, c_mass=0.0, c_stiff=0.0, c_gradx=0.0, c_grady=0.0, cu=None, cv=None,
                             diag=None, c_acc=0.0, dir_mode=_lib.DIR_NONE, dir_mask=None, dir_sides=0, pos=None,
                             stream=None, eb=None, ec=None, ed=None, dir_val=None, algo=_lib.ALGO_AUTO):
        """Transposed apply of this handle's own matrix (include/sem_ops.h, sem_apply_transpose_part):
        y = A_s^T z + c_acc y for the A_s that `apply` applies here -- on a strip the partial sums of its
        own elements on both interface lines, the pointwise terms and Dirichlet entries of the right
        interface line left to its right-hand owner -- so that summing the strips' results over the shared
        lines (the forward exchange) gives the whole mesh's A_D^T z; z must agree on shared lines.
        pos = (begin, end): write only the output lines of those element positions (0..ncols, ncols = the
        closing line).  eb, ec, ed, dir_val and algo are refused as by apply_transpose."""
        return self._apply_launch(self._lib.sem_apply_transpose_part, z, "z", y, c_mass, c_stiff, c_gradx, c_grady, cu,
                                  cv, 1.0 if diag is not None else 0.0, diag, "diag", eb, ec, ed, c_acc, dir_mode,
                                  dir_mask, dir_val, dir_sides, algo, pos, stream)

    def transpose_kernel_name(self):
        buf = C.create_string_buffer(128)
        _lib.check(self._lib.sem_transpose_kernel_name(self._h, buf, 128))
        return buf.value.decode()

    def kernel_name(self, algo=_lib.ALGO_AUTO):
        buf = C.create_string_buffer(128)
        _lib.check(self._lib.sem_kernel_name(self._h, int(algo), buf, 128))
        return buf.value.decode()

    def gather_elements(self, u, out=None, stream=None):
        """SEM.scatter (SEM.py:149-167) on the device: u[N] -> u_e[m, n, i, j]."""
        u = self._vec(u, "u")
        n = self.P + 1
        shape = (self.ex_end - self.ex_begin, self.ney, n, n)
        out = torch.empty(shape, dtype=torch.float64, device=self.device) if out is None else out
        if out.shape != shape or not out.is_contiguous() or out.dtype != torch.float64:
            raise ValueError(f"out must be a contiguous float64 tensor of shape {shape}")
        _lib.check(self._lib.sem_gather_elements(self._h, _ptr(u), _ptr(out), self.stream_ptr(stream)))
        return out

    def dss(self, a_e, out=None, stream=None):
        """SEM.assemble for a 4-D element array (SEM.py:113-127): direct-stiffness summation."""
        n = self.P + 1
        shape = (self.ex_end - self.ex_begin, self.ney, n, n)
        if tuple(a_e.shape) != shape:
            raise ValueError(f"element array must have shape {shape}, got {tuple(a_e.shape)}")
        a_e = self.to_device(a_e)
        out = torch.empty(self.n_local, dtype=torch.float64, device=self.device) if out is None else self._vec(out,
                                                                                                             "out")
        _lib.check(self._lib.sem_dss(self._h, _ptr(a_e), _ptr(out), self.stream_ptr(stream)))
        return out

    def interface_pack(self, y, bounds, buf, stream=None):
        b = (C.c_int * len(bounds))(*bounds)
        _lib.check(self._lib.sem_interface_pack(self._h, _ptr(y), b, len(bounds) - 1, _ptr(buf),
                                                self.stream_ptr(stream)))

    def interface_unpack(self, buf, bounds, y, stream=None):
        b = (C.c_int * len(bounds))(*bounds)
        _lib.check(self._lib.sem_interface_unpack(self._h, _ptr(buf), b, len(bounds) - 1, _ptr(y),
                                                  self.stream_ptr(stream)))

    def _lines_args(self, Y, buf, bounds, cols, width):
        """The host checks of interface_pack_lines / interface_unpack_lines: Y the handle's lines as a 2-D float64
        view with unit column stride (row pitch = its row stride), `width` entries per line exchanged (default: the
        view's row length), cols a sequence of in-line offsets in [0, width) or None (whole lines), buf large
        enough for every slot.  The offsets are checked here, on the host, and kept on the device per distinct list
        (the library does not read them back).  Returns the C arguments between the handle and the buffer."""
        lines = self.line_end - self.line_begin + 1
        if (not isinstance(Y, torch.Tensor) or Y.device != self.device or Y.dtype != torch.float64 or Y.dim() != 2
                or Y.shape[0] != lines or (Y.shape[1] > 1 and Y.stride(1) != 1)):
            raise ValueError(f"Y must be a float64 ({lines}, width) line array on {self.device} with unit column stride")
        width = Y.shape[1] if width is None else int(width)
        pitch = Y.stride(0)
        if not 1 <= width <= Y.shape[1] or pitch < width:
            raise ValueError("interface lines: need 1 <= width <= the row length <= the row pitch")
        n, cptr = width, None
        if cols is not None:
            key = tuple(int(c) for c in cols)
            if not key or min(key) < 0 or max(key) >= width:
                raise ValueError("interface lines: cols must be a non-empty list of offsets in [0, width)")
            cache = self.__dict__.setdefault("_line_cols", {})
            if key not in cache:
                cache[key] = torch.tensor(key, dtype=torch.int32, device=self.device)
            n, cptr = len(key), _ptr(cache[key])
        G = len(bounds) - 1
        if (not isinstance(buf, torch.Tensor) or buf.device != self.device or buf.dtype != torch.float64
                or not buf.is_contiguous() or buf.numel() < (G - 1) * n):
            raise ValueError(f"buf must be a contiguous float64 tensor of at least {(G - 1) * n} entries on {self.device}")
        b = (C.c_int * len(bounds))(*bounds)
        return width, pitch, cptr, (0 if cols is None else n), b, G

    def interface_pack_lines(self, Y, bounds, buf, cols=None, width=None, stream=None):
        """sem_interface_pack_lines: the two interface lines of the line-layout array Y (first and last row; every
        component of a [u | v] line at once) into buf's slots, zeros in the slots of other boundaries; with cols only
        those in-line offsets.  A sum all-reduce of buf and interface_unpack_lines assemble Y's shared lines."""
        w, pitch, cptr, nc, b, G = self._lines_args(Y, buf, bounds, cols, width)
        _lib.check(self._lib.sem_interface_pack_lines(self._h, _ptr(Y), w, pitch, cptr, nc, b, G, _ptr(buf),
                                                      self.stream_ptr(stream)))

    def interface_unpack_lines(self, buf, bounds, Y, cols=None, width=None, stream=None):
        """sem_interface_unpack_lines: buf's slots of this handle's boundaries back onto Y's first / last row (with
        cols: only those offsets; everything else in Y is left alone)."""
        w, pitch, cptr, nc, b, G = self._lines_args(Y, buf, bounds, cols, width)
        _lib.check(self._lib.sem_interface_unpack_lines(self._h, _ptr(buf), w, pitch, cptr, nc, b, G, _ptr(Y),
                                                        self.stream_ptr(stream)))

    def _velocity_desc(self, c_mass, c_stiff, c_gradx, c_grady, cu, cv, juu, juv, jvu, jvv, dir_mask, dir_sides, ncomp,
                       cols):
        """The checks and the SemVelocityDesc of the two block writers; returns (descriptor, c0, c1)."""
        for nm, t in (("cu", cu), ("cv", cv), ("juu", juu), ("juv", juv), ("jvu", jvu), ("jvv", jvv)):
            self._vec(t, nm)
        self._mask(dir_mask)
        c0, c1 = (self.ex_begin, self.ex_end) if cols is None else (int(cols[0]), int(cols[1]))
        if not self.ex_begin <= c0 < c1 <= self.ex_end:
            raise ValueError("cols must be a non-empty element-column range of the handle's strip")
        d = _lib.SemVelocityDesc(float(c_mass), float(c_stiff), float(c_gradx), float(c_grady), _ptr(cu), _ptr(cv),
                                 _ptr(juu), _ptr(juv), _ptr(jvu), _ptr(jvv), _ptr(dir_mask), int(dir_sides),
                                 int(ncomp), c0, c1)
        return d, c0, c1

    def _check_blocks(self, blocks, want, empty_too=False):
        """Every wanted block is a contiguous float64 device tensor of its size (empty_too: a block of size 0 also)."""
        for nm, sz in want:
            t = blocks.get(nm)
            if (sz or empty_too) and (t is None or t.numel() != sz or t.dtype != torch.float64
                                      or t.device != self.device or not t.is_contiguous()):
                raise ValueError(f"block {nm} must be a contiguous float64 tensor of {sz} entries on {self.device}")

    def velocity_blocks(self, blocks, *, c_mass=0.0, c_stiff=0.0, c_gradx=0.0, c_grady=0.0, cu=None, cv=None,
                        juu=None, juv=None, jvu=None, jvv=None, dir_mask=None, dir_sides=0, ncomp=2, cols=None,
                        stream=None):
        """Static-condensation pieces of the NS velocity Jacobian (include/sem_ops.h,
        sem_velocity_blocks) into `blocks` (VelocityJacobianSolver.empty_blocks layout); ncomp=1:
        the scalar operator A + diag(juu) alone.  cols=(c0, c1): blocks["AII"] holds the dense
        interiors of element columns [c0, c1) only."""
        d, c0, c1 = self._velocity_desc(c_mass, c_stiff, c_gradx, c_grady, cu, cv, juu, juv, jvu, jvv, dir_mask,
                                        dir_sides, ncomp, cols)
        sizes = (C.c_int64 * 6)()
        _lib.check(self._lib.sem_line_block_sizes(self._h, int(ncomp), sizes))
        names = ("AII", "D", "aIB", "aBI", "E", "F")
        sizes[0] = sizes[0] // (self.ex_end - self.ex_begin) * (c1 - c0)
        self._check_blocks(blocks, zip(names, sizes))
        _lib.check(self._lib.sem_velocity_blocks(self._h, C.byref(d), *(_ptr(blocks.get(nm)) for nm in names),
                                                 self.stream_ptr(stream)))
        return blocks

    def condensed_blocks(self, blocks, *, c_mass=0.0, c_stiff=0.0, c_gradx=0.0, c_grady=0.0, cu=None, cv=None,
                         juu=None, juv=None, jvu=None, jvv=None, dir_mask=None, dir_sides=0, ncomp=2, cols=None,
                         stream=None):
        """The velocity (ncomp=2) or scalar (ncomp=1) Jacobian in the nested condensation's layout
        (include/sem_ops.h, sem_condensed_blocks, ABI 7): blocks["Aii", "Aie", "Aei", "Aed", "Aeu", "Ael"]
        hold element columns cols = (c0, c1); "D", "aIB", "aBI", "E", "F" the whole mesh's interface pieces."""
        d, c0, c1 = self._velocity_desc(c_mass, c_stiff, c_gradx, c_grady, cu, cv, juu, juv, jvu, jvv, dir_mask,
                                        dir_sides, ncomp, cols)
        line = (C.c_int64 * 6)()
        _lib.check(self._lib.sem_line_block_sizes(self._h, int(ncomp), line))
        cs = (C.c_int64 * 6)()
        _lib.check(self._lib.sem_condensed_block_sizes(self._h, int(ncomp), cs))
        cnames = ("Aii", "Aie", "Aei", "Aed", "Aeu", "Ael")
        lnames = ("D", "aIB", "aBI", "E", "F")
        self._check_blocks(blocks, [(nm, cs[i] * (c1 - c0)) for i, nm in enumerate(cnames)]
                           + list(zip(lnames, list(line)[1:])), empty_too=True)
        _lib.check(self._lib.sem_condensed_blocks(self._h, C.byref(d), *(_ptr(blocks[nm]) for nm in cnames + lnames),
                                                  self.stream_ptr(stream)))
        return blocks

    def _line_view(self, t, name, lines=None):
        """u, v, ru, rv of sem_ns_apply: a plain vector, or an (NX, NY) view with row stride >= NY (lines: the
        line count of the view when it is not NX)."""
        NX = self.NX if lines is None else lines
        if t is None:
            return None, 0
        if t.dim() == 1:
            return self._vec(t, name), 0
        if (not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.float64
                or tuple(t.shape) != (NX, self.NY) or t.stride(1) != 1 or t.stride(0) < self.NY):
            raise ValueError(f"{name} must be a float64 ({NX}, {self.NY}) line view on {self.device}")
        return t, t.stride(0)

    def ns_apply(self, u=None, v=None, p=None, ru=None, rv=None, rc=None, *, c_mass=0.0, c_stiff=0.0, c_gradx=0.0,
                 c_grady=0.0, cu=None, cv=None, juu=None, juv=None, jvu=None, jvv=None, c_T=0.0, T=None, c_div=1.0,
                 dval_u=None, dval_v=None, dir_mask=None, dir_sides=0, pin=-1, pin_val=0.0, pin_first=False,
                 stream=None):
        """Fused Navier-Stokes residuals (include/sem_ops.h, sem_ns_apply): ru, rv, rc in one launch.
        u, v, ru, rv are plain vectors or (NX, NY) line views sharing one row stride (the velocity
        solve's interleaved [u | v] lines); a None output is not computed.  Every other operand is a plain
        vector: cu may be u itself (cv: v) only when u, v are plain vectors too (ValueError otherwise)."""
        return self._ns_launch(self._lib.sem_ns_apply, ("u", "v", "p", "ru", "rv", "rc"), u, v, p, ru, rv, (rc,),
                               c_mass, c_stiff, c_gradx, c_grady, cu, cv, juu, juv, jvu, jvv, c_T, T, c_div, dval_u,
                               dval_v, dir_mask, dir_sides, pin, pin_val, pin_first, stream)

    def ns_apply_transpose(self, zu=None, zv=None, zc=None, yu=None, yv=None, yp=None, yT=None, *, c_mass=0.0,
                           c_stiff=0.0, c_gradx=0.0, c_grady=0.0, cu=None, cv=None, juu=None, juv=None, jvu=None,
                           jvv=None, c_T=0.0, T=None, c_div=1.0, dval_u=None, dval_v=None, dir_mask=None, dir_sides=0,
                           pin=-1, pin_val=0.0, pin_first=False, stream=None):
        """Fused transposed apply of ns_apply's linear part (include/sem_ops.h, sem_ns_apply_transpose):
        (yu, yv, yp) = A^T (zu, zv, zc) and yT = c_T M (1 - m) zv in one launch; returns (yu, yv, yp, yT).  zu, zv,
        yu, yv are plain vectors or (NX, NY) line views sharing one row stride; a None input is zeros, a None output
        is not computed.  Whole-mesh handles only.  T, dval_u, dval_v and pin_val are the descriptor fields the
        transpose of the linear part does not take: the library refuses them as the header documents."""
        return self._ns_launch(self._lib.sem_ns_apply_transpose, _NS_T_NAMES, zu, zv, zc, yu, yv, (yp, yT), c_mass,
                               c_stiff, c_gradx, c_grady, cu, cv, juu, juv, jvu, jvv, c_T, T, c_div, dval_u, dval_v,
                               dir_mask, dir_sides, pin, pin_val, pin_first, stream)

    def ns_apply_transpose_part(self, zu=None, zv=None, zc=None, yu=None, yv=None, yp=None, yT=None, *, c_mass=0.0,
                                c_stiff=0.0, c_gradx=0.0, c_grady=0.0, cu=None, cv=None, juu=None, juv=None, jvu=None,
                                jvv=None, c_T=0.0, T=None, c_div=1.0, dval_u=None, dval_v=None, dir_mask=None,
                                dir_sides=0, pin=-1, pin_val=0.0, pin_first=False, stream=None):
        """ns_apply_transpose for this handle's own matrix (include/sem_ops.h, sem_ns_apply_transpose_part):
        (yu, yv, yp) = A_s^T (zu, zv, zc) and yT for the A_s that `ns_apply` applies here -- on a strip the partial
        sums of its own elements on both interface lines, the pointwise terms, Dirichlet entries and the pinned row
        of the right interface line left to its right-hand owner -- so that summing the strips' results over the
        shared lines (the forward exchange) gives the whole mesh's A^T z; z must agree on shared lines.  Line views
        hold the handle's own lines; `pin` stays a global node index.  On a whole-mesh handle: bitwise
        ns_apply_transpose."""
        return self._ns_launch(self._lib.sem_ns_apply_transpose_part, _NS_T_NAMES, zu, zv, zc, yu, yv, (yp, yT), c_mass,
                               c_stiff, c_gradx, c_grady, cu, cv, juu, juv, jvu, jvv, c_T, T, c_div, dval_u, dval_v,
                               dir_mask, dir_sides, pin, pin_val, pin_first, stream,
                               lines=int(self.line_end - self.line_begin + 1))

    def _ns_launch(self, entry, names, u, v, p, ru, rv, tail, c_mass, c_stiff, c_gradx, c_grady, cu, cv, juu, juv, jvu,
                   jvv, c_T, T, c_div, dval_u, dval_v, dir_mask, dir_sides, pin, pin_val, pin_first, stream,
                   lines=None):
        """The checks, the SemNsDesc and the launch of the three Navier-Stokes entry points: entry(u, v, p, ru, rv,
        *tail) with `names` the operands' names in that order; u, v, ru, rv may be line views, the rest are plain
        vectors.  Returns (ru, rv, *tail)."""
        pitch = set()
        views = []
        for nm, t in zip(names[:2] + names[3:5], (u, v, ru, rv)):
            t, s = self._line_view(t, nm, lines)
            views.append(t)
            if t is not None:
                pitch.add(s)
        if len(pitch) > 1:
            raise ValueError(f"{', '.join(names[:2] + names[3:5])} must share one layout")
        for nm, t in ((names[2], p), *zip(names[5:], tail), ("T", T), ("cu", cu), ("cv", cv), ("juu", juu),
                      ("juv", juv), ("jvu", jvu), ("jvv", jvv), ("dval_u", dval_u), ("dval_v", dval_v)):
            self._vec(t, nm)
        self._mask(dir_mask)
        d = _lib.SemNsDesc(float(c_mass), float(c_stiff), float(c_gradx), float(c_grady), _ptr(cu), _ptr(cv),
                           _ptr(juu), _ptr(juv), _ptr(jvu), _ptr(jvv), float(c_T), _ptr(T), float(c_div),
                           _ptr(dval_u), _ptr(dval_v), _ptr(dir_mask), int(dir_sides), int(bool(pin_first)), int(pin),
                           float(pin_val), pitch.pop() if pitch else 0)
        _lib.check(entry(self._h, C.byref(d), *(_ptr(t) for t in views[:2]), _ptr(p), *(_ptr(t) for t in views[2:]),
                         *(_ptr(t) for t in tail), self.stream_ptr(stream)))
        return (views[2], views[3], *tail)

    # ------------------------------------------------------------------ host-side 1-D tables
    def weights_1d(self):
        """Assembled 1-D GLL weights over the locally held lines (x) and all columns (y)."""
        from . import GLL
        w = GLL.standard_nodes(self.P)[1]
        return (_assembled_diag(w, self.P, self.ex_begin, self.ex_end, self.line_begin, self.line_end),
                _assembled_diag(w, self.P, 0, self.ney, 0, self.NY - 1))


def _assembled_diag(vals, P, e_lo, e_hi, g_lo, g_hi):
    """sum over elements e in [e_lo, e_hi) of vals[local index] at each 1-D node g in [g_lo, g_hi]."""
    out = np.zeros(g_hi - g_lo + 1)
    for e in range(e_lo, e_hi):
        out[e * P - g_lo: e * P + P + 1 - g_lo] += vals
    return out


def mass_diagonal(P, nex, ney, dx, dy):
    """Diagonal of the whole mesh's assembled mass matrix (SEM.py:170-183): (dx/2)(dy/2) wx_g wy_g with the GLL
    weights summed over the elements holding each 1-D node (Mesh.weights_1d's sums, without a handle)."""
    from . import GLL
    w = GLL.standard_nodes(P)[1]
    wx, wy = _assembled_diag(w, P, 0, nex, 0, nex * P), _assembled_diag(w, P, 0, ney, 0, ney * P)
    return ((dx / 2) * (dy / 2)) * np.outer(wx, wy).ravel()


_MESHES = {}


def get_mesh(P, nex, ney, dx, dy, ex_begin=0, ex_end=None, device=None):
    """Cached Mesh per (P, N_ex, N_ey, dx, dy, partition, device)."""
    require_gpu()
    dev = torch.cuda.current_device() if device is None else int(device)
    ex_end = nex if ex_end is None else ex_end
    key = (int(P), int(nex), int(ney), float(dx), float(dy), int(ex_begin), int(ex_end), dev)
    m = _MESHES.get(key)
    if m is None:
        m = _MESHES[key] = Mesh(P, nex, ney, dx, dy, ex_begin, ex_end, dev)
    return m


@contextlib.contextmanager
def no_gc():
    """Keep Python's cyclic GC from running inside a stream capture: a collection there can run the
    finaliser of an unrelated object (an old hipGraph, a mesh handle) whose device calls are illegal
    while the stream captures, which aborts the process.  torch.cuda.graph collects on entry (an
    explicit gc.collect runs while the GC is disabled); enter no_gc() first so that the capture has
    ended before collection is enabled again, as CapturedOp does."""
    enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if enabled:
            gc.enable()


class CapturedOp:
    """v -> fn(v), replayed from a hipGraph when one could be captured: the package's one capture path (the line
    solves of both directions and the four Schur operators).  `graph` is the hipGraph or None (eager), `x` and `out`
    its input and output buffers: op(v) copies v into x, replays and returns a clone of out (v is left alone); a
    caller may instead fill views of x, replay `graph` and read views of out itself.

    Nothing is captured, and `agree` is never called, unless `capture` is true and the device is a GPU.  Otherwise:
    x (float64, `shape`) is filled with a probe seeded by `seed`; fn(x) runs once on a side stream (the warm-up outside
    the capture: library workspaces, lazily built tables, communicators), and its result is the eager reference; then
    fn(x) is captured on the current stream under no_gc().  A RuntimeError (the device libraries refuse) is followed by
    a synchronise and counts as not captured.  A capture executes no collective, so a rank whose capture fails
    desynchronises no other rank.
    agree(ok) -> bool, the same answer on every rank (parallel.all_agree), is for an fn with collectives in it, whose
    graph must be used by every rank or by none: agree(captured); if yes every rank copies the probe into x, replays
    (the collectives need every rank) and compares out with the warm-up's result in the relative max norm, and
    agree(error <= 1e-12) decides.  Without agree the graph is used as captured."""

    def __init__(self, device, fn, shape, *, capture=True, agree=None, seed=0):
        self.fn = fn
        self.graph = self.x = self.out = None
        device = torch.device(device)
        if not capture or device.type != "cuda":
            return
        self.x = torch.rand(shape, dtype=torch.float64, device=device,
                            generator=torch.Generator(device=device).manual_seed(seed))
        probe = self.x.clone()
        # The error mode of every capture is decided here.  A process group's watchdog thread (ProcessGroupNCCL) polls
        # the events of earlier collectives -- the warm-up's -- while this thread captures; in "global" mode another
        # thread's HIP call during a capture is an error that ends the process, in "thread_local" mode it is not.
        pg = torch.distributed.is_available() and torch.distributed.is_initialized()
        cur = torch.cuda.current_stream(device)
        side = torch.cuda.Stream(device)
        side.wait_stream(cur)
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.stream(side):
                want = fn(self.x)
            cur.wait_stream(side)
            with no_gc(), torch.cuda.graph(g, capture_error_mode="thread_local" if pg else "global"):
                out = fn(self.x)
            ok = True
        except RuntimeError:
            torch.cuda.synchronize(device)
            ok = False
        if agree is not None:
            ok = agree(ok)
            if ok:
                self.x.copy_(probe)
                g.replay()
                err = (out - want).abs().max() / want.abs().max().clamp(min=1e-300)
                ok = agree(bool(err <= 1e-12))
        if ok:
            self.graph, self.out = g, out

    def __call__(self, v):
        if self.graph is None:
            return self.fn(v)
        self.x.copy_(v)
        self.graph.replay()
        return self.out.clone()
