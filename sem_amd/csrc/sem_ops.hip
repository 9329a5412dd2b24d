// libsemops: the C ABI of the SEM operator layer for MI355X (gfx950) and its small grid-stride kernels
// (gather, direct-stiffness sum, interface pack / unpack, interpolation and its transpose).  The apply kernels
// live in apply_tp.hip, apply_band.hip and apply_transpose.hip; apply_select.h picks among them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "apply_common.h"
#include "apply_select.h"

namespace sem {

// --------------------------------------------------------------------------- gather / DSS

__global__ void gather_kernel(const double* __restrict__ u, double* __restrict__ ue, int P, int ney, int ex_begin,
                              int64_t line_begin, int64_t NY, int64_t total) {
  const int n = P + 1;
  for (int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; t < total;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int j = static_cast<int>(t % n);
    int64_t r = t / n;
    const int i = static_cast<int>(r % n);
    r /= n;
    const int ne = static_cast<int>(r % ney);
    const int64_t me = r / ney + ex_begin;
    const int64_t gx = me * P + i, gy = static_cast<int64_t>(ne) * P + j;
    ue[t] = u[(gx - line_begin) * NY + gy];
  }
}

__global__ void dss_kernel(const double* __restrict__ ae, double* __restrict__ out, int P, int ney, int ex_begin,
                           int ex_end, int64_t line_begin, int64_t NY, int64_t total) {
  const int n = P + 1;
  for (int64_t p = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; p < total;
       p += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t gx = line_begin + p / NY, gy = p % NY;
    // candidate (element, local index) pairs, in increasing element order
    int64_t mc[2], ic[2], nc[2], jc[2];
    int nm = 0, nn = 0;
    const int64_t mx = gx / P, ix = gx - mx * P;
    if (ix == 0 && mx - 1 >= ex_begin && mx - 1 < ex_end) { mc[nm] = mx - 1; ic[nm++] = P; }
    if (mx >= ex_begin && mx < ex_end) { mc[nm] = mx; ic[nm++] = ix; }
    const int64_t my = gy / P, jy = gy - my * P;
    if (jy == 0 && my - 1 >= 0) { nc[nn] = my - 1; jc[nn++] = P; }
    if (my < ney) { nc[nn] = my; jc[nn++] = jy; }
    double s = 0.0;
    for (int a = 0; a < nm; ++a)
      for (int b = 0; b < nn; ++b)
        s += ae[(((mc[a] - ex_begin) * ney + nc[b]) * n + ic[a]) * n + jc[b]];
    out[p] = s;
  }
}

__global__ void iface_pack_kernel(const double* __restrict__ y, double* __restrict__ buf, int64_t NY, int nslots,
                                  int left_slot, int64_t left_off, int right_slot, int64_t right_off) {
  const int64_t total = static_cast<int64_t>(nslots) * NY;
  for (int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; t < total;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int s = static_cast<int>(t / NY);
    const int64_t c = t - s * NY;
    double v = 0.0;
    if (s == left_slot) v = y[left_off + c];
    if (s == right_slot) v = y[right_off + c];
    buf[t] = v;
  }
}

__global__ void iface_unpack_kernel(const double* __restrict__ buf, double* __restrict__ y, int64_t NY, int left_slot,
                                    int64_t left_off, int right_slot, int64_t right_off) {
  for (int64_t c = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; c < NY;
       c += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    if (left_slot >= 0) y[left_off + c] = buf[left_slot * NY + c];
    if (right_slot >= 0) y[right_off + c] = buf[right_slot * NY + c];
  }
}

// The line-layout twins of the two kernels above: Y holds the handle's lines with row pitch `pitch`, the two interface
// lines at offsets 0 and right_off; n entries per line are exchanged, the in-line offsets cols[0..n) (cols == nullptr:
// 0..n-1, the whole line -- every component of a [u | v] line in the one launch).
__global__ void iface_pack_lines_kernel(const double* __restrict__ Y, double* __restrict__ buf, int64_t n,
                                        const int* __restrict__ cols, int nslots, int left_slot, int right_slot,
                                        int64_t right_off) {
  const int64_t total = static_cast<int64_t>(nslots) * n;
  for (int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; t < total;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int s = static_cast<int>(t / n);
    const int64_t c = t - s * n;
    const int64_t off = cols ? cols[c] : c;
    double v = 0.0;
    if (s == left_slot) v = Y[off];
    if (s == right_slot) v = Y[right_off + off];
    buf[t] = v;
  }
}

__global__ void iface_unpack_lines_kernel(const double* __restrict__ buf, double* __restrict__ Y, int64_t n,
                                          const int* __restrict__ cols, int left_slot, int right_slot,
                                          int64_t right_off) {
  for (int64_t c = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; c < n;
       c += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t off = cols ? cols[c] : c;
    if (left_slot >= 0) Y[off] = buf[left_slot * n + c];
    if (right_slot >= 0) Y[right_off + off] = buf[right_slot * n + c];
  }
}

// SEM.eval_interpolation (SEM.py:248-273): out[a][b] = sum_kl Sx[a][k] u_e[m_a][n_b][k][l] Sy[b][l]
// for plot rows a (element m_a, evaluation row Sx[a]) and plot columns b; points whose element
// index is negative (outside the mesh) are left untouched, like the reference's np.place.
__global__ void interp_kernel(const double* __restrict__ ue, int P, int ney, int ex_begin, int ex_end,
                              const int* __restrict__ mi, const double* __restrict__ Sx, int na,
                              const int* __restrict__ ni, const double* __restrict__ Sy, int nb,
                              double* __restrict__ out) {
  const int n = P + 1;
  const int64_t total = static_cast<int64_t>(na) * nb;
  for (int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; t < total;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int a = static_cast<int>(t / nb), b = static_cast<int>(t - static_cast<int64_t>(a) * nb);
    const int m = mi[a], e = ni[b];
    if (m < ex_begin || m >= ex_end || e < 0 || e >= ney) continue;
    const double* u = ue + (static_cast<int64_t>(m - ex_begin) * ney + e) * n * n;
    double s = 0.0;
    for (int k = 0; k < n; ++k) {
      double r = 0.0;
      for (int l = 0; l < n; ++l) r = fma(u[k * n + l], Sy[static_cast<int64_t>(b) * n + l], r);
      s = fma(Sx[static_cast<int64_t>(a) * n + k], r, s);
    }
    out[t] = s;
  }
}

// Transpose of interp_kernel with respect to u_e: one thread per entry (m, n, k, l) of u_e_bar sums the plot
// rows of element column m (a_list, ascending) and the plot columns of element row n (b_list, ascending).
__global__ void interp_adjoint_kernel(const double* __restrict__ ob, int P, int ney, const int* __restrict__ ap,
                                      const int* __restrict__ al, const double* __restrict__ Sx,
                                      const int* __restrict__ bp, const int* __restrict__ bl,
                                      const double* __restrict__ Sy, int nb, double* __restrict__ ueb, int64_t total) {
  const int n = P + 1;
  for (int64_t t = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; t < total;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int l = static_cast<int>(t % n), k = static_cast<int>((t / n) % n);
    const int64_t el = t / (n * n);
    const int e = static_cast<int>(el % ney), m = static_cast<int>(el / ney);
    double s = 0.0;
    for (int ia = ap[m]; ia < ap[m + 1]; ++ia) {
      const int a = al[ia];
      double r = 0.0;
      for (int ib = bp[e]; ib < bp[e + 1]; ++ib) {
        const int b = bl[ib];
        r = fma(Sy[static_cast<int64_t>(b) * n + l], ob[static_cast<int64_t>(a) * nb + b], r);
      }
      s = fma(Sx[static_cast<int64_t>(a) * n + k], r, s);
    }
    ueb[t] = s;
  }
}

static unsigned grid_for(int64_t total, int threads) {
  int64_t g = (total + threads - 1) / threads;
  return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(g, 65536)));
}

}  // namespace sem

// =========================================================================== C ABI
using namespace sem;

// Every launcher runs on the handle's device: a handle used while another device is current
// would launch there against this device's pointers, so it is an error (SEM_EINVAL).
static int on_device(const sem_handle* h) {
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess) return sem::set_error(SEM_EHIP, "hipGetDevice failed");
  if (cur != h->device)
    return sem::set_error(SEM_EINVAL, "handle belongs to device " + std::to_string(h->device) + " but device " +
                                          std::to_string(cur) + " is current");
  return SEM_OK;
}

extern "C" {

int sem_abi_version(void) { return SEM_ABI_VERSION; }

static bool retired_knob(int knob) {
  return knob == SEM_TUNE_RETIRED_1 || knob == SEM_TUNE_RETIRED_3 || knob == SEM_TUNE_RETIRED_5 ||
         (knob >= SEM_TUNE_RETIRED_8 && knob <= SEM_TUNE_RETIRED_12);
}

int sem_set_tuning(int knob, int value) {
  if (knob < 0 || knob >= SEM_TUNE_COUNT) return set_error(SEM_EINVAL, "unknown tuning knob");
  if (retired_knob(knob)) return set_error(SEM_EINVAL, "retired tuning knob (round 6)");
  tuning().v[knob] = value;
  return SEM_OK;
}

int sem_get_tuning(int knob, int* value) {
  if (knob < 0 || knob >= SEM_TUNE_COUNT || !value) return set_error(SEM_EINVAL, "unknown tuning knob");
  *value = tuning().v[knob];
  return SEM_OK;
}
const char* sem_last_error(void) { return last_error(); }
int sem_max_order(void) { return kMaxOrder; }

int sem_gll_nodes(int P, double* xi, double* w, double* V) { return gll_nodes(P, xi, w, V); }
int sem_gll_differentiation(int P, double* D) {
  if (!D) return set_error(SEM_EINVAL, "null output");
  return gll_differentiation(P, D);
}
int sem_gll_gradient(int P, double* G) {
  if (!G) return set_error(SEM_EINVAL, "null output");
  return gll_gradient(P, G);
}
int sem_gll_stiffness(int P, double* K) {
  if (!K) return set_error(SEM_EINVAL, "null output");
  return gll_stiffness(P, K);
}
int sem_gll_evaluation(int P, const double* xe, int64_t count, double* S) {
  if (count < 0 || (count > 0 && (!xe || !S))) return set_error(SEM_EINVAL, "bad evaluation arguments");
  return gll_evaluation(P, xe, count, S);
}
int sem_global_index(int P, int nex, int ney, const int64_t* m, const int64_t* n, const int64_t* i, const int64_t* j,
                     int64_t count, int64_t* out) {
  if (count < 0 || (count > 0 && (!m || !n || !i || !j || !out))) return set_error(SEM_EINVAL, "bad index arguments");
  return global_index(P, nex, ney, m, n, i, j, count, out);
}

int sem_create(int P, int nex, int ney, double dx, double dy, int ex_begin, int ex_end, int device, sem_handle** out) {
  if (!out) return set_error(SEM_EINVAL, "null handle output");
  *out = nullptr;
  if (P < 1 || P > kMaxOrder) return set_error(SEM_EUNSUPPORTED, "polynomial order outside compiled range [1, 16]");
  if (nex < 1 || ney < 1) return set_error(SEM_EINVAL, "N_ex and N_ey must be positive");
  if (!(dx > 0.0) || !(dy > 0.0)) return set_error(SEM_EINVAL, "element widths must be positive");
  if (ex_begin < 0 || ex_end > nex || ex_begin >= ex_end) return set_error(SEM_EINVAL, "bad element-column range");
  const int n = P + 1;
  std::vector<double> tab(2 * n * n + n);
  int st = gll_stiffness(P, tab.data());
  if (!st) st = gll_gradient(P, tab.data() + n * n);
  if (!st) st = gll_nodes(P, nullptr, tab.data() + 2 * n * n, nullptr);
  if (st) return st;
  int prev = 0;
  if ((st = hip_check(hipGetDevice(&prev), "hipGetDevice"))) return st;
  if ((st = hip_check(hipSetDevice(device), "hipSetDevice"))) return st;
  double* d_tab = nullptr;
  hipError_t e = hipMalloc(&d_tab, tab.size() * sizeof(double));
  if (e != hipSuccess) {
    (void)hipSetDevice(prev);
    return set_error(SEM_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
  e = hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice);
  (void)hipSetDevice(prev);
  if (e != hipSuccess) {
    (void)hipFree(d_tab);
    return set_error(SEM_EHIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
  }
  sem_handle* h = new sem_handle;
  h->P = P;
  h->nex = nex;
  h->ney = ney;
  h->ex_begin = ex_begin;
  h->ex_end = ex_end;
  h->device = device;
  h->dx = dx;
  h->dy = dy;
  h->NX = static_cast<int64_t>(nex) * P + 1;
  h->NY = static_cast<int64_t>(ney) * P + 1;
  h->N = h->NX * h->NY;
  h->line_begin = static_cast<int64_t>(ex_begin) * P;
  h->line_end = static_cast<int64_t>(ex_end) * P;
  h->n_local = (h->line_end - h->line_begin + 1) * h->NY;
  h->d_tab = d_tab;
  *out = h;
  return SEM_OK;
}

int sem_destroy(sem_handle* h) {
  if (!h) return SEM_OK;
  int prev = 0;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(h->device);
  (void)hipFree(h->d_tab);
  (void)hipSetDevice(prev);
  delete h;
  return SEM_OK;
}

int sem_get_info(const sem_handle* h, sem_info* o) {
  if (!h || !o) return set_error(SEM_EINVAL, "null argument");
  o->P = h->P;
  o->nex = h->nex;
  o->ney = h->ney;
  o->ex_begin = h->ex_begin;
  o->ex_end = h->ex_end;
  o->device = h->device;
  o->dx = h->dx;
  o->dy = h->dy;
  o->NX = h->NX;
  o->NY = h->NY;
  o->N = h->N;
  o->line_begin = h->line_begin;
  o->line_end = h->line_end;
  o->n_local = h->n_local;
  o->dof_begin = h->line_begin * h->NY;
  return SEM_OK;
}

// The policy's view of a handle (apply_select.h).
static ApplyMesh mesh_of(const sem_handle* h) {
  return {h->P, h->nex, h->ney, h->ex_begin, h->ex_end, h->NY, h->n_local};
}

// The ApplyArgs fields sem_apply and sem_apply_transpose fill alike, from the handle and the descriptor.
static ApplyArgs common_args(const sem_handle* h, const sem_apply_desc* d, const double* x, double* y) {
  ApplyArgs a{};
  a.x = x;
  a.y = y;
  a.cu = d->cu;
  a.cv = d->cv;
  a.ea = d->ea;
  a.mask = d->dir_mask;
  a.cM = d->c_mass;
  a.cK = d->c_stiff;
  a.cX = d->c_gradx;
  a.cY = d->c_grady;
  a.cA = d->c_acc;
  a.sx = h->dy / h->dx;
  a.sy = h->dx / h->dy;
  a.hx = h->dx / 2.0;
  a.hy = h->dy / 2.0;
  a.hxy = (h->dx / 2.0) * (h->dy / 2.0);
  a.NY = h->NY;
  a.NXg = h->NX;
  a.line_begin = h->line_begin;
  a.line_end = h->line_end;
  a.nex = h->nex;
  a.ney = h->ney;
  a.ex_begin = h->ex_begin;
  a.ex_end = h->ex_end;
  a.dir_mode = d->dir_mode;
  a.sides = d->dir_sides;
  a.n_local32 = static_cast<int>(std::min<int64_t>(h->n_local, 0x7fffffff));
  return a;
}

int sem_apply(sem_handle* h, const sem_apply_desc* d, const double* x, double* y, void* stream) {
  if (!h || !d) return set_error(SEM_EINVAL, "null handle or descriptor");
  if (!x || !y) return set_error(SEM_EINVAL, "null x or y");
  if (x == y) return set_error(SEM_EINVAL, "x and y must not alias");
  if (d->dir_mode < SEM_DIR_NONE || d->dir_mode > SEM_DIR_REPLACE) return set_error(SEM_EINVAL, "bad dir_mode");
  if (d->dir_mode == SEM_DIR_REPLACE && !d->dir_val) return set_error(SEM_EINVAL, "SEM_DIR_REPLACE needs dir_val");
  const ApplyChoice c = select_apply(mesh_of(h), d->algo, d->pos_begin, d->pos_end, tune(SEM_TUNE_MFMA_TILE));
  if (c.status) return set_error(c.status, c.message);
  if (int st = on_device(h)) return st;
  ApplyArgs a = common_args(h, d, x, y);
  const bool ranged = d->pos_end > 0;
  a.pos0 = ranged ? d->pos_begin : 0;
  a.pos1 = ranged ? d->pos_end : 0;
  a.eb = d->eb;
  a.ec = d->ec;
  a.ed = d->ed;
  a.has_e1 = (d->c_extra != 0.0 && d->ea && d->eb) ? 1 : 0;
  a.has_e2 = (d->c_extra != 0.0 && d->ec && d->ed) ? 1 : 0;
  a.dval = d->dir_val;
  a.tab = h->d_tab;
  a.cE = d->c_extra;
  a.diag = kDiag ? diag_bits() : 0;
  a.stamps = (kDiag && (a.diag & 8)) ? diag_stamps() : nullptr;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch (c.kind) {
    case ApplyKind::Band:
      return launch_apply_band(a, h, s);
    case ApplyKind::BandMfma:
      return launch_apply_bmfma(a, h, s);
    case ApplyKind::ElemMfma:
      return launch_apply_emfma(a, h, s);
    case ApplyKind::Column:
      return launch_apply_col(a, h, s);
    default:
      return launch_apply_valu(a, h, s);
  }
}

// The argument checks sem_apply_transpose and sem_apply_transpose_part share (before the kernel selection).
static int transpose_args(const sem_handle* h, const sem_apply_desc* d, const double* z, const double* y) {
  if (!h || !d) return set_error(SEM_EINVAL, "null handle or descriptor");
  if (!z || !y) return set_error(SEM_EINVAL, "null z or y");
  if (z == y) return set_error(SEM_EINVAL, "z and y must not alias");
  if (d->dir_mode != SEM_DIR_NONE && d->dir_mode != SEM_DIR_IDENTITY)
    return set_error(SEM_EINVAL, "the transposed apply takes SEM_DIR_NONE or SEM_DIR_IDENTITY");
  if (d->eb || d->ec || d->ed) return set_error(SEM_EINVAL, "the transposed apply takes no eb / ec / ed (d = c_extra * ea)");
  if (d->dir_val) return set_error(SEM_EINVAL, "the transposed apply takes no dir_val");
  return SEM_OK;
}

int sem_apply_transpose(sem_handle* h, const sem_apply_desc* d, const double* z, double* y, void* stream) {
  if (int st = transpose_args(h, d, z, y)) return st;
  const ApplyChoice c = select_apply_transpose(mesh_of(h), d->algo, d->pos_end, kMaxOrder);
  if (c.status) return set_error(c.status, c.message);
  if (int st = on_device(h)) return st;
  ApplyArgs a = common_args(h, d, z, y);
  a.cE = d->ea ? d->c_extra : 0.0;
  return launch_apply_transpose(a, h, reinterpret_cast<hipStream_t>(stream));
}

int sem_apply_transpose_part(sem_handle* h, const sem_apply_desc* d, const double* z, double* y, void* stream) {
  if (int st = transpose_args(h, d, z, y)) return st;
  const ApplyChoice c = select_apply_transpose_part(mesh_of(h), d->algo, d->pos_begin, d->pos_end, kMaxOrder);
  if (c.status) return set_error(c.status, c.message);
  if (int st = on_device(h)) return st;
  ApplyArgs a = common_args(h, d, z, y);
  a.cE = d->ea ? d->c_extra : 0.0;
  a.pos0 = d->pos_begin;
  a.pos1 = d->pos_end;
  return launch_apply_transpose(a, h, reinterpret_cast<hipStream_t>(stream));
}

int sem_transpose_kernel_name(const sem_handle* h, char* buf, int len) {
  if (!h || !buf || len < 1) return set_error(SEM_EINVAL, "bad arguments");
  const std::string name = apply_kernel_name(ApplyKind::Transpose, mesh_of(h), 0, 0);
  std::snprintf(buf, static_cast<size_t>(len), "%s", name.c_str());
  return SEM_OK;
}

// The kernel sem_apply launches for (handle, algo) without a position range, or the status it refuses the pair with.
int sem_kernel_name(const sem_handle* h, int algo, char* buf, int len) {
  if (!h || !buf || len < 1) return set_error(SEM_EINVAL, "bad arguments");
  const ApplyChoice c = select_apply(mesh_of(h), algo, 0, 0, tune(SEM_TUNE_MFMA_TILE));
  if (c.status) return set_error(c.status, c.message);
  const std::string name =
      apply_kernel_name(c.kind, mesh_of(h), tune(SEM_TUNE_BAND_TILE), tune(SEM_TUNE_BAND_KP));
  std::snprintf(buf, static_cast<size_t>(len), "%s", name.c_str());
  return SEM_OK;
}

int sem_gather_elements(sem_handle* h, const double* u, double* ue, void* stream) {
  if (!h || !u || !ue) return set_error(SEM_EINVAL, "null argument");
  if (int st = on_device(h)) return st;
  const int n = h->P + 1;
  const int64_t total = static_cast<int64_t>(h->ex_end - h->ex_begin) * h->ney * n * n;
  hipLaunchKernelGGL(gather_kernel, dim3(grid_for(total, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), u,
                     ue, h->P, h->ney, h->ex_begin, h->line_begin, h->NY, total);
  return hip_check(hipGetLastError(), "gather launch");
}

int sem_dss(sem_handle* h, const double* ae, double* out, void* stream) {
  if (!h || !ae || !out) return set_error(SEM_EINVAL, "null argument");
  if (static_cast<const void*>(ae) == static_cast<const void*>(out)) return set_error(SEM_EINVAL, "in/out alias");
  if (int st = on_device(h)) return st;
  hipLaunchKernelGGL(dss_kernel, dim3(grid_for(h->n_local, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     ae, out, h->P, h->ney, h->ex_begin, h->ex_end, h->line_begin, h->NY, h->n_local);
  return hip_check(hipGetLastError(), "dss launch");
}

int sem_eval_interpolation(sem_handle* h, const double* ue, int na, const int* m_idx, const double* Sx, int nb,
                           const int* n_idx, const double* Sy, double* out, void* stream) {
  if (!h || !ue || !out || na < 0 || nb < 0) return set_error(SEM_EINVAL, "bad interpolation arguments");
  if (na == 0 || nb == 0) return SEM_OK;
  if (!m_idx || !Sx || !n_idx || !Sy) return set_error(SEM_EINVAL, "null interpolation table");
  if (int st = on_device(h)) return st;
  hipLaunchKernelGGL(interp_kernel, dim3(grid_for(static_cast<int64_t>(na) * nb, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), ue, h->P, h->ney, h->ex_begin, h->ex_end, m_idx, Sx, na,
                     n_idx, Sy, nb, out);
  return hip_check(hipGetLastError(), "interpolation launch");
}

int sem_eval_interpolation_adjoint(sem_handle* h, const double* out_bar, int na, const int* a_ptr, const int* a_list,
                                   const double* Sx, int nb, const int* b_ptr, const int* b_list, const double* Sy,
                                   double* u_e_bar, void* stream) {
  if (!h || !u_e_bar || na < 0 || nb < 0) return set_error(SEM_EINVAL, "bad interpolation arguments");
  if (!a_ptr || !b_ptr) return set_error(SEM_EINVAL, "null interpolation row / column list");  // empty lists may be null
  if ((na > 0 && nb > 0 && !out_bar) || (na > 0 && !Sx) || (nb > 0 && !Sy))
    return set_error(SEM_EINVAL, "null interpolation table");
  if (h->ex_begin != 0 || h->ex_end != h->nex)
    return set_error(SEM_EUNSUPPORTED, "the transposed interpolation is implemented for whole-mesh handles only");
  if (int st = on_device(h)) return st;
  const int n = h->P + 1;
  const int64_t total = static_cast<int64_t>(h->nex) * h->ney * n * n;
  hipLaunchKernelGGL(interp_adjoint_kernel, dim3(grid_for(total, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), out_bar, h->P, h->ney, a_ptr, a_list, Sx, b_ptr, b_list, Sy,
                     nb, u_e_bar, total);
  return hip_check(hipGetLastError(), "transposed interpolation launch");
}

static int iface_slots(const sem_handle* h, const int* bounds, int G, int* left, int* right) {
  if (!bounds || G < 1) return set_error(SEM_EINVAL, "bad partition");
  if (bounds[0] != 0 || bounds[G] != h->nex) return set_error(SEM_EINVAL, "partition must cover [0, N_ex]");
  int r = -1;
  for (int k = 0; k < G; ++k) {
    if (bounds[k] >= bounds[k + 1]) return set_error(SEM_EINVAL, "partition bounds must increase");
    if (bounds[k] == h->ex_begin && bounds[k + 1] == h->ex_end) r = k;
  }
  if (r < 0) return set_error(SEM_EINVAL, "handle's element range is not a part of the partition");
  *left = r > 0 ? r - 1 : -1;
  *right = r < G - 1 ? r : -1;
  return SEM_OK;
}

int sem_interface_pack(sem_handle* h, const double* y, const int* bounds, int G, double* buf, void* stream) {
  if (!h || !y || !buf) return set_error(SEM_EINVAL, "null argument");
  int L, R, st;
  if ((st = iface_slots(h, bounds, G, &L, &R))) return st;
  if (G < 2) return SEM_OK;
  if ((st = on_device(h))) return st;
  const int64_t total = static_cast<int64_t>(G - 1) * h->NY;
  hipLaunchKernelGGL(iface_pack_kernel, dim3(grid_for(total, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     y, buf, h->NY, G - 1, L, static_cast<int64_t>(0), R, h->n_local - h->NY);
  return hip_check(hipGetLastError(), "interface pack launch");
}

int sem_interface_unpack(sem_handle* h, const double* buf, const int* bounds, int G, double* y, void* stream) {
  if (!h || !y || !buf) return set_error(SEM_EINVAL, "null argument");
  int L, R, st;
  if ((st = iface_slots(h, bounds, G, &L, &R))) return st;
  if (G < 2) return SEM_OK;
  if ((st = on_device(h))) return st;
  hipLaunchKernelGGL(iface_unpack_kernel, dim3(grid_for(h->NY, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), buf, y, h->NY, L, static_cast<int64_t>(0), R,
                     h->n_local - h->NY);
  return hip_check(hipGetLastError(), "interface unpack launch");
}

// the checks the two line-layout entry points share; *n = entries exchanged per line, *right_off = the last line's offset
static int iface_lines_args(const sem_handle* h, const void* Y, const void* buf, int64_t width, int64_t pitch,
                            const int* cols, int ncols, const int* bounds, int G, int* left, int* right, int64_t* n,
                            int64_t* right_off) {
  if (!h || !Y || !buf) return set_error(SEM_EINVAL, "null argument");
  if (width < 1) return set_error(SEM_EINVAL, "interface lines: width must be at least 1");
  if (pitch < width) return set_error(SEM_EINVAL, "interface lines: pitch must be at least width");
  if (cols ? ncols < 1 : ncols != 0)
    return set_error(SEM_EINVAL, "interface lines: ncols must be >= 1 with a column list and 0 without one");
  if (int st = iface_slots(h, bounds, G, left, right)) return st;
  *n = cols ? ncols : width;
  *right_off = (h->line_end - h->line_begin) * pitch;   // line_end is the last line itself
  return SEM_OK;
}

int sem_interface_pack_lines(sem_handle* h, const double* Y, int64_t width, int64_t pitch, const int* cols, int ncols,
                             const int* bounds, int G, double* buf, void* stream) {
  int L, R, st;
  int64_t n, roff;
  if ((st = iface_lines_args(h, Y, buf, width, pitch, cols, ncols, bounds, G, &L, &R, &n, &roff))) return st;
  if (G < 2) return SEM_OK;
  if ((st = on_device(h))) return st;
  const int64_t total = static_cast<int64_t>(G - 1) * n;
  hipLaunchKernelGGL(iface_pack_lines_kernel, dim3(grid_for(total, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), Y, buf, n, cols, G - 1, L, R, roff);
  return hip_check(hipGetLastError(), "interface lines pack launch");
}

int sem_interface_unpack_lines(sem_handle* h, const double* buf, int64_t width, int64_t pitch, const int* cols,
                               int ncols, const int* bounds, int G, double* Y, void* stream) {
  int L, R, st;
  int64_t n, roff;
  if ((st = iface_lines_args(h, Y, buf, width, pitch, cols, ncols, bounds, G, &L, &R, &n, &roff))) return st;
  if (G < 2) return SEM_OK;
  if ((st = on_device(h))) return st;
  hipLaunchKernelGGL(iface_unpack_lines_kernel, dim3(grid_for(n, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), buf, Y, n, cols, L, R, roff);
  return hip_check(hipGetLastError(), "interface lines unpack launch");
}

}  // extern "C"
