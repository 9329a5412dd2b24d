// Transposed nested-dissection solve J^T x = b (sem_amd/solvers/nested_dissection.py, _build_steps_T): the
// reverse-mode twin of the reference's SuperLU triangular solves (NavierStokes_Solver.py:189-203), from the factor
// the forward solve stores -- no transposed copies of the operators.
//
// sem_front_gemv_t: one level of y_f = A_f^T x_f in ONE launch from the row-major A_f (R_f operand rows, K_f
// output columns).  A workgroup takes 2 LC columns of one item and one part of its rows: LC lanes run along the
// contiguous columns (a 16-byte non-temporal load per lane and row: each operator is read once), the 256 / LC row
// groups of the workgroup stride over the part's rows, whose operands W[xidx[.]] sit in LDS.  Each thread sums its
// rows in increasing order; the row groups are summed in increasing order through LDS; with nparts > 1 the parts'
// sums go to a partials buffer and front_gemv_t_reduce adds them in increasing part order.  No atomics: bitwise
// repeatable.
// sem_leaf_sparse_t: the dense leaves' W[i] -= A_bi^T x_b on A_bi's pattern read the other way.
// sem_leaf_transpose: the split leaves' W[i] = A_ii^-T (W[i] - A_bi^T x_b) from sem_leaf_forward's blobs.
#include <hip/hip_runtime.h>

#include <string>

#include "sem_internal.h"

namespace sem {

using dvec2t = double __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double2 load_nt2t(const double* p) {
  const dvec2t v = __builtin_nontemporal_load(reinterpret_cast<const dvec2t*>(p));
  return make_double2(v.x, v.y);
}

__device__ __forceinline__ void gemv_t_finish(const sem_front_t_launch& a, int f, int c, double v) {
  if (a.back) {
    const int p = a.yidx[a.yoff[f] + c];
    a.W[p] -= v;
  } else {
    a.stage[a.yoff[f] + c] = v;
  }
}

// LC lanes per column tile (2 LC columns), RG = 256 / LC row groups, U rows of a group in flight.
template <int LC, int U>
__global__ __launch_bounds__(256) void front_gemv_t_kernel(const sem_front_t_launch a) {
  constexpr int RG = 256 / LC;
  extern __shared__ double sh[];
  const int f = a.tiles[4 * blockIdx.x], c0 = a.tiles[4 * blockIdx.x + 1], part = a.tiles[4 * blockIdx.x + 2];
  const int R = a.dims[4 * f], K = a.dims[4 * f + 1], ld = a.dims[4 * f + 2];
  const int rp = (R + a.nparts - 1) / a.nparts;          // rows per part; the last parts may be short or empty
  const int r0 = min(R, part * rp), nr = min(R, r0 + rp) - r0;
  const int32_t* xi = a.xidx + a.xoff[f] + r0;
  for (int k = threadIdx.x; k < nr; k += 256) {
    const int p = xi[k];
    sh[k] = p >= 0 ? a.W[p] : 0.0;
  }
  __syncthreads();
  const int cl = threadIdx.x % LC, g = threadIdx.x / LC;
  const int c = c0 + 2 * cl;                               // K is even: a pair is inside the row or beyond it
  double acc0 = 0.0, acc1 = 0.0;
  if (c < K) {
    const double* A = reinterpret_cast<const double*>(a.op[f]) + static_cast<int64_t>(r0) * ld + c;
    int r = g;
    for (; r + RG * (U - 1) < nr; r += RG * U) {
      double2 av[U];
#pragma unroll
      for (int t = 0; t < U; ++t) av[t] = load_nt2t(A + static_cast<int64_t>(r + RG * t) * ld);
#pragma unroll
      for (int t = 0; t < U; ++t) {
        const double x = sh[r + RG * t];
        acc0 = fma(av[t].x, x, acc0);
        acc1 = fma(av[t].y, x, acc1);
      }
    }
    for (; r < nr; r += RG) {                              // the group's last < U rows, same order
      const double2 av = load_nt2t(A + static_cast<int64_t>(r) * ld);
      const double x = sh[r];
      acc0 = fma(av.x, x, acc0);
      acc1 = fma(av.y, x, acc1);
    }
  }
  __syncthreads();                                         // the operands are dead: the row groups' sums take their place
  sh[g * 2 * LC + 2 * cl] = acc0;
  sh[g * 2 * LC + 2 * cl + 1] = acc1;
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 2 * LC && c0 + t < K) {
    double v = sh[t];
#pragma unroll 4
    for (int q = 1; q < RG; ++q) v += sh[q * 2 * LC + t];
    if (a.nparts == 1)
      gemv_t_finish(a, f, c0 + t, v);
    else
      a.partials[a.poff[f] + static_cast<int64_t>(part) * K + c0 + t] = v;
  }
}

// nparts > 1: the same tiles; the workgroups of part 0 add the parts of their columns in increasing part order.
__global__ __launch_bounds__(256) void front_gemv_t_reduce(const sem_front_t_launch a) {
  const int f = a.tiles[4 * blockIdx.x], c0 = a.tiles[4 * blockIdx.x + 1], part = a.tiles[4 * blockIdx.x + 2];
  if (part != 0) return;
  const int K = a.dims[4 * f + 1];
  const int t = threadIdx.x;
  if (t >= 2 * a.lanes || c0 + t >= K) return;
  const double* p = a.partials + a.poff[f] + c0 + t;
  double v = p[0];
  for (int q = 1; q < a.nparts; ++q) v += p[static_cast<int64_t>(q) * K];
  gemv_t_finish(a, f, c0 + t, v);
}

// sum_j coef[ipat[j ni + k]] x_b[brow[j ni + k]], j = 0..3 in order (ipat = -1: no coupling; x_b = 0 where
// bidx = -1): interior unknown k's share of A_bi^T x_b.
__device__ __forceinline__ double sparse_t(const double* coef, const int32_t* ipat, const int32_t* brow,
                                           const int32_t* bidx, const double* W, int ni, int k) {
  double v = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ci = ipat[j * ni + k];
    if (ci < 0) continue;
    const int p = bidx[brow[j * ni + k]];
    if (p >= 0) v = fma(coef[ci], W[p], v);
  }
  return v;
}

__global__ __launch_bounds__(256) void leaf_sparse_t_kernel(int nelem, int ni, int nb, const double* __restrict__ coef,
                                                            int64_t cstride, const int32_t* __restrict__ ipat,
                                                            const int32_t* __restrict__ brow,
                                                            const int32_t* __restrict__ iidx,
                                                            const int32_t* __restrict__ bidx, double* W) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= static_cast<int64_t>(nelem) * ni) return;
  const int64_t e = t / ni;
  const int k = static_cast<int>(t - e * ni);
  const int p = iidx[t];
  // the boundary entries read here are no launch's targets (interior entries only are written)
  W[p] -= sparse_t(coef + e * cstride, ipat, brow, bidx + e * nb, W, ni, k);
}

// sem_leaf_transpose: one workgroup per element, the register fragment of sem_leaf_forward -- thread (rs = tid / 8,
// s = tid % 8) holds rows rs + 32 k (k < RK) and column pairs s + 8 u (u < 2 RK).  A transposed product sums over
// the fragment's rows: the thread adds its RK rows (k in order) into partials for its own 4 RK columns, the 32 row
// groups' partials go through LDS and column c's thread adds them in rs order.
template <int NR, int NU>
__device__ __forceinline__ void leaf_load_t(double2 (&f)[NR][NU], const double* A, int n, int ld, int rs, int s) {
#pragma unroll
  for (int k = 0; k < NR; ++k)
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int r = rs + 32 * k, c = 2 * (s + 8 * u);
      f[k][u] = (r < n && c < n) ? load_nt2t(A + static_cast<int64_t>(r) * ld + c) : make_double2(0.0, 0.0);
    }
}

// part[u] += sum_k f[k][u] x[rs + 32 (k0 + k)]
template <int NR, int NU>
__device__ __forceinline__ void leaf_cols(const double2 (&f)[NR][NU], const double* x, int rs, int k0,
                                          double2 (&part)[NU]) {
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const double xv = x[rs + 32 * (k0 + k)];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      part[u].x = fma(f[k][u].x, xv, part[u].x);
      part[u].y = fma(f[k][u].y, xv, part[u].y);
    }
  }
}

// out[c] = sum over the 32 row groups, c < n; the slots from n on stay zero (they are operands of the next product)
template <int NU, int NX>
__device__ __forceinline__ void leaf_reduce(double2 (&part)[NU], double2* red, double* out, int n, int rs, int s,
                                            int tid, bool subtract) {
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    red[rs * (NX / 2) + s + 8 * u] = part[u];
    part[u] = make_double2(0.0, 0.0);
  }
  __syncthreads();
  const double* r = reinterpret_cast<const double*>(red);
  if (tid < n) {
    double v = r[tid];
#pragma unroll 8
    for (int q = 1; q < 32; ++q) v += r[q * NX + tid];
    out[tid] = subtract ? out[tid] - v : v;
  }
  __syncthreads();
}

// KH rows of S_v^-1 tiles per load batch.  RK = 4 takes one, in a loop that is NOT unrolled: unrolled, the scheduler
// issues every batch's loads at once and, beside A_uu^-1's 128 registers and the 32 of the column partials, spills
// (256 VGPRs, 68 bytes of scratch per lane); rolled, 208 VGPRs and no scratch.
template <int RK, int KH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void leaf_transpose_kernel(
    const sem_leaf_t_launch a) {
  constexpr int NX = 32 * RK;   // operand / output slots: every row and every column a thread touches
  __shared__ double ru[NX], rv[NX], tt[NX], zv[NX];
  __shared__ double2 red[32 * (NX / 2)];
  const int e = blockIdx.x, n = a.n, ld = a.ld;
  const double* Au = a.blob + static_cast<int64_t>(e) * a.stride;
  const double* Sv = Au + static_cast<int64_t>(n) * ld;
  const double* d1 = Sv + static_cast<int64_t>(n) * ld;
  const double* d2 = d1 + ld;
  const double* coef = d2 + ld;
  const int tid = threadIdx.x, s = tid & 7, rs = tid >> 3;
  double2 fa[RK][2 * RK], fs[KH][2 * RK], part[2 * RK];
  leaf_load_t<RK, 2 * RK>(fa, Au, n, ld, rs, s);           // in flight while the right-hand side is formed
  leaf_load_t<KH, 2 * RK>(fs, Sv, n, ld, rs, s);
#pragma unroll
  for (int u = 0; u < 2 * RK; ++u) part[u] = make_double2(0.0, 0.0);
  const int32_t* ix = a.iidx + static_cast<int64_t>(e) * 2 * n;
  const int32_t* bx = a.bidx + static_cast<int64_t>(e) * a.nb;
  for (int k = tid; k < 2 * NX; k += 256) {                // r = b_i - A_bi^T x_b, [u; v], zero beyond n
    const int c = k < NX ? k : k - NX;
    double v = 0.0;
    if (c < n) {
      const int kk = k < NX ? c : n + c;
      v = a.W[ix[kk]] - sparse_t(coef, a.ipat, a.brow, bx, a.W, 2 * n, kk);
    }
    (k < NX ? ru : rv)[c] = v;
    (k < NX ? tt : zv)[c] = 0.0;
  }
  __syncthreads();
  leaf_cols<RK, 2 * RK>(fa, ru, rs, 0, part);              // t = A_uu^-T r_u
  leaf_reduce<2 * RK, NX>(part, red, tt, n, rs, s, tid, false);
  if (tid < n) rv[tid] -= d1[tid] * tt[tid];               // r_v - D1 t
  __syncthreads();
#pragma unroll 1
  for (int h = 0; h < RK; h += KH) {                       // z_v = S_v^-T (r_v - D1 t), KH rows of tiles at a time
    if (h) leaf_load_t<KH, 2 * RK>(fs, Sv, n, ld, rs + 32 * h, s);
    leaf_cols<KH, 2 * RK>(fs, rv, rs, h, part);
  }
  leaf_reduce<2 * RK, NX>(part, red, zv, n, rs, s, tid, false);
  if (tid < n) ru[tid] = d2[tid] * zv[tid];                // D2 z_v
  __syncthreads();
  leaf_cols<RK, 2 * RK>(fa, ru, rs, 0, part);              // z_u = t - A_uu^-T (D2 z_v)
  leaf_reduce<2 * RK, NX>(part, red, tt, n, rs, s, tid, true);
  for (int k = tid; k < n; k += 256) {
    a.W[ix[k]] = tt[k];
    a.W[ix[n + k]] = zv[k];
  }
}

}  // namespace sem

extern "C" {

int sem_front_gemv_t(const sem_front_t_launch* d, void* stream) {
  if (!d) return sem::set_error(SEM_EINVAL, "front_gemv_t: null descriptor");
  if (d->ntiles < 0 || d->kmax < 0 || d->nparts < 1 || d->nparts > SEM_FRONT_T_MAX_PARTS)
    return sem::set_error(SEM_EINVAL, "front_gemv_t: bad sizes (1 <= nparts <= 16)");
  if (d->ntiles == 0) return SEM_OK;
  if (!d->op || !d->dims || !d->xoff || !d->yoff || !d->tiles || !d->xidx || !d->W ||
      (d->back ? !d->yidx : !d->stage) || (d->nparts > 1 && (!d->poff || !d->partials)))
    return sem::set_error(SEM_EINVAL, "front_gemv_t: null argument");
  if (d->kmax > 8192) return sem::set_error(SEM_EUNSUPPORTED, "front_gemv_t: more than 8192 operands per front");
  const size_t rows = (static_cast<size_t>(d->kmax) + d->nparts - 1) / d->nparts;
  const size_t lds = (rows > 512 ? rows : 512) * sizeof(double);   // the part's operands, then 256 x 2 sums
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(d->ntiles), block(256);
#define SEM_FRONT_T_CASE(L)                                                          \
  if (d->lanes == L) {                                                               \
    hipLaunchKernelGGL((sem::front_gemv_t_kernel<L, 4>), grid, block, lds, s, *d);   \
  } else
  SEM_FRONT_T_CASE(64) SEM_FRONT_T_CASE(32) SEM_FRONT_T_CASE(16) SEM_FRONT_T_CASE(8) SEM_FRONT_T_CASE(4) {
    return sem::set_error(SEM_EINVAL, "front_gemv_t: lanes must be 64, 32, 16, 8 or 4");
  }
#undef SEM_FRONT_T_CASE
  if (d->nparts > 1) hipLaunchKernelGGL(sem::front_gemv_t_reduce, grid, block, 0, s, *d);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return sem::set_error(SEM_EHIP, std::string("front_gemv_t launch: ") + hipGetErrorString(e));
  return SEM_OK;
}

int sem_leaf_sparse_t(int nelem, int ni, int nb, const double* coef, int64_t cstride, const int32_t* ipat,
                      const int32_t* brow, const int32_t* iidx, const int32_t* bidx, double* W, void* stream) {
  if (nelem < 0 || ni < 0 || nb < 0 || cstride < 0) return sem::set_error(SEM_EINVAL, "leaf_sparse_t: bad sizes");
  const int64_t n = static_cast<int64_t>(nelem) * ni;
  if (n == 0) return SEM_OK;
  if (!coef || !ipat || !brow || !iidx || !bidx || !W) return sem::set_error(SEM_EINVAL, "leaf_sparse_t: null argument");
  hipLaunchKernelGGL(sem::leaf_sparse_t_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), nelem, ni, nb, coef, cstride, ipat, brow, iidx, bidx, W);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return sem::set_error(SEM_EHIP, std::string("leaf_sparse_t launch: ") + hipGetErrorString(e));
  return SEM_OK;
}

int sem_leaf_transpose(const sem_leaf_t_launch* d, void* stream) {
  if (!d) return sem::set_error(SEM_EINVAL, "leaf_transpose: null descriptor");
  if (d->nelem < 0 || d->n < 1 || d->n > 121 || d->ld < d->n || d->ld % 2 || d->nb < 0 || d->nnz < 0 ||
      d->stride < 2 * static_cast<int64_t>(d->n) * d->ld + 2 * d->ld + static_cast<int64_t>(d->nnz) * d->nb ||
      d->stride % 2)
    return sem::set_error(SEM_EINVAL, "leaf_transpose: bad sizes (n <= 121, ld even >= n, stride even >= the blob)");
  if (d->nelem == 0) return SEM_OK;
  if (!d->blob || !d->iidx || !d->bidx || !d->ipat || !d->brow || !d->W)
    return sem::set_error(SEM_EINVAL, "leaf_transpose: null argument");
  if (reinterpret_cast<uintptr_t>(d->blob) % 16)
    return sem::set_error(SEM_EINVAL, "leaf_transpose: blob not 16-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(d->nelem), block(256);
  const int rk = (d->n + 32) / 32;   // sem_leaf_forward's register tiles
  if (rk == 1)
    hipLaunchKernelGGL((sem::leaf_transpose_kernel<1, 1>), grid, block, 0, s, *d);
  else if (rk == 2)
    hipLaunchKernelGGL((sem::leaf_transpose_kernel<2, 2>), grid, block, 0, s, *d);
  else if (rk == 3)
    hipLaunchKernelGGL((sem::leaf_transpose_kernel<3, 3>), grid, block, 0, s, *d);
  else
    hipLaunchKernelGGL((sem::leaf_transpose_kernel<4, 1>), grid, block, 0, s, *d);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return sem::set_error(SEM_EHIP, std::string("leaf_transpose launch: ") + hipGetErrorString(e));
  return SEM_OK;
}

}  // extern "C"
