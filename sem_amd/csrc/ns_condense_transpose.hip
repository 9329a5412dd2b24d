// The transposed nested static condensation: y = A_II^-T r for every element column, from the factor the forward
// solve keeps (ns_condense.hip, lines 1-26: Xi, Aei, Yie column-major, the block-Thomas factors Ed, El, Eu of the
// edge Schur complement S_e = A_ee - A_ei Xi A_ie row-major) -- no transposed copy of any of them.  The adjoint
// solves of VelocityJacobianSolver(transpose=True) (sem_amd/solvers/velocity_solve.py: _nested_solve_T) run it in
// place of the reference's SuperLU transposed triangular solves.
//
//   K1t (one workgroup per element):  C = Yie^T r_i
//   K2t (one wavefront per column):   r_e[k] -= C[n=k][0:ne1] + C[n=k-1][ne1:],  then S_e^-T r_e by the transposed sweep
//                                       forward  w_k = r_k - Eu_{k-1}^T w_{k-1}
//                                       back     y_k = Ed_k^T (w_k - El_k^T y_{k+1}),   y_last = Ed_last^T w_last
//   K3t (one workgroup per element):  y_i = Xi^T (r_i - Aei^T [y_e(n); y_e(n+1)])
//
// A column-major block applied transposed is a set of dot products along contiguous memory (Yie^T: 2 ne1 stored
// rows of ni; Aei^T: ni rows of 2 ne1; Xi^T: ni rows of ni): L lanes share a stored row (L = 4 .. 64 from the row
// length), each lane sums its elements in increasing order into two accumulators, and the lanes meet in a butterfly
// of shuffles, so the order of summation is fixed by the shape (and by whether the rows are 16-byte aligned: then
// the loads are 16 bytes wide).  A row-major edge block applied transposed has the lane own an output column and
// walk the rows: every load is coalesced across the lanes, the rows are split over the two half-waves exactly as
// the forward sweep splits its columns, and the operands of the next D steps sit in the same register ring.
// The right-hand side is rhs() of the forward solve, the interface correction r = b - A_BI^T x_B being the forward
// one with aBI permuted into aIB's layout (the caller's aBIt).  Nothing is allocated: graph-capturable.
#include <hip/hip_runtime.h>

#include <string>

#include "cond_common.h"
#include "sem_internal.h"

namespace sem {

// lanes per stored row: at most four elements per lane up to rows of 256
__host__ __device__ constexpr int dot_lanes(int len) {
  return len <= 16 ? 4 : len <= 32 ? 8 : len <= 64 ? 16 : len <= 128 ? 32 : 64;
}

// out(row, <Mt[row], x>) for the nrows stored rows of length len at Mt (row r at Mt + r len), x in LDS, by the whole
// workgroup: 256 / L rows at a time, L lanes per row.  Every thread runs every pass (clamped rows are computed, not
// stored), so the shuffles are never divergent.  VEC: the rows and x are 16-byte aligned and len is even.
template <int L, bool VEC, typename Out>
__device__ __forceinline__ void rows_dot_l(const double* __restrict__ Mt, int nrows, int len, const double* x, Out out) {
  constexpr int G = kCondThreads / L;
  const int lane = threadIdx.x % L, grp = threadIdx.x / L;
  for (int r0 = 0; r0 < nrows; r0 += G) {
    const int row = r0 + grp;
    const double* p = Mt + static_cast<int64_t>(row < nrows ? row : nrows - 1) * len;
    double a0 = 0.0, a1 = 0.0;
    if constexpr (VEC) {
#pragma unroll 4
      for (int j = 2 * lane; j < len; j += 2 * L) {
        const double2 v = *reinterpret_cast<const double2*>(p + j);
        const double2 xv = *reinterpret_cast<const double2*>(x + j);
        a0 = fma(v.x, xv.x, a0);
        a1 = fma(v.y, xv.y, a1);
      }
    } else {
      int j = lane;
#pragma unroll 4
      for (; j + L < len; j += 2 * L) {
        a0 = fma(p[j], x[j], a0);
        a1 = fma(p[j + L], x[j + L], a1);
      }
      if (j < len) a0 = fma(p[j], x[j], a0);
    }
    double v = a0 + a1;
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0 && row < nrows) out(row, v);
  }
}

template <bool VEC, typename Out>
__device__ __forceinline__ void rows_dot_v(const double* Mt, int nrows, int len, const double* x, Out out) {
  switch (dot_lanes(len)) {  // workgroup-uniform
    case 4: rows_dot_l<4, VEC>(Mt, nrows, len, x, out); break;
    case 8: rows_dot_l<8, VEC>(Mt, nrows, len, x, out); break;
    case 16: rows_dot_l<16, VEC>(Mt, nrows, len, x, out); break;
    case 32: rows_dot_l<32, VEC>(Mt, nrows, len, x, out); break;
    default: rows_dot_l<64, VEC>(Mt, nrows, len, x, out); break;
  }
}

template <typename Out>
__device__ __forceinline__ void rows_dot(const double* Mt, int nrows, int len, const double* x, bool vec, Out out) {
  if (vec)
    rows_dot_v<true>(Mt, nrows, len, x, out);
  else
    rows_dot_v<false>(Mt, nrows, len, x, out);
}

// which factor arrays take 16-byte loads (host: base aligned and an even row length; blocks are whole rows apart)
enum { kVecYie = 1, kVecAei = 2, kVecXi = 4 };

// K1t: C = Yie^T r_i for element (e, n) = (blockIdx.x / ney, blockIdx.x % ney).
__global__ __launch_bounds__(kCondThreads) void cond_fwd_t_kernel(const CondArgs a, const int vec) {
  extern __shared__ double lds[];
  double* x = lds;  // ni: r_i
  const int el = blockIdx.x, e = el / a.ney, n = el - e * a.ney;
  const int64_t* pin = a.pi + static_cast<int64_t>(n) * a.ni;
  for (int i = threadIdx.x; i < a.ni; i += blockDim.x) x[i] = rhs(a, e, pin[i]);
  __syncthreads();
  const int G2 = 2 * a.ne1;
  const double* Yie = a.Yie + static_cast<int64_t>(el) * a.ni * G2;  // stored: 2 ne1 rows of ni
  double* C = a.C + static_cast<int64_t>(el) * G2;
  rows_dot(Yie, G2, a.ni, x, (vec & kVecYie) != 0, [&](int q, double v) { C[q] = v; });
}

// column j's entries of rows [h H, h H + H) of the row-major B x B block M: what lane (h, j) multiplies in M^T v.
// As load_half_row of the forward sweep, every lane issues the same loads from clamped addresses and nothing is
// computed from them here (see there for the compiler's wait counts); rows at or past B hold in-block values and
// meet zero partial sums in half_dot, columns past B are unused.
template <int B>
__device__ __forceinline__ void load_half_col(const double* __restrict__ M, int j, int h,
                                              double (&r)[EdgeThomas<B>::H]) {
  constexpr int H = EdgeThomas<B>::H;
  const int i0 = h * H, jc = j < B ? j : B - 1;
#pragma unroll
  for (int q = 0; q < H; ++q) {
    const int i = i0 + q, ic = i < B ? i : B - 1;
    r[q] = M[ic * B + jc];
  }
}

// K2t: the transposed block-Thomas sweep, one wavefront per column (grid = nex), templated on the block width
// B = ne1.  Lane (h, j) owns output column j over the rows [h H, h H + H) of a block; the two halves' partial sums
// of every vector meet in LDS, where each lane reads the pair sums of its own rows for the next product.
template <int B>
__global__ __launch_bounds__(64) void cond_edge_thomas_t_kernel(const CondArgs a) {
  constexpr int H = EdgeThomas<B>::H, D = EdgeThomas<B>::D;
  constexpr int64_t bb = static_cast<int64_t>(B) * B;
  __shared__ double pw[2][2 * H], pt[2][2 * H];  // [half][column] partial sums of w / y and of t
  const int e = blockIdx.x, nb = a.ney + 1, lane = threadIdx.x, j = lane & 31, h = lane >> 5, i0 = h * H;
  const bool col = j < B, own = col && h == 0;  // own: the lane that holds column j's value
  const double* C = a.C + static_cast<int64_t>(e) * a.ney * 2 * B;
  const double* Ed = a.Ed + static_cast<int64_t>(e) * nb * bb;
  const double* El = a.El + static_cast<int64_t>(e) * a.ney * bb;
  const double* Eu = a.Eu + static_cast<int64_t>(e) * a.ney * bb;
  double* Ye = a.Ye + static_cast<int64_t>(e) * a.n_e;
  double* Y = a.Y + e * a.ld_y;
  // edge offset of entry j of edge k: j = (l-1) nc + c  ->  (l-1) m + c N_y + k P  (VelocityJacobianSolver._pe)
  const int nc = B / (a.P - 1), NY = a.m / nc;
  const int jc = j < B ? j : B - 1;
  const int64_t off_j = static_cast<int64_t>(jc / nc) * a.m + static_cast<int64_t>(jc % nc) * NY;
  auto edge_off = [&](int k) { return off_j + static_cast<int64_t>(k) * a.P; };
  // the reduced edge right-hand side's terms, loaded raw into the ring exactly as the forward sweep loads them
  const bool coupled = a.aIB != nullptr;
  auto redge = [&](int k, EdgeRhs& q) {
    const int64_t o = off_j + static_cast<int64_t>(k) * a.P, l1 = o / a.m, r = o - l1 * a.m;
    const double* rp = a.R + e * a.ld_r + o;
    const double* ab = coupled ? a.aIB + ((static_cast<int64_t>(e) * (a.P - 1) + l1) * 2) * a.m + r : rp;
    const double* xb = coupled ? a.xB + static_cast<int64_t>(e) * a.m + r : rp;
    const int64_t am = coupled ? a.m : 0;
    const int kc0 = k < a.ney ? k : a.ney - 1, kc1 = k > 0 ? k - 1 : 0;
    q.r = *rp;
    q.a0 = ab[0];
    q.x0 = xb[0];
    q.a1 = ab[am];
    q.x1 = xb[am];
    q.c0 = C[static_cast<int64_t>(kc0) * 2 * B + jc];
    q.c1 = C[static_cast<int64_t>(kc1) * 2 * B + B + jc];
  };
  if (j >= 2 * H) return;  // no column and no row of this lane (B <= 2 H - 1 < 32); never reaches a barrier
  // ---- forward: w_k = r_k - Eu_{k-1}^T w_{k-1}, operands of steps k .. k+D-1 in the ring (slot k % D); whole
  // rounds refill unconditionally (past the last step: clamped, unused), the last nb % D steps run without refills
  double ru[D][H];
  EdgeRhs rr[D];
  auto load_fwd = [&](int k, int s) {
    const int kk = k < nb ? k : nb - 1;
    load_half_col<B>(Eu + (kk > 0 ? kk - 1 : 0) * bb, j, h, ru[s]);
    redge(kk, rr[s]);
  };
  auto fwd_step = [&](int k, int s) {
    double w = rr[s].value(own, coupled, k, a.ney);
    if (k > 0) w -= half_dot<H>(ru[s], &pw[0][i0], &pw[1][i0]);
    wave_lds_sync();
    pw[h][j] = col ? w : 0.0;
    wave_lds_sync();
    if (own) Ye[static_cast<int64_t>(k) * B + j] = pw[0][j] + pw[1][j];  // w_k, read back by the back sweep
  };
#pragma unroll
  for (int s = 0; s < D; ++s) load_fwd(s, s);
  int k0 = 0;
  for (; k0 + D <= nb; k0 += D) {
#pragma unroll
    for (int s = 0; s < D; ++s) {
      fwd_step(k0 + s, s);
      load_fwd(k0 + s + D, s);
    }
  }
#pragma unroll
  for (int s = 0; s < D - 1; ++s)
    if (k0 + s < nb) fwd_step(k0 + s, s);
  // ---- back: t = w_k - El_k^T y_{k+1}, y_k = Ed_k^T t; steps k = nb-1 .. 0, slot (nb-1-k) % D.  pw holds y_{k+1}
  // (as partial sums) from the second step on; the first step has no El term.
  double rl[D][H], rd[D][H], rw[D];
  auto load_back = [&](int k, int s) {
    const int kk = k > 0 ? k : 0, kl = kk < a.ney ? kk : a.ney - 1;
    load_half_col<B>(El + kl * bb, j, h, rl[s]);
    load_half_col<B>(Ed + kk * bb, j, h, rd[s]);
    rw[s] = Ye[static_cast<int64_t>(kk) * B + jc];
  };
  auto back_step = [&](int k, int s) {
    double t = own ? rw[s] : 0.0;
    if (k < nb - 1) t -= half_dot<H>(rl[s], &pw[0][i0], &pw[1][i0]);
    wave_lds_sync();
    pt[h][j] = col ? t : 0.0;
    wave_lds_sync();
    const double y = half_dot<H>(rd[s], &pt[0][i0], &pt[1][i0]);
    wave_lds_sync();
    pw[h][j] = col ? y : 0.0;
    wave_lds_sync();
    if (own) {
      const double v = pw[0][j] + pw[1][j];
      Ye[static_cast<int64_t>(k) * B + j] = v;
      Y[edge_off(k)] = v;
    }
  };
#pragma unroll
  for (int s = 0; s < D; ++s) load_back(nb - 1 - s, s);
  int c0 = 0;
  for (; c0 + D <= nb; c0 += D) {
#pragma unroll
    for (int s = 0; s < D; ++s) {
      back_step(nb - 1 - (c0 + s), s);
      load_back(nb - 1 - (c0 + s) - D, s);
    }
  }
#pragma unroll
  for (int s = 0; s < D - 1; ++s)
    if (c0 + s < nb) back_step(nb - 1 - (c0 + s), s);
}

template <int B>
static void launch_edge_thomas_t(const CondArgs& a, hipStream_t s) {
  if (a.ne1 == B)
    hipLaunchKernelGGL(cond_edge_thomas_t_kernel<B>, dim3(a.nex), dim3(64), 0, s, a);
  else if constexpr (B < kThomasB)
    launch_edge_thomas_t<B + 1>(a, s);
}

// K3t: y_i = Xi^T (r_i - Aei^T [y_e(n); y_e(n+1)]) for element (e, n), written to the element's interior nodes.
__global__ __launch_bounds__(kCondThreads) void cond_back_t_kernel(const CondArgs a, const int vec) {
  extern __shared__ double lds[];
  double* x = lds;                          // ni: r_i, then s = r_i - Aei^T y_e
  double* ye = lds + ((a.ni + 1) & ~1);     // 2 ne1: edges n, n+1 (contiguous in Ye); 16-byte aligned
  const int el = blockIdx.x, e = el / a.ney, n = el - e * a.ney, G2 = 2 * a.ne1;
  const int64_t* pin = a.pi + static_cast<int64_t>(n) * a.ni;
  for (int i = threadIdx.x; i < a.ni; i += blockDim.x) x[i] = rhs(a, e, pin[i]);
  const double* src = a.Ye + static_cast<int64_t>(e) * a.n_e + static_cast<int64_t>(n) * a.ne1;
  for (int i = threadIdx.x; i < G2; i += blockDim.x) ye[i] = src[i];
  __syncthreads();
  const double* Aei = a.Aei + static_cast<int64_t>(el) * G2 * a.ni;  // stored: ni rows of 2 ne1
  rows_dot(Aei, a.ni, G2, ye, (vec & kVecAei) != 0, [&](int i, double v) { x[i] -= v; });  // x[i]: this thread's alone
  __syncthreads();
  const double* Xi = a.Xi + static_cast<int64_t>(el) * a.ni * a.ni;  // stored: ni rows of ni
  double* Y = a.Y + e * a.ld_y;
  rows_dot(Xi, a.ni, a.ni, x, (vec & kVecXi) != 0, [&](int r, double v) { Y[pin[r]] = v; });
}

}  // namespace sem

extern "C" {

int sem_nested_solve_t(const sem_nested_desc* d, const double* R, int64_t ld_r, const double* aBIt, const double* xB,
                       double* Y, int64_t ld_y, void* stream) {
  sem::CondArgs a;
  if (int st = sem::nested_args(d, R, ld_r, aBIt, xB, Y, ld_y, a)) return st;
  if (a.Se != nullptr)
    return sem::set_error(SEM_EUNSUPPORTED, "nested_solve_t: the dense edge inverse has no transposed kernel");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  auto aligned = [](const double* p) { return (reinterpret_cast<uintptr_t>(p) % 16) == 0; };
  const bool even = (a.ni % 2) == 0;
  const int vec = (even && aligned(a.Yie) ? sem::kVecYie : 0) | (aligned(a.Aei) ? sem::kVecAei : 0) |
                  (even && aligned(a.Xi) ? sem::kVecXi : 0);
  const unsigned elems = static_cast<unsigned>(a.nex) * a.ney;
  hipLaunchKernelGGL(sem::cond_fwd_t_kernel, dim3(elems), dim3(sem::kCondThreads), a.ni * sizeof(double), s, a, vec);
  if (int st = sem::launch_check("nested_solve_t fwd")) return st;
  sem::launch_edge_thomas_t<1>(a, s);
  if (int st = sem::launch_check("nested_solve_t edge")) return st;
  hipLaunchKernelGGL(sem::cond_back_t_kernel, dim3(elems), dim3(sem::kCondThreads),
                     (((a.ni + 1) & ~1) + 2 * a.ne1) * sizeof(double), s, a, vec);
  return sem::launch_check("nested_solve_t back");
}

}  // extern "C"
