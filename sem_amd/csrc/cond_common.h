// What the nested-condensation kernels share: the forward solve (ns_condense.hip) and its transposed twin
// (ns_condense_transpose.hip) read the same factor through the same argument block, form the same right-hand side
// and run the same half-split block-Thomas machinery.  Layouts: ns_condense.hip, lines 1-26.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "sem_internal.h"

namespace sem {

constexpr int kCondThreads = 256;

struct CondArgs {
  const double *Xi, *Aei, *Yie, *Se;
  const double *XiB, *AXB;     // ABI 11: Xi A_iB (ni x 2 ne1) and A_ei Xi A_iB (2 ne1 x 2 ne1) per element
  const double* ABY;           // ABI 11: A_Bi Xi A_ie (2 ne1 x 2 ne1) per element
  double* Pw;                  // ABI 11: per-column interface partial sums (nex, 2, m)
  const double* aBI;           // ABI 11 (sem_nested_iface_rhs): interface <- interior lines, (nex, 2, P-1, m)
  const double *Ed, *El, *Eu;  // block-Thomas factors of the edge Schur complement (Se == nullptr)
  const int64_t *pi, *pe;
  double *T, *C, *Ye;
  const double* R;     // column e interior at R + e ld_r (offset o)
  int64_t ld_r;
  const double* aIB;   // nullable: r -= aIB[e][l-1][0][r'] xB[e][r'] + aIB[e][l-1][1][r'] xB[e+1][r']
  const double* xB;    // (nex+1, m)
  double* Y;           // column e interior result at Y + e ld_y (offset o)
  int64_t ld_y;
  int P, nex, ney, m, ni, ne1, n_e;
};

// right-hand side at column offset o of column e (with the optional interface correction)
__device__ __forceinline__ double rhs(const CondArgs& a, int e, int64_t o) {
  double v = a.R[e * a.ld_r + o];
  if (a.aIB) {
    const int64_t l1 = o / a.m, r = o - l1 * a.m;
    const double* ab = a.aIB + ((static_cast<int64_t>(e) * (a.P - 1) + l1) * 2) * a.m + r;
    v -= ab[0] * a.xB[static_cast<int64_t>(e) * a.m + r] + ab[a.m] * a.xB[static_cast<int64_t>(e + 1) * a.m + r];
  }
  return v;
}

// LDS doubles colmajor_gemv needs for its split partial sums
__host__ __device__ constexpr int part_size() { return kCondThreads; }

constexpr int kThomasB = 32;  // largest ne1 (= nc (P-1)) of the block-Thomas form

template <int B>
struct EdgeThomas {
  static constexpr int H = B <= 1 ? 2 : (((B + 1) / 2 + 1) & ~1);  // columns per half-row (even)
  static constexpr bool VEC = (B % 2) == 0;                         // 16-byte aligned half-rows
  // steps loaded ahead: 3 (5-8, AGPR-backed, measured no faster at cfg5: 10.37 against 10.33 ms per velocity
  // solve, so the ~1.2 us per step is the chain of LDS round trips, barriers and FMAs, not memory latency)
  static constexpr int D = 3;
};

// LDS ordering inside a one-wave workgroup (round 4).  __syncthreads() is a workgroup release + acquire on
// every address space: after the sweep's global stores (Ye) it compiled to s_waitcnt vmcnt(0), i.e. it also
// waited for the loads the operand ring had issued steps ahead, so every step paid a full memory round trip
// (1.2 us per step, no faster with a deeper ring).  A wave's LDS operations execute in order; all the sweep
// needs is that the compiler keeps them in program order and that the writes have completed.
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// the terms of one edge row's reduced right-hand side, r - (a0 x0 + a1 x1) - c0 - c1 (rhs() and the two
// element couplings of edge k), as loaded; value() selects the present terms, in rhs()'s order of operations
struct EdgeRhs {
  double r, a0, x0, a1, x1, c0, c1;
  __device__ __forceinline__ double value(bool own, bool coupled, int k, int ney) const {
    double v = r;
    if (coupled) v -= a0 * x0 + a1 * x1;
    if (k < ney) v -= c0;
    if (k > 0) v -= c1;
    return own ? v : 0.0;
  }
};

// sum over this lane's columns of M-row * (p[0][j] + p[1][j]): the two halves' partial sums of the vector
template <int H>
__device__ __forceinline__ double half_dot(const double (&r)[H], const double* p0, const double* p1) {
  double a0 = 0.0, a1 = 0.0;
#pragma unroll
  for (int q = 0; q < H; q += 2) {
    a0 = fma(r[q], p0[q] + p1[q], a0);
    a1 = fma(r[q + 1], p0[q + 1] + p1[q + 1], a1);
  }
  return a0 + a1;
}

inline int launch_check(const char* what) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) return SEM_OK;
  return set_error(SEM_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// CondArgs of a nested solve from the descriptor (checks shared by every entry point; ns_condense.hip)
int nested_args(const sem_nested_desc* d, const double* R, int64_t ld_r, const double* aIB, const double* xB,
                double* Y, int64_t ld_y, CondArgs& a);

}  // namespace sem
