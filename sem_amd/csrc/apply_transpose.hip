// Fused transposed (adjoint) operator apply for gfx950 (sem_apply_transpose).
//
//     y = A_D^T z + c_acc y_in,    A = cM M + cK K + cX diag(cu) G_x + cY diag(cv) G_y + diag(cE ea)
//
// with A_D = A with identity Dirichlet rows, so A_D^T z = A^T ((1 - m) z) + m z (m = the Dirichlet
// mask).  M and K are symmetric.  GLL quadrature is exact for degree 2P - 1, so the assembled 1-D
// gradient satisfies Gx1d^T = -Gx1d + B with B = -1 at the first line, +1 at the last one, and
//
//     G_x^T w = -G_x w + b_x w,   b_x[gx, gy] = -/+ (dy/2) My[gy] on the lines gx = 0 / N_x - 1
//
// (likewise in y): the transposed gradient is the forward rows of apply_band.hip applied to the
// pre-multiplied operand cu z plus a pointwise term on the four boundary lines.
//
// Layout: the band kernel's (apply_band.hip).  One workgroup = one tile of TXE x TYE element
// positions (BX = TXE P lines, BY = TYE P columns) of the nex + 1 x ney + 1 positions, the last of
// each direction being the ghost element that holds the closing line / column.  Staging reads z, cu,
// cv and the mask once per window node and writes THREE operands to LDS: z' = (1 - m) z over the
// whole window, cu z' over the tile's columns (x halo only) and cv z' over the tile's lines (y halo
// only); the original z of the tile's Dirichlet nodes is kept for the m z term.  Then
//   X waves    lane = column, wave = (element position, row split): K rows on z' and G rows on cu z'
//              along x from a (2P+1)-node window in registers, one after the other;
//   Y waves    lane = (line, element position), wave = column split: the same along y with cv z';
// and every wave runs the epilogue of its nodes.  All coefficients are compile-time constants
// (gll_consts.h), every sum has a fixed order, there are no atomics: results are bitwise
// reproducible.
//
// Strips (sem_apply_transpose_part).  The matrix A_s that sem_apply applies on a strip handle is the operator
// of the sub-mesh of the strip's own columns with the owner rule on its right interface line, so the kernel
// runs on strip-local geometry: nex, NX, every gx and the mask index count from the strip's first line, the
// 1-D weights and the boundary term b_x of the transposed gradient sit on the STRIP's first and last line
// (the interface parts cancel in the exchange), and the W / E side bits reach the kernel only where the strip
// touches the mesh boundary.  On a right interface line z' = (1 - m) z is formed as everywhere -- a Dirichlet
// row of A_s is all zero there -- and m z, the diagonal term and the accumulate term are left to the right-hand
// owner at no cost per node: the buffer resources of the two pointwise operands end before that line (nown
// bytes: loads past them return 0), and the tiles that hold the line clear its Zo row between the barriers.
// A launch covers element positions [pos0, pos1) of 0..nex (nex = the ghost position of the closing line);
// tile tx starts at position pos0 + tx TXE.  A node's sums do not depend on where its tile starts, so ranged
// launches that cover every position give bitwise the unranged result.  The strip / range code is the PART = true
// instantiation; the whole-mesh launch without a range runs PART = false, the code it ran before strips existed.
#include <hip/hip_runtime.h>

#include "apply_common.h"
#include "apply_select.h"

namespace sem {

template <int P>
struct TCfg {
  static constexpr int n = P + 1;
  static constexpr int TYE = BandShape<P>::TYE, TXE = BandShape<P>::TXE;  // the band kernel's tile
  static constexpr int NS = BandShape<P>::NS;            // row splits of an element
  static constexpr int BX = TXE * P, BY = TYE * P;       // lines / columns of the tile
  static constexpr int XW = (BY + 63) / 64;
  static constexpr int LW = 64 * XW;                     // lanes per tile line (X role, epilogue)
  static constexpr int NXW = TXE * NS * XW;              // X waves
  static constexpr int YL = BX * TYE;                    // Y lanes per split
  static constexpr int YW = (YL + 63) / 64;
  static constexpr int NYW = NS * YW;                    // Y waves
  static constexpr int NW = NXW + NYW;
  static constexpr int THREADS = 64 * NW;
  static constexpr int RX = BX + P + 1, RY = BY + P + 1; // staged window [gx0-P, gx0+BX] x [gy0-P, gy0+BY]
  static constexpr int PT = RY | 1;                      // odd pitches
  static constexpr int PY = LW + 1;
  static constexpr int NSTAGE = (RX * RY + THREADS - 1) / THREADS;
  static constexpr int NE = (BX * LW + THREADS - 1) / THREADS;
  static constexpr int r0(int s) { return s * P / NS; }  // rows [r0, r1) of split s
  static constexpr int r1(int s) { return (s + 1) * P / NS; }
  static_assert(THREADS <= 1024, "workgroup too large");
};

struct TArgs {
  const double* z;
  double* y;
  const double* cu;
  const double* cv;
  const double* ea;
  const uint8_t* mask;
  double fKx, fKy, fM, fX, fY, cE, cA;  // cK dy/dx, cK dx/dy, cM dx dy/4, cX dy/2, cY dx/2
  int NY, NX, nex, ney, tiles_y, nblk, nbytes, dir_mode, cpol;  // NX, nex: the handle's own lines / columns
  unsigned sides;
  int pos0, pos1;  // element positions of the launch
  int nown;        // bytes of the lines whose pointwise terms this handle writes (nbytes, or one line less)
};

// GLL weights of order P as a device table (ws[] in LDS is filled from it)
template <int P>
struct TWTab {
  double v[P + 1];
  static constexpr TWTab make() {
    TWTab t{};
    for (int k = 0; k <= P; ++k) t.v[k] = GllConst<P>::w[k];
    return t;
  }
};
template <int P>
__device__ const TWTab<P> kTransposeW = TWTab<P>::make();

// sum_l A[ROW][l] t[l] with A = K_s (G = false) or G_s (G = true), coefficients folded into the code
template <int P, int ROW, bool G, int... L>
__device__ __forceinline__ double tdot(const double* t, std::integer_sequence<int, L...>) {
  double s = 0.0;
  if constexpr (G)
    ((s = fma(gc<P, ROW * (P + 1) + L>(), t[L], s)), ...);
  else
    ((s = fma(kc<P, ROW * (P + 1) + L>(), t[L], s)), ...);
  return s;
}

// Rows [R0, R1) of one element from a (2P+1)-node window (t[P..2P] = the element, t[0..P] = its left
// neighbour, used by the shared-node row 0 only; absent elements are staged as 0 and fL, fR in {0, 1}
// switch off their part of the shared node).
template <int P, int R0, int R1, bool G>
__device__ __forceinline__ void trows(const double (&t)[2 * P + 1], double fL, double fR, double* out) {
  using Seq = std::make_integer_sequence<int, P + 1>;
  for_rows(std::make_integer_sequence<int, R1 - R0>{}, [&](auto I) {
    constexpr int row = R0 + decltype(I)::value;
    double s = tdot<P, row, G>(t + P, Seq{});
    if constexpr (row == 0) s = fma(fL, tdot<P, P, G>(t, Seq{}), fR * s);
    out[decltype(I)::value] = s;
  });
}

// PART = false: every position of a handle that owns its last line (pos0, pos1 and nown are not read: the code of
// the whole-mesh launch); PART = true: a position range and / or a right interface line.  The axis exists because a
// measurement asked for it: with the three values read on every launch the whole-mesh apply at 64^2, P = 8 sat
// 0.9 % above the previous kernel's range in an alternated A/B (profiles/strip_adjoint/ab_summary.txt).
template <int P, bool PART>
__global__ __launch_bounds__((TCfg<P>::THREADS)) void apply_transpose(const TArgs a) {
  using C = TCfg<P>;
  constexpr int n = C::n, BX = C::BX, BY = C::BY, PT = C::PT, PY = C::PY, LW = C::LW, NS = C::NS;
  constexpr int TXE = C::TXE, TYE = C::TYE, RX = C::RX, RY = C::RY;
  __shared__ double Ts[RX * PT];   // z' = (1 - m) z
  __shared__ double Us[RX * PY];   // cu z', tile columns
  __shared__ double Vs[BX * PT];   // cv z', tile lines
  __shared__ double Zo[BX * PY];   // m z of the tile's nodes
  __shared__ double Rx[BX * PY];   // x-direction results
  __shared__ double Ry[BX * PY];   // y-direction results
  __shared__ double ws[n];

  // XCD-aware remap (as the band kernel): each XCD gets a contiguous run of tiles, y fastest
  const int nb = a.nblk, bid = blockIdx.x, tyn = a.tiles_y;
  const int xcd = bid & 7, rk = bid >> 3, q8 = nb >> 3, rem = nb & 7;
  const int L = (xcd < rem ? xcd * (q8 + 1) : rem * (q8 + 1) + (xcd - rem) * q8) + rk;
  const int tx = L / tyn, ty = L - tx * tyn;

  const int NY = a.NY, NX = a.NX, nex = a.nex, ney = a.ney;
  const int m0 = (PART ? a.pos0 : 0) + tx * TXE, m1 = min(m0 + TXE, PART ? a.pos1 : nex + 1);
  const int n0 = ty * TYE, n1 = min(n0 + TYE, ney + 1);
  const int gx0 = m0 * P, gy0 = n0 * P;
  const int rows_ok = (min(m1, nex) - m0) * P + (m1 > nex ? 1 : 0);
  const int cols_ok = (min(n1, ney) - n0) * P + (n1 > ney ? 1 : 0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int nbytes = a.nbytes;
  const bool grad = a.fX != 0.0 || a.fY != 0.0;
  const bool has_u = grad && a.cu != nullptr, has_v = grad && a.cv != nullptr;
  const bool has_e = a.cE != 0.0 && a.ea != nullptr, has_a = a.cA != 0.0;
  const bool dir = a.dir_mode != SEM_DIR_NONE, has_m = dir && a.mask != nullptr;
  // a resource of 0 bytes returns 0 for every load without touching memory, as does any offset outside
  // [0, nbytes): absent operands and absent nodes need no branch
  const auto rz = brsrc(a.z, nbytes), ru = brsrc(a.cu, has_u ? nbytes : 0), rv = brsrc(a.cv, has_v ? nbytes : 0);
  const auto rm = brsrc(a.mask, has_m ? nbytes / 8 : 0);
  // the pointwise operands end where the owned lines end: loads on a right interface line return 0 (y_in is not read)
  const int nown = PART ? a.nown : nbytes;
  const auto re = brsrc(a.ea, has_e ? nown : 0), ra = brsrc(a.y, has_a ? nown : 0);
  const auto ry = brsrc(a.y, nbytes);

  const double wsv = tid < n ? kTransposeW<P>.v[tid] : 0.0;

  // ---- staging loads: window node idx = tid + k THREADS -> (line rr, column cc), consecutive lanes along y
  double sz[C::NSTAGE], su[C::NSTAGE], sv[C::NSTAGE];
  unsigned sm[C::NSTAGE];
#pragma unroll
  for (int k = 0; k < C::NSTAGE; ++k) {
    const int idx = tid + k * C::THREADS;
    const int rr = idx / RY, cc = idx - rr * RY;
    const int gx = gx0 - P + rr, gy = gy0 - P + cc;
    const bool ok = idx < RX * RY && gx >= 0 && gx < NX && gy >= 0 && gy < NY;
    const int p = ok ? gx * NY + gy : -1;
    const bool inx = cc >= P && cc < P + BY, iny = rr >= P && rr < P + BX;
    sz[k] = bload(rz, p * 8);
    su[k] = bload(ru, (inx ? p : -1) * 8);
    sv[k] = bload(rv, (iny ? p : -1) * 8);
    sm[k] = __builtin_amdgcn_raw_buffer_load_b8(rm, p, 0, 0);
  }
  // ---- the epilogue's pointwise operands, behind the staging loads
  int eoff[C::NE];
  double pe[C::NE], pa[C::NE];
#pragma unroll
  for (int e = 0; e < C::NE; ++e) {
    const int q = tid + e * C::THREADS;
    const int r = q / LW, c = q - r * LW;
    const bool ok = q < BX * LW && r < rows_ok && c < cols_ok;
    eoff[e] = ok ? (gx0 + r) * NY + gy0 + c : -1;
    pe[e] = bload(re, eoff[e] * 8);
    pa[e] = bload(ra, eoff[e] * 8);
  }

  // ---- LDS: the three operands, formed while staging
  const unsigned sd = dir ? a.sides : 0u;
#pragma unroll
  for (int k = 0; k < C::NSTAGE; ++k) {
    const int idx = tid + k * C::THREADS;
    if (idx < RX * RY) {
      const int rr = idx / RY, cc = idx - rr * RY;
      const int gx = gx0 - P + rr, gy = gy0 - P + cc;
      const bool inx = cc >= P && cc < P + BY, iny = rr >= P && rr < P + BX;
      const bool side = ((sd & SEM_SIDE_W) && gx == 0) || ((sd & SEM_SIDE_E) && gx == NX - 1) ||
                        ((sd & SEM_SIDE_S) && gy == 0) || ((sd & SEM_SIDE_N) && gy == NY - 1);
      const bool isd = has_m ? (sm[k] & 0xff) != 0 : side;
      const double zp = isd ? 0.0 : sz[k];
      Ts[rr * PT + cc] = zp;
      if (inx) Us[rr * PY + cc - P] = has_u ? su[k] * zp : zp;
      if (iny) Vs[(rr - P) * PT + cc] = has_v ? sv[k] * zp : zp;
      if (inx && iny) Zo[(rr - P) * PY + cc - P] = isd ? sz[k] : 0.0;
    }
  }
  if (tid < n) ws[tid] = wsv;
  __syncthreads();
  // a right interface line's m z entries are its owner's: cleared here, between the barriers, in the strip tiles
  // that hold that line (the roles below do not touch Zo; the epilogue reads it behind the second barrier)
  if constexpr (PART) {
    if (nown != nbytes && m1 > nex) {
      for (int c = tid; c < BY; c += C::THREADS) Zo[(rows_ok - 1) * PY + c] = 0.0;
    }
  }

  constexpr double w0 = GllConst<P>::w[0], wP = GllConst<P>::w[P];
  if (w < C::NXW) {
    // ---- X role: wave = (element position xa, split xs), lane = column xc
    const int xg = w / C::XW;
    const int xa = xg / NS, xs = xg - xa * NS;
    const int xc = (w - xg * C::XW) * 64 + lane;
    if (xa < m1 - m0 && xc < BY) {
      const bool xghost = m0 + xa == nex, hasLx = m0 + xa - 1 >= 0;  // wave-uniform
      const double fL = hasLx ? 1.0 : 0.0, fR = xghost ? 0.0 : 1.0;
      const int jc = xc % P, nc = n0 + xc / P;
      const double myc = jc != 0 ? ws[jc] : (nc - 1 >= 0 ? wP : 0.0) + (nc < ney ? w0 : 0.0);
      const double sk = a.fKx * myc, sg = -a.fX * myc;
      for_rows(std::make_integer_sequence<int, NS>{}, [&](auto S) {
        constexpr int s = decltype(S)::value;
        if (xs != s) return;
        constexpr int R0 = C::r0(s), R1 = C::r1(s);
        constexpr int q0 = R0 == 0 ? 0 : P;  // only row 0 reads the left element
        double t[2 * P + 1];
        double k[R1 - R0], g[R1 - R0];
#pragma unroll
        for (int qq = 0; qq < q0; ++qq) t[qq] = 0.0;
#pragma unroll
        for (int qq = q0; qq <= 2 * P; ++qq) t[qq] = Ts[(xa * P + qq) * PT + P + xc];
        trows<P, R0, R1, false>(t, fL, fR, k);
        if (grad) {
#pragma unroll
          for (int qq = q0; qq <= 2 * P; ++qq) t[qq] = Us[(xa * P + qq) * PY + xc];
          trows<P, R0, R1, true>(t, fL, fR, g);
        } else {
#pragma unroll
          for (int i = 0; i < R1 - R0; ++i) g[i] = 0.0;
        }
#pragma unroll
        for (int i = 0; i < R1 - R0; ++i) {
          if (xghost && R0 + i != 0) continue;  // a ghost position holds its row 0 only
          Rx[(xa * P + R0 + i) * PY + xc] = fma(sk, k[i], sg * g[i]);
        }
      });
    }
  } else {
    // ---- Y role: wave = split h, lane = (line r, element position b)
    const int wy = w - C::NXW;
    const int h = wy / C::YW;
    const int t2 = (wy - h * C::YW) * 64 + lane;
    const int r = t2 % BX, b = t2 / BX;
    if (t2 < C::YL && r < rows_ok && b < n1 - n0) {
      const bool yghost = n0 + b == ney, hasLy = n0 + b - 1 >= 0;
      const double fL = hasLy ? 1.0 : 0.0, fR = yghost ? 0.0 : 1.0;
      const int i = r % P, ex = m0 + r / P;
      const double mx = i != 0 ? ws[i] : (ex - 1 >= 0 ? wP : 0.0) + (ex < nex ? w0 : 0.0);
      const double sk = a.fKy * mx, sg = -a.fY * mx;
      for_rows(std::make_integer_sequence<int, NS>{}, [&](auto H) {
        constexpr int hh = decltype(H)::value;
        if (h != hh) return;
        constexpr int R0 = C::r0(hh), R1 = C::r1(hh);
        constexpr int q0 = R0 == 0 ? 0 : P;
        double t[2 * P + 1];
        double k[R1 - R0], g[R1 - R0];
#pragma unroll
        for (int qq = 0; qq < q0; ++qq) t[qq] = 0.0;
#pragma unroll
        for (int qq = q0; qq <= 2 * P; ++qq) t[qq] = Ts[(P + r) * PT + b * P + qq];
        trows<P, R0, R1, false>(t, fL, fR, k);
        if (grad) {
#pragma unroll
          for (int qq = q0; qq <= 2 * P; ++qq) t[qq] = Vs[r * PT + b * P + qq];
          trows<P, R0, R1, true>(t, fL, fR, g);
        } else {
#pragma unroll
          for (int j = 0; j < R1 - R0; ++j) g[j] = 0.0;
        }
#pragma unroll
        for (int j = 0; j < R1 - R0; ++j) {
          if (yghost && R0 + j != 0) continue;
          Ry[r * PY + b * P + R0 + j] = fma(sk, k[j], sg * g[j]);
        }
      });
    }
  }
  __syncthreads();

  // ---- epilogue, every wave: x + y rows, mass, the boundary-line terms of the transposed gradients, the
  // diagonal term, the Dirichlet entries m z and the accumulate term
  double zz[C::NE];
#pragma unroll
  for (int e = 0; e < C::NE; ++e) {
    const int q = tid + e * C::THREADS;
    const int r = q / LW, c = q - r * LW;
    double val = 0.0;
    if (eoff[e] >= 0) {
      const int o = r * PY + c;
      const double zc = Ts[(P + r) * PT + P + c];
      const int i = r % P, me = m0 + r / P, j = c % P, ne = n0 + c / P;
      const double mx = i != 0 ? ws[i] : (me - 1 >= 0 ? wP : 0.0) + (me < nex ? w0 : 0.0);
      const double my = j != 0 ? ws[j] : (ne - 1 >= 0 ? wP : 0.0) + (ne < ney ? w0 : 0.0);
      val = Rx[o] + Ry[o];
      val = fma(a.fM * mx * my, zc, val);
      if (grad) {
        const int gx = gx0 + r, gy = gy0 + c;
        const double bx = (gx == NX - 1 ? 1.0 : 0.0) - (gx == 0 ? 1.0 : 0.0);
        const double by = (gy == NY - 1 ? 1.0 : 0.0) - (gy == 0 ? 1.0 : 0.0);
        val = fma(a.fX * my * bx, Us[(P + r) * PY + c], val);
        val = fma(a.fY * mx * by, Vs[r * PT + P + c], val);
      }
      if (has_e) val = fma(a.cE * pe[e], zc, val);
      val += Zo[o];
      if (has_a) val = fma(a.cA, pa[e], val);
    }
    zz[e] = val;
  }
  if (a.cpol == 3) {  // system-scope stores on a mesh whose working set stays in the MALL (transpose_cpol)
#pragma unroll
    for (int e = 0; e < C::NE; ++e)
      if (eoff[e] >= 0) bstore_c<17>(ry, eoff[e] * 8, zz[e]);
  } else {
#pragma unroll
    for (int e = 0; e < C::NE; ++e)
      if (eoff[e] >= 0) bstore(ry, eoff[e] * 8, zz[e]);
  }
}

template <int P>
static int launch_transpose(const ApplyArgs& g, const sem_handle* h, hipStream_t s) {
  using C = TCfg<P>;
  const int ncols = h->ex_end - h->ex_begin;
  // element positions [pos0, pos1) of 0..ncols (ncols = the ghost position of the closing line)
  const bool ranged = g.pos1 > 0;
  const int pos0 = ranged ? g.pos0 : 0, pos1 = ranged ? g.pos1 : ncols + 1;
  const long long tiles_x = (pos1 - pos0 + C::TXE - 1) / C::TXE;
  const long long tiles_y = (h->ney + 1 + C::TYE - 1) / C::TYE;
  const long long nblk = tiles_x * tiles_y;
  if (nblk <= 0 || nblk > 0x7fffffffLL) return set_error(SEM_EINVAL, "mesh too large for one launch");
  TArgs t{};
  t.z = g.x;
  t.y = g.y;
  t.cu = g.cu;
  t.cv = g.cv;
  t.ea = g.ea;
  t.mask = g.mask;
  t.fKx = g.cK * g.sx;
  t.fKy = g.cK * g.sy;
  t.fM = g.cM * g.hxy;
  t.fX = g.cX * g.hy;
  t.fY = g.cY * g.hx;
  t.cE = g.cE;
  t.cA = g.cA;
  t.NY = static_cast<int>(g.NY);
  t.NX = static_cast<int>(g.line_end - g.line_begin + 1);
  t.nex = ncols;
  t.ney = g.ney;
  t.tiles_y = static_cast<int>(tiles_y);
  t.nblk = static_cast<int>(nblk);
  t.nbytes = g.n_local32 * 8;
  t.dir_mode = g.dir_mode;
  t.cpol = transpose_cpol(g.n_local32);
  // W and E are mesh sides: a strip's first / last line is one only where the strip touches the boundary
  t.sides = g.sides & ~((h->ex_begin != 0 ? SEM_SIDE_W : 0u) | (h->ex_end != h->nex ? SEM_SIDE_E : 0u));
  t.pos0 = pos0;
  t.pos1 = pos1;
  t.nown = t.nbytes - (h->ex_end == h->nex ? 0 : t.NY * 8);
  if (ranged || t.nown != t.nbytes)
    hipLaunchKernelGGL((apply_transpose<P, true>), dim3(static_cast<unsigned>(nblk)), dim3(C::THREADS), 0, s, t);
  else
    hipLaunchKernelGGL((apply_transpose<P, false>), dim3(static_cast<unsigned>(nblk)), dim3(C::THREADS), 0, s, t);
  return hip_check(hipGetLastError(), "apply (transpose) launch");
}

int launch_apply_transpose(const ApplyArgs& a, const sem_handle* h, hipStream_t s) {
  return dispatch_order(h->P, [&](auto P) { return launch_transpose<decltype(P)::value>(a, h, s); });
}

}  // namespace sem
