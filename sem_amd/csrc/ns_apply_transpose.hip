// Fused transposed (adjoint) Navier-Stokes differential apply for gfx950 (sem_ns_apply_transpose): A^T z for the
// operator A of sem_ns_apply's differential form (_get_dresiduals at dT = 0, NavierStokes_Solver.py:138-160),
//
//     A = [ J  B ]    J = velocity Jacobian with identity Dirichlet rows,   B = (1 - m) [G_x; G_y],
//         [ C  E ]    C = c_div (1 - m_c) [G_x, G_y],                       E = diag(m_b) K + e_pin e_pin^T,
//
// m the Dirichlet mask, the pinned row written after the Neumann rows (m_c = m + pin, m_b = m - pin) or, with
// pin_first, before them (a pin on a Dirichlet node then stays a (K p) row: m_b = m).  With
//
//     z'_u = (1 - m) zu,   z'_v = (1 - m) zv,   w = c_div (1 - m_c) zc,   k = m_b zc,
//     Sys  = cM M + cK K + cX diag(cu) G_x + cY diag(cv) G_y,
//
//     yu = Sys^T z'_u + juu z'_u + jvu z'_v + G_x^T w + m zu
//     yv = Sys^T z'_v + jvv z'_v + juv z'_u + G_y^T w + m zv
//     yp = G_x^T z'_u + G_y^T z'_v + K k + e_pin zc[pin]
//     yT = c_T M z'_v                                       (the adjoint of the c_T M T term; pointwise)
//
// M and K are symmetric.  GLL quadrature is exact for degree 2P - 1, so the assembled 1-D gradient satisfies
// G1d^T = -G1d + B with B = -1 at the first node, +1 at the last one (apply_transpose.hip), and
//
//     G_x^T a = -G_x a + b_x a,   b_x[gx, gy] = -/+ (dy/2) My[gy] on the lines gx = 0 / N_x - 1
//
// (likewise in y).  In Sys^T the operand is a = cu z', so one row of Sys^T z' along x is
// My[gy] sum_q (cK (dy/dx) K[r, q] - cX (dy/2) cu[q] G[r, q]) z'[q]: the FORWARD 1-D rows of the GLL tables with the
// convection coefficient taken at the column node q instead of the row node.  Every sum is therefore a forward row
// over operands that staging masked or scaled on their way into LDS; there is no scatter and there are no atomics,
// each output has one fixed summation order (x rows: left element then right element, nodes increasing; then the
// y rows likewise; then the pointwise terms in the order of the epilogue below) and is bitwise reproducible.
//
// Layout: sem_ns_apply's LDS-tile form (ns_apply.hip, NsTile).  One workgroup per tile of one element-column position x
// TYE element-row positions (P lines x TYE P columns of owned nodes, one thread per owned node; the closing line /
// column of the mesh belongs to a ghost position past the last element), tiles in the XCD-aware order of the forward
// kernel.  Phase 1 stages, once per window node, over the P lines / columns before the owned block and the one after it:
//     z'_u, z'_v, w, k   the cross of the window (the tile's columns over the x halo, its lines over the y halo)
//     -cX (dy/2) cu      the tile's columns, x halo only (the x rows are its only readers)
//     -cY (dx/2) cv      the tile's lines, y halo only
// with odd pitches; the GLL tables (gll_consts.h) go to LDS beside them.  Phase 2 forms every owned node's outputs from
// LDS: one pass per direction over the node's element row(s), each staged value and table entry read once and feeding
// all the sums that use it, then the pointwise terms and the stores.  The form flags fix at compile time which operands
// are staged and which sums are formed for the forms the solvers launch (transposed gradient: zc -> yu, yv;
// transposed divergence: zu, zv, zc -> yp; velocity rows: zu, zv -> yu, yv; everything).
//
// Strips (sem_ns_apply_transpose_part).  The matrix A_s that sem_ns_apply applies on a strip handle is the operator of
// the sub-mesh of the strip's own element columns with the owner rule on its right interface line, so the kernel runs
// on strip-local geometry: NX, nex, every gx, the mask index and the pin count from the strip's first line (a pin
// outside the strip is no pin), the 1-D x weights, the K and G rows and the boundary term b_x of G_x^T stop at / sit on
// the STRIP's first and last line (the interface parts cancel in the exchange), and the W / E side bits reach the
// kernel only where the strip touches the mesh boundary.  On a right interface line the forward pinned row and
// Dirichlet velocity rows are all zero and the j** terms are the right-hand owner's: z', w, k are staged there as
// everywhere (a kept pin gives w = k = 0 on any line), and m zu, m zv, the j** terms and e_pin zc[pin] are not added.
// That line is the one line of the ghost position tx = nex, so the gate is workgroup-uniform (tx < nex), and it
// exists only in the PART = true instantiations, which a handle with a right interface line launches.  A handle
// that owns its last line runs PART = false: the kernel arguments and the instruction stream of the whole-mesh
// kernel as it was before strips (profiles/ns_strip_adjoint/ab_summary.txt: why the axis exists).
#include <hip/hip_runtime.h>

#include <string>

#include "gll_consts.h"
#include "hip_util.h"
#include "sem_internal.h"

namespace sem {

struct NsTArgs {
  const double *zu, *zv, *zc;
  double *yu, *yv, *yp, *yT;
  const double *cu, *cv, *juu, *juv, *jvu, *jvv;
  const uint8_t* mask;
  double fKx, fKy, fM, fX, fY;  // Sys: cK dy/dx, cK dx/dy, cM dx dy/4, cX dy/2, cY dx/2
  double hy, hx, sx, sy;        // plain G_x / G_y / K factors: dy/2, dx/2, dy/dx, dx/dy
  double fT, c_div;             // c_T dx dy/4
  int pitch;                    // node (gx, gy) of zu, zv, yu, yv at gx * pitch + gy
  int pin;                      // pinned node, -1: none
  int NY, NX, nex, ney, pin_first;  // NX, nex: the handle's own lines / element columns
  unsigned sides;                    // W, E: only where the handle touches the mesh boundary
};

enum : int { NT_ZUV = 1, NT_ZC = 2, NT_YUV = 4, NT_YP = 8, NT_ALL = 15 };

// Which operands a form stages and which sums it forms (compile time).
template <int F>
struct NsTForm {
  static constexpr bool ZUV = (F & NT_ZUV) != 0, ZC = (F & NT_ZC) != 0;
  static constexpr bool YUV = (F & NT_YUV) != 0, YP = (F & NT_YP) != 0;
  static constexpr bool SYS = ZUV && YUV;  // Sys^T z'_u, Sys^T z'_v: z', cu, cv
  static constexpr bool GW = ZC && YUV;    // G_x^T w, G_y^T w: w
  static constexpr bool GZ = ZUV && YP;    // G_x^T z'_u + G_y^T z'_v: z'
  static constexpr bool KK = ZC && YP;     // K k: k
};

// The forward tile form's shape (NsTile, ns_apply.hip): ~32 owned columns, twice the workgroups of a 64-wide tile.
template <int P>
struct NsTTile {
  static constexpr int n = P + 1;
  static constexpr int TYE = (32 / P) > 0 ? 32 / P : 1;
  static constexpr int BX = P, BY = TYE * P;
  static constexpr int SX = BX + P + 1, SY = BY + P + 1;  // staged lines gx0-P .. gx0+P, columns gy0-P .. gy0+BY
  static constexpr int PIT = SY | 1;                      // odd pitches
  static constexpr int PC = BY | 1;
  // one owned node per thread: with a second trip of the node loop the compiler keeps both trips' LDS reads in flight
  // (255 VGPRs and one wave per SIMD at P = 12 against 89 at P = 11)
  static constexpr int THREADS = (BX * BY + 63) / 64 * 64;
  static constexpr int NTAB = 2 * n * n + n;
  // the full form: four windows, cu over the x halo, cv over the y halo, the tables
  static constexpr int FULL_BYTES = (4 * SX * PIT + SX * PC + BX * PIT + NTAB) * 8;
  static_assert(FULL_BYTES <= 80 * 1024, "two workgroups of the full form per CU (160 KiB of LDS)");
};

// K_s | G_s | w of order P as one device table (copied to LDS by every workgroup)
template <int P>
struct NsTTab {
  double v[NsTTile<P>::NTAB];
  static constexpr NsTTab make() {
    NsTTab t{};
    constexpr int n = P + 1;
    for (int k = 0; k < n * n; ++k) {
      t.v[k] = GllConst<P>::K[k];
      t.v[n * n + k] = GllConst<P>::G[k];
    }
    for (int k = 0; k < n; ++k) t.v[2 * n * n + k] = GllConst<P>::w[k];
    return t;
  }
};
template <int P>
__device__ const NsTTab<P> kNsTTab = NsTTab<P>::make();

// The element row(s) of 1-D node (e, i) over elements [0, e_hi): f(row, first) for row `row` of an element whose node 0
// lies `first` nodes from the node (first <= 0) -- row i of its element, or at an element boundary row P of the
// element on the left, then row 0 of the element on the right.
template <int P, class Fn>
__device__ __forceinline__ void nst_rows(int e, int i, int e_hi, Fn&& f) {
  if (i != 0) {
    f(i, -i);
    return;
  }
  if (e > 0) f(P, -P);
  if (e < e_hi) f(0, 0);
}

__device__ __forceinline__ double nst_wsum(int g, int P, int e_hi, const double* w) {
  const int e = g / P, i = g - e * P;
  return i != 0 ? w[i] : (e > 0 ? w[P] : 0.0) + (e < e_hi ? w[0] : 0.0);
}

__device__ __forceinline__ bool nst_dir(const NsTArgs& a, int q, int gx, int gy) {
  return a.mask ? a.mask[q] != 0
                : (((a.sides & SEM_SIDE_W) && gx == 0) || ((a.sides & SEM_SIDE_E) && gx == a.NX - 1) ||
                   ((a.sides & SEM_SIDE_S) && gy == 0) || ((a.sides & SEM_SIDE_N) && gy == a.NY - 1));
}

// the row of rc that the forward apply keeps as the pinned row p[pin]
__device__ __forceinline__ bool nst_pin(const NsTArgs& a, int q, bool dir) {
  return q == a.pin && (!a.pin_first || !dir);
}

// PART = true: a strip with a right interface line (ex_end < nex), whose pointwise terms are its right-hand owner's.
template <int P, int F, bool PART>
__global__ __launch_bounds__((NsTTile<P>::THREADS)) void ns_apply_transpose_tile(const NsTArgs a, int tiles_y, int ntiles, int per_xcd) {
  using T = NsTTile<P>;
  using M = NsTForm<F>;
  constexpr int n = T::n, BX = T::BX, BY = T::BY, SX = T::SX, SY = T::SY, PIT = T::PIT, PC = T::PC;
  __shared__ double tab[T::NTAB];
  __shared__ double sZu[M::ZUV ? SX * PIT : 1], sZv[M::ZUV ? SX * PIT : 1];  // z'_u, z'_v
  __shared__ double sW[M::GW ? SX * PIT : 1], sK[M::KK ? SX * PIT : 1];      // w, k
  __shared__ double sCu[M::SYS ? SX * PC : 1], sCv[M::SYS ? BX * PIT : 1];   // -fX cu (tile columns), -fY cv (tile lines)
  const int b = blockIdx.x;
  const int tile = (b & 7) * per_xcd + (b >> 3);
  if (tile >= ntiles) return;
  const int tx = tile / tiles_y, ty = tile - tx * tiles_y;
  const int NY = a.NY, NX = a.NX, pitch = a.pitch;
  const int gx0 = tx * P, gy0 = ty * T::TYE * P;
  const int sx0 = gx0 - P, sy0 = gy0 - P;  // staged origin
  for (int i = threadIdx.x; i < T::NTAB; i += T::THREADS) tab[i] = kNsTTab<P>.v[i];

  // ---- phase 1: staging.  Only the cross of the window is read in phase 2 (its corners stay unset); nodes outside the
  // mesh are staged as zeros.
  for (int k = threadIdx.x; k < SX * SY; k += T::THREADS) {
    const int r = k / SY, c = k - r * SY;
    const bool inx = c >= P && c < P + BY, iny = r >= P && r < P + BX;
    if (!inx && !iny) continue;
    const int gx = sx0 + r, gy = sy0 + c;
    double zu = 0.0, zv = 0.0, w = 0.0, kk = 0.0, ncu = 0.0, ncv = 0.0;
    if (gx >= 0 && gx < NX && gy >= 0 && gy < NY) {
      const int q = gx * NY + gy, qv = gx * pitch + gy;
      const bool dir = nst_dir(a, q, gx, gy);
      if constexpr (M::ZUV) {
        if (!dir) {
          if (a.zu) zu = a.zu[qv];
          if (a.zv) zv = a.zv[qv];
        }
      }
      if constexpr (M::GW || M::KK) {
        if (a.zc && !nst_pin(a, q, dir)) {
          const double zc = a.zc[q];
          if (dir)
            kk = zc;
          else
            w = a.c_div * zc;
        }
      }
      if constexpr (M::SYS) {
        if (inx) ncu = -a.fX * (a.cu ? a.cu[q] : 1.0);
        if (iny) ncv = -a.fY * (a.cv ? a.cv[q] : 1.0);
      }
    }
    if constexpr (M::ZUV) {
      sZu[r * PIT + c] = zu;
      sZv[r * PIT + c] = zv;
    }
    if constexpr (M::GW) sW[r * PIT + c] = w;
    if constexpr (M::KK) sK[r * PIT + c] = kk;
    if constexpr (M::SYS) {
      if (inx) sCu[r * PC + c - P] = ncu;
      if (iny) sCv[(r - P) * PIT + c] = ncv;
    }
  }
  __syncthreads();

  // ---- phase 2: every owned node's outputs from LDS
  const double* Ks = tab;
  const double* Gs = tab + n * n;
  const double* wt = tab + 2 * n * n;
  const bool want_uv = M::YUV && (a.yu || a.yv);  // yT is pointwise: it needs none of the rows
  const bool want_T = M::YUV && a.yT;
  const bool want_p = M::YP && a.yp;
  const bool own = !PART || tx < a.nex;  // false in the ghost position (the closing line) of a PART launch only
  static_assert(BX * BY <= T::THREADS, "one owned node per thread");
  for (int k = threadIdx.x; k < BX * BY; k += T::THREADS) {  // one trip
    const int ox = k / BY, oy = k - ox * BY;
    const int gx = gx0 + ox, gy = gy0 + oy;
    if (gx >= NX || gy >= NY) continue;
    const int ex = gx / P, ix = gx - ex * P, ey = gy / P, iy = gy - ey * P;
    const double mx = nst_wsum(gx, P, a.nex, wt), my = nst_wsum(gy, P, a.ney, wt);
    const int q = gx * NY + gy, qv = gx * pitch + gy;
    const int sidx = (ox + P) * PIT + (oy + P);  // the node in the staged windows
    const bool sys = M::SYS && want_uv, gw = M::GW && want_uv, gz = M::GZ && want_p, kp = M::KK && want_p;
    double Sux = 0.0, Svx = 0.0, Suy = 0.0, Svy = 0.0;              // Sys^T z' rows, without their My / Mx factor
    double gwx = 0.0, gwy = 0.0, gzx = 0.0, gzy = 0.0, kx = 0.0, ky = 0.0;  // G w, G z', K k rows
    nst_rows<P>(ex, ix, a.nex, [&](int row, int first) {
      const int o = sidx + first * PIT, oc = (ox + P + first) * PC + oy;
#pragma unroll
      for (int c = 0; c <= P; ++c) {
        const double K = Ks[row * n + c], G = Gs[row * n + c];
        if constexpr (M::ZUV) {
          const double uq = sZu[o + c * PIT];
          if constexpr (M::SYS) {
            if (sys) {
              const double co = fma(sCu[oc + c * PC], G, a.fKx * K);
              Sux = fma(co, uq, Sux);
              Svx = fma(co, sZv[o + c * PIT], Svx);
            }
          }
          if constexpr (M::GZ) {
            if (gz) gzx = fma(G, uq, gzx);
          }
        }
        if constexpr (M::GW) {
          if (gw) gwx = fma(G, sW[o + c * PIT], gwx);
        }
        if constexpr (M::KK) {
          if (kp) kx = fma(K, sK[o + c * PIT], kx);
        }
      }
    });
    nst_rows<P>(ey, iy, a.ney, [&](int row, int first) {
      const int o = sidx + first, oc = ox * PIT + (oy + P + first);
#pragma unroll
      for (int c = 0; c <= P; ++c) {
        const double K = Ks[row * n + c], G = Gs[row * n + c];
        if constexpr (M::ZUV) {
          const double vq = sZv[o + c];
          if constexpr (M::SYS) {
            if (sys) {
              const double co = fma(sCv[oc + c], G, a.fKy * K);
              Suy = fma(co, sZu[o + c], Suy);
              Svy = fma(co, vq, Svy);
            }
          }
          if constexpr (M::GZ) {
            if (gz) gzy = fma(G, vq, gzy);
          }
        }
        if constexpr (M::GW) {
          if (gw) gwy = fma(G, sW[o + c], gwy);
        }
        if constexpr (M::KK) {
          if (kp) ky = fma(K, sK[o + c], ky);
        }
      }
    });
    // the boundary-line terms of the transposed gradients: b_x = bx (dy/2) My, b_y = by (dx/2) Mx
    const double bx = (gx == NX - 1 ? 1.0 : 0.0) - (gx == 0 ? 1.0 : 0.0);
    const double by = (gy == NY - 1 ? 1.0 : 0.0) - (gy == 0 ? 1.0 : 0.0);
    const bool dir = nst_dir(a, q, gx, gy);
    double zu0 = 0.0, zv0 = 0.0;
    if constexpr (M::ZUV) {
      zu0 = sZu[sidx];
      zv0 = sZv[sidx];
    }
    if constexpr (M::YUV) {
      if (want_uv) {
        double su = 0.0, sv = 0.0;  // the rows shared by yu and yv up to their operand
        if constexpr (M::SYS) {
          // the convection coefficient of the node on its boundary lines: -(bx My)(-fX cu) - (by Mx)(-fY cv)
          const double cb = fma(-(by * mx), sCv[ox * PIT + oy + P], -(bx * my) * sCu[(ox + P) * PC + oy]);
          const double pm = fma(a.fM * mx, my, cb);  // + the mass term: one pointwise coefficient
          su = fma(pm, zu0, fma(my, Sux, mx * Suy));
          sv = fma(pm, zv0, fma(my, Svx, mx * Svy));
        }
        if (a.yu) {
          double z = su;
          if constexpr (M::SYS) {
            if (own && a.juu) z = fma(a.juu[q], zu0, z);
            if (own && a.jvu) z = fma(a.jvu[q], zv0, z);
          }
          if constexpr (M::GW) z = fma(a.hy * my, bx * sW[sidx] - gwx, z);
          if constexpr (M::ZUV) {
            if (own && dir && a.zu) z += a.zu[qv];  // m zu
          }
          a.yu[qv] = z;
        }
        if (a.yv) {
          double z = sv;
          if constexpr (M::SYS) {
            if (own && a.juv) z = fma(a.juv[q], zu0, z);
            if (own && a.jvv) z = fma(a.jvv[q], zv0, z);
          }
          if constexpr (M::GW) z = fma(a.hx * mx, by * sW[sidx] - gwy, z);
          if constexpr (M::ZUV) {
            if (own && dir && a.zv) z += a.zv[qv];  // m zv
          }
          a.yv[qv] = z;
        }
      }
      if (want_T) a.yT[q] = (a.fT * mx * my) * zv0;
    }
    if constexpr (M::YP) {
      if (want_p) {
        double z = 0.0;
        if constexpr (M::GZ) z = fma(a.hx * mx, by * zv0 - gzy, (a.hy * my) * (bx * zu0 - gzx));
        if constexpr (M::KK) {
          z = fma(a.sx * my, kx, z);
          z = fma(a.sy * mx, ky, z);
        }
        if constexpr (M::ZC) {
          if (own && a.zc && nst_pin(a, q, dir)) z += a.zc[q];  // e_pin zc[pin]
        }
        a.yp[q] = z;
      }
    }
  }
}

template <int P, int F>
static int launch_ns_transpose(const NsTArgs& a, bool open_right, hipStream_t s) {
  using T = NsTTile<P>;
  const int tiles_x = a.nex + 1;  // positions 0..nex of the handle's own columns (nex: the closing line)
  const int tiles_y = (a.ney + T::TYE) / T::TYE;
  const long long ntiles = static_cast<long long>(tiles_x) * tiles_y;
  const long long per_xcd = (ntiles + 7) / 8;
  if (8 * per_xcd > 0x7fffffffLL) return set_error(SEM_EUNSUPPORTED, "mesh too large for one launch");
  const dim3 grid(static_cast<unsigned>(8 * per_xcd)), block(T::THREADS);
  if (open_right)
    hipLaunchKernelGGL((ns_apply_transpose_tile<P, F, true>), grid, block, 0, s, a, tiles_y, static_cast<int>(ntiles),
                       static_cast<int>(per_xcd));
  else
    hipLaunchKernelGGL((ns_apply_transpose_tile<P, F, false>), grid, block, 0, s, a, tiles_y, static_cast<int>(ntiles),
                       static_cast<int>(per_xcd));
  return SEM_OK;
}

// The two entry points: `part` lifts the strip refusal; everything else is one contract.
static int ns_transpose(const char* name, bool part, sem_handle* h, const sem_ns_desc* d, const double* zu,
                        const double* zv, const double* zc, double* yu, double* yv, double* yp, double* yT, void* stream) {
  if (!h || !d) return set_error(SEM_EINVAL, "null argument");
  if (d->uv_pitch != 0 && d->uv_pitch < h->NY) return set_error(SEM_EINVAL, "uv_pitch below the line length");
  if (d->pin < -1 || d->pin >= h->NX * h->NY) return set_error(SEM_EINVAL, "pinned node out of range");
  if (d->T || d->dval_u || d->dval_v || d->pin_val != 0.0)
    return set_error(SEM_EINVAL, "the transposed apply is that of the linear part: T, dval_u, dval_v must be NULL "
                                 "and pin_val 0");
  const double* const ins[3] = {zu, zv, zc};
  const double* const outs[4] = {yu, yv, yp, yT};
  for (const double* o : outs)
    for (const double* i : ins)
      if (o && o == i) return set_error(SEM_EINVAL, "an output aliases an input");
  if (d->uv_pitch != 0 && d->uv_pitch != h->NY) {
    // cu, cv are plain vectors, zu, zv line views: the same pointer would name different nodes
    if (d->cu && (d->cu == zu || d->cu == zv))
      return set_error(SEM_EINVAL, "cu aliases zu or zv, but they are line views (uv_pitch != NY)");
    if (d->cv && (d->cv == zu || d->cv == zv))
      return set_error(SEM_EINVAL, "cv aliases zu or zv, but they are line views (uv_pitch != NY)");
  }
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != h->device)
    return set_error(SEM_EINVAL, "handle belongs to device " + std::to_string(h->device) +
                                     ", but the current device is " + std::to_string(cur));
  if (!part && (h->ex_begin != 0 || h->ex_end != h->nex))
    return set_error(SEM_EUNSUPPORTED, "sem_ns_apply_transpose: whole-mesh handles only (no transposed strip apply)");
  const int64_t pitch = d->uv_pitch ? d->uv_pitch : h->NY;
  const int64_t lines = h->line_end - h->line_begin + 1;  // the handle's own lines (NX on a whole mesh)
  // the kernel addresses every vector through 32-bit node offsets
  if (h->n_local > 0x7fffffffLL || (lines - 1) * pitch + h->NY > 0x7fffffffLL)
    return set_error(SEM_EUNSUPPORTED, std::string(name) + ": mesh past the 32-bit node-offset limit "
                                                           "(n_local or (NX - 1) uv_pitch + NY above 2^31 - 1)");
  if (!yu && !yv && !yp && !yT) return SEM_OK;
  NsTArgs a{};
  a.zu = zu;
  a.zv = zv;
  a.zc = zc;
  a.yu = yu;
  a.yv = yv;
  a.yp = yp;
  a.yT = yT;
  a.cu = d->cu;
  a.cv = d->cv;
  a.juu = d->juu;
  a.juv = d->juv;
  a.jvu = d->jvu;
  a.jvv = d->jvv;
  a.mask = d->dir_mask;
  // W and E are mesh sides: a strip's first / last line is one only where the strip touches the boundary
  a.sides = d->dir_sides & ~((h->ex_begin != 0 ? SEM_SIDE_W : 0u) | (h->ex_end != h->nex ? SEM_SIDE_E : 0u));
  const double dx = h->dx, dy = h->dy;
  a.fKx = d->c_stiff * (dy / dx);
  a.fKy = d->c_stiff * (dx / dy);
  a.fM = d->c_mass * ((dx / 2.0) * (dy / 2.0));
  a.fX = d->c_gradx * (dy / 2.0);
  a.fY = d->c_grady * (dx / 2.0);
  a.hy = dy / 2.0;
  a.hx = dx / 2.0;
  a.sx = dy / dx;
  a.sy = dx / dy;
  a.fT = d->c_T * ((dx / 2.0) * (dy / 2.0));
  a.c_div = d->c_div;
  a.pitch = static_cast<int>(pitch);
  // the pin is a global node; the kernel counts nodes from the handle's first line (outside the strip: no pin)
  const int64_t pin = d->pin < 0 ? -1 : d->pin - h->line_begin * h->NY;
  a.pin = pin >= 0 && pin < h->n_local ? static_cast<int>(pin) : -1;
  a.pin_first = d->pin_first;
  a.NY = static_cast<int>(h->NY);
  a.NX = static_cast<int>(lines);
  a.nex = h->ex_end - h->ex_begin;
  a.ney = h->ney;
  const bool open_right = h->ex_end != h->nex;  // a right interface line: its right-hand owner's pointwise terms
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // the forms the solvers launch run specialised kernels: the transposed divergence (yp alone out), the transposed
  // gradient (zc alone in; yu, yv out) and the velocity rows (zu, zv in; yu, yv out); anything else the full form
  const bool uv_in = zu || zv, uv_out_only = !yp && !yT;
  constexpr int kGradT = NT_ZC | NT_YUV, kDivT = NT_ZUV | NT_ZC | NT_YP, kVelT = NT_ZUV | NT_YUV;
  const int st = dispatch_order(h->P, [&](auto PC) {
    constexpr int P = decltype(PC)::value;
    if (yp && !yu && !yv && !yT) return launch_ns_transpose<P, kDivT>(a, open_right, s);
    if (uv_out_only && !uv_in) return launch_ns_transpose<P, kGradT>(a, open_right, s);
    if (uv_out_only && !zc) return launch_ns_transpose<P, kVelT>(a, open_right, s);
    return launch_ns_transpose<P, NT_ALL>(a, open_right, s);
  });
  if (st) return st;
  return hip_check(hipGetLastError(), "ns apply (transpose) launch");
}

}  // namespace sem

extern "C" {

int sem_ns_apply_transpose(sem_handle* h, const sem_ns_desc* d, const double* zu, const double* zv, const double* zc,
                           double* yu, double* yv, double* yp, double* yT, void* stream) {
  return sem::ns_transpose("sem_ns_apply_transpose", false, h, d, zu, zv, zc, yu, yv, yp, yT, stream);
}

int sem_ns_apply_transpose_part(sem_handle* h, const sem_ns_desc* d, const double* zu, const double* zv, const double* zc,
                                double* yu, double* yv, double* yp, double* yT, void* stream) {
  return sem::ns_transpose("sem_ns_apply_transpose_part", true, h, d, zu, zv, zc, yu, yv, yp, yT, stream);
}

}  // extern "C"
