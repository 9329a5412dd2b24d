// Apply-kernel selection: which kernel sem_apply / sem_apply_transpose(_part) run for a handle, an algo, an
// element-position range and the tuning knobs, the tile shapes and thresholds that decision rests on, and the
// kernel names reported for it.  Pure host functions of plain values (no HIP header): sem_ops.hip, the band
// and transposed launchers and tests/host/apply_select_main.cpp all read the policy from here.
#pragma once

#include <cstdint>
#include <string>

#include "../../include/sem_ops.h"

namespace sem {

enum class ApplyKind { Band, BandMfma, ElemMfma, Column, Valu, Transpose };

// What the policy reads of a handle.
struct ApplyMesh {
  int P, nex, ney, ex_begin, ex_end;
  int64_t NY, n_local;
};

// A kernel, or the status and message sem_apply / sem_apply_transpose return instead of launching.
struct ApplyChoice {
  int status;
  ApplyKind kind;
  const char* message;
};
constexpr ApplyChoice chosen(ApplyKind k) { return {SEM_OK, k, ""}; }
constexpr ApplyChoice refused(int status, const char* message) { return {status, ApplyKind::Valu, message}; }

// The band, band-MFMA and transposed kernels stage through 32-bit buffer byte offsets, an absent column at
// 2^31 plus a line offset: those stay outside the buffer while n_local + (P + 1) N_y < 2^28 (apply_band.hip,
// band_body).  The element-block MFMA kernel, which also
// addresses through 32-bit buffer offsets, runs under the same gate: one refusal rule for SEM_ALGO_MFMA.
constexpr bool band_fits(int P, int64_t NY, int64_t n_local) { return n_local + (P + 1) * NY < (int64_t(1) << 28); }
constexpr bool band_fits(const ApplyMesh& m) { return band_fits(m.P, m.NY, m.n_local); }

// Band tile shape per order (band and transposed kernels): ~64 columns (TYE = 64/P element positions) so a
// wave spans one tile line; TXE element columns for ~512-node tiles; rows of an element split over NS threads.
constexpr int band_tye(int P) { return 64 / P > 0 ? 64 / P : 1; }
constexpr int band_txe(int P) { return 8 / P > 4 ? 4 : (8 / P > 0 ? 8 / P : 1); }
constexpr int band_ns(int P) { return P >= 2 ? 2 : 1; }
template <int P>
struct BandShape {
  static constexpr int TYE = band_tye(P), TXE = band_txe(P), NS = band_ns(P);
};
// Band-MFMA tile (BMCfg, apply_band.hip): TXE whole element columns in at most 16 lines, kBmfmaNB column blocks.
constexpr int bmfma_txe(int P) { return 16 / P > 0 ? 16 / P : 1; }
constexpr int kBmfmaNB = 4;
// Element-block MFMA tile (MCfg, apply_tp.hip; SEM_MFMA_TILE != 0, P <= 15): element tiles of ~32 x 32 nodes (4
// waves, persistent) for large meshes; ~16 x 16 nodes for meshes too small to give every CU several workgroups
// (4 waves with the K and G chains as separate tasks).
constexpr int emfma_tl(int P) { return 32 / P > 0 ? 32 / P : 1; }
constexpr int emfma_ts(int P) { return 16 / P > 0 ? 16 / P : 1; }
constexpr bool emfma_large(int P, int ncols, int ney) {
  return static_cast<long long>((ncols + emfma_tl(P) - 1) / emfma_tl(P)) * ((ney + emfma_tl(P) - 1) / emfma_tl(P)) >=
         4 * 256;
}
// Column-kernel tile (CCfg, apply_tp.hip): 2 element columns x 64 lines, no row split (the other tiles of
// rounds 1-2 lost their A/B; retired in round 6).
constexpr int kColTX = 2, kColBY = 64, kColRS = 1;

// Band coefficient mode: DPP-broadcast lists from ~1M DOFs up (the issue-bound regime), fp64 immediates below
// (the launch-latency-bound meshes, whose extra coefficient loads sit on the critical path:
// profiles/r01/band/dpp_ab.txt); SEM_BAND_TILE = 3 / 4 forces DPP / immediates (the bitwise-variant tests).
constexpr bool band_dpp(int band_tile, int64_t n_local) {
  return band_tile == 3 || (band_tile != 4 && n_local >= (1 << 20));
}

// Whether the working set of one apply (~32 bytes per node) stays in the 128 MiB MALL.  The band kernels then
// run cache policy 3 (system-scope y stores, written through L2 as they are issued: no end-of-kernel L2
// writeback, 4.66 -> 4.38 us at cfg2; tools/ab_env.py, profiles/r01/band/cpol_ab.txt) and otherwise 256
// (non-temporal u, v loads; system-scope stores cost ~1 % on HBM-sized meshes); the transposed kernel 3 / 0.
constexpr bool fits_mall(int64_t n_local) { return 32LL * n_local < (128LL << 20); }
constexpr int band_cpol(int64_t n_local) { return fits_mall(n_local) ? 3 : 256; }
constexpr int transpose_cpol(int64_t n_local) { return fits_mall(n_local) ? 3 : 0; }

// sem_apply.  AUTO, measured on MI355X (tools/kbench.py): the band kernel on every mesh that fits its buffer
// offsets (it beats the other kernels from 64^2 to 1024^2 elements), the single-phase column kernel above that.
// pos_end > 0 gives an element-position range.  SEM_ALGO_MFMA is the band-form MFMA kernel; mfma_tile (the
// SEM_TUNE_MFMA_TILE knob) != 0 selects the element-block MFMA kernel of rounds 1-4 instead (A/B, P <= 15).
inline ApplyChoice select_apply(const ApplyMesh& m, int algo, int pos_begin, int pos_end, int mfma_tile) {
  if (algo < SEM_ALGO_AUTO || algo > SEM_ALGO_BAND) return refused(SEM_EINVAL, "bad algo");
  const bool legacy_mfma = algo == SEM_ALGO_MFMA && mfma_tile != 0;
  if (legacy_mfma && m.P > 15) return refused(SEM_EUNSUPPORTED, "the element-block MFMA path needs P <= 15");
  const bool ranged = pos_end > 0;
  if (ranged && (pos_begin < 0 || pos_begin >= pos_end || pos_end > m.ex_end - m.ex_begin + 1))
    return refused(SEM_EINVAL, "element-position range outside [0, ex_end - ex_begin + 1)");
  if (ranged && algo != SEM_ALGO_AUTO && algo != SEM_ALGO_BAND)
    return refused(SEM_EUNSUPPORTED, "element-position ranges are implemented by the band kernel only");
  const bool fits = band_fits(m);
  if (ranged && !fits) return refused(SEM_EUNSUPPORTED, "element-position ranges need n_local + (P+1) N_y < 2^28");
  switch (algo) {
    case SEM_ALGO_AUTO:
      return chosen(fits ? ApplyKind::Band : ApplyKind::Column);
    case SEM_ALGO_BAND:
      if (!fits) return refused(SEM_EUNSUPPORTED, "band path needs n_local + (P+1) N_y < 2^28");
      return chosen(ApplyKind::Band);
    case SEM_ALGO_MFMA:
      if (!fits) return refused(SEM_EUNSUPPORTED, "MFMA path needs n_local + (P+1) N_y < 2^28");
      return chosen(legacy_mfma ? ApplyKind::ElemMfma : ApplyKind::BandMfma);
    case SEM_ALGO_COLUMN:
      return chosen(ApplyKind::Column);
    default:
      return chosen(ApplyKind::Valu);
  }
}

// sem_apply_transpose: one kernel, whole-mesh handles, no ranges.
inline ApplyChoice select_apply_transpose(const ApplyMesh& m, int algo, int pos_end, int max_order) {
  if (m.ex_begin != 0 || m.ex_end != m.nex)
    return refused(SEM_EUNSUPPORTED, "the transposed apply is implemented for whole-mesh handles only");
  if (pos_end != 0) return refused(SEM_EUNSUPPORTED, "the transposed apply has no element-position ranges");
  if (algo != SEM_ALGO_AUTO) return refused(SEM_EUNSUPPORTED, "the transposed apply has one kernel (SEM_ALGO_AUTO)");
  if (m.P < 1 || m.P > max_order) return refused(SEM_EUNSUPPORTED, "polynomial order outside compiled range");
  if (!band_fits(m)) return refused(SEM_EUNSUPPORTED, "the transposed apply needs n_local + (P+1) N_y < 2^28");
  return chosen(ApplyKind::Transpose);
}

// sem_apply_transpose_part: the same kernel on any handle (a strip applies its own A_s^T) and any
// element-position range of it; pos_begin = pos_end = 0 gives all positions.
inline ApplyChoice select_apply_transpose_part(const ApplyMesh& m, int algo, int pos_begin, int pos_end, int max_order) {
  const bool ranged = pos_begin != 0 || pos_end != 0;
  if (ranged && (pos_begin < 0 || pos_begin >= pos_end || pos_end > m.ex_end - m.ex_begin + 1))
    return refused(SEM_EINVAL, "element-position range outside [0, ex_end - ex_begin + 1)");
  if (algo != SEM_ALGO_AUTO) return refused(SEM_EUNSUPPORTED, "the transposed apply has one kernel (SEM_ALGO_AUTO)");
  if (m.P < 1 || m.P > max_order) return refused(SEM_EUNSUPPORTED, "polynomial order outside compiled range");
  if (!band_fits(m)) return refused(SEM_EUNSUPPORTED, "the transposed apply needs n_local + (P+1) N_y < 2^28");
  return chosen(ApplyKind::Transpose);
}

// Name of the kernel family a choice launches (reports, PMC traffic matching).  band_tile, band_kp: the
// SEM_TUNE_BAND_TILE / SEM_TUNE_BAND_KP knobs.
inline std::string apply_kernel_name(ApplyKind kind, const ApplyMesh& m, int band_tile, int band_kp) {
  const int P = m.P;
  const int64_t n_local = m.n_local;
  const std::string p = std::to_string(P);
  switch (kind) {
    case ApplyKind::Band:
      return std::string(band_kp >= 0 ? "sem::apply_band_kp<" : "sem::apply_band<") + p + ", " +
             std::to_string(band_txe(P)) + ", " + std::to_string(band_tye(P)) + ", " + std::to_string(band_ns(P)) +
             (band_dpp(band_tile, n_local) ? ", dpp" : "") + ">";
    case ApplyKind::BandMfma:
      return "sem::apply_bmfma<" + p + ", " + std::to_string(bmfma_txe(P) * P) + " x " +
             std::to_string(kBmfmaNB * bmfma_txe(P) * P) + ">";
    case ApplyKind::ElemMfma: {
      const bool large = emfma_large(P, m.ex_end - m.ex_begin, m.ney);
      const std::string t = std::to_string(large ? emfma_tl(P) : emfma_ts(P));
      return "sem::apply_tp_mfma<" + p + ", " + t + ", " + t + (large ? ", 4, true, false>" : ", 4, false, true>");
    }
    case ApplyKind::Column:
      return "sem::apply_tp_col<" + p + ", " + std::to_string(kColTX) + ", " + std::to_string(kColBY) + ", " +
             std::to_string(kColRS) + ">";
    case ApplyKind::Valu:
      return "sem::apply_tp_valu<" + p + ">";
    default:
      return "sem::apply_transpose<" + p + ">";
  }
}

}  // namespace sem
