// Host test of the apply-kernel selection policy (sem_amd/csrc/apply_select.h): a stand-alone program, built by
// tests/test_apply_select.py with the host compiler and its address / undefined-behaviour sanitizers.  It loads
// no library and needs no GPU.  Exit status 0 = every case holds; each failure prints one line.
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/sem_ops.h"
#include "../../sem_amd/csrc/apply_select.h"

using namespace sem;

static int failures = 0;

static void fail(const char* what, const std::string& got) {
  std::printf("FAIL %s: got %s\n", what, got.c_str());
  ++failures;
}

static void expect_kind(const char* what, const ApplyChoice& c, ApplyKind kind) {
  if (c.status != SEM_OK || c.kind != kind)
    fail(what, "status " + std::to_string(c.status) + " kind " + std::to_string(static_cast<int>(c.kind)) + " (" +
                   c.message + ")");
}

static void expect_status(const char* what, const ApplyChoice& c, int status, const char* word) {
  if (c.status != status || std::string(c.message).find(word) == std::string::npos)
    fail(what, "status " + std::to_string(c.status) + " (" + c.message + ")");
}

static void expect_name(const char* what, const std::string& got, const char* want) {
  if (got != want) fail(what, got);
}

static void expect(const char* what, bool ok) {
  if (!ok) fail(what, "false");
}

// A whole-mesh handle of order P whose lines hold NY nodes and whose local vector holds n_local.
static ApplyMesh mesh(int P, int64_t NY, int64_t n_local, int nex = 64) {
  return {P, nex, static_cast<int>((NY - 1) / P), 0, nex, NY, n_local};
}

int main() {
  const int64_t lim = int64_t(1) << 28;
  const int P = 8;
  const int64_t NY = 1025, halo = (P + 1) * NY;  // 9225

  // ---- the offset limit n_local + (P + 1) N_y < 2^28, per algo
  const ApplyMesh in = mesh(P, NY, lim - halo - 1), out = mesh(P, NY, lim - halo), big = mesh(P, NY, lim);
  expect("band_fits below", band_fits(in));
  expect("band_fits at", !band_fits(out));
  expect_kind("fits AUTO", select_apply(in, SEM_ALGO_AUTO, 0, 0, 0), ApplyKind::Band);
  expect_kind("fits BAND", select_apply(in, SEM_ALGO_BAND, 0, 0, 0), ApplyKind::Band);
  expect_kind("fits MFMA", select_apply(in, SEM_ALGO_MFMA, 0, 0, 0), ApplyKind::BandMfma);
  expect_kind("past AUTO", select_apply(out, SEM_ALGO_AUTO, 0, 0, 0), ApplyKind::Column);
  expect_status("past BAND", select_apply(out, SEM_ALGO_BAND, 0, 0, 0), SEM_EUNSUPPORTED, "band path");
  expect_status("past MFMA", select_apply(out, SEM_ALGO_MFMA, 0, 0, 0), SEM_EUNSUPPORTED, "MFMA path");
  expect_status("2^28 MFMA", select_apply(big, SEM_ALGO_MFMA, 0, 0, 0), SEM_EUNSUPPORTED, "MFMA path");
  expect_kind("2^28 VALU", select_apply(big, SEM_ALGO_VALU, 0, 0, 0), ApplyKind::Valu);
  expect_kind("2^28 COLUMN", select_apply(big, SEM_ALGO_COLUMN, 0, 0, 0), ApplyKind::Column);
  expect_kind("small VALU", select_apply(in, SEM_ALGO_VALU, 0, 0, 0), ApplyKind::Valu);
  expect_kind("small COLUMN", select_apply(in, SEM_ALGO_COLUMN, 0, 0, 0), ApplyKind::Column);

  // ---- element-position ranges (ncols = 64: positions 0..64)
  expect_kind("range AUTO", select_apply(in, SEM_ALGO_AUTO, 0, 65, 0), ApplyKind::Band);
  expect_kind("range BAND", select_apply(in, SEM_ALGO_BAND, 3, 4, 0), ApplyKind::Band);
  for (int algo : {SEM_ALGO_VALU, SEM_ALGO_MFMA, SEM_ALGO_COLUMN})
    expect_status("range other algo", select_apply(in, algo, 0, 1, 0), SEM_EUNSUPPORTED, "element-position");
  expect_status("range past AUTO", select_apply(out, SEM_ALGO_AUTO, 0, 1, 0), SEM_EUNSUPPORTED, "element-position");
  expect_status("range past BAND", select_apply(out, SEM_ALGO_BAND, 0, 1, 0), SEM_EUNSUPPORTED, "element-position");
  expect_status("range empty", select_apply(in, SEM_ALGO_AUTO, 2, 2, 0), SEM_EINVAL, "range");
  expect_status("range reversed", select_apply(in, SEM_ALGO_AUTO, 3, 2, 0), SEM_EINVAL, "range");
  expect_status("range negative", select_apply(in, SEM_ALGO_AUTO, -1, 2, 0), SEM_EINVAL, "range");
  expect_status("range long", select_apply(in, SEM_ALGO_AUTO, 0, 66, 0), SEM_EINVAL, "range");
  // precedence: a bad range is SEM_EINVAL before the algo or the limit is looked at
  expect_status("bad range first", select_apply(out, SEM_ALGO_VALU, 0, 66, 0), SEM_EINVAL, "range");
  expect_status("range algo before limit", select_apply(out, SEM_ALGO_MFMA, 0, 1, 0), SEM_EUNSUPPORTED, "band kernel only");

  // ---- SEM_MFMA_TILE != 0: the element-block MFMA kernel for SEM_ALGO_MFMA only, P <= 15, same offset limit
  expect_kind("eb MFMA", select_apply(in, SEM_ALGO_MFMA, 0, 0, 3), ApplyKind::ElemMfma);
  expect_status("eb MFMA past", select_apply(out, SEM_ALGO_MFMA, 0, 0, 3), SEM_EUNSUPPORTED, "MFMA path");
  expect_status("eb MFMA 2^28", select_apply(big, SEM_ALGO_MFMA, 0, 0, 3), SEM_EUNSUPPORTED, "MFMA path");
  expect_status("eb MFMA P 16", select_apply(mesh(16, NY, 1000), SEM_ALGO_MFMA, 0, 0, 3), SEM_EUNSUPPORTED, "P <= 15");
  expect_status("eb MFMA range", select_apply(in, SEM_ALGO_MFMA, 0, 1, 3), SEM_EUNSUPPORTED, "element-position");
  expect_kind("eb knob, AUTO", select_apply(in, SEM_ALGO_AUTO, 0, 0, 3), ApplyKind::Band);
  expect_kind("eb knob, BAND P 16", select_apply(mesh(16, NY, 1000), SEM_ALGO_BAND, 0, 0, 3), ApplyKind::Band);

  // ---- algo
  expect_status("algo -1", select_apply(in, -1, 0, 0, 0), SEM_EINVAL, "algo");
  expect_status("algo 5", select_apply(in, 5, 0, 0, 0), SEM_EINVAL, "algo");
  expect_status("algo before range", select_apply(in, 5, 0, 66, 0), SEM_EINVAL, "algo");

  // ---- transposed apply
  expect_kind("T whole", select_apply_transpose(in, SEM_ALGO_AUTO, 0, 16), ApplyKind::Transpose);
  ApplyMesh strip = in;
  strip.ex_end = 32;
  expect_status("T strip", select_apply_transpose(strip, SEM_ALGO_AUTO, 0, 16), SEM_EUNSUPPORTED, "whole-mesh");
  strip = in;
  strip.ex_begin = 1;
  expect_status("T strip right", select_apply_transpose(strip, SEM_ALGO_AUTO, 0, 16), SEM_EUNSUPPORTED, "whole-mesh");
  expect_status("T range", select_apply_transpose(in, SEM_ALGO_AUTO, 1, 16), SEM_EUNSUPPORTED, "element-position");
  for (int algo : {SEM_ALGO_VALU, SEM_ALGO_MFMA, SEM_ALGO_COLUMN, SEM_ALGO_BAND})
    expect_status("T algo", select_apply_transpose(in, algo, 0, 16), SEM_EUNSUPPORTED, "SEM_ALGO_AUTO");
  expect_status("T order", select_apply_transpose(mesh(17, NY, 1000), SEM_ALGO_AUTO, 0, 16), SEM_EUNSUPPORTED, "order");
  expect_status("T past", select_apply_transpose(out, SEM_ALGO_AUTO, 0, 16), SEM_EUNSUPPORTED, "2^28");

  // ---- coefficient mode: DPP from 2^20 nodes up, SEM_BAND_TILE = 3 / 4 overrides
  expect("imm below 2^20", !band_dpp(0, (1 << 20) - 1));
  expect("dpp at 2^20", band_dpp(0, 1 << 20));
  expect("tile 3 forces dpp", band_dpp(3, 100));
  expect("tile 4 forces imm", !band_dpp(4, int64_t(1) << 24));
  expect("tile 3 keeps dpp", band_dpp(3, int64_t(1) << 24));
  expect("tile 4 keeps imm", !band_dpp(4, 100));

  // ---- MALL predicate 32 n_local < 128 MiB and its two cache-policy mappings
  const int64_t mall = (int64_t(128) << 20) / 32;
  expect("mall below", fits_mall(mall - 1));
  expect("mall at", !fits_mall(mall));
  expect("band cpol", band_cpol(mall - 1) == 3 && band_cpol(mall) == 256);
  expect("transpose cpol", transpose_cpol(mall - 1) == 3 && transpose_cpol(mall) == 0);

  // ---- tile shapes
  static_assert(BandShape<1>::TXE == 4 && BandShape<1>::TYE == 64 && BandShape<1>::NS == 1, "P = 1");
  static_assert(BandShape<4>::TXE == 2 && BandShape<4>::TYE == 16 && BandShape<4>::NS == 2, "P = 4");
  static_assert(BandShape<8>::TXE == 1 && BandShape<8>::TYE == 8 && BandShape<8>::NS == 2, "P = 8");
  static_assert(BandShape<16>::TXE == 1 && BandShape<16>::TYE == 4 && BandShape<16>::NS == 2, "P = 16");

  // ---- names (the strings tests/test_gpu_apply.py expects from the library for the same inputs)
  const int64_t n4 = 13 * 9, n1 = 3 * 3, n16 = 17 * 17, nlo = 1017 * 1025, nhi = 1025 * 1025;
  expect_name("P4 band", apply_kernel_name(ApplyKind::Band, mesh(4, 4 + 1, n4), 0, 0), "sem::apply_band_kp<4, 2, 16, 2>");
  expect_name("P4 band dpp", apply_kernel_name(ApplyKind::Band, mesh(4, 4 + 1, n4), 3, 0), "sem::apply_band_kp<4, 2, 16, 2, dpp>");
  expect_name("P4 band struct", apply_kernel_name(ApplyKind::Band, mesh(4, 4 + 1, n4), 0, -1), "sem::apply_band<4, 2, 16, 2>");
  expect_name("P4 column", apply_kernel_name(ApplyKind::Column, mesh(4, 4 + 1, n4), 0, 0), "sem::apply_tp_col<4, 2, 64, 1>");
  expect_name("P4 mfma", apply_kernel_name(ApplyKind::BandMfma, mesh(4, 4 + 1, n4), 0, 0), "sem::apply_bmfma<4, 16 x 64>");
  expect_name("P4 valu", apply_kernel_name(ApplyKind::Valu, mesh(4, 4 + 1, n4), 0, 0), "sem::apply_tp_valu<4>");
  expect_name("P4 transpose", apply_kernel_name(ApplyKind::Transpose, mesh(4, 4 + 1, n4), 0, 0), "sem::apply_transpose<4>");
  expect_name("P1 band", apply_kernel_name(ApplyKind::Band, mesh(1, 1 + 1, n1), 0, 0), "sem::apply_band_kp<1, 4, 64, 1>");
  expect_name("P1 mfma", apply_kernel_name(ApplyKind::BandMfma, mesh(1, 1 + 1, n1), 0, 0), "sem::apply_bmfma<1, 16 x 64>");
  expect_name("P16 band", apply_kernel_name(ApplyKind::Band, mesh(16, 16 + 1, n16), 0, 0), "sem::apply_band_kp<16, 1, 4, 2>");
  expect_name("P16 mfma", apply_kernel_name(ApplyKind::BandMfma, mesh(16, 16 + 1, n16), 0, 0), "sem::apply_bmfma<16, 16 x 64>");
  expect("127 x 128 below 2^20", nlo == 1042425 && nlo < (1 << 20));
  expect_name("P8 127x128", apply_kernel_name(ApplyKind::Band, mesh(8, 8 + 1, nlo), 0, 0), "sem::apply_band_kp<8, 1, 8, 2>");
  expect_name("P8 128x128", apply_kernel_name(ApplyKind::Band, mesh(8, 8 + 1, nhi), 0, 0), "sem::apply_band_kp<8, 1, 8, 2, dpp>");
  expect_name("P8 128x128 imm", apply_kernel_name(ApplyKind::Band, mesh(8, 8 + 1, nhi), 4, 0), "sem::apply_band_kp<8, 1, 8, 2>");

  const ApplyMesh e64 = {8, 64, 64, 0, 64, 513, 513 * 513}, e128 = {8, 128, 128, 0, 128, 1025, nhi};
  expect_name("P8 64x64 eb", apply_kernel_name(ApplyKind::ElemMfma, e64, 0, 0), "sem::apply_tp_mfma<8, 2, 2, 4, false, true>");
  expect_name("P8 128x128 eb", apply_kernel_name(ApplyKind::ElemMfma, e128, 0, 0), "sem::apply_tp_mfma<8, 4, 4, 4, true, false>");

  if (failures) {
    std::printf("%d case(s) failed\n", failures);
    return 1;
  }
  std::printf("apply_select: all cases hold\n");
  return 0;
}
