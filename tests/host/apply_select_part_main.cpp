// Host test of select_apply_transpose_part (sem_amd/csrc/apply_select.h): a stand-alone program, built by
// tests/test_apply_select_part.py with the host compiler and its address / undefined-behaviour sanitizers.  It
// loads no library and needs no GPU.  Exit status 0 = every case holds; each failure prints one line.
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/sem_ops.h"
#include "../../sem_amd/csrc/apply_select.h"

using namespace sem;

static int failures = 0;

static void fail(const char* what, const ApplyChoice& c) {
  std::printf("FAIL %s: got status %d kind %d (%s)\n", what, c.status, static_cast<int>(c.kind), c.message);
  ++failures;
}

static void expect_transpose(const char* what, const ApplyChoice& c) {
  if (c.status != SEM_OK || c.kind != ApplyKind::Transpose) fail(what, c);
}

static void expect_status(const char* what, const ApplyChoice& c, int status, const char* word) {
  if (c.status != status || std::string(c.message).find(word) == std::string::npos) fail(what, c);
}

// A handle of order P holding element columns [eb, ee) of nex, lines of NY nodes, a local vector of n_local.
static ApplyMesh mesh(int P, int64_t NY, int64_t n_local, int eb, int ee, int nex = 64) {
  return {P, nex, P > 0 ? static_cast<int>((NY - 1) / P) : 0, eb, ee, NY, n_local};
}

int main() {
  const int64_t lim = int64_t(1) << 28;
  const int P = 8;
  const int64_t NY = 1025, halo = (P + 1) * NY;
  const ApplyMesh whole = mesh(P, NY, 1000, 0, 64), left = mesh(P, NY, 1000, 0, 24), mid = mesh(P, NY, 1000, 24, 25),
                  right = mesh(P, NY, 1000, 25, 64);

  // ---- every kind of handle, without a range
  expect_transpose("whole", select_apply_transpose_part(whole, SEM_ALGO_AUTO, 0, 0, 16));
  expect_transpose("left strip", select_apply_transpose_part(left, SEM_ALGO_AUTO, 0, 0, 16));
  expect_transpose("one-column strip", select_apply_transpose_part(mid, SEM_ALGO_AUTO, 0, 0, 16));
  expect_transpose("right strip", select_apply_transpose_part(right, SEM_ALGO_AUTO, 0, 0, 16));

  // ---- element-position ranges inside [0, ncols + 1)
  expect_transpose("whole all", select_apply_transpose_part(whole, SEM_ALGO_AUTO, 0, 65, 16));
  expect_transpose("whole closing", select_apply_transpose_part(whole, SEM_ALGO_AUTO, 64, 65, 16));
  expect_transpose("left first", select_apply_transpose_part(left, SEM_ALGO_AUTO, 0, 1, 16));
  expect_transpose("left interior", select_apply_transpose_part(left, SEM_ALGO_AUTO, 1, 24, 16));
  expect_transpose("left closing", select_apply_transpose_part(left, SEM_ALGO_AUTO, 24, 25, 16));
  expect_transpose("mid first", select_apply_transpose_part(mid, SEM_ALGO_AUTO, 0, 1, 16));
  expect_transpose("mid closing", select_apply_transpose_part(mid, SEM_ALGO_AUTO, 1, 2, 16));
  expect_transpose("right all", select_apply_transpose_part(right, SEM_ALGO_AUTO, 0, 40, 16));

  // ---- ranges outside it: SEM_EINVAL (the range counts the handle's OWN columns, not the mesh's)
  expect_status("empty", select_apply_transpose_part(left, SEM_ALGO_AUTO, 2, 2, 16), SEM_EINVAL, "range");
  expect_status("reversed", select_apply_transpose_part(left, SEM_ALGO_AUTO, 3, 2, 16), SEM_EINVAL, "range");
  expect_status("negative", select_apply_transpose_part(left, SEM_ALGO_AUTO, -1, 2, 16), SEM_EINVAL, "range");
  expect_status("long", select_apply_transpose_part(left, SEM_ALGO_AUTO, 0, 26, 16), SEM_EINVAL, "range");
  expect_status("mid long", select_apply_transpose_part(mid, SEM_ALGO_AUTO, 0, 3, 16), SEM_EINVAL, "range");
  expect_status("mesh-wide on strip", select_apply_transpose_part(right, SEM_ALGO_AUTO, 0, 65, 16), SEM_EINVAL, "range");
  expect_status("begin, no end", select_apply_transpose_part(left, SEM_ALGO_AUTO, 1, 0, 16), SEM_EINVAL, "range");
  expect_status("negative end", select_apply_transpose_part(left, SEM_ALGO_AUTO, 0, -1, 16), SEM_EINVAL, "range");

  // ---- algo: one kernel
  for (int algo : {int(SEM_ALGO_VALU), int(SEM_ALGO_MFMA), int(SEM_ALGO_COLUMN), int(SEM_ALGO_BAND), -1, 5}) {
    expect_status("algo", select_apply_transpose_part(left, algo, 0, 0, 16), SEM_EUNSUPPORTED, "SEM_ALGO_AUTO");
    expect_status("algo ranged", select_apply_transpose_part(left, algo, 0, 1, 16), SEM_EUNSUPPORTED, "SEM_ALGO_AUTO");
  }

  // ---- polynomial order
  expect_transpose("P 1", select_apply_transpose_part(mesh(1, 65, 1000, 1, 3), SEM_ALGO_AUTO, 0, 0, 16));
  expect_transpose("P 16", select_apply_transpose_part(mesh(16, NY, 1000, 1, 3), SEM_ALGO_AUTO, 0, 0, 16));
  expect_status("P 17", select_apply_transpose_part(mesh(17, NY, 1000, 1, 3), SEM_ALGO_AUTO, 0, 0, 16), SEM_EUNSUPPORTED, "order");
  expect_status("P 0", select_apply_transpose_part(mesh(0, NY, 1000, 1, 3), SEM_ALGO_AUTO, 0, 0, 16), SEM_EUNSUPPORTED, "order");
  expect_status("P 9 of 8", select_apply_transpose_part(mesh(9, NY, 1000, 1, 3), SEM_ALGO_AUTO, 0, 0, 8), SEM_EUNSUPPORTED, "order");

  // ---- the offset limit n_local + (P + 1) N_y < 2^28 counts the handle's LOCAL vector
  const ApplyMesh in = mesh(P, NY, lim - halo - 1, 8, 40), out = mesh(P, NY, lim - halo, 8, 40);
  expect_transpose("below the limit", select_apply_transpose_part(in, SEM_ALGO_AUTO, 0, 0, 16));
  expect_transpose("below the limit, ranged", select_apply_transpose_part(in, SEM_ALGO_AUTO, 0, 1, 16));
  expect_status("at the limit", select_apply_transpose_part(out, SEM_ALGO_AUTO, 0, 0, 16), SEM_EUNSUPPORTED, "2^28");
  expect_status("at the limit, ranged", select_apply_transpose_part(out, SEM_ALGO_AUTO, 0, 1, 16), SEM_EUNSUPPORTED, "2^28");

  // ---- precedence: range, then algo, then order, then the limit
  expect_status("range first", select_apply_transpose_part(mesh(17, NY, lim, 8, 40), SEM_ALGO_BAND, 0, 34, 16), SEM_EINVAL, "range");
  expect_status("algo second", select_apply_transpose_part(mesh(17, NY, lim, 8, 40), SEM_ALGO_BAND, 0, 33, 16), SEM_EUNSUPPORTED, "SEM_ALGO_AUTO");
  expect_status("order third", select_apply_transpose_part(mesh(17, NY, lim, 8, 40), SEM_ALGO_AUTO, 0, 33, 16), SEM_EUNSUPPORTED, "order");

  // ---- the whole-mesh form keeps its refusals
  expect_status("old: strip", select_apply_transpose(left, SEM_ALGO_AUTO, 0, 16), SEM_EUNSUPPORTED, "whole-mesh");
  expect_status("old: range", select_apply_transpose(whole, SEM_ALGO_AUTO, 1, 16), SEM_EUNSUPPORTED, "element-position");
  expect_transpose("old: whole", select_apply_transpose(whole, SEM_ALGO_AUTO, 0, 16));

  if (failures) {
    std::printf("%d case(s) failed\n", failures);
    return 1;
  }
  std::printf("apply_select_part: all cases hold\n");
  return 0;
}
