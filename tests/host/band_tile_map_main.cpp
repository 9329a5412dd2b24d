// Host test of the band kernel's division-free tile map (sem_amd/csrc/band_tile_map.h): a stand-alone program
// over the header alone, built by tests/test_band_tile_map.py with the host compiler's sanitizers.
//
//  1. the reciprocal split equals / and % for every tiles_y in 1..4096 and every L < 2^20;
//  2. for every tiles_y up to the derived bound (tiles_y < 2^26): L = k tiles_y - 1, k tiles_y, k tiles_y + 1 for
//     k = 1, the middle and the largest k with L <= 2^31 - 1 (the launcher's tile limit; band_fits allows fewer
//     tiles), and for tiles_y <= 2^16 the neighbouring k as well;
//  3. blockIdx -> (tx, ty), XCD remap included, is a bijection onto the tiles_x x tiles_y grid for every
//     nblk in 1..600 (every factorisation) and for 65 x 9 = 585.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../sem_amd/csrc/band_tile_map.h"

namespace {

std::atomic<int> failures{0};
constexpr uint32_t kThreads = 4;  // the two exhaustive parts are dealt to threads by tiles_y % kThreads

void fail(const char* what, uint64_t L, uint32_t d, int tx, int ty) {
  if (failures++ < 20)
    std::fprintf(stderr, "FAIL %s: L=%llu tiles_y=%u -> (%d, %d), want (%llu, %llu)\n", what,
                 static_cast<unsigned long long>(L), d, tx, ty, static_cast<unsigned long long>(L / d),
                 static_cast<unsigned long long>(L % d));
}

void check(const char* what, uint32_t L, uint32_t d, const sem::BandTileDiv& td) {
  const sem::BandTile t = sem::band_tile_split(L, td.mul, td.packed);
  if (static_cast<uint32_t>(t.tx) != L / d || static_cast<uint32_t>(t.ty) != L % d) fail(what, L, d, t.tx, t.ty);
}

// every L of [0, n): the quotient and remainder are advanced by counting, which is what / and % return
void sweep(uint32_t d, uint32_t n) {
  const sem::BandTileDiv td = sem::band_tile_div(d);
  uint32_t q = 0, r = 0;
  for (uint32_t L = 0; L < n; ++L) {
    const sem::BandTile t = sem::band_tile_split(L, td.mul, td.packed);
    if (static_cast<uint32_t>(t.tx) != q || static_cast<uint32_t>(t.ty) != r) fail("sweep", L, d, t.tx, t.ty);
    if (++r == d) r = 0, ++q;
  }
  // the counters themselves against the operators, at the end of the range
  if (q != n / d || r != n % d) fail("sweep counters", n, d, static_cast<int>(q), static_cast<int>(r));
}

void edges(uint32_t d, bool wide) {
  const sem::BandTileDiv td = sem::band_tile_div(d);
  if ((td.packed & ((1u << sem::kBandTyBits) - 1)) != d) fail("packed tiles_y", 0, d, 0, 0);
  const uint64_t lmax = sem::kBandTileMax;  // largest L + 1 a launch can hold
  const uint64_t kmax = lmax / d;
  const uint64_t ks[] = {1, kmax / 2, kmax, 0, 2, 3, kmax / 2 - 1, kmax / 2 + 1, kmax - 2, kmax - 1};
  const int nk = wide ? 10 : 3;
  for (int i = 0; i < nk; ++i) {
    const uint64_t k = ks[i];
    if (k > kmax) continue;  // wrapped below 0 for a small kmax
    for (int o = -1; o <= 1; ++o) {
      const int64_t L = static_cast<int64_t>(k * d) + o;
      if (L < 0 || static_cast<uint64_t>(L) > lmax) continue;
      check("edge", static_cast<uint32_t>(L), d, td);
    }
  }
  check("edge", static_cast<uint32_t>(lmax), d, td);
}

void bijection(uint32_t tiles_x, uint32_t tiles_y) {
  const uint32_t nblk = tiles_x * tiles_y;
  const sem::BandTileDiv td = sem::band_tile_div(tiles_y);
  std::vector<int> seen(nblk, 0);
  for (uint32_t bid = 0; bid < nblk; ++bid) {
    const uint32_t L = sem::band_tile_linear(bid, nblk);
    if (L >= nblk) {
      fail("remap range", L, tiles_y, static_cast<int>(bid), static_cast<int>(nblk));
      continue;
    }
    const sem::BandTile t = sem::band_tile_map(bid, nblk, td.mul, td.packed);
    if (t.tx < 0 || t.ty < 0 || static_cast<uint32_t>(t.tx) >= tiles_x || static_cast<uint32_t>(t.ty) >= tiles_y) {
      fail("tile range", L, tiles_y, t.tx, t.ty);
      continue;
    }
    ++seen[static_cast<uint32_t>(t.tx) * tiles_y + static_cast<uint32_t>(t.ty)];
  }
  for (uint32_t i = 0; i < nblk; ++i)
    if (seen[i] != 1) fail("bijection", i, tiles_y, seen[i], static_cast<int>(nblk));
}

}  // namespace

int main() {
  const uint32_t dmax = (1u << sem::kBandTyBits) - 1;
  std::vector<std::thread> pool;
  for (uint32_t t = 0; t < kThreads; ++t)
    pool.emplace_back([t, dmax] {
      for (uint32_t d = 1 + t; d <= 4096; d += kThreads) sweep(d, 1u << 20);
      for (uint32_t d = 1 + t; d <= dmax; d += kThreads) edges(d, d <= (1u << 16));
    });
  for (auto& th : pool) th.join();

  for (uint32_t nblk = 1; nblk <= 600; ++nblk)
    for (uint32_t ty = 1; ty <= nblk; ++ty)
      if (nblk % ty == 0) bijection(nblk / ty, ty);
  bijection(65, 9);

  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures.load());
    return 1;
  }
  std::puts("band tile map ok");
  return 0;
}
