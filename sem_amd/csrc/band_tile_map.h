// Block index -> tile (tx, ty) of the band kernel (apply_band.hip, band_body), without a division.
//
// The XCD-aware remap gives each of the 8 XCDs a contiguous run of the linear tile indices L in [0, nblk) (blocks
// b and b + 8 share an XCD), and L = tx * tiles_y + ty (y fastest).  tx = L / tiles_y is formed as
//     tx = (L * mul) >> shift,   mul = ceil(2^shift / tiles_y),   shift = 31 + ceil(log2 tiles_y)
// with a 64-bit product.  Writing mul = (2^shift + e) / tiles_y, 0 <= e < tiles_y, the product is
// L / tiles_y + L e / (tiles_y 2^shift), whose floor is floor(L / tiles_y) whenever L e < 2^shift.  Since
// e < tiles_y <= 2^(shift - 31) that holds for every L <= 2^31, and mul <= 2^32 - 1 (2^31 exactly for a power of
// two).  The launcher refuses nblk > 2^31 - 1, so the map is exact for every launch; band_fits
// (n_local + (P + 1) N_y < 2^28) gives much less: nblk <= (ncols + 1)(ney + 1) < 2^28 tiles and, with
// ney + 1 <= N_y and ncols >= 1, tiles_y <= N_y < 2^28 / (2 P + 2) <= 2^26.  tiles_y and shift - 31 <= 26 therefore
// share one 32-bit word (kBandTyBits), which keeps the kernel at 14 preloaded argument SGPRs.
//
// Plain C++ for host and device: tests/host/band_tile_map_main.cpp checks it against / and % on the CPU.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SEM_HOST_DEVICE __host__ __device__
#else
#define SEM_HOST_DEVICE
#endif

namespace sem {

constexpr int kBandTyBits = 26;                             // tiles_y < 2^26 (see above)
constexpr uint32_t kBandTileMax = 0x7fffffffu;              // largest tile count of one launch

struct BandTileDiv {
  uint32_t mul;     // ceil(2^shift / tiles_y)
  uint32_t packed;  // tiles_y | (shift - 31) << kBandTyBits
};

// Host side (launch_band): the reciprocal of tiles_y in [1, 2^26).
constexpr BandTileDiv band_tile_div(uint32_t tiles_y) {
  uint32_t lg = 0;  // ceil(log2 tiles_y)
  while ((uint64_t(1) << lg) < tiles_y) ++lg;
  const uint64_t pw = uint64_t(1) << (31 + lg);
  return {static_cast<uint32_t>((pw + tiles_y - 1) / tiles_y), tiles_y | (lg << kBandTyBits)};
}

struct BandTile {
  int tx, ty;
};

// L -> (L / tiles_y, L % tiles_y), L <= 2^31.
SEM_HOST_DEVICE inline BandTile band_tile_split(uint32_t L, uint32_t mul, uint32_t packed) {
  const uint32_t tiles_y = packed & ((1u << kBandTyBits) - 1), shift = 31 + (packed >> kBandTyBits);
  const uint32_t tx = static_cast<uint32_t>((static_cast<uint64_t>(L) * mul) >> shift);
  return {static_cast<int>(tx), static_cast<int>(L - tx * tiles_y)};
}

// Linear tile index of block bid of nblk: XCD bid & 7 holds the indices of its blocks as one contiguous run.
SEM_HOST_DEVICE inline uint32_t band_tile_linear(uint32_t bid, uint32_t nblk) {
  const uint32_t xcd = bid & 7, rk = bid >> 3, q8 = nblk >> 3, rem = nblk & 7;
  return (xcd < rem ? xcd * (q8 + 1) : rem * (q8 + 1) + (xcd - rem) * q8) + rk;
}

SEM_HOST_DEVICE inline BandTile band_tile_map(uint32_t bid, uint32_t nblk, uint32_t mul, uint32_t packed) {
  return band_tile_split(band_tile_linear(bid, nblk), mul, packed);
}

}  // namespace sem
