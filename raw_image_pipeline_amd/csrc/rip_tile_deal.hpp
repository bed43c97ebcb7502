// rip_tile_deal.hpp -- the order in which the persistent workgroups of the ring kernels (rip_remap.hip, rip_fused.hip) visit the
// tiles of a remap plan: the launcher's half (tile_deal_geometry) and the kernels' half (TileDeal).  Integer arithmetic only and no
// device intrinsics, so tests/cpp/tile_deal_test.cpp walks the very same code on the host.
#pragma once

namespace rip {

// What the launcher hands to the kernels (RemapTiledParams::deal_run / deal_order / deal_shift).
struct TileDealGeometry {
  int run;    // tiles per run of the round-robin deal; 0 = one contiguous range of tiles per XCD
  int order;  // inside a run: 0 = row-major, 1 = column strips (needs a run of exactly 2^shift whole tile rows)
  int shift;  // log2 of the strip height in tile rows (order 1)
};

// remap_deal: run length in tile rows (Tunables::remap_deal), 0 = contiguous; remap_order: Tunables::remap_order (0 row-major,
// 1 column strips, 2 column strips where they deal out evenly over the eight XCDs and row-major elsewhere; anything else: 0).
// Row-major runs are "about" remap_deal tile rows, sized so that every XCD gets the same number of runs (a ragged last run at
// most).  Column strips need whole tile rows and a power of two of them: remap_deal rounded down to one.
inline TileDealGeometry tile_deal_geometry(int tiles_x, int tiles_y, int remap_deal, int remap_order) {
  TileDealGeometry g = {0, 0, 0};
  if (remap_deal <= 0 || tiles_x <= 0 || tiles_y <= 0) return g;
  const long long ntiles = (long long)tiles_x * tiles_y;
  if (remap_order == 1 || remap_order == 2) {
    int shift = 0;  // no higher than the first power of two that holds every tile row: the run stays below 2 * ntiles
    while ((2 << shift) <= remap_deal && (1 << shift) < tiles_y) shift++;
    // Strips of whole tile rows cannot be sized to the plan as the row-major runs below are: 19 strips (1920 x 1200) give three XCDs
    // three strips and five XCDs two, and the launch takes as long as the fullest share (measured: +20 %; 3840 x 2160, 34
    // strips: +16 %).  Order 2 therefore takes column strips only where they deal out evenly, a ragged last strip apart.
    const int strips = (tiles_y + (1 << shift) - 1) >> shift;
    if (remap_order == 1 || strips % 8 == 0) {
      g.run = tiles_x << shift;
      g.order = 1;
      g.shift = shift;
      return g;
    }
  }
  const long long runs_per_xcd = ((long long)tiles_y + 8ll * remap_deal - 1) / (8ll * remap_deal);
  g.run = (int)((ntiles + 8 * runs_per_xcd - 1) / (8 * runs_per_xcd));
  return g;
}

// How the persistent workgroups of the ring kernels find their tiles.  Workgroup b runs on XCD b % 8 (observed dispatch order;
// speed only) and takes the positions ti = b / 8, b / 8 + gridDim.x / 8, ... of that XCD's share.  Rounds 1-5 gave every XCD one
// contiguous range of tiles (eight bands of the image in flight at once, each marching down on its own).  Round 6: runs of
// `run` consecutive tiles (about one tile row) are dealt round-robin, so the tiles in flight on the whole chip form ONE band of
// consecutive tile rows, read and written by all XCDs together -- the same requests, served 5 % faster at 4 frames per visit
// and 12 % faster with 8 (which the contiguous deal could not use: its XCDs drift apart).  EXPERIMENTS.md "the deal".
// order 1: a run is R = 2^shift whole tile rows and is walked in column strips, position i -> row i % R, column i / R of the run,
// so that consecutive positions -- consecutive workgroups of one XCD -- are vertical neighbours and the horizontal neighbour
// comes R positions later: both halos of a tile's source rectangle are then in the XCD's L2 when its neighbours ask for them
// (row-major, the vertical neighbour comes tiles_x positions later).  A ragged last run (fewer than R tile rows) is walked
// row-major.  Plan words and tile descriptors stay indexed by tile number; only the visiting order changes.
struct TileDeal {
  int run, per_xcd, ntiles, tiles_x, order, shift;
  __device__ __forceinline__ TileDeal(int tiles_x_, int tiles_y_, int run_, int order_, int shift_)
      : run(run_), ntiles(tiles_x_ * tiles_y_), tiles_x(tiles_x_), order(run_ > 0 && run_ == (tiles_x_ << shift_) ? order_ : 0), shift(shift_) {
    per_xcd = run > 0 ? ((ntiles + run - 1) / run + 7) / 8 * run : (ntiles + 7) / 8;
  }
  // tile at position ti of XCD xcd; -1: none here (a ragged last run), keep going; -2: past the end of a contiguous range
  __device__ __forceinline__ int tile(int ti, int xcd) const {
    if (run > 0) {
      const int r = ti / run;
      const int i = ti - r * run;
      const int base = (r * 8 + xcd) * run;
      int t = base + i;
      if (order == 1 && base + run <= ntiles) t = base + (i & ((1 << shift) - 1)) * tiles_x + (i >> shift);
      return t < ntiles ? t : -1;
    }
    const int t = xcd * per_xcd + ti;
    return t < ntiles ? t : -2;
  }
};

}  // namespace rip
