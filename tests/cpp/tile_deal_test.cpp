// TileDeal and tile_deal_geometry of csrc/rip_tile_deal.hpp on the host (hip_host_stub): the loop of the ring kernels over their
// tiles, restated for every workgroup of a grid, must visit every tile of the plan exactly once under every run length and order --
// ragged last runs (fewer tile rows than the strip height), fewer runs than XCDs, one tile, grids smaller and larger than the share.
// Under order 1 a full run is walked in column strips (position i -> run_base + (i % R) * tiles_x + i / R, R a power of two of whole
// tile rows); under order 0 the mapping is the one of the rounds before (restated here); order 2 is order 1 where the number of
// strips is a multiple of 8 and order 0 elsewhere; any other order is order 0.  Stand-alone: may be built with
// -fsanitize=address,undefined.
// usage: tile_deal_test
#include <hip/hip_runtime.h>
dim3 blockIdx, threadIdx, gridDim, blockDim;
#include "rip_tile.hpp"
#include "rip_tile_deal.hpp"
#include <cstdio>
#include <vector>

static int g_cases = 0, g_bad = 0;

static void fail(const char* what, int w, int h, int deal, int order, int blocks, int a, int b) {
  if (g_bad++ < 20) printf("%dx%d remap_deal %d order %d blocks %d: %s (%d, %d)\n", w, h, deal, order, blocks, what, a, b);
}

// the tile loop of remap_ring_kernel / remap_bayer_ring_kernel for every workgroup of a grid of `blocks`
static void walk(int w, int h, int remap_deal, int remap_order, int blocks) {
  const int tiles_x = (w + rip::kRemapTileW - 1) / rip::kRemapTileW, tiles_y = (h + rip::kRemapTileH - 1) / rip::kRemapTileH;
  const int ntiles = tiles_x * tiles_y;
  const rip::TileDealGeometry g = rip::tile_deal_geometry(tiles_x, tiles_y, remap_deal, remap_order);
  g_cases++;
  if (remap_deal == 0 && g.run != 0) fail("contiguous deal with a run", w, h, remap_deal, remap_order, blocks, g.run, 0);
  if (remap_deal > 0 && g.run <= 0) fail("no run", w, h, remap_deal, remap_order, blocks, g.run, 0);
  if (g.order == 1) {
    const int R = 1 << g.shift;
    // remap_deal rounded down to a power of two, but no more than the first power of two that holds every tile row
    const bool capped = R >= tiles_y && (R == 1 || R / 2 < tiles_y);
    if ((remap_order != 1 && remap_order != 2) || (remap_order == 2 && ((tiles_y + R - 1) / R) % 8 != 0) || R > remap_deal || (2 * R <= remap_deal && !capped) || g.run != R * tiles_x) fail("strip height", w, h, remap_deal, remap_order, blocks, R, g.run);
  } else if (remap_order == 1 && remap_deal > 0) {
    fail("column strips refused", w, h, remap_deal, remap_order, blocks, g.run, g.shift);
  }
  if (g.order == 0 && remap_deal > 0) {  // the run of the rounds before: about remap_deal tile rows, the same number of runs for every XCD
    const int runs_per_xcd = (tiles_y + 8 * remap_deal - 1) / (8 * remap_deal);
    if (g.run != (ntiles + 8 * runs_per_xcd - 1) / (8 * runs_per_xcd)) fail("row-major run length", w, h, remap_deal, remap_order, blocks, g.run, runs_per_xcd);
  }
  const rip::TileDeal deal(tiles_x, tiles_y, g.run, g.order, g.shift);
  std::vector<int> seen((size_t)ntiles, 0);
  for (int b = 0; b < blocks; b++) {
    const int xcd = b & 7;
    for (int ti = b >> 3; ti < deal.per_xcd; ti += blocks >> 3) {
      const int tile = deal.tile(ti, xcd);
      if (tile == -1) continue;
      if (tile < 0) break;
      if (tile >= ntiles) {
        fail("tile out of range", w, h, remap_deal, remap_order, blocks, tile, ntiles);
        continue;
      }
      seen[(size_t)tile]++;
      if (g.run > 0) {
        const int r = ti / g.run, i = ti % g.run, base = (r * 8 + xcd) * g.run;
        int want = base + i;
        if (g.order == 1 && base + g.run <= ntiles) {
          const int R = 1 << g.shift;
          want = base + (i % R) * tiles_x + i / R;
          // the next position is the tile below, or the top of the next column of the strip
          if (i + 1 < g.run && deal.tile(ti + 1, xcd) != ((i + 1) % R ? tile + tiles_x : tile - (R - 1) * tiles_x + 1))
            fail("not a column strip", w, h, remap_deal, remap_order, blocks, tile, deal.tile(ti + 1, xcd));
        }
        if (tile != want) fail("mapping", w, h, remap_deal, remap_order, blocks, tile, want);
      } else if (tile != xcd * ((ntiles + 7) / 8) + ti) {
        fail("contiguous mapping", w, h, remap_deal, remap_order, blocks, tile, ti);
      }
    }
  }
  for (int t = 0; t < ntiles; t++)
    if (seen[(size_t)t] != 1) fail("tile not visited exactly once", w, h, remap_deal, remap_order, blocks, t, seen[(size_t)t]);
}

int main() {
  const int sizes[][2] = {{64, 16}, {200, 72}, {328, 144}, {448, 272}, {1000, 752}, {1440, 1080}, {2448, 2048}, {1920, 1200}, {3840, 2160}, {65535, 48}, {64, 65535}};
  const int deals[] = {0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 32, 64, 4096, 1 << 20};
  for (const auto& s : sizes) {
    const int ntiles = ((s[0] + rip::kRemapTileW - 1) / rip::kRemapTileW) * ((s[1] + rip::kRemapTileH - 1) / rip::kRemapTileH);
    const int grids[] = {8, 16, 64, 1536, 2048, (ntiles + 7) / 8 * 8};  // the launchers' grids are multiples of 8
    for (int deal : deals)
      for (int order = 0; order <= 3; order++)  // 2: column strips where they deal out evenly; 3: an unknown order is row-major
        for (int blocks : grids) walk(s[0], s[1], deal, order, blocks);
  }
  printf("tile deal: %d cases, %d bad\n", g_cases, g_bad);
  return g_bad != 0;
}
