// Work units of the split-bf16 Winograd kernels as seen from outside them: the spatial block of winograd4c_kernel (winograd_conv4.hip),
// the tile chunk of winograd4_wgrad_kernel (winograd_wgrad4.hip), and the block lists bev_blocks.hip builds for both. One place for the
// numbers: the kernels, their launch code and the list builder all read them here.
#pragma once
#include <cstdint>

namespace wino_blocks {

constexpr int TILE = 2;                          // F(2x2, 3x3): a tile is 2 x 2 output pixels
// winograd4c_kernel: spatial block = 8 tile rows (running over the whole batch: tile row R = n * ceil(H / 2) + ty) x 4 tile columns
constexpr int C4_TB_ROWS = 8, C4_TB_COLS = 4;
// winograd4_wgrad_kernel: chunk = 4 tile rows x 4 tile columns of ONE image (16 tiles = the K of one MFMA)
constexpr int WG4_CH_ROWS = 4, WG4_CH_COLS = 4;

struct Geometry {
  int th, tw;            // tile rows per image, tiles per row
  int RT;                // tile rows over the batch
  int tw4, nblocks;      // conv: block columns, blocks = ceil(RT / C4_TB_ROWS) * tw4
  int rp, tc4, nchunks;  // wgrad: chunk rows per image, chunk columns, chunks = N * rp * tc4
};

__host__ __device__ inline Geometry geometry(int N, int H, int W) {
  Geometry g;
  g.th = (H + TILE - 1) / TILE;
  g.tw = (W + TILE - 1) / TILE;
  g.RT = N * g.th;
  g.tw4 = (g.tw + C4_TB_COLS - 1) / C4_TB_COLS;
  g.nblocks = ((g.RT + C4_TB_ROWS - 1) / C4_TB_ROWS) * g.tw4;
  g.rp = (g.th + WG4_CH_ROWS - 1) / WG4_CH_ROWS;
  g.tc4 = (g.tw + WG4_CH_COLS - 1) / WG4_CH_COLS;
  g.nchunks = N * g.rp * g.tc4;
  return g;
}

// the conv block / wgrad chunk that holds pixel (n, y, x) of the map
__host__ __device__ inline int conv_block_of(const Geometry& g, int n, int y, int x) {
  return ((n * g.th + y / TILE) / C4_TB_ROWS) * g.tw4 + (x / TILE) / C4_TB_COLS;
}
__host__ __device__ inline int wgrad_chunk_of(const Geometry& g, int n, int y, int x) {
  return (n * g.rp + (y / TILE) / WG4_CH_ROWS) * g.tc4 + (x / TILE) / WG4_CH_COLS;
}

// layout of the int32 buffer crb_bev_blocks writes (include/crb_hip.h): eight counts, then the five lists
enum { CNT_CONV_IN = 0, CNT_CONV_OUT = 1, CNT_WGRAD = 2, CNT_CONV_IN_REST = 3, CNT_CONV_OUT_REST = 4, N_COUNTS = 8 };

}  // namespace wino_blocks
