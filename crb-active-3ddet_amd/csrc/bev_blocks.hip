// Block lists of a sparse BEV map for the split-bf16 Winograd kernels (winograd_blocks.h): which spatial blocks of winograd4c_kernel and
// which tile chunks of winograd4_wgrad_kernel can see an active pixel. The first 3x3 layer of the BEV backbone reads the scattered
// output of the sparse backbone (88 % of its pixels are exactly zero): a block whose input patch holds no active pixel produces +0
// everywhere, a chunk whose x patch holds none adds nothing to the weight gradient, and the input gradient is only read at the active
// pixels. The kernels walk these lists instead of every block.
//
// Three passes, no atomics: flags cleared | one thread per index marks at most four blocks per list with plain byte stores of 1
// (idempotent: the order of the stores does not matter) | one workgroup per list compacts its flags by an ordered scan. The lists are
// ascending, so a launch that walks them is as reproducible as the dense launch. Counts stay in device memory.
#include "crb_common.h"
#include "winograd_blocks.h"
#include "../../include/crb_hip.h"

namespace {

namespace wb = wino_blocks;
constexpr int SCAN_NT = 1024;

__global__ __launch_bounds__(256) void bev_blocks_mark_kernel(const int32_t* __restrict__ idx, int64_t n, int N, int H, int W,
                                                              wb::Geometry g, unsigned char* __restrict__ f_in,
                                                              unsigned char* __restrict__ f_out, unsigned char* __restrict__ f_wg) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b = idx[4 * i], y = idx[4 * i + 2], x = idx[4 * i + 3];
  if ((unsigned)b >= (unsigned)N || (unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return;
  f_out[wb::conv_block_of(g, b, y, x)] = 1;
  // the 3 x 3 neighbourhood inside the map spans at most two block rows and two block columns: its corners name them all
  const int y0 = max(y - 1, 0), y1 = min(y + 1, H - 1), x0 = max(x - 1, 0), x1 = min(x + 1, W - 1);
  f_in[wb::conv_block_of(g, b, y0, x0)] = 1;
  f_in[wb::conv_block_of(g, b, y0, x1)] = 1;
  f_in[wb::conv_block_of(g, b, y1, x0)] = 1;
  f_in[wb::conv_block_of(g, b, y1, x1)] = 1;
  f_wg[wb::wgrad_chunk_of(g, b, y0, x0)] = 1;
  f_wg[wb::wgrad_chunk_of(g, b, y0, x1)] = 1;
  f_wg[wb::wgrad_chunk_of(g, b, y1, x0)] = 1;
  f_wg[wb::wgrad_chunk_of(g, b, y1, x1)] = 1;
}

struct CompactJob { const unsigned char* flags; int n; int32_t* list; int32_t* rest; int32_t* count; int32_t* rest_count; };
struct CompactJobs { CompactJob job[3]; };

// workgroup = one list: thread t owns items [t * per, (t + 1) * per), the workgroup scans the 1024 thread counts in LDS
__global__ __launch_bounds__(SCAN_NT) void bev_blocks_compact_kernel(CompactJobs jobs) {
  __shared__ int sh[SCAN_NT];
  const CompactJob q = jobs.job[blockIdx.x];
  const int t = threadIdx.x;
  const int per = (q.n + SCAN_NT - 1) / SCAN_NT;
  const int lo = min(t * per, q.n), hi = min(lo + per, q.n);
  int mine = 0;
  for (int i = lo; i < hi; ++i) mine += q.flags[i] ? 1 : 0;
  sh[t] = mine;
  __syncthreads();
  for (int d = 1; d < SCAN_NT; d <<= 1) {
    const int v = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += v;
    __syncthreads();
  }
  int pos = sh[t] - mine;                        // listed items in front of this thread's first one
  for (int i = lo; i < hi; ++i) {
    if (q.flags[i]) q.list[pos++] = i;
    else if (q.rest) q.rest[i - pos] = i;
  }
  if (t == SCAN_NT - 1) {
    *q.count = sh[t];
    if (q.rest_count) *q.rest_count = q.n - sh[t];
  }
}

}  // namespace

extern "C" int crb_bev_blocks_geometry(int N, int H, int W, int32_t* geom) {
  if (N <= 0 || H <= 0 || W <= 0 || !geom) return CRB_ERR_ARG;
  if ((int64_t)N * ((H + 1) / 2) >= (1LL << 30)) return CRB_ERR_ARG;
  const wb::Geometry g = wb::geometry(N, H, W);
  const int32_t v[12] = {g.nblocks, g.nchunks, g.th, g.tw, g.tw4, g.rp, g.tc4, wb::TILE, wb::C4_TB_ROWS, wb::C4_TB_COLS, wb::WG4_CH_ROWS,
                         wb::WG4_CH_COLS};
  for (int i = 0; i < 12; ++i) geom[i] = v[i];
  return CRB_OK;
}

extern "C" int64_t crb_bev_blocks_ints(int N, int H, int W) {
  int32_t geom[12];
  if (crb_bev_blocks_geometry(N, H, W, geom) != CRB_OK) return 0;
  const int64_t nb = geom[0], nc = geom[1];
  return wb::N_COUNTS + 4 * nb + nc + (2 * nb + nc + 3) / 4;       // counts, five lists, the three flag arrays (bytes)
}

extern "C" int crb_bev_blocks(const int32_t* indices, int64_t n, int N, int H, int W, int32_t* out, int64_t out_ints, void* stream) {
  if (n < 0 || (n > 0 && !indices) || !out) return CRB_ERR_ARG;
  const int64_t need = crb_bev_blocks_ints(N, H, W);
  if (need == 0) return CRB_ERR_ARG;
  if (out_ints < need) return CRB_ERR_WORKSPACE;
  const wb::Geometry g = wb::geometry(N, H, W);
  const int64_t nb = g.nblocks, nc = g.nchunks;
  if (nb >= (1LL << 26) || nc >= (1LL << 30) || n >= (1LL << 38)) return CRB_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  int32_t* const counts = out;
  int32_t* const l_in = out + wb::N_COUNTS;
  int32_t* const r_in = l_in + nb;
  int32_t* const l_out = r_in + nb;
  int32_t* const r_out = l_out + nb;
  int32_t* const l_wg = r_out + nb;
  unsigned char* const flags = (unsigned char*)(l_wg + nc);
  CRB_HIP(hipMemsetAsync(counts, 0, wb::N_COUNTS * sizeof(int32_t), st));
  CRB_HIP(hipMemsetAsync(flags, 0, (size_t)(2 * nb + nc), st));
  if (n > 0) {
    hipLaunchKernelGGL(bev_blocks_mark_kernel, dim3((unsigned)crb_cdiv(n, 256)), dim3(256), 0, st, indices, n, N, H, W, g, flags,
                       flags + nb, flags + 2 * nb);
    CRB_CHECK_LAUNCH();
  }
  CompactJobs jobs;
  jobs.job[0] = CompactJob{flags, (int)nb, l_in, r_in, counts + wb::CNT_CONV_IN, counts + wb::CNT_CONV_IN_REST};
  jobs.job[1] = CompactJob{flags + nb, (int)nb, l_out, r_out, counts + wb::CNT_CONV_OUT, counts + wb::CNT_CONV_OUT_REST};
  jobs.job[2] = CompactJob{flags + 2 * nb, (int)nc, l_wg, nullptr, counts + wb::CNT_WGRAD, nullptr};
  hipLaunchKernelGGL(bev_blocks_compact_kernel, dim3(3), dim3(SCAN_NT), 0, st, jobs);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
