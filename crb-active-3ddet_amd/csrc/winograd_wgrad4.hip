// Weight gradient of the 3x3 stride-1 pad-1 convolution on channels_last (NHWC) f32 maps in the Winograd F(2x2, 3x3) domain with the
// 16 GEMMs on the bf16 matrix pipe through the exact three-way split of winograd_conv4.hip (winograd_split.h). Same algebra as
// winograd_wgrad.hip (the f32-MFMA kernel, which stays the instance for channel counts that are multiples of 64 but not of 128):
//     dU[xi][ci][co] = sum_tiles V[xi][tile][ci] * M[xi][tile][co],   V = B^T d B,   M = A dY A^T,   dW = G^T dU G
// V and M are formed in f32 with the additions of the f32 kernel, each is split into three bf16 pieces (and / subtract: no rounding
// instruction), and every product runs as the six v_mfma_f32_32x32x16_bf16 passes with piece indices i + j <= 4, accumulated in f32
// in the matrix pipe: what is dropped is below 2^-23 of the product. Inf / NaN / tiny values behave as in the forward kernel's
// split: an Inf operand becomes NaN (inf - inf), pieces below ~2^-110 are flushed.
//
// Why another block shape: v_mfma_f32_16x16x4_f32 runs at the f32 vector rate (1/16 of the bf16 rate), and the 64 x 64 x 16-xi block of
// the f32 kernel forms V once per output-channel block and M once per input-channel block and again in every wave. Here
//   * a workgroup (256 threads, one wave per SIMD, 256 accumulators per wave in AGPRs by name as in winograd4c_kernel) owns ONE xi ROW
//     (4 xi) x 128 input x 128 output channels over a contiguous range of tile chunks; wave = a 64 x 64 channel quadrant = 2 x 2 blocks
//     of 32 x 32 per xi. Row i of V needs two of the four patch rows, row i of M one or two gradient rows: nothing of the row pass is
//     computed twice across the four xi-row workgroups, and each element is transformed and split Cout/128 (V) / Cin/128 (M) times;
//   * chunk = 16 tiles = 4 tile rows x 4 tile columns of one image = the K of one MFMA. Thread (channel c, k group g) of the
//     transform owns the 8 tiles of tile rows 2 g, 2 g + 1 for ITS channel of V and of M: it reads its pixels straight from the maps
//     into registers (lanes = consecutive channels: 256-byte segments; the overlap of neighbouring patches stays in registers), and
//     ends with the 8 consecutive k that one MFMA lane wants: one ds_write_b128 per (xi, piece), conflict-free;
//   * LDS images [V | M][xi 4][piece 3][k group 2][channel 128][8 tiles] bf16 = 2 x 48 KB; an MFMA lane reads its fragment with one
//     conflict-free ds_read_b128: 12 fragment reads serve the 24 MFMAs of an xi (2 x 2 blocks x six passes);
//   * a chunk runs as two phases of two xi (48 MFMAs each, one barrier behind each); the two halves of the images are the two
//     buffers. Behind every MFMA stands one piece of the other work (one wave per SIMD: what is issued between two MFMAs runs under
//     the first one): one value of the OTHER image half (add, split, pack; 3 stores per 8 values), the row pass of the next chunk,
//     or the requests for the pixels of the chunk after next (inline asm, waited for by a hand-counted vmcnt). A first form that
//     ran [transform | barrier | 96 MFMAs | barrier] took 660 us where this one takes 506 (128 -> 128 @ 16 x 200 x 176). No
//     LDS-DMA, so the barriers need no counted copies.
// Every workgroup writes its partial dU rows in the f32 kernel's layout (64 x 64 blocks); the reduce kernel adds the ranges in range
// order in double and applies G^T . G (the arithmetic of winograd2_wgrad_reduce_kernel): two calls are bit-equal, whatever the stream or
// the CU reservation. No float atomics. Measurements and what was tried and dropped: DESIGN.md section 6.
#include <atomic>
#include <type_traits>
#include <utility>
#include "crb_common.h"
#include "winograd_split.h"
#include "winograd_blocks.h"     // the tile chunk as bev_blocks.hip sees it (chunk lists of a sparse map)
#include "../../include/crb_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int CB = 128;                       // channels per workgroup on either side
constexpr int PB = 64;                        // channel block of the partial layout (the f32 kernel's)
constexpr int NT = 256;
constexpr int IMG_KG = CB * 16;               // one k group: [channel 128][8 bf16] = 2048 bytes
constexpr int IMG_XP = 2 * IMG_KG;            // one (xi, piece) = 4096 bytes
constexpr int IMG_BYTES = 12 * IMG_XP;        // 4 xi x 3 pieces = 49152
constexpr int LDS_BYTES = 2 * IMG_BYTES;      // V and M
constexpr int CMAX = 1024;                    // largest channel count (bounds the zero page)

// source of everything outside the maps and of the gradient row an xi row does not use (zero-initialised, never written): a lane
// reads it at the offsets it uses inside a pixel row: channel + column * channels (column < 18 with the prefetch of the next chunk)
__device__ float g_wgrad4_zero_page[18 * CMAX + CB];

struct Wg4Args {
  const float* x;      // (N,H,W,Cin)
  const float* dy;     // (N,H,W,Cout)
  float* part;         // (ranges, Cin/64 * Cout/64 blocks, 16, 64 ci, 64 co)
  const float* zero;   // g_wgrad4_zero_page
  int N, H, W, cin, cout;
  int th, tw;          // tile rows / columns per image
  int tc4, rp;         // chunk columns / rows per image = ceil(tw / 4), ceil(th / 4)
  int nchunks;         // N * rp * tc4
  int nci, nco;        // channel blocks of 128
  int nranges;         // K ranges (multiple of 8)
  const int32_t* list;        // LIST instances: the ascending chunks to walk (crb_bev_blocks: chunks whose x patch holds an active pixel) ...
  const int32_t* list_count;  // ... and how many of them (device memory)
};

__device__ __forceinline__ int sload1(const int32_t* p) {
  int r;
  asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(p));
  return r;
}

struct ChunkPos { int n, p, bc; };
__device__ __forceinline__ void chunk_next(ChunkPos& c, const Wg4Args& a) {
  if (++c.bc < a.tc4) return;
  c.bc = 0;
  if (++c.p < a.rp) return;
  c.p = 0;
  ++c.n;
}

template <typename F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// accumulator block B (16 registers) = a[16 B : 16 B + 15] by name (see winograd_conv4.hip: as C++ values the register allocator parks
// accumulator tuples in VGPRs and copies them around every MFMA). MFMA -> MFMA on the same accumulator needs no wait states; MFMA ->
// v_accvgpr_read does: acc_settle() in front of the partial stores.
template <int B>
__device__ __forceinline__ void mfma_acc(const bf16x8& A, const bf16x8& Bv) {
  asm volatile("v_mfma_f32_32x32x16_bf16 a[%2:%3], %0, %1, a[%2:%3]" : : "v"(A), "v"(Bv), "n"(B * 16), "n"(B * 16 + 15));
}
template <int R>
__device__ __forceinline__ float acc_read() {
  float x;
  asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(x) : "n"(R));
  return x;
}
template <int R>
__device__ __forceinline__ void acc_zero() { asm volatile("v_accvgpr_write_b32 a[%0], 0" : : "n"(R)); }
__device__ __forceinline__ void acc_settle() { asm volatile("s_nop 15\n\ts_nop 15" ::: "memory"); }

// 4 bytes at (uniform base in SGPRs) + (lane byte offset), requested HERE and waited for by hand (s_waitcnt vmcnt(n) + reg_anchor
// before the first use): the compiler does not know this is a memory operation, so it neither spends two VALU instructions per load on
// a 64-bit lane address nor waits for the prefetches that are requested behind it
__device__ __forceinline__ float gload(const float* sbase, unsigned voff) {
  float r;
  asm volatile("global_load_dword %0, %1, %2" : "=v"(r) : "v"(voff), "s"(sbase));
  return r;
}
// (volatile asm statements keep their order: a value passed through here exists at this point of the instruction stream, and its
// uses come behind every volatile statement in front of it - the counter waits in particular)
__device__ __forceinline__ void reg_anchor(float& x) { asm volatile("" : "+v"(x)); }

// MODE (measurement builds, wrong results): 1 = no MFMAs, 2 = no transform (row pass, split and image stores; the loads are still
// requested and waited for), 3 = no map loads (the transform runs on register garbage)
// TOUCH: every wave also reads one dword of each 128-byte line of the chunk AFTER the one it requests (8 loads per chunk whose values
// nobody uses): the maps are first-touch HBM lines, and one chunk of lead (64 MFMAs) does not cover that latency under load; the
// pixels themselves then come from L2
// LIST: the ranges split a.list instead of all chunks and every chunk position is decoded from its list entry (a skipped chunk adds
// exact zeros, so only the summation order moves with the range boundaries); the prefetch touches assume the next chunk of a row
// is the neighbour: no LIST instance with TOUCH
template <int MODE, bool TOUCH, int LP2 = 3, bool LIST = false>
__global__ __launch_bounds__(NT, 1) void winograd4_wgrad_kernel(Wg4Args a) {
  static_assert(!(LIST && TOUCH), "the prefetch touches follow chunk_next");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* const Vimg = lds;
  unsigned char* const Mimg = lds + IMG_BYTES;
  const int T = threadIdx.x, lane = T & 63, wave = __builtin_amdgcn_readfirstlane(T >> 6);
  asm volatile("" ::: "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17",
               "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33", "a34", "a35",
               "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", "a48", "a49", "a50", "a51", "a52", "a53",
               "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71",
               "a72", "a73", "a74", "a75", "a76", "a77", "a78", "a79", "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89",
               "a90", "a91", "a92", "a93", "a94", "a95", "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106",
               "a107", "a108", "a109", "a110", "a111", "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121",
               "a122", "a123", "a124", "a125", "a126", "a127", "a128", "a129", "a130", "a131", "a132", "a133", "a134", "a135", "a136",
               "a137", "a138", "a139", "a140", "a141", "a142", "a143", "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151",
               "a152", "a153", "a154", "a155", "a156", "a157", "a158", "a159", "a160", "a161", "a162", "a163", "a164", "a165", "a166",
               "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175", "a176", "a177", "a178", "a179", "a180", "a181",
               "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191", "a192", "a193", "a194", "a195", "a196",
               "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207", "a208", "a209", "a210", "a211",
               "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222", "a223", "a224", "a225", "a226",
               "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237", "a238", "a239", "a240", "a241",
               "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252", "a253", "a254", "a255");

  // ---- xi row, channel blocks and range of this workgroup: the 4 * nci * nco workgroups of ONE range read the same maps: same XCD
  const int nb = 4 * a.nci * a.nco;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int sub = slot % nb, range = (slot / nb) * 8 + xcd;
  if (range >= a.nranges) return;
  const int xr = sub & 3, blk = sub >> 2;      // xi row i of the 4 x 4 Winograd domain
  const int cib = blk / a.nco, cob = blk - cib * a.nco;
  const int nwalk = LIST ? min(max(*a.list_count, 0), a.nchunks) : a.nchunks;
  const int c_first = (int)((int64_t)range * nwalk / a.nranges);
  const int c_end = (int)((int64_t)(range + 1) * nwalk / a.nranges);
  const int total = c_end - c_first;          // (0 with more ranges than chunks: a zero partial)

  static_for<256>([](auto r) { acc_zero<decltype(r)::value>(); });

  // ---- transform role: thread = (channel c of the block, k group g = tile rows 2 g, 2 g + 1 of the chunk)
  const int c = T & (CB - 1), g = wave >> 1;
  const float* const xblk = a.x + cib * CB;
  const float* const dyblk = a.dy + cob * CB;
  // row i of B^T d = d[ra] + sgn * d[rb], B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
  const int ra = xr == 0 ? 0 : xr == 2 ? 2 : 1, rb = xr == 0 ? 2 : xr == 1 ? 2 : xr == 2 ? 1 : 3;
  const float sgn = xr == 1 ? 1.f : -1.f;
  // row i of A dY = (g0, g0 + g1, g0 - g1, -g1)[i] = ga + sb * gb with the unused row read from the zero page
  const bool use_g0 = xr < 3, use_g1 = xr > 0;
  const float sb = xr == 1 ? 1.f : -1.f;
  const int img_wr = g * IMG_KG + c * 16;

  // byte offsets of the lane's channel in pixel column j of a row. Columns outside the map are CLAMPED into the row (every address
  // stays inside the row it belongs to) and their values are zeroed after the row pass; only chunks at the left / right border need it
  unsigned vx[10], vg[8];
  auto is_edge = [&](int bc) { return bc == 0 || 8 * bc + 8 >= a.W; };
  auto set_cols = [&](int bc) __attribute__((always_inline)) {
    const int x0 = 8 * bc - 1;
#pragma unroll
    for (int j = 0; j < 10; ++j) vx[j] = (unsigned)(c + (min(max(x0 + j, 0), a.W - 1) - x0) * a.cin) * 4u;
#pragma unroll
    for (int j = 0; j < 8; ++j) vg[j] = (unsigned)(c + (min(x0 + 1 + j, a.W - 1) - (x0 + 1)) * a.cout) * 4u;
  };
  // the wave's 8 pixel rows of a chunk (uniform): [tile row r][patch row a / b] of x from pixel column 8 bc - 1, [r][gradient row] of dy
  // from pixel column 8 bc; a row outside the map (or one this xi row does not use) is read from the zero page
  const float* px[2][2];
  const float* pg[2][2];
  bool okx[2][2], okg[2][2];
  ChunkPos cp;                                 // the chunk the pointers describe = the latest one requested
  bool cols_dirty = false;
  auto set_rows = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int ty = 4 * cp.p + 2 * g + r;
#pragma unroll
      for (int ab = 0; ab < 2; ++ab) {
        const int y = 2 * ty - 1 + (ab ? rb : ra);
        okx[r][ab] = cp.n < a.N && ty < a.th && (unsigned)y < (unsigned)a.H;
        px[r][ab] = xblk + (((int64_t)cp.n * a.H + y) * a.W + (8 * cp.bc - 1)) * a.cin;
        const int yg = 2 * ty + ab;
        okg[r][ab] = cp.n < a.N && (ab ? use_g1 : use_g0) && yg < a.H;
        pg[r][ab] = dyblk + (((int64_t)cp.n * a.H + yg) * a.W + 8 * cp.bc) * a.cout;
      }
    }
  };
  int walk = c_first;                          // LIST: the list entry cp came from
  auto at_entry = [&](int e) __attribute__((always_inline)) {     // cp = chunk of list entry e (clamped: requests past the end of the list
                                                                  // fetch its last chunk, nobody reads them)
    const int ch = min(max(sload1(a.list + min(e, nwalk - 1)), 0), a.nchunks - 1);
    const int rows = ch / a.tc4;
    cp.bc = ch - rows * a.tc4;
    cp.n = rows / a.rp;
    cp.p = rows - cp.n * a.rp;
  };
  auto advance = [&]() __attribute__((always_inline)) {       // cp -> the next chunk; the pointers follow
    if (LIST) {
      at_entry(++walk);
      set_rows();
    } else if (cp.bc + 1 < a.tc4) {
      ++cp.bc;
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int ab = 0; ab < 2; ++ab) { px[r][ab] += 8 * a.cin; pg[r][ab] += 8 * a.cout; }
    } else {
      chunk_next(cp, a);
      set_rows();
    }
    const bool e = is_edge(cp.bc);
    if (e || cols_dirty) set_cols(cp.bc);
    cols_dirty = e;
  };

  // ---- the lane's pixels of a chunk: request (72 loads), wait, row pass
  float xv[2][2][10], gv[2][2][8];             // [tile row][patch row a / b | gradient row][column]
  float t[2][10], m[2][8];                     // row pass: row i of B^T d and of A dY
  const float* sx[2][2];
  const float* sg[2][2];
  auto select_rows = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int ab = 0; ab < 2; ++ab) {
        sx[r][ab] = okx[r][ab] ? px[r][ab] : a.zero;
        sg[r][ab] = okg[r][ab] ? pg[r][ab] : a.zero;
      }
  };
  auto load_slot = [&](auto lc) __attribute__((always_inline)) {       // L = 0 .. 71
    constexpr int L = decltype(lc)::value, r = L / 36, k = L % 36;
    if constexpr (k < 20) {
      constexpr int ab = k / 10, j = k % 10;
      if (MODE == 3) asm volatile("" : "=v"(xv[r][ab][j]));
      else xv[r][ab][j] = gload(sx[r][ab], vx[j]);
    } else {
      constexpr int ab = (k - 20) / 8, j = (k - 20) % 8;
      if (MODE == 3) asm volatile("" : "=v"(gv[r][ab][j]));
      else gv[r][ab][j] = gload(sg[r][ab], vg[j]);
    }
  };
  // prefetch of the chunk behind the one just requested: lane -> (pixel column, 128-byte line of the wave's 256 channel bytes) of
  // each of the 8 rows. Only inside a row of chunks and where that chunk does not touch the right border (clamping again would need
  // per-lane columns); the values land in td[] and are never used, but the registers stay reserved until they have landed
  float td[8];
  const unsigned tvx = (unsigned)((c & 64) + (lane & 1) * 32 + (8 + min(lane >> 1, 9)) * a.cin) * 4u;
  const unsigned tvg = (unsigned)((c & 64) + (lane & 1) * 32 + (8 + min(lane >> 1, 7)) * a.cout) * 4u;
  auto touch = [&]() __attribute__((always_inline)) {
    if (!TOUCH) return;
    const bool on = cp.bc + 1 < a.tc4 && 8 * (cp.bc + 1) + 8 < a.W;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int ab = 0; ab < 2; ++ab) {
        td[r * 4 + ab] = gload(on ? sx[r][ab] : a.zero, tvx);
        td[r * 4 + 2 + ab] = gload(on ? sg[r][ab] : a.zero, tvg);
      }
  };
  auto touch_retire = [&]() __attribute__((always_inline)) {  // behind 60 loads of the next request (the counter has 6 bits): the previous
    if (!TOUCH) return;                                       // touches are older than those, so they have landed long ago
    asm volatile("s_waitcnt vmcnt(60)" ::: "memory");
    asm volatile("" :: "v"(td[0]), "v"(td[1]), "v"(td[2]), "v"(td[3]), "v"(td[4]), "v"(td[5]), "v"(td[6]), "v"(td[7]));
  };
  auto wait_loads = [&]() __attribute__((always_inline)) {    // the 72 loads of the latest request (its 8 touches may stay in flight)
    if (MODE != 3) {
      if (TOUCH) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int ab = 0; ab < 2; ++ab) {
#pragma unroll
        for (int j = 0; j < 10; ++j) reg_anchor(xv[r][ab][j]);
#pragma unroll
        for (int j = 0; j < 8; ++j) reg_anchor(gv[r][ab][j]);
      }
  };
  auto row_slot = [&](auto rc) __attribute__((always_inline)) {        // R = 0 .. 35 (sgn, sb = +-1: the exact sum / difference)
    constexpr int R = decltype(rc)::value;
    if (MODE == 2) return;
    if constexpr (R < 20) {
      constexpr int r = R / 10, j = R % 10;
      t[r][j] = __builtin_fmaf(sgn, xv[r][1][j], xv[r][0][j]);
      reg_anchor(t[r][j]);
    } else if constexpr (R < 36) {
      constexpr int r = (R - 20) / 8, j = (R - 20) % 8;
      m[r][j] = __builtin_fmaf(sb, gv[r][1][j], gv[r][0][j]);
      reg_anchor(m[r][j]);
    }
  };
  auto mask_cols = [&]() __attribute__((always_inline)) {     // t, m of the chunk at cp: columns outside the map are zero
    if (MODE == 2 || !is_edge(cp.bc)) return;
    const int x0 = 8 * cp.bc - 1;
#pragma unroll
    for (int j = 0; j < 10; ++j)
      if ((unsigned)(x0 + j) >= (unsigned)a.W) { t[0][j] = 0.f; t[1][j] = 0.f; }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (x0 + 1 + j >= a.W) { m[0][j] = 0.f; m[1][j] = 0.f; }
  };

  // ---- one value of the operand images per slot: slot s = 0 .. 31 of xi pair P: group s >> 3 = (xi 2 P, V), (xi 2 P, M), (xi 2 P + 1, V),
  //      (xi 2 P + 1, M); element e = s & 7 = tile (row e >> 2, column e & 3) of the lane's k group: value, split; behind every second
  //      one the three packs (v_perm_b32: high half of the even value | high half of the odd one << 16), behind the eighth the stores
  float sv[2], s1[2], s2[2];
  u32x4 q0, q1, q2;
  auto value_slot = [&](auto pc, auto sc) __attribute__((always_inline)) {
    constexpr int P = decltype(pc)::value, s = decltype(sc)::value;
    constexpr int gi = s >> 3, e = s & 7, jx = 2 * P + (gi >> 1), r = e >> 2, tc = e & 3, h = e & 1;
    constexpr bool is_m = (gi & 1) != 0;
    if (MODE == 2) return;
    float v;
    if constexpr (!is_m) {                     // (t B)[jx] = (t0 - t2, t1 + t2, t2 - t1, t1 - t3)
      const float* q = &t[r][2 * tc];
      v = jx == 0 ? q[0] - q[2] : jx == 1 ? q[1] + q[2] : jx == 2 ? q[2] - q[1] : q[1] - q[3];
    } else {                                   // (m A^T)[jx] = (a, a + b, a - b, -b)
      const float p = m[r][2 * tc], q = m[r][2 * tc + 1];
      v = jx == 0 ? p : jx == 1 ? p + q : jx == 2 ? p - q : -q;
    }
    sv[h] = v;
    split3f(v, s1[h], s2[h]);
    reg_anchor(sv[h]); reg_anchor(s1[h]); reg_anchor(s2[h]);
    if constexpr (h == 1) {
      constexpr int k = e >> 1;
      q0[k] = __builtin_amdgcn_perm(__float_as_uint(sv[1]), __float_as_uint(sv[0]), 0x07060302u);
      q1[k] = __builtin_amdgcn_perm(__float_as_uint(s1[1]), __float_as_uint(s1[0]), 0x07060302u);
      q2[k] = __builtin_amdgcn_perm(__float_as_uint(s2[1]), __float_as_uint(s2[0]), 0x07060302u);
      asm volatile("" : "+v"(q0[k]), "+v"(q1[k]), "+v"(q2[k]));
    }
    if constexpr (e == 7) {
      unsigned char* const dst = (is_m ? Mimg : Vimg) + jx * 3 * IMG_XP + img_wr;
      *reinterpret_cast<u32x4*>(dst) = q0;
      *reinterpret_cast<u32x4*>(dst + IMG_XP) = q1;
      *reinterpret_cast<u32x4*>(dst + 2 * IMG_XP) = q2;
    }
  };

  // ---- MFMA role: wave = input-channel half wi (B operand: columns) x output-channel half wo (A operand: rows); accumulator block of
  //      (xi jx, output block bo, input block bi) = 4 jx + 2 bo + bi
  const int wi = wave & 1, wo = wave >> 1;
  const int l31 = lane & 31, lhi = lane >> 5;
  const unsigned char* const a_rd = Mimg + lhi * IMG_KG + (wo * 64 + l31) * 16;
  const unsigned char* const b_rd = Vimg + lhi * IMG_KG + (wi * 64 + l31) * 16;
  auto frag = [&](int jx, bf16x8 (&A)[2][3], bf16x8 (&B)[2][3]) __attribute__((always_inline)) {
    constexpr int order[3] = {0, 2, 1};        // (the first passes take pieces (0, 2) and (2, 0))
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int p = order[o];
        A[h][p] = *reinterpret_cast<const bf16x8*>(a_rd + (jx * 3 + p) * IMG_XP + h * 32 * 16);
        B[h][p] = *reinterpret_cast<const bf16x8*>(b_rd + (jx * 3 + p) * IMG_XP + h * 32 * 16);
      }
  };

  // ---- phases. A chunk runs as phase 0 (MFMAs of xi 0, 1 of the row) and phase 1 (xi 2, 3), one barrier behind each; the two halves
  //      of the images are the two buffers. One piece of the other work stands behind every MFMA (one wave per SIMD: what is issued
  //      between two MFMAs runs under the first one):
  //        phase 0 of chunk q: values of xi 2, 3 of chunk q (gaps 0 .. 31); wait for the pixels of chunk q + 1 and their row pass
  //                            (gaps 40 .. 47; t, m of chunk q are done with)
  //        phase 1 of chunk q: request the pixels of chunk q + 2 (three loads per two gaps, all 48 gaps); values of xi 0, 1 of chunk
  //                            q + 1 (gaps 16 .. 47)
  //      so the last load of a request has 40 gaps before its wait, the first one 88. Past the end of the range the requests read another range's chunk or the zero
  //      page and the values go to an image half nobody reads: every phase runs the same instructions.
  auto phase = [&](auto pc) __attribute__((always_inline)) {
    constexpr int P = decltype(pc)::value;
    bf16x8 A0[2][3], B0[2][3], A1[2][3], B1[2][3];
    frag(2 * P, A0, B0);
    if (P == 1) {
      advance();
      select_rows();
    }
    __builtin_amdgcn_sched_barrier(0);
    static_for<48>([&](auto kc) __attribute__((always_inline)) {
      constexpr int k = decltype(kc)::value, u = k / 24, w = k % 24, pass = w / 4, bo = (w >> 1) & 1, bi = w & 1;
      constexpr int pa = pass == 0 ? 0 : pass == 1 ? 2 : pass == 2 ? 1 : pass == 3 ? 0 : pass == 4 ? 1 : 0;
      constexpr int pb = pass == 0 ? 2 : pass == 1 ? 0 : pass == 2 ? 1 : pass == 3 ? 1 : 0;
      if (MODE != 1) {
        if constexpr (u == 0) mfma_acc<4 * (2 * P) + 2 * bo + bi>(A0[bo][pa], B0[bi][pb]);
        else mfma_acc<4 * (2 * P + 1) + 2 * bo + bi>(A1[bo][pa], B1[bi][pb]);
      } else if constexpr (w == 23) {
        if constexpr (u == 0) asm volatile("" :: "v"(A0[0][0]), "v"(A0[1][1]), "v"(A0[1][2]), "v"(B0[0][0]), "v"(B0[1][1]), "v"(B0[1][2]));
        else asm volatile("" :: "v"(A1[0][0]), "v"(A1[1][1]), "v"(A1[1][2]), "v"(B1[0][0]), "v"(B1[1][1]), "v"(B1[1][2]));
      }
      if constexpr (k == 2) frag(2 * P + 1, A1, B1);
      if constexpr (P == 0) {
        if constexpr (k < 32) value_slot(std::integral_constant<int, 1>{}, kc);
        if constexpr (k == 40) wait_loads();
        if constexpr (k >= 40) {
          static_for<5>([&](auto ic) __attribute__((always_inline)) {
            row_slot(std::integral_constant<int, 5 * (k - 40) + decltype(ic)::value>{});
          });
        }
      } else {
        // LP2 pixel loads per TWO gaps (measured at 128 -> 128 with one round of workgroups: 5 loads per gap 561 us, 3 per gap 532, 2 per
        // gap 506; with two rounds 2 per gap 578, 1.5 per gap 564: a burst of loads holds the wave at the issue of the next one)
        constexpr int L0 = k * LP2 / 2, L1 = (k + 1) * LP2 / 2;
        if constexpr (L0 < 72) {
          if constexpr (L0 <= 60 && L1 > 60) touch_retire();
          static_for<L1 - L0>([&](auto ic) __attribute__((always_inline)) {
            constexpr int L = L0 + decltype(ic)::value;
            if constexpr (L < 72) load_slot(std::integral_constant<int, L>{});
          });
        }
        if constexpr (L0 < 72 && (L1 >= 72 || k == 47)) touch();
        if constexpr (k >= 16) value_slot(std::integral_constant<int, 0>{}, std::integral_constant<int, k - 16>{});
      }
      __builtin_amdgcn_sched_barrier(0);
    });
    if (P == 0) mask_cols();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };

  if (total > 0) {
    // ---- prologue: chunk 0 -> t, m -> xi 0, 1 of the images; chunk 1 requested
    if (LIST) at_entry(c_first);
    else {
      const int rows = c_first / a.tc4;
      cp.bc = c_first - rows * a.tc4;
      cp.n = rows / a.rp;
      cp.p = rows - cp.n * a.rp;
    }
    set_rows();
    set_cols(cp.bc);
    cols_dirty = is_edge(cp.bc);
    select_rows();
    static_for<72>([&](auto lc) __attribute__((always_inline)) { load_slot(lc); });
    if (MODE != 3) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (TOUCH) {
#pragma unroll
      for (int k = 0; k < 8; ++k) asm volatile("v_mov_b32 %0, 0" : "=v"(td[k]));
    }
    {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int ab = 0; ab < 2; ++ab) {
#pragma unroll
          for (int j = 0; j < 10; ++j) reg_anchor(xv[r][ab][j]);
#pragma unroll
          for (int j = 0; j < 8; ++j) reg_anchor(gv[r][ab][j]);
        }
    }
    static_for<36>([&](auto rc) __attribute__((always_inline)) { row_slot(rc); });
    mask_cols();
    static_for<32>([&](auto sc) __attribute__((always_inline)) { value_slot(std::integral_constant<int, 0>{}, sc); });
    advance();
    select_rows();
    static_for<72>([&](auto lc) __attribute__((always_inline)) { load_slot(lc); });
    touch();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    for (int q = 0; q < total; ++q) {
      phase(std::integral_constant<int, 0>{});
      phase(std::integral_constant<int, 1>{});
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (requests past the end of the range: nothing may land in a reused register)
    if (TOUCH) asm volatile("" :: "v"(td[0]), "v"(td[1]), "v"(td[2]), "v"(td[3]), "v"(td[4]), "v"(td[5]), "v"(td[6]), "v"(td[7]));
  }

  // ---- partial dU in the f32 kernel's layout: block (ci / 64, co / 64), [xi][ci % 64][co % 64]. Accumulator register 4 j + e of a
  //      block: row (output channel) 8 j + 4 lhi + e, column (input channel) l31: 16-byte stores
  acc_settle();
  const int pblk = (cib * 2 + wi) * (a.nco * 2) + cob * 2 + wo;
  float* const out = a.part + ((int64_t)range * (a.nci * a.nco * 4) + pblk) * (16 * PB * PB) + (xr * 4) * (PB * PB) + l31 * PB + 4 * lhi;
  static_for<64>([&](auto qc) {
    constexpr int Q = decltype(qc)::value;     // (block, register group j)
    constexpr int B = Q >> 2, j = Q & 3, jx = B >> 2, bo = (B >> 1) & 1, bi = B & 1;
    const f32x4 v = (f32x4){acc_read<B * 16 + 4 * j>(), acc_read<B * 16 + 4 * j + 1>(), acc_read<B * 16 + 4 * j + 2>(),
                            acc_read<B * 16 + 4 * j + 3>()};
    *reinterpret_cast<f32x4*>(out + jx * (PB * PB) + bi * 32 * PB + bo * 32 + 8 * j) = v;
  });
}

// dW[co][ci][ky][kx] = (G^T dU[.][ci][co] G)[ky][kx], dU = sum over the ranges in range order (double), written with the element
// strides of the weight tensor: the arithmetic of winograd2_wgrad_reduce_kernel on the same partial layout, with the 16 xi of a
// (ci, co) pair summed by four threads (one xi row each; the sums meet in LDS): one thread per pair is 64 workgroups at 128 -> 128,
// too few to stream the 128 MB of partials. Workgroup = one input channel x 64 output channels. G^T = [1 .5 .5 0; 0 .5 -.5 0; 0 .5 .5 1]
__global__ __launch_bounds__(256) void winograd4_wgrad_reduce_kernel(const float* __restrict__ part, int nranges, int nci, int nco,
                                                                     float* __restrict__ dw, int64_t so, int64_t si, int64_t sky,
                                                                     int64_t skx, int cin, int cout) {
  __shared__ double sh[16][PB];
  const int col = threadIdx.x & (PB - 1), xrow = threadIdx.x >> 6;
  const int ci = blockIdx.x / nco, cob = blockIdx.x - ci * nco;     // nco = Cout / 64 blocks of the partial layout
  const int co = cob * PB + col;
  const int blk = (ci / PB) * nco + cob;
  const int64_t nblk = (int64_t)nci * nco;
  const float* p = part + blk * (int64_t)(16 * PB * PB) + (xrow * 4) * (PB * PB) + (ci % PB) * PB + col;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int r = 0; r < nranges; ++r) {
    const float* q = p + r * nblk * (16 * PB * PB);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] += (double)q[j * PB * PB];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) sh[xrow * 4 + j][col] = s[j];
  __syncthreads();
  if (xrow != 0) return;
  double u[16];
#pragma unroll
  for (int xi = 0; xi < 16; ++xi) u[xi] = sh[xi][col];
  double h[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    h[0][j] = u[0 * 4 + j] + 0.5 * (u[1 * 4 + j] + u[2 * 4 + j]);
    h[1][j] = 0.5 * (u[1 * 4 + j] - u[2 * 4 + j]);
    h[2][j] = 0.5 * (u[1 * 4 + j] + u[2 * 4 + j]) + u[3 * 4 + j];
  }
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    float* o = dw + co * so + ci * si + ky * sky;
    o[0 * skx] = (float)(h[ky][0] + 0.5 * (h[ky][1] + h[ky][2]));
    o[1 * skx] = (float)(0.5 * (h[ky][1] - h[ky][2]));
    o[2 * skx] = (float)(0.5 * (h[ky][1] + h[ky][2]) + h[ky][3]);
  }
}

// ranges so that the workgroup count (4 xi rows x channel blocks x ranges) fills the CUs TWICE; a multiple of 8 (XCD placement).
// Twice, for the accumulation error: a workgroup adds six MFMA results per chunk into its f32 accumulators (the f32 kernel: four per 16
// tiles), and with one round of workgroups (137 chunks each at 16 x 128 -> 128 @ 200 x 176) the error against f64 was 1.4 - 1.6 x the
// f32 kernel's; chains of half the length bring it to the f32 kernel's level. Price: twice the partial blocks for the reduce kernel.
__host__ int wgrad4_ranges(int nb) {
  static std::atomic<int> n_cu{0};
  int n = n_cu.load(std::memory_order_relaxed);
  if (!n) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 8;
    n = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    n_cu.store(n, std::memory_order_relaxed);
  }
  const int r = (2 * n / nb) & ~7;
  return r < 8 ? 8 : r;
}

}  // namespace

CRB_KNOB g_wgrad4_mode = 0;     // measurement builds: 1 = no MFMAs, 2 = no transforms, 3 = no map loads; A/B with correct results: 4 = with prefetch
                                // touches of the chunk after next (at 2 loads per gap), 5 / 6 = 2 / 5 pixel loads per MFMA gap instead of 1.5
#ifdef CRB_MEASURE
extern "C" int crb_winograd4_wgrad_set_mode(int mode) { g_wgrad4_mode = (mode >= 1 && mode <= 6) ? mode : 0; return CRB_OK; }
#endif

extern "C" int crb_winograd4_wgrad_supported(int cin, int cout, int H, int W) {
  return (cin > 0 && cout > 0 && cin % CB == 0 && cout % CB == 0 && cin <= CMAX && cout <= CMAX && H >= 1 && W >= 1) ? 1 : 0;
}

extern "C" int64_t crb_winograd4_wgrad_workspace_bytes(int cin, int cout) {
  if (!crb_winograd4_wgrad_supported(cin, cout, 1, 1)) return 0;
  const int nblk = (cin / CB) * (cout / CB);
  return (int64_t)wgrad4_ranges(4 * nblk) * nblk * 4 * 16 * PB * PB * 4;
}

// x (N,H,W,Cin), dy (N,H,W,Cout) f32 NHWC -> dw = gradient of the nn.Conv2d weight (Cout,Cin,3,3), written with the element
// strides (so, si, sky, skx) of that tensor. workspace: crb_winograd4_wgrad_workspace_bytes(cin, cout).
static int wgrad4_launch(const float* x, const float* dy, float* dw, int64_t so, int64_t si, int64_t sky, int64_t skx, int N, int H, int W,
                         int cin, int cout, void* workspace, int64_t workspace_bytes, void* stream, const int32_t* list,
                         const int32_t* list_count) {
  if (N <= 0 || H <= 0 || W <= 0) return CRB_ERR_ARG;
  if (!crb_winograd4_wgrad_supported(cin, cout, H, W)) return CRB_ERR_UNSUPPORTED;
  if (workspace_bytes < crb_winograd4_wgrad_workspace_bytes(cin, cout) || !workspace) return CRB_ERR_WORKSPACE;
  if (((int64_t)N * H + 8) * (W + 16) * (cin > cout ? cin : cout) >= (1LL << 31)) return CRB_ERR_ARG;
  static std::atomic<const float*> zero_pages[64];
  static std::atomic<unsigned> attr_done[64];
  int dev = 0;
  CRB_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return CRB_ERR_ARG;
  const float* zero_page = zero_pages[dev].load(std::memory_order_acquire);
  if (!zero_page) {
    CRB_HIP(hipGetSymbolAddress((void**)&zero_page, HIP_SYMBOL(g_wgrad4_zero_page)));
    zero_pages[dev].store(zero_page, std::memory_order_release);
  }
  Wg4Args a;
  a.x = x; a.dy = dy; a.part = (float*)workspace; a.zero = zero_page;
  a.list = list; a.list_count = list_count;
  a.N = N; a.H = H; a.W = W; a.cin = cin; a.cout = cout;
  a.th = (H + 1) / 2; a.tw = (W + 1) / 2;
  a.tc4 = (a.tw + wino_blocks::WG4_CH_COLS - 1) / wino_blocks::WG4_CH_COLS;
  a.rp = (a.th + wino_blocks::WG4_CH_ROWS - 1) / wino_blocks::WG4_CH_ROWS;
  const int64_t nch = (int64_t)N * a.rp * a.tc4;
  if (nch >= (1LL << 30)) return CRB_ERR_ARG;
  a.nchunks = (int)nch;
  a.nci = cin / CB; a.nco = cout / CB;
  const int nb = 4 * a.nci * a.nco;
  a.nranges = wgrad4_ranges(nb);
  auto kern = winograd4_wgrad_kernel<0, false>;
#ifdef CRB_MEASURE
  if (g_wgrad4_mode == 1) kern = winograd4_wgrad_kernel<1, false>;
  if (g_wgrad4_mode == 2) kern = winograd4_wgrad_kernel<2, false>;
  if (g_wgrad4_mode == 3) kern = winograd4_wgrad_kernel<3, false>;
  if (g_wgrad4_mode == 4) kern = winograd4_wgrad_kernel<0, true, 4>;
  if (g_wgrad4_mode == 5) kern = winograd4_wgrad_kernel<0, false, 4>;
  if (g_wgrad4_mode == 6) kern = winograd4_wgrad_kernel<0, false, 10>;
#endif
  if (list) kern = winograd4_wgrad_kernel<0, false, 3, true>;
  const unsigned bit = list ? (1u << 8) : 1u << (g_wgrad4_mode & 7);
  if (!(attr_done[dev].load(std::memory_order_acquire) & bit)) {
    CRB_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    attr_done[dev].fetch_or(bit, std::memory_order_release);
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)(a.nranges * nb)), dim3(NT), LDS_BYTES, (hipStream_t)stream, a);
  CRB_CHECK_LAUNCH();
  hipLaunchKernelGGL(winograd4_wgrad_reduce_kernel, dim3((unsigned)(cin * (cout / PB))), dim3(256), 0, (hipStream_t)stream,
                     (const float*)workspace, a.nranges, a.nci * 2, a.nco * 2, dw, so, si, sky, skx, cin, cout);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_winograd4_wgrad(const float* x, const float* dy, float* dw, int64_t so, int64_t si, int64_t sky, int64_t skx,
                                   int N, int H, int W, int cin, int cout, void* workspace, int64_t workspace_bytes, void* stream) {
  return wgrad4_launch(x, dy, dw, so, si, sky, skx, N, H, W, cin, cout, workspace, workspace_bytes, stream, nullptr, nullptr);
}

// the same gradient over the listed chunks only: x is zero in the patch of every other chunk (crb_bev_blocks: the wgrad list)
extern "C" int crb_winograd4_wgrad_blocks(const float* x, const float* dy, float* dw, int64_t so, int64_t si, int64_t sky, int64_t skx,
                                          int N, int H, int W, int cin, int cout, const int32_t* list, const int32_t* count,
                                          void* workspace, int64_t workspace_bytes, void* stream) {
  if (!list || !count) return CRB_ERR_ARG;
  return wgrad4_launch(x, dy, dw, so, si, sky, skx, N, H, W, cin, cout, workspace, workspace_bytes, stream, list, count);
}
