// Transposed convolutions with kernel = stride (1 or 2) on channels_last (NHWC) f32 maps as plain row GEMMs on the bf16 matrix pipe,
// through the exact three-way split of winograd_conv4.hip (winograd_split.h): a channels_last map IS the row matrix (pixels x channels),
//     forward         Y[out_row(m, t)][co] = sum_ci        X[m][ci]              * w[ci][co][t]       (T = s * s taps, scattered rows)
//     input gradient  dX[m][ci]            = sum_(t, co)   dY[out_row(m, t)][co] * w[ci][co][t]       (gathered rows)
//     weight gradient dW[ci][co][t]        = sum_m         X[m][ci]              * dY[out_row(m, t)][co]
// with out_row(m, t = (a, b)) the NHWC pixel (n, s h + a, s w + b) of input pixel m = (n, h, w). For s = 1 all three are the identity map.
// Operands are f32, each written as the exact sum of three bf16 pieces (and / subtract: no rounding instruction); every product runs
// as the six v_mfma_f32_32x32x16_bf16 passes with piece indices i + j <= 4, accumulated in f32 in the matrix pipe: what is dropped is
// below 2^-23 of the product. An Inf operand becomes NaN (inf - inf), pieces below ~2^-110 of a tiny value are flushed: the behaviour of
// the Winograd split kernels.
//
// rows_gemm4_kernel (forward and input gradient: one kernel, the two directions differ in which side is gathered / scattered):
//   * computed transposed, D[channel][row] = W^T . X^T, so a lane ends with 4 consecutive output channels of ITS row: 16-byte stores;
//   * the activations need no LDS: lane (r, h) of the MFMA wants X[row r][8 consecutive k], which is contiguous in the row. A lane
//     loads 64 contiguous bytes of its row per 32 k (lanes r and r + 32 together a 128-byte line) and uses them for two MFMA k steps:
//     k step 2 c + u of the weight image holds k = 32 c + 16 h + 8 u + j for lane half h, element j;
//   * the weight is split once per step and weight version (crb_rows_gemm4_weights) into an image in the order the lanes read it,
//     [n / 32][k step][piece][lane][8 bf16]: a fragment is one 16-byte load per lane, 1 KB contiguous per wave, straight from L2 (the
//     waves of a workgroup that share columns hit in L1);
//   * persistent workgroups, one wave per SIMD; wave tile 64 rows x 128 columns = 2 x 128 accumulators (leading pass | the five small ones) in AGPRs by name (as C++ values the
//     register allocator copies accumulator tuples around every MFMA, see winograd_conv4.hip); workgroup = 2 x 2 waves (128 rows x 256
//     columns) or 4 x 1 where the column count is not a multiple of 256. Column tiles of one row tile are consecutive tiles (measured:
//     the rows are still fetched once per column tile at the k2s2 forward);
//   * the gathered direction (input gradient, K = taps x channels) moves the large sum to LDS after every tap and restarts the accumulators:
//     the matrix pipe truncates what it adds to a large accumulator, and four chains of a quarter of the length with four f32 additions
//     keep the error against f64 at the vendor kernel's level on small maps too;
//   * one loop over (tile, 32 k): the loads of the next step of the loop - whichever tile it belongs to - are requested before the 96
//     MFMAs of this one, and the split of the next operands stands in the gaps between them. No atomics, fixed order: bit-reproducible.
// rows_gemm4_wgrad_kernel: the contraction index is the row, so both operands reach the MFMA transposed, through LDS (the model is
//   winograd_wgrad4.hip): thread = channel reads 8 consecutive rows of its channel (lanes = consecutive channels: coalesced), splits,
//   and writes the 8 consecutive k of one MFMA lane with one ds_write_b128 per piece. Workgroup = tap x 256 input x 256 output channels
//   over a contiguous range of 16-row chunks, wave = 128 x 128 quadrant = 256 accumulators; double-buffered images, one barrier per chunk.
//   Partials per range, added in range order in double by rows_gemm4_wgrad_reduce_kernel and written with the parameter's strides.
#include <atomic>
#include <type_traits>
#include <utility>
#include "crb_common.h"
#include "winograd_split.h"
#include "../../include/crb_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int NT = 256;

template <typename F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// accumulator block B (16 registers) = a[16 B : 16 B + 15] by name. MFMA -> MFMA on the same accumulator needs no wait states; MFMA ->
// v_accvgpr_read does: acc_settle() in front of the stores.
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

#define RG_ACC_0_127                                                                                                                   \
  "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17", "a18", "a19",   \
      "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33", "a34", "a35", "a36", "a37",   \
      "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55",   \
      "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73",   \
      "a74", "a75", "a76", "a77", "a78", "a79", "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", "a91",   \
      "a92", "a93", "a94", "a95", "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106", "a107", "a108", \
      "a109", "a110", "a111", "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124", \
      "a125", "a126", "a127"
#define RG_ACC_128_255                                                                                                                 \
  "a128", "a129", "a130", "a131", "a132", "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140", "a141", "a142", "a143",     \
      "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156", "a157", "a158", "a159", \
      "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175", \
      "a176", "a177", "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191", \
      "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207", \
      "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222", "a223", \
      "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237", "a238", "a239", \
      "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252", "a253", "a254", "a255"

// the six passes in the order of the Winograd kernels (smallest products first): piece of the first / second operand
__device__ constexpr int pass_a(int p) { return p == 0 ? 0 : p == 1 ? 2 : p == 2 ? 1 : p == 3 ? 0 : p == 4 ? 1 : 0; }
__device__ constexpr int pass_b(int p) { return p == 0 ? 2 : p == 1 ? 0 : p == 2 ? 1 : p == 3 ? 1 : 0; }

// three bf16x8 fragments (pieces) of 8 f32 values, built one value at a time: put<E>() takes value E (in order), done after E = 7
struct Split8 {
  float sv[2], s1[2], s2[2];
  u32x4 q0, q1, q2;
  template <int E>
  __device__ __forceinline__ void put(float v) {
    constexpr int hh = E & 1;
    sv[hh] = v;
    split3f(v, s1[hh], s2[hh]);
    if constexpr (hh == 1) {      // v_perm_b32: high half of the even value | high half of the odd one << 16
      q0[E >> 1] = __builtin_amdgcn_perm(__float_as_uint(sv[1]), __float_as_uint(sv[0]), 0x07060302u);
      q1[E >> 1] = __builtin_amdgcn_perm(__float_as_uint(s1[1]), __float_as_uint(s1[0]), 0x07060302u);
      q2[E >> 1] = __builtin_amdgcn_perm(__float_as_uint(s2[1]), __float_as_uint(s2[0]), 0x07060302u);
    }
  }
  __device__ __forceinline__ void get(bf16x8 (&f)[3]) const {
    f[0] = __builtin_bit_cast(bf16x8, q0);
    f[1] = __builtin_bit_cast(bf16x8, q1);
    f[2] = __builtin_bit_cast(bf16x8, q2);
  }
};

// ------------------------------------------------------------------------------------------------------------------------------
// weight image: [n / 32][k step = K / 16][piece 3][lane 64][8 bf16] of the matrix Wm[k][n],
//   direction 0 (forward):        k = ci,            n = t * cout + co
//   direction 1 (input gradient): k = t * cout + co, n = ci
// with Wm = w[ci * s_ci + co * s_co + a * s_a + b * s_b], t = a * s + b. Lane (r, h), element j of k step 2 c + u: k = 32 c + 16 h + 8 u + j,
// n = 32 nb + r.
__global__ __launch_bounds__(256) void rows_gemm4_weights_kernel(const float* __restrict__ w, int64_t s_ci, int64_t s_co, int64_t s_a,
                                                                 int64_t s_b, unsigned char* __restrict__ img, int cin, int cout, int s,
                                                                 int direction, int K, int N) {
  const int KS = K >> 4;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (nb, k step, lane)
  if (id >= (int64_t)(N >> 5) * KS * 64) return;
  const int lane = (int)(id & 63), r = lane & 31, h = lane >> 5;
  const int ks = (int)((id >> 6) % KS), nb = (int)((id >> 6) / KS);
  const int n = nb * 32 + r, k0 = (ks >> 1) * 32 + h * 16 + (ks & 1) * 8;
  u32x4 q[3];
  unsigned lo[3] = {0, 0, 0};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = k0 + j;
    const int ci = direction ? n : k, tc = direction ? k : n;
    const int t = tc / cout, co = tc - t * cout;
    const float v = w[ci * s_ci + co * s_co + (t / s) * s_a + (t % s) * s_b];
    unsigned p[3];
    split3(v, p[0], p[1], p[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (j & 1) q[i][j >> 1] = lo[i] | (p[i] << 16);
      else lo[i] = p[i];
    }
  }
  unsigned char* dst = img + ((int64_t)(nb * KS + ks) * 3) * 1024 + lane * 16;
#pragma unroll
  for (int i = 0; i < 3; ++i) *reinterpret_cast<u32x4*>(dst + i * 1024) = q[i];
}

// ------------------------------------------------------------------------------------------------------------------------------
constexpr int RG_LDS_BYTES = 4 * 32 * 64 * 16;      // per wave [register quad 32][lane 64] f32x4: the sums of the taps done so far

struct RgArgs {
  const float* x;             // gathered side: rows of ldx floats
  float* y;                   // scattered side: rows of ldy floats
  const unsigned char* wimg;
  int M;                      // rows = input pixels N * H * W
  int W, s;                   // width of the small map, stride (T = s * s)
  int kseg, nseg;             // channels per K segment / N segment
  int tin, tout;              // segments: (1, T) forward, (T, 1) input gradient
  int K, N;                   // kseg * tin, nseg * tout
  int ldx, ldy;
  int wrn;                    // waves along the rows of a workgroup tile: 2 (tile 128 rows x 256 columns) or 4 (256 x 128)
  int col_tiles, tiles;
};

// pixel of the large map that tap (0, 0) of small-map pixel m touches: s (m + (s - 1) W (m / W)); tap (a, b) adds a W s + b
__device__ __forceinline__ unsigned big_pix(int m, int W, int s) { return (unsigned)(s * (m + (s - 1) * W * (m / W))); }

__global__ __launch_bounds__(NT, 1) void rows_gemm4_kernel(RgArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rg_lds[];       // gathered direction only: RG_LDS_BYTES
  asm volatile("" ::: RG_ACC_0_127, RG_ACC_128_255);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave % a.wrn, wc = wave / a.wrn, r = lane & 31, h = lane >> 5;
  const int tile_rows = a.wrn * 64, tile_cols = (4 / a.wrn) * 128;
  const int KC = a.K >> 5, KS = a.K >> 4, kcs = a.kseg >> 5;
  int lt = blockIdx.x, lc = 0;
  if (lt >= a.tiles) return;
  const unsigned char* const wl = a.wimg + lane * 16;
  const int Ws = a.W * a.s;

  static_for<256>([](auto rc) { acc_zero<decltype(rc)::value>(); });

  unsigned xpix[2];           // the lane's rows of the tile the loads belong to, on the gathered side (rows past M: the last row)
  auto set_xpix = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const int m = min((tile / a.col_tiles) * tile_rows + wr * 64 + rb * 32 + r, a.M - 1);
      xpix[rb] = a.tin > 1 ? big_pix(m, a.W, a.s) : (unsigned)m;
    }
  };
  auto load_a = [&](int c, f32x4 (&dst)[2][4]) __attribute__((always_inline)) {
    const int t = c / kcs, cs = c - t * kcs;
    const unsigned tap = a.tin > 1 ? (unsigned)((t / a.s) * Ws + (t % a.s)) : 0u;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const float* p = a.x + (size_t)(xpix[rb] + tap) * a.ldx + cs * 32 + h * 16;
#pragma unroll
      for (int q = 0; q < 4; ++q) dst[rb][q] = *reinterpret_cast<const f32x4*>(p + 4 * q);
    }
  };
  auto load_b = [&](int tile, int ks, bf16x8 (&dst)[4][3]) __attribute__((always_inline)) {
    const int nb0 = ((tile % a.col_tiles) * tile_cols + wc * 128) >> 5;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int p = 0; p < 3; ++p)
        dst[cb][p] = *reinterpret_cast<const bf16x8*>(wl + ((size_t)((nb0 + cb) * KS + ks) * 3 + p) * 1024);
  };
  // D[channel][row] += W^T fragment (first operand, column block cb) . X fragment (second operand, row block rb). Two accumulator sets:
  // block 4 rb + cb takes the pass of the two leading pieces, block 8 + 4 rb + cb the five passes below 2^-8 of it, and the two are added
  // in the epilogue: the large sum is rounded once per 16 k instead of six times (with one set the error against f64 of a 256-deep sum
  // was 5.1e-7 of the largest entry where the vendor kernel had 2.0e-7)
  auto step = [&](const bf16x8 (&Bw)[4][3], const bf16x8 (&Xf)[2][3], auto&& gap) __attribute__((always_inline)) {
    static_for<48>([&](auto kc) __attribute__((always_inline)) {
      constexpr int k = decltype(kc)::value, cb = k / 12, rb = (k / 6) & 1, pass = k % 6;
      mfma_acc<(pass == 5 ? 0 : 8) + 4 * rb + cb>(Bw[cb][pass_a(pass)], Xf[rb][pass_b(pass)]);
      gap(kc);
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  f32x4 Ahi[2][2];
  bf16x8 XF0[2][3], B0[4][3];
  set_xpix(lt);
  {
    f32x4 A0[2][4];
    load_a(0, A0);
    load_b(lt, 0, B0);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      Split8 sp;
      static_for<8>([&](auto ec) { constexpr int e = decltype(ec)::value; sp.put<e>(A0[rb][e >> 2][e & 3]); });
      sp.get(XF0[rb]);
      Ahi[rb][0] = A0[rb][2];
      Ahi[rb][1] = A0[rb][3];
    }
  }
  asm volatile("s_nop 4" ::: "memory");

  for (;;) {
    int nt = lt, nc = lc + 1;
    if (nc == KC) { nc = 0; nt = lt + (int)gridDim.x; }
    const bool more = nt < a.tiles;
    if (!more) { nt = lt; nc = lc; }            // (the last step of the loop requests its own operands again; nobody uses them)
    bf16x8 B1[4][3];
    load_b(lt, 2 * lc + 1, B1);
    if (nt != lt) set_xpix(nt);
    f32x4 An[2][4];
    load_a(nc, An);
    __builtin_amdgcn_sched_barrier(0);

    // k step 0 of these 32 k; in its gaps the split of k step 1
    bf16x8 XF1[2][3];
    Split8 sp;
    step(B0, XF0, [&](auto kc) __attribute__((always_inline)) {
      constexpr int k = decltype(kc)::value;
      if constexpr (k < 16) {
        constexpr int rb = k >> 3, e = k & 7;
        sp.put<e>(Ahi[rb][e >> 2][e & 3]);
        if constexpr (e == 7) sp.get(XF1[rb]);
      }
    });
    bf16x8 B0n[4][3];
    load_b(nt, 2 * nc, B0n);
    __builtin_amdgcn_sched_barrier(0);
    // k step 1; in its gaps the split of k step 0 of the next 32 k
    bf16x8 XF0n[2][3];
    step(B1, XF1, [&](auto kc) __attribute__((always_inline)) {
      constexpr int k = decltype(kc)::value;
      if constexpr (k >= 24 && k < 40) {
        constexpr int rb = (k - 24) >> 3, e = (k - 24) & 7;
        sp.put<e>(An[rb][e >> 2][e & 3]);
        if constexpr (e == 7) sp.get(XF0n[rb]);
      }
    });

    if (a.tin > 1 && lc != KC - 1 && (lc + 1) % kcs == 0) {
      // ---- gathered direction, a tap is complete: the large sum moves to LDS (added there in f32, round to nearest) and the accumulators
      //      start the next tap from zero. The matrix pipe truncates what it adds to a large accumulator: one chain over the 64 k steps of
      //      the bench layer's input gradient was 5.3e-7 of the largest entry from f64 on a small map where the vendor kernel had 2.6e-7
      f32x4* const part = reinterpret_cast<f32x4*>(rg_lds) + wave * (32 * 64) + lane;
      const bool first = lc + 1 == kcs;
      acc_settle();
      static_for<32>([&](auto qc) __attribute__((always_inline)) {
        constexpr int R0 = 4 * decltype(qc)::value;
        f32x4 v = (f32x4){acc_read<R0>(), acc_read<R0 + 1>(), acc_read<R0 + 2>(), acc_read<R0 + 3>()};
        if (!first) v += part[decltype(qc)::value * 64];
        part[decltype(qc)::value * 64] = v;
      });
      static_for<128>([](auto rc) { acc_zero<decltype(rc)::value>(); });
      asm volatile("s_nop 4" ::: "memory");
    }
    if (lc == KC - 1) {
      // ---- the tile is complete: accumulator register 4 j + e of block (rb, cb) = row 32 rb + r, channel 32 cb + 8 j + 4 h + e
      const int ctile = lt % a.col_tiles;
      const int col0 = ctile * tile_cols + wc * 128;
      const int tseg = col0 / a.nseg, ncol = col0 - tseg * a.nseg;
      const unsigned tap = a.tout > 1 ? (unsigned)((tseg / a.s) * Ws + (tseg % a.s)) : 0u;
      acc_settle();
      static_for<2>([&](auto rbc) __attribute__((always_inline)) {
        constexpr int rb = decltype(rbc)::value;
        const int m = (lt / a.col_tiles) * tile_rows + wr * 64 + rb * 32 + r;
        const bool ok = m < a.M;
        const unsigned pix = (a.tout > 1 ? big_pix(min(m, a.M - 1), a.W, a.s) : (unsigned)m) + tap;
        float* const out = a.y + (size_t)pix * a.ldy + ncol + 4 * h;
        static_for<16>([&](auto qc) __attribute__((always_inline)) {
          constexpr int cb = decltype(qc)::value >> 2, j = decltype(qc)::value & 3, R0 = (4 * rb + cb) * 16 + 4 * j;
          f32x4 v = (f32x4){acc_read<R0>() + acc_read<128 + R0>(), acc_read<R0 + 1>() + acc_read<129 + R0>(),
                            acc_read<R0 + 2>() + acc_read<130 + R0>(), acc_read<R0 + 3>() + acc_read<131 + R0>()};
          if (a.tin > 1) v += (reinterpret_cast<const f32x4*>(rg_lds) + wave * (32 * 64) + lane)[(R0 / 4) * 64];
          if (ok) *reinterpret_cast<f32x4*>(out + cb * 32 + 8 * j) = v;
        });
      });
      static_for<256>([](auto rc) { acc_zero<decltype(rc)::value>(); });
      asm volatile("s_nop 4" ::: "memory");
    }
    if (!more) break;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      Ahi[rb][0] = An[rb][2];
      Ahi[rb][1] = An[rb][3];
#pragma unroll
      for (int p = 0; p < 3; ++p) XF0[rb][p] = XF0n[rb][p];
    }
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int p = 0; p < 3; ++p) B0[cb][p] = B0n[cb][p];
    lt = nt;
    lc = nc;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
constexpr int WCB = 256;                          // channels per workgroup on either side
constexpr int WIMG_G = WCB * 16;                  // one k group: [channel 256][8 bf16] = 4096 bytes
constexpr int WIMG_P = 2 * WIMG_G;                // one piece: two k groups
constexpr int WIMG_OP = 3 * WIMG_P;               // one operand: 24576 bytes
constexpr int WIMG_BUF = 2 * WIMG_OP;             // X and dY
constexpr int WLDS_BYTES = 2 * WIMG_BUF;          // double-buffered: 98304 bytes

struct RwArgs {
  const float* x;      // (M, cin)
  const float* dy;     // (pixels of the large map, cout)
  float* part;         // (ranges, blocks, 256 ci, 256 co)
  int M, W, s, T;
  int cin, cout, nci, nco;
  int nchunks;         // ceil(M / 16)
  int nranges;         // multiple of 8
};

__global__ __launch_bounds__(NT, 1) void rows_gemm4_wgrad_kernel(RwArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  asm volatile("" ::: RG_ACC_0_127, RG_ACC_128_255);
  const int c = threadIdx.x, lane = c & 63, wave = __builtin_amdgcn_readfirstlane(c >> 6);
  // the workgroups of ONE range read the same rows: same XCD
  const int nb = a.T * a.nci * a.nco;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int sub = slot % nb, range = (slot / nb) * 8 + xcd;
  if (range >= a.nranges) return;
  const int t = sub % a.T, blk = sub / a.T;
  const int cib = blk / a.nco, cob = blk - cib * a.nco;
  const int c_first = (int)((int64_t)range * a.nchunks / a.nranges);
  const int c_end = (int)((int64_t)(range + 1) * a.nchunks / a.nranges);
  const int total = c_end - c_first;              // (0 with more ranges than chunks: a zero partial)

  static_for<256>([](auto rc) { acc_zero<decltype(rc)::value>(); });

  const float* const xp = a.x + cib * WCB + c;
  const float* const gp = a.dy + cob * WCB + c;
  const unsigned tap = (unsigned)((t / a.s) * (a.W * a.s) + (t % a.s));
  // row cursors of the requests (rows are requested strictly in order): x row, and the row of dy with its position in the small map
  int xm = c_first * 16;
  int gm = xm, gq = gm / a.W, gr = gm - gq * a.W;
  float val[32];                                   // [0..15] x rows of a chunk, [16..31] dy rows, as loaded (rows past M: the last row's)
  unsigned gpix = tap;
  auto request = [&](auto ic) __attribute__((always_inline)) {
    constexpr int i = decltype(ic)::value;
    if constexpr (i < 16) {
      val[i] = xp[(size_t)min(xm, a.M - 1) * a.cin];
      ++xm;
    } else {
      if (gm < a.M) gpix = (unsigned)(a.s * (gm + (a.s - 1) * a.W * gq)) + tap;
      val[i] = gp[(size_t)gpix * a.cout];
      ++gm;
      if (++gr == a.W) { gr = 0; ++gq; }
    }
  };
  // value i of the chunk whose first row is m0 -> images of buffer `buf` (rows past M count as zero): 8 values = the 8 consecutive k
  // of one MFMA lane: one 16-byte store per piece
  Split8 sp;
  auto value = [&](auto ic, unsigned char* buf, int m0) __attribute__((always_inline)) {
    constexpr int i = decltype(ic)::value, e = i & 7, g = (i >> 3) & 1, op = i >> 4;
    sp.put<e>(m0 + (i & 15) < a.M ? val[i] : 0.f);
    if constexpr (e == 7) {
      unsigned char* const dst = buf + op * WIMG_OP + g * WIMG_G + c * 16;
      *reinterpret_cast<u32x4*>(dst) = sp.q0;
      *reinterpret_cast<u32x4*>(dst + WIMG_P) = sp.q1;
      *reinterpret_cast<u32x4*>(dst + 2 * WIMG_P) = sp.q2;
    }
  };

  // MFMA role: wave = input-channel half wi (second operand: columns) x output-channel half wo (first operand: rows); accumulator
  // block 4 bo + bi
  const int wi = wave & 1, wo = wave >> 1, l31 = lane & 31, lhi = lane >> 5;
  const int a_rd = WIMG_OP + lhi * WIMG_G + (wo * 128 + l31) * 16;       // dy image
  const int b_rd = lhi * WIMG_G + (wi * 128 + l31) * 16;                  // x image

  if (total > 0) {
    static_for<32>([&](auto ic) __attribute__((always_inline)) { request(ic); });
    static_for<32>([&](auto ic) __attribute__((always_inline)) { value(ic, lds, c_first * 16); });
    static_for<32>([&](auto ic) __attribute__((always_inline)) { request(ic); });       // chunk 1 (past the end: clamped rows, unused)
    __syncthreads();
    for (int q = 0; q < total; ++q) {
      const unsigned char* const cur = lds + (q & 1) * WIMG_BUF;
      unsigned char* const nxt = lds + ((q + 1) & 1) * WIMG_BUF;
      bf16x8 A[4][3], B[4][3];
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          if (b == 0) A[0][p] = *reinterpret_cast<const bf16x8*>(cur + a_rd + p * WIMG_P);
          B[b][p] = *reinterpret_cast<const bf16x8*>(cur + b_rd + p * WIMG_P + b * 32 * 16);
        }
#pragma unroll
      for (int b = 1; b < 4; ++b)
#pragma unroll
        for (int p = 0; p < 3; ++p) A[b][p] = *reinterpret_cast<const bf16x8*>(cur + a_rd + p * WIMG_P + b * 32 * 16);
      __builtin_amdgcn_sched_barrier(0);
      // in the gaps: value i of chunk q + 1 (requested one chunk ago) into the other buffer, then the request of value i of chunk q + 2
      static_for<96>([&](auto kc) __attribute__((always_inline)) {
        constexpr int k = decltype(kc)::value, bo = k / 24, bi = (k / 6) & 3, pass = k % 6;
        mfma_acc<4 * bo + bi>(A[bo][pass_a(pass)], B[bi][pass_b(pass)]);
        if constexpr ((k & 1) == 0 && k < 64) {
          value(std::integral_constant<int, k / 2>{}, nxt, (c_first + q + 1) * 16);
          request(std::integral_constant<int, k / 2>{});
        }
        __builtin_amdgcn_sched_barrier(0);
      });
      __syncthreads();
    }
  }

  // partial block [ci 256][co 256]: accumulator register 4 j + e of block (bo, bi): output channel 32 bo + 8 j + 4 lhi + e, input
  // channel 32 bi + l31
  acc_settle();
  float* const out = a.part + ((int64_t)range * nb + sub) * (WCB * WCB) + (wi * 128 + l31) * WCB + wo * 128 + 4 * lhi;
  static_for<64>([&](auto qc) {
    constexpr int Q = decltype(qc)::value, B = Q >> 2, j = Q & 3, bo = B >> 2, bi = B & 3;
    const f32x4 v = (f32x4){acc_read<B * 16 + 4 * j>(), acc_read<B * 16 + 4 * j + 1>(), acc_read<B * 16 + 4 * j + 2>(),
                            acc_read<B * 16 + 4 * j + 3>()};
    *reinterpret_cast<f32x4*>(out + bi * 32 * WCB + bo * 32 + 8 * j) = v;
  });
}

// dW[ci][co][a][b] = sum over the ranges in range order (double), written with the element strides of the weight tensor
__global__ __launch_bounds__(256) void rows_gemm4_wgrad_reduce_kernel(const float* __restrict__ part, int nranges, int T, int nci, int nco,
                                                                      int s, float* __restrict__ dw, int64_t s_ci, int64_t s_co,
                                                                      int64_t s_a, int64_t s_b) {
  const int sub = blockIdx.x / WCB, cil = blockIdx.x - sub * WCB, col = threadIdx.x;
  const int t = sub % T, blk = sub / T, cib = blk / nco, cob = blk - cib * nco;
  const int64_t nb = (int64_t)T * nci * nco;
  const float* p = part + (int64_t)sub * (WCB * WCB) + cil * WCB + col;
  double sum = 0.0;
#pragma unroll 8
  for (int r = 0; r < nranges; ++r) sum += (double)p[r * nb * (WCB * WCB)];
  dw[(int64_t)(cib * WCB + cil) * s_ci + (int64_t)(cob * WCB + col) * s_co + (t / s) * s_a + (t % s) * s_b] = (float)sum;
}

__host__ int rg_cu_count() {
  static std::atomic<int> n_cu{0};
  int n = n_cu.load(std::memory_order_relaxed);
  if (!n) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
    n = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    n_cu.store(n, std::memory_order_relaxed);
  }
  return n;
}

// ranges so that the workgroups fill the CUs TWICE (a multiple of 8: XCD placement): a workgroup adds six MFMA results per 16 rows into
// its f32 accumulators, and chains of half the length keep the error against f64 at the level it has in crb_winograd4_wgrad
__host__ int rg_wgrad_ranges(int nb) {
  const int r = (2 * rg_cu_count() / nb) & ~7;
  return r < 8 ? 8 : r;
}

__host__ bool rg_shape_ok(int cin, int cout, int stride) {
  return cin > 0 && cout > 0 && (stride == 1 || stride == 2) && cin <= 4096 && cout <= 4096;
}

__host__ int rg_launch(const float* x, const void* img, float* y, int64_t M, int W, int s, int kseg, int nseg, int tin, int tout,
                       void* stream) {
  RgArgs a;
  a.x = x; a.y = y; a.wimg = (const unsigned char*)img;
  a.M = (int)M; a.W = W; a.s = s;
  a.kseg = kseg; a.nseg = nseg; a.tin = tin; a.tout = tout;
  a.K = kseg * tin; a.N = nseg * tout;
  a.ldx = kseg; a.ldy = nseg;
  a.wrn = a.N % 256 == 0 ? 2 : 4;
  const int tile_rows = a.wrn * 64, tile_cols = (4 / a.wrn) * 128;
  a.col_tiles = a.N / tile_cols;
  const int64_t tiles = ((M + tile_rows - 1) / tile_rows) * a.col_tiles;
  if (tiles >= (1LL << 30)) return CRB_ERR_ARG;
  a.tiles = (int)tiles;
  const int grid = (int)(tiles < rg_cu_count() ? tiles : rg_cu_count());
  static std::atomic<unsigned> attr_done[64];
  int dev = 0;
  CRB_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return CRB_ERR_ARG;
  if (tin > 1 && !attr_done[dev].load(std::memory_order_acquire)) {
    CRB_HIP(hipFuncSetAttribute((const void*)rows_gemm4_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RG_LDS_BYTES));
    attr_done[dev].store(1u, std::memory_order_release);
  }
  hipLaunchKernelGGL(rows_gemm4_kernel, dim3((unsigned)grid), dim3(NT), tin > 1 ? RG_LDS_BYTES : 0, (hipStream_t)stream, a);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

}  // namespace

// direction 0 = forward, 1 = input gradient, 2 = weight gradient
extern "C" int crb_rows_gemm4_supported(int cin, int cout, int stride, int direction) {
  if (!rg_shape_ok(cin, cout, stride)) return 0;
  if (direction == 0) return (cin % 32 == 0 && cout % 128 == 0) ? 1 : 0;
  if (direction == 1) return (cout % 32 == 0 && cin % 128 == 0) ? 1 : 0;
  if (direction == 2) return (cin % WCB == 0 && cout % WCB == 0) ? 1 : 0;
  return 0;
}

extern "C" int64_t crb_rows_gemm4_weights_bytes(int cin, int cout, int stride) {
  if (!rg_shape_ok(cin, cout, stride)) return 0;
  return (int64_t)stride * stride * cin * cout * 6;
}

extern "C" int crb_rows_gemm4_weights(const float* w, int64_t s_ci, int64_t s_co, int64_t s_a, int64_t s_b, void* image, int cin,
                                      int cout, int stride, int direction, void* stream) {
  if (direction != 0 && direction != 1) return CRB_ERR_ARG;
  if (!crb_rows_gemm4_supported(cin, cout, stride, direction)) return CRB_ERR_UNSUPPORTED;
  if (!w || !image) return CRB_ERR_ARG;
  const int T = stride * stride;
  const int K = direction ? T * cout : cin, N = direction ? cin : T * cout;
  const int64_t threads = (int64_t)(N / 32) * (K / 16) * 64;
  hipLaunchKernelGGL(rows_gemm4_weights_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, s_ci, s_co,
                     s_a, s_b, (unsigned char*)image, cin, cout, stride, direction, K, N);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_rows_gemm4_forward(const float* x, const void* image, float* y, int N, int H, int W, int cin, int cout, int stride,
                                      void* stream) {
  if (N <= 0 || H <= 0 || W <= 0 || !x || !image || !y) return CRB_ERR_ARG;
  if (!crb_rows_gemm4_supported(cin, cout, stride, 0)) return CRB_ERR_UNSUPPORTED;
  const int64_t M = (int64_t)N * H * W, T = stride * stride;
  if (M * T * (cin > cout ? cin : cout) >= (1LL << 31)) return CRB_ERR_ARG;
  return rg_launch(x, image, y, M, W, stride, cin, cout, 1, (int)T, stream);
}

extern "C" int crb_rows_gemm4_input_grad(const float* dy, const void* image, float* dx, int N, int H, int W, int cin, int cout,
                                         int stride, void* stream) {
  if (N <= 0 || H <= 0 || W <= 0 || !dy || !image || !dx) return CRB_ERR_ARG;
  if (!crb_rows_gemm4_supported(cin, cout, stride, 1)) return CRB_ERR_UNSUPPORTED;
  const int64_t M = (int64_t)N * H * W, T = stride * stride;
  if (M * T * (cin > cout ? cin : cout) >= (1LL << 31)) return CRB_ERR_ARG;
  return rg_launch(dy, image, dx, M, W, stride, cout, cin, (int)T, 1, stream);
}

extern "C" int64_t crb_rows_gemm4_wgrad_workspace_bytes(int cin, int cout, int stride) {
  if (!crb_rows_gemm4_supported(cin, cout, stride, 2)) return 0;
  const int nb = stride * stride * (cin / WCB) * (cout / WCB);
  return (int64_t)rg_wgrad_ranges(nb) * nb * WCB * WCB * 4;
}

extern "C" int crb_rows_gemm4_wgrad(const float* x, const float* dy, float* dw, int64_t s_ci, int64_t s_co, int64_t s_a, int64_t s_b,
                                    int N, int H, int W, int cin, int cout, int stride, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
  if (N <= 0 || H <= 0 || W <= 0 || !x || !dy || !dw) return CRB_ERR_ARG;
  if (!crb_rows_gemm4_supported(cin, cout, stride, 2)) return CRB_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < crb_rows_gemm4_wgrad_workspace_bytes(cin, cout, stride)) return CRB_ERR_WORKSPACE;
  const int64_t M = (int64_t)N * H * W, T = stride * stride;
  if (M * T * (cin > cout ? cin : cout) >= (1LL << 31)) return CRB_ERR_ARG;
  static std::atomic<unsigned> attr_done[64];
  int dev = 0;
  CRB_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return CRB_ERR_ARG;
  if (!attr_done[dev].load(std::memory_order_acquire)) {
    CRB_HIP(hipFuncSetAttribute((const void*)rows_gemm4_wgrad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, WLDS_BYTES));
    attr_done[dev].store(1u, std::memory_order_release);
  }
  RwArgs a;
  a.x = x; a.dy = dy; a.part = (float*)workspace;
  a.M = (int)M; a.W = W; a.s = stride; a.T = (int)T;
  a.cin = cin; a.cout = cout; a.nci = cin / WCB; a.nco = cout / WCB;
  a.nchunks = (int)((M + 15) / 16);
  const int nb = a.T * a.nci * a.nco;
  a.nranges = rg_wgrad_ranges(nb);
  hipLaunchKernelGGL(rows_gemm4_wgrad_kernel, dim3((unsigned)(a.nranges * nb)), dim3(NT), WLDS_BYTES, (hipStream_t)stream, a);
  CRB_CHECK_LAUNCH();
  hipLaunchKernelGGL(rows_gemm4_wgrad_reduce_kernel, dim3((unsigned)(nb * WCB)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)workspace, a.nranges, a.T, a.nci, a.nco, stride, dw, s_ci, s_co, s_a, s_b);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
