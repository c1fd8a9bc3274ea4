// Backward of  BatchNorm(train) -> ReLU -> concat -> linear head  without the gradient of the concatenated map.
// The map z (n, Ct = sum C_i) is relu(gamma xhat + beta) of the branch inputs x_i (n, C_i), the head is out = z W^T + b with W (K, Ct),
// K = 72 at the KITTI head. dz = dOut W has rank K; with mask = [gamma xhat + beta > 0], xhat = (x - mean) invstd:
//     P2[k][c] = sum_r dOut[r][k] mask[r][c]                 P3[k][c] = sum_r dOut[r][k] mask[r][c] xhat[r][c]
//     dbeta_c = sum_k W[k][c] P2[k][c]      dgamma_c = sum_k W[k][c] P3[k][c]      dW[k][c] = gamma_c P3[k][c] + beta_c P2[k][c]
//     dx[r][c] = gamma_c invstd_c (mask (dOut[r][:] . W[:][c]) - dbeta_c / n - xhat dgamma_c / n)
// so neither dz nor z is read or written: launch A (head_bn_sums_kernel + reduce) streams x and dOut once, the finalize is tiny, launch B
// (head_bn_apply_kernel) streams dOut and x and writes dx. All products run on the bf16 matrix pipe through the exact three-way split of
// winograd_split.h (six passes with piece indices i + j <= 2; the mask is exact in one piece: three passes). An Inf operand becomes NaN,
// pieces below ~2^-110 of a tiny value are flushed: the behaviour of the other split kernels. No atomics, fixed order: bit-reproducible.
//
// Both kernels: wave = one block of 32 channels (the MFMA column = the lane, so the per-channel constants are seven registers of the
// lane and a load / store instruction covers two whole 128-byte lines of a row), workgroup = 4 waves = 128 consecutive channels of the
// same rows (the dOut lines of three of the four waves hit in L1), two workgroups per CU. No LDS.
//   A: the contraction index is the row. Lane (r, h) of the MFMA wants dOut[8 rows 8 h + j][k = 32 kb + r] and M[8 rows 8 h + j][channel r]:
//      for a fixed j the 32 lanes of a half read 128 consecutive bytes, so both operands are loaded in MFMA order by 4-byte loads and
//      split in registers. A chunk's nine passes are summed by the matrix pipe from zero and added to f32 running sums (round to nearest).
//      Workgroup = one range of 16-row chunks; partials [range][P2 | P3][K][Ct] f32, added in a fixed order in double by
//      head_bn_reduce_kernel. The column sums of dOut (the head's bias gradient) are kept in double by one wave per range.
//   B: D[row][channel] = dOut[row][k] . W[k][channel]; the wave holds the split image of its 32 columns of W in registers (built once
//      per call by head_bn_weights_kernel in lane order) and walks 8 blocks of 32 rows. The five passes below 2^-8 of the product go into
//      the accumulator first, the leading pass of every k step last: the matrix pipe truncates what it adds to a large accumulator, so the
//      large sum is added ceil(K / 16) times. Epilogue: bn_bwd_apply_kernel's expression, in its order (-ffp-contract=off).
// k past K is zero IN REGISTERS, rows past n count as zero / are not stored: their loads go to the last entries of the row / the last row of
// the chunk instead (unconditional loads at clamped offsets from a uniform base), nothing is read past a row's end or past row n - 1.
//
// The forward of the same region, out = relu(bn(x)) W^T + b from the branch inputs without writing z, is head_bn_forward_kernel below
// (its own comment): with it z does not exist in a training step.
#include <atomic>
#include <type_traits>
#include <utility>
#include "crb_common.h"
#include "winograd_split.h"
#include "../../include/crb_hip.h"

typedef float hb_f32x4 __attribute__((ext_vector_type(4)));
typedef float hb_f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int HB_NT = 256;
constexpr int HB_RBG = 8;                 // B: blocks of 32 rows per workgroup
constexpr int HB_COLP = 96;               // column-sum partial slots per (range, lane half)

template <typename F, int... I>
__device__ __forceinline__ void hb_static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void hb_static_for(F&& f) { hb_static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// the six passes, smallest products first: piece of the first / second operand
__device__ constexpr int hb_pass_a(int p) { return p == 0 ? 0 : p == 1 ? 2 : p == 2 ? 1 : p == 3 ? 0 : p == 4 ? 1 : 0; }
__device__ constexpr int hb_pass_b(int p) { return p == 0 ? 2 : p == 1 ? 0 : p == 2 ? 1 : p == 3 ? 1 : 0; }

__device__ __forceinline__ hb_f32x16 hb_mfma(const bf16x8& a, const bf16x8& b, const hb_f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// three bf16x8 fragments (pieces) of 8 f32 values, built one value at a time (rows_gemm4.hip)
struct HbSplit8 {
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

// the forward kernel's accumulators: block B (16 registers) = a[16 B : 16 B + 15] by name (rows_gemm4.hip: as C++ values the register
// allocator copies accumulator tuples around the MFMAs and spills). MFMA -> v_accvgpr_read needs wait states: hb_acc_settle()
template <int B>
__device__ __forceinline__ void hb_mfma_acc(const bf16x8& A, const bf16x8& Bv) {
  asm volatile("v_mfma_f32_32x32x16_bf16 a[%2:%3], %0, %1, a[%2:%3]" : : "v"(A), "v"(Bv), "n"(B * 16), "n"(B * 16 + 15));
}
template <int R>
__device__ __forceinline__ float hb_acc_read() {
  float x;
  asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(x) : "n"(R));
  return x;
}
template <int R>
__device__ __forceinline__ void hb_acc_zero() { asm volatile("v_accvgpr_write_b32 a[%0], 0" : : "n"(R)); }
__device__ __forceinline__ void hb_acc_settle() { asm volatile("s_nop 15\n\ts_nop 15" ::: "memory"); }

#define HB_ACC_0_127                                                                                                                   \
  "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17", "a18", "a19",   \
      "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33", "a34", "a35", "a36", "a37",   \
      "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55",   \
      "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73",   \
      "a74", "a75", "a76", "a77", "a78", "a79", "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", "a91",   \
      "a92", "a93", "a94", "a95", "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106", "a107", "a108", \
      "a109", "a110", "a111", "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124", \
      "a125", "a126", "a127"
#define HB_ACC_128_255                                                                                                                 \
  "a128", "a129", "a130", "a131", "a132", "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140", "a141", "a142", "a143",     \
      "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156", "a157", "a158", "a159", \
      "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175", \
      "a176", "a177", "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191", \
      "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207", \
      "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222", "a223", \
      "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237", "a238", "a239", \
      "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252", "a253", "a254", "a255"

// ------------------------------------------------------------------------------------------------------------------------------
// par (4, Ct): mean | invstd | gamma | beta of the concatenated channels
struct HsArgs {
  const float* x0;
  const float* x1;
  const float* par;
  const float* dout;          // (n, K)
  float* part;                // (nranges, 2, K, Ct)
  double* colpart;            // (nranges, 2, HB_COLP)
  int64_t n;
  int C, Ct, K, ncg;          // branch width, sum of widths, head outputs, groups of 128 channels
  int nchunks, nranges;       // ceil(n / 16)
};

template <int NKB>
__global__ __launch_bounds__(HB_NT, 2) void head_bn_sums_kernel(HsArgs a) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int cg = blockIdx.x % a.ncg, range = blockIdx.x / a.ncg;
  const int cb = cg * 4 + wave, c = cb * 32 + r;
  const int branch = (cb * 32) / a.C;
  const float* const xbase = branch ? a.x1 : a.x0;
  const unsigned cl = (unsigned)(c - branch * a.C);
  const float mu = a.par[c], is = a.par[a.Ct + c], ga = a.par[2 * a.Ct + c], be = a.par[3 * a.Ct + c];
  const int c_first = (int)((int64_t)range * a.nchunks / a.nranges);
  const int c_end = (int)((int64_t)(range + 1) * a.nchunks / a.nranges);      // (== c_first with more ranges than chunks: a zero partial)
  const bool do_col = cg == 0 && wave == 0;

  // running sums in f32, round to nearest: every chunk's products are summed by the matrix pipe from zero and added here. One MFMA chain
  // over the 275 chunks of a bench-size range truncates 9 times per chunk into the large sum (dgamma 2.5e-6 of the largest entry from f64
  // at 563,200 rows where the reduce pass it replaces had 2.1e-7)
  hb_f32x16 s2[NKB], s3[NKB];
  double colsum[NKB];
  bool kin[NKB];
  unsigned kc[NKB];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
    for (int i = 0; i < 16; ++i) { s2[kb][i] = 0.f; s3[kb][i] = 0.f; }
    colsum[kb] = 0.0;
    kin[kb] = 32 * kb + r < a.K;
    kc[kb] = (unsigned)(kin[kb] ? 32 * kb + r : a.K - 1);           // k past K: the row's last entry is loaded and not used
  }

  // the lane's 8 rows of chunk q (rows past n: the chunk's last row, not used): x of its channel, dOut of its k of every block.
  // Unconditional loads at clamped offsets from a uniform base: no branch, no wait between them
  auto load = [&](int q, float (&xv)[8], float (&dv)[NKB][8]) __attribute__((always_inline)) {
    const int64_t r0 = (int64_t)q * 16, rem = a.n - r0;
    const unsigned last = (unsigned)(rem < 16 ? rem : 16) - 1u;
    const float* const xq = xbase + r0 * a.C;
    const float* const dq = a.dout + r0 * a.K;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned rj = min((unsigned)(8 * h + j), last);
      xv[j] = xq[rj * (unsigned)a.C + cl];
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) dv[kb][j] = dq[rj * (unsigned)a.K + kc[kb]];
    }
  };

  float xv[8], dv[NKB][8];
  if (c_first < c_end) load(c_first, xv, dv);
  for (int q = c_first; q < c_end; ++q) {
    float xn[8], dn[NKB][8];
    load(q + 1 < c_end ? q + 1 : q, xn, dn);
    const int64_t left64 = a.n - ((int64_t)q * 16 + 8 * h);
    const int left = left64 < 8 ? (int)left64 : 8;                   // rows of the lane's eight that exist (may be <= 0)

    HbSplit8 sx;
    u32x4 mk;
    unsigned mlo = 0;
    hb_static_for<8>([&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      const float xh = (xv[j] - mu) * is;
      const float z = ga * xh + be;
      const bool m = j < left && z > 0.f;
      sx.put<j>(m ? xh : 0.f);
      const unsigned mb = m ? 0x3f80u : 0u;                          // 1.0 as bf16
      if constexpr (j & 1) mk[j >> 1] = mlo | (mb << 16);
      else mlo = mb;
    });
    bf16x8 X[3];
    sx.get(X);
    const bf16x8 Mk = __builtin_bit_cast(bf16x8, mk);

    hb_static_for<NKB>([&](auto kc_) __attribute__((always_inline)) {
      constexpr int kb = decltype(kc_)::value;
      HbSplit8 sd;
      float d[8];
      hb_static_for<8>([&](auto jc) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value;
        d[j] = (j < left && kin[kb]) ? dv[kb][j] : 0.f;
        sd.put<j>(d[j]);
      });
      if (do_col) {                       // (uniform: one wave per range)
#pragma unroll
        for (int j = 0; j < 8; ++j) colsum[kb] += (double)d[j];
      }
      bf16x8 D[3];
      sd.get(D);
      hb_f32x16 t2, t3;
#pragma unroll
      for (int i = 0; i < 16; ++i) { t2[i] = 0.f; t3[i] = 0.f; }
      t2 = hb_mfma(D[2], Mk, t2);
      t2 = hb_mfma(D[1], Mk, t2);
      t2 = hb_mfma(D[0], Mk, t2);
      hb_static_for<6>([&](auto pc) __attribute__((always_inline)) {
        constexpr int p = decltype(pc)::value;
        t3 = hb_mfma(D[hb_pass_a(p)], X[hb_pass_b(p)], t3);
      });
      s2[kb] += t2;
      s3[kb] += t3;
    });
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xv[j] = xn[j];
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) dv[kb][j] = dn[kb][j];
    }
  }

  // register i of block kb: k = 32 kb + (i & 3) + 8 (i >> 2) + 4 h, channel = the lane's
  float* const p2 = a.part + ((int64_t)range * 2) * a.K * a.Ct + c;
  float* const p3 = p2 + (int64_t)a.K * a.Ct;
  hb_static_for<NKB>([&](auto kc_) __attribute__((always_inline)) {
    constexpr int kb = decltype(kc_)::value;
    hb_static_for<16>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      const int k = 32 * kb + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (k < a.K) {
        p2[(int64_t)k * a.Ct] = s2[kb][i];
        p3[(int64_t)k * a.Ct] = s3[kb][i];
      }
    });
    if (do_col) a.colpart[((int64_t)range * 2 + h) * HB_COLP + 32 * kb + r] = colsum[kb];
  });
}

// sums (2 K Ct + K) f64: P2 | P3 | column sums of dOut. 256 threads = 32 entries x 8 slices of the ranges (range g in slice g % 8), the
// slices added in slice order through LDS: a fixed order
__global__ __launch_bounds__(256) void head_bn_reduce_kernel(const float* __restrict__ part, const double* __restrict__ colpart,
                                                             int nranges, int K, int Ct, double* __restrict__ sums) {
  __shared__ double sh[8][32];
  const int64_t per = (int64_t)2 * K * Ct;
  const int il = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int64_t id = (int64_t)blockIdx.x * 32 + il;
  double s = 0.0;
  if (id < per) {
    for (int g = sl; g < nranges; g += 8) s += (double)part[g * per + id];
  } else if (id < per + K) {
    for (int g = sl; g < 2 * nranges; g += 8) s += colpart[(int64_t)g * HB_COLP + (id - per)];
  }
  sh[sl][il] = s;
  __syncthreads();
  if (sl == 0 && id < per + K) {
    for (int k = 1; k < 8; ++k) s += sh[k][il];
    sums[id] = s;
  }
}

// dgb (2, Ct) = dbeta | dgamma, dw (K, Ct), dbias (K) (may be NULL), all from the f64 sums. 256 threads = 32 channels x 8 slices of k
// (k in slice k % 8), the slices added in slice order through LDS
__global__ __launch_bounds__(256) void head_bn_finalize_kernel(const double* __restrict__ sums, const float* __restrict__ w,
                                                               const float* __restrict__ par, int K, int Ct, float* __restrict__ dgb,
                                                               float* __restrict__ dw, float* __restrict__ dbias) {
  __shared__ double sb[8][32], sg[8][32];
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;                     // Ct is a multiple of 32
  const double ga = (double)par[2 * Ct + c], be = (double)par[3 * Ct + c];
  double db = 0.0, dg = 0.0;
  for (int k = sl; k < K; k += 8) {
    const double p2 = sums[(int64_t)k * Ct + c], p3 = sums[(int64_t)(K + k) * Ct + c], wk = (double)w[(int64_t)k * Ct + c];
    db += wk * p2;
    dg += wk * p3;
    dw[(int64_t)k * Ct + c] = (float)(ga * p3 + be * p2);
  }
  sb[sl][cl] = db;
  sg[sl][cl] = dg;
  __syncthreads();
  if (sl == 0) {
    for (int k = 1; k < 8; ++k) { db += sb[k][cl]; dg += sg[k][cl]; }
    dgb[c] = (float)db;
    dgb[Ct + c] = (float)dg;
  }
  if (dbias && blockIdx.x == 0 && (int)threadIdx.x < K) dbias[threadIdx.x] = (float)sums[(int64_t)2 * K * Ct + threadIdx.x];
}

// ------------------------------------------------------------------------------------------------------------------------------
// image [Ct / 32][k step NKS][piece 3][lane 64][8 bf16] of W (K, Ct): lane (r, h), element j of k step ks holds W[16 ks + 8 h + j][32 cb + r]
// (zero past K)
__global__ __launch_bounds__(256) void head_bn_weights_kernel(const float* __restrict__ w, unsigned char* __restrict__ img, int K, int Ct,
                                                              int NKS) {
  const int id = blockIdx.x * 256 + threadIdx.x;         // (cb, k step, lane)
  if (id >= (Ct >> 5) * NKS * 64) return;
  const int lane = id & 63, r = lane & 31, h = lane >> 5;
  const int ks = (id >> 6) % NKS, cb = (id >> 6) / NKS;
  u32x4 q[3];
  unsigned lo[3] = {0, 0, 0};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 16 * ks + 8 * h + j;
    const float v = k < K ? w[(int64_t)k * Ct + cb * 32 + r] : 0.f;
    unsigned p[3];
    split3(v, p[0], p[1], p[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (j & 1) q[i][j >> 1] = lo[i] | (p[i] << 16);
      else lo[i] = p[i];
    }
  }
  unsigned char* dst = img + ((int64_t)(cb * NKS + ks) * 3) * 1024 + lane * 16;
#pragma unroll
  for (int i = 0; i < 3; ++i) *reinterpret_cast<u32x4*>(dst + i * 1024) = q[i];
}

struct HaArgs {
  const float* x0;
  const float* x1;
  float* dx0;
  float* dx1;
  const float* par;           // (4, Ct)
  const float* dgb;           // (2, Ct) dbeta | dgamma
  const float* dout;          // (n, K)
  const unsigned char* wimg;
  int64_t n, nrb;             // rows, blocks of 32 rows
  int C, Ct, K, ncg;
  float inv_n;
};

template <int NKS>
__global__ __launch_bounds__(HB_NT, 2) void head_bn_apply_kernel(HaArgs a) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int cg = blockIdx.x % a.ncg;
  const int64_t rg = blockIdx.x / a.ncg;
  const int cb = cg * 4 + wave, c = cb * 32 + r;
  const int branch = (cb * 32) / a.C;
  const float* const xbase = branch ? a.x1 : a.x0;
  float* const obase = branch ? a.dx1 : a.dx0;
  const unsigned cl = (unsigned)(c - branch * a.C);
  const float mu = a.par[c], is = a.par[a.Ct + c], ga = a.par[2 * a.Ct + c], be = a.par[3 * a.Ct + c];
  const float gis = ga * is, dbn = a.dgb[c] * a.inv_n, dgn = a.dgb[a.Ct + c] * a.inv_n;

  bf16x8 W[NKS][3];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
    for (int p = 0; p < 3; ++p)
      W[ks][p] = *reinterpret_cast<const bf16x8*>(a.wimg + ((int64_t)(cb * NKS + ks) * 3 + p) * 1024 + lane * 16);

  const int64_t rb0 = rg * HB_RBG;
  const int64_t rb1 = rb0 + HB_RBG < a.nrb ? rb0 + HB_RBG : a.nrb;
  // the last k step: which of the lane's two groups of four k exist (the supported K fill every other k step), and where the loads of
  // the missing ones go instead (the row's last four entries, not used)
  const int kl = 16 * (NKS - 1) + 8 * h;
  const bool kok[2] = {kl + 4 <= a.K, kl + 8 <= a.K};
  const unsigned klo[2] = {(unsigned)(kok[0] ? kl : a.K - 4), (unsigned)(kok[1] ? kl + 4 : a.K - 4)};
  // the lane's row of block rb (past n: the block's last row, not stored), its 8 k of every k step. Unconditional loads at clamped
  // offsets from a uniform base
  auto rows_of = [&](int64_t rb) __attribute__((always_inline)) {
    const int64_t rem = a.n - rb * 32;
    return (unsigned)(rem < 32 ? rem : 32);
  };
  auto load_d = [&](int64_t rb, hb_f32x4 (&raw)[NKS][2]) __attribute__((always_inline)) {
    const float* const dq = a.dout + rb * 32 * a.K;
    const unsigned ro = min((unsigned)r, rows_of(rb) - 1u) * (unsigned)a.K;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const unsigned ko = ks == NKS - 1 ? klo[q] : (unsigned)(16 * ks + 8 * h + 4 * q);
        raw[ks][q] = *reinterpret_cast<const hb_f32x4*>(dq + (ro + ko));
      }
  };

  hb_f32x4 raw[NKS][2];
  if (rb0 < rb1) load_d(rb0, raw);
  for (int64_t rb = rb0; rb < rb1; ++rb) {
    // accumulator register i: row 32 rb + (i & 3) + 8 (i >> 2) + 4 h, channel = the lane's
    const unsigned rows = rows_of(rb);
    const float* const xq = xbase + rb * 32 * a.C;
    float* const oq = obase + rb * 32 * a.C;
    float xv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) xv[i] = xq[min((unsigned)(4 * h + (i & 3) + 8 * (i >> 2)), rows - 1u) * (unsigned)a.C + cl];
    hb_f32x4 rawn[NKS][2];
    load_d(rb + 1 < rb1 ? rb + 1 : rb, rawn);

    hb_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    bf16x8 D0[NKS];
    hb_static_for<NKS>([&](auto kc) __attribute__((always_inline)) {
      constexpr int ks = decltype(kc)::value;
      HbSplit8 sp;
      hb_static_for<8>([&](auto ec) __attribute__((always_inline)) {
        constexpr int e = decltype(ec)::value;
        if constexpr (ks == NKS - 1) sp.put<e>(kok[e >> 2] ? raw[ks][e >> 2][e & 3] : 0.f);
        else sp.put<e>(raw[ks][e >> 2][e & 3]);
      });
      bf16x8 D[3];
      sp.get(D);
      D0[ks] = D[0];
      hb_static_for<5>([&](auto pc) __attribute__((always_inline)) {
        constexpr int p = decltype(pc)::value;
        acc = hb_mfma(D[hb_pass_a(p)], W[ks][hb_pass_b(p)], acc);
      });
    });
    hb_static_for<NKS>([&](auto kc) __attribute__((always_inline)) {
      constexpr int ks = decltype(kc)::value;
      acc = hb_mfma(D0[ks], W[ks][0], acc);
    });

    auto value = [&](int i) __attribute__((always_inline)) {
      const float xh = (xv[i] - mu) * is;
      const float z = ga * xh + be;
      const float d = z > 0.f ? acc[i] : 0.f;
      return gis * (d - dbn - xh * dgn);
    };
    if (rows == 32) {
#pragma unroll
      for (int i = 0; i < 16; ++i) oq[(unsigned)(4 * h + (i & 3) + 8 * (i >> 2)) * (unsigned)a.C + cl] = value(i);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const unsigned ri = (unsigned)(4 * h + (i & 3) + 8 * (i >> 2));
        if (ri < rows) oq[ri * (unsigned)a.C + cl] = value(i);
      }
    }
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      raw[ks][0] = rawn[ks][0];
      raw[ks][1] = rawn[ks][1];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Forward of the same region without the map: out[r][k] = sum_c relu(gamma_c ((x[r][c] - mean_c) invstd_c) + beta_c) W[k][c] + b[k].
// The structure of rows_gemm4_kernel's forward: computed transposed, D[k][row], so a lane ends with 4 consecutive outputs of ITS row
// (16-byte stores); lane (r, h) loads 64 contiguous bytes of its row per 32 channels and uses them for two MFMA k steps (k step 2 c + u
// holds channel 32 c + 16 h + 8 u + j for lane half h, element j); the activation is bn_apply_kernel's expression in its order on the
// loaded values (a NaN stays a NaN where that kernel's comparison writes 0: a bad row shows in the head's outputs), the per-channel
// constants of the 32 channels come from an LDS copy of par; the weight fragments are 16-byte loads from the lane-order image
// [K block][k step Ct / 16][piece 3][lane 64][8 bf16] (lane (r, h), element j: W[32 kb + r][channel], zero past K) straight from L2.
// Persistent workgroups of 4 waves, one per SIMD, wave tile 64 rows x all K; one loop over (tile, 32 channels) that requests the next
// step's rows and fragments ahead of this step's MFMAs. Two accumulator sets (the leading pass | the five small ones) added in the
// epilogue with the bias. No atomics, fixed order.
constexpr int HF_TILE = 256;              // rows per workgroup tile

struct HfArgs {
  const float* x0;
  const float* x1;
  const float* par;           // (4, Ct)
  const unsigned char* wimg;
  const float* bias;          // (K)
  float* out;                 // (n, K)
  int64_t n, tiles;
  int C, Ct, K;
};

__global__ __launch_bounds__(256) void head_bn_forward_weights_kernel(const float* __restrict__ w, unsigned char* __restrict__ img, int K,
                                                                      int Ct, int NKB) {
  const int KS = Ct >> 4;
  const int id = blockIdx.x * 256 + threadIdx.x;         // (kb, k step, lane)
  if (id >= NKB * KS * 64) return;
  const int lane = id & 63, r = lane & 31, h = lane >> 5;
  const int ks = (id >> 6) % KS, kb = (id >> 6) / KS;
  const int k = 32 * kb + r, c0 = (ks >> 1) * 32 + h * 16 + (ks & 1) * 8;
  u32x4 q[3];
  unsigned lo[3] = {0, 0, 0};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = k < K ? w[(int64_t)k * Ct + c0 + j] : 0.f;
    unsigned p[3];
    split3(v, p[0], p[1], p[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (j & 1) q[i][j >> 1] = lo[i] | (p[i] << 16);
      else lo[i] = p[i];
    }
  }
  unsigned char* dst = img + ((int64_t)(kb * KS + ks) * 3) * 1024 + lane * 16;
#pragma unroll
  for (int i = 0; i < 3; ++i) *reinterpret_cast<u32x4*>(dst + i * 1024) = q[i];
}

template <int NKB>
__global__ __launch_bounds__(HB_NT, 1) void head_bn_forward_kernel(HfArgs a) {
  __shared__ __attribute__((aligned(16))) float cst[4 * 512];      // par: mean | invstd | gamma | beta, (4, Ct)
  asm volatile("" ::: HB_ACC_0_127, HB_ACC_128_255);
  for (int i = threadIdx.x; i < 4 * a.Ct; i += HB_NT) cst[i] = a.par[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int KC = a.Ct >> 5, KS = a.Ct >> 4;
  int64_t lt = blockIdx.x;
  int lc = 0;
  if (lt >= a.tiles) return;
  const unsigned char* const wl = a.wimg + lane * 16;

  int64_t xoff[2];            // the lane's rows of the tile the loads belong to (rows past n: the last row), as element offsets
  auto set_rows = [&](int64_t tile) __attribute__((always_inline)) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const int64_t m = tile * HF_TILE + wave * 64 + rb * 32 + r;
      xoff[rb] = (m < a.n ? m : a.n - 1) * a.C;
    }
  };
  // the lane's 64 bytes of 32 channels as two halves: `hi` = 0 the 8 values of k step 2 c, 1 those of k step 2 c + 1
  auto load_a = [&](int c, int hi, hb_f32x4 (&dst)[2][2]) __attribute__((always_inline)) {
    const int branch = (32 * c) / a.C;
    const float* const xb = (branch ? a.x1 : a.x0) + (32 * c - branch * a.C + 16 * h + 8 * hi);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 2; ++q) dst[rb][q] = *reinterpret_cast<const hb_f32x4*>(xb + xoff[rb] + 4 * q);
  };
  auto load_b = [&](int ks, bf16x8 (&dst)[NKB][3]) __attribute__((always_inline)) {
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int p = 0; p < 3; ++p) dst[kb][p] = *reinterpret_cast<const bf16x8*>(wl + ((size_t)(kb * KS + ks) * 3 + p) * 1024);
  };
  // the constants of the 8 channels 32 c + 16 h + 8 u + (0 .. 7): [q][mean | invstd | gamma | beta]
  auto load_c = [&](int c, int u, hb_f32x4 (&dst)[2][4]) __attribute__((always_inline)) {
    const float* const cp = cst + 32 * c + 16 * h + 8 * u;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int p = 0; p < 4; ++p) dst[q][p] = *reinterpret_cast<const hb_f32x4*>(cp + p * a.Ct + 4 * q);
  };
  // value e of 8: bn_apply_kernel's expression in its order, four values at a time (a NaN stays a NaN), then its three pieces
  hb_f32x4 act;
  auto value = [&](auto ec, HbSplit8& sp, const hb_f32x4 (&v)[2], const hb_f32x4 (&cs)[2][4]) __attribute__((always_inline)) {
    constexpr int e = decltype(ec)::value, q = e >> 2;
    if constexpr ((e & 3) == 0) act = cs[q][2] * ((v[q] - cs[q][0]) * cs[q][1]) + cs[q][3];
    sp.put<e>(act[e & 3] <= 0.f ? 0.f : act[e & 3]);
  };
  // D[k][row] += W fragment (first operand, K block kb) . activation fragment (second operand, row block rb): the pass of the two leading
  // pieces into accumulator block rb NKB + kb, the five passes below 2^-8 of it into block 2 NKB + rb NKB + kb (rows_gemm4.hip)
  auto step = [&](const bf16x8 (&Bw)[NKB][3], const bf16x8 (&Xf)[2][3], auto&& gap) __attribute__((always_inline)) {
    hb_static_for<12 * NKB>([&](auto kc) __attribute__((always_inline)) {
      constexpr int k = decltype(kc)::value, rb = k / (6 * NKB), kb = (k / 6) % NKB, pass = k % 6;
      hb_mfma_acc<(pass == 5 ? 0 : 2 * NKB) + rb * NKB + kb>(Bw[kb][hb_pass_a(pass)], Xf[rb][hb_pass_b(pass)]);
      gap(kc);
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  hb_static_for<64 * NKB>([](auto rc) { hb_acc_zero<decltype(rc)::value>(); });
  hb_f32x4 Ahi[2][2], CS1[2][4];
  bf16x8 XF0[2][3], B0[NKB][3];
  set_rows(lt);
  {
    hb_f32x4 A0[2][2], CS0[2][4];
    load_a(0, 0, A0);
    load_a(0, 1, Ahi);
    load_b(0, B0);
    load_c(0, 0, CS0);
    load_c(0, 1, CS1);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      HbSplit8 sp;
      hb_static_for<8>([&](auto ec) __attribute__((always_inline)) { value(ec, sp, A0[rb], CS0); });
      sp.get(XF0[rb]);
    }
  }
  asm volatile("s_nop 4" ::: "memory");

  for (;;) {
    int64_t nt = lt;
    int nc = lc + 1;
    if (nc == KC) { nc = 0; nt = lt + gridDim.x; }
    const bool more = nt < a.tiles;
    if (!more) { nt = lt; nc = lc; }            // (the last step of the loop requests its own operands again; nobody uses them)
    bf16x8 B1[NKB][3];
    load_b(2 * lc + 1, B1);
    if (nt != lt) set_rows(nt);
    hb_f32x4 An[2][2], CS0n[2][4];
    load_a(nc, 0, An);
    load_c(nc, 0, CS0n);
    __builtin_amdgcn_sched_barrier(0);

    // k step 0 of these 32 channels; in its gaps the activation and split of k step 1
    bf16x8 XF1[2][3];
    HbSplit8 sp;
    step(B0, XF0, [&](auto kc) __attribute__((always_inline)) {
      constexpr int k = decltype(kc)::value;
      if constexpr (k < 16) {
        constexpr int rb = k >> 3, e = k & 7;
        value(std::integral_constant<int, e>{}, sp, Ahi[rb], CS1);
        if constexpr (e == 7) sp.get(XF1[rb]);
      }
    });
    load_b(2 * nc, B0);
    load_a(nc, 1, Ahi);       // (the other half of the 64 bytes whose first half is already requested)
    load_c(nc, 1, CS1);
    __builtin_amdgcn_sched_barrier(0);
    // k step 1; in its gaps the activation and split of k step 0 of the next 32 channels
    bf16x8 XF0n[2][3];
    step(B1, XF1, [&](auto kc) __attribute__((always_inline)) {
      constexpr int k = decltype(kc)::value;
      if constexpr (k >= 8 && k < 24) {
        constexpr int rb = (k - 8) >> 3, e = (k - 8) & 7;
        value(std::integral_constant<int, e>{}, sp, An[rb], CS0n);
        if constexpr (e == 7) sp.get(XF0n[rb]);
      }
    });

    if (lc == KC - 1) {
      // ---- the tile is complete: accumulator register 4 j + e of block (rb, kb) = row 32 rb + r, output 32 kb + 8 j + 4 h + e
      hb_acc_settle();
      hb_static_for<2>([&](auto rbc) __attribute__((always_inline)) {
        constexpr int rb = decltype(rbc)::value;
        const int64_t m = lt * HF_TILE + wave * 64 + rb * 32 + r;
        const bool ok = m < a.n;
        float* const out = a.out + (ok ? m : a.n - 1) * a.K + 4 * h;
        hb_static_for<4 * NKB>([&](auto qc) __attribute__((always_inline)) {
          constexpr int kb = decltype(qc)::value >> 2, j = decltype(qc)::value & 3;
          constexpr int R0 = (rb * NKB + kb) * 16 + 4 * j, R1 = R0 + 2 * NKB * 16;
          const int k0 = 32 * kb + 8 * j + 4 * h;
          const hb_f32x4 v = (hb_f32x4){hb_acc_read<R0>() + hb_acc_read<R1>(), hb_acc_read<R0 + 1>() + hb_acc_read<R1 + 1>(),
                                        hb_acc_read<R0 + 2>() + hb_acc_read<R1 + 2>(), hb_acc_read<R0 + 3>() + hb_acc_read<R1 + 3>()};
          if (k0 < a.K) {                                   // K is a multiple of 4: a quad is inside or outside
            const hb_f32x4 b = (hb_f32x4){a.bias[k0], a.bias[k0 + 1], a.bias[k0 + 2], a.bias[k0 + 3]};
            if (ok) *reinterpret_cast<hb_f32x4*>(out + 32 * kb + 8 * j) = v + b;
          }
        });
      });
      hb_static_for<64 * NKB>([](auto rc) { hb_acc_zero<decltype(rc)::value>(); });
      asm volatile("s_nop 4" ::: "memory");
    }
    if (!more) break;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int p = 0; p < 3; ++p) XF0[rb][p] = XF0n[rb][p];
    lt = nt;
    lc = nc;
  }
}

__host__ int hb_cu_count() {
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

// ranges so that the workgroups fill the CUs once at two workgroups per CU
__host__ int hb_ranges(int ncg) {
  const int r = 2 * hb_cu_count() / ncg;
  return r < 8 ? 8 : r;
}

__host__ int64_t hb_part_bytes(int nranges, int K, int Ct) { return crb_align_up((int64_t)nranges * 2 * K * Ct * 4, 256); }

}  // namespace

extern "C" int crb_head_bn_supported(int nbranch, int width, int K) {
  return (nbranch == 2 && (width == 128 || width == 256) && (K == 60 || K == 72)) ? 1 : 0;
}

extern "C" int64_t crb_head_bn_workspace_bytes(int nbranch, int width, int K) {
  if (!crb_head_bn_supported(nbranch, width, K)) return 0;
  const int Ct = nbranch * width, nranges = hb_ranges(Ct / 128);
  return hb_part_bytes(nranges, K, Ct) + (int64_t)nranges * 2 * HB_COLP * 8;
}

extern "C" int64_t crb_head_bn_sums_count(int nbranch, int width, int K) {
  if (!crb_head_bn_supported(nbranch, width, K)) return 0;
  return (int64_t)2 * K * nbranch * width + K;
}

extern "C" int crb_head_bn_sums(const float* x0, const float* x1, const float* par, const float* dout, int64_t n, int nbranch, int width,
                                int K, double* sums, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!crb_head_bn_supported(nbranch, width, K)) return CRB_ERR_UNSUPPORTED;
  if (n <= 0 || n >= (1LL << 34) || !x0 || !x1 || !par || !dout || !sums) return CRB_ERR_ARG;
  if (!workspace || workspace_bytes < crb_head_bn_workspace_bytes(nbranch, width, K)) return CRB_ERR_WORKSPACE;
  HsArgs a;
  a.x0 = x0; a.x1 = x1; a.par = par; a.dout = dout;
  a.n = n; a.C = width; a.Ct = nbranch * width; a.K = K; a.ncg = a.Ct / 128;
  a.nchunks = (int)((n + 15) / 16);
  a.nranges = hb_ranges(a.ncg);
  a.part = (float*)workspace;
  a.colpart = (double*)((char*)workspace + hb_part_bytes(a.nranges, K, a.Ct));
  const dim3 grid((unsigned)(a.nranges * a.ncg));
  if (K > 64) hipLaunchKernelGGL(head_bn_sums_kernel<3>, grid, dim3(HB_NT), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(head_bn_sums_kernel<2>, grid, dim3(HB_NT), 0, (hipStream_t)stream, a);
  CRB_CHECK_LAUNCH();
  const int64_t total = (int64_t)2 * K * a.Ct + K;
  hipLaunchKernelGGL(head_bn_reduce_kernel, dim3((unsigned)crb_cdiv(total, 32)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)a.part, (const double*)a.colpart, a.nranges, K, a.Ct, sums);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_head_bn_finalize(const double* sums, const float* w, const float* par, int nbranch, int width, int K, float* dgb,
                                    float* dw, float* dbias, void* stream) {
  if (!crb_head_bn_supported(nbranch, width, K)) return CRB_ERR_UNSUPPORTED;
  if (!sums || !w || !par || !dgb || !dw) return CRB_ERR_ARG;
  const int Ct = nbranch * width;
  hipLaunchKernelGGL(head_bn_finalize_kernel, dim3((unsigned)(Ct / 32)), dim3(256), 0, (hipStream_t)stream, sums, w, par, K, Ct, dgb, dw,
                     dbias);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int64_t crb_head_bn_weights_bytes(int nbranch, int width, int K) {
  if (!crb_head_bn_supported(nbranch, width, K)) return 0;
  return (int64_t)(nbranch * width / 32) * ((K + 15) / 16) * 3 * 1024;
}

extern "C" int crb_head_bn_weights(const float* w, void* image, int nbranch, int width, int K, void* stream) {
  if (!crb_head_bn_supported(nbranch, width, K)) return CRB_ERR_UNSUPPORTED;
  if (!w || !image) return CRB_ERR_ARG;
  const int Ct = nbranch * width, NKS = (K + 15) / 16;
  const int threads = (Ct / 32) * NKS * 64;
  hipLaunchKernelGGL(head_bn_weights_kernel, dim3((unsigned)crb_cdiv(threads, 256)), dim3(256), 0, (hipStream_t)stream, w,
                     (unsigned char*)image, K, Ct, NKS);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_head_bn_apply(const float* x0, const float* x1, const float* par, const float* dgb, const float* dout,
                                 const void* image, int64_t n, int nbranch, int width, int K, float* dx0, float* dx1, void* stream) {
  if (!crb_head_bn_supported(nbranch, width, K)) return CRB_ERR_UNSUPPORTED;
  if (n <= 0 || n >= (1LL << 34) || !x0 || !x1 || !par || !dgb || !dout || !image || !dx0 || !dx1) return CRB_ERR_ARG;
  HaArgs a;
  a.x0 = x0; a.x1 = x1; a.dx0 = dx0; a.dx1 = dx1; a.par = par; a.dgb = dgb; a.dout = dout; a.wimg = (const unsigned char*)image;
  a.n = n; a.nrb = (n + 31) / 32;
  a.C = width; a.Ct = nbranch * width; a.K = K; a.ncg = a.Ct / 128;
  a.inv_n = 1.0f / (float)n;
  const int64_t groups = (a.nrb + HB_RBG - 1) / HB_RBG;
  if (groups * a.ncg >= (1LL << 31)) return CRB_ERR_ARG;
  const dim3 grid((unsigned)(groups * a.ncg));
  if (K > 64) hipLaunchKernelGGL(head_bn_apply_kernel<5>, grid, dim3(HB_NT), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(head_bn_apply_kernel<4>, grid, dim3(HB_NT), 0, (hipStream_t)stream, a);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int64_t crb_bn_head_forward_weights_bytes(int nbranch, int width, int K) {
  if (!crb_head_bn_supported(nbranch, width, K)) return 0;
  return (int64_t)((K + 31) / 32) * (nbranch * width / 16) * 3 * 1024;
}

extern "C" int crb_bn_head_forward_weights(const float* w, void* image, int nbranch, int width, int K, void* stream) {
  if (!crb_head_bn_supported(nbranch, width, K)) return CRB_ERR_UNSUPPORTED;
  if (!w || !image) return CRB_ERR_ARG;
  const int Ct = nbranch * width, NKB = (K + 31) / 32;
  const int threads = NKB * (Ct / 16) * 64;
  hipLaunchKernelGGL(head_bn_forward_weights_kernel, dim3((unsigned)crb_cdiv(threads, 256)), dim3(256), 0, (hipStream_t)stream, w,
                     (unsigned char*)image, K, Ct, NKB);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_bn_head_forward(const float* x0, const float* x1, const float* par, const void* image, const float* bias, int64_t n,
                                   int nbranch, int width, int K, float* out, void* stream) {
  if (!crb_head_bn_supported(nbranch, width, K)) return CRB_ERR_UNSUPPORTED;
  if (n <= 0 || n >= (1LL << 34) || !x0 || !x1 || !par || !image || !bias || !out) return CRB_ERR_ARG;
  HfArgs a;
  a.x0 = x0; a.x1 = x1; a.par = par; a.wimg = (const unsigned char*)image; a.bias = bias; a.out = out;
  a.n = n; a.tiles = (n + HF_TILE - 1) / HF_TILE;
  a.C = width; a.Ct = nbranch * width; a.K = K;
  const int cus = hb_cu_count();
  const dim3 grid((unsigned)(a.tiles < cus ? a.tiles : cus));
  if (K > 64) hipLaunchKernelGGL(head_bn_forward_kernel<3>, grid, dim3(HB_NT), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(head_bn_forward_kernel<2>, grid, dim3(HB_NT), 0, (hipStream_t)stream, a);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
