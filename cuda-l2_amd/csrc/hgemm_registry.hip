// Kernel registry (config id -> launch thunk) and the two helper kernels' launchers.
#include "hgemm_launch.hpp"
#include "hgemm_kernel_rg.hpp"
#include "hgemm_kernel_ta.hpp"
#include "hgemm_kernel_tn.hpp"

#include <algorithm>
#include <cstdio>

namespace hgemm_mi355x {

#define HGEMM_THUNK(G, FN, ...) extern template void FN<__VA_ARGS__>(const GemmArgs&, int, hipStream_t, int, TimingSlot);
#include "hgemm_thunks.inc"

// The table holds host function pointers: keep it out of the device pass.
#if !defined(__HIP_DEVICE_COMPILE__)
thread_local LaunchTiming t_launch_timing;
// stream-K workgroups of a classic geometry one CU holds: LDS, 8 waves per SIMD, and the accumulator + fragment registers of a
// wave (512 per SIMD lane); at most 4 (more persistent workgroups only mean more slabs)
constexpr int sk_residency(int lds_bytes, int nw, int acc_regs) {
  const int by_lds = 160 * 1024 / lds_bytes, by_waves = 32 / nw, by_regs = 512 / (acc_regs + 64) * 4 / nw;
  const int r = by_lds < by_waves ? (by_lds < by_regs ? by_lds : by_regs) : (by_waves < by_regs ? by_waves : by_regs);
  return acc_regs * 64 * nw > 256 * 128 ? 0 : r < 1 ? 1 : r > 4 ? 4 : r;   // (no stream-K kernel beyond 256 x 128: hgemm_launch.hpp)
}
// "w<BM>x<BN>[_k4]" with the workgroup tile computed from the template arguments (static storage per instantiation)
template <int BM, int BN, int KW>
const char* wd_name() {
  static char buf[24];
  if (!buf[0]) snprintf(buf, sizeof buf, "w%dx%d%s", BM, BN, KW == 4 ? "_k4" : "");
  return buf;
}

// One row builder per family, C = the member's config type.  Fields in KernelEntry's order: name, family, tile, wave grid, MI, ring
// depth, threads, LDS bytes, thunk, persistent workgroups, single-launch split-K, K granularity, K-tail rule, stream-K residency,
// explicit plans only.
template <class C>
constexpr KernelEntry row_t(const char* name) {
  return {name, Family::T, C::BM, C::BN, C::WM, C::WN, C::MI, C::NBUF, C::THREADS, C::LDS_BYTES, &launch_cfg<C>, 0, true, 64, KTail::PADDED,
          sk_residency(C::LDS_BYTES + 64, C::NW, C::BM * C::BN / (64 * C::NW)), false};
}
template <class C>
constexpr KernelEntry row_s(const char* name) {
  return {name, Family::S, C::BM, C::BN, C::WM, C::WN, C::MI, 2, C::THREADS, C::LDS_BYTES + 64, &launch_sp<C>,
          256 * (160 * 1024 / (C::LDS_BYTES + 64)), true, 64, KTail::NONE, 0, C::MI == 32};
}
template <class C>
constexpr KernelEntry row_q(const char* name) {
  return {name, Family::Q, C::BM, C::BN, C::WM, C::WN, C::MI, 2, C::THREADS, C::LDS_BYTES + (C::WGS == 2 ? 0 : 64), &launch_sq<C>,
          256 * C::WGS, true, 64 * C::KT, C::MI == 16 ? KTail::DIRECT : KTail::NONE, 0, C::MI == 32};
}
template <class C>
constexpr KernelEntry row_r(const char* name) {
  return {name, Family::R, C::BM, C::BN, 2, 2, 16, C::LB, C::THREADS, C::LDS_BYTES, &launch_rs<C>, 0, true, C::BKS, KTail::DIRECT,
          C::WGS_PER_CU, false};
}
// family "w": named by its WORKGROUP tile; "_k4" = the four waves split the K walk of one wave tile.  (K granularity 64: a
// split-K chunk is then a whole number of K = 32 slices whatever the split count.)
template <class C>
KernelEntry row_w() {
  return {wd_name<C::BM, C::BN, C::KW>(), Family::W, C::BM, C::BN, C::WM, C::WN, 16, 1, C::THREADS, C::LDS_BYTES, &launch_wd<C>, 0, true, 64,
          KTail::NONE, 0, false};
}
// family "u" (hgemm_kernel_lu.hpp), behind every other family so that their ids stay put: WM x WN is the wave grid of ONE of the
// four K-groups ("_k4": threads = WM * WN * 4 * 64); no single-launch split-K, no K tail, no stream-K; K granularity = the stage
template <class C>
constexpr KernelEntry row_u(const char* name) {
  return {name, Family::U, C::BM, C::BN, C::WM, C::WN, 16, C::NBUF, C::THREADS, C::LDS_BYTES, &launch_lu<C>, 0, false, C::STAGE_K, KTail::NONE,
          0, true};
}

// names are the persisted keys of plans (tuned tables, shape files): literals built from the entry's arguments
#define HGEMM_STR2(x) #x
#define HGEMM_STR(x) HGEMM_STR2(x)
#define HGEMM_TILE_NAME(F, BM, BN, WM, WN) F HGEMM_STR(BM) "x" HGEMM_STR(BN) "_w" HGEMM_STR(WM) "x" HGEMM_STR(WN)
// MI = 16 members keep their round-1 names (tuned tables refer to plans by name); MI = 32 members add "_m32"
#define HGEMM_SP_SUFFIX_16 ""
#define HGEMM_SP_SUFFIX_32 "_m32"
#define HGEMM_SQ_SUFFIX_1_16 ""
#define HGEMM_SQ_SUFFIX_2_16 "_k128"
#define HGEMM_SQ_SUFFIX_1_32 "_m32"
#define HGEMM_RS_SUFFIX_1 ""
#define HGEMM_RS_SUFFIX_2 "_d"

// Config ids are positions in this table: every t row, then the s and q rows in list order, then r, w and u
const KernelEntry g_kernel_table[] = {
#define HGEMM_CFG(G, BM, BN, WM, WN, MI, NB) \
  row_t<Cfg<BM, BN, WM, WN, MI, NB>>(HGEMM_TILE_NAME("t", BM, BN, WM, WN) "_m" HGEMM_STR(MI) "_s" HGEMM_STR(NB)),
#include "hgemm_configs.def"
#define HGEMM_SP(G, BM, BN, WM, WN, MI) row_s<CfgSP<BM, BN, WM, WN, MI>>(HGEMM_TILE_NAME("s", BM, BN, WM, WN) HGEMM_SP_SUFFIX_##MI),
#define HGEMM_SQ(G, BM, BN, WM, WN, KT, MI) \
  row_q<CfgSQ<BM, BN, WM, WN, KT, MI>>(HGEMM_TILE_NAME("q", BM, BN, WM, WN) HGEMM_SQ_SUFFIX_##KT##_##MI),
#include "hgemm_configs.def"
#define HGEMM_RS(G, BM, BN, BKS, LB) \
  row_r<CfgRS<BM, BN, BKS, LB>>("r" HGEMM_STR(BM) "x" HGEMM_STR(BN) "_k" HGEMM_STR(BKS) HGEMM_RS_SUFFIX_##LB),
#include "hgemm_configs.def"
#define HGEMM_WD(G, FM, FN, KW) row_w<CfgWD<FM, FN, KW>>(),
#include "hgemm_configs.def"
#define HGEMM_LU(BM, BN, WM, WN, NIMG, NB) row_u<CfgLU<BM, BN, WM, WN, NIMG, NB>>(HGEMM_TILE_NAME("u", BM, BN, WM, WN) "_k4"),
#include "hgemm_configs_lu.def"
};
const int g_num_kernels = (int)(sizeof(g_kernel_table) / sizeof(g_kernel_table[0]));
#endif  // !__HIP_DEVICE_COMPILE__

// Split-K combine: C[m][n] = T( sum_s partial[s][m][n] ), fp32 adds in split order, the sum rounded to T once -- fp16 (the b_col_major
// families and the fp16 calls of the transposed-read layouts) or bf16 (bgemm_mi355x_nn / _ta: round to nearest even).  Slabs are fp32
// whatever the operands were.
// (deterministic, unlike the reference's atomicAdd split-K, a100_F32F16F16F32/64_256_16384.cu:149-152).
template <class T>
__global__ void __launch_bounds__(256) hgemm_splitk_reduce_kernel(const float* __restrict__ partial,
                                                                  T* __restrict__ C, int M, int N,
                                                                  int ldc, int splits) {
  using Tx4 = __attribute__((ext_vector_type(4))) T;
  const size_t total4 = ((size_t)M * N) >> 2;  // N % 4 == 0 on this path
  const size_t slab   = (size_t)M * N;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total4;
       q += (size_t)gridDim.x * blockDim.x) {
    const size_t e = q << 2;
    f32x4 s = *(const f32x4*)(partial + e);
    int k = 1;
    // eight slabs' loads in flight per thread, added in split order: with tiny M*N this kernel is a
    // chain of dependent-looking global loads (measured: 64 splits cost +12 us before the unroll)
    for (; k + 8 <= splits; k += 8) {
      f32x4 p[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) p[u] = *(const f32x4*)(partial + (size_t)(k + u) * slab + e);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += p[u];
    }
    for (; k < splits; ++k) {
      const f32x4 p = *(const f32x4*)(partial + (size_t)k * slab + e);
      s += p;
    }
    const int m = (int)(e / N), n = (int)(e % N);
    Tx4 o = {(T)s[0], (T)s[1], (T)s[2], (T)s[3]};
    *(Tx4*)(C + (size_t)m * ldc + n) = o;
  }
}

// The combine of the fp32-C calls (hgemm_mi355x_ta_c32, bgemm_mi355x_ta_c32): t = p[0] + p[1] + ... + p[S-1] in split order, then
// C32 = accumulate ? C32 + t : t -- the shape of the unsplit result, old + fl(sum), and one fixed order per plan.  C32 is read only
// with `accumulate`; rows are ldc fp32 elements apart and the pad between N and ldc is never touched.  (N % 4 == 0, ldc % 4 == 0 and
// a 16-byte aligned C32 on this path.)
__global__ void __launch_bounds__(256) hgemm_splitk_reduce_c32_kernel(const float* __restrict__ partial, float* __restrict__ C32, int M,
                                                                      int N, int ldc, int splits, int accumulate) {
  const size_t total4 = ((size_t)M * N) >> 2;
  const size_t slab   = (size_t)M * N;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total4; q += (size_t)gridDim.x * blockDim.x) {
    const size_t e = q << 2;
    const int m = (int)(e / N), n = (int)(e % N);
    f32x4* out = (f32x4*)(C32 + (size_t)m * ldc + n);
    f32x4 old = {0.f, 0.f, 0.f, 0.f};
    if (accumulate) old = *out;   // in flight with the slab loads
    f32x4 s = *(const f32x4*)(partial + e);
    int k = 1;
    for (; k + 8 <= splits; k += 8) {   // eight slabs' loads in flight per thread, added in split order (hgemm_splitk_reduce_kernel)
      f32x4 p[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) p[u] = *(const f32x4*)(partial + (size_t)(k + u) * slab + e);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += p[u];
    }
    for (; k < splits; ++k) {
      const f32x4 p = *(const f32x4*)(partial + (size_t)k * slab + e);
      s += p;
    }
    *out = accumulate ? old + s : s;
  }
}

// Combine of the hybrid schedule's tail pass: C tile t = fp16( sum_s partial[s * tail_tiles + t][BM][BN] ),
// slices added in K order.  One workgroup per (tail tile, 16-row band); the tile origin comes from the same
// raster map the GEMM kernel used.
__global__ void __launch_bounds__(256) hgemm_tail_reduce_kernel(const GemmArgs g, int BM, int BN) {
  const int bands = BM / 16;
  const int t = blockIdx.x / bands, band = blockIdx.x % bands;
  const TileCoord tc = map_logical(g, t, BM, BN);  // slice 0 of tail tile t: gives (m0, n0)
  const size_t slab = (size_t)BM * BN, stride = slab * g.tail_tiles;
  const float* base = g.partial + (size_t)t * slab;
  const int quads_per_row = BN / 4;
  for (int q = threadIdx.x; q < 16 * quads_per_row; q += blockDim.x) {
    const int r = band * 16 + q / quads_per_row, c = (q % quads_per_row) * 4;
    const int m = tc.m0 + r, n = tc.n0 + c;
    if (m >= g.M || n >= g.N) continue;
    const float* p = base + (size_t)r * BN + c;
    f32x4 s = *(const f32x4*)p;
    for (int k = 1; k < g.splits; ++k) s += *(const f32x4*)(p + (size_t)k * stride);
    f16x4 o = {(f16)s[0], (f16)s[1], (f16)s[2], (f16)s[3]};
    *(f16x4*)(g.C + (size_t)m * g.ldc + n) = o;
  }
}

// Any-shape / any-alignment fallback (one output per thread, an fmaf chain in k order, fp32 accumulate, rounded to T once).
// Correctness net for shapes the MFMA paths do not accept (K % 8 != 0, unaligned views); never tuned.  The reference kernel of every
// 16-bit call: <f16, false> the b_col_major families' and the NN layout's, A_COL the TA layout's (hgemm_kernel_ta.hpp: A given as
// a_col_major, read as A[k * lda + m] -- same sum order, so the same bits on the transposed operand), T = __bf16 the bgemm_ calls'.
template <class T, bool A_COL>
__global__ void __launch_bounds__(256) hgemm_generic_kernel(const T* __restrict__ A,
                                                            const T* __restrict__ B,
                                                            T* __restrict__ C, int M, int N, int K,
                                                            int lda, int ldb_rowmajor, int ldc) {
  const int n = blockIdx.x * 64 + (threadIdx.x & 63);
  if (n >= N) return;
  // grid-stride over M: gridDim.y is capped at 65535 (M > 262140 used to fail the launch)
  for (int m = blockIdx.y * 4 + (threadIdx.x >> 6); m < M; m += gridDim.y * 4) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = fmaf((float)A[A_COL ? (size_t)k * lda + m : (size_t)m * lda + k], (float)B[(size_t)k * ldb_rowmajor + n], s);
    C[(size_t)m * ldc + n] = (T)s;
  }
}

// The reference kernel of the TN layout (bgemm_mi355x_tn, hgemm_kernel_tn.hpp): B given as b_col_major, read as B[n * ldb + k] -- the same
// one output per thread, the same fma chain in k order and the one rounding to T.  A kernel of its own: hgemm_generic_kernel keeps its
// template arguments, and with them the symbols of its instances.
template <class T>
__global__ void __launch_bounds__(256) hgemm_generic_tn_kernel(const T* __restrict__ A, const T* __restrict__ Bcol, T* __restrict__ C, int M,
                                                               int N, int K, int lda, int ldb_colmajor, int ldc) {
  const int n = blockIdx.x * 64 + (threadIdx.x & 63);
  if (n >= N) return;
  for (int m = blockIdx.y * 4 + (threadIdx.x >> 6); m < M; m += gridDim.y * 4) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = fmaf((float)A[(size_t)m * lda + k], (float)Bcol[(size_t)n * ldb_colmajor + k], s);
    C[(size_t)m * ldc + n] = (T)s;
  }
}

// The reference kernel of the fp32-C calls: the same fma chain in k order, then C32 = accumulate ? C32 + s : s (no rounding).
template <class T, bool A_COL>
__global__ void __launch_bounds__(256) hgemm_generic_c32_kernel(const T* __restrict__ A, const T* __restrict__ B,
                                                                float* __restrict__ C32, int M, int N, int K, int lda,
                                                                int ldb_rowmajor, int ldc, int accumulate) {
  const int n = blockIdx.x * 64 + (threadIdx.x & 63);
  if (n >= N) return;
  for (int m = blockIdx.y * 4 + (threadIdx.x >> 6); m < M; m += gridDim.y * 4) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = fmaf((float)A[A_COL ? (size_t)k * lda + m : (size_t)m * lda + k], (float)B[(size_t)k * ldb_rowmajor + n], s);
    float* out = C32 + (size_t)m * ldc + n;
    *out = accumulate ? *out + s : s;
  }
}

// The combine of the fused-bias calls (bgemm_mi355x_tn_bias): s = p[0] + p[1] + ... + p[S-1] in split order, as hgemm_splitk_reduce_kernel
// adds them, THEN s + float(bias[n]) as one fp32 add, then the one rounding to bf16 (nearest even).  The bias is not added into a slab.
// A kernel of its own: hgemm_splitk_reduce_kernel keeps its symbols and streams.  (N % 8 == 0 and a 16-byte aligned bias on this path, so
// the four bias values of a quad are one aligned 8-byte load inside the vector.)
__global__ void __launch_bounds__(256) hgemm_splitk_reduce_bias_kernel(const float* __restrict__ partial, __bf16* __restrict__ C,
                                                                       const __bf16* __restrict__ bias, int M, int N, int ldc, int splits) {
  using bx4 = __attribute__((ext_vector_type(4))) __bf16;
  const size_t total4 = ((size_t)M * N) >> 2;
  const size_t slab   = (size_t)M * N;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total4; q += (size_t)gridDim.x * blockDim.x) {
    const size_t e = q << 2;
    const int m = (int)(e / N), n = (int)(e % N);
    const bx4 b = *(const bx4*)(bias + n);   // in flight with the slab loads
    f32x4 s = *(const f32x4*)(partial + e);
    int k = 1;
    for (; k + 8 <= splits; k += 8) {   // eight slabs' loads in flight per thread, added in split order (hgemm_splitk_reduce_kernel)
      f32x4 p[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) p[u] = *(const f32x4*)(partial + (size_t)(k + u) * slab + e);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += p[u];
    }
    for (; k < splits; ++k) {
      const f32x4 p = *(const f32x4*)(partial + (size_t)k * slab + e);
      s += p;
    }
    const bx4 o = {(__bf16)(s[0] + (float)b[0]), (__bf16)(s[1] + (float)b[1]), (__bf16)(s[2] + (float)b[2]), (__bf16)(s[3] + (float)b[3])};
    *(bx4*)(C + (size_t)m * ldc + n) = o;
  }
}

// The reference kernel of the fused-bias calls: hgemm_generic_tn_kernel's one output per thread and its fma chain in k order, then the
// fp32 add of float(bias[n]) to the finished sum, then the one rounding.  Any shape, stride and alignment (bias 2-byte aligned).
__global__ void __launch_bounds__(256) hgemm_generic_tn_bias_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ Bcol,
                                                                    __bf16* __restrict__ C, const __bf16* __restrict__ bias, int M, int N,
                                                                    int K, int lda, int ldb_colmajor, int ldc) {
  const int n = blockIdx.x * 64 + (threadIdx.x & 63);
  if (n >= N) return;
  const float b = (float)bias[n];
  for (int m = blockIdx.y * 4 + (threadIdx.x >> 6); m < M; m += gridDim.y * 4) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = fmaf((float)A[(size_t)m * lda + k], (float)Bcol[(size_t)n * ldb_colmajor + k], s);
    C[(size_t)m * ldc + n] = (__bf16)(s + b);
  }
}

// The combine of the fused bias+activation calls (bgemm_mi355x_tn_bias_act): hgemm_splitk_reduce_bias_kernel's text -- the slabs in split
// order, THEN the bias as one fp32 add -- then act_apply<ACT> (hgemm_act.hpp, the kernels' own text) on the unrounded fp32 value, then the
// one rounding to bf16.  The activation is never applied to a slab.  New symbols: the kernels above keep theirs and their streams.
template <int ACT>
__global__ void __launch_bounds__(256) hgemm_splitk_reduce_bias_act_kernel(const float* __restrict__ partial, __bf16* __restrict__ C,
                                                                           const __bf16* __restrict__ bias, int M, int N, int ldc, int splits) {
  using bx4 = __attribute__((ext_vector_type(4))) __bf16;
  const size_t total4 = ((size_t)M * N) >> 2;
  const size_t slab   = (size_t)M * N;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total4; q += (size_t)gridDim.x * blockDim.x) {
    const size_t e = q << 2;
    const int m = (int)(e / N), n = (int)(e % N);
    const bx4 b = *(const bx4*)(bias + n);   // in flight with the slab loads
    f32x4 s = *(const f32x4*)(partial + e);
    int k = 1;
    for (; k + 8 <= splits; k += 8) {   // eight slabs' loads in flight per thread, added in split order (hgemm_splitk_reduce_kernel)
      f32x4 p[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) p[u] = *(const f32x4*)(partial + (size_t)(k + u) * slab + e);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += p[u];
    }
    for (; k < splits; ++k) {
      const f32x4 p = *(const f32x4*)(partial + (size_t)k * slab + e);
      s += p;
    }
    const bx4 o = {(__bf16)act_apply<ACT>(s[0] + (float)b[0]), (__bf16)act_apply<ACT>(s[1] + (float)b[1]),
                   (__bf16)act_apply<ACT>(s[2] + (float)b[2]), (__bf16)act_apply<ACT>(s[3] + (float)b[3])};
    *(bx4*)(C + (size_t)m * ldc + n) = o;
  }
}

// The reference kernel of the fused bias+activation calls: hgemm_generic_tn_bias_kernel's fma chain in k order and its fp32 add of
// float(bias[n]), then act_apply<ACT>, then the one rounding.  Any shape, stride and alignment (bias 2-byte aligned).
template <int ACT>
__global__ void __launch_bounds__(256) hgemm_generic_tn_bias_act_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ Bcol,
                                                                        __bf16* __restrict__ C, const __bf16* __restrict__ bias, int M, int N,
                                                                        int K, int lda, int ldb_colmajor, int ldc) {
  const int n = blockIdx.x * 64 + (threadIdx.x & 63);
  if (n >= N) return;
  const float b = (float)bias[n];
  for (int m = blockIdx.y * 4 + (threadIdx.x >> 6); m < M; m += gridDim.y * 4) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = fmaf((float)A[(size_t)m * lda + k], (float)Bcol[(size_t)n * ldb_colmajor + k], s);
    C[(size_t)m * ldc + n] = (__bf16)act_apply<ACT>(s + b);
  }
}

// The combine of bgemm_mi355x_tn_bias_act_aux: hgemm_splitk_reduce_bias_act_kernel's text with a second output -- the slabs in split
// order, the bias as one fp32 add, then z_out = bf16(z) at stride ldz and C = bf16(act_apply<ACT>(z)) of the UNROUNDED z.  No slab is touched.
template <int ACT>
__global__ void __launch_bounds__(256) hgemm_splitk_reduce_bias_act_aux_kernel(const float* __restrict__ partial, __bf16* __restrict__ C,
                                                                               const __bf16* __restrict__ bias, __bf16* __restrict__ Z, int M,
                                                                               int N, int ldc, int ldz, int splits) {
  using bx4 = __attribute__((ext_vector_type(4))) __bf16;
  const size_t total4 = ((size_t)M * N) >> 2;
  const size_t slab   = (size_t)M * N;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total4; q += (size_t)gridDim.x * blockDim.x) {
    const size_t e = q << 2;
    const int m = (int)(e / N), n = (int)(e % N);
    const bx4 b = *(const bx4*)(bias + n);   // in flight with the slab loads
    f32x4 s = *(const f32x4*)(partial + e);
    int k = 1;
    for (; k + 8 <= splits; k += 8) {   // eight slabs' loads in flight per thread, added in split order (hgemm_splitk_reduce_kernel)
      f32x4 p[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) p[u] = *(const f32x4*)(partial + (size_t)(k + u) * slab + e);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += p[u];
    }
    for (; k < splits; ++k) {
      const f32x4 p = *(const f32x4*)(partial + (size_t)k * slab + e);
      s += p;
    }
    const float z0 = s[0] + (float)b[0], z1 = s[1] + (float)b[1], z2 = s[2] + (float)b[2], z3 = s[3] + (float)b[3];
    const bx4 zo = {(__bf16)z0, (__bf16)z1, (__bf16)z2, (__bf16)z3};
    *(bx4*)(Z + (size_t)m * ldz + n) = zo;
    const bx4 o = {(__bf16)act_apply<ACT>(z0), (__bf16)act_apply<ACT>(z1), (__bf16)act_apply<ACT>(z2), (__bf16)act_apply<ACT>(z3)};
    *(bx4*)(C + (size_t)m * ldc + n) = o;
  }
}

// The reference kernel of bgemm_mi355x_tn_bias_act_aux: hgemm_generic_tn_bias_act_kernel's chain and add, both outputs from the one z.
template <int ACT>
__global__ void __launch_bounds__(256) hgemm_generic_tn_bias_act_aux_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ Bcol,
                                                                            __bf16* __restrict__ C, const __bf16* __restrict__ bias,
                                                                            __bf16* __restrict__ Z, int M, int N, int K, int lda,
                                                                            int ldb_colmajor, int ldc, int ldz) {
  const int n = blockIdx.x * 64 + (threadIdx.x & 63);
  if (n >= N) return;
  const float b = (float)bias[n];
  for (int m = blockIdx.y * 4 + (threadIdx.x >> 6); m < M; m += gridDim.y * 4) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = fmaf((float)A[(size_t)m * lda + k], (float)Bcol[(size_t)n * ldb_colmajor + k], s);
    const float z = s + b;
    Z[(size_t)m * ldz + n] = (__bf16)z;
    C[(size_t)m * ldc + n] = (__bf16)act_apply<ACT>(z);
  }
}

// The combine of bgemm_mi355x_nn_dact: the slabs added in split order (hgemm_splitk_reduce_kernel), THEN dact_mul<ACT> (hgemm_act.hpp, the
// kernels' own text) of the finished sum and float(Z[m][n]) -- one fp32 multiply, ReLU a select --, then the one rounding to bf16.  No
// slab is multiplied.  (N % 8 == 0, ldz % 8 == 0 and a 16-byte aligned Z on this path: the four z of a quad are one aligned 8-byte load.)
template <int ACT>
__global__ void __launch_bounds__(256) hgemm_splitk_reduce_dact_kernel(const float* __restrict__ partial, __bf16* __restrict__ C,
                                                                       const __bf16* __restrict__ Z, int M, int N, int ldc, int ldz,
                                                                       int splits) {
  using bx4 = __attribute__((ext_vector_type(4))) __bf16;
  const size_t total4 = ((size_t)M * N) >> 2;
  const size_t slab   = (size_t)M * N;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total4; q += (size_t)gridDim.x * blockDim.x) {
    const size_t e = q << 2;
    const int m = (int)(e / N), n = (int)(e % N);
    const bx4 z = *(const bx4*)(Z + (size_t)m * ldz + n);   // in flight with the slab loads
    f32x4 s = *(const f32x4*)(partial + e);
    int k = 1;
    for (; k + 8 <= splits; k += 8) {
      f32x4 p[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) p[u] = *(const f32x4*)(partial + (size_t)(k + u) * slab + e);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += p[u];
    }
    for (; k < splits; ++k) {
      const f32x4 p = *(const f32x4*)(partial + (size_t)k * slab + e);
      s += p;
    }
    const bx4 o = {(__bf16)dact_mul<ACT>(s[0], (float)z[0]), (__bf16)dact_mul<ACT>(s[1], (float)z[1]),
                   (__bf16)dact_mul<ACT>(s[2], (float)z[2]), (__bf16)dact_mul<ACT>(s[3], (float)z[3])};
    *(bx4*)(C + (size_t)m * ldc + n) = o;
  }
}

// The reference kernel of bgemm_mi355x_nn_dact: hgemm_generic_kernel's fma chain in k order (B row-major), dact_mul<ACT>, one rounding.
// Any shape, stride and alignment (Z 2-byte aligned).
template <int ACT>
__global__ void __launch_bounds__(256) hgemm_generic_nn_dact_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ B,
                                                                    __bf16* __restrict__ C, const __bf16* __restrict__ Z, int M, int N, int K,
                                                                    int lda, int ldb_rowmajor, int ldc, int ldz) {
  const int n = blockIdx.x * 64 + (threadIdx.x & 63);
  if (n >= N) return;
  for (int m = blockIdx.y * 4 + (threadIdx.x >> 6); m < M; m += gridDim.y * 4) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = fmaf((float)A[(size_t)m * lda + k], (float)B[(size_t)k * ldb_rowmajor + n], s);
    C[(size_t)m * ldc + n] = (__bf16)dact_mul<ACT>(s, (float)Z[(size_t)m * ldz + n]);
  }
}

// ---- the column sum of a bf16 matrix in fp32 (bgemm_mi355x_colsum_c32; part 2 of bgemm_mi355x_nn_dact_dbias's other forms; the finish
// kernel of its fused form).  hgemm_dbias.hpp states the forms and the order of the adds. --------------------------------------------------
// direct: a thread per column, the M rows in order; the one add into the old value last
__global__ void __launch_bounds__(256) hgemm_colsum_direct_kernel(const __bf16* __restrict__ X, float* __restrict__ out, int M, int N, int ldx,
                                                                  int accumulate) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float s = (float)X[n];
  for (int m = 1; m < M; ++m) s += (float)X[(size_t)m * ldx + n];
  out[n] = accumulate ? out[n] + s : s;
}

// blocked: blockIdx.y is the row block, blockIdx.x a group of COLSUM_COL_GROUPS x VEC columns; P[blockIdx.y][n] for every n < N
template <int VEC>
__global__ void __launch_bounds__(COLSUM_ROW_LANES * COLSUM_COL_GROUPS) hgemm_colsum_blocked_kernel(const __bf16* __restrict__ X,
                                                                                                   float* __restrict__ P, int M, int N, int ldx) {
  using bxv = __attribute__((ext_vector_type(VEC))) __bf16;
  __shared__ float red[COLSUM_ROW_LANES][COLSUM_COL_GROUPS * VEC];
  const int cg = threadIdx.x % COLSUM_COL_GROUPS, rl = threadIdx.x / COLSUM_COL_GROUPS;
  const int n = (blockIdx.x * COLSUM_COL_GROUPS + cg) * VEC;
  const int r0 = blockIdx.y * COLSUM_BLOCK_ROWS, r1 = min(M, r0 + COLSUM_BLOCK_ROWS);
  float s[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) s[e] = 0.0f;
  if (n + VEC <= N) {
    for (int m = r0 + rl; m < r1; m += COLSUM_ROW_LANES) {
      if constexpr (VEC == 1) {
        s[0] += (float)X[(size_t)m * ldx + n];
      } else {
        const bxv v = *(const bxv*)(X + (size_t)m * ldx + n);
#pragma unroll
        for (int e = 0; e < VEC; ++e) s[e] += (float)v[e];
      }
    }
  } else if (n < N) {   // (VEC = 8, N % 8 != 0) the ragged last group: element loads of its N - n columns -- a 16-byte load of the last row
                        // could reach behind x's last element.  Per column the same adds in the same order.
    for (int m = r0 + rl; m < r1; m += COLSUM_ROW_LANES)
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (n + e < N) s[e] += (float)X[(size_t)m * ldx + n + e];
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) red[rl][cg * VEC + e] = s[e];
  __syncthreads();
  const int c = threadIdx.x;   // a thread per column of the block's group again, the row lanes in order
  if (c < COLSUM_COL_GROUPS * VEC) {
    const int nc = blockIdx.x * COLSUM_COL_GROUPS * VEC + c;
    float a = red[0][c];
#pragma unroll
    for (int r = 1; r < COLSUM_ROW_LANES; ++r) a += red[r][c];
    if (nc < N) P[(size_t)blockIdx.y * N + nc] = a;
  }
}

// finish: the partial rows in order, then the one add into the old value
__global__ void __launch_bounds__(256) hgemm_colsum_finish_kernel(const float* __restrict__ P, float* __restrict__ out, int rows, int N,
                                                                  int accumulate) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float s = P[n];
  for (int t = 1; t < rows; ++t) s += P[(size_t)t * N + n];
  out[n] = accumulate ? out[n] + s : s;
}

void launch_colsum_direct(const void* x, float* out32, int M, int N, int ldx, bool accumulate, hipStream_t stream, TimingSlot ts) {
  HGEMM_LAUNCH(hgemm_colsum_direct_kernel, (N + 255) / 256, 256, stream, ts, (const __bf16*)x, out32, M, N, ldx, (int)accumulate);
}
void launch_colsum_blocked(const void* x, float* partial, int M, int N, int ldx, hipStream_t stream, TimingSlot ts) {
  const bool vec = (ldx & 7) == 0 && ((uintptr_t)x & 15) == 0;
  const int cols = COLSUM_COL_GROUPS * (vec ? 8 : 1);
  const dim3 grid((N + cols - 1) / cols, colsum_blocks(M));
  if (vec) HGEMM_LAUNCH(hgemm_colsum_blocked_kernel<8>, grid, COLSUM_ROW_LANES * COLSUM_COL_GROUPS, stream, ts, (const __bf16*)x, partial, M, N, ldx);
  else     HGEMM_LAUNCH(hgemm_colsum_blocked_kernel<1>, grid, COLSUM_ROW_LANES * COLSUM_COL_GROUPS, stream, ts, (const __bf16*)x, partial, M, N, ldx);
}
void launch_colsum_finish(const float* partial, float* out32, int rows, int N, bool accumulate, hipStream_t stream, TimingSlot ts) {
  HGEMM_LAUNCH(hgemm_colsum_finish_kernel, (N + 255) / 256, 256, stream, ts, partial, out32, rows, N, (int)accumulate);
}

// ---- launchers of the combines and the reference kernels, with the signatures of TrKernels (hgemm_kernel_nn.hpp) ----------------------
// grid and block of a combine: a thread per four outputs
struct CombineGrid { int grid, threads; };
static CombineGrid combine_grid(int M, int N) {
  const size_t quads = ((size_t)M * N) >> 2;
  // small outputs: 64-thread blocks so the (latency-bound) slab reads spread over more CUs
  const int threads = quads <= 64 * 1024 ? 64 : 256;
  int grid = (int)((quads + threads - 1) / threads);
  if (grid > 256 * 8) grid = 256 * 8;  // grid-stride beyond 8 blocks per CU
  if (grid < 1) grid = 1;
  return {grid, threads};
}

template <class T>
static void launch_combine(const float* partial, void* C, const void*, int M, int N, int ldc, int splits, bool, hipStream_t stream, TimingSlot ts) {
  const CombineGrid cg = combine_grid(M, N);
  HGEMM_LAUNCH((hgemm_splitk_reduce_kernel<T>), cg.grid, cg.threads, stream, ts, partial, (T*)C, M, N, ldc, splits);
}

// ldc in fp32 elements; accumulate: C32 += the sum, otherwise C32 is never read
static void launch_combine_c32(const float* partial, void* C32, const void*, int M, int N, int ldc, int splits, bool accumulate,
                               hipStream_t stream, TimingSlot ts) {
  const CombineGrid cg = combine_grid(M, N);
  HGEMM_LAUNCH(hgemm_splitk_reduce_c32_kernel, cg.grid, cg.threads, stream, ts, partial, (float*)C32, M, N, ldc, splits, accumulate ? 1 : 0);
}

template <class T, bool A_COL, bool C32>
static void launch_reference(const void* A, const void* B, void* C, const void*, int M, int N, int K, int lda, int ldb, int ldc,
                             bool accumulate, hipStream_t stream, TimingSlot ts) {
  dim3 grid((N + 63) / 64, (unsigned)std::min<long>(((long)M + 3) / 4, 65535));
  if constexpr (C32)
    HGEMM_LAUNCH((hgemm_generic_c32_kernel<T, A_COL>), grid, 256, stream, ts, (const T*)A, (const T*)B, (float*)C, M, N, K, lda, ldb, ldc,
                 accumulate ? 1 : 0);
  else
    HGEMM_LAUNCH((hgemm_generic_kernel<T, A_COL>), grid, 256, stream, ts, (const T*)A, (const T*)B, (T*)C, M, N, K, lda, ldb, ldc);
}

template <class T>
static void launch_reference_tn(const void* A, const void* Bcol, void* C, const void*, int M, int N, int K, int lda, int ldb, int ldc, bool,
                                hipStream_t stream, TimingSlot ts) {
  dim3 grid((N + 63) / 64, (unsigned)std::min<long>(((long)M + 3) / 4, 65535));
  HGEMM_LAUNCH((hgemm_generic_tn_kernel<T>), grid, 256, stream, ts, (const T*)A, (const T*)Bcol, (T*)C, M, N, K, lda, ldb, ldc);
}

// the fused-bias set's two (bgemm_mi355x_tn_bias): `bias` is the bf16 vector of N elements
static void launch_combine_bias(const float* partial, void* C, const void* bias, int M, int N, int ldc, int splits, bool, hipStream_t stream,
                                TimingSlot ts) {
  const CombineGrid cg = combine_grid(M, N);
  HGEMM_LAUNCH(hgemm_splitk_reduce_bias_kernel, cg.grid, cg.threads, stream, ts, partial, (__bf16*)C, (const __bf16*)bias, M, N, ldc, splits);
}

static void launch_reference_tn_bias(const void* A, const void* Bcol, void* C, const void* bias, int M, int N, int K, int lda, int ldb, int ldc,
                                     bool, hipStream_t stream, TimingSlot ts) {
  dim3 grid((N + 63) / 64, (unsigned)std::min<long>(((long)M + 3) / 4, 65535));
  HGEMM_LAUNCH(hgemm_generic_tn_bias_kernel, grid, 256, stream, ts, (const __bf16*)A, (const __bf16*)Bcol, (__bf16*)C, (const __bf16*)bias, M, N,
               K, lda, ldb, ldc);
}

// the fused bias+activation sets' two (bgemm_mi355x_tn_bias_act), per activation
template <int ACT>
static void launch_combine_bias_act(const float* partial, void* C, const void* bias, int M, int N, int ldc, int splits, bool, hipStream_t stream,
                                    TimingSlot ts) {
  const CombineGrid cg = combine_grid(M, N);
  HGEMM_LAUNCH((hgemm_splitk_reduce_bias_act_kernel<ACT>), cg.grid, cg.threads, stream, ts, partial, (__bf16*)C, (const __bf16*)bias, M, N, ldc,
               splits);
}

template <int ACT>
static void launch_reference_tn_bias_act(const void* A, const void* Bcol, void* C, const void* bias, int M, int N, int K, int lda, int ldb,
                                         int ldc, bool, hipStream_t stream, TimingSlot ts) {
  dim3 grid((N + 63) / 64, (unsigned)std::min<long>(((long)M + 3) / 4, 65535));
  HGEMM_LAUNCH((hgemm_generic_tn_bias_act_kernel<ACT>), grid, 256, stream, ts, (const __bf16*)A, (const __bf16*)Bcol, (__bf16*)C,
               (const __bf16*)bias, M, N, K, lda, ldb, ldc);
}

// the sets with a second matrix (TrKernels::combine_z / reference_z): bgemm_mi355x_tn_bias_act_aux's z_out, bgemm_mi355x_nn_dact's z
template <int ACT>
static void launch_combine_aux(const float* partial, void* C, const void* bias, void* z, int M, int N, int ldc, int ldz, int splits,
                               hipStream_t stream, TimingSlot ts) {
  const CombineGrid cg = combine_grid(M, N);
  HGEMM_LAUNCH((hgemm_splitk_reduce_bias_act_aux_kernel<ACT>), cg.grid, cg.threads, stream, ts, partial, (__bf16*)C, (const __bf16*)bias,
               (__bf16*)z, M, N, ldc, ldz, splits);
}
template <int ACT>
static void launch_reference_tn_aux(const void* A, const void* Bcol, void* C, const void* bias, void* z, int M, int N, int K, int lda, int ldb,
                                    int ldc, int ldz, hipStream_t stream, TimingSlot ts) {
  dim3 grid((N + 63) / 64, (unsigned)std::min<long>(((long)M + 3) / 4, 65535));
  HGEMM_LAUNCH((hgemm_generic_tn_bias_act_aux_kernel<ACT>), grid, 256, stream, ts, (const __bf16*)A, (const __bf16*)Bcol, (__bf16*)C,
               (const __bf16*)bias, (__bf16*)z, M, N, K, lda, ldb, ldc, ldz);
}
template <int ACT>
static void launch_combine_dact(const float* partial, void* C, const void*, void* z, int M, int N, int ldc, int ldz, int splits,
                                hipStream_t stream, TimingSlot ts) {
  const CombineGrid cg = combine_grid(M, N);
  HGEMM_LAUNCH((hgemm_splitk_reduce_dact_kernel<ACT>), cg.grid, cg.threads, stream, ts, partial, (__bf16*)C, (const __bf16*)z, M, N, ldc, ldz,
               splits);
}
template <int ACT>
static void launch_reference_nn_dact(const void* A, const void* B, void* C, const void*, void* z, int M, int N, int K, int lda, int ldb, int ldc,
                                     int ldz, hipStream_t stream, TimingSlot ts) {
  dim3 grid((N + 63) / 64, (unsigned)std::min<long>(((long)M + 3) / 4, 65535));
  HGEMM_LAUNCH((hgemm_generic_nn_dact_kernel<ACT>), grid, 256, stream, ts, (const __bf16*)A, (const __bf16*)B, (__bf16*)C, (const __bf16*)z, M,
               N, K, lda, ldb, ldc, ldz);
}

// the b_col_major families' names for their two (hgemm_launch.hpp)
void launch_splitk_reduce(const float* partial, f16* C, int M, int N, int ldc, int splits,
                          hipStream_t stream, TimingSlot ts) {
  launch_combine<f16>(partial, C, nullptr, M, N, ldc, splits, false, stream, ts);
}

void launch_generic(const f16* A, const f16* B, f16* C, int M, int N, int K, int lda, int ldb,
                    int ldc, hipStream_t stream, TimingSlot ts) {
  launch_reference<f16, false, false>(A, B, C, nullptr, M, N, K, lda, ldb, ldc, false, stream, ts);
}

// ---- the tables of the three layouts of the transposed-read host path (hgemm_kernel_nn.hpp: TrTable), each built by ONE expansion of the member list: a
// row is the member's geometry and its launcher in every kernel set of the layout, [TrElem][TrKind]; `kernels` names the same sets'
// combine and reference kernel.  A new kernel set is one more cell in the layout's row macro and in its `kernels`; a cell left out is
// empty (null launcher, TrKernels{}) and a call for it is refused -- the fused-bias and bias+activation kinds of NN and TA.
// (Inside functions, which both passes read: the device pass instantiates a combine or a reference kernel where it sees its launcher
// named, and a table of host function pointers at namespace scope would be emitted as a device constant.)
#define HGEMM_NN_ROW(P, ...)                                                                                \
  {HGEMM_TR_ENTRY(P, CfgNN, __VA_ARGS__), {{&HGEMM_TR_LAUNCHER(CfgNN, false, __VA_ARGS__), nullptr},        \
                                           {&HGEMM_TR_LAUNCHER(CfgNNB, false, __VA_ARGS__), nullptr, nullptr, nullptr, nullptr, nullptr, \
                                            nullptr, nullptr, nullptr,   /* the bf16 dact sets, TR_C16_DACT + ACT_* */                   \
                                            &HGEMM_NN_DACT_LAUNCHER(ACT_RELU, CfgNNB, __VA_ARGS__),                                      \
                                            &HGEMM_NN_DACT_LAUNCHER(ACT_GELU, CfgNNB, __VA_ARGS__),                                      \
                                            &HGEMM_NN_DACT_LAUNCHER(ACT_GELU_TANH, CfgNNB, __VA_ARGS__),                                 \
                                            /* the bf16 dact + dbias sets, TR_C16_DACT_DBIAS + ACT_* */                                  \
                                            &HGEMM_NN_DBIAS_LAUNCHER(ACT_RELU, CfgNNB, __VA_ARGS__),                                     \
                                            &HGEMM_NN_DBIAS_LAUNCHER(ACT_GELU, CfgNNB, __VA_ARGS__),                                     \
                                            &HGEMM_NN_DBIAS_LAUNCHER(ACT_GELU_TANH, CfgNNB, __VA_ARGS__)}}},
#define HGEMM_TA_ROW(P, ...)                                                                                                                 \
  {HGEMM_TR_ENTRY(P, CfgTA, __VA_ARGS__), {{&HGEMM_TR_LAUNCHER(CfgTA, false, __VA_ARGS__), &HGEMM_TR_LAUNCHER(CfgTA, true, __VA_ARGS__)},    \
                                           {&HGEMM_TR_LAUNCHER(CfgTAB, false, __VA_ARGS__), &HGEMM_TR_LAUNCHER(CfgTAB, true, __VA_ARGS__)}}},
// TN (family f, hgemm_kernel_tn.hpp): the bf16 sets with a 16-bit C -- plain, with the fused bias, with the bias and each activation
// (TR_C16_BIAS + ACT_*), and those again with the pre-activation as a second output (TR_C16_BIAS_AUX + ACT_*) --; every other cell is empty and a call for it is refused
#define HGEMM_TN_ROW(P, ...)                                                                                        \
  {HGEMM_TR_ENTRY(P, CfgTNB, __VA_ARGS__), {{nullptr, nullptr}, {&HGEMM_TR_LAUNCHER(CfgTNB, false, __VA_ARGS__), nullptr, \
                                                                 &HGEMM_TN_BIAS_LAUNCHER(CfgTNB, __VA_ARGS__),            \
                                                                 &HGEMM_TN_ACT_LAUNCHER(ACT_RELU, CfgTNB, __VA_ARGS__),   \
                                                                 &HGEMM_TN_ACT_LAUNCHER(ACT_GELU, CfgTNB, __VA_ARGS__),   \
                                                                 &HGEMM_TN_ACT_LAUNCHER(ACT_GELU_TANH, CfgTNB, __VA_ARGS__), \
                                                                 &HGEMM_TN_AUX_LAUNCHER(ACT_RELU, CfgTNB, __VA_ARGS__),   \
                                                                 &HGEMM_TN_AUX_LAUNCHER(ACT_GELU, CfgTNB, __VA_ARGS__),   \
                                                                 &HGEMM_TN_AUX_LAUNCHER(ACT_GELU_TANH, CfgTNB, __VA_ARGS__)}}},
// The cells of the rows and of `kernels` are positional: these are the slots the initialisers below count out.
static_assert(TR_C16_BIAS == 2 && TR_C16_BIAS + ACT_RELU == 3 && TR_C16_BIAS_AUX + ACT_RELU == 6 && TR_C16_DACT + ACT_RELU == 9 &&
              TR_C16_DACT + ACT_GELU_TANH == 11 && TR_C16_DACT_DBIAS + ACT_RELU == 12 && TR_KINDS == 15, "the slots of the positional initialisers of the three tables");
const TrTable& tr_table_nn() {
  static const TrRow rows[] = {HGEMM_TR_MEMBERS(HGEMM_NN_ROW, "n")};
  static const TrTable t = {rows, (int)(sizeof(rows) / sizeof(rows[0])),
                            {{{launch_combine<f16>, launch_reference<f16, false, false>}, {}},
                             {{launch_combine<__bf16>, launch_reference<__bf16, false, false>}, {}, {}, {}, {}, {}, {}, {}, {},
                              {nullptr, nullptr, launch_combine_dact<ACT_RELU>, launch_reference_nn_dact<ACT_RELU>},
                              {nullptr, nullptr, launch_combine_dact<ACT_GELU>, launch_reference_nn_dact<ACT_GELU>},
                              {nullptr, nullptr, launch_combine_dact<ACT_GELU_TANH>, launch_reference_nn_dact<ACT_GELU_TANH>},
                              // TR_C16_DACT_DBIAS + ACT_*: the dact sets' combine and reference kernel, unchanged; the column sum follows them
                              {nullptr, nullptr, launch_combine_dact<ACT_RELU>, launch_reference_nn_dact<ACT_RELU>},
                              {nullptr, nullptr, launch_combine_dact<ACT_GELU>, launch_reference_nn_dact<ACT_GELU>},
                              {nullptr, nullptr, launch_combine_dact<ACT_GELU_TANH>, launch_reference_nn_dact<ACT_GELU_TANH>}}}};
  return t;
}
const TrTable& tr_table_ta() {
  static const TrRow rows[] = {HGEMM_TR_MEMBERS(HGEMM_TA_ROW, "a")};
  static const TrTable t = {rows, (int)(sizeof(rows) / sizeof(rows[0])),
                            {{{launch_combine<f16>, launch_reference<f16, true, false>}, {launch_combine_c32, launch_reference<f16, true, true>}},
                             {{launch_combine<__bf16>, launch_reference<__bf16, true, false>}, {launch_combine_c32, launch_reference<__bf16, true, true>}}}};
  return t;
}

const TrTable& tr_table_tn() {
  static const TrRow rows[] = {HGEMM_TR_MEMBERS(HGEMM_TN_ROW, "f")};
  static const TrTable t = {rows, (int)(sizeof(rows) / sizeof(rows[0])),
                            {{{}, {}}, {{launch_combine<__bf16>, launch_reference_tn<__bf16>}, {}, {launch_combine_bias, launch_reference_tn_bias},
                                        {launch_combine_bias_act<ACT_RELU>, launch_reference_tn_bias_act<ACT_RELU>},
                                        {launch_combine_bias_act<ACT_GELU>, launch_reference_tn_bias_act<ACT_GELU>},
                                        {launch_combine_bias_act<ACT_GELU_TANH>, launch_reference_tn_bias_act<ACT_GELU_TANH>},
                                        {nullptr, nullptr, launch_combine_aux<ACT_RELU>, launch_reference_tn_aux<ACT_RELU>},
                                        {nullptr, nullptr, launch_combine_aux<ACT_GELU>, launch_reference_tn_aux<ACT_GELU>},
                                        {nullptr, nullptr, launch_combine_aux<ACT_GELU_TANH>, launch_reference_tn_aux<ACT_GELU_TANH>}}}};
  return t;
}

void launch_tail_reduce(const GemmArgs& g, int BM, int BN, hipStream_t stream, TimingSlot ts) {
  HGEMM_LAUNCH(hgemm_tail_reduce_kernel, g.tail_tiles * (BM / 16), 256, stream, ts, g, BM, BN);
}

// largest power of two <= 8 (halfs) that divides the row stride, K and the pointer's alignment
static int piece_width(const void* p, int ld, int K) {
  int w = 8;
  while (w > 1 && ((ld % w) || (K % w) || (reinterpret_cast<uintptr_t>(p) % (2 * w)))) w >>= 1;
  return w;
}

void launch_ragged(const GemmArgs& g0, hipStream_t stream, TimingSlot ts) {
  GemmArgs g = g0;
  const int wa = piece_width(g.A, g.lda, g.K), wb = piece_width(g.Bt, g.ldb, g.K);
  const int vec_c = ((g.N & 3) == 0) && ((g.ldc & 3) == 0) && ((reinterpret_cast<uintptr_t>(g.C) & 7) == 0);
  using Small = Cfg<64, 64, 2, 2, 16, 2>;
  using Big = Cfg<128, 128, 2, 2, 16, 2>;
  const long tiles_big = (long)((g.M + 127) / 128) * ((g.N + 127) / 128);
  if (tiles_big >= 256) {
    g.tiles_m = (g.M + 127) / 128; g.tiles_n = (g.N + 127) / 128;
    HGEMM_LAUNCH((hgemm_tn_ragged_kernel<Big>), g.tiles_m * g.tiles_n, Big::THREADS, stream, ts, g, wa, wb, vec_c);
  } else {
    g.tiles_m = (g.M + 63) / 64; g.tiles_n = (g.N + 63) / 64;
    HGEMM_LAUNCH((hgemm_tn_ragged_kernel<Small>), g.tiles_m * g.tiles_n, Small::THREADS, stream, ts, g, wa, wb, vec_c);
  }
}

}  // namespace hgemm_mi355x
