// Kernel registry (config id -> launch thunk) and the two helper kernels' launchers.
#include "hgemm_launch.hpp"
#include "hgemm_kernel_rg.hpp"
#include "hgemm_kernel_ta.hpp"
#include "hgemm_kernel_tn.hpp"
#include "hgemm_kernel_tn_gated.hpp"

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

// ---- the output kinds of the two helper kernels -----------------------------------------------------------------------------------------
// A kernel set (hgemm_kernel_nn.hpp: TrKind) has, besides its member kernels, the combine of its two-pass form and a reference kernel.  Both
// end the same way: a finished fp32 sum S[m][n] becomes the kind's output(s).  A kind states that ONCE, as a policy: its pointers and
// strides, what it reads early -- early<V>(at), issued in front of the sum so that the read is in flight with the loads that feed it --
// and what it stores from the sum, store<V>(at, S, early).  V = 4 consecutive n in the combine, whose calls are aligned as a row of C is
// (N % 8 == 0, 16-byte aligned pointers, strides that keep rows aligned: a quad is one vector access), V = 1 in the reference kernel, which
// takes any shape, stride and alignment.  act_apply / dact_mul (hgemm_act.hpp) are the member kernels' own texts.
// `at` is where the V outputs lie, m() and n(): the reference kernel's thread knows both; the combine's thread owns quad e / 4 of the M x N
// outputs and divides only where the kind asks.  (Dividing in the kernel, in front of the call, cost hgemm_splitk_reduce_kernel<OutC16<f16>>
// ten VGPRs: the quotient of a kind that reads nothing early was carried through the slab loop.)
struct ElemPos { int row, col; __device__ int m() const { return row; } __device__ int n() const { return col; } };
struct QuadPos { size_t e; int N; __device__ int m() const { return (int)(e / N); } __device__ int n() const { return (int)(e % N); } };
template <class T, int V>
using vec_t = T __attribute__((ext_vector_type(V)));
// what TrKernels' launchers are handed (host).  r / ldr: the read-only residual matrix of the add kinds and its row stride -- TrKernels' `z` /
// ldz under the name the kinds use.  r may be c (ldr == ldc): early() loads r[m][n] and store() writes C[m][n] in the same thread, the load first.
struct OutArgs { void* c; const void* bias; void* z; int ldc, ldz; bool accumulate; const void* b2; const void* bias2; const void* r; int ldr; };

template <class T, int V>
__device__ __forceinline__ vec_t<T, V> out_load(const T* p) { return *(const vec_t<T, V>*)p; }
template <int V, class T>
__device__ __forceinline__ void out_store(T* p, vec_t<float, V> v) {   // each element converted to T once: round to nearest even
  vec_t<T, V> o;
#pragma unroll
  for (int i = 0; i < V; ++i) o[i] = (T)v[i];
  *(vec_t<T, V>*)p = o;
}

// a 16-bit C of type T (f16, or __bf16: the bgemm_ calls): C = T(S)
template <class T>
struct OutC16 {
  static constexpr int SUMS = 1;   // fp32 sums per output (2: the gated kind)
  T* C; int ldc;
  static OutC16 make(const OutArgs& o) { return {(T*)o.c, o.ldc}; }
  template <int V, class At> __device__ int early(At) const { return 0; }
  template <int V, class At> __device__ void store(At at, vec_t<float, V> s, int) const { out_store<V>(C + (size_t)at.m() * ldc + at.n(), s); }
};
// the fp32 C (hgemm_mi355x_ta_c32, bgemm_mi355x_ta_c32): C32 = accumulate ? C32 + S : S -- the shape of the unsplit result, old + fl(sum);
// C32 is read only with `accumulate`, ldc counts fp32 elements
struct OutC32 {
  static constexpr int SUMS = 1;
  float* C; int ldc, accumulate;
  static OutC32 make(const OutArgs& o) { return {(float*)o.c, o.ldc, o.accumulate ? 1 : 0}; }
  template <int V, class At> __device__ vec_t<float, V> early(At at) const {
    vec_t<float, V> old = 0.f;
    if (accumulate) old = out_load<float, V>(C + (size_t)at.m() * ldc + at.n());
    return old;
  }
  template <int V, class At> __device__ void store(At at, vec_t<float, V> s, vec_t<float, V> old) const {
    *(vec_t<float, V>*)(C + (size_t)at.m() * ldc + at.n()) = accumulate ? old + s : s;
  }
};
// the fused bias (bgemm_mi355x_tn_bias, ACT_NONE) and bias + activation (bgemm_mi355x_tn_bias_act): z = S + float(bias[n]) as one fp32 add,
// C = bf16(act_apply<ACT>(z)) of the unrounded z
template <int ACT>
__device__ __forceinline__ float out_act(float z) {
  if constexpr (ACT == ACT_NONE) return z;
  else return act_apply<ACT>(z);
}
template <int ACT>
struct OutBias {
  static constexpr int SUMS = 1;
  __bf16* C; const __bf16* bias; int ldc;
  static OutBias make(const OutArgs& o) { return {(__bf16*)o.c, (const __bf16*)o.bias, o.ldc}; }
  template <int V, class At> __device__ vec_t<__bf16, V> early(At at) const { return out_load<__bf16, V>(bias + at.n()); }
  template <int V, class At> __device__ void store(At at, vec_t<float, V> s, vec_t<__bf16, V> b) const {
#pragma unroll
    for (int i = 0; i < V; ++i) s[i] = out_act<ACT>(s[i] + (float)b[i]);
    out_store<V>(C + (size_t)at.m() * ldc + at.n(), s);
  }
};
// the same with the pre-activation as a second output (bgemm_mi355x_tn_bias_act_aux): z_out = bf16(z) at stride ldz, both from the one z
template <int ACT>
struct OutBiasAux {
  static constexpr int SUMS = 1;
  __bf16* C; const __bf16* bias; __bf16* Z; int ldc, ldz;
  static OutBiasAux make(const OutArgs& o) { return {(__bf16*)o.c, (const __bf16*)o.bias, (__bf16*)o.z, o.ldc, o.ldz}; }
  template <int V, class At> __device__ vec_t<__bf16, V> early(At at) const { return out_load<__bf16, V>(bias + at.n()); }
  template <int V, class At> __device__ void store(At at, vec_t<float, V> s, vec_t<__bf16, V> b) const {
#pragma unroll
    for (int i = 0; i < V; ++i) s[i] += (float)b[i];
    out_store<V>(Z + (size_t)at.m() * ldz + at.n(), s);
#pragma unroll
    for (int i = 0; i < V; ++i) s[i] = act_apply<ACT>(s[i]);
    out_store<V>(C + (size_t)at.m() * ldc + at.n(), s);
  }
};
// the activation's derivative at a saved pre-activation (bgemm_mi355x_nn_dact, and the C of _nn_dact_dbias): C = bf16(dact_mul<ACT>(S,
// float(Z[m][n]))) -- one fp32 multiply on the finished sum, ReLU a select; Z is read-only, at stride ldz
template <int ACT>
struct OutDact {
  static constexpr int SUMS = 1;
  __bf16* C; const __bf16* Z; int ldc, ldz;
  static OutDact make(const OutArgs& o) { return {(__bf16*)o.c, (const __bf16*)o.z, o.ldc, o.ldz}; }
  template <int V, class At> __device__ vec_t<__bf16, V> early(At at) const { return out_load<__bf16, V>(Z + (size_t)at.m() * ldz + at.n()); }
  template <int V, class At> __device__ void store(At at, vec_t<float, V> s, vec_t<__bf16, V> z) const {
#pragma unroll
    for (int i = 0; i < V; ++i) s[i] = dact_mul<ACT>(s[i], (float)z[i]);
    out_store<V>(C + (size_t)at.m() * ldc + at.n(), s);
  }
};
// the fused residual add (bgemm_mi355x_nn_add): C = bf16(residual_add(S, float(R[m][n]))), hgemm_residual.hpp's one fp32 add on the finished sum;
// R is read-only at stride ldr and MAY BE C (ldr == ldc): the thread that stores C[m][n .. n + V) is the one that loaded R[m][n .. n + V) in
// early(), in front of the sum -- the combine's quad and the reference kernel's element alike --, and no other thread touches those elements.
// No __restrict__ on either pointer.
struct OutAdd {
  static constexpr int SUMS = 1;
  __bf16* C; const __bf16* R; int ldc, ldr;
  static OutAdd make(const OutArgs& o) { return {(__bf16*)o.c, (const __bf16*)o.r, o.ldc, o.ldr}; }
  template <int V, class At> __device__ vec_t<__bf16, V> early(At at) const { return out_load<__bf16, V>(R + (size_t)at.m() * ldr + at.n()); }
  template <int V, class At> __device__ void store(At at, vec_t<float, V> s, vec_t<__bf16, V> r) const {
#pragma unroll
    for (int i = 0; i < V; ++i) s[i] = residual_add(s[i], (float)r[i]);
    out_store<V>(C + (size_t)at.m() * ldc + at.n(), s);
  }
};
// the same behind a bias (bgemm_mi355x_tn_bias_add): C = bf16(bias_residual_add(S, float(bias[n]), float(R[m][n]))), two fp32 adds in that order
// and one rounding.  A null bias vector counts as +0.0, added like any other: the bits of a zero-filled vector (the gated kinds' rule).
template <int V> struct BiasAddEarly { vec_t<__bf16, V> b, r; };
struct OutBiasAdd {
  static constexpr int SUMS = 1;
  __bf16* C; const __bf16* bias; const __bf16* R; int ldc, ldr;
  static OutBiasAdd make(const OutArgs& o) { return {(__bf16*)o.c, (const __bf16*)o.bias, (const __bf16*)o.r, o.ldc, o.ldr}; }
  template <int V, class At> __device__ BiasAddEarly<V> early(At at) const {
    BiasAddEarly<V> e;
    e.b = (__bf16)0.0f;
    if (bias) e.b = out_load<__bf16, V>(bias + at.n());
    e.r = out_load<__bf16, V>(R + (size_t)at.m() * ldr + at.n());
    return e;
  }
  template <int V, class At> __device__ void store(At at, vec_t<float, V> s, BiasAddEarly<V> e) const {
#pragma unroll
    for (int i = 0; i < V; ++i) s[i] = bias_residual_add(s[i], (float)e.b[i], (float)e.r[i]);
    out_store<V>(C + (size_t)at.m() * ldc + at.n(), s);
  }
};
// the gated kind (bgemm_mi355x_tn_gated): TWO finished sums per output, Sg = X Wg^T and Su = X Wu^T; g = Sg + float(bias_g[n]) and
// u = Su + float(bias_u[n]) one fp32 add each, C = bf16(act_apply<ACT>(g) * u), one product and one rounding (hgemm_gated.hpp).  A null
// bias vector counts as +0.0, added like any other: the bits of a zero-filled vector.  Wu is the reference kernel's second B operand; it
// travels here, with the kind's other pointers, so that the kernel's argument list stays the one every other kind compiles with.
template <int V> struct GatedBias { vec_t<__bf16, V> g, u; };
template <int ACT>
struct OutGated {
  static constexpr int SUMS = 2;
  __bf16* C; const __bf16* Wu; const __bf16* bias_g; const __bf16* bias_u; int ldc;
  static OutGated make(const OutArgs& o) { return {(__bf16*)o.c, (const __bf16*)o.b2, (const __bf16*)o.bias, (const __bf16*)o.bias2, o.ldc}; }
  template <int V, class At> __device__ GatedBias<V> early(At at) const {
    GatedBias<V> b;
    b.g = (__bf16)0.0f; b.u = (__bf16)0.0f;
    if (bias_g) b.g = out_load<__bf16, V>(bias_g + at.n());
    if (bias_u) b.u = out_load<__bf16, V>(bias_u + at.n());
    return b;
  }
  template <int V, class At> __device__ void store(At at, vec_t<float, V> sg, vec_t<float, V> su, GatedBias<V> b) const {
#pragma unroll
    for (int i = 0; i < V; ++i) sg[i] = gated_mul(act_apply<ACT>(sg[i] + (float)b.g[i]), su[i] + (float)b.u[i]);
    out_store<V>(C + (size_t)at.m() * ldc + at.n(), sg);
  }
};

// the same with the rounded pre-activations as two more outputs (bgemm_mi355x_tn_gated_aux): g_out = bf16(g) and u_out = bf16(u), both at
// stride ldz, and C = bf16(act_apply<ACT>(g) * u) of the UNROUNDED g and u (gated_pre, hgemm_gated.hpp) -- three stores, each value rounded
// once.  TrKernels' signatures have no slot for a third output: `z` is the address of a host-side GatedAuxOut, which make() reads on the
// host; the two pointers travel in the policy, as Wu does.
template <int ACT>
struct OutGatedAux {
  static constexpr int SUMS = 2;
  __bf16* C; const __bf16* Wu; const __bf16* bias_g; const __bf16* bias_u; __bf16* G; __bf16* U; int ldc, ldz;
  static OutGatedAux make(const OutArgs& o) {
    const GatedAuxOut* z = (const GatedAuxOut*)o.z;
    return {(__bf16*)o.c, (const __bf16*)o.b2, (const __bf16*)o.bias, (const __bf16*)o.bias2, (__bf16*)z->g_out, (__bf16*)z->u_out, o.ldc, o.ldz};
  }
  template <int V, class At> __device__ GatedBias<V> early(At at) const {
    GatedBias<V> b;
    b.g = (__bf16)0.0f; b.u = (__bf16)0.0f;
    if (bias_g) b.g = out_load<__bf16, V>(bias_g + at.n());
    if (bias_u) b.u = out_load<__bf16, V>(bias_u + at.n());
    return b;
  }
  template <int V, class At> __device__ void store(At at, vec_t<float, V> sg, vec_t<float, V> su, GatedBias<V> b) const {
#pragma unroll
    for (int i = 0; i < V; ++i) { sg[i] = gated_pre(sg[i], (float)b.g[i]); su[i] = gated_pre(su[i], (float)b.u[i]); }
    const size_t at_z = (size_t)at.m() * ldz + at.n();
    out_store<V>(G + at_z, sg);
    out_store<V>(U + at_z, su);
#pragma unroll
    for (int i = 0; i < V; ++i) sg[i] = gated_mul(act_apply<ACT>(sg[i]), su[i]);
    out_store<V>(C + (size_t)at.m() * ldc + at.n(), sg);
  }
};

// the gated MLP's input gradient (bgemm_mi355x_nn_dgated): ONE finished sum S = dY Wd, two saved pre-activations read early (G and U, both
// at ldz) and two outputs (dG and dU, both at ldc): dgated_store (hgemm_dgated.hpp), each value rounded once.  U arrives in the signatures'
// `bias` and dU in their `bias2`, two pointers this kind has no other use for (hgemm_kernel_nn.hpp: TrKernels).
template <int V> struct DgatedSaved { vec_t<__bf16, V> g, u; };
template <int ACT>
struct OutDgated {
  static constexpr int SUMS = 1;
  __bf16* dG; __bf16* dU; const __bf16* G; const __bf16* U; int ldc, ldz;
  static OutDgated make(const OutArgs& o) {
    return {(__bf16*)o.c, (__bf16*)const_cast<void*>(o.bias2), (const __bf16*)o.z, (const __bf16*)o.bias, o.ldc, o.ldz};
  }
  template <int V, class At> __device__ DgatedSaved<V> early(At at) const {
    const size_t at_z = (size_t)at.m() * ldz + at.n();
    return {out_load<__bf16, V>(G + at_z), out_load<__bf16, V>(U + at_z)};
  }
  template <int V, class At> __device__ void store(At at, vec_t<float, V> s, DgatedSaved<V> z) const {
    vec_t<float, V> du;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const DgatedPair y = dgated_store<ACT>(s[i], (float)z.g[i], (float)z.u[i]);
      s[i] = y.dg; du[i] = y.du;
    }
    const size_t at_c = (size_t)at.m() * ldc + at.n();
    out_store<V>(dU + at_c, du);
    out_store<V>(dG + at_c, s);
  }
};

// Split-K combine of every kind: S = p[0] + p[1] + ... + p[S-1], fp32 adds in split order and one fixed order per plan, THEN the kind's
// store.  Nothing is ever applied to a slab; slabs are fp32 whatever the operands were.  (N % 4 == 0 on this path.)
// (deterministic, unlike the reference's atomicAdd split-K, a100_F32F16F16F32/64_256_16384.cu:149-152).
template <class Out>
__global__ void __launch_bounds__(256) hgemm_splitk_reduce_kernel(const float* __restrict__ partial, const Out out, int M, int N, int splits) {
  const size_t total4 = ((size_t)M * N) >> 2;
  const size_t slab   = (size_t)M * N;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total4; q += (size_t)gridDim.x * blockDim.x) {
    const size_t e = q << 2;
    const QuadPos at{e, N};
    const auto early = out.template early<4>(at);   // in flight with the slab loads
    if constexpr (Out::SUMS == 2) {
      // the gated kind: a slab is [M][2 N], row m holding its N gate sums and then its N up sums (gated_slab_index); both columns of an
      // output added over the splits in split order, then the kind's store of the two finished sums
      const int m = at.m(), n = at.n();
      f32x4 sg = *(const f32x4*)(partial + gated_slab_index(M, N, 0, m, n, 0));
      f32x4 su = *(const f32x4*)(partial + gated_slab_index(M, N, 0, m, n, 1));
      for (int k = 1; k < splits; ++k) {
        sg += *(const f32x4*)(partial + gated_slab_index(M, N, k, m, n, 0));
        su += *(const f32x4*)(partial + gated_slab_index(M, N, k, m, n, 1));
      }
      out.template store<4>(at, sg, su, early);
    } else {
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
    out.template store<4>(at, s, early);
    }
  }
}

// The combine of the fp32-C calls keeps a text of its own: as hgemm_splitk_reduce_kernel<OutC32> it measured slower than this one on an
// MI355X (tuning/combine_refactor_mi355x.jsonl: 64 x 64 outputs, 32 splits), the only kind that did.  The same sum in split order, then
// OutC32's rule: C32 = accumulate ? C32 + t : t, C32 read only with `accumulate`, the pad between N and ldc never touched.  (N % 4 == 0,
// ldc % 4 == 0 and a 16-byte aligned C32 on this path.)  The reference kernel of these calls is the shared one, with OutC32.
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

// Any-shape / any-alignment fallback of every kind (one output per thread, an fmaf chain in k order, fp32 accumulate, then the kind's store
// of the finished sum).  Correctness net for shapes the MFMA paths do not accept (K % 8 != 0, unaligned views); never tuned.  Operands<T,
// A_COL, B_COL> is how the two operands lie: A as [M][lda] or -- A_COL, the TA layout (hgemm_kernel_ta.hpp) -- a_col_major, read as
// A[k * lda + m]; B row-major [K][ldb] or -- B_COL, the TN layout (hgemm_kernel_tn.hpp) -- b_col_major, read as B[n * ldb + k].  The sum
// order is the same in all of them, so the same bits on a transposed operand.  <f16, false, false> with OutC16<f16> is the b_col_major
// families' reference kernel (launch_generic).
template <class T_, bool A_COL, bool B_COL>
struct Operands {
  using T = T_;
  static __device__ size_t a(int m, int k, int lda) { return A_COL ? (size_t)k * lda + m : (size_t)m * lda + k; }
  static __device__ size_t b(int k, int n, int ldb) { return B_COL ? (size_t)n * ldb + k : (size_t)k * ldb + n; }
};
template <class Ops, class Out>
__global__ void __launch_bounds__(256) hgemm_generic_kernel(const typename Ops::T* __restrict__ A, const typename Ops::T* __restrict__ B,
                                                            const Out out, int M, int N, int K, int lda, int ldb) {
  const int n = blockIdx.x * 64 + (threadIdx.x & 63);
  if (n >= N) return;
  // grid-stride over M: gridDim.y is capped at 65535 (M > 262140 used to fail the launch)
  for (int m = blockIdx.y * 4 + (threadIdx.x >> 6); m < M; m += gridDim.y * 4) {
    const auto early = out.template early<1>(ElemPos{m, n});
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = fmaf((float)A[Ops::a(m, k, lda)], (float)B[Ops::b(k, n, ldb)], s);
    if constexpr (Out::SUMS == 2) {   // the gated kind: a second chain in k order over the kind's second weight, then its store of both sums
      float u = 0.f;
      for (int k = 0; k < K; ++k) u = fmaf((float)A[Ops::a(m, k, lda)], (float)out.Wu[Ops::b(k, n, ldb)], u);
      out.template store<1>(ElemPos{m, n}, vec_t<float, 1>(s), vec_t<float, 1>(u), early);
    } else {
    out.template store<1>(ElemPos{m, n}, vec_t<float, 1>(s), early);
    }
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

// (Out::make() runs HERE, on the host, in front of the launch, and may READ THROUGH `z`: the gated aux kinds are handed the address of a
// host-side GatedAuxOut there -- hgemm_kernel_nn.hpp -- and OutGatedAux::make copies the two device pointers out of it.  Every other kind
// treats `z` as the device pointer it is and only stores it.  The same holds for launch_reference below.)
template <class Out>
static void launch_combine(const float* partial, void* c, const void* bias, const void* bias2, void* z, int M, int N, int ldc, int ldz, int splits,
                           bool accumulate, hipStream_t stream, TimingSlot ts) {
  const CombineGrid cg = combine_grid(M, N);
  const Out out = Out::make({c, bias, z, ldc, ldz, accumulate, nullptr, bias2, z, ldz});
  HGEMM_LAUNCH((hgemm_splitk_reduce_kernel<Out>), cg.grid, cg.threads, stream, ts, partial, out, M, N, splits);
}
// the fp32-C kind's combine is the kernel that kept its text (see there)
template <>
void launch_combine<OutC32>(const float* partial, void* c, const void*, const void*, void*, int M, int N, int ldc, int, int splits, bool accumulate,
                            hipStream_t stream, TimingSlot ts) {
  const CombineGrid cg = combine_grid(M, N);
  HGEMM_LAUNCH(hgemm_splitk_reduce_c32_kernel, cg.grid, cg.threads, stream, ts, partial, (float*)c, M, N, ldc, splits, accumulate ? 1 : 0);
}

template <class Ops, class Out>
static void launch_reference(const void* A, const void* B, const void* B2, void* c, const void* bias, const void* bias2, void* z, int M, int N, int K,
                             int lda, int ldb, int ldc, int ldz, bool accumulate, hipStream_t stream, TimingSlot ts) {
  using T = typename Ops::T;
  dim3 grid((N + 63) / 64, (unsigned)std::min<long>(((long)M + 3) / 4, 65535));
  const Out out = Out::make({c, bias, z, ldc, ldz, accumulate, B2, bias2, z, ldz});
  HGEMM_LAUNCH((hgemm_generic_kernel<Ops, Out>), grid, 256, stream, ts, (const T*)A, (const T*)B, out, M, N, K, lda, ldb);
}

// the b_col_major families' names for their two (hgemm_launch.hpp)
void launch_splitk_reduce(const float* partial, f16* C, int M, int N, int ldc, int splits,
                          hipStream_t stream, TimingSlot ts) {
  launch_combine<OutC16<f16>>(partial, C, nullptr, nullptr, nullptr, M, N, ldc, 0, splits, false, stream, ts);
}

void launch_generic(const f16* A, const f16* B, f16* C, int M, int N, int K, int lda, int ldb,
                    int ldc, hipStream_t stream, TimingSlot ts) {
  launch_reference<Operands<f16, false, false>, OutC16<f16>>(A, B, nullptr, C, nullptr, nullptr, nullptr, M, N, K, lda, ldb, ldc, 0, false, stream, ts);
}

// ---- the tables of the three layouts of the transposed-read host path (hgemm_kernel_nn.hpp: TrTable), each built by ONE expansion of the
// member list: a row is the member's geometry and its launcher in every kernel set of the layout, `kernels` names the same sets' combine
// and reference kernel, both filled by [TrElem][TrKind] index.  A new kernel set is one cell in the layout's row builder and one in its
// `kernels`; a cell that is not assigned is empty (null launcher, TrKernels{}) and a call for it is refused -- the fused-bias kinds of NN
// and TA, say.
// (Inside functions, which both passes read: the device pass instantiates a combine or a reference kernel where it sees its launcher
// named, and a table of host function pointers at namespace scope would be emitted as a device constant.)
template <class Ops, class Out>
static TrKernels tr_kernels() { return {launch_combine<Out>, launch_reference<Ops, Out>}; }

// G: the member's BM, BN, WM, WN, NBUF (HGEMM_TR_MEMBERS)
template <int... G>
static TrRow nn_row(TrEntry e) {
  using F = CfgNN<G...>;
  using B = CfgNNB<G...>;
  TrRow r{e, {}};
  r.launch[TR_F16][TR_C16] = &launch_tr<F, false>;
  r.launch[TR_BF16][TR_C16] = &launch_tr<B, false>;
  r.launch[TR_BF16][TR_C16_DACT + ACT_RELU] = &launch_nn_dact<B, ACT_RELU>;
  r.launch[TR_BF16][TR_C16_DACT + ACT_GELU] = &launch_nn_dact<B, ACT_GELU>;
  r.launch[TR_BF16][TR_C16_DACT + ACT_GELU_TANH] = &launch_nn_dact<B, ACT_GELU_TANH>;
  r.launch[TR_BF16][TR_C16_DACT_DBIAS + ACT_RELU] = &launch_nn_dbias<B, ACT_RELU>;
  r.launch[TR_BF16][TR_C16_DACT_DBIAS + ACT_GELU] = &launch_nn_dbias<B, ACT_GELU>;
  r.launch[TR_BF16][TR_C16_DACT_DBIAS + ACT_GELU_TANH] = &launch_nn_dbias<B, ACT_GELU_TANH>;
  r.launch[TR_BF16][TR_C16_DGATED + ACT_RELU] = &launch_nn_dgated<B, ACT_RELU>;
  r.launch[TR_BF16][TR_C16_DGATED + ACT_GELU] = &launch_nn_dgated<B, ACT_GELU>;
  r.launch[TR_BF16][TR_C16_DGATED + ACT_GELU_TANH] = &launch_nn_dgated<B, ACT_GELU_TANH>;
  r.launch[TR_BF16][TR_C16_DGATED + ACT_SILU] = &launch_nn_dgated<B, ACT_SILU>;
  r.launch[TR_BF16][TR_C16_ADD] = &launch_nn_add<B>;
  return r;
}
template <int... G>
static TrRow ta_row(TrEntry e) {
  TrRow r{e, {}};
  r.launch[TR_F16][TR_C16] = &launch_tr<CfgTA<G...>, false>;
  r.launch[TR_F16][TR_C32] = &launch_tr<CfgTA<G...>, true>;
  r.launch[TR_BF16][TR_C16] = &launch_tr<CfgTAB<G...>, false>;
  r.launch[TR_BF16][TR_C32] = &launch_tr<CfgTAB<G...>, true>;
  return r;
}
// TN (family f, hgemm_kernel_tn.hpp): bf16 sets with a 16-bit C only
template <int... G>
static TrRow tn_row(TrEntry e) {
  using B = CfgTNB<G...>;
  TrRow r{e, {}};
  r.launch[TR_BF16][TR_C16] = &launch_tr<B, false>;
  r.launch[TR_BF16][TR_C16_BIAS] = &launch_tn_bias<B>;
  r.launch[TR_BF16][TR_C16_BIAS + ACT_RELU] = &launch_tn_bias_act<B, ACT_RELU>;
  r.launch[TR_BF16][TR_C16_BIAS + ACT_GELU] = &launch_tn_bias_act<B, ACT_GELU>;
  r.launch[TR_BF16][TR_C16_BIAS + ACT_GELU_TANH] = &launch_tn_bias_act<B, ACT_GELU_TANH>;
  r.launch[TR_BF16][TR_C16_BIAS_AUX + ACT_RELU] = &launch_tn_bias_act_aux<B, ACT_RELU>;
  r.launch[TR_BF16][TR_C16_BIAS_AUX + ACT_GELU] = &launch_tn_bias_act_aux<B, ACT_GELU>;
  r.launch[TR_BF16][TR_C16_BIAS_AUX + ACT_GELU_TANH] = &launch_tn_bias_act_aux<B, ACT_GELU_TANH>;
  r.launch[TR_BF16][TR_C16_GATED + ACT_RELU] = &launch_tn_gated<B, ACT_RELU>;
  r.launch[TR_BF16][TR_C16_GATED + ACT_GELU] = &launch_tn_gated<B, ACT_GELU>;
  r.launch[TR_BF16][TR_C16_GATED + ACT_GELU_TANH] = &launch_tn_gated<B, ACT_GELU_TANH>;
  r.launch[TR_BF16][TR_C16_GATED + ACT_SILU] = &launch_tn_gated<B, ACT_SILU>;
  r.launch[TR_BF16][TR_C16_GATED_AUX + ACT_RELU] = &launch_tn_gated_aux<B, ACT_RELU>;
  r.launch[TR_BF16][TR_C16_GATED_AUX + ACT_GELU] = &launch_tn_gated_aux<B, ACT_GELU>;
  r.launch[TR_BF16][TR_C16_GATED_AUX + ACT_GELU_TANH] = &launch_tn_gated_aux<B, ACT_GELU_TANH>;
  r.launch[TR_BF16][TR_C16_GATED_AUX + ACT_SILU] = &launch_tn_gated_aux<B, ACT_SILU>;
  r.launch[TR_BF16][TR_C16_BIAS_ADD] = &launch_tn_bias_add<B>;
  return r;
}
#define HGEMM_TR_ROW(ROW, P, CFG, ...) ROW<__VA_ARGS__>(HGEMM_TR_ENTRY(P, CFG, __VA_ARGS__)),

const TrTable& tr_table_nn() {
  static const TrRow rows[] = {HGEMM_TR_MEMBERS(HGEMM_TR_ROW, nn_row, "n", CfgNN)};
  static const TrTable table = [] {
    using F = Operands<f16, false, false>;
    using B = Operands<__bf16, false, false>;
    TrTable t{rows, (int)(sizeof(rows) / sizeof(rows[0])), {}};
    t.kernels[TR_F16][TR_C16] = tr_kernels<F, OutC16<f16>>();
    t.kernels[TR_BF16][TR_C16] = tr_kernels<B, OutC16<__bf16>>();
    t.kernels[TR_BF16][TR_C16_DACT + ACT_RELU] = tr_kernels<B, OutDact<ACT_RELU>>();
    t.kernels[TR_BF16][TR_C16_DACT + ACT_GELU] = tr_kernels<B, OutDact<ACT_GELU>>();
    t.kernels[TR_BF16][TR_C16_DACT + ACT_GELU_TANH] = tr_kernels<B, OutDact<ACT_GELU_TANH>>();
    // the dact sets' combine and reference kernel, unchanged; the column sum follows them
    t.kernels[TR_BF16][TR_C16_DACT_DBIAS + ACT_RELU] = tr_kernels<B, OutDact<ACT_RELU>>();
    t.kernels[TR_BF16][TR_C16_DACT_DBIAS + ACT_GELU] = tr_kernels<B, OutDact<ACT_GELU>>();
    t.kernels[TR_BF16][TR_C16_DACT_DBIAS + ACT_GELU_TANH] = tr_kernels<B, OutDact<ACT_GELU_TANH>>();
    t.kernels[TR_BF16][TR_C16_DGATED + ACT_RELU] = tr_kernels<B, OutDgated<ACT_RELU>>();
    t.kernels[TR_BF16][TR_C16_DGATED + ACT_GELU] = tr_kernels<B, OutDgated<ACT_GELU>>();
    t.kernels[TR_BF16][TR_C16_DGATED + ACT_GELU_TANH] = tr_kernels<B, OutDgated<ACT_GELU_TANH>>();
    t.kernels[TR_BF16][TR_C16_DGATED + ACT_SILU] = tr_kernels<B, OutDgated<ACT_SILU>>();
    t.kernels[TR_BF16][TR_C16_ADD] = tr_kernels<B, OutAdd>();
    return t;
  }();
  return table;
}
const TrTable& tr_table_ta() {
  static const TrRow rows[] = {HGEMM_TR_MEMBERS(HGEMM_TR_ROW, ta_row, "a", CfgTA)};
  static const TrTable table = [] {
    using F = Operands<f16, true, false>;
    using B = Operands<__bf16, true, false>;
    TrTable t{rows, (int)(sizeof(rows) / sizeof(rows[0])), {}};
    t.kernels[TR_F16][TR_C16] = tr_kernels<F, OutC16<f16>>();
    t.kernels[TR_F16][TR_C32] = tr_kernels<F, OutC32>();
    t.kernels[TR_BF16][TR_C16] = tr_kernels<B, OutC16<__bf16>>();
    t.kernels[TR_BF16][TR_C32] = tr_kernels<B, OutC32>();
    return t;
  }();
  return table;
}
const TrTable& tr_table_tn() {
  static const TrRow rows[] = {HGEMM_TR_MEMBERS(HGEMM_TR_ROW, tn_row, "f", CfgTNB)};
  static const TrTable table = [] {
    using B = Operands<__bf16, false, true>;
    TrTable t{rows, (int)(sizeof(rows) / sizeof(rows[0])), {}};
    t.kernels[TR_BF16][TR_C16] = tr_kernels<B, OutC16<__bf16>>();
    t.kernels[TR_BF16][TR_C16_BIAS] = tr_kernels<B, OutBias<ACT_NONE>>();
    t.kernels[TR_BF16][TR_C16_BIAS + ACT_RELU] = tr_kernels<B, OutBias<ACT_RELU>>();
    t.kernels[TR_BF16][TR_C16_BIAS + ACT_GELU] = tr_kernels<B, OutBias<ACT_GELU>>();
    t.kernels[TR_BF16][TR_C16_BIAS + ACT_GELU_TANH] = tr_kernels<B, OutBias<ACT_GELU_TANH>>();
    t.kernels[TR_BF16][TR_C16_BIAS_AUX + ACT_RELU] = tr_kernels<B, OutBiasAux<ACT_RELU>>();
    t.kernels[TR_BF16][TR_C16_BIAS_AUX + ACT_GELU] = tr_kernels<B, OutBiasAux<ACT_GELU>>();
    t.kernels[TR_BF16][TR_C16_BIAS_AUX + ACT_GELU_TANH] = tr_kernels<B, OutBiasAux<ACT_GELU_TANH>>();
    t.kernels[TR_BF16][TR_C16_GATED + ACT_RELU] = tr_kernels<B, OutGated<ACT_RELU>>();
    t.kernels[TR_BF16][TR_C16_GATED + ACT_GELU] = tr_kernels<B, OutGated<ACT_GELU>>();
    t.kernels[TR_BF16][TR_C16_GATED + ACT_GELU_TANH] = tr_kernels<B, OutGated<ACT_GELU_TANH>>();
    t.kernels[TR_BF16][TR_C16_GATED + ACT_SILU] = tr_kernels<B, OutGated<ACT_SILU>>();
    t.kernels[TR_BF16][TR_C16_GATED_AUX + ACT_RELU] = tr_kernels<B, OutGatedAux<ACT_RELU>>();
    t.kernels[TR_BF16][TR_C16_GATED_AUX + ACT_GELU] = tr_kernels<B, OutGatedAux<ACT_GELU>>();
    t.kernels[TR_BF16][TR_C16_GATED_AUX + ACT_GELU_TANH] = tr_kernels<B, OutGatedAux<ACT_GELU_TANH>>();
    t.kernels[TR_BF16][TR_C16_GATED_AUX + ACT_SILU] = tr_kernels<B, OutGatedAux<ACT_SILU>>();
    t.kernels[TR_BF16][TR_C16_BIAS_ADD] = tr_kernels<B, OutBiasAdd>();
    return t;
  }();
  return table;
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
