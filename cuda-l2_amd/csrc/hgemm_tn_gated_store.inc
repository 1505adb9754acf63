// The bf16 store of one output of family f's gated kernels (hgemm_kernel_tn_gated.hpp): the statements behind the finished values, which
// the kernel provides as acc[FM][FN_ALL] with g, tc, lane, wave_m, wave_n, FM, OFN, TN, elem, MEMBER and the types u32x2 / u32x4.  A text
// and not a function, for hgemm_tr_store_c16.inc's reason; entered once by the kernels of bgemm_mi355x_tn_gated (C) and three times by
// those of bgemm_mi355x_tn_gated_aux, which name the output in front of the include:
//   HGEMM_GATED_STORE_OUTPUT   which matrix                     base                stride               the lane's values
//   0                          g_out = bf16(g)                  tn_gated_aux_g(g)   tn_gated_aux_ldz(g)  acc[i][jo]
//   1                          u_out = bf16(u)                  tn_gated_aux_u(g)   tn_gated_aux_ldz(g)  acc[i][jo + OFN]
//   2 (or not defined)         C                                g.C                 g.ldc                acc[i][jo]
// THE ONE PLACE that pairs an output's base with its stride: tests/test_tn_gated_aux_host.py compiles this text for the CPU, enters it as the
// kernel does and holds every store of every lane inside its own matrix at its own stride.
// Two output fragments per wave (BN = 128): the family's 16-bit C epilogue, convert, swap and 16-byte stores.  One (BN = 64): the lane's
// four columns, one 8-byte buffer store; the NT hint an instruction of its own.
#ifndef HGEMM_GATED_STORE_OUTPUT
#define HGEMM_GATED_STORE_OUTPUT 2
#define HGEMM_GATED_STORE_DEFAULT
#endif
#if HGEMM_GATED_STORE_OUTPUT == 0
#define HGEMM_GATED_STORE_BASE tn_gated_aux_g(g)
#define HGEMM_GATED_STORE_STRIDE tn_gated_aux_ldz(g)
#define HGEMM_GATED_STORE_J0 0
#elif HGEMM_GATED_STORE_OUTPUT == 1
#define HGEMM_GATED_STORE_BASE tn_gated_aux_u(g)
#define HGEMM_GATED_STORE_STRIDE tn_gated_aux_ldz(g)
#define HGEMM_GATED_STORE_J0 OFN
#else
#define HGEMM_GATED_STORE_BASE g.C
#define HGEMM_GATED_STORE_STRIDE g.ldc
#define HGEMM_GATED_STORE_J0 0
#endif
    if constexpr (OFN >= 2) {
      // two output fragments per wave: the family's 16-bit C epilogue over acc[i][0 .. OFN - 1]
      constexpr int FN = OFN;
      using CFG = GatedOutView<MEMBER>;
#if HGEMM_GATED_STORE_OUTPUT == 2
#include "hgemm_tr_store_c16.inc"
#else
#define HGEMM_TR_STORE_C HGEMM_GATED_STORE_BASE
#define HGEMM_TR_STORE_LD HGEMM_GATED_STORE_STRIDE
#if HGEMM_GATED_STORE_OUTPUT == 0
#include "hgemm_tr_store_c16.inc"
#else
      // (the store text reads `acc[i][j]`: the up values are the fragments OFN .. 2 OFN - 1 of the same array)
      auto& gated_acc_all = acc;
      {
        const GatedFragView<f32x4, FM, 2 * OFN, HGEMM_GATED_STORE_J0> acc{gated_acc_all};
#include "hgemm_tr_store_c16.inc"
      }
#endif
#undef HGEMM_TR_STORE_C
#undef HGEMM_TR_STORE_LD
#endif
    } else {
      // one output fragment per wave: the lane's four columns, one 8-byte buffer store; the NT hint an instruction of its own
      using h2 = __attribute__((ext_vector_type(2))) elem;
      const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc((void*)(HGEMM_GATED_STORE_BASE + (size_t)tc.m0 * HGEMM_GATED_STORE_STRIDE), 0, 0xFFFFFFFFu, 0x00020000);
      const int n = tc.n0 + gated_lane_col(wave_n, TN, 0, lane, 0);
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int row = dbias_row(wave_m, MEMBER::TM, i, lane);
        const h2 y01 = {(elem)acc[i][HGEMM_GATED_STORE_J0][0], (elem)acc[i][HGEMM_GATED_STORE_J0][1]}, y23 = {(elem)acc[i][HGEMM_GATED_STORE_J0][2], (elem)acc[i][HGEMM_GATED_STORE_J0][3]};
        if (tc.m0 + row < g.M && n < g.N) {
          const u32x2 o = {__builtin_bit_cast(unsigned, y01), __builtin_bit_cast(unsigned, y23)};
          const uint32_t off = ((uint32_t)row * (uint32_t)HGEMM_GATED_STORE_STRIDE + (uint32_t)n) * 2u;
          if (g.flags & ARG_NT_STORE) __builtin_amdgcn_raw_buffer_store_b64(o, rsC, off, 0, 2);
          else                        __builtin_amdgcn_raw_buffer_store_b64(o, rsC, off, 0, 0);
        }
      }
    }
#undef HGEMM_GATED_STORE_BASE
#undef HGEMM_GATED_STORE_STRIDE
#undef HGEMM_GATED_STORE_J0
#ifdef HGEMM_GATED_STORE_DEFAULT
#undef HGEMM_GATED_STORE_OUTPUT
#undef HGEMM_GATED_STORE_DEFAULT
#endif
