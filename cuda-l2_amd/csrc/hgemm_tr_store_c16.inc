// The 16-bit C epilogue of families n, a and f (hgemm_kernel_nn.hpp, _ta.hpp, _tn.hpp): the statements of the `else` branch behind
// EPI_SLAB / EPI_C32 in each of the three kernels, which provide g, tc, acc, lane, wave_m, wave_n, FM, FN, elem and CFG.  A text and not
// a function: as a force-inlined function (g and tc by reference, the wave index or wave_m / wave_n by value) it compiled to another
// instruction stream in all 20 EPI_C16 kernels, registers in front of the K loop included (DESIGN.md 4.22); included, the compiler
// sees what it saw when the text stood in each kernel.
//
// fp16 C, or bf16 C from v_cvt_pk_bf16_f32 (round to nearest even, once), in the 16-byte form of store_tile_row alone (the host sends
// the kernels N % 8 == 0, ldc % 8 == 0 and a 16-byte aligned C): v_permlane16_swap exchanges the odd 16-lane rows of column tile j with
// the even rows of tile j + 1, after which row q = lane >> 4 owns n = 16 (j + (q & 1)) + 8 (q >> 1) + 0 .. 7 of its C row.  Buffer
// stores: the non-temporal form is an instruction of its own (two plain C++ stores that differ only in the hint are merged by the
// optimiser and the hint is lost); the tile's bytes are below 2 GiB from its first row (host check).
// HGEMM_TR_STORE_C / HGEMM_TR_STORE_LD: the output's base pointer and row stride, g.C and g.ldc unless the including kernel names others
// (family f's second output, bgemm_mi355x_tn_bias_act_aux, enters the text a second time with z_out and ldz).  A block of its own, so
// that it can be entered twice.
#ifndef HGEMM_TR_STORE_C
#define HGEMM_TR_STORE_C g.C
#define HGEMM_TR_STORE_LD g.ldc
#define HGEMM_TR_STORE_DEFAULTS
#endif
  {
    using h2 = __attribute__((ext_vector_type(2))) elem;
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc((void*)(HGEMM_TR_STORE_C + (size_t)tc.m0 * HGEMM_TR_STORE_LD), 0, 0xFFFFFFFFu, 0x00020000);
    const int q = lane >> 4;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      __builtin_amdgcn_sched_barrier(0);   // one fragment row's accumulator reads at a time (store_tile)
      const int row = wave_m * CFG::TM + i * 16 + (lane & 15);
#pragma unroll
      for (int j = 0; j < FN; j += 2) {
        const h2 a01 = {(elem)acc[i][j][0], (elem)acc[i][j][1]}, a23 = {(elem)acc[i][j][2], (elem)acc[i][j][3]};
        const h2 b01 = {(elem)acc[i][j + 1][0], (elem)acc[i][j + 1][1]}, b23 = {(elem)acc[i][j + 1][2], (elem)acc[i][j + 1][3]};
        const auto r0 = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a01), __builtin_bit_cast(unsigned, b01), false, false);
        const auto r1 = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a23), __builtin_bit_cast(unsigned, b23), false, false);
        const int n = tc.n0 + wave_n * CFG::TN + 16 * (j + (q & 1)) + 8 * (q >> 1);
        if (tc.m0 + row < g.M && n < g.N) {
          const u32x4 o = {r0[0], r1[0], r0[1], r1[1]};
          const uint32_t off = ((uint32_t)row * (uint32_t)HGEMM_TR_STORE_LD + (uint32_t)n) * 2u;
          if (g.flags & ARG_NT_STORE) __builtin_amdgcn_raw_buffer_store_b128(o, rsC, off, 0, 2);
          else                        __builtin_amdgcn_raw_buffer_store_b128(o, rsC, off, 0, 0);
        }
      }
    }
  }
#ifdef HGEMM_TR_STORE_DEFAULTS
#undef HGEMM_TR_STORE_C
#undef HGEMM_TR_STORE_LD
#undef HGEMM_TR_STORE_DEFAULTS
#endif
