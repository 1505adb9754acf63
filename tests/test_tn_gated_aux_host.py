"""CPU tests of the gated forward product's training form, bgemm_mi355x_tn_gated_aux (H, g_out = bf16(g) and u_out = bf16(u) in one call:
family f's gated aux kernels in hgemm_inst_g20.hip, the kinds TR_C16_GATED_AUX + act): the names and constants; the self-check hook against
the gated call's answer over tests/test_tn_bias_host.py's sweep and the rules of ldz; refusals; the store text of
hgemm_tn_gated_store.inc compiled for the CPU and walked over every lane of every member and every ragged N for all three outputs; and an
ISA audit of unit g20 by counting, against the gated twins of unit g18."""
import ctypes
import itertools
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from test_ta_host import CSRC, HIPCC, PKG, REPO
from test_ta_host import lib as ta_lib  # noqa: F401  (fixture: the built library)
from test_tn_bf16_host import EPI_SLAB, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, MEMBERS, TILES, WORDS, tn_info
from test_tn_bf16_host import lib  # noqa: F401  (fixture: the library with the tn prototypes)
from test_tn_bias_act_host import k_loop, reg
from test_tn_bias_host import SHAPES
from test_tn_gated_host import ACTS, EPI_C16_GATED, RELU, SILU, gated_answer, gated_isa, member_kernel

EPI_C16_GATED_AUX = 128
PUBLIC = ("bgemm_mi355x_tn_gated_aux", "bgemm_mi355x_launch_tn_gated_aux", "bgemm_mi355x_tn_gated_aux_runs")
HOOK = "bgemm_mi355x_selfcheck_launch_tn_gated_aux"


def aux_answer(lib, act, cid, word, aligned, m, n, k, lda, ldb, ldc, ldz, ruled_out=0, hook=HOOK):
    out = (ctypes.c_longlong * 20)()
    st = getattr(lib, hook)(cid, word, 4 if aligned else 0, m, n, k, lda, ldb, ldc, ldz, ruled_out, act, out)
    return [st] if st != 0 else [0] + list(out[:4]) + [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def with_aux_epi(gated, act):
    if gated == [-1]:
        return gated
    return list(gated[:5]) + [(t, grid, EPI_C16_GATED_AUX + act if epi == EPI_C16_GATED + act else epi, s, kc) for t, grid, epi, s, kc in gated[5:]]


def test_the_names_the_constants_and_the_unit(lib):
    header = (REPO / "include" / "hgemm_mi355x.h").read_text()
    for nm in PUBLIC:
        assert re.search(rf"\b{nm}\(", header), f"{nm} is not declared in include/hgemm_mi355x.h"
        assert getattr(lib, nm) is not None
    assert getattr(lib, HOOK) is not None and "selfcheck_launch_tn_gated_aux" not in header
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index("Training form of the gated forward product"):header.index("int bgemm_mi355x_tn_gated_aux(")])
    for words in ("u_out = g_out + N with ldz >= 2N", "g_out[m][n] = bf16_rne( g[m][n] )", "u_out[m][n] = bf16_rne( u[m][n] )", "see the UNROUNDED g and u",
                  "Each of the three outputs is rounded once", "the combine writes all three outputs", "HGEMM_PLAN_NT_STORE applies to all three outputs",
                  "C is the C of bgemm_mi355x_launch_tn_gated, bit for bit", "g_out is the C of bgemm_mi355x_launch_tn_bias", "g_out == u_out", "ldz < N",
                  "bgemm_mi355x_tn_plan(M, 2N, K)", "(BM ldz + N) 2"):
        assert words in block, words
    for nm in ("hgemm_mi355x_tn_gated_aux", "bgemm_mi355x_nn_gated_aux", "bgemm_mi355x_ta_gated_aux", "bgemm_mi355x_tn_gated_aux_plan"):
        assert not hasattr(lib, nm), nm
    assert "hgemm_inst_g20.hip" in (PKG / "build.py").read_text()
    g20 = (CSRC / "hgemm_inst_g20.hip").read_text()
    for act in ("ACT_RELU", "ACT_GELU", "ACT_GELU_TANH", "ACT_SILU"):
        assert f"HGEMM_TR_MEMBERS(HGEMM_TN_GATED_AUX_INST, {act}, CfgTNB)" in g20
    assert "SLAB" not in g20, "the K slices are unit g18's slab kernels: not instantiated again"
    assert "constexpr int EPI_C16_GATED_AUX = 128;" in (CSRC / "hgemm_kernel.hpp").read_text()
    for src in ("hgemm_kernel_tn_gated.hpp", "hgemm_registry.hip"):
        text = (CSRC / src).read_text()
        assert "gated_pre(" in text and "gated_mul(" in text and "act_apply<" in text, f"{src} does not use the shared texts"


def test_the_hook_answers_as_the_gated_call_with_the_rules_of_ldz_added(lib):
    """Over the sweep of tests/test_tn_bias_host.py: the gated call's answer with the epi id replaced, for ldz = N, N + 8 and 2 N + 8; an
    ldz % 8 != 0 sends the call to the reference kernel, ldz < N refuses it, and _runs says the same."""
    seen = set()
    for cid, (m, n, k), word in itertools.product(range(4), SHAPES, WORDS):
        for lds in ((k, k, n), (k + 8, k + 16, n + 8)):
            for aligned, ruled_out in ((True, 0), (False, 0), (True, 1 << FORM_SPLITK)):
                for act in (RELU, SILU):
                    gated = gated_answer(lib, act, cid, word, aligned, m, n, k, *lds, ruled_out)
                    for ldz in (n, n + 8, 2 * n + 8):
                        got = aux_answer(lib, act, cid, word, aligned, m, n, k, *lds, ldz, ruled_out)
                        if ldz % 8 and gated != [-1]:
                            assert got[:3] == [0, FORM_REFERENCE, 1] and got[5][2] == EPI_C16_GATED_AUX + act
                            continue
                        assert got == with_aux_epi(gated, act), (MEMBERS[cid], (m, n, k), hex(word), lds, ldz, aligned, ruled_out, act)
                        if got != [-1]:
                            seen.add((got[1], tuple(d[2] for d in got[5:])))
                    got = aux_answer(lib, act, cid, word, aligned, m, n, k, *lds, n + 4, ruled_out)
                    assert got[:3] == [0, FORM_REFERENCE, 1] and got[5][2] == EPI_C16_GATED_AUX + act
                    assert aux_answer(lib, act, cid, word, aligned, m, n, k, *lds, n - 1, ruled_out) == [-1]
            want = lib.bgemm_mi355x_tn_gated_runs(cid, m, n, k, *lds)
            assert lib.bgemm_mi355x_tn_gated_aux_runs(cid, m, n, k, *lds, n + 8) == (want if n % 8 == 0 else 0)
            assert lib.bgemm_mi355x_tn_gated_aux_runs(cid, m, n, k, *lds, n + 4) == 0 and lib.bgemm_mi355x_tn_gated_aux_runs(cid, m, n, k, *lds, n - 8) == 0
    for act in (RELU, SILU):
        assert {(FORM_REFERENCE, (EPI_C16_GATED_AUX + act,)), (FORM_PLAIN, (EPI_C16_GATED_AUX + act,)), (FORM_SPLITK, (EPI_SLAB, EPI_C16_GATED_AUX + act))} <= seen


def test_the_reach_of_g_out_and_u_out_is_cs(lib):
    """(BM ldz + N) 2 bytes below 2 GiB: the largest ldz that runs is the rule's; from the edge on the reference kernel."""
    for cid, (bm, bn) in enumerate(TILES):
        m, n, k = bm + 8, bn + 8, 128
        edge = ((1 << 30) - n) // bm // 8 * 8
        while (bm * edge + n) * 2 < (1 << 31):
            edge += 8
        assert aux_answer(lib, RELU, cid, 1, True, m, n, k, k, k, n, edge - 8)[1] == FORM_PLAIN and lib.bgemm_mi355x_tn_gated_aux_runs(cid, m, n, k, k, k, n, edge - 8) == 1
        assert aux_answer(lib, RELU, cid, 1, True, m, n, k, k, k, n, edge)[:2] == [0, FORM_REFERENCE] and lib.bgemm_mi355x_tn_gated_aux_runs(cid, m, n, k, k, k, n, edge) == 0


def test_the_nn_and_ta_layouts_refuse_the_kinds_and_bad_arguments_are_refused_before_any_hip_call(lib):
    for hook, lds in (("bgemm_mi355x_selfcheck_launch_nn_gated_aux", lambda m, n, k: (k, n, n)), ("bgemm_mi355x_selfcheck_launch_ta_gated_aux", lambda m, n, k: (m, n, n))):
        for cid, (m, n, k), word, act in itertools.product(range(4), SHAPES[:4], (1, 2), ACTS):
            assert aux_answer(lib, act, cid, word, True, m, n, k, *lds(m, n, k), n, hook=hook) == [-1], (hook, cid, (m, n, k), word, act)
    m, n, k = 200, 136, 128
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_launch_tn_gated_aux.argtypes = [ci] * 2 + [vp] * 8 + [ci] * 8 + [vp]
    lib.bgemm_mi355x_tn_gated_aux.argtypes = [vp] * 8 + [ci] * 4 + [vp]
    null, some, other, third = vp(0), vp(4096), vp(1 << 20), vp(1 << 21)
    launch = lambda a, wg, wu, c, go, uo, ldz=n, act=SILU, cid=0: lib.bgemm_mi355x_launch_tn_gated_aux(cid, 1, a, wg, wu, null, null, c, go, uo, m, n, k, k, k, n, ldz, act, null)  # noqa: E731
    for ptrs in ((null, some, some, some, other, third), (some, null, some, some, other, third), (some, some, null, some, other, third),
                 (some, some, some, null, other, third), (some, some, some, some, null, third), (some, some, some, some, other, null),
                 (some, some, some, some, other, other), (some, some, some, some, some, third), (some, some, some, some, other, some)):
        assert launch(*ptrs) == -1, ptrs
        assert lib.bgemm_mi355x_tn_gated_aux(ptrs[0], ptrs[1], ptrs[2], null, null, ptrs[3], ptrs[4], ptrs[5], m, n, k, SILU, null) == -1
    assert launch(some, some, some, some, other, third, ldz=n - 8) == -1
    for act in (0, 5, -1):
        assert launch(some, some, some, some, other, third, act=act) == -1 and aux_answer(lib, act, 0, 1, True, m, n, k, k, k, n, n) == [-1]
    for cid in (-1, 4):
        assert launch(some, some, some, some, other, third, cid=cid) == -1 and lib.bgemm_mi355x_tn_gated_aux_runs(cid, m, n, k, k, k, n, n) == 0
    for shape in ((0, n, k), (m, 0, k), (m, n, 0), (-1, n, k)):
        assert lib.bgemm_mi355x_tn_gated_aux(some, some, some, null, null, some, other, third, *shape, SILU, null) == -1
        assert lib.bgemm_mi355x_tn_gated_aux_runs(0, *shape, k, k, n, n) == 0


# ---- the store text on the CPU ---------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
// hgemm_tn_gated_store.inc (and through it hgemm_tr_store_c16.inc) compiled for the CPU: the device builtins are macros that RECORD a
// store's descriptor base, byte offset and width.  Entered as hgemm_kernel_tn_gated.hpp enters it: outputs 0 and 1 named, C unnamed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "hgemm_dbias.hpp"
#include "hgemm_gated.hpp"
using namespace hgemm_mi355x;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using elem = unsigned short;
constexpr unsigned ARG_NT_STORE = 1;
struct Args { int M, N, ldc, ldz; unsigned flags; elem *C, *G, *U; };
struct Tile { int m0, n0; };
static elem* tn_gated_aux_g(const Args& g) { return g.G; }
static elem* tn_gated_aux_u(const Args& g) { return g.U; }
static int tn_gated_aux_ldz(const Args& g) { return g.ldz; }
struct MockRsrc { const char* base; };
struct MockPair { unsigned v[2]; unsigned operator[](int i) const { return v[i]; } };
struct Store { const char* at; int bytes; };
static std::vector<Store> stores;
#define __amdgpu_buffer_rsrc_t MockRsrc
#define __builtin_amdgcn_make_buffer_rsrc(p, a, b, c) MockRsrc{(const char*)(p)}
#define __builtin_amdgcn_permlane16_swap(a, b, c, d) MockPair{{(a), (b)}}
#define __builtin_amdgcn_sched_barrier(x) ((void)0)
#define __builtin_amdgcn_raw_buffer_store_b128(o, rs, off, s, aux) ((void)(o), stores.push_back(Store{(rs).base + (off), 16}))
#define __builtin_amdgcn_raw_buffer_store_b64(o, rs, off, s, aux) ((void)(o), stores.push_back(Store{(rs).base + (off), 8}))
template <int BM_, int BN_> struct Member { static constexpr int BM = BM_, BN = BN_, TM = BM / 2, TN = BN / 2, FM = TM / 16, FN = TN / 16; };
#define PREAMBLE \
  constexpr int FM = MEMBER::FM, OFN = MEMBER::FN / 2, TN = MEMBER::TN; \
  f32x4 acc[FM][2 * OFN] = {};
template <class MEMBER> static void store_g(const Args& g, Tile tc, int lane, int wave_m, int wave_n) {
  PREAMBLE
#define HGEMM_GATED_STORE_OUTPUT 0
#include "hgemm_tn_gated_store.inc"
#undef HGEMM_GATED_STORE_OUTPUT
}
template <class MEMBER> static void store_u(const Args& g, Tile tc, int lane, int wave_m, int wave_n) {
  PREAMBLE
#define HGEMM_GATED_STORE_OUTPUT 1
#include "hgemm_tn_gated_store.inc"
#undef HGEMM_GATED_STORE_OUTPUT
}
template <class MEMBER> static void store_c(const Args& g, Tile tc, int lane, int wave_m, int wave_n) {
  PREAMBLE
#include "hgemm_tn_gated_store.inc"
}
// every tile, wave and lane of a launch; then every store must lie in ITS matrix at ITS stride and every element be written exactly once
template <class MEMBER> static int walk(int M, int N, bool fused, unsigned flags) {
  const int ldc = N + 16, ldz = fused ? 2 * N + 8 : N + 8;
  std::vector<elem> arena((size_t)(M + 1) * (ldc + 2 * ldz) + 64);
  Args g{M, N, ldc, ldz, flags, arena.data(), nullptr, nullptr};
  g.G = g.C + (size_t)(M + 1) * ldc + 8;
  g.U = fused ? g.G + N : g.G + (size_t)(M + 1) * ldz + 8;
  elem* const base[3] = {g.G, g.U, g.C};
  const int ld[3] = {ldz, ldz, ldc};
  for (int out = 0; out < 3; ++out) {
    stores.clear();
    for (int m0 = 0; m0 < M; m0 += MEMBER::BM)
      for (int n0 = 0; n0 < N; n0 += MEMBER::BN / 2)
        for (int wave = 0; wave < 4; ++wave)
          for (int lane = 0; lane < 64; ++lane) {
            const Tile tc{m0, n0};
            if (out == 0) store_g<MEMBER>(g, tc, lane, wave / 2, wave % 2);
            else if (out == 1) store_u<MEMBER>(g, tc, lane, wave / 2, wave % 2);
            else store_c<MEMBER>(g, tc, lane, wave / 2, wave % 2);
          }
    std::vector<char> seen((size_t)M * N, 0);
    for (const Store& s : stores) {
      const long byte = s.at - (const char*)base[out];
      if (byte < 0 || byte % 2) return 10 + out;
      const long e = byte / 2, m = e / ld[out], n = e % ld[out];
      const int w = s.bytes / 2;
      if (s.bytes != (MEMBER::BN == 128 ? 16 : 8)) return 20 + out;
      if (m >= M || n + w > N) return 30 + out;            // outside the matrix: another row, the pad, or behind the last row
      for (int j = 0; j < w; ++j)
        if (seen[(size_t)m * N + n + j]++) return 40 + out;
    }
    for (char c : seen)
      if (c != 1) return 50 + out;
  }
  return 0;
}
template <int BM, int BN> static int member() {
  for (int N = 8; N <= 3 * (BN / 2) + 8; N += 8)                 // every ragged N over three tiles
    for (int M : {8, BM - 8, BM, BM + 24})
      for (int fused = 0; fused < 2; ++fused)
        for (unsigned flags = 0; flags < 2; ++flags)
          if (const int r = walk<Member<BM, BN>>(M, N, fused != 0, flags)) return r * 1000 + N;
  return 0;
}
int main() {
  printf("store %d %d %d %d\n", member<64, 64>(), member<128, 64>(), member<64, 128>(), member<128, 128>());
  uint32_t b[2];
  const float p = gated_pre(1.5f, 0.25f), q = gated_pre(1.0f, 0x1p-24f);
  memcpy(&b[0], &p, 4);
  memcpy(&b[1], &q, 4);
  printf("pre %08x %08x\n", b[0], b[1]);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    llvm = [Path(HIPCC).resolve().parent.parent / sub / "clang++" for sub in ("llvm/bin", "lib/llvm/bin")]
    cxx = next((str(p) for p in llvm if p.exists()), None) or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no clang++ (the one hipcc drives, or one on PATH): the store text uses clang's vector types and cannot be built for the CPU")
    d = tmp_path_factory.mktemp("gated_aux_cpu")
    (d / "store_main.cpp").write_text(PROGRAM)
    done = subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-Wno-pass-failed", f"-I{CSRC}", str(d / "store_main.cpp"), "-o",
                           str(d / "store_main")], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-3000:]
    run = subprocess.run([str(d / "store_main")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    return run.stdout.splitlines()


def test_every_store_of_every_lane_lies_in_its_own_matrix_at_its_own_stride(program):
    """g_out, u_out (separate at ldz = N + 8, fused at ldz = 2 N + 8) and C (ldc = N + 16), every member, every ragged N over three tiles,
    four M, plain and NT: each store starts inside its own matrix, ends inside the row's N columns, has the member's width, and the stores
    of an output cover its M x N elements exactly once.  A store entered with another output's stride fails here, not on a GPU."""
    assert program[0] == "store 0 0 0 0", program[0]
    assert program[1] == "pre 3fe00000 3f800000", "gated_pre is one fp32 add, round to nearest even"
    kernel = (CSRC / "hgemm_kernel_tn_gated.hpp").read_text()
    assert kernel.count('#include "hgemm_tn_gated_store.inc"') == 3 and "raw_buffer_store" not in kernel, "the kernels store through the one text alone"
    assert re.search(r"#define HGEMM_GATED_STORE_OUTPUT 0\n#include \"hgemm_tn_gated_store.inc\"\n#undef HGEMM_GATED_STORE_OUTPUT\n#define HGEMM_GATED_STORE_OUTPUT 1\n"
                     r"#include \"hgemm_tn_gated_store.inc\"\n#undef HGEMM_GATED_STORE_OUTPUT\n", kernel)


# ---- ISA audit of unit g20 -------------------------------------------------------------------------------------------------------------------
AUX_KERNEL = r"_ZN12hgemm_mi355x25hgemm_tn_gated_aux_kernel\w+"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not available: the audit needs the gfx950 cross-compiler")
    tmp = tmp_path_factory.mktemp("audit_tn_gated_aux")
    out = tmp / "g20.s"
    done = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{CSRC}", f"-I{REPO / 'include'}", "-S", "--cuda-device-only",
                           str(CSRC / "hgemm_inst_g20.hip"), "-o", str(out)], capture_output=True, text=True, timeout=900)
    assert done.returncode == 0, done.stderr[-2000:]
    text = out.read_text()
    meta = {m.group(1): m.group(2) for m in re.finditer(rf"\.amdhsa_kernel ({AUX_KERNEL})\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    funcs = {}
    for m in re.finditer(rf"^({AUX_KERNEL}):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M):
        funcs[m.group(1)] = [c for c in (ln.split(";")[0].strip() for ln in m.group(2).splitlines()) if c and (c.endswith(":") or not c.startswith("."))]
    return (text, funcs, meta), gated_isa(tmp)


def test_unit_g20_holds_the_sixteen_kernels_without_a_private_segment(lib, isa):
    (text, funcs, meta), _ = isa
    assert set(funcs) == set(meta) and len(funcs) == 16
    assert set(re.findall(r"\.amdhsa_kernel (\S+)", text)) == set(meta), "a kernel of another family in the unit (a slab kernel twice)"
    for cid, act in itertools.product(range(4), ACTS):
        md = meta[member_kernel(funcs, cid, act)]
        assert reg(md, "private_segment_fixed_size") == 0, (MEMBERS[cid], act, "private segment")
        assert reg(md, "group_segment_fixed_size") == tn_info(lib, cid)[7], (MEMBERS[cid], act, "LDS bytes")
    assert not re.search(r"^\s*scratch_", text, re.M)


def test_the_k_loop_is_the_gated_twins_and_the_registers_are_within_them(isa):
    """Per stage the MFMA, ds_read_b128, LDS-DMA and barrier counts of the member's gated kernel of the same activation in unit g18;
    next_free_vgpr at most the twin's; behind the loop FN 8-byte bias loads, three times the twin's conversions to bf16 and three times its
    stores, all of the member's width.  Prints the register table."""
    (_, funcs, meta), (_, funcs18, meta18) = isa
    print("member act accum_offset next_free_vgpr | twin accum_offset next_free_vgpr")
    for cid in range(4):
        bm, bn = TILES[cid]
        fm, fn = bm // 32, bn // 32
        for act in ACTS:
            name, twin = member_kernel(funcs, cid, act), member_kernel(funcs18, cid, act)
            codes, tcodes = funcs[name], funcs18[twin]
            (lo, hi), (tlo, thi) = k_loop(name, codes), k_loop(twin, tcodes)
            body, tbody = codes[lo:hi + 1], tcodes[tlo:thi + 1]
            for prefix in ("v_mfma_f32_16x16x32_bf16", "ds_read_b128", "buffer_load_dwordx4", "s_barrier"):
                mine, his = (sum(1 for c in seq if c.startswith(prefix)) for seq in (body, tbody))
                assert mine == his, (name, prefix, mine, his)
            assert sum(1 for c in body if c.startswith("v_mfma")) == 2 * fm * fn and sum(1 for c in body if c.startswith("ds_read_b128")) == 2 * (fm + fn)
            assert not any(c.startswith(("v_mfma", "ds_read")) for c in codes[:lo] + codes[hi + 1:]), name
            print(MEMBERS[cid], {1: "relu", 2: "gelu", 3: "gelu_tanh", 4: "silu"}[act], reg(meta[name], "accum_offset"), reg(meta[name], "next_free_vgpr"), "|",
                  reg(meta18[twin], "accum_offset"), reg(meta18[twin], "next_free_vgpr"))
            assert reg(meta[name], "next_free_vgpr") <= reg(meta18[twin], "next_free_vgpr"), (name, "next_free_vgpr above the gated twin's")
            tail, ttail = codes[hi + 1:], tcodes[thi + 1:]
            assert sum(1 for c in tail if c.startswith("buffer_load_dwordx2")) == fn and not any(c.startswith("buffer_load_dwordx2") for c in codes[:hi + 1]), name
            assert sum(1 for c in tail if c.startswith("v_cvt_pk_bf16_f32")) == 3 * fm * fn == 3 * sum(1 for c in ttail if c.startswith("v_cvt_pk_bf16_f32")), name
            stores, tstores = ([c for c in t if c.startswith(("buffer_store", "global_store", "flat_store"))] for t in (tail, ttail))
            want = "buffer_store_dwordx4" if bn == 128 else "buffer_store_dwordx2"
            assert len(stores) == 3 * len(tstores) and all(c.startswith(want) for c in stores), (name, "the stores of the three outputs")
