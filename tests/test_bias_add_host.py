"""CPU tests of the fused residual add, bgemm_mi355x_tn_bias_add (family f, hgemm_inst_g21.hip, the kind TR_C16_BIAS_ADD) and bgemm_mi355x_nn_add
(family n, hgemm_inst_g22.hip, TR_C16_ADD): the names, the constants and the header blocks; the self-check hooks against the parent call of
the same arguments; _runs against the scope rules; the refusals; an audit of both units by counting, against their bias / dact twins and the
EPI_C16 kernels; and the evidence that the GPU tests' bit-for-bit comparison sees each mistake, computed from the reference data alone."""
import concurrent.futures as cf
import ctypes
import itertools
import re
from pathlib import Path

import pytest

import residual_common as rc
from residual_common import EPI_C16_ADD, EPI_C16_BIAS_ADD
from test_mlp_backward_host import NN_KERNEL, TN_KERNEL, device_isa, k_loop, kernel_of, mnemonics, nn_answer, reg, with_epi
from test_nn_host import MEMBERS as NN_MEMBERS, nn_info
from test_ta_host import CSRC, HIPCC, PKG, REPO
from test_ta_host import lib as ta_lib  # noqa: F401  (fixture: the built library)
from test_tn_bf16_host import EPI_C16, EPI_SLAB, FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, MEMBERS as TN_MEMBERS, TILES, WORDS, tn_info
from test_tn_bf16_host import lib  # noqa: F401  (fixture: the library with the prototypes)
from test_tn_bias_host import EPI_C16_BIAS, SHAPES

EPI_C16_DACT_RELU = 12
PUBLIC = ("bgemm_mi355x_tn_bias_add", "bgemm_mi355x_launch_tn_bias_add", "bgemm_mi355x_tn_bias_add_runs", "bgemm_mi355x_nn_add", "bgemm_mi355x_launch_nn_add",
          "bgemm_mi355x_nn_add_runs")
HOOKS = ("bgemm_mi355x_selfcheck_launch_tn_bias_add", "bgemm_mi355x_selfcheck_launch_nn_add", "bgemm_mi355x_selfcheck_launch_nn_bias_add",
         "bgemm_mi355x_selfcheck_launch_tn_add")


def answer(lib, hook, cid, word, aligned, m, n, k, lda, ldb, ldc, ldr, ruled_out=0):
    out = (ctypes.c_longlong * 20)()
    st = getattr(lib, hook)(cid, word, 4 if aligned else 0, m, n, k, lda, ldb, ldc, ldr, ruled_out, out)
    return [st] if st != 0 else [0] + list(out[:4]) + [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def bias_answer(lib, cid, word, aligned, m, n, k, lda, ldb, ldc, ruled_out=0):
    out = (ctypes.c_longlong * 20)()
    st = lib.bgemm_mi355x_selfcheck_launch_tn_bias(cid, word, 4 if aligned else 0, m, n, k, lda, ldb, ldc, ruled_out, out)
    return [st] if st != 0 else [0] + list(out[:4]) + [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def test_the_names_the_constants_the_units_and_the_header_blocks(lib):
    header = (REPO / "include" / "hgemm_mi355x.h").read_text()
    for nm in PUBLIC:
        assert re.search(rf"\b{nm}\(", header), f"{nm} is not declared in include/hgemm_mi355x.h"
        assert getattr(lib, nm) is not None
    for hook in HOOKS:
        assert getattr(lib, hook) is not None and hook not in header
    for nm in ("hgemm_mi355x_nn_add", "bgemm_mi355x_ta_add", "bgemm_mi355x_tn_add", "bgemm_mi355x_nn_bias_add", "bgemm_mi355x_tn_bias_act_add", "bgemm_mi355x_tn_gated_add",
               "bgemm_mi355x_tn_bias_add_plan", "bgemm_mi355x_nn_add_reserve_workspace"):
        assert not hasattr(lib, nm), nm                                       # no fp16, activation, TA or gated form; no second plan or workspace call
    flat = lambda a, b: re.sub(r"\s*\n \*\s*", " ", header[header.index(a):header.index(b)])   # noqa: E731
    block = flat("Forward product with a fused bias and residual add", "int bgemm_mi355x_tn_bias_add(")
    for words in ("= fl32( S[m][n] + float(bias[n]) )", "C[m][n] = bf16_rne( fl32( z + float(r[m][n]) ) )", "Two fp32 adds IN THIS ORDER, then one rounding",
                  "Nothing is added to a slab", "bias == NULL means a vector of +0.0, bit for bit", "for z = -0 this call gives +0",
                  "r == c with ldr == ldc is allowed and defined", "computed from the OLD r[m][n]", "r == c with ldr != ldc: HGEMM_ERR_BAD_ARG",
                  "ldr >= N (less: HGEMM_ERR_BAD_ARG)", "16-byte aligned, ldr % 8 == 0 and (BM ldr + N) 2 bytes below 2 GiB", "ends at its last valid element",
                  "a captured split call without a workspace runs unsplit, status 0, and allocates nothing", "beta other than 1"):
        assert words in block, words
    block = flat("Input gradient with a fused residual add", "int bgemm_mi355x_nn_add(")
    for words in ("C[m][n] = bf16_rne( fl32( S[m][n] + float(r[m][n]) ) )", "ONE fp32 add on the finished sum, then one rounding", "Nothing is added to a slab",
                  "There is no bias", "r == c needs ldr == ldc", "bgemm_mi355x_launch_nn call with the same arguments"):
        assert words in block, words
    assert "bgemm_mi355x_tn_bias_add and bgemm_mi355x_nn_add" in header[:header.index("#ifndef HGEMM_MI355X_H_")], "the first paragraph names the two beta = 1 calls"
    build_py = (PKG / "build.py").read_text()
    assert "hgemm_inst_g21.hip" in build_py and "hgemm_inst_g22.hip" in build_py
    g21, g22 = (CSRC / "hgemm_inst_g21.hip").read_text(), (CSRC / "hgemm_inst_g22.hip").read_text()
    assert "HGEMM_TR_MEMBERS(HGEMM_TN_ADD_INST, CfgTNB)" in g21 and "HGEMM_TR_MEMBERS(HGEMM_NN_ADD_INST, CfgNNB)" in g22
    assert "SLAB" not in g21 + g22, "the K slices are the 16-bit sets' slab kernels: not instantiated again"
    assert f"constexpr int EPI_C16_BIAS_ADD = {EPI_C16_BIAS_ADD}, EPI_C16_ADD = {EPI_C16_ADD};" in (CSRC / "hgemm_kernel.hpp").read_text()
    assert not (EPI_C16_BIAS_ADD & 24) and not (EPI_C16_ADD & 24), "neither flag bit (EPI_KTAIL, EPI_KSTAGGER) is set"
    # the add text stands once, in hgemm_residual.hpp, and kernel, combine and reference use it
    residual = (CSRC / "hgemm_residual.hpp").read_text()
    assert "float residual_add(float s, float r) { return s + r; }" in residual
    assert "float bias_residual_add(float s, float bias, float r) { return residual_add(s + bias, r); }" in residual
    for src, fn in (("hgemm_kernel_tn.hpp", "bias_residual_add("), ("hgemm_kernel_nn.hpp", "residual_add("), ("hgemm_registry.hip", "bias_residual_add("),
                    ("hgemm_registry.hip", "s[i] = residual_add(")):
        assert fn in (CSRC / src).read_text(), (src, fn)
    # both kernels reuse the dact range: no byte behind r's last valid element
    for src in ("hgemm_kernel_tn.hpp", "hgemm_kernel_nn.hpp"):
        assert "const uint32_t r_bytes = dact_z_range_bytes(g.M, g.N, g.tail_first, tc.m0);" in (CSRC / src).read_text(), src


def test_the_hooks_answer_as_the_parent_call_of_the_same_arguments_over_the_sweep(lib):
    """Every (member, shape, plan word, stride set, aligned / misaligned / no workspace): the parent call's answer with its epi id replaced by the
    add kind's in the plain dispatch and in the combine dispatch -- the same tiles, cuts and slabs; an ldr outside r's rules sends the call to the
    reference kernel and changes nothing else.  _runs agrees with the hook."""
    seen = set()
    for cid, (m, n, k), word in itertools.product(range(4), SHAPES, WORDS):
        for lda, ldc, ldr, pad_b in ((k, n, n, 0), (k + 8, n + 16, n + 24, 16), (k, n, n + 4, 0), (k, n + 4, n, 0), (k + 4, n, n, 0)):
            for aligned, ruled_out in ((True, 0), (False, 0), (True, 1 << FORM_SPLITK)):
                for hook, parent, ldb, epi_parent, epi_new in (
                        ("bgemm_mi355x_selfcheck_launch_tn_bias_add", bias_answer, k + pad_b, EPI_C16_BIAS, EPI_C16_BIAS_ADD),
                        ("bgemm_mi355x_selfcheck_launch_nn_add", nn_answer, n + pad_b, EPI_C16, EPI_C16_ADD)):
                    twin = parent(lib, cid, word, aligned and ldr % 8 == 0, m, n, k, lda, ldb, ldc, ruled_out)
                    # (the plain NN call's combine dispatch carries EPI_SLAB, the add call's its own id: with_epi)
                    want = with_epi(twin, epi_new) if epi_parent == EPI_C16 else twin[:5] + [(t, g, epi_new if e == epi_parent else e, s, kc) for t, g, e, s, kc in twin[5:]]
                    got = answer(lib, hook, cid, word, aligned, m, n, k, lda, ldb, ldc, ldr, ruled_out)
                    assert got == want, (hook, cid, (m, n, k), hex(word), (lda, ldb, ldc, ldr), aligned, ruled_out)
                    epis = tuple(d[2] for d in got[5:])
                    assert epis.count(epi_new) == 1 and EPI_C16 not in epis
                    seen.add((epi_new, got[1], epis))
            for runs, hook, ldb in ((lib.bgemm_mi355x_tn_bias_add_runs, "bgemm_mi355x_selfcheck_launch_tn_bias_add", k + pad_b),
                                    (lib.bgemm_mi355x_nn_add_runs, "bgemm_mi355x_selfcheck_launch_nn_add", n + pad_b)):
                assert runs(cid, m, n, k, lda, ldb, ldc, ldr) == (1 if answer(lib, hook, cid, 1, True, m, n, k, lda, ldb, ldc, ldr)[1] != FORM_REFERENCE else 0)
    assert seen == {(e, form, epis) for e in (EPI_C16_BIAS_ADD, EPI_C16_ADD) for form, epis in ((FORM_REFERENCE, (e,)), (FORM_PLAIN, (e,)), (FORM_SPLITK, (EPI_SLAB, e)))}
    # the layouts without the kind refuse it
    out = (ctypes.c_longlong * 20)()
    assert lib.bgemm_mi355x_selfcheck_launch_nn_bias_add(0, 1, 4, 64, 64, 64, 64, 64, 64, 64, 0, out) == -1
    assert lib.bgemm_mi355x_selfcheck_launch_tn_add(0, 1, 4, 64, 64, 64, 64, 64, 64, 64, 0, out) == -1


def test_runs_follows_the_scope_rules(lib):
    m, n, k = 200, 136, 128
    for runs, parent, ldb in ((lib.bgemm_mi355x_tn_bias_add_runs, lib.bgemm_mi355x_tn_bias_runs, k), (lib.bgemm_mi355x_nn_add_runs, lib.bgemm_mi355x_nn_runs, n)):
        assert runs(0, m, n, k, k, ldb, n, n) == 1 and parent(0, m, n, k, k, ldb, n) == 1
        assert runs(0, m, n, k, k, ldb, n, n + 8) == 1 and runs(0, m, n, k, k, ldb, n + 8, n) == 1          # ldr != ldc is in scope
        for shape, lds in (((m, n + 4, k), (k, ldb + 8, n + 8, n + 8)),      # N % 8 == 4
                           ((m, n, k + 8), (k + 8, ldb + 8, n, n)),         # K % 64 != 0
                           ((m, n, k), (k + 4, ldb, n, n)), ((m, n, k), (k, ldb + 4, n, n)), ((m, n, k), (k, ldb, n + 4, n)), ((m, n, k), (k, ldb, n, n + 4)),   # a stride % 8 == 4
                           ((m, n, k), (k, ldb, n, n - 8)), ((m, n, k), (k, ldb, n - 8, n)),     # refused by the launch: 0 here
                           ((m, n, k), (k, ldb, n, 1 << 24)), ((m, n, k), (k, ldb, 1 << 24, n))):   # (BM ld + N) 2 >= 2 GiB at BM = 64
            assert runs(0, *shape, *lds) == 0, (shape, lds)
        assert runs(0, m, n, k, k, ldb, n, (1 << 24) - 8) == 1
        assert runs(3, m, n, k, k, ldb, n, 1 << 23) == 0 and runs(0, m, n, k, k, ldb, n, 1 << 23) == 1   # BM = 128 against 64
        for cid in (-1, 4):
            assert runs(cid, m, n, k, k, ldb, n, n) == 0


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    rc.prototypes(lib)
    m, n, k = 200, 136, 128
    vp = ctypes.c_void_p
    null = vp(0)
    a, b, bias, r, c = (vp(4096 * (i + 1)) for i in range(5))
    tn = lambda ptrs, lds=(k, k, n, n), cid=0: lib.bgemm_mi355x_launch_tn_bias_add(cid, 1, *ptrs, m, n, k, *lds, null)   # noqa: E731
    nn = lambda ptrs, lds=(k, n, n, n), cid=0: lib.bgemm_mi355x_launch_nn_add(cid, 1, *ptrs, m, n, k, *lds, null)         # noqa: E731
    for i in (0, 1, 3, 4):                                                    # a NULL a, b, r or c (a NULL bias is +0.0: no refusal)
        ptrs = [a, b, bias, r, c]
        ptrs[i] = null
        assert tn(ptrs) == -1 and lib.bgemm_mi355x_tn_bias_add(*ptrs, m, n, k, null) == -1, i
    for i in range(4):
        ptrs = [a, b, r, c]
        ptrs[i] = null
        assert nn(ptrs) == -1 and lib.bgemm_mi355x_nn_add(*ptrs, m, n, k, null) == -1, i
    assert tn((a, b, bias, c, c), (k, k, n + 8, n)) == -1 and tn((a, b, bias, c, c), (k, k, n, n + 8)) == -1        # r == c with ldr != ldc
    assert nn((a, b, c, c), (k, n, n + 8, n)) == -1 and nn((a, b, c, c), (k, n, n, n + 8)) == -1
    for lds in ((k - 8, k, n, n), (k, k - 8, n, n), (k, k, n - 8, n), (k, k, n, n - 8)):
        assert tn((a, b, bias, r, c), lds) == -1, lds
    for lds in ((k - 8, n, n, n), (k, n - 8, n, n), (k, n, n - 8, n), (k, n, n, n - 8)):
        assert nn((a, b, r, c), lds) == -1, lds
    for cid in (-1, 4):
        assert tn((a, b, bias, r, c), cid=cid) == -1 and nn((a, b, r, c), cid=cid) == -1
    for dims in ((0, n, k), (m, 0, k), (m, n, 0)):
        assert lib.bgemm_mi355x_launch_tn_bias_add(0, 1, a, b, bias, r, c, *dims, k, k, n, n, null) == -1
        assert lib.bgemm_mi355x_launch_nn_add(0, 1, a, b, r, c, *dims, k, n, n, n, null) == -1


# ---- the evidence that a bit-for-bit comparison sees each mistake, from the reference data alone (DESIGN.md 4.35 records the counts) ----------
@pytest.mark.parametrize("shape", [s for s in rc.SHAPES if s[0] * s[1] >= 2048], ids=lambda s: "x".join(map(str, s)))
def test_each_wrong_variant_differs_from_the_expectation_on_its_floor_of_the_outputs(shape):
    m, n, k = shape
    ops = rc.Ops(*shape)
    for kind in ("tn", "nn"):
        expect = rc.want(kind, ops)
        for name, wrong in rc.wrong_variants(ops, kind).items():
            count = rc.differing(wrong, expect)
            if name == "order of the adds":
                assert count == 0, "on the random data every sum is exact: the order of the adds is invisible"
                continue
            print(f"{kind} {shape} {name}: {count} of {m * n} differ (floor {rc.FLOOR[name]})")
            assert count >= rc.FLOOR[name] * m * n, (kind, name, count)
    order = rc.Ops(*shape, data="order")
    count = rc.differing(rc.wrong_variants(order, "tn")["order of the adds"], rc.want("tn", order))
    print(f"tn {shape} order of the adds, the order data: {count} of {m * n} differ (floor {rc.FLOOR['order of the adds']})")
    assert count >= rc.FLOOR["order of the adds"] * m * n


def test_a_null_bias_is_not_a_dropped_add_of_minus_zero():
    """z = S + (+0.0) turns a -0 sum into +0; the expectation adds the zero like any other value."""
    import torch

    s = torch.tensor([-0.0, 0.0, 1.5])
    r = torch.tensor([-0.0, -0.0, -0.0]).bfloat16()
    got = rc.want_bias_add(s, torch.zeros(3, dtype=torch.bfloat16), r)
    assert rc.bits(got).tolist() == [0, 0, rc.bits(torch.tensor([1.5]).bfloat16()).item()]
    assert rc.bits(rc.want_add(s, r)).tolist()[0] == -32768                        # (-0) + (-0) = -0 without the bias add


# ---- audit of units g21 and g22 against their twins, by counting -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not available: the audit needs the gfx950 cross-compiler")
    tmp = tmp_path_factory.mktemp("audit_bias_add")
    with cf.ThreadPoolExecutor(max_workers=3) as ex:
        jobs = {u: ex.submit(device_isa, tmp, u, kk) for u, kk in (("g21", TN_KERNEL), ("g12", TN_KERNEL), ("g11", TN_KERNEL), ("g22", NN_KERNEL), ("g16", NN_KERNEL),
                                                                   ("g8", NN_KERNEL))}
        return {u: j.result() for u, j in jobs.items()}


@pytest.mark.parametrize("unit", ["g21", "g22"])
def test_the_new_units_hold_four_kernels_without_a_private_segment_with_their_twins_registers_and_k_loop(lib, isa, unit):
    """g21 against the EPI_C16_BIAS twins of g12 and the EPI_C16 kernels of g11, g22 against the EPI_C16_DACT + ReLU twins of g16 and the EPI_C16
    kernels of g8: no private segment, the member's LDS, next_free_vgpr equal to the bias / dact twin's, and a K loop with the EPI_C16 kernel's
    instructions by mnemonic and count and its counted vmcnt -- the r loads (and the bias loads) stand behind it."""
    twin_unit, plain_unit, cfg, epi, twin_epi, info, names = (("g12", "g11", "CfgTNB", EPI_C16_BIAS_ADD, EPI_C16_BIAS, tn_info, TN_MEMBERS) if unit == "g21" else
                                                              ("g16", "g8", "CfgNNB", EPI_C16_ADD, EPI_C16_DACT_RELU, nn_info, NN_MEMBERS))
    (text, funcs, meta), (_, _, tmeta), (_, pfuncs, _) = isa[unit], isa[twin_unit], isa[plain_unit]
    assert set(funcs) == set(meta) and len(funcs) == 4
    assert set(re.findall(r"\.amdhsa_kernel (\S+)", text)) == set(meta), "a kernel of another family, element type or epilogue in the unit"
    assert not re.search(r"^\s*scratch_", text, re.M)
    print("member accum_offset next_free_vgpr next_free_sgpr | twin")
    for cid in range(4):
        name = kernel_of(funcs, cfg, cid, epi)
        twin = kernel_of(tmeta, cfg, cid, twin_epi)
        plain = kernel_of(pfuncs, cfg, cid, EPI_C16)
        md = meta[name]
        print(names[cid], *(reg(md, kk) for kk in ("accum_offset", "next_free_vgpr", "next_free_sgpr")), "|",
              *(reg(tmeta[twin], kk) for kk in ("accum_offset", "next_free_vgpr", "next_free_sgpr")))
        assert reg(md, "private_segment_fixed_size") == 0, (name, "private segment: the epilogue spills")
        assert reg(md, "group_segment_fixed_size") == info(lib, cid)[7], (name, "LDS bytes")
        assert reg(md, "next_free_vgpr") == reg(tmeta[twin], "next_free_vgpr"), (name, "occupancy differs from the twin's")
        codes, pcodes = funcs[name], pfuncs[plain]
        (lo, hi), (plo, phi) = k_loop(name, codes), k_loop(plain, pcodes)
        body, pbody = codes[lo:hi + 1], pcodes[plo:phi + 1]
        assert mnemonics(body) == mnemonics(pbody), (name, "the K loop differs from the EPI_C16 kernel's")
        bm, bn = TILES[cid]
        fm, fn = bm // 32, bn // 32
        assert sum(1 for c in body if c.startswith("v_mfma")) == 2 * fm * fn and sum(1 for c in body if c.startswith("s_barrier")) == 1
        assert [c for c in body if c.startswith("s_waitcnt vmcnt")] == [c for c in pbody if c.startswith("s_waitcnt vmcnt")], (name, "the counted vmcnt")
        tail = codes[hi + 1:]
        loads = fm * fn + (fn if unit == "g21" else 0)                         # one 8-byte load of r per fragment, and of the bias per column tile
        assert sum(1 for c in tail if c.startswith("buffer_load_dwordx2")) == loads and not any(c.startswith("buffer_load_dwordx2") for c in codes[:hi + 1]), name
        assert sum(1 for c in tail if c.startswith("v_cvt_pk_bf16_f32")) == 2 * fm * fn, name
        stores = [c for c in tail if c.startswith(("buffer_store", "global_store", "flat_store"))]
        assert stores and all(c.startswith("buffer_store_dwordx4") for c in stores), (name, "the 16-byte stores")
        assert not any(c.startswith(("v_mfma", "ds_read")) for c in tail), name
        # in place: every load of r stands in front of the first store
        first_store = min(i for i, c in enumerate(tail) if c.startswith("buffer_store"))
        assert not any(c.startswith("buffer_load") for c in tail[first_store:]), (name, "a load of r behind a store")
