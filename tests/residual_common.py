"""What the tests of the fused residual add share (bgemm_mi355x_tn_bias_add, bgemm_mi355x_nn_add): the operands, the expectation computed by
torch on the CPU, the deliberately wrong variants, and the one GPU call runner.  No test lives here.

Operands (tests/test_gpu_nn_dgated.py's Ops): A and B hold integers of [-15, 15], A scaled by 2^-9, so the finished sum S is a multiple of 2^-9
below 2^9 and exact in fp32 in any summation order.  With a bf16 bias and a bf16 r the whole result is then defined BIT FOR BIT by two IEEE
fp32 adds and one rounding: ((s + bias.float()) + r.float()).bfloat16().  Every comparison is on bits; nothing here has a tolerance."""
import ctypes

import numpy as np
import torch

SHAPES = ((64, 32, 64), (8, 8, 64), (136, 72, 128), (152, 152, 320))
NT = 0x20000                                                   # HGEMM_PLAN_NT_STORE
WORDS = (1, 1 | NT, 2, 5)                                      # plain, NT store, 2 and 5 two-pass splits (clamped to K / 64)
SEED = 7
EPI_C16_BIAS_ADD, EPI_C16_ADD = 160, 161
FORM_REFERENCE, FORM_SPLITK, FORM_PLAIN = 0, 3, 6            # hgemm_api.hip: enum Form
OUT_FILL = -3.0 * 2.0 ** -12                                  # prefill of everything an output buffer holds besides its M x N elements
HOOKS = {"tn": "bgemm_mi355x_selfcheck_launch_tn_bias_add", "nn": "bgemm_mi355x_selfcheck_launch_nn_add"}
# The share of the outputs on which each wrong variant must differ from the expectation (shapes with >= 2048 outputs); the measured counts
# are in DESIGN.md 4.35 and are recomputed by tests/test_bias_add_host.py from this data alone.
FLOOR = {"z rounded to bf16 first": 0.10, "S rounded to bf16 first": 0.10, "r dropped": 0.90, "bias dropped": 0.90, "order of the adds": 0.15}


class Ops:
    """A [M][K], B [K][N] (bt: [N][K]), bias [N], r [M][N] on the CPU, and S exactly.  data = "random": bias N(0, 1), r 4 N(0, 1), both bf16.
    data = "order": bias[n] = +-2^16 (1 + (n mod 128) / 128), the sign alternating in n, and r[m][n] = -bias[n] -- (S + bias) + r loses S's
    low bits, S + (bias + r) does not."""

    def __init__(self, m, n, k, seed=SEED, data="random"):
        rng = np.random.default_rng(seed)
        ai, bi = rng.integers(-15, 16, size=(m, k)), rng.integers(-15, 16, size=(k, n))
        self.m, self.n, self.k = m, n, k
        self.a = torch.from_numpy(ai * 2.0 ** -9).bfloat16()
        self.b = torch.from_numpy(bi.astype(np.float64)).bfloat16()
        self.bt = self.b.t().contiguous()
        self.s = torch.from_numpy((ai @ bi) * 2.0 ** -9).float()                  # exact: integers below 2^18
        assert float(self.s.abs().max()) < 2.0 ** 9 and torch.equal(self.s.double(), self.a.double() @ self.b.double())
        if data == "random":
            self.bias = torch.from_numpy(rng.standard_normal(n)).bfloat16()
            self.r = torch.from_numpy(4.0 * rng.standard_normal((m, n))).bfloat16()
        else:
            j = torch.arange(n)
            bias64 = 2.0 ** 16 * (1.0 + (j % 128).double() / 128.0) * torch.where(j % 2 == 0, 1.0, -1.0).double()
            self.bias = bias64.bfloat16()
            assert torch.equal(self.bias.double(), bias64), "the order data's bias is a bf16 vector"
            self.r = (-self.bias).expand(m, n).contiguous()


def want_bias_add(s, bias, r):
    """bgemm_mi355x_tn_bias_add, bit for bit: z = fl32(S + bias), fl32(z + r), one rounding"""
    return ((s.float() + bias.float()) + r.float()).bfloat16()


def want_add(s, r):
    """bgemm_mi355x_nn_add, bit for bit"""
    return (s.float() + r.float()).bfloat16()


def wrong_variants(ops, kind):
    """name -> a result a mistaken implementation would give, from the reference data alone"""
    s, b, r = ops.s, ops.bias.float(), ops.r.float()
    if kind == "nn":
        return {"S rounded to bf16 first": (s.bfloat16().float() + r).bfloat16(), "r dropped": s.bfloat16()}
    return {"z rounded to bf16 first": ((s + b).bfloat16().float() + r).bfloat16(),
            "S rounded to bf16 first": ((s.bfloat16().float() + b) + r).bfloat16(),
            "r dropped": (s + b).bfloat16(), "bias dropped": (s + r).bfloat16(),
            "order of the adds": (s + (b + r)).bfloat16()}


def bits(t):
    return t.contiguous().view(torch.int16)


def differing(a, b):
    return int((bits(a) != bits(b)).sum())


# ---- the GPU side ----------------------------------------------------------------------------------------------------------------------------
def prototypes(lib):
    p, i = ctypes.c_void_p, ctypes.c_int
    lib.bgemm_mi355x_launch_tn_bias_add.argtypes = [i] * 2 + [p] * 5 + [i] * 7 + [p]
    lib.bgemm_mi355x_tn_bias_add.argtypes = [p] * 5 + [i] * 3 + [p]
    lib.bgemm_mi355x_launch_nn_add.argtypes = [i] * 2 + [p] * 4 + [i] * 7 + [p]
    lib.bgemm_mi355x_nn_add.argtypes = [p] * 4 + [i] * 3 + [p]
    return lib


def place(x, ld, off=0, fill=float("nan")):
    """x [rows][cols] (cpu) at row stride ld in a device buffer of `fill`, `off` elements behind the buffer's aligned start: (flat, view)"""
    rows, cols = x.shape
    flat = torch.full((rows * ld + 8,), fill, dtype=x.dtype, device="cuda")
    view = flat[off:off + rows * ld].view(rows, ld)
    view[:, :cols] = x.cuda()
    return flat, view


def decision(lib, kind, cfg, word, m, n, k, lda, ldb, ldc, ldr, aligned=True, ruled_out=0):
    out = (ctypes.c_longlong * 20)()
    st = getattr(lib, HOOKS[kind])(cfg, word, 4 if aligned else 0, m, n, k, lda, ldb, ldc, ldr, ruled_out, out)
    return st, out[0], [tuple(out[4 + 8 * i:9 + 8 * i]) for i in range(out[1])]


def run(lib, kind, ops, cfg, word, lds=None, inplace=False, bias="vector", off_r=0, want_form=None, planned=False, stream=0, what=""):
    """One call of bgemm_mi355x_launch_tn_bias_add (kind "tn") or bgemm_mi355x_launch_nn_add ("nn"); lds = (lda, ldb, ldc, ldr).  The output
    starts as NaN inside and OUT_FILL outside its M x N elements -- in place (r == c, ldr == ldc) it starts as r inside --; the outside and every
    input must come back unchanged.  bias: "vector", "zeros" or "null" (tn).  off_r: r moved by that many elements (out of scope).  -> C (cpu)"""
    m, n, k = ops.m, ops.n, ops.k
    b_op = ops.bt if kind == "tn" else ops.b
    lda, ldb, ldc, ldr = lds or (k, b_op.shape[1], n, n)
    if inplace:
        assert ldr == ldc and not off_r
    aligned = not off_r and not ((lda | ldb | ldc | ldr) & 7)
    if want_form is not None:
        st, form, disp = decision(lib, kind, cfg, word, m, n, k, lda, ldb, ldc, ldr, aligned)
        assert (st, form) == (0, want_form), (what, st, form, disp)
    keep = [place(ops.a, lda), place(b_op, ldb)]
    if kind == "tn" and bias != "null":
        vec = ops.bias if bias == "vector" else torch.zeros(n, dtype=torch.bfloat16)
        keep.append(place(vec.view(1, n), n))
    p_bias = keep[2][0].data_ptr() if len(keep) == 3 else None
    if inplace:
        out = place(ops.r, ldc, fill=OUT_FILL)
        p_r = out[0].data_ptr()
    else:
        out = place(torch.full((m, n), float("nan"), dtype=torch.bfloat16), ldc, fill=OUT_FILL)
        keep.append(place(ops.r, ldr, off_r))
        p_r = keep[-1][0].data_ptr() + 2 * off_r
    before, inputs = out[0].clone(), [flat.clone() for flat, _ in keep]
    pa, pb, pc = keep[0][0].data_ptr(), keep[1][0].data_ptr(), out[0].data_ptr()
    if kind == "tn":
        st = (lib.bgemm_mi355x_tn_bias_add(pa, pb, p_bias, p_r, pc, m, n, k, stream) if planned else
              lib.bgemm_mi355x_launch_tn_bias_add(cfg, word, pa, pb, p_bias, p_r, pc, m, n, k, lda, ldb, ldc, ldr, stream))
    else:
        st = (lib.bgemm_mi355x_nn_add(pa, pb, p_r, pc, m, n, k, stream) if planned else
              lib.bgemm_mi355x_launch_nn_add(cfg, word, pa, pb, p_r, pc, m, n, k, lda, ldb, ldc, ldr, stream))
    torch.cuda.synchronize()
    assert st == 0, (what, st)
    got = out[1][:, :n].cpu().clone()
    out[1][:, :n] = 0
    before[:m * ldc].view(m, ldc)[:, :n] = 0
    assert torch.equal(bits(out[0]), bits(before)), f"{what}: the output was written outside its M x N elements"
    assert all(torch.equal(bits(flat), bits(was)) for (flat, _), was in zip(keep, inputs)), f"{what}: an input changed"
    return got


def want(kind, ops, bias="vector"):
    if kind == "nn":
        return want_add(ops.s, ops.r)
    return want_bias_add(ops.s, ops.bias if bias == "vector" else torch.zeros(ops.n, dtype=torch.bfloat16), ops.r)
