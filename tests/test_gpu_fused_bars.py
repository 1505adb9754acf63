"""GPU tests that hold the eight calls with a second M x N matrix (or a second weight) behind a buffer descriptor of its own to the reach,
raster and K-ladder bars families n, a and f are held to for A, B and C (tests/test_gpu_nn_bars.py, tests/test_gpu_tn_bars.py): CALLS below
has a row per call.  Run with `-m gpu` on an MI355X; tests/test_fused_bars_host.py shows on the CPU that this data tells mistakes apart.

Operands (residual_common.Ops' manner): A holds integers of [-15, 15] scaled by 2^-9, every weight integers of [-15, 15], so each finished
sum S is a whole number of 2^-9 below 2^15 of them and exact in fp32 in any order and grouping.  The activation is ReLU throughout (a
select), so every output is defined BIT FOR BIT by IEEE fp32 operations and one bf16 rounding, which torch computes on the CPU (`expect`).
The second matrices z / g / u / r are random bf16 of both signs, never zero, different at every position: a descriptor range that is too
short (reads return 0) and a displaced read both show.  The biases are pairwise distinct over N.

1. The reach rules of the second matrices (z_ok of tr_resolve_gemm, the gated weight rule of TrLayout::reach_ok), executed on both sides
   of the edge: the member kernel, plain and in 2 splits, at the largest stride it takes, the reference kernel at the next multiple of 8.
2. The clamped descriptor range (dact_z_range_bytes): a second matrix of 4.6 GB.
3. Rasters of more than eight tile rows: every call, member and store word at 1160 x 136 x 128.
4. The K ladder, 1 to 7 stages, and 127 stages: every stage count modulo 3 and 4 behind the fused epilogues' loads.

Every comparison is on bits and unmasked.  Outputs start as NaN inside their M x N window and as a sentinel outside, input padding is
NaN; after each launch every buffer must be bit-unchanged outside its windows (big buffers in chunks) and every input inside them.
Before each launch the call's selfcheck hook must report the form the test is about."""
import ctypes
import functools
import time
from collections import namedtuple

import numpy as np
import pytest
import torch

from residual_common import FORM_PLAIN, FORM_REFERENCE, FORM_SPLITK, NT, OUT_FILL
from test_gpu_dbias import EPI_DBIAS, RELU
from test_gpu_nn import MEMBERS as NN_MEMBERS
from test_gpu_nn import g  # noqa: F401  (fixture: the GPU helpers)
from test_gpu_ta import GIB
from test_gpu_tn_bars import all_same_bits, largest_stride
from test_gpu_tn_bf16 import MEMBERS as TN_MEMBERS
from test_gpu_tr_bf16 import ibits as bits

pytestmark = pytest.mark.gpu

TILES = ((64, 64), (128, 64), (64, 128), (128, 128))            # (BM, BN) of config ids 0 .. 3 of both families; asserted in `L`
BK = 64
DB_SENTINEL = -12345.625

# ---- the table: one row per call ---------------------------------------------------------------------------------------------------------
# args: the pointer arguments of bgemm_mi355x_launch_<name> in order; strides: its stride arguments in order (z: ldz / ldr), which are also
# those of bgemm_mi355x_<name>_runs and of bgemm_mi355x_selfcheck_launch_<name>; act: an activation id follows the strides (ReLU here);
# tail: further int arguments; second: (matrix, its stride, "r" read / "w" written) of everything besides A, the first weight and C;
# fusable: the pairs that may share one buffer -- [M][ld] with the second N columns in, the weights [2 N][ldb] with the second N rows down.
Call = namedtuple("Call", "family args strides act tail second fusable")
CALLS = {
    "tn_bias_act_aux": Call("tn", ("a", "b", "bias", "c", "z_out"), "abcz", True, (), (("z_out", "z", "w"),), ()),
    "nn_dact": Call("nn", ("a", "b", "z", "c"), "abcz", True, (), (("z", "z", "r"),), ()),
    "nn_dact_dbias": Call("nn", ("a", "b", "z", "c", "db32"), "abcz", True, (0,), (("z", "z", "r"),), ()),
    "nn_dgated": Call("nn", ("a", "b", "g", "u", "dg", "du"), "abzc", True, (), (("g", "z", "r"), ("u", "z", "r"), ("du", "c", "w")), (("g", "u"), ("dg", "du"))),
    "tn_gated": Call("tn", ("a", "wg", "wu", "bias_g", "bias_u", "c"), "abc", True, (), (("wu", "b", "r"),), (("wg", "wu"),)),
    "tn_gated_aux": Call("tn", ("a", "wg", "wu", "bias_g", "bias_u", "c", "g_out", "u_out"), "abcz", True, (),
                         (("wu", "b", "r"), ("g_out", "z", "w"), ("u_out", "z", "w")), (("wg", "wu"), ("g_out", "u_out"))),
    "tn_bias_add": Call("tn", ("a", "b", "bias", "r", "c"), "abcz", False, (), (("r", "z", "r"),), ()),
    "nn_add": Call("nn", ("a", "b", "r", "c"), "abcz", False, (), (("r", "z", "r"),), ()),
}
VECTORS = ("bias", "bias_g", "bias_u", "db32")
WRITTEN = ("c", "dg", "du", "z_out", "g_out", "u_out")
STRIDE_OF = dict(a="a", b="b", wg="b", wu="b", c="c", dg="c", du="c", z_out="z", z="z", g="z", u="z", g_out="z", u_out="z", r="z")
SOURCE = dict(a="a", wg="bt", wu="b2t", z="z", g="z", r="z", u="u", bias="bias", bias_g="bias", bias_u="bias2")   # Ops attribute of an input
READS_SECOND = ("nn_dact", "nn_dact_dbias", "nn_dgated", "tn_bias_add", "nn_add")     # calls whose second M x N matrices are inputs
IN_PLACE = ("tn_bias_add", "nn_add")
FUSED_TOO = ("nn_dgated", "tn_gated_aux")

# ---- the cases (tests/test_fused_bars_host.py reads them through operand_sets) ---------------------------------------------------------
REACH_CASES = [  # (call, config id, what lies at the edge, the strides at the edge, fused pairs (first names), in place, M, N): K = 128
    ("tn_bias_act_aux", 3, "z_out", "z", (), False, 136, 72),
    ("nn_dact", 0, "z", "z", (), False, 72, 72),
    ("nn_dact_dbias", 1, "z", "z", (), False, 136, 72),
    ("nn_dgated", 2, "g|u", "z", ("g",), False, 72, 72),
    ("nn_dgated", 1, "dg|du", "c", ("dg",), False, 136, 72),
    ("tn_gated_aux", 0, "g_out|u_out", "z", ("g_out",), False, 72, 72),
    ("tn_gated", 3, "wg|wu", "b", ("wg",), False, 136, 72),
    ("tn_bias_add", 2, "r", "z", (), False, 72, 72),
    ("nn_add", 3, "r", "z", (), False, 136, 72),
    ("tn_bias_add", 1, "r=c", "zc", (), True, 136, 72),
    ("nn_add", 0, "r=c", "zc", (), True, 72, 72),
]
REACH_K = 128
CLAMP_CASES = ("nn_dact", "tn_bias_add")                       # on config 0 (64 x 64), out of place
CLAMP = (136, 72, 128)
RASTER = (1160, 136, 128)
RASTER_WORDS = (1, 1 | NT, 2)
LADDER = [(136, 72, BK * s) for s in range(1, 8)]
LONG = (64, 64, 8128)                                          # 127 stages
LONG_WORDS = (1, 5)
LONG_MEMBERS = (0, 3)


def seed_of(shape):
    return sum(shape)


def operand_sets():
    """[(shape, seed, section)] of every operand set the tests below draw; one set serves every call at its shape."""
    sets = [((m, n, REACH_K), "reach") for m, n in sorted({c[6:8] for c in REACH_CASES})] + [(CLAMP, "clamp"), (RASTER, "raster")]
    sets += [(shape, "ladder") for shape in LADDER] + [(LONG, "long K")]
    return [(shape, seed_of(shape), section) for shape, section in sets]


# ---- the reference, all on the CPU -------------------------------------------------------------------------------------------------------
class Ops:
    """A [M][K], two weights B, B2 [K][N] (bt, b2t: [N][K]), two biases [N] and the second matrices z, u [M][N], on the CPU, and the two sums
    S = A B, S2 = A B2 exactly.  z serves as z, g and r."""

    def __init__(self, m, n, k, seed):
        rng = np.random.default_rng(seed)
        self.shape = (m, n, k)
        self.ints = ai, bi, b2i = rng.integers(-15, 16, size=(m, k)), rng.integers(-15, 16, size=(k, n)), rng.integers(-15, 16, size=(k, n))
        self.a = torch.from_numpy(ai * 2.0 ** -9).bfloat16()
        self.b, self.b2 = torch.from_numpy(bi.astype(np.float64)).bfloat16(), torch.from_numpy(b2i.astype(np.float64)).bfloat16()
        self.bt, self.b2t = self.b.t().contiguous(), self.b2.t().contiguous()
        self.s, self.s2 = (torch.from_numpy((ai @ w) * 2.0 ** -9).float() for w in (bi, b2i))     # exact: integers below 2^24
        assert k * 225 < 2 ** 24 and n <= 256
        j = torch.arange(n)
        sign = torch.where(j % 2 == 0, 1.0, -1.0)
        self.bias, self.bias2 = (sign * (j + 1) / 16.0).bfloat16(), (-sign * (j + 1) / 32.0).bfloat16()   # integers up to 256 over 16 / 32: bf16 values
        assert len(set(self.bias.tolist())) == n == len(set(self.bias2.tolist())), "the biases are pairwise distinct over N"
        self.z, self.u = (self._second(rng, m, n) for _ in range(2))
        self._dev = {}

    @staticmethod
    def _second(rng, m, n):
        x = torch.from_numpy(4.0 * rng.standard_normal((m, n))).bfloat16()
        x[x == 0] = 1.0
        assert bool((x != 0).all()) and bool((x > 0).any()) and bool((x < 0).any())
        return x

    def source(self, call, name):
        return self.bt if (name == "b" and CALLS[call].family == "tn") else self.b if name == "b" else getattr(self, SOURCE[name])

    def dev(self, call, name):
        key = (CALLS[call].family, name)
        if key not in self._dev:
            self._dev[key] = self.source(call, name).cuda()
        return self._dev[key]


@functools.lru_cache(maxsize=None)
def ops_of(shape):
    """Built once per shape and shared by every test; nothing writes to it."""
    return Ops(*shape, seed_of(shape))


def relu(x):
    return torch.where(x > 0, x, torch.zeros_like(x))            # act_apply<ACT_RELU>: +0 for everything else (no NaN here)


def expect(call, ops, z=None, u=None):
    """{output: what the call must store}, by torch on the CPU: the formulas of include/hgemm_mi355x.h with ReLU.  z / u: a second matrix
    in place of the operand set's own (the displaced and cut-short variants)."""
    s, s2, b, b2 = ops.s, ops.s2, ops.bias.float(), ops.bias2.float()
    zf, uf = (ops.z if z is None else z).float(), (ops.u if u is None else u).float()
    zero = torch.zeros_like(s)
    if call == "tn_bias_act_aux":
        return {"z_out": (s + b).bfloat16(), "c": relu(s + b).bfloat16()}
    if call in ("nn_dact", "nn_dact_dbias"):
        out = {"c": torch.where(zf <= 0, zero, s).bfloat16()}
        if call == "nn_dact_dbias":
            c64 = out["c"].double()
            assert float(c64.abs().sum(0).max()) < 2.0 ** 15 and torch.equal((c64 * 2.0 ** 9).round(), c64 * 2.0 ** 9), "a column sum is not exact in fp32"
            out["db32"] = c64.sum(0).float()                     # multiples of 2^-9, sum |C| below 2^15: exact in fp32 in any order
            assert torch.equal(out["db32"].double(), c64.sum(0))
        return out
    if call == "nn_dgated":
        return {"dg": torch.where(zf <= 0, zero, s * uf).bfloat16(), "du": (relu(zf) * s).bfloat16()}
    if call in ("tn_gated", "tn_gated_aux"):
        gp, up = s + b, s2 + b2
        out = {"c": (relu(gp) * up).bfloat16()}
        if call == "tn_gated_aux":
            out.update(g_out=gp.bfloat16(), u_out=up.bfloat16())
        return out
    if call == "tn_bias_add":
        return {"c": ((s + b) + zf).bfloat16()}
    assert call == "nn_add"
    return {"c": (s + zf).bfloat16()}


# ---- the mistakes the data must tell apart (tests/test_fused_bars_host.py), from the reference data alone -----------------------------------
DISPLACEMENTS = {"one row": (1, 0), "one 4-column group": (0, 4), "one tile row": (64, 0), "one tile column": (0, 64)}
PREVIOUS_TILE = "the previous tile column"                      # every column tile with n0 > 0 reads at n0 - 64
SHORT_RANGES = (7, 64)                                          # zeros from that row on: what a range that ends too early reads (7: a wrapped one, section 2)


def displaced(x, dr, dc):
    """x read dr rows and dc columns further on; what lies outside reads 0, as behind a descriptor's range."""
    m, n = x.shape
    out = torch.zeros_like(x)
    r0, r1, c0, c1 = max(0, -dr), min(m, m - dr), max(0, -dc), min(n, n - dc)
    if r0 < r1 and c0 < c1:
        out[r0:r1, c0:c1] = x[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return out


def previous_tile_column(x):
    return torch.cat([x[:, :64], x[:, :max(0, x.shape[1] - 64)]], 1)


def cut_short(x, row):
    out = x.clone()
    out[row:] = 0
    return out


def wrong_expectations(call, ops):
    """{name: ({output: bits a mistaken kernel would store}, (first tile row, first tile column) it can differ from)} for a call that reads
    its second matrices; both matrices of nn_dgated move together (one stride, one range rule)."""
    assert call in READS_SECOND
    out = {}
    for name, (dr, dc) in DISPLACEMENTS.items():
        out[name] = (expect(call, ops, displaced(ops.z, dr, dc), displaced(ops.u, dr, dc)), (0, 0))
    if ops.shape[1] > 64:
        out[PREVIOUS_TILE] = (expect(call, ops, previous_tile_column(ops.z), previous_tile_column(ops.u)), (0, 1))
    for row in SHORT_RANGES:
        if row < ops.shape[0]:
            out[f"zeros from row {row}"] = (expect(call, ops, cut_short(ops.z, row), cut_short(ops.u, row)), (row // 64, 0))
    return out


def tiles_differing(a, b):
    """[tile rows][tile columns] bool: the 64 x 64 tiles of the output in which a and b differ in some element"""
    diff = bits(a) != bits(b)
    m, n = diff.shape
    return torch.tensor([[bool(diff[i:i + 64, j:j + 64].any()) for j in range(0, n, 64)] for i in range(0, m, 64)])


def verdict(call, ops, got, what=""):
    """None if every output in `got` ({name: cpu tensor}) is what the call must store, else the finding: how many elements differ, where
    first, and which mistaken expectation the output equals, if any."""
    want, said = expect(call, ops), []
    assert set(got) == set(want), (set(got), set(want))
    for name in want:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, name
        bad = bits(got[name]) != bits(want[name])
        if not bool(bad.any()):
            continue
        first = tuple(bad.nonzero()[0].tolist())
        line = f"{what}: {name} differs in {int(bad.sum())} of {bad.numel()} elements, first at {first}: got {float(got[name][first])!r} for {float(want[name][first])!r}"
        if call in READS_SECOND and name != "db32":
            equal = [wrong for wrong, (outs, _) in wrong_expectations(call, ops).items() if torch.equal(bits(got[name]), bits(outs[name]))]
            line += "; it equals the expectation with the second matrix " + (" / ".join(equal) if equal else "of none of the known mistakes")
        if name != "db32":
            line += f"; {int(tiles_differing(got[name], want[name]).sum())} of its 64 x 64 tiles differ"
        said.append(line)
    return "\n".join(said) or None


# ---- the device side -------------------------------------------------------------------------------------------------------------------
class Flat:
    """One device buffer filled with `pad`, and the windows in it that hold matrices."""

    def __init__(self, numel, pad, dtype=torch.bfloat16):
        self.t, self.pad, self.windows = torch.full((numel,), pad, dtype=dtype, device="cuda"), pad, []

    def window(self, off, rows, cols, ld):
        assert off + (rows - 1) * ld + cols <= self.t.numel()
        self.windows.append(self.t.as_strided((rows, cols), (ld, 1), off))
        return self.windows[-1]

    def untouched_outside(self):
        """refills the windows; True if the whole buffer then holds the pad's bits"""
        for w in self.windows:
            w.fill_(self.pad)
        self.windows = []
        return all_same_bits(self.t, self.pad)


@pytest.fixture(scope="module")
def L(g):
    lib = g.lib()
    p, i = ctypes.c_void_p, ctypes.c_int
    for name, call in CALLS.items():
        getattr(lib, f"bgemm_mi355x_launch_{name}").argtypes = [i] * 2 + [p] * len(call.args) + [i] * (3 + len(call.strides) + call.act + len(call.tail)) + [p]
    lib.bgemm_mi355x_selfcheck_dact_z_range.restype = ctypes.c_uint
    lib.bgemm_mi355x_tn_config_by_name.argtypes = lib.hgemm_mi355x_nn_config_by_name.argtypes = [ctypes.c_char_p]
    info = (ctypes.c_int * 8)()
    for cid in range(4):
        assert lib.bgemm_mi355x_tn_config_by_name(TN_MEMBERS[cid].encode()) == cid == lib.hgemm_mi355x_nn_config_by_name(NN_MEMBERS[cid].encode())
        for fn in (lib.bgemm_mi355x_tn_config_info, lib.hgemm_mi355x_nn_config_info):
            assert fn(cid, info) == 0 and (info[0], info[1]) == TILES[cid]
    return lib


def member(call, cid):
    return (TN_MEMBERS if CALLS[call].family == "tn" else NN_MEMBERS)[cid]


def contiguous(call, shape):
    m, n, k = shape
    return {"a": k, "b": k if CALLS[call].family == "tn" else n, "c": n, "z": n}


def kernel_runs(L, call, cid, shape, lds):
    return getattr(L, f"bgemm_mi355x_{call}_runs")(cid, *shape, *(lds[s] for s in CALLS[call].strides)) == 1


def decision(L, call, cid, word, shape, lds):
    """(status, form, [(thunk, grid, epi, splits, k_chunk, items)]) of the call's selfcheck hook, aligned operands"""
    out = (ctypes.c_longlong * 44)()
    st = getattr(L, f"bgemm_mi355x_selfcheck_launch_{call}")(cid, word, 4, *shape, *(lds[s] for s in CALLS[call].strides), 0, *([RELU] if CALLS[call].act else []), out)
    return st, out[0], [tuple(out[4 + 8 * i:10 + 8 * i]) for i in range(out[1])]


def splits_of(word, k):
    """the two-pass split count that runs for a plan word: at most one split per stage, no empty split (tr_resolve_gemm)"""
    steps = k // BK
    splits = max(1, min(word & 0xFFFF, steps))
    per = -(-steps // splits)
    return -(-steps // per)


def shape_of(call, name, shape):
    m, n, k = shape
    return (m, k) if name == "a" else (n, k) if name in ("wg", "wu") or (name == "b" and CALLS[call].family == "tn") else (k, n) if name == "b" else (m, n)


class Runs:
    """The launches of one test: every wrong result is kept with the mistake it matches, and all of them fail the test at the end."""

    def __init__(self, g, L):
        self.g, self.L, self.lines, self.runs, self.t0, self.pool = g, L, [], 0, time.perf_counter(), {}

    def flat(self, key, numel, pad, dtype=torch.bfloat16):
        """a buffer of the pool (left all pad by the run before) if it is large enough, else a new one"""
        old = self.pool.get(key)
        if old is None or old.t.numel() < numel or old.windows:
            self.pool.pop(key, None)                             # (freed before its successor is allocated)
            del old
            self.pool[key] = Flat(numel, pad, dtype)
        return self.pool[key]

    def run(self, call, ops, cid, word, lds=None, fuse=(), inplace=False, reference=False, want_epi=None, what=""):
        """One call of bgemm_mi355x_launch_<call>.  lds: {a, b, c, z} -> stride (default: contiguous, a fused pair 2 N wide); fuse: the first
        names of the fusable pairs that share a buffer; inplace: r == c.  The hook must report the reference kernel (reference) or the
        member kernel in the form the word asks for."""
        L, spec, shape = self.L, CALLS[call], ops.shape
        m, n, k = shape
        lds = dict(contiguous(call, shape), **(lds or {}))
        partner = {first: second for first, second in spec.fusable if first in fuse}
        for first in partner:
            if first != "wg":
                lds[STRIDE_OF[first]] = max(lds[STRIDE_OF[first]], 2 * n)
        what = f"{call} {member(call, cid)} {hex(word)} {m}x{n}x{k} ld={lds}{' fused ' + '+'.join(fuse) if fuse else ''}{' in place' if inplace else ''} {what}"
        splits = splits_of(word, k)
        st, form, disp = decision(L, call, cid, word, shape, lds)
        want_form = FORM_REFERENCE if reference else FORM_SPLITK if splits > 1 else FORM_PLAIN
        assert (st, form) == (0, want_form) and kernel_runs(L, call, cid, shape, lds) == (not reference), (what, st, form, disp)
        assert reference or disp[0][3] == splits, (what, disp)
        assert want_epi is None or disp[0][2] == want_epi, (what, disp)
        # place every argument
        flats, win, ptr, inputs = [], {}, {}, []
        second_of = {second: first for first, second in partner.items()}
        for name in spec.args:
            if name in VECTORS:
                if name == "db32":
                    f = Flat(n + 8, DB_SENTINEL, torch.float32)
                    win[name] = f.window(0, 1, n, n)
                    win[name].fill_(float("nan"))
                else:
                    f = Flat(n + 8, float("nan"))
                    win[name] = f.window(0, 1, n, n)
                    win[name].copy_(ops.dev(call, name).view(1, n))
                    inputs.append(name)
                flats.append(f)
                ptr[name] = win[name].data_ptr()
                continue
            if name in second_of or (inplace and name == "r"):
                continue                                         # placed with its partner / with c
            rows, cols = shape_of(call, name, shape)
            ld = lds[STRIDE_OF[name]]
            written = name in WRITTEN
            pair = (name, partner[name]) if name in partner else (name,)
            numel = (2 if name == "wg" and len(pair) == 2 else 1) * rows * ld + 8
            f = self.flat((call, name, written), numel, OUT_FILL if written else float("nan"))
            flats.append(f)
            for idx, each in enumerate(pair):
                win[each] = f.window(idx * (rows * ld if name == "wg" else cols), rows, cols, ld)
                ptr[each] = win[each].data_ptr()
                if written and not (inplace and each == "c"):
                    win[each].fill_(float("nan"))
                else:
                    win[each].copy_(ops.dev(call, "r" if inplace and each == "c" else each))
                    if not written:
                        inputs.append(each)
        if inplace:
            assert lds["z"] == lds["c"]
            ptr["r"] = ptr["c"]
        assert all(p % 16 == 0 for p in ptr.values())
        st = getattr(L, f"bgemm_mi355x_launch_{call}")(cid, word, *(ptr[name] for name in spec.args), m, n, k, *(lds[s] for s in spec.strides),
                                                      *([RELU] if spec.act else []), *spec.tail, self.g.stream())
        torch.cuda.synchronize()
        assert st == 0, (what, L.hgemm_mi355x_strerror(st))
        self.runs += 1
        got = {name: (win[name].cpu().view(n) if name == "db32" else win[name].cpu().contiguous()) for name in spec.args if name in WRITTEN or name == "db32"}
        said = verdict(call, ops, got, what)
        for name in inputs:
            if not torch.equal(bits(win[name]), bits(ops.dev(call, name).view(win[name].shape))):
                said = (said + "\n" if said else "") + f"{what}: the input {name} changed"
        if not all(f.untouched_outside() for f in flats):
            said = (said + "\n" if said else "") + f"{what}: a buffer changed outside its matrices"
        if said:
            self.lines.append(said)

    def close(self, what, expect_runs):
        print(f"{what}: {self.runs} launches, {len(self.lines)} wrong, {time.perf_counter() - self.t0:.2f} s")
        assert not self.lines, f"{what}: {len(self.lines)} of {self.runs} runs are wrong:\n" + "\n".join(self.lines)
        assert self.runs == expect_runs, (self.runs, expect_runs)
        self.pool.clear()
        torch.cuda.empty_cache()


def layouts_of(call):
    """[(fuse, inplace)] of a sweep: the plain layout, the residual calls once more in place, dgated and gated_aux once more fused"""
    out = [((), False)]
    if call in IN_PLACE:
        out.append(((), True))
    if call in FUSED_TOO:
        out.append((tuple(first for first, _ in CALLS[call].fusable), False))
    return out


# ---- 1. the reach edges of the second matrices, both sides executed ------------------------------------------------------------------------
def reach_rule(call, cid, what, shape):
    """(rows, tail bytes): rows x ld x 2 + tail < 2 GiB.  A second M x N matrix is addressed from a tile's first row, BM rows and then the
    row's N elements (z_ok of tr_resolve_gemm; C's rule for dg|du and for an in-place r); a gated weight from its tile's first row, BN / 2
    rows of each weight and then the row's K elements (TrLayout::reach_ok)."""
    bm, bn = TILES[cid]
    m, n, k = shape
    return (bn // 2, 2 * k) if what == "wg|wu" else (bm, 2 * n)


def edge_stride(L, call, cid, shape, edge, fuse):
    """the largest stride at which the member's kernel still runs, every other operand contiguous (a fused pair: 2 N wide), by bisection over
    the call's _runs function"""
    base = contiguous(call, shape)
    if fuse and fuse[0] != "wg":
        base[STRIDE_OF[fuse[0]]] = 2 * shape[1]
    return largest_stride(lambda s: kernel_runs(L, call, cid, shape, dict(base, **{e: s for e in edge})), max(base[e] for e in edge))


@pytest.mark.parametrize("case", REACH_CASES, ids=lambda c: f"{c[0]}-{c[2]}-{'x'.join(map(str, TILES[c[1]]))}")
def test_fused_reach_edges_run_exact_on_both_sides(g, L, case):
    """Per second matrix: the largest stride at which the member's kernel still runs, asserted against the written rule, run plain and in
    2 splits; the next multiple of 8, run by the reference kernel (64-bit addressing).  M is a little over one tile row, so the ragged
    second row band's descriptor base lies just below the limit (the gated weights: N a little over one tile column).  The matrix lies in
    one flat buffer whose bytes outside the windows must come back unchanged."""
    call, cid, what, edge, fuse, inplace, m, n = case
    shape = (m, n, REACH_K)
    bm, bn = TILES[cid]
    assert bm < m < 2 * bm and (what != "wg|wu" or bn // 2 < n < bn)
    s = edge_stride(L, call, cid, shape, edge, fuse)
    rows, tail = reach_rule(call, cid, what, shape)
    assert rows * s * 2 + tail < 2 * GIB <= rows * (s + 8) * 2 + tail, (s, rows, tail)            # the documented rule
    ops, r = ops_of(shape), Runs(g, L)
    for stride, reference in ((s + 8, True), (s, False)):
        for word in (1, 2):
            r.run(call, ops, cid, word, {e: stride for e in edge}, fuse, inplace, reference, what=f"{what} at the edge")
    big = max(f.t.numel() for f in r.pool.values()) * 2 / 1e9
    print(f"reach {call} {what} {member(call, cid)}: edge stride {s}, buffer {big:.2f} GB")
    r.close(f"reach {call} {what}", 4)


# ---- 2. the clamped descriptor range ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", CLAMP_CASES)
def test_a_second_matrix_of_more_than_4_gib_is_read_through_a_clamped_range(g, L, call):
    """z / r at the edge stride of the 64 x 64 member with M = 136: behind the first tile's first row the matrix goes on for more than
    4 GiB, so its range is clamped to 2^32 - 1; the second tile's fits; the third's ends at the last valid element.  A range that wrapped
    would be (135 ldz + N) 2 - 2^32 bytes, just under 7 rows: the first tile would read zeros from row 7 on, which the data show."""
    m, n, k = CLAMP
    ldz = edge_stride(L, call, 0, CLAMP, "z", ())
    ranges = [L.bgemm_mi355x_selfcheck_dact_z_range(m, n, ldz, m0) for m0 in (0, 64, 128)]
    full = [((m - 1 - m0) * ldz + n) * 2 for m0 in (0, 64, 128)]
    assert full[0] > 0xFFFFFFFF and ranges[0] == 0xFFFFFFFF, "the first tile's range is clamped"
    assert 63 * ldz * 2 + n * 2 < full[1] < 0xFFFFFFFF and ranges[1] == full[1], "the second tile's range is not, and goes on behind the tile"
    assert ranges[2] == full[2] == (7 * ldz + n) * 2, "the third tile's range ends at the last valid element"
    ops, r = ops_of(CLAMP), Runs(g, L)
    for word in (1, 2):
        r.run(call, ops, 0, word, {"z": ldz}, what="clamped range")
    print(f"clamp {call}: ldz {ldz}, buffer {max(f.t.numel() for f in r.pool.values()) * 2 / 1e9:.2f} GB")
    r.close(f"clamp {call}", 2)


# ---- 3. rasters of more than eight tile rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", list(CALLS))
def test_fused_rasters_of_more_than_eight_tile_rows_are_exact(g, L, call):
    """1160 x 136 x 128: 19 / 10 tile rows -- group_m = 8, whole groups and a ragged last one -- with ragged M and N; the stride of the second
    matrix travels in the field the raster map takes as tail_first.  Every member, the plain store, the NT store and 2 splits; the residual
    calls also in place, dgated and gated_aux also with fused buffers."""
    m, n, k = RASTER
    assert all(-(-m // bm) > 8 and -(-m // bm) % 8 for bm, _ in TILES) and m % 128 and n % 64
    ops, r = ops_of(RASTER), Runs(g, L)
    for fuse, inplace in layouts_of(call):
        for cid in range(4):
            for word in RASTER_WORDS:
                r.run(call, ops, cid, word, None, fuse, inplace, what="raster")
    r.close(f"raster {call}", len(layouts_of(call)) * 4 * len(RASTER_WORDS))


# ---- 4. the K ladder and long K ---------------------------------------------------------------------------------------------------------------
def ladder_words(k):
    """the plain word, one split per stage and 2 splits -- those that run differently"""
    return sorted({splits_of(w, k): w for w in (2, k // BK, 1)}.values())


@pytest.mark.parametrize("call", list(CALLS))
def test_fused_epilogues_behind_every_stage_count_of_the_k_ladder(g, L, call):
    """136 x 72 x 64 s, s = 1 .. 7: behind both ring depths every stage count modulo 3 and modulo 4 ends a fused kernel, whose loads stand
    behind the K loop under a counted vmcnt; dact_dbias runs with its workspace, so the fused tile sums reuse the ring's LDS (asserted
    through the hook's epilogue id).  Every member; the residual calls also in place."""
    r, want = Runs(g, L), 0
    for shape in LADDER:
        ops = ops_of(shape)
        for fuse, inplace in layouts_of(call)[:2 if call in IN_PLACE else 1]:
            for cid in range(4):
                for word in ladder_words(shape[2]):
                    fused_sum = call == "nn_dact_dbias" and splits_of(word, shape[2]) == 1
                    r.run(call, ops, cid, word, None, fuse, inplace, want_epi=EPI_DBIAS + RELU if fused_sum else None, what="ladder")
                    want += 1
    assert want == (2 if call in IN_PLACE else 1) * 4 * (1 + 2 + 3 * 5)
    r.close(f"ladder {call}", want)


@pytest.mark.parametrize("call", list(CALLS))
def test_fused_epilogues_behind_127_stages(g, L, call):
    """64 x 64 x 8128, plain and in five chunks, the 64 x 64 and the 128 x 128 member; the residual calls also in place."""
    assert LONG[2] // BK == 127 and splits_of(5, LONG[2]) == 5
    ops, r = ops_of(LONG), Runs(g, L)
    layouts = layouts_of(call)[:2 if call in IN_PLACE else 1]
    for fuse, inplace in layouts:
        for cid in LONG_MEMBERS:
            for word in LONG_WORDS:
                r.run(call, ops, cid, word, None, fuse, inplace, want_epi=EPI_DBIAS + RELU if call == "nn_dact_dbias" and word == 1 else None, what="long K")
    r.close(f"long K {call}", len(layouts) * len(LONG_MEMBERS) * len(LONG_WORDS))
