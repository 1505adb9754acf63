"""CPU test of the selection rule of q256x256_w2x2's one-tile-per-workgroup kernel (sq_one_takes, hgemm_inst_g13.hip), read through
hgemm_mi355x_one_item_kernel_takes: the launch hgemm_mi355x_launch would make for these arguments (b_col_major given, aligned pointers),
nothing launched.  The plan, its config id and flags are the caller's: the rule only picks the kernel."""
import ctypes

import pytest

NT_STORE, FUSED, STREAMK, XCD_STAGGER, PHASE, WAVE_PRIORITY, PHASE4 = 0x20000, 0x10000, 0x40000, 0x80000, 0x200000, 0x400000, 0x800000
KMIN = 3


@pytest.fixture(scope="module")
def lib():
    import build

    L = ctypes.CDLL(str(build.build_library()))
    L.hgemm_mi355x_config_by_name.argtypes = [ctypes.c_char_p]
    L.hgemm_mi355x_one_item_kernel_launches.restype = ctypes.c_ulonglong
    yield L
    L.hgemm_mi355x_set_one_item_kernel(1)


def takes(L, name, splits, m, n, k, ld=None, group=2):
    lda, ldb, ldc = ld or (k, k, n)
    return L.hgemm_mi355x_one_item_kernel_takes(L.hgemm_mi355x_config_by_name(name.encode()), splits, group, m, n, k, lda, ldb, ldc)


def test_the_switch_is_on_by_default_and_returns_the_previous_value(lib):
    assert lib.hgemm_mi355x_set_one_item_kernel(0) == 1
    assert takes(lib, "q256x256_w2x2", 1, 4096, 4096, 4096) == 0
    assert lib.hgemm_mi355x_set_one_item_kernel(1) == 0
    assert lib.hgemm_mi355x_set_one_item_kernel(1) == 1
    assert takes(lib, "q256x256_w2x2", 1, 4096, 4096, 4096) == 1
    assert lib.hgemm_mi355x_one_item_kernel_launches() == 0      # a query launches nothing


@pytest.mark.parametrize("splits, m, n, k, ld, want", [
    (1, 4096, 4096, 4096, None, 1),                 # the headline launch: 256 tiles on 256 workgroups
    (1 | NT_STORE, 4096, 4096, 4096, None, 1),      # ... as the tuned table runs it
    (1 | WAVE_PRIORITY, 4096, 4096, 512, None, 1),  # (the flag means nothing to a one-workgroup-per-CU member)
    (1, 256, 256, 64 * KMIN, None, 1),
    (1, 256, 256, 64 * KMIN + 64, None, 1),
    (1, 512, 768, 1024, None, 1),
    (1, 200, 248, 640, None, 1),                    # ragged M and N inside one tile, N % 8 == 0
    (1, 512, 768, 1024, (1032, 1056, 808), 1),      # padded strides, ldc % 8 == 0
    (1, 256, 256, 64 * (KMIN - 1), None, 0),        # fewer K-steps than the streams are deep
    (1, 256, 256, 64 * KMIN + 8, None, 0),          # K tail: the ktail variant of the general kernel
    (1, 4352, 4096, 512, None, 0),                  # 272 tiles > 256 workgroups
    (1, 4352, 4352, 512, None, 0),                  # 289 tiles
    (1, 512, 764, 1024, None, 0),                   # N % 8 != 0: narrow epilogue
    (1, 512, 768, 1024, (1024, 1024, 772), 0),      # ldc % 8 != 0: narrow epilogue
    (2, 512, 768, 1024, None, 0),                   # two-pass split-K: slab epilogue
    (2 | FUSED, 512, 768, 1024, None, 0),           # single-launch split-K
    (1 | XCD_STAGGER, 4096, 4096, 4096, None, 0),   # the kstagger variant
    (1 | PHASE, 4096, 4096, 4096, None, 0),
    (1 | PHASE4, 4096, 4096, 4096, None, 0),
    (1 | PHASE | PHASE4, 4096, 4096, 4096, None, 0),
])
def test_selection_rule(lib, splits, m, n, k, ld, want):
    lib.hgemm_mi355x_set_one_item_kernel(1)
    assert takes(lib, "q256x256_w2x2", splits, m, n, k, ld) == want
    lib.hgemm_mi355x_set_one_item_kernel(0)
    assert takes(lib, "q256x256_w2x2", splits, m, n, k, ld) == 0
    lib.hgemm_mi355x_set_one_item_kernel(1)


def test_only_the_one_geometry_has_the_kernel(lib):
    lib.hgemm_mi355x_config_name.restype = ctypes.c_char_p
    for i in range(lib.hgemm_mi355x_num_configs()):
        name = lib.hgemm_mi355x_config_name(i).decode()
        if lib.hgemm_mi355x_config_accepts_k(i, 1024) != 1:
            continue
        got = lib.hgemm_mi355x_one_item_kernel_takes(i, 1, 2, 512, 768, 1024, 1024, 1024, 768)
        assert got == (1 if name == "q256x256_w2x2" else 0), name


def test_the_planned_headline_call_takes_it_and_its_plan_is_unchanged(lib):
    cfg, splits, group = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.hgemm_mi355x_plan(4096, 4096, 4096, ctypes.byref(cfg), ctypes.byref(splits), ctypes.byref(group)) == 0
    lib.hgemm_mi355x_config_name.restype = ctypes.c_char_p
    assert lib.hgemm_mi355x_config_name(cfg.value) == b"q256x256_w2x2"
    assert lib.hgemm_mi355x_one_item_kernel_takes(cfg.value, splits.value, group.value, 4096, 4096, 4096, 4096, 4096, 4096) == 1


def test_bad_arguments_are_the_launch_s_errors(lib):
    q = lib.hgemm_mi355x_config_by_name(b"q256x256_w2x2")
    assert lib.hgemm_mi355x_one_item_kernel_takes(q, 1, 2, 0, 256, 256, 256, 256, 256) == -1
    assert lib.hgemm_mi355x_one_item_kernel_takes(q, 1, 2, 256, 256, 256, 128, 256, 256) == -1      # lda < K
    assert lib.hgemm_mi355x_one_item_kernel_takes(10 ** 6, 1, 2, 256, 256, 256, 256, 256, 256) == -1
