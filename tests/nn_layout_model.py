"""CPU replay of family n's B image (cuda-l2_amd/csrc/hgemm_kernel_nn.hpp): the LDS-DMA write map, the transposed-read address
map and what ds_read_b64_tr_b16 hands each lane, restated in Python from the kernel's comments so that tests/test_nn_host.py can
check them against the MFMA operand contract without a GPU.

Image of one stage: [64 k-rows][BN halfs], k-row kr at byte kr * 2 BN, its 16-byte chunk c at slot c ^ swz(kr).
  DMA piece `il` (1 KiB, lane-linear destination): lane l writes 16 bytes at il * 1024 + 16 l, i.e. k-row il * (512 / BN) + l // (BN / 8),
  slot l % (BN / 8); the lane's SOURCE chunk is slot ^ swz(k-row).
  Transposed read h (0, 1) of K = 32 slice ks, column tile jn of wave column wave_n: lane 4q + p of 16-lane group gq addresses
  k-row 32 ks + 8 gq + 4 h + q, chunk (wave_n TN + 16 jn) / 8 + (p >> 1), its 8-byte half p & 1.
  The instruction: lane 4q + p of a group supplies the address of block row q, columns 4p .. 4p + 3; lane i receives column i with
  row q in element q.
  MFMA contract (v_mfma_f32_16x16x32_f16, this operand): lane (n = lane & 15, kq = lane >> 4) holds k = 8 kq .. 8 kq + 7 of column n.
"""
BK = 64


def swz(bn: int, kr: int) -> int:
    if bn == 128:
        return ((kr & 3) << 2) | ((kr >> 2) & 3)
    assert bn == 64
    return (((kr >> 1) & 1) | (((kr >> 3) & 1) << 1)) << 1


def dma_writes(bn: int):
    """Every (LDS byte offset inside the B image, k-row, source chunk) one stage's DMA pieces write, 16 bytes each."""
    ch = bn // 8
    rows_per_piece = 64 // ch
    out = []
    for il in range(BK * bn * 2 // 1024):
        for lane in range(64):
            kr = il * rows_per_piece + lane // ch
            out.append((il * 1024 + lane * 16, kr, (lane % ch) ^ swz(bn, kr)))
    return out


def build_image(bn: int):
    """The image as the DMA leaves it: byte offset of every half -> (k, n) of the tile; asserts that no byte is written twice."""
    image = {}
    for off, kr, chunk in dma_writes(bn):
        for e in range(8):
            assert off + 2 * e not in image, "two DMA lanes write the same LDS bytes"
            image[off + 2 * e] = (kr, chunk * 8 + e)
    return image


def read_addresses(bn: int, tn: int, wave_n: int, ks: int, h: int, jn: int):
    """Byte address (inside the B image) of each of the 64 lanes for one transposed read."""
    out = []
    for lane in range(64):
        gq, q, p = lane >> 4, (lane >> 2) & 3, lane & 3
        kr = 8 * gq + 4 * h + q
        chunk = (wave_n * tn + jn * 16) // 8 + (p >> 1)
        out.append((ks * 32 + kr) * bn * 2 + ((chunk ^ swz(bn, kr)) << 4) + 8 * (p & 1))
    return out


def transposed_read(image, addrs):
    """What ds_read_b64_tr_b16 returns: per lane the four (k, n) ids of its elements 0..3."""
    out = []
    for lane in range(64):
        base, i = lane & ~15, lane & 15
        elems = []
        for q in range(4):
            src = addrs[base + 4 * q + (i >> 2)]          # the lane that addresses block row q, columns 4 (i >> 2) ..
            elems.append(image[src + 2 * (i & 3)])
        out.append(elems)
    return out


def bank_conflict_ways(addrs) -> int:
    """Worst number of distinct 4-byte words one bank serves within a 32-lane half (64 banks of 4 bytes; 8 bytes per lane)."""
    worst = 1
    for half in (addrs[:32], addrs[32:]):
        words = {}
        for a in half:
            for w in (a // 4, a // 4 + 1):
                words.setdefault(w % 64, set()).add(w)
        worst = max(worst, max(len(v) for v in words.values()))
    return worst
