"""Index model of the v_mfma_f32_16x16x32_bf16 K loop of k_gemm_pq / k_gemm_pz (gemm.hip: pq_frag16, pq_mma16, pq_acc_swap16), no GPU needed.

This is a model of the intended map, not a check of the .hip text: frag16() and swap23() below restate pq_frag16 by hand, so the test proves that the design is
consistent with the ISA layouts; tests/test_gemm_bounds_gpu.py and tests/test_conv_bounds_gpu.py tie the kernel itself to the result.

A wave's 64 features x 128 tokens x one K-tile (64 k) are pushed through a per-lane model of
  * the staged LDS image (128-byte rows, 16-byte chunk c of region row r at chunk c ^ ((r >> 1) & 7)),
  * the fragment addresses of pq_frag16 (W rows read with bits 2 and 3 of the in-tile row swapped),
  * the operand and result layouts of the 16x16x32 MFMA (lane l: A row / B column l & 15, k = 8 (l >> 4) .. + 8; C column l & 15, rows 4 (l >> 4) + reg),
  * the register placement of pq_mma16 (tile fi, tj of a 32 x 32 block -> registers 8 fi + 4 tj + b) and
  * v_permlane16_swap as pq_acc_swap16 applies it (odd 16-lane rows of the first register <-> even rows of the second),
and every accumulator must end up where the epilogues read it: the 32x32x16 layout, lane l register 4 a + b of acc[i][j] = token 32 j + (l & 31), feature
32 i + 8 a + 4 (l >> 5) + b.  The four phases of a K-tile pair (feature half i, token half) as in the kernel; the products are exact integers."""
import numpy as np

LANES = 64


def swap23(r):
    return (r & 3) | ((r & 4) << 1) | ((r & 8) >> 1)


def stage(rows):
    """rows [n, 64] (k elements) -> LDS image [n, 8 chunks, 8 elements] as the LDS-DMA leaves it"""
    n = rows.shape[0]
    img = np.zeros((n, 8, 8), dtype=rows.dtype)
    for r in range(n):
        for c in range(8):
            img[r, c ^ ((r >> 1) & 7)] = rows[r, 8 * c:8 * c + 8]
    return img


def frag16(lane, w_operand):
    """pq_frag16: byte offsets (relative to the 32-row block) of fragments q = 2 tile + ks"""
    l15, kq = lane & 15, lane >> 4
    row = swap23(l15) if w_operand else l15
    return [(16 * (q >> 1) + row) * 128 + (((4 * (q & 1) + kq) ^ ((row >> 1) & 7)) << 4) for q in range(4)]


def read_b128(img, byte):
    assert byte % 16 == 0
    return img[byte // 128, (byte % 128) // 16]


def mfma16(a, b, c):
    """a, b: [64 lanes, 8]; c: [64 lanes, 4] -> c + A B^T in the layouts of v_mfma_f32_16x16x32_bf16"""
    A = np.zeros((16, 32), dtype=np.int64)
    B = np.zeros((16, 32), dtype=np.int64)
    for l in range(LANES):
        A[l & 15, 8 * (l >> 4):8 * (l >> 4) + 8] = a[l]
        B[l & 15, 8 * (l >> 4):8 * (l >> 4) + 8] = b[l]
    D = A @ B.T                                   # [row = A row, col = B row]
    out = c.copy()
    for l in range(LANES):
        for r in range(4):
            out[l, r] += D[4 * (l >> 4) + r, l & 15]
    return out


def permlane16_swap(v0, v1):
    """v_permlane16_swap_b32 v0, v1: rows of 16 lanes; odd rows of v0 <-> even rows of v1"""
    r0, r1 = v0.copy(), v1.copy()
    for l in range(LANES):
        if (l >> 4) & 1:
            r0[l] = v1[l - 16]
        else:
            r1[l] = v0[l + 16]
    return r0, r1


def run_wave_tile(W, X):
    """W [64 features, 64 k], X [128 tokens, 64 k] -> acc[2][4][lane][16] after the K loop and the swap"""
    acc = np.zeros((2, 4, LANES, 16), dtype=np.int64)
    for i, th in ((0, 0), (1, 0), (1, 1), (0, 1)):             # P0 WA x XA, P1 WB x XA, P2 WB x XB, P3 WA x XB
        wimg = stage(W[32 * i:32 * i + 32])
        ximg = stage(X[64 * th:64 * th + 64])
        wf = [np.stack([read_b128(wimg, frag16(l, True)[q]) for l in range(LANES)]) for q in range(4)]
        xf = [[np.stack([read_b128(ximg, frag16(l, False)[q] + j * 4096) for l in range(LANES)]) for q in range(4)] for j in range(2)]
        for ks in range(2):
            for fi in range(2):
                for j in range(2):
                    for tj in range(2):
                        r0 = 8 * fi + 4 * tj
                        a = acc[i, 2 * th + j]
                        a[:, r0:r0 + 4] = mfma16(wf[2 * fi + ks], xf[j][2 * tj + ks], a[:, r0:r0 + 4])
    for i in range(2):
        for j in range(4):
            for fi in range(2):
                for b in range(4):
                    lo, hi = 8 * fi + b, 8 * fi + 4 + b
                    acc[i, j, :, lo], acc[i, j, :, hi] = permlane16_swap(acc[i, j, :, lo], acc[i, j, :, hi])
    return acc


def test_every_accumulator_lands_where_the_epilogues_read_it():
    rng = np.random.default_rng(0)
    W = rng.integers(-8, 9, size=(64, 64))
    X = rng.integers(-8, 9, size=(128, 64))
    acc = run_wave_tile(W, X)
    want = W @ X.T                                              # [feature, token]
    assert len(np.unique(want)) > 100                           # (a map error cannot hide behind equal values)
    for i in range(2):
        for j in range(4):
            for l in range(LANES):
                for reg in range(16):
                    f = 32 * i + 8 * (reg >> 2) + 4 * (l >> 5) + (reg & 3)
                    t = 32 * j + (l & 31)
                    assert acc[i, j, l, reg] == want[f, t], (i, j, l, reg)


def test_map_is_a_rotation_of_lane_bits_5_4_and_register_bit_2():
    """before the swap: lane l, register 8 fi + 4 tj + b holds token 16 tj + (l & 15), feature 16 fi + 8 (l >> 4 & 1) + 4 (l >> 5) + b of the 32 x 32 block"""
    for l in range(LANES):
        for fi in range(2):
            for tj in range(2):
                for b in range(4):
                    row = 4 * (l >> 4) + b                      # C row of the 16x16 result = A row = W row swap23(row) of tile fi
                    assert 16 * fi + swap23(row) == 16 * fi + 8 * ((l >> 4) & 1) + 4 * (l >> 5) + b
    # the swap exchanges lane bit 4 with register bit 2 (tj) and leaves lane bit 5 alone
    v0 = np.arange(LANES)
    v1 = 100 + np.arange(LANES)
    r0, r1 = permlane16_swap(v0, v1)
    for l in range(LANES):
        src_lane = (l & ~16)
        assert r0[l] == (v0[l] if not (l & 16) else v1[src_lane])
        assert r1[l] == (v1[l] if (l & 16) else v0[l | 16])


def test_fragment_reads_cover_the_k_tile_once_and_are_bank_conflict_free():
    for w_operand in (False, True):
        for q in range(4):
            for g in range(4):                                  # the four 16-lane groups a ds_read_b128 is served in
                groups = {(frag16(l, w_operand)[q] % 256) // 16 for l in range(16 * g, 16 * g + 16)}
                assert len(groups) == 16, (w_operand, q, g)     # 16 distinct 16-byte groups of the 64 x 4-byte banks
        # the k chunk a lane reads back (un-swizzled) is 4 ks + (lane >> 4), the same for both operands: both MFMA operands pair equal k
        img = stage(np.tile(np.repeat(np.arange(8), 8), (32, 1)))
        for l in range(LANES):
            for q in range(4):
                assert (read_b128(img, frag16(l, w_operand)[q]) == 4 * (q & 1) + (l >> 4)).all()
        rows = {(frag16(l, w_operand)[q] // 128) for l in range(LANES) for q in range(4)}
        assert rows == set(range(32))
