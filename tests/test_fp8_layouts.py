"""Symbolic (host-side) replay of the fp8 GEMM's LDS staging, fragment reads
and epilogue (dinov3_amd/ops/csrc/fp8_gemm.hip), at 16-byte-slot granularity.

Transcribes the kernel's integer index arithmetic for one K-step and checks,
cell by cell, that staging writes never collide or leave the allocation, that
every fragment read sees the (row, k-slot) the math needs, that A and B use
the same k order, that edge rows/columns read zeros, that the ds_read_b128
lane groups are bank-conflict free, and that the epilogue stores every output
exactly once.
"""

import pytest

BM = BN = 128
BK = 128            # bytes per row of an operand image
THREADS = 256
WAVE = 64
TILE_BYTES = BM * BK
BUF_BYTES = 2 * TILE_BYTES
PIECES = TILE_BYTES // (THREADS * 16)
ROWS_PER_PIECE = THREADS * 16 // BK
ZERO = ("zero",)

# ds_read_b128 is served in four 16-lane groups (two per 32-lane half).
_G0 = [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27]
_G1 = [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]
B128_GROUPS = [_G0, _G1, [l + 32 for l in _G0], [l + 32 for l in _G1]]


def _swz(r):
    return ((r >> 1) & 1) | (((r >> 2) & 1) << 2)


def _stage_block(brow, bcol, M, N):
    """LDS image of one buffer after the zero prefill and one stage() call:
    byte offset of a 16-byte slot -> ("A"|"B", global row, k-slot) or ZERO."""
    lds = {}

    def put(addr, what):
        assert 0 <= addr and addr + 16 <= BUF_BYTES, "write leaves the buffer"
        assert addr % 16 == 0
        assert addr not in lds, f"two writes to LDS byte {addr}"
        lds[addr] = what

    for tid in range(THREADS):
        lane, wid = tid % WAVE, tid // WAVE
        srow = tid >> 3
        sslot = (tid & 7) ^ _swz(srow)
        for i in range(PIECES):
            a_row = brow + i * ROWS_PER_PIECE + srow
            b_row = bcol + i * ROWS_PER_PIECE + srow
            zero_off = i * (THREADS * 16) + tid * 16                # ds_write of zeros
            dma_off = wid * (WAVE * 16) + i * (THREADS * 16) + lane * 16  # base + lane*16
            if a_row < M:
                put(dma_off, ("A", a_row, sslot))
            else:
                put(zero_off, ZERO)
            if b_row < N:
                put(TILE_BYTES + dma_off, ("B", b_row, sslot))
            else:
                put(TILE_BYTES + zero_off, ZERO)
    assert len(lds) == BUF_BYTES // 16, "some LDS slot is never written"
    return lds


@pytest.mark.parametrize("N", [16, 48, 272])
@pytest.mark.parametrize("M", [1, 33, 130])
def test_fp8_gemm_stage_read_store_layout(M, N):
    stored = {}
    for by in range((M + BM - 1) // BM):
        for bx in range((N + BN - 1) // BN):
            brow, bcol = by * BM, bx * BN
            lds = _stage_block(brow, bcol, M, N)
            for wid in range(THREADS // WAVE):
                wm, wn = wid >> 1, wid & 1
                for t in range(4):  # the m (A) / n (B) fragment repeat
                    a_addrs, b_addrs = {}, {}
                    for lane in range(WAVE):
                        fr, fg = lane & 15, lane >> 4
                        foff = [fr * BK + (((2 * fg + h) ^ _swz(fr)) * 16) for h in (0, 1)]
                        for h in (0, 1):
                            a_addr = wm * 64 * BK + t * 16 * BK + foff[h]
                            b_addr = TILE_BYTES + wn * 64 * BK + t * 16 * BK + foff[h]
                            a_addrs[(lane, h)] = a_addr
                            b_addrs[(lane, h)] = b_addr
                            a_row = brow + wm * 64 + t * 16 + fr
                            b_row = bcol + wn * 64 + t * 16 + fr
                            # lane l, half h must hold k-slot 2*(l>>4)+h of row
                            # l&15 of the tile: the same k order for A and B
                            want_a = ("A", a_row, 2 * fg + h) if a_row < M else ZERO
                            want_b = ("B", b_row, 2 * fg + h) if b_row < N else ZERO
                            assert lds[a_addr] == want_a
                            assert lds[b_addr] == want_b
                    # bank conflicts: inside one lane group every 16-byte read
                    # must sit on its own 16-byte position of the 256-byte bank row
                    for addrs in (a_addrs, b_addrs):
                        for h in (0, 1):
                            for group in B128_GROUPS:
                                pos = [(addrs[(l, h)] % 256) // 16 for l in group]
                                assert len(set(pos)) == 16, f"bank conflict: {sorted(pos)}"
                # epilogue: lane holds 4 consecutive columns of one row
                for m in range(4):
                    for n in range(4):
                        for lane in range(WAVE):
                            fr, fg = lane & 15, lane >> 4
                            row = brow + wm * 64 + m * 16 + fr
                            col = bcol + wn * 64 + n * 16 + fg * 4
                            if row >= M or col >= N:
                                continue
                            for j in range(4):
                                assert col + j < N
                                assert (row, col + j) not in stored
                                # D[i = 4*fg + j][jj = fr] of the transposed tile:
                                # i indexes the weight row, jj the activation row
                                stored[(row, col + j)] = (
                                    brow + wm * 64 + m * 16 + fr, bcol + wn * 64 + n * 16 + 4 * fg + j)
    assert len(stored) == M * N, "some output element is never stored"
    for (row, col), src in stored.items():
        assert src == (row, col)


def test_fp8_swizzle_is_an_involution_on_slots():
    for r in range(128):
        seen = {c ^ _swz(r) for c in range(8)}
        assert seen == set(range(8))
        assert _swz(r) == _swz(r & 15) == _swz(r % 32)
