"""Row bookkeeping of conv_hx's halo carry (csrc/fastsvc_hx.hip, hx_carry), restated in Python - no GPU.

From a workgroup's second tile on the staging waves stage only the NT fresh rows of a window and copy the 2 halo_al rows it
shares with the previous tile's window out of LDS.  Checked here, for every (NT, halo_al, tiles, tiles per workgroup, K chunks)
the kernel takes that path with:
  * the item maps: the 256 staging threads' (2 channels, 8 rows) items cover the fresh rows x 32 channels exactly once, the
    16-byte carry pieces cover rows [0, 2 halo_al) exactly once, and through the tile swizzle (hx_lds_off) a piece's source
    is the same slot NT rows further down;
  * the schedule: replaying the staging waves' halves (request / carry read / carry write / commit / barrier) against the
    consumers' reads, every unit's window holds, row by row, the absolute time step and K chunk it stands for when the
    consumers multiply from it, nothing is written to a buffer while it is read, and every carried row was copied from a
    row of the same absolute time and chunk."""
import itertools

import pytest

HX_ROW = 64
NPROD = 256


def hx_lds_off(row, octet):
    return ((row ^ ((row >> 2) & 1)) * HX_ROW) + ((octet ^ ((row >> 1) & 2)) << 4)


def carries(NT, halo_al, tpw, nch):
    """the kernel's run-time gate (conv_hx_kernel, staging waves)"""
    return NT == 128 and tpw > 1 and nch <= 2 and 2 * halo_al <= NT and 8 * halo_al <= NPROD


HALOS = [8, 16, 24, 32]          # (dil + 7) & ~7 for every dilation the kernel takes (dil <= 28)


@pytest.mark.parametrize("halo_al", HALOS)
def test_fresh_items_cover_the_fresh_rows_once(halo_al):
    NT = 128
    W = NT + 2 * halo_al
    seen = {}
    for ptid in range(NPROD):
        pair, octet = ptid & 15, ptid >> 4
        for j in range(8):
            row = 2 * halo_al + 8 * octet + j
            off = hx_lds_off(row, pair >> 2) + (pair & 3) * 4          # 4 bytes: channels 2 pair, 2 pair + 1
            for byte in range(off, off + 4):
                assert byte not in seen
                seen[byte] = (row, pair)
    want = {hx_lds_off(r, s) + k for r in range(2 * halo_al, W) for s in range(4) for k in range(16)}
    assert set(seen) == want
    # a thread's 8 rows start at a multiple of 8 in time whatever the tile: the item lies inside the row or outside it
    assert (2 * halo_al) % 8 == 0 and NT % 8 == 0


@pytest.mark.parametrize("halo_al", HALOS)
def test_carry_pieces_cover_the_shared_rows_once(halo_al):
    NT = 128
    W = NT + 2 * halo_al
    slot_of = {hx_lds_off(r, s): (r, s) for r in range(W + 8) for s in range(4)}      # (+ the 8 spare rows)
    dst_rows = set()
    for ptid in range(NPROD):
        live = ptid < 8 * halo_al
        src = NT * HX_ROW + (ptid if live else 0) * 16
        dst = ptid * 16 if live else W * HX_ROW + (ptid & 31) * 16
        (rs, ss), (rd, sd) = slot_of[src], slot_of[dst]
        if not live:
            assert W <= rd < W + 8                                       # parked in the spare rows
            continue
        assert (rd, sd) not in dst_rows
        dst_rows.add((rd, sd))
        assert rs == rd + NT and ss == sd                                # same slot, NT rows down: the same absolute time
        assert hx_lds_off(rs, ss) - hx_lds_off(rd, sd) == NT * HX_ROW
    assert dst_rows == {(r, s) for r in range(2 * halo_al) for s in range(4)}
    # the source rows of a piece are fresh rows of the previous window (never carried ones): one copy deep
    assert NT >= 2 * halo_al


class Lds:
    """two window buffers of W (+ spare) rows; a row holds (absolute time, chunk) or None = never written"""

    def __init__(self, W):
        self.W = W
        self.buf = [[None] * (W + 8) for _ in range(2)]
        self.written = [set(), set()]                                   # rows written in the current half

    def write(self, b, row, val):
        self.buf[b][row] = val
        self.written[b].add(row)

    def barrier(self):
        self.written = [set(), set()]


def replay(NT, halo_al, ntiles_wg, nch, tile0):
    """the staging waves' schedule of one workgroup with the consumers' reads in between; returns the number of window
    rows staged from memory"""
    W = NT + 2 * halo_al
    nunits = ntiles_wg * nch
    lds = Lds(W)
    staged = 0

    def unit(un):
        return (tile0 + un // nch, un % nch)                            # (tile, chunk)

    def t_start(un):
        return unit(un)[0] * NT - halo_al

    def commit_full(un, b):
        nonlocal staged
        for r in range(W):
            lds.write(b, r, (t_start(un) + r, unit(un)[1]) if un < nunits else ("phantom", un))
        staged += W if un < nunits else 0

    def commit_fresh(un, b):
        nonlocal staged
        for r in range(2 * halo_al, W):
            lds.write(b, r, (t_start(un) + r, unit(un)[1]) if un < nunits else ("phantom", un))
        staged += NT if un < nunits else 0

    def cread(b):
        return [lds.buf[b][NT + r] for r in range(2 * halo_al)]

    def cwrite(b, rows, un):
        for r, v in enumerate(rows):
            if un < nunits:                                              # a carried row stands for the same time step and chunk
                assert v == (t_start(un) + r, unit(un)[1]), (un, r, v)
            lds.write(b, r, v)

    def consume(un):
        """the consumers multiply unit `un` from buffer un & 1 during the half that just ran: complete, and untouched"""
        if un >= nunits:
            return
        b = un & 1
        assert not lds.written[b], (un, sorted(lds.written[b])[:4])
        for r in range(W):
            assert lds.buf[b][r] == (t_start(un) + r, unit(un)[1]), (un, r, lds.buf[b][r])

    if nch == 1:
        commit_full(0, 0)
        lds.barrier()
        for u in range(0, nunits, 2):
            cwrite(1, cread(0), u + 1); commit_fresh(u + 1, 1)
            consume(u); lds.barrier()
            cwrite(0, cread(1), u + 2); commit_fresh(u + 2, 0)
            consume(u + 1); lds.barrier()
    else:
        commit_full(0, 0)
        lds.barrier()
        ca = cread(0)
        commit_full(1, 1)
        consume(0); lds.barrier()
        cb = cread(1)
        cwrite(0, ca, 2); commit_fresh(2, 0)
        consume(1); lds.barrier()
        for u in range(2, nunits, 2):
            ca = cread(0)
            cwrite(1, cb, u + 1); commit_fresh(u + 1, 1)
            consume(u); lds.barrier()
            cb = cread(1)
            cwrite(0, ca, u + 2); commit_fresh(u + 2, 0)
            consume(u + 1); lds.barrier()
    return staged


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("halo_al", HALOS)
def test_schedule_gives_every_unit_its_window(halo_al, nch):
    NT = 128
    for ntiles, tpw in itertools.product(range(1, 8), range(2, 9)):
        assert carries(NT, halo_al, tpw, nch)
        total = 0
        for tile0 in range(0, ntiles, tpw):
            n = min(tpw, ntiles - tile0)
            total += replay(NT, halo_al, n, nch, tile0)
        nwg = (ntiles + tpw - 1) // tpw
        # rows staged from memory: a whole window per workgroup and chunk, NT rows for every further tile
        assert total == nch * (nwg * (NT + 2 * halo_al) + (ntiles - nwg) * NT)


def test_gate():
    assert not carries(128, 32, 1, 1)            # one tile per workgroup: every tile is a first tile (the in-library reference)
    assert not carries(128, 32, 4, 3)            # three K chunks: the chunk's buffer has been overwritten in between
    assert not carries(128, 72, 4, 1)            # 2 halo_al > NT
    assert not carries(128, 40, 4, 1)            # more 16-byte carry pieces than staging threads
    assert not carries(192, 32, 4, 1)            # (192-column tiles keep the window items)
    assert carries(128, 16, 2, 2) and carries(128, 32, 24, 1)
