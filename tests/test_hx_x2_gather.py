"""Host-side arithmetic of the raw LDS tile the staging waves fetch the stretched residual operand through (S = 4 / 5,
2-byte storage; csrc/fastsvc_hx.hip, hx_x2_gather / F_X2_GATHER): the workgroup's LDS with the tile added, the columns
the tile must hold for every tile start and window length, the gather's indices and its LDS banks.  No GPU."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svcc23_fastsvc_amd", "csrc")


@pytest.fixture(scope="module")
def tile():
    """the tile's constants as the kernel file states them"""
    src = open(os.path.join(CSRC, "fastsvc_hx.hip")).read()
    env = {}
    for name in ("HX_X2G_COLS", "HX_X2G_ROW", "HX_X2G_GROUP", "HX_X2G_BYTES"):
        expr = re.search(rf"constexpr int {name} = ([^;]+);", src).group(1)
        env[name] = eval(expr, {}, env)
    # the launcher's window gate: W <= (HX_X2G_COLS - 8) * s2 + 1
    assert "W <= (HX_X2G_COLS - 8) * p.s2 + 1" in src
    return env


def _window_ok(tile, W, S):
    return W <= (tile["HX_X2G_COLS"] - 8) * S + 1


def test_tile_layout(tile):
    assert tile["HX_X2G_COLS"] == 64 and tile["HX_X2G_ROW"] == 128              # 8 pieces of 16 bytes per channel row
    assert tile["HX_X2G_GROUP"] % 16 == 0 and tile["HX_X2G_BYTES"] == 4 * tile["HX_X2G_GROUP"]
    assert tile["HX_X2G_GROUP"] >= 8 * tile["HX_X2G_ROW"]                         # 8 channel rows per group, then the skew


def test_two_workgroups_with_the_raw_tile_fit_the_lds_of_a_cu(tile):
    """hx_launch_shape's dynamic LDS of the two-per-CU instances that take a second operand - C = 48 (MW 3, two K chunks,
    S = 4) and C = 24 (MW 2, one chunk, S = 5), NW 2 x WN 4 - with the raw tile, plus the static part, for every dilation
    the kernel takes: at most half of a CU's 160 KB (tests/test_hx_budget.py::test_two_workgroups_fit_the_lds_of_a_cu
    without the tile)."""
    NW, WN = 2, 4
    for MW, KC32, S in ((3, 2, 4), (2, 1, 5)):
        for dil in range(1, 29):
            halo_al = (dil + 7) & ~7
            W = 16 * NW * WN + 2 * halo_al
            assert _window_ok(tile, W, S), (dil, W, S)
            smem = 8 * 2 * 16 * MW + 4 * 2 * (KC32 * 32 + 8) + 2 * (W + 8) * 64        # sums | prologue coefficients | two windows
            smem += 4 * 4 * 2 * (MW * (NW // 2) * 256)                                # scale and shift slots of four waves
            smem += 4 * 4 * 16 * 36                                                    # re-layout patches
            smem += 4 * MW * 2 * 64 * 8                                                # the lanes' float64 InstanceNorm sums
            smem += tile["HX_X2G_BYTES"]                                               # the second operand's raw tile
            assert smem + 4096 <= 80 * 1024, (MW, S, dil, smem)


def _starts(S):
    """tile starts t_start = tile * NT - halo_al: multiples of 8 - the negative ones of a row's first tile and every
    residue modulo 8 S (twice over)"""
    return range(-32, 16 * S + 8, 8)


WINDOWS = sorted({nt + 2 * h for nt in (128, 192) for h in (8, 16, 24, 32)})


@pytest.mark.parametrize("S", [4, 5])
def test_tile_columns_cover_every_window(tile, S):
    """columns floor((t_start + r) / S), r < W, against the tile's 64 columns from j0 = floor(t_start / S) & ~7 on - and
    the commit's lane map (thread xg: column g0 + xg -> rows r0 .. r0 + S) against the column every row must show"""
    cols = tile["HX_X2G_COLS"]
    checked = 0
    for W in WINDOWS:
        for t_start in _starts(S):
            g0 = int((t_start + 8 * S) / S) - 8                  # the kernel's form: C division of a non-negative numerator
            assert t_start + 8 * S >= 0 and g0 == t_start // S
            j0 = g0 & ~7
            assert j0 % 8 == 0 and j0 <= g0 < j0 + 8
            need = [(t_start + r) // S for r in range(W)]
            if not _window_ok(tile, W, S):
                continue
            checked += 1
            assert j0 <= min(need) and max(need) < j0 + cols, (S, W, t_start, j0, max(need))
            # every 16-byte piece (8 columns from a multiple of 8 on) lies wholly before column 0 or starts at >= 0
            assert all((j0 + 8 * pc) % 8 == 0 for pc in range(cols // 8))
            seen = {}
            for xg in range(64):
                ci = min((g0 & 7) + xg, cols - 1)               # the gather's column index inside the tile
                r0 = (g0 + xg) * S - t_start
                for ph in range(S):
                    r = r0 + ph
                    if 0 <= r < W:
                        assert (g0 & 7) + xg <= cols - 1 and j0 + ci == need[r], (S, W, t_start, xg, r)
                        seen[r] = seen.get(r, 0) + 1
            assert len(seen) == W and set(seen.values()) == {1}, (S, W, t_start)     # every window row written once
    assert checked > 0


def test_the_window_gate_is_not_vacuous(tile):
    """a window the gate refuses really needs more than the tile's columns at some start (S = 4, 192-column tiles,
    dilation > 16)"""
    S, W = 4, 192 + 2 * 32
    assert not _window_ok(tile, W, S)
    worst = max((t + W - 1) // S - ((t // S) & ~7) + 1 for t in _starts(S))
    assert worst > tile["HX_X2G_COLS"]


def test_the_tail_of_a_piece_that_straddles_the_row_end_is_zeroed():
    """the raw commit's mask per dword k of a piece with nv columns inside the row: both halves, the low one, none"""
    for nv in range(0, 9):
        keep = []
        for k in range(4):
            m = 0xFFFFFFFF if nv >= 2 * k + 2 else 0x0000FFFF if nv == 2 * k + 1 else 0
            keep += [bool(m & 0xFFFF), bool(m >> 16)]
        assert keep == [e < nv for e in range(8)], nv


def test_gather_reads_spread_over_the_banks(tile):
    """one gather instruction of a wave: lanes (octet = lane & 3, column xg0 + (lane >> 2)) read 2 bytes of channel row
    8 octet + c; on the LDS's 64 four-byte banks no bank serves more than two different words"""
    for off in range(8):
        for c in range(8):
            for xg0 in (0, 16, 32, 48):
                words = {}
                for lane in range(64):
                    ci = min(off + xg0 + (lane >> 2), tile["HX_X2G_COLS"] - 1)
                    addr = (lane & 3) * tile["HX_X2G_GROUP"] + c * tile["HX_X2G_ROW"] + ci * 2
                    assert addr + 2 <= tile["HX_X2G_BYTES"]
                    words.setdefault((addr // 4) % 64, set()).add(addr // 4)
                assert max(len(w) for w in words.values()) <= 2, (off, c, xg0)
