"""
The moved head carry of the streamed chol Q and b WITHOUT a GPU: tests/host_sim/q_move_b_head_sim.cpp compiles the kernel's own
layouts, decision helpers and two-word per-lane schedules (Stream<288, KeepLower<6, 8>, true> with MovedSchedule<., 2>, and
Stream<48, KeepAll, true, 1, true> with MovedSchedule, of markovflow_amd/csrc/mf_head_carry.hpp) for the CPU and walks a whole
wavefront - 64 chunks, every DMA instruction and lane, step after step, a chunk's first fetch whole and no fetch behind the last
step (`more == false`) - over a slot-by-slot model of the LDS image in which a slot that a masked-out lane leaves alone keeps what
it held and the lane copies its next row's carried head from the tail slots to the head slots at the top of every step:
  (a) every unit a consumer reads - always from the row's OWN slot - holds the bytes of its row and came the way the consumer
      expects: a carried unit by the previous fetch and the move, any other by this step's fetch;
  (b) no unit is lost when rows of chol Q carry on consecutive steps (32, 64, then 96 bytes into a line) out of one tail set;
  (c) the fetch of a row whose head is carried does not request the line that holds it, and nothing is fetched that nobody reads;
  (d) 128-B lines: chol Q 3, 2, 2, 2 = 9 per four steps for line-aligned bases (12 plain) - the 2.25 lines that hold the kept
      units; b 9 per eight steps (10 plain): the row that starts 112 bytes into a line no longer touches two.
The expected counts are worked out from the byte ranges of the kept units (see the docstrings), not from the walk.
What this does NOT cover is the memory side itself (LDS-DMA under an EXEC mask, the ds_read / ds_write move):
tests/test_gpu_kalman_q_move_b_head.py.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
LIB = os.path.join(HERE, "libmf_q_move_b_head_sim.so")
SRC = os.path.join(HERE, "q_move_b_head_sim.cpp")
HDR = os.path.join(os.path.dirname(HERE), "..", "markovflow_amd", "csrc", "mf_head_carry.hpp")

BASE = 0x7F0000001000
Q, B = 0, 1
LENGTHS = list(range(1, 12)) + [157]


@pytest.fixture(scope="module")
def lib():
    cxx = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cxx):
        cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler found")
    stale = not os.path.exists(LIB) or any(os.path.getmtime(f) > os.path.getmtime(LIB) for f in (SRC, HDR))
    if stale:
        subprocess.check_call([cxx, "-x", "c++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    so = ctypes.CDLL(LIB)
    so.mf_q_move_b_head_layout.restype = None
    so.mf_q_move_b_head_layout.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    so.mf_q_move_b_head_rule.restype = ctypes.c_uint
    so.mf_q_move_b_head_rule.argtypes = [ctypes.c_int, ctypes.c_int]
    so.mf_q_move_b_head_walk.restype = ctypes.c_int
    so.mf_q_move_b_head_walk.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_long, ctypes.POINTER(ctypes.c_double)]
    return so


def _walk(so, which, base, length):
    out = (ctypes.c_double * 6)()
    bad = so.mf_q_move_b_head_walk(which, base, length, out)
    return bad, dict(steps=out[0], lines=out[1], plain=out[2], carried=out[3], chunks=out[4], running=out[5])


def _layout(so, which):
    out = (ctypes.c_int * 8)()
    so.mf_q_move_b_head_layout(which, out)
    return list(out)


def test_layout_and_rule_of_chol_q(lib):
    # two tail slots (the next row's units 0 and 3), period 4, 12 + 2 units; a lane meets 2 head or tail units in every block of 7
    # instructions (two instructions apart), 2 such blocks: 4 x 2 x 2 = 16 fetch bits in word 0, word 1 holds 4 + 8 bits
    assert _layout(lib, Q) == [2, 4, 14, 7, 2, 2, 16, 12]
    # kept units: 0, 3, 6, 7, 9, ... - unit 0 is carried where the row's part of its first line ends before unit 6 (byte 96), unit 3
    # with it where that part reaches its end (byte 64)
    assert {r: lib.mf_q_move_b_head_rule(Q, r) for r in range(0, 128, 16)} == {0: 0, 16: 0, 32: 3, 48: 3, 64: 3, 80: 1, 96: 1, 112: 1}


def test_layout_and_rule_of_b(lib):
    # one tail slot (the next row's unit 0), period 8, 3 + 1 units; a lane moves the same unit in all 4 instructions (blocks of
    # one), at most one of them special: 8 x 4 x 1 = 32 fetch bits fill word 0, word 1 holds 4 + 8 bits
    assert _layout(lib, B) == [1, 8, 4, 1, 4, 1, 32, 12]
    # only the row whose part of its first line is exactly unit 0 carries it
    assert {r: lib.mf_q_move_b_head_rule(B, r) for r in range(0, 128, 16)} == {r: int(r == 112) for r in range(0, 128, 16)}
    assert all(lib.mf_q_move_b_head_rule(B, r) == 0 for r in range(0, 128, 4) if r % 16)


@pytest.mark.parametrize("which", [Q, B], ids=["cholQ", "b"])
@pytest.mark.parametrize("phase", range(0, 128, 16))
@pytest.mark.parametrize("length", LENGTHS)
def test_every_read_finds_the_unit_it_expects(lib, which, phase, length):
    """Every lane, every row byte phase, 1 ... 11 and 157 consecutive steps; the first fetch of a chunk is whole, nothing is
    fetched behind the last step."""
    bad, st = _walk(lib, which, BASE + phase, length)
    assert bad == 0, f"violations {bad:#x}"
    assert st["steps"] == 64 * length
    assert st["lines"] <= st["plain"] + st["chunks"]          # a chunk's first fetch: at most one line more than the plain row
    if which == Q and length >= 5:
        assert st["running"] > 0                              # rows did carry on consecutive steps
    if length >= 9:
        assert st["carried"] > 0


@pytest.mark.parametrize("which", [Q, B], ids=["cholQ", "b"])
@pytest.mark.parametrize("phase", range(8, 128, 16))
def test_rows_off_the_16_byte_grid(lib, which, phase):
    """8 bytes off the grid a unit of b straddles the end of the row's first line: nothing is carried.  chol Q drops the units in
    between, so its rows may still carry (the rule is the same function of the byte address): the walk holds there too."""
    bad, st = _walk(lib, which, BASE + phase, 9)
    assert bad == 0, f"violations {bad:#x}"
    if which == B:
        assert st["carried"] == 0


@pytest.mark.parametrize("phase,per_four,plain_per_four", [(0, 9, 12), (32, 9, 12), (64, 9, 12), (96, 9, 12),
                                                           (16, 10, 13), (48, 10, 13), (80, 10, 13), (112, 10, 13)])
def test_chol_q_lines_per_four_steps_on_long_chunks(lib, phase, per_four, plain_per_four):
    """Kept bytes of a row: [0, 16), [48, 64), [96, 128), [144, 176), [192, 288).  32-B aligned bases: a row 0 bytes into a line
    takes 3 lines; rows 32, 64 and 96 bytes in have only carried units in their first line and take the other 2: 9 per four steps,
    the 2.25 lines of data.  Bases that are only 16-B aligned: a row 16 bytes in takes 3; 48 and 80 bytes in 2 (first line
    carried); 112 bytes in its kept bytes end 400 bytes past the line's start: lines 1, 2, 3 without the carried first: 10, where
    the plain fetch takes 3 + 3 + 3 + 4."""
    length = 400
    bad, st = _walk(lib, Q, BASE + phase, length)
    assert bad == 0
    # (a chunk's first fetch takes the whole row, carried or not, and its tails unasked: at most two lines more per chunk)
    assert 0 <= 4 * st["lines"] - per_four * st["steps"] <= 4 * 2 * st["chunks"]
    assert st["plain"] / st["steps"] == plain_per_four / 4
    units = 5 if phase % 32 == 0 else 4                                      # 2 + 2 + 1, or 2 + 1 + 1, carried per four rows
    assert abs(4 * st["carried"] - units * st["steps"]) <= 4 * units * st["chunks"]       # (a chunk's step 0 carries nothing)


@pytest.mark.parametrize("phase", range(0, 128, 16))
def test_b_lines_per_eight_steps_on_long_chunks(lib, phase):
    """48-byte rows of a 16-B aligned base start 0, 48, 96, 16, 64, 112, 32, 80 bytes into a line in turn (every base runs through
    the same eight phases): the rows at 96 and 112 straddle two lines, 10 requests per eight steps; with unit 0 of the row at 112
    brought along by the row at 64, whose last unit shares its line, 9."""
    length = 400
    bad, st = _walk(lib, B, BASE + phase, length)
    assert bad == 0
    assert 0 <= 8 * st["lines"] - 9 * st["steps"] <= 8 * 2 * st["chunks"]
    assert st["plain"] / st["steps"] == 10 / 8
    assert abs(8 * st["carried"] - st["steps"]) <= 8 * st["chunks"]
    assert st["running"] == 0
