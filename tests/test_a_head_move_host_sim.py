"""
The moved head carry of the streamed A WITHOUT a GPU: tests/host_sim/a_head_move_sim.cpp compiles the kernel's own layout, decision
helpers and two-word per-lane schedule (Stream<288, KeepAll, true, 4>, HeadCarry with four tail units, MovedSchedule of
markovflow_amd/csrc/mf_head_carry.hpp) for the CPU and walks a whole wavefront - 64 chunks, every DMA instruction and lane, step
after step - over a model of the LDS image in which a slot that a masked-out lane leaves alone keeps what it held and the lane
copies its next row's carried head from the tail slots to the head slots at the top of every step:
  (a) every unit a consumer reads - always from the row's OWN slot - holds the bytes of its row and came the way the consumer
      expects: a carried unit by the previous step's fetch and the move, any other by this step's fetch;
  (b) no unit is lost when rows carry on consecutive steps (64 then 96 bytes into a line, or 80 then 112), although there is one
      tail set: the move never reads a tail slot that a later fetch has overwritten;
  (c) the fetch of a row whose head is carried does not touch the line that holds it, and nothing is fetched that nobody reads;
  (d) 128-B lines over four steps: 3, 3, 2, 2 = 10 for line-aligned bases (11 with the carry at 96 alone, 12 without any).
What this does NOT cover is the memory side itself (LDS-DMA under an EXEC mask, the ds_read / ds_write move, H and y through
registers): tests/test_gpu_kalman_a_head_move.py.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
LIB = os.path.join(HERE, "libmf_a_head_move_sim.so")
SRC = os.path.join(HERE, "a_head_move_sim.cpp")
HDR = os.path.join(os.path.dirname(HERE), "..", "markovflow_amd", "csrc", "mf_head_carry.hpp")

BASE = 0x7F0000001000


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
    so.mf_a_head_move_layout.restype = None
    so.mf_a_head_move_layout.argtypes = [ctypes.POINTER(ctypes.c_int)]
    so.mf_a_head_move_rule.restype = ctypes.c_uint
    so.mf_a_head_move_rule.argtypes = [ctypes.c_int]
    so.mf_a_head_move_walk.restype = ctypes.c_int
    so.mf_a_head_move_walk.argtypes = [ctypes.c_uint64, ctypes.c_long, ctypes.POINTER(ctypes.c_double)]
    return so


def _walk(so, base, length):
    out = (ctypes.c_double * 6)()
    bad = so.mf_a_head_move_walk(base, length, out)
    return bad, dict(steps=out[0], lines=out[1], plain=out[2], carried=out[3], chunks=out[4], running=out[5])


def test_layout_and_rule(lib):
    out = (ctypes.c_int * 8)()
    lib.mf_a_head_move_layout(out)
    # four tail slots (the next row's units 0 ... 3), period 4, 18 + 4 units; a lane meets 4 head or tail units, at consecutive
    # instructions, in every block of 11, 2 such blocks: 4 x 2 x 4 = 32 fetch bits fill word 0, word 1 holds 4 + 16 bits
    assert list(out) == [4, 4, 22, 11, 2, 4, 32, 20]
    # a row carries where its part of its first line is at most 64 bytes, and then all of that part
    assert {r: lib.mf_a_head_move_rule(r) for r in range(0, 128, 16)} == {0: 0, 16: 0, 32: 0, 48: 0, 64: 15, 80: 7, 96: 3, 112: 1}
    # a row that is not 16-byte aligned has a unit that straddles the end of its first line: it carries nothing
    assert all(lib.mf_a_head_move_rule(r) == 0 for r in range(0, 128, 4) if r % 16)


@pytest.mark.parametrize("phase", range(0, 128, 16))
@pytest.mark.parametrize("length", list(range(1, 10)) + [157])
def test_every_read_finds_the_unit_it_expects(lib, phase, length):
    bad, st = _walk(lib, BASE + phase, length)
    assert bad == 0, f"violations {bad:#x}"
    assert st["steps"] == 64 * length
    assert st["lines"] <= st["plain"] + st["chunks"]          # a chunk's first fetch: at most one line more than the plain row
    if length >= 5:
        assert st["running"] > 0                              # rows did carry on consecutive steps


@pytest.mark.parametrize("phase", range(4, 128, 16))
def test_rows_off_the_16_byte_grid_carry_nothing(lib, phase):
    bad, st = _walk(lib, BASE + phase, 9)
    assert bad == 0, f"violations {bad:#x}"
    assert st["carried"] == 0


@pytest.mark.parametrize("phase,per_four,plain_per_four", [(0, 10, 12), (32, 10, 12), (64, 10, 12), (96, 10, 12),
                                                           (16, 11, 13), (48, 11, 13), (80, 11, 13), (112, 11, 13)])
def test_lines_per_four_steps_on_long_chunks(lib, phase, per_four, plain_per_four):
    """Line-aligned (32-B aligned) bases: 3, 3, 2, 2 = 10 where the carry at 96 alone had 3, 3, 3, 2 = 11.  Bases that are only
    16-B aligned: a row touches 3, 3, 3, 4 lines; the row 80 bytes into a line carries units 0 ... 2, all it had in its first line,
    and the row 112 bytes in carries unit 0, likewise: 3, 3, 2, 3 = 11 where the carry at 96 and 112 alone had 12."""
    length = 400
    bad, st = _walk(lib, BASE + phase, length)
    assert bad == 0
    # (a chunk's first fetch takes the whole row, carried or not, and its tails unasked: at most two lines more per chunk)
    assert 0 <= 4 * st["lines"] - per_four * st["steps"] <= 4 * 2 * st["chunks"]
    assert st["plain"] / st["steps"] == plain_per_four / 4
    units = 6 if phase % 32 == 0 else 4                                      # 4 + 2, or 3 + 1, carried per four rows
    assert abs(4 * st["carried"] - units * st["steps"]) <= 4 * units * st["chunks"]       # (a chunk's step 0 carries nothing)
    assert abs(4 * st["running"] - st["steps"]) <= 4 * 2 * st["chunks"]                   # one row in four follows a carrying row
