"""
The head carry of the streamed A WITHOUT a GPU: tests/host_sim/a_head_carry_sim.cpp compiles the kernel's own layout, decision
helpers and packed per-lane schedule (Stream<288, KeepAll, true>, HeadCarry, MaskedSchedule of markovflow_amd/csrc/
mf_head_carry.hpp) for the CPU and walks a whole wavefront - 64 chunks, every DMA instruction and lane, step after step - over a
model of the LDS image in which a slot that a masked-out lane leaves alone keeps what it held:
  (a) every unit a consumer reads holds the bytes of its row and was written by exactly the fetch the consumer expects: its own
      slots by this step's fetch, a tail slot by the previous step's - never rewritten in between;
  (b) the fetch of a row whose head is carried does not touch the line that holds it, and nothing is fetched that nobody reads;
  (c) 128-B lines over four steps: 3, 3, 3, 2 = 11 for line-aligned bases (12 without the carry).
What this does NOT cover is the memory side itself (LDS-DMA under an EXEC mask, y through registers):
tests/test_gpu_kalman_a_head_carry.py.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
LIB = os.path.join(HERE, "libmf_a_head_carry_sim.so")
SRC = os.path.join(HERE, "a_head_carry_sim.cpp")
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
    so.mf_a_head_carry_layout.restype = None
    so.mf_a_head_carry_layout.argtypes = [ctypes.POINTER(ctypes.c_int)]
    so.mf_a_head_carry_rule.restype = ctypes.c_uint
    so.mf_a_head_carry_rule.argtypes = [ctypes.c_int]
    so.mf_a_head_carry_walk.restype = ctypes.c_int
    so.mf_a_head_carry_walk.argtypes = [ctypes.c_uint64, ctypes.c_long, ctypes.POINTER(ctypes.c_double)]
    return so


def _walk(so, base, length):
    out = (ctypes.c_double * 5)()
    bad = so.mf_a_head_carry_walk(base, length, out)
    return bad, dict(steps=out[0], lines=out[1], plain=out[2], carried=out[3], chunks=out[4])


def test_layout_and_rule(lib):
    out = (ctypes.c_int * 8)()
    lib.mf_a_head_carry_layout(out)
    # two tail slots (the next row's units 0 and 1), period 4, 18 + 2 units; a lane meets its one head or tail unit once in every
    # 5 instructions, 4 such blocks; 4 + 16 + 8 schedule bits in one word
    assert list(out) == [2, 0, 1, 4, 20, 5, 4, 28]
    # a row carries where its part of its first line is at most 32 bytes: units 0 and 1 at 96, unit 0 at 112, nothing elsewhere
    assert {r: lib.mf_a_head_carry_rule(r) for r in range(0, 128, 16)} == {0: 0, 16: 0, 32: 0, 48: 0, 64: 0, 80: 0, 96: 3, 112: 1}


@pytest.mark.parametrize("phase", range(0, 128, 16))
@pytest.mark.parametrize("length", list(range(1, 10)) + [157])
def test_every_read_finds_the_fetch_it_expects(lib, phase, length):
    bad, st = _walk(lib, BASE + phase, length)
    assert bad == 0, f"violations {bad:#x}"
    assert st["steps"] == 64 * length
    assert st["lines"] <= st["plain"] + st["chunks"]          # a chunk's first fetch: at most one line more than the plain row


@pytest.mark.parametrize("phase,per_four,plain_per_four", [(0, 11, 12), (32, 11, 12), (64, 11, 12), (96, 11, 12),
                                                           (16, 12, 13), (48, 12, 13), (80, 12, 13), (112, 12, 13)])
def test_lines_per_four_steps_on_long_chunks(lib, phase, per_four, plain_per_four):
    """Line-aligned (32-B aligned) bases: 3, 3, 3, 2.  Bases that are only 16-B aligned: a row touches 3, 3, 3, 4 lines and the row
    112 bytes into a line carries unit 0 only, but that was all it had in its first line: 3, 3, 3, 3."""
    length = 400
    bad, st = _walk(lib, BASE + phase, length)
    assert bad == 0
    # (a chunk's first fetch takes the whole row, carried or not, and its tails unasked: at most two lines more per chunk)
    assert 0 <= 4 * st["lines"] - per_four * st["steps"] <= 4 * 2 * st["chunks"]
    assert st["plain"] / st["steps"] == plain_per_four / 4
    units = 2 if phase % 32 == 0 else 1                                      # carried by every fourth row (never by step 0)
    assert abs(4 * st["carried"] - units * st["steps"]) <= 4 * units * st["chunks"]       # (a chunk's step 0 carries nothing)
