"""
The head-carry decisions of the streamed chol Q WITHOUT a GPU: tests/host_sim/head_carry_sim.cpp compiles the kernel's own layout
and decision helpers (markovflow_amd/csrc/mf_head_carry.hpp, plain constexpr integer arithmetic on byte addresses) for the CPU and
walks consecutive rows as the producer (the DMA lane that fetches a unit) and the consumer (the lane that reads the row) take them:
  (a) the consumer's schedule equals the address rule, and producer and consumer agree for every row;
  (b) every kept unit of every row is either fetched into its slot or carried - exactly one of the two;
  (c) 128-B lines touched per step: 2.25 instead of 3.0 for d = 6 fp64 on long chunks (32-B aligned bases), 2.5 instead of 3.25
      for bases that are only 16-B aligned.
What this does NOT cover is the kernel's memory side (LDS-DMA, the registers that hold the carry): tests/test_gpu_kalman_head_carry.py.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sim")
LIB = os.path.join(HERE, "libmf_head_carry_sim.so")
SRC = os.path.join(HERE, "head_carry_sim.cpp")
HDR = os.path.join(os.path.dirname(HERE), "..", "markovflow_amd", "csrc", "mf_head_carry.hpp")

ROWS = 4096


def _lib():
    cxx = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cxx):
        cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler found")
    stale = not os.path.exists(LIB) or any(os.path.getmtime(f) > os.path.getmtime(LIB) for f in (SRC, HDR))
    if stale:
        subprocess.check_call([cxx, "-x", "c++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.mf_head_carry_layout.restype = ctypes.c_int
    lib.mf_head_carry_layout.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.mf_head_carry_walk.restype = ctypes.c_int
    lib.mf_head_carry_walk.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_long, ctypes.c_long,
                                       ctypes.POINTER(ctypes.c_double)]
    return lib


def _walk(lib, d, s, tail, base, rows, length):
    out = (ctypes.c_double * 5)()
    bad = lib.mf_head_carry_walk(d, s, int(tail), base, rows, length, out)
    assert bad >= 0, "case not instantiated"
    return bad, dict(rows=out[0], lines=out[1], plain=out[2], carried=out[3], chunks=out[4])


def test_layout_of_the_fp64_d6_stream():
    lib = _lib()
    out = (ctypes.c_int * 5)()
    assert lib.mf_head_carry_layout(6, 8, out) == 0
    # two tail slots: the next row's units 0 and 3 (C[0][0]; C[1][0], C[1][1]); decisions repeat every 4 steps; 12 + 2 units
    assert list(out) == [2, 0, 3, 4, 14]
    assert lib.mf_head_carry_layout(4, 8, out) == 0
    assert out[0] == 0                      # rows are whole lines: nothing to carry


@pytest.mark.parametrize("phase", range(0, 128, 16))
@pytest.mark.parametrize("length", list(range(1, 10)) + [157, ROWS])
def test_producer_and_consumer_agree_and_no_unit_is_lost(phase, length):
    lib = _lib()
    bad, st = _walk(lib, 6, 8, True, 0x7F0000001000 + phase, ROWS, length)
    assert bad == 0, f"violations {bad:#x}"
    assert st["rows"] == ROWS
    assert st["lines"] <= st["plain"] + st["chunks"]          # a chunk's first fetch: at most one line more than the plain row


@pytest.mark.parametrize("phase,want,plain", [(0, 2.25, 3.0), (32, 2.25, 3.0), (64, 2.25, 3.0), (96, 2.25, 3.0),
                                              (16, 2.5, 3.25), (48, 2.5, 3.25), (80, 2.5, 3.25), (112, 2.5, 3.25)])
def test_lines_per_step_on_long_chunks(phase, want, plain):
    lib = _lib()
    bad, st = _walk(lib, 6, 8, True, 0x7F0000001000 + phase, ROWS, ROWS)
    assert bad == 0
    assert abs(st["lines"] / ROWS - want) <= 2.0 / ROWS          # (a chunk's first fetch takes its tails unconditionally)
    bad, st0 = _walk(lib, 6, 8, False, 0x7F0000001000 + phase, ROWS, ROWS)
    assert bad == 0 and st0["carried"] == 0
    assert abs(st0["lines"] / ROWS - plain) <= 2.0 / ROWS
    assert st0["lines"] == st0["plain"]
    # chunks of the headline partition (157 steps): the first fetch of each chunk costs at most one line more
    bad, st157 = _walk(lib, 6, 8, True, 0x7F0000001000 + phase, ROWS, 157)
    assert bad == 0
    assert st157["lines"] / ROWS <= want + 2.0 / 157


@pytest.mark.parametrize("d,s", [(6, 4), (5, 8), (7, 8), (3, 8), (4, 8)])
@pytest.mark.parametrize("length", [1, 2, 3, 5, 8, 33, ROWS])
def test_the_rule_holds_for_other_row_sizes(d, s, length):
    """The helpers are generic in (d, element size); the kernel enables the tail only where it fits (fp64 d = 6), but the
    decisions must be consistent wherever the set of tail units is not empty."""
    lib = _lib()
    for phase in range(0, 128, s):
        bad, st = _walk(lib, d, s, True, 0x7F0000002000 + phase, ROWS, length)
        assert bad == 0, f"phase {phase}: violations {bad:#x}"
