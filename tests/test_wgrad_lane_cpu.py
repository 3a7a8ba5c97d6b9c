"""Host logic of calm_gemm's side lane without a GPU: the CALM_GEMM_OPT_LANE option round trip, fork and join that have
nothing to do issue nothing (no runtime call: they answer on a host without a device), the Python switch, and the
bookkeeping of csrc/gemm_lane.h — event ring, fork / launch / join counters, capture, devices, failures, two threads — in
the stand-alone program tests/host/lane_book_main.cpp, which drives it with a recording stub in place of the runtime."""
import ctypes
import os
import subprocess
import sys
from importlib import import_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
binding = import_module("calm_vit_dte_amd._lib")
backend = import_module("calm_vit_dte_amd.backend")
ops = import_module("calm_vit_dte_amd.ops")
OPT_LANE = 3


def _stats(lib):
    out = (ctypes.c_int64 * 4)()
    assert lib.calm_gemm_lane_stats(ctypes.byref(out)) == 0
    return list(out)


def test_option_round_trip():
    lib = binding.load()
    assert backend.HipBackend.GEMM_OPT_LANE == OPT_LANE
    header = open(os.path.join(ROOT, "include", "calm_vit.h")).read()
    assert "#define CALM_GEMM_OPT_LANE 3" in header
    prev = lib.calm_gemm_set_option(OPT_LANE, 1)
    try:
        assert prev in (0, 1)
        assert lib.calm_gemm_set_option(OPT_LANE, 0) == 1          # the previous value comes back
        assert lib.calm_gemm_set_option(OPT_LANE, 0) == 0
        assert lib.calm_gemm_set_option(OPT_LANE, 2) == binding.E_INVAL and lib.calm_gemm_set_option(OPT_LANE, -1) == binding.E_INVAL
        assert lib.calm_gemm_set_option(OPT_LANE + 1, 1) == binding.E_INVAL
        assert lib.calm_gemm_set_option(OPT_LANE, 0) == 0          # a rejected value changed nothing
    finally:
        lib.calm_gemm_set_option(OPT_LANE, prev)


def test_fork_and_join_with_nothing_to_do_issue_nothing():
    """Option off: a fork does nothing.  No launch on the lane: a join does nothing.  Neither reaches the runtime, so
    both return 0 here, and no counter moves."""
    lib = binding.load()
    prev = lib.calm_gemm_set_option(OPT_LANE, 0)
    try:
        before = _stats(lib)
        assert lib.calm_gemm_lane_fork(None) == 0
        assert lib.calm_gemm_lane_join(None) == 0
        assert _stats(lib) == before
        assert lib.calm_gemm_lane_stats(None) == binding.E_INVAL
    finally:
        lib.calm_gemm_set_option(OPT_LANE, prev)


def test_python_switch_follows_the_environment_and_leaves_a_disarmed_backward_alone():
    assert backend._wgrad_lane is (os.environ.get("CALM_WGRAD_LANE", "1") != "0")          # on unless CALM_WGRAD_LANE=0
    prev = backend.get_wgrad_lane()
    try:
        backend.set_wgrad_lane(True)
        assert backend.get_wgrad_lane() is True and backend.wgrad_lane()
        # the tail is not armed (a plain loss.backward()): no weight gradient takes the lane, whatever the switch says
        assert not ops._tail.armed and not ops._wgrad_on_lane(object(), object())
    finally:
        backend.set_wgrad_lane(prev)
    assert ops._tail.lane == []


def test_lane_bookkeeping_program(tmp_path):
    exe = str(tmp_path / "lane_book")
    subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "calm-vit-dte_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "lane_book_main.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "lane_book: ok" in run.stdout, run.stdout + run.stderr
