"""CPU checks of the recovery pool's multi-loss entry points: declared in the header,
exported by the library, bound by cocytus_amd.ec; refused with a NULL pool without a
launch; and the pool's host bookkeeping (cec_poolbook.hpp) under ASan + UBSan in a
stand-alone program."""
from __future__ import annotations

import ctypes
import os
import subprocess

import pytest

import test_abi

ROOT = test_abi.ROOT
NEW = ["cec_recovery_pool_parity_staging", "cec_recovery_pool_add_residual", "cec_recovery_pool_add_residuals",
       "cec_recovery_pool_ready", "cec_recovery_pool_output_lost"]


@pytest.fixture(scope="module")
def lib():
    from cocytus_amd import build, ec

    build.build(verbose=False)
    return ec


def test_new_symbols_declared_exported_bound(lib):
    decl = test_abi.declared_functions()
    syms = test_abi.exported_symbols(lib.LIB_PATH)
    for name in NEW:
        assert name in decl, f"{name} is not declared in include/cocytus_ec.h"
        assert name in syms, f"{name} is not exported"
        assert getattr(lib.lib(), name).argtypes is not None, f"{name} is not bound"
    for method in ("parity_staging", "add_residual", "add_residuals", "ready", "output"):
        assert callable(getattr(lib.RecoveryPool, method))


def test_null_pool_is_refused_without_a_launch(lib):
    c = lib.lib()
    seq0 = lib.last_launch()["seq"]
    n = ctypes.c_size_t(7)
    buf = (ctypes.c_uint8 * 4096)()
    ids, lids = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(4)
    ptrs = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    assert not c.cec_recovery_pool_parity_staging(None, 0, 4, ctypes.byref(n))
    assert not c.cec_recovery_pool_output_lost(None, 0, 0, ctypes.byref(n))
    assert n.value == 7
    assert c.cec_recovery_pool_add_residual(None, 0, 4, ctypes.addressof(buf)) == lib.CEC_EINVAL
    assert c.cec_recovery_pool_add_residuals(None, ids, lids, ptrs, 1) == lib.CEC_EINVAL
    assert c.cec_recovery_pool_ready(None, 0) == 0
    assert lib.last_launch()["seq"] == seq0


def test_pool_bookkeeping_under_sanitizers(tmp_path):
    """cec_poolbook.hpp as shipped, included by tests/drain_c/pool_book_main.cpp: the slot
    layout of a flush for every (k, m) (distinct slots, 42 of 48 at RS(16,8), k inputs at
    most), readiness against brute force, the batch check (first refusal, repeated pairs,
    nothing changed) on 4,000 random batches, and the pattern keys."""
    exe = tmp_path / "pool_book_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cocytus_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "drain_c", "pool_book_main.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr[-2000:]
