"""CPU: the SET path's digest op -- its declarations and bindings, its launch planning under
ASan + UBSan, and the model the GPU file (tests/test_gpu_digest_set.py) takes its expected
bytes from.

The model (tests/digest_set_case.py) applies a SET batch to all five arenas of an RS(3,2)
group in numpy; the digests of every arena after the batch must equal the positioned fold of
new ^ old (tests/digest_update_case.py) into the digests before it, with the identity row for
the source data lid and the matrix row for a parity.  No GPU, no library arithmetic.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_set_case as sc  # noqa: E402
import digest_update_case as uc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("cec_digest_set", "cec_diff_update_digests")


def test_header_declares_and_library_resolves_the_new_functions():
    from cocytus_amd import build, ec

    build.build(verbose=False)
    text = open(os.path.join(ROOT, "include", "cocytus_ec.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ec.lib()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in ec._SIGS and getattr(L, name).restype is ec._i, name
    assert callable(ec.digest_set) and callable(ec.diff_update_digests)
    assert re.search(r"CEC_KERNEL_DIGEST_SET\s*=\s*7\b", src)
    assert ec.CEC_KERNEL_DIGEST_SET == 7
    # LIVE DIGESTS points the SET path at the new op, and no longer says it cannot keep them
    live = text[text.index("LIVE DIGESTS: a process may keep"):text.index("#define CEC_DIGEST_BYTES")]
    assert "cec_diff_update_digests" in live
    assert "its fused path does not keep digests" not in text
    assert "cec_encode_region" in live  # the digests of a full-stripe encode, by linearity


def test_refusals_that_need_no_device():
    """A bad code and a NULL argument are answered before the library looks for a device."""
    from cocytus_amd import build, ec

    build.build(verbose=False)
    one = [0x1000]
    for call in (
        lambda: ec.digest_set(0, 2, sc.RS32, one, 0x1000, None, None, 8, _NoPlan()),
        lambda: ec.digest_set(3, 9, sc.RS32, one, 0x1000, None, None, 8, _NoPlan()),
        lambda: ec.diff_update_digests(17, 2, sc.RS32, one, 0x1000, one, True, one, one, 8, _NoPlan()),
    ):
        with pytest.raises(ec.CecError) as ei:
            call()
        assert ei.value.code == ec.CEC_EINVAL and "unsupported code" in str(ei.value)
    for call in (
        lambda: ec.digest_set(3, 2, sc.RS32, [1, 2, 3], 0x1000, None, None, 8, _NoPlan()),
        lambda: ec.digest_set(3, 2, sc.RS32, None, 0x1000, None, None, 8, _NoPlan()),
        lambda: ec.diff_update_digests(3, 2, sc.RS32, [1, 2, 3], 0x1000, [1, 2], True, None, None, 8, _NoPlan()),
        lambda: ec.diff_update_digests(3, 2, sc.RS32, [1, 2, 3], None, [1, 2], True, None, None, 8, _NoPlan()),
    ):
        with pytest.raises(ec.CecError) as ei:
            call()
        assert ei.value.code == ec.CEC_EINVAL and "NULL" in str(ei.value)


class _NoPlan:
    handle = None


def test_plan_digest_set_under_sanitizers(tmp_path):
    """plan_digest_set (cec_launchplan.hpp), included from the shipped header by
    tests/drain_c/digest_set_plan_main.cpp and run under ASan + UBSan: nothing at 0 tiles,
    grid 1, 1, 1, 2 at 1, 3, 4, 5 tiles, the limit of one dispatch held and one above it
    refused, and every field of the launch record."""
    exe = tmp_path / "digest_set_plan_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cocytus_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    "-pthread", "-o", str(exe), os.path.join(ROOT, "tests", "drain_c", "digest_set_plan_main.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr[-2000:]


@pytest.mark.parametrize("install", [True, False], ids=["install", "no-install"])
def test_the_model_is_pinned(install):
    """For uc.EXTENTS on RS(3,2): fold_into_digests(region_digests(before), new ^ old, rows, row)
    equals region_digests(after) for each of the five arenas -- identity row for the source
    data lid (zero without install: the data arenas do not change), the matrix row for a
    parity -- and units no tile touches keep their digests."""
    k, m, mat = 3, 2, sc.RS32
    rows = sc.rows_for(k)
    assert rows == uc.packed(uc.EXTENTS)
    data, parity, staging = sc.random_group(k, m, mat, rows, seed=1)
    d_after, p_after = sc.set_model(mat, k, m, data, parity, staging, rows, install)
    diffs = sc.diffs_of(data, staging, rows)
    assert diffs.any()
    for lid in range(k + m):
        before = (data + parity)[lid]
        after = (d_after + p_after)[lid]
        if lid < k:
            row = uc.identity_row(k, lid) if install else [0] * k
            assert np.array_equal(after, before) == (not install)
        else:
            row = sc.row_of(mat, k, lid)
            assert not np.array_equal(after, before)
        folded = uc.fold_into_digests(uc.region_digests(before), diffs, rows, row)
        assert np.array_equal(folded, uc.region_digests(after)), lid
        touched = {off // uc.TILE for off, _, _, j in uc.tiles_of(rows) if row[j]}
        for u in set(range(uc.N_UNITS)) - touched:
            assert np.array_equal(folded[u], uc.region_digests(before)[u]), (lid, u)
    # the same through the helper the GPU file calls, with a lost parity as well
    assert len(sc.digests_after(mat, k, m, data, parity, staging, rows, install)) == k + m
    lost = sc.digests_after(mat, k, m, data, parity, staging, rows, install, lost=(1,))
    assert np.array_equal(lost[k + 1], uc.region_digests(parity[1]))


def test_rows_of_the_larger_codes_name_every_lid():
    assert len(uc.EXTENTS) == 11
    assert [j for _, _, _, j in sc.rows_for(11)] == list(range(11))
    assert {j for _, _, _, j in sc.rows_for(6)} == set(range(6))
