"""The write-through tail of large launches (DESIGN.md §4 *Store policy*), on the GPU.

A launch that streams more than CEC_WT_MAX_BYTES keeps non-temporal stores for its body and
writes its last CEC_WT_TAIL_BYTES (all outputs together) through: work items g >= wt_from
take the write-through store.  The choice must change which store instruction writes a
byte and nothing else, so every case here compares the whole slab with the oracle
(tests/store_tail_case.py: every output byte, and every byte around every extent) and
asserts the launch record's flag bits and wt_from.

The library reads its environment once per process: every case is a child process under
CEC_WT_MAX_BYTES=0 (so that these small launches take the non-temporal body) and its own
CEC_WT_TAIL_BYTES.  The expected wt_from is plain arithmetic, written out at each case:
a work item writes lt * (4096 >> split_shift) bytes, the tail is ceil(T / that) items.
"""
from __future__ import annotations

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = ("CEC_STORE_POLICY", "CEC_WT_MAX_BYTES", "CEC_WT_TAIL_BYTES", "CEC_SPLIT_SHIFT")
KIB = 1024


def run_case(env, *args):
    e = {x: v for x, v in os.environ.items() if x not in PINNED}
    e.update(env)
    r = subprocess.run(["python", os.path.join(ROOT, "tests", "store_tail_case.py"), *args], env=e,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]


def tail_env(tail, **more):
    return dict({"CEC_WT_MAX_BYTES": "0", "CEC_WT_TAIL_BYTES": str(tail)}, **more)


@pytest.mark.gpu
@pytest.mark.parametrize("tail,expect", [
    # RS(3,2) encode of 9 full line-aligned tiles, four workgroups each: 36 work items of
    # 2 outputs x 1 KiB.  10 KiB = 5 items: from item 31, the last part of tile 7
    pytest.param(10 * KIB, "tail:31", id="10KiB_inside_tile_7"),
    pytest.param(0, "nt", id="no_tail"),
    pytest.param(72 * KIB, "wt", id="72KiB_whole_launch"),
    pytest.param(1 << 30, "wt", id="1GiB_whole_launch"),
    pytest.param(70 * KIB, "tail:1", id="70KiB_all_but_one_item"),
    pytest.param(1, "tail:35", id="1B_rounds_up_to_one_item"),
])
def test_encode_tail_boundary(gpu, tail, expect):
    """(1) the exact RS(3,2) kernel: the record's wt_from and flag bits, bytes equal."""
    run_case(tail_env(tail), "encode9", expect)


@pytest.mark.gpu
@pytest.mark.parametrize("shift,expect", [
    pytest.param(0, "tail:7", id="one_workgroup_per_tile"),   # 9 items of 8 KiB: 10 KiB = 2 items
    pytest.param(1, "tail:15", id="two_workgroups_per_tile"),  # 18 items of 4 KiB: 10 KiB = 3 items
])
def test_encode_tail_follows_the_split(gpu, shift, expect):
    """(2) the same plan with one and two workgroups per tile: the boundary moves."""
    run_case(tail_env(10 * KIB, CEC_SPLIT_SHIFT=str(shift)), "encode9", expect)


@pytest.mark.gpu
@pytest.mark.parametrize("tail,expect", [
    pytest.param(1 << 20, "wt", id="tail_covers_all"),
    # one 256-lane workgroup per tile, 2 outputs: 8 KiB per item; all but the first six items
    pytest.param(6 * 8 * KIB, "tail:-6", id="tail_from_inside"),
])
def test_ragged_tiles_under_a_tail(gpu, tail, expect):
    """(3) extents of 1, 15, 17, 4095, 4096 and 4098 bytes at offsets that are no multiple of
    16: every chunk takes the byte scatter, which must not take the buffer store."""
    run_case(tail_env(tail), "ragged", expect)


@pytest.mark.gpu
def test_other_kernel_kinds_under_a_mid_launch_tail(gpu):
    """(4) a 10 KiB tail, four workgroups per tile:
    rotating decode, 6 masks over 13 tiles, exact 3 x 1: 52 items of 1 KiB, 10 items: from 42;
    diff-update + install (all-but-last read-modify-write), 3 outputs: 36 items of 3 KiB,
      4 items: from 32;
    RS(5,3) encode: 3 outputs, from 32 likewise;  RS(9,2) encode on the 16 x 2 capacity
      kernel: 2 outputs, 5 items: from 31;
    the narrow region multiply does not carry wt_from and never has a tail."""
    run_case(tail_env(10 * KIB), "decode13", "tail:42", "diff9", "tail:32", "rs53", "tail:32", "rs92", "tail:31",
             "narrow", "nt")


@pytest.mark.gpu
def test_narrow_launch_is_write_through_as_a_whole(gpu):
    """(4) the narrow region multiply under the default limit: a small launch, fully
    write-through whatever the tail, and the record says so."""
    run_case({"CEC_WT_TAIL_BYTES": str(6 * KIB)}, "narrow", "wt")


@pytest.mark.gpu
def test_lds_engine_has_no_tail(gpu):
    """(5) the LDS engine on case 1: its kernels have no write-through store path, the
    record shows neither bit, the bytes are equal."""
    run_case(tail_env(10 * KIB), "--engine", "lds", "encode9", "nt")


@pytest.mark.gpu
@pytest.mark.parametrize("policy,expect", [("nt", "nt"), ("wt", "wt")])
def test_forced_policies_keep_their_meaning(gpu, policy, expect):
    """(6) CEC_STORE_POLICY=nt: no tail at all; =wt: everything written through."""
    run_case(tail_env(10 * KIB, CEC_STORE_POLICY=policy), "encode9", expect, "decode13", expect)
