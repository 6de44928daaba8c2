"""CPU: the digest-emitting encode and decode -- their declarations and bindings, their launch
planning and unit rule under ASan + UBSan, and the model the GPU file
(tests/test_gpu_fused_digest.py) takes its expected bytes from.

The model (tests/fused_digest_case.py) is the oracle's encode / decode followed by the word
model's digest per unit.  The verified recovery rests on one property of it, pinned here on
the oracle alone: digest(decode(arenas)) == decode(digests(arenas)), unit by unit, for
rotating masks -- the digest is GF(2^8)-linear and so is the decode.  No GPU.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_case as dc  # noqa: E402
import fused_digest_case as fc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("cec_encode_digests", "cec_encode_region_digests", "cec_decode_digests")


def test_header_declares_and_library_resolves_the_new_functions():
    from cocytus_amd import build, ec

    build.build(verbose=False)
    text = open(os.path.join(ROOT, "include", "cocytus_ec.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ec.lib()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in ec._SIGS and getattr(L, name).restype is ec._i, name
    assert callable(ec.encode_digests) and callable(ec.encode_region_digests) and callable(ec.decode_digests)
    assert re.search(r"CEC_KERNEL_COMBINE_DIGEST\s*=\s*8\b", src)
    assert ec.CEC_KERNEL_COMBINE_DIGEST == 8
    # LIVE DIGESTS names the bulk ops, lists only what still needs a re-base, and the recipe is there
    live = text[text.index("LIVE DIGESTS: a process may keep"):text.index("VERIFIED RECOVERY:")]
    for name in NEW_FUNCTIONS:
        assert name in live, name
    for still in ("cec_scrub_repair", "cec_solve", "recovery pool"):
        assert still in live, still
    recipe = text[text.index("VERIFIED RECOVERY:"):text.index("#define CEC_DIGEST_BYTES")]
    for step in ("cec_decode over them", "cec_decode_digests", "cec_digest_verify_region", "LIMIT"):
        assert step in recipe, step


class _NoPlan:
    handle = None


def test_refusals_that_need_no_device():
    """A bad code and a NULL array are answered before the library looks for a device."""
    from cocytus_amd import build, ec

    build.build(verbose=False)
    mat = fc.matrix(3, 2)
    one, three = [0x1000], [0x1000, 0x2000, 0x3000]
    for call in (
        lambda: ec.encode_region_digests(0, 2, mat, three, one, None, None, 4096),
        lambda: ec.encode_region_digests(3, 9, mat, three, one, None, None, 4096),
        lambda: ec.decode_digests(17, 2, mat, [0xB], three, three, three, 4096, _NoPlan()),
    ):
        with pytest.raises(ec.CecError) as ei:
            call()
        assert ei.value.code == ec.CEC_EINVAL and "unsupported code" in str(ei.value)
    for call, word in (
        (lambda: ec.encode_region_digests(3, 2, mat, None, [1, 2], None, None, 4096), "NULL"),
        (lambda: ec.encode_region_digests(3, 2, mat, three, None, None, None, 4096), "NULL"),
        (lambda: ec.encode_digests(3, 2, mat, three, [1, 2], None, None, 4096, _NoPlan()), "plan is NULL"),
        (lambda: ec.decode_digests(3, 2, mat, [0xB], three + [1, 2], three, three, 4096, _NoPlan()), "bad args"),
    ):
        with pytest.raises(ec.CecError) as ei:
            call()
        assert ei.value.code == ec.CEC_EINVAL and word in str(ei.value)


def test_plan_and_unit_rule_under_sanitizers(tmp_path):
    """plan_combine_digest and the unit rule (cec_launchplan.hpp), included from the shipped
    header by tests/drain_c/fused_digest_plan_main.cpp and run under ASan + UBSan: grid, block
    and every field of the launch record, the limit of one dispatch held and one above it
    refused, the output capacities; extents at a 4 KiB offset against one at 16, a short last
    tile that ends at arena_len against one 16 bytes before it, an extent beyond arena_len,
    and regions of 0, 1, 4095, 4096 and 4097 bytes."""
    exe = tmp_path / "fused_digest_plan_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "cocytus_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    "-pthread", "-o", str(exe), os.path.join(ROOT, "tests", "drain_c", "fused_digest_plan_main.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr[-2000:]


def test_the_case_generator():
    assert [fc.n_units(n) for n in fc.LENGTHS] == [1, 4, 5, 9, 9, 9]
    assert fc.scattered_units(fc.TILE) == [0]
    assert fc.scattered_units(4 * fc.TILE) == [0, 3]
    assert fc.scattered_units(fc.LENGTHS[4]) == [0, 2, 3, 4, 5, 6, 8]
    rows = fc.unit_extents(fc.scattered_units(fc.LENGTHS[4]), fc.LENGTHS[4])
    assert rows[0] == (0, 0, 4096, 0) and rows[-1] == (8 * 4096, 0, 2064, 0)
    for k, m, n_lost in ((3, 2, 1), (3, 2, 2), (6, 3, 3), (6, 5, 5)):
        masks = fc.rotating_masks(k, m, n_lost)
        assert len(masks) == k and len(set(masks)) > 1
        lost = set()
        for mask in masks:
            assert bin(mask).count("1") == k and mask >> (k + m) == 0
            assert len(fc.lost_of(k, mask)) == n_lost
            lost |= set(fc.lost_of(k, mask))
        assert lost == set(range(k))  # rotating: every data lid is rebuilt somewhere


@pytest.mark.parametrize("k,m", [(3, 2), (4, 2), (16, 8)])
def test_the_encode_model_is_pinned(oracle, k, m):
    """The parity digests of the model are the encode of the data digests (linearity), for a
    ragged arena: what cec_encode_region over the digest arrays yields, and what the fused
    encode must emit."""
    length = fc.LENGTHS[4]
    mat, data, parity, dig = fc.encode_case(k, m, length)
    assert all(d.shape == (9, 32) for d in dig)
    by_linearity = oracle.encode(mat, k, m, [np.ascontiguousarray(d.reshape(-1)) for d in dig[:k]])
    for p in range(m):
        assert np.array_equal(by_linearity[p], dig[k + p].reshape(-1)), p
    # the ragged unit is digested zero-padded
    lo, hi = fc.unit_span(8, length)
    assert hi - lo == 2064 and np.array_equal(dig[0][8], dc.digest(data[0][lo:hi]))


@pytest.mark.parametrize("k,m,n_lost", [(3, 2, 1), (3, 2, 2), (6, 3, 3), (6, 5, 5)])
def test_digest_of_decode_is_decode_of_digests(oracle, k, m, n_lost):
    """digest(decode(arenas)) == decode(digests(arenas)) on the oracle, unit by unit with the
    masks rotating, the ragged last unit included: the prediction of VERIFIED RECOVERY.  And a
    survivor byte that changes moves the rebuilt unit's digest off the prediction, which is made
    from the survivors' live digests and stays."""
    length = fc.LENGTHS[4]
    mat, data, parity, dig = fc.encode_case(k, m, length)
    arenas = list(data + parity)
    masks = fc.rotating_masks(k, m, n_lost)
    for u in range(fc.n_units(length)):
        mask = masks[u % len(masks)]
        lo, hi = fc.unit_span(u, length)
        rebuilt = fc.decode_unit(mat, k, m, mask, arenas, lo, hi)
        predicted = fc.decode_unit(mat, k, m, mask, [d[u] for d in dig], 0, 32)
        assert sorted(rebuilt) == fc.lost_of(k, mask)
        for lid, b in rebuilt.items():
            assert np.array_equal(b, data[lid][lo:hi]), (u, lid)          # the decode is a decode
            assert np.array_equal(dc.digest(b), predicted[lid]), (u, lid)  # and commutes with the digest
    # one flipped survivor byte: the rebuilt unit's digest leaves the prediction
    u, mask = 5, masks[5 % len(masks)]
    lo, hi = fc.unit_span(u, length)
    surv = next(lid for lid in range(k + m) if (mask >> lid) & 1)
    rotten = [a.copy() for a in arenas]
    rotten[surv][lo + 1234] ^= 0x40
    rebuilt = fc.decode_unit(mat, k, m, mask, rotten, lo, hi)
    predicted = fc.decode_unit(mat, k, m, mask, [d[u] for d in dig], 0, 32)
    for lid, b in rebuilt.items():
        assert not np.array_equal(dc.digest(b), predicted[lid]), lid


def test_the_decode_model_covers_its_rows(oracle):
    k, m, length = 3, 2, fc.LENGTHS[3]
    mat, data, parity, dig = fc.encode_case(k, m, length)
    masks = fc.rotating_masks(k, m, 1)
    rows = fc.unit_extents(fc.scattered_units(length), length, lambda u: u % len(masks))
    got = fc.decode_model(mat, k, m, masks, list(data + parity), rows, length)
    seen = sorted((u, lid) for lid in got for u in got[lid])
    assert seen == sorted((u, fc.lost_of(k, masks[u % len(masks)])[0]) for u in fc.scattered_units(length))
    for lid in got:
        for u, (b, d) in got[lid].items():
            lo, hi = fc.unit_span(u, length)
            assert np.array_equal(b, data[lid][lo:hi]) and np.array_equal(d, dig[lid][u])
