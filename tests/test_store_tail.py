"""The write-through tail's host side: CEC_WT_TAIL_BYTES and the wt_from arithmetic
(cec_internal_wt_from launches nothing; no GPU needed).

The library reads its environment once per process, so every environment is a child."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_TAIL = 96 << 20   # the tail in force when CEC_WT_TAIL_BYTES is unset
WT_MAX = 512 << 20        # auto's write-through limit
NO_TAIL = 2**64 - 1
TILE = 4096
KIB = 1024


@pytest.fixture(scope="module", autouse=True)
def built():
    from cocytus_amd import build

    build.build(verbose=False)


def in_child(env_extra, shapes):
    """[ec.wt_from(*s) for s in shapes] in a child under env_extra, and the child's stderr."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("CEC_STORE_POLICY", "CEC_WT_MAX_BYTES", "CEC_WT_TAIL_BYTES")}
    env.update(env_extra)
    code = ("import sys, json; sys.path.insert(0, %r)\nfrom cocytus_amd import ec\n"
            "print(json.dumps([ec.wt_from(*s) for s in json.loads(sys.argv[1])]))\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code, json.dumps(shapes)], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    return [tuple(x) for x in json.loads(r.stdout.strip().splitlines()[-1])], r.stderr


def tail_in_force(env_extra):
    got, err = in_child(env_extra, [(1, 0, 1, 1)])
    return got[0][2], err


def test_tail_bytes_environment():
    """CEC_WT_TAIL_BYTES is parsed as strictly as CEC_WT_MAX_BYTES: digits only (decimal,
    0x hex), in range; anything else is reported once on stderr and ignored."""
    assert tail_in_force({}) == (DEFAULT_TAIL, "")
    assert tail_in_force({"CEC_WT_TAIL_BYTES": ""}) == (DEFAULT_TAIL, "")
    assert tail_in_force({"CEC_WT_TAIL_BYTES": "0"}) == (0, "")
    assert tail_in_force({"CEC_WT_TAIL_BYTES": "4194304"}) == (4 << 20, "")
    assert tail_in_force({"CEC_WT_TAIL_BYTES": "0x1000"}) == (4096, "")
    for bad in ("-1", "lots", " 4096", "+4096", "4096 ", "4k", "99999999999999999999999"):
        got, err = tail_in_force({"CEC_WT_TAIL_BYTES": bad})
        assert got == DEFAULT_TAIL and err.count("CEC_WT_TAIL_BYTES=") == 1, (bad, got, err)
    # the two variables do not disturb each other
    got, err = in_child({"CEC_WT_MAX_BYTES": "lots", "CEC_WT_TAIL_BYTES": "8192"}, [(1, 0, 1, 1)])
    assert got[0][2] == 8192 and "CEC_WT_MAX_BYTES=lots" in err and "CEC_WT_TAIL_BYTES" not in err


def plain(n_tiles, shift, lt, streamed, tail, wt_max=WT_MAX, policy="auto"):
    """The rule in plain arithmetic."""
    if policy != "auto":
        return (policy, NO_TAIL)
    if streamed <= wt_max:
        return ("wt", NO_TAIL)
    if tail == 0:
        return ("nt", NO_TAIL)
    per_item = lt * (TILE >> shift)
    items = -(-tail // per_item)
    n_work = n_tiles << shift
    return ("wt", NO_TAIL) if items >= n_work else ("tail", n_work - items)


# (n_tiles, split_shift, lt, streamed bytes): the GPU cases' shapes, then the whole batch
SMALL = [(9, 2, 2, 9 * TILE * 5), (9, 0, 2, 9 * TILE * 5), (9, 1, 2, 9 * TILE * 5), (13, 2, 1, 13 * TILE * 4),
         (9, 2, 3, 9 * TILE * 5), (9, 2, 3, 9 * TILE * 8), (7, 0, 2, 7 * TILE * 5), (3, 2, 1, 3 * TILE * 2)]
WHOLE = [(65536, 2, 2, 65536 * TILE * 5), (65536, 2, 1, 65536 * TILE * 4), (65536, 0, 2, 65536 * TILE * 5),
         (32768, 2, 2, 32768 * TILE * 5), (0xFFFFFFFF, 2, 4, 0xFFFFFFFF * TILE * 20)]


@pytest.mark.parametrize("tail", [0, 1, 10 * KIB, 70 * KIB, 72 * KIB, 1 << 30])
def test_wt_from_small_launches(tail):
    """CEC_WT_MAX_BYTES=0: every launch is 'large'.  Case 1 of the GPU test by hand: 36 work
    items of 2 KiB, a 10 KiB tail is 5 items, from item 31."""
    got, _ = in_child({"CEC_WT_MAX_BYTES": "0", "CEC_WT_TAIL_BYTES": str(tail)}, SMALL + WHOLE)
    assert [g[:2] for g in got] == [plain(*s, tail, wt_max=0) for s in SMALL + WHOLE]
    if tail == 10 * KIB:
        assert got[0][:2] == ("tail", 31) and got[1][:2] == ("tail", 7) and got[2][:2] == ("tail", 15)
        assert got[3][:2] == ("tail", 42)


def test_wt_from_default_environment():
    """The defaults: launches of up to 512 MiB streamed stay fully write-through, larger ones
    get the default tail.  The whole batch (65,536 tiles, four workgroups each): the encode
    (2 outputs) writes 2 KiB per item, 96 MiB = 49,152 items, from 212,992; the decode (1
    output) 1 KiB per item, 98,304 items, from 163,840.  The half batch's encode streams
    640 MiB: a tail; its decode 512 MiB: write-through."""
    got, _ = in_child({}, SMALL + WHOLE + [(32768, 2, 1, 32768 * TILE * 4)])
    assert [g[:2] for g in got[:-1]] == [plain(*s, DEFAULT_TAIL) for s in SMALL + WHOLE]
    assert all(g[:2] == ("wt", NO_TAIL) for g in got[:len(SMALL)])
    n = len(SMALL)
    assert got[n][:2] == ("tail", 262144 - 49152) and got[n + 1][:2] == ("tail", 262144 - 98304)
    assert got[n + 3][:2] == ("tail", 131072 - 49152) and got[-1][:2] == ("wt", NO_TAIL)


@pytest.mark.parametrize("policy", ["nt", "wt"])
def test_forced_policies_have_no_tail(policy):
    got, _ = in_child({"CEC_STORE_POLICY": policy, "CEC_WT_TAIL_BYTES": str(10 * KIB)}, SMALL + WHOLE)
    assert [g[:2] for g in got] == [(policy, NO_TAIL)] * len(SMALL + WHOLE)


def test_wt_from_refuses_bad_shapes():
    from cocytus_amd import ec

    with pytest.raises(ec.CecError):
        ec.wt_from(9, 3, 2, 1)
    with pytest.raises(ec.CecError):
        ec.wt_from(1 << 32, 2, 2, 1)
