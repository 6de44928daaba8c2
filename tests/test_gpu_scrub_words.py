"""GPU: every compiled scrub and digest-check kernel reports the word model's words.

tests/test_gpu_scrub.py checks single flips, where the report word is obvious, on six codes
that reach five of the twelve scrub kernels and four of the nine digest-check kernels.  Here
every kernel runs (the census at the end says so), and what it reports is compared bit for
bit -- syndromes, ruled_out and the lid that follows from them -- with the numpy model of
the word (scrub_case.kernel_word, pinned on the CPU in tests/test_scrub.py) evaluated on a
host copy of each tile's corrupted bytes: one or several lids, one byte or hundreds, data
and parity together, in one launch group or across two.  The digest check gets the same
function applied to the model digests of tests/digest_case.py; the digest is linear, so that
is exact for any corruption.

One arena group per code carries all scenarios at once (scrub_case.scenarios), each on a
tile of its own with clean tiles between them, and one run per plan checks them all: plan M
(ragged tiles, then full ones: one workgroup per tile) and plan F (full tiles: four
workgroups per tile).  The field arithmetic of the expected words is the bit-serial table
of tests/digest_case.py; the matrix is the oracle's.  Every test leaves the groups clean.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_case as dc  # noqa: E402
import scrub_case as sc  # noqa: E402

CODES = sc.WORD_CODES + sc.EXACT_CODES
REPAIR_CODES = [(4, 5), (8, 5), (13, 6), (16, 8), (2, 2)]
MUL = dc.MUL
DIV = sc.table_div(MUL)
M_TILES = sc.tiles_of(sc.WORD_M)
F_TILES = sc.tiles_of(sc.WORD_F)
PLANS = (("M", sc.WORD_M, M_TILES, 0), ("F", sc.WORD_F, F_TILES, 2))

_groups = {}
_seen = set()  # (kind, nt, lt, exact) of every scrub and digest-check launch record seen
_ran = set()   # (kind, k, m): the runs that put them there


def group(gpu, oracle, k, m):
    torch, ec = gpu
    if (k, m) not in _groups:
        _groups[k, m] = sc.Group(torch, ec, oracle, k, m, size=sc.WORD_SIZE)
    return _groups[k, m]


def plan_of(ec, extents):
    return ec.Plan([(o, 0, n, 0) for o, n in extents])


def host_of(g):
    return [a.cpu().numpy() for a in g.arenas]


def xor_hits(g, hits, host=None):
    """XOR (lid, position, value) into the device arenas, one indexed update per lid, and
    into the host copies."""
    torch = g.torch
    for lid in sorted({h[0] for h in hits}):
        pos = np.array([p for l, p, _ in hits if l == lid], dtype=np.int64)
        val = np.array([v for l, _, v in hits if l == lid], dtype=np.uint8)
        assert len(set(pos.tolist())) == len(pos)
        idx = torch.from_numpy(pos).cuda()
        g.arenas[lid][idx] = g.arenas[lid][idx] ^ torch.from_numpy(val).cuda()
        if host is not None:
            host[lid][pos] ^= val
    torch.cuda.synchronize()


def device_equals(g, host) -> bool:
    return all(np.array_equal(a.cpu().numpy(), h) for a, h in zip(g.arenas, host))


def check_record(ec, g, seq, kind, tiles, shift):
    """One launch per four parities; the last one ran the kernel the table names."""
    k, m = g.k, g.m
    rec = ec.last_launch()
    assert rec["seq"] - seq == (m + 3) // 4, (rec, seq)
    want = (k, m) if kind == sc.KIND_SCRUB and (k, m) in sc.EXACT_CODES else sc.last_capacity(k, m)
    assert (rec["kind"], rec["nt"], rec["lt"]) == (kind, *want), rec
    if (k, m) in sc.WORD_CODES:
        assert want == sc.WORD_LAST[sc.WORD_CODES.index((k, m))]
    assert (rec["acc"], rec["engine"], rec["flags"], rec["n_tiles"]) == (
        ec.CEC_ACC_ALL, ec.CEC_ENGINE_PERM, 0, len(tiles)), rec
    if kind == sc.KIND_SCRUB:
        assert (rec["split_shift"], rec["grid"]) == (shift, len(tiles) << shift), rec
    else:
        assert (rec["split_shift"], rec["grid"]) == (0, 1), rec
    _seen.add(sc.scrub_inst(rec, k, m))
    _ran.add((kind, k, m))


def run_scrub(ec, g, report, plan, tiles, shift):
    seq = ec.last_launch()["seq"]
    n = g.scrub(report, plan)
    check_record(ec, g, seq, sc.KIND_SCRUB, tiles, shift)
    return n, report.findings()


def run_digests(gpu, g, report, plan, tiles):
    """ec.digest of all k + m arenas in one launch, then the check over them."""
    torch, ec = gpu
    bufs = dc.DigestBuffers(torch, g.k + g.m, len(tiles))
    ec.digest(g.arenas, bufs.views, plan)
    seq = ec.last_launch()["seq"]
    report.run_digests(g.k, g.m, g.mat, bufs.views[:g.k], bufs.views[g.k:], plan)
    n = report.wait()
    check_record(ec, g, seq, sc.KIND_DIGEST_CHECK, tiles, 0)
    return n, report.findings(), bufs


def same(found, want, what):
    """wait()'s count aside, the findings equal the model's, field for field."""
    assert [f["tile"] for f in found] == [f["tile"] for f in want], (what, found, want)
    for f, w in zip(found, want):
        assert f == w, (what, {x: hex(v) if x in ("syndromes", "ruled_out") else v for x, v in f.items()}, w)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", CODES)
def test_words_equal_the_model(gpu, oracle, k, m):
    """All scenarios at once, plan M then plan F: wait() is the number of tiles the model
    flags, findings() lists exactly those, ascending, with the model's syndromes, ruled_out
    and classification; the scenarios' own verdicts hold (a single corrupt lid is that lid,
    scenario 6 is the data lid at m = 5 and UNLOCATED at m >= 6, the (7,2) alias is lid 2);
    the clean tiles in between and the bytes outside the ragged tiles flag nothing.  The
    digests of all k + m arenas in one launch are the model's, the digest check reports the
    model's words over them, and where a tile's corruption lies within two 16-byte chunks
    exactly what cec_scrub reported."""
    torch, ec = gpu
    g = group(gpu, oracle, k, m)
    before = g.slab.clone()
    host = host_of(g)
    scen, outside = sc.scenarios(k, m)
    hits = outside + [h for s in scen for h in s.hits]
    by_tile = {(s.off, s.len): s for s in scen}
    xor_hits(g, hits, host)
    try:
        assert device_equals(g, host)
        with ec.Scrub(len(M_TILES)) as report:
            for name, extents, tiles, shift in PLANS:
                want = sc.expected_findings(sc.model_words(MUL, DIV, g.mat, k, m, host, tiles), tiles, k, m, g.mat)
                by_t = {f["tile"]: f for f in want}
                for t, tile in enumerate(tiles):  # what the scenarios demand of the model
                    s = by_tile.get(tile)
                    if name == "M" or tile[0] >= sc.FULL0:
                        assert (t in by_t) == (s is not None), (name, t)
                    if s is not None and s.lid is not None:
                        assert by_t[t]["lid"] == s.lid, (name, s.name, by_t[t])
                with plan_of(ec, extents) as plan:
                    n, found = run_scrub(ec, g, report, plan, tiles, shift)
                    same(found, want, (name, "scrub"))
                    assert n == len(want)
                    n, dfound, bufs = run_digests(gpu, g, report, plan, tiles)
                    dig = [dc.digests_of(h, tiles) for h in host]
                    for i in range(k + m):
                        assert np.array_equal(bufs.host(i), dig[i]), (name, "digest of lid", i)
                    assert bufs.guards_intact()
                    units = [(dc.DIGEST_BYTES * t, dc.DIGEST_BYTES) for t in range(len(tiles))]
                    dwant = sc.expected_findings(sc.model_words(MUL, DIV, g.mat, k, m, dig, units), tiles, k, m,
                                                 g.mat)
                    same(dfound, dwant, (name, "digest check"))
                    assert n == len(dwant)
                    by_d = {f["tile"]: f for f in dfound}
                    for f in found:  # the header's GUARANTEE
                        s = by_tile.get((f["off"], f["len"]))
                        if s is not None and s.two_chunks:
                            assert by_d.get(f["tile"]) == f, (name, s.name, f, by_d.get(f["tile"]))
    finally:
        xor_hits(g, hits)
    assert torch.equal(g.slab, before)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", REPAIR_CODES)
def test_repair_generic_codes(gpu, oracle, k, m):
    """cec_scrub_repair on the same corruption (less the alias): it returns the model's
    count of UNLOCATED tiles, every located tile holds its original bytes again (the decode
    of a capacity shape; the encode of one parity out of m, at p >= 4 the multi-launch
    encode with holes) and no other byte of the slab changed.  A second scrub flags the
    unlocated tiles and, at m = 5, scenario 6's tile, now as parity k + 4 (the data lid was
    rebuilt in the first round); a second repair clears that.  With the unlocated tiles'
    bytes flipped back the slab equals its clone and the scrub returns 0."""
    torch, ec = gpu
    g = group(gpu, oracle, k, m)
    before = g.slab.clone()
    clean = host_of(g)
    host = [h.copy() for h in clean]
    scen, outside = sc.scenarios(k, m, alias=False)
    hits = outside + [h for s in scen for h in s.hits]
    six = [M_TILES.index((s.off, s.len)) for s in scen if s.name.startswith("6") and m == 5]
    assert len(six) == (m == 5)

    def slab_as(state):
        exp = before.clone()
        for a, h in zip(g.arenas, state):
            o = a.storage_offset() - g.slab.storage_offset()
            exp[o:o + len(h)] = torch.from_numpy(h).cuda()
        return exp

    def model():
        return sc.expected_findings(sc.model_words(MUL, DIV, g.mat, k, m, host, M_TILES), M_TILES, k, m, g.mat)

    def repair_round(report, plan, what):
        want = model()
        n, found = run_scrub(ec, g, report, plan, M_TILES, 0)
        same(found, want, what)
        assert n == len(want)
        unlocated = [f["tile"] for f in want if f["lid"] == sc.UNLOCATED]
        assert report.repair(k, m, g.mat, g.data, g.parity) == len(unlocated), what
        torch.cuda.synchronize()
        for f in want:
            if f["lid"] != sc.UNLOCATED:
                host[f["lid"]][f["off"]:f["off"] + f["len"]] = clean[f["lid"]][f["off"]:f["off"] + f["len"]]
        assert torch.equal(g.slab, slab_as(host)), what
        return want, unlocated

    xor_hits(g, hits, host)
    try:
        assert torch.equal(g.slab, slab_as(host))
        with ec.Scrub(len(M_TILES)) as report, plan_of(ec, sc.WORD_M) as plan:
            first, unlocated = repair_round(report, plan, "first round")
            assert len(first) == len(scen) and 0 < len(unlocated) < len(first)
            assert any(k <= f["lid"] for f in first) and any(0 <= f["lid"] < k for f in first)
            if m > 4:
                assert any(f["lid"] >= k + 4 for f in first)  # a parity the encode's second launch writes
            second, again = repair_round(report, plan, "second round")
            assert [f["tile"] for f in second] == sorted(unlocated + six)
            assert again == unlocated
            assert all(f["lid"] == k + 4 for f in second if f["tile"] in six)
            n, found = run_scrub(ec, g, report, plan, M_TILES, 0)
            assert n == len(unlocated) and [f["tile"] for f in found] == unlocated
            assert all(f["lid"] == sc.UNLOCATED for f in found)
            left = [h for h in hits if host[h[0]][h[1]] != clean[h[0]][h[1]]]
            inside = [h for h in left if h not in outside]
            assert all(any(M_TILES[t][0] <= pos < sum(M_TILES[t]) for t in unlocated) for _, pos, _ in inside)
            assert len(left) == len(inside) + len(outside)
            xor_hits(g, left, host)
            assert torch.equal(g.slab, before)
            assert run_scrub(ec, g, report, plan, M_TILES, 0) == (0, [])
            assert report.repair(k, m, g.mat, g.data, g.parity) == 0
    finally:
        for a, h in zip(g.arenas, clean):
            a.copy_(torch.from_numpy(h))
        torch.cuda.synchronize()
    assert torch.equal(g.slab, before)


@pytest.mark.gpu
def test_census_of_scrub_instantiations(gpu, oracle):
    """The launch records seen in this file (a clean run of any code not yet run), with
    scrub_case.UNREACHABLE_SCRUB, are exactly the 12 + 9 compiled scrub and digest-check
    kernels: a change to launch_scrub or launch_digest_check shows up here."""
    torch, ec = gpu
    with ec.Scrub(len(M_TILES)) as report, plan_of(ec, sc.WORD_M) as plan:
        for k, m in CODES:
            g = group(gpu, oracle, k, m)
            if (sc.KIND_SCRUB, k, m) not in _ran:
                assert run_scrub(ec, g, report, plan, M_TILES, 0) == (0, [])
            if (sc.KIND_DIGEST_CHECK, k, m) not in _ran:
                assert run_digests(gpu, g, report, plan, M_TILES)[:2] == (0, [])
    reached, unreachable, compiled = set(_seen), set(sc.UNREACHABLE_SCRUB), sc.all_instantiations()
    assert not reached & unreachable, sorted(reached & unreachable)
    assert reached | unreachable == compiled, (sorted(compiled - reached - unreachable), sorted(reached - compiled))
    assert (len(reached), len(unreachable)) == (21, 0)
