"""GPU: cec_encode_digests, cec_encode_region_digests and cec_decode_digests leave the arena
bytes of cec_encode / cec_encode_region / cec_decode and, in every kept array, the digest that
cec_digest_region of that arena yields for each unit of the plan.

Expected bytes come from the oracle and the digests from the word model, through
tests/fused_digest_case.py (pinned on the CPU in tests/test_fused_digest.py), never from the
library; a second family of tests compares the fused ops with the unfused ones on the device,
bit for bit.  Every array lies between guard bytes, and units outside a plan hold a sentinel
that must survive.  Arenas are 1, 4, 5 and 9 units (the ninth ragged: 16, 2064, 4095 bytes).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_case as dc  # noqa: E402
import fused_digest_case as fc  # noqa: E402

TILE, DB = fc.TILE, fc.DIGEST_BYTES
GUARD, FILL, SENTINEL = 64, 0xEE, 0x5A
MAX_TILES = 67108860  # one dispatch (kDigestMaxWork)


class Buf:
    """`size` device bytes between two guards of GUARD bytes, the view's base moved by `shift`
    bytes off 16-byte alignment; filled with `init` (host bytes) or the sentinel."""

    def __init__(self, torch, size, init=None, shift=0, fill=SENTINEL):
        self.raw = torch.full((2 * GUARD + size + 16,), FILL, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 16 == 0
        self.lo, self.size = GUARD + shift, size
        self.v = self.raw[self.lo:self.lo + size]
        if init is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(init)))
        else:
            self.v.fill_(fill)

    def host(self) -> np.ndarray:
        return self.v.cpu().numpy()

    def guards_intact(self) -> bool:
        r = self.raw.cpu().numpy()
        return bool((r[:self.lo] == FILL).all() and (r[self.lo + self.size:] == FILL).all())


def digest_buf(torch, units):
    return Buf(torch, units * DB, fill=0xA5)


def untouched(b: Buf, fill=SENTINEL) -> bool:
    return bool((b.host() == fill).all()) and b.guards_intact()


def check_units(got: np.ndarray, want_of_unit, units, n_all, width, fill, what):
    """`got` (n_all x width bytes, the last row possibly short) equals want_of_unit(u) on the
    plan's units and the fill everywhere else."""
    for u in range(n_all):
        row = got[u * width:(u + 1) * width]
        if u in units:
            assert np.array_equal(row, want_of_unit(u)), (what, u)
        else:
            assert (row == fill).all(), (what, u, "outside the plan")


def expect_record(ec, nt, lt, n_tiles):
    rec = ec.last_launch()
    assert (rec["kind"], rec["nt"], rec["lt"], rec["acc"], rec["engine"]) == (
        8, nt, lt, ec.CEC_ACC_NONE, ec.CEC_ENGINE_PERM), rec
    assert rec["kind"] == ec.CEC_KERNEL_COMBINE_DIGEST
    assert (rec["split_shift"], rec["flags"], rec["n_tiles"], rec["grid"], rec["lds_bytes"]) == (
        0, 0, n_tiles, (n_tiles + 3) // 4, 0), rec
    assert ec.last_engine() == ec.CEC_ENGINE_PERM


class engine_set:
    def __init__(self, ec, name):
        self.ec, self.want = ec, {"perm": ec.CEC_ENGINE_PERM, "lds": ec.CEC_ENGINE_LDS}[name]

    def __enter__(self):
        self.saved = self.ec.get_engine()
        self.ec.set_engine(self.want)

    def __exit__(self, *exc):
        self.ec.set_engine(self.saved)


def capacity(n_out: int) -> int:
    return 1 if n_out <= 1 else 2 if n_out <= 2 else 4


# ------------------------------------------------------------------ encode
class EncodeGroup:
    def __init__(self, torch, k, m, length, shift):
        self.mat, self.h_data, self.h_parity, self.h_dig = fc.encode_case(k, m, length)
        self.k, self.m, self.length, self.n = k, m, length, fc.n_units(length)
        self.data = [Buf(torch, length, a, shift) for a in self.h_data]
        self.parity = [Buf(torch, length, None, shift) for _ in range(m)]
        self.dig = [digest_buf(torch, self.n) for _ in range(k + m)]

    def views(self, bufs):
        return [b.v for b in bufs]

    def check(self, units, lost=(), unkept=()):
        """Parities and every kept digest array on `units`; sentinels elsewhere; data unchanged."""
        for j in range(self.k):
            assert np.array_equal(self.data[j].host(), self.h_data[j]) and self.data[j].guards_intact(), j
        for p in range(self.m):
            if p in lost:
                assert untouched(self.parity[p]), p
                continue
            check_units(self.parity[p].host(), lambda u: self.h_parity[p][u * TILE:(u + 1) * TILE], units, self.n,
                        TILE, SENTINEL, "parity %d" % p)
            assert self.parity[p].guards_intact(), p
        for lid in range(self.k + self.m):
            if lid in unkept or lid - self.k in lost:
                assert untouched(self.dig[lid], 0xA5), lid
                continue
            check_units(self.dig[lid].host(), lambda u: self.h_dig[lid][u], units, self.n, DB, 0xA5,
                        "digests of lid %d" % lid)
            assert self.dig[lid].guards_intact(), lid


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["perm", "lds"])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "base+1"])
@pytest.mark.parametrize("form", ["region", "plan"])
@pytest.mark.parametrize("length", fc.LENGTHS, ids=fc.LENGTH_IDS)
@pytest.mark.parametrize("k,m", [(3, 2), (4, 2), (16, 8)], ids=["rs32", "rs42", "rs168"])
def test_encode_bytes_and_digests(gpu, k, m, length, form, shift, engine):
    """Parities equal the oracle's and ec.encode's on this engine setting; every digest array
    equals the model on the plan's units; units outside the plan, guards and data are as they
    were; the launches are ceil(m / 4) of kind 8, PERM whatever the setting."""
    torch, ec = gpu
    g = EncodeGroup(torch, k, m, length, shift)
    units = list(range(g.n)) if form == "region" else fc.scattered_units(length)
    ref = [Buf(torch, length, None, shift) for _ in range(m)]
    with engine_set(ec, engine):
        seq = ec.last_launch()["seq"]
        if form == "region":
            ec.encode_region_digests(k, m, g.mat, g.views(g.data), g.views(g.parity), g.views(g.dig[:k]),
                                     g.views(g.dig[k:]), length)
            assert ec.last_launch()["seq"] == seq + (m + 3) // 4
            expect_record(ec, k, capacity(min(m, 4)), len(units))
            ec.encode_region(k, m, g.mat, g.views(g.data), g.views(ref), length)
        else:
            with ec.Plan(fc.unit_extents(units, length)) as plan:
                assert plan.num_tiles == len(units)
                ec.encode_digests(k, m, g.mat, g.views(g.data), g.views(g.parity), g.views(g.dig[:k]),
                                  g.views(g.dig[k:]), length, plan)
                assert ec.last_launch()["seq"] == seq + (m + 3) // 4
                expect_record(ec, k, capacity(min(m, 4)), len(units))
                ec.encode(k, m, g.mat, g.views(g.data), g.views(ref), plan)
                torch.cuda.synchronize()
        torch.cuda.synchronize()
    g.check(set(units))
    for p in range(m):
        assert np.array_equal(g.parity[p].host(), ref[p].host()), p


@pytest.mark.gpu
def test_encode_null_digest_entries_and_a_lost_parity(gpu):
    """A NULL digest entry, a NULL digest array and a lost parity: their arrays stay as they
    were, everything else is kept."""
    torch, ec = gpu
    k, m, length = 3, 2, fc.LENGTHS[4]
    g = EncodeGroup(torch, k, m, length, 0)
    dd = g.views(g.dig[:k])
    dd[1] = None
    ec.encode_region_digests(k, m, g.mat, g.views(g.data), [g.parity[0].v, None], dd, g.views(g.dig[k:]), length)
    torch.cuda.synchronize()
    expect_record(ec, k, 1, g.n)
    g.check(set(range(g.n)), lost=(1,), unkept=(1,))

    g = EncodeGroup(torch, k, m, length, 0)
    ec.encode_region_digests(k, m, g.mat, g.views(g.data), g.views(g.parity), None, g.views(g.dig[k:]), length)
    torch.cuda.synchronize()
    g.check(set(range(g.n)), unkept=(0, 1, 2))

    g = EncodeGroup(torch, k, m, length, 0)
    ec.encode_region_digests(k, m, g.mat, g.views(g.data), g.views(g.parity), g.views(g.dig[:k]), None, length)
    torch.cuda.synchronize()
    g.check(set(range(g.n)), unkept=(3, 4))

    # every parity lost: the launch only digests the data
    g = EncodeGroup(torch, k, m, length, 0)
    ec.encode_region_digests(k, m, g.mat, g.views(g.data), [None, None], g.views(g.dig[:k]), g.views(g.dig[k:]), length)
    torch.cuda.synchronize()
    expect_record(ec, k, 1, g.n)
    g.check(set(range(g.n)), lost=(0, 1))

    # an empty plan and a region of no bytes launch nothing
    seq = ec.last_launch()["seq"]
    ec.encode_region_digests(k, m, g.mat, g.views(g.data), g.views(g.parity), g.views(g.dig[:k]), g.views(g.dig[k:]), 0)
    with ec.Plan([]) as plan:
        ec.encode_digests(k, m, g.mat, g.views(g.data), g.views(g.parity), g.views(g.dig[:k]), g.views(g.dig[k:]),
                          length, plan)
    with ec.Plan([(0, 0, 0, 0)]) as plan:
        ec.decode_digests(k, m, g.mat, [0b01011], g.views(g.data) + g.views(g.parity), g.views(g.data),
                          g.views(g.dig[:k]), length, plan)
    assert ec.last_launch()["seq"] == seq


# ------------------------------------------------------------------ decode
DECODE_CODES = [(3, 2, 1), (3, 2, 2), (6, 3, 3), (6, 5, 5)]


class DecodeGroup:
    def __init__(self, torch, k, m, length, shift):
        self.mat, self.h_data, self.h_parity, self.h_dig = fc.encode_case(k, m, length)
        self.k, self.m, self.length, self.n = k, m, length, fc.n_units(length)
        self.h_arenas = list(self.h_data + self.h_parity)
        self.arenas = [Buf(torch, length, a, shift) for a in self.h_arenas]
        self.out = [Buf(torch, length, None, shift) for _ in range(k)]
        self.dig = [digest_buf(torch, self.n) for _ in range(k)]

    def views(self, bufs):
        return [b.v for b in bufs]

    def check(self, masks, rows):
        want = fc.decode_model(self.mat, self.k, self.m, masks, self.h_arenas, rows, self.length)
        for lid in range(self.k):
            units = want.get(lid, {})
            check_units(self.out[lid].host(), lambda u: units[u][0], units, self.n, TILE, SENTINEL, "out %d" % lid)
            check_units(self.dig[lid].host(), lambda u: units[u][1], units, self.n, DB, 0xA5, "digests %d" % lid)
            assert self.out[lid].guards_intact() and self.dig[lid].guards_intact(), lid
            for u, (b, _) in units.items():  # (the oracle's decode is the lost data itself)
                lo, hi = fc.unit_span(u, self.length)
                assert np.array_equal(b, self.h_data[lid][lo:hi])
        for lid, a in enumerate(self.arenas):
            assert np.array_equal(a.host(), self.h_arenas[lid]) and a.guards_intact(), lid


def decode_rows(length, masks, rotate):
    if not rotate:
        return [(0, 0, length, 0)]
    return fc.unit_extents(fc.scattered_units(length), length, lambda u: u % len(masks))


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "base+1"])
@pytest.mark.parametrize("rotate", [True, False], ids=["rotating", "one-mask"])
@pytest.mark.parametrize("length", fc.LENGTHS, ids=fc.LENGTH_IDS)
@pytest.mark.parametrize("k,m,n_lost", DECODE_CODES, ids=["rs32-1", "rs32-2", "rs63-3", "rs65-5"])
def test_decode_bytes_and_digests(gpu, k, m, n_lost, length, rotate, shift):
    """Rebuilt units equal the oracle's decode (the lost data) and their emitted digests the
    model, on the plan's units; everything else holds its sentinel; ceil(losses / 4) launches."""
    torch, ec = gpu
    g = DecodeGroup(torch, k, m, length, shift)
    masks = fc.rotating_masks(k, m, n_lost)
    if not rotate:
        masks = masks[1:2]
    rows = decode_rows(length, masks, rotate)
    with ec.Plan(rows) as plan:
        seq = ec.last_launch()["seq"]
        ec.decode_digests(k, m, g.mat, masks, g.views(g.arenas), g.views(g.out), g.views(g.dig), length, plan)
        assert ec.last_launch()["seq"] == seq + (n_lost + 3) // 4
        expect_record(ec, k, capacity(n_lost - 4 if n_lost > 4 else n_lost), plan.num_tiles)
        torch.cuda.synchronize()
    g.check(masks, rows)


# ------------------------------------------------------------------ fused == unfused, on the device
@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["perm", "lds"])
@pytest.mark.parametrize("k,m", [(3, 2), (16, 8)], ids=["rs32", "rs168"])
def test_encode_equals_the_unfused_ops(gpu, k, m, engine):
    """cec_encode_region_digests against cec_encode_region + cec_digest_region, bit for bit."""
    torch, ec = gpu
    length = fc.LENGTHS[5]
    g = EncodeGroup(torch, k, m, length, 0)
    ref = [Buf(torch, length, None, 0) for _ in range(m)]
    ref_dig = [digest_buf(torch, g.n) for _ in range(k + m)]
    with engine_set(ec, engine):
        ec.encode_region_digests(k, m, g.mat, g.views(g.data), g.views(g.parity), g.views(g.dig[:k]),
                                 g.views(g.dig[k:]), length)
        ec.encode_region(k, m, g.mat, g.views(g.data), g.views(ref), length)
        ec.digest_region(g.views(g.data) + g.views(ref), g.views(ref_dig), length)
        torch.cuda.synchronize()
    for p in range(m):
        assert np.array_equal(g.parity[p].host(), ref[p].host()), p
    for lid in range(k + m):
        assert np.array_equal(g.dig[lid].host(), ref_dig[lid].host()), lid


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["perm", "lds"])
@pytest.mark.parametrize("k,m,n_lost", [(3, 2, 1), (6, 5, 5)], ids=["rs32-1", "rs65-5"])
def test_decode_equals_the_unfused_ops(gpu, k, m, n_lost, engine):
    """cec_decode_digests against cec_decode + cec_digest of the rebuilt units, bit for bit
    (a plan over every unit in order: cec_digest's tile t is unit t)."""
    torch, ec = gpu
    length = fc.LENGTHS[4]
    g = DecodeGroup(torch, k, m, length, 0)
    masks = fc.rotating_masks(k, m, n_lost)
    rows = fc.unit_extents(range(g.n), length, lambda u: u % len(masks))
    ref = [Buf(torch, length, None, 0) for _ in range(k)]
    ref_dig = [digest_buf(torch, g.n) for _ in range(k)]
    with engine_set(ec, engine), ec.Plan(rows) as plan, ec.Plan(fc.unit_extents(range(g.n), length)) as every:
        ec.decode_digests(k, m, g.mat, masks, g.views(g.arenas), g.views(g.out), g.views(g.dig), length, plan)
        assert ec.last_engine() == ec.CEC_ENGINE_PERM
        ec.decode(k, m, g.mat, masks, g.views(g.arenas), g.views(ref), plan)
        ec.digest(g.views(ref), g.views(ref_dig), every)
        torch.cuda.synchronize()
    for lid in range(k):
        got, want = g.out[lid].host(), ref[lid].host()
        assert np.array_equal(got, want), lid
        rebuilt = [u for u in range(g.n) if lid in fc.lost_of(k, masks[u % len(masks)])]
        gd, wd = g.dig[lid].host().reshape(g.n, DB), ref_dig[lid].host().reshape(g.n, DB)
        for u in range(g.n):
            if u in rebuilt:
                assert np.array_equal(gd[u], wd[u]), (lid, u)
            else:
                assert (gd[u] == 0xA5).all(), (lid, u)


# ------------------------------------------------------------------ refusals
@pytest.mark.gpu
def test_refusals_launch_nothing(gpu):
    """Every CEC_EINVAL of the three ops leaves arenas, digests and the launch count as they were."""
    torch, ec = gpu
    k, m, length = 3, 2, fc.LENGTHS[4]
    g = EncodeGroup(torch, k, m, length, 0)
    d = DecodeGroup(torch, k, m, length, 0)
    data, parity, dd, pd = g.views(g.data), g.views(g.parity), g.views(g.dig[:k]), g.views(g.dig[k:])
    arenas, out, od = d.views(d.arenas), d.views(d.out), d.views(d.dig)
    masks = fc.rotating_masks(k, m, 1)
    crooked = Buf(torch, g.n * DB, None, 8, fill=0xA5)  # a digest array off 16-byte alignment
    other = torch.zeros(64, dtype=torch.uint8, device="cuda")

    def enc(rows, arena_len=length, data=data, parity=parity, dd=dd, pd=pd, mat=g.mat, kk=k):
        with ec.Plan(rows) as plan:
            ec.encode_digests(kk, m, mat, data, parity, dd, pd, arena_len, plan)

    def dec(rows, arena_len=length, masks=masks, arenas=arenas, out=out, od=od):
        with ec.Plan(rows) as plan:
            ec.decode_digests(k, m, g.mat, masks, arenas, out, od, arena_len, plan)

    whole = [(0, 0, length, 0)]
    cases = [
        # what cec_encode refuses
        (lambda: enc(whole, kk=0), "unsupported code"),
        (lambda: enc(whole, mat=[300] + g.mat[1:]), "outside GF"),
        (lambda: enc(whole, data=[data[0], None, data[2]]), "data[1] is NULL"),
        (lambda: enc([(0, 0, TILE, 1)]), "pattern 1"),
        # what cec_decode refuses
        (lambda: dec([(0, 0, TILE, 3)]), "names mask 3"),
        (lambda: dec(whole, masks=[0b00011]), "not a recovery mask"),
        (lambda: dec(whole, masks=masks[:1], arenas=[None, None] + arenas[2:]), "arena 1"),
        (lambda: dec(whole, masks=masks[:1], out=[None] + out[1:]), "out[0] is NULL"),
        # a misaligned digest array
        (lambda: enc(whole, dd=[dd[0], crooked.v, dd[2]]), "data_digests[1] is not 16-byte aligned"),
        (lambda: enc(whole, pd=[pd[0], crooked.v]), "parity_digests[1] is not 16-byte aligned"),
        (lambda: dec(whole, masks=masks[:1], od=[crooked.v] + od[1:]), "out_digests[0] is not 16-byte aligned"),
        (lambda: ec.encode_region_digests(k, m, g.mat, data, parity, [crooked.v] + dd[1:], pd, length),
         "data_digests[0] is not 16-byte aligned"),
        # out_digests missing a lost lid
        (lambda: dec(whole, masks=masks[:1], od=[None] + od[1:]), "out_digests[0] is NULL"),
        (lambda: dec(whole, masks=masks[:1], od=None), "out_digests[0] is NULL"),
        (lambda: dec([(0, 0, TILE, 0)], od=[od[0], od[1], None]), "out_digests[2] is NULL"),  # lost by a mask no extent names
        # the unit rule
        (lambda: enc([(16, 0, TILE, 0)]), "4096-byte arena boundary"),
        (lambda: enc([(0, 0, TILE, 0), (2 * TILE, 0, 100, 0)]), "partial unit"),
        (lambda: enc([(7 * TILE, 0, TILE + 2048, 0)]), "partial unit"),   # ends 16 bytes before arena_len
        (lambda: enc([(7 * TILE, 0, 2 * TILE, 0)]), "beyond arena_len"),
        (lambda: enc(whole, arena_len=length + TILE), "partial unit"),     # the ragged unit is not this arena's last
        (lambda: dec([(TILE + 16, 0, TILE - 16, 0)]), "4096-byte arena boundary"),
        (lambda: dec([(8 * TILE, 0, 2048, 0)]), "partial unit"),
        (lambda: dec([(8 * TILE, 0, 2080, 0)]), "beyond arena_len"),
        # more tiles than one dispatch holds (refused before any address is used)
        (lambda: ec.encode_region_digests(k, m, g.mat, [other] * k, [other] * m, None, None, (MAX_TILES + 1) * TILE),
         "one launch holds"),
    ]
    seq = ec.last_launch()["seq"]
    for call, word in cases:
        with pytest.raises(ec.CecError) as ei:
            call()
        assert ei.value.code == ec.CEC_EINVAL and word in str(ei.value), (word, str(ei.value))
        assert ec.last_launch()["seq"] == seq, word
    torch.cuda.synchronize()
    for b in g.parity + d.out:
        assert untouched(b)
    for b in g.dig + d.dig + [crooked]:
        assert untouched(b, 0xA5)
    for b, h in zip(g.data + d.arenas, list(g.h_data) + d.h_arenas):
        assert np.array_equal(b.host(), h) and b.guards_intact()
    # ... and the same calls, mended, run
    enc([(7 * TILE, 0, TILE + 2064, 0)])
    dec([(8 * TILE, 0, 2064, 0)])
    torch.cuda.synchronize()
    assert ec.last_launch()["seq"] == seq + 2


# ------------------------------------------------------------------ failed launches
@pytest.mark.gpu
@pytest.mark.parametrize("after", [0, 1])
def test_a_failed_launch_leaves_whole_launches(gpu, after):
    """The two-launch RS(16,8) encode with launch `after` failed on the host
    (cec_internal_fail_launch): the launches before it are complete, bytes with digests; its
    own outputs and the later ones hold their sentinels in bytes and digests."""
    torch, ec = gpu
    k, m, length = 16, 8, fc.LENGTHS[3]
    g = EncodeGroup(torch, k, m, length, 0)
    seq = ec.last_launch()["seq"]
    ec.fail_launch(after)
    try:
        with pytest.raises(ec.CecError) as ei:
            ec.encode_region_digests(k, m, g.mat, g.views(g.data), g.views(g.parity), g.views(g.dig[:k]),
                                     g.views(g.dig[k:]), length)
    finally:
        ec.fail_launch(-1)
    assert ei.value.code == ec.CEC_EHIP and "injected" in str(ei.value)
    torch.cuda.synchronize()
    assert ec.last_launch()["seq"] == seq + after  # the launches made: the injection hit launch `after`
    if after == 0:  # nothing ran: no parity, no digest -- the inputs' digests neither
        g.check(set(), lost=range(m), unkept=range(k + m))
    else:           # launch 0 ran whole: parities 0..3 and the data digests; 4..7 untouched
        expect_record(ec, k, 4, g.n)
        g.check(set(range(g.n)), lost=(4, 5, 6, 7))
    # the op again, unhindered, completes the group
    ec.encode_region_digests(k, m, g.mat, g.views(g.data), g.views(g.parity), g.views(g.dig[:k]), g.views(g.dig[k:]),
                             length)
    torch.cuda.synchronize()
    assert ec.last_launch()["seq"] == seq + after + 2
    g.check(set(range(g.n)))


# ------------------------------------------------------------------ verified recovery
@pytest.mark.gpu
@pytest.mark.parametrize("rotten", [None, 0, 3], ids=["clean", "data-survivor", "leading-parity"])
def test_verified_recovery(gpu, rotten):
    """The recipe of VERIFIED RECOVERY (cocytus_ec.h) on an RS(3,2) group of 8 units that lost
    data lid 1: the digests predicted from the survivors' live arrays against the digests the
    rebuild emits.  A clean group differs nowhere; one flipped byte of a survivor's unit 5 --
    its live digest left alone -- is found as exactly unit 5; and the emitted array is the
    digest of the rebuilt shard either way."""
    torch, ec = gpu
    k, m, n = 3, 2, 8
    length = n * TILE
    mat, h_data, _, h_dig = fc.encode_case(k, m, length)
    data = [Buf(torch, length, a) for a in h_data]
    parity = [Buf(torch, length) for _ in range(m)]
    live = [digest_buf(torch, n) for _ in range(k + m)]
    # 1. base the group
    ec.encode_region_digests(k, m, mat, [b.v for b in data], [b.v for b in parity], [b.v for b in live[:k]],
                             [b.v for b in live[k:]], length)
    torch.cuda.synchronize()
    for lid in range(k + m):
        assert np.array_equal(live[lid].host().reshape(n, DB), h_dig[lid]), lid
    # 2. lose data lid 1; the mask takes D0, D2 and the leading parity
    mask = fc.mask_of(k, m, [1], [0])
    arenas = [data[0].v, None, data[2].v, parity[0].v, None]
    if rotten is not None:
        arenas[rotten][5 * TILE + 777] ^= 0x10
    # 3. predict the rebuilt units' digests from the survivors' live arrays
    predicted, emitted, rebuilt = digest_buf(torch, n), digest_buf(torch, n), Buf(torch, length)
    live_views = [live[0].v, None, live[2].v, live[3].v, None]
    with ec.Plan([(0, 0, DB * n, 0)]) as dplan:
        ec.decode(k, m, mat, [mask], live_views, [None, predicted.v, None], dplan)
        torch.cuda.synchronize()
    assert np.array_equal(predicted.host().reshape(n, DB), h_dig[1])
    # 4. rebuild, emitting digests, and compare
    with ec.Plan([(0, 0, length, 0)]) as plan, ec.Scrub(n) as scrub:
        ec.decode_digests(k, m, mat, [mask], arenas, [None, rebuilt.v, None], [None, emitted.v, None], length, plan)
        scrub.verify_region(predicted.v, emitted.v, length)
        differing = scrub.wait()
        found = sorted(f["tile"] for f in scrub.findings())
    assert differing == (0 if rotten is None else 1)
    assert found == ([] if rotten is None else [5])
    got = rebuilt.host()
    for u in range(n):
        assert np.array_equal(got[u * TILE:(u + 1) * TILE], h_data[1][u * TILE:(u + 1) * TILE]) == (
            rotten is None or u != 5), u
    # 6. the emitted array is the digest of what was rebuilt
    fresh = digest_buf(torch, n)
    ec.digest_region([rebuilt.v], [fresh.v], length)
    torch.cuda.synchronize()
    assert np.array_equal(emitted.host(), fresh.host())
    assert np.array_equal(emitted.host().reshape(n, DB), fc.unit_digests(got))
    assert rebuilt.guards_intact() and emitted.guards_intact() and predicted.guards_intact()
