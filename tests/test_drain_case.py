"""CPU: the batches of tests/drain_case.py sit on the boundaries they claim, so that a pass
of tests/test_gpu_drainer_paths.py means the boundary ran; the model is an involution; the
predictor's waves are overlap-free."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drain_case as dr  # noqa: E402

ALL = [dr.case_a(False), dr.case_a(True), dr.case_b(False), dr.case_b(True), dr.case_c(), dr.case_d(),
       dr.case_e(), dr.case_f(), dr.case_g1(), dr.case_g2(), dr.case_g3(), dr.case_g5(),
       dr.case_h(40, False), dr.case_h(40, True), dr.case_h(1100, False), dr.case_h(1100, True),
       dr.case_i_empty(False), dr.case_i_empty(True), dr.case_i_leading_empty(False),
       dr.case_i_leading_empty(True)]
BY_NAME = {c.name: c for c in ALL}


def sizes(pred):
    return [len(r) for r in pred.rounds]


def test_names_are_distinct():
    assert len(BY_NAME) == len(ALL)


def test_constants():
    """The drainer's geometry for the three staging sizes used."""
    assert (dr.half_of(1 << 20), dr.tile_half_of(1 << 20)) == (1 << 20, 65536 + 1024)
    assert (dr.half_of(64 << 10), dr.tile_half_of(64 << 10)) == (64 << 10, 5120)
    assert (dr.half_of(4096), dr.tile_half_of(4096)) == (4096, 1280)
    assert dr.half_of(4097) == 4112
    assert [dr.tiles_of(a, n) for a, n in ((0, 0), (0, 1), (4095, 1), (4095, 2), (1, 4096), (0, 4096), (16, 8192))] == [
        0, 1, 1, 2, 2, 1, 3]


def test_a_byte_boundary():
    a, a16 = BY_NAME["A"], BY_NAME["A+16"]
    assert dr.packed_bytes(a) == 1 << 20 == dr.SMALL_BYTES and dr.total_tiles(a) == 256
    assert dr.packed_bytes(a16) == (1 << 20) + 16 and dr.total_tiles(a16) == 257
    assert len({u.addr for u in a.updates}) == 256 and all(u.addr % dr.TILE == 0 for u in a.updates)
    assert dr.predict_case(a) == dr.Prediction("small", [list(range(256))], 1)
    p = dr.predict_case(a16)
    assert (p.path, sizes(p), p.launches) == ("pack", [256, 1], 2)


def test_b_tile_boundary():
    b, b1 = BY_NAME["B"], BY_NAME["B+1"]
    assert dr.total_tiles(b) == 8192 == dr.SMALL_TILES and dr.packed_bytes(b) == 64 << 10
    assert dr.total_tiles(b1) == 8193 and dr.packed_bytes(b1) == (64 << 10) + 16 <= dr.SMALL_BYTES
    assert all(dr.tiles_of(u.addr, u.length) == 2 for u in b.updates)
    p = dr.predict_case(b)
    assert (p.path, sizes(p), p.launches) == ("small", [4096], 1)
    p = dr.predict_case(b1)
    assert (p.path, sizes(p), p.launches) == ("pack", [2560, 1537], 2)


def test_c_cut_by_tiles():
    c = BY_NAME["C"]
    assert dr.tile_half_of(c.staging_bytes) == 5120
    assert dr.packed_bytes(c) == 5200 * 16 <= 2 * dr.half_of(c.staging_bytes)  # bytes alone: two rounds
    assert dr.packed_bytes(c) > dr.half_of(c.staging_bytes)
    p = dr.predict_case(c)
    assert (p.path, sizes(p), p.launches) == ("pack", [2560, 2560, 80], 3)


def test_d_in_place_rounds():
    d = BY_NAME["D"]
    area = 2 * dr.half_of(d.staging_bytes)
    assert area == 8192 and 2 * dr.tile_half_of(d.staging_bytes) == 2560
    assert [u.stage for u in d.updates] == list(range(8192)) and all(u.length == 1 for u in d.updates)
    assert d.updates[-1].stage + d.updates[-1].length == area
    assert sum(1 for u in d.updates if u.stage % 16) == 8192 - 512
    assert set(dr.waves_of(d.updates)) == {0}
    p = dr.predict_case(d)
    assert (p.path, sizes(p), p.launches) == ("in_place", [2560, 2560, 2560, 512], 4)


def test_e_wave_cut_by_rounds():
    e = BY_NAME["E"]
    wave = dr.waves_of(e.updates)
    assert wave[:8092] == [0] * 8092 and wave[8092:] == [1] * 100
    assert [u.addr for u in e.updates[8092:]] == [u.addr for u in e.updates[:100]]
    p = dr.predict_case(e)
    assert (p.path, sizes(p), p.launches) == ("in_place", [2560, 2560, 2560, 512], 5)
    assert p.rounds[3] == list(range(7680, 8192))  # 412 of wave 0, then wave 1: two launches


def test_f_second_half_only():
    f = BY_NAME["F"]
    half = dr.half_of(f.staging_bytes)
    assert all(half <= u.stage and u.stage + u.length <= 2 * half for u in f.updates)
    assert f.updates[-1].stage + f.updates[-1].length == 2 * half
    assert [u.stage % 16 for u in f.updates] == [0, 5, 15]
    assert dr.predict_case(f) == dr.Prediction("in_place", [[0, 1, 2]], 1)
    assert dr.predict_case(f, digests=True).launches == 2


def test_g_mixed():
    g1, g2, g3, g5 = (BY_NAME[n] for n in ("G1", "G2", "G3", "G5"))
    assert [i for i, u in enumerate(g1.updates) if u.stage is None] == [0] and len(g1.updates) == 301
    assert [i for i, u in enumerate(g2.updates) if u.stage is None] == [0, 150, 299] and len(g2.updates) == 301
    for g in (g1, g2, g3):
        staged = [u.stage for u in g.updates if u.stage is not None]
        assert staged == [dr.TILE * i for i in range(len(staged))]  # consecutive, 16-byte aligned, from 0
    for g in (g1, g2, g5):
        assert dr.packed_bytes(g) > dr.SMALL_BYTES
        assert dr.predict_case(g) == dr.Prediction("mixed", None, None)
    assert sorted(set(dr.waves_of(g1.updates))) == [0]
    wave = dr.waves_of(g2.updates)
    assert sorted(set(wave)) == [0, 1] and [i for i, w in enumerate(wave) if w] == list(range(200, 240))
    assert g2.updates[200].addr == g2.updates[0].addr  # staged onto the pageable first update
    assert len(g3.updates) == 21
    p = dr.predict_case(g3)
    assert (p.path, sizes(p), p.launches) == ("small", [21], 1)
    assert g5.updates[0].length > dr.SMALL_BYTES and g5.updates[0].length <= dr.half_of(g5.staging_bytes)
    rest = [u for u in g5.updates if u.stage is None]
    assert sum(dr.pad16(u.length) for u in rest) > 2 * dr.SMALL_BYTES  # at least three windows
    assert sorted(set(dr.waves_of(rest))) == [0, 1]


@pytest.mark.parametrize("n", [40, 1100])
def test_h_window(n):
    for staged in (False, True):
        h = BY_NAME[f"H{n}{'s' if staged else 'p'}"]
        lo, hi = dr.H_MID - dr.H_WINDOW, dr.H_MID + dr.H_WINDOW
        assert len(h.updates) == n and h.arena == (1 << 32) + (1 << 20) and h.origin == lo - dr.H_GUARD
        assert all(lo <= u.addr and u.addr + u.length <= hi and u.length for u in h.updates)
        spans = [(u.addr, u.length) for u in h.updates]
        assert (dr.H_MID - 1, 2) in spans and any(a == dr.H_MID for a, _ in spans)
        assert any(a < dr.H_MID - 1 and a + ln > dr.H_MID + 1 for a, ln in spans)  # straddles 2^32
        assert sum(1 for a, _ in spans if a >= dr.H_MID) >= n // 3 and sum(1 for a, _ in spans if a % 16) >= n // 4
        assert sorted(set(dr.waves_of(h.updates))) == [0, 1, 2]
        p = dr.predict_case(h)
        assert (p.path, len(p.rounds), p.launches) == ("in_place" if staged else "small", 1, 3)


def test_i_empty():
    for name in ("I0", "I0s"):
        p = dr.predict_case(BY_NAME[name])
        assert (p.path, sizes(p), p.launches) == ("in_place", [5], 0)  # (no non-empty update is outside)
    assert dr.predict(BY_NAME["I0"].updates[:0], 1 << 20, []) == dr.Prediction("none", [], 0)
    a, b = BY_NAME["I1"], BY_NAME["I1e"]
    assert b.updates[1:] == a.updates and b.updates[0].length == 0
    assert dr.predict_case(a).launches == dr.predict_case(b).launches == 2


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_case_is_well_formed(case):
    """Every update inside the arena (case H: inside what is compared), at most half the
    staging area long; staged diffs inside the area and disjoint; no wave holds an overlap."""
    half = dr.half_of(case.staging_bytes)
    for u in case.updates:
        assert 0 <= u.src_lid < dr.K and u.length <= half
        assert case.origin <= u.addr and u.addr + u.length <= case.arena
        if u.stage is not None:
            assert 0 <= u.stage and u.stage + u.length <= 2 * half
    staged = sorted((u.stage, u.length) for u in case.updates if u.stage is not None and u.length)
    assert all(a + n <= b for (a, n), (b, _) in zip(staged, staged[1:]))
    wave = dr.waves_of(case.updates)
    for w in set(wave):
        spans = sorted((u.addr, u.length) for u, x in zip(case.updates, wave) if x == w and u.length)
        assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])), w
    order = dr.apply_order(wave)
    assert sorted(order) == list(range(len(wave)))
    assert all((wave[a], a) < (wave[b], b) for a, b in zip(order, order[1:]))
    p = dr.predict_case(case)
    if p.rounds is not None:
        assert [i for r in p.rounds for i in r] == order


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_model_twice_is_identity(case):
    """x ^= c * d twice is x: the model applied twice returns the initial arena, and once it
    changes exactly the bytes some update with a non-zero diff covers."""
    size = case.arena - case.origin if not case.origin else 2 * (dr.H_WINDOW + dr.H_GUARD)
    rng = np.random.default_rng(len(case.name))
    arena0 = rng.integers(0, 256, size, dtype=np.uint8)
    bufs = dr.diff_bytes(case)
    assert [len(b) for b in bufs] == [u.length for u in case.updates]
    for row in dr.RS32_ROWS.values():
        once = dr.model(arena0, case.updates, bufs, row, case.origin)
        covered = np.zeros(size, bool)
        for u in case.updates:
            covered[u.addr - case.origin:u.addr - case.origin + u.length] = True
        assert not (once != arena0)[~covered].any()
        assert (once != arena0).any() == any(u.length for u in case.updates)
        assert np.array_equal(dr.model(once, case.updates, bufs, row, case.origin), arena0)
