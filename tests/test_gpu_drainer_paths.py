"""GPU: every path of cec_drainer_apply at its boundaries, against the sequential loop.

The combine kernels under the drainer are tested by test_gpu_kernel_matrix.py and its wave
colouring by tests/drain_c/waves_main.cpp; this file tests what lies between: which path a
batch takes (in place, small window, pack, and the two-part apply of a batch that mixes diffs
inside the staging area with diffs elsewhere), where the path cuts its rounds, and what it
does to the staging area.  The batches, the model (the loop parity[addr:addr+len] ^=
MUL[MATRIX(lid_self, src_lid)][buf] over the bit-serial table) and the predicted path, rounds
and launches are those of tests/drain_case.py, pinned on the CPU by tests/test_drain_case.py.

Every comparison is bit-exact and over the whole arena, which starts as random bytes (case H:
over the initialised window and its guards).  cec_drainer_last_launches and the thread's
launch counter are compared with the prediction; for the mixed batches only launches >= 1 is
promised.  The small path is told from the other two by its completion: cec_last_sync moves
by one there and not at all on the others.  The staging area is filled with a sentinel before
the diffs are placed and compared whole after every apply that does not pack into it: the
library writes it on the pack path alone, which no batch with a source inside it takes.

Code: RS(3,2), lid_self = both parities.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_case as dc  # noqa: E402
import drain_case as dr  # noqa: E402
import kernel_matrix_case as kc  # noqa: E402

pytestmark = pytest.mark.gpu

K, M, TILE = dr.K, dr.M, dr.TILE
STAGE_FILL = 0x5A
LIDS = [pytest.param(3, id="p0"), pytest.param(4, id="p1")]


@pytest.fixture(params=[pytest.param(kc.PERM, id="perm"), pytest.param(kc.LDS, id="lds")])
def engine(request, gpu):
    torch, ec = gpu
    default = ec.get_engine()
    ec.set_engine(request.param)
    yield request.param
    ec.set_engine(default)


# ------------------------------------------------------------------ references, computed once
def compared_bytes(case) -> int:
    return 2 * (dr.H_WINDOW + dr.H_GUARD) if case.origin else case.arena


def by_name(fn):
    """fn(case, *rest) computed once per (case.name, *rest)."""
    memo = {}

    @functools.wraps(fn)
    def cached(case, *rest):
        key = (case.name,) + rest
        if key not in memo:
            memo[key] = fn(case, *rest)
        return memo[key]

    return cached


@by_name
def inputs(case):
    """(initial bytes of what is compared, the diffs), read-only."""
    rng = np.random.default_rng([0xD7A1] + [ord(c) for c in case.seed or case.name])
    arena0 = rng.integers(0, 256, compared_bytes(case), dtype=np.uint8)
    if case.origin:  # case H: a guard on each side of the window
        arena0[:dr.H_GUARD] = arena0[-dr.H_GUARD:] = 0xA5
    arena0.setflags(write=False)
    bufs = dr.diff_bytes(case)
    for b in bufs:
        b.setflags(write=False)
    return arena0, bufs


@by_name
def expected(case, lid_self):
    arena0, bufs = inputs(case)
    want = dr.model(arena0, case.updates, bufs, dr.RS32_ROWS[lid_self], case.origin)
    want.setflags(write=False)
    return want


def mismatch(got, want, origin=0) -> str:
    bad = np.flatnonzero(got != want)
    return "" if not bad.size else f"{bad.size} wrong bytes, the first at {origin + int(bad[0]):#x}"


# ------------------------------------------------------------------ one apply
def dev_arena(torch, init: np.ndarray, shift: int = 0):
    """A device arena whose base sits `shift` bytes past a 128-byte line."""
    t = torch.empty(init.size + 256, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 128 == 0
    t = t[shift:shift + init.size]
    t.copy_(torch.from_numpy(init.copy()))
    return t


def place(case, d, bufs):
    """The staging area as the server would leave it: a sentinel, the staged diffs where the
    case puts them.  Returns (the update tuples, the area's view, a copy of its image)."""
    base, view = d.staging()
    assert view.size == 2 * dr.half_of(case.staging_bytes)
    view[:] = STAGE_FILL
    ups = []
    for u, b in zip(case.updates, bufs):
        if u.stage is not None:
            view[u.stage:u.stage + u.length] = b
            ups.append((base + u.stage, u.addr, u.src_lid, u.length))
        else:
            ups.append((b if u.length else None, u.addr, u.src_lid, u.length))
    return ups, view, view.copy()


def apply_case(gpu, case, lid_self, *, shift=0, host_arena=False, digests=False, device_arena=None):
    """The case through a fresh drainer.  Asserts the path, the launches, the arena, the
    staging area and (digests) the live digest array; returns the launches."""
    torch, ec = gpu
    mat = ec.coding_matrix(K, M)
    assert mat[lid_self * K:(lid_self + 1) * K] == dr.RS32_ROWS[lid_self]
    arena0, bufs = inputs(case)
    want = expected(case, lid_self)
    pred = dr.predict_case(case, digests)
    host = alias = live = None
    if device_arena is not None:  # case H: the caller's arena, `origin` its first compared byte
        arena = device_arena
        arena[case.origin:case.origin + arena0.size].copy_(torch.from_numpy(arena0.copy()))
    elif host_arena:
        host = arena0.copy()
        arena = alias = ec.host_register(host)
    else:
        arena = dev_arena(torch, arena0, shift)
    try:
        with ec.Drainer(K, M, mat, lid_self, staging_bytes=case.staging_bytes) as d:
            ups, view, image = place(case, d, bufs)
            if digests:
                n_units = (case.arena + TILE - 1) // TILE
                live = dc.DigestBuffers(torch, 1, n_units)
                ec.digest_region([arena], live.views, case.arena)
                torch.cuda.synchronize()
                d.set_digests(live.views[0], n_units)
            syncs, seq = ec.last_sync()["seq"], ec.last_launch()["seq"]
            launches = d.apply(ups, arena)
            syncs, seq = ec.last_sync()["seq"] - syncs, ec.last_launch()["seq"] - seq
            if host is not None:
                got = host.copy()  # on return, without a device sync
            torch.cuda.synchronize()
            if device_arena is not None:
                got = arena[case.origin:case.origin + arena0.size].cpu().numpy()
            elif host is None:
                got = arena.cpu().numpy()
            stage_bad = "" if pred.path == "pack" else mismatch(view, image)
            report = (f"{case.name} lid {lid_self}: {pred.path}, {launches} launches, {syncs} syncs; arena: "
                      f"{mismatch(got, want, case.origin) or 'ok'}; staging area: {stage_bad or 'ok'}")
            print(report)
            assert np.array_equal(got, want) and not stage_bad, report
            assert launches == seq, report
            if pred.path == "mixed":
                assert launches >= 1, report
            else:
                assert launches == pred.launches, (report, pred.launches)
                assert syncs == (1 if pred.path == "small" else 0), report
            if digests:
                fresh = dc.DigestBuffers(torch, 1, n_units)
                ec.digest_region([arena], fresh.views, case.arena)
                torch.cuda.synchronize()
                assert np.array_equal(live.host(0), fresh.host(0)), report
                assert live.guards_intact() and fresh.guards_intact()
    finally:
        if alias is not None:
            ec.host_unregister(host)
    return launches


# ------------------------------------------------------------------ A-E: the round cutting
@pytest.mark.parametrize("lid_self", LIDS)
@pytest.mark.parametrize("extra", [False, True], ids=["1MiB", "1MiB+16"])
def test_a_small_window_byte_boundary(gpu, engine, lid_self, extra):
    """Exactly 1 MiB of packed diffs: the small path, one launch, its completion recorded.
    Sixteen bytes more: the pack path, two rounds (1 MiB halves), no such completion."""
    assert apply_case(gpu, dr.case_a(extra), lid_self) == (2 if extra else 1)


@pytest.mark.parametrize("lid_self", LIDS)
@pytest.mark.parametrize("extra", [False, True], ids=["8192", "8193"])
def test_b_small_window_tile_boundary(gpu, engine, lid_self, extra):
    """8192 tiles (4096 two-byte updates over a 4 KiB boundary each): the small path.  One
    tile more: the pack path, whose rounds the tile limit of 5120 cuts (2560 + 1537 updates)."""
    assert apply_case(gpu, dr.case_b(extra), lid_self) == (2 if extra else 1)


@pytest.mark.parametrize("lid_self", LIDS)
def test_c_pack_rounds_cut_by_tiles(gpu, engine, lid_self):
    """5200 two-tile updates of 16 packed bytes through 64 KiB halves: bytes alone would make
    two rounds, the 5120 tiles of a half make three (2560 + 2560 + 80 updates)."""
    assert apply_case(gpu, dr.case_c(), lid_self) == 3


@pytest.mark.parametrize("lid_self", LIDS)
def test_d_in_place_tile_rounds(gpu, engine, lid_self):
    """8192 one-byte diffs at consecutive, mostly unaligned bytes of an 8 KiB staging area, up
    to its last byte: four rounds of the in-place path's 2560-tile list, four launches."""
    assert apply_case(gpu, dr.case_d(), lid_self) == 4


@pytest.mark.parametrize("lid_self", LIDS)
def test_e_in_place_wave_cut_by_rounds(gpu, engine, lid_self):
    """D with its last 100 updates on the addresses of the first 100: wave 0 spans all four
    rounds, wave 1 shares the last one -- five launches, the sequential loop's bytes."""
    assert apply_case(gpu, dr.case_e(), lid_self) == 5


# ------------------------------------------------------------------ F: in-place edges
@pytest.mark.parametrize("lid_self", LIDS)
@pytest.mark.parametrize("shift", [0, 1, 16])
def test_f_second_half_of_staging(gpu, lid_self, shift):
    """Three ragged diffs in the second half of the staging area only (the uploaded span
    starts there; one source at an odd offset, one ending on the area's last byte), into an
    arena on a 128-byte line, one byte off a 16-byte boundary, and 16 bytes off the line."""
    assert apply_case(gpu, dr.case_f(), lid_self, shift=shift) == 1


def test_f_buffer_one_byte_before_staging(gpu):
    """A diff whose buffer starts one byte before the staging area is not in place (the small
    path must take it).  The area is an allocation of its own: the byte before it belongs to
    nobody this test knows, and no pinned view that contains it can be made without reading
    memory outside the area.  Skipped on the GPU for that reason; the classification itself
    (inside_area, meets_area and split_by_area of cec_hostplan.hpp, one byte before, one byte
    beyond, ending on the last byte) is tested on the CPU by tests/drain_c/waves_main.cpp."""
    pytest.skip("no view one byte before the staging area exists without touching memory outside it")


# ------------------------------------------------------------------ G: mixed batches
@pytest.mark.parametrize("lid_self", LIDS)
@pytest.mark.parametrize("name", ["G1", "G2", "G3", "G5"])
def test_g_mixed_batch(gpu, lid_self, name):
    """Diffs inside the staging area and diffs elsewhere in one batch.  G1: a pageable diff
    first, 300 staged ones behind it.  G2: pageable at 0, 150 and 299, and 40 staged updates
    on earlier addresses (two waves).  G3: below the small window.  G5: the part outside the
    area is itself several small windows and holds a diff larger than one.  The arena is the
    sequential loop's and every staged source still holds what was put there."""
    case = {"G1": dr.case_g1, "G2": dr.case_g2, "G3": dr.case_g3, "G5": dr.case_g5}[name]()
    apply_case(gpu, case, lid_self)


def test_g2_registered_host_arena(gpu):
    """G2 into a registered host arena: the host copy is right on return, without a sync."""
    apply_case(gpu, dr.case_g2(), 4, host_arena=True)


def test_g4_mixed_batch_with_digests(gpu):
    """G2 with live digests attached: afterwards the live array equals a fresh cec_digest_region
    of the arena (which equals the model), guards intact."""
    apply_case(gpu, dr.case_g2(), 4, digests=True)


# ------------------------------------------------------------------ H: arena offsets around 2^32
@pytest.fixture(scope="module")
def arena_4g(gpu):
    torch, _ = gpu
    need = dr.H_MID + (1 << 20)
    free, _total = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip(f"{free >> 20} MiB of device memory free: under the 8 GiB this test asks for")
    t = torch.empty(need, dtype=torch.uint8, device="cuda")
    yield t
    del t
    torch.cuda.empty_cache()


@pytest.mark.parametrize("staged", [False, True], ids=["small", "in_place"])
@pytest.mark.parametrize("n", [40, 1100])
def test_h_offsets_around_4gib(gpu, arena_4g, n, staged):
    """Ragged updates inside [2^32 - 64 KiB, 2^32 + 64 KiB) of one allocation of 2^32 + 1 MiB
    bytes, one across 2^32, one the two bytes around it, one starting on it: Tile::off, the
    address sort and the kernel's base + off carry 64 bits.  Only the window is initialised
    and compared, with a 4 KiB guard of 0xA5 on each side.  40 updates as the std::sort branch
    of the address sort takes them, 1100 through its radix passes."""
    apply_case(gpu, dr.case_h(n, staged), 4 if staged else 3, device_arena=arena_4g)


# ------------------------------------------------------------------ I: empty work
@pytest.mark.parametrize("staged", [False, True], ids=["null", "in_staging"])
def test_i_only_empty_updates(gpu, staged):
    """Five updates of length 0: no launch, the arena unchanged."""
    assert apply_case(gpu, dr.case_i_empty(staged), 3) == 0


def test_i_leading_empty_update(gpu):
    """An empty first update changes nothing: same launches, same bytes as without it."""
    a, b = dr.case_i_leading_empty(False), dr.case_i_leading_empty(True)
    assert np.array_equal(inputs(a)[0], inputs(b)[0])  # (one seed: the same arena, the same diffs)
    assert all(np.array_equal(x, y) for x, y in zip(inputs(a)[1], inputs(b)[1][1:]))
    assert np.array_equal(expected(a, 4), expected(b, 4))
    assert apply_case(gpu, a, 4) == apply_case(gpu, b, 4) == 2
