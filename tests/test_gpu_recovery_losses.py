"""GPU: recovery at every loss count, against the reference of tests/recovery_case.py.

The combine kernels have a census of their own (tests/test_gpu_kernel_matrix.py); the
recovery ops built on them were run at RS(3,2) / RS(4,2) with one or two lost shards.  The
library allows m = 8, and a combination of more than four outputs runs as successive
launches of four (run_combos), which is only right if no later launch reads what an earlier
one wrote.  These tests run every op that rebuilds shards at every loss count of RS(3,2),
RS(6,4) and RS(10,8), on both engines:

* (a) cec_residual + cec_solve and (b) cec_decode over a plan of full, ragged, misaligned
  and unit-crossing extents: all 209 masks of RS(6,4), recovery_case.loss_sets of RS(10,8);
  all 209 masks in one launch, dealt over 209 small extents;
* (c) recovery sessions, add_peer then solve, every participating parity leading in turn,
  device and pageable buffers; (d) a diff folded between the first and the last peer;
* (e) cec_recovery_finish's fused path, touched and untouched, against the two-step path;
* (f) cec_diff_update with 5, 7 and 8 parities: the same split of one combination.

Every comparison is bit-exact.  Output buffers lie in the 0xA5 sentinel, and bytes no extent
names must come back unchanged; in the plan tests the shards a mask does not name (the lost
ones, the parities left out) are XORed with 0xFF first, so reading one shows.  The sessions
are handed the named buffers only.  The launch count of every split op is asserted from
the launch record.
"""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_matrix_case as kc  # noqa: E402
import recovery_case as rc  # noqa: E402

pytestmark = pytest.mark.gpu

SENT, U, ROW = kc.SENT, kc.TILE, kc.ROW
PAD = 128                      # sentinel bytes either side of a session buffer
UB, UE = 2, 4                  # the sessions' unit range: it does not start at 0
LO, NB = UB * U, (UE - UB + 1) * U
HI = LO + NB
SESSION_ARENA = 6 * U          # a unit either side of the range and one more
DIFF_ADDR, DIFF_LEN = LO + U + 16, 5000  # units 3 and 4 of the range
CODES = [(3, 2), (6, 4), (10, 8)]


def ceil_div(a, b):
    return -(-a // b)


@pytest.fixture(params=[pytest.param(kc.PERM, id="perm"), pytest.param(kc.LDS, id="lds")])
def engine(request, gpu):
    torch, ec = gpu
    default = ec.get_engine()
    ec.set_engine(request.param)
    yield request.param
    ec.set_engine(default)


def dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).cuda()  # (a copy: inputs are read-only)


def seq_now(ec):
    return ec.last_launch()["seq"]


# ------------------------------------------------------------------ shared inputs and references
_CODES: dict = {}


class CodeCase:
    """One code's matrix, seeded shards and parities (with the reference table), computed
    once per session and never written again; the references per mask are cached on it."""

    def __init__(self, ec, oracle, k, m):
        self.k, self.m = k, m
        self.mat = ec.coding_matrix(k, m)
        assert self.mat == oracle.big_vandermonde(k + m, k)
        rng = np.random.default_rng(0x10550 + 100 * k + m)
        # the plan tests' rows
        self.data = rng.integers(0, 256, (k, ROW), dtype=np.uint8)
        self.parity = np.stack(rc.encode(self.mat, k, m, list(self.data)))
        # the sessions' arenas
        self.sdata = rng.integers(0, 256, (k, SESSION_ARENA), dtype=np.uint8)
        self.sparity = np.stack(rc.encode(self.mat, k, m, list(self.sdata)))
        self.diff = rng.integers(0, 256, DIFF_LEN, dtype=np.uint8)
        for a in (self.data, self.parity, self.sdata, self.sparity, self.diff):
            a.setflags(write=False)
        self._plan_ref: dict = {}
        self._full_res: dict = {}

    def coef(self, lid, j):
        return int(self.mat[lid * self.k + j])

    def plan_ref(self, mask):
        """Over the bytes of plan C's extents: {parity: residual} and {lost: bytes}."""
        if mask not in self._plan_ref:
            k, m = self.k, self.m
            surv = {j: self.data[j, IDX_C] for j in rc.surviving_of(k, mask)}
            res = {p: rc.residual_of(self.mat, k, p, self.parity[p - k, IDX_C], surv) for p in rc.pars_of(k, m, mask)}
            sol = rc.solve_lost(self.mat, k, m, mask, res)
            for j, v in sol.items():  # (tests/test_recovery_case.py, on these bytes)
                assert np.array_equal(v, self.data[j, IDX_C]), (k, m, hex(mask), j)
            self._plan_ref[mask] = (res, sol)
        return self._plan_ref[mask]

    def session_residual(self, p, peers, parity=None):
        """residual_of over the sessions' unit range: parity p's bytes and {peer: bytes}."""
        par = self.sparity[p - self.k] if parity is None else parity
        return rc.residual_of(self.mat, self.k, p, par[LO:HI], peers)

    def full_residuals(self, mask):
        """{parity: residual over the unit range with every surviving peer in}, and the
        lost shards solved from them (asserted equal to the data)."""
        if mask not in self._full_res:
            k, m = self.k, self.m
            peers = {j: self.sdata[j, LO:HI] for j in rc.surviving_of(k, mask)}
            res = {p: self.session_residual(p, peers) for p in rc.pars_of(k, m, mask)}
            for j, v in rc.solve_lost(self.mat, k, m, mask, res).items():
                assert np.array_equal(v, self.sdata[j, LO:HI]), (k, m, hex(mask), j)
            self._full_res[mask] = res
        return self._full_res[mask]


def code_case(ec, oracle, k, m) -> CodeCase:
    if (k, m) not in _CODES:
        _CODES[(k, m)] = CodeCase(ec, oracle, k, m)
    return _CODES[(k, m)]


def masks_for(k, m):
    """(a), (b): every mask of RS(6,4); the session subset of RS(10,8)."""
    return rc.all_masks(k, m) if (k, m) == (6, 4) else rc.loss_sets(k, m)


EXT_C = [(o, o, n, 0) for o, n in kc.plan_c()]
IDX_C = np.concatenate([np.arange(o, o + n) for o, n in kc.plan_c()])
assert EXT_C[-1][0] + EXT_C[-1][2] <= kc.ARENA and len(IDX_C) == 2 * U + 100 + 33 + 4097


def unnamed_rows(k, m, mask):
    """The arena rows a mask does not name: the lost shards and the parities left out."""
    return [lid for lid in range(k + m) if not (mask >> lid) & 1]


def assert_slab(got, exp, what):
    if not np.array_equal(got, exp):
        r, p = np.argwhere(got != exp)[0]
        raise AssertionError(f"{what}: row {r} byte {p}: got {got[r, p]:#x} want {exp[r, p]:#x} "
                             f"({int((got != exp).sum())} bytes wrong)")


# ------------------------------------------------------------------ (a) cec_residual + cec_solve
@pytest.mark.parametrize("k,m", [(6, 4), (10, 8)])
def test_residual_solve_every_mask(gpu, oracle, engine, k, m):
    """(a) each participating parity's cec_residual, then one cec_solve, over plan C.  Rows:
    k + m arenas, m residuals (parity p's in row m + p), k outputs.  The residuals equal
    residual_of, the rebuilt bytes the data and solve_lost; a solve of n >= 5 is
    ceil(n / 4) launches."""
    torch, ec = gpu
    C = code_case(ec, oracle, k, m)
    base = np.full((2 * k + 2 * m, ROW), SENT, np.uint8)
    base[:k], base[k:k + m] = C.data, C.parity
    masks = masks_for(k, m)
    assert len(masks) == (209 if (k, m) == (6, 4) else 16)
    with ec.Plan(EXT_C) as plan:
        for mask in masks:
            lost, pars = rc.lost_of(k, mask), rc.pars_of(k, m, mask)
            n = len(lost)
            res, sol = C.plan_ref(mask)
            host0 = base.copy()
            host0[np.ix_(unnamed_rows(k, m, mask), IDX_C)] ^= 0xFF
            exp = host0.copy()
            for p in pars:
                exp[m + p, IDX_C] = res[p]
            for j in lost:
                exp[k + 2 * m + j, IDX_C] = sol[j]
            slab = dev(torch, host0)
            rows = [slab[r] for r in range(len(host0))]
            seq0 = seq_now(ec)
            for p in pars:
                ec.residual(k, m, C.mat, p, mask, rows[:k + m], rows[m + p], plan)
            assert seq_now(ec) == seq0 + n, hex(mask)
            ec.solve(k, m, C.mat, mask, [rows[m + lid] if lid in pars else None for lid in range(k + m)],
                     [rows[k + 2 * m + j] if j in lost else None for j in range(k)], plan)
            assert seq_now(ec) == seq0 + n + ceil_div(n, 4), (hex(mask), n)
            torch.cuda.synchronize()
            assert_slab(slab.cpu().numpy(), exp, f"RS({k},{m}) mask {mask:#x} residual + solve")


# ------------------------------------------------------------------ (b) cec_decode
@pytest.mark.parametrize("k,m", [(6, 4), (10, 8)])
def test_decode_every_mask(gpu, oracle, engine, k, m):
    """(b) cec_decode of one mask per launch over plan C.  Rows: k + m arenas, k outputs."""
    torch, ec = gpu
    C = code_case(ec, oracle, k, m)
    base = np.full((2 * k + m, ROW), SENT, np.uint8)
    base[:k], base[k:k + m] = C.data, C.parity
    with ec.Plan(EXT_C) as plan:
        for mask in masks_for(k, m):
            lost = rc.lost_of(k, mask)
            host0 = base.copy()
            host0[np.ix_(unnamed_rows(k, m, mask), IDX_C)] ^= 0xFF
            exp = host0.copy()
            for j in lost:
                exp[k + m + j, IDX_C] = C.data[j, IDX_C]
            slab = dev(torch, host0)
            rows = [slab[r] for r in range(len(host0))]
            seq0 = seq_now(ec)
            ec.decode(k, m, C.mat, [mask], rows[:k + m], rows[k + m:], plan)
            assert seq_now(ec) == seq0 + ceil_div(len(lost), 4), hex(mask)
            torch.cuda.synchronize()
            assert_slab(slab.cpu().numpy(), exp, f"RS({k},{m}) mask {mask:#x} decode")


def test_decode_all_masks_in_one_launch(gpu, oracle, engine):
    """(b) RS(6,4): all 209 masks dealt over 209 extents of 48 bytes at 16-byte-aligned
    offsets, one launch: loss counts 1..4 side by side on the 8 x 4 capacity kernel."""
    torch, ec = gpu
    k, m = 6, 4
    mat = ec.coding_matrix(k, m)
    masks = rc.all_masks(k, m)
    assert len(masks) == 209
    ext = [(16 + 64 * e, 16 + 64 * e, 48, e) for e in range(len(masks))]
    row = ext[-1][0] + 48 + 16
    row += -row % 128
    rng = np.random.default_rng(0xA11 + engine)
    data = rng.integers(0, 256, (k, row), dtype=np.uint8)
    host0 = np.full((2 * k + m, row), SENT, np.uint8)
    host0[:k] = data
    host0[k:k + m] = np.stack(rc.encode(mat, k, m, list(data)))
    for (off, _, n, e) in ext:
        host0[unnamed_rows(k, m, masks[e]), off:off + n] ^= 0xFF
    exp = host0.copy()
    for (off, _, n, e) in ext:
        for j in rc.lost_of(k, masks[e]):
            exp[k + m + j, off:off + n] = data[j, off:off + n]
    slab = dev(torch, host0)
    rows = [slab[r] for r in range(len(host0))]
    seq0 = seq_now(ec)
    with ec.Plan(ext) as plan:
        ec.decode(k, m, mat, masks, rows[:k + m], rows[k + m:], plan)
        rec = ec.last_launch()
        torch.cuda.synchronize()
    assert rec["seq"] == seq0 + 1, rec
    assert (rec["kind"], rec["nt"], rec["lt"], rec["acc"]) == (kc.GENERIC, 8, 4, kc.ACC_RUNTIME), rec
    assert rec["engine"] == engine, rec
    assert_slab(slab.cpu().numpy(), exp, "RS(6,4) 209 masks in one launch")


# ------------------------------------------------------------------ session buffers
class Guarded:
    """A buffer of n bytes with PAD sentinel bytes either side, on the device or pageable."""

    def __init__(self, torch, n, payload=None, device=True):
        host = np.full(n + 2 * PAD, SENT, np.uint8)
        if payload is not None:
            host[PAD:PAD + n] = payload
        self.n, self.device = n, device
        self.buf = dev(torch, host) if device else host

    @property
    def view(self):
        return self.buf[PAD:PAD + self.n]

    def bytes(self, what="") -> np.ndarray:
        """The n bytes; the sentinel either side must be whole."""
        whole = self.buf.cpu().numpy() if self.device else self.buf
        assert (whole[:PAD] == SENT).all() and (whole[PAD + self.n:] == SENT).all(), f"{what}: written out of bounds"
        return whole[PAD:PAD + self.n]


class Sessions:
    """What the session tests share for one code: the parity arenas and every data shard's
    units of the range on the device, checked unchanged at the end."""

    def __init__(self, torch, ec, C: CodeCase):
        self.torch, self.ec, self.C = torch, ec, C
        self.pdev = [dev(torch, p) for p in C.sparity]
        self.units = [Guarded(torch, NB, C.sdata[j, LO:HI]) for j in range(C.k)]
        self.tmp = torch.empty(NB, dtype=torch.uint8, device="cuda")

    def open(self, stack, p, mask):
        C = self.C
        rec = stack.enter_context(self.ec.Recovery(C.k, C.m, C.mat, p, mask, UB, UE, self.pdev[p - C.k]))
        assert rec.nbytes == NB and not rec.complete
        return rec

    def residual(self, rec) -> np.ndarray:
        self.ec.region_multiply(rec.residual, 1, NB, self.tmp, 0)  # copy the device residual out
        self.torch.cuda.synchronize()
        return self.tmp.cpu().numpy()

    def outputs(self, lost, device=True):
        return {j: Guarded(self.torch, NB, None, device) for j in lost}

    def check_outputs(self, outs, what, data=None):
        data = self.C.sdata if data is None else data
        for j, g in outs.items():
            got = g.bytes(what)
            want = data[j, LO:HI]
            assert np.array_equal(got, want), (f"{what}: rebuilt shard {j}: {int((got != want).sum())} of {NB} bytes "
                                               f"wrong, first at {int(np.argmax(got != want))}")

    def check_inputs(self):
        for p, t in enumerate(self.pdev):
            assert np.array_equal(t.cpu().numpy(), self.C.sparity[p]), f"parity arena {p} was written"
        for j, g in enumerate(self.units):
            assert np.array_equal(g.bytes(f"units of shard {j}"), self.C.sdata[j, LO:HI]), f"units of shard {j} written"


def what_of(C, mask, leader=None, extra=""):
    s = f"RS({C.k},{C.m}) mask {mask:#x} lost {rc.lost_of(C.k, mask)} parities {rc.pars_of(C.k, C.m, mask)}"
    return s + (f" leader {leader}" if leader is not None else "") + (f" {extra}" if extra else "")


# ------------------------------------------------------------------ (c) sessions, two-step
def run_two_step(S: Sessions, mask, descending, pageable):
    """One session per participating parity; every surviving lid's add_peer in the given
    order, the residual read back and compared after each; then every parity leads a solve
    with the others' residuals as read back."""
    C, ec, torch = S.C, S.ec, S.torch
    k, m = C.k, C.m
    lost, pars, surv = rc.lost_of(k, mask), rc.pars_of(k, m, mask), rc.surviving_of(k, mask)
    n = len(lost)
    with contextlib.ExitStack() as stack:
        recs = {p: S.open(stack, p, mask) for p in pars}
        sent, res = {}, {}
        for j in (surv[::-1] if descending else surv):
            sent[j] = C.sdata[j, LO:HI]
            for p in pars:
                recs[p].add_peer(j, S.units[j].view)
                res[p] = S.residual(recs[p])
                assert np.array_equal(res[p], C.session_residual(p, sent)), \
                    what_of(C, mask, extra=f"residual of {p} after peers {sorted(sent)}")
                assert recs[p].complete == (len(sent) == len(surv))
        for leader in pars:
            what = what_of(C, mask, leader, "pageable" if pageable else "device")
            peers = {q: Guarded(torch, NB, res[q], device=not pageable) for q in pars if q != leader}
            outs = S.outputs(lost, device=not pageable)
            seq0 = seq_now(ec)
            recs[leader].solve({q: g.view for q, g in peers.items()}, {j: g.view for j, g in outs.items()})
            if not pageable:
                assert seq_now(ec) == seq0 + ceil_div(n, 4), what
            torch.cuda.synchronize()
            S.check_outputs(outs, what)
            for q, g in peers.items():
                assert np.array_equal(g.bytes(what), res[q]), f"{what}: residual of {q} written"
            assert np.array_equal(S.residual(recs[leader]), res[leader]), f"{what}: solve changed the residual"


@pytest.mark.parametrize("k,m", CODES)
def test_sessions_two_step(gpu, oracle, engine, k, m):
    """(c) add_peer + solve at every loss count of loss_sets, every participating parity
    leading in turn: peers in ascending and in descending order on device buffers, and one
    pass with pageable peer residuals and outputs (up to 15 staged buffers in one call)."""
    torch, ec = gpu
    S = Sessions(torch, ec, code_case(ec, oracle, k, m))
    sets = rc.loss_sets(k, m)
    assert [len(rc.lost_of(k, s)) for s in sets] == [n for n in range(1, min(m, k - 1) + 1) for _ in (0, 1)]
    for mask in sets:
        run_two_step(S, mask, descending=False, pageable=False)
        run_two_step(S, mask, descending=True, pageable=False)
        run_two_step(S, mask, descending=False, pageable=True)
    S.check_inputs()


# ------------------------------------------------------------------ (d) fold_update at n >= 2
def run_fold(S: Sessions, mask):
    """A write to the last surviving peer lands between the first and the last add_peer: the
    diff is folded into every participating session, the peer then ships its new bytes."""
    C, ec, torch = S.C, S.ec, S.torch
    k, m = C.k, C.m
    lost, pars, surv = rc.lost_of(k, mask), rc.pars_of(k, m, mask), rc.surviving_of(k, mask)
    assert len(lost) >= 2 and len(surv) >= 2
    first, last = surv[0], surv[-1]
    new_last = C.sdata[last].copy()
    new_last[DIFF_ADDR:DIFF_ADDR + DIFF_LEN] ^= C.diff
    new_units = Guarded(torch, NB, new_last[LO:HI])
    ddiff = dev(torch, C.diff)
    res = {}
    with contextlib.ExitStack() as stack:
        recs = {p: S.open(stack, p, mask) for p in pars}
        for i, p in enumerate(pars):
            rec, what = recs[p], what_of(C, mask, extra=f"fold into {p}")
            diff = ddiff if i % 2 == 0 else C.diff.copy()  # device and pageable diffs
            new_parity = C.sparity[p - k].copy()
            new_parity[DIFF_ADDR:DIFF_ADDR + DIFF_LEN] ^= kc.MUL[C.coef(p, last)][C.diff]
            # before first touch: the parity arena picks the update up; nothing to fold
            before = S.residual(rec)
            assert rec.fold_update(first, DIFF_ADDR, diff) == 0, what
            assert np.array_equal(S.residual(rec), before), what
            sent = {}
            for j in surv[:-1]:
                rec.add_peer(j, S.units[j].view)
                sent[j] = C.sdata[j, LO:HI]
            before = S.residual(rec)
            assert np.array_equal(before, C.session_residual(p, sent)), what
            # a peer that already contributed sent post-update bytes; nothing to fold
            assert rec.fold_update(first, DIFF_ADDR, diff) == 0, what
            assert np.array_equal(S.residual(rec), before), what
            # the fold for the peer still to come: units 3 and 4
            assert rec.fold_update(last, DIFF_ADDR, diff) == 2, what
            assert np.array_equal(S.residual(rec), C.session_residual(p, sent, new_parity)), what
            assert not rec.complete
            rec.add_peer(last, new_units.view)
            sent[last] = new_last[LO:HI]
            res[p] = S.residual(rec)
            assert np.array_equal(res[p], C.session_residual(p, sent, new_parity)), what
            assert rec.complete
        for leader in pars:
            what = what_of(C, mask, leader, "after a fold")
            peers = {q: Guarded(torch, NB, res[q]) for q in pars if q != leader}
            outs = S.outputs(lost)
            recs[leader].solve({q: g.view for q, g in peers.items()}, {j: g.view for j, g in outs.items()})
            torch.cuda.synchronize()
            S.check_outputs(outs, what)
    assert np.array_equal(new_units.bytes(), new_last[LO:HI])


@pytest.mark.parametrize("k,m", [(6, 4), (10, 8)])
def test_sessions_fold_update_multi_loss(gpu, oracle, engine, k, m):
    """(d) every loss set with n >= 2 lost and k - n >= 2 surviving (RS(3,2) has none: its
    double loss leaves one peer, which is first and last at once).  Residuals equal
    residual_of over the updated parity and the updated peer's bytes, the rebuilt shards
    the lost data; a fold before first touch and one for a peer that already contributed
    return 0 and leave the residual alone."""
    torch, ec = gpu
    assert all(len(rc.lost_of(3, s)) < 2 or len(rc.surviving_of(3, s)) < 2 for s in rc.loss_sets(3, 2))
    S = Sessions(torch, ec, code_case(ec, oracle, k, m))
    sets = [s for s in rc.loss_sets(k, m) if len(rc.lost_of(k, s)) >= 2 and len(rc.surviving_of(k, s)) >= 2]
    assert len(sets) == {(6, 4): 6, (10, 8): 14}[(k, m)]
    for mask in sets:
        run_fold(S, mask)
    S.check_inputs()


# ------------------------------------------------------------------ (e) cec_recovery_finish, fused
def run_finish(S: Sessions, mask, leader, engine):
    """The leader's last peer through cec_recovery_finish (device units, outputs and peer
    residuals: the fused path) and, in a second session on the same inputs, through
    add_peer + solve.  Touched (k - n >= 2): every surviving lid but the last went in
    before; untouched (k - n == 1): finish reads the parity arena itself."""
    C, ec, torch = S.C, S.ec, S.torch
    k, m = C.k, C.m
    lost, pars, surv = rc.lost_of(k, mask), rc.pars_of(k, m, mask), rc.surviving_of(k, mask)
    n = len(lost)
    full = C.full_residuals(mask)
    what = what_of(C, mask, leader, "finish, touched" if len(surv) >= 2 else "finish, untouched")
    last = surv[-1]
    peers = {q: Guarded(torch, NB, full[q]) for q in pars if q != leader}
    pr = {q: g.view for q, g in peers.items()}
    with contextlib.ExitStack() as stack:
        fused, two = S.open(stack, leader, mask), S.open(stack, leader, mask)
        for rec in (fused, two):
            sent = {}
            for j in surv[:-1]:
                rec.add_peer(j, S.units[j].view)
                sent[j] = C.sdata[j, LO:HI]
            if sent:
                assert np.array_equal(S.residual(rec), C.session_residual(leader, sent)), what
            assert not rec.complete
        outs_f, outs_t = S.outputs(lost), S.outputs(lost)
        torch.cuda.synchronize()
        seq0 = seq_now(ec)
        fused.finish(last, S.units[last].view, pr, {j: g.view for j, g in outs_f.items()})
        rec = ec.last_launch()
        assert rec["seq"] == seq0 + ceil_div(n + 1, 4), (what, rec)
        assert rec["engine"] == engine, (what, rec)
        if n <= 3:  # one launch: the last peer, the residual and the other parities' in, R' and n shards out
            assert (rec["kind"], rec["nt"], rec["lt"]) == (kc.EXACT, 1 + n, 1 + n), (what, rec)
        two.add_peer(last, S.units[last].view)
        two.solve(pr, {j: g.view for j, g in outs_t.items()})
        torch.cuda.synchronize()
        assert fused.complete and two.complete, what
        S.check_outputs(outs_f, what)
        S.check_outputs(outs_t, what + " (two-step)")
        res_f, res_t = S.residual(fused), S.residual(two)
        assert np.array_equal(res_f, full[leader]), f"{what}: residual"
        assert np.array_equal(res_t, full[leader]), f"{what}: residual (two-step)"
        for j in lost:
            assert np.array_equal(outs_f[j].bytes(), outs_t[j].bytes()), f"{what}: shard {j} differs from the two-step path"
        for q, g in peers.items():
            assert np.array_equal(g.bytes(what), full[q]), f"{what}: residual of {q} written"


def finish_sets(k, m):
    """(loss set, touched): CODES run all their loss sets; the one-off codes RS(5,4) and
    RS(9,8) only the sets that lose k - 1 shards (4 and 8), the untouched case past 3 losses."""
    sets = rc.loss_sets(k, m)
    if (k, m) not in CODES:
        sets = [s for s in sets if len(rc.surviving_of(k, s)) == 1]
    return [(s, len(rc.surviving_of(k, s)) >= 2) for s in sets]


@pytest.mark.parametrize("k,m", CODES + [(5, 4), (9, 8)])
def test_finish_fused_every_loss_count(gpu, oracle, engine, k, m):
    """(e) cec_recovery_finish at every loss count, every participating parity leading:
    rebuilt shards equal the data, the residual residual_of, the session is complete, and
    all of it is what add_peer + solve leave.  ceil((n + 1) / 4) launches; up to three
    losses one exact launch of (1 + n) x (1 + n).  Past three losses the combination
    splits, and R' -- which overwrites the touched session's residual, an input -- must be
    written by the last launch: with R' first, every shard after the third is rebuilt
    from the new residual and loses the last peer's contribution."""
    torch, ec = gpu
    S = Sessions(torch, ec, code_case(ec, oracle, k, m))
    sets = finish_sets(k, m)
    untouched = [s for s, touched in sets if not touched]
    assert len(untouched) == {(3, 2): 2, (6, 4): 0, (10, 8): 0, (5, 4): 2, (9, 8): 2}[(k, m)]
    if (k, m) in CODES:
        assert len(sets) == 2 * min(m, k - 1)
    for mask, _ in sets:
        for leader in rc.pars_of(k, m, mask):
            run_finish(S, mask, leader, engine)
    S.check_inputs()


# ------------------------------------------------------------------ (f) diff-update past four parities
@pytest.mark.parametrize("install", [False, True], ids=["plain", "install"])
@pytest.mark.parametrize("m", [5, 7, 8])
def test_diff_update_past_four_parities(gpu, engine, m, install):
    """(f) cec_diff_update, k = 2 and m parities (+ the install): ceil(outputs / 4) launches
    over plan A and plan B.  The reference computes every parity from the bytes before the
    op, so an install that ran before a launch that reads the old bytes would show; the
    record of the last launch holds the write output (the install) where there is one."""
    torch, ec = gpu
    case = kc.Case(torch, ec)
    rng = np.random.default_rng(0xF00D + 16 * m + install + 2 * engine)
    outputs = m + install
    launches = ceil_div(outputs, 4)
    lt_last = outputs - 4 * (launches - 1)
    # the last launch: all XOR, or the parities XOR and the install written last
    acc = kc.ACC_ALL if not install else kc.ACC_NONE if lt_last == 1 else kc.ACC_ABL
    for which in ("A", "B"):
        for low in (False, True):
            n_rows, patterns, call = kc.diff_update_op(2, m, kc.coef_rows(rng, 2, m, low), install)
            kc.run_op(case, rng, which, n_rows, patterns, lambda rows, plan: call(ec, rows, plan),
                      launches=launches, kind=kc.EXACT, nt=2, lt=lt_last, acc=acc, engine=engine,
                      what=f"diff_update m={m} install={install} low={low}")
