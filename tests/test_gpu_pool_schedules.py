"""GPU: random schedules of the recovery pool against the model of tests/pool_schedule_case.py.

One pool of 24 units over arenas of 32 units per case; RS(3,2), RS(6,4), RS(3,4) and RS(10,8)
with the leaders of pool_schedule_case.CODES, each seed started on the PERM and on the LDS
engine (the schedule switches anyway).  The generator draws every step from the model, so the
steps are those of the dry run that tests/test_pool_schedule_case.py holds to its coverage
conditions; what the pool does is compared with what the model predicts:

  after every step   the call's return value (requests folded or solved, units folded per
                     update, CEC_EFULL of a full probe, CEC_EINVAL of a solve list with a request
                     that is not ready and of a residual read of a request that holds none);
                     complete, ready and solved of every live request, and active;
                     both output slabs (device and pinned, k arenas each in the 0xA5 sentinel)
                     whole, byte for byte -- a solve may write only its own units of its own
                     lost lids, and no other call may write any; output(rid, x) of every live
                     request for every x, None where the model says so
  after a read       residual(rid), with the guard bytes either side of its destination
  at the end         residual of every live request that holds one; then all are ended, and the
                     parity arena, and every reply, residual and diff buffer handed to the pool
                     (pageable and device ones between guard bytes) are compared unwritten

Every comparison is bit-exact.  On a mismatch the code, seed, step index and step are in the
assertion, and the steps so far with the model's request table are written to tmp_path: the
cause is found by replaying the model on a CPU.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_matrix_case as kc  # noqa: E402
import pool_schedule_case as ps  # noqa: E402

pytestmark = pytest.mark.gpu

SENT, U = kc.SENT, kc.TILE
PAD = 128
CASES = [pytest.param(k, m, seed, id=f"rs{k}_{m}-seed{seed}") for (k, m), cfg in ps.CODES.items() for seed in cfg["seeds"]]


class Runner:
    """Drives one pool through the steps the model has just taken."""

    def __init__(self, torch, ec, k, m, mat, seed, start_engine, tmp_path):
        self.torch, self.ec, self.k, self.m, self.mat, self.seed = torch, ec, k, m, mat, seed
        self.engines = [start_engine, kc.LDS if start_engine == kc.PERM else kc.PERM]
        self.tmp_path = tmp_path
        self.ids: dict = {}       # handle -> request id
        self.guards: list = []    # (buffer, its bytes when handed over)
        self.done: list = []      # the steps so far
        self.streams = [None, torch.cuda.Stream(), torch.cuda.Stream()]
        self.pool = None

    # ---------------------------------------------------------------- buffers
    def start(self, model):
        torch = self.torch
        self.ec.set_engine(self.engines[0])
        self.parity = torch.from_numpy(model.P.copy()).cuda()
        self.slabs = {"dev": torch.full((self.k, ps.ARENA), SENT, dtype=torch.uint8, device="cuda"),
                      "pin": torch.full((self.k, ps.ARENA), SENT, dtype=torch.uint8).pin_memory()}
        torch.cuda.synchronize()
        self.pool = self.ec.RecoveryPool(self.k, self.m, self.mat, model.leader, self.parity, capacity_units=ps.CAP)

    def guarded(self, payload, device, off=0):
        """payload between guard bytes, pageable or device; the view to hand over."""
        n = len(payload)
        host = np.full(n + 2 * PAD + off, SENT, np.uint8)
        host[PAD + off:PAD + off + n] = payload
        whole = self.torch.from_numpy(host.copy()).cuda() if device else host
        self.guards.append((whole, host.copy()))
        return whole[PAD + off:PAD + off + n]

    def hand_over(self, step, out, staging):
        """(ids, lids, buffers or staging addresses) of a replies / residuals step."""
        ids, lids, bufs = [], [], []
        for (h, lid, way), payload in zip(step["items"], out.payload):
            rid = self.ids[h]
            if way == "staging":
                addr, view = staging(rid, lid)
                assert len(view) == len(payload)
                view[:] = payload
                bufs.append(addr)
            else:
                bufs.append(self.guarded(payload, way == "device"))
            ids.append(rid)
            lids.append(lid)
        return ids, lids, bufs

    def arenas(self, slab, none_lid=None):
        return [None if j == none_lid else self.slabs[slab][j] for j in range(self.k)]

    def refused(self, call, *args, **kw):
        """The call's status: 0, or the code it was refused with."""
        try:
            call(*args, **kw)
        except self.ec.CecError as e:
            return e.code
        return 0

    # ---------------------------------------------------------------- one step
    def execute(self, step, out, model):
        ec, pool, op = self.ec, self.pool, step["op"]
        stream = self.streams[step.get("stream", 0)]
        if op == "begin":
            if step["expect"] == "full":
                assert self.refused(pool.begin, step["mask"], step["ub"], step["ue"]) == ps.EFULL
            else:
                rid = pool.begin(step["mask"], step["ub"], step["ue"])
                assert rid >= 0 and rid not in self.ids.values(), rid
                self.ids[step["h"]] = rid
        elif op == "replies":
            ids, lids, bufs = self.hand_over(step, out, pool.staging)
            if step["batch"]:
                pool.add_peers(ids, lids, bufs)
            else:
                pool.add_peer(ids[0], lids[0], bufs[0])
        elif op == "residuals":
            ids, lids, bufs = self.hand_over(step, out, pool.parity_staging)
            if step["batch"]:
                pool.add_residuals(ids, lids, bufs)
            else:
                pool.add_residual(ids[0], lids[0], bufs[0])
        elif op == "flush":
            assert pool.flush(stream) == out.ret
        elif op == "flush_solve":
            assert pool.flush_solve(self.arenas(step["slab"], step["none_lid"]), stream) == out.ret
        elif op == "flush_solve_host":
            assert pool.flush_solve_host(stream) == out.ret
        elif op == "solve":
            rids = [self.ids[h] for h in step["hs"]]
            assert self.refused(pool.solve, rids, self.arenas(step["slab"]), stream) == out.ret
        elif op == "solve_host":
            rids = [self.ids[h] for h in step["hs"]]
            assert self.refused(pool.solve_host, rids, stream) == out.ret
        elif op == "fold_update":
            buf = self.guarded(out.payload[0], step["way"] == "device", step["boff"])
            assert pool.fold_update(step["peer"], step["addr"], buf, stream) == out.ret
        elif op == "fold_updates":
            ups = [(self.guarded(d, False, u["boff"]), u["addr"], u["peer"]) for u, d in zip(step["ups"], out.payload)]
            assert pool.fold_updates(ups, stream) == out.ret
        elif op == "residual":
            r = model.reqs[step["h"]]
            dst = self.guarded(np.full(r.n * U, SENT, np.uint8), step["way"] == "device")
            whole, want = self.guards.pop()
            assert self.refused(pool.residual, self.ids[step["h"]], dst, stream) == out.ret
            if out.read is not None:
                want[PAD:PAD + r.n * U] = out.read
            got = whole.cpu().numpy() if hasattr(whole, "cpu") else whole
            assert np.array_equal(got, want), "residual (with its guard bytes)"
        elif op == "end":
            pool.end(self.ids.pop(step["h"]))
        elif op == "engine":
            ec.set_engine(self.engines[model.engine])
        # the caller's own apply of the diffs to the parity arena, after the fold
        for addr, ln in out.p_ranges:
            self.parity[addr:addr + ln] = self.torch.from_numpy(model.P[addr:addr + ln].copy()).cuda()
        if out.p_ranges:
            self.torch.cuda.synchronize()

    def compare(self, model):
        pool = self.pool
        assert pool.active == len(model.reqs) == len(self.ids)
        for h, r in model.reqs.items():
            rid = self.ids[h]
            got = (pool.complete(rid), pool.ready(rid), pool.solved(rid))
            assert got == (model.complete(r), model.ready(r), r.solved), f"handle {h}: complete, ready, solved {got}"
        for name, slab in self.slabs.items():
            got, want = slab.cpu().numpy(), model.out[name]
            if not np.array_equal(got, want):
                j, p = np.argwhere(got != want)[0]
                raise AssertionError(f"{name} arena {j} byte {p} (unit {p // U}): got {got[j, p]:#x} want "
                                     f"{want[j, p]:#x}, {int((got != want).sum())} bytes wrong")
        for h, r in model.reqs.items():
            for x in range(len(model.lost(r)) + 1):
                got, want = pool.output(self.ids[h], x), model.output(r, x)
                assert (got is None) == (want is None), f"handle {h}: output({x}) {'missing' if got is None else 'there'}"
                assert got is None or np.array_equal(got, want), f"handle {h}: host plane {x}"

    def on_step(self, i, step, out, model):
        self.done.append(step)
        try:
            self.execute(step, out, model)
            self.compare(model)
        except (AssertionError, self.ec.CecError) as e:
            path = os.path.join(str(self.tmp_path), f"rs{self.k}_{self.m}_seed{self.seed}_engine{self.engines[0]}.json")
            with open(path, "w") as f:
                json.dump(dict(k=self.k, m=self.m, seed=self.seed, start_engine=self.engines[0], failed_step=i,
                               steps=self.done, requests=model.table(), ids={str(h): v for h, v in self.ids.items()}), f)
            raise AssertionError(f"RS({self.k},{self.m}) seed {self.seed} start engine {self.engines[0]} step {i} "
                                 f"{step}: {e} (steps and the model's requests: {path})") from e

    def close(self, model):
        assert self.pool.active == 0 and not model.reqs
        self.torch.cuda.synchronize()
        assert np.array_equal(self.parity.cpu().numpy(), model.P), "the parity arena was written"
        for whole, want in self.guards:
            got = whole.cpu().numpy() if hasattr(whole, "cpu") else whole
            assert np.array_equal(got, want), "a buffer handed to the pool was written"
        self.pool.destroy()


@pytest.mark.parametrize("start_engine", [pytest.param(kc.PERM, id="perm"), pytest.param(kc.LDS, id="lds")])
@pytest.mark.parametrize("k,m,seed", CASES)
def test_pool_random_schedule(gpu, oracle, tmp_path, k, m, seed, start_engine):
    torch, ec = gpu
    mat = ec.coding_matrix(k, m)
    assert mat == oracle.big_vandermonde(k + m, k)  # the matrix the CPU tie-down of the model used
    default = ec.get_engine()
    run = Runner(torch, ec, k, m, mat, seed, start_engine, tmp_path)
    try:
        model, steps = ps.schedule(k, m, mat, seed, on_step=run.on_step, on_start=run.start)
        assert ps.coverage_gaps(model) == []
        ps.finish(model, run.on_step, len(steps))
        run.close(model)
    finally:
        ec.set_engine(default)
        if run.pool is not None:
            run.pool.destroy()


def test_residual_of_a_request_that_holds_none_is_refused(gpu):
    """A live request whose mask names data lids and that no reply has reached holds no
    residual: CEC_EINVAL, nothing copied, nothing flushed; after its first reply it is read."""
    torch, ec = gpu
    k, m, leader = 3, 2, 4
    mat = ec.coding_matrix(k, m)
    rng = np.random.default_rng(0x9006)
    parity = rng.integers(0, 256, 4 * U, dtype=np.uint8)
    reply = rng.integers(0, 256, 2 * U, dtype=np.uint8)
    arena = torch.from_numpy(parity).cuda()  # (kept alive: the pool reads it at every first touch)
    with ec.RecoveryPool(k, m, mat, leader, arena, capacity_units=4) as pool:
        other = pool.begin(0b10110, 0, 0)
        pool.add_peer(other, 1, reply[:U])        # stays queued: the refused read flushes nothing
        rid = pool.begin(0b10110, 1, 2)
        for dst in (np.full(2 * U, SENT, np.uint8), torch.full((2 * U,), SENT, dtype=torch.uint8, device="cuda")):
            with pytest.raises(ec.CecError) as e:
                pool.residual(rid, dst)
            assert e.value.code == ec.CEC_EINVAL
            assert (np.asarray(dst.cpu() if hasattr(dst, "cpu") else dst) == SENT).all()
        assert pool.flush() == 1
        pool.add_peer(rid, 2, reply)
        got = np.zeros(2 * U, np.uint8)
        pool.residual(rid, got)
        assert np.array_equal(got, parity[U:3 * U] ^ kc.MUL[int(mat[leader * k + 2])][reply])
        pool.end(rid)
        pool.end(other)
