"""Every compiled instantiation of combine_kernel against a bit-serial GF(2^8) reference.

The body of tests/test_gpu_kernel_matrix.py, in a plain module so that it runs in-process
and as a child under a pinned environment (the library reads CEC_STORE_POLICY and
CEC_SPLIT_SHIFT once per process):

    python tests/kernel_matrix_case.py --expect-wt 0        (with CEC_STORE_POLICY=nt)
    python tests/kernel_matrix_case.py --expect-split 1     (with CEC_SPLIT_SHIFT=1)

runs check_exact_shapes on both engines and prints "OK".

The reference is the 256 x 256 product table built here by shift-and-add with reduction
by 0x11D, bit by bit; nothing of oracle/ or of the library's tables is read.  Expected
bytes are XOR_i MUL[coef[l][i]][in_i], XORed onto the previous contents for accumulate
outputs.  Every comparison is bit-exact, and after every launch the launch record
(ec.last_launch) is asserted: which kernel ran is part of what is tested.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SENT = 0xA5
TILE = 4096
ARENA = 6 * TILE          # bytes of every arena an extent may touch
SRC_SHIFT = 256           # src_off = off + SRC_SHIFT: the two addressings never coincide
ROW = ARENA + 2 * SRC_SHIFT  # row stride of the slab: a multiple of 128

PERM, LDS = 0, 1
NARROW, EXACT, GENERIC = 0, 1, 2
ACC_NONE, ACC_ALL, ACC_ABL, ACC_RUNTIME = 0, 1, 2, 3
SYS_RELEASE, WRITE_THROUGH = 1, 2


def mul_table() -> np.ndarray:
    """MUL[a][b] = a * b in GF(2^8) mod x^8 + x^4 + x^3 + x^2 + 1 (0x11D), bit-serial."""
    a = np.repeat(np.arange(256, dtype=np.uint16)[:, None], 256, axis=1)
    b = np.repeat(np.arange(256, dtype=np.uint16)[None, :], 256, axis=0)
    p = np.zeros((256, 256), np.uint16)
    for bit in range(8):
        p ^= np.where((b >> bit) & 1, a, 0).astype(np.uint16)
        a = (a << 1).astype(np.uint16)
        a = np.where(a & 0x100, a ^ 0x11D, a).astype(np.uint16)
    assert p.max() < 256
    return p.astype(np.uint8)


MUL = mul_table()


def gf_inv(a: int) -> int:
    (hit,) = np.nonzero(MUL[a] == 1)
    assert len(hit) == 1, a
    return int(hit[0])


def combine(coefs, xs) -> np.ndarray:
    acc = np.zeros(len(xs[0]), np.uint8)
    for c, x in zip(coefs, xs):
        acc ^= MUL[int(c)][x]
    return acc


# ------------------------------------------------------------------ instantiations
def inst(rec: dict) -> tuple:
    """(engine, kind, nt, lt, acc, system release) of a launch record: one compiled kernel.
    The release is a template parameter of the narrow kernels only."""
    rel = rec["kind"] == NARROW and bool(rec["flags"] & SYS_RELEASE)
    return (rec["engine"], rec["kind"], rec["nt"], rec["lt"], rec["acc"], rel)


def all_instantiations() -> set:
    """What launch_narrow, launch_exact and launch_generic compile, per engine: 4 + 40 + 12."""
    s = set()
    for e in (PERM, LDS):
        for acc in (ACC_NONE, ACC_ALL):
            for rel in (False, True):
                s.add((e, NARROW, 1, 1, acc, rel))
        for n in range(1, 9):
            for l in range(1, 5):
                s.add((e, EXACT, n, l, ACC_NONE, False))
        s.add((e, EXACT, 1, 1, ACC_ALL, False))
        for l in range(1, 5):
            s.add((e, EXACT, 2, l, ACC_ALL, False))
        for l in range(2, 5):
            s.add((e, EXACT, 2, l, ACC_ABL, False))
        for nt in (2, 4, 8, 16):
            for lt in (1, 2, 4):
                s.add((e, GENERIC, nt, lt, ACC_RUNTIME, False))
    return s


# Compiled, but no public call lands on them (per engine), and why.  A change to the
# dispatch (has_exact, exact_shape, launch_generic, the narrow rule) that makes one of
# these reachable, or another one unreachable, fails the census in the test file.
UNREACHABLE = {
    # every 1 x 1 accumulate op (cec_apply_diffs, the drainer, the recovery folds, the host
    # batch's XOR jobs, region multiply-XOR) names stream slots 0 and 1 only, and such a
    # launch takes the narrow two-slot kernel; the 48-slot 1 x 1 accumulate kernel is left
    # to callers that do not exist yet
    (EXACT, 1, 1, ACC_ALL): "1 x 1 accumulate ops use slots 0 and 1: they take the narrow kernel",
    # at most 2 inputs and 3-4 outputs is the diff-update only; all its patterns share one
    # shape (2 inputs, the same outputs and modes), which always has an exact kernel
    (GENERIC, 2, 4, ACC_RUNTIME): "<= 2 inputs with 3-4 outputs is the diff-update, always an exact shape",
}


def unreachable_instantiations() -> set:
    return {(e, kind, nt, lt, acc, False) for e in (PERM, LDS) for (kind, nt, lt, acc) in UNREACHABLE}


# ------------------------------------------------------------------ plans
def plan_a():
    """Two full tiles on 4 KiB (so 128-byte) offsets: the automatic rule splits every tile
    over four 64-lane workgroups (split_shift 2)."""
    return [(TILE, TILE), (3 * TILE, TILE)]


def plan_b():
    """Ragged and misaligned extents: lengths 1, 15, 16, 17, 4095, 4097 at 16-byte-aligned
    offsets (4097 crosses a 4 KiB boundary: two tiles), 33 and 4098 at offsets 1 and 7 past
    one (the byte gather / scatter path).  One 256-lane workgroup per tile (split_shift 0)."""
    ext = [(16, 1), (48, 15), (80, 16), (112, 17), (160, 4095), (4272, 4097), (8385, 33), (8439, 4098)]
    assert all(o % 16 == 0 for o, _ in ext[:6]) and ext[6][0] % 16 == 1 and ext[7][0] % 16 == 7
    return ext


def plan_c():
    """A short mixed plan for the capacity kernels: full tiles, a ragged and a misaligned one."""
    return [(0, TILE), (TILE + 16, 100), (2 * TILE + 7, 33), (3 * TILE, TILE), (4 * TILE + 32, 4097)]


PLANS = {"A": (plan_a, 2), "B": (plan_b, 0), "C": (plan_c, 0)}


def extents(which: str, n_patterns: int):
    """(off, src_off, len, pattern) with the patterns dealt round-robin."""
    ext = PLANS[which][0]()
    assert all(a[0] + a[1] <= b[0] for a, b in zip(ext, ext[1:])) and ext[-1][0] + ext[-1][1] <= ARENA
    return [(o, o + SRC_SHIFT, n, e % n_patterns) for e, (o, n) in enumerate(ext)]


# ------------------------------------------------------------------ the harness
class Case:
    """torch, ec and what this process's environment makes of every launch."""

    def __init__(self, torch, ec, expect_wt: bool = True, expect_split: int | None = None):
        self.torch, self.ec = torch, ec
        self.expect_wt = expect_wt        # the write-through bit of these small launches
        self.expect_split = expect_split  # a pinned CEC_SPLIT_SHIFT, or None: the automatic rule

    def split(self, auto: int) -> int:
        return auto if self.expect_split is None else self.expect_split

    def dev(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).cuda()
        assert t.data_ptr() % 128 == 0
        return t

    def check_record(self, rec, seq0, *, launches=1, kind, nt, lt, acc, engine, split=None, what=""):
        ctx = (what, rec)
        assert rec["seq"] == seq0 + launches, ctx
        assert (rec["kind"], rec["nt"], rec["lt"], rec["acc"]) == (kind, nt, lt, acc), ctx
        assert rec["engine"] == engine and self.ec.last_engine() == engine, ctx
        if split is not None:
            assert rec["split_shift"] == split, ctx
            assert rec["grid"] == rec["n_tiles"] << split, ctx
        assert bool(rec["flags"] & WRITE_THROUGH) == self.expect_wt, ctx
        if engine == PERM:
            assert rec["lds_bytes"] == 0, ctx


def reference(host0: np.ndarray, ext, patterns) -> np.ndarray:
    """The slab after one op: per extent, every output of its pattern from the bytes the
    slab held BEFORE the op (inputs are read before any output of the launch is written)."""
    exp = host0.copy()
    for off, src, n, pi in ext:
        ins, outs = patterns[pi]
        xs = [host0[r, (src if s else off):(src if s else off) + n] for r, s in ins]
        for r, s, xor, coefs in outs:
            o = src if s else off
            v = combine(coefs, xs)
            if xor:
                v ^= host0[r, o:o + n]
            exp[r, o:o + n] = v
    return exp


def init_slab(rng, n_rows, ext, patterns) -> np.ndarray:
    """Inputs: random everywhere.  Rows that are only written: the sentinel everywhere.
    Accumulate outputs: the sentinel, with random prior contents inside the extents."""
    host = np.full((n_rows, ROW), SENT, np.uint8)
    in_rows = {r for ins, _ in patterns for r, _ in ins}
    for r in in_rows:
        host[r] = rng.integers(0, 256, ROW, dtype=np.uint8)
    for off, src, n, pi in ext:
        for r, s, xor, _ in patterns[pi][1]:
            if xor and r not in in_rows:
                o = src if s else off
                host[r, o:o + n] = rng.integers(0, 256, n, dtype=np.uint8)
    return host


def run_op(case: Case, rng, which: str, n_rows: int, patterns, call, **expect) -> dict:
    """One op over plan `which`: upload, call(rows, plan), assert the record, compare the
    whole slab (every output byte, and every byte no extent names) with the reference."""
    ec, torch = case.ec, case.torch
    ext = extents(which, len(patterns))
    host0 = init_slab(rng, n_rows, ext, patterns)
    slab = case.dev(host0)
    seq0 = ec.last_launch()["seq"]
    with ec.Plan(ext) as plan:
        call([slab[r] for r in range(n_rows)], plan)
        rec = ec.last_launch()
        torch.cuda.synchronize()
    case.check_record(rec, seq0, split=case.split(PLANS[which][1]), **expect)
    got = slab.cpu().numpy()
    exp = reference(host0, ext, patterns)
    if not np.array_equal(got, exp):
        r, p = np.argwhere(got != exp)[0]
        raise AssertionError(f"{expect.get('what')}: plan {which} row {r} byte {p}: "
                             f"got {got[r, p]:#x} want {exp[r, p]:#x} ({int((got != exp).sum())} wrong)")
    return rec


# ------------------------------------------------------------------ ops as patterns (cocytus_ec.h)
def matrix_of(k: int, rows) -> list:
    """A (k + m) x k coding matrix: identity on top (never read by these ops), then rows."""
    top = np.eye(k, dtype=np.int64)
    return [int(v) for v in np.vstack([top, np.asarray(rows, np.int64).reshape(-1, k)]).flatten()]


def encode_op(k, m, coef, skip=()):
    """cec_encode: parity[p] = sum_j MATRIX(k + p, j) * data[j]; a NULL parity is not produced.
    Rows 0..k-1 data, k..k+m-1 parity."""
    mat = matrix_of(k, coef)
    outs = [(k + p, 0, False, list(coef[p])) for p in range(m) if p not in skip]
    patterns = [([(j, 0) for j in range(k)], outs)]

    def call(ec, rows, plan):
        ec.encode(k, m, mat, rows[:k], [None if p in skip else rows[k + p] for p in range(m)], plan)

    return k + m, patterns, call


def diff_update_op(k, m, coef, install):
    """cec_diff_update: for source shard j = pattern, d = staging[src_off] ^ data[j][off];
    parity[p][off] ^= MATRIX(k + p, j) * d; install: data[j][off] = staging[src_off].
    Rows 0..k-1 data, k..k+m-1 parity, k+m staging."""
    mat = matrix_of(k, coef)
    patterns = []
    for j in range(k):
        outs = [(k + p, 0, True, [coef[p][j], coef[p][j]]) for p in range(m)]
        if install:
            outs.append((j, 0, False, [0, 1]))
        patterns.append(([(j, 0), (k + m, 1)], outs))

    def call(ec, rows, plan):
        ec.diff_update(k, m, mat, rows[:k], rows[k + m], rows[k:k + m], install, plan)

    return k + m + 1, patterns, call


def apply_diffs_op(k, coefrow):
    """cec_apply_diffs on parity lid k: parity[off] ^= MATRIX(k, j) * diffs[src_off],
    j = pattern.  Row 0 diffs, row 1 the parity."""
    mat = matrix_of(k, [coefrow])
    patterns = [([(0, 1)], [(1, 0, True, [coefrow[j]])]) for j in range(k)]

    def call(ec, rows, plan):
        ec.apply_diffs(k, 1, mat, k, rows[0], rows[1], plan)

    return 2, patterns, call


def coef_rows(rng, n, l, low=False):
    """l rows of n coefficients >= 2, all distinct.  n >= 3: every row also holds one 0 and
    one 1 (the kernel's skip and plain-XOR branches, in every instantiation).  `low` (the
    second set of the 1- and 2-input shapes, which have no room for both): one of them."""
    vals = iter(rng.permutation(np.arange(2, 256))[:n * l])
    rows = [[int(next(vals)) for _ in range(n)] for _ in range(l)]
    for r, row in enumerate(rows):
        if n >= 3:
            row[r % n] = 0
            row[(r + 1) % n] = 1
        elif low:
            row[r % n] = r % 2
    return rows


# ------------------------------------------------------------------ (a) every coefficient
STREAM_CONST = [0x00, 0x5B, 0xC6, 0x1F, 0xA9, 0x72, 0xE4, 0x3D]
NA = 1024


def stream_bytes(i: int) -> np.ndarray:
    """1024 bytes with every byte value at every byte lane of a dword."""
    p = np.arange(NA)
    s = (((p + p // 256) & 255) ^ STREAM_CONST[i]).astype(np.uint8)
    for lane in range(4):
        assert len(set(s[lane::4].tolist())) == 256
    return s


def check_every_coefficient(case: Case, engine: int) -> set:
    """All 256 coefficients through the narrow kernels (region multiply, write and XOR,
    device memory and -- the system-release variants -- the drop-in over pinned host
    memory) and through the exact 8 x 4 kernel (32 coefficients per launch), aligned and
    with one input and one output base a byte off (gather / scatter)."""
    ec, torch = case.ec, case.torch
    ec.set_engine(engine)
    reached = set()
    rng = np.random.default_rng(0xC0EF + engine)
    s = stream_bytes(1)
    src = case.dev(s)
    prior = rng.integers(0, 256, (258, NA), dtype=np.uint8)  # rows 0 and 257: guards
    for add in (0, 1):
        acc = ACC_ALL if add else ACC_NONE
        exp = prior.copy()
        for c in range(256):
            exp[1 + c] = MUL[c][s] ^ (prior[1 + c] if add else 0)
        # device memory
        dst = case.dev(prior)
        for c in range(256):
            seq0 = ec.last_launch()["seq"]
            ec.region_multiply(src, c, NA, dst[1 + c], add)
            rec = ec.last_launch()
            if add and c == 0:  # dst ^= 0 * src: documented as no launch at all
                assert rec["seq"] == seq0
                continue
            case.check_record(rec, seq0, kind=NARROW, nt=1, lt=1, acc=acc, engine=engine,
                              split=case.split(2), what=f"region c={c} add={add}")
            assert not rec["flags"] & SYS_RELEASE
            reached.add(inst(rec))
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert np.array_equal(got, exp), ("region_multiply", add, np.argwhere(got != exp)[:4])
        # the drop-in over pinned host memory: every wave ends with a system-scope release
        hsrc = torch.from_numpy(s.copy()).pin_memory()
        hdst = torch.from_numpy(prior.copy()).pin_memory()
        for c in range(256):
            seq0 = ec.last_launch()["seq"]
            ec.galois_w08_region_multiply(hsrc, c, NA, hdst[1 + c], add)
            rec = ec.last_launch()
            if add and c == 0:
                assert rec["seq"] == seq0
                continue
            case.check_record(rec, seq0, kind=NARROW, nt=1, lt=1, acc=acc, engine=engine,
                              what=f"drop-in c={c} add={add}")
            assert rec["flags"] & SYS_RELEASE and ec.last_sync()["waves_released"] == 1, rec
            reached.add(inst(rec))
        got = hdst.numpy()
        assert np.array_equal(got, exp), ("drop-in", add, np.argwhere(got != exp)[:4])

    # exact 8 x 4: coefficients 32g .. 32g + 31 in launch g
    ins = [stream_bytes(i) for i in range(8)]
    stride = NA + 128
    for shifted in (False, True):
        din = np.full((8, stride), SENT, np.uint8)
        ioff = [1 if shifted and i == 3 else 0 for i in range(8)]
        ooff = [1 if shifted and l == 2 else 0 for l in range(4)]
        for i in range(8):
            din[i, ioff[i]:ioff[i] + NA] = ins[i]
        data = case.dev(din)
        parity = case.dev(np.full((4, stride), SENT, np.uint8))
        full_rows = 0
        for g in range(8):
            coef = np.arange(32 * g, 32 * g + 32).reshape(4, 8)
            seq0 = ec.last_launch()["seq"]
            ec.encode_region(8, 4, matrix_of(8, coef), [data[i][ioff[i]:] for i in range(8)],
                             [parity[l][ooff[l]:] for l in range(4)], NA)
            rec = ec.last_launch()
            torch.cuda.synchronize()
            case.check_record(rec, seq0, kind=EXACT, nt=8, lt=4, acc=ACC_NONE, engine=engine,
                              split=case.split(0 if shifted else 2), what=f"8x4 g={g} shifted={shifted}")
            reached.add(inst(rec))
            if engine == LDS:
                # one 256-byte product row per distinct coefficient >= 2: 32 rows are 512
                # 16-byte chunks for 256 (or 64) lanes, the one place where the kernel's
                # row-staging loop runs more than once per lane
                n_rows = int((coef >= 2).sum())
                assert rec["lds_bytes"] >= n_rows * 256, rec
                full_rows += n_rows == 32 and rec["lds_bytes"] >= 32 * 256
            got = parity.cpu().numpy()
            for l in range(4):
                want = np.full(stride, SENT, np.uint8)
                want[ooff[l]:ooff[l] + NA] = combine(coef[l], ins)
                assert np.array_equal(got[l], want), (f"8x4 g={g} shifted={shifted} out {l}",
                                                      np.argwhere(got[l] != want)[:4])
        if engine == LDS:
            assert full_rows == 7  # every launch but the one that holds coefficients 0 and 1
    return reached


# ------------------------------------------------------------------ (b) every exact shape
def check_exact_shapes(case: Case, engine: int) -> set:
    """Every shape launch_exact compiles, over plan A (full aligned tiles, four workgroups
    per tile) and plan B (ragged and misaligned tiles, one workgroup per tile)."""
    ec = case.ec
    ec.set_engine(engine)
    reached = set()
    rng = np.random.default_rng(0xE8AC7 + engine)

    def run(which, op, **expect):
        n_rows, patterns, call = op
        rec = run_op(case, rng, which, n_rows, patterns, lambda rows, plan: call(ec, rows, plan),
                     engine=engine, **expect)
        reached.add(inst(rec))

    for which in ("A", "B"):
        # write shapes: encode(k = n, m = l)
        for n in range(1, 9):
            for l in range(1, 5):
                # a 1 x 1 launch over slots 0 and 1 takes the narrow kernel
                kind = NARROW if (n, l) == (1, 1) else EXACT
                for low in ((False, True) if n < 3 else (False,)):
                    run(which, encode_op(n, l, coef_rows(rng, n, l, low)), kind=kind, nt=n, lt=l,
                        acc=ACC_NONE, what=f"encode {n}x{l} low={low}")
        # ... and the 48-slot 1 x 1 write kernel: one input, the second parity only (slot 2)
        for low in (False, True):
            run(which, encode_op(1, 2, coef_rows(rng, 1, 2, low), skip=(0,)), kind=EXACT, nt=1, lt=1,
                acc=ACC_NONE, what=f"encode 1x2 without parity 0 low={low}")
        # read-modify-write shapes.  With the LDS engine, plan A's accumulate launches of
        # the 2-input shapes below are the kEarlyRows path of combine_kernel (full aligned
        # tiles: product rows staged before the stream loads); split_shift == 2, asserted in
        # run_op, is what says every tile was full and on a line, so that path ran.  Plan B
        # runs the same kernels through the general path.
        for low in (False, True):
            (row,) = coef_rows(rng, 2, 1, low)
            run(which, apply_diffs_op(2, row), kind=NARROW, nt=1, lt=1, acc=ACC_ALL,
                what=f"apply_diffs low={low}")
        for l in range(1, 5):
            for low in (False, True):
                run(which, diff_update_op(2, l, coef_rows(rng, 2, l, low), False), kind=EXACT, nt=2, lt=l,
                    acc=ACC_ALL, what=f"diff_update m={l} low={low}")
        for l in range(2, 5):
            for low in (False, True):
                run(which, diff_update_op(2, l - 1, coef_rows(rng, 2, l - 1, low), True), kind=EXACT, nt=2,
                    lt=l, acc=ACC_ABL, what=f"diff_update + install m={l - 1} low={low}")
    return reached


# ------------------------------------------------------------------ (c) the capacity kernels
def loss_mask(k, lost):
    """A recovery mask: the surviving data lids and as many parities as shards are lost."""
    mask = sum(1 << j for j in range(k) if j not in lost)
    return mask | sum(1 << (k + r) for r in range(len(lost)))


def check_decode_mixed(case: Case, rng, engine, k, m, losses, nt, lt) -> dict:
    """cec_decode with masks of differing loss counts in one plan: the patterns differ in
    their output counts, so the launch takes a capacity kernel.  The rebuilt bytes must be
    the data the parity was computed from (with the reference table)."""
    ec, torch = case.ec, case.torch
    mat = ec.coding_matrix(k, m)
    lost_sets = [tuple(range(q, q + n)) for q, n in enumerate(losses)]  # loss counts as given
    masks = [loss_mask(k, ls) for ls in lost_sets]
    ext = extents("C", len(masks))
    data = rng.integers(0, 256, (k, ROW), dtype=np.uint8)
    host0 = np.full((2 * k + m, ROW), SENT, np.uint8)
    host0[:k] = data
    for p in range(m):
        host0[k + p] = combine(mat[(k + p) * k:(k + p + 1) * k], list(data))
    exp = host0.copy()
    for off, _, n, pi in ext:
        for j in lost_sets[pi]:
            exp[k + m + j, off:off + n] = data[j, off:off + n]
            host0[j, off:off + n] ^= 0xFF  # a lost shard's bytes must not be read
            exp[j, off:off + n] = host0[j, off:off + n]
        for p in range(len(lost_sets[pi]), m):  # nor a parity the mask does not name
            host0[k + p, off:off + n] ^= 0xFF
            exp[k + p, off:off + n] = host0[k + p, off:off + n]
    slab = case.dev(host0)
    seq0 = ec.last_launch()["seq"]
    with ec.Plan(ext) as plan:
        ec.decode(k, m, mat, masks, [slab[r] for r in range(k + m)], [slab[k + m + j] for j in range(k)], plan)
        rec = ec.last_launch()
        torch.cuda.synchronize()
    case.check_record(rec, seq0, kind=GENERIC, nt=nt, lt=lt, acc=ACC_RUNTIME, engine=engine,
                      split=case.split(0), what=f"decode k={k} m={m} losses={losses}")
    got = slab.cpu().numpy()
    assert np.array_equal(got, exp), (k, m, losses, np.argwhere(got != exp)[:4])
    return rec


def check_pool_flush(case: Case, rng, engine, k, peers, nt) -> dict:
    """cec_recovery_pool_flush of two requests with differing numbers of queued replies:
    patterns of 1 + peers inputs each and one output, so a capacity kernel of one output."""
    ec = case.ec
    m, lid_self = 2, k + 1
    coef = coef_rows(rng, k, m)
    mat = matrix_of(k, coef)
    mask = loss_mask(k, (0,)) & ~(1 << k) | (1 << lid_self)  # D0 lost, led by this parity
    par = rng.integers(0, 256, 2 * TILE, dtype=np.uint8)
    dpar = case.dev(par)
    seq0 = ec.last_launch()["seq"]
    with ec.RecoveryPool(k, m, mat, lid_self, dpar, capacity_units=2) as pool:
        want = []
        for u, n_peers in enumerate(peers):
            rid = pool.begin(mask, u, u)
            r = par[u * TILE:(u + 1) * TILE].copy()
            for j in range(1, 1 + n_peers):
                units = rng.integers(0, 256, TILE, dtype=np.uint8)
                pool.add_peer(rid, j, units)
                r ^= MUL[coef[1][j]][units]
            want.append((rid, r))
        assert pool.flush() == 2
        rec = ec.last_launch()
        case.check_record(rec, seq0, kind=GENERIC, nt=nt, lt=1, acc=ACC_RUNTIME, engine=engine,
                          what=f"pool flush k={k} peers={peers}")
        for rid, r in want:
            got = np.empty(TILE, np.uint8)
            pool.residual(rid, got)
            assert np.array_equal(got, r), (k, peers, rid)
    return rec


def check_pool_flush_solve(case: Case, rng, engine) -> dict:
    """cec_recovery_pool_flush_solve, k = 2: one request solved in the pass (2 inputs, 2
    outputs), one whose lost lid has no output arena (2 inputs, 1 output): capacity 2 x 2."""
    ec, torch = case.ec, case.torch
    k, m, lid_self = 2, 2, 3
    coef = [[int(v) for v in rng.permutation(np.arange(2, 256))[:2]] for _ in range(m)]
    mat = matrix_of(k, coef)
    c = coef[1]
    par = rng.integers(0, 256, 2 * TILE, dtype=np.uint8)
    dpar = case.dev(par)
    out0 = case.dev(np.full(2 * TILE, SENT, np.uint8))
    d1 = rng.integers(0, 256, TILE, dtype=np.uint8)
    d0 = rng.integers(0, 256, TILE, dtype=np.uint8)
    seq0 = ec.last_launch()["seq"]
    with ec.RecoveryPool(k, m, mat, lid_self, dpar, capacity_units=2) as pool:
        ra = pool.begin((1 << 1) | (1 << lid_self), 0, 0)  # D0 lost: D1 replies
        rb = pool.begin((1 << 0) | (1 << lid_self), 1, 1)  # D1 lost: D0 replies, no arena for D1
        pool.add_peer(ra, 1, d1)
        pool.add_peer(rb, 0, d0)
        assert pool.flush_solve([out0, None]) == 1
        rec = ec.last_launch()
        case.check_record(rec, seq0, kind=GENERIC, nt=2, lt=2, acc=ACC_RUNTIME, engine=engine,
                          what="pool flush_solve k=2")
        assert pool.solved(ra) and not pool.solved(rb)
        res_a = par[:TILE] ^ MUL[c[1]][d1]
        res_b = par[TILE:] ^ MUL[c[0]][d0]
        for rid, want in ((ra, res_a), (rb, res_b)):
            got = np.empty(TILE, np.uint8)
            pool.residual(rid, got)
            assert np.array_equal(got, want), rid
        torch.cuda.synchronize()
        want0 = np.full(2 * TILE, SENT, np.uint8)
        want0[:TILE] = MUL[gf_inv(c[0])][res_a]
        assert np.array_equal(out0.cpu().numpy(), want0)
    return rec


def check_host_batch_mixed(case: Case, rng, engine) -> dict:
    """cec_region_multiply_batch with a first-touch job (dst = base ^ c * src: 2 inputs)
    and a plain XOR job (1 input) in one wave: capacity 2 x 1."""
    ec = case.ec
    src = rng.integers(0, 256, (2, TILE), dtype=np.uint8)
    base = rng.integers(0, 256, 1000, dtype=np.uint8)
    dst = rng.integers(0, 256, (2, TILE + 64), dtype=np.uint8)
    want = dst.copy()
    want[0, 3:1003] = base ^ MUL[0x8E][src[0, :1000]]
    want[1, 16:16 + TILE] ^= MUL[0x02][src[1]]
    seq0 = ec.last_launch()["seq"]
    launches, _ = ec.region_multiply_batch([(src[0], dst[0, 3:], base, 1000, 0x8E, 1),
                                            (src[1], dst[1, 16:], None, TILE, 0x02, 1)])
    rec = ec.last_launch()
    assert launches == 1
    case.check_record(rec, seq0, kind=GENERIC, nt=2, lt=1, acc=ACC_RUNTIME, engine=engine, what="host batch")
    assert np.array_equal(dst, want)
    return rec


def check_capacity_kernels(case: Case, engine: int) -> set:
    """A public call for every capacity kernel that has one; returns the instantiations
    reached (the test asserts them against the 12 compiled, less UNREACHABLE)."""
    ec = case.ec
    ec.set_engine(engine)
    reached = set()
    rng = np.random.default_rng(0xCA9 + engine)
    # 9..16 inputs: encodes (one pattern, no exact kernel above 8 inputs)
    for k, m, lt in ((9, 1, 1), (12, 2, 2), (10, 3, 4), (16, 4, 4)):
        n_rows, patterns, call = encode_op(k, m, coef_rows(rng, k, m))
        rec = run_op(case, rng, "C", n_rows, patterns, lambda rows, plan: call(ec, rows, plan), kind=GENERIC,
                     nt=16, lt=lt, acc=ACC_RUNTIME, engine=engine, what=f"encode {k}x{m}")
        reached.add(inst(rec))
    # masks of differing loss counts in one plan
    for k, m, losses, nt, lt in ((3, 2, (1, 2), 4, 2), (4, 3, (1, 3), 4, 4), (6, 3, (1, 2), 8, 2),
                                 (7, 4, (1, 2, 4), 8, 4)):
        reached.add(inst(check_decode_mixed(case, rng, engine, k, m, losses, nt, lt)))
    # one output, differing input counts: the pool's flush; mixed 1- and 2-input jobs
    reached.add(inst(check_pool_flush(case, rng, engine, 4, (1, 3), 4)))
    reached.add(inst(check_pool_flush(case, rng, engine, 8, (4, 7), 8)))
    reached.add(inst(check_pool_flush_solve(case, rng, engine)))
    reached.add(inst(check_host_batch_mixed(case, rng, engine)))
    return reached


def check_five_outputs(case: Case, engine: int) -> set:
    """cec_diff_update with m = 4 and install: 5 outputs, split 4 + 1 over two launches.
    The install (the second launch) overwrites the data shard the first launch read, so it
    must run after it: the shard ends as the new value and all four parities hold the
    update computed from the OLD bytes (the reference computes everything from them)."""
    ec = case.ec
    ec.set_engine(engine)
    rng = np.random.default_rng(0x5007 + engine)
    reached = set()
    for which in ("A", "B"):
        n_rows, patterns, call = diff_update_op(3, 4, coef_rows(rng, 3, 4), True)
        rec = run_op(case, rng, which, n_rows, patterns, lambda rows, plan: call(ec, rows, plan), launches=2,
                     kind=EXACT, nt=2, lt=1, acc=ACC_NONE, engine=engine, what="diff_update m=4 + install")
        reached.add(inst(rec))
    return reached


# ------------------------------------------------------------------ (d) limits
def check_residual_limits(case: Case, engine: int) -> set:
    """cec_residual at k = 16: all 16 data lids in the mask would be 17 inputs with the
    parity -- refused, nothing launched, the residual untouched; a recovery mask (15 data
    lids and the parity: 16 inputs) computes the residual."""
    ec, torch = case.ec, case.torch
    ec.set_engine(engine)
    rng = np.random.default_rng(0x11417 + engine)
    k, m, lid_self = 16, 4, 16
    coef = coef_rows(rng, k, m)
    mat = matrix_of(k, coef)
    ext = extents("C", 1)
    host0 = np.full((k + m + 1, ROW), SENT, np.uint8)
    host0[:k + m] = rng.integers(0, 256, (k + m, ROW), dtype=np.uint8)
    slab = case.dev(host0)
    rows = [slab[r] for r in range(k + m + 1)]
    seq0 = ec.last_launch()["seq"]
    with ec.Plan(ext) as plan:
        try:
            ec.residual(k, m, mat, lid_self, 0xFFFF, rows[:k + m], rows[k + m], plan)
        except ec.CecError as e:
            assert e.code == ec.CEC_EINVAL, e
        else:
            raise AssertionError("cec_residual took 17 inputs")
        assert ec.last_launch()["seq"] == seq0
        torch.cuda.synchronize()
        assert np.array_equal(slab.cpu().numpy(), host0)
        mask = (0xFFFF & ~1) | (1 << lid_self)
        ec.residual(k, m, mat, lid_self, mask, rows[:k + m], rows[k + m], plan)
        rec = ec.last_launch()
        torch.cuda.synchronize()
    case.check_record(rec, seq0, kind=GENERIC, nt=16, lt=1, acc=ACC_RUNTIME, engine=engine,
                      split=case.split(0), what="residual of 16 inputs")
    ins = [(lid_self, 0)] + [(s, 0) for s in range(1, k)]
    exp = reference(host0, ext, [(ins, [(k + m, 0, False, [1] + coef[0][1:])])])
    assert np.array_equal(slab.cpu().numpy(), exp)
    return {inst(rec)}


# ------------------------------------------------------------------ child entry
def main(argv) -> None:
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--expect-wt", type=int, default=1)
    ap.add_argument("--expect-split", type=int, default=None)
    args = ap.parse_args(argv)
    import torch

    torch.cuda.set_device(0)
    torch.empty(1, device="cuda")
    from cocytus_amd import ec

    assert ec.device_check() == ec.CEC_OK, ec.lib().cec_last_error()
    case = Case(torch, ec, expect_wt=bool(args.expect_wt), expect_split=args.expect_split)
    n = 0
    for engine in (PERM, LDS):
        n += len(check_exact_shapes(case, engine))
    print(f"{n} instantiations")
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
