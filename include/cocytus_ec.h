/*
 * cocytus_ec.h -- batched, device-resident erasure-coding API of libcocytus_ec.so
 * (MI355X / gfx950, hand-written HIP kernels; no MFMA, no Jerasure).
 *
 * This is the additive entry-point set SURVEY.md §8(b) asks for next to the three
 * drop-in Jerasure symbols (galois.h / jerasure.h / reed_sol.h).  Every call is
 * asynchronous on the given HIP stream (NULL = the default stream), takes device
 * pointers only, and returns a cec_status.  Nothing here falls back to the CPU:
 * a missing GPU is CEC_ENODEV.
 *
 * Layout contract (Cocytus): every data shard j and every parity p owns an arena
 * (ecmem, /root/reference/ecmem.h:29-58).  A value is the byte range
 * [off, off+len) of an arena; parity bytes sit at the SAME offset as the data
 * they encode (/root/reference/memcached.c:7704-7717), offsets are 16-B aligned
 * (/root/reference/ecalloc.c:176) and recovery works on 4 KiB units
 * (/root/reference/const.h:26).  Unaligned offsets and lengths are accepted
 * (slower byte path for the affected tiles), bit-exact either way.
 *
 * LIFETIME RULE (every object: plan, drainer, recovery session, recovery pool, scrub report):
 * destroy the object BEFORE any stream it was used on.  An object records the streams
 * its calls used and its destroy synchronises exactly those (never the whole device);
 * a handle of a destroyed stream cannot be synchronised (it crashes the HIP runtime).
 * This is a change from the first release, whose destroy waited for the whole device.
 * The recorded list grows with every distinct stream an object is used on.  A long-lived
 * object used on short-lived streams (one per client connection) calls its
 * *_release_stream(obj, stream) before destroying such a stream: that waits for the
 * object's work on it and drops it from the list, which then stays bounded by the
 * streams alive (and the object's destroy no longer touches the dead handle).
 *
 * THREADS: every entry point may be called from any thread.  The library's shared
 * state (caches, the engine and occupancy settings) is thread-safe, and each op reads
 * the process-wide engine once, so a concurrent cec_set_engine changes later ops only.
 * A plan is immutable once created and may be used by several threads' ops at once.
 * Drainers, recovery sessions and recovery pools carry per-object state: calls on one
 * such object must not overlap (one thread at a time, as Cocytus' single worker thread
 * per process makes them).
 *
 * Coding matrix: int[(k+m)*k], row-major, MATRIX(x,y) = matrix[x*k+y]
 * (/root/reference/memcached.h:52), as returned by
 * reed_sol_big_vandermonde_distribution_matrix(k+m, k, 8)
 * (/root/reference/memcached.c:6845).  Limits: 1 <= k <= CEC_MAX_K,
 * 1 <= m <= CEC_MAX_M, k+m <= 32 (Cocytus masks are uint32_t).
 */
#ifndef COCYTUS_EC_H
#define COCYTUS_EC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CEC_MAX_K 16
#define CEC_MAX_M 8
#define CEC_UNIT_SIZE 4096 /* UNITSIZE, /root/reference/const.h:26; also the kernel tile */

typedef enum cec_status {
    CEC_OK = 0,
    CEC_EINVAL = -1,      /* bad argument (k/m/lid/mask/pointer/pattern index) */
    CEC_ESINGULAR = -2,   /* decode submatrix not invertible (memcached.c:7908 asserts) */
    CEC_EHIP = -3,        /* a HIP runtime call failed; see cec_last_error() */
    CEC_ENOMEM = -4,      /* device or pinned-host allocation failed */
    CEC_EOVERLAP = -5,    /* read-modify-write op on a plan whose extents overlap */
    CEC_ENODEV = -6,      /* no usable gfx950 device: there is no CPU fallback */
    CEC_EFULL = -7        /* a recovery pool has no room for the request */
} cec_status;

/* One value of a batch.  `off` addresses the arenas (item->addr, memcached.h:441);
 * `src_off` addresses the staging buffer that carries values from / to the network
 * (c->vbuf, e->vbuf: memcached.c:3646-3655, 7727-7735); `pattern` is per-op:
 *   cec_diff_update / cec_apply_diffs /
 *   cec_set_diff                       : source data shard lid j (0..k-1)
 *   cec_decode                         : index into the op's mask array
 *   other ops (encode, residual, solve): 0.
 * An index out of range (j >= k, >= n_masks, or not 0) makes the op return
 * CEC_EINVAL before anything is launched. */
typedef struct cec_extent {
    uint64_t off;
    uint64_t src_off;
    uint32_t len;
    uint32_t pattern;
} cec_extent;

/* A device-resident batch: the extents plus the 4 KiB tile work-list the kernels
 * walk (load balance across mixed 256 B .. 1 MiB values).  Build once per batch. */
typedef struct cec_plan cec_plan;

/* GF(2^8) engine used by the kernels.  Both are bit-exact and within a few % of each
 * other.  PERM looks up three 8-entry byte tables per coefficient with v_perm_b32
 * (pure VALU, no LDS); LDS stages one 256-entry product row per coefficient,
 * exp[log x + log c] built from the log / antilog tables, in LDS (one ds_read_u8 per
 * byte).  AUTO (default) runs the LDS engine only where it led PERM by more than 2 % on
 * the median of the recorded boxes: cec_decode of values of 64 KiB and
 * more (the plan's mean extent), with one mask or many.  Every other op runs PERM:
 * encodes (any size), decodes of smaller values, the diff-update, residual, solve, set
 * diff, apply, region multiply and the recovery sessions and pool. */
typedef enum cec_engine { CEC_ENGINE_PERM = 0, CEC_ENGINE_LDS = 1, CEC_ENGINE_AUTO = 2 } cec_engine;

/* ---- runtime ---- */
const char *cec_version(void);
const char *cec_last_error(void);               /* thread-local message of the last failure */
int cec_device_check(void);                     /* CEC_OK if the current device is gfx950 */
int cec_set_engine(cec_engine e);               /* process-wide; default CEC_ENGINE_AUTO */
cec_engine cec_get_engine(void);
/* The engine (CEC_ENGINE_PERM or CEC_ENGINE_LDS) the calling thread's last op chose
 * (AUTO resolved), -1 before its first op.  Diagnostics: which kernel family ran. */
int cec_last_engine(void);
/* Occupancy of the streaming kernels: at most waves_per_cu waves of one launch per CU
 * (0 = as many as fit).  Process-wide; the initial value comes from the
 * CEC_WAVES_PER_CU environment variable.  A tuning knob: every value is bit-exact. */
int cec_set_waves_per_cu(int waves_per_cu);
int cec_get_waves_per_cu(void);

/* ---- arena layout in HBM ----
 * The kernels stream every arena at the same offset at once.  Arenas carved from one
 * allocation at a stride that is an ODD number of 4 KiB pages keep those concurrent
 * streams off the same HBM channel / bank group; even strides (and separate hipMallocs,
 * by chance) collide: measured 0.386-0.395 ms vs 0.418-0.426 ms per RS(3,2) 4 KiB
 * encode + decode step.  Use these for ecmem-style arenas. */
size_t cec_arena_stride(size_t bytes);             /* smallest odd multiple of 4 KiB >= bytes */
/* count arenas of `bytes` each in one device allocation; arenas[i] = base + i * stride.
 * *slab receives the allocation (pass it to cec_arenas_free). */
int cec_arenas_alloc(int count, size_t bytes, uint8_t **arenas, void **slab);
int cec_arenas_free(void *slab);

/* ---- plans ---- */
/* extents: HOST array of n cec_extent (n >= 0).  The tile list is built on the host
 * and copied to the device on `stream`; the plan is usable by later calls on any
 * stream ordered after it.  Overlapping [off, off+len) ranges are recorded: RMW ops
 * (cec_diff_update, cec_apply_diffs) refuse such a plan with CEC_EOVERLAP. */
int cec_plan_create(cec_plan **out, const cec_extent *extents, int n, void *stream);
/* Waits for the streams the plan was used on (its upload and launches), never for the
 * device or other streams.  LIFETIME RULE (top of this header): destroy plans (and
 * sessions, drainers, pools) before the streams they were used on.  A plan used inside
 * a captured graph must outlive the graph's replays. */
int cec_plan_destroy(cec_plan *plan);
/* Before destroying `stream`: wait for this plan's work on it and stop tracking it
 * (LIFETIME RULE above).  Not used on it: no-op.  cec_plan_tracked_streams: how many
 * streams the plan's destroy would synchronise now. */
int cec_plan_release_stream(cec_plan *plan, void *stream);
int cec_plan_tracked_streams(const cec_plan *plan);
int cec_plan_num_extents(const cec_plan *plan);
int64_t cec_plan_num_tiles(const cec_plan *plan);
uint64_t cec_plan_total_bytes(const cec_plan *plan); /* sum of extent lengths */

/* ---- ops (all async on `stream`) ---- */

/* Device form of galois_w08_region_multiply:
 * add != 0: dst[i] ^= c*src[i]; add == 0: dst[i] = c*src[i]; dst == NULL: in place. */
int cec_region_multiply(const void *src, int multby, size_t nbytes, void *dst, int add,
                        void *stream);

/* Full-stripe encode over arena extents (a5): parity[p][off..] = sum_j
 * MATRIX(k+p, j) * data[j][off..].  data: k device arena bases, parity: m. */
int cec_encode(int k, int m, const int *matrix, const uint8_t *const *data,
               uint8_t *const *parity, const cec_plan *plan, void *stream);

/* Encode one contiguous range [0, len) of every arena (no plan needed). */
int cec_encode_region(int k, int m, const int *matrix, const uint8_t *const *data,
                      uint8_t *const *parity, size_t len, void *stream);

/* Fused per-SET diff-update (a4 = a2 + M x a3): for each extent with source shard
 * j = pattern: d = staging[src_off..] ^ data[j][off..]; parity[p][off..] ^=
 * MATRIX(k+p, j) * d for every p with parity[p] != NULL (a lost parity is
 * skipped, memcached.c:2692-2694); if install, data[j][off..] = new value
 * (memcached.c:5666).  Extents must not overlap (CEC_EOVERLAP).  Live unit digests of
 * the arenas are not kept by this op: cec_diff_update_digests (LIVE DIGESTS) keeps them. */
int cec_diff_update(int k, int m, const int *matrix, uint8_t *const *data,
                    const uint8_t *staging, uint8_t *const *parity, int install,
                    const cec_plan *plan, void *stream);

/* Data-side diff only (memcached.c:2673-2681): diff[src_off..] = staging[src_off..]
 * ^ data[pattern][off..].  diff and staging share src_off addressing. */
int cec_set_diff(int k, const uint8_t *const *data, const uint8_t *staging, uint8_t *diff,
                 const cec_plan *plan, void *stream);

/* Parity-side deferred apply of shipped diffs (memcached.c:7762-7767, the drain
 * loops at :4231, :4322, :4350, :8068): parity[off..] ^= MATRIX(lid_self, j) *
 * diffs[src_off..] with j = pattern.  Extents must not overlap (CEC_EOVERLAP). */
int cec_apply_diffs(int k, int m, const int *matrix, int lid_self, const uint8_t *diffs,
                    uint8_t *parity, const cec_plan *plan, void *stream);

/* Recovery residual on parity lid_self (recovery.c:61-96): residual[off..] =
 * arenas[lid_self][off..] ^ sum_{data lid s in mask, s != lid_self}
 * MATRIX(lid_self, s) * arenas[s][off..].  arenas: k+m bases indexed by lid (only
 * the ones the mask names are read).  Every data lid < k in the mask is one input and
 * the parity itself is one more; a kernel combines at most 16 inputs, so a mask that
 * names 16 data lids (k = 16 with all of them: never a recovery mask, which holds
 * lid_self among its k lids) is refused with CEC_EINVAL and nothing is launched. */
int cec_residual(int k, int m, const int *matrix, int lid_self, uint32_t mask,
                 const uint8_t *const *arenas, uint8_t *residual, const cec_plan *plan,
                 void *stream);

/* Leader solve (memcached.c:7842-7922): with n lost data lids (not in mask) and the
 * n parities in mask, out[lost_i][off..] = sum_r inv[i][r] * residuals[par_r][off..].
 * residuals: k+m bases indexed by parity lid; out: k bases indexed by data lid. */
int cec_solve(int k, int m, const int *matrix, uint32_t mask,
              const uint8_t *const *residuals, uint8_t *const *out, const cec_plan *plan,
              void *stream);

/* Fused online recovery (residual + solve in one pass, bit-exact because GF(2^8)
 * arithmetic is exact): for each extent, mask = masks[pattern]; every data lid not
 * in the mask is rebuilt into out[lid][off..] from the k participants' arenas.
 * masks follow start_recovery (memcached.c:8136-8151): exactly k lids. */
int cec_decode(int k, int m, const int *matrix, const uint32_t *masks, int n_masks,
               const uint8_t *const *arenas, uint8_t *const *out, const cec_plan *plan,
               void *stream);

/* Mask helper identical to start_recovery (memcached.c:8136-8151).  connected:
 * k+m ints.  Returns 0 if fewer than k lids are available. */
uint32_t cec_recovery_mask(int k, int m, int leader_lid, const int *connected);

/* ---- server-side batching: the parity's deferred-commit drain ----
 * Replaces the drain loops `while (done_xid < stable_xid) process_rep_command(...)`
 * (memcached.c:4231, 4322, 4350, 8068) with one call per batch of pending diffs. */
typedef struct cec_host_update {   /* one pending rep_queue_item (rep_queue.h:28-39) */
    const void *buf;               /* e->vbuf: the shipped diff, host memory (any kind; inside
                                    * cec_drainer_staging or not, in any mix within one batch) */
    uint64_t addr;                 /* e->addr: arena offset (replayed ecalloc address) */
    uint32_t len;                  /* it->nbytes */
    uint32_t src_lid;              /* data shard lid the diff came from (0..k-1) */
} cec_host_update;

typedef struct cec_drainer cec_drainer;

/* A drainer for parity lid_self owns pinned + device staging of staging_bytes (diffs
 * larger than that are applied in several rounds) and a reusable tile list. */
int cec_drainer_create(cec_drainer **out, int k, int m, const int *matrix, int lid_self,
                       size_t staging_bytes);
int cec_drainer_destroy(cec_drainer *d);
int cec_drainer_release_stream(cec_drainer *d, void *stream);   /* LIFETIME RULE, top */

/* parity[addr..] ^= MATRIX(lid_self, src_lid) * buf for every update, as the sequential
 * loop of memcached.c:7762-7767 would leave it (XOR accumulation commutes; updates
 * whose ranges overlap are put in separate launches, never raced).  Synchronous: on a
 * CEC_OK return every update is applied and the host buffers may be reused / acked.
 * On CEC_EHIP the launches of earlier overlap waves or rounds may already be applied and
 * the later ones not, and a retry would apply the earlier ones twice: the parity arena is
 * then inconsistent in some 4 KiB units of the window's ranges.  Where every arena of the
 * group is on this device, cec_scrub + cec_scrub_repair over those ranges find and rebuild
 * them (below); otherwise the process must stop -- or, with live digests (LIVE DIGESTS,
 * below), let cec_scrub_digests over the group's live arrays name the units a lost or
 * twice-applied diff left wrong.  Attached digests (cec_drainer_set_digests) are then as
 * uncertain as the arena in the window's units: after units [u0, u0 + n) are rebuilt,
 * re-base them: cec_digest_region of `arena + 4096 * u0` into `digests + 32 * u0`, len 4096 * n. */
int cec_drainer_apply(cec_drainer *d, const cec_host_update *updates, int n,
                      uint8_t *parity, void *stream);

/* The checks cec_drainer_apply makes on its updates before it touches anything (src_lid
 * < k, buf non-NULL when len > 0, len <= half the staging area, and with digests attached
 * addr + len <= n_units * 4096), on the host only: CEC_OK
 * or CEC_EINVAL.  A caller with side effects per update (the server's recovery fold) runs
 * it first, so that an update the apply would refuse is refused before any of them. */
int cec_drainer_validate(const cec_drainer *d, const cec_host_update *updates, int n);

/* Launches the last cec_drainer_apply needed (>= 1 when n > 0: overlap waves x rounds,
 * plus one per round while digests are attached). */
int cec_drainer_last_launches(const cec_drainer *d);

/* Attach the parity's live digest array (LIVE DIGESTS, below: device memory, 32 B per 4 KiB
 * unit of the arena, n_units units, 16-byte aligned; the caller owns it and keeps it alive
 * while attached).  Every cec_drainer_apply then also folds each round's staged diffs into
 * it: one cec_digest_apply_diffs launch per round, behind the round's fold launches on the
 * same stream, over all the round's tiles at once.  digests == NULL detaches: every path
 * then does exactly what it does without this call.  CEC_EINVAL: a NULL drainer, a
 * misaligned array, n_units above 2^52. */
int cec_drainer_set_digests(cec_drainer *d, uint8_t *digests, uint64_t n_units);

/* The drainer's pinned staging area (2 x staging_bytes; *capacity receives its size).
 * A server can receive diffs straight into it (conn_nread of the "rep" payload,
 * memcached.c:7727-7735, into e->vbuf carved from this area).  When every update of a
 * cec_drainer_apply call points into it, the call skips the pack copy: one H2D of the
 * used span, then the fold.  A batch that mixes updates inside the area with updates
 * elsewhere is applied as well: the ones wholly inside it in place, the others (a buffer
 * that lies only partly in the area among them) from a copy in staging of the library's
 * own; above 1 MiB of diffs or 8192 tiles such a batch completes in several synchronous
 * steps, so a server that wants the pipelined pack path keeps a batch on one side.
 * The caller must not write the area during an apply, and the library never writes over
 * an update's source that lies in it: on return every such source holds what the caller
 * put there. */
uint8_t *cec_drainer_staging(cec_drainer *d, size_t *capacity);

/* ---- galois_w08_region_multiply, batched, over host memory ----
 * The unchanged server keeps its recovery state in host memory -- one malloc'd 4 KiB
 * buffer per recovery unit (recovery.c:79), the parity arena ecmem (recovery.c:81),
 * malloc'd peer replies and diffs, calloc'd solve outputs (memcached.c:7913) -- and calls
 * galois_w08_region_multiply once per unit (recovery.c:91, 123; memcached.c:7918).  This
 * runs a whole list of such calls as one staged pass (one kernel launch per overlap wave):
 *
 *   add = 0              : dst  = multby * src
 *   add = 1, base = NULL : dst ^= multby * src      (galois_w08_region_multiply(src, multby, len, dst, 1))
 *   add = 1, base != NULL: dst  = base ^ multby * src  (the first-touch copy of recovery.c:79-82,
 *                                                      then the fold of :91, fused)
 *
 * The bytes equal the calls run one by one in job order: jobs whose dst ranges overlap are
 * applied in separate launches (in job order when one of them writes; XOR accumulation
 * commutes).  A src or base range must not overlap any job's dst (CEC_EOVERLAP; base ==
 * dst is the in-place add).  Every pointer is HOST memory (pageable, pinned or registered;
 * device-resident state uses the device ops above).  Bases inside a region registered with
 * cec_host_register (the server's ecmem) are read in place through its device alias when
 * no two destinations of a staging round overlap: one copy less.  Synchronous: on return every dst
 * holds its bytes.  Lengths and alignments are arbitrary.  Staging is per calling thread:
 * mapped pinned memory, up to 2 x 24 MiB (more for one larger overlapping cluster), kept
 * for the thread's next call; batches above 4 MiB are pipelined over double-buffered
 * rounds.  A HIP failure (CEC_EHIP) may leave some destinations written and others not. */
typedef struct cec_region_job {
    const void *src;    /* region (read) */
    void *dst;          /* r2 (written) */
    const void *base;   /* see above; NULL for the plain call */
    uint32_t len;       /* nbytes */
    int32_t multby;     /* 0..255 */
    int32_t add;        /* 0 or 1 */
} cec_region_job;

int cec_region_multiply_batch(const cec_region_job *jobs, int n, void *stream);
/* Diagnostics of the calling thread's last batch: kernel launches (overlap waves x
 * rounds), staging rounds, and host wall time in microseconds spent planning (clusters,
 * waves, patterns), packing the inputs into the staging, in the GPU pass (launch to
 * completion) and unpacking the results. */
typedef struct cec_batch_stats {
    int launches, rounds;
    float plan_us, pack_us, gpu_us, unpack_us;
    int in_place_launches; /* launches that read their bases in place (cec_host_register'd) */
} cec_batch_stats;
int cec_region_multiply_batch_stats(cec_batch_stats *out);

/* ---- online recovery over 4 KiB unit ranges ----
 * One recovery request on a participating parity (recovery_queue_item,
 * recovery.h:57-69): units [unit_begin, unit_end] (UNITSIZE = 4 KiB, const.h:26) of
 * the arenas, participants `mask` (start_recovery, memcached.c:8136-8151).  The
 * residual lives in HBM.  Peer data, diffs and the other parities' residuals may be
 * host memory (pageable or pinned: staged through a pipelined pinned uploader) or
 * device memory (used in place).  All calls are synchronous: their results (device,
 * pinned or pageable) are complete on return and the caller may reuse its buffers.
 * destroy waits only for the streams the session's calls used; work the CALLER queued
 * on cec_recovery_residual(r) (e.g. shipping it with cec_copy on another stream) must
 * be complete before destroy, since the residual's memory is then reused.
 *
 * A MASK THAT NAMES NO DATA LID (k <= m: k parities rebuild all k shards).  No peer replies,
 * so such a request -- a session or a pool request -- is complete from the start and holds the
 * residual R = P[range] from the start: the live parity bytes (the first-touch copy of
 * recovery.c:79-82 with no fold behind it), with every update folded that the parity arena
 * has also received.  It is ready once the other n - 1 parities' residuals are given; for
 * n = 1, which is k = 1, at once.  The reference never completes such a request
 * (check_recovery_1st_completeness runs only when a reply arrives), so there is no behaviour
 * of its to match; the bytes are those of its own arithmetic over the parities.
 *   session: cec_recovery_create makes the copy, ONE launch on its stream, complete on
 *     return; cec_recovery_residual holds P's bytes from then on, cec_recovery_fold_update
 *     folds every later diff of any data lid, cec_recovery_solve rebuilds all k shards in
 *     ceil(k / 4) launches.  cec_recovery_finish takes a data peer of the mask: CEC_EINVAL.
 *   pool: cec_recovery_pool_begin queues the copy for the next flush of any kind, which makes
 *     it in its one launch (no launch of its own) and, if it solves and the request is ready,
 *     rebuilds the shards as for any request: in that launch up to three losses, by
 *     ceil(n / 4) behind it past three.  _solve, _solve_host, _residual and _fold_update(s)
 *     flush first, so an explicit solve or a _residual that finds the copy still queued is
 *     that one flush launch (shared by every queued request) ahead of its own work.  As for a
 *     queued reply, the copy reads the arena at the flush: call _fold_update(s) BEFORE the
 *     diff is applied to the parity arena. */
typedef struct cec_recovery cec_recovery;

int cec_recovery_create(cec_recovery **out, int k, int m, const int *matrix, int lid_self,
                        uint32_t mask, int unit_begin, int unit_end,
                        const uint8_t *parity_arena /* device: this parity's arena */,
                        void *stream);
int cec_recovery_destroy(cec_recovery *r);
int cec_recovery_release_stream(cec_recovery *r, void *stream); /* LIFETIME RULE, top */

/* recovery_recover_units (recovery.c:61-96): data peer peer_lid (in mask, not yet
 * applied) sent its raw bytes of the whole range (nbuf bytes).  The first peer also
 * copies the parity units in (first touch, recovery.c:79-82), fused into one pass. */
int cec_recovery_add_peer(cec_recovery *r, int peer_lid, const void *units, void *stream);

/* recovery_try_update_unit (recovery.c:99-131): a diff of len bytes at arena address
 * addr from data peer peer_lid reached this parity during recovery.  It is folded into
 * the residual where the range is touched and the peer has not contributed yet.
 * Returns the number of units folded (>= 0) or a negative cec_status. */
int cec_recovery_fold_update(cec_recovery *r, int peer_lid, uint64_t addr, const void *diff,
                             uint32_t len, void *stream);

/* check_recovery_1st_completeness (memcached.c:2522-2545): 1 when every data lid of
 * the mask has contributed, else 0. */
int cec_recovery_complete(const cec_recovery *r);

/* The residual (device memory, cec_recovery_bytes(r) bytes). */
const uint8_t *cec_recovery_residual(const cec_recovery *r);
uint64_t cec_recovery_bytes(const cec_recovery *r);

/* Leader (complete_recovery_bottom_half, memcached.c:7842-7922): C[j] = residual of
 * the j-th parity in the mask (this session's own for lid_self; peer_residuals[lid]
 * for the others, host or device); out[lost lid] (host or device, nbuf bytes each) =
 * sum_j inv[i][j] * C[j] for the n lost data lids. */
int cec_recovery_solve(cec_recovery *leader, const void *const *peer_residuals,
                       void *const *out, void *stream);

/* The last data peer and the leader solve (= cec_recovery_add_peer of that peer, then
 * cec_recovery_solve; same bytes, same residual afterwards).  With device or pinned
 * buffers it is ONE pass: the kernel reads the peer's bytes and writes the rebuilt
 * bytes (over PCIe in both directions at once for pinned host memory).  Pageable
 * buffers take the two-step path.  Any loss count n up to m: the pass is
 * ceil((n + 1) / 4) launches (the residual and the n rebuilt shards, four outputs a
 * launch; one launch up to three losses).  EINVAL if peer is not the last data peer. */
int cec_recovery_finish(cec_recovery *leader, int peer_lid, const void *units,
                        const void *const *peer_residuals, void *const *out, void *stream);

/* ---- background recovery of many small unit ranges ----
 * The idle recoverer issues one 4 KiB unit per request, up to TOO_MANY_RECOVERY = 85
 * in flight (idle_event_handler, memcached.c:5712-5734; const.h:27).  A pool keeps
 * every in-flight request's residual in one HBM buffer: replies are queued with a
 * host memcpy into per-peer pinned staging, and cec_recovery_pool_flush folds all of
 * them in ONE launch (first-touch parity copy fused, recovery.c:61-96).  The leader
 * solves any number of ready requests, of any loss count n up to m, into the lost lids'
 * arenas (memcached.c:7842-7922): single losses in one launch, n losses in ceil(n / 4).
 * A request that loses n >= 2 data lids is ready once it is complete and the other n - 1
 * participating parities' residuals have been given (cec_recovery_pool_add_residual: what
 * recover_units_gather receives into data_from_parity[lid], memcached.c:4190-4219).  Same
 * bytes as the reference chain.
 * Every call that launches ends synchronously.  A call that fails with CEC_EHIP or
 * CEC_ENOMEM before its launch leaves the pool's bookkeeping as it was: queued replies
 * stay queued, nothing is marked given or solved. */
typedef struct cec_recovery_pool cec_recovery_pool;

int cec_recovery_pool_create(cec_recovery_pool **out, int k, int m, const int *matrix, int lid_self,
                             const uint8_t *parity_arena /* device */, int capacity_units);
int cec_recovery_pool_destroy(cec_recovery_pool *pool);
int cec_recovery_pool_release_stream(cec_recovery_pool *pool, void *stream); /* LIFETIME RULE */
/* start_recovery / do_recovery: returns the request id (>= 0), CEC_EFULL when the pool
 * has no unit_end - unit_begin + 1 free contiguous units, or CEC_EINVAL. */
int cec_recovery_pool_begin(cec_recovery_pool *pool, uint32_t mask, int unit_begin, int unit_end);
/* complete_recovery_nread: data peer peer_lid's raw units of request id (host or
 * device).  Queued, not yet folded. */
int cec_recovery_pool_add_peer(cec_recovery_pool *pool, int id, int peer_lid, const void *units);
/* The same for n replies of an event-loop pass (reply i: request ids[i], data peer
 * peer_lids[i], bytes units[i]), in one call: every reply is checked as add_peer checks it
 * (and no (request, peer) pair twice) before any is queued; CEC_EINVAL queues nothing. */
int cec_recovery_pool_add_peers(cec_recovery_pool *pool, const int *ids, const int *peer_lids,
                                const void *const *units, int n);
/* Where peer peer_lid's reply for request id may be received in place (pinned, mapped;
 * *len bytes): add_peer on this pointer copies nothing. */
uint8_t *cec_recovery_pool_staging(cec_recovery_pool *pool, int id, int peer_lid, size_t *len);
/* Where parity peer parity_lid's residual for request id may be received in place (pinned,
 * mapped; *len bytes): add_residual on this pointer copies nothing.  One staging buffer per
 * other parity lid, capacity x 4 KiB, acquired on the first use of that lid (a pool that
 * never sees a multi-loss request holds none).  NULL, with nothing acquired: no such
 * request, a single-loss request, or a lid that is not another parity of the request's
 * mask; NULL also when there is no memory (cec_last_error tells which). */
uint8_t *cec_recovery_pool_parity_staging(cec_recovery_pool *pool, int id, int parity_lid, size_t *len);
/* The residual of participating parity parity_lid for multi-loss request id (its units x
 * 4 KiB; host memory, device memory, or the parity_staging pointer): C[p] of the leader's
 * solve.  Static once given: later fold_updates do not touch it, as the reference never
 * touches data_from_parity.  CEC_EINVAL: an id that is not live, a lid that is not a
 * parity of the request's mask, the pool's own lid, a parity given twice, a single-loss
 * request (it takes none).  The request goes into the next flush, which solves it if this
 * made it ready.  The copy is made before any bookkeeping changes: CEC_EHIP / CEC_ENOMEM
 * leave nothing given and nothing queued.  Host memory of any kind (pageable, pinned,
 * registered) is copied with memcpy; device memory with one synchronous copy per residual
 * -- receive into cec_recovery_pool_parity_staging where the rate matters.  A request
 * ended (cec_recovery_pool_end) before the next flush leaves the queue with it. */
int cec_recovery_pool_add_residual(cec_recovery_pool *pool, int id, int parity_lid, const void *residual);
/* The same for n residuals in one call: every entry is checked as add_residual checks it
 * (and no (request, parity) pair twice) before any is queued, CEC_EINVAL queues nothing;
 * then every copy is made before any entry is marked given, so CEC_EHIP / CEC_ENOMEM queue
 * nothing either. */
int cec_recovery_pool_add_residuals(cec_recovery_pool *pool, const int *ids, const int *parity_lids,
                                    const void *const *residuals, int n);
/* 1 when cec_recovery_pool_complete(id) holds and every other participating parity's
 * residual has been given: the request can be solved.  A single loss: == complete. */
int cec_recovery_pool_ready(const cec_recovery_pool *pool, int id);
/* Fold every queued reply in one launch; returns the requests folded (>= 0): those with a
 * reply queued, not those a residual alone put into the pass, nor those whose mask names no
 * data lid and whose first touch (R = P) the pass makes.  The pass empties the queue: a
 * request that is ready after it is NOT solved by a later _flush_solve, which looks only at
 * what has been queued since; cec_recovery_pool_solve / _solve_host solve it. */
int cec_recovery_pool_flush(cec_recovery_pool *pool, void *stream);
/* The same call also solves every queued request that it makes ready -- by its last reply or
 * by its last residual: out[lost lid] (k device arenas by data lid, arena-addressed) =
 * sum_p inv[x][p] * C[p], C[self] the new residual.  Up to three losses in the flush's own
 * launch (the residual and the shards are its four outputs); requests of n >= 4 losses are
 * folded by that launch and solved by ceil(n_max / 4) launches behind it, which read the
 * new residual from device memory.  A pass with nothing to fold has no fold launch.
 * Only requests in the queue (a reply, a residual or a begin without data lids since the
 * last flush of any kind) that are ready are solved, and of those only the ones whose lost
 * lids all have an arena: out[j] may be NULL, and a ready request that loses such a lid is
 * folded only and leaves the queue unsolved, for an explicit solve.
 * Returns the requests solved; cec_recovery_pool_solved tells which. */
int cec_recovery_pool_flush_solve(cec_recovery_pool *pool, uint8_t *const *out, void *stream);
/* 1 while the request's rebuilt bytes are current: a solve (fused or explicit) wrote them
 * and no fold_update has changed its residual since (a lost lid's diff, recovery.c:116-120,
 * clears it). */
int cec_recovery_pool_solved(const cec_recovery_pool *pool, int id);
/* check_recovery_1st_completeness: every data lid of the request's mask applied or queued. */
int cec_recovery_pool_complete(const cec_recovery_pool *pool, int id);
/* recovery_try_update_unit for every request of the pool (flushes first); returns the
 * units folded (>= 0) or a negative cec_status.  The diff is folded into every live request
 * that holds a residual, meets [addr, addr + len) and has had no reply of peer_lid -- a lid
 * the request has lost included (recovery.c:116-120) -- and requests over the same arena
 * units each take it (each counts its units).  A request folded into is no longer solved
 * (its rebuilt bytes are stale; _output is NULL) but stays ready and out of the queue: only
 * an explicit solve rebuilds it again.  Given residuals never move. */
int cec_recovery_pool_fold_update(cec_recovery_pool *pool, int peer_lid, uint64_t addr, const void *diff,
                                  uint32_t len, void *stream);
/* The same for a drain window: every update u[i] (host buffers; any data lid) folded as
 * cec_recovery_pool_fold_update would fold it, in one upload and one launch per overlap
 * wave (flushes first).  units[i] (optional) = update i's units folded; returns their sum. */
int cec_recovery_pool_fold_updates(cec_recovery_pool *pool, const cec_host_update *u, int n, int *units,
                                   void *stream);
/* Leader: out[lost lid] (k device arenas by data lid, arena-addressed) = sum_p inv[x][p] *
 * C[p] for every listed ready request (flushes first): one launch for single losses,
 * ceil(n_max / 4) for the largest loss count listed.  CEC_EINVAL (nothing solved) if a
 * listed request is not ready. */
int cec_recovery_pool_solve(cec_recovery_pool *pool, const int *ids, int n, uint8_t *const *out,
                            void *stream);
/* For a server whose recovery state stays in host memory (integration/
 * cocytus_recovery_pool.c): the same two solves, but into the pool's own mapped pinned
 * output at each request's slots instead of an arena, so no unit the caller has not
 * chosen is written (fill_completed_recovered_data skips sub_flags == 2 units,
 * memcached.c:7967-8000): plane x holds the x-th lost data lid's units, lost lids
 * ascending (as C[] / data[] are ordered, memcached.c:7911-7922); planes past the first
 * are acquired on first use.  The bytes are fenced for the host when the call returns. */
int cec_recovery_pool_flush_solve_host(cec_recovery_pool *pool, void *stream);
int cec_recovery_pool_solve_host(cec_recovery_pool *pool, const int *ids, int n, void *stream);
/* Request id's rebuilt bytes (*len = its units x 4 KiB) if its last solve was a _host one
 * and cec_recovery_pool_solved(id) still holds; NULL otherwise (never solved, last solved
 * into an arena, or folded into since).  Valid until the request ends. */
const uint8_t *cec_recovery_pool_output(const cec_recovery_pool *pool, int id, size_t *len);
/* The same for the x-th lost data lid of the request (x = 0: cec_recovery_pool_output). */
const uint8_t *cec_recovery_pool_output_lost(const cec_recovery_pool *pool, int id, int x, size_t *len);
/* Non-leader: copy request id's residual (its units x 4 KiB) to dst (host or device);
 * flushes first.  A live request that holds no residual -- its mask names data lids and no
 * reply has ever been queued, so its slots still hold what their previous owner left -- is
 * CEC_EINVAL with nothing copied and nothing flushed, as the solves refuse it. */
int cec_recovery_pool_residual(cec_recovery_pool *pool, int id, void *dst, void *stream);
/* recovery_req_remove: release the request's units.  A reply of its still queued is folded
 * first (one flush of the whole queue); a request queued by a residual or by its begin alone
 * just leaves the queue. */
int cec_recovery_pool_end(cec_recovery_pool *pool, int id);
int cec_recovery_pool_active(const cec_recovery_pool *pool);

/* ---- scrub: is the group still consistent, and if not, where? ----
 * The ops above produce parity and rebuild shards the caller knows are lost.  cec_scrub
 * asks the device whether parity still matches data: per 4 KiB tile of a plan (or of
 * [0, len)) it reads the k data and m parity streams, forms the syndromes
 * S_p = parity[p] ^ sum_j MATRIX(k+p, j) * data[j] in registers and writes NOTHING to the
 * arenas; a clean wave touches no memory but its inputs.  Where a syndrome is non-zero the
 * tile is flagged, counted once, and the wave records which data lids it can rule out as
 * the single corrupt shard (lid j is ruled out where MATRIX(k+q, j) / MATRIX(k+p0, j) * S_p0
 * != S_q in some byte, for the parities p0, q of one launch; m > 4 runs one launch per four
 * parities, and a launch of one parity rules out nothing).
 *
 * PLACEMENT: a cross-shard scrub needs all k + m arenas of the group on this device
 * (DESIGN.md §3's single-GPU placement).  A process that holds only its own shard cannot
 * scrub alone.  Where the server would call it: the idle loop (idle_event_handler,
 * memcached.c:5712-5734), over the arenas in idle time; and after a CEC_EHIP from
 * cec_drainer_apply / cec_recovery_pool_fold_updates, over the window's ranges, instead of
 * stopping.
 *
 * ENGINE: always PERM, whatever cec_set_engine says (no LDS staging, no barrier; the two
 * engines are within 2 % on every 4 KiB op); cec_last_engine() reports PERM.
 *
 * ASSUMPTION: a located lid is exact when at most one lid is corrupt in the tile.  With
 * two or more the verdict is CEC_SCRUB_UNLOCATED or, improbably, a wrong lid, as with any
 * syndrome decoder.  One such case is deterministic: where m mod 4 = 1 (m = 5) the last
 * parity is alone in its launch and rules out nothing, so a tile with one corrupt data lid
 * and that parity corrupt as well is reported as the data lid; the repair is correct for
 * that lid, and the next scrub finds the parity.  m = 1 detects but never locates.  The
 * location rests on the MDS property of the matrices
 * reed_sol_big_vandermonde_distribution_matrix returns: non-zero parity coefficients whose
 * ratios between two parity rows differ from column to column.
 * The scrub over digests (cec_scrub_digests, below) adds one limit of its own: corruption
 * of three or more 16-byte chunks of a tile in one byte column can cancel in the digest --
 * errors (1, 2, 3) * v in chunks 1, 2, 3 do -- and is then not seen at all; random
 * corruption of that kind is missed with probability 2^-16 per column.  Corruption within
 * one or two chunks of a tile is always seen, and reported exactly as cec_scrub reports it.
 *
 * A cec_scrub_report is reusable (device words + counter, pinned mirror) for runs of up to
 * max_tiles tiles; at most 0xFFFFFFFF / 256 tiles (64 GiB per arena), one dispatch.  (The
 * type is not named cec_scrub: C keeps typedefs and functions in one namespace.)  Calls on
 * one report must not overlap.  LIFETIME RULE (top): destroy waits for the streams the
 * report was used on, only.  The report keeps no pointer of a run but the plan, which must
 * outlive cec_scrub_findings / cec_scrub_repair.  Not for use inside a stream capture. */
typedef struct cec_scrub_report cec_scrub_report;
#define CEC_SCRUB_UNLOCATED (-1)
typedef struct cec_scrub_finding {
    uint64_t tile;        /* index into the run's tile list */
    uint64_t off;         /* arena offset of the tile's bytes */
    uint32_t len;         /* 1..4096 */
    uint32_t syndromes;   /* bit p: parity p's syndrome is non-zero in this tile */
    uint32_t ruled_out;   /* bit j: data lid j cannot be the single corrupt shard */
    int32_t  lid;         /* the corrupt lid (data 0..k-1, parity k..k+m-1) or CEC_SCRUB_UNLOCATED */
} cec_scrub_finding;

int cec_scrub_create(cec_scrub_report **out, uint64_t max_tiles);
int cec_scrub_destroy(cec_scrub_report *s);                /* LIFETIME RULE: waits for its streams only */
int cec_scrub_release_stream(cec_scrub_report *s, void *stream);
/* Async on `stream`: clear the report, launch, copy the counter back.  Checked as cec_encode
 * checks (code, NULL arenas, the plan's device, extent patterns must be 0); in addition
 * every data AND parity base is needed (a lost parity cannot be checked: CEC_EINVAL), and a
 * run of more tiles than the report holds is CEC_EINVAL.  A failed run leaves the report
 * invalid: wait / findings / repair return CEC_EINVAL until the next successful run. */
int cec_scrub(cec_scrub_report *s, int k, int m, const int *matrix, const uint8_t *const *data,
              const uint8_t *const *parity, const cec_plan *plan, void *stream);
int cec_scrub_region(cec_scrub_report *s, int k, int m, const int *matrix, const uint8_t *const *data,
                     const uint8_t *const *parity, size_t len, void *stream);
/* Synchronises the run's stream (never the device): flagged tiles (>= 0) or a negative cec_status. */
int64_t cec_scrub_wait(cec_scrub_report *s);
/* After the run (waits if cec_scrub_wait has not): up to cap findings, ascending tile; returns
 * the number written.  The per-tile words are copied back only when the counter is non-zero. */
int cec_scrub_findings(cec_scrub_report *s, cec_scrub_finding *out, int cap);
/* Host only.  word = syndromes | ruled_out << 8.  With exactly one syndrome bit p (m >= 2):
 * parity lid k + p.  With the syndrome bits of every parity whose coefficient for j is
 * non-zero (all m for an MDS matrix) and j the only data lid not ruled out: j.  Anything
 * else (every finding when m = 1, two lids corrupt in one tile) is CEC_SCRUB_UNLOCATED,
 * with an empty cec_last_error().  A word without a syndrome bit, or a bad code, is
 * CEC_EINVAL (the same value: cec_last_error() then holds a message). */
int cec_scrub_classify(uint32_t word, int k, int m, const int *matrix);
/* Rebuild every located finding of the last run in place, with the existing ops: one
 * cec_decode over the tiles of located data lids (per lost lid j the mask is every lid but
 * j, led by the first parity, as cec_recovery_mask builds it; out[j] is the data arena
 * itself), one cec_encode per located parity.  Unlocated findings are left untouched and
 * counted into *unrepaired.  Returns after the rebuilds completed on `stream`.  Run
 * cec_scrub again to confirm. */
int cec_scrub_repair(cec_scrub_report *s, int k, int m, const int *matrix, uint8_t *const *data,
                     uint8_t *const *parity, void *stream, int *unrepaired);

/* ---- unit digests: the scrub across processes ----
 * Cocytus runs one process per shard, each with its own arena on its own host, so no
 * process can call cec_scrub (PLACEMENT above).  The code is linear over GF(2^8); a digest
 * that is linear over GF(2^8) as well commutes with it,
 *     digest(parity_p) = sum_j MATRIX(k+p, j) * digest(data_j),
 * (homomorphic fingerprinting).  Each process digests its own arena on its own device,
 * CEC_DIGEST_BYTES per 4 KiB unit (1/128 of the bytes), ships the digests, and the leader
 * runs the scrub's syndrome and ratio test on them: the same cec_scrub_report, the same
 * wait / findings / classify, and a located unit goes to the recovery path.
 *
 * THE DIGEST.  Field: this library's (polynomial 0x11D).  A tile (a piece of an extent
 * that ends on a 4 KiB arena boundary, len = 1..4096, as cec_plan_create and the implicit
 * region make them) is padded with zeros to 4096 bytes and read as 256 chunks c_0..c_255 of
 * 16 bytes, chunk i = bytes [16 i, 16 i + 16) from the tile's first byte.  For each of the
 * 16 byte columns t:
 *     D0[t] = XOR_i c_i[t]
 *     D1[t] = sum_i w_i * c_i[t],   w_i = the field element whose byte value is i
 * digest = D0 || D1.  The digest of tile t of a plan or region is at digests + 32 * t.
 * GUARANTEE: the 256 weights are distinct, so per column the digest is a distance-3 code:
 * any corruption confined to one or two chunks of a tile changes the digest, with
 * certainty, and for such corruption the report word of cec_scrub_digests equals cec_scrub's
 * bit for bit (digest(S_p) is the syndrome of the digests, digest(ratio * S_0 ^ S_q) their
 * ratio test).  LIMIT (beside the ASSUMPTION above): corruption of three or more chunks in
 * one column can cancel -- errors (1, 2, 3) * v in chunks 1, 2, 3 of one column lie in the
 * digest's null space; random corruption of that kind is missed with probability 2^-16,
 * 2^-16c over c columns.
 *
 * SNAPSHOT RULE: the digests of a group must be taken with every shard at the same stable
 * xid, in the idle loop -- the condition cec_scrub's idle-loop placement already assumes.
 *
 * LIVE DIGESTS: a process may keep one digest array of its arena current instead of taking
 * it anew for every scrub.  The array has cec_digest_region's geometry -- unit u of the
 * arena at digests + 32 * u, chunk i of unit u = arena bytes [4096 u + 16 i, +16) -- and is
 * based once with cec_digest_region.  The digest is linear, so every diff that is XORed into
 * the arena is folded into the array too (cec_digest_apply_diffs; a parity's drainer does it
 * itself, cec_drainer_set_digests):
 *     digest(unit after) = digest(unit before) ^ c * digest(the diff, placed where it lands).
 * A live array equals cec_digest_region of the arena at any quiescent point of the owning
 * process (no diff applied to one and not yet to the other).  That gives two checks:
 *   - local, no peer, any time: cec_digest_verify_region(live, a fresh cec_digest_region of
 *     the own arena).  A mismatch is bit rot or a stray write in that arena;
 *   - across processes, no arena read: cec_scrub_digests over the shards' live arrays (same
 *     SNAPSHOT RULE).  It catches what the local check cannot: a lost or twice-applied diff.
 * With all k + m arenas on one device the SET path keeps them too: cec_diff_update_digests
 * (below) is cec_diff_update with the digests of every arena it writes kept current, from one
 * pass over new ^ old and no diff buffer.  Plain cec_diff_update does not keep digests.
 * The bulk paths keep them as well: cec_encode_digests / cec_encode_region_digests and
 * cec_decode_digests (below) are cec_encode / cec_encode_region / cec_decode whose launches
 * also emit the digests of the units they read and write, from the bytes in registers, so
 * basing a group and rebuilding a lost shard need no second pass over any arena.
 * The ops that still write an arena outside this path, and are followed by a re-base of the
 * units they wrote, are: cec_scrub_repair (it rewrites partial tiles), cec_solve, the
 * recovery sessions' and the recovery pool's solves into arenas, a plain cec_encode /
 * cec_encode_region / cec_decode / cec_diff_update (the forms without _digests; an encode or
 * decode over extents that are not whole units has no other form: the _digests ops refuse
 * them), and the units of a drain window after a CEC_EHIP.  A re-base is cec_digest_region of the one arena
 * `arena + 4096 * u0` into `digests + 32 * u0`, len = 4096 * n, for units [u0, u0 + n) (to
 * the arena's end for the last, ragged unit); the unit geometry makes that pointer arithmetic
 * valid.
 *
 * VERIFIED RECOVERY: the digest is linear, so the digest of every rebuilt unit is predictable
 * from the survivors' live digest arrays alone, and cec_decode_digests emits the digest of the
 * bytes it actually wrote.  The recipe, for units [u0, u0 + n) rebuilt under mask index q:
 *   1. take the survivors' live digest arrays (the k lids of the mask);
 *   2. cec_decode over them as "arenas", with a plan of the extent {off = 32 * u0, len = 32 * n,
 *      pattern = q} (one per run of units with the same mask), into a predicted array per lost
 *      lid;
 *   3. cec_decode_digests over the arenas, which rebuilds the units and emits their digests
 *      into an emitted array per lost lid;
 *   4. cec_digest_verify_region(report, predicted + 32 * u0, emitted + 32 * u0, 4096 * n), then
 *      cec_scrub_wait.
 * A unit that differs means: in that unit some survivor's bytes no longer match its live
 * digest (bit rot, a stray write, a lost diff), so the rebuilt unit was computed from bytes
 * the group never agreed on and is not to be trusted -- found before the shard is served, at
 * no extra arena read.  (Every decoding coefficient of an MDS code is non-zero, so a changed
 * survivor digest always changes the prediction.)  LIMIT: the digest's own, above -- corruption
 * of three or more chunks of one unit that lies in the digest's null space is not seen.
 *
 * cec_digest: digests[a] + 32 * t = digest of tile t of arenas[a], for n arenas (1..24: a
 * whole group, or a process's own) in one launch; async on `stream`.  Read-only on the
 * arenas; bytes outside the tiles are never fetched.  Every digest is written with plain
 * stores (no clear beforehand; a re-run overwrites).  Checked as cec_scrub checks: NULL
 * arrays or entries and n outside [1, 24] are CEC_EINVAL, the plan's device is checked and
 * its extent patterns must be 0, no device is CEC_ENODEV; digest arrays must be 16-byte
 * aligned (CEC_EINVAL), and tiles x n is at most 67,108,860 per call.  An empty plan or
 * len == 0 launches nothing and returns CEC_OK.  ENGINE: PERM arithmetic, as cec_scrub. */
#define CEC_DIGEST_BYTES 32
int cec_digest(int n, const uint8_t *const *arenas, uint8_t *const *digests,
               const cec_plan *plan, void *stream);
int cec_digest_region(int n, const uint8_t *const *arenas, uint8_t *const *digests,
                      size_t len, void *stream);
/* The scrub over digests (device arrays of 32 B per unit, 16-byte aligned): the sequence,
 * refusals and validity rules of cec_scrub -- clear the report, one launch per four
 * parities, copy the counter back; more units than the report holds or a NULL (lost)
 * parity digest array is CEC_EINVAL; a failed run leaves the report invalid.  `plan` / `len`
 * describe the units the digests were taken over: they give the unit count and each
 * finding's off / len; no arena is read.  Sets the same fields of the report, so
 * cec_scrub_wait / _findings / _repair work after it unchanged.  cec_scrub_repair still
 * needs the arenas on this device: it is the single-device convenience; a distributed
 * server takes each finding's lid and unit to its recovery path. */
int cec_scrub_digests(cec_scrub_report *s, int k, int m, const int *matrix,
                      const uint8_t *const *data_digests, const uint8_t *const *parity_digests,
                      const cec_plan *plan, void *stream);
int cec_scrub_digests_region(cec_scrub_report *s, int k, int m, const int *matrix,
                             const uint8_t *const *data_digests, const uint8_t *const *parity_digests,
                             size_t len, void *stream);

/* Fold applied diffs into a live digest array (LIVE DIGESTS above); async on `stream`.
 * digests: this shard's live array, unit u of the arena at digests + 32 * u (the geometry of
 * cec_digest_region: chunk i of unit u = arena bytes [4096 u + 16 i, +16)), n_units units.
 * The plan's extents are those of cec_apply_diffs: `off` the arena offset, `src_off` the
 * offset into `diffs`, `pattern` the source data lid j.  For every 4 KiB tile of the plan
 *     digests[off >> 12] ^= MATRIX(lid_self, j) * D,
 * D = the digest of a 4 KiB unit that is zero but for the tile's diff bytes at in-unit offset
 * off & 4095.  Any offset and length are accepted (16-byte aligned ones take the wide path).
 * lid_self is any lid in 0..k+m-1: for a parity the coefficient is cec_apply_diffs'; for a
 * data lid the matrix row is the identity row, so a data shard folds its own cec_set_diff
 * output with coefficient 1 and an extent that names another shard contributes nothing.
 * Tiles whose coefficient is 0 read nothing.  Bytes of `diffs` outside the tiles are never
 * fetched, and `diffs` is only read.
 * The totals are accumulated with relaxed agent-scope atomic XORs, because several values
 * share a unit; XOR commutes, so the result is bit-exact in any order.  For the same reason
 * this op ACCEPTS plans whose extents overlap: there is no CEC_EOVERLAP here (two extents on
 * the same bytes fold twice, as applying both diffs to the arena would).  Applying the same
 * plan twice restores the digests.
 * Refused with CEC_EINVAL before anything is launched: a bad code or lid_self, NULL diffs,
 * digests or plan, digests not 16-byte aligned, an extent pattern >= k, a plan of another
 * device, n_units above 2^52, and an extent that ends beyond n_units * 4096 (the message
 * names it).  An empty plan launches nothing.  A failed launch (CEC_EHIP) changes no digest.
 * ENGINE: PERM arithmetic, as cec_digest. */
int cec_digest_apply_diffs(int k, int m, const int *matrix, int lid_self, const uint8_t *diffs,
                           uint8_t *digests, uint64_t n_units, const cec_plan *plan, void *stream);

/* Fold the diff a SET batch would make into the live digests; touches no arena.  One launch,
 * async on `stream`.  The plan's extents are cec_diff_update's: `off` the arena offset,
 * `src_off` the offset into `staging`, `pattern` the source data lid j.  For every 4 KiB tile
 *     D = digest(a 4 KiB unit, zero but for (staging[src_off ..] ^ data[j][off ..]) at off & 4095)
 *     data_digests[j][off >> 12]   ^= D
 *     parity_digests[p][off >> 12] ^= MATRIX(k+p, j) * D      for p in 0..m-1
 * data_digests (k entries) and parity_digests (m entries) are live arrays of n_units units
 * each (the geometry of cec_digest_region).  Either array of pointers may be NULL, and so may
 * any entry: that array is not kept.  A destination whose coefficient is 0 is skipped as
 * well, and a tile with no destination left reads nothing.  Arena and staging bytes are only
 * read, and never outside the tiles; the two sources may have any alignment, each on its own
 * (16-byte aligned ones take the wide path).  The totals go in with relaxed agent-scope
 * atomic XORs, as in cec_digest_apply_diffs.
 * The op reads the old bytes, so it describes the batch only BEFORE the batch is installed,
 * and an extent that overlaps another would read bytes the batch itself replaces: a plan
 * whose extents overlap is CEC_EOVERLAP (unlike cec_digest_apply_diffs).  While arenas and
 * staging are unchanged, running it twice restores the digests.
 * Refused with CEC_EINVAL before anything is launched, the message naming the offender: a
 * bad code, NULL data, staging or plan, a NULL data[j] (j < k), a non-NULL digest array that
 * is not 16-byte aligned, an extent pattern >= k, a plan of another device, n_units above
 * 2^52, an extent that ends beyond n_units * 4096, and more than 67,108,860 tiles.  An empty
 * plan launches nothing.  A failed launch (CEC_EHIP) changes no digest.
 * ENGINE: PERM arithmetic whatever cec_set_engine says; cec_last_engine() reports PERM. */
int cec_digest_set(int k, int m, const int *matrix, const uint8_t *const *data,
                   const uint8_t *staging, uint8_t *const *data_digests,
                   uint8_t *const *parity_digests, uint64_t n_units,
                   const cec_plan *plan, void *stream);

/* cec_diff_update, with the digests of every arena it writes kept current: the SET op of a
 * placement with all k + m arenas on one device.  Every check of cec_diff_update and of
 * cec_digest_set is made, and both steps are planned, before anything is launched.  The op
 * is strict about the arrays: data_digests[j] must be non-NULL for every j < k when install
 * != 0, and parity_digests[p] for every p with parity[p] != NULL, else CEC_EINVAL -- a
 * silently stale array is worse than a refusal.  It then enqueues on `stream`
 *   1. the cec_digest_set launch, over the parity digests of the live parities and, when
 *      install != 0, the data digests (install == 0 leaves the data arenas as they are, so
 *      their digests are not touched); a lost parity (parity[p] == NULL) is skipped;
 *   2. behind it, cec_diff_update itself, unchanged: one launch per four outputs (one for
 *      m + install <= 4).  Arena bytes after the op are cec_diff_update's, on either engine.
 * If step 2 fails before its first launch (CEC_EHIP) the arenas and staging are untouched,
 * so the op enqueues the digest launch once more, which restores the digests, and returns
 * CEC_EHIP: arenas and digests are then as before the call.  If that restoring launch fails
 * too, or step 2 failed after one of its launches ran (m + install > 4), the message says
 * that the digests of the plan's units are uncertain: re-base them with cec_digest_region
 * as LIVE DIGESTS describes. */
int cec_diff_update_digests(int k, int m, const int *matrix, uint8_t *const *data,
                            const uint8_t *staging, uint8_t *const *parity, int install,
                            uint8_t *const *data_digests, uint8_t *const *parity_digests,
                            uint64_t n_units, const cec_plan *plan, void *stream);

/* Digest-emitting encode and decode: the bulk paths with live digests kept (LIVE DIGESTS,
 * VERIFIED RECOVERY above).  cec_encode / cec_encode_region / cec_decode on the same
 * arguments, and in the same launches the digests of the units read and written: one wave per
 * 4 KiB unit holds the unit of each stream in registers, so no arena byte is read twice.
 * ARENA BYTES after each op are those of the op without _digests, on either engine setting.
 * DIGESTS: arrays of cec_digest_region's geometry (unit u of the arena at array + 32 * u,
 * 16-byte aligned).  For every unit u of the plan (unit off >> 12 of each tile), array[u] of
 * every kept array equals what cec_digest_region of that arena yields for unit u afterwards;
 * units outside the plan are not touched in any array.
 *   cec_encode_digests / cec_encode_region_digests keep data_digests (k entries, the inputs)
 *   and parity_digests (m entries, the outputs).  Either array of pointers may be NULL, and so
 *   may any entry: that array is not kept.  A lost parity (parity[p] == NULL) is not produced
 *   and its digest entry is ignored.  In cec_encode_region_digests, len is the arena length.
 *   cec_decode_digests keeps out_digests (k entries, indexed by data lid like `out`): the
 *   digests of the rebuilt units.  The entry of every lid that some mask loses must be
 *   non-NULL, else CEC_EINVAL -- strictness where staleness would be silent, as in
 *   cec_diff_update_digests.  Masks rotate per extent through `pattern`, as in cec_decode.
 * UNIT RULE: the digest of a partly written unit cannot be formed without its old bytes, so
 * every extent has off % 4096 == 0 and every tile is a whole 4 KiB unit, except a last tile
 * shorter than 4096 bytes, accepted only where it ends exactly at arena_len (the arena's own
 * ragged last unit: its digest is that of the bytes zero-padded); no extent ends beyond
 * arena_len.
 * LAUNCHES: one per four outputs (CEC_KERNEL_COMBINE_DIGEST), in order on `stream`; input
 * digests are written by the first launch only.  Every launch writes a unit's bytes and that
 * unit's digests together.  FAILURE: after a CEC_EHIP on launch g, the outputs of the launches
 * before g are complete with matching digests, and the outputs of g and of later launches are
 * untouched in bytes and in digests (the input digests are complete if g > 0, untouched if
 * g == 0); cec_last_launch's seq tells how many ran.
 * REFUSED with CEC_EINVAL before anything is launched, the message naming the offender:
 * everything cec_encode / cec_decode refuse, a non-NULL digest array that is not 16-byte
 * aligned, a breach of the unit rule, an out_digests entry missing for a lost lid, and more
 * than 67,108,860 tiles (one dispatch).  An empty plan or len == 0 launches nothing and
 * returns CEC_OK.
 * ENGINE: PERM arithmetic whatever cec_set_engine says; cec_last_engine() reports PERM.
 * COST: by byte counts, basing an RS(3,2) group moves 5/8 of the traffic of cec_encode_region
 * + cec_digest_region over the data + an encode over the digest arrays, and a rebuild 4/5 of
 * cec_decode + cec_digest of the rebuilt units.  MEASURED on one MI355X, 65,536 units per
 * arena, HIP events, fused and unfused interleaved in one process, three processes
 * (tools/fused_digest_bench.py, profiles/fused_digest_bench.jsonl): basing
 * takes 0.66 of the unfused sequence's time (219-221 us against 334-337 us), the rebuild with
 * masks rotating per unit 0.84-0.86 (189-190 us against 220-226 us).  The ops' reason is
 * their consistency contract; the time saved comes with it. */
int cec_encode_digests(int k, int m, const int *matrix, const uint8_t *const *data,
                       uint8_t *const *parity, uint8_t *const *data_digests,
                       uint8_t *const *parity_digests, uint64_t arena_len,
                       const cec_plan *plan, void *stream);
int cec_encode_region_digests(int k, int m, const int *matrix, const uint8_t *const *data,
                              uint8_t *const *parity, uint8_t *const *data_digests,
                              uint8_t *const *parity_digests, size_t len, void *stream);
int cec_decode_digests(int k, int m, const int *matrix, const uint32_t *masks, int n_masks,
                       const uint8_t *const *arenas, uint8_t *const *out,
                       uint8_t *const *out_digests, uint64_t arena_len,
                       const cec_plan *plan, void *stream);

/* A process's check of itself: compare its live array with a fresh cec_digest_region of its
 * own arena (both device arrays of 32 B per unit over [0, len), 16-byte aligned).  It is
 * cec_scrub_digests_region with the code k = 1, m = 1, matrix {1, 1}, `fresh` as the data
 * digests and `live` as the parity's: the syndrome is live ^ fresh.  Same report, same
 * refusals; cec_scrub_wait returns the differing units and cec_scrub_findings their tile,
 * off and len.  Every finding's lid is CEC_SCRUB_UNLOCATED (m = 1 never locates): the caller
 * knows the lid is its own.  cec_scrub_repair does not apply to such a run. */
int cec_digest_verify_region(cec_scrub_report *s, const uint8_t *live, const uint8_t *fresh,
                             size_t len, void *stream);

/* ---- process-wide caches ----
 * Coefficient tables are uploaded once per distinct content (asynchronously, on the
 * caller's stream; another stream waits on the upload event) and kept in an LRU cache
 * of at most pattern_entry_limit sets per device.  Evicting synchronises the device once
 * per batch of victims; a fixed set of codes and masks never evicts.  Tables used inside
 * a stream capture stay for the life of the process (the graph holds their address).
 * Idle device and pinned buffers of plans, recovery sessions, drainers, pools and the
 * drop-in are kept for reuse (freeing them would wait for the whole device), capped at
 * 2 GiB device / 1 GiB pinned / 512 MiB mapped pinned.  At process exit the library
 * synchronises each device it cached state for and frees it. */
typedef struct cec_cache_info {
    uint64_t pattern_entries;      /* coefficient-table sets cached on this device */
    uint64_t pattern_bytes;        /* their device bytes (a pinned mirror each as well) */
    uint64_t pattern_uploads;      /* sets uploaded since start (misses) */
    uint64_t pattern_evictions;    /* LRU evictions since start */
    uint64_t pattern_entry_limit;
    uint64_t device_cached_bytes;  /* idle device buffers held for reuse (all devices) */
    uint64_t pinned_cached_bytes;  /* idle pinned host buffers held for reuse */
} cec_cache_info;
int cec_cache_get_info(cec_cache_info *out);       /* current device */
int cec_cache_set_pattern_limit(int entries);      /* default 4096 (CEC_PATTERN_CACHE_ENTRIES) */
/* Free every idle cached buffer and every coefficient-table set not used by a captured
 * graph (synchronises the current device first). */
int cec_cache_trim(void);

/* ---- completion record (diagnostics) ----
 * How the calling thread's last synchronous completion (the drop-in
 * galois_w08_region_multiply, cec_recovery_fold_update / _solve / _finish,
 * cec_recovery_pool_flush / _flush_solve / _fold_update / _solve) made its results
 * visible to the host on return.  A result in
 * host-visible memory (pinned, mapped or managed) may still sit in the L2 of the XCD
 * that wrote it; it is visible only if every writing wave ended with a system-scope
 * release or a system-scope fence ran behind the op.  Tests assert the protocol with it
 * on any box, whether or not the box's host mappings expose a missing release. */
typedef struct cec_sync_record {
    uint64_t seq;           /* synchronous completions on this thread so far */
    int host_results;       /* the op wrote host-visible memory */
    int waves_released;     /* every writing wave ended with a system-scope release */
    int fenced;             /* a system-scope fence ran behind the op (fence event or stream sync) */
} cec_sync_record;
int cec_last_sync(cec_sync_record *out);

/* ---- launch record (tests and diagnostics) ----
 * Which kernel the calling thread's last enqueued launch ran, and how.  Per thread, like
 * cec_last_sync, and for tests and diagnostics only: every op of the library runs one
 * kernel template compiled into about a hundred kernels (narrow 1 x 1, exact shapes,
 * capacity kernels, each for both engines), and which of them an op lands on is decided
 * by the host -- a test that compares bytes alone cannot tell.  Filled after every
 * successful launch; a refused or failed launch leaves it as it was.  Before the thread's
 * first launch seq is 0 and kind / acc / engine are -1. */
enum { CEC_KERNEL_NARROW = 0, CEC_KERNEL_EXACT = 1, CEC_KERNEL_GENERIC = 2,
       CEC_KERNEL_SCRUB = 3 /* cec_scrub's read-only kernel: nt = k or its capacity {4,8,16}, lt = the
                             * launch's parities or their capacity {1,2,4}, acc = CEC_ACC_ALL, PERM */,
       CEC_KERNEL_DIGEST = 4 /* cec_digest: nt = the arenas of the launch, lt = 0, acc = CEC_ACC_NONE,
                              * split_shift 0, PERM, flags 0 */,
       CEC_KERNEL_DIGEST_CHECK = 5 /* cec_scrub_digests: nt / lt = the capacities {4,8,16} x {1,2,4},
                                    * acc = CEC_ACC_ALL, PERM, flags 0 */,
       CEC_KERNEL_DIGEST_UPDATE = 6 /* cec_digest_apply_diffs and the drainer's digest launch: nt = 1,
                                     * lt = 0, acc = CEC_ACC_ALL, split_shift 0, PERM, flags 0, grid =
                                     * ceil(tiles / 4) */,
       CEC_KERNEL_DIGEST_SET = 7 /* cec_digest_set and the digest launch of cec_diff_update_digests:
                                  * nt = 2 (the staged value and the old bytes), lt = 0, acc =
                                  * CEC_ACC_ALL, split_shift 0, PERM, flags 0, grid = ceil(tiles / 4) */,
       CEC_KERNEL_COMBINE_DIGEST = 8 /* cec_encode_digests, cec_encode_region_digests, cec_decode_digests:
                                      * nt = the launch's inputs, lt = the output capacity {1,2,4}, acc =
                                      * CEC_ACC_NONE, split_shift 0, PERM, flags 0, grid = ceil(tiles / 4) */ };
enum { CEC_ACC_NONE = 0, CEC_ACC_ALL = 1, CEC_ACC_ALL_BUT_LAST = 2, CEC_ACC_RUNTIME = 3 };
enum { CEC_LAUNCH_SYS_RELEASE = 1, CEC_LAUNCH_WRITE_THROUGH = 2,
       CEC_LAUNCH_WT_TAIL = 4 /* non-temporal body, write-through stores from work item wt_from on */ };
#define CEC_NO_WT_TAIL UINT64_MAX
typedef struct cec_launch_record {
    uint64_t seq;           /* launches this thread has enqueued so far, this one included; never resets */
    int kind;               /* CEC_KERNEL_NARROW (two-slot 1 x 1), _EXACT (shape) or _GENERIC (capacity) */
    int nt, lt;             /* input / output counts the kernel was instantiated with: the shape
                             * itself (narrow, exact) or the capacities chosen, {2,4,8,16} x {1,2,4} */
    int acc;                /* read-modify-write outputs: CEC_ACC_NONE, _ALL, _ALL_BUT_LAST (exact and
                             * narrow kernels) or _RUNTIME (capacity kernels: per pattern) */
    int engine;             /* CEC_ENGINE_PERM or CEC_ENGINE_LDS */
    uint32_t split_shift;   /* 2^split_shift workgroups of 256 >> split_shift lanes per tile */
    uint32_t flags;         /* CEC_LAUNCH_* bits passed to the kernel (the LDS engine's kernels keep
                             * non-temporal stores whatever the write-through bit says) */
    uint32_t grid;          /* workgroups */
    uint64_t n_tiles;
    uint64_t lds_bytes;     /* dynamic LDS of the launch */
    uint64_t wt_from;       /* CEC_LAUNCH_WT_TAIL: the first work item (tile << split_shift | part) whose
                             * stores write through; CEC_NO_WT_TAIL otherwise */
} cec_launch_record;
int cec_last_launch(cec_launch_record *out);

/* ---- test hooks (host only, launch nothing themselves; not for servers) ----
 * cec_internal_check_launch_layout: the launch-time check every op's launch runs, on one
 * pattern reading in_slots and writing out_slots, against the kernel argument block built
 * from bases[0..n_bases) -- the two-slot block of the narrow 1 x 1 kernels (narrow != 0)
 * or the full one.  CEC_OK, or CEC_EINVAL where the launch would be refused (a slot the
 * block does not carry, or a NULL base).
 * cec_internal_store_policy: the store policy parsed from CEC_STORE_POLICY (0 auto,
 * 1 non-temporal, 2 write-through; unknown values warn once and mean auto) and, in
 * *wt_max_bytes, auto's write-through limit (CEC_WT_MAX_BYTES, default 512 MiB). */
int cec_internal_check_launch_layout(int narrow, const int *in_slots, int n_in, const int *out_slots,
                                     int n_out, const void *const *bases, int n_bases);
int cec_internal_store_policy(uint64_t *wt_max_bytes);
/* cec_internal_wt_from: the store choice of a launch of n_tiles tiles in 2^split_shift
 * workgroups each, lt outputs, `streamed` bytes read and written: 0 non-temporal, 2
 * write-through, 1 a non-temporal body and a write-through tail from work item *wt_from
 * (CEC_NO_WT_TAIL otherwise).  *wt_tail_bytes: the tail in force (CEC_WT_TAIL_BYTES). */
int cec_internal_wt_from(uint64_t n_tiles, uint32_t split_shift, int lt, uint64_t streamed,
                         uint64_t *wt_tail_bytes, uint64_t *wt_from);
/* cec_internal_fail_launch: fault injection for the error paths (tests only) -- the calling
 * thread's next `after` kernel launches run and the one after them fails as a HIP error
 * would (CEC_EHIP, nothing launched); then the hook disarms.  after < 0 disarms it. */
int cec_internal_fail_launch(int after);

/* ---- stream / event helpers, so C and ctypes callers need no HIP header ----
 * Events are for timing: recorded without the system-scope fence, so waiting on one
 * does not make results written into host memory visible.  Use cec_stream_synchronize
 * (or a synchronous call) before reading those. */
int cec_event_create(void **ev);
int cec_event_destroy(void *ev);
int cec_event_record(void *ev, void *stream);
int cec_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on stop */
int cec_stream_synchronize(void *stream);
/* Device selection for C callers (one host thread per GPU): the calling
 * thread's current device, as hipGetDeviceCount / hipSetDevice. */
int cec_device_count(int *count);
int cec_set_device(int device);
/* A non-blocking stream of the current device (each is a hardware queue: use one per
 * thread). */
int cec_stream_create(void **stream);
int cec_stream_destroy(void *stream);
/* Async copy between any host / device buffers (arena bytes to and from the server's
 * buffers); complete after cec_stream_synchronize(stream). */
int cec_copy(void *dst, const void *src, size_t n, void *stream);
/* A host arena the server keeps in its own memory (ecmem: mmap'd, ecmem.h:36-42) made
 * reachable by the kernels: page-locked and mapped once
 * (hipHostRegister), *device_alias = its address for the device ops (cec_encode,
 * cec_drainer_apply, ...; results are complete for the host after the op's stream
 * synchronises, or on return of the synchronous calls).  Unregister before freeing it. */
int cec_host_register(void *p, size_t bytes, uint8_t **device_alias);
int cec_host_unregister(void *p);

#ifdef __cplusplus
}
#endif
#endif /* COCYTUS_EC_H */
