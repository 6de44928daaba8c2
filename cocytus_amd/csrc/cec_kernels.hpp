// cec_kernels.hpp -- CDNA4 (gfx950) HIP kernels for Cocytus' erasure-coding hot path.
//
// Every op on the path -- galois_w08_region_multiply, the per-SET
// diff-update (a2 + a3 = a4), full-stripe encode (a5), the recovery residual (a6)
// and the leader solve (a7) -- is a GF(2^8) linear combination of byte streams
// taken at the same arena offset:
//
//     out[l][off .. off+len)  (^)=  sum_i  coef[l][i] * in[i][off .. off+len)
//
// so one kernel family implements all of them.  A launch walks a work-list of
// 4 KiB tiles (CEC_UNIT_SIZE, /root/reference/const.h:26) built from the batch's
// extents; each tile carries a pattern index that selects the inputs, outputs and
// coefficients (per source shard for diff-update, per erasure mask for decode).
//
// Hardware mapping (MI355X):
//   * one 16-byte chunk per lane: a 4 KiB tile is 256 lanes, as one 256-lane
//     workgroup or (full, line-aligned tiles) four one-wave workgroups of 64
//     (split_shift); every stream of a tile is read with one fully coalesced
//     global_load_dwordx4 per lane (uniform SGPR base + per-lane VGPR offset);
//   * tile metadata and coefficient tables are wave-uniform and live in SGPRs
//     (constant-address-space loads -> s_load);
//   * GF multiply by a uniform coefficient c on 4 packed bytes:
//       PERM engine: c*x = T0[x&7] ^ T1[(x>>3)&7] ^ T2[x>>6], three v_perm_b32
//                    byte lookups per dword (tables are 8 bytes: two SGPRs);
//       LDS engine : 256-entry product rows c*x = exp[log x + log c], one per
//                    coefficient of the tile's pattern, built from the log / antilog
//                    tables and staged in LDS per workgroup: one ds_read_u8 per byte;
//     no MFMA: this is byte-field arithmetic, HBM-bound.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cec_layout.hpp"
#include "gf256.hpp"

namespace cec {

// Kernel arguments with S stream slots.  Patterns name streams by slot.  The host
// writes a launch's whole kernarg segment for every dispatch, and 424 B of arguments
// cost 1.3 us more host time per launch than none (tools/dropin_breakdown.hip).  So a
// launch whose patterns use only slots 0 and 1 (region multiply, the drop-in) takes
// S = 2, and the kernel reads its grid size from here rather than from gridDim /
// blockDim: those come from the hidden arguments, which add 256 B to every segment.
template <int S>
struct CombineArgsCore {
    uint8_t *base[S];
    const Tile *tiles;       // NULL: implicit region [0, implicit_len), pattern 0
    const Pattern *patterns;
    const uint8_t *rows;     // LDS engine: 256-B product rows (c*x for x = 0..255)
    uint64_t implicit_len;
    uint32_t n_tiles;
    uint32_t split_shift;  // 2^split_shift workgroups of kBlock >> split_shift lanes per tile
    uint32_t grid;         // workgroups in the launch (the grid-stride step)
    uint32_t flags;        // kFlag* bits (fills the struct's padding)
};
// The full block adds the write-through tail: work items g >= wt_from store as a
// kFlagWriteThrough launch does, the ones before them non-temporally (kNoWtTail: none).
// It comes last, so every other field keeps its offset.  The narrow block does not carry it:
// narrow launches are small and write through as a whole.
template <int S>
struct CombineArgsN : CombineArgsCore<S> {
    uint64_t wt_from;
};
template <>
struct CombineArgsN<kNarrowStreams> : CombineArgsCore<kNarrowStreams> {};
using CombineArgs = CombineArgsN<kMaxStreams>;
static_assert(sizeof(CombineArgsN<kNarrowStreams>) == 64, "the narrow kernels' argument block must not grow");

#define CEC_CONST __attribute__((address_space(4)))
#define CEC_GLOBAL __attribute__((address_space(1)))

// Read-only kernel inputs are re-addressed in the constant address space so that
// wave-uniform loads of them become scalar (s_load) loads.
template <class T>
__device__ inline const CEC_CONST T *as_const(const T *p) {
    return (const CEC_CONST T *)(uintptr_t)p;
}

// Arena bytes: global address space, so a uniform base + per-lane offset becomes
// global_load_dwordx4 v, v_off, s[base] (no flat addressing, no 64-bit VGPR math).
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Streamed bytes are touched once per launch: non-temporal loads and stores (nt)
// measured +5-10 % over the default policy on this access pattern.
__device__ inline uint4 ld16(const uint8_t *base, uint32_t off) {
    const u32x4 v = __builtin_nontemporal_load((const CEC_GLOBAL u32x4 *)((uintptr_t)base + off));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ inline void st16(uint8_t *base, uint32_t off, const uint4 &v) {
    u32x4 w;
    w.x = v.x;
    w.y = v.y;
    w.z = v.z;
    w.w = v.w;
    __builtin_nontemporal_store(w, (CEC_GLOBAL u32x4 *)((uintptr_t)base + off));
}
// Write-through (sc1) store of one 16-B chunk at base + off, off < kTile: a buffer store
// through a descriptor built from the wave-uniform tile base (SGPRs).
__device__ inline void st16_wt(uint8_t *base, uint32_t off, const uint4 &v) {
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, kTile, 0x00020000);
    u32x4 w;
    w.x = v.x;
    w.y = v.y;
    w.z = v.z;
    w.w = v.w;
    __builtin_amdgcn_raw_buffer_store_b128(w, rs, off, 0, 16 /* sc1 */);
}
__device__ inline uint32_t ld8(const uint8_t *base, uint32_t off) {
    return *(const CEC_GLOBAL uint8_t *)((uintptr_t)base + off);
}
__device__ inline void st8(uint8_t *base, uint32_t off, uint32_t v) {
    *(CEC_GLOBAL uint8_t *)((uintptr_t)base + off) = static_cast<uint8_t>(v);
}

// ---------------------------------------------------------------- engines
struct PermEngine {
    static constexpr bool kStaged = false;
    struct Sel {
        uint32_t s0, s1, s2;
    };
    __device__ static inline Sel sel(uint32_t x) {
        return Sel{x & 0x07070707u, (x >> 3) & 0x07070707u, (x >> 6) & 0x03030303u};
    }
    __device__ static inline uint32_t mul(const Sel &s, const CEC_CONST uint32_t *t,
                                          const uint8_t *) {
        const uint32_t a = __builtin_amdgcn_perm(t[1], t[0], s.s0);
        const uint32_t b = __builtin_amdgcn_perm(t[3], t[2], s.s1);
        const uint32_t c = __builtin_amdgcn_perm(t[4], t[4], s.s2);
        return a ^ b ^ c;
    }
};

// One 256-B row per non-trivial coefficient of the tile's pattern, row_c[x] = c*x
// (row_c[0] = 0: no zero sentinel).  A ds_read_u8 of a 64-dword row has at most two
// distinct dwords per bank (32 banks for byte / dword reads), and lanes that hit the
// same dword broadcast, so a random lookup costs <= 2 LDS cycles per 32-lane group.
struct LdsEngine {
    static constexpr bool kStaged = true;
    struct Sel {
        uint32_t b0, b1, b2, b3;
    };
    __device__ static inline Sel sel(uint32_t x) {
        return Sel{x & 0xFFu, (x >> 8) & 0xFFu, (x >> 16) & 0xFFu, x >> 24};
    }
    __device__ static inline uint32_t mul(const Sel &s, const CEC_CONST uint32_t *t,
                                          const uint8_t *lds) {
        const uint8_t *row = lds + t[0];
        return static_cast<uint32_t>(row[s.b0]) | (static_cast<uint32_t>(row[s.b1]) << 8) |
               (static_cast<uint32_t>(row[s.b2]) << 16) | (static_cast<uint32_t>(row[s.b3]) << 24);
    }
};

// ---------------------------------------------------------------- helpers
struct TileRef {
    uint64_t off, src_off;
    uint32_t len;  // bytes of this tile, 1..kTile
    uint32_t pattern;
};

template <class A>
__device__ inline TileRef load_tile(const A &a, uint32_t t) {
    TileRef r;
    if (a.tiles == nullptr) {
        const uint64_t o = static_cast<uint64_t>(t) * kTile;
        const uint64_t rem = a.implicit_len - o;
        r.off = o;
        r.src_off = o;
        r.len = rem < kTile ? static_cast<uint32_t>(rem) : kTile;
        r.pattern = 0;
    } else {
        const CEC_CONST Tile *tl = as_const(a.tiles) + t;
        r.off = tl->off;
        r.src_off = tl->src_off;
        r.len = tl->len;
        r.pattern = tl->pattern;
    }
    return r;
}

// A ragged chunk: the first cnt (1..16) bytes at base+off.  Branch-free: byte b
// reads address off + min(b, cnt-1), so all 16 loads are in bounds and in flight
// together (one memory latency, not sixteen dependent ones); bytes >= cnt read 0.
__device__ inline uint4 gather16(const uint8_t *base, uint32_t off, uint32_t cnt) {
    uint32_t v[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) v[b] = ld8(base, off + min(static_cast<uint32_t>(b), cnt - 1));
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < 16; ++b) w[b >> 2] |= (static_cast<uint32_t>(b) < cnt ? v[b] : 0u) << (8 * (b & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// Store the first cnt bytes of v at base+off.  Byte b goes to off + min(b, cnt-1)
// with the value of that clamped byte, so surplus stores rewrite the last valid byte
// with its own (correct) value: no predication, never out of bounds.
__device__ inline void scatter16(uint8_t *base, uint32_t off, uint32_t cnt, const uint4 &v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        const uint32_t q = min(static_cast<uint32_t>(b), cnt - 1);
        st8(base, off + q, w[q >> 2] >> (8 * (q & 3)));
    }
}

// acc[l] ^= sum_i coef[l][i] * x[i] on one 16-byte chunk of every stream.
template <int NT, int LT, class Eng>
__device__ inline void compute_chunk(const CEC_CONST Pattern *P, int n_in, int n_out,
                                     const uint4 (&x)[NT], uint4 (&acc)[LT], const uint8_t *lds) {
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        if (i >= n_in) continue;
        const uint32_t xv[4] = {x[i].x, x[i].y, x[i].z, x[i].w};
        typename Eng::Sel s[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) s[w] = Eng::sel(xv[w]);
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            if (l >= n_out) continue;
            const int c = P->coef[l][i];
            if (c == 0) continue;
            if (c == 1) {
                acc[l].x ^= xv[0];
                acc[l].y ^= xv[1];
                acc[l].z ^= xv[2];
                acc[l].w ^= xv[3];
            } else {
                const CEC_CONST uint32_t *tb = P->tab[l][i];
                acc[l].x ^= Eng::mul(s[0], tb, lds);
                acc[l].y ^= Eng::mul(s[1], tb, lds);
                acc[l].z ^= Eng::mul(s[2], tb, lds);
                acc[l].w ^= Eng::mul(s[3], tb, lds);
            }
        }
    }
}

// ---------------------------------------------------------------- the kernel
// NT / LT: input / output counts.  kExact: the patterns have exactly NT inputs and
// LT outputs (the hot shapes: straight-line loads, no guards); otherwise NT / LT
// are capacities and the pattern's n_in / n_out are wave-uniform runtime counts.
// kAcc: which outputs are read-modify-write (XOR-accumulate):
//   0 none, 1 all, 2 all but the last (diff-update + install), 3 per pattern.

// A workgroup covers 1 / 2^split_shift of a tile (blockDim = kBlock >> split_shift):
// work item g is tile g >> split_shift, part g & (2^split_shift - 1).
// kSysRel: every wave ends with a system-scope release (kFlagSysRelease launches; a
// template parameter, so the batched kernels carry no epilogue at all).
// LDS engine, full aligned tiles: stage the product rows before the stream loads (the
// fast path in combine_kernel) for the diff-update shapes only (2 inputs, parity
// read-modify-write).  There it ran the diff-update + install 2.4 % faster; in the
// encode (3 x 2) the second path's registers cost SGPR spills and occupancy (+10 %),
// and the fixed-mask decode / residual (3 x 1) lost 2-3 %
// (profiles/r03_evidence/lds_early_rows/).
template <int NT, int kAcc, bool kExact>
constexpr bool kEarlyRows = kExact && NT == 2 && (kAcc == kAccAll || kAcc == kAccAllButLast);

template <int NT, int LT, class Eng, int kAcc, bool kExact, int S = kMaxStreams, bool kSysRel = false>
__global__ __launch_bounds__(kBlock) void combine_kernel(CombineArgsN<S> a) {
    extern __shared__ uint4 cec_lds_rows[];  // LDS engine: the pattern's product rows
    const uint8_t *lds = reinterpret_cast<const uint8_t *>(cec_lds_rows);
    const uint32_t sh = a.split_shift;
    const uint64_t n_work = static_cast<uint64_t>(a.n_tiles) << sh;

    // The LDS engine keeps the hardware grid / workgroup sizes: with them its register
    // allocation holds the step in a register, while a.grid was re-loaded (with a full
    // scalar wait) at the end of every tile, 3 % slower on the encode (tools/track_ab.sh).
    const uint32_t step = Eng::kStaged ? gridDim.x : a.grid;
    for (uint64_t g = blockIdx.x; g < n_work; g += step) {
        const uint32_t t = static_cast<uint32_t>(g >> sh);
        const uint32_t part = static_cast<uint32_t>(g) & ((1u << sh) - 1u);
        const uint32_t lane = (part << (kBlockLog2 - sh)) + threadIdx.x;
        const TileRef tr = load_tile(a, t);
        const CEC_CONST Pattern *P = as_const(a.patterns) + tr.pattern;
        const int n_in = kExact ? NT : P->n_in;
        const int n_out = kExact ? LT : P->n_out;
        if (!kExact && n_out == 0) continue;
        // A workgroup that walks several tiles (a launch past one dispatch's 2^32 - 1
        // work items) must not re-stage LDS rows while lanes still read the previous tile's.
        if constexpr (Eng::kStaged)
            if (g != blockIdx.x) __syncthreads();
        auto is_acc = [&](int l) -> bool {
            if constexpr (kAcc == kAccNone) return false;
            else if constexpr (kAcc == kAccAll) return true;
            else if constexpr (kAcc == kAccAllButLast) return l < LT - 1;
            else return P->out_mode[l] == kModeXor;
        };

        const uint8_t *in[NT];
        uint8_t *out[LT];
        uint64_t mis = 0;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            in[i] = nullptr;
            if (i < n_in) {
                in[i] = a.base[P->in_stream[i]] + (P->in_src[i] ? tr.src_off : tr.off);
                mis |= reinterpret_cast<uint64_t>(in[i]);
            }
        }
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            out[l] = nullptr;
            if (l < n_out) {
                out[l] = a.base[P->out_stream[l]] + (P->out_src[l] ? tr.src_off : tr.off);
                mis |= reinterpret_cast<uint64_t>(out[l]);
            }
        }

        // one 16-byte chunk per lane; the value's ragged tail (len = vlen + 2 is
        // rarely a multiple of 16) and tiles of misaligned device pointers use the
        // branch-free byte gather / scatter, everything else dwordx4.
        const uint32_t pos = lane * 16;
        if constexpr (Eng::kStaged && kEarlyRows<NT, kAcc, kExact>) {
            if ((mis & 15) == 0 && tr.len == kTile) {
                // A full, aligned tile (wave-uniform: every lane one whole chunk), the
                // LDS engine's common case.  Its product rows are fetched BEFORE the
                // stream loads, and the stream loads are unconditional, so the LDS write
                // waits only for the rows (vmcnt counts loads in order) and the write
                // and the barrier complete under the streams' HBM latency; the lookups
                // start as soon as the stream data lands.  (Staged after the stream
                // loads, below, the write waits for every stream load.)
                const uint32_t nb16 = static_cast<uint32_t>(P->lds_rows) * 16u;
                const uint4 *row_src = reinterpret_cast<const uint4 *>(a.rows) + P->lds_row_base * 16;
                uint4 row0 = make_uint4(0, 0, 0, 0);
                if (threadIdx.x < nb16) row0 = row_src[threadIdx.x];
                uint4 x[NT];
                uint4 acc[LT];
#pragma unroll
                for (int i = 0; i < NT; ++i)
                    if (i < n_in) x[i] = ld16(in[i], pos);
#pragma unroll
                for (int l = 0; l < LT; ++l) {
                    acc[l] = make_uint4(0, 0, 0, 0);
                    if (l < n_out && is_acc(l)) acc[l] = ld16(out[l], pos);
                }
                if (nb16) {
                    if (threadIdx.x < nb16) cec_lds_rows[threadIdx.x] = row0;
                    for (uint32_t b = threadIdx.x + blockDim.x; b < nb16; b += blockDim.x)
                        cec_lds_rows[b] = row_src[b];  // (more rows than lanes)
                    __syncthreads();
                }
                compute_chunk<NT, LT, Eng>(P, n_in, n_out, x, acc, lds);
#pragma unroll
                for (int l = 0; l < LT; ++l)
                    if (l < n_out) st16(out[l], pos, acc[l]);
                continue;
            }
        }
        const bool active = pos < tr.len;
        if constexpr (!Eng::kStaged)
            if (!active) continue;  // (staged engines keep every lane to the barrier)
        const uint32_t cnt = active ? min(16u, tr.len - pos) : 16u;
        const bool wide = (mis & 15) == 0 && cnt == 16;
        uint4 x[NT];
        uint4 acc[LT];
        if (!active) {
        } else if (wide) {
#pragma unroll
            for (int i = 0; i < NT; ++i)
                if (i < n_in) x[i] = ld16(in[i], pos);
#pragma unroll
            for (int l = 0; l < LT; ++l) {
                acc[l] = make_uint4(0, 0, 0, 0);
                if (l < n_out && is_acc(l)) acc[l] = ld16(out[l], pos);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NT; ++i)
                if (i < n_in) x[i] = gather16(in[i], pos, cnt);
#pragma unroll
            for (int l = 0; l < LT; ++l) {
                acc[l] = make_uint4(0, 0, 0, 0);
                if (l < n_out && is_acc(l)) acc[l] = gather16(out[l], pos, cnt);
            }
        }
        if constexpr (Eng::kStaged) {
            // Stage this pattern's product rows (L2-resident, 256 B each; 512 B for an
            // RS(3,2) encode) while the stream loads above are in flight.
            // A pattern of XORs only (coefficients 0 / 1: e.g. every decode led by the
            // all-ones parity row) has no rows and skips the barrier; the branch is
            // uniform over the workgroup (one tile, one pattern).
            const uint32_t nb = static_cast<uint32_t>(P->lds_rows) * 256u;
            if (nb) {
                const uint4 *src = reinterpret_cast<const uint4 *>(a.rows) + P->lds_row_base * 16;
                for (uint32_t b = threadIdx.x; b < nb / 16; b += blockDim.x) cec_lds_rows[b] = src[b];
                __syncthreads();
            }
            if (!active) continue;
        }
        compute_chunk<NT, LT, Eng>(P, n_in, n_out, x, acc, lds);
        if (wide) {
            // (the LDS engine keeps non-temporal stores: the branch alone cost its encode
            // 1 %, profiles/r03_evidence/lds_engine_ab/)
            bool wt = false;
            if constexpr (!Eng::kStaged) {
                wt = (a.flags & kFlagWriteThrough) != 0;
                if constexpr (S > kNarrowStreams) wt = wt || g >= a.wt_from;  // (uniform: g is the work item)
            }
            if (wt) {
#pragma unroll
                for (int l = 0; l < LT; ++l)
                    if (l < n_out) st16_wt(out[l], pos, acc[l]);
            } else {
#pragma unroll
                for (int l = 0; l < LT; ++l)
                    if (l < n_out) st16(out[l], pos, acc[l]);
            }
        } else {
#pragma unroll
            for (int l = 0; l < LT; ++l)
                if (l < n_out) scatter16(out[l], pos, cnt, acc[l]);
        }
    }
    if constexpr (kSysRel) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope: this XCD's L2 written back
        // ... and completed before the wave ends (the fence alone leaves the wait to a
        // following store, and there is none)
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}

// ---------------------------------------------------------------- the scrub kernel
// cec_scrub: the read side of combine_kernel with every output read-modify-write, and no
// write side.  Per tile it reads the k data streams and LT parity streams and forms the
// syndromes S_l = P_l ^ sum_j coef[l][j] * D_j in registers.  A wave whose syndromes are
// all zero (one ballot) ends there: no store, no atomic, a pure read stream.  Otherwise
// (wave-uniform, rare) it reports into the tile's word:
//   bits [0, 8)  : parity syn_shift + l has a non-zero syndrome somewhere in the wave;
//   bits [8, 24) : data lid j cannot be the single corrupt shard: ratio[q][j] * S_0 != S_q
//                  in some byte, for some q >= 1 (ratio[q][j] = coef[q][j] / coef[0][j]);
// and counts the tile once (the first wave that sets a syndrome bit of the word).
// PERM engine only: no LDS staging, no barrier.  One workgroup per (part of a) tile: the
// host refuses a run over more tiles than one dispatch holds, so there is no grid-stride.
struct ScrubArgs {
    const uint8_t *base[kScrubStreams];  // [0, k): data; [k, k + n_out): this launch's parities
    const Tile *tiles;                   // NULL: implicit region [0, implicit_len)
    const Pattern *pattern;              // [0]: coefficients (n_in = k, n_out); [1]: ratio tables
    uint32_t *words;                     // one report word per tile
    uint32_t *counter;                   // flagged tiles
    uint64_t implicit_len;
    uint32_t n_tiles;
    uint32_t split_shift;
    uint32_t grid;
    uint32_t syn_shift;                  // index of the launch's first parity (its syndrome bit)
};

template <int NT, int LT, bool kExact>
__global__ __launch_bounds__(kBlock) void scrub_kernel(ScrubArgs a) {
    const uint32_t sh = a.split_shift;
    const uint32_t g = blockIdx.x;
    if (g >= a.grid) return;
    const uint32_t t = g >> sh;
    const uint32_t part = g & ((1u << sh) - 1u);
    const uint32_t lane = (part << (kBlockLog2 - sh)) + threadIdx.x;
    const TileRef tr = load_tile(a, t);
    const CEC_CONST Pattern *P = as_const(a.pattern);
    const int n_in = kExact ? NT : P->n_in;
    const int n_out = kExact ? LT : P->n_out;

    const uint8_t *in[NT];
    const uint8_t *par[LT];
    uint64_t mis = 0;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        in[i] = nullptr;
        if (i < n_in) {
            in[i] = a.base[i] + tr.off;
            mis |= reinterpret_cast<uint64_t>(in[i]);
        }
    }
#pragma unroll
    for (int l = 0; l < LT; ++l) {
        par[l] = nullptr;
        if (l < n_out) {
            par[l] = a.base[n_in + l] + tr.off;
            mis |= reinterpret_cast<uint64_t>(par[l]);
        }
    }

    const uint32_t pos = lane * 16;
    if (pos >= tr.len) return;
    const uint32_t cnt = min(16u, tr.len - pos);
    uint4 x[NT];
    uint4 acc[LT];
    if ((mis & 15) == 0 && cnt == 16) {
#pragma unroll
        for (int i = 0; i < NT; ++i)
            if (i < n_in) x[i] = ld16(in[i], pos);
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            acc[l] = make_uint4(0, 0, 0, 0);
            if (l < n_out) acc[l] = ld16(par[l], pos);
        }
    } else {
        // bytes >= cnt read 0 in every stream, so bytes past the extent never contribute
#pragma unroll
        for (int i = 0; i < NT; ++i)
            if (i < n_in) x[i] = gather16(in[i], pos, cnt);
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            acc[l] = make_uint4(0, 0, 0, 0);
            if (l < n_out) acc[l] = gather16(par[l], pos, cnt);
        }
    }
    compute_chunk<NT, LT, PermEngine>(P, n_in, n_out, x, acc, nullptr);

    uint32_t nz[LT];
    uint32_t any = 0;
#pragma unroll
    for (int l = 0; l < LT; ++l) {
        nz[l] = acc[l].x | acc[l].y | acc[l].z | acc[l].w;  // (0 for l >= n_out)
        any |= nz[l];
    }
    if (__ballot(any != 0) == 0) return;  // the common case: a clean wave

    uint32_t w = 0;
#pragma unroll
    for (int l = 0; l < LT; ++l)
        if (l < n_out && __ballot(nz[l] != 0) != 0) w |= 1u << (a.syn_shift + l);
    if constexpr (LT >= 2) {
        if (n_out >= 2) {
            const CEC_CONST Pattern *R = P + 1;
            const PermEngine::Sel s0[4] = {PermEngine::sel(acc[0].x), PermEngine::sel(acc[0].y),
                                           PermEngine::sel(acc[0].z), PermEngine::sel(acc[0].w)};
#pragma unroll 1
            for (int j = 0; j < n_in; ++j) {
                uint32_t differ = 0;
#pragma unroll
                for (int q = 1; q < LT; ++q) {
                    if (q >= n_out) continue;
                    const CEC_CONST uint32_t *tb = R->tab[q][j];
                    differ |= (PermEngine::mul(s0[0], tb, nullptr) ^ acc[q].x) |
                              (PermEngine::mul(s0[1], tb, nullptr) ^ acc[q].y) |
                              (PermEngine::mul(s0[2], tb, nullptr) ^ acc[q].z) |
                              (PermEngine::mul(s0[3], tb, nullptr) ^ acc[q].w);
                }
                if (__ballot(differ != 0) != 0) w |= 1u << (8 + j);
            }
        }
    }
    // one report per wave, by its first active lane
    const unsigned long long live = __ballot(1);
    if (static_cast<int>(__lane_id()) == __ffsll(live) - 1) {
        const uint32_t old = atomicOr(a.words + t, w);
        if ((old & 0xFFu) == 0) atomicAdd(a.counter, 1u);
    }
}

// ---------------------------------------------------------------- the digest kernels
// cec_digest: a 32-byte GF(2^8)-linear digest of every tile of every arena, so that a
// process that holds one shard can take part in a scrub by shipping 1/128 of its bytes.
// A tile, zero-padded to 4 KiB, is 256 chunks c_0..c_255 of 16 bytes; per byte column
//     D0 = XOR_i c_i          D1 = sum_i w_i * c_i,  w_i = the field element of byte value i
// and the digest is D0 || D1 (cocytus_ec.h).  digest_kernel is a read-only reduction:
// one wave per (tile, arena), work item g = tile g / n, arena g % n, so the n arenas of a
// tile are read together as the combine kernels read them; a workgroup is 2^waves_shift
// independent waves (four by default).  No LDS, no barrier, no atomics;
// the wave's last lane writes the 32 bytes with plain stores (nothing to clear beforehand).
//   * lane L holds chunks L, L + 64, L + 128, L + 192: four coalesced global_load_dwordx4
//     (full tile, 16-B aligned base), else gather16 with the valid count: bytes past len
//     read 0 and are never fetched;
//   * in registers, with A = c0 ^ c1 ^ c2 ^ c3 (this lane's share of D0): w is GF(2)-linear
//     in the bits of i, so the lane's share of D1 is  L * A  ^  0x40 * (c1 ^ c3)  ^
//     0x80 * (c2 ^ c3)  =  L * A ^ 0x40 * ((c1 ^ c3) ^ 2 * (c2 ^ c3)).  L * x is the PERM
//     lookup (three v_perm_b32 per dword) with the lane's own tables in VGPRs, read from
//     kDigestLaneTabs (1,280 B, every wave reads the same lines); 0x40 * x the same lookup
//     with compile-time tables;
//   * what is left is a plain XOR reduction of 8 dwords over the 64 lanes: DPP inside a
//     row of 16 (quad_perm, row_ror), row_bcast15 / row_bcast31 across rows; lane 63 ends
//     with the total.
struct DigestLaneTabs {
    uint32_t w[5][64];  // w[.][L]: PermTab of coefficient L, one 256-B line per table word
};
constexpr DigestLaneTabs make_digest_lane_tabs() {
    DigestLaneTabs t{};
    for (int l = 0; l < 64; ++l) {
        const PermTab p = make_perm_tab(l);
        for (int w = 0; w < 5; ++w) t.w[w][l] = p.w[w];
    }
    return t;
}
static __device__ const DigestLaneTabs kDigestLaneTabs = make_digest_lane_tabs();

struct DigestArgs {
    const uint8_t *base[kDigestArenas];
    uint8_t *out[kDigestArenas];  // out[a] + 32 * t: digest of tile t of base[a]; 16-B aligned
    const Tile *tiles;            // NULL: implicit region [0, implicit_len)
    uint64_t implicit_len;
    uint32_t n_tiles;
    uint32_t n;                   // arenas, 1..kDigestArenas
    uint32_t n_work;              // n_tiles * n
    uint32_t waves_shift;         // 2^waves_shift waves (work items) per workgroup
};

// 2 * x on four packed bytes
__device__ inline uint32_t xtime4(uint32_t x) {
    return ((x & 0x7F7F7F7Fu) << 1) ^ (((x >> 7) & 0x01010101u) * 0x1Du);
}
// the PERM lookup with tables in registers (PermEngine::mul reads them with scalar loads)
__device__ inline uint32_t perm_mul(uint32_t x, const uint32_t (&t)[5]) {
    const PermEngine::Sel s = PermEngine::sel(x);
    return __builtin_amdgcn_perm(t[1], t[0], s.s0) ^ __builtin_amdgcn_perm(t[3], t[2], s.s1) ^
           __builtin_amdgcn_perm(t[4], t[4], s.s2);
}
// x ^ (x of the lane the DPP control names); rows outside kRowMask keep x
template <int kCtrl, int kRowMask = 0xF>
__device__ inline uint32_t dpp_xor(uint32_t x) {
    return x ^ static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), kCtrl, kRowMask, 0xF, false));
}
// XOR over the wave's 64 lanes; the total is in lane 63 (every lane must be active)
__device__ inline uint32_t wave_xor_to_last(uint32_t x) {
    x = dpp_xor<0xB1>(x);        // quad_perm [1,0,3,2]
    x = dpp_xor<0x4E>(x);        // quad_perm [2,3,0,1]
    x = dpp_xor<0x124>(x);       // row_ror:4
    x = dpp_xor<0x128>(x);       // row_ror:8: every lane holds its row's total
    x = dpp_xor<0x142, 0xA>(x);  // row_bcast15: rows 1, 3 ^= rows 0, 2
    x = dpp_xor<0x143, 0xC>(x);  // row_bcast31: row 3 ^= row 1
    return x;
}
// The digest of the unit whose chunks lane, lane + 64, lane + 128, lane + 192 this lane holds
// in c[0..3]: the lane's shares of D0 and D1, then the wave's XOR; lane 63 ends with d[0..8).
__device__ inline void digest_wave_total(const uint4 (&c)[4], uint32_t lane, uint32_t (&d)[8]) {
    uint32_t tab[5];
#pragma unroll
    for (int w = 0; w < 5; ++w) tab[w] = kDigestLaneTabs.w[w][lane];
    constexpr PermTab k40 = make_perm_tab(0x40);
    const uint32_t t40[5] = {k40.w[0], k40.w[1], k40.w[2], k40.w[3], k40.w[4]};

    const uint32_t cw[4][4] = {{c[0].x, c[0].y, c[0].z, c[0].w}, {c[1].x, c[1].y, c[1].z, c[1].w},
                               {c[2].x, c[2].y, c[2].z, c[2].w}, {c[3].x, c[3].y, c[3].z, c[3].w}};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t hi6 = cw[1][w] ^ cw[3][w];  // chunks whose index has bit 6
        const uint32_t hi7 = cw[2][w] ^ cw[3][w];  // ... bit 7
        const uint32_t A = cw[0][w] ^ cw[2][w] ^ hi6;
        d[w] = A;
        d[4 + w] = perm_mul(A, tab) ^ perm_mul(hi6 ^ xtime4(hi7), t40);
    }
#pragma unroll
    for (int w = 0; w < 8; ++w) d[w] = wave_xor_to_last(d[w]);
}

__global__ __launch_bounds__(kBlock) void digest_kernel(DigestArgs a) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t g = (blockIdx.x << a.waves_shift) + wave;
    if (g >= a.n_work) return;  // (wave-uniform)
    const uint32_t t = g / a.n;
    const uint32_t ar = g - t * a.n;
    const uint32_t lane = threadIdx.x & 63u;
    const TileRef tr = load_tile(a, t);
    const uint8_t *in = a.base[ar] + tr.off;

    uint4 c[4];
    if ((reinterpret_cast<uint64_t>(in) & 15) == 0 && tr.len == kTile) {
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = ld16(in, (lane + 64u * j) * 16u);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t pos = (lane + 64u * j) * 16u;
            c[j] = make_uint4(0, 0, 0, 0);
            if (pos < tr.len) c[j] = gather16(in, pos, min(16u, tr.len - pos));
        }
    }
    uint32_t tab[5];
#pragma unroll
    for (int w = 0; w < 5; ++w) tab[w] = kDigestLaneTabs.w[w][lane];
    constexpr PermTab k40 = make_perm_tab(0x40);
    const uint32_t t40[5] = {k40.w[0], k40.w[1], k40.w[2], k40.w[3], k40.w[4]};

    const uint32_t cw[4][4] = {{c[0].x, c[0].y, c[0].z, c[0].w}, {c[1].x, c[1].y, c[1].z, c[1].w},
                               {c[2].x, c[2].y, c[2].z, c[2].w}, {c[3].x, c[3].y, c[3].z, c[3].w}};
    uint32_t d[8];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t hi6 = cw[1][w] ^ cw[3][w];  // chunks whose index has bit 6
        const uint32_t hi7 = cw[2][w] ^ cw[3][w];  // ... bit 7
        const uint32_t A = cw[0][w] ^ cw[2][w] ^ hi6;
        d[w] = A;
        d[4 + w] = perm_mul(A, tab) ^ perm_mul(hi6 ^ xtime4(hi7), t40);
    }
#pragma unroll
    for (int w = 0; w < 8; ++w) d[w] = wave_xor_to_last(d[w]);
    if (lane == 63) {
        CEC_GLOBAL u32x4 *o = (CEC_GLOBAL u32x4 *)((uintptr_t)a.out[ar] + static_cast<uint64_t>(t) * kDigestBytes);
        u32x4 v0, v1;
        v0.x = d[0]; v0.y = d[1]; v0.z = d[2]; v0.w = d[3];
        v1.x = d[4]; v1.y = d[5]; v1.z = d[6]; v1.w = d[7];
        o[0] = v0;
        o[1] = v1;
    }
}

// cec_digest_apply_diffs: keep a live digest array current.  The digest is linear, so a diff
// that is XORed into an arena (times a coefficient) is folded into the arena's digests as
//     digests[off >> 12] ^= coef * digest(a unit, zero but for the diff bytes at off & 4095).
// digest_update_kernel is digest_kernel's reduction over a diff placed in its unit: one wave
// per tile (a tile never crosses a 4 KiB arena boundary), four waves per workgroup, no LDS,
// no barrier.
//   * lane L holds UNIT chunks L, L + 64, L + 128, L + 192.  A chunk that lies inside the
//     tile is one global_load_dwordx4 when the diff's address is 16-B aligned with the arena
//     offset (ecalloc's offsets: every chunk of the tile but a ragged last one); a chunk the
//     tile covers in part, or at any other alignment, is the byte gather over the covered
//     bytes only; a chunk outside the tile is zero.  Bytes outside the tile are never fetched;
//   * the wave's 32-byte total (digest_wave_total) is spread over lanes 0..7, one dword each,
//     multiplied there by the tile's coefficient (pattern [0]: coef[0][j] / tab[0][j] of source
//     lid j, scalar loads; a tile whose coefficient is 0 returns before it reads anything),
//   * and XORed into the live digest by ONE wave instruction: a no-return global_atomic_xor
//     of eight lanes on the 32 contiguous bytes, relaxed, agent scope.  Sixteen 256-byte values
//     share a unit, so several waves of a launch meet in one digest; XOR commutes, so the
//     bytes are the same in any order, overlapping extents included.
struct DigestUpdateArgs {
    const uint8_t *diffs;    // tiles' src_off count from here
    uint8_t *digests;        // unit u at digests + 32 * u; 16-B aligned
    const Tile *tiles;
    const Pattern *pattern;  // [0]: coef[0][j], tab[0][j] = MATRIX(lid_self, j) for source lid j
    uint32_t n_tiles;
};

// Bytes [first, first + cnt) of the 16-byte chunk at base + off (cnt >= 1, first + cnt <= 16);
// the other bytes read 0.  gather16's scheme: byte b reads the address of the nearest
// covered byte, so all 16 loads are in bounds and in flight together.
__device__ inline uint4 gather16_at(const uint8_t *base, uint32_t off, uint32_t first, uint32_t cnt) {
    uint32_t v[16];
#pragma unroll
    for (int b = 0; b < 16; ++b)
        v[b] = ld8(base, off + min(max(static_cast<uint32_t>(b), first), first + cnt - 1));
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < 16; ++b) w[b >> 2] |= (static_cast<uint32_t>(b) - first < cnt ? v[b] : 0u) << (8 * (b & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(kBlock) void digest_update_kernel(DigestUpdateArgs a) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t t = (blockIdx.x << 2) + wave;
    if (t >= a.n_tiles) return;  // (wave-uniform)
    const CEC_CONST Tile *tl = as_const(a.tiles) + t;
    const uint64_t off = tl->off;
    const uint32_t len = tl->len;
    const uint32_t src = tl->pattern;
    const CEC_CONST Pattern *P = as_const(a.pattern);
    if (P->coef[0][src] == 0) return;  // another shard's diff: nothing read
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lo = static_cast<uint32_t>(off) & (kTile - 1u), hi = lo + len;  // the tile in its unit
    // where unit byte 0 would lie in the diffs: only bytes [lo, hi) of it are addressed
    const uint8_t *unit = a.diffs + tl->src_off - lo;
    const bool aligned = (reinterpret_cast<uint64_t>(unit) & 15) == 0;

    uint4 c[4];
    if (aligned && len == kTile) {
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = ld16(unit, (lane + 64u * j) * 16u);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t pos = (lane + 64u * j) * 16u;
            const uint32_t b0 = max(pos, lo), b1 = min(pos + 16u, hi);  // covered bytes of the chunk
            c[j] = make_uint4(0, 0, 0, 0);
            if (b0 < b1) c[j] = aligned && b1 - b0 == 16u ? ld16(unit, pos) : gather16_at(unit, pos, b0 - pos, b1 - b0);
        }
    }
    uint32_t d[8];
    digest_wave_total(c, lane, d);
    uint32_t v = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        const uint32_t total = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(d[w]), 63));
        v = lane == static_cast<uint32_t>(w) ? total : v;
    }
    if (lane < 8) {
        v = PermEngine::mul(PermEngine::sel(v), P->tab[0][src], nullptr);
        CEC_GLOBAL uint32_t *o = (CEC_GLOBAL uint32_t *)((uintptr_t)a.digests + (off >> 12) * kDigestBytes) + lane;
        __hip_atomic_fetch_xor(o, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// cec_digest_set: the live digests of a group kept current through the SET path, where the
// diff is never stored: it is formed here from its two sources, d = new ^ old, and its ONE
// digest is scattered to every array the SET changes,
//     data_digests[j][u] ^= D        parity_digests[p][u] ^= MATRIX(k+p, j) * D.
// digest_update_kernel's form: one wave per tile, four waves per workgroup, no LDS, no barrier.
//   * lane L holds unit chunks L, L + 64, L + 128, L + 192 of d.  The new value is addressed
//     from staging with the tile's src_off, the old bytes from data[j] with its arena offset;
//     the two have independent alignment, so each source on its own takes one
//     global_load_dwordx4 for a chunk that lies wholly inside the tile (16-B aligned address)
//     or the byte gather over the covered bytes.  A chunk outside the tile is zero, and bytes
//     outside the tile are never fetched from either source;
//   * the wave's 32-byte total (digest_wave_total) is spread over ALL eight-lane groups, lane
//     L holding dword L & 7; group L >> 3 serves destination slot L >> 3: slot 0 the data lid
//     (coefficient 1), slot 1 + p parity p (patterns[p / 4]: coef[p % 4][j] / tab[p % 4][j],
//     scalar loads; the multiply is a wave-uniform loop over the live slots with a per-lane
//     select, 3 v_perm_b32 per slot);
//   * ONE no-return global_atomic_xor, relaxed, agent scope, then carries eight slots, 32
//     contiguous bytes per slot (RS(3,2): 24 active lanes); a ninth slot (m = 8 with the data
//     digest) takes a second one.  A slot whose digest pointer is NULL or whose coefficient is
//     0 is masked out; a tile with no slot left returns before it reads anything.
struct DigestSetArgs {
    const uint8_t *data[kPatN];         // data arenas: tiles' off counts from data[pattern]
    const uint8_t *staging;             // tiles' src_off count from here
    uint8_t *digests[kDigestArenas];    // [0, k): data lids; [k, k + m): parities; NULL: not kept
    const Tile *tiles;
    const Pattern *patterns;            // [p / 4]: coef / tab[p % 4][j] = MATRIX(k + p, j)
    uint32_t n_tiles;
    uint32_t k, m;
};

// Chunk `pos` of a unit whose byte 0 would lie at `unit`: its covered bytes [b0, b1) only.
__device__ inline uint4 ld_covered(const uint8_t *unit, bool aligned, uint32_t pos, uint32_t b0, uint32_t b1) {
    return aligned && b1 - b0 == 16u ? ld16(unit, pos) : gather16_at(unit, pos, b0 - pos, b1 - b0);
}

__global__ __launch_bounds__(kBlock) void digest_set_kernel(DigestSetArgs a) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t t = (blockIdx.x << 2) + wave;
    if (t >= a.n_tiles) return;  // (wave-uniform)
    const CEC_CONST Tile *tl = as_const(a.tiles) + t;
    const uint64_t off = tl->off;
    const uint32_t len = tl->len;
    const uint32_t src = tl->pattern;
    const CEC_CONST Pattern *P = as_const(a.patterns);
    // the destination slots of this tile (wave-uniform): bit 0 the data lid, bit 1 + p parity p
    uint32_t live = a.digests[src] != nullptr ? 1u : 0u;
#pragma unroll
    for (uint32_t p = 0; p < 8; ++p)  // (CEC_MAX_M)
        if (p < a.m && a.digests[a.k + p] != nullptr && P[p >> 2].coef[p & 3][src] != 0) live |= 2u << p;
    if (live == 0) return;  // nothing kept: nothing read
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lo = static_cast<uint32_t>(off) & (kTile - 1u), hi = lo + len;  // the tile in its unit
    // where unit byte 0 would lie in each source: only bytes [lo, hi) of it are addressed
    const uint8_t *nu = a.staging + tl->src_off - lo;
    const uint8_t *old = a.data[src] + off - lo;
    const bool nu_al = (reinterpret_cast<uint64_t>(nu) & 15) == 0;
    const bool old_al = (reinterpret_cast<uint64_t>(old) & 15) == 0;

    uint4 c[4];
    if (nu_al && old_al && len == kTile) {
        uint4 x[4], y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = ld16(nu, (lane + 64u * j) * 16u);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = ld16(old, (lane + 64u * j) * 16u);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = make_uint4(x[j].x ^ y[j].x, x[j].y ^ y[j].y, x[j].z ^ y[j].z, x[j].w ^ y[j].w);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t pos = (lane + 64u * j) * 16u;
            const uint32_t b0 = max(pos, lo), b1 = min(pos + 16u, hi);  // covered bytes of the chunk
            c[j] = make_uint4(0, 0, 0, 0);
            if (b0 < b1) {
                const uint4 x = ld_covered(nu, nu_al, pos, b0, b1);
                const uint4 y = ld_covered(old, old_al, pos, b0, b1);
                c[j] = make_uint4(x.x ^ y.x, x.y ^ y.y, x.z ^ y.z, x.w ^ y.w);
            }
        }
    }
    uint32_t d[8];
    digest_wave_total(c, lane, d);
    uint32_t v = 0;  // dword lane & 7 of the total, in every lane
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        const uint32_t total = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(d[w]), 63));
        v = (lane & 7u) == static_cast<uint32_t>(w) ? total : v;
    }
    const PermEngine::Sel sel = PermEngine::sel(v);
    const uint64_t at = (off >> 12) * kDigestBytes + (lane & 7u) * 4u;
#pragma unroll 1
    for (uint32_t base = 0; (live >> base) != 0; base += 8) {  // (one round; two for nine slots)
        uint32_t x = 0;
        uintptr_t to = 0;
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) {
            const uint32_t slot = base + q;  // (wave-uniform)
            if (((live >> slot) & 1u) == 0) continue;
            const uint32_t p = slot - 1u;    // the parity of a slot >= 1
            const uint32_t prod = slot == 0 ? v : PermEngine::mul(sel, P[p >> 2].tab[p & 3][src], nullptr);
            const uintptr_t dst = reinterpret_cast<uintptr_t>(a.digests[slot == 0 ? src : a.k + p]);
            const bool mine = (lane >> 3) == q;
            x = mine ? prod : x;
            to = mine ? dst : to;
        }
        if (to != 0)
            __hip_atomic_fetch_xor((CEC_GLOBAL uint32_t *)(to + at), x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// cec_encode_digests / cec_decode_digests: a combination whose launch also emits the unit
// digests of the streams it holds, so the bulk paths keep live digests without reading an
// arena twice.  The digest kernels' geometry, not combine_kernel's split: one wave per whole
// 4 KiB unit, four waves per workgroup, no LDS, no barrier, no atomics, one workgroup per
// four tiles and no grid-stride (the host refuses more tiles than one dispatch holds).
//   * lane L holds chunks L, L + 64, L + 128, L + 192 of the unit (digest_wave_total's
//     layout) of ONE input at a time: the pattern's n_in inputs are walked in a wave-uniform
//     loop, each accumulated as coef * x into the outputs' accumulators with the PERM
//     arithmetic (tables from Pattern::tab, scalar loads).  Registers: 4 uint4 of input and
//     4 uint4 per output, whatever k is; LT is the output capacity, the pattern's n_out the
//     runtime count.  Outputs are written (kModeWrite), never read;
//   * a stream on its own takes four global_load_dwordx4 / non-temporal st16 for a full unit
//     at a 16-B aligned address, else gather16 / scatter16 with the valid count: bytes past
//     the tile's len read 0, are never fetched and are never stored;
//   * every stream slot whose dig[] pointer is non-NULL, input or output, gets the digest of
//     the four chunks the lane holds of it (digest_wave_total); the wave's last lane writes
//     the 32 bytes at dig[slot] + 32 * (off >> 12) with two plain 16-byte stores, as
//     digest_kernel ends.  The bytes digested are the bytes loaded or stored, in registers.
struct CombineDigestArgs {
    uint8_t *base[kMaxStreams];
    uint8_t *dig[kMaxStreams];  // parallel to base[]: the stream's live digest array (16-B aligned); NULL: not kept
    const Tile *tiles;          // NULL: implicit region [0, implicit_len), pattern 0
    const Pattern *patterns;
    uint64_t implicit_len;
    uint32_t n_tiles;
    uint32_t in_digests;        // some input slot has a digest: a tile without outputs still reads
};

// The byte gather / scatter of a misaligned or ragged unit derives 64 byte offsets and lane
// masks from len alone.  They are the same for every stream of a tile, so the compiler would
// compute them once ahead of the input loop and hold them across it, and the full units'
// path would pay for them in registers (242 VGPRs against 60 with one output).  An opaque copy of len
// where the rare path begins keeps them local to it.
__device__ inline uint32_t rare_path(uint32_t len) {
    __asm__ volatile("" : "+s"(len));
    return len;
}
// The unit at `p`, this lane's four chunks; bytes from len on read 0 and are not fetched.
__device__ inline void load_unit(const uint8_t *p, uint32_t lane, uint32_t len, uint4 (&c)[4]) {
    if ((reinterpret_cast<uint64_t>(p) & 15) == 0 && len == kTile) {  // (wave-uniform)
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = ld16(p, (lane + 64u * j) * 16u);
    } else {
        len = rare_path(len);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t pos = (lane + 64u * j) * 16u;
            c[j] = make_uint4(0, 0, 0, 0);
            if (pos < len) c[j] = gather16(p, pos, min(16u, len - pos));
        }
    }
}
// ... and its store: the first len bytes of the unit, nothing past them.
__device__ inline void store_unit(uint8_t *p, uint32_t lane, uint32_t len, const uint4 (&c)[4]) {
    if ((reinterpret_cast<uint64_t>(p) & 15) == 0 && len == kTile) {  // (wave-uniform)
#pragma unroll
        for (int j = 0; j < 4; ++j) st16(p, (lane + 64u * j) * 16u, c[j]);
    } else {
        len = rare_path(len);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t pos = (lane + 64u * j) * 16u;
            if (pos < len) scatter16(p, pos, min(16u, len - pos), c[j]);
        }
    }
}
// The digest of the unit in c[] to dig + 32 * unit (every lane of the wave must be active).
__device__ inline void emit_digest(uint8_t *dig, uint64_t unit, const uint4 (&c)[4], uint32_t lane) {
    uint32_t d[8];
    digest_wave_total(c, lane, d);
    if (lane == 63) {
        CEC_GLOBAL u32x4 *o = (CEC_GLOBAL u32x4 *)((uintptr_t)dig + unit * kDigestBytes);
        u32x4 v0, v1;
        v0.x = d[0]; v0.y = d[1]; v0.z = d[2]; v0.w = d[3];
        v1.x = d[4]; v1.y = d[5]; v1.z = d[6]; v1.w = d[7];
        o[0] = v0;
        o[1] = v1;
    }
}

template <int LT>
__global__ __launch_bounds__(kBlock) void combine_digest_kernel(CombineDigestArgs a) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t t = (blockIdx.x << 2) + wave;
    if (t >= a.n_tiles) return;  // (wave-uniform)
    const uint32_t lane = threadIdx.x & 63u;
    const TileRef tr = load_tile(a, t);
    const CEC_CONST Pattern *P = as_const(a.patterns) + tr.pattern;
    const int n_in = P->n_in;
    const int n_out = min(P->n_out, LT);
    if (n_out == 0 && a.in_digests == 0) return;  // nothing written, nothing kept: nothing read
    const uint64_t unit = tr.off >> 12;
    // base[] and dig[] are indexed by a slot the pattern names: read them from the kernarg
    // segment with scalar loads (indexing the by-value copy selects among all 96 pointers)
    const CEC_CONST CombineDigestArgs *ka = (const CEC_CONST CombineDigestArgs *)__builtin_amdgcn_kernarg_segment_ptr();

    uint4 acc[LT][4];
#pragma unroll
    for (int l = 0; l < LT; ++l)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[l][j] = make_uint4(0, 0, 0, 0);

#pragma unroll 1
    for (int i = 0; i < n_in; ++i) {
        const int slot = P->in_stream[i];
        uint4 c[4];
        load_unit(ka->base[slot] + (P->in_src[i] ? tr.src_off : tr.off), lane, tr.len, c);
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            if (l >= n_out) continue;
            const int cf = P->coef[l][i];
            if (cf == 0) continue;
            const CEC_CONST uint32_t *tb = P->tab[l][i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (cf == 1) {
                    acc[l][j].x ^= c[j].x;
                    acc[l][j].y ^= c[j].y;
                    acc[l][j].z ^= c[j].z;
                    acc[l][j].w ^= c[j].w;
                } else {
                    acc[l][j].x ^= PermEngine::mul(PermEngine::sel(c[j].x), tb, nullptr);
                    acc[l][j].y ^= PermEngine::mul(PermEngine::sel(c[j].y), tb, nullptr);
                    acc[l][j].z ^= PermEngine::mul(PermEngine::sel(c[j].z), tb, nullptr);
                    acc[l][j].w ^= PermEngine::mul(PermEngine::sel(c[j].w), tb, nullptr);
                }
            }
        }
        uint8_t *dg = ka->dig[slot];
        if (dg != nullptr) emit_digest(dg, unit, c, lane);
    }
#pragma unroll
    for (int l = 0; l < LT; ++l) {
        if (l >= n_out) continue;
        const int slot = P->out_stream[l];
        store_unit(ka->base[slot] + (P->out_src[l] ? tr.src_off : tr.off), lane, tr.len, acc[l]);
        uint8_t *dg = ka->dig[slot];
        if (dg != nullptr) emit_digest(dg, unit, acc[l], lane);
    }
}

// cec_scrub_digests: the scrub's syndrome and ratio test on the digests.  The digest is
// linear and commutes with scalars, so digest(S_p) is the syndrome of the digests and
// digest(ratio * S_0 ^ S_q) their ratio test: the report word has cec_scrub's exact meaning
// (scrub_kernel above), and for corruption within two chunks of a tile its exact bits.
// One lane per unit: it loads the 2 x 16 bytes of the k data digests and of the launch's
// parity digests, runs compute_chunk on each half with scrub_launch's own two patterns,
// and decides alone (a wave holds 64 different units: no ballot).  Capacity shapes only.
struct DigestCheckArgs {
    const uint8_t *dig[kScrubStreams];  // [0, k): data digests; [k, k + n_out): the launch's parity digests
    const Pattern *pattern;             // [0]: coefficients; [1]: ratio tables
    uint32_t *words;
    uint32_t *counter;
    uint32_t n_units;
    uint32_t syn_shift;
};

// (default cache policy: both halves of a digest share a line)
__device__ inline uint4 ld16_cached(const uint8_t *p) {
    const u32x4 v = *(const CEC_GLOBAL u32x4 *)(uintptr_t)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}

template <int NT, int LT>
__global__ __launch_bounds__(kBlock) void digest_check_kernel(DigestCheckArgs a) {
    const uint32_t u = blockIdx.x * kBlock + threadIdx.x;
    if (u >= a.n_units) return;
    const CEC_CONST Pattern *P = as_const(a.pattern);
    const int n_in = P->n_in;
    const int n_out = P->n_out;
    const uint64_t at = static_cast<uint64_t>(u) * kDigestBytes;
    uint32_t word = 0;
#pragma unroll 1
    for (uint32_t h = 0; h < 2; ++h) {
        uint4 x[NT];
        uint4 acc[LT];
#pragma unroll
        for (int i = 0; i < NT; ++i)
            if (i < n_in) x[i] = ld16_cached(a.dig[i] + at + 16 * h);
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            acc[l] = make_uint4(0, 0, 0, 0);
            if (l < n_out) acc[l] = ld16_cached(a.dig[n_in + l] + at + 16 * h);
        }
        compute_chunk<NT, LT, PermEngine>(P, n_in, n_out, x, acc, nullptr);
        uint32_t any = 0;
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            const uint32_t nz = acc[l].x | acc[l].y | acc[l].z | acc[l].w;  // (0 for l >= n_out)
            if (nz) word |= 1u << (a.syn_shift + l);
            any |= nz;
        }
        if constexpr (LT >= 2) {
            if (any != 0 && n_out >= 2) {
                const CEC_CONST Pattern *R = P + 1;
                const PermEngine::Sel s0[4] = {PermEngine::sel(acc[0].x), PermEngine::sel(acc[0].y),
                                               PermEngine::sel(acc[0].z), PermEngine::sel(acc[0].w)};
#pragma unroll 1
                for (int j = 0; j < n_in; ++j) {
                    uint32_t differ = 0;
#pragma unroll
                    for (int q = 1; q < LT; ++q) {
                        if (q >= n_out) continue;
                        const CEC_CONST uint32_t *tb = R->tab[q][j];
                        differ |= (PermEngine::mul(s0[0], tb, nullptr) ^ acc[q].x) |
                                  (PermEngine::mul(s0[1], tb, nullptr) ^ acc[q].y) |
                                  (PermEngine::mul(s0[2], tb, nullptr) ^ acc[q].z) |
                                  (PermEngine::mul(s0[3], tb, nullptr) ^ acc[q].w);
                    }
                    if (differ) word |= 1u << (8 + j);
                }
            }
        }
    }
    if (word & 0xFFu) {
        const uint32_t old = atomicOr(a.words + u, word);
        if ((old & 0xFFu) == 0) atomicAdd(a.counter, 1u);
    }
}

}  // namespace cec
