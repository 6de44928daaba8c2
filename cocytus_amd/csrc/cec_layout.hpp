// cec_layout.hpp -- the PODs and constants that the kernels (cec_kernels.hpp) and the host's
// launch planning (cec_launchplan.hpp) share.  Standard headers only -- no HIP type -- so the
// CPU tests include the planning, and with it this very file, under ASan + UBSan.
#pragma once

#include <stdint.h>

namespace cec {

constexpr int kTile = 4096;      // bytes per tile = kBlock lanes x 16 B
constexpr int kBlock = 256;
constexpr int kBlockLog2 = 8;
constexpr uint64_t kLineBytes = 128;  // L2 / HBM line
static_assert(kBlock == 1 << kBlockLog2, "kBlock must be a power of two");
constexpr int kMaxStreams = 48;  // 16 data + 8 parity + 16 recovered + staging/diff ...
constexpr int kPatN = 16;        // inputs per pattern (k <= CEC_MAX_K)
constexpr int kPatL = 4;         // outputs per launch pattern (host splits more)

enum : int32_t { kModeWrite = 0, kModeXor = 1 };

// One linear combination.  Lives in device memory and is read with scalar loads,
// so every field is 32-bit (gfx9 scalar loads are dword-granular).
struct alignas(16) Pattern {
    int32_t n_in;
    int32_t n_out;
    int32_t in_stream[kPatN];
    int32_t in_src[kPatN];        // 1: address with extent.src_off, 0: with extent.off
    int32_t out_stream[kPatL];
    int32_t out_src[kPatL];
    int32_t out_mode[kPatL];      // kModeWrite / kModeXor
    int32_t lds_rows;             // LDS engine: product rows this pattern stages ...
    int32_t lds_row_base;         // ... starting at row lds_row_base of CombineArgs::rows
    int32_t coef[kPatL][kPatN];
    uint32_t tab[kPatL][kPatN][5];  // PERM: PermTab; LDS: tab[..][0] = LDS byte offset of the row
};

// One tile of the work-list: a <= 4 KiB piece of one extent, same layout as
// cec_extent, so a tile is fetched with one scalar load and no indirection.
struct Tile {
    uint64_t off;      // arena offset of the piece
    uint64_t src_off;  // staging offset of the piece
    uint32_t len;      // 1 .. kTile
    uint32_t pattern;
};

// CombineArgsN::flags: every wave ends with a system-scope release (its XCD's L2 written
// back, its stores complete), for launches whose outputs the host reads on a signal
// that does not come from the runtime (the synchronous drop-in over host memory).
// Honoured by the 1 x 1 (region multiply) launches, which select the kSysRel kernel.
constexpr uint32_t kFlagSysRelease = 1u;
// CombineArgsN::flags: the wide stores write through the XCD's L2 (sc1) instead of
// non-temporal stores that keep the line there.  The host sets it for launches small
// enough that what they write is read again from the memory-side cache, or that the
// dirty lines they would leave in L2 are a visible part of the launch (DESIGN.md §4:
// the per-GPU shares of strong scaling).
constexpr uint32_t kFlagWriteThrough = 2u;
// CombineArgsN::flags, for the launch record only: the launch has a write-through tail
// (CombineArgs::wt_from names a work item).  The kernel reads wt_from, not this bit.
constexpr uint32_t kFlagWtTail = 4u;

constexpr int kNarrowStreams = 2;

// CombineArgs::wt_from of a launch without a write-through tail.
constexpr uint64_t kNoWtTail = ~uint64_t(0);

// kAcc: which outputs are read-modify-write (XOR-accumulate):
//   0 none, 1 all, 2 all but the last (diff-update + install), 3 per pattern.
enum : int { kAccNone = 0, kAccAll = 1, kAccAllButLast = 2, kAccRuntime = 3 };

constexpr int kScrubStreams = 24;  // k data slots, then the launch's parities (k + m <= 24 fit)

constexpr int kDigestBytes = 32;
constexpr int kDigestArenas = 24;  // as kScrubStreams: a whole group in one launch

}  // namespace cec
