// gswt_frame_layout.h -- the device bookkeeping of a frame, laid out once for the kernels of the frame chain (gswt_kernels.hip), the host that
// plans, launches and reads it (gswt_api*.hip, gswt_worker.hip) and the test hooks: the counter block, the radix sort's count record and
// workspace, k_project's super-group sums, the live-chunk count table and the per-tile range words.  THE place that knows where a word lies:
// no other file indexes these regions by a literal or splits one of their words.
// Free of HIP: <cstddef> and <cstdint> are all it needs (tools/frame_layout_main.cpp compiles it with the host compiler alone).  GSWT_HD as in
// host/gswt_math.h: empty for a host compiler; gswt_device.h includes this header with it set to __host__ __device__.
#pragma once
#ifndef GSWT_HD
#define GSWT_HD
#endif
#include <cstddef>
#include <cstdint>

namespace gswt {

// ---- the frame's counter block: 64 bytes at the head of the `ghist` region, zeroed by k_cull ---------------------------------------------
// Byte offsets, and the 64-bit word each field had as `counters[i]`:
//    0  [0]     n_visible            visible splats of the frame (k_totals)
//    8  [1]     n_pairs              (tile, slot) pairs of the frame, in 64 bits (k_totals): the pair sort's item count
//   16  [2] lo  depth_passes_needed  8-bit passes the frame's depth key range needs (k_items; GSWT_ORDER_DEPTH, global passes)
//   20  [2] hi  max_tile_len         longest per-tile pair list (k_items, atomicMax; GSWT_ORDER_DEPTH)
//   24  [3]     rerun                nonzero: the frame is incomplete and the host runs it again -- pair buffers too small (k_totals, k_emit),
//                                    launch grid shorter than a live list (k_totals), fewer depth passes than needed (k_items); the sort
//                                    kernels then see no items at all (SortCount::refused)
//   32  [4]     live_longest         longest of the eight live-chunk lists (k_totals): the host sizes the next frames' launch grids by it
//   40  [5]     krange[2]            depth key range, (~smallest, largest), both raised by atomicMax (k_emit<DEPTH>; load_krange)
//   48  [6..7]  reserved
// The fields up to live_longest are the frame's RESULT: k_combine (or, for a frame without screen tiles, a copy) hands them to the slot's
// pinned host words (FrameSlot::hc), where finish_frame reads them.
struct FrameResult {
    unsigned long long n_visible, n_pairs;
    uint32_t depth_passes_needed, max_tile_len;
    unsigned long long rerun, live_longest;
};
struct FrameCounters {
    FrameResult res;
    uint32_t krange[2];
    unsigned long long reserved[2];
};
constexpr uint32_t kFrameCounterWords = (uint32_t)(sizeof(FrameCounters) / sizeof(uint32_t));                  // u32 words of the block in `ghist`
constexpr uint32_t kFrameResultWords64 = (uint32_t)(sizeof(FrameResult) / sizeof(unsigned long long));         // 64-bit words that travel back
static_assert(sizeof(FrameCounters) == 64 && kFrameCounterWords == 16, "the counter block is one cache line");
static_assert(sizeof(FrameResult) == 40 && kFrameResultWords64 == 5, "five 64-bit words travel back to the host");
static_assert(offsetof(FrameCounters, res) == 0 && offsetof(FrameResult, n_visible) == 0 && offsetof(FrameResult, n_pairs) == 8, "counter word map");
static_assert(offsetof(FrameResult, depth_passes_needed) == 16 && offsetof(FrameResult, max_tile_len) == 20, "counter word map");
static_assert(offsetof(FrameResult, rerun) == 24 && offsetof(FrameResult, live_longest) == 32, "counter word map");
static_assert(offsetof(FrameCounters, krange) == 40 && offsetof(FrameCounters, reserved) == 48, "counter word map");
// krange[0] holds the smallest key as this word, so that atomicMax on the zeroed block finds the minimum (its own inverse)
GSWT_HD constexpr uint32_t krange_min_word(uint32_t kmin) { return ~kmin; }
// 64-bit word i (< kFrameResultWords64) of the result, from the device's block to the host's words: k_combine's copy, a thread per word
GSWT_HD inline void copy_frame_result_word(FrameResult* dst, const FrameCounters* src, uint32_t i)
{
    reinterpret_cast<unsigned long long*>(dst)[i] = reinterpret_cast<const unsigned long long*>(&src->res)[i];
}

// ---- the radix sort's count record (clamped_count of gswt_kernels.hip) -------------------------------------------------------------------
// The sort reads its item count on the device, and a refusal word 16 bytes behind it: nonzero, or a count above the capacity the grids were
// sized for, and every sort kernel sees zero items.  The 16-byte gap is the device contract: it is what lets a frame's counter block serve
// as the record of its own pair sort, n_pairs as `n` and rerun as `refused` (sort_count_of).  Anyone else stages a record of its own.
struct SortCount {
    unsigned long long n, _pad0, refused, _pad1;
};
static_assert(sizeof(SortCount) == 32 && offsetof(SortCount, n) == 0 && offsetof(SortCount, refused) == 16, "the sort kernels' count contract");
GSWT_HD constexpr SortCount sort_count(unsigned long long n, bool refused = false) { return {n, 0ull, refused ? 1ull : 0ull, 0ull}; }
static_assert(offsetof(FrameResult, rerun) - offsetof(FrameResult, n_pairs) == offsetof(SortCount, refused) - offsetof(SortCount, n), "rerun overlays refused");
static_assert(offsetof(FrameResult, n_pairs) + sizeof(SortCount) <= sizeof(FrameCounters), "the view stays inside the block");
// the SortCount view of a frame's counter block (address arithmetic only: c may be a device pointer on the host)
GSWT_HD inline const SortCount* sort_count_of(const FrameCounters* c) { return reinterpret_cast<const SortCount*>(&c->res.n_pairs); }

// ---- the radix sort's workspace (launch_sort) ----------------------------------------------------------------------------------------------
// A sort workgroup takes kSortBlock consecutive items; workgroups come in groups of 2^kSupShift.  Per pass k_radix_hist leaves, for every
// digit d, the per-workgroup counts ghist[blk][d], their sums over each group gsup[group][d] and the digit totals gtot[d].  In u32 words:
//   [ gsup 256 x nsup | gtot 256 ] x passes      targets of atomic adds: ZERO when a sort starts (the part a frame's k_cull clears)
//   [ ghist 256 x nblk ] x passes                written in full by k_radix_hist: never cleared
constexpr int kSortBlock = 4096;
constexpr uint32_t kSupShift = 5;
struct RadixWs {
    uint32_t nblk, nsup;     // workgroups, groups of workgroups (one more than the whole ones: the sums of a partial last group)
    int passes;              // 8-bit passes over key bits [0, key_bits)
    GSWT_HD constexpr size_t pass_zero_words() const { return (size_t)256 * nsup + 256; }
    GSWT_HD constexpr size_t zero_words() const { return (size_t)passes * pass_zero_words(); }
    GSWT_HD constexpr size_t words() const { return zero_words() + (size_t)passes * 256 * nblk; }
    GSWT_HD constexpr size_t gsup(int pass) const { return (size_t)pass * pass_zero_words(); }
    GSWT_HD constexpr size_t gtot(int pass) const { return gsup(pass) + (size_t)256 * nsup; }
    GSWT_HD constexpr size_t ghist(int pass) const { return zero_words() + (size_t)pass * 256 * nblk; }
};
GSWT_HD constexpr RadixWs radix_ws_of(uint32_t n_cap, int key_bits)
{
    const uint32_t nblk = (n_cap + kSortBlock - 1) / kSortBlock;
    return {nblk, (nblk >> kSupShift) + 1u, (key_bits + 7) / 8};
}

// ---- k_project's super-group sums ----------------------------------------------------------------------------------------------------------
// Two-level sums: one word per super-group (256 chunks) for the pairs and one for the visible splats, each on a cache line of its own
// (kSuperStride words apart), then k_totals' exclusive prefix of the pair words, side by side.  Device-scope atomics on one 64-byte line
// retire at ~10 ns each whichever XCD they come from (measured: 43 k atomics on 4 lines = +125 us), and side by side the 64 super-group words
// of c3 were 4 + 4 lines taking 2.7 k atomics each.  Zeroed by k_cull.
constexpr uint32_t kSuperStride = 16;
constexpr uint32_t kSuperShift = 8;              // chunks per super-group, as a shift
struct SuperSums {
    uint32_t n_super;
    GSWT_HD constexpr size_t words() const { return (2 * (size_t)kSuperStride + 1) * n_super; }
    GSWT_HD constexpr uint32_t pair_word(uint32_t j) const { return j * kSuperStride; }
    GSWT_HD constexpr uint32_t visible_word(uint32_t j) const { return (n_super + j) * kSuperStride; }
    GSWT_HD constexpr uint32_t prefix_word(uint32_t j) const { return 2u * kSuperStride * n_super + j; }
};
GSWT_HD constexpr uint32_t super_of_chunk(uint32_t chunk) { return chunk >> kSuperShift; }
// (one more than the whole super-groups: n_chunks = 0 still has a word to clamp loads to)
GSWT_HD constexpr SuperSums super_sums_of(uint32_t n_chunks) { return {super_of_chunk(n_chunks) + 1u}; }

// ---- the live-chunk count table --------------------------------------------------------------------------------------------------------------
// One row (a cache line, kSuperStride words) per count.  Rows 0..7: entries of each XCD's list of live chunks (k_cull adds, k_project reads,
// k_totals clears them for the slot's next frame); rows 8..15: k_totals' copy of them, which k_emit walks by.
constexpr uint32_t kLiveLists = 8;
GSWT_HD constexpr uint32_t live_count_word(uint32_t x) { return x * kSuperStride; }
GSWT_HD constexpr uint32_t live_copy_word(uint32_t x) { return (kLiveLists + x) * kSuperStride; }
constexpr uint32_t kLiveTableWords = 2u * kLiveLists * kSuperStride;

// ---- the per-tile ranges of the sorted pair list -----------------------------------------------------------------------------------------------
// A tile's pairs are [start, end) of the sorted list, kept as the words (~start, end): the last sort pass raises both by atomicMax on the
// zeroed table (a tile's run can continue in the next sort block, and the smallest start must win), so (0, 0) is a tile without pairs.
GSWT_HD constexpr uint32_t tile_range_start_word(uint32_t start) { return ~start; }      // (its own inverse: word -> start of a tile that has pairs)
GSWT_HD inline void encode_tile_range(uint32_t start, uint32_t end, uint32_t& x, uint32_t& y)
{
    const bool some = end > start;
    x = some ? tile_range_start_word(start) : 0u; y = some ? end : 0u;
}
// an empty tile reads as start = end = 0 (the end is its word as it stands)
GSWT_HD constexpr uint32_t tile_range_start(uint32_t x, uint32_t y) { return y ? tile_range_start_word(x) : 0u; }
GSWT_HD inline void decode_tile_range(uint32_t x, uint32_t y, uint32_t& start, uint32_t& end)
{
    start = tile_range_start(x, y); end = y;
}

}  // namespace gswt
