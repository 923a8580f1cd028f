// frame_layout_main.cpp -- gswt_frame_layout.h (the frame's device bookkeeping: counter block, sort count, radix workspace, super-group sums,
// tile ranges) as a stand-alone host program, for tests/test_frame_layout_cpu.py:
//   g++ -std=c++17 -O1 -Wall -Wextra -Werror -I gswt_renderer_amd/csrc tools/frame_layout_main.cpp -o frame_layout
// It prints one line per layout, a tag and then key=value fields:
//   counters   size and byte offset of every field of FrameCounters, the result's size and 64-bit word count
//   sortcount  size and offsets of SortCount; n / refused read through the view of a block with n_pairs = 123456789012, rerun = 7
//   radix      per (n_cap, key_bits) of the list below: nblk, nsup, passes, zero, total, and per pass gsup / gtot / ghist
//   super      per n_chunks: n_super, words, and pair / visible / prefix word of j = 0, 1, 5
//   live       count and copy word of lists 0 and 3, the table's words
//   range      (start, end) -> words -> decoded
#include <cstdio>
#include <initializer_list>

#include "gswt_frame_layout.h"

using namespace gswt;

int main()
{
    std::printf("counters size=%zu n_visible=%zu n_pairs=%zu depth_passes_needed=%zu max_tile_len=%zu rerun=%zu live_longest=%zu krange=%zu reserved=%zu "
                "result_size=%zu result_words64=%u counter_words=%u\n",
                sizeof(FrameCounters), offsetof(FrameCounters, res) + offsetof(FrameResult, n_visible), offsetof(FrameCounters, res) + offsetof(FrameResult, n_pairs),
                offsetof(FrameCounters, res) + offsetof(FrameResult, depth_passes_needed), offsetof(FrameCounters, res) + offsetof(FrameResult, max_tile_len),
                offsetof(FrameCounters, res) + offsetof(FrameResult, rerun), offsetof(FrameCounters, res) + offsetof(FrameResult, live_longest),
                offsetof(FrameCounters, krange), offsetof(FrameCounters, reserved), sizeof(FrameResult), kFrameResultWords64, kFrameCounterWords);

    FrameCounters blk{};
    blk.res.n_visible = 1ull; blk.res.n_pairs = 123456789012ull; blk.res.depth_passes_needed = 3u; blk.res.max_tile_len = 4u; blk.res.rerun = 7ull;
    blk.res.live_longest = 5ull;
    const SortCount* const view = sort_count_of(&blk);
    const SortCount staged = sort_count(42ull, true), plain = sort_count(43ull);
    std::printf("sortcount size=%zu n=%zu refused=%zu view_n=%llu view_refused=%llu staged_n=%llu staged_refused=%llu plain_n=%llu plain_refused=%llu\n",
                sizeof(SortCount), offsetof(SortCount, n), offsetof(SortCount, refused), view->n, view->refused, staged.n, staged.refused, plain.n,
                plain.refused);
    FrameResult back{};
    for (uint32_t i = 0; i < kFrameResultWords64; i++) copy_frame_result_word(&back, &blk, i);
    std::printf("result n_visible=%llu n_pairs=%llu depth_passes_needed=%u max_tile_len=%u rerun=%llu live_longest=%llu\n", back.n_visible, back.n_pairs,
                back.depth_passes_needed, back.max_tile_len, back.rerun, back.live_longest);

    const struct { uint32_t n_cap; int key_bits; } sorts[] = {{1u, 1}, {4096u, 8}, {4097u, 9}, {131072u, 32}, {131073u, 16}, {131073u, 0}};
    for (const auto& q : sorts) {
        const RadixWs w = radix_ws_of(q.n_cap, q.key_bits);
        std::printf("radix n_cap=%u key_bits=%d nblk=%u nsup=%u passes=%d zero=%zu total=%zu", q.n_cap, q.key_bits, w.nblk, w.nsup, w.passes, w.zero_words(),
                    w.words());
        for (int p = 0; p < w.passes; p++) std::printf(" gsup%d=%zu gtot%d=%zu ghist%d=%zu", p, w.gsup(p), p, w.gtot(p), p, w.ghist(p));
        std::printf("\n");
    }

    for (uint32_t n_chunks : {0u, 255u, 256u, 1000u}) {
        const SuperSums ss = super_sums_of(n_chunks);
        std::printf("super n_chunks=%u n_super=%u words=%zu", n_chunks, ss.n_super, ss.words());
        for (uint32_t j : {0u, 1u, 5u}) std::printf(" pair%u=%u visible%u=%u prefix%u=%u", j, ss.pair_word(j), j, ss.visible_word(j), j, ss.prefix_word(j));
        std::printf(" super_of_last=%u\n", super_of_chunk(n_chunks ? n_chunks - 1u : 0u));
    }

    std::printf("live count0=%u count3=%u copy0=%u copy3=%u words=%u lists=%u\n", live_count_word(0), live_count_word(3), live_copy_word(0), live_copy_word(3),
                kLiveTableWords, kLiveLists);

    const uint32_t ranges[][2] = {{3u, 7u}, {0u, 0u}, {0u, 1u}, {5u, 5u}, {0xFFFFFF00u, 0xFFFFFFFFu}};
    for (const auto& r : ranges) {
        uint32_t x, y, start, end;
        encode_tile_range(r[0], r[1], x, y);
        decode_tile_range(x, y, start, end);
        std::printf("range start=%u end=%u x=%u y=%u dec_start=%u dec_end=%u start_word=%u\n", r[0], r[1], x, y, start, end, tile_range_start_word(r[0]));
    }
    std::printf("krange min_word_of_9=%u back=%u\n", krange_min_word(9u), krange_min_word(krange_min_word(9u)));
    return 0;
}
