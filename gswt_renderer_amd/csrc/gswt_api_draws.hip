// gswt_api_draws.hip -- sort events of libgswt_hip.so (host only): which draw set an event fills and when frames start reading it,
// gswt_set_draws (merged lists from the host), gswt_set_draws_merge_groups (merged lists built on the device, groups of earlier
// events copied instead of re-sorted), and the readers of what an event left.  Both entry points read top to bottom: choose the
// target set, collect the frames on it, plan the upload block, fill it, assign slots and XCDs, their own list work, upload and
// launch, record, publish.  The kernels are in gswt_kernels.hip; everything here runs on set_stream, beside the frames.
#include "gswt_ctx.h"

#include <algorithm>
#include <unordered_map>

using namespace gswt;

#define GSWT_TRY(expr)                          \
    do {                                        \
        const int _rc = (expr);                 \
        if (_rc != GSWT_OK) return _rc;         \
    } while (0)

// The merged lists the draw sets retain as copy sources belong to ONE scene and ONE set of raw depths: a re-uploaded scene of the same
// shape (same counts, other depths or gs_index values) would otherwise match the old lists by (view, member tile ids, length) from the
// second sort event on and copy the old scene's order.
void gswt::invalidate_merge_sources(gswt_ctx* c)
{
    for (auto& ds : c->sets) { ds.g_valid = false; ds.g_desc.clear(); ds.g_members.clear(); ds.src_mask = 0; }
}

// Frames still in flight on draw set `set` are run to completion before that set is refilled.
// host_upload: the refill writes the set's merged arrays with copies that are NOT ordered on the build stream (gswt_set_draws with host
// lists), so a device-side build of another set that is still copying from them has to be waited for; a refill on the build stream
// (gswt_set_draws_merge_groups) is ordered behind such a copy anyway.
static void collect_set(gswt_ctx* c, int set, bool host_upload)
{
    for (auto& sl : c->slots)
        if (sl.set == set) collect_slot(c, sl);
    // ... and no device-side list build still in flight may be COPYING from this set's merged arrays (the lists of the last sort events
    // stay addressable as copy sources): everything that refills the set on the build stream is ordered behind such a copy anyway, a
    // host-side upload (gswt_set_draws with host lists) is not
    if (!host_upload) return;
    for (int k = 0; k < kDrawSets; k++) {
        DrawSet& o = c->sets[k];
        if (k != set && o.ev_up_pending && ((o.src_mask >> set) & 1u)) { (void)hipEventSynchronize(o.ev_up); o.ev_up_pending = false; }
    }
}

// The set the next sort event fills (when frames start reading it: activate_pending, gswt_ctx.h).  The new list goes into a draw set
// that is not current; the frames in flight keep the set they were submitted with (only a frame still running on the set being
// refilled is waited for, collect_set), so a sort event does not drain the frame pipeline.
static int next_target(gswt_ctx* c)
{
    activate_pending(c, true);
    return c->draws_ready ? (c->latest_set + 1) % kDrawSets : c->cur_set;
}
static void publish_set(gswt_ctx* c, int target)
{
    const bool first = !c->draws_ready || target == c->cur_set;
    c->latest_set = target;
    if (c->opt.defer_swap && !first) { c->pending_set = target; c->pending_frames = c->opt.defer_swap - 1; }
    else { c->cur_set = target; c->pending_set = -1; }
    c->draws_ready = true;
}

static int check_draw_list(gswt_ctx* c, const gswt_draw* draws, int n_draws)
{
    if (!c->scene_ready) return fail(c, GSWT_ERR_STATE, "gswt_set_draws before gswt_upload_scene");
    if (n_draws < 0 || (n_draws > 0 && !draws)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_draws: bad draw list");
    return GSWT_OK;
}

// the set's pinned staging is free again once its previous upload has been consumed
static int staging_ready(gswt_ctx* c, DrawSet& D)
{
    if (D.ev_up_pending) { HIP_TRY(c, hipEventSynchronize(D.ev_up)); D.ev_up_pending = false; }
    if (!D.ev_up) HIP_TRY(c, hipEventCreateWithFlags(&D.ev_up, hipEventDisableTiming));
    return GSWT_OK;
}

// The draw records, from gswt_draw[] into the set's staging: a merged draw reads [merged_offset, + merged_count) of the event's
// n_merged merged entries, a static draw one of the scene's base lists (LOD-filtered where the draw's own LOD is all it keeps).
// have_lod_ids: a merged draw with merged_has_lod finds its lod ids (the device-side build writes them itself).  *entries: the
// list entries of all draws, entry_base of each being the sum in front of it.
static int fill_draw_records(gswt_ctx* c, DrawSet& D, const gswt_draw* draws, int n_draws, size_t n_merged, bool have_lod_ids, uint64_t* entries_out)
{
    DrawDev* const dd = D.hp<DrawDev>(D.off_draws);
    uint64_t entries = 0;
    for (int i = 0; i < n_draws; i++) {
        const gswt_draw& g = draws[i];
        DrawDev& d = dd[i];
        memset(&d, 0, sizeof(d));
        d.single_draw = g.tile.single_draw;
        d.valid_lod_id = g.tile.valid_lod_id;
        d.changing = g.tile.changing;
        d.changing_to_lower = g.tile.changing_to_lower;
        d.tile_lod = g.tile.tile_id[0];
        d.tile_idx = g.tile.tile_id[1]; d.tile_view = g.tile.tile_id[2];
        d.single_lod_id = g.tile.single_lod_id;
        d.map_coord[0] = g.tile.map_coord[0]; d.map_coord[1] = g.tile.map_coord[1];
        d.map_index = g.tile.map_index;
        d.off[0] = g.tile.offset[0]; d.off[1] = g.tile.offset[1]; d.off[2] = g.tile.offset[2];
        d.cull_enable = g.cull_enable;
        d.lod = g.lod;
        memcpy(d.corners, g.corners, sizeof(d.corners));
        if (g.merged) {
            if ((size_t)g.merged_offset + g.merged_count > n_merged)
                return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_draws: draw %d merged range out of bounds", i);
            if (g.merged_has_lod && !have_lod_ids)
                return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_draws: draw %d needs merged_lod_id", i);
            if (g.tile.single_draw != 1u) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_draws: merged draw %d without single_draw", i);
            d.merged = 1; d.list_base = g.merged_offset; d.count = g.merged_count; d.box_base = 0xFFFFFFFFu;
        } else {
            if (g.tile.single_draw == 1u) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_draws: single_draw on static draw %d", i);
            if ((int)g.base_lod >= c->n_lod || (int)g.base_tile >= c->n_tile || (int)g.base_view >= c->n_view)
                return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_draws: draw %d base list (%u,%u,%u) out of range", i, g.base_lod,
                            g.base_tile, g.base_view);
            const ListRef& L = c->lists[((size_t)g.base_lod * c->n_tile + g.base_tile) * c->n_view + g.base_view];
            const bool prefilter = !c->opt.no_prefilter && g.tile.valid_lod_id >= 0 && (uint32_t)g.tile.valid_lod_id == g.base_lod;
            d.merged = 0;
            d.list_base = prefilter ? L.self_base : L.pair_base;
            d.count = prefilter ? L.self_count : L.pair_count;
            d.box_base = prefilter ? L.self_box : L.pair_box;
        }
        d.entry_base = (uint32_t)entries;
        entries += d.count;
    }
    if (entries >= 0xFFFFFF00ull) return fail(c, GSWT_ERR_CAPACITY, "gswt_set_draws: %llu list entries exceed 2^32", (unsigned long long)entries);
    *entries_out = entries;
    return GSWT_OK;
}

// composite-order slots: the LAST draw is nearest (drawn last = on top), so it gets the lowest slots.  A chunk = 256 list
// entries of one draw; chunk c of the frame = slot c * 256.  The two chunk tables (slot order; k_project's launch order:
// per-XCD lists, a draw's XCD = DrawDev::xcd, interleaved so that position p runs on XCD p % 8) are written on the DEVICE from the
// draw records (k_chunk_tabs): the host only sums the O(#draws) counts, and a sort event uploads O(#draws) bytes.
// Leaves slot_base / xcd in the staged records, xcd_first beside them, per_xcd / longest / n_launch in the set, and the two chunk
// tables sized; *n_chunks_out: the chunks of the draw list.
static int assign_slots(gswt_ctx* c, DrawSet& D, int n_draws, size_t* n_chunks_out)
{
    DrawDev* const dd = D.hp<DrawDev>(D.off_draws);
    uint32_t* const h_xcd_first = D.hp<uint32_t>(D.off_xcd);
    uint64_t slot = 0, per_xcd[8] = {};
    for (int i = n_draws - 1; i >= 0; i--) {
        DrawDev& d = dd[i];
        d.slot_base = (uint32_t)slot;
        const uint32_t nch = (d.count + kChunk - 1) / kChunk;
        // all chunks of a draw on one XCD (its gathers stay in that XCD's L2): the least loaded one.  (draw % 8 until round 4: a few merged
        // groups of ~190 chunks each made the longest of the eight lists 2.6 x the mean at c3 -- 42.8 k launch positions for 16.3 k chunks,
        // and every position past an XCD's live count is a workgroup that starts, reads the count and leaves.)
        int x = 0;
        for (int q = 1; q < 8; q++) if (per_xcd[q] < per_xcd[x]) x = q;
        d.xcd = (uint32_t)x;
        h_xcd_first[i] = (uint32_t)per_xcd[x];
        per_xcd[x] += nch;
        slot += (uint64_t)nch * kChunk;
    }
    if (slot >= 0xFFFFFFFFull) return fail(c, GSWT_ERR_CAPACITY, "gswt_set_draws: slot space exceeds 2^32");
    const size_t n_chunks = (size_t)(slot / kChunk);
    size_t longest = 0;
    for (int x = 0; x < 8; x++) longest = std::max<size_t>(longest, (size_t)per_xcd[x]);
    if (longest * 8 >= 0xFFFFFFFFull) return fail(c, GSWT_ERR_CAPACITY, "gswt_set_draws: chunk table too large");
    HIP_TRY(c, D.chunk_tab.ensure_roomy(n_chunks + 1));
    HIP_TRY(c, D.chunk_tab_xcd.ensure_roomy(longest * 8 + 1));
    D.n_launch = (uint32_t)(longest * 8);
    for (int x = 0; x < 8; x++) D.per_xcd[x] = per_xcd[x];
    D.longest = longest;
    *n_chunks_out = n_chunks;
    return GSWT_OK;
}

// The set now describes this event's draw list; its merged arrays are no copy source until a device-side build says so.
static void commit_draw_list(DrawSet& D, int n_draws, size_t n_chunks, uint64_t entries)
{
    D.n_draws = (uint32_t)n_draws;
    D.n_chunks = (uint32_t)n_chunks;
    D.g_valid = false;
    D.src_mask = 0;
    D.n_entries = entries;
}

static int size_merged_arrays(gswt_ctx* c, DrawSet& D, size_t n_merged)
{
    HIP_TRY(c, D.merged_list.ensure_roomy(n_merged + 1));
    HIP_TRY(c, D.merged_map.ensure_roomy(n_merged + 1));
    D.n_merged = n_merged;
    return GSWT_OK;
}

// The one upload of the event -- the whole staged block -- and the chunk tables written from the uploaded draw records.
static int upload_block(gswt_ctx* c, DrawSet& D, int n_draws)
{
    hipStream_t s = c->set_stream;
    HIP_TRY(c, hipMemcpyAsync(D.d_blob.p, D.h_blob.p, D.blob_bytes, hipMemcpyHostToDevice, s));
    launch_chunk_tabs(s, D.draws, D.xcd_first, (uint32_t)n_draws, D.chunk_tab.p, D.chunk_tab_xcd.p, D.per_xcd, D.longest);
    return GSWT_OK;
}

// Behind everything the event enqueued on set_stream: frames on this set start after ev_up (enqueue_frame), and the staging is
// refilled only once it has fired (staging_ready).
static int record_upload(gswt_ctx* c, DrawSet& D)
{
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(D.ev_up, c->set_stream));
    D.ev_up_pending = true; D.built = false;
    return GSWT_OK;
}

// The first draw list of a scene sizes the other draw sets too: every set's first fill used to allocate its own buffers (a
// pinned upload block, its device mirror, chunk tables, merged arrays) inside the sort event that reached it -- the first five
// swap-ins of a run each stalled the render thread for most of a millisecond.
// A set that already has buffers grows with the largest one seen only while nothing reads it (no frame in flight, not the
// current / pending / latest set: the next event's group copies read the latest one).
static int grow_idle_sets(gswt_ctx* c, const DrawSet& D)
{
    for (int k = 0; k < kDrawSets; k++) {
        DrawSet& o = c->sets[k];
        if (&o == &D) continue;
        const bool empty = !o.d_blob.p && !o.chunk_tab.p && !o.merged_list.p;
        bool used = k == c->cur_set || k == c->pending_set || k == c->latest_set || o.ev_up_pending;
        for (const FrameSlot& fs : c->slots) used = used || (fs.pending && fs.set == k);
        if (used && !empty) continue;
        if (o.g_valid) continue;      // it holds the group lists of an earlier sort event that later events may still copy from
        if (o.h_blob.cap >= D.h_blob.cap && o.d_blob.cap >= D.d_blob.cap && o.chunk_tab.cap >= D.chunk_tab.cap &&
            o.chunk_tab_xcd.cap >= D.chunk_tab_xcd.cap && o.merged_list.cap >= D.merged_list.cap && o.merged_map.cap >= D.merged_map.cap) continue;
        HIP_TRY(c, o.h_blob.ensure(D.h_blob.cap)); HIP_TRY(c, o.d_blob.ensure(D.d_blob.cap));
        HIP_TRY(c, o.chunk_tab.ensure(D.chunk_tab.cap)); HIP_TRY(c, o.chunk_tab_xcd.ensure(D.chunk_tab_xcd.cap));
        {
            const uint32_t* const l0 = o.merged_list.p; const uint32_t* const m0 = o.merged_map.p;
            HIP_TRY(c, o.merged_list.ensure(D.merged_list.cap)); HIP_TRY(c, o.merged_map.ensure(D.merged_map.cap));
            if (o.merged_list.p != l0 || o.merged_map.p != m0) o.g_valid = false;      // its lists are gone: no later event may copy from them
        }
    }
    return GSWT_OK;
}

// What gswt_set_draws_merge_groups stages for the device-side build of one event (counts of the tables in the set's pinned block).
struct MergePlan {
    size_t n_segs = 0, n_build = 0, n_jobs = 0, n_remap = 0, n_cblocks = 0, n_blocks = 0;
    uint64_t total = 0, build_total = 0;          // merged entries of the event; of the groups that are sorted
    std::vector<DrawSet::GroupDesc> desc;         // every group's range in the merged arrays
};

// Group ranges in the merged arrays (the concatenation order IS the merged-arena order).  A group whose view and ordered
// member tids equal a group of an earlier sort event whose set (`sources`, newest first) still holds its list keeps that list:
// it is copied on the device from that draw set with the members' map ids rewritten -- the reference's LRU hit
// (wangtile.rs:575-593) -- and only the other groups go through the segmented sort.  Everything is staged in the target set's
// pinned memory: the groups to sort with their segments and block table, the copy jobs with their block table and map-id remap
// pairs, the sort's item count.  Host work only; the merged draws are checked against their groups' ranges on the way.
static int match_groups(gswt_ctx* c, DrawSet& D, const std::vector<int>& sources, const gswt_draw* draws, int n_draws,
                        const gswt_merge_group* groups, int n_groups, const gswt_merge_member* members, int n_members, MergePlan& P)
{
    MergeSeg* const segs = D.hp<MergeSeg>(D.off_segs);
    MergeGroup* const grp = D.hp<MergeGroup>(D.off_groups);       // build space: only the groups that are sorted
    MergeCopy* const jobs = D.hp<MergeCopy>(D.off_jobs);
    uint2* const h_remap = D.hp<uint2>(D.off_remap);
    // hash -> (set, group) of every retained event; a set listed earlier (newer) wins on equal keys
    std::unordered_multimap<uint64_t, std::pair<int, uint32_t>> prev_by_hash;
    for (int k : sources) for (uint32_t q = 0; q < c->sets[k].g_desc.size(); q++) prev_by_hash.emplace(c->sets[k].g_desc[q].hash, std::make_pair(k, q));
    P.desc.assign((size_t)n_groups, DrawSet::GroupDesc{});
    uint64_t total = 0, build_total = 0;
    const size_t nv = (size_t)c->n_view;
    for (int g = 0; g < n_groups; g++) {
        const gswt_merge_group& G = groups[g];
        if ((uint64_t)G.first_member + G.n_members > (uint64_t)n_members || (int)G.view_id >= c->n_view)
            return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_draws_merge_groups: group %d out of range", g);
        uint64_t h = 1469598103934665603ull ^ G.view_id, len = 0;
        for (uint32_t m = 0; m < G.n_members; m++) {
            const gswt_merge_member& M = members[G.first_member + m];
            const int lods[2] = {(int)M.lod, M.other_lod};
            for (int k = 0; k < 2; k++) {
                if (lods[k] < 0) continue;
                if (lods[k] >= c->n_lod || (int)M.tile >= c->n_tile) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_draws_merge_groups: member tid out of range");
                len += c->raw_cnt[(size_t)lods[k] * c->n_tile + M.tile];
            }
            h = (h ^ (((uint64_t)M.lod << 40) | ((uint64_t)M.tile << 8) | (uint64_t)(uint8_t)(M.other_lod + 1))) * 1099511628211ull;
        }
        DrawSet::GroupDesc& d = P.desc[g];
        d.view = G.view_id; d.base = (uint32_t)total; d.len = (uint32_t)len; d.first = G.first_member; d.n = G.n_members; d.hash = h;
        int match = -1, match_set = -1, match_rank = 1 << 30;
        if (!sources.empty() && len) {
            auto range = prev_by_hash.equal_range(h);
            for (auto it = range.first; it != range.second; ++it) {
                const DrawSet& ps = c->sets[it->second.first];
                const DrawSet::GroupDesc& p = ps.g_desc[it->second.second];
                if (p.view != G.view_id || p.n != G.n_members || p.len != (uint32_t)len || G.n_members > 256u) continue;
                bool same = true;
                for (uint32_t m = 0; m < G.n_members && same; m++) {
                    const gswt_merge_member& a = members[G.first_member + m];
                    const gswt_merge_member& b = ps.g_members[p.first + m];
                    same = a.lod == b.lod && a.tile == b.tile && a.other_lod == b.other_lod;
                }
                if (!same) continue;
                // the newest holder (fewest map ids to rewrite, and its buffers are the warmest)
                int rank = 0;
                while (rank < (int)sources.size() && sources[rank] != it->second.first) rank++;
                if (rank < match_rank) { match_rank = rank; match = (int)it->second.second; match_set = it->second.first; }
            }
        }
        if (match >= 0) {
            const DrawSet& ps = c->sets[match_set];
            const DrawSet::GroupDesc& p = ps.g_desc[match];
            MergeCopy jb;
            jb.src = p.base; jb.dst = (uint32_t)total; jb.len = (uint32_t)len; jb.first_pair = (uint32_t)P.n_remap; jb.n_pairs = 0; jb.src_set = (uint32_t)match_set; jb._pad[0] = jb._pad[1] = 0;
            bool moved = false;
            for (uint32_t m = 0; m < G.n_members; m++) moved = moved || members[G.first_member + m].map_index != ps.g_members[p.first + m].map_index;
            if (moved) {
                for (uint32_t m = 0; m < G.n_members; m++)
                    h_remap[P.n_remap++] = make_uint2(ps.g_members[p.first + m].map_index, members[G.first_member + m].map_index);
                jb.n_pairs = G.n_members;
            }
            jobs[P.n_jobs++] = jb;
            if (match_rank > 0) c->stat_groups_reused_deep++;
        } else if (len) {
            MergeGroup& B = grp[P.n_build];
            B.base = (uint32_t)build_total; B.len = (uint32_t)len; B.mn = 2147483647; B.mx = -2147483647 - 1; B.out_base = (uint32_t)total; B._pad[0] = B._pad[1] = B._pad[2] = 0;
            for (uint32_t m = 0; m < G.n_members; m++) {
                const gswt_merge_member& M = members[G.first_member + m];
                const int lods[2] = {(int)M.lod, M.other_lod};
                for (int k = 0; k < 2; k++) {
                    if (lods[k] < 0) continue;
                    const size_t lt = (size_t)lods[k] * c->n_tile + M.tile;
                    MergeSeg sg;
                    sg.group = (uint32_t)P.n_build; sg.src = c->raw_off[lt * nv + G.view_id]; sg.len = c->raw_cnt[lt]; sg.start = (uint32_t)build_total;
                    sg.gs_offset = c->raw_merge_offset[lt]; sg.map_index = M.map_index; sg.lod = (uint32_t)lods[k]; sg._pad = 0;
                    if (sg.len) segs[P.n_segs++] = sg;
                    build_total += sg.len;
                }
            }
            P.n_build++;
        }
        total += len;
    }
    if (total >= 0xFFFFFFFFull) return fail(c, GSWT_ERR_CAPACITY, "gswt_set_draws_merge_groups: merged lists exceed 2^32 entries");
    for (int i = 0; i < n_draws; i++)
        if (draws[i].merged) {
            const uint32_t g = draws[i].merged_group;
            if ((int)g >= n_groups || draws[i].merged_offset != P.desc[g].base || draws[i].merged_count != P.desc[g].len)
                return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_draws_merge_groups: draw %d does not match group %u (offset %u/%u count %u/%u)", i, g,
                            draws[i].merged_offset, (int)g < n_groups ? P.desc[g].base : 0u, draws[i].merged_count, (int)g < n_groups ? P.desc[g].len : 0u);
        }
    // block tables: every copy job / segment cut into runs of <= 1024 entries (what one workgroup handles)
    uint2* const h_cblocks = D.hp<uint2>(D.off_cblocks);
    uint2* const h_blocks = D.hp<uint2>(D.off_blocks);
    for (size_t q = 0; q < P.n_jobs; q++)
        for (uint32_t off = 0; off < jobs[q].len; off += 1024u) h_cblocks[P.n_cblocks++] = make_uint2((uint32_t)q, off);
    for (size_t q = 0; q < P.n_segs; q++)
        for (uint32_t off = 0; off < segs[q].len; off += 1024u) h_blocks[P.n_blocks++] = make_uint2((uint32_t)q, off);
    *D.hp<SortCount>(D.off_count) = sort_count((uint32_t)build_total);       // the sort's item count, as its kernels read it
    P.total = total; P.build_total = build_total;
    return GSWT_OK;
}

extern "C" {

int gswt_set_draws(gswt_ctx* c, const gswt_draw* draws, int n_draws, const uint32_t* merged_gs_index,
                   const uint32_t* merged_map_id, const uint32_t* merged_lod_id, size_t n_merged)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    GSWT_TRY(check_draw_list(c, draws, n_draws));
    if (n_merged && (!merged_gs_index || !merged_map_id)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_draws: merged arrays missing");
    if (n_merged >= 0xFFFFFFFFull) return fail(c, GSWT_ERR_CAPACITY, "gswt_set_draws: merged lists exceed 2^32 entries");
    hipSetDevice(c->device);
    const int target = next_target(c);
    collect_set(c, target, true);
    DrawSet& D = c->sets[target];
    GSWT_TRY(staging_ready(c, D));
    HIP_TRY(c, D.plan((size_t)n_draws, 0, 0, 0));
    uint64_t entries = 0;
    size_t n_chunks = 0;
    GSWT_TRY(fill_draw_records(c, D, draws, n_draws, n_merged, merged_lod_id != nullptr, &entries));
    GSWT_TRY(assign_slots(c, D, n_draws, &n_chunks));
    // The upload is asynchronous on set_stream from the set's pinned staging; every frame submitted afterwards starts behind the
    // event recorded on that stream (enqueue_frame).
    GSWT_TRY(upload_block(c, D, n_draws));
    GSWT_TRY(record_upload(c, D));
    // merged arrays: pack gs_index | lod << 28
    GSWT_TRY(size_merged_arrays(c, D, n_merged));
    if (n_merged) {
        std::vector<uint32_t> packed(n_merged);
        for (size_t k = 0; k < n_merged; k++) {
            if (merged_gs_index[k] >= c->n_splats) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_draws: merged gs_index[%zu] out of range", k);
            packed[k] = merged_gs_index[k];
        }
        for (int i = 0; i < n_draws; i++) {
            const gswt_draw& g = draws[i];
            if (g.merged && g.merged_has_lod)
                for (uint32_t k = 0; k < g.merged_count; k++) {
                    uint32_t l = merged_lod_id[g.merged_offset + k];
                    if (l > 15u) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_draws: merged lod id out of range");
                    packed[g.merged_offset + k] |= l << kLodShift;
                }
        }
        HIP_TRY(c, hipMemcpy(D.merged_list.p, packed.data(), n_merged * 4, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(D.merged_map.p, merged_map_id, n_merged * 4, hipMemcpyHostToDevice));
        HIP_TRY(c, null_stream_done());
    }
    commit_draw_list(D, n_draws, n_chunks, entries);
    GSWT_TRY(grow_idle_sets(c, D));
    publish_set(c, target);
    return GSWT_OK;
} GSWT_CATCH

int gswt_set_draws_merge_groups(gswt_ctx* c, const gswt_draw* draws, int n_draws, const gswt_merge_group* groups, int n_groups,
                                const gswt_merge_member* members, int n_members)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    if (n_groups < 0 || n_members < 0 || (n_groups && (!groups || !members))) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_draws_merge_groups: bad groups");
    if (n_groups && c->raw_cnt.empty()) return fail(c, GSWT_ERR_STATE, "gswt_set_draws_merge_groups before gswt_upload_raw_depth");
    if (n_groups > 32768) return fail(c, GSWT_ERR_CAPACITY, "gswt_set_draws_merge_groups: more than 32768 merged groups");
    hipSetDevice(c->device);
    const int target = next_target(c);
    collect_set(c, target, false);
    DrawSet& D = c->sets[target];
    // every other set that still holds the group lists of an earlier sort event, newest first (the sets are refilled round robin)
    std::vector<int> sources;
    if (c->draws_ready && !c->opt.no_merge_reuse)
        for (int j = 0; j < kDrawSets - 1; j++) {
            const int k = ((c->latest_set - j) % kDrawSets + kDrawSets) % kDrawSets;
            if (k != target && c->sets[k].g_valid && c->sets[k].merged_list.p) sources.push_back(k);
        }
    GSWT_TRY(staging_ready(c, D));
    {   // upper bound of the merged entries (sizes the block tables of the upload block)
        size_t total_upper = 0;
        for (int q = 0; q < n_members; q++) {
            const gswt_merge_member& M = members[q];
            if ((int)M.lod < c->n_lod && (int)M.tile < c->n_tile) total_upper += c->raw_cnt[(size_t)M.lod * c->n_tile + M.tile];
            if (M.other_lod >= 0 && M.other_lod < c->n_lod && (int)M.tile < c->n_tile) total_upper += c->raw_cnt[(size_t)M.other_lod * c->n_tile + M.tile];
        }
        HIP_TRY(c, D.plan((size_t)std::max(n_draws, 0), (size_t)n_groups, (size_t)n_members, total_upper));
    }
    MergePlan P;
    GSWT_TRY(match_groups(c, D, sources, draws, n_draws, groups, n_groups, members, n_members, P));
    GSWT_TRY(check_draw_list(c, draws, n_draws));
    uint64_t entries = 0;
    size_t n_chunks = 0;
    GSWT_TRY(fill_draw_records(c, D, draws, n_draws, (size_t)P.total, true, &entries));
    GSWT_TRY(assign_slots(c, D, n_draws, &n_chunks));
    GSWT_TRY(size_merged_arrays(c, D, (size_t)P.total));
    commit_draw_list(D, n_draws, n_chunks, entries);
    GSWT_TRY(grow_idle_sets(c, D));
    // (grow_idle_sets grows the arrays of sets nothing reads; a source whose arrays it re-allocated lost g_valid: that cannot be one
    // of `sources` -- a set with g_valid is kept from growing -- but it is checked all the same)
    MergeSources msrc;
    for (int k = 0; k < kMergeSources; k++) { msrc.list[k] = nullptr; msrc.map[k] = nullptr; }
    for (int k : sources) {
        if (!c->sets[k].g_valid) return fail(c, GSWT_ERR_STATE, "gswt_set_draws_merge_groups: a source set lost its lists");
        msrc.list[k] = c->sets[k].merged_list.p; msrc.map[k] = c->sets[k].merged_map.p;
    }
    const MergeCopy* const jobs = D.hp<MergeCopy>(D.off_jobs);
    for (size_t q = 0; q < P.n_jobs; q++) D.src_mask |= 1u << jobs[q].src_set;
    D.g_desc.swap(P.desc);
    D.g_members.assign(members, members + n_members);
    // (g_valid stays false -- commit_draw_list -- until everything below has been enqueued: a failed HIP call leaves unbuilt lists)
    c->stat_groups_built += P.n_build; c->stat_groups_reused += P.n_jobs;
    hipStream_t s = c->set_stream;
    const uint32_t n_total = (uint32_t)P.build_total;
    // ONE upload for the whole event, then the chunk tables, the copies and (for the groups that changed) the segmented sort, all
    // on set_stream.  Nothing is waited for: every frame submitted from now on starts behind an event recorded on that
    // stream (enqueue_frame), i.e. behind the finished lists.  (A grown buffer is the exception: hipFree waits for the device.)
    GSWT_TRY(upload_block(c, D, n_draws));
    if (P.n_jobs)
        launch_merge_copy(s, D.dp<MergeCopy>(D.off_jobs), D.dp<uint2>(D.off_cblocks), (uint32_t)P.n_cblocks, D.dp<uint2>(D.off_remap), msrc,
                          D.merged_list.p, D.merged_map.p);
    if (P.n_build) {
        int gbits = 1;
        while ((1u << gbits) < P.n_build) gbits++;
        const size_t radix_words = radix_ws_words(n_total, 16 + gbits);
        HIP_TRY(c, c->mg_ws.ensure_roomy(4 * (size_t)n_total + radix_words + 16));        // sort workspace, shared by all events (stream-ordered)
        uint32_t* w = c->mg_ws.p;
        uint32_t* radix = w + 4 * (size_t)n_total;
        HIP_TRY(c, hipMemsetAsync(radix, 0, (radix_words + 16) * 4, s));
        launch_merge_build(s, D.dp<MergeSeg>(D.off_segs), (uint32_t)P.n_segs, D.dp<uint2>(D.off_blocks), (uint32_t)P.n_blocks, D.dp<MergeGroup>(D.off_groups),
                           (uint32_t)P.n_build, c->raw_depth.p, n_total, D.dp<SortCount>(D.off_count), w, w + n_total, w + 2 * (size_t)n_total,
                           w + 3 * (size_t)n_total, radix, gbits, D.merged_list.p, D.merged_map.p);
    }
    GSWT_TRY(record_upload(c, D));
    D.g_valid = true;
    publish_set(c, target);
    return GSWT_OK;
} GSWT_CATCH

int gswt_debug_read_merged(gswt_ctx* c, uint32_t* packed_list, uint32_t* map_id, size_t capacity, size_t* n)
try {
    if (!c || !n) return GSWT_ERR_BAD_ARG;
    const DrawSet& D = c->sets[c->cur_set];
    *n = D.n_merged;
    if (!packed_list || !map_id) return GSWT_OK;
    if (capacity < D.n_merged) return fail(c, GSWT_ERR_CAPACITY, "buffer holds %zu entries, need %zu", capacity, D.n_merged);
    hipSetDevice(c->device);
    HIP_TRY(c, sync_all(c));
    if (D.n_merged) {
        HIP_TRY(c, hipMemcpy(packed_list, D.merged_list.p, D.n_merged * 4, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(map_id, D.merged_map.p, D.n_merged * 4, hipMemcpyDeviceToHost));
    }
    return GSWT_OK;
} GSWT_CATCH

int gswt_debug_merge_stats(const gswt_ctx* c, unsigned long long out[2])
{
    if (!c || !out) return GSWT_ERR_BAD_ARG;
    out[0] = c->stat_groups_built; out[1] = c->stat_groups_reused;
    return GSWT_OK;
}

int gswt_debug_merge_stats_deep(const gswt_ctx* c, unsigned long long* out)
{
    if (!c || !out) return GSWT_ERR_BAD_ARG;
    *out = c->stat_groups_reused_deep;
    return GSWT_OK;
}

}  // extern "C"
