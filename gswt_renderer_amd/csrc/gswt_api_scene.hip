// gswt_api_scene.hip -- the scene of libgswt_hip.so (host only): gswt_upload_scene (texture and base lists from the host),
// gswt_upload_scene_rows (the same tables built on the device from the normalised rows, kernels in gswt_scene.hip),
// gswt_upload_raw_depth (the raw depths of the device-side merged-list build) and gswt_debug_read_scene.
#include "gswt_ctx.h"
#include "host/gswt_math.h"

#include <algorithm>
#include <cmath>

using namespace gswt;

// The tile-local bounds of the splat centres and the largest covariance bound, as the band cull of column-sharded frames reads them.
// odd: a non-finite coordinate anywhere (or no splat at all, lo > hi) -> the infinite box: never cull.
static void commit_local_bounds(gswt_ctx* c, float lo[3], float hi[3], bool odd, float max_trace)
{
    if (odd || lo[0] > hi[0]) { for (int k = 0; k < 3; k++) { lo[k] = -3.402823466e+38f; hi[k] = 3.402823466e+38f; } }
    for (int k = 0; k < 3; k++) { c->loc_lo[k] = lo[k]; c->loc_hi[k] = hi[k]; }
    c->loc_max_trace = max_trace;
}

extern "C" {

int gswt_upload_scene(gswt_ctx* c, const uint32_t* tex_data, size_t n_splats, const gswt_base_list* lists, int n_lod,
                      int n_tile, int n_view)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    if (!tex_data || n_splats == 0 || !lists || n_lod <= 0 || n_tile <= 0 || n_view <= 0)
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_upload_scene: empty scene");
    if (n_lod > 16) return fail(c, GSWT_ERR_BAD_ARG, "gswt_upload_scene: n_lod %d > 16 (transition_dist_vec holds 16)", n_lod);
    if (n_splats > (size_t)kIdxMask) return fail(c, GSWT_ERR_CAPACITY, "gswt_upload_scene: %zu splats exceed 2^28", n_splats);
    hipSetDevice(c->device);
    HIP_TRY(c, collect_pending(c));
    c->scene_ready = false; c->draws_ready = false;
    invalidate_merge_sources(c);
    HIP_TRY(c, c->tex.ensure(2 * n_splats));
    HIP_TRY(c, hipMemcpy(c->tex.p, tex_data, n_splats * 32, hipMemcpyHostToDevice));
    c->n_splats = n_splats;
    {   // tile-local bounds of every splat centre and the largest covariance bound: what the band cull of column-sharded frames
        // places at a map cell's origin (every Wang-tile instance is the same tile-local content)
        float lo[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, hi[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
        float tr_max = 0.0f;
        bool odd = false;
        for (size_t i = 0; i < n_splats; i++) {
            const uint32_t* r = tex_data + 8 * i;
            float p[3];
            memcpy(p, r, 12);
            for (int k = 0; k < 3; k++) {
                if (!gswt_host::finite_coord(p[k])) { odd = true; continue; }
                lo[k] = std::min(lo[k], p[k]); hi[k] = std::max(hi[k], p[k]);
            }
            const float tr = gswt_host::cov_extent_bound(r);      // (k_scene_tex folds the same bound on the device)
            if (tr == tr) tr_max = std::max(tr_max, tr);
        }
        commit_local_bounds(c, lo, hi, odd, tr_max);
    }
    const size_t nl = (size_t)n_lod * n_tile * n_view;
    c->lists.assign(nl, ListRef{});
    std::vector<uint32_t> arena;
    std::vector<float> boxes;               // six floats per chunk
    // bounding box of every chunk (chunk_entry_range: k_project's order) of list [base, base + count);
    // a chunk that holds a non-finite position gets the infinite box (never culled)
    auto add_boxes = [&](uint32_t base, uint32_t count) -> uint32_t {
        const uint32_t first = (uint32_t)(boxes.size() / 6);
        for (uint32_t k = 0; (size_t)k * kChunk < count; k++) {
            uint32_t lo_i, hi_i;
            chunk_entry_range(count, k, lo_i, hi_i);
            float lo[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, hi[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
            bool odd = false;
            for (uint32_t j = lo_i; j < hi_i; j++) {
                float pq[3];
                memcpy(pq, tex_data + 8 * (size_t)(arena[base + j] & kIdxMask), 12);
                for (int a = 0; a < 3; a++) {
                    if (!gswt_host::finite_coord(pq[a])) odd = true;
                    lo[a] = std::min(lo[a], pq[a]); hi[a] = std::max(hi[a], pq[a]);
                }
            }
            for (int a = 0; a < 3; a++) boxes.push_back(odd ? -__builtin_inff() : lo[a]);
            for (int a = 0; a < 3; a++) boxes.push_back(odd ? __builtin_inff() : hi[a]);
        }
        return first;
    };
    size_t total = 0;
    for (size_t i = 0; i < nl; i++) total += lists[i].splat_count;
    arena.reserve(2 * total);
    for (size_t i = 0; i < nl; i++) {
        const gswt_base_list& L = lists[i];
        const uint32_t lod = (uint32_t)(i / ((size_t)n_tile * n_view));
        if (L.splat_count && (!L.gs_index || !L.gs_lod_id)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_upload_scene: list %zu has null arrays", i);
        ListRef ref;
        ref.pair_base = (uint32_t)arena.size();
        ref.pair_count = L.splat_count;
        for (uint32_t j = 0; j < L.splat_count; j++) {
            if (L.gs_index[j] >= n_splats) return fail(c, GSWT_ERR_BAD_ARG, "gswt_upload_scene: list %zu entry %u out of range", i, j);
            if (L.gs_lod_id[j] > 15u) return fail(c, GSWT_ERR_BAD_ARG, "gswt_upload_scene: list %zu lod id out of range", i);
            arena.push_back(L.gs_index[j] | (L.gs_lod_id[j] << kLodShift));
        }
        ref.self_base = (uint32_t)arena.size();
        for (uint32_t j = 0; j < L.splat_count; j++)
            if (L.gs_lod_id[j] == lod) arena.push_back(L.gs_index[j] | (lod << kLodShift));
        ref.self_count = (uint32_t)arena.size() - ref.self_base;
        ref.pair_box = add_boxes(ref.pair_base, ref.pair_count);
        ref.self_box = add_boxes(ref.self_base, ref.self_count);
        c->lists[i] = ref;
    }
    if (arena.size() >= 0xFFFFFFFFull) return fail(c, GSWT_ERR_CAPACITY, "gswt_upload_scene: static lists exceed 2^32 entries");
    HIP_TRY(c, c->static_list.ensure(arena.size() + 1));
    HIP_TRY(c, hipMemcpy(c->static_list.p, arena.data(), arena.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, c->static_boxes.ensure(boxes.size() + 6));
    if (!boxes.empty()) HIP_TRY(c, hipMemcpy(c->static_boxes.p, boxes.data(), boxes.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, null_stream_done());
    c->static_n = arena.size(); c->boxes_n = boxes.size() / 6;
    c->n_lod = n_lod; c->n_tile = n_tile; c->n_view = n_view;
    c->scene_ready = true;
    return GSWT_OK;
} GSWT_CATCH

// gswt_upload_scene + gswt_upload_raw_depth of a full wang, built on the device from the normalised rows (gswt_scene.hip):
// the same texture, raw-depth arena and tables, static arena, ListRef table, chunk boxes and local bounds.  Every offset follows
// from the counts, so the host lays out the tables first and reads back only the eight words of the bounds.
int gswt_upload_scene_rows(gswt_ctx* c, const uint8_t* const* rows32, const uint32_t* counts, int n_lod, int n_tile, const float* presort_vp,
                           int n_view)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    if (!rows32 || !counts || !presort_vp || n_lod <= 0 || n_tile <= 0 || n_view <= 0)
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_upload_scene_rows: empty scene");
    if (n_lod > 16) return fail(c, GSWT_ERR_BAD_ARG, "gswt_upload_scene_rows: n_lod %d > 16 (transition_dist_vec holds 16)", n_lod);
    if (n_view > kSceneMaxViews) return fail(c, GSWT_ERR_BAD_ARG, "gswt_upload_scene_rows: n_view %d > %d", n_view, kSceneMaxViews);
    const size_t n_lt = (size_t)n_lod * n_tile, nv = (size_t)n_view;
    // one view's lists are sorted together: key = list << 16 | bucket must fit 32 bits
    if (n_lt > 65536) return fail(c, GSWT_ERR_CAPACITY, "gswt_upload_scene_rows: %zu lists per view exceed the 16 list bits of the sort key", n_lt);
    std::vector<uint32_t> moff(n_lt);
    size_t n_splats = 0;
    for (size_t i = 0; i < n_lt; i++) {
        if (counts[i] == 0) return fail(c, GSWT_ERR_BAD_ARG, "gswt_upload_scene_rows: tile scene %zu is empty", i);
        if (!rows32[i]) return fail(c, GSWT_ERR_BAD_ARG, "gswt_upload_scene_rows: tile scene %zu has null rows", i);
        moff[i] = (uint32_t)std::min(n_splats, (size_t)kIdxMask);
        n_splats += counts[i];
        if (n_splats > (size_t)kIdxMask) return fail(c, GSWT_ERR_CAPACITY, "gswt_upload_scene_rows: more than 2^28 splats");
    }
    auto cnt = [&](size_t l, size_t t) -> uint32_t { return counts[l * n_tile + t]; };
    auto list_len = [&](size_t l, size_t t) -> uint32_t { return cnt(l, t) + (l + 1 < (size_t)n_lod ? cnt(l + 1, t) : 0u); };
    // the ListRef table and the box numbering of gswt_upload_scene (per list: pair list, self list; pair boxes, self boxes)
    const size_t nl = n_lt * nv;
    std::vector<ListRef> lists(nl);
    size_t arena_n = 0, boxes_n = 0;
    for (size_t l = 0; l < (size_t)n_lod; l++)
        for (size_t t = 0; t < (size_t)n_tile; t++)
            for (size_t v = 0; v < nv; v++) {
                ListRef& r = lists[(l * n_tile + t) * nv + v];
                r.pair_base = (uint32_t)arena_n; r.pair_count = list_len(l, t);
                r.self_base = (uint32_t)(arena_n + r.pair_count); r.self_count = cnt(l, t);
                arena_n += (size_t)r.pair_count + r.self_count;
                r.pair_box = (uint32_t)boxes_n; boxes_n += (r.pair_count + kChunk - 1) / kChunk;
                r.self_box = (uint32_t)boxes_n; boxes_n += (r.self_count + kChunk - 1) / kChunk;
                if (arena_n >= 0xFFFFFFFFull) return fail(c, GSWT_ERR_CAPACITY, "gswt_upload_scene_rows: static lists exceed 2^32 entries");
            }
    if (nv * n_splats >= 0xFFFFFFFFull) return fail(c, GSWT_ERR_CAPACITY, "gswt_upload_scene_rows: raw depth arena exceeds 2^32");
    // per view: one group per (lod, tile) = its base list, segments raw(l, t, v) then raw(l + 1, t, v); blocks of <= 1024 entries
    size_t n_total = 0;
    for (size_t l = 0; l < (size_t)n_lod; l++) for (size_t t = 0; t < (size_t)n_tile; t++) n_total += list_len(l, t);
    std::vector<MergeSeg> segs;
    std::vector<MergeGroup> groups;
    std::vector<uint2> blocks;
    std::vector<size_t> seg_first(nv + 1), blk_first(nv + 1);
    for (size_t v = 0; v < nv; v++) {
        seg_first[v] = segs.size(); blk_first[v] = blocks.size();
        uint32_t build = 0;
        for (size_t l = 0; l < (size_t)n_lod; l++)
            for (size_t t = 0; t < (size_t)n_tile; t++) {
                const uint32_t g = (uint32_t)(l * n_tile + t);
                MergeGroup G;
                G.base = build; G.len = list_len(l, t); G.mn = 2147483647; G.mx = -2147483647 - 1;
                G.out_base = lists[(size_t)g * nv + v].pair_base; G._pad[0] = G._pad[1] = G._pad[2] = 0;
                groups.push_back(G);
                for (size_t q = l; q < (size_t)n_lod && q <= l + 1; q++) {
                    const size_t lt = q * n_tile + t;
                    MergeSeg sg;
                    sg.group = g; sg.src = (uint32_t)(nv * moff[lt] + v * counts[lt]); sg.len = counts[lt]; sg.start = build;
                    sg.gs_offset = moff[lt]; sg.map_index = 0; sg.lod = (uint32_t)q; sg._pad = 0;
                    for (uint32_t off = 0; off < sg.len; off += 1024u) blocks.push_back(make_uint2((uint32_t)(segs.size() - seg_first[v]), off));
                    segs.push_back(sg);
                    build += sg.len;
                }
            }
    }
    seg_first[nv] = segs.size(); blk_first[nv] = blocks.size();
    SceneViews vps;
    memset(&vps, 0, sizeof(vps));
    vps.n_view = (uint32_t)nv;
    memcpy(vps.vp, presort_vp, nv * 16 * sizeof(float));
    int gbits = 1;
    while ((1u << gbits) < n_lt) gbits++;

    hipSetDevice(c->device);
    // every frame in flight (and its re-run on a pair overflow or a short grid) finishes against the scene it was submitted with
    HIP_TRY(c, collect_pending(c));
    c->scene_ready = false; c->draws_ready = false;
    invalidate_merge_sources(c);
    c->raw_cnt.clear(); c->raw_merge_offset.clear(); c->raw_off.clear();
    hipStream_t s = c->stream;
    // scratch of the build (freed on return): the rows, the tables, the sort's keys / vals and workspace
    const size_t radix_words = radix_ws_words((uint32_t)n_total, 16 + gbits);
    DevBuf<uint4> rows_d;
    DevBuf<uint32_t> tabs, sortbuf;
    DevBuf<int32_t> bounds_d;
    HIP_TRY(c, rows_d.ensure(2 * n_splats));
    const size_t seg_words = segs.size() * sizeof(MergeSeg) / 4, grp_words = groups.size() * sizeof(MergeGroup) / 4;
    const size_t blk_words = 2 * blocks.size(), list_words = nl * sizeof(ListRef) / 4;
    HIP_TRY(c, tabs.ensure(2 * n_lt + seg_words + grp_words + blk_words + list_words));
    const size_t count_words = 2 * sizeof(SortCount) / 4;       // the sort's count record, on a 64-byte line of its own
    HIP_TRY(c, sortbuf.ensure(4 * n_total + count_words + radix_words + 16));
    HIP_TRY(c, bounds_d.ensure(8));
    HIP_TRY(c, c->tex.ensure(2 * n_splats));
    HIP_TRY(c, c->raw_depth.ensure(nv * n_splats + 1));
    HIP_TRY(c, c->static_list.ensure(arena_n + 1));
    HIP_TRY(c, c->static_boxes.ensure(6 * boxes_n + 6));
    uint32_t* const d_moff = tabs.p;
    uint32_t* const d_cnt = d_moff + n_lt;
    MergeSeg* const d_segs = reinterpret_cast<MergeSeg*>(d_cnt + n_lt);
    MergeGroup* const d_groups = reinterpret_cast<MergeGroup*>(tabs.p + 2 * n_lt + seg_words);
    uint2* const d_blocks = reinterpret_cast<uint2*>(tabs.p + 2 * n_lt + seg_words + grp_words);
    ListRef* const d_lists = reinterpret_cast<ListRef*>(tabs.p + 2 * n_lt + seg_words + grp_words + blk_words);
    for (size_t i = 0; i < n_lt; i++)
        HIP_TRY(c, hipMemcpyAsync(rows_d.p + 2 * (size_t)moff[i], rows32[i], (size_t)counts[i] * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_moff, moff.data(), n_lt * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_cnt, counts, n_lt * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_segs, segs.data(), seg_words * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_groups, groups.data(), grp_words * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_blocks, blocks.data(), blk_words * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_lists, lists.data(), list_words * 4, hipMemcpyHostToDevice, s));
    const int32_t bounds_init[8] = {2147483647, 2147483647, 2147483647, -2147483647 - 1, -2147483647 - 1, -2147483647 - 1, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(bounds_d.p, bounds_init, sizeof(bounds_init), hipMemcpyHostToDevice, s));
    launch_scene_tex(s, rows_d.p, (uint32_t)n_splats, c->tex.p, bounds_d.p);
    launch_scene_raw(s, rows_d.p, (uint32_t)n_splats, d_moff, d_cnt, (uint32_t)n_lt, vps, c->raw_depth.p);
    // base lists, one view at a time (the sort's scratch covers one view); sorted keys / vals -> reversed pair lists in the arena
    uint32_t* const ka = sortbuf.p;
    uint32_t* const va = ka + n_total;
    uint32_t* const kb = va + n_total;
    uint32_t* const vb = kb + n_total;
    SortCount* const d_count = reinterpret_cast<SortCount*>(vb + n_total);      // the sort's item count (read only)
    uint32_t* const ws = vb + n_total + count_words;
    const SortCount n_items = sort_count(n_total);
    HIP_TRY(c, hipMemcpyAsync(d_count, &n_items, sizeof(n_items), hipMemcpyHostToDevice, s));
    for (size_t v = 0; v < nv; v++) {
        HIP_TRY(c, hipMemsetAsync(ws, 0, radix_words * 4, s));
        const int where = launch_scene_sort(s, d_segs + seg_first[v], d_blocks + blk_first[v], (uint32_t)(blk_first[v + 1] - blk_first[v]),
                                            d_groups + v * n_lt, c->raw_depth.p, (uint32_t)n_total, d_count,
                                            ka, va, kb, vb, ws, gbits);
        launch_scene_scatter(s, d_segs + seg_first[v], (uint32_t)(seg_first[v + 1] - seg_first[v]), d_groups + v * n_lt, where ? kb : ka,
                             where ? vb : va, (uint32_t)n_total, c->static_list.p, (uint32_t)arena_n);
    }
    launch_scene_self(s, d_lists, (uint32_t)nl, (uint32_t)((size_t)n_tile * nv), c->static_list.p);
    launch_scene_boxes(s, d_lists, (uint32_t)nl, (uint32_t)boxes_n, c->static_list.p, c->tex.p, (uint32_t)n_splats, c->static_boxes.p);
    HIP_TRY(c, hipGetLastError());
    int32_t bounds[8];
    HIP_TRY(c, hipMemcpyAsync(bounds, bounds_d.p, sizeof(bounds), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    {   // decode as gswt_upload_scene leaves them
        auto ord2f = [](int32_t i) { const int32_t b = i >= 0 ? i : i ^ 0x7FFFFFFF; float f; memcpy(&f, &b, 4); return f; };
        float lo[3], hi[3], max_trace;
        for (int k = 0; k < 3; k++) { lo[k] = ord2f(bounds[k]); hi[k] = ord2f(bounds[3 + k]); }
        memcpy(&max_trace, &bounds[7], 4);
        commit_local_bounds(c, lo, hi, bounds[6] != 0, max_trace);
    }
    c->n_splats = n_splats;
    c->lists = std::move(lists);
    c->static_n = arena_n; c->boxes_n = boxes_n;
    c->raw_cnt.assign(counts, counts + n_lt);
    c->raw_merge_offset = moff;
    c->raw_off.assign(n_lt * nv, 0);
    for (size_t i = 0; i < n_lt; i++) for (size_t v = 0; v < nv; v++) c->raw_off[i * nv + v] = (uint32_t)(nv * moff[i] + v * counts[i]);
    c->n_lod = n_lod; c->n_tile = n_tile; c->n_view = n_view;
    c->scene_ready = true;
    return GSWT_OK;
} GSWT_CATCH

int gswt_debug_read_scene(gswt_ctx* c, int what, void* out, size_t cap_bytes, size_t* n_bytes)
try {
    if (!c || !n_bytes) return GSWT_ERR_BAD_ARG;
    if (!c->scene_ready) return fail(c, GSWT_ERR_STATE, "gswt_debug_read_scene before a scene upload");
    const void* dev = nullptr;
    const void* hostp = nullptr;
    size_t bytes = 0;
    std::vector<uint32_t> tmp;
    switch (what) {
    case GSWT_SCENE_TEX: dev = c->tex.p; bytes = c->n_splats * 32; break;
    case GSWT_SCENE_RAW_DEPTH: {
        size_t total = 0;
        for (uint32_t k : c->raw_cnt) total += (size_t)k * c->n_view;
        dev = c->raw_depth.p; bytes = total * 4; break;
    }
    case GSWT_SCENE_RAW_TABLES:
        tmp = c->raw_off;
        tmp.insert(tmp.end(), c->raw_cnt.begin(), c->raw_cnt.end());
        tmp.insert(tmp.end(), c->raw_merge_offset.begin(), c->raw_merge_offset.end());
        hostp = tmp.data(); bytes = tmp.size() * 4; break;
    case GSWT_SCENE_STATIC_LIST: dev = c->static_list.p; bytes = c->static_n * 4; break;
    case GSWT_SCENE_STATIC_BOXES: dev = c->static_boxes.p; bytes = c->boxes_n * 24; break;
    case GSWT_SCENE_LISTS: hostp = c->lists.data(); bytes = c->lists.size() * sizeof(ListRef); break;
    case GSWT_SCENE_BOUNDS: {
        tmp.resize(7);
        memcpy(tmp.data(), c->loc_lo, 12); memcpy(tmp.data() + 3, c->loc_hi, 12); memcpy(tmp.data() + 6, &c->loc_max_trace, 4);
        hostp = tmp.data(); bytes = 28; break;
    }
    default: return fail(c, GSWT_ERR_BAD_ARG, "gswt_debug_read_scene: unknown item %d", what);
    }
    *n_bytes = bytes;
    if (!out) return GSWT_OK;
    if (cap_bytes < bytes) return fail(c, GSWT_ERR_CAPACITY, "gswt_debug_read_scene: buffer holds %zu bytes, need %zu", cap_bytes, bytes);
    if (hostp) { memcpy(out, hostp, bytes); return GSWT_OK; }
    hipSetDevice(c->device);
    HIP_TRY(c, sync_all(c));
    if (bytes) HIP_TRY(c, hipMemcpy(out, dev, bytes, hipMemcpyDeviceToHost));
    return GSWT_OK;
} GSWT_CATCH

int gswt_upload_raw_depth(gswt_ctx* c, const int32_t* const* raw_depth, const uint32_t* counts, const uint32_t* merge_offset)
try {
    if (!c || !raw_depth || !counts || !merge_offset) return GSWT_ERR_BAD_ARG;
    if (!c->scene_ready) return fail(c, GSWT_ERR_STATE, "gswt_upload_raw_depth before gswt_upload_scene");
    hipSetDevice(c->device);
    HIP_TRY(c, sync_all(c));
    invalidate_merge_sources(c);
    const size_t nlt = (size_t)c->n_lod * c->n_tile, nv = (size_t)c->n_view;
    c->raw_cnt.assign(counts, counts + nlt);
    c->raw_merge_offset.assign(merge_offset, merge_offset + nlt);
    c->raw_off.assign(nlt * nv, 0);
    size_t total = 0;
    for (size_t i = 0; i < nlt; i++) for (size_t v = 0; v < nv; v++) { c->raw_off[i * nv + v] = (uint32_t)total; total += counts[i]; }
    if (total >= 0xFFFFFFFFull) return fail(c, GSWT_ERR_CAPACITY, "gswt_upload_raw_depth: raw depth arena exceeds 2^32");
    std::vector<int32_t> arena(total);
    for (size_t i = 0; i < nlt; i++)
        for (size_t v = 0; v < nv; v++) {
            if (counts[i] && !raw_depth[i * nv + v]) return fail(c, GSWT_ERR_BAD_ARG, "gswt_upload_raw_depth: null array");
            if (counts[i]) memcpy(arena.data() + c->raw_off[i * nv + v], raw_depth[i * nv + v], (size_t)counts[i] * 4);
        }
    HIP_TRY(c, c->raw_depth.ensure(total + 1));
    if (total) HIP_TRY(c, hipMemcpy(c->raw_depth.p, arena.data(), total * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, null_stream_done());
    return GSWT_OK;
} GSWT_CATCH

}  // extern "C"
