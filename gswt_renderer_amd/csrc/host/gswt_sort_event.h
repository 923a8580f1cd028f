// gswt_sort_event.h -- the per-cell, per-edge and per-record arithmetic of one sort event (WangTile::update_lod, the edge tests
// of selective merging and of the Graph order, the order keys, the presort-view choice, the SortData records and the draw the
// render loop makes of one), shared by libgswt_host (g++: gswt_wang_sort_tiles, gswt_renderer_build_draws) and the worker kernels
// of libgswt_hip (hipcc, GSWT_HD = __host__ __device__: gswt_worker.hip): one source, one operator sequence, so the two sides'
// records and draws agree bit for bit.  The order-defined sequential algorithms around these (top-k union, convexity closure,
// breadth-first order, toposort, axis merge) stay with each side.  No state: plain values, tables and the POD records in and out.
#pragma once
#include "../../../include/gswt_hip.h"
#include "gswt_math.h"
#include "gswt_surface.h"

namespace gswt_host {

// structure.rs data contracts
enum { SORT_DISTANCE = 0, SORT_VIEWPORT = 1, SORT_OBJECT = 2, SORT_GRAPH = 3 };
enum { MERGE_NONE = 0, MERGE_AXIS = 1, MERGE_EDGE = 2 };
enum { TR_NONE = 0, TR_SPAWNING = 1, TR_CHANGING_HIGHER = 2, TR_CHANGING_LOWER = 3 };   // Changing(false) / Changing(true)
enum { MS_NONE = 0, MS_FROM = 1, MS_TO = 2 };
// what draw_from_tile reports: places where the reference's render loop panics
enum { ERR_LOD0_HIGHER = 1, ERR_NO_CORNERS = 2 };

// ---- lod_select_spatial, wangtile.rs:1496-1560: the LOD of the cell (x, y) and whether it is Changing -----------------
// lod_dist[n_lod] are the transition distances, lo / hi / centre_local the tile scene's box and centre before the cell's offset.
GSWT_HD inline void lod_select(const SurfaceParams& sp, int x, int y, V3 tile_center_world, const float* lod_dist, int n_lod, bool blending, bool bbox_check,
                               V3 lo, V3 hi, V3 centre_local, float ratio, float tol, V3 cam, int& lod, int& transition)
{
    int ccx, ccy;
    sp_map_to_coord(sp, x, y, ccx, ccy);
    const V3 pos_offset = sp_coord_to_pos(sp, ccx, ccy);
    const float center_dist = distance(tile_center_world, cam);
    int sel = n_lod - 1;
    for (int l = 0; l < n_lod; l++)
        if (center_dist <= lod_dist[l]) { sel = l; break; }
    int status = TR_NONE;
    if (blending) {
        float mn = -1.0f, mx = -1.0f;
        const int npts = bbox_check ? 8 : 1;
        for (int k = 0; k < npts; k++) {
            V3 p;
            if (bbox_check) p = V3{(k & 4) ? hi.x : lo.x, (k & 2) ? hi.y : lo.y, (k & 1) ? hi.z : lo.z};
            else p = centre_local;
            V3 q; M3 tr;
            surface_mapping(sp, x, y, p + pos_offset, true, q, tr);
            const float d = distance(q, cam);
            if (mn < 0.0f || d < mn) mn = d;
            if (mx < 0.0f || d > mx) mx = d;
        }
        if (sel > 0 && mn < lod_dist[sel - 1] * (1.0f + ratio) + tol) status = TR_CHANGING_HIGHER;
        if (sel < n_lod - 1 && mx > lod_dist[sel] * (1.0f - ratio) - tol) status = TR_CHANGING_LOWER;
    }
    lod = sel;
    transition = status;
}

// ---- border spawning, update_lod :1575-1605: the camera's place in the centre cell, then a border cell's factor ------------
GSWT_HD inline void spawning_cam_uv(const SurfaceParams& sp, V3 cam, float& cam_u, float& cam_v)
{
    const V3 cc = sp_coord_to_pos(sp, sp.center_x, sp.center_y);
    cam_u = (cam.x - cc.x) / sp.tile_width;
    cam_v = (cam.y - cc.y) / sp.tile_width;
}
GSWT_HD inline bool spawning_factor(const SurfaceParams& sp, bool blending, int x, int y, float cam_u, float cam_v, float& factor)     // true: the cell is Spawning
{
    factor = 0.0f;
    if (!blending || sp.surface_type == 2) return false;
    float bf = 1.0f;
    if (x == 0) bf *= 1.0f - cam_u;
    else if (x == sp.map_w - 1) bf *= cam_u;
    if (y == 0) bf *= 1.0f - cam_v;
    else if (y == sp.map_h - 1) bf *= cam_v;
    if (bf == 1.0f) return false;
    factor = bf;
    return true;
}

// ---- the edge between two neighbour cells -------------------------------------------------------------------------------
// Graph order, :1150-1165: which of the two is in front (+1: the edge's owner, -1: its neighbour, 0: no edge)
GSWT_HD inline int edge_direction(V3 edge_pos, V3 edge_normal, V3 cam)
{
    const V3 vd = edge_pos - cam;
    if (is_zero(vd)) return 0;
    const float dr = dot(edge_normal, vd);
    return dr > 0.0f ? 1 : (dr < 0.0f ? -1 : 0);
}
// selective_merge_edge, :860-905: whether the edge may merge its two cells; dabs is its sort key, ndot what the caller holds
// against merge_dot_threshold
GSWT_HD inline bool edge_candidate(V3 edge_pos, V3 edge_normal, V3 corner_a, V3 corner_b, V3 up_a, V3 up_b, V3 cam, const float* vp16, float& dabs, float& ndot)
{
    const V3 vd = edge_pos - cam;
    const float vlen = magnitude(vd);
    if (is_zero(vd)) return false;
    if (dot(vd, up_a) > 0.0f || dot(vd, up_b) > 0.0f) return false;
    const float a4[4] = {corner_a.x, corner_a.y, corner_a.z, 1.0f}, b4[4] = {corner_b.x, corner_b.y, corner_b.z, 1.0f};
    float p1[4], p2[4];
    mat4_vec(vp16, a4, p1);
    mat4_vec(vp16, b4, p2);
    const V3 q1 = V3{p1[0], p1[1], p1[2]} / p1[3], q2 = V3{p2[0], p2[1], p2[2]} / p2[3];
    const float clip = 1.0f;
    const bool o1 = q1.z < -clip || q1.x < -clip || q1.x > clip || q1.y < -clip || q1.y > clip;
    const bool o2 = q2.z < -clip || q2.x < -clip || q2.x > clip || q2.y < -clip || q2.y > clip;
    if (o1 && o2) return false;
    dabs = std::fabs(dot(edge_normal, vd));
    ndot = dabs / vlen;
    return true;
}

// ---- Distance / Viewport order key of a tile centre, :1029-1060 (larger = drawn earlier) ------------------------------------
GSWT_HD inline float order_key(int sort_type, V3 cam, const float* vp16, V3 centre)
{
    return sort_type == SORT_DISTANCE ? distance2(cam, centre) : (vp16[2] * centre.x + vp16[6] * centre.y) + vp16[10] * centre.z;
}

// ---- choose_presort_view, :700-716: the presort direction (dirs[n_view][3]) nearest to the view direction in tile space -------
GSWT_HD inline uint32_t choose_presort_view(const float* dirs, int n_view, const M3& transform, V3 pos, V3 cam)
{
    const V3 dl = transform * normalize(pos - cam);
    uint32_t best = 0;
    float best_err = 1000.0f;
    for (int i = 0; i < n_view; i++) {
        const float ex = dl.x - dirs[3 * i], ey = dl.y - dirs[3 * i + 1], ez = dl.z - dirs[3 * i + 2];
        const float err = (ex * ex + ey * ey) + ez * ez;
        if (err < best_err) { best = (uint32_t)i; best_err = err; }
    }
    return best;
}

// ---- the view of a merged group, :520-560: members added in merged_from order, then the averaged centre and rotation ------------
struct GroupView {
    bool merge_x = true, merge_y = true;        // every member in the head's column / row
    V3 sum_c;
    Quat sum_q;
};
GSWT_HD inline void group_view_add(GroupView& g, int head_x, int head_y, int x, int y, V3 tile_center, const M3& to_local)
{
    if (x != head_x) g.merge_x = false;
    if (y != head_y) g.merge_y = false;
    g.sum_c = g.sum_c + tile_center;
    const Quat q = quat_from_mat3(to_local);
    g.sum_q.s += q.s; g.sum_q.x += q.x; g.sum_q.y += q.y; g.sum_q.z += q.z;
}
GSWT_HD inline uint32_t group_view_finish(const GroupView& g, uint32_t n_members, const float* dirs, int n_view, V3 cam)
{
    if (!g.merge_x && !g.merge_y) return (uint32_t)n_view - 1u;
    const float n = (float)n_members;
    const Quat q{g.sum_q.s / n, g.sum_q.x / n, g.sum_q.y / n, g.sum_q.z / n};
    return choose_presort_view(dirs, n_view, mat3_from_quat(q), g.sum_c / n, cam);
}

// one member of a merged group; do_transition is raised when any member is in transition (:600-606)
GSWT_HD inline gswt_merge_member merge_member_of(uint32_t map_index, uint32_t lod, uint32_t tile, int transition, bool& do_transition)
{
    gswt_merge_member mm;
    mm.map_index = map_index; mm.lod = lod; mm.tile = tile; mm.other_lod = -1;
    if (transition == TR_CHANGING_LOWER) mm.other_lod = (int32_t)lod + 1;
    else if (transition == TR_CHANGING_HIGHER) mm.other_lod = (int32_t)lod - 1;
    if (transition != TR_NONE) do_transition = true;
    return mm;
}

// ---- one SortData record, :500-690, as an unmerged tile; the caller of a group head sets merged, merged_group / _offset /
// _count, single_lod_id and cache_hit from its own bookkeeping.  corner_pos[12] is read only where has_corner is set.
GSWT_HD inline gswt_sorted_tile sorted_tile_of(uint32_t lod, uint32_t tile, uint32_t view_id, V3 tile_offset, uint32_t map_index, int map_x, int map_y, V3 tile_center,
                                               int transition, float spawning_factor, uint32_t has_corner, const float* corner_pos, uint32_t key_len)
{
    gswt_sorted_tile st;
    memset(&st, 0, sizeof(st));
    st.lod = lod; st.tile = tile; st.view_id = view_id;
    st.tile_offset[0] = tile_offset.x; st.tile_offset[1] = tile_offset.y; st.tile_offset[2] = tile_offset.z;
    st.map_index = map_index; st.map_coord[0] = (uint32_t)map_x; st.map_coord[1] = (uint32_t)map_y;
    st.tile_center[0] = tile_center.x; st.tile_center[1] = tile_center.y; st.tile_center[2] = tile_center.z;
    st.transition = transition; st.spawning_factor = spawning_factor;
    st.has_corners = has_corner;
    for (int i = 0; i < 12; i++) st.corners[i] = has_corner ? corner_pos[i] : 0.0f;
    st.key_len = key_len;
    st.single_lod_id = -1;
    return st;
}

// ---- the draw of one record: renderer.rs:466-591 (host half) + TileUniforms::from_tile :691-725.  Returns ERR_* bits where the
// reference panics; the draw is filled all the same.
GSWT_HD inline uint32_t draw_from_tile(const gswt_sorted_tile& t, gswt_draw& d)
{
    uint32_t err = 0;
    memset(&d, 0, sizeof(d));
    gswt_tile_uniforms& u = d.tile;
    u.single_draw = 0; u.map_index = t.map_index; u.single_lod_id = -1; u.valid_lod_id = -1; u.changing = 0; u.changing_to_lower = -1;
    u.tile_id[0] = t.lod; u.tile_id[1] = t.tile; u.tile_id[2] = t.view_id; u.tile_id[3] = 0;
    u.offset[0] = t.tile_offset[0]; u.offset[1] = t.tile_offset[1]; u.offset[2] = t.tile_offset[2]; u.offset[3] = 0.0f;
    u.map_coord[0] = t.map_coord[0]; u.map_coord[1] = t.map_coord[1];
    d.lod = t.lod;
    if (t.merged) {
        u.single_draw = 1;
        u.single_lod_id = t.single_lod_id;
        u.changing = t.single_lod_id == -1 ? 1u : 0u;
        d.merged = 1; d.merged_offset = t.merged_offset; d.merged_count = t.merged_count; d.merged_group = t.merged_group;
        d.merged_has_lod = t.single_lod_id == -1 ? 1u : 0u;
    } else {
        d.base_lod = t.lod;
        if (t.transition == TR_CHANGING_LOWER) { u.changing = 1; u.changing_to_lower = 1; }
        else if (t.transition == TR_CHANGING_HIGHER) {
            u.changing = 1; u.changing_to_lower = 0;
            if (t.lod == 0) err |= ERR_LOD0_HIGHER;         // index underflow in the reference
            d.base_lod = t.lod - 1;
        } else u.valid_lod_id = (int32_t)t.lod;
        d.base_tile = t.tile; d.base_view = t.view_id;
    }
    if (t.key_len == 1) {                                   // viewport culling only for non-merged tiles, :472
        if (!t.has_corners) err |= ERR_NO_CORNERS;         // corner_data is None
        d.cull_enable = 1;
        for (int i = 0; i < 12; i++) d.corners[i] = t.corners[i];
    }
    return err;
}

}  // namespace gswt_host
