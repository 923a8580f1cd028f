// gswt_api.hip -- C ABI of libgswt_hip.so (include/gswt_hip.h): context, HBM buffers, frame slots (up to five frames in flight,
// each on its own stream with its own per-frame buffers), draw sets (one per frame in flight + 1, filled by sort events on a stream
// of their own) and the per-frame launch sequence
// cull -> project -> totals -> emit -> sort -> ranges -> items -> composite -> combine, launched kernel by kernel or replayed as one
// hipGraphLaunch (GSWT_OPT_GRAPH); background passes; sharding; the framebuffer gather (RCCL or peer copies).
//
// HBM layout (all resident, sized for a 288 GB part; nothing is re-uploaded per frame):
//   tex          U x 32 B      packed splat records, exactly Scene.tex_data (scene.rs:306-411)
//   static_list  4 B / entry   every base list [lod][tile][view], entry = gs_index | lod_id << 28,
//                              stored twice: interleaved (as the reference binds it) and
//                              LOD-filtered (what survives A1 for a plain tile)
//   merged_*     4+4 B / entry per-sort-event merged-group lists (gs_index|lod, map_id)
//   draws        DrawDev[]     one per reference draw call; chunk_tab maps a 256-entry workgroup
//                              to (draw, first entry)
//   rects/recs   8 + 32 B / slot  per-frame projection output, slot = composite order (+ 4 B depth side array when depth-tested)
//   keys/vals    2 x (4+4) B / pair  ping-pong for the tile sort
#include "gswt_ctx.h"
#include "host/gswt_surface.h"

#include <algorithm>
#include <limits>
#include <memory>

using namespace gswt;

// The host side of the library by subsystem: this file keeps the context's lifetime, the options, gswt_configure, the whole frame path
// (validate_frame .. gswt_render_fence, graph replay included: its helpers are static and inline into each other, and the per-frame host
// time is part of the benchmark) and the frame debug readers.  gswt_api_scene.hip: the scene uploads; gswt_api_draws.hip: sort events;
// gswt_api_passes.hip: skybox and proxy; gswt_api_comm.hip: sharding and the two gather transports.  gswt_ctx.h is what they share.

static int finish_frame(gswt_ctx* c, FrameSlot& sl);

void gswt::collect_slot(gswt_ctx* c, FrameSlot& sl)
{
    if (!sl.pending || sl.collected) return;
    sl.collected_rc = finish_frame(c, sl);
    sl.collected_timings = c->timings;
    sl.collected = true;
}

hipError_t gswt::collect_pending(gswt_ctx* c)
{
    for (auto& sl : c->slots) collect_slot(c, sl);
    return sync_all(c);
}

// Hands back what a collected slot left (gswt_render_wait, and gswt_render_async when it reuses the oldest slot): the ticket is
// spent, and the frame's status and timings are the ones finish_frame produced -- just now, or earlier for a fence / a state change.
static int take_slot(gswt_ctx* c, FrameSlot& sl)
{
    sl.pending = false;
    if (!sl.collected) return finish_frame(c, sl);
    sl.collected = false;
    c->timings = sl.collected_timings;
    return sl.collected_rc;
}

gswt_ctx::~gswt_ctx()
{
    if (comm) rccl_comm_destroy(comm);
    if (ev_push) hipEventDestroy(ev_push);
    if (ev_unshard) hipEventDestroy(ev_unshard);
    for (auto& ds : sets)
        if (ds.ev_up) hipEventDestroy(ds.ev_up);
    for (auto& sl : slots) {
        sl.release_graph();
        for (auto& e : sl.ev) if (e) hipEventDestroy(e);
        if (sl.ev_in) hipEventDestroy(sl.ev_in);
        if (sl.ev_gather) hipEventDestroy(sl.ev_gather);
        if (sl.hc) hipHostFree(sl.hc);
        if (sl.stream) hipStreamDestroy(sl.stream);
    }
    if (own_stream && stream) hipStreamDestroy(stream);
    if (set_stream) hipStreamDestroy(set_stream);
    for (hipStream_t ps : pad_streams) hipStreamDestroy(ps);
}

extern "C" {

int gswt_create(int device_id, gswt_ctx** out)
try {
    if (!out) return GSWT_ERR_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return GSWT_ERR_HIP;
    if (device_id < 0 || device_id >= ndev) return GSWT_ERR_BAD_ARG;
    if (hipSetDevice(device_id) != hipSuccess) return GSWT_ERR_HIP;
    std::unique_ptr<gswt_ctx> c(new (std::nothrow) gswt_ctx());      // (a failure below returns through ~gswt_ctx: nothing created so far leaks)
    if (!c) return GSWT_ERR_CAPACITY;
    c->device = device_id;
    // Stream creation order matters: the runtime spreads streams over 4 hardware queues (GPU_MAX_HW_QUEUES) in creation order, and
    // streams that share a queue run one behind the other.  The layout string names the order: c = ctx stream, 0-4 = frame slot
    // streams, s = the stream of the sort-event builds, p = a placeholder that is never used; a slot stream the string leaves out is
    // created when that slot is first used.  (GSWT_STREAM_LAYOUT overrides it: tuning only.)
    const char* layout = getenv("GSWT_STREAM_LAYOUT");
    if (!layout || !*layout) layout = kStreamLayout;
    for (const char* q = layout; *q; q++) {
        hipStream_t* dst = nullptr;
        hipStream_t pad = nullptr;
        if (*q == 'c') dst = &c->stream;
        else if (*q == 's') dst = &c->set_stream;
        else if (*q >= '0' && *q < '0' + kFrameSlots) dst = &c->slots[*q - '0'].stream;
        else if (*q == 'p') dst = &pad;
        else continue;
        if (*dst) continue;
        if ((q[1] == '+' || q[1] == '-')) {                   // "s+" / "s-": highest / lowest stream priority (tuning experiments)
            int lo = 0, hi = 0;
            hipDeviceGetStreamPriorityRange(&lo, &hi);          // lo = least, hi = greatest priority (numerically lower)
            if (hipStreamCreateWithPriority(dst, hipStreamNonBlocking, q[1] == '+' ? hi : lo) != hipSuccess) return GSWT_ERR_HIP;
        } else
        if (hipStreamCreateWithFlags(dst, hipStreamNonBlocking) != hipSuccess) return GSWT_ERR_HIP;
        if (dst == &pad) c->pad_streams.push_back(pad);
    }
    if (!c->stream && hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return GSWT_ERR_HIP;
    if (!c->set_stream && hipStreamCreateWithFlags(&c->set_stream, hipStreamNonBlocking) != hipSuccess) return GSWT_ERR_HIP;
    for (auto& sl : c->slots) {
        if (hipEventCreateWithFlags(&sl.ev_in, hipEventDisableTiming) != hipSuccess) return GSWT_ERR_HIP;
        if (hipEventCreate(&sl.ev_gather) != hipSuccess) return GSWT_ERR_HIP;
        for (auto& e : sl.ev)
            if (hipEventCreate(&e) != hipSuccess) return GSWT_ERR_HIP;
        if (hipHostMalloc(reinterpret_cast<void**>(&sl.hc), sizeof(FrameResult), hipHostMallocMapped) != hipSuccess) return GSWT_ERR_HIP;
        memset(sl.hc, 0, sizeof(FrameResult));
        if (hipHostGetDevicePointer(reinterpret_cast<void**>(&sl.hc_dev), sl.hc, 0) != hipSuccess) sl.hc_dev = nullptr;   // then the copy stays
    }
    *out = c.release();
    return GSWT_OK;
} GSWT_CATCH

void gswt_destroy(gswt_ctx* c)
{
    if (!c) return;
    hipSetDevice(c->device);
    sync_all(c);
    for (gswt_ctx* m : std::vector<gswt_ctx*>(c->group))       // leave a peer-copy group before the memory goes away
        if (m && m != c) m->group.clear();
    c->group.clear();
    delete c;
}

const char* gswt_last_error(const gswt_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int gswt_set_stream(gswt_ctx* c, void* hip_stream)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    collect_pending(c);
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    if (hip_stream) { c->stream = (hipStream_t)hip_stream; c->own_stream = false; return GSWT_OK; }
    c->stream = nullptr; c->own_stream = true;            // NULL: back to a stream of the ctx's own
    hipSetDevice(c->device);
    HIP_TRY(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    return GSWT_OK;
} GSWT_CATCH

int gswt_set_option(gswt_ctx* c, int key, int value)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    switch (key) {
    case GSWT_OPT_NO_LOD_PREFILTER: c->opt.no_prefilter = value; c->draws_ready = false; return GSWT_OK;
    case GSWT_OPT_DEBUG_VARYINGS: c->opt.debug_varyings = value; return GSWT_OK;
    case GSWT_OPT_DEBUG_FLAGS:          // reserved
        if (value != 0) return fail(c, GSWT_ERR_BAD_ARG, "GSWT_OPT_DEBUG_FLAGS is reserved: only 0 is accepted");
        return GSWT_OK;
    case GSWT_OPT_TIMING: c->opt.timing = value; return GSWT_OK;
    case GSWT_OPT_NO_MERGE_REUSE: c->opt.no_merge_reuse = value; return GSWT_OK;
    case GSWT_OPT_DEFER_SWAP: c->opt.defer_swap = value; return GSWT_OK;
    case GSWT_OPT_GRAPH: c->opt.graph = value; return GSWT_OK;
    case GSWT_OPT_STRICT_VS: c->opt.strict_vs = value != 0; return GSWT_OK;
    case GSWT_OPT_PROJECTION:
        if (value != 0 && value != 1) return fail(c, GSWT_ERR_BAD_ARG, "GSWT_OPT_PROJECTION: 0 (perspective) or 1 (orthographic), not %d", value);
        c->opt.projection = value; return GSWT_OK;
    case GSWT_OPT_ANTIALIAS:
        if (value < 0 || value > 4096) return fail(c, GSWT_ERR_BAD_ARG, "GSWT_OPT_ANTIALIAS: 0 (off) or 1..4096 (filter variance in 1/1024 px^2), not %d", value);
        c->opt.antialias = value; return GSWT_OK;
    case GSWT_OPT_COMPOSITE:
        // (1: once the decoupled-waves compositor, 2: once k_composite<FOLD>; both removed, DESIGN.md sections 6 and 10.  Accepted, without effect.)
        if (value < 0 || value > 2) return fail(c, GSWT_ERR_BAD_ARG, "unknown compositor variant %d", value);
        return GSWT_OK;
    case GSWT_OPT_NO_CHUNK_CULL: c->opt.no_chunk_cull = value != 0; return GSWT_OK;
    case GSWT_OPT_ITEM_ORDER: return GSWT_OK;      // (once heaviest-first work items; removed.  Accepted, without effect.)
    case GSWT_OPT_DEPTH_SORT:
        if (value < 0 || value > 2) return fail(c, GSWT_ERR_BAD_ARG, "GSWT_OPT_DEPTH_SORT: 0 (auto), 1 (global passes) or 2 (tile-local)");
        c->opt.depth_sort = value; c->depth_max_tile_len = 0;
        return GSWT_OK;
    case GSWT_OPT_DEPTH_PASSES:
        if (value < 1 || value > 4) return fail(c, GSWT_ERR_BAD_ARG, "depth-sort passes must be 1..4");
        c->depth_passes = (uint32_t)value; c->depth_passes_low_run = 0;
        return GSWT_OK;
    case GSWT_OPT_PAIR_CAP:
        if (value < 0) return fail(c, GSWT_ERR_BAD_ARG, "pair capacity must be >= 0");
        c->opt.fixed_pair_cap = value > 0; if (value > 0) c->pair_cap = (uint32_t)value;
        return GSWT_OK;
    case GSWT_OPT_SEGMENT:
        if (value < 256 || value % 256) return fail(c, GSWT_ERR_BAD_ARG, "segment must be a positive multiple of 256");
        c->opt.segment = value; return GSWT_OK;
    default: return fail(c, GSWT_ERR_BAD_ARG, "unknown option %d", key);
    }
} GSWT_CATCH

int gswt_set_atmosphere(gswt_ctx* c, const gswt_atmosphere* a)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    if (!a) { c->atm = gswt_atmosphere{}; return GSWT_OK; }
    const float inf = std::numeric_limits<float>::infinity();
    const struct { const char* name; float v; } fields[] = {
        {"fade_start", a->fade_start}, {"fade_end", a->fade_end}, {"fog_density", a->fog_density}, {"fog_start", a->fog_start},
        {"fog_max", a->fog_max}, {"fog_color[0]", a->fog_color[0]}, {"fog_color[1]", a->fog_color[1]}, {"fog_color[2]", a->fog_color[2]}};
    for (const auto& fd : fields)
        if (!(std::fabs(fd.v) < inf)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_atmosphere: %s = %g is not finite", fd.name, fd.v);
    if (a->fade_start != 0.0f || a->fade_end != 0.0f) {
        if (!(a->fade_start >= 0.0f)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_atmosphere: fade_start = %g, not >= 0", a->fade_start);
        if (!(a->fade_end > a->fade_start))
            return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_atmosphere: fade_end = %g, not above fade_start = %g", a->fade_end, a->fade_start);
        const float inv = 1.0f / (a->fade_end - a->fade_start);
        if (!(std::fabs(inv) < inf))
            return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_atmosphere: fade_end - fade_start = %g is too small: 1 / it is not finite", a->fade_end - a->fade_start);
    }
    if (!(a->fog_density >= 0.0f)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_atmosphere: fog_density = %g, not 0 (off) or > 0", a->fog_density);
    if (!(a->fog_start >= 0.0f)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_atmosphere: fog_start = %g, not >= 0", a->fog_start);
    if (a->fog_density > 0.0f && !(a->fog_max > 0.0f && a->fog_max <= 1.0f))
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_atmosphere: fog_max = %g, not in (0, 1]", a->fog_max);
    for (int k = 0; k < 3; k++)
        if (!(a->fog_color[k] >= 0.0f && a->fog_color[k] <= 1.0f))
            return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_atmosphere: fog_color[%d] = %g, not in [0, 1]", k, a->fog_color[k]);
    c->atm = *a;
    return GSWT_OK;
} GSWT_CATCH

int gswt_set_tile_styles(gswt_ctx* c, const gswt_tile_style* styles, size_t n_styles)
try {
    static_assert(sizeof(gswt_tile_style) == 8 && sizeof(uint2) == 8, "k_project reads an entry as one uint2: (tint | tint_strength << 24, dim)");
    if (!c) return GSWT_ERR_BAD_ARG;
    if (!styles && n_styles > 0) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_tile_styles: styles is NULL with n_styles = %zu", n_styles);
    if (n_styles > ((size_t)1 << 20)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_tile_styles: n_styles = %zu, more than 1 << 20 map cells", n_styles);
    bool on = false;
    for (size_t i = 0; i < n_styles; i++) {
        const gswt_tile_style& e = styles[i];
        if (e._pad[0] | e._pad[1] | e._pad[2])
            return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_tile_styles: styles[%zu]._pad = (%u, %u, %u), must be zero", i, e._pad[0], e._pad[1], e._pad[2]);
        on = on || e.tint_strength != 0 || e.dim != 0;
    }
    if (!on) { c->styles.off(); return GSWT_OK; }
    const int v = c->styles.free_version(c->slots, &FrameModes::sty_ver);
    if (v < 0) return fail(c, GSWT_ERR_STATE, "gswt_set_tile_styles: no free table version");
    hipSetDevice(c->device);
    StyleVersion* sv = nullptr;
    HIP_TRY(c, c->styles.begin_fill(v, &sv));
    // (buffers grow to twice the request: a host that sets a table per frame allocates once per version)
    if (n_styles > sv->h.cap) HIP_TRY(c, sv->h.ensure(2 * n_styles));
    HIP_TRY(c, sv->d.ensure_roomy(n_styles));
    memcpy(sv->h.p, styles, n_styles * sizeof(gswt_tile_style));
    // (on the ctx stream: a copy on the null stream would synchronise with every blocking stream)
    HIP_TRY(c, hipMemcpyAsync(sv->d.p, sv->h.p, n_styles * sizeof(gswt_tile_style), hipMemcpyHostToDevice, c->stream));
    sv->n = (uint32_t)n_styles;
    HIP_TRY(c, c->styles.commit(v, c->stream));
    return GSWT_OK;
} GSWT_CATCH

int gswt_set_shadow_map(gswt_ctx* c, const gswt_shadow_params* p, const float* depth, int width, int height, int depth_on_device)
try {
    static_assert(sizeof(gswt_shadow_params) == 96, "gswt_shadow_params layout");
    if (!c) return GSWT_ERR_BAD_ARG;
    if (!p || !depth) { c->shadows.off(); return GSWT_OK; }
    const float inf = std::numeric_limits<float>::infinity();
    const float* M = p->world_to_light;
    for (int k = 0; k < 16; k++)
        if (!(std::fabs(M[k]) < inf)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_shadow_map: world_to_light[%d] = %g is not finite", k, M[k]);
    const struct { const char* name; float v; } fields[] = {
        {"bias", p->bias}, {"strength", p->strength}, {"shade_color[0]", p->shade_color[0]}, {"shade_color[1]", p->shade_color[1]},
        {"shade_color[2]", p->shade_color[2]}};
    for (const auto& fd : fields)
        if (!(std::fabs(fd.v) < inf)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_shadow_map: %s = %g is not finite", fd.name, fd.v);
    if (!(M[3] == 0.0f && M[7] == 0.0f && M[11] == 0.0f && M[15] == 1.0f))
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_shadow_map: world_to_light needs the bottom row (0, 0, 0, 1), not (%g, %g, %g, %g)", M[3], M[7], M[11], M[15]);
    if (!(p->bias >= 0.0f)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_shadow_map: bias = %g, not >= 0", p->bias);
    if (!(p->strength > 0.0f && p->strength <= 1.0f)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_shadow_map: strength = %g, not in (0, 1]", p->strength);
    for (int k = 0; k < 3; k++)
        if (!(p->shade_color[k] >= 0.0f && p->shade_color[k] <= 1.0f))
            return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_shadow_map: shade_color[%d] = %g, not in [0, 1]", k, p->shade_color[k]);
    if (p->_pad[0] | p->_pad[1] | p->_pad[2])
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_shadow_map: _pad = (%u, %u, %u), must be zero", p->_pad[0], p->_pad[1], p->_pad[2]);
    if (width < 1 || width > 4096) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_shadow_map: width = %d, not in 1..4096", width);
    if (height < 1 || height > 4096) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_shadow_map: height = %d, not in 1..4096", height);
    const int v = c->shadows.free_version(c->slots, &FrameModes::shd_ver);
    if (v < 0) return fail(c, GSWT_ERR_STATE, "gswt_set_shadow_map: no free map version");
    const size_t n = (size_t)width * height;
    hipSetDevice(c->device);
    ShadowVersion* sv = nullptr;
    HIP_TRY(c, c->shadows.begin_fill(v, &sv));
    // (buffers grow to twice the request, like the styles': growing frees the old buffer, which waits for the device, so a host whose image
    // sizes creep upwards stalls once per version and doubling, not at every set)
    HIP_TRY(c, sv->d.ensure_roomy(n));
    // (on the ctx stream, like the styles' copy: an earlier proxy pass that read this version is on the same stream, in front of the copy)
    if (depth_on_device)
        HIP_TRY(c, hipMemcpyAsync(sv->d.p, depth, n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    else {
        if (n > sv->h.cap) HIP_TRY(c, sv->h.ensure(2 * n));
        memcpy(sv->h.p, depth, n * sizeof(float));
        HIP_TRY(c, hipMemcpyAsync(sv->d.p, sv->h.p, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    Shadow& k = sv->p;
    k = Shadow{};
    for (int r = 0; r < 3; r++)
        for (int j = 0; j < 4; j++) k.row[r][j] = M[4 * j + r];
    k.bias = p->bias; k.strength = p->strength;
    for (int j = 0; j < 3; j++) k.shade[j] = p->shade_color[j];
    k.w = width; k.h = height; k.z = sv->d.p;
    HIP_TRY(c, c->shadows.commit(v, c->stream));
    return GSWT_OK;
} GSWT_CATCH

int gswt_set_clip_volumes(gswt_ctx* c, const gswt_clip_volume* v, size_t n)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    if (!v && n > 0) return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_clip_volumes: v is NULL with n = %zu", n);
    if (n > (size_t)GSWT_MAX_CLIP_VOLUMES)
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_clip_volumes: n = %zu, more than GSWT_MAX_CLIP_VOLUMES = %d", n, GSWT_MAX_CLIP_VOLUMES);
    const float inf = std::numeric_limits<float>::infinity();
    ClipSet s = {};
    for (size_t i = 0; i < n; i++) {
        const gswt_clip_volume& e = v[i];
        if (e.shape > GSWT_CLIP_HALFSPACE)
            return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_clip_volumes: v[%zu].shape = %u, not GSWT_CLIP_BOX, _ELLIPSOID or _HALFSPACE", i, e.shape);
        if (e.flags & ~(GSWT_CLIP_KEEP | GSWT_CLIP_GROUND))
            return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_clip_volumes: v[%zu].flags = 0x%x has bits beyond GSWT_CLIP_KEEP | GSWT_CLIP_GROUND", i, e.flags);
        if (e.reserved[0] | e.reserved[1])
            return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_clip_volumes: v[%zu].reserved = (%u, %u), must be zero", i, e.reserved[0], e.reserved[1]);
        // (a half-space reads row 2 alone: what its rows 0 and 1 hold is not looked at, and travels as zeros)
        for (int k = e.shape == GSWT_CLIP_HALFSPACE ? 8 : 0; k < 12; k++)
            if (!(std::fabs(e.world_to_unit[k]) < inf))
                return fail(c, GSWT_ERR_BAD_ARG, "gswt_set_clip_volumes: v[%zu].world_to_unit[%d] = %g is not finite", i, k, e.world_to_unit[k]);
        ClipVolume& q = s.v[i];
        for (int k = e.shape == GSWT_CLIP_HALFSPACE ? 8 : 0; k < 12; k++) q.row[k / 4][k % 4] = e.world_to_unit[k];
        q.shape = e.shape; q.flags = e.flags;
        s.n_keep += (e.flags & GSWT_CLIP_KEEP) ? 1u : 0u;
    }
    s.n = (uint32_t)n;
    c->clip = s;              // by value: frames already submitted keep their own copy (FrameModes), nothing to wait for
    return GSWT_OK;
} GSWT_CATCH

int gswt_configure(gswt_ctx* c, const float* height_map, int hm_w, int hm_h)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    hipSetDevice(c->device);
    HIP_TRY(c, collect_pending(c));
    if (!height_map || hm_w <= 0 || hm_h <= 0) { c->hm_w = c->hm_h = 0; return GSWT_OK; }
    HIP_TRY(c, c->hmap.ensure((size_t)hm_w * hm_h + 2));         // + padding: sample_height (k_project, k_proxy) loads a row's two texels as 8 bytes
    HIP_TRY(c, hipMemcpy(c->hmap.p, height_map, (size_t)hm_w * hm_h * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemset(c->hmap.p + (size_t)hm_w * hm_h, 0, 8));
    {
        float mn = height_map[0], mx = height_map[0], du = 0.f, dv = 0.f;
        bool finite = true;
        for (int y = 0; y < hm_h; y++)
            for (int x = 0; x < hm_w; x++) {
                const float h = height_map[(size_t)y * hm_w + x];
                const float hr = height_map[(size_t)y * hm_w + (x + 1 == hm_w ? 0 : x + 1)], hd = height_map[(size_t)(y + 1 == hm_h ? 0 : y + 1) * hm_w + x];
                if (!gswt_host::finite_coord(h)) finite = false;
                mn = std::min(mn, h); mx = std::max(mx, h);
                du = std::max(du, std::fabs(hr - h)); dv = std::max(dv, std::fabs(hd - h));
            }
        c->hm_min = mn; c->hm_max = mx; c->hm_du = du * (float)hm_w; c->hm_dv = dv * (float)hm_h;
        if (!finite) { c->hm_min = -3e38f; c->hm_max = 3e38f; c->hm_du = c->hm_dv = 3e38f; }      // the band cull then keeps everything
    }
    HIP_TRY(c, null_stream_done());
    c->hm_w = hm_w; c->hm_h = hm_h;
    return GSWT_OK;
} GSWT_CATCH

}  // extern "C"

// ---- frame machinery ------------------------------------------------------------------------------
// GSWT_OPT_ANTIALIAS: s = 4 v / splat_scale^2 with v = value / 1024 (exact), one binary32 operation per operator (include/gswt_hip.h)
static float antialias_s(int value, float splat_scale) { return (4.0f * ((float)value / 1024.0f)) / (splat_scale * splat_scale); }

// What a frame submitted now keeps from the context (submit_frame; validate_frame_modes has accepted it, so s is a finite positive number).
static FrameModes frame_modes(const gswt_ctx& c, const gswt_scene_uniforms& su)
{
    const float aa_s = c.opt.antialias > 0 ? antialias_s(c.opt.antialias, su.splat_scale) : 0.0f;
    return FrameModes{c.opt.strict_vs != 0, c.opt.projection == 1, aa_s, atmo_constants(c.atm), c.styles.cur, c.shadows.cur, c.clip};
}

// The preconditions of the modes a frame submitted now would run with.  Every mode exists in the strict vertex stage only (project_modes,
// gswt_frame_modes.h); the orthographic projection and the pixel filter also constrain the frame's uniforms.
static int validate_frame_modes(gswt_ctx* c, const gswt_camera_uniforms* cam, const gswt_scene_uniforms* su, const ShardGeom& g)
{
    const float inf = std::numeric_limits<float>::infinity();
    const bool ortho = c->opt.projection == 1, aa = c->opt.antialias > 0;
    if (ortho) {
        // the projection must be affine (clip w = 1 exactly) and focal is pixels per world unit
        const float* P = cam->projection;
        if (!(P[3] == 0.0f && P[7] == 0.0f && P[11] == 0.0f && P[15] == 1.0f))
            return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: GSWT_OPT_PROJECTION = 1 needs an affine projection, bottom row (0, 0, 0, 1), not (%g, %g, %g, %g)",
                        P[3], P[7], P[11], P[15]);
        for (int k = 0; k < 2; k++)
            if (!(cam->focal[k] > 0.0f) || !(cam->focal[k] < inf))
                return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: GSWT_OPT_PROJECTION = 1 needs a finite focal > 0 (pixels per world unit), not focal[%d] = %g", k, cam->focal[k]);
    }
    // (mode is on, who needs the strict sequence, which form the v2 sequence lacks); the first one on is refused, so what follows checks a strict frame
    const struct { bool on; const char* who; const char* form; } modes[] = {
        {ortho, "GSWT_OPT_PROJECTION = 1", "orthographic"},
        {aa, "GSWT_OPT_ANTIALIAS > 0", "filtered"},
        {c->atm.fade_end > 0.0f || c->atm.fog_density > 0.0f, "gswt_set_atmosphere's fade or fog", "atmospheric"},
        {c->styles.cur >= 0, "gswt_set_tile_styles' table", "styled"},
        {c->shadows.cur >= 0, "gswt_set_shadow_map's map", "shadowed"},
        {c->clip.n > 0u, "gswt_set_clip_volumes' set", "clipped"}};
    for (const auto& m : modes)
        if (m.on && !c->opt.strict_vs)
            return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: %s needs GSWT_OPT_STRICT_VS = 1 (the v2 sequence has no %s form)", m.who, m.form);
    if (ortho && g.cols)
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: GSWT_OPT_PROJECTION = 1 does not take column-band shards (their band cull is perspective-only); use GSWT_SHARD_ROWS");
    if (aa) {
        // s = 4 v / splat_scale^2 needs a splat_scale, and one whose square neither overflows (s = 0: the filter would switch off silently)
        // nor underflows (s = inf: every alpha 0)
        if (su->splat_scale == 0.0f || !(std::fabs(su->splat_scale) < inf))
            return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: GSWT_OPT_ANTIALIAS > 0 needs a finite splat_scale != 0, not %g", su->splat_scale);
        const float s = antialias_s(c->opt.antialias, su->splat_scale);
        if (!(s > 0.0f && s < inf))
            return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: GSWT_OPT_ANTIALIAS = %d with splat_scale %g gives s = 4 v / splat_scale^2 = %g, not a finite positive number",
                        c->opt.antialias, su->splat_scale, s);
    }
    return GSWT_OK;
}

// A frame is enqueued without any host round trip (enqueue_frame) and collected later (finish_frame).
// gswt_render = enqueue + finish; gswt_render_async / gswt_render_wait expose the two halves so a caller
// can queue frame i+1 before collecting frame i (two slots, same stream, executed in order).
static int validate_frame(gswt_ctx* c, const gswt_camera_uniforms* cam, const gswt_scene_uniforms* su, const gswt_render_config* cfg,
                          int width, int height, const void* out_rgba)
{
    if (!cam || !su || !cfg || !out_rgba) return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: null argument");
    if (!c->draws_ready) return fail(c, GSWT_ERR_STATE, "gswt_render before gswt_set_draws");
    if (width <= 0 || height <= 0 || width > 65535 * kTile || height > 65535 * kTile)
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: bad target size %dx%d", width, height);
    if ((float)width != cam->viewport[0] || (float)height != cam->viewport[1])
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: camera viewport (%g,%g) != target %dx%d", cam->viewport[0], cam->viewport[1], width, height);
    if (su->surface_type == 1u && (c->hm_w == 0 || c->hm_h == 0))
        return fail(c, GSWT_ERR_STATE, "gswt_render: surface_type HeightMap without gswt_configure height map");
    if (su->surface_type > 2u) return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: unknown surface_type %u", su->surface_type);
    if (su->surface_type == 2u && (su->map_half_wh[0] == 0u || su->map_half_wh[1] == 0u))
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: Sphere surface needs a non-empty map");
    if (su->draw_mode > 4u) return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: unknown draw_mode %u", su->draw_mode);
    if (cfg->order_mode != GSWT_ORDER_REFERENCE && cfg->order_mode != GSWT_ORDER_DEPTH)
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: unknown order mode %d", cfg->order_mode);
    const ShardGeom g = shard_geom(*cfg, width, height);
    if (g.world > 1 && (cfg->shard_index < 0 || cfg->shard_index >= g.world)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: bad shard index");
    if (cfg->shard_mode != GSWT_SHARD_ROWS && cfg->shard_mode != GSWT_SHARD_COLUMNS) return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: unknown shard mode %d", cfg->shard_mode);
    if (cfg->out_format > (uint32_t)kOutI420 || out_image_bytes((int)cfg->out_format, 2, 2) == 0)
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: unknown out_format %u", cfg->out_format);
    if (out_is_video((int)cfg->out_format) && ((width | height) & 1))
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_render: the video formats need an even target size, not %dx%d", width, height);
    return validate_frame_modes(c, cam, su, g);
}

// GSWT_OPT_GRAPH: the frame's launch sequence was recorded, not launched (gswt_device.h); replay it as one hipGraphLaunch on the
// slot's stream.  The graph is a chain of kernel nodes; it is rebuilt when the sequence of kernels changes (another template
// variant, a k_radix_supscan more or less) and otherwise only the nodes whose grid or arguments differ from the previous frame of
// this slot are updated in the executable graph: with a moving camera the five kernels that take the frame constants, after a
// sort event also those that take draw-set pointers or sizes.
static int replay_graph(gswt_ctx* c, FrameSlot& sl)
{
    GraphRec& R = sl.grec;
    if (R.overflow || R.n == 0) return fail(c, GSWT_ERR_STATE, "gswt_render: frame graph record overflow");
    bool rebuild = !sl.graph_exec || sl.graph_n != R.n;
    for (uint32_t i = 0; !rebuild && i < R.n; i++) rebuild = sl.graph_last[i].fn != R.nodes[i].fn;
    void* ptrs[40];
    auto fill = [&](GraphNodeRec& nd, hipKernelNodeParams& kp) {
        memset(&kp, 0, sizeof(kp));
        for (uint32_t a = 0; a < nd.n_args; a++) ptrs[a] = nd.args + nd.offs[a];
        kp.func = const_cast<void*>(nd.fn);
        kp.gridDim = nd.grid; kp.blockDim = nd.block; kp.sharedMemBytes = 0;
        kp.kernelParams = ptrs; kp.extra = nullptr;
    };
    if (rebuild) {
        sl.release_graph();
        HIP_TRY(c, hipGraphCreate(&sl.graph, 0));
        for (uint32_t i = 0; i < R.n; i++) {
            hipKernelNodeParams kp;
            fill(R.nodes[i], kp);
            HIP_TRY(c, hipGraphAddKernelNode(&sl.graph_nodes[i], sl.graph, i ? &sl.graph_nodes[i - 1] : nullptr, i ? 1 : 0, &kp));
            sl.graph_last[i] = R.nodes[i];
        }
        HIP_TRY(c, hipGraphInstantiate(&sl.graph_exec, sl.graph, nullptr, nullptr, 0));
        sl.graph_n = R.n;
        c->stat_graph_rebuilds++;
    } else {
        for (uint32_t i = 0; i < R.n; i++) {
            if (sl.graph_last[i].same(R.nodes[i])) continue;
            hipKernelNodeParams kp;
            fill(R.nodes[i], kp);
            HIP_TRY(c, hipGraphExecKernelNodeSetParams(sl.graph_exec, sl.graph_nodes[i], &kp));
            sl.graph_last[i] = R.nodes[i];
            c->stat_graph_node_updates++;
        }
    }
    HIP_TRY(c, hipGraphLaunch(sl.graph_exec, sl.stream));
    c->stat_graph_launches++;
    return GSWT_OK;
}

// The frame constants of k_cull .. k_combine: the uniforms as the kernels read them, the screen tiles of the frame's shard and the
// band-cull bounds of a column shard.  Host arithmetic only.
static Frame make_frame(const gswt_ctx& c, const FrameArgs& a, const ShardGeom& g)
{
    const gswt_camera_uniforms* cam = &a.cam;
    const gswt_scene_uniforms* su = &a.su;
    const gswt_render_config* cfg = &a.cfg;
    const int width = a.width, height = a.height;
    Frame f;
    memset(&f, 0, sizeof(f));
    memcpy(f.V, cam->view, 64);
    gl_to_wgpu_projection(cam->projection, f.GP);
    gswt_host::mat4_mul(cam->projection, cam->view, f.VP);
    f.focal[0] = cam->focal[0]; f.focal[1] = cam->focal[1];
    f.htan[0] = cam->htan_fov[0]; f.htan[1] = cam->htan_fov[1];
    f.cam_pos[0] = cam->cam_pos[0]; f.cam_pos[1] = cam->cam_pos[1]; f.cam_pos[2] = cam->cam_pos[2];
    f.W = (float)width; f.H = (float)height;
    f.splat_scale = su->splat_scale; f.tile_width = su->tile_width; f.clip_height = su->clip_height;
    f.point_cloud_radius = su->point_cloud_radius; f.transition_width_ratio = su->transition_width_ratio;
    f.sphere_radius = su->sphere_radius;
    f.use_clip = su->use_clip; f.surface_type = su->surface_type; f.num_lod = su->num_lod; f.draw_mode = su->draw_mode;
    f.map_half_wh[0] = su->map_half_wh[0]; f.map_half_wh[1] = su->map_half_wh[1];
    f.center_coord[0] = su->center_coord[0]; f.center_coord[1] = su->center_coord[1];
    memcpy(f.transition_dist, su->transition_dist_vec, 64);
    for (int k = 0; k < 3; k++) { f.height_map_scale[k] = su->height_map_scale[k]; f.scene_scale[k] = su->scene_scale[k]; }
    f.culling_dist = cfg->culling_dist; f.lod_enable_mask = cfg->lod_enable_mask; f.t_eps = cfg->transmittance_eps;
    f.has_depth = a.img.d_bgd ? 1 : 0;
    f.width = width; f.height = height;
    // the shard's screen tiles: every column of the interleaved tile rows, or (column mode) a contiguous band of tile columns
    f.tiles_x = g.col1 - g.col0; f.tiles_y = (height + kTile - 1) / kTile;
    f.col0 = g.col0; f.col1 = g.col1; f.out_w = g.out_w; f.out_x0 = g.out_x0; f.band_cull = 0;
    f.shard_index = g.world > 1 && !g.cols ? cfg->shard_index : 0; f.shard_count = g.cols ? 1 : g.world;
    if (g.cols) {
        // band culling bounds where a cell's splats can land: the plain surface (positions are the list positions) and the
        // HeightMap surface (the reference's default, structure.rs:75: the mapped centre is (x, y, h(x, y) hz) + n z with |n| = 1 and h
        // between the map's extremes; the covariance becomes F Vrk F^T with |F|_F^2 <= 3 + slope_x^2 + slope_y^2) and the
        // Sphere surface (cells whose footprint stays inside one block of the strip parametrisation: sphere_cell_box in gswt_kernels.hip;
        // the columns of F are finite differences of lz R, |.| <= 2.5 R / block_w, and lz itself).  Not the point-cloud covariance.
        f.band_cull = (su->surface_type <= 2u && !(su->point_cloud_radius > 0.0f)) ? 1 : 0;
    }
    for (int k = 0; k < 3; k++) { f.loc_lo[k] = c.loc_lo[k]; f.loc_hi[k] = c.loc_hi[k]; }
    f.loc_max_trace = c.loc_max_trace;
    f.surf_zlo = f.surf_zhi = 0.0f; f.surf_f2 = 1.0f;
    if (su->surface_type == 1u) {
        const float hz = su->height_map_scale[2];
        f.surf_zlo = std::min(c.hm_min * hz, c.hm_max * hz); f.surf_zhi = std::max(c.hm_min * hz, c.hm_max * hz);
        // slopes of the mapped surface per world unit: |dh/du| hz / x_range, |dh/dv| hz / y_range (gswt.wgsl:565-599)
        const float xr = gswt_host::hm_axis_range(su->map_half_wh[0], su->tile_width, su->height_map_scale[0]);
        const float yr = gswt_host::hm_axis_range(su->map_half_wh[1], su->tile_width, su->height_map_scale[1]);
        const float sx = c.hm_du * std::fabs(hz) / std::fabs(xr), sy = c.hm_dv * std::fabs(hz) / std::fabs(yr);
        f.surf_f2 = (3.0f + sx * sx + sy * sy) * 1.01f;
        // a non-finite height map (gswt_configure leaves +-3e38 bounds), an infinite or NaN range or slope bound: no band culling at all
        // (fminf / fmaxf drop NaN operands, so a box with NaN corners used to read as "misses the band")
        const float fmax_ = 3.0e38f;
        if (!(f.surf_f2 == f.surf_f2) || !(f.surf_zlo == f.surf_zlo) || !(f.surf_zhi == f.surf_zhi) || !(std::fabs(f.surf_f2) < fmax_) ||
            !(std::fabs(f.surf_zlo) < fmax_) || !(std::fabs(f.surf_zhi) < fmax_) || !(c.hm_du < fmax_) || !(c.hm_dv < fmax_)) f.band_cull = 0;
    }
    if (su->surface_type == 2u) {
        const float block_w = ((float)su->map_half_wh[0] * 2.0f) * su->tile_width / 5.0f;
        const float g = 2.5f * std::fabs(su->sphere_radius) / block_w;
        f.surf_f2 = (2.0f * g * g + 1.0f) * 1.01f;
        if (!(block_w > 0.0f) || !(f.surf_f2 == f.surf_f2) || su->map_half_wh[0] == 0u || su->map_half_wh[1] == 0u) f.band_cull = 0;
    }
    f.hm_w = c.hm_w; f.hm_h = c.hm_h;
    f.map_wh_y = 2u * su->map_half_wh[1] + (su->surface_type != 2u ? 1u : 0u);
    // (0 = "divide": a one-row map, map_wh_y == 1, would wrap the magic to 0 and the multiply-high quotient to 0 -- ADVICE r3)
    f.map_wh_y_magic = f.map_wh_y >= 2u && f.map_wh_y < 65536u ? 0xFFFFFFFFu / f.map_wh_y + 1u : 0u;
    f.tiles_x_magic = f.tiles_x > 0 && f.tiles_x < 65536 ? 0xFFFFFFFFu / (uint32_t)f.tiles_x + 1u : 0u;
    f.aa_s = a.modes.aa_s;
    f.atm = a.modes.atm;
    return f;
}

// Every buffer of the slot's frame: sized for n_tiles screen tiles, `cap` pairs and the two sorts' key widths (depth_bits 0: no global
// depth passes), carved and pointed to in `b` with the lengths k_cull clears.
static int plan_frame_buffers(gswt_ctx* c, FrameSlot& sl, const DrawSet& D, const Frame& f, int n_tiles, uint32_t cap, int key_bits, int depth_bits,
                              FrameBufs& b)
{
    const FrameArgs& a = sl.args;
    const FrameImages& im = a.img;
    const size_t nt = (size_t)n_tiles, n_slots_all = (size_t)D.n_chunks * kChunk;
    const bool depth_order = a.cfg.order_mode == GSWT_ORDER_DEPTH, need_depths = im.d_bgd != nullptr || depth_order || im.d_out_depth != nullptr || im.d_out_pick != nullptr;
    const uint32_t seg = (uint32_t)c->opt.segment;      // (opt_segment: the measured segment sizes are at Options::segment, gswt_ctx.h)
    b.n_cells = f.band_cull ? (2u * f.map_half_wh[0] + 1u) * (2u * f.map_half_wh[1] + 1u) : 0u;
    HIP_TRY(c, sl.rects.ensure(n_slots_all + 1));
    HIP_TRY(c, sl.recs.ensure(n_slots_all + 1));
    HIP_TRY(c, sl.block_sums.ensure_roomy((size_t)D.n_chunks + 1));
    HIP_TRY(c, sl.live_tab.ensure_roomy((size_t)D.n_launch + 8));
    HIP_TRY(c, sl.live_cid.ensure_roomy((size_t)D.n_launch + 8));
    // (cleared ON THE SLOT'S STREAM: the slot streams are non-blocking, so a null-stream hipMemset -- asynchronous to the host for
    // device memory -- could land after this frame's k_cull had filled the counts: the slot's FIRST frame then projected nothing
    // and came back as background.  Seen once five slots made test_async_all_slots_in_flight_and_slot_reuse the first user of slot 4.)
    if (!sl.live_cnt.p) { HIP_TRY(c, sl.live_cnt.ensure(kLiveTableWords)); HIP_TRY(c, hipMemsetAsync(sl.live_cnt.p, 0, sl.live_cnt.cap * 4, sl.stream)); }
    HIP_TRY(c, sl.draw_culled.ensure_roomy((size_t)D.n_draws + 1));
    HIP_TRY(c, sl.cell_culled.ensure((size_t)b.n_cells + 1));
    if (a.su.draw_mode != 0u) HIP_TRY(c, sl.col_f.ensure(n_slots_all + 1));
    if (need_depths) HIP_TRY(c, sl.depths.ensure(n_slots_all + 1));
    if (c->opt.debug_varyings) HIP_TRY(c, c->dbg.ensure((size_t)D.n_entries + 1));
    // the `ranges` region (uint2 units): every tile's range words (encode_tile_range) and one more, then the tile-local depth sort's two lists of long tiles;
    // the list parts are padded to whole uint2s plus one.  k_cull clears the ranges, the first list and the second list's count.
    const size_t range_words = 2 * (nt + 1), list_words = tile_depth_list_words(nt);
    auto uint2s = [](size_t words) { return (words + 1) / 2 + 1; };
    HIP_TRY(c, sl.ranges.ensure(range_words / 2 + 2 * uint2s(list_words)));
    b.n_zero_ranges = (uint32_t)(range_words + list_words + 1);
    // the `ghist` region (u32): [FrameCounters][SuperSums][pair sort's RadixWs][depth sort's RadixWs] (gswt_frame_layout.h); a workspace has
    // its zeroed part in front.  k_cull clears the head up to the end of the pair sort's zeroed part, and the depth sort's zeroed part.
    const size_t counter_words = kFrameCounterWords, super_words = super_sums_of(D.n_chunks).words();
    const RadixWs ws_pair = radix_ws_of(cap, key_bits), ws_depth = radix_ws_of(cap, depth_bits);       // (depth_bits 0: no passes, no words)
    HIP_TRY(c, sl.ghist.ensure_roomy(counter_words + super_words + ws_pair.words() + ws_depth.words() + 16));
    b.n_zero_head = (uint32_t)(counter_words + super_words + ws_pair.zero_words());
    b.n_zero_depth = (uint32_t)ws_depth.zero_words();
    HIP_TRY(c, sl.keys_a.ensure_roomy((size_t)cap + 1)); HIP_TRY(c, sl.keys_b.ensure_roomy((size_t)cap + 1));
    HIP_TRY(c, sl.vals_a.ensure_roomy((size_t)cap + 1)); HIP_TRY(c, sl.vals_b.ensure_roomy((size_t)cap + 1));
    if (depth_order) { HIP_TRY(c, sl.aux_a.ensure_roomy((size_t)cap + 1)); HIP_TRY(c, sl.aux_b.ensure_roomy((size_t)cap + 1)); }
    HIP_TRY(c, sl.item_base.ensure_roomy(nt + 2));
    HIP_TRY(c, sl.partials.ensure_roomy((nt + cap / seg + 1) * 256));
    if (im.d_out_depth) HIP_TRY(c, sl.partials_z.ensure_roomy((nt + cap / seg + 1) * 256));
    if (im.d_out_pick) HIP_TRY(c, sl.partials_pick.ensure_roomy((nt + cap / seg + 1) * 256));
    HIP_TRY(c, sl.item_tab.ensure_roomy(nt + cap / seg + 2));

    b.draws = D.draws; b.n_chunks = D.n_chunks; b.chunk_tab = D.chunk_tab.p; b.chunk_tab_xcd = D.chunk_tab_xcd.p;
    b.static_list = c->static_list.p; b.merged_list = D.merged_list.p; b.merged_map = D.merged_map.p;
    b.tex = c->tex.p; b.hmap = c->hmap.p; b.boxes = c->static_boxes.p;
    // (the versions the frame was submitted with: no setter refills them while this slot names them)
    const StyleVersion* const sty = c->styles.get(a.modes.sty_ver);
    b.styles = sty ? sty->d.p : nullptr; b.n_styles = sty ? sty->n : 0u;
    b.shadow = shadow_version(c, a.modes.shd_ver);
    b.clip = a.modes.clip;
    b.bg_rgba = im.d_bg; b.bg_depth = im.d_bgd; b.out = im.d_out; b.out_depth = im.d_out_depth; b.host_counters = sl.hc_dev;
    b.out_pick = reinterpret_cast<uint4*>(im.d_out_pick);
    b.n_tiles = (uint32_t)n_tiles; b.pair_cap = cap; b.seg = seg;
    b.rects = sl.rects.p; b.recs = sl.recs.p; b.depths = need_depths ? sl.depths.p : nullptr; b.col_f = sl.col_f.p; b.dbg = c->dbg.p;
    b.draw_culled = sl.draw_culled.p; b.cell_culled = sl.cell_culled.p;
    b.live_cnt = sl.live_cnt.p; b.live_cid = sl.live_cid.p; b.live_tab = sl.live_tab.p; b.block_sums = sl.block_sums.p;
    b.ghist = sl.ghist.p;
    b.counters = reinterpret_cast<FrameCounters*>(b.ghist);
    b.super_sums = b.ghist + counter_words;
    b.radix_pair = b.super_sums + super_words;
    b.radix_depth = b.radix_pair + ws_pair.words();
    b.keys_a = sl.keys_a.p; b.keys_b = sl.keys_b.p; b.vals_a = sl.vals_a.p; b.vals_b = sl.vals_b.p; b.aux_a = sl.aux_a.p; b.aux_b = sl.aux_b.p;
    b.ranges = sl.ranges.p;
    b.long_tiles = reinterpret_cast<uint32_t*>(sl.ranges.p) + range_words;
    b.item_base = sl.item_base.p; b.item_tab = sl.item_tab.p; b.partials = sl.partials.p; b.partials_z = im.d_out_depth ? sl.partials_z.p : nullptr;
    b.partials_pick = im.d_out_pick ? sl.partials_pick.p : nullptr;
    const bool time_pick = im.d_out_pick != nullptr && c->opt.timing >= 1;
    b.ev_pick_begin = time_pick ? sl.ev[kEvPickBegin] : nullptr; b.ev_pick_end = time_pick ? sl.ev[kEvPickEnd] : nullptr;
    sl.pick_timed = time_pick && n_tiles > 0;
    return GSWT_OK;
}

// Emits the frame's (tile, slot) pairs and sorts them; *sorted = the slots in composite order.
// Reference order: the pairs in slot order, stably sorted on the tile bits.  Depth order: inside a tile true depth order, equal depths in
// slot order, by one of two paths.  Tile-local: the tile passes carry the depth bits as payload, then k_tile_depth_sort orders every tile's
// slice (lists of any length).  Global (GSWT_OPT_DEPTH_SORT = 1): the depth passes in use first (payload: the tile ids), then the tile
// passes.  The last tile pass also leaves every screen tile's [start, end) of the sorted list in b.ranges (zeroed by k_cull).
static int emit_and_sort(gswt_ctx* c, const FrameSlot& sl, const Frame& f, const FrameBufs& b, int key_bits, const uint32_t** sorted)
{
    hipStream_t s = sl.stream;
    const uint32_t n_launch = c->opt.debug_varyings ? 0u : sl.n_launch_eff;       // (the debug-varyings frame emits from every chunk)
    const SortCount* const n_pairs = sort_count_of(b.counters);      // the pair count, refused while the frame is flagged for a re-run
    const uint32_t cap = b.pair_cap;
    if (sl.args.cfg.order_mode != GSWT_ORDER_DEPTH) {
        launch_emit(s, f, b, b.keys_a, nullptr, nullptr, n_launch);
        if (c->opt.timing >= 2) HIP_TRY(c, hipEventRecord(sl.ev[kEvEmitted], s));
        const int where = launch_sort(s, b.keys_a, b.vals_a, b.keys_b, b.vals_b, cap, n_pairs, key_bits, b.radix_pair, b.ranges);
        *sorted = where ? b.vals_b : b.vals_a;
    } else if (sl.depth_local) {
        launch_emit(s, f, b, b.keys_a, b.aux_a, nullptr, n_launch);
        if (c->opt.timing >= 2) HIP_TRY(c, hipEventRecord(sl.ev[kEvEmitted], s));
        const int where = launch_sort(s, b.keys_a, b.vals_a, b.keys_b, b.vals_b, cap, n_pairs, key_bits, b.radix_pair, b.ranges, nullptr, b.aux_a, b.aux_b);
        uint32_t* const vals = where ? b.vals_b : b.vals_a;
        launch_tile_depth_sort(s, b.ranges, vals, where ? b.aux_b : b.aux_a, where ? b.vals_a : b.vals_b, where ? b.aux_a : b.aux_b, (int)b.n_tiles,
                               b.long_tiles, b.counters);
        *sorted = vals;
    } else {
        launch_emit(s, f, b, b.aux_a, b.keys_a, b.krange(), n_launch);
        if (c->opt.timing >= 2) HIP_TRY(c, hipEventRecord(sl.ev[kEvEmitted], s));
        const int wd = launch_sort(s, b.keys_a, b.vals_a, b.keys_b, b.vals_b, cap, n_pairs, 8 * (int)sl.depth_passes, b.radix_depth, nullptr, b.krange(),
                                   b.aux_a, b.aux_b);
        // (the depth keys are dead now: keys_a serves as the other half of the tile-key ping-pong)
        uint32_t* const tiles_in = wd ? b.aux_b : b.aux_a;
        uint32_t* const vals_in = wd ? b.vals_b : b.vals_a;
        uint32_t* const vals_other = wd ? b.vals_a : b.vals_b;
        const int where = launch_sort(s, tiles_in, vals_in, b.keys_a, vals_other, cap, n_pairs, key_bits, b.radix_pair, b.ranges);
        *sorted = where ? vals_other : vals_in;
    }
    return GSWT_OK;
}

// Enqueues every kernel of one frame on the slot's stream.  All pointers in sl.args are device pointers.
static int enqueue_frame(gswt_ctx* c, FrameSlot& sl)
{
    const FrameArgs& a = sl.args;
    DrawSet& D = c->sets[sl.set];
    hipStream_t s = sl.stream;
    const ShardGeom g = shard_geom(a.cfg, a.width, a.height);
    const Frame f = make_frame(*c, a, g);
    const int rsc = f.shard_count;                                  // row-shard count (1 in column mode)
    const int tiles_y_local = rsc > 1 ? (f.tiles_y - f.shard_index + rsc - 1) / rsc : f.tiles_y;
    const int n_tiles = f.tiles_x * (tiles_y_local > 0 ? tiles_y_local : 0);
    const int out_rows = g.out_rows;
    const size_t out_px = g.px;
    sl.n_tiles = n_tiles;
    const bool dbg = c->opt.debug_varyings != 0;
    // The pair count P is only known on the device.  Everything downstream of k_project is launched
    // for a capacity `pair_cap` (blocks past the real P do nothing), so a frame needs no host round
    // trip; the count and an overflow flag travel back with the frame.  If P exceeded the capacity
    // the buffers grow and the frame is re-run by finish_frame (first frame / sudden scene change only).
    int key_bits = 1;
    while ((1 << key_bits) < n_tiles) key_bits++;
    if (c->pair_cap == 0) c->pair_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(D.n_entries / 4, 1u << 20), 0xFFFFFF00ull);
    sl.cap = c->pair_cap;
    // GSWT_ORDER_DEPTH: the global depth passes take as many 8-bit passes as the key ranges of the recent frames needed (k_items flags a
    // frame that needs more: finish_frame re-runs it).  GSWT_OPT_DEPTH_SORT: 0 / 2 = the tile-local sort, 1 = the global passes.
    const bool depth_order = a.cfg.order_mode == GSWT_ORDER_DEPTH;
    sl.depth_passes = depth_order ? std::min<uint32_t>(std::max<uint32_t>(c->depth_passes, 1u), 4u) : 0u;
    sl.depth_local = depth_order && c->opt.depth_sort != 1;
    if (depth_order) (sl.depth_local ? c->stat_depth_local : c->stat_depth_global)++;
    FrameBufs b;
    int rc = plan_frame_buffers(c, sl, D, f, n_tiles, sl.cap, key_bits, sl.depth_local ? 0 : 8 * (int)sl.depth_passes, b);
    if (rc != GSWT_OK) return rc;
    // the frame starts after everything submitted to the ctx stream so far (inputs produced there, earlier readers of
    // the output buffer, the device-side merged-list build and the draw bounds of its draw set), on the slot's own stream
    // (an idle ctx stream has nothing to wait for; a cross-stream event wait per frame is not free: c3 static camera 4 700 -> 4 900 frames/s)
    if (hipStreamQuery(c->stream) != hipSuccess) {
        HIP_TRY(c, hipEventRecord(sl.ev_in, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(s, sl.ev_in, 0));
    }
    // ... and behind its draw set's upload / merged-list build on set_stream, unless that has long finished (the usual case: a
    // wait on another stream's event costs a barrier packet per frame)
    if (D.ev_up && D.ev_up_pending && !D.built) {
        if (hipEventQuery(D.ev_up) == hipSuccess) D.built = true;
        else HIP_TRY(c, hipStreamWaitEvent(s, D.ev_up, 0));
    }
    if (g.world > 1 && out_px > 0) HIP_TRY(c, hipMemsetAsync(a.img.d_out, 0, g.bytes, s));
    if (g.world > 1 && out_px > 0 && a.img.d_out_depth) HIP_TRY(c, hipMemsetAsync(a.img.d_out_depth, 0, out_px * sizeof(float), s));
    if (g.world > 1 && out_px > 0 && a.img.d_out_pick) HIP_TRY(c, hipMemsetAsync(a.img.d_out_pick, 0, out_px * sizeof(gswt_pick), s));
    // GSWT_OPT_GRAPH: from here to the end of the frame the launch sites record instead of launching (frames that carry timing
    // events, debug varyings and shards without tiles launch as before)
    const bool use_graph = c->opt.graph != 0 && c->opt.timing == 0 && !dbg && n_tiles > 0 && sl.hc_dev != nullptr;
    struct RecorderScope {
        explicit RecorderScope(GraphRec* r) { if (r) { r->n = 0; r->overflow = false; } graph_recorder() = r; }
        ~RecorderScope() { graph_recorder() = nullptr; }
    } recorder_scope(use_graph ? &sl.grec : nullptr);
    hipEvent_t* ev = sl.ev;
    if (c->opt.timing >= 1) HIP_TRY(c, hipEventRecord(ev[kEvStart], s));
    // ---- cull (+ clears the frame's accumulators) + project
    launch_cull(s, f, b, c->opt.no_chunk_cull == 0 && !dbg);
    {
        uint64_t eff = D.n_launch;
        if (!dbg && !sl.full_grid && c->live_hint) {
            const uint64_t cut = 8ull * ((uint64_t)c->live_hint + c->live_hint / 2 + 256);
            if (cut * 2 <= eff) eff = cut;                     // (only where it removes most of the grid: a re-run costs a frame)
        }
        sl.n_launch_eff = (uint32_t)eff;
    }
    launch_project(s, f, b, sl.n_launch_eff, dbg, project_modes(a.modes));
    if (c->opt.timing >= 2) HIP_TRY(c, hipEventRecord(ev[kEvProjected], s));
    // ---- emit + sort, ranges, composite
    const uint32_t* vals = nullptr;
    rc = emit_and_sort(c, sl, f, b, key_bits, &vals);
    if (rc != GSWT_OK) return rc;
    sl.sorted_vals = vals; sl.sorted_final = false;
    if (c->opt.timing >= 2) HIP_TRY(c, hipEventRecord(ev[kEvSorted], s));
    if (c->opt.timing >= 2) HIP_TRY(c, hipEventRecord(ev[kEvRanges], s));
    launch_composite(s, f, b, vals, out_rows, depth_order && !sl.depth_local ? b.krange() : nullptr, sl.depth_passes, depth_order,
                     c->opt.timing >= 1 ? ev[kEvCompositeBegin] : nullptr, c->opt.timing >= 1 ? ev[kEvCompositeEnd] : nullptr,
                     (int)a.cfg.out_format);
    c->last_n_tiles = (uint32_t)n_tiles;
    c->last_slot = (int)(&sl - c->slots);
    if (c->opt.timing >= 1) HIP_TRY(c, hipEventRecord(ev[kEvEnd], s));
    if (use_graph) {
        graph_recorder() = nullptr;
        const int grc = replay_graph(c, sl);
        if (grc != GSWT_OK) return grc;
    }
    HIP_TRY(c, hipGetLastError());
    // k_combine (the last kernel of the frame, or the last but k_pick_resolve) stores the result counters into the pinned host words itself; only a frame
    // without screen tiles has no such launch
    if (n_tiles == 0 || !sl.hc_dev) HIP_TRY(c, hipMemcpyAsync(sl.hc, &b.counters->res, kFrameResultWords64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipEventRecord(ev[kEvDone], s));
    sl.timing_level = c->opt.timing;
    return GSWT_OK;
}

// Waits for the slot's frame; re-runs it with larger pair buffers if it overflowed; fills c->timings.
static int finish_frame(gswt_ctx* c, FrameSlot& sl)
{
    for (int attempt = 0;; attempt++) {
        HIP_TRY(c, hipEventSynchronize(sl.ev[kEvDone]));
        const unsigned long long P64 = sl.hc->n_pairs;
        if (P64 >= 0xFFFFFF00ull) return fail(c, GSWT_ERR_CAPACITY, "gswt_render: %llu pairs exceed 2^32", P64);
        if (sl.hc->rerun == 0 && P64 <= sl.cap) break;
        if (attempt >= 3) return fail(c, GSWT_ERR_CAPACITY, "gswt_render: pair capacity did not converge");      // (a short launch grid, a pair overflow and a depth-pass shortfall can each cost one re-run)
        if (P64 > sl.cap || sl.args.cfg.order_mode != GSWT_ORDER_DEPTH)
            c->pair_cap = std::max<uint32_t>(c->pair_cap, (uint32_t)std::min<uint64_t>(P64 + P64 / 2 + 4096, 0xFFFFFF00ull));
        if (sl.args.cfg.order_mode == GSWT_ORDER_DEPTH) {
            const uint32_t need = sl.hc->depth_passes_needed, max_len = sl.hc->max_tile_len;
            if (!sl.depth_local && need > sl.depth_passes) { c->depth_passes = std::min<uint32_t>(need, 4u); c->depth_passes_low_run = 0; }
            // a re-run tile-local frame (pair overflow, short launch grid: lists of any length fit k_tile_depth_sort) keeps the same path;
            // gswt_debug_depth_stats reports at least one list past the LDS buffer (k_items may not have seen the whole frame's lengths yet
            // when the flag was raised)
            if (sl.depth_local) c->depth_max_tile_len = std::max<uint32_t>(std::max<uint32_t>(max_len, c->depth_max_tile_len), tile_depth_sort_cap() + 1u);
        }
        sl.full_grid = true;                                   // (whatever flagged it: the re-run covers the whole launch table)
        c->live_hint = std::max<uint32_t>(c->live_hint, (uint32_t)std::min<unsigned long long>(sl.hc->live_longest, 0xFFFFFFFFull));
        int rc = enqueue_frame(c, sl);
        sl.full_grid = false;
        if (rc != GSWT_OK) return rc;
    }
    c->live_hint = (uint32_t)std::min<unsigned long long>(sl.hc->live_longest, 0xFFFFFFFFull);
    const uint32_t P = (uint32_t)sl.hc->n_pairs;
    sl.sorted_pairs = P; sl.sorted_final = true;
    // keep 25-50 % headroom over the running pair count without shrinking on every small dip
    if (!c->opt.fixed_pair_cap && (uint64_t)P + P / 4 > c->pair_cap) c->pair_cap = (uint32_t)std::min<uint64_t>((uint64_t)P + P / 2 + 4096, 0xFFFFFF00ull);
    if (sl.args.cfg.order_mode == GSWT_ORDER_DEPTH) {
        const uint32_t need = std::min<uint32_t>(std::max<uint32_t>(sl.hc->depth_passes_needed, 1u), 4u);
        c->depth_max_tile_len = sl.hc->max_tile_len;       // (every depth-ordered frame reports it: gswt_debug_depth_stats)
        if (sl.depth_local) { /* the pass count is the kernel's own business there */ }
        else if (need < c->depth_passes && sl.depth_passes == c->depth_passes) {
            c->depth_passes_low_max = c->depth_passes_low_run ? std::max(c->depth_passes_low_max, need) : need;
            if (++c->depth_passes_low_run >= 32u) { c->depth_passes = c->depth_passes_low_max; c->depth_passes_low_run = 0; }
        } else if (need >= c->depth_passes) c->depth_passes_low_run = 0;
    }
    gswt_timings& t = c->timings;
    memset(&t, 0, sizeof(t));
    hipEvent_t* ev = sl.ev;
    if (sl.timing_level >= 2) {
        HIP_TRY(c, hipEventElapsedTime(&t.ms_project, ev[kEvStart], ev[kEvProjected]));
        HIP_TRY(c, hipEventElapsedTime(&t.ms_emit, ev[kEvProjected], ev[kEvEmitted]));
        HIP_TRY(c, hipEventElapsedTime(&t.ms_sort, ev[kEvEmitted], ev[kEvSorted]));
        HIP_TRY(c, hipEventElapsedTime(&t.ms_ranges, ev[kEvSorted], ev[kEvRanges]));
        HIP_TRY(c, hipEventElapsedTime(&t.ms_composite, ev[kEvRanges], ev[kEvEnd]));
    }
    if (sl.timing_level >= 1) {
        HIP_TRY(c, hipEventElapsedTime(&t.ms_total, ev[kEvStart], ev[kEvEnd]));
        HIP_TRY(c, hipEventElapsedTime(&t.ms_composite_kernel, ev[kEvCompositeBegin], ev[kEvCompositeEnd]));
        if (sl.pick_timed) HIP_TRY(c, hipEventElapsedTime(&t.ms_pick_resolve, ev[kEvPickBegin], ev[kEvPickEnd]));
    }
    t.n_draws = c->sets[sl.set].n_draws; t.n_instanced = c->sets[sl.set].n_entries; t.n_visible = sl.hc->n_visible; t.n_pairs = P; t.n_tiles = (uint32_t)sl.n_tiles;
    return GSWT_OK;
}

// Submits a frame in slot `sl` (gswt_render, gswt_render_async): the slot's stream on first use, the draw set current now, the arguments.
static int submit_frame(gswt_ctx* c, FrameSlot& sl, const gswt_camera_uniforms* cam, const gswt_scene_uniforms* su, const gswt_render_config* cfg,
                        int width, int height, const FrameImages& img)
{
    if (!sl.stream) HIP_TRY(c, hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));      // a slot past the fourth: first use
    activate_pending(c, false);
    sl.set = c->cur_set;
    sl.args = FrameArgs{*cam, *su, *cfg, width, height, img, frame_modes(*c, *su)};
    return enqueue_frame(c, sl);
}

// The output images of one frame must be distinct (validate_frame has refused a null out_rgba).  `fn` / `sfx` name the entry point and
// its arguments in the message: "gswt_render" / "" or "gswt_render_async" / "_dev".
static int check_frame_outputs(gswt_ctx* c, const char* fn, const char* sfx, const void* out_rgba, const void* out_depth, const void* out_pick)
{
    if (out_depth && out_depth == out_rgba) return fail(c, GSWT_ERR_BAD_ARG, "%s_depth: out_depth%s is out_rgba%s", fn, sfx, sfx);
    if (out_pick && (out_pick == out_rgba || out_pick == out_depth))
        return fail(c, GSWT_ERR_BAD_ARG, "%s_pick: out_pick%s is out_rgba%s or out_depth%s", fn, sfx, sfx, sfx);
    return GSWT_OK;
}

// The slot of the next frame: the lowest free one (a caller that keeps fewer frames in flight than there are slots then cycles over
// fewer buffer sets: the per-frame buffers of a c5-sized frame are ~5 GB per slot).  All in flight: the slot of the oldest frame
// (its caller collects that frame first), or -1 when the caller cannot take a ticket back.
static int select_slot(const gswt_ctx* c, bool reuse_oldest)
{
    for (int k = 0; k < kFrameSlots; k++) if (!c->slots[k].pending) return k;
    if (!reuse_oldest) return -1;
    int si = 0;
    for (int k = 1; k < kFrameSlots; k++) if (c->slots[k].seq < c->slots[si].seq) si = k;
    return si;
}

// gswt_render's images (null: none).  An input of n elements: read in place on the device, or copied from the host into the context's
// staging on the ctx stream.
template <typename T>
static int stage_input(gswt_ctx* c, DevBuf<T>& staging, const float* src, size_t n, bool on_device, const T** d)
{
    if (!src || on_device) { *d = reinterpret_cast<const T*>(src); return GSWT_OK; }
    HIP_TRY(c, staging.ensure(n));
    HIP_TRY(c, hipMemcpyAsync(staging.p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *d = staging.p;
    return GSWT_OK;
}
// An output of `bytes` bytes: written in place on the device, or into the context's staging and copied to the host behind the frame (`back`).
struct HostOutput { void* host = nullptr; const void* dev = nullptr; size_t bytes = 0; };
template <typename T, typename U, typename H>
static int stage_output(gswt_ctx* c, DevBuf<U>& staging, H* out, size_t bytes, bool on_device, T** d, HostOutput* back)
{
    if (!out || on_device) { *d = reinterpret_cast<T*>(out); return GSWT_OK; }
    HIP_TRY(c, staging.ensure((bytes + sizeof(U) - 1) / sizeof(U)));
    *d = reinterpret_cast<T*>(staging.p);
    *back = HostOutput{out, staging.p, bytes};
    return GSWT_OK;
}

extern "C" {

int gswt_render(gswt_ctx* c, const gswt_camera_uniforms* cam, const gswt_scene_uniforms* su, const gswt_render_config* cfg,
                int width, int height, const float* bg_rgba, const float* bg_depth, int bg_on_device, float* out_rgba,
                int out_on_device)
{
    return gswt_render_depth(c, cam, su, cfg, width, height, bg_rgba, bg_depth, bg_on_device, out_rgba, nullptr, out_on_device);
}

int gswt_render_depth(gswt_ctx* c, const gswt_camera_uniforms* cam, const gswt_scene_uniforms* su, const gswt_render_config* cfg,
                      int width, int height, const float* bg_rgba, const float* bg_depth, int bg_on_device, float* out_rgba,
                      float* out_depth, int out_on_device)
{
    return gswt_render_pick(c, cam, su, cfg, width, height, bg_rgba, bg_depth, bg_on_device, out_rgba, out_depth, nullptr, out_on_device);
}

int gswt_render_pick(gswt_ctx* c, const gswt_camera_uniforms* cam, const gswt_scene_uniforms* su, const gswt_render_config* cfg,
                     int width, int height, const float* bg_rgba, const float* bg_depth, int bg_on_device, float* out_rgba,
                     float* out_depth, gswt_pick* out_pick, int out_on_device)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    int rc = validate_frame(c, cam, su, cfg, width, height, out_rgba);
    if (rc != GSWT_OK) return rc;
    rc = check_frame_outputs(c, "gswt_render", "", out_rgba, out_depth, out_pick);
    if (rc != GSWT_OK) return rc;
    hipSetDevice(c->device);
    HIP_TRY(c, collect_pending(c));                // frames still in flight from the async API keep their tickets
    const ShardGeom g = shard_geom(*cfg, width, height);
    const size_t out_px = g.px, npx = (size_t)width * height;
    FrameImages img;
    HostOutput back[3];
    if ((rc = stage_input(c, c->bg_rgba, bg_rgba, npx, bg_on_device != 0, &img.d_bg)) != GSWT_OK) return rc;
    if ((rc = stage_input(c, c->bg_depth, bg_depth, npx, bg_on_device != 0, &img.d_bgd)) != GSWT_OK) return rc;
    if ((rc = stage_output(c, c->out_img, out_rgba, g.bytes, out_on_device != 0, &img.d_out, &back[0])) != GSWT_OK) return rc;
    if ((rc = stage_output(c, c->out_depth_img, out_depth, out_px * sizeof(float), out_on_device != 0, &img.d_out_depth, &back[1])) != GSWT_OK) return rc;
    if ((rc = stage_output(c, c->out_pick_img, out_pick, out_px * sizeof(gswt_pick), out_on_device != 0, &img.d_out_pick, &back[2])) != GSWT_OK) return rc;
    const int si = select_slot(c, false);
    if (si < 0) return fail(c, GSWT_ERR_STATE, "gswt_render: every frame slot holds an uncollected gswt_render_async ticket");
    FrameSlot& sl = c->slots[si];
    if ((rc = submit_frame(c, sl, cam, su, cfg, width, height, img)) != GSWT_OK) return rc;
    if ((rc = finish_frame(c, sl)) != GSWT_OK) return rc;
    for (const HostOutput& o : back)
        if (o.host) HIP_TRY(c, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, c->stream));
    if (!out_on_device) HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GSWT_OK;
} GSWT_CATCH

int gswt_render_async(gswt_ctx* c, const gswt_camera_uniforms* cam, const gswt_scene_uniforms* su, const gswt_render_config* cfg,
                      int width, int height, const float* bg_rgba_dev, const float* bg_depth_dev, float* out_rgba_dev, int* ticket)
{
    return gswt_render_async_depth(c, cam, su, cfg, width, height, bg_rgba_dev, bg_depth_dev, out_rgba_dev, nullptr, ticket);
}

int gswt_render_async_depth(gswt_ctx* c, const gswt_camera_uniforms* cam, const gswt_scene_uniforms* su, const gswt_render_config* cfg,
                            int width, int height, const float* bg_rgba_dev, const float* bg_depth_dev, float* out_rgba_dev,
                            float* out_depth_dev, int* ticket)
{
    return gswt_render_async_pick(c, cam, su, cfg, width, height, bg_rgba_dev, bg_depth_dev, out_rgba_dev, out_depth_dev, nullptr, ticket);
}

int gswt_render_async_pick(gswt_ctx* c, const gswt_camera_uniforms* cam, const gswt_scene_uniforms* su, const gswt_render_config* cfg,
                           int width, int height, const float* bg_rgba_dev, const float* bg_depth_dev, float* out_rgba_dev,
                           float* out_depth_dev, gswt_pick* out_pick_dev, int* ticket)
try {
    if (!c || !ticket) return GSWT_ERR_BAD_ARG;
    int rc = validate_frame(c, cam, su, cfg, width, height, out_rgba_dev);
    if (rc != GSWT_OK) return rc;
    rc = check_frame_outputs(c, "gswt_render_async", "_dev", out_rgba_dev, out_depth_dev, out_pick_dev);
    if (rc != GSWT_OK) return rc;
    hipSetDevice(c->device);
    const int si = select_slot(c, true);
    FrameSlot& sl = c->slots[si];
    if (sl.pending) {                   // every slot in flight: the oldest frame is collected here and its slot reused
        rc = take_slot(c, sl);
        if (rc != GSWT_OK) return rc;
    }
    sl.seq = ++c->frame_seq;
    sl.gather_recorded = false;
    rc = submit_frame(c, sl, cam, su, cfg, width, height, FrameImages{reinterpret_cast<const float4*>(bg_rgba_dev), bg_depth_dev,
                                                                      reinterpret_cast<float4*>(out_rgba_dev), out_depth_dev, out_pick_dev});
    if (rc != GSWT_OK) return rc;
    sl.pending = true; sl.collected = false;
    *ticket = si;
    return GSWT_OK;
} GSWT_CATCH

int gswt_frame_slots(void) { return kFrameSlots; }

int gswt_render_wait(gswt_ctx* c, int ticket)
try {
    if (!c || ticket < 0 || ticket >= kFrameSlots) return GSWT_ERR_BAD_ARG;
    FrameSlot& sl = c->slots[ticket];
    if (!sl.pending) return fail(c, GSWT_ERR_STATE, "gswt_render_wait: ticket %d is not in flight", ticket);
    hipSetDevice(c->device);
    return take_slot(c, sl);
} GSWT_CATCH

// All-or-nothing, like GSWTRenderer::render (renderer.rs:407-414): work ordered behind the fence never reads a frame whose pair
// buffers overflowed.  Overflow is only known once the frame's counters are back on the host, so the fence first waits
// (host side) for THIS frame -- the younger frames in flight keep the GPU busy meanwhile --, lets finish_frame re-run it
// with grown buffers if it has to, and only then orders the ctx stream behind the frame's final completion event.
int gswt_render_fence(gswt_ctx* c, int ticket)
try {
    if (!c || ticket < 0 || ticket >= kFrameSlots) return GSWT_ERR_BAD_ARG;
    FrameSlot& sl = c->slots[ticket];
    if (!sl.pending) return fail(c, GSWT_ERR_STATE, "gswt_render_fence: ticket %d is not in flight", ticket);
    hipSetDevice(c->device);
    collect_slot(c, sl);
    if (sl.collected_rc != GSWT_OK) return sl.collected_rc;
    HIP_TRY(c, hipStreamWaitEvent(c->stream, sl.ev[kEvDone], 0));
    return GSWT_OK;
} GSWT_CATCH

int gswt_synchronize(gswt_ctx* c)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    hipSetDevice(c->device);
    HIP_TRY(c, sync_all(c));
    return GSWT_OK;
} GSWT_CATCH

int gswt_last_timings(const gswt_ctx* c, gswt_timings* out)
try {
    if (!c || !out) return GSWT_ERR_BAD_ARG;
    *out = c->timings;
    return GSWT_OK;
} GSWT_CATCH

int gswt_debug_totals(gswt_ctx* c, const uint32_t* pair_sums, const uint32_t* visible_sums, uint32_t n_super, uint32_t pair_cap,
                      unsigned long long counters_out[4], uint32_t* super_excl_out)
try {
    if (!c || !pair_sums || !visible_sums || n_super == 0 || !counters_out) return GSWT_ERR_BAD_ARG;
    hipSetDevice(c->device);
    DevBuf<uint32_t> buf;
    DevBuf<FrameCounters> d_cnt;
    const SuperSums ss{n_super};
    HIP_TRY(c, buf.ensure(ss.words())); HIP_TRY(c, d_cnt.ensure(1));
    HIP_TRY(c, hipMemset(buf.p, 0, ss.words() * 4));
    HIP_TRY(c, hipMemset(d_cnt.p, 0, sizeof(FrameCounters)));
    // one word per super-group, each at its place in the region (a cache line apart)
    const size_t pitch = (size_t)(ss.pair_word(1) - ss.pair_word(0)) * 4;
    HIP_TRY(c, hipMemcpy2D(buf.p + ss.pair_word(0), pitch, pair_sums, 4, 4, n_super, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy2D(buf.p + ss.visible_word(0), pitch, visible_sums, 4, 4, n_super, hipMemcpyHostToDevice));
    launch_totals(c->stream, buf.p, ss, d_cnt.p, pair_cap);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // (the hook's four words: the block's first four 64-bit words, up to the re-run flag)
    static_assert(offsetof(FrameResult, rerun) + sizeof(unsigned long long) == 4 * sizeof(unsigned long long), "gswt_debug_totals' counters_out");
    HIP_TRY(c, hipMemcpy(counters_out, &d_cnt.p->res, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (super_excl_out) HIP_TRY(c, hipMemcpy(super_excl_out, buf.p + ss.prefix_word(0), (size_t)n_super * 4, hipMemcpyDeviceToHost));
    return GSWT_OK;
} GSWT_CATCH

// launch_sort alone (gswt_debug_sort, gswt_debug_sort_ex; arguments as the latter's, checked there): the sort reads its count through the
// SortCount view of a counter block staged as a frame's would be -- n pairs, flagged for a re-run when `refused` -- and, with krange
// ({smallest, largest} key; null: none), the key range from the same block.
static int debug_sort(gswt_ctx* c, uint32_t* keys, uint32_t* vals, uint32_t* aux, size_t n_cap, unsigned long long n, bool refused, int key_bits,
                      const uint32_t* krange, uint32_t* ranges_out, size_t n_range_keys, int threads, int aux_form)
{
    hipSetDevice(c->device);
    const uint32_t cap = (uint32_t)n_cap;
    DevBuf<uint32_t> ka, kb, va, vb, xa, xb, ws;
    DevBuf<uint2> rg;
    DevBuf<FrameCounters> blk;
    HIP_TRY(c, ka.ensure(n_cap + 4)); HIP_TRY(c, kb.ensure(n_cap + 4)); HIP_TRY(c, va.ensure(n_cap + 1)); HIP_TRY(c, vb.ensure(n_cap + 1));
    if (aux) { HIP_TRY(c, xa.ensure(n_cap + 1)); HIP_TRY(c, xb.ensure(n_cap + 1)); }
    if (ranges_out) { HIP_TRY(c, rg.ensure(n_range_keys + 1)); HIP_TRY(c, hipMemset(rg.p, 0, (n_range_keys + 1) * 8)); }
    const size_t words = radix_ws_words(cap, key_bits);
    HIP_TRY(c, ws.ensure(words)); HIP_TRY(c, blk.ensure(1));
    HIP_TRY(c, hipMemset(ws.p, 0, words * 4));
    FrameCounters h{};
    h.res.n_pairs = n; h.res.rerun = refused ? 1ull : 0ull;
    if (krange) { h.krange[0] = krange_min_word(krange[0]); h.krange[1] = krange[1]; }       // as k_emit<DEPTH>'s atomicMax pair leaves it
    HIP_TRY(c, hipMemcpy(blk.p, &h, sizeof(h), hipMemcpyHostToDevice));
    for (uint32_t* p : {ka.p, kb.p}) HIP_TRY(c, hipMemcpy(p, keys, n_cap * 4, hipMemcpyHostToDevice));
    for (uint32_t* p : {va.p, vb.p}) HIP_TRY(c, hipMemcpy(p, vals, n_cap * 4, hipMemcpyHostToDevice));
    if (aux) for (uint32_t* p : {xa.p, xb.p}) HIP_TRY(c, hipMemcpy(p, aux, n_cap * 4, hipMemcpyHostToDevice));
    const int where = launch_sort(c->stream, ka.p, va.p, kb.p, vb.p, cap, sort_count_of(blk.p), key_bits, ws.p, ranges_out ? rg.p : nullptr,
                                  krange ? blk.p->krange : nullptr, aux ? xa.p : nullptr, aux ? xb.p : nullptr, threads, aux_form);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!ranges_out) HIP_TRY(c, hipMemcpy(keys, where ? kb.p : ka.p, n_cap * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(vals, where ? vb.p : va.p, n_cap * 4, hipMemcpyDeviceToHost));
    if (aux) HIP_TRY(c, hipMemcpy(aux, where ? xb.p : xa.p, n_cap * 4, hipMemcpyDeviceToHost));
    if (ranges_out) {
        HIP_TRY(c, hipMemcpy(ranges_out, rg.p, n_range_keys * 8, hipMemcpyDeviceToHost));
        for (size_t t = 0; t < n_range_keys; t++) decode_tile_range(ranges_out[2 * t], ranges_out[2 * t + 1], ranges_out[2 * t], ranges_out[2 * t + 1]);
    }
    return GSWT_OK;
}

int gswt_debug_sort(gswt_ctx* c, uint32_t* keys, uint32_t* vals, size_t n, int key_bits)
try {
    if (!c || !keys || !vals || n == 0 || n >= 0xFFFFFF00ull || key_bits < 1 || key_bits > 32) return GSWT_ERR_BAD_ARG;
    return debug_sort(c, keys, vals, nullptr, n, n, false, key_bits, nullptr, nullptr, 0, 0, 0);
} GSWT_CATCH

int gswt_debug_sort_ex(gswt_ctx* c, uint32_t* keys, uint32_t* vals, uint32_t* aux, size_t n_cap, unsigned long long n, int overflow, int key_bits,
                       int use_krange, uint32_t krange_min, uint32_t krange_max, uint32_t* ranges_out, size_t n_range_keys, int threads, int aux_form)
try {
    if (!c || !keys || !vals || n_cap == 0 || n_cap >= 0xFFFFFF00ull || key_bits < 1 || key_bits > 32) return GSWT_ERR_BAD_ARG;
    if ((threads != 0 && threads != 256 && threads != 512) || aux_form < 0 || aux_form > 2 || (aux_form != 0 && !aux)) return GSWT_ERR_BAD_ARG;
    if (ranges_out && (n_range_keys == 0 || n_range_keys > 0x7FFFFFFFull)) return GSWT_ERR_BAD_ARG;
    if (use_krange && (krange_max < krange_min || (key_bits < 32 && ((krange_max - krange_min) >> key_bits) != 0u)))
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_debug_sort_ex: the key range does not fit %d key bits", key_bits);
    // what the kernels will look at: the first n items, unless the count is refused (clamped_count)
    const size_t n_seen = (overflow || n > n_cap) ? 0 : (size_t)n;
    for (size_t i = 0; i < n_seen; i++) {
        if (ranges_out && keys[i] >= n_range_keys) return fail(c, GSWT_ERR_BAD_ARG, "gswt_debug_sort_ex: key %u at %zu is outside the range table", keys[i], i);
        if (use_krange && (keys[i] < krange_min || keys[i] > krange_max)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_debug_sort_ex: key %u at %zu is outside the key range", keys[i], i);
    }
    const uint32_t kr[2] = {krange_min, krange_max};
    return debug_sort(c, keys, vals, aux, n_cap, n, overflow != 0, key_bits, use_krange ? kr : nullptr, ranges_out, n_range_keys, threads, aux_form);
} GSWT_CATCH

// Test hook: k_tile_depth_sort alone.  lens[t] = length of screen tile t's slice of the (tile-sorted) pair list, the slices back to back;
// vals / dkeys: the list's values and depth keys (n = sum of lens).  Sorts every slice's vals by its dkeys, stably, in place.  flagged_out:
// 1 when a slice was longer than the LDS buffer holds (nothing is then guaranteed about that slice; a frame would be re-run).
int gswt_debug_tile_depth_sort(gswt_ctx* c, const uint32_t* lens, size_t n_tiles, uint32_t* vals, const uint32_t* dkeys, size_t n, int* flagged_out)
try {
    if (!c || !lens || !vals || !dkeys || n_tiles == 0 || n_tiles > 0x7FFFFFFFull || n == 0 || n >= 0xFFFFFF00ull) return GSWT_ERR_BAD_ARG;
    hipSetDevice(c->device);
    std::vector<uint2> rg(n_tiles);
    size_t at = 0;
    for (size_t t = 0; t < n_tiles; t++) {                 // the range words the last sort pass would leave
        encode_tile_range((uint32_t)at, (uint32_t)(at + lens[t]), rg[t].x, rg[t].y);
        at += lens[t];
    }
    if (at != n) return fail(c, GSWT_ERR_BAD_ARG, "gswt_debug_tile_depth_sort: the lengths sum to %zu, not %zu", at, n);
    DevBuf<uint2> d_rg; DevBuf<uint32_t> d_vals, d_keys, d_vals2, d_keys2, d_long; DevBuf<FrameCounters> d_cnt;
    HIP_TRY(c, d_rg.ensure(n_tiles)); HIP_TRY(c, d_vals.ensure(n + 1)); HIP_TRY(c, d_keys.ensure(n + 1)); HIP_TRY(c, d_vals2.ensure(n + 1)); HIP_TRY(c, d_keys2.ensure(n + 1));
    const size_t long_words = 2 * tile_depth_list_words(n_tiles);
    HIP_TRY(c, d_long.ensure(long_words)); HIP_TRY(c, d_cnt.ensure(1));
    HIP_TRY(c, hipMemcpy(d_rg.p, rg.data(), n_tiles * 8, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_vals.p, vals, n * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_keys.p, dkeys, n * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemset(d_long.p, 0, long_words * 4));
    HIP_TRY(c, hipMemset(d_cnt.p, 0, sizeof(FrameCounters)));
    launch_tile_depth_sort(c->stream, d_rg.p, d_vals.p, d_keys.p, d_vals2.p, d_keys2.p, (int)n_tiles, d_long.p, d_cnt.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    FrameResult res;
    HIP_TRY(c, hipMemcpy(&res, &d_cnt.p->res, sizeof(res), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(vals, d_vals.p, n * 4, hipMemcpyDeviceToHost));
    if (flagged_out) *flagged_out = res.rerun != 0ull;
    return GSWT_OK;
} GSWT_CATCH

int gswt_debug_graph_stats(const gswt_ctx* c, unsigned long long out[3])
{
    if (!c || !out) return GSWT_ERR_BAD_ARG;
    out[0] = c->stat_graph_launches; out[1] = c->stat_graph_rebuilds; out[2] = c->stat_graph_node_updates;
    return GSWT_OK;
}

int gswt_debug_depth_stats(const gswt_ctx* c, unsigned long long out[3])
try {
    if (!c || !out) return GSWT_ERR_BAD_ARG;
    out[0] = c->stat_depth_local; out[1] = c->stat_depth_global; out[2] = c->depth_max_tile_len;
    return GSWT_OK;
} GSWT_CATCH

// Device timeline of frame slots (tests of the overlap claims): out_ms[0] = start of slot `ticket`'s frame kernels, [1] = their end,
// [2] = end of its gather + re-assembly on the ctx stream (NaN when the frame was not gathered), all in milliseconds after the START of
// slot `ticket_ref`'s frame.  Both frames must have been submitted with GSWT_OPT_TIMING >= 1 and have completed.
int gswt_debug_frame_times(gswt_ctx* c, int ticket_ref, int ticket, float out_ms[3])
try {
    if (!c || !out_ms || ticket_ref < 0 || ticket_ref >= kFrameSlots || ticket < 0 || ticket >= kFrameSlots) return GSWT_ERR_BAD_ARG;
    hipSetDevice(c->device);
    HIP_TRY(c, sync_all(c));
    FrameSlot& a = c->slots[ticket_ref];
    FrameSlot& b = c->slots[ticket];
    if (a.timing_level < 1 || b.timing_level < 1) return fail(c, GSWT_ERR_STATE, "gswt_debug_frame_times: frames without timing events");
    HIP_TRY(c, hipEventElapsedTime(&out_ms[0], a.ev[kEvStart], b.ev[kEvStart]));
    HIP_TRY(c, hipEventElapsedTime(&out_ms[1], a.ev[kEvStart], b.ev[kEvEnd]));
    out_ms[2] = __builtin_nanf("");
    if (b.gather_recorded) HIP_TRY(c, hipEventElapsedTime(&out_ms[2], a.ev[kEvStart], b.ev_gather));
    return GSWT_OK;
} GSWT_CATCH

int gswt_debug_read_ranges(gswt_ctx* c, uint32_t* out, size_t capacity_tiles, size_t* n_tiles)
try {
    if (!c || !n_tiles) return GSWT_ERR_BAD_ARG;
    *n_tiles = c->last_n_tiles;
    if (!out) return GSWT_OK;
    if (capacity_tiles < c->last_n_tiles) return fail(c, GSWT_ERR_CAPACITY, "buffer holds %zu tiles, need %u", capacity_tiles, c->last_n_tiles);
    hipSetDevice(c->device);
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(out, c->slots[c->last_slot].ranges.p, (size_t)c->last_n_tiles * 8, hipMemcpyDeviceToHost));
    for (uint32_t t = 0; t < c->last_n_tiles; t++)         // the device keeps range words; (0, 0) for a tile without pairs
        decode_tile_range(out[2 * (size_t)t], out[2 * (size_t)t + 1], out[2 * (size_t)t], out[2 * (size_t)t + 1]);
    return GSWT_OK;
} GSWT_CATCH

int gswt_debug_read_pairs(gswt_ctx* c, uint32_t* out, size_t capacity_pairs, size_t* n_pairs)
try {
    if (!c || !n_pairs) return GSWT_ERR_BAD_ARG;
    const FrameSlot& sl = c->slots[c->last_slot];
    if (!sl.sorted_vals) return fail(c, GSWT_ERR_STATE, "gswt_debug_read_pairs: no frame yet");
    if (!sl.sorted_final) return fail(c, GSWT_ERR_STATE, "gswt_debug_read_pairs: the last frame has not been waited for");
    *n_pairs = sl.sorted_pairs;
    if (!out) return GSWT_OK;
    const size_t n = sl.sorted_pairs;
    if (capacity_pairs < n) return fail(c, GSWT_ERR_CAPACITY, "buffer holds %zu pairs, need %zu", capacity_pairs, n);
    hipSetDevice(c->device);
    HIP_TRY(c, sync_all(c));
    const DrawSet& D = c->sets[sl.set];
    std::vector<DrawDev> draws(D.n_draws);
    std::vector<uint2> tab(D.n_chunks);
    if (D.n_draws) HIP_TRY(c, hipMemcpy(draws.data(), D.draws, draws.size() * sizeof(DrawDev), hipMemcpyDeviceToHost));
    if (D.n_chunks) HIP_TRY(c, hipMemcpy(tab.data(), D.chunk_tab.p, tab.size() * sizeof(uint2), hipMemcpyDeviceToHost));
    if (n) HIP_TRY(c, hipMemcpy(out, sl.sorted_vals, n * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) {                       // slot -> draw -> list entry in draw order (k_pick_resolve's walk; k_project's dbg index)
        const uint32_t slot = out[i];
        uint32_t entry = 0xFFFFFFFFu;
        if ((slot >> 8) < D.n_chunks && tab[slot >> 8].x < D.n_draws) {
            const DrawDev& d = draws[tab[slot >> 8].x];
            const uint32_t r = slot - d.slot_base;
            if (r < d.count) entry = d.entry_base + (d.count - 1u - r);
        }
        out[i] = entry;
    }
    return GSWT_OK;
} GSWT_CATCH

int gswt_debug_read_projected(gswt_ctx* c, void* out, size_t capacity_entries, size_t* n_entries)
try {
    if (!c || !n_entries) return GSWT_ERR_BAD_ARG;
    *n_entries = (size_t)c->sets[c->cur_set].n_entries;
    if (!out) return GSWT_OK;
    if (!c->opt.debug_varyings || !c->dbg.p) return fail(c, GSWT_ERR_STATE, "enable GSWT_OPT_DEBUG_VARYINGS and render first");
    if (capacity_entries < c->sets[c->cur_set].n_entries) return fail(c, GSWT_ERR_CAPACITY, "buffer holds %zu entries, need %llu", capacity_entries, (unsigned long long)c->sets[c->cur_set].n_entries);
    hipSetDevice(c->device);
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(out, c->dbg.p, (size_t)c->sets[c->cur_set].n_entries * sizeof(Varyings), hipMemcpyDeviceToHost));
    return GSWT_OK;
} GSWT_CATCH

}  // extern "C"
