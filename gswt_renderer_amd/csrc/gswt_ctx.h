// gswt_ctx.h -- what the host files of libgswt_hip.so share (gswt_api*.hip, gswt_worker.hip): the owning buffers, a sort event's
// draw set, a frame slot, the context itself, the error helpers and the few functions that cross files.  Internal: not part of
// the C ABI (include/gswt_hip.h), and host only -- nothing here is device code.
#pragma once

#include "../../include/gswt_hip.h"
#include "gswt_device.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

namespace gswt {

// Device and pinned host buffers own their memory: freed when the buffer goes out of scope (or by release()), moved but never copied.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // elements
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t n)
    {
        if (n <= cap) return hipSuccess;
        size_t ncap = n + n / 4 + 1024;
        T* np = nullptr;
        // (GSWT_LOG_ALLOC=1: every device allocation of the library on stderr -- a growth inside a frame loop frees the old buffer,
        // which waits for the device)
        static const bool log_alloc = getenv("GSWT_LOG_ALLOC") != nullptr;
        if (log_alloc) fprintf(stderr, "gswt alloc: %zu -> %zu bytes%s\n", cap * sizeof(T), ncap * sizeof(T), p ? " (grow: frees the old buffer)" : "");
        hipError_t e = hipMalloc(&np, ncap * sizeof(T));
        if (e != hipSuccess) return e;
        if (p) hipFree(p);
        p = np; cap = ncap;
        return hipSuccess;
    }
    // Buffers whose size follows the frame's pair count or a sort event's list sizes: when one has to grow it grows to TWICE the
    // request.  Growing frees the old buffer, which waits for the device -- with four frames in flight most of a millisecond, and
    // each frame slot / draw set repeats it when its turn comes (a fly path whose pair count crosses the old capacity stalled ~1 ms
    // per slot); 288 GB of HBM make the headroom cheap.
    hipError_t ensure_roomy(size_t n) { return n <= cap ? hipSuccess : ensure(2 * n); }
    void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
};
// (pair_box / self_box: first chunk box of the list in static_boxes; chunk k = the k-th 256 entries from the END of the list, as k_project walks it)
using ListRef = gswt::SceneList;       // (gswt_device.h: gswt_upload_scene_rows fills the same table on the device side)

// Behind synchronous copies whose data the frames read: the frame slots' streams are non-blocking, i.e. not ordered behind the
// null stream, and a synchronous copy from pageable memory may return once the data is staged.  Setup paths only.
static inline hipError_t null_stream_done() { return hipStreamSynchronize(nullptr); }

// pinned host staging (asynchronous uploads read it after the call has returned)
template <typename T>
struct HostBuf {
    T* p = nullptr;
    size_t cap = 0;
    HostBuf() = default;
    HostBuf(HostBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    HostBuf& operator=(HostBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~HostBuf() { release(); }
    hipError_t ensure(size_t n)
    {
        if (n <= cap) return hipSuccess;
        const size_t ncap = n + n / 4 + 64;
        T* np = nullptr;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&np), ncap * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) return e;
        if (p) hipHostFree(p);
        p = np; cap = ncap;
        return hipSuccess;
    }
    void release() { if (p) hipHostFree(p); p = nullptr; cap = 0; }
};

// Frame slots.  Round 1: c3 4 220 (two in flight) -> 4 600 frames/s (three); a fourth was SLOWER on a static camera (the frames then
// rotate over four sets of per-frame buffers and the working set outgrows the Infinity Cache).  Round 2: with sort events in the
// frame stream a fourth frame in flight covers the bubble a swap-in leaves (fly path 3 570 -> 3 770 frames/s) while it still costs
// a static camera 6 % (4 476 -> 4 214), so the library offers four and the caller decides how many it keeps in flight:
// gswt_render_async takes the lowest free slot, unused slots cost nothing.
// Frame slots = frames that can be in flight.  c3 fly path (worker thread + swap-ins), frames/s on one box with every slot in flight:
// 2: 3 770, 3: 4 095, 4: 4 445-4 500, 5: 4 770-4 790, 6: 4 700-4 765.  A static camera peaks at three in flight (bench.py keeps three
// there): more frames rotate over more sets of per-frame buffers and the working set outgrows the Infinity Cache.
#ifndef GSWT_FRAME_SLOTS
#define GSWT_FRAME_SLOTS 5
#endif
constexpr int kFrameSlots = GSWT_FRAME_SLOTS;
// Stream creation order (see gswt_create).  Measured on one box, c3 (tools: GSWT_STREAM_LAYOUT sweeps, gpurun_out/stream_layouts.txt):
//   layout        fly path, 4 / 5 in flight   static, 3 in flight   rank 0 of 8 (fake world): fly / static
//   c012p3s       4 492 / 4 658                4 924                 8 240 / 11 099      (fifth slot stream created at first use)
//   c012p34s      4 490 / 4 821                4 857                 8 055 /  8 849
//   c012p3ps      4 510 / 4 321                4 901                 7 790 /  8 767
//   c0123s        4 506 / 4 621                4 899                 7 317 / 10 241
// Four frames in flight do not care; the fifth frame pays only with its stream created in front of the build stream (which then
// shares its hardware queue with slot 2), and band frames of a sharded run want the older layout (bench.py sets it for --gpus N > 1).
constexpr const char* kStreamLayout = "c012p34s";

// The per-sort-event state (GSWTRenderer's swap-in of a SortData, state.rs:361-376): draw descriptors, chunk tables, merged
// lists, band-cull bounds.  Double-buffered: gswt_set_draws* fills the set that is NOT current while the frames in flight
// keep reading the one they were submitted with, so a sort event does not drain the frame pipeline.
// frames in flight + 1 (the set being refilled is never one a frame in flight still reads) + 4 more, so that with the sets refilled
// round robin the merged lists of the last kDrawSets - 1 = 9 sort events stay addressable for gswt_set_draws_merge_groups
constexpr int kDrawSets = kFrameSlots + 5;
static_assert(kDrawSets <= kMergeSources, "MergeSources holds one pointer pair per draw set");
static_assert(sizeof(gswt_render_config) == 32 && offsetof(gswt_render_config, out_format) == 28, "gswt_render_config layout");
static_assert(GSWT_OUT_RGBA32F == kOutF32 && GSWT_OUT_RGBA8_UNORM == kOutRGBA8 && GSWT_OUT_BGRA8_UNORM == kOutBGRA8, "output formats");
static_assert(GSWT_VIDEO_NV12 == kOutNV12 && GSWT_VIDEO_I420 == kOutI420, "video output formats");
static_assert(GSWT_MAX_CLIP_VOLUMES == kMaxClipVolumes && sizeof(gswt_clip_volume) == sizeof(ClipVolume) && sizeof(gswt_clip_volume) == 64 &&
              offsetof(gswt_clip_volume, shape) == offsetof(ClipVolume, shape), "gswt_clip_volume is ClipVolume");
static_assert(GSWT_CLIP_BOX == kClipBox && GSWT_CLIP_ELLIPSOID == kClipEllipsoid && GSWT_CLIP_HALFSPACE == kClipHalfspace &&
              GSWT_CLIP_KEEP == kClipKeep && GSWT_CLIP_GROUND == kClipGround, "clip shapes and flags");

struct DrawSet {
    // Everything a sort event uploads lives in ONE pinned host block mirrored by one device block of the same layout (a
    // single asynchronous copy on the ctx stream per event): draw records, per-draw XCD positions, and the tables of the
    // device-side merged-list step (groups to sort, their segments and block table; groups to copy, their block table and
    // map-id remap pairs; the sort's item count).  The views below point into the device block.
    HostBuf<uint8_t> h_blob;
    DevBuf<uint8_t> d_blob;
    size_t blob_bytes = 0;
    size_t off_draws = 0, off_xcd = 0, off_groups = 0, off_jobs = 0, off_remap = 0, off_segs = 0, off_blocks = 0, off_cblocks = 0, off_count = 0;
    template <typename T> T* hp(size_t off) { return reinterpret_cast<T*>(h_blob.p + off); }
    template <typename T> T* dp(size_t off) { return reinterpret_cast<T*>(d_blob.p + off); }
    hipError_t plan(size_t n_draws, size_t n_groups, size_t n_members, size_t total_entries)
    {
        size_t o = 0;
        auto take = [&o](size_t bytes) { const size_t at = o; o = (o + bytes + 255) & ~(size_t)255; return at; };
        const size_t n_blk = total_entries / 1024 + 2 * n_members + 2;          // upper bound of either block table
        off_draws = take((n_draws + 1) * sizeof(DrawDev)); off_xcd = take((n_draws + 1) * 4);
        off_groups = take((n_groups + 1) * sizeof(MergeGroup)); off_jobs = take((n_groups + 1) * sizeof(MergeCopy));
        off_remap = take((n_members + 1) * sizeof(uint2)); off_segs = take((2 * n_members + 1) * sizeof(MergeSeg));
        off_blocks = take(n_blk * sizeof(uint2)); off_cblocks = take(n_blk * sizeof(uint2)); off_count = take(sizeof(SortCount));
        blob_bytes = o;
        hipError_t e = o <= h_blob.cap ? hipSuccess : h_blob.ensure(2 * o);      // (grows to twice the request, like DevBuf::ensure_roomy)
        if (e != hipSuccess) return e;
        e = d_blob.ensure_roomy(o);
        if (e != hipSuccess) return e;
        draws = dp<DrawDev>(off_draws); xcd_first = dp<uint32_t>(off_xcd);
        return hipSuccess;
    }
    uint64_t per_xcd[8] = {};              // chunks per XCD launch list, and the longest of them
    uint64_t longest = 0;
    DrawDev* draws = nullptr;
    DevBuf<uint2> chunk_tab;
    DevBuf<uint2> chunk_tab_xcd;           // chunk_tab in k_project's launch order: all chunks of a draw on one XCD (DrawDev::xcd)
    DevBuf<uint32_t> merged_list, merged_map;
    uint32_t* xcd_first = nullptr;              // per draw: position of its first chunk in its XCD's launch list
    // what the merged arrays of this set hold, for the next sort event's reuse test (device-built sets only)
    struct GroupDesc { uint32_t view, base, len, first, n; uint64_t hash; };
    std::vector<GroupDesc> g_desc;
    std::vector<gswt_merge_member> g_members;
    bool g_valid = false;
    uint32_t src_mask = 0;                 // draw sets the device-side build of THIS set copies merged lists from (bit per set)
    hipEvent_t ev_up = nullptr;            // behind the upload: the pinned block may be refilled once it has fired
    bool ev_up_pending = false;
    bool built = false;                    // ev_up has been seen complete: frames on this set need not wait for it any more
    size_t n_merged = 0;
    uint32_t n_launch = 0;                 // length of chunk_tab_xcd (>= n_chunks: short per-XCD lists are padded)
    uint32_t n_draws = 0, n_chunks = 0;
    uint64_t n_entries = 0;
};

struct FrameImages {                       // the frame's images, all on the device (null: none; d_out is never null)
    const float4* d_bg = nullptr;          // the background's colour ...
    const float* d_bgd = nullptr;          // ... and depth
    float4* d_out = nullptr;
    float* d_out_depth = nullptr;          // gswt_render_depth / gswt_render_async_depth: the frame's depth image
    gswt_pick* d_out_pick = nullptr;       // gswt_render_pick / gswt_render_async_pick: the frame's pick image
};

// What a frame keeps from its submission: the state in force when it was submitted, which frames in flight and re-runs keep whatever is set
// meanwhile.  frame_modes (gswt_api.hip) takes the snapshot, project_modes (gswt_frame_modes.h) reads k_project's instantiation from it.
struct FrameModes {
    bool strict_vs = false, ortho = false; // GSWT_OPT_STRICT_VS, GSWT_OPT_PROJECTION = 1
    float aa_s = 0.0f;                     // GSWT_OPT_ANTIALIAS: s = 4 v / splat_scale^2 (0: off)
    Atmo atm = {};                         // gswt_set_atmosphere's block with its derived constants (all zero: off)
    int sty_ver = -1, shd_ver = -1;        // gswt_set_tile_styles' table, gswt_set_shadow_map's block and image: their versions in gswt_ctx::styles / shadows (-1: off)
    ClipSet clip = {};                     // gswt_set_clip_volumes' set, by value (n = 0: off): no version pool, the frame's copy is the version
};

struct FrameArgs {
    gswt_camera_uniforms cam;
    gswt_scene_uniforms su;
    gswt_render_config cfg;
    int width = 0, height = 0;
    FrameImages img;
    FrameModes modes;
};

// One version of gswt_set_tile_styles' table (a VersionPool payload): pinned staging (the host's entries) and the device copy k_project reads.
struct StyleVersion {
    HostBuf<uint2> h;
    DevBuf<uint2> d;
    uint32_t n = 0;
};

// One version of gswt_set_shadow_map's map, likewise: the validated block as the kernels read it (p.z: the device image) and pinned staging
// for an image that comes from a host pointer (a device image is copied device to device, no staging).
struct ShadowVersion {
    HostBuf<float> h;
    DevBuf<float> d;
    Shadow p = {};
};

// A frame's events on its slot's stream.  GSWT_OPT_TIMING >= 1 records kEvStart, kEvEnd and the compositor kernel's pair, 2 also the
// stage boundaries in between (nothing runs between kEvSorted and kEvRanges); kEvDone follows the frame's last command in any case.
enum FrameEvent { kEvStart, kEvProjected, kEvEmitted, kEvSorted, kEvRanges, kEvEnd, kEvCompositeBegin, kEvCompositeEnd, kEvPickBegin, kEvPickEnd, kEvDone, kFrameEvents };

// One frame in flight.  Each slot owns a stream and every per-frame buffer, so two frames overlap on the GPU:
// the latency-bound kernels of one (sort passes, single-workgroup scans, tails) fill the gaps of the other.
struct FrameSlot {
    hipStream_t stream = nullptr;
    hipEvent_t ev[kFrameEvents] = {};
    hipEvent_t ev_in = nullptr;            // recorded on the ctx stream at enqueue: the frame starts after it
    hipEvent_t ev_gather = nullptr;        // recorded on the ctx stream behind the frame's gather + re-assembly (gswt_render_gather / gswt_group_render_gather)
    bool gather_recorded = false;
    unsigned long long seq = 0;            // submission order of the frame in this slot
    FrameResult* hc = nullptr;             // pinned host: the result part of the frame's counter block (gswt_frame_layout.h)
    FrameResult* hc_dev = nullptr;         // the same words as the device sees them (k_combine writes them at the end of a frame)
    bool pending = false;                  // submitted through gswt_render_async, ticket not yet handed back by gswt_render_wait
    bool collected = false;                // finish_frame already ran for the pending frame (fence / gswt_set_draws*): its status and
    int collected_rc = 0;                  // timings wait here for gswt_render_wait
    gswt_timings collected_timings = {};
    FrameArgs args;
    int set = 0;                           // draw set the frame was submitted with (a re-run after overflow uses the same one)
    uint32_t cap = 0;
    int n_tiles = 0;
    int timing_level = 0;
    // per-frame HBM buffers
    DevBuf<uint2> rects;
    DevBuf<Rec> recs;
    DevBuf<uint4> live_tab;                // this frame's launch table of k_project: the chunks of the draws that survive k_cull
    DevBuf<uint32_t> live_cnt;             // entries per XCD list of live_tab (8 words, a cache line apart; zero between frames) + k_totals' copy for k_emit
    DevBuf<uint32_t> live_cid;             // live_tab's chunks as chunk numbers in slot order (k_emit walks the same table)
    DevBuf<uint32_t> cell_culled;          // column-band shards: per map cell, 1 = no splat of that tile instance can reach the band
    DevBuf<uint32_t> block_sums, draw_culled, keys_a, keys_b, vals_a, vals_b, ghist;
    DevBuf<uint2> ranges;
    DevBuf<uint32_t> item_base;
    DevBuf<uint4> item_tab;
    DevBuf<uint32_t> aux_a, aux_b;         // GSWT_ORDER_DEPTH: the pairs' tile ids, carried through the depth passes as the sort's payload
    uint32_t depth_passes = 0;             // GSWT_ORDER_DEPTH: radix passes this frame's depth sort was launched with
    bool depth_local = false;              // ... or the tile-local depth sort (k_tile_depth_sort)
    bool full_grid = false;                // this (re-run) frame launches k_project / k_emit over the whole launch table, whatever the hint says
    uint32_t n_launch_eff = 0;             // positions of the launch table this frame's grids cover
    // gswt_debug_read_pairs: the ping-pong buffer that held this slot's last frame's sorted slots (what the compositor walked), and that
    // frame's pair count once finish_frame has seen it complete (sorted_final; a re-run enqueues again and clears it)
    const uint32_t* sorted_vals = nullptr;
    uint32_t sorted_pairs = 0;
    bool sorted_final = false;
    DevBuf<float4> partials;
    DevBuf<float> partials_z;              // frames that write their depth: a segment's partial depth beside its partial colour
    DevBuf<uint2> partials_pick;           // frames that write their pick: a segment's (largest weight, pair) beside its partial colour
    bool pick_timed = false;               // this frame's k_pick_resolve carries kEvPickBegin / kEvPickEnd
    DevBuf<float4> col_f;                  // debug draw modes: float colours per slot
    DevBuf<float> depths;                  // per-slot depth: frames with a proxy depth buffer, GSWT_ORDER_DEPTH or a depth image only
    // hipGraph replay (GSWT_OPT_GRAPH): the chain of kernel nodes of this slot's frames and the argument records they were last set to
    GraphRec grec;
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    hipGraphNode_t graph_nodes[kGraphMaxNodes] = {};
    GraphNodeRec graph_last[kGraphMaxNodes];
    uint32_t graph_n = 0;
    void release_graph()
    {
        if (graph_exec) hipGraphExecDestroy(graph_exec);
        if (graph) hipGraphDestroy(graph);
        graph_exec = nullptr; graph = nullptr; graph_n = 0;
    }
};

// A resource that frames in flight keep their own version of (gswt_set_tile_styles' table, gswt_set_shadow_map's map), filled by asynchronous
// copies on the ctx stream.  A version is in use while it is the current one or a frame slot was last submitted with it (frames in flight and
// re-runs; `ver`: the FrameModes member that names it).  Any other one may be refilled, and of kFrameSlots + 2 one always can: no setter waits for a frame.
template <typename Payload>
struct VersionPool {
    static constexpr int kVersions = kFrameSlots + 2;
    struct Version : Payload {
        hipEvent_t ev_copied = nullptr;    // behind the version's copy: its staging may be refilled once it has fired ...
        bool copy_pending = false;         // ... and until then a refill waits for it
        ~Version() { if (ev_copied) hipEventDestroy(ev_copied); }
    };
    Version pool[kVersions];
    int cur = -1;                          // the version in force (-1: off), read when a frame is submitted
    void off() { cur = -1; }
    const Payload* get(int v) const { return v >= 0 ? &pool[v] : nullptr; }
    int free_version(const FrameSlot (&slots)[kFrameSlots], int FrameModes::*ver) const
    { return gswt::free_version(kVersions, cur, slots, [ver](const FrameSlot& sl) { return sl.args.modes.*ver; }); }
    // Before free version v is filled: only its own earlier copy (of a payload no frame ever used) can still be queued on the ctx stream.
    hipError_t begin_fill(int v, Payload** p)
    {
        Version& e = pool[v];
        *p = &e;
        const hipError_t err = e.copy_pending ? hipEventSynchronize(e.ev_copied) : hipSuccess;
        if (err != hipSuccess) return err;
        e.copy_pending = false;
        return e.ev_copied ? hipSuccess : hipEventCreateWithFlags(&e.ev_copied, hipEventDisableTiming);
    }
    // Behind version v's copies on the ctx stream: frames and proxy passes submitted from now on read it, and start behind that stream's queue.
    hipError_t commit(int v, hipStream_t ctx_stream)
    {
        const hipError_t err = hipEventRecord(pool[v].ev_copied, ctx_stream);
        if (err == hipSuccess) { pool[v].copy_pending = true; cur = v; }
        return err;
    }
};

// gswt_set_option's values with their defaults: read when the frame (or the sort event) is enqueued, but for the ones FrameModes snapshots.
struct Options {
    int no_prefilter = 0;                  // GSWT_OPT_NO_LOD_PREFILTER
    int debug_varyings = 0;
    int timing = 2;      // 0: no events, 1: frame + k_composite, 2: every stage
    // pairs per compositor work item (multiple of 256).  A tile's list is cut into segments that are composited in parallel and folded
    // by k_combine; a segment cannot know that the segments in front of it already saturated its pixels, so with the early-out on
    // (transmittance_eps > 0) short segments redo work that a longer one would have skipped.  k_composite alone, us (stage events):
    //   segment   512    768   1024   1536   2048   4096
    //   c3        96.3   96.9   96.0   95.7   97.9  141.5     (horizon tiles of 5-7 k pairs serialise at 4096)
    //   c3d (P = 8.2 M)  430    385    342    298    268    236
    //   c5        551     -     542     -     540     -
    // 1536 is the default; a host that knows its scene is dense raises it (bench.py: from the first frame's pairs per screen tile).
    int segment = 1536;
    int fixed_pair_cap = 0;   // test hook (GSWT_OPT_PAIR_CAP): the pair capacity is pinned until a frame overflows it
    int defer_swap = 0;
    int graph = 0;
    // GSWT_OPT_STRICT_VS (default ON since round 4: k_project<.,.,STRICT> costs +1 us of 71 at c3 and nothing in frames/s): vs_main is
    // evaluated operator by operator as gswt.wgsl:152-258 writes it; 0 selects the fma-chain / single-reciprocal sequence v2
    int strict_vs = 1;
    // GSWT_OPT_PROJECTION: 0 = perspective (vs_main as written), 1 = orthographic (k_project<.,.,.,ORTHO>: the constant affine Jacobian in place of
    // gswt.wgsl:213-232).  Read when a frame is submitted (validate_frame, submit_frame); setting it waits for nothing.
    int projection = 0;
    // GSWT_OPT_ANTIALIAS: variance of the pixel filter in 1/1024 px^2 (0 = off, 1..4096).  Read when a frame is submitted, like the projection.
    int antialias = 0;
    int no_chunk_cull = 0;                 // GSWT_OPT_NO_CHUNK_CULL: k_cull keeps every chunk of a surviving draw (A/B and tests: same image)
    int no_merge_reuse = 0;                // GSWT_OPT_NO_MERGE_REUSE: every merged group is re-sorted at every sort event
    // GSWT_OPT_DEPTH_SORT: 0 / 2 = tile-local (lists of any length: the ones beyond the LDS buffer go through global memory,
    // k_tile_depth_sort_xl), 1 = the global passes.
    int depth_sort = 0;
};

}  // namespace gswt

struct gswt_ctx {
    int device = 0;
    gswt::FrameSlot slots[gswt::kFrameSlots];
    unsigned long long frame_seq = 0;      // frames submitted through gswt_render_async
    hipStream_t stream = nullptr;
    bool own_stream = true;
    std::string err;
    gswt::Options opt;
    // gswt_set_atmosphere: the block in force, validated (all zero: off).  Read when a frame is submitted and when gswt_proxy_render is called.
    gswt_atmosphere atm = {};
    gswt::VersionPool<gswt::StyleVersion> styles;      // gswt_set_tile_styles' table
    gswt::VersionPool<gswt::ShadowVersion> shadows;    // gswt_set_shadow_map's map: read when a proxy pass is called, too
    gswt::ClipSet clip = {};                           // gswt_set_clip_volumes' set in force, validated (n = 0: off): read when a frame is submitted and when a proxy pass is called
    // scene
    gswt::DevBuf<uint4> tex;
    size_t n_splats = 0;
    float loc_lo[3] = {}, loc_hi[3] = {}, loc_max_trace = 0.0f;      // tile-local bounds of the splat centres, largest covariance bound (trace when PSD)
    gswt::DevBuf<uint32_t> static_list;
    gswt::DevBuf<float> static_boxes;      // tile-local bounding box (lo.xyz, hi.xyz) of every 256-entry chunk of every static list (k_live's chunk cull)
    std::vector<gswt::ListRef> lists;
    size_t static_n = 0, boxes_n = 0;      // entries of static_list, chunk boxes of static_boxes
    int n_lod = 0, n_tile = 0, n_view = 0;
    bool scene_ready = false;
    gswt::DevBuf<float> hmap;
    int hm_w = 0, hm_h = 0;
    // bounds of the height map for the column-band cull on the HeightMap surface: texel min / max, and the largest texel-to-texel
    // step along u and along v (repeat addressing) times the map's width / height = the largest slope of the bilinear surface
    // per unit of u / v (a bilinear sample lies between its texels, a difference quotient of it below the largest texel slope)
    float hm_min = 0.f, hm_max = 0.f, hm_du = 0.f, hm_dv = 0.f;
    // background passes
    gswt::DevBuf<float4> sky_faces;
    int sky_size = 0, sky_equi = 0;
    gswt::DevBuf<float4> proxy_tex;
    int proxy_size = 0, proxy_mips = 0, proxy_grid_dim = 2048;
    uint32_t proxy_mip_off[16] = {};
    // draws
    gswt::DrawSet sets[gswt::kDrawSets];
    int cur_set = 0;                       // the set frames submitted from now on read
    int latest_set = 0;                    // the set filled last (== cur_set unless a deferred swap-in is pending)
    int pending_set = -1;                  // GSWT_OPT_DEFER_SWAP: filled, still being built on set_stream, not yet read by frames
    hipStream_t set_stream = nullptr;      // uploads and device-side builds of a sort event: beside the frames, not in front of them
    std::vector<hipStream_t> pad_streams;  // never used: they steer the hardware-queue assignment (gswt_create)
    unsigned long long stat_graph_launches = 0, stat_graph_rebuilds = 0, stat_graph_node_updates = 0;
    int pending_frames = 0;                // GSWT_OPT_DEFER_SWAP >= 2: frames still to be submitted on the old set
    // on-device merged lists
    gswt::DevBuf<int32_t> raw_depth;
    std::vector<uint32_t> raw_off;          // [(lod*n_tile + tile)*n_view + view] -> offset in raw_depth
    std::vector<uint32_t> raw_cnt, raw_merge_offset;   // [lod*n_tile + tile]
    unsigned long long stat_groups_built = 0, stat_groups_reused = 0, stat_groups_reused_deep = 0;
    gswt::DevBuf<uint32_t> mg_ws;
    bool draws_ready = false;
    // frame (the per-frame buffers live in the slots)
    uint32_t pair_cap = 0;                 // capacity the pair buffers / grids are sized for (grows on overflow)
    // GSWT_ORDER_DEPTH: the number of 8-bit passes of the depth sort: as many as the key ranges of the recent frames needed (the depths of one c3 frame span ~2^21
    // ulps: three).  A frame that needs more is flagged on the device and re-run; 32 frames in a row that need fewer give one back.
    uint32_t depth_passes = 3;
    uint32_t depth_passes_low_run = 0, depth_passes_low_max = 0;
    // ... or the tile-local path: tile passes first (depth bits as payload), then one kernel that depth-sorts each tile's slice in LDS
    // (Options::depth_sort).
    // Launch grids of k_project / k_emit: the launch table has a position for every chunk of the draw list, the frame's live chunks fill its
    // head (k_cull), and every position past an XCD's live count is a workgroup that starts, reads the count and leaves -- 300 k of them at c5.
    // The grids cover the longest live list of the last finished frame (k_totals reports it) + 50 % + 256; a frame whose own lists turn out
    // longer is flagged by k_totals and re-run with the full grid, like a pair overflow.  (+ 25 % + 64 was too tight on c3's fly path: a sort
    // event re-balances the lists, frames were re-run, 5 250-5 310 against 5 440-5 470 frames/s; with + 50 % c3's grid is the whole table again
    // -- 17.8 k positions for 10.7 k live chunks -- and c5's is 80 k of 366 k: 736-742 against 723-728 frames/s.  The cut is only taken where it
    // removes at least half of the grid.)
    uint32_t live_hint = 0;                // longest live list (per XCD) of the last finished frame; 0: none yet
    uint32_t depth_max_tile_len = 0;       // longest tile list of the last finished depth-ordered frame (0: none yet; gswt_debug_depth_stats)
    unsigned long long stat_depth_local = 0, stat_depth_global = 0;     // depth-ordered frames enqueued on either path (re-runs included)
    int last_slot = 0;
    gswt::DevBuf<float4> bg_rgba, out_img;
    gswt::DevBuf<float> bg_depth, out_depth_img;       // (gswt_render's staging of host images)
    gswt::DevBuf<uint4> out_pick_img;
    gswt::DevBuf<gswt::Varyings> dbg;
    uint32_t last_n_tiles = 0;
    gswt_timings timings = {};
    // multi-GPU gather: RCCL communicator (one process per GPU) or a local group of contexts (one process, peer copies)
    void* comm = nullptr;                  // ncclComm_t
    int comm_rank = 0, comm_world = 0;
    std::vector<gswt_ctx*> group;          // non-empty: hipMemcpyPeerAsync transport; group[r] is rank r
    int group_rank = 0;
    gswt::DevBuf<float4> gather_buf;       // world x shard image, as an all-gather delivers them
    hipEvent_t ev_push = nullptr;          // local group: this rank's shard has been pushed to every peer
    hipEvent_t ev_unshard = nullptr;       // local group: this rank's re-assembly of the PREVIOUS gather has read its gather buffer
    bool unshard_pending = false;          // ... and has been recorded at least once

    // Releases what the members do not release themselves (the buffers and the version pools do): streams, events, the pinned counter words, graphs and the
    // RCCL communicator.  The caller has made the ctx's device current and nothing is in flight (gswt_api.hip).
    ~gswt_ctx();
};

namespace gswt {

inline int fail(gswt_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

// waits for the ctx stream and every frame slot's stream
inline hipError_t sync_all(gswt_ctx* c)
{
    hipError_t e = hipStreamSynchronize(c->stream);
    if (c->set_stream) { hipError_t e2 = hipStreamSynchronize(c->set_stream); if (e == hipSuccess) e = e2; }
    for (auto& sl : c->slots)
        if (sl.stream) { hipError_t e2 = hipStreamSynchronize(sl.stream); if (e == hipSuccess) e = e2; }
    return e;
}

// No C++ exception may unwind through the C ABI: every extern "C" body that returns a status is a function-try-block
// closed by this handler (std::vector / std::string allocations of the draw-list code are the throwing sites; the worker's
// entry points are called from a second host thread and take a std::mutex).
#define GSWT_CATCH                                                                         \
    catch (const std::bad_alloc&) { return GSWT_ERR_CAPACITY; }                             \
    catch (...) { return GSWT_ERR_HIP; }

#define HIP_TRY(c, expr)                                                                              \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) return gswt::fail((c), GSWT_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// Which draw set the next sort event fills, and when frames start reading it.  Sets rotate; the one after the set filled last is
// free once the frames still reading it have been collected.  By default a new set is current at once (the next frame waits for its
// build on the device).  With GSWT_OPT_DEFER_SWAP it becomes current with the first frame submitted AFTER its build has finished
// on set_stream: frames submitted meanwhile keep the previous list and nothing waits -- the reference's swap-in likewise takes
// effect with the frame after the worker's message (state.rs:361-376).  With a value n >= 2 it becomes current with the n-th frame
// submitted after the call whatever the device is doing (that frame waits if the build is late): ranks that render the shards of
// one frame stream then all switch at the same frame.  At most one set is pending: the next event makes it current.
// (Here because every submitted frame calls it, gswt_api.hip, and every sort event, gswt_api_draws.hip.)
inline void activate_pending(gswt_ctx* c, bool force)
{
    if (c->pending_set < 0) return;
    DrawSet& P = c->sets[c->pending_set];
    bool now = force;
    if (!now && c->opt.defer_swap >= 2) now = c->pending_frames-- <= 0;                       // a fixed number of frames later: the same on every rank
    else if (!now) now = !P.ev_up || hipEventQuery(P.ev_up) == hipSuccess;                    // as soon as it has been built
    if (now) { c->cur_set = c->pending_set; c->pending_set = -1; }
}

// gswt_set_atmosphere's block as the kernels read it: the derived constants in binary32, one operation per operator (include/gswt_hip.h).
// A part that is off leaves its fields zero.
inline Atmo atmo_constants(const gswt_atmosphere& a)
{
    Atmo m = {};
    if (a.fade_end > 0.0f) { m.fade_end = a.fade_end; m.fade_inv = 1.0f / (a.fade_end - a.fade_start); }
    if (a.fog_density > 0.0f) {
        m.fog_density = a.fog_density; m.fog_start = a.fog_start; m.fog_max = a.fog_max;
        for (int k = 0; k < 3; k++) m.fog_color[k] = a.fog_color[k];
    }
    return m;
}

// gswt_set_shadow_map's version v as a kernel argument (-1: off, all zero)
inline Shadow shadow_version(const gswt_ctx* c, int v) { const ShadowVersion* sv = c->shadows.get(v); return sv ? sv->p : Shadow{}; }

// What the proxy passes see of gswt_set_clip_volumes' set: its volumes flagged GSWT_CLIP_GROUND, in their order (n = 0: the pass is unclipped)
inline ClipSet clip_ground_subset(const ClipSet& s)
{
    ClipSet g = {};
    for (uint32_t k = 0; k < s.n; k++)
        if (s.v[k].flags & kClipGround) {
            g.n_keep += (s.v[k].flags & kClipKeep) ? 1u : 0u;
            g.v[g.n++] = s.v[k];
        }
    return g;
}

// opengl_to_wgpu * projection (gswt.wgsl:152-160, proxy.wgsl:84-91): clip z = (z + w) / 2, the other rows as they are
inline void gl_to_wgpu_projection(const float* P, float* GP)
{
    for (int cc = 0; cc < 4; cc++) {
        GP[4 * cc + 0] = P[4 * cc + 0];
        GP[4 * cc + 1] = P[4 * cc + 1];
        GP[4 * cc + 2] = 0.5f * P[4 * cc + 2] + 0.5f * P[4 * cc + 3];
        GP[4 * cc + 3] = P[4 * cc + 3];
    }
}

// Which rows and columns a shard's frame writes and how large its image is: `world` shards in all, interleaved tile rows (each
// shard's image is out_rows x width) or, in column mode, one contiguous band of tile columns of equal width on every rank
// (height x out_w).  Built on gswt_shard_rows_padded / gswt_shard_cols_padded.  rows_padded and band_px are what k_unshard takes:
// the rows of a row shard's image, and the band width of the column layout (0: row layout) -- the layout of an unshard follows
// the mode alone, so band_px is set for a single column "shard" too, where `cols` (a frame's band mode) is not.
struct ShardGeom {
    int world;
    bool cols;
    int out_rows, out_w;
    size_t px, bytes;
    int band_tiles, col0, col1, out_x0;    // the band in screen tiles [col0, col1) and its first pixel column (row mode: every column)
    int rows_padded, band_px;
};
ShardGeom shard_geom(const gswt_render_config& cfg, int width, int height);      // gswt_api_comm.hip

// ---- slot collection (gswt_api.hip, beside finish_frame) ----
// Runs the slot's pending frame to completion (including the re-run of a frame whose pair buffers overflowed); its status and timings
// wait in the slot for the ticket's gswt_render_wait.  Nothing to do for a slot without a pending frame or one already collected.
void collect_slot(gswt_ctx* c, FrameSlot& sl);
// collect_slot on every slot while the state the frames were submitted with -- scene, draw list, capacities -- is still in place, then
// waits for every stream.  Called before anything that changes that state.
hipError_t collect_pending(gswt_ctx* c);

// ---- between subsystems ----
void invalidate_merge_sources(gswt_ctx* c);                   // gswt_api_draws.hip: a new scene or new raw depths retire the retained merged lists
void rccl_comm_destroy(void* comm);                           // gswt_api_comm.hip: ncclCommDestroy through the loaded library

}  // namespace gswt
