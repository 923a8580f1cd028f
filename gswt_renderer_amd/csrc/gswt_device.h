// gswt_device.h -- device-side data layout shared by the kernels and the C-ABI host code.
// Internal to libgswt_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
// the frame's bookkeeping layouts (counter block, sort count and workspace, super-group sums, live table, tile ranges): free of HIP,
// __host__ __device__ here.  (GSWT_HD is left as it was found: gswt_device_fn.h sets it for host/gswt_math.h and its like.)
#ifndef GSWT_HD
#define GSWT_HD __host__ __device__
#include "gswt_frame_layout.h"
#undef GSWT_HD
#else
#include "gswt_frame_layout.h"
#endif
#include "gswt_frame_modes.h"

namespace gswt {

constexpr int kTile = 16;            // screen tile edge, pixels (BASELINE north_star: 16x16 binning)
constexpr int kChunk = 256;          // list entries per projection workgroup
// Chunk k of a list of `count` entries is its k-th 256 entries from the END, [count - 256 (k + 1), count - 256 k) cut at 0: the order
// k_project walks a list in, and what a chunk box of the static lists bounds (gswt_upload_scene on the host, k_scene_boxes).
__host__ __device__ inline void chunk_entry_range(uint32_t count, uint32_t k, uint32_t& lo, uint32_t& hi)
{
    hi = count - k * (uint32_t)kChunk;
    lo = hi > (uint32_t)kChunk ? hi - (uint32_t)kChunk : 0u;
}
constexpr uint32_t kLodShift = 28;   // packed list entry = gs_index | lod_id << 28
constexpr uint32_t kIdxMask = (1u << kLodShift) - 1u;
// output image formats, GSWT_OUT_* of gswt_hip.h: RGBA f32 (16 B per pixel), bytes R G B A, bytes B G R A (4 B per pixel)
constexpr int kOutF32 = 0, kOutRGBA8 = 1, kOutBGRA8 = 2;
// ... and the 4:2:0 video formats, GSWT_VIDEO_*: plane Y (rows x out_w bytes), then the interleaved Cb Cr plane (NV12) or the Cb and the Cr
// plane (I420), rows / 2 x out_w / 2 samples each; rows and out_w even
constexpr int kOutNV12 = 16, kOutI420 = 17;
constexpr bool out_is_video(int out_format) { return out_format == kOutNV12 || out_format == kOutI420; }
// Bytes of a rows x out_w image in out_format: THE place that knows the layouts (gswt_out_image_bytes exports it).  0: unknown format,
// negative size, or a video format with an odd size.
inline size_t out_image_bytes(int out_format, int rows, int out_w)
{
    if (rows < 0 || out_w < 0) return 0;
    const size_t px = (size_t)rows * (size_t)out_w;
    if (out_format == kOutF32) return px * 16u;
    if (out_format == kOutRGBA8 || out_format == kOutBGRA8) return px * 4u;
    if (out_is_video(out_format)) return ((rows | out_w) & 1) ? 0 : px + px / 2u;
    return 0;
}

// Device-side draw descriptor: what one reference draw call binds (renderer.rs:499-590).
struct DrawDev {
    uint32_t single_draw;
    int32_t valid_lod_id;
    uint32_t changing;
    int32_t changing_to_lower;
    uint32_t tile_lod;        // tile_id.x
    float off[3];             // tile offset
    uint32_t list_base;       // first packed entry of this draw's list in its arena
    uint32_t count;           // list length
    uint32_t merged;          // 0: static arena, 1: merged arena (has map ids)
    uint32_t slot_base;       // first composite-order slot of this draw (multiple of kChunk)
    uint32_t cull_enable;
    uint32_t lod;             // tid.0 for lod_enable
    float corners[12];
    uint32_t entry_base;      // index of the first entry in draw order (debug output)
    int32_t single_lod_id;    // TileUniforms.single_lod_id (debug draw mode 3)
    uint32_t tile_idx;        // tile_id.y (debug draw mode 1)
    uint32_t tile_view;       // tile_id.z (debug draw mode 4)
    uint32_t map_coord[2];    // TileUniforms.map_coord (sphere surface)
    uint32_t box_base;        // static draws: first chunk box of the draw's list (chunk k = the k-th 256 entries from the END of the list); ~0: none
    uint32_t xcd;             // the XCD (0..7) all chunks of this draw are projected on (gswt_set_draws: the least loaded one when the draw is planned)
    uint32_t map_index;       // TileUniforms.map_index: the tile instance a static draw's splats belong to (pick output; a merged draw's come from merged_map)
    uint32_t _pad;
};

// gswt_set_atmosphere's block as the kernels read it (include/gswt_hip.h): the host derives it once per frame / proxy pass in binary32.
// All zero: off.  fade_end > 0: the far fade is on; fog_density > 0: the distance fog is on.
struct Atmo {
    float fade_end, fade_inv;              // fade_inv = 1.0f / (fade_end - fade_start)
    float fog_density, fog_start, fog_max;
    float fog_color[3];
};

// gswt_set_shadow_map's block and image as the kernels read them (include/gswt_hip.h): a kernel argument of its own beside Frame / ProxyArgs,
// so that neither struct grows and the instantiations without SHD stay the code they were.  z null: shadows off (all zero).
struct Shadow {
    float row[3][4];                       // rows 0..2 of world_to_light: light NDC x, y and the depth image's depth of a world point
    float bias, strength;
    float shade[3];
    int32_t w, h;                          // the depth image, row 0 at the top
    uint32_t _pad;                         // (no implicit padding: a recorded graph node compares its argument bytes)
    const float* z;
};
static_assert(sizeof(Shadow) == 88, "Shadow has no implicit padding");

// gswt_set_clip_volumes' set as the kernels read it (include/gswt_hip.h): by value, a kernel argument of its own beside Frame / ProxyArgs like
// Shadow, so that neither struct grows and the instantiations without CLIP stay the code they were.  n = 0: off.  Entries past n are zero.
// The proxy passes get the subset flagged GSWT_CLIP_GROUND (clip_ground_subset).
constexpr uint32_t kMaxClipVolumes = 8;
constexpr uint32_t kClipBox = 0, kClipEllipsoid = 1, kClipHalfspace = 2;      // GSWT_CLIP_* shapes
constexpr uint32_t kClipKeep = 1, kClipGround = 2;                            // ... and flags
struct ClipVolume {
    float row[3][4];                       // world_to_unit, rows 0..2
    uint32_t shape, flags;                 // GSWT_CLIP_BOX / _ELLIPSOID / _HALFSPACE; GSWT_CLIP_KEEP | GSWT_CLIP_GROUND
    uint32_t _pad[2];
};
struct ClipSet {
    uint32_t n, n_keep;                    // volumes in force, and how many of them are keep volumes
    uint32_t _pad[2];                      // (no implicit padding: a recorded graph node compares its argument bytes)
    ClipVolume v[kMaxClipVolumes];
};
static_assert(sizeof(ClipVolume) == 64 && sizeof(ClipSet) == 16 + 64 * kMaxClipVolumes, "ClipSet has no implicit padding");

// Per-frame constants (kernel argument, by value).
struct Frame {
    float V[16];       // view
    float GP[16];      // opengl_to_wgpu * projection   (gswt.wgsl:152-160)
    float VP[16];      // projection * view             (camera.rs:86-88) for the tile cull
    float focal[2];
    float htan[2];
    float cam_pos[3];
    float W, H;
    // scene uniforms
    float splat_scale, tile_width, clip_height, point_cloud_radius, transition_width_ratio, sphere_radius;
    uint32_t use_clip, surface_type, num_lod, draw_mode;
    uint32_t map_half_wh[2];
    int32_t center_coord[2];
    float transition_dist[16];
    float height_map_scale[3];
    float scene_scale[3];
    // render config
    float culling_dist;
    uint32_t lod_enable_mask;
    float t_eps;
    int32_t has_depth;       // proxy depth buffer bound
    // screen tiling / sharding
    int32_t width, height, tiles_x, tiles_y;
    int32_t shard_index, shard_count;      // interleaved tile-row sharding (count 1 = off)
    // contiguous tile-column band (off: col0 = 0, col1 = all columns).  tiles_x is the number of columns THIS ctx composites.
    int32_t col0, col1;
    int32_t out_w, out_x0;                 // width of the output image in pixels and the frame pixel column of its column 0
    int32_t band_cull;                     // 1: k_cull drops the draws / merged-group members whose splats cannot reach the band
    float loc_lo[3], loc_hi[3];            // tile-local bounds of every splat centre of the scene (gswt_upload_scene)
    float loc_max_trace;                   // largest trace of a stored covariance (>= its largest eigenvalue)
    float surf_zlo, surf_zhi;              // HeightMap surface: range of the mapped height h(x, y) * height_map_scale.z (0, 0 on the plain surface)
    float surf_f2;                         // bound of |F|^2 of the surface frame F (1 on the plain surface): Vrk -> F Vrk F^T
    int32_t hm_w, hm_h;
    uint32_t tiles_x_magic;                // floor(2^32 / tiles_x) + 1: tile -> (column, row) by multiply-high for tile ids below 2^16 (tile_xy)
    uint32_t map_wh_y, map_wh_y_magic;     // height of the tile map in cells (gswt.wgsl:53-56) and floor(2^32 / it) + 1 (quotients of 16-bit map ids by multiply-high)
    float aa_s;                            // GSWT_OPT_ANTIALIAS: s = 4 v / splat_scale^2, what the pixel filter adds to cov2d's diagonal (0: off)
    Atmo atm;                              // gswt_set_atmosphere as it stood when the frame was submitted (k_project<.., ATM> only)
};

// Projected splat record consumed by the compositor (32 B, two 16-B words; one 32-B-aligned sector per gather).
//   q0 = (iux, iuy, ivx, ivy)   q1 = (ndc.x, ndc.y, alpha, rgba8 bits)
// iu / iv: rows of the inverse affine map pixel -> quad space (F2); the centre stays in NDC (round 4): the compositor derives its offset
// from a tile origin with one rounding (F3), instead of subtracting the origin from a pixel-space centre that carries two roundings at ~W.
// The conservative pixel half extents of |p| <= 2 are re-derived from iu / iv by the compositor's staging lane; the depth
// lives in a side array (4 B per slot) that only depth-tested (proxy depth bound) and depth-ordered frames touch.
struct __attribute__((aligned(32))) Rec {
    float iux, iuy, ivx, ivy;
    float ndcx, ndcy, alpha, rgba8;
};

// Device-side merged-list building (see k_mg_* in gswt_kernels.hip)
struct MergeSeg {
    uint32_t group, src, len, start, gs_offset, map_index, lod, _pad;
};
struct MergeGroup {
    uint32_t base, len;       // range in the BUILD space (the concatenation of the groups that are sorted this event)
    int32_t mn, mx;
    uint32_t out_base;        // first entry of the group in the merged arrays
    uint32_t _pad[3];
};
// A group whose (view, ordered member tids) equal a group of the previous sort event: its list is copied from the previous
// draw set, map ids rewritten member by member (the reference's LRU hit, wangtile.rs:575-593).
struct MergeCopy {
    uint32_t src, dst, len;   // ranges in the source / new merged arrays
    uint32_t first_pair, n_pairs;   // (old map index, new map index) pairs of its members in the remap table; n_pairs = 0: map ids unchanged
    uint32_t src_set;         // which retained draw set holds the source list (MergeSources)
    uint32_t _pad[2];
};
// Scene preparation on the device (gswt_upload_scene_rows, gswt_scene.hip).  One static list [lod][tile][view] of the arena: its pair list
// at pair_base, then its self list; pair_box / self_box: the first chunk box of each in static_boxes (chunk k = the k-th 256 entries from
// the END of the list, as k_project walks it).  Also the host-side table of gswt_upload_scene.
struct SceneList { uint32_t pair_base, pair_count, self_base, self_count, pair_box, self_box; };
constexpr int kSceneMaxViews = 16;
struct SceneViews {
    uint32_t n_view;
    float vp[kSceneMaxViews][16];     // sort_projection * view of every presort view, column-major
};
// The merged arrays of the retained draw sets a copy job may read from: the lists of the last kMergeSources - 1 sort events stay
// addressable, keyed by (view, ordered member tile ids, transition states) -- the reference's LRU of merged lists (wangtile.rs:427,575-593).
constexpr int kMergeSources = 12;
struct MergeSources {
    const uint32_t* list[kMergeSources];
    const uint32_t* map[kMergeSources];
};

// vs_main varyings for the debug/parity hook (48 B, same layout as the oracle's orc_splat)
struct Varyings {
    int32_t visible;
    float ndc[2];
    float depth;
    float major[2];
    float minor[2];
    float rgba[4];
};

// Kernel arguments of the background passes (gswt_passes.hip)
struct SkyArgs {
    float V[16];          // view (only its rotation is used: skybox.wgsl:41-47 removes the translation)
    float p00, p11;       // projection[0][0], projection[1][1] (symmetric perspective, camera.rs:94)
    int width, height, face_size, equirectangular;
};

// k_skybox_bake (skybox.rs:490-668): per face i the rows s, u, f of the bake view look_at_rh(0, target_i, up_i) (skybox.rs:584-617);
// the view ray of the face pixel at NDC (x, y) is s*x + u*y + f
struct SkyBakeArgs {
    float basis[6][9];    // [face] = s.xyz, u.xyz, f.xyz
    int face_size, equi_w, equi_h;
};

// One level of the proxy texture's Lanczos3 mip build (upload_proxy_texture, proxy.rs:513-554: image::imageops::resize of the
// ORIGINAL image to n x n): plan_proxy_mip fills it; the tap tables, the vertical pass (h -> n rows, f32 intermediate
// [n][src_w]) and the horizontal pass (src_w -> n columns, quantised into the chain) of gswt_passes.hip read it.
struct ProxyMipArgs {
    int src_w, src_h, n;
    int u16;                // 0: RGBA8 source (4 B per texel), 1: RGBA16 (8 B per texel)
    int pitch;              // staged source row pitch in bytes, a multiple of 16
    int copy;               // (n, n) == (src_w, src_h): the crate copies; the level is a conversion, not a resample
    int stride_v, stride_h; // weights per output in the vertical / horizontal tap table (>= any output's tap count)
    int splits, chunk;      // vertical pass: the taps of every output split into `splits` runs of `chunk`; > 1: partial sums
    float maxv;             // 255 or 65535
};
ProxyMipArgs plan_proxy_mip(int src_w, int src_h, int n, int u16, int pitch);
// device elements each buffer of one level's build needs (0 for a copy level)
inline size_t proxy_mip_tmp_texels(const ProxyMipArgs& a) { return a.copy ? 0 : (size_t)a.n * a.src_w; }
inline size_t proxy_mip_part_texels(const ProxyMipArgs& a) { return a.copy || a.splits == 1 ? 0 : (size_t)a.splits * a.n * a.src_w; }
inline size_t proxy_mip_weights(const ProxyMipArgs& a, int axis) { return a.copy ? 0 : (size_t)a.n * (axis == 0 ? a.stride_v : a.stride_h); }

struct ProxyArgs {
    // proxy.wgsl Uniforms
    float height_offset, tile_width, width_scale, clip_height, brightness;
    uint32_t surface_type, use_clip, black_background;
    float V[16], GP[16];
    float p00, p11;
    float cam[3];
    uint32_t map_half_wh[2];
    float height_map_scale[3];
    // grid
    int nx, ny;
    float cs, gx0, gy0;
    // resources
    int hm_w, hm_h, tex_size, n_mips;
    uint32_t mip_off[16];          // float4 offsets of the mip levels
    int width, height;
    Atmo atm;                      // gswt_set_atmosphere as it stands when the pass is called: proxy_colour<FOG> reads the fog part
    // The orthographic passes only (proxy_ray<ORTHO> of either kernel; zero for a perspective pass, which never reads them).  k_proxy<., ORTHO>
    // works in the GRID FRAME, world - (gx0, gy0, 0): V[12..14] and cam are given in it, so that no sum cancels at the magnitude of the world
    // coordinates; k_proxy_sphere<., ORTHO> in the world frame (g = 0).
    float ortho_t[2];              // projection[12], projection[13]
    float ortho_o[3];              // grid-frame point of camera-space (0, 0, z0): the ray origin of ndc (p[12], p[13])
    float ortho_d[3];              // the rays' direction: -(V[2], V[6], V[10]), or its negative where depth falls along the view axis
    float ortho_uv0[2];            // frac((gx0, gy0) / tile_width / 4): what the grid frame's uv lacks, up to whole texture periods
};

// gswt_proxy_render_sphere only: what k_proxy_sphere's own part (the sphere roots, the unfolding's uv, the LOD) reads beside a ProxyArgs whose
// grid fields it leaves alone; the shared stages (proxy_ray, proxy_write, proxy_colour) read the ProxyArgs.  The orthographic form runs with
// g = 0: the sphere is centred at the world origin, the rays are of the planet's size there.
struct SphereProxyArgs {
    float r;                       // sphere_radius + height_offset: the ground sphere
    float sphere_radius;           // the splats' sphere: mapped_z = (hit.z / r) * sphere_radius is what use_clip tests
    float block_w;                 // (2 half_w tile_width) / 5
    float org[2];                  // (center_coord - half) tile_width: the plane origin map_sphere_surface subtracts
    float lod_k;                   // half_w tex_size / (4 PI r): texels per world unit at the equator
};

// ---- hipGraph replay of a frame's launch sequence (GSWT_OPT_GRAPH) -------------------------------------------------------------
// The frame is a fixed chain of kernel launches whose grids follow capacities; what changes from frame to frame is a handful of
// kernel arguments (the camera block, the output pointer).  With a recorder set, the launch sites of the frame path do not
// launch: they leave (function, grid, block, packed arguments) per kernel, and the caller replays the chain as ONE
// hipGraphLaunch, after updating only the kernel nodes whose record differs from the previous frame's.
struct GraphNodeRec {
    const void* fn = nullptr;
    dim3 grid, block;
    uint32_t n_args = 0, n_bytes = 0;
    uint16_t offs[40];
    alignas(16) unsigned char args[1536];      // (k_project: Frame, 19 pointers, the shadow block and the clip set are 1 320 bytes)
    template <typename T>
    void push(const T& v)
    {
        static_assert(alignof(T) <= 16, "kernel argument alignment");
        n_bytes = (n_bytes + (uint32_t)alignof(T) - 1u) & ~((uint32_t)alignof(T) - 1u);
        if (n_args >= 40u || n_bytes + sizeof(T) > sizeof(args)) { fn = nullptr; return; }      // (checked by the caller: a null fn fails the frame)
        memcpy(args + n_bytes, &v, sizeof(T));
        offs[n_args++] = (uint16_t)n_bytes;
        n_bytes += (uint32_t)sizeof(T);
    }
    bool same(const GraphNodeRec& o) const
    {
        return fn == o.fn && grid.x == o.grid.x && grid.y == o.grid.y && grid.z == o.grid.z && block.x == o.block.x && n_args == o.n_args &&
               n_bytes == o.n_bytes && memcmp(args, o.args, n_bytes) == 0;
    }
};
constexpr uint32_t kGraphMaxNodes = 32;          // reference order: 10-12 kernels per frame; GSWT_ORDER_DEPTH: 19-23
struct GraphRec {
    GraphNodeRec nodes[kGraphMaxNodes];
    uint32_t n = 0;
    bool overflow = false;
};
// the recorder of the calling thread (null: the launch sites launch); set around the frame's launch sequence by gswt_api.hip
GraphRec*& graph_recorder();

template <typename... KA, typename... A>
inline void graph_record(GraphRec* rec, void (*k)(KA...), dim3 g, dim3 b, A&&... a)
{
    static_assert(sizeof...(KA) == sizeof...(A), "kernel argument count");
    if (rec->n >= kGraphMaxNodes) { rec->overflow = true; return; }
    GraphNodeRec& nd = rec->nodes[rec->n++];
    nd.fn = reinterpret_cast<const void*>(k);
    nd.grid = g; nd.block = b; nd.n_args = 0; nd.n_bytes = 0;
    memset(nd.args, 0, sizeof(nd.args));            // padding bytes take part in the comparison
    (nd.push(static_cast<typename std::decay<KA>::type>(a)), ...);
    if (!nd.fn) rec->overflow = true;
}
#define GSWT_LAUNCH(K, G, B, S, ...)                                                                     \
    do {                                                                                                 \
        if (GraphRec* rec_ = graph_recorder()) graph_record(rec_, K, G, B, __VA_ARGS__);                 \
        else hipLaunchKernelGGL(K, G, B, 0, S, __VA_ARGS__);                                             \
    } while (0)

// A launch that carries its own pair of timing events (E0, E1 non-null, no graph recorder): hipExtLaunchKernelGGL binds both to the DISPATCH,
// so hipEventElapsedTime(E0, E1) is the kernel's own begin -> end on the device -- the interval rocprofv3 --kernel-trace reports -- rather than
// "previous command of the stream done -> this kernel done" of two hipEventRecord calls (GSWT_KERNEL_EVENTS=0).  Measured at the end of round 4
// (profiles/r04_kernel_events.txt): the two read alike (c3 fly path, k_composite 0.104-0.106 against 0.100-0.114 ms, frame rate unchanged), and
// under rocprofv3 either agrees with the profiler's own average of the same run (0.0907 / 0.0919 against 0.0909 / 0.0969 ms): what separates the
// bench line's kernel time (0.105 ms) from a rocprofv3 summary (0.089-0.097) is the run -- under the profiler fewer frames overlap (4 090-4 750
// against 5 450 frames/s) and the kernel shares the chip with less -- not the events.
bool kernel_events_enabled();
#define GSWT_LAUNCH_TIMED(K, G, B, S, E0, E1, ...)                                                       \
    do {                                                                                                 \
        if ((E0) && (E1) && !graph_recorder() && kernel_events_enabled())                                \
            hipExtLaunchKernelGGL(K, G, B, 0, S, E0, E1, 0, __VA_ARGS__);                                \
        else {                                                                                           \
            if (E0) hipEventRecord(E0, S);                                                               \
            GSWT_LAUNCH(K, G, B, S, __VA_ARGS__);                                                        \
            if (E1) hipEventRecord(E1, S);                                                               \
        }                                                                                                \
    } while (0)

// ---- host side: what one frame's kernels read and write (gswt_api.hip: plan_frame_buffers) ------------------------------------------
// The layouts of the bookkeeping regions (counters, super_sums, live_cnt, radix_*, ranges) are gswt_frame_layout.h's.
struct FrameBufs {
    // inputs: the frame's draw set, the scene, the caller's images (bg_rgba / bg_depth null: none) and the slot's pinned result words
    const DrawDev* draws;
    const uint2 *chunk_tab, *chunk_tab_xcd;    // slot order; k_project's launch order
    const uint32_t *static_list, *merged_list, *merged_map;
    const uint4* tex;
    const float *hmap, *boxes;                 // boxes: tile-local bounds of every chunk of the static lists (k_cull's chunk cull)
    // gswt_set_tile_styles' table as the frame was submitted with it, per map cell (tint r | g << 8 | b << 16 | tint_strength << 24, dim);
    // null: styles off (k_project<.., STY = false>)
    const uint2* styles; uint32_t n_styles;
    // gswt_set_shadow_map's block and image version as the frame was submitted with them; shadow.z null: shadows off (k_project<.., SHD = false>)
    Shadow shadow;
    // gswt_set_clip_volumes' set as the frame was submitted with it; n = 0: off (k_project<.., CLIP = false>)
    ClipSet clip;
    const float4* bg_rgba; const float* bg_depth; float4* out;
    float* out_depth;                          // the frame's depth image (f32, the colour's geometry); null: none (gswt_render_depth)
    uint4* out_pick;                           // the frame's pick image (gswt_pick records, the colour's geometry); null: none (gswt_render_pick)
    FrameResult* host_counters;                // as the device sees them (null: copied behind the frame)
    // the sizes the buffers were planned for
    uint32_t n_chunks, n_cells, n_tiles, pair_cap, seg;
    // per slot (= composite order), per draw, per map cell (the band cull), per chunk
    uint2* rects; Rec* recs; float4* col_f; Varyings* dbg;
    float* depths;                             // null unless the frame is depth-tested, depth-ordered or writes its depth or pick image
    uint32_t *draw_culled, *cell_culled, *live_cnt, *live_cid, *block_sums; uint4* live_tab;
    // the `ghist` region: the counter block, k_project's super-group sums (SuperSums of n_chunks), the two sorts' radix workspaces (RadixWs)
    uint32_t* ghist;                           // the region's first word: where k_cull's clear of n_zero_head words starts
    FrameCounters* counters;
    uint32_t* krange() const { return counters->krange; }      // the depth key range (k_emit<DEPTH>); address arithmetic on a device pointer
    uint32_t *super_sums, *radix_pair, *radix_depth;
    // per pair: tile keys, slots, and the depth order's tile ids / depth bits
    uint32_t *keys_a, *keys_b, *vals_a, *vals_b, *aux_a, *aux_b;
    // the `ranges` region: per tile (~start, end), the tile-local depth sort's lists of long tiles
    uint2* ranges; uint32_t* long_tiles;
    uint32_t* item_base; uint4* item_tab; float4* partials;
    float* partials_z;                         // a segment's partial depth per pixel beside `partials` (out_depth only)
    uint2* partials_pick;                      // a segment's (largest weight, its pair) per pixel beside `partials` (out_pick only)
    hipEvent_t ev_pick_begin, ev_pick_end;     // GSWT_OPT_TIMING: the events k_pick_resolve's launch carries (null: none)
    // the words k_cull clears: the head of `ghist` to the end of the pair sort's zeroed part, the `ranges` region, the depth sort's zeroed part
    uint32_t n_zero_head, n_zero_ranges, n_zero_depth;
};

// ---- launch wrappers (gswt_kernels.hip, gswt_passes.hip) ------------------------------------------------------------------------------
void launch_chunk_tabs(hipStream_t s, const DrawDev* draws, const uint32_t* xcd_first, uint32_t n_draws, uint2* chunk_tab, uint2* chunk_tab_xcd,
                       const uint64_t per_xcd[8], uint64_t longest);
void launch_merge_build(hipStream_t s, const MergeSeg* segs, uint32_t n_segs, const uint2* blocks, uint32_t n_blocks, MergeGroup* groups, uint32_t n_groups,
                        const int32_t* raw, uint32_t n_total, const SortCount* n_total_dev, uint32_t* ka, uint32_t* va,
                        uint32_t* kb, uint32_t* vb, uint32_t* radix_ws, int group_bits, uint32_t* merged_list, uint32_t* merged_map);
// Base lists of one presort view: the k_mg_* keys of gswt_upload_scene_rows' groups (one per (lod, tile)) and the stable radix sort;
// returns launch_sort's 0 / 1 (sorted keys / vals in ka, va or kb, vb).  Arguments as launch_merge_build.
int launch_scene_sort(hipStream_t s, const MergeSeg* segs, const uint2* blocks, uint32_t n_blocks, MergeGroup* groups, const int32_t* raw,
                      uint32_t n_total, const SortCount* n_total_dev, uint32_t* ka, uint32_t* va, uint32_t* kb, uint32_t* vb,
                      uint32_t* radix_ws, int group_bits);
// gswt_scene.hip.  bounds: 8 words, {INT_MAX x3, INT_MIN x3, 0, 0} on entry (k_scene_tex).
void launch_scene_tex(hipStream_t s, const uint4* rows, uint32_t n, uint4* tex, int32_t* bounds);
void launch_scene_raw(hipStream_t s, const uint4* rows, uint32_t n, const uint32_t* moff, const uint32_t* cnt, uint32_t n_lt, const SceneViews& vps,
                      int32_t* raw);
void launch_scene_scatter(hipStream_t s, const MergeSeg* segs, uint32_t n_segs, const MergeGroup* groups, const uint32_t* sorted_keys,
                          const uint32_t* sorted_vals, uint32_t n_total, uint32_t* arena, uint32_t arena_n);
void launch_scene_self(hipStream_t s, const SceneList* lists, uint32_t n_lists, uint32_t lists_per_lod, uint32_t* arena);
void launch_scene_boxes(hipStream_t s, const SceneList* lists, uint32_t n_lists, uint32_t n_boxes, const uint32_t* arena, const uint4* tex,
                        uint32_t n_splats, float* boxes);
void launch_merge_copy(hipStream_t s, const MergeCopy* jobs, const uint2* blocks, uint32_t n_blocks, const uint2* remap, const MergeSources& src,
                       uint32_t* new_list, uint32_t* new_map);

// The frame: k_cull (+ the clears of b.n_zero_*), k_project + k_totals over the first n_launch positions of the launch table, k_emit
// (keys -> `keys`, slots -> b.vals_a; depth-ordered frames also the depth bits -> dkeys and, with krange, the frame's key range; n_launch 0:
// over every chunk instead of the live table), k_items + the compositor over the sorted slots `vals`.
void launch_cull(hipStream_t s, const Frame& f, const FrameBufs& b, bool chunk_cull);
// (m: the instantiation's mode bits, project_modes of gswt_frame_modes.h)
void launch_project(hipStream_t s, const Frame& f, const FrameBufs& b, uint32_t n_launch, bool debug, ProjectModes m);
void launch_emit(hipStream_t s, const Frame& f, const FrameBufs& b, uint32_t* keys, uint32_t* dkeys, uint32_t* krange, uint32_t n_launch);
// b.out receives the image in out_format (kOut*; the 8-bit formats store one u32 per pixel through the float4 pointer, the video formats
// their planes of out_rows x f.out_w samples, both even), b.out_depth (when set) the depth image in f32, b.out_pick (when set) the pick image
// (gswt_pick records; then `vals` is also what k_pick_resolve reads behind the compositor).
void launch_composite(hipStream_t s, const Frame& f, const FrameBufs& b, const uint32_t* vals, int out_rows, const uint32_t* krange,
                      uint32_t depth_passes, bool report_max, hipEvent_t ev_begin, hipEvent_t ev_end, int out_format);
void launch_totals(hipStream_t s, uint32_t* super_sums, SuperSums ss, FrameCounters* counters, uint32_t pair_cap);

// LSD radix sort of (keys, vals) on key bits [0, key_bits), ping-pong between the a and b buffers; returns 0 if the result is in a, 1 if in b.
// The item count is read on the device (count: a SortCount record, a frame's own through sort_count_of), grids are sized for n_cap.  ws: the
// RadixWs of (n_cap, key_bits) in gswt_frame_layout.h -- radix_ws_words words whose first radix_ws_zero_words are zero on entry.  ranges
// (zero on entry): the last pass also writes every key's range words (encode_tile_range);
// krange: the key range the passes cover (depth keys); aux: a payload carried with the vals.  threads_override (256 / 512) and
// aux_override (1 / 2) replace the workgroup width and payload form the capacity selects (0: they stand; gswt_debug_sort_ex).
inline size_t radix_ws_words(uint32_t n_cap, int key_bits) { return radix_ws_of(n_cap, key_bits).words(); }
inline size_t radix_ws_zero_words(uint32_t n_cap, int key_bits) { return radix_ws_of(n_cap, key_bits).zero_words(); }
int launch_sort(hipStream_t s, uint32_t* keys_a, uint32_t* vals_a, uint32_t* keys_b, uint32_t* vals_b, uint32_t n_cap,
                const SortCount* count, int key_bits, uint32_t* ws, uint2* ranges = nullptr, const uint32_t* krange = nullptr,
                uint32_t* aux_a = nullptr, uint32_t* aux_b = nullptr, int threads_override = 0, int aux_override = 0);

// GSWT_ORDER_DEPTH, tile-local path: depth-sorts every tile's slice of the tile-sorted list in place.  long_list: two lists of tiles, each
// tile_depth_list_words(n_tiles) words ([0] count, [1 .. n_tiles] tiles), back to back; both counts zero on entry.
void launch_tile_depth_sort(hipStream_t s, const uint2* ranges, uint32_t* vals, uint32_t* dkeys, uint32_t* vals_scratch, uint32_t* dkeys_scratch, int n_tiles,
                            uint32_t* long_list, FrameCounters* counters);
inline size_t tile_depth_list_words(size_t n_tiles) { return n_tiles + 1; }
uint32_t tile_depth_sort_cap();

// out_format: kOut* (16- or 4-byte pixels, or the video planes, reassembled plane by plane: width, height, rows_padded, band_px even)
void launch_unshard(hipStream_t s, const void* gathered, void* out, int width, int height, int shard_count, int rows_padded, int band_px,
                    int out_format);
void launch_skybox(hipStream_t s, const float* view16, float p00, float p11, int width, int height, int face_size, int equirect,
                   const float4* faces, float4* out);
void launch_skybox_bake(hipStream_t s, const SkyBakeArgs& a, const float4* equi, float4* faces);
// The proxy passes, k_proxy / k_proxy_sphere<FOG, ORTHO, SHD, CLIP>.  ortho: the pass reads a's ortho_* fields (gswt_proxy_render_ortho: set up in
// the grid frame; gswt_proxy_render_sphere: with g = 0); shd.z set: it shades the ground by gswt_set_shadow_map's image; clip.n > 0: it
// discards the fragments gswt_set_clip_volumes' GROUND volumes hide (clip: clip_ground_subset of the set in force).
void launch_proxy(hipStream_t s, const ProxyArgs& a, bool ortho, const Shadow& shd, const ClipSet& clip, const float* hm, const float4* tex,
                  float4* rgba, float* depth);
void launch_proxy_sphere(hipStream_t s, const ProxyArgs& a, const SphereProxyArgs& sp, bool ortho, const Shadow& shd, const ClipSet& clip,
                         const float4* tex, float4* rgba, float* depth);
// One level of the proxy mip build into dst (n x n float4).  src: the staged source, a.pitch bytes per row.  ranges: 2 n int2,
// wv / wh: the tap weights, tmp: the intermediate, part: the partial sums (sizes: proxy_mip_* above; unused on a copy level).
void launch_proxy_mip(hipStream_t s, const ProxyMipArgs& a, const uint8_t* src, int2* ranges, float* wv, float* wh, float4* tmp,
                      float4* part, float4* dst);
void launch_fill_f32(hipStream_t s, float* p, size_t n, float v);

}  // namespace gswt
