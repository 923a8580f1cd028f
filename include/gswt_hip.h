/*
 * gswt_hip.h -- C ABI of libgswt_hip.so, the MI355X-native drop-in for the GPU half
 * of the GSWT hot path: per-frame Wang-tile instancing, Gaussian projection,
 * ordering, 16x16 screen-tile binning and alpha compositing.
 *
 * Each entry point names the reference interface it replaces (file:line are into
 * zengyf131/gswt_renderer).  Plain pointers and sizes only; no C++/torch types.
 * INTEGRATION.md shows the Rust `extern "C"` block a maintainer would add.
 *
 * Threading (mirrors renderer.rs: render runs on the main thread only): a ctx is
 * single-owner, one caller thread at a time.  A ctx owns one HIP stream; all work
 * of a call is enqueued on it.  Every host pointer is borrowed for the duration of
 * the call only.  No call aborts or throws across the ABI: all return an int status
 * and gswt_last_error() holds the text of the last failure on that ctx.
 */
#ifndef GSWT_HIP_H
#define GSWT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSWT_API __attribute__((visibility("default")))

typedef struct gswt_ctx gswt_ctx;

enum {
    GSWT_OK = 0,
    GSWT_ERR_BAD_ARG = -1,   /* reference: assert!/unwrap panic on malformed input      */
    GSWT_ERR_CAPACITY = -2,  /* reference: silent wgpu validation error past 20 000 draws
                                / 10 M merged splats (renderer.rs:253,273); here buffers
                                grow on demand, this code only reports a failed grow     */
    GSWT_ERR_HIP = -3,       /* any HIP runtime error                                    */
    GSWT_ERR_STATE = -4,     /* call order violated (e.g. render before upload_scene)    */
    /* -5 is GSWT_ERR_IO of gswt_host.h */
    GSWT_ERR_RCCL = -6       /* RCCL missing / a collective failed (text in gswt_last_error) */
};

/* Composite order.  REFERENCE reproduces the reference's order exactly: draw rank
 * (back-to-front tile list, wangtile.rs:489-499) x position in that draw's presorted
 * list (scene.rs:685-695).  DEPTH is a true per-splat global depth sort. */
enum { GSWT_ORDER_REFERENCE = 0, GSWT_ORDER_DEPTH = 1 };

/* ---- byte-exact mirrors of the reference's uniform blocks ------------------------ */

/* CameraUniforms, camera.rs:158-167 / gswt.wgsl:437-444 (176 bytes) */
typedef struct {
    float projection[16]; /* column-major */
    float view[16];
    float focal[2];
    float viewport[2];
    float htan_fov[4];
    float cam_pos[4];
} gswt_camera_uniforms;

/* SceneUniforms, renderer.rs:602-622 / gswt.wgsl:446-463 (160 bytes) */
typedef struct {
    float splat_scale;
    float tile_width;
    uint32_t use_clip;
    float clip_height;
    uint32_t surface_type; /* 0 None, 1 HeightMap, 2 Sphere (structure.rs:435-440) */
    float sphere_radius;
    float point_cloud_radius;
    float transition_width_ratio;
    uint32_t num_lod;
    uint32_t draw_mode;
    uint32_t map_half_wh[2];
    int32_t center_coord[2];
    uint32_t _pad0[2];
    float transition_dist_vec[16];
    float height_map_scale[4];
    float scene_scale[4];
} gswt_scene_uniforms;

/* TileUniforms, renderer.rs:675-689 / gswt.wgsl:465-476 (80 bytes) */
typedef struct {
    uint32_t single_draw;
    uint32_t map_index;
    int32_t single_lod_id;
    int32_t valid_lod_id;
    uint32_t changing;
    int32_t changing_to_lower;
    uint32_t _pad0[2];
    uint32_t tile_id[4]; /* lod, tile, view, 0 */
    float offset[4];
    uint32_t map_coord[4];
} gswt_tile_uniforms;

/* One static presorted list of PreloadData.tile_base_data[lod][tile][view]
 * (structure.rs:546-554: gs_index + gs_lod_id, splat_count entries each). */
typedef struct {
    const uint32_t *gs_index;
    const uint32_t *gs_lod_id;
    uint32_t splat_count;
    uint32_t _pad;
} gswt_base_list;

/* One iteration of the draw loop in GSWTRenderer::render (renderer.rs:466-591):
 * the tile uniforms written at :499-515 plus which instance buffers get bound. */
typedef struct {
    gswt_tile_uniforms tile;
    /* list selection, renderer.rs:517-579 */
    uint32_t merged;        /* 1: merged group (Some(render_data_value)) -> range of the
                               merged arrays passed to gswt_set_draws; 0: static base list */
    uint32_t base_lod;      /* static list [base_lod][base_tile][base_view]; the caller   */
    uint32_t base_tile;     /* applies renderer.rs:564-572 (Changing(false) -> lod-1)     */
    uint32_t base_view;
    uint32_t merged_offset; /* first element of this draw in the merged arrays            */
    uint32_t merged_count;  /* render_data_value.splat_count                              */
    uint32_t merged_has_lod;/* 1 iff single_lod_id == -1 (gs_lod_id uploaded, :544-556)   */
    /* CPU viewport culling inputs, renderer.rs:472-494 (non-merged draws only) */
    uint32_t cull_enable;   /* 1 iff render_data_key.tid.len() == 1                        */
    float corners[12];      /* tile_instance.corner_data[ci].0, ci = 0..3                  */
    uint32_t lod;           /* tid.0, index into lod_enable (renderer.rs:495)              */
    uint32_t merged_group;  /* gswt_set_draws_merge_groups only: index of this draw's group        */
    uint32_t _pad[2];
} gswt_draw;

/* The parts of RenderConfig (structure.rs:346-388) read on the hot path. */
typedef struct {
    float culling_dist;       /* render_config.culling_dist, renderer.rs:490 */
    uint32_t lod_enable_mask; /* bit l = render_config.lod_enable[l], renderer.rs:495.  A draw is kept iff bit
                                 (gswt_draw.lod & 31) is set: gswt_draw.lod is tid.0 -- of a blending draw the tile's own LOD,
                                 not base_lod; of a merged draw its head's -- and a lod of 32 or more wraps (32 reads bit 0),
                                 where the reference would index past lod_enable and panic */
    int32_t order_mode;       /* GSWT_ORDER_* */
    float transmittance_eps;  /* front-to-back early-out threshold; 0 = never stop early */
    /* screen-tile sharding for multi-GPU; shard_count <= 1 renders the whole frame.
       GSWT_SHARD_ROWS: this ctx composites only the 16-px tile rows with (row % shard_count) == shard_index and writes
         them compacted, in row order (gswt_shard_rows_padded rows x W).  Every rank projects every splat.
       GSWT_SHARD_COLUMNS: this ctx composites the contiguous band of ceil(tiles_x / shard_count) tile columns number
         shard_index (H rows x gswt_shard_cols_padded pixels) and, on the plain surface, skips the draws none of whose
         splats can reach the band -- projection is sharded too.  Pair counts are even across column bands for a
         horizon-dominated view, across contiguous row bands they are not. */
    int32_t shard_index;
    int32_t shard_count;
    int32_t shard_mode;       /* GSWT_SHARD_* */
    uint32_t out_format;      /* GSWT_OUT_* or GSWT_VIDEO_*; 0 (a zero-initialised config) is the RGBA f32 image */
} gswt_render_config;

enum { GSWT_SHARD_ROWS = 0, GSWT_SHARD_COLUMNS = 1 };

/* Output image formats (gswt_render_config.out_format).  GSWT_OUT_RGBA32F: 16 bytes per pixel, premultiplied colour and alpha as
 * four floats.  The 8-bit formats are the layouts of the reference's non-sRGB swapchain surface (state.rs:96-101: Rgba8Unorm /
 * Bgra8Unorm), 4 bytes per pixel, written by the compositor's own store.  Each byte is q(x) of the float x the same frame writes in
 * GSWT_OUT_RGBA32F:
 *     q(x) = (uint8) round_half_even(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f)      (one binary32 product, not fused; NaN -> 0)
 * so an 8-bit frame equals q of its f32 frame bit for bit, in every mode and compositor variant.  No gamma step (the surface is not
 * sRGB).  This is NOT the reference's own 8-bit result: its blend state rounds the 8-bit target after every blended splat.
 * For the 8-bit formats every `float *` output pointer of gswt_render / gswt_render_async / the gathers addresses
 * rows_out x out_w x 4 BYTES (pass the byte buffer cast to float *); shard geometry (gswt_shard_rows_padded,
 * gswt_shard_cols_padded) counts pixels and does not change. */
enum { GSWT_OUT_RGBA32F = 0, GSWT_OUT_RGBA8_UNORM = 1 /* bytes R, G, B, A */, GSWT_OUT_BGRA8_UNORM = 2 /* bytes B, G, R, A */ };

/* 4:2:0 video frames (gswt_render_config.out_format, accepted wherever an output format is): what a video encoder reads, BT.709,
 * limited ("video") range, 12 bits per pixel, written by the compositor's own store (nothing in the reference corresponds to them).
 * width and height must be even (GSWT_ERR_BAD_ARG before anything is enqueued otherwise).  The output pointer addresses the planes
 * back to back without padding, rows_out * out_w * 3 / 2 bytes (gswt_out_image_bytes); a shard's buffer is itself a complete small
 * image of out_w x rows_out (both multiples of 16), its padding rows / columns zero bytes in every plane.
 * A video frame is a pure function of the GSWT_OUT_RGBA32F pixels o the same call would write (alpha is dropped), every operation
 * one binary32 operation, not fused:
 *     c   = fminf(fmaxf(o.c, 0), 1)                      for c = r, g, b   (NaN -> 0, as q() above)
 *     yl  = (0.2126f * r + 0.7152f * g) + 0.0722f * b    BT.709 luma, left to right
 *     Y   = (uint8) round_half_even(16.0f + 219.0f * yl)                    16..235
 *     cb  = (b - yl) * fl(1 / 1.8556),   cr = (r - yl) * fl(1 / 1.5748)     per pixel, in [-0.5, 0.5]; fl = the double quotient rounded to binary32
 *     per 2x2 block (x, y even):  m = ((c00 + c01) + (c10 + c11)) * 0.25f   c00 top left, c01 top right, c10 bottom left
 *     Cb  = (uint8) round_half_even(128.0f + 224.0f * m_cb),  Cr likewise   16..240
 * Chroma is the plain mean of the block's four samples, i.e. sited at the block's centre (as JPEG / MPEG-1, not the co-sited-left
 * convention of MPEG-2 / H.264's default).  So a video frame equals this function of its f32 frame byte for byte, in every mode and
 * compositor variant.  The depth image of gswt_render_depth stays rows_out x out_w f32. */
enum {
    GSWT_VIDEO_NV12 = 16,  /* plane Y (rows x out_w bytes), then ONE plane of interleaved Cb, Cr pairs (rows/2 x out_w bytes) */
    GSWT_VIDEO_I420 = 17   /* plane Y, then plane Cb (rows/2 x out_w/2 bytes), then plane Cr (the same size) */
};
/* Bytes of a rows x out_w image in any output format (16 / 4 bytes per pixel, or the planes above); 0 for an unknown format, a
 * negative size or odd video dimensions.  The library sizes its own copies, clears and gathers with it. */
GSWT_API size_t gswt_out_image_bytes(int out_format, int rows, int out_w);

/* Per-stage device times of the last gswt_render (hipEvent, ms) and workload sizes.  ms_ranges is ~0 since the per-tile
 * [start, end) table is left by the last pass of the pair sort (its time is inside ms_sort); ms_scan is unused (no scan launch). */
typedef struct {
    float ms_project, ms_scan, ms_emit, ms_sort, ms_ranges, ms_composite, ms_total;
    uint32_t n_draws;
    uint64_t n_instanced; /* N: list entries iterated             */
    uint64_t n_visible;   /* survivors of the vertex stage        */
    uint64_t n_pairs;     /* P: (splat, 16x16 screen tile) pairs  */
    uint32_t n_tiles;     /* screen tiles composited by this ctx  */
    uint32_t _pad;
    float ms_composite_kernel; /* k_composite alone (ms_composite also covers work-item setup + k_combine) */
    float ms_pick_resolve;     /* k_pick_resolve alone (part of ms_composite; 0 on a frame without a pick image) */
} gswt_timings;

/* ---- lifecycle ------------------------------------------------------------------- */

/* wgpu adapter/device acquisition in State::new (state.rs:56-92). */
GSWT_API int gswt_create(int device_id, gswt_ctx **out);
GSWT_API void gswt_destroy(gswt_ctx *ctx);
GSWT_API const char *gswt_last_error(const gswt_ctx *ctx);
/* Runs on a user-provided HIP stream (hipStream_t as void*) instead of the ctx's own; NULL returns to a stream of the ctx's own. */
GSWT_API int gswt_set_stream(gswt_ctx *ctx, void *hip_stream);

/* Options (no reference counterpart; test / profiling switches).
 * NO_LOD_PREFILTER: a plain tile iterates the interleaved LOD l / l+1 base list exactly as the
 *   reference binds it (renderer.rs:571-578) instead of the pre-filtered own-LOD list; results
 *   are identical (gswt.wgsl:38-42 discards the other LOD), only the entry count differs.
 * DEBUG_VARYINGS: keep vs_main's per-entry outputs for gswt_debug_read_projected. */
enum { GSWT_OPT_NO_LOD_PREFILTER = 1, GSWT_OPT_DEBUG_VARYINGS = 2,
       GSWT_OPT_SEGMENT = 3 /* pairs per compositor work item, multiple of 256 (default 1536; dense scenes with the early-out on
                               gain from up to 4096: a segment cannot skip what the segments in front of it already saturated) */,
       GSWT_OPT_DEBUG_FLAGS = 4 /* reserved: 0 is accepted, any other value returns GSWT_ERR_BAD_ARG */,
       GSWT_OPT_TIMING = 5 /* hipEvent timing: 0 none, 1 frame + k_composite, 2 every stage (default) */,
       GSWT_OPT_PAIR_CAP = 6 /* test hook: pin the pair-buffer capacity to `value` pairs until a frame overflows it (0: automatic) */,
       GSWT_OPT_NO_MERGE_REUSE = 7 /* gswt_set_draws_merge_groups re-sorts every merged group at every sort event instead of copying
                                      the groups that did not change since the previous one (results are identical) */,
       GSWT_OPT_DEFER_SWAP = 8 /* 1: a gswt_set_draws* call takes effect with the first frame submitted AFTER its uploads and device-side
                                  list builds have finished (frames submitted meanwhile keep the previous draw list and nothing waits);
                                  n >= 2: with the n-th frame submitted after the call, finished or not (deterministic: for ranks that
                                  render shards of the same frames); 0 (default): with the next frame, which then waits for them on
                                  the device */,
       GSWT_OPT_GRAPH = 9 /* 1: a frame's kernel launches are replayed as ONE hipGraphLaunch per frame slot (a chain of kernel nodes;
                             only the nodes whose grid or arguments changed since the slot's previous frame are updated in the
                             executable graph) instead of ~13 separate launches: less submitting-thread time per frame, same
                             kernels, same results.  Frames with GSWT_OPT_TIMING > 0 or debug varyings
                             launch as before.  0 (default): separate launches */,
       GSWT_OPT_STRICT_VS = 10 /* 1 (default): the vertex stage evaluates gswt.wgsl:152-258,260-265,402-419 operator by operator -- one correctly
                                  rounded binary32 operation per written `*` `+` `-` `/`, full matrix products, no fused multiply-add; per
                                  splat bit-identical to the CPU checker's restatement of the shader text.  0: the rounding sequence "v2"
                                  (fma chains, one reciprocal per quotient: also legal WGSL, ~25 % fewer instructions, the default until
                                  round 3); the two differ by up to 5e-4 in the image on thin ellipses */,
       GSWT_OPT_DEPTH_PASSES = 12 /* test hook: 8-bit radix passes on the depth bits the next GSWT_ORDER_DEPTH frame launches (1..4; default 3,
                                     then as many as the depth ranges of the recent frames needed); a frame whose visible depths span more
                                     bits is flagged on the device and re-run with more, like a pair-buffer overflow */,
       GSWT_OPT_COMPOSITE = 13 /* no effect: there is one compositor, k_composite (256-pair batches staged by the whole workgroup, two barriers
                                  per batch) + k_combine.  1 (once the four waves of a work item decoupled) and 2 (once a compositor that folded
                                  the segments itself instead of launching k_combine) are accepted and run the default compositor; 3 and above
                                  are refused */,
       GSWT_OPT_DEPTH_SORT = 14 /* how GSWT_ORDER_DEPTH orders the pairs: 0 (default) / 2 = tile passes first (depth bits as payload), then every
                                   screen tile's slice is depth-sorted by one wave / workgroup (k_tile_depth_sort: inside LDS up to 16 384 pairs,
                                   through global memory beyond); 1 = global radix passes on the depth bits in front of the tile passes.
                                   Same image bit for bit */,
       GSWT_OPT_NO_CHUNK_CULL = 15 /* 1: the per-chunk frustum cull in front of the projection is off (every 256-entry chunk of a draw that
                                      survives the reference's tile cull is projected, as until round 3).  Same image bit for bit: the cull
                                      only leaves out chunks none of whose splats vs_main's own frustum test (gswt.wgsl:163-167) would keep */,
       GSWT_OPT_ITEM_ORDER = 16 /* no effect: the compositor's work items (screen tile, segment of its pair list) are handed out in tile order.
                                  1 (once heaviest first) is accepted and runs the default tile order */,
       GSWT_OPT_PROJECTION = 17 /* 0 (default): perspective, vs_main as written.  1: orthographic -- top-down maps, minimaps, sun-direction depth
                                   maps, height fields.  The vertex stage is vs_main except gswt.wgsl:213-232: the perspective Jacobian (focal / t.z,
                                   the 1.3 * htan_fov clamp, -focal t / t.z^2) is replaced by the constant affine one, J_T columns (fx, 0, 0),
                                   (0, fy, 0), (0, 0, 0); T = transpose(view3) * J_T and cov2d = transpose(T) * Vrk * T stay the written full
                                   products, operator by operator as GSWT_OPT_STRICT_VS.  For these frames `projection` is an affine matrix
                                   (bottom row exactly (0, 0, 0, 1), OpenGL depth convention like the perspective one), `focal` is PIXELS PER WORLD
                                   UNIT, |0.5 P[0][0] W| and |0.5 P[1][1] H|, htan_fov is ignored, and cam_pos is only the reference point of the
                                   LOD transition (gswt.wgsl:91-150: cam_dist = distance(center, cam_pos)) -- e.g. the main view's eye.  The
                                   frustum test (1.2 w with w = 1: a 1.2x box in NDC), surface mapping, clip test, eigen-decomposition, colour and
                                   depth (q.z / q.w of opengl_to_wgpu * projection, here LINEAR in view depth) are the same code; depth, pick,
                                   every output format, both order modes, row shards, GSWT_OPT_GRAPH and frames in flight work unchanged.
                                   Read when a frame is submitted (gswt_render*, gswt_render_async*, depth and pick forms): setting it waits for
                                   nothing, frames in flight and a frame re-run after a pair-buffer overflow keep the projection they were
                                   submitted with.  With the option on a submit returns GSWT_ERR_BAD_ARG before anything is enqueued for: a
                                   projection whose bottom row is not (0, 0, 0, 1); a focal component that is not finite or <= 0;
                                   GSWT_OPT_STRICT_VS = 0 (sequence v2 has no orthographic form); GSWT_SHARD_COLUMNS with shard_count > 1 (the
                                   band cull is perspective-specific).  Any value other than 0 / 1 is refused.  gswt_skybox_render remains
                                   perspective-only (a straight-down map never sees the sky); the ground under an orthographic frame comes from
                                   gswt_proxy_render_ortho, an entry point of its own that does not read this option, and the frame takes its
                                   outputs as bg_rgba / bg_depth like any others.  Order: the worker's tile order is by distance from the sort event's camera, so a top-down view that
                                   shares the main view's draw set should use GSWT_ORDER_DEPTH, which is exact per splat; GSWT_ORDER_REFERENCE
                                   also runs and is well defined (draw rank x list position).  The CPU oracle has no orthographic mode */,
       GSWT_OPT_ANTIALIAS = 18 /* anti-aliased splats: a screen-space low-pass with opacity compensation.  `value` is the variance of an
                                  isotropic Gaussian pixel filter in 1/1024 px^2 OF THE SCREEN: 0 (default) off, 1..4096 on, anything else
                                  refused (GSWT_ERR_BAD_ARG).  v = value / 1024 is exact in binary32; 307 is about 0.3 px^2, the usual 3DGS
                                  constant, 102 about 0.1 px^2, the Mip-Splatting one.  vs_main has no such filter (gswt.wgsl:245-258: cov2d
                                  goes straight into the eigen-decomposition), so with the option off a splat whose footprint is below a
                                  pixel is drawn at full opacity or not at all, depending on where its centre falls between pixel centres.
                                  Why s = 4 v / splat_scale^2: the fragment stage weights a pixel at offset x = 0.5 splat_scale (p.x major +
                                  p.y minor) by exp(-|p|^2) with major = sqrt(2 lambda1) e, so a splat's on-screen Gaussian has covariance
                                  (splat_scale^2 / 4) cov2d; convolving it with the pixel filter adds v I on screen, i.e. s I on cov2d.  The
                                  host computes s once per frame in binary32 as (4.0f * v) / (splat_scale * splat_scale).
                                  Vertex stage: the strict sequence is unchanged up to and including `if (l2 < 0) discard` -- the rejection
                                  is decided on the unfiltered l2 and the direction (ex, ey) comes from the unfiltered c01, l1 - c00 (adding
                                  s I does not change eigenvectors).  Then, one binary32 operation per written operator, nothing fused:
                                      l1f = l1 + s;  l2f = l2 + s;
                                      smaj = fminf(sqrtf(2.0f * l1f), 1024.0f);   smin = fminf(sqrtf(2.0f * l2f), 1024.0f);
                                      comp = clamp(sqrtf(l1 / l1f) * sqrtf(l2 / l2f), 0.0f, 1.0f);      a NaN gives 0
                                  major / minor are built from smaj, smin, ex, ey as before, and alpha = alpha * comp goes after the
                                  LOD-transition product and before the near fade.  comp keeps the splat's integrated opacity: alpha'
                                  sqrt(l1f l2f) = alpha sqrt(l1 l2).  Everything downstream reads the stored axes and alpha and follows
                                  without change: the pair rectangle and the compositor's |p|^2 <= 4, depth and pick weights, every output
                                  format, both order modes, shards (the column-band cull bounds a splat's reach with lambda + s),
                                  GSWT_OPT_PROJECTION = 1, the surface mappings, the point-cloud radius and the debug draw modes (the filter
                                  sits after cov2d in all of them).  gswt_debug_read_projected reports the filtered axes and the compensated
                                  alpha.  The visible set can only grow: a splat with l2 == 0, or whose |minor|^2 underflowed in the fragment
                                  setup, was invisible and is now drawn.  Read when a frame is submitted, like GSWT_OPT_PROJECTION: setting
                                  it waits for nothing; frames in flight and a frame re-run after a pair-buffer overflow keep the value they
                                  were submitted with.  With value > 0 a submit returns GSWT_ERR_BAD_ARG before anything is enqueued for
                                  GSWT_OPT_STRICT_VS = 0 (sequence v2 has no filtered form) and for a splat_scale that is zero or not finite, or
                                  so large or small that s as computed above is not a finite positive number (|splat_scale| beyond about
                                  1.8e19, or below about 2e-19 at value 4096).
                                  Out of scope: the uncompensated "dilate only" variant; a filter for gswt_skybox_render / gswt_proxy_render;
                                  the CPU oracle, which has no filter */ };
GSWT_API int gswt_set_option(gswt_ctx *ctx, int key, int value);

/* ---- atmosphere: per-splat far fade and distance fog --------------------------------------------
 * The splat tiles of the unbounded terrain end at the tile cull (`culling_dist`, renderer.rs:472-494), which drops whole tile
 * instances: full-opacity tiles appear and vanish at the far edge as the camera moves.  The reference has no remedy (vs_main has
 * neither a fade nor a fog).  This block adds the two every terrain renderer ships, both per splat and both functions of the camera
 * distance A5 computes for the LOD transition:
 *   far fade : a splat's alpha ramps to zero between fade_start and fade_end, so that the splat layer dissolves into the proxy ground;
 *   fog      : a splat's colour goes toward fog_color with distance (aerial perspective), and so does the proxy ground under it.
 * NULL or an all-zero block: off, the default; a frame with the block off launches exactly the kernels it launches without this
 * call and is bit for bit the same frame.  A part is on when fade_end > 0 / fog_density > 0.
 *
 * Validation when a block is given: every field finite; fade_start = fade_end = 0 (no fade) or 0 <= fade_start < fade_end with
 * 1.0f / (fade_end - fade_start) finite; fog_density = 0 (no fog) or > 0; fog_start >= 0; fog_max in (0, 1] when fog_density > 0;
 * every fog_color component in [0, 1].  Anything else returns GSWT_ERR_BAD_ARG with the field named in gswt_last_error, and the
 * block in force stays.
 *
 * The block is copied into the frame when it is submitted (gswt_render*, gswt_render_async*, depth and pick forms), like
 * GSWT_OPT_ANTIALIAS: setting it waits for nothing, frames in flight and a frame re-run after a pair-buffer overflow keep the block
 * they were submitted with.  With either part on, a submit returns GSWT_ERR_BAD_ARG before anything is enqueued when
 * GSWT_OPT_STRICT_VS = 0 (sequence v2 has no atmospheric form).  The host derives fade_inv = 1.0f / (fade_end - fade_start) once
 * per frame in binary32.
 *
 * Vertex stage (strict sequence).  Every written operator is one correctly rounded binary32 operation, nothing fused:
 *     d = center - cam_pos;   dist = sqrtf((dx*dx + dy*dy) + dz*dz)
 * on the surface-mapped centre: A5's cam_dist expression, computed once, after the clip-height test, and reused by A5 when the draw
 * is changing.  For orthographic frames cam_pos is what it already is there, the reference point of the LOD transition: a minimap
 * fades and fogs around the main view's eye.
 *   Fade (fade_end > 0):
 *     t = clampf((fade_end - dist) * fade_inv, 0, 1)
 *     t == 0 discards the splat right there: it is not visible (not in n_visible) and makes no pairs, like A5's t_ratio discards.
 *     A NaN dist clamps to 0.  Otherwise
 *     fs = (t * t) * (3.0f - 2.0f * t);   alpha = alpha * fs
 *     with the product after the LOD-transition product and after the pixel filter's comp.  The smoothstep has no kink in
 *     brightness at either end of the ramp.
 *   Fog (fog_density > 0 and draw_mode == 0):
 *     x = fog_density * fmaxf(dist - fog_start, 0.0f)
 *     F = fog_max * (1.0f - e),   e = __expf(-x): the hardware exp2 of (-x) * log2(e), within 2 ulp of exp(-x) for x up to a few units
 *         and always within 1e-7 absolute (e <= 1 and x e^-x <= 0.37)
 *     per channel  c' = c * (1.0f - F) + fog_c * F
 *     byte' = (uint32_t)rintf(fminf(fmaxf(c', 0), 1) * 255.0f)
 *     and the record's colour word becomes byte'_r | byte'_g << 8 | byte'_b << 16 | (word & 0xFF000000).
 *     Re-quantising to the record's 8-bit colour is deliberate: the projected record stays 32 bytes, the compositor is untouched and
 *     every one of its forms stays available (early-out, depth test, depth and pick outputs).  The added
 *     error is at most half a code per splat, uncorrelated between splats.
 *   In the debug draw modes (draw_mode != 0) the colours stay the debug colours and only the fade applies.
 * gswt_debug_read_projected reports what the compositor will read: rgba[k] = (float)byte' / 255.0f for the three colours and the
 * faded alpha in rgba[3].
 * Untouched: pair rectangles, the tile / chunk / column-band culls (their bounds only have to hold without the atmosphere, which can
 * only remove splats), the sorts, the compositors and the pick resolve.  A chunk-level cull by fade_end is not part of this.
 *
 * Proxy pass.  gswt_proxy_render reads the block in force when it is called.  With the fog on, a pixel the proxy writes gets
 *     dist = best_t * sqrtf((d0*d0 + d1*d1) + d2*d2)      the ray's hit distance from cam_pos
 *     rgb' = rgb * (1.0f - F) + fog_color * F              the same F(dist), after `brightness`, alpha 1
 * The depth it writes, the pixels it does not write and the black_background output are unchanged.  The fade does not apply to the
 * proxy: it is what the splats fade into.  gswt_skybox_render is not fogged: pick fog_color near the sky's horizon colour, so that
 * the fogged ground meets the sky without a seam. */
typedef struct {
    float fade_start, fade_end;   /* world units from cam_pos.  Both 0: no fade.  Otherwise 0 <= fade_start < fade_end. */
    float fog_density;            /* per world unit.  0: no fog.  Otherwise > 0. */
    float fog_start;              /* >= 0: fog begins at this distance */
    float fog_max;                /* in (0, 1] when fog_density > 0: cap on the fog amount */
    float fog_color[3];           /* each in [0, 1] */
} gswt_atmosphere;                /* 32 bytes */
GSWT_API int gswt_set_atmosphere(gswt_ctx *ctx, const gswt_atmosphere *a);   /* NULL or an all-zero block: off (the default) */

/* ---- tile-instance styles: hide, dim and tint map cells per splat ---------------------------------
 * The pick image (gswt_render_pick) names the tile instance a pixel shows, its map_index.  This table lets the host act on it:
 * highlight the picked instance, ghost a tile, cut a hole into the splat layer, mark a region of a minimap -- also for a member of a
 * merged draw, which cannot be left out of the draw list on its own.  The reference has no per-instance appearance.
 *
 * Key.  The table is indexed by map cell: a splat's style is styles[id] with id the map_index the pick image reports for it --
 * gswt_tile_uniforms.map_index of a static draw, the member's map_index for an entry of a merged draw.  id >= n_styles reads as
 * neutral.  Map indices move with the map window at a build event; keeping a world cell styled across build events is the
 * caller's job (the Python layer does it: styles.TileStyles, GSWTPipeline.set_tile_styles).
 *
 * Off.  NULL, n_styles == 0 or a table whose entries are all neutral (tint_strength == 0 and dim == 0; the call scans it): styles
 * off, the default.  A frame with styles off launches exactly the kernels it launches without this call and is bit for bit the
 * same frame.
 *
 * Vertex stage (strict sequence).  Every written operator is one correctly rounded binary32 operation, nothing fused; s = styles[id]:
 *   Hide (s.dim == 255): the splat is discarded directly behind A1 (the valid_lod_id test), before its record is fetched: it is not
 *     visible (not in n_visible), makes no pairs and cannot appear in the colour, depth or pick image.
 *   Dim (0 < s.dim < 255):
 *     a_s = (float)(255 - s.dim) / 255.0f;   alpha = alpha * a_s
 *     with the product after the LOD-transition product, after the pixel filter's comp and after the far fade's fs.
 *   Tint (s.tint_strength > 0 and draw_mode == 0):
 *     k = (float)s.tint_strength / 255.0f;   tc = (float)s.tint[c] / 255.0f
 *     per channel  c_t = c * (1.0f - k) + tc * k      on the float colour of the record's bytes
 *     With the fog on, the fog's formula takes c_t in place of c.  The colour is re-quantised once, at the end, by the fog's own
 *     expression: byte' = (uint32_t)rintf(fminf(fmaxf(c', 0), 1) * 255.0f), and the record's colour word becomes
 *     byte'_r | byte'_g << 8 | byte'_b << 16 | (word & 0xFF000000).  At strength 255 the bytes are the tint's.
 *   The debug draw modes (draw_mode != 0) keep their colours; hide and dim still apply to them.
 *   A neutral entry of a table that is on leaves the splat's record bit-identical to the unstyled frame's.
 * gswt_debug_read_projected reports what the compositor will read: (float)byte' / 255.0f and the dimmed alpha.
 * Untouched: pair rectangles, the tile / chunk / column-band culls (styles only remove splats), the sorts, every compositor form, the
 * pick resolve, every output format, both order modes and both shard modes, GSWT_OPT_PROJECTION = 1, GSWT_OPT_ANTIALIAS and the
 * atmosphere.  The projected record stays 32 bytes.
 *
 * Lifetime.  The table is copied by the call (the host pointer is borrowed for the call only) into a device buffer of the library's:
 * one of a small pool of table versions, each kept while it is the current one or a frame slot was last submitted with it.  A frame
 * uses the table that was in force when it was submitted; frames in flight keep theirs, and so does a frame re-run after a
 * pair-buffer overflow, whatever is set afterwards.  Setting a table does not wait for frames in flight: the copy goes through a
 * pinned staging buffer on the ctx stream, and the frames submitted afterwards are ordered behind it (only a version whose buffers
 * must grow past the largest table seen so far allocates).  Under GSWT_OPT_GRAPH the table's pointer and length are arguments of
 * the k_project node; switching styles on or off selects another k_project instantiation and the slot's graph is rebuilt.
 *
 * Refused with GSWT_ERR_BAD_ARG, the reason in gswt_last_error and the table in force unchanged: styles == NULL with n_styles > 0;
 * n_styles > 1 << 20; an entry with a nonzero _pad byte (the message names the entry).  With styles on, a submit returns
 * GSWT_ERR_BAD_ARG before anything is enqueued when GSWT_OPT_STRICT_VS = 0 (sequence v2 has no styled form).
 * Out of scope: styles for gswt_proxy_render / gswt_skybox_render, outlines, per-splat styles, the CPU oracle. */
typedef struct {
    uint8_t tint[3];        /* R, G, B of the tint colour */
    uint8_t tint_strength;  /* 0: no tint ... 255: the tint colour replaces the splat's */
    uint8_t dim;            /* 0: opacity unchanged ... 254; 255: the cell is hidden */
    uint8_t _pad[3];        /* must be zero */
} gswt_tile_style;          /* 8 bytes; all-zero = neutral */
GSWT_API int gswt_set_tile_styles(gswt_ctx *ctx, const gswt_tile_style *styles, size_t n_styles);

/* ---- sun shadows: shade splats and proxy ground by a light-space depth map -------------------------
 * An orthographic frame along the sun's direction (GSWT_OPT_PROJECTION = 1 with gswt_render_depth, over gswt_proxy_render_ortho's
 * ground) is a shadow map: the depth of the first surface the light meets.  This call is its consumer: every splat of the frames
 * submitted afterwards, and every ground pixel of the proxy passes called afterwards, is tested against the map and, where something
 * lies between it and the light, goes toward shade_color.  The host may equally pass a map of its own occluders (a building placed
 * on the terrain) in the same convention, or the minimum of both.  The reference has no shadows.
 *
 * Input image.  depth is width x height f32, row 0 at the top, 0 near .. 1 far: exactly what gswt_render_depth writes for an
 * orthographic frame of that size.  depth_on_device != 0: a device pointer, copied device to device on the ctx stream (the caller
 * orders later writes to it behind that stream, as for every device pointer the library reads); otherwise a host pointer, copied
 * inside the call.  p == NULL or depth == NULL: shadows off, the default.  A frame with shadows off launches exactly the kernels it
 * launches without this call and is bit for bit the same frame.
 *
 * world_to_light (M, column-major, affine) takes a world point to the light's image: row 0 and 1 light NDC x, y (+y up, -1..1 over
 * the image), row 2 the depth in the image's convention.  For a map rendered by this library, M = opengl_to_wgpu * projection * view
 * of the orthographic camera (shadows.from_ortho_camera in the Python layer evaluates it in float64 and rounds once).
 *
 * Definition.  Every written operator is one correctly rounded binary32 operation, nothing fused.  c is the surface-mapped,
 * scene-scaled centre A6 feeds to the view matrix; W, H = width, height; Z the image:
 *     lx = ((M[0]*c0 + M[4]*c1) + M[8]*c2) + M[12]        ly, ld likewise from rows 1, 2
 *     u  = (lx * 0.5f + 0.5f) * (float)W - 0.5f           v = (0.5f - ly * 0.5f) * (float)H - 0.5f
 *     outside:  !(ld >= 0 && ld <= 1) || !(u > -1 && u < W) || !(v > -1 && v < H)   (NaN included)  ->  lit = 1
 *     x0 = floorf(u); y0 = floorf(v); wx = u - x0; wy = v - y0;   r = ld - bias
 *     t(i, j) = texel in range ? (r > Z[j*W + i] ? 0.0f : 1.0f) : 1.0f            (a NaN texel is lit)
 *     lit = (t00*(1.0f - wx) + t10*wx)*(1.0f - wy) + (t01*(1.0f - wx) + t11*wx)*wy
 *     sh  = strength * (1.0f - lit)
 *     sh == 0: the colour word stays as it is.  Otherwise per channel  c' = c*(1.0f - sh) + shade_c*sh
 * Pixel centres sit at integers: pixel x of the orthographic frame that produced the map is u = x.  The 2 x 2 compare is the usual
 * percentage-closer filter: a shadow's edge is a ramp one texel wide.
 * Order: tile-style tint, then the shadow, then the fog.  The colour is quantised once at the end, by the fog's expression (or, with
 * the fog off, by the same expression on the shaded floats): byte' = (uint32_t)rintf(fminf(fmaxf(c', 0), 1) * 255.0f), and the
 * record's colour word becomes byte'_r | byte'_g << 8 | byte'_b << 16 | (word & 0xFF000000).  The debug draw modes (draw_mode != 0)
 * keep their colours.  The shadow changes the colour word only: visibility, n_visible, pairs, axes, alpha, depth and the pick
 * identity are those of the frame without it, the record stays 32 bytes and the compositors are untouched.
 * gswt_debug_read_projected reports the shaded bytes, (float)byte' / 255.0f.
 * M * c is evaluated in binary32 at the world coordinates' magnitude: far from the world origin the lookup loses the bits the
 * coordinates have lost (at |c| = 2^17 and 1 world unit per texel, about 2^-6 texel); exactness there is out of scope.
 *
 * Vertex stage.  k_project gains an eighth template flag SHD on its strict instantiations; the image pointer, its size and the block
 * are a kernel argument of their own (under GSWT_OPT_GRAPH a node argument: another map updates one node, switching shadows on or off
 * selects another instantiation and the slot's graph is rebuilt).  The four texel loads are issued behind the frustum rejection, in
 * front of A7 / A8, unconditionally from indices clamped into the image, and read behind A9.
 *
 * Proxy pass.  gswt_proxy_render and gswt_proxy_render_ortho read the map in force when they are called and apply the same function
 * at the ray's hit point in world coordinates (the orthographic pass works in its grid frame and adds the grid's origin back):
 *     rgb' = rgb*(1.0f - sh) + shade_color*sh        behind `brightness`, in front of the fog, alpha 1
 * The depth they write, the pixels they leave alone and the black_background output are unchanged.
 *
 * Copy and lifetime.  The image is copied by the call into a buffer of the library's: one of a small pool of map versions (frame
 * slots + 2, allocated when first used), each kept while it is the current one or a frame slot was last submitted with it.  A frame
 * uses the version in force when it was submitted; frames in flight and a frame re-run after a pair-buffer overflow keep theirs.
 * Setting a map waits for no frame: the copy is queued on the ctx stream (through pinned staging from a host pointer) and the frames
 * and proxy passes submitted afterwards are ordered behind it.  The one exception: a version that meets an image larger than its buffers
 * (they are allocated at twice the first image's size) frees and reallocates them, and freeing device memory waits for the device, frames in
 * flight included.  A host that keeps its map's size, or halves and doubles it, never meets it after each version's first use.
 *
 * Refused with GSWT_ERR_BAD_ARG, the field named in gswt_last_error and the map in force unchanged: any non-finite field; a bottom
 * row of world_to_light other than (0, 0, 0, 1); bias < 0; strength outside (0, 1]; a shade_color component outside [0, 1]; a
 * nonzero _pad; width or height outside 1..4096.  With a map on, a submit returns GSWT_ERR_BAD_ARG before anything is enqueued when
 * GSWT_OPT_STRICT_VS = 0 (sequence v2 has no shadowed form).
 * Out of scope: filters wider than 2 x 2, slope-scaled bias, cascades, perspective (spot) lights, shadows on the skybox, the CPU
 * oracle. */
typedef struct {
    float world_to_light[16]; /* column-major, affine: bottom row exactly (0,0,0,1).  Row 0, 1: light NDC x, y (+y up, -1..1 over the
                                 image); row 2: depth in the depth image's convention, 0 near .. 1 far */
    float bias;               /* >= 0, depth units */
    float strength;           /* in (0, 1] */
    float shade_color[3];     /* each in [0, 1]: what a fully shadowed colour goes toward at strength 1 */
    uint32_t _pad[3];         /* zero */
} gswt_shadow_params;         /* 96 bytes */
GSWT_API int gswt_set_shadow_map(gswt_ctx *ctx, const gswt_shadow_params *p, const float *depth, int width, int height, int depth_on_device);

/* ---- clip volumes: cut splats and proxy ground by boxes, ellipsoids and half-spaces ------------------
 * The reference's "Clip by Z" (use_clip / clip_height) removes everything below one horizontal plane and tile styles hide whole map
 * cells.  A clip volume is the per-splat control between them: a cross-section along any plane, a region of interest, a hole of the
 * host's own shape, a sun map from which the cut-away part casts no shadow.  Up to GSWT_MAX_CLIP_VOLUMES volumes are in force at a
 * time; v == NULL or n == 0 switches them off (the default), and a frame with none launches exactly the kernels it launches without
 * this call and is bit for bit the same frame.  The reference has no clip volumes.
 *
 * A volume is an affine map world_to_unit (M, rows 0..2, row-major 3 x 4) into the volume's unit frame and a shape there.  The tested
 * point c is the surface-mapped, scene-scaled centre A6 feeds to the view matrix, the point gswt_set_shadow_map looks up.  (clip_height
 * tests the SURFACE's height under the splat -- 0 for every splat without a surface --, these volumes the centre itself.)  Every written operator is one correctly rounded binary32 operation, nothing fused:
 *     u_r = ((M[4r]*c0 + M[4r+1]*c1) + M[4r+2]*c2) + M[4r+3]                    r = 0, 1, 2
 *     GSWT_CLIP_BOX        inside:  |u0| <= 1 && |u1| <= 1 && |u2| <= 1         (max(|u0|, |u1|, |u2|) <= 1)
 *     GSWT_CLIP_ELLIPSOID  inside:  (u0*u0 + u1*u1) + u2*u2 <= 1
 *     GSWT_CLIP_HALFSPACE  inside:  u2 <= 0                                      (rows 0 and 1 are not read and may hold anything)
 * Every comparison is an ordinary IEEE compare: a NaN coordinate is not inside, a point on the boundary is.
 * A splat stays exactly when (there is no GSWT_CLIP_KEEP volume, or it is inside at least one of them) and it is inside no volume
 * without that flag (a cut volume).  The cut is by centre, like clip_height's; there is no feathered edge.  A splat that stays is bit
 * for bit what it was -- record, depth, pair rectangle, alpha --; a hidden one counts neither in n_visible nor in n_pairs and never
 * appears in the pick image.  M c is evaluated in binary32 at the world coordinates' magnitude, like the shadow lookup.
 *
 * Vertex stage.  k_project gains a ninth template flag CLIP on its strict instantiations; the test sits directly behind the clip_height
 * test, in front of the atmosphere's fade, so that a hidden splat costs nothing more.  The set travels by value, as one kernel argument
 * of its own: a frame keeps the set it was submitted with (frames in flight, a re-run after an overflow, GSWT_OPT_GRAPH's replay -- a
 * node argument), setting volumes waits for no frame and allocates nothing.
 *
 * Proxy passes.  gswt_proxy_render, gswt_proxy_render_ortho and gswt_proxy_render_sphere read the set in force when they are called
 * and see only its volumes flagged GSWT_CLIP_GROUND; the same rule is applied to those volumes alone at the fragment's world hit point.
 * A hidden fragment is discarded: its colour and depth keep what was there, like a fragment under clip_height.  In the sphere pass the
 * test joins what each of the two candidates (near, then far) must pass, so a near surface that is cut away shows the inside of the far
 * one.  Without a GROUND volume the passes are bit for bit what they were.
 *
 * Refused with GSWT_ERR_BAD_ARG, the volume's index and the field named in gswt_last_error and the set in force unchanged:
 * n > GSWT_MAX_CLIP_VOLUMES; v == NULL with n > 0; an unknown shape; an unknown flag bit; a nonzero reserved word; a non-finite entry of
 * a row the shape reads.  With volumes set, a submit returns GSWT_ERR_BAD_ARG before anything is enqueued when GSWT_OPT_STRICT_VS = 0
 * (sequence v2 has no clipped form).  Out of scope: soft edges, per-pixel clipping of a splat's footprint, the CPU oracle. */
#define GSWT_MAX_CLIP_VOLUMES 8
#define GSWT_CLIP_BOX        0u   /* inside: max(|u0|, |u1|, |u2|) <= 1          */
#define GSWT_CLIP_ELLIPSOID  1u   /* inside: (u0*u0 + u1*u1) + u2*u2 <= 1        */
#define GSWT_CLIP_HALFSPACE  2u   /* inside: u2 <= 0   (rows 0 and 1 are unread) */
#define GSWT_CLIP_KEEP    1u      /* flag: a keep volume (hide what is outside); without it a cut volume (hide what is inside) */
#define GSWT_CLIP_GROUND  2u      /* flag: the proxy passes apply this volume too */
typedef struct gswt_clip_volume {
    float    world_to_unit[12];   /* rows 0..2 of an affine map, row-major 3 x 4: world point -> the volume's unit frame */
    uint32_t shape, flags;
    uint32_t reserved[2];         /* 0 */
} gswt_clip_volume;               /* 64 bytes */
GSWT_API int gswt_set_clip_volumes(gswt_ctx *ctx, const gswt_clip_volume *v, size_t n);   /* NULL or n = 0: off (the default) */

/* GSWTRenderer::new (renderer.rs:31-349): uploads PreloadData.tile_splats_merged.tex_data
 * (8 u32 per splat, renderer.rs:236-248) and all static base lists (renderer.rs:290-327).
 * lists is [n_lod][n_tile][n_view] row-major. */
GSWT_API int gswt_upload_scene(gswt_ctx *ctx, const uint32_t *tex_data, size_t n_splats,
                               const gswt_base_list *lists, int n_lod, int n_tile, int n_view);

/* GSWTRenderer::configure (renderer.rs:351-405): height map, R32Float / linear / repeat.
 * height_map may be NULL (surface_type None). */
GSWT_API int gswt_configure(gswt_ctx *ctx, const float *height_map, int hm_w, int hm_h);

/* Swap-in of a SortData (state.rs:361-376) = the per-sort-event part of render():
 * the ordered draw list (back-to-front, renderer.rs:466) and the concatenated
 * gs_index / gs_map_id / gs_lod_id arrays of all merged groups (renderer.rs:517-561).
 * merged_lod_id may be NULL when no draw has merged_has_lod. */
GSWT_API int gswt_set_draws(gswt_ctx *ctx, const gswt_draw *draws, int n_draws,
                            const uint32_t *merged_gs_index, const uint32_t *merged_map_id,
                            const uint32_t *merged_lod_id, size_t n_merged);

/* On-device merged lists (replaces the CPU hot loop of sort_tiles, wangtile.rs:595-670, and the per-sort-event
 * upload of 12 B per merged splat, renderer.rs:517-561).
 * gswt_upload_raw_depth: TileBaseData.raw_depth of every [lod][tile][view] (structure.rs:551; one i32 per splat
 *   of that tile scene) and splats_merge_offset[lod][tile] (wangtile.rs:34), once after gswt_upload_scene.
 * gswt_set_draws_merge_groups: like gswt_set_draws, but the merged arrays are built on the device from the
 *   group descriptions: group g = one MergedFrom tile (view_id, members in from_vec order); member = (map index,
 *   tid, and the other LOD it is Changing to, or -1).  A merged draw's merged_offset / merged_count must be
 *   the group's range in the concatenation of all groups (sum of the members' raw-depth lengths, in order);
 *   draws[i].merged_group names its group. */
typedef struct {
    uint32_t view_id;
    uint32_t first_member;
    uint32_t n_members;
    uint32_t _pad;
} gswt_merge_group;
typedef struct {
    uint32_t map_index;
    uint32_t lod, tile;
    int32_t other_lod;   /* lod + 1 for Changing(true), lod - 1 for Changing(false), -1 otherwise */
} gswt_merge_member;
GSWT_API int gswt_upload_raw_depth(gswt_ctx *ctx, const int32_t *const *raw_depth /* [n_lod*n_tile*n_view] */,
                                   const uint32_t *counts /* [n_lod*n_tile] */,
                                   const uint32_t *merge_offset /* [n_lod*n_tile] */);
GSWT_API int gswt_set_draws_merge_groups(gswt_ctx *ctx, const gswt_draw *draws, int n_draws,
                                         const gswt_merge_group *groups, int n_groups,
                                         const gswt_merge_member *members, int n_members);
/* GSWTRenderer::new from a rows-only wang (gswt_wang_new_rows): uploads the normalised 32-byte rows of every tile scene
 * (rows32 / counts [n_lod*n_tile], lod-major; gswt_wang_rows) and builds on the device what gswt_upload_scene(preload) +
 * gswt_upload_raw_depth(raw_depth_tables) of a full wang leave behind, bit for bit: the texture (generate_texture), the raw
 * depths of every presort view, the base lists (sort_raw_depth of each tile's LOD followed by the next LOD), the static
 * arena with its pair and self lists, their 256-entry chunk boxes and the tile-local bounds.  presort_vp: the n_view
 * sort_projection * view matrices (gswt_wang_presort_view_proj), n_view <= 16.  gswt_set_draws_merge_groups works right
 * after it.  Refused before anything is enqueued: null rows, an empty tile scene, n_lod > 16, more than 2^28 splats, more
 * than 65 536 (lod, tile) lists (the list id takes 16 bits of the sort key).  Returns when the build has finished. */
GSWT_API int gswt_upload_scene_rows(gswt_ctx *ctx, const uint8_t *const *rows32, const uint32_t *counts, int n_lod, int n_tile,
                                    const float *presort_vp, int n_view);
/* Test hook: reads back one item of the scene state for comparing two contexts.  n_bytes receives its size; out may be
 * NULL to ask for the size only.  Items: the texture (32 B per splat), the raw-depth arena (i32), its tables (raw_off
 * [n_lod*n_tile*n_view], counts, merge offsets [n_lod*n_tile], u32), the static arena (u32), the chunk boxes (6 f32 each),
 * the list table (pair_base, pair_count, self_base, self_count, pair_box, self_box: 6 u32 per list [lod][tile][view]), the
 * local bounds (lo.xyz, hi.xyz, largest covariance bound: 7 f32). */
enum { GSWT_SCENE_TEX = 0, GSWT_SCENE_RAW_DEPTH = 1, GSWT_SCENE_RAW_TABLES = 2, GSWT_SCENE_STATIC_LIST = 3, GSWT_SCENE_STATIC_BOXES = 4,
       GSWT_SCENE_LISTS = 5, GSWT_SCENE_BOUNDS = 6 };
GSWT_API int gswt_debug_read_scene(gswt_ctx *ctx, int what, void *out, size_t cap_bytes, size_t *n_bytes);
/* Test hook: the device-resident merged arrays (gs_index | lod << 28, map id), n entries each. Host pointers. */
GSWT_API int gswt_debug_read_merged(gswt_ctx *ctx, uint32_t *packed_list, uint32_t *map_id, size_t capacity, size_t *n);

/* GSWTRenderer::render (renderer.rs:407-592), per frame.  bg_rgba (W*H*4 f32) is the
 * colour attachment content the pass loads (LoadOp::Load, :425; skybox/proxy output) or
 * NULL for transparent black; bg_depth (W*H f32) is the proxy depth buffer (:433-434) or
 * NULL for the 1.0 clear (:436).  out_rgba receives rows_out*W*4 f32 where rows_out = H,
 * or the shard's rows when cfg->shard_count > 1 (see gswt_shard_rows); for the 8-bit
 * cfg->out_format values rows_out*W*4 bytes, for the video ones rows_out*W*3/2 bytes
 * (gswt_out_image_bytes).  Pointers are device pointers when *_on_device is nonzero,
 * host pointers otherwise.  An out_format other than GSWT_OUT_* / GSWT_VIDEO_*, or a
 * video format with an odd width or height, returns GSWT_ERR_BAD_ARG before anything is
 * enqueued. */
GSWT_API int gswt_render(gswt_ctx *ctx, const gswt_camera_uniforms *camera,
                         const gswt_scene_uniforms *scene, const gswt_render_config *cfg,
                         int width, int height,
                         const float *bg_rgba, const float *bg_depth, int bg_on_device,
                         float *out_rgba, int out_on_device);

/* Asynchronous form of gswt_render for pipelining consecutive frames (State::render is called once per
 * display refresh; with the device library the next frame can be queued while the previous one is still
 * executing).  All pointers are DEVICE pointers.  gswt_render_async enqueues the frame and returns a
 * ticket; gswt_render_wait(ticket) blocks the host until it finished, re-runs it if the pair buffers had
 * to grow, and makes gswt_last_timings refer to it.  At most gswt_frame_slots() (= 4) frames may be in
 * flight (enqueuing one more waits for the oldest).  Each frame in flight runs on its own internal stream
 * with its own per-frame buffers, so the frames OVERLAP on the GPU; frames in flight together must write
 * different output buffers.  Ordering against the ctx stream (gswt_set_stream):
 *   - a frame starts after all work submitted to the ctx stream before its gswt_render_async call
 *     (producers of bg_*, earlier consumers of out_rgba_dev);
 *   - gswt_render_fence(ticket) orders the ctx stream behind that frame, so work submitted to the ctx stream afterwards sees
 *     its output (e.g. the RCCL all-gather of the shards).  All-or-nothing like GSWTRenderer::render (renderer.rs:407-414): a
 *     frame whose pair buffers overflowed is re-run with larger ones BEFORE the fence releases the ctx stream, so a fenced
 *     consumer never reads an incomplete image.  Overflow is only known on the host, hence the call blocks the host until
 *     THIS frame has finished (not the younger frames in flight: submit them before fencing frame i and the GPU stays
 *     busy).  The ticket stays valid; gswt_render_wait(ticket) then returns at once with the frame's status and timings.
 *   - gswt_set_draws*, gswt_upload_scene, gswt_configure first run every frame in flight to completion against the state it
 *     was submitted with (tickets stay valid). */
GSWT_API int gswt_render_async(gswt_ctx *ctx, const gswt_camera_uniforms *camera,
                               const gswt_scene_uniforms *scene, const gswt_render_config *cfg,
                               int width, int height, const float *bg_rgba_dev, const float *bg_depth_dev,
                               float *out_rgba_dev, int *ticket);
GSWT_API int gswt_frame_slots(void);   /* frames that may be in flight at once */

/* gswt_render / gswt_render_async that also write the frame's composited DEPTH image.  out_depth receives rows_out*W f32
 * (the colour output's geometry in every shard mode; the padding rows / columns of a shard are zeroed like the colour's),
 * whatever cfg->out_format is; NULL behaves exactly as gswt_render / gswt_render_async, which are these calls with NULL.
 * Definition, per pixel: the splats are walked in the compositor's blend order with the colour's coverage decisions, its
 * weights w_i = T_i * e_i and its early-out (transmittance_eps), and
 *     Z = T_final * z_bg + sum_i w_i * z_i
 * where z_i is the splat's NDC depth -- clip z / w of the centre, the value the proxy depth test compares (renderer.rs:181-182)
 * -- and z_bg is bg_depth[p] with a proxy depth buffer bound, 1.0 (the clear value, :436) without one.  So depth is blended
 * like one more colour channel over a background surface at z_bg: a pixel no splat covers gets exactly z_bg, and the
 * normalised expected depth of the splats alone is (Z - T_final * z_bg) / (1 - T_final), T_final being the transmittance
 * left (1 - alpha of the f32 colour output when no bg_rgba is bound).  Z is in the depth-buffer convention (NDC z, 0 near .. 1 far), not linear view depth.  Pointer rules are
 * those of gswt_render (out_depth is a host pointer unless out_on_device) and gswt_render_async (device pointers; frames in
 * flight together must write different depth buffers as well); a frame re-run after a pair-buffer overflow rewrites its depth.
 * A missing out_rgba, or an out_depth that is out_rgba, returns GSWT_ERR_BAD_ARG before anything is enqueued.  The depth image
 * is not part of the gathers (gswt_render_gather, gswt_unshard*). */
GSWT_API int gswt_render_depth(gswt_ctx *ctx, const gswt_camera_uniforms *camera,
                               const gswt_scene_uniforms *scene, const gswt_render_config *cfg,
                               int width, int height,
                               const float *bg_rgba, const float *bg_depth, int bg_on_device,
                               float *out_rgba, float *out_depth, int out_on_device);
GSWT_API int gswt_render_async_depth(gswt_ctx *ctx, const gswt_camera_uniforms *camera,
                                     const gswt_scene_uniforms *scene, const gswt_render_config *cfg,
                                     int width, int height, const float *bg_rgba_dev, const float *bg_depth_dev,
                                     float *out_rgba_dev, float *out_depth_dev, int *ticket);

/* gswt_render_depth / gswt_render_async_depth that also write the frame's PICK image: which tile instance and which splat
 * each pixel shows.  out_pick receives rows_out*W records of 16 bytes (the colour output's geometry in every shard mode; the
 * padding rows / columns of a shard are zero bytes like the other outputs), whatever cfg->out_format is; out_depth may be
 * NULL; a NULL out_pick behaves exactly as gswt_render_depth / gswt_render_async_depth, which are these calls with NULL.
 * Definition, per pixel: the splats are walked in the compositor's blend order with the colour's coverage decisions
 * (|p|^2 <= 4, the proxy depth test when bg_depth is bound), its weights w_i = T_i * e_i and its early-out
 * (transmittance_eps).  The pixel's pick is the splat with the LARGEST w_i -- the one that contributes most to the pixel's
 * colour; among equal weights the front-most wins (the comparison is a strict >).  A pixel no splat covers gets
 * map_index = entry = 0xFFFFFFFF, weight = 0 and depth = z_bg: bg_depth[p] with a proxy depth buffer bound, 1.0 without
 * one (the depth image's convention).
 * A tile's list may be walked in segments (GSWT_OPT_SEGMENT).  A segment starts from T = 1, so its weights are the pixel's
 * divided by the transmittance in front of the segment and its own winner is its candidate; the candidates are compared as
 * T_prefix * w'_max, front to back, again with a strict >.  What is promised about identity: it is exact wherever the winner
 * leads by more than rounding (weights are binary32; the segmented product rounds once more); between candidates whose
 * weights agree to rounding either may be returned.  The returned weight and depth always belong to the returned splat.
 * Pointer rules are those of the depth output: out_pick is a host pointer (staged) unless out_on_device; frames in flight
 * together must write different pick buffers; a frame re-run after a pair-buffer overflow rewrites its pick.  A missing
 * out_rgba, or an out_pick equal to out_rgba or out_depth, returns GSWT_ERR_BAD_ARG before anything is enqueued.  Pick
 * frames run under GSWT_OPT_GRAPH and GSWT_OPT_TIMING as depth-output frames do.  GSWT_OPT_COMPOSITE = 1 is accepted
 * and runs the default compositor, for a pick frame as for any other.  The pick image is not part of the gathers (gswt_render_gather,
 * gswt_unshard*). */
typedef struct {
    uint32_t map_index;  /* tile instance: TileUniforms.map_index of a static draw, the member's map id of a merged one */
    uint32_t entry;      /* the list word of the splat: gs_index | lod_id << 28 */
    float depth;         /* that splat's NDC depth: the value the depth test compares, bit-identical to the vertex stage's */
    float weight;        /* its w_i, in (0, 1] */
} gswt_pick;
GSWT_API int gswt_render_pick(gswt_ctx *ctx, const gswt_camera_uniforms *camera,
                              const gswt_scene_uniforms *scene, const gswt_render_config *cfg,
                              int width, int height,
                              const float *bg_rgba, const float *bg_depth, int bg_on_device,
                              float *out_rgba, float *out_depth, gswt_pick *out_pick, int out_on_device);
GSWT_API int gswt_render_async_pick(gswt_ctx *ctx, const gswt_camera_uniforms *camera,
                                    const gswt_scene_uniforms *scene, const gswt_render_config *cfg,
                                    int width, int height, const float *bg_rgba_dev, const float *bg_depth_dev,
                                    float *out_rgba_dev, float *out_depth_dev, gswt_pick *out_pick_dev, int *ticket);
GSWT_API int gswt_render_wait(gswt_ctx *ctx, int ticket);
GSWT_API int gswt_render_fence(gswt_ctx *ctx, int ticket);

/* ---- background passes (state.rs:384-392) -------------------------------------------------------
 * State::render runs Skybox::render and Proxy::render before GSWTRenderer::render; their colour /
 * depth targets are what gswt_render takes as bg_rgba / bg_depth.  Here they are per-pixel compute
 * passes on the ctx stream (a following gswt_render / gswt_render_async is ordered after them). */

/* proxy.wgsl `Uniforms` / proxy.rs:470-511, byte-exact (224 B) */
typedef struct gswt_proxy_uniforms {
    float height_offset;            /*   0 */
    float tile_width;               /*   4 */
    uint32_t surface_type;          /*   8 */
    float width_scale;              /*  12 */
    uint32_t map_proxy;             /*  16 */
    uint32_t use_clip;              /*  20 */
    float clip_height;              /*  24 */
    float brightness;               /*  28 */
    uint32_t black_background;      /*  32 */
    uint32_t _pad0[3];              /*  36 */
    float view[16];                 /*  48 */
    float projection[16];           /* 112 */
    uint32_t map_half_wh[2];        /* 176 */
    int32_t center_coord[2];        /* 184 */
    float height_map_scale[4];      /* 192 */
    float cam_pos[4];               /* 208 */
} gswt_proxy_uniforms;              /* 224 */

/* Skybox::configure (skybox.rs:341-455): the cube map, 6 faces (+X -X +Y -Y +Z -Z) of face_size^2 RGBA f32 texels
 * (host pointer).  `equirectangular` is Skybox.is_equi (skybox.wgsl:35-38). */
GSWT_API int gswt_skybox_configure(gswt_ctx *ctx, const float *faces_rgba, int face_size, int equirectangular);
/* Skybox::configure with an HDR panorama (skybox.rs:490-668, skybox.wgsl:62-96): bakes the equirectangular image
 * (host pointer, equi_width x equi_height RGBA f32, row-major, linear HDR, row 0 at the top; alpha ignored) into the
 * cube map on the device -- per texel the face's view ray, SampleSphericalMap, one bilinear Repeat tap, Reinhard and
 * 1/2.2 gamma -- and sets is_equi.  The reference bakes at face_size = CUBEMAP_RESO = 2048.  The panorama is staged in
 * a temporary device buffer for the call only.  GSWT_ERR_BAD_ARG (nothing launched, previous skybox kept) for a null
 * pointer, equi_width / equi_height outside 1..32768 or face_size outside 1..16384. */
GSWT_API int gswt_skybox_configure_equirect(gswt_ctx *ctx, const float *equi_rgba, int equi_width, int equi_height, int face_size);
/* Copies the current cube map to the host: 6 * face_size^2 * 4 floats (+X -X +Y -Y +Z -Z), as gswt_skybox_configure
 * takes them.  GSWT_ERR_STATE before any skybox configure. */
GSWT_API int gswt_skybox_download(gswt_ctx *ctx, float *faces_rgba_host);
/* Skybox::render (skybox.rs:457-488): LoadOp::Clear + the cube drawn at depth 1 = every pixel of out_rgba_dev
 * (W*H*4 f32, device) is overwritten with (cube rgb, 1). */
GSWT_API int gswt_skybox_render(gswt_ctx *ctx, const gswt_camera_uniforms *camera, int width, int height, float *out_rgba_dev);
/* Proxy::configure (proxy.rs:208-364): the mip chain of the proxy texture (square, tex_size >> level, RGBA f32, host
 * pointers) and the grid dimension of the "full" proxy (Proxy::GRID_DIM = 2048, proxy.rs:29).  The height map is the one
 * given to gswt_configure. */
GSWT_API int gswt_proxy_configure(gswt_ctx *ctx, const float *const *mips, int tex_size, int n_mips, int grid_dim);
#define GSWT_PROXY_SRC_RGBA8   0   /* decoded 8-bit RGBA, 4 B per texel (PNG/JPEG via to_rgba8) */
#define GSWT_PROXY_SRC_RGBA16  1   /* decoded 16-bit RGBA, 8 B per texel (16-bit PNG via to_rgba16) */
/* upload_proxy_texture + Proxy::configure (proxy.rs:513-554, 289-318) from the decoded image: `pixels` (host pointer) is
 * width x height texels of src_format, row-major, row 0 first, channels R G B A (img.to_rgba8().into_raw() or to_rgba16()).
 * Builds the whole chain tex_size, tex_size / 2, ..., 1 (log2(tex_size) + 1 levels) on the device, each level resampled from
 * the ORIGINAL image as image::imageops::resize(.., n, n, Lanczos3) + to_rgba32f does: a vertical then a horizontal Lanczos3
 * pass in f32, window clipped and renormalised at the image edges, the result clamped, rounded half away from zero and
 * divided by 255 / 65535; a level with (n, n) == (width, height) is a copy.  Afterwards the context is exactly as after
 * gswt_proxy_configure with that chain (gswt_proxy_download reads it back).  tex_size is the caller's max_size (the
 * reference computes 2^floor(ln(width) / ln(2)) in f32, whose value at width 8192 depends on the logf rounding); it may
 * exceed width or height (then the same formula upsamples).
 * Device memory for the call, besides the chain (tex_size^2 * 16 * 4/3 B): the source (rows padded to 16 B), the f32
 * intermediate of the largest resampled level (width * n * 16 B: 128 MiB for a 4096^2 image at tex_size 4096, whose level 0
 * is a copy; 4 GiB at the 16384 limit, not strip-mined), partial sums of the small levels (<= 8 MiB) and the tap tables,
 * each staging buffer with up to a quarter of allocator headroom.
 * GSWT_ERR_BAD_ARG (nothing staged, previous proxy kept) for a null image, width / height outside 1..16384, an unknown
 * src_format, tex_size not a power of two in 1..16384 or grid_dim outside 1..32768.  A failure after the old texture starts
 * being overwritten leaves no proxy (as before any configure). */
GSWT_API int gswt_proxy_configure_image(gswt_ctx *ctx, const void *pixels, int width, int height, int src_format,
                                        int tex_size, int grid_dim);
/* Copies the current proxy chain to the host, levels packed tex_size >> l for l = 0.., each (tex_size >> l)^2 RGBA f32 texels,
 * whichever configure call produced it.  GSWT_ERR_STATE before any proxy configure. */
GSWT_API int gswt_proxy_download(gswt_ctx *ctx, float *mips_rgba_host);
/* ONE draw of Proxy::render (proxy.rs:366-447): u->map_proxy selects the GRID_DIM grid (0, `proxy_full`) or the tile-map
 * grid (1, `proxy_map`).  rgba_dev (W*H*4) and depth_dev (W*H) are device buffers updated in place: colour LoadOp::Load,
 * depth test Less with depth write.  clear_depth != 0 first fills depth_dev with 1.0 (the pass's LoadOp::Clear(1.0)). */
GSWT_API int gswt_proxy_render(gswt_ctx *ctx, const gswt_proxy_uniforms *u, int width, int height, float *rgba_dev, float *depth_dev,
                               int clear_depth);
/* ---- orthographic proxy pass: the ground under top-down maps, minimaps, height fields and sun-direction depth maps ----
 * ONE proxy draw under an orthographic camera: the same 224-byte block, the same buffers (colour loaded, depth tested Less and
 * written, clear_depth != 0 fills depth_dev with 1.0 first), on the ctx stream; map_proxy selects the grid as above.  It is an
 * entry point of its own, NOT a reading of GSWT_OPT_PROJECTION: gswt_proxy_render, its validation and its launch do not depend on
 * that option or on this call.  The fields mean what they mean in an orthographic gswt_camera_uniforms: `projection` is an affine
 * OpenGL-convention ortho() matrix, `view` the look-at, and `cam_pos` the REFERENCE POINT, not the eye -- the pass uses it for the
 * fog distance only.  gswt_skybox_render has no orthographic form.
 *
 * Returns GSWT_ERR_BAD_ARG with the reason in gswt_last_error, nothing enqueued and clear_depth not performed, for: everything
 * gswt_proxy_render refuses (null pointers, width / height <= 0, tile_width <= 0, width_scale <= 0 with the full grid); a
 * projection p (column-major) whose bottom row p[3], p[7], p[11], p[15] is not exactly (0, 0, 0, 1); p[1], p[2], p[4], p[6],
 * p[8], p[9] not all zero (not of ortho() form); p[0], p[5] or p[10] zero or not finite; p[12], p[13] or p[14] not finite; a view
 * whose upper 3x3 cannot be inverted to finite numbers.  GSWT_ERR_STATE as gswt_proxy_render: no proxy texture unless
 * black_background (a depth-only ground -- the height-field and shadow-map use -- needs no texture), a HeightMap surface without
 * a height map.
 *
 * The definition.  Every written operator is one binary32 operation, nothing fused, except the host part marked (binary64).
 * V = view, GP = opengl_to_wgpu * projection as in the perspective pass (GP[10] = 0.5f * p[10] + 0.5f * p[11], GP[14] = 0.5f *
 * p[14] + 0.5f * p[15]; depth = GP[10] z + GP[14] of camera-space z, q.w = 1).
 *   The pass works in the GRID FRAME, world - g with g = (gx0, gy0, 0), (gx0, gy0) the binary32 position of lattice point (0, 0) as the
 *   perspective pass computes it: far from the world origin (1e5: ulp 0.008) the rays, the triangles and the depth are then of the
 *   size of the map, and nothing but the lattice itself -- the reference's binary32 vertices -- is rounded at the world coordinates'
 *   magnitude.  A lattice vertex (rx, ry, z) of the perspective pass enters as (rx - gx0, ry - gy0, z).
 *   Host, once per call (binary64 from the binary32 entries, each result rounded to binary32 once):
 *     zn = (0 - GP[14]) / GP[10],  zf = (1 - GP[14]) / GP[10]            camera-space z of depth 0 and depth 1
 *     sz = -1 if GP[10] < 0 (depth grows along -z of the camera: ortho() with near < far), else +1
 *     z0 = zn - sz * 0.125 * |zf - zn|                                    the rays run the way depth grows and start an eighth of
 *                                                                         the depth range before the depth-0 plane: the whole range
 *                                                                         [0, 1] lies at ray parameter > 0, also with near < 0
 *     e  = R^-1 ((0, 0, z0) - t) - g,  R = upper 3x3 of V, t = (V[12], V[13], V[14]), the inverse by cofactors / determinant
 *     t' = t + R g            the view's translation in the grid frame: the depth of a hit is (V with t' for t, then GP) applied to it
 *     c' = cam_pos - g        the fog's reference point in the grid frame
 *     uv0 = frac(g.xy / tile_width / 4)       what the grid frame's texture coordinate lacks, whole periods dropped (Repeat)
 *   Ray of pixel (x, y):
 *     ndc.x = ((float)x + 0.5f) / (float)W * 2.0f - 1.0f;   ndc.y = 1.0f - ((float)y + 0.5f) / (float)H * 2.0f      (as the perspective pass)
 *     cx = (ndc.x - p[12]) / p[0];   cy = (ndc.y - p[13]) / p[5]
 *     o[k] = (V[4k] * cx + V[4k+1] * cy) + e[k],  k = 0, 1, 2       i.e. R^T (cx, cy, 0) + e = R^T (c - t) - g with c = (cx, cy, z0)
 *     d = sz * (V[2], V[6], V[10])                                   the view axis -(V[2], V[6], V[10]) (its negative for a matrix
 *                                                                    whose depth falls along it), the same for every pixel
 *   Why the host inverts: in binary32 R^T (c - t) cancels at the magnitude of the world coordinates and adds three products rounded
 *   there per component, different from pixel to pixel -- a lateral error of the ray that a slope turns into a depth error.  Here every
 *   large term is a constant of the frame, folded in binary64, and the per-pixel arithmetic is at the size of the view.  R^T stands
 *   in for R^-1 only on (cx, cy, 0), where a look-at's 2^-24 departure from orthonormal is 2^-24 of the view's extent.
 *   The ray parameter has no meaning of its own: the pass keeps the nearest fragment whose depth lies in [0, 1].
 *   Hit: the lattice, the two triangles per cell and their diagonal, the inclusive Moeller-Trumbore tests, the use_clip /
 *   clip_height discard on the interpolated mapped height and the depth (V then GP applied to o + t d, q.z / q.w) are the
 *   perspective pass's code.  The flat-surface branch cuts the plane z = height_offset directly.
 *   Grid walk: the perspective pass's 2-D DDA from the pixel's own origin.  A ray with d.x == d.y == 0 (every pixel of a top_down
 *   camera) tests the one cell under it and stops; a ray with one zero component walks a single row or column; at most
 *   nx + ny + 2 cells in any case.
 *   Texture LOD: the rays of the right and the lower pixel -- the same d from the origins of (x + 1, y) and (x, y + 1) -- are cut
 *   with the hit triangle's plane; rho = max |delta uv| * tex_size, lod = clamp(log2 rho, 0, n_mips - 1), trilinear Repeat taps
 *   and `brightness` as in the perspective pass.
 *   Texture coordinate: the perspective pass's (o + t d).xy / tile_width / 4 on the hit triangle's plane, in the grid frame, + uv0
 *   (added after the LOD differences are taken).
 *   Fog (gswt_set_atmosphere's fog part in force when the pass is called): hit = o + t d per component, (dx, dy, dz) = hit - c',
 *   dist = sqrtf((dx*dx + dy*dy) + dz*dz), rgb' = rgb * (1.0f - F) + fog_color * F with the F(dist) above -- the reference point the
 *   orthographic splat stage fades and fogs around, so the ground and the splats of a minimap fog by the same distance.
 *   The depth written, the pixels not written and the black_background output do not depend on the fog. */
GSWT_API int gswt_proxy_render_ortho(gswt_ctx *ctx, const gswt_proxy_uniforms *u, int width, int height, float *rgba_dev, float *depth_dev,
                                     int clear_depth);
/* ---- sphere proxy pass: the ground under the Sphere surface (planets), with depth and sun shade ----
 * ONE draw of the ground sphere |x| = r about the world origin, r = sphere_radius + height_offset, where WangTile::surface_mapping puts the
 * Sphere surface: the same 224-byte block and buffers as gswt_proxy_render (colour loaded, depth tested Less and written, clear_depth != 0
 * fills depth_dev with 1.0 first), on the ctx stream.  projection 0: perspective, the fields as in gswt_proxy_render; projection 1:
 * orthographic, the fields and the host-side binary64 set-up of gswt_proxy_render_ortho with g = 0 (the rays are of the planet's size at the
 * origin; cam_pos is the fog's reference point).  map_proxy, width_scale, surface_type and height_map_scale of the block are NOT read.
 * It is an entry point of its own: gswt_proxy_render and gswt_proxy_render_ortho with surface_type == 2 keep drawing the plane
 * z = height_offset, as the reference does, bit for bit.  Its depth image is what hides the far hemisphere's splats (bg_depth of
 * gswt_render), what the atmosphere's far fade dissolves into, and, drawn orthographically along the sun with black_background, the
 * occluder of a sun map (gswt_set_shadow_map): the planet shades its own night side.
 *
 * Returns GSWT_ERR_BAD_ARG with the reason in gswt_last_error, nothing enqueued and clear_depth not performed, for: what gswt_proxy_render
 * refuses (null pointers, width / height <= 0, tile_width <= 0 or not finite, with projection 0 a singular projection); projection not 0 or 1;
 * with projection 1 everything gswt_proxy_render_ortho refuses of the projection and the view; sphere_radius not finite or not positive;
 * sphere_radius + height_offset not finite or not positive; map_half_wh[0] == 0.  GSWT_ERR_STATE without a proxy texture, unless
 * black_background.
 *
 * The definition.  Every written operator is one binary32 operation, nothing fused; sqrtf, atan2f and log2f are named as such.
 *   Ray: o = cam_pos, d = the perspective pass's pixel ray (projection 0); o, d = the orthographic pass's origin and direction (projection 1).
 *   d is not normalised.  Dot products are (x x' + y y') + z z'.
 *   Intersection, written so that a grazing ray does not cancel at the size of |o|^2:
 *     dd = d.d;  tc = -(o.d) / dd;  c = o + tc d;  disc = r * r - c.c;  disc < 0: the ray misses;  h = sqrtf(disc / dd)
 *     candidates t1 = tc - h, then t2 = tc + h; hit = o + t d per component.  A candidate is kept if t > 0, the depth test of the plane
 *     passes accepts it (V then GP applied to hit: q.w > 0, q.z / q.w in [0, 1]) and it is not clipped: with use_clip == 1 a candidate with
 *     (hit.z / r) * sphere_radius < clip_height is dropped -- the splats' mapped_z of the same ground point.  The first kept candidate is
 *     the fragment: a camera inside the sphere, or a clipped cap, shows the inside of the far surface, as an unculled mesh would.
 *   Depth: the fragment's q.z / q.w, tested Less against depth_dev, then written.  black_background == 1 writes (0, 0, 0, 1) and is done.
 *   Texture coordinate, the inverse of the sphere unfolding (host/gswt_surface.h: sphere_plane_pos beside sphere_point):
 *     n = hit / r;  v = atan2f(n.z, sqrtf(n.x * n.x + n.y * n.y)) / PI + 0.5f;  u = atan2f(n.y, n.x) / (2 PI), u = u - floorf(u), 1 -> 0
 *       (v is asin(n.z) / PI + 0.5 written so that it keeps its digits at the poles: d asin / dz = 1 / |n.xy| turns the binary32 rounding of a
 *       hit point one pixel from a pole into 1e-3 texels or more; atan2 of the two legs is conditioned like the angle itself)
 *     bw = (2 half_w tile_width) / 5;  x mod 5 = x - 5 floorf(x / 5), a result outside [0, 5) -> 0;  bidx = min(floorf(t), 4), f = t - bidx
 *     v < 1/3  (south caps):  s = 3 v;      t = 5 u mod 5;              bidy = 0;  by = f bw s;  bx = by + bw (1 - s)
 *     v < 2/3  (mid bands):   w = 3 v - 1;  t = (5 u - 0.5 w) mod 5;    bx = f bw;  f <= 1 - w: bidy = 0, by = bx + w bw;
 *                                                                                   else:       bidy = 1, by = bx - bw (1 - w)
 *     else     (north caps):  s = 3 v - 2;  t = (5 u - 0.5) mod 5;      bidy = 1;  bx = f bw (1 - s);  by = bx + s bw
 *     p = ((center_coord - map_half_wh) tile_width) + (bidx bw + bx, bidy bw + by)      the origin map_sphere_surface subtracts
 *     uv = p / tile_width / 4, as in the plane pass.
 *   Texture LOD, free of the unfolding's seams and of the pinch at the poles: the rays of pixels (x + 1, y) and (x, y + 1) are cut with the
 *     same sphere at the same root, disc clamped at 0 (a neighbour that misses at the silhouette takes its closest point) -> hx, hy;
 *     rho = max(|hx - hit|, |hy - hit|) * k,  k = (half_w * tex_size) / ((4 PI) * r): texels per world unit at the equator;
 *     lod = clamp(log2f(rho), 0, n_mips - 1); trilinear Repeat taps and `brightness` as in gswt_proxy_render.
 *   Shade and fog: gswt_set_shadow_map's lookup at the world hit point, then gswt_set_atmosphere's fog, order and formulas as in the plane
 *     passes; dist = t * sqrtf(dd) (projection 0) or |hit - cam_pos| (projection 1).  The depth written does not depend on either.
 * Out of scope: a height-mapped sphere (the Sphere surface has no height map); a sphere mode of the CPU oracle's proxy_render; any change to
 * what gswt_proxy_render does with surface_type == 2; the bench workloads. */
GSWT_API int gswt_proxy_render_sphere(gswt_ctx *ctx, const gswt_proxy_uniforms *u, float sphere_radius, int projection, int width, int height,
                                      float *rgba_dev, float *depth_dev, int clear_depth);


/* Number of pixel rows the shard (index, count) owns for a frame of `height` rows. */
GSWT_API int gswt_shard_rows(int height, int shard_index, int shard_count);
/* Scatter `shard_count` gathered shard images (concatenated in shard order, as an
 * all-gather delivers them; each padded to gswt_shard_rows_padded rows) back into a full
 * H x W frame.  Device pointers; runs on the ctx stream. */
GSWT_API int gswt_shard_rows_padded(int height, int shard_count);
/* Width in pixels of every rank's shard image in GSWT_SHARD_COLUMNS mode (ceil(tiles_x / shard_count) * 16). */
GSWT_API int gswt_shard_cols_padded(int width, int shard_count);
GSWT_API int gswt_unshard(gswt_ctx *ctx, const float *gathered, int width, int height,
                          int shard_count, float *out_rgba);
/* The same for either shard mode (GSWT_SHARD_COLUMNS: the gathered shards are H x gswt_shard_cols_padded images). */
GSWT_API int gswt_unshard_mode(gswt_ctx *ctx, const float *gathered, int width, int height,
                               int shard_count, int shard_mode, float *out_rgba);
/* The same for any output format (GSWT_OUT_*: 16 or 4 bytes per pixel; GSWT_VIDEO_*: every shard a complete image of planes, reassembled
 * plane by plane, width and height even); gswt_unshard_mode is out_format = GSWT_OUT_RGBA32F of it. */
GSWT_API int gswt_unshard_format(gswt_ctx *ctx, const void *gathered, int width, int height,
                                 int shard_count, int shard_mode, int out_format, void *out);

/* ---- multi-GPU: the framebuffer all-gather behind the ABI (new; the reference is single-GPU) ---------------------
 * One ctx per GPU.  Every rank renders its shard (cfg->shard_index = rank, shard_count = world) with gswt_render_async,
 * then gswt_render_gather(ticket, frame) = overflow-safe fence + all-gather of the equal-sized shard images + the index
 * permutation of gswt_unshard_mode, all on the ctx stream: `frame` (W*H*4 f32, device) then holds the whole image on
 * every rank.  A gather moves the image in the format its frame was rendered in (cfg->out_format: W*H*4 bytes for the 8-bit
 * formats); in a group gather every rank's frame must have the same format (GSWT_ERR_BAD_ARG otherwise).  Two transports:
 *   RCCL (one process per GPU, xGMI): rank 0 calls gswt_comm_unique_id, ships the 128 bytes to the other ranks by any
 *     means (MPI, a file, torch.distributed ...), every rank calls gswt_comm_init(ctx, id, rank, world) ->
 *     ncclCommInitRank; the gather is one ncclAllGather.  librccl is loaded on first use (dlopen), so a single-GPU host
 *     does not need it; GSWT_ERR_RCCL reports a missing library or a failed collective.
 *   hipMemcpyPeerAsync (all GPUs in ONE process, no RCCL): gswt_group_init binds n contexts into a group;
 *     gswt_group_render_gather pushes every rank's shard into every peer's gather buffer (n x n peer copies), orders the
 *     peers' streams behind them with events and runs the permutation on each.  Also what the single-GPU tests use
 *     (several contexts on one device). */
#define GSWT_COMM_ID_BYTES 128
GSWT_API int gswt_comm_unique_id(void *id_out /* GSWT_COMM_ID_BYTES */);
GSWT_API int gswt_comm_init(gswt_ctx *ctx, const void *unique_id, int rank, int world);
GSWT_API int gswt_comm_destroy(gswt_ctx *ctx);
GSWT_API int gswt_render_gather(gswt_ctx *ctx, int ticket, float *frame_out_dev);
GSWT_API int gswt_group_init(gswt_ctx *const *ctxs, int n);          /* rank r = ctxs[r]; undone by gswt_comm_destroy on each */
GSWT_API int gswt_group_render_gather(gswt_ctx *const *ctxs, const int *tickets, float *const *frames_out_dev, int n);


/* ---- SortData: what one sort event hands from the worker to the renderer --------------- */
/* One element of SortData.tile_instance_vec + render_data_vec (structure.rs:488-509,670-694). */
typedef struct {
    uint32_t lod, tile, view_id;      /* tid.0, tid.1, view_id                                   */
    float tile_offset[3];
    uint32_t map_index;
    uint32_t map_coord[2];
    float tile_center[3];
    int32_t transition;               /* 0 None, 1 Spawning, 2 Changing(false), 3 Changing(true)   */
    float spawning_factor;
    uint32_t has_corners;
    float corners[12];                /* corner_data[ci].0                                        */
    uint32_t key_len;                 /* render_data_key.tid.len()                                */
    uint32_t merged;                  /* Some(render_data_value)                                  */
    uint32_t merged_offset;           /* into the concatenated merged arrays of gswt_sort_data    */
    uint32_t merged_count;
    int32_t single_lod_id;
    uint32_t cache_hit;               /* value came from the LRU cache (wangtile.rs:575-593)      */
    uint32_t merged_group;            /* index into gswt_sort_data.groups when merged               */
} gswt_sorted_tile;

typedef struct {
    uint32_t scene_id;
    uint32_t n_tiles;
    const gswt_sorted_tile *tiles;    /* back-to-front */
    size_t n_merged;
    const uint32_t *merged_gs_index, *merged_map_id, *merged_lod_id;   /* NULL in device-merge mode */
    /* group descriptions for gswt_set_draws_merge_groups (always filled) */
    uint32_t n_groups, n_members;
    const gswt_merge_group *groups;
    const gswt_merge_member *members;
} gswt_sort_data;


/* ---- Device-side worker stages: update_lod, selective merging, the four tile orders and the presort-view
 * choice of WangTile (wangtile.rs:476-690,720-1218,1496-1607) as HIP kernels.  The tile MAP itself (update_tile_map,
 * :1671-1781: map shift, tile ids from the RNG, centres / corners / edges through surface_mapping) stays in libgswt_host and
 * is handed over once per build event as gswt_cell[]; every per-sort-event stage then runs on the device and leaves a
 * gswt_sort_data (device-merge form: group descriptions, no CPU lists) that is byte-identical to gswt_wang_sort_tiles'. */

/* One map cell, TileInstance as update_tile_map leaves it (structure.rs:495-509); index = x * map_h + y. */
typedef struct {
    uint32_t tile;             /* tid.1 */
    uint32_t has_corner;
    float tile_offset[3];
    float tile_center[3];
    float to_local[9];         /* column-major Matrix3 */
    float corner_pos[12];      /* corner_data[ci].0 */
    float corner_up[12];       /* corner_data[ci].1 column 2 (surface normal at the corner) */
    float edge_pos[12];        /* edge_data[ei].0 */
    float edge_normal[12];     /* edge_data[ei].1 */
} gswt_cell;                   /* 260 bytes */

/* Per-cell results of update_lod and of selective merging (the TileInstance fields those stages write). */
typedef struct {
    uint32_t lod;
    int32_t transition;        /* 0 None, 1 Spawning, 2 Changing(false), 3 Changing(true) */
    float spawning_factor;
    uint32_t merge;            /* 0 None, 1 MergedFrom (group head), 2 MergedTo */
    uint32_t merged_to;        /* map index of the head when merge == 2 */
} gswt_cell_state;

/* UserData fields the stages read plus the tables preprocess / configure leave behind.  Filled by
 * gswt_wang_worker_config (pointers borrowed from the gswt_wang); gswt_worker_create copies everything to the device. */
typedef struct {
    uint32_t map_w, map_h, half_w, half_h;
    uint32_t n_lod, n_tile, n_view;
    float tile_width;
    uint32_t surface_type, tile_sort_type, merge_type;
    float height_map_scale[3];
    float sphere_radius;
    uint32_t lod_blending, lod_bbox_check;
    float lod_transition_width_ratio, lod_dist_tolerance;
    int32_t merge_tile_dist[2];
    float merge_dot_threshold;
    uint32_t merge_topk;
    uint32_t hm_w, hm_h;
    const float *height_map;          /* hm_w * hm_h, or NULL */
    const float *lod_transition_dist; /* n_lod */
    const float *tile_center;         /* n_tile * 3 */
    const float *tile_aabb;           /* n_tile * 6: lo.xyz, hi.xyz */
    const uint32_t *splat_count;      /* n_lod * n_tile: raw_depth lengths */
    const float *presort_dirs;        /* n_view * 3 */
    const int32_t *neighbors;         /* map_w * map_h * 4 slots (W, N, E, S): neighbour map index << 2 | its slot for us, or -1 */
} gswt_worker_config;

typedef struct gswt_worker gswt_worker;
/* Lives on ctx's device with a stream of its own (the reference's worker is a thread of its own, state.rs:478-561).
 * GSWT_ERR_CAPACITY: maps beyond 32 767 cells (u16 ids), or beyond 17 749 cells with Edge merging (its LDS tables). */
GSWT_API int gswt_worker_create(gswt_ctx *ctx, const gswt_worker_config *cfg, gswt_worker **out);
GSWT_API void gswt_worker_destroy(gswt_worker *w);
GSWT_API const char *gswt_worker_last_error(const gswt_worker *w);
/* After every build event on the host (update_tile_map): the whole map and its centre coordinate. */
GSWT_API int gswt_worker_set_cells(gswt_worker *w, const gswt_cell *cells, size_t n_cells, const int32_t center_coord[2]);
/* update_lod (wangtile.rs:1496-1607): LOD, transition status and spawning factor of every cell. */
GSWT_API int gswt_worker_update_lod(gswt_worker *w, const float cam_pos[3]);
/* sort_tiles (wangtile.rs:476-690): merge, order, views, records.  Enqueued on the worker's stream. */
GSWT_API int gswt_worker_sort_tiles(gswt_worker *w, const float cam_pos[3], const float view_proj16[16]);
/* Threads: every gswt_worker_* call belongs to ONE thread (the reference's worker thread); gswt_set_draws_from_worker belongs to
 * the ctx's thread.  The two meet in three host-side result sets: gswt_worker_fetch waits for the worker's stream, copies the
 * records, group descriptions and draws of the last sort event into a free set and publishes it; gswt_set_draws_from_worker
 * takes the set published last (GSWT_ERR_STATE if there is none yet).  Neither waits for the other. */
GSWT_API int gswt_worker_fetch(gswt_worker *w);
/* Test hooks (worker thread, blocking).  read_sort fetches if needed; its pointers stay valid for two further fetches. */
GSWT_API int gswt_worker_read_cell_state(gswt_worker *w, gswt_cell_state *out, size_t capacity);
GSWT_API int gswt_worker_read_sort(gswt_worker *w, gswt_sort_data *out);
/* Swap-in (state.rs:521-540 + renderer.rs:466-591 host half): the draws were built on the device (TileUniforms, list
 * selection, cull inputs per record); this runs gswt_set_draws_merge_groups' planning on the published set.  ctx must be the
 * worker's ctx; a failure's text is in gswt_last_error(ctx). */
GSWT_API int gswt_set_draws_from_worker(gswt_ctx *ctx, gswt_worker *w);

GSWT_API int gswt_synchronize(gswt_ctx *ctx);
GSWT_API int gswt_last_timings(const gswt_ctx *ctx, gswt_timings *out);

/* Test / profiling hook: per-splat vertex-stage output of the last gswt_render, one
 * 48-byte record per list entry in draw order (visible, ndc.xy, depth, major.xy,
 * minor.xy, rgba) -- the varyings of vs_main (gswt.wgsl:4-8,412-419). Host pointer. */
GSWT_API int gswt_debug_read_projected(gswt_ctx *ctx, void *out, size_t capacity_entries,
                                       size_t *n_entries);

/* Test hook: k_totals alone -- folds n_super (pair, visible) super-group sums into the frame counters {visible, pairs, -,
 * overflow flag} (64-bit) and the exclusive pair prefix per super-group (u32).  Host pointers. */
GSWT_API int gswt_debug_totals(gswt_ctx *ctx, const uint32_t *pair_sums, const uint32_t *visible_sums, uint32_t n_super,
                               uint32_t pair_cap, unsigned long long counters_out[4], uint32_t *super_excl_out);

/* Test hook: the frame's stable LSD radix sort alone (k_radix_hist / k_radix_supscan / k_radix_scatter) on the low `key_bits` bits
 * of n (key, value) pairs, in place.  Equal keys keep their input order (the order contract of scene.rs:685-695 rests on it).
 * Host pointers. */
GSWT_API int gswt_debug_sort(gswt_ctx *ctx, uint32_t *keys, uint32_t *vals, size_t n, int key_bits);

/* Test hook: the same sort driven the way a frame drives it.  keys, vals and (optional) aux: n_cap words each, copied in full into BOTH
 * ping-pong buffers, so that after any number of passes every word the sort did not write is still the caller's.  n: the item count the
 * kernels read on the device -- 0, below n_cap, or above it; overflow: the frame's overflow flag beside it (either of the last two makes
 * the sort process nothing).  aux: a second payload carried with the vals (the tile ids of the depth passes).  use_krange: the key range
 * {~krange_min, krange_max} is uploaded and the digits are taken from key - krange_min; the caller keeps every key inside the range and
 * krange_max - krange_min < 2^key_bits (in a frame k_items flags a range that needs more passes).  ranges_out (n_range_keys x 2 words,
 * optional; every key < n_range_keys): a zeroed table goes to the last pass, which leaves every key's slice of the sorted list there and
 * writes no keys; returned decoded like gswt_debug_read_ranges, (start, end), (0, 0) for an absent key.  threads: 0 = the sort's own
 * choice, else 256 or 512 per workgroup; aux_form: 0 = its own choice, else payload form 1 or 2 (only with aux).
 * On return vals and aux hold all n_cap words of the final buffers, keys too unless ranges_out is set.  Host pointers. */
GSWT_API int gswt_debug_sort_ex(gswt_ctx *ctx, uint32_t *keys, uint32_t *vals, uint32_t *aux, size_t n_cap, unsigned long long n, int overflow,
                                int key_bits, int use_krange, uint32_t krange_min, uint32_t krange_max, uint32_t *ranges_out,
                                size_t n_range_keys, int threads, int aux_form);

/* Test hook: the tile-local depth sort of GSWT_ORDER_DEPTH alone (k_tile_depth_sort).  lens[t] = length of screen tile t's slice of the pair
 * list (the slices lie back to back, n = their sum); every slice's vals are sorted by its dkeys, stably, in place (any length: slices of
 * more than 16 384 pairs go through k_tile_depth_sort_xl).  *flagged_out: the frame-level error flag of the kernels (0).  Host pointers. */
GSWT_API int gswt_debug_tile_depth_sort(gswt_ctx *ctx, const uint32_t *lens, size_t n_tiles, uint32_t *vals, const uint32_t *dkeys, size_t n,
                                        int *flagged_out);

/* GSWT_OPT_GRAPH bookkeeping since gswt_create: {frames replayed through hipGraphLaunch, graphs (re)built, kernel nodes updated}. */
GSWT_API int gswt_debug_graph_stats(const gswt_ctx *ctx, unsigned long long out[3]);

/* Merged groups sorted / copied from a retained earlier sort event by gswt_set_draws_merge_groups since gswt_create. */
GSWT_API int gswt_debug_merge_stats(const gswt_ctx *ctx, unsigned long long out[2]);
/* ... and how many of the copied ones came from an event OLDER than the previous one (the lists of the last 9 events stay addressable by
 * (view, ordered member tile ids, transition states): the reference's 1 024-entry LRU of merged lists, wangtile.rs:427,575-593). */
GSWT_API int gswt_debug_merge_stats_deep(const gswt_ctx *ctx, unsigned long long *out);

/* Test / profiling hook: [start, end) of every screen tile in the sorted pair list of the last
 * gswt_render (2 u32 per tile, shard-local tile order). Host pointer. */
GSWT_API int gswt_debug_read_ranges(gswt_ctx *ctx, uint32_t *out, size_t capacity_tiles, size_t *n_tiles);
/* Test hook: the sorted pair list the compositor of the last gswt_render walked (the list gswt_debug_read_ranges' slices index), one u32
 * per pair: the pair's list entry in draw order (gswt_debug_read_projected's index), resolved on the host from its slot as k_pick_resolve
 * does -- draw = chunk table[slot >> 8], entry = entry_base + (count - 1 - (slot - slot_base)); 0xFFFFFFFF for a slot that names no entry.
 * out = NULL: only *n_pairs.  Needs no GSWT_OPT_DEBUG_VARYINGS.  GSWT_ERR_STATE before any frame, and while the last frame submitted
 * through gswt_render_async has not been waited for (an overflowed frame is only re-run by the wait).  Host pointer. */
GSWT_API int gswt_debug_read_pairs(gswt_ctx *ctx, uint32_t *out, size_t capacity_pairs, size_t *n_pairs);
/* GSWT_ORDER_DEPTH bookkeeping: out[0] = frames enqueued on the tile-local path (k_tile_depth_sort), [1] = on the global depth passes
 * (re-runs count), [2] = the longest screen-tile pair list of the last finished depth-ordered frame. */
GSWT_API int gswt_debug_depth_stats(const gswt_ctx *ctx, unsigned long long out[3]);
/* Device timeline of two frame slots (tests of the frame / gather overlap): out_ms[0] = start of slot `ticket`'s frame kernels, [1] = their
 * end, [2] = end of its gather + re-assembly (NaN if it was not gathered), in ms after the START of slot `ticket_ref`'s frame.  Both frames
 * submitted with GSWT_OPT_TIMING >= 1 and complete (the call synchronises). */
GSWT_API int gswt_debug_frame_times(gswt_ctx *ctx, int ticket_ref, int ticket, float out_ms[3]);

#ifdef __cplusplus
}
#endif
#endif /* GSWT_HIP_H */
