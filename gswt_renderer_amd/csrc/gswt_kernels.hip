// gswt_kernels.hip -- hand-written CDNA4 (gfx950) kernels of the GSWT hot path.
//
//   k_cull        : per-draw viewport cull + lod_enable skip (renderer.rs:472-497), column-band cull; clears the frame counters
//   k_project     : Wang-tile instancing + vs_main (gswt.wgsl:27-422) per list entry: None / HeightMap / Sphere surface,
//                   LOD blend, EWA projection, debug draw modes; <STRICT> (default) evaluates the shader text operator by operator
//   k_totals/k_emit : (splat, 16x16 screen tile) pair emission in composite order, no scan launches; k_emit<DEPTH> also keys every
//                   pair with its splat's depth bits (GSWT_ORDER_DEPTH: the global radix depth sort)
//   radix sort    : stable LSD sort of the pairs on the tile bits (reference order), preceded by passes on the depth bits in use with
//                   the tile id as payload (depth order); k_mg_* : merged-group lists on the device
//   k_items       : work items (tile, segment of its list: GSWT_OPT_SEGMENT pairs) from the per-tile [start, end) the last pass leaves
//   k_composite   : front-to-back alpha compositing (fs_main gswt.wgsl:425-435 + blend/depth state
//                   renderer.rs:118-129,179-185): LDS-staged batches, per-sub-block lists, wave ballot early termination
//   k_combine     : folds the segment partials of long tile lists; k_unshard : all-gathered shards -> frame
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off.  Contraction is OFF for the
// whole file: the float sequences that feed discontinuous decisions (culling, |p|^2 <= 4,
// depth test) are the canonical sequences of DESIGN.md and must round exactly like the
// CPU oracle; every fused multiply-add below is an explicit fmaf().
// Wavefront = 64 lanes everywhere in this file.
// What other kernel files use too (lane masks, half decode, the height map's sampler) is in gswt_device_fn.h; what the host computes
// as well (canonical sin / cos, the sphere unfolding, the height-map coordinates) is gswt_host:: of host/gswt_surface.h, one source.
#include "gswt_device_fn.h"
#include "gswt_variant.h"

namespace gswt {

// Wave-wide scans and sums through DPP (data-parallel primitives: the neighbour's register arrives with the VALU instruction) instead of
// __shfl_up / __shfl_down, which compile to ds_bpermute_b32 -- an LDS-crossbar round trip per step, six of them in a dependent chain per
// scan.  row_shr:1 / 2 / 4 / 8 make the inclusive scan of every 16-lane row (a lane whose source lies outside its row adds 0),
// row_bcast:15 on rows 1 and 3 adds the row in front, row_bcast:31 on rows 2 and 3 the first half of the wave: the GFX9 sequence of
// rocPRIM's warp scan.  Every lane of the wave must be active (it was so with the shuffles: a lane that has left reads as undefined there).
// Integer adds: the same values bit for bit.  (End of round 4: the scans of k_radix_scatter / k_emit / k_items / k_totals / the tile-local
// depth sort and the sums of k_project; profiles/r04_dpp_scans.txt.)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_or_zero(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROW_MASK, 0xF, true);
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane)
{
    (void)lane;
    v += dpp_or_zero<0x111, 0xF>(v);          // row_shr:1
    v += dpp_or_zero<0x112, 0xF>(v);          // row_shr:2
    v += dpp_or_zero<0x114, 0xF>(v);          // row_shr:4
    v += dpp_or_zero<0x118, 0xF>(v);          // row_shr:8
    v += dpp_or_zero<0x142, 0xA>(v);          // row_bcast:15 -> rows 1, 3
    v += dpp_or_zero<0x143, 0xC>(v);          // row_bcast:31 -> rows 2, 3
    return v;
}
// the wave's smallest / largest value, in every lane (uniform): the same six DPP steps with min / max; a lane whose source lies outside its row
// (or whose row the step does not address) compares with itself
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_or_self(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
    v = min(v, dpp_or_self<0x111, 0xF>(v)); v = min(v, dpp_or_self<0x112, 0xF>(v)); v = min(v, dpp_or_self<0x114, 0xF>(v));
    v = min(v, dpp_or_self<0x118, 0xF>(v)); v = min(v, dpp_or_self<0x142, 0xA>(v)); v = min(v, dpp_or_self<0x143, 0xC>(v));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    v = max(v, dpp_or_self<0x111, 0xF>(v)); v = max(v, dpp_or_self<0x112, 0xF>(v)); v = max(v, dpp_or_self<0x114, 0xF>(v));
    v = max(v, dpp_or_self<0x118, 0xF>(v)); v = max(v, dpp_or_self<0x142, 0xA>(v)); v = max(v, dpp_or_self<0x143, 0xC>(v));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// the wave's sum, in every lane (uniform: a scalar register)
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(v, 0u), 63);
}

// rand(), gswt.wgsl:502-504 (the canonical sin of DESIGN.md section 4: host/gswt_surface.h)
__device__ __forceinline__ float dbg_rand(float cx, float cy)
{
    const float d = cx * 12.9898f + cy * 78.233f;
    float sn, cs;
    gswt_host::csincosf(d, sn, cs);
    const float v = sn * 43758.5453f;
    return v - floorf(v);
}

// Debug draw recolouring, gswt.wgsl:268-399 (draw_mode 1..4); rgb in / out
__device__ __forceinline__ void debug_draw_color(const Frame& f, const DrawDev& d, float vx, float vy, uint32_t lod_id, float t_ratio,
                                                 float& cr, float& cg, float& cb)
{
    const float tw = f.tile_width;
    if (f.draw_mode == 1u) {
        const float g = clampf(((cr + cg) + cb) / 0.6f, 0.0f, 1.0f);
        cr = cg = cb = g;
        const float margin = 0.05f * tw;
        const bool sphere = f.surface_type == 2u;
        if (d.single_draw == 1u) {
            cr = cr * dbg_rand(d.off[0], d.off[1]);
            cg = cg * dbg_rand(d.off[0] + 23.45f, d.off[1] + 23.45f);
            cb = cb * dbg_rand(d.off[0] + 67.89f, d.off[1] + 67.89f);
        } else if (vx < margin || vx > tw - margin) {
            const uint32_t bit = vx < margin ? d.tile_idx / 8u % 2u : d.tile_idx / 2u % 2u;
            if (vy < margin || vy > tw - margin) { cr = cg = cb = 0.5f; }
            else if (bit == 0u) { cr = 1.0f; cg = 0.0f; cb = 0.0f; }
            else { cr = 0.0f; cg = 1.0f; cb = 0.13f; }
        } else if (vy < margin || vy > tw - margin) {
            const uint32_t bit = vy < margin ? d.tile_idx % 2u : d.tile_idx / 4u % 2u;
            if (bit == 0u) {
                if (sphere) { cr = 1.0f; cg = 0.0f; cb = 0.0f; } else { cr = 1.0f; cg = 0.85f; cb = 0.0f; }
            } else {
                if (sphere) { cr = 0.0f; cg = 1.0f; cb = 0.13f; } else { cr = 0.0f; cg = 0.58f; cb = 1.0f; }
            }
        }
    } else if (f.draw_mode == 2u || f.draw_mode == 3u) {
        if (t_ratio > 0.0f && t_ratio < 1.0f) { cr = cg = cb = 0.0f; return; }
        if (f.draw_mode == 2u && d.changing == 1u) { cr = 0.0f; cg = 1.0f; cb = 0.0f; return; }
        uint32_t L = d.tile_lod;
        if (f.draw_mode == 3u) L = d.single_lod_id >= 0 ? (uint32_t)d.single_lod_id : lod_id;
        float cx = 0.0f, cy = 1.0f;
        if (L < 3u) cx = (3.0f - (float)L) / 3.0f;
        else cy = (6.0f - (float)L) / 3.0f;
        cr = 0.5f; cg = cx; cb = cy;
    } else if (f.draw_mode == 4u) {
        const uint32_t v = d.tile_view;
        float cx = 0.0f, cy = 0.0f;
        if (v < 4u) cx = (4.0f - (float)v) / 4.0f;
        if (v >= 4u) cy = (8.0f - (float)v) / 4.0f;
        if (v >= 8u) { cx = 1.0f; cy = 1.0f; }
        cr = 0.5f; cg = cx; cb = cy;
    }
}

// Screen tile id -> (column, row) of this ctx's tile grid.  The id is uniform per workgroup: for ids and widths below 2^16 the quotient is
// the high word of id * (floor(2^32 / tiles_x) + 1) -- one scalar multiply instead of the ~25 vector instructions of a 32-bit division
// that every wave of k_composite / k_combine used to spend on it (exact: the error of the product stays below 2^-16 <= 1 / tiles_x).
__device__ __forceinline__ void tile_xy(const Frame& f, uint32_t tile, int& tx, int& ty)
{
    uint32_t q;
    if (f.tiles_x_magic != 0u && tile < 65536u) q = __umulhi(tile, f.tiles_x_magic);
    else q = tile / (uint32_t)f.tiles_x;
    tx = (int)(tile - q * (uint32_t)f.tiles_x); ty = (int)q;
}

// Number of 16-px tile rows in [ty0, ty1] owned by this shard (row % count == index).
__device__ __forceinline__ int owned_rows(int ty0, int ty1, int index, int count)
{
    if (count <= 1) return ty1 - ty0 + 1;
    // first owned row >= ty0
    int first = ty0 + ((index - ty0 % count) + count) % count;
    if (first > ty1) return 0;
    return (ty1 - first) / count + 1;
}

// Chunk tables of a draw set, written on the device from the draw records (per sort event): a chunk = 256 list entries of
// one draw.  chunk_tab is in slot order (chunk c = slots c * 256 ...); chunk_tab_xcd is k_project's launch order: the
// chunks of draw d sit in the list of XCD d % 8, lists interleaved so that launch position p runs on XCD p % 8 (short
// lists are padded with 0xFFFFFFFF by the eight extra workgroups at the end of the grid).  One workgroup per draw.
struct XcdLens { uint32_t len[8]; uint32_t longest; };
__global__ __launch_bounds__(256) void k_chunk_tabs(const DrawDev* __restrict__ draws, const uint32_t* __restrict__ xcd_first, uint32_t n_draws,
                                                    uint2* __restrict__ chunk_tab, uint2* __restrict__ chunk_tab_xcd, const XcdLens xl)
{
    const uint32_t d = blockIdx.x;
    if (d >= n_draws) {
        const uint32_t x = d - n_draws;              // 0..7: padding of XCD x's list up to the longest one
        for (uint32_t k = xl.len[x & 7u] + threadIdx.x; k < xl.longest; k += 256u) chunk_tab_xcd[(size_t)k * 8u + x] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        return;
    }
    const uint32_t nch = (draws[d].count + (uint32_t)kChunk - 1u) / (uint32_t)kChunk;
    const uint32_t c0 = draws[d].slot_base / (uint32_t)kChunk, x0 = xcd_first[d];
    for (uint32_t k = threadIdx.x; k < nch; k += 256u) {
        const uint2 e = make_uint2(d, k * (uint32_t)kChunk);
        chunk_tab[c0 + k] = e;
        chunk_tab_xcd[(size_t)(x0 + k) * 8u + (draws[d].xcd & 7u)] = e;
    }
}

// ------------------------------------------------------------------------------------
// k_cull: the CPU viewport culling + lod_enable skip of renderer.rs:472-497, one thread per draw.
// ------------------------------------------------------------------------------------
// Column-band sharding: can any splat whose centre lies in the box [lo, hi] (world space, before scene_scale) reach this
// rank's pixel columns?  Conservative: the centres lie in the convex hull of the 8 projected box corners (all in front of
// the camera, else keep), and a splat's pixel half extent is <= 2 s sqrt(lambda1) with lambda1 <= |J|_F^2 max(scene_scale)^2
// trace(Vrk) at the nearest depth, capped by the 1024-px axis clamp (gswt.wgsl:257-258); 25 % + 2 px of slack on top.
// lo / hi: bounds of the splat centres BEFORE scene_scale and surface mapping (cell origin + the scene's tile-local bounds).
// HeightMap surface (gswt.wgsl:565-599): the mapped centre is (x, y, h(x, y) hz) + n z with |n| = 1, so x and y move by at most
// |z| and the height lies in [surf_zlo - |z|, surf_zhi + |z|]; the covariance is F Vrk F^T, lambda1 <= |F|_F^2 trace(Vrk).
// Sphere surface: sphere_cell_box above (bidx, bidy: the block of the draw's cell; unused elsewhere).
// Sphere surface (gswt.wgsl:515-564, 600-623): a splat centre is lz (R + z), lz = the unit vector of the strip parametrisation at the
// centre's block coordinates (bx, by).  Inside one block, 0 <= bx, by <= block_w, that map is continuous (also across the block's
// diagonal and at the pole) and |d lz| <= K (|d bx| + |d by|) / block_w with K = max(0.2 pi + pi / 3, 2 pi^2 / 15 + pi / 3) = 2.363
// (equatorial triangles: u, v linear; polar triangles: cos v <= pi (block_w - t) / (3 block_w) against |du| <= 2 pi / (5 (block_w - t))):
// the centres of a cell lie within rho = R K (w + h) / (2 n block_w) + max |z| of the lz R of n x n sample points of its footprint.
// K = 2.5 and 2 % on rho are the slack for the +-0.001 y_max taps of F and the rounding of the evaluation.  A footprint that leaves
// its block (cells astride a block seam) is not bounded: such cells are kept.  lo / hi: scaled flat bounds; out: bounds of the centres.
__device__ __forceinline__ bool sphere_cell_box(const Frame& f, float bidx, float bidy, const float lo[3], const float hi[3], float blo[3], float bhi[3])
{
    const float xmax = ((float)f.map_half_wh[0] * 2.0f) * f.tile_width;
    const float block_w = xmax / 5.0f;
    const float ox = (float)(f.center_coord[0] - (int32_t)f.map_half_wh[0]) * f.tile_width + bidx * block_w;
    const float oy = (float)(f.center_coord[1] - (int32_t)f.map_half_wh[1]) * f.tile_width + bidy * block_w;
    const float bx0 = lo[0] - ox, bx1 = hi[0] - ox, by0 = lo[1] - oy, by1 = hi[1] - oy;
    if (!(block_w > 0.0f && bx0 >= 0.0f && bx1 <= block_w && by0 >= 0.0f && by1 <= block_w)) return false;
    constexpr int n = 3;
    const float R = fabsf(f.sphere_radius);
    const float zmax = fmaxf(fabsf(lo[2]), fabsf(hi[2]));
    const float rho = (R * 2.5f * ((bx1 - bx0) + (by1 - by0)) / (2.0f * (float)n * block_w) + zmax) * 1.02f + 1e-4f * R;
    if (!(rho == rho)) return false;
    for (int k = 0; k < 3; k++) { blo[k] = 3.402823466e+38f; bhi[k] = -3.402823466e+38f; }
    for (int j = 0; j < n; j++)
        for (int i = 0; i < n; i++) {
            const gswt_host::V3 pt = gswt_host::sphere_point(block_w, bidx, bidy, bx0 + (bx1 - bx0) * (((float)i + 0.5f) / (float)n),
                                                             by0 + (by1 - by0) * (((float)j + 0.5f) / (float)n));
            const float p[3] = {pt.x, pt.y, pt.z};
            for (int k = 0; k < 3; k++) { blo[k] = fminf(blo[k], p[k] * f.sphere_radius - rho); bhi[k] = fmaxf(bhi[k], p[k] * f.sphere_radius + rho); }
        }
    return blo[0] == blo[0] && bhi[0] == bhi[0] && blo[1] == blo[1] && bhi[1] == bhi[1] && blo[2] == blo[2] && bhi[2] == bhi[2];
}

__device__ __forceinline__ bool band_misses(const Frame& f, const float lo[3], const float hi[3], float bidx, float bidy)
{
    float blo[3], bhi[3];
    for (int k = 0; k < 3; k++) {
        const float a = lo[k] * f.scene_scale[k], b = hi[k] * f.scene_scale[k];
        blo[k] = fminf(a, b); bhi[k] = fmaxf(a, b);
    }
    if (f.surface_type == 1u) {
        const float zp = fmaxf(fabsf(blo[2]), fabsf(bhi[2])) * 1.0001f;
        blo[0] -= zp; bhi[0] += zp; blo[1] -= zp; bhi[1] += zp;
        blo[2] = f.surf_zlo - zp; bhi[2] = f.surf_zhi + zp;
    } else if (f.surface_type == 2u) {
        float slo[3], shi[3];
        if (!sphere_cell_box(f, bidx, bidy, blo, bhi, slo, shi)) return false;
        for (int k = 0; k < 3; k++) { blo[k] = slo[k]; bhi[k] = shi[k]; }
    }
    float xmin = 3.402823466e+38f, xmax = -3.402823466e+38f, wmin = 3.402823466e+38f;
    bool odd = false;                 // a NaN anywhere: keep (fminf / fmaxf drop NaN operands, so the extremes alone would not show it)
    for (int k = 0; k < 8; k++) {
        const float px = (k & 1) ? bhi[0] : blo[0];
        const float py = (k & 2) ? bhi[1] : blo[1];
        const float pz = (k & 4) ? bhi[2] : blo[2];
        const float cx = ((f.VP[0] * px + f.VP[4] * py) + f.VP[8] * pz) + f.VP[12];
        const float cw = ((f.VP[3] * px + f.VP[7] * py) + f.VP[11] * pz) + f.VP[15];
        wmin = fminf(wmin, cw);
        const float xp = (0.5f * (cx / cw) + 0.5f) * f.W;
        odd = odd || !(cw == cw) || !(xp == xp);
        xmin = fminf(xmin, xp); xmax = fmaxf(xmax, xp);
    }
    if (odd || !(wmin > 1e-6f && xmin == xmin && xmax == xmax)) return false;
    const float smax = fmaxf(fabsf(f.scene_scale[0]), fmaxf(fabsf(f.scene_scale[1]), fabsf(f.scene_scale[2])));
    const float hx = 1.3f * f.htan[0], hy = 1.3f * f.htan[1];
    const float jn2 = (f.focal[0] * f.focal[0] * (1.0f + hx * hx) + f.focal[1] * f.focal[1] * (1.0f + hy * hy)) / (wmin * wmin);
    // (GSWT_OPT_ANTIALIAS: the pixel filter adds aa_s to both eigenvalues of cov2d; the 1024 clamp applies after it, so the cap below stays)
    const float lam = jn2 * smax * smax * fmaxf(f.loc_max_trace, 0.0f) * f.surf_f2 + f.aa_s;
    const float ss = fabsf(f.splat_scale);
    const float rad = fminf(2.0f * ss * sqrtf(lam), 1448.2f * ss) * 1.25f + 2.0f;
    if (!(rad == rad)) return false;
    return xmax + rad < (float)(f.col0 * kTile) || xmin - rad >= (float)(f.col1 * kTile);
}

// The CPU viewport culling + lod_enable skip of renderer.rs:472-497 for one draw (+ the band cull of a column-band shard).
// Band culling works on MAP CELLS: every splat of a Wang-tile instance lies in (cell origin + the scene's tile-local position
// bounds), f.loc_lo .. f.loc_hi, so a plain / blending draw is tested with its own offset and the members of a merged group
// through cell_culled[map id] (k_project skips such entries before gathering their records): the heaviest band no longer
// projects whole merged groups that merely touch it.  No per-sort-event bounds pass.
__device__ __forceinline__ bool draw_is_culled(const Frame& f, const DrawDev& d)
{
    bool culled = false;
    if (d.cull_enable) {
        float mx = 3.402823466e+38f, my = 3.402823466e+38f, mz = -3.402823466e+38f;
        for (int ci = 0; ci < 4; ci++) {
            float px = d.corners[3 * ci], py = d.corners[3 * ci + 1], pz = d.corners[3 * ci + 2];
            float c4[4];
            for (int r = 0; r < 4; r++)
                c4[r] = ((f.VP[r] * px + f.VP[4 + r] * py) + f.VP[8 + r] * pz) + f.VP[12 + r] * 1.0f;
            float cx = c4[0] / c4[3], cy = c4[1] / c4[3], cz = c4[2] / c4[3];
            if (fabsf(cx) < mx) mx = fabsf(cx);
            if (fabsf(cy) < my) my = fabsf(cy);
            if (cz > mz) mz = cz;
        }
        float clip = f.culling_dist;
        if (mz < -clip || mx > clip || my > clip) culled = true;
    }
    if (!((f.lod_enable_mask >> (d.lod & 31u)) & 1u)) culled = true;
    // Column-band sharding: drop the draw when none of its splats can touch this rank's pixel columns.  (Doing the same
    // cull on the host and launching k_project / k_emit over the surviving chunks only was measured: no gain -- the
    // workgroups of culled chunks exit at once and the frames overlap.)
    if (!culled && f.band_cull && d.count && d.single_draw != 1u) {
        const float lo[3] = {f.loc_lo[0] + d.off[0], f.loc_lo[1] + d.off[1], f.loc_lo[2] + d.off[2]};
        const float hi[3] = {f.loc_hi[0] + d.off[0], f.loc_hi[1] + d.off[1], f.loc_hi[2] + d.off[2]};
        float bidx = 0.0f, bidy = 0.0f;
        if (f.surface_type == 2u) {
            bidx = (float)(5u * d.map_coord[0] / (f.map_half_wh[0] * 2u));
            bidy = (float)(2u * d.map_coord[1] / (f.map_half_wh[1] * 2u));
        }
        if (band_misses(f, lo, hi, bidx, bidy)) culled = true;
    }
    return culled;
}

// ------------------------------------------------------------------------------------
// k_cull (first kernel of the frame): clears the per-frame accumulators (saves three memset launches), fills the band-cull table of a
// column-band shard, and builds the launch table of k_project for THIS frame, one thread per chunk (a chunk = 256 list entries of one draw): only the chunks of
// the draws that survive the reference's per-draw cull (draw_is_culled: every chunk's thread evaluates its own draw's -- until late in round 4 a
// kernel of its own in front of this one, one launch and ~6 us more), in the per-XCD layout of chunk_tab_xcd (position k * 8 + x runs on XCD x = the draw's DrawDev::xcd; the order inside an
// XCD's list is the order of the atomic adds: irrelevant, a chunk's output slots are fixed).  An entry carries what the chunk's first load
// needs -- the list position of its lane 0 and the list's length and arena -- so that k_project's list-word load does not wait for the draw record.
// Round 4: CHUNK-LEVEL FRUSTUM CULL.  The reference culls whole tile draws on the CPU (renderer.rs:472-494: min |x|, min |y|, max z of the four
// corner NDCs, which lets every tile through that has one corner near the view axis), and vs_main then drops splat by splat
// (gswt.wgsl:163-167).  A draw's list is presorted by depth, so a chunk of it is a slab of the tile: measured on the c3 frame, 49 % of the
// chunks of the surviving draws hold NO splat that passes vs_main's frustum test -- half of k_project's live workgroups gathered 256 records
// to find that out.  Every static list carries the tile-local bounding box of each of its chunks (gswt_upload_scene); a chunk whose box,
// moved to the draw's offset, lies on the far side of ONE of the five planes of that test at all eight corners (clip-space coordinates are
// affine in the position, so then at every point of the box; a relative margin of 1e-3 covers the rounding of both evaluations) is left out
// of the table.  Nothing that vs_main would keep is dropped: images, visible and pair counts are bit-identical (GSWT_OPT_NO_CHUNK_CULL).
// Plain and HeightMap surfaces (the Sphere mapping moves a splat far from its flat position: no cull there); merged groups carry no boxes
// yet (their lists are rebuilt per sort event and mix member tiles) and stay whole.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cull(const Frame f, const DrawDev* __restrict__ draws, uint32_t* __restrict__ draw_culled,
                                              uint32_t* __restrict__ cell_culled, uint32_t n_cells,
                                              uint32_t* __restrict__ zero_a, uint32_t n_zero_a, uint32_t* __restrict__ zero_b, uint32_t n_zero_b,
                                              uint32_t* __restrict__ zero_c, uint32_t n_zero_c, uint32_t* __restrict__ zero_d, uint32_t n_zero_d,
                                              const uint2* __restrict__ chunk_tab, uint32_t n_chunks, const float* __restrict__ boxes, uint32_t chunk_cull,
                                              uint32_t* __restrict__ live_cnt, uint4* __restrict__ live_tab, uint32_t* __restrict__ live_cid)
{
    __shared__ uint32_t s_cnt[8], s_base[8];
    if (threadIdx.x < 8u) s_cnt[threadIdx.x] = 0u;
    const uint32_t gtid = blockIdx.x * 256u + threadIdx.x;
    for (uint32_t j = gtid; j < n_zero_a; j += gridDim.x * 256u) zero_a[j] = 0u;
    for (uint32_t j = gtid; j < n_zero_b; j += gridDim.x * 256u) zero_b[j] = 0u;
    for (uint32_t j = gtid; j < n_zero_c; j += gridDim.x * 256u) zero_c[j] = 0u;       // per-chunk pair counts: culled chunks never run
    for (uint32_t j = gtid; j < n_zero_d; j += gridDim.x * 256u) zero_d[j] = 0u;       // GSWT_ORDER_DEPTH: group rows / digit totals of the depth sort
    if (f.band_cull) {
        const uint32_t map_wh_y = f.map_wh_y;                                // 2 h + 1; 2 h on the Sphere (gswt.wgsl:52-63, 606-610)
        for (uint32_t j = gtid; j < n_cells; j += gridDim.x * 256u) {
            // the merged-member offset of gswt.wgsl:52-63, same expression as k_project
            const uint32_t mq = j / map_wh_y, mr = j % map_wh_y;
            const float ox = (float)((int32_t)(mq - f.map_half_wh[0]) + f.center_coord[0]) * f.tile_width;
            const float oy = (float)((int32_t)(mr - f.map_half_wh[1]) + f.center_coord[1]) * f.tile_width;
            const float lo[3] = {f.loc_lo[0] + ox, f.loc_lo[1] + oy, f.loc_lo[2]}, hi[3] = {f.loc_hi[0] + ox, f.loc_hi[1] + oy, f.loc_hi[2]};
            float bidx = 0.0f, bidy = 0.0f;
            if (f.surface_type == 2u) {                                      // a merged member's block, as k_project derives it from the map id
                bidx = (float)(5u * mq / (f.map_half_wh[0] * 2u));
                bidy = (float)(2u * mr / (f.map_half_wh[1] * 2u));
            }
            cell_culled[j] = band_misses(f, lo, hi, bidx, bidy) ? 1u : 0u;
        }
    }
    __syncthreads();
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    bool live = false;
    uint4 e = make_uint4(0u, 0u, 0u, 0u);
    uint32_t x = 0, rank = 0;
    if (c < n_chunks) {
        const uint2 ct = chunk_tab[c];
        const DrawDev& d = draws[ct.x];
        const bool dc = draw_is_culled(f, d);
        if (ct.y == 0u) draw_culled[ct.x] = dc ? 1u : 0u;      // (read by the debug-varyings build of k_project only)
        live = !dc && d.count != 0u;
        if (live && chunk_cull && d.merged == 0u && d.box_base != 0xFFFFFFFFu && f.surface_type <= 1u) {
            const float* b = boxes + 6u * (size_t)(d.box_base + (ct.y >> 8));
            float lo[3], hi[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {                 // the same (pos + offset) * scene_scale as vs_main: rounding is monotonic, so the box still holds every centre
                const float a = (b[k] + d.off[k]) * f.scene_scale[k], z = (b[3 + k] + d.off[k]) * f.scene_scale[k];
                lo[k] = fminf(a, z); hi[k] = fmaxf(a, z);
            }
            if (f.surface_type == 1u) {
                // HeightMap surface (gswt.wgsl:565-599): the mapped centre is (x, y, h(x, y) hz) + n z with |n| = 1 and h between the map's
                // extremes (k_cull's band cull bounds a cell the same way): x and y move by at most |z|, the height lies in
                // [surf_zlo - |z|, surf_zhi + |z|]; a little slack for the rounding of the bilinear sample and of n
                const float zp = fmaxf(fabsf(lo[2]), fabsf(hi[2])) * 1.0001f + 1e-6f;
                lo[0] -= zp; hi[0] += zp; lo[1] -= zp; hi[1] += zp;
                lo[2] = f.surf_zlo - zp - 1e-4f * (fabsf(f.surf_zlo) + 1.0f); hi[2] = f.surf_zhi + zp + 1e-4f * (fabsf(f.surf_zhi) + 1.0f);
            }
            bool xp = true, xn = true, yp = true, yn = true, zn = true;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const float px = (k & 1) ? hi[0] : lo[0], py = (k & 2) ? hi[1] : lo[1], pz = (k & 4) ? hi[2] : lo[2];
                float cv[4], q[4];
#pragma unroll
                for (int r = 0; r < 4; r++) cv[r] = ((f.V[r] * px + f.V[4 + r] * py) + f.V[8 + r] * pz) + f.V[12 + r];
#pragma unroll
                for (int r = 0; r < 4; r++) q[r] = ((f.GP[r] * cv[0] + f.GP[4 + r] * cv[1]) + f.GP[8 + r] * cv[2]) + f.GP[12 + r] * cv[3];
                const float clip = 1.2f * q[3];
                const float m = 1e-3f * (((fabsf(q[0]) + fabsf(q[1])) + fabsf(q[2])) + fabsf(clip)) + 1e-3f;
                xp = xp && (q[0] - clip > m); xn = xn && (-q[0] - clip > m);        // (a NaN compares false: such a chunk stays)
                yp = yp && (q[1] - clip > m); yn = yn && (-q[1] - clip > m);
                zn = zn && (-q[2] - clip > m);
            }
            if (xp || xn || yp || yn || zn) live = false;
        }
        x = d.xcd & 7u;
        if (live) {
            e = make_uint4(ct.x, ct.y, d.list_base + d.count - 1u - ct.y, d.count | (d.merged ? 0x80000000u : 0u));
            rank = atomicAdd(&s_cnt[x], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 8u && s_cnt[threadIdx.x] != 0u) s_base[threadIdx.x] = atomicAdd(&live_cnt[live_count_word(threadIdx.x)], s_cnt[threadIdx.x]);      // (a cache line per XCD's count: gswt_frame_layout.h)
    __syncthreads();
    if (live) {
        live_tab[(size_t)(s_base[x] + rank) * 8u + x] = e;
        live_cid[(size_t)(s_base[x] + rank) * 8u + x] = c;       // the chunk's number in slot order (k_emit walks the same table)
    }
}

// ------------------------------------------------------------------------------------
// k_project
// One workgroup = one 256-entry chunk of one draw, in composite (front-to-back) order:
// slot = slot_base + r, r-th entry from the END of the draw's list.
// ------------------------------------------------------------------------------------
// FULL = false is the lean variant the normal frame runs (surface None / HeightMap, draw_mode 0); the Sphere mapping
// (five sin / cos pairs per splat) and the debug recolouring live only in FULL = true.
// Measured and dropped (c3, isolated 103 us): (1) a persistent grid over a device-compacted chunk list -- static striding
// loses the dispatcher's dynamic balance (-8 % frames/s), a shared work counter serialises on one L2 address (230 us);
// (2) culling on the host and launching over the surviving chunks only -- the 20 k empty workgroups cost nothing
// measurable once two frames overlap (3519 vs 3517 frames/s); (3) four chunks per workgroup with all list / record
// loads issued up front (88 VGPRs, 123 us); (4) a per-chunk copy of the draw record + per-chunk cull flag to shorten the
// scalar chain chunk table -> draw -> flag: those were L2 hits, the 5.6 MB of copies are HBM misses (106 -> 113 us).
// (5) four table entries per workgroup, flags of the group fetched together and culled chunks settled at once (what
// paid in k_emit): unrolled, four inlined bodies = 77 VGPRs, 95 -> 101 us and c5 unchanged (527 frames/s); as a loop
// around one body the uniform float sub-expressions are hoisted into VGPRs (85).
// (6) the static lists a second time as 32-byte records in list order (plain / blending draws read 256 consecutive records,
// coalesced, addressed from the launch-table entry alone: no list word, no dependent gather; 150 MB at c3): 91.8 -> 88.2 us at c3,
// 128.1 -> 128.6 on the HeightMap surface, 461 -> 457 at c5 (stage events) -- the gather latency is hidden by the other waves.
// (7) column-band shards: a per-entry pre-pass (k_cull's cell table for merged groups, then position, the frustum test and a
// per-splat bound of the pixel extent against the band) followed by a compaction of the surviving entries to the front of the
// workgroup (ballot ranks + LDS exchange of entry / map id / slot), so that only ceil(survivors / 64) waves run the projection: the
// splats a rank of 8 carries through the whole projection fell from 471-619 k to 217-266 k (union of the bands still bitwise the
// unsharded image), and the kernel's time did not move (49-66 us per rank before and after; c5 441 -> 451 us per frame): in band
// mode, too, the kernel is paced by its workgroups' load chains, not by the projection's instructions.
// (9) round 3, with per-workgroup phase stamps (-DGSWT_TRACE, tools/project_trace.py): c3's 13.7 k live workgroups live 5.1 us each (launch
// table 0.4, list word 1.0, record 1.0, projection 1.7, barrier 0.5, sums 0.4) and start at ~260 per us, so that ~1 300 of the 2 048 slots are
// filled on average (each CU peaks at 7-8): lifetimes sum to 34 us x 2 048.  Two / four chunks per workgroup (half / a quarter of the
// workgroups for the dispatcher): 87 -> 101 -> 113 us.  A PERSISTENT grid taking launch positions from per-XCD queue heads (one returning
// atomic per chunk, issued a chunk ahead; the frame constants through device memory so that the loop does not hoist 150 scalar loads):
// 240 us with the eight heads in one cache line (~65 returning atomics per us and line), 114 us with the heads 256 bytes apart -- the loop
// costs 83 VGPRs (5 workgroups per CU, all of them busy: 1 150 resident, a chunk lives 5.8 us, 199 chunks per us against 264).
// (8) the grid sized from the previous frame's table of live chunks (+ 50 % + 64 per XCD list; k_totals flags a frame whose table
// outgrew its grid and the host re-runs it) instead of from the whole table: the dispatcher hands out ~4.6 k workgroups per us
// (flag 256: c5's 366 k workgroups that only read the launch table and leave take ~80 us), but the workgroups of culled chunks
// overlap with the live ones: project stage 461 -> 433 us at c5, 87 -> 87 us at c3, frame rates unchanged.
// -DGSWT_TRACE (tools/composite_trace.py): per work item, 100 MHz wall-clock stamps of the compositor's phases, left by lane 0 of wave 0:
// [0] entry, [1] item known, [2] first batch staged (gathers have arrived), [3] last walk done, [4] pairs of the item,
// [5] unused, [6] ticks wave 0 spent in bin + walk, [7] hardware id (HW_ID | XCC_ID << 32)
#ifdef GSWT_TRACE
constexpr uint32_t kTraceItems = 1u << 17;
__device__ unsigned long long g_trace[kTraceItems * 8];
#define GSWT_TR(K, V) { if (tr_on) g_trace[(size_t)tr_item * 8u + (K)] = (unsigned long long)(V); }
#define GSWT_NOW() wall_clock64()
#else
#define GSWT_TR(K, V)
#define GSWT_NOW() 0ull
#endif

// ---- k_project's stages, in the order the kernel calls them (A1..A10: vs_main of gswt.wgsl; F1, F2: DESIGN.md section 4).  A stage that discards the
// splat returns false and the kernel leaves; the discards are tested in vs_main's order (n_visible depends on it). ----
// What A3..A5 and the atmosphere hand to the vertex sequences
struct Mapped {
    float c0, c1, c2;                       // the centre: scene space behind A3, on the surface behind A4
    float F[9];                             // A4's surface frame (column major), the identity without a surface
    float mapped_z;
    float t_ratio; uint32_t higher_lod;     // A5
    float atm_dist, atm_fs;                 // atmosphere_fade: A5's camera distance and the far fade's alpha factor
};
// What a vertex sequence yields
struct VertexOut {
    float majx, majy, minx, miny, cr, cg, cb, ca, ndcx, ndcy, depth;
    uint32_t col_word;                      // the record's colour word: the splat's own bytes unless the fog re-quantises them
    float fade;                             // clamp(z/w + 1, 0, 1) on rgba: identically 1 for 0 <= z/w, kept for the debug output only
};

// gswt_set_tile_styles (no counterpart in vs_main), directly behind A1: the style of the map cell the entry belongs to -- the map_index the
// pick image reports for it, k_pick_resolve's expression -- as (tint r | g << 8 | b << 16 | tint_strength << 24, dim); a cell past the table
// reads as neutral.  A static draw's index is uniform (one scalar load per chunk), a merged draw's is the map id already loaded beside the
// list word.  A hidden cell (dim == 255) discards the splat before its record is fetched: not visible, no pairs.
__device__ __forceinline__ bool tile_style(const DrawDev& d, bool mrg, uint32_t map_id_m, const uint2* __restrict__ styles, uint32_t n_styles, uint2& sty)
{
    sty = make_uint2(0u, 0u);
    if (mrg) { if (map_id_m < n_styles) sty = styles[map_id_m]; }
    else if (d.map_index < n_styles) sty = styles[d.map_index];
    return (sty.y & 0xFFu) != 255u;
}

// tile_style's dim, behind the LOD-transition product, the pixel filter's comp and the far fade's factor, and its tint, in front of the fog:
// every written operator one binary32 operation (include/gswt_hip.h).  Returns whether the colour was tinted (the debug draw modes keep theirs).
__device__ __forceinline__ bool tile_style_shade(const Frame& f, const uint2& sty, VertexOut& v)
{
    const uint32_t dim = sty.y & 0xFFu, strength = sty.x >> 24;
    if (dim != 0u) v.ca = v.ca * ((float)(255u - dim) / 255.0f);
    if (strength == 0u || f.draw_mode != 0u) return false;
    const float k = (float)strength / 255.0f;
    v.cr = v.cr * (1.0f - k) + ((float)(sty.x & 0xFFu) / 255.0f) * k;
    v.cg = v.cg * (1.0f - k) + ((float)((sty.x >> 8) & 0xFFu) / 255.0f) * k;
    v.cb = v.cb * (1.0f - k) + ((float)((sty.x >> 16) & 0xFFu) / 255.0f) * k;
    return true;
}

// gswt_set_shadow_map (no counterpart in vs_main), behind A9 and the tint, in front of the fog: the float colour goes toward shade_color by
// sh = strength * (1 - lit) of the texels shadow_fetch loaded behind the frustum rejection (gswt_device_fn.h).  Returns whether the colour
// changed: sh == 0 (fully lit, outside the image or the depth range) leaves the record's colour word alone; the debug draw modes keep theirs.
__device__ __forceinline__ bool sun_shadow(const Frame& f, const Shadow& shd, const ShadowTap& tap, VertexOut& v)
{
    if (f.draw_mode != 0u) return false;
    const float sh = shadow_amount(shd, tap);
    if (sh == 0.0f) return false;
    v.cr = v.cr * (1.0f - sh) + shd.shade[0] * sh;
    v.cg = v.cg * (1.0f - sh) + shd.shade[1] * sh;
    v.cb = v.cb * (1.0f - sh) + shd.shade[2] * sh;
    return true;
}

// A3 :52-65 -- the offset of the entry's tile: the draw's own, or that of the member tile map_id of a merged group
__device__ __forceinline__ void tile_offset(const Frame& f, const DrawDev& d, uint32_t map_id, float& ox, float& oy, float& oz)
{
    ox = d.off[0]; oy = d.off[1]; oz = d.off[2];
    if (d.single_draw == 1u) {
        uint32_t map_wh_y = 2u * f.map_half_wh[1];
        if (f.surface_type != 2u) map_wh_y += 1u;
        // map_id / map_wh_y with a uniform divisor: for operands below 2^16 the quotient is the high word of map_id * (floor(2^32 / d) + 1)
        // (three instructions instead of the ~40 of a 32-bit division); larger maps take the division
        uint32_t mq, mr;
        if (f.map_wh_y_magic != 0u && map_id < 65536u) {
            mq = __umulhi(map_id, f.map_wh_y_magic);
            mr = map_id - mq * map_wh_y;
        } else { mq = map_id / map_wh_y; mr = map_id % map_wh_y; }
        ox = (float)((int32_t)(mq - f.map_half_wh[0]) + f.center_coord[0]) * f.tile_width;
        oy = (float)((int32_t)(mr - f.map_half_wh[1]) + f.center_coord[1]) * f.tile_width;
        oz = 0.0f;
    }
}

// A4 :75-87, surface HeightMap: the centre onto the height field, F = its tangent frame there
__device__ __forceinline__ void map_height_surface(const Frame& f, const float* hmap, Mapped& m)
{
    const float DELTA = 0.001f;
    float xr = gswt_host::hm_axis_range(f.map_half_wh[0], f.tile_width, f.height_map_scale[0]);
    float yr = gswt_host::hm_axis_range(f.map_half_wh[1], f.tile_width, f.height_map_scale[1]);
    float h_u = gswt_host::hm_axis_coord(m.c0, f.map_half_wh[0], f.tile_width, xr);
    float h_v = gswt_host::hm_axis_coord(m.c1, f.map_half_wh[1], f.tile_width, yr);
    float hz = f.height_map_scale[2];
    float nz = sample_height(hmap, f.hm_w, f.hm_h, h_u, h_v) * hz;
    float dt = DELTA;
    float h_r = sample_height(hmap, f.hm_w, f.hm_h, h_u + dt, h_v) * hz;
    float h_l = sample_height(hmap, f.hm_w, f.hm_h, h_u - dt, h_v) * hz;
    float h_up = sample_height(hmap, f.hm_w, f.hm_h, h_u, h_v + dt) * hz;
    float h_d = sample_height(hmap, f.hm_w, f.hm_h, h_u, h_v - dt) * hz;
    float lx[3] = {1.0f, 0.0f, (h_r - h_l) / (2.0f * dt * xr)};
    float ly[3] = {0.0f, 1.0f, (h_up - h_d) / (2.0f * dt * yr)};
    float cz0 = lx[1] * ly[2] - lx[2] * ly[1];
    float cz1 = lx[2] * ly[0] - lx[0] * ly[2];
    float cz2 = lx[0] * ly[1] - lx[1] * ly[0];
    float len = sqrtf((cz0 * cz0 + cz1 * cz1) + cz2 * cz2);
    float* const F = m.F;
    F[0] = lx[0]; F[1] = lx[1]; F[2] = lx[2];
    F[3] = ly[0]; F[4] = ly[1]; F[5] = ly[2];
    F[6] = cz0 / len; F[7] = cz1 / len; F[8] = cz2 / len;
    float z = m.c2;
    m.c0 = m.c0 + F[6] * z;
    m.c1 = m.c1 + F[7] * z;
    m.c2 = nz + F[8] * z;
    m.mapped_z = nz;
}

// A4, surface Sphere: surface_mapping, gswt.wgsl:600-623 (icosahedral-strip parametrisation, 5 x 2 blocks); sphere_get_uv + sphere_uv_to_pos
// (gswt.wgsl:515-564) are gswt_host::sphere_point, the one the host's tile centres use
__device__ __forceinline__ void map_sphere_surface(const Frame& f, const DrawDev& d, uint32_t map_id, Mapped& m)
{
    const float DELTA = 0.001f;
    const float xmax = ((float)f.map_half_wh[0] * 2.0f) * f.tile_width;
    const float ymax = ((float)f.map_half_wh[1] * 2.0f) * f.tile_width;
    const float block_w = xmax / 5.0f;
    const float nx = m.c0 - (float)(f.center_coord[0] - (int32_t)f.map_half_wh[0]) * f.tile_width;
    const float ny = m.c1 - (float)(f.center_coord[1] - (int32_t)f.map_half_wh[1]) * f.tile_width;
    float bidx = (float)(5u * d.map_coord[0] / (f.map_half_wh[0] * 2u));
    float bidy = (float)(2u * d.map_coord[1] / (f.map_half_wh[1] * 2u));
    if (d.single_draw == 1u) {
        const uint32_t map_height = 2u * f.map_half_wh[1];
        bidx = (float)(5u * (map_id / map_height) / (f.map_half_wh[0] * 2u));
        bidy = (float)(2u * (map_id % map_height) / (f.map_half_wh[1] * 2u));
    }
    const float bx = nx - bidx * block_w, by = ny - bidy * block_w;
    using gswt_host::V3;
    using gswt_host::sphere_point;
    const V3 lzv = sphere_point(block_w, bidx, bidy, bx, by);
    const float R = f.sphere_radius;
    const float dt = DELTA * ymax;
    const V3 prv = sphere_point(block_w, bidx, bidy, bx + dt, by), plv = sphere_point(block_w, bidx, bidy, bx - dt, by);
    const V3 puv = sphere_point(block_w, bidx, bidy, bx, by + dt), pdv = sphere_point(block_w, bidx, bidy, bx, by - dt);
    // (by component for the loop below: the nine entries written out from the V3 fields schedule k_project<FULL> differently, and its
    // instantiations are held to the registers and instruction counts recorded in profiles/project_stages_ab.txt; the device assembly of
    // every other kernel of this file is kept byte for byte)
    const float lz[3] = {lzv.x, lzv.y, lzv.z}, pr[3] = {prv.x, prv.y, prv.z}, pl[3] = {plv.x, plv.y, plv.z};
    const float pu[3] = {puv.x, puv.y, puv.z}, pd[3] = {pdv.x, pdv.y, pdv.z};
    float* const F = m.F;
    for (int k = 0; k < 3; k++) {
        F[k] = (pr[k] * R - pl[k] * R) / (2.0f * dt);
        F[3 + k] = (pu[k] * R - pd[k] * R) / (2.0f * dt);
        F[6 + k] = lz[k];
    }
    const float z = m.c2;
    const float n0 = lz[0] * R, n1 = lz[1] * R, n2 = lz[2] * R;
    m.c0 = n0 + F[6] * z;
    m.c1 = n1 + F[7] * z;
    m.c2 = n2 + F[8] * z;
    m.mapped_z = n2;
}

// gswt_set_atmosphere (no counterpart in vs_main): dist is A5's cam_dist expression, computed once here; a splat the far fade takes
// to t == 0 is discarded right away (not visible, no pairs), like A5's t_ratio discards.  A NaN dist clamps to t = 0 (fmaxf drops it).
__device__ __forceinline__ bool atmosphere_fade(const Frame& f, Mapped& m)
{
    const float dx = m.c0 - f.cam_pos[0], dy = m.c1 - f.cam_pos[1], dz = m.c2 - f.cam_pos[2];
    m.atm_dist = sqrtf((dx * dx + dy * dy) + dz * dz);
    if (f.atm.fade_end > 0.0f) {
        const float t = clampf((f.atm.fade_end - m.atm_dist) * f.atm.fade_inv, 0.0f, 1.0f);
        if (t == 0.0f) return false;
        m.atm_fs = (t * t) * (3.0f - 2.0f * t);
    }
    return true;
}

// A5 :91-150 -- a tile in transition between two LODs: which of them this splat blends against and how far the blend is; a splat whose share
// of the blend is zero is discarded
template <bool ATM>
__device__ __forceinline__ bool lod_transition(const Frame& f, const DrawDev& d, uint32_t lod_id, Mapped& m)
{
    if (d.changing == 1u) {
        float dx = m.c0 - f.cam_pos[0], dy = m.c1 - f.cam_pos[1], dz = m.c2 - f.cam_pos[2];
        float cam_dist = ATM ? m.atm_dist : sqrtf((dx * dx + dy * dy) + dz * dz);
        uint32_t higher_lod;
        if (d.single_draw == 1u) {
            if (lod_id == 0u) higher_lod = 0u;
            else if (lod_id == f.num_lod - 1u) higher_lod = lod_id - 1u;
            else {
                float d1 = f.transition_dist[(lod_id - 1u) & 15u];
                float d2 = f.transition_dist[lod_id & 15u];
                higher_lod = (cam_dist - d1 < d2 - cam_dist) ? lod_id - 1u : lod_id;
            }
        } else {
            higher_lod = (d.changing_to_lower == 1) ? d.tile_lod : d.tile_lod - 1u;
        }
        float td = f.transition_dist[higher_lod & 15u];
        float thw = f.transition_width_ratio * td;
        const float t_ratio = clampf((cam_dist - td) / thw + 0.5f, 0.0f, 1.0f);
        m.t_ratio = t_ratio; m.higher_lod = higher_lod;
        if ((lod_id == higher_lod + 1u && t_ratio == 0.0f) || (lod_id == higher_lod && t_ratio == 1.0f)) return false;
    }
    return true;
}

// A7 :169-205, first half, the same in both sequences: Vrk from the record's six halves, or the point cloud's isotropic one
__device__ __forceinline__ void splat_cov3(const Frame& f, const DrawDev& d, const uint4& w1, float (&K)[9])
{
    {
        float a = half_decode(w1.x & 0xFFFFu), b = half_decode(w1.x >> 16);
        float cc = half_decode(w1.y & 0xFFFFu), dd = half_decode(w1.y >> 16);
        float e = half_decode(w1.z & 0xFFFFu), ff = half_decode(w1.z >> 16);
        K[0] = a; K[1] = b; K[2] = cc; K[3] = b; K[4] = dd; K[5] = e; K[6] = cc; K[7] = e; K[8] = ff;
    }
    if (f.point_cloud_radius > 0.0f) {
        float pr = f.point_cloud_radius;
        if (f.draw_mode > 0u) pr *= ldexpf(1.0f, (int)d.tile_lod);
        K[0] = pr; K[1] = 0; K[2] = 0; K[3] = 0; K[4] = pr; K[5] = 0; K[6] = 0; K[7] = 0; K[8] = pr;
    }
}

// A9 :268-399, 402-410 behind the byte -> float conversion, the same in both sequences: the debug draw modes' colours, and the share of a LOD
// transition's blend in alpha
template <bool FULL>
__device__ __forceinline__ void lod_blend_color(const Frame& f, const DrawDev& d, const uint4& w0, uint32_t lod_id, const Mapped& m, VertexOut& v)
{
    if (FULL && f.draw_mode != 0u) debug_draw_color(f, d, u2f(w0.x), u2f(w0.y), lod_id, m.t_ratio, v.cr, v.cg, v.cb);   // :268-399
    if (d.changing == 1u) {
        if (lod_id != m.higher_lod) v.ca = v.ca * m.t_ratio;
        else v.ca = v.ca * (1.0f - m.t_ratio);
    }
}

// distance fog: the colour goes toward fog_color by F(dist) and back into the record's 8 bits, so that Rec and the compositors
// stay what they are; the debug draw modes keep their float colours (col_f)
__device__ __forceinline__ void fog_requantise(const Frame& f, float atm_dist, uint32_t rgba8, VertexOut& v)
{
    const float F = fog_amount(f.atm, atm_dist);
    const float fr = v.cr * (1.0f - F) + f.atm.fog_color[0] * F;
    const float fg = v.cg * (1.0f - F) + f.atm.fog_color[1] * F;
    const float fb = v.cb * (1.0f - F) + f.atm.fog_color[2] * F;
    const uint32_t br = (uint32_t)rintf(fminf(fmaxf(fr, 0.0f), 1.0f) * 255.0f);
    const uint32_t bg = (uint32_t)rintf(fminf(fmaxf(fg, 0.0f), 1.0f) * 255.0f);
    const uint32_t bb = (uint32_t)rintf(fminf(fmaxf(fb, 0.0f), 1.0f) * 255.0f);
    v.col_word = br | bg << 8 | bb << 16 | (rgba8 & 0xFF000000u);
    v.cr = (float)br / 255.0f; v.cg = (float)bg / 255.0f; v.cb = (float)bb / 255.0f;     // what the compositor will read
}

// a tinted or shaded colour the fog does not touch goes back into the record's 8 bits by the fog's own expression (with the fog on, fog_requantise
// takes the tinted floats and this is not called: one quantisation either way)
__device__ __forceinline__ void tint_requantise(uint32_t rgba8, VertexOut& v)
{
    const uint32_t br = (uint32_t)rintf(fminf(fmaxf(v.cr, 0.0f), 1.0f) * 255.0f);
    const uint32_t bg = (uint32_t)rintf(fminf(fmaxf(v.cg, 0.0f), 1.0f) * 255.0f);
    const uint32_t bb = (uint32_t)rintf(fminf(fmaxf(v.cb, 0.0f), 1.0f) * 255.0f);
    v.col_word = br | bg << 8 | bb << 16 | (rgba8 & 0xFF000000u);
    v.cr = (float)br / 255.0f; v.cg = (float)bg / 255.0f; v.cb = (float)bb / 255.0f;     // what the compositor will read
}

// A6..A10, STRICT: operator by operator as the shader text writes them (the comment above k_project)
template <bool FULL, bool ORTHO, bool AA, bool ATM, bool STY, bool SHD>
__device__ __forceinline__ bool vertex_strict(const Frame& f, const DrawDev& d, const uint4& w0, const uint4& w1, uint32_t lod_id, const Mapped& m, const uint2& sty,
                                              const Shadow& shd, VertexOut& v)
{
    const float c0 = m.c0, c1 = m.c1, c2 = m.c2;
    const float* const F = m.F;
    // A6 :152-167
    float cv[4], q[4];
    for (int rr = 0; rr < 4; rr++) cv[rr] = ((f.V[rr] * c0 + f.V[4 + rr] * c1) + f.V[8 + rr] * c2) + f.V[12 + rr] * 1.0f;
    for (int rr = 0; rr < 4; rr++)
        q[rr] = ((f.GP[rr] * cv[0] + f.GP[4 + rr] * cv[1]) + f.GP[8 + rr] * cv[2]) + f.GP[12 + rr] * cv[3];
    const float clip = 1.2f * q[3];
    if (q[2] < -clip || q[0] < -clip || q[0] > clip || q[1] < -clip || q[1] > clip) return false;
    // gswt_set_shadow_map: the centre into the light's image and its four texel loads, issued here, behind the frustum rejection, so that
    // their round trip passes under A7 and A8; sun_shadow reads them behind A9.  (The loads are unconditional, gswt_device_fn.h: the wait for w1
    // in front of A7 is then a counted vmcnt(4) that leaves them in flight, not a vmcnt(0).)
    ShadowTap tap = {};
    if (SHD) tap = shadow_fetch(shd, c0, c1, c2);
    // A7 :169-205
    float K[9];
    splat_cov3(f, d, w1, K);
    if (f.surface_type > 0u) {          // Vrk = transform * Vrk * transpose(transform)
        float FK[9], R[9];
        for (int cc = 0; cc < 3; cc++)
            for (int rr = 0; rr < 3; rr++)
                FK[3 * cc + rr] = (F[rr] * K[3 * cc] + F[3 + rr] * K[3 * cc + 1]) + F[6 + rr] * K[3 * cc + 2];
        for (int cc = 0; cc < 3; cc++)
            for (int rr = 0; rr < 3; rr++)
                R[3 * cc + rr] = (FK[rr] * F[cc] + FK[3 + rr] * F[3 + cc]) + FK[6 + rr] * F[6 + cc];
        for (int k = 0; k < 9; k++) K[k] = R[k];
    }
    {                                   // scene_scale_mat * Vrk * transpose(scene_scale_mat): the full matrix products, zeros included
        const float S[9] = {f.scene_scale[0], 0.0f, 0.0f, 0.0f, f.scene_scale[1], 0.0f, 0.0f, 0.0f, f.scene_scale[2]};
        float SK[9], R[9];
        for (int cc = 0; cc < 3; cc++)
            for (int rr = 0; rr < 3; rr++)
                SK[3 * cc + rr] = (S[rr] * K[3 * cc] + S[3 + rr] * K[3 * cc + 1]) + S[6 + rr] * K[3 * cc + 2];
        for (int cc = 0; cc < 3; cc++)
            for (int rr = 0; rr < 3; rr++)
                R[3 * cc + rr] = (SK[rr] * S[cc] + SK[3 + rr] * S[3 + cc]) + SK[6 + rr] * S[6 + cc];
        for (int k = 0; k < 9; k++) K[k] = R[k];
    }
    // A8 :207-258
    float JT[9];
    if (ORTHO) {
        // J_T columns of the affine projection: (fx, 0, 0), (0, fy, 0), (0, 0, 0)
        JT[0] = f.focal[0]; JT[1] = 0.0f; JT[2] = 0.0f;
        JT[3] = 0.0f; JT[4] = f.focal[1]; JT[5] = 0.0f;
        JT[6] = 0.0f; JT[7] = 0.0f; JT[8] = 0.0f;
    } else {
        const float dd0 = c0 - f.cam_pos[0], dd1 = c1 - f.cam_pos[1], dd2 = c2 - f.cam_pos[2];
        float t[3];
        for (int rr = 0; rr < 3; rr++) t[rr] = (f.V[rr] * dd0 + f.V[4 + rr] * dd1) + f.V[8 + rr] * dd2;
        const float txtz = t[0] / t[2], tytz = t[1] / t[2];
        const float limx = 1.3f * f.htan[0], limy = 1.3f * f.htan[1];
        t[0] = clampf(txtz, -limx, limx) * t[2];
        t[1] = clampf(tytz, -limy, limy) * t[2];
        const float tz2 = t[2] * t[2];
        // J_T columns: (fx / tz, 0, -fx tx / tz^2), (0, fy / tz, -fy ty / tz^2), (0, 0, 0)
        JT[0] = f.focal[0] / t[2]; JT[1] = 0.0f; JT[2] = (-f.focal[0] * t[0]) / tz2;
        JT[3] = 0.0f; JT[4] = f.focal[1] / t[2]; JT[5] = (-f.focal[1] * t[1]) / tz2;
        JT[6] = 0.0f; JT[7] = 0.0f; JT[8] = 0.0f;
    }
    float Tm[9];                        // T = transpose(view3) * J_T
    for (int cc = 0; cc < 3; cc++)
        for (int rr = 0; rr < 3; rr++)
            Tm[3 * cc + rr] = (f.V[4 * rr + 0] * JT[3 * cc] + f.V[4 * rr + 1] * JT[3 * cc + 1]) + f.V[4 * rr + 2] * JT[3 * cc + 2];
    float Am[9], C2[9];                 // cov2d = transpose(T) * Vrk * T
    for (int cc = 0; cc < 3; cc++)
        for (int rr = 0; rr < 3; rr++)
            Am[3 * cc + rr] = (Tm[3 * rr + 0] * K[3 * cc] + Tm[3 * rr + 1] * K[3 * cc + 1]) + Tm[3 * rr + 2] * K[3 * cc + 2];
    for (int cc = 0; cc < 3; cc++)
        for (int rr = 0; rr < 3; rr++)
            C2[3 * cc + rr] = (Am[rr] * Tm[3 * cc] + Am[3 + rr] * Tm[3 * cc + 1]) + Am[6 + rr] * Tm[3 * cc + 2];
    const float c00 = C2[0], c01 = C2[1], c11 = C2[4];
    const float mid = 0.5f * (c00 + c11);
    const float hxx = 0.5f * (c00 - c11);
    const float radius = sqrtf(hxx * hxx + c01 * c01);
    const float l1 = mid + radius, l2 = mid - radius;
    if (l2 < 0.0f) return false;
    const float vx = c01, vy = l1 - c00;
    const float vlen = sqrtf(vx * vx + vy * vy);
    const float ex = vx / vlen, ey = vy / vlen;
    // GSWT_OPT_ANTIALIAS (no counterpart in vs_main): the pixel filter adds s to both eigenvalues -- the rejection above and the
    // direction stay those of the unfiltered cov2d -- and comp keeps the integrated opacity.  AA = false compiles what there was
    float l1f = l1, l2f = l2, comp = 1.0f;
    if (AA) {
        l1f = l1 + f.aa_s; l2f = l2 + f.aa_s;
        comp = clampf(sqrtf(l1 / l1f) * sqrtf(l2 / l2f), 0.0f, 1.0f);      // (fmaxf drops a NaN: 0)
    }
    const float smaj = fminf(sqrtf(2.0f * l1f), 1024.0f);
    const float smin = fminf(sqrtf(2.0f * l2f), 1024.0f);
    v.majx = smaj * ex; v.majy = smaj * ey;
    v.minx = smin * ey; v.miny = smin * -ex;
    // A9 :260-265, 402-410
    v.cr = (float)(w1.w & 0xFFu) / 255.0f;
    v.cg = (float)((w1.w >> 8) & 0xFFu) / 255.0f;
    v.cb = (float)((w1.w >> 16) & 0xFFu) / 255.0f;
    v.ca = (float)((w1.w >> 24) & 0xFFu) / 255.0f;
    lod_blend_color<FULL>(f, d, w0, lod_id, m, v);
    if (AA) v.ca = v.ca * comp;
    v.col_word = w1.w;
    if (ATM) {
        // far fade: behind the LOD-transition product and the pixel filter's comp (1.0f with the fade off: exact)
        v.ca = v.ca * m.atm_fs;
    }
    // gswt_set_tile_styles: dim behind the three alpha products above, tint in front of the fog, which then mixes the tinted floats
    bool tinted = false;
    if (STY) tinted = tile_style_shade(f, sty, v);
    // gswt_set_shadow_map: behind the tint, in front of the fog
    if (SHD) tinted = sun_shadow(f, shd, tap, v) || tinted;
    if (ATM && f.atm.fog_density > 0.0f && f.draw_mode == 0u) fog_requantise(f, m.atm_dist, w1.w, v);
    else if ((STY || SHD) && tinted) tint_requantise(w1.w, v);
    // A10 :415-419
    v.ndcx = q[0] / q[3]; v.ndcy = q[1] / q[3]; v.depth = q[2] / q[3];
    v.fade = clampf(q[2] / q[3] + 1.0f, 0.0f, 1.0f);
    return true;
}

// A6..A10, canonical sequence v2: dot products are fma chains, quotients are products with one correctly rounded
// reciprocal; the CPU checker evaluates exactly the same operations.  No ORTHO, AA or ATM form.
template <bool FULL>
__device__ __forceinline__ bool vertex_v2(const Frame& f, const DrawDev& d, const uint4& w0, const uint4& w1, uint32_t lod_id, const Mapped& m, VertexOut& v)
{
    const float c0 = m.c0, c1 = m.c1, c2 = m.c2;
    const float* const F = m.F;
    // A6 :152-167
    float cv[4], q[4];
    for (int rr = 0; rr < 4; rr++) cv[rr] = fmaf(f.V[8 + rr], c2, fmaf(f.V[4 + rr], c1, f.V[rr] * c0)) + f.V[12 + rr];
    for (int rr = 0; rr < 4; rr++)
        q[rr] = fmaf(f.GP[12 + rr], cv[3], fmaf(f.GP[8 + rr], cv[2], fmaf(f.GP[4 + rr], cv[1], f.GP[rr] * cv[0])));
    float clip = 1.2f * q[3];
    if (q[2] < -clip || q[0] < -clip || q[0] > clip || q[1] < -clip || q[1] > clip) return false;
    // A7 :169-205
    float K[9];
    splat_cov3(f, d, w1, K);
    if (f.surface_type > 0u) {
        float FK[9], R[9];
        for (int cc = 0; cc < 3; cc++)
            for (int rr = 0; rr < 3; rr++)
                FK[3 * cc + rr] = fmaf(F[6 + rr], K[3 * cc + 2], fmaf(F[3 + rr], K[3 * cc + 1], F[rr] * K[3 * cc]));
        for (int cc = 0; cc < 3; cc++)
            for (int rr = 0; rr < 3; rr++)
                R[3 * cc + rr] = fmaf(FK[6 + rr], F[6 + cc], fmaf(FK[3 + rr], F[3 + cc], FK[rr] * F[cc]));
        for (int k = 0; k < 9; k++) K[k] = R[k];
    }
    // scene_scale_mat * Vrk * transpose(scene_scale_mat): a product with 1.0 is exact, so the usual unit scale skips 18 multiplications
    // (uniform branch; same bits)
    if (f.scene_scale[0] != 1.0f || f.scene_scale[1] != 1.0f || f.scene_scale[2] != 1.0f)
        for (int cc = 0; cc < 3; cc++)
            for (int rr = 0; rr < 3; rr++) K[3 * cc + rr] = (f.scene_scale[rr] * K[3 * cc + rr]) * f.scene_scale[cc];
    // A8 :207-258
    float d0 = c0 - f.cam_pos[0], d1 = c1 - f.cam_pos[1], d2 = c2 - f.cam_pos[2];
    float t[3];
    for (int rr = 0; rr < 3; rr++) t[rr] = fmaf(f.V[8 + rr], d2, fmaf(f.V[4 + rr], d1, f.V[rr] * d0));
    const float rz = 1.0f / t[2];
    float txtz = t[0] * rz, tytz = t[1] * rz;
    float limx = 1.3f * f.htan[0], limy = 1.3f * f.htan[1];
    t[0] = clampf(txtz, -limx, limx) * t[2];
    t[1] = clampf(tytz, -limy, limy) * t[2];
    const float rz2 = rz * rz;
    float j00 = f.focal[0] * rz, j02 = -((f.focal[0] * t[0]) * rz2);
    float j11 = f.focal[1] * rz, j12 = -((f.focal[1] * t[1]) * rz2);
    float T0[3], T1[3];
    for (int rr = 0; rr < 3; rr++) {
        T0[rr] = fmaf(f.V[4 * rr + 2], j02, f.V[4 * rr + 0] * j00);
        T1[rr] = fmaf(f.V[4 * rr + 2], j12, f.V[4 * rr + 1] * j11);
    }
    float A0[3], A1[3];
    for (int k = 0; k < 3; k++) {
        A0[k] = fmaf(T0[2], K[3 * k + 2], fmaf(T0[1], K[3 * k + 1], T0[0] * K[3 * k]));
        A1[k] = fmaf(T1[2], K[3 * k + 2], fmaf(T1[1], K[3 * k + 1], T1[0] * K[3 * k]));
    }
    float c00 = fmaf(A0[2], T0[2], fmaf(A0[1], T0[1], A0[0] * T0[0]));
    float c01 = fmaf(A1[2], T0[2], fmaf(A1[1], T0[1], A1[0] * T0[0]));
    float c11 = fmaf(A1[2], T1[2], fmaf(A1[1], T1[1], A1[0] * T1[0]));
    float mid = 0.5f * (c00 + c11);
    float hxx = 0.5f * (c00 - c11);
    float radius = sqrtf(fmaf(hxx, hxx, c01 * c01));
    float l1 = mid + radius, l2 = mid - radius;
    if (l2 < 0.0f) return false;
    float vx = c01, vy = l1 - c00;
    float vlen = sqrtf(fmaf(vx, vx, vy * vy));
    const float rv = 1.0f / vlen;
    float ex = vx * rv, ey = vy * rv;
    float smaj = fminf(sqrtf(2.0f * l1), 1024.0f);
    float smin = fminf(sqrtf(2.0f * l2), 1024.0f);
    v.majx = smaj * ex; v.majy = smaj * ey;
    v.minx = smin * ey; v.miny = smin * -ex;
    // A9 :260-265, 402-410 (byte / 255 as byte * fl(1 / 255))
    const float k255 = 1.0f / 255.0f;
    v.cr = (float)(w1.w & 0xFFu) * k255;
    v.cg = (float)((w1.w >> 8) & 0xFFu) * k255;
    v.cb = (float)((w1.w >> 16) & 0xFFu) * k255;
    v.ca = (float)((w1.w >> 24) & 0xFFu) * k255;
    lod_blend_color<FULL>(f, d, w0, lod_id, m, v);
    v.col_word = w1.w;
    // A10 :415-419
    const float rq = 1.0f / q[3];
    v.ndcx = q[0] * rq; v.ndcy = q[1] * rq; v.depth = q[2] * rq;
    v.fade = clampf(fmaf(q[2], rq, 1.0f), 0.0f, 1.0f);
    return true;
}

// Fragment setup F1, F2: pixel-space centre and inverse affine map, the splat's rectangle of screen tiles, and its record.
// visible: the splat survived the vertex stage (counted in n_visible); count: its (tile, splat) pairs, 0 with my_rect left empty
template <bool FULL>
__device__ __forceinline__ void fragment_setup(const Frame& f, const VertexOut& v, uint32_t slot, Rec* recs, float* depths, float4* col_f,
                                               uint32_t& count, uint2& my_rect, bool& visible)
{
    float cxp = fmaf(0.5f, v.ndcx, 0.5f) * f.W;
    float cyp = fmaf(-0.5f, v.ndcy, 0.5f) * f.H;
    float hs = 0.5f * f.splat_scale;
    float ux = hs * v.majx, uy = -(hs * v.majy);
    float wx = hs * v.minx, wy = -(hs * v.miny);
    float uu = fmaf(uy, uy, ux * ux);
    float ww = fmaf(wy, wy, wx * wx);
    if (!((uu > 0.0f) && (ww > 0.0f) && (uu < __builtin_inff()) && (ww < __builtin_inff()))) return;
    visible = true;
    // depth_compare Less against the 1.0 clear when no proxy depth is bound (renderer.rs:182,436): a vertex-stage survivor
    // (counted in n_visible) that no fragment of can pass -- no pairs
    if (!f.has_depth && !(v.depth < 1.0f)) return;
    const float ruu = 1.0f / uu, rww = 1.0f / ww;
    const float r_iux = ux * ruu, r_iuy = uy * ruu, r_ivx = wx * rww, r_ivy = wy * rww;
    // half extents of |p| <= 2, inflated by 1e-5 relative + 1e-3 px (conservative under f32 rounding)
    float hx = fmaf(2.0f * sqrtf(fmaf(wx, wx, ux * ux)), 1.00001f, 0.001f);
    float hy = fmaf(2.0f * sqrtf(fmaf(wy, wy, uy * uy)), 1.00001f, 0.001f);
    // pixels whose CENTRE lies inside the box: x in [ceil(c - h - 0.5), floor(c + h - 0.5)]
    float fx0 = ceilf(cxp - hx - 0.5f), fx1 = floorf(cxp + hx - 0.5f);
    float fy0 = ceilf(cyp - hy - 0.5f), fy1 = floorf(cyp + hy - 0.5f);
    if (fx1 >= fx0 && fy1 >= fy0 && fx1 >= 0.0f && fy1 >= 0.0f && fx0 <= f.W - 1.0f && fy0 <= f.H - 1.0f) {
        int x0 = fx0 < 0.0f ? 0 : (int)fx0, x1 = fx1 > f.W - 1.0f ? f.width - 1 : (int)fx1;
        int y0 = fy0 < 0.0f ? 0 : (int)fy0, y1 = fy1 > f.H - 1.0f ? f.height - 1 : (int)fy1;
        int tx0 = x0 >> 4, tx1 = x1 >> 4, ty0 = y0 >> 4, ty1 = y1 >> 4;
        tx0 = max(tx0, f.col0); tx1 = min(tx1, f.col1 - 1);          // column band of this ctx (the whole frame when off)
        int rows = owned_rows(ty0, ty1, f.shard_index, f.shard_count);
        count = tx1 >= tx0 ? (uint32_t)((tx1 - tx0 + 1) * rows) : 0u;
        if (count) {
            my_rect = make_uint2((uint32_t)tx0 | ((uint32_t)tx1 << 16), (uint32_t)ty0 | ((uint32_t)ty1 << 16));
            // 32-byte record: the inverse map, the centre, alpha and the packed colour (unpacked by the compositor's blend);
            // the pixel half extents are re-derived from the inverse map by the compositor's staging lane, the depth
            // goes to a side array that only depth-tested / depth-ordered frames read
            Rec* dst = recs + slot;
            reinterpret_cast<float4*>(dst)[0] = make_float4(r_iux, r_iuy, r_ivx, r_ivy);
            // (the centre travels in NDC: the compositor takes its offset from a tile origin with one rounding, F3 of DESIGN.md section 4)
            reinterpret_cast<float4*>(dst)[1] = make_float4(v.ndcx, v.ndcy, v.ca, __uint_as_float(v.col_word));
            if (depths) depths[slot] = v.depth;
            if (FULL && f.draw_mode != 0u) col_f[slot] = make_float4(v.cr, v.cg, v.cb, 0.0f);   // debug colours are not bytes
        }
    }
}

// The kernel itself keeps the loads (launch table, list word, record: A1, A2 and the trace stamps around them) and the workgroup's sums; per
// splat it calls, in this order, the stages above: tile_offset (A3), map_height_surface / map_sphere_surface (A4), atmosphere_fade,
// clip_hidden (CLIP), lod_transition (A5), vertex_strict<FULL, ORTHO, AA, ATM, STY, SHD> or vertex_v2<FULL> (A6..A10; both over splat_cov3 and lod_blend_color, the
// strict one over shadow_fetch, tile_style_shade, sun_shadow, fog_requantise and tint_requantise) and fragment_setup (F1, F2, tile rectangle, record); with STY,
// tile_style runs directly behind A1, in front of the record's loads.  A new per-splat feature goes into the stage it
// belongs to; a new template flag into that stage's parameters.
// k_project's stamps (tools/project_trace.py), rows 8192 + launch position: [0] entry, [1] launch-table entry known, [2] list word arrived (lane 0),
// [3] record arrived (lane 0, when it gets that far), [4] wave 0 through the projection, [5] behind the workgroup barrier, [6] end,
// [7] hardware id (HW_ID | XCC_ID << 32) | chunk has pairs << 63
// The quotients and roots of the projection are IEEE operations (correctly rounded: what the CPU checker reproduces).
// STRICT (GSWT_OPT_STRICT_VS): A6..A10 as the shader text writes them (gswt.wgsl:152-258, 260-265, 402-419) -- every `*`, `+`, `-`, `/` its own
// correctly rounded binary32 operation, matrix x vector as the left-to-right sum of column products, the full `scene_scale_mat * Vrk *
// transpose(..)` and `transpose(T) * Vrk * T` matrix products, length = sqrt(x*x + y*y), normalize = v / length(v), no fused multiply-add:
// the same operations, in the same order, as the CPU checker's strict mode, per splat bit for bit.  The default (sequence v2, DESIGN.md
// section 4) evaluates the same expressions with fma chains and one reciprocal per quotient -- also legal WGSL, ~25 % fewer instructions,
// and up to 5e-4 away from this one on thin ellipses (lambda2 = mid - radius cancels).
// ORTHO (GSWT_OPT_PROJECTION = 1, STRICT only): the orthographic vertex stage.  vs_main as above except A8's Jacobian, gswt.wgsl:213-232: the
// projection is affine, so J_T is the constant ((fx, 0, 0), (0, fy, 0), (0, 0, 0)) with fx, fy = focal in pixels per world unit -- no t, no
// quotient by t.z, no htan_fov clamp.  T and cov2d stay the written full products.  Everything around it (instancing, surface mapping, clip test,
// LOD blend against cam_pos, the 1.2 w frustum test with w = 1, eigen-decomposition, colour, A10) is the same code.
// AA (GSWT_OPT_ANTIALIAS > 0, STRICT only): the screen-space pixel filter, f.aa_s on both eigenvalues of cov2d and the opacity compensation
// (include/gswt_hip.h).  A template parameter, not a branch on f.aa_s: the branch cost k_project 0.5 us at c3 with the filter off.
// ATM (gswt_set_atmosphere with either part on, STRICT only): the per-splat far fade and distance fog of include/gswt_hip.h, both functions of
// A5's camera distance.  A template parameter like AA, so that a frame with the block off launches the instantiation it always did; which
// of the two parts is on is a uniform branch on f.atm inside the ATM instantiations only.
// STY (gswt_set_tile_styles with a table on, STRICT only): the per-cell hide, dim and tint of include/gswt_hip.h.  A template parameter like
// ATM: a frame with styles off launches the instantiation it always did and never reads `styles`; which parts of a style are on for a splat
// is a branch on the loaded entry inside the STY instantiations only.
// SHD (gswt_set_shadow_map with a map on, STRICT only): the sun shadow of include/gswt_hip.h, a 2 x 2 depth compare in the light's image per
// splat that passed the frustum test.  A template parameter like STY: a frame with shadows off launches the instantiation it always did and
// never reads `shd`, which is a kernel argument of its own so that Frame stays what it was.
// CLIP (gswt_set_clip_volumes with a volume in force, STRICT only): the clip volumes of include/gswt_hip.h, clip_hidden (gswt_device_fn.h) on
// A4's centre directly behind the clip_height test.  A template parameter like SHD: a frame without volumes launches the instantiation it
// always did and never reads `clip`, the set by value as a kernel argument of its own behind `shd`.
template <bool DEBUG, bool FULL, bool STRICT, bool ORTHO, bool AA, bool ATM, bool STY, bool SHD, bool CLIP>
__global__ __launch_bounds__(256) void k_project(
    const Frame f, const DrawDev* __restrict__ draws, const uint2* __restrict__ chunk_tab,
    const uint32_t* __restrict__ static_list, const uint32_t* __restrict__ merged_list,
    const uint32_t* __restrict__ merged_map, const uint4* __restrict__ tex,
    const float* __restrict__ hmap, const uint32_t* __restrict__ draw_culled, const uint32_t* __restrict__ cell_culled,
    const uint32_t* __restrict__ live_cnt, const uint4* __restrict__ live_tab, uint2* __restrict__ rects,
    Rec* __restrict__ recs, float* __restrict__ depths, uint32_t* __restrict__ block_sums, uint32_t* __restrict__ super_sums, uint32_t n_super,
    Varyings* __restrict__ dbg, float4* __restrict__ col_f, const uint2* __restrict__ styles, uint32_t n_styles, const Shadow shd,
    const ClipSet clip)
{
    __shared__ uint32_t s_wsum[4], s_wvis[4];
    // chunk_tab is in LAUNCH order, which is not slot order: workgroup b runs on XCD b % 8, and the table is laid out so
    // that all chunks of a draw land on one XCD (DrawDev::xcd) -- a draw's gathers stay inside one tile type's 313 KB of the
    // record table, so an XCD's 4 MB L2 then holds the few tile types it is working on instead of all 48 (6.6 MB).
    // The normal frame launches over k_cull's table of live chunks (same layout, culled draws left out; workgroups past an XCD's
    // live count exit after one cached scalar load); the debug-varyings build visits every chunk through the static table.
    uint2 ct;
    uint32_t list_top = 0, list_cnt = 0;      // non-DEBUG: list index of this chunk's lane 0, list length | merged << 31 (from k_cull)
#ifdef GSWT_TRACE
    const bool tr_on = threadIdx.x == 0 && blockIdx.x < 49152u;
    const uint32_t tr_item = 8192u + blockIdx.x;
    GSWT_TR(0, GSWT_NOW())
#endif
    if (DEBUG) {
        ct = chunk_tab[blockIdx.x];
        if (ct.y == 0xFFFFFFFFu) return;    // padding of a short per-XCD list
    } else {
        const uint32_t x = blockIdx.x & 7u, k = blockIdx.x >> 3;
        if (k >= live_cnt[live_count_word(x)]) return;
        const uint4 lt = live_tab[(size_t)k * 8u + x];
        ct = make_uint2(lt.x, lt.y);
        list_top = lt.z; list_cnt = lt.w;
#ifdef GSWT_TRACE
        { unsigned long long sink = lt.x + lt.w; asm volatile("" :: "s"(sink)); }
        GSWT_TR(1, GSWT_NOW())
#endif
    }
    const DrawDev& d = draws[ct.x];
    const uint32_t tid = threadIdx.x;
    const uint32_t cid = (d.slot_base + ct.y) >> 8;      // chunk id in slot space
    const bool s_culled = DEBUG ? draw_culled[ct.x] != 0u : false;

    const uint32_t r = ct.y + tid;
    const uint32_t slot = d.slot_base + r;
    const bool in_list = DEBUG ? r < d.count : r < (list_cnt & 0x7FFFFFFFu);
    uint32_t count = 0;
    bool visible = false;
    uint2 my_rect = make_uint2(1u, 0u);     // empty: tx0 = 1 > tx1 = 0
    Varyings vout;
    if (DEBUG) { vout.visible = 0; vout.ndc[0] = vout.ndc[1] = vout.depth = 0.f; vout.major[0] = vout.major[1] = 0.f;
                 vout.minor[0] = vout.minor[1] = 0.f; vout.rgba[0] = vout.rgba[1] = vout.rgba[2] = vout.rgba[3] = 0.f; }

    if (in_list && !s_culled) {
        // list word (and, for a merged draw, the map id beside it: one round trip, not a third dependent one).  The normal frame
        // addresses it from the launch-table entry alone, so the load is in flight while the draw record is still being fetched.
        const bool mrg = DEBUG ? d.merged != 0u : (list_cnt >> 31) != 0u;
        const uint32_t li = DEBUG ? d.list_base + (d.count - 1u - r) : list_top - tid;
        const uint32_t* list = mrg ? merged_list : static_list;
        const uint32_t entry = list[li];
        const uint32_t map_id_m = mrg ? merged_map[li] : 0u;
        const uint32_t gs_index = entry & kIdxMask;
        const uint32_t lod_id = entry >> kLodShift;
#ifdef GSWT_TRACE
        { unsigned long long sink = entry; asm volatile("" :: "v"(sink)); }
        GSWT_TR(2, GSWT_NOW())
#endif
        do {
            // column-band shard: the member tile this entry belongs to cannot reach the band (k_cull's cell table)
            if (f.band_cull && d.single_draw == 1u && cell_culled[map_id_m] != 0u) break;
            // A1 gswt.wgsl:38-42
            if (d.valid_lod_id >= 0 && d.valid_lod_id != (int32_t)lod_id) break;
            uint2 sty = make_uint2(0u, 0u);
            if (STY && !tile_style(d, mrg, map_id_m, styles, n_styles, sty)) break;
            // A2 :45-49
            const uint4 w0 = tex[2 * (size_t)gs_index];
            const uint4 w1 = tex[2 * (size_t)gs_index + 1];
#ifdef GSWT_TRACE
            { unsigned long long sink = w0.x + w1.w; asm volatile("" :: "v"(sink)); }
            GSWT_TR(3, GSWT_NOW())
#endif
            // A3: the centre in scene space
            float ox, oy, oz;
            tile_offset(f, d, map_id_m, ox, oy, oz);
            Mapped m = {(u2f(w0.x) + ox) * f.scene_scale[0], (u2f(w0.y) + oy) * f.scene_scale[1], (u2f(w0.z) + oz) * f.scene_scale[2],
                        {1, 0, 0, 0, 1, 0, 0, 0, 1}, 0.0f, -1.0f, 0u, 0.0f, 1.0f};
            // A4: onto the surface
            if (f.surface_type == 1u) map_height_surface(f, hmap, m);
            else if (FULL && f.surface_type == 2u) map_sphere_surface(f, d, map_id_m, m);
            if (f.use_clip == 1u && m.mapped_z < f.clip_height) break;
            if (CLIP && clip_hidden(clip, m.c0, m.c1, m.c2)) break;
            if (ATM && !atmosphere_fade(f, m)) break;
            // A5
            if (!lod_transition<ATM>(f, d, lod_id, m)) break;
            // A6..A10
            VertexOut v;
            bool kept;
            if constexpr (STRICT) kept = vertex_strict<FULL, ORTHO, AA, ATM, STY, SHD>(f, d, w0, w1, lod_id, m, sty, shd, v);
            else kept = vertex_v2<FULL>(f, d, w0, w1, lod_id, m, v);
            if (!kept) break;
            if (DEBUG) {
                vout.ndc[0] = v.ndcx; vout.ndc[1] = v.ndcy; vout.depth = v.depth;
                vout.major[0] = v.majx; vout.major[1] = v.majy; vout.minor[0] = v.minx; vout.minor[1] = v.miny;
                vout.rgba[0] = v.cr * v.fade; vout.rgba[1] = v.cg * v.fade; vout.rgba[2] = v.cb * v.fade; vout.rgba[3] = v.ca * v.fade;
            }
            if (!(v.depth >= 0.0f && v.depth <= 1.0f)) break;
            // F1, F2, the tile rectangle and the record
            fragment_setup<FULL>(f, v, slot, recs, depths, col_f, count, my_rect, visible);
            if (DEBUG) vout.visible = visible;
        } while (0);
    }
    if (DEBUG && in_list) dbg[d.entry_base + (d.count - 1u - r)] = vout;
    GSWT_TR(4, GSWT_NOW())

    // workgroup sums: pairs and visible splats
    const uint32_t wsum = wave_sum(count), wvis = (uint32_t)__popcll(ballot64(visible));
    // (Round 4, measured and reverted: no barrier here -- every wave adding its own sums with fire-and-forget atomics (12 per workgroup
    // instead of 2 + a store, the rects stored whether or not the chunk emits pairs): k_project 57 -> 183 us at c3, 379 -> 561 at c5.  The
    // device-scope atomics of a kernel retire at ~1 per ns chip-wide whatever their addresses: 107 k more of them cost 125 us.)
    if ((tid & 63u) == 0) { s_wsum[tid >> 6] = wsum; s_wvis[tid >> 6] = wvis; }
    __syncthreads();
    GSWT_TR(5, GSWT_NOW())
    const uint32_t bsum = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
#ifdef GSWT_TRACE
    { unsigned hwid, xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid)); asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      GSWT_TR(7, (unsigned long long)hwid | ((unsigned long long)(xcc & 0xFFu) << 32) | ((unsigned long long)(bsum ? 1u : 0u) << 63)) }
#endif
    // k_emit reads the rects of a chunk only when the chunk has pairs
    if (bsum) rects[slot] = my_rect;
    if (tid == 0) {
        block_sums[cid] = bsum;
        // two-level sums, spread over n_chunks / 256 addresses (a single hot counter serialises the whole grid);
        // k_totals folds them into the frame's visible-splat and pair counts
        const SuperSums ss{n_super};
        if (bsum) atomicAdd(&super_sums[ss.pair_word(super_of_chunk(cid))], bsum);
        uint32_t v = s_wvis[0] + s_wvis[1] + s_wvis[2] + s_wvis[3];
        if (v) atomicAdd(&super_sums[ss.visible_word(super_of_chunk(cid))], v);
    }
    GSWT_TR(6, GSWT_NOW())
}

__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_w, uint32_t* total);

// The frame's visible-splat and pair counts (FrameCounters); super_excl[j] = pairs of all chunks before super-group j (exclusive
// scan of the pair half of super_sums: SuperSums' prefix words), so that k_emit reads one word instead of summing up to n_chunks / 256 of them
// (c5: 1 430 per workgroup).  Single workgroup.  (Folding it into k_emit -- every workgroup sums the super-group counts
// in front of it, workgroup 0 leaves the totals -- was measured: k_emit +6 us for the 4.6 us saved, 4015 -> 3881 frames/s.)
__global__ __launch_bounds__(256) void k_totals(const uint32_t* __restrict__ super_sums, uint32_t n_super,
                                                FrameCounters* __restrict__ counters, uint32_t* __restrict__ super_excl, uint32_t pair_cap,
                                                uint32_t* __restrict__ live_cnt, uint32_t launched_per_xcd)
{
    const SuperSums ss{n_super};
    // k_project is done with this frame's live-chunk counts: cleared here for the slot's next frame (k_cull both clears
    // buffers and adds to these counters, so it cannot clear them itself)
    if (live_cnt && threadIdx.x < 64u) {
        // the longest of the eight live lists: the host sizes the next frames' launch grids by it (live_longest); a frame whose grid was cut
        // shorter than its own lists has chunks that nobody projected: flagged, the host re-runs it with the full grid (gswt_api.hip, live_hint)
        uint32_t v = threadIdx.x < kLiveLists ? live_cnt[live_count_word(threadIdx.x)] : 0u;
        if (threadIdx.x < kLiveLists) {
            live_cnt[live_copy_word(threadIdx.x)] = v;            // (k_emit runs behind this kernel and walks the same table)
            live_cnt[live_count_word(threadIdx.x)] = 0u;
        }
        for (int o = 4; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
        if (threadIdx.x == 0u) {
            counters->res.live_longest = v;
            if (v > launched_per_xcd) counters->res.rerun = 1ull;
        }
    }
    __shared__ unsigned long long s_v[4];
    __shared__ uint32_t s_w[4];
    unsigned long long v = 0;
    // the frame's pair count is carried in 64 bits (a super-group sum is a u32 of at most 65 536 slots x #screen tiles); the
    // prefix words k_emit reads stay 32-bit: once the running total passes the pair capacity the frame is flagged as
    // overflowed right here, and nothing downstream of k_emit consumes pairs of a flagged frame
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < n_super; base += 1024u) {
        const uint32_t i = base + threadIdx.x * 4u;
        uint32_t p[4];
        unsigned long long sum = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t idx = min(i + (uint32_t)k, n_super - 1u);              // clamped, unmasked loads
            const uint32_t pv = super_sums[ss.pair_word(idx)], vv = super_sums[ss.visible_word(idx)];
            p[k] = i + k < n_super ? pv : 0u;
            v += i + k < n_super ? vv : 0u;
            sum += p[k];
        }
        // block scan of the low words; the high part of the block total is recovered from a 64-bit reduction
        uint32_t tot32;
        uint32_t ex = block_excl_scan((uint32_t)sum, s_w, &tot32) + (uint32_t)carry;
#pragma unroll
        for (int k = 0; k < 4; k++) { if (i + k < n_super) super_excl[i + k] = ex; ex += p[k]; }
        unsigned long long t64 = sum;
        for (int off = 32; off > 0; off >>= 1) t64 += __shfl_down(t64, off, 64);
        __syncthreads();
        if ((threadIdx.x & 63u) == 0) s_v[threadIdx.x >> 6] = t64;
        __syncthreads();
        carry += s_v[0] + s_v[1] + s_v[2] + s_v[3];
        __syncthreads();
    }
    v = wave_sum(v);
    if ((threadIdx.x & 63u) == 0) s_v[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        counters->res.n_pairs = carry; counters->res.n_visible = s_v[0] + s_v[1] + s_v[2] + s_v[3];
        if (carry > (unsigned long long)pair_cap) counters->res.rerun = 1ull;       // pair buffers too small: the host re-runs the frame
    }
}

// block-wide exclusive scan of one value per thread (256 threads); returns exclusive prefix,
// *total = block sum
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_w /*[4]*/, uint32_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t inc = wave_incl_scan(v, lane);
    if (lane == 63u) s_w[w] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t i = 0; i < w; i++) base += s_w[i];
    *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    return base + inc - v;
}

// ------------------------------------------------------------------------------------
// k_emit: one thread per slot; pairs written at block_off[blk] + local exclusive prefix,
// so the pair array is in composite (slot) order before the stable tile sort.
// key = screen tile index local to the shard; val = slot.
// ------------------------------------------------------------------------------------
// A workgroup takes kEmitGroup consecutive chunks: most chunks emit nothing (culled draws, LOD rings) and a workgroup
// that only learns so from a load costs a full memory round trip per chunk -- with one chunk per workgroup the kernel ran
// as (chunks / 2048 resident workgroups) x ~1.07 us: 22 us on c3, 190 us on c5's 365 k chunks.
// Measured and dropped: the four chunks side by side in a 1024-thread workgroup with a single barrier (32 us at c3 -- four times
// the waves for the empty groups); per-slot pair offsets left by k_project so that no per-chunk scan is needed here (18 us, +1.3 us
// there, no gain); groups of 8 / 16 (serialise the live chunks: 26 / 35 us at c3); launching over k_cull's table of LIVE chunks
// (what k_project does: 18 k of c3's 39 k chunks, 76 k of c5's 366 k; groups of 1 / 2 / 4 table entries): one more dependent load in
// front of everything, 24 / 22 / 24 us at c3 and 223 / 170 / 143 us at c5 against 23 / 130 for four consecutive chunks (stage
// events, gpurun_out s6) -- the workgroups of empty groups are not what the kernel's time is made of.
// (Round 4: nor the splats that cover many screen tiles -- a slot writing at most eight of its pairs itself and the workgroup the rest, 256
// consecutive pairs per step, from a queue in LDS: c3 18.7 us either way, c5 165 against 124, the dense c3d 277 against 46.)
// (Round 4, c5 again -- 366 k chunks, ~40 k with pairs: sixteen chunks per workgroup, the sixteen pair counts first and then each chunk that has
// pairs with loads of its own: 180 us against 129, c3 36.7 against 18.7.)
// ... nor the rects read for chunks that turn out to have no pairs (round 4: the pair counts first, everything else only for the chunks
// that have any -- c5 reads 750 MB of rects per frame for ~40 k of 366 k chunks: 131 us against 129, c3 18.5 either way);
// and neither is the barrier-separated walk over a workgroup's live chunks: ONE WAVE PER CHUNK (lane l owns slots 4 l .. 4 l + 3,
// offsets from one wave scan, the chunk's base from one wave reduction over its super-group's sums, no barrier, no LDS, the four
// chunks of a workgroup side by side) ran in 20.6 us at c3 and 146 us at c5 against 19.9 / 127.
constexpr uint32_t kEmitGroup = 4;

// block-wide (256 threads): exclusive scan of v and, in the same barrier pair, the sum of r
__device__ __forceinline__ uint32_t block_scan_and_sum(uint32_t v, uint32_t r, uint32_t* s_w /*[8]*/, uint32_t* v_total, uint32_t* r_total)
{
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t inc = wave_incl_scan(v, lane);
    r = wave_sum(r);
    if (lane == 63u) s_w[w] = inc;
    if (lane == 0u) s_w[4u + w] = r;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t i = 0; i < w; i++) base += s_w[i];
    *v_total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    *r_total = s_w[4] + s_w[5] + s_w[6] + s_w[7];
    __syncthreads();
    return base + inc - v;
}

// DEPTH (GSWT_ORDER_DEPTH, north_star's "global radix depth sort"): every pair also gets its splat's depth bits as a second key (dkeys), and
// the smallest / largest depth key of the frame is left in krange.  The pair list is then sorted stably on the depth bits in use (the tile id
// travels as the sort's payload) and after that on the tile bits as always: inside a screen tile the pairs end up in true depth order, equal
// depths in composite order.  Round 4's first version sorted the emitting SPLATS by depth and emitted the pairs in that order (compaction,
// three passes with the tile rect as payload, per-group pair counts, a scan, the emission: five more kernels and 111 us per c3 frame);
// keying the PAIRS costs one more 4-byte word per pair in k_emit and in the depth passes and needs none of that.
// TAB (every frame with a live-chunk table; without one, in the debug-varyings frame: four consecutive chunks of the frame): the workgroup takes four entries of k_cull's table of live chunks (k_project's launch table: one XCD's list, so the chunks are not
// neighbours in slot order -- they need not be: a chunk's first pair comes from the prefix arrays) instead of four consecutive chunks of
// the frame.  At c3 73 % of the chunks are not live, and 39 % of this kernel's workgroup-time was workgroups that loaded four zeros and left
// (tools/emit_trace.py); the price is one more dependent load in front of everything.  One frame at a time the kernel takes what it took (c3 18.9
// against 18.7 us, c5 125 against 124 -- as in round 2, when the table held 46 % of the chunks), but with frames in flight the workgroups that
// are no longer launched leave their slots to the other frames' kernels: c5 fly path 719-720 against 692-698 frames/s, c3 the same.
template <bool DEPTH, bool TAB>
__global__ __launch_bounds__(256) void k_emit(const Frame f, const uint2* __restrict__ rects,
                                              const uint32_t* __restrict__ block_sums, const uint32_t* __restrict__ super_excl,
                                              uint32_t n_chunks, uint32_t pair_cap, FrameCounters* __restrict__ counters,
                                              uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                              const float* __restrict__ depths, uint32_t* __restrict__ dkeys, uint32_t* __restrict__ krange,
                                              const uint32_t* __restrict__ live_cnt2, const uint32_t* __restrict__ live_cid)
{
    __shared__ uint32_t s_w[8];
    __shared__ uint32_t s_mn[DEPTH ? 4 : 1], s_mx[DEPTH ? 4 : 1];
#ifdef GSWT_TRACE
    // phase stamps of k_emit (tools/emit_trace.py), rows 81920 + workgroup: [0] entry, [1] every load has arrived, [2] exit, [3] chunks with pairs, [4] pairs
    const bool tr_on = threadIdx.x == 0 && blockIdx.x < 8192u;
    const uint32_t tr_item = 81920u + blockIdx.x;
    uint32_t tr_live = 0, tr_pairs = 0;
    GSWT_TR(0, GSWT_NOW())
    GSWT_TR(2, 0ull)
#endif
    uint32_t cid[kEmitGroup], sums[kEmitGroup], bs[kEmitGroup], sbase[kEmitGroup];
    uint2 rcs[kEmitGroup];
    float dep[kEmitGroup];
    uint32_t kmn = 0xFFFFFFFFu, kmx = 0u;
    uint32_t n_mine;
    if (TAB) {
        const uint32_t x = blockIdx.x & 7u, k0 = (blockIdx.x >> 3) * kEmitGroup;
        const uint32_t n_live = live_cnt2[live_count_word(x)];      // (live_cnt2: the table's copy rows, from live_copy_word(0))
        if (k0 >= n_live) return;
        n_mine = min(kEmitGroup, n_live - k0);
#pragma unroll
        for (uint32_t k = 0; k < kEmitGroup; k++) cid[k] = min(live_cid[(size_t)min(k0 + k, n_live - 1u) * 8u + x], n_chunks - 1u);
    } else {
        const uint32_t c0 = blockIdx.x * kEmitGroup;
        n_mine = min(kEmitGroup, n_chunks - c0);
#pragma unroll
        for (uint32_t k = 0; k < kEmitGroup; k++) cid[k] = min(c0 + k, n_chunks - 1u);
    }
    // All loads are issued together with clamped indices (masked loads are waited for one at a time): the chunks' pair counts, the
    // sums of the chunks in front of each inside its super-group, the super-group prefixes and the tile rects of this thread's slot
    // in every chunk.
#pragma unroll
    for (uint32_t k = 0; k < kEmitGroup; k++) {
        sums[k] = block_sums[cid[k]];
        bs[k] = block_sums[min((cid[k] & ~255u) + threadIdx.x, cid[k])];
        sbase[k] = super_excl[super_of_chunk(cid[k])];                         // pairs of all chunks before the chunk's super-group (k_totals)
        rcs[k] = rects[(size_t)cid[k] * 256u + threadIdx.x];         // only meaningful when sums[k] != 0 (k_project wrote it then)
        dep[k] = DEPTH ? depths[(size_t)cid[k] * 256u + threadIdx.x] : 0.0f;      // likewise (k_project stores a slot's depth beside its record)
    }
    uint32_t any = 0;
#pragma unroll
    for (uint32_t k = 0; k < kEmitGroup; k++) { if (k >= n_mine) sums[k] = 0u; any |= sums[k]; }
#ifdef GSWT_TRACE
    { unsigned long long sink = sums[0] + bs[0] + sbase[3] + rcs[0].x + rcs[3].y; asm volatile("" :: "v"(sink)); }
    GSWT_TR(1, GSWT_NOW())
    for (uint32_t k = 0; k < kEmitGroup; k++) { tr_live += sums[k] ? 1u : 0u; tr_pairs += sums[k]; }
    GSWT_TR(3, tr_live)
    GSWT_TR(4, tr_pairs)
    if (any == 0u) { GSWT_TR(2, GSWT_NOW()) }
#endif
    if (any == 0u) return;
    const int sc = f.shard_count <= 1 ? 1 : f.shard_count;
#pragma unroll
    for (uint32_t k = 0; k < kEmitGroup; k++) {
        if (sums[k] == 0u) continue;                                 // workgroup-uniform
        const uint2 rc = rcs[k];
        const uint32_t slot = cid[k] * 256u + threadIdx.x;
        const int tx0 = rc.x & 0xFFFFu, tx1 = rc.x >> 16, ty0 = rc.y & 0xFFFFu, ty1 = rc.y >> 16;
        uint32_t count = 0;
        if (tx1 >= tx0) count = (uint32_t)((tx1 - tx0 + 1) * owned_rows(ty0, ty1, f.shard_index, f.shard_count));
        // first pair of the chunk = pairs of the earlier super-groups + of the earlier chunks of its own group; one barrier pair
        // yields that sum and the exclusive scan of this chunk's per-slot pair counts
        uint32_t tot, chunk_base;
        uint32_t off = block_scan_and_sum(count, (cid[k] & ~255u) + threadIdx.x < cid[k] ? bs[k] : 0u, s_w, &tot, &chunk_base);
        chunk_base += sbase[k];
        off += chunk_base;
        if ((unsigned long long)chunk_base + tot > (unsigned long long)pair_cap) {   // pair buffers too small: host re-runs the frame
            if (threadIdx.x == 0) atomicOr(&counters->res.rerun, 1ull);
            return;
        }
        if (count == 0) continue;
        // depth in [0, 1]: bit order = value order once -0.0 (which k_project lets through) is made +0.0 -- the oracle's float
        // comparison ties the two, its key 0x80000000 would sort last
        const uint32_t dkey = __float_as_uint(dep[k] + 0.0f);
        if (DEPTH) { kmn = min(kmn, dkey); kmx = max(kmx, dkey); }
        if (sc > 1) {                                                // row shards: this rank's rows of the rect, numbered locally
            for (int ty = ty0 + ((f.shard_index - ty0 % sc) + sc) % sc; ty <= ty1; ty += sc) {
                const uint32_t row = (uint32_t)(ty / sc) * (uint32_t)f.tiles_x;
                for (int tx = tx0; tx <= tx1; tx++) {
                    keys[off] = row + (uint32_t)(tx - f.col0);
                    vals[off] = slot;
                    if (DEPTH) dkeys[off] = dkey;
                    off++;
                }
            }
        } else {
            // the usual frame: a loop of its own, so that the ~25-instruction integer division by the shard count is not part of every row of
            // every splat (as `ty / sc` with sc == 1 it was: the compiler cannot know the uniform's value)
            for (int ty = ty0; ty <= ty1; ty++) {
                const uint32_t row = (uint32_t)ty * (uint32_t)f.tiles_x;
                for (int tx = tx0; tx <= tx1; tx++) {
                    keys[off] = row + (uint32_t)(tx - f.col0);
                    vals[off] = slot;
                    if (DEPTH) dkeys[off] = dkey;
                    off++;
                }
            }
        }
    }
    GSWT_TR(2, GSWT_NOW())
    if (DEPTH && krange) {                                      // (the tile-local depth sort takes each tile's own range: no krange)
        // key range of the frame: one guarded atomic pair per workgroup.  (One pair per WAVE on the two words is tens of thousands of
        // atomics on two addresses, which the memory side serialises at ~8 ns each.)  The words only grow ([0] holds ~min), so a stale read
        // can only cause a redundant atomic, never a missed one.
        kmn = wave_min(kmn); kmx = wave_max(kmx);
        if ((threadIdx.x & 63u) == 0u) { s_mn[DEPTH ? threadIdx.x >> 6 : 0u] = kmn; s_mx[DEPTH ? threadIdx.x >> 6 : 0u] = kmx; }
        __syncthreads();
        if (threadIdx.x == 0u) {
            kmn = min(min(s_mn[0], s_mn[DEPTH ? 1 : 0]), min(s_mn[DEPTH ? 2 : 0], s_mn[DEPTH ? 3 : 0]));
            kmx = max(max(s_mx[0], s_mx[DEPTH ? 1 : 0]), max(s_mx[DEPTH ? 2 : 0], s_mx[DEPTH ? 3 : 0]));
            if (kmn <= kmx) {
                if (krange_min_word(kmn) > __builtin_nontemporal_load(&krange[0])) atomicMax(&krange[0], krange_min_word(kmn));     // (load_krange)
                if (kmx > __builtin_nontemporal_load(&krange[1])) atomicMax(&krange[1], kmx);
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// Stable LSD radix sort pass on `nbits` (<= 8) key bits starting at `shift`.
// 4096 items per workgroup; each of the 4 waves owns 1024 consecutive items and ranks
// them 64 at a time with ballot match-any, so in-wave order == memory order.
// ------------------------------------------------------------------------------------
// pair count as seen by the kernels downstream of k_emit: never more than the buffers hold
// (a frame's SortCount is the view of its counter block: n = the pair count, refused = the re-run flag k_emit sets).  On overflow part of
// the pair buffer is unwritten, so the whole downstream chain processes nothing and the host re-runs the frame with larger buffers.
__device__ __forceinline__ uint32_t clamped_count(const SortCount* count, uint32_t n_cap)
{
    const unsigned long long n = count->n;
    if (count->refused != 0ull || n > (unsigned long long)n_cap) return 0u;
    return (uint32_t)n;
}

// A sort workgroup takes 4096 consecutive items whatever its width: THREADS x (4096 / THREADS) per thread, each wave ranking
// its share 64 at a time.  Sweeps, frames/s with two frames in flight (bench.py, 300 steps): c3 (2.66 M pairs) 256 threads
// 3733, 512 3925, 1024 3899; c3h 3105 / 3578 / 3589; c5 (21 M pairs) 537.5 / 531.6 / 506.2.  The sort stage alone at c3:
// 77 / 69 / 76 us (other splits of the block: 1024x8 78, 512x16 82, 1024x2 95, 512x4 84).  launch_sort picks 512 threads up
// to kSortWideMax pairs of capacity and 256 above.  (kSortBlock: gswt_frame_layout.h, with the workspace the block size shapes.)
constexpr uint32_t kSortWideMax = 0xFFFFFFFFu;  // pair capacities up to this use 512-thread workgroups (every size since k_radix_supscan: the 256-thread build only won at c5 while each workgroup summed ~100 group rows)

// Per pass: k_radix_hist leaves, for every digit d, the per-workgroup counts ghist[d][blk], the sums over
// groups of 32 workgroups gsup[d][blk >> 5] and the digit totals gtot[d] (integer atomics, spread over
// 256 x nblk/32 addresses).  k_radix_scatter derives its global offsets from those directly -- digit d's
// base = sum of gtot[< d] + gsup[d][< blk >> 5] + ghist[d][same group, < blk] -- so no scan kernel runs.  (kSupShift and where the
// three lie in the workspace: RadixWs, gswt_frame_layout.h.)
constexpr uint32_t kSupDirect = 32;             // up to this many groups the scatter kernel reads every group row instead of digit totals

// Key range of the depth sort as k_emit<DEPTH> leaves it: [0] = ~smallest key, [1] = largest (both through atomicMax, so the frame's zeroed
// scratch words are the neutral start); no keys at all reads as (0, 0).
__device__ __forceinline__ void load_krange(const uint32_t* __restrict__ krange, uint32_t& kmin, uint32_t& kmax)
{
    kmin = krange_min_word(krange[0]); kmax = krange[1];
    if (kmax < kmin) { kmin = 0u; kmax = 0u; }
}
// Number of radix passes the keys in [kmin, kmax] need (see k_radix_hist): pass p covers bits 8p .. 8p+7 of key - kmin.  The host
// launches as many passes as the previous frames needed (three at c3: visible depths of one frame span ~2^21 ulps); a frame that needs
// more is flagged by k_items and re-run, like a capacity overflow; one that needs fewer is sorted all the same (the extra passes see one
// digit and move nothing) and the host gives the pass back after a while.
__device__ __forceinline__ uint32_t sort_passes_needed(const uint32_t* __restrict__ krange)
{
    uint32_t kmin, kmax;
    load_krange(krange, kmin, kmax);
    const uint32_t span = kmax - kmin;
    uint32_t p = 1;                                     // the first pass always runs
    for (uint32_t sh = 8; sh < 32u; sh += 8u) if ((span >> sh) != 0u) p++;
    return p;
}

// Lanes of the wave that hold the same digit as this one (match-any on `nbits` bits), restricted to valid lanes.
// (Round 4, measured and dropped: a fast path for rounds whose 64 items share one digit -- one broadcast + one ballot instead of nbits
// ballots, taken in the passes after the first, where the pairs of one screen tile are neighbours: the last pass of the c3 pair sort went
// from 18.5 to 21.8 us.  Too few rounds are uniform, and the mixed ones pay the two extra wave-wide operations.)
// One step per key bit, six vector instructions each: the lane's bit sign-extended (v_bfe_i32: -1 / 0), the ballot of the set bits
// (v_cmp straight into a scalar pair), and per half of the mask peers &= ~(ballot ^ own) (v_xnor, v_and).  Unrolled, so no loop counter
// either.  (Until round 4 the loop was rolled and went through __ballot(int): ten vector instructions, two s_nop and the loop's scalar
// bookkeeping per bit -- about twice the issue slots.)
__device__ __forceinline__ unsigned long long match_digit(uint32_t dgt, bool valid, uint32_t nbits)
{
    const unsigned long long vm = __builtin_amdgcn_ballot_w64(valid);
    uint32_t plo = (uint32_t)vm, phi = (uint32_t)(vm >> 32);
    // (all eight steps whatever the digit's width: the callers mask the digit, so a bit above it is clear in every lane and its step
    // changes nothing -- five instructions, against a branch per bit on a count the compiler keeps as a lane mask)
    (void)nbits;
#pragma unroll
    for (uint32_t b = 0; b < 8u; b++) {
        const uint32_t own = (uint32_t)__builtin_amdgcn_sbfe((int)dgt, b, 1u);
        const unsigned long long m = __builtin_amdgcn_ballot_w64(own != 0u);
        plo &= ~((uint32_t)m ^ own);
        phi &= ~((uint32_t)(m >> 32) ^ own);
    }
    return ((unsigned long long)phi << 32) | plo;
}

template <int kSortThreads>
__global__ __launch_bounds__(kSortThreads) void k_radix_hist(const uint32_t* __restrict__ keys, const SortCount* __restrict__ count,
                                                    uint32_t n_cap, uint32_t shift, uint32_t mask, uint32_t nbits, uint32_t* __restrict__ ghist,
                                                    uint32_t* __restrict__ gsup, uint32_t* __restrict__ gtot, uint32_t nblk,
                                                    uint32_t nsup, const uint32_t* __restrict__ krange)
{
    constexpr int kSortItems = kSortBlock / kSortThreads;
    // krange (the depth passes only): the frame's smallest / largest depth key.  Digits are taken from key - smallest, so the passes the host
    // launches cover the bits of (largest - smallest): visible depths of one c3 frame span ~2^21 ulps -- three 8-bit passes, not four
    // (sort_passes_needed; a frame that needs more than were launched is flagged by k_items and re-run).
    uint32_t kmin = 0;
    if (krange) { uint32_t kmax; load_krange(krange, kmin, kmax); }
    const uint32_t n = clamped_count(count, n_cap);
    __shared__ uint32_t s_h[256];
    if (threadIdx.x < 256u) s_h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t base = blockIdx.x * kSortBlock + w * (64 * kSortItems);
    if (base < n) {                               // wave-uniform
        // all loads first, with clamped indices (a load under a lane mask is waited for on the spot, which made
        // the loads of a lane dependent round trips)
        uint32_t key[kSortItems];
#pragma unroll
        for (int k = 0; k < kSortItems; k++) key[k] = keys[min(base + (uint32_t)k * 64u + lane, n - 1u)];
        // One LDS add per RUN of equal digits in a round, by the run's first lane: pairs of one screen tile are neighbours from the
        // second pass on (the first pass ordered them by the low digit, stably), so a round's 64 lanes used to add 1 to the same one
        // or two LDS words, which the LDS serialises -- the second pass's histogram took 13 us at c3 and 85 us at c5 against 4.7 / 28
        // for the first.  (One add per distinct digit through match-any, as k_radix_scatter counts, was measured here earlier: 12.1 us
        // against 11.2 -- eight ballots per round; a run needs one lane shift and one ballot.)
#pragma unroll
        for (int k = 0; k < kSortItems; k++) {
            const bool valid = base + (uint32_t)k * 64u + lane < n;           // valid lanes are a prefix of the wave
            const uint32_t dgt = ((key[k] - kmin) >> shift) & mask;
            const uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)dgt, 0x138, 0xF, 0xF, true);      // wave_shr:1 (lane 0 is a head anyway)
            const unsigned long long heads = ballot64(valid && (lane == 0u || prev != dgt));
            const unsigned long long vmask = ballot64(valid);
            if ((heads >> lane) & 1ull) {
                const unsigned long long later = heads & ~((2ull << lane) - 1ull);      // run heads behind this lane
                const uint32_t end = later ? (uint32_t)__ffsll((long long)later) - 1u : (uint32_t)__popcll(vmask);
                atomicAdd(&s_h[dgt], end - lane);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x >= 256u) return;
    const uint32_t cnt = s_h[threadIdx.x];
    // digit-minor layouts ([blk][256], [group][256]) so that one workgroup's reads and writes are contiguous
    ghist[blockIdx.x * 256u + threadIdx.x] = cnt;
    if (cnt) {
        atomicAdd(&gsup[(blockIdx.x >> kSupShift) * 256u + threadIdx.x], cnt);
        // digit totals: with few groups k_radix_scatter sums the group rows itself, with many k_radix_supscan leaves them -- every
        // workgroup adding to the same 256 words (650 adds per word at c3, 5 300 at c5) was the most contended traffic of the sort
    }
    (void)nblk; (void)nbits; (void)gtot; (void)nsup;
}

// Large sorts only (more than kSupDirect groups of 32 workgroups: above ~4 M items): turns the group rows gsup[group][digit] into
// their exclusive prefix over the groups and leaves the digit totals in gtot.  Without it every scatter workgroup summed the rows of
// all groups in front of it -- at c5 (21.8 M pairs, 208 groups) on average 104 KB of L2 reads per workgroup, 690 MB per pass, more than
// the pass moves in keys and values -- and the digit totals were 5 300-way contended atomics.  One wave per digit, 64 groups per round.
// (Summing up to 64 group rows in the scatter workgroups, two rounds of 32, so that the fly path's frames whose pair capacity
// crosses 4 M pairs need no launch of this kernel: 4 219 / 4 139 frames/s against 4 262 / 4 240 with it, same box -- not better.)
__global__ __launch_bounds__(256) void k_radix_supscan(uint32_t* __restrict__ gsup, uint32_t* __restrict__ gtot, uint32_t nsup)
{
    const uint32_t lane = threadIdx.x & 63u, d = blockIdx.x * 4u + (threadIdx.x >> 6);
    uint32_t carry = 0;
    for (uint32_t g0 = 0; g0 < nsup; g0 += 256u) {
        // four rounds of loads in flight together (clamped, unmasked)
        uint32_t v[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) v[k] = gsup[(size_t)min(g0 + k * 64u + lane, nsup - 1u) * 256u + d];
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t g = g0 + k * 64u + lane;
            const uint32_t x = g < nsup ? v[k] : 0u;
            const uint32_t inc = wave_incl_scan(x, lane);
            if (g < nsup) gsup[(size_t)g * 256u + d] = carry + inc - x;
            carry += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        }
    }
    if (lane == 0u) gtot[d] = carry;
}

// The block's 4096 items are first ranked INTO LDS (sorted by digit inside the block), then copied out: consecutive threads
// write consecutive addresses of a digit's run instead of every lane storing two separate words to its own rank position
// (a wave's store instruction used to touch as many regions as it held distinct digits).
// AUX (the depth passes of GSWT_ORDER_DEPTH): a second 4-byte payload per item -- the pair's tile id -- travels with it.
//   AUX = 1: the ranking leaves each sorted item's source position inside the block (u16, 8 KB of LDS) and the copy-out fetches the payload
//            from the block's own 16 KB window of the input (64 scattered dwords per wave instruction).  Three workgroups per CU.
//   AUX = 2: the payload is staged through LDS beside the (key, value) pair (16 KB more: 60 KB per workgroup, two workgroups per CU).
// Measured per pass (scatter<512>, without payload / AUX 1 / AUX 2): c3 (2.66 M pairs) 18.5 / 22.7 / 26.6 us, c3d (8.2 M) 37.5 / 55.7 / 54.8,
// c5 (21.4 M) 99 / 164 / 145: the small sort is a latency chain that wants the third workgroup, the large one pays for the scattered
// reads.  launch_sort takes AUX 2 above 12 M pairs of capacity.
// (512-thread build: at most 80 VGPRs, so that THREE workgroups fit a CU -- c3's 649 blocks are then all resident at once (768 slots) and the
// kernel lasts one block's chain; at 86 VGPRs, where the five-instruction match_digit first left it, two fit, the blocks ran in two
// generations, and the chain it had shortened from 12.8 to 9.0 us bought nothing)
template <int kSortThreads, int AUX>
__global__ __launch_bounds__(kSortThreads) __attribute__((amdgpu_waves_per_eu((kSortThreads == 512 && AUX != 2) ? 6 : 1, 8))) void k_radix_scatter(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in,
                                                       uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out,
                                                       const SortCount* __restrict__ count, uint32_t n_cap, uint32_t shift,
                                                       uint32_t mask, uint32_t nbits, const uint32_t* __restrict__ ghist,
                                                       const uint32_t* __restrict__ gsup, const uint32_t* __restrict__ gtot,
                                                       uint32_t nblk, uint32_t nsup, uint2* __restrict__ ranges, const uint32_t* __restrict__ krange,
                                                       const uint32_t* __restrict__ aux_in, uint32_t* __restrict__ aux_out)
{
    constexpr int kSortItems = kSortBlock / kSortThreads, kSortWaves = kSortThreads / 64;
    uint32_t kmin = 0;                                  // (see k_radix_hist)
    if (krange) { uint32_t kmax; load_krange(krange, kmin, kmax); }
    const uint32_t n = clamped_count(count, n_cap);
    if (blockIdx.x * kSortBlock >= n) return;
#ifdef GSWT_TRACE
    // phase stamps of the scatter pass (tools/sort_trace.py): rows kTraceItems / 2 + (shift ? 4096 : 0) + block
    const bool tr_on = threadIdx.x == 0 && blockIdx.x < 4096u;
    const uint32_t tr_item = kTraceItems / 2u + (shift ? 4096u : 0u) + blockIdx.x;
    GSWT_TR(0, GSWT_NOW())
#endif
    __shared__ uint32_t s_h[kSortWaves][256];
    __shared__ uint32_t s_g[256];                       // digit -> (global base of this block's run) - (its start inside the block)
    __shared__ uint32_t s_w[4], s_w2[4];
    __shared__ uint32_t s_gs[2][256];                   // direct group sums: [0] earlier groups, [1] all groups (waves 4..7 -> waves 0..3)
    __shared__ uint2 s_kv[kSortBlock];
    __shared__ uint32_t s_aux[AUX == 2 ? kSortBlock : 1];    // AUX 2: the payload, ranked beside s_kv
    __shared__ uint16_t s_src[AUX == 1 ? kSortBlock : 1];    // AUX 1: sorted position inside the block -> source position inside the block
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (int k = 0; k < kSortWaves * 256 / kSortThreads; k++) (&s_h[0][0])[k * kSortThreads + threadIdx.x] = 0;
    __syncthreads();
    const uint32_t blk0 = blockIdx.x * kSortBlock;
    const uint32_t base = blk0 + w * (64 * kSortItems);
    uint32_t key[kSortItems], val[kSortItems], aux[AUX == 2 ? kSortItems : 1];
    // every load of the workgroup is issued before anything is consumed: clamped indices instead of lane masks
    // (masked loads were waited for one by one: 16 + ~30 dependent round trips per wave, the whole 31 us of this kernel)
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const uint32_t i = min(base + (uint32_t)k * 64u + lane, n - 1u);      // n > 0 here
        key[k] = keys_in[i];
        val[k] = vals_in[i];
        if (AUX == 2) aux[AUX == 2 ? k : 0] = aux_in[i];
    }
    // digit = threadIdx.x (first 256 threads): global base of this workgroup's first item with that digit = items with a
    // smaller digit + the same digit in earlier groups of 32 workgroups (gsup) + in earlier workgroups of this group (ghist)
    const uint32_t d = threadIdx.x & 255u;
    const bool dig = threadIdx.x < 256u;
    const uint32_t sb = blockIdx.x >> kSupShift;
    uint32_t pre = 0, g_tot = 0;
    if (dig) {                                                                   // wave-uniform (waves 0..3)
        uint32_t t[32];
#pragma unroll
        for (uint32_t u = 0; u < 32u; u++) {                                     // <= 31 earlier workgroups of this group
            const uint32_t j = (sb << kSupShift) + u;
            t[u] = ghist[min(j, nblk - 1u) * 256u + d];
        }
        if (nsup <= kSupDirect && kSortThreads >= 512) {
            // the group rows are summed by the upper half of the workgroup (below), which has no digit column of its own
        } else if (nsup <= kSupDirect) {                                         // every group row at once: digit total + earlier groups
            uint32_t g[kSupDirect];
#pragma unroll
            for (uint32_t u = 0; u < kSupDirect; u++) g[u] = gsup[min(u, nsup - 1u) * 256u + d];
#pragma unroll
            for (uint32_t u = 0; u < kSupDirect; u++) { if (u < nsup) g_tot += g[u]; if (u < sb) pre += g[u]; }
        } else {                                                                 // k_radix_supscan ran: exclusive group prefixes + digit totals
            g_tot = gtot[d];
            pre = gsup[(size_t)sb * 256u + d];
        }
#pragma unroll
        for (uint32_t u = 0; u < 32u; u++) if ((sb << kSupShift) + u < blockIdx.x) pre += t[u];
    } else if (nsup <= kSupDirect && kSortThreads >= 512 && threadIdx.x < 512u) {
        uint32_t g[kSupDirect], ge = 0, ga = 0;
#pragma unroll
        for (uint32_t u = 0; u < kSupDirect; u++) g[u] = gsup[min(u, nsup - 1u) * 256u + d];
#pragma unroll
        for (uint32_t u = 0; u < kSupDirect; u++) { if (u < nsup) ga += g[u]; if (u < sb) ge += g[u]; }
        s_gs[0][d] = ge; s_gs[1][d] = ga;                                        // read by thread d after the next barrier
    }
#ifdef GSWT_TRACE
    { unsigned long long sink = key[0] + val[0] + pre; asm volatile("" :: "v"(sink)); }     // the loads have arrived
    GSWT_TR(1, GSWT_NOW())
#endif
    // per-wave digit counts: one LDS add per distinct digit of a 64-item round (see k_radix_hist); the peer masks are kept for
    // the ranking below
    // (a lane's rank among its peers = the peers below it: v_mbcnt on the mask, no (1 << lane) - 1 kept in two registers across the kernel)
    constexpr bool kCachePeers = kSortItems <= 8;       // 16 rounds of masks would cost the 256-thread build a wave per SIMD
    unsigned long long pm[kCachePeers ? kSortItems : 1];
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const bool valid = base + (uint32_t)k * 64u + lane < n;
        const uint32_t dgt = ((key[k] - kmin) >> shift) & mask;
        const unsigned long long peers = match_digit(dgt, valid, nbits);
        if (kCachePeers) pm[k] = peers;
        if (valid && lanes_below(peers) == 0u) atomicAdd(&s_h[w][dgt], (uint32_t)__popcll(peers));
    }
    GSWT_TR(2, GSWT_NOW())
    {
        // exclusive scans over the first 256 threads (the other waves only take part in the barriers): of the digit totals
        // (global bases) and of this block's digit counts (positions inside the block)
        const bool direct = nsup <= kSupDirect && kSortThreads >= 512;
        if (direct) {                                                            // uniform
            __syncthreads();
            if (dig) { pre += s_gs[0][d]; g_tot = s_gs[1][d]; }
        }
        uint32_t inc = wave_incl_scan(g_tot, lane);
        if (dig && lane == 63u) s_w[w] = inc;
        __syncthreads();                                                         // also: the LDS counts are complete
        uint32_t cnt[kSortWaves], blk_cnt = 0;
        if (dig) {
#pragma unroll
            for (int k = 0; k < kSortWaves; k++) { cnt[k] = s_h[k][d]; blk_cnt += cnt[k]; }
        }
        const uint32_t inc2 = wave_incl_scan(blk_cnt, lane);
        if (dig && lane == 63u) s_w2[w] = inc2;
        __syncthreads();
        if (dig) {
            uint32_t wb = 0, wb2 = 0;
            for (uint32_t i = 0; i < w; i++) { wb += s_w[i]; wb2 += s_w2[i]; }
            const uint32_t gbase = wb + inc - g_tot + pre;
            uint32_t lb = wb2 + inc2 - blk_cnt;                                  // start of digit d inside the block
            s_g[d] = gbase - lb;
#pragma unroll
            for (int k = 0; k < kSortWaves; k++) { s_h[k][d] = lb; lb += cnt[k]; }      // per-wave positions inside the block
        }
    }
    __syncthreads();
    GSWT_TR(3, GSWT_NOW())
    // Ranking, 64 items per round: match-any on the digit bits gives every lane its peers; the lowest peer takes the run's
    // position with ONE returning LDS add and hands it to the others through a lane shuffle.  (Round 1 read the counter,
    // fenced the wave, wrote it back and fenced again: two dependent LDS round trips per round that no other round could
    // overlap; the adds of consecutive rounds are independent instructions.)
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        uint32_t i = base + k * 64 + lane;
        bool valid = i < n;
        uint32_t dgt = valid ? (((key[k] - kmin) >> shift) & mask) : 0u;
        const unsigned long long peers = kCachePeers ? pm[kCachePeers ? k : 0] : match_digit(dgt, valid, nbits);
        const uint32_t rank = lanes_below(peers);
        uint32_t pos = 0;
        if (valid && rank == 0u) pos = atomicAdd(&s_h[w][dgt], (uint32_t)__popcll(peers));
        const int leader = valid ? (int)__ffsll((long long)peers) - 1 : (int)lane;
        pos = (uint32_t)__shfl((int)pos, leader, 64);
        if (valid) {
            s_kv[pos + rank] = make_uint2(key[k], val[k]);
            if (AUX == 2) s_aux[AUX == 2 ? pos + rank : 0u] = aux[AUX == 2 ? k : 0];
            if (AUX == 1) s_src[AUX == 1 ? pos + rank : 0u] = (uint16_t)(w * (64u * kSortItems) + (uint32_t)k * 64u + lane);
        }
    }
    __syncthreads();
    GSWT_TR(4, GSWT_NOW())
    const uint32_t n_blk = min((uint32_t)kSortBlock, n - blk0);
#pragma unroll
    for (int k = 0; k < kSortItems; k++) {
        const uint32_t i = (uint32_t)k * kSortThreads + threadIdx.x;
        if (i < n_blk) {
            const uint2 kv = s_kv[i];
            const uint32_t gp = s_g[((kv.x - kmin) >> shift) & mask] + i;
            vals_out[gp] = kv.y;
            if (AUX == 2) aux_out[gp] = s_aux[AUX == 2 ? i : 0u];
            if (AUX == 1) aux_out[gp] = aux_in[blk0 + s_src[AUX == 1 ? i : 0u]];
            if (!ranges) keys_out[gp] = kv.x;
            else {
                // LAST pass of the frame's pair sort: the block in LDS is sorted by the whole key (the passes before ordered the
                // input by the lower digits, stably), so the first and last item of every run of equal keys are neighbours' business --
                // they leave the tile's [start, end) in the sorted pair list: the range words of encode_tile_range, both through atomicMax on
                // the zeroed table, because a tile's run can continue in the next block.  This replaces a pass over the sorted keys (k_ranges,
                // 5 us + a launch at c3), and the sorted keys themselves are not written any more: nothing reads them.
                const uint32_t kp = s_kv[i == 0u ? 0u : i - 1u].x, kn = s_kv[min(i + 1u, n_blk - 1u)].x;
                if (i == 0u || kp != kv.x) atomicMax(&ranges[kv.x].x, tile_range_start_word(gp));
                if (i == n_blk - 1u || kn != kv.x) atomicMax(&ranges[kv.x].y, gp + 1u);
            }
        }
    }
    GSWT_TR(5, GSWT_NOW())
}

// ------------------------------------------------------------------------------------
// Merged-group lists on the device (Scene::sort_raw_depth_vec for every MergedFrom group of a sort event,
// wangtile.rs:595-670 + scene.rs:655-698, in one segmented sort).
//   segment  = one member's raw-depth array (plus the other LOD's when the member is Changing)
//   k_mg_minmax : per group min / max of the concatenated raw depths
//   k_mg_keys   : key = group << 16 | bucket, bucket = clamp(floor((d - min) as f32 * (65535 / (max - min)))),
//                 NaN -> 0 as in Rust's `as i32`; val = position in the concatenation
//   radix sort  : stable on 16 + log2(groups) bits  == the CPU's stable scatter by bucket
//   k_mg_final  : reverse inside each group (`depth_index.reverse()`), map concat position -> gs_index / map id / lod
// ------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mg_find_seg(const MergeSeg* __restrict__ segs, uint32_t n_segs, uint32_t e)
{
    uint32_t lo = 0, hi = n_segs;                     // largest s with segs[s].start <= e
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (segs[mid].start <= e) lo = mid; else hi = mid; }
    return lo;
}

// (a group's mn / mx arrive as INT_MAX / INT_MIN with the event's upload: gswt_set_draws_merge_groups -- until the end of round 4 a
// kernel of its own, k_mg_init, set them: one launch per sort event)
// Both passes over the concatenation run on a block table built with the segments: block = (segment, first entry of up to
// 1024 inside it), so a workgroup reads ONE segment record instead of binary-searching the segment of every entry
// (k_mg_minmax was 75 us for 1.24 M entries that way: nine dependent loads per entry plus per-lane atomics).
__global__ __launch_bounds__(256) void k_mg_minmax(const MergeSeg* __restrict__ segs, const uint2* __restrict__ blocks, const int32_t* __restrict__ raw,
                                                   MergeGroup* __restrict__ groups)
{
    __shared__ int32_t s_mn[4], s_mx[4];
    const uint2 b = blocks[blockIdx.x];
    const MergeSeg sg = segs[b.x];
    int32_t mn = 2147483647, mx = -2147483647 - 1;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t i = b.y + k * 256u + threadIdx.x;
        const int32_t d = raw[sg.src + min(i, sg.len - 1u)];             // clamped, unmasked: the duplicate changes neither min nor max
        mn = min(mn, d); mx = max(mx, d);
    }
    for (int off = 32; off > 0; off >>= 1) { mn = min(mn, __shfl_down(mn, off, 64)); mx = max(mx, __shfl_down(mx, off, 64)); }
    if ((threadIdx.x & 63u) == 0) { s_mn[threadIdx.x >> 6] = mn; s_mx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(&groups[sg.group].mn, min(min(s_mn[0], s_mn[1]), min(s_mn[2], s_mn[3])));
        atomicMax(&groups[sg.group].mx, max(max(s_mx[0], s_mx[1]), max(s_mx[2], s_mx[3])));
    }
}

__global__ __launch_bounds__(256) void k_mg_keys(const MergeSeg* __restrict__ segs, const uint2* __restrict__ blocks, const int32_t* __restrict__ raw,
                                                 const MergeGroup* __restrict__ groups, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const uint2 b = blocks[blockIdx.x];
    const MergeSeg sg = segs[b.x];
    const MergeGroup g = groups[sg.group];
    // scene.rs:669-676: depth_inv = 65535 / (max - min) (f32), bucket = floor((d - min) as f32 * depth_inv) as i32, clamped.
    // Both differences are Rust's wrapping i32 subtractions (a span beyond 2^31 - 1 wraps negative): done in u32 here, where
    // wrapping is defined.
    const float depth_inv = 65535.0f / (float)(int32_t)((uint32_t)g.mx - (uint32_t)g.mn);
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t i = b.y + k * 256u + threadIdx.x;
        if (i >= sg.len) break;
        const int32_t d = raw[sg.src + i];
        const float v = floorf((float)(int32_t)((uint32_t)d - (uint32_t)g.mn) * depth_inv);
        int32_t bk;
        if (v != v) bk = 0;                                  // NaN (max == min: 0 * inf) -> 0
        else if (v >= 2147483648.0f) bk = 2147483647;
        else if (v <= -2147483648.0f) bk = -2147483647 - 1;
        else bk = (int32_t)v;
        bk = min(max(bk, 0), 65535);
        const uint32_t e = sg.start + i;
        keys[e] = (sg.group << 16) | (uint32_t)bk;
        vals[e] = e;
    }
}

__global__ __launch_bounds__(256) void k_mg_final(const MergeSeg* __restrict__ segs, uint32_t n_segs, const MergeGroup* __restrict__ groups,
                                                  const uint32_t* __restrict__ sorted_keys, const uint32_t* __restrict__ sorted_vals,
                                                  uint32_t n_total, uint32_t* __restrict__ merged_list, uint32_t* __restrict__ merged_map)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n_total) return;
    const uint32_t g = sorted_keys[p] >> 16;
    const MergeGroup gr = groups[g];
    const uint32_t out = gr.out_base + (gr.len - 1u - (p - gr.base));      // depth_index.reverse()
    const uint32_t e = sorted_vals[p];
    const MergeSeg sg = segs[mg_find_seg(segs, n_segs, e)];
    merged_list[out] = ((e - sg.start) + sg.gs_offset) | (sg.lod << kLodShift);
    merged_map[out] = sg.map_index;
}

// Groups whose list one of the retained sort events already holds: one workgroup per 1024 entries of a copy job (block table as above).
__global__ __launch_bounds__(256) void k_mg_copy(const MergeCopy* __restrict__ jobs, const uint2* __restrict__ blocks, const uint2* __restrict__ remap,
                                                 const MergeSources src, uint32_t* __restrict__ new_list, uint32_t* __restrict__ new_map)
{
    __shared__ uint2 s_pairs[256];
    const uint2 b = blocks[blockIdx.x];
    const MergeCopy jb = jobs[b.x];
    const uint32_t* __restrict__ old_list = src.list[jb.src_set < (uint32_t)kMergeSources ? jb.src_set : 0u];
    const uint32_t* __restrict__ old_map = src.map[jb.src_set < (uint32_t)kMergeSources ? jb.src_set : 0u];
    const uint32_t np = min(jb.n_pairs, 256u);
    if (threadIdx.x < np) s_pairs[threadIdx.x] = remap[jb.first_pair + threadIdx.x];
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t i = b.y + k * 256u + threadIdx.x;
        if (i >= jb.len) break;
        new_list[jb.dst + i] = old_list[jb.src + i];
        uint32_t m = old_map[jb.src + i];
        for (uint32_t q = 0; q < np; q++) if (s_pairs[q].x == m) { m = s_pairs[q].y; break; }
        new_map[jb.dst + i] = m;
    }
}

// ------------------------------------------------------------------------------------
// [start, end) of each screen tile in the sorted pair list: left by the LAST pass of the pair sort (k_radix_scatter, `ranges`) as
// (~start, end) per tile, (0, 0) for a tile without pairs; k_items decodes it.  (Until the end of round 2 a kernel of its own,
// k_ranges, read the sorted keys back for it: 5 us + a launch at c3, 18 us at c5.)
// ------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------
// k_tile_depth_sort -- GSWT_ORDER_DEPTH, the tile-local path: the pair list has been sorted on the tile bits with each pair's depth bits as
// the payload; one workgroup per screen tile now sorts that tile's slice by depth INSIDE LDS -- a stable LSD radix sort on the bits of
// (depth key - the TILE's smallest key), all passes back to back -- and writes the slots back in place.  Inside a tile: true depth order,
// equal depths in composite order: bit for bit what the global depth passes in front of the tile sort produce, without their three trips
// through HBM, their histogram kernels and their launches.  The ranking is k_radix_scatter's: each wave owns a run of consecutive
// 64-item rounds and ranks them with ballot match-any (in-wave order = list order), per-wave digit counters in LDS, one exclusive scan
// over (digit, wave).  The digit width follows the tile's own key span: `passes` = ceil(bits / 8) digits of ceil(bits / passes) bits.
//
// Four size classes, one launch each (c3: 8 160 screen tiles, 4 679 of them sky; 2 133 lists of up to 512 pairs hold 18 % of the 2.66 M
// pairs, 1 290 of 513 .. 4 096 hold 72 %, 58 longer ones 10 % -- tools/tile_lengths.py):
//   <64, 8, false>    one WAVE per screen tile, lists of up to 512 pairs (5 KB of LDS, no barrier that costs anything)
//   <256, 16, false>  one 256-thread workgroup per tile, 513 .. 4 096 pairs (36 KB); a longer list's tile id goes onto `long_list`
//                     ([0] = count, cleared by k_cull)
//   <1024, 16, true>  a fixed grid that walks long_list: up to 16 384 pairs per list (144 KB of LDS, one workgroup per CU)
//   k_tile_depth_sort_xl (below)  lists beyond that: the same passes through global memory, one workgroup per list of a second list
// (The first build -- one 512-thread / 64-KB workgroup for every tile, 32 unconditional loads per thread -- took 115 us at c3; the classes
// as built here 12.6 + 27.9 + 16.0 us, each with ~4.8 us of launch floor, against 3 x (24.7 + 5.1) us for the global depth passes.  Other
// cuts measured: profiles/r04_depth_sort_variants.txt.)
// ------------------------------------------------------------------------------------
constexpr uint32_t kTileSortCap = 16384u, kTileSortLongGrid = 256u;
// WAVE: one wave of a larger workgroup sorts a list on its own (THREADS = 64): its LDS slices are private and a wave's LDS operations complete
// in order, so the workgroup barriers become compiler-level fences
template <bool WAVE>
__device__ __forceinline__ void tls_sync()
{
    if (WAVE) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    else __syncthreads();
}
template <int THREADS, int ROUNDS, bool LONG, bool WAVE = false>
__device__ __forceinline__ void tile_depth_sort_one(uint32_t tile, const uint2* __restrict__ ranges, uint32_t* __restrict__ vals, const uint32_t* __restrict__ dkeys,
                                                    uint32_t* __restrict__ long_list, uint32_t* __restrict__ xl_list, FrameCounters* __restrict__ counters,
                                                    uint32_t n_lo, bool push, uint2* s_kv, uint32_t (*s_h)[256], uint32_t* s_w, uint32_t* s_mn, uint32_t* s_mx)
{
    constexpr uint32_t CAP = (uint32_t)(THREADS * ROUNDS);
    constexpr int NW = THREADS / 64;
    // (everything the control flow hangs on is read through v_readfirstlane: a value loaded from memory sits in a vector register, and the
    // compiler then predicates every "uniform" branch below with exec-mask nests instead of scalar branches)
    const uint2 rgv = ranges[__builtin_amdgcn_readfirstlane(tile)];  // the tile's range words; (0, 0): no pairs
    const uint32_t rg_x = __builtin_amdgcn_readfirstlane(rgv.x), rg_y = __builtin_amdgcn_readfirstlane(rgv.y);
    if (rg_y == 0u) return;
    const uint32_t start = tile_range_start_word(rg_x), n = rg_y - start;
    if (n <= max(n_lo, 1u)) return;                               // (a shorter list: the class below's)
    if (n > CAP) {                                                // workgroup-uniform
        if ((WAVE ? (threadIdx.x & 63u) : threadIdx.x) == 0u && (LONG || push)) {
            if (LONG) counters->res.rerun = 1ull;                 // (cannot happen: the list only holds what fits)
            else {
                uint32_t* const lst = n > kTileSortCap ? xl_list : long_list;      // beyond the LDS buffer: k_tile_depth_sort_xl
                lst[1u + atomicAdd(&lst[0], 1u)] = tile;
            }
        }
        return;
    }
    static_assert(!WAVE || THREADS == 64, "wave-local mode is one wave");
    const uint32_t lane = threadIdx.x & 63u, w = WAVE ? 0u : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), tid = WAVE ? lane : threadIdx.x;
    const uint32_t rounds = (n + 63u) >> 6, rpw = (rounds + (uint32_t)NW - 1u) / (uint32_t)NW;   // wave w owns rounds [w rpw, (w + 1) rpw)
    const uint32_t base_w = w * rpw * 64u;
    uint32_t key[ROUNDS], val[ROUNDS];
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
    for (int k = 0; k < ROUNDS; k++) {
        key[k] = 0u; val[k] = 0u;
        if ((uint32_t)k >= rpw || base_w + (uint32_t)k * 64u >= n) continue;                      // wave-uniform: this round holds no item
        const uint32_t i = min(base_w + (uint32_t)k * 64u + lane, n - 1u);                         // (the lanes past the end repeat the last item)
        key[k] = dkeys[start + i];
        val[k] = vals[start + i];
        mn = min(mn, key[k]); mx = max(mx, key[k]);
    }
    mn = wave_min(mn); mx = wave_max(mx);
    if (lane == 0u) { s_mn[w] = mn; s_mx[w] = mx; }
    tls_sync<WAVE>();
#pragma unroll
    for (int q = 0; q < NW; q++) { mn = min(mn, s_mn[q]); mx = max(mx, s_mx[q]); }
    mn = __builtin_amdgcn_readfirstlane(mn); mx = __builtin_amdgcn_readfirstlane(mx);
    const uint32_t span = mx - mn;
    if (span == 0u) return;                                       // one depth: the list is in order already
    const uint32_t bits = 32u - (uint32_t)__clz((int)span), passes = (bits + 7u) >> 3, nb = (bits + passes - 1u) / passes, dmask = (1u << nb) - 1u;
#pragma unroll
    for (int k = 0; k < ROUNDS; k++) key[k] -= mn;
    for (uint32_t p = 0; p < passes; p++) {
        const uint32_t shift = nb * p;
        for (uint32_t q = tid; q < (uint32_t)NW * 256u; q += (uint32_t)THREADS) (&s_h[0][0])[q] = 0u;
        tls_sync<WAVE>();                                          // (also: the previous pass's reads of s_kv are done)
        uint32_t pm[ROUNDS];                                     // per round: rank among the peers | first peer's lane << 8 | peers << 16
#pragma unroll
        for (int k = 0; k < ROUNDS; k++) {
            pm[k] = 0u;
            if ((uint32_t)k >= rpw || base_w + (uint32_t)k * 64u >= n) continue;
            const bool valid = base_w + (uint32_t)k * 64u + lane < n;
            const uint32_t dgt = (key[k] >> shift) & dmask;
            const unsigned long long peers = match_digit(dgt, valid, nb);
            const uint32_t rank = lanes_below(peers), cnt = (uint32_t)__popcll(peers);
            pm[k] = rank | (valid ? (uint32_t)(__ffsll((long long)peers) - 1) : lane) << 8 | cnt << 16;
            if (valid && rank == 0u) atomicAdd(&s_h[w][dgt], cnt);
        }
        tls_sync<WAVE>();
        // exclusive scan over (digit, wave): the first 256 threads own one digit each (a one-wave workgroup: four per lane)
        constexpr int SCAN_T = THREADS < 256 ? THREADS : 256, DPT = 256 / SCAN_T;
        uint32_t cnt[DPT][NW], tot = 0, inc = 0;
        const bool dig = tid < (uint32_t)SCAN_T;
        const uint32_t d0 = (tid & (uint32_t)(SCAN_T - 1)) * (uint32_t)DPT;
        if (dig) {
#pragma unroll
            for (int j = 0; j < DPT; j++)
#pragma unroll
                for (int q = 0; q < NW; q++) { cnt[j][q] = s_h[q][d0 + (uint32_t)j]; tot += cnt[j][q]; }
            inc = wave_incl_scan(tot, lane);
            if (lane == 63u) s_w[w] = inc;
        }
        tls_sync<WAVE>();
        if (dig) {
            uint32_t b = inc - tot;
            for (uint32_t q = 0; q < w; q++) b += s_w[q];
#pragma unroll
            for (int j = 0; j < DPT; j++)
#pragma unroll
                for (int q = 0; q < NW; q++) { s_h[q][d0 + (uint32_t)j] = b; b += cnt[j][q]; }
        }
        tls_sync<WAVE>();
        // (measured and dropped: the counter updates, broadcasts and stores of all rounds as three loops instead of one, so that the LDS
        // round trips of different rounds overlap: 35.3 against 30.6 us at c3 for the 256-thread class -- the extra live registers cost a wave)
#pragma unroll
        for (int k = 0; k < ROUNDS; k++) {
            if ((uint32_t)k >= rpw || base_w + (uint32_t)k * 64u >= n) continue;
            const bool valid = base_w + (uint32_t)k * 64u + lane < n;
            const uint32_t dgt = (key[k] >> shift) & dmask;
            uint32_t pos = 0;
            if (valid && (pm[k] & 255u) == 0u) pos = atomicAdd(&s_h[w][dgt], pm[k] >> 16);
            pos = (uint32_t)__shfl((int)pos, (int)((pm[k] >> 8) & 255u), 64) + (pm[k] & 255u);
            if (valid) s_kv[pos] = make_uint2(key[k], val[k]);
        }
        tls_sync<WAVE>();
        if (p + 1u == passes) break;
#pragma unroll
        for (int k = 0; k < ROUNDS; k++) {                        // back into list order for the next pass
            const uint32_t i = base_w + (uint32_t)k * 64u + lane;
            if ((uint32_t)k < rpw && i < n) { const uint2 kv = s_kv[i]; key[k] = kv.x; val[k] = kv.y; }
        }
    }
    for (uint32_t i = tid; i < n; i += (uint32_t)THREADS) vals[start + i] = s_kv[i].y;
}

// tile_depth_sort_xl (k_tile_depth_sort_xl in the documents): the lists that do not fit the LDS buffer (more than 16 384 pairs: c5's horizon tiles hold up to 27 908, a small
// framebuffer in front of a big scene more).  One 1 024-thread workgroup per list (a fixed grid over xl_list, which the 256-thread class
// fills), the same stable LSD passes on (key - the list's smallest key), but the items stay in global memory: a pass counts the digits of
// the list wave by wave (wave w owns one contiguous sixteenth of it, so in-wave order = list order), scans (digit, wave) in LDS, and
// scatters into the other half of the sort's ping-pong buffers (free once the tile passes are done) at the list's own offset; an odd
// number of passes is followed by a copy back.  Two reads of the list per pass instead of none -- a few lists per frame, one per CU, in
// place of three global passes over every pair of the frame (c5: 3 x (22 + 88) us), and no frame is ever re-run for the length of a list.
// Not a launch of its own: the long-list workgroups of k_tile_depth_sort<1024, 16, true> walk this list behind theirs (an empty launch is 4.8 us).
__device__ __forceinline__ void tile_depth_sort_xl(const uint2* __restrict__ ranges, uint32_t* vals_a, uint32_t* keys_a, uint32_t* vals_b,
                                                   uint32_t* keys_b, uint32_t n_tiles, const uint32_t* __restrict__ long_list,
                                                   uint32_t (*s_h)[256], uint32_t* s_w, uint32_t* s_mn, uint32_t* s_mx)
{
    constexpr uint32_t NW = 16u;                                   // (called by the 1 024-thread long-list workgroups behind their own list)
    const uint32_t* const xl_list = long_list + n_tiles + 1u;
    const uint32_t n_xl = min(xl_list[0], n_tiles);                // written by the launch in front of this one
    const uint32_t lane = threadIdx.x & 63u, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t t = blockIdx.x; t < n_xl; t += gridDim.x) {
        const uint2 rgv = ranges[__builtin_amdgcn_readfirstlane(xl_list[1u + t])];
        // (a listed tile has pairs: its start word decodes without the empty case)
        const uint32_t start = tile_range_start_word((uint32_t)__builtin_amdgcn_readfirstlane(rgv.x)), n = (uint32_t)__builtin_amdgcn_readfirstlane(rgv.y) - start;
        const uint32_t per = ((n + NW * 64u - 1u) / (NW * 64u)) * 64u;            // items per wave: whole 64-item rounds
        const uint32_t lo = min(w * per, n), hi = min(lo + per, n);
        // the list's key range
        uint32_t mn = 0xFFFFFFFFu, mx = 0u;
        for (uint32_t i = lo + lane; i < hi; i += 64u) { const uint32_t k = keys_a[start + i]; mn = min(mn, k); mx = max(mx, k); }
        mn = wave_min(mn); mx = wave_max(mx);
        if (lane == 0u) { s_mn[w] = mn; s_mx[w] = mx; }
        __syncthreads();
#pragma unroll
        for (uint32_t q = 0; q < NW; q++) { mn = min(mn, s_mn[q]); mx = max(mx, s_mx[q]); }
        mn = __builtin_amdgcn_readfirstlane(mn); mx = __builtin_amdgcn_readfirstlane(mx);
        const uint32_t span = mx - mn;
        uint32_t passes = 0, nb = 8u;
        if (span != 0u) { const uint32_t bits = 32u - (uint32_t)__clz((int)span); passes = (bits + 7u) >> 3; nb = (bits + passes - 1u) / passes; }
        const uint32_t dmask = (1u << nb) - 1u;
        uint32_t* src_k = keys_a; uint32_t* src_v = vals_a; uint32_t* dst_k = keys_b; uint32_t* dst_v = vals_b;
        for (uint32_t p = 0; p < passes; p++) {
            const uint32_t shift = nb * p;
            for (uint32_t q = threadIdx.x; q < NW * 256u; q += 1024u) (&s_h[0][0])[q] = 0u;
            __syncthreads();
            for (uint32_t r = lo; r < hi; r += 64u) {              // (wave-uniform bounds)
                const bool valid = r + lane < hi;
                const uint32_t dgt = ((src_k[start + min(r + lane, hi - 1u)] - mn) >> shift) & dmask;
                const unsigned long long peers = match_digit(dgt, valid, nb);
                if (valid && lanes_below(peers) == 0u) atomicAdd(&s_h[w][dgt], (uint32_t)__popcll(peers));
            }
            __syncthreads();
            // exclusive scan over (digit, wave): thread d < 256 owns digit d
            uint32_t cnt[NW], tot = 0, inc = 0;
            const bool dig = threadIdx.x < 256u;
            const uint32_t d = threadIdx.x & 255u;
            if (dig) {
#pragma unroll
                for (uint32_t q = 0; q < NW; q++) { cnt[q] = s_h[q][d]; tot += cnt[q]; }
                inc = wave_incl_scan(tot, lane);
                if (lane == 63u) s_w[w] = inc;
            }
            __syncthreads();
            if (dig) {
                uint32_t b = inc - tot;
                for (uint32_t q = 0; q < w; q++) b += s_w[q];
#pragma unroll
                for (uint32_t q = 0; q < NW; q++) { s_h[q][d] = b; b += cnt[q]; }
            }
            __syncthreads();
            for (uint32_t r = lo; r < hi; r += 64u) {
                const bool valid = r + lane < hi;
                const uint32_t i = start + min(r + lane, hi - 1u);
                const uint32_t key = src_k[i], val = src_v[i];
                const uint32_t dgt = ((key - mn) >> shift) & dmask;
                const unsigned long long peers = match_digit(dgt, valid, nb);
                const uint32_t rank = lanes_below(peers);
                uint32_t pos = 0;
                if (valid && rank == 0u) pos = atomicAdd(&s_h[w][dgt], (uint32_t)__popcll(peers));
                pos = (uint32_t)__shfl((int)pos, valid ? (int)__ffsll((long long)peers) - 1 : (int)lane, 64) + rank;
                if (valid) { dst_k[start + pos] = key; dst_v[start + pos] = val; }
            }
            __syncthreads();                                       // (the workgroup's global stores are visible to its own next pass)
            uint32_t* tk = src_k; src_k = dst_k; dst_k = tk;
            uint32_t* tv = src_v; src_v = dst_v; dst_v = tv;
        }
        if (passes & 1u) {                                         // the sorted slots lie in the other buffer: back to where the compositor reads
            for (uint32_t i = threadIdx.x; i < n; i += 1024u) vals_a[start + i] = vals_b[start + i];
        }
        __syncthreads();
    }
}

template <int THREADS, int ROUNDS, bool LONG>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(THREADS == 256 ? 4 : 1, 8))) void k_tile_depth_sort(const uint2* __restrict__ ranges, uint32_t* vals, uint32_t* dkeys,      // (no __restrict__: the last class writes both)
                                                             uint32_t n_tiles, uint32_t* __restrict__ long_list, FrameCounters* __restrict__ counters,
                                                             uint32_t n_lo, uint32_t push, uint32_t* vals_scratch, uint32_t* dkeys_scratch)
{
    constexpr int NW = THREADS / 64;
    __shared__ uint2 s_kv[THREADS * ROUNDS];
    __shared__ uint32_t s_h[NW][256];
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_mn[NW], s_mx[NW];
    if (!LONG) {
        if (blockIdx.x < n_tiles) tile_depth_sort_one<THREADS, ROUNDS, LONG>(blockIdx.x, ranges, vals, dkeys, long_list, long_list + n_tiles + 1u, counters, n_lo, push != 0u, s_kv, s_h, s_w, s_mn, s_mx);
    } else {
        const uint32_t n_long = min(long_list[0], n_tiles);      // written by the launch in front of this one
        for (uint32_t t = blockIdx.x; t < n_long; t += gridDim.x) {
            tile_depth_sort_one<THREADS, ROUNDS, LONG>(long_list[1u + t], ranges, vals, dkeys, long_list, long_list + n_tiles + 1u, counters, n_lo, false, s_kv, s_h, s_w, s_mn, s_mx);
            __syncthreads();                                      // the next list reuses the LDS
        }
        // ... and the lists beyond the LDS buffer, through global memory (dkeys is written there: the pass buffers alternate)
        if (THREADS == 1024) tile_depth_sort_xl(ranges, vals, dkeys, vals_scratch, dkeys_scratch, n_tiles, long_list, s_h, s_w, s_mn, s_mx);
    }
}

// ------------------------------------------------------------------------------------
// k_composite: one workgroup (4 wave64) per work item = (16x16 screen tile, segment of its pair list).
// Wave w owns the 16x4 pixel strip of rows 4w .. 4w+3; inside a wave the four 16-lane groups own the
// four 4x4 sub-blocks of that strip and walk DIFFERENT splats concurrently (the c3 scene averages ~9 covered
// pixels per pair, so a whole wave per splat would leave most lanes idle).
//   stage   : 256 pairs per batch -> LDS (16 KB): the staging lane gathers the 48-B record, unpacks the
//             colour, evaluates the per-(splat, tile) constants F3 and the tile-local pixel-centre box
//   bin     : every wave ballots the batch against its four sub-blocks and appends the hits, in list
//             order, to four wave-private index lists in LDS (mbcnt-compacted byte stores)
//   walk    : counted loop to the longest of the four lists; each group reads its own next index and
//             record (LDS, four distinct addresses per wave), evaluates the canonical per-pixel
//             sequence F4 and blends under predication; a wave whose ballot of "T >= eps" is empty stops
// ------------------------------------------------------------------------------------
// Work items: a tile's pair list is cut into segments of `seg` pairs; item = (tile, segment).
// seg_count[t] = ceil(len / seg): a tile without pairs has no item (k_combine, which visits every tile anyway, writes its background).
// item_base[t] = exclusive scan of seg_count, item_base[n_tiles] = number of items; item_tab[item] =
// (tile, segment << 1 | tile has several segments, first pair, end pair): everything k_composite needs in one load.  Single workgroup (n_tiles is a few thousand to a few
// tens of thousands): one launch instead of count + 3 scan launches.
// GSWT_ORDER_DEPTH (krange != nullptr): also the depth sort's pass check -- depth_passes_needed = 8-bit passes this frame's depth range needs;
// more than were launched = the pair list is not in depth order: the frame is flagged (rerun) and the host re-runs it with more passes.
__global__ __launch_bounds__(1024) void k_items(const uint2* __restrict__ ranges, int n_tiles, uint32_t seg,
                                                uint32_t* __restrict__ item_base, uint4* __restrict__ item_tab, uint32_t max_items,
                                                const uint32_t* __restrict__ krange, uint32_t n_launched, FrameCounters* __restrict__ counters,
                                                uint32_t report_max)
{
    if (krange && blockIdx.x == 0u && threadIdx.x == 0u) {
        const uint32_t need = sort_passes_needed(krange);
        counters->res.depth_passes_needed = need;
        if (need > n_launched) counters->res.rerun = 1ull;
    }
    // One workgroup per 8192 tiles (c3: one workgroup, c5: four).  Thread t owns tiles base + j * 1024 + t, j = 0..7: every
    // load and store of a wave is contiguous (eight tiles per thread SIDE BY SIDE made each of them 64 separate 8-byte
    // requests: ~8 k requests through one CU's address path, the larger part of the old kernel's 14 us).  The eight block
    // scans are batched: eight wave scans back to back, one table of 8 x 16 wave sums, one 128-entry scan of it by wave 0.
    // A workgroup's first item = the segment count of all tiles in front of it, which it sums itself (<= 8 k tiles per
    // earlier workgroup, contiguous reads) instead of waiting for the others: no inter-workgroup dependence.
    constexpr int kPer = 8;
    __shared__ uint32_t s_t[kPer * 16];           // [j][wave]: wave sums, then their exclusive scan in tile order
    __shared__ uint32_t s_tot, s_carry[16];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const int last = n_tiles > 0 ? n_tiles - 1 : 0;
    const bool seg_pow2 = (seg & (seg - 1u)) == 0u;
    const uint32_t seg_sh = (uint32_t)__ffs((int)seg) - 1u;
    const int base = (int)blockIdx.x * 1024 * kPer;
    uint2 r[kPer];
    // (ranges[t] = the range words the last sort pass leaves, decoded in place: r[j] = (start, end), (0, 0) for a tile without pairs)
#pragma unroll
    for (int j = 0; j < kPer; j++) { r[j] = ranges[min(base + j * 1024 + (int)threadIdx.x, last)]; r[j].x = tile_range_start(r[j].x, r[j].y); }
    // segments of the tiles in front of this workgroup
    uint32_t carry = 0;
    if (base > 0) {
        uint32_t part = 0;
        for (int t0 = 0; t0 < base; t0 += 1024 * kPer) {
            uint2 e[kPer];
#pragma unroll
            for (int j = 0; j < kPer; j++) { e[j] = ranges[t0 + j * 1024 + (int)threadIdx.x]; e[j].x = tile_range_start(e[j].x, e[j].y); }      // t0 + 8191 < base <= n_tiles
#pragma unroll
            for (int j = 0; j < kPer; j++) {
                const uint32_t len = e[j].y - e[j].x;
                part += seg_pow2 ? (len + seg - 1u) >> seg_sh : (len + seg - 1u) / seg;
            }
        }
        const uint32_t pi = wave_incl_scan(part, lane);
        if (lane == 63u) s_carry[w] = pi;
        __syncthreads();
        for (uint32_t i = 0; i < 16u; i++) carry += s_carry[i];
    }
    if (report_max) {
        // GSWT_ORDER_DEPTH: the longest tile list of the frame -> max_tile_len: the host picks the tile-local depth sort (lists that
        // fit its LDS buffer) or the global depth passes for the next frames by it
        uint32_t mx = 0;
#pragma unroll
        for (int j = 0; j < kPer; j++) mx = max(mx, base + j * 1024 + (int)threadIdx.x < n_tiles ? r[j].y - r[j].x : 0u);
        mx = wave_max(mx);
        if (lane == 0u && mx) atomicMax(&counters->res.max_tile_len, mx);     // <= 16 per workgroup, <= 4 workgroups
    }
    uint32_t cnt[kPer], inc[kPer];
#pragma unroll
    for (int j = 0; j < kPer; j++) {
        const uint32_t len = r[j].y - r[j].x;
        const uint32_t q = seg_pow2 ? (len + seg - 1u) >> seg_sh : (len + seg - 1u) / seg;   // (a 32-bit divide is ~40 VALU)
        cnt[j] = base + j * 1024 + (int)threadIdx.x < n_tiles ? q : 0u;
    }
#pragma unroll
    for (int j = 0; j < kPer; j++) {
        inc[j] = wave_incl_scan(cnt[j], lane);
        if (lane == 63u) s_t[j * 16 + (int)w] = inc[j];
    }
    __syncthreads();
    if (w == 0u) {                            // exclusive scan of the 128 wave sums, two per lane
        const uint32_t a = s_t[2u * lane], b2 = s_t[2u * lane + 1u];
        const uint32_t pi = wave_incl_scan(a + b2, lane);
        s_t[2u * lane] = pi - a - b2;
        s_t[2u * lane + 1u] = pi - b2;
        if (lane == 63u) s_tot = pi;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPer; j++) {
        const int t = base + j * 1024 + (int)threadIdx.x;
        if (t < n_tiles) {
            const uint32_t first = carry + s_t[j * 16 + (int)w] + inc[j] - cnt[j];
            item_base[t] = first;
            const uint32_t multi = cnt[j] > 1u ? 1u : 0u;
            for (uint32_t k = 0; k < cnt[j] && first + k < max_items; k++) {
                const uint32_t a = r[j].x + k * seg;
                item_tab[first + k] = make_uint4((uint32_t)t, (k << 1) | multi, a, min(r[j].y, a + seg));
            }
        }
    }
    if (threadIdx.x == 0 && base + 1024 * kPer >= n_tiles) item_base[n_tiles] = carry + s_tot;      // the last workgroup
}

#ifdef GSWT_STATS
__device__ unsigned long long g_stats[8];
#define GSWT_STAT_STEP(C) { unsigned long long cm_ = ballot64(C); if ((threadIdx.x & 63u) == 0) { atomicAdd(&g_stats[0], 1ull); \
    atomicAdd(&g_stats[1], (unsigned long long)__popcll(cm_)); if (cm_ == 0ull) atomicAdd(&g_stats[2], 1ull); \
    unsigned z_ = 0; for (int q_ = 0; q_ < 4; q_++) if (((cm_ >> (16 * q_)) & 0xFFFFull) == 0ull) z_++; atomicAdd(&g_stats[6], (unsigned long long)z_); } }
#define GSWT_STAT_BATCH(NMAX, C0, C1, C2, C3) { if ((threadIdx.x & 63u) == 0) { atomicAdd(&g_stats[3], 1ull); atomicAdd(&g_stats[4], (unsigned long long)(NMAX)); \
    atomicAdd(&g_stats[5], (unsigned long long)((C0) + (C1) + (C2) + (C3))); } }
#else
#define GSWT_STAT_STEP(C)
#define GSWT_STAT_BATCH(NMAX, C0, C1, C2, C3)
#endif
// LDS record of a staged pair (two 16-B words; one more dword when a depth buffer is bound):
//   q0 = (iu.x, iu.y, -ku, log2 alpha)   q1 = (iv.x, iv.y, -kv, rgba8 bits)
// alpha rides in the exponent (B = 2^(-r2 log2 e + log2 alpha): one fma + v_exp), the colour stays packed and is
// unpacked by v_cvt_f32_ubyteN in the blend; the accumulators run in 0..255 units and are scaled once at the end.
// COLF (debug draw modes only): colours are floats from the side buffer col_f[slot], staged into a third LDS word.
// Lane geometry of the compositor: wave w owns the 16x4 strip of rows 4w .. 4w+3, 16-lane group g its 4x4 sub-block of columns 4g .. 4g+3.
struct CompLane {
    float lx, ly;                 // tile-local pixel centre of this lane
    int r0;                       // first pixel row (tile-local) of the wave's 16 x 4 strip
    uint32_t lane, grp;
};

constexpr uint32_t kListStride = 264u;     // u16 entries per sub-block list: 256 hits + padding to an even count + 2 of prefetch overrun
constexpr uint32_t kNullRec = 256u;        // LDS record no pixel is ever inside (list padding)

// bin + walk of one staged batch (n pairs in LDS) for one wave; updates the lane's (T, colour) state.
// Wave w owns the 16 x 4 pixel strip of rows 4w .. 4w+3, its 16-lane group g the 4 x 4 sub-block of columns 4g .. 4g+3
// (rows, not quadrants: the splat density varies down the screen, so the four lists of a strip are alike and the
// longest one -- which paces the wave -- is close to their mean: 1.98 M wave-steps against 2.28 M on the c3 frame).
// List entries are LDS byte offsets of the records (u16), padded to an even length with the offset of a null record
// whose r^2 is +inf: the walk needs neither a shift nor an `i < n` test nor a mid-pair exit.
// ZOUT: also blends the splats' depths (s_dep, staged as for the depth test) into az with the colour's weights (gswt_hip.h, depth output).
// PICK: also keeps the lane's largest weight so far (wmax, strict >: the front-most of equal weights stays) and the pair that had it (wpair,
// its index in the sorted pair list; pair_base = the index of the batch's first pair).  Inside the walk the winner is the STEP number -- uniform,
// so the select takes it from an SGPR -- and the step's list entry is looked up once behind the loop (gswt_hip.h, pick output).
template <bool EARLY, bool DEPTH, bool COLF, bool ZOUT, bool PICK>
__device__ __forceinline__ void composite_bin_walk(const Frame& f, const CompLane& g, uint32_t n, const float4* s_q0, const float4* s_q1,
                                                   const float4* s_q2, const uint32_t* s_bb, const float* s_dep, uint16_t* wlist,
                                                   float dbuf, float t_eps, float& T, float& ar, float& ag, float& ab, float& az, bool& wave_live,
                                                   uint32_t pair_base, float& wmax, uint32_t& wpair)
{
    constexpr bool SDEP = DEPTH || ZOUT;                                       // the pairs' depths are staged in s_dep
    const uint32_t lane = g.lane, grp = g.grp;
    const float lx = g.lx, ly = g.ly;
    uint16_t* const my_list = wlist + grp * kListStride;
    // bin: append this batch's hits to the four sub-block lists (list order preserved)
    uint32_t cnt0 = 0, cnt1 = 0, cnt2 = 0, cnt3 = 0;
#pragma unroll
    for (int c = 0; c < (int)(256u / 64u); c++) {
        const uint32_t idx = (uint32_t)c * 64u + lane;
        // the staged hit mask of the pair: this wave's strip is bits r0 .. r0 + 3 (r0 = 4 x strip).  Read unconditionally (idx < 256: a
        // slot past the batch's end holds an older batch's word) and cleared by a select: predicates that come out of an `if` reach the
        // ballots as 0 / 1 registers compared once more -- eight vector instructions per 64 pairs that four v_cmp already answered
        const uint32_t hm_raw = s_bb[idx] >> (uint32_t)g.r0;
        const uint32_t hm = idx < n ? hm_raw : 0u;
        const bool h0 = (hm & 1u) != 0u, h1 = (hm & 2u) != 0u, h2 = (hm & 4u) != 0u, h3 = (hm & 8u) != 0u;
        const unsigned long long m0 = ballot64(h0), m1 = ballot64(h1), m2 = ballot64(h2), m3 = ballot64(h3);
#define GSWT_APPEND(H, M, CNT, G)                                                                                         \
        if (M) {                                                                                                            \
            if (H) wlist[(G) * kListStride + (CNT) + __builtin_amdgcn_mbcnt_hi((uint32_t)((M) >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)(M), 0u))] = (uint16_t)(idx * 16u); \
            CNT += (uint32_t)__popcll(M);                                                                                   \
        }
        GSWT_APPEND(h0, m0, cnt0, 0u) GSWT_APPEND(h1, m1, cnt1, 1u) GSWT_APPEND(h2, m2, cnt2, 2u) GSWT_APPEND(h3, m3, cnt3, 3u)
#undef GSWT_APPEND
    }
    const uint32_t n_mine = grp == 0u ? cnt0 : grp == 1u ? cnt1 : grp == 2u ? cnt2 : cnt3;
    const uint32_t n_max = max(max(cnt0, cnt1), max(cnt2, cnt3));
    GSWT_STAT_BATCH(n_max, cnt0, cnt1, cnt2, cnt3)
    if (n_max == 0u) return;
    // pad this group's list with the null record up to the wave's even step count (+2: the walk reads two entries ahead)
    const uint32_t n_steps = (n_max + 1u) & ~1u;
    for (uint32_t p = n_mine + (lane & 15u); p < n_steps + 2u; p += 16u) my_list[p] = (uint16_t)(kNullRec * 16u);
    // walk: one splat per 16-lane group per step.  Two-deep software pipeline, unrolled x2 so the two record register
    // sets (A, B) never need copying: the list entry is fetched two steps ahead, the record one step ahead.
    const char* const q0b = reinterpret_cast<const char*>(s_q0);
    const char* const q1b = reinterpret_cast<const char*>(s_q1);
    const char* const q2b = reinterpret_cast<const char*>(s_q2);
    const char* const dpb = reinterpret_cast<const char*>(s_dep);
#define GSWT_REC0(O) (*reinterpret_cast<const float4*>(q0b + (O)))
#define GSWT_REC1(O) (*reinterpret_cast<const float4*>(q1b + (O)))
#define GSWT_REC2(O) (*reinterpret_cast<const float4*>(q2b + (O)))
#define GSWT_RECD(O) (*reinterpret_cast<const float*>(dpb + ((O) >> 2)))
#define GSWT_STEP(Q0, Q1, Q2, DV, STEP)                                                             \
    {                                                                                               \
        const float pu_y = fmaf(Q0.y, ly, Q0.z);                                                    \
        const float pv_y = fmaf(Q1.y, ly, Q1.z);                                                    \
        const float ppx = fmaf(Q0.x, lx, pu_y);                                                     \
        const float ppy = fmaf(Q1.x, lx, pv_y);                                                     \
        const float r2 = fmaf(ppy, ppy, ppx * ppx);                                                 \
        bool cover = r2 <= 4.0f;                                                                    \
        if (DEPTH) cover = cover && DV < dbuf;                                                      \
        GSWT_STAT_STEP(cover)                                                                       \
        /* the blend runs under EXEC masking (s_and_saveexec on the coverage mask, skipped when no lane is covered): round 2 predicated it   \
           with a v_cndmask behind a wave-uniform ballot test; one VALU instruction less per step, 95.8 -> 93.0 us at c3 (round 3) */        \
        if (cover) {                                                                                \
            const float e = __builtin_amdgcn_exp2f(fmaf(r2, -1.4426950408889634f, Q0.w));           \
            const float wgt = T * e;                                                                \
            const uint32_t cw = __float_as_uint(Q1.w);                                              \
            ar = fmaf(wgt, COLF ? Q2.x : (float)(cw & 0xFFu), ar);                                  \
            ag = fmaf(wgt, COLF ? Q2.y : (float)((cw >> 8) & 0xFFu), ag);                           \
            ab = fmaf(wgt, COLF ? Q2.z : (float)((cw >> 16) & 0xFFu), ab);                          \
            if (ZOUT) az = fmaf(wgt, DV, az);                                                       \
            if (PICK) { if (wgt > wmax) { wmax = wgt; wstep = (STEP); } }                           \
            T = T - wgt;                                                                            \
        }                                                                                           \
    }
    {
        // (every list entry goes through an empty asm as soon as it is loaded: carried around the loop as a 16-bit value, the compiler
        // masks each one again before using it as an LDS address -- one VALU instruction per step; a 32-bit register it cannot look
        // into stays as ds_read_u16 left it.  c3 97.8 -> 96.5 us under stage events, c3d 450 -> 447.)
        uint32_t kA = my_list[0], kB = my_list[1];
        asm("" : "+v"(kA)); asm("" : "+v"(kB));
        float4 a0 = GSWT_REC0(kA), a1 = GSWT_REC1(kA);
        float4 a2 = make_float4(0.f, 0.f, 0.f, 0.f), b2 = a2;
        if (COLF) a2 = GSWT_REC2(kA);
        float da = SDEP ? GSWT_RECD(kA) : 0.0f, db = 0.0f;
        uint32_t wstep = 0xFFFFFFFFu;                                      // PICK: the step of this batch that raised wmax last (none yet)
        for (uint32_t i = 0; i < n_steps; i += 2u) {
            kA = my_list[i + 2u];                                          // entry of step i+2: issued BEFORE the record reads, so that pinning it
            const float4 b0 = GSWT_REC0(kB), b1 = GSWT_REC1(kB);           // (below) waits for the oldest LDS read only, not for the records behind it
            if (COLF) b2 = GSWT_REC2(kB);
            if (SDEP) db = GSWT_RECD(kB);
            asm("" : "+v"(kA));
            GSWT_STEP(a0, a1, a2, da, i)
            kB = my_list[i + 3u];                                          // entry of step i+3
            a0 = GSWT_REC0(kA); a1 = GSWT_REC1(kA);                        // record of step i+2
            if (COLF) a2 = GSWT_REC2(kA);
            if (SDEP) da = GSWT_RECD(kA);
            asm("" : "+v"(kB));
            GSWT_STEP(b0, b1, b2, db, i + 1u)
        }
        if (PICK) { if (wstep != 0xFFFFFFFFu) wpair = pair_base + ((uint32_t)my_list[wstep] >> 4); }      // entry = 16 x the pair's index in the batch
    }
#undef GSWT_STEP
#undef GSWT_REC0
#undef GSWT_REC1
#undef GSWT_REC2
#undef GSWT_RECD
    // Saturated pixels keep accumulating weights below t_eps (the oracle has no cut at all); the early-out is per wave
    // and per batch: once no pixel of the strip has T >= t_eps the wave stops binning and walking.
    if (EARLY && ballot64(T >= t_eps) == 0ull) wave_live = false;
}

// Measured and dropped in the walk (all bit-identical, c3, base 97 us):
//  * records through ONE ds_read_b32 per two steps + DPP row_newbcast of each dword (LDS cycles per step 9 -> 2): the
//    compiler folds the broadcast into v_cvt_f32_ubyteN but not into v_fmac, +7 VALU per step, 135 us.  LDS-array
//    cycles are not what bounds the walk; every VALU instruction added to a step costs ~5 us of kernel.
//  * geometry A, geometry B, one skip test on (cover A | cover B), blend A, blend B in one basic block (more ILP:
//    tools/ubench/valu_issue.hip measures 4.8 cycles per dependent v_fma per SIMD at 8 waves, 2.9 with two independent
//    chains): the compiler sinks the record prefetch to the loop top and splits the .w dwords into extra ds_read_b32
//    inside the blend, exposing two LDS latencies per iteration: 126 us.  Without any skip test: 97 us (no gain).  With
//    the pipeline restored by hand (four record sets ping-pong, the next PAIR's records in flight, steps padded to a
//    multiple of 4): the intended schedule in the ISA, but 81 VGPRs = 5 waves per SIMD: 105 us.
//  * XCD-grouped item order (segments of a tile and x-neighbour tiles on one XCD, groups of 2..16): 96.4 - 97.7 us; the
//    record gathers are not what bounds the kernel either.
//  (Occupancy matters here: one workgroup per CU LESS -- LDS padded -- costs 5 % of the frame rate.  The eighth came from the
//  pixel boxes as four signed bytes (LDS 20.8 -> 17.9 KB) plus, to get from 69 to 63 VGPRs without spills: the prefetched record
//  trimmed to the ten words the staging uses, the tile origin and the wave index through readfirstlane (SGPRs), and the output
//  pixel recomputed at the end from an opaque copy of the thread id.  c3 3990 -> 4078, c3h 3555 -> 3685 frames/s on one box.
//  The depth / float-colour variants need 71-72 VGPRs and stay at 7 waves: forcing 8 spilled loop invariants to scratch.)
// Measured and dropped: the same compositor as a PERSISTENT grid (one workgroup walks many items, the gathers of the next
// item's first batch in flight during the current item's walk; items dealt by weight class, boustrophedon, so that the
// busiest workgroup is 3 % above the mean).  Bit-identical output, 142 us against 114 us: the time goes with the number
// of resident workgroups (2 / 4 / 6 per CU: 262 / 167 / 143 us), i.e. the kernel is bound by the walk's per-wave
// progress (VALU 50 us + LDS 53 us + SALU 42 us of issue that do not overlap perfectly, two barriers per batch), and
// the gather latency was already covered by the other workgroups of the CU.  "stage-only 58 us" in the ablation is
// what staging costs with nothing to hide behind, not a serial share of the full kernel.

// The store of a final pixel (comp_final_pixel) in an 8-bit output format (gswt_hip.h, GSWT_OUT_*; kOutF32 stores the float4 as it is).
// Per channel q(x) = round_half_even(min(max(x, 0), 1) * 255) -- fmaxf drops a NaN (-> 0),
// the product is one binary32 multiplication (-ffp-contract=off), v_rndne_f32 rounds half to even, the integral result converts exactly --,
// packed into ONE 32-bit store per lane: the 16 lanes of a pixel row of the tile (the lane -> pixel map) write 64 contiguous bytes.  (The
// compiler folds the clamp into the blend's final v_fma_f32 as its clamp modifier, which also takes NaN to 0.)
__device__ __forceinline__ uint32_t unorm8(float x) { return (uint32_t)__builtin_rintf(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f); }
template <int OUTF>
__device__ __forceinline__ void store_unorm8(float4* out, size_t i, const float4& o)
{
    static_assert(OUTF == kOutRGBA8 || OUTF == kOutBGRA8, "8-bit formats only");
    const uint32_t r = unorm8(o.x), g = unorm8(o.y), b = unorm8(o.z), a = unorm8(o.w);
    reinterpret_cast<uint32_t*>(out)[i] = OUTF == kOutBGRA8 ? (b | g << 8 | r << 16 | a << 24) : (r | g << 8 | b << 16 | a << 24);
}

// The store of a final pixel in a 4:2:0 video format (gswt_hip.h, GSWT_VIDEO_*: BT.709, limited range), at (row, col) of this shard's
// rows x out_w image; every operation is the one binary32 operation the header writes, in its order.  Luma: one byte per lane.  Chroma: the
// lane -> pixel map (lx = (lane >> 4) * 4 + (lane & 3), ly = wave * 4 + ((lane & 15) >> 2)) puts the 2x2 block of an even (row, col) in
// lanes l, l ^ 1, l ^ 4, l ^ 5 of one 16-lane DPP row, so the block's mean takes two DPP moves per component and no LDS: quad_perm [1,0,3,2]
// adds the horizontal neighbour (l ^ 1), row_shl:4 hands lane l the sum of lane l + 4 (= l ^ 4 for the block's top lanes, whose bit 2 is
// clear), and the top-left lane stores.  rows and out_w are even and the image's origin in the frame is a multiple of the tile, so a block is
// wholly inside the frame or wholly outside: all four of its lanes reach this store together (every caller's bounds test removes
// whole blocks).
template <int CTRL>
__device__ __forceinline__ float dpp_move_f32(float x)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float block_mean_2x2(float c)
{
    const float h = c + dpp_move_f32<0xB1>(c);               // quad_perm:[1,0,3,2]: c00 + c01 in the top lanes, c10 + c11 in the bottom ones
    return (h + dpp_move_f32<0x104>(h)) * 0.25f;            // row_shl:4: (c00 + c01) + (c10 + c11) in the top lanes
}
template <int OUTF>
__device__ __forceinline__ void store_video(float4* out, int rows, int out_w, int row, int col, bool inside, const float4& o)
{
    static_assert(OUTF == kOutNV12 || OUTF == kOutI420, "video formats only");
    const float r = fminf(fmaxf(o.x, 0.0f), 1.0f), g = fminf(fmaxf(o.y, 0.0f), 1.0f), b = fminf(fmaxf(o.z, 0.0f), 1.0f);
    const float yl = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    const uint32_t y8 = (uint32_t)__builtin_rintf(16.0f + 219.0f * yl);
    constexpr float kCb = (float)(1.0 / 1.8556), kCr = (float)(1.0 / 1.5748);
    const float mb = block_mean_2x2((b - yl) * kCb), mr = block_mean_2x2((r - yl) * kCr);
    if (!inside) return;
    uint8_t* const plane_y = reinterpret_cast<uint8_t*>(out);
    plane_y[(size_t)row * out_w + col] = (uint8_t)y8;
    if (((row | col) & 1) != 0) return;
    const uint32_t cb8 = (uint32_t)__builtin_rintf(128.0f + 224.0f * mb), cr8 = (uint32_t)__builtin_rintf(128.0f + 224.0f * mr);
    uint8_t* const plane_c = plane_y + (size_t)rows * out_w;
    if constexpr (OUTF == kOutNV12) {
        // (row / 2) * out_w + col: the pair's byte offset, even
        *reinterpret_cast<uint16_t*>(plane_c + (size_t)(row >> 1) * out_w + col) = (uint16_t)(cb8 | cr8 << 8);
    } else {
        const size_t half_w = (size_t)(out_w >> 1), ci = (size_t)(row >> 1) * half_w + (col >> 1);
        plane_c[ci] = (uint8_t)cb8;
        plane_c[(size_t)(rows >> 1) * half_w + ci] = (uint8_t)cr8;
    }
}

// ---- the pieces k_composite and k_combine share: one statement each, so that the two stay bit-identical ----
// Where a work item's screen tile lies: tile row tyl inside this shard's image (the rows it stores) and pixel origin (bx, by) in the frame
// (a row-sharded ctx owns tile rows shard_index, + shard_count, ...)
struct CompTile { int tyl, bx, by; };
__device__ __forceinline__ CompTile comp_tile(const Frame& f, uint32_t tile)
{
    int tx, tyl;
    tile_xy(f, tile, tx, tyl);
    const int sc = f.shard_count <= 1 ? 1 : f.shard_count;
    const int ty = tyl * sc + (sc > 1 ? f.shard_index : 0);
    return {tyl, (tx + f.col0) * kTile, ty * kTile};
}

// Stages one pair for the bin + walk: its LDS record at index `at` (s_q0, s_q1; s_dep with a depth buffer, s_q2 with float colours) and
// its sub-block mask at s_bb[bi], from the first two quads of its Rec (ra, rb), its depth rbw and its float colour rd.  (hW, hHn, c0x, c0y):
// the tile's half of F3 (k_composite).
template <bool DEPTH, bool COLF>
__device__ __forceinline__ void comp_stage(float hW, float hHn, float c0x, float c0y, const float4& ra, const float4& rb, float rbw, const float4& rd,
                                           float4* s_q0, float4* s_q1, float4* s_q2, float* s_dep, uint32_t* s_bb, uint32_t at, uint32_t bi)
{
    // F3: per-(splat, tile) constants
    const float ox = fmaf(hW, rb.x, c0x), oy = fmaf(hHn, rb.y, c0y);
    const float nku = -fmaf(ra.x, ox, ra.y * oy);
    const float nkv = -fmaf(ra.z, ox, ra.w * oy);
    const float l2a = __builtin_amdgcn_logf(rb.z);                           // v_log_f32 = log2; log2(0) = -inf -> B = 0
    s_q0[at] = make_float4(ra.x, ra.y, nku, l2a);
    s_q1[at] = make_float4(ra.z, ra.w, nkv, rb.w);
    // Pixel half extents of |p| <= 2 from the inverse map: the quad axes are u = iu / |iu|^2, w = iv / |iv|^2 and the
    // box is 2 sqrt(u.x^2 + w.x^2) by 2 sqrt(u.y^2 + w.y^2).  Approximate reciprocals / roots (1 ulp) under a 1e-4
    // relative + 2e-3 px margin: the box only has to CONTAIN every pixel centre with r^2 <= 4 (it decides which
    // sub-block lists a pair enters, never a pixel's coverage), and k_project's own box decided the pair's tiles.
    const float ria = __builtin_amdgcn_rcpf(fmaf(ra.y, ra.y, ra.x * ra.x)), rib = __builtin_amdgcn_rcpf(fmaf(ra.w, ra.w, ra.z * ra.z));
    const float qux = ra.x * ria, quy = ra.y * ria, qwx = ra.z * rib, qwy = ra.w * rib;
    const float bhx = fmaf(2.0f * __builtin_amdgcn_sqrtf(fmaf(qwx, qwx, qux * qux)), 1.0001f, 0.002f);
    const float bhy = fmaf(2.0f * __builtin_amdgcn_sqrtf(fmaf(qwy, qwy, quy * quy)), 1.0001f, 0.002f);
    // Pixel box, tile-local, as the integer pixel ranges whose centres it holds: x_lo <= k + 0.5  <=>  ceil(x_lo - 0.5) <= k and
    // x_hi >= k + 0.5  <=>  floor(x_hi - 0.5) >= k for every integer k (x - 0.5 is exact in binary32 wherever the
    // outcome can depend on it), so the byte form bins exactly like the float box did; 16 -> 4 bytes of LDS per pair.
    // Clamped to [-2, 17]: only 0..15 are ever compared.
    const int xa = min(max((int)ceilf((ox - bhx) - 0.5f), -2), 17), xb = min(max((int)floorf((ox + bhx) - 0.5f), -2), 17);
    const int ya = min(max((int)ceilf((oy - bhy) - 0.5f), -2), 17), yb = min(max((int)floorf((oy + bhy) - 0.5f), -2), 17);
    // The 16 sub-blocks the box touches, as a bit mask (bit 4 s + g: strip s, column group g), computed ONCE here instead of four
    // column and one row test per wave and pair in the bin loop: columns g with 4 g + 3 >= xa and 4 g <= xb are g_lo .. g_hi,
    // g_lo = max(xa >> 2, 0), g_hi = min(xb >> 2, 3) (arithmetic shifts: xa, xb in [-2, 17]); rows likewise; the outer product of the
    // two 4-bit masks is one multiplication (the row bits spread to positions 0, 4, 8, 12: no carries).
    const int gx0 = max(xa >> 2, 0), gx1 = min(xb >> 2, 3), gy0 = max(ya >> 2, 0), gy1 = min(yb >> 2, 3);
    const uint32_t cx = gx1 >= gx0 ? (2u << gx1) - (1u << gx0) : 0u;
    const uint32_t ry = gy1 >= gy0 ? (2u << gy1) - (1u << gy0) : 0u;
    const uint32_t spread = (ry & 1u) | ((ry & 2u) << 3) | ((ry & 4u) << 6) | ((ry & 8u) << 9);
    s_bb[bi] = cx * spread;
    if (DEPTH) s_dep[at] = rbw;
    if (COLF) s_q2[at] = rd;
}

// The null record at LDS index `at` (list padding): p.x = +inf for every pixel (0 * l + inf), so r^2 = +inf and no pixel is ever inside
template <bool DEPTH, bool COLF>
__device__ __forceinline__ void comp_null_record(float4* s_q0, float4* s_q1, float4* s_q2, float* s_dep, uint32_t at)
{
    s_q0[at] = make_float4(0.f, 0.f, __builtin_inff(), 0.f);
    s_q1[at] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (DEPTH) s_dep[at] = 0.0f;
    if (COLF) s_q2[at] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// A final pixel (px, py inside the frame): the background under the transmittance left, stored in format OUTF at row orow of this shard's
// image (rows from out_rows on pad the last tile row: not stored).  ZOUT: the depth az blended over the background depth z_bg (the proxy's
// bg_depth, 1.0 = the clear value without one) the same way, Z = T z_bg + az, stored as f32 at the same place of out_depth.
template <int OUTF, bool ZOUT>
__device__ __forceinline__ void comp_final_pixel(const Frame& f, const float4* bg_rgba, float4* out, int out_rows, int px, int py, int orow,
                                                 float T, float ar, float ag, float ab, const float* bg_depth, float* out_depth, float az)
{
    if constexpr (ZOUT) {
        const float zb = bg_depth ? bg_depth[(size_t)py * f.width + px] : 1.0f;
        if (orow < out_rows) out_depth[(size_t)orow * f.out_w + (px - f.out_x0)] = fmaf(T, zb, az);
    }
    float4 bg = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bg_rgba) bg = bg_rgba[(size_t)py * f.width + px];
    float4 o;
    o.x = fmaf(T, bg.x, ar);
    o.y = fmaf(T, bg.y, ag);
    o.z = fmaf(T, bg.z, ab);
    o.w = fmaf(T, bg.w, 1.0f - T);
    if constexpr (OUTF == kOutF32) { if (orow < out_rows) out[(size_t)orow * f.out_w + (px - f.out_x0)] = o; }
    else if constexpr (out_is_video(OUTF)) store_video<OUTF>(out, out_rows, f.out_w, orow, px - f.out_x0, orow < out_rows, o);
    else if (orow < out_rows) store_unorm8<OUTF>(out, (size_t)orow * f.out_w + (px - f.out_x0), o);
}

// The pick of a final pixel (px, py inside the frame), stored at row orow of this shard's pick image as k_pick_resolve expects it: a hit as
// (pair, 0, 0, weight > 0) -- the pair's index in the sorted list, resolved in place afterwards --, a pixel no splat covers as the final no-hit
// record (~0, ~0, z_bg, 0), z_bg as the depth image has it.
__device__ __forceinline__ void comp_final_pick(const Frame& f, const float* bg_depth, uint4* out_pick, int out_rows, int px, int py, int orow,
                                                float wmax, uint32_t wpair)
{
    if (orow >= out_rows) return;
    uint4 o = make_uint4(wpair, 0u, 0u, __float_as_uint(wmax));
    if (!(wmax > 0.0f)) o = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, __float_as_uint(bg_depth ? bg_depth[(size_t)py * f.width + px] : 1.0f), 0u);
    out_pick[(size_t)orow * f.out_w + (px - f.out_x0)] = o;
}

// OUTF: the output format (kOut*); only the final store differs.  ZOUT: the frame also writes its depth image (out_depth; a multi-segment
// item leaves its partial depth in partials_z): the pairs' depths are staged as for the depth test, whether or not they are also tested.
// PICK: the frame also writes its pick image (out_pick, raw: comp_final_pick; a multi-segment item leaves its (largest weight, pair) in
// partials_pick).  No staging of its own: the winner's depth is read by k_pick_resolve.
template <bool EARLY, bool DEPTH, bool COLF, int OUTF, bool ZOUT, bool PICK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((DEPTH || COLF || ZOUT) ? 7 : 8, 8))) void k_composite(const Frame f, const uint2* __restrict__ ranges,
                                                   const uint32_t* __restrict__ item_base, const uint4* __restrict__ item_tab,
                                                   uint32_t seg, const uint32_t* __restrict__ vals, const Rec* __restrict__ recs,
                                                   const float* __restrict__ depths, const float4* __restrict__ col_f,
                                                   const float4* __restrict__ bg_rgba, const float* __restrict__ bg_depth,
                                                   float4* __restrict__ out, float4* __restrict__ partials,
                                                   int n_tiles, int out_rows, float* __restrict__ out_depth, float* __restrict__ partials_z,
                                                   uint4* __restrict__ out_pick, uint2* __restrict__ partials_pick)
{
    __shared__ float4 s_q0[257], s_q1[257];                     // [256] = the null record (list padding)
    __shared__ uint32_t s_bb[256];                              // the 16 sub-blocks a staged pair's pixel box touches (bit 4 strip + column group)
    __shared__ float4 s_q2[COLF ? 257 : 1];
    __shared__ float s_dep[(DEPTH || ZOUT) ? 257 : 1];
    __shared__ uint16_t s_list[4][4][kListStride];     // [wave][sub-block][i] -> LDS byte offset of the i-th hit's record
    __shared__ uint4 s_dead;                           // EARLY: .x .. .w = wave 0 .. 3 has no pixel with T >= t_eps left
    // work item -> (tile, segment) through the table k_items left behind.  Consecutive items are dealt
    // round-robin over the 8 XCDs by the dispatcher, which balances the skewed tile-list lengths.
    const uint32_t item = blockIdx.x;
#ifdef GSWT_TRACE
    const bool tr_on = threadIdx.x == 0 && item < kTraceItems;
    const uint32_t tr_item = item;
    unsigned long long tr_walk = 0;
    bool tr_first = true;
    GSWT_TR(0, GSWT_NOW())
#endif
    const uint32_t n_items = item_base[n_tiles];
    const uint4 it = item_tab[item];                 // (in flight together with n_items; garbage past n_items, unused)
    if (item >= n_items) return;
    GSWT_TR(1, GSWT_NOW())
    GSWT_TR(4, it.w - it.z)
#ifdef GSWT_TRACE
    { unsigned hwid, xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid)); asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc)); GSWT_TR(7, (unsigned long long)hwid | ((unsigned long long)xcc << 32)) }
#endif
    const int tile = (int)it.x;
    const bool multi_seg = (it.y & 1u) != 0u;
    const auto [tyl, bx, by] = comp_tile(f, (uint32_t)tile);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));      // uniform per wave: everything derived from it stays scalar
    const uint32_t grp = lane >> 4, gi = lane & 15u;                 // wave = 16 x 4 strip, 16-lane group = 4 x 4 sub-block
    const int lxi = (int)grp * 4 + (int)(gi & 3u), lyi = (int)wave * 4 + (int)(gi >> 2);
    const int px = bx + lxi, py = by + lyi;
    const bool inside = px < f.width && py < f.height;
    const float lx = (float)lxi + 0.5f, ly = (float)lyi + 0.5f;
    // tile origin as floats: uniform, kept in SGPRs (a v_cvt of a scalar would park them in two VGPRs for the whole kernel)
    const float fbx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int((float)bx)));
    const float fby = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int((float)by)));
    // F3 (sequence v3): centre - tile origin = fma(W/2, ndc.x, W/2 - bx), fma(-H/2, ndc.y, H/2 - by): ONE rounding at the magnitude of the
    // offset; W/2 - bx and H/2 - by are exact and uniform (SGPRs)
    const float hW = 0.5f * f.W, hHn = -0.5f * f.H;
    const float c0x = hW - fbx, c0y = 0.5f * f.H - fby;
    uint16_t* const wlist = &s_list[wave][0][0];
    const CompLane cl = {lx, ly, (int)(wave * 4u), lane, grp};
    const uint2 rg = make_uint2(it.z, it.w);         // this item's slice of the tile's pair list
    // Transmittance doubles as the "still active" state: a lane is live while T >= t_eps.  Pixels
    // outside the target start at T = 0 when early-out is on (never live); with t_eps = 0 they just
    // accumulate and are never stored.
    float T = (EARLY && !inside) ? 0.0f : 1.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, az = 0.0f;
    float dbuf = 1.0f;
    if (DEPTH && inside) dbuf = bg_depth[(size_t)py * f.width + px];
    const float t_eps = f.t_eps;
    bool wave_live = true;
    float wmax = 0.0f;                               // PICK: the largest weight of the item so far and its pair
    uint32_t wpair = 0u;
    if (tid == 0) {
        if (EARLY) s_dead = make_uint4(0u, 0u, 0u, 0u);
        comp_null_record<DEPTH || ZOUT, COLF>(s_q0, s_q1, s_q2, s_dep, kNullRec);
    }
    // Software-pipelined gather: the records of batch b+1 and the slot indices of batch b+2 are in flight
    // while batch b is binned and walked (two dependent HBM latencies per batch otherwise sit between barriers).
    // The loads are unconditional with clamped indices (lanes past the end re-read the last pair and never stage
    // it): a load under a lane mask would be merged back through register copies that wait for it on the spot.
    // (only the words the staging needs are kept in registers: the depth word rides along with a depth buffer only, the
    // pad word of the third quad never)
    float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra, rd = ra;
    float rbw = 0.f;
#define GSWT_LOAD_REC(SLOT)                                                                          \
        {                                                                                           \
            const float4* rp = reinterpret_cast<const float4*>(recs + (SLOT));                      \
            ra = rp[0];                                                                             \
            rb = rp[1];                                                                             \
            if (DEPTH || ZOUT) rbw = depths[(SLOT)];                                                \
        }
    uint32_t slot_nxt = 0;
    const uint32_t last_pair = rg.y - 1u;
    if (rg.x < rg.y) {
        const uint32_t slot0 = vals[min(rg.x + tid, last_pair)];
        GSWT_LOAD_REC(slot0)
        if (COLF) rd = col_f[slot0];
        slot_nxt = vals[min(rg.x + 256u + tid, last_pair)];
    }
    for (uint32_t base = rg.x; base < rg.y; base += 256u) {
        const uint32_t n = min(256u, rg.y - base);
        if (tid < n) comp_stage<DEPTH || ZOUT, COLF>(hW, hHn, c0x, c0y, ra, rb, rbw, rd, s_q0, s_q1, s_q2, s_dep, s_bb, tid, tid);
        __syncthreads();
#ifdef GSWT_TRACE
        if (tr_first) { GSWT_TR(2, GSWT_NOW()) tr_first = false; }
        const unsigned long long tr_t0 = GSWT_NOW();
#endif
        {
            GSWT_LOAD_REC(slot_nxt)
            if (COLF) rd = col_f[slot_nxt];
            slot_nxt = vals[min(base + 512u + tid, last_pair)];
        }
        if (wave_live)
            composite_bin_walk<EARLY, DEPTH, COLF, ZOUT, PICK>(f, cl, n, s_q0, s_q1, s_q2, s_bb, s_dep, wlist, dbuf, t_eps, T, ar, ag, ab, az, wave_live,
                                                                     base, wmax, wpair);
#ifdef GSWT_TRACE
        tr_walk += GSWT_NOW() - tr_t0;
#endif
        if (base + 256u >= rg.y) break;                     // last batch of the item: nothing is staged after it, no barrier needed
        // EARLY: the item ends once all four strips are saturated.  A saturated wave leaves a flag in LDS in front of the batch's closing
        // barrier and everybody reads the four flags behind it (flags are written between a batch's two barriers and read between
        // batches: no race; they never go back to 0).  Until the end of round 4 this was __syncthreads_and(): a workgroup reduction with
        // a second barrier per batch, which made the early-out cost 1.5 % of c3's frame rate, where it saves nothing.
        if (EARLY && !wave_live && lane == 0u) (&s_dead.x)[wave] = 1u;
        __syncthreads();
        if (EARLY) {
            const uint4 dd = s_dead;
            if (__builtin_amdgcn_readfirstlane((int)(dd.x & dd.y & dd.z & dd.w)) != 0) break;
        }
    }
    GSWT_TR(3, GSWT_NOW())
    GSWT_TR(6, tr_walk)
    const float k255 = 1.0f / 255.0f;      // colour is continuous: sum(w * byte) / 255 vs sum(w * (byte / 255)) differ in the last bits only
    if (!COLF) { ar *= k255; ag *= k255; ab *= k255; }
    if (multi_seg) {
        // partial (C, T) of this segment, in the slot the tile's first + the segment's number; k_combine folds the segments front to back
        const size_t pi = (size_t)(item_base[tile] + (it.y >> 1)) * 256u + tid;
        partials[pi] = make_float4(ar, ag, ab, T);
        if (ZOUT) partials_z[pi] = az;
        if (PICK) partials_pick[pi] = make_uint2(__float_as_uint(wmax), wpair);
        return;
    }
    // pixel coordinates again, from a copy of the thread id the compiler cannot connect to the one above: otherwise px, py
    // and the output row stay in VGPRs across the whole walk (the kernel sits exactly at the 64-VGPR / 8-wave limit)
    uint32_t tid2 = threadIdx.x;
    asm volatile("" : "+v"(tid2));
    const int lxi2 = (int)(((tid2 & 63u) >> 4) * 4u + (tid2 & 3u)), lyi2 = (int)((tid2 >> 6) * 4u + ((tid2 & 15u) >> 2));
    const int px2 = bx + lxi2, py2 = by + lyi2;
    if (px2 < f.width && py2 < f.height) {
        if constexpr (PICK) comp_final_pick(f, bg_depth, out_pick, out_rows, px2, py2, tyl * kTile + lyi2, wmax, wpair);
        comp_final_pixel<OUTF, ZOUT>(f, bg_rgba, out, out_rows, px2, py2, tyl * kTile + lyi2, T, ar, ag, ab, bg_depth, out_depth, az);
    }
}

// Measured and dropped again in round 2 (the item STREAM: a resident grid of workgroups, each taking items b, b + G, b + 2G, ...
// as single 256-pair batches with the next item's records and the one-after-next item's slot indices in flight while it bins
// and walks the current one -- the batch pipeline above carried across items; bit-identical output): c3 120 us at 7 workgroups
// per CU (72 VGPRs), 133 us at 8 (64 VGPRs, 20 spilled), 146 / 174 us at 4 per CU, against 96 us for one workgroup per item.
// The phases of this kernel add up (round-2 ablations at c3: 15 us launch + output, 28 us record gathers, 2.5 us binning,
// 50 us walk), but hiding the gathers behind another item's walk inside a workgroup is not what makes them overlap: the
// dispatcher's dynamic hand-out of ~16 k short workgroups does that better than a static stride over them.

// Folds the per-segment partials of multi-segment tiles: (C1,T1) o (C2,T2) = (C1 + T1*C2, T1*T2).
// One workgroup per tile, same lane -> pixel map as k_composite.  ZOUT: the partial depths fold like a colour channel (Z1 + T1*Z2).
// PICK: a segment walks from T = 1, so its largest local weight w' is its candidate and T_prefix * w' that candidate's weight in the pixel: the
// fold keeps the largest, front to back with a strict > (gswt_hip.h, pick output).
template <int OUTF, bool ZOUT, bool PICK>
__global__ __launch_bounds__(256) void k_combine(const Frame f, const uint32_t* __restrict__ item_base,
                                                 const float4* __restrict__ partials, const float4* __restrict__ bg_rgba,
                                                 float4* __restrict__ out, int n_tiles, int out_rows,
                                                 const FrameCounters* __restrict__ counters, FrameResult* __restrict__ host_counters,
                                                 const float* __restrict__ partials_z, const float* __restrict__ bg_depth, float* __restrict__ out_depth,
                                                 const uint2* __restrict__ partials_pick, uint4* __restrict__ out_pick)
{
    const int tile = blockIdx.x;
    // last kernel of a frame without a pick image (k_pick_resolve follows otherwise; the host reads the words behind the frame's final event
    // either way): the frame's result (FrameResult) goes straight into the slot's pinned host words (instead of a
    // separate device-to-host copy, ~4 us of stream time and one more API call per frame)
    if (tile == 0 && threadIdx.x < kFrameResultWords64 && host_counters) copy_frame_result_word(host_counters, counters, threadIdx.x);
    const uint32_t i0 = item_base[tile], n_seg = item_base[tile + 1] - i0;
    if (n_seg == 1u) return;                      // the tile's only work item wrote the pixels itself; n_seg == 0: no pairs, background only
    const auto [tyl, bx, by] = comp_tile(f, (uint32_t)tile);
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t grp = lane >> 4, gi = lane & 15u;      // same lane -> pixel map as k_composite
    const int lxi = (int)grp * 4 + (int)(gi & 3u);
    const int lyi = (int)wave * 4 + (int)(gi >> 2);
    const int px = bx + lxi, py = by + lyi;
    if (px >= f.width || py >= f.height) return;
    float T = 1.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, az = 0.0f;
    float wmax = 0.0f;
    uint32_t wpair = 0u;
    // eight segments' partials in flight together (clamped, unmasked): a horizon tile of c5 has 40 segments, and one dependent
    // 4-KB load per segment made the longest tile the kernel's duration (59 us at c5)
    for (uint32_t s0 = 0; s0 < n_seg; s0 += 8u) {
        float4 p[8];
        float pz[8];
        uint2 pp[8];
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) {
            const size_t pi = (size_t)(i0 + min(s0 + k, n_seg - 1u)) * 256u + tid;
            p[k] = partials[pi];
            if (ZOUT) pz[k] = partials_z[pi];
            if (PICK) pp[k] = partials_pick[pi];
        }
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) {
            if (s0 + k < n_seg) {                 // workgroup-uniform
                ar = fmaf(T, p[k].x, ar);
                ag = fmaf(T, p[k].y, ag);
                ab = fmaf(T, p[k].z, ab);
                if (ZOUT) az = fmaf(T, pz[k], az);
                if (PICK) {
                    const float wc = T * __uint_as_float(pp[k].x);
                    if (wc > wmax) { wmax = wc; wpair = pp[k].y; }
                }
                T = T * p[k].w;
            }
        }
    }
    if constexpr (PICK) comp_final_pick(f, bg_depth, out_pick, out_rows, px, py, tyl * kTile + lyi, wmax, wpair);
    comp_final_pixel<OUTF, ZOUT>(f, bg_rgba, out, out_rows, px, py, tyl * kTile + lyi, T, ar, ag, ab, bg_depth, out_depth, az);
}

// The raw pick image of the compositors -> the public records (gswt_pick), in place, one lane per output pixel.  A raw hit (weight > 0)
// names a pair of the sorted list `vals` the compositor walked: pair -> slot -> draw (chunk_tab) -> the list word at k_project's address
// li = list_base + (count - 1 - r), r = slot - slot_base -> the member's map id (merged_map) or the draw's own -> depths[slot].  Everything
// else -- no-hit records, the zero bytes of a shard's padding -- has weight 0 and stays.  (A frame whose pair buffer overflowed is re-run;
// until then its pairs may name anything: indices are bounded, not trusted.)
__global__ __launch_bounds__(256) void k_pick_resolve(uint4* __restrict__ out_pick, uint32_t n_px, const uint32_t* __restrict__ vals, uint32_t pair_cap,
                                                      const uint2* __restrict__ chunk_tab, uint32_t n_chunks, const DrawDev* __restrict__ draws,
                                                      const uint32_t* __restrict__ static_list, const uint32_t* __restrict__ merged_list,
                                                      const uint32_t* __restrict__ merged_map, const float* __restrict__ depths)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_px) return;
    const uint4 raw = out_pick[i];
    if (raw.w == 0u) return;
    uint4 o = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, __float_as_uint(1.0f), 0u);
    if (raw.x < pair_cap) {
        const uint32_t slot = vals[raw.x];
        if ((slot >> 8) < n_chunks) {
            const DrawDev& d = draws[chunk_tab[slot >> 8].x];
            const uint32_t r = slot - d.slot_base;
            if (r < d.count) {
                const uint32_t li = d.list_base + (d.count - 1u - r);
                const bool mrg = d.merged != 0u;
                o = make_uint4(mrg ? merged_map[li] : d.map_index, (mrg ? merged_list : static_list)[li], __float_as_uint(depths[slot]), raw.w);
            }
        }
    }
    out_pick[i] = o;
}

// all-gathered shards -> frame.  rows: shard = tile row % count (rows_padded rows each, full width);
// columns: shard = tile column / band_tiles (height rows each, band_px wide).  P: the pixel (float4, or uint32_t for the 8-bit formats)
template <typename P>
__global__ void k_unshard(const P* __restrict__ gathered, P* __restrict__ out, int width, int height,
                          int shard_count, int rows_padded, int band_px)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x;
    int y = blockIdx.y;
    if (x >= width || y >= height) return;
    size_t src;
    if (band_px > 0) {
        const int shard = x / band_px;
        src = ((size_t)shard * height + y) * band_px + (x - shard * band_px);
    } else {
        int ty = y >> 4;
        int shard = ty % shard_count, tyl = ty / shard_count;
        src = ((size_t)shard * rows_padded + (size_t)tyl * kTile + (y & 15)) * width + x;
    }
    out[(size_t)y * width + x] = gathered[src];
}

// The same for ONE PLANE of a video format (P: its sample, a byte or NV12's Cb Cr pair; TILE: the plane's rows per screen tile row, kTile or,
// for the half-size chroma planes, kTile / 2).  gathered / out: the plane inside shard 0's image / inside the frame; stride: samples from
// one shard's image to the next (the whole image of all planes, not this plane alone); width, height, rows_padded, band_px: the plane's.
template <typename P, int TILE>
__global__ void k_unshard_plane(const P* __restrict__ gathered, P* __restrict__ out, int width, int height,
                                int shard_count, int rows_padded, int band_px, size_t stride)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= width || y >= height) return;
    size_t src;
    if (band_px > 0) {
        const int shard = x / band_px;
        src = (size_t)shard * stride + (size_t)y * band_px + (x - shard * band_px);
    } else {
        const int ty = y / TILE;
        const int shard = ty % shard_count, tyl = ty / shard_count;
        src = (size_t)shard * stride + ((size_t)tyl * TILE + (y % TILE)) * width + x;
    }
    out[(size_t)y * width + x] = gathered[src];
}

// ---- launch wrappers (called from gswt_api.hip) -------------------------------------
// Every wrapper picks its kernel instantiation from runtime values through with_variant (gswt_variant.h).
void launch_chunk_tabs(hipStream_t s, const DrawDev* draws, const uint32_t* xcd_first, uint32_t n_draws, uint2* chunk_tab, uint2* chunk_tab_xcd,
                       const uint64_t per_xcd[8], uint64_t longest)
{
    XcdLens xl;
    for (int x = 0; x < 8; x++) xl.len[x] = (uint32_t)per_xcd[x];
    xl.longest = (uint32_t)longest;
    if (n_draws) hipLaunchKernelGGL(k_chunk_tabs, dim3(n_draws + 8u), dim3(256), 0, s, draws, xcd_first, n_draws, chunk_tab, chunk_tab_xcd, xl);
}

GraphRec*& graph_recorder()
{
    static thread_local GraphRec* rec = nullptr;
    return rec;
}

bool kernel_events_enabled()
{
    static const bool on = !(getenv("GSWT_KERNEL_EVENTS") && atoi(getenv("GSWT_KERNEL_EVENTS")) == 0);
    return on;
}

void launch_cull(hipStream_t s, const Frame& f, const FrameBufs& b, bool chunk_cull)
{
    uint32_t grid = (b.n_chunks + 255u) / 256u;            // one thread per chunk; the clears and the cell table stride over the grid
    if (grid < 32) grid = 32;
    GSWT_LAUNCH(k_cull, dim3(grid), dim3(256), s, f, b.draws, b.draw_culled, b.cell_culled, b.n_cells, b.ghist, b.n_zero_head,
                reinterpret_cast<uint32_t*>(b.ranges), b.n_zero_ranges, b.block_sums, b.n_chunks, b.radix_depth, b.n_zero_depth,
                b.chunk_tab, b.n_chunks, b.boxes, chunk_cull && b.boxes ? 1u : 0u, b.live_cnt, b.live_tab, b.live_cid);
}

void launch_project(hipStream_t s, const Frame& f, const FrameBufs& b, uint32_t n_launch, bool debug, ProjectModes m)
{
    if (b.n_chunks == 0) return;
    const SuperSums ss = super_sums_of(b.n_chunks);     // (zeroed by k_cull)
    const bool full = f.surface_type == 2u || f.draw_mode != 0u;
    with_variant([&](auto D, auto F, auto S, auto O, auto A, auto M, auto Y, auto Z, auto C) {
        if constexpr (S || !(O || A || M || Y || Z || C))
            GSWT_LAUNCH((k_project<D, F, S, O, A, M, Y, Z, C>), dim3(n_launch), dim3(256), s, f, b.draws, b.chunk_tab_xcd, b.static_list, b.merged_list,
                        b.merged_map, b.tex, b.hmap, b.draw_culled, b.cell_culled, b.live_cnt, b.live_tab, b.rects, b.recs, b.depths, b.block_sums,
                        b.super_sums, ss.n_super, b.dbg, b.col_f, b.styles, b.n_styles, b.shadow, b.clip);
    }, debug, full, m.strict, m.ortho, m.aa, m.atm, m.sty, m.shd, m.clip);
    GSWT_LAUNCH(k_totals, dim3(1), dim3(256), s, b.super_sums, ss.n_super, b.counters, b.super_sums + ss.prefix_word(0), b.pair_cap, b.live_cnt, n_launch / kLiveLists);
}

// keys: tile ids, vals: slots.  GSWT_ORDER_DEPTH (dkeys != nullptr): also each pair's depth bits -> dkeys and the frame's key range -> krange.
void launch_emit(hipStream_t s, const Frame& f, const FrameBufs& b, uint32_t* keys, uint32_t* dkeys, uint32_t* krange, uint32_t n_launch)
{
    const uint32_t n_chunks = b.n_chunks, pair_cap = b.pair_cap;
    if (n_chunks == 0) return;
    const uint32_t* const excl = b.super_sums + super_sums_of(n_chunks).prefix_word(0);
    const float* const no_f = nullptr; uint32_t* const no_u = nullptr;
    // over k_cull's table of live chunks (k_totals' copy of its counts); without one (n_launch 0: the debug-varyings frame) over every chunk of
    // the frame, four consecutive ones per workgroup
    const uint32_t* const cnt2 = n_launch ? b.live_cnt + live_copy_word(0) : nullptr;
    const uint32_t* const cid = n_launch ? b.live_cid : nullptr;
    const dim3 grid(n_launch ? ((n_launch / 8u + kEmitGroup - 1u) / kEmitGroup) * 8u : (n_chunks + kEmitGroup - 1u) / kEmitGroup);
    with_variant([&](auto L, auto D) {
        GSWT_LAUNCH((k_emit<D, L>), grid, dim3(256), s, f, b.rects, b.block_sums, excl, n_chunks, pair_cap, b.counters, keys, b.vals_a,
                    D ? b.depths : no_f, D ? dkeys : no_u, D ? krange : no_u, cnt2, cid);
    }, n_launch != 0u, dkeys != nullptr);
}

// ws: the RadixWs of (n_cap, key_bits), gswt_frame_layout.h.  Its zeroed part -- the group rows and digit totals of every pass, targets of
// atomic adds -- comes first; the per-workgroup rows behind it are written in full by k_radix_hist (every launched workgroup stores its
// 256 counts, zeros past the item count) -- a frame used to clear them too: 2 MB at c3, 13.6 MB at c5, by k_cull's 32 workgroups.
int launch_sort(hipStream_t s, uint32_t* keys_a, uint32_t* vals_a, uint32_t* keys_b, uint32_t* vals_b, uint32_t n_cap,
                const SortCount* count, int key_bits, uint32_t* ws, uint2* ranges, const uint32_t* krange, uint32_t* aux_a, uint32_t* aux_b,
                int threads_override, int aux_override)
{
    if (n_cap == 0) return 0;
    const RadixWs lay = radix_ws_of(n_cap, key_bits);
    const uint32_t nblk = lay.nblk, nsup = lay.nsup;
    // (the overrides: gswt_debug_sort_ex only -- a frame takes 512 threads at every capacity and payload form 1 up to 12 M pairs, 2 above)
    const int threads = threads_override ? threads_override : n_cap <= kSortWideMax ? 512 : 256;
    const int aux = !aux_a ? 0 : aux_override ? aux_override : n_cap > (12u << 20) ? 2 : 1;       // k_radix_scatter's payload forms
    int cur = 0;
    for (int shift = 0, pass = 0; shift < key_bits; shift += 8, pass++) {
        uint32_t nbits = (uint32_t)((key_bits - shift) < 8 ? (key_bits - shift) : 8);
        uint32_t mask = (1u << nbits) - 1u;
        uint32_t* const gsup = ws + lay.gsup(pass); uint32_t* const gtot = ws + lay.gtot(pass); uint32_t* const ghist = ws + lay.ghist(pass);
        uint32_t* ki = cur ? keys_b : keys_a; uint32_t* vi = cur ? vals_b : vals_a;
        uint32_t* ko = cur ? keys_a : keys_b; uint32_t* vo = cur ? vals_a : vals_b;
        const uint32_t* xi = cur ? aux_b : aux_a; uint32_t* xo = cur ? aux_a : aux_b;
        with_variant([&](auto T, auto AUX) {
            GSWT_LAUNCH(k_radix_hist<T>, dim3(nblk), dim3(T), s, ki, count, n_cap, (uint32_t)shift, mask, nbits, ghist, gsup, gtot, nblk, nsup, krange);
            if (nsup > kSupDirect) GSWT_LAUNCH(k_radix_supscan, dim3(64), dim3(256), s, gsup, gtot, nsup);
            GSWT_LAUNCH((k_radix_scatter<T, AUX>), dim3(nblk), dim3(T), s, ki, vi, ko, vo, count, n_cap, (uint32_t)shift, mask, nbits,
                        ghist, gsup, gtot, nblk, nsup, shift + 8 >= key_bits ? ranges : (uint2*)nullptr, krange, xi, xo);
        }, OneOf<512, 256>{threads}, OneOf<2, 1, 0>{aux});
        cur ^= 1;
    }
    return cur;
}

// Builds every merged group's (gs_index | lod, map_id) list on the device.  keys/vals a,b: n_total u32 each;
// ws: radix_ws_words(n_total, 16 + group_bits) zeroed words; n_total_dev: the device's SortCount record of n_total.
void launch_merge_build(hipStream_t s, const MergeSeg* segs, uint32_t n_segs, const uint2* blocks, uint32_t n_blocks, MergeGroup* groups, uint32_t n_groups,
                        const int32_t* raw, uint32_t n_total, const SortCount* n_total_dev, uint32_t* ka, uint32_t* va,
                        uint32_t* kb, uint32_t* vb, uint32_t* radix_ws, int group_bits, uint32_t* merged_list, uint32_t* merged_map)
{
    if (n_total == 0 || n_groups == 0 || n_blocks == 0) return;
    hipLaunchKernelGGL(k_mg_minmax, dim3(n_blocks), dim3(256), 0, s, segs, blocks, raw, groups);
    hipLaunchKernelGGL(k_mg_keys, dim3(n_blocks), dim3(256), 0, s, segs, blocks, raw, groups, ka, va);
    const int where = launch_sort(s, ka, va, kb, vb, n_total, n_total_dev, 16 + group_bits, radix_ws);
    hipLaunchKernelGGL(k_mg_final, dim3((n_total + 255) / 256), dim3(256), 0, s, segs, n_segs, groups, where ? kb : ka, where ? vb : va,
                       n_total, merged_list, merged_map);
}

int launch_scene_sort(hipStream_t s, const MergeSeg* segs, const uint2* blocks, uint32_t n_blocks, MergeGroup* groups, const int32_t* raw,
                      uint32_t n_total, const SortCount* n_total_dev, uint32_t* ka, uint32_t* va, uint32_t* kb, uint32_t* vb,
                      uint32_t* radix_ws, int group_bits)
{
    if (n_total == 0 || n_blocks == 0) return 0;
    hipLaunchKernelGGL(k_mg_minmax, dim3(n_blocks), dim3(256), 0, s, segs, blocks, raw, groups);
    hipLaunchKernelGGL(k_mg_keys, dim3(n_blocks), dim3(256), 0, s, segs, blocks, raw, groups, ka, va);
    return launch_sort(s, ka, va, kb, vb, n_total, n_total_dev, 16 + group_bits, radix_ws);
}

void launch_merge_copy(hipStream_t s, const MergeCopy* jobs, const uint2* blocks, uint32_t n_blocks, const uint2* remap, const MergeSources& src,
                       uint32_t* new_list, uint32_t* new_map)
{
    if (n_blocks) hipLaunchKernelGGL(k_mg_copy, dim3(n_blocks), dim3(256), 0, s, jobs, blocks, remap, src, new_list, new_map);
}

// dkeys = the pairs' depth bits in the order of vals (the tile sort's payload)
void launch_tile_depth_sort(hipStream_t s, const uint2* ranges, uint32_t* vals, uint32_t* dkeys, uint32_t* vals_scratch, uint32_t* dkeys_scratch, int n_tiles,
                            uint32_t* long_list, FrameCounters* counters)
{
    if (n_tiles <= 0) return;
    // four size classes in three launches: a wave per tile, a 256-thread workgroup per tile, a fixed grid over the list of still longer ones
    // which then also walks the list of those that do not fit LDS at all (long_list: [0] count, [1 .. n_tiles] tiles; the second list behind it)
    const uint32_t nt = (uint32_t)n_tiles;
    GSWT_LAUNCH((k_tile_depth_sort<64, 8, false>), dim3(nt), dim3(64), s, ranges, vals, dkeys, nt, long_list, counters, 0u, 0u, vals_scratch, dkeys_scratch);
    GSWT_LAUNCH((k_tile_depth_sort<256, 16, false>), dim3(nt), dim3(256), s, ranges, vals, dkeys, nt, long_list, counters, 512u, 1u, vals_scratch, dkeys_scratch);
    GSWT_LAUNCH((k_tile_depth_sort<1024, 16, true>), dim3(kTileSortLongGrid), dim3(1024), s, ranges, vals, dkeys, nt, long_list, counters, 4096u, 0u,
                vals_scratch, dkeys_scratch);
}
uint32_t tile_depth_sort_cap() { return kTileSortCap; }

// ranges -> per-tile segment counts -> item_base (exclusive scan, item_base[n_tiles] = #items) ->
// k_composite over an upper bound of items -> k_combine, storing the image in format OUTF.
// ZOUT: the frame's depth image is written as well, when b.out_depth is set (gswt_render_depth).
// PICK: its pick image, when b.out_pick is set (gswt_render_pick), resolved in place by k_pick_resolve from the same `vals`.
// E, D, C: the compositor's <early-out, depth test, float colours> (debug draw modes: float colours from the side buffer, no early-out).
void launch_composite(hipStream_t s, const Frame& f, const FrameBufs& b, const uint32_t* vals, int out_rows, const uint32_t* krange,
                      uint32_t depth_passes, bool report_max, hipEvent_t ev_begin, hipEvent_t ev_end, int out_format)
{
    const int n_tiles = (int)b.n_tiles;
    const uint32_t seg = b.seg;
    if (n_tiles == 0) {                 // a shard without screen tiles (more ranks than tile columns): the events still exist
        if (ev_begin) hipEventRecord(ev_begin, s);
        if (ev_end) hipEventRecord(ev_end, s);
        return;
    }
    const uint32_t max_items = (uint32_t)n_tiles + b.pair_cap / seg + 1u;
    GSWT_LAUNCH(k_items, dim3((n_tiles + 8191) / 8192), dim3(1024), s, b.ranges, n_tiles, seg, b.item_base, b.item_tab, max_items, krange, depth_passes, b.counters,
                report_max ? 1u : 0u);
    const bool colf = f.draw_mode != 0u;
    with_variant([&](auto outf, auto pick, auto zout) {
        constexpr int OUTF = outf;          // (constants of their own: the inner lambda cannot read a captured argument at compile time)
        constexpr bool PICK = pick, ZOUT = zout;
        with_variant([&](auto C, auto E, auto D) {
            // (The compositor carries ev_begin / ev_end itself: GSWT_LAUNCH_TIMED.)
            if constexpr (C && E) return;       // (float colours have no early-out form)
            else
                GSWT_LAUNCH_TIMED((k_composite<E, D, C, OUTF, ZOUT, PICK>), dim3(max_items), dim3(256), s, ev_begin, ev_end, f, b.ranges, b.item_base, b.item_tab, seg, vals,
                                  b.recs, b.depths, b.col_f, b.bg_rgba, b.bg_depth, b.out, b.partials, n_tiles, out_rows, b.out_depth, b.partials_z,
                                  b.out_pick, b.partials_pick);
        }, colf, !colf && f.t_eps > 0.0f, f.has_depth != 0);
        GSWT_LAUNCH((k_combine<OUTF, ZOUT, PICK>), dim3(n_tiles), dim3(256), s, f, b.item_base, b.partials, b.bg_rgba, b.out, n_tiles, out_rows,
                    (const FrameCounters*)b.counters, b.host_counters, (const float*)b.partials_z, b.bg_depth, b.out_depth,
                    (const uint2*)b.partials_pick, b.out_pick);
        if (PICK) {
            const uint32_t n_px = (uint32_t)out_rows * (uint32_t)f.out_w;
            GSWT_LAUNCH_TIMED(k_pick_resolve, dim3((n_px + 255u) / 256u), dim3(256), s, b.ev_pick_begin, b.ev_pick_end, b.out_pick, n_px, vals, b.pair_cap, b.chunk_tab, b.n_chunks, b.draws,
                        b.static_list, b.merged_list, b.merged_map, (const float*)b.depths);
        }
    }, OneOf<kOutNV12, kOutI420, kOutRGBA8, kOutBGRA8, kOutF32>{out_format}, b.out_pick != nullptr, b.out_depth != nullptr);
}

// k_totals alone on caller-provided sums (unit test of the 64-bit pair count)
void launch_totals(hipStream_t s, uint32_t* super_sums, SuperSums ss, FrameCounters* counters, uint32_t pair_cap)
{
    hipLaunchKernelGGL(k_totals, dim3(1), dim3(256), 0, s, super_sums, ss.n_super, counters, super_sums + ss.prefix_word(0), pair_cap, (uint32_t*)nullptr, 0xFFFFFFFFu);
}

void launch_unshard(hipStream_t s, const void* gathered, void* out, int width, int height, int shard_count, int rows_padded, int band_px,
                    int out_format)
{
    const dim3 grid((width + 255) / 256, height);
    if (out_is_video(out_format)) {
        // plane by plane: Y as bytes; the chroma planes are half-size images whose tile is 8 rows (k_unshard's TILE), NV12's as 2-byte pairs
        const uint8_t* const src = static_cast<const uint8_t*>(gathered);
        uint8_t* const dst = static_cast<uint8_t*>(out);
        const int n = shard_count < 1 ? 1 : shard_count, hw = width / 2, hh = height / 2;
        // a shard's own image: rows_padded x width (rows), height x band_px (columns)
        const size_t shard_px = band_px > 0 ? (size_t)height * band_px : (size_t)rows_padded * width, frame_px = (size_t)width * height;
        const dim3 hgrid((hw + 255) / 256, hh);
        hipLaunchKernelGGL((k_unshard_plane<uint8_t, kTile>), grid, dim3(256), 0, s, src, dst, width, height, n, rows_padded, band_px, shard_px * 3u / 2u);
        if (out_format == kOutNV12)
            hipLaunchKernelGGL((k_unshard_plane<uint16_t, kTile / 2>), hgrid, dim3(256), 0, s, reinterpret_cast<const uint16_t*>(src + shard_px),
                               reinterpret_cast<uint16_t*>(dst + frame_px), hw, hh, n, rows_padded / 2, band_px / 2, shard_px * 3u / 4u);
        else
            for (int p = 0; p < 2; p++)
                hipLaunchKernelGGL((k_unshard_plane<uint8_t, kTile / 2>), hgrid, dim3(256), 0, s, src + shard_px + p * (shard_px / 4u),
                                   dst + frame_px + p * (frame_px / 4u), hw, hh, n, rows_padded / 2, band_px / 2, shard_px * 3u / 2u);
    } else if (out_format == kOutF32)
        hipLaunchKernelGGL(k_unshard<float4>, grid, dim3(256), 0, s, static_cast<const float4*>(gathered), static_cast<float4*>(out), width, height,
                           shard_count, rows_padded, band_px);
    else
        hipLaunchKernelGGL(k_unshard<uint32_t>, grid, dim3(256), 0, s, static_cast<const uint32_t*>(gathered), static_cast<uint32_t*>(out), width,
                           height, shard_count, rows_padded, band_px);
}

}  // namespace gswt
#ifdef GSWT_TRACE
extern "C" __attribute__((visibility("default"))) int gswt_debug_trace(unsigned long long* out, unsigned n_items)
{
    hipDeviceSynchronize();
    if (n_items > gswt::kTraceItems) n_items = gswt::kTraceItems;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(gswt::g_trace), (size_t)n_items * 64);
}
#endif
#ifdef GSWT_STATS
extern "C" __attribute__((visibility("default"))) int gswt_debug_stats(unsigned long long* out)
{
    hipDeviceSynchronize();
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(gswt::g_stats), 64);
}
#endif
