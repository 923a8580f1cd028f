// gswt_scene.hip -- scene preparation on the device (gswt_upload_scene_rows): the per-splat and per-list half of
// WangTile::preprocess (wangtile.rs:71-255) and of the static-arena build of gswt_upload_scene, from the normalised 32-byte rows.
//
//   k_scene_tex     : Scene::generate_texture per splat (the host's operator sequence, host/gswt_math.h), and the tile-local bounds of the
//                     splat centres + the largest covariance bound that gswt_upload_scene computes on the host (band cull)
//   k_scene_raw     : the raw depth of every splat for every presort view, in gswt_upload_raw_depth's arena layout
//   (base lists)    : k_mg_minmax / k_mg_keys + the stable radix sort of gswt_kernels.hip, one group per (lod, tile) of a view
//   k_scene_scatter : sorted position -> reversed slot of the list's pair list in the static arena, entry = gs_index | lod << 28
//   k_scene_self    : self list = the pair list's own-LOD entries, order kept (stable compaction, one workgroup per list)
//   k_scene_boxes   : tile-local bounding box of every 256-entry chunk of every static list (one wave per chunk)
//
// Built with -ffp-contract=off like the host library: the texture words, raw depths and bounds are the host's bit for bit -- the
// per-record arithmetic (texture row, raw depth, half decode, covariance bound, finite test) is gswt_host:: of host/gswt_math.h, the
// chunk ranges chunk_entry_range of gswt_device.h: the sources the host path compiles.
// Wavefront = 64 lanes.
#include "gswt_device_fn.h"

namespace gswt {

namespace {

// order-preserving map f32 -> i32 (and back: the map is its own inverse); -0 sorts below +0, which the bounds compare as equal
__device__ __forceinline__ int32_t f2ord(float f)
{
    const int32_t i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7FFFFFFF;
}

__device__ __forceinline__ uint32_t scene_find_lt(const uint32_t* __restrict__ moff, uint32_t n_lt, uint32_t g)
{
    uint32_t lo = 0, hi = n_lt;                       // largest i with moff[i] <= g
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (moff[mid] <= g) lo = mid; else hi = mid; }
    return lo;
}

}  // namespace

// Grid-stride over the splats; bounds: [0..2] lo, [3..5] hi (f2ord, atomic min / max), [6] non-finite seen, [7] largest bound (f32 bits)
__global__ __launch_bounds__(256) void k_scene_tex(const uint4* __restrict__ rows, uint32_t n, uint4* __restrict__ tex, int32_t* __restrict__ bounds)
{
    __shared__ int32_t s_red[4][8];
    int32_t lo[3] = {2147483647, 2147483647, 2147483647}, hi[3] = {-2147483647 - 1, -2147483647 - 1, -2147483647 - 1};
    int32_t odd = 0;
    uint32_t tr_max = 0;                              // bits of a non-negative float: ordered as u32
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        uint4 rw[2] = {rows[2 * (size_t)i], rows[2 * (size_t)i + 1]};
        uint32_t t[8];
        gswt_host::generate_texture_row(reinterpret_cast<const uint8_t*>(rw), t);
        tex[2 * (size_t)i] = make_uint4(t[0], t[1], t[2], t[3]);
        tex[2 * (size_t)i + 1] = make_uint4(t[4], t[5], t[6], t[7]);
        // gswt_upload_scene's loop over the texture records
        for (int k = 0; k < 3; k++) {
            const float p = __uint_as_float(t[k]);
            if (!gswt_host::finite_coord(p)) { odd = 1; continue; }
            lo[k] = min(lo[k], f2ord(p)); hi[k] = max(hi[k], f2ord(p));
        }
        const float tr = gswt_host::cov_extent_bound(t);
        if (tr > 0.0f) tr_max = max(tr_max, __float_as_uint(tr));      // (the host's max from 0 keeps +0 for any tr <= 0)
    }
    int32_t v[8] = {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], odd, (int32_t)tr_max};
    for (int off = 32; off > 0; off >>= 1) {
        for (int k = 0; k < 3; k++) v[k] = min(v[k], __shfl_down(v[k], off, 64));
        for (int k = 3; k < 6; k++) v[k] = max(v[k], __shfl_down(v[k], off, 64));
        v[6] |= __shfl_down(v[6], off, 64);
        v[7] = (int32_t)max((uint32_t)v[7], (uint32_t)__shfl_down(v[7], off, 64));
    }
    if ((threadIdx.x & 63u) == 0)
        for (int k = 0; k < 8; k++) s_red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 8u) {
        const int k = (int)threadIdx.x;
        int32_t r = s_red[0][k];
        for (int w = 1; w < 4; w++) {
            const int32_t q = s_red[w][k];
            r = k < 3 ? min(r, q) : k < 6 ? max(r, q) : k == 6 ? (r | q) : (int32_t)max((uint32_t)r, (uint32_t)q);
        }
        if (k < 3) atomicMin(&bounds[k], r);
        else if (k < 6) atomicMax(&bounds[k], r);
        else if (k == 6) { if (r) atomicOr(&bounds[6], r); }
        else if (r) atomicMax(reinterpret_cast<uint32_t*>(&bounds[7]), (uint32_t)r);
    }
}

// raw[n_view * moff[lt] + v * cnt[lt] + j] = raw depth of splat j of tile scene lt for view v (gswt_upload_raw_depth's layout)
__global__ __launch_bounds__(256) void k_scene_raw(const uint4* __restrict__ rows, uint32_t n, const uint32_t* __restrict__ moff,
                                                   const uint32_t* __restrict__ cnt, uint32_t n_lt, const SceneViews vps, int32_t* __restrict__ raw)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4 r = rows[2 * (size_t)i];
    const float x = __uint_as_float(r.x), y = __uint_as_float(r.y), z = __uint_as_float(r.z);
    const uint32_t lt = scene_find_lt(moff, n_lt, i);
    const uint32_t c = cnt[lt];
    int32_t* dst = raw + (size_t)vps.n_view * moff[lt] + (i - moff[lt]);
    for (uint32_t v = 0; v < vps.n_view; v++) dst[(size_t)v * c] = gswt_host::raw_depth_of(vps.vp[v], x, y, z);
}

// k_mg_final without map ids: the group is the list, its pair list starts at out_base in the static arena
__global__ __launch_bounds__(256) void k_scene_scatter(const MergeSeg* __restrict__ segs, uint32_t n_segs, const MergeGroup* __restrict__ groups,
                                                       const uint32_t* __restrict__ sorted_keys, const uint32_t* __restrict__ sorted_vals,
                                                       uint32_t n_total, uint32_t* __restrict__ arena, uint32_t arena_n)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n_total) return;
    const MergeGroup gr = groups[sorted_keys[p] >> 16];
    const uint32_t out = gr.out_base + (gr.len - 1u - (p - gr.base));      // depth_index.reverse()
    const uint32_t e = sorted_vals[p];
    uint32_t lo = 0, hi = n_segs;                     // largest s with segs[s].start <= e
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (segs[mid].start <= e) lo = mid; else hi = mid; }
    const MergeSeg sg = segs[lo];
    if (out < arena_n) arena[out] = ((e - sg.start) + sg.gs_offset) | (sg.lod << kLodShift);
}

// One workgroup per list: its self list = the entries of its pair list whose lod is the list's own, in order.
// 1024 pair entries per step (four per lane); each step's keeps are ranked by (sub-step, wave, lane).
__global__ __launch_bounds__(256) void k_scene_self(const SceneList* __restrict__ lists, uint32_t lists_per_lod, uint32_t* __restrict__ arena)
{
    __shared__ uint32_t s_cnt[16];
    const SceneList L = lists[blockIdx.x];
    const uint32_t lod = blockIdx.x / lists_per_lod;
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t written = 0;
    for (uint32_t base = 0; base < L.pair_count; base += 1024u) {
        uint32_t e[4], rank[4];
        bool keep[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t j = base + (uint32_t)k * 256u + threadIdx.x;
            e[k] = j < L.pair_count ? arena[L.pair_base + j] : 0u;
            keep[k] = j < L.pair_count && (e[k] >> kLodShift) == lod;
            const unsigned long long m = ballot64(keep[k]);
            rank[k] = lanes_below(m);
            if ((threadIdx.x & 63u) == 0) s_cnt[k * 4 + wave] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        uint32_t total = 0;
        uint32_t before[4] = {0, 0, 0, 0};
        for (int q = 0; q < 16; q++) {
            const uint32_t cq = s_cnt[q];
#pragma unroll
            for (int k = 0; k < 4; k++) if (q == k * 4 + (int)wave) before[k] = total;
            total += cq;
        }
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (keep[k]) {
                const uint32_t dst = written + before[k] + rank[k];
                if (dst < L.self_count) arena[L.self_base + dst] = e[k];
            }
        written += total;
        __syncthreads();
    }
}

// One wave per chunk box.  Box b belongs to the list whose pair_box is the largest <= b; chunk k of a list of `count` entries covers
// chunk_entry_range(count, k), its k-th 256 entries from the end (k_project's order).  A chunk that holds a non-finite coordinate gets the infinite box.
__global__ __launch_bounds__(256) void k_scene_boxes(const SceneList* __restrict__ lists, uint32_t n_lists, uint32_t n_boxes,
                                                     const uint32_t* __restrict__ arena, const uint4* __restrict__ tex, uint32_t n_splats,
                                                     float* __restrict__ boxes)
{
    const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (b >= n_boxes) return;
    uint32_t lo_l = 0, hi_l = n_lists;
    while (hi_l - lo_l > 1u) { const uint32_t mid = (lo_l + hi_l) >> 1; if (lists[mid].pair_box <= b) lo_l = mid; else hi_l = mid; }
    const SceneList L = lists[lo_l];
    const uint32_t n_pair_boxes = (L.pair_count + (uint32_t)kChunk - 1u) / (uint32_t)kChunk;
    const bool pair = b - L.pair_box < n_pair_boxes;
    const uint32_t base = pair ? L.pair_base : L.self_base, count = pair ? L.pair_count : L.self_count;
    const uint32_t k = pair ? b - L.pair_box : b - L.self_box;
    uint32_t lo_i, hi_i;
    chunk_entry_range(count, k, lo_i, hi_i);
    float lo[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, hi[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
    bool odd = false;
    for (uint32_t j = lo_i + lane; j < hi_i; j += 64u) {
        const uint4 r = tex[2 * (size_t)min(arena[base + j] & kIdxMask, n_splats - 1u)];
        const float p[3] = {__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z)};
        for (int a = 0; a < 3; a++) {
            if (!gswt_host::finite_coord(p[a])) odd = true;
            lo[a] = fminf(lo[a], p[a]); hi[a] = fmaxf(hi[a], p[a]);
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], __shfl_down(lo[a], off, 64)); hi[a] = fmaxf(hi[a], __shfl_down(hi[a], off, 64)); }
    odd = ballot64(odd) != 0ull;
    if (lane == 0) {
        float* o = boxes + 6 * (size_t)b;
        for (int a = 0; a < 3; a++) { o[a] = odd ? -__builtin_inff() : lo[a]; o[3 + a] = odd ? __builtin_inff() : hi[a]; }
    }
}

// ---- launch wrappers (gswt_device.h) -------------------------------------------------------------------------------------------------

void launch_scene_tex(hipStream_t s, const uint4* rows, uint32_t n, uint4* tex, int32_t* bounds)
{
    if (n == 0) return;
    const uint32_t grid = std::min<uint32_t>((n + 255u) / 256u, 2048u);
    hipLaunchKernelGGL(k_scene_tex, dim3(grid), dim3(256), 0, s, rows, n, tex, bounds);
}

void launch_scene_raw(hipStream_t s, const uint4* rows, uint32_t n, const uint32_t* moff, const uint32_t* cnt, uint32_t n_lt, const SceneViews& vps,
                      int32_t* raw)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_scene_raw, dim3((n + 255u) / 256u), dim3(256), 0, s, rows, n, moff, cnt, n_lt, vps, raw);
}

void launch_scene_scatter(hipStream_t s, const MergeSeg* segs, uint32_t n_segs, const MergeGroup* groups, const uint32_t* sorted_keys,
                          const uint32_t* sorted_vals, uint32_t n_total, uint32_t* arena, uint32_t arena_n)
{
    if (n_total == 0) return;
    hipLaunchKernelGGL(k_scene_scatter, dim3((n_total + 255u) / 256u), dim3(256), 0, s, segs, n_segs, groups, sorted_keys, sorted_vals, n_total, arena,
                       arena_n);
}

void launch_scene_self(hipStream_t s, const SceneList* lists, uint32_t n_lists, uint32_t lists_per_lod, uint32_t* arena)
{
    if (n_lists == 0) return;
    hipLaunchKernelGGL(k_scene_self, dim3(n_lists), dim3(256), 0, s, lists, lists_per_lod, arena);
}

void launch_scene_boxes(hipStream_t s, const SceneList* lists, uint32_t n_lists, uint32_t n_boxes, const uint32_t* arena, const uint4* tex,
                        uint32_t n_splats, float* boxes)
{
    if (n_boxes == 0 || n_splats == 0) return;
    hipLaunchKernelGGL(k_scene_boxes, dim3((n_boxes + 3u) / 4u), dim3(256), 0, s, lists, n_lists, n_boxes, arena, tex, n_splats, boxes);
}

}  // namespace gswt
