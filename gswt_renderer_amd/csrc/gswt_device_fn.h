// gswt_device_fn.h -- the device functions more than one kernel file uses, defined once: lane masks, the bit casts, the hot path's half
// decode and the repeat sampler of the height map.  Included by the four kernel files only (gswt_kernels.hip, gswt_passes.hip,
// gswt_scene.hip, gswt_worker.hip); the host-only C-ABI files never see it.
//
// It is also THE place that makes host/gswt_math.h and host/gswt_surface.h __host__ __device__ (GSWT_HD) for the kernel files: what the
// host library and the kernels must compute alike (the sphere mapping, the scene's texture words, the worker's surface_mapping) is
// written there once and compiled into both.
// Wavefront = 64 lanes.
#pragma once
#include "gswt_device.h"

#define GSWT_HD __host__ __device__
#include "host/gswt_math.h"
#include "host/gswt_surface.h"

namespace gswt {

// Lane mask of a predicate.  (Not __ballot(int): its argument is an int, so the compiler first materialises the predicate as 0 / 1 in a
// vector register and compares that again -- two vector instructions per ballot that v_cmp had already answered.)
__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// bits of a lane mask below the calling lane (v_mbcnt_lo / _hi): a lane's rank among the lanes the mask names
__device__ __forceinline__ uint32_t lanes_below(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ float u2f(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ float clampf(float e, float lo, float hi) { return fminf(fmaxf(e, lo), hi); }
// gswt_set_atmosphere's fog amount F(dist) (include/gswt_hip.h), shared by k_project<.., ATM> and k_proxy<FOG>: every written operator one
// binary32 operation, e = __expf(-x) (the hardware exp2 of x * log2(e): within 2 ulp of exp(-x) where it matters, x e^-x <= 0.37).
// A NaN dist gives F = 0 (fmaxf drops it); an infinite x gives F = fog_max.
__device__ __forceinline__ float fog_amount(const Atmo& a, float dist)
{
    const float x = a.fog_density * fmaxf(dist - a.fog_start, 0.0f);
    const float e = __expf(-x);
    return a.fog_max * (1.0f - e);
}

// gswt_set_shadow_map's lookup (include/gswt_hip.h), shared by k_project<.., SHD> and k_proxy<.., SHD>, in two halves so that a caller can
// put work between the texel loads and their use.  Every written operator is one binary32 operation.
// shadow_fetch: the world point into the light's image and the 2 x 2 texels around it.  The four loads are UNCONDITIONAL, from clamped
// indices, and nothing here reads what they return: which of them count is the tap's `ok` mask (bit k: texel k lies inside the image and
// the point inside the image and the depth range), applied by shadow_amount.  Loads under a lane condition, or a select on their result
// here, would make the wait for whatever the caller still has in flight an uncounted vmcnt(0) directly behind them.
// Bounds: for a point outside (NaN included) u and v are replaced by 0; otherwise u is in (-1, w) and v in (-1, h), so i0 is in
// [-1, w - 1] and i1 in [0, w] (rows likewise).  Every index is clamped to [0, w - 1] x [0, h - 1] (w, h >= 1), and j * w + i <
// 4096 * 4096 fits an int.
struct ShadowTap { float z00, z10, z01, z11, wx, wy, r; uint32_t ok; };
__device__ __forceinline__ ShadowTap shadow_fetch(const Shadow& s, float c0, float c1, float c2)
{
    const float lx = ((s.row[0][0] * c0 + s.row[0][1] * c1) + s.row[0][2] * c2) + s.row[0][3];
    const float ly = ((s.row[1][0] * c0 + s.row[1][1] * c1) + s.row[1][2] * c2) + s.row[1][3];
    const float ld = ((s.row[2][0] * c0 + s.row[2][1] * c1) + s.row[2][2] * c2) + s.row[2][3];
    const float W = (float)s.w, H = (float)s.h;
    const float u = (lx * 0.5f + 0.5f) * W - 0.5f;
    const float v = (0.5f - ly * 0.5f) * H - 0.5f;
    const bool inside = (ld >= 0.0f && ld <= 1.0f) && (u > -1.0f && u < W) && (v > -1.0f && v < H);
    const float us = inside ? u : 0.0f, vs = inside ? v : 0.0f;
    const float x0 = floorf(us), y0 = floorf(vs);
    ShadowTap t;
    t.wx = us - x0; t.wy = vs - y0; t.r = ld - s.bias;
    const int i0 = (int)x0, j0 = (int)y0, i1 = i0 + 1, j1 = j0 + 1;
    const bool xa = i0 >= 0, xb = i1 < s.w, ya = j0 >= 0, yb = j1 < s.h;          // (i0 <= w - 1 and i1 >= 0 always, rows likewise)
    t.ok = inside ? (uint32_t)(xa && ya) | (uint32_t)(xb && ya) << 1 | (uint32_t)(xa && yb) << 2 | (uint32_t)(xb && yb) << 3 : 0u;
    const int ia = max(i0, 0), ib = min(i1, s.w - 1), ja = max(j0, 0) * s.w, jb = min(j1, s.h - 1) * s.w;
    t.z00 = s.z[ja + ia]; t.z10 = s.z[ja + ib]; t.z01 = s.z[jb + ia]; t.z11 = s.z[jb + ib];
    return t;
}
// shadow_amount: sh = strength * (1 - lit), lit the bilinear mix of the four depth compares; a texel that does not count (shadow_fetch's
// mask) and a NaN texel are lit, and a point outside has weights 0 and every texel lit: lit = 1 exactly
__device__ __forceinline__ float shadow_amount(const Shadow& s, const ShadowTap& t)
{
    const float t00 = (t.ok & 1u) && t.r > t.z00 ? 0.0f : 1.0f, t10 = (t.ok & 2u) && t.r > t.z10 ? 0.0f : 1.0f;
    const float t01 = (t.ok & 4u) && t.r > t.z01 ? 0.0f : 1.0f, t11 = (t.ok & 8u) && t.r > t.z11 ? 0.0f : 1.0f;
    const float lit = (t00 * (1.0f - t.wx) + t10 * t.wx) * (1.0f - t.wy) + (t01 * (1.0f - t.wx) + t11 * t.wx) * t.wy;
    return s.strength * (1.0f - lit);
}

// gswt_set_clip_volumes' test (include/gswt_hip.h), shared by k_project<.., CLIP> and the proxy kernels' CLIP forms.  Every written operator
// is one binary32 operation, the rows summed as shadow_fetch sums its own; every comparison is an ordinary IEEE compare, so a NaN coordinate
// is not inside.  The shape is uniform: a half-space never reads rows 0 and 1.
__device__ __forceinline__ bool clip_inside(const ClipVolume& q, float c0, float c1, float c2)
{
    const float u2 = ((q.row[2][0] * c0 + q.row[2][1] * c1) + q.row[2][2] * c2) + q.row[2][3];
    if (q.shape == kClipHalfspace) return u2 <= 0.0f;
    const float u0 = ((q.row[0][0] * c0 + q.row[0][1] * c1) + q.row[0][2] * c2) + q.row[0][3];
    const float u1 = ((q.row[1][0] * c0 + q.row[1][1] * c1) + q.row[1][2] * c2) + q.row[1][3];
    if (q.shape == kClipBox) return fabsf(u0) <= 1.0f && fabsf(u1) <= 1.0f && fabsf(u2) <= 1.0f;
    return (u0 * u0 + u1 * u1) + u2 * u2 <= 1.0f;
}
// The visibility rule: hidden unless (no keep volume, or inside one of them) and inside no cut volume.  The trip count and everything the
// loop reads of the set are uniform -- the set is a kernel argument, indexed by the loop counter alone -- so the rows arrive by scalar loads
// and feed the vector multiplies as scalar operands; no lane leaves the loop early, which keeps the counter uniform.
__device__ __forceinline__ bool clip_hidden(const ClipSet& s, float c0, float c1, float c2)
{
    bool in_keep = s.n_keep == 0u, in_cut = false;
    for (uint32_t k = 0; k < s.n; k++) {
        const bool in = clip_inside(s.v[k], c0, c1, c2);
        if (s.v[k].flags & kClipKeep) in_keep = in_keep || in;
        else in_cut = in_cut || in;
    }
    return !in_keep || in_cut;
}

// halfToFloat, gswt.wgsl:478-494: normals as IEEE; subnormals scale 2^-15 (f * 2^-25);
// Inf/NaN -> 0.  The definition is gswt_host::half_to_float (host/gswt_math.h, the shader's arithmetic): this is the hot path's form of
// it and must equal it on all 65536 bit patterns, signs of zero included.
// (v_cvt_f32_f16 is exact for every finite half, subnormals included: the shader's subnormal scale is half of IEEE's, and its
// Inf / NaN are 0 -- two selects on the exponent field instead of a branchy bit construction.)
__device__ __forceinline__ float half_decode(uint32_t h)
{
    // on the CONVERTED value: a half's Inf / NaN converts to Inf / NaN (-> 0), its subnormals and zeros to |x| < 2^-14, the smallest normal
    // half (-> x / 2: exact), everything else is already the shader's value
    const float x = __half2float(__ushort_as_half((unsigned short)h));
    const float y = fabsf(x) < 6.103515625e-05f ? x * 0.5f : x;
    return __builtin_amdgcn_class(x, 0x3 | 0x4 | 0x200) ? 0.0f : y;      // signalling / quiet NaN, -Inf, +Inf
}

// x mod w for the repeat sampler, identical to ((x % w) + w) % w in integer arithmetic but without the 64-bit
// division sequences (5 samples x 4 wraps per splat made the HeightMap path ~3000 instructions): the quotient is
// estimated in float (exact operands below 2^23, so it is off by at most one) and fixed up with two compares.
__device__ __noinline__ int wrap_repeat_slow(float fx, int w)
{
    const long xl = (long)fx;
    return (int)(((xl % w) + w) % w);
}

__device__ __forceinline__ int wrap_repeat(float fx, int w)
{
    if (fabsf(fx) < 8388608.0f && w < 8388608) {
        const int x = (int)fx;
        // a power-of-two map (the reference resizes its random maps to 1024 x 1024, wangtile.rs:405-412): two's-complement AND is the
        // mathematical modulus; the branch is uniform
        if ((w & (w - 1)) == 0) return x & (w - 1);
        int r = x - w * (int)floorf((float)x / (float)w);
        if (r < 0) r += w;
        if (r >= w) r -= w;
        return r;
    }
    return wrap_repeat_slow(fx, w);                 // far outside any real map: the exact 64-bit path, out of line
}

// WebGPU bilinear sample, R32Float, repeat addressing, level 0 (renderer.rs:376-388): the height map of k_project and of k_proxy.
// The two texels of a row are neighbours unless the cell straddles the map's seam: one 8-byte load per row (the buffer carries one
// float of padding behind its last row: gswt_configure), the seam case re-reads column 0.  Same texels, same arithmetic as four scalar
// loads: a splat on the HeightMap surface issues 10 height loads instead of 20.
__device__ __forceinline__ float sample_height(const float* __restrict__ hm, int w, int h, float u, float v)
{
    float x = u * (float)w - 0.5f;
    float y = v * (float)h - 0.5f;
    float fx0 = floorf(x), fy0 = floorf(y);
    float tx = x - fx0, ty = y - fy0;
    const int xa = wrap_repeat(fx0, w), ya = wrap_repeat(fy0, h);
    const int yb = ya + 1 == h ? 0 : ya + 1;
    const float* r0 = hm + (size_t)ya * w + xa;
    const float* r1 = hm + (size_t)yb * w + xa;
    // (a two-float vector type with 4-byte alignment: global memory takes a dword-aligned 8-byte load as ONE global_load_dwordx2;
    // a memcpy of 8 bytes at alignment 4 is lowered to two dword loads)
    typedef float hm_pair __attribute__((ext_vector_type(2), aligned(4)));
    hm_pair p0 = *reinterpret_cast<const hm_pair*>(r0), p1 = *reinterpret_cast<const hm_pair*>(r1);
    if (xa + 1 == w) { p0.y = hm[(size_t)ya * w]; p1.y = hm[(size_t)yb * w]; }
    float i00 = p0.x, i10 = p0.y;
    float i01 = p1.x, i11 = p1.y;
    float i0 = i00 * (1.0f - tx) + i10 * tx;
    float i1 = i01 * (1.0f - tx) + i11 * tx;
    return i0 * (1.0f - ty) + i1 * ty;
}

}  // namespace gswt
