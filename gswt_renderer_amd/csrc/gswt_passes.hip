// gswt_passes.hip -- the two background passes State::render runs before the splats (state.rs:384-392), as
// per-pixel compute kernels: their outputs are the bg_rgba / bg_depth inputs of gswt_render.
//
//   k_skybox : skybox.wgsl vs_main + fs_main (cube map lookup along the pixel's view ray), skybox.rs:457-488
//   k_skybox_bake : skybox.wgsl vs_bake + fs_bake (skybox.rs:490-668), configure time: an equirectangular HDR panorama baked
//              into the cube map k_skybox samples
//   k_lanczos_taps / k_lanczos_v / k_lanczos_v_sum / k_lanczos_h / k_proxy_mip_copy : configure time, the proxy texture's
//              Lanczos3 mip chain from its 8- / 16-bit RGBA image (upload_proxy_texture, proxy.rs:513-554)
//   k_proxy  : proxy.wgsl vs_main + fs_main + depth state (proxy.rs:96-134,366-447): the height-mapped ground grid.  Instead of
//              pushing up to 2 x 2048^2 triangles through a rasteriser, every pixel casts its view ray at the height field
//              (2-D DDA over the grid cells, two triangles per cell); the nearest fragment with depth in [0, 1] is exactly
//              what depth-test-Less rasterisation keeps.  Implicit-LOD trilinear texturing from the uv differences to the
//              right / lower pixel on the fragment's plane.  The height map is read through sample_height, the splat path's
//              sampler (gswt_device_fn.h: one definition, the padded buffer of gswt_configure); the repeat wraps of the proxy
//              texture and of the panorama are its wrap_repeat.
//   k_proxy_sphere : gswt_proxy_render_sphere (no counterpart in the reference, whose proxy draws the plane under every surface): the
//              ground of the Sphere surface, the pixel's ray against the sphere about the world origin, textured through the inverse of
//              the sphere unfolding (host/gswt_surface.h: sphere_plane_pos)
// k_proxy and k_proxy_sphere differ in how a pixel finds its hit, its texture coordinate and its LOD.  The rest is one definition each:
// proxy_ray (pixel -> ray, perspective or orthographic, also of the neighbour pixels), proxy_write (depth test and store, black_background,
// the shadow map's loads), proxy_colour (trilinear texture, brightness, shade, fog), and with_proxy_variant behind both launch wrappers.
// bilerp is the one bilinear blend of the cube map, the proxy texture and the panorama.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (same flags as gswt_kernels.hip).
#include "gswt_device_fn.h"
#include "gswt_variant.h"

#include <algorithm>

namespace gswt {

// The bilinear blend of four taps, every channel (a caller that wants rgb drops w): the filter of sample_cube, proxy_tex_bilinear and
// k_skybox_bake, each with its own addressing (clamp to edge, repeat).
__device__ __forceinline__ float4 bilerp(const float4 c00, const float4 c10, const float4 c01, const float4 c11, float wx, float wy)
{
    const auto mix = [wx, wy](float a, float b, float c, float d) { return (a * (1.0f - wx) + b * wx) * (1.0f - wy) + (c * (1.0f - wx) + d * wx) * wy; };
    return make_float4(mix(c00.x, c10.x, c01.x, c11.x), mix(c00.y, c10.y, c01.y, c11.y), mix(c00.z, c10.z, c01.z, c11.z), mix(c00.w, c10.w, c01.w, c11.w));
}

// Direction of the perspective view ray of pixel (x, y): d = R^T v, R = upper 3x3 of the view V (column-major), v = (ndc / (p00, p11), -1)
__device__ __forceinline__ void pixel_ray(const float* V, float p00, float p11, int x, int y, int W, int H, float d[3])
{
    const float nx = ((float)x + 0.5f) / (float)W * 2.0f - 1.0f;
    const float ny = 1.0f - ((float)y + 0.5f) / (float)H * 2.0f;
    const float vx = nx / p00, vy = ny / p11, vz = -1.0f;
    d[0] = (V[0] * vx + V[1] * vy) + V[2] * vz;
    d[1] = (V[4] * vx + V[5] * vy) + V[6] * vz;
    d[2] = (V[8] * vx + V[9] * vy) + V[10] * vz;
}

// Cube-map face selection (WebGPU / Vulkan major-axis rule) + bilinear filter inside the face, clamp to edge
// (skybox.rs:420-426: ClampToEdge, Linear, level 0).  faces: [6][n][n] float4, +X -X +Y -Y +Z -Z.
__device__ __forceinline__ float4 sample_cube(const float4* __restrict__ faces, int n, float tx, float ty, float tz)
{
    const float ax = fabsf(tx), ay = fabsf(ty), az = fabsf(tz);
    int face;
    float sc, tc, ma;
    if (az >= ax && az >= ay) { face = tz < 0.0f ? 5 : 4; sc = tz < 0.0f ? -tx : tx; tc = -ty; ma = az; }
    else if (ay >= ax) { face = ty < 0.0f ? 3 : 2; sc = tx; tc = ty < 0.0f ? -tz : tz; ma = ay; }
    else { face = tx < 0.0f ? 1 : 0; sc = tx < 0.0f ? tz : -tz; tc = -ty; ma = ax; }
    const float s = 0.5f * (sc / ma + 1.0f), t = 0.5f * (tc / ma + 1.0f);
    const float x = s * (float)n - 0.5f, y = t * (float)n - 0.5f;
    const float fx0 = floorf(x), fy0 = floorf(y);
    const float wx = x - fx0, wy = y - fy0;
    int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
    x0 = min(max(x0, 0), n - 1); x1 = min(max(x1, 0), n - 1);
    y0 = min(max(y0, 0), n - 1); y1 = min(max(y1, 0), n - 1);
    const float4* f = faces + (size_t)face * n * n;
    const float4 o = bilerp(f[(size_t)y0 * n + x0], f[(size_t)y0 * n + x1], f[(size_t)y1 * n + x0], f[(size_t)y1 * n + x1], wx, wy);
    return make_float4(o.x, o.y, o.z, 1.0f);
}

// One thread per pixel.  The rasterised cube's interpolated attribute `position` at a pixel is a positive multiple
// of the pixel's world-space view direction, so the lookup vector is that direction, re-ordered as the vertex
// shader does (skybox.wgsl:31-38): (x, -z, y), y negated again for a cube map.
__global__ __launch_bounds__(256) void k_skybox(const SkyArgs a, const float4* __restrict__ faces, float4* __restrict__ out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    float d[3];
    pixel_ray(a.V, a.p00, a.p11, x, y, a.width, a.height, d);
    float tx = d[0], ty = -d[2], tz = d[1];
    if (a.equirectangular == 0) ty = -ty;
    out[(size_t)y * a.width + x] = sample_cube(faces, a.face_size, tx, ty, tz);
}

void launch_skybox(hipStream_t s, const float* view16, float p00, float p11, int width, int height, int face_size, int equirect,
                   const float4* faces, float4* out)
{
    SkyArgs a;
    for (int i = 0; i < 16; i++) a.V[i] = view16[i];
    a.p00 = p00; a.p11 = p11; a.width = width; a.height = height; a.face_size = face_size; a.equirectangular = equirect;
    hipLaunchKernelGGL(k_skybox, dim3((width + 63) / 64, (height + 3) / 4), dim3(256), 0, s, a, faces, out);
}


// ---- proxy -----------------------------------------------------------------------------------------

// gswt_proxy_render_ortho (include/gswt_hip.h, "Ray of pixel (x, y)"): the origin of the pixel's ray, in the grid frame (world - (gx0, gy0, 0)).
// All rays share the direction ortho_d, -(V[2], V[6], V[10]); ortho_o is the point of camera-space (0, 0, z0), inverted in binary64 by the host.
__device__ __forceinline__ void ortho_origin(const ProxyArgs& a, int x, int y, float o[3])
{
    const float nx = ((float)x + 0.5f) / (float)a.width * 2.0f - 1.0f;
    const float ny = 1.0f - ((float)y + 0.5f) / (float)a.height * 2.0f;
    const float cx = (nx - a.ortho_t[0]) / a.p00, cy = (ny - a.ortho_t[1]) / a.p11;
    o[0] = (a.V[0] * cx + a.V[1] * cy) + a.ortho_o[0];
    o[1] = (a.V[4] * cx + a.V[5] * cy) + a.ortho_o[1];
    o[2] = (a.V[8] * cx + a.V[9] * cy) + a.ortho_o[2];
}

// Origin and direction of the ray of pixel (x, y), of both proxy kernels: the pixel's own and those of its right and lower neighbour.
// Perspective: the eye a.cam and pixel_ray; ORTHO: ortho_origin and the one direction a.ortho_d.
template <bool ORTHO>
__device__ __forceinline__ void proxy_ray(const ProxyArgs& a, int x, int y, float o[3], float d[3])
{
    if (ORTHO) {
        ortho_origin(a, x, y, o);
        d[0] = a.ortho_d[0]; d[1] = a.ortho_d[1]; d[2] = a.ortho_d[2];
    } else {
        o[0] = a.cam[0]; o[1] = a.cam[1]; o[2] = a.cam[2];
        pixel_ray(a.V, a.p00, a.p11, x, y, a.width, a.height, d);
    }
}

__device__ __forceinline__ float proxy_mapped_height(const ProxyArgs& a, const float* __restrict__ hm, float rx, float ry)
{
    if (a.surface_type != 1u) return 0.0f;
    const float xr = gswt_host::hm_axis_range(a.map_half_wh[0], a.tile_width, a.height_map_scale[0]);
    const float yr = gswt_host::hm_axis_range(a.map_half_wh[1], a.tile_width, a.height_map_scale[1]);
    const float h_u = gswt_host::hm_axis_coord(rx, a.map_half_wh[0], a.tile_width, xr);
    const float h_v = gswt_host::hm_axis_coord(ry, a.map_half_wh[1], a.tile_width, yr);
    return sample_height(hm, a.hm_w, a.hm_h, h_u, h_v) * a.height_map_scale[2];
}

__device__ __forceinline__ bool proxy_depth(const ProxyArgs& a, const float hp[3], float& depth)
{
    float cv[4], q[4];
    for (int r = 0; r < 4; r++) cv[r] = ((a.V[r] * hp[0] + a.V[4 + r] * hp[1]) + a.V[8 + r] * hp[2]) + a.V[12 + r];
    for (int r = 0; r < 4; r++) q[r] = ((a.GP[r] * cv[0] + a.GP[4 + r] * cv[1]) + a.GP[8 + r] * cv[2]) + a.GP[12 + r] * cv[3];
    depth = q[2] / q[3];
    return q[3] > 0.0f && depth >= 0.0f && depth <= 1.0f;
}

// Moeller-Trumbore + the fragment tests (fs_main discard, near / far clip); keeps the nearest
__device__ __forceinline__ bool proxy_tri(const ProxyArgs& a, const float o[3], const float d[3], const float* va, const float* vb,
                                          const float* vc, float ma, float mb, float mc, float& best_t, float& depth_out,
                                          float nrm[3], float pa[3])
{
    const float e1[3] = {vb[0] - va[0], vb[1] - va[1], vb[2] - va[2]}, e2[3] = {vc[0] - va[0], vc[1] - va[1], vc[2] - va[2]};
    const float pv[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
    const float det = (e1[0] * pv[0] + e1[1] * pv[1]) + e1[2] * pv[2];
    if (det == 0.0f) return false;
    const float tv[3] = {o[0] - va[0], o[1] - va[1], o[2] - va[2]};
    const float bu = ((tv[0] * pv[0] + tv[1] * pv[1]) + tv[2] * pv[2]) / det;
    if (!(bu >= 0.0f && bu <= 1.0f)) return false;
    const float qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
    const float bv = ((d[0] * qv[0] + d[1] * qv[1]) + d[2] * qv[2]) / det;
    if (!(bv >= 0.0f && bu + bv <= 1.0f)) return false;
    const float t = ((e2[0] * qv[0] + e2[1] * qv[1]) + e2[2] * qv[2]) / det;
    if (!(t > 0.0f && t < best_t)) return false;
    const float mh = (ma + bu * (mb - ma)) + bv * (mc - ma);
    if (a.use_clip == 1u && mh < a.clip_height) return false;
    const float hp[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
    float depth;
    if (!proxy_depth(a, hp, depth)) return false;
    best_t = t; depth_out = depth;
    nrm[0] = e1[1] * e2[2] - e1[2] * e2[1]; nrm[1] = e1[2] * e2[0] - e1[0] * e2[2]; nrm[2] = e1[0] * e2[1] - e1[1] * e2[0];
    pa[0] = va[0]; pa[1] = va[1]; pa[2] = va[2];
    return true;
}

__device__ __forceinline__ void proxy_plane_uv(const ProxyArgs& a, const float o[3], const float d[3], const float pa[3], const float nrm[3],
                                               float uv[2])
{
    const float num = (nrm[0] * (pa[0] - o[0]) + nrm[1] * (pa[1] - o[1])) + nrm[2] * (pa[2] - o[2]);
    const float den = (nrm[0] * d[0] + nrm[1] * d[1]) + nrm[2] * d[2];
    const float t = num / den;
    uv[0] = (o[0] + t * d[0]) / a.tile_width / 4.0f;
    uv[1] = (o[1] + t * d[1]) / a.tile_width / 4.0f;
}

__device__ __forceinline__ float4 proxy_tex_bilinear(const float4* __restrict__ lvl, int n, float u, float v)
{
    const float x = u * (float)n - 0.5f, y = v * (float)n - 0.5f;
    const float fx0 = floorf(x), fy0 = floorf(y);
    const float wx = x - fx0, wy = y - fy0;
    const int xa = wrap_repeat(fx0, n), ya = wrap_repeat(fy0, n);
    const int xb = xa + 1 == n ? 0 : xa + 1, yb = ya + 1 == n ? 0 : ya + 1;
    return bilerp(lvl[ya * n + xa], lvl[ya * n + xb], lvl[yb * n + xa], lvl[yb * n + xb], wx, wy);
}

// The two stages k_proxy and k_proxy_sphere share behind their own hit search.  What a kernel brings: the fragment's depth `dep`, its point
// hp = o + t d in the rays' frame with t and dd = |d|^2, the same point in WORLD coordinates hw, and (for the colour stage) the texture
// coordinate uv and the LOD's texels per pixel rho.
//
// proxy_write -- a fragment's depth state and what needs no texture: CompareFunction::Less against the depth buffer with depth write on, the
// black_background output, and (SHD) the shadow map's texel loads at hw, issued here so that the kernel's texturing arithmetic and the
// colour stage's own loads pass over their latency (shadow_fetch, gswt_device_fn.h).  false: the pixel is done.  Every store of either
// stage goes to pixel pi of the frame.
template <bool SHD>
__device__ __forceinline__ bool proxy_write(const ProxyArgs& a, const Shadow& shd, size_t pi, float dep, const float hw[3],
                                            float4* __restrict__ rgba, float* __restrict__ depth_buf, ShadowTap& tap)
{
    if (!(dep < depth_buf[pi])) return false;                     // CompareFunction::Less, depth write on
    depth_buf[pi] = dep;
    if (a.black_background == 1u) { rgba[pi] = make_float4(0.0f, 0.0f, 0.0f, 1.0f); return false; }
    if (SHD) tap = shadow_fetch(shd, hw[0], hw[1], hw[2]);
    return true;
}

// proxy_colour -- implicit-LOD trilinear texturing (levels clamped to [0, n_mips - 1], proxy_tex_bilinear's wrapped indices), `brightness`,
// then SHD: toward shade_color by the splats' own sh = strength * (1 - lit) (shadow_amount on proxy_write's tap), then FOG: toward fog_color
// by F of the hit's distance from the eye -- t |d| under the perspective camera, |hp - a.cam| under ORTHO, where a.cam is the reference
// point and not the rays' origin.
template <bool FOG, bool ORTHO, bool SHD>
__device__ __forceinline__ float4 proxy_colour(const ProxyArgs& a, const Shadow& shd, const ShadowTap& tap, const float4* __restrict__ tex,
                                               const float uv[2], float rho, const float hp[3], float t, float dd)
{
    float lod = log2f(rho);
    if (!(lod > 0.0f)) lod = 0.0f;
    if (lod > (float)(a.n_mips - 1)) lod = (float)(a.n_mips - 1);
    const int l0 = (int)floorf(lod), l1 = l0 + 1 > a.n_mips - 1 ? a.n_mips - 1 : l0 + 1;
    const float fl = lod - (float)l0;
    const float4 c0 = proxy_tex_bilinear(tex + a.mip_off[l0], a.tex_size >> l0, uv[0], uv[1]);
    const float4 c1 = proxy_tex_bilinear(tex + a.mip_off[l1], a.tex_size >> l1, uv[0], uv[1]);
    float4 px = make_float4((c0.x * (1.0f - fl) + c1.x * fl) * a.brightness, (c0.y * (1.0f - fl) + c1.y * fl) * a.brightness,
                            (c0.z * (1.0f - fl) + c1.z * fl) * a.brightness, 1.0f);
    if (SHD) {
        const float sh = shadow_amount(shd, tap);
        if (sh != 0.0f) {
            px.x = px.x * (1.0f - sh) + shd.shade[0] * sh;
            px.y = px.y * (1.0f - sh) + shd.shade[1] * sh;
            px.z = px.z * (1.0f - sh) + shd.shade[2] * sh;
        }
    }
    if (FOG) {
        float dist;
        if (ORTHO) {
            const float fx = hp[0] - a.cam[0], fy = hp[1] - a.cam[1], fz = hp[2] - a.cam[2];
            dist = sqrtf((fx * fx + fy * fy) + fz * fz);
        } else
            dist = t * sqrtf(dd);
        const float F = fog_amount(a.atm, dist);
        px.x = px.x * (1.0f - F) + a.atm.fog_color[0] * F;
        px.y = px.y * (1.0f - F) + a.atm.fog_color[1] * F;
        px.z = px.z * (1.0f - F) + a.atm.fog_color[2] * F;
    }
    return px;
}

// FOG (gswt_set_atmosphere's fog part on when the pass is called), SHD (gswt_set_shadow_map with a map on when the pass is called): the
// colour stage above; the depth, the pixels left alone and the black_background output are what they are without them.
// ORTHO (gswt_proxy_render_ortho): parallel rays, one origin per pixel (proxy_ray).  The grid walk, the hit and depth tests and the
// texturing are the same code; the rays of the right and the lower pixel differ from the pixel's own by their origin instead of their
// direction.  Rays, vertices, a.cam and the view's translation are in the grid frame, whose lattice starts at (0, 0): far from the world
// origin nothing here is rounded at the world coordinates' magnitude but the lattice itself (rx, ry: the reference's f32 vertices); the
// hit point goes back to WORLD coordinates by (gx0, gy0) for the shadow map and the clip volumes.
// CLIP (gswt_set_clip_volumes with a GSWT_CLIP_GROUND volume in force when the pass is called): clip_hidden (gswt_device_fn.h) over those
// volumes at the world hit point, in front of proxy_write: a hidden fragment is discarded, colour and depth keep what was there.  (On the
// HeightMap surface the fragment is the walk's first hit; the walk does not go on behind a hidden one.)
template <bool FOG, bool ORTHO, bool SHD, bool CLIP>
__global__ __launch_bounds__(256) void k_proxy(const ProxyArgs a, const float* __restrict__ hm, const float4* __restrict__ tex,
                                               float4* __restrict__ rgba, float* __restrict__ depth_buf, const Shadow shd, const ClipSet clip)
{
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= a.width || y >= a.height) return;
    float o[3], d[3];
    proxy_ray<ORTHO>(a, x, y, o, d);
    float best_t = 3.0e38f, dep = 1.0f, nrm[3] = {0.0f, 0.0f, 1.0f}, pa[3] = {0.0f, 0.0f, 0.0f};
    bool hit = false;
    const float fx0 = ORTHO ? 0.0f : a.gx0, fy0 = ORTHO ? 0.0f : a.gy0;      // the lattice's origin in the rays' frame
    const float ogx = (o[0] - fx0) / a.cs, ogy = (o[1] - fy0) / a.cs;
    const float dgx = d[0] / a.cs, dgy = d[1] / a.cs;
    float t0 = 0.0f, t1 = 3.0e38f;
    bool ok = true;
    if (dgx != 0.0f) {
        const float ta = (0.0f - ogx) / dgx, tb = ((float)a.nx - ogx) / dgx;
        t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb));
    } else if (!(ogx >= 0.0f && ogx <= (float)a.nx)) ok = false;
    if (dgy != 0.0f) {
        const float ta = (0.0f - ogy) / dgy, tb = ((float)a.ny - ogy) / dgy;
        t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb));
    } else if (!(ogy >= 0.0f && ogy <= (float)a.ny)) ok = false;
    if (ok && t0 <= t1) {
        if (a.surface_type != 1u) {
            const float tz = (a.height_offset - o[2]) / d[2];
            const float hx = o[0] + tz * d[0], hy = o[1] + tz * d[1];
            const float cxf = (hx - fx0) / a.cs, cyf = (hy - fy0) / a.cs;
            if (d[2] != 0.0f && tz > 0.0f && cxf >= 0.0f && cxf <= (float)a.nx && cyf >= 0.0f && cyf <= (float)a.ny &&
                !(a.use_clip == 1u && 0.0f < a.clip_height)) {
                const float hp[3] = {hx, hy, o[2] + tz * d[2]};
                float dz;
                if (proxy_depth(a, hp, dz)) {
                    hit = true; dep = dz; best_t = tz;
                    pa[0] = fx0; pa[1] = fy0; pa[2] = a.height_offset;
                }
            }
        } else {
            const float ex = ogx + t0 * dgx, ey = ogy + t0 * dgy;
            int ci = (int)floorf(ex), cj = (int)floorf(ey);
            ci = ci < 0 ? 0 : (ci > a.nx - 1 ? a.nx - 1 : ci); cj = cj < 0 ? 0 : (cj > a.ny - 1 ? a.ny - 1 : cj);
            const int sx = dgx > 0.0f ? 1 : -1, sy = dgy > 0.0f ? 1 : -1;
            float tmx = dgx != 0.0f ? ((float)(ci + (sx > 0 ? 1 : 0)) - ogx) / dgx : 3.0e38f;
            float tmy = dgy != 0.0f ? ((float)(cj + (sy > 0 ? 1 : 0)) - ogy) / dgy : 3.0e38f;
            const float tdx = dgx != 0.0f ? fabsf(1.0f / dgx) : 3.0e38f, tdy = dgy != 0.0f ? fabsf(1.0f / dgy) : 3.0e38f;
            const int max_steps = a.nx + a.ny + 2;          // every wave leaves the loop after at most this many cells
            for (int step = 0; step < max_steps; step++) {
                float v[4][3], m[4];
                for (int k = 0; k < 4; k++) {
                    const int vi = ci + (k & 1), vj = cj + (k >> 1);
                    const float rx = a.gx0 + (float)vi * a.cs, ry = a.gy0 + (float)vj * a.cs;
                    m[k] = proxy_mapped_height(a, hm, rx, ry);
                    v[k][0] = ORTHO ? rx - a.gx0 : rx; v[k][1] = ORTHO ? ry - a.gy0 : ry; v[k][2] = a.height_offset + m[k];
                }
                const bool h1 = proxy_tri(a, o, d, v[0], v[1], v[2], m[0], m[1], m[2], best_t, dep, nrm, pa);
                const bool h2 = proxy_tri(a, o, d, v[1], v[3], v[2], m[1], m[3], m[2], best_t, dep, nrm, pa);
                hit = hit || h1 || h2;
                if (hit) break;
                if (ORTHO && dgx == 0.0f && dgy == 0.0f) break;   // straight down: the one cell under the pixel
                if (tmx < tmy) { ci += sx; tmx += tdx; } else { cj += sy; tmy += tdy; }
                if (ci < 0 || ci >= a.nx || cj < 0 || cj >= a.ny) break;
            }
        }
    }
    if (!hit) return;
    const size_t pi = (size_t)y * a.width + x;
    float hw[3] = {0.0f, 0.0f, 0.0f};
    if (SHD || CLIP) {                                           // the hit point back in WORLD coordinates
        const float hx = o[0] + best_t * d[0], hy = o[1] + best_t * d[1], hz = o[2] + best_t * d[2];
        hw[0] = ORTHO ? hx + a.gx0 : hx; hw[1] = ORTHO ? hy + a.gy0 : hy; hw[2] = hz;
    }
    if (CLIP && clip_hidden(clip, hw[0], hw[1], hw[2])) return;
    ShadowTap tap;                                               // (SHD only: proxy_write sets it, proxy_colour reads it)
    if (!proxy_write<SHD>(a, shd, pi, dep, hw, rgba, depth_buf, tap)) return;
    float uv[2], uvx[2], uvy[2], on[3], dn[3];
    proxy_plane_uv(a, o, d, pa, nrm, uv);
    proxy_ray<ORTHO>(a, x + 1, y, on, dn);
    proxy_plane_uv(a, on, dn, pa, nrm, uvx);
    proxy_ray<ORTHO>(a, x, y + 1, on, dn);
    proxy_plane_uv(a, on, dn, pa, nrm, uvy);
    const float sz = (float)a.tex_size;
    const float ax = (uvx[0] - uv[0]) * sz, ay = (uvx[1] - uv[1]) * sz, bx = (uvy[0] - uv[0]) * sz, by = (uvy[1] - uv[1]) * sz;
    const float rho = fmaxf(sqrtf(ax * ax + ay * ay), sqrtf(bx * bx + by * by));
    if (ORTHO) { uv[0] = uv[0] + a.ortho_uv0[0]; uv[1] = uv[1] + a.ortho_uv0[1]; }      // grid frame -> world, modulo the texture's period
    // ... and in the rays' frame, for the fog: the same sums, written where they are used (in front of the depth test they stay live across the
    // texturing, 2 % more instructions in k_proxy<FOG, ORTHO>)
    const float hp[3] = {o[0] + best_t * d[0], o[1] + best_t * d[1], o[2] + best_t * d[2]};
    rgba[pi] = proxy_colour<FOG, ORTHO, SHD>(a, shd, tap, tex, uv, rho, hp, best_t, (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
}

// ---- sphere proxy ------------------------------------------------------------------------------------
// gswt_proxy_render_sphere (include/gswt_hip.h, "sphere proxy pass"): the ground under the Sphere surface.  The pixel's ray against the
// sphere |x| = r about the world origin, r = sphere_radius + height_offset; no grid, no walk: one pixel per lane, two candidate roots.
// The ray's closest point c to the centre comes first and the half chord from r r - c.c, so that a grazing ray cancels at the size of
// r^2 and not of |o|^2.  clamp: a neighbour ray of the LOD differences that misses at the silhouette takes its closest point.
__device__ __forceinline__ bool sphere_cut(const float o[3], const float d[3], float r, bool clamp, float& tc, float& h, float& dd)
{
    dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    tc = -((o[0] * d[0] + o[1] * d[1]) + o[2] * d[2]) / dd;
    const float c[3] = {o[0] + tc * d[0], o[1] + tc * d[1], o[2] + tc * d[2]};
    float disc = r * r - ((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    if (disc < 0.0f) {
        if (!clamp) return false;
        disc = 0.0f;
    }
    h = sqrtf(disc / dd);
    return true;
}

// the neighbour pixel's ray cut with the same sphere at the same root (second: tc + h), and its distance from the pixel's own hit
__device__ __forceinline__ float sphere_neighbour_dist(const float o[3], const float d[3], float r, bool second, const float hit[3])
{
    float tc, h, dd;
    sphere_cut(o, d, r, true, tc, h, dd);
    const float t = second ? tc + h : tc - h;
    const float ex = (o[0] + t * d[0]) - hit[0], ey = (o[1] + t * d[1]) - hit[1], ez = (o[2] + t * d[2]) - hit[2];
    return sqrtf((ex * ex + ey * ey) + ez * ez);
}

// FOG / ORTHO / SHD: proxy_ray, proxy_write and proxy_colour, the stages k_proxy runs; the ORTHO host set-up runs with g = 0, so origin,
// a.cam, the view's translation and the hit are in world coordinates.  The grid fields of a (nx, ny, cs, gx0, gy0), map_proxy, width_scale,
// surface_type and the height map are not read.  Every store goes to pixel (x, y) of the frame, inside width x height by the first test.
// CLIP: the GROUND volumes' test joins what a candidate must pass, beside clip_height's: behind a near surface that is cut away the inside
// of the far one shows.
template <bool FOG, bool ORTHO, bool SHD, bool CLIP>
__global__ __launch_bounds__(256) void k_proxy_sphere(const ProxyArgs a, const SphereProxyArgs sp, const float4* __restrict__ tex,
                                                      float4* __restrict__ rgba, float* __restrict__ depth_buf, const Shadow shd,
                                                      const ClipSet clip)
{
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= a.width || y >= a.height) return;
    float o[3], d[3];
    proxy_ray<ORTHO>(a, x, y, o, d);
    float tc, h, dd;
    if (!sphere_cut(o, d, sp.r, false, tc, h, dd)) return;
    bool hit = false, second = false;
    float t = 0.0f, dep = 1.0f, hp[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 2 && !hit; k++) {                        // t1 = tc - h, then t2 = tc + h: the first kept candidate is the fragment
        const float tk = k == 0 ? tc - h : tc + h;
        const float p[3] = {o[0] + tk * d[0], o[1] + tk * d[1], o[2] + tk * d[2]};
        float dz;
        if (!(tk > 0.0f) || !proxy_depth(a, p, dz)) continue;
        if (a.use_clip == 1u && (p[2] / sp.r) * sp.sphere_radius < a.clip_height) continue;
        if (CLIP && clip_hidden(clip, p[0], p[1], p[2])) continue;
        hit = true; second = k == 1; t = tk; dep = dz;
        hp[0] = p[0]; hp[1] = p[1]; hp[2] = p[2];
    }
    const size_t pi = (size_t)y * a.width + x;
    ShadowTap tap;                                               // (SHD only: proxy_write sets it, proxy_colour reads it)
    if (!hit) return;
    if (!proxy_write<SHD>(a, shd, pi, dep, hp, rgba, depth_buf, tap)) return;          // (g = 0: the rays' frame is the world)
    float px, py;
    gswt_host::sphere_plane_pos(sp.block_w, gswt_host::V3{hp[0] / sp.r, hp[1] / sp.r, hp[2] / sp.r}, px, py);
    float uv[2] = {(sp.org[0] + px) / a.tile_width / 4.0f, (sp.org[1] + py) / a.tile_width / 4.0f};
    if (!(fabsf(uv[0]) < 3.0e38f)) uv[0] = 0.0f;                 // (a finite hit gives finite coordinates; nothing else reaches the sampler)
    if (!(fabsf(uv[1]) < 3.0e38f)) uv[1] = 0.0f;
    // LOD from the world distance to the neighbour pixels' hits: free of the unfolding's seams and of the pinch at the poles
    float on[3], dn[3];
    proxy_ray<ORTHO>(a, x + 1, y, on, dn);
    const float ex = sphere_neighbour_dist(on, dn, sp.r, second, hp);
    proxy_ray<ORTHO>(a, x, y + 1, on, dn);
    const float ey = sphere_neighbour_dist(on, dn, sp.r, second, hp);
    rgba[pi] = proxy_colour<FOG, ORTHO, SHD>(a, shd, tap, tex, uv, fmaxf(ex, ey) * sp.lod_k, hp, t, dd);
}

// ---- skybox bake -----------------------------------------------------------------------------------
// skybox.wgsl vs_bake + fs_bake: one render pass per face draws the unit cube from the origin with perspective(90 deg, 1, 0.1, 10)
// and look_at_rh(0, target_i, up_i) into the face; the interpolated cube position is a positive multiple of the pixel's view ray,
// s*ndc_x/P00 + u*ndc_y/P11 + f, and P00 = P11 cancels in the normalize.  Then SampleSphericalMap with its truncated constants
// (skybox.wgsl:89-96), one bilinear tap of the Rgba32Float panorama (Linear, Repeat in u and v, level 0; row 0 = v 0) and the
// Reinhard + 1/2.2 gamma tone map (skybox.wgsl:74-84).  One lane per output texel, a wave per 64 texels of a row (1 KB of float4).
__global__ __launch_bounds__(256) void k_skybox_bake(const SkyBakeArgs a, const float4* __restrict__ equi, float4* __restrict__ faces)
{
    const int n = a.face_size;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), face = blockIdx.z;
    if (x >= n || y >= n) return;
    const float nx = ((float)x + 0.5f) / (float)n * 2.0f - 1.0f;
    const float ny = 1.0f - ((float)y + 0.5f) / (float)n * 2.0f;
    const float* b = a.basis[face];
    float dx = (b[0] * nx + b[3] * ny) + b[6];
    float dy = (b[1] * nx + b[4] * ny) + b[7];
    float dz = (b[2] * nx + b[5] * ny) + b[8];
    const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
    dx /= len; dy /= len; dz /= len;
    const float u = atan2f(dz, dx) * 0.1591f + 0.5f;
    const float v = asinf(fminf(fmaxf(dy, -1.0f), 1.0f)) * 0.3183f + 0.5f;
    const int w = a.equi_w, h = a.equi_h;
    const float sx = u * (float)w - 0.5f, sy = v * (float)h - 0.5f;
    const float fx0 = floorf(sx), fy0 = floorf(sy);
    const float tx = sx - fx0, ty = sy - fy0;
    const int xa = wrap_repeat(fx0, w), ya = wrap_repeat(fy0, h);
    const int xb = xa + 1 == w ? 0 : xa + 1, yb = ya + 1 == h ? 0 : ya + 1;
    const float4 tap = bilerp(equi[(size_t)ya * w + xa], equi[(size_t)ya * w + xb], equi[(size_t)yb * w + xa], equi[(size_t)yb * w + xb], tx, ty);
    float c[3] = {tap.x, tap.y, tap.z};
    const float gamma = (float)(1.0 / 2.2);          // the f32 constant of pow(color, vec3(1.0/2.2))
    for (int k = 0; k < 3; k++) {
        const float r = c[k] / (c[k] + 1.0f);
        c[k] = exp2f(log2f(r) * gamma);              // pow(r, g) = exp2(g * log2 r); r = 0 -> 0
    }
    // Non-temporal: the 403 MB of faces are not read again by this kernel (k_skybox_bake, 4096 x 2048 -> 2048^2 x 6, rocprofv3
    // mean of 22 calls: 227.3 us against 232.9 us with plain stores; profiles/skybox_bake_2048.txt)
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v o = {c[0], c[1], c[2], 1.0f};
    __builtin_nontemporal_store(o, reinterpret_cast<f4v*>(faces) + ((size_t)face * n + y) * n + x);
}

void launch_skybox_bake(hipStream_t s, const SkyBakeArgs& a, const float4* equi, float4* faces)
{
    const int n = a.face_size;
    hipLaunchKernelGGL(k_skybox_bake, dim3((n + 63) / 64, (n + 3) / 4, 6), dim3(256), 0, s, a, equi, faces);
}

// ---- proxy texture mip build ------------------------------------------------------------------------
// upload_proxy_texture (proxy.rs:513-554): level n = image::imageops::resize(original, n, n, Lanczos3), then to_rgba32f.  For an
// 8- / 16-bit RGBA image the crate runs, all in f32:
//   per axis (in -> out): ratio = in / out, sratio = max(ratio, 1), support = 3 sratio; output o has centre c = (o + 0.5) ratio,
//     taps i in [left, right) with left = clamp(floor(c - support), 0, in - 1), right = clamp(ceil(c + support), left + 1, in),
//     weights L((i - (c - 0.5)) / sratio) divided by their sum (taps outside the image are dropped, the rest renormalised);
//     L(x) = sinc(x) sinc(x / 3) for |x| < 3, sinc(t) = sin(pi t) / (pi t);
//   a vertical pass (h -> n rows) into an unclamped f32 image in source units, then a horizontal pass (w -> n columns) whose
//   outputs are clamp(t, 0, MAX) rounded half away from zero; to_rgba32f divides by MAX.  (n, n) == (w, h) is a plain copy.
// Accumulation is t = t + v * w (-ffp-contract=off: no fma), like the crate's loop.  The crate sums in tap order; here the
// vertical pass may split an output's taps into runs summed separately and the horizontal pass spreads them over G lanes,
// both reduced in a fixed order: the result is deterministic, and within the f32 rounding of a reordered sum of the crate's.

constexpr float kPiF = 3.14159265358979323846f;     // core::f32::consts::PI

__device__ __forceinline__ float lanczos3(float x)
{
    if (!(fabsf(x) < 3.0f)) return 0.0f;
    const float x3 = x / 3.0f;
    const float a = x * kPiF, b = x3 * kPiF;
    const float s0 = x == 0.0f ? 1.0f : sinf(a) / a;           // full-precision sinf, IEEE division
    const float s1 = x3 == 0.0f ? 1.0f : sinf(b) / b;
    return s0 * s1;
}

// Tap tables of one level, both axes (blockIdx.y: 0 vertical over the source rows, 1 horizontal over its columns): one wave per
// output; ranges[axis * n + o] = (left, count), w[o * stride + k] = the normalised weight of source index left + k.
__global__ __launch_bounds__(64) void k_lanczos_taps(const ProxyMipArgs a, int2* __restrict__ ranges, float* __restrict__ wv,
                                                     float* __restrict__ wh)
{
    const int axis = blockIdx.y, o = blockIdx.x, lane = threadIdx.x;
    const int in = axis == 0 ? a.src_h : a.src_w, stride = axis == 0 ? a.stride_v : a.stride_h;
    float* w = (axis == 0 ? wv : wh) + (size_t)o * stride;
    const float ratio = (float)in / (float)a.n;
    const float sratio = ratio < 1.0f ? 1.0f : ratio;
    const float support = 3.0f * sratio;
    const float c = ((float)o + 0.5f) * ratio;
    const int left = min(max((int)floorf(c - support), 0), in - 1);
    const int right = min(max((int)ceilf(c + support), left + 1), in);
    const int cnt = min(right - left, stride);                  // (plan_proxy_mip sizes stride above any count)
    const float cc = c - 0.5f;
    float part = 0.0f;
    for (int k = lane; k < cnt; k += 64) {
        const float r = lanczos3(((float)(left + k) - cc) / sratio);
        w[k] = r;
        part = part + r;
    }
    for (int off = 32; off > 0; off >>= 1) part = part + __shfl_down(part, off, 64);
    const float sum = __shfl(part, 0, 64);
    for (int k = lane; k < cnt; k += 64) w[k] = w[k] / sum;     // each lane rescales what it wrote
    if (lane == 0) ranges[axis * a.n + o] = make_int2(left, cnt);
}

// 16 source bytes: 4 RGBA8 texels (R in the low byte of each dword) or 2 RGBA16 texels (R in the low half of the first dword)
template <bool U16>
__device__ __forceinline__ void unpack16(const uint4 q, float4* v)
{
    if (U16) {
        v[0] = make_float4((float)(q.x & 0xffffu), (float)(q.x >> 16), (float)(q.y & 0xffffu), (float)(q.y >> 16));
        v[1] = make_float4((float)(q.z & 0xffffu), (float)(q.z >> 16), (float)(q.w & 0xffffu), (float)(q.w >> 16));
    } else {
        const uint32_t d[4] = {q.x, q.y, q.z, q.w};
        for (int p = 0; p < 4; p++)
            v[p] = make_float4((float)(d[p] & 255u), (float)((d[p] >> 8) & 255u), (float)((d[p] >> 16) & 255u), (float)(d[p] >> 24));
    }
}

// Vertical pass: lane = one 16-byte column group of the source (4 or 2 texels), blockIdx.y = output row o, blockIdx.z = run s of
// o's taps.  Every lane of a wave loads 16 B of the same source row (1 KiB per wave-instruction); the weight is wave-uniform.
// out: the intermediate [n][src_w] (one run) or the partial sums [splits][n][src_w].
template <bool U16>
__global__ __launch_bounds__(64) void k_lanczos_v(const ProxyMipArgs a, const uint8_t* __restrict__ src, const int2* __restrict__ ranges,
                                                  const float* __restrict__ wv, float4* __restrict__ out)
{
    constexpr int P = U16 ? 2 : 4;
    const int g = blockIdx.x * 64 + threadIdx.x, o = blockIdx.y, s = blockIdx.z;
    const int x0 = g * P;
    if (x0 >= a.src_w) return;
    const int2 r = ranges[o];
    const int k0 = s * a.chunk, k1 = min(r.y, k0 + a.chunk);
    const float* w = wv + (size_t)o * a.stride_v;
    const uint8_t* col = src + (size_t)r.x * a.pitch + (size_t)g * 16;
    float4 acc[P];
    for (int p = 0; p < P; p++) acc[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 4
    for (int k = k0; k < k1; k++) {
        float4 v[P];
        unpack16<U16>(*reinterpret_cast<const uint4*>(col + (size_t)k * a.pitch), v);
        const float wk = w[k];
        for (int p = 0; p < P; p++) {
            acc[p].x = acc[p].x + v[p].x * wk;
            acc[p].y = acc[p].y + v[p].y * wk;
            acc[p].z = acc[p].z + v[p].z * wk;
            acc[p].w = acc[p].w + v[p].w * wk;
        }
    }
    float4* dst = out + ((size_t)s * a.n + o) * a.src_w + x0;
    for (int p = 0; p < P; p++)
        if (x0 + p < a.src_w) dst[p] = acc[p];
}

// The runs of a split vertical pass, summed in run order.
__global__ __launch_bounds__(256) void k_lanczos_v_sum(const ProxyMipArgs a, const float4* __restrict__ part, float4* __restrict__ out)
{
    const size_t m = (size_t)a.n * a.src_w, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    float4 t = part[i];
    for (int s = 1; s < a.splits; s++) {
        const float4 v = part[(size_t)s * m + i];
        t.x = t.x + v.x; t.y = t.y + v.y; t.z = t.z + v.z; t.w = t.w + v.w;
    }
    out[i] = t;
}

__device__ __forceinline__ float quantise(float t, float maxv)
{
    return roundf(fminf(fmaxf(t, 0.0f), maxv)) / maxv;          // clamp, FloatNearest (half away from zero), to_rgba32f
}

// Horizontal pass: G consecutive lanes per output texel (o, y) take its taps k = j, j + G, ... (adjacent lanes read adjacent
// intermediate texels), then a shuffle tree in a fixed order; lane j = 0 stores the quantised texel.
template <int G>
__global__ __launch_bounds__(256) void k_lanczos_h(const ProxyMipArgs a, const float4* __restrict__ tmp, const int2* __restrict__ ranges,
                                                   const float* __restrict__ wh, float4* __restrict__ dst)
{
    const int o = blockIdx.x * (256 / G) + threadIdx.x / G, j = threadIdx.x % G, y = blockIdx.y;
    float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (o < a.n) {
        const int2 r = ranges[a.n + o];
        const float* w = wh + (size_t)o * a.stride_h;
        const float4* row = tmp + (size_t)y * a.src_w + r.x;
        for (int k = j; k < r.y; k += G) {
            const float4 v = row[k];
            const float wk = w[k];
            t.x = t.x + v.x * wk; t.y = t.y + v.y * wk; t.z = t.z + v.z * wk; t.w = t.w + v.w * wk;
        }
    }
    for (int off = G / 2; off > 0; off >>= 1) {
        t.x = t.x + __shfl_down(t.x, off, G); t.y = t.y + __shfl_down(t.y, off, G);
        t.z = t.z + __shfl_down(t.z, off, G); t.w = t.w + __shfl_down(t.w, off, G);
    }
    if (j == 0 && o < a.n)
        dst[(size_t)y * a.n + o] = make_float4(quantise(t.x, a.maxv), quantise(t.y, a.maxv), quantise(t.z, a.maxv), quantise(t.w, a.maxv));
}

// Copy level: x / MAX per channel, 16 source bytes per lane.
template <bool U16>
__global__ __launch_bounds__(64) void k_proxy_mip_copy(const ProxyMipArgs a, const uint8_t* __restrict__ src, float4* __restrict__ dst)
{
    constexpr int P = U16 ? 2 : 4;
    const int g = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y;
    const int x0 = g * P;
    if (x0 >= a.n) return;
    float4 v[P];
    unpack16<U16>(*reinterpret_cast<const uint4*>(src + (size_t)y * a.pitch + (size_t)g * 16), v);
    float4* d = dst + (size_t)y * a.n + x0;
    for (int p = 0; p < P; p++)
        if (x0 + p < a.n) d[p] = make_float4(v[p].x / a.maxv, v[p].y / a.maxv, v[p].z / a.maxv, v[p].w / a.maxv);
}

ProxyMipArgs plan_proxy_mip(int src_w, int src_h, int n, int u16, int pitch)
{
    ProxyMipArgs a{};
    a.src_w = src_w; a.src_h = src_h; a.n = n; a.u16 = u16; a.pitch = pitch;
    a.copy = n == src_w && n == src_h;
    a.maxv = u16 ? 65535.0f : 255.0f;
    // A count is right - left <= ceil(fl(c + support)) - floor(fl(c - support)) < 2 support + 2 + (rounding of the two sums,
    // < 2^-6 at these sizes): at most floor(2 support) + 3 taps, and never more than the axis has.
    auto stride = [n](int in) {
        const float ratio = (float)in / (float)n, support = 3.0f * (ratio < 1.0f ? 1.0f : ratio);
        return std::min(in, (int)(2.0f * support) + 4);
    };
    a.stride_v = stride(src_h); a.stride_h = stride(src_w);
    // Split the vertical taps when the level has few outputs: aim at ~2048 waves, runs of at least 64 taps.  splits * n *
    // groups <= 2048 bounds the partial sums at 2048 * 64 * 4 texels * 16 B = 8 MiB.
    const int groups = ((src_w + (u16 ? 1 : 3)) / (u16 ? 2 : 4) + 63) / 64;
    const long base = (long)groups * n;
    a.splits = 1;
    if (a.stride_v >= 128 && base < 2048) a.splits = (int)std::max(1L, std::min(2048 / base, (long)(a.stride_v / 64)));
    a.chunk = (a.stride_v + a.splits - 1) / a.splits;
    a.splits = (a.stride_v + a.chunk - 1) / a.chunk;
    return a;
}

template <int G>
static void launch_lanczos_h(hipStream_t s, const ProxyMipArgs& a, const float4* tmp, const int2* ranges, const float* wh, float4* dst)
{
    hipLaunchKernelGGL(k_lanczos_h<G>, dim3((a.n + 256 / G - 1) / (256 / G), a.n), dim3(256), 0, s, a, tmp, ranges, wh, dst);
}

void launch_proxy_mip(hipStream_t s, const ProxyMipArgs& a, const uint8_t* src, int2* ranges, float* wv, float* wh, float4* tmp,
                      float4* part, float4* dst)
{
    const int P = a.u16 ? 2 : 4;
    if (a.copy) {
        const dim3 grid(((a.n + P - 1) / P + 63) / 64, a.n);
        if (a.u16) hipLaunchKernelGGL(k_proxy_mip_copy<true>, grid, dim3(64), 0, s, a, src, dst);
        else hipLaunchKernelGGL(k_proxy_mip_copy<false>, grid, dim3(64), 0, s, a, src, dst);
        return;
    }
    hipLaunchKernelGGL(k_lanczos_taps, dim3(a.n, 2), dim3(64), 0, s, a, ranges, wv, wh);
    const dim3 vgrid(((a.src_w + P - 1) / P + 63) / 64, a.n, a.splits);
    float4* vout = a.splits > 1 ? part : tmp;
    if (a.u16) hipLaunchKernelGGL(k_lanczos_v<true>, vgrid, dim3(64), 0, s, a, src, ranges, wv, vout);
    else hipLaunchKernelGGL(k_lanczos_v<false>, vgrid, dim3(64), 0, s, a, src, ranges, wv, vout);
    if (a.splits > 1) {
        const size_t m = (size_t)a.n * a.src_w;
        hipLaunchKernelGGL(k_lanczos_v_sum, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, s, a, part, tmp);
    }
    // G lanes per output: about 16 taps per lane or more, up to a wave
    int G = 1;
    while (G < 64 && G * 16 < a.stride_h) G *= 2;
    switch (G) {
    case 1: launch_lanczos_h<1>(s, a, tmp, ranges, wh, dst); break;
    case 2: launch_lanczos_h<2>(s, a, tmp, ranges, wh, dst); break;
    case 4: launch_lanczos_h<4>(s, a, tmp, ranges, wh, dst); break;
    case 8: launch_lanczos_h<8>(s, a, tmp, ranges, wh, dst); break;
    case 16: launch_lanczos_h<16>(s, a, tmp, ranges, wh, dst); break;
    case 32: launch_lanczos_h<32>(s, a, tmp, ranges, wh, dst); break;
    default: launch_lanczos_h<64>(s, a, tmp, ranges, wh, dst); break;
    }
}

__global__ __launch_bounds__(256) void k_fill_f32(float* __restrict__ p, size_t n, float v)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

void launch_fill_f32(hipStream_t s, float* p, size_t n, float v)
{
    if (n) hipLaunchKernelGGL(k_fill_f32, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, p, n, v);
}

// A proxy pass's instantiation, for both kernels: fn(FOG, ORTHO, SHD, CLIP, grid), the constants in the kernels' template order
// <FOG, ORTHO, SHD, CLIP>.  FOG from the fog part of a.atm, SHD from the shadow map in force, CLIP from the GROUND volumes in force (all read
// when the pass is called), ORTHO from the entry point.
template <typename Fn>
static void with_proxy_variant(const ProxyArgs& a, bool ortho, const Shadow& shd, const ClipSet& clip, Fn&& fn)
{
    const dim3 grid((a.width + 15) / 16, (a.height + 15) / 16);
    const bool fog = a.atm.fog_density > 0.0f, shade = shd.z != nullptr;
    with_variant([&](auto FOG, auto ORTHO, auto SHD, auto CLIP) { fn(FOG, ORTHO, SHD, CLIP, grid); }, fog, ortho, shade, clip.n > 0u);
}

void launch_proxy(hipStream_t s, const ProxyArgs& a, bool ortho, const Shadow& shd, const ClipSet& clip, const float* hm, const float4* tex,
                  float4* rgba, float* depth)
{
    with_proxy_variant(a, ortho, shd, clip, [&](auto FOG, auto ORTHO, auto SHD, auto CLIP, dim3 grid) {
        hipLaunchKernelGGL((k_proxy<FOG, ORTHO, SHD, CLIP>), grid, dim3(256), 0, s, a, hm, tex, rgba, depth, shd, clip);
    });
}

void launch_proxy_sphere(hipStream_t s, const ProxyArgs& a, const SphereProxyArgs& sp, bool ortho, const Shadow& shd, const ClipSet& clip,
                         const float4* tex, float4* rgba, float* depth)
{
    with_proxy_variant(a, ortho, shd, clip, [&](auto FOG, auto ORTHO, auto SHD, auto CLIP, dim3 grid) {
        hipLaunchKernelGGL((k_proxy_sphere<FOG, ORTHO, SHD, CLIP>), grid, dim3(256), 0, s, a, sp, tex, rgba, depth, shd, clip);
    });
}

}  // namespace gswt
