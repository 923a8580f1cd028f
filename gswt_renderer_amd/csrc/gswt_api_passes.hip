// gswt_api_passes.hip -- the background passes of libgswt_hip.so (host only): the skybox (cube map from the host or baked from an
// equirectangular panorama) and the proxy plane (mip chain from the host or built from its image); kernels in gswt_passes.hip.
#include "gswt_ctx.h"

#include <algorithm>
#include <cmath>

using namespace gswt;

extern "C" {

int gswt_skybox_configure(gswt_ctx* c, const float* faces_rgba, int face_size, int equirectangular)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    if (!faces_rgba || face_size <= 0 || face_size > 16384) return fail(c, GSWT_ERR_BAD_ARG, "gswt_skybox_configure: bad cube map");
    hipSetDevice(c->device);
    HIP_TRY(c, sync_all(c));
    const size_t n = (size_t)6 * face_size * face_size;
    HIP_TRY(c, c->sky_faces.ensure(n));
    HIP_TRY(c, hipMemcpy(c->sky_faces.p, faces_rgba, n * 16, hipMemcpyHostToDevice));
    HIP_TRY(c, null_stream_done());
    c->sky_size = face_size; c->sky_equi = equirectangular ? 1 : 0;
    return GSWT_OK;
} GSWT_CATCH

// The bake views of skybox.rs:584-617 as cgmath's Matrix4::look_at_rh(origin, target, up) builds them: f = normalize(target),
// s = normalize(f x up), u = s x f (the view's rows are s, u, -f).  Their entries are 0 / +-1, so the f32 arithmetic is exact.
static void sky_bake_basis(const float t[3], const float up[3], float out[9])
{
    const float fl = sqrtf((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    const float f[3] = {t[0] / fl, t[1] / fl, t[2] / fl};
    float s[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
    const float sl = sqrtf((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    for (float& v : s) v /= sl;
    const float u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
    for (int k = 0; k < 3; k++) { out[k] = s[k]; out[3 + k] = u[k]; out[6 + k] = f[k]; }
}

int gswt_skybox_configure_equirect(gswt_ctx* c, const float* equi_rgba, int equi_width, int equi_height, int face_size)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    if (!equi_rgba) return fail(c, GSWT_ERR_BAD_ARG, "gswt_skybox_configure_equirect: null panorama");
    if (equi_width <= 0 || equi_width > 32768 || equi_height <= 0 || equi_height > 32768)
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_skybox_configure_equirect: bad panorama size %d x %d", equi_width, equi_height);
    if (face_size <= 0 || face_size > 16384) return fail(c, GSWT_ERR_BAD_ARG, "gswt_skybox_configure_equirect: bad face size %d", face_size);
    hipSetDevice(c->device);
    HIP_TRY(c, sync_all(c));
    // the panorama is staged for this call only (up to 16 GiB at the size limit; the reference's 4096 x 2048 is 128 MiB)
    const size_t ne = (size_t)equi_width * equi_height, nf = (size_t)6 * face_size * face_size;
    DevBuf<float4> equi;
    HIP_TRY(c, equi.ensure(ne));
    HIP_TRY(c, hipMemcpy(equi.p, equi_rgba, ne * 16, hipMemcpyHostToDevice));
    HIP_TRY(c, null_stream_done());
    HIP_TRY(c, c->sky_faces.ensure(nf));          // a failed allocation keeps the old buffer
    // Up to here a failure leaves the previous skybox as it was; from here on the faces are being overwritten (or the old buffer
    // is gone), so a failed bake leaves no skybox (gswt_skybox_render returns GSWT_ERR_STATE) rather than a half-written one.
    c->sky_size = 0;
    SkyBakeArgs a;
    static const float target[6][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, -1}, {0, 0, 1}};
    static const float up[6][3] = {{0, 1, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, -1}, {0, 1, 0}, {0, 1, 0}};
    for (int i = 0; i < 6; i++) sky_bake_basis(target[i], up[i], a.basis[i]);
    a.face_size = face_size; a.equi_w = equi_width; a.equi_h = equi_height;
    launch_skybox_bake(c->stream, a, equi.p, c->sky_faces.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->sky_size = face_size; c->sky_equi = 1;
    return GSWT_OK;
} GSWT_CATCH

int gswt_skybox_download(gswt_ctx* c, float* faces_rgba_host)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    if (!faces_rgba_host) return fail(c, GSWT_ERR_BAD_ARG, "gswt_skybox_download: null destination");
    if (c->sky_size == 0) return fail(c, GSWT_ERR_STATE, "gswt_skybox_download before a skybox configure");
    hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(faces_rgba_host, c->sky_faces.p, (size_t)6 * c->sky_size * c->sky_size * 16, hipMemcpyDeviceToHost));
    return GSWT_OK;
} GSWT_CATCH

int gswt_skybox_render(gswt_ctx* c, const gswt_camera_uniforms* cam, int width, int height, float* out_rgba_dev)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    if (!cam || !out_rgba_dev || width <= 0 || height <= 0) return fail(c, GSWT_ERR_BAD_ARG, "gswt_skybox_render: bad argument");
    if (c->sky_size == 0) return fail(c, GSWT_ERR_STATE, "gswt_skybox_render before gswt_skybox_configure");
    if (cam->projection[0] == 0.0f || cam->projection[5] == 0.0f) return fail(c, GSWT_ERR_BAD_ARG, "gswt_skybox_render: singular projection");
    hipSetDevice(c->device);
    launch_skybox(c->stream, cam->view, cam->projection[0], cam->projection[5], width, height, c->sky_size, c->sky_equi, c->sky_faces.p,
                  reinterpret_cast<float4*>(out_rgba_dev));
    HIP_TRY(c, hipGetLastError());
    return GSWT_OK;
} GSWT_CATCH

int gswt_proxy_configure(gswt_ctx* c, const float* const* mips, int tex_size, int n_mips, int grid_dim)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    if (!mips || tex_size <= 0 || n_mips <= 0 || n_mips > 16 || (tex_size >> (n_mips - 1)) < 1 || grid_dim <= 0 || grid_dim > 32768)
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_proxy_configure: bad mip chain / grid");
    hipSetDevice(c->device);
    HIP_TRY(c, sync_all(c));
    size_t total = 0;
    for (int l = 0; l < n_mips; l++) {
        if (!mips[l]) return fail(c, GSWT_ERR_BAD_ARG, "gswt_proxy_configure: mip %d is null", l);
        c->proxy_mip_off[l] = (uint32_t)total;
        total += (size_t)(tex_size >> l) * (tex_size >> l);
    }
    if (total >= 0xFFFFFFFFull) return fail(c, GSWT_ERR_CAPACITY, "gswt_proxy_configure: texture too large");
    HIP_TRY(c, c->proxy_tex.ensure(total));
    for (int l = 0; l < n_mips; l++)
        HIP_TRY(c, hipMemcpy(c->proxy_tex.p + c->proxy_mip_off[l], mips[l], (size_t)(tex_size >> l) * (tex_size >> l) * 16, hipMemcpyHostToDevice));
    HIP_TRY(c, null_stream_done());
    c->proxy_size = tex_size; c->proxy_mips = n_mips; c->proxy_grid_dim = grid_dim;
    return GSWT_OK;
} GSWT_CATCH

// upload_proxy_texture + Proxy::configure (proxy.rs:513-554, 289-318): every level resampled from the original image on the device
// (gswt_passes.hip, "proxy texture mip build").  The source, the tap tables, the intermediate and the partial sums live for this
// call only; the staged source rows are padded to 16 bytes so that every lane's 16-byte load is aligned.
int gswt_proxy_configure_image(gswt_ctx* c, const void* pixels, int width, int height, int src_format, int tex_size, int grid_dim)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    if (!pixels) return fail(c, GSWT_ERR_BAD_ARG, "gswt_proxy_configure_image: null image");
    if (width <= 0 || width > 16384 || height <= 0 || height > 16384)
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_proxy_configure_image: bad image size %d x %d", width, height);
    if (src_format != GSWT_PROXY_SRC_RGBA8 && src_format != GSWT_PROXY_SRC_RGBA16)
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_proxy_configure_image: bad source format %d", src_format);
    if (tex_size <= 0 || tex_size > 16384 || (tex_size & (tex_size - 1)) != 0)
        return fail(c, GSWT_ERR_BAD_ARG, "gswt_proxy_configure_image: texture size %d is not a power of two in 1..16384", tex_size);
    if (grid_dim <= 0 || grid_dim > 32768) return fail(c, GSWT_ERR_BAD_ARG, "gswt_proxy_configure_image: bad grid %d", grid_dim);
    hipSetDevice(c->device);
    HIP_TRY(c, sync_all(c));
    const int u16 = src_format == GSWT_PROXY_SRC_RGBA16 ? 1 : 0;
    const size_t row_bytes = (size_t)width * (u16 ? 8 : 4), pitch = (row_bytes + 15) / 16 * 16;
    int n_mips = 0;
    uint32_t mip_off[16] = {};
    size_t total = 0, n_tmp = 0, n_part = 0, n_wv = 0, n_wh = 0;
    std::vector<ProxyMipArgs> plan;
    for (int n = tex_size; n >= 1; n >>= 1, n_mips++) {
        mip_off[n_mips] = (uint32_t)total;
        total += (size_t)n * n;
        plan.push_back(plan_proxy_mip(width, height, n, u16, (int)pitch));
        n_tmp = std::max(n_tmp, proxy_mip_tmp_texels(plan.back()));
        n_part = std::max(n_part, proxy_mip_part_texels(plan.back()));
        n_wv = std::max(n_wv, proxy_mip_weights(plan.back(), 0));
        n_wh = std::max(n_wh, proxy_mip_weights(plan.back(), 1));
    }
    DevBuf<uint8_t> src;
    DevBuf<float4> tmp, part;
    DevBuf<int2> ranges;
    DevBuf<float> wv, wh;
    HIP_TRY(c, src.ensure(pitch * height));
    HIP_TRY(c, hipMemcpy2D(src.p, pitch, pixels, row_bytes, row_bytes, height, hipMemcpyHostToDevice));
    HIP_TRY(c, null_stream_done());
    HIP_TRY(c, tmp.ensure(n_tmp));
    HIP_TRY(c, part.ensure(n_part));
    HIP_TRY(c, ranges.ensure((size_t)2 * tex_size));
    HIP_TRY(c, wv.ensure(n_wv));
    HIP_TRY(c, wh.ensure(n_wh));
    HIP_TRY(c, c->proxy_tex.ensure(total));       // a failed allocation keeps the old texture
    // From here on the old texture is being overwritten: a failure leaves no proxy (proxy_size = 0), never a half-written one.
    c->proxy_size = 0; c->proxy_mips = 0;
    for (int l = 0; l < n_mips; l++)
        launch_proxy_mip(c->stream, plan[l], src.p, ranges.p, wv.p, wh.p, tmp.p, part.p, c->proxy_tex.p + mip_off[l]);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    memcpy(c->proxy_mip_off, mip_off, sizeof(mip_off));
    c->proxy_size = tex_size; c->proxy_mips = n_mips; c->proxy_grid_dim = grid_dim;
    return GSWT_OK;
} GSWT_CATCH

int gswt_proxy_download(gswt_ctx* c, float* mips_rgba_host)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    if (!mips_rgba_host) return fail(c, GSWT_ERR_BAD_ARG, "gswt_proxy_download: null destination");
    if (c->proxy_size == 0) return fail(c, GSWT_ERR_STATE, "gswt_proxy_download before a proxy configure");
    hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    size_t total = 0;                             // the levels are packed (proxy_mip_off)
    for (int l = 0; l < c->proxy_mips; l++) total += (size_t)(c->proxy_size >> l) * (c->proxy_size >> l);
    HIP_TRY(c, hipMemcpy(mips_rgba_host, c->proxy_tex.p, total * 16, hipMemcpyDeviceToHost));
    return GSWT_OK;
} GSWT_CATCH

// The kernel's argument block of one proxy draw: the uniforms, the grid they select (proxy.rs:136-163 / 219-251) and the context's resources.
static void proxy_args(const gswt_ctx* c, const gswt_proxy_uniforms* u, int width, int height, ProxyArgs& a)
{
    memset(&a, 0, sizeof(a));
    a.height_offset = u->height_offset; a.tile_width = u->tile_width; a.width_scale = u->width_scale; a.clip_height = u->clip_height;
    a.brightness = u->brightness; a.surface_type = u->surface_type; a.use_clip = u->use_clip; a.black_background = u->black_background;
    memcpy(a.V, u->view, 64);
    gl_to_wgpu_projection(u->projection, a.GP);
    a.p00 = u->projection[0]; a.p11 = u->projection[5];
    for (int k = 0; k < 3; k++) { a.cam[k] = u->cam_pos[k]; a.height_map_scale[k] = u->height_map_scale[k]; }
    a.map_half_wh[0] = u->map_half_wh[0]; a.map_half_wh[1] = u->map_half_wh[1];
    const float tw = u->tile_width;
    if (u->map_proxy == 1u) {                 // proxy.rs:219-251 + proxy.wgsl:51
        a.nx = 2 * (int)u->map_half_wh[0] + 1; a.ny = 2 * (int)u->map_half_wh[1] + 1; a.cs = tw;
        a.gx0 = (float)(-(int)u->map_half_wh[0]) * tw + (float)u->center_coord[0] * tw;
        a.gy0 = (float)(-(int)u->map_half_wh[1]) * tw + (float)u->center_coord[1] * tw;
    } else {                                  // proxy.rs:136-163 + proxy.wgsl:66-68
        const int g = c->proxy_grid_dim;
        a.nx = a.ny = g; a.cs = u->width_scale;
        a.gx0 = (float)(-(g / 2)) * u->width_scale + floorf((float)u->center_coord[0] * tw / u->width_scale) * u->width_scale;
        a.gy0 = (float)(-(g / 2)) * u->width_scale + floorf((float)u->center_coord[1] * tw / u->width_scale) * u->width_scale;
    }
    a.hm_w = c->hm_w; a.hm_h = c->hm_h; a.tex_size = c->proxy_size > 0 ? c->proxy_size : 1; a.n_mips = c->proxy_mips > 0 ? c->proxy_mips : 1;
    memcpy(a.mip_off, c->proxy_mip_off, sizeof(a.mip_off));
    a.width = width; a.height = height;
    a.atm = atmo_constants(c->atm);           // the block in force now: the fog part (the fade does not apply: the proxy is what the splats fade into)
}

// What the proxy passes check in common before anything is launched or written (fn: the entry point the refusal names); GSWT_OK or the
// refusal.  grid: the pass reads the block's grid (the plane passes), so the HeightMap surface needs its map and both cell sizes count.
static int proxy_call_check(gswt_ctx* c, const gswt_proxy_uniforms* u, int width, int height, const float* rgba_dev, const float* depth_dev, bool grid,
                            const char* fn)
{
    if (!u || !rgba_dev || !depth_dev || width <= 0 || height <= 0) return fail(c, GSWT_ERR_BAD_ARG, "%s: bad argument", fn);
    if (c->proxy_size == 0 && !u->black_background) return fail(c, GSWT_ERR_STATE, "%s before gswt_proxy_configure", fn);
    if (!grid) return GSWT_OK;
    if (u->surface_type == 1u && (c->hm_w == 0 || c->hm_h == 0)) return fail(c, GSWT_ERR_STATE, "%s: HeightMap surface without gswt_configure height map", fn);
    if (!(u->tile_width > 0.0f) || (!u->map_proxy && !(u->width_scale > 0.0f)))
        return fail(c, GSWT_ERR_BAD_ARG, "%s: tile_width / width_scale: cell size must be positive", fn);
    return GSWT_OK;
}

// The common end of the proxy passes: the optional depth fill, the launch (sp set: k_proxy_sphere) with the shadow map in force, its status.
static int proxy_draw(gswt_ctx* c, const ProxyArgs& a, const SphereProxyArgs* sp, bool ortho, float* rgba_dev, float* depth_dev, int clear_depth)
{
    hipSetDevice(c->device);
    if (clear_depth) launch_fill_f32(c->stream, depth_dev, (size_t)a.width * a.height, 1.0f);
    const Shadow shd = shadow_version(c, c->shadows.cur);
    const ClipSet clip = clip_ground_subset(c->clip);
    if (sp) launch_proxy_sphere(c->stream, a, *sp, ortho, shd, clip, c->proxy_tex.p, reinterpret_cast<float4*>(rgba_dev), depth_dev);
    else launch_proxy(c->stream, a, ortho, shd, clip, c->hmap.p, c->proxy_tex.p, reinterpret_cast<float4*>(rgba_dev), depth_dev);
    HIP_TRY(c, hipGetLastError());
    return GSWT_OK;
}

// The checks gswt_proxy_render_ortho makes on the block's projection (fn: the entry point the refusal names); GSWT_OK or the refusal.
static int ortho_projection_check(gswt_ctx* c, const gswt_proxy_uniforms* u, const char* fn)
{
    const float* P = u->projection;
    if (!(P[3] == 0.0f && P[7] == 0.0f && P[11] == 0.0f && P[15] == 1.0f))
        return fail(c, GSWT_ERR_BAD_ARG, "%s: projection must be affine, bottom row (0, 0, 0, 1), not (%g, %g, %g, %g)", fn, P[3], P[7], P[11], P[15]);
    for (int k : {1, 2, 4, 6, 8, 9})
        if (!(P[k] == 0.0f)) return fail(c, GSWT_ERR_BAD_ARG, "%s: projection[%d] = %g: not of ortho() form (no shear or rotation)", fn, k, P[k]);
    for (int k : {0, 5, 10})
        if (!std::isfinite(P[k]) || P[k] == 0.0f) return fail(c, GSWT_ERR_BAD_ARG, "%s: projection[%d] = %g: singular projection", fn, k, P[k]);
    for (int k : {12, 13, 14})
        if (!std::isfinite(P[k])) return fail(c, GSWT_ERR_BAD_ARG, "%s: projection[%d] = %g is not finite", fn, k, P[k]);
    return GSWT_OK;
}

// The orthographic pass's host set-up in the frame world - g (g[2] = 0): a.ortho_*, and a.V[12..14] / a.cam moved into that frame.
// The rays run the way depth grows (depth = GP[10] z + GP[14]: along -z of the camera for an ortho() matrix with near < far, sz = -1) and
// start at z0, an eighth of the depth range before the depth-0 plane.  ortho_o = R^-1 ((0, 0, z0) - t) - g, the view's translation becomes
// t + R g, cam_pos becomes cam_pos - g, and the texture coordinate the frame lacks, g / tile_width / 4, is reduced to its fraction (Repeat
// addressing).  Binary64, each rounded once.
static int ortho_frame(gswt_ctx* c, const gswt_proxy_uniforms* u, ProxyArgs& a, const double g[3], const char* fn)
{
    const float* P = u->projection;
    const double g10 = a.GP[10], g14 = a.GP[14];
    const double zn = (0.0 - g14) / g10, zf = (1.0 - g14) / g10;
    const float sz = g10 < 0.0 ? -1.0f : 1.0f;
    const double z0 = zn - (double)sz * 0.125 * std::fabs(zf - zn);
    const float* V = u->view;                 // column-major: R[r][k] = V[4 k + r], t[r] = V[12 + r]
    const double r[3][3] = {{V[0], V[4], V[8]}, {V[1], V[5], V[9]}, {V[2], V[6], V[10]}};
    const double b[3] = {0.0 - V[12], 0.0 - V[13], z0 - V[14]};
    const double co[3][3] = {{r[1][1] * r[2][2] - r[1][2] * r[2][1], r[1][2] * r[2][0] - r[1][0] * r[2][2], r[1][0] * r[2][1] - r[1][1] * r[2][0]},
                             {r[0][2] * r[2][1] - r[0][1] * r[2][2], r[0][0] * r[2][2] - r[0][2] * r[2][0], r[0][1] * r[2][0] - r[0][0] * r[2][1]},
                             {r[0][1] * r[1][2] - r[0][2] * r[1][1], r[0][2] * r[1][0] - r[0][0] * r[1][2], r[0][0] * r[1][1] - r[0][1] * r[1][0]}};
    const double det = r[0][0] * co[0][0] + r[0][1] * co[0][1] + r[0][2] * co[0][2];
    for (int k = 0; k < 3; k++) {             // R^-1 = cofactor^T / det
        const double w = (co[0][k] * b[0] + co[1][k] * b[1] + co[2][k] * b[2]) / det;
        a.ortho_o[k] = (float)(w - g[k]);
        if (!std::isfinite(a.ortho_o[k])) return fail(c, GSWT_ERR_BAD_ARG, "%s: view is singular or not finite", fn);
        a.V[12 + k] = (float)((double)V[12 + k] + (r[k][0] * g[0] + r[k][1] * g[1]));
        a.cam[k] = (float)((double)u->cam_pos[k] - g[k]);
    }
    for (int k = 0; k < 2; k++) {
        const double t = g[k] / (double)u->tile_width / 4.0;
        a.ortho_uv0[k] = (float)(t - std::floor(t));
    }
    a.ortho_t[0] = P[12]; a.ortho_t[1] = P[13];
    a.ortho_d[0] = sz * V[2]; a.ortho_d[1] = sz * V[6]; a.ortho_d[2] = sz * V[10];
    return GSWT_OK;
}

int gswt_proxy_render(gswt_ctx* c, const gswt_proxy_uniforms* u, int width, int height, float* rgba_dev, float* depth_dev, int clear_depth)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    if (int e = proxy_call_check(c, u, width, height, rgba_dev, depth_dev, true, "gswt_proxy_render")) return e;
    if (u->projection[0] == 0.0f || u->projection[5] == 0.0f) return fail(c, GSWT_ERR_BAD_ARG, "gswt_proxy_render: singular projection");
    ProxyArgs a;
    proxy_args(c, u, width, height, a);
    return proxy_draw(c, a, nullptr, false, rgba_dev, depth_dev, clear_depth);
} GSWT_CATCH

// The orthographic form (include/gswt_hip.h, "orthographic proxy pass"): the same block under an affine projection, k_proxy<., ORTHO>, in the
// grid frame g = (gx0, gy0, 0).
int gswt_proxy_render_ortho(gswt_ctx* c, const gswt_proxy_uniforms* u, int width, int height, float* rgba_dev, float* depth_dev, int clear_depth)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    if (int e = proxy_call_check(c, u, width, height, rgba_dev, depth_dev, true, "gswt_proxy_render_ortho")) return e;
    if (int e = ortho_projection_check(c, u, "gswt_proxy_render_ortho")) return e;
    ProxyArgs a;
    proxy_args(c, u, width, height, a);
    const double g[3] = {a.gx0, a.gy0, 0.0};
    if (int e = ortho_frame(c, u, a, g, "gswt_proxy_render_ortho")) return e;
    return proxy_draw(c, a, nullptr, true, rgba_dev, depth_dev, clear_depth);
} GSWT_CATCH

// The ground under the Sphere surface (include/gswt_hip.h, "sphere proxy pass"): k_proxy_sphere, an entry point of its own -- gswt_proxy_render
// and gswt_proxy_render_ortho with surface_type == 2 keep drawing the plane.  The sphere is centred at the world origin, so the orthographic
// set-up runs with g = 0.
int gswt_proxy_render_sphere(gswt_ctx* c, const gswt_proxy_uniforms* u, float sphere_radius, int projection, int width, int height, float* rgba_dev,
                             float* depth_dev, int clear_depth)
try {
    if (!c) return GSWT_ERR_BAD_ARG;
    if (projection != 0 && projection != 1) return fail(c, GSWT_ERR_BAD_ARG, "gswt_proxy_render_sphere: projection %d is neither 0 (perspective) nor 1 (orthographic)", projection);
    if (int e = proxy_call_check(c, u, width, height, rgba_dev, depth_dev, false, "gswt_proxy_render_sphere")) return e;
    if (!(u->tile_width > 0.0f) || !std::isfinite(u->tile_width)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_proxy_render_sphere: tile_width must be positive and finite");
    if (!std::isfinite(sphere_radius) || !(sphere_radius > 0.0f)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_proxy_render_sphere: sphere_radius %g must be positive and finite", sphere_radius);
    const float r = sphere_radius + u->height_offset;
    if (!std::isfinite(r) || !(r > 0.0f)) return fail(c, GSWT_ERR_BAD_ARG, "gswt_proxy_render_sphere: sphere_radius + height_offset = %g must be positive and finite", r);
    if (u->map_half_wh[0] == 0u) return fail(c, GSWT_ERR_BAD_ARG, "gswt_proxy_render_sphere: map_half_wh[0] is 0: the unfolding has no width");
    if (projection == 0) {
        if (u->projection[0] == 0.0f || u->projection[5] == 0.0f) return fail(c, GSWT_ERR_BAD_ARG, "gswt_proxy_render_sphere: singular projection");
    } else if (int e = ortho_projection_check(c, u, "gswt_proxy_render_sphere")) return e;
    // the block with the grid the pass never reads pinned to the map grid (no division by width_scale, whatever the caller left there)
    gswt_proxy_uniforms v = *u;
    v.map_proxy = 1u;
    ProxyArgs a;
    proxy_args(c, &v, width, height, a);
    if (projection == 1) {
        const double g[3] = {0.0, 0.0, 0.0};
        if (int e = ortho_frame(c, u, a, g, "gswt_proxy_render_sphere")) return e;
    }
    const float PI = 3.14159265358979323846f;
    SphereProxyArgs sp;
    sp.r = r; sp.sphere_radius = sphere_radius;
    sp.block_w = (2.0f * (float)u->map_half_wh[0] * u->tile_width) / 5.0f;
    sp.org[0] = (float)((long)u->center_coord[0] - (long)u->map_half_wh[0]) * u->tile_width;
    sp.org[1] = (float)((long)u->center_coord[1] - (long)u->map_half_wh[1]) * u->tile_width;
    sp.lod_k = ((float)u->map_half_wh[0] * (float)a.tex_size) / ((4.0f * PI) * r);
    return proxy_draw(c, a, &sp, projection == 1, rgba_dev, depth_dev, clear_depth);
} GSWT_CATCH

}  // extern "C"
