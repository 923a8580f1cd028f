// gswt_math.h -- f32 vector / matrix helpers with cgmath 0.18's operand order.
// One rounding per operator (build with -ffp-contract=off); column-major matrices.
#pragma once
// GSWT_HD: empty for g++ (libgswt_host) and for the host-only files of libgswt_hip; gswt_device_fn.h defines it as __host__ __device__ for
// the kernel files, so the device runs the very same operator sequences.
#ifndef GSWT_HD
#define GSWT_HD
#endif
#include <cmath>
#include <cstdint>
#include <cstring>

namespace gswt_host {

struct V3 {
    float x = 0, y = 0, z = 0;
};
GSWT_HD inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
GSWT_HD inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
GSWT_HD inline V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
GSWT_HD inline V3 operator/(V3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
GSWT_HD inline bool is_zero(V3 a) { return a.x == 0.0f && a.y == 0.0f && a.z == 0.0f; }
GSWT_HD inline float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
GSWT_HD inline float magnitude(V3 a) { return std::sqrt(dot(a, a)); }
GSWT_HD inline float distance2(V3 a, V3 b) { V3 d = b - a; return dot(d, d); }     // MetricSpace: (other - self).magnitude2()
GSWT_HD inline float distance(V3 a, V3 b) { return magnitude(b - a); }
GSWT_HD inline V3 normalize(V3 a) { return a * (1.0f / magnitude(a)); }            // InnerSpace::normalize
GSWT_HD inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

struct M3 {
    float m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // [3*c + r]
    GSWT_HD V3 col(int c) const { return {m[3 * c], m[3 * c + 1], m[3 * c + 2]}; }
    GSWT_HD float at(int c, int r) const { return m[3 * c + r]; }
};
GSWT_HD inline M3 from_cols(V3 a, V3 b, V3 c) { M3 r; r.m[0] = a.x; r.m[1] = a.y; r.m[2] = a.z; r.m[3] = b.x; r.m[4] = b.y; r.m[5] = b.z; r.m[6] = c.x; r.m[7] = c.y; r.m[8] = c.z; return r; }
GSWT_HD inline V3 operator*(const M3& m, V3 v) { return (m.col(0) * v.x + m.col(1) * v.y) + m.col(2) * v.z; }
GSWT_HD inline M3 invert(const M3& m)    // cgmath Matrix3::invert (determinant nonzero assumed by the reference's unwrap)
{
    V3 c0 = m.col(0), c1 = m.col(1), c2 = m.col(2);
    float det = (c0.x * (c1.y * c2.z - c2.y * c1.z) - c1.x * (c0.y * c2.z - c2.y * c0.z)) + c2.x * (c0.y * c1.z - c1.y * c0.z);
    V3 r0 = cross(c1, c2) / det, r1 = cross(c2, c0) / det, r2 = cross(c0, c1) / det;
    M3 o;   // from_cols(r0, r1, r2).transpose()
    o.m[0] = r0.x; o.m[1] = r1.x; o.m[2] = r2.x;
    o.m[3] = r0.y; o.m[4] = r1.y; o.m[5] = r2.y;
    o.m[6] = r0.z; o.m[7] = r1.z; o.m[8] = r2.z;
    return o;
}

struct Quat {
    float s = 0, x = 0, y = 0, z = 0;
};
GSWT_HD inline Quat quat_from_mat3(const M3& m)     // cgmath From<Matrix3> for Quaternion
{
    float trace = (m.at(0, 0) + m.at(1, 1)) + m.at(2, 2);
    const float half = 0.5f;
    Quat q;
    if (trace >= 0.0f) {
        float s = std::sqrt(1.0f + trace);
        q.s = half * s;
        s = half / s;
        q.x = (m.at(1, 2) - m.at(2, 1)) * s;
        q.y = (m.at(2, 0) - m.at(0, 2)) * s;
        q.z = (m.at(0, 1) - m.at(1, 0)) * s;
    } else if (m.at(0, 0) > m.at(1, 1) && m.at(0, 0) > m.at(2, 2)) {
        float s = std::sqrt(((m.at(0, 0) - m.at(1, 1)) - m.at(2, 2)) + 1.0f);
        q.x = half * s;
        s = half / s;
        q.y = (m.at(1, 0) + m.at(0, 1)) * s;
        q.z = (m.at(0, 2) + m.at(2, 0)) * s;
        q.s = (m.at(1, 2) - m.at(2, 1)) * s;
    } else if (m.at(1, 1) > m.at(2, 2)) {
        float s = std::sqrt(((m.at(1, 1) - m.at(0, 0)) - m.at(2, 2)) + 1.0f);
        q.y = half * s;
        s = half / s;
        q.z = (m.at(2, 1) + m.at(1, 2)) * s;
        q.x = (m.at(1, 0) + m.at(0, 1)) * s;
        q.s = (m.at(2, 0) - m.at(0, 2)) * s;
    } else {
        float s = std::sqrt(((m.at(2, 2) - m.at(0, 0)) - m.at(1, 1)) + 1.0f);
        q.z = half * s;
        s = half / s;
        q.x = (m.at(0, 2) + m.at(2, 0)) * s;
        q.y = (m.at(2, 1) + m.at(1, 2)) * s;
        q.s = (m.at(0, 1) - m.at(1, 0)) * s;
    }
    return q;
}
GSWT_HD inline M3 mat3_from_quat(Quat q)            // cgmath From<Quaternion> for Matrix3
{
    float x2 = q.x + q.x, y2 = q.y + q.y, z2 = q.z + q.z;
    float xx2 = x2 * q.x, xy2 = x2 * q.y, xz2 = x2 * q.z;
    float yy2 = y2 * q.y, yz2 = y2 * q.z, zz2 = z2 * q.z;
    float sy2 = y2 * q.s, sz2 = z2 * q.s, sx2 = x2 * q.s;
    M3 r;
    r.m[0] = (1.0f - yy2) - zz2; r.m[1] = xy2 + sz2; r.m[2] = xz2 - sy2;
    r.m[3] = xy2 - sz2; r.m[4] = (1.0f - xx2) - zz2; r.m[5] = yz2 + sx2;
    r.m[6] = xz2 + sy2; r.m[7] = yz2 - sx2; r.m[8] = (1.0f - xx2) - yy2;
    return r;
}

// cgmath Matrix4 * Matrix4 (camera.rs:86-88: out[c][r] = sum_k a[k][r] * b[c][k], left to right) and Matrix4 * (x, y, z, w),
// flat column-major [4*c + r]
GSWT_HD inline void mat4_mul(const float* a, const float* b, float* out)
{
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) {
            float acc = a[r] * b[4 * c];
            for (int k = 1; k < 4; k++) acc = acc + a[4 * k + r] * b[4 * c + k];
            out[4 * c + r] = acc;
        }
}
GSWT_HD inline void mat4_vec(const float* m, const float v[4], float out[4])
{
    for (int r = 0; r < 4; r++) {
        float acc = m[r] * v[0];
        for (int k = 1; k < 4; k++) acc = acc + m[4 * k + r] * v[k];
        out[r] = acc;
    }
}
// cgmath::perspective; cot(fovy/2) evaluated in double and rounded once
GSWT_HD inline void perspective(float fovy_deg, float aspect, float near_, float far_, float* m)
{
    float fovy = fovy_deg * (float)(3.14159265358979323846 / 180.0);
    float f = (float)(1.0 / std::tan((double)fovy / 2.0));
    for (int i = 0; i < 16; i++) m[i] = 0.0f;
    m[0] = f / aspect;
    m[5] = f;
    m[10] = (far_ + near_) / (near_ - far_);
    m[11] = -1.0f;
    m[14] = (2.0f * far_ * near_) / (near_ - far_);
}
// Matrix4::look_at_rh -> look_to_rh(eye, center - eye, up)
GSWT_HD inline void look_at_rh(V3 eye, V3 center, V3 up, float* m)
{
    V3 f = normalize(center - eye);
    V3 s = normalize(cross(f, up));
    V3 u = cross(s, f);
    m[0] = s.x; m[1] = u.x; m[2] = -f.x; m[3] = 0.0f;
    m[4] = s.y; m[5] = u.y; m[6] = -f.y; m[7] = 0.0f;
    m[8] = s.z; m[9] = u.z; m[10] = -f.z; m[11] = 0.0f;
    m[12] = -dot(eye, s); m[13] = -dot(eye, u); m[14] = dot(eye, f); m[15] = 1.0f;
}

// Rust `as i32` / `as u8` on f32: saturating, NaN -> 0
GSWT_HD inline int32_t rust_as_i32(float v)
{
    if (v != v) return 0;
    if (v >= 2147483648.0f) return INT32_MAX;
    if (v <= -2147483648.0f) return INT32_MIN;
    return (int32_t)v;
}
GSWT_HD inline uint8_t rust_as_u8(float v)
{
    if (v != v) return 0;
    if (v <= 0.0f) return 0;
    if (v >= 255.0f) return 255;
    return (uint8_t)v;
}

// ---- scene preparation, shared by libgswt_host (WangTile::preprocess) and libgswt_hip (gswt_upload_scene_rows) ----------------

// half 2.7.1 f16::from_f32 (round to nearest even), utils.rs:66-73
GSWT_HD inline uint32_t float_to_half(float value)
{
    uint32_t x;
    memcpy(&x, &value, 4);
    uint32_t sign = x & 0x80000000u, exp = x & 0x7F800000u, man = x & 0x007FFFFFu;
    if (exp == 0x7F800000u) {
        uint32_t nan_bit = man == 0 ? 0 : 0x0200u;
        return (sign >> 16) | 0x7C00u | nan_bit | (man >> 13);
    }
    uint32_t half_sign = sign >> 16;
    int32_t half_exp = (int32_t)(exp >> 23) - 127 + 15;
    if (half_exp >= 0x1F) return half_sign | 0x7C00u;
    if (half_exp <= 0) {
        if (14 - half_exp > 24) return half_sign;
        man |= 0x00800000u;
        uint32_t shift = (uint32_t)(14 - half_exp);
        uint32_t half_man = man >> shift;
        uint32_t round_bit = 1u << (shift - 1);
        if ((man & round_bit) != 0 && (man & (3 * round_bit - 1)) != 0) half_man += 1;
        return half_sign | half_man;
    }
    uint32_t half_e = (uint32_t)half_exp << 10, half_man = man >> 13;
    const uint32_t round_bit = 0x00001000u;
    if ((man & round_bit) != 0 && (man & (3 * round_bit - 1)) != 0) return (half_sign | half_e | half_man) + 1;
    return half_sign | half_e | half_man;
}

GSWT_HD inline uint32_t pack_half_2x16(float x, float y) { return float_to_half(x) | (float_to_half(y) << 16); }

// halfToFloat of the shader (gswt.wgsl:478-494), its arithmetic: normals as IEEE, subnormals fr * 2^-25 (half of IEEE's), Inf / NaN read
// as 0.  THE definition: the kernels' half_decode (gswt_device_fn.h) is a faster form that equals it on all 65536 bit patterns.
GSWT_HD inline float half_to_float(uint32_t h)
{
    const uint32_t e = (h >> 10) & 0x1Fu, fr = h & 0x3FFu;
    if (e == 31u) return 0.0f;
    const float m = e == 0u ? (float)fr * 2.98023223876953125e-08f : std::ldexp(1.0f + (float)fr / 1024.0f, (int)e - 15);
    return (h & 0x8000u) ? -m : m;
}

// A coordinate the scene's bounds can hold: not NaN and within +-3e38 (an Inf, or a value about to overflow, makes its box infinite)
GSWT_HD inline bool finite_coord(float p) { return !(!(p == p) || p > 3e38f || p < -3e38f); }

// Bound of one texture record's (t: its eight words) projected extent, for the band cull: the sum of the decoded covariance's POSITIVE
// eigenvalues is at most the trace when the decoded matrix is positive semi-definite, otherwise at most (trace + sqrt(3) |S|_F) / 2
// (nuclear norm <= sqrt(3) Frobenius norm).  The decode makes stored covariances indefinite: an overflowed (Inf) diagonal reads as 0
// beside finite off-diagonals (lambda_1 up to several times the trace), a raw row may hold a negative diagonal.
GSWT_HD inline float cov_extent_bound(const uint32_t* t)
{
    const double xx = half_to_float(t[4] & 0xFFFFu), xy = half_to_float(t[4] >> 16), xz = half_to_float(t[5] & 0xFFFFu);
    const double yy = half_to_float(t[5] >> 16), yz = half_to_float(t[6] & 0xFFFFu), zz = half_to_float(t[6] >> 16);
    const double tr_d = xx + yy + zz;
    const bool psd = xx >= 0.0 && yy >= 0.0 && zz >= 0.0 && xx * yy - xy * xy >= 0.0 && xx * zz - xz * xz >= 0.0 &&
                     yy * zz - yz * yz >= 0.0 && xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz) >= 0.0;
    const double fro = std::sqrt(xx * xx + yy * yy + zz * zz + 2.0 * (xy * xy + xz * xz + yz * yz));
    return psd ? (float)tr_d : (float)(0.5 * (tr_d + 1.7320508075688772 * fro) * (1.0 + 1e-6));
}

// One splat of Scene::generate_texture, scene.rs:306-411: 32-byte row -> 8 u32 texture words
GSWT_HD inline void generate_texture_row(const uint8_t* row, uint32_t* t)
{
    float fb[6];
    memcpy(fb, row, 24);
    memcpy(t, row, 12);
    t[3] = 0;
    memcpy(&t[7], row + 24, 4);
    float rot[4];
    for (int k = 0; k < 4; k++) rot[k] = ((float)row[28 + k] / 255.0f) * 2.0f - 1.0f;
    float r[9];
    r[0] = 1.0f - 2.0f * (rot[2] * rot[2] + rot[3] * rot[3]);
    r[1] = 2.0f * (rot[1] * rot[2] + rot[0] * rot[3]);
    r[2] = 2.0f * (rot[1] * rot[3] - rot[0] * rot[2]);
    r[3] = 2.0f * (rot[1] * rot[2] - rot[0] * rot[3]);
    r[4] = 1.0f - 2.0f * (rot[1] * rot[1] + rot[3] * rot[3]);
    r[5] = 2.0f * (rot[2] * rot[3] + rot[0] * rot[1]);
    r[6] = 2.0f * (rot[1] * rot[3] + rot[0] * rot[2]);
    r[7] = 2.0f * (rot[2] * rot[3] - rot[0] * rot[1]);
    r[8] = 1.0f - 2.0f * (rot[1] * rot[1] + rot[2] * rot[2]);
    float m[9];   // r * diag(scale): the products with the zeros of diag() contribute +-0
    for (int c = 0; c < 3; c++)
        for (int rr = 0; rr < 3; rr++) {
            float acc = 0.0f;
            for (int k = 0; k < 3; k++) {
                float sk = (k == c) ? fb[3 + c] : 0.0f;
                float term = r[3 * k + rr] * sk;
                acc = (k == 0) ? term : acc + term;
            }
            m[3 * c + rr] = acc;
        }
    float sg[6];
    sg[0] = m[0] * m[0] + m[3] * m[3] + m[6] * m[6];
    sg[1] = m[0] * m[1] + m[3] * m[4] + m[6] * m[7];
    sg[2] = m[0] * m[2] + m[3] * m[5] + m[6] * m[8];
    sg[3] = m[1] * m[1] + m[4] * m[4] + m[7] * m[7];
    sg[4] = m[1] * m[2] + m[4] * m[5] + m[7] * m[8];
    sg[5] = m[2] * m[2] + m[5] * m[5] + m[8] * m[8];
    t[4] = pack_half_2x16(4.0f * sg[0], 4.0f * sg[1]);
    t[5] = pack_half_2x16(4.0f * sg[2], 4.0f * sg[3]);
    t[6] = pack_half_2x16(4.0f * sg[4], 4.0f * sg[5]);
}

// raw depth of one splat centre for a presort view (Scene::sort_self, scene.rs:537-552)
GSWT_HD inline int32_t raw_depth_of(const float* vp, float x, float y, float z)
{
    return rust_as_i32((vp[2] * x + vp[6] * y + vp[10] * z) * 4096.0f);
}

}  // namespace gswt_host
