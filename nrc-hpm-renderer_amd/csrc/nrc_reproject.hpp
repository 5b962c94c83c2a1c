// nrc_reproject.hpp -- history reuse by reprojection (include/nrc_hpm.h, "Reproject"): the frame accumulated over the views before this one
// is carried into the current view through the view AOV's exact depth, and blended with the current frames by effective frame counts.
// Device-free: plain C++17 over nrc_math.h and nrc_view_aov.hpp, the per-pixel rule host + device (NRC_HD).  k_reproject
// (nrc_integrator.hip) and the host restatements (nrc_test_reproject_host, tests/cpp/reproject_main.cpp under the sanitizers) run THIS code,
// so the fp32 arithmetic is stated once.
//
// Per call (reproject_setup, host, fp64, handed to the kernel by value as ReprojectView): from the HISTORY camera's fp32 inv_proj_view m and
// pos the three vectors of view_aov_camera_ray,
//     A_k = m[k] - pos_k m[3],   B_k = m[4 + k] - pos_k m[7],   C_k = m[12 + k] - pos_k m[15]          (k = 0, 1, 2; in double)
// A history pixel's ray direction is ~ sx A + sy B + C, so with N = [A B C]^-1 (inverted in double, rounded to fp32, row-major N[3 k + j]) a
// world point X has q = N (X - pos_hist) ~ (sx, sy, 1): no 4 x 4 inverse, no second matrix.  A determinant of 0 or a non-finite N is refused.
// Per pixel P = (x, y) of the current view, in fp32, in this order:
//   1. c_P, g_P: the current colour and AOV.  alpha_P == 0, a non-finite R, G or B of c_P, or no history: out = c_P bit for bit, out_n = n_cur.
//   2. z = finite(z_half_P) ? z_half_P : z_front_P                                                   (the representative depth)
//   3. the ray r = view_aov_camera_ray(m_cur, pos_cur, x inv_w, y inv_h), inv_w = 1.0f / w, inv_h = 1.0f / h: k_view_aov's u, v, no half-pixel
//      offset;  X_k = fma(z, rd_k, ro_k)
//   4. D_k = X_k - pos_hist_k;  q_k = fma(N[3k + 2], D_2, fma(N[3k + 1], D_1, N[3k] D_0));  sx = q_0 / q_2, sy = q_1 / q_2;
//      ww = fma(m[7], sy, fma(m[3], sx, m[15])) of the history camera; no history unless q_2 ww > 0 (X lies in front of the history camera);
//      dist = sqrtf(fma(D_2, D_2, fma(D_1, D_1, D_0 D_0)))
//   5. fx = ((sx + 1) 0.5) w, fy = ((sy + 1) 0.5) h;  no history unless -1 <= fx < w and -1 <= fy < h (a NaN fails: no tap could lie inside);
//      x0 = floorf(fx), tx = fx - x0, likewise y0, ty
//   6. the four taps Q = (x0 + i, y0 + j), rows j = 0, 1 outside, columns i = 0, 1 inside; a tap outside the image, with alpha_Q == 0 or with a
//      non-finite R, G or B of the history colour is skipped.  z_Q as in step 2;  b = (i ? tx : 1 - tx) (j ? ty : 1 - ty);
//          d = |alpha_Q - alpha_P| inv_sa;  d = fma(|z_Q - dist|, inv_sz, d);  wgt = b (1 - nrc_expm1_negf(d))
//          acc_c = fma(wgt, c_Q - c_P, acc_c) for R, G, B;  acc_w += wgt;  acc_n = fma(wgt, n_Q, acc_n)
//      The depth term is the disocclusion test: the history pixel must have seen the medium at the distance X has from the history camera.
//      The mean is formed around the centre for nrc_denoise.hpp's reason: every difference of a constant colour is an exact 0.
//   7. acc_w == 0: the pixel passes through.  Otherwise n_h = fminf(acc_n, max_history), a = n_h / (n_h + n_cur),
//      out_c = fma(a, acc_c / acc_w, c_P), out_n = n_h + n_cur, out.a = c_P.a.
// What the contract leaves open is decided here:
//   * inv_sa = 1 / sigma_alpha, inv_sz = 1 / sigma_depth; a parameter set is valid only if both are finite (reproject_params_error), so
//     sigma = +inf gives an inverse, and for a finite difference a term, of exactly 0.
//   * d is not clamped: nrc_expm1_negf is exactly 1 from d = 17.5 on (wgt = 0: the tap adds nothing) and 0 for a NaN, which only a guide
//     outside the view AOV's contract can produce and which so counts as d = 0.
//   * acc_n is NOT normalised by acc_w: the bilinear weights and exp(-d) shrink it, so poorly matched history counts for little without a
//     threshold.  The rule is continuous in (fx, fy): where the tap set changes, the taps that come or go have b = 0.
//   * n_cur > 0 and max_history > 0, so n_h + n_cur > 0: a is never 0 / 0.
#pragma once
#include <cstddef>
#include <cstdint>

#include "nrc_math.h"
#include "nrc_view_aov.hpp"

namespace nrc {

struct ReprojectParams {
    float max_history, sigma_alpha, sigma_depth;
};
NRC_HD inline ReprojectParams reproject_defaults() { return ReprojectParams{64.0f, 0.1f, 4.0f}; }

NRC_HD inline bool reproject_finite(float x) { return (nrc_f2u(x) & 0x7f800000u) != 0x7f800000u; }

// null, or why the parameters are refused
inline const char* reproject_params_error(const ReprojectParams& p)
{
    if (!(p.max_history > 0.0f) || !reproject_finite(p.max_history)) return "max_history must be > 0 and finite";
    if (!(p.sigma_alpha > 0.0f) || !(p.sigma_depth > 0.0f)) return "every sigma must be > 0 (+inf switches a term off)";
    if (!reproject_finite(1.0f / p.sigma_alpha) || !reproject_finite(1.0f / p.sigma_depth)) return "a sigma is too small: its inverse is not finite";
    return nullptr;
}

// the largest image: a pixel index stays a positive int
constexpr uint64_t kReprojectMaxPixels = 0x7fffffffull;

// a call's constants
struct ReprojectView {
    float m[16], pos[3];      // the current camera
    float hpos[3];            // the history camera's position
    float N[9];               // [A B C]^-1 of the history camera, row-major
    float hm3, hm7, hm15;     // the history camera's m[3], m[7], m[15]
    float inv_sa, inv_sz, max_history, n_cur;
    float inv_w, inv_h;
    int has_history;
};

// The call's constants.  hist_m == null: no history (hist_pos is not looked at).  Null, or why the call is refused; the parameters have been
// checked (reproject_params_error).
inline const char* reproject_setup(const float* hist_m, const float* hist_pos, const float* m, const float* pos, uint32_t w, uint32_t h, float n_cur,
                                   const ReprojectParams& p, ReprojectView* v)
{
    if (!(n_cur > 0.0f) || !reproject_finite(n_cur)) return "frames must be > 0 and finite";
    if (w == 0u || h == 0u || (uint64_t)w * h > kReprojectMaxPixels) return "bad image size";
    *v = ReprojectView{};
    for (int k = 0; k < 16; k++) v->m[k] = m[k];
    for (int k = 0; k < 3; k++) v->pos[k] = pos[k];
    v->inv_sa = 1.0f / p.sigma_alpha;
    v->inv_sz = 1.0f / p.sigma_depth;
    v->max_history = p.max_history;
    v->n_cur = n_cur;
    v->inv_w = 1.0f / (float)w;
    v->inv_h = 1.0f / (float)h;
    v->has_history = hist_m != nullptr ? 1 : 0;
    if (hist_m == nullptr) return nullptr;
    double M[3][3];      // M[k][0 .. 2] = A_k, B_k, C_k
    for (int k = 0; k < 3; k++) {
        M[k][0] = (double)hist_m[k] - (double)hist_pos[k] * (double)hist_m[3];
        M[k][1] = (double)hist_m[4 + k] - (double)hist_pos[k] * (double)hist_m[7];
        M[k][2] = (double)hist_m[12 + k] - (double)hist_pos[k] * (double)hist_m[15];
    }
    const double c00 = M[1][1] * M[2][2] - M[1][2] * M[2][1], c01 = M[1][2] * M[2][0] - M[1][0] * M[2][2], c02 = M[1][0] * M[2][1] - M[1][1] * M[2][0];
    const double det = M[0][0] * c00 + M[0][1] * c01 + M[0][2] * c02;
    if (!(det != 0.0) || !(fabs(det) < (double)__builtin_huge_valf())) return "the history camera is singular";
    const double adj[9] = {c00, M[0][2] * M[2][1] - M[0][1] * M[2][2], M[0][1] * M[1][2] - M[0][2] * M[1][1],
                           c01, M[0][0] * M[2][2] - M[0][2] * M[2][0], M[0][2] * M[1][0] - M[0][0] * M[1][2],
                           c02, M[0][1] * M[2][0] - M[0][0] * M[2][1], M[0][0] * M[1][1] - M[0][1] * M[1][0]};
    for (int k = 0; k < 9; k++) {
        v->N[k] = (float)(adj[k] / det);
        if (!reproject_finite(v->N[k])) return "the history camera is singular";
    }
    for (int k = 0; k < 3; k++) v->hpos[k] = hist_pos[k];
    v->hm3 = hist_m[3];
    v->hm7 = hist_m[7];
    v->hm15 = hist_m[15];
    return nullptr;
}

struct ReprojectRgba {
    float r, g, b, a;
};
struct ReprojectGuide {
    float alpha, z_front, z_half;
};
struct ReprojectOut {
    ReprojectRgba c;
    float n;
};
NRC_HD inline bool reproject_finite_rgb(const ReprojectRgba& c) { return reproject_finite(c.r) && reproject_finite(c.g) && reproject_finite(c.b); }
NRC_HD inline float reproject_depth(const ReprojectGuide& g) { return reproject_finite(g.z_half) ? g.z_half : g.z_front; }

// Pixel (x, y) of the output.  Image: colour(x, y), guide(x, y) of the current view; hist_colour(x, y), hist_guide(x, y), hist_count(x, y) of
// the history.  None is called outside the image, the history's none without history, and a tap's colour and count are not read when its
// alpha is 0.
template <class Image>
NRC_HD inline ReprojectOut reproject_pixel(const Image& im, const ReprojectView& v, int w, int h, int x, int y)
{
    const ReprojectRgba cp = im.colour(x, y);
    const ReprojectOut through{cp, v.n_cur};
    if (!v.has_history) return through;
    const ReprojectGuide gp = im.guide(x, y);
    if (gp.alpha == 0.0f || !reproject_finite_rgb(cp)) return through;
    const float z = reproject_depth(gp);
    const AovRay r = view_aov_camera_ray(v.m, v.pos, (float)x * v.inv_w, (float)y * v.inv_h);
    const float D0 = nrc_fmaf_(z, r.rd[0], r.ro[0]) - v.hpos[0];
    const float D1 = nrc_fmaf_(z, r.rd[1], r.ro[1]) - v.hpos[1];
    const float D2 = nrc_fmaf_(z, r.rd[2], r.ro[2]) - v.hpos[2];
    const float q0 = nrc_fmaf_(v.N[2], D2, nrc_fmaf_(v.N[1], D1, v.N[0] * D0));
    const float q1 = nrc_fmaf_(v.N[5], D2, nrc_fmaf_(v.N[4], D1, v.N[3] * D0));
    const float q2 = nrc_fmaf_(v.N[8], D2, nrc_fmaf_(v.N[7], D1, v.N[6] * D0));
    const float sx = q0 / q2, sy = q1 / q2;
    const float ww = nrc_fmaf_(v.hm7, sy, nrc_fmaf_(v.hm3, sx, v.hm15));
    if (!(q2 * ww > 0.0f)) return through;
    const float dist = sqrtf(nrc_fmaf_(D2, D2, nrc_fmaf_(D1, D1, D0 * D0)));
    const float fx = ((sx + 1.0f) * 0.5f) * (float)w, fy = ((sy + 1.0f) * 0.5f) * (float)h;
    if (!(fx >= -1.0f && fx < (float)w && fy >= -1.0f && fy < (float)h)) return through;
    const float fx0 = floorf(fx), fy0 = floorf(fy);
    const float tx = fx - fx0, ty = fy - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f, acc_w = 0.0f, acc_n = 0.0f;
    for (int j = 0; j <= 1; j++) {
        const int qy = y0 + j;
        if (qy < 0 || qy >= h) continue;
        for (int i = 0; i <= 1; i++) {
            const int qx = x0 + i;
            if (qx < 0 || qx >= w) continue;
            const ReprojectGuide gq = im.hist_guide(qx, qy);
            if (gq.alpha == 0.0f) continue;
            const ReprojectRgba cq = im.hist_colour(qx, qy);
            if (!reproject_finite_rgb(cq)) continue;
            const float nq = im.hist_count(qx, qy);
            const float b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
            float d = fabsf(gq.alpha - gp.alpha) * v.inv_sa;
            d = nrc_fmaf_(fabsf(reproject_depth(gq) - dist), v.inv_sz, d);
            const float wgt = b * (1.0f - nrc_expm1_negf(d));
            acc_r = nrc_fmaf_(wgt, cq.r - cp.r, acc_r);
            acc_g = nrc_fmaf_(wgt, cq.g - cp.g, acc_g);
            acc_b = nrc_fmaf_(wgt, cq.b - cp.b, acc_b);
            acc_w += wgt;
            acc_n = nrc_fmaf_(wgt, nq, acc_n);
        }
    }
    if (acc_w == 0.0f) return through;
    const float n_h = fminf(acc_n, v.max_history);
    const float a = n_h / (n_h + v.n_cur);
    return ReprojectOut{ReprojectRgba{nrc_fmaf_(a, acc_r / acc_w, cp.r), nrc_fmaf_(a, acc_g / acc_w, cp.g), nrc_fmaf_(a, acc_b / acc_w, cp.b), cp.a},
                        n_h + v.n_cur};
}

// ---- the whole image on the host: rgba, aov, hist_rgba, hist_aov [h][w][4] (the framebuffer's and the view AOV's layouts), hist_n [h][w]
// -> out [h][w][4], out_n [h][w]; the outputs must not overlap the inputs.  Without history (v.has_history == 0) the history pointers are
// not looked at.
struct ReprojectHostImage {
    const float *rgba, *aov, *hist_rgba, *hist_aov, *hist_n;
    int w;
    static ReprojectRgba rgba_at(const float* p, size_t i) { return ReprojectRgba{p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]}; }
    static ReprojectGuide guide_at(const float* p, size_t i) { return ReprojectGuide{p[4 * i], p[4 * i + 2], p[4 * i + 3]}; }
    size_t at(int x, int y) const { return (size_t)y * (size_t)w + (size_t)x; }
    ReprojectRgba colour(int x, int y) const { return rgba_at(rgba, at(x, y)); }
    ReprojectGuide guide(int x, int y) const { return guide_at(aov, at(x, y)); }
    ReprojectRgba hist_colour(int x, int y) const { return rgba_at(hist_rgba, at(x, y)); }
    ReprojectGuide hist_guide(int x, int y) const { return guide_at(hist_aov, at(x, y)); }
    float hist_count(int x, int y) const { return hist_n[at(x, y)]; }
};
inline void reproject_host(const float* hist_rgba, const float* hist_n, const float* hist_aov, const float* rgba, const float* aov, uint32_t w, uint32_t h,
                           const ReprojectView& v, float* out, float* out_n)
{
    const ReprojectHostImage im{rgba, aov, hist_rgba, hist_aov, hist_n, (int)w};
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const ReprojectOut o = reproject_pixel(im, v, (int)w, (int)h, (int)x, (int)y);
            float* c = out + ((size_t)y * w + x) * 4;
            c[0] = o.c.r; c[1] = o.c.g; c[2] = o.c.b; c[3] = o.c.a;
            out_n[(size_t)y * w + x] = o.n;
        }
}

}  // namespace nrc
