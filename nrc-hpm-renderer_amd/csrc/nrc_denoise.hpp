// nrc_denoise.hpp -- the edge-avoiding a-trous filter guided by the view AOV (include/nrc_hpm.h, "Denoise").  Device-free: plain C++17 over
// nrc_math.h, the per-pixel rule host + device (NRC_HD).  k_denoise_pass (nrc_integrator.hip) and the host restatements (nrc_test_denoise_host,
// tests/cpp/denoise_main.cpp under the sanitizers) run THIS code, so the fp32 arithmetic is stated once.
//
// Pass p = 0 .. passes - 1 has stride s = 1 << p, reads c_p (c_0: the caller's colour) and writes c_{p+1}; the guide {alpha, z_front} is the
// same in every pass.  A pixel with alpha == 0, or with a non-finite R, G or B, is copied bit for bit; every other pixel is the normalised
// sum of its 5 x 5 taps at distance s -- rows j = -2 .. 2 outside, columns i = -2 .. 2 inside -- with the weight
//     k = h[i + 2] h[j + 2],  h = {1, 4, 6, 4, 1} / 16                                   (the products are exact)
//     d = |alpha_Q - alpha_P| inv_sa;  d = fma(|z_Q - z_P|, inv_sz, d);  d = fma(|lum_Q - lum_P|, inv_sc, d)
//     wgt = k (1 - nrc_expm1_negf(d))
// over the taps inside the image whose alpha is not 0 and whose R, G and B are finite.  The alpha channel of the colour is never touched.
// The weighted mean is formed AROUND THE CENTRE:
//     acc_c = fma(wgt, c_Q - c_P, acc_c);  acc_w += wgt;  out = c_P + acc_c / acc_w
// which is sum(wgt c_Q) / sum(wgt) in exact arithmetic.  Summing wgt c_Q itself rounds 25 times at the size of the colour, and a constant
// colour over a constant guide came back up to 2 ulp off after one pass and 5 after three; around the centre every difference of a
// constant image is an exact 0 and the colour comes back bit for bit, after any number of passes, and in general the roundings are of the
// size of the local contrast, not of the colour.
// What the contract leaves open is decided here:
//   * inv_sa = 1 / sigma_alpha, inv_sz = 1 / sigma_depth, and the pass's inv_sc = 1 / (sigma_color color_decay^p), the power by p fp32
//     multiplications of sigma_color.  A parameter set is valid only if every one of these inverses is finite (denoise_params_error), so a
//     difference of 0 always gives a term of exactly 0, and sigma = +inf an inverse of exactly 0.
//   * d is not clamped: nrc_expm1_negf returns exactly 1 from d = 17.5 on (the tap then adds fma(0, c, acc) = acc) and 0 for a NaN, so a d
//     that is NaN -- possible only for a guide outside the view AOV's contract (alpha != 0 beside a non-finite z_front: inf - inf, inf * 0)
//     -- counts as d = 0.  The centre tap has d = 0 or NaN either way: wgt = 36 / 256, and the sum of the weights is never 0.
//   * lum is taken from the pass's own input c_p.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "nrc_math.h"

namespace nrc {

constexpr uint32_t kDenoiseMaxPasses = 6;

struct DenoiseParams {
    uint32_t passes;
    float sigma_alpha, sigma_depth, sigma_color, color_decay;
};
NRC_HD inline DenoiseParams denoise_defaults() { return DenoiseParams{3u, 0.1f, 4.0f, __builtin_huge_valf(), 0.5f}; }

// a pass's constants
struct DenoisePass {
    int stride;
    float inv_sa, inv_sz, inv_sc;
};
NRC_HD inline DenoisePass denoise_pass(const DenoiseParams& p, uint32_t pass)
{
    float sc = p.sigma_color;
    for (uint32_t k = 0; k < pass; k++) sc = sc * p.color_decay;
    return DenoisePass{1 << pass, 1.0f / p.sigma_alpha, 1.0f / p.sigma_depth, 1.0f / sc};
}

NRC_HD inline bool denoise_finite(float x) { return (nrc_f2u(x) & 0x7f800000u) != 0x7f800000u; }

// null, or why the parameters are refused
inline const char* denoise_params_error(const DenoiseParams& p)
{
    if (p.passes < 1u || p.passes > kDenoiseMaxPasses) return "passes must be 1 .. 6";
    if (!(p.sigma_alpha > 0.0f) || !(p.sigma_depth > 0.0f) || !(p.sigma_color > 0.0f)) return "every sigma must be > 0 (+inf switches a term off)";
    if (!(p.color_decay > 0.0f) || !(p.color_decay <= 1.0f)) return "color_decay must lie in (0, 1]";
    const DenoisePass last = denoise_pass(p, p.passes - 1u);      // (the smallest colour sigma of the call)
    if (!denoise_finite(last.inv_sa) || !denoise_finite(last.inv_sz) || !denoise_finite(last.inv_sc)) return "a sigma is too small: its inverse is not finite";
    return nullptr;
}

struct DenoiseRgba {
    float r, g, b, a;
};
struct DenoiseGuide {
    float alpha, z_front;
};
NRC_HD inline bool denoise_finite_rgb(const DenoiseRgba& c) { return denoise_finite(c.r) && denoise_finite(c.g) && denoise_finite(c.b); }
NRC_HD inline float denoise_lum(const DenoiseRgba& c) { return nrc_fmaf_(0.114f, c.b, nrc_fmaf_(0.587f, c.g, 0.299f * c.r)); }
// h[i + 2] for i = -2 .. 2
NRC_HD inline float denoise_h(int i) { return i == 0 ? 0.375f : ((i == 1 || i == -1) ? 0.25f : 0.0625f); }

// Pixel (x, y) of c_{p+1}.  Image: colour(x, y) -> DenoiseRgba of c_p, guide(x, y) -> DenoiseGuide; neither is called outside the image,
// and a tap's colour is not read when its alpha is 0.
template <class Image>
NRC_HD inline DenoiseRgba denoise_pixel(const Image& im, const DenoisePass& ps, int w, int h, int x, int y)
{
    const DenoiseRgba cp = im.colour(x, y);
    const DenoiseGuide gp = im.guide(x, y);
    if (gp.alpha == 0.0f || !denoise_finite_rgb(cp)) return cp;
    const float lum_p = denoise_lum(cp);
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f, acc_w = 0.0f;
    for (int j = -2; j <= 2; j++) {
        const int qy = y + j * ps.stride;
        if (qy < 0 || qy >= h) continue;
        for (int i = -2; i <= 2; i++) {
            const int qx = x + i * ps.stride;
            if (qx < 0 || qx >= w) continue;
            const DenoiseGuide gq = im.guide(qx, qy);
            if (gq.alpha == 0.0f) continue;
            const DenoiseRgba cq = im.colour(qx, qy);
            if (!denoise_finite_rgb(cq)) continue;
            const float k = denoise_h(i) * denoise_h(j);
            float d = fabsf(gq.alpha - gp.alpha) * ps.inv_sa;
            d = nrc_fmaf_(fabsf(gq.z_front - gp.z_front), ps.inv_sz, d);
            d = nrc_fmaf_(fabsf(denoise_lum(cq) - lum_p), ps.inv_sc, d);
            const float wgt = k * (1.0f - nrc_expm1_negf(d));
            acc_r = nrc_fmaf_(wgt, cq.r - cp.r, acc_r);
            acc_g = nrc_fmaf_(wgt, cq.g - cp.g, acc_g);
            acc_b = nrc_fmaf_(wgt, cq.b - cp.b, acc_b);
            acc_w += wgt;
        }
    }
    return DenoiseRgba{cp.r + acc_r / acc_w, cp.g + acc_g / acc_w, cp.b + acc_b / acc_w, cp.a};
}

// the largest image side: a tap's coordinate, x + 2 * 32, stays an int
constexpr uint32_t kDenoiseMaxSide = 1u << 30;

// ---- the whole filter on the host: rgba and aov [h][w][4] (the framebuffer's and the view AOV's layouts) -> out [h][w][4]; out must not
// overlap the inputs.  The parameters have been checked (denoise_params_error).
struct DenoiseHostImage {
    const float* rgba;
    const float* aov;
    int w;
    DenoiseRgba colour(int x, int y) const
    {
        const float* c = rgba + ((size_t)y * (size_t)w + (size_t)x) * 4;
        return DenoiseRgba{c[0], c[1], c[2], c[3]};
    }
    DenoiseGuide guide(int x, int y) const
    {
        const float* g = aov + ((size_t)y * (size_t)w + (size_t)x) * 4;
        return DenoiseGuide{g[0], g[2]};
    }
};
inline void denoise_host(const float* rgba, const float* aov, uint32_t w, uint32_t h, const DenoiseParams& p, float* out)
{
    const size_t n = (size_t)w * h * 4;
    std::vector<float> ping(p.passes > 1u ? n : 0), pong(p.passes > 2u ? n : 0);
    const float* src = rgba;
    for (uint32_t pass = 0; pass < p.passes; pass++) {
        float* dst = pass + 1u == p.passes ? out : (pass & 1u ? pong.data() : ping.data());
        const DenoisePass ps = denoise_pass(p, pass);
        const DenoiseHostImage im{src, aov, (int)w};
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) {
                const DenoiseRgba c = denoise_pixel(im, ps, (int)w, (int)h, (int)x, (int)y);
                float* o = dst + ((size_t)y * w + x) * 4;
                o[0] = c.r; o[1] = c.g; o[2] = c.b; o[3] = c.a;
            }
        src = dst;
    }
}

}  // namespace nrc
