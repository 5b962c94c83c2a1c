// nrc_view_aov.hpp -- the view AOV of a camera ray: {alpha, tau, z_front, z_half} (include/nrc_hpm.h, "View AOV"), and the same of any
// ray segment ("Ray AOV": view_aov_walk_range).  Device-free: plain C++17 over nrc_math.h, every function host + device (NRC_HD).
// k_view_aov and k_ray_aov (nrc_integrator.hip) and the host restatements (nrc_test_view_aov_host, nrc_test_ray_aov_host,
// tests/cpp/view_aov_main.cpp and ray_aov_main.cpp under the sanitizers) run THIS code, so the fp32 arithmetic is stated once.
// The deep AOV ("Deep AOV": deep_aov_walk_range, at the end) is the same walk with another sum: k_deep_aov, nrc_test_deep_ray_aov_host and
// tests/cpp/deep_aov_main.cpp run it.
//
// The medium is piecewise constant (get_density samples an R8 grid NEAREST), so the optical depth of a ray is the sum over the voxels
// it crosses of sigma_i * (length inside voxel i).  The arithmetic is arranged so that the result does not depend on HOW a traversal
// gets from one non-empty voxel to the next:
//   * the parameter of voxel plane i of axis a is t_a(i) = fma(i, k_a, c_a), from the plane's INDEX -- never a running sum;
//   * the planes a ray crosses are ordered by (t, axis, index along the ray) -- a strict total order; the ray's state after any of
//     them is a function of that plane alone (per axis: how many of its planes come before), so a traversal may pop the planes one
//     by one (a voxel DDA) or jump to any later plane and COUNT (AovAxis::planes_before) and arrives at the same voxel and the same t;
//   * tau accumulates front to back, tau = fma(sigma_i, t_next - t_cur, tau); a voxel of density 0 adds exactly 0, and so does any
//     run of them that is skipped.
// view_aov_walk<Occ> is the two-level traversal: coarse cells of (1 << shift)^3 voxels against the exact occupancy bits (an empty
// cell is left in one jump), voxel steps inside occupied cells.  With NoOccupancy it is the plain voxel DDA.  Both give the same bits.
#pragma once
#include <cstddef>
#include <cstdint>

#include "nrc_math.h"

namespace nrc {

#define NRC_AOV_INF __builtin_huge_valf()
#define NRC_AOV_LN2 0x1.62e430p-1f

struct ViewAov {
    float alpha, tau, z_front, z_half;
};
NRC_HD inline ViewAov view_aov_empty() { return ViewAov{0.0f, 0.0f, NRC_AOV_INF, NRC_AOV_INF}; }

// the grid a ray walks: dims, world size (the box is centred at the origin), sigma of byte 255, the occupancy table's geometry
struct AovGrid {
    uint32_t nx, ny, nz;
    float size[3];
    float density_factor;
    uint32_t occ_shift, occ_gx, occ_gy;
};

// ---- the camera ray of pixel (u, v): the ray camera_ray of nrc_integrator.hip stands for (mc/render.comp:42-60) -- the fp32 inv_proj_view
// applied to clip (2u - 1, 2v - 1, 0, 1), the camera position subtracted -- without that function's cancellation.  camera_ray forms the
// point w.xyz / w.w, which lies 2 near far / (near + far) in front of the eye, and subtracts the position: at |pos| = 70 the quotient is
// rounded to 4e-6, which is 2e-5 rad of a 0.2-long vector -- nothing to a path tracer, but 1.5e-3 of a voxel plane's distance 70 away.
// Here the direction is  d_k ~ N_k - pos_k N_3  with N = m (sx, sy, 0, 1):
//   d_k w.w = sx (m[k] - pos_k m[3]) + sy (m[4 + k] - pos_k m[7]) + (m[12 + k] - pos_k m[15]),
// every bracket as an unevaluated pair hi + lo (the product exactly by fma, the difference exactly by TwoSum), so the large terms cancel
// before anything is rounded; the common factor 1 / w.w only has to carry its sign.  The result lies within 1e-7 rad of the exact ray of
// the fp32 matrix and position for the fp32 sx, sy (tests/test_view_aov_cpu.py asserts 5e-7 against u, v in fp64), the frames' own
// direction within 3e-5 rad of it.  fma, + and - only: the same bits on host and device.
struct AovRay {
    float ro[3], rd[3];
};
struct AovPair {
    float hi, lo;
};
// a - p * q as a pair: exact up to the rounding of lo
NRC_HD inline AovPair view_aov_diff(float a, float p, float q)
{
    const float ph = p * q, pl = nrc_fmaf_(p, q, -ph);      // p q = ph + pl
    const float s = a - ph, bb = s - a;                      // TwoSum(a, -ph) = s + e
    const float e = (a - (s - bb)) + (-ph - bb);
    return AovPair{s, e - pl};
}
NRC_HD inline AovRay view_aov_camera_ray(const float* m, const float* pos, float u, float v)
{
    const float sx = nrc_fmaf_(u, 2.0f, -1.0f), sy = nrc_fmaf_(v, 2.0f, -1.0f);
    const float ww = nrc_fmaf_(m[7], sy, nrc_fmaf_(m[3], sx, m[15]));
    float d[3];
    for (int k = 0; k < 3; k++) {
        const AovPair A = view_aov_diff(m[k], pos[k], m[3]), B = view_aov_diff(m[4 + k], pos[k], m[7]), C = view_aov_diff(m[12 + k], pos[k], m[15]);
        const float hi = nrc_fmaf_(sx, A.hi, nrc_fmaf_(sy, B.hi, C.hi)), lo = nrc_fmaf_(sx, A.lo, nrc_fmaf_(sy, B.lo, C.lo));
        d[k] = (hi + lo) / ww;
    }
    const float inv = 1.0f / sqrtf(nrc_fmaf_(d[2], d[2], nrc_fmaf_(d[1], d[1], d[0] * d[0])));
    return AovRay{{pos[0], pos[1], pos[2]}, {d[0] * inv, d[1] * inv, d[2] * inv}};
}

// ---- one axis of a ray.  Planes are numbered ALONG the ray, s = 0 .. n (s = 0: the plane the ray enters the slab through), voxels
// likewise, v = 0 .. n - 1 (voxel v lies between planes v and v + 1); index() maps either back to the grid's own numbering.
struct AovAxis {
    float k, c, inv_k;      // t of grid plane i: fma(i, k, c)
    uint32_t n;
    int dir;                // +1 / -1: the ray's direction along the axis; 0: the axis is never crossed (v is the grid's own index)
    NRC_HD float plane_t(uint32_t s) const
    {
        if (dir == 0) return NRC_AOV_INF;
        return nrc_fmaf_((float)(dir > 0 ? s : n - s), k, c);
    }
    NRC_HD uint32_t index(uint32_t v) const { return dir < 0 ? n - 1u - v : v; }
    // how many of the planes s = 0 .. n come before parameter T in the order of the planes: those with t <= T (inclusive) or t < T.
    // t is non-decreasing in s (a rounded affine function of the index), so the count is found from an estimate and settled by
    // evaluating plane_t itself: the estimate's rounding never reaches the result.  dir != 0.
    NRC_HD uint32_t planes_before(float T, bool inclusive) const
    {
        const float pf = (T - c) * inv_k;                           // the grid plane at T, roughly
        float sf = dir > 0 ? pf : (float)n - pf;
        sf = fminf(fmaxf(sf, 0.0f), (float)n);                      // (NaN -> 0: fmaxf returns the other operand)
        uint32_t m = (uint32_t)sf + 1u;                             // 1 .. n + 1
        while (m <= n && (inclusive ? plane_t(m) <= T : plane_t(m) < T)) m++;
        while (m > 0u && !(inclusive ? plane_t(m - 1u) <= T : plane_t(m - 1u) < T)) m--;
        return m;
    }
};

// Axis a of the ray.  false: the ray cannot meet the box because of this axis alone (parallel and outside).  A direction component
// that is 0 -- or so small that the plane parameters are not finite -- is never crossed: the ray stays in the voxel layer of ro.
NRC_HD inline bool view_aov_axis(float ro, float rd, float size, uint32_t n, AovAxis* A)
{
    const float half = size * 0.5f, vs = size / (float)n;
    A->n = n;
    A->k = vs / rd;
    A->c = (-half - ro) / rd;
    A->inv_k = 1.0f / A->k;
    A->dir = rd > 0.0f ? 1 : -1;
    const float span = fabsf(A->k) * (float)n + fabsf(A->c);        // (only its finiteness is used)
    if (rd == 0.0f || !(span < NRC_AOV_INF) || !(fabsf(A->inv_k) < NRC_AOV_INF)) {
        A->dir = 0; A->k = 0.0f; A->c = 0.0f; A->inv_k = 0.0f;
        if (!(fabsf(ro) < half)) return false;
    }
    return true;
}
// the voxel layer of coordinate p on an axis that is never crossed
NRC_HD inline uint32_t view_aov_layer(float p, float size, uint32_t n)
{
    const float f = (p + size * 0.5f) * ((float)n / size);
    const float g = fminf(fmaxf(f, 0.0f), (float)(n - 1u));
    return (uint32_t)g;
}

// the traversals' two sources: Density()(ix, iy, iz) returns the voxel's byte; Occ()(cell index) whether the cell holds a non-zero byte
struct AovVolumeBytes {      // a volume in the caller's address space, index ix + nx * (iy + ny * iz)
    const uint8_t* vol;
    uint32_t nx, ny;
    NRC_HD uint32_t operator()(uint32_t ix, uint32_t iy, uint32_t iz) const { return vol[((size_t)iz * ny + iy) * nx + ix]; }
};
struct AovOccupancyBits {    // the exact occupancy bits (nrc_occupancy.hpp), likewise
    static constexpr bool enabled = true;
    const uint32_t* bits;
    NRC_HD bool operator()(uint32_t cell) const { return ((bits[cell >> 5] >> (cell & 31u)) & 1u) != 0u; }
};
struct NoOccupancy {
    static constexpr bool enabled = false;
    NRC_HD bool operator()(uint32_t) const { return true; }
};

// lowest axis first among equal parameters: the order of the planes
NRC_HD inline int view_aov_first(float tx, float ty, float tz) { return (tx <= ty && tx <= tz) ? 0 : (ty <= tz ? 1 : 2); }

// a voxel step: through the first of the three next planes; returns its parameter
NRC_HD inline float view_aov_step(const AovAxis& X, const AovAxis& Y, const AovAxis& Z, uint32_t* vx, uint32_t* vy, uint32_t* vz)
{
    const float tx = X.plane_t(*vx + 1u), ty = Y.plane_t(*vy + 1u), tz = Z.plane_t(*vz + 1u);
    const int a = view_aov_first(tx, ty, tz);
    *vx += a == 0 ? 1u : 0u;
    *vy += a == 1 ? 1u : 0u;
    *vz += a == 2 ? 1u : 0u;
    return a == 0 ? tx : (a == 1 ? ty : tz);
}

// the front-to-back sum over the segments [ta, tb] of voxels with byte != 0
struct AovSum {
    float tau = 0.0f, z_front = NRC_AOV_INF, z_half = NRC_AOV_INF;
    NRC_HD void add(float density_factor, uint32_t byte, float ta, float tb)
    {
        if (byte == 0u) return;
        const float sigma = density_factor * ((float)byte * (1.0f / 255.0f));      // get_density's value
        const float tau_new = nrc_fmaf_(sigma, tb - ta, tau);
        z_front = fminf(z_front, ta);
        if (tau < NRC_AOV_LN2 && tau_new >= NRC_AOV_LN2) z_half = fminf(ta + (NRC_AOV_LN2 - tau) / sigma, tb);
        tau = tau_new;
    }
    // the same for a voxel whose segment [ta, tb] a range cuts at te <= tb: the optical depth is that of [ta, te]; z_half, where the cut
    // segment reaches ln 2, is formed as on the whole ray -- clamped to the voxel's own far plane, not to te --, so a cut ray's z_half has
    // the whole ray's bits (it may lie beyond te by the rounding of its quotient, never by more).  (add() stays its own statement of the
    // whole segment: a version that wrote it as add_cut(.., tb, tb), and the whole walk as a wrapper, cost k_view_aov a register.)
    NRC_HD void add_cut(float density_factor, uint32_t byte, float ta, float tb, float te)
    {
        if (byte == 0u) return;
        const float sigma = density_factor * ((float)byte * (1.0f / 255.0f));      // get_density's value
        const float tau_new = nrc_fmaf_(sigma, te - ta, tau);
        z_front = fminf(z_front, ta);
        if (tau < NRC_AOV_LN2 && tau_new >= NRC_AOV_LN2) z_half = fminf(ta + (NRC_AOV_LN2 - tau) / sigma, tb);
        tau = tau_new;
    }
};
constexpr uint32_t kAovRound = 4;

// Ranged (view_aov_walk_range below, which states the rules): the part of the ray with max(t_min, 0) <= t <= t_max; otherwise the whole
// ray, t in [max(box entry, 0), box exit], and t_min, t_max are not looked at -- every line the range adds is behind `if constexpr
// (Ranged)`, so the whole-ray walk is the code it was.
// Policy: what is made of the segments.  policy.sum() is the walk's sum, made where the walk starts summing -- add / add_cut as AovSum has
// them, and its tau, z_front, z_half.  The default, AovFlat, makes AovSum itself, so the view and ray AOV's instantiations are the code
// they were (the deep AOV's policy: AovDeep below).
struct AovFlat {
    using Sum = AovSum;
    NRC_HD AovSum sum() const { return AovSum(); }
};
template <class Density, class Occ, bool Ranged = false, class Policy = AovFlat>
NRC_HD inline ViewAov view_aov_walk(const AovGrid& g, const AovRay& r, const Density& density, const Occ& occupied, float t_min = 0.0f,
                                    float t_max = NRC_AOV_INF, const Policy& policy = Policy())
{
    float t_from = 0.0f;
    if constexpr (Ranged) {
        // (every comparison is false for a NaN: one in any of the eight numbers ends here, and so does an infinite origin or direction)
        const bool finite = fabsf(r.ro[0]) < NRC_AOV_INF && fabsf(r.ro[1]) < NRC_AOV_INF && fabsf(r.ro[2]) < NRC_AOV_INF &&
                            fabsf(r.rd[0]) < NRC_AOV_INF && fabsf(r.rd[1]) < NRC_AOV_INF && fabsf(r.rd[2]) < NRC_AOV_INF;
        t_from = fmaxf(t_min, 0.0f);
        if (!finite || !(t_min == t_min) || !(t_from < t_max)) return view_aov_empty();
    }
    AovAxis X, Y, Z;
    const bool hx = view_aov_axis(r.ro[0], r.rd[0], g.size[0], g.nx, &X);
    const bool hy = view_aov_axis(r.ro[1], r.rd[1], g.size[1], g.ny, &Y);
    const bool hz = view_aov_axis(r.ro[2], r.rd[2], g.size[2], g.nz, &Z);
    if (!(hx && hy && hz)) return view_aov_empty();
    // slab test: plane_t is +inf on an axis that is never crossed, which leaves t1 alone; its entry is "always inside"
    const float ex = X.dir ? X.plane_t(0) : 0.0f, ey = Y.dir ? Y.plane_t(0) : 0.0f, ez = Z.dir ? Z.plane_t(0) : 0.0f;
    const float t0 = fmaxf(fmaxf(ex, ey), fmaxf(ez, Ranged ? t_from : 0.0f)) + 0.0f;      // (+ 0: never -0, whichever zero a maximum of two returns)
    const float t1 = fminf(fminf(X.plane_t(X.n), Y.plane_t(Y.n)), Z.plane_t(Z.n));
    if (!(t0 < t1) || !(t1 < NRC_AOV_INF)) return view_aov_empty();      // (t1 = +inf: no axis is crossed -- not a ray)
    if constexpr (Ranged) {
        if (!(t0 < t_max)) return view_aov_empty();      // the range ends in front of the box
    }
    // the state at t0: every plane with t <= t0 is behind the ray.  (At least plane 0 of every crossed axis is, and plane n is not:
    // t(n) >= t1 > t0 -- the clamps never act, they are what keeps a voxel index inside the grid whatever the arithmetic does.)
    uint32_t vx = X.dir ? X.planes_before(t0, true) : view_aov_layer(r.ro[0], g.size[0], g.nx) + 1u;
    uint32_t vy = Y.dir ? Y.planes_before(t0, true) : view_aov_layer(r.ro[1], g.size[1], g.ny) + 1u;
    uint32_t vz = Z.dir ? Z.planes_before(t0, true) : view_aov_layer(r.ro[2], g.size[2], g.nz) + 1u;
    vx = (vx < 1u ? 1u : (vx > X.n ? X.n : vx)) - 1u;
    vy = (vy < 1u ? 1u : (vy > Y.n ? Y.n : vy)) - 1u;
    vz = (vz < 1u ? 1u : (vz > Z.n ? Z.n : vz)) - 1u;
    typename Policy::Sum sum = policy.sum();
    float t_cur = t0;
    const uint32_t sh = g.occ_shift;
    // Every trip crosses at least one plane: at most nx + ny + nz trips.  They are made in rounds of kAovRound: the first trip of a round is
    // whatever the voxel asks for -- a step, or the jump out of an empty cell --, the others are voxel steps for as long as the ray stays in
    // occupied cells, and the round's segments are summed, in order, only after its last trip: the bytes of a round (up to kAovRound
    // look-ups per ray, where the medium is dense) are in flight together instead of one behind the other.  The order of the sum is the
    // order of the trips, so the rounds change no bit.
    uint32_t trips = g.nx + g.ny + g.nz;
    bool done = false;
    while (!done) {
        uint32_t byte[kAovRound];
        float ta[kAovRound], tb[kAovRound];
        {
            const uint32_t ix = X.index(vx), iy = Y.index(vy), iz = Z.index(vz);
            bool occ = true;
            if constexpr (Occ::enabled) occ = occupied(((iz >> sh) * g.occ_gy + (iy >> sh)) * g.occ_gx + (ix >> sh));
            float t_next;
            byte[0] = 0u;
            if (occ) {
                byte[0] = density(ix, iy, iz);
                t_next = view_aov_step(X, Y, Z, &vx, &vy, &vz);
            } else {
                // an empty cell: to the first of the three planes that bound it, and the other axes to where the voxel steps would
                // have left them there -- the planes in front of (T, a) in the order: t <= T on a lower axis, t < T on a higher one
                uint32_t sx = X.dir > 0 ? (((ix >> sh) + 1u) << sh) : (X.dir < 0 ? X.n - ((ix >> sh) << sh) : 0u);
                uint32_t sy = Y.dir > 0 ? (((iy >> sh) + 1u) << sh) : (Y.dir < 0 ? Y.n - ((iy >> sh) << sh) : 0u);
                uint32_t sz = Z.dir > 0 ? (((iz >> sh) + 1u) << sh) : (Z.dir < 0 ? Z.n - ((iz >> sh) << sh) : 0u);
                sx = sx > X.n ? X.n : sx;
                sy = sy > Y.n ? Y.n : sy;
                sz = sz > Z.n ? Z.n : sz;
                const float tx = X.plane_t(sx), ty = Y.plane_t(sy), tz = Z.plane_t(sz);
                const int a = view_aov_first(tx, ty, tz);
                t_next = a == 0 ? tx : (a == 1 ? ty : tz);
                uint32_t nx_ = sx, ny_ = sy, nz_ = sz;
                if (a != 0 && X.dir) nx_ = X.planes_before(t_next, true) - 1u;                  // (x is the lowest axis: always "t <= T")
                if (a != 1 && Y.dir) ny_ = Y.planes_before(t_next, a == 2) - 1u;
                if (a != 2 && Z.dir) nz_ = Z.planes_before(t_next, false) - 1u;                 // (z is the highest: always "t < T")
                // (never backwards and never past the cell's own bounding plane: true of the exact counts, kept true whatever they return)
                vx = X.dir ? (nx_ < vx ? vx : (a != 0 && nx_ >= sx ? sx - 1u : nx_)) : vx;
                vy = Y.dir ? (ny_ < vy ? vy : (a != 1 && ny_ >= sy ? sy - 1u : ny_)) : vy;
                vz = Z.dir ? (nz_ < vz ? vz : (a != 2 && nz_ >= sz ? sz - 1u : nz_)) : vz;
            }
            ta[0] = t_cur;
            tb[0] = t_next;
            t_cur = t_next;
            done = vx >= X.n || vy >= Y.n || vz >= Z.n || --trips == 0u;      // through the box's exit plane
            if constexpr (Ranged) done = done || !(t_next < t_max);             // ... or the range's end: the trip's far plane is at or beyond it
        }
#if defined(__clang__)
#pragma unroll
#endif
        for (uint32_t k = 1; k < kAovRound; k++) {
            byte[k] = 0u;
            ta[k] = tb[k] = t_cur;
            bool go = !done;
            uint32_t ix = 0u, iy = 0u, iz = 0u;
            if (go) {
                ix = X.index(vx); iy = Y.index(vy); iz = Z.index(vz);
                if constexpr (Occ::enabled) go = occupied(((iz >> sh) * g.occ_gy + (iy >> sh)) * g.occ_gx + (ix >> sh));
            }
            if (go) {
                byte[k] = density(ix, iy, iz);
                t_cur = tb[k] = view_aov_step(X, Y, Z, &vx, &vy, &vz);
                done = vx >= X.n || vy >= Y.n || vz >= Z.n || --trips == 0u;
                if constexpr (Ranged) done = done || !(t_cur < t_max);
            }
        }
#if defined(__clang__)
#pragma unroll
#endif
        for (uint32_t k = 0; k < kAovRound; k++) {
            if constexpr (Ranged) sum.add_cut(g.density_factor, byte[k], ta[k], tb[k], fminf(tb[k], t_max));
            else sum.add(g.density_factor, byte[k], ta[k], tb[k]);
        }
    }
    const float tau = sum.tau, z_front = sum.z_front, z_half = sum.z_half;
    if (!(tau > 0.0f)) return view_aov_empty();      // (a ray that only grazes non-empty voxels along zero-length segments saw nothing)
    return ViewAov{nrc_expm1_negf(tau), tau, z_front, z_half};
}

// ---- a ray segment (include/nrc_hpm.h, "Ray AOV"): {alpha, tau, z_front, z_half} over the part of the ray ro + t rd with
// max(t_min, 0) <= t <= t_max.  rd is used as given: t is the ray parameter and the optical depth is integrated against it -- with
// |rd| = 1, t is distance and tau the optical depth the renderers mean.
//   start   t0 = max(box entry, t_min, 0) + 0; the state at t0 is the whole walk's rule (every plane with t <= t0 is behind the ray:
//           planes_before(t0, true)), so where t0 falls inside a non-empty voxel z_front is exactly t0.
//   end     min(box exit, t_max): a voxel's segment [ta, tb] counts as [ta, fminf(tb, t_max)], and the walk is done after the first trip
//           whose far plane is at or beyond t_max -- the jump out of an empty cell is such a trip.  A segment of length 0 adds nothing.
//   bits    t_min <= 0 and t_max = +inf: view_aov_walk's bits.  A ray cut at t_max = T keeps the whole ray's z_front, and its z_half
//           wherever the cut ray has one (AovSum::add_cut); tau accumulates identically up to the cut segment.  The plain walk
//           (NoOccupancy) and the walk with jumps agree in every bit for every range: a jump only leaves out segments that add an exact 0.
//   empty   {0, 0, +inf, +inf} for t_max <= max(t_min, 0), a NaN in any of the eight numbers, a zero or non-finite direction, a non-finite
//           origin, and a range that holds no medium.  Never a NaN.
template <class Density, class Occ>
NRC_HD inline ViewAov view_aov_walk_range(const AovGrid& g, const AovRay& r, float t_min, float t_max, const Density& density, const Occ& occupied)
{
    return view_aov_walk<Density, Occ, true>(g, r, density, occupied, t_min, t_max);
}

// ---- the rays of the image-shaped sources, as records {ox, oy, oz, t_min, dx, dy, dz, t_max} (fma, +, - and / only: the same bits on
// host and device).  The camera ray is view_aov_camera_ray's, whole.  An orthographic view is a parallelogram origin + su du + sv dv,
// su = (i + 1/2) / w, sv = (j + 1/2) / h for pixel (i, j) of w x h, every ray with the view's direction as given.
struct AovOrthoView {
    float origin[3], du[3], dv[3], dir[3];
};
NRC_HD inline AovRay ray_aov_ortho_ray(const AovOrthoView& view, uint32_t i, uint32_t j, uint32_t w, uint32_t h)
{
    const float su = ((float)i + 0.5f) / (float)w, sv = ((float)j + 0.5f) / (float)h;
    AovRay r;
    for (int k = 0; k < 3; k++) {
        r.ro[k] = nrc_fmaf_(su, view.du[k], nrc_fmaf_(sv, view.dv[k], view.origin[k]));
        r.rd[k] = view.dir[k];
    }
    return r;
}

// ---- the deep AOV (include/nrc_hpm.h, "Deep AOV"): the ray parameters z[k] at which the accumulated optical depth of a ray segment reaches
// the caller's levels L[0] < L[1] < .. < L[K - 1] (1 <= K <= kAovDeepMaxLevels, finite, L[0] > 0), in the SAME single walk that forms the
// flat {alpha, tau, z_front, z_half}.  z_half is the one-level case and the rule is its rule: in the non-empty voxel whose segment
// [ta, tb], cut at te, takes tau to tau_new = fma(sigma, te - ta, tau),
//     while (next < K && tau_new >= L[next]) { z[next] = fminf(ta + (L[next] - tau) / sigma, tb); next++; }
// tau < L[next] holds on entry (next has moved past every level tau has reached), so for K = 1, L = {NRC_AOV_LN2} the plane is z_half bit
// for bit; several levels may be crossed in one voxel; the clamp is to the voxel's own far plane, as in add_cut.  A crossing is handed to
// the sink, emit(k, z), when it happens -- the sum keeps no depth.  tau never decreases along the walk and the flat result's tau is the
// last tau_new, so level k was emitted exactly when the result's tau >= L[k] (an fp32 compare): the levels never reached are the tail
// behind the last one that compare admits, and they are emitted as +inf after the walk -- for an empty or degenerate record all K.
constexpr uint32_t kAovDeepMaxLevels = 32;
template <class Sink>
struct AovDeepSum {
    const float* levels;
    uint32_t n_levels;
    Sink* sink;
    uint32_t next = 0u;
    float tau = 0.0f, z_front = NRC_AOV_INF, z_half = NRC_AOV_INF;
    NRC_HD void add_cut(float density_factor, uint32_t byte, float ta, float tb, float te)
    {
        if (byte == 0u) return;
        const float sigma = density_factor * ((float)byte * (1.0f / 255.0f));      // get_density's value
        const float tau_new = nrc_fmaf_(sigma, te - ta, tau);
        z_front = fminf(z_front, ta);
        if (tau < NRC_AOV_LN2 && tau_new >= NRC_AOV_LN2) z_half = fminf(ta + (NRC_AOV_LN2 - tau) / sigma, tb);
        while (next < n_levels && tau_new >= levels[next]) {
            sink->emit(next, fminf(ta + (levels[next] - tau) / sigma, tb));
            next++;
        }
        tau = tau_new;
    }
    NRC_HD void add(float density_factor, uint32_t byte, float ta, float tb) { add_cut(density_factor, byte, ta, tb, tb); }
};
template <class Sink>
struct AovDeep {
    using Sum = AovDeepSum<Sink>;
    const float* levels;
    uint32_t n_levels;
    Sink* sink;
    NRC_HD Sum sum() const { return Sum{levels, n_levels, sink}; }
};
// the range walk's record and rules (above), its flat result with the same bits, and the K depths through sink.emit(k, z): every k once
template <class Density, class Occ, class Sink>
NRC_HD inline ViewAov deep_aov_walk_range(const AovGrid& g, const AovRay& r, float t_min, float t_max, const Density& density, const Occ& occupied,
                                          const float* levels, uint32_t n_levels, Sink* sink)
{
    const ViewAov a = view_aov_walk<Density, Occ, true, AovDeep<Sink>>(g, r, density, occupied, t_min, t_max, AovDeep<Sink>{levels, n_levels, sink});
    uint32_t k = 0u;
    while (k < n_levels && a.tau >= levels[k]) k++;
    for (; k < n_levels; k++) sink->emit(k, NRC_AOV_INF);
    return a;
}
// the host sink: plane k of the ray into z[k * stride]
struct AovDeepArray {
    float* z;
    size_t stride;
    NRC_HD void emit(uint32_t k, float v) { z[(size_t)k * stride] = v; }
};
// the levels' rule, for every entry point: NULL when they are in order, otherwise what is wrong with them
inline const char* deep_aov_levels_error(uint32_t n_levels, const float* levels)
{
    if (n_levels == 0u || n_levels > kAovDeepMaxLevels) return "the number of levels must be 1 .. 32";
    if (levels == nullptr) return "levels is NULL";
    for (uint32_t k = 0; k < n_levels; k++) {
        if (!(fabsf(levels[k]) < NRC_AOV_INF)) return "every level must be finite";
        if (!(levels[k] > 0.0f)) return "every level must be positive";
        if (k > 0u && !(levels[k] > levels[k - 1u])) return "the levels must be strictly ascending";
    }
    return nullptr;
}

}  // namespace nrc
