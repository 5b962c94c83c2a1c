// nrc_integrator.hip -- headless HIP path integrator for gfx950: one lane per pixel path, density grid as R8 in HBM
// (served from L2 / Infinity Cache), HDR framebuffer out.  Compiled with -ffp-contract=off and with every fused
// multiply-add written explicitly (nrc_fmaf_): together with nrc_math.h this makes every per-pixel branch decision
// reproducible against the CPU oracle.
//
// Restates (paths relative to the reference checkout):
//   data/shader/include/random.glsl      hash RNG                         -> Rng
//   data/shader/include/volume.glsl      box SDF, entry/exit, density     -> sky_sdf, find_entry_exit, get_density
//   data/shader/include/dir_gen.glsl     HG phase + direction sampling    -> hg_phase, new_ray_dir
//   data/shader/include/path_trace.glsl  ratio/delta tracking, lights     -> ratio_track, delta_track, trace_scene
//   data/shader/nrc/gen_rays.comp + prep_infer_rays.comp (fused)          -> k_gen_rays
//   data/shader/mc/render.comp                                            -> k_mc_render
//   data/shader/nrc/clear.comp + prep_train_rays.comp                     -> k_train_scan + k_prep_train
//   data/shader/nrc/render.comp                                           -> k_composite
//   data/shader/ref/{cmp1,norm,cmp2}.comp                                 -> k_compare_*
#include "nrc_integrator.hpp"

#include <cstdlib>
#include <string>

#include "nrc_denoise.hpp"
#include "nrc_math.h"
#include "nrc_reproject.hpp"
#include "nrc_view_aov.hpp"
#include "nrc_volume_keys.hpp"

// waves per SIMD the camera kernels are register-allocated for
#ifndef NRC_CAMERA_WAVES_PER_SIMD
#define NRC_CAMERA_WAVES_PER_SIMD 5
#endif

namespace nrc {
namespace {

struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 mul(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 neg(V3 a) { return v3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return nrc_fmaf_(a.z, b.z, nrc_fmaf_(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ float length(V3 a) { return sqrtf(dot(a, a)); }
__device__ __forceinline__ V3 normalize(V3 a)
{
    float inv = 1.0f / length(a);
    return v3(a.x * inv, a.y * inv, a.z * inv);
}
// b ? x : y per component (a ternary on the struct makes hipcc select between two stack copies)
__device__ __forceinline__ V3 sel(bool b, V3 x, V3 y) { return v3(b ? x.x : y.x, b ? x.y : y.y, b ? x.z : y.z); }
__device__ __forceinline__ V3 madd(V3 d, float t, V3 o) { return v3(nrc_fmaf_(d.x, t, o.x), nrc_fmaf_(d.y, t, o.y), nrc_fmaf_(d.z, t, o.z)); }   // o + d*t

// ---- include/random.glsl:24-70
// (hash1, float_construct: nrc_hot_tiles.hpp)
__device__ __forceinline__ float random1(float x) { return float_construct(hash1(nrc_f2u(x))); }
__device__ __forceinline__ float random2(float x, float y) { return float_construct(hash1(nrc_f2u(x) ^ hash1(nrc_f2u(y)))); }
__device__ __forceinline__ float random4(const float* v)
{
    return float_construct(hash1(nrc_f2u(v[0]) ^ hash1(nrc_f2u(v[1])) ^ hash1(nrc_f2u(v[2])) ^ hash1(nrc_f2u(v[3]))));
}

// two fp32 lanes per VGPR pair: v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 perform the same IEEE operation on each half,
// so the packed forms below are bit-identical to their scalar statements (nrc_math.h) at half the VALU issue cost
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 splat(float x) { return f2{x, x}; }
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

// ---- the free-flight log (nrc_math.h: nrc_logf).  Its 128-bin table lives in LDS: one instance per kernel that uses it (a file-scope
// __shared__ object), filled by every wave for itself -- identical values to identical addresses, no workgroup barrier, like
// load_occupancy_per_wave -- from the constant copy in device memory.
__device__ const NrcLogBin g_log_tab[128] = {
#include "nrc_log_table.inc"
};
__shared__ NrcLogBin s_log_tab[128];
__device__ __forceinline__ void fill_log_table()
{
    const uint4* src = reinterpret_cast<const uint4*>(g_log_tab);
    uint4* dst = reinterpret_cast<uint4*>(s_log_tab);
    dst[threadIdx.x & 63u] = src[threadIdx.x & 63u];      // 64 lanes x 16 bytes = the 1 KB table
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// nrc_logf on two arguments: the table reads and the integer part per argument, the arithmetic packed (bit-identical, see above)
__device__ __forceinline__ f2 logf2(f2 x)
{
    const uint32_t i0 = nrc_f2u(x.x), i1 = nrc_f2u(x.y);
    const f2 fe = f2{(float)__builtin_amdgcn_frexp_expf(x.x), (float)__builtin_amdgcn_frexp_expf(x.y)};     // == ((i >> 23) & 255) - 126 for normal x
    const f2 m = f2{__builtin_amdgcn_frexp_mantf(x.x), __builtin_amdgcn_frexp_mantf(x.y)};                 // == (i & 0x7fffff) | 0x3f000000
    const f2 t0 = *reinterpret_cast<const f2*>(reinterpret_cast<const char*>(s_log_tab) + ((i0 >> 13) & 0x3f8u));      // {inv_c, log_c}
    const f2 t1 = *reinterpret_cast<const f2*>(reinterpret_cast<const char*>(s_log_tab) + ((i1 >> 13) & 0x3f8u));
    // (the two table entries arrive in two register pairs: the steps that take them are scalar, or each would cost a move to re-pair)
    const f2 r = f2{nrc_fmaf_(m.x, t0.x, -1.0f), nrc_fmaf_(m.y, t1.x, -1.0f)};
    f2 q = fma2(r, splat(NRC_THIRD), splat(-0.5f));
    q = fma2(q, r, splat(1.0f));
    const f2 s = f2{nrc_fmaf_(fe.x, NRC_LN2, t0.y), nrc_fmaf_(fe.y, NRC_LN2, t1.y)};
    return fma2(q, r, s);
}

// correctly rounded sqrt for x == 0 or normal x: v_sqrt_f32 (1 ulp) + the one-ulp fix-up hipcc's own sqrtf lowering uses,
// without its denormal pre-scaling and class test.  Only sky_sdf calls it: its argument is a sum of squares of
// |p| - half_size terms, each 0 or >= half an ulp of a scene-sized coordinate, never denormal.
__device__ __forceinline__ float sqrt_rn_normal(float x)
{
    float y = __builtin_amdgcn_sqrtf(x);
    const float ym = nrc_u2f(nrc_f2u(y) - 1u), yp = nrc_u2f(nrc_f2u(y) + 1u);
    const float rm = nrc_fmaf_(-ym, y, x), rp = nrc_fmaf_(-yp, y, x);
    y = (rm <= 0.0f) ? ym : y;
    y = (rp > 0.0f) ? yp : y;
    return y;
}

// tools/loop_profile.py builds a second library with -DNRC_LOOP_PROFILE: per loop kind, iterations summed over lanes
// ("useful") and 64 x iterations issued by the wave ("issued"); never defined in the product build
#ifdef NRC_LOOP_PROFILE
// wave-level trips of the tracking loops by the number of walks alive: [0] ratio, 64-lane trips; [1] ratio, pair trips; [2] delta;
// classes 1, 2, 3-4, 5-8, 9-16, 17-32, 33-64
__device__ unsigned long long g_live_hist[3][8];
__device__ unsigned long long g_loop_prof[16];
__device__ unsigned long long g_wave_times[4 * 65536];
#endif
// -DNRC_NO_LOOP_COUNTERS keeps only the per-wave time stamps (the counters slow the kernel several-fold)
#if defined(NRC_LOOP_PROFILE) && !defined(NRC_NO_LOOP_COUNTERS)
#define NRC_PROF(c, k)                                                                    \
    do {                                                                                  \
        (c).useful[k]++;                                                                  \
        const unsigned long long m_ = __ballot(1);                                        \
        if ((int)(threadIdx.x & 63u) == __ffsll((long long)m_) - 1) {                     \
            (c).issued[k] += 64u;                                                         \
            if ((k) == 2 || (k) == 3) {      /* tracking loops: trips issued with <= 32 / <= 16 lanes active (kinds 6, 7) */ \
                if (__popcll(m_) <= 32) (c).issued[6] += 64u;                             \
                if (__popcll(m_) <= 16) (c).issued[7] += 64u;                             \
            }                                                                             \
        }                                                                                 \
    } while (0)
#define NRC_PROF_LIVE(which, mask)                                                           \
    do {                                                                                     \
        const int n_ = __popcll(mask);                                                       \
        if (n_ > 0 && (threadIdx.x & 63u) == 0u) {                                           \
            const int cls_ = n_ <= 1 ? 0 : n_ <= 2 ? 1 : n_ <= 4 ? 2 : n_ <= 8 ? 3 : n_ <= 16 ? 4 : n_ <= 32 ? 5 : 6; \
            atomicAdd(&g_live_hist[which][cls_], 1ull);                                      \
        }                                                                                    \
    } while (0)
#else
#define NRC_PROF(c, k) do { } while (0)
#define NRC_PROF_LIVE(which, mask) do { } while (0)
#endif

// COUNT: the density look-ups are counted (nrc_renderer_count_fetches: a measurement launch); in the product launch the counter,
// its register and its adds do not exist
template <bool COUNT>
struct CtxT {
    const DevScene& sc;
    float rng;              // randomState
    uint32_t fetches;
    uint32_t masked = 0u;   // look-ups the dead-walk rule kept from memory (ratio_track), counted beside `fetches`: the WAVE's sum, uniform
    static constexpr bool counting = COUNT;
    // raw buffer view of the volume: offsets >= the voxel count read 0, which is the sampler's black border
    __amdgpu_buffer_rsrc_t vol = __builtin_amdgcn_make_buffer_rsrc((void*)sc.density, 0, (int)(sc.nx * sc.ny * sc.nz), 0x00020000);
    const uint32_t* occ = nullptr;      // LDS copy of DevScene::occ_bits (load_occupancy), or nullptr
#ifdef NRC_LOOP_PROFILE
    uint32_t useful[8] = {0, 0, 0, 0, 0, 0, 0, 0}, issued[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t fee_kind = 1;
#endif
    __device__ __forceinline__ float rand(float max_val)
    {
        rng = random1(rng);
        return rng * max_val;
    }
    __device__ __forceinline__ void count(uint32_t n)
    {
        if constexpr (COUNT) fetches += n;
    }
    __device__ __forceinline__ void count_masked(uint32_t n)
    {
        if constexpr (COUNT) masked += n;
    }
    // the far cut's proof (delta_track): the camera walk's collisions at or behind the cut, and those of them that met density; the WAVE's sums
    uint32_t cut_n = 0u, cut_met = 0u;
    __device__ __forceinline__ void count_cut(unsigned long long behind, unsigned long long met)
    {
        if constexpr (COUNT) { cut_n += (uint32_t)__popcll(behind); cut_met += (uint32_t)__popcll(behind & met); }
    }
};

// The integrator is bound by the rate at which a CU gets scattered bytes out of the L2 (tools/gather_rate.hip: 2.3 cycles per
// distinct line per CU from L2, 7.6 from the Infinity Cache, against 0.1 from LDS), not by arithmetic.  Most look-ups of a
// shadow or sky ray fall into empty space around the cloud, where the answer is known to be 0: every kernel that samples the
// volume keeps the scene's occupancy bits (<= 8 KB) in LDS, and a look-up whose cell holds no non-zero voxel is answered from
// there -- it goes to the raw buffer with the out-of-range offset, which returns 0 without a memory access.  Exact by
// construction: the bit says that the byte the gather would have fetched is 0.
__device__ __forceinline__ const uint32_t* load_occupancy(const DevScene& sc, uint32_t* s_occ)
{
    fill_log_table();      // (every kernel that walks the volume draws free flights; the __syncthreads below covers it)
    if (sc.occ_bits == nullptr) return nullptr;
    for (uint32_t i = threadIdx.x; i < sc.occ_words; i += blockDim.x) s_occ[i] = sc.occ_bits[i];
    __syncthreads();
    return s_occ;
}
// The same for a kernel whose waves leave the workgroup at different times (k_gen_rays: a wave whose tile misses the medium is
// gone before this point): every wave copies the whole table for itself -- identical values to identical addresses -- and there is
// no workgroup barrier.  occ_words is a multiple of 4 (Scene::build_occupancy_bits).
__device__ __forceinline__ const uint32_t* load_occupancy_per_wave(const DevScene& sc, uint32_t* s_occ)
{
    fill_log_table();
    if (sc.occ_bits == nullptr) return nullptr;
    const uint4* src = reinterpret_cast<const uint4*>(sc.occ_bits);
    uint4* dst = reinterpret_cast<uint4*>(s_occ);
    for (uint32_t i = threadIdx.x & 63u; i < (sc.occ_words >> 2); i += 64u) dst[i] = src[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return s_occ;
}

// wave-uniform 32-bit loads through the scalar cache (the compiler takes the vector path for a pointer it cannot prove unwritten)
__device__ __forceinline__ uint32_t scalar_load(const uint32_t* p)
{
    uint32_t r;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(p) : "memory");
    return r;
}
__device__ __forceinline__ void scalar_load3(const uint32_t* p, const uint32_t* q, const uint32_t* r, uint32_t* a, uint32_t* b, uint32_t* c)
{
    uint32_t r0, r1, r2;
    asm volatile("s_load_dword %0, %3, 0x0\n\ts_load_dword %1, %4, 0x0\n\ts_load_dword %2, %5, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(r0), "=&s"(r1), "=&s"(r2) : "s"(p), "s"(q), "s"(r) : "memory");
    *a = r0;
    *b = r1;
    *c = r2;
}
__device__ __forceinline__ void scalar_load2(const uint32_t* p, const uint32_t* q, uint32_t* a, uint32_t* b)
{
    uint32_t r0, r1;
    asm volatile("s_load_dword %0, %2, 0x0\n\ts_load_dword %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(r0), "=&s"(r1) : "s"(p), "s"(q) : "memory");
    *a = r0;
    *b = r1;
}

template <class C>
__device__ __forceinline__ void init_random(C& c, float u, float v, const float* frame_random)
{
    c.rng = random2(random2(u, v), random4(frame_random));
}

// ---- include/volume.glsl
__device__ __forceinline__ float sky_sdf(const DevScene& s, V3 p)
{
    V3 d = v3(fabsf(p.x) - s.half_size[0], fabsf(p.y) - s.half_size[1], fabsf(p.z) - s.half_size[2]);
    V3 dm = v3(fmaxf(d.x, 0.0f), fmaxf(d.y, 0.0f), fmaxf(d.z, 0.0f));
    return sqrt_rn_normal(dot(dm, dm)) + fminf(fmaxf(d.x, fmaxf(d.y, d.z)), 0.0f);
}

// sky_sdf inside the sphere-trace loops.  When at most one of the three per-axis distances is positive (the point is inside
// the box or in front of one face: med3 <= 0) the box distance is max3 itself -- length((0,0,x)) = sqrt(fl(x*x)) = x under
// correct rounding, and 0 + min(max3,0) = max3 -- so the square root is skipped whenever every active lane of the wave is
// in that case (4 of 5 iterations on the bench view); "+ 0.0f" keeps the -0 -> +0 of the general formula.
__device__ __forceinline__ float sky_sdf_step(const DevScene& s, V3 p)
{
    const float dx = fabsf(p.x) - s.half_size[0], dy = fabsf(p.y) - s.half_size[1], dz = fabsf(p.z) - s.half_size[2];
    const float m3 = fmaxf(dx, fmaxf(dy, dz));
    const bool general = !(__builtin_amdgcn_fmed3f(dx, dy, dz) <= 0.0f);
    if (__ballot(general) == 0ull) return m3 + 0.0f;
    const V3 dm = v3(fmaxf(dx, 0.0f), fmaxf(dy, 0.0f), fmaxf(dz, 0.0f));
    return sqrt_rn_normal(dot(dm, dm)) + fminf(m3, 0.0f);
}

template <class C>
__device__ __forceinline__ void find_entry_exit(C& c, V3 ro, V3 rd, V3* entry, V3* exit_)
{
    const DevScene& s = c.sc;
    float dist;
    do {
        NRC_PROF(c, c.fee_kind);
        dist = sky_sdf_step(s, ro);
        ro = madd(rd, dist, ro);
    } while (dist > 0.125f && dist < 100000.0f);
    *entry = ro;
    ro = madd(rd, s.len2size, ro);
    rd = neg(rd);
    do {
        NRC_PROF(c, c.fee_kind);
        dist = sky_sdf_step(s, ro);
        ro = madd(rd, dist, ro);
    } while (dist > 0.125f && dist < 100000.0f);
    *exit_ = ro;
}

// (z * ny + y) * nx + x on the full-rate 24-bit multiplier (hipcc turns __umul24 of an unbounded operand back into a quarter-rate
// 32-bit multiply); exact when every factor is below 2^24 and the result fits 32 bits -- guaranteed by the size checks at scene
// upload.  The two multiply-adds of an index are ONE asm statement that opens with two wait states: ny and nx are scalar operands,
// the compiler may have just reloaded them from an SGPR spill lane with v_readlane_b32, and a vector instruction that reads an SGPR
// another vector instruction wrote needs two wait states on this target -- which the compiler's hazard recognizer inserts for its
// own instructions but cannot see inside an asm string.
__device__ __forceinline__ uint32_t index24(uint32_t z, uint32_t ny, uint32_t y, uint32_t nx, uint32_t x)
{
    uint32_t r;
    asm("s_nop 1\n\tv_mad_u32_u24 %0, %1, %2, %3\n\tv_mad_u32_u24 %0, %0, %4, %5" : "=&v"(r) : "v"(z), "s"(ny), "v"(y), "s"(nx), "v"(x));
    return r;
}
// Two indices with the same ny, nx (the two collisions of a trip) behind ONE pad: the hazard can only come from an instruction in front of
// the statement -- inside it nothing writes a scalar register, and the pad's two wait states plus every mad issued since only add distance.
__device__ __forceinline__ void index24x2(uint32_t ny, uint32_t nx, uint32_t z0, uint32_t y0, uint32_t x0, uint32_t z1, uint32_t y1, uint32_t x1,
                                          uint32_t* i0, uint32_t* i1)
{
    uint32_t r0, r1;
    asm("s_nop 1\n\tv_mad_u32_u24 %0, %2, %3, %4\n\tv_mad_u32_u24 %1, %7, %3, %8\n\tv_mad_u32_u24 %0, %0, %5, %6\n\tv_mad_u32_u24 %1, %1, %5, %9"
        : "=&v"(r0), "=&v"(r1) : "v"(z0), "s"(ny), "v"(y0), "s"(nx), "v"(x0), "v"(z1), "v"(y1), "v"(x1));
    *i0 = r0;
    *i1 = r1;
}

// volume.glsl:31-39; sampler: R8 UNORM, NEAREST, CLAMP_TO_BORDER black (src/Texture3D.cpp:79-81,221).
// One byte per voxel, fetched with a 32-bit voxel index (24-bit mads); the per-axis border test is branch-free and
// out-of-range lanes read voxel 0 and discard it.
template <class C>
__device__ __forceinline__ float get_density(C& c, V3 p)
{
    const DevScene& s = c.sc;
    float u = nrc_fmaf_(p.x, s.inv_size[0], 0.5f);
    float v = nrc_fmaf_(p.y, s.inv_size[1], 0.5f);
    float w = nrc_fmaf_(p.z, s.inv_size[2], 0.5f);
    float fx = u * s.fnx, fy = v * s.fny, fz = w * s.fnz;
    c.count(1u);
    const bool inb = (fx >= 0.0f) & (fx < s.fnx) & (fy >= 0.0f) & (fy < s.fny) & (fz >= 0.0f) & (fz < s.fnz);
    const uint32_t ix = (uint32_t)fx, iy = (uint32_t)fy, iz = (uint32_t)fz;
    uint32_t idx = index24(iz, s.ny, iy, s.nx, ix);
    idx = inb ? idx : 0u;
    const uint8_t t = s.density[idx];
    const float d = s.density_factor * ((float)t * (1.0f / 255.0f));
    return inb ? d : 0.0f;
}

// Two density look-ups, at start + dir*t1 and start + dir*t2, split into address, load and use so that the tracking loops can
// locate the NEXT pair of collisions while the gathers of the current pair are in flight (software pipelining: the free-flight
// chain does not depend on the fetched densities).  fetch2_addr computes both voxel indices (slots that are masked off or
// outside the volume get offset 2^31: the raw buffer returns the sampler's black border without a memory access), fetch2_load
// issues the two 1-byte gathers, fetch2_density turns the bytes into getDensity()'s value, volume.glsl:31-39.
// `dead`: the lane's walk has a transmittance of exactly 0 (ratio_track): both slots get the border offset whatever they hold.
// n_masked (counting builds): how many slots of the wave `dead` kept from memory, i.e. that the occupancy bits would have sent there
// (a wave-uniform sum: a per-lane counter is a register the counting kernels do not have).
struct Addr2 {
    uint32_t i0, i1;
};
struct Fetch2 {
    uint32_t b0, b1;
};
template <class C>
__device__ __forceinline__ Addr2 fetch2_addr(const C& c, V3 dir, V3 start, float t1, float t2, bool first, bool second, bool dead = false,
                                             uint32_t* n_masked = nullptr)
{
    const DevScene& s = c.sc;
    const f2 t = f2{t1, t2};
    const f2 px = fma2(splat(dir.x), t, splat(start.x));
    const f2 py = fma2(splat(dir.y), t, splat(start.y));
    const f2 pz = fma2(splat(dir.z), t, splat(start.z));
    const f2 u = fma2(px, splat(s.inv_size[0]), splat(0.5f));
    const f2 v = fma2(py, splat(s.inv_size[1]), splat(0.5f));
    const f2 w = fma2(pz, splat(s.inv_size[2]), splat(0.5f));
    const f2 fx = u * splat(s.fnx), fy = v * splat(s.fny), fz = w * splat(s.fnz);
    // 0 <= f < n  <=>  0 <= u < 1 (n >= 1; u*n never rounds up to n; u is never -0)  <=>  bits(u) < bits(1.0f)
    bool in0 = (max(max(nrc_f2u(u.x), nrc_f2u(v.x)), nrc_f2u(w.x)) < 0x3f800000u) & first;
    bool in1 = (max(max(nrc_f2u(u.y), nrc_f2u(v.y)), nrc_f2u(w.y)) < 0x3f800000u) & second;
    const uint32_t x0 = (uint32_t)fx.x, y0 = (uint32_t)fy.x, z0 = (uint32_t)fz.x;
    const uint32_t x1 = (uint32_t)fx.y, y1 = (uint32_t)fy.y, z1 = (uint32_t)fz.y;
    uint32_t idx0, idx1;
    index24x2(s.ny, s.nx, z0, y0, x0, z1, y1, x1, &idx0, &idx1);
    // The LDS occupancy bits are tested behind a wave-uniform test for the table, as in round 3.  Round 4 measured both: without the test
    // k_gen_rays is 1 % faster alone (0.2092 against 0.2117 ms: one branch and four mask merges fewer per trip) and 12 % faster inside the
    // configs[4] frame (0.283 against 0.318 ms) -- and the FRAMES are slower, 7 730 against 7 850 Msamples/s on the default preset and 4 160
    // against 4 810 on configs[4]: a camera kernel that issues more densely leaves the inference / training kernels beside it fewer issue
    // slots (train stage 0.18 -> 0.23 ms, configs[4] train rays 0.53 -> 0.98 ms), and those set the frame rate wherever they are the
    // longer chain.  (tools/ab_config.sh, same box, lib / lib_o0 / lib_m0o0 / round 3's.)  Measured again with the masks and pads of DESIGN.md
    // section 4.4 "Trip overhead" in place: 11 / 8 instructions fewer per delta / ratio trip without the test, two registers fewer -- and the
    // default frame at 9 385-9 413 Msamples/s against 9 467-9 534 with the test (the parent: 9 408-9 427).  The test stays.
    if (c.occ != nullptr) {
        // occupancy bit of the voxel's cell from LDS: an empty cell's byte is 0 without asking memory.  (The table always exists --
        // Scene::build_occupancy_bits.)
        const uint32_t sh = s.occ_shift;
        uint32_t c0, c1;
        index24x2(s.occ_gy, s.occ_gx, z0 >> sh, y0 >> sh, x0 >> sh, z1 >> sh, y1 >> sh, x1 >> sh, &c0, &c1);
        c0 = in0 ? c0 : 0u;
        c1 = in1 ? c1 : 0u;
        in0 &= ((c.occ[c0 >> 5] >> (c0 & 31u)) & 1u) != 0u;
        in1 &= ((c.occ[c1 >> 5] >> (c1 & 31u)) & 1u) != 0u;
    }
    if (n_masked != nullptr) *n_masked = (uint32_t)(__popcll(__ballot(dead & in0)) + __popcll(__ballot(dead & in1)));
    in0 &= !dead;
    in1 &= !dead;
    return Addr2{in0 ? idx0 : 0x80000000u, in1 ? idx1 : 0x80000000u};
}
template <class C>
__device__ __forceinline__ Fetch2 fetch2_load(C& c, const Addr2& a)
{
    Fetch2 f;
    f.b0 = __builtin_amdgcn_raw_buffer_load_b8(c.vol, (int)a.i0, 0, 0);
    f.b1 = __builtin_amdgcn_raw_buffer_load_b8(c.vol, (int)a.i1, 0, 0);
    return f;
}
__device__ __forceinline__ f2 fetch2_density(const DevScene& s, const Fetch2& f)
{
    return splat(s.density_factor) * (f2{(float)f.b0, (float)f.b1} * splat(1.0f / 255.0f));
}

// ---- include/dir_gen.glsl
__device__ __forceinline__ float hg_phase(const DevScene& s, float cos_theta)
{
    float g = s.g;
    float g2 = g * g;
    float x = nrc_fmaf_(-(2.0f * g), cos_theta, 1.0f + g2);
    return (0.5f * (1.0f - g2)) / (x * sqrtf(x));
}

template <bool SECOND = false>
__device__ __forceinline__ V3 rotate(V3 axis, float angle, V3 v)
{
    axis = normalize(axis);
    float s, co;
    nrc_sincosf(angle, &s, &co);
    float oc = 1.0f - co;
    const float ox = oc * axis.x, oy = oc * axis.y, oz = oc * axis.z;
    V3 c0 = v3(nrc_fmaf_(ox, axis.x, co), nrc_fmaf_(ox, axis.y, -(axis.z * s)), nrc_fmaf_(oz, axis.x, axis.y * s));
    V3 c1 = v3(nrc_fmaf_(ox, axis.y, axis.z * s), nrc_fmaf_(oy, axis.y, co), nrc_fmaf_(oy, axis.z, -(axis.x * s)));
    V3 c2 = v3(nrc_fmaf_(oz, axis.x, -(axis.y * s)), nrc_fmaf_(oy, axis.z, axis.x * s), nrc_fmaf_(oz, axis.z, co));
    const V3 r = v3(nrc_fmaf_(c2.x, v.z, nrc_fmaf_(c1.x, v.y, c0.x * v.x)),
                    nrc_fmaf_(c2.y, v.z, nrc_fmaf_(c1.y, v.y, c0.y * v.x)),
                    nrc_fmaf_(c2.z, v.z, nrc_fmaf_(c1.z, v.y, c0.z * v.x)));
    return r;
}

// (The diagnostic builds of DESIGN.md section 7.1 -- -DNRC_DIAG_LASTDIR, -DNRC_DIAG_BISECT=<mask>: code regions of new_ray_dir bracketed with
// s_setprio -- did their work in round 3 and left the product source in round 6; tools/stress_lastdir.sh, bisect_build.sh and
// asm_patch_experiment.sh name the commit that still builds them.)
template <class C>
__device__ __forceinline__ V3 new_ray_dir(C& c, V3 old_dir, bool phase_sampling)
{
    NRC_PROF(c, 4);
    old_dir = normalize(old_dir);
    V3 ortho = old_dir.z < old_dir.x ? v3(old_dir.y, -old_dir.x, 0.0f) : v3(0.0f, -old_dir.z, old_dir.y);
    if (ortho.x == 0.0f && ortho.y == 0.0f && ortho.z == 0.0f) ortho = v3(0.0f, 1.0f, 0.0f);   // robustness
    ortho = normalize(ortho);
    float angle;
    if (phase_sampling) {
        float g = c.sc.g;
        float cos_theta;
        if (fabsf(g) < 0.001f) {
            cos_theta = 1.0f - 2.0f * c.rand(1.0f);
        } else {
            float sqr_term = (1.0f - g * g) / nrc_fmaf_(2.0f * g, c.rand(1.0f), 1.0f - g);
            cos_theta = nrc_fmaf_(-sqr_term, sqr_term, 1.0f + g * g) / (2.0f * g);
        }
        angle = nrc_acosf_clamped(cos_theta);
    } else {
        angle = c.rand(NRC_PI);
    }
    V3 nd = rotate(ortho, angle, old_dir);
    angle = c.rand(NRC_TWO_PI);
    nd = rotate<true>(old_dir, angle, nd);
    nd = normalize(nd);
    return nd;
}

// a per-lane predicate as a wave-uniform 64-bit lane mask and back (why the loops carry masks: see ratio_track)
__device__ __forceinline__ bool lane_bool(unsigned long long m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
__device__ __forceinline__ unsigned long long lane_mask(bool b) { return __builtin_amdgcn_ballot_w64(b); }
// ---- include/path_trace.glsl
// RatioTrack, path_trace.glsl:24-43.  Two collisions per trip: nothing in a step depends on the previous fetch, so both free-
// flight logs share packed math.  The loop is software-pipelined: a trip's two gathers are issued at the top of the loop body,
// the NEXT trip is located (hash chain, logs, positions, voxel indices -- about 80 instructions that do not depend on any
// density) while they are in flight, and only then are the densities used.  A lane that ends on a collision keeps the RNG state
// of that draw, exactly as the one-step loop would; the trip located ahead of it is dropped.
// The two predicates of a located trip leave it as lane masks, formed where the compare is (the compare writes the mask: no instruction).
// Handed on as bools and turned into masks at the bottom of the loop -- another basic block -- each cost a v_cndmask 0/1 and a v_cmp_ne.
// ("Trip overhead": what each of these rewrites took out of a trip, and the ones that were measured and dropped.)
struct RatioTrip {
    float s1, s2, t1, t2;
    unsigned long long live1_m, second_m;       // collision 1 / collision 2 lie inside the segment
};
__device__ __forceinline__ RatioTrip ratio_trip(float rng, float t, float t_max, float inv)
{
    RatioTrip r;
    r.s1 = random1(rng);
    r.s2 = random1(r.s1);
    const f2 l = logf2(f2{1.0f - r.s1, 1.0f - r.s2});
    r.t1 = nrc_fmaf_(-l.x, inv, t);
    r.t2 = nrc_fmaf_(-l.y, inv, r.t1);
    r.live1_m = lane_mask(!(r.t1 >= t_max));
    r.second_m = lane_mask(!(r.t2 >= t_max));
    return r;
}
// The cap of 128 collisions as a lane mask: all ones in the trips that start at collisions 0 .. 124, 0 in the 64th.  An ordinary 64-bit value
// that the loops AND into their masks; written as `last ? 0 : m` at every use, the compiler turns each use into its own compare-and-select
// chain through SCC (twelve scalar instructions in a delta trip).  The empty asm keeps it from folding the mask back into selects.
// (delta_track only: ratio_track's single use costs no more as a select, and a uniform `break` behind the 64th trip made both loops longer.)
__device__ __forceinline__ unsigned long long cap_mask(uint32_t i)
{
    unsigned long long m = (unsigned long long)((long long)((int)i - 126) >> 63);
    asm("" : "+s"(m));
    return m;
}
// ---- thin trips: two lanes per surviving walk ---------------------------------------------------------------------------------
// A tracking loop runs until its last walk ends: the trips issued with at most 32 of the 64 lanes still walking cost 28 % of the
// launch (round 2's cut-tail build, docs/MEASUREMENT_LOG.md).  When a loop is down to 32 walks or fewer they are handed to lane PAIRS (lane p and p + 32, state pushed
// there with ds_permute): an iteration then advances a walk by FOUR collisions -- the hash chain is drawn by both lanes (it is the
// only serial part, a quarter of a trip's instructions), the two free-flight logs, positions, look-ups and transmittance factors
// of collisions 1, 2 are lane p's work and those of 3, 4 lane p + 32's, exchanged with v_permlane32_swap, and the free-flight sums
// and transmittance products are then formed by both lanes in the sequential order -- bit for bit the walk of the one-lane loop.
// (value of the lower-half lane, value of the upper-half lane) of a pair, on both of its lanes
__device__ __forceinline__ void pair_both(float x, float* lo, float* hi)
{
    const auto r = __builtin_amdgcn_permlane32_swap(nrc_f2u(x), nrc_f2u(x), false, false);
    *lo = nrc_u2f(r[0]);
    *hi = nrc_u2f(r[1]);
}

// (Two further tails were built bit-exact, measured and removed -- docs/MEASUREMENT_LOG.md: `ratio_wide`, 32 lanes for each of a wave's last one
// or two ratio walks: the walks it applies to are too few and its registers cost the kernel 0.038 ms; `delta_pairs`, the pair tail for
// delta tracking: 144 B of scratch under the 96-register cap, slower at five waves per SIMD.  Their sources: git history, round 5's tree.)
// the surviving walks of a ratio_track loop, two lanes per walk.  On entry: `alive` lanes have a located trip whose base state is
// (bs, bt) = (chain value before its first draw, free-flight position before it), n collisions done.  On exit: tr / rng of the alive
// lanes are the finished walks' results.
template <class C>
__device__ __forceinline__ void ratio_pairs(C& c, unsigned long long am, bool alive, V3 start, V3 dir, float t_max, float inv, float bs,
                                            float bt, uint32_t n, float& tr, float& rng)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(am >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)am, 0u));
    const uint32_t k = (uint32_t)__popcll(am);
    const bool is_b = (lane & 32u) != 0u;
    // walk state -> lanes rank and rank + 32 (rank = the lane's position among the surviving ones)
    float y[11];
    {
        const float x[11] = {bs, bt, t_max, tr, nrc_u2f(n), start.x, start.y, start.z, dir.x, dir.y, dir.z};
#pragma unroll
        for (int q = 0; q < 11; q++) {
            // every lane pushes (a lane that is masked off neither sends nor receives): the lanes without a walk push to lanes 31 and
            // 63, which are never part of a pair (at most 31 walks survive)
            const int lo = __builtin_amdgcn_ds_permute((int)((alive ? rank : 31u) * 4u), (int)nrc_f2u(x[q]));
            const int hi = __builtin_amdgcn_ds_permute((int)((alive ? rank + 32u : 63u) * 4u), (int)nrc_f2u(x[q]));
            y[q] = nrc_u2f((uint32_t)(is_b ? hi : lo));
        }
    }
    float R0 = y[0], t0 = y[1], T = y[3];
    const float tm = y[2];
    uint32_t nn = nrc_f2u(y[4]);
    const V3 st = v3(y[5], y[6], y[7]), dr = v3(y[8], y[9], y[10]);
    bool act = (lane & 31u) < k;
    float rf = R0;
    unsigned long long deadm = lane_mask(T == 0.0f);      // pairs whose product is exactly 0 and stays so: see ratio_track
    for (;;) {
        const unsigned long long actm = __ballot(act);
        if (actm == 0ull) break;
        NRC_PROF_LIVE(1, actm & 0xffffffffull);
        const float R1 = random1(R0), R2 = random1(R1), R3 = random1(R2), R4 = random1(R3);
        const f2 l = logf2(f2{1.0f - (is_b ? R3 : R1), 1.0f - (is_b ? R4 : R2)});
        float l1, l2, l3, l4;
        pair_both(l.x, &l1, &l3);
        pair_both(l.y, &l2, &l4);
        const float t1 = nrc_fmaf_(-l1, inv, t0), t2 = nrc_fmaf_(-l2, inv, t1), t3 = nrc_fmaf_(-l3, inv, t2), t4 = nrc_fmaf_(-l4, inv, t3);
        // the sequential walk: draw k is made unless 128 collisions are done; the walk ends on a draw that lies beyond the segment
        bool go = act;
        const bool d1 = go & (nn + 1u <= 128u); rf = d1 ? R1 : rf; const bool p1 = d1 & !(t1 >= tm); go = p1;
        const bool d2 = go & (nn + 2u <= 128u); rf = d2 ? R2 : rf; const bool p2 = d2 & !(t2 >= tm); go = p2;
        const bool d3 = go & (nn + 3u <= 128u); rf = d3 ? R3 : rf; const bool p3 = d3 & !(t3 >= tm); go = p3;
        const bool d4 = go & (nn + 4u <= 128u); rf = d4 ? R4 : rf; const bool p4 = d4 & !(t4 >= tm); go = p4;
        // look-ups: collisions 1, 2 on the lower lane, 3, 4 on the upper one
        const bool ma = is_b ? p3 : p1, mb = is_b ? p4 : p2;
        uint32_t n_masked = 0u;
        const Addr2 ad = fetch2_addr(c, dr, st, is_b ? t3 : t1, is_b ? t4 : t2, ma, mb, lane_bool(deadm), C::counting ? &n_masked : nullptr);
        const Fetch2 fa = fetch2_load(c, ad);
        const f2 dens = fetch2_density(c.sc, fa);
        c.count((ma ? 1u : 0u) + (mb ? 1u : 0u));
        c.count_masked(n_masked);
        float f1, f2_, f3, f4;
        pair_both(nrc_fmaf_(-dens.x, inv, 1.0f), &f1, &f3);
        pair_both(nrc_fmaf_(-dens.y, inv, 1.0f), &f2_, &f4);
        T = p1 ? T * f1 : T;
        T = p2 ? T * f2_ : T;
        T = p3 ? T * f3 : T;
        T = p4 ? T * f4 : T;
        deadm = lane_mask(T == 0.0f);
        act = p4 & (nn + 4u < 128u);
        nn += 4u;
        R0 = R4;
        t0 = t4;
    }
    // results back to the walks' own lanes (from the lower lane of their pair)
    const float tr_new = nrc_u2f((uint32_t)__builtin_amdgcn_ds_bpermute((int)(rank * 4u), (int)nrc_f2u(T)));
    const float rng_new = nrc_u2f((uint32_t)__builtin_amdgcn_ds_bpermute((int)(rank * 4u), (int)nrc_f2u(rf)));
    tr = alive ? tr_new : tr;
    rng = alive ? rng_new : rng;
}

// The loop is wave-uniform (it runs while any lane still walks) and its body is predicated with selects instead of per-lane
// branches: with `break`s the compiler sinks the look-ahead into the continue path, i.e. behind the wait for the gathers, and
// the overlap is gone.  Lanes that have finished keep their results and issue no gathers (offset 2^31).
// UNI: the call sits in wave-uniform control flow (every lane of the wave executes it, `valid` says which lanes have a walk), so
// the lanes without a walk can help with the thin trips at the end (ratio_pairs)
// Round 4: the predicates the loop carries from trip to trip (who still walks, whether the located trip's collisions lie inside the
// segment) are 64-bit LANE MASKS in scalar registers, not per-lane bools.  A loop-carried bool is a divergent i1 phi, which the
// compiler merges with three scalar instructions per predicate, per loop header and per exit (s_andn2 / s_and / s_or with exec:
// 30 of them in front of every delta trip) -- and a scalar instruction costs a SIMD as much issue time as a vector one here
// (tools/issue_mix.hip: at five waves per SIMD a v_fma_f32 1.6 clocks, a v_fma_f32 + s_and_b64 pair 3.6).  A uniform mask is an
// ordinary 64-bit value: its phi is a copy.  lane_bool() hands it to v_cndmask as the select mask (no instruction).

// Round 5 measured the next step of that idea and took it out again (commit 4f700df has the code; DESIGN.md section 4 "Lane groups"): every
// surviving walk on a GROUP of L = 2^floor(log2(64 / walks alive)) lanes, chunks of 2 Lc collisions per iteration, the walk's serial
// recurrences (hash chain, free-flight sums, transmittance product) as DPP wave_shr:1 scans along the group (tools/scan_probe.hip,
// tools/dpp_probe.hip).  Bit-exact at the first run of every oracle comparison -- and slower than the pair tail on every preset
// (k_gen_rays alone 0.2111 -> 0.2138 ... 0.2181 ms by entry threshold, frame - 5 %, configs[4] - 4.7 %, Monte-Carlo renderer - 1.5 %).
template <bool UNI = false, class C>
__device__ __forceinline__ float ratio_track(C& c, V3 start, V3 end, bool valid = true)
{
    V3 d = sub(end, start);
    const V3 dir = normalize(d);
    const float t_max = length(d);
    const float inv = c.sc.inv_max_density;
    float tr = 1.0f;
    float rng = c.rng;
    unsigned long long alive_m = lane_mask(valid);
    // Dead walks: only tr leaves the walk, every factor is finite, so a tr of exactly +-0 stays +-0 and what its
    // lane would still fetch is never used.  Such a lane's look-ups get the border offset (one trip late: trip j + 1 is located before
    // trip j is consumed -- a look-up too many, never one too few).  c.count() keeps counting the algorithm's collisions.  (A reduced
    // trip for waves whose walking lanes are all dead -- the chain alone -- was measured and did not move the frame: section 4.4.)
    unsigned long long dead_m = 0ull;
    uint32_t pend = 0u;                        // (counting builds) the wave's masked look-ups of the located trip that would have gone to memory
    RatioTrip a = ratio_trip(rng, 0.0f, t_max, inv);
    unsigned long long live1_m = a.live1_m, second_m = a.second_m;
    Addr2 ia = fetch2_addr(c, dir, start, a.t1, a.t2, lane_bool(a.live1_m), lane_bool(a.live1_m & a.second_m));
    float bs = rng, bt = 0.0f;                 // base of the located trip `a`: chain value and position before its first draw
    for (uint32_t i = 0;; i += 2) {            // i counts collisions: at most 128 (path_trace.glsl:34)
        rng = lane_bool(alive_m & ~live1_m) ? a.s1 : rng;             // collision 1 beyond the segment: the walk ends on this draw
        alive_m &= live1_m;
        if (alive_m == 0ull) break;
        if constexpr (UNI) {
            if (__popcll(alive_m) <= 31) {        // few walks left: two lanes each (ratio_pairs; lanes 31 and 63 stay free as push targets)
                ratio_pairs(c, alive_m, lane_bool(alive_m), start, dir, t_max, inv, bs, bt, i, tr, rng);
                break;
            }
        }
        const bool alive = lane_bool(alive_m);
        if (alive) NRC_PROF(c, 3);
        NRC_PROF_LIVE(0, alive_m);
        const Fetch2 fa = fetch2_load(c, ia);                        // this trip's gathers ...
        __builtin_amdgcn_sched_barrier(0);
        const bool last = i + 2 >= 128;
        const unsigned long long two_m = alive_m & second_m;
        const unsigned long long more_m = last ? 0ull : two_m;
        const RatioTrip b = ratio_trip(a.s2, a.t2, t_max, inv);      // ... fly while the next trip is located
        uint32_t pend_b = 0u;
        const unsigned long long go1_m = more_m & b.live1_m;
        const Addr2 ib = fetch2_addr(c, dir, start, b.t1, b.t2, lane_bool(go1_m), lane_bool(go1_m & b.second_m), lane_bool(dead_m),
                                     C::counting ? &pend_b : nullptr);
        __builtin_amdgcn_sched_barrier(0);
        const f2 dens = fetch2_density(c.sc, fa);
        c.count(alive ? (lane_bool(second_m) ? 2u : 1u) : 0u);
        c.count_masked(pend);
        pend = pend_b;
        tr = alive ? tr * nrc_fmaf_(-dens.x, inv, 1.0f) : tr;
        tr = lane_bool(two_m) ? tr * nrc_fmaf_(-dens.y, inv, 1.0f) : tr;
        dead_m = lane_mask(tr == 0.0f);
        rng = lane_bool(alive_m & ~more_m) ? a.s2 : rng;              // ends after collision 1 / after the 128th collision
        alive_m = more_m;
        live1_m = b.live1_m;
        second_m = b.second_m;
        bs = a.s2;
        bt = a.t2;
        a.s1 = b.s1; a.s2 = b.s2; a.t1 = b.t1; a.t2 = b.t2;
        ia = ib;
    }
    c.rng = rng;
    return tr;
}

template <bool UNI = false, class C>
__device__ __forceinline__ V3 trace_dir_light(C& c, V3 pos, V3 dir, bool valid = true)
{
    const DevScene& s = c.sc;
    if (s.dir_light_strength == 0.0f) return v3(0, 0, 0);
    V3 ld = v3(s.dir_light_dir[0], s.dir_light_dir[1], s.dir_light_dir[2]);
    V3 en, ex;
    if constexpr (UNI) pos = sel(valid, pos, v3(0.0f, 0.0f, 0.0f));
    find_entry_exit(c, pos, neg(normalize(ld)), &en, &ex);
    float tr = ratio_track<UNI>(c, pos, ex, valid);
    float phase = hg_phase(s, dot(ld, neg(dir)));
    float l = (1.0f * tr) * s.dir_light_strength * phase;
    return v3(l, l, l);
}

template <bool UNI = false, class C>
__device__ __forceinline__ V3 trace_point_light(C& c, V3 pos, V3 dir, bool valid = true)
{
    const DevScene& s = c.sc;
    if (s.point_light_strength == 0.0f) return v3(0, 0, 0);
    V3 lp = v3(s.point_light_pos[0], s.point_light_pos[1], s.point_light_pos[2]);
    float tr = ratio_track<UNI>(c, lp, pos, valid);
    float phase = hg_phase(s, dot(normalize(sub(lp, pos)), neg(dir)));
    return v3(((s.point_light_color[0] * s.point_light_strength) * tr) * phase,
              ((s.point_light_color[1] * s.point_light_strength) * tr) * phase,
              ((s.point_light_color[2] * s.point_light_strength) * tr) * phase);
}

__device__ __forceinline__ V3 env_lookup(const DevScene& s, float u, float v)
{
    if (s.env == nullptr || s.env_w == 0) return v3(0, 0, 0);
    float fx = u * (float)s.env_w - 0.5f, fy = v * (float)s.env_h - 0.5f;
    float flx = floorf(fx), fly = floorf(fy);
    float wx = fx - flx, wy = fy - fly;
    int x0 = (int)flx, y0 = (int)fly, x1 = x0 + 1, y1 = y0 + 1;
    int mw = (int)s.env_w - 1, mh = (int)s.env_h - 1;
    x0 = min(max(x0, 0), mw);
    x1 = min(max(x1, 0), mw);
    y0 = min(max(y0, 0), mh);
    y1 = min(max(y1, 0), mh);
    const float* p00 = s.env + 4 * ((size_t)y0 * s.env_w + x0);
    const float* p10 = s.env + 4 * ((size_t)y0 * s.env_w + x1);
    const float* p01 = s.env + 4 * ((size_t)y1 * s.env_w + x0);
    const float* p11 = s.env + 4 * ((size_t)y1 * s.env_w + x1);
    float r[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float a = nrc_fmaf_(wx, p10[k] - p00[k], p00[k]);
        float b = nrc_fmaf_(wx, p11[k] - p01[k], p01[k]);
        r[k] = nrc_fmaf_(wy, b - a, a) * s.env_strength;
    }
    return v3(r[0], r[1], r[2]);
}

__device__ __forceinline__ V3 sample_env_dir(const DevScene& s, V3 dir)
{
    float phi = nrc_atan2f(dir.z, dir.x);
    float theta = nrc_asinf(dir.y);
    return env_lookup(s, nrc_fmaf_(phi, 0.1591f, 0.5f), nrc_fmaf_(theta, 0.3183f, 0.5f));
}

template <bool UNI = false, class C>
__device__ __forceinline__ V3 sample_env(C& c, V3 pos, V3 dir, bool valid = true)
{
    if (c.sc.env_strength == 0.0f) return v3(0, 0, 0);
    V3 rdir = v3(0.0f, 0.0f, 1.0f);
    if constexpr (UNI) {
        if (valid) rdir = new_ray_dir(c, dir, false);      // lanes without a walk draw nothing
        pos = sel(valid, pos, v3(0.0f, 0.0f, 0.0f));
    } else {
        rdir = new_ray_dir(c, dir, false);
    }
    float phase = hg_phase(c.sc, dot(rdir, neg(dir)));
    V3 en, ex;
    find_entry_exit(c, pos, rdir, &en, &ex);
    float tr = ratio_track<UNI>(c, pos, ex, valid);
    V3 e = sample_env_dir(c.sc, rdir);
    return v3((e.x * phase) * tr, (e.y * phase) * tr, (e.z * phase) * tr);
}

template <bool UNI = false, class C>
__device__ __forceinline__ V3 trace_scene(C& c, V3 pos, V3 dir, bool valid = true)
{
    NRC_PROF(c, 5);
    V3 a = trace_dir_light<UNI>(c, pos, dir, valid);
    V3 b = trace_point_light<UNI>(c, pos, dir, valid);
    V3 e = sample_env<UNI>(c, pos, dir, valid);
    return add(add(a, b), e);
}

// DeltaTrack, path_trace.glsl:150-174, two collisions per trip, software-pipelined like ratio_track: the second collision's free
// flight and fetch are issued beside the first's and the NEXT trip's two collisions are located while the gathers are in flight
// (the RNG chain does not depend on the density); whichever event comes first in sequence order -- exit, accept 1, exit,
// accept 2 -- ends the walk with the RNG state the one-step loop would have, and the trip located ahead is dropped
struct DeltaTrip {
    float s1, a1, s2, a2, t1, t2;
    unsigned long long live1_m, second_m;       // as RatioTrip's
};
__device__ __forceinline__ DeltaTrip delta_trip(float rng, float t, float t_max, float inv)
{
    DeltaTrip r;
    r.s1 = random1(rng);
    r.a1 = random1(r.s1);
    r.s2 = random1(r.a1);
    r.a2 = random1(r.s2);
    const f2 l = logf2(f2{1.0f - r.s1, 1.0f - r.s2});
    r.t1 = nrc_fmaf_(-l.x, inv, t);
    r.t2 = nrc_fmaf_(-l.y, inv, r.t1);
    r.live1_m = lane_mask(!(r.t1 >= t_max));
    r.second_m = lane_mask(!(r.t2 >= t_max));
    return r;
}
// CUT, `cut` (the first walk of a camera path, DESIGN.md section 4.4 "Far cut"): behind t = cut the ray is in empty space for good and the
// lane's RNG state is not a capped one, so every further collision would be rejected and the walk would leave the volume before the cap --
// it leaves at the cut instead: t_max becomes min(t_max, cut).  Hits lie in front of the cut and are the whole walk's; what a leaving lane
// returns (a point of the shorter segment) and its RNG state are never read.  +inf: no cut.  The counting instantiations walk whole, so
// that c.count() stays the algorithm's number, and count the collisions at or behind the cut and those of them that met density
// (a non-zero byte, or an acceptance): the second number is 0 when the cut is sound.
template <bool UNI = false, bool CUT = false, class C>
__device__ __forceinline__ V3 delta_track(C& c, V3 ro, V3 rd, bool* volume_exit, bool valid = true, float cut = __builtin_huge_valf())
{
    V3 en, ex;
    if constexpr (UNI) {      // lanes without a walk march a harmless ray (from the centre along +z): the march must end for them too
        find_entry_exit(c, sel(valid, ro, v3(0.0f, 0.0f, 0.0f)), sel(valid, rd, v3(0.0f, 0.0f, 1.0f)), &en, &ex);
    } else {
        find_entry_exit(c, ro, rd, &en, &ex);
    }
    float t_max = length(sub(ex, ro));
    if constexpr (CUT && !C::counting) t_max = fminf(t_max, cut);
    const float inv = c.sc.inv_max_density;
    float rng = c.rng;
    // loop-carried predicates as uniform lane masks (see ratio_track)
    unsigned long long alive_m = lane_mask(valid), hit_m = 0ull, vexit_m = 0ull;
    float t_hit = 0.0f;
    DeltaTrip a = delta_trip(rng, 0.0f, t_max, inv);
    unsigned long long live1_m = a.live1_m, second_m = a.second_m;
    Addr2 ia = fetch2_addr(c, rd, ro, a.t1, a.t2, lane_bool(a.live1_m), lane_bool(a.live1_m & a.second_m));
    float bs = rng, bt = 0.0f;                 // base of the located trip `a`
    for (uint32_t i = 0;; i += 2) {            // i counts collisions: at most 128 (path_trace.glsl:161); predicated like ratio_track
        const unsigned long long out1_m = alive_m & ~live1_m;        // collision 1 beyond the exit point
        rng = lane_bool(out1_m) ? a.s1 : rng;
        vexit_m |= out1_m;
        alive_m &= live1_m;
        if (alive_m == 0ull) break;
        const bool alive = lane_bool(alive_m);
        if (alive) NRC_PROF(c, 2);
        NRC_PROF_LIVE(2, alive_m);
        const Fetch2 fa = fetch2_load(c, ia);
        __builtin_amdgcn_sched_barrier(0);
        const DeltaTrip b = delta_trip(a.a2, a.t2, t_max, inv);      // located ahead; used only if this trip accepts nothing
        const unsigned long long cap_m = cap_mask(i);
        const unsigned long long go1_m = alive_m & second_m & cap_m & b.live1_m;
        const Addr2 ib = fetch2_addr(c, rd, ro, b.t1, b.t2, lane_bool(go1_m), lane_bool(go1_m & b.second_m));
        __builtin_amdgcn_sched_barrier(0);
        const f2 dens = fetch2_density(c.sc, fa) * splat(inv);
        c.count(alive ? 1u : 0u);
        const unsigned long long acc1_m = alive_m & lane_mask(dens.x > a.a1);
        const unsigned long long alive2_m = alive_m & ~acc1_m;
        const unsigned long long out2_m = alive2_m & ~second_m;      // collision 2 beyond the exit point
        const unsigned long long alive3_m = alive2_m & second_m;
        c.count(lane_bool(alive3_m) ? 1u : 0u);
        const unsigned long long acc2_m = alive3_m & lane_mask(dens.y > a.a2);
        if constexpr (CUT && C::counting) {
            c.count_cut(alive_m & lane_mask(a.t1 >= cut), acc1_m | lane_mask(fa.b0 != 0u));
            c.count_cut(alive3_m & lane_mask(a.t2 >= cut), acc2_m | lane_mask(fa.b1 != 0u));
        }
        hit_m |= acc1_m | acc2_m;
        t_hit = lane_bool(acc2_m) ? a.t2 : t_hit;                    // (two plain selects: the masks are disjoint)
        t_hit = lane_bool(acc1_m) ? a.t1 : t_hit;
        vexit_m |= out2_m;
        // RNG state of the event that ended the walk: accept 1 -> a1, exit 2 -> s2, accept 2 or the 128-collision cap -> a2
        rng = lane_bool(acc1_m) ? a.a1 : rng;
        rng = lane_bool(out2_m) ? a.s2 : rng;
        rng = lane_bool(acc2_m | (alive3_m & ~cap_m)) ? a.a2 : rng;
        alive_m = alive3_m & ~acc2_m & cap_m;
        live1_m = b.live1_m;
        second_m = b.second_m;
        bs = a.a2;
        bt = a.t2;
        a.s1 = b.s1; a.a1 = b.a1; a.s2 = b.s2; a.a2 = b.a2; a.t1 = b.t1; a.t2 = b.t2;
        const bool go = lane_bool(alive_m);
        ia.i0 = go ? ib.i0 : 0x80000000u;                            // a lane that has just finished fetches nothing next trip
        ia.i1 = go ? ib.i1 : 0x80000000u;
    }
    c.rng = rng;
    const bool hit = lane_bool(hit_m);
    *volume_exit = lane_bool(vexit_m);
    if (hit) return madd(rd, t_hit, ro);
    if constexpr (UNI) {
        if (!valid) return ro;          // no walk: no draw
    }
    return madd(rd, c.rand(t_max), ro);
}

// camera ray: mc/render.comp:42-60, nrc/gen_rays.comp:53-72 (no half-pixel offset, no y flip)
__device__ __forceinline__ void camera_ray(const DevCamera& cam, float u, float v, V3* ro, V3* rd)
{
    float sx = nrc_fmaf_(u, 2.0f, -1.0f), sy = nrc_fmaf_(v, 2.0f, -1.0f);
    const float* m = cam.m;
    float wx = nrc_fmaf_(m[4], sy, nrc_fmaf_(m[0], sx, m[12]));
    float wy = nrc_fmaf_(m[5], sy, nrc_fmaf_(m[1], sx, m[13]));
    float wz = nrc_fmaf_(m[6], sy, nrc_fmaf_(m[2], sx, m[14]));
    float ww = nrc_fmaf_(m[7], sy, nrc_fmaf_(m[3], sx, m[15]));
    V3 p = v3(wx / ww, wy / ww, wz / ww);
    *ro = v3(cam.pos[0], cam.pos[1], cam.pos[2]);
    *rd = normalize(sub(p, *ro));
}

// StoreNrcInferInput / StoreNrcTrainData normalisation (quirks Q3-Q5 kept)
__device__ __forceinline__ void nrc_query(const DevScene& s, V3 pos, V3 dir, float* q)
{
    q[0] = pos.x / s.size[0] + s.size[0] / 2.0f;
    q[1] = pos.y / s.size[1] + s.size[1] / 2.0f;
    q[2] = pos.z / s.size[2] + s.size[2] / 2.0f;
    float theta = nrc_atan2f(dir.z, dir.x);
    q[3] = theta / NRC_PI + 0.5f;
    float lxz = sqrtf(dir.x * dir.x + dir.z * dir.z);
    float phi = nrc_acosf(dir.y / lxz);
    q[4] = phi / NRC_PI;
}

// global column of local column lx (nrc_tile: strips of 2^x_block_log2 columns, every x_stride-th strip)
__device__ __forceinline__ uint32_t global_x(const DevFrame& fr, uint32_t lx)
{
    return nrc::global_x(fr.x_offset, fr.x_stride, fr.x_block_log2, lx);
}

// 16x16 pixel tile per 256-thread workgroup, 8x8 per wave (coherent paths inside a wave)
__device__ __forceinline__ bool pixel_of_thread(const DevFrame& fr, uint32_t* lx, uint32_t* y)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    *lx = blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u);
    *y = blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3);
    return *lx < fr.w && *y < fr.h;
}

// Camera kernels: each wave renders one 8x8 pixel tile (coherent paths inside a wave), four tiles of a row per workgroup.
// Tile rows are issued centre-out, so the expensive middle of the image starts first and the cheap rim fills the tail of the
// launch.  Workgroups are dealt to the 8 XCDs round-robin (workgroup b runs on XCD (b + c) mod 8, MI355X_MICROARCH.md) and an
// XCD never helps another out, so the MAPPING must spread the expensive tiles evenly: with 60 workgroups per tile row (1920
// pixels) the XCD of a column alternates between only two values from row to row, every XCD ends up with its own comb of
// columns, and the per-XCD work differed by 1.9x between the lightest and the heaviest (tools/loop_profile.py) -- the launch
// ended with three of eight XCDs busy.  Rows are therefore padded to an ODD number of workgroups (the padding workgroup exits):
// the XCD of a column then walks through all eight values over eight consecutive rows.
// On top of that mapping the tiles are launched costliest first (DevFrame::tile_order, k_tile_order below): slot d of the grid
// renders tile order[d].  (Measured and rejected, tools/loop_profile.py: one-wave workgroups.)
#ifndef NRC_CAMERA_WAVES_PER_BLOCK
#define NRC_CAMERA_WAVES_PER_BLOCK 4
#endif
constexpr uint32_t CAMERA_WAVES_PER_BLOCK = NRC_CAMERA_WAVES_PER_BLOCK;
// (wave priority of the camera kernels: NRC_RAISE_WAVE_PRIORITY in nrc_common.hpp)
__device__ __forceinline__ void camera_wave_priority(const DevFrame& fr)
{
    if (!((NRC_DIAG_LOWPRIO) & 8) && fr.raise_priority != 0u) __builtin_amdgcn_s_setprio(NRC_WAVE_PRIORITY);
}
__host__ __device__ inline uint32_t camera_row_blocks(uint32_t w)
{
    const uint32_t blocks_x = (((w + 7u) >> 3) + CAMERA_WAVES_PER_BLOCK - 1u) / CAMERA_WAVES_PER_BLOCK;
    return blocks_x | 1u;
}
// *slot: the wave's default slot (index into DevFrame::tile_cost)
// The renderer's query / radiance buffers are tile-major INSIDE the renderer: query ((ty * tiles_x + tx) * 64 + (y & 7) * 8 + (x & 7)) is
// pixel (x, y) of the camera kernels' 8x8 tile (tx, ty) -- a gen_rays wave stores its 64 queries as one 1 280-byte run, and the 32
// queries of an inference tile are four rows of eight neighbouring pixels, so the compositing epilogue of the inference kernel reads
// and writes whole 128-byte row segments of the images.  Tiles beyond the image's edge keep all-zero queries (never computed).  The
// reference's x * H + y order (nrc/prep_infer_rays.comp:31) is what nrc_renderer_buffer hands out (k_query_layout), and what the
// cache's own API speaks.
__host__ __device__ inline size_t query_index(uint32_t w, uint32_t lx, uint32_t y)
{
    const uint32_t tiles_x = (w + 7u) >> 3;
    return ((size_t)((y >> 3) * tiles_x + (lx >> 3)) << 6) + ((y & 7u) << 3) + (lx & 7u);
}
// launch slot (workgroup * 4 + wave) -> the wave's pixel
__device__ __forceinline__ bool pixel_of_launch_slot(const DevFrame& fr, uint32_t d, uint32_t* lx, uint32_t* y, uint32_t* slot = nullptr)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tiles_x = (fr.w + 7u) >> 3, tiles_y = (fr.h + 7u) >> 3;
    const uint32_t row_blocks = camera_row_blocks(fr.w);
    if (fr.tile_order != nullptr) d = scalar_load(fr.tile_order + d);      // costliest tiles first
    if (slot) *slot = d;
    const uint32_t bd = d / CAMERA_WAVES_PER_BLOCK;
    const uint32_t k = bd / row_blocks, jb = bd - k * row_blocks;
    const uint32_t tx = jb * CAMERA_WAVES_PER_BLOCK + (d - bd * CAMERA_WAVES_PER_BLOCK);
    if (k >= tiles_y || tx >= tiles_x) return false;
    const uint32_t mid = tiles_y >> 1;
    const uint32_t ty = (k & 1u) ? mid - ((k + 1u) >> 1) : mid + (k >> 1);      // mid, mid-1, mid+1, ...: a bijection
    *lx = tx * 8u + (lane & 7u);
    *y = ty * 8u + (lane >> 3);
    return *lx < fr.w && *y < fr.h;
}
__device__ __forceinline__ bool pixel_of_wave_tile(const DevFrame& fr, uint32_t* lx, uint32_t* y, uint32_t* slot = nullptr)
{
    return pixel_of_launch_slot(fr, __builtin_amdgcn_readfirstlane(blockIdx.x * CAMERA_WAVES_PER_BLOCK + (threadIdx.x >> 6)), lx, y, slot);
}

// Empty-space early-out, exact: the tile mask (k_tile_mask) clears the bit of an 8x8 tile only when no camera ray of the tile can
// come within a voxel of non-empty density.  Every density such a ray's delta tracking fetches is 0, so every tentative collision
// is rejected and the walk can end in two ways only: it leaves the volume (the pixel is env(rd), didScatter = 0, an all-zero
// query, and the RNG state behind the walk is never used), or it runs into DeltaTrack's cap of 128 collisions
// (path_trace.glsl:161-173) and "scatters" at a random point of the segment.  Which of the two happens is a function of the
// pixel's RNG state alone: the hash chain has only 2^23 states, and k_flight_table computes, for every state, the optical distance
// the 128 free flights drawn from it cover.  A state whose distance exceeds the largest optical depth any ray of the scene can
// have (with a margin for the rounding of the walk's own sums) provably leaves the volume before the cap; the others ("capped":
// k_flight_select) reach the kernels as a short list -- for the bench scene the chain's fixed point 0 alone (hash(0) = 0: every
// flight has length 0) -- or, for denser media, as one bit per state.  A tile's waves skip the walk only when no pixel of the
// tile is in a capped state.
__device__ __forceinline__ bool tile_mask_clear(const DevFrame& fr, uint32_t lx, uint32_t y)
{
    if (fr.tile_mask == nullptr || fr.flight_mode == 0u) return false;
    const uint32_t tiles_x = (fr.w + 7u) >> 3, tiles_y = (fr.h + 7u) >> 3;
    const uint32_t id = __builtin_amdgcn_readfirstlane((y >> 3) * tiles_x + (lx >> 3));      // wave-uniform: one tile per wave
    const uint32_t n_words = (tiles_x * tiles_y + 31u) >> 5;
    uint32_t word, ignore;
    scalar_load2(fr.tile_mask + (id >> 5), fr.tile_mask + n_words, &word, &ignore);
    return ignore == 0u && ((word >> (id & 31u)) & 1u) == 0u;
}
// is a pixel of the wave's tile in a capped RNG state?  (wave-uniform)
__device__ __forceinline__ bool tile_has_capped_state(const DevFrame& fr, bool inside, float rng0)
{
    // state -> mantissa: the states are the multiples of 2^-23 in [0, 1), so rng0 + 1 is exact
    const uint32_t m = nrc_f2u(rng0 + 1.0f) & 0x007fffffu;
    bool capped = false;
    if (fr.flight_mode == 1u) {      // a handful of states: compared one by one (no memory access)
#pragma unroll
        for (uint32_t k = 0; k < kFlightListMax; k++) capped |= (k < fr.flight_n) & (m == fr.flight_list[k]);
    } else {
        capped = ((fr.flight_bits[m >> 5] >> (m & 31u)) & 1u) != 0u;
    }
    return __ballot(inside & capped) != 0ull;
}
__device__ __forceinline__ bool tile_is_empty(const DevFrame& fr, uint32_t lx, uint32_t y, bool inside, float rng0)
{
    return tile_mask_clear(fr, lx, y) && !tile_has_capped_state(fr, inside, rng0);
}
// Far cut: the same argument for the TAIL of a camera ray.  DevFrame::tile_far bounds the distance from the camera
// position to the farthest point of every mask box the tile's rays can pass through; a collision farther out reads density 0, and so does
// every later one.  tile_mask_look is tile_mask_clear for the camera kernels: the tile's bound comes with the mask word, in the same
// round trip through the scalar cache (*far_bits; +inf where there is no mask in force or a box behind the eye switches it off).
// tile_far_cut: the bound the wave may use -- +inf as well when a pixel of the tile is in a capped state (such a walk may end at the cap,
// not outside).  Wave-uniform.
__device__ __forceinline__ bool tile_mask_look(const DevFrame& fr, uint32_t lx, uint32_t y, uint32_t* far_bits)
{
    *far_bits = 0x7f800000u;
    if (fr.tile_mask == nullptr || fr.flight_mode == 0u) return false;
    const uint32_t tiles_x = (fr.w + 7u) >> 3, tiles_y = (fr.h + 7u) >> 3;
    const uint32_t id = __builtin_amdgcn_readfirstlane((y >> 3) * tiles_x + (lx >> 3));      // wave-uniform: one tile per wave
    const uint32_t n_words = (tiles_x * tiles_y + 31u) >> 5;
    uint32_t word, ignore, far;
    const uint32_t* farp = fr.tile_far != nullptr ? reinterpret_cast<const uint32_t*>(fr.tile_far) + id : fr.tile_mask + n_words;
    scalar_load3(fr.tile_mask + (id >> 5), fr.tile_mask + n_words, farp, &word, &ignore, &far);
    if (ignore == 0u && fr.tile_far != nullptr) *far_bits = far;
    return ignore == 0u && ((word >> (id & 31u)) & 1u) == 0u;
}
__device__ __forceinline__ float tile_far_cut(const DevFrame& fr, uint32_t far_bits, bool inside, float rng0)
{
    if (far_bits == 0x7f800000u || tile_has_capped_state(fr, inside, rng0)) return __builtin_huge_valf();
    return nrc_u2f(far_bits);
}
// a lane's cut for the walk that starts at `entry`: the walk's t counts from there, and entry = eye + s * rd with s = dot(entry - eye, rd)
// (signed: an eye inside the box has s <= 0).  The rounding of s and of the difference is inside tile_far_bound's margin.
__device__ __forceinline__ float camera_far_cut(float far, const DevCamera& cam, V3 entry, V3 rd)
{
    return far - dot(sub(entry, v3(cam.pos[0], cam.pos[1], cam.pos[2])), rd);
}

// optical distance (in units of 1 / sigma_max) covered by the 128 free flights of a delta walk that starts in RNG state
// float_construct(m) and rejects every tentative collision: draws alternate flight, acceptance (path_trace.glsl:163-170)
__global__ __launch_bounds__(256) void k_flight_table(float* __restrict__ table)
{
    fill_log_table();
    const uint32_t m = blockIdx.x * 256u + threadIdx.x;
    float r = float_construct(m);
    float d = 0.0f;
    for (int k = 0; k < 128; k++) {
        const float s = random1(r);
        d = d - nrc_logf(1.0f - s, s_log_tab);
        r = random1(s);
    }
    table[m] = d;
}

__global__ __launch_bounds__(256) void k_flight_select(const float* __restrict__ table, float lambda, uint32_t* __restrict__ out, uint32_t* __restrict__ bits)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    const uint32_t m = blockIdx.x * 256u + threadIdx.x;
    const bool capped = !(table[m] > lambda);
    const unsigned long long b = __ballot(capped);
    if ((threadIdx.x & 63u) == 0u) {
        bits[m >> 5] = (uint32_t)b;
        bits[(m >> 5) + 1u] = (uint32_t)(b >> 32);
    }
    if (capped) {
        const uint32_t k = atomicAdd(&out[0], 1u);
        if (k < kFlightListMax) out[1u + k] = m;
    }
}

// The tile of a camera kernel's wave.  With hot tiles (DevFrame::hot_front) the launch has kHotTilesMax waves in front of the
// ordered ones: wave k traces hot tile k, and the wave the order gives that tile to leaves.  false: the wave has nothing to do.
__device__ __forceinline__ bool camera_wave_tile(const DevFrame& fr, uint32_t* lx_, uint32_t* y_, uint32_t* slot_, bool* inside_, bool* hot_wave_)
{
    uint32_t lx = 0, y = 0, slot = 0;
    bool inside;
    bool hot_wave = false;
    {
        uint32_t d = __builtin_amdgcn_readfirstlane(blockIdx.x * CAMERA_WAVES_PER_BLOCK + (threadIdx.x >> 6));
        if (fr.hot_front != 0u) {
            // the launch has kHotTilesMax waves in front of the ordered ones: wave k traces hot tile k, and the wave the order
            // gives that tile to leaves.  The list is a kernel argument: scalar registers, no load to wait for.
            const uint32_t hot_n = fr.hot_n;
            const uint32_t* hot = fr.hot;
            if (d < kHotTilesMax) {
                if (d >= hot_n) return false;
                uint32_t t = 0;
#pragma unroll
                for (uint32_t k = 0; k < kHotTilesMax; k++) t = d == k ? hot[k] : t;
                // the list has one entry per capped PIXEL: two such pixels in one tile list the tile twice, and the tile must
                // still be traced exactly once (k_mc_render blends in place) -- the later duplicate leaves
                bool dup = false;
#pragma unroll
                for (uint32_t k = 0; k + 1u < kHotTilesMax; k++) dup |= (k < d) & (hot[k] == t);
                if (dup) return false;
                const uint32_t lane = threadIdx.x & 63u;
                lx = (t & 0xffffu) * 8u + (lane & 7u);
                y = (t >> 16) * 8u + (lane >> 3);
                inside = lx < fr.w && y < fr.h;
                hot_wave = true;
            } else {
                inside = pixel_of_launch_slot(fr, d - kHotTilesMax, &lx, &y, &slot);
                const uint32_t t = __builtin_amdgcn_readfirstlane(((y >> 3) << 16) | (lx >> 3));
                bool is_hot = false;
#pragma unroll
                for (uint32_t k = 0; k < kHotTilesMax; k++) is_hot |= (k < hot_n) & (t == hot[k]);
                if (is_hot) return false;
            }
        } else {
            inside = pixel_of_launch_slot(fr, d, &lx, &y, &slot);
        }
    }
    *lx_ = lx; *y_ = y; *slot_ = slot; *inside_ = inside; *hot_wave_ = hot_wave;
    return true;
}

// what a tile cost in this launch, kept as a decaying maximum over the sampled launches (DevFrame::tile_cost_keep)
__device__ __forceinline__ void store_tile_cost(const DevFrame& fr, uint32_t slot, unsigned long long cycles)
{
    uint32_t c = (uint32_t)min(cycles, 0xffffffffull);
    if (fr.tile_cost_keep != 0u) {
        const uint32_t old = fr.tile_cost[slot];
        c = max(c, old - (old >> fr.tile_cost_keep));
    }
    fr.tile_cost[slot] = c;
}

// [2], [3]: the far cut's proof (CtxT::count_cut)
template <class C>
__device__ __forceinline__ void count_cut_fetches(unsigned long long* counter, const C& c)
{
    if (counter == nullptr || (threadIdx.x & 63u) != 0u) return;
    if (c.cut_n != 0u) atomicAdd(counter + 2, (unsigned long long)c.cut_n);
    if (c.cut_met != 0u) atomicAdd(counter + 3, (unsigned long long)c.cut_met);
}
__device__ __forceinline__ void count_fetches(unsigned long long* counter, uint32_t n)
{
    if (counter == nullptr) return;
    unsigned long long v = n;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63u) == 0) atomicAdd(counter, v);
}

// The stores of k_gen_rays' frame outputs (primary colour, scatter flag, query: 40 B per pixel = 83 MB per 1080p launch) are plain
// write-back stores; write-through (sc0 sc1) and non-temporal stores were measured and lost (docs/MEASUREMENT_LOG.md).
typedef float out_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void out_store(float4* p, float4 v)
{
    *p = v;
}
__device__ __forceinline__ void out_store(float* p, float v)
{
    *p = v;
}

// ------------------------------------------------------------------------------------------------ the view AOV (nrc_view_aov.hpp)
// {alpha, tau, z_front, z_half} of every pixel's camera ray: exact for the piecewise-constant medium, no random numbers.  One wave per
// 8x8 tile and one lane per pixel, as in k_gen_rays, in the default tile order.  A tile the view's mask rejects stores the empty result
// and is gone before the occupancy table is copied (no ray of such a tile comes within a voxel of a non-empty one: what a walk would
// return).  The other lanes run the header's two-level walk: empty coarse cells are left in one jump against the occupancy bits in LDS,
// voxels of occupied cells are fetched through the raw buffer (an offset beyond the volume reads 0 without a memory access) -- the
// byte's load is issued before the step's plane parameters are formed and used behind them.  Lanes of a tile cross nearly the same
// cells, so the jump / step branches diverge at the silhouette only.
struct AovDensity {
    __amdgpu_buffer_rsrc_t vol;
    uint32_t nx, ny;
    __device__ __forceinline__ uint32_t operator()(uint32_t ix, uint32_t iy, uint32_t iz) const
    {
        return __builtin_amdgcn_raw_buffer_load_b8(vol, (int)((iz * ny + iy) * nx + ix), 0, 0);
    }
};
__global__ __launch_bounds__(64 * CAMERA_WAVES_PER_BLOCK) void k_view_aov(DevScene sc, DevCamera cam, DevFrame fr, float4* __restrict__ out)
{
    camera_wave_priority(fr);
    __shared__ uint32_t s_occ[kOccMaxWords];
    uint32_t lx = 0, y = 0;
    const bool inside = pixel_of_wave_tile(fr, &lx, &y);
    if (__ballot(inside) == 0ull) return;      // a padding workgroup's wave
    const size_t pix = (size_t)y * fr.w + lx;
    if (tile_mask_clear(fr, lx, y)) {
        if (inside) out[pix] = make_float4(0.0f, 0.0f, NRC_AOV_INF, NRC_AOV_INF);
        return;
    }
    const uint32_t* occ = load_occupancy_per_wave(sc, s_occ);
    if (!inside) return;
    const uint32_t gx = global_x(fr, lx);
    const float u = (float)gx * fr.inv_gw, v = (float)y * fr.inv_gh;      // k_gen_rays' u, v
    const AovRay ray = view_aov_camera_ray(cam.m, cam.pos, u, v);
    const AovGrid g{sc.nx, sc.ny, sc.nz, {sc.size[0], sc.size[1], sc.size[2]}, sc.density_factor, sc.occ_shift, sc.occ_gx, sc.occ_gy};
    const AovDensity den{__builtin_amdgcn_make_buffer_rsrc((void*)sc.density, 0, (int)(sc.nx * sc.ny * sc.nz), 0x00020000), sc.nx, sc.ny};
    const ViewAov r = occ != nullptr ? view_aov_walk(g, ray, den, AovOccupancyBits{occ}) : view_aov_walk(g, ray, den, NoOccupancy{});
    out[pix] = make_float4(r.alpha, r.tau, r.z_front, r.z_half);
}

// ------------------------------------------------------------------------------------------------ the ray AOV (nrc_view_aov.hpp, view_aov_walk_range)
// The same of caller-supplied ray segments: one kernel over a ray SOURCE, which says which ray a lane has, its range and where the result
// goes -- nothing else.  The kernel owns the rest once: the wave priority of the camera kernels, the occupancy copy into LDS (<= 8 KB per
// workgroup of four waves, as in k_view_aov), the raw-buffer density functor, the choice of the walk for a medium without a table, and
// the one 16-byte store per ray.  A source has
//   raise      the launcher's wave-priority switch (DevFrame::raise_priority)
//   Lane       a lane's own state; lane(&ln): does the lane have a ray (ln.at: its index in out)
//   rejected   wave-uniform: no ray of the wave can meet the medium, whatever its range -- the wave stores empty results and is gone
//              before the table is copied
//   ray        the lane's ray and range
struct RayListLane { size_t at; };
// ray i of a list: d_rays[i] = {ox, oy, oz, t_min, dx, dy, dz, t_max}, read as two 16-byte loads; lane i of the grid takes ray i
struct RayList {
    const float4* __restrict__ rays;
    float4* __restrict__ out;
    size_t n;
    uint32_t raise;
    using Lane = RayListLane;
    __device__ __forceinline__ bool lane(Lane* ln) const
    {
        ln->at = (size_t)blockIdx.x * (64u * CAMERA_WAVES_PER_BLOCK) + threadIdx.x;
        return ln->at < n;
    }
    __device__ __forceinline__ bool rejected(const Lane&) const { return false; }
    __device__ __forceinline__ void ray(const Lane& ln, AovRay* r, float* t_min, float* t_max) const
    {
        const float4 a = rays[2u * ln.at], b = rays[2u * ln.at + 1u];
        *r = AovRay{{a.x, a.y, a.z}, {b.x, b.y, b.z}};
        *t_min = a.w;
        *t_max = b.w;
    }
};
// the renderer's frame, every pixel's camera ray up to the pixel's depth (a holdout): k_view_aov's tiles, columns and mask -- the mask's
// guarantee (no ray of the tile comes within a voxel of a non-empty one) does not depend on the depth
struct ViewDepthLane { size_t at; uint32_t lx, y; };
struct ViewDepth {
    DevCamera cam;
    DevFrame fr;
    const float* __restrict__ depth;
    float4* __restrict__ out;
    uint32_t raise;
    using Lane = ViewDepthLane;
    __device__ __forceinline__ bool lane(Lane* ln) const
    {
        ln->lx = ln->y = 0u;
        const bool inside = pixel_of_wave_tile(fr, &ln->lx, &ln->y);
        ln->at = (size_t)ln->y * fr.w + ln->lx;
        return inside;
    }
    __device__ __forceinline__ bool rejected(const Lane& ln) const { return tile_mask_clear(fr, ln.lx, ln.y); }
    __device__ __forceinline__ void ray(const Lane& ln, AovRay* r, float* t_min, float* t_max) const
    {
        const uint32_t gx = global_x(fr, ln.lx);
        *r = view_aov_camera_ray(cam.m, cam.pos, (float)gx * fr.inv_gw, (float)ln.y * fr.inv_gh);      // k_view_aov's ray
        *t_min = 0.0f;
        *t_max = depth != nullptr ? depth[ln.at] : NRC_AOV_INF;      // (null: every pixel's whole ray)
    }
};
// an orthographic image of w x h pixels, its size the caller's: one 8x8 pixel tile per wave in row-major tile order, so that a wave's
// rays cross neighbouring voxels; every ray walked whole
struct OrthoViewLane { size_t at; uint32_t i, j; };
struct OrthoView {
    AovOrthoView view;
    uint32_t w, h;
    float4* __restrict__ out;
    uint32_t raise;
    using Lane = OrthoViewLane;
    __device__ __forceinline__ bool lane(Lane* ln) const
    {
        const uint32_t tiles_x = (w + 7u) >> 3, lane = threadIdx.x & 63u;
        const uint32_t tile = __builtin_amdgcn_readfirstlane(blockIdx.x * CAMERA_WAVES_PER_BLOCK + (threadIdx.x >> 6));
        const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
        ln->i = tx * 8u + (lane & 7u);
        ln->j = ty * 8u + (lane >> 3);
        ln->at = (size_t)ln->j * w + ln->i;
        return ln->i < w && ln->j < h;      // (a tile row beyond the image: j >= h)
    }
    __device__ __forceinline__ bool rejected(const Lane&) const { return false; }
    __device__ __forceinline__ void ray(const Lane& ln, AovRay* r, float* t_min, float* t_max) const
    {
        *r = ray_aov_ortho_ray(view, ln.i, ln.j, w, h);
        *t_min = 0.0f;
        *t_max = NRC_AOV_INF;
    }
};
// ------------------------------------------------------------------------------------------------ the deep AOV (nrc_view_aov.hpp, deep_aov_walk_range)
// The depths at which a ray reaches the caller's K optical depths, in the one walk that also forms the flat result: the same kernel over
// the same three sources with another OUTPUT -- FlatOut: the four numbers alone, to the source's `out`; DeepOut: the header's deep sum in
// the walk (a source's `out` is the flat image there, and may be null).
//   output   planar: level k of ray i at z[k * n + i], so the 64 stores a wave makes of one level are neighbours.  A lane stores z[k] when
//            it crosses level k (the sum keeps no depth: K registers would not fit) and +inf to the planes it never reached after the walk.
//   levels   the same for every ray, but `next` is the lane's own: they come by value in the kernel arguments and every wave copies them to
//            its own 128 bytes of LDS (beside the 8 KB table and the 1 KB log table), where a per-lane index costs neither scratch nor K
//            registers.  The copy is the wave's own -- a wave fence, no workgroup barrier, as for the table.
//   rejected a wave whose tile the mask rejects stores +inf to all K planes (and the empty flat result) and is gone before either copy.
struct AovLevels { float v[kAovDeepMaxLevels]; };
struct FlatOut {
    static constexpr bool deep = false;
};
struct DeepOut {
    static constexpr bool deep = true;
    float* __restrict__ z;
    size_t n;                // rays: the stride of a plane
    uint32_t n_levels;
    AovLevels levels;        // (those beyond n_levels: 0, never read by the walk)
};
template <typename Src, typename Out>
__global__ __launch_bounds__(64 * CAMERA_WAVES_PER_BLOCK) void k_ray_aov(DevScene sc, Src src, Out o)
{
    if (!((NRC_DIAG_LOWPRIO) & 8) && src.raise != 0u) __builtin_amdgcn_s_setprio(NRC_WAVE_PRIORITY);      // camera_wave_priority
    __shared__ uint32_t s_occ[kOccMaxWords];
    typename Src::Lane ln;
    const bool inside = src.lane(&ln);
    if (__ballot(inside) == 0ull) return;      // a wave beyond the rays
    if (src.rejected(ln)) {
        if (inside) {
            if constexpr (Out::deep)
                for (uint32_t k = 0; k < o.n_levels; k++) o.z[(size_t)k * o.n + ln.at] = NRC_AOV_INF;
            if (!Out::deep || src.out != nullptr) src.out[ln.at] = make_float4(0.0f, 0.0f, NRC_AOV_INF, NRC_AOV_INF);
        }
        return;
    }
    float* levels = nullptr;
    if constexpr (Out::deep) {
        __shared__ float s_levels[CAMERA_WAVES_PER_BLOCK][kAovDeepMaxLevels];
        levels = s_levels[threadIdx.x >> 6];
        if ((threadIdx.x & 63u) < kAovDeepMaxLevels) levels[threadIdx.x & 63u] = o.levels.v[threadIdx.x & 63u];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    const uint32_t* occ = load_occupancy_per_wave(sc, s_occ);
    if (!inside) return;
    AovRay ray;
    float t_min, t_max;
    src.ray(ln, &ray, &t_min, &t_max);
    const AovGrid g{sc.nx, sc.ny, sc.nz, {sc.size[0], sc.size[1], sc.size[2]}, sc.density_factor, sc.occ_shift, sc.occ_gx, sc.occ_gy};
    const AovDensity den{__builtin_amdgcn_make_buffer_rsrc((void*)sc.density, 0, (int)(sc.nx * sc.ny * sc.nz), 0x00020000), sc.nx, sc.ny};
    ViewAov r;
    if constexpr (Out::deep) {
        AovDeepArray sink{o.z + ln.at, o.n};
        r = occ != nullptr ? deep_aov_walk_range(g, ray, t_min, t_max, den, AovOccupancyBits{occ}, levels, o.n_levels, &sink)
                           : deep_aov_walk_range(g, ray, t_min, t_max, den, NoOccupancy{}, levels, o.n_levels, &sink);
    } else {
        r = occ != nullptr ? view_aov_walk_range(g, ray, t_min, t_max, den, AovOccupancyBits{occ})
                           : view_aov_walk_range(g, ray, t_min, t_max, den, NoOccupancy{});
    }
    if (!Out::deep || src.out != nullptr) src.out[ln.at] = make_float4(r.alpha, r.tau, r.z_front, r.z_half);
}

// ------------------------------------------------------------------------------------------------ nrc/gen_rays.comp + prep_infer_rays.comp
#ifndef NRC_GEN_WAVES_PER_SIMD
#define NRC_GEN_WAVES_PER_SIMD NRC_CAMERA_WAVES_PER_SIMD
#endif
template <bool COUNT>
__global__ __launch_bounds__(64 * CAMERA_WAVES_PER_BLOCK, NRC_GEN_WAVES_PER_SIMD) void k_gen_rays(DevScene sc, DevCamera cam, DevFrame fr, uint32_t primary_ray_length,
                                                 float primary_ray_prob, float4* __restrict__ primary,
                                                 float* __restrict__ info, float4* __restrict__ origin,
                                                 float4* __restrict__ dirs, float* __restrict__ infer_in,
                                                 unsigned long long* fetch_counter, TrainGrid tg, int full_vertex_images)
{
    camera_wave_priority(fr);
    const unsigned long long t_start = __builtin_amdgcn_s_memtime();
    __shared__ uint32_t s_occ[kOccMaxWords];
    uint32_t lx = 0, y = 0, slot = 0;
    bool inside, hot_wave;
    if (!camera_wave_tile(fr, &lx, &y, &slot, &inside, &hot_wave)) return;
#ifdef NRC_LOOP_PROFILE
    const uint32_t wave_id = blockIdx.x * CAMERA_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if ((threadIdx.x & 63u) == 0 && wave_id < 65536u) {
        unsigned xcc, hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        g_wave_times[4 * wave_id] = wall_clock64();
        g_wave_times[4 * wave_id + 2] = xcc;
        g_wave_times[4 * wave_id + 3] = hw;
    }
#endif
    if (__ballot(inside) == 0ull) return;      // a padding workgroup's wave (the grid is rounded up to whole rows of workgroups)
    CtxT<COUNT> c{sc, 0.0f, 0u};
    const uint32_t gx = global_x(fr, lx);
    const float u = (float)gx * fr.inv_gw, v = (float)y * fr.inv_gh;
    const float seed_uv = random2(u, v);      // the pixel's part of init_random's seed
    // Two of three tiles of the bench view miss the medium.  Their waves are the tail of the launch (k_tile_order starts the
    // costliest tiles first): the tile's bit comes through the scalar cache, and the wave is gone before the occupancy table is
    // copied (there is no workgroup barrier in this kernel: load_occupancy_per_wave).  What is left of them is dispatch: ~1000
    // waves per microsecond start at the end of the launch (tools/loop_profile.py), and all they do costs 0.004 ms of 0.215.
    if (tile_mask_clear(fr, lx, y)) {
        c.rng = random2(seed_uv, random4(fr.random));      // init_random
        if (!tile_has_capped_state(fr, inside, c.rng)) {
            if (inside) {
                V3 ro, rd;
                camera_ray(cam, u, v, &ro, &rd);
                const V3 e = sample_env_dir(sc, rd);
                const size_t pix = (size_t)y * fr.w + lx;
                out_store(&primary[pix], make_float4(e.x, e.y, e.z, 1.0f));
                out_store(&info[pix], 0.0f);
                if (fr.skip_dead_queries == 0u) {
                    float* qo = infer_in + query_index(fr.w, lx, y) * 5u;
#pragma unroll
                    for (int k = 0; k < 5; k++) out_store(&qo[k], 0.0f);
                }
            }
            if (fr.tile_cost != nullptr && !hot_wave && (threadIdx.x & 63u) == 0) store_tile_cost(fr, slot, __builtin_amdgcn_s_memtime() - t_start);
#ifdef NRC_LOOP_PROFILE
            if (inside && full_vertex_images != 0) reinterpret_cast<float*>(origin)[4 * ((size_t)y * fr.w + lx) + 3] = 0.0f;
            if ((threadIdx.x & 63u) == 0 && wave_id < 65536u) g_wave_times[4 * wave_id + 1] = wall_clock64();
#endif
            return;
        }
    }
    c.occ = load_occupancy_per_wave(sc, s_occ);
    uint32_t far_bits;
    tile_mask_look(fr, lx, y, &far_bits);      // (the tile's far bound: a wave that walks pays a second trip through the scalar cache for it)
    // Wave-uniform control flow with per-lane predicates from here to the stores: a lane whose path has ended (or that has none)
    // stays in the instruction stream, so that the tracking loops can hand the last walks to lane pairs (ratio_pairs).
    V3 ro, rd;
    camera_ray(cam, u, v, &ro, &rd);
    c.rng = random2(seed_uv, random4(fr.random));      // init_random
    const float far = tile_far_cut(fr, far_bits, inside, c.rng);
    const bool enter = inside;
    V3 entry = ro, ex;
    {
#ifdef NRC_LOOP_PROFILE
        c.fee_kind = 0;
#endif
        find_entry_exit(c, sel(enter, ro, v3(0.0f, 0.0f, 0.0f)), sel(enter, rd, v3(0.0f, 0.0f, 1.0f)), &entry, &ex);
#ifdef NRC_LOOP_PROFILE
        c.fee_kind = 1;
#endif
    }
    const bool entered = enter && !(sky_sdf(sc, entry) > 100000.0f);
    // The colour of a pixel that does not scatter -- the environment along its camera ray, throughput 1 (gen_rays.comp:86-95) -- is
    // stored NOW, before the walk; a pixel that scatters overwrites it at the end (same lane, same address: the stores are
    // performed in order).  The camera ray direction is therefore dead during the walk; kept live for the end, two of its
    // components were the one value this kernel spilled to scratch (tests/test_abi.py checks that there is none).
    if (inside) {
        const V3 e = sample_env_dir(sc, rd);
        out_store(&primary[(size_t)y * fr.w + lx], make_float4(e.x, e.y, e.z, 1.0f));
    }
    V3 light = v3(0, 0, 0);
    V3 cur = entry, dir = rd;      // TracePath recomputes the same entry (gen_rays.comp:11)
    float factor = 1.0f;
    bool did_scatter = false, walking = entered;
    for (int i = 0;; i++) {
        if (__ballot(walking) == 0ull) break;
        bool vexit = false;
        // the far cut ends the FIRST walk only: the later ones start from RNG states nobody has classified, and the second vertex's exit
        // point is read (the query)
        const float cut = camera_far_cut(i == 0 ? far : __builtin_huge_valf(), cam, cur, dir);
        const V3 nc = delta_track<true, true>(c, cur, dir, &vexit, walking, cut);
        cur = sel(walking, nc, cur);
        walking &= !vexit;
        did_scatter |= walking;
        factor = walking ? factor * 0.5f : factor;
        if (__ballot(walking) == 0ull) break;
        const V3 ts = trace_scene<true>(c, cur, dir, walking);
        if (walking) {
            light = add(light, mul(ts, factor));
            dir = new_ray_dir(c, dir, true);
            if ((uint32_t)i >= primary_ray_length) {
                if (c.rand(1.0f) >= primary_ray_prob || i == 128) walking = false;
            }
        }
    }
    if (inside) {
        const size_t pix = (size_t)y * fr.w + lx;
        float q[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (entered) {
            // the NRC vertex images (nrcRayOrigin / nrcRayDir of gen_rays.comp:97-100) have one reader besides the query packing
            // fused in here: prep_train_rays, at the pixels (tx * xDist, ty * yDist) of the train grid.  Only those are stored
            // (32 B for 16 384 of 2 073 600 pixels instead of 66 MB per frame) unless the caller asks for the whole images.
            bool on_grid = full_vertex_images != 0;
            if (!on_grid) {
                const uint32_t qx = tg.x_dist ? lx / tg.x_dist : 0u, qy = tg.y_dist ? y / tg.y_dist : 0u;
                on_grid = (qx * tg.x_dist == lx) & (qy * tg.y_dist == y) & (qx < tg.tw) & (qy < tg.th);
            }
            // (scattered pixels only: prep_train_rays reads the images where info == 1, and an unscattered pixel's point is where its walk
            // left -- with the far cut no longer the reference's exit point)
            if (on_grid && did_scatter) {
                origin[pix] = make_float4(cur.x, cur.y, cur.z, 0.0f);
                dirs[pix] = make_float4(dir.x, dir.y, dir.z, 0.0f);
            }
            if (did_scatter) {
                nrc_query(sc, cur, dir, q);
                out_store(&primary[pix], make_float4(light.x, light.y, light.z, factor));      // replaces the environment colour stored above
            }
        }
        out_store(&info[pix], did_scatter ? 1.0f : 0.0f);
        // the reference zero-fills the query buffer each frame (vkCmdFillBuffer, NrcHpmRenderer.cu:1996) and prep_infer_rays writes only
        // scattered pixels.  Here: no memset; without the live-query list every slot is written (zeros for the others: the list-free
        // inference recognises them), with it only the scattered pixels' (DevFrame::skip_dead_queries: nobody reads the rest)
        if (fr.skip_dead_queries == 0u || (entered && did_scatter)) {
            float* qo = infer_in + query_index(fr.w, lx, y) * 5u;
#pragma unroll
            for (int k = 0; k < 5; k++) out_store(&qo[k], q[k]);
        }
    }
    if (fr.live_list != nullptr) {      // the frame's live queries, which the renderer's inference walks (DevFrame::live_list): one atomic per wave
        const bool live = inside && entered && did_scatter;
        const unsigned long long lm = __ballot(live);
        if (lm != 0ull) {
            uint32_t base = 0;
            if ((threadIdx.x & 63u) == 0u) base = atomicAdd(fr.live_count, (uint32_t)__popcll(lm));
            base = __builtin_amdgcn_readfirstlane(base);
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(lm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)lm, 0u));
            if (live) fr.live_list[base + rank] = (uint32_t)query_index(fr.w, lx, y);
        }
    }
#ifdef NRC_LOOP_PROFILE
    // per-pixel look-up count in the w component of the origin image (tools/lane_model.py)
    if (inside && full_vertex_images != 0) reinterpret_cast<float*>(origin)[4 * ((size_t)y * fr.w + lx) + 3] = (float)c.fetches;
#endif
    if constexpr (COUNT) {      // [0] the algorithm's look-ups, [1] those of them the dead-walk rule kept from memory
        count_fetches(fetch_counter, c.fetches);
        if (fetch_counter != nullptr && (threadIdx.x & 63u) == 0u && c.masked != 0u) atomicAdd(fetch_counter + 1, (unsigned long long)c.masked);
        count_cut_fetches(fetch_counter, c);
    }
    // what this tile cost (shader cycles): next frames launch the costliest tiles first (k_tile_order).  (Not for a hot wave: what
    // it measured is this frame's one pixel in a capped state, not the tile.)
    if (fr.tile_cost != nullptr && !hot_wave && (threadIdx.x & 63u) == 0) store_tile_cost(fr, slot, __builtin_amdgcn_s_memtime() - t_start);
#if defined(NRC_LOOP_PROFILE) && !defined(NRC_NO_LOOP_COUNTERS)
    for (int k = 0; k < 8; k++) { count_fetches(&g_loop_prof[k], c.useful[k]); count_fetches(&g_loop_prof[8 + k], c.issued[k]); }
#endif
#ifdef NRC_LOOP_PROFILE
    if ((threadIdx.x & 63u) == 0 && wave_id < 65536u) g_wave_times[4 * wave_id + 1] = wall_clock64();
#endif
}

// ------------------------------------------------------------------------------------------------ mc/render.comp
template <bool COUNT>
__global__ __launch_bounds__(64 * CAMERA_WAVES_PER_BLOCK, NRC_CAMERA_WAVES_PER_SIMD) void k_mc_render(DevScene sc, DevCamera cam, DevFrame fr, uint32_t path_length,
                                                  float blend_factor, float4* __restrict__ out_rgba,
                                                  float* __restrict__ info, unsigned long long* fetch_counter)
{
    camera_wave_priority(fr);
    const unsigned long long t_start = __builtin_amdgcn_s_memtime();
    __shared__ uint32_t s_occ[kOccMaxWords];
    const uint32_t* occ = load_occupancy(sc, s_occ);
    uint32_t lx = 0, y = 0, slot = 0;
    bool inside, hot_wave;
    if (!camera_wave_tile(fr, &lx, &y, &slot, &inside, &hot_wave)) return;
    CtxT<COUNT> c{sc, 0.0f, 0u};
    c.occ = occ;
    // wave-uniform control flow with per-lane predicates, as in k_gen_rays (the thin trips of the 32 x 3 tracking loops go to lane pairs)
    const uint32_t gx = global_x(fr, lx);
    const float u = (float)gx * fr.inv_gw, v = (float)y * fr.inv_gh;
    V3 ro, rd;
    camera_ray(cam, u, v, &ro, &rd);
    init_random(c, u, v, fr.random);
    // (the capped states are looked up only where the mask is in force: without it there is no selection -- flight_bits is null)
    uint32_t far_bits;
    const bool clear = tile_mask_look(fr, lx, y, &far_bits);
    const bool capped = (clear || far_bits != 0x7f800000u) && tile_has_capped_state(fr, inside, c.rng);
    const bool empty = clear && !capped;      // wave-uniform, see tile_is_empty
    const float far = capped ? __builtin_huge_valf() : nrc_u2f(far_bits);
    const bool enter = inside & !empty;
    V3 entry = ro, ex;
    if (__ballot(enter) != 0ull) find_entry_exit(c, sel(enter, ro, v3(0.0f, 0.0f, 0.0f)), sel(enter, rd, v3(0.0f, 0.0f, 1.0f)), &entry, &ex);
    const bool entered = enter && !(sky_sdf(sc, entry) > 100000.0f);
    V3 light = v3(0, 0, 0);
    V3 cur = entry, dir = rd;
    float factor = 1.0f;
    bool did_scatter = false, walking = entered;
    for (uint32_t i = 0; i < path_length; i++) {
        if (__ballot(walking) == 0ull) break;
        bool vexit = false;
        const float cut = camera_far_cut(i == 0u ? far : __builtin_huge_valf(), cam, cur, dir);      // the first walk only, as in k_gen_rays
        const V3 nc = delta_track<true, true>(c, cur, dir, &vexit, walking, cut);
        cur = sel(walking, nc, cur);
        walking &= !vexit;
        did_scatter |= walking;
        factor = walking ? factor * 0.5f : factor;
        if (__ballot(walking) == 0ull) break;
        const V3 ts = trace_scene<true>(c, cur, dir, walking);
        if (walking) {
            light = add(light, mul(ts, factor));
            dir = new_ray_dir(c, dir, true);
        }
    }
    if (inside) {
        V3 col = light;
        if (!did_scatter) col = sample_env_dir(sc, rd);
        const float a = did_scatter ? 1.0f : 0.0f;
        const size_t pix = (size_t)y * fr.w + lx;
        const float4 prev = out_rgba[pix];
        const float ib = 1.0f - blend_factor;
        out_rgba[pix] = make_float4(blend_factor * col.x + ib * prev.x, blend_factor * col.y + ib * prev.y,
                                    blend_factor * col.z + ib * prev.z, blend_factor * a + ib * prev.w);
        if (info) info[pix] = a;
    }
    if constexpr (COUNT) {      // [0] the algorithm's look-ups, [1] those of them the dead-walk rule kept from memory
        count_fetches(fetch_counter, c.fetches);
        if (fetch_counter != nullptr && (threadIdx.x & 63u) == 0u && c.masked != 0u) atomicAdd(fetch_counter + 1, (unsigned long long)c.masked);
        count_cut_fetches(fetch_counter, c);
    }
    if (fr.tile_cost != nullptr && !hot_wave && (threadIdx.x & 63u) == 0)      // see k_gen_rays / k_tile_order (a longer walk: 8 192-cycle classes)
        store_tile_cost(fr, slot, (__builtin_amdgcn_s_memtime() - t_start) >> 4);
}

// ------------------------------------------------------------------------------------------------ costliest-first launch order
// A tile costs between 2 us (provably empty) and 160 us (cloud interior), a launch holds ~4 200 of its 32 400 waves at a time, and
// the hardware starts workgroups in index order: in the default centre-out order the last expensive tiles start at 60 % of the
// launch and a third of its duration is a thinning tail (tools/loop_profile.py).  Tile costs repeat from frame to frame
// (correlation 0.95), so the waves are launched in order of decreasing cost of an earlier frame: a counting sort over 1024
// cost classes of 512 cycles, one workgroup, order within a class arbitrary -- any permutation gives the same frame.
// (Measured and taken out again, rounds 2-4: ranking a tile by the maximum over its four neighbours; listing the costliest tiles as two
// half tiles -- DESIGN.md section 4.)
__global__ __launch_bounds__(1024) void k_tile_order(const uint32_t* __restrict__ cost, uint32_t n, uint32_t* __restrict__ order)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    __shared__ uint32_t hist[1024];
    const uint32_t tid = threadIdx.x;
    hist[tid] = 0u;
    __syncthreads();
    auto key_of = [=](uint32_t i) { return 1023u - min(cost[i] >> 9, 1023u); };      // descending cost
    for (uint32_t i = tid; i < n; i += 1024u) atomicAdd(&hist[key_of(i)], 1u);
    __syncthreads();
    // exclusive prefix sum over the 1024 classes (wave scans + wave totals)
    const uint32_t v = hist[tid];
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off);
        if ((int)(tid & 63u) >= off) incl += t;
    }
    __shared__ uint32_t wsum[16];
    if ((tid & 63u) == 63u) wsum[tid >> 6] = incl;
    __syncthreads();
    uint32_t woff = 0;
    for (uint32_t w = 0; w < (tid >> 6); w++) woff += wsum[w];
    __syncthreads();
    hist[tid] = woff + incl - v;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += 1024u) order[atomicAdd(&hist[key_of(i)], 1u)] = i;
}

// XCD-aware finish of the order (round 4; xcd_row_len = slots per tile row).  The hardware deals workgroups to the eight XCDs round-robin, so
// the 32 M consecutive ranks of workgroups 8 M j .. 8 M (j + 1) - 1 -- tiles of about the same cost -- start together, 4 M on each XCD.  Within
// such a window the tiles are handed out by SCREEN ROW: the 4 M topmost to the first XCD, the next to the second, ...  Every XCD then works
// on a band of rows -- in whatever class of cost the launch is at -- and the volume's [z][y][x] lines its camera rays touch are its own: each
// 4 MB L2 sees a part of the volume instead of all of it.  The order stays a permutation, costliest first.  wg_off = the workgroups in
// front of the ordered ones (the hot tiles' two).  A kernel of its own because k_tile_order is ONE workgroup.
__global__ __launch_bounds__(1024) void k_tile_order_xcd(uint32_t* __restrict__ order, uint32_t n, uint32_t xcd_row_len, uint32_t wg_off)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    // one workgroup per window of blockDim.x = 32 M ranks (M workgroups per XCD); a window that is not whole (the first one behind the hot
    // tiles' workgroups, the last one) keeps its order
    __shared__ uint32_t keys[1024];
    const uint32_t S = blockDim.x, m4 = S >> 3;                // ranks per XCD and window
    const uint32_t tid = threadIdx.x;
    const uint32_t tiles_y = n / xcd_row_len, mid = tiles_y >> 1;
    const long long r0 = (long long)blockIdx.x * S - (long long)wg_off * 4;      // rank of the window's first slot
    if (r0 < 0 || (unsigned long long)r0 + S > n) return;      // (workgroup-uniform)
    const uint32_t t = order[(uint32_t)r0 + tid];
    const uint32_t k = t / xcd_row_len, j = t - k * xcd_row_len;
    const uint32_t ty = (k & 1u) ? mid - ((k + 1u) >> 1) : mid + (k >> 1);      // pixel_of_launch_slot's row bijection
    const uint32_t key = (ty << 16) | j;                       // unique per tile
    keys[tid] = key;
    __syncthreads();
    uint32_t pos = 0u;
    for (uint32_t q = 0; q < S; q++) pos += keys[q] < key ? 1u : 0u;
    // position pos of the window's tiles by screen row -> XCD pos / m4, its (pos % m4)-th slot: workgroup xcd + 8 * (slot / 4) of the window
    const uint32_t xcd = pos / m4, q = pos - xcd * m4;
    order[(uint32_t)r0 + ((xcd + 8u * (q >> 2)) << 2) + (q & 3u)] = t;
}

// ------------------------------------------------------------------------------------------------ empty-space tile mask
// One thread per occupancy box (world-space AABB around a run of non-empty 8^3-voxel cells, grown by one voxel): its eight
// corners are projected with the camera's forward transform; the screen rectangle around them, grown by a pixel, covers every
// pixel whose camera ray can pass through the box (a pixel's ray consists of the points that project onto the pixel).  The 8x8
// tiles the rectangle touches are marked.  A box with a corner at or behind the eye plane switches the mask off for this camera.
// kRects (k_tile_rects, the tile-parallel build below): instead of marking tiles, the box's tile rectangle goes to *rect, packed into 64
// bits, tx0 | tx1 << 16 | ty0 << 32 | ty1 << 48 (camera_slots bounds a frame's tiles far below 2^16 per axis); a box behind the eye plane
// and one off screen are two sentinels whose row range ty0 > ty1 is empty.  One body, so that the two builds agree to the last bit.
constexpr unsigned long long kTileRectOff = 0x0000ffff00000000ull | 0xfffeull;        // ty0 = 0xffff > ty1 = 0, tx0 = 0xfffe: behind
constexpr unsigned long long kTileRectNone = 0x0000ffff00000000ull | 0xffffull;       // ... tx0 = 0xffff: off screen
// The far cut's bound (DevFrame::tile_far, DESIGN.md section 4.4 "Far cut"): both builds also raise, for every tile the box's rectangle
// touches, the tile's float to tile_far_bound of the box -- the distance from the camera position to the box's farthest point (a corner: the
// distance to a point is convex, and a convex function on a box is largest at a vertex), rounded up and grown.  The values are positive
// floats, whose order is the order of their bit patterns: an atomic max on the bits is the maximum, whatever the order of the boxes.
// The margin: the boxes already stand one voxel off every non-empty voxel; on top of that far_margin (a voxel diagonal, from the host) and
// 2^-16 of the distance itself, some hundred times the rounding error of the three products, two sums and the square root here and of
// the lane's own dot product and subtraction in camera_far_cut.
__device__ __forceinline__ float tile_far_bound(const float* b, const DevProjView& pv)
{
    float d2 = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const float x = b[(k & 1) ? 3 : 0] - pv.eye[0], y = b[(k & 2) ? 4 : 1] - pv.eye[1], z = b[(k & 4) ? 5 : 2] - pv.eye[2];
        d2 = fmaxf(d2, x * x + y * y + z * z);
    }
    const float d = sqrtf(d2);
    return d + (d * 0x1p-16f + pv.far_margin);
}
// the tile rectangle of box b = {lo xyz, hi xyz}: t = {tx0, tx1, ty0, ty1}.  0: on screen; 1: a corner at or behind the eye plane; 2: off screen
__device__ __forceinline__ int tile_rect_of(const float* b, const DevProjView& pv, const DevFrame& fr, uint32_t* t)
{
    float xmin = 3.0e38f, xmax = -3.0e38f, ymin = 3.0e38f, ymax = -3.0e38f;
    bool behind = false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const float x = b[(k & 1) ? 3 : 0], y = b[(k & 2) ? 4 : 1], z = b[(k & 4) ? 5 : 2];
        const float cx = pv.m[0] * x + pv.m[4] * y + pv.m[8] * z + pv.m[12];
        const float cy = pv.m[1] * x + pv.m[5] * y + pv.m[9] * z + pv.m[13];
        const float cw = pv.m[3] * x + pv.m[7] * y + pv.m[11] * z + pv.m[15];
        if (!(cw > 1.0e-3f)) { behind = true; continue; }
        const float nx = cx / cw, ny = cy / cw;
        xmin = fminf(xmin, nx); xmax = fmaxf(xmax, nx);
        ymin = fminf(ymin, ny); ymax = fmaxf(ymax, ny);
    }
    if (behind || !(xmin <= xmax) || !(ymin <= ymax)) return 1;      // NaN-safe
    // pixel (gx, y) looks along ndc = (2 gx / gw - 1, 2 y / gh - 1): gx = (ndc.x + 1) / 2 * gw
    const float gw = 1.0f / fr.inv_gw, gh = 1.0f / fr.inv_gh;
    float gx0 = floorf((xmin + 1.0f) * 0.5f * gw) - 1.0f, gx1 = ceilf((xmax + 1.0f) * 0.5f * gw) + 1.0f;
    float gy0 = floorf((ymin + 1.0f) * 0.5f * gh) - 1.0f, gy1 = ceilf((ymax + 1.0f) * 0.5f * gh) + 1.0f;
    // local columns: strip s = gx >> b of the global frame is the local strip (s - x_offset) / x_stride (global_x); every local
    // column of the local strips the rectangle can touch is taken (conservative).  The rectangle touches the global strips s0 .. s1, so the
    // local strips l with s0 <= x_offset + l * x_stride <= s1: from ceil((s0 - x_offset) / x_stride) to floor((s1 - x_offset) / x_stride)
    // (near the frame these are small integers, whose fp32 quotient is an integer only when the true one is: ceil and floor are exact;
    // far outside it the clamps below decide)
    const float blk = (float)(1u << fr.x_block_log2);
    float lx0 = ceilf((floorf(gx0 / blk) - (float)fr.x_offset) / (float)fr.x_stride) * blk;
    float lx1 = (floorf((floorf(gx1 / blk) - (float)fr.x_offset) / (float)fr.x_stride) + 1.0f) * blk - 1.0f;
    lx0 = fmaxf(lx0, 0.0f); gy0 = fmaxf(gy0, 0.0f);
    lx1 = fminf(lx1, (float)(fr.w - 1u)); gy1 = fminf(gy1, (float)(fr.h - 1u));
    if (!(lx0 <= lx1) || !(gy0 <= gy1)) return 2;
    t[0] = (uint32_t)lx0 >> 3; t[1] = (uint32_t)lx1 >> 3; t[2] = (uint32_t)gy0 >> 3; t[3] = (uint32_t)gy1 >> 3;
    return 0;
}
template <bool kRects = false>
__device__ __forceinline__ void tile_mask_box(const float* __restrict__ boxes, uint32_t i, const DevProjView& pv, const DevFrame& fr,
                                              uint32_t* __restrict__ mask, float* __restrict__ far, unsigned long long* __restrict__ rect = nullptr)
{
    const uint32_t tiles_x = (fr.w + 7u) >> 3, tiles_y = (fr.h + 7u) >> 3;
    const uint32_t n_words = (tiles_x * tiles_y + 31u) >> 5;
    const float* b = boxes + 6u * (size_t)i;
    uint32_t t[4];
    const int st = tile_rect_of(b, pv, fr, t);
    if (st == 1) {
        if constexpr (kRects) *rect = kTileRectOff;
        else atomicOr(&mask[n_words], 1u);
        return;
    }
    if (st == 2) {                    // off screen
        if constexpr (kRects) *rect = kTileRectNone;
        return;
    }
    if constexpr (kRects) {
        *rect = (unsigned long long)t[0] | ((unsigned long long)t[1] << 16) | ((unsigned long long)t[2] << 32) | ((unsigned long long)t[3] << 48);
    } else {
        for (uint32_t ty = t[2]; ty <= t[3]; ty++)
            for (uint32_t tx = t[0]; tx <= t[1]; tx++) {
                const uint32_t id = ty * tiles_x + tx;
                const uint32_t bit = 1u << (id & 31u);
                if ((mask[id >> 5] & bit) == 0u) atomicOr(&mask[id >> 5], bit);
            }
    }
    // The far bounds, piece by piece: a box is a run of cells along x, up to the volume's width long, and its farthest corner says little
    // about a tile that sees its near end.  The run is cut into pieces of pv.far_piece (a cell's length) -- consecutive, the same expression
    // for a shared boundary, the last one ending at the box's end: together they are the box.  A ray that passes through the box meets
    // density only inside pieces whose rectangle holds its pixel, so every piece raises the tiles of its OWN rectangle to its own bound.
    // (A piece the projection cannot place -- it cannot be behind the eye when the box is not, but the test is made in fp32 -- raises the
    // box's whole rectangle.)
    uint32_t* far_u = reinterpret_cast<uint32_t*>(far);
    for (uint32_t k = 0; k < 4096u; k++) {
        const float x0 = b[0] + (float)k * pv.far_piece, x1 = fminf(b[0] + (float)(k + 1u) * pv.far_piece, b[3]);
        if (!(x0 < b[3])) break;
        const float piece[6] = {x0, b[1], b[2], k + 1u == 4096u ? b[3] : x1, b[4], b[5]};
        uint32_t q[4];
        const int sp = tile_rect_of(piece, pv, fr, q);
        if (sp == 2) continue;
        if (sp == 1) { q[0] = t[0]; q[1] = t[1]; q[2] = t[2]; q[3] = t[3]; }
        const uint32_t far_bits = nrc_f2u(tile_far_bound(piece, pv));
        for (uint32_t ty = q[2]; ty <= q[3]; ty++)
            for (uint32_t tx = q[0]; tx <= q[1]; tx++) {
                const uint32_t id = ty * tiles_x + tx;
                if (far_u[id] < far_bits) atomicMax(&far_u[id], far_bits);
            }
    }
}

// n = *n_dev when the count lives in device memory (a volume rebuilt on the device, k_vol_rows; the grid covers the capacity), else n_host
__global__ __launch_bounds__(256) void k_tile_mask(const float* __restrict__ boxes, uint32_t n_host, const uint32_t* __restrict__ n_dev, DevProjView pv,
                                                  DevFrame fr, uint32_t* __restrict__ mask, float* __restrict__ far)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    const uint32_t n = n_dev != nullptr ? *n_dev : n_host;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    tile_mask_box(boxes, i, pv, fr, mask, far);
}

// ---- the same mask, built in parallel over its words (nrc_renderer_render_path: a mask per view, beside the previous view's frames).
// k_tile_rects, one lane per box: tile_mask_box's packed rectangle, or one of its two sentinels.  k_tile_mask_words, one wave per mask
// word: the workgroup stages the rectangles through LDS 1024 at a time (each is read from memory once per workgroup), a lane takes every 64th of them and ORs, per tile row of the word the rectangle covers, the span of
// bits [row * tiles_x + tx0, row * tiles_x + tx1] clipped to the word; the lanes' words are OR-reduced across the wave and lane 0 stores the
// result.  The wave behind the last bit word owns the trailing "off" word: 1 when any box is behind the eye plane.  Every word is written,
// once, by a plain store: no atomics, and the buffer needs no clear.
constexpr uint32_t kTileRectChunk = 1024u;

__global__ __launch_bounds__(256) void k_tile_rects(const float* __restrict__ boxes, uint32_t n_host, const uint32_t* __restrict__ n_dev, DevProjView pv,
                                                   DevFrame fr, unsigned long long* __restrict__ rects, float* __restrict__ far)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    const uint32_t n = n_dev != nullptr ? *n_dev : n_host;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    tile_mask_box<true>(boxes, i, pv, fr, nullptr, far, rects + i);
}

__global__ __launch_bounds__(256) void k_tile_mask_words(const unsigned long long* __restrict__ rects, uint32_t n_host, const uint32_t* __restrict__ n_dev,
                                                        DevFrame fr, uint32_t* __restrict__ mask)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    __shared__ unsigned long long stage[kTileRectChunk];
    const uint32_t tiles_x = (fr.w + 7u) >> 3, tiles_y = (fr.h + 7u) >> 3;
    const uint32_t n_words = (tiles_x * tiles_y + 31u) >> 5;
    const uint32_t n = n_dev != nullptr ? *n_dev : n_host;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t word = blockIdx.x * 4u + (threadIdx.x >> 6);      // wave-uniform; n_words: the off word; beyond: staging only
    const uint32_t b0 = word << 5, b1 = b0 + 31u;                     // the word's tile ids
    const uint32_t row_a = b0 / tiles_x, row_b = min(b1 / tiles_x, tiles_y - 1u);
    uint32_t acc = 0u;
    for (uint32_t base = 0; base < n; base += kTileRectChunk) {
        const uint32_t m = min(kTileRectChunk, n - base);
        for (uint32_t k = threadIdx.x; k < m; k += 256u) stage[k] = rects[base + k];
        __syncthreads();
        if (word < n_words) {
            for (uint32_t k = lane; k < m; k += 64u) {
                const unsigned long long r = stage[k];
                const uint32_t tx0 = (uint32_t)r & 0xffffu, tx1 = (uint32_t)(r >> 16) & 0xffffu;
                const uint32_t ty0 = (uint32_t)(r >> 32) & 0xffffu, ty1 = (uint32_t)(r >> 48);
                const uint32_t r0 = max(ty0, row_a), r1 = min(ty1, row_b);
                for (uint32_t row = r0; row <= r1; row++) {
                    const uint32_t lo = max(row * tiles_x + tx0, b0), hi = min(row * tiles_x + tx1, b1);
                    if (lo <= hi) acc |= (0xffffffffu >> (31u - (hi - lo))) << (lo - b0);
                }
            }
        } else if (word == n_words) {
            for (uint32_t k = lane; k < m; k += 64u) acc |= stage[k] == kTileRectOff ? 1u : 0u;
        }
        __syncthreads();
    }
    if (word > n_words) return;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc |= (uint32_t)__shfl_xor((int)acc, off);
    if (lane == 0u) mask[word] = acc;
}

// ------------------------------------------------------------------------------------------------ nrc/clear.comp + ring ordering
// scratch layout: [0..T) scatter flag, [T..2T) exclusive rank among its kind (push rank if scattered, pop rank otherwise),
// [2T] n_push, [2T+1] n_pop, [2T+2] head (wrapped), [2T+3] tail (wrapped).
// Deterministic replacement of the two atomic counters of prep_train_rays.comp:7-31: ranks in linear train-index order.
__global__ __launch_bounds__(1024) void k_train_scan(DevFrame fr, TrainGrid tg, const float* __restrict__ info,
                                                    uint32_t* __restrict__ ring, uint32_t* __restrict__ scratch)
{
    NRC_RAISE_WAVE_PRIORITY(4);
    __shared__ uint32_t wsum[16];
    const uint32_t T = tg.tw * tg.th;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // each thread owns a contiguous run of train indices: flags -> local count -> block-wide exclusive scan -> ranks.
    // Runs of <= 64 indices (T <= 65536, the reference's default 4 x 2^14 included) keep their flags in a register mask, so
    // the strided gathers from the info image are independent and all in flight together; longer runs re-read the flags.
    const uint32_t per = (T + 1023u) / 1024u;
    const uint32_t i0 = min(tid * per, T), i1 = min(i0 + per, T);
    const bool in_regs = per <= 64u;
    auto flag_of = [&](uint32_t i) -> uint32_t {
        const uint32_t tx = i % tg.tw, ty = i / tg.tw;
        const uint32_t rx = tx * tg.x_dist, ry = ty * tg.y_dist;
        return (rx < fr.w && ry < fr.h) ? (info[(size_t)ry * fr.w + rx] == 1.0f ? 1u : 0u) : 0u;   // OOB imageLoad -> 0 (Q1)
    };
    unsigned long long flags = 0ull;
    uint32_t cnt = 0;
    if (in_regs) {
#pragma unroll 8
        for (uint32_t j = 0; j < i1 - i0; j++) flags |= (unsigned long long)flag_of(i0 + j) << j;
        cnt = (uint32_t)__popcll(flags);
    } else {
        for (uint32_t i = i0; i < i1; i++) cnt += flag_of(i);
    }
    uint32_t incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off);
        if ((int)lane >= off) incl += t;
    }
    if (lane == 63u) wsum[wave] = incl;
    __syncthreads();
    uint32_t woff = 0, total = 0;
    for (uint32_t w = 0; w < 16u; w++) {
        if (w < wave) woff += wsum[w];
        total += wsum[w];
    }
    uint32_t push_rank = woff + incl - cnt;        // scattered entries before i0
    for (uint32_t i = i0; i < i1; i++) {
        const uint32_t f = in_regs ? (uint32_t)(flags >> (i - i0)) & 1u : flag_of(i);
        scratch[i] = f;
        scratch[T + i] = f ? push_rank : (i - push_rank);
        push_rank += f;
    }
    if (tid == 0) {
        uint32_t head = ring[0], tail = ring[1];
        if (tg.ring_size > 0) {          // clear.comp:5-9
            head %= tg.ring_size;
            tail %= tg.ring_size;
        }
        scratch[2 * T] = total;
        scratch[2 * T + 1] = T - total;
        scratch[2 * T + 2] = head;
        scratch[2 * T + 3] = tail;
    }
}

// ------------------------------------------------------------------------------------------------ nrc/prep_train_rays.comp
// Phase A (k_prep_train): pop / trace / write train data; pushes are deferred into `pending` so that every pop sees the
// ring as it was at frame start.  Phase B (k_ring_push): apply pushes in linear order, advance head/tail.
// MODE 0: the whole of prep_train_rays.comp in one launch (pop / trace / write).  Long train paths (quirk Q2 fixed: up to 32 vertices) make
// that launch the longest of the frame -- a few hundred latency-bound waves, ~0.8 ms beside the camera kernels -- and its place in the
// frame graph (behind gen_rays(N), in front of ring_push(N), on ONE stream) makes the frames queue up behind it.  The frame graph then
// splits it: MODE 1 (k_train_start's work: tiny) takes the rays' start vertices from the images or the ring, writes them to `start`
// ([T][6] floats) and the training INPUT they determine; MODE 2 traces from `start` and writes the TARGET -- it touches neither the
// images nor the ring, so frame N's trace can run beside frame N + 1's on another stream.  Same arithmetic, same results, bit for bit.
//
// ST (self-training, include/nrc_hpm.h: nrc_config.self_train; MODE 0 and 2): every sample also writes its tail record at i * spp + s --
// the query at its last vertex (zeros: no tail) and {light.rgb, factor} (factor 0: the walk left the medium) -- for the tail inference
// and k_self_train_combine; the targets written here stay those without a tail.  The records' pointers are the one trailing argument
// `tail` of an ST instantiation; without ST the pack is empty, so k_prep_train<0|1|2> keep today's signature and code.
struct TailOut {
    float* query;        // [T * spp][5]
    float4* rec;         // [T * spp]: light.rgb, factor
};

template <int MODE, bool ST = false, class... Tail>
__global__ __launch_bounds__(256) void k_prep_train(DevScene sc, DevFrame fr, TrainGrid tg, const float4* __restrict__ origin,
                                                   const float4* __restrict__ dirs, const uint32_t* __restrict__ ring,
                                                   const uint32_t* __restrict__ scratch, float* __restrict__ train_in,
                                                   float* __restrict__ train_target, uint32_t rays_per_wave, float* __restrict__ start,
                                                   Tail... tail)
{
    static_assert(sizeof...(Tail) == (ST ? 1u : 0u), "k_prep_train: the tail records are the one trailing argument of ST");
    NRC_RAISE_WAVE_PRIORITY(4);
    __shared__ uint32_t s_occ[kOccMaxWords];
    const uint32_t* occ = load_occupancy(sc, s_occ);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t T = tg.tw * tg.th;
    uint32_t tx = blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u);
    uint32_t ty = blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3);
    // wave-uniform control flow with per-lane predicates, as in k_gen_rays: lanes beyond the train grid or done with their path stay in
    // the instruction stream and help with the last walks of every tracking loop (ratio_pairs)
    bool in_grid = tx < tg.tw && ty < tg.th;
    // Long train paths (quirk Q2 fixed: up to TRAIN_RAY_LENGTH = 32 vertices, three walks each): the launch is a few hundred waves whose
    // duration is the longest of their 64 paths, on a chip with 5 120 wave slots.  rays_per_wave < 64 gives a wave only that many rays (its
    // first lanes; the others help with the pair tails): the maximum runs over fewer paths, every ratio walk starts on lane pairs, and four
    // to eight times as many waves share the chip -- the same rays, the same targets, bit for bit (a ray's result does not depend on its lane).
    if (rays_per_wave < 64u) {
        const uint32_t i_lin = ((blockIdx.y * gridDim.x + blockIdx.x) * 4u + wave) * rays_per_wave + lane;
        in_grid = lane < rays_per_wave && i_lin < T;
        tx = in_grid ? i_lin % tg.tw : 0u;
        ty = in_grid ? i_lin / tg.tw : 0u;
    }
    const uint32_t i = in_grid ? ty * tg.tw + tx : 0u;
    CtxT<false> c{sc, 0.0f, 0u};
    c.occ = occ;
    // seed from TRAIN coordinates over the render size (quirk Q6, prep_train_rays.comp:108); sharded: global column
    const uint32_t gx = global_x(fr, tx);
    init_random(c, (float)gx * fr.inv_gw, (float)ty * fr.inv_gh, fr.random);
    V3 ro = v3(0, 0, 0);
    V3 rdir = normalize(v3(1.0f, 1.0f, 1.0f));
    if constexpr (MODE == 2) {
        if (in_grid) {
            const float* r = start + 6 * (size_t)i;
            ro = v3(r[0], r[1], r[2]);
            rdir = v3(r[3], r[4], r[5]);
        }
    } else {
        const bool scat = in_grid && scratch[i] != 0u;
        if (scat) {
            const size_t p = (size_t)(ty * tg.y_dist) * fr.w + tx * tg.x_dist;
            const float4 o = origin[p], d = dirs[p];
            ro = v3(o.x, o.y, o.z);
            rdir = v3(d.x, d.y, d.z);
        } else if (in_grid && tg.ring_size > 0) {
            const uint32_t tail = scratch[2 * T + 3];
            const float* r = reinterpret_cast<const float*>(ring + 2) + 6 * (size_t)((tail + scratch[T + i]) % tg.ring_size);
            ro = v3(r[0], r[1], r[2]);
            rdir = v3(r[3], r[4], r[5]);
        }
    }
    if constexpr (MODE == 1) {      // the start vertices and the input they determine; the trace is another launch's
        if (in_grid) {
            float* r = start + 6 * (size_t)i;
            r[0] = ro.x; r[1] = ro.y; r[2] = ro.z; r[3] = rdir.x; r[4] = rdir.y; r[5] = rdir.z;
            if (tg.ring_size > 0) {
                float q[5];
                nrc_query(sc, ro, rdir, q);
#pragma unroll
                for (int k = 0; k < 5; k++) train_in[5 * (size_t)i + k] = q[k];
            }
        }
        return;
    }
    V3 target = v3(0, 0, 0);
    for (uint32_t s = 0; s < tg.spp; s++) {
        V3 light = v3(0, 0, 0);
        V3 en, ex;
        find_entry_exit(c, ro, rdir, &en, &ex);      // (lanes beyond the grid march the default ray from the centre)
        V3 cur = en, dir = rdir;
        float factor = 1.0f;
        bool walking = in_grid;
        for (uint32_t k = 0; k < tg.ray_length; k++) {
            if (__ballot(walking) == 0ull) break;
            bool vexit = false;
            const V3 nc = delta_track<true>(c, cur, dir, &vexit, walking);
            cur = sel(walking, nc, cur);
            walking &= !vexit;
            factor = walking ? factor * 0.5f : factor;
            if (__ballot(walking) == 0ull) break;
            const V3 ts = trace_scene<true>(c, cur, dir, walking);
            if (walking) {
                light = add(light, mul(ts, factor));
                dir = new_ray_dir(c, dir, true);
            }
        }
        if constexpr (ST) {
            // a lane still walking has run all L vertices: it stands at its last scatter point with the direction after new_ray_dir
            if (in_grid && tg.ring_size > 0) {
                const TailOut to{tail...};
                const size_t r = (size_t)i * tg.spp + s;
                float q[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                if (walking) nrc_query(sc, cur, dir, q);
#pragma unroll
                for (int k = 0; k < 5; k++) to.query[5 * r + k] = q[k];
                to.rec[r] = make_float4(light.x, light.y, light.z, walking ? factor : 0.0f);
            }
        }
        target = add(target, light);
    }
    const float fs = (float)tg.spp;
    target = v3(target.x / fs, target.y / fs, target.z / fs);
    if (in_grid && tg.ring_size > 0) {
        if constexpr (MODE == 0) {
            float q[5];
            nrc_query(sc, ro, rdir, q);
#pragma unroll
            for (int k = 0; k < 5; k++) train_in[5 * (size_t)i + k] = q[k];
        }
        train_target[3 * (size_t)i + 0] = fminf(8.0f, target.x);
        train_target[3 * (size_t)i + 1] = fminf(8.0f, target.y);
        train_target[3 * (size_t)i + 2] = fminf(8.0f, target.z);
    }
}

// Self-training's training targets (include/nrc_hpm.h, nrc_config.self_train): the tail records of k_prep_train<MODE, true> and the cache's
// inference at the tails -> the targets, in the specified order and without contraction (this file is compiled with -ffp-contract=off).
// One thread per (train ray, channel).
__global__ __launch_bounds__(256) void k_self_train_combine(uint32_t T, uint32_t spp, const float4* __restrict__ rec, const float* __restrict__ y,
                                                           float* __restrict__ train_target)
{
    NRC_RAISE_WAVE_PRIORITY(4);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 3u * T) return;
    const uint32_t i = t / 3u, ch = t - 3u * i;
    float acc = 0.0f;
    for (uint32_t s = 0; s < spp; s++) {
        const size_t r = (size_t)i * spp + s;
        const float4 e = rec[r];
        const float light = ch == 0u ? e.x : (ch == 1u ? e.y : e.z);
        float u = light;
        if (e.w != 0.0f) u = light + e.w * fmaxf(0.0f, y[3 * r + ch]);      // (no tail: nothing added -- 0 * Inf would be NaN)
        acc = acc + u;
    }
    train_target[t] = fminf(8.0f, acc / (float)spp);
}

__global__ void k_ring_push(DevFrame fr, TrainGrid tg, const float4* __restrict__ origin, const float4* __restrict__ dirs,
                            uint32_t* __restrict__ ring, const uint32_t* __restrict__ scratch)
{
    NRC_RAISE_WAVE_PRIORITY(4);
    const uint32_t T = tg.tw * tg.th;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (tg.ring_size == 0) return;
    const uint32_t head = scratch[2 * T + 2], n_push = scratch[2 * T];
    // pushes are applied in linear train-index order; when a frame pushes more entries than the ring holds, a slot is written
    // several times and the last push in that order must win: only the final ring_size pushes are written at all
    if (i < T && scratch[i] != 0u && scratch[T + i] + tg.ring_size >= n_push) {
        const uint32_t tx = i % tg.tw, ty = i / tg.tw;
        const size_t p = (size_t)(ty * tg.y_dist) * fr.w + tx * tg.x_dist;
        const float4 o = origin[p], d = dirs[p];
        float* r = reinterpret_cast<float*>(ring + 2) + 6 * (size_t)((head + scratch[T + i]) % tg.ring_size);
        r[0] = o.x; r[1] = o.y; r[2] = o.z;
        r[3] = d.x; r[4] = d.y; r[5] = d.z;
    }
    if (i == 0) {
        ring[0] = head + scratch[2 * T];         // un-wrapped, as atomicAdd leaves them; wrapped next frame (clear.comp)
        ring[1] = scratch[2 * T + 3] + scratch[2 * T + 1];
    }
}

// ------------------------------------------------------------------------------------------------ nrc/render.comp
__global__ __launch_bounds__(256) void k_composite(DevFrame fr, uint32_t show_nrc, float blend_factor,
                                                  const float4* __restrict__ primary, const float* __restrict__ info,
                                                  const float* __restrict__ infer_out, float4* __restrict__ out_rgba,
                                                  uint32_t* __restrict__ live_count_reset)
{
    NRC_RAISE_WAVE_PRIORITY(2);
    // the frame's live-query list (DevFrame::live_list) has had its last reader -- this launch is ordered behind the frame's inference --
    // and the set's next gen_rays waits for this launch: the count is reset here instead of by a memset on the render stream
    if (live_count_reset != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *live_count_reset = 0u;
    uint32_t lx, y;
    if (!pixel_of_thread(fr, &lx, &y)) return;
    const size_t pix = (size_t)y * fr.w + lx, lin = query_index(fr.w, lx, y);
    const float4 p = primary[pix];
    float cr = p.x, cg = p.y, cb = p.z;
    if (show_nrc == 1u && info[pix] == 1.0f) {
        cr += fmaxf(0.0f, infer_out[3 * lin + 0]) * p.w;
        cg += fmaxf(0.0f, infer_out[3 * lin + 1]) * p.w;
        cb += fmaxf(0.0f, infer_out[3 * lin + 2]) * p.w;
    }
    const float4 prev = out_rgba[pix];
    const float ib = 1.0f - blend_factor;
    out_rgba[pix] = make_float4(blend_factor * cr + ib * prev.x, blend_factor * cg + ib * prev.y,
                                blend_factor * cb + ib * prev.z, blend_factor * 1.0f + ib * prev.w);
}

// tile-major (query_index) -> the reference's x * H + y order, C floats per query: what nrc_renderer_buffer hands out
// info (the frame's didScatter image, or nullptr): the entries of pixels that did not scatter are handed out as zeros -- the reference's
// zero-filled query buffer (NrcHpmRenderer.cu:1996); inside the renderer those slots are not written at all (DevFrame::skip_dead_queries,
// the live-query list)
__global__ __launch_bounds__(256) void k_query_layout(DevFrame fr, uint32_t C, const float* __restrict__ tiled, float* __restrict__ linear,
                                                     const float* __restrict__ info)
{
    uint32_t lx, y;
    if (!pixel_of_thread(fr, &lx, &y)) return;
    const size_t q = query_index(fr.w, lx, y), lin = (size_t)lx * fr.h + y;
    const bool dead = info != nullptr && info[(size_t)y * fr.w + lx] != 1.0f;
    for (uint32_t c = 0; c < C; c++) linear[lin * C + c] = dead ? 0.0f : tiled[q * C + c];
}

// ------------------------------------------------------------------------------------------------ ref/cmp1, norm, cmp2
// deterministic two-level reductions in fp64 instead of float atomics
constexpr int CMP_BLOCKS = 256;

__device__ __forceinline__ double block_sum(double v, double* sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    double r = sh[0];
    __syncthreads();
    return r;
}

// pass 1: per-block partials of {sq err, ref sum, own sum, valid count}; scratch[8 + 4*b + k]
__global__ __launch_bounds__(256) void k_compare_1(const float4* __restrict__ ref, const float4* __restrict__ own, uint32_t n,
                                                  double* __restrict__ scratch)
{
    __shared__ double sh[256];
    double se = 0, rs = 0, os = 0, cnt = 0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += CMP_BLOCKS * 256u) {
        const float4 r = ref[i], o = own[i];
        if (r.w == 0.0f) continue;            // cmp1.comp:32
        cnt += 1.0;
        const double dx = (double)o.x - r.x, dy = (double)o.y - r.y, dz = (double)o.z - r.z;
        se += dx * dx + dy * dy + dz * dz;
        rs += (double)r.x + r.y + r.z;
        os += (double)o.x + o.y + o.z;
    }
    se = block_sum(se, sh); rs = block_sum(rs, sh); os = block_sum(os, sh); cnt = block_sum(cnt, sh);
    if (threadIdx.x == 0) {
        double* p = scratch + 8 + 4 * blockIdx.x;
        p[0] = se; p[1] = rs; p[2] = os; p[3] = cnt;
    }
}
// norm.comp: fold partials -> scratch[0..3] = {mse, refMean, ownMean, count}
__global__ void k_compare_norm(double* __restrict__ scratch)
{
    if (threadIdx.x != 0) return;
    double se = 0, rs = 0, os = 0, cnt = 0;
    for (int b = 0; b < CMP_BLOCKS; b++) {
        const double* p = scratch + 8 + 4 * b;
        se += p[0]; rs += p[1]; os += p[2]; cnt += p[3];
    }
    const double inv = cnt > 0 ? 1.0 / (cnt * 3.0) : 0.0;
    scratch[0] = se * inv; scratch[1] = rs * inv; scratch[2] = os * inv; scratch[3] = cnt;
}
// cmp2.comp: variance of own around ownMean
__global__ __launch_bounds__(256) void k_compare_2(const float4* __restrict__ ref, const float4* __restrict__ own, uint32_t n,
                                                  double* __restrict__ scratch)
{
    __shared__ double sh[256];
    const double mean = scratch[2];
    double var = 0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += CMP_BLOCKS * 256u) {
        const float4 r = ref[i], o = own[i];
        if (r.w == 0.0f) continue;
        const double dx = o.x - mean, dy = o.y - mean, dz = o.z - mean;
        var += dx * dx + dy * dy + dz * dz;
    }
    var = block_sum(var, sh);
    if (threadIdx.x == 0) scratch[8 + 4 * CMP_BLOCKS + blockIdx.x] = var;
}
__global__ void k_compare_final(const double* __restrict__ scratch, float* __restrict__ result5)
{
    if (threadIdx.x != 0) return;
    double var = 0;
    for (int b = 0; b < CMP_BLOCKS; b++) var += scratch[8 + 4 * CMP_BLOCKS + b];
    const double cnt = scratch[3];
    const double inv = cnt > 0 ? 1.0 / (cnt * 3.0) : 0.0;
    result5[0] = (float)scratch[0];
    result5[1] = (float)scratch[1];
    result5[2] = (float)scratch[2];
    result5[3] = (float)(var * inv);
    result5[4] = (float)cnt;
}

// ---- the same metrics of a frame sharded over ranks ("reduce only the metrics"): pass 1 leaves the rank's RAW sums
// {sq err, ref sum, own sum, valid count} in scratch[0..3], the caller all-reduces them, k_compare_scale turns the global sums into
// {mse, refMean, ownMean, count}; pass 2 (k_compare_2 with the GLOBAL ownMean) leaves the rank's raw variance sum in scratch[4], the
// caller all-reduces it, k_compare_final_sharded writes the Result.
__global__ void k_compare_fold(double* __restrict__ scratch)
{
    if (threadIdx.x != 0) return;
    double se = 0, rs = 0, os = 0, cnt = 0;
    for (int b = 0; b < CMP_BLOCKS; b++) {
        const double* p = scratch + 8 + 4 * b;
        se += p[0]; rs += p[1]; os += p[2]; cnt += p[3];
    }
    scratch[0] = se; scratch[1] = rs; scratch[2] = os; scratch[3] = cnt;
}
__global__ void k_compare_scale(double* __restrict__ scratch)
{
    if (threadIdx.x != 0) return;
    const double cnt = scratch[3];
    const double inv = cnt > 0 ? 1.0 / (cnt * 3.0) : 0.0;
    scratch[0] *= inv; scratch[1] *= inv; scratch[2] *= inv;
}
__global__ void k_compare_fold_var(double* __restrict__ scratch)
{
    if (threadIdx.x != 0) return;
    double var = 0;
    for (int b = 0; b < CMP_BLOCKS; b++) var += scratch[8 + 4 * CMP_BLOCKS + b];
    scratch[4] = var;
}
__global__ void k_compare_final_sharded(const double* __restrict__ scratch, float* __restrict__ result5)
{
    if (threadIdx.x != 0) return;
    const double cnt = scratch[3];
    const double inv = cnt > 0 ? 1.0 / (cnt * 3.0) : 0.0;
    result5[0] = (float)scratch[0];
    result5[1] = (float)scratch[1];
    result5[2] = (float)scratch[2];
    result5[3] = (float)(scratch[4] * inv);
    result5[4] = (float)cnt;
}

// ---- a sharded frame put together again (nrc_tile: strips of 2^block_log2 columns dealt round-robin over `world` ranks):
// gathered = [world][h][max_lw] RGBA32F, rank r's local image padded to max_lw columns; out = [h][gw]
__global__ __launch_bounds__(256) void k_assemble_columns(const float4* __restrict__ gathered, uint32_t world, uint32_t block_log2, uint32_t gw, uint32_t h,
                                                         uint32_t max_lw, float4* __restrict__ out)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    const uint32_t gx = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y;
    if (gx >= gw) return;
    const uint32_t strip = gx >> block_log2, rank = strip % world, lstrip = strip / world;
    const uint32_t lx = (lstrip << block_log2) + (gx & ((1u << block_log2) - 1u));
    out[(size_t)y * gw + gx] = gathered[((size_t)rank * h + y) * max_lw + lx];
}
// local image [h][lw] -> [h][max_lw] (the all-gather moves equal blocks; a rank's last strip may be short or missing)
__global__ __launch_bounds__(256) void k_pad_columns(const float4* __restrict__ local, uint32_t lw, uint32_t h, uint32_t max_lw, float4* __restrict__ padded)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y;
    if (x >= max_lw) return;
    padded[(size_t)y * max_lw + x] = x < lw ? local[(size_t)y * lw + x] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// ------------------------------------------------------------------------------------------------ test hooks
__global__ void k_test_math(int fn, const float* __restrict__ a, const float* __restrict__ b, uint32_t n,
                            float* __restrict__ out, float* __restrict__ out2)
{
    fill_log_table();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f, c = 0.0f;
    switch (fn) {
    case 0: s = nrc_logf(a[i], s_log_tab); break;
    case 1: nrc_sincosf(a[i], &s, &c); break;
    case 2: s = nrc_acosf(a[i]); break;
    case 3: s = nrc_asinf(a[i]); break;
    case 4: s = nrc_atan2f(a[i], b[i]); break;
    case 5: s = nrc_acosf_clamped(a[i]); break;
    case 6: s = a[i] / b[i]; break;
    case 7: s = sqrtf(a[i]); break;
    case 8: s = (float)(_Float16)a[i]; break;
    case 9: { const f2 r = logf2(f2{a[i], b[i]}); s = r.x; c = r.y; break; }
    case 10: s = sqrt_rn_normal(a[i]); break;
    default: break;
    }
    out[i] = s;
    if (out2) out2[i] = c;
}

__global__ void k_test_rng(float u, float v, float r0, float r1, float r2, float r3, uint32_t n, float* __restrict__ out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const float fr[4] = {r0, r1, r2, r3};
    float state = random2(random2(u, v), random4(fr));
    out[0] = state;
    for (uint32_t i = 0; i < n; i++) {
        state = random1(state);
        out[1 + i] = state * 1.0f;
    }
}

// ------------------------------------------------------------------------------------------------ volume rebuild (set_volume)
// What renderer creation builds on the host (SceneDev::upload / build_occupancy / build_occupancy_bits in nrc_api.hip), built on the
// device from a volume already in device memory: the R8 density, the exact occupancy bits and the dilated 8^3-cell boxes, bit for bit.
// Three launches: k_vol_ingest (one streaming pass over the voxels), k_vol_cells (the dilation per 8^3 cell + the occupancy words),
// k_vol_rows (one workgroup: runs per cell row, an exclusive scan, the boxes in the host builder's order and their count).
//
// Neighbour sets of a voxel along one axis: bit 0 = the cell below is touched (the voxel is its cell's first and has a voxel below it),
// bit 1 = its own cell, bit 2 = the cell above (the cell's last voxel with a voxel above it): build_occupancy marks the cells of
// [v - 1, v + 1] clamped to the volume.
__device__ __forceinline__ uint32_t vol_axis_set(uint32_t v, uint32_t n)
{
    return 2u | ((v & 7u) == 0u && v > 0u ? 1u : 0u) | ((v & 7u) == 7u && v + 1u < n ? 4u : 0u);
}
// the 27-bit mask of the cells (cell + (dx, dy, dz), d in -1..1) a set of voxels touches: bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)
__device__ __forceinline__ uint32_t vol_touch_mask(uint32_t xs, uint32_t ys, uint32_t zs)
{
    uint32_t m = 0u;
#pragma unroll
    for (uint32_t dz = 0; dz < 3u; dz++)
#pragma unroll
        for (uint32_t dy = 0; dy < 3u; dy++)
            if (((zs >> dz) & 1u) && ((ys >> dy) & 1u)) m |= xs << (dz * 9u + dy * 3u);
    return m;
}
// NRC_VOLUME_F32 -> R8: uint8(v * 255) truncated (the reference's quantisation, src/Texture3D.cpp:106); v <= 0 and NaN -> 0, v >= 1 -> 255
__device__ __forceinline__ uint32_t vol_quantize(float v)
{
    if (!(v > 0.0f)) return 0u;
    if (v >= 1.0f) return 255u;
    return (uint32_t)(v * 255.0f);
}

// ---- voxel sources of k_vol_ingest: where a lane's four voxels come from, nothing else.  fetch<VEC>() fills q[k] with the quantised voxels
// x + k of one voxel row (idx: the first one's element in the volume, r = 8 * dz + dy: the row inside the lane's cell).  VEC (nx % 4 == 0
// and the source readable four elements at a time): returns the four as the word the kernel stores.  Otherwise no voxel of the volume
// with x + k >= nx is read (q[k] = 0) and the source stores the others itself through vol_scalar4.  stage(): lane t < 32 in front of the
// workgroup's barrier, for the workgroup's cell t (`in`: it exists); lane(): a lane's own state behind the barrier.
struct VolNoLane {};
__device__ __forceinline__ void vol_unpack4(uint32_t w, uint32_t q[4])
{
    q[0] = w & 255u; q[1] = (w >> 8) & 255u; q[2] = (w >> 16) & 255u; q[3] = w >> 24;
}
__device__ __forceinline__ uint32_t vol_pack4(const uint32_t q[4]) { return q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24); }
// the scalar path: voxel k = one(k) is read and stored only inside the volume (the load and its store under one guard: docs/MEASUREMENT_LOG.md)
template <typename One>
__device__ __forceinline__ uint32_t vol_scalar4(One one, uint32_t x, uint32_t nx, uint32_t q[4], uint8_t* __restrict__ row)
{
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        q[k] = 0u;
        if (x + k < nx) {
            q[k] = one(k);
            row[k] = (uint8_t)q[k];
        }
    }
    return 0u;
}

// a dense volume (nrc_renderer_set_volume): element idx + k.  VEC: src aligned to 4 elements (one 4- / 16-byte load per lane and row)
template <bool F32>
struct VolDense {
    const void* src;
    __device__ __forceinline__ void stage(uint32_t, size_t, bool) const {}
    __device__ __forceinline__ VolNoLane lane(uint32_t) const { return {}; }
    template <bool VEC>
    __device__ __forceinline__ uint32_t fetch(VolNoLane, size_t idx, uint32_t, uint32_t x, uint32_t nx, uint32_t q[4], uint8_t* __restrict__ density) const
    {
        if (!VEC)
            return vol_scalar4([&](uint32_t k) { return F32 ? vol_quantize(((const float*)src)[idx + k]) : (uint32_t)((const uint8_t*)src)[idx + k]; },
                               x, nx, q, density + idx);
        if (F32) {
            const float4 f = *(const float4*)((const float*)src + idx);
            q[0] = vol_quantize(f.x); q[1] = vol_quantize(f.y); q[2] = vol_quantize(f.z); q[3] = vol_quantize(f.w);
        } else vol_unpack4(*(const uint32_t*)((const uint8_t*)src + idx), q);
        return vol_pack4(q);
    }
};

// two R8 keys blended (nrc_renderer_set_volume_time): voxel = lerp_voxel(a, b, W), 0 < W < 256 (nrc_volume_keys.hpp; an end of the range is
// VolDense on one key).  VEC: both keys 4-byte aligned -- four bytes of each key per lane and row, blended as two pairs of 16-bit fields.
// The touch masks follow the blended voxel, not the keys.
struct VolLerp {
    const uint8_t *key_a, *key_b;
    uint32_t W;
    __device__ __forceinline__ void stage(uint32_t, size_t, bool) const {}
    __device__ __forceinline__ VolNoLane lane(uint32_t) const { return {}; }
    template <bool VEC>
    __device__ __forceinline__ uint32_t fetch(VolNoLane, size_t idx, uint32_t, uint32_t x, uint32_t nx, uint32_t q[4], uint8_t* __restrict__ density) const
    {
        if (!VEC) return vol_scalar4([&](uint32_t k) { return lerp_voxel(key_a[idx + k], key_b[idx + k], W); }, x, nx, q, density + idx);
        const uint32_t w = lerp_voxels4(*(const uint32_t*)(key_a + idx), *(const uint32_t*)(key_b + idx), W);
        vol_unpack4(w, q);
        return w;
    }
};

// the 8^3 bricks k_vol_brick_index named (nrc_renderer_set_volume_bricks; cell_brick[cell] = 1 + the brick, 0 = none): element
// 64 * dz + 8 * dy + dx of brick b, a lane's four are half a brick row (one 4- / 16-byte load when `aligned`: the brick base is aligned to 4
// elements, whatever nx is).  Voxels of a cell without a brick are 0: every voxel of the volume is written, nothing of the density's old
// contents is read or kept.  A brick voxel past the volume's edge is read and ignored.
template <bool F32>
struct VolBricks {
    const void* bricks;
    const uint32_t* cell_brick;
    uint32_t aligned;
    struct Lane { uint32_t b; size_t base; };
    // the brick ids of the workgroup's 32 cells: a function-local __shared__ has static storage, so stage() and lane() see one LDS array
    // per kernel instantiation (128 of its 256 bytes)
    static __device__ __forceinline__ uint32_t* lbrick() { __shared__ uint32_t l[32]; return l; }
    __device__ __forceinline__ void stage(uint32_t t, size_t cell, bool in) const { lbrick()[t] = in ? cell_brick[cell] : 0u; }
    __device__ __forceinline__ Lane lane(uint32_t t) const
    {
        const uint32_t b = lbrick()[(t & 63u) >> 1];
        return {b, b ? (size_t)(b - 1u) * 512u + 4u * (t & 1u) : 0u};
    }
    template <bool VEC>
    __device__ __forceinline__ uint32_t fetch(const Lane& ln, size_t idx, uint32_t r, uint32_t x, uint32_t nx, uint32_t q[4], uint8_t* __restrict__ density) const
    {
        uint32_t b[4] = {0u, 0u, 0u, 0u};
        if (ln.b) fetch_brick(ln.base + 8u * r, b);      // 64 * dz + 8 * dy: r = 8 * dz + dy
        if (!VEC) return vol_scalar4([&](uint32_t k) { return b[k]; }, x, nx, q, density + idx);
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) q[k] = b[k];
        return vol_pack4(q);
    }
    __device__ __forceinline__ void fetch_brick(size_t e, uint32_t q[4]) const
    {
        if (F32) {
            float f[4];
            if (aligned) {
                const float4 v = *(const float4*)((const float*)bricks + e);
                f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) f[k] = ((const float*)bricks)[e + k];
            }
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) q[k] = vol_quantize(f[k]);
        } else if (aligned) vol_unpack4(*(const uint32_t*)((const uint8_t*)bricks + e), q);
        else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) q[k] = (uint32_t)((const uint8_t*)bricks)[e + k];
        }
    }
};

// two keys held as bricks, blended (nrc_renderer_set_volume_key_bricks + set_volume_time, 0 < W < 256): `bricks` is the library's own R8
// array of every key's bricks (4-byte aligned at every half row), cell_a / cell_b the two keys' resident cell_brick indices (1 + the brick
// in that array, 0 = none).  A key without a brick in the lane's cell counts as 0 -- lerp_voxel(a, 0, W), not a copy of a -- and where
// neither key has one nothing is loaded.  Every voxel of the volume is written.
struct VolLerpBricks {
    const uint8_t* bricks;
    const uint32_t *cell_a, *cell_b;
    uint32_t W;
    struct Lane { uint32_t a, b; size_t base_a, base_b; };
    // both keys' brick ids of the workgroup's 32 cells (a first, b behind it): one LDS array per kernel instantiation, as VolBricks::lbrick()
    static __device__ __forceinline__ uint32_t* lbrick() { __shared__ uint32_t l[64]; return l; }
    __device__ __forceinline__ void stage(uint32_t t, size_t cell, bool in) const
    {
        lbrick()[t] = in ? cell_a[cell] : 0u;
        lbrick()[32u + t] = in ? cell_b[cell] : 0u;
    }
    __device__ __forceinline__ Lane lane(uint32_t t) const
    {
        const uint32_t c = (t & 63u) >> 1, a = lbrick()[c], b = lbrick()[32u + c];
        return {a, b, a ? (size_t)(a - 1u) * 512u + 4u * (t & 1u) : 0u, b ? (size_t)(b - 1u) * 512u + 4u * (t & 1u) : 0u};
    }
    template <bool VEC>
    __device__ __forceinline__ uint32_t fetch(const Lane& ln, size_t idx, uint32_t r, uint32_t x, uint32_t nx, uint32_t q[4], uint8_t* __restrict__ density) const
    {
        uint32_t wa = 0u, wb = 0u;      // one 4-byte load per present key and row (64 * dz + 8 * dy: r = 8 * dz + dy)
        if (ln.a) wa = *(const uint32_t*)(bricks + ln.base_a + 8u * r);
        if (ln.b) wb = *(const uint32_t*)(bricks + ln.base_b + 8u * r);
        if (!VEC) {
            uint32_t a[4], b[4];
            vol_unpack4(wa, a);
            vol_unpack4(wb, b);
            return vol_scalar4([&](uint32_t k) { return lerp_voxel(a[k], b[k], W); }, x, nx, q, density + idx);
        }
        const uint32_t w = (ln.a | ln.b) ? lerp_voxels4(wa, wb, W) : 0u;
        vol_unpack4(w, q);
        return w;
    }
};

// One workgroup per (32 cells along x) x (one 8x8 row of cells in y, z): 256 lanes, a lane owns four consecutive voxels of x (in one
// cell) in 16 of the 64 voxel rows.  Writes the density and every cell's 27-bit touch mask (the workgroup owns its cells: no global atomics).
// VEC: nx % 4 == 0 and what the source asks for (one 4-byte store per lane and row; otherwise the source stores, vol_scalar4).
template <typename Src, bool VEC>
__global__ __launch_bounds__(256) void k_vol_ingest(Src src, uint8_t* __restrict__ density, uint32_t* __restrict__ cell_mask, uint32_t nx, uint32_t ny,
                                                   uint32_t nz, uint32_t gx, uint32_t gy, uint32_t n_chunks)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    __shared__ uint32_t lmask[32];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = blockIdx.x % n_chunks, crow = blockIdx.x / n_chunks;
    const uint32_t cy = crow % gy, cz = crow / gy;
    const uint32_t cx = chunk * 32u + t;      // (t < 32: the workgroup's cells)
    const size_t cell = ((size_t)cz * gy + cy) * gx + cx;
    if (t < 32u) {
        lmask[t] = 0u;
        src.stage(t, cell, cx < gx);
    }
    __syncthreads();
    const uint32_t x = chunk * 256u + 4u * (t & 63u);
    uint32_t m = 0u;
    if (x < nx) {
        const auto ln = src.lane(t);
        uint32_t xs_q[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) xs_q[k] = x + k < nx ? vol_axis_set(x + k, nx) : 0u;
        for (uint32_t r = t >> 6; r < 64u; r += 4u) {
            const uint32_t y = cy * 8u + (r & 7u), z = cz * 8u + (r >> 3);
            if (y >= ny || z >= nz) continue;
            const size_t idx = ((size_t)z * ny + y) * nx + x;
            uint32_t q[4];
            const uint32_t w = src.template fetch<VEC>(ln, idx, r, x, nx, q, density);
            if (VEC) *(uint32_t*)(density + idx) = w;
            const uint32_t xs = (q[0] ? xs_q[0] : 0u) | (q[1] ? xs_q[1] : 0u) | (q[2] ? xs_q[2] : 0u) | (q[3] ? xs_q[3] : 0u);
            if (xs) m |= vol_touch_mask(xs, vol_axis_set(y, ny), vol_axis_set(z, nz));
        }
    }
    if (m) atomicOr(&lmask[(t & 63u) >> 1], m);
    __syncthreads();
    if (t < 32u && cx < gx) cell_mask[cell] = lmask[t];
}

// NRC_VOLUME_F32 key volumes -> R8 at upload (nrc_renderer_set_volume_keys): the bytes k_vol_ingest<VolDense<true>, ...> would write, nothing else
__global__ __launch_bounds__(256) void k_vol_quantize(const float* __restrict__ src, uint8_t* __restrict__ dst, size_t n)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    const size_t stride = (size_t)gridDim.x * 256u;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) dst[i] = (uint8_t)vol_quantize(src[i]);
}

// Blocks [0, n_cell_blocks): one lane per 8^3 cell -- occupied (build_occupancy's dilation) when a neighbour's touch mask, or its own,
// names it.  Blocks from n_cell_blocks on: one lane per bit of the exact occupancy table (cells of 2^occ_shift voxels, occ_shift >= 3:
// the OR of the own-cell bits of the 8^3 cells inside), a 64-bit ballot per wave = two whole words (occ_words is a multiple of four).
__global__ __launch_bounds__(256) void k_vol_cells(const uint32_t* __restrict__ cell_mask, uint8_t* __restrict__ cell_occ, uint32_t* __restrict__ occ_bits,
                                                  uint32_t gx, uint32_t gy, uint32_t gz, uint32_t n_cell_blocks, uint32_t occ_shift,
                                                  uint32_t occ_gx, uint32_t occ_gy, uint32_t occ_gz, uint32_t occ_words)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    if (blockIdx.x < n_cell_blocks) {
        const uint32_t i = blockIdx.x * 256u + threadIdx.x;
        if (i >= gx * gy * gz) return;
        const uint32_t cx = i % gx, cy = (i / gx) % gy, cz = i / (gx * gy);
        bool occ = false;
        for (int dz = -1; dz <= 1; dz++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int nx_ = (int)cx + dx, ny_ = (int)cy + dy, nz_ = (int)cz + dz;
                    if (nx_ < 0 || ny_ < 0 || nz_ < 0 || nx_ >= (int)gx || ny_ >= (int)gy || nz_ >= (int)gz) continue;
                    // the neighbour at +d touches this cell when it names the offset -d
                    const uint32_t bit = (uint32_t)((1 - dz) * 9 + (1 - dy) * 3 + (1 - dx));
                    occ = occ || ((cell_mask[((size_t)nz_ * gy + ny_) * gx + nx_] >> bit) & 1u);
                }
        cell_occ[i] = occ ? 1u : 0u;
        return;
    }
    const uint32_t j = (blockIdx.x - n_cell_blocks) * 256u + threadIdx.x;      // bit j of the occupancy table
    if (j >= occ_words * 32u) return;      // (whole waves: occ_words * 32 is a multiple of 128)
    bool set = false;
    if (j < occ_gx * occ_gy * occ_gz) {
        const uint32_t ox = j % occ_gx, oy = (j / occ_gx) % occ_gy, oz = j / (occ_gx * occ_gy);
        const uint32_t s = occ_shift - 3u;
        const uint32_t x1 = min((ox + 1u) << s, gx), y1 = min((oy + 1u) << s, gy), z1 = min((oz + 1u) << s, gz);
        for (uint32_t z = oz << s; z < z1 && !set; z++)
            for (uint32_t y = oy << s; y < y1 && !set; y++)
                for (uint32_t x = ox << s; x < x1; x++)
                    if ((cell_mask[((size_t)z * gy + y) * gx + x] >> 13) & 1u) { set = true; break; }
    }
    const unsigned long long b = __ballot(set);
    const uint32_t lane = threadIdx.x & 63u;
    if (lane == 0u) occ_bits[j >> 5] = (uint32_t)b;
    if (lane == 32u) occ_bits[j >> 5] = (uint32_t)(b >> 32);
}

// occupancy of the cells cx0 .. cx0 + 31 of a row of k_vol_cells' flags (bytes 0 / 1) as bits; cells past gx read 0.  words: gx % 4 == 0
// (rows start on 4-byte boundaries: eight independent word loads instead of 32 byte loads)
__device__ __forceinline__ uint32_t vol_row_bits(const uint8_t* __restrict__ row, uint32_t cx0, uint32_t gx, bool words)
{
    uint32_t m = 0u;
    if (words && cx0 + 32u <= gx) {
        const uint32_t* w = (const uint32_t*)(row + cx0);
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) {
            const uint32_t v = w[k];
            m |= ((v & 1u) | ((v >> 7) & 2u) | ((v >> 14) & 4u) | ((v >> 21) & 8u)) << (4u * k);
        }
    } else {
        for (uint32_t k = 0; k < 32u && cx0 + k < gx; k++) m |= (row[cx0 + k] ? 1u : 0u) << k;
    }
    return m;
}

// One workgroup: the cell rows (cy, cz) in chunks of 1024, a lane per row counts its runs of occupied cells, an exclusive scan over the
// chunk places them, and each lane writes its boxes -- z, then y, then x: build_occupancy's order, deterministically.  World coordinates
// with build_occupancy's fp64 expression (lo = -0.5 * size, vs = size / n: computed by the host the same way).
__global__ __launch_bounds__(1024) void k_vol_rows(const uint8_t* __restrict__ cell_occ, float* __restrict__ boxes, uint32_t* __restrict__ n_boxes,
                                                  uint32_t nx, uint32_t ny, uint32_t nz, uint32_t gx, uint32_t gy, uint32_t gz,
                                                  double lo_x, double lo_y, double lo_z, double vs_x, double vs_y, double vs_z)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    __shared__ uint32_t scan[1024];
    const uint32_t t = threadIdx.x, rows = gy * gz;
    const bool words = (gx & 3u) == 0u;
    uint32_t base = 0u;
    for (uint32_t r0 = 0; r0 < rows; r0 += 1024u) {
        const uint32_t r = r0 + t;
        const uint8_t* row = cell_occ + (size_t)r * gx;
        uint32_t cnt = 0u;
        if (r < rows) {
            uint32_t carry = 0u;      // the previous cell (bit 31 of the previous word)
            for (uint32_t cx0 = 0; cx0 < gx; cx0 += 32u) {
                const uint32_t m = vol_row_bits(row, cx0, gx, words);
                cnt += __builtin_popcount(m & ~((m << 1) | carry));      // run starts
                carry = m >> 31;
            }
        }
        scan[t] = cnt;
        __syncthreads();
        for (uint32_t off = 1u; off < 1024u; off <<= 1) {      // inclusive Hillis-Steele scan
            const uint32_t v = t >= off ? scan[t - off] : 0u;
            __syncthreads();
            scan[t] += v;
            __syncthreads();
        }
        const uint32_t total = scan[1023];
        if (cnt) {
            uint32_t k = base + scan[t] - cnt;
            const uint32_t cy = r % gy, cz = r / gy;
            const float y0 = (float)(lo_y + vs_y * (double)(8u * cy)), y1 = (float)(lo_y + vs_y * (double)min(8u * (cy + 1u), ny));
            const float z0 = (float)(lo_z + vs_z * (double)(8u * cz)), z1 = (float)(lo_z + vs_z * (double)min(8u * (cz + 1u), nz));
            uint32_t carry = 0u, run = 0u;
            for (uint32_t cx0 = 0; cx0 < gx; cx0 += 32u) {
                const uint32_t m = vol_row_bits(row, cx0, gx, words);
                uint32_t starts = m & ~((m << 1) | carry), ends = m & ~(m >> 1);
                // (bit 31 ends a run only when the next word's first cell is empty)
                if ((ends >> 31) && cx0 + 32u < gx && row[cx0 + 32u]) ends &= 0x7fffffffu;
                carry = m >> 31;
                while (starts | ends) {
                    const uint32_t b = __builtin_ctz(starts | ends), bit = 1u << b;
                    if (starts & bit) run = cx0 + b;
                    if (ends & bit) {
                        const uint32_t e = cx0 + b;
                        float* o = boxes + 6u * (size_t)k++;
                        o[0] = (float)(lo_x + vs_x * (double)(8u * run)); o[1] = y0; o[2] = z0;
                        o[3] = (float)(lo_x + vs_x * (double)min(8u * (e + 1u), nx)); o[4] = y1; o[5] = z1;
                    }
                    starts &= ~bit; ends &= ~bit;
                }
            }
        }
        base += total;
        __syncthreads();      // (scan[] is rewritten by the next chunk)
    }
    if (t == 0u) *n_boxes = base;
}

// ---- the same rebuild from a list of 8^3 bricks (nrc_renderer_set_volume_bricks): k_vol_brick_index runs in front of k_vol_ingest, whose
// VolBricks source reads what it wrote; k_vol_cells and k_vol_rows run behind them unchanged.
//
// One lane per brick: cell_brick[cell] = 1 + the highest index of the bricks that name the cell (cleared to 0 = none by the caller).
// atomicMax on integers: which brick wins does not depend on the order the lanes run in.  An origin that is not a multiple of 8 or
// lies outside the volume is ignored (a device list cannot be checked by the host without a wait).  first: the number of brick 0 of
// this list (0, or where a key's slice starts in the concatenated array of nrc_renderer_set_volume_key_bricks).
__global__ __launch_bounds__(256) void k_vol_brick_index(const int32_t* __restrict__ origins, uint32_t n_bricks, uint32_t* __restrict__ cell_brick,
                                                        uint32_t nx, uint32_t ny, uint32_t nz, uint32_t gx, uint32_t gy, uint32_t first)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_bricks) return;
    const int32_t x0 = origins[3u * (size_t)i], y0 = origins[3u * (size_t)i + 1u], z0 = origins[3u * (size_t)i + 2u];
    if ((x0 | y0 | z0) < 0 || ((x0 | y0 | z0) & 7) != 0) return;
    if ((uint32_t)x0 >= nx || (uint32_t)y0 >= ny || (uint32_t)z0 >= nz) return;
    atomicMax(&cell_brick[((size_t)((uint32_t)z0 >> 3) * gy + ((uint32_t)y0 >> 3)) * gx + ((uint32_t)x0 >> 3)], first + i + 1u);
}

// ------------------------------------------------------------------------------------------------ the denoise filter (nrc_denoise.hpp)
// The guide's two floats {alpha, z_front} of every pixel, packed once per call: the passes read 8 bytes per tap instead of 16.
__global__ __launch_bounds__(256) void k_denoise_pack(const float4* __restrict__ aov, float2* __restrict__ guide, uint32_t n)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 a = aov[i];
    guide[i] = make_float2(a.x, a.z);
}

// One pass: a lane per pixel, a workgroup per 32 x 8 tile (a wave covers two rows of 32 pixels: a tap is two 512-byte row segments of
// colour per wave).  Every tap inside the image is loaded straight from memory under the lane's own predicate -- nothing is read outside the
// image, nothing is staged: the 25 taps of neighbouring lanes overlap and are served by the L1 / L2.  in and out never alias (launch_denoise).
struct DenoiseDevImage {
    const float4* __restrict__ c;
    const float2* __restrict__ g;
    uint32_t w;
    __device__ DenoiseRgba colour(int x, int y) const
    {
        const float4 v = c[(size_t)y * w + (uint32_t)x];
        return DenoiseRgba{v.x, v.y, v.z, v.w};
    }
    __device__ DenoiseGuide guide(int x, int y) const
    {
        const float2 v = g[(size_t)y * w + (uint32_t)x];
        return DenoiseGuide{v.x, v.y};
    }
};
__global__ __launch_bounds__(256) void k_denoise_pass(const float4* __restrict__ in, const float2* __restrict__ guide, float4* __restrict__ out,
                                                     uint32_t w, uint32_t h, DenoisePass ps)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    const uint32_t x = blockIdx.x * 32u + (threadIdx.x & 31u), y = blockIdx.y * 8u + (threadIdx.x >> 5);
    if (x >= w || y >= h) return;
    const DenoiseRgba r = denoise_pixel(DenoiseDevImage{in, guide, w}, ps, (int)w, (int)h, (int)x, (int)y);
    out[(size_t)y * w + x] = make_float4(r.r, r.g, r.b, r.a);
}

// ------------------------------------------------------------------------------------------------ reprojection (nrc_reproject.hpp)
// A lane per pixel of the current view, a workgroup per 32 x 8 tile, as k_denoise_pass.  The lane streams its own colour and AOV and gathers
// the up to four history taps its point projects onto -- neighbours, so a wave's gathers of colour, AOV and count fall into a few cache
// lines.  Every tap is loaded straight from memory under the lane's own predicate: nothing is read outside the images, nothing is staged.
// The outputs never alias an input (launch_reproject).  The history guide is read as the AOV's own float4: it is not packed.
struct ReprojectDevImage {
    const float4* __restrict__ c;
    const float4* __restrict__ g;
    const float4* __restrict__ hc;
    const float4* __restrict__ hg;
    const float* __restrict__ hn;
    uint32_t w;
    __device__ size_t at(int x, int y) const { return (size_t)y * w + (uint32_t)x; }
    __device__ ReprojectRgba colour(int x, int y) const
    {
        const float4 v = c[at(x, y)];
        return ReprojectRgba{v.x, v.y, v.z, v.w};
    }
    __device__ ReprojectGuide guide(int x, int y) const
    {
        const float4 v = g[at(x, y)];
        return ReprojectGuide{v.x, v.z, v.w};
    }
    __device__ ReprojectRgba hist_colour(int x, int y) const
    {
        const float4 v = hc[at(x, y)];
        return ReprojectRgba{v.x, v.y, v.z, v.w};
    }
    __device__ ReprojectGuide hist_guide(int x, int y) const
    {
        const float4 v = hg[at(x, y)];
        return ReprojectGuide{v.x, v.z, v.w};
    }
    __device__ float hist_count(int x, int y) const { return hn[at(x, y)]; }
};
__global__ __launch_bounds__(256) void k_reproject(const float4* __restrict__ hist_rgba, const float* __restrict__ hist_n, const float4* __restrict__ hist_aov,
                                                  const float4* __restrict__ rgba, const float4* __restrict__ aov, float4* __restrict__ out,
                                                  float* __restrict__ out_n, uint32_t w, uint32_t h, ReprojectView view)
{
    NRC_RAISE_WAVE_PRIORITY(16);
    const uint32_t x = blockIdx.x * 32u + (threadIdx.x & 31u), y = blockIdx.y * 8u + (threadIdx.x >> 5);
    if (x >= w || y >= h) return;
    const ReprojectOut r = reproject_pixel(ReprojectDevImage{rgba, aov, hist_rgba, hist_aov, hist_n, w}, view, (int)w, (int)h, (int)x, (int)y);
    out[(size_t)y * w + x] = make_float4(r.c.r, r.c.g, r.c.b, r.c.a);
    out_n[(size_t)y * w + x] = r.n;
}

}  // namespace

// ================================================================================================ launchers
static dim3 pixel_grid(uint32_t w, uint32_t h) { return dim3(ceil_div(w, 16), ceil_div(h, 16)); }
// k_gen_rays / k_mc_render: one 8x8 pixel tile per wave, see pixel_of_wave_tile
static dim3 wave_tile_grid(uint32_t w, uint32_t h) { return dim3(camera_row_blocks(w) * ceil_div(h, 8)); }

static int g_host_raise_wave_priority = 1;      // (integrator_set_wave_priority_raise)

void launch_gen_rays(const DevScene& sc, const DevCamera& cam, const DevFrame& fr, uint32_t primary_ray_length,
                     float primary_ray_prob, float* primary, float* info, float* origin, float* dir, float* infer_in,
                     unsigned long long* fetch_counter, const TrainGrid& tg, bool full_vertex_images, hipStream_t s)
{
    auto kernel = fetch_counter ? k_gen_rays<true> : k_gen_rays<false>;      // the look-up counter exists only in measurement launches
#ifdef NRC_LOOP_PROFILE
    kernel = k_gen_rays<true>;      // (the profiling build's per-pixel look-up counts, tools/lane_model.py)
#endif
    dim3 grid = wave_tile_grid(fr.w, fr.h);
    if (fr.hot_front != 0u) grid.x += kHotTilesMax / CAMERA_WAVES_PER_BLOCK;
    DevFrame fa = fr;
    fa.raise_priority = (g_host_raise_wave_priority != 0 && fr.camera_priority_low == 0u) ? 1u : 0u;
    // (launch_last: the frame's start / "gen_rays done" events ride on the launch when the frame graph armed them -- nrc_common.hpp)
    launch_last(kernel, grid, dim3(64 * CAMERA_WAVES_PER_BLOCK), 0u, s, sc, cam, fa,
                primary_ray_length, primary_ray_prob, (float4*)primary, info, (float4*)origin, (float4*)dir, infer_in,
                fetch_counter, tg, full_vertex_images ? 1 : 0);
    NRC_HIP(hipGetLastError());
}

static uint32_t ray_aov_raise(const DevFrame& fr) { return (g_host_raise_wave_priority != 0 && fr.camera_priority_low == 0u) ? 1u : 0u; }
// the frame of the AOV kernels: the view's geometry and mask; the default tile order, no hot tiles, no cost samples
static DevFrame aov_frame(const DevFrame& fr)
{
    DevFrame fa = fr;
    fa.tile_order = nullptr;
    fa.tile_cost = nullptr;
    fa.hot_front = fa.hot_n = 0u;
    fa.raise_priority = ray_aov_raise(fr);
    return fa;
}
void launch_view_aov(const DevScene& sc, const DevCamera& cam, const DevFrame& fr, float* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_view_aov, wave_tile_grid(fr.w, fr.h), dim3(64 * CAMERA_WAVES_PER_BLOCK), 0, s, sc, cam, aov_frame(fr), (float4*)out);
    NRC_HIP(hipGetLastError());
}

// the ray and the deep AOV.  A launcher per source owns that source's checks and grid; the launch itself is the same for all of them.
// fr: the renderer's frame -- the view's geometry and mask for the depth source, the priority switch for all
template <class Src, class Out>
static void launch_ray_aov(const DevScene& sc, dim3 grid, const Src& src, const Out& out, hipStream_t s)
{
    hipLaunchKernelGGL((k_ray_aov<Src, Out>), grid, dim3(64 * CAMERA_WAVES_PER_BLOCK), 0, s, sc, src, out);
    NRC_HIP(hipGetLastError());
}
// n: the source's rays (the stride of a deep plane); deep: null for the flat result alone, which then goes to src.out
template <class Src>
static void launch_ray_aov(const DevScene& sc, dim3 grid, const Src& src, size_t n, const AovPlanes* deep, hipStream_t s)
{
    if (deep == nullptr) {
        if (((uintptr_t)src.out) & 15u) fail("ray AOV: out must be 16-byte aligned");
        return launch_ray_aov(sc, grid, src, FlatOut{}, s);
    }
    if (deep->n_levels == 0u || deep->n_levels > kAovDeepMaxLevels) fail("deep AOV: the number of levels must be 1 .. 32");
    if (((uintptr_t)src.out) & 15u) fail("deep AOV: flat must be 16-byte aligned");
    DeepOut d{deep->z, n, deep->n_levels, {}};
    for (uint32_t k = 0; k < deep->n_levels; k++) d.levels.v[k] = deep->levels[k];
    launch_ray_aov(sc, grid, src, d, s);
}
static std::string aov_name(const AovPlanes* deep) { return deep != nullptr ? "deep AOV" : "ray AOV"; }

void launch_ray_aov_list(const DevScene& sc, const DevFrame& fr, size_t n, const float* rays, float* out, const AovPlanes* deep, hipStream_t s)
{
    const size_t blocks = (n + 64u * CAMERA_WAVES_PER_BLOCK - 1u) / (64u * CAMERA_WAVES_PER_BLOCK);
    if (blocks == 0u) return;
    if (blocks > 0x7fffffffull) fail(aov_name(deep) + ": too many rays for one launch");
    if (deep == nullptr) {
        if ((((uintptr_t)rays) | ((uintptr_t)out)) & 15u) fail("ray AOV: rays and out must be 16-byte aligned");
    } else if (((uintptr_t)rays) & 15u) fail("deep AOV: rays must be 16-byte aligned");
    launch_ray_aov(sc, dim3((uint32_t)blocks), RayList{(const float4*)rays, (float4*)out, n, ray_aov_raise(fr)}, n, deep, s);
}
void launch_ray_aov_view_depth(const DevScene& sc, const DevCamera& cam, const DevFrame& fr, const float* depth, float* out, const AovPlanes* deep,
                               hipStream_t s)
{
    launch_ray_aov(sc, wave_tile_grid(fr.w, fr.h), ViewDepth{cam, aov_frame(fr), depth, (float4*)out, ray_aov_raise(fr)}, (size_t)fr.w * fr.h, deep, s);
}
void launch_ray_aov_ortho(const DevScene& sc, const DevFrame& fr, const AovOrthoView& view, uint32_t w, uint32_t h, float* out, const AovPlanes* deep,
                          hipStream_t s)
{
    if (w == 0u || h == 0u) return;
    const uint64_t tiles = (uint64_t)ceil_div(w, 8) * ceil_div(h, 8);
    const uint64_t blocks = (tiles + CAMERA_WAVES_PER_BLOCK - 1u) / CAMERA_WAVES_PER_BLOCK;
    if (tiles > 0x7fffffffull) fail(aov_name(deep) + ": the orthographic view is too large for one launch");      // (the kernel numbers its tiles in 32 bits)
    launch_ray_aov(sc, dim3((uint32_t)blocks), OrthoView{view, w, h, (float4*)out, ray_aov_raise(fr)}, (size_t)w * h, deep, s);
}

uint32_t camera_slots(uint32_t w, uint32_t h) { return camera_row_blocks(w) * CAMERA_WAVES_PER_BLOCK * ceil_div(h, 8); }

void launch_tile_order(const uint32_t* cost, uint32_t n_slots, uint32_t* order, uint32_t w, hipStream_t s, uint32_t xcd_window, uint32_t workgroups_in_front)
{
    const uint32_t row_len = camera_row_blocks(w) * CAMERA_WAVES_PER_BLOCK;
    // (the sort's last launch carries the "order ready" event when the frame graph armed one -- nrc_common.hpp, LaunchTail)
    const bool xcd = xcd_window != 0u && CAMERA_WAVES_PER_BLOCK == 4u && n_slots % row_len == 0u;
    if (!xcd) launch_last(k_tile_order, dim3(1), dim3(1024), 0u, s, cost, n_slots, order);
    else {
        hipLaunchKernelGGL(k_tile_order, dim3(1), dim3(1024), 0, s, cost, n_slots, order);
        const uint32_t S = 32u * std::min(32u, xcd_window);
        launch_last(k_tile_order_xcd, dim3((n_slots + workgroups_in_front * 4u + S - 1u) / S), dim3(S), 0u, s, order, n_slots, row_len, workgroups_in_front);
    }
    NRC_HIP(hipGetLastError());
}

uint32_t tile_mask_words(uint32_t w, uint32_t h) { return (ceil_div(w, 8) * ceil_div(h, 8) + 31u) / 32u + 1u; }

void launch_tile_mask(const BoxList& b, const DevProjView& pv, const DevFrame& fr, uint32_t* mask, float* far, hipStream_t s)
{
    NRC_HIP(hipMemsetAsync(mask, 0, (size_t)tile_mask_words(fr.w, fr.h) * 4, s));
    NRC_HIP(hipMemsetAsync(far, 0, (size_t)ceil_div(fr.w, 8) * ceil_div(fr.h, 8) * 4, s));
    if (b.grid == 0) return;
    hipLaunchKernelGGL(k_tile_mask, dim3(ceil_div(b.grid, 256)), dim3(256), 0, s, b.boxes, b.n_host, b.n_dev, pv, fr, mask, far);
    NRC_HIP(hipGetLastError());
}

void launch_tile_mask_tiles(const BoxList& b, const DevProjView& pv, const DevFrame& fr, void* rects, uint32_t* mask, float* far, hipStream_t s)
{
    NRC_HIP(hipMemsetAsync(far, 0, (size_t)ceil_div(fr.w, 8) * ceil_div(fr.h, 8) * 4, s));      // (the far bounds are a maximum: they start from 0)
    if (b.grid > 0) {      // (no box: k_tile_mask_words alone writes an all-clear mask)
        hipLaunchKernelGGL(k_tile_rects, dim3(ceil_div(b.grid, 256)), dim3(256), 0, s, b.boxes, b.n_host, b.n_dev, pv, fr, (unsigned long long*)rects,
                           far);
        NRC_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_tile_mask_words, dim3(ceil_div(tile_mask_words(fr.w, fr.h), 4)), dim3(256), 0, s, (const unsigned long long*)rects,
                       b.grid > 0 ? b.n_host : 0u, b.grid > 0 ? b.n_dev : nullptr, fr, mask);
    NRC_HIP(hipGetLastError());
}

uint32_t volume_box_capacity(uint32_t nx, uint32_t ny, uint32_t nz)
{
    const uint32_t gx = ceil_div(nx, 8), gy = ceil_div(ny, 8), gz = ceil_div(nz, 8);
    return gy * gz * ceil_div(gx, 2);      // runs are separated by at least one empty cell
}

size_t volume_scratch_bytes(uint32_t nx, uint32_t ny, uint32_t nz)
{
    return (size_t)ceil_div(nx, 8) * ceil_div(ny, 8) * ceil_div(nz, 8) * 5;
}

static void launch_volume_cells_rows(const VolumeRebuild& v, void* scratch, hipStream_t s);

// the rebuild's three launches from a voxel source; vec: nx % 4 == 0 and the source's own condition (k_vol_ingest)
template <typename Src>
static void launch_volume_ingest(const Src& src, bool vec, const VolumeRebuild& v, void* scratch, hipStream_t s)
{
    const uint32_t gx = ceil_div(v.nx, 8), gy = ceil_div(v.ny, 8), gz = ceil_div(v.nz, 8);
    const uint32_t n_chunks = ceil_div(gx, 32);
    auto ingest = vec ? k_vol_ingest<Src, true> : k_vol_ingest<Src, false>;
    hipLaunchKernelGGL(ingest, dim3(n_chunks * gy * gz), dim3(256), 0, s, src, v.density, (uint32_t*)scratch, v.nx, v.ny, v.nz, gx, gy, n_chunks);
    NRC_HIP(hipGetLastError());
    launch_volume_cells_rows(v, scratch, s);
}

void launch_volume_rebuild(const void* src, int format, const VolumeRebuild& v, void* scratch, hipStream_t s)
{
    const bool f32 = format == NRC_VOLUME_F32, vec = v.nx % 4 == 0 && (uintptr_t)src % (f32 ? 16 : 4) == 0;
    if (f32) launch_volume_ingest(VolDense<true>{src}, vec, v, scratch, s);
    else launch_volume_ingest(VolDense<false>{src}, vec, v, scratch, s);
}

void launch_volume_quantize(const float* src, uint8_t* dst, size_t n, hipStream_t s)
{
    if (n == 0) return;
    const size_t blocks = std::min<size_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(k_vol_quantize, dim3((uint32_t)blocks), dim3(256), 0, s, src, dst, n);
    NRC_HIP(hipGetLastError());
}

void launch_volume_rebuild_lerp(const uint8_t* key_a, const uint8_t* key_b, uint32_t W, const VolumeRebuild& v, void* scratch, hipStream_t s)
{
    if (W == 0u || W >= 256u) {      // one key as it is (key_b may be null at W == 0: the last key has no successor)
        launch_volume_rebuild(W == 0u ? key_a : key_b, NRC_VOLUME_U8, v, scratch, s);
        return;
    }
    const bool vec = v.nx % 4 == 0 && (uintptr_t)key_a % 4 == 0 && (uintptr_t)key_b % 4 == 0;
    launch_volume_ingest(VolLerp{key_a, key_b, W}, vec, v, scratch, s);
}

size_t volume_brick_index_bytes(uint32_t nx, uint32_t ny, uint32_t nz)
{
    return (size_t)ceil_div(nx, 8) * ceil_div(ny, 8) * ceil_div(nz, 8) * 4;
}

void launch_volume_brick_index(const int32_t* origins, uint32_t n_bricks, uint32_t first, uint32_t* cell_brick, uint32_t nx, uint32_t ny, uint32_t nz,
                               hipStream_t s)
{
    NRC_HIP(hipMemsetAsync(cell_brick, 0, volume_brick_index_bytes(nx, ny, nz), s));
    if (n_bricks == 0) return;
    hipLaunchKernelGGL(k_vol_brick_index, dim3(ceil_div(n_bricks, 256)), dim3(256), 0, s, origins, n_bricks, cell_brick, nx, ny, nz, ceil_div(nx, 8),
                       ceil_div(ny, 8), first);
    NRC_HIP(hipGetLastError());
}

void launch_volume_rebuild_indexed(const uint8_t* bricks, const uint32_t* cell_brick, const VolumeRebuild& v, void* scratch, hipStream_t s)
{
    launch_volume_ingest(VolBricks<false>{bricks, cell_brick, 1u}, v.nx % 4 == 0, v, scratch, s);
}

void launch_volume_rebuild_lerp_bricks(const uint8_t* bricks, const uint32_t* cell_a, const uint32_t* cell_b, uint32_t W, const VolumeRebuild& v,
                                       void* scratch, hipStream_t s)
{
    if (W == 0u || W >= 256u) {      // one key as it is, through its resident index (cell_b may be null at W == 0: the last key has no successor)
        launch_volume_rebuild_indexed(bricks, W == 0u ? cell_a : cell_b, v, scratch, s);
        return;
    }
    launch_volume_ingest(VolLerpBricks{bricks, cell_a, cell_b, W}, v.nx % 4 == 0, v, scratch, s);
}

void launch_volume_rebuild_bricks(const int32_t* origins, const void* bricks, uint32_t n_bricks, int format, const VolumeRebuild& v, void* scratch,
                                  uint32_t* brick_index, hipStream_t s)
{
    launch_volume_brick_index(origins, n_bricks, 0u, brick_index, v.nx, v.ny, v.nz, s);
    const bool f32 = format == NRC_VOLUME_F32, vec = v.nx % 4 == 0;
    const uint32_t aligned = (uintptr_t)bricks % (f32 ? 16 : 4) == 0 ? 1u : 0u;
    if (f32) launch_volume_ingest(VolBricks<true>{bricks, brick_index, aligned}, vec, v, scratch, s);
    else launch_volume_ingest(VolBricks<false>{bricks, brick_index, aligned}, vec, v, scratch, s);
}

// the two launches behind k_vol_ingest: scratch holds the cells' touch masks, then their occupancy flags
static void launch_volume_cells_rows(const VolumeRebuild& v, void* scratch, hipStream_t s)
{
    const uint32_t gx = ceil_div(v.nx, 8), gy = ceil_div(v.ny, 8), gz = ceil_div(v.nz, 8);
    const size_t cells = (size_t)gx * gy * gz;
    uint32_t* cell_mask = (uint32_t*)scratch;
    uint8_t* cell_occ = (uint8_t*)(cell_mask + cells);
    const uint32_t cell_blocks = ceil_div((uint32_t)cells, 256), occ_blocks = ceil_div(v.occ_words * 32u, 256);
    hipLaunchKernelGGL(k_vol_cells, dim3(cell_blocks + occ_blocks), dim3(256), 0, s, (const uint32_t*)cell_mask, cell_occ, v.occ_bits, gx, gy, gz,
                       cell_blocks, v.occ_shift, v.occ_gx, v.occ_gy, v.occ_gz, v.occ_words);
    NRC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_vol_rows, dim3(1), dim3(1024), 0, s, (const uint8_t*)cell_occ, v.boxes, v.n_boxes, v.nx, v.ny, v.nz, gx, gy, gz,
                       v.lo[0], v.lo[1], v.lo[2], v.vs[0], v.vs[1], v.vs[2]);
    NRC_HIP(hipGetLastError());
}

void launch_flight_table(float* table, hipStream_t s)
{
    hipLaunchKernelGGL(k_flight_table, dim3(kFlightStates / 256u), dim3(256), 0, s, table);
    NRC_HIP(hipGetLastError());
}

void launch_flight_select(const float* table, float lambda, uint32_t* count_and_list, uint32_t* bits, hipStream_t s)
{
    NRC_HIP(hipMemsetAsync(count_and_list, 0, (1 + kFlightListMax) * 4, s));
    hipLaunchKernelGGL(k_flight_select, dim3(kFlightStates / 256u), dim3(256), 0, s, table, lambda, count_and_list, bits);
    NRC_HIP(hipGetLastError());
}

void launch_mc_render(const DevScene& sc, const DevCamera& cam, const DevFrame& fr, uint32_t path_length,
                      float blend_factor, float* out_rgba, float* info, unsigned long long* fetch_counter, hipStream_t s)
{
    dim3 grid = wave_tile_grid(fr.w, fr.h);
    if (fr.hot_front != 0u) grid.x += kHotTilesMax / CAMERA_WAVES_PER_BLOCK;
    DevFrame fa = fr;
    fa.raise_priority = (g_host_raise_wave_priority != 0 && fr.camera_priority_low == 0u) ? 1u : 0u;
    hipLaunchKernelGGL(fetch_counter ? k_mc_render<true> : k_mc_render<false>, grid, dim3(64 * CAMERA_WAVES_PER_BLOCK), 0, s, sc,
                       cam, fa, path_length, blend_factor, (float4*)out_rgba, info, fetch_counter);
    NRC_HIP(hipGetLastError());
}

void launch_prep_train(const DevScene& sc, const DevFrame& fr, const TrainGrid& tg, const float* info, const float* origin,
                       const float* dir, uint32_t* ring, uint32_t* scratch, float* train_in, float* train_target,
                       hipStream_t s, float* start, float* tail_query, float* tail_rec)
{
    const uint32_t T = tg.tw * tg.th;
    hipLaunchKernelGGL(k_train_scan, dim3(1), dim3(1024), 0, s, fr, tg, info, ring, scratch);
    NRC_HIP(hipGetLastError());
    // (one 8x8 block of the train grid per wave for the reference's single-vertex targets; 32 rays per wave for long paths: k_prep_train)
    // (measured on the bench frame with train ray length 32: 64 / 32 / 16 / 8 rays per wave -> 2 309 / 2 412 / 2 367 / 2 347 Msamples/s)
    const uint32_t rpw = train_paths_are_long(tg) ? 32u : 64u;
    const dim3 grid = rpw >= 64u ? pixel_grid(tg.tw, tg.th) : dim3(ceil_div(T, 4u * rpw), 1);
    if (start == nullptr && tail_query != nullptr)      // self-training: the same launch, plus the tail records
        hipLaunchKernelGGL((k_prep_train<0, true, TailOut>), grid, dim3(256), 0, s, sc, fr, tg, (const float4*)origin, (const float4*)dir, (const uint32_t*)ring,
                           (const uint32_t*)scratch, train_in, train_target, rpw, (float*)nullptr, TailOut{tail_query, (float4*)tail_rec});
    else if (start == nullptr)
        hipLaunchKernelGGL(k_prep_train<0>, grid, dim3(256), 0, s, sc, fr, tg, (const float4*)origin, (const float4*)dir, (const uint32_t*)ring,
                           (const uint32_t*)scratch, train_in, train_target, rpw, (float*)nullptr);
    else      // the split frame graph: start vertices + inputs here, the trace by launch_train_trace on a stream of its own
        hipLaunchKernelGGL(k_prep_train<1>, pixel_grid(tg.tw, tg.th), dim3(256), 0, s, sc, fr, tg, (const float4*)origin, (const float4*)dir,
                           (const uint32_t*)ring, (const uint32_t*)scratch, train_in, train_target, 64u, start);
    NRC_HIP(hipGetLastError());
    launch_last(k_ring_push, dim3(ceil_div(T, 256)), dim3(256), 0u, s, fr, tg, (const float4*)origin,
                (const float4*)dir, ring, (const uint32_t*)scratch);
    NRC_HIP(hipGetLastError());
}

bool train_paths_are_long(const TrainGrid& tg) { return tg.ray_length * tg.spp >= 4u; }

// the trace of the split frame graph (k_prep_train<2>): from the start vertices launch_prep_train(..., start) left, to the training targets
void launch_train_trace(const DevScene& sc, const DevFrame& fr, const TrainGrid& tg, const float* start, float* train_target, hipStream_t s,
                        float* tail_query, float* tail_rec)
{
    const uint32_t T = tg.tw * tg.th;
    const uint32_t rpw = 32u;
    if (tail_query != nullptr) {
        launch_last((k_prep_train<2, true, TailOut>), dim3(ceil_div(T, 4u * rpw), 1), dim3(256), 0u, s, sc, fr, tg, (const float4*)nullptr, (const float4*)nullptr,
                    (const uint32_t*)nullptr, (const uint32_t*)nullptr, (float*)nullptr, train_target, rpw, const_cast<float*>(start),
                    TailOut{tail_query, (float4*)tail_rec});
        NRC_HIP(hipGetLastError());
        return;
    }
    launch_last(k_prep_train<2>, dim3(ceil_div(T, 4u * rpw), 1), dim3(256), 0u, s, sc, fr, tg, (const float4*)nullptr, (const float4*)nullptr,
                (const uint32_t*)nullptr, (const uint32_t*)nullptr, (float*)nullptr, train_target, rpw, const_cast<float*>(start));
    NRC_HIP(hipGetLastError());
}

void launch_self_train_combine(uint32_t T, uint32_t spp, const float* tail_rec, const float* tail_y, float* train_target, hipStream_t s)
{
    launch_last(k_self_train_combine, dim3(ceil_div(3u * T, 256u)), dim3(256), 0u, s, T, spp, (const float4*)tail_rec, tail_y, train_target);
    NRC_HIP(hipGetLastError());
}

// this translation unit's copy of the run-time priority switch (nrc_common.hpp), and the host-side value the camera kernels' launchers
// hand over as a kernel argument (DevFrame::raise_priority)
void integrator_set_wave_priority_raise(int on)
{
    NRC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_raise_wave_priority), &on, sizeof(int)));
    g_host_raise_wave_priority = on;
}

void launch_composite(const DevFrame& fr, uint32_t show_nrc, float blend_factor, const float* primary, const float* info,
                      const float* infer_out, float* out_rgba, hipStream_t s, uint32_t* live_count_reset)
{
    launch_last(k_composite, pixel_grid(fr.w, fr.h), dim3(256), 0u, s, fr, show_nrc, blend_factor,
                (const float4*)primary, info, infer_out, (float4*)out_rgba, live_count_reset);
    NRC_HIP(hipGetLastError());
}

void launch_query_layout(const DevFrame& fr, uint32_t floats_per_query, const float* tiled, float* linear, hipStream_t s, const float* info)
{
    hipLaunchKernelGGL(k_query_layout, pixel_grid(fr.w, fr.h), dim3(256), 0, s, fr, floats_per_query, tiled, linear, info);
    NRC_HIP(hipGetLastError());
}
uint32_t query_count(uint32_t w, uint32_t h) { return ceil_div(w, 8) * ceil_div(h, 8) * 64u; }

void launch_compare(const float* ref_rgba, const float* own_rgba, uint32_t n_pixels, double* d_scratch, float* d_result5,
                    hipStream_t s)
{
    hipLaunchKernelGGL(k_compare_1, dim3(CMP_BLOCKS), dim3(256), 0, s, (const float4*)ref_rgba, (const float4*)own_rgba,
                       n_pixels, d_scratch);
    hipLaunchKernelGGL(k_compare_norm, dim3(1), dim3(64), 0, s, d_scratch);
    hipLaunchKernelGGL(k_compare_2, dim3(CMP_BLOCKS), dim3(256), 0, s, (const float4*)ref_rgba, (const float4*)own_rgba,
                       n_pixels, d_scratch);
    hipLaunchKernelGGL(k_compare_final, dim3(1), dim3(64), 0, s, (const double*)d_scratch, d_result5);
    NRC_HIP(hipGetLastError());
}

void launch_compare_sharded_1(const float* ref_rgba, const float* own_rgba, uint32_t n_pixels, double* d_scratch, hipStream_t s)
{
    hipLaunchKernelGGL(k_compare_1, dim3(CMP_BLOCKS), dim3(256), 0, s, (const float4*)ref_rgba, (const float4*)own_rgba, n_pixels, d_scratch);
    hipLaunchKernelGGL(k_compare_fold, dim3(1), dim3(64), 0, s, d_scratch);
    NRC_HIP(hipGetLastError());
}
void launch_compare_sharded_2(const float* ref_rgba, const float* own_rgba, uint32_t n_pixels, double* d_scratch, hipStream_t s)
{
    hipLaunchKernelGGL(k_compare_scale, dim3(1), dim3(64), 0, s, d_scratch);
    hipLaunchKernelGGL(k_compare_2, dim3(CMP_BLOCKS), dim3(256), 0, s, (const float4*)ref_rgba, (const float4*)own_rgba, n_pixels, d_scratch);
    hipLaunchKernelGGL(k_compare_fold_var, dim3(1), dim3(64), 0, s, d_scratch);
    NRC_HIP(hipGetLastError());
}
void launch_compare_sharded_3(double* d_scratch, float* d_result5, hipStream_t s)
{
    hipLaunchKernelGGL(k_compare_final_sharded, dim3(1), dim3(64), 0, s, (const double*)d_scratch, d_result5);
    NRC_HIP(hipGetLastError());
}
void launch_pad_columns(const float* local, uint32_t lw, uint32_t h, uint32_t max_lw, float* padded, hipStream_t s)
{
    hipLaunchKernelGGL(k_pad_columns, dim3(ceil_div(max_lw, 256), h), dim3(256), 0, s, (const float4*)local, lw, h, max_lw, (float4*)padded);
    NRC_HIP(hipGetLastError());
}
void launch_assemble_columns(const float* gathered, uint32_t world, uint32_t block_log2, uint32_t gw, uint32_t h, uint32_t max_lw, float* out,
                             hipStream_t s)
{
    hipLaunchKernelGGL(k_assemble_columns, dim3(ceil_div(gw, 256), h), dim3(256), 0, s, (const float4*)gathered, world, block_log2, gw, h, max_lw,
                       (float4*)out);
    NRC_HIP(hipGetLastError());
}

// ---- the denoise filter.  Scratch: [passes > 1: image][passes > 2: image][guide pairs]; 16-byte aligned.
static size_t denoise_images(uint32_t passes) { return passes > 2u ? 2u : (passes > 1u ? 1u : 0u); }
size_t denoise_scratch_bytes(uint32_t w, uint32_t h, uint32_t passes) { return (size_t)w * h * (16u * denoise_images(passes) + 8u); }
void launch_denoise(const float* rgba, const float* aov, uint32_t w, uint32_t h, const DenoiseParams& p, float* out, void* scratch, hipStream_t s)
{
    if (const char* what = denoise_params_error(p)) fail(std::string("denoise: ") + what);
    if (w == 0u || h == 0u || w > kDenoiseMaxSide || h > kDenoiseMaxSide || (uint64_t)w * h > 0x7fffffffull || ceil_div(h, 8) > 65535u)
        fail("denoise: bad image size");
    if ((((uintptr_t)rgba) | ((uintptr_t)aov) | ((uintptr_t)out) | ((uintptr_t)scratch)) & 15u) fail("denoise: the images and the scratch must be 16-byte aligned");
    const size_t px = (size_t)w * h, img = px * 16u, need = denoise_scratch_bytes(w, h, p.passes);
    const char *o0 = (const char*)out, *s0 = (const char*)scratch, *c0 = (const char*)rgba, *a0 = (const char*)aov;
    auto overlap = [](const char* a, size_t na, const char* b, size_t nb) { return a < b + nb && b < a + na; };
    if (overlap(o0, img, c0, img) || overlap(o0, img, a0, img) || overlap(o0, img, s0, need)) fail("denoise: d_out overlaps an input or the scratch (no in-place operation)");
    if (overlap(s0, need, c0, img) || overlap(s0, need, a0, img)) fail("denoise: the scratch overlaps an input");
    float4* ping = (float4*)scratch;
    float4* pong = ping + px;
    float2* guide = (float2*)(ping + px * denoise_images(p.passes));
    hipLaunchKernelGGL(k_denoise_pack, dim3(ceil_div((uint32_t)px, 256)), dim3(256), 0, s, (const float4*)aov, guide, (uint32_t)px);
    const float4* src = (const float4*)rgba;
    for (uint32_t pass = 0; pass < p.passes; pass++) {      // the last pass writes the output
        float4* dst = pass + 1u == p.passes ? (float4*)out : ((pass & 1u) ? pong : ping);
        hipLaunchKernelGGL(k_denoise_pass, dim3(ceil_div(w, 32), ceil_div(h, 8)), dim3(256), 0, s, src, (const float2*)guide, dst, w, h, denoise_pass(p, pass));
        src = dst;
    }
    NRC_HIP(hipGetLastError());
}

// ---- reprojection.  view comes from reproject_setup: the parameters, the frame count and the history camera have been checked.
void launch_reproject(const float* hist_rgba, const float* hist_n, const float* hist_aov, const float* rgba, const float* aov, uint32_t w, uint32_t h,
                      const ReprojectView& view, float* out, float* out_n, hipStream_t s)
{
    if (w == 0u || h == 0u || (uint64_t)w * h > kReprojectMaxPixels || ceil_div(h, 8) > 65535u) fail("reproject: bad image size");
    const bool hist = view.has_history != 0;
    if (hist != (hist_rgba != nullptr) || hist != (hist_n != nullptr) || hist != (hist_aov != nullptr)) fail("reproject: the history is all or none");
    if (rgba == nullptr || aov == nullptr || out == nullptr || out_n == nullptr) fail("reproject: null image");
    if ((((uintptr_t)rgba) | ((uintptr_t)aov) | ((uintptr_t)out) | ((uintptr_t)hist_rgba) | ((uintptr_t)hist_aov)) & 15u) fail("reproject: the images must be 16-byte aligned");
    if ((((uintptr_t)out_n) | ((uintptr_t)hist_n)) & 3u) fail("reproject: the counts must be 4-byte aligned");
    const size_t px = (size_t)w * h, img = px * 16u, cnt = px * 4u;
    auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
        return b != nullptr && (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na;
    };
    auto hits_input = [&](const void* o, size_t no) {
        return overlap(o, no, rgba, img) || overlap(o, no, aov, img) || overlap(o, no, hist_rgba, img) || overlap(o, no, hist_aov, img) || overlap(o, no, hist_n, cnt);
    };
    if (hits_input(out, img) || hits_input(out_n, cnt) || overlap(out, img, out_n, cnt)) fail("reproject: an output overlaps an input or the other output (no in-place operation)");
    hipLaunchKernelGGL(k_reproject, dim3(ceil_div(w, 32), ceil_div(h, 8)), dim3(256), 0, s, (const float4*)hist_rgba, hist_n, (const float4*)hist_aov,
                       (const float4*)rgba, (const float4*)aov, (float4*)out, out_n, w, h, view);
    NRC_HIP(hipGetLastError());
}

void launch_test_math(int fn, const float* a, const float* b, uint32_t n, float* out, float* out2, hipStream_t s)
{
    hipLaunchKernelGGL(k_test_math, dim3(ceil_div(n, 256)), dim3(256), 0, s, fn, a, b, n, out, out2);
    NRC_HIP(hipGetLastError());
}

void launch_test_rng(float u, float v, const float* fr, uint32_t n, float* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_test_rng, dim3(1), dim3(64), 0, s, u, v, fr[0], fr[1], fr[2], fr[3], n, out);
    NRC_HIP(hipGetLastError());
}

}  // namespace nrc

#ifdef NRC_LOOP_PROFILE
// profiling build only (tools/loop_profile.py): read / reset the loop counters
extern "C" int nrc_debug_wave_times(unsigned long long* out, unsigned n_waves)
{
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(nrc::g_wave_times), (size_t)n_waves * 32) == hipSuccess ? 0 : 1;
}

extern "C" int nrc_debug_loop_profile(unsigned long long* out16, int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    if (out16 && hipMemcpyFromSymbol(out16, HIP_SYMBOL(nrc::g_loop_prof), 16 * sizeof(unsigned long long)) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[24] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(nrc::g_loop_prof), z, 16 * sizeof(unsigned long long)) != hipSuccess) return 1;
        if (hipMemcpyToSymbol(HIP_SYMBOL(nrc::g_live_hist), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
// trips of the tracking loops by the number of walks alive (g_live_hist)
extern "C" int nrc_debug_live_hist(unsigned long long* out24)
{
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    return hipMemcpyFromSymbol(out24, HIP_SYMBOL(nrc::g_live_hist), 24 * sizeof(unsigned long long)) == hipSuccess ? 0 : 1;
}
#endif
