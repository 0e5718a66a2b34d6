// lk.hip -- pyramidal Lucas-Kanade tracker for gfx950 (wave64).
//
// Replaces cv::calcOpticalFlowPyrLK(prev, next, pts, ...) with default arguments as the
// reference calls it at src/tracking.cpp:18 (left->right) and src/tracking.cpp:52
// (t-1 -> t): 21x21 window, 4 pyramid levels, <=30 iterations, eps 0.01, minEig 1e-4,
// 14-bit fixed-point bilinear weights, int16 patches, Scharr derivatives.
//
// Mapping: ONE WAVEFRONT PER KEYPOINT, all pyramid levels inside one launch (the levels
// of one point depend on each other, points never do).  Lane l owns window row l/3 and a
// 7-pixel segment (l%3) of it, i.e. 7*C patch elements that stay in VGPRs for the whole
// level (template patch I and both derivative patches).  Per level a wave
//   1. stages the 24x24 neighbourhood of the previous image and the 22x22 tile of its Scharr
//      derivative level (pyramid.hip materialises the derivative levels once per image, zero
//      outside the image as OpenCV pads its derivative buffer) in LDS with aligned 16-byte row
//      loads, builds its patch registers and the 2x2 normal matrix;
//   2. stages a (22+2*JR)^2 tile of the next image around the current guess and iterates
//      out of LDS; the tile is re-staged only when the guess drifts more than JR pixels, and the
//      lane's rows are re-read from it only when the guess enters another pixel cell.
// All sums of integer products are exact (int32 per lane, int64 across the wave via
// cross-lane shuffles) and are rounded to float once, so the result does not depend on
// the reduction order; scalar float math is compiled with -ffp-contract=off.
//
// Roofline: the kernel's algorithmic HBM traffic is both pyramids once plus 21 B/point
// (SURVEY.md section 8d); its time is VALU/LDS work, see DESIGN.md.
#include <cstdlib>
#include <type_traits>

#include "svo_internal.h"

namespace {

constexpr int WIN = SVO_LK_WIN;
constexpr int JR = 5;                  // drift radius one staged J tile tolerates
constexpr int TS = WIN + 1 + 2 * JR;   // 32: J tile side
constexpr int PT = WIN + 3;            // 24: previous-image tile side (Scharr + bilinear halo)
constexpr int DT = WIN + 1;            // 22: derivative tile side
constexpr int SEG = 7;                 // pixels per lane; 3 lanes per window row
constexpr int WAVES = 1;               // waves (= keypoints) per workgroup: a slow point never
                                       // holds the LDS of finished neighbours
constexpr int W_BITS = 14;

struct LkParams {
    int max_level;
    int max_count;
    double eps_sq;
    float eps_pre;  // a step with max(|dx|, |dy|) above this cannot pass the eps_sq test (1.01 * sqrt(eps_sq))
    float min_eig_thr;
    int doff[SVO_MAX_LEVELS];    // derivative levels of the jobs' first pyramids: element (0,0), in ints
    int dpitch[SVO_MAX_LEVELS];  // bytes, multiple of 16
    int interleave;              // 1: keypoint = workgroup index (a lone launch: balance before L2 locality), 0: XCD bands
    int lattice;                 // 0: every level interpolates its patches, integer positions too (SVO_LK_LATTICE=0, for A/B and tests)
    int cell_cache;              // 0: every iteration reloads and pairs its two tile rows, same cell or not (SVO_LK_CELL_CACHE=0, for A/B and tests)
    int mono;                    // 0: grey frames stored as BGR get the three-channel arithmetic too (SVO_LK_MONO=0, for A/B and tests)
    // the grey regions of grey-stored three-channel pyramids (svo_internal.h): bytes from pixel (0, 0) of level l to pixel
    // (0, 0) of grey level l, and element (0, 0) of grey derivative level l in ints; the pitches follow from the widths
    int gdelta[SVO_MAX_LEVELS], gdoff[SVO_MAX_LEVELS];
};
static_assert(sizeof(LkBatch) + sizeof(LkParams) <= 4096, "kernel arguments are limited to 4 KB");

// An LDS tile keeps the 16-byte-aligned row segments exactly as loaded: row r, byte b of
// the tile lives at r*ROW + shift + b, where shift = (address of the tile origin) & 15 is
// the same for every row because the level pitch is a multiple of 16.
template <int C, int SIDE> struct Tile {
    static constexpr int ROWB = SIDE * C;
    static constexpr int VEC = (ROWB + 15 + 15) / 16;  // 16-byte vectors per row, any shift
    // row stride: an ODD number of 16-byte units, so that the rows of a tile spread over the LDS banks
    // (with 6 units = 24 dwords every 4th or 8th row of the Scharr pass's byte reads shared its banks)
    static constexpr int ROW = (VEC | 1) * 16;
    static constexpr int BYTES = SIDE * ROW;
};
// the derivative tile: DT x DT "pixels" of 4 * C bytes, rows as loaded (16-byte vectors, any shift)
template <int C> struct DTile {
    static constexpr int ROWB = DT * C * 4;
    static constexpr int VEC = (ROWB + 15 + 15) / 16;
    static constexpr int ROW = (VEC | 1) * 16;  // odd number of 16-byte units: rows spread over the banks
    static constexpr int BYTES = DT * ROW;
};
template <int C> struct Lds {
    static constexpr int T_BYTES = Tile<C, PT>::BYTES;
    static constexpr int D_BYTES = DTile<C>::BYTES;
    static constexpr int J_BYTES = Tile<C, TS>::BYTES;
    // the three tiles take turns in the same space: 6.7 KB per wave, so that the 16 waves of a tracking
    // launch leave a third of a CU's LDS to the short kernels of the other chunks' stages (with the
    // previous-image tile beside the derivative tile, 9.4 KB, those waited for tracking waves to end)
    static constexpr int A = T_BYTES > D_BYTES ? T_BYTES : D_BYTES;
    static constexpr int WAVE_BYTES = (((A > J_BYTES ? A : J_BYTES) + 15) / 16) * 16;
};

// LDS produced by some lanes of a wave and consumed by others of the SAME wave: LDS
// instructions of one wave execute in order; this only stops the compiler from moving
// accesses across the hand-off.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Exact sum over the 64 lanes of a per-lane int32 partial (|v| < 2^30).  The partial is split
// into its low 16 bits and its (signed) high part; each half is summed with DPP butterflies
// inside the 16-lane rows (no carries can occur: 64 * 2^16 < 2^31) and the four row totals
// are combined on the scalar unit.  Result is wave-uniform.
__device__ __forceinline__ int row16_sum(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);  // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);  // row_mirror
    return v;
}
// the total of all 64 lanes, valid in lane 63 only: two more DPP steps carry the row totals
// across (row_bcast15 into rows 1 and 3, row_bcast31 into rows 2 and 3)
__device__ __forceinline__ int wave_total_lane63(int v)
{
    v = row16_sum(v);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31
    return __builtin_amdgcn_readlane(v, 63);
}
// exact 64-lane sum as a double (|total| < 2^37: exactly representable), wave-uniform
__device__ __forceinline__ double wave_sum_exact(int v)
{
    const int slo = wave_total_lane63(v & 0xffff), shi = wave_total_lane63(v >> 16);
    return (double)shi * 65536. + (double)slo;
}

// MUL (1 or 3) in the sums below: the one-channel body of the tracker (lk_track_kernel, "mono") sums a third of the
// elements of a grey frame stored as BGR, and every three-channel total is exactly MUL times its total.  The factor is
// applied to the EXACT INTEGER total, on the scalar unit, before the one rounding to float, so the float is the one the
// three-channel sum gives, bit for bit.  Ranges with MUL = 3: a lane's one-channel partial is a third of its
// three-channel one (|v| < 2^30 / 3), so the split halves behave as before, |total| < 2^37 / 3, and MUL * total is below
// 2^37 like the three-channel total: exact as a long long and as a double.

// the same total (times MUL) rounded to float (round to nearest even of the exact integer, like the double
// path): it nearly always fits 32 bits, then one v_cvt_f32_i32 does it (scalar test)
template <int MUL = 1> __device__ __forceinline__ float wave_sum_float(int v)
{
    const int slo = wave_total_lane63(v & 0xffff), shi = wave_total_lane63(v >> 16);
    const long long t = ((long long)shi * 65536 + slo) * MUL;
    if (t == (long long)(int)t)
        return (float)(int)t;
    return (float)(((double)shi * 65536. + (double)slo) * (double)MUL);  // |total| < 2^37: exact
}

// Two exact totals at once.  When every lane's partials lie in [-2^25, 2^25) -- nearly always: a
// lane would need a mean |residual * derivative| above 1.6e6 per element to leave it -- neither the
// totals nor any partial sum of the butterflies can leave int32, so one DPP chain per total does
// it; otherwise the split path.  Both are exact: the choice never changes a result.
// With MUL = 3 the narrow range is [-2^23, 2^23) per lane -- the same bound per element, a lane has a third of them --
// so that the 64-lane total lies in [-2^29, 2^29) and three times it in [-3 * 2^29, 3 * 2^29), inside int32: one
// s_mul_i32 before the v_cvt_f32_i32.
template <int MUL = 1> __device__ __forceinline__ void wave_sum2_float(int a, int b, float &fa, float &fb)
{
    constexpr int NB = MUL == 1 ? 25 : 23;
    static_assert(MUL == 1 || MUL == 3, "the narrow range is worked out for these");
    const unsigned wide = ((unsigned)(a + (1 << NB)) | (unsigned)(b + (1 << NB))) >> (NB + 1);
    if (__builtin_amdgcn_ballot_w64(wide != 0) == 0) {
        fa = (float)(wave_total_lane63(a) * MUL);
        fb = (float)(wave_total_lane63(b) * MUL);
    } else {
        fa = wave_sum_float<MUL>(a);
        fb = wave_sum_float<MUL>(b);
    }
}

template <int MUL = 1>
__device__ __forceinline__ void wave_sum3_float(int a, int b, int c, float &fa, float &fb, float &fc)
{
    constexpr int NB = MUL == 1 ? 25 : 23;
    static_assert(MUL == 1 || MUL == 3, "the narrow range is worked out for these");
    const unsigned wide = ((unsigned)(a + (1 << NB)) | (unsigned)(b + (1 << NB)) | (unsigned)(c + (1 << NB))) >> (NB + 1);
    if (__builtin_amdgcn_ballot_w64(wide != 0) == 0) {
        fa = (float)(wave_total_lane63(a) * MUL);
        fb = (float)(wave_total_lane63(b) * MUL);
        fc = (float)(wave_total_lane63(c) * MUL);
    } else {
        fa = (float)(wave_sum_exact(a) * (double)MUL);  // |total| < 2^37: the product is exact
        fb = (float)(wave_sum_exact(b) * (double)MUL);
        fc = (float)(wave_sum_exact(c) * (double)MUL);
    }
}

// The iteration's form of the weights, already packed as the column-pair sampling wants them:
// wv0 = (w00 | w10 << 16), wv1 = (w01 | w11 << 16).  Same values as bilinear_weights bit for bit:
//  - scaling by 2^14 is exact, so it is applied to (1 - a) and a once instead of to three products;
//  - rint(x) for 0 <= x < 2^22 is the low mantissa of x + 1.5 * 2^23 (round to nearest even in the
//    add), i.e. the low 16 bits of that float's bit pattern ARE the int16 weight: no v_rndne / v_cvt,
//    and one v_perm_b32 packs two of them;
//  - w11 = 2^14 - w00 - w01 - w10 from the same bit patterns (the three magic offsets cancel in the
//    constant), low half taken by the permute (w11 may be -1).
__device__ __forceinline__ void bilinear_weight_pairs(float a, float b, int &wv0, int &wv1)
{
    const float MAGIC = 12582912.f;  // 1.5 * 2^23, bit pattern 0x4B400000
    const float na = 1.f - a, nb = 1.f - b;
    const float A1 = na * (float)(1 << W_BITS), A0 = a * (float)(1 << W_BITS);
    const unsigned b00 = __builtin_bit_cast(unsigned, A1 * nb + MAGIC);
    const unsigned b01 = __builtin_bit_cast(unsigned, A0 * nb + MAGIC);
    const unsigned b10 = __builtin_bit_cast(unsigned, A1 * b + MAGIC);
    const unsigned b11 = (unsigned)(1 << W_BITS) + 3u * 0x4B400000u - (b00 + b01 + b10);
    wv0 = (int)__builtin_amdgcn_perm(b10, b00, 0x05040100u);
    wv1 = (int)__builtin_amdgcn_perm(b11, b01, 0x05040100u);
}

__device__ __forceinline__ void bilinear_weights(float a, float b, int &w00, int &w01, int &w10,
                                                 int &w11)
{
    w00 = (int)rintf((1.f - a) * (1.f - b) * (float)(1 << W_BITS));
    w01 = (int)rintf(a * (1.f - b) * (float)(1 << W_BITS));
    w10 = (int)rintf((1.f - a) * b * (float)(1 << W_BITS));
    w11 = (1 << W_BITS) - w00 - w01 - w10;
}

// Stage a SIDE x SIDE pixel tile whose top-left pixel is (ox, oy) into LDS with aligned 16-byte loads
// (global_load_dwordx4 -> ds_write_b128), in two halves so that a later staging's loads can be in flight
// while this tile is consumed: tile_issue starts the loads into registers, tile_commit<LATER> waits until at
// most LATER younger vector-memory loads are outstanding (loads return in order) and writes the LDS rows.
// Between the two NOTHING may touch the registers of `t.v`.  lane -> (row group, 16-byte vector): LPR lanes
// per row (the lanes past VEC repeat the last vector), RPI rows per step; the k-th step differs from the
// first by k * RPI rows only, which goes into the scalar base and the ds_write immediate -- one lane offset
// for all the loads, written out as SGPR base + 32-bit lane offset (left to itself the compiler forms 64-bit
// lane addresses per load and level, keeps them across the iteration loop and spills).
typedef unsigned uint4v __attribute__((ext_vector_type(4)));
template <int C, int SIDE> struct TileLoad {
    using TL = Tile<C, SIDE>;
    static constexpr int LPR = TL::VEC <= 4 ? 4 : 8, RPI = 64 / LPR, ITER = (SIDE + RPI - 1) / RPI;
    static_assert(TL::VEC <= LPR, "row wider than a lane group");
    uint4v v[ITER];
    int shift;  // byte shift of the tile: pixel (0, 0) lives at tile + shift
};

template <int C, int SIDE>
__device__ __forceinline__ void tile_issue(TileLoad<C, SIDE> &t, const uint8_t *__restrict__ lvl, int pitch, int ox,
                                           int oy, int lane)
{
    using LD = TileLoad<C, SIDE>;
    // wave-uniform base (said so explicitly: the loads then take an SGPR base + a 32-bit lane offset)
    const int off = oy * pitch + ox * C;  // inside one padded level: fits 32 bits
    t.shift = (int)(((unsigned)reinterpret_cast<uintptr_t>(lvl) + (unsigned)off) & 15u);
    const uint8_t *a16 = lvl + (ptrdiff_t)__builtin_amdgcn_readfirstlane(off - t.shift);
    const unsigned r0 = (unsigned)lane / LD::LPR, vv = min((unsigned)lane % LD::LPR, (unsigned)LD::TL::VEC - 1);
#pragma unroll
    for (int k = 0; k < LD::ITER; k++) {
        // the last step may reach past the tile: those lanes repeat the last row
        const bool clamp = (k + 1) * LD::RPI > SIDE;
        const unsigned goff = (clamp ? min(r0, (unsigned)(SIDE - 1 - k * LD::RPI)) : r0) * (unsigned)pitch + vv * 16u;
        asm volatile("global_load_dwordx4 %0, %1, %2"
                     : "=&v"(t.v[k])
                     : "v"(goff), "s"(a16 + (ptrdiff_t)(k * LD::RPI) * pitch)
                     : "memory");
    }
}

template <int C, int SIDE, int LATER = 0>
__device__ __forceinline__ void tile_commit(TileLoad<C, SIDE> &t, uint8_t *tile, int lane)
{
    using LD = TileLoad<C, SIDE>;
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(t.v[0]) : "n"(LATER) : "memory");
#pragma unroll
    for (int k = 1; k < LD::ITER; k++)
        asm volatile("" : "+v"(t.v[k]));
    const unsigned r0 = (unsigned)lane / LD::LPR, vv = min((unsigned)lane % LD::LPR, (unsigned)LD::TL::VEC - 1);
#pragma unroll
    for (int k = 0; k < LD::ITER; k++) {
        const bool clamp = (k + 1) * LD::RPI > SIDE;
        const unsigned r = clamp ? min(r0, (unsigned)(SIDE - 1 - k * LD::RPI)) : r0;
        *reinterpret_cast<uint4v *>(tile + (k * LD::RPI + r) * LD::TL::ROW + vv * 16) = t.v[k];
    }
}

// issue + commit back to back; returns the byte shift
template <int C, int SIDE>
__device__ __forceinline__ int stage_tile(uint8_t *tile, const uint8_t *__restrict__ lvl, int pitch, int ox,
                                          int oy, int lane)
{
    TileLoad<C, SIDE> t;
    tile_issue<C, SIDE>(t, lvl, pitch, ox, oy, lane);
    tile_commit<C, SIDE>(t, tile, lane);
    return t.shift;
}

// The DT x DT tile of a derivative level whose top-left element is pixel (ox, oy): rows of DT * C ints,
// fetched as aligned 16-byte vectors (the level's pitch is a multiple of 16, so every row starts at the same
// byte shift, a multiple of 4).  Lane -> (row, vector) by shifts and masks only (a linear deal of the VEC = 19
// vectors per row cost a division per load, 70 instructions per level): part A takes vectors 0..15 of four
// rows per step, part B the remaining VEC - 16 vectors of sixteen rows per step (four lanes per row; spare
// lanes repeat the last vector).  dtile_issue starts ALL the loads (eight vectors per lane at C = 3: the tile
// is in flight while the template patch is formed from the previous-image tile, which occupies the same LDS
// area), dtile_commit waits for them and writes the rows.
template <int C> struct DtileLoad {
    using DL = DTile<C>;
    static constexpr int VA = DL::VEC < 16 ? DL::VEC : 16, VB = DL::VEC - VA;  // vectors per row in part A / part B
    static_assert(VB <= 4, "part B deals four lanes to a row");
    static constexpr int ITA = (DT + 3) / 4, ITB = VB > 0 ? (DT + 15) / 16 : 0, N = ITA + ITB;
    uint4v v[N];
    int shift;
};

template <int C>
__device__ __forceinline__ void dtile_issue(DtileLoad<C> &t, const int *__restrict__ lvl, int dpitch, int ox, int oy,
                                            int lane)
{
    using LD = DtileLoad<C>;
    const int off = oy * dpitch + ox * (C * 4);  // bytes from element (0,0); inside one padded level: fits 32 bits
    t.shift = (int)(((unsigned)reinterpret_cast<uintptr_t>(lvl) + (unsigned)off) & 15u);
    const uint8_t *a16 = reinterpret_cast<const uint8_t *>(lvl) + (ptrdiff_t)__builtin_amdgcn_readfirstlane(off - t.shift);
    // the lane offsets are a handful of instructions: recomputed per level (an opaque copy of the lane stops
    // the compiler from keeping them in registers across the level loop -- the kernel has none to spare)
    asm volatile("" : "+v"(lane));
    {
        const unsigned r0 = (unsigned)lane >> 4, c = min((unsigned)lane & 15u, (unsigned)LD::VA - 1);
#pragma unroll
        for (int k = 0; k < LD::ITA; k++) {
            const bool clamp = (k + 1) * 4 > DT;  // the last step may reach past the tile: those lanes repeat the last row
            const unsigned goff = (clamp ? min(r0, (unsigned)(DT - 1 - k * 4)) : r0) * (unsigned)dpitch + c * 16u;
            asm volatile("global_load_dwordx4 %0, %1, %2"
                         : "=&v"(t.v[k])
                         : "v"(goff), "s"(a16 + (ptrdiff_t)(k * 4) * dpitch)
                         : "memory");
        }
    }
    if (LD::VB > 0) {
        const unsigned r0 = (unsigned)lane >> 2, c = (unsigned)LD::VA + min((unsigned)lane & 3u, (unsigned)(LD::VB > 0 ? LD::VB - 1 : 0));
#pragma unroll
        for (int k = 0; k < LD::ITB; k++) {
            const bool clamp = (k + 1) * 16 > DT;
            const unsigned goff = (clamp ? min(r0, (unsigned)(DT - 1 - k * 16)) : r0) * (unsigned)dpitch + c * 16u;
            asm volatile("global_load_dwordx4 %0, %1, %2"
                         : "=&v"(t.v[LD::ITA + k])
                         : "v"(goff), "s"(a16 + (ptrdiff_t)(k * 16) * dpitch)
                         : "memory");
        }
    }
}

template <int C> __device__ __forceinline__ void dtile_commit(DtileLoad<C> &t, uint8_t *tile, int lane)
{
    using LD = DtileLoad<C>;
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(t.v[0])::"memory");
#pragma unroll
    for (int k = 1; k < LD::N; k++)
        asm volatile("" : "+v"(t.v[k]));
    asm volatile("" : "+v"(lane));
    {
        const unsigned r0 = (unsigned)lane >> 4, c = min((unsigned)lane & 15u, (unsigned)LD::VA - 1);
#pragma unroll
        for (int k = 0; k < LD::ITA; k++) {
            const bool clamp = (k + 1) * 4 > DT;
            const unsigned r = clamp ? min(r0, (unsigned)(DT - 1 - k * 4)) : r0;
            *reinterpret_cast<uint4v *>(tile + (k * 4 + r) * LD::DL::ROW + c * 16) = t.v[k];
        }
    }
    if (LD::VB > 0) {
        const unsigned r0 = (unsigned)lane >> 2, c = (unsigned)LD::VA + min((unsigned)lane & 3u, (unsigned)(LD::VB > 0 ? LD::VB - 1 : 0));
#pragma unroll
        for (int k = 0; k < LD::ITB; k++) {
            const bool clamp = (k + 1) * 16 > DT;
            const unsigned r = clamp ? min(r0, (unsigned)(DT - 1 - k * 16)) : r0;
            *reinterpret_cast<uint4v *>(tile + (k * 16 + r) * LD::DL::ROW + c * 16) = t.v[LD::ITA + k];
        }
    }
}

// Every lane of a wave computes the same control values (guess, step, tile origin): telling the
// compiler so turns the loop's branches into scalar compares instead of exec-mask juggling.
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
// (int)f of a wave-uniform, already floored float as a scalar: convert, then read the first lane.  Written
// out because the compiler turns readfirstlane(cvt(f)) into cvt(readfirstlane(f)) and then needs a second
// readfirstlane to get the integer out of the vector register again.
__device__ __forceinline__ int uniform_int_of(float f)
{
    int i;
    asm("v_cvt_i32_f32 %0, %1" : "=v"(i) : "v"(f));
    return __builtin_amdgcn_readfirstlane(i);
}
__device__ __forceinline__ bool uniform(bool c) { return __builtin_amdgcn_ballot_w64(c) != 0; }

typedef short short2v __attribute__((ext_vector_type(2)));
constexpr int npairs(int c) { return (SEG * c + 1) / 2; }
constexpr int ndwords(int c) { return ((SEG + 1) * c + 3) / 4; }  // packed dwords of one (SEG+1)-pixel row run
// The arithmetic below is written for CA channels per pixel out of the S the level STORES: CA == S everywhere but in the
// one-channel body for grey frames stored as BGR (CA = 1, S = 3), which takes channel 0 of every pixel.  Element k of a
// lane's run is byte (of an image row run) / entry (of a derivative row run) elem_at(k, CA, S).
constexpr int elem_at(int k, int ca, int s) { return (k / ca) * s + k % ca; }

__device__ __forceinline__ int sdot2(int a, int b, int c)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, b), c, false);
}

// dot(a, b) + c with c in an SGPR: the VOP3P form, so a rounding constant costs no v_mov per
// element (the compiler's own choice is v_mov + the accumulate-in-place VOP2 form)
__device__ __forceinline__ int sdot2_sconst(int a, int b, int c_uniform)
{
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c_uniform));
    return d;
}

// The (SEG+1)*C bytes of a row run starting at LDS byte offset `off` (any alignment), as
// packed dwords: aligned ds_read_b32 (never the misaligned b64/b128 the compiler would form
// from byte loads, which replay at 64 cycles) + one v_alignbyte_b32 per dword.
template <int C>
__device__ __forceinline__ void load_row_packed(const uint8_t *lds, int off, unsigned (&d)[ndwords(C)])
{
    const unsigned sh = (unsigned)off & 3u;
    const unsigned *base = reinterpret_cast<const unsigned *>(lds + (off & ~3));
    unsigned raw[ndwords(C) + 1];
#pragma unroll
    for (int i = 0; i <= ndwords(C); i++)
        raw[i] = base[i];
#pragma unroll
    for (int i = 0; i < ndwords(C); i++)
        d[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], sh);
}

template <int C, int K> struct ForEachElem {
    template <class F> static __device__ __forceinline__ void run(F &&f)
    {
        ForEachElem<C, K - 1>::run(f);
        f(std::integral_constant<int, K - 1>());
    }
};
template <int C> struct ForEachElem<C, 0> {
    template <class F> static __device__ __forceinline__ void run(F &&) {}
};

// (byte K of the upper row run) | (byte K of the lower row run) << 16: the two VERTICAL bilinear
// neighbours of column K as an int16 pair, one v_perm_b32 (selector bytes 0-3 pick from the second
// source, 4-7 from the first, 0x0c is a zero byte).  Element k needs columns k and k+C, so a lane
// builds (SEG+1)*C such pairs per sample instead of 2*SEG*C horizontal ones.
template <int C, int K>
__device__ __forceinline__ int column_pair(const unsigned (&up)[ndwords(C)], const unsigned (&lo)[ndwords(C)])
{
    constexpr unsigned sel = (unsigned)(K & 3) | (0x0cu << 8) | ((4u + (unsigned)(K & 3)) << 16) | (0x0cu << 24);
    return (int)__builtin_amdgcn_perm(lo[K >> 2], up[K >> 2], sel);
}

// The (SEG+1)*C column pairs of a lane's two row runs.  They depend on the staged tile and on the integer
// cell of the sampling position only, not on its fractions.
template <int CA, int S>
__device__ __forceinline__ void lane_column_pairs(const unsigned (&up)[ndwords(S)], const unsigned (&lo)[ndwords(S)],
                                                  int (&V)[(SEG + 1) * CA])
{
    ForEachElem<CA, (SEG + 1) * CA>::run([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        V[k] = column_pair<S, elem_at(k, CA, S)>(up, lo);
    });
}

// The bilinear samples of a lane's SEG*C elements, descaled by `SHIFT` bits and packed as int16
// pairs (low half = even element; an odd count is padded with 0):
//   S_k = w00 p[k] + w10 q[k] + w01 p[k+C] + w11 q[k+C] + RND          (p, q: upper / lower row)
// = two v_dot2_i32_i16 on column pairs with the weight pairs wv0 = (w00 | w10 << 16) and
// wv1 = (w01 | w11 << 16) (pixel <= 255, -1 <= weight <= 2^14: exact).  S >> SHIFT of two elements is
// packed without per-element shifts: one v_perm_b32 takes bits 8..23 of both sums (|S| < 2^23), one
// v_pk_ashrrev_i16 drops the remaining SHIFT - 8 bits.
template <int C, int SHIFT>
__device__ __forceinline__ void samples_of_pairs(const int (&V)[(SEG + 1) * C], int wv0, int wv1, int (&out)[npairs(C)])
{
    static_assert(SHIFT >= 8 && SHIFT < 16, "the packing below takes bits 8..23 of each sum");
    constexpr int NE = SEG * C;
    constexpr int RND = 1 << (SHIFT - 1);
    int S[NE + 1];
    S[NE] = 0;
#pragma unroll
    for (int k = 0; k < NE; k++)
        S[k] = sdot2(V[k + C], wv1, sdot2_sconst(V[k], wv0, RND));
#pragma unroll
    for (int j = 0; j < npairs(C); j++) {
        const int k0 = 2 * j, k1 = 2 * j + 1 < NE ? 2 * j + 1 : NE;
        const int mid = (int)__builtin_amdgcn_perm((unsigned)S[k1], (unsigned)S[k0], 0x06050201u);  // bytes 1,2 of each
        const short2v sh = {(short)(SHIFT - 8), (short)(SHIFT - 8)};
        out[j] = __builtin_bit_cast(int, (short2v)(__builtin_bit_cast(short2v, mid) >> sh));
    }
}

template <int CA, int S, int SHIFT>
__device__ __forceinline__ void lane_samples(const unsigned (&up)[ndwords(S)], const unsigned (&lo)[ndwords(S)],
                                             int wv0, int wv1, int (&out)[npairs(CA)])
{
    int V[(SEG + 1) * CA];
    lane_column_pairs<CA, S>(up, lo, V);
    samples_of_pairs<CA, SHIFT>(V, wv0, wv1, out);
}

// low (HI = false) or high (HI = true) int16 halves of two dwords as a pair: (x.half, y.half)
template <bool HI> __device__ __forceinline__ int half_pair(int x, int y)
{
    constexpr unsigned sel = HI ? 0x07060302u : 0x05040100u;
    return (int)__builtin_amdgcn_perm((unsigned)y, (unsigned)x, sel);
}

// One lane's share of  sum |J - I|  over its 7*C patch elements (the err output of the reference,
// level 0, once per keypoint): lane_samples, then per element pair one v_pk_sub_i16 against the
// packed template.
template <int CA, int S>
__device__ __forceinline__ int lane_abs_residual(const uint8_t *lds, int off, int wv0, int wv1,
                                                 const int (&Ivp)[npairs(CA)])
{
    constexpr int NE = SEG * CA;
    unsigned r0[ndwords(S)], r1[ndwords(S)];
    load_row_packed<S>(lds, off, r0);
    load_row_packed<S>(lds, off + Tile<S, TS>::ROW, r1);
    int Jp[npairs(CA)];
    lane_samples<CA, S, W_BITS - 5>(r0, r1, wv0, wv1, Jp);
    int s = 0;
#pragma unroll
    for (int j = 0; j < npairs(CA); j++) {
        const short2v d = __builtin_bit_cast(short2v, Jp[j]) - __builtin_bit_cast(short2v, Ivp[j]);
        const int d0 = d.x, d1 = d.y;
        s += (d0 < 0 ? -d0 : d0) + (2 * j + 1 < NE ? (d1 < 0 ? -d1 : d1) : 0);
    }
    return s;
}

// The iteration samples the staged J tile in two halves.  "Load and pair": the lane's two row runs at the
// guess's integer cell, as column pairs.  They do not depend on the guess's fractions, so the iteration loop
// keeps them while the guess stays in its cell and the tile is not re-staged.
template <int CA, int S>
__device__ __forceinline__ void lane_load_pairs(const uint8_t *lds, int off, int (&V)[(SEG + 1) * CA])
{
    unsigned r0[ndwords(S)], r1[ndwords(S)];
    load_row_packed<S>(lds, off, r0);
    load_row_packed<S>(lds, off + Tile<S, TS>::ROW, r1);
    lane_column_pairs<CA, S>(r0, r1, V);
}

// "Weigh and dot", the iteration's form of the residual sums:  sum (J - I) * Ix = sum J * Ix - sum I * Ix, and
// the second term does not change during a level -- the caller passes it (negated) as the start of the
// accumulator chain, which saves the v_pk_sub_i16 per element pair.  Integer arithmetic, no
// overflow (|sum J * Ix| and |sum I * Ix| < 2^30 per lane): the same value bit for bit.
template <int C>
__device__ __forceinline__ void lane_mismatch(const int (&V)[(SEG + 1) * C], int wv0, int wv1,
                                              const int (&Ixp)[npairs(C)], const int (&Iyp)[npairs(C)], int neg_c1,
                                              int neg_c2, int &s1, int &s2)
{
    // element pair by element pair, GROUP pairs at a time: the sums of a group are finished before the next
    // group's samples start, so that few of them are alive beside the cached column pairs
    constexpr int NE = SEG * C, RND = 1 << (W_BITS - 5 - 1), GROUP = 4;
    const short2v sh = {(short)(W_BITS - 5 - 8), (short)(W_BITS - 5 - 8)};
#pragma unroll
    for (int j = 0; j < npairs(C); j++) {
        const int k0 = 2 * j, k1 = 2 * j + 1;
        const int S0 = sdot2(V[k0 + C], wv1, sdot2_sconst(V[k0], wv0, RND));
        const int S1 = k1 < NE ? sdot2(V[k1 + C], wv1, sdot2_sconst(V[k1], wv0, RND)) : 0;
        const int mid = (int)__builtin_amdgcn_perm((unsigned)S1, (unsigned)S0, 0x06050201u);  // bytes 1,2 of each
        const int Jp = __builtin_bit_cast(int, (short2v)(__builtin_bit_cast(short2v, mid) >> sh));
        if (j == 0) {
            // the chains start from the level's constants: the first link in the three-operand form (the compiler's
            // accumulate-in-place form costs a copy of each constant per iteration)
            asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(s1) : "v"(Jp), "v"(Ixp[0]), "v"(neg_c1));
            asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(s2) : "v"(Jp), "v"(Iyp[0]), "v"(neg_c2));
        } else {
            s1 = sdot2(Jp, Ixp[j], s1);
            s2 = sdot2(Jp, Iyp[j], s2);
        }
        if (j % GROUP == GROUP - 1 && j + 1 < npairs(C))
            asm volatile("" : "+v"(s1), "+v"(s2), "+v"(wv0), "+v"(wv1));
    }
}

// One launch may carry the LK passes of several independent chunks of the stream (blockIdx.y picks
// the job): the launch lasts as long as the slowest keypoint of ANY job, so two jobs cost little
// more than one (svo_vo_run_chunks, chunks that share a context).
// WANT_ERR = false: no job of the launch asks for the level-0 residual (the front-end never does).  The template
// patch then dies with step 1 of a level instead of occupying its registers through the iteration loop.
// Register budget: <1, *, *> compile to the 64 / 70 registers they had before the kernel held two bodies.  With both bodies
// <3, *, false> wants 98 registers (one body alone: 96): the launch bound forces it back to 96 = five waves per SIMD, without
// scratch.  Measured on colour frames: without the bound (104 allocated, four waves) the 16-job launch
// is 28 us of 700 slower, with it 8 us -- the bound is not what colour frames pay.  <3, *, true> takes 102 (100 before), the
// same allocation of 104.
template <int C, int NJ, bool WANT_ERR>
__global__ __launch_bounds__(64 * WAVES, C == 3 && !WANT_ERR ? 5 : 4) void lk_track_kernel(LkBatchN<NJ> batch, LkParams prm)
{
    const LkJob &job = batch.j[blockIdx.y];
    if (job.gate && *job.gate == 0)
        return;  // a pass of the chain runner that is not due (no keyframe / the chain halted): scalar load, scalar branch
    const PyrDev &prev = job.prev, &next = job.next;
    const int *__restrict__ dprev = job.dprev;
    const float *__restrict__ prev_pts = job.prev_pts;
    const int n_cap = job.n_cap;
    const int *__restrict__ d_n = job.d_n;
    float *__restrict__ next_pts = job.next_pts;
    uint8_t *__restrict__ status = job.status;
    float *__restrict__ err = WANT_ERR ? job.err : nullptr;
    float *__restrict__ min_eig_out = job.min_eig;
    const int n = d_n ? min(*d_n, n_cap) : n_cap;  // live count may sit in HBM (chained stages)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // XCD-aware point order: workgroups go to the 8 XCDs round-robin, keypoints arrive in raster
    // order, so XCD x is given the x-th contiguous eighth of the list -- one band of the image.
    // Each XCD's L2 then fetches its band of both pyramids once instead of all of them.
    const int band = (n + 7) >> 3, in_band = (blockIdx.x >> 3) * WAVES + wave;
    // A launch that has the chip to itself holds one wave per slot from start to end: with bands, the XCD whose band
    // of the image needs the most iterations sets the launch's length; dealt out round-robin every XCD gets the same mix.
    const int p = prm.interleave ? (int)blockIdx.x * WAVES + wave : (blockIdx.x & 7) * band + in_band;
    if ((!prm.interleave && in_band >= band) || p >= n)
        return;  // whole wave leaves; no workgroup barrier is used below
    uint8_t *lds = smem + wave * Lds<C>::WAVE_BYTES;
    uint8_t *T = lds;                                           // PT x PT x C bytes
    uint8_t *DB = lds;                                          // DT rows of packed (4 dx | 4 dy << 16), as loaded (after T)
    uint8_t *TJ = lds;                                          // TS x TS x C bytes (after D)

    const bool active = lane < 3 * WIN;
    const int wy = active ? lane / 3 : WIN - 1;  // window row of this lane
    const int ws = active ? lane - 3 * wy : 0;   // segment
    const int wx = ws * SEG;

    const float ptx = prev_pts[2 * p], pty = prev_pts[2 * p + 1];
    const float half = (WIN - 1) * 0.5f;
    const float FLT_SCALE = 1.f / (1 << 20);

    float outx = 0.f, outy = 0.f;  // == nextPts[ptidx] of the reference implementation
    int st = 1;
    float errv = 0.f, mineig0 = 0.f;

    // The levels (lk_levels.hip.h, included once per body), written once for CA channels of arithmetic per pixel out of the C the pyramids store.  CA == C is the
    // tracker as it always was.  CA = 1 with C = 3 is the one-channel body for GREY frames stored as BGR: with B == G == R in
    // both images every patch element, derivative and product of the window exists three times with the same value, and
    // since every sum below is an exact integer that is rounded once, the three-channel total is exactly three times the
    // total over channel 0.  That body reads bytes 3 p of the staged image tiles and every third entry of the derivative
    // tile (tiles, staging, LDS layout and the lane <-> window mapping are the same: the pyramids keep their layout for
    // everybody else), keeps 7 patch elements per lane instead of 21, and multiplies the exact totals -- the normal
    // matrix, the two mismatch sums of every iteration, the level-0 residual -- by MUL = 3 before their rounding
    // (wave_sum*_float<MUL>).  Everything after the rounding is this same code: the same result bit for bit.
    if constexpr (C == 3) {
        // Wave-uniform, per job (the jobs of one launch may differ): the "channels agree" words of both pyramids, which sit
        // in front of level 0's padded buffer (svo_internal.h) -- two scalar loads and a scalar branch.
        // Where both pyramids are grey-STORED as well (their storage words), the one-channel body stages one-channel tiles
        // from their grey regions: a third of the bytes through the LDS, bytes and derivative words read directly.  Every
        // other pair reads the three-channel regions, which lk_expand_kernel has filled for a grey-stored pyramid of it.
        bool mono = false, grey = false;
        if (prm.mono) {
            const int *wp = svo_pyr_words(prev.lvl[0] - (ptrdiff_t)SVO_PYR_PAD * prev.pitch[0] - SVO_PYR_PAD * C);
            const int *wn = svo_pyr_words(next.lvl[0] - (ptrdiff_t)SVO_PYR_PAD * next.pitch[0] - SVO_PYR_PAD * C);
            mono = uniform(wp[SVO_PYR_MONO] & wn[SVO_PYR_MONO]) != 0;
            grey = mono && uniform((wp[SVO_PYR_STORED] == 1) & (wn[SVO_PYR_STORED] == 1)) != 0;
        }
        // the three-channel body first: it is the fall-through of the branch (colour frames measured 2 us of 700 faster so)
        if (!mono) {
            constexpr int CA = 3, CS = 3, MUL = C / CA;
            static_assert(CA == C || (CA == 1 && C == 3), "the one-channel body is for three equal channels");
#include "lk_levels.hip.h"
        } else if (!grey) {
            constexpr int CA = 1, CS = 3, MUL = C / CA;
            static_assert(CA == C || (CA == 1 && C == 3), "the one-channel body is for three equal channels");
#include "lk_levels.hip.h"
        } else {
            constexpr int CA = 1, CS = 1, MUL = C / CA;
            static_assert(CA == C || (CA == 1 && C == 3), "the one-channel body is for three equal channels");
#include "lk_levels.hip.h"
        }
    } else {
        constexpr int CA = C, CS = C, MUL = C / CA;
        static_assert(CA == C || (CA == 1 && C == 3), "the one-channel body is for three equal channels");
#include "lk_levels.hip.h"
    }

    if (lane == 0) {
        next_pts[2 * p] = outx;
        next_pts[2 * p + 1] = outy;
        status[p] = (uint8_t)st;
        if (err)
            err[p] = st ? errv : 0.f;
        if (min_eig_out)
            min_eig_out[p] = mineig0;
    }
}

// A pair the three-channel-storage bodies must serve although a pyramid of it is grey-stored (the other is colour,
// SVO_LK_MONO=0, a pyramid that never published its mono word): one small launch ahead of the tracking kernel writes the
// pyramid's three-channel levels -- and derivative levels, for the pair's first image -- from its grey ones and marks them
// valid (SVO_PYR_COLOUR_VALID; the pyramid's next build clears the mark).  EXPAND_WGS single-wave workgroups per job and
// image loop over the dwords; in every other case they leave after their scalar loads.
// Whether a slot (job, image) has work does not change during the launch, except through the mark itself.  All workgroups of
// a slot that has work count themselves on the slot's ticket when they are done, and the last one sets the mark: so the
// mark is first set by a slot ALL of whose workgroups did their share, and a workgroup that finds it set (two slots may name
// one pyramid; an earlier launch may have expanded it) skips its share and still counts itself.
constexpr int EXPAND_WGS = 32;
template <int NJ>
__global__ __launch_bounds__(64) void lk_expand_kernel(LkBatchN<NJ> batch, LkParams prm, unsigned *__restrict__ tickets, int force)
{
    svo_chain_priority();
    const LkJob &job = batch.j[blockIdx.z];
    if (job.gate && *job.gate == 0)
        return;
    const PyrDev &prev = job.prev, &next = job.next;
    const bool first = blockIdx.y == 0;
    const PyrDev &pyr = first ? prev : next;
    int *wp = svo_pyr_words(prev.lvl[0] - (ptrdiff_t)SVO_PYR_PAD * prev.pitch[0] - SVO_PYR_PAD * 3);
    int *wn = svo_pyr_words(next.lvl[0] - (ptrdiff_t)SVO_PYR_PAD * next.pitch[0] - SVO_PYR_PAD * 3);
    int *words = first ? wp : wn;
    if (uniform(words[SVO_PYR_STORED]) != 1)
        return;
    // the tracking kernel's own rule for the body that stages the grey regions
    if (!force && prm.mono && uniform(wp[SVO_PYR_MONO] & wn[SVO_PYR_MONO]) != 0 &&
        uniform((wp[SVO_PYR_STORED] == 1) & (wn[SVO_PYR_STORED] == 1)) != 0)
        return;
    const int need = first && job.dprev ? 3 : 1;
    const int todo = need & ~uniform(__hip_atomic_load(&words[SVO_PYR_COLOUR_VALID], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const int tid = blockIdx.x * 64 + threadIdx.x, nthreads = EXPAND_WGS * 64;
    for (int l = 0; l <= prm.max_level; l++) {
        const int w = pyr.w[l], h = pyr.h[l];
        if (todo & 1) {
            // the whole padded buffer, border and all: byte b of a row is byte b / 3 of the grey row (zero past the last pixel)
            const int pitch = pyr.pitch[l], gpitch = svo_grey_pitch(w), nd = pitch >> 2, total = nd * (h + 2 * SVO_PYR_PAD);
            uint8_t *dst = const_cast<uint8_t *>(pyr.lvl[l]) - (ptrdiff_t)SVO_PYR_PAD * pitch - SVO_PYR_PAD * 3;
            const uint8_t *src = pyr.lvl[l] + prm.gdelta[l] - (ptrdiff_t)SVO_PYR_PAD * gpitch - SVO_PYR_PAD;
            for (int i = tid; i < total; i += nthreads) {
                const int row = i / nd, d = i - row * nd;
                unsigned out = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int px = (4 * d + b) / 3;
                    if (px < w + 2 * SVO_PYR_PAD)
                        out |= (unsigned)src[(size_t)row * gpitch + px] << (8 * b);
                }
                reinterpret_cast<unsigned *>(dst + (size_t)row * pitch)[d] = out;
            }
        }
        if (todo & 2) {
            // the interiors: both zero borders stay as they are
            const int dp = prm.dpitch[l] >> 2, gdp = svo_grey_dpitch(w) >> 2, ne = 3 * w, total = ne * h;
            int *dst = const_cast<int *>(job.dprev) + prm.doff[l];
            const int *src = job.dprev + prm.gdoff[l];
            for (int i = tid; i < total; i += nthreads) {
                const int y = i / ne, e = i - y * ne;
                dst[(size_t)y * dp + e] = src[(size_t)y * gdp + e / 3];
            }
        }
    }
    __threadfence();
    unsigned *ticket = tickets + 32 + 2 * blockIdx.z + blockIdx.y;  // slots 32..63 (0..31: fransac.hip, pnp.hip)
    __shared__ unsigned s_last;
    if (threadIdx.x == 0)
        s_last = atomicAdd(ticket, 1u) == EXPAND_WGS - 1;
    __syncthreads();
    if (s_last && threadIdx.x == 0) {
        __threadfence();
        atomicOr(&words[SVO_PYR_COLOUR_VALID], need);
        *ticket = 0;
    }
}

__global__ void grid_keypoints_kernel(int rows, int cols, int step, int nx, int total,
                                      float *__restrict__ out_xy)
{
    __builtin_amdgcn_s_setprio(3);  // short latency-bound kernel: win issue arbitration against co-resident LK waves
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total)
        return;
    int gy = i / nx, gx = i - gy * nx;
    out_xy[2 * i] = (float)((gx + 1) * step);
    out_xy[2 * i + 1] = (float)((gy + 1) * step);
}

}  // namespace

int svo_launch_lk_batch(svo_ctx *ctx, int n_jobs, const LkJob *jobs, const svo_pyramid *geom)
{
    if (n_jobs <= 0)
        return SVO_OK;
    if (n_jobs > SVO_LK_MAX_JOBS) {
        svo_set_error("lk: at most %d jobs per launch", SVO_LK_MAX_JOBS);
        return SVO_ERR_ARG;
    }
    LkBatch batch;
    int n_max = 0, c = jobs[0].prev.c, levels = jobs[0].prev.levels;
    for (int k = 0; k < n_jobs; k++) {
        batch.j[k] = jobs[k];
        n_max = jobs[k].n_cap > n_max ? jobs[k].n_cap : n_max;
        if (jobs[k].prev.c != c || jobs[k].prev.levels != levels || jobs[k].prev.w[0] != geom->w ||
            jobs[k].prev.h[0] != geom->h || !jobs[k].dprev) {
            svo_set_error("lk: the jobs of one launch must share their pyramid geometry and carry derivative levels");
            return SVO_ERR_ARG;
        }
    }
    for (int k = n_jobs; k < SVO_LK_MAX_JOBS; k++)
        batch.j[k] = jobs[0];
    if (n_max == 0)
        return SVO_OK;
    LkBatchN<1> one;
    one.j[0] = jobs[0];
    LkParams prm;
    prm.max_level = levels - 1;
    prm.max_count = 30;
    prm.eps_sq = 0.01 * 0.01;
    prm.eps_pre = 0.0101f;
    prm.min_eig_thr = (float)1e-4;
    for (int l = 0; l < SVO_MAX_LEVELS; l++) {
        prm.doff[l] = (int)geom->doff[l];
        prm.dpitch[l] = geom->dpitch[l];
        prm.gdelta[l] = geom->gdelta[l];
        prm.gdoff[l] = (int)geom->gdoff[l];
    }
    static const int lone_interleave = getenv("SVO_LK_INTERLEAVE") ? atoi(getenv("SVO_LK_INTERLEAVE")) : 1;  // A/B: +2.8 % frames/s for one chunk per GPU
    // Round 4: the launches of the lock-step groups deal their keypoints round-robin too.  Until then XCD x was given the
    // x-th eighth of every job's list ("one band of the image per L2"): +11 % frames/s for dropping that (11.17 k -> 12.4 k, three
    // alternating runs on one box) -- the L2-miss bytes a spatial order saves cost the kernel no time, the imbalance between
    // the bands does (profiles/r04_lk_locality.txt: the order that fetches 5 x the bytes is the fastest).  SVO_LK_INTERLEAVE_BATCH=0
    // restores the bands for an A/B.
    static const int batch_interleave = getenv("SVO_LK_INTERLEAVE_BATCH") ? atoi(getenv("SVO_LK_INTERLEAVE_BATCH")) : 1;
    prm.interleave = n_jobs <= 2 ? lone_interleave : batch_interleave;  // two jobs: the two candidate passes of a pipelined chunk
    // the identity path for windows on integer positions (step 1 of the kernel) computes what the interpolating path
    // computes; SVO_LK_LATTICE=0 switches it off for an A/B and for the tests that compare the two
    static const int lattice = getenv("SVO_LK_LATTICE") ? atoi(getenv("SVO_LK_LATTICE")) : 1;
    prm.lattice = lattice;
    // the iteration loop keeps a lane's column pairs while the guess stays in its pixel cell; SVO_LK_CELL_CACHE=0 reloads
    // them in every iteration (the same values), for an A/B and for the tests that compare the two
    static const int cell_cache = getenv("SVO_LK_CELL_CACHE") ? atoi(getenv("SVO_LK_CELL_CACHE")) : 1;
    prm.cell_cache = cell_cache;
    // grey frames stored as BGR take the one-channel body (the kernel's own choice per job, from the pyramids' words);
    // SVO_LK_MONO=0 keeps the three-channel arithmetic (the same values), for an A/B and for the tests that compare the two
    static const int mono = getenv("SVO_LK_MONO") ? atoi(getenv("SVO_LK_MONO")) : 1;
    prm.mono = mono;
    // the level-0 residual is compiled in only where some job of the launch asks for it
    bool want_err = false;
    for (int k = 0; k < n_jobs; k++)
        want_err = want_err || jobs[k].err != nullptr;
    dim3 grid(((n_max + 7) / 8 + WAVES - 1) / WAVES * 8, n_jobs), block(64 * WAVES);  // x: a multiple of 8, every XCD band has all its slots
    ScopedKernelTime t(ctx, SVO_K_LK);
    if (c != 1 && c != 3) {
        svo_set_error("lk: unsupported channel count %d (1 or 3)", c);
        return SVO_ERR_ARG;
    }
    if (c == 3) {
        // grey-stored pyramids of pairs that the three-channel-storage bodies will serve (lk_expand_kernel)
        if (n_jobs == 1)
            hipLaunchKernelGGL((lk_expand_kernel<1>), dim3(EXPAND_WGS, 2, 1), dim3(64), 0, ctx->stream, one, prm, ctx->d_tickets, 0);
        else
            hipLaunchKernelGGL((lk_expand_kernel<SVO_LK_MAX_JOBS>), dim3(EXPAND_WGS, 2, n_jobs), dim3(64), 0, ctx->stream, batch, prm,
                               ctx->d_tickets, 0);
    }
    auto launch = [&](auto c_c, auto err_c) {
        constexpr int CC = decltype(c_c)::value;
        constexpr bool WE = decltype(err_c)::value;
        if (n_jobs == 1)
            hipLaunchKernelGGL((lk_track_kernel<CC, 1, WE>), grid, block, WAVES * Lds<CC>::WAVE_BYTES, ctx->stream, one, prm);
        else
            hipLaunchKernelGGL((lk_track_kernel<CC, SVO_LK_MAX_JOBS, WE>), grid, block, WAVES * Lds<CC>::WAVE_BYTES,
                               ctx->stream, batch, prm);
    };
    using one_c = std::integral_constant<int, 1>;
    using three_c = std::integral_constant<int, 3>;
    if (c == 1)
        want_err ? launch(one_c(), std::true_type()) : launch(one_c(), std::false_type());
    else
        want_err ? launch(three_c(), std::true_type()) : launch(three_c(), std::false_type());
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

int svo_launch_lk(svo_ctx *ctx, svo_pyramid *prev, const svo_pyramid *next, const float *prev_pts, int n,
                  float *next_pts, uint8_t *status, float *err, float *min_eig, const int *d_n)
{
    if (n == 0)
        return SVO_OK;
    if (!prev->has_deriv) {  // a pyramid built without its derivative levels: derive them now
        int rc = svo_build_derivatives(ctx, 1, &prev);
        if (rc)
            return rc;
    }
    LkJob job;
    job.prev = prev->dev;
    job.next = next->dev;
    job.dprev = prev->dbase;
    job.prev_pts = prev_pts;
    job.n_cap = n;
    job.d_n = d_n;
    job.next_pts = next_pts;
    job.status = status;
    job.err = err;
    job.min_eig = min_eig;
    return svo_launch_lk_batch(ctx, 1, &job, prev);
}

int svo_expand_grey_storage(svo_ctx *ctx, const svo_pyramid *pyr, bool deriv)
{
    if (pyr->c != 3)
        return SVO_OK;
    LkBatchN<1> one;
    LkJob &job = one.j[0];
    job.prev = job.next = pyr->dev;
    job.dprev = deriv ? pyr->dbase : nullptr;
    job.prev_pts = job.next_pts = job.err = job.min_eig = nullptr;
    job.status = nullptr;
    job.d_n = nullptr;
    job.n_cap = 0;
    LkParams prm = {};
    prm.max_level = pyr->levels - 1;
    for (int l = 0; l < SVO_MAX_LEVELS; l++) {
        prm.doff[l] = (int)pyr->doff[l];
        prm.dpitch[l] = pyr->dpitch[l];
        prm.gdelta[l] = pyr->gdelta[l];
        prm.gdoff[l] = (int)pyr->gdoff[l];
    }
    hipLaunchKernelGGL((lk_expand_kernel<1>), dim3(EXPAND_WGS, 2, 1), dim3(64), 0, ctx->stream, one, prm, ctx->d_tickets, 1);
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

// number of lattice points of the reference's loop `for (v = s; v < dim - s; v += s)`
static int grid_axis_count(int dim, int step)
{
    int k = 0;
    for (int v = step; v < dim - step; v += step)
        k++;
    return k;
}

int svo_launch_grid(svo_ctx *ctx, int rows, int cols, int step, float *out_xy, int cap)
{
    int nx = grid_axis_count(cols, step), ny = grid_axis_count(rows, step);
    int total = nx * ny;
    if (total > cap)
        total = cap;
    if (total <= 0)
        return SVO_OK;
    hipLaunchKernelGGL(grid_keypoints_kernel, dim3((total + 255) / 256), dim3(256), 0, ctx->stream, rows,
                       cols, step, nx, total, out_xy);
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

extern "C" {

int svo_grid_keypoints(svo_ctx *ctx, int rows, int cols, int step, float *out_xy, int cap, int mem,
                       int *count)
{
    SVO_CHECK_ARG(ctx && step > 0 && rows > 0 && cols > 0 && cap >= 0);
    int total = grid_axis_count(cols, step) * grid_axis_count(rows, step);
    if (count)
        *count = total;
    if (!out_xy)
        return SVO_OK;
    if (total > cap) {
        svo_set_error("grid: %d keypoints exceed capacity %d", total, cap);
        return SVO_ERR_CAPACITY;
    }
    if (total == 0)
        return SVO_OK;
    float *d = out_xy;
    if (mem == SVO_MEM_HOST) {
        int rc = ctx->s_a.ensure((size_t)total * 8);
        if (rc)
            return rc;
        d = ctx->s_a.as<float>();
    }
    int rc = svo_launch_grid(ctx, rows, cols, step, d, total);
    if (rc)
        return rc;
    if (mem == SVO_MEM_HOST) {
        SVO_HIP(hipMemcpyAsync(out_xy, d, (size_t)total * 8, hipMemcpyDeviceToHost, ctx->stream));
        SVO_HIP(hipStreamSynchronize(ctx->stream));
    }
    return SVO_OK;
}

int svo_lk_track(svo_ctx *ctx, const svo_pyramid *prev, const svo_pyramid *next, const float *prev_pts,
                 int n, float *next_pts, uint8_t *status, float *err, float *min_eig, int mem)
{
    SVO_CHECK_ARG(ctx && prev && next && n >= 0);
    SVO_CHECK_ARG(prev->w == next->w && prev->h == next->h && prev->c == next->c &&
                  prev->levels == next->levels);
    SVO_CHECK_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE);
    if (n == 0)
        return SVO_OK;
    SVO_CHECK_ARG(prev_pts && next_pts && status);
    svo_pyramid *pv = const_cast<svo_pyramid *>(prev);  // its derivative levels may be filled in on first use
    if (mem == SVO_MEM_DEVICE)
        return svo_launch_lk(ctx, pv, next, prev_pts, n, next_pts, status, err, min_eig, nullptr);

    int rc;
    if ((rc = ctx->s_a.ensure((size_t)n * 8)) || (rc = ctx->s_b.ensure((size_t)n * 8)) ||
        (rc = ctx->s_c.ensure((size_t)n)) || (rc = ctx->s_d.ensure((size_t)n * 4)) ||
        (rc = ctx->s_e.ensure((size_t)n * 4)))
        return rc;
    SVO_HIP(hipMemcpyAsync(ctx->s_a.p, prev_pts, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    rc = svo_launch_lk(ctx, pv, next, ctx->s_a.as<float>(), n, ctx->s_b.as<float>(),
                       ctx->s_c.as<uint8_t>(), ctx->s_d.as<float>(), ctx->s_e.as<float>(), nullptr);
    if (rc)
        return rc;
    SVO_HIP(hipMemcpyAsync(next_pts, ctx->s_b.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipMemcpyAsync(status, ctx->s_c.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (err)
        SVO_HIP(hipMemcpyAsync(err, ctx->s_d.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (min_eig)
        SVO_HIP(hipMemcpyAsync(min_eig, ctx->s_e.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

}  // extern "C"
