// Fragment of the cone translation unit (ffa_kernels.hip), device code only:
// the fused boxcar S/N of a final pass's output level (row-group form
// snr_rows / snr_epilogue, segmented form snr_segments).
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "cone_merge.hpp"
#include "cone_unit.hpp"

namespace rt {

template <int CTRL>
__device__ __forceinline__ double dpp_d(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}

// row_shr:d within 16-lane rows: lane g (of a G-lane group, G <= 16) takes
// lane g - d of its group when g >= d.
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_d_rows(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWS, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWS, 0xF, false);
    return __hiloint2double(hi, lo);
}

// Inclusive scan over each G-lane group (G = 2 .. 64): row_shr steps inside
// 16-lane rows, then row_bcast:15 / row_bcast:31 across rows.  The partial
// sums start at +0.0 and are never -0.0, so adding the +0.0 that masked
// lanes receive is an exact no-op.
template <int G>
__device__ __forceinline__ double seg_scan_dpp(double v, int lane)
{
    const int g = lane & (G < 16 ? G - 1 : 15);     // position inside the group's part of the 16-lane row
    double y = dpp_d<0x111>(v);
    v = g >= 1 ? v + y : v;
    if (G >= 4) {
        y = dpp_d<0x112>(v);
        v = g >= 2 ? v + y : v;
    }
    if (G >= 8) {
        y = dpp_d<0x114>(v);
        v = g >= 4 ? v + y : v;
    }
    if (G >= 16) {
        y = dpp_d<0x118>(v);
        v = g >= 8 ? v + y : v;
    }
    if (G >= 32) v = v + dpp_d_rows<0x142, 0xA>(v);   // rows 1, 3 += lane 15 of rows 0, 2
    if (G >= 64) v = v + dpp_d_rows<0x143, 0xC>(v);   // rows 2, 3 += lane 31
    return v;
}

// diff_max (kernels.hpp:50-60) of width W over the lane's columns (cp[i] =
// +inf past the lane's chunk, so those differences are -inf).
// v_sub_f32 / v_max3_f32 as volatile asm: the width's work stays inside its
// switch case (from plain code the compiler evaluated every case -- all
// kSnrWin widths -- ahead of the width loop in every row pass).  v_max3_f32
// (IEEE mode) never returns a quiet-NaN operand over a number, as diff_max's
// comparison (kernels.hpp:50-60).
template <int CH, int W>
__device__ __forceinline__ float window_max(const float (&z)[CH + kSnrWin], const float (&cp)[CH])
{
    float dm = -INFINITY;
#pragma unroll
    for (int i = 0; i + 1 < CH; i += 2) {
        float t0, t1;
        asm volatile("v_sub_f32 %1, %3, %4\n\tv_sub_f32 %2, %5, %6\n\tv_max3_f32 %0, %0, %1, %2"
                     : "+v"(dm), "=&v"(t0), "=&v"(t1)
                     : "v"(z[i + W]), "v"(cp[i]), "v"(z[i + 1 + W]), "v"(cp[i + 1]));
    }
    if constexpr (CH & 1) {
        float t0;
        asm volatile("v_sub_f32 %1, %2, %3\n\tv_max_f32 %0, %0, %1"
                     : "+v"(dm), "=&v"(t0)
                     : "v"(z[CH - 1 + W]), "v"(cp[CH - 1]));
    }
    return dm;
}

// width dispatch: one switch (a jump, not a chain of scalar compares)
template <int CH>
__device__ __forceinline__ float window_dispatch(int w, const float (&z)[CH + kSnrWin], const float (&cp)[CH])
{
    static_assert(kSnrWin == 12, "cases below");
    switch (w) {
    case 1: return window_max<CH, 1>(z, cp);
    case 2: return window_max<CH, 2>(z, cp);
    case 3: return window_max<CH, 3>(z, cp);
    case 4: return window_max<CH, 4>(z, cp);
    case 5: return window_max<CH, 5>(z, cp);
    case 6: return window_max<CH, 6>(z, cp);
    case 7: return window_max<CH, 7>(z, cp);
    case 8: return window_max<CH, 8>(z, cp);
    case 9: return window_max<CH, 9>(z, cp);
    case 10: return window_max<CH, 10>(z, cp);
    case 11: return window_max<CH, 11>(z, cp);
    case 12: return window_max<CH, 12>(z, cp);
    default: return -INFINITY;
    }
}

// The standard ladder of small boxcar widths: generate_width_trials
// (ffautils.py:3-10) with wtsp 1.5 always starts 1, 2, 3, 4, 6, 9 (every
// BASELINE config: W = 6 or 10 from 240 bins).  When a plan's widths begin
// with it, the S/N evaluates those six window maxima in one straight block
// (independent v_max3 chains the compiler may interleave, no width switch,
// one interleaved DPP all-reduce), instead of one switch case and one
// all-reduce per width.  Same float operations, same results.
constexpr int kStdWidths[6] = {1, 2, 3, 4, 6, 9};

template <int CH, int W>
__device__ __forceinline__ float window_max_nv(const float (&z)[CH + kSnrWin], const float (&cp)[CH])
{
    // diff_max (kernels.hpp:50-60) as window_max, without volatile: the six
    // widths' chains are independent and may be interleaved
    float dm = -INFINITY;
#pragma unroll
    for (int i = 0; i + 1 < CH; i += 2) {
        float t0, t1;
        asm("v_sub_f32 %1, %3, %4\n\tv_sub_f32 %2, %5, %6\n\tv_max3_f32 %0, %0, %1, %2"
            : "+v"(dm), "=&v"(t0), "=&v"(t1)
            : "v"(z[i + W]), "v"(cp[i]), "v"(z[i + 1 + W]), "v"(cp[i + 1]));
    }
    if constexpr (CH & 1) {
        float t0;
        asm("v_sub_f32 %1, %2, %3\n\tv_max_f32 %0, %0, %1" : "+v"(dm), "=&v"(t0) : "v"(z[CH - 1 + W]), "v"(cp[CH - 1]));
    }
    return dm;
}

// one v_max_f32 with a DPP source per value and step, six values interleaved
// (each DPP reads a register written six instructions earlier: no wait states)
#define RT_MAX6_STEP(CTRL)                                                                                  \
    asm volatile("v_max_f32_dpp %0, %0, %0 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                        \
                 "v_max_f32_dpp %1, %1, %1 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                        \
                 "v_max_f32_dpp %2, %2, %2 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                        \
                 "v_max_f32_dpp %3, %3, %3 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                        \
                 "v_max_f32_dpp %4, %4, %4 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                        \
                 "v_max_f32_dpp %5, %5, %5 " CTRL " row_mask:0xf bank_mask:0xf"                              \
                 : "+v"(m[0]), "+v"(m[1]), "+v"(m[2]), "+v"(m[3]), "+v"(m[4]), "+v"(m[5]))

// The six standard widths' row maxima all-reduced over each G-lane group
// (grp_allmax for six values at once); lane g of a group then keeps width g.
template <int CH, int G>
__device__ __forceinline__ float snr_std6(const float (&z)[CH + kSnrWin], const float (&cp)[CH], int g)
{
    static_assert(G == 8 || G == 16, "one DPP row per group");
    float m[6] = {window_max_nv<CH, 1>(z, cp), window_max_nv<CH, 2>(z, cp), window_max_nv<CH, 3>(z, cp),
                  window_max_nv<CH, 4>(z, cp), window_max_nv<CH, 6>(z, cp), window_max_nv<CH, 9>(z, cp)};
    asm volatile("s_nop 1" ::: "memory");
    RT_MAX6_STEP("quad_perm:[1,0,3,2]");
    RT_MAX6_STEP("quad_perm:[2,3,0,1]");
    RT_MAX6_STEP("row_half_mirror");
    if constexpr (G >= 16) RT_MAX6_STEP("row_mirror");
    float r = m[0];
#pragma unroll
    for (int i = 1; i < 6; ++i) r = g == i ? m[i] : r;
    return r;
}
#undef RT_MAX6_STEP

// The short rows' standard ladder 1, 2, 3 (generate_width_trials from 16-32
// bins: BASELINE configs[3]) in 4-lane groups: three independent window
// maxima and one interleaved quad all-reduce (each DPP reads a register
// written three instructions earlier), instead of a width switch and an
// all-reduce with its wait states per width.  Same float operations.
#define RT_MAX3_STEP(CTRL)                                                                                  \
    asm volatile("v_max_f32_dpp %0, %0, %0 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                        \
                 "v_max_f32_dpp %1, %1, %1 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                        \
                 "v_max_f32_dpp %2, %2, %2 " CTRL " row_mask:0xf bank_mask:0xf"                              \
                 : "+v"(m[0]), "+v"(m[1]), "+v"(m[2]))

template <int CH>
__device__ __forceinline__ float snr_std3(const float (&z)[CH + kSnrWin], const float (&cp)[CH], int g)
{
    float m[3] = {window_max_nv<CH, 1>(z, cp), window_max_nv<CH, 2>(z, cp), window_max_nv<CH, 3>(z, cp)};
    asm volatile("s_nop 1" ::: "memory");
    RT_MAX3_STEP("quad_perm:[1,0,3,2]");
    RT_MAX3_STEP("quad_perm:[2,3,0,1]");
    return g == 0 ? m[0] : (g == 1 ? m[1] : m[2]);
}
#undef RT_MAX3_STEP


#ifdef RT_STAMPS
#define RT_SNR_MARK(i)                                                           \
    do {                                                                         \
        if (tid == 0 && base == 0 && tl) tl[i] = __builtin_amdgcn_s_memtime();   \
    } while (0)
#else
#define RT_SNR_MARK(i) do { } while (0)
#endif

// Per-width constants of the S/N formula (snr.hpp:37-65): h + b and b of
// width w over p bins.
__device__ __forceinline__ void snr_width_consts(int w, int p, float* out)
{
    const float h = sqrtf((float)(p - w) / (float)(p * w));
    const float b = (float)w / (float)(p - w) * h;
    out[0] = h + b;
    out[1] = b;
}

// max over each G-lane group (G = 2 .. 64, groups aligned), in every lane
// of the group: quad swaps, then the half-row and row mirrors, then (G >= 32)
// cross-row exchanges (max never returns a NaN operand over a number, as
// diff_max's comparison)
template <int G>
__device__ __forceinline__ float grp_allmax(float v)
{
    static_assert(G == 2 || G == 4 || G == 8 || G == 16 || G == 32 || G == 64, "lane groups");
    // v_max_f32 with a DPP source (no canonicalising moves around a
    // separate DPP move); s_nop 1: the DPP read of a VGPR written by the
    // previous VALU instruction
    asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "+v"(v));
    if constexpr (G >= 4)
        asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "+v"(v));
    if constexpr (G >= 8)
        asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf" : "+v"(v));
    if constexpr (G >= 16)
        asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf" : "+v"(v));
    // 32- and 64-lane groups: lane i <-> i ^ 16 by ds_swizzle (xor mask 16
    // inside 32 lanes), lane i <-> i ^ 32 by ds_bpermute
    if constexpr (G >= 32) v = fmaxf(v, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F)));
    if constexpr (G == 64) v = fmaxf(v, __shfl_xor(v, 32, 64));
    return v;
}

// Fused boxcar S/N (snr.hpp:37-65) of the output rows s < rows_eval held in
// LDS (row stride q): G lanes per row, each lane a chunk of c <= CH columns
// held in registers (c odd: the G chunks of a row start on distinct banks).
// fp64 prefix: sequential in the chunk + log2(G)-step segmented scan
// (kernels.hpp:73-86).  For G <= 16 (one DPP row) the scan and the width
// maxima's all-reduce run on DPP row shifts (VALU, no LDS round trip); each
// lane then reads its window c[j0 .. j0 + CH + kSnrWin) (the wrap c[p + j] =
// c[j] + sum applied once per element) and evaluates every width w <= kSnrWin
// from registers.  Wider widths read LDS per width.  Transposed emit: the
// row's max of width iw goes to every lane of its group (DPP all-reduce) and
// lane g keeps widths g, g + G, ...; one S/N formula (one fp32 division) and
// one store per lane and slot after the widths, the stores of a row
// consecutive.  Row passes without workgroup barriers: a row's G <= 64 lanes
// are one wave, and a wave's LDS accesses complete in order.
// (kSnrWin, kSnrMaxChunk: common.hpp)
template <int CH, int G, bool WIDE = false>
__device__ __forceinline__ void snr_rows(const ConeArgs& a, const UnitView& U, float* data, int q, const int* wl,
                                         int nev, int c, int tid, const float* whb, unsigned long long* tl)
{
    const int lane = tid & 63;
    const int p = U.p;
    const int g = lane & (G - 1);
    // rows with room for the wrapped prefix extension (final-pass output
    // levels at the S/N stride); only the register-window path uses it
    const bool ext = CH <= kSnrMaxChunk && q >= p + kSnrWin;
    // WIDE (the caller checked snr_wide_ok): every width past the register
    // window read as a plain LDS window, the wrapped prefix stored up to
    // p + wmax
    const int next = WIDE ? wl[kMaxWidths] : kSnrWin;   // wrapped prefix words stored past p
    // rows with room past p for a lane's whole CH-column prefix write
    const bool wfull = q >= p + CH;
    // lanes past the row keep their natural chunk start g * c (their
    // columns are masked) where the row stride holds every lane's chunk:
    // clamped to p they read the banks of another row's lane (a 2-way
    // conflict on every chunk and window read at p = 240-254)
    const bool natural = ext && wfull && (G - 1) * c + CH <= q;
    int j0 = natural ? g * c : min(g * c, p);
    int cnt = max(min(j0 + c, p) - j0, 0);        // columns of this lane (may be 0)
    const int owner = (p - 1) / c;
    constexpr int rows_per_pass = kConeBlock / G;
    constexpr int writer = G - 1;
    (void)writer;
    const uint32_t nw = a.num_widths;
    float* snr = a.snr + (uint64_t)U.trial * a.snr_stride + (U.snr_row + (uint64_t)U.s0) * (uint64_t)nw;
    const __amdgpu_buffer_rsrc_t srs = buffer_rsrc(snr, (uint32_t)nev * nw * 4u);
    // the widths in lanes (lane i: width i), taken per width by v_readlane
    // instead of an LDS read and its wait
    const int wlane = wl[min(lane, (int)nw - 1)];
    // the plan's widths begin with the standard ladder 1, 2, 3, 4, 6, 9
    bool std6 = nw >= 6;
#pragma unroll
    for (int i = 0; i < 6; ++i) std6 = std6 && __builtin_amdgcn_readlane(wlane, i) == kStdWidths[i];
    // ... or begin 1, 2, 3 in 4-lane groups (short rows)
    bool std3 = G == 4 && nw >= 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) std3 = std3 && __builtin_amdgcn_readlane(wlane, i) == kStdWidths[i];
    for (int base = 0; base < nev; base += rows_per_pass) {
        // opaque per row pass: the column masks (i < cnt, j0 + k >= p) are
        // recomputed by one v_cmp each instead of being hoisted out of the
        // loop into SGPR pairs that spill (two v_readlane per use)
        asm volatile("" : "+v"(j0), "+v"(cnt));
        const int r = base + (tid / G);
        const bool active = r < nev;
        float* const row = data + min(r, nev - 1) * q + j0;
        float cp[CH];
        // every lane reads CH columns at immediate offsets (past its chunk:
        // the next chunk, the next row or the LDS pad), masked to 0
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const float x = row[i];
            cp[i] = i < cnt ? x : 0.0f;
            // the select on the float, before the fp64 conversion (else two
            // selects on the converted halves)
            asm("" : "+v"(cp[i]));
        }
        // fp64 prefix: the masked columns add +0.0 (the partial sums start at
        // +0.0 and are never -0.0, so the additions are exact no-ops)
        double part = 0.0;
#pragma unroll
        for (int i = 0; i < CH; ++i) part = part + (double)cp[i];
        double acc = dpp_d<0x138>(seg_scan_dpp<G>(part, lane));   // wave_shr:1 -- lane g takes lane g - 1
        if (g == 0) acc = 0.0;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            acc = acc + (double)cp[i];
            cp[i] = (float)acc;
        }
        const float sum = __shfl((float)acc, owner, G);
        {
            // columns past the lane's chunk (and rows past nev) go to dummy
            // words in the LDS pad: a base select per column (the column an
            // immediate offset) instead of exec masks
            typedef __attribute__((address_space(3))) float* lds_ptr;
            if (wfull) {
                // every lane of an active row writes all CH columns, last
                // column first: a column past the lane's chunk is the next
                // lane's column i - c, which that lane writes later (a
                // wave's LDS writes land in order), or lies past the row
                // inside its stride (q >= p + CH)
                if (active) {
                    // volatile: the compiler keeps the descending order
                    volatile __attribute__((address_space(3))) float* const rk =
                        (volatile __attribute__((address_space(3))) float*)row;
#pragma unroll
                    for (int i = CH - 1; i >= 0; --i) rk[i] = cp[i];
                }
            } else {
                // one dummy word per lane and column (the same word for
                // every lane serialised those stores on one bank)
                const lds_ptr dummy = (lds_ptr)(data + kLdsDataFloats + 4 + lane);
                int cw = active ? cnt : 0;
                asm("" : "+v"(cw));
                const lds_ptr rk = (lds_ptr)row;
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    lds_ptr b = i < cw ? rk : dummy;
                    asm("" : "+v"(b));
                    b[i] = cp[i];
                }
            }
        }
        // rows at a stride q >= p + kSnrWin: the wrapped prefix c[p + j] =
        // c[j] + sum (kernels.hpp:88-97, j < kSnrWin, or j < wmax on the wide
        // stride) stored after the row by its own lanes (the wave's LDS
        // accesses complete in order), so the window reads below take
        // c[j0 .. j0 + CH + kSnrWin) -- and c[j0 + w ..] -- without a wrap
        const float* const crow = data + min(r, nev - 1) * q;
        if (ext) {
            float* const rb = data + min(r, nev - 1) * q;
            auto put = [&](int e) {
                if (active && e < next)
                    *(volatile __attribute__((address_space(3))) float*)(rb + p + e) =
                        __fadd_rn(lds_ld((lds_cptr)(rb + e)), sum);
            };
            if constexpr (WIDE) {
                for (int e0 = 0; e0 < next; e0 += G) put(e0 + g);
            } else {
#pragma unroll
                for (int e0 = 0; e0 < kSnrWin; e0 += G) put(e0 + g);
            }
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) cp[i] = i < cnt ? cp[i] : INFINITY;
        RT_SNR_MARK(7);
        // a row's lanes are one wave: its prefix writes are seen by its
        // window reads below without a workgroup barrier (a compiler barrier
        // only), so the waves of a unit run their row passes independently
        __asm__ __volatile__("" ::: "memory");
        RT_SNR_MARK(8);
        constexpr int NSEL = (kMaxWidths + G - 1) / G;
        float sel[NSEL] = {};
        auto emit = [&](uint32_t iw, float dmax) {
            const float dm = grp_allmax<G>(dmax);
#pragma unroll
            for (int sl = 0; sl < NSEL; ++sl)
                if (sl * G < (int)nw) sel[sl] = (int)iw == g + sl * G ? dm : sel[sl];
        };
        if constexpr (CH <= kSnrMaxChunk) {
            // widths <= kSnrWin from the register window c[j0 .. j0 + CH + kSnrWin)
            float z[CH + kSnrWin];
            // two opaque bases (row and row - p), slot offsets immediate; one
            // volatile read per element from the selected base (a plain read
            // of each base was sunk into a branch per element, each with its
            // own s_waitcnt lgkmcnt(0): 29 serialised LDS round trips per row
            // pass)
            lds_cptr za = (lds_cptr)(crow + j0);
            lds_cptr zb = za - p;
            asm("" : "+v"(za), "+v"(zb));
            if (ext) {
                // past the row: its wrapped extension (or, past that, words
                // only differences with masked columns read)
#pragma unroll
                for (int t = 0; t < CH + kSnrWin; ++t) z[t] = lds_ld(za + t);
            } else {
                // the wrap term as an addend (+0.0 before the wrap point: the
                // prefix values are never -0.0, so x + 0.0 == x exactly), so
                // no compare mask lives across the reads
                float x[CH + kSnrWin], ad[CH + kSnrWin];
#pragma unroll
                for (int t = 0; t < CH + kSnrWin; ++t) {
                    const bool wrap = j0 + t >= p;
                    ad[t] = wrap ? sum : 0.0f;
                    x[t] = lds_ld((wrap ? zb : za) + t);
                }
#pragma unroll
                for (int t = 0; t < CH + kSnrWin; ++t) z[t] = __fadd_rn(x[t], ad[t]);
            }
            RT_SNR_MARK(9);
            uint32_t iw0 = 0;
            if constexpr (G == 8 || G == 16) {
                if (std6) {
                    // widths 0-5 are the standard ladder: lane g < 6 keeps width g
                    sel[0] = snr_std6<CH, G>(z, cp, g);
                    iw0 = 6;
                }
            }
            if constexpr (G == 4) {
                if (std3) {
                    // widths 0-2 are 1, 2, 3: lane g < 3 keeps width g
                    sel[0] = snr_std3<CH>(z, cp, g);
                    iw0 = 3;
                }
            }
            for (uint32_t iw = iw0; iw < nw; ++iw) {
                const int w = __builtin_amdgcn_readlane(wlane, (int)iw);
                if (w <= kSnrWin) emit(iw, window_dispatch<CH>(w, z, cp));
            }
        }
        // wider widths: the window c[j0 + w ..] read from LDS per width
        for (uint32_t iw = 0; iw < nw; ++iw) {
            const int w = __builtin_amdgcn_readlane(wlane, (int)iw);
            if (CH <= kSnrMaxChunk && w <= kSnrWin) continue;
            if constexpr (CH <= kSnrMaxChunk) {
                // c[j0 + w + t] for the lane's columns t at immediate offsets:
                // WIDE, inside the row or its stored extension; else the wrap
                // (j >= p) as a second base za - p and the addend sum (+0.0
                // before the wrap point: exact, the prefix values are never
                // -0.0).  Columns past the chunk read words whose differences
                // with cp = +inf are dropped.
                lds_cptr za = (lds_cptr)(crow + j0 + w);
                lds_cptr zb = za - p;
                asm("" : "+v"(za), "+v"(zb));
                float d[CH];
                if constexpr (WIDE) {
#pragma unroll
                    for (int t = 0; t < CH; ++t) d[t] = __fsub_rn(lds_ld(za + t), cp[t]);   // diff_max, kernels.hpp:50-60
                } else {
                    const int tw = p - j0 - w;        // first wrapped column
                    float x[CH], ad[CH];
#pragma unroll
                    for (int t = 0; t < CH; ++t) {
                        const bool wrap = t >= tw;
                        ad[t] = wrap ? sum : 0.0f;
                        x[t] = lds_ld((wrap ? zb : za) + t);
                    }
#pragma unroll
                    for (int t = 0; t < CH; ++t) d[t] = __fsub_rn(__fadd_rn(x[t], ad[t]), cp[t]);
                }
                float m = d[0];
#pragma unroll
                for (int t = 1; t + 1 < CH; t += 2) m = fmaxf(m, fmaxf(d[t], d[t + 1]));
                if constexpr (CH % 2 == 0) m = fmaxf(m, d[CH - 1]);
                emit(iw, m);
                continue;
            }
            const int last = max(cnt - 1, 0);
            float dmax = -INFINITY;
            float lv[CH];
#pragma unroll
            for (int t = 0; t < CH; ++t) {
                const int j = j0 + min(t, last) + w;
                lv[t] = crow[j >= p ? j - p : j];
            }
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const bool wrap = j0 + min(i, last) + w >= p;
                const float ck = wrap ? __fadd_rn(lv[i], sum) : lv[i];
                dmax = fmaxf(dmax, __fsub_rn(ck, cp[i]));  // diff_max, kernels.hpp:50-60
            }
            emit(iw, dmax);
        }
#pragma unroll
        for (int sl = 0; sl < NSEL; ++sl) {
            if (sl * G < (int)nw) {
                const int iw = g + sl * G;
                const int iwc = min(iw, (int)nw - 1);
                const float hpb = whb[2 * iwc], b = whb[2 * iwc + 1];
                const float v = (hpb * sel[sl] - b * sum) / U.stdnoise;
                const uint32_t o = (active && iw < (int)nw) ? ((uint32_t)r * nw + (uint32_t)iw) * 4u : 0x80000000u;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), srs, (int)o, 0, kSnrCpol);
            }
        }
        RT_SNR_MARK(10);
    }
}

typedef float f2v __attribute__((ext_vector_type(2)));

// diff_max (kernels.hpp:50-60) of width W over the S = 2 K + 1 window starts
// of a segment, c[0 .. S + W) in K + 5 register pairs P (P[k] = c[2k],
// c[2k + 1]) and, for odd W, the shifted pairs H[k] = c[2k + 1], c[2k + 2]:
// max_i c[i + W] - c[i], two differences per v_pk_add_f32 (negated second
// operand: x + (-y) == x - y, signed zeros included) and one v_max3_f32.
template <int K, int W>
__device__ __forceinline__ float seg_window_max(const f2v (&P)[K + 5], const f2v (&H)[K + 4])
{
    float dm = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const f2v hi = (W & 1) ? H[k + (W - 1) / 2] : P[k + W / 2];
        f2v d;
        asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(hi), "v"(P[k]));
        asm("v_max3_f32 %0, %0, %1, %2" : "+v"(dm) : "v"(d.x), "v"(d.y));
    }
    // the last start, 2K
    constexpr int e = 2 * K + W;
    const float ce = (e & 1) ? P[e / 2].y : P[e / 2].x;
    float t;
    asm("v_sub_f32 %1, %2, %3\n\tv_max_f32 %0, %0, %1" : "+v"(dm), "=&v"(t) : "v"(ce), "v"(P[K].x));
    return dm;
}

// Segmented boxcar S/N (snr.hpp:37-65, kernels.hpp:50-101) of a final level
// of <= 64 rows of 240-264 bins, row r at slot + r * kSnrSegStride + r0 (r0 =
// 8 S - p <= 24 columns of slack in front of the row): lane = row, wave w =
// slot columns [w S, w S + S).  The slack columns count as +0.0 samples and
// +inf prefix values (selects in wave 0 only), so they add nothing to the
// sums and never start a window.
//   A. the segment's S samples and the next segment's first E (the last
//      segment: the row's first E) into registers; the segment's fp64 sum to
//      the exchange area (kSnrSegExch floats at the end of the level buffer);
//   B. the segment's offset (the sums of the segments before it, in order),
//      the row total, the segment's fp64 running sum cast per column
//      (circular_prefix_sum, kernels.hpp:62-80), and the next segment's first
//      E prefix values the same way from offset + this segment's sum -- the
//      very additions the next wave makes -- (the last segment: the wrap
//      c[p + e] = c[e] + sum, kernels.hpp:88-97, c[e] from the row's first
//      samples from +0.0, as wave 0 does);
//   C. every width's window maximum over the segment's starts, to a maxima
//      area below the exchange area (the rows' samples are all in registers
//      by then: the phase-A barrier);
//   D. width iw on wave iw (mod 8): the 8 segment maxima, the S/N formula,
//      one store per row.
// Each lane works on its own row throughout: no shuffles or scans, and no
// prefix values exchanged (2 workgroup barriers).
template <int SMAX>
__device__ __forceinline__ void snr_segments(const ConeArgs& a, const UnitView& U, float* slot, const int* wl,
                                             int nrows, int tid, const float* whb)
{
    constexpr int S = kSnrSegCols;
    constexpr int E = kSnrSegWmax;
    constexpr int K = S / 2;
    constexpr int q = kSnrSegStride;
    constexpr int kMax = 8 * E * 64;          // maxima area: [segment][width - 1][lane]
    static_assert(S == 2 * K + 1 && 2 * (K + 5) >= S + E && 8 * S - 24 > 0, "segment shape");
    static_assert(kSnrSegRows <= 64 && kLdsBufFloats - kSnrSegExch - kMax >= 0, "segmented S/N areas");
    // an opaque thread index (as snr_epilogue)
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int wave = uni(tid >> 6);
    const int p = U.p;
    const int nev = (int)min((int64_t)nrows, (int64_t)U.rows_eval - (int64_t)U.s0);
    if (nev <= 0) return;
    const uint32_t nw = a.num_widths;
    const int r0 = 8 * S - p;                 // slack columns in front of the row (0 .. 24)
    // r0 in a VGPR: the slack selects of wave 0 as v_cmp + v_cndmask (uniform
    // masks per column were hoisted into SGPR pairs that spill)
    int r0v = r0;
    asm volatile("" : "+v"(r0v));
    uint32_t wmask = 0;
    for (uint32_t iw = 0; iw < nw; ++iw) wmask |= 1u << uni(wl[iw]);
    double* const exch = reinterpret_cast<double*>(slot + kLdsBufFloats - kSnrSegExch);
    float* const maxa = slot + kLdsBufFloats - kSnrSegExch - kMax;
    float* const snr = a.snr + (uint64_t)U.trial * a.snr_stride + (U.snr_row + (uint64_t)U.s0) * (uint64_t)nw;
    const __amdgpu_buffer_rsrc_t srs = buffer_rsrc(snr, (uint32_t)nev * nw * 4u);
    // one block of <= 64 rows (snr_seg_ok); rows past nev compute the values
    // of row nev - 1 again and do not store
    const int r = lane;
    const bool act = r < nev;
    float* const row = slot + min(r, nev - 1) * q;
    const float* const seg = row + wave * S;
    float c[S], n[E];
    // A: samples (this segment, then the next one's first E) and the sum
#pragma unroll
    for (int g = 0; g < S; ++g) c[g] = lds_ld((lds_cptr)(seg + g));
    {
        const lds_cptr nx = (lds_cptr)(wave < 7 ? seg + S : row + r0);
#pragma unroll
        for (int e = 0; e < E; ++e) n[e] = lds_ld(nx + e);
    }
    if (wave == 0) {
        asm volatile("" : "+v"(r0v));
#pragma unroll
        for (int g = 0; g < 24; ++g) c[g] = g < r0v ? 0.0f : c[g];
    }
    // (the first addition of 0.0 dropped: a -0.0 sum is made +0.0 by the
    // offsets' and the total's +0.0 starts)
    double part = (double)c[0];
#pragma unroll
    for (int g = 1; g < S; ++g) part = part + (double)c[g];
    exch[wave * 64 + lane] = part;
    lds_barrier();
    // B: offset, total, prefix values of this segment and of the next one's
    // first E columns
    double off = 0.0, tot = 0.0;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        const double pv = exch[w * 64 + lane];
        if (w < wave) off = off + pv;
        tot = tot + pv;
    }
    const float sumx = (float)tot;
    double acc = off;
#pragma unroll
    for (int g = 0; g < S; ++g) {
        acc = acc + (double)c[g];
        c[g] = (float)acc;
    }
    {
        // the next wave's offset is ((p_0 + p_1) + ...) + p_wave: off + part,
        // the same additions; the last wave starts the row over from +0.0
        double an = wave < 7 ? off + part : 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            an = an + (double)n[e];
            n[e] = (float)an;
        }
        if (wave == 7) {
#pragma unroll
            for (int e = 0; e < E; ++e) n[e] = __fadd_rn(n[e], sumx);
        }
    }
    // C: the window maxima; prefix values as pairs P[k] = c[2k], c[2k + 1]
    // (wave 0: +inf at the slack starts), c[S + e] = n[e]
    f2v P[K + 5], H[K + 4];
#pragma unroll
    for (int k = 0; k < K; ++k) P[k] = f2v{c[2 * k], c[2 * k + 1]};
    P[K] = f2v{c[2 * K], n[0]};
#pragma unroll
    for (int k = K + 1; k < K + 5; ++k) P[k] = f2v{n[2 * (k - K) - 1], n[2 * (k - K)]};
    if (wave == 0) {
        asm volatile("" : "+v"(r0v));
#pragma unroll
        for (int g = 0; g < 24; ++g) {
            if (g & 1) P[g / 2].y = g < r0v ? INFINITY : P[g / 2].y;
            else P[g / 2].x = g < r0v ? INFINITY : P[g / 2].x;
        }
    }
#pragma unroll
    for (int k = 0; k < K + 4; ++k) H[k] = f2v{P[k].y, P[k + 1].x};
    float m[E + 1];
#pragma unroll
    for (int w = 0; w <= E; ++w) m[w] = -INFINITY;
    constexpr uint32_t kStdMask = (1u << 1) | (1u << 2) | (1u << 3) | (1u << 4) | (1u << 6) | (1u << 9);
    if (wmask == kStdMask) {
        // the standard ladder 1, 2, 3, 4, 6, 9 in one block: six independent
        // max chains for the scheduler to interleave
        m[1] = seg_window_max<K, 1>(P, H);
        m[2] = seg_window_max<K, 2>(P, H);
        m[3] = seg_window_max<K, 3>(P, H);
        m[4] = seg_window_max<K, 4>(P, H);
        m[6] = seg_window_max<K, 6>(P, H);
        m[9] = seg_window_max<K, 9>(P, H);
    } else {
        if (wmask & (1u << 1)) m[1] = seg_window_max<K, 1>(P, H);
        if (wmask & (1u << 2)) m[2] = seg_window_max<K, 2>(P, H);
        if (wmask & (1u << 3)) m[3] = seg_window_max<K, 3>(P, H);
        if (wmask & (1u << 4)) m[4] = seg_window_max<K, 4>(P, H);
        if (wmask & (1u << 5)) m[5] = seg_window_max<K, 5>(P, H);
        if (wmask & (1u << 6)) m[6] = seg_window_max<K, 6>(P, H);
        if (wmask & (1u << 7)) m[7] = seg_window_max<K, 7>(P, H);
        if (wmask & (1u << 8)) m[8] = seg_window_max<K, 8>(P, H);
        if (wmask & (1u << 9)) m[9] = seg_window_max<K, 9>(P, H);
    }
#pragma unroll
    for (int w = 1; w <= E; ++w)
        if (wmask & (1u << w)) maxa[(wave * E + w - 1) * 64 + lane] = m[w];
    lds_barrier();
    // D: width iw on wave iw (mod 8)
    for (int iw = wave; iw < (int)nw; iw += 8) {
        const int w = uni(wl[iw]);
        const lds_cptr mx = (lds_cptr)(maxa + (w - 1) * 64 + lane);
        float dm = lds_ld(mx);
#pragma unroll
        for (int k = 1; k < 8; ++k) dm = fmaxf(dm, lds_ld(mx + E * 64 * k));
        const float hpb = whb[2 * iw], b = whb[2 * iw + 1];
        const float v = (hpb * dm - b * sumx) / U.stdnoise;
        const uint32_t o = act ? ((uint32_t)r * nw + (uint32_t)iw) * 4u : 0x80000000u;
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), srs, (int)o, 0, kSnrCpol);
    }
}

// Phase-bin range [lo, hi] a cone kernel variant runs, and the S/N lane-group
// size G of a row of p bins: the epilogue instantiates only the row shapes its
// variant can meet (smaller kernels; the rest is compiled out).
// The wide variants' slot widths are the register staging's breakpoints
// (merge_rows_per_wave = 45 / slots rows per wave): 11 slots stage 4 rows
// per wave (32-row units at p = 513-704, where 16 slots staged 2), 22 slots
// 2 (16-row units at p = 1025-1408, where 45 slots staged 1).
constexpr int variant_pmin(int smax)
{
    return smax == kPack2 ? 1
                          : (smax <= 5 ? 64 * (smax - 1) + 1
                                       : (smax == 8 ? 321 : (smax == 11 ? 513 : (smax == 16 ? 705 : (smax == 22 ? 1025 : 1409)))));
}
constexpr int variant_pmax(int smax) { return smax == kPack2 ? 32 : 64 * smax; }
constexpr bool variant_has_group(int smax, int G)
{
    return snr_group(variant_pmin(smax)) <= G && G <= snr_group(variant_pmax(smax));
}

// S/N lane-group size of the short-row variant (kPack2, p <= 32).  A/B, same
// box, cone ms per cfg4 trial (profiles/r03zf_ab_cfg4.log): G = 8 0.837 /
// 0.837, G = 4 0.777 / 0.778, G = 2 0.796 / 0.797, S/N identical -- 4.
constexpr int kSnrShortG = 4;

// register chunk of a short row's S/N lane (snr_epilogue's kPack2 case)
__device__ __forceinline__ int snr_short_ch(int p)
{
    const int cs = ((p + kSnrShortG - 1) / kSnrShortG) | 1;
    return cs <= 5 ? 5 : (cs <= 9 ? 9 : kSnrMaxChunk);
}

// Row stride of a short-row final pass's output level: room for the S/N's
// whole-chunk prefix writes and its wrapped prefix extension (snr_rows'
// wfull / ext / natural paths: no per-column dummy selects, no wrap selects
// in the window reads), and = 4 (mod 8), so the 8 rows x 4 chunks of a 32-lane
// LDS group (chunk stride c odd) start on 32 distinct banks (at the odd merge
// stride p | 1 they collided).
__device__ __forceinline__ int snr_short_stride(int p)
{
    const int cs = ((p + kSnrShortG - 1) / kSnrShortG) | 1;
    const int ch = snr_short_ch(p);
    const int q0 = max(p + max(ch, kSnrWin), (kSnrShortG - 1) * cs + ch);
    return q0 + ((4 - q0) & 7);
}

template <int SMAX, bool WIDE = false>
__device__ __forceinline__ void snr_epilogue(const ConeArgs& a, const UnitView& U, float* data, int q, const int* wl,
                                             int nrows, int tid, float* whb, unsigned long long* tl)
{
    // an opaque thread index: nothing lane-derived of the S/N is hoisted out
    // of the kernel's trial loop into registers live across the merge
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = tid >> 6;
    const int p = U.p;
    const int nev = (int)min((int64_t)nrows, (int64_t)U.rows_eval - (int64_t)U.s0);
    if (nev <= 0) return;
    // G lanes per row: the smallest power of two >= 8 whose chunks fit
    // kSnrMaxChunk columns; chunk lengths odd (the G chunks of a row start
    // on distinct banks)
    int G = 8;
    while (G < 64 && (((p + G - 1) / G) | 1) > kSnrMaxChunk) G <<= 1;
    int c = (p + G - 1) / G;
    if (c < kSnrMaxChunk) c |= 1;
    const uint32_t nw = a.num_widths;
    float* snr = a.snr + (uint64_t)U.trial * a.snr_stride + (U.snr_row + (uint64_t)U.s0) * (uint64_t)nw;
    if constexpr (SMAX == kPack2) {
        // short rows (p <= 32): kSnrShortG lanes per row, so a pass covers
        // 512 / G rows (cfg4's ~380-row final units: 3 passes at G = 4
        // instead of 6 at G = 8)
        constexpr int GS = kSnrShortG;
        const int cs = ((p + GS - 1) / GS) | 1;
        if (cs <= 5) snr_rows<5, GS>(a, U, data, q, wl, nev, cs, tid, whb, tl);
        else if (cs <= 9) snr_rows<9, GS>(a, U, data, q, wl, nev, cs, tid, whb, tl);
        else snr_rows<kSnrMaxChunk, GS>(a, U, data, q, wl, nev, cs, tid, whb, tl);
        return;
    }
    if (c <= kSnrMaxChunk) {
        // short rows (p <= 40 / 72): register chunks sized to the row, not 17
        if constexpr (variant_has_group(SMAX, 8)) {
            if (G == 8) {
                if (c <= 5) snr_rows<5, 8>(a, U, data, q, wl, nev, c, tid, whb, tl);
                else if (c <= 9) snr_rows<9, 8>(a, U, data, q, wl, nev, c, tid, whb, tl);
                else snr_rows<kSnrMaxChunk, 8>(a, U, data, q, wl, nev, c, tid, whb, tl);
                return;
            }
        }
        if constexpr (variant_has_group(SMAX, 16)) {
            if (G == 16) {
                if constexpr (WIDE) {
                    if (snr_wide_ok(p, q, wl[kMaxWidths])) {
                        snr_rows<kSnrMaxChunk, 16, true>(a, U, data, q, wl, nev, c, tid, whb, tl);
                        return;
                    }
                }
                snr_rows<kSnrMaxChunk, 16>(a, U, data, q, wl, nev, c, tid, whb, tl);
                return;
            }
        }
        if constexpr (variant_has_group(SMAX, 32)) {
            if (G == 32) {
                snr_rows<kSnrMaxChunk, 32>(a, U, data, q, wl, nev, c, tid, whb, tl);
                return;
            }
        }
        if constexpr (variant_has_group(SMAX, 64)) snr_rows<kSnrMaxChunk, 64>(a, U, data, q, wl, nev, c, tid, whb, tl);
    } else if (c <= kSnrChunk) {
        if constexpr (variant_has_group(SMAX, 64)) snr_rows<kSnrChunk, 64>(a, U, data, q, wl, nev, c, tid, whb, tl);
    } else if constexpr (variant_pmax(SMAX) > 64 * kSnrChunk) {
        // very wide rows (p > 64 * kSnrChunk): one wave per row, chunks from LDS
        const int g = lane;
        const int j0 = min(g * c, p);
        const int cnt = min(j0 + c, p) - j0;
        const int owner = (p - 1) / c;
        for (int base = 0; base < nev; base += kConeWaves) {
            const int r = base + wave;
            const bool active = r < nev;
            float* row = data + min(r, nev - 1) * q;
            double part = 0.0;
            for (int j = j0; j < j0 + cnt; ++j) part += (double)row[j];
            double incl = part;
            for (int d = 1; d < 64; d <<= 1) {
                const double y = __shfl_up(incl, d, 64);
                if (g >= d) incl += y;
            }
            double acc = __shfl_up(incl, 1, 64);
            if (g == 0) acc = 0.0;
            lds_barrier();
            if (active)
                for (int j = j0; j < j0 + cnt; ++j) {
                    acc += (double)row[j];
                    row[j] = (float)acc;
                }
            const float sum = __shfl((float)acc, owner, 64);
            lds_barrier();
            for (uint32_t iw = 0; iw < nw; ++iw) {
                const int w = uni(wl[iw]);
                float dmax = -INFINITY;
                for (int i = j0; i < j0 + cnt; ++i) {
                    const int k = i + w;
                    const float ck = k < p ? row[k] : __fadd_rn(row[k - p], sum);
                    dmax = fmaxf(dmax, __fsub_rn(ck, row[i]));
                }
                for (int o = 32; o > 0; o >>= 1) dmax = fmaxf(dmax, __shfl_xor(dmax, o, 64));
                if (active && g == 0) {
                    const float h = sqrtf((float)(p - w) / (float)(p * w));
                    const float b = (float)w / (float)(p - w) * h;
                    snr[(uint64_t)r * nw + iw] = ((h + b) * dmax - b * sum) / U.stdnoise;
                }
            }
            lds_barrier();
        }
    }
}

}  // namespace rt
