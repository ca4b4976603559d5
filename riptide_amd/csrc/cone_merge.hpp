// Fragment of the cone translation unit (ffa_kernels.hip), device code only:
// the merge steps of a unit's levels in LDS (dense rows, row slots, short rows
// as lanes and as tasks) with their write-back and store helpers and roll
// tables, and merge_levels, which runs them deepest level first.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "cone_unit.hpp"

namespace rt {

template <int N> struct IntC { static constexpr int value = N; };

typedef const __attribute__((address_space(3))) float* lds_cptr;

// LDS reads the compiler must not pair into ds_read2_b32 / ds_read2st64_b32
// (those issue at a lower rate than separate ds_read_b32 on gfx950,
// tools/microbench/lds_b64.hip): volatile accesses are never merged.
__device__ __forceinline__ float lds_ld(lds_cptr p) { return *(const volatile __attribute__((address_space(3))) float*)p; }

// Outputs of level l (rows wave + 8i) into v, from the level below in dense
// rows of stride p at `src`:
//   out[j] = H[j] + T[(j + s) mod p]
// Bins j = lane + 64k: one ds_read_b32 of H and one of T per slot, T[j + s]
// before the wrap point p - s and T[j + s - p] from it on (two opaque
// per-row bases and a compare/select per slot; the slot offset 256k an
// immediate).  Per row the descriptor is one v_readlane of the packed word
// (unpacked in SALU).  The additions are the reference's, element by
// element.  CARRIED: the level may hold size-1 nodes (whole units near their
// leaves), whose rows add -0.0 to H (x + (-0.0) == x exactly, as the
// reference's copy).  Branch-free over rows and slots: rows i >= nr and bins
// past p read in-bounds garbage that is never written back.
template <int SMAX, int RW, bool CARRIED>
__device__ __forceinline__ void merge_level_dense(const UnitCtx& C, const float* src, int p, int l, int lane,
                                                  int wave, int nr, float (&v)[RW][SMAX], const int* loff)
{
    const int S = (p + 63) >> 6;
    // lane i unpacks the descriptor of the wave's i-th row into LDS float
    // offsets (head row, tail row + shift) and the shift; the row loop takes
    // them with v_readlane, so no per-row scalar unpacking or multiplies
    int ho = 0, to = 0, sh = 0, car = 0;
    if (lane < nr) {
        const uint32_t d = unit_desc(C, l, wave + kConeWaves * lane, p);
        const uint32_t tc = (d >> 10) & 1023u;
        sh = (int)(d >> 20);
        // source rows: dense (stride p), or the bottom level's fill layout
        ho = loff ? loff[d & 1023u] : (int)(d & 1023u) * p;
        to = (tc == kCarried ? ho : (loff ? loff[tc] : (int)tc * p)) + sh;
        car = tc == kCarried;
    }
    const lds_cptr l1 = (lds_cptr)src + lane;
#pragma unroll
    for (int i = 0; i < RW; ++i) {
        const int hoi = __builtin_amdgcn_readlane(ho, i);
        const int toi = __builtin_amdgcn_readlane(to, i);
        const int si = __builtin_amdgcn_readlane(sh, i);
        uint32_t keep = 0xFFFFFFFFu, neg0 = 0u;
        if (CARRIED) {
            keep = __builtin_amdgcn_readlane(car, i) ? 0u : 0xFFFFFFFFu;
            neg0 = ~keep & 0x80000000u;
        }
        const lds_cptr hrow = l1 + hoi;
        lds_cptr ta = l1 + toi;
        lds_cptr tw = ta - p;
        asm("" : "+v"(ta), "+v"(tw));
        const int ls = lane + si;               // bin j = lane + 64k wraps when ls >= p - 64k
#pragma unroll
        for (int k = 0; k < SMAX; ++k) {
            if (SMAX <= 5 || k < S) {
                const lds_cptr tp = ls >= p - 64 * k ? tw : ta;
                float x = lds_ld(tp + 64 * k);
                if (CARRIED) x = __uint_as_float((__float_as_uint(x) & keep) | neg0);
                v[i][k] = __fadd_rn(hrow[64 * k], x);
            }
        }
    }
}

// Two merge levels in one LDS round trip: the outputs of level l from the
// rows of level l + 2 (the level l + 1 in between is never stored).  Output
// row r of level l is H[h] + roll(T[t], sh) with H, T rows of level l + 1,
// and H[h] = HH[hh] + roll(HT[ht], sH), T[t] = TH[th] + roll(TT[tt], sT) from
// level l + 2, so bin j is
//     (HH[hh][j] + HT[ht][(j + sH) mod p])
//   + (TH[th][(j + sh) mod p] + TT[tt][(j + sh + sT) mod p])
// -- the reference's float additions on the same operands in the same
// association (transforms.hpp:13-27 applied twice), so bit-exact.  Per
// 64-bin slot: 4 ds_read_b32 + 1 ds_write_b32 per two levels instead of 4 + 2.
// Only levels whose nodes all have >= 2 rows (no carried size-1 nodes at
// level l + 1) are fused.
template <int SMAX, int RW>
__device__ __forceinline__ void merge_level2_dense(const UnitCtx& C, const float* src, int p, int l, int lane,
                                                   int wave, int nr, float (&v)[RW][SMAX], const int* loff)
{
    const int S = (p + 63) >> 6;
    int o0 = 0, o1 = 0, o2 = 0, o3 = 0, s1 = 0, s2 = 0, s3 = 0;
    if (lane < nr) {
        const uint32_t d0 = unit_desc(C, l, wave + kConeWaves * lane, p);
        const uint32_t dh = unit_desc(C, l + 1, (int)(d0 & 1023u), p);
        const uint32_t dt = unit_desc(C, l + 1, (int)((d0 >> 10) & 1023u), p);
        const int sh = (int)(d0 >> 20), sH = (int)(dh >> 20), sT = (int)(dt >> 20);
        int sTT = sh + sT;
        sTT = sTT >= p ? sTT - p : sTT;
        // source rows: dense (stride p), or the bottom level's fill layout
        const uint32_t r0 = dh & 1023u, r1 = (dh >> 10) & 1023u, r2 = dt & 1023u, r3 = (dt >> 10) & 1023u;
        o0 = (loff ? loff[r0] : (int)r0 * p);
        o1 = (loff ? loff[r1] : (int)r1 * p) + sH;
        o2 = (loff ? loff[r2] : (int)r2 * p) + sh;
        o3 = (loff ? loff[r3] : (int)r3 * p) + sTT;
        s1 = sH;
        s2 = sh;
        s3 = sTT;
    }
    const lds_cptr l1 = (lds_cptr)src + lane;
#pragma unroll
    for (int i = 0; i < RW; ++i) {
        const lds_cptr hrow = l1 + __builtin_amdgcn_readlane(o0, i);
        lds_cptr b1 = l1 + __builtin_amdgcn_readlane(o1, i);
        lds_cptr b2 = l1 + __builtin_amdgcn_readlane(o2, i);
        lds_cptr b3 = l1 + __builtin_amdgcn_readlane(o3, i);
        lds_cptr w1 = b1 - p, w2 = b2 - p, w3 = b3 - p;
        asm("" : "+v"(b1), "+v"(w1), "+v"(b2), "+v"(w2), "+v"(b3), "+v"(w3));
        const int ls1 = lane + __builtin_amdgcn_readlane(s1, i);
        const int ls2 = lane + __builtin_amdgcn_readlane(s2, i);
        const int ls3 = lane + __builtin_amdgcn_readlane(s3, i);
#pragma unroll
        for (int k = 0; k < SMAX; ++k) {
            if (SMAX <= 5 || k < S) {
                const int wk = p - 64 * k;
                const float x1 = lds_ld((ls1 >= wk ? w1 : b1) + 64 * k);
                const float x2 = lds_ld((ls2 >= wk ? w2 : b2) + 64 * k);
                const float x3 = lds_ld((ls3 >= wk ? w3 : b3) + 64 * k);
                v[i][k] = __fadd_rn(__fadd_rn(hrow[64 * k], x1), __fadd_rn(x2, x3));
            }
        }
    }
}

// Output level l == 0 of a non-final pass: straight from the staging
// registers to global memory at byte offset st_o0 (the tile's rows are one
// contiguous segment).
template <int SMAX, int RW>
__device__ __forceinline__ void store_rows(const float (&v)[RW][SMAX], int p, int lane, int wave, int nr,
                                           __amdgpu_buffer_rsrc_t rs, uint32_t st_o0)
{
    const int S = (p + 63) >> 6;
    const bool tail_ok = lane + 64 * (SMAX - 1) < p;
#pragma unroll
    for (int i = 0; i < RW; ++i) {
        if (i < nr) {
            const uint32_t ob = st_o0 + (uint32_t)((wave + kConeWaves * i) * p + lane) * 4u;
#pragma unroll
            for (int k = 0; k < SMAX; ++k) {
                if constexpr (SMAX <= 5) {
                    // rows of exactly SMAX slots: the last slot's lanes past p
                    // store out of the buffer's range, which drops them
                    const uint32_t o = k < SMAX - 1 ? ob + 256u * (uint32_t)k
                                                    : (tail_ok ? ob + 256u * (uint32_t)k : 0x80000000u);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[i][k]), rs, (int)o, 0, kStoreCpol);
                } else if (64 * (k + 1) <= p || (k < S && lane + 64 * k < p)) {
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[i][k]), rs,
                                                          (int)(ob + 256u * (uint32_t)k), 0, kStoreCpol);
                }
            }
        }
    }
}

// Write-back of a level's staged rows into the dense LDS rows at `base`.
// SMAX <= 5 kernels run rows of exactly SMAX slots: all but the last are
// full; the last slot's lanes past p write to a dummy word in the LDS pad
// (an address select instead of an exec-mask save/restore per row).
template <int SMAX, int RW>
__device__ __forceinline__ void write_rows(float* base, float* dummy, const float (&v)[RW][SMAX], int p, int lane,
                                           int wave, int nr)
{
    const int S = (p + 63) >> 6;
    const bool tail_ok = lane + 64 * (SMAX - 1) < p;
#pragma unroll
    for (int i = 0; i < RW; ++i) {
        if (i < nr) {
            float* orow = base + (wave + kConeWaves * i) * p + lane;
#pragma unroll
            for (int k = 0; k < SMAX; ++k) {
                if constexpr (SMAX <= 5) {
                    if (k < SMAX - 1) orow[64 * k] = v[i][k];
                    else *(tail_ok ? orow + 64 * k : dummy) = v[i][k];
                } else {
                    if (64 * (k + 1) <= p || (k < S && lane + 64 * k < p)) orow[64 * k] = v[i][k];
                }
            }
        }
    }
}

// Row-slot merge steps (units with a blob, SMAX <= 5 rows of exactly SMAX
// slots; common.hpp kSlotPair).  A wave's slot q fills register rows 2q and
// 2q + 1: one output row, two independent rows, or a row pair r, r + 1 with
// the same head and tail rows and roll shifts s, s + 1.  The pair's second
// row reuses the first's terms: with H = the head term and T the rolled tail
// term of row r (fused: H = HH + roll(HT, sH), T = roll(TH, s) +
// roll(TT, s + sT)), row r + 1 is H[j] + T[(j + 1) mod p] -- the same float
// operands in the same association as computing it directly, so bit-exact --
// taken with one DPP lane shift (wave_shl:1) per 64-bin slot, the slot's
// lane 63 from lane 0 of the next slot, and bin p - 1 from bin 0.  Half the
// LDS reads of the pair.
//
// Per-row terms from the row's scalars (SGPRs): r0 head row offset, r1..r3
// the rolled rows' offsets (+ their rolls), t1..t3 the rolls, c1 carried.
// HEAD false (row B of a kSlotHalf): only the tail term; hs is row A's.
template <int SMAX, bool TWO, bool HEAD = true>
__device__ __forceinline__ void row_terms_s(lds_cptr l1, int p, int lane, int r0, int r1, int r2, int r3, int t1,
                                            int t2, int t3, int c1, float (&hs)[SMAX], float (&ts)[SMAX])
{
    if constexpr (TWO && !HEAD) {
        lds_cptr b2 = l1 + r2;
        lds_cptr b3 = l1 + r3;
        lds_cptr w2 = b2 - p, w3 = b3 - p;
        asm("" : "+v"(b2), "+v"(w2), "+v"(b3), "+v"(w3));
        const int ls2 = lane + t2;
        const int ls3 = lane + t3;
#pragma unroll
        for (int k = 0; k < SMAX; ++k) {
            const int wk = p - 64 * k;
            const float x2 = lds_ld((ls2 >= wk ? w2 : b2) + 64 * k);
            const float x3 = lds_ld((ls3 >= wk ? w3 : b3) + 64 * k);
            ts[k] = __fadd_rn(x2, x3);
        }
    } else if constexpr (TWO) {
        const lds_cptr hrow = l1 + r0;
        lds_cptr b1 = l1 + r1;
        lds_cptr b2 = l1 + r2;
        lds_cptr b3 = l1 + r3;
        lds_cptr w1 = b1 - p, w2 = b2 - p, w3 = b3 - p;
        asm("" : "+v"(b1), "+v"(w1), "+v"(b2), "+v"(w2), "+v"(b3), "+v"(w3));
        const int ls1 = lane + t1;
        const int ls2 = lane + t2;
        const int ls3 = lane + t3;
#pragma unroll
        for (int k = 0; k < SMAX; ++k) {
            const int wk = p - 64 * k;
            const float x1 = lds_ld((ls1 >= wk ? w1 : b1) + 64 * k);
            const float x2 = lds_ld((ls2 >= wk ? w2 : b2) + 64 * k);
            const float x3 = lds_ld((ls3 >= wk ? w3 : b3) + 64 * k);
            hs[k] = __fadd_rn(lds_ld(hrow + 64 * k), x1);
            ts[k] = __fadd_rn(x2, x3);
        }
    } else if constexpr (!HEAD) {
        // single step, row B of a half: its tail only (never carried)
        lds_cptr ta = l1 + r1;
        lds_cptr tw = ta - p;
        asm("" : "+v"(ta), "+v"(tw));
        const int ls = lane + t1;
#pragma unroll
        for (int k = 0; k < SMAX; ++k) ts[k] = lds_ld((ls >= p - 64 * k ? tw : ta) + 64 * k);
    } else {
        // r0 head row, r1 tail row + shift, t1 shift, c1 carried (size-1 node:
        // the tail term is -0.0, x + (-0.0) == x exactly)
        const lds_cptr hrow = l1 + r0;
        lds_cptr ta = l1 + r1;
        lds_cptr tw = ta - p;
        asm("" : "+v"(ta), "+v"(tw));
        const int ls = lane + t1;
        const uint32_t keep = c1 ? 0u : 0xFFFFFFFFu;
        const uint32_t neg0 = ~keep & 0x80000000u;
#pragma unroll
        for (int k = 0; k < SMAX; ++k) {
            const float x = lds_ld((ls >= p - 64 * k ? tw : ta) + 64 * k);
            hs[k] = lds_ld(hrow + 64 * k);
            ts[k] = __uint_as_float((__float_as_uint(x) & keep) | neg0);
        }
    }
}

// Roll table (4-slot rows, p = 193..256): a rolled read of a
// row at roll t takes bin j = lane + 64k from T[(lane + t + 64k) mod p].
// Entry x = lane + t (x < p + 64) of a per-unit LDS table holds the four
// byte offsets 4 ((x + 64k) mod p), k = 0..3, as 16-bit halves of 8 bytes:
// one conflict-free ds_read_b64 per rolled row (consecutive lanes,
// consecutive entries), then one address add per slot from the row's start
// (an SGPR) -- instead of a compare and a select per slot against the wrap
// point.  Same LDS words, same additions: bit-exact.  The table sits at the
// end of the unit's metadata area (kLut4Off, past every blob's LDS part:
// validate_exec_plan) and is rebuilt by every unit of a 4-slot instance.
typedef const __attribute__((address_space(3))) unsigned long long* lut_cptr;
typedef const __attribute__((address_space(3))) char* lds_ccptr;

// rolled row whose roll-table entry is e and whose row starts at byte `rb`
// of LDS (uniform)
__device__ __forceinline__ void rolled_lut4(lds_ccptr rb, unsigned long long e, float (&x)[4])
{
    const uint32_t e0 = (uint32_t)e, e1 = (uint32_t)(e >> 32);
    x[0] = lds_ld((lds_cptr)(rb + (e0 & 0xFFFFu)));
    x[1] = lds_ld((lds_cptr)(rb + (e0 >> 16)));
    x[2] = lds_ld((lds_cptr)(rb + (e1 & 0xFFFFu)));
    x[3] = lds_ld((lds_cptr)(rb + (e1 >> 16)));
}

// row_terms_s with the roll table: s0 the level's rows (uniform), r0 the head
// row's offset, q1..q3 the rolled rows' offsets WITHOUT their rolls t1..t3.
// The table entries are read first (plain loads, free to move) and the head
// row before the rolled rows (the volatile reads keep their order), so the
// head reads are in flight while the entries return.
template <bool TWO, bool HEAD = true>
__device__ __forceinline__ void row_terms_lut(lds_cptr l1, lds_cptr s0, lut_cptr lutl, int r0, int q1, int q2, int q3,
                                              int t1, int t2, int t3, int c1, float (&hs)[4], float (&ts)[4])
{
    const lds_ccptr b = (lds_ccptr)s0;
    if constexpr (TWO) {
        const unsigned long long e1 = HEAD ? lutl[t1] : 0ull;
        const unsigned long long e2 = lutl[t2], e3 = lutl[t3];
        float h[4], x1[4], x2[4], x3[4];
        if constexpr (HEAD) {
#pragma unroll
            for (int k = 0; k < 4; ++k) h[k] = lds_ld(l1 + r0 + 64 * k);
            rolled_lut4(b + 4 * q1, e1, x1);
        }
        rolled_lut4(b + 4 * q2, e2, x2);
        rolled_lut4(b + 4 * q3, e3, x3);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (HEAD) hs[k] = __fadd_rn(h[k], x1[k]);
            ts[k] = __fadd_rn(x2[k], x3[k]);
        }
    } else {
        const unsigned long long e = lutl[t1];
        float x[4];
        if constexpr (HEAD) {
#pragma unroll
            for (int k = 0; k < 4; ++k) hs[k] = lds_ld(l1 + r0 + 64 * k);
        }
        rolled_lut4(b + 4 * q1, e, x);
        if constexpr (HEAD) {
            // c1: a carried size-1 node (its tail term is -0.0, x + (-0.0) == x)
            const uint32_t keep = c1 ? 0u : 0xFFFFFFFFu;
            const uint32_t neg0 = ~keep & 0x80000000u;
#pragma unroll
            for (int k = 0; k < 4; ++k) ts[k] = __uint_as_float((__float_as_uint(x[k]) & keep) | neg0);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) ts[k] = x[k];
        }
    }
}

// Builds the roll table of rows of p bins (4-slot instances) at `lut`:
// entry x < p + 64 = {4 (x mod p) | 4 ((x + 64) mod p) << 16,
//                     4 ((x + 128) mod p) | 4 ((x + 192) mod p) << 16}.
__device__ __forceinline__ void build_roll_lut4(uint32_t* lut, int p, int tid)
{
    for (int w = tid; w < 2 * (p + 64); w += kConeBlock) {
        const int x = (w >> 1) + 128 * (w & 1);
        int y0 = x, y1 = x + 64;
        // y < p + 256 < 3p (p >= 193): at most two subtractions
        y0 -= y0 >= p ? p : 0;
        y0 -= y0 >= p ? p : 0;
        y1 -= y1 >= p ? p : 0;
        y1 -= y1 >= p ? p : 0;
        lut[w] = (uint32_t)(4 * y0) | ((uint32_t)(4 * y1) << 16);
    }
}

// Per-row terms of the row whose resolved descriptor sits in lane i
// (unpacked per lane: o0 .. o3, s1 .. s3; seven v_readlane per row).
template <int SMAX, bool TWO, bool HEAD = true>
__device__ __forceinline__ void row_terms(lds_cptr l1, int p, int lane, int i, int o0, int o1, int o2, int o3, int s1,
                                          int s2, int s3, float (&hs)[SMAX], float (&ts)[SMAX],
                                          lds_cptr s0 = nullptr, lut_cptr lutl = nullptr)
{
    if constexpr (SMAX == 4) {
        // o1 .. o3 are the rolled rows' offsets without their rolls here
        if constexpr (TWO) {
            if constexpr (HEAD) {
                int r0 = __builtin_amdgcn_readlane(o0, i), q1 = __builtin_amdgcn_readlane(o1, i);
                int q2 = __builtin_amdgcn_readlane(o2, i), q3 = __builtin_amdgcn_readlane(o3, i);
                int t1 = __builtin_amdgcn_readlane(s1, i), t2 = __builtin_amdgcn_readlane(s2, i);
                int t3 = __builtin_amdgcn_readlane(s3, i);
                asm volatile("" : "+s"(r0), "+s"(q1), "+s"(q2), "+s"(q3), "+s"(t1), "+s"(t2), "+s"(t3));
                row_terms_lut<true>(l1, s0, lutl, r0, q1, q2, q3, t1, t2, t3, 0, hs, ts);
            } else {
                int q2 = __builtin_amdgcn_readlane(o2, i), q3 = __builtin_amdgcn_readlane(o3, i);
                int t2 = __builtin_amdgcn_readlane(s2, i), t3 = __builtin_amdgcn_readlane(s3, i);
                asm volatile("" : "+s"(q2), "+s"(q3), "+s"(t2), "+s"(t3));
                row_terms_lut<true, false>(l1, s0, lutl, 0, 0, q2, q3, 0, t2, t3, 0, hs, ts);
            }
        } else {
            if constexpr (HEAD) {
                int r0 = __builtin_amdgcn_readlane(o0, i), q1 = __builtin_amdgcn_readlane(o1, i);
                int t1 = __builtin_amdgcn_readlane(s1, i), c1 = __builtin_amdgcn_readlane(o2, i);
                asm volatile("" : "+s"(r0), "+s"(q1), "+s"(t1), "+s"(c1));
                row_terms_lut<false>(l1, s0, lutl, r0, q1, 0, 0, t1, 0, 0, c1, hs, ts);
            } else {
                int q1 = __builtin_amdgcn_readlane(o1, i), t1 = __builtin_amdgcn_readlane(s1, i);
                asm volatile("" : "+s"(q1), "+s"(t1));
                row_terms_lut<false, false>(l1, s0, lutl, 0, q1, 0, 0, t1, 0, 0, 0, hs, ts);
            }
        }
        return;
    }
    // all of the row's scalars first, in distinct SGPRs: a v_readlane result
    // read by the next VALU instruction costs s_nop wait states
    if constexpr (TWO) {
        if constexpr (HEAD) {
            int r0 = __builtin_amdgcn_readlane(o0, i), r1 = __builtin_amdgcn_readlane(o1, i);
            int r2 = __builtin_amdgcn_readlane(o2, i), r3 = __builtin_amdgcn_readlane(o3, i);
            int t1 = __builtin_amdgcn_readlane(s1, i), t2 = __builtin_amdgcn_readlane(s2, i);
            int t3 = __builtin_amdgcn_readlane(s3, i);
            asm volatile("" : "+s"(r0), "+s"(r1), "+s"(r2), "+s"(r3), "+s"(t1), "+s"(t2), "+s"(t3));
            row_terms_s<SMAX, true>(l1, p, lane, r0, r1, r2, r3, t1, t2, t3, 0, hs, ts);
        } else {
            int r2 = __builtin_amdgcn_readlane(o2, i), r3 = __builtin_amdgcn_readlane(o3, i);
            int t2 = __builtin_amdgcn_readlane(s2, i), t3 = __builtin_amdgcn_readlane(s3, i);
            asm volatile("" : "+s"(r2), "+s"(r3), "+s"(t2), "+s"(t3));
            row_terms_s<SMAX, true, false>(l1, p, lane, 0, 0, r2, r3, 0, t2, t3, 0, hs, ts);
        }
    } else {
        if constexpr (HEAD) {
            int r0 = __builtin_amdgcn_readlane(o0, i), r1 = __builtin_amdgcn_readlane(o1, i);
            int t1 = __builtin_amdgcn_readlane(s1, i), c1 = __builtin_amdgcn_readlane(o2, i);
            asm volatile("" : "+s"(r0), "+s"(r1), "+s"(t1), "+s"(c1));
            row_terms_s<SMAX, false>(l1, p, lane, r0, r1, 0, 0, t1, 0, 0, c1, hs, ts);
        } else {
            int r1 = __builtin_amdgcn_readlane(o1, i), t1 = __builtin_amdgcn_readlane(s1, i);
            asm volatile("" : "+s"(r1), "+s"(t1));
            row_terms_s<SMAX, false, false>(l1, p, lane, 0, r1, 0, 0, t1, 0, 0, 0, hs, ts);
        }
    }
}

template <int SMAX, int RW, bool TWO>
__device__ __forceinline__ void merge_step_slots(const UnitCtx& C, const float* src, int p, int lo, int lane,
                                                 int wave, float (&v)[RW][SMAX], const int* loff, uint32_t& sw,
                                                 int& nq)
{
    constexpr int Q = (RW + 1) / 2;
    static_assert(Q <= 32, "row slots: one lane per slot row");
    const uint32_t* st = slot_table(C, lo);
    const int ns = uni((int)st[0]);
    nq = uni(ns > wave ? (ns - wave + kConeWaves - 1) / kConeWaves : 0);
    // lane i < 32 resolves row A of the wave's slot i, lane 32 + i its row B
    const int qi = lane & 31;
    int o0 = 0, o1 = 0, o2 = 0, o3 = 0, s1 = 0, s2 = 0, s3 = 0;
    if constexpr (resolved_slots(SMAX)) {
        // host-resolved rows: one 16-byte entry per lane (the slot's row A in
        // lanes 0-31 with the slot word, row B in lanes 32-63)
        // wave-major halves (build_tile_blob): the 32 lanes of a half read
        // consecutive 16-byte entries; lanes past Q re-read entry Q - 1
        const int qc = qi < Q ? qi : Q - 1;
        const uint4 e = reinterpret_cast<const uint4*>(st)[1 + (lane >> 5) * (kConeWaves * Q) + wave * Q + qc];
        sw = lane < 32 ? e.w : 0u;
        s1 = (int)(e.z & 1023u);
        // the roll table path takes the rolled rows' offsets without rolls
        constexpr int roll_in = SMAX == 4 ? 0 : 1;
        if constexpr (TWO) {
            s2 = (int)((e.z >> 10) & 1023u);
            s3 = (int)((e.z >> 20) & 1023u);
            o0 = (int)(e.x & 0xFFFFu);
            o1 = (int)(e.x >> 16) + roll_in * s1;
            o2 = (int)(e.y & 0xFFFFu) + roll_in * s2;
            o3 = (int)(e.y >> 16) + roll_in * s3;
        } else {
            o0 = (int)(e.x & 0xFFFFu);
            o1 = (int)(e.x >> 16) + roll_in * s1;
            o2 = (int)((e.z >> 30) & 1u);
        }
        (void)loff;
    } else {
    sw = qi < nq ? st[1 + wave + kConeWaves * qi] : 0u;
    const bool act = qi < nq && (lane < 32 || (sw >> 20) == kSlotTwo || (sw >> 20) == kSlotHalf);
    const int r = lane < 32 ? (int)(sw & 1023u) : (int)((sw >> 10) & 1023u);
    const uint32_t* const desc = desc_table(C);
    // the first step reads the bottom level through its row offsets
    const bool use_loff = loff != nullptr;
    if (act) {
        if constexpr (TWO) {
            const uint32_t d0 = desc[desc_offset(C, lo) + r];
            const uint32_t dh = desc[desc_offset(C, lo + 1) + (int)(d0 & 1023u)];
            const uint32_t dt = desc[desc_offset(C, lo + 1) + (int)((d0 >> 10) & 1023u)];
            const int sh = (int)(d0 >> 20), sH = (int)(dh >> 20), sT = (int)(dt >> 20);
            int sTT = sh + sT;
            sTT = sTT >= p ? sTT - p : sTT;
            const uint32_t r0 = dh & 1023u, r1 = (dh >> 10) & 1023u, r2 = dt & 1023u, r3 = (dt >> 10) & 1023u;
            o0 = (use_loff ? loff[r0] : (int)__umul24(r0, (uint32_t)p));
            o1 = (use_loff ? loff[r1] : (int)__umul24(r1, (uint32_t)p)) + sH;
            o2 = (use_loff ? loff[r2] : (int)__umul24(r2, (uint32_t)p)) + sh;
            o3 = (use_loff ? loff[r3] : (int)__umul24(r3, (uint32_t)p)) + sTT;
            s1 = sH;
            s2 = sh;
            s3 = sTT;
        } else {
            const uint32_t d = desc[desc_offset(C, lo) + r];
            const uint32_t tc = (d >> 10) & 1023u;
            s1 = (int)(d >> 20);
            o0 = use_loff ? loff[d & 1023u] : (int)__umul24(d & 1023u, (uint32_t)p);
            o1 = (tc == kCarried ? o0 : (use_loff ? loff[tc] : (int)__umul24(tc, (uint32_t)p))) + s1;
            o2 = tc == kCarried;
        }
    }
    }
    const lds_cptr l1 = (lds_cptr)src + lane;
    const lds_cptr s0 = (lds_cptr)src;
    const lut_cptr lutl = (lut_cptr)(C.aux0 + kLut4Off) + lane;
    const int jl = p - 1 - 64 * (SMAX - 1);   // lane of bin p - 1 in the last slot
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if (q < nq) {
            const uint32_t kq = (uint32_t)__builtin_amdgcn_readlane((int)sw, q) >> 20;
            float hs[SMAX], ts[SMAX];
            row_terms<SMAX, TWO>(l1, p, lane, q, o0, o1, o2, o3, s1, s2, s3, hs, ts, s0, lutl);
#pragma unroll
            for (int k = 0; k < SMAX; ++k) v[2 * q][k] = __fadd_rn(hs[k], ts[k]);
            const int qb = 2 * q + 1 < RW ? 2 * q + 1 : RW - 1;   // row B's register row (q < Q: in range)
            if (2 * q + 1 < RW) {
                if (kq == kSlotPair) {
                    // bin j + 1 of the rolled tail term: slot k's lanes 0-62
                    // from lanes 1-63 (wave_shl:1, bound_ctrl off: lane 63 has
                    // no source and keeps the old value), lane 63 from lane 0
                    // of slot k + 1 (the old value: wave_rol:1 of slot k + 1);
                    // the last slot's bin p - 1 (lane jl) takes bin 0 (lane 0
                    // of slot 0) by v_writelane -- two or three VALU per slot
                    // instead of a v_readlane, a move and a select each
                    const int w0 = __builtin_amdgcn_readlane(__float_as_int(ts[0]), 0);
#pragma unroll
                    for (int k = 0; k < SMAX; ++k) {
                        int x;
                        if (k + 1 < SMAX) {
                            const int nx = __builtin_amdgcn_mov_dpp(__float_as_int(ts[k + 1]), 0x134, 0xF, 0xF, false);
                            x = __builtin_amdgcn_update_dpp(nx, __float_as_int(ts[k]), 0x130, 0xF, 0xF, false);
                        } else {
                            x = __builtin_amdgcn_mov_dpp(__float_as_int(ts[k]), 0x130, 0xF, 0xF, true);
                            // lane select in M0 (gfx9: one SGPR operand per VALU instruction)
                            asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(x) : "s"(w0), "s"(jl)
                                         : "m0");
                        }
                        v[qb][k] = __fadd_rn(hs[k], __int_as_float(x));
                    }
                } else if (kq == kSlotHalf) {
                    // row B shares row A's head term: only its tail term
                    float tb[SMAX];
                    row_terms<SMAX, TWO, false>(l1, p, lane, 32 + q, o0, o1, o2, o3, s1, s2, s3, hs, tb, s0, lutl);
#pragma unroll
                    for (int k = 0; k < SMAX; ++k) v[qb][k] = __fadd_rn(hs[k], tb[k]);
                } else if (kq == kSlotTwo) {
                    row_terms<SMAX, TWO>(l1, p, lane, 32 + q, o0, o1, o2, o3, s1, s2, s3, hs, ts, s0, lutl);
#pragma unroll
                    for (int k = 0; k < SMAX; ++k) v[qb][k] = __fadd_rn(hs[k], ts[k]);
                }
            }
        }
    }
}

// Slot-step write-back into the dense LDS rows at base / store to global
// memory (a non-final pass's output level): register rows 2q, 2q + 1 to the
// slot's rows A and B (row stride q: p, or a final pass's S/N stride).
// A row's full 64-bin slots (all but the last) by ds_write_addtid_b32: the
// address is M0 + offset + 4 lane (no address VGPR), 2 LDS cycles per wave
// instruction instead of ds_write_b32's 4.  M0 holds 16 bits: rows past
// 64 KiB - 1 KiB take M0 = a - 32 KiB and offsets from 32 KiB.  Same-box
// A/B, cone ms per trial (profiles/r05q_ab_*.log): cfg2 6.56-6.58 vs
// 6.59-6.62, cfg3 1.658-1.693 vs 1.670-1.697 with ds_write_b32 for every
// slot.
template <int SMAX>
__device__ __forceinline__ void write_row_addtid(uint32_t a, const float (&x)[SMAX])
{
    static_assert(SMAX == 4 || SMAX == 5, "4/5-slot rows");
    if (a <= 0xFFFFu - 256u * (SMAX - 2)) {
        if constexpr (SMAX == 4)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tds_write_addtid_b32 %1\n\tds_write_addtid_b32 %2 offset:256\n\t"
                         "ds_write_addtid_b32 %3 offset:512"
                         :: "s"(a), "v"(x[0]), "v"(x[1]), "v"(x[2]) : "memory", "m0");
        else
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tds_write_addtid_b32 %1\n\tds_write_addtid_b32 %2 offset:256\n\t"
                         "ds_write_addtid_b32 %3 offset:512\n\tds_write_addtid_b32 %4 offset:768"
                         :: "s"(a), "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]) : "memory", "m0");
    } else {
        const uint32_t b = a - 32768u;
        if constexpr (SMAX == 4)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tds_write_addtid_b32 %1 offset:32768\n\t"
                         "ds_write_addtid_b32 %2 offset:33024\n\tds_write_addtid_b32 %3 offset:33280"
                         :: "s"(b), "v"(x[0]), "v"(x[1]), "v"(x[2]) : "memory", "m0");
        else
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tds_write_addtid_b32 %1 offset:32768\n\t"
                         "ds_write_addtid_b32 %2 offset:33024\n\tds_write_addtid_b32 %3 offset:33280\n\t"
                         "ds_write_addtid_b32 %4 offset:33536"
                         :: "s"(b), "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]) : "memory", "m0");
    }
}

// The 4/5-slot instances write by ds_write_addtid_b32; the 1-3-slot ones
// (row-slot steps of units with slot tables, merge_levels) by ds_write_b32.
template <int SMAX, int RW>
__device__ __forceinline__ void write_rows_slots(float* base, float* dummy, const float (&v)[RW][SMAX], int p,
                                                 int lane, uint32_t sw, int nq, int q)
{
    const bool tail_ok = lane + 64 * (SMAX - 1) < p;
    if constexpr (resolved_slots(SMAX)) {
        typedef __attribute__((address_space(3))) float* lds_fptr;
        const uint32_t b0 = (uint32_t)(uintptr_t)(lds_fptr)base;
#pragma unroll
        for (int i = 0; i < RW; ++i) {
            if (i / 2 < nq) {
                const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)sw, i / 2);
                if (i % 2 == 0 || (w >> 20) != kSlotOne) {
                    const int row = (int)((i % 2 == 0 ? w : w >> 10) & 1023u);
                    write_row_addtid<SMAX>(b0 + 4u * (uint32_t)(row * q), v[i]);
                    float* orow = base + row * q + lane;
                    *(tail_ok ? orow + 64 * (SMAX - 1) : dummy) = v[i][SMAX - 1];
                }
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < RW; ++i) {
        if (i / 2 < nq) {
            const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)sw, i / 2);
            if (i % 2 == 0 || (w >> 20) != kSlotOne) {
                const int row = (int)((i % 2 == 0 ? w : w >> 10) & 1023u);
                float* orow = base + row * q + lane;
#pragma unroll
                for (int k = 0; k < SMAX; ++k) {
                    if (k < SMAX - 1) orow[64 * k] = v[i][k];
                    else *(tail_ok ? orow + 64 * k : dummy) = v[i][k];
                }
            }
        }
    }
}

template <int SMAX, int RW>
__device__ __forceinline__ void store_rows_slots(const float (&v)[RW][SMAX], int p, int lane, uint32_t sw, int nq,
                                                 __amdgpu_buffer_rsrc_t rs, uint32_t st_o0)
{
    const bool tail_ok = lane + 64 * (SMAX - 1) < p;
#pragma unroll
    for (int i = 0; i < RW; ++i) {
        if (i / 2 < nq) {
            const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)sw, i / 2);
            if (i % 2 == 0 || (w >> 20) != kSlotOne) {
                const int row = (int)((i % 2 == 0 ? w : w >> 10) & 1023u);
                const uint32_t ob = st_o0 + (uint32_t)(row * p + lane) * 4u;
#pragma unroll
                for (int k = 0; k < SMAX; ++k) {
                    const uint32_t o = k < SMAX - 1 ? ob + 256u * (uint32_t)k
                                                    : (tail_ok ? ob + 256u * (uint32_t)k : 0x80000000u);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[i][k]), rs, (int)o, 0, kStoreCpol);
                }
            }
        }
    }
}

// kPack2 merge step (p <= 32; units always with a blob): register row i of
// wave w holds two adjacent output rows, 2(w + 8i) in lanes 0-31 and
// 2(w + 8i) + 1 in lanes 32-63, bin j = lane & 31 (adjacent rows: the two
// halves of a read or write hit disjoint banks -- rows 8 apart, as before,
// collided on every bank at p = 16 or 32).  Every lane resolves its own row's
// descriptor (the two halves read different table words; lanes of a half
// read the same word) and computes its bin's wrapped indices itself: no
// v_readlane and no per-row scalar work, so a wave instruction does the
// work of two rows at the cost of one.  TWO: two levels per step, the
// additions of merge_level2_dense; otherwise one level (carried size-1 nodes
// add -0.0).  Rows past nrows and bins past p compute in-bounds garbage that
// is never written back.
template <int RW, bool TWO, bool FIRST>
__device__ __forceinline__ void merge_step_lanes(const UnitCtx& C, const float* src, int p, int lo, int lane, int wave,
                                                 int nrows, float (&v)[RW][1], const int* loff)
{
    // an opaque copy of the lane, so per-row addresses are not hoisted out of
    // the level loop into 2 x RW long-lived registers (spills)
    int ln = lane;
    asm volatile("" : "+v"(ln));
    // bins past p read bin 0's words (a broadcast, no extra bank cycles)
    const int h = ln >> 5, j = (ln & 31) < p ? (ln & 31) : 0;
    const uint32_t* const desc = desc_table(C);
    const int dl = TWO ? 0 : desc_offset(C, lo);
    const uint2* const step = reinterpret_cast<const uint2*>(TWO ? slot_table(C, lo) : C.aux);
    const lds_cptr sp = (lds_cptr)src;
    // groups of G register rows without a branch between them, so the
    // descriptor chains (2-4 dependent LDS reads per row) of a group overlap
    constexpr int G = 4;
    auto rowidx = [&](int i) {
        const int r = 2 * (wave + kConeWaves * i) + h;
        return r < nrows ? r : nrows - 1;
    };
    // the next row's entry is read before this row's (volatile) data reads:
    // LDS reads complete in order, so a descriptor read issued after them
    // waited for all of them (lgkmcnt(0)) before its decode could start
    uint2 enext = make_uint2(0u, 0u);
    auto row = [&](int i, bool pre) {
        const int r = rowidx(i);
        if constexpr (TWO) {
            // the host-resolved row: source rows q0..q3 of level lo + 2, rolls
            const uint2 e = enext;
            if (pre) enext = step[rowidx(i + 1)];
            const uint32_t q0 = e.x & 1023u, q1 = (e.x >> 10) & 1023u, q2 = (e.x >> 20) & 1023u, q3 = e.y & 1023u;
            const int sH = (int)((e.y >> 10) & 63u), sh = (int)((e.y >> 16) & 63u), sTT = (int)((e.y >> 22) & 63u);
            const int o0 = FIRST ? loff[q0] : (int)__umul24(q0, (uint32_t)p);
            const int o1 = FIRST ? loff[q1] : (int)__umul24(q1, (uint32_t)p);
            const int o2 = FIRST ? loff[q2] : (int)__umul24(q2, (uint32_t)p);
            const int o3 = FIRST ? loff[q3] : (int)__umul24(q3, (uint32_t)p);
            // (j + s) mod p for j, s < p: min of the sum and the sum - p as
            // unsigned (the latter wraps to a huge value below p)
            uint32_t u1 = (uint32_t)(j + sH), u2 = (uint32_t)(j + sh), u3 = (uint32_t)(j + sTT);
            const int i1 = (int)min(u1, u1 - (uint32_t)p), i2 = (int)min(u2, u2 - (uint32_t)p);
            const int i3 = (int)min(u3, u3 - (uint32_t)p);
            const float x0 = lds_ld(sp + o0 + j);
            const float x1 = lds_ld(sp + o1 + i1);
            const float x2 = lds_ld(sp + o2 + i2);
            const float x3 = lds_ld(sp + o3 + i3);
            v[i][0] = __fadd_rn(__fadd_rn(x0, x1), __fadd_rn(x2, x3));
        } else {
            const uint32_t d = desc[dl + r];
            const uint32_t tc = (d >> 10) & 1023u;
            const bool car = tc == kCarried;
            const int sh = (int)(d >> 20);
            const int ho = FIRST ? loff[d & 1023u] : (int)__umul24(d & 1023u, (uint32_t)p);
            const int to = car ? ho : (FIRST ? loff[tc & 1023u] : (int)__umul24(tc, (uint32_t)p));
            const uint32_t u1 = (uint32_t)(j + sh);
            const int i1 = (int)min(u1, u1 - (uint32_t)p);
            const float x0 = lds_ld(sp + ho + j);
            float x1 = lds_ld(sp + to + i1);
            x1 = car ? -0.0f : x1;
            v[i][0] = __fadd_rn(x0, x1);
        }
    };
#pragma unroll
    for (int g = 0; g < RW; g += G) {
        if (2 * (wave + kConeWaves * g) < nrows) {
            const int ge = g + G < RW ? g + G : RW;
            if constexpr (TWO) enext = step[rowidx(g)];
#pragma unroll
            for (int i = g; i < ge; ++i) row(i, i + 1 < ge);
        }
    }
}

template <int RW>
__device__ __forceinline__ void write_rows_lanes(float* base, float* dummy, const float (&v)[RW][1], int p, int lane,
                                                 int wave, int nrows)
{
    // an opaque copy of the lane, so per-row addresses are not hoisted out of
    // the level loop into 2 x RW long-lived registers (spills)
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int h = ln >> 5, j = ln & 31;
#pragma unroll
    for (int i = 0; i < RW; ++i) {
        if (2 * (wave + kConeWaves * i) < nrows) {
            const int r = 2 * (wave + kConeWaves * i) + h;
            *((r < nrows && j < p) ? base + (int)__umul24((uint32_t)r, (uint32_t)p) + j : dummy) = v[i][0];
        }
    }
}

template <int RW>
__device__ __forceinline__ void store_rows_lanes(const float (&v)[RW][1], int p, int lane, int wave, int nrows,
                                                 __amdgpu_buffer_rsrc_t rs, uint32_t st_o0)
{
    // an opaque copy of the lane, so per-row addresses are not hoisted out of
    // the level loop into 2 x RW long-lived registers (spills)
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int h = ln >> 5, j = ln & 31;
#pragma unroll
    for (int i = 0; i < RW; ++i) {
        if (2 * (wave + kConeWaves * i) < nrows) {
            const int r = 2 * (wave + kConeWaves * i) + h;
            const uint32_t o = (r < nrows && j < p) ? st_o0 + (__umul24((uint32_t)r, (uint32_t)p) + (uint32_t)j) * 4u : 0x80000000u;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[i][0]), rs, (int)o, 0, 0);
        }
    }
}

// kPack2 rows of p >= 8 bins as (row, 8-bin segment) tasks, one per lane
// (merge_step_tasks): task t = tid + kConeBlock * i is row t / segs, segment
// t % segs, bins j0 .. j0 + 7 with j0 = min(8 * seg, p - 8) (the last
// segment of a row overlaps the one before it when 8 does not divide p:
// those bins are computed twice, identically, and written twice with the
// same value).  A lane resolves its row's entry once for its 8 bins, the
// head read is the row plus an immediate offset, and a rolled read picks one
// of two bases (before / after the wrap point) per bin: a third of the VALU
// of the lane-per-bin layout, where every lane decoded its row's entry and
// wrapped its own index.  Tasks past the level's rows redo the last task
// (same values, same addresses).  Levels above the fill at the odd stride
// qs = p | 1 (the 32-lane halves of a read or write then hit distinct banks
// for distinct rows).
constexpr int kPackSeg = 8;
constexpr int kPackTasks = 3;                 // tasks per lane: kMaxRows rows x 4 segments
static_assert(kMaxRows * 4 <= kPackTasks * kConeBlock, "short-row tasks per lane");
RT_HD inline int pack_segments(int p) { return (p + kPackSeg - 1) / kPackSeg; }

// task -> (row, first bin); segs in 1..4, t < 2^11
__device__ __forceinline__ void pack_task(int t, int segs, int p, int& r, int& j0)
{
    const uint32_t m = segs == 1 ? (1u << 20) : (segs == 2 ? (1u << 19) : (segs == 3 ? 349526u : (1u << 18)));
    r = (int)(__umul24((uint32_t)t, m) >> 20);
    j0 = min((t - r * segs) * kPackSeg, p - kPackSeg);
}

// The same from the short-row roll table: entry x = j0 + s
// (x < 2p <= 64) holds the byte offsets 4 ((x + e) mod p) of the segment's
// eight elements as bytes: one conflict-free ds_read_b64 per rolled segment,
// then one address add per element (byte select) instead of a compare and a
// select.  Same LDS words: bit-exact.  The table lives in the metadata area,
// which short-row units do not use (their blob is in their level buffer).
__device__ __forceinline__ void pack_rolled_lut(lds_cptr sp, int o, unsigned long long e, float (&x)[kPackSeg])
{
    const lds_ccptr rb = (lds_ccptr)(sp + o);
    const uint32_t e0 = (uint32_t)e, e1 = (uint32_t)(e >> 32);
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = lds_ld((lds_cptr)(rb + ((e0 >> (8 * k)) & 0xFFu)));
#pragma unroll
    for (int k = 0; k < 4; ++k) x[4 + k] = lds_ld((lds_cptr)(rb + ((e1 >> (8 * k)) & 0xFFu)));
}

// Interleaved short-row tasks (SEGS = segs >= 2, every step whose output
// stays in LDS): lane (row, segment s) takes bins s + SEGS * k, k < 8, so the
// segs lanes of a row read consecutive words of each source row (shared
// words broadcast) and a 32-lane group of a read touches few distinct rows'
// words per bank; with the per-p strides of pack_stride the steps' reads run
// at 1.05-1.34 x the conflict-free LDS cycles instead of 1.08-2.25 x (host
// simulation of the cfg4 schedule).  Bins past p (8 * SEGS > p) are computed
// from in-bounds words and written into the row's padding (pack_stride >=
// 8 * SEGS): never read as data.  The interleaved roll table at
// kPackLutI: entry x = s + roll (x < p + SEGS) holds the byte offsets
// 4 ((x + SEGS * e) mod p), e < 8.  The HBM-bound last step of a merge-only
// pass keeps the contiguous tasks (16-byte stores).
constexpr int kPackLutI = 128;                // word offset: past the contiguous table's 4p <= 128 words
static_assert(kPackLutI + 2 * (32 + 4) <= kAuxWords, "short-row roll tables");

__device__ __forceinline__ void build_pack_lut(uint32_t* lut, int p, int tid)
{
    for (int w = tid; w < 4 * p; w += kConeBlock) {
        const int x = (w >> 1) + 4 * (w & 1);
        uint32_t word = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int y = x + i;                        // < 2p + 8 <= 3p (p >= 8)
            y -= y >= p ? p : 0;
            y -= y >= p ? p : 0;
            word |= (uint32_t)(4 * y) << (8 * i);
        }
        lut[w] = word;
    }
    const int segs = pack_segments(p);
    if (segs >= 2)
        for (int w = tid; w < 2 * (p + segs); w += kConeBlock) {
            const int x = w >> 1, e0 = 4 * (w & 1);
            uint32_t word = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int y = x + segs * (e0 + i);      // < p + 8 segs <= 2p + 7 < 3p
                y -= y >= p ? p : 0;
                y -= y >= p ? p : 0;
                word |= (uint32_t)(4 * y) << (8 * i);
            }
            lut[kPackLutI + w] = word;
        }
}

// task -> (row, segment) of the interleaved layout
template <int SEGS>
__device__ __forceinline__ void pack_task_i(int t, int& r, int& seg)
{
    r = t / SEGS;
    seg = t - r * SEGS;
}

// SEGS = 0: contiguous tasks; SEGS = segs >= 2: interleaved tasks
template <bool TWO, bool FIRST, int SEGS>
__device__ __forceinline__ void merge_step_tasks(const UnitCtx& C, const float* src, int p, int qs, int lo, int tid,
                                                 int nrows, float (&v)[kPackTasks][kPackSeg], const int* loff)
{
    const lut_cptr plut = (lut_cptr)(C.aux0 + (SEGS ? kPackLutI : 0));
    const int segs = SEGS ? SEGS : pack_segments(p);
    constexpr int ES = SEGS ? SEGS : 1;           // word stride of a task's bins
    const int ntask = nrows * segs;
    const uint32_t* const desc = desc_table(C);
    const int dl = TWO ? 0 : desc_offset(C, lo);
    const uint2* const step = reinterpret_cast<const uint2*>(TWO ? slot_table(C, lo) : C.aux);
    const lds_cptr sp = (lds_cptr)src;
    // waves whose tasks all lie past the level skip the block (per wave:
    // a partly filled block would otherwise run every wave)
    const int wave0 = tid & ~63;
#pragma unroll
    for (int i = 0; i < kPackTasks; ++i) {
        if (kConeBlock * i + wave0 < ntask) {
            int r, j0;
            if constexpr (SEGS) pack_task_i<SEGS>(min(tid + kConeBlock * i, ntask - 1), r, j0);   // j0: the segment
            else pack_task(min(tid + kConeBlock * i, ntask - 1), segs, p, r, j0);
            float x0[kPackSeg], x1[kPackSeg];
            if constexpr (TWO) {
                // the host-resolved row: source rows q0..q3 of level lo + 2, rolls
                const uint2 e = step[r];
                const uint32_t q0 = e.x & 1023u, q1 = (e.x >> 10) & 1023u, q2 = (e.x >> 20) & 1023u, q3 = e.y & 1023u;
                const int sH = (int)((e.y >> 10) & 63u), sh = (int)((e.y >> 16) & 63u), sTT = (int)((e.y >> 22) & 63u);
                const int o0 = FIRST ? loff[q0] : (int)__umul24(q0, (uint32_t)qs);
                const int o1 = FIRST ? loff[q1] : (int)__umul24(q1, (uint32_t)qs);
                const int o2 = FIRST ? loff[q2] : (int)__umul24(q2, (uint32_t)qs);
                const int o3 = FIRST ? loff[q3] : (int)__umul24(q3, (uint32_t)qs);
                float x2[kPackSeg], x3[kPackSeg];
                const lds_cptr h0 = sp + o0 + j0;
                // table entries first (plain loads), then the volatile reads
                const unsigned long long e1 = plut[j0 + sH], e2 = plut[j0 + sh], e3 = plut[j0 + sTT];
#pragma unroll
                for (int k = 0; k < kPackSeg; ++k) x0[k] = lds_ld(h0 + ES * k);
                pack_rolled_lut(sp, o1, e1, x1);
                pack_rolled_lut(sp, o2, e2, x2);
                pack_rolled_lut(sp, o3, e3, x3);
#pragma unroll
                for (int k = 0; k < kPackSeg; ++k) v[i][k] = __fadd_rn(__fadd_rn(x0[k], x1[k]), __fadd_rn(x2[k], x3[k]));
            } else {
                const uint32_t d = desc[dl + r];
                const uint32_t tc = (d >> 10) & 1023u;
                const bool car = tc == kCarried;
                const int sh = (int)(d >> 20);
                const int ho = FIRST ? loff[d & 1023u] : (int)__umul24(d & 1023u, (uint32_t)qs);
                const int to = car ? ho : (FIRST ? loff[tc & 1023u] : (int)__umul24(tc, (uint32_t)qs));
                const lds_cptr h0 = sp + ho + j0;
                const unsigned long long e1 = plut[j0 + (car ? 0 : sh)];
#pragma unroll
                for (int k = 0; k < kPackSeg; ++k) x0[k] = lds_ld(h0 + ES * k);
                pack_rolled_lut(sp, to, e1, x1);
                // a carried size-1 node adds -0.0 (x + (-0.0) == x: the reference's copy)
#pragma unroll
                for (int k = 0; k < kPackSeg; ++k) v[i][k] = __fadd_rn(x0[k], car ? -0.0f : x1[k]);
            }
        }
    }
}

// short-row tasks stored to HBM with 16-byte stores: a wave instruction
// writes 1 KiB of contiguous rows instead of 64 words 8 apart.  A/B, same
// box, cone ms per cfg4 trial (profiles/r03zi_ab_cfg4.log): 0.771 / 0.772
// with eight 4-byte stores per task, 0.679 / 0.679 with two 16-byte ones,
// S/N identical.
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

template <bool GLOBAL, int SEGS>
__device__ __forceinline__ void put_tasks(float* base, int q, const float (&v)[kPackTasks][kPackSeg], int p, int tid,
                                          int nrows, __amdgpu_buffer_rsrc_t rs, uint32_t st_o0)
{
    static_assert(!(GLOBAL && SEGS), "HBM stores take the contiguous tasks");
    const int segs = SEGS ? SEGS : pack_segments(p);
    constexpr int ES = SEGS ? SEGS : 1;
    const int ntask = nrows * segs;
    const int wave0 = tid & ~63;
#pragma unroll
    for (int i = 0; i < kPackTasks; ++i) {
        if (kConeBlock * i + wave0 < ntask) {
            int r, j0;
            if constexpr (SEGS) pack_task_i<SEGS>(min(tid + kConeBlock * i, ntask - 1), r, j0);
            else pack_task(min(tid + kConeBlock * i, ntask - 1), segs, p, r, j0);
            if constexpr (GLOBAL) {
                const uint32_t ob = st_o0 + (uint32_t)(r * p + j0) * 4u;
                // the task's 8 bins as two 16-byte stores (dword-aligned
                // multi-dword buffer stores)
#pragma unroll
                for (int k = 0; k < kPackSeg; k += 4) {
                    const v4u w = {__float_as_uint(v[i][k]), __float_as_uint(v[i][k + 1]),
                                   __float_as_uint(v[i][k + 2]), __float_as_uint(v[i][k + 3])};
                    __builtin_amdgcn_raw_buffer_store_b128(w, rs, (int)(ob + 4u * k), 0, 0);
                }
            } else {
                float* const o = base + r * q + j0;
#pragma unroll
                for (int k = 0; k < kPackSeg; ++k) o[ES * k] = v[i][k];
            }
        }
    }
}

// All merge levels of one unit, deepest first, in place in the dense rows
// at `base`.  SMAX >= ceil(p/64) slots per row, RW rows per wave
// (lds_row_capacity(p, SMAX) guarantees ceil(rows/8) <= RW at every level).
// Each level's outputs are staged in registers between two barriers, then
// written back.  With `st` set (a non-final pass), the output level goes from
// the staging registers straight to global memory instead of back into LDS.
// pre_store(): called by every wave after the last merge step's LDS reads
// and before its output level is stored from registers (st): the level
// buffer is then free for the next trial's fill.  A final pass's output
// level (row-slot steps) starts oshift floats past base.
template <int SMAX, int RW, class PreStore>
__device__ __forceinline__ void merge_levels(const UnitCtx& C, float* base, int p, int L, int tid, bool st,
                                             __amdgpu_buffer_rsrc_t rs, uint32_t st_o0, uint32_t flags, float* dummy,
                                             int qout, int oshift, PreStore&& pre_store)
{
    const int lane = tid & 63, wave = tid >> 6;
    const bool tile = C.tile;
    const int node_size = C.U.node_size;
    // the first step reads the bottom level in its fill layout: through the
    // blob's bottom-row offsets, or (whole unit without a blob) as dense rows
    // at the block's 16-byte phase; every later level is dense rows (stride
    // p) at base
    const int* const loff = C.table ? bottom_offsets(C) : nullptr;
    float* const src0 = C.table ? base : base + C.al;
    // deepest first; two levels per step (merge_level2_dense) once no level
    // below the step's output holds size-1 nodes, single steps before that
    // and for a last odd level
    const bool fuse = (flags & kConeFuse2) != 0;
    if constexpr (SMAX == kPack2) {
        if (p >= kPackSeg) {
            const int qs = pack_stride(p);
            for (int l = L - 1; l >= 0;) {
                const bool two = fuse && l >= 1 && (tile || (node_size >> l) >= 2);
                const int lo = two ? l - 1 : l;
                const int nrows = rows_at(C, lo);
                float v[kPackTasks][kPackSeg];
                const bool first = l == L - 1;
                const float* src = first ? src0 : base;
                // interleaved tasks unless the step's output goes to HBM
                const int segs = pack_segments(p);
                const int inter = (segs >= 2 && !(lo == 0 && st)) ? segs : 0;
                auto step = [&](auto sc) {
                    constexpr int S = decltype(sc)::value;
                    if (first) {
                        if (two) merge_step_tasks<true, true, S>(C, src, p, qs, lo, tid, nrows, v, loff);
                        else merge_step_tasks<false, true, S>(C, src, p, qs, lo, tid, nrows, v, loff);
                    } else {
                        if (two) merge_step_tasks<true, false, S>(C, src, p, qs, lo, tid, nrows, v, nullptr);
                        else merge_step_tasks<false, false, S>(C, src, p, qs, lo, tid, nrows, v, nullptr);
                    }
                };
                if (inter == 2) step(IntC<2>{});
                else if (inter == 3) step(IntC<3>{});
                else if (inter == 4) step(IntC<4>{});
                else step(IntC<0>{});
                l = lo - 1;
                if (lo == 0 && st) {
                    pre_store();
                    put_tasks<true, 0>(base, qs, v, p, tid, nrows, rs, st_o0);
                    return;
                }
                if (!(flags & kConeDiagNoBarrier)) lds_barrier();
                // the output level (lo == 0) at the caller's stride qout
                if (!(flags & kConeDiagNoWrite)) {
                    const int qw = lo == 0 ? qout : qs;
                    if (inter == 2) put_tasks<false, 2>(base, qw, v, p, tid, nrows, rs, st_o0);
                    else if (inter == 3) put_tasks<false, 3>(base, qw, v, p, tid, nrows, rs, st_o0);
                    else if (inter == 4) put_tasks<false, 4>(base, qw, v, p, tid, nrows, rs, st_o0);
                    else put_tasks<false, 0>(base, qw, v, p, tid, nrows, rs, st_o0);
                }
                if (!(flags & kConeDiagNoBarrier)) lds_barrier();
            }
            return;
        }
        for (int l = L - 1; l >= 0;) {
            const bool two = fuse && l >= 1 && (tile || (node_size >> l) >= 2);
            const int lo = two ? l - 1 : l;
            const int nrows = rows_at(C, lo);
            float v[RW][1];
            const bool first = l == L - 1;
            const float* src = first ? src0 : base;
            const int* lo_src = first ? loff : nullptr;
            if (first) {
                if (two) merge_step_lanes<RW, true, true>(C, src, p, lo, lane, wave, nrows, v, lo_src);
                else merge_step_lanes<RW, false, true>(C, src, p, lo, lane, wave, nrows, v, lo_src);
            } else {
                if (two) merge_step_lanes<RW, true, false>(C, src, p, lo, lane, wave, nrows, v, lo_src);
                else merge_step_lanes<RW, false, false>(C, src, p, lo, lane, wave, nrows, v, lo_src);
            }
            l = lo - 1;
            if (lo == 0 && st) {
                pre_store();
                store_rows_lanes<RW>(v, p, lane, wave, nrows, rs, st_o0);
                return;
            }
            if (!(flags & kConeDiagNoBarrier)) lds_barrier();
            if (!(flags & kConeDiagNoWrite)) write_rows_lanes<RW>(base, dummy, v, p, lane, wave, nrows);
            if (!(flags & kConeDiagNoBarrier)) lds_barrier();
        }
        return;
    }
    if constexpr (SMAX <= 5) {
        // the 4/5-slot instances (p = 193-320) run only row-slot steps: every
        // unit of theirs carries slot tables (validate_exec_plan; unit_begin
        // refuses a unit without them), so the dense per-level paths below are
        // compiled out of these, the hottest instances
        if (resolved_slots(SMAX) || (C.slots && fuse)) {
            // row-slot steps (the host's slot tables follow this step order;
            // a unit with a zero row fuses every step)
            const bool all2 = C.U.zero_row != 0;
            for (int l = L - 1; l >= 0;) {
                const bool two = l >= 1 && (tile || all2 || (node_size >> l) >= 2);
                const int lo = two ? l - 1 : l;
                float v[RW][SMAX];
                const bool first = l == L - 1;
                const float* src = first ? src0 : base;
                const int* lo_src = first ? loff : nullptr;
                uint32_t sw;
                int nq;
                if (two) merge_step_slots<SMAX, RW, true>(C, src, p, lo, lane, wave, v, lo_src, sw, nq);
                else merge_step_slots<SMAX, RW, false>(C, src, p, lo, lane, wave, v, lo_src, sw, nq);
                l = lo - 1;
                if (lo == 0 && st) {
                    pre_store();
                    store_rows_slots<SMAX, RW>(v, p, lane, sw, nq, rs, st_o0);
                    return;
                }
                if (!(flags & kConeDiagNoBarrier)) lds_barrier();
                // the output level of a final pass at row stride qout (the S/N's)
                if (!(flags & kConeDiagNoWrite))
                    write_rows_slots<SMAX, RW>(lo == 0 ? base + oshift : base, dummy, v, p, lane, sw, nq,
                                               lo == 0 ? qout : p);
                if (!(flags & kConeDiagNoBarrier)) lds_barrier();
            }
            return;
        }
    }
    if constexpr (!resolved_slots(SMAX)) {
    for (int l = L - 1; l >= 0;) {
        // size-1 nodes exist at depth l only in whole units with node_size >> l < 2
        const bool two = fuse && l >= 1 && (tile || (node_size >> l) >= 2);
        const int lo = two ? l - 1 : l;          // output level of this step
        const int orows = rows_at(C, lo);
        const int nr = uni(orows > wave ? (orows - wave + kConeWaves - 1) / kConeWaves : 0);
        constexpr int S = slot_count(SMAX);
        float v[RW][S];
        const bool carried = !tile && (node_size >> l) < 2;
        const bool first = l == L - 1;
        const float* src = first ? src0 : base;
        const int* lo_src = first ? loff : nullptr;
        if (two)
            merge_level2_dense<S, RW>(C, src, p, lo, lane, wave, nr, v, lo_src);
        else if (carried)
            merge_level_dense<S, RW, true>(C, src, p, l, lane, wave, nr, v, lo_src);
        else
            merge_level_dense<S, RW, false>(C, src, p, l, lane, wave, nr, v, lo_src);
        l = lo - 1;
        if (lo == 0 && st) {
            pre_store();
            store_rows<S, RW>(v, p, lane, wave, nr, rs, st_o0);
            return;
        }
        if (!(flags & kConeDiagNoBarrier)) lds_barrier();
        if (!(flags & kConeDiagNoWrite)) {
            write_rows<S, RW>(base, dummy, v, p, lane, wave, nr);
        }
        if (!(flags & kConeDiagNoBarrier)) lds_barrier();
    }
    }
}

}  // namespace rt
