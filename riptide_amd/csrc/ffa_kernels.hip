// FFA periodogram hot path for MI355X (gfx950): the LDS cone kernel (several
// FFA merge levels per HBM pass) with its fused boxcar S/N epilogue, and the
// global-memory fallback for rows too wide for it.  The downsampling ladder
// is ladder_kernels.hip; the cone kernel's parts are the fragments
// cone_unit.hpp (unit view, fill, descriptors), cone_merge.hpp (merge steps)
// and cone_snr.hpp (S/N), included below in that order.
//
// Exactness: every float operation that the reference performs is performed
// here on the same operands in the same association (explicit *_rn intrinsics
// where hipcc would otherwise contract into FMA), so the FFA transform is
// bit-identical to riptide::transform (transforms.hpp:30-61).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "common.hpp"
#include "kernels.hpp"

// ---------------------------------------------------------------------------
// Cone kernel
// ---------------------------------------------------------------------------
// A work unit = one work item (UnitDesc) of one trial: `levels` merge levels
// of the FFA recursion for the rows of one tile (or one whole node), in LDS.
//   1. begin: the unit's view (one scalar load of its UnitDesc); the bottom
//      level is LDS-DMA'd from the transform block (a whole unit: one run of
//      16-byte chunks; a tile unit: one run per range of its dependency cone,
//      listed in the host-built blob, which is DMA'd alongside: rows per
//      level, the row-descriptor table of every level, the bottom rows' LDS
//      offsets -- build_tile_blob, plan.cpp)
//   2. merge levels, deepest first (transforms.hpp:13-27), one row per wave
//      and one phase bin per lane, two levels per LDS round trip where no
//      level holds size-1 nodes:
//          out[r][j] = H[h(r)][j] + T[t(r)][(j + shift(r)) mod p]
//      Lane i holds the descriptor of the wave's i-th row as LDS offsets;
//      the row loop takes them with v_readlane.  Bins j = lane + 64k use
//      immediate offsets, so a 64-bin slot is one ds_read per operand
//      (consecutive lanes -> consecutive banks) and one ds_write.  A step's
//      outputs are staged in registers between two barriers (in place).
//   3. a non-final pass stores its last level straight from the registers;
//      a final pass runs the fused boxcar S/N epilogue (snr.hpp:37-65) on it.
// Whole units compute their descriptors on the fly (node partition
// arithmetic, no table).
#include "cone_unit.hpp"
#include "cone_merge.hpp"
#include "cone_snr.hpp"

namespace rt {

// Diagnostic build only (make stamps, -DRT_STAMPS): thread 0 of every unit
// writes one record of s_memtime marks at phase boundaries to a.stamps +
// kStampRecWords * u (the host offsets a.stamps per launch; no atomics, so
// the timing is not perturbed by contention).
#ifdef RT_STAMPS
#define RT_MARK(i)                                                               \
    do {                                                                         \
        if (tid == 0) tl[i] = __builtin_amdgcn_s_memtime();                      \
    } while (0)
#else
#define RT_MARK(i) do { } while (0)
#endif

// One kernel per merge slot width SMAX (units with ceil(p/64) <= SMAX), so each
// gets its own register allocation; one workgroup per unit u = blockIdx.x
// (workgroup b runs item b / G for one of its G trial groups, ConeArgs::
// trials_per_wg; the planner orders a launch's items for dispatch -- longest
// first, pass 0 by rung and leaf span, plan.cpp order_launch_units -- and
// nothing here depends on that order),
// two workgroups per CU: a unit's DMA is waited for at its start, the CU's
// other workgroup filling the wait.
//   begin(u) [DMA] | wait | merge(u) | store or S/N(u)
// SNR (kSnrNone / kSnrRows / kSnrSeg): the launch's units all end in the
// fused S/N (final passes), all in its row-group form (snr_epilogue) or all in
// its segmented form (snr_segments) -- or none does (the merge-only passes
// store their output level): separate instances, so a merge-only launch
// carries no S/N code and no S/N register floor, and a final launch only its
// own form's (the planner keys final launches by the form, plan.cpp
// final_snr_kind; the segmented form exists for the 4/5-slot instances).
// WIDE: final units whose S/N takes the widths past its register window as
// plain LDS windows (snr_wide_ok; a separate instantiation, so the plans
// without such widths run code without it)
// instances whose workgroups run several trials of an item (ConeArgs::
// trials_per_wg); the others one trial each
template <int SMAX> constexpr bool kTrialLoop = SMAX >= 4;

template <int SMAX, bool WIDE, uint32_t SNR>
__global__ __launch_bounds__(kConeBlock, kConeWavesPerSimd) void cone_kernel(ConeArgs a)
{
    constexpr bool FIN = SNR != kSnrNone;   // a final launch
    constexpr bool SEG = SNR == kSnrSeg;    // ... of the segmented S/N
    static_assert(SNR <= kSnrSeg && (!WIDE || SNR == kSnrRows), "S/N kind");
    static_assert(!SEG || resolved_slots(SMAX), "the segmented S/N: 4/5-slot instances");
    constexpr int RW = merge_rows_per_wave(SMAX);   // register rows per wave
    __shared__ __attribute__((aligned(16))) float data[kLdsBufFloats + kLdsPadFloats];
    __shared__ __attribute__((aligned(16))) uint32_t aux[kAuxWords + kLutPad];   // the host blob (+ roll table)
    // boxcar widths (LDS reads never wait on the S/N stores in flight), then
    // the widest of them
    __shared__ int wl[kMaxWidths + 1];
    __shared__ float whb[2 * kMaxWidths];   // S/N: h + b and b per width

    const int tid = threadIdx.x;
#ifdef RT_STAMPS
    unsigned long long t_entry = __builtin_amdgcn_s_memtime();
    unsigned long long r_entry = __builtin_amdgcn_s_memrealtime();
    unsigned long long t_begin[3] = {};
#endif
    // workgroup -> (item, its trials t0 .. t0 + tn - 1); the 1-3-slot
    // instances (p = 33-192, no BASELINE config) run one trial per workgroup
    // (launch_cone): their trial loop would spill
    const uint32_t tpw = (kTrialLoop<SMAX> && a.trials_per_wg) ? a.trials_per_wg : 1u;
    const uint32_t groups = cone_trial_groups(a.batch, tpw);
    const uint32_t total = a.num_items * groups;
    if (blockIdx.x >= total) return;
    const uint32_t item = blockIdx.x / groups;
    const uint32_t t0 = (blockIdx.x - item * groups) * tpw;
    const int tn = (int)min(tpw, a.batch - t0);
    if (tid < (int)a.num_widths) wl[tid] = (int)a.widths[tid];   // visible after the first barrier
    if (tid == 0) {
        uint32_t wm = 0;
        for (uint32_t i = 0; i < a.num_widths; ++i) wm = max(wm, a.widths[i]);
        wl[kMaxWidths] = (int)wm;
    }
    const bool dma = !(a.flags & kConeDiagNoLand);
    bool ok;
#ifdef RT_STAMPS
    UnitCtx C = unit_begin<SMAX, RW>(a, item, t0, aux, data, tid, dma, ok, t_begin);
    unsigned long long tl[kStampMarks] = {};
    tl[0] = __builtin_amdgcn_s_memtime();
#else
    UnitCtx C = unit_begin<SMAX, RW>(a, item, t0, aux, data, tid, dma, ok);
#endif
    const UnitView& U = C.U;
    const int p = U.p;
    const int L = U.levels;
    float* const buf = data;
    // the launch kind is the unit's (the planner splits final and merge-only
    // launches; validate_exec_plan)
    // -- a final launch's instance also the unit's S/N form: a unit planned
    // for the segmented form runs the row-group one where the feature bit is
    // off at run time (launch_cone picks the instance by the same rule)
    {
        const uint32_t ukind = U.dst == kSelSnrSeg ? ((a.flags & kConeSnrSeg) ? kSnrSeg : kSnrRows)
                                                   : (U.dst == kSelSnr ? kSnrRows : kSnrNone);
        ok = ok && ukind == SNR;
    }
    // a final pass's per-width S/N constants, published by the barrier below
    // (the S/N row passes have no barrier of their own)
    if (FIN && tid < (int)a.num_widths) snr_width_consts(wl[tid], p, whb + 2 * tid);
    // the roll table of a 4-slot unit (past its blob's LDS part, which the
    // DMA may still be writing), published by the barrier below
    if constexpr (SMAX == 4)
        if (C.slots && ok) build_roll_lut4(aux + kLut4Off, p, tid);
    // the -0.0 row of an all-fused whole unit (past the fill: no trial's DMA
    // or merge level writes it, so once per workgroup)
    if constexpr (resolved_slots(SMAX))
        if (ok && U.zero_row)
            for (int j = tid; j < 64 * SMAX; j += kConeBlock) data[U.zero_row + j] = -0.0f;
    // the short-row roll table in the unused metadata area
    if constexpr (SMAX == kPack2)
        if (ok && p >= kPackSeg) build_pack_lut(aux, p, tid);
    // every wave waits for its own DMA, the barrier publishes all of them
    __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0)
    lds_barrier();
    RT_MARK(1);
    RT_MARK(2);
    // the segmented instance runs only the units of its form (snr_seg_unit,
    // the planner's rule: <= 64 output rows in segment slots, widths <= 9),
    // with the slot tables whose last step writes those slots
    if constexpr (SEG)
        ok = ok && C.slots && snr_seg_unit(SMAX, L, p, wl[kMaxWidths], rows_at(C, 0));
    if (!ok) {
        if (tid == 0 && a.error_flag) atomicOr(a.error_flag, 1);
        return;
    }
    // merge levels, deepest first; a non-final pass stores its output level
    // straight from registers (st), a final pass keeps it in LDS for the S/N
    // epilogue
    constexpr bool st = !FIN;
    const bool st_regs = st && (a.flags & kConeStoreFromRegs);
    const uint32_t o0 = (uint32_t)(U.node_start + U.s0) * (uint32_t)p * 4u;
    const int n0 = rows_at(C, 0);
    // a final pass's output level at a row stride = 16 (mod 32): the S/N
    // epilogue's lane groups (two rows of 16 lanes per 32-lane LDS group, odd
    // chunk strides) then read and write on distinct banks (at stride p they
    // collided on up to 10 of 32 banks)
    // (the segmented S/N, snr_segments: rows of 240-264 bins, widths <= 9,
    // <= 64 rows in slots of kSnrSegStride floats -- a compile-time constant
    // in its instance, which holds none of the strides selected below)
    int qout = SEG ? kSnrSegStride : p;
    // short rows keep their blob's LDS part at the end of the level buffer,
    // which a final pass's output level (at the S/N stride) and its S/N's
    // dummy words may overwrite: every trial's fill then re-DMAs it -- unless
    // the output level at the short-row S/N stride ends below the blob (set
    // below: that stride takes the S/N's whole-chunk path, which writes no
    // dummy words, only the rows [0, n0 q) and their wrapped extensions)
    bool blob_clobbered = SMAX == kPack2 && FIN;
    // short rows in (row, segment) tasks: every level above the fill at the
    // odd stride pack_stride(p)
    if constexpr (SMAX == kPack2) {
        if (L > 0) qout = pack_stride(p);
        // a final pass's output level at the short-row S/N stride where the
        // unit's rows fit (over the blob: the blob is dead once the last
        // merge step has read its table, a barrier before the level's
        // write-back)
        if (FIN && L > 0 && p >= kPackSeg && (a.flags & kConeSnrStride)) {
            const int qf = snr_short_stride(p);
            if (n0 * qf <= kLdsDataFloats) qout = qf;
            // the blob survives the S/N: loaded once per workgroup, not per
            // trial (cfg4's final units re-read ~12 KB of
            // blob per trial, 0.1 GB of its 1.34 GB)
            if (qout == qf && n0 * qf + U.run_off <= kLdsBufFloats) blob_clobbered = false;
        }
    }
    if constexpr (SMAX <= 5 && SMAX != kPack2 && !SEG) {
        // = 16 (mod 32) and >= p + kSnrMaxChunk (room for the S/N's whole-
        // chunk prefix writes and its wrapped prefix extension), else >=
        // p + kSnrWin (the extension only)
        const int qa = p + kSnrMaxChunk + ((16 - ((p + kSnrMaxChunk) & 31)) & 31);
        const int qb = p + kSnrWin + ((16 - ((p + kSnrWin) & 31)) & 31);
        if (!st && L > 0 && C.slots && (a.flags & kConeFuse2) && (a.flags & kConeSnrStride)) {
            qout = n0 * qa <= kLdsDataFloats ? qa : (n0 * qb <= kLdsDataFloats ? qb : p);
            // widths past the register window: a stride with room for their
            // plain-LDS windows (snr_wide_stride), = 16 (mod 32) where that
            // fits too
            const int wmax = wl[kMaxWidths];
            if (WIDE && snr_group(p) == 16 && wmax > kSnrWin && wmax < p) {
                const int qw = snr_wide_stride(p, wmax);
                const int qwp = qw + ((16 - (qw & 31)) & 31);
                if (n0 * qwp <= kLdsDataFloats) qout = qwp;
                else if (n0 * qw <= kLdsDataFloats) qout = qw;
            }
        }
    }
    // the trials of this workgroup, one after the other: trial k's level
    // buffer is free once its last merge step has read it (merge-only units
    // store that step from registers: the next trial's fill is issued before
    // those stores) or once its S/N has read it (final units)
    for (int k = 0;;) {
        const int trial = C.U.trial;
        const float* dst = (U.dst == kSelPing ? a.ping : a.pong) + (uint64_t)trial * a.buf_stride + U.buf_off;
        const __amdgpu_buffer_rsrc_t rs = buffer_rsrc(dst, (((uint32_t)U.m * (uint32_t)p + 3u) & ~3u) * 4u);
        const bool more = k + 1 < tn;
        bool next_issued = false;
        auto fill_next = [&]() {
            if (more) {
                lds_barrier();           // every wave is past its last read of the level buffer
                if (dma) unit_fill<SMAX>(a, C, trial + 1, buf, tid, blob_clobbered);
            }
            next_issued = true;
        };
        if (L > 0 && !(a.flags & kConeDiagNoMerge))
            merge_levels<SMAX, RW>(C, buf, p, L, tid, st_regs, rs, o0, a.flags, buf + kLdsBufFloats + 4 + (tid & 63),
                                   qout, SEG ? 8 * kSnrSegCols - p : 0, fill_next);
        RT_MARK(3);
        // the output level: dense rows from the buffer start, or (no merge
        // level) the single bottom row where the DMA left it
        float* const obase = L > 0 ? buf : buf + (C.table ? uni(bottom_offsets(C)[0]) : C.al);
        if (st) {
            if (L == 0 || !st_regs) {
                const int qst = L > 0 ? qout : p;    // the merged level's LDS row stride
                for (int r = 0; r < n0; ++r)
                    for (int j = tid; j < p; j += kConeBlock)
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(obase[r * qst + j]), rs,
                                                              (int)(o0 + (uint32_t)(r * p + j) * 4u), 0, kStoreCpol);
            }
        } else if constexpr (SEG) {
            if (!(a.flags & kConeDiagNoSnr)) snr_segments<SMAX>(a, C.U, buf, wl, n0, tid, whb);
        } else if constexpr (FIN) {
#ifdef RT_STAMPS
            if (!(a.flags & kConeDiagNoSnr)) snr_epilogue<SMAX, WIDE>(a, C.U, obase, qout, wl, n0, tid, whb, tl);
#else
            if (!(a.flags & kConeDiagNoSnr)) snr_epilogue<SMAX, WIDE>(a, C.U, obase, qout, wl, n0, tid, whb, nullptr);
#endif
        }
#ifdef RT_STAMPS
        lds_barrier();
        RT_MARK(4);
        tl[5] = t_entry;
        tl[11] = t_begin[0];
        tl[12] = t_begin[1];
        tl[13] = t_begin[2];
        RT_MARK(6);
        tl[14] = r_entry;
        tl[15] = __builtin_amdgcn_s_memrealtime();
        if (tid == 0 && a.stamps) {
            unsigned long long* e = a.stamps + (uint64_t)kStampRecWords * ((uint64_t)item * a.batch + (uint32_t)trial);
            const uint32_t hw = (uint32_t)__builtin_amdgcn_s_getreg(4 | (31 << 11));     // HW_REG_HW_ID
            const uint32_t xcc = (uint32_t)__builtin_amdgcn_s_getreg(20 | (31 << 11));   // HW_REG_XCC_ID
            e[0] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
#pragma unroll
            for (int i = 0; i < kStampMarks; ++i) e[1 + i] = tl[i];
            e[1 + kStampMarks] = (unsigned long long)p | ((unsigned long long)L << 16) |
                                 ((unsigned long long)U.mode << 24) | ((unsigned long long)rows_at(C, 0) << 32) |
                                 ((unsigned long long)is_snr_dst(U.dst) << 48);
        }
#endif
        if (!kTrialLoop<SMAX> || !more) break;
        // final units (and merge-only units not stored from registers): the
        // next trial's fill once every wave is done with the level buffer
        if (!next_issued) fill_next();
        // a final unit's output level (at the S/N stride) may have covered the
        // zero row: rewritten for the next trial (its first step reads it)
        if constexpr (resolved_slots(SMAX) && FIN)
            if (U.zero_row)
                for (int j = tid; j < 64 * SMAX; j += kConeBlock) data[U.zero_row + j] = -0.0f;
        ++k;
        C.U.trial = trial + 1;
#ifdef RT_STAMPS
        t_entry = __builtin_amdgcn_s_memtime();
        r_entry = __builtin_amdgcn_s_memrealtime();
        t_begin[0] = t_begin[1] = t_begin[2] = t_entry;
        tl[0] = t_entry;
#endif
        // the next trial's fill (and this trial's stores, which count in the
        // same in-order counter) landed; the barrier publishes every wave's
        __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0)
        lds_barrier();
        RT_MARK(1);
        RT_MARK(2);
    }
    // every DMA was waited for before its trial, and the stores need no wait
    // before the end of the program
}

// One workgroup per unit: the hardware dispatcher keeps both of a CU's
// workgroup slots busy to the end of the launch (measured: 10.37 vs 11.55 ms
// per cfg2 trial against a persistent grid, round 1).
template <int SMAX>
static hipError_t launch_kind(const ConeArgs& args, dim3 g, dim3 b, bool wide_snr, uint32_t snr, hipStream_t s)
{
    if (snr == kSnrNone) {
        if (wide_snr) return hipErrorInvalidValue;
        hipLaunchKernelGGL((cone_kernel<SMAX, false, kSnrNone>), g, b, 0, s, args);
    } else if (snr == kSnrSeg) {
        // the segmented S/N: 4/5-slot units only, never with wide widths
        if (wide_snr || !resolved_slots(SMAX)) return hipErrorInvalidValue;
        if constexpr (resolved_slots(SMAX)) hipLaunchKernelGGL((cone_kernel<SMAX, false, kSnrSeg>), g, b, 0, s, args);
    } else if (snr != kSnrRows) {
        return hipErrorInvalidValue;
    } else if (wide_snr && SMAX >= 3 && SMAX <= 5) {
        // (the other instances have no WIDE form: their S/N reads the wide
        // widths through the general per-width path)
        if constexpr (SMAX >= 3 && SMAX <= 5) hipLaunchKernelGGL((cone_kernel<SMAX, true, kSnrRows>), g, b, 0, s, args);
    } else {
        hipLaunchKernelGGL((cone_kernel<SMAX, false, kSnrRows>), g, b, 0, s, args);
    }
    return hipSuccess;
}

hipError_t launch_cone(const ConeArgs& args_in, uint32_t smax, bool wide_snr, uint32_t snr, hipStream_t s)
{
    if (!args_in.num_items || !args_in.batch) return hipSuccess;
    ConeArgs args = args_in;
    // a segmented launch with the feature bit off at run time (A/B): its
    // units run the row-group S/N (cone_kernel's unit-kind check agrees)
    if (snr == kSnrSeg && !(args.flags & kConeSnrSeg)) snr = kSnrRows;
    if (smax < 4) args.trials_per_wg = 1;    // kTrialLoop: one trial per workgroup
    const uint64_t total = (uint64_t)args.num_items * cone_trial_groups(args.batch, args.trials_per_wg);
    if (total > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const dim3 g((uint32_t)total), b(kConeBlock);
    hipError_t e = hipErrorInvalidValue;
    // one instance per slot width: every unit runs the variant's register
    // rows, merge_rows_per_wave(smax)
    switch (smax) {
    case 1: e = launch_kind<1>(args, g, b, wide_snr, snr, s); break;
    case 2: e = launch_kind<2>(args, g, b, wide_snr, snr, s); break;
    case 3: e = launch_kind<3>(args, g, b, wide_snr, snr, s); break;
    case 4: e = launch_kind<4>(args, g, b, wide_snr, snr, s); break;
    case 5: e = launch_kind<5>(args, g, b, wide_snr, snr, s); break;
    case 8: e = launch_kind<8>(args, g, b, wide_snr, snr, s); break;
    case 11: e = launch_kind<11>(args, g, b, wide_snr, snr, s); break;
    case 16: e = launch_kind<16>(args, g, b, wide_snr, snr, s); break;
    case 22: e = launch_kind<22>(args, g, b, wide_snr, snr, s); break;
    case kMaxSlots: e = launch_kind<kMaxSlots>(args, g, b, wide_snr, snr, s); break;
    case kPack2: e = launch_kind<kPack2>(args, g, b, wide_snr, snr, s); break;
    default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Fallback for rows too wide for the LDS cone kernel (ffa2 with p > ~11k):
// one launch per tree depth, one workgroup per output row, global memory.
// nodes[] = (start, size) of every node at this depth, sorted by start.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ffa_level_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                        const uint2* __restrict__ nodes, uint32_t num_nodes,
                                                        uint32_t p)
{
    const uint32_t u = blockIdx.x;
    uint32_t lo = 0, hi = num_nodes - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (nodes[mid].x <= u) lo = mid; else hi = mid - 1;
    }
    const uint2 nd = nodes[lo];
    const float* hrow;
    const float* trow = nullptr;
    uint32_t shift = 0;
    if (nd.y <= 1) {
        hrow = in + (uint64_t)u * p;
    } else {
        const uint32_t s = u - nd.x, sh = nd.y >> 1, st = nd.y - sh;
        const uint32_t h = merge_index(merge_coef(sh, nd.y), s);
        const uint32_t t = merge_index(merge_coef(st, nd.y), s);
        hrow = in + (uint64_t)(nd.x + h) * p;
        trow = in + (uint64_t)(nd.x + sh + t) * p;
        shift = (s - t) % p;
    }
    float* o = out + (uint64_t)u * p;
    for (uint32_t j = threadIdx.x; j < p; j += 256) {
        float v = hrow[j];
        if (trow) {
            uint32_t c = j + shift;
            if (c >= p) c -= p;
            v = __fadd_rn(v, trow[c]);
        }
        o[j] = v;
    }
}

hipError_t launch_ffa_level(const float* in, float* out, const uint2* d_nodes, uint32_t num_nodes,
                            uint32_t rows, uint32_t p, hipStream_t s)
{
    hipLaunchKernelGGL(ffa_level_kernel, dim3(rows), dim3(256), 0, s, in, out, d_nodes, num_nodes, p);
    return hipGetLastError();
}

}  // namespace rt
