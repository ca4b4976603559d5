// Fragment of the cone translation unit (ffa_kernels.hip), device code only:
// a work unit's wave-uniform view and context, its LDS-DMA fill, and the row
// descriptors of its merge levels.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace rt {

// Cache policy bits (gfx950: 1 sc0, 2 nt, 16 sc1) of the fill's LDS-DMA
// loads, of the merge passes' output stores and of the S/N stores.  A/B,
// same box, cone ms per trial (profiles/r03zg_ab_*.log): nt stores cfg2
// 7.663 -> 7.616, cfg3 1.907 -> 1.883 (the next pass reads them from HBM
// anyway); nt fills 7.86 / 1.94, slower (adjacent tiles' cones overlap and
// share their L2 lines) -- stores nt, fills default.  Only the whole-slot
// stores (64 consecutive words per wave instruction) are nt: the short-row
// stores (4-byte scattered per lane) took cfg4 from 0.776 to 1.306 ms per
// trial with nt (r03zh_ab_cfg4.log) and keep the default.
constexpr int kFillCpol = 0, kStoreCpol = 2, kSnrCpol = 0;

// LDS-only workgroup barrier: orders LDS accesses without waiting for the
// global loads or stores that are still in flight.
__device__ __forceinline__ void lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ uint64_t uni64(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

template <class T>
__device__ __forceinline__ T* uni_ptr(T* p)
{
    return reinterpret_cast<T*>(uni64(reinterpret_cast<uint64_t>(p)));
}

// Wave-uniform view of one unit (scalar registers).
struct UnitView {
    int item, trial;
    int node_start, node_size, s0, s1, levels, mode, src, dst;
    int p, m, rows_eval;
    uint64_t src_off, buf_off, snr_row;
    float stdnoise;
    uint32_t blob;            // word offset of the host-built blob (kNoBlob: none)
    int nruns, entries, nb, slot_words, run_off;   // its header counts
    int fill_chunks;          // 16-byte chunks of the bottom-level fill
    int zero_row;             // LDS float offset of the unit's -0.0 row (0: none; kHdrZero)
};

typedef const __attribute__((address_space(4))) uint32_t* const_u32_ptr;

__device__ __forceinline__ UnitView unit_view(const ConeArgs& a, int item, int trial)
{
    UnitView v;
    v.item = uni(item);
    v.trial = uni(trial);
    // constant address space: scalar (SMEM) loads, counted in lgkmcnt, so
    // they never wait behind the vector-memory queue (DMA fills, stores)
    const const_u32_ptr w = (const_u32_ptr)(uintptr_t)(a.items + v.item);
    uint32_t x[sizeof(UnitDesc) / 4];
#pragma unroll
    for (int i = 0; i < (int)(sizeof(UnitDesc) / 4); ++i) x[i] = w[i];
    UnitDesc d;
    __builtin_memcpy(&d, x, sizeof d);
    v.node_start = uni((int)d.node_start);
    v.node_size = uni((int)d.node_size);
    v.s0 = uni((int)d.s0);
    v.s1 = uni((int)d.s1);
    v.levels = uni((int)d.levels);
    v.mode = uni((int)d.mode);
    v.src = uni((int)d.src);
    v.dst = uni((int)d.dst);
    v.p = uni((int)d.p);
    v.m = uni((int)d.m);
    v.rows_eval = uni((int)d.rows_eval);
    v.src_off = uni64(d.src_off);
    v.buf_off = uni64(d.buf_off);
    v.snr_row = uni64(d.snr_row);
    v.stdnoise = __int_as_float(uni(__float_as_int(d.stdnoise)));
    v.blob = (uint32_t)uni((int)d.pad);
    v.nruns = uni((int)d.nruns);
    v.entries = uni((int)d.entries);
    v.nb = uni((int)d.nb);
    v.slot_words = uni((int)d.slot_words);
    v.run_off = uni((int)d.run_off);
    v.fill_chunks = uni((int)d.fill_chunks);
    v.zero_row = uni((int)d.zero_row);
    return v;
}

// Per-unit context (wave-uniform) and its LDS metadata: for tile units the
// blob (kBlobHeader words of header, the DMA runs, the descriptor table, the
// bottom-row offsets) DMA'd into `aux`.
constexpr int kAuxWords = kBlobHeader + kDescEntries + kMaxRows + kSlotWords;
static_assert(kAuxWords == kAuxMetaWords, "metadata area");
struct UnitCtx {
    UnitView U;
    bool tile;                // a tile unit (else: a whole node)
    bool table;               // the host-built blob is in aux (every tile unit, most whole units)
    int al;                   // whole units: 16-byte phase (floats) of the block
    bool slots;               // the blob holds row-slot tables (merge_step_slots)
    int nruns, entries, nb;   // blob header counts
    const uint32_t* aux;      // the blob's LDS part in LDS
    const uint32_t* aux0;     // the workgroup's metadata area (roll table at kLut4Off)
    uint4 sv;                 // tile units: this wave's DMA segments (lane i: segment wave + 8i), the
    int mine;                 // same for every trial; `mine` of them
};

__device__ __forceinline__ int rows_at(const UnitCtx& C, int l)
{
    return C.table ? uni((int)C.aux[kHdrRows + l]) : C.U.node_size;
}
__device__ __forceinline__ int desc_offset(const UnitCtx& C, int l) { return uni((int)C.aux[kHdrDesc + l]); }
__device__ __forceinline__ const uint32_t* desc_table(const UnitCtx& C) { return C.aux + kBlobHeader; }
// the row-slot table of the merge step whose output level is lo: its slot
// count, then one word per slot
__device__ __forceinline__ const uint32_t* slot_table(const UnitCtx& C, int lo)
{
    return C.aux + uni((int)C.aux[kHdrSlotOff + lo]);
}
__device__ __forceinline__ const int* bottom_offsets(const UnitCtx& C)
{
    return reinterpret_cast<const int*>(desc_table(C) + C.entries);
}

// Raw buffer resource over `bytes` bytes at p (gfx9 dword3: 32-bit data
// format); out-of-range buffer loads return 0 and stores are dropped.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(uni_ptr(const_cast<void*>(p)), (short)0, uni((int)bytes), 0x00020000);
}

// LDS DMA of `nch` 16-byte chunks from byte offset `goff` of resource rs
// into lds[0 .. 4 nch) (floats), by the waves `wave0 .. W - 1` of the
// workgroup in steps of `wstep` waves: a wave instruction moves 64
// consecutive chunks (destination M0 + 16 lane); lanes past the end are
// exec-masked off and write nothing.
__device__ __forceinline__ void dma_run(__amdgpu_buffer_rsrc_t rs, uint32_t goff, int nch, float* lds, int wave,
                                        int wstep, int lane)
{
    for (int c0 = wave * 64; c0 < nch; c0 += wstep * 64) {
        const int c = c0 + lane;
        if (c < nch)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(lds + 4 * c0), 16,
                                                     (int)(goff + 16u * (uint32_t)c), 0, 0, kFillCpol);
    }
}

// Source block (the transform's rows in the leaf buffer or ping / pong) of a
// unit's bottom level for `trial`, as a buffer resource over the block.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t unit_src(const ConeArgs& a, const UnitView& U, int trial)
{
    const float* src;
    if (U.src == kSelLeaves) src = a.leaves + (uint64_t)trial * a.leaves_stride + U.src_off;
    else src = (U.src == kSelPing ? a.ping : a.pong) + (uint64_t)trial * a.buf_stride + U.buf_off;
    // transform blocks start 16-byte aligned and are padded to 4 floats
    return buffer_rsrc(src, (((uint32_t)U.m * (uint32_t)U.p + 3u) & ~3u) * 4u);
}

// Issues the LDS DMA of a unit's bottom level for `trial` into `buf` (a whole
// unit: one run of 16-byte chunks; a tile unit: the host-built DMA segments,
// one vector load, lane i of wave w holding segment w + 8i) and, with
// `blob_too`, the blob's LDS part (header, descriptors, bottom-row offsets,
// slot tables) into the metadata area.  Nothing is waited for.
template <int SMAX>
__device__ __forceinline__ void unit_fill(const ConeArgs& a, const UnitCtx& C, int trial, float* buf, int tid,
                                          bool blob_too)
{
    const int lane = tid & 63, wave = tid >> 6;
    const UnitView& U = C.U;
    const int p = U.p;
    const __amdgpu_buffer_rsrc_t rs = unit_src(a, U, trial);
    if (!C.table) {
        const int nch = (U.node_size * p + C.al + 3) >> 2;
        dma_run(rs, ((uint32_t)U.node_start * (uint32_t)p - (uint32_t)C.al) * 4u, nch, buf, wave, kConeWaves, lane);
        return;
    }
    const int words = U.run_off;   // the LDS part: header .. slot tables
    // the wave's DMA segments (unit_segments, loaded once per workgroup)
    const uint4 sv = C.sv;
    const int mine = C.mine;
    if (blob_too && wave == kConeWaves - 1) {
        const __amdgpu_buffer_rsrc_t rb = buffer_rsrc(a.blob + U.blob, (uint32_t)words * 4u);
        dma_run(rb, 0u, words >> 2, (float*)const_cast<uint32_t*>(C.aux), 0, 1, lane);
    }
    for (int i = 0; i < mine; ++i) {
        const int c0 = __builtin_amdgcn_readlane((int)sv.x, i);
        const int n = __builtin_amdgcn_readlane((int)sv.y, i);
        const uint32_t g = (uint32_t)__builtin_amdgcn_readlane((int)sv.z, i);
        if (lane < n && 4 * (c0 + n) <= kLdsBufFloats && !(a.flags & kConeDiagNoFill))
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(buf + 4 * c0), 16,
                                                     (int)((g + (uint32_t)lane) * 16u), 0, 0, kFillCpol);
    }
}

// The wave's DMA segments of a tile unit: wave w issues segments w, w + 8,
// ...; its lane i holds segment w + 8i (one coalesced vector load; wave-major
// table, build_tile_blob: the wave's segments are consecutive).  Trial-
// independent: kept in registers for every trial of the workgroup.
__device__ __forceinline__ void unit_segments(const ConeArgs& a, UnitCtx& C, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    const uint4* const segs = reinterpret_cast<const uint4*>(a.blob + C.U.blob + C.U.run_off);
    C.mine = uni(C.nruns > wave ? (C.nruns - wave + kConeWaves - 1) / kConeWaves : 0);
    C.sv = make_uint4(0u, 0u, 0u, 0u);
    const int K = (C.nruns + kConeWaves - 1) / kConeWaves;
    if (lane < C.mine) C.sv = segs[wave * K + lane];
}

// Starts the unit of `item` at trial `trial`: its view (one scalar load of
// its UnitDesc) and, with `dma`, the LDS DMA of its blob into `aux` and of its
// bottom level into `buf` (unit_fill).  Nothing is waited for: the caller
// waits (vmcnt) and barriers before reading LDS.  `ok` = the kernel instance
// can run the unit (the host validates every schedule, validate_exec_plan;
// this guards the error flag): LDS buffer and register rows, the metadata
// area, rows of exactly SMAX slots for SMAX <= 5 (unmasked full slots;
// kPack2: the p <= 32 rows).
template <int SMAX, int RW>
__device__ __forceinline__ UnitCtx unit_begin(const ConeArgs& a, uint32_t item, uint32_t trial, uint32_t* aux,
                                              float* buf, int tid, bool dma, bool& ok, unsigned long long* ts = nullptr)
{
    UnitCtx C;
    C.U = unit_view(a, (int)item, (int)trial);
    const UnitView& U = C.U;
#ifdef RT_STAMPS
    if (ts) ts[0] = __builtin_amdgcn_s_memtime() + (U.p & 0);
#endif
    C.tile = U.mode == kModeTile;
    C.table = U.blob != kNoBlob;
    C.aux = aux;
    C.aux0 = aux;
    const int p = U.p;
    const int slots = merge_slots((uint32_t)p);
    ok = U.levels <= kMaxLevels && p > 0 &&
         ((SMAX <= 5 || SMAX == kPack2) ? slots == SMAX : (slots <= SMAX && slots != kPack2));
    const int cap = min(lds_row_capacity((uint32_t)p, SMAX), kConeWaves * RW * row_pack(SMAX));
    if (!C.table) {
        // short-row units always carry a blob, 4/5-slot units slot tables
        ok = ok && SMAX != kPack2 && (!resolved_slots(SMAX) || U.levels == 0);
        C.al = (int)(((uint32_t)U.node_start * (uint32_t)p) & 3u);
        C.slots = false;
        C.nruns = C.entries = C.nb = 0;
        const int nch = (U.node_size * p + C.al + 3) >> 2;
        ok = ok && !C.tile && U.node_size <= cap && 4 * nch <= kLdsBufFloats;
    } else {
        C.al = 0;
        // the blob's header counts come with the view (UnitDesc); its DMA
        // runs with one vector load -- the unit's DMA is issued two memory
        // round trips after the workgroup starts (a scalar load per run took
        // ~10K cycles for a 16-run tile)
        C.nruns = U.nruns;
        C.entries = U.entries;
        C.nb = U.nb;
        C.slots = U.slot_words != 0;
        const int words = U.run_off;   // the LDS part: header .. slot tables
        if constexpr (SMAX == kPack2) {
            // at the end of the level buffer, above the fill and every level
            // (validate_exec_plan; pack_blob_words)
            C.aux = reinterpret_cast<uint32_t*>(buf + kLdsBufFloats) - words;
            ok = ok && C.nb <= cap && 4 * U.fill_chunks + words <= kLdsBufFloats &&
                 C.nb * pack_stride(p) + words <= kLdsBufFloats;
        } else {
            ok = ok && C.nb <= cap && C.entries <= kDescEntries && words <= kAuxWords;
            // the 4-slot roll table lies past the blob's LDS part
            if (SMAX == 4 && C.slots) ok = ok && words <= kLut4Off;
            // the 4/5-slot instances run row-slot steps only (merge_levels)
            if (resolved_slots(SMAX)) ok = ok && (U.levels == 0 || (C.slots && (a.flags & kConeFuse2)));
            // the zero row of an all-fused whole unit: past its fill, inside the level buffer
            if (U.zero_row)
                ok = ok && resolved_slots(SMAX) && !C.tile && U.zero_row >= 4 * U.fill_chunks &&
                     U.zero_row + 64 * SMAX <= kLdsDataFloats;
        }
        ok = ok && words >= kBlobHeader + C.entries + C.nb && C.nruns <= 64 * kConeWaves && (words & 3) == 0;
    }
#ifdef RT_STAMPS
    if (ts) ts[1] = __builtin_amdgcn_s_memtime() + (ok ? 0 : 0);
#endif
    C.sv = make_uint4(0u, 0u, 0u, 0u);
    C.mine = 0;
    if (ok && dma) {
        if (C.table) unit_segments(a, C, tid);
        unit_fill<SMAX>(a, C, (int)trial, buf, tid, true);
    }
#ifdef RT_STAMPS
    if (ts) ts[2] = __builtin_amdgcn_s_memtime();
#endif
    return C;
}

// x mod p for 0 <= x < 2^22 and p >= 1 (roll shifts: x = s - t(s) < node
// size): a float-reciprocal quotient, off by at most one, then corrected --
// ~8 VALU instead of the ~35 of an integer remainder by a run-time p.
__device__ __forceinline__ int mod_small(int x, int p)
{
    const int q = (int)((float)x * __builtin_amdgcn_rcpf((float)p));
    int r = x - (int)__umul24((unsigned)q, (unsigned)p);
    r = r < 0 ? r + p : r;
    return r >= p ? r - p : r;
}

// Row descriptor (head row, tail row, roll shift) of output row r at level
// l of a whole unit (the node partition of its split tree), as row indices
// of the level below; t = -1 for a carried leaf (size-1 node).
__device__ __forceinline__ void row_desc(int node_size, int l, int r, int p, int& h, int& t, int& sh)
{
    int a0 = 0, sz = node_size;
    for (int d = 0; d < l; ++d) {
        if (sz > 1) {
            const int hs = sz >> 1;
            if (r - a0 < hs) sz = hs;
            else {
                a0 += hs;
                sz -= hs;
            }
        }
    }
    if (sz <= 1) {
        h = r;
        t = -1;
        sh = 0;
    } else {
        const int s = r - a0;
        const uint32_t hs = (uint32_t)sz >> 1, ts = (uint32_t)sz - hs;
        const int hh = (int)merge_index(merge_coef(hs, (uint32_t)sz), (uint32_t)s);
        const int tt = (int)merge_index(merge_coef(ts, (uint32_t)sz), (uint32_t)s);
        h = a0 + hh;
        t = a0 + (int)hs + tt;
        sh = mod_small(s - tt, p);
    }
}

// Packed row descriptor: head row | tail row << 10 | shift << 20 (tail row
// kCarried: a size-1 node carried unchanged).  Rows < 1023, shift < 4096.
constexpr uint32_t kCarried = kCarriedRow;

__device__ __forceinline__ uint32_t pack_desc(int h, int t, int sh)
{
    return (uint32_t)h | ((t < 0 ? kCarried : (uint32_t)t) << 10) | ((uint32_t)sh << 20);
}

// Descriptor of output row r of level l: the tile table, or the node partition.
__device__ __forceinline__ uint32_t unit_desc(const UnitCtx& C, int l, int r, int p)
{
    if (C.table) return desc_table(C)[desc_offset(C, l) + r];
    int h, t, sh;
    row_desc(C.U.node_size, l, r, p, h, t, sh);
    return pack_desc(h, t, sh);
}

}  // namespace rt
