// Downsampling ladder of the FFA periodogram for MI355X (gfx950): the per-rung
// kernel and the fused one (every rung from one read of the series).
//
// Exactness: every float operation that the reference performs is performed
// here on the same operands in the same association (explicit *_rn intrinsics
// where hipcc would otherwise contract into FMA), so downsample is
// bit-identical to the strict restatement of downsample.hpp:44-82.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "kernels.hpp"

namespace rt {

template <int N> struct IntC { static constexpr int value = N; };

// ---------------------------------------------------------------------------
// Downsampling ladder (downsample.hpp:44-82; periodogram.hpp:162-168)
// ---------------------------------------------------------------------------
// wmin * w[0] + w[1] + ... + w[cnt - 1], added one by one in that order
// (downsample.hpp:44-82).  The reads go out eight at a time ahead of their
// additions (a plain loop waited for every LDS read in turn: at f ~ 100 the
// ladder was bound by that latency); the elements past cnt - 1 of the last
// group add -0.0, an exact no-op (x + (-0.0) == x).
__device__ __forceinline__ float window_sum(const float* w, float wmin, uint32_t cnt)
{
    float acc = __fmul_rn(wmin, w[0]);
    uint32_t i = 1;
    for (; i + 8 <= cnt; i += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = w[i + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = __fadd_rn(acc, v[j]);
    }
    if (i < cnt) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = i + j < cnt ? w[i + j] : -0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = __fadd_rn(acc, v[j]);
    }
    return acc;
}

// One block = up to 256 consecutive outputs of one rung of one trial (fewer for
// large f, so the block's input span fits the LDS stage).  The span is loaded
// with coalesced loads, then each thread sums its window from LDS in the
// reference's order.  Rungs are flattened along blockIdx.x through a per-rung
// first-block table; blockIdx.y = trial.
__global__ __launch_bounds__(256) void downsample_ladder_kernel(
    const float* __restrict__ x, uint64_t n_in, uint64_t x_stride,
    const DsRung* __restrict__ rungs, uint32_t num_rungs,
    float* __restrict__ out, uint64_t out_stride)
{
    __shared__ float span[kDsSpanFloats];
    uint32_t lo = 0, hi = num_rungs - 1;
    const uint32_t b = blockIdx.x;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (rungs[mid].first_block <= b) lo = mid; else hi = mid - 1;
    }
    const DsRung r = rungs[lo];
    const uint64_t k0 = (uint64_t)(b - r.first_block) * r.per_block;
    const uint64_t k1 = min(k0 + r.per_block, r.n);
    x += (uint64_t)blockIdx.y * x_stride;
    out += (uint64_t)blockIdx.y * out_stride + r.out_off;
    const uint64_t k = k0 + threadIdx.x;
    if (r.identity) {           // f == 1: the rung searches the data at its own resolution
        if (k < k1) out[k] = x[k];
        return;
    }
    const double f = r.f;
    const double last = (double)n_in - 1.0;
    // input span of the block: [imin(k0), imax(k1 - 1)]
    const uint64_t s0 = (uint64_t)floor(__dmul_rn((double)k0, f));
    double e1 = floor(__dadd_rn(__dmul_rn((double)(k1 - 1), f), f));
    if (e1 > last) e1 = last;
    const uint64_t s1 = (uint64_t)e1;
    const float* src = x + s0;
    if (r.staged) {
        const uint32_t len = (uint32_t)(s1 - s0 + 1);
        for (uint32_t i = threadIdx.x; i < len; i += 256) span[i] = x[s0 + i];
        __syncthreads();
        src = span;
    }
    if (k >= k1) return;
    const double start = __dmul_rn((double)k, f);
    const double end = __dadd_rn(start, f);
    const uint64_t imin = (uint64_t)floor(start);
    double dmax = floor(end);
    if (dmax > last) dmax = last;
    const uint64_t imax = (uint64_t)dmax;
    const float wmin = (float)__dsub_rn((double)(imin + 1), start);
    const float wmax = (float)__dsub_rn(end, (double)imax);
    const float* w = src + (imin - s0);
    const uint32_t cnt = (uint32_t)(imax - imin);
    out[k] = __fadd_rn(window_sum(w, wmin, cnt), __fmul_rn(wmax, w[cnt]));
}

// Fused ladder: one block per input span (and trial pair) computes the
// outputs of EVERY rung whose window starts in the span, so the series is
// read from HBM once instead of once per rung (57 rungs at cfg2).  The span
// plus a margin (the plan's: ceil(f) + 2 for its largest fused rung, rounded
// up to 64, <= kDsFusedMargin) is staged in LDS, kDsPairSpan samples in
// all; each output is the same sequential window sum as the per-rung kernel.

// first output k of a rung whose window start floor(k f) is >= s
__device__ __forceinline__ uint64_t ds_first_output(double f, uint64_t s)
{
    uint64_t k = (uint64_t)ceil((double)s / f);
    while (k > 0 && (uint64_t)floor(__dmul_rn((double)(k - 1), f)) >= s) --k;
    while ((uint64_t)floor(__dmul_rn((double)k, f)) < s) ++k;
    return k;
}

// The first output of a rung whose window start floor(k f) is >= s, clipped
// to the rung's length: k_lo of a block's span [s0, s_end) at s = s0, k_hi
// at s = s_end (s_end = n_in for the last block: every remaining output).
__device__ __forceinline__ uint32_t ds_rung_bound(const DsRung& r, uint64_t s, uint64_t n_in)
{
    if (r.identity) return (uint32_t)min(s, r.n);
    return (uint32_t)(s >= n_in ? r.n : min(ds_first_output(r.f, s), r.n));
}

// Every rung's window sums over one staged span.  Indices are 32-bit (the
// planner keeps every series below 2^29 samples), the start / end / floor
// arithmetic is the reference's in float64 (downsample.hpp:53-75: (imin + 1)
// - start is (floor(start) + 1.0) - start exactly, end - imax is end -
// min(floor(end), N - 1)), and each rung's output range in the span is
// computed once per block by one lane per rung instead of by every thread.
//
// The span is staged as overlapping pairs: pair i holds samples s0 + i and
// s0 + i + 1, 8-byte aligned, so a window's consecutive samples from ANY
// start come in ds_read_b64 reads at immediate offsets (2 LDS cycles per 64
// lanes x 2 samples, 64 banks) -- with single samples (ds_read_b32 or the
// compiler's ds_read2_b32, 32 banks) the reads took twice the LDS cycles
// and, the window starts of adjacent outputs lying f apart, conflicted
// alike (tools/ladder_conflicts.py).  Volatile reads: the
// compiler would fuse two of them into ds_read2_b64 (8 cycles).
typedef float ds_pair __attribute__((ext_vector_type(2), aligned(8)));
// A workgroup runs NT = 2 trials of one span: each output's float64 bounds
// (most of the VALU work at f < 12) are computed once for both trials'
// windows.  1024 threads: 2 x 32 KiB of pairs allow two workgroups per CU,
// sixteen waves each (the CU's 32; 512 threads left it half full).
constexpr uint32_t kDsFusedThreads = 1024;
constexpr uint32_t kDsFusedTrials = 2;
static_assert((kDsFusedThreads & (kDsFusedThreads - 1)) == 0 && kDsFusedThreads >= 64, "whole waves, power of two");
static_assert(kDsFusedTrials == 1 || kDsFusedTrials == 2, "trials per workgroup");
// samples staged per trial (pairs): two trials' pairs and the rung table fill
// just under half the CU's 160 KiB, so two workgroups stay resident
// (tests/golden/inputs.py LADDER_SPAN follows this value)
constexpr uint32_t kDsPairSpan = 4864;
static_assert(kDsPairSpan >= 4 * kDsFusedMargin && kDsPairSpan % 64 == 0, "span: whole waves, margin <= a quarter");
static_assert(2 * (kDsFusedTrials * kDsPairSpan * 8 + 8 * kDsMaxRungs) <= 160 * 1024, "two workgroups per CU");
typedef const volatile __attribute__((address_space(3))) ds_pair* ds_pptr;

__global__ __launch_bounds__(kDsFusedThreads) void downsample_fused_kernel(
    const float* __restrict__ x, uint64_t n_in, uint64_t x_stride,
    const DsRung* __restrict__ rungs, uint32_t num_rungs,
    float* __restrict__ out, uint64_t out_stride, uint32_t batch, uint32_t span)
{
    constexpr uint32_t NT = kDsFusedTrials;
    __shared__ ds_pair pairs[NT * kDsPairSpan];
    __shared__ uint32_t kr[2 * kDsMaxRungs];
    const uint64_t s0 = (uint64_t)blockIdx.x * span;
    const uint64_t s_end = min(s0 + (uint64_t)span, n_in);             // window starts owned by this block
    const uint64_t l_end = min(s0 + (uint64_t)kDsPairSpan, n_in);    // staged input
    // trials t0 .. t0 + nt - 1 (a last workgroup of an odd batch stages its
    // one trial twice and stores the same values twice)
    const uint32_t t0 = blockIdx.y * NT;
    const uint32_t nt = min(NT, batch - t0);
    // Only a block staged up to the end of the series can hold windows that
    // min(floor(end), N - 1) clips (otherwise end < s_end + margin <= l_end
    // < N); every other block stages all kDsPairSpan pairs, sample
    // s0 + kDsPairSpan included.  Its loads go out together, ahead of the
    // rung ranges (one lane per rung bound, k_lo and k_hi in two waves:
    // float64 divisions and loops), so the two latencies overlap.
    const bool tail = l_end >= n_in;
    static_assert(2 * kDsMaxRungs <= kDsFusedThreads, "one lane per rung bound");
    const uint32_t r_hi = threadIdx.x / kDsMaxRungs, r_i = threadIdx.x % kDsMaxRungs;
    const bool has_rung = r_hi < 2 && r_i < num_rungs;
    DsRung rr{};
    if (has_rung) rr = rungs[r_i];
    constexpr uint32_t SU = (kDsPairSpan + kDsFusedThreads - 1) / kDsFusedThreads;
    float sa[NT][SU], sb[NT][SU];
    if (!tail) {
#pragma unroll
        for (uint32_t q = 0; q < NT; ++q) {
            const float* xs = x + (uint64_t)(t0 + min(q, nt - 1)) * x_stride + s0 + threadIdx.x;
#pragma unroll
            for (uint32_t u = 0; u < SU; ++u) {
                if (kDsPairSpan % kDsFusedThreads == 0 || threadIdx.x + u * kDsFusedThreads < kDsPairSpan) {
                    sa[q][u] = xs[u * kDsFusedThreads];
                    sb[q][u] = xs[u * kDsFusedThreads + 1];
                }
            }
        }
    }
    if (has_rung) kr[2 * r_i + r_hi] = ds_rung_bound(rr, r_hi ? s_end : s0, n_in);
    if (!tail) {
#pragma unroll
        for (uint32_t q = 0; q < NT; ++q)
#pragma unroll
            for (uint32_t u = 0; u < SU; ++u)
                if (kDsPairSpan % kDsFusedThreads == 0 || threadIdx.x + u * kDsFusedThreads < kDsPairSpan)
                    pairs[q * kDsPairSpan + threadIdx.x + u * kDsFusedThreads] = ds_pair{sa[q][u], sb[q][u]};
    } else {
        for (uint32_t q = 0; q < NT; ++q) {
            const float* xq = x + (uint64_t)(t0 + min(q, nt - 1)) * x_stride;
            for (uint64_t i = s0 + threadIdx.x; i < l_end; i += kDsFusedThreads)
                pairs[q * kDsPairSpan + (i - s0)] = ds_pair{xq[i], i + 1 < n_in ? xq[i + 1] : 0.0f};
        }
    }
    __syncthreads();
    const double last = (double)n_in - 1.0;
    const uint32_t b0 = (uint32_t)s0;
    // lp[s] (+ q kDsPairSpan for trial q): the pair of sample s (pointer
    // arithmetic, so the compiler folds a window's pair offsets, and the
    // second trial's 32 KiB, into the reads' immediate offsets)
    const ds_pptr lp = (ds_pptr)pairs - b0;
    // A non-clipping block has cnt = floor(f) or floor(f) + 1 (floor and
    // rounding are monotone and start + floor(f) is exact), so with F =
    // floor(f) its samples w[1 .. F - 1] all add, w[F] adds when cnt = F + 1
    // (else -0.0, an exact no-op) and w[cnt] is a select of w[F] and w[F + 1]
    // (inside the staged margin: the plan's >= ceil(f) + 2); the clipping
    // block takes the general sum.  The non-clipping bounds come from fract
    // and truncation: (floor(start) + 1) - start is 1 - frac(start) rounded
    // once, as 1.0 - fract(start) is (fract is exact for start >= 0);
    // end - floor(end) is fract(end) exactly (Sterbenz); the uint32
    // truncations are the floors.
    //
    // F < 12 (most of the ladder's outputs: f ~ 1.5-10 at cfg2): one template
    // instance per F, every read at an immediate offset.
    // trial q's rung output (a missing second trial: the first's, whose
    // values it recomputes from the same staged samples -- no branch)
    float* oq[NT];
    // vo: the output's byte offset (32 bits: a rung holds < 2^29 outputs),
    // one offset for both trials' stores (global_store with an SGPR base)
    auto put = [&](uint32_t q, uint32_t vo, float v) { *(float*)((char*)oq[q] + vo) = v; };
    // kd: the output index k as float64 (exact), the window start's operand
    auto output_small = [&](auto ff, double f, double kd, uint32_t vo) {
        constexpr int F = decltype(ff)::value;
        const double start = __dmul_rn(kd, f);
        const double end = __dadd_rn(start, f);
        const uint32_t imin = (uint32_t)start, imax = (uint32_t)end;
        const float wmin = (float)__dsub_rn(1.0, __builtin_amdgcn_fract(start));
        const float wmax = (float)__builtin_amdgcn_fract(end);
        const bool full = imax - imin > (uint32_t)F;
        const ds_pptr w = lp + imin;
        // every read of both trials first (volatile reads issue in program
        // order), then the two independent sums
        float v[NT][F + 3];
#pragma unroll
        for (uint32_t q = 0; q < NT; ++q)
#pragma unroll
            for (int j = 0; j <= F + 1; j += 2) {
                const ds_pair p = w[q * kDsPairSpan + j];
                v[q][j] = p.x;
                v[q][j + 1] = p.y;
            }
#pragma unroll
        for (uint32_t q = 0; q < NT; ++q) {
            float acc = __fmul_rn(wmin, v[q][0]);
#pragma unroll
            for (int j = 1; j < F; ++j) acc = __fadd_rn(acc, v[q][j]);
            acc = __fadd_rn(acc, full ? v[q][F] : -0.0f);
            put(q, vo, __fadd_rn(acc, __fmul_rn(wmax, full ? v[q][F + 1] : v[q][F])));
        }
    };
    // F >= 12: the same sum with uniform trip counts (F is the rung's), four
    // pair reads ahead of their eight additions
    auto output_large = [&](double f, uint32_t F, double kd, uint32_t vo) {
        const double start = __dmul_rn(kd, f);
        const double end = __dadd_rn(start, f);
        const uint32_t imin = (uint32_t)start, imax = (uint32_t)end;
        const float wmin = (float)__dsub_rn(1.0, __builtin_amdgcn_fract(start));
        const float wmax = (float)__builtin_amdgcn_fract(end);
        const bool full = imax - imin > F;
        const ds_pptr w = lp + imin;
        // both trials' sums side by side (independent chains)
        float acc[NT];
#pragma unroll
        for (uint32_t q = 0; q < NT; ++q) {
            const ds_pair p = w[q * kDsPairSpan];
            acc[q] = __fadd_rn(__fmul_rn(wmin, p.x), p.y);
        }
        uint32_t e = 2;
        for (; e + 8 <= F; e += 8) {
            ds_pair g[NT][4];
#pragma unroll
            for (uint32_t q = 0; q < NT; ++q)
#pragma unroll
                for (int i = 0; i < 4; ++i) g[q][i] = w[q * kDsPairSpan + e + 2 * i];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (uint32_t q = 0; q < NT; ++q) acc[q] = __fadd_rn(__fadd_rn(acc[q], g[q][i].x), g[q][i].y);
        }
        for (; e + 2 <= F; e += 2)
#pragma unroll
            for (uint32_t q = 0; q < NT; ++q) {
                const ds_pair p = w[q * kDsPairSpan + e];
                acc[q] = __fadd_rn(__fadd_rn(acc[q], p.x), p.y);
            }
        if (e < F)
#pragma unroll
            for (uint32_t q = 0; q < NT; ++q) acc[q] = __fadd_rn(acc[q], w[q * kDsPairSpan + e].x);
#pragma unroll
        for (uint32_t q = 0; q < NT; ++q) {
            const ds_pair p = w[q * kDsPairSpan + F];
            const float a = __fadd_rn(acc[q], full ? p.x : -0.0f);
            put(q, vo, __fadd_rn(a, __fmul_rn(wmax, full ? p.y : p.x)));
        }
    };
    // the clipping block: the reference's bounds with min(floor(end), N - 1)
    // and the window sum sample by sample
    auto output_tail = [&](double f, double kd, uint32_t vo) {
        const double start = __dmul_rn(kd, f);
        const double end = __dadd_rn(start, f);
        const double fs = floor(start);
        double dmax = floor(end);
        if (dmax > last) dmax = last;
        const uint32_t imin = (uint32_t)fs, imax = (uint32_t)dmax;
        const float wmin = (float)__dsub_rn(__dadd_rn(fs, 1.0), start);
        const float wmax = (float)__dsub_rn(end, dmax);
        for (uint32_t q = 0; q < NT; ++q) {
            const ds_pptr w = lp + q * kDsPairSpan + imin;
            float acc = __fmul_rn(wmin, w[0].x);
            for (uint32_t j = 1; j < imax - imin; ++j) acc = __fadd_rn(acc, w[j].x);
            put(q, vo, __fadd_rn(acc, __fmul_rn(wmax, w[imax - imin].x)));
        }
    };
    // the rung table in lanes: lane l of every wave holds rung c + l's output
    // range and parameters (one LDS read and one global load per 64 rungs),
    // taken per rung with v_readlane -- a per-rung LDS read and scalar load
    // were a memory wait per rung and wave (57 rungs at cfg2)
    const uint32_t lane = threadIdx.x & 63;
    // Work balance: the rungs' outputs tile the waves in turn -- output
    // k_lo + i of a rung goes to thread (rot + i) mod T, rot advancing by
    // each rung's output count rounded up to whole waves -- so the short
    // rungs (f > 7: fewer than T outputs in a span) land on successive waves
    // instead of all on the first ones, and the workgroup's waves finish
    // together (its LDS frees for the next one only when the last does).  A
    // wave's lanes stay consecutive outputs; a wave without outputs in a
    // rung skips it on scalar compares.
    const uint32_t wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
    uint32_t rot = 0;
    for (uint32_t c = 0; c < num_rungs; c += 64) {
        const uint32_t rl = min(c + lane, num_rungs - 1);
        const int my_lo = (int)kr[2 * rl], my_hi = (int)kr[2 * rl + 1];
        const DsRung mr = rungs[rl];
        const long long my_f = __double_as_longlong(mr.f);
        const int my_f_lo = (int)(uint32_t)my_f, my_f_hi = (int)(uint32_t)((uint64_t)my_f >> 32);
        const int my_o_lo = (int)(uint32_t)mr.out_off, my_o_hi = (int)(uint32_t)(mr.out_off >> 32);
        const int my_id = (int)mr.identity;
        const uint32_t nr = min(64u, num_rungs - c);
        for (uint32_t j = 0; j < nr; ++j) {
            const uint32_t k_lo = (uint32_t)__builtin_amdgcn_readlane(my_lo, (int)j);
            const uint32_t k_hi = (uint32_t)__builtin_amdgcn_readlane(my_hi, (int)j);
            const uint32_t nk = k_hi - k_lo;
            const uint32_t wfirst = (wbase - rot) & (kDsFusedThreads - 1);
            const uint32_t i0 = (threadIdx.x - rot) & (kDsFusedThreads - 1);
            rot = (rot + ((nk + 63) & ~63u)) & (kDsFusedThreads - 1);
            if (wfirst >= nk) continue;          // rot: a multiple of 64
            const uint64_t off = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(my_o_lo, (int)j) |
                                 ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(my_o_hi, (int)j) << 32);
#pragma unroll
            for (uint32_t q = 0; q < NT; ++q) oq[q] = out + (uint64_t)(t0 + min(q, nt - 1)) * out_stride + off;
            if (__builtin_amdgcn_readlane(my_id, (int)j)) {
                for (uint32_t k = k_lo + i0; k < k_hi; k += kDsFusedThreads)
#pragma unroll
                    for (uint32_t q = 0; q < NT; ++q) put(q, 4u * k, lp[q * kDsPairSpan + k].x);
                continue;
            }
            const double f = __longlong_as_double(
                (long long)((uint64_t)(uint32_t)__builtin_amdgcn_readlane(my_f_lo, (int)j) |
                            ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(my_f_hi, (int)j) << 32)));
            // this thread's outputs k = k_lo + i0, + T, ... < k_hi of the rung, as
            // (k as float64, byte offset 4 k): the loop runs on those two alone
            auto outputs = [&](auto body) {
                const double kend = (double)k_hi;
                double kd = (double)(k_lo + i0);
                for (uint32_t vo = 4u * (k_lo + i0); kd < kend; kd += (double)kDsFusedThreads, vo += 4u * kDsFusedThreads)
                    body(kd, vo);
            };
            if (tail) {
                outputs([&](double kd, uint32_t vo) { output_tail(f, kd, vo); });
                continue;
            }
            auto rung = [&](auto ff) {
                outputs([&](double kd, uint32_t vo) { output_small(ff, f, kd, vo); });
            };
            const uint32_t F = (uint32_t)f;
            switch (F) {
            case 1: rung(IntC<1>{}); break;
            case 2: rung(IntC<2>{}); break;
            case 3: rung(IntC<3>{}); break;
            case 4: rung(IntC<4>{}); break;
            case 5: rung(IntC<5>{}); break;
            case 6: rung(IntC<6>{}); break;
            case 7: rung(IntC<7>{}); break;
            case 8: rung(IntC<8>{}); break;
            case 9: rung(IntC<9>{}); break;
            case 10: rung(IntC<10>{}); break;
            case 11: rung(IntC<11>{}); break;
            default:
                // F >= 12 (F = 0 does not occur: f > 1 off the identity rung)
                if (F >= 12)
                    outputs([&](double kd, uint32_t vo) { output_large(f, F, kd, vo); });
                else
                    outputs([&](double kd, uint32_t vo) { output_tail(f, kd, vo); });
                break;
            }
        }
    }
}

hipError_t launch_downsample_fused(const float* x, uint64_t n_in, uint64_t x_stride, const DsRung* d_rungs,
                                   uint32_t num_rungs, uint32_t margin, float* out, uint64_t out_stride,
                                   uint32_t batch, hipStream_t s)
{
    if (!num_rungs || !batch || !n_in) return hipSuccess;
    if (margin < 2 || margin > kDsFusedMargin) return hipErrorInvalidValue;
    const uint32_t span = kDsPairSpan - margin;
    const uint64_t blocks = (n_in + span - 1) / span;
    hipLaunchKernelGGL(downsample_fused_kernel, dim3((uint32_t)blocks, (batch + kDsFusedTrials - 1) / kDsFusedTrials),
                       dim3(kDsFusedThreads), 0, s, x, n_in, x_stride, d_rungs, num_rungs, out, out_stride, batch,
                       span);
    return hipGetLastError();
}

hipError_t launch_downsample_ladder(const float* x, uint64_t n_in, uint64_t x_stride,
                                    const DsRung* d_rungs, uint32_t num_rungs, uint32_t total_blocks,
                                    float* out, uint64_t out_stride, uint32_t batch, hipStream_t s)
{
    if (!num_rungs || !total_blocks || !batch) return hipSuccess;
    hipLaunchKernelGGL(downsample_ladder_kernel, dim3(total_blocks, batch), dim3(256), 0, s,
                       x, n_in, x_stride, d_rungs, num_rungs, out, out_stride);
    return hipGetLastError();
}

}  // namespace rt
