// Signal injection into a filterbank block: the argument checks, the integer
// map from (absolute sample, channel, signal) to a template entry, the dither
// and the sequential specification, and the launch shape of the device form.
// No HIP header: shared by the kernel (inject_kernels.hip), the C ABI
// (capi_inject.cpp, inject_host.cpp) and the sanitizer checker
// (inject_check_main.cpp).
//
// The specification is the "signal injection" section of
// include/riptide_amd.h.  Every integer step is 64-bit two's-complement
// arithmetic that wraps (formed in uint64_t here, so no step is undefined
// behaviour whatever the delays are); the one double product is that of
// resample_host.hpp.  The cast of rint's result is always in range: the
// checks leave |factor| * span < 1 with span >= 1, so |factor| < 1 and
// |factor * q| < 2^63.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>

#include "capi_common.hpp"

namespace rt {

constexpr uint64_t kInjectMaxSpan = RT_RESAMPLE_MAX_SAMPLES;
constexpr uint64_t kInjectMaxChans = RT_INJECT_MAX_CHANS;
constexpr uint64_t kInjectGolden = 0x9E3779B97F4A7C15ull;
constexpr uint32_t kInjectThreads = 256;   // lanes of a workgroup: consecutive dword columns
constexpr uint32_t kInjectLaneSamples = 32;   // samples of one lane: its accumulators

inline bool inject_is_8bit(int dtype) { return dtype == RT_DEDISP_U8 || dtype == RT_DEDISP_I8; }

// the table's own checks: everything that needs no array value
inline void inject_check_table(int dtype, size_t nsamp, size_t nchans, uint64_t t_origin, const rt_inject_spec* specs,
                               size_t nspecs, size_t tmpl_len, size_t amp_len, size_t delay_len)
{
    if (!inject_is_8bit(dtype) && dtype != RT_DEDISP_F32)
        throw std::invalid_argument("inject: the sample type must be uint8, int8 or float32 (packed rows are refused)");
    if (nchans > kInjectMaxChans) throw std::invalid_argument("inject: more than 2^24 channels");
    if (t_origin >= (1ull << 31) || nsamp >= (1ull << 31) || t_origin + nsamp >= (1ull << 31))
        throw std::invalid_argument("inject: t_origin + nsamp must be below 2^31");
    if (nspecs && !specs) throw std::invalid_argument("inject: null signal table");
    auto inside = [](uint64_t off, uint64_t n, size_t len) { return off <= len && n <= len - off; };
    for (size_t k = 0; k < nspecs; ++k) {
        const rt_inject_spec& sp = specs[k];
        uint64_t entries = 0;
        if (sp.kind == 0) {
            if (sp.log2bins < 1 || sp.log2bins > 16) throw std::invalid_argument("inject: log2bins outside [1, 16]");
            entries = 1ull << sp.log2bins;
        } else if (sp.kind == 1) {
            if (!sp.length) throw std::invalid_argument("inject: a pulse template of length 0");
            entries = sp.length;
        } else {
            throw std::invalid_argument("inject: kind must be 0 (periodic) or 1 (single pulse)");
        }
        if (sp.reserved) throw std::invalid_argument("inject: reserved must be 0");
        if (sp.span > kInjectMaxSpan) throw std::invalid_argument("inject: span above 2^27");
        if (!std::isfinite(sp.factor)) throw std::invalid_argument("inject: a factor is not finite");
        if (std::fabs(sp.factor) * (double)sp.span >= 1.0)
            throw std::invalid_argument("inject: |factor| * span must be below 1");
        if (sp.factor != 0.0 && !sp.span) throw std::invalid_argument("inject: a factor needs a span of at least 1");
        if (!inside(sp.tmpl_off, entries, tmpl_len)) throw std::invalid_argument("inject: a template runs past tmpl");
        if (!inside(sp.amp_off, nchans, amp_len)) throw std::invalid_argument("inject: amplitudes run past amp");
        if (!inside(sp.delay_off, nchans, delay_len)) throw std::invalid_argument("inject: delays run past delay");
    }
}

// and the values of the host arrays
inline void inject_check(int dtype, size_t nsamp, size_t nchans, uint64_t t_origin, const rt_inject_spec* specs,
                         size_t nspecs, const float* tmpl, size_t tmpl_len, const float* amp, size_t amp_len,
                         const int32_t* delay, size_t delay_len)
{
    inject_check_table(dtype, nsamp, nchans, t_origin, specs, nspecs, tmpl_len, amp_len, delay_len);
    if (!nspecs) return;
    if (!tmpl || (nchans && (!amp || !delay))) throw std::invalid_argument("inject: null array");
    for (size_t k = 0; k < nspecs; ++k) {
        const rt_inject_spec& sp = specs[k];
        const uint64_t entries = sp.kind == 0 ? 1ull << sp.log2bins : sp.length;
        for (uint64_t i = 0; i < entries; ++i)
            if (!std::isfinite(tmpl[sp.tmpl_off + i])) throw std::invalid_argument("inject: a template value is not finite");
        for (size_t c = 0; c < nchans; ++c)
            if (!std::isfinite(amp[sp.amp_off + c])) throw std::invalid_argument("inject: an amplitude is not finite");
    }
}

// ue of the specification for u = t - delay
inline int64_t inject_time(const rt_inject_spec& sp, int64_t u)
{
    if (sp.factor == 0.0) return u;
    const int64_t q = (int64_t)((uint64_t)u * (sp.span - (uint64_t)u));
    const int64_t s = (int64_t)std::rint(sp.factor * (double)q);
    return (int64_t)((uint64_t)u + (uint64_t)s);
}

// v_k: the float32 product, or 0.0f outside a pulse's window
inline float inject_value(const rt_inject_spec& sp, const float* tmpl, float amp, int64_t ue)
{
    const float* tp = tmpl + sp.tmpl_off;
    if (sp.kind == 0) {
        const uint64_t ph = sp.phase0 + (uint64_t)ue * sp.step;
        return amp * tp[ph >> (64 - sp.log2bins)];
    }
    const uint64_t i = (uint64_t)ue - (uint64_t)sp.t0;
    return i < sp.length ? amp * tp[i] : 0.0f;
}

inline uint64_t inject_mix(uint64_t z)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// the dither of sample (t, c); salt = seed * kInjectGolden
inline float inject_dither(uint64_t t, uint64_t nchans, uint64_t c, uint64_t salt)
{
    return (float)(inject_mix(t * nchans + c + salt) >> 40) * 0x1p-24f;
}

// the integer added to an 8-bit sample
inline int32_t inject_increment(float acc, float r)
{
    return (int32_t)std::floor(std::fmin(std::fmax(acc + r, -65536.0f), 65536.0f));
}

// The specification, sequential, in place.
static inline void inject_host(void* x, int dtype, size_t nsamp, size_t nchans, uint64_t t_origin, uint64_t seed,
                               const rt_inject_spec* specs, size_t nspecs, const float* tmpl, size_t tmpl_len,
                               const float* amp, size_t amp_len, const int32_t* delay, size_t delay_len)
{
    inject_check(dtype, nsamp, nchans, t_origin, specs, nspecs, tmpl, tmpl_len, amp, amp_len, delay, delay_len);
    if (!nspecs || !nsamp || !nchans) return;
    if (!x) throw std::invalid_argument("inject: null block");
    const uint64_t salt = seed * kInjectGolden;
    for (size_t row = 0; row < nsamp; ++row) {
        const int64_t t = (int64_t)(t_origin + row);
        for (size_t c = 0; c < nchans; ++c) {
            float acc = 0.0f;
            for (size_t k = 0; k < nspecs; ++k) {
                const rt_inject_spec& sp = specs[k];
                const int64_t ue = inject_time(sp, t - (int64_t)delay[sp.delay_off + c]);
                const float v = inject_value(sp, tmpl, amp[sp.amp_off + c], ue);
                acc = acc + v;
            }
            const size_t at = row * nchans + c;
            if (dtype == RT_DEDISP_F32) {
                float* p = (float*)x + at;
                *p = *p + acc;
                continue;
            }
            const int32_t d = inject_increment(acc, inject_dither((uint64_t)t, nchans, c, salt));
            if (dtype == RT_DEDISP_U8) {
                uint8_t* p = (uint8_t*)x + at;
                const int32_t y = (int32_t)*p + d;
                *p = (uint8_t)(y < 0 ? 0 : y > 255 ? 255 : y);
            } else {
                int8_t* p = (int8_t*)x + at;
                const int32_t y = (int32_t)*p + d;
                *p = (int8_t)(y < -128 ? -128 : y > 127 ? 127 : y);
            }
        }
    }
}

// ---- the device form
// A lane owns one aligned dword of the block: four consecutive bytes of an
// 8-bit block, one float of a float32 one.  "Super-rows" of spd rows (spd: the
// samples per dword, 4 or 1) are nchans dwords long whatever nchans is, so a
// lane that steps from super-row to super-row keeps its (row within the
// super-row, channel) pairs, and with them its delays and amplitudes.  m is
// the block's misalignment in bytes (8-bit only): the flat byte e = spd * j + b
// - m of dword column j, byte b, is row floor(e / nchans), channel e mod nchans
// of the super-row.
struct InjectShape {
    uint32_t spd = 1;         // samples per dword
    uint32_t m = 0;           // bytes from the aligned address below the block to the block
    uint32_t super_rows = 0;  // of spd rows
    uint32_t lane_rows = 0;   // super-rows a lane walks: kInjectLaneSamples / spd
    uint32_t col_blocks = 0;  // workgroups across the nchans dword columns
    uint64_t blocks = 0;      // col_blocks * ceil(super_rows / lane_rows)
};

inline InjectShape inject_shape(int dtype, size_t nsamp, size_t nchans, uintptr_t address)
{
    InjectShape S;
    S.spd = inject_is_8bit(dtype) ? 4 : 1;
    S.m = S.spd == 4 ? (uint32_t)(address & 3) : 0;
    S.lane_rows = kInjectLaneSamples / S.spd;
    if (!nsamp || !nchans) return S;
    const uint64_t per = (uint64_t)S.spd * nchans;
    S.super_rows = (uint32_t)((S.m + (uint64_t)nsamp * nchans + per - 1) / per);
    S.col_blocks = (uint32_t)((nchans + kInjectThreads - 1) / kInjectThreads);
    S.blocks = (uint64_t)S.col_blocks * ((S.super_rows + S.lane_rows - 1) / S.lane_rows);
    return S;
}

struct InjectArgs {   // the kernel's arguments
    void* x;          // the aligned address at or below the block
    const rt_inject_spec* specs;
    const float* tmpl;
    const float* amp;
    const int32_t* delay;
    uint64_t salt;    // seed * kInjectGolden
    int64_t t_origin;
    uint32_t nspecs, nchans, nsamp, m, super_rows, col_blocks;
};

}  // namespace rt
