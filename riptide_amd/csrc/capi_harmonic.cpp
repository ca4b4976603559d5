// C ABI, harmonic flagging (harmonic.hpp, harmonic_kernels.hip): the pair
// diagnostics on the host and on the device, and the tiled pair matrix whose
// tiles harmonic_host.hpp resolves.
#include "riptide_amd.h"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>

#include "capi_device.hpp"
#include "harmonic_host.hpp"
#include "kernels.hpp"

using namespace rt;

namespace {

static_assert(sizeof(HParams) == sizeof(rt_htest_params) && offsetof(HParams, denom_max) == offsetof(rt_htest_params, denom_max),
              "HParams is rt_htest_params");
static_assert(sizeof(HNearPair) == sizeof(uint2), "HNearPair is the device's uint2");

// A tile of the pair matrix is at most kHTileWords 64-bit words (4 MiB)
// whatever n is: rows-per-tile = kHTileWords / ceil(n / 64), at least 1 since
// n <= kHMaxClusters.  Two tiles are in flight (one computing, one being
// resolved), each with a near list of kHNearCap pairs and a 16-byte header
// (harmonic_host.hpp).
constexpr size_t kHTileWords = (size_t)1 << 19;
constexpr size_t kHMaxClusters = (size_t)1 << 24;
constexpr size_t kHDefaultRows = 1024;
static_assert(kHMaxClusters / 64 <= kHTileWords, "one row fits a tile");

struct HStats {
    uint64_t tiles = 0, near_pairs = 0, host_rows = 0;
    double kernel_ms = 0;
};
thread_local HStats g_hstats;

HParams hparams_checked(const rt_htest_params* p)
{
    if (!p) throw std::invalid_argument("harmonics: null params");
    HParams P;
    std::memcpy(&P, p, sizeof P);
    if (!(P.tobs > 0.0)) throw std::invalid_argument("harmonics: tobs must be > 0");
    if (!hparams_ok(P)) throw std::invalid_argument("harmonics: denom_max must be in [1, 1024]");
    return P;
}

void hcheck_pairs(const HInputs& in, size_t n, const int32_t* pi, const int32_t* pj, size_t npairs)
{
    for (size_t k = 0; k < npairs; ++k) {
        if (pi[k] < 0 || pj[k] < 0 || (size_t)pi[k] >= n || (size_t)pj[k] >= n)
            throw std::invalid_argument("harmonics: pair index out of range");
        if (!hpair_ok(in.at(pi[k]), in.at(pj[k])))
            throw std::invalid_argument(
                "harmonics: freq and ducy must be finite and positive, the frequency ratio below 2^40");
    }
}

// What rt_hdiag_host and rt_hdiag_pairs check alike (outputs: none of the
// five result arrays is null), then run(in, P) on the checked inputs (not
// called for an empty pair list).
template <class F>
int hdiag_call(const double* freq, const double* snr, const double* ducy, const double* dm, size_t n,
               const int32_t* pi, const int32_t* pj, size_t npairs, const rt_htest_params* params, bool outputs,
               F&& run)
{
    return guarded([&] {
        const HParams P = hparams_checked(params);
        if (!npairs) return RT_OK;
        if (!freq || !snr || !ducy || !dm || !pi || !pj || !outputs)
            throw std::invalid_argument("harmonics: null buffer");
        const HInputs in{freq, snr, ducy, dm};
        hcheck_pairs(in, n, pi, pj, npairs);
        run(in, P);
        return RT_OK;
    });
}

// pinned staging of the two tiles in flight and their events, per device;
// grow-only, kept for the rest of the process (guarded by g_mu)
struct HSlot {
    char* h = nullptr;
    hipEvent_t done = nullptr, k0 = nullptr, k1 = nullptr;
};
struct HStage {
    size_t bytes = 0;
    HSlot slot[2];
};
std::map<int, HStage> g_hstage;

HStage& harmonic_stage(int device, size_t bytes)
{
    HStage& st = g_hstage[device];
    for (HSlot& s : st.slot) {
        if (!s.done) {
            ck(hipEventCreateWithFlags(&s.done, hipEventDisableTiming), "hipEventCreate");
            ck(hipEventCreate(&s.k0), "hipEventCreate");
            ck(hipEventCreate(&s.k1), "hipEventCreate");
        }
    }
    if (bytes > st.bytes) {
        for (HSlot& s : st.slot) {
            if (s.h) (void)hipHostFree(s.h);
            s.h = nullptr;
        }
        st.bytes = 0;
        for (HSlot& s : st.slot) ck(hipHostMalloc((void**)&s.h, bytes, hipHostMallocDefault), "hipHostMalloc");
        st.bytes = bytes;
    }
    return st;
}

// The tile pipeline: tile t + 1 is computed and copied back while the host
// resolves tile t (hresolve_tile), in rank order.
void flag_harmonics(const HInputs& in, size_t n, const HParams& P, size_t block_rows, int32_t* parent, int64_t* hnum,
                    int64_t* hden)
{
    const size_t wpr = (n + 63) / 64;
    const size_t rows_cap = std::max<size_t>(1, kHTileWords / wpr);
    const size_t rows = std::min(block_rows ? block_rows : kHDefaultRows, rows_cap);
    const size_t nrows = n - 1;   // the last cluster has no pair to its right
    const size_t ntiles = (nrows + rows - 1) / rows;
    const size_t slot_bytes = kHWordsOff + std::min(rows, nrows) * wpr * sizeof(uint64_t);

    std::lock_guard<std::mutex> lk(g_mu);
    Context& c = context();
    double* din = dev<double>(c, 0, 4 * n);
    const double* src[4] = {in.freq, in.snr, in.ducy, in.dm};
    for (int a = 0; a < 4; ++a) h2d(din + a * n, src[a], n * sizeof(double), c.stream);
    char* dslot[2] = {(char*)c.buf[1].get(slot_bytes), (char*)c.buf[2].get(slot_bytes)};
    HStage& st = harmonic_stage(c.device, slot_bytes);

    auto issue = [&](size_t t) {
        HSlot& s = st.slot[t & 1];
        char* d = dslot[t & 1];
        const size_t i0 = t * rows, r = std::min(rows, nrows - i0);
        ck(hipMemsetAsync(d, 0, kHHeaderBytes, c.stream), "hipMemsetAsync");
        ck(hipEventRecord(s.k0, c.stream), "hipEventRecord");
        ck(launch_harmonic_pairs(din, din + n, din + 2 * n, din + 3 * n, (uint32_t)n, (uint32_t)i0, (uint32_t)r,
                                 (uint32_t)wpr, P, (uint64_t*)(d + kHWordsOff), (uint2*)(d + kHHeaderBytes), kHNearCap,
                                 (uint32_t*)d, c.stream),
           "harmonic_pairs");
        ck(hipEventRecord(s.k1, c.stream), "hipEventRecord");
        d2h(s.h, d, kHWordsOff + r * wpr * sizeof(uint64_t), c.stream);
        ck(hipEventRecord(s.done, c.stream), "hipEventRecord");
    };

    try {
        issue(0);
        for (size_t t = 0; t < ntiles; ++t) {
            if (t + 1 < ntiles) issue(t + 1);   // its slot held tile t - 1, resolved already
            HSlot& s = st.slot[t & 1];
            ck(hipEventSynchronize(s.done), "hipEventSynchronize");
            float ms = 0;
            ck(hipEventElapsedTime(&ms, s.k0, s.k1), "hipEventElapsedTime");
            g_hstats.kernel_ms += ms;
            g_hstats.tiles++;

            const size_t i0 = t * rows, r = std::min(rows, nrows - i0);
            const HTileCounts tc =
                hresolve_tile(*(const uint32_t*)s.h, (const HNearPair*)(s.h + kHHeaderBytes),
                              (uint64_t*)(s.h + kHWordsOff), i0, r, wpr, n, in, P, parent, hnum, hden);
            g_hstats.near_pairs += tc.near_pairs;
            g_hstats.host_rows += tc.host_rows;
        }
    } catch (...) {
        (void)hipStreamSynchronize(c.stream);   // nothing of this call stays in flight
        throw;
    }
}

}  // namespace

extern "C" {

int rt_hdiag_host(const double* freq, const double* snr, const double* ducy, const double* dm, size_t n,
                  const int32_t* pi, const int32_t* pj, size_t npairs, const rt_htest_params* params, int64_t* num,
                  int64_t* den, double* phase_distance, double* dm_distance, double* snr_distance)
{
    auto run = [&](const HInputs& in, const HParams& P) {
        for (size_t k = 0; k < npairs; ++k) {
            const HDiag d = hdiag_pair(in.at(pi[k]), in.at(pj[k]), P);
            num[k] = d.num;
            den[k] = d.den;
            phase_distance[k] = d.phase_distance;
            dm_distance[k] = d.dm_distance;
            snr_distance[k] = d.snr_distance;
        }
    };
    return hdiag_call(freq, snr, ducy, dm, n, pi, pj, npairs, params,
                      num && den && phase_distance && dm_distance && snr_distance, run);
}

int rt_hdiag_pairs(const double* freq, const double* snr, const double* ducy, const double* dm, size_t n,
                   const int32_t* pi, const int32_t* pj, size_t npairs, const rt_htest_params* params, int64_t* num,
                   int64_t* den, double* phase_distance, double* dm_distance, double* snr_distance)
{
    auto run = [&](const HInputs&, const HParams& P) {
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        double* din = dev<double>(c, 0, 4 * n);
        int32_t* dp = dev<int32_t>(c, 1, 2 * npairs);
        int64_t* dout = dev<int64_t>(c, 2, 5 * npairs);   // num, den, then the three distances (8 bytes each)
        double* dd = (double*)(dout + 2 * npairs);
        const double* src[4] = {freq, snr, ducy, dm};
        for (int a = 0; a < 4; ++a) h2d(din + a * n, src[a], n * sizeof(double), c.stream);
        h2d(dp, pi, npairs * sizeof(int32_t), c.stream);
        h2d(dp + npairs, pj, npairs * sizeof(int32_t), c.stream);
        ck(launch_harmonic_diag(din, din + n, din + 2 * n, din + 3 * n, dp, dp + npairs, npairs, P, dout, dout + npairs,
                                dd, dd + npairs, dd + 2 * npairs, c.stream),
           "harmonic_diag");
        d2h(num, dout, npairs * 8, c.stream);
        d2h(den, dout + npairs, npairs * 8, c.stream);
        d2h(phase_distance, dd, npairs * 8, c.stream);
        d2h(dm_distance, dd + npairs, npairs * 8, c.stream);
        d2h(snr_distance, dd + 2 * npairs, npairs * 8, c.stream);
        sync(c.stream);
    };
    return hdiag_call(freq, snr, ducy, dm, n, pi, pj, npairs, params,
                      num && den && phase_distance && dm_distance && snr_distance, run);
}

int rt_flag_harmonics(const double* freq, const double* snr, const double* ducy, const double* dm, size_t n,
                      const rt_htest_params* params, size_t block_rows, int32_t* parent, int64_t* hnum, int64_t* hden)
{
    return guarded([&] {
        g_hstats = HStats();
        if (n && (!parent || !hnum || !hden)) throw std::invalid_argument("harmonics: null buffer");
        for (size_t i = 0; i < n; ++i) {
            parent[i] = -1;
            hnum[i] = hden[i] = 0;
        }
        if (n <= 1) return RT_OK;
        if (!freq || !snr || !ducy || !dm) throw std::invalid_argument("harmonics: null buffer");
        const HParams P = hparams_checked(params);
        if (n > kHMaxClusters) throw std::invalid_argument("harmonics: more than 2^24 clusters");
        const HInputs in{freq, snr, ducy, dm};
        double lo = freq[0], hi = freq[0];
        for (size_t i = 0; i < n; ++i) {
            if (!hcand_ok(in.at(i))) throw std::invalid_argument("harmonics: freq and ducy must be finite and positive");
            lo = std::min(lo, freq[i]);
            hi = std::max(hi, freq[i]);
        }
        // IEEE division is monotonic: every pair's ratio is at most hi / lo
        if (!(hi / lo < kHRatioMax)) throw std::invalid_argument("harmonics: frequency ratios must be below 2^40");
        flag_harmonics(in, n, P, block_rows, parent, hnum, hden);
        return RT_OK;
    });
}

int rt_flag_harmonics_stats(uint64_t* tiles, uint64_t* near_pairs, uint64_t* host_rows, double* kernel_ms)
{
    if (tiles) *tiles = g_hstats.tiles;
    if (near_pairs) *near_pairs = g_hstats.near_pairs;
    if (host_rows) *host_rows = g_hstats.host_rows;
    if (kernel_ms) *kernel_ms = g_hstats.kernel_ms;
    return RT_OK;
}

}  // extern "C"
