// Harmonic pair test shared by the host and the device: riptide's hdiag / htest
// (riptide/pipeline/harmonic_testing.py:9-155) for one pair of clusters, the
// reference's arithmetic operation for operation.  Compiled with
// -ffp-contract=off everywhere, so a * b - c is two roundings on both sides.
//
// F is the postulated fundamental (the brighter cluster), H the postulated
// harmonic.  With slow / fast the two ordered by frequency (equal frequencies:
// slow = F, Python's stable sort):
//
//   x        = fast.freq / slow.freq                        (>= 1)
//   num/den  = Fraction(x).limit_denominator(denom_max)     hfraction()
//   phase    = |num/den * slow.freq - fast.freq| * tobs / fast.ducy
//   dm       = |F.dm - H.dm| * 4.15e3 * band / min(F.ducy/F.freq, H.ducy/H.freq)
//   snr      = |H.snr - F.snr / (num * den) ** 0.5|
//
// and the fraction reported is H.freq / F.freq: den/num when H is the slower.
//
// Ranges (checked by hpair_ok / hparams_ok, RT_EINVAL outside them):
//   1 <= denom_max <= kHDenomMax = 1024,   x < kHRatioMax = 2^40.
// With them q <= 2^10 and p <= x * q + 1 <= 2^50 + 1 for every convergent and
// semi-convergent p/q, so: a * q1 <= 2^52 * 2^10 and q0 + a * q1 < 2^63; p0 +
// a * p1 is formed only when a <= denom_max, below 2^61; the final comparison
// 2 * d * qb < 2 * 2^52 * 2^10 = 2^63; num * den <= 2^61 in int64; num and den
// are below 2^53, so double(num) / double(den) is the correctly rounded
// quotient that float(Fraction) is.  No 128-bit arithmetic is needed.
//
// The square root is the one operation that differs by side.  Python's
// int ** 0.5 is libm pow(double(n), 0.5), which is not sqrt(n) for about one
// integer in a thousand; the host build calls that same pow, the device uses
// sqrt (at most 1 ulp from the true root, as is pow).  See hguard().
#pragma once
#include <cmath>
#include <cstdint>

#include "common.hpp"

namespace rt {

constexpr uint32_t kHDenomMax = 1024;
constexpr double kHRatioMax = 1099511627776.0;   // 2^40
constexpr double kHTwo52 = 4503599627370496.0;   // 2^52

struct HCand {
    double freq, snr, ducy, dm;
};

// rt_htest_params, by another name (capi_harmonic.cpp asserts the layout)
struct HParams {
    double tobs, band, phase_distance_max, dm_distance_max, snr_distance_max;
    uint32_t denom_max;
};

struct HDiag {
    int64_t num, den;   // H.freq / F.freq
    double phase_distance, dm_distance, snr_distance;
};

RT_HD inline bool hcand_ok(const HCand& c)
{
    // finite and positive (a NaN fails both comparisons)
    return c.freq > 0.0 && c.freq < INFINITY && c.ducy > 0.0 && c.ducy < INFINITY;
}

RT_HD inline bool hparams_ok(const HParams& p)
{
    return p.tobs > 0.0 && p.denom_max >= 1 && p.denom_max <= kHDenomMax;
}

// Fraction(x).limit_denominator(dmax) for a double 1 <= x < 2^40.
//
// x = I + fr / 2^52 exactly, I = floor(x) and fr = (x - I) * 2^52 both exact
// in fp64.  Fraction(x) in lowest terms has denominator 2^(52 - tz(fr)) (1 when
// fr == 0); when that is <= dmax the fraction itself is returned, as
// limit_denominator does (the recurrence below would reach a zero remainder).
//
// Otherwise the continued fraction of x.  limit_denominator starts from
// (p0, q0, p1, q1) = (0, 1, 1, 0) and n/d = x; its first step has a = I and
// q2 = 1 <= dmax, leaving (1, 0, I, 1) and n/d = 2^52 / fr, which is where the
// loop below starts, in uint64.  Not reducing n/d by 2^tz(fr) scales every
// remainder by that factor and changes no quotient.
//
// The last step picks between bound2 = p1/q1 and bound1 = (p0 + k p1)/(q0 + k q1)
// by |bound2 - x| <= |bound1 - x|.  x lies between the two, which are
// 1 / (q1 qb) apart (qb = q0 + k q1), and |x - p1/q1| = d / (q1 D) with D the
// denominator of x in the scaling of the remainders (q1 n + q0 d == D is the
// recurrence's invariant; here D = 2^52).  So bound2 wins, ties included,
// exactly when 2 d qb <= 2^52.
RT_HD inline void hfraction(double x, uint32_t dmax, uint64_t& num, uint64_t& den)
{
    const double fl = floor(x);
    const uint64_t I = (uint64_t)fl;
    const uint64_t fr = (uint64_t)((x - fl) * kHTwo52);
    if (fr == 0) {
        num = I;
        den = 1;
        return;
    }
    const int tz = __builtin_ctzll(fr);
    const uint64_t exact_den = 1ull << (52 - tz);
    if (exact_den <= dmax) {
        num = I * exact_den + (fr >> tz);
        den = exact_den;
        return;
    }
    uint64_t p0 = 1, q0 = 0, p1 = I, q1 = 1;
    uint64_t n = 1ull << 52, d = fr;
    for (;;) {   // ends before d reaches 0: the last convergent's denominator is exact_den > dmax
        const uint64_t a = n / d;
        const uint64_t q2 = q0 + a * q1;
        if (q2 > dmax) break;
        const uint64_t p2 = p0 + a * p1;
        p0 = p1;
        q0 = q1;
        p1 = p2;
        q1 = q2;
        const uint64_t r = n - a * d;
        n = d;
        d = r;
    }
    const uint64_t k = (dmax - q0) / q1;
    const uint64_t qb = q0 + k * q1;
    if (2 * d * qb <= (1ull << 52)) {
        num = p1;
        den = q1;
    } else {
        num = p0 + k * p1;
        den = qb;
    }
}

// x = fast.freq / slow.freq of a valid pair, inside the range of hfraction
RT_HD inline bool hpair_ok(const HCand& F, const HCand& H)
{
    if (!hcand_ok(F) || !hcand_ok(H)) return false;
    const double x = H.freq < F.freq ? F.freq / H.freq : H.freq / F.freq;
    return x < kHRatioMax;
}

RT_HD inline double hdm_distance(const HCand& F, const HCand& H, const HParams& P)
{
    const double wf = F.ducy / F.freq, wh = H.ducy / H.freq;
    const double delay = fabs(F.dm - H.dm) * 4.15e3 * P.band;
    return delay / (wh < wf ? wh : wf);   // Python's min(wf, wh)
}

// The fraction fast.freq / slow.freq (not yet inverted) and the phase distance.
RT_HD inline double hphase_distance(const HCand& F, const HCand& H, const HParams& P, uint64_t& num, uint64_t& den)
{
    const bool h_slow = H.freq < F.freq;
    const HCand& slow = h_slow ? H : F;
    const HCand& fast = h_slow ? F : H;
    hfraction(fast.freq / slow.freq, P.denom_max, num, den);
    const double ratio = (double)num / (double)den;
    return fabs(ratio * slow.freq - fast.freq) * P.tobs / fast.ducy;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// pow with an exponent the compiler cannot see: clang folds pow(x, 0.5) of a
// value known to be finite into sqrt(x), which is not CPython's result
inline double hroot_host(double v)
{
    static const volatile double half = 0.5;
    return std::pow(v, half);
}
#endif

RT_HD inline double hsnr_distance(const HCand& F, const HCand& H, uint64_t num, uint64_t den)
{
    const double v = (double)(int64_t)(num * den);
#if defined(__HIP_DEVICE_COMPILE__)
    const double root = sqrt(v);
#else
    const double root = hroot_host(v);
#endif
    return fabs(H.snr - F.snr / root);
}

// How far the device's snr_distance can be from the host's.  The two roots
// are each within 1 ulp of the true one, so within 2 ulp of each other; the
// quotient F.snr / root rounds once more on each side: the two expected S/N
// differ by at most 3 ulp of a value <= |F.snr| (num * den >= 1).  The
// subtraction rounds once on each side, within 1 ulp in total of a result
// <= |H.snr| + |F.snr| <= 2 max.  That is 5 * 2^-52 * max(|F.snr|, |H.snr|);
// the band is 8 of them.  A pair whose device snr_distance is farther than
// the band from snr_distance_max falls on the same side on the host.
RT_HD inline double hguard(const HCand& F, const HCand& H)
{
    const double a = fabs(F.snr), b = fabs(H.snr);
    return 8.0 * 2.220446049250313e-16 * (a > b ? a : b);
}

RT_HD inline HDiag hdiag_pair(const HCand& F, const HCand& H, const HParams& P)
{
    HDiag r;
    uint64_t num, den;
    r.phase_distance = hphase_distance(F, H, P, num, den);
    r.dm_distance = hdm_distance(F, H, P);
    r.snr_distance = hsnr_distance(F, H, num, den);
    const bool h_slow = H.freq < F.freq;
    r.num = (int64_t)(h_slow ? den : num);
    r.den = (int64_t)(h_slow ? num : den);
    return r;
}

// htest's verdict.  *near (device callers): the two other tests pass and the
// S/N distance is within hguard() of its bound, so the host decides the pair.
RT_HD inline bool htest_pair(const HCand& F, const HCand& H, const HParams& P, bool* near)
{
    if (near) *near = false;
    if (!(hdm_distance(F, H, P) <= P.dm_distance_max)) return false;
    uint64_t num, den;
    if (!(hphase_distance(F, H, P, num, den) <= P.phase_distance_max)) return false;
    const double s = hsnr_distance(F, H, num, den);
    if (near) *near = fabs(s - P.snr_distance_max) <= hguard(F, H);
    return s <= P.snr_distance_max;
}

}  // namespace rt
