// Host-only checker of the planning that the C ABI's device files rely on,
// built with AddressSanitizer + UBSan by `make -C riptide_amd/csrc asan`:
//   fold      fold_plan / fold_check_ranges / rt_fold_workspace_bytes (fold_host.hpp)
//   dered     dered_geom / dered_ws_layout / dered_ws_bytes / dered_forms and
//             rt_deredden_forms (dered_host.hpp)
//   harmonic  hresolve_tile (harmonic_host.hpp)
// Every array is a heap block of exactly the size the code may touch.  No
// device call, and none linked.  Usage: host_check [fold|dered|harmonic]
// (no argument: all three).  Exit status 0 iff every check holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "dered_host.hpp"
#include "fold_host.hpp"
#include "harmonic_host.hpp"
#include "riptide_amd.h"

using namespace rt;

namespace {

int fails = 0;
void expect(bool ok, const std::string& what)
{
    if (!ok) {
        std::printf("FAILED: %s\n", what.c_str());
        ++fails;
    }
}

// ---- fold
struct Spec {
    double factor;
    uint32_t bins, subints, series;
    uint64_t out_off;
};
std::unique_ptr<rt_fold_spec[]> table(const std::vector<Spec>& v)   // exact size
{
    std::unique_ptr<rt_fold_spec[]> t(new rt_fold_spec[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) t[i] = rt_fold_spec{v[i].factor, v[i].out_off, v[i].series, v[i].bins, v[i].subints, 0};
    return t;
}

// "" if the table plans and its ranges check, else the error text
std::string fold_try(size_t size, const std::vector<Spec>& v, size_t nseries, size_t out_floats, FoldPlan* plan = nullptr)
{
    const auto t = table(v);
    try {
        const FoldPlan P = fold_plan(size, t.get(), v.size());
        fold_check_ranges(P, t.get(), nseries, out_floats);
        if (plan) *plan = P;
    } catch (const std::invalid_argument& e) {
        return e.what();
    }
    return "";
}

// every candidate's rows and result lie inside the workspace and the output
void fold_inside(const char* name, size_t size, const std::vector<Spec>& v, size_t out_floats)
{
    FoldPlan P;
    expect(fold_try(size, v, 2, out_floats, &P).empty(), std::string(name) + ": accepted");
    size_t ws = 0;
    const auto t = table(v);
    expect(rt_fold_workspace_bytes(size, t.get(), v.size(), &ws) == RT_OK && ws == P.ws_bytes, std::string(name) + ": ws");
    expect((P.rows.size() + P.sub.size()) * sizeof(FoldCand) <= P.table_bytes, std::string(name) + ": tables");
    uint64_t blocks = 0, ws_end = 0;
    for (const FoldCand& c : P.rows) {
        expect(c.first_block == blocks, std::string(name) + ": first_block");
        blocks += (c.n_rows_out + c.per_block - 1) / c.per_block;
        expect(c.out_off + fold_result_floats(c) <= out_floats, std::string(name) + ": result inside the output");
        if (c.rows_in_ws) {
            expect(c.rows_off == ws_end, std::string(name) + ": workspace rows follow each other");
            ws_end = c.rows_off + c.n_rows_out;
            expect(P.table_bytes + ws_end * sizeof(float) <= ws, std::string(name) + ": rows inside the workspace");
        } else {
            expect(c.rows_off + c.n_rows_out <= out_floats, std::string(name) + ": rows inside the output");
        }
    }
    expect(blocks == P.rows_blocks, std::string(name) + ": rows_blocks");
    blocks = 0;
    for (const FoldCand& c : P.sub) {
        expect(c.first_block == blocks && c.rows_in_ws, std::string(name) + ": subints table");
        blocks += ((uint64_t)c.sub_rows * c.bins + 255) / 256;
    }
    expect(blocks == P.sub_blocks, std::string(name) + ": sub_blocks");
}

void check_fold()
{
    const size_t SIZE = 4096;
    const Spec GOOD{4.0, 16, 0, 0, 0};   // m = 64, rows result: 1024 floats
    auto with = [&](double f, uint32_t bins, uint32_t subints, uint32_t series, uint64_t off) {
        return Spec{f, bins, subints, series, off};
    };
    // the accept cases of tests/test_fold_host.py
    fold_inside("two specs", SIZE, {with(4.0, 16, 4, 0, 0), with(4.0, 16, 0, 0, 64)}, 64 + 1024);
    size_t ws = 1;
    expect(rt_fold_workspace_bytes(SIZE, nullptr, 0, &ws) == RT_OK && ws == 0, "no specs");
    // its EINVAL_CASES: specs, nseries, out_floats, and whether the plan itself is refused
    struct Bad {
        const char* name;
        std::vector<Spec> v;
        size_t nseries, out_floats;
        bool plan;
    };
    const size_t big = (size_t)1 << 20;
    const Bad bad[] = {
        {"factor_one", {with(1.0, 16, 0, 0, 0)}, 1, big, true},
        {"factor_below_one", {with(0.5, 16, 0, 0, 0)}, 1, big, true},
        {"factor_above_size", {with(SIZE + 0.5, 16, 0, 0, 0)}, 1, big, true},
        {"factor_nan", {with(std::nan(""), 16, 0, 0, 0)}, 1, big, true},
        {"bins_one", {with(4.0, 1, 0, 0, 0)}, 1, big, true},
        {"bins_zero", {with(4.0, 0, 0, 0, 0)}, 1, big, true},
        {"no_whole_period", {with(400.0, 16, 0, 0, 0)}, 1, big, true},
        {"subints_above_m", {with(4.0, 16, 65, 0, 0)}, 1, big, true},
        {"series_out_of_range", {with(4.0, 16, 0, 2, 0)}, 2, big, false},
        {"output_past_end", {with(4.0, 16, 0, 0, 1)}, 1, 1024, false},
        {"output_offset_past_end", {with(4.0, 16, 1, 0, (uint64_t)1 << 40)}, 1, 1024, false},
        {"outputs_overlap", {GOOD, with(4.0, 16, 1, 0, 1023)}, 1, big, false},
        {"second_spec_bad", {GOOD, with(4.0, 1, 0, 0, 1024)}, 1, big, true},
    };
    for (const Bad& b : bad) {
        expect(!fold_try(SIZE, b.v, b.nseries, b.out_floats).empty(), std::string(b.name) + ": refused");
        const auto t = table(b.v);
        expect(rt_fold_workspace_bytes(SIZE, t.get(), b.v.size(), &ws) == (b.plan ? RT_EINVAL : RT_OK),
               std::string(b.name) + ": rt_fold_workspace_bytes");
    }
    // the three modes, with staged (f = 4, 1.7) and unstaged (f = 200) factors, two series
    const size_t N = 65536;
    std::vector<Spec> mix;
    uint64_t off = 0;
    const double fs[] = {4.0, 200.0, 1.7};
    const uint32_t subs[] = {0, 1, 7};
    for (double f : fs)
        for (uint32_t sub : subs) {
            const uint32_t bins = f == 1.7 ? 13 : 16;
            size_t m = 0, rows = 0;
            expect(rt_fold_shape(N, f, bins, sub, &m, &rows) == RT_OK, "mixed: shape");
            mix.push_back(with(f, bins, sub, f == 1.7, off));
            off += (rows ? rows : 1) * bins;
        }
    expect(ds_per_block(4.0) >= 32 && ds_per_block(200.0) < 32, "mixed: staged and unstaged factors");
    fold_inside("mixed", N, mix, off);
    expect(!fold_try(N, mix, 2, off - 1).empty(), "mixed: output one float short");
}

// ---- dered
// rt_deredden_forms against the predicates it is built from, each record a
// heap block of exact size: over scrunch factors on both sides of every
// switch, both alignments of either buffer, strides that keep and break the
// 16-byte rows, and the three stage selections.
void check_dered_forms()
{
    const size_t factors[] = {1, 2, 4, 128, 129, 248, 249, 255, 256, 257, 773, 8192, 8193, 16385};
    const size_t minpts[] = {1, 3, 255, 257};
    size_t seen_scrunch[4] = {0, 0, 0, 0}, seen_sub[4] = {0, 0, 0, 0}, fused = 0, two_pass = 0, calls = 0;
    for (size_t sf : factors)
        for (size_t mp : minpts)
            for (size_t n_lo : {mp + 1, mp + 70})
                for (size_t tail : {(size_t)0, sf - 1})
                    for (unsigned ia : {0u, 4u})
                        for (unsigned oa : {0u, 12u})
                            for (size_t pad : {(size_t)0, (size_t)1, (size_t)4})
                                for (int mode = 1; mode < 4; ++mode) {
                                    const size_t n = n_lo * sf + tail, ws = sf * mp;
                                    const bool dered = mode & 1, norm = mode & 2;
                                    const bool in16 = ia == 0 && (n + pad) % 4 == 0, out16 = oa == 0 && (n + 2 * pad) % 4 == 0;
                                    std::unique_ptr<rt_dered_forms> f(new rt_dered_forms);
                                    std::memset(f.get(), 0xff, sizeof(rt_dered_forms));
                                    const int rc = rt_deredden_forms(n, ws, mp, dered, norm, ia, oa, n + pad, n + 2 * pad,
                                                                     f.get());
                                    expect(rc == RT_OK, "dered forms: accepted");
                                    if (rc != RT_OK) continue;
                                    ++calls;
                                    const DeredGeom g = dered_geom(n, ws, mp, 1, dered);
                                    expect(f->scrunch_factor == g.sf && f->n_lo == g.n_lo && f->rmed_width == g.rmed_w,
                                           "dered forms: geometry");
                                    expect(f->scrunch <= RT_SCRUNCH_GENERAL && f->subtract <= RT_SUBTRACT_SLOPE4 &&
                                               f->rmed <= RT_RMED_LARGE && f->fused <= 1 && f->norm_partial <= RT_NORM_VEC &&
                                               f->norm_apply <= RT_NORM_VEC && f->norm_passes <= 2,
                                           "dered forms: values in range");
                                    ++seen_scrunch[f->scrunch];
                                    ++seen_sub[f->subtract];
                                    fused += f->fused;
                                    two_pass += f->norm_passes == 2;
                                    if (!dered) {
                                        expect(!f->scrunch && !f->rmed && !f->subtract && !f->fused && f->scrunch_factor == 1,
                                               "dered forms: no dereddening stage");
                                    } else {
                                        expect((f->scrunch == 0) == (g.sf == 1) &&
                                                   (f->scrunch == RT_SCRUNCH_GENERAL) == (g.sf > 1 && !scrunch_staged((uint32_t)g.sf)) &&
                                                   f->scrunch_chunks == (g.sf > 1 ? scrunch_chunks((uint32_t)g.sf) : 0),
                                               "dered forms: scrunch");
                                        if (f->scrunch == RT_SCRUNCH_STAGED_VEC)
                                            expect(in16, "dered forms: staged loads aligned");
                                        expect((f->rmed == RT_RMED_SMALL) == (g.rmed_w <= 255), "dered forms: rmed");
                                        expect((f->subtract == RT_SUBTRACT_PER_SAMPLE) == (g.sf == 1), "dered forms: per sample");
                                        if (f->subtract == RT_SUBTRACT_SLOPE4)
                                            expect(in16 && out16, "dered forms: groups aligned");
                                        expect(f->fused == (norm && f->subtract == RT_SUBTRACT_SLOPE4), "dered forms: fused");
                                    }
                                    expect((f->norm_apply != 0) == norm && (f->norm_partial != 0) == (norm && !f->fused),
                                           "dered forms: normalisation stages");
                                    if (f->norm_apply == RT_NORM_VEC)
                                        expect(out16 && (dered || in16), "dered forms: apply aligned");
                                }
    expect(calls > 5000 && seen_scrunch[0] && seen_scrunch[1] && seen_scrunch[2] && seen_scrunch[3] && seen_sub[1] &&
               seen_sub[2] && seen_sub[3] && fused && two_pass,
           "dered forms: the sweep reaches every form");
    // the statistics grid's second load: n / 4 and n against kNormBlocks * 256
    for (size_t n : {(size_t)131072, (size_t)131073, (size_t)524291, (size_t)524292}) {
        std::unique_ptr<rt_dered_forms> v(new rt_dered_forms), s(new rt_dered_forms);
        const size_t stride = (n + 3) / 4 * 4;
        expect(rt_deredden_forms(n, 5, 3, 0, 1, 0, 0, stride, stride, v.get()) == RT_OK &&
                   rt_deredden_forms(n, 5, 3, 0, 1, 4, 0, stride, stride, s.get()) == RT_OK,
               "dered forms: normalise only");
        expect(v->norm_partial == RT_NORM_VEC && v->norm_passes == (n / 4 > 131072 ? 2u : 1u) &&
                   s->norm_partial == RT_NORM_SCALAR && s->norm_passes == (n > 131072 ? 2u : 1u),
               "dered forms: norm_passes");
    }
    std::unique_ptr<rt_dered_forms> f(new rt_dered_forms);
    expect(rt_deredden_forms(1000, 100, 4, 1, 1, 0, 0, 1000, 1000, f.get()) == RT_EINVAL &&
               rt_deredden_forms(1000, 100, 3, 1, 1, 2, 0, 1000, 1000, f.get()) == RT_EINVAL &&
               rt_deredden_forms(1000, 100, 3, 1, 1, 0, 16, 1000, 1000, f.get()) == RT_EINVAL &&
               rt_deredden_forms(1000, 100, 3, 1, 1, 0, 0, 1000, 1000, nullptr) == RT_EINVAL,
           "dered forms: refusals");
}

void check_dered()
{
    const size_t sizes[] = {30011, 32768, 4097, 1000};   // 30011: the GPU dereddening tests' series
    const size_t widths[] = {5, 151, 203, 303, 404, 1001, 15625};
    const size_t minpts[] = {3, 39, 101};
    size_t cases = 0, sf1 = 0, sfn = 0;
    for (size_t size : sizes)
        for (size_t ws : widths)
            for (size_t mp : minpts)
                for (size_t batch : {(size_t)1, (size_t)3})
                    for (int dered = 0; dered < 2; ++dered) {
                        DeredGeom g;
                        try {
                            g = dered_geom(size, ws, mp, batch, dered != 0);
                        } catch (const std::invalid_argument&) {
                            continue;   // an even or too wide window
                        }
                        ++cases;
                        if (dered) ++(g.sf == 1 ? sf1 : sfn);
                        const size_t bytes = dered_ws_bytes(g);
                        size_t api = 0;
                        if (dered)
                            expect(rt_deredden_workspace_bytes(size, ws, mp, batch, &api) == RT_OK && api == bytes,
                                   "dered: rt_deredden_workspace_bytes");
                        // the fused normalisation's partials and stats, the unfused one's partials
                        expect((dered ? 2 * dered_norm_blocks(size) * batch + 2 * batch : 0) <= g.partial_doubles &&
                                   (size_t)kNormBlocks * batch + 2 * batch <= g.partial_doubles,
                               "dered: partials");
                        for (size_t shift : {(size_t)0, (size_t)4, (size_t)252}) {   // workspaces at any float address
                            std::unique_ptr<char[]> buf(new char[bytes + shift]);
                            char* const base = buf.get() + shift;
                            const DeredWs w = dered_ws_layout(base, g);
                            expect((char*)w.lores == base && w.rmed == w.lores + g.lores_floats, "dered: floats");
                            expect((char*)w.slopes >= (char*)(w.rmed + g.rmed_floats) && (uintptr_t)w.slopes % 8 == 0 &&
                                       w.partials == w.slopes + g.slope_doubles,
                                   "dered: doubles follow the floats, on 8 bytes");
                            expect((char*)(w.partials + g.partial_doubles) <= base + bytes, "dered: ends inside");
                            std::memset(w.lores, 1, g.lores_floats * sizeof(float));
                            std::memset(w.rmed, 2, g.rmed_floats * sizeof(float));
                            std::memset(w.slopes, 3, g.slope_doubles * sizeof(double));
                            std::memset(w.partials, 4, g.partial_doubles * sizeof(double));
                        }
                    }
    expect(cases > 100 && sf1 > 0 && sfn > 0, "dered: the sweep covers sf == 1 and sf > 1");
    check_dered_forms();
}

// ---- harmonic
struct Clusters {
    std::vector<double> freq, snr, ducy, dm;
    HInputs in() const { return HInputs{freq.data(), snr.data(), ducy.data(), dm.data()}; }
};

Clusters clusters(size_t n)   // ranked by S/N; small-integer frequency ratios, some a little off, four DMs
{
    Clusters c;
    for (size_t i = 0; i < n; ++i) {
        c.freq.push_back(0.5 * (double)(i % 7 + 1) / (double)(i % 3 + 1) * (i % 5 == 0 ? 1.0 + 1e-4 : 1.0));
        c.snr.push_back(60.0 - 0.3 * (double)i);
        c.ducy.push_back(0.05);
        c.dm.push_back(40.0 * (double)(i % 4));
    }
    return c;
}

struct Flags {
    std::vector<int32_t> parent;
    std::vector<int64_t> hnum, hden;
    explicit Flags(size_t n) : parent(n, -1), hnum(n, 0), hden(n, 0) {}
    bool operator==(const Flags& o) const { return parent == o.parent && hnum == o.hnum && hden == o.hden; }
};

// Tiles of `rows` rows computed by htest_pair as the device would, resolved
// one after the other.  flip: every fifth pair is listed as near with the
// wrong bit.  overflow_tile: that tile reports more near pairs than the cap
// and carries neither list nor words.
Flags resolve(const Clusters& c, size_t n, size_t rows, const HParams& P, bool flip, size_t overflow_tile,
              HTileCounts* total)
{
    Flags f(n);
    const HInputs in = c.in();
    const size_t wpr = (n + 63) / 64, nrows = n - 1;
    for (size_t t = 0, i0 = 0; i0 < nrows; ++t, i0 += rows) {
        const size_t r = std::min(rows, nrows - i0);
        HTileCounts tc;
        if (t == overflow_tile) {
            tc = hresolve_tile(kHNearCap + 1, nullptr, nullptr, i0, r, wpr, n, in, P, f.parent.data(), f.hnum.data(),
                               f.hden.data());
        } else {
            std::unique_ptr<uint64_t[]> words(new uint64_t[r * wpr]());
            std::vector<HNearPair> near;
            for (size_t i = i0; i < i0 + r; ++i)
                for (size_t j = i + 1; j < n; ++j) {
                    bool bit = htest_pair(in.at(i), in.at(j), P, nullptr);
                    if (flip && (i * 31 + j) % 5 == 0) {
                        near.push_back(HNearPair{(uint32_t)i, (uint32_t)j});
                        bit = !bit;
                    }
                    if (bit) words[(i - i0) * wpr + j / 64] |= (uint64_t)1 << (j % 64);
                }
            std::unique_ptr<HNearPair[]> list(new HNearPair[near.size()]);
            std::copy(near.begin(), near.end(), list.get());
            tc = hresolve_tile((uint32_t)near.size(), list.get(), words.get(), i0, r, wpr, n, in, P, f.parent.data(),
                               f.hnum.data(), f.hden.data());
            expect(tc.near_pairs == near.size() && tc.host_rows == 0, "harmonic: a tile's counts");
        }
        total->near_pairs += tc.near_pairs;
        total->host_rows += tc.host_rows;
    }
    return f;
}

void check_harmonic()
{
    HParams P{};
    P.tobs = 600.0;
    P.band = 2.5e-7;
    P.phase_distance_max = 1.0;
    P.dm_distance_max = 3.0;
    P.snr_distance_max = 25.0;
    P.denom_max = 100;
    for (size_t n : {(size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)130}) {
        const Clusters c = clusters(n);
        const HInputs in = c.in();
        Flags want(n);   // the plain rank-order loop
        size_t flagged = 0;
        for (size_t i = 0; i + 1 < n; ++i) {
            if (want.parent[i] >= 0) continue;
            for (size_t j = i + 1; j < n; ++j)
                if (want.parent[j] < 0 && htest_pair(in.at(i), in.at(j), P, nullptr)) {
                    const HDiag d = hdiag_pair(in.at(i), in.at(j), P);
                    want.parent[j] = (int32_t)i;
                    want.hnum[j] = d.num;
                    want.hden[j] = d.den;
                    ++flagged;
                }
        }
        if (n >= 63) expect(flagged > n / 8 && flagged < n - 1, "harmonic: the clusters are a mix");
        for (size_t rows : {(size_t)1, (size_t)7, n - 1}) {
            if (rows > n - 1) continue;
            const std::string tag = "harmonic n " + std::to_string(n) + " rows " + std::to_string(rows);
            HTileCounts tc;
            expect(resolve(c, n, rows, P, false, ~(size_t)0, &tc) == want && !tc.near_pairs, tag + ": plain");
            tc = HTileCounts();
            expect(resolve(c, n, rows, P, true, ~(size_t)0, &tc) == want && (n < 6 || tc.near_pairs), tag + ": near pairs");
            tc = HTileCounts();
            expect(resolve(c, n, rows, P, true, 0, &tc) == want && tc.host_rows >= 1, tag + ": overflow");
        }
        // a near pair outside the tile or the matrix: the library's own error, nothing read or written
        const size_t wpr = (n + 63) / 64;
        const HNearPair outside[] = {{0, (uint32_t)n}, {1, 1}, {(uint32_t)n - 1, (uint32_t)n}, {0, (uint32_t)(64 * wpr)}};
        for (const HNearPair& bad : outside) {
            Flags f(n);
            std::unique_ptr<uint64_t[]> words(new uint64_t[wpr]());
            std::unique_ptr<HNearPair[]> list(new HNearPair[1]{bad});
            std::string err;
            try {
                hresolve_tile(1, list.get(), words.get(), 0, 1, wpr, n, in, P, f.parent.data(), f.hnum.data(),
                              f.hden.data());
            } catch (const std::runtime_error& e) {
                err = e.what();
            }
            expect(err == "harmonics: bad near pair" && f == Flags(n), "harmonic: bad near pair");
        }
    }
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "all";
    if (mode != "all" && mode != "fold" && mode != "dered" && mode != "harmonic") {
        std::fprintf(stderr, "usage: host_check [fold|dered|harmonic]\n");
        return 2;
    }
    if (mode == "all" || mode == "fold") check_fold();
    if (mode == "all" || mode == "dered") check_dered();
    if (mode == "all" || mode == "harmonic") check_harmonic();
    if (fails)
        std::printf("host_check: %d failures\n", fails);
    else
        std::printf("host_check %s OK\n", mode.c_str());
    return fails ? 1 : 0;
}
