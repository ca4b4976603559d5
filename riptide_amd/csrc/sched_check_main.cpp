// Host-only schedule checker, built with AddressSanitizer + UBSan by
// `make -C riptide_amd/csrc asan`: drives the host
// planner and the C ABI's host-only entry points -- rt_periodogram_grid,
// rt_schedule_check, rt_ffa_schedule_check, rt_ladder_check, rt_ladder_layout -- which build
// every unit blob, DMA segment table and row-slot table the cone kernel
// trusts.  No device call, and none linked: the checker is this file,
// plan.cpp and host_api.cpp.  Usage:
//   sched_check pgram N TSAMP PMIN PMAX BMIN BMAX NWIDTHS
//   sched_check ffa ROWS COLS
//   sched_check kinds N TSAMP PMIN PMAX BMIN BMAX WIDTH...
// (kinds: the plan built for these boxcar widths, its final launches by S/N
// kind -- rt_schedule_final_kinds -- and the bins of the final units of each).
// Prints one line of results; exit status 0 iff every call returned RT_OK.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "riptide_amd.h"

int main(int argc, char** argv)
{
    if (argc >= 9 && !std::strcmp(argv[1], "pgram")) {
        const size_t n = std::strtoull(argv[2], nullptr, 10);
        const double tsamp = std::atof(argv[3]), pmin = std::atof(argv[4]), pmax = std::atof(argv[5]);
        const size_t bmin = std::strtoull(argv[6], nullptr, 10), bmax = std::strtoull(argv[7], nullptr, 10);
        const size_t nw = std::strtoull(argv[8], nullptr, 10);
        size_t L = 0;
        if (rt_periodogram_length(n, tsamp, pmin, pmax, bmin, bmax, &L)) {
            std::printf("length: %s\n", rt_last_error());
            return 1;
        }
        std::vector<double> periods(L);
        std::vector<uint32_t> foldbins(L);
        if (rt_periodogram_grid(n, tsamp, pmin, pmax, bmin, bmax, periods.data(), foldbins.data())) {
            std::printf("grid: %s\n", rt_last_error());
            return 1;
        }
        uint64_t xf = 0, items = 0, launches = 0, cells = 0;
        double alg = 0, moved = 0;
        if (rt_schedule_check(n, tsamp, nw, pmin, pmax, bmin, bmax, &xf, &items, &launches, &alg, &moved, &cells)) {
            std::printf("schedule: %s\n", rt_last_error());
            return 1;
        }
        int fused = -1;
        uint64_t rungs = 0;
        if (rt_ladder_check(n, tsamp, pmin, pmax, bmin, bmax, &fused, &rungs)) {
            std::printf("ladder: %s\n", rt_last_error());
            return 1;
        }
        // the ladder's layout, first its size alone, then every rung's record
        uint64_t nr = 0, leaf = 0;
        int mode = -1;
        uint32_t margin = 0;
        if (rt_ladder_layout(n, tsamp, pmin, pmax, bmin, bmax, nullptr, 0, &nr, nullptr, nullptr, nullptr)) {
            std::printf("ladder layout: %s\n", rt_last_error());
            return 1;
        }
        std::vector<rt_ladder_rung> lr(nr);
        if (rt_ladder_layout(n, tsamp, pmin, pmax, bmin, bmax, lr.data(), lr.size(), &nr, &leaf, &mode, &margin) ||
            nr != rungs || mode != fused) {
            std::printf("ladder layout: %s\n", rt_last_error());
            return 1;
        }
        for (const rt_ladder_rung& r : lr)
            if (r.leaf_off + r.n > leaf) {
                std::printf("ladder layout: a rung ends past the leaf buffer\n");
                return 1;
            }
        std::printf("pgram L=%zu transforms=%llu items=%llu launches=%llu alg=%.6e moved=%.6e fused=%d rungs=%llu\n", L,
                    (unsigned long long)xf, (unsigned long long)items, (unsigned long long)launches, alg, moved, fused,
                    (unsigned long long)rungs);
        return 0;
    }
    if (argc >= 9 && !std::strcmp(argv[1], "kinds")) {
        const size_t n = std::strtoull(argv[2], nullptr, 10);
        const double tsamp = std::atof(argv[3]), pmin = std::atof(argv[4]), pmax = std::atof(argv[5]);
        const size_t bmin = std::strtoull(argv[6], nullptr, 10), bmax = std::strtoull(argv[7], nullptr, 10);
        std::vector<uint64_t> widths;
        for (int i = 8; i < argc; ++i) widths.push_back(std::strtoull(argv[i], nullptr, 10));
        uint64_t launches = 0, nrows = 0, nseg = 0;
        std::vector<uint8_t> kinds(bmax + 2, 0);
        if (rt_schedule_final_kinds(n, tsamp, widths.data(), widths.size(), pmin, pmax, bmin, bmax, &launches, &nrows, &nseg,
                                    kinds.data(), kinds.size())) {
            std::printf("kinds: %s\n", rt_last_error());
            return 1;
        }
        std::printf("kinds launches=%llu final_row_group=%llu final_segmented=%llu", (unsigned long long)launches,
                    (unsigned long long)nrows, (unsigned long long)nseg);
        // bins ranges of the final units of each kind
        for (int k = 1; k <= 2; ++k) {
            std::printf(k == 1 ? " row_group_bins=" : " segmented_bins=");
            bool any = false;
            for (size_t b = 0; b < kinds.size();) {
                if (!(kinds[b] & k)) {
                    ++b;
                    continue;
                }
                size_t e = b;
                while (e + 1 < kinds.size() && (kinds[e + 1] & k)) ++e;
                if (e > b) std::printf("%s%zu-%zu", any ? "," : "", b, e);
                else std::printf("%s%zu", any ? "," : "", b);
                any = true;
                b = e + 1;
            }
            if (!any) std::printf("none");
        }
        std::printf("\n");
        return 0;
    }
    if (argc >= 4 && !std::strcmp(argv[1], "ffa")) {
        uint64_t launches = 0;
        if (rt_ffa_schedule_check(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), &launches)) {
            std::printf("ffa: %s\n", rt_last_error());
            return 1;
        }
        std::printf("ffa launches=%llu\n", (unsigned long long)launches);
        return 0;
    }
    std::fprintf(stderr, "usage: sched_check pgram N TSAMP PMIN PMAX BMIN BMAX NWIDTHS | kinds N TSAMP PMIN PMAX BMIN BMAX "
                         "WIDTH... | ffa ROWS COLS\n");
    return 2;
}
