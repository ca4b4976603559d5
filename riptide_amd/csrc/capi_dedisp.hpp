// What the C ABI's translation units of the filterbank side share
// (capi_dedisp.cpp, capi_cutout.cpp): the block mask of a device call.
#pragma once
#include <cstdint>
#include <stdexcept>

#include "dedisp_types.hpp"
#include "kernels.hpp"

namespace rt {

// A block mask of a device call over nsamp_blk rows (the shape is checked):
// the shared check, the fill aligned to its type, then the kernels' form of
// it.  No mask (a null pointer) is no DedispCells: the plain kernels.
struct DeviceCells {
    DedispCells cells{};
    bool set = false;
    DeviceCells(const rt_block_mask* bm, int dtype, size_t nsamp_blk)
    {
        dedisp_check_block_mask(bm, nsamp_blk);
        if (!bm) return;
        if ((uintptr_t)bm->fill % dedisp_fill_bytes(dtype))
            throw std::invalid_argument("block_mask: misaligned fill");
        cells = DedispCells{bm->cells, bm->fill, bm->t_origin, (uint64_t)bm->block_len};
        set = true;
    }
    const DedispCells* get() const { return set ? &cells : nullptr; }
};

}  // namespace rt
