// Incoherent dedispersion for MI355X (gfx950): a resident block of
// channelised samples, time-major [nsamp, nchans] as a SIGPROC filterbank
// stores them, summed along the sweep of every trial DM
//   out[d, t] = sum over unmasked c of x[t + delay[d, c], c]
// (the specification: rt_dedisperse_host, dedisp_host.cpp).
//
//   dedisp_transpose*_kernel  the block to channel-major rows in the
//                             workspace, through an LDS tile; 8-bit data stays
//                             8-bit (signed samples are stored biased by 128),
//                             the row pitch is padded to 16 bytes and the
//                             padding is written as zero
//   dedisp_unpack_transpose_kernel  1-, 2- and 4-bit packed rows unpacked inside
//                             that transpose, to the same 8-bit rows; 16-bit
//                             rows go to exact float32 rows (the zero-DM
//                             transpose without the mean).  The zero-DM and
//                             statistics kernels read packed rows through DdRow
//   dedisp_sum_kernel         one workgroup = 16 DMs x 256 outputs; per step
//                             of 16 channels the span of each channel that the
//                             tile's DMs read is staged in LDS with aligned
//                             dword loads, then every wave adds its four DMs
//                             (one DM at a time, its delay wave-uniform)
//   dedisp_sum_kernel<T, DdBandTable>  the same tile over the channels [lo, hi)
//                             of one band of a table, a grid layer per band:
//                             out[d, b, t], every band of a batch of DMs from
//                             one pass over the transposed block
//   dedisp_decimate_kernel    a step of a DM plan (launch_dedisperse_steps): the
//                             transposed rows summed f samples at a time into
//                             float32 rows, which dedisp_sum_kernel<float> then
//                             sums with the step's delays
//   dedisp_rowmean_kernel     zero-DM filter (RT_DEDISP_ZERO_DM): m[t], the mean
//                             of time sample t over the unmasked channels, one
//                             wave per sample
//   dedisp_transpose_zdm_kernel  the zero-DM form of both transposes: float32
//                             x - m rows for every sample type, then summed by
//                             dedisp_sum_kernel<float>
//   dedisp_chanstats*_kernel  per-channel sum and sum of squares: partial sums
//                             per chunk of time, folded in chunk order (no
//                             atomics: the same bits every time)
//   dedisp_blockstats*_kernel the same sums per (block of block_len time
//                             samples, channel): rt_block_stats_device
//   Cells = DdCells           the block mask (rt_block_mask, riptide_amd.h) as
//                             the last template argument of every kernel that
//                             reads the time-major block: a flagged cell's
//                             sample is replaced by its channel's fill as it
//                             is read.  Cells = DdNoCells (empty, the default)
//                             is the plain kernel: every masked statement is
//                             under `if constexpr`
//
// No load leaves its buffer: the transpose reads x only at t < nsamp, the
// staging loads are clamped to the row's padded pitch inside the workspace,
// and delays are clamped to [0, max_delay] as they are read.
// Exactness: 8-bit sums are integers (16-bit packed partial sums of at most
// 16 channels, then int32), converted once; float sums are float32 additions
// in channel order.
//
// The launchers at the end choose by sample type in one place, dd_dispatch:
// launch_zero_dm_mean, launch_channel_stats and the zero-DM transpose are one
// call of it each.  launch_dedisp_rows fills the workspace with 8-bit or
// float32 rows; launch_dedisperse calls it, then makes the one launch_sum call
// of those rows.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "dedisp_types.hpp"
#include "kernels.hpp"

namespace rt {

namespace {

constexpr uint32_t kDdThreads = 256;
constexpr uint32_t kDdWaves = 4;
constexpr uint32_t kDdTile = kDedispTile;   // outputs of a time tile (256): 4 per lane
constexpr uint32_t kDdPerWave = 4;      // DMs a wave sums
constexpr uint32_t kDdDms = kDdWaves * kDdPerWave;
constexpr uint32_t kDdChans = 16;       // channels staged per step
constexpr uint32_t kDdSkip = 0xFFFFFFFFu;     // channel masked or past nchans
constexpr uint32_t kDdDirect = 0xFFFFFFFEu;   // span too long to stage: read from the workspace row

// dwords of one channel's staged span: the time tile plus the spread of the
// tile's delays.  The numbers and the rule are dedisp_types.hpp's (dedisp_span,
// which rt_dedisperse_span_plan restates for the tests): 8-bit data is staged
// up to a spread hi - (lo & ~3) of 800 samples, that is hi - lo of 800, 799,
// 798 or 797 for lo % 4 = 0 .. 3, float data up to hi - lo of 264; a wider
// spread takes the direct path
template <class T>
struct DdSpan {
    static constexpr uint32_t dwords = dedisp_span_dwords(sizeof(T));
};

// ---- the block mask (rt_block_mask, riptide_amd.h)
// Which samples a kernel reading the time-major block replaces, its last
// argument, as Sel is dedisp_sum_kernel's.  DdNoCells (empty: the plain call)
// replaces nothing.  DdCells: sample (t, c) of the block is fill[c] where
// cells[(t_origin + t) / block_len, c] is not zero; the caller has checked
// that every row t < nsamp lies in a block below nblocks
// (rt_dedisperse_device_cells), and no kernel looks a cell up for any other
// row or for a channel at or past nchans.  fill holds one value per channel in
// the sample's own type (dedisp_fill_bytes).
struct DdNoCells {};
using DdCells = DedispCells;   // kernels.hpp: cells, fill, t_origin, block_len

template <class Cells>
constexpr bool kDdMasked = !std::is_same<Cells, DdNoCells>::value;

// The flag of one channel along the rows of a tile, held in a register: rows
// are asked for in ascending order, and the flag is loaded again only when a
// row lies past the block it was loaded for -- a load per block the tile
// touches, not per sample.  `first` is the absolute sample of tile row 0.
struct DdCellFlag {
    const uint8_t* col;   // cells + c
    uint64_t first;
    uint32_t nchans;
    uint64_t block_len;
    uint32_t end = 0;     // first tile row past the block `flag` is of (0: nothing loaded)
    uint32_t flag = 0;
    __device__ inline DdCellFlag(const DdCells& k, uint64_t t0, uint32_t c, uint32_t nch)
        : col(k.cells + c), first(k.t_origin + t0), nchans(nch), block_len(k.block_len)
    {
    }
    __device__ inline bool at(uint32_t i)
    {
        if (i >= end) {
            const uint64_t blk = (first + i) / block_len;
            const uint64_t e = (blk + 1) * block_len - first;   // > i
            end = (uint32_t)min(e, (uint64_t)0xFFFFFFFFu);
            flag = col[blk * nchans];
        }
        return flag != 0;
    }
};

// A lane's state of the mask along a tile's rows in a kernel's one load loop:
// State (DdCellFlag, DdPackedCells) with a mask, nothing without one, so the
// loop holds a single masked statement under `if constexpr`.
struct DdNoState {
    template <class... A>
    __device__ inline DdNoState(const A&...)
    {
    }
};
template <class Cells, class State>
using DdStateOf = typename std::conditional<kDdMasked<Cells>, State, DdNoState>::type;

// 8-bit: tile of 64 channels x 256 samples, read a byte per lane along the
// channels, written a dword per lane along time.  A tile row has one t for
// the whole wave and a lane one channel for all rows: the masked form keeps
// the lane's fill (biased as the samples are) and its cell in registers.
template <class Cells = DdNoCells>
__global__ __launch_bounds__(kDdThreads) void dedisp_transpose8_kernel(
    const uint8_t* __restrict__ x, uint32_t nsamp, uint32_t nchans, uint8_t* __restrict__ ws, uint64_t pitch,
    uint32_t flip, Cells cells)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[64][260];
    const uint32_t tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * 256;
    const uint32_t c0 = blockIdx.y * 64;
    const uint32_t c = c0 + tx;
    [[maybe_unused]] DdStateOf<Cells, DdCellFlag> cf(cells, t0, c, nchans);
    [[maybe_unused]] uint32_t fv = 0;
    if constexpr (kDdMasked<Cells>) {
        if (c < nchans) fv = (uint32_t)static_cast<const uint8_t*>(cells.fill)[c] ^ flip;
    }
    for (uint32_t i = ty; i < 256; i += 4) {
        const uint64_t t = t0 + i;
        uint32_t v = 0;
        if (c < nchans && t < nsamp) {
            v = x[t * nchans + c] ^ flip;
            if constexpr (kDdMasked<Cells>) {
                if (cf.at(i)) v = fv;
            }
        }
        tile[tx][i] = (uint8_t)v;
    }
    __syncthreads();
    const uint64_t tb = t0 + tx * 4;
    for (uint32_t i = ty; i < 64; i += 4) {
        const uint32_t co = c0 + i;
        if (co < nchans && tb < pitch)   // the pitch is a multiple of 16: the dword is inside the row
            *reinterpret_cast<uint32_t*>(ws + (uint64_t)co * pitch + tb) =
                *reinterpret_cast<const uint32_t*>(&tile[i][tx * 4]);
    }
}

// ---- packed sample types (riptide_amd.h: RT_DEDISP_U1, U2, U4, U16)
// Tag of rows of NBITS-bit unsigned samples: the T of a kernel whose block is
// packed bytes, [nsamp, nchans * NBITS / 8], only byte-aligned.
template <int NBITS>
struct DdBits {
    static constexpr int kBits = NBITS;
};

// (row pointer, c) -> sample, for every T a kernel reads rows of.  Plain
// types: the load itself.  kIntSums: int32 partial sums are in range (the
// kernels say why), float64 otherwise.
template <class T>
struct DdRow {
    static constexpr bool kIntSums = sizeof(T) == 1;
    static __device__ inline const T* at(const T* x, uint64_t t, uint32_t nchans) { return x + t * nchans; }
    static __device__ inline T get(const T* row, uint32_t c) { return row[c]; }
};

// Packed rows: byte loads (these readers are not the hot path).  1/2/4 bit,
// least significant bits first; 16 bit little-endian.  c * NBITS < 2^26.
template <int NBITS>
struct DdRow<DdBits<NBITS>> {
    static constexpr bool kIntSums = NBITS < 16;
    static __device__ inline const uint8_t* at(const DdBits<NBITS>* x, uint64_t t, uint32_t nchans)
    {
        return reinterpret_cast<const uint8_t*>(x) + t * ((uint64_t)nchans * NBITS / 8);
    }
    static __device__ inline uint32_t get(const uint8_t* row, uint32_t c)
    {
        if constexpr (NBITS == 16) {
            return (uint32_t)row[2 * c] | (uint32_t)row[2 * c + 1] << 8;
        } else {
            const uint32_t bit = c * NBITS;
            return ((uint32_t)row[bit >> 3] >> (bit & 7)) & ((1u << NBITS) - 1u);
        }
    }
};

// (fill pointer of a block mask, c) -> the channel's fill as DdRow<T>::get
// returns a sample: T itself for the plain types, for packed rows the low
// NBITS bits of a byte (1/2/4 bit) or a uint16
template <class T>
struct DdFill {
    static __device__ inline T get(const void* fill, uint32_t c) { return static_cast<const T*>(fill)[c]; }
};
template <int NBITS>
struct DdFill<DdBits<NBITS>> {
    static __device__ inline uint32_t get(const void* fill, uint32_t c)
    {
        if constexpr (NBITS == 16) return static_cast<const uint16_t*>(fill)[c];
        else return static_cast<const uint8_t*>(fill)[c] & ((1u << NBITS) - 1u);
    }
};

// The cells of the nb packed bytes from byte b of a row (nb * 8 / NBITS
// channels, nb = 1 or 4: what a lane of dedisp_unpack_transpose_kernel loads
// at once), as bits in the packed word itself: `fillw` is the fills of those
// channels packed as the samples are, `selw` has every bit of a flagged
// channel's field set, so the replacement of all the word's channels is
//   (w & ~selw) | (fillw & selw)
// -- replacing after unpacking, channel by channel, gives the same bits.  selw
// is loaded again only when a row lies past the block it was loaded for.  A
// byte below row_bytes holds channels below nchans only (rows are whole bytes).
template <int NBITS>
struct DdPackedCells {
    static constexpr uint32_t kPer = 8 / NBITS;
    static constexpr uint32_t kField = (1u << NBITS) - 1u;
    const uint8_t* col;   // cells + the word's first channel
    uint64_t first, block_len;
    uint32_t nchans, nch;   // nch: channels of the word
    uint32_t end = 0, fillw = 0, selw = 0;
    __device__ inline DdPackedCells(const DdCells& k, uint64_t t0, uint32_t b, uint32_t nb, uint32_t nchans_)
        : col(k.cells + (uint64_t)b * kPer), first(k.t_origin + t0), block_len(k.block_len), nchans(nchans_),
          nch(nb * kPer)
    {
        const uint8_t* f = static_cast<const uint8_t*>(k.fill) + (uint64_t)b * kPer;
        for (uint32_t j = 0; j < nch; ++j) fillw |= ((uint32_t)f[j] & kField) << (j * NBITS);
    }
    __device__ inline uint32_t replace(uint32_t w, uint32_t i)
    {
        if (i >= end) {
            const uint64_t blk = (first + i) / block_len;
            const uint64_t e = (blk + 1) * block_len - first;   // > i
            end = (uint32_t)min(e, (uint64_t)0xFFFFFFFFu);
            const uint8_t* row = col + blk * nchans;
            selw = 0;
            for (uint32_t j = 0; j < nch; ++j)
                if (row[j]) selw |= kField << (j * NBITS);
        }
        return (w & ~selw) | (fillw & selw);
    }
};

// 1/2/4 bit: packed rows to the 8-bit workspace rows dedisp_transpose8_kernel
// writes, the values unbiased, for dedisp_sum_kernel<uint8_t> with bias 0.
// Tile of 64 packed bytes x 256 samples, that is 512, 256 or 128 channels: a
// wave's reads of a time row cover 64 contiguous bytes at every width.  The
// tile stays packed in LDS (16.25 KB), transposed byte by byte; the bits come
// out on the way to the workspace: lane l reads the dword of samples 4 l .. 4 l
// + 3 of a packed byte once, then one shift and one mask per channel of that
// byte give four samples at a time (a field never crosses a byte), stored as
// one dword per lane along time.
// x is only byte-aligned: dword loads (16 lanes a row, four rows a wave
// instruction) when `dwords` says x and row_bytes are multiples of 4, byte
// loads otherwise.  A load touches byte b < row_bytes of a row t < nsamp only
// (the dword path: b + 3 < row_bytes, both multiples of 4), nothing at or
// beyond nsamp * row_bytes.
// The masked form replaces in the packed word as it is loaded (DdPackedCells),
// where a lane keeps its bytes -- its channels -- across rows; the tile then
// holds x' and the rest of the kernel is the plain one.
template <int NBITS, class Cells = DdNoCells>
__global__ __launch_bounds__(kDdThreads) void dedisp_unpack_transpose_kernel(
    const uint8_t* __restrict__ x, uint32_t nsamp, uint32_t nchans, uint32_t row_bytes, uint8_t* __restrict__ ws,
    uint64_t pitch, uint32_t dwords, Cells cells)
{
    constexpr uint32_t kPer = 8 / NBITS;                              // channels of a packed byte
    constexpr uint32_t kMask = ((1u << NBITS) - 1u) * 0x01010101u;    // the low field of each of four bytes
    __shared__ __attribute__((aligned(16))) uint8_t tile[64][260];
    const uint32_t tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * 256;
    const uint32_t b0 = blockIdx.y * 64;
    if (dwords) {   // uniform over the grid
        const uint32_t j = tx & 15, r = tx >> 4;
        const uint32_t b = b0 + 4 * j;
        [[maybe_unused]] DdStateOf<Cells, DdPackedCells<NBITS>> pc(cells, t0, b, b < row_bytes ? 4u : 0u, nchans);
        for (uint32_t i = ty * 4 + r; i < 256; i += 16) {
            const uint64_t t = t0 + i;
            uint32_t v = 0;
            if (b < row_bytes && t < nsamp) {
                v = *reinterpret_cast<const uint32_t*>(x + t * row_bytes + b);
                if constexpr (kDdMasked<Cells>) v = pc.replace(v, i);
            }
            tile[4 * j][i] = (uint8_t)v;
            tile[4 * j + 1][i] = (uint8_t)(v >> 8);
            tile[4 * j + 2][i] = (uint8_t)(v >> 16);
            tile[4 * j + 3][i] = (uint8_t)(v >> 24);
        }
    } else {
        const uint32_t b = b0 + tx;
        [[maybe_unused]] DdStateOf<Cells, DdPackedCells<NBITS>> pc(cells, t0, b, b < row_bytes ? 1u : 0u, nchans);
        for (uint32_t i = ty; i < 256; i += 4) {
            const uint64_t t = t0 + i;
            uint32_t v = 0;
            if (b < row_bytes && t < nsamp) {
                v = x[t * row_bytes + b];
                if constexpr (kDdMasked<Cells>) v = pc.replace(v, i);
            }
            tile[tx][i] = (uint8_t)v;
        }
    }
    __syncthreads();
    const uint64_t tb = t0 + tx * 4;
    if (tb >= pitch) return;   // the pitch is a multiple of 16: a dword at tb < pitch is inside the row
    for (uint32_t i = ty; i < 64; i += 4) {
        const uint32_t b = b0 + i;
        if (b >= row_bytes) break;
        const uint32_t w = *reinterpret_cast<const uint32_t*>(&tile[i][tx * 4]);
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t co = b * kPer + k;   // < row_bytes * kPer = nchans
            if (co < nchans)
                *reinterpret_cast<uint32_t*>(ws + (uint64_t)co * pitch + tb) = (w >> (k * NBITS)) & kMask;
        }
    }
}

// float: tile of 64 channels x 64 samples.
template <class Cells = DdNoCells>
__global__ __launch_bounds__(kDdThreads) void dedisp_transpose32_kernel(
    const float* __restrict__ x, uint32_t nsamp, uint32_t nchans, float* __restrict__ ws, uint64_t pitch, Cells cells)
{
    __shared__ float tile[64][65];
    const uint32_t tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * 64;
    const uint32_t c0 = blockIdx.y * 64;
    const uint32_t c = c0 + tx;
    [[maybe_unused]] DdStateOf<Cells, DdCellFlag> cf(cells, t0, c, nchans);
    [[maybe_unused]] float fv = 0.0f;
    if constexpr (kDdMasked<Cells>) {
        if (c < nchans) fv = static_cast<const float*>(cells.fill)[c];
    }
    for (uint32_t i = ty; i < 64; i += 4) {
        const uint64_t t = t0 + i;
        float v = 0.0f;
        if (c < nchans && t < nsamp) {
            v = x[t * nchans + c];
            if constexpr (kDdMasked<Cells>) {
                if (cf.at(i)) v = fv;
            }
        }
        tile[tx][i] = v;
    }
    __syncthreads();
    const uint64_t t = t0 + tx;
    for (uint32_t i = ty; i < 64; i += 4) {
        const uint32_t co = c0 + i;
        if (co < nchans && t < pitch) ws[(uint64_t)co * pitch + t] = tile[i][tx];
    }
}

// ---- zero-DM filter (RT_DEDISP_ZERO_DM, riptide_amd.h) and channel statistics
constexpr uint32_t kRmRows = 4;                          // time samples a wave takes, one after the other
constexpr uint32_t kRmRowsPerWg = kDdWaves * kRmRows;    // time samples of a workgroup
constexpr uint32_t kCsChunk = 2048;                      // time samples of one partial sum of the statistics

// the sample as the value it stands for: int8 signed, no bias
template <class T>
__device__ inline float dd_value(T v)
{
    return (float)v;
}

// m[t] = (float32)(S[t] / Nu), S the sum of row t over the unmasked channels,
// Nu their number.  One wave per time sample, the lanes striding the channels
// (the fastest index: coalesced); int32 partial sums for 8-bit samples (at
// most 65793 * 255), float64 for float samples; a 64-lane butterfly, so every
// lane holds the same total, summed in an order that depends on nchans alone.
// Packed rows are read through DdRow: 1/2/4 bit in int32 (at most 65793 * 15),
// 16 bit in float64 (integers below 2^16 * 2^22 channels: exact).
// The masked form sums x' in the same order: a lane still adds its channels
// lane, lane + 64, ... of a row one after the other and the butterfly is the
// same, so it gives the bits the plain kernel gives on a block holding x'.
// Only the loops are exchanged -- the wave's four rows inside the channel
// loop, a sum per row -- so that a lane loads its channel's fill once and the
// cell once per block the four rows touch.
template <class T, class Cells = DdNoCells>
__global__ __launch_bounds__(kDdThreads) void dedisp_rowmean_kernel(
    const T* __restrict__ x, uint32_t nsamp, uint32_t nchans, const uint8_t* __restrict__ mask,
    float* __restrict__ m, Cells cells)
{
    using R = DdRow<T>;
    using Acc = typename std::conditional<R::kIntSums, int32_t, double>::type;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * kRmRowsPerWg + wave * kRmRows;
    if constexpr (kDdMasked<Cells>) {
        if (t0 >= nsamp) return;   // wave-uniform
        const uint32_t nr = (uint32_t)min((uint64_t)kRmRows, nsamp - t0);
        uint64_t blk[kRmRows];
#pragma unroll
        for (uint32_t r = 0; r < kRmRows; ++r) blk[r] = (cells.t_origin + t0 + min(r, nr - 1)) / cells.block_len;
        Acc s[kRmRows];
#pragma unroll
        for (uint32_t r = 0; r < kRmRows; ++r) s[r] = 0;
        int32_t nu = 0;
        for (uint32_t c = lane; c < nchans; c += 64) {
            if (mask && mask[c]) continue;
            const auto fv = DdFill<T>::get(cells.fill, c);
            uint32_t flag = cells.cells[blk[0] * nchans + c];
#pragma unroll
            for (uint32_t r = 0; r < kRmRows; ++r) {
                if (r >= nr) break;
                if (r && blk[r] != blk[r - 1]) flag = cells.cells[blk[r] * nchans + c];
                const auto v = R::get(R::at(x, t0 + r, nchans), c);
                s[r] += flag ? (Acc)fv : (Acc)v;
            }
            ++nu;
        }
#pragma unroll
        for (uint32_t r = 0; r < kRmRows; ++r) {
#pragma unroll
            for (uint32_t off = 32; off > 0; off >>= 1) s[r] += __shfl_xor(s[r], off, 64);
        }
#pragma unroll
        for (uint32_t off = 32; off > 0; off >>= 1) nu += __shfl_xor(nu, off, 64);
#pragma unroll
        for (uint32_t r = 0; r < kRmRows; ++r)
            if (lane == 0 && r < nr) m[t0 + r] = nu ? (float)((double)s[r] / (double)nu) : 0.0f;
        return;
    }
    for (uint32_t r = 0; r < kRmRows; ++r) {
        const uint64_t t = t0 + r;
        if (t >= nsamp) return;   // wave-uniform
        const auto* row = R::at(x, t, nchans);
        Acc s = 0;
        int32_t nu = 0;
        for (uint32_t c = lane; c < nchans; c += 64) {
            if (mask && mask[c]) continue;
            s += (Acc)R::get(row, c);
            ++nu;
        }
#pragma unroll
        for (uint32_t off = 32; off > 0; off >>= 1) {
            s += __shfl_xor(s, off, 64);
            nu += __shfl_xor(nu, off, 64);
        }
        if (lane == 0) m[t] = nu ? (float)((double)s / (double)nu) : 0.0f;
    }
}

// Zero-DM variant of both transposes: T = uint8_t, int8_t or float in, float32
// x - m out, channel-major; tile of 64 channels x 64 samples, the pitch in
// floats, its padding (and every t >= nsamp) written as zero.  T may be a
// packed row type (DdRow); kMean = false is the plain transpose of 16-bit rows
// to float32 (the values converted exactly, m not read).
template <class T, bool kMean = true, class Cells = DdNoCells>
__global__ __launch_bounds__(kDdThreads) void dedisp_transpose_zdm_kernel(
    const T* __restrict__ x, uint32_t nsamp, uint32_t nchans, const float* __restrict__ m, float* __restrict__ ws,
    uint64_t pitch, Cells cells)
{
    __shared__ float tile[64][65];
    const uint32_t tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * 64;
    const uint32_t c0 = blockIdx.y * 64;
    const uint32_t c = c0 + tx;
    [[maybe_unused]] DdStateOf<Cells, DdCellFlag> cf(cells, t0, c, nchans);
    [[maybe_unused]] float fv = 0.0f;   // the fill as the value it stands for
    if constexpr (kDdMasked<Cells>) {
        if (c < nchans) fv = dd_value(DdFill<T>::get(cells.fill, c));
    }
    for (uint32_t i = ty; i < 64; i += 4) {
        const uint64_t t = t0 + i;
        float v = 0.0f;
        if (t < nsamp) {   // wave-uniform: m[t] is one broadcast load
            float mt = 0.0f;
            if constexpr (kMean) mt = m[t];
            if (c < nchans) {
                v = dd_value(DdRow<T>::get(DdRow<T>::at(x, t, nchans), c));
                if constexpr (kDdMasked<Cells>) {
                    if (cf.at(i)) v = fv;
                }
                if constexpr (kMean) v = v - mt;
            }
        }
        tile[tx][i] = v;
    }
    __syncthreads();
    const uint64_t t = t0 + tx;
    for (uint32_t i = ty; i < 64; i += 4) {
        const uint32_t co = c0 + i;
        if (co < nchans && t < pitch) ws[(uint64_t)co * pitch + t] = tile[i][tx];
    }
}

// Per-channel sum and sum of squares of one chunk of kCsChunk time samples:
// the lanes across 64 channels, the four waves interleaved over the chunk's
// rows, their partial sums added in wave order through LDS.  8-bit samples
// are summed as integers (at most 512 rows x 128^2 or 255^2 per wave: below
// 2^31 / 2^32), float samples in float64.  part is [nchunks, 2, nchans].
// Packed rows (DdRow): 1/2/4 bit as integers (at most 512 x 15^2), 16 bit in
// float64 (512 x 65535^2 < 2^41: exact).
// dd_chunk_stats is the body of both statistics kernels: part[chunk] = those
// sums over the rows [t0, t1), t1 - t0 <= kCsChunk.  In float64 the order is:
// wave w adds the rows t0 + w, t0 + w + 4, ... one after the other from 0.0,
// then ((p0 + p1) + p2) + p3.
template <class T>
__device__ inline void dd_chunk_stats(const T* __restrict__ x, uint64_t t0, uint64_t t1, uint32_t nchans,
                                      double* __restrict__ part, uint32_t chunk)
{
    constexpr bool kBytes = DdRow<T>::kIntSums;
    using Sum = typename std::conditional<kBytes, int32_t, double>::type;
    using Sq = typename std::conditional<kBytes, uint32_t, double>::type;
    __shared__ double red[2][kDdWaves][64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t c = blockIdx.y * 64 + lane;
    Sum s = 0;
    Sq q = 0;
    if (c < nchans)
        for (uint64_t t = t0 + wave; t < t1; t += kDdWaves) {
            const Sum v = (Sum)DdRow<T>::get(DdRow<T>::at(x, t, nchans), c);
            s += v;
            q += (Sq)(v * v);
        }
    red[0][wave][lane] = (double)s;
    red[1][wave][lane] = (double)q;
    __syncthreads();
    if (wave < 2 && c < nchans) {   // wave 0 the sums, wave 1 the squares
        double a = red[wave][0][lane];
#pragma unroll
        for (uint32_t w = 1; w < kDdWaves; ++w) a += red[wave][w][lane];
        part[((uint64_t)chunk * 2 + wave) * nchans + c] = a;
    }
}

// The channel statistics: chunk blockIdx.x of the whole block.
template <class T>
__global__ __launch_bounds__(kDdThreads) void dedisp_chanstats_kernel(
    const T* __restrict__ x, uint32_t nsamp, uint32_t nchans, double* __restrict__ part)
{
    const uint64_t t0 = (uint64_t)blockIdx.x * kCsChunk;
    const uint64_t t1 = min(t0 + kCsChunk, (uint64_t)nsamp);
    dd_chunk_stats(x, t0, t1, nchans, part, blockIdx.x);
}

// The same sums per block of block_len time samples, blocks counted from row 0
// (rt_block_stats_device): workgroup blockIdx.x is chunk k = blockIdx.x % cpb
// of block b = blockIdx.x / cpb, the rows [b * block_len + k * kCsChunk, + kCsChunk)
// that lie in the block and below nsamp (none: zeros), cpb = ceil(block_len /
// kCsChunk).  dst is [nblk * cpb, 2, nchans]: the result itself when cpb == 1,
// the per-chunk partial sums otherwise.  The integer bounds are the chunk's.
template <class T>
__global__ __launch_bounds__(kDdThreads) void dedisp_blockstats_kernel(
    const T* __restrict__ x, uint32_t nsamp, uint32_t nchans, uint32_t block_len, uint32_t cpb,
    double* __restrict__ dst)
{
    const uint32_t b = blockIdx.x / cpb, k = blockIdx.x - b * cpb;
    const uint64_t t0 = (uint64_t)b * block_len + (uint64_t)k * kCsChunk;
    const uint64_t t1 = min(min(t0 + kCsChunk, ((uint64_t)b + 1) * block_len), (uint64_t)nsamp);
    dd_chunk_stats(x, t0, t1, nchans, dst, blockIdx.x);
}

// out[b, k, c] = the partial sums of block b's cpb chunks added in chunk order
// from 0.0 (written, not accumulated): one thread per (b, k, c)
__global__ __launch_bounds__(kDdThreads) void dedisp_blockstats_fold_kernel(
    const double* __restrict__ part, uint32_t cpb, uint64_t total, uint32_t nchans, double* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kDdThreads + threadIdx.x;   // (b * 2 + k) * nchans + c
    if (i >= total) return;
    const uint64_t b = i / (2ull * nchans), rest = i - b * 2ull * nchans;
    double a = 0.0;
    for (uint32_t k = 0; k < cpb; ++k) a += part[(b * cpb + k) * 2ull * nchans + rest];
    out[i] = a;
}

// acc[k, c] += the chunks' partial sums, in chunk order: one thread per (k, c)
__global__ __launch_bounds__(kDdThreads) void dedisp_chanstats_fold_kernel(
    const double* __restrict__ part, uint32_t nchunks, uint32_t nchans, double* __restrict__ acc)
{
    const uint32_t i = blockIdx.x * kDdThreads + threadIdx.x;   // k * nchans + c
    if (i >= 2 * nchans) return;
    double a = acc[i];
    for (uint32_t k = 0; k < nchunks; ++k) a += part[(uint64_t)k * 2 * nchans + i];
    acc[i] = a;
}

// Which channels a workgroup of dedisp_sum_kernel sums, its last argument.
// DdAllChans (empty: the plain call) is every channel, grid (time tiles, DM
// tiles), out[d * out_stride + t].  DdBandTable (rt_dedisperse_bands_device)
// is the channels [lo, hi) of band blockIdx.z of uint32 bands[nbands][2], a
// grid layer per band, out[(d * nbands + b) * out_stride + t]; the edges are
// clamped as they are read, hi to nchans and lo to hi, so a band of any two
// numbers reads rows of the workspace only.  An empty band, or one whose
// channels are all masked, stores zeros.
struct DdAllChans {};
struct DdBandTable {
    const uint32_t* bands;
    uint32_t nbands;
};

// T = uint8_t (signed samples biased by 128: bias = 128) or float.  pitch is
// in elements.  Lane l of a wave owns the outputs t0 + 4 l + j (8-bit) or
// t0 + l + 64 j (float), j = 0..3, of each of the wave's four DMs.  nsum,
// which the 8-bit bias correction multiplies, counts the channels summed by
// this workgroup: those of its band, not of the file.
template <class T, class Sel = DdAllChans>
__global__ __launch_bounds__(kDdThreads) void dedisp_sum_kernel(
    const T* __restrict__ ws, uint64_t pitch, uint32_t nchans, const int32_t* __restrict__ delays,
    const uint8_t* __restrict__ mask, uint32_t ndm, uint32_t max_delay, uint32_t nout, float* __restrict__ out,
    uint64_t out_stride, int32_t bias, Sel sel)
{
    uint32_t c_lo = 0, c_hi = nchans;
    uint64_t row_stride = out_stride;
    if constexpr (std::is_same<Sel, DdBandTable>::value) {
        const uint32_t b = blockIdx.z;
        c_hi = min(sel.bands[2 * b + 1], nchans);
        c_lo = min(sel.bands[2 * b], c_hi);
        out += (uint64_t)b * out_stride;
        row_stride = (uint64_t)sel.nbands * out_stride;
    }
    constexpr bool kBytes = sizeof(T) == 1;
    constexpr uint32_t kE = 4 / sizeof(T);   // elements per dword
    constexpr uint32_t kSpan = DdSpan<T>::dwords;
    using Acc = typename std::conditional<kBytes, int32_t, float>::type;
    __shared__ uint32_t span[kDdChans][kSpan + 1];   // + 1: the high dword of an aligned last read
    __shared__ int32_t sdel[kDdDms][kDdChans];
    __shared__ uint32_t sbase[kDdChans];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t t0 = blockIdx.x * kDdTile;
    const uint32_t d0 = blockIdx.y * kDdDms;
    const uint32_t row_dw = (uint32_t)(pitch / kE);
    Acc acc[kDdPerWave][4];
#pragma unroll
    for (uint32_t r = 0; r < kDdPerWave; ++r)
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) acc[r][j] = 0;
    int32_t nsum = 0;

    for (uint32_t c0 = c_lo; c0 < c_hi; c0 += kDdChans) {
        __syncthreads();   // the previous step's spans and delays are consumed
        {
            // the tile's delays: rows past ndm repeat the last DM (never stored)
            const uint32_t dd = tid >> 4, cc = tid & 15;
            const uint32_t d = min(d0 + dd, ndm - 1), c = c0 + cc;
            int32_t v = 0;
            if (c < c_hi) v = min(max(delays[(uint64_t)d * nchans + c], 0), (int32_t)max_delay);
            sdel[dd][cc] = v;
        }
        __syncthreads();
        for (uint32_t cc = wave; cc < kDdChans; cc += kDdWaves) {
            const uint32_t c = c0 + cc;
            if (c >= c_hi || (mask && mask[c])) {
                if (lane == 0) sbase[cc] = kDdSkip;
                continue;
            }
            // smallest and largest delay of the tile's 16 DMs: 16 broadcast
            // LDS reads, the same in every lane (a cross-lane butterfly over
            // one read per lane measured 4 % slower for the whole call)
            int32_t lo = sdel[0][cc], hi = lo;
#pragma unroll
            for (uint32_t dd = 1; dd < kDdDms; ++dd) {
                lo = min(lo, sdel[dd][cc]);
                hi = max(hi, sdel[dd][cc]);
            }
            // first element staged, dwords up to one past the last element read, and whether they fit
            const DedispSpan sp = dedisp_span(sizeof(T), t0 + (uint32_t)lo, t0 + (uint32_t)hi);
            const uint32_t e0 = sp.first, ndw = sp.ndw;
            if (sp.direct) {
                if (lane == 0) sbase[cc] = kDdDirect;
                continue;
            }
            const uint32_t* row = reinterpret_cast<const uint32_t*>(ws + (uint64_t)c * pitch);
            const uint32_t w0 = e0 / kE;
            for (uint32_t i = lane; i < ndw; i += 64) {
                const uint32_t w = w0 + i;
                span[cc][i] = w < row_dw ? row[w] : 0u;
            }
            if (lane == 0) sbase[cc] = e0;
        }
        __syncthreads();

        uint32_t pe[kDdPerWave], po[kDdPerWave];   // 8-bit: 16-bit partial sums of outputs (0, 2) and (1, 3)
#pragma unroll
        for (uint32_t r = 0; r < kDdPerWave; ++r) pe[r] = po[r] = 0;
        for (uint32_t cc = 0; cc < kDdChans; ++cc) {
            const uint32_t base = __builtin_amdgcn_readfirstlane(sbase[cc]);
            if (base == kDdSkip) continue;
            ++nsum;
            if (base == kDdDirect) {
                const T* row = ws + (uint64_t)(c0 + cc) * pitch;
#pragma unroll
                for (uint32_t r = 0; r < kDdPerWave; ++r) {
                    const uint32_t del = (uint32_t)__builtin_amdgcn_readfirstlane(sdel[wave * kDdPerWave + r][cc]);
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) {
                        const uint64_t e = (uint64_t)t0 + del + (kBytes ? lane * 4 + j : lane + 64 * j);
                        acc[r][j] += e < pitch ? (Acc)row[e] : (Acc)0;
                    }
                }
                continue;
            }
#pragma unroll
            for (uint32_t r = 0; r < kDdPerWave; ++r) {
                const uint32_t del = (uint32_t)__builtin_amdgcn_readfirstlane(sdel[wave * kDdPerWave + r][cc]);
                const uint32_t p = t0 + del - base;   // element of output t0 in the span
                if constexpr (kBytes) {
                    const uint32_t w = (p >> 2) + lane;
                    const uint32_t v = __builtin_amdgcn_alignbyte(span[cc][w + 1], span[cc][w], p & 3);
                    pe[r] += v & 0x00FF00FFu;
                    po[r] += (v >> 8) & 0x00FF00FFu;
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) acc[r][j] += __uint_as_float(span[cc][p + lane + 64 * j]);
                }
            }
        }
        if constexpr (kBytes) {   // at most 16 x 255 per 16-bit field
#pragma unroll
            for (uint32_t r = 0; r < kDdPerWave; ++r) {
                acc[r][0] += (int32_t)(pe[r] & 0xFFFFu);
                acc[r][1] += (int32_t)(po[r] & 0xFFFFu);
                acc[r][2] += (int32_t)(pe[r] >> 16);
                acc[r][3] += (int32_t)(po[r] >> 16);
            }
        }
    }

#pragma unroll
    for (uint32_t r = 0; r < kDdPerWave; ++r) {
        const uint32_t d = d0 + wave * kDdPerWave + r;
        if (d >= ndm) continue;
        float* o = out + (uint64_t)d * row_stride;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t t = t0 + (kBytes ? lane * 4 + j : lane + 64 * j);
            if (t >= nout) continue;
            if constexpr (kBytes) o[t] = (float)(acc[r][j] - bias * nsum);
            else o[t] = acc[r][j];
        }
    }
}

// ---- time decimation of the transposed rows (launch_dedisperse_steps)
// z[c, u] = sum over i < f of row_c[f u + i] for u < nz = floor(nsamp_blk / f),
// float32 rows of pitch zpitch (a multiple of 4 floats); [nz, zpitch) is
// written as zero.  T = uint8_t: 8-bit rows, summed in int32, the bias removed
// (bias * f) and converted once.  T = float: float32 additions from 0.0f in
// index order.  Reading the transposed rows, it needs no form per packed type,
// block mask or zero-DM filter: those stay in the transposes.
// A workgroup takes 256 outputs of one channel, a wave 64 of them: the 64 f
// contiguous elements from element 64 f (u0 / 64) of the row, a stretch that
// starts on a 64-byte boundary.  When an output's f elements are 4, 8 or a
// multiple of 16 bytes, lane l loads its own chunk with dword, 2-dword or
// 4-dword loads (aligned: the row pitch is a multiple of 16 bytes) -- at 4, 8
// and 16 bytes one instruction of the wave covers the whole stretch.  Any
// other f goes through LDS: the wave loads the stretch with coalesced dword
// loads, kDcStageDw dwords at a time, and every lane adds the elements of its
// chunk that lie in the piece, so no lane issues f byte loads.
// No load leaves the row's padded pitch: a chunk is loaded only for u < nz
// (f u + f <= nsamp_blk <= pitch) and the staged dwords are clamped to the
// pitch; no store goes past zpitch.
// kStaged is the launcher's choice by f (dc_staged): the staged form alone
// holds the 16 KiB of LDS, the vector-load form none.
constexpr uint32_t kDcTile = 256;        // outputs of a workgroup
constexpr uint32_t kDcStageDw = 1024;    // dwords of a wave's staged piece

template <class T, class Acc>
__device__ inline void dc_add_dword(Acc& acc, uint32_t v)
{
    if constexpr (sizeof(T) == 1) acc += (Acc)((v & 0xFFu) + ((v >> 8) & 0xFFu) + ((v >> 16) & 0xFFu) + (v >> 24));
    else acc += __uint_as_float(v);
}

// whether a chunk of cb bytes goes through LDS: not 4, 8 or a multiple of 16 bytes
constexpr bool dc_staged(uint32_t cb) { return cb % 16 != 0 && cb != 8 && cb != 4; }

template <class T, bool kStaged>
__global__ __launch_bounds__(kDdThreads) void dedisp_decimate_kernel(
    const T* __restrict__ ws, uint64_t pitch, uint32_t nchans, uint32_t f, uint32_t nz, float* __restrict__ z,
    uint64_t zpitch, int32_t bias)
{
    constexpr bool kBytes = sizeof(T) == 1;
    constexpr uint32_t kE = 4 / sizeof(T);   // elements per dword
    using Acc = typename std::conditional<kBytes, int32_t, float>::type;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t u0 = blockIdx.x * kDcTile + wave * 64;   // the wave's first output
    const uint32_t u = u0 + lane;
    const uint32_t cb = f * (uint32_t)sizeof(T);            // bytes of an output's chunk
    [[maybe_unused]] const uint64_t row_dw = pitch / kE;
    for (uint32_t c = blockIdx.y; c < nchans; c += gridDim.y) {
        const T* row = ws + (uint64_t)c * pitch;
        Acc acc = 0;
        if constexpr (kStaged) {
            __shared__ __attribute__((aligned(16))) uint32_t stage[kDdWaves][kDcStageDw];
            const uint32_t* rdw = reinterpret_cast<const uint32_t*>(row);
            const uint64_t w0 = (uint64_t)u0 * cb / 4;    // u0 is a multiple of 64: a whole dword
            const uint32_t ndw = 16 * cb;                 // dwords of the wave's stretch, 64 cb / 4
            const uint32_t e_lo = lane * f, e_hi = e_lo + f;   // the lane's elements of the stretch
            for (uint32_t p0 = 0; p0 < ndw; p0 += kDcStageDw) {
                __syncthreads();   // the previous piece is consumed
                const uint32_t n = min(kDcStageDw, ndw - p0);
                for (uint32_t i = lane; i < n; i += 64) {
                    const uint64_t w = w0 + p0 + i;
                    stage[wave][i] = w < row_dw ? rdw[w] : 0u;
                }
                __syncthreads();
                const uint32_t s0 = p0 * kE;   // first element of the piece
                const uint32_t lo = max(e_lo, s0), hi = min(e_hi, s0 + n * kE);
                for (uint32_t e = lo; e < hi; ++e) {
                    if constexpr (kBytes) acc += (Acc) reinterpret_cast<const uint8_t*>(stage[wave])[e - s0];
                    else acc += __uint_as_float(stage[wave][e - s0]);
                }
            }
        } else if (cb % 16 == 0) {   // the same in every workgroup
            if (u < nz) {
                const uint4* p = reinterpret_cast<const uint4*>(row + (uint64_t)u * f);
                for (uint32_t k = 0; k < cb / 16; ++k) {
                    const uint4 v = p[k];
                    dc_add_dword<T>(acc, v.x);
                    dc_add_dword<T>(acc, v.y);
                    dc_add_dword<T>(acc, v.z);
                    dc_add_dword<T>(acc, v.w);
                }
            }
        } else if (cb == 8) {
            if (u < nz) {
                const uint2 v = *reinterpret_cast<const uint2*>(row + (uint64_t)u * f);
                dc_add_dword<T>(acc, v.x);
                dc_add_dword<T>(acc, v.y);
            }
        } else {   // cb == 4
            if (u < nz) dc_add_dword<T>(acc, *reinterpret_cast<const uint32_t*>(row + (uint64_t)u * f));
        }
        if (u < zpitch) {
            float v = 0.0f;
            if (u < nz) {
                if constexpr (kBytes) v = (float)(acc - bias * (int32_t)f);
                else v = acc;
            }
            z[(uint64_t)c * zpitch + u] = v;
        }
    }
}

// the sum over the transposed rows: the plain instantiation, or with a band
// table the band one on a grid with a z layer per band
template <class T>
void launch_sum(dim3 grid, hipStream_t s, const T* ws, uint64_t pitch, uint32_t nchans, const int32_t* delays,
                const uint8_t* mask, uint32_t ndm, uint32_t max_delay, uint32_t nout, float* out, uint64_t out_stride,
                int32_t bias, const uint32_t* bands, uint32_t nbands)
{
    if (bands) {
        grid.z = nbands;
        hipLaunchKernelGGL((dedisp_sum_kernel<T, DdBandTable>), grid, dim3(kDdThreads), 0, s, ws, pitch, nchans, delays,
                           mask, ndm, max_delay, nout, out, out_stride, bias, DdBandTable{bands, nbands});
    } else {
        hipLaunchKernelGGL((dedisp_sum_kernel<T, DdAllChans>), grid, dim3(kDdThreads), 0, s, ws, pitch, nchans, delays,
                           mask, ndm, max_delay, nout, out, out_stride, bias, DdAllChans{});
    }
}

// f(tag), tag a value of the T that kernels reading rows of this sample type
// code are instantiated for: the one dispatch on the sample type
template <class F>
void dd_dispatch(int dtype, F f)
{
    switch (dtype) {
    case RT_DEDISP_U1: f(DdBits<1>{}); break;
    case RT_DEDISP_U2: f(DdBits<2>{}); break;
    case RT_DEDISP_U4: f(DdBits<4>{}); break;
    case RT_DEDISP_U16: f(DdBits<16>{}); break;
    case RT_DEDISP_U8: f(uint8_t{}); break;
    case RT_DEDISP_I8: f(int8_t{}); break;
    default: f(float{}); break;
    }
}

// f(cells), cells the last argument of a kernel reading the block: no block
// mask is DdNoCells, the plain instantiation
template <class F>
void dd_cells(const DedispCells* bm, F f)
{
    if (bm) f(*bm);
    else f(DdNoCells{});
}

}  // namespace

uint64_t dedisp_pitch_bytes(int dtype, uint64_t nsamp_blk)
{
    const uint64_t esize = dtype == RT_DEDISP_F32 || dtype == RT_DEDISP_U16 ? 4 : 1;
    return (nsamp_blk * esize + 15) / 16 * 16;
}

uint64_t dedisp_workspace_bytes(int dtype, uint64_t nsamp_blk, uint64_t nchans, uint32_t flags)
{
    if (flags & RT_DEDISP_ZERO_DM)   // float rows, then m
        return dedisp_pitch_bytes(RT_DEDISP_F32, nsamp_blk) * (nchans + 1);
    return dedisp_pitch_bytes(dtype, nsamp_blk) * nchans;
}

hipError_t launch_zero_dm_mean(const void* block, int dtype, uint32_t nsamp_blk, uint32_t nchans,
                               const uint8_t* d_mask, float* m, hipStream_t s, const DedispCells* bm)
{
    const dim3 grid((nsamp_blk + kRmRowsPerWg - 1) / kRmRowsPerWg);
    dd_dispatch(dtype, [&](auto tag) {
        using T = decltype(tag);
        dd_cells(bm, [&](auto cells) {
            hipLaunchKernelGGL((dedisp_rowmean_kernel<T, decltype(cells)>), grid, dim3(kDdThreads), 0, s,
                               (const T*)block, nsamp_blk, nchans, d_mask, m, cells);
        });
    });
    return hipGetLastError();
}

uint64_t chanstats_workspace_bytes(uint64_t nsamp_blk, uint64_t nchans)
{
    return (nsamp_blk + kCsChunk - 1) / kCsChunk * 2 * nchans * sizeof(double);
}

hipError_t launch_channel_stats(const void* block, int dtype, uint32_t nsamp_blk, uint32_t nchans, double* acc,
                                void* ws, hipStream_t s)
{
    const uint32_t nchunks = (nsamp_blk + kCsChunk - 1) / kCsChunk;
    const dim3 grid(nchunks, (nchans + 63) / 64);
    double* part = (double*)ws;
    dd_dispatch(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(dedisp_chanstats_kernel<T>, grid, dim3(kDdThreads), 0, s, (const T*)block, nsamp_blk,
                           nchans, part);
    });
    hipLaunchKernelGGL(dedisp_chanstats_fold_kernel, dim3((2 * nchans + kDdThreads - 1) / kDdThreads),
                       dim3(kDdThreads), 0, s, (const double*)part, nchunks, nchans, acc);
    return hipGetLastError();
}

// chunks of one block, and of the whole call (the grid's x: the caller keeps it below 2^31)
uint64_t blockstats_chunks(uint64_t nsamp_blk, uint64_t block_len)
{
    const uint64_t cpb = (block_len + kCsChunk - 1) / kCsChunk;
    return (nsamp_blk + block_len - 1) / block_len * cpb;
}

uint64_t blockstats_workspace_bytes(uint64_t nsamp_blk, uint64_t nchans, uint64_t block_len)
{
    if (block_len <= kCsChunk) return 0;   // a block is one chunk: written in place
    return blockstats_chunks(nsamp_blk, block_len) * 2 * nchans * sizeof(double);
}

hipError_t launch_block_stats(const void* block, int dtype, uint32_t nsamp_blk, uint32_t nchans, uint32_t block_len,
                              double* stats, void* ws, hipStream_t s)
{
    const uint32_t cpb = (uint32_t)(((uint64_t)block_len + kCsChunk - 1) / kCsChunk);
    const uint32_t nchunks = (uint32_t)blockstats_chunks(nsamp_blk, block_len);
    const dim3 grid(nchunks, (nchans + 63) / 64);
    double* dst = cpb == 1 ? stats : (double*)ws;
    dd_dispatch(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(dedisp_blockstats_kernel<T>, grid, dim3(kDdThreads), 0, s, (const T*)block, nsamp_blk,
                           nchans, block_len, cpb, dst);
    });
    if (cpb > 1) {
        const uint64_t total = (uint64_t)(nchunks / cpb) * 2 * nchans;
        hipLaunchKernelGGL(dedisp_blockstats_fold_kernel, dim3((uint32_t)((total + kDdThreads - 1) / kDdThreads)),
                           dim3(kDdThreads), 0, s, (const double*)ws, cpb, total, nchans, stats);
    }
    return hipGetLastError();
}

// The first step of launch_dedisperse, alone (launch_pulse_cutouts of
// cutout_kernels.hip reads the same rows): the block to channel-major rows in
// the workspace -- float32 rows for float and 16-bit data and for every type
// under the zero-DM filter (x - m, m behind the rows), 8-bit rows otherwise
// (signed samples biased by 128, 1/2/4-bit samples unpacked).  With a block
// mask the kernels are the DdCells instantiations: the workspace then holds x'
// (or x' - m).
hipError_t launch_dedisp_rows(const void* block, int dtype, uint32_t nsamp_blk, uint32_t nchans,
                              const uint8_t* d_mask, void* ws, uint32_t flags, hipStream_t s, const DedispCells* bm)
{
    const int nbits = dedisp_packed_bits(dtype);
    const bool zero_dm = flags & RT_DEDISP_ZERO_DM;
    const uint64_t pitch_bytes = dedisp_pitch_bytes(dedisp_float_rows(dtype, flags) ? RT_DEDISP_F32 : dtype, nsamp_blk);
    if (dedisp_float_rows(dtype, flags)) {
        const uint64_t pitch = pitch_bytes / 4;
        const dim3 grid((uint32_t)((pitch + 63) / 64), (nchans + 63) / 64);
        if (zero_dm) {
            float* m = (float*)ws + pitch * nchans;
            const hipError_t e = launch_zero_dm_mean(block, dtype, nsamp_blk, nchans, d_mask, m, s, bm);
            if (e != hipSuccess) return e;
            dd_dispatch(dtype, [&](auto tag) {
                using T = decltype(tag);
                dd_cells(bm, [&](auto cells) {
                    hipLaunchKernelGGL((dedisp_transpose_zdm_kernel<T, true, decltype(cells)>), grid, dim3(kDdThreads),
                                       0, s, (const T*)block, nsamp_blk, nchans, (const float*)m, (float*)ws, pitch,
                                       cells);
                });
            });
        } else if (nbits == 16) {   // exact float32 values
            dd_cells(bm, [&](auto cells) {
                hipLaunchKernelGGL((dedisp_transpose_zdm_kernel<DdBits<16>, false, decltype(cells)>), grid,
                                   dim3(kDdThreads), 0, s, (const DdBits<16>*)block, nsamp_blk, nchans,
                                   (const float*)nullptr, (float*)ws, pitch, cells);
            });
        } else {
            dd_cells(bm, [&](auto cells) {
                hipLaunchKernelGGL(dedisp_transpose32_kernel<decltype(cells)>, grid, dim3(kDdThreads), 0, s,
                                   (const float*)block, nsamp_blk, nchans, (float*)ws, pitch, cells);
            });
        }
    } else if (nbits) {   // the values themselves: no bias
        const uint32_t row_bytes = (uint32_t)((uint64_t)nchans * nbits / 8);
        const uint32_t dwords = row_bytes % 4 == 0 && (uintptr_t)block % 4 == 0;
        const dim3 grid((uint32_t)((pitch_bytes + 255) / 256), (row_bytes + 63) / 64);
        const auto unpack = [&](auto tag) {
            dd_cells(bm, [&](auto cells) {
                hipLaunchKernelGGL((dedisp_unpack_transpose_kernel<decltype(tag)::kBits, decltype(cells)>), grid,
                                   dim3(kDdThreads), 0, s, (const uint8_t*)block, nsamp_blk, nchans, row_bytes,
                                   (uint8_t*)ws, pitch_bytes, dwords, cells);
            });
        };
        if (nbits == 1) unpack(DdBits<1>{});
        else if (nbits == 2) unpack(DdBits<2>{});
        else unpack(DdBits<4>{});
    } else {
        const dim3 grid((uint32_t)((pitch_bytes + 255) / 256), (nchans + 63) / 64);
        dd_cells(bm, [&](auto cells) {
            hipLaunchKernelGGL(dedisp_transpose8_kernel<decltype(cells)>, grid, dim3(kDdThreads), 0, s,
                               (const uint8_t*)block, nsamp_blk, nchans, (uint8_t*)ws, pitch_bytes,
                               dtype == RT_DEDISP_I8 ? 0x80u : 0u, cells);
        });
    }
    return hipGetLastError();
}

// Two steps.  The block goes to channel-major rows in the workspace
// (launch_dedisp_rows).  Then one sum over whichever rows they are.
hipError_t launch_dedisperse(const void* block, int dtype, uint32_t nsamp_blk, uint32_t nchans,
                             const int32_t* d_delays, const uint8_t* d_mask, uint32_t ndm, uint32_t max_delay,
                             float* out, uint64_t out_stride, void* ws, uint32_t flags, hipStream_t s,
                             const uint32_t* d_bands, uint32_t nbands, const DedispCells* bm)
{
    const uint32_t nout = nsamp_blk - max_delay;
    const bool float_rows = dedisp_float_rows(dtype, flags);
    const uint64_t pitch_bytes = dedisp_pitch_bytes(float_rows ? RT_DEDISP_F32 : dtype, nsamp_blk);
    const dim3 sum_grid((nout + kDdTile - 1) / kDdTile, (ndm + kDdDms - 1) / kDdDms);
    const hipError_t e = launch_dedisp_rows(block, dtype, nsamp_blk, nchans, d_mask, ws, flags, s, bm);
    if (e != hipSuccess) return e;
    if (float_rows)
        launch_sum(sum_grid, s, (const float*)ws, pitch_bytes / 4, nchans, d_delays, d_mask, ndm, max_delay, nout, out,
                   out_stride, 0, d_bands, nbands);
    else
        launch_sum(sum_grid, s, (const uint8_t*)ws, pitch_bytes, nchans, d_delays, d_mask, ndm, max_delay, nout, out,
                   out_stride, dtype == RT_DEDISP_I8 ? 128 : 0, d_bands, nbands);
    return hipGetLastError();
}

uint64_t dedisp_steps_workspace_bytes(int dtype, uint64_t nsamp_blk, uint64_t nchans, uint32_t flags,
                                      uint32_t min_factor)
{
    const uint64_t rows = dedisp_workspace_bytes(dtype, nsamp_blk, nchans, flags);   // a multiple of 16
    if (!min_factor) return rows;
    return rows + dedisp_pitch_bytes(RT_DEDISP_F32, nsamp_blk / min_factor) * nchans;
}

// The rows once, then step after step in stream order: a step of downsamp 1
// is launch_dedisperse's sum of those rows; any other decimates them into the
// float32 area behind them, which the step before has finished reading, and
// runs the float32 sum over that area with the step's own pitch.
hipError_t launch_dedisperse_steps(const void* block, int dtype, uint32_t nsamp_blk, uint32_t nchans,
                                   const int32_t* d_delays, const uint8_t* d_mask, const rt_dedisp_step* steps,
                                   size_t nsteps, float* out, void* ws, uint32_t flags, hipStream_t s,
                                   const DedispCells* bm)
{
    const bool float_rows = dedisp_float_rows(dtype, flags);
    const uint64_t pitch_bytes = dedisp_pitch_bytes(float_rows ? RT_DEDISP_F32 : dtype, nsamp_blk);
    const int32_t bias = !float_rows && dtype == RT_DEDISP_I8 ? 128 : 0;
    float* z = reinterpret_cast<float*>(static_cast<uint8_t*>(ws) + dedisp_workspace_bytes(dtype, nsamp_blk, nchans, flags));
    const hipError_t e = launch_dedisp_rows(block, dtype, nsamp_blk, nchans, d_mask, ws, flags, s, bm);
    if (e != hipSuccess) return e;
    for (size_t k = 0; k < nsteps; ++k) {
        const rt_dedisp_step& st = steps[k];
        const int32_t* delays = d_delays + st.delays_off;
        float* o = out + st.out_off + st.out_offset;
        const uint32_t f = st.downsamp, nz = nsamp_blk / f, nout = nz - st.max_delay;
        const dim3 sum_grid((nout + kDdTile - 1) / kDdTile, (st.ndm + kDdDms - 1) / kDdDms);
        if (f == 1) {
            if (float_rows)
                launch_sum(sum_grid, s, (const float*)ws, pitch_bytes / 4, nchans, delays, d_mask, st.ndm,
                           st.max_delay, nout, o, st.out_stride, 0, nullptr, 0);
            else
                launch_sum(sum_grid, s, (const uint8_t*)ws, pitch_bytes, nchans, delays, d_mask, st.ndm, st.max_delay,
                           nout, o, st.out_stride, bias, nullptr, 0);
            continue;
        }
        const uint64_t zpitch = dedisp_pitch_bytes(RT_DEDISP_F32, nz) / 4;
        const dim3 grid((uint32_t)((zpitch + kDcTile - 1) / kDcTile), nchans < 65535u ? nchans : 65535u);
        const auto decimate = [&](auto staged) {
            constexpr bool kStaged = decltype(staged)::value;
            if (float_rows)
                hipLaunchKernelGGL((dedisp_decimate_kernel<float, kStaged>), grid, dim3(kDdThreads), 0, s,
                                   (const float*)ws, pitch_bytes / 4, nchans, f, nz, z, zpitch, 0);
            else
                hipLaunchKernelGGL((dedisp_decimate_kernel<uint8_t, kStaged>), grid, dim3(kDdThreads), 0, s,
                                   (const uint8_t*)ws, pitch_bytes, nchans, f, nz, z, zpitch, bias);
        };
        if (dc_staged(f * (float_rows ? 4u : 1u))) decimate(std::true_type{});
        else decimate(std::false_type{});
        launch_sum(sum_grid, s, (const float*)z, zpitch, nchans, delays, d_mask, st.ndm, st.max_delay, nout, o,
                   st.out_stride, 0, nullptr, 0);
    }
    return hipGetLastError();
}

}  // namespace rt
