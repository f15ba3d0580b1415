// The tile binning of the two rasterisers, one copy: raster.hip (scene snapshots) and raster_bodies.hip (bodies drawn into them) set their
// pieces up themselves (records, packed tile boxes, per-tile counts through count_box_tiles) and rasterise the bins themselves; what lies
// between is here:
//   for_each_tile    the tiles of a packed tile box (raster_device.h: pack_box)
//   rs_fill_kernel   one lane per (row, piece slot): the slot's bin entry into every tile of its box (integer atomic cursor)
//   BinLayout        the workspace regions of the binning, and where a caller's own regions go among them
//   rs_bin_pass      the host sequence of one call or pass: rs_scan -> rs_view_base -> the ONE stream synchronisation with the read-back of
//                    the pair counts -> refusals -> the bins (the workspace's, or the handle's grown ones) -> rs_fill
// Header-inline, so that a host program that compiles one of the two files alone sees it (tools/result_images_host_check.hip).
#pragma once
#include "raster_device.h"
#include <vector>

namespace {

// fn(ty * tiles_x + tx) for every tile of a packed tile box, row by row
template <typename Fn>
__device__ __forceinline__ void for_each_tile(unsigned box, int tiles_x, Fn fn)
{
    const int tx0 = box & 255, ty0 = (box >> 8) & 255, tx1 = (box >> 16) & 255, ty1 = box >> 24;
    for (int ty = ty0; ty <= ty1; ty++)
        for (int tx = tx0; tx <= tx1; tx++) fn(ty * tiles_x + tx);
}

// the count loop of a setup kernel: one more piece in every tile of the box
__device__ __forceinline__ void count_box_tiles(unsigned box, int view, int tiles_x, int ntiles, int *__restrict__ tcount)
{
    for_each_tile(box, tiles_x, [&](int t) { atomicAdd(&tcount[(size_t)view * ntiles + t], 1); });
}

// A row is `slots` piece slots with one view: view `row` itself (draw_view == nullptr: the snapshots, whose tile kernel reads a view's
// records from the view's own base), or the view of draw d0 + row of a pass (the bodies, whose tile kernel reads the pass's records from one
// base).  The bin entry follows the tile kernel: the slot within the row for the first, within the pass for the second.  They are not
// unified: the snapshots' n_views * slots can reach 65535 * 2^30, beyond a 32-bit entry.  The order inside a bin is free.
__global__ __launch_bounds__(256) void rs_fill_kernel(int slots, const int *__restrict__ draw_view, int d0, int tiles_x, int ntiles,
                                                      const unsigned *__restrict__ pbox, const int *__restrict__ toff, const long long *__restrict__ vbase,
                                                      int *__restrict__ tcursor, int *__restrict__ bins)
{
    const int row = blockIdx.y;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= slots) return;
    const size_t slot = (size_t)row * slots + s;
    const unsigned box = pbox[slot];
    if (box == NOBOX) return;                                 // every slot of a draw with a bad view is empty
    const int view = draw_view ? draw_view[d0 + row] : row;
    const int entry = draw_view ? (int)slot : s;
    int *base = bins + vbase[view];
    for_each_tile(box, tiles_x, [&](int t) {
        const size_t tile = (size_t)view * ntiles + t;
        const int pos = atomicAdd(&tcursor[tile], 1);
        base[toff[tile] + pos] = entry;
    });
}

// The workspace of the binning: begin() places recs .. vbase for `slots` piece slots and n_views views of W x H pixels, the caller may
// take() regions of its own, place_bins() ends it.  Every region starts on a 256-byte boundary.
struct BinLayout {
    size_t o_recs, o_pbox, o_tcount, o_tcursor, o_toff, o_vbase, o_bins, bytes;
    size_t pair_cap;
    int tiles_x, tiles_y, ntiles;

    size_t take(size_t n)
    {
        const size_t at = bytes;
        bytes += (n + 255) & ~(size_t)255;
        return at;
    }

    void begin(size_t slots, int n_views, int W, int H)
    {
        bytes = 0;
        tiles_x = psi_cdiv(W, TILE);
        tiles_y = psi_cdiv(H, TILE);
        ntiles = tiles_x * tiles_y;
        const size_t vt = (size_t)n_views * ntiles;
        o_recs = take(slots * sizeof(PieceRec));
        o_pbox = take(slots * 4);
        o_tcount = take(vt * 4);             // tcount and tcursor are adjacent: one memset of count_bytes() clears both
        o_tcursor = take(vt * 4);
        o_toff = take(vt * 4);
        o_vbase = take((size_t)n_views * 8);
        // room for the bins: every piece in one tile, plus 64 pieces in every tile (large triangles cover many tiles); a call or pass that
        // needs more takes the bins from the buffer its handle owns (rs_bin_pass)
        pair_cap = slots + (size_t)64 * vt;
    }

    void place_bins() { o_bins = take(pair_cap * 4); }
    size_t count_bytes() const { return o_toff - o_tcount; }
};

struct BinRegions {
    PieceRec *recs;
    unsigned *pbox;
    int *tcount, *tcursor, *toff;
    long long *vbase;
    int *bins;

    BinRegions(const BinLayout &L, char *ws)
        : recs((PieceRec *)(ws + L.o_recs)), pbox((unsigned *)(ws + L.o_pbox)), tcount((int *)(ws + L.o_tcount)), tcursor((int *)(ws + L.o_tcursor)),
          toff((int *)(ws + L.o_toff)), vbase((long long *)(ws + L.o_vbase)), bins((int *)(ws + L.o_bins))
    {
    }
};

// From the per-tile counts of a setup kernel to filled bins, for `rows` rows of `slots` piece slots (rs_fill_kernel) of entry point `who`.
// d_pairs [n_views][2] receives the views' pair counts in its first column.  The bins are sized from the counts: the one host read, which
// also brings the word *d_bad when that is given; a non-zero word refuses the call with bad_msg.  *bins is what the tile kernel reads: the
// workspace's bins, or the handle's bins_extra, enlarged (with 25 % head-room) when they are too small.
int rs_bin_pass(const char *who, const BinLayout &L, const BinRegions &R, RsGrownBins &bins_extra, int n_views, int *d_pairs, const int *d_bad,
                const char *bad_msg, int rows, int slots, const int *d_draw_view, int d0, hipStream_t st, int **bins)
{
    hipLaunchKernelGGL(rs_scan_kernel, dim3(n_views), dim3(256), 0, st, R.tcount, L.ntiles, R.toff, d_pairs);
    PSI_CHECK_LAUNCH("rs_scan_kernel");
    hipLaunchKernelGGL(rs_view_base_kernel, dim3(1), dim3(64), 0, st, d_pairs, n_views, R.vbase);
    PSI_CHECK_LAUNCH("rs_view_base_kernel");
    std::vector<int> h_stats((size_t)n_views * 2);
    int bad = 0;
    PSI_CHECK_HIP(hipMemcpyAsync(h_stats.data(), d_pairs, (size_t)n_views * 8, hipMemcpyDeviceToHost, st));
    if (d_bad) PSI_CHECK_HIP(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    PSI_CHECK_HIP(hipStreamSynchronize(st));
    PSI_REQUIRE(!bad, bad_msg);
    size_t pairs = 0;
    for (int v = 0; v < n_views; v++) {
        PSI_REQUIRE(h_stats[(size_t)v * 2] >= 0, "a view's (tile, piece) pairs exceed 2^31");
        pairs += (size_t)h_stats[(size_t)v * 2];
    }
    *bins = R.bins;
    if (pairs > L.pair_cap) {
        if (bins_extra.bytes < pairs * 4) {
            rs_free_grown_bins(bins_extra);                   // one call at a time per handle (psi_hip.h) and this call's stream is idle: nothing reads the old buffer
            const size_t want = pairs * 4 + pairs;
            hipError_t e = hipMalloc(&bins_extra.ptr, want);
            if (e != hipSuccess) {
                psi_set_error("%s: hipMalloc of %zu bytes for the bins failed: %s", who, want, hipGetErrorString(e));
                return PSI_ENOMEM;
            }
            bins_extra.bytes = want;
        }
        *bins = (int *)bins_extra.ptr;
    }
    hipLaunchKernelGGL(rs_fill_kernel, dim3(psi_cdiv(slots, 256), rows), dim3(256), 0, st, slots, d_draw_view, d0, L.tiles_x, L.ntiles, R.pbox, R.toff,
                       R.vbase, R.tcursor, *bins);
    PSI_CHECK_LAUNCH("rs_fill_kernel");
    return 0;
}

}  // namespace
