// What the entry points of the two crossing searches, csrc/surface_crossings.hip and csrc/scene_crossings.hip, share on the host: the
// argument rules of their count-or-emit passes and the launch of a test kernel's two forms.  (On the device they share the per-pair
// statements, csrc/surface_crossings_shared.h, and the workgroup passes, csrc/wg_device.h.  The test kernels stay two, and keep their own
// triangle load, emit slot and count epilogue: their staged records, self-pair rules, keys and row guards differ, and their instruction
// streams are pinned by profiles/crossings_commons_isa.txt.)
#pragma once
#include "psi_common.h"
#include "wg_device.h"

// psi_*_crossings_tiles: the count pass takes neither the offsets nor the table, the emit pass both and the table's rows
#define SC_REQUIRE_TILE_PASS(d_job_off, n_tiles, d_tiles)                                                                                   \
    PSI_REQUIRE((d_tiles == nullptr) == (d_job_off == nullptr), "the emit pass takes d_job_off and d_tiles, the count pass neither");      \
    PSI_REQUIRE(d_tiles ? (n_tiles >= 1 && n_tiles < (1ll << 31)) : n_tiles == 0, "1 <= n_tiles < 2^31 to emit, 0 to count")

// psi_*_crossings_test: d_keys decides the pass.  batch_rule: the search's own rule on B, checked between the two as it always was (the
// order decides which message a doubly wrong call gets)
#define SC_REQUIRE_TEST_PASS(n_tiles, batch_rule, d_tile_off, n_pairs, d_keys, d_events, d_length)                                          \
    PSI_REQUIRE(n_tiles >= 1 && n_tiles < (1ll << 31), "1 <= n_tiles < 2^31");                                                              \
    batch_rule;                                                                                                                             \
    PSI_REQUIRE(d_keys ? (d_tile_off && d_events && d_length && n_pairs >= 1 && n_pairs < (1ll << 31))                                      \
                       : (!d_tile_off && !d_events && !d_length && n_pairs == 0),                                                           \
                "the emit pass takes d_tile_off, d_keys, d_events, d_length and 1 <= n_pairs < 2^31; the count pass none of them")

// kernel<true> with d_keys, else kernel<false>, one workgroup per tile, from one argument list (the rules above make the emit arguments of
// a count pass null and zero)
#define SC_LAUNCH_TEST(kernel, n_tiles, stream, d_keys, ...)                                                                                \
    do {                                                                                                                                    \
        if (d_keys) hipLaunchKernelGGL(kernel<true>, dim3((unsigned)(n_tiles)), dim3(WG_LANES), 0, (hipStream_t)(stream), __VA_ARGS__);     \
        else hipLaunchKernelGGL(kernel<false>, dim3((unsigned)(n_tiles)), dim3(WG_LANES), 0, (hipStream_t)(stream), __VA_ARGS__);           \
    } while (0)
