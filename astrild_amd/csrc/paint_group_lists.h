// The wave-private LDS lists of the paint's grouping kernel (mesh_paint_tiled.hip, tile_group_kernel): how many
// entries a wave's slice holds, and where entry e of the four slices taken as ONE list lies.  Plain integer code,
// compiled for the device by the kernel and for the host by tests/host/paint_group_lists_test.cpp.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AST_GROUP_HD __host__ __device__
#else
#define AST_GROUP_HD
#endif

namespace ast {

constexpr int GROUP_WAVES = 4;      // waves of a grouping workgroup

// Group records one wave can make per interval: it looks at `slots` particle slots (trips x particles per thread) of two
// 32-particle windows each, and a window gets at most `iters` records.  A slice of this size is never full.
AST_GROUP_HD constexpr uint32_t wave_record_capacity(int slots, int iters) { return (uint32_t)(slots * 2 * iters); }

// Entry e < c0 + c1 + c2 + c3 of the four slices [w * cap, w * cap + c_w) taken as one list -> its index in LDS.
// e1 = c0, e2 = c0 + c1, e3 = c0 + c1 + c2 (prefix sums, every c_w <= cap).
AST_GROUP_HD inline uint32_t slice_entry(uint32_t e, uint32_t e1, uint32_t e2, uint32_t e3, uint32_t cap) {
    // (unsigned wrap-around is meant: cap * w - e_w may be "negative", the sum is not)
    return e + (e >= e3 ? 3u * cap - e3 : e >= e2 ? 2u * cap - e2 : e >= e1 ? cap - e1 : 0u);
}

}  // namespace ast
