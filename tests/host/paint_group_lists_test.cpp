// Stand-alone host check of astrild_amd/csrc/paint_group_lists.h (built with -fsanitize=address,undefined by
// tests/test_paint_group_lists_host.py): the four wave slices walked as one list reach every filled entry exactly
// once, never an unfilled one, never one outside the list - for every combination of fills from a set that holds the
// ends (0, 1, cap - 1, cap) and some in between.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "paint_group_lists.h"

static int check(uint32_t cap, const uint32_t (&c)[4]) {
    std::vector<int> seen(4 * (size_t)cap, 0);
    const uint32_t e1 = c[0], e2 = e1 + c[1], e3 = e2 + c[2], n = e3 + c[3];
    for (uint32_t e = 0; e < n; ++e) {
        const uint32_t k = ast::slice_entry(e, e1, e2, e3, cap);
        if (k >= 4 * cap) { std::printf("cap %u fills %u %u %u %u: entry %u -> %u outside the list\n", cap, c[0], c[1], c[2], c[3], e, k); return 1; }
        ++seen.at(k);
    }
    for (uint32_t w = 0; w < 4; ++w)
        for (uint32_t i = 0; i < cap; ++i)
            if (seen[w * (size_t)cap + i] != (i < c[w] ? 1 : 0)) {
                std::printf("cap %u fills %u %u %u %u: slice %u entry %u visited %d times\n", cap, c[0], c[1], c[2], c[3], w, i, seen[w * (size_t)cap + i]);
                return 1;
            }
    return 0;
}

int main() {
    static_assert(ast::wave_record_capacity(16, 3) == 96, "4 trips x 4 particles per thread, three candidates");
    static_assert(ast::GROUP_WAVES == 4, "slice_entry is written for four slices");
    long cases = 0;
    for (uint32_t cap : {1u, 2u, 96u, 208u, 1024u}) {
        std::vector<uint32_t> fills = {0u, 1u, cap / 3, cap / 2, cap - 1, cap};
        for (uint32_t a : fills) for (uint32_t b : fills) for (uint32_t c : fills) for (uint32_t d : fills) {
            const uint32_t f[4] = {a, b, c, d};
            if (check(cap, f)) return 1;
            ++cases;
        }
    }
    std::printf("paint_group_lists: %ld fill combinations ok\n", cases);
    return 0;
}
