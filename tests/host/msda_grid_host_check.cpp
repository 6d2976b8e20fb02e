// Host-side check of csrc/msda_grid.h, the region-grid chooser of the three encoder window kernels: plain C++, its geometry built
// from the knobs of csrc/msda_tuning.h.  Built for the host by tools/msda_grid_host_check.sh (under -fsanitize=address,undefined by
// hand, plain by tests/test_msda_grid_host.py); no GPU, no HIP header.
#include <stdio.h>

#include "msda_tuning.h"
#include "msda_grid.h"

#define CHECK(cond) \
    do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

// the product's geometry per (kernel, levels), as msda_dispatch.h's configurations put it together
static GridGeom geom(int kernel, int L)
{
    if (kernel == 0) return L == 5 ? grid_geom_of(0, SEMIDETR_RW_RTH5, 16, SEMIDETR_RW_NT5 / 8, 1) : grid_geom_of(0, SEMIDETR_RW_RTH, 16, SEMIDETR_RW_NT / 8, 1);
    if (kernel == 1)
        return L == 5 ? grid_geom_of(1, SEMIDETR_GW_RTH5, SEMIDETR_GW_RTW, (SEMIDETR_GW_NT5 / 64) * 3, 1)
                      : grid_geom_of(1, SEMIDETR_GW_RTH, SEMIDETR_GW_RTW, (SEMIDETR_GW_NT / 64) * 4, 1);
    return grid_geom_of(2, SEMIDETR_SCATTER_RTH, SEMIDETR_SCATTER_RTW, SEMIDETR_SCATTER_Q, 2);
}

static bool same(const GridChoice &a, const GridChoice &b)
{
    return a.nry == b.nry && a.nrx == b.nrx && a.regions == b.regions && a.tail == b.tail && a.max_queries == b.max_queries;
}

static GridChoice ask(int kernel, const int64_t *hs, int L, int N, int M, int cus)
{
    return region_grid_choice(kernel, geom(kernel, L), hs, L, N, M, cus, kernel == 0 && L == 4);
}

static void pin(int kernel, int nry, int nrx) { g_grid_pin[kernel].store(nry << 16 | nrx, std::memory_order_relaxed); }

int main()
{
    static const int64_t tables[5][10] = {{100, 167, 50, 84, 25, 42, 13, 21},
                                          {100, 167, 50, 84, 25, 42, 13, 21, 7, 11},
                                          {9, 13, 5, 7, 3, 4, 2, 2},
                                          {9, 13, 5, 7, 3, 4, 2, 2, 1, 1},
                                          {80, 80, 40, 40, 20, 20, 10, 10}};
    static const int levels[5] = {4, 5, 4, 5, 4};
    static const int batches[4] = {1, 2, 4, 8}, cu_counts[3] = {256, 304, 0};
    const int M = 8;
    int cases = 0;
    for (int kernel = 0; kernel < kGridKernels; ++kernel)
        for (int t = 0; t < 5; ++t)
            for (int N : batches)
                for (int cus : cu_counts) {
                    const int64_t *hs = tables[t];
                    const int L = levels[t];
                    const GridGeom g = geom(kernel, L);
                    int lb = 0;      // the level that carries the grid: level 0, for the scatter the one with the most pixels
                    if (kernel == 2)
                        for (int l = 1; l < L; ++l)
                            if (hs[2 * l] * hs[2 * l + 1] > hs[2 * lb] * hs[2 * lb + 1]) lb = l;
                    const int ny0 = (int)(hs[2 * lb] + g.rth - 1) / g.rth, nx0 = (int)(hs[2 * lb + 1] + g.rtw - 1) / g.rtw;
                    for (int pinned = 0; pinned < 2; ++pinned) {
                        pin(kernel, pinned ? ny0 + 1 : 0, pinned ? nx0 + 1 : 0);
                        const GridChoice c = ask(kernel, hs, L, N, M, cus);
                        CHECK(same(c, ask(kernel, hs, L, N, M, cus)));      // asking twice (the second answer comes from the cache)
                        if (cus == 0) {      // no table: the grid size stays a hint, the kernel gets the pin (or nothing)
                            CHECK(c.regions == 0 && c.max_queries == 0 && !c.tail);
                            CHECK(c.nry == (pinned ? ny0 + 1 : 0) && c.nrx == (pinned ? nx0 + 1 : 0));
                        } else {
                            // (0 x 0: the kernel's own coarsest grid -- the scatter's, which tiles it in steps of rth x rtw)
                            CHECK((c.nry == 0) == (c.nrx == 0) && (c.nry != 0 || (kernel == 2 && !pinned)));
                            const int ny = c.nry ? c.nry : ny0, nx = c.nrx ? c.nrx : nx0;
                            CHECK(ny >= ny0 && nx >= nx0);      // never coarser than the windows allow
                            CHECK(c.regions == ny * nx);
                            CHECK(c.max_queries > 0 && (!c.tail || (kernel == 0 && L == 4)));
                            if (pinned) CHECK(ny == ny0 + 1 && nx == nx0 + 1);
                        }
                        ++cases;
                    }
                    pin(kernel, 0, 0);
                }

    // an answer survives its eviction from the 64-entry cache
    g_grid_cache.clear();
    const int64_t *first_table = tables[0];
    const GridChoice first = ask(0, first_table, 4, 1, M, 256);      // computed, then remembered
    CHECK(g_grid_cache.size() == 1 && first.regions > 0);
    for (int i = 0; i < 70; ++i) {
        const int64_t hs[8] = {101 + i, 167, 50, 84, 25, 42, 13, 21};
        CHECK(ask(0, hs, 4, 1, M, 256).regions > 0);
    }
    CHECK(g_grid_cache.size() == 64);
    for (const GridCacheEntry &e : g_grid_cache) CHECK(!(e.kernel == 0 && e.N == 1 && e.hw[0] == 100 && e.hw[1] == 167));      // gone
    CHECK(same(first, ask(0, first_table, 4, 1, M, 256)));       // computed again ...
    CHECK(g_grid_cache.size() == 64 && same(first, ask(0, first_table, 4, 1, M, 256)));      // ... and remembered again
    g_grid_cache.clear();
    CHECK(same(first, ask(0, first_table, 4, 1, M, 256)));       // a fresh computation

    // eight levels fill the cache entry's 16 words; nine levels, a side above 32766 and no CU count are "no table"
    int64_t deep[18];
    for (int l = 0; l < 9; ++l) {
        deep[2 * l] = 256 >> l;
        deep[2 * l + 1] = 300 >> l;
    }
    for (int kernel = 0; kernel < kGridKernels; ++kernel) {
        const GridChoice c8 = ask(kernel, deep, 8, 2, M, 256);
        CHECK(c8.regions > 0 && c8.max_queries > 0 && same(c8, ask(kernel, deep, 8, 2, M, 256)));
        CHECK(ask(kernel, deep, 9, 2, M, 256).regions == 0);
        CHECK(ask(kernel, deep, 8, 2, M, 0).regions == 0 && ask(kernel, nullptr, 4, 2, M, 256).regions == 0);
        const int64_t huge_h[8] = {32767, 167, 50, 84, 25, 42, 13, 21}, huge_w[8] = {100, 167, 50, 84, 25, 32767, 13, 21};
        const int64_t widest[8] = {32766, 16, 50, 84, 25, 42, 13, 21};
        CHECK(ask(kernel, huge_h, 4, 1, M, 256).regions == 0 && ask(kernel, huge_w, 4, 1, M, 256).regions == 0);
        CHECK(ask(kernel, widest, 4, 1, M, 256).regions > 0);
        pin(kernel, 3, 5);      // without a table a pinned grid is handed to the kernel as it is
        const GridChoice p = ask(kernel, deep, 9, 2, M, 256);
        CHECK(p.regions == 0 && p.nry == 3 && p.nrx == 5);
        pin(kernel, 0, 0);
    }
    printf("msda_grid_host_check: ok (%d cases)\n", cases);
    return 0;
}
