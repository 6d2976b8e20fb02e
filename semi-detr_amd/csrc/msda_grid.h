// The region-grid chooser of the three encoder window kernels: pure host arithmetic with a small cache.  Plain C++ -- no HIP header, no
// knob read from a macro: the kernels' geometry (GridGeom) is handed in by the dispatch (msda_dispatch.h: grid_geom, built from the
// ...Product configurations) and by tests/host/msda_grid_host_check.cpp, which exercises this header alone on a CPU.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <mutex>
#include <vector>

namespace {

// ---- the region grid of the three encoder window kernels, chosen per launch on the host.
// msda_rw_d32, msda_gw_d32 and msda_bwd_scatter_d32_reg cut the finest level into regions, one workgroup per (image, region, head).  The
// windows are sized for regions of up to RTH x RTW pixels, so ceil(H / RTH) x ceil(W / RTW) is the COARSEST grid; any finer one is correct
// too (smaller regions, wider effective margin) and is a launch argument (grid_ry, grid_rx).  One workgroup per CU (the scatter: two) makes
// a launch cost ceil(units / slots) unit times, so where the caller hands over a host copy of the level table (the `_v2` entry points)
// the grid is picked to fill whole waves of workgroups: score = ceil(N * regions * M / slots) * (set-up + rounds(queries of the largest region)).
// Without a table the launch is what it was: the coarsest grid, the grid size a hint.
// Measured (profiles/region_grid_probe.txt, 800 x 1333 pyramid, fused prologue + mask, 256 CUs): launches of one image gain -- forward 4 x 11 with
// the tail split 50.8 -> 4 x 16 without 48.1 us, window gather 7 x 11 -> 8 x 12: the backward 182.5 -> 176.0 us; launches of four images
// (5.5 waves: the workgroups no longer finish in step, the wave count stops mattering and every extra region only adds set-ups) do not --
// forward 4 x 11 159.0, 4 x 12 161.6, 4 x 16 170.8 us; gather 7 x 11 551.7, 8 x 12 562.5 us; and the scatter, bound by its row atomics,
// gains at neither size (one image 13 x 7 175.1, 16 x 8 176.1, 13 x 9 172.6 us; four images every finer grid +2 .. +22 %).
constexpr int kGridKernels = 3;            // SEMIDETR_MSDA_GRID_FORWARD / _GATHER / _SCATTER
constexpr int kGridCap = 8;                // grids of up to this many region rows / columns above the coarsest are scored
constexpr int kGridMaxAxis = 0x7fff;       // a pinned count beyond the level's pixels is legal (regions without a level-0 pixel), up to this
struct GridGeom {
    int rth, rtw;          // the kernel's largest region
    int round;             // queries per round (forward: threads / 8, gather: rows per wave x waves) or per pass (scatter)
    int per_cu;            // workgroups per CU
    float setup;           // a unit's set-up (windows staged, lists built, rows flushed) in units of one full round / pass
    bool even;             // the coarsest grid is tiled evenly (the scatter's steps RTH x RTW and leaves the remainder at the edges)
};
// The set-up shares, fitted to the one-image sweep of profiles/region_grid_probe.txt with rounds counted FRACTIONALLY (a round's cost follows
// the queries in it: 402 queries = 4.2 rounds of 96 cost 3 % more than 374 = 3.9, not a fifth round):
//   forward  0.5 round of 96 (the windows of the coarse levels; also what a part of a split unit pays again, msda_rw.h): unit times 24.0 / 17.2 us
//            at 3.9 / 2.66 rounds -> 5.0 us per round + 2.7 us; the grids rank as measured (4 x 16 < 5 x 12 < 4 x 14 < 4 x 13 < 6 x 16 < 7 x 13)
//   gather   3 rounds of 64 (its windows cover level 0 too, and the far lists are rebuilt per region): 7 x 11 / 8 x 12 / 10 x 12 = 64.8 / 58.3 / 66.2 us
//            against 24.2 / 20.6 / 23.9 model units
//   scatter  0.45 of a 256-query pass (count / scan / fill of the window rows and the flush do not shrink with the region: round 5's 8 x 16
//            regions cost +10 % at bs 4 for 2/3 of the queries) -- not confirmed by the sweep: no grid won, both classes keep the coarsest grid
// What the kernel itself fixes -- largest region, queries per round, workgroups per CU -- comes from its ...Product configuration.
constexpr GridGeom grid_geom_of(int kernel, int rth, int rtw, int round, int per_cu)
{
    if (kernel == 0) return GridGeom{rth, rtw, round, per_cu, 0.5f, true};
    if (kernel == 1) return GridGeom{rth, rtw, round, per_cu, 3.0f, true};
    return GridGeom{rth, rtw, round, per_cu, 0.45f, false};
}
// Which (kernel, launch class) takes a chosen grid: [kernel][0] launches of fewer than three waves of the coarsest grid's units (one image), [1] larger
// ones.  A class whose best grid did not beat the coarsest by more than the run-to-run spread keeps the coarsest grid (profiles/region_grid_probe.txt).
constexpr bool kGridAuto[kGridKernels][2] = {{true, false}, {true, false}, {false, false}};
struct GridChoice {
    int nry = 0, nrx = 0;      // what the kernel is given (0 / 0: its own coarsest grid, tiled as before)
    int regions = 0;           // exact region count of that grid (0: level table unknown, the grid size stays a hint)
    bool tail = false;         // forward, four levels: helper workgroups for the last wave
    int max_queries = 0;       // queries of the largest region (0: unknown)
};
std::atomic<int> g_grid_pin[kGridKernels];      // nry << 16 | nrx, 0: automatic (semidetr_msda_set_region_grid)

// smallest q in [0, nq] whose pixel centre maps into row >= bound of the nb-row grid level (rw_first on the host)
int64_t grid_first(int64_t bound, int64_t nq, int64_t nb) { return std::min(nq, ((2 * nq * bound + nb - 1) / nb) >> 1); }

// queries of the largest region of an nry x nrx grid on level `lb` of the host table (H, W pairs); `even`: balanced tiling, else steps of rth x rtw
int grid_max_queries(const int64_t *hs, int L, int lb, int nry, int nrx, bool even, int rth, int rtw)
{
    const int64_t Hb = hs[2 * lb], Wb = hs[2 * lb + 1];
    std::vector<int> cy((size_t)L * nry), cx((size_t)L * nrx);
    for (int l = 0; l < L; ++l) {
        const int64_t Hq = hs[2 * l], Wq = hs[2 * l + 1];
        for (int r = 0; r < nry; ++r) {
            const int64_t y0 = even ? r * Hb / nry : (int64_t)r * rth, y1 = even ? (r + 1) * Hb / nry : std::min<int64_t>(y0 + rth, Hb);
            cy[(size_t)l * nry + r] = (int)std::max<int64_t>((y1 >= Hb ? Hq : grid_first(y1, Hq, Hb)) - grid_first(y0, Hq, Hb), 0);
        }
        for (int r = 0; r < nrx; ++r) {
            const int64_t x0 = even ? r * Wb / nrx : (int64_t)r * rtw, x1 = even ? (r + 1) * Wb / nrx : std::min<int64_t>(x0 + rtw, Wb);
            cx[(size_t)l * nrx + r] = (int)std::max<int64_t>((x1 >= Wb ? Wq : grid_first(x1, Wq, Wb)) - grid_first(x0, Wq, Wb), 0);
        }
    }
    int best = 0;
    for (int ry = 0; ry < nry; ++ry)
        for (int rx = 0; rx < nrx; ++rx) {
            int q = 0;
            for (int l = 0; l < L; ++l) q += cy[(size_t)l * nry + ry] * cx[(size_t)l * nrx + rx];
            best = std::max(best, q);
        }
    return best;
}

// the launch's cost in rounds; `tail` in: the kernel has a tail split, out: the split pays
double grid_score(const GridGeom &g, int64_t units, int cus, int max_queries, bool &tail)
{
    const int64_t slots = (int64_t)cus * g.per_cu;
    const double rounds = (double)max_queries / g.round;
    const double unit = g.setup + rounds;
    const int64_t full = units / slots, rem = units % slots;
    const double plain = (double)(full + (rem > 0)) * unit;
    if (tail) {
        tail = false;
        // (msda_rw.h: launches of fewer than three waves, the last wave's units cut into s <= 4 parts of their rounds, each staging the windows
        //  again; + 1 round for the helpers' late start: 4 x 11 / 4 x 12 / 4 x 17 / 5 x 13 with the split measured 9.3 / 9.5 / 9.6 / 9.6 model
        //  units beside 4 x 16's 8.8 without it, the formula gives 10.3 / 9.4 / 10.4 / 10.7)
        const int s = rem > 0 ? (int)std::min<int64_t>(slots / rem, 4) : 1;
        if (units < 3 * slots && s > 1) {
            const double split = full * unit + g.setup + rounds / s + 1.0;
            if (split < plain) {
                tail = true;
                return split;
            }
        }
    }
    return plain;
}

struct GridCacheEntry {
    int kernel, L, N, M, cus;
    int64_t hw[2 * 8];
    GridChoice choice;
};
std::mutex g_grid_mu;
std::vector<GridCacheEntry> g_grid_cache;

// The grid of one launch.  g: the kernel's geometry for this pyramid (one per (kernel, levels), whatever the IO).  hs: host copy of
// spatial_shapes (num_levels x {H, W}) or null.  tail_kernel: the configuration has a tail split.
GridChoice region_grid_choice(int kernel, const GridGeom &g, const int64_t *hs, int L, int N, int M, int cus, bool tail_kernel)
{
    GridChoice c;
    const int pin = g_grid_pin[kernel].load(std::memory_order_relaxed);
    bool known = hs != nullptr && cus > 0 && L > 0 && L <= 8 && N > 0 && M > 0;
    for (int l = 0; known && l < L; ++l) known = hs[2 * l] > 0 && hs[2 * l] <= 32766 && hs[2 * l + 1] > 0 && hs[2 * l + 1] <= 32766;
    if (!known) {      // the kernel derives its grid from the device table (a pinned grid: max(pin, coarsest)); grid size by hint
        c.nry = pin >> 16;
        c.nrx = pin & 0xffff;
        return c;
    }
    // the level that carries the grid: level 0 for the window kernels, the one with the most pixels for the scatter
    int lb = 0;
    if (kernel == 2)
        for (int l = 1; l < L; ++l)
            if (hs[2 * l] * hs[2 * l + 1] > hs[2 * lb] * hs[2 * lb + 1]) lb = l;
    const int Hb = (int)hs[2 * lb], Wb = (int)hs[2 * lb + 1];
    const int ny0 = (Hb + g.rth - 1) / g.rth, nx0 = (Wb + g.rtw - 1) / g.rtw;
    auto finish = [&](int ny, int nx, bool as_coarsest) {
        const bool even = !as_coarsest || g.even;
        c.nry = as_coarsest && !g.even ? 0 : ny;
        c.nrx = as_coarsest && !g.even ? 0 : nx;
        c.regions = ny * nx;
        c.max_queries = grid_max_queries(hs, L, lb, ny, nx, even, g.rth, g.rtw);
        bool t = tail_kernel;
        (void)grid_score(g, (int64_t)N * c.regions * M, cus, c.max_queries, t);
        c.tail = t;
    };
    if (pin) {
        finish(std::max(pin >> 16, ny0), std::max(pin & 0xffff, nx0), false);
        return c;
    }
    {
        std::lock_guard<std::mutex> lock(g_grid_mu);
        for (const auto &e : g_grid_cache)
            if (e.kernel == kernel && e.L == L && e.N == N && e.M == M && e.cus == cus && std::equal(hs, hs + 2 * L, e.hw)) return e.choice;
    }
    finish(ny0, nx0, true);
    bool t0 = tail_kernel;
    const double coarse = grid_score(g, (int64_t)N * ny0 * nx0 * M, cus, c.max_queries, t0);
    const bool small = (int64_t)N * ny0 * nx0 * M < (int64_t)3 * cus * g.per_cu;
    if (kGridAuto[kernel][small ? 0 : 1]) {
        double best = coarse * 0.98;      // ties, and gains the model cannot tell from nothing, keep the coarsest grid
        int by = 0, bx = 0;
        for (int ny = ny0; ny <= std::min(ny0 + kGridCap, Hb); ++ny)
            for (int nx = nx0; nx <= std::min(nx0 + kGridCap, Wb); ++nx) {
                if (ny == ny0 && nx == nx0 && g.even) continue;
                bool t = tail_kernel;
                const double s = grid_score(g, (int64_t)N * ny * nx * M, cus, grid_max_queries(hs, L, lb, ny, nx, true, g.rth, g.rtw), t);
                if (s < best) { best = s; by = ny; bx = nx; }
            }
        if (by) finish(by, bx, false);
    }
    GridCacheEntry e{kernel, L, N, M, cus, {0}, c};
    std::copy(hs, hs + 2 * L, e.hw);
    std::lock_guard<std::mutex> lock(g_grid_mu);
    if (g_grid_cache.size() >= 64) g_grid_cache.erase(g_grid_cache.begin());
    g_grid_cache.push_back(e);
    return c;
}

}  // namespace
