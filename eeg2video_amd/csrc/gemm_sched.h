// The tile schedule of the GEMM kernels (igemm.hip, bgemm.hip, bgemm256.hip): one rule, written once.
//
// A launch has `nbm` row blocks (128 or 256 rows; the row blocks of all batch entries together).  They are dealt to 8 XCD chunks,
// chunk x = blockIdx % 8 owning the contiguous row blocks [x nbm / 8, (x + 1) nbm / 8): blocks go to the XCDs round-robin, so the
// column tiles that share one gathered A tile hit the same L2.  The LAST min(length, tail_rb) row blocks of a chunk are its tail, cut
// into s2 tiles of 128x64 only; the row blocks in front of them are cut into w1 tiles of 128x128 followed by s1 tiles of 128x64
// (N = 320 -> 2 + 1, no wasted columns).  Every chunk therefore ends on half-size tiles.  The grid is 8 x the tile count of the longest
// chunk; the blocks a shorter chunk does not need are invalid and return at once.
//
// Plain C++ and HIP; no switches, no getenv, no HIP calls: the launchers pass the values of their switches in.
// tests/test_gemm_sched_host.py sweeps this header on the CPU; tests/igemm_schedule.py restates the planner independently.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define E2V_SCHED_HD __host__ __device__
#else
#define E2V_SCHED_HD
#endif

namespace e2v {

struct RowBlocks {
    int lo, n;                      // first row block of a chunk and how many
};
E2V_SCHED_HD inline RowBlocks xcd_row_blocks(const int x, const int nbm) {
    const int lo = (int)(((long)x * nbm) >> 3), hi = (int)(((long)(x + 1) * nbm) >> 3);
    return RowBlocks{lo, hi - lo};
}

struct TileSched {                  // what the kernels need of a plan (IgemmArgs carries the same fields: tile_sched(), kernels.h)
    int nbm, w1, s1, s2, tail_rb;
};
struct Tile {
    int rbg, n0, wide, valid;       // row block (over all batch entries), first column, 128 columns wide (else 64), not a padding block
};

// block `loc` of chunk x: columns fastest, the wide part of the chunk in front of its tail
E2V_SCHED_HD inline Tile tile_decode(const TileSched& p, const int x, const int loc) {
    Tile t{0, 0, 0, 0};
    const RowBlocks rb = xcd_row_blocks(x, p.nbm);
    const int tail = rb.n < p.tail_rb ? rb.n : p.tail_rb;
    const int per1 = p.w1 + p.s1;
    const int n1 = (rb.n - tail) * per1;
    if (loc < n1) {
        const int r = loc / per1, j = loc - r * per1;
        t.rbg = rb.lo + r;
        t.wide = j < p.w1;
        t.n0 = t.wide ? j * 128 : p.w1 * 128 + (j - p.w1) * 64;
        t.valid = 1;
    } else {
        const int q = loc - n1;
        if (q < tail * p.s2) {
            const int r = q / p.s2;
            t.rbg = rb.lo + (rb.n - tail) + r;
            t.n0 = (q - r * p.s2) * 64;
            t.valid = 1;
        }
    }
    return t;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
inline int chunk_tiles(const TileSched& p, const int x) {
    const int nrb = xcd_row_blocks(x, p.nbm).n;
    const int tail = nrb < p.tail_rb ? nrb : p.tail_rb;
    return (nrb - tail) * (p.w1 + p.s1) + tail * p.s2;
}
inline int sched_grid(const TileSched& p) {                 // blocks of a launch: 8 x the longest chunk's tiles
    int most = 0;
    for (int x = 0; x < 8; ++x) most = chunk_tiles(p, x) > most ? chunk_tiles(p, x) : most;
    return 8 * most;
}
inline long sched_real_tiles(const TileSched& p) {          // the tiles the grid really holds
    long real = 0;
    for (int x = 0; x < 8; ++x) real += chunk_tiles(p, x);
    return real;
}
inline int longest_chunk(const int nbm) { return (nbm + 7) / 8; }      // row blocks of the longest chunk

struct PlanIn {
    int M, N, batch;                // rows per batch entry, GEMM columns (GEGLU: both halves), batch entries
    bool geglu;
    int rows, slots;                // row-block height and the resident tiles a round is sized by: 128 / 512 or 256 / 256
    bool all_narrow;                // the caller wants 128x64 tiles only
    bool full_only;                 // split-K: full-size tiles, no tail (the runs multiply the workgroup count)
    int sched;                      // E2V_IGEMM_SCHED (0: no half-size tails)
    int half_below;                 // E2V_IGEMM_HALF_BELOW (r x 100 > 0: fewer than r rounds run entirely as 128x64 tiles; 0: off)
};
struct Plan {
    int rb1, w1, s1, s2, nbm, nbm_per, tail_rb;          // rb1: the wide row blocks the rule asks for (0: narrow, nbm: wide, else mixed)
    TileSched sched() const { return TileSched{nbm, w1, s1, s2, tail_rb}; }
};

inline Plan plan_tiles(const PlanIn& in) {
    Plan p{};
    p.nbm_per = (in.M + in.rows - 1) / in.rows;
    p.nbm = p.nbm_per * in.batch;                            // batch entries are just more row blocks (dealt to the XCDs together)
    p.s2 = (in.N + 63) / 64;
    p.w1 = in.N / 128;                                       // full 128-wide column tiles
    const int rem = in.N - p.w1 * 128;
    p.s1 = rem == 0 ? 0 : (rem <= 64 ? 1 : 0);
    if (rem > 64) p.w1 += 1;                                 // 65..127 leftover columns: one more (masked) wide tile
    p.rb1 = p.nbm;
    const int nrb = longest_chunk(p.nbm);
    const int xslots = in.slots / 8;                         // per XCD: resident tiles per round
    if (in.geglu) {                                          // the GEGLU epilogue pairs the two 32-column halves of a wave
        p.w1 = (in.N + 127) / 128; p.s1 = 0;
    } else if (p.w1 == 0) {                                  // N <= 64
        p.rb1 = 0;
    } else if (in.full_only) {
    } else if (in.sched == 1) {
        // Keep whole rounds of full-size tiles; if what is left of the XCD's chunk is at most half a round, run it as half-size
        // tiles (it then takes about half a round's time).
        const double per_rb = p.w1 + 0.5 * p.s1;             // cost of one row block in 128x128 units
        const double units = per_rb * nrb;
        if (units * 8 < in.slots) {
            p.rb1 = 0;                                       // less than one round: half-size tiles spread over more CUs
        } else {
            const int full = (int)std::floor(units / xslots);
            const int wide_rb = (int)std::floor(full * xslots / per_rb);
            const int tail = nrb - wide_rb;
            if (tail > 0 && tail * per_rb <= 0.5 * xslots) p.rb1 = p.nbm - 8 * tail < 0 ? 0 : p.nbm - 8 * tail;
        }
    }
    if (in.half_below > 0 && !in.geglu && p.w1 > 0 && p.rb1 > 0) {
        const double per_rb = p.w1 + 0.5 * p.s1;
        const double rounds = per_rb * nrb / xslots;
        if (rounds * 100.0 < (double)in.half_below) p.rb1 = 0;
    }
    if (in.all_narrow) p.rb1 = 0;
    p.tail_rb = p.rb1 == 0 ? p.nbm : (p.nbm - p.rb1 + 7) / 8;       // per XCD chunk (rb1 == 0: every row block is "tail")
    return p;
}

}  // namespace e2v
