// Stand-alone host program (plain C++, no HIP): sweeps the tile schedule of eeg2video_amd/csrc/gemm_sched.h.
// tests/test_gemm_sched_host.py builds it with -fsanitize=address,undefined and runs it.
//
// For every launch of the sweep it decodes the whole 8 x longest-chunk grid the way the kernels do (x = block % 8, loc = block / 8) and
// asserts: (a) the valid tiles cover every (row block, 64-column group below N) of the launch exactly once, a wide tile two groups;
// (b) in every XCD chunk the valid blocks are a prefix -- invalid blocks lie only past the chunk's end -- of chunk_tiles() blocks;
// (c) sched_grid() is 8 x the longest chunk's tile count and sched_real_tiles() the sum.  For the launches at the default switches it
// prints the plan, one line each: the pytest compares them with the independent restatement of tests/igemm_schedule.py.
#include "gemm_sched.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace e2v;

static long checked = 0;

#define REQUIRE(cond, ...)                                                        \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "gemm_sched_driver: %s failed: ", #cond);        \
            std::fprintf(stderr, __VA_ARGS__);                                    \
            std::fprintf(stderr, "\n");                                           \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

static void check(const PlanIn& in, const TileSched& s, const char* what) {
    const int groups = (in.N + 63) / 64;                     // 64-column groups that hold a column of the launch
    std::vector<unsigned char> seen((size_t)s.nbm * groups, 0);
    const int grid = sched_grid(s);
    REQUIRE(grid % 8 == 0, "%s M%d N%d b%d: grid %d", what, in.M, in.N, in.batch, grid);
    int longest = 0;
    long real = 0;
    for (int x = 0; x < 8; ++x) {
        const RowBlocks rb = xcd_row_blocks(x, s.nbm);
        REQUIRE(rb.lo == (int)((long)x * s.nbm / 8) && rb.lo + rb.n == (int)((long)(x + 1) * s.nbm / 8), "%s nbm %d chunk %d", what, s.nbm, x);
        int valid = 0;
        for (int loc = 0; loc < grid / 8 + 2; ++loc) {       // (two blocks past the grid: still invalid)
            const Tile t = tile_decode(s, x, loc);
            if (!t.valid) continue;
            REQUIRE(loc == valid, "%s M%d N%d b%d: chunk %d has a valid block %d behind an invalid one", what, in.M, in.N, in.batch, x, loc);
            ++valid;
            REQUIRE(t.rbg >= rb.lo && t.rbg < rb.lo + rb.n, "%s M%d N%d b%d: chunk %d block %d decodes row block %d", what, in.M, in.N, in.batch, x, loc, t.rbg);
            REQUIRE(t.n0 >= 0 && t.n0 % 64 == 0 && t.n0 < in.N, "%s M%d N%d b%d: chunk %d block %d starts at column %d", what, in.M, in.N, in.batch, x, loc, t.n0);
            for (int g = t.n0 / 64; g < t.n0 / 64 + (t.wide ? 2 : 1) && g < groups; ++g) {
                unsigned char& c = seen[(size_t)t.rbg * groups + g];
                REQUIRE(c == 0, "%s M%d N%d b%d: row block %d, columns %d.. covered twice", what, in.M, in.N, in.batch, t.rbg, g * 64);
                c = 1;
            }
        }
        REQUIRE(valid == chunk_tiles(s, x), "%s M%d N%d b%d: chunk %d decodes %d tiles, chunk_tiles() says %d", what, in.M, in.N, in.batch, x, valid, chunk_tiles(s, x));
        REQUIRE(valid <= grid / 8, "%s M%d N%d b%d: chunk %d needs %d blocks of a grid of 8 x %d", what, in.M, in.N, in.batch, x, valid, grid / 8);
        longest = valid > longest ? valid : longest;
        real += valid;
        REQUIRE(rb.n <= longest_chunk(s.nbm), "%s nbm %d: chunk %d is longer than longest_chunk()", what, s.nbm, x);
    }
    for (size_t i = 0; i < seen.size(); ++i)
        REQUIRE(seen[i] == 1, "%s M%d N%d b%d: row block %d, columns %d.. not covered", what, in.M, in.N, in.batch, (int)(i / groups), (int)(i % groups) * 64);
    REQUIRE(grid == 8 * longest, "%s M%d N%d b%d: grid %d, longest chunk %d tiles", what, in.M, in.N, in.batch, grid, longest);
    REQUIRE(real == sched_real_tiles(s), "%s M%d N%d b%d: %ld tiles, sched_real_tiles() says %ld", what, in.M, in.N, in.batch, real, sched_real_tiles(s));
    REQUIRE((s.nbm + 7) / 8 == longest_chunk(s.nbm) && xcd_row_blocks(7, s.nbm).n == longest_chunk(s.nbm), "%s nbm %d: longest_chunk()", what, s.nbm);
    ++checked;
}

int main() {
    static const int NS[] = {40, 64, 72, 128, 192, 320, 1024, 2560}, BATCH[] = {1, 16, 36}, PAIRS[][2] = {{128, 512}, {256, 256}};
    // row blocks at whose boundaries M is taken (-1, 0, +1): every count up to 17 (one and two per chunk), then the counts of the graph's
    // launches and of the suite's cases, up to 547 x 128 = 70 016 rows
    static const int KS[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 23, 31, 43, 51, 64, 75, 100, 127, 178, 204, 254, 299, 400, 547};
    for (const auto& pair : PAIRS)
        for (const int k : KS)
            for (int d = -1; d <= 1; ++d) {
                const int M = k * pair[0] + d;
                if (M < 1 || M > 70100) continue;
                for (const int N : NS)
                    for (const int batch : BATCH)
                        for (int geglu = 0; geglu < 2; ++geglu) {
                            PlanIn in{};
                            in.M = M; in.N = N; in.batch = batch; in.geglu = geglu != 0;
                            in.rows = pair[0]; in.slots = pair[1];
                            in.all_narrow = false; in.full_only = false; in.sched = 1; in.half_below = 0;
                            const Plan p = plan_tiles(in);
                            check(in, p.sched(), "default");
                            std::printf("plan M%d N%d b%d g%d rows%d slots%d: rb1=%d w1=%d s1=%d s2=%d nbm=%d nbm_per=%d tail_rb=%d grid=%d real=%ld\n", M, N, batch,
                                        geglu, in.rows, in.slots, p.rb1, p.w1, p.s1, p.s2, p.nbm, p.nbm_per, p.tail_rb, sched_grid(p.sched()),
                                        sched_real_tiles(p.sched()));
                            if (batch != 1) continue;
                            // the other requests and switch values: the same three properties, and what each request means
                            PlanIn v = in;
                            v.sched = 0;
                            const Plan p0 = plan_tiles(v);
                            check(v, p0.sched(), "sched0");
                            REQUIRE(p0.rb1 == (p0.w1 == 0 ? 0 : p0.nbm) || geglu, "sched0 M%d N%d: rb1 %d", M, N, p0.rb1);
                            v = in; v.all_narrow = true;
                            const Plan pn = plan_tiles(v);
                            check(v, pn.sched(), "all_narrow");
                            REQUIRE(pn.rb1 == 0 && pn.tail_rb == pn.nbm, "all_narrow M%d N%d: rb1 %d tail_rb %d", M, N, pn.rb1, pn.tail_rb);
                            v = in; v.full_only = true;
                            const Plan pf = plan_tiles(v);
                            check(v, pf.sched(), "full_only");
                            REQUIRE(pf.rb1 == (pf.w1 == 0 ? 0 : pf.nbm), "full_only M%d N%d: rb1 %d", M, N, pf.rb1);
                            TileSched notail = pf.sched();           // as the split-K kernel walks it: no tail at all
                            notail.tail_rb = 0;
                            check(v, notail, "full_only, no tail");
                            v = in; v.half_below = 150;
                            const Plan ph = plan_tiles(v);
                            check(v, ph.sched(), "half_below");
                            REQUIRE(ph.rb1 == p.rb1 || ph.rb1 == 0, "half_below M%d N%d: rb1 %d (default %d)", M, N, ph.rb1, p.rb1);
                        }
            }
    std::printf("gemm_sched_driver: ok, %ld schedules checked\n", checked);
    return 0;
}
