// Stand-alone host check of the geometry kernel's group deal (4k-nerf_amd/csrc/k4_geom_deal.h), built and run by tests/test_geom_deal_host.py.
// For every sample count n = 1..256 and the worst case "every sample of every ray is a record":
//   1. (ray, group) <-> (wave, ray, slot) is a bijection;
//   2. no (wave, slot) segment takes more than quarter / 4 records, and every segment lies inside its slice quarter and the 5-quarter slice;
//   3. the tail's segment order i = 0..3 of a ray's depth quarter is depth-ascending;
//   4. the append bound of the hazard argument: the records of depth quarters 0..j number at most (j + 1) * quarter, and no record of quarter j
//      lies below (j + 1) * quarter -- so the survivors appended while quarter j is scanned stay below every record not yet read.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "k4_geom_deal.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } ++fails; } } while (0)

int main() {
    const int GRP = 16;
    for (int n = 1; n <= 256; ++n) {
        const int quarter = 16 * ((n + 255) / 256 * 256);                 // ent_quarter_of(max_steps = n)
        const int ng = (n + GRP - 1) / GRP;
        std::vector<int> owner(64 * 16, -1);                              // (r, G) -> wave * 4 + slot
        long long per_seg[4][4] = {};                                     // records of (wave, slot), every sample a record
        for (int w = 0; w < 4; ++w)
            for (int r = 0; r < 64; ++r)
                for (int j = 0; j < 4; ++j) {
                    const int G = k4_deal_group(w, r, j);
                    CHECK(G >= 0 && G < 16, "n=%d w=%d r=%d j=%d G=%d", n, w, r, j, G);
                    CHECK(k4_deal_slot(G) == j, "n=%d G=%d slot %d != %d", n, G, k4_deal_slot(G), j);
                    CHECK(k4_deal_wave(r, G) == w, "n=%d r=%d G=%d wave %d != %d", n, r, G, k4_deal_wave(r, G), w);
                    if (G >= ng) continue;                                // the group starts at or behind the ray's last sample
                    CHECK(owner[r * 16 + G] == -1, "n=%d r=%d G=%d dealt twice", n, r, G);
                    owner[r * 16 + G] = w * 4 + j;
                    const int lo = G * GRP, hi = (G + 1) * GRP < n ? (G + 1) * GRP : n;
                    per_seg[w][j] += hi - lo;
                    for (int k = lo; k < hi; ++k) CHECK((k >> 6) == j, "n=%d k=%d not in quarter %d", n, k, j);      // stage B files a record by k >> 6
                }
        for (int r = 0; r < 64; ++r)
            for (int G = 0; G < ng; ++G) CHECK(owner[r * 16 + G] >= 0, "n=%d r=%d G=%d dealt to no wave", n, r, G);
        long long upto = 0;
        for (int j = 0; j < 4; ++j) {
            for (int w = 0; w < 4; ++w) {
                CHECK(per_seg[w][j] <= quarter / 4, "n=%d w=%d j=%d %lld records > %d", n, w, j, per_seg[w][j], quarter / 4);
                const long long base = k4_deal_seg_base(w, j, quarter);
                CHECK(base >= (long long)(j + 1) * quarter, "n=%d w=%d j=%d base %lld below quarter", n, w, j, base);
                CHECK(base + quarter / 4 <= (long long)(j + 2) * quarter && base + quarter / 4 <= 5LL * quarter, "n=%d w=%d j=%d segment leaves its quarter", n, w, j);
                if (w > 0) CHECK(base == k4_deal_seg_base(w - 1, j, quarter) + quarter / 4, "n=%d segments overlap or gap", n);
                upto += per_seg[w][j];
            }
            CHECK(upto <= (long long)(j + 1) * quarter, "n=%d j=%d appends %lld can pass %lld", n, j, upto, (long long)(j + 1) * quarter);
        }
        for (int r = 0; r < 64; ++r)
            for (int j = 0; j < 4; ++j)
                for (int i = 0; i < 4; ++i) {
                    const int G = k4_deal_group(k4_deal_seg_wave(r, i), r, j);
                    CHECK(G == 4 * j + i, "n=%d r=%d j=%d segment %d holds group %d", n, r, j, i, G);
                }
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("geom deal: sample counts 1..256 ok\n");
    return 0;
}
