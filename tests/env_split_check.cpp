// Host check of 4k-nerf_amd/csrc/k4_env.h (tests/test_env_split_host.py compiles this twice, with and without -DK4_ABLATE): k4_env_of turns the raw
// K4_DEBUG / K4_SR_DEBUG values into exact selectors, which every build honours, and ablation masks, which only a -DK4_ABLATE build keeps.
#include "k4_env.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s (K4_DEBUG=%d K4_SR_DEBUG=%d)\n", __LINE__, #c, d, s); ++fails; } } while (0)

static void check(int d, int s) {
    const K4Env e = k4_env_of(d, s);
    // the wrong-result bits, spelled out here on purpose (not the header's macros)
    const int abl = 1 | 2 | 16 | 32 | 128 | 512 | 4096 | 8192, sr_abl = 1 | 2 | 4 | 8 | 16 | 64 | 128 | 256 | 512;
#ifdef K4_ABLATE
    CHECK(e.ablate == (d & abl));
    CHECK(e.sr_ablate == (s & sr_abl));
    CHECK(K4_ABL(d, 2) == (d & 2));
#else
    CHECK(e.ablate == 0);
    CHECK(e.sr_ablate == 0);
    CHECK(K4_ABL(d, 2) == 0);
    (void)abl; (void)sr_abl;
#endif
    CHECK(e.no_fast_shade == ((d & 1024) != 0));
    CHECK(e.single_launch == ((d & 2048) != 0));
    CHECK(e.no_fast_geom == ((d & 16384) != 0));
    CHECK(e.sft_unpiped == ((s & 32) != 0));
    CHECK(e.row_kernel == ((s & 2048) != 0));
    CHECK(e.wgrad_per_tap == ((s & 4096) != 0));
    CHECK(e.geom_skip == 1);
}

int main() {
    static_assert(K4_ABLATE_BITS == 12979 && K4_SR_ABLATE_BITS == 991, "the ablation bits of the two variables");
    static_assert((K4_ABLATE_BITS & (1024 | 2048 | 16384)) == 0 && (K4_SR_ABLATE_BITS & (32 | 2048 | 4096)) == 0, "no bit is both");
    check(0, 0);
    for (int b = 0; b < 16; ++b) {
        check(1 << b, 0);
        check(0, 1 << b);
        check(1 << b, 1 << b);
    }
    check(0xffff, 0xffff);
    check(-1, -1);
    if (fails) return 1;
    printf("env split ok (%s build)\n", K4_ABLATE_BUILD ? "ablation" : "product");
    return 0;
}
