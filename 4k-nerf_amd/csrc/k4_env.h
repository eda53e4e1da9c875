// Process-wide switches of lib4k_hip.so: environment variables read ONCE while the library is being loaded; launches never call getenv.
// Nothing from HIP in here: a plain host compiler builds it (tests/env_split_check.cpp).
//
// K4_DEBUG and K4_SR_DEBUG each carry two kinds of bits:
//  - exact selectors pick another path that computes the SAME bits (A/B runs, tests): named bools of K4Env, honoured by every build;
//  - ablations switch parts of a kernel off for timing and give WRONG results: they exist only in a library built with -DK4_ABLATE
//    (python 4k-nerf_amd/build.py --tag ablate -DK4_ABLATE, loaded through K4_LIB).  The product build keeps both masks at 0 whatever
//    the environment says and says so once on stderr; K4_ABL below is the constant 0 there, so the compiler drops the branches behind it.
#pragma once
#include <stdio.h>
#include <stdlib.h>

// K4_DEBUG ablations: 1 = k0 fetch replaced by constants, 2 = rgbnet layers skipped, 512 = no per-ray sums (shading kernel); geometry kernel,
// general instantiation only: 16 = no density fetch, 32 = no transmittance scan, 128 = no survivor compaction, 4096 = no groups (the kernel's
// fixed cost), 8192 = not even the arrival / scan
#define K4_GEOM_ABLATE_BITS (16 | 32 | 128 | 4096 | 8192)
#define K4_ABLATE_BITS (1 | 2 | 512 | K4_GEOM_ABLATE_BITS)
// K4_SR_DEBUG ablations: 1 = input channel stride 0 (no memory traffic); 2, 4, 8, 16 = phases of the 3x3 kernel (k4_sr.hip ConvParams);
// 64, 128, 256, 512 = phases of the p16 kernels (k4_sr_p16.hip)
#define K4_SR_ABLATE_BITS (1 | 2 | 4 | 8 | 16 | 64 | 128 | 256 | 512)

// The one place that knows whether this is an ablation build.  A site that reads an ablation bit goes through K4_ABL: the p16 decoder kernels and
// every host site.  The two marcher kernels and the 3x3 convolution kernel of k4_sr.hip test the (always-zero) runtime field instead: with the
// branches folded away the marcher's register allocation got worse and the bf16x6 decoder frame 3 % slower (profiles/ablate_build.md).  What
// keeps the product right is the zero mask, not the folding.
#ifdef K4_ABLATE
#define K4_ABLATE_BUILD 1
#define K4_ABL(mask, bits) ((mask) & (bits))
#else
#define K4_ABLATE_BUILD 0
#define K4_ABL(mask, bits) ((void)(mask), 0)
#endif

struct K4Env {
    int geom_skip;       // K4_GEOM_SKIP    (1) 0: do not use the coarse occupancy summary (A/B of the empty-space skipping)
    int ablate;          // K4_DEBUG & K4_ABLATE_BITS        (0) marcher ablations; always 0 in the product build
    int sr_ablate;       // K4_SR_DEBUG & K4_SR_ABLATE_BITS  (0) decoder ablations; always 0 in the product build
    // exact selectors (A/B, tests: identical outputs)
    bool no_fast_shade;  // K4_DEBUG & 1024: the shading kernel's general path on shapes the FAST path covers
    bool single_launch;  // K4_DEBUG & 2048: one geometry launch whatever k4_grid_desc.depth_split says
    bool no_fast_geom;   // K4_DEBUG & 16384: the geometry kernel's general path on shapes its FAST path covers
    bool sft_unpiped;    // K4_SR_DEBUG & 32: SFT layers on the unpipelined kernel
    bool row_kernel;     // K4_SR_DEBUG & 2048: row kernel instead of the K-split 3x3 kernel on small images
    bool wgrad_per_tap;  // K4_SR_DEBUG & 4096: per-tap weight-gradient kernel instead of the nine-tap one
};

// pure: the raw values of K4_DEBUG and K4_SR_DEBUG (and K4_GEOM_SKIP) -> the switches of this build
inline K4Env k4_env_of(int debug, int sr_debug, int geom_skip = 1) {
    K4Env e{};
    e.geom_skip = geom_skip;
    e.ablate = K4_ABLATE_BUILD ? debug & K4_ABLATE_BITS : 0;
    e.sr_ablate = K4_ABLATE_BUILD ? sr_debug & K4_SR_ABLATE_BITS : 0;
    e.no_fast_shade = (debug & 1024) != 0;
    e.single_launch = (debug & 2048) != 0;
    e.no_fast_geom = (debug & 16384) != 0;
    e.sft_unpiped = (sr_debug & 32) != 0;
    e.row_kernel = (sr_debug & 2048) != 0;
    e.wgrad_per_tap = (sr_debug & 4096) != 0;
    return e;
}

inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
inline K4Env k4_env_load() {
    const int debug = env_int("K4_DEBUG", 0), sr_debug = env_int("K4_SR_DEBUG", 0);
    if (!K4_ABLATE_BUILD && ((debug & K4_ABLATE_BITS) || (sr_debug & K4_SR_ABLATE_BITS)))
        fprintf(stderr, "lib4k_hip: ignored ablation bits K4_DEBUG & %d, K4_SR_DEBUG & %d: this build has no ablations (they need a -DK4_ABLATE build)\n",
                debug & K4_ABLATE_BITS, sr_debug & K4_SR_ABLATE_BITS);
    return k4_env_of(debug, sr_debug, env_int("K4_GEOM_SKIP", 1));
}
// namespace-scope constant (one for the whole library): initialised while the library is loaded, immutable afterwards
inline const K4Env g_k4_env = k4_env_load();
inline const K4Env& k4_env() { return g_k4_env; }
