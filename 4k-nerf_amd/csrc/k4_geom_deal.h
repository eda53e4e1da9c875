// The deal of a bundle's 16-sample depth groups over the four waves of a geometry workgroup (k4_geom3_kernel, FAST instantiation), as index
// arithmetic only: shared by the kernel and by the stand-alone host check (tests/test_geom_deal_host.py), so it includes nothing.
//
// A bundle is 64 ray slots r = 0..63; a ray's samples k = 0..n-1 (n <= 256) fall into groups G = k >> 4 (0..15) and depth quarters k >> 6.
// Depth QUARTERS per wave (the general instantiation) leave one wave with most of a bundle's work, because a scene's content sits in a few
// neighbouring groups.  Here group G of ray r belongs to wave (G + (r >> 4)) & 3: consecutive groups of a ray go to consecutive waves, and the
// skew by the ray's 16-ray subset spreads ONE group column (the same G on all 64 rays) over all four waves.  Seen from wave w, ray r has the
// four SLOTS j = 0..3 with group 4 j + ((w - (r >> 4)) & 3): slot j lies in depth quarter j, and a wave still holds at most 4 groups = 64
// samples of a ray.
//
// Workspace slice of a bundle (5 quarters of `quarter` records): the raw records of depth quarter j live in slice quarter j + 1, cut into four
// segments of quarter / 4 records; segment w is written by wave w alone, ray-major and depth-ascending.  A ray's records of quarter j in depth
// order are its pieces of the segments of waves (i + (r >> 4)) & 3 for i = 0..3.
#ifndef K4_GEOM_DEAL_H
#define K4_GEOM_DEAL_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define K4_DEAL_HD __host__ __device__ __forceinline__
#else
#define K4_DEAL_HD inline
#endif

K4_DEAL_HD int k4_deal_skew(int r) { return r >> 4; }                                      // s(r): the ray slot's 16-ray subset
K4_DEAL_HD int k4_deal_wave(int r, int G) { return (G + k4_deal_skew(r)) & 3; }            // the wave that owns group G of ray r
K4_DEAL_HD int k4_deal_offset(int w, int r) { return (w - k4_deal_skew(r)) & 3; }          // wave w's group inside every depth quarter of ray r
K4_DEAL_HD int k4_deal_group(int w, int r, int j) { return 4 * j + k4_deal_offset(w, r); } // group of wave w's slot j of ray r
K4_DEAL_HD int k4_deal_slot(int G) { return G >> 2; }                                      // slot = depth quarter of group G
K4_DEAL_HD int k4_deal_seg_wave(int r, int i) { return (i + k4_deal_skew(r)) & 3; }        // owner of the i-th segment (depth order) of ray r's quarter
// first record of wave w's segment of depth quarter j, in records from the start of the bundle's slice (quarter % 4 == 0: ent_quarter_of)
K4_DEAL_HD long long k4_deal_seg_base(int w, int j, int quarter) { return (long long)(j + 1) * quarter + (long long)w * (quarter >> 2); }

#endif
