// Host predicate of the geometry kernel's 32-bit addressing (k4_march.hip: K4_IDX_OFF32): plain C++, includes nothing of HIP.
//
// The FAST instantiation of the geometry kernel addresses every array as a uniform base + an unsigned 32-bit per-lane byte offset and forms
// the summary index in 32 bits.  That is an integer identity when
//   X*Y*Z*4 < 2^32                       a density byte offset fits 32 bits
//   MX*MY*MZ < 2^32                      a mask byte offset fits 32 bits
//   occ_bytes < 2^32                     the occupancy summary's four tables of 8-byte windows (what the kernel reads)
//   slice_bytes < 2^32                   a bundle's workspace slice (ent_stride records of 8 bytes)
// The predicate also asks for
//   X*Y < 2^24, Z < 2^24, MX*MY < 2^24, MZ < 2^24
// which is what 24-bit multiply-adds for (x*Y + y)*Z and (mi*MY + mj)*MZ + mk would need.  Those were measured no faster than the 32-bit
// multiplies on gfx950 and are not built (profiles/march_index32.md); the limits stay, so that such a form can come back without moving the
// line between the two instantiations.  A grid the byte limits admit with 64 .. 2^24 - 1 planes meets them anyway.
// launch_march ANDs this into the geometry kernel's FAST predicate; a grid beyond any limit takes the general instantiation, whose 64-bit
// forms have none.
#ifndef K4_INDEX32_H
#define K4_INDEX32_H
#include <stdint.h>

static inline int k4_index32_ok(int64_t X, int64_t Y, int64_t Z, int64_t MX, int64_t MY, int64_t MZ, int64_t occ_bytes, int64_t slice_bytes) {
    const int64_t b24 = (int64_t)1 << 24, b32 = (int64_t)1 << 32;
    if (X <= 0 || Y <= 0 || Z <= 0 || MX <= 0 || MY <= 0 || MZ <= 0 || occ_bytes < 0 || slice_bytes < 0) return 0;
    // every factor is tested before the product it enters, so no product below can overflow 64 bits
    if (X >= b24 || Y >= b24 || Z >= b24 || MX >= b24 || MY >= b24 || MZ >= b24) return 0;
    if (X * Y >= b24 || MX * MY >= b24) return 0;
    if (X * Y * Z * 4 >= b32) return 0;
    if (MX * MY * MZ >= b32) return 0;
    if (occ_bytes >= b32 || slice_bytes >= b32) return 0;
    return 1;
}
#endif
