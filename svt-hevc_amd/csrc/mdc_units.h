/*
 * mdc_units.h - the 85 coded units of an LCU in MD-scan order as the leaf-list kernels see them (k_mdc_leaves of mdc_kernels.hip, k_mdctl_lcu of
 * mdctl_kernels.hip): a set of units as two wave-uniform words, and GetCodedUnitStats of one unit.  Device code only; every function is inlined.
 */
#ifndef SVT_AMD_MDC_UNITS_H
#define SVT_AMD_MDC_UNITS_H
#include <hip/hip_runtime.h>

/* a set of the 85 coded units in MD-scan order: two wave-uniform words */
struct MdcSet {
    unsigned long long lo, hi; /* units 0..63, units 64..84 */
};
__device__ __forceinline__ bool mdc_in(const MdcSet &s, int u) { return u >= 0 && ((u < 64 ? s.lo >> u : s.hi >> (u - 64)) & 1ull); }
/* the set of the units whose lane says yes: lane b speaks for unit b (first) and, below 21, for unit 64 + b (second) */
__device__ __forceinline__ MdcSet mdc_set(bool first, bool second)
{
    MdcSet s;
    s.lo = __ballot(first), s.hi = __ballot(second) & 0x1FFFFFull;
    return s;
}

/* GetCodedUnitStats (Codec/EbUtility.c) of MD-scan unit cu: depth, origin, the raster-scan index of the ME records, and its ancestors (-1: none) */
struct MdcUnit {
    int depth, x, y, raster, parent, grand, great;
};
__device__ __forceinline__ MdcUnit mdc_unit(int cu)
{
    MdcUnit u;
    u.depth = 0, u.x = 0, u.y = 0, u.raster = 0, u.parent = -1, u.grand = -1, u.great = -1;
    if (cu > 0) {
        const int c = cu - 1, q1 = c / 21, r1 = c % 21, p1 = 1 + q1 * 21;
        u.x = (q1 & 1) * 32, u.y = (q1 >> 1) * 32;
        if (r1 == 0)
            u.depth = 1, u.raster = 1 + q1, u.parent = 0;
        else {
            const int c2 = r1 - 1, q2 = c2 / 5, r2 = c2 % 5, p2 = p1 + 1 + q2 * 5;
            u.x += (q2 & 1) * 16, u.y += (q2 >> 1) * 16;
            if (r2 == 0)
                u.depth = 2, u.raster = 5 + (u.y >> 4) * 4 + (u.x >> 4), u.parent = p1, u.grand = 0;
            else {
                const int q3 = r2 - 1;
                u.x += (q3 & 1) * 8, u.y += (q3 >> 1) * 8;
                u.depth = 3, u.raster = 21 + (u.y >> 3) * 8 + (u.x >> 3), u.parent = p2, u.grand = p1, u.great = 0;
            }
        }
    }
    return u;
}

#endif
