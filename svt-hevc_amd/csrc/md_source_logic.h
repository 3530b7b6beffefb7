/* md_source_logic.h - the row arithmetic of k_md_source (mdlaunch_kernels.hip): a caller's source plane, at the caller's pitch and alignment, into the picture
 * object's own plane, and for 16-bit samples the 8-MSB view (sample >> 2) beside it.  One text for the device and for the host (tools/md_source_check.c: a plain C
 * program over seeded shapes, every plane in a heap block of its exact size), as tail_logic.h does with TAIL_FN.
 *
 * A row of `row_bytes` bytes (a multiple of 4: plane widths are multiples of 4 samples) is a list of independent ITEMS:
 *   where the source row, the destination row (both 16-byte aligned) and the view row (8-byte aligned) allow it, row_bytes / 16 CHUNKS of 16 bytes, then the
 *   (row_bytes % 16) / 4 dwords of the row's tail;
 *   otherwise row_bytes / 4 dwords.
 * Item i of a row touches bytes [o, o + 16) or [o, o + 4) of source and destination and samples-many bytes of the view, o from mdsrc_item: nothing before byte 0 or
 * behind byte row_bytes of a row is read or written.  Source pointers, row starts and pitches are 4-byte aligned (the entry checks them), so every dword access is
 * aligned; a 16-bit dword is two samples, its view a 2-byte store at an even offset. */
#ifndef SVT_AMD_MD_SOURCE_LOGIC_H
#define SVT_AMD_MD_SOURCE_LOGIC_H
#include <stdint.h>

#ifndef MDSRC_FN
#define MDSRC_FN static inline
#endif

typedef struct MdSrcRow {
    uint32_t chunks;      /* whole 16-byte chunks at the row's start */
    uint32_t items;       /* chunks + the dwords behind them */
} MdSrcRow;
typedef struct __attribute__((aligned(16))) MdSrc128 { uint32_t w[4]; } MdSrc128;
typedef struct __attribute__((aligned(8))) MdSrc64 { uint32_t w[2]; } MdSrc64;

/* view: the view row's address, or 0 (8-bit samples: no view) */
MDSRC_FN MdSrcRow mdsrc_row(uintptr_t src, uintptr_t dst, uintptr_t view, uint32_t row_bytes)
{
    MdSrcRow r;
    const int wide = ((src | dst) & 15u) == 0 && (view & 7u) == 0;
    r.chunks = wide ? row_bytes >> 4 : 0u;
    r.items = r.chunks + ((row_bytes - (r.chunks << 4)) >> 2);
    return r;
}

/* the four 8-MSB bytes of two dwords of 16-bit samples */
MDSRC_FN uint32_t mdsrc_msb4(uint32_t a, uint32_t b)
{
    return ((a >> 2) & 0xffu) | ((a >> 10) & 0xff00u) | (((b >> 2) & 0xffu) << 16) | (((b >> 18) & 0xffu) << 24);
}

/* item i < r.items of a row.  bps: bytes per sample (1 or 2); view: the view row for bps == 2, unused otherwise */
MDSRC_FN void mdsrc_item(const uint8_t *src, uint8_t *dst, uint8_t *view, MdSrcRow r, uint32_t i, int bps)
{
    if (i < r.chunks) {
        const uint32_t o = i << 4;
        const MdSrc128 v = *(const MdSrc128 *)(src + o);
        *(MdSrc128 *)(dst + o) = v;
        if (bps == 2) {
            MdSrc64 m;
            m.w[0] = mdsrc_msb4(v.w[0], v.w[1]), m.w[1] = mdsrc_msb4(v.w[2], v.w[3]);
            *(MdSrc64 *)(view + (o >> 1)) = m;
        }
    } else {
        const uint32_t o = (r.chunks << 4) + ((i - r.chunks) << 2);
        const uint32_t v = *(const uint32_t *)(src + o);
        *(uint32_t *)(dst + o) = v;
        if (bps == 2)
            *(uint16_t *)(view + (o >> 1)) = (uint16_t)(((v >> 2) & 0xffu) | ((v >> 10) & 0xff00u));
    }
}

#endif
