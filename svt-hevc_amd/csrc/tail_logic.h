/* tail_logic.h - the filter inputs of ONE LCU from its contract records, as the host loops of svt_amd_encdec_picture_deblock / _sao derive them
 * (encdec_kernels.hip:picture_deblock, :picture_sao; tests/tail_numpy.py restates both): the coding unit per 8x8 block, the QP per 8x8 block, the luma cbf per 4x4 block,
 * the deblocking edge byte, the SAO edge flags, the `follow` bits of the encoder-order composite and the LCU's status byte.  One text for the device
 * (tail_kernels.hip: a workgroup per LCU, the tile in LDS) and for the host (tools/tail_logic_check.c: a plain C program over fixtures and malformed records),
 * as md_logic.h does with MD_FN.  Integer logic on bytes; no sample is read.
 *
 * The routine is written for `lanes` cooperating callers (lane = 0 .. lanes - 1; the host calls it with lane 0 of 1): every phase is a loop "item = lane; item < n;
 * item += lanes" over independent items, TAIL_SYNC() between the phases.  Cells are GATHERED - a cell walks the unit list and keeps the LAST unit that covers it -
 * so that the later unit in list order wins as on the host, without atomics and without an order among the lanes; a cell no unit covers is 0.
 *
 * What is counted instead of refused (the host loops return SVT_AMD_ERR_BAD_PARAM; the kernel cannot): an LCU that is not at its raster position or has
 * num_cus > 64 (status bit 7; none of its units is looked at, all its cells are 0, its source samples are not scattered), and per unit (status bits 0..6: how many)
 * a size other than 8 / 16 / 32 / 64, a unit that leaves its LCU (x + size > 64 or y + size > 64), one that leaves the picture, and a 64x64 unit whose four result
 * slots c + 1 .. c + 4 leave the result record.  An offending unit writes nothing.  With these checks no index leaves the tile or the records.
 * The three flag bytes need no geometry and are derived for every LCU. */
#ifndef SVT_AMD_TAIL_LOGIC_H
#define SVT_AMD_TAIL_LOGIC_H
#include <stdint.h>

#ifndef TAIL_FN
#define TAIL_FN static inline
#endif
#ifndef TAIL_SYNC
#define TAIL_SYNC() do { } while (0)
#endif

/* byte offsets inside SvtAmdLcuWork / SvtAmdLcuWork16 (shared head and unit list), SvtAmdLcuCu and SvtAmdLcuResult[16] (tail_kernels.hip asserts them) */
#define TAIL_W_LCU_X 0
#define TAIL_W_LCU_Y 2
#define TAIL_W_NUM_CUS 4
#define TAIL_W_TILE_LEFT 9
#define TAIL_W_TILE_TOP 10
#define TAIL_W_TILE_RIGHT 11
#define TAIL_W_CU 48
#define TAIL_W_SRC 1584
#define TAIL_CU_BYTES 24
#define TAIL_CU_X 0
#define TAIL_CU_Y 1
#define TAIL_CU_SIZE 2
#define TAIL_CU_MODE 3
#define TAIL_CU_QP 7
#define TAIL_CU_DIR 10
#define TAIL_CU_MV 16
#define TAIL_R_CU_BYTES 12   /* SvtAmdLcuCuResult; cbf[0] is its first byte */
#define TAIL_MAX_CUS 64
#define TAIL_LCU_BAD 0x80u

typedef struct TailTile {
    uint32_t map[64 * 3];   /* SvtAmdCuMapEntry of the 8x8 cells of the LCU, raster, 12 bytes each: {mode, dir, size_log2, 0}, mv[0], mv[1] */
    uint8_t qp[64];         /* QP of the 8x8 cells */
    uint8_t cbf[256];       /* luma cbf of the 4x4 cells */
    uint32_t geo[TAIL_MAX_CUS]; /* per unit: x | y << 8 | size << 16 | taken << 24 - one word a step of the walks */
    uint8_t status;         /* TAIL_LCU_BAD, or the number of offending units */
    uint8_t edge;           /* deblocking: tile_left | tile_top << 1 */
    uint8_t sao_edge;       /* SvtAmdSaoLcuParams.edge_flags: 1 left, 2 right, 4 top, 8 bottom */
    uint8_t follow;         /* k_tail_composite: bit 0 an LCU of the same tile follows to the right, bit 1 below */
} TailTile;

typedef struct TailCheckSums { uint32_t bad_lcus, first_bad_lcu, bad_units, first_bad_unit_lcu; } TailCheckSums; /* = SvtAmdTailCheck */

TAIL_FN uint32_t tail_u16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
TAIL_FN uint32_t tail_u32(const uint8_t *p) { return tail_u16(p) | tail_u16(p + 2) << 16; }

/* 0 = the unit is taken; anything else = it is counted and writes nothing */
TAIL_FN int tail_unit_bad(const uint8_t *cu, int c, int lcu_x, int lcu_y, int width, int height)
{
    const int x = cu[TAIL_CU_X], y = cu[TAIL_CU_Y], s = cu[TAIL_CU_SIZE];
    if (s != 8 && s != 16 && s != 32 && s != 64)
        return 1;
    if (x + s > 64 || y + s > 64)
        return 2;
    if (lcu_x + x + s > width || lcu_y + y + s > height)
        return 3;
    if (s == 64 && c + 4 >= TAIL_MAX_CUS)
        return 4;
    return 0;
}

/* work: head and unit list of LCU `lcu` (1584 bytes); below_tile_top: works[lcu + lcu_cols].tile_top (any value in the last LCU row); res_cu: SvtAmdLcuResult.cu of the
 * LCU (64 x 12 bytes, read in place).  width and height are multiples of 8. */
TAIL_FN void tail_lcu_build(const uint8_t *work, const uint8_t *res_cu, int below_tile_top, int lcu, int lcu_cols, int lcus, int width, int height, TailTile *T, int lane,
                            int lanes)
{
    const int ox = (lcu % lcu_cols) * 64, oy = (lcu / lcu_cols) * 64;
    const int num = work[TAIL_W_NUM_CUS];
    const int lcu_bad = (int)tail_u16(work + TAIL_W_LCU_X) != ox || (int)tail_u16(work + TAIL_W_LCU_Y) != oy || num > TAIL_MAX_CUS;
    const int count = lcu_bad ? 0 : num;

    /* phase 1: which units are taken */
    for (int c = lane; c < TAIL_MAX_CUS; c += lanes) {
        const uint8_t *cu = work + TAIL_W_CU + c * TAIL_CU_BYTES;
        const uint32_t taken = c < count && !tail_unit_bad(cu, c, ox, oy, width, height);
        T->geo[c] = (uint32_t)cu[TAIL_CU_X] | (uint32_t)cu[TAIL_CU_Y] << 8 | (uint32_t)cu[TAIL_CU_SIZE] << 16 | taken << 24;
    }
    TAIL_SYNC();

    /* phase 2: items 0..255 the 4x4 cells (cbf) - the cell in the top-left corner of an 8x8 cell speaks for that cell too (map entry and QP), in the same walk -
     * and item 256 the flags and the status */
    for (int item = lane; item <= 256; item += lanes) {
        if (item < 256) {
            const int cx = item & 15, cy = item >> 4;
            int v = 0, unit = -1;
            for (int c = 0; c < count; c++) {
                const uint32_t g = T->geo[c];
                const int x = (int)(g & 0xFFu), y = (int)(g >> 8 & 0xFFu), s = (int)(g >> 16 & 0xFFu);
                if (!(g >> 24))
                    continue;
                if (cx >= x >> 2 && cx < (x + s) >> 2 && cy >= y >> 2 && cy < (y + s) >> 2) {
                    /* a 64x64 unit: four 32x32 transform units, result entries c + 1 .. c + 4, one per quadrant */
                    const int slot = s == 64 ? c + 1 + 2 * (cy >> 3) + (cx >> 3) : c;
                    v = res_cu[slot * TAIL_R_CU_BYTES];
                }
                if (cx >> 1 >= x >> 3 && cx >> 1 < (x + s) >> 3 && cy >> 1 >= y >> 3 && cy >> 1 < (y + s) >> 3)
                    unit = c;
            }
            T->cbf[item] = (uint8_t)v;
            if (!(cx & 1) && !(cy & 1)) {
                const int cell = (cy >> 1) * 8 + (cx >> 1);
                uint32_t e0 = 0, e1 = 0, e2 = 0, q = 0;
                if (unit >= 0) {
                    const uint8_t *cu = work + TAIL_W_CU + unit * TAIL_CU_BYTES;
                    const uint32_t s = cu[TAIL_CU_SIZE], mode = cu[TAIL_CU_MODE], lg = s == 8 ? 3u : s == 16 ? 4u : s == 32 ? 5u : 6u;
                    const int inter = mode == 1; /* inter: the prediction unit's direction and vectors decide the strength of its edges */
                    e0 = mode | (inter ? (uint32_t)cu[TAIL_CU_DIR] << 8 : 0u) | lg << 16;
                    e1 = inter ? tail_u32(cu + TAIL_CU_MV) : 0u;
                    e2 = inter ? tail_u32(cu + TAIL_CU_MV + 4) : 0u;
                    q = cu[TAIL_CU_QP];
                }
                T->map[cell * 3] = e0, T->map[cell * 3 + 1] = e1, T->map[cell * 3 + 2] = e2;
                T->qp[cell] = (uint8_t)q;
            }
        } else {
            const int left = work[TAIL_W_TILE_LEFT] != 0, top = work[TAIL_W_TILE_TOP] != 0, right = work[TAIL_W_TILE_RIGHT] != 0;
            const int bottom = lcu + lcu_cols >= lcus || below_tile_top;
            T->edge = (uint8_t)(left | top << 1);
            T->sao_edge = (uint8_t)(left | right << 1 | top << 2 | bottom << 3);
            T->follow = (uint8_t)(((lcu % lcu_cols) + 1 < lcu_cols && !right ? 1 : 0) | (!bottom ? 2 : 0));
            int bad = 0;
            for (int c = 0; c < count; c++)
                bad += !(T->geo[c] >> 24);
            T->status = (uint8_t)(lcu_bad ? TAIL_LCU_BAD : (unsigned)bad);
        }
    }
    TAIL_SYNC();
}

/* the status bytes of lcus [first, first + n) folded into `acc` (start it with tail_check_none) */
TAIL_FN TailCheckSums tail_check_none(void)
{
    TailCheckSums s;
    s.bad_lcus = 0, s.first_bad_lcu = 0xFFFFFFFFu, s.bad_units = 0, s.first_bad_unit_lcu = 0xFFFFFFFFu;
    return s;
}
TAIL_FN TailCheckSums tail_check_add(TailCheckSums a, uint32_t lcu, uint8_t status)
{
    if (status & TAIL_LCU_BAD) {
        a.bad_lcus++;
        a.first_bad_lcu = lcu < a.first_bad_lcu ? lcu : a.first_bad_lcu;
    } else if (status) {
        a.bad_units += status;
        a.first_bad_unit_lcu = lcu < a.first_bad_unit_lcu ? lcu : a.first_bad_unit_lcu;
    }
    return a;
}
TAIL_FN TailCheckSums tail_check_merge(TailCheckSums a, TailCheckSums b)
{
    a.bad_lcus += b.bad_lcus, a.bad_units += b.bad_units;
    a.first_bad_lcu = b.first_bad_lcu < a.first_bad_lcu ? b.first_bad_lcu : a.first_bad_lcu;
    a.first_bad_unit_lcu = b.first_bad_unit_lcu < a.first_bad_unit_lcu ? b.first_bad_unit_lcu : a.first_bad_unit_lcu;
    return a;
}
#endif
