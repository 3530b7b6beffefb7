/* tail_logic_check.c - the per-LCU routine of the picture tail (svt-hevc_amd/csrc/tail_logic.h) as a plain C program, so that it can run under
 * -fsanitize=address,undefined over fixtures and over malformed records before the same text runs on a device (tests/test_tail_cpu.py builds and runs it).
 *   tail_logic_check IN OUT
 * IN:  int32 width, height, lcus, then per LCU the 1584 bytes of head and unit list and the 768 bytes of SvtAmdLcuResult.cu.
 * OUT: the picture-sized map (12 bytes a cell), cbf and QP arrays assembled from the tiles as the kernel stores them, then edge, SAO edge, follow and status bytes
 *      ([lcus] each) and the 16-byte check record.  Every array is a heap block of its exact size: an index that leaves it is reported. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../svt-hevc_amd/csrc/tail_logic.h"

#define REC (TAIL_W_SRC + TAIL_MAX_CUS * TAIL_R_CU_BYTES)

static int fail(const char *what)
{
    fprintf(stderr, "tail_logic_check: %s\n", what);
    return 2;
}

int main(int argc, char **argv)
{
    if (argc != 3)
        return fail("usage: tail_logic_check IN OUT");
    FILE *in = fopen(argv[1], "rb");
    int32_t hdr[3];
    if (!in || fread(hdr, sizeof(hdr), 1, in) != 1)
        return fail("cannot read the input");
    const int w = hdr[0], h = hdr[1], n = hdr[2], cols = (w + 63) / 64, rows = (h + 63) / 64;
    if (w < 8 || h < 8 || (w & 7) || (h & 7) || n != cols * rows)
        return fail("bad header");
    uint8_t *rec = malloc((size_t)n * REC);
    if (!rec || fread(rec, REC, (size_t)n, in) != (size_t)n)
        return fail("short input");
    fclose(in);
    const int w8 = w / 8, h8 = h / 8;
    uint32_t *map = malloc((size_t)w8 * h8 * 12);
    uint8_t *qp = malloc((size_t)w8 * h8), *cbf = malloc((size_t)w8 * h8 * 4), *bytes = malloc((size_t)n * 4);
    if (!map || !qp || !cbf || !bytes)
        return fail("no memory");
    TailCheckSums sums = tail_check_none();
    for (int i = 0; i < n; i++) {
        /* the record in a block of its own: a read behind head and unit list, or behind the 64 result entries, is reported */
        uint8_t *work = malloc(TAIL_W_SRC), *res = malloc(TAIL_MAX_CUS * TAIL_R_CU_BYTES);
        TailTile *T = malloc(sizeof(*T));
        if (!work || !res || !T)
            return fail("no memory");
        memcpy(work, rec + (size_t)i * REC, TAIL_W_SRC);
        memcpy(res, rec + (size_t)i * REC + TAIL_W_SRC, TAIL_MAX_CUS * TAIL_R_CU_BYTES);
        const int below = i + cols < n ? rec[(size_t)(i + cols) * REC + TAIL_W_TILE_TOP] : 0;
        tail_lcu_build(work, res, below, i, cols, n, w, h, T, 0, 1);
        const int lx8 = (i % cols) * 8, ly8 = (i / cols) * 8, cw = w8 - lx8 < 8 ? w8 - lx8 : 8, ch = h8 - ly8 < 8 ? h8 - ly8 : 8;
        for (int r = 0; r < ch; r++) {
            memcpy(map + ((size_t)(ly8 + r) * w8 + lx8) * 3, T->map + r * 24, (size_t)cw * 12);
            memcpy(qp + (size_t)(ly8 + r) * w8 + lx8, T->qp + r * 8, (size_t)cw);
        }
        for (int r = 0; r < 2 * ch; r++)
            memcpy(cbf + (size_t)(2 * ly8 + r) * (2 * w8) + 2 * lx8, T->cbf + r * 16, (size_t)cw * 2);
        bytes[i] = T->edge, bytes[n + i] = T->sao_edge, bytes[2 * n + i] = T->follow, bytes[3 * n + i] = T->status;
        sums = tail_check_add(sums, (uint32_t)i, T->status);
        free(work), free(res), free(T);
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out || fwrite(map, 12, (size_t)w8 * h8, out) != (size_t)w8 * h8 || fwrite(cbf, 4, (size_t)w8 * h8, out) != (size_t)w8 * h8 ||
        fwrite(qp, 1, (size_t)w8 * h8, out) != (size_t)w8 * h8 || fwrite(bytes, 4, (size_t)n, out) != (size_t)n || fwrite(&sums, sizeof(sums), 1, out) != 1 || fclose(out))
        return fail("cannot write the output");
    free(rec), free(map), free(qp), free(cbf), free(bytes);
    return 0;
}
