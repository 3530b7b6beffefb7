/* md_source_check.c - the row arithmetic of k_md_source (svt-hevc_amd/csrc/md_source_logic.h) as a plain C program, built by tests/test_mdlaunch_cpu.py with
 * -fsanitize=address,undefined: a plane at a caller's pitch and base offset into a plane at the object's pitch, every plane in a heap block of its exact size, so
 * that an access before a row's first or behind its last byte - or a misaligned one - ends the program.
 *   md_source_check {<bytes per sample> <width> <rows> <source pitch> <base offset in bytes> <destination pitch> <seed>} ...     (pitches in samples)
 * compares with a row-by-row memcpy (and sample >> 2 for the view of 16-bit samples), and checks that nothing between the rows of the destination was written.
 * The lanes of a wave are a loop: item = lane, lane + 64, ... as the kernel walks a row. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../svt-hevc_amd/csrc/md_source_logic.h"

#define FILL 0xA5

static int run(char **argv)
{
    const int bps = atoi(argv[1]);
    const uint32_t width = (uint32_t)atoi(argv[2]), rows = (uint32_t)atoi(argv[3]), sp = (uint32_t)atoi(argv[4]), base = (uint32_t)atoi(argv[5]), dp = (uint32_t)atoi(argv[6]);
    uint32_t seed = (uint32_t)atoi(argv[7]);
    if ((bps != 1 && bps != 2) || !width || !rows || sp < width || dp < width || base % 4 || (sp * (uint32_t)bps) % 4 || (width * (uint32_t)bps) % 4)
        return 2;
    const size_t row_bytes = (size_t)width * (size_t)bps, sbytes = (size_t)sp * (size_t)bps, dbytes = (size_t)dp * (size_t)bps;
    /* exact sizes: the last row ends the block */
    const size_t src_size = base + sbytes * (rows - 1) + row_bytes, dst_size = dbytes * (rows - 1) + row_bytes, view_size = (size_t)dp * (rows - 1) + width;
    uint8_t *src = malloc(src_size), *dst = malloc(dst_size), *view = bps == 2 ? malloc(view_size) : NULL;
    if (!src || !dst || (bps == 2 && !view))
        return 3;
    for (size_t i = 0; i < src_size; i++) {
        seed = seed * 1664525u + 1013904223u;
        src[i] = (uint8_t)(seed >> 24);
    }
    if (bps == 2) /* 10-bit samples */
        for (size_t i = 1; i < src_size; i += 2)
            src[i] &= 3;
    memset(dst, FILL, dst_size);
    if (view)
        memset(view, FILL, view_size);
    uint32_t chunk_rows = 0;
    for (uint32_t y = 0; y < rows; y++) {
        const uint8_t *s = src + base + (size_t)y * sbytes;
        uint8_t *d = dst + (size_t)y * dbytes, *v = view ? view + (size_t)y * dp : NULL;
        const MdSrcRow r = mdsrc_row((uintptr_t)s, (uintptr_t)d, (uintptr_t)v, (uint32_t)row_bytes);
        chunk_rows += r.chunks != 0;
        for (uint32_t lane = 0; lane < 64; lane++)
            for (uint32_t i = lane; i < r.items; i += 64)
                mdsrc_item(s, d, v, r, i, bps);
    }
    int bad = 0;
    for (uint32_t y = 0; y < rows && !bad; y++) {
        const uint8_t *s = src + base + (size_t)y * sbytes;
        if (memcmp(dst + (size_t)y * dbytes, s, row_bytes))
            bad = 1;
        for (size_t i = row_bytes; y + 1 < rows && i < dbytes; i++)
            if (dst[(size_t)y * dbytes + i] != FILL)
                bad = 2;
        if (view) {
            for (uint32_t x = 0; x < width; x++)
                if (view[(size_t)y * dp + x] != (uint8_t)((s[2 * x] | s[2 * x + 1] << 8) >> 2))
                    bad = 3;
            for (size_t i = width; y + 1 < rows && i < dp; i++)
                if (view[(size_t)y * dp + i] != FILL)
                    bad = 4;
        }
    }
    printf("%u\n", chunk_rows); /* rows that took the 16-byte path */
    free(src), free(dst), free(view);
    return bad ? 10 + bad : 0;
}

int main(int argc, char **argv)
{
    if (argc < 8 || (argc - 1) % 7)
        return 2;
    for (int k = 1; k < argc; k += 7) {
        const int rc = run(argv + k - 1);
        if (rc) {
            fprintf(stderr, "case %d: %d\n", (k - 1) / 7, rc);
            return rc;
        }
    }
    return 0;
}
