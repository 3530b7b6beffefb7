/* inter_ifree_check.c - the positions of the interpolation-free inter prediction of pictures coded without sub-sample search (svt-hevc_amd/csrc/inter_position.h:
 * inter_mv_round, inter_mv_round2, inter_ifree_luma_x / _y, inter_ifree_chroma) as a plain C program, built by tests/test_md_ifree_cpu.py with
 * -fsanitize=address,undefined (a signed overflow or a shift of a negative value ends the program).
 *   inter_ifree_check round <v> ...
 *       prints inter_mv_round(v) per value
 *   inter_ifree_check sweep <width> <height> <origin>
 *       unit positions 0 .. 192 in steps of 8 (x and y together) x vectors {-32768, -5, -3, -2, -1, 0, 1, 2, 3, 5, 6, 7, 32767}^2, per case one line:
 *       "at mv_x mv_y  rx ry  r2x r2y  qx qy lx ly cx cy  Qx Qy Lx Ly Cx Cy"
 *       rx ry: the rounded components; r2x r2y: the halves of the packed rounding; q..: the clamped position of the vector AS IT IS, its interpolation-free luma sample
 *       and its nearest chroma sample; Q..: the same of the rounded vector (what the mode decision predicts from) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../svt-hevc_amd/csrc/inter_position.h"

static void position(int at, int mvx, int mvy, int o, int w, int h)
{
    const int qx = INTER_POS_CLAMP(at, o, mvx, w), qy = INTER_POS_CLAMP(at, o, mvy, h);
    printf(" %d %d %d %d %d %d", qx, qy, inter_ifree_luma_x(qx, qy), inter_ifree_luma_y(qx, qy), inter_ifree_chroma(qx), inter_ifree_chroma(qy));
}

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "round")) {
        for (int k = 2; k < argc; k++)
            printf("%d\n", inter_mv_round(atoi(argv[k])));
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "sweep")) {
        static const int mvs[13] = {-32768, -5, -3, -2, -1, 0, 1, 2, 3, 5, 6, 7, 32767};
        const int w = atoi(argv[2]), h = atoi(argv[3]), o = atoi(argv[4]);
        for (int at = 0; at <= 192; at += 8)
            for (int a = 0; a < 13; a++)
                for (int b = 0; b < 13; b++) {
                    const int rx = inter_mv_round(mvs[a]), ry = inter_mv_round(mvs[b]);
                    const unsigned r2 = inter_mv_round2((unsigned)(uint16_t)mvs[a] | ((unsigned)(uint16_t)mvs[b] << 16));
                    printf("%d %d %d %d %d %d %d", at, mvs[a], mvs[b], rx, ry, (int)(int16_t)(r2 & 0xFFFFu), (int)(int16_t)(r2 >> 16));
                    position(at, mvs[a], mvs[b], o, w, h);
                    position(at, rx, ry, o, w, h);
                    printf("\n");
                }
        return 0;
    }
    return 2;
}
