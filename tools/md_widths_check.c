/* md_widths_check.c - the launch widths of the mode-decision picture kernel (svt-hevc_amd/csrc/md_widths.h) as a plain C program, built by tests/test_md_widths_cpu.py
 * with -fsanitize=address,undefined (a signed overflow in the arithmetic ends the program).
 *   md_widths_check {<wl> <hl> <tiles> <n_active> <forced> <fnarrow> <fwide>} ...        prints "lone wide narrow" per case
 *   md_widths_check sweep <wl max> <hl max>      every wl x hl up to the maxima x tiles {1, 2, 4, 16} x n_active {1, n / 2 (at least 1), n}, no overrides:
 *                                                "wl hl tiles n_active lone wide narrow" per point */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../svt-hevc_amd/csrc/md_widths.h"

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "sweep")) {
        static const int tiles[4] = {1, 2, 4, 16};
        const int wmax = atoi(argv[2]), hmax = atoi(argv[3]);
        for (int wl = 1; wl <= wmax; wl++)
            for (int hl = 1; hl <= hmax; hl++)
                for (int t = 0; t < 4; t++) {
                    const int n = wl * hl, active[3] = {1, n / 2 > 1 ? n / 2 : 1, n};
                    for (int a = 0; a < 3; a++) {
                        const MdWidths w = md_widths(wl, hl, tiles[t], active[a], 0, 0, 0);
                        printf("%d %d %d %d %d %d %d\n", wl, hl, tiles[t], active[a], w.lone, w.wide, w.narrow);
                    }
                }
        return 0;
    }
    if (argc < 8 || (argc - 1) % 7)
        return 2;
    for (int k = 1; k < argc; k += 7) {
        const MdWidths w = md_widths(atoi(argv[k]), atoi(argv[k + 1]), atoi(argv[k + 2]), atoi(argv[k + 3]), atoi(argv[k + 4]), atoi(argv[k + 5]), atoi(argv[k + 6]));
        printf("%d %d %d\n", w.lone, w.wide, w.narrow);
    }
    return 0;
}
