/* scd_logic_check.c - the rules of the batched scene-transition detection (svt-hevc_amd/csrc/scd_logic.h) as a plain C program, so that the text the device
 * compiles runs under -fsanitize=address,undefined over the planted cases first (tests/test_scd_cpu.py builds and runs it; tests/scd_records.py:write_case writes
 * its input).  The jobs run in order, as the second kernel walks them.
 *   scd_logic_check IN OUT
 * IN:  int32 width, height, regions_w, regions_h, scd_mode, jobs, has_state; with has_state the 196 bytes of an SvtAmdScdState; then per job the luma histograms
 *      of the past and of the current picture ([regions][256] uint32 each), their chroma histograms ([regions][2][256] each), the luma average bytes of the past,
 *      the current and the future picture ([regions] each) and pic_avg_variance of the past and of the current picture (uint16 each).
 * OUT: the three output arrays of svt_amd_scene_detect_batch_launch: SvtAmdScdPic[jobs], uint32[jobs][16][3], SvtAmdScdState[jobs].
 * Every record and every output is a heap block of its exact size: an index that leaves it is reported. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../svt-hevc_amd/csrc/scd_logic.h"

#define PIC_BYTES 24
#define STATE_BYTES 196
#define AHD_WORDS (SCD_MAX_REGIONS * 3)

static int fail(const char *what)
{
    fprintf(stderr, "scd_logic_check: %s\n", what);
    return 2;
}

static void *take(FILE *in, size_t bytes)
{
    void *p = malloc(bytes);
    if (!p || fread(p, 1, bytes, in) != bytes) {
        fail("short input");
        exit(2);
    }
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 3)
        return fail("usage: scd_logic_check IN OUT");
    FILE *in = fopen(argv[1], "rb");
    int32_t hdr[7];
    if (!in || fread(hdr, sizeof(hdr), 1, in) != 1)
        return fail("cannot read the input");
    const uint32_t w = (uint32_t)hdr[0], h = (uint32_t)hdr[1], rw = (uint32_t)hdr[2], rh = (uint32_t)hdr[3], mode = (uint32_t)hdr[4], regions = rw * rh;
    const int jobs = hdr[5];
    if (hdr[0] < 8 || hdr[1] < 8 || hdr[2] < 1 || hdr[2] > 4 || hdr[3] < 1 || hdr[3] > 4 || hdr[4] < 1 || hdr[4] > 2 || jobs < 1 || jobs > 256)
        return fail("bad header");
    uint32_t avg[SCD_MAX_REGIONS][3] = {{0}}, reset = 1;
    if (hdr[6]) {
        uint8_t *s = take(in, STATE_BYTES);
        for (uint32_t r = 0; r < regions; r++)
            for (int k = 0; k < 3; k++)
                memcpy(&avg[r][k], s + 64 * k + 4 * r, 4);
        reset = s[192] != 0;
        free(s);
    }
    uint8_t *pics = calloc((size_t)jobs, PIC_BYTES), *states = calloc((size_t)jobs, STATE_BYTES);
    uint32_t *ahds = calloc((size_t)jobs * AHD_WORDS, 4);
    if (!pics || !states || !ahds)
        return fail("no memory");
    const uint32_t vote = scd_vote_threshold(regions, mode);
    for (int i = 0; i < jobs; i++) {
        uint32_t *past_luma = take(in, (size_t)regions * SCD_BINS * 4), *cur_luma = take(in, (size_t)regions * SCD_BINS * 4);
        uint32_t *past_chroma = take(in, (size_t)regions * 2 * SCD_BINS * 4), *cur_chroma = take(in, (size_t)regions * 2 * SCD_BINS * 4);
        uint8_t *past_avg = take(in, regions), *cur_avg = take(in, regions), *future_avg = take(in, regions);
        uint16_t *variance = take(in, 4); /* past, current */
        const uint32_t scene_th = scd_scene_th(variance[1], variance[0]);
        uint32_t abrupt = 0, scene = 0;
        uint8_t *p = pics + (size_t)i * PIC_BYTES, *s = states + (size_t)i * STATE_BYTES;
        for (uint32_t r = 0; r < regions; r++) {
            uint32_t *ahd = ahds + (size_t)i * AHD_WORDS + r * 3; /* the first stage: a sum per plane */
            for (uint32_t b = 0; b < SCD_BINS; b++) {
                ahd[0] += scd_abs_diff(cur_luma[r * SCD_BINS + b], past_luma[r * SCD_BINS + b]);
                ahd[1] += scd_abs_diff(cur_chroma[r * 2 * SCD_BINS + b], past_chroma[r * 2 * SCD_BINS + b]);
                ahd[2] += scd_abs_diff(cur_chroma[(r * 2 + 1) * SCD_BINS + b], past_chroma[(r * 2 + 1) * SCD_BINS + b]);
            }
            const uint32_t th = scd_region_threshold(w, h, rw, rh, r / rh, r % rh, scene_th);
            const uint32_t cls = scd_region(ahd, avg[r], reset, th, th / 4u, past_avg[r], cur_avg[r], future_avg[r]);
            abrupt += cls >= SCD_FLASH, scene += cls == SCD_SCENE;
            p[8 + r] = (uint8_t)cls;
        }
        reset = abrupt >= vote;
        p[0] = scene >= vote, p[1] = (uint8_t)reset, p[2] = (uint8_t)abrupt, p[3] = (uint8_t)scene, p[4] = (uint8_t)vote;
        for (uint32_t r = 0; r < regions; r++)
            for (int k = 0; k < 3; k++)
                memcpy(s + 64 * k + 4 * r, &avg[r][k], 4);
        s[192] = (uint8_t)reset;
        free(past_luma), free(cur_luma), free(past_chroma), free(cur_chroma), free(past_avg), free(cur_avg), free(future_avg), free(variance);
    }
    fclose(in);
    FILE *out = fopen(argv[2], "wb");
    if (!out || fwrite(pics, PIC_BYTES, (size_t)jobs, out) != (size_t)jobs || fwrite(ahds, AHD_WORDS * 4, (size_t)jobs, out) != (size_t)jobs ||
        fwrite(states, STATE_BYTES, (size_t)jobs, out) != (size_t)jobs || fclose(out))
        return fail("cannot write the output");
    free(pics), free(states), free(ahds);
    return 0;
}
