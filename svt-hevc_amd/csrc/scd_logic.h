/* scd_logic.h - the rules of SceneTransitionDetector (Codec/EbPictureDecisionProcess.c:73-258) on records, restated as the reference has them and repaired nowhere
 * (include/svt_hevc_amd.h "Batched scene-transition detection"; tests/scd_numpy.py spells every width out): the vote threshold, the region size the loops
 * accumulate, the region thresholds, and the step of ONE region - its class and its new running averages.  One text for the device (scd_kernels.hip:
 * k_scd_decide, a lane per region) and for the host (tools/scd_logic_check.c: a plain C program under the sanitizers), as tail_logic.h and md_logic.h do.
 * Integer logic; 32-bit unsigned arithmetic wraps where the reference's EB_U32 does. */
#ifndef SVT_AMD_SCD_LOGIC_H
#define SVT_AMD_SCD_LOGIC_H
#include <stdint.h>

#ifndef SCD_FN
#define SCD_FN static inline
#endif

#define SCD_MAX_REGIONS 16
#define SCD_BINS 256
/* the branch a region took: = SVT_AMD_SCD_CLASS_* */
#define SCD_NONE 0
#define SCD_GRADUAL 1
#define SCD_FLASH 2
#define SCD_FADE 3
#define SCD_SCENE 4

/* regionCountThreshold (:126-128): (EB_U32)((float)(regions * P) / 100 + 0.5), P = 75 for SCD_MODE_2 and 50 otherwise.  regions * P is an integer below 2^24 and
 * exact as a float; its hundredth is a multiple of 1 / 2 (P = 50) or of 1 / 4 (P = 75) below 16 and exact as well, so nothing is rounded before the
 * truncation and the value is floor(regions * P / 100 + 1 / 2) = (regions * P + 50) / 100:
 *   regions   1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16
 *   P = 50    1  1  2  2  3  3  4  4  5  5  6  6  7  7  8  8
 *   P = 75    1  2  2  3  4  5  5  6  7  8  8  9 10 11 11 12
 * (tests/golden/make_scd_golden.py records the reference's own 32 values; tests/test_scd_cpu.py compares) */
SCD_FN uint32_t scd_vote_threshold(uint32_t regions, uint32_t scd_mode) { return (regions * (scd_mode == 2 ? 75u : 50u) + 50u) / 100u; }

/* regionWidth / regionHeight after `steps` runs of `size += total - regions * size` (:147-156) from size = total / regions.  With e = regions * size - total a step
 * is e -> (1 - regions) * e, so size_k = q + rem * (1 + (1 - regions) + .. + (1 - regions)^(k - 1)), q and rem the quotient and the remainder of total / regions;
 * every term is an integer, so the form holds modulo 2^32 where the reference's EB_U32 wraps (a size below 0 is a large unsigned number there, and here) */
SCD_FN uint32_t scd_accumulated(uint32_t total, uint32_t regions, uint32_t steps)
{
    const uint32_t q = total / regions, rem = total - regions * q, ratio = 1u - regions;
    uint32_t sum = 0, power = 1;
    for (uint32_t k = 0; k < steps; k++)
        sum += power, power *= ratio;
    return q + rem * sum;
}
/* the size in use at iteration (wi, hi), wi the outer loop: the width steps once per iteration of the last column, the height once per column in its last row */
SCD_FN uint32_t scd_region_width(uint32_t w, uint32_t rw, uint32_t wi, uint32_t hi) { return scd_accumulated(w, rw, wi == rw - 1 ? hi + 1 : 0); }
SCD_FN uint32_t scd_region_height(uint32_t h, uint32_t rh, uint32_t wi, uint32_t hi) { return scd_accumulated(h, rh, wi + (hi == rh - 1)); }

/* NOISY_SCENE_TH / SCENE_TH (:158-163) */
SCD_FN uint32_t scd_scene_th(uint32_t cur_variance, uint32_t past_variance)
{
    const uint32_t step = cur_variance > past_variance ? cur_variance - past_variance : past_variance - cur_variance;
    return step > 390u && (cur_variance > 1500u || past_variance > 1500u) ? 4500u : 3000u;
}
/* regionThreshHold of iteration (wi, hi): T * NUM64x64INPIC(regionWidth, regionHeight); regionThreshHoldChroma is a quarter of it */
SCD_FN uint32_t scd_region_threshold(uint32_t w, uint32_t h, uint32_t rw, uint32_t rh, uint32_t wi, uint32_t hi, uint32_t scene_th)
{
    return scene_th * ((scd_region_width(w, rw, wi, hi) * scd_region_height(h, rh, wi, hi)) >> 12);
}

/* ABS((EB_S32)a - (EB_S32)b) as an EB_U32 */
SCD_FN uint32_t scd_abs_diff(uint32_t a, uint32_t b)
{
    const int32_t d = (int32_t)(a - b);
    return d < 0 ? 0u - (uint32_t)d : (uint32_t)d;
}
/* (EB_U8)ABS((EB_S16)a - (EB_S16)b) of two bytes */
SCD_FN uint32_t scd_aid(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

/* one region of one call (:174-232): ahd[3] the sums of luma, Cb, Cr; avg[3] the running averages, updated in place; reset: resetRunningAvg as the call found
 * it; th / th_chroma of this iteration; the luma averageIntensityPerRegion of the past, the current and the future picture.  -> the class */
SCD_FN uint32_t scd_region(const uint32_t ahd[3], uint32_t avg[3], uint32_t reset, uint32_t th, uint32_t th_chroma, uint32_t past, uint32_t cur, uint32_t future)
{
    if (reset)
        avg[0] = ahd[0], avg[1] = ahd[1], avg[2] = ahd[2];
    const uint32_t err = scd_abs_diff(avg[0], ahd[0]), err_cb = scd_abs_diff(avg[1], ahd[1]), err_cr = scd_abs_diff(avg[2], ahd[2]);
    const int abrupt = (err > th && ahd[0] >= err) || (err_cb > th_chroma && ahd[1] >= err_cb) || (err_cr > th_chroma && ahd[2] >= err_cr);
    if (abrupt) { /* the luma average stays */
        const uint32_t fp = scd_aid(future, past), fpr = scd_aid(future, cur), pp = scd_aid(cur, past);
        return fp < 5u && fpr >= 5u && pp >= 5u ? SCD_FLASH : fpr < 3u && pp < 3u ? SCD_FADE : SCD_SCENE;
    }
    const int gradual = err > (th >> 1) && ahd[0] >= err;
    avg[0] = (3u * avg[0] + ahd[0]) / 4u; /* both arms of the gradual branch and the last arm (:221, :226, :231) */
    return gradual ? SCD_GRADUAL : SCD_NONE;
}

#endif
