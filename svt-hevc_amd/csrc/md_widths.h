/* md_widths.h - the launch widths of k_md_picture (md_kernels.hip): how many workgroups a picture's mode-decision launch gets.  One text for the blocking entries
 * (svt_amd_md_encode_picture*: MdFlight grants `lone`, `wide` or `narrow`) and for svt_amd_md_encode_picture_launch (`lone` or `narrow`), and for the host
 * (tools/md_widths_check.c: a plain C program, tests/test_md_widths_cpu.py pins the widths).  Plain C: no HIP, no environment - md_launch_widths (md_picture.hip) reads
 * the measurement overrides and passes them in. */
#ifndef SVT_AMD_MD_WIDTHS_H
#define SVT_AMD_MD_WIDTHS_H

#define MD_WIDTH_MAX 224

typedef struct MdWidths {
    int lone;   /* a launch that finds the device without any other mode-decision launch */
    int wide;   /* a device that is shared, but nearly idle */
    int narrow; /* what the launch gets while other pictures share the device */
} MdWidths;

/* wl x hl: the picture in LCUs; tiles: its tile count (0 counts as 1); n_active: the LCUs the launch decides (the picture's, or a rank rectangle's);
 * forced / fnarrow / fwide: the measurement overrides SVT_AMD_MD_GRID / _NARROW / _WIDE, 0 = none */
static inline MdWidths md_widths(int wl, int hl, int tiles, int n_active, int forced, int fnarrow, int fwide)
{
    /* the wavefront is at most min((W/64 + 1) / 2, H/64) LCUs wide; the mode decision runs ahead of the encode pass, so twice that many workgroups
     * find work (all of them resident: a workgroup that waits holds its CU) */
    /* ... but a workgroup holds a whole CU (its LDS) while it waits, and the encoder keeps several pictures in flight: five 62-workgroup launches do not fit the 256 CUs.
     * The wavefront of a picture is (W/64 + 1) / 2 LCUs wide at its widest and 16 on average at 4K; one workgroup per LCU of the widest front plus a few for the encode
     * passes behind it costs a lone picture 3 - 4 % and lets six pictures' launches run side by side (profiles/r04_w_md_flights_*: the kernel keeps its 51 ms with
     * twelve calls in flight, 100 pictures/s - given enough hardware queues, svt_amd_runtime_env_defaults). */
    /* Round 6: a lone picture on an idle device gets two workgroups per LCU of the widest front again - behind an LCU's decisions its workgroup spends ~15 % of the LCU's
     * time on the merge / skip decisions with chroma and the work record, ahead of them on the next LCU's inputs, and with one workgroup per LCU of the front a ready LCU
     * waits for a workgroup (4K: 40 / 48 / 56 / 64 workgroups = 27.1 / 27.05 / 26.85 / 26.7 ms for a layer-2 picture).  The widths a launch gets while other pictures' launches
     * are on the device - the encoder's steady state - stay what round 5 measured best (40 / 20 at 4K). */
    const int front = ((wl + 1) / 2 < hl ? (wl + 1) / 2 : hl) * (tiles > 0 ? tiles : 1);
    MdWidths w;
    w.lone = 2 * front + 2;
    w.wide = front + 2 + (wl + 7) / 8;
    w.narrow = (w.wide + 1) / 2 < 8 ? 8 : (w.wide + 1) / 2;
    if (forced > 0)
        w.lone = w.wide = w.narrow = forced;
    if (fnarrow > 0)
        w.narrow = fnarrow;
    if (fwide > 0)
        w.lone = w.wide = fwide;
    /* no more workgroups than LCUs, and never more than MD_WIDTH_MAX.  (Until round 30 the two limits were tried in turn, `w > n_active ? n_active : w > 224 ? 224 : w`,
     * which let a launch of 225 or more LCUs whose formula asked for still more have one workgroup per LCU: 960x960 in 16 tiles got 225.) */
    const int cap = n_active < MD_WIDTH_MAX ? n_active : MD_WIDTH_MAX;
    w.wide = w.wide > cap ? cap : w.wide;
    w.lone = w.lone > cap ? cap : w.lone;
    w.lone = w.lone < w.wide ? w.wide : w.lone;
    w.narrow = w.narrow > w.wide ? w.wide : w.narrow;
    return w;
}

#endif
