#!/usr/bin/env python3
"""Generate the temporal-motion-field fixtures from the REFERENCE itself.

Runs oracle/_ref/SvtHevcEncApp_ref with SVT_REF_MD_DUMP and SVT_REF_ENCODEPASS_DUMP set, as make_md_golden.py:run_case does (its cases, its parser): the first
records, per picture that goes through ModeDecisionLcu (a READER), the co-located motion field the reference's mode decision read (tmvpMap of the co-located
reference object) and the picture's inter controls; the second records the final coding tree of every LCU of every picture as EncodePass walked it, with the
picture's refPOC per list.  Per case -> tests/golden/tmvp_<case>.npz, results only:
  q_*    for every co-located picture q a recorded reader names: q_poc, q_heads (the work records of q up to the source samples: num_cus, slice_type,
         temporal_layer, cu[64] ...; no samples), q_ref_poc, q_slice_type, q_tmvp (the raw recorded field of ONE reader, q_reader)
  r_*    for every reader: r_poc, r_colocated_poc, r_skip_cost_bias, r_is_reference, r_slice_type, r_ref_poc
  pic_*  for every picture of the encode: pic_poc, pic_slice_type, pic_layer, pic_area_sum and pic_area
The generator asserts that every LCU of q has an EncodePass record, that ref_poc is the same in all of them and that two readers of the same q agree on the
observable fields (tests/tmvp_numpy.py:observable).
pic_area is the reference's own: a small C driver of our own text, written into a temporary directory, #includes Codec/EbEncDecProcess.c by path (the function is
`static`), links against oracle/_ref/libsvtref.so and calls CopyStatisticsToRefObject on a calloc'd control set whose intraCodedArea is pic_area_sum; what the
reference object then holds is stored.  pic_area_sum ITSELF is stated here, in the generator's words (the sum of size^2 over the units with pred_mode == 2 of the
picture's EncodePass records): the reference accumulates it inside EncodePass (Codec/EbCodingLoop.c:3264-3269, :3574), which cannot be called on records.
Nothing compiled is kept.  Needs the reference tree and `make -C oracle ref`.  Usage: python tests/golden/make_tmvp_golden.py [case ...]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_encodepass_golden as EPG  # noqa: E402
import make_md_golden as MDG  # noqa: E402
import svtlib as S  # noqa: E402
import tmvp_numpy as N  # noqa: E402
import tmvplib as T  # noqa: E402

REF_SRC = os.environ.get("SVT_REF_SOURCE", "/root/reference/Source")
CASES = ("b_objects_416x240_m8", "p_objects_320x192_m8_ld", "b_xc_binary_200x136_m8_q51", "bref_tiles_motion_640x384_m8", "b_noise_320x256_m9_q24")

DRIVER = r"""
#include "EbEncDecProcess.c"
#include <stdio.h>
int main(int argc, char **argv)
{
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    uint32_t n, in[4];
    if (argc < 3 || !fi || !fo || fread(&n, 4, 1, fi) != 1) return 2;
    for (uint32_t i = 0; i < n; i++) {
        if (fread(in, 4, 4, fi) != 4) return 3;
        PictureControlSet_t *pcs = calloc(1, sizeof(*pcs));
        PictureParentControlSet_t *ppcs = calloc(1, sizeof(*ppcs));
        SequenceControlSet_t *scs = calloc(1, sizeof(*scs));
        EbObjectWrapper_t *wrap = calloc(3, sizeof(*wrap));
        EbReferenceObject_t *obj = calloc(3, sizeof(*obj));
        for (int k = 0; k < 3; k++) wrap[k].objectPtr = &obj[k];
        pcs->ParentPcsPtr = ppcs, ppcs->referencePictureWrapperPtr = &wrap[0];
        pcs->refPicPtrArray[0] = &wrap[1], pcs->refPicPtrArray[1] = &wrap[2];
        obj[0].intraCodedArea = 0xA5;
        pcs->intraCodedArea = in[0], scs->lumaWidth = in[1], scs->lumaHeight = in[2], pcs->sliceType = in[3];
        CopyStatisticsToRefObject(pcs, scs);
        if (fwrite(&obj[0].intraCodedArea, 1, 1, fo) != 1) return 4;
    }
    fclose(fo);
    return 0;
}
"""


def _compile(td, name, text):
    ref_dir = os.path.dirname(S.REF_SO)
    inc = [ref_dir] + [os.path.join(REF_SRC, d) for d in ("API", "Lib/Codec", "Lib/C_DEFAULT", "Lib/ASM_SSE2", "Lib/ASM_SSSE3", "Lib/ASM_SSE4_1", "Lib/ASM_AVX2")]
    src, exe = os.path.join(td, name + ".c"), os.path.join(td, name)
    with open(src, "w") as f:
        f.write(text)
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-mavx2", "-msse4.1", "-w"] + ["-I" + i for i in inc] +
                          [src, "-o", exe, "-L" + ref_dir, "-lsvtref", "-Wl,-rpath," + ref_dir, "-lpthread", "-lm"])
    return exe


def reference_areas(exe, td, rows):
    """rows: (area_sum, w, h, slice_type) -> what CopyStatisticsToRefObject leaves in the reference object"""
    fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([len(rows)], "<u4").tobytes() + np.array(rows, "<u4").tobytes())
    subprocess.check_call([exe, fin, fout])
    out = np.fromfile(fout, np.uint8)
    assert len(out) == len(rows)
    return out


def run_case(name, exe, td):
    kind, w, h, n, seed, args = MDG.CASES[name][:6]
    yuv, dump, epdump = os.path.join(td, "clip.yuv"), os.path.join(td, "md.dump"), os.path.join(td, "ep.dump")
    S.write_clip(yuv, kind, w, h, n, seed)
    cmd = [S.REF_APP, "-i", yuv, "-w", str(w), "-h", str(h), "-n", str(n), "-asm", "0", "-b", os.path.join(td, "out.265")] + args
    subprocess.run(cmd, env=dict(os.environ, SVT_REF_MD_DUMP=dump, SVT_REF_ENCODEPASS_DUMP=epdump), check=True, stdout=subprocess.DEVNULL)
    pics, _ = MDG.parse_dump(open(dump, "rb").read())
    ep, _, _ = EPG.parse_dump(open(epdump, "rb").read(), S.EP_RECORD_DTYPE)
    nl = S.lcu_count(w, h)

    # every picture of the encode: its trees, its area
    trees = {}
    for poc in sorted(set(ep["picture_number"].tolist())):
        r = ep[ep["picture_number"] == poc]
        r = r[np.argsort(r["lcu_index"], kind="stable")]
        assert np.array_equal(r["lcu_index"], np.arange(nl)), "picture %d: not every LCU has an EncodePass record" % poc
        assert (r["ref_poc"] == r["ref_poc"][0]).all(), "picture %d: ref_poc differs between its records" % poc
        assert (r["work"]["slice_type"] == r["work"]["slice_type"][0]).all() and (r["work"]["temporal_layer"] == r["work"]["temporal_layer"][0]).all()
        heads = np.zeros(nl, T.WORK_HEAD_DTYPE)
        for f in T.WORK_HEAD_DTYPE.names:
            heads[f] = r["work"][f]
        trees[poc] = (heads, r["ref_poc"][0].copy())
    pocs = sorted(trees)
    rows = []
    for poc in pocs:
        heads = trees[poc][0]
        total = 0
        for hd in heads:                        # the generator's words: size^2 of the units EncodePass coded as intra
            for cu in hd["cu"][:int(hd["num_cus"])]:
                if cu["pred_mode"] == 2:
                    total += int(cu["size"]) ** 2
        rows.append((total, w, h, int(heads[0]["slice_type"])))
    areas = reference_areas(exe, td, rows)

    # the readers and the co-located pictures they name
    readers = [p for p in sorted(pics) if pics[p][5] is not None and pics[p][5][1] is not None and pics[p][0]["inter"]["tmvp_enable"]]
    assert readers, "no picture read a co-located motion field"
    by_q = {}
    for p in readers:
        by_q.setdefault(int(pics[p][0]["inter"]["colocated_poc"]), []).append(p)
    qs = sorted(by_q)
    q_tmvp = []
    for q in qs:
        assert q in trees, "co-located picture %d has no EncodePass records" % q
        first = pics[by_q[q][0]][5][1]
        for p in by_q[q][1:]:                   # two readers of the same q agree on what they can see
            assert N.mismatches(pics[p][5][1], first, w, h) == 0 and N.mismatches(first, pics[p][5][1], w, h) == 0, (q, by_q[q][0], p)
        q_tmvp.append(np.array(first))
    everyone = [p for p in sorted(pics) if pics[p][5] is not None]
    out = {
        "clip": np.array([kind, str(w), str(h), str(n), str(seed)]), "enc_args": np.array(args),
        "q_poc": np.array(qs, np.uint64), "q_heads": np.stack([trees[q][0] for q in qs]), "q_ref_poc": np.stack([trees[q][1] for q in qs]).astype(np.uint64),
        "q_slice_type": np.array([trees[q][0][0]["slice_type"] for q in qs], np.uint8), "q_tmvp": np.stack(q_tmvp),
        "q_reader": np.array([by_q[q][0] for q in qs], np.uint64),
        "r_poc": np.array(everyone, np.uint64), "r_colocated_poc": np.array([pics[p][0]["inter"]["colocated_poc"] for p in everyone], np.uint64),
        "r_tmvp_enable": np.array([pics[p][0]["inter"]["tmvp_enable"] for p in everyone], np.uint8),
        "r_skip_cost_bias": np.array([pics[p][0]["inter"]["skip_cost_bias"] for p in everyone], np.uint8),
        "r_is_reference": np.array([pics[p][0]["pic"]["is_reference"] for p in everyone], np.uint8),
        "r_slice_type": np.array([pics[p][0]["pic"]["slice_type"] for p in everyone], np.uint8),
        "r_ref_poc": np.stack([pics[p][0]["inter"]["ref_poc"] for p in everyone]).astype(np.uint64),
        "pic_poc": np.array(pocs, np.uint64), "pic_slice_type": np.array([r[3] for r in rows], np.uint8),
        "pic_layer": np.array([trees[p][0][0]["temporal_layer"] for p in pocs], np.uint8), "pic_area_sum": np.array([r[0] for r in rows], np.uint32),
        "pic_area": areas,
    }
    path = os.path.join(S.GOLDEN_DIR, "tmvp_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("%-30s %dx%d, %d LCUs: co-located pictures %s (slice types %s) read by %s; areas %s -> %s (%.1f KiB)" %
          (name, w, h, nl, qs, out["q_slice_type"].tolist(), [by_q[q] for q in qs], areas.tolist(), os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    if not os.path.exists(S.REF_APP) or not os.path.isdir(os.path.join(REF_SRC, "Lib", "Codec")):
        sys.exit("needs oracle/_ref (`make -C oracle ref`) and the reference's sources (SVT_REF_SOURCE, default /root/reference/Source)")
    with tempfile.TemporaryDirectory() as tmp:
        driver = _compile(tmp, "driver", DRIVER)
        for nm in (sys.argv[1:] or CASES):
            run_case(nm, driver, tmp)
