"""GPU, whole encoder: an encMode 9 encode at the 4K input class (2688x1024: luma area >= INPUT_SIZE_4K_TH), where the reference codes every P / B picture above temporal
layer 0 WITHOUT sub-sample search (useSubpelFlag = (temporalLayerIndex == 0), Codec/EbPictureDecisionProcess.c:334).  With the library's defaults (no SVT_HOOK_* switch:
the closed loop of the P / B pictures on the device) the drop-in encoder hands exactly those pictures to the device call - the interpolation-free instance of the kernel -
and its bitstream is the unmodified reference's.  The clip is the fixtures' own (tests/md_ifree_clip.py)."""
import hashlib
import os
import re
import subprocess

import pytest

import md_ifree_clip as CLIP
import svtlib as S

pytestmark = pytest.mark.gpu
W, H, N = CLIP.WIDTH, CLIP.HEIGHT, CLIP.FRAMES
ARGS = ["-encMode", "9"]


def encode(app, yuv, out, env=None):
    r = subprocess.run([app, "-i", yuv, "-w", str(W), "-h", str(H), "-n", str(N), "-b", out, "-asm", "1", "-q", "32"] + ARGS, capture_output=True, text=True, timeout=400,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return hashlib.md5(open(out, "rb").read()).hexdigest()


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    assert os.path.exists(S.HIP_APP) and os.path.exists(S.REF_APP), \
        "oracle/_ref/hooked and oracle/_ref must be prebuilt (python __graft_entry__.py build, needs the reference sources)"
    d = tmp_path_factory.mktemp("ifree_e2e")
    yuv = str(d / "clip.yuv")
    CLIP.write_clip(yuv)
    return d, yuv, encode(S.REF_APP, yuv, str(d / "ref.265"))


def test_the_reference_agrees_with_itself(clip):
    """the control of the comparison below: a second encode of the unmodified reference gives the first one's bitstream (no rate control: nothing depends on timing)"""
    d, yuv, ref_md5 = clip
    assert encode(S.REF_APP, yuv, str(d / "ref2.265")) == ref_md5


def test_bitstream_identical_and_every_picture_above_layer_0_on_the_device(clip):
    d, yuv, ref_md5 = clip
    assert not [k for k in os.environ if k.startswith("SVT_HOOK_")], "this case runs the library's defaults"
    rp = str(d / "report.txt")
    hip_md5 = encode(S.HIP_APP, yuv, str(d / "hip.265"), {"SVT_HOOK_REPORT": rp})
    rep = open(rp).read()
    m = re.search(r"mode decision: (\d+) pictures \((\d+) of them P / B; (\d+) LCUs\).*?; (\d+) pictures outside", rep)
    assert m, rep
    pics, inter, lcus, left = (int(v) for v in m.groups())
    print("MD_COUNTS ifree", N, pics, inter, left)
    # 9 pictures of the default prediction structure (random access, three hierarchical levels): the I picture (not offered to the device call at the default
    # SVT_HOOK_MD=pb, and not counted) and ONE base-layer B picture (picture 8: closed-loop intra, the reference code's) - every other picture lies above layer 0, is coded
    # without sub-sample search, and must be inside the device call
    assert (pics, inter, left) == (N - 2, N - 2, 1) and lcus == pics * S.lcu_count(W, H), rep
    assert hip_md5 == ref_md5, "bitstream differs from the reference\n" + rep
    assert os.path.getsize(str(d / "hip.265")) > 100
