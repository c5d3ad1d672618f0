"""ViT-L/14@336px without a GPU: the model strings, the 577-token architecture, the size of its weight blob, and the attention
dispatch (csrc/clipx_attn_plan.h) driven by a stand-alone program under the sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "clip-retrieval_amd", "csrc", "clipx_attn_plan.h")


@pytest.mark.parametrize("name", ["ViT-L/14@336px", "open_clip:ViT-L-14-336/openai", "open_clip:ViT-L-14-336",
                                  "hf_clip:openai/clip-vit-large-patch14-336"])
def test_model_strings_resolve(name):
    from clip_retrieval_amd.encoder import ARCHS, resolve_arch_name

    assert resolve_arch_name(name) == "ViT-L/14@336px"
    assert "ViT-L/14@336px" in ARCHS


def test_the_224_strings_still_resolve_to_the_224_model():
    """A guard, not a test of new code: the first three lines pass before the 336 model existed.  The last one runs the new
    open_clip table with a pretrained tag it does not hold."""
    from clip_retrieval_amd.encoder import resolve_arch_name

    assert resolve_arch_name("open_clip:ViT-L-14/openai") == "ViT-L/14"
    assert resolve_arch_name("hf_clip:openai/clip-vit-large-patch14") == "ViT-L/14"
    assert resolve_arch_name("open_clip:ViT-L-14/laion2b_s32b_b82k") == "open_clip:ViT-L-14"
    with pytest.raises(ValueError):
        resolve_arch_name("open_clip:ViT-L-14-336/laion2b")  # open_clip has OpenAI's weights only for this architecture


def test_arch_is_vit_l14_at_577_tokens():
    from clip_retrieval_amd.encoder import ARCHS, ClipArch

    a = ARCHS["ViT-L/14@336px"]
    assert a.v_tokens == 577 and a.image_size == 336
    assert a == ClipArch(image_size=336)  # everything else is ViT-L/14
    assert a.v_width // a.v_heads == 64 and a.ctx_len == 77


def test_blob_floats_of_the_two_layer_336_model():
    """clipx_blob_floats (host arithmetic of the library) against the length of the blob the oracle exports: the positional table
    has 577 rows, everything else is the 224 model's.  The function was generic in the image size before the 336 model came, so this
    records that it is, and covers no new code."""
    from clip_retrieval_amd.encoder import ClipArch, blob_floats
    from oracle.clip_oracle import ClipArch as OracleArch
    from oracle.clip_oracle import HFClipOracle

    arch = OracleArch(image_size=336, v_layers=2, t_layers=2)
    blob = HFClipOracle(arch, seed=0).export_blob()
    n = blob_floats(ClipArch(image_size=336, v_layers=2, t_layers=2))
    assert n == blob.size == 79_948_544
    assert n - blob_floats(ClipArch(v_layers=2, t_layers=2)) == (577 - 257) * 1024


def test_model_desc_limits():
    """check_desc, reached without a device through clipx_create with a blob of the wrong length: a description it accepts comes
    back as CLIPX_E_ARG (the blob), one it refuses as CLIPX_E_UNSUPPORTED, both before the first HIP call.  608 image tokens at head
    dimension 64, 288 at head dimension 80, and the text context stays at 288."""
    import numpy as np

    from clip_retrieval_amd import load_library
    from clip_retrieval_amd.encoder import ClipArch

    lib = load_library()
    E_ARG, E_UNSUPPORTED = -1, -5
    one = np.zeros(1, np.float32)

    def create(**kw):
        d, h = ClipArch(**kw).to_desc(), C.c_void_p()
        rc = lib.clipx_create(C.byref(d), one.ctypes.data, 1, 0, C.byref(h))
        assert not h.value
        return rc, lib.clipx_last_error().decode()

    assert create(image_size=336)[0] == E_ARG                    # 577 tokens
    assert create(image_size=336, patch_size=16)[0] == E_ARG     # 442
    assert create(image_size=336, patch_size=14, v_width=1024, v_heads=16)[0] == E_ARG
    assert create(v_width=1280)[0] == E_ARG                      # 257 tokens at head dimension 80 (ViT-H/14)
    rc, msg = create(image_size=350)                             # 626 tokens
    assert rc == E_UNSUPPORTED and "608" in msg
    rc, msg = create(image_size=336, v_width=1280)               # 577 tokens at head dimension 80
    assert rc == E_UNSUPPORTED and "288" in msg
    assert create(image_size=238, v_width=1280)[0] == E_UNSUPPORTED  # 290 tokens at head dimension 80
    rc, msg = create(ctx_len=300)
    assert rc == E_UNSUPPORTED and "288" in msg


def test_attention_entry_points_refuse_before_any_launch():
    """The T limits are checked before the device is touched, so the refusals can be seen without one (the pointers are never read)."""
    from clip_retrieval_amd import load_library

    lib = load_library()
    fake = C.c_void_p(4096)
    for T, dh, causal, word in ((609, 64, 0, "608"), (300, 64, 1, "288"), (577, 80, 0, "288"), (700, 80, 1, "608")):
        if dh == 64:
            assert lib.clipx_attention_device(0, fake, fake, 1, T, 1, causal, None) == -5
            assert word in lib.clipx_last_error().decode()
        assert lib.clipx_attention_dh_device(0, fake, fake, 1, T, 1, dh, causal, None) == -5
        assert word in lib.clipx_last_error().decode()


def test_dispatch_under_sanitizers(tmp_path):
    """tools/attn_plan_check.cpp (its own main, only clipx_attn_plan.h) built with -fsanitize=address,undefined and run as a child:
    every T in 1 .. 700 x dh in {64, 80} x causal in {0, 1} -- the old decision for T <= 288, the long-sequence kernel exactly for
    dh 64, not causal, 289 .. 608, refusal elsewhere, LDS <= 163 840 bytes, every query block below q_blocks owned by one wave."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "attn_plan_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "clip-retrieval_amd", "csrc"), os.path.join(ROOT, "tools", "attn_plan_check.cpp"), "-o", exe]
    build = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("attn plan ok") and "FAILED" not in run.stdout
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("plan dh")]
    assert len(lines) == 4
    assert "320 long" in lines[0] and all("  0 long" in ln for ln in lines[1:])  # 289 .. 608 = 320 lengths, dh 64 not causal only


def test_dispatch_header_has_no_hip():
    text = open(HEADER, encoding="utf-8").read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(inc.startswith("<") and "hip" not in inc for inc in includes), includes  # system headers only, none of HIP's
    assert "__global__" not in text and "__device__" not in text and "hipStream" not in text and "hipError" not in text
