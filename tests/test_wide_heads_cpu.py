"""ViT-g/14 and ViT-bigG/14 without a GPU: the model strings, the shapes and parameter counts, the state-dict loaders at the new
widths, the model-description limits, and the attention dispatch of head dimensions 88 / 104 (csrc/clipx_attn_plan.h) driven by a
stand-alone program under the sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, BIGG = "open_clip:ViT-g-14", "open_clip:ViT-bigG-14"


def test_the_six_new_spellings_resolve():
    from clip_retrieval_amd.encoder import ARCHS, resolve_arch_name

    assert G in ARCHS and BIGG in ARCHS
    assert resolve_arch_name("open_clip:ViT-g-14") == G
    assert resolve_arch_name("open_clip:ViT-g-14/laion2b_s12b_b42k") == G
    assert resolve_arch_name("hf_clip:laion/CLIP-ViT-g-14-laion2B-s12B-b42K") == G
    assert resolve_arch_name("open_clip:ViT-bigG-14") == BIGG
    assert resolve_arch_name("open_clip:ViT-bigG-14/laion2b_s39b_b160k") == BIGG
    assert resolve_arch_name("hf_clip:laion/CLIP-ViT-bigG-14-laion2B-39B-b160k") == BIGG
    for unknown in ("open_clip:ViT-e-14/laion2b", "hf_clip:laion/CLIP-ViT-G-14", "ViT-bigG/14"):
        with pytest.raises(ValueError):
            resolve_arch_name(unknown)
    assert resolve_arch_name("open_clip:ViT-H-14/laion2b_s32b_b79k") == "open_clip:ViT-H-14"  # and the neighbours stay put


def _param_count(a):
    """parameters of the two towers, from the shapes alone (biases and LayerNorms included, as the checkpoints hold them)"""
    def tower(w, mlp, layers):
        return layers * (2 * w + 3 * w * w + 3 * w + w * w + w + 2 * w + mlp * w + mlp + w * mlp + w)

    image = a.v_width * 3 * a.patch_size ** 2 + a.v_width + a.v_tokens * a.v_width + 2 * a.v_width \
        + tower(a.v_width, a.v_mlp, a.v_layers) + 2 * a.v_width + a.embed_dim * a.v_width
    text = a.vocab * a.t_width + a.ctx_len * a.t_width + tower(a.t_width, a.t_mlp, a.t_layers) + 2 * a.t_width + a.embed_dim * a.t_width
    return image + text


@pytest.mark.parametrize("name,dh,embed,billions", [(G, 88, 1024, 1.37), (BIGG, 104, 1280, 2.54)])
def test_archs_have_the_shapes_of_the_table(name, dh, embed, billions):
    from clip_retrieval_amd.encoder import ARCHS, blob_floats

    a = ARCHS[name]
    assert a.v_width // a.v_heads == dh and a.v_width % a.v_heads == 0 and a.t_width // a.t_heads == 64
    assert (a.patch_size, a.image_size, a.v_tokens, a.ctx_len, a.vocab, a.act, a.embed_dim) == (14, 224, 257, 77, 49408, "gelu", embed)
    assert a.v_width % 128 == 0 and a.v_width % 256 == 128  # an odd multiple of 128: what the row-wise kernels had to learn
    n = _param_count(a)
    print(f"{name}: {n} parameters ({n / 1e9:.4f} B)")
    assert abs(n / 1e9 - billions) < 0.01 * billions
    assert blob_floats(a) == n  # the library's own host arithmetic (clipx_blob_floats) agrees


def _two_layer(name):
    """the two-layer arch of the model (a small vocabulary: the token table is the one part whose shape has nothing new)"""
    from dataclasses import replace

    from clip_retrieval_amd.encoder import ARCHS

    return replace(ARCHS[name], v_layers=2, t_layers=2, vocab=1024)


def _oracle_arch(arch):
    from oracle.clip_oracle import ClipArch

    return ClipArch(**{k: getattr(arch, k) for k in ClipArch.__dataclass_fields__})


@pytest.mark.parametrize("name", [G, BIGG])
def test_state_dict_loaders_at_the_new_widths(name):
    """Synthetic OpenAI / open_clip and HF state dicts cut from one blob: both loaders give back exactly that blob, i.e. what
    oracle.clip_oracle.unpack_blob sees in their output is the tensors the state dicts were made of."""
    import torch

    from clip_retrieval_amd.encoder import blob_floats, blob_from_hf_state_dict, blob_from_openai_state_dict
    from oracle.clip_oracle import unpack_blob

    arch = _two_layer(name)
    oarch = _oracle_arch(arch)
    n = blob_floats(arch)
    blob = np.random.default_rng(7).random(n, dtype=np.float32)
    W = unpack_blob(blob, oarch)
    w, P = arch.v_width, arch.patch_size
    openai, hf = {}, {}
    openai["visual.conv1.weight"] = W["conv"].reshape(w, 3, P, P)
    openai["visual.class_embedding"], openai["visual.positional_embedding"] = W["cls"], W["vpos"]
    openai["visual.ln_pre.weight"], openai["visual.ln_pre.bias"] = W["ln_pre_w"], W["ln_pre_b"]
    openai["visual.ln_post.weight"], openai["visual.ln_post.bias"] = W["ln_post_w"], W["ln_post_b"]
    openai["visual.proj"] = W["vproj"].T.contiguous()
    openai["token_embedding.weight"], openai["positional_embedding"] = W["tok"], W["tpos"]
    openai["ln_final.weight"], openai["ln_final.bias"] = W["ln_final_w"], W["ln_final_b"]
    openai["text_projection"] = W["tproj"].T.contiguous()
    v, t = "vision_model", "text_model"
    hf[v + ".embeddings.patch_embedding.weight"] = W["conv"].reshape(w, 3, P, P)
    hf[v + ".embeddings.class_embedding"], hf[v + ".embeddings.position_embedding.weight"] = W["cls"], W["vpos"]
    hf[v + ".pre_layrnorm.weight"], hf[v + ".pre_layrnorm.bias"] = W["ln_pre_w"], W["ln_pre_b"]
    hf[v + ".post_layernorm.weight"], hf[v + ".post_layernorm.bias"] = W["ln_post_w"], W["ln_post_b"]
    hf["visual_projection.weight"] = W["vproj"]
    hf[t + ".embeddings.token_embedding.weight"], hf[t + ".embeddings.position_embedding.weight"] = W["tok"], W["tpos"]
    hf[t + ".final_layer_norm.weight"], hf[t + ".final_layer_norm.bias"] = W["ln_final_w"], W["ln_final_b"]
    hf["text_projection.weight"] = W["tproj"]
    for o_pre, h_pre, layers in (("visual.transformer", v, W["vlayers"]), ("transformer", t, W["tlayers"])):
        for l, L in enumerate(layers):
            width = L["out_w"].shape[0]
            po, ph = f"{o_pre}.resblocks.{l}.", f"{h_pre}.encoder.layers.{l}."
            for ok, hk, key in (("ln_1.weight", "layer_norm1.weight", "ln1_w"), ("ln_1.bias", "layer_norm1.bias", "ln1_b"),
                                ("attn.out_proj.weight", "self_attn.out_proj.weight", "out_w"), ("attn.out_proj.bias", "self_attn.out_proj.bias", "out_b"),
                                ("ln_2.weight", "layer_norm2.weight", "ln2_w"), ("ln_2.bias", "layer_norm2.bias", "ln2_b"),
                                ("mlp.c_fc.weight", "mlp.fc1.weight", "fc1_w"), ("mlp.c_fc.bias", "mlp.fc1.bias", "fc1_b"),
                                ("mlp.c_proj.weight", "mlp.fc2.weight", "fc2_w"), ("mlp.c_proj.bias", "mlp.fc2.bias", "fc2_b")):
                openai[po + ok] = hf[ph + hk] = L[key]
            openai[po + "attn.in_proj_weight"], openai[po + "attn.in_proj_bias"] = L["qkv_w"], L["qkv_b"]
            for i, x in enumerate("qkv"):
                hf[ph + f"self_attn.{x}_proj.weight"] = L["qkv_w"][i * width:(i + 1) * width]
                hf[ph + f"self_attn.{x}_proj.bias"] = L["qkv_b"][i * width:(i + 1) * width]
    for what, got in (("openai", blob_from_openai_state_dict(openai, arch)), ("hf", blob_from_hf_state_dict(hf, arch))):
        assert got.dtype == np.float32 and got.shape == (n,), what
        W2 = unpack_blob(got, oarch)
        assert torch.equal(W2["vproj"], W["vproj"]) and torch.equal(W2["vlayers"][1]["qkv_w"], W["vlayers"][1]["qkv_w"]), what
        assert torch.equal(W2["tlayers"][1]["fc2_w"], W["tlayers"][1]["fc2_w"]) and torch.equal(W2["tproj"], W["tproj"]), what
        assert np.array_equal(got, blob), what
        del got, W2


def test_random_blob_has_the_length_of_the_new_archs():
    from clip_retrieval_amd.encoder import blob_floats, random_blob

    arch = _two_layer(G)
    blob = random_blob(arch, 3)
    assert blob.dtype == np.float32 and blob.size == blob_floats(arch) and np.isfinite(blob[:: 4099]).all()


def test_model_desc_limits_of_the_wide_heads():
    """check_desc, reached without a device through clipx_create with a blob of the wrong length (tests/test_long_seq_cpu.py): a
    description it accepts comes back as CLIPX_E_ARG (the blob), one it refuses as CLIPX_E_UNSUPPORTED."""
    from dataclasses import replace

    from clip_retrieval_amd import load_library
    from clip_retrieval_amd.encoder import ARCHS, ClipArch

    lib = load_library()
    E_ARG, E_UNSUPPORTED = -1, -5
    one = np.zeros(1, np.float32)

    def create(arch):
        d, h = arch.to_desc(), C.c_void_p()
        rc = lib.clipx_create(C.byref(d), one.ctypes.data, 1, 0, C.byref(h))
        assert not h.value
        return rc, lib.clipx_last_error().decode()

    for name in (G, BIGG):
        a = ARCHS[name]
        assert create(a)[0] == E_ARG                                       # 257 tokens: nine key blocks
        assert create(replace(a, patch_size=32))[0] == E_ARG               # 50 tokens: two key blocks
        assert create(replace(a, image_size=238))[0] == E_UNSUPPORTED      # 290 tokens
        rc, msg = create(replace(a, patch_size=16))                        # 197 tokens: no kernel at 4 .. 8 key blocks
        assert rc == E_UNSUPPORTED and "96" in msg and "257" in msg, msg
        rc, msg = create(replace(a, image_size=336))                       # 577 tokens
        assert rc == E_UNSUPPORTED and "288" in msg, msg
    rc, msg = create(ClipArch(t_width=1408, t_heads=16))                   # a text tower with 88-wide heads: causal, no kernel
    assert rc == E_UNSUPPORTED and "text" in msg, msg
    rc, msg = create(ClipArch(v_width=1536, v_heads=16))                   # head dimension 96
    assert rc == E_UNSUPPORTED and "104" in msg, msg
    rc, msg = create(ClipArch(v_width=1344, v_heads=21, v_mlp=5376))       # 64-wide heads, but a width that is no multiple of 128
    assert rc == E_UNSUPPORTED and "128" in msg, msg
    assert create(ClipArch(v_width=1408, v_heads=22))[0] == E_ARG          # 64-wide heads at an odd multiple of 128: accepted


def test_wide_dispatch_under_sanitizers(tmp_path):
    """tools/attn_wide_plan_check.cpp (its own main, only clipx_attn_plan.h) built with -fsanitize=address,undefined and run as a
    child: for dh 88 / 104, T in 1 .. 700, causal in {0, 1} a kernel exactly at 1, 2, 3 and 9 key blocks and not causal, its LDS
    bytes the one expression of the header and within the limit, refusal in every other cell; every dh 64 / 80 cell what it was."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "attn_wide_plan_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "clip-retrieval_amd", "csrc"), os.path.join(ROOT, "tools", "attn_wide_plan_check.cpp"), "-o", exe]
    build = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("wide plan ok") and "FAILED" not in run.stdout
    wide = [ln for ln in run.stdout.splitlines() if ln.startswith("wide dh")]
    assert len(wide) == 4
    # T 1 .. 96 and 257 .. 288 = 128 lengths, not causal only; the LDS of nine key blocks: 113.25 and 140.5 KiB
    assert "128 planned" in wide[0] and "115968 bytes" in wide[0] and "128 planned" in wide[2] and "143872 bytes" in wide[2]
    assert "  0 planned, 700 refused" in wide[1] and "  0 planned, 700 refused" in wide[3]
    old = [ln for ln in run.stdout.splitlines() if ln.startswith("old dh")]
    assert len(old) == 4 and all("700 cells unchanged" in ln for ln in old)


def test_library_builds_from_a_clean_tree_and_exports_the_abi(tmp_path):
    """A copy of the sources alone (no lib/, no object files) is built by its own __graft_entry__.build() in a child process, and the
    library that comes out exports every function include/clipx.h and include/knnx.h declare (what tests/test_abi.py asks of the
    tree's library).  The copy keeps the library this process has loaded untouched; it holds the new row-wise and attention
    instantiations and the constexpr plan header to compiling from scratch through the Makefile."""
    import sys

    if not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None:
        pytest.skip("no hipcc / make")
    tree = tmp_path / "tree"
    skip = shutil.ignore_patterns("lib", "build", "build_ablate", "__pycache__", "*.o", "*.so")
    for name in ("clip-retrieval_amd", "include", "oracle"):
        shutil.copytree(os.path.join(ROOT, name), tree / name, ignore=skip)
    for name in ("__graft_entry__.py", "clip_retrieval_amd.py"):
        shutil.copy(os.path.join(ROOT, name), tree / name)
    assert not (tree / "clip-retrieval_amd" / "lib").exists()
    child = (
        "import os, re, sys\n"
        "sys.path.insert(0, os.getcwd())\n"
        "import __graft_entry__ as g\n"
        "g.build()\n"
        "import clip_retrieval_amd\n"
        "lib = clip_retrieval_amd.load_library()\n"
        "assert os.path.realpath(lib._name).startswith(os.path.realpath(os.getcwd())), lib._name\n"
        "n = 0\n"
        "for header in ('knnx.h', 'clipx.h'):\n"
        "    text = re.sub(r'/\\*.*?\\*/', '', open(os.path.join('include', header)).read(), flags=re.S)\n"
        "    for name in sorted(set(re.findall(r'\\b(' + header[:-2] + r'_[a-z0-9_]+)\\s*\\(', text))):\n"
        "        assert hasattr(lib, name), name\n"
        "        n += 1\n"
        "print('clean build ok', n)\n")
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "MAKEFLAGS", "MFLAGS")}
    run = subprocess.run([sys.executable, "-c", child], cwd=tree, env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    last = run.stdout.rstrip().splitlines()[-1].split()
    assert last[:3] == ["clean", "build", "ok"] and int(last[3]) >= 20, run.stdout[-500:]
    assert (tree / "clip-retrieval_amd" / "lib" / "libclipx.so").exists()


def test_library_exports_and_limits_without_a_device():
    """The entry points the feature goes through are exported, and their refusals at the new head dimensions are made before the
    device is touched (the pointers are never read)."""
    from clip_retrieval_amd import load_library

    lib = load_library()
    fake = C.c_void_p(4096)
    for sym in ("clipx_attention_dh_device", "clipx_attention_ex_device", "clipx_rowstats_device", "clipx_layernorm_device",
                "clipx_gemm_f16_ln_device", "clipx_create", "clipx_blob_floats"):
        assert getattr(lib, sym) is not None
    for T, dh, causal, word in ((257, 88, 1, "causal"), (128, 104, 0, "97"), (300, 88, 0, "288"), (609, 104, 0, "608"), (77, 96, 0, "104")):
        assert lib.clipx_attention_dh_device(0, fake, fake, 1, T, 1, dh, causal, None) == -5
        assert word in lib.clipx_last_error().decode()
        assert lib.clipx_attention_ex_device(0, fake, fake, 1, T, 1, dh, causal, 0, None, None, None) == -5
        assert word in lib.clipx_last_error().decode()
    assert lib.clipx_attention_ex_device(0, fake, fake, 1, 77, 1, 104, 0, 0, fake, fake, None) == -5
    assert "ragged" in lib.clipx_last_error().decode()
    assert lib.clipx_rowstats_device(0, fake, 1, fake, 4, 1408 + 64, C.c_float(1e-5), None) == -5
    assert "128" in lib.clipx_last_error().decode()
