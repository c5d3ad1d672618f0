"""Encode throughput of a full-depth model -- by default ViT-L/14@336px (577 image tokens: the long-sequence attention kernel) --
with random weights.

    python tools/long_seq_bench.py [--model ViT-L/14@336px] [--bs 256] [--steps 10] [--warmup 3] [--rounds 5] [--split]
    python tools/long_seq_bench.py --model open_clip:ViT-bigG-14 --split      (any key of encoder.ARCHS)

One step = a batch of `bs` images and `bs` captions through both towers, device buffers in, device buffers out (what bench.py times
for the 224 model).  Prints samples/s per round, their median and spread, the achieved fraction of the bf16 MFMA peak from
synth.tower_gflop of the architecture, and the share of the step the attention launches take (hipEvent brackets, a pass of its own).
--split adds where the step goes: the encoder's profile brackets (GEMMs, attention, LayerNorm / statistics, the rest) in a pass of
their own, the four GEMMs of an image-tower block timed alone at the step's row count with the kernel each lands in (N a multiple of
256: the 256x256 kernel; else the 128x128 kernel in one launch) scaled to the tower's depth, and the HBM the handle took.
A record beside the 224 model's numbers, not a bar."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BF16_PEAK_TFLOPS = 2500.0  # dense MFMA bf16 / f16 of the MI355X, the figure bench.py uses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L/14@336px")
    ap.add_argument("--bs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--split", action="store_true", help="also report where the step goes (profile brackets, image-tower GEMMs alone, HBM)")
    a = ap.parse_args()
    from clip_retrieval_amd.encoder import ARCHS, ClipEncoder, random_blob
    from clip_retrieval_amd.synth import normalise_u8_nhwc, synth_pixels_u8, synth_tokens, tower_gflop

    arch = ARCHS[a.model]
    blob = random_blob(arch, 0)
    torch.cuda.init()
    free0 = torch.cuda.mem_get_info()[0]
    enc = ClipEncoder(arch, blob, 0)
    hbm_handle = free0 - torch.cuda.mem_get_info()[0]  # weights (f32 blob + 16-bit matrices) and the activation workspace of max_batch
    del blob
    B = min(a.bs, enc.max_batch)
    gf_img, gf_txt = tower_gflop(arch)
    ids_host = synth_tokens(B, arch.ctx_len, arch.vocab, seed=2)
    pix = torch.from_numpy(normalise_u8_nhwc(synth_pixels_u8(B, arch.image_size, seed=1))).cuda()
    ids = torch.from_numpy(ids_host).cuda()
    out_i = torch.empty(B, arch.embed_dim, dtype=torch.float16, device="cuda")
    out_t = torch.empty(B, arch.embed_dim, dtype=torch.float16, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        enc.encode_image_device(pix.data_ptr(), B, 0, out_i.data_ptr(), None, stream)
        enc.encode_text_device(ids.data_ptr(), B, out_t.data_ptr(), None, stream, ids_host=ids_host)

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    enc.check_range(stream)
    rates = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        rates.append(a.steps * B / (time.perf_counter() - t0))
    assert torch.isfinite(out_i.float()).all() and torch.isfinite(out_t.float()).all()
    med = float(np.median(rates))
    # attention's share: every launch of kind 1 bracketed by hipEvents, in a pass of its own
    enc.profile(4)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    enc.profile(0)
    n, ms, _ = enc.profile_get(1)
    res = {"model": a.model, "bs": B, "image_tokens": arch.v_tokens, "samples_per_s": round(med, 1),
           "samples_per_s_rounds": [round(r, 1) for r in rates], "spread": [round(min(rates), 1), round(max(rates), 1)],
           "gflop_per_sample": round(gf_img + gf_txt, 2), "achieved_tflops": round(med * (gf_img + gf_txt) / 1e3, 1),
           "frac_of_bf16_peak": round(med * (gf_img + gf_txt) / 1e3 / BF16_PEAK_TFLOPS, 4),
           "attention": {"launches_per_step": n // a.steps, "ms_per_step": round(ms / a.steps, 3), "share_of_step": round(ms / (dt * 1e3), 4)}}
    res["ms_per_step"] = round(1e3 * B / med, 2)
    if a.split:
        res["hbm_gib"] = {"handle": round(hbm_handle / 2 ** 30, 2), "weights_f32_blob": round(4 * enc_blob_floats(arch) / 2 ** 30, 2)}
        res["split"] = step_split(enc, step, a.steps)
        res["image_tower_gemms"] = image_tower_gemms(arch, B)
    print(json.dumps(res))
    enc.close()


def enc_blob_floats(arch):
    from clip_retrieval_amd.encoder import blob_floats

    return blob_floats(arch)


def step_split(enc, step, steps):
    """ms per step inside the encoder's profile brackets: kind 0 the GEMMs (every kernel timed on its own dispatch), 1 attention,
    2 LayerNorm / row statistics, 3 im2col, gathers and the projection tail; `wall` is the step with the brackets on"""
    enc.profile(1)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    enc.profile(0)
    out = {"wall_ms_with_brackets": round(wall, 2)}
    for kind, name in ((0, "gemm"), (1, "attention"), (2, "layernorm_stats"), (3, "rest")):
        n, ms, fl = enc.profile_get(kind)
        out[name] = {"launch_scopes_per_step": n // steps, "ms_per_step": round(ms / steps, 3),
                     "tflops": round(fl / (ms * 1e-3) / 1e12, 1) if ms > 0 and fl > 0 else None}
    return out


def image_tower_gemms(arch, B):
    """The four GEMMs of one image-tower block at M = B * tokens rows, each timed alone through the library's per-kernel entry
    points (median of 7 after 2 warm-ups), and their sum over the tower's depth.  N % 256 != 0 sends a GEMM to the 128x128 kernel."""
    import ctypes as C

    from clip_retrieval_amd import load_library
    from clip_retrieval_amd._lib import check

    lib = load_library()
    M, w, mlp = B * arch.v_tokens, arch.v_width, arch.v_mlp
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    act = 1 if arch.act == "quick_gelu" else 2
    rs = torch.rand(M, generator=g, device="cuda") * 0.3 + 0.05
    out = {}
    tot = {"128x128": 0.0, "256x256": 0.0}
    for name, N, K, f16, epi in (("qkv", 3 * w, w, True, 7), ("out_proj", w, w, False, 6), ("fc1", mlp, w, True, act), ("fc2", w, mlp, False, 6)):
        dt = torch.float16 if f16 else torch.bfloat16
        A = (torch.randn(M, K, generator=g, device="cuda") * 0.5).to(dt)
        W = (torch.randn(N, K, generator=g, device="cuda") * 0.03).to(dt)
        bias = torch.randn(N, generator=g, device="cuda")
        y = torch.zeros(M, N, device="cuda", dtype=torch.float16 if epi in (6, 7) else torch.bfloat16)
        p = lambda t: C.c_void_p(t.data_ptr())

        def call():
            if f16:
                check(lib, lib.clipx_gemm_f16_device(0, p(A), p(W), p(bias), p(y), M, N, K, epi, p(rs), C.c_void_p(st)), "clipx")
            else:
                check(lib, lib.clipx_gemm_bf16_ex_device(0, p(A), p(W), p(bias), p(y), M, N, K, epi, None, None, C.c_void_p(st)), "clipx")

        ts = []
        for i in range(9):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            y.zero_()
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ts.append(e0.elapsed_time(e1))
        ms = float(np.median(ts))
        # the label is inferred, not read back from the dispatch: launch_gemm sends N % 256 != 0 to the 128x128 kernel, and at the
        # M of this tool (bs x tokens, far above the 256x256 path's tile threshold) every other shape to the 256x256 kernels
        kern = "256x256" if N % 256 == 0 else "128x128"
        tot[kern] += ms * arch.v_layers
        out[name] = {"M": M, "N": N, "K": K, "kernel": kern, "ms": round(ms, 3), "tflops": round(2.0 * M * N * K / (ms * 1e-3) / 1e12, 1)}
        del A, W, y
    out["ms_per_step_over_the_tower"] = {k: round(v, 2) for k, v in tot.items()}
    return out


if __name__ == "__main__":
    main()
