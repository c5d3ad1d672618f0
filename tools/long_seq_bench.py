"""Encode throughput of the full-depth ViT-L/14@336px (577 image tokens: the long-sequence attention kernel), random weights.

    python tools/long_seq_bench.py [--model ViT-L/14@336px] [--bs 256] [--steps 10] [--warmup 3] [--rounds 5]

One step = a batch of `bs` images and `bs` captions through both towers, device buffers in, device buffers out (what bench.py times
for the 224 model).  Prints samples/s per round, their median and spread, the achieved fraction of the bf16 MFMA peak from
synth.tower_gflop of the architecture, and the share of the step the attention launches take (hipEvent brackets, a pass of its own).
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
    a = ap.parse_args()
    from clip_retrieval_amd.encoder import ARCHS, ClipEncoder, random_blob
    from clip_retrieval_amd.synth import normalise_u8_nhwc, synth_pixels_u8, synth_tokens, tower_gflop

    arch = ARCHS[a.model]
    enc = ClipEncoder(arch, random_blob(arch, 0), 0)
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
    print(json.dumps(res))
    enc.close()


if __name__ == "__main__":
    main()
