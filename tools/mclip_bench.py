"""Captions per second of the multilingual text towers (use_mclip) at B = 256, random weights, both family members, next to the HF
model in torch fp16 on the same GPU, in the same run, on the same ids.

    python tools/mclip_bench.py [--bs 256] [--steps 200] [--warmup 3] [--rounds 5] [--vocab 0] [--log profiles/mclip_encode.log]

Caption lengths (tokens, [CLS] and [SEP] included): 2 + round(lognormal(mean = ln 18, sigma = 0.6)), clipped to 3 .. 128, seed 1 --
median about 19, mean about 22, a few per cent at 60 and more: the shape of alt-text captions.  The ids are i.i.d. uniform over the
vocabulary (speed does not depend on them).
One step = `bs` captions, ids and outputs resident in HBM.  This library: clipx_bert_encode_device (ragged rows: sum of the lengths,
padded to whole GEMM tiles).  Yardstick: `DistilBertModel` / `XLMRobertaModel(add_pooling_layer=False)` `.half().cuda()` on the batch
padded to its longest caption with the attention mask, then the masked mean and the dense layer in torch -- what
SentenceTransformer.encode / M-CLIP's forward run on a GPU in fp16, without their tokenizers.  Both are timed with a host clock around
steps that end in a device synchronise, `rounds` windows each, alternating; the median window and the spread are reported.
--vocab N cuts both vocabularies to N rows (the embedding gather does not depend on the table's height; building a 250 002-row
random table on the host takes most of the run).  No threshold: a record, not a bar.  Also printed: the cosine between the two
outputs (the weights are the same), so that the pair is known to compute the same thing."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def caption_lengths(n, seed=1):
    rng = np.random.default_rng(seed)
    return np.clip(2 + np.rint(rng.lognormal(np.log(18.0), 0.6, n)), 3, 128).astype(np.int32)


def windows(fn, steps, rounds, B):
    rates = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        rates.append(steps * B / (time.perf_counter() - t0))
    return rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200, help="steps per timed window (a window should last a fraction of a second at least)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=0, help="cut both vocabularies to this many rows (0: the published sizes)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "mclip_encode.log"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    import dataclasses

    import bert_cases as bc
    from clip_retrieval_amd import mclip

    B = a.bs
    lens = caption_lengths(B)
    lines = [f"mclip_bench: B = {B}, lengths 2 + lognormal(ln 18, 0.6) clipped to 3 .. 128 (seed 1): sum {int(lens.sum())}, median "
             f"{int(np.median(lens))}, max {int(lens.max())}; {a.steps} steps x {a.rounds} windows after {a.warmup} warm-up steps; "
             f"device {torch.cuda.get_device_name(0)}"]
    for kind, name in (("distilbert", "distilbert-multilingual"), ("xlmr", "xlm-roberta-large/768")):
        arch = mclip.BERT_ARCHS[name]
        if a.vocab:
            arch = dataclasses.replace(arch, vocab=a.vocab)
        model, dw, db = bc.hf_model(kind, arch, seed=0)
        pack = mclip.blob_from_distilbert_state_dict if kind == "distilbert" else mclip.blob_from_xlmr_state_dict
        enc = mclip.BertTextEncoder(arch, pack(model.state_dict(), dw, db, arch), 0)
        ids_host = bc.synth_ids(B, lens, arch.vocab, arch.max_len, seed=2)
        ids = torch.from_numpy(ids_host).cuda()
        out = torch.empty(B, arch.out_dim, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def ours():
            enc.encode_ids_device(ids.data_ptr(), lens, B, out.data_ptr(), None, stream)

        T = int(lens.max())
        hf = model.half().cuda()
        dw16, db16 = dw.half().cuda(), (db.half().cuda() if db is not None else None)
        mask = (torch.arange(T, device="cuda")[None, :] < torch.from_numpy(lens).cuda()[:, None]).long()
        hf_ids = ids[:, :T].long().clone()
        hf_ids[mask == 0] = 1 if kind == "xlmr" else 0
        hf_out = [None]

        @torch.no_grad()
        def theirs():
            x = hf(input_ids=hf_ids, attention_mask=mask)[0]
            p = (x * mask[..., None]).sum(1) / mask.sum(1, keepdim=True)
            y = p @ dw16.T
            y = y + db16 if db16 is not None else y
            hf_out[0] = y / y.norm(dim=-1, keepdim=True)

        for _ in range(a.warmup):
            ours()
            theirs()
        torch.cuda.synchronize()
        enc.check_range(stream)
        r_ours, r_theirs = [], []
        for _ in range(a.rounds):  # alternating windows: the two share whatever the box is doing
            r_ours += windows(ours, a.steps, 1, B)
            r_theirs += windows(theirs, a.steps, 1, B)
        cos = float((out.double() * hf_out[0].double()).sum(1).min())
        rec = {"model": name, "vocab": arch.vocab, "layers": arch.layers, "width": arch.width, "rows": int(lens.sum()),
               "hip_captions_per_s": round(float(np.median(r_ours)), 1), "hip_windows": [round(r, 1) for r in r_ours],
               "hf_fp16_captions_per_s": round(float(np.median(r_theirs)), 1), "hf_windows": [round(r, 1) for r in r_theirs],
               "min_cosine_hip_vs_hf_fp16": round(cos, 6)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        enc.close()
        del hf, model, enc
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[0])


if __name__ == "__main__":
    main()
