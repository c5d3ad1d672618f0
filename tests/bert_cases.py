"""The multilingual text-tower family restated in fp32 torch on the CPU, from the weight blob ALONE (include/clipx.h:
clipx_bert_blob_floats gives the order): what the new tests compare the HIP tower -- and the blob packers -- against.

    x = LN_emb(word[id] + pos[pos_offset + t])
    per layer:  x = LN_att(x + out_proj(softmax(q k^T / 8, keys of the sample's own tokens) v));  x = LN_out(x + fc2(gelu(fc1(x))))
    y = dense(mean over the sample's tokens of x) (+ bias)

Also the HF models of the two family members at random init (both construct offline) and their masked-mean + dense outputs."""
import json
import os

import numpy as np
import torch

LENS_EDGE = [1, 2, 31, 32, 33, 64, 65, 127, 128]


def carve(blob, arch):
    """blob -> dict of torch f32 tensors (views)"""
    b = torch.from_numpy(np.ascontiguousarray(blob, dtype=np.float32))
    w, m, E = arch.width, arch.mlp, arch.out_dim
    o = 0

    def take(*shape):
        nonlocal o
        n = int(np.prod(shape))
        t = b[o:o + n].reshape(*shape)
        o += n
        return t

    W = {"word": take(arch.vocab, w), "pos": take(arch.max_pos, w), "ln_emb": (take(w), take(w)), "layers": []}
    for _ in range(arch.layers):
        W["layers"].append({"qkv_w": take(3 * w, w), "qkv_b": take(3 * w), "out_w": take(w, w), "out_b": take(w), "ln_att": (take(w), take(w)),
                            "fc1_w": take(m, w), "fc1_b": take(m), "fc2_w": take(w, m), "fc2_b": take(w), "ln_out": (take(w), take(w))})
    W["dense_w"] = take(E, w)
    W["dense_b"] = take(E) if arch.dense_bias else None
    assert o == b.numel(), (o, b.numel())
    return W


def _ln(x, gb, eps):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), gb[0], gb[1], eps)


@torch.no_grad()
def forward(blob, arch, ids, lens, dtype=torch.float32):
    """ids int [B, T] left-aligned, lens [B] -> y [B, out_dim] (NOT normalised), sample by sample so that nothing past a sample's
    length can matter"""
    W = carve(blob, arch)
    ids = torch.as_tensor(np.asarray(ids)).long()
    out = []
    H, dh = arch.heads, arch.width // arch.heads
    for b, n in enumerate(int(v) for v in lens):
        x = (W["word"][ids[b, :n]] + W["pos"][arch.pos_offset:arch.pos_offset + n]).to(dtype)
        x = _ln(x, [t.to(dtype) for t in W["ln_emb"]], arch.ln_eps)
        for L in W["layers"]:
            qkv = x @ L["qkv_w"].to(dtype).T + L["qkv_b"].to(dtype)
            q, k, v = (t.reshape(n, H, dh).transpose(0, 1) for t in qkv.chunk(3, dim=-1))
            p = torch.softmax(q @ k.transpose(1, 2) / dh ** 0.5, dim=-1)
            a = (p @ v).transpose(0, 1).reshape(n, arch.width)
            x = _ln(x + a @ L["out_w"].to(dtype).T + L["out_b"].to(dtype), [t.to(dtype) for t in L["ln_att"]], arch.ln_eps)
            h = torch.nn.functional.gelu(x @ L["fc1_w"].to(dtype).T + L["fc1_b"].to(dtype))
            x = _ln(x + h @ L["fc2_w"].to(dtype).T + L["fc2_b"].to(dtype), [t.to(dtype) for t in L["ln_out"]], arch.ln_eps)
        y = x.mean(dim=0) @ W["dense_w"].to(dtype).T
        if W["dense_b"] is not None:
            y = y + W["dense_b"].to(dtype)
        out.append(y)
    return torch.stack(out).float().numpy()


def unit(y):
    y = np.asarray(y, dtype=np.float32)
    n = np.linalg.norm(y, axis=-1, keepdims=True)
    n[n == 0] = 1
    return y / n


# ----------------------------------------------------------------------------------------------
# the HF models at random init
# ----------------------------------------------------------------------------------------------
def hf_model(kind, arch, seed=0, scale=None):
    """kind 'distilbert' | 'xlmr' -> (model in eval mode, dense weight [E, w], dense bias or None).  scale: std of the random
    LayerNorm gains / biases and embeddings is raised so that random rows separate (tests of deep towers)."""
    import transformers

    torch.manual_seed(seed)
    if kind == "distilbert":
        cfg = transformers.DistilBertConfig(vocab_size=arch.vocab, max_position_embeddings=arch.max_pos, dim=arch.width, n_layers=arch.layers,
                                            n_heads=arch.heads, hidden_dim=arch.mlp, dropout=0.0, attention_dropout=0.0)
        model = transformers.DistilBertModel(cfg)
    else:
        cfg = transformers.XLMRobertaConfig(vocab_size=arch.vocab, max_position_embeddings=arch.max_pos, hidden_size=arch.width,
                                            num_hidden_layers=arch.layers, num_attention_heads=arch.heads, intermediate_size=arch.mlp,
                                            layer_norm_eps=arch.ln_eps, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                                            type_vocab_size=1, pad_token_id=1)
        model = transformers.XLMRobertaModel(cfg, add_pooling_layer=False)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in model.named_parameters():  # HF's init leaves every bias 0 and every LayerNorm (1, 0): make them matter
            if name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
            elif "LayerNorm.weight" in name or "layer_norm.weight" in name:
                p.copy_(1.0 + torch.randn(p.shape, generator=g) * 0.1)
            elif scale is not None and p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * scale)
    dense_w = torch.randn(arch.out_dim, arch.width, generator=g) * arch.width ** -0.5
    dense_b = torch.randn(arch.out_dim, generator=g) * 0.05 if arch.dense_bias else None
    return model.eval(), dense_w, dense_b


@torch.no_grad()
def hf_forward(model, dense_w, dense_b, ids, lens, pad_id):
    """the HF model on the padded batch with its attention mask -> masked mean -> dense: [B, out_dim] f32 (NOT normalised).
    Positions past lens hold pad_id, as the tokenizers leave them (XLM-R derives its position ids from that)."""
    ids = torch.as_tensor(np.asarray(ids)).long().clone()
    lens = torch.as_tensor(np.asarray(lens)).long()
    T = int(lens.max())
    ids = ids[:, :T]
    mask = (torch.arange(T)[None, :] < lens[:, None]).long()
    ids[mask == 0] = pad_id
    x = model(input_ids=ids, attention_mask=mask)[0]
    p = (x * mask[..., None]).sum(1) / mask.sum(1, keepdim=True)
    y = p @ dense_w.T
    return (y + dense_b if dense_b is not None else y).float().numpy()


def synth_ids(B, lens, vocab, max_len, seed=0, lo=5, per_sample=0):
    """random ids in [lo, vocab) (clear of the special / pad ids), rectangular [B, max_len], zeros past lens.  per_sample = k > 0:
    sample b draws its tokens from k ids of its own (a text about one thing).  The mean over 128 i.i.d. tokens of a random-init
    tower is nearly the same vector for every sample, and parity_gate's centred cosine and nearest-row conditions need rows that
    differ, as the CLIP tests' structured images do (oracle.clip_oracle.synth_pixels_u8)."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((B, max_len), dtype=np.int32)
    for b, n in enumerate(lens):
        if per_sample:
            own = rng.choice(np.arange(lo, vocab), size=per_sample, replace=False)
            ids[b, :n] = own[rng.integers(0, per_sample, n)]
        else:
            ids[b, :n] = rng.integers(lo, vocab, n)
    return ids


# ----------------------------------------------------------------------------------------------
# a synthetic sentence-transformers folder
# ----------------------------------------------------------------------------------------------
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "hello", "world", "un", "##believ", "##able", "##s", "!", ",", ".", "?", "'",
         "café", "cafe", "naïve", "Hello", "the", "a", "##a", "b", "##b", "c", "##c", "中", "国", "人", "x", "##x", "-", "(", ")", "é", "##é",
         "ab", "##ab", "1", "##1", "2", "##2", "straße", "Straße"]


def write_vocab(path):
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(VOCAB) + "\n")
    return str(path)


def write_st_folder(root, vocab_file, arch, seed=5, safetensors=True):
    """a sentence-transformers folder: modules.json, the transformer's config / weights / vocab / sentence_bert_config, 1_Pooling, 2_Dense"""
    model, dw, db = hf_model("distilbert", arch, seed=seed)
    os.makedirs(os.path.join(root, "1_Pooling"))
    os.makedirs(os.path.join(root, "2_Dense"))
    json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
               {"idx": 2, "name": "2", "path": "2_Dense", "type": "sentence_transformers.models.Dense"}], open(os.path.join(root, "modules.json"), "w"))
    json.dump(model.config.to_dict(), open(os.path.join(root, "config.json"), "w"))
    json.dump({"max_seq_length": 12, "do_lower_case": False}, open(os.path.join(root, "sentence_bert_config.json"), "w"))
    json.dump({"do_lower_case": False}, open(os.path.join(root, "tokenizer_config.json"), "w"))
    json.dump({"word_embedding_dimension": arch.width, "pooling_mode_mean_tokens": True, "pooling_mode_cls_token": False,
               "pooling_mode_max_tokens": False}, open(os.path.join(root, "1_Pooling", "config.json"), "w"))
    json.dump({"in_features": arch.width, "out_features": arch.out_dim, "bias": False,
               "activation_function": "torch.nn.modules.linear.Identity"}, open(os.path.join(root, "2_Dense", "config.json"), "w"))
    if safetensors:
        from safetensors.torch import save_file

        save_file({k: v.contiguous() for k, v in model.state_dict().items()}, os.path.join(root, "model.safetensors"))
    else:
        torch.save(model.state_dict(), os.path.join(root, "pytorch_model.bin"))
    torch.save({"linear.weight": dw}, os.path.join(root, "2_Dense", "pytorch_model.bin"))
    with open(vocab_file, encoding="utf-8") as f:
        open(os.path.join(root, "vocab.txt"), "w", encoding="utf-8").write(f.read())
    return model, dw
