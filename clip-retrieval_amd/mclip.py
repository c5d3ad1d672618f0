"""Multilingual text towers -- the reference's `use_mclip` switch -- on the HIP encoder (include/clipx.h: clipx_bert_*).

Reference seams mirrored here
  * `clip inference --use_mclip`: `SentenceTransformer(mclip_model).encode(item["text"])` replaces the CLIP text tower and the
    result is normalised in numpy, float32 (clip_inference/mapper.py:44-47, 62-63).  The default `mclip_model` is
    sentence-transformers/clip-ViT-B-32-multilingual-v1: DistilBERT multilingual -> mean pooling -> Dense 768 -> 512.
  * `clip back`: `clip_resource.model_txt_mclip(text)` (clip_back.py:222-224, 837-859): M-CLIP's XLM-R large -> masked mean ->
    `LinearTransformation`.
Both are one family -- a post-LN, bidirectional, padding-masked BERT encoder, masked mean pooling, one dense layer -- and run as one
set of kernels (csrc/bert_kernels.hip + the CLIP encoder's GEMMs and ragged attention).  This file only moves bytes: arch
descriptions, weight-blob assembly from the HF checkpoint names, BERT's WordPiece tokenisation restated (no `transformers` on the
product path, as in tokenizer.py), and loaders for LOCAL checkpoint folders.  Nothing is ever fetched.

Limit: a text is at most 128 tokens (the ragged attention kernels).  sentence-transformers truncates to `max_seq_length` (128 for
the default model) and so does `load_sentence_transformer`; M-CLIP does not truncate, and `load_mclip` raises ValueError for a
longer text instead of truncating silently.
"""

import ctypes as C
import json
import os
import unicodedata
from dataclasses import dataclass

import numpy as np

from ._lib import ClipxBertDesc, check, load_library

MAX_TOKENS = 128


@dataclass(frozen=True)
class BertArch:
    vocab: int = 119547
    max_pos: int = 512
    pos_offset: int = 0
    width: int = 768
    layers: int = 6
    heads: int = 12
    mlp: int = 3072
    out_dim: int = 512
    dense_bias: bool = False
    max_len: int = 128
    ln_eps: float = 1e-12

    def to_desc(self):
        d = ClipxBertDesc()
        for f in ("vocab", "max_pos", "pos_offset", "width", "layers", "heads", "mlp", "out_dim", "max_len"):
            setattr(d, f, int(getattr(self, f)))
        d.dense_bias = 1 if self.dense_bias else 0
        d.ln_eps = float(self.ln_eps)
        return d


# Shapes recalled from memory of the published configurations, not read from the checkpoints (as the ViT-g / bigG rows of
# encoder.ARCHS): the loaders below take the true values from the checkpoint's config.json and tensors, never from this table.
BERT_ARCHS = {
    "distilbert-multilingual": BertArch(),
    "xlm-roberta-large/768": BertArch(vocab=250002, max_pos=514, pos_offset=2, width=1024, layers=24, heads=16, mlp=4096, out_dim=768,
                                      dense_bias=True, ln_eps=1e-5),
    "xlm-roberta-large/512": BertArch(vocab=250002, max_pos=514, pos_offset=2, width=1024, layers=24, heads=16, mlp=4096, out_dim=512,
                                      dense_bias=True, ln_eps=1e-5),
}


def bert_blob_floats(arch: BertArch) -> int:
    d = arch.to_desc()
    return int(load_library().clipx_bert_blob_floats(C.byref(d)))


# ----------------------------------------------------------------------------------------------
# weight blobs (order: include/clipx.h, clipx_bert_blob_floats)
# ----------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().float().cpu().numpy() if hasattr(t, "detach") else np.asarray(t, dtype=np.float32)


def _cat(parts):
    return np.concatenate([np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in parts])


def _strip(sd, prefixes):
    sd = dict(sd)
    for pre in prefixes:
        if sd and all(k.startswith(pre) for k in sd):
            sd = {k[len(pre):]: v for k, v in sd.items()}
    return sd


def _dense_parts(dense_w, dense_b, arch):
    w = _np(dense_w)
    if w.shape != (arch.out_dim, arch.width):
        raise ValueError(f"dense weight is {w.shape}, the arch says {(arch.out_dim, arch.width)}")
    if arch.dense_bias != (dense_b is not None):
        raise ValueError("dense_bias of the arch and the presence of a dense bias disagree")
    return [w] + ([_np(dense_b)] if arch.dense_bias else [])


def blob_from_distilbert_state_dict(sd, dense_w, dense_b, arch: BertArch) -> np.ndarray:
    """HF `DistilBertModel` names (embeddings.word_embeddings.weight, transformer.layer.N.attention.q_lin.weight, ...; a leading
    'distilbert.' is dropped); q / k / v are stacked into the in_proj layout.  dense_w [out_dim, width], dense_b or None."""
    sd = _strip(sd, ("distilbert.",))
    parts = [_np(sd["embeddings.word_embeddings.weight"]), _np(sd["embeddings.position_embeddings.weight"]),
             _np(sd["embeddings.LayerNorm.weight"]), _np(sd["embeddings.LayerNorm.bias"])]
    for l in range(arch.layers):
        p = f"transformer.layer.{l}."
        parts.append(np.concatenate([_np(sd[p + f"attention.{x}_lin.weight"]) for x in "qkv"], 0))
        parts.append(np.concatenate([_np(sd[p + f"attention.{x}_lin.bias"]) for x in "qkv"], 0))
        for k in ("attention.out_lin", "sa_layer_norm", "ffn.lin1", "ffn.lin2", "output_layer_norm"):
            parts += [_np(sd[p + k + ".weight"]), _np(sd[p + k + ".bias"])]
    return _finish(parts + _dense_parts(dense_w, dense_b, arch), arch)


def blob_from_xlmr_state_dict(sd, dense_w, dense_b, arch: BertArch) -> np.ndarray:
    """HF `XLMRobertaModel` / `BertModel` names (encoder.layer.N.attention.self.query.weight, ...; a leading 'roberta.' or
    'transformer.' is dropped).  Row 0 of token_type_embeddings -- the only type these models ever see -- is added to every row of
    the position table here, once, instead of per token on the device."""
    sd = _strip(sd, ("transformer.", "roberta."))
    pos = _np(sd["embeddings.position_embeddings.weight"]).copy()
    if "embeddings.token_type_embeddings.weight" in sd:
        pos += _np(sd["embeddings.token_type_embeddings.weight"])[0][None, :]
    parts = [_np(sd["embeddings.word_embeddings.weight"]), pos, _np(sd["embeddings.LayerNorm.weight"]), _np(sd["embeddings.LayerNorm.bias"])]
    for l in range(arch.layers):
        p = f"encoder.layer.{l}."
        parts.append(np.concatenate([_np(sd[p + f"attention.self.{x}.weight"]) for x in ("query", "key", "value")], 0))
        parts.append(np.concatenate([_np(sd[p + f"attention.self.{x}.bias"]) for x in ("query", "key", "value")], 0))
        for k in ("attention.output.dense", "attention.output.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm"):
            parts += [_np(sd[p + k + ".weight"]), _np(sd[p + k + ".bias"])]
    return _finish(parts + _dense_parts(dense_w, dense_b, arch), arch)


def expected_blob_floats(arch: BertArch) -> int:
    """The count clipx_bert_blob_floats returns, restated (the packers check themselves against it without the library)."""
    w, m, E = arch.width, arch.mlp, arch.out_dim
    layer = 3 * w * w + 3 * w + w * w + w + 2 * w + m * w + m + w * m + w + 2 * w
    return arch.vocab * w + arch.max_pos * w + 2 * w + arch.layers * layer + E * w + (E if arch.dense_bias else 0)


def _finish(parts, arch):
    blob = _cat(parts)
    if blob.size != expected_blob_floats(arch):
        raise ValueError(f"the state dict gives {blob.size} floats, the arch {arch} needs {expected_blob_floats(arch)}")
    return blob


def random_bert_blob(arch: BertArch, seed: int = 0) -> np.ndarray:
    """Random-init weights of the right shapes (benchmarks: no checkpoints offline): BERT's 0.02 everywhere, LayerNorm gains near 1."""
    import torch  # pylint: disable=import-outside-toplevel

    w, m, E = arch.width, arch.mlp, arch.out_dim
    segs = [(arch.vocab * w, 0.02, 0.0), (arch.max_pos * w, 0.02, 0.0), (w, 0.05, 1.0), (w, 0.02, 0.0)]
    for _ in range(arch.layers):
        segs += [(3 * w * w, 0.02, 0.0), (3 * w, 0.02, 0.0), (w * w, 0.02, 0.0), (w, 0.02, 0.0), (w, 0.05, 1.0), (w, 0.02, 0.0),
                 (m * w, 0.02, 0.0), (m, 0.02, 0.0), (w * m, 0.02, 0.0), (w, 0.02, 0.0), (w, 0.05, 1.0), (w, 0.02, 0.0)]
    segs.append((E * w, w ** -0.5, 0.0))
    if arch.dense_bias:
        segs.append((E, 0.02, 0.0))
    blob = torch.empty(sum(c for c, _, _ in segs), dtype=torch.float32)
    blob.normal_(0.0, 1.0, generator=torch.Generator().manual_seed(seed))
    o = 0
    for c, std, off in segs:
        v = blob[o:o + c]
        v.mul_(std)
        if off:
            v.add_(off)
        o += c
    return blob.numpy()


# ----------------------------------------------------------------------------------------------
# the encoder object
# ----------------------------------------------------------------------------------------------
class BertTextEncoder:
    """One multilingual text tower resident on one GPU.  `encode_ids` returns fresh float32 [B, E] unit-norm rows."""

    def __init__(self, arch: BertArch, blob: np.ndarray, device: int = 0):
        self._lib = load_library()
        self.arch = arch
        self.device = int(device)
        blob = np.ascontiguousarray(blob, dtype=np.float32).reshape(-1)
        desc = arch.to_desc()
        h = C.c_void_p()
        # (the library checks the description first -- an unsupported shape is reported as that, whatever the blob)
        check(self._lib, self._lib.clipx_bert_create(C.byref(desc), blob.ctypes.data, blob.size, self.device, C.byref(h)), "clipx")
        self._h = h
        self.embed_dim = int(self._lib.clipx_bert_out_dim(self._h))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.clipx_bert_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # pylint: disable=broad-except
            pass

    def _ids_lens(self, ids, lens, attention_mask):
        a = ids.numpy() if hasattr(ids, "numpy") else np.asarray(ids)
        if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] > self.arch.max_len:
            raise ValueError(f"token ids must be [B >= 1, <= {self.arch.max_len}], got {a.shape}")
        if (lens is None) == (attention_mask is None):
            raise ValueError("give exactly one of lens / attention_mask")
        if lens is None:
            m = attention_mask.numpy() if hasattr(attention_mask, "numpy") else np.asarray(attention_mask)
            m = m != 0
            lens = m.sum(axis=1)
            if m.shape != a.shape or not (m == (np.arange(a.shape[1])[None, :] < lens[:, None])).all():
                raise ValueError("attention_mask must be 1 on a prefix of every row (right padding), the tokenizers' layout")
        lens = np.ascontiguousarray(lens, dtype=np.int32).reshape(-1)
        if lens.shape[0] != a.shape[0]:
            raise ValueError("one length per row")
        rect = np.zeros((a.shape[0], self.arch.max_len), dtype=np.int32)
        rect[:, :a.shape[1]] = a
        live = np.arange(self.arch.max_len)[None, :] < lens[:, None]
        if (live & ((rect < 0) | (rect >= self.arch.vocab))).any():
            # the reference's nn.Embedding raises on an out-of-range id; the kernel would clamp it silently
            raise IndexError(f"token id out of range [0, {self.arch.vocab})")
        return rect, lens

    def encode_ids(self, ids, lens=None, attention_mask=None, f16=False):
        """ids int [B, T <= max_len], left-aligned; `lens` [B] or the tokenizer's `attention_mask` [B, T].  float32 [B, E] unit-norm
        rows (f16=True: also their IEEE fp16 rounding, as a second array)."""
        rect, lens = self._ids_lens(ids, lens, attention_mask)
        B = rect.shape[0]
        out = np.empty((B, self.embed_dim), dtype=np.float32)
        out16 = np.empty((B, self.embed_dim), dtype=np.float16) if f16 else None
        check(self._lib, self._lib.clipx_bert_encode(self._h, rect.ctypes.data, lens.ctypes.data, B, out.ctypes.data,
                                                     out16.ctypes.data if f16 else None), "clipx")
        return (out, out16) if f16 else out

    def encode_ids_device(self, ids_ptr, lens, B, out_f32_ptr, out_f16_ptr=None, stream=None):
        """ids int32 [B, max_len] and the outputs on the device, `lens` on the host; asynchronous on `stream` (check_range after)."""
        lens = np.ascontiguousarray(lens, dtype=np.int32).reshape(-1)
        if lens.shape[0] != int(B):
            raise ValueError("one length per row")
        check(self._lib, self._lib.clipx_bert_encode_device(
            self._h, C.c_void_p(int(ids_ptr)), lens.ctypes.data, int(B), C.c_void_p(int(out_f32_ptr)),
            C.c_void_p(int(out_f16_ptr)) if out_f16_ptr else None, C.c_void_p(int(stream)) if stream else None), "clipx")

    def check_range(self, stream=None):
        check(self._lib, self._lib.clipx_bert_range_check(self._h, C.c_void_p(int(stream)) if stream else None), "clipx")


# ----------------------------------------------------------------------------------------------
# BERT's basic + WordPiece tokenisation, restated (transformers.BertTokenizer is the parity pin: tests/test_mclip_cpu.py)
# ----------------------------------------------------------------------------------------------
def _is_whitespace(ch):
    return ch in " \t\n\r" or unicodedata.category(ch) == "Zs"


def _is_control(ch):
    return ch not in "\t\n\r" and unicodedata.category(ch).startswith("C")


def _is_punctuation(ch):
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(ch).startswith("P")


_CJK = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F), (0x2B820, 0x2CEAF),
        (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))


def _is_cjk(cp):
    return any(lo <= cp <= hi for lo, hi in _CJK)


class WordPieceTokenizer:
    """`tok(texts, max_length=None)` -> {"input_ids": int64 [n, T], "attention_mask": int64 [n, T]} (numpy, right-padded with
    [PAD] to the longest row, truncated to max_length).  Steps, in BERT's order: drop NUL / U+FFFD / control characters and turn
    every whitespace into a space; put spaces around CJK ideographs; split on whitespace (no Unicode normalisation, as the
    `tokenizers` BertNormalizer that AutoTokenizer resolves to does none when it keeps case); (do_lower_case: lower-case and strip
    accents;) split every punctuation character off; greedy longest-match WordPiece with '##' continuations, a word of more than
    100 characters or with an unmatched rest becomes [UNK]; [CLS] pieces [SEP]."""

    SPECIALS = ("[UNK]", "[SEP]", "[PAD]", "[CLS]", "[MASK]")

    def __init__(self, vocab_path, do_lower_case=False, max_length=MAX_TOKENS):
        if not os.path.isfile(vocab_path):
            raise FileNotFoundError(f"WordPiece vocabulary {vocab_path} not found (nothing is fetched: bring the checkpoint's vocab.txt)")
        with open(vocab_path, "r", encoding="utf-8") as f:
            self.vocab = {tok.rstrip("\n"): i for i, tok in enumerate(f.readlines())}
        self.do_lower_case = bool(do_lower_case)
        self.max_length = int(max_length)
        self.unk, self.cls, self.sep, self.pad = (self.vocab[t] for t in ("[UNK]", "[CLS]", "[SEP]", "[PAD]"))

    def _split_specials(self, text):
        """the special tokens are cut out of the text first and kept whole (PreTrainedTokenizer.tokenize)"""
        out, i = [], 0
        while i < len(text):
            hit = min(((text.find(s, i), -len(s), s) for s in self.SPECIALS if text.find(s, i) >= 0), default=None)
            if hit is None:
                out.append((text[i:], False))
                break
            j, _, s = hit
            if j > i:
                out.append((text[i:j], False))
            out.append((s, True))
            i = j + len(s)
        return out

    def _basic(self, text):
        chars = []
        for ch in text:
            cp = ord(ch)
            if cp == 0 or cp == 0xFFFD or _is_control(ch):
                continue
            if _is_whitespace(ch):
                chars.append(" ")
            elif _is_cjk(cp):
                chars += [" ", ch, " "]
            else:
                chars.append(ch)
        words = []
        for tok in "".join(chars).split():
            if self.do_lower_case:
                tok = "".join(c for c in unicodedata.normalize("NFD", tok.lower()) if unicodedata.category(c) != "Mn")
            cur = []
            for ch in tok:
                if _is_punctuation(ch):
                    if cur:
                        words.append("".join(cur))
                    words.append(ch)
                    cur = []
                else:
                    cur.append(ch)
            if cur:
                words.append("".join(cur))
        return words

    def _wordpiece(self, word):
        if len(word) > 100:
            return [self.unk]
        ids, start = [], 0
        while start < len(word):
            end = len(word)
            while end > start:
                piece = ("##" if start else "") + word[start:end]
                if piece in self.vocab:
                    break
                end -= 1
            if end == start:
                return [self.unk]
            ids.append(self.vocab[piece])
            start = end
        return ids

    def encode(self, text, max_length=None):
        L = max_length or self.max_length
        ids = []
        for piece, special in self._split_specials(text):
            if special:
                ids.append(self.vocab[piece])
            else:
                for w in self._basic(piece):
                    ids.extend(self._wordpiece(w))
        return [self.cls] + ids[:max(L - 2, 0)] + [self.sep]

    def __call__(self, texts, max_length=None):
        if isinstance(texts, str):
            texts = [texts]
        rows = [self.encode(t, max_length) for t in texts]
        T = max(len(r) for r in rows) if rows else 0
        ids = np.full((len(rows), T), self.pad, dtype=np.int64)
        mask = np.zeros((len(rows), T), dtype=np.int64)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = r
            mask[i, :len(r)] = 1
        return {"input_ids": ids, "attention_mask": mask}


# ----------------------------------------------------------------------------------------------
# loaders of local checkpoint folders
# ----------------------------------------------------------------------------------------------
def _read_json(path):
    with open(path, "r", encoding="utf-8") as f:
        return json.load(f)


def _load_weights(folder):
    """model.safetensors or pytorch_model.bin of a HF / sentence-transformers module folder -> dict of tensors / arrays"""
    st = os.path.join(folder, "model.safetensors")
    if os.path.isfile(st):
        from safetensors.numpy import load_file  # pylint: disable=import-outside-toplevel

        return load_file(st)
    pt = os.path.join(folder, "pytorch_model.bin")
    if os.path.isfile(pt):
        import torch  # pylint: disable=import-outside-toplevel

        return torch.load(pt, map_location="cpu", weights_only=True)
    raise FileNotFoundError(f"no model.safetensors / pytorch_model.bin in {folder}")


def arch_from_hf_config(cfg, out_dim, dense_bias, max_len) -> BertArch:
    """The transformer's own config.json -> BertArch: `distilbert` (dim / n_layers / n_heads / hidden_dim, eps fixed at 1e-12 in the
    model code) or the BERT / XLM-R spelling (hidden_size / ..., layer_norm_eps; RoBERTa's positions start at pad_token_id + 1)."""
    kind = cfg.get("model_type", "")
    if cfg.get("activation", cfg.get("hidden_act", "gelu")) != "gelu":
        raise ValueError("only erf-GELU checkpoints are supported")
    if kind == "distilbert":
        return BertArch(vocab=cfg["vocab_size"], max_pos=cfg["max_position_embeddings"], pos_offset=0, width=cfg["dim"],
                        layers=cfg["n_layers"], heads=cfg["n_heads"], mlp=cfg["hidden_dim"], out_dim=out_dim, dense_bias=dense_bias,
                        max_len=max_len, ln_eps=1e-12)
    if kind in ("xlm-roberta", "roberta", "bert"):
        if cfg.get("position_embedding_type", "absolute") != "absolute":
            raise ValueError("only absolute position embeddings are supported")
        off = cfg.get("pad_token_id", 1) + 1 if kind != "bert" else 0
        return BertArch(vocab=cfg["vocab_size"], max_pos=cfg["max_position_embeddings"], pos_offset=off, width=cfg["hidden_size"],
                        layers=cfg["num_hidden_layers"], heads=cfg["num_attention_heads"], mlp=cfg["intermediate_size"],
                        out_dim=out_dim, dense_bias=dense_bias, max_len=max_len, ln_eps=float(cfg.get("layer_norm_eps", 1e-12)))
    raise ValueError(f"model_type {kind!r} is not in the supported family (distilbert, bert, roberta, xlm-roberta)")


class MclipModelNotFound(FileNotFoundError, NotImplementedError):
    """No local checkpoint folder for the requested multilingual model.  A FileNotFoundError that names the places searched; also a
    NotImplementedError, which is what `ClipMapper(use_mclip=True)` raised before the towers existed: a caller that catches that
    to learn that `use_mclip` cannot be served with what is installed keeps working."""


def resolve_mclip_folder(mclip_model, clip_cache_path=None):
    """`mclip_model` as a local folder, or its name (with or without the organisation) under `clip_cache_path`."""
    cands = [mclip_model]
    if clip_cache_path:
        base = clip_cache_path if os.path.isdir(clip_cache_path) else os.path.dirname(clip_cache_path)
        cands += [os.path.join(base, mclip_model), os.path.join(base, mclip_model.replace("/", "_")), os.path.join(base, os.path.basename(mclip_model))]
    for c in cands:
        if os.path.isfile(os.path.join(c, "modules.json")) or os.path.isfile(os.path.join(c, "config.json")):
            return c
    raise MclipModelNotFound(
        f"no local checkpoint folder for mclip model {mclip_model!r} (looked at {cands}); nothing is fetched here: put the "
        "sentence-transformers / M-CLIP folder there or pass its path")


class SentenceEncoder:
    """What `load_sentence_transformer` returns: `.encode(list_of_str) -> float32 [n, E]` (SentenceTransformer.encode's dtype;
    mapper.py:63 normalises it in numpy without a cast).  `make_encoder(arch, blob, device)` builds the resident tower; tests
    pass a stand-in."""

    def __init__(self, arch, blob, tokenizer, max_seq_length, lower_text=False, device=0, make_encoder=BertTextEncoder):
        self.arch, self.tokenizer, self.max_seq_length, self.lower_text = arch, tokenizer, int(max_seq_length), bool(lower_text)
        self._enc = make_encoder(arch, blob, device)

    def tokenize(self, texts):
        texts = [str(t).strip() for t in texts]  # (sentence_transformers.models.Transformer.tokenize)
        if self.lower_text:
            texts = [t.lower() for t in texts]
        return self.tokenizer(texts, max_length=self.max_seq_length)

    def encode(self, texts, batch_size=None, **_):
        del batch_size  # the library chunks by itself
        if isinstance(texts, str):
            return self.encode([texts])[0]
        if len(texts) == 0:
            return np.zeros((0, self.arch.out_dim), dtype=np.float32)
        tok = self.tokenize(list(texts))
        return self._enc.encode_ids(tok["input_ids"], attention_mask=tok["attention_mask"])

    def close(self):
        self._enc.close()


def load_sentence_transformer(mclip_model, clip_cache_path=None, device=0, make_encoder=BertTextEncoder) -> SentenceEncoder:
    """A LOCAL sentence-transformers folder (modules.json: Transformer -> Pooling (mean) -> Dense) -> SentenceEncoder."""
    folder = resolve_mclip_folder(mclip_model, clip_cache_path)
    if not os.path.isfile(os.path.join(folder, "modules.json")):
        raise FileNotFoundError(f"{folder} has no modules.json: not a sentence-transformers folder")
    mods = {m["type"].rsplit(".", 1)[-1]: os.path.join(folder, m.get("path", "")) for m in _read_json(os.path.join(folder, "modules.json"))}
    if "Transformer" not in mods or "Dense" not in mods:
        raise ValueError(f"{folder}: expected Transformer -> Pooling -> Dense modules, found {sorted(mods)}")
    tdir, ddir = mods["Transformer"], mods["Dense"]
    if "Pooling" in mods and os.path.isfile(os.path.join(mods["Pooling"], "config.json")):
        pc = _read_json(os.path.join(mods["Pooling"], "config.json"))
        if not pc.get("pooling_mode_mean_tokens", False) or pc.get("pooling_mode_cls_token") or pc.get("pooling_mode_max_tokens"):
            raise ValueError("only mean pooling is supported")
    sb = os.path.join(tdir, "sentence_bert_config.json")
    sbc = _read_json(sb) if os.path.isfile(sb) else {}
    max_seq = int(sbc.get("max_seq_length") or MAX_TOKENS)
    if max_seq > MAX_TOKENS:
        raise ValueError(f"max_seq_length {max_seq} exceeds the {MAX_TOKENS}-token limit of this encoder")
    dc = _read_json(os.path.join(ddir, "config.json"))
    if "Identity" not in dc.get("activation_function", "Identity"):
        raise ValueError("the Dense module must have the identity activation")
    dsd = _load_weights(ddir)
    dense_w, dense_b = dsd["linear.weight"], dsd.get("linear.bias") if dc.get("bias", True) else None
    cfg = _read_json(os.path.join(tdir, "config.json"))
    arch = arch_from_hf_config(cfg, int(dc["out_features"]), dense_b is not None, max_seq)
    sd = _load_weights(tdir)
    pack = blob_from_distilbert_state_dict if cfg.get("model_type") == "distilbert" else blob_from_xlmr_state_dict
    blob = pack(sd, dense_w, dense_b, arch)
    tc = os.path.join(tdir, "tokenizer_config.json")
    lower = bool(_read_json(tc).get("do_lower_case", False)) if os.path.isfile(tc) else False
    tok = WordPieceTokenizer(os.path.join(tdir, "vocab.txt"), do_lower_case=lower, max_length=max_seq)
    return SentenceEncoder(arch, blob, tok, max_seq, bool(sbc.get("do_lower_case", False)), device, make_encoder)


def load_mclip(checkpoint_folder, tokenizer, device=0, make_encoder=BertTextEncoder):
    """M-CLIP (XLM-R + `LinearTransformation`) from a LOCAL folder -> the `model_txt_mclip(text) -> float32 [1, E]` callable of
    clip_back.py:854-858.  The folder holds M-CLIP's config.json (numDims / transformerDimensions), its weights
    (transformer.* and LinearTransformation.*) and optionally the base model's own config as xlmr_config.json; without that the
    shape is read off the tensors.  `tokenizer`: any callable `tok([text]) -> {"input_ids", "attention_mask"}` (SentencePiece is
    not restated here).  A text of more than 128 tokens raises ValueError: M-CLIP does not truncate, and neither does this."""
    folder = resolve_mclip_folder(checkpoint_folder)
    sd = _strip(_load_weights(folder), ("module.",))
    dense_w, dense_b = sd.pop("LinearTransformation.weight"), sd.pop("LinearTransformation.bias", None)
    sd = _strip(sd, ("transformer.",))
    xc = os.path.join(folder, "xlmr_config.json")
    out_dim = int(_np(dense_w).shape[0])
    if os.path.isfile(xc):
        arch = arch_from_hf_config(_read_json(xc), out_dim, dense_b is not None, MAX_TOKENS)
    else:
        word, pos = _np(sd["embeddings.word_embeddings.weight"]), _np(sd["embeddings.position_embeddings.weight"])
        layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layer."))
        width = word.shape[1]
        arch = BertArch(vocab=word.shape[0], max_pos=pos.shape[0], pos_offset=2, width=width, layers=layers, heads=width // 64,
                        mlp=_np(sd["encoder.layer.0.intermediate.dense.weight"]).shape[0], out_dim=out_dim,
                        dense_bias=dense_b is not None, max_len=MAX_TOKENS, ln_eps=1e-5)
    enc = make_encoder(arch, blob_from_xlmr_state_dict(sd, dense_w, dense_b, arch), device)

    def model_txt_mclip(text):
        tok = tokenizer([text])
        ids, mask = np.asarray(tok["input_ids"]), np.asarray(tok["attention_mask"])
        if int(mask.sum()) > MAX_TOKENS:
            raise ValueError(f"the text has {int(mask.sum())} tokens; this encoder takes at most {MAX_TOKENS} and does not truncate")
        return enc.encode_ids(ids[:, :MAX_TOKENS], attention_mask=mask[:, :MAX_TOKENS])

    model_txt_mclip.encoder = enc
    return model_txt_mclip
