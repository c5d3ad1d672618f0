"""use_mclip without a GPU: the WordPiece restatement against transformers.BertTokenizer, the blob packers against the HF models (through
the blob-only fp32 restatement of tests/bert_cases.py), the folder loader, and the mapper / service seams with a stub tower."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_cases as bc  # noqa: E402

VOCAB = bc.VOCAB


@pytest.fixture(scope="module")
def vocab_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("wp") / "vocab.txt"
    p.write_text("\n".join(VOCAB) + "\n", encoding="utf-8")
    return str(p)


TEXTS = ["hello world", "unbelievable", "unbelievables!", "Hello, world. hello?", "café cafe naïve", "中国人 hello", "hello中国world",
         "zzzz hello", "", "   ", "a b c a b c a b c a b c", "hello\tworld\nhello world", "he\u0000llo wor‍ld", "(ab)-ab12",
         "x" * 101, "Straße straße", "hello [SEP] world [MASK]", "café", "don't", "aab abc cab"]


def test_wordpiece_equals_bert_tokenizer(vocab_file):
    """id for id: continuation pieces, punctuation, accents kept (do_lower_case=False), CJK, an unknown word, the empty string ->
    [CLS][SEP], and truncation at max_length 8.  (transformers.BertTokenizer builds offline from a vocab.txt.)"""
    import transformers

    from clip_retrieval_amd.mclip import WordPieceTokenizer

    ref = transformers.BertTokenizer(vocab_file, do_lower_case=False)
    mine = WordPieceTokenizer(vocab_file, do_lower_case=False)
    for t in TEXTS:
        assert mine.encode(t, 128) == ref.encode(t, max_length=128, truncation=True), repr(t)
        assert mine.encode(t, 8) == ref.encode(t, max_length=8, truncation=True), repr(t)
    assert mine.encode("") == [VOCAB.index("[CLS]"), VOCAB.index("[SEP]")]
    assert VOCAB.index("[UNK]") in mine.encode("zzzz hello")
    assert len(mine.encode("a b c a b c a b c a b c", 8)) == 8
    got = mine(TEXTS[:4])
    want = ref(TEXTS[:4], padding=True, truncation=True, max_length=128, return_tensors="np")
    assert np.array_equal(got["input_ids"], want["input_ids"]) and np.array_equal(got["attention_mask"], want["attention_mask"])


def test_wordpiece_lower_case_variant(vocab_file):
    import transformers

    from clip_retrieval_amd.mclip import WordPieceTokenizer

    ref = transformers.BertTokenizer(vocab_file, do_lower_case=True)
    mine = WordPieceTokenizer(vocab_file, do_lower_case=True)
    for t in TEXTS:
        assert mine.encode(t, 128) == ref.encode(t, max_length=128, truncation=True), repr(t)


def _tiny(kind):
    from clip_retrieval_amd.mclip import BertArch

    if kind == "distilbert":
        return BertArch(vocab=300, max_pos=40, pos_offset=0, width=128, layers=2, heads=2, mlp=256, out_dim=64, dense_bias=False, max_len=16,
                        ln_eps=1e-12)
    return BertArch(vocab=300, max_pos=40, pos_offset=2, width=128, layers=2, heads=2, mlp=256, out_dim=64, dense_bias=True, max_len=16,
                    ln_eps=1e-5)


@pytest.mark.parametrize("kind", ["distilbert", "xlmr"])
def test_packed_blob_reproduces_the_hf_model(kind):
    """blob order, q|k|v stacking, pos_offset = 2 and the folded token-type row: the restatement, which reads only the blob, gives the
    HF model's masked-mean-pooled, dense-projected output to fp32 round-off."""
    from clip_retrieval_amd import mclip

    arch = _tiny(kind)
    model, dw, db = bc.hf_model(kind, arch, seed=3)
    if kind == "xlmr":
        with torch.no_grad():
            model.embeddings.token_type_embeddings.weight.normal_(0, 0.5)  # a type row that is visible if it is not folded
    pack = mclip.blob_from_distilbert_state_dict if kind == "distilbert" else mclip.blob_from_xlmr_state_dict
    blob = pack(model.state_dict(), dw, db, arch)
    assert blob.dtype == np.float32 and blob.size == mclip.expected_blob_floats(arch)
    lens = [1, 2, 7, 16, 9]
    ids = bc.synth_ids(len(lens), lens, arch.vocab, arch.max_len, seed=4)
    want = bc.hf_forward(model, dw, db, ids, lens, pad_id=1 if kind == "xlmr" else 0)
    got = bc.forward(blob, arch, ids, lens)
    assert np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max()), np.abs(got - want).max()
    garbage = ids.copy()
    for b, n in enumerate(lens):
        garbage[b, n:] = 299
    assert np.array_equal(bc.forward(blob, arch, garbage, lens), got)


def test_blob_floats_agrees_with_the_packers(lib):
    from clip_retrieval_amd import mclip

    for arch in list(mclip.BERT_ARCHS.values()) + [_tiny("distilbert"), _tiny("xlmr")]:
        assert mclip.bert_blob_floats(arch) == mclip.expected_blob_floats(arch)
    arch = _tiny("xlmr")
    assert mclip.random_bert_blob(arch, 0).size == mclip.bert_blob_floats(arch)


# ------------------------------------------------------------------------------------------ folder loader
class StubTower:
    """stands in for BertTextEncoder: float32 rows that depend on the tokens only"""

    def __init__(self, arch, blob, device):
        self.arch, self.blob, self.calls = arch, blob, []

    def encode_ids(self, ids, lens=None, attention_mask=None):
        ids, m = np.asarray(ids), np.asarray(attention_mask)
        self.calls.append((ids.copy(), m.copy()))
        rows = np.zeros((ids.shape[0], self.arch.out_dim), dtype=np.float32)
        for b in range(ids.shape[0]):
            for t in range(int(m[b].sum())):
                rows[b, (int(ids[b, t]) * 7 + t) % self.arch.out_dim] += 1.0 + t
        return rows / np.linalg.norm(rows, axis=1, keepdims=True)

    def close(self):
        pass


@pytest.fixture(scope="module")
def st_folder(tmp_path_factory, vocab_file):
    from clip_retrieval_amd.mclip import BertArch

    root = str(tmp_path_factory.mktemp("cache") / "clip-ViT-B-32-multilingual-v1")
    os.makedirs(root)
    arch = BertArch(vocab=len(VOCAB), max_pos=32, pos_offset=0, width=128, layers=2, heads=2, mlp=256, out_dim=64, dense_bias=False, max_len=12,
                    ln_eps=1e-12)
    model, dw = bc.write_st_folder(root, vocab_file, arch)
    return root, arch, model, dw


@pytest.mark.parametrize("how", ["path", "name_under_cache", "org_name_under_cache"])
def test_load_sentence_transformer_reads_a_local_folder(st_folder, how):
    from clip_retrieval_amd import mclip

    root, arch, model, dw = st_folder
    name, cache = {"path": (root, None), "name_under_cache": (os.path.basename(root), os.path.dirname(root)),
                   "org_name_under_cache": ("sentence-transformers/" + os.path.basename(root), os.path.dirname(root))}[how]
    st = mclip.load_sentence_transformer(name, cache, make_encoder=StubTower)
    assert st.arch == arch and st.max_seq_length == 12
    want = mclip.blob_from_distilbert_state_dict(model.state_dict(), dw, None, arch)
    assert np.array_equal(st._enc.blob, want)
    out = st.encode(["hello world", "a b c a b c a b c a b c a b c", ""])
    assert out.dtype == np.float32 and out.shape == (3, 64)
    ids, mask = st._enc.calls[-1]
    assert ids.shape[1] == 12 and mask.sum(1).tolist() == [4, 12, 2]  # truncated to max_seq_length, [CLS] [SEP] for the empty string


def test_missing_folder_is_a_clear_error(tmp_path):
    from clip_retrieval_amd import mclip

    with pytest.raises(FileNotFoundError, match="nothing is fetched"):
        mclip.load_sentence_transformer("sentence-transformers/clip-ViT-B-32-multilingual-v1", str(tmp_path), make_encoder=StubTower)
    with pytest.raises(FileNotFoundError):
        mclip.load_sentence_transformer(str(tmp_path / "nope"), None, make_encoder=StubTower)
    # the same error is still the NotImplementedError that use_mclip raised before the towers existed (callers that catch it keep working)
    with pytest.raises(NotImplementedError):
        mclip.load_sentence_transformer(str(tmp_path / "nope"), None, make_encoder=StubTower)


def test_load_mclip_refuses_long_texts_and_returns_one_row(tmp_path):
    from clip_retrieval_amd import mclip

    arch = _tiny("xlmr")
    model, dw, db = bc.hf_model("xlmr", arch, seed=6)
    sd = {"transformer." + k: v for k, v in model.state_dict().items()}
    sd["LinearTransformation.weight"], sd["LinearTransformation.bias"] = dw, db
    torch.save(sd, str(tmp_path / "pytorch_model.bin"))
    json.dump({"modelBase": "xlm-roberta-large", "numDims": arch.out_dim, "transformerDimensions": arch.width}, open(tmp_path / "config.json", "w"))

    def tok(texts):
        n = len(texts[0].split())
        return {"input_ids": np.arange(5, 5 + n)[None, :] % 300, "attention_mask": np.ones((1, n), dtype=np.int64)}

    fn = mclip.load_mclip(str(tmp_path), tok, make_encoder=StubTower)
    enc = fn.encoder
    assert (enc.arch.vocab, enc.arch.max_pos, enc.arch.pos_offset, enc.arch.width, enc.arch.layers, enc.arch.mlp, enc.arch.out_dim,
            enc.arch.dense_bias, enc.arch.max_len) == (300, 40, 2, 128, 2, 256, 64, True, 128)
    assert np.array_equal(enc.blob, mclip.blob_from_xlmr_state_dict(model.state_dict(), dw, db, enc.arch))
    out = fn("a b c")
    assert out.shape == (1, 64) and out.dtype == np.float32
    assert fn(" ".join(["w"] * 128)).shape == (1, 64)
    with pytest.raises(ValueError, match="128"):
        fn(" ".join(["w"] * 129))


# ------------------------------------------------------------------------------------------ mapper and service
def test_mapper_use_mclip_returns_float32_unit_rows(st_folder, monkeypatch):
    from clip_retrieval_amd import mapper as mp
    from clip_retrieval_amd import mclip

    root, arch, _, _ = st_folder
    monkeypatch.setattr(mp, "get_encoder", lambda *a, **k: object())
    real = mclip.load_sentence_transformer
    monkeypatch.setattr(mclip, "load_sentence_transformer", lambda m, c, d: real(m, c, d, make_encoder=StubTower))
    m = mp.ClipMapper(enable_image=False, enable_text=True, enable_metadata=True, use_mclip=True, clip_model="ViT-B/32", use_jit=False,
                      mclip_model=root, warmup_batch_size=0)
    item = {"text": ["hello world", "café", "中国人"], "text_tokens": None, "metadata": ["m0", "m1", "m2"]}
    for out in (m(item), m.collect(m.submit(item))):
        e = out["text_embs"]
        assert e.dtype == np.float32 and e.shape == (3, 64) and out["image_embs"] is None
        assert np.allclose(np.linalg.norm(e, axis=1), 1, atol=1e-6)
        assert out["text"] == item["text"] and out["metadata"] == item["metadata"]
    assert not np.allclose(e[0], e[1])


def test_compute_query_use_mclip():
    from types import SimpleNamespace

    from clip_retrieval_amd.service import KnnHotPath

    hot = KnnHotPath.__new__(KnnHotPath)  # compute_query touches no state of the object
    seen = []

    def model_txt_mclip(text):
        seen.append(text)
        return np.arange(1, 9, dtype=np.float32)[None, :] * 3

    res = SimpleNamespace(model_txt_mclip=model_txt_mclip, aesthetic_embeddings=None)
    q = hot.compute_query(res, "bonjour le monde", None, None, None, use_mclip=True)
    assert seen == ["bonjour le monde"] and q.dtype == np.float32 and q.shape == (1, 8)
    assert abs(float(np.linalg.norm(q)) - 1) < 1e-6 and np.allclose(q[0] * np.linalg.norm(np.arange(1, 9)), np.arange(1, 9))
    # the reference's callable returns one row [E] (clip_back.py:856): normalized() makes it [1, E]
    res1 = SimpleNamespace(model_txt_mclip=lambda t: np.arange(1, 9, dtype=np.float32), aesthetic_embeddings=None)
    assert hot.compute_query(res1, "x", None, None, None, use_mclip=True).shape == (1, 8)
    with pytest.raises(NotImplementedError, match="model_txt_mclip"):
        hot.compute_query(SimpleNamespace(aesthetic_embeddings=None), "hola", None, None, None, use_mclip=True)
    # an embedding query does not need the tower, whatever the flag
    q = hot.compute_query(SimpleNamespace(aesthetic_embeddings=None), None, None, None, [1.0, 0.0], use_mclip=True)
    assert q.shape == (1, 2)
