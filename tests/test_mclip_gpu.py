"""The multilingual text towers (use_mclip) on the GPU: the three new kernels one by one, the ragged attention without the causal
mask, the whole tower against the HF models in fp32 on the CPU, its invariances, its refusals, and the mapper / service seams."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as ac  # noqa: E402
import bert_cases as bc  # noqa: E402

pytestmark = pytest.mark.gpu
E_ARG, E_UNSUPPORTED = -1, -5


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _i32(xs):
    return torch.tensor(np.asarray(xs, dtype=np.int32), device="cuda")


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)


def _ok(lib, rc):
    assert rc == 0, lib.clipx_last_error().decode()
    torch.cuda.synchronize()


def fp16_tol(want):
    return 1e-3 + 1.2e-3 * want.abs()  # the project's fp16 tolerance (test_clip_gpu.py: the fp16 residual epilogue)


# ------------------------------------------------------------------------------------------ 1. post-LN in place
def _ln64(x16, gamma, beta, eps):
    x = x16.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


@pytest.mark.parametrize("eps", [1e-12, 1e-5])
@pytest.mark.parametrize("M", [1, 33, 300])
@pytest.mark.parametrize("d", [256, 768, 1024])
def test_postln_kernel(lib, d, M, eps):
    g = torch.Generator().manual_seed(d + M)
    gamma = 1.0 + 0.2 * torch.randn(d, generator=g)
    beta = 0.3 * torch.randn(d, generator=g)
    const = torch.full((d,), 0.37).half()
    big = (3e4 * (2 * torch.rand(d, generator=g) - 1)).half()
    batches = [(torch.randn(M, d, generator=g) * 2 + 0.5).half()]
    if M >= 3:
        batches[0][1], batches[0][M - 1] = const, big
    else:
        batches += [const[None, :].clone(), big[None, :].clone()]
    gd, bd = gamma.cuda(), beta.cuda()  # (device tensors stay referenced until the kernel that reads them has run)
    for x in batches:
        xd = x.cuda()
        _ok(lib, lib.clipx_postln_f16_device(0, _ptr(xd), _ptr(gd), _ptr(bd), x.shape[0], d, C.c_float(eps), None))
        got = xd.cpu()
        want = _ln64(x, gamma, beta, eps)
        err = (got.double() - want).abs()
        print(f"postln d={d} M={x.shape[0]} eps={eps}: max err {float(err.max()):.3g}, worst err / tol {float((err / fp16_tol(want)).max()):.3f}")
        assert torch.isfinite(got.float()).all()
        for r in range(x.shape[0]):
            if (x[r] == x[r, 0]).all():  # the constant row: exact zeros after centring, so exactly beta -- no NaN, no inf * 0
                assert torch.equal(got[r].view(torch.int16), beta.half().view(torch.int16)), "a constant row must give fp16(beta) bit for bit"
        assert (err <= fp16_tol(want)).all(), f"max err {float(err.max()):.4g}"


# ------------------------------------------------------------------------------------------ 2. embedding + LayerNorm
@pytest.mark.parametrize("pos_offset", [0, 2])
@pytest.mark.parametrize("d", [256, 768])
def test_embed_kernel(lib, d, pos_offset):
    vocab, max_pos, T, eps = 500, 130, 128, 1e-5
    lens = [1, 2, 128]
    g = torch.Generator().manual_seed(d + pos_offset)
    word = torch.randn(vocab, d, generator=g) * 0.5
    pos = torch.randn(max_pos, d, generator=g) * 0.5
    gamma = 1.0 + 0.2 * torch.randn(d, generator=g)
    beta = 0.3 * torch.randn(d, generator=g)
    ids = torch.from_numpy(bc.synth_ids(3, lens, vocab, T, seed=3, lo=0))
    ids[2, 5], ids[2, 6] = vocab + 7, -3  # out of range where it IS read: clamped into the table (launch_text_embed's behaviour)
    offs, rows = _offsets(lens), sum(lens)
    dev = [t.cuda() for t in (word, pos, gamma, beta)]

    def run(ids_t, stride, offs_, lens_, n_rows):
        out = torch.full((n_rows + 1, d), 7.0, dtype=torch.float16, device="cuda")
        ids_d, offs_d, lens_d = ids_t.int().cuda(), _i32(offs_), _i32(lens_)
        _ok(lib, lib.clipx_bert_embed_device(0, _ptr(ids_d), stride, _ptr(offs_d), _ptr(lens_d), len(lens_), T, n_rows,
                                             _ptr(dev[0]), _ptr(dev[1]), pos_offset, max_pos, _ptr(dev[2]), _ptr(dev[3]), _ptr(out), d, vocab,
                                             C.c_float(eps), None))
        assert (out[n_rows].float() == 7.0).all(), "the row behind the last sample was written"
        return out[:n_rows].cpu()

    got = run(ids, T, offs, lens, rows)
    want = []
    for b, n in enumerate(lens):
        x = word[ids[b, :n].clamp(0, vocab - 1).long()] + pos[pos_offset:pos_offset + n]
        want.append(_ln64(x, gamma, beta, eps))
    want = torch.cat(want)
    err = (got.double() - want).abs()
    print(f"embed d={d} pos_offset={pos_offset}: max err {float(err.max()):.3g}, worst err / tol {float((err / fp16_tol(want)).max()):.3f}")
    assert (err <= fp16_tol(want)).all(), f"max err {float(err.max()):.4g}"
    # ids beyond lens are never read: garbage there, out of range included, changes no byte
    garbage = ids.clone()
    junk = torch.tensor([2 ** 31 - 1, -2 ** 31, vocab, -1, 123456789, 7], dtype=torch.int64)
    for b, n in enumerate(lens):
        garbage[b, n:] = junk[torch.arange(T - n) % len(junk)]
    assert torch.equal(run(garbage, T, offs, lens, rows).view(torch.int16), got.view(torch.int16))
    # packed ids (ids_stride 0) are the same rows
    packed = torch.cat([ids[b, :n] for b, n in enumerate(lens)])
    assert torch.equal(run(packed, 0, offs, lens, rows).view(torch.int16), got.view(torch.int16))
    # refusals launch nothing
    out = torch.full((4, d), 7.0, dtype=torch.float16, device="cuda")
    args = (_ptr(dev[0]), _ptr(dev[1]))
    ids_d, offs_d, lens_d = ids.int().cuda(), _i32(offs), _i32(lens)
    assert lib.clipx_bert_embed_device(0, _ptr(ids_d), T, _ptr(offs_d), _ptr(lens_d), 3, T, 4, *args, 3, max_pos, _ptr(dev[2]),
                                       _ptr(dev[3]), _ptr(out), d, vocab, C.c_float(eps), None) == E_ARG  # 3 + 128 > 130 positions
    assert lib.clipx_bert_embed_device(0, _ptr(ids_d), T, _ptr(offs_d), _ptr(lens_d), 3, T, 4, *args, 0, max_pos, _ptr(dev[2]),
                                       _ptr(dev[3]), _ptr(out), 200, vocab, C.c_float(eps), None) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out.float() == 7.0).all()


# ------------------------------------------------------------------------------------------ 3. masked mean + dense + normalise
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("E", [128, 512])
def test_pool_kernel(lib, E, bias):
    d = 1024
    lens = [1, 2, 31, 32, 33, 128, 5]  # the last sample is all zeros
    g = torch.Generator().manual_seed(E + bias)
    x = (torch.randn(sum(lens), d, generator=g) * 1.5 + 0.25).half()
    x[-5:] = 0
    W = torch.randn(E, d, generator=g) * d ** -0.5
    b = torch.randn(E, generator=g) * 0.1 if bias else None
    offs = _offsets(lens)
    B = len(lens)
    y_raw = torch.full((B, E), 7.0, device="cuda")
    o32 = torch.full((B, E), 7.0, device="cuda")
    o16 = torch.full((B, E), 7.0, dtype=torch.float16, device="cuda")
    xd, offs_d, lens_d, Wd, bd = x.cuda(), _i32(offs), _i32(lens), W.cuda(), (b.cuda() if bias else None)
    _ok(lib, lib.clipx_bert_pool_device(0, _ptr(xd), _ptr(offs_d), _ptr(lens_d), _ptr(Wd), _ptr(bd), _ptr(y_raw), _ptr(o32), _ptr(o16), B, d, E, None))
    y_raw, o32, o16 = y_raw.cpu(), o32.cpu(), o16.cpu()
    for i, (o, n) in enumerate(zip(offs, lens)):
        rows = x[o:o + n].double()
        p = rows.mean(0)
        want = W.double() @ p + (b.double() if bias else 0)
        # fp32 accumulation: 1e-5 sum_k |W_k p_k| for the dense layer (K = 1024 terms, gamma_K = K 2^-24 = 6e-5 worst case, 1e-5 in
        # expectation-free practice is the issue's figure) plus the same for the mean that feeds it (up to 128 terms per column)
        bound = 1e-5 * (W.double().abs() @ p.abs()) + 1e-5 * (W.double().abs() @ rows.abs().mean(0)) + 1e-30
        err = (y_raw[i].double() - want).abs()
        print(f"pool E={E} bias={bias} len={n}: worst err / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), f"sample {i} (length {n}): err / bound {float((err / bound).max()):.3f}"
        nrm = float(want.norm())
        if nrm == 0:
            assert (o32[i] == 0).all() and (o16[i].float() == 0).all(), "a zero row must give zeros, not NaN"
        else:
            assert abs(float(o32[i].double().norm()) - 1) < 1e-5
            assert ((o32[i].double() - want / nrm).abs() <= 2 * bound / nrm + 2e-7).all()
    if not bias:
        assert (y_raw[-1] == 0).all() and (o32[-1] == 0).all()
    assert torch.isfinite(o32).all()
    assert torch.equal(o16.view(torch.int16), o32.half().view(torch.int16)), "the fp16 output is the rounding of the f32 one"
    # the fp16 output is optional
    o32b, yb = torch.empty(B, E, device="cuda"), torch.empty(B, E, device="cuda")
    _ok(lib, lib.clipx_bert_pool_device(0, _ptr(xd), _ptr(offs_d), _ptr(lens_d), _ptr(Wd), _ptr(bd), _ptr(yb), _ptr(o32b), None, B, d, E, None))
    assert torch.equal(o32b.cpu(), o32)


# ------------------------------------------------------------------------------------------ 4. ragged attention, not causal
LENS_ATT = [33, 128, 1, 64, 127, 2, 31, 65, 32]  # {1, 2, 31, 32, 33, 64, 65, 127, 128} mixed in one batch


def test_ragged_attention_without_the_causal_mask(lib):
    """the launch the tower makes: one packed batch, causal = 0, T = the longest length; every sample within the element-wise bound
    E of tests/attention_cases.py (as test_attention_edges_gpu.py) of the float64 reference at its own length"""
    H, dh, lens = 2, 64, LENS_ATT
    offs, n = _offsets(lens), sum(lens)
    for fam in ac.families(0):
        qkv = ac.ragged(fam, lens, H, dh, 21, 0).cuda()
        assert qkv.shape[0] == n
        out = torch.full((n + 1, H * dh), 7.0, dtype=torch.bfloat16, device="cuda")
        offs_d, lens_d = _i32(offs), _i32(lens)
        _ok(lib, lib.clipx_attention_ex_device(0, _ptr(qkv), _ptr(out), len(lens), max(lens), H, dh, 0, 0, _ptr(offs_d), _ptr(lens_d), None))
        assert (out[n].float() == 7.0).all()
        for i, (o, ln) in enumerate(zip(offs, lens)):
            mine = qkv[o:o + ln]
            want, pav = ac.reference(mine, 1, ln, H, dh, 0)
            ratio = ac.worst(out[o:o + ln], want, pav, ln, ac.vmax_of(mine, H, dh))
            assert ratio <= 1.0, f"{fam} sample {i} (length {ln}): err/E {ratio:.3f}"


# ------------------------------------------------------------------------------------------ 5. the whole tower
def _arch(kind, **kw):
    from clip_retrieval_amd.mclip import BertArch

    base = dict(pos_offset=0, dense_bias=False, ln_eps=1e-12) if kind == "distilbert" else dict(pos_offset=2, dense_bias=True, ln_eps=1e-5)
    return BertArch(**{**base, **kw})


TINY = dict(vocab=1000, max_pos=130, width=256, layers=2, heads=4, mlp=512, out_dim=128, max_len=128)
LENS40 = (bc.LENS_EDGE * 5)[:40]


def _build(kind, arch, seed):
    from clip_retrieval_amd import mclip

    model, dw, db = bc.hf_model(kind, arch, seed=seed)
    pack = mclip.blob_from_distilbert_state_dict if kind == "distilbert" else mclip.blob_from_xlmr_state_dict
    return model, dw, db, mclip.BertTextEncoder(arch, pack(model.state_dict(), dw, db, arch), 0)


@pytest.fixture(scope="module", params=["distilbert", "xlmr"])
def tiny(request):
    """the tiny tower of one family member, 40 texts and their HF fp32 embeddings (computed once, shared, never changed)"""
    kind = request.param
    arch = _arch(kind, **TINY)
    model, dw, db, enc = _build(kind, arch, seed=11)
    ids = bc.synth_ids(40, LENS40, arch.vocab, arch.max_len, seed=12, per_sample=3)
    want = bc.unit(bc.hf_forward(model, dw, db, ids, LENS40, pad_id=1 if kind == "xlmr" else 0))
    want.setflags(write=False)
    yield kind, arch, enc, ids, np.asarray(LENS40, dtype=np.int32), want
    enc.close()


def _gate(got, want, what):
    from oracle.clip_oracle import NORTH_STAR_BAR, parity_gate, parity_report

    rep = parity_report(got, want)
    print(f"{what}: 1 - cos max {1 - rep['cos'].min():.3g}" + ("" if rep["centred"] is None else
          f", centred min {rep['centred'].min():.5f}, nearest wrong row at {rep['other'].max():.4f}"))
    parity_gate(got, want, what, bar=NORTH_STAR_BAR)


@pytest.mark.parametrize("B", [1, 9, 40])
def test_tiny_tower_against_hf(tiny, B):
    kind, arch, enc, ids, lens, want = tiny
    got, got16 = enc.encode_ids(ids[:B], lens=lens[:B], f16=True)
    assert got.dtype == np.float32 and got.shape == (B, arch.out_dim) and got16.dtype == np.float16
    _gate(got, want[:B], f"tiny {kind} B={B}")
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-5
    assert np.array_equal(got16, got.astype(np.float16))
    if B == 1:  # the longest text alone, and through the attention-mask spelling of the lengths
        one = enc.encode_ids(ids[1:2], attention_mask=(np.arange(128)[None, :] < lens[1]).astype(np.int64))
        _gate(np.concatenate([one, got]), want[[1, 0]], f"tiny {kind} row 1 alone")


def test_tiny_tower_invariances(tiny):
    kind, arch, enc, ids, lens, want = tiny
    base = enc.encode_ids(ids, lens=lens)
    garbage = ids.copy()
    rng = np.random.default_rng(5)
    for b, n in enumerate(lens):
        garbage[b, n:] = rng.integers(0, arch.vocab, arch.max_len - n)
    again = enc.encode_ids(garbage, lens=lens)
    assert np.array_equal(again.view(np.int32), base.view(np.int32)), "a tower that ignores the mask: rows changed with the ids past lens"
    perm = rng.permutation(len(lens))
    shuffled = enc.encode_ids(ids[perm], lens=lens[perm])
    cos = (shuffled.astype(np.float64) * base[perm].astype(np.float64)).sum(1)
    print(f"tiny {kind}: 1 - cos under a permutation of the batch {float((1 - cos).max()):.3g}")
    assert (1 - cos).max() < 1e-5
    # device pointers: the same bytes as the host entry point
    ids_d = torch.from_numpy(ids).cuda()
    o32 = torch.empty(len(lens), arch.out_dim, device="cuda")
    enc.encode_ids_device(ids_d.data_ptr(), lens, len(lens), o32.data_ptr())
    enc.check_range()
    assert np.array_equal(o32.cpu().numpy().view(np.int32), base.view(np.int32))


def test_chunked_batches_give_the_same_rows(tiny, monkeypatch):
    """any B >= 1 is chunked internally: a handle with room for 16 texts per chunk gives the rows of the unchunked call (1 - cos < 1e-5;
    a chunk's longest text picks the attention instantiation, so the bits may differ)"""
    from clip_retrieval_amd import mclip

    kind, arch, enc, ids, lens, want = tiny
    monkeypatch.setenv("CLIPX_MAX_BATCH", "16")
    small = mclip.BertTextEncoder(arch, mclip.random_bert_blob(arch, 4), 0)
    monkeypatch.delenv("CLIPX_MAX_BATCH")
    big = mclip.BertTextEncoder(arch, mclip.random_bert_blob(arch, 4), 0)
    a, b = small.encode_ids(ids, lens=lens), big.encode_ids(ids, lens=lens)
    small.close()
    big.close()
    assert (1 - (a.astype(np.float64) * b.astype(np.float64)).sum(1)).max() < 1e-5


FULL = {"distilbert": dict(vocab=2000, max_pos=512, width=768, layers=6, heads=12, mlp=3072, out_dim=512, max_len=128),
        "xlmr": dict(vocab=2000, max_pos=514, width=1024, layers=24, heads=16, mlp=4096, out_dim=768, max_len=128)}


@pytest.mark.parametrize("kind", ["distilbert", "xlmr"])
def test_full_depth_tower_against_hf(kind):
    """the DistilBERT-multilingual and XLM-R-large shapes (vocabulary cut to 2 000), random weights, B = 4"""
    arch = _arch(kind, **FULL[kind])
    model, dw, db, enc = _build(kind, arch, seed=21)
    lens = [128, 33, 2, 65]
    ids = bc.synth_ids(4, lens, arch.vocab, arch.max_len, seed=22, per_sample=3)
    want = bc.unit(bc.hf_forward(model, dw, db, ids, lens, pad_id=1 if kind == "xlmr" else 0))
    got = enc.encode_ids(ids, lens=np.asarray(lens))
    enc.close()
    _gate(got, want, f"full {kind}")


# ------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_launch_nothing(lib, tiny):
    from clip_retrieval_amd import HipLibraryError, mclip

    kind, arch, enc, ids, lens, want = tiny
    for bad, word in ((dict(max_len=129), "128"), (dict(width=640, heads=8, mlp=512), "64"), (dict(width=320, heads=5), "128")):
        a = _arch(kind, **{**TINY, **bad})
        desc, h = a.to_desc(), C.c_void_p()
        blob = np.zeros(8, dtype=np.float32)  # the description is refused before the blob is looked at
        assert lib.clipx_bert_create(C.byref(desc), blob.ctypes.data, blob.size, 0, C.byref(h)) == E_UNSUPPORTED and not h
        assert word in lib.clipx_last_error().decode()
    with pytest.raises(HipLibraryError):
        mclip.BertTextEncoder(_arch(kind, **{**TINY, "max_len": 129}), np.zeros(8, dtype=np.float32), 0)
    rect = np.ascontiguousarray(ids[:3], dtype=np.int32)
    out = np.full((3, arch.out_dim), 7.0, dtype=np.float32)
    for bad_lens in ([5, 0, 7], [5, 129, 7], [5, -1, 7]):
        ln = np.asarray(bad_lens, dtype=np.int32)
        assert lib.clipx_bert_encode(enc._h, rect.ctypes.data, ln.ctypes.data, 3, out.ctypes.data, None) == E_ARG
        assert "lens[1]" in lib.clipx_last_error().decode()
        o_d = torch.full((3, arch.out_dim), 7.0, device="cuda")
        rect_d = torch.from_numpy(rect).cuda()
        assert lib.clipx_bert_encode_device(enc._h, _ptr(rect_d), ln.ctypes.data, 3, _ptr(o_d), None, None) == E_ARG
        torch.cuda.synchronize()
        assert (o_d == 7.0).all() and (out == 7.0).all()
    # the handle still serves
    _gate(enc.encode_ids(ids[:3], lens=lens[:3]), want[:3], "after the refusals")


# ------------------------------------------------------------------------------------------ 7. mapper and service
def test_mapper_and_service_use_mclip(tmp_path):
    from types import SimpleNamespace

    from clip_retrieval_amd import mclip
    from clip_retrieval_amd.encoder import ClipArch, ClipEncoder, register_encoder
    from clip_retrieval_amd.knn import Mi355xIndex
    from clip_retrieval_amd.mapper import ClipMapper
    from clip_retrieval_amd.service import KnnHotPath
    from oracle.clip_oracle import ARCHS, HFClipOracle

    root = str(tmp_path / "clip-ViT-B-32-multilingual-v1")
    os.makedirs(root)
    arch = mclip.BertArch(vocab=len(bc.VOCAB), max_pos=40, pos_offset=0, width=128, layers=2, heads=2, mlp=256, out_dim=64, dense_bias=False,
                          max_len=12, ln_eps=1e-12)
    model, dw = bc.write_st_folder(root, bc.write_vocab(tmp_path / "v.txt"), arch)
    oarch = ARCHS["tiny-B/32"]
    clip = ClipEncoder(ClipArch(**{k: getattr(oarch, k) for k in ClipArch.__dataclass_fields__}), HFClipOracle(oarch, seed=0).export_blob(), 0)
    register_encoder("mclip-test", clip)
    m = ClipMapper(enable_image=False, enable_text=True, enable_metadata=False, use_mclip=True, clip_model="registered:mclip-test",
                   use_jit=False, mclip_model=os.path.basename(root), warmup_batch_size=1, clip_cache_path=str(tmp_path))
    texts = ["hello world", "unbelievable, hello!", "中国人", "café naïve a b c", "", "a b c a b c a b c a b c a b c a b c"]
    embs = m({"text": texts, "text_tokens": None})["text_embs"]
    assert embs.dtype == np.float32 and embs.shape == (len(texts), 64)
    assert np.abs(np.linalg.norm(embs, axis=1) - 1).max() < 1e-5
    st = mclip.load_sentence_transformer(root)
    tok = st.tokenize(texts)
    assert tok["input_ids"].shape[1] == 12  # the long text is truncated to max_seq_length
    direct = st._enc.encode_ids(tok["input_ids"], attention_mask=tok["attention_mask"])
    assert np.allclose(embs, direct, atol=1e-6)
    # and the tower is the HF model of the folder
    blob = mclip.blob_from_distilbert_state_dict(model.state_dict(), dw, None, arch)
    want = bc.unit(bc.forward(blob, arch, tok["input_ids"], tok["attention_mask"].sum(1)))
    _gate(embs, want, "mapper use_mclip")

    # service: the M-CLIP callable -> compute_query -> knn_search finds the planted image row
    def model_txt_mclip(text):
        t = st.tokenize([text])
        return st._enc.encode_ids(t["input_ids"], attention_mask=t["attention_mask"])

    rng = np.random.default_rng(0)
    rows = rng.standard_normal((500, 64)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows[123] = embs[1]
    ix = Mi355xIndex(64)
    ix.add(rows.astype(np.float16))
    res = SimpleNamespace(model_txt_mclip=model_txt_mclip, image_index=ix, text_index=ix, metadata_is_ordered_by_ivf=False, safety_model=None,
                          violence_detector=None, aesthetic_embeddings=None)
    hp = KnnHotPath()
    q = hp.compute_query(res, texts[1], None, None, None, use_mclip=True)
    assert q.dtype == np.float32 and q.shape == (1, 64) and abs(float(np.linalg.norm(q)) - 1) < 1e-5
    dist, ids = hp.knn_search(q, "image", 5, res, deduplicate=False, use_safety_model=False, use_violence_detector=False)
    assert ids[0] == 123 and dist[0] > 0.999
    with pytest.raises(NotImplementedError):
        hp.compute_query(SimpleNamespace(aesthetic_embeddings=None), texts[1], None, None, None, use_mclip=True)
    ix.close()
    st.close()
    clip.close()
