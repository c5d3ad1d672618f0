"""ViT-g/14 and ViT-bigG/14 on the GPU: the attention kernel at head dimensions 88 and 104 (a half k-step closes QK^T), the row-wise
kernels at widths 1408 and 1664 (odd multiples of 128), the GEMMs at the new shapes, and two-layer encoders of both models against
the CPU oracle.  Bars and references are the ones the existing per-kernel and encoder tests apply (named at each test)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
E_UNSUPPORTED = -5
SENTINEL = 7.0
DHS = (88, 104)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


@pytest.fixture(scope="module")
def lib():
    import clip_retrieval_amd

    return clip_retrieval_amd.load_library()


# ------------------------------------------------------------------------------------------ attention
def _inputs(B, T, H, dh):
    """tests/test_long_seq_gpu.py's inputs: randn in fp16 from the CPU generator seeded T * 31 + H, q scaled by 2"""
    g = torch.Generator().manual_seed(T * 31 + H)
    qkv = (torch.randn(B * T, 3 * H * dh, generator=g)).to(torch.float16)
    qkv[:, : H * dh] *= 2.0
    return qkv


def _reference(qkv, B, T, H, dh):
    """fp32 softmax(q k^T / sqrt(dh)) v on the same fp16 inputs -> ([B T, H dh] fp32, probabilities, logits)"""
    q, k, v = qkv.float().view(B, T, 3, H, dh).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * dh ** -0.5
    p = torch.softmax(s, -1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B * T, H * dh), p, s


def _assert_close(out, want, what, scale=1.0):
    """tests/test_long_seq_gpu.py's bars: max abs error < 2e-2, mean < 2e-3 (`scale` divides the error of a head whose inputs were
    scaled up by it: the bars are absolute)"""
    assert torch.isfinite(out.float()).all(), f"{what}: NaN or Inf in the output"
    err = (out.float() - want).abs() / scale
    print(f"{what}: max abs err {err.max().item():.4g} mean {err.mean().item():.4g}")
    assert err.max() < 2e-2, f"{what}: max err {err.max().item():.4g} at {err.argmax().item()}"
    assert err.mean() < 2e-3, f"{what}: mean err {err.mean().item():.4g}"


def _run(lib, qkv, B, T, H, dh, q_blocks=None):
    """A checked launch into a buffer of exactly B T rows, pre-filled with a sentinel.  q_blocks None: clipx_attention_dh_device."""
    from clip_retrieval_amd._lib import check

    assert qkv.shape == (B * T, 3 * H * dh) and qkv.is_contiguous()  # sized exactly: nothing lies behind the last head of the last row
    out = torch.full((B * T, H * dh), SENTINEL, dtype=torch.bfloat16, device="cuda")
    if q_blocks is None:
        check(lib, lib.clipx_attention_dh_device(0, _ptr(qkv), _ptr(out), B, T, H, dh, 0, None), "clipx")
    else:
        check(lib, lib.clipx_attention_ex_device(0, _ptr(qkv), _ptr(out), B, T, H, dh, 0, q_blocks, None, None, None), "clipx")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("T", [1, 32, 33, 50, 96, 257, 258, 288])
@pytest.mark.parametrize("dh", DHS)
def test_wide_attention_vs_fp32(lib, dh, T):
    """B = 2, H = 3: every row of the plan (1, 2, 3 and 9 key blocks), whole last blocks (32, 96, 288), one real key in the last
    block (33, 257), two (258).  Three heads and two batch rows, so a fragment or chunk that reaches into the next head or the next
    token reads other data than its own.  Through both entry points; at T = 257 also the pooled launch (q_blocks = 1), whose query
    rows 0 .. 31 must be the bits of the full launch and every other row untouched."""
    B, H = 2, 3
    qkv = _inputs(B, T, H, dh).cuda()
    want, _, _ = _reference(qkv, B, T, H, dh)
    out = _run(lib, qkv, B, T, H, dh)
    _assert_close(out, want, f"dh={dh} T={T}")
    out_ex = _run(lib, qkv, B, T, H, dh, q_blocks=0)
    assert torch.equal(out.view(torch.int16), out_ex.view(torch.int16)), "the two entry points run the same kernel"
    if T == 257:
        pooled = _run(lib, qkv, B, T, H, dh, q_blocks=1).view(B, T, H * dh)
        _assert_close(pooled[:, :32], want.view(B, T, H * dh)[:, :32], f"dh={dh} T={T} q_blocks=1")
        assert torch.equal(pooled[:, :32].contiguous().view(torch.int16), out.view(B, T, H * dh)[:, :32].contiguous().view(torch.int16))
        assert (pooled[:, 32:].float() == SENTINEL).all(), "the pooled launch writes query block 0 only"


@pytest.mark.parametrize("big_head", [1, 0])
@pytest.mark.parametrize("dh", DHS)
def test_neighbouring_head_does_not_leak(lib, dh, big_head):
    """T = 257, B = 1, H = 2, the qkv tensor sized exactly.  One head's q, k, v are the ordinary inputs times 30, the other's the
    ordinary inputs; the ordinary head must meet the bars of test_wide_attention_vs_fp32 -- what fails if the hb = 1 half of the last
    k-step or the pad rows of V^T pick up the neighbouring head: a leak of 8 columns at 900 x the products.  Both orders, so each
    head is the last of the row once (its half step would read past the row, on the last token past the allocation).  The
    magnitude-30 head is checked too, its error divided by 30 (the bars are absolute)."""
    B, T, H = 1, 257, 2
    qkv = _inputs(B, T, H, dh)
    view = qkv.view(B * T, 3, H, dh)
    view[:, :, big_head] *= 30.0
    assert torch.isfinite(qkv).all()
    qkv = qkv.cuda()
    want, _, _ = _reference(qkv, B, T, H, dh)
    out = _run(lib, qkv, B, T, H, dh)
    small = 1 - big_head
    _assert_close(out.view(T, H, dh)[:, small], want.view(T, H, dh)[:, small], f"dh={dh} ordinary head {small} beside a head x 30")
    _assert_close(out.view(T, H, dh)[:, big_head], want.view(T, H, dh)[:, big_head], f"dh={dh} the x 30 head {big_head}", scale=30.0)


@pytest.mark.parametrize("dh", DHS)
def test_one_dominant_key(lib, dh):
    """test_long_attention_online_softmax_corners' construction at T = 257 (8 blocks of 32 keys + one key), one head, |v| <= 2.
    Queries i % 3 == 0: key 256 -- the only real key of the last block -- has the largest logit by more than 2; i % 3 == 1: key 0
    has it; i % 3 == 2: q = 8 k[j], a softmax that is one-hot to fp16, j walking over all nine blocks.  A one-hot row is its key's
    V row to the bf16 rounding: a NaN (0 x NaN from an unwritten pad chunk) or a stale chunk in the half k-step moves it, where
    random inputs can hide that under the 2e-2 bar."""
    B, T, H = 1, 257, 1
    g = torch.Generator().manual_seed(257 + dh)
    u = torch.where(torch.rand(dh, generator=g) < 0.5, -1.0, 1.0)
    k = torch.randn(T, dh, generator=g)
    k *= 8.0 / k.norm(dim=1, keepdim=True)
    k[256], k[0] = 1.25 * u, -1.25 * u
    v = torch.randn(T, dh, generator=g).clamp_(-2, 2)
    q = torch.empty(T, dh)
    i = torch.arange(T)
    last, first, hot = i % 3 == 0, i % 3 == 1, i % 3 == 2
    noise = 0.25 * torch.randn(T, dh, generator=g)
    q[last] = 2.0 * (0.45 * u + noise[last])
    q[first] = 2.0 * (-0.45 * u + noise[first])
    target = (i * 7) % T
    target[254], target[2] = 256, 0  # the two planted keys as one-hot targets too: the single key of the last block, the first key
    q[hot] = 8.0 * k[target[hot]]
    qkv = torch.cat([q, k, v], 1).to(torch.float16).cuda()
    want, p, s = _reference(qkv, B, T, H, dh)
    p, s = p[0, 0], s[0, 0]
    # the crafting holds in the reference itself
    others = s.clone()
    others[:, 256] = float("-inf")
    assert (s[last.cuda(), 256] - others[last.cuda()].max(-1).values).min() > 2.0
    others = s.clone()
    others[:, 0] = float("-inf")
    assert (s[first.cuda(), 0] - others[first.cuda()].max(-1).values).min() > 2.0
    ph = p[hot.cuda()]
    assert (ph.argmax(-1).cpu() == target[hot]).all() and ph.max(-1).values.min() > 1 - 1e-6
    second = ph.clone().scatter_(1, ph.argmax(-1, keepdim=True), 0.0).max()
    assert second < 2.0 ** -25, "every P outside the one key must round to 0 in fp16"
    assert set((target[hot] // 32).tolist()) == set(range(9)), "the one-hot key visits every key block"
    out = _run(lib, qkv, B, T, H, dh)
    _assert_close(out, want, f"crafted T=257 dh={dh}")
    got_hot = out[hot.cuda()].float().cpu()
    v_hot = v.to(torch.float16).float()[target[hot]]
    assert ((got_hot - v_hot).abs() <= v_hot.abs() * 2.0 ** -8).all()


def test_wide_refusals_launch_nothing(lib):
    """dh 88 causal, dh 104 at T = 128 (4 key blocks), dh 88 at T = 300, dh 104 ragged and dh 96: CLIPX_E_UNSUPPORTED, a message that
    names the limit, and the sentinel-filled output untouched."""
    T = 300
    qkv = torch.zeros(T, 3 * 104, dtype=torch.float16, device="cuda")
    out = torch.full((T, 104), SENTINEL, dtype=torch.bfloat16, device="cuda")
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    lens = torch.full((1,), 77, dtype=torch.int32, device="cuda")

    def ex(T, dh, causal, offs=None, lens=None):
        rc = lib.clipx_attention_ex_device(0, _ptr(qkv), _ptr(out), 1, T, 1, dh, causal, 0, _ptr(offs), _ptr(lens), None)
        return rc, lib.clipx_last_error().decode()

    def plain(T, dh, causal):
        rc = lib.clipx_attention_dh_device(0, _ptr(qkv), _ptr(out), 1, T, 1, dh, causal, None)
        return rc, lib.clipx_last_error().decode()

    for call in (ex, plain):
        rc, msg = call(257, 88, 1)
        assert rc == E_UNSUPPORTED and "causal" in msg and "88" in msg, msg
        rc, msg = call(128, 104, 0)
        assert rc == E_UNSUPPORTED and "97" in msg and "256" in msg and "104" in msg, msg
        rc, msg = call(300, 88, 0)
        assert rc == E_UNSUPPORTED and "288" in msg, msg
        rc, msg = call(77, 96, 0)
        assert rc == E_UNSUPPORTED and "88" in msg and "104" in msg, msg
    rc, msg = ex(77, 104, 0, one, lens)
    assert rc == E_UNSUPPORTED and "ragged" in msg and "64" in msg, msg
    torch.cuda.synchronize()
    assert (out.float() == SENTINEL).all()


# ------------------------------------------------------------------------------------------ row-wise kernels
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("d", [384, 1408, 1664])
def test_rowstats_and_layernorm_at_odd_multiples_of_128(lib, d, M):
    """Against the float64 numpy restatement on the same 16-bit rows, with the bars tests/test_clip_gpu.py applies to the same entry
    points: the canonical one-pass fp16 statistics rtol 2e-5 (test_gemm_with_layernorm_statistics_inside), the two-pass statistics
    (fp16 and bf16 rows) rtol 1e-4 (test_gemm_fp16_residual_stream_hooks_both_kernels), LayerNorm 2e-5 in f32 and 0.02 in the
    16-bit outputs (test_layernorm).  M = 63 / 64 / 65: the two sides of the 64-row workgroup of the one-pass kernel.  d = 384 stands
    for the other odd multiples of 128 the switches instantiate (one whole step and the half step).
    A row holding an fp16 inf: these entry points pass no range flag (the encoder's own calls do: test_clip_gpu's overflow test), so
    what is checked is that no other row moves and that the two-pass scale of the row is not a usable number."""
    from clip_retrieval_amd._lib import check

    eps = 1e-5
    g = torch.Generator().manual_seed(d + M)
    x = torch.randn(M, d, generator=g) * 2.0 + 0.3
    x[:, 7] += 60.0                                 # a 'massive activation' channel in the first wave step
    x[:, d - 3] -= 40.0                             # and one in the half step only lanes 0 .. 31 take
    x[:, 1] += (torch.arange(M) % 113) * 0.02
    for is_f16, kinds in ((True, (2, 1)), (False, (0,))):
        rows = x.to(torch.float16 if is_f16 else torch.bfloat16)
        rows_dev = rows.cuda()
        want = 1.0 / np.sqrt(rows.double().numpy().var(axis=1) + eps)
        for kind in kinds:
            rstd = torch.full((M,), float("nan"), device="cuda")
            check(lib, lib.clipx_rowstats_device(0, _ptr(rows_dev), kind, _ptr(rstd), M, d, C.c_float(eps), None), "clipx")
            torch.cuda.synchronize()
            rel = np.abs(rstd.cpu().double().numpy() - want) / want
            print(f"rowstats d={d} M={M} kind={kind}: max rel err {rel.max():.3g}")
            assert rel.max() <= (2e-5 if kind == 2 else 1e-4), (kind, rel.max())
            if is_f16:  # one row with an inf: its scale is not usable, every other row keeps its bits
                bad = rows.clone()
                bad[M // 2, d - 5] = float("inf")
                r2 = torch.full((M,), float("nan"), device="cuda")
                bad_dev = bad.cuda()
                check(lib, lib.clipx_rowstats_device(0, _ptr(bad_dev), kind, _ptr(r2), M, d, C.c_float(eps), None), "clipx")
                torch.cuda.synchronize()
                if kind == 1:  # (the one-pass form clamps its NaN variance to 0: there the flag is the only witness)
                    v = float(r2[M // 2])
                    assert not (np.isfinite(v) and v > 0.0), v
                keep = torch.arange(M) != M // 2
                assert torch.equal(r2.cpu()[keep].view(torch.int32), rstd.cpu()[keep].view(torch.int32))
    # LayerNorm (f32 rows in; f32, bf16 and fp16 out)
    x32 = (torch.randn(M, d, generator=g) * 3 + 0.7)
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    xd = x32.double().numpy()
    mu, var = xd.mean(axis=1, keepdims=True), xd.var(axis=1, keepdims=True)
    want = (xd - mu) / np.sqrt(var + eps) * gamma.double().numpy() + beta.double().numpy()
    x_dev, gamma_dev, beta_dev = x32.cuda(), gamma.cuda(), beta.cuda()
    for kind, dt, bar in ((0, torch.float32, 2e-5), (1, torch.bfloat16, 0.02), (2, torch.float16, 0.02)):
        y = torch.full((M, d), SENTINEL, dtype=dt, device="cuda")
        check(lib, lib.clipx_layernorm_device(0, _ptr(x_dev), _ptr(gamma_dev), _ptr(beta_dev), _ptr(y), kind, M, d, C.c_float(eps), None), "clipx")
        torch.cuda.synchronize()
        err = np.abs(y.cpu().double().numpy() - want).max()
        print(f"layernorm d={d} M={M} out={kind}: max abs err {err:.3g}")
        assert err < bar, (kind, err)
    # a width that is no multiple of 128 is refused
    assert lib.clipx_rowstats_device(0, _ptr(x_dev), 1, _ptr(rstd), M, d + 64, C.c_float(eps), None) == E_UNSUPPORTED
    assert "128" in lib.clipx_last_error().decode()


# ------------------------------------------------------------------------------------------ GEMMs at the new shapes
@pytest.mark.parametrize("M,N,K", [(2048 + 77, 6144, 1408), (2048 + 77, 8192, 1664), (514, 1408, 6144), (514, 4992, 1664)])
def test_gemm_at_the_new_shapes(lib, M, N, K):
    """test_gemm_epilogues' reference and bar (fp32 matmul of the same bf16-rounded operands; 1e-3 + 4e-3 |want| for the bf16
    outputs, 1e-3 + 1e-4 |want| for the f32 residual), default dispatch: fc1 of the two towers (256x256 kernel, K = 11 / 13 tiles of
    128, 77 rows left to the 128x128 kernel), fc2 and QKV at widths that are no multiple of 256 (128x128 kernel in one launch)."""
    from clip_retrieval_amd._lib import check

    g = torch.Generator(device="cuda").manual_seed(M * 7 + N)
    A = (torch.randn(M, K, generator=g, device="cuda") * 0.5).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g, device="cuda") * 0.05).to(torch.bfloat16)
    A[:, 0] += torch.arange(M, device="cuda").to(torch.bfloat16) * 0.01
    W[:, 1] += torch.arange(N, device="cuda").to(torch.bfloat16) * 0.003
    bias = torch.randn(N, generator=g, device="cuda")
    ref = A.float() @ W.float().T + bias
    for epi in (0, 1, 2, 3):
        if epi == 3:
            out = torch.randn(M, N, generator=g, device="cuda")
            want = out + ref
        else:
            out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
            want = ref if epi == 0 else (ref * torch.sigmoid(1.702 * ref) if epi == 1 else torch.nn.functional.gelu(ref))
        check(lib, lib.clipx_gemm_bf16_device(0, _ptr(A), _ptr(W), _ptr(bias), _ptr(out), M, N, K, epi, None), "clipx")
        torch.cuda.synchronize()
        err = (out.float() - want).abs()
        tol = 1e-3 + (4e-3 * want.abs() if epi != 3 else 1e-4 * want.abs())
        bad = (err > tol).nonzero()
        assert bad.numel() == 0, f"epi={epi} M={M} N={N} K={K}: {bad.shape[0]} bad, first {bad[:4].tolist()} max err {err.max().item():.4g}"


@pytest.mark.parametrize("K", [1408, 1664])
def test_layernorm_folded_gemm_rows_do_not_depend_on_the_kernel(lib, K):
    """clipx_gemm_f16_ln_device at N = 4096: M = 2048 + 77 in one call (eight m-tiles in the 256x256 kernel, which takes the LayerNorm
    sums from its own A fragments; the 77 other rows from the one-pass statistics kernel), then the first 2048 rows again as four
    calls of 512 rows -- too few tiles for the 256x256 kernel, so the 128x128 kernel with every row scale from the statistics pass.
    Every output row must be the same bits: the fused statistics stay ON at K = 1408 / 1664 (the statistics kernel keeps the
    canonical order at 44 and 52 chunks per lane part), and this is the test of it.  Both 16-bit epilogues the encoder uses."""
    from clip_retrieval_amd._lib import check

    M, N, eps = 2048 + 77, 4096, 1e-5
    g = torch.Generator(device="cuda").manual_seed(K)
    Ah = (torch.randn(M, K, generator=g, device="cuda") * 2.0 + 0.3).to(torch.float16)
    Ah[:, 7] += 60.0
    Ah[:, K - 3] -= 40.0
    Ah[:, 1] += (torch.arange(M, device="cuda") % 113).to(torch.float16) * 0.02
    Wh = (torch.randn(N, K, generator=g, device="cuda") * 0.04).to(torch.float16)
    bias = torch.randn(N, generator=g, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    want_r = 1.0 / torch.sqrt(Ah.double().var(dim=1, unbiased=False) + eps)
    ref = (Ah.float() @ Wh.float().T) * want_r.float()[:, None] + bias
    for epi in (7, 2):
        dt = torch.float16 if epi == 7 else torch.bfloat16
        whole = torch.empty(M, N, device="cuda", dtype=dt)
        scratch = torch.full((M,), float("nan"), device="cuda")
        check(lib, lib.clipx_gemm_f16_ln_device(0, _ptr(Ah), _ptr(Wh), _ptr(bias), _ptr(whole), M, N, K, epi, _ptr(scratch), C.c_float(eps),
                                                C.c_void_p(st)), "clipx")
        parts = torch.empty(2048, N, device="cuda", dtype=dt)
        scratch2 = torch.full((2048,), float("nan"), device="cuda")
        for r0 in range(0, 2048, 512):
            check(lib, lib.clipx_gemm_f16_ln_device(0, _ptr(Ah[r0:r0 + 512]), _ptr(Wh), _ptr(bias), _ptr(parts[r0:r0 + 512]), 512, N, K, epi,
                                                    _ptr(scratch2[r0:r0 + 512]), C.c_float(eps), C.c_void_p(st)), "clipx")
        torch.cuda.synchronize()
        assert bool(torch.isnan(scratch[0])) and bool(torch.isnan(scratch[2047])), "the 256x256 kernel took the first 2048 rows, statistics inside"
        assert not torch.isnan(scratch[2048:]).any() and not torch.isnan(scratch2).any()
        bad = (whole[:2048].view(torch.int16) != parts.view(torch.int16)).nonzero()
        assert bad.numel() == 0, f"K={K} epi {epi}: {bad.shape[0]} elements differ, first {bad[:5].tolist()}"
        w = ref if epi == 7 else torch.nn.functional.gelu(ref)
        e = (whole.float() - w).abs()
        t = (3e-4 + 6e-4 * w.abs()) if epi == 7 else (2e-3 + 4e-3 * w.abs())  # test_gemm_with_layernorm_statistics_inside's
        assert (e <= t).all(), f"K={K} epi {epi}: max err {float(e.max()):.4g}"


# ------------------------------------------------------------------------------------------ the encoders
def _oracle_arch(name):
    from oracle.clip_oracle import ClipArch

    if name == "g":
        return ClipArch(v_width=1408, v_heads=16, v_mlp=6144, v_layers=2, t_width=1024, t_heads=16, t_mlp=4096, t_layers=2,
                        embed_dim=1024, act="gelu")
    return ClipArch(v_width=1664, v_heads=16, v_mlp=8192, v_layers=2, t_width=1280, t_heads=20, t_mlp=5120, t_layers=2,
                    embed_dim=1280, act="gelu")


def _product_arch(arch):
    from clip_retrieval_amd.encoder import ClipArch

    return ClipArch(**{k: getattr(arch, k) for k in ClipArch.__dataclass_fields__})


class _Oracle:
    """the plain-torch restatement of the CLIP graph (oracle.clip_oracle.functional_encode_*) over the blob the encoder was given"""

    def __init__(self, blob, arch):
        from oracle.clip_oracle import unpack_blob

        self.W, self.arch = unpack_blob(blob, arch), arch

    def encode_image(self, pix):
        from oracle.clip_oracle import functional_encode_image

        return functional_encode_image(self.W, self.arch, pix)

    def encode_text(self, ids):
        from oracle.clip_oracle import functional_encode_text

        return functional_encode_text(self.W, self.arch, ids)


@pytest.fixture(scope="module", params=["g", "bigG"])
def tiny_wide(request):
    """Two layers per tower, everything else the real shapes of ViT-g/14 / ViT-bigG/14; random_blob weights, seed 0."""
    from clip_retrieval_amd.encoder import ClipEncoder, random_blob

    arch = _oracle_arch(request.param)
    parch = _product_arch(arch)
    blob = random_blob(parch, 0)
    enc = ClipEncoder(parch, blob, 0)
    yield request.param, arch, _Oracle(blob, arch), enc, blob
    enc.close()


@pytest.mark.parametrize("B", [1, 2, 9])
def test_wide_encoder_parity_vs_oracle(tiny_wide, B):
    """B = 1 (graph replay, split-K), 2 (graph replay), 9 (plain launches).  test_encoder_336_parity_vs_oracle's bars, for image and
    text alike: the parity gate (cosine 1 - 1e-4, centred cosine, nearest row), embeddings within 0.02 of the oracle's fp16 rows,
    norms within 2e-3 of 1, the uint8 and float input paths to cosine 1 - 1e-4."""
    from oracle.clip_oracle import mapper_semantics, normalise_u8_nhwc, parity_gate, synth_pixels_u8, synth_tokens

    name, arch, oracle, enc, _ = tiny_wide
    assert arch.v_width // arch.v_heads == (88 if name == "g" else 104) and arch.v_tokens == 257
    u8 = synth_pixels_u8(B, seed=B)
    pix = normalise_u8_nhwc(u8)
    ids = synth_tokens(B, seed=10 + B)
    want_i16, want_i32 = mapper_semantics(oracle.encode_image(torch.from_numpy(pix)))
    want_t16, want_t32 = mapper_semantics(oracle.encode_text(torch.from_numpy(ids)))
    for _ in range(2):  # twice: the second call of a small batch is the one that is captured and replayed
        got_i = enc.encode_image(pix)
        got_t = enc.encode_text(ids)
        assert got_i.dtype == np.float16 and got_i.shape == (B, arch.embed_dim) and got_i.flags["C_CONTIGUOUS"]
        assert got_t.dtype == np.float16 and got_t.shape == (B, arch.embed_dim)
        parity_gate(got_i, want_i32, f"ViT-{name}/14 image")
        parity_gate(got_t, want_t32, f"ViT-{name}/14 text")
        for got, want16 in ((got_i, want_i16), (got_t, want_t16)):
            assert np.allclose(np.linalg.norm(got.astype(np.float32), axis=1), 1, atol=2e-3)
            assert np.abs(got.astype(np.float32) - want16.astype(np.float32)).max() < 0.02
    got_u8 = enc.encode_image(u8)
    assert _cos(got_u8, got_i).min() > 1 - 1e-4


def test_wide_stream_overflow_raises_the_range_flag():
    """The range flag of the row-statistics kernels at width 1408, which the per-kernel entry point does not expose: a two-layer
    ViT-g/14 whose first image block adds 70 000 to column d - 5 of the fp16 residual stream (a column of the half step that only
    lanes 0 .. 31 take) must give ResidualStreamOverflow, as tests/test_clip_gpu.py's overflow test asks of the narrow models --
    B = 1 three times (plain launches, then the replayed graph) and B = 9 (plain launches); the text tower keeps working."""
    from clip_retrieval_amd import ResidualStreamOverflow
    from clip_retrieval_amd.encoder import ClipEncoder, random_blob
    from oracle.clip_oracle import mapper_semantics, normalise_u8_nhwc, parity_gate, synth_pixels_u8, synth_tokens, unpack_blob

    arch = _oracle_arch("g")
    parch = _product_arch(arch)
    blob = random_blob(parch, 0).copy()
    W = unpack_blob(blob, arch)  # views of the blob
    assert np.shares_memory(W["vlayers"][0]["fc2_b"].numpy(), blob)
    W["vlayers"][0]["fc2_b"][arch.v_width - 5] += 70000.0
    enc = ClipEncoder(parch, blob, 0)
    try:
        for B in (1, 9):
            pix, ids = normalise_u8_nhwc(synth_pixels_u8(B, seed=60 + B)), synth_tokens(B, seed=70 + B)
            for _ in range(3):
                with pytest.raises(ResidualStreamOverflow):
                    enc.encode_image(pix)
                enc.encode_text(ids)
        ids = synth_tokens(4, seed=8)
        want = mapper_semantics(_Oracle(blob, arch).encode_text(torch.from_numpy(ids)))[1]
        parity_gate(enc.encode_text(ids), want, "text tower beside an overflowing 1408-wide image tower")
    finally:
        enc.close()


def test_wide_pooled_last_block_equals_the_full_block(tiny_wide):
    """The last image block asks the attention for query block 0 only (q_blocks = 1 of the nine-wave kernel).  Against an encoder with
    the full last block: cosine > 1 - 1e-5 (the existing test's bar) for the single query; batches of two and more give the same
    bytes, as they do for every other model."""
    from clip_retrieval_amd.encoder import ClipEncoder
    from oracle.clip_oracle import normalise_u8_nhwc, synth_pixels_u8, synth_tokens

    name, arch, _, enc, blob = tiny_wide
    os.environ["CLIPX_FULL_LAST_BLOCK"] = "1"
    try:
        full = ClipEncoder(_product_arch(arch), blob, 0)
    finally:
        os.environ.pop("CLIPX_FULL_LAST_BLOCK")
    try:
        assert enc.get_option(enc.OPT_POOL_LAST_BLOCK) == 1 and full.get_option(full.OPT_POOL_LAST_BLOCK) == 0
        for B in (2, 9):
            pix, ids = normalise_u8_nhwc(synth_pixels_u8(B, seed=40 + B)), synth_tokens(B, seed=50 + B)
            a, b = enc.encode_image(pix), full.encode_image(pix)
            assert _cos(a, b.astype(np.float32)).min() > 1 - 1e-5
            assert np.array_equal(a, b), f"ViT-{name}/14 image B={B}"
            assert np.array_equal(enc.encode_text(ids), full.encode_text(ids)), f"ViT-{name}/14 text B={B}"
        pix = normalise_u8_nhwc(synth_pixels_u8(1, seed=3))
        assert _cos(enc.encode_image(pix), full.encode_image(pix).astype(np.float32)).min() > 1 - 1e-5
    finally:
        full.close()


def test_clip_mapper_takes_the_wide_models(tiny_wide):
    """ClipMapper on the two models, the two-layer encoder registered under the model's name (test_clip_mapper_takes_the_336_model):
    a batch of 3 returns float16 [3, 1024] (ViT-g/14) / [3, 1280] (ViT-bigG/14) for both towers."""
    from clip_retrieval_amd.encoder import ARCHS, register_encoder, resolve_arch_name
    from clip_retrieval_amd.mapper import ClipMapper
    from oracle.clip_oracle import mapper_semantics, normalise_u8_nhwc, parity_gate, synth_pixels_u8, synth_tokens

    short, arch, oracle, enc, _ = tiny_wide
    name = resolve_arch_name("open_clip:ViT-g-14/laion2b_s12b_b42k" if short == "g" else "open_clip:ViT-bigG-14/laion2b_s39b_b160k")
    full = ARCHS[name]
    assert (full.v_width, full.v_heads, full.v_mlp, full.embed_dim) == (arch.v_width, arch.v_heads, arch.v_mlp, arch.embed_dim)
    register_encoder(name, enc)
    mapper = ClipMapper(enable_image=True, enable_text=True, enable_metadata=False, use_mclip=False,
                        clip_model="registered:" + name, use_jit=True, mclip_model="", warmup_batch_size=1)
    pix = torch.from_numpy(normalise_u8_nhwc(synth_pixels_u8(3, seed=23)))
    ids = torch.from_numpy(synth_tokens(3, seed=33)).long()
    out = mapper({"image_tensor": pix, "text_tokens": ids, "image_filename": ["0.jpg", "1.jpg", "2.jpg"], "text": ["a", "b", "c"]})
    E = 1024 if short == "g" else 1280
    assert out["image_embs"].shape == (3, E) and out["image_embs"].dtype == np.float16
    assert out["text_embs"].shape == (3, E) and out["text_embs"].dtype == np.float16
    parity_gate(out["image_embs"], mapper_semantics(oracle.encode_image(pix))[1], f"ViT-{short}/14 mapper image")
    parity_gate(out["text_embs"], mapper_semantics(oracle.encode_text(ids))[1], f"ViT-{short}/14 mapper text")
