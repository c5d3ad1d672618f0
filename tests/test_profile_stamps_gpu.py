"""The stamp form of the GEMM brackets: every kernel launch_gemm can issue writes its own first start and last end into
a slot of the profiler, and clipx_profile_get sums last_end - first_start over the kernels of a scope.

One GEMM per launch site, on the smallest shapes whose plan (csrc/clipx_gemm_plan.h) names each kernel, through the test entry
clipx_profile_gemm_device; the split-K pair through a B = 1 text query of the encoder.  The reference for a stamp time is a pair of
marker events recorded around the same call: a span that contains the kernels.  The floor is the one bench.py uses: no GEMM runs
faster than 2.5 PFLOP/s."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
KIND_GEMM, PROF_GEMM = 0, 2
EPI_BIAS_BF16, EPI_TABLE_F32, EPI_BIAS_RESID_H16, EPI_BIAS_F16 = 0, 4, 6, 7
PEAK_FLOPS = 2.5e15
CHUNK_SLOTS = 8192  # csrc/clipx_host.h PROF_CHUNK_SLOTS

# name -> (M, N, K, epilogue, fp16 operands): the kernels each plan names are in the comments
CASES = {
    "w4": (8192, 1024, 1024, EPI_BIAS_F16, True),             # 4-wave 256x256
    "w8": (8192, 1024, 640, EPI_TABLE_F32, False),            # 8-wave 256x256 (the 4-wave kernel has no f32-table epilogue)
    "w4+128": (8224, 1024, 1024, EPI_BIAS_RESID_H16, False),  # 4-wave + a 128x128 launch for the 32 leftover rows: two kernels, one scope
    "128": (300, 768, 768, EPI_BIAS_BF16, False),             # 128x128 only
}


@pytest.fixture(scope="module")
def enc():
    from clip_retrieval_amd.encoder import get_encoder

    e = get_encoder("random:ViT-B/32")
    e.set_option(e.OPT_PROF_MARKERS, 0)
    yield e
    e.profile(0)
    try:
        e.profile_get(KIND_GEMM)
    except Exception:  # pylint: disable=broad-except
        pass


@pytest.fixture(scope="module")
def operands():
    """Per case, made once and never written: A, W (16-bit), bias, row scales, table and the initial contents of the output."""
    out = {}
    g = torch.Generator(device="cuda").manual_seed(7)
    for name, (M, N, K, epi, f16) in CASES.items():
        dt = torch.float16 if f16 else torch.bfloat16
        o = {"A": (torch.randn(M, K, device="cuda", generator=g) * 0.5).to(dt), "W": (torch.randn(N, K, device="cuda", generator=g) * 0.05).to(dt),
             "bias": torch.randn(N, device="cuda", generator=g), "ones": torch.ones(M, device="cuda"),
             "table": torch.randn(50, N, device="cuda", generator=g)}
        if epi == EPI_TABLE_F32:
            o["out0"] = torch.zeros(M, N, device="cuda")
        elif epi == EPI_BIAS_RESID_H16:
            o["out0"] = torch.randn(M, N, device="cuda", generator=g).to(torch.float16)
        else:
            o["out0"] = torch.zeros(M, N, device="cuda", dtype=torch.float16)  # 16-bit outputs: the bits are what is compared
        out[name] = o
    torch.cuda.synchronize()
    return out


def _fresh_out(name, ops):
    out = ops[name]["out0"].clone()  # (the residual epilogue works in place)
    torch.cuda.synchronize()
    return out


def _gemm(enc, name, ops, out=None):
    """One call of case `name` on the null stream (torch's current stream here) into `out` -> the output tensor."""
    M, N, K, epi, f16 = CASES[name]
    o = ops[name]
    out = _fresh_out(name, ops) if out is None else out
    enc.profile_gemm(o["A"].data_ptr(), o["W"].data_ptr(), o["bias"].data_ptr(), out.data_ptr(), M, N, K, epi, f16=f16,
                     rowscale=o["ones"].data_ptr(), table=o["table"].data_ptr() if epi == EPI_TABLE_F32 else None, T=50)
    return out


def _bytes(t):
    return t.cpu().contiguous().view(torch.uint8).numpy()


def _query_ids(enc):
    from oracle.clip_oracle import synth_tokens

    return synth_tokens(1, enc.arch.ctx_len, enc.arch.vocab, seed=5)


@pytest.fixture(scope="module")
def plain(enc, operands):
    """Every case with profiling off (also the warm-up of every kernel): the outputs the profiled calls must reproduce."""
    enc.profile(0)
    ref = {name: _bytes(_gemm(enc, name, operands)) for name in CASES}
    ref["query"] = enc.encode_text(_query_ids(enc)).copy()
    torch.cuda.synchronize()
    return ref


def _profiled(enc, run):
    """run() under the stamp form between two marker events -> (launches, stamp ms, flops, marker ms, what run returned)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    enc.profile(PROF_GEMM)
    try:
        a.record()
        got = run()
        b.record()
    finally:
        enc.profile(0)
    n, ms, fl = enc.profile_get(KIND_GEMM)  # synchronises the stream; fails if first_start > last_end or a slot is unwritten
    b.synchronize()
    return n, ms, fl, a.elapsed_time(b), got


@pytest.mark.parametrize("name", list(CASES))
def test_every_family_stamps_and_null_is_the_old_kernel(enc, operands, plain, name):
    M, N, K, _, _ = CASES[name]
    out = _fresh_out(name, operands)  # made outside the marker pair: between the two events lies the GEMM call and nothing else
    n, ms, fl, marker_ms, _ = _profiled(enc, lambda: _gemm(enc, name, operands, out))
    floor_ms = 2.0 * M * N * K / PEAK_FLOPS * 1e3
    print(f"{name}: stamps {ms:.4f} ms, markers {marker_ms:.4f} ms, floor {floor_ms:.4f} ms")
    assert (n, fl) == (1, 2.0 * M * N * K)
    assert floor_ms < ms <= marker_ms
    assert np.array_equal(_bytes(out), plain[name]), "profiling changed the output"


def test_split_k_pair_stamps(enc, plain):
    """A B = 1 text query: every GEMM of the tower is the split-K kernel plus its reduction (48 scopes of two kernels; that these
    shapes plan onto split-K is asserted on the CPU, tests/test_stamp_slots_cpu.py).  The marker pair around the call also holds
    the attention, the embedding, the tail and the copy back, so the bound that bites is the library's own marker form of the same
    query: a marker pair around every GEMM scope, the two kernels of the scope and the gaps around them."""
    ids = _query_ids(enc)
    n, ms, fl, around_ms, out = _profiled(enc, lambda: enc.encode_text(ids))
    enc.set_option(enc.OPT_PROF_MARKERS, 1)
    try:
        marker = [_profiled(enc, lambda: enc.encode_text(ids))[1] for _ in range(3)]
    finally:
        enc.set_option(enc.OPT_PROF_MARKERS, 0)
    floor_ms = fl / PEAK_FLOPS * 1e3
    print(f"query: {n} scopes, stamps {ms:.4f} ms, marker form {[round(v, 4) for v in marker]} ms, pair around the call {around_ms:.4f} ms, floor {floor_ms:.5f} ms")
    assert n == 4 * enc.arch.t_layers and fl > 0
    assert floor_ms < ms <= min(marker) and ms <= around_ms
    assert np.array_equal(out.view(np.uint16), plain["query"].view(np.uint16)), "profiling changed the embedding"


def test_slots_recycle(enc):
    """More GEMM kernels than a chunk has slots without a clipx_profile_get in between: the second chunk is allocated.  After the
    read both chunks are free again, and crossing the boundary a second time allocates nothing."""
    from oracle.clip_oracle import synth_pixels_u8, synth_tokens

    B = 32
    pix, ids = synth_pixels_u8(B, size=enc.arch.image_size, seed=3), synth_tokens(B, enc.arch.ctx_len, enc.arch.vocab, seed=4)

    def steps(k):
        enc.profile(PROF_GEMM)
        try:
            for _ in range(k):
                enc.encode_image(pix)
                enc.encode_text(ids)
        finally:
            enc.profile(0)
        return enc.profile_get(KIND_GEMM)

    n1, ms1, fl1 = steps(1)
    assert n1 == 1 + 4 * enc.arch.v_layers + 4 * enc.arch.t_layers and ms1 > 0.0
    k = CHUNK_SLOTS // n1 + 1  # every scope takes at least one slot: more than a chunk of them
    free = []
    for _ in range(2):
        n, ms, fl = steps(k)
        assert n == k * n1 and fl == pytest.approx(k * fl1, rel=1e-12) and ms > 0.0
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert free[1] >= free[0], f"the profiler's device memory grew on the second crossing: free {free[0]} -> {free[1]} bytes"


def test_a_refused_launch_is_an_error_and_is_consumed(enc, operands, plain):
    """fp16 operands with the residual epilogue: no plan, launch_gemm refuses before any kernel runs.  The scope has no stamped
    kernel: clipx_profile_get says so (CLIPX_E_STATE), consumes it, and the next profiled call is read as usual."""
    from clip_retrieval_amd._lib import HipLibraryError

    o = operands["128"]
    M, N, K, _, _ = CASES["128"]
    out = o["out0"].clone()
    enc.profile(PROF_GEMM)
    try:
        with pytest.raises(HipLibraryError):
            enc.profile_gemm(o["A"].data_ptr(), o["W"].data_ptr(), o["bias"].data_ptr(), out.data_ptr(), M, N, K, EPI_BIAS_RESID_H16, f16=True,
                             rowscale=o["ones"].data_ptr())
        good = _gemm(enc, "128", operands)  # a good scope behind the starved one: consumed with it
    finally:
        enc.profile(0)
    with pytest.raises(HipLibraryError, match=r"code -4"):
        enc.profile_get(KIND_GEMM)
    assert np.array_equal(_bytes(good), plain["128"])
    n, ms, fl, _, out = _profiled(enc, lambda: _gemm(enc, "128", operands))
    assert (n, fl) == (1, 2.0 * M * N * K) and ms > 0.0
    assert np.array_equal(_bytes(out), plain["128"])
