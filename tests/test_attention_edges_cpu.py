"""The attention edge tests, tested without a GPU: an fp32 emulation of the arithmetic include/clipx.h documents (fp32 scores, P
rounded to fp16, the row sum taken over the unrounded p, bf16 output) stays under the bound E of tests/attention_cases.py for
every input family, and the same emulation with a planted defect -- one padding key zeroed but not masked, or the clamped copy of
the last key not masked -- exceeds E several times over under the family that names that defect.  So a kernel that passes
test_attention_edges_gpu.py does not have those defects, and a correct kernel is not asked for more than its number formats give."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as ac  # noqa: E402

TS = (1, 31, 32, 33, 77, 128, 197, 257, 260, 261, 288)
B, H = 2, 2


def emulate(qkv, B, T, H, dh, causal, defect=None):
    """The documented arithmetic in fp32 torch.  defect 'zero_key': one more key with k = 0, v = 0 that every row sees (a padding
    key of the last block that was zeroed and not masked); 'dup_last': one more copy of key T - 1 that every row sees (the clamped
    staging row, not masked)."""
    q, k, v = (x.float() for x in ac.split(qkv, B, T, H, dh))
    if defect == "zero_key":
        k = torch.cat([k, torch.zeros_like(k[:, :, :1])], 2)
        v = torch.cat([v, torch.zeros_like(v[:, :, :1])], 2)
    elif defect == "dup_last":
        k, v = torch.cat([k, k[:, :, -1:]], 2), torch.cat([v, v[:, :, -1:]], 2)
    s = q @ k.transpose(-1, -2)
    if causal:
        mask = torch.ones(T, T, dtype=torch.bool).triu_(1)
        s[..., :T] = s[..., :T].masked_fill(mask, float("-inf"))
    c = torch.tensor((1.0 / math.sqrt(dh)) * 1.4426950408889634, dtype=torch.float32)
    m = s.max(-1, keepdim=True).values
    p = torch.exp2(s * c - m * c)
    total = p.sum(-1, keepdim=True)
    o = (p.to(torch.float16).float() @ v) / total
    return o.to(torch.bfloat16).permute(0, 2, 1, 3).reshape(B * T, H * dh)


@pytest.fixture(scope="module")
def table():
    """(family, T, dh, causal) -> (qkv, want, pav, vmax): every reference is computed once"""
    out = {}
    for dh in (64, 80):
        for causal in (0, 1):
            for fam in ac.families(causal):
                for T in TS:
                    qkv = ac.MAKE[fam](B, T, H, dh, 3, causal)
                    want, pav = ac.reference(qkv, B, T, H, dh, causal)
                    out[fam, T, dh, causal] = (qkv, want, pav, ac.vmax_of(qkv, H, dh))
    return out


def _ratio(table, fam, T, dh, causal, defect=None):
    qkv, want, pav, vmax = table[fam, T, dh, causal]
    return ac.worst(emulate(qkv, B, T, H, dh, causal, defect), want, pav, T, vmax)


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("dh", [64, 80])
def test_emulation_stays_under_the_bound(table, dh, causal):
    worst = {}
    for fam in ac.families(causal):
        worst[fam] = max(_ratio(table, fam, T, dh, causal) for T in TS)
    print(f"dh={dh} causal={causal}: max err/E " + " ".join(f"{f}={r:.3f}" for f, r in worst.items()))
    assert all(r <= 1.0 for r in worst.values()), worst


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("dh", [64, 80])
def test_neg_sees_one_unmasked_zeroed_key(table, dh, causal):
    ratios = {T: _ratio(table, "neg", T, dh, causal, "zero_key") for T in TS}
    print(f"dh={dh} causal={causal}: zeroed key under neg, err/E " + " ".join(f"{T}:{r:.0f}" for T, r in ratios.items()))
    assert all(r >= 5.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("dh", [64, 80])
def test_last_heavy_sees_an_unmasked_copy_of_the_last_key(table, dh, causal):
    """T = 1 is left out: there the copy is a copy of the only key, the softmax over {v0, v0} is v0, and no test can see it."""
    ratios = {T: _ratio(table, "last_heavy", T, dh, causal, "dup_last") for T in TS if T > 1}
    print(f"dh={dh} causal={causal}: copied last key under last_heavy, err/E " + " ".join(f"{T}:{r:.0f}" for T, r in ratios.items()))
    assert all(r >= 5.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("dh", [64, 80])
def test_the_families_are_what_they_claim(table, dh, causal):
    """neg: every real logit below -5; ramp: the logit grows by >= 0.5 per key and a leaked next key would change a row grossly;
    onehot: the reference row is v_t(i) to 1e-4 of max |v|, and the targets visit every key block."""
    for T in TS:
        qkv = table["neg", T, dh, causal][0]
        q, k, _ = ac.split(qkv.double(), B, T, H, dh)
        assert ((q @ k.transpose(-1, -2)) / math.sqrt(dh)).max() < -5.0
        qkv, want, _, vmax = table["onehot", T, dh, causal]
        assert (want - ac.onehot_want(qkv, B, T, H, dh, causal)).abs().max() < 1e-4 * vmax
        if not causal:
            assert set((ac.onehot_targets(T, 0) // 32).tolist()) == set(range((T + 31) // 32))
        if causal and T > 1:
            qkv = table["ramp", T, dh, causal][0]
            q, k, _ = ac.split(qkv.double(), B, T, H, dh)
            s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
            assert (s[..., 1:] - s[..., :-1]).min() >= 0.5


def test_kernel_of_matches_the_dispatch_table():
    """attention_cases.kernel_of restates csrc/clipx_attn_plan.h for the tests' bookkeeping; the refusals it names are the ones the
    entry points make without a device."""
    import ctypes as C

    from clip_retrieval_amd import load_library

    lib = load_library()
    fake = C.c_void_p(4096)
    for dh in (64, 80):
        for causal in (0, 1):
            for T in (97, 256, 289, 608, 609):
                if ac.kernel_of(T, dh, causal) is None:
                    assert lib.clipx_attention_ex_device(0, fake, fake, 1, T, 1, dh, causal, 0, None, None, None) == -5, (T, dh, causal)
    assert ac.kernel_of(257, 64, 0) == "persistent" and ac.kernel_of(257, 64, 1) == "block" and ac.kernel_of(288, 80, 0) == "block"
    assert ac.kernel_of(289, 64, 0) == "long" and ac.kernel_of(96, 80, 1) == "block" and ac.kernel_of(256, 64, 0) == "block"


def test_new_entry_point_refuses_before_any_launch():
    """The refusals of clipx_attention_ex_device are made before the device is touched (the pointers are never read)."""
    import ctypes as C

    from clip_retrieval_amd import load_library

    lib = load_library()
    fake = C.c_void_p(4096)
    E_ARG, E_UNSUPPORTED = -1, -5

    def call(T, dh, causal, q_blocks=0, offs=None, lens=None, B=1):
        return lib.clipx_attention_ex_device(0, fake, fake, B, T, 1, dh, causal, q_blocks, offs, lens, None), lib.clipx_last_error().decode()

    for T, dh, causal, word in ((609, 64, 0, "608"), (300, 64, 1, "288"), (577, 80, 0, "288"), (700, 80, 1, "608")):
        rc, msg = call(T, dh, causal)
        assert rc == E_UNSUPPORTED and word in msg
    assert call(77, 64, 1, offs=fake)[0] == E_ARG and call(77, 64, 1, lens=fake)[0] == E_ARG
    rc, msg = call(77, 80, 0, offs=fake, lens=fake)
    assert rc == E_UNSUPPORTED and "ragged" in msg
    rc, msg = call(129, 64, 0, offs=fake, lens=fake)
    assert rc == E_UNSUPPORTED and "128" in msg
    for T in (97, 256):
        rc, msg = call(T, 80, 0)
        assert rc == E_UNSUPPORTED and "97" in msg and "256" in msg
    assert call(77, 72, 0)[0] == E_UNSUPPORTED
    assert call(77, 64, 0, q_blocks=-1)[0] == E_ARG and call(0, 64, 0)[0] == E_ARG and call(77, 64, 0, B=0)[0] == E_ARG
