"""Adversarial inputs, the float64 reference and the error bound of the attention kernel tests (test_attention_edges_cpu.py
tests them without a GPU, test_attention_edges_gpu.py runs the kernels on them).  A plain module, imported by both.

Layout everywhere: qkv is IEEE fp16 [rows, 3 * H * dh] = q | k | v, head h in columns h * dh .. of each third; a rectangular batch
has rows = B * T (sample b owns rows b * T ..), a ragged one packs the samples' rows one after the other.  The kernels' output is
[rows, H * dh]."""
import math

import torch

FAMILIES = ("sharp", "neg", "last_heavy", "ramp", "onehot")  # ramp: causal only
T_SHORT_MAX, T_LONG_MAX = 288, 608


def kernel_of(T, dh, causal):
    """Which kernel a (T, dh, causal) runs (csrc/clipx_attn_plan.h): 'block' attention_kernel, 'persistent' attention_pk_kernel,
    'long' attention_long_kernel, None where the launch is refused."""
    nkb = (T + 31) // 32
    if T < 1 or T > T_LONG_MAX or dh not in (64, 80):
        return None
    if T > T_SHORT_MAX:
        return "long" if dh == 64 and not causal else None
    if dh == 80:
        return "block" if nkb <= 3 or nkb == 9 else None
    return "persistent" if nkb == 9 and not causal else "block"


def split(qkv, B, T, H, dh):
    """[B * T, 3 H dh] -> q, k, v as [B, H, T, dh] views"""
    q, k, v = qkv.view(B, T, 3, H, dh).permute(2, 0, 3, 1, 4)
    return q, k, v


def join(q, k, v):
    """q, k, v [B, T, H, dh] float -> fp16 [B * T, 3 H dh]"""
    B, T, H, dh = q.shape
    return torch.stack([q, k, v], 2).reshape(B * T, 3 * H * dh).to(torch.float16).contiguous()


def unit(dh):
    """u: a fixed vector of +-1"""
    g = torch.Generator().manual_seed(8191)
    return torch.where(torch.rand(dh, generator=g) < 0.5, -1.0, 1.0)


# ------------------------------------------------------------------------------------------ reference and bound
def reference(qkv, B, T, H, dh, causal, lens=None):
    """softmax(q k^T / sqrt(dh) [+ causal mask]) in float64 on the same fp16 inputs: returns want = P v and pav = P |v|, both
    float64 [rows, H dh].  lens (a list of B lengths): the rows are packed, sample b has lens[b] of them, T is ignored."""
    if lens is not None:
        outs, row = [], 0
        for n in lens:
            outs.append(reference(qkv[row:row + n], 1, n, H, dh, causal))
            row += n
        return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    q, k, v = split(qkv.double(), B, T, H, dh)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    if causal:
        s = s.masked_fill(torch.ones(T, T, dtype=torch.bool, device=qkv.device).triu_(1), float("-inf"))
    p = torch.softmax(s, -1)
    back = lambda o: o.permute(0, 2, 1, 3).reshape(B * T, H * dh)
    return back(p @ v), back(p @ v.abs())


def bound(want, pav, T, vmax):
    """The per-element error bound E of an attention output, from the arithmetic include/clipx.h documents (fp16 operands, fp32
    scores and softmax, P rounded to fp16, fp32 accumulation, bf16 output), not from any kernel:

        E = 2^-8 |want| + 2^-10 pav + T 2^-24 vmax + 1e-6

    2^-8 |want|     the bf16 rounding of the output: half an ulp of an 8-bit significand is at most 2^-8 of the value;
    2^-10 pav       every P is rounded to fp16, a relative 2^-11, so the sum over keys of |dP v| is at most 2^-11 P |v| = 2^-11
                    pav; doubled for the hardware exp2 (an ulp of fp32) and the order of the fp32 sums, both far smaller;
    T 2^-24 vmax    a P below the fp16 subnormal spacing loses up to 2^-25 absolutely (it may round to 0): T keys of at most
                    vmax, doubled as above;
    1e-6            an absolute floor for elements that cancel to (nearly) nothing.
    want, pav: reference(); T: keys of the (longest) sample; vmax: max |v| of the input."""
    return want.abs() * 2.0 ** -8 + pav * 2.0 ** -10 + T * 2.0 ** -24 * vmax + 1e-6


def vmax_of(qkv, H, dh):
    return qkv[:, 2 * H * dh:].abs().max().item()


def worst(out, want, pav, T, vmax):
    """max over the elements of |out - want| / E; inf where the output is not finite"""
    out = out.double()
    if not torch.isfinite(out).all():
        return float("inf")
    return ((out - want).abs() / bound(want, pav, T, vmax)).max().item()


# ------------------------------------------------------------------------------------------ the input families
def _gen(B, T, H, dh, seed):
    return torch.Generator().manual_seed(1_000_003 * seed + 7919 * T + 131 * H + dh + 17 * B)


def sharp(B, T, H, dh, seed, causal=0):
    """test_attention's inputs: randn, q scaled by 2."""
    g = _gen(B, T, H, dh, seed)
    q, k, v = (torch.randn(B, T, H, dh, generator=g) for _ in range(3))
    return join(2.0 * q, k, v)


def neg(B, T, H, dh, seed, causal=0):
    """q = u + 0.25 randn, k = -u + 0.25 randn: every real logit is about -sqrt(dh) (-8 or -8.9, spread about 0.4), so a key that
    was zeroed instead of masked (logit 0) takes nearly all the weight of its row, in whichever block it sits."""
    g = _gen(B, T, H, dh, seed)
    u = unit(dh)
    q = u + 0.25 * torch.randn(B, T, H, dh, generator=g)
    k = -u + 0.25 * torch.randn(B, T, H, dh, generator=g)
    return join(q, k, torch.randn(B, T, H, dh, generator=g))


def last_heavy(B, T, H, dh, seed, causal=0):
    """q = 0: a uniform softmax over the keys a row sees; v[T - 1] = 64 in every column.  The staging paths clamp rows past T to
    row T - 1: if such a copy is not masked, the last row's share doubles."""
    g = _gen(B, T, H, dh, seed)
    k, v = torch.randn(B, T, H, dh, generator=g), torch.randn(B, T, H, dh, generator=g)
    v[:, T - 1] = 64.0
    return join(torch.zeros(B, T, H, dh), k, v)


RAMP_STEP = 1.0 / 16  # exact in fp16 up to j = 2048


def ramp(B, T, H, dh, seed, causal=1):
    """Causal only.  q = u, k_j = (c j / T) u with c = T / 16, i.e. k_j = j / 16 u exactly in fp16: the logit grows by sqrt(dh) / 16
    (0.5 at dh 64, 0.56 at dh 80) per key, so a row's own key holds 0.39 (0.43) of its weight and the next key, were it to leak,
    would hold 1.65 (1.75) times that."""
    assert causal, "ramp is a causal family"
    g = _gen(B, T, H, dh, seed)
    u = unit(dh)
    q = u.expand(B, T, H, dh)
    k = (torch.arange(T, dtype=torch.float32) * RAMP_STEP).view(1, T, 1, 1) * u
    return join(q, k.expand(B, T, H, dh), torch.randn(B, T, H, dh, generator=g))


def onehot_targets(T, causal):
    i = torch.arange(T)
    return (7 * i + 3) % (i + 1) if causal else (7 * i + 3) % T


def onehot(B, T, H, dh, seed, causal=0):
    """k_j = random rows of +-1, q_i = 4 k_t(i), t(i) = (7 i + 3) mod T (causal: mod (i + 1)): the logit of key t(i) is 4 sqrt(dh)
    = 32 (35.8), every other key's is 4 / sqrt(dh) times a sum of dh signs (spread 4), so the softmax is one-hot to fp16 and the
    output row is v_t(i): the key index -> V row permutation of the PV product, in every block."""
    g = _gen(B, T, H, dh, seed)
    k = torch.where(torch.rand(B, T, H, dh, generator=g) < 0.5, -1.0, 1.0)
    q = 4.0 * k[:, onehot_targets(T, causal)]
    return join(q, k, torch.randn(B, T, H, dh, generator=g))


def onehot_want(qkv, B, T, H, dh, causal):
    """v_t(i) for every row, [B T, H dh] float64"""
    _, _, v = split(qkv.double(), B, T, H, dh)
    return v[:, :, onehot_targets(T, causal).to(qkv.device)].permute(0, 2, 1, 3).reshape(B * T, H * dh)


MAKE = {"sharp": sharp, "neg": neg, "last_heavy": last_heavy, "ramp": ramp, "onehot": onehot}


def families(causal):
    return [f for f in FAMILIES if causal or f != "ramp"]


def poison(family, T, H, dh, seed, causal=0):
    """B = 3: the middle sample is `family`'s, its two neighbours hold q, k = +-60 and v alternating NaN and 60000.  Returns
    (the batch of three, the middle sample alone).  What lies beyond a sample must not reach it: the middle sample's output bits
    are those of its launch alone."""
    mid = MAKE[family](1, T, H, dh, seed, causal)
    n = 3 * H * dh
    sign = torch.where(torch.arange(T * n) % 3 == 0, -60.0, 60.0).view(T, n)
    bad = sign.clone()
    alt = torch.where(torch.arange(T * H * dh) % 2 == 0, float("nan"), 60000.0).view(T, H * dh)
    bad[:, 2 * H * dh:] = alt
    bad = bad.to(torch.float16)
    return torch.cat([bad, mid, bad]).contiguous(), mid


def ragged(family, lens, H, dh, seed, causal=0):
    """The samples of a ragged batch packed one after the other: sample i is family(1, lens[i], ...) with its own seed."""
    return torch.cat([MAKE[family](1, n, H, dh, seed + 101 * i, causal) for i, n in enumerate(lens)]).contiguous()
