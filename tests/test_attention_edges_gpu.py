"""Every attention kernel at its edges, on the GPU: each instantiation launch_attention holds, at sequence lengths on both sides of
every block boundary and of the short-tail shortcut, on inputs built so that the defect a kernel of this shape can have -- a padding
key not masked, a clamped row counted twice, a future key leaking, a permuted V row, a neighbour's data reaching a sample, a wrong
buffer in the persistent kernel's walk -- is a gross error, against a float64 reference and the element-wise bound E of
tests/attention_cases.py (tests/test_attention_edges_cpu.py shows that E separates a correct kernel from those defects).

Largest |out - want| / E measured on an MI355X, per kernel and family (E is never scaled; a case passes at <= 1):
    block       sharp 0.813  neg 0.810  last_heavy 0.794  ramp 0.797  onehot 0.797   (attention_kernel, ragged launches included)
    persistent  sharp 0.787  neg 0.554  last_heavy 0.323  onehot 0.791               (attention_pk_kernel)
    long        neg 0.380  last_heavy 0.308                                          (attention_long_kernel)
The module prints this table again at the end of a run with -s.

What the file found when it was written: a ragged batch that is not causal was wrong wherever a sample was shorter than the launch's
key blocks minus one (105 E at length 33 of 4 blocks): attention_kernel masked key >= T in the last key block only, and the zeroed K
rows of a short sample's earlier blocks sat in its softmax at logit 0.  The encoder's own ragged batches are causal, where every
block is masked, so no embedding was affected; such launches now run a form of the kernel that masks every block."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as ac  # noqa: E402

pytestmark = pytest.mark.gpu
E_ARG, E_UNSUPPORTED = -1, -5
B, H = 3, 2
SENTINEL = 7.0
WORST = {}  # (kernel, family) -> largest err / E seen in this session


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture(scope="module")
def lib():
    import clip_retrieval_amd

    yield clip_retrieval_amd.load_library()
    for (kern, fam), r in sorted(WORST.items()):
        print(f"\nmax err/E  {kern:10s} {fam:10s} {r:.3f}", end="")
    print()


def launch(lib, qkv, out, B, T, H, dh, causal, q_blocks=0, offs=None, lens=None):
    rc = lib.clipx_attention_ex_device(0, _ptr(qkv), _ptr(out), B, T, H, dh, causal, q_blocks, _ptr(offs), _ptr(lens), None)
    torch.cuda.synchronize()
    return rc


def run(lib, qkv, B, T, H, dh, causal, q_blocks=0, rows=None):
    """a checked launch into a fresh buffer (filled with the sentinel, so that a row nobody wrote shows)"""
    out = torch.full((B * T if rows is None else rows, H * dh), SENTINEL, dtype=torch.bfloat16, device="cuda")
    rc = launch(lib, qkv, out, B, T, H, dh, causal, q_blocks)
    assert rc == 0, lib.clipx_last_error().decode()
    return out


def bits(t):
    return t.contiguous().view(torch.int16)


def note(kern, fam, ratio, what):
    print(f"EDGE {kern} {fam} {what}: err/E {ratio:.3f}")
    WORST[kern, fam] = max(WORST.get((kern, fam), 0.0), ratio)


def check_family(lib, fam, B, T, H, dh, causal, seed=1):
    """one launch of `fam` against the float64 reference: the worst err / E, and for onehot the rows themselves"""
    qkv = ac.MAKE[fam](B, T, H, dh, seed, causal).cuda()
    out = run(lib, qkv, B, T, H, dh, causal)
    want, pav = ac.reference(qkv, B, T, H, dh, causal)
    vmax = ac.vmax_of(qkv, H, dh)
    ratio = ac.worst(out, want, pav, T, vmax)
    if fam == "onehot" and ratio <= 1.0:
        # the row is v_t(i) to the bf16 rounding; what the reference itself keeps of the other keys (below 1e-4 vmax, the CPU
        # test) is allowed on top, with E's absolute terms
        vt = ac.onehot_want(qkv, B, T, H, dh, causal)
        slack = vt.abs() * 2.0 ** -8 + (want - vt).abs() + T * 2.0 ** -24 * vmax + 1e-6
        if not ((out.double() - vt).abs() <= slack).all():
            ratio = float("inf")
    return ratio


# ------------------------------------------------------------------------------------------ 1. every instantiation at its edges
T64_BLOCK = (1, 2, 4, 5, 31, 32, 33, 36, 37, 64, 65, 96, 97, 100, 101, 128, 129, 160, 161, 192, 193, 224, 225, 256)
T64_NINE = (257, 258, 260, 261, 264, 272, 287, 288)  # not causal: attention_pk_kernel; causal: attention_kernel<64, 9, 3, 3>
T80 = (1, 4, 5, 32, 33, 64, 65, 77, 96, 257, 260, 261, 288)
CASES = [(64, T) for T in T64_BLOCK + T64_NINE] + [(80, T) for T in T80]


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("dh,T", CASES)
def test_every_instantiation_at_its_edges(lib, dh, T, causal):
    """B = 3, H = 2.  The lengths: 32 k (no padding in the last block), 32 k + 1 (one real key in it), 32 k + 4 and 32 k + 5 (the two
    sides of the shortcut that skips 12 of the last block's 16 exponentials), 31 / 287 (one padding key), and 1, 2."""
    kern = ac.kernel_of(T, dh, causal)
    assert kern == ("persistent" if (dh == 64 and T > 256 and not causal) else "block")
    bad = {}
    for fam in ac.families(causal):
        ratio = check_family(lib, fam, B, T, H, dh, causal)
        note(kern, fam, ratio, f"dh={dh} T={T} causal={causal}")
        if not ratio <= 1.0:
            bad[fam] = ratio
    assert not bad, f"dh={dh} T={T} causal={causal}: |out - want| exceeds E: {bad}"


@pytest.mark.parametrize("T", [97, 256])
def test_dh80_has_no_kernel_between_97_and_256(lib, T):
    qkv = torch.zeros(T, 3 * 80, dtype=torch.float16, device="cuda")
    out = torch.full((T, 80), SENTINEL, dtype=torch.bfloat16, device="cuda")
    for causal in (0, 1):
        assert launch(lib, qkv, out, 1, T, 1, 80, causal) == E_UNSUPPORTED
        assert "80" in lib.clipx_last_error().decode()
        assert lib.clipx_attention_dh_device(0, _ptr(qkv), _ptr(out), 1, T, 1, 80, causal, None) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out.float() == SENTINEL).all()


# ------------------------------------------------------------------------------------------ 2. the long kernel
T_LONG = (289, 292, 293, 320, 321, 576, 577, 580, 581, 608)


def check_poison(lib, fam, T, dh, causal):
    """the middle sample of the poisoned batch of three has the bits of its launch alone, and they are finite"""
    three, mid = ac.poison(fam, T, H, dh, 2, causal)
    alone = run(lib, mid.cuda(), 1, T, H, dh, causal)
    got = run(lib, three.cuda(), 3, T, H, dh, causal)[T:2 * T]
    assert torch.isfinite(alone.float()).all(), "the sample alone is not finite"
    assert torch.equal(bits(got), bits(alone)), (
        f"{fam} dh={dh} T={T} causal={causal}: {int((bits(got) != bits(alone)).sum())} elements of the middle sample depend on its neighbours")


@pytest.mark.parametrize("T", T_LONG)
def test_long_kernel_masking_and_isolation(lib, T):
    """attention_long_kernel (dh 64, not causal) on the families test_long_seq_gpu.py does not have."""
    assert ac.kernel_of(T, 64, 0) == "long"
    bad = {}
    for fam in ("neg", "last_heavy"):
        ratio = check_family(lib, fam, B, T, H, 64, 0)
        note("long", fam, ratio, f"T={T}")
        if not ratio <= 1.0:
            bad[fam] = ratio
    assert not bad, f"T={T}: |out - want| exceeds E: {bad}"
    for fam in ("neg", "last_heavy"):
        check_poison(lib, fam, T, 64, 0)


# ------------------------------------------------------------------------------------------ 3. several pairs per workgroup
@pytest.mark.parametrize("fam", ["sharp", "neg"])
@pytest.mark.parametrize("T", [257, 261, 288])
def test_persistent_kernel_walks_several_pairs(lib, T, fam):
    """attention_pk_kernel launches min(B H, CUs) workgroups: with H = 16 and the smallest B that gives B H >= 2 CUs + 37 pairs, 37
    workgroups or more walk three pairs and the others two -- the walk, the LDS-DMA of the next pair into the other half of the
    LDS, the buffer parity and the last pair, every pair's data its own.  E on every element of the batch (reference sample by
    sample), and a second launch gives the same bits."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    Hp = 16
    Bp = -(-(2 * cus + 37) // Hp)
    assert Bp * Hp >= 2 * cus + 37 and (Bp - 1) * Hp < 2 * cus + 37
    qkv = ac.MAKE[fam](Bp, T, Hp, 64, 5).cuda()
    out = run(lib, qkv, Bp, T, Hp, 64, 0)
    vmax = ac.vmax_of(qkv, Hp, 64)
    ratios = []
    for b in range(Bp):
        rows = slice(b * T, (b + 1) * T)
        want, pav = ac.reference(qkv[rows], 1, T, Hp, 64, 0)
        ratios.append(ac.worst(out[rows], want, pav, T, vmax))
    note("persistent", fam, max(ratios), f"T={T} B={Bp} H={Hp} ({Bp * Hp} pairs on {cus} CUs)")
    worst_b = max(range(Bp), key=lambda b: ratios[b])
    assert ratios[worst_b] <= 1.0, f"sample {worst_b}: err/E {ratios[worst_b]:.3f}; samples over E: {[b for b in range(Bp) if not ratios[b] <= 1.0]}"
    again = run(lib, qkv, Bp, T, Hp, 64, 0)
    assert torch.equal(bits(out), bits(again))


# ------------------------------------------------------------------------------------------ 4. isolation
@pytest.mark.parametrize("dh,T,causal", [(64, 33, 0), (64, 77, 1), (64, 128, 0), (64, 197, 0), (64, 257, 0), (64, 288, 0),
                                         (64, 257, 1), (64, 577, 0), (80, 33, 0), (80, 257, 0)])
def test_a_sample_does_not_depend_on_its_neighbours(lib, dh, T, causal):
    """One case per kernel form.  The neighbours hold +-60 in q and k and NaN / 60000 in v: a staging path that reads past the
    sample's rows, or a clamped row that lands in a neighbour, changes bits or leaves a NaN."""
    for fam in ("sharp", "neg", "last_heavy"):
        check_poison(lib, fam, T, dh, causal)


# ------------------------------------------------------------------------------------------ 5. ragged batches
LENS_128 = [33, 128, 1, 64, 97, 2, 77, 31, 96, 65, 32, 63]  # [1, 2, 31, 32, 33, 63, 64, 65, 77, 96, 97, 128] shuffled
LENS_77 = [50, 77, 1, 33, 64, 5, 32, 76]


def _i32(xs):
    return torch.tensor(xs, dtype=torch.int32, device="cuda")


def _offsets(lens):
    offs = [0]
    for n in lens[:-1]:
        offs.append(offs[-1] + n)
    return offs


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("lens", [LENS_128, LENS_77], ids=["max128", "max77"])
def test_ragged_batches(lib, lens, causal):
    """One launch of the packed batch (T = the longest length: 4 key blocks, then 3).  Every sample meets E against the reference
    at its own length; every sample has the bits of that sample launched without its batch -- in a launch of two, followed by a
    dummy of the longest length so that the kernel instantiation is the same, and, where the sample's own length already
    selects that instantiation, in a plain rectangular launch of it alone; the sentinel row behind the last sample is untouched."""
    dh, Tmax, n = 64, max(lens), sum(lens)
    offs = _offsets(lens)
    for fam in ac.families(causal):
        qkv = ac.ragged(fam, lens, H, dh, 11, causal).cuda()
        assert qkv.shape[0] == n
        out = torch.full((n + 1, H * dh), SENTINEL, dtype=torch.bfloat16, device="cuda")
        rc = launch(lib, qkv, out, len(lens), Tmax, H, dh, causal, 0, _i32(offs), _i32(lens))
        assert rc == 0, lib.clipx_last_error().decode()
        assert (out[n].float() == SENTINEL).all(), "the row behind the last sample was written"
        dummy = ac.sharp(1, Tmax, H, dh, 99).cuda()
        worst = 0.0
        for i, (o, ln) in enumerate(zip(offs, lens)):
            mine = qkv[o:o + ln]
            want, pav = ac.reference(mine, 1, ln, H, dh, causal)
            ratio = ac.worst(out[o:o + ln], want, pav, ln, ac.vmax_of(mine, H, dh))
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{fam} causal={causal} sample {i} (length {ln}): err/E {ratio:.3f}"
            pair = torch.cat([mine, dummy]).contiguous()
            out2 = torch.full((ln + Tmax, H * dh), SENTINEL, dtype=torch.bfloat16, device="cuda")
            rc = launch(lib, pair, out2, 2, Tmax, H, dh, causal, 0, _i32([0, ln]), _i32([ln, Tmax]))
            assert rc == 0, lib.clipx_last_error().decode()
            assert torch.equal(bits(out2[:ln]), bits(out[o:o + ln])), f"{fam} causal={causal} sample {i} (length {ln}) depends on its batch"
            if (ln + 31) // 32 == (Tmax + 31) // 32:
                alone = run(lib, mine.contiguous(), 1, ln, H, dh, causal)
                assert torch.equal(bits(alone), bits(out[o:o + ln])), f"{fam} causal={causal} sample {i} (length {ln}) differs from its rectangular launch"
        note("block", fam, worst, f"ragged max {Tmax} causal={causal}")


# ------------------------------------------------------------------------------------------ 6. the pooled last block
@pytest.mark.parametrize("dh,T,causal", [(64, 50, 0), (64, 77, 1), (64, 197, 0), (64, 257, 0), (64, 288, 0), (64, 577, 0), (80, 257, 0)])
def test_first_query_block_alone(lib, dh, T, causal):
    """q_blocks = 1: rows 0 .. min(32, T) - 1 of every sample are the bits of the full launch (the other rows are unspecified)."""
    for fam in ("sharp", "neg"):
        qkv = ac.MAKE[fam](B, T, H, dh, 4, causal).cuda()
        full = run(lib, qkv, B, T, H, dh, causal).view(B, T, H * dh)
        first = run(lib, qkv, B, T, H, dh, causal, q_blocks=1).view(B, T, H * dh)
        n = min(32, T)
        assert torch.isfinite(full.float()).all()
        assert torch.equal(bits(first[:, :n]), bits(full[:, :n])), f"{fam} dh={dh} T={T} causal={causal}"


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_of_the_new_entry_point_launch_nothing(lib):
    """Each refusal returns its code with a message and leaves the output buffer as it was; a good launch before and after gives
    the same bits."""
    qkv77 = ac.sharp(B, 77, H, 64, 6).cuda()
    before = run(lib, qkv77, B, 77, H, 64, 1)
    rows = 700
    qkv = torch.zeros(rows, 3 * 80, dtype=torch.float16, device="cuda")
    out = torch.full((rows, 80), SENTINEL, dtype=torch.bfloat16, device="cuda")
    one = _i32([0])
    for T, dh, causal, word in ((609, 64, 0, "608"), (609, 80, 0, "608"), (289, 64, 1, "288"), (289, 80, 0, "288"), (577, 80, 0, "288")):
        assert launch(lib, qkv, out, 1, T, 1, dh, causal) == E_UNSUPPORTED
        assert word in lib.clipx_last_error().decode()
    assert launch(lib, qkv, out, 1, 77, 1, 64, 1, 0, one, None) == E_ARG
    assert launch(lib, qkv, out, 1, 77, 1, 64, 1, 0, None, _i32([77])) == E_ARG
    assert launch(lib, qkv, out, 1, 77, 1, 80, 0, 0, one, _i32([77])) == E_UNSUPPORTED
    assert "ragged" in lib.clipx_last_error().decode()
    assert launch(lib, qkv, out, 1, 129, 1, 64, 0, 0, one, _i32([129])) == E_UNSUPPORTED
    assert "128" in lib.clipx_last_error().decode()
    for T in (97, 256):
        assert launch(lib, qkv, out, 1, T, 1, 80, 0) == E_UNSUPPORTED
        assert "97" in lib.clipx_last_error().decode()
    assert launch(lib, qkv, out, 1, 77, 1, 72, 0) == E_UNSUPPORTED
    assert launch(lib, qkv, out, 0, 77, 1, 64, 0) == E_ARG
    assert launch(lib, qkv, out, 1, 77, 1, 64, 0, -1) == E_ARG
    assert launch(lib, None, out, 1, 77, 1, 64, 0) == E_ARG
    assert (out.float() == SENTINEL).all()
    after = run(lib, qkv77, B, 77, H, 64, 1)
    assert torch.equal(bits(before), bits(after))
