"""Pins of the encode half's host layer: what a call launches and what bytes it returns, recorded before the host layer was
rebuilt (csrc/clipx_host.h) and demanded of every later version of it.

Per call of the tiny CLIP model (tiny-B/32, the oracle's seed-0 weights, the synthetic pixels / tokens of the encoder tests):
  * with clipx_profile_enable(1): per kind 0 .. 3 the (launches, flops) of clipx_profile_get, and clipx_last_text_rows -- exact
    integers and shape-derived doubles, compared with ==;
  * with profiling off: the sha256 of the fp16 output bytes, three calls in a row (B = 3 is first launched plainly, then captured
    into a hipGraph, then replayed).
The multilingual tower (the tiny shape of test_mclip_gpu.py, random weights, texts of bert_cases.synth_ids): B = 5 with mixed
lengths, whole and in chunks of two (CLIPX_MAX_BATCH=2), sha256 of the f32 and fp16 outputs.

tests/golden/encode_pins/pins.json was written by record() of this module, run at the parent commit of the rebuild (259febb) with
ENCODE_PINS_RECORD set; a hash is kept only where two separate processes gave the same one: tests/golden/encode_pins/README.md."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_cases as bc  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_pins", "pins.json")

# case -> (tower, B, options switched OFF for the call)
CLIP_CASES = {
    "image-b3": ("image", 3, ()),
    "image-b12": ("image", 12, ()),
    "text-b3": ("text", 3, ()),
    "text-b12-ragged": ("text", 12, ()),
    "text-b12-rectangular": ("text", 12, ("OPT_RAGGED_TEXT",)),
    "text-b12-full-last-block": ("text", 12, ("OPT_POOL_LAST_BLOCK",)),
}
BERT_TINY = dict(vocab=1000, max_pos=130, pos_offset=0, width=256, layers=2, heads=4, mlp=512, out_dim=128, max_len=128,
                 dense_bias=False, ln_eps=1e-12)
BERT_LENS = [1, 33, 128, 2, 64]
BERT_CASES = {"bert-b5-whole": None, "bert-b5-chunks-of-2": "2"}  # case -> CLIPX_MAX_BATCH


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _clip_encoder():
    from clip_retrieval_amd.encoder import ClipArch, ClipEncoder
    from oracle.clip_oracle import ARCHS, HFClipOracle

    arch = ARCHS["tiny-B/32"]
    blob = HFClipOracle(arch, seed=0).export_blob()
    return ClipEncoder(ClipArch(**{k: getattr(arch, k) for k in ClipArch.__dataclass_fields__}), blob, 0)


def clip_pins(enc, case):
    """{"profile": [[launches, flops] per kind], "text_rows": n, "sha256": [three calls]} of one case."""
    from oracle.clip_oracle import synth_pixels_u8, synth_tokens

    tower, B, off = CLIP_CASES[case]
    if tower == "image":
        data, call = synth_pixels_u8(B), enc.encode_image
    else:
        data, call = synth_tokens(B), enc.encode_text
    for o in off:
        enc.set_option(getattr(enc, o), 0)
    try:
        enc.profile(1)
        try:
            call(data)
        finally:
            enc.profile(0)
        prof = []
        for kind in range(4):
            n, _, fl = enc.profile_get(kind)
            prof.append([n, fl])
        rows = enc.last_text_rows() if tower == "text" else None
        hashes = [_sha(call(data).view(np.uint16)) for _ in range(3)]
    finally:
        for o in off:
            enc.set_option(getattr(enc, o), 1)
    return {"profile": prof, "text_rows": rows, "sha256": hashes}


def bert_pins(case):
    """{"sha256_f32": ..., "sha256_f16": ...} of the multilingual tower's case, on a handle of its own."""
    from clip_retrieval_amd import mclip

    arch = mclip.BertArch(**BERT_TINY)
    ids = bc.synth_ids(len(BERT_LENS), BERT_LENS, arch.vocab, arch.max_len, seed=12, per_sample=3)
    old, mb = os.environ.get("CLIPX_MAX_BATCH"), BERT_CASES[case]
    if mb:
        os.environ["CLIPX_MAX_BATCH"] = mb
    try:
        enc = mclip.BertTextEncoder(arch, mclip.random_bert_blob(arch, 4), 0)
    finally:
        if mb:
            os.environ.pop("CLIPX_MAX_BATCH")
            if old is not None:
                os.environ["CLIPX_MAX_BATCH"] = old
    try:
        o32, o16 = enc.encode_ids(ids, lens=BERT_LENS, f16=True)
    finally:
        enc.close()
    return {"sha256_f32": _sha(o32.view(np.uint32)), "sha256_f16": _sha(o16.view(np.uint16))}


def record():
    """Every case -> its pins.  Run at a commit whose behaviour is trusted (module docstring), never against new code."""
    enc = _clip_encoder()
    try:
        pins = {case: clip_pins(enc, case) for case in sorted(CLIP_CASES)}
    finally:
        enc.close()
    pins.update({case: bert_pins(case) for case in sorted(BERT_CASES)})
    return pins


def merge(first, second):
    """Keeps a hash only where both processes' recordings agree (and, per case, where its three calls did); everything else of
    the two recordings must be equal.  -> (pins, {case: reason} of the hashes left out)"""
    out, left = {}, {}
    for case in sorted(first):
        a, b = dict(first[case]), dict(second[case])
        for key in [k for k in a if k.startswith("sha256")]:
            va, vb = a.pop(key), b.pop(key)
            if va != vb:
                left[f"{case}:{key}"] = "the two processes gave different bytes"
            elif isinstance(va, list) and len(set(va)) != 1:
                left[f"{case}:{key}"] = "three calls of one process gave different bytes"
            else:
                out.setdefault(case, {})[key] = va
        assert a == b, f"{case}: the profile counts of the two processes differ: {a} / {b}"
        out.setdefault(case, {}).update(a)
    return out, left


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN, encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def clip_enc():
    enc = _clip_encoder()
    yield enc
    enc.close()


def test_golden_file_holds_the_required_hashes(golden):
    for case in ("image-b12", "text-b12-ragged", "text-b12-rectangular", "text-b12-full-last-block"):
        assert "sha256" in golden[case], f"{case}: no output hash was recorded"
    assert sorted(golden) == sorted(list(CLIP_CASES) + list(BERT_CASES))


@pytest.mark.parametrize("case", sorted(CLIP_CASES))
def test_clip_call_launches_and_returns_what_was_recorded(clip_enc, golden, case):
    want, got = golden[case], clip_pins(clip_enc, case)
    print(f"{case}: profile {got['profile']}, text rows {got['text_rows']}")
    assert got["profile"] == want["profile"]
    assert got["text_rows"] == want["text_rows"]
    if "sha256" in want:
        assert got["sha256"] == want["sha256"], "the fp16 embeddings are not the recorded bytes"


@pytest.mark.parametrize("case", sorted(BERT_CASES))
def test_multilingual_tower_returns_what_was_recorded(golden, case):
    want, got = golden[case], bert_pins(case)
    for key, v in want.items():
        assert got[key] == v, f"{case}: {key} is not the recorded one"


if __name__ == "__main__":
    # ENCODE_PINS_RECORD=out.json python tests/test_encode_pins_gpu.py [first.json]: records into out.json; with the recording of
    # an earlier process as argument, writes the merged golden file (hashes both agree on) and a list of what was left out.
    target = os.environ.get("ENCODE_PINS_RECORD")
    if not target:
        sys.exit("set ENCODE_PINS_RECORD to the file to write")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    result = record()
    if len(sys.argv) > 1:
        with open(sys.argv[1], encoding="utf-8") as f:
            result, left_out = merge(json.load(f), result)
        print("left out:", json.dumps(left_out, indent=1, sort_keys=True))
    with open(target, "w", encoding="utf-8") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {target}")
