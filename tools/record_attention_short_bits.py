"""Records tests/golden/attention_short_bits.npz: SHA-256 of the attention output bits at two short shapes, from a given libclipx.so.

The long-sequence kernel must leave every shape at T <= 288 on the kernel it ran before, bit for bit
(tests/test_long_seq_gpu.py::test_old_shapes_give_the_old_bits).  The file is recorded ONCE from the library of the commit before
that kernel: build that commit's clip-retrieval_amd/csrc into a library of its own and, on the MI355X,

    python tools/record_attention_short_bits.py --lib <that libclipx.so> --out tests/golden/attention_short_bits.npz

Inputs are test_attention's (tests/test_clip_gpu.py): randn -> fp16 from the CPU generator seeded T * 31 + H, q scaled by 2.
Per shape the file keeps in_<name> (SHA-256 of the input bytes), out_<name> (SHA-256 of the bf16 output bytes) and head_<name> (the
first 256 output values as int16 bits, to see at a glance how far off a mismatch is)."""
import argparse
import ctypes as C
import hashlib

import numpy as np
import torch

SHAPES = (("b2_t257_h16", (2, 257, 16, 0)), ("b3_t77_h12_causal", (3, 77, 12, 1)))


def inputs(B, T, H, dh=64):
    g = torch.Generator().manual_seed(T * 31 + H)
    qkv = (torch.randn(B * T, 3 * H * dh, generator=g)).to(torch.float16)
    qkv[:, : H * dh] *= 2.0
    return qkv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    lib = C.CDLL(a.lib)
    lib.clipx_attention_device.restype = C.c_int
    lib.clipx_attention_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    rec = {}
    for name, (B, T, H, causal) in SHAPES:
        qkv = inputs(B, T, H)
        rec["in_" + name] = np.frombuffer(hashlib.sha256(qkv.numpy().tobytes()).digest(), dtype=np.uint8)
        dev = qkv.cuda()
        outs = []
        for _ in range(2):  # twice: the bits must not depend on the run
            out = torch.empty(B * T, H * 64, dtype=torch.bfloat16, device="cuda")
            rc = lib.clipx_attention_device(0, C.c_void_p(dev.data_ptr()), C.c_void_p(out.data_ptr()), B, T, H, causal, None)
            assert rc == 0, rc
            torch.cuda.synchronize()
            outs.append(out.view(torch.int16).cpu().numpy())
        assert np.array_equal(outs[0], outs[1])
        rec["out_" + name] = np.frombuffer(hashlib.sha256(outs[0].tobytes()).digest(), dtype=np.uint8)
        rec["head_" + name] = outs[0].reshape(-1)[:256].copy()
        print(name, hashlib.sha256(outs[0].tobytes()).hexdigest())
    np.savez(a.out, **rec)


if __name__ == "__main__":
    main()
