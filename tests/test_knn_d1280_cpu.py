"""The width limit of the kNN library: 1280 is taken, anything wider is refused before the first HIP call, and the message names the limit."""
import ctypes as C


def test_create_refuses_widths_above_1280_and_takes_1280():
    from clip_retrieval_amd import load_library

    lib, h, E_UNSUPPORTED = load_library(), C.c_void_p(), -5
    for d in (1536, 1300):
        assert lib.knnx_create(0, d, 0, C.byref(h)) == E_UNSUPPORTED and b"1280" in lib.knnx_last_error() and not h.value
    rc = lib.knnx_create(0, 1280, 0, C.byref(h))  # (without a GPU this fails later, in HIP; with one it succeeds)
    assert rc != E_UNSUPPORTED
    if rc == 0:
        lib.knnx_destroy(h)
