"""CPU: the C ABI of the shared-prefix decode attention (csrc/decode_shared.hip).  Every case here is refused by the argument
checks, which return before any HIP call, so no GPU is needed."""
import ctypes as C

import pytest

HQ, HKV = 12, 2
ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
            C.c_void_p]
NAMES = ("qkv", "qw", "kw", "eps", "und", "cos", "sin", "kp", "vp", "plen", "ks", "vs", "slen", "batch", "srows", "smax", "Hq", "Hkv",
         "scale", "out", "ws", "stream")


@pytest.fixture(scope="module")
def lib():
    from g2vlm_amd import build
    lib = C.CDLL(build.build())
    lib.g2v_decode_attn_shared.argtypes = ARGTYPES
    lib.g2v_decode_attn_shared.restype = C.c_int
    lib.g2v_decode_attn_shared_workspace.argtypes = [C.c_int] * 5
    lib.g2v_decode_attn_shared_workspace.restype = C.c_int64
    return lib


def good(**kw):
    """A valid argument set (the pointers are never dereferenced: every call below is refused first), with overrides."""
    a = dict(qkv=16, qw=16, kw=16, eps=1e-6, und=1, cos=16, sin=16, kp=16, vp=16, plen=100, ks=16, vs=16, slen=16, batch=4, srows=256,
             smax=256, Hq=HQ, Hkv=HKV, scale=128 ** -0.5, out=16, ws=16, stream=None)
    a.update(kw)
    return [a[n] for n in NAMES]


def test_library_exports_the_shared_prefix_symbols(lib):
    from g2vlm_amd import hip
    assert hasattr(lib, "g2v_decode_attn_shared") and hasattr(lib, "g2v_decode_attn_shared_workspace")
    assert "g2v_decode_attn_shared" in hip.EXPORTS and "g2v_decode_attn_shared_workspace" in hip.EXPORTS
    assert callable(hip.decode_attn_shared) and callable(hip.decode_attn_shared_workspace)


@pytest.mark.parametrize("ptr", ["qkv", "qw", "kw", "cos", "sin", "kp", "vp", "ks", "vs", "slen", "out", "ws"])
def test_null_pointers_are_refused(lib, ptr):
    assert lib.g2v_decode_attn_shared(*good(**{ptr: None})) == -22


@pytest.mark.parametrize("bad", [dict(batch=0), dict(batch=65), dict(batch=-3), dict(plen=0), dict(plen=-1), dict(Hq=13),
                                 dict(Hq=18, Hkv=2), dict(Hq=12, Hkv=1), dict(Hkv=0), dict(srows=255), dict(smax=300, srows=299),
                                 dict(smax=0)])
def test_invalid_shapes_are_refused(lib, bad):
    assert lib.g2v_decode_attn_shared(*good(**bad)) == -22


def test_workspace_is_zero_for_invalid_shapes_and_grows_with_batch(lib):
    ws = lib.g2v_decode_attn_shared_workspace
    for args in [(HQ, HKV, 0, 100, 64), (HQ, HKV, 65, 100, 64), (HQ, HKV, 4, 0, 64), (13, HKV, 4, 100, 64), (18, 2, 4, 100, 64),
                 (HQ, 0, 4, 100, 64), (HQ, HKV, 4, 100, 0)]:
        assert ws(*args) == 0, args
    sizes = [ws(HQ, HKV, b, 17000, 192) for b in (1, 2, 5, 8, 16, 64)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    # what the engine allocates must not depend on the prefix length
    assert ws(HQ, HKV, 8, 1, 192) == ws(HQ, HKV, 8, 17000, 192) == ws(HQ, HKV, 8, 250000, 192)
    # at least the combine's [B][Hq][128][130] fp32 partials
    assert ws(HQ, HKV, 8, 17000, 192) >= 8 * HQ * 128 * 130 * 4
