"""CPU: the host side of the plain GEMM harness (sc_diag_gemm_bf16_ex, sc_diag_gemm_path, sc_diag_gemm_splitk) -- no device.

The harness checks its arguments by host arithmetic before it looks at the runtime, so with rt = NULL a call it would serve fails on the
NULL runtime alone and a call it refuses fails with its own status and message first.  Which kernel the launcher picks for a shape
(sc_gemm_plain_path, the function the launcher itself dispatches on) is host arithmetic too, given a CU count."""
import ctypes as C

import numpy as np
import pytest

from semcode_amd import _native

INVALID, UNSUPPORTED = -1, -4
CBLOCK, ABLOCK, SPLITK, TILE128 = 1, 2, 4, 8
DUMMY = np.zeros(4, np.float32)  # never touched before the runtime is


@pytest.fixture
def options():
    def set_(**kw):
        for k, v in kw.items():
            _native.diag_set_option(k, v)
    yield set_
    set_(gemm_order=-1, gemm_pp=-1, gemm_nt=-1)


def raw(epi=0, flags=0, M=256, N=256, K=64, A=DUMMY, W=DUMMY, bias=DUMMY, R=None, out=DUMMY):
    """(status, message) of one sc_diag_gemm_bf16_ex call with rt = NULL."""
    p = _native._ptr
    st = _native.lib().sc_diag_gemm_bf16_ex(None, epi, flags, p(A), p(W), p(bias), p(R), M, N, K, p(out), None)
    buf = C.create_string_buffer(1024)
    _native.lib().sc_last_error(buf, 1024)
    return st, buf.value.decode()


def host_state():
    """What the host-side entry points answer for a few fixed questions: must not move when a call is refused."""
    return (_native.diag_gemm_path(256, 768, 768, cus=256), _native.diag_gemm_path(256, 768, 768, cus=256, splitk=True),
            _native.diag_gemm_path(128, 384, 128, cus=256), _native.diag_gemm_splitk(512, 768, 768, 256), _native.diag_gemm_path())


VALID = [dict(), dict(epi=1), dict(epi=2, R=DUMMY), dict(flags=CBLOCK), dict(flags=ABLOCK), dict(flags=ABLOCK | CBLOCK), dict(flags=SPLITK),
         dict(flags=SPLITK | CBLOCK), dict(flags=TILE128 | CBLOCK), dict(flags=CBLOCK, M=128, N=384, K=128), dict(flags=ABLOCK, M=512, N=768, K=3072),
         dict(flags=TILE128 | SPLITK)]


@pytest.mark.parametrize("i", range(len(VALID)))
def test_a_call_the_harness_serves_fails_on_the_null_runtime_alone(i):
    st, msg = raw(**VALID[i])
    assert st == INVALID and "runtime is NULL" in msg, (VALID[i], st, msg)


BLOCKED_A = ("blocked A", "256-tile kernel only", "M%256==0", "N%256==0", "no split-K scratch", "128-tile")
REFUSED = [
    (dict(A=None), INVALID, ("NULL argument",)),
    (dict(W=None), INVALID, ("NULL argument",)),
    (dict(bias=None), INVALID, ("NULL argument",)),
    (dict(out=None), INVALID, ("NULL argument",)),
    (dict(epi=3), INVALID, ("bad epilogue",)),
    (dict(epi=-1), INVALID, ("bad epilogue",)),
    (dict(epi=16), INVALID, ("bad epilogue",)),              # the old entry's "+ 16" is a flag here
    (dict(epi=2), INVALID, ("missing residual",)),
    (dict(flags=16), INVALID, ("flags 16",)),
    (dict(flags=-1), INVALID, ("flags -1",)),
    (dict(M=64), UNSUPPORTED, ("M%128==0",)),
    (dict(N=192), UNSUPPORTED, ("N%128==0",)),
    (dict(K=96), UNSUPPORTED, ("K%64==0",)),
    (dict(M=0), UNSUPPORTED, ("M%128==0",)),
    (dict(flags=ABLOCK, M=128), UNSUPPORTED, BLOCKED_A + ("M 128",)),
    (dict(flags=ABLOCK, M=384), UNSUPPORTED, BLOCKED_A + ("M 384",)),
    (dict(flags=ABLOCK, N=384), UNSUPPORTED, BLOCKED_A + ("N 384",)),
    (dict(flags=ABLOCK | SPLITK), UNSUPPORTED, BLOCKED_A + ("flags 6",)),
    (dict(flags=ABLOCK | CBLOCK | SPLITK, M=512, N=768, K=768), UNSUPPORTED, BLOCKED_A + ("flags 7",)),
    (dict(flags=ABLOCK | TILE128), UNSUPPORTED, BLOCKED_A + ("flags 10",)),
]


@pytest.mark.parametrize("i", range(len(REFUSED)))
def test_a_refused_call_fails_with_its_own_status_and_message(i):
    fields, status, words = REFUSED[i]
    before = host_state()
    st, msg = raw(**fields)
    assert st == status and all(w in msg for w in words) and "sc_diag_gemm_bf16_ex" in msg and "runtime" not in msg, (fields, st, msg)
    assert host_state() == before
    st, msg = raw()  # and the next call the harness serves gets as far as before
    assert st == INVALID and "runtime is NULL" in msg


def test_python_wrapper_reaches_the_library_with_no_runtime():
    A, W, b = np.zeros((256, 128), np.float32), np.zeros((256, 128), np.float32), np.zeros(256, np.float32)
    with pytest.raises(_native.ScError, match="runtime is NULL"):
        _native.diag_gemm_bf16_ex(None, A, W, b, a_blocked=True, c_blocked=True)
    with pytest.raises(_native.ScError, match="blocked A"):
        _native.diag_gemm_bf16_ex(None, A, W, b, a_blocked=True, splitk=True)
    with pytest.raises(_native.ScError, match="blocked A"):
        _native.diag_gemm_bf16_ex(None, A[:128], W, b, a_blocked=True)
    with pytest.raises(ValueError):
        _native.diag_gemm_bf16_ex(None, A, W, b, R=np.zeros((128, 256), np.float32), epi=2)
    p = _native._ptr
    with pytest.raises(_native.ScError, match="sc_diag_gemm_bf16: NULL argument"):  # the old entry point: the runtime first, its own name
        _native._check(_native.lib().sc_diag_gemm_bf16(None, 0, p(A), p(W), p(b), None, 256, 256, 128, p(A)))


def test_gemm_order_option_round_trip(options):
    """-1 (and anything below) = by shape: order 0 while N K 2 bytes of weights fit 8 MiB, 16 beyond; another value is the order word."""
    small, large = (256, 768, 768), (256, 6144, 1024)  # 1.1 MiB and 12 MiB of weights
    for v in (0, 1, 16, 17, 6):
        options(gemm_order=v)
        assert _native.diag_gemm_path(*small, cus=256)["order"] == v and _native.diag_gemm_path(*large, cus=256)["order"] == v
    for v in (-1, -7):
        options(gemm_order=v)
        assert _native.diag_gemm_path(*small, cus=256)["order"] == 0 and _native.diag_gemm_path(*large, cus=256)["order"] == 16
    assert _native.diag_gemm_path(256, 4096, 1024, cus=256)["order"] == 0   # exactly 8 MiB still walks row panel by row panel
    assert _native.diag_gemm_path(256, 4352, 1024, cus=256)["order"] == 16
    with pytest.raises(_native.ScError, match="unknown option"):
        _native.diag_set_option("gemm_orders", 1)
    assert _native.diag_gemm_path(*large, cus=256)["order"] == 16


def test_path_follows_shape_and_options(options):
    path = _native.diag_gemm_path
    options(gemm_order=-1, gemm_pp=-1, gemm_nt=-1)
    assert path(256, 768, 768, cus=256) == dict(tile=256, splitk=1, order=0, pp=4, nt=0)
    assert path(256, 256, 64, cus=256)["pp"] == 0 and path(256, 256, 128, cus=256)["pp"] == 4  # one K-tile has no ring
    for shape in ((128, 384, 128), (256, 1152, 896), (384, 768, 3072), (256, 896, 4864)):        # M or N not a multiple of 256
        assert path(*shape, cus=256) == path(*shape, cus=256, splitk=True) == dict(tile=128, splitk=1, order=0, pp=0, nt=0)
    # split-K: only with the scratch, only where the rule splits; the pair walks row-major on the one-barrier loop
    assert path(256, 768, 768, cus=256, splitk=True) == dict(tile=256, splitk=4, order=1, pp=0, nt=0)
    assert path(256, 256, 64, cus=256, splitk=True) == path(256, 256, 64, cus=256)
    assert path(2048, 768, 768, cus=256, splitk=True)["splitk"] == 1
    assert path(256, 768, 768, cus=4, splitk=True)["splitk"] == 1
    assert path(32768, 1024, 64, cus=256)["nt"] == 1 and path(32768 - 256, 1024, 64, cus=256)["nt"] == 0  # 64 MiB of output
    options(gemm_pp=0, gemm_nt=1)
    assert path(256, 768, 768, cus=256) == dict(tile=256, splitk=1, order=0, pp=0, nt=1)
    options(gemm_pp=-1, gemm_nt=0)
    assert path(32768, 1024, 128, cus=256) == dict(tile=256, splitk=1, order=0, pp=4, nt=0)
    with pytest.raises(_native.ScError, match="M%128==0"):
        path(200, 256, 64, cus=256)


def splitk_rule(M, N, K, cus):
    """sc_gemm_splitk_factor restated: the largest divisor d of the K-tile count with at least 3 K-tiles per slice and tiles * d <= cus,
    for 256-tile shapes of at most 1024 rows whose tiles fill at most half the CUs."""
    if M % 256 or N % 256 or M > 1024:
        return 1
    tiles, nk = (M // 256) * (N // 256), K // 64
    best = max([d for d in range(2, nk + 1) if nk % d == 0 and nk // d >= 3 and tiles * d <= cus], default=1)
    return best if tiles * 2 <= cus else 1


def test_splitk_factor_matches_its_rule():
    seen = set()
    for cus in (4, 8, 64, 104, 256, 304):
        for M in (128, 256, 384, 512, 768, 1024, 1280, 2048):
            for N in (128, 256, 384, 768, 1152, 2304, 3072):
                for K in (64, 128, 192, 256, 384, 448, 576, 768, 1024, 1536, 3072, 4864):
                    got = _native.diag_gemm_splitk(M, N, K, cus)
                    assert got == splitk_rule(M, N, K, cus), (M, N, K, cus, got)
                    seen.add(got)
                    if got > 1:
                        tiles = (M // 256) * (N // 256)
                        assert (K // 64) % got == 0 and K // 64 // got >= 3 and tiles * got <= cus and M <= 1024
    assert {1, 2, 3, 4, 6, 8, 16} <= seen
    assert _native.diag_gemm_splitk(1280, 256, 768, 256) == 1      # M > 1024
    assert _native.diag_gemm_splitk(1024, 768, 768, 16) == 1       # 12 tiles: tiles * 2 > cus
    assert _native.diag_gemm_splitk(256, 256, 64, 256) == 1        # a single K-tile
    assert _native.diag_gemm_splitk(256, 768, 3072, 256) == 16 and _native.diag_gemm_splitk(512, 768, 768, 256) == 4
