"""CPU: which EPI_LNA_* launches the GEMM launcher runs as strips (sc_gemm_strip_rule / sc_gemm_strip_tiles through
sc_diag_gemm_strip with an explicit CU count: host arithmetic, no device).

A strip makes the scheduling quantum L tiles instead of one.  With C workgroups side by side, S strips of L tiles take
ceil(S / C) * L tile-times and T single tiles ceil(T / C); the rule may choose a strip only where that is no more, only with at
least one strip per CU, and only for the two measured shapes (N = 2304 -> 3, N = 3072 -> 6, K = 768)."""
import pytest

from semcode_amd import _native


@pytest.fixture
def options():
    def set_(**kw):
        for k, v in kw.items():
            _native.diag_set_option(k, v)
    yield set_
    set_(gemm_strip=-1, gemm_strip_n=0, gemm_pp=-1)


def ceil_div(a, b):
    return -(-a // b)


@pytest.mark.parametrize("M,N,K,cus,want", [
    (65536, 2304, 768, 256, 3),    # the benchmark's step: 768 strips = 3 rounds x 3 = 9 = ceil(2304 / 256)
    (65536, 3072, 768, 256, 6),    # 512 strips = 2 rounds x 6 = 12 = ceil(3072 / 256)
    (131072, 2304, 768, 256, 3),
    (131072, 3072, 768, 256, 6),
    (32768, 2304, 768, 256, 0),    # 384 strips: 2 rounds x 3 = 6 tile-times against 5
    (32768, 3072, 768, 256, 6),    # 256 strips, one per CU: 6 tile-times against 6
    (49152, 3072, 768, 256, 0),    # 384 strips would take 12 tile-times against 9
    (49152, 2304, 768, 256, 0),
    (65536 + 256, 2304, 768, 256, 0),  # a packed batch just over a whole number of rounds: 12 against 10
    (65536 - 256, 3072, 768, 256, 6),  # 510 strips: 2 rounds x 6 = 12 = ceil(3060 / 256)
    (16384, 3072, 768, 256, 0),    # 128 strips: fewer than CUs
    (1024, 2304, 768, 256, 0),
    (65536, 768, 768, 256, 0),     # out-projection shape: not an EPI_LNA_* GEMM, and not a measured N
    (65536, 2304, 1024, 256, 0),   # not a measured K
    (65536, 2304, 768, 304, 0),    # another CU count: 768 strips = 3 rounds x 3 = 9 against ceil(2304 / 304) = 8
    (65500, 2304, 768, 256, 0),
])
def test_shape_rule_cases(options, M, N, K, cus, want):
    options(gemm_strip=-1, gemm_strip_n=0, gemm_pp=-1)
    assert _native.diag_gemm_strip(M, N, K, cus) == want


def test_shape_rule_never_adds_a_round(options):
    """Every M (multiples of 256 up to 2^18) x both shapes x several CU counts: a chosen strip takes no more tile-times than the
    per-tile walk and leaves at least one strip per CU."""
    options(gemm_strip=-1, gemm_strip_n=0, gemm_pp=-1)
    chosen = 0
    for cus in (64, 128, 256, 304):
        for N, L0 in ((2304, 3), (3072, 6)):
            for M in range(256, 2 ** 18 + 1, 256):
                L = _native.diag_gemm_strip(M, N, 768, cus)
                assert L in (0, L0)
                if L:
                    chosen += 1
                    panels, tiles_n = M // 256, N // 256
                    strips = panels * (tiles_n // L)
                    assert strips >= cus, (M, N, cus)
                    assert ceil_div(strips, cus) * L <= ceil_div(panels * tiles_n, cus), (M, N, cus)
    assert chosen > 0


def test_forced_values_and_what_switches_strips_off(options):
    options(gemm_strip=4, gemm_strip_n=0, gemm_pp=-1)
    assert _native.diag_gemm_strip(256, 1024, 256, 256) == 4
    assert _native.diag_gemm_strip(256, 768, 256, 256) == 3       # clamped to the tiles of a row panel
    options(gemm_strip_n=1024)
    assert _native.diag_gemm_strip(256, 1024, 256, 256) == 4
    assert _native.diag_gemm_strip(256, 768, 256, 256) == 0       # other N: per tile, whatever the shape rule says
    assert _native.diag_gemm_strip(65536, 2304, 768, 256) == 0
    options(gemm_strip_n=0, gemm_pp=0)                            # the one-barrier loop has no prefetching form
    assert _native.diag_gemm_strip(256, 1024, 256, 256) == 0
    assert _native.diag_gemm_strip(65536, 2304, 768, 256) == 0
    options(gemm_pp=-1, gemm_strip=0)
    assert _native.diag_gemm_strip(65536, 2304, 768, 256) == 0
    options(gemm_strip=-1)
    assert _native.diag_gemm_strip(65536, 2304, 768, 256) == 3
