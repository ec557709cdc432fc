"""Host-side checks of the K-view preprocess's LDS-staged SH row loader (no GPU): it is eligible
only for rows of exactly (D + 1)^2 coefficients that are whole 16-B pieces (3 M a multiple of 4) at a
16-B aligned base; every other layout takes the per-lane loader (gs_debug_sh_rows_staged: the
predicate a -DGS_PREVIEWS_ROWS=1 build of gs_forward_preprocess_views launches by; the default
build holds every layout's rows in registers and needs no such condition)."""
import ctypes


def _staged(D, M, addr):
    from diff_gaussian_rasterization import _native

    return _native.load().gs_debug_sh_rows_staged(D, M, ctypes.c_void_p(addr))


def test_staged_loader_eligibility():
    base = 0x7F0000001000
    for D in range(0, 4):
        M = (D + 1) ** 2
        assert _staged(D, M, base) == (1 if (3 * M) % 4 == 0 else 0), D
    assert [_staged(D, (D + 1) ** 2, base) for D in range(4)] == [0, 1, 0, 1]
    # rows longer than the degree needs (a stride), of any length
    for D, M in ((0, 4), (0, 16), (1, 9), (1, 16), (2, 16), (3, 25)):
        assert _staged(D, M, base) == 0, (D, M)
    # alignment of the row base: every offset but a multiple of 16 B is refused
    for off in range(0, 64, 4):
        assert _staged(3, 16, base + off) == (1 if off % 16 == 0 else 0), off
        assert _staged(1, 4, base + off) == (1 if off % 16 == 0 else 0), off
    # no rows (precomputed colours), degrees outside 0..3
    assert _staged(3, 16, None) == 0
    assert _staged(-1, 0, base) == 0 and _staged(4, 25, base) == 0 and _staged(5, 36, base) == 0
