"""The dispatch decision of pd_gemm_tn_f16x2 (csrc/gemm_f16x2.hip: f16x2_plan) through its host-only query pd_gemm_tn_f16x2_which, on the
boundaries of every rule: 0 = 128 x 128 tiles, 1 = 256 x 256 tiles, 2 = row stream, 5 = producer / consumer wavefronts, -1 = refused.
The expectations were read off the launcher's chain of tests as it stood before the decision became one function.  No GPU is needed: the
query and pd_debug_set are host code, and without a device the CU count falls back to 256, which is also the MI355X's count — the two
N = 8192 / 8448 rows (the row stream's N / 256 <= CUs / 8) ASSUME 256 CUs."""
import pytest

AMAX, A_ONLY, B_ONLY, BITS, C, BF16 = "amax", "a only", "b only", "bits", "c", "bf16out"

CASES = [
    # (debug value, mode, (M, N, K), options, expected id)
    (0, 0, (8192, 256, 256), {AMAX}, 2),
    (0, 0, (8191, 256, 256), {AMAX}, 0),
    (0, 0, (8192, 256, 256), {A_ONLY}, 0),
    (0, 0, (8192, 256, 256), {AMAX, BF16}, 0),
    (0, 0, (8192, 320, 256), set(), 0),
    (0, 0, (8192, 1024, 256), set(), 2),
    (0, 0, (8192, 8192, 256), set(), 2),            # 32 panels: 256 CUs / 8
    (0, 0, (8192, 8448, 256), set(), 1),            # 33 panels: no whole group of 8 x 33 workgroups on 256 CUs
    (0, 0, (8192, 256, 512), set(), 5),
    (0, 0, (8192, 256, 512), {C}, 0),
    (0, 0, (8192, 256, 512), {BF16}, 0),
    (0, 0, (8192, 256, 512), {A_ONLY}, 0),
    (0, 0, (8192, 512, 512), set(), 5),
    (0, 0, (8192, 768, 512), set(), 0),
    (0, 0, (8192, 1024, 512), set(), 1),
    (0, 0, (8192, 256, 544), set(), 5),
    (0, 0, (8192, 256, 520), set(), 0),
    (0, 0, (8191, 256, 512), set(), 0),
    (0, 0, (524287, 256, 1024), set(), 5),
    (0, 0, (524288, 256, 1024), set(), 0),          # A reaches 2^31 bytes
    (0, 1, (8192, 512, 256), {BITS, AMAX}, 2),
    (0, 1, (8192, 256, 256), {BITS, AMAX}, 1),
    (0, 1, (8192, 1024, 256), {AMAX}, 1),
    (0, 1, (7936, 1024, 256), {AMAX}, 0),
    (0, 1, (2304, 512, 256), {BITS, B_ONLY}, 1),
    (0, 1, (2048, 384, 256), {BITS}, -1),
    (0, 2, (8192, 1024, 256), {BITS, AMAX}, 2),
    (80, 0, (8192, 256, 256), {AMAX}, 0),
    (80, 0, (8192, 256, 512), set(), 0),
    (80, 0, (8192, 1024, 256), set(), 1),
    (61, 0, (8192, 256, 256), set(), 2),
    (61, 0, (8192, 256, 512), set(), 0),
    (62, 1, (8192, 1024, 256), {BITS, AMAX}, 1),
    (62, 0, (8192, 256, 256), {AMAX}, 0),
    (70, 0, (8192, 1024, 256), set(), 1),
    (70, 1, (8192, 1024, 256), {BITS, AMAX}, 1),
    (3, 0, (2048, 256, 256), set(), 1),
    (13, 0, (2048, 256, 256), set(), 1),
    (3, 0, (333, 72, 40), set(), -1),
    (13, 0, (333, 72, 40), set(), -1),
    (4, 0, (2048, 1024, 256), set(), 0),
    (14, 0, (2048, 1024, 256), set(), 0),
    (92, 0, (8192, 256, 128), set(), 5),
    (92, 0, (8192, 1024, 512), set(), 5),
    (94, 0, (8192, 256, 512), set(), 5),
]


@pytest.mark.parametrize("dbg,mode,shape,opts,want", CASES, ids=lambda v: "-".join(sorted(v)) or "plain" if isinstance(v, set) else None)
def test_f16x2_which_is_the_launchers_decision(dbg, mode, shape, opts, want):
    from partdistillation_amd import lib
    L = lib.load()
    M, N, K = shape
    L.pd_debug_set(b"f16x2_tile", dbg)
    try:
        got = L.pd_gemm_tn_f16x2_which(M, N, K, K, K, mode, int(BITS in opts), int(AMAX in opts or A_ONLY in opts), int(AMAX in opts or B_ONLY in opts),
                                       int(C in opts), int(BF16 in opts))
    finally:
        L.pd_debug_set(b"f16x2_tile", 0)
    assert got == want
