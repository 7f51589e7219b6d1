"""`window_stencil_plan` (csrc/window_stencil.hip) and the query around it (`ipsr_window_corr_plan`, csrc/corr_argmax.hip), restated:
which kernel forms the window arg-max of a shift_sz > 1 forward, over how many workgroups and ranges of k', with how much LDS.
tests/test_window_stencil_abi.py holds it against the library without a GPU; the GPU tests take their cases' plans from the library
and their expectations (which case splits, which does not, which falls outside the envelope) from here.
"""
import corr_plan as P

LDS_LIMIT = 160 * 1024        # WS_LDS_LIMIT: the LDS a workgroup may have
THREADS = 256                 # WS_THREADS
MAXQ = 3                      # WS_MAXQ: columns qx per thread, 64 apart
MIN_KROWS = 8                 # WS_MIN_KROWS: a range of window rows ky is at least this long
CHIP_WGS = 256                # WS_CHIP_WGS
MAX_WGS_PER_CU = 8            # WS_MAX_WGS_PER_CU
MIN_WG_ROWS = 1               # WS_MIN_WG_ROWS: the size rule of option 8 = 0 (profiles/window_stencil_lds.txt): workgroup rows B * nH

STREAMING, LDS_TILED = 0, 1


def envelope(h, w, p):
    """The shapes the LDS-tiled kernel can run: the p blocks of w x w floats and the row of inverse norms in one workgroup's LDS."""
    return p >= 2 and (p * w * w + w) * 4 <= LDS_LIMIT and w - p + 1 <= 64 * MAXQ


def lds_bytes(w, p):
    words = p * w * w + w
    nbuf = 2 if 2 * words * 4 <= LDS_LIMIT // 2 else 1
    return 4 * max(nbuf * words, 2 * THREADS * MAXQ)


def admitted(B, h, w, p, option):
    if option == 1 or not envelope(h, w, p):
        return False
    return option == 2 or B * (h - p + 1) >= MIN_WG_ROWS


def plan(B, h, w, p, option=0):
    """-> what ipsr_window_corr_plan answers under ipsr_debug_set_option(8, option)."""
    nH, nW = h - p + 1, w - p + 1
    Np = nH * nW
    slices = P.window_plan(B, Np)[0]
    if not admitted(B, h, w, p, option):
        return {"variant": STREAMING, "workgroups": P.cdiv(Np, 256) * slices * B, "split": slices, "lds_bytes": 0}
    per_cu = min(LDS_LIMIT // lds_bytes(w, p), MAX_WGS_PER_CU)
    split = max(1, min((CHIP_WGS * per_cu + B * nH // 2) // (B * nH), nH // MIN_KROWS, slices))
    kper = P.cdiv(nH, split)
    split = P.cdiv(nH, kper)
    return {"variant": LDS_TILED, "workgroups": B * nH * split, "split": split, "lds_bytes": lds_bytes(w, p)}


# the sweep of the host test
EXTENTS = {p: sorted(set(range(p, 13)) | {31, 32, 33, 64, 96, 116, 117, 120}) for p in (2, 3, 4)}
BATCHES = (1, 3, 4, 8)
OPTIONS = (0, 1, 2)

# (B, C, h, w, p) of the GPU cases -> what each is there for
GPU_CASES = {
    "one_window": (1, 8, 3, 3, 3),                 # nH = nW = 1
    "p2_odd_w": (2, 8, 4, 5, 2),
    "unaligned_rows": (1, 8, 5, 7, 3),             # block rows that start at odd multiples of 4 bytes
    "batch": (3, 16, 6, 6, 3),
    "p4_one_column": (1, 8, 9, 4, 4),              # nW = 1
    "many_per_thread_split": (1, 16, 34, 33, 3),   # 961 results per step: several per thread; the k' rows split at B = 1
    "wider_than_a_wave": (1, 8, 5, 70, 3),         # nW = 68: a second column per thread
    "one_range_no_merge": (8, 16, 12, 12, 3),      # split == 1: the partials are the merged values, no merge launch
}
FALLBACK_CASE = (1, 8, 4, 120, 3)                  # 3 * 120 * 120 floats: outside the LDS envelope
