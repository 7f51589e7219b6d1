"""The host-side plans of csrc/winograd.hip and csrc/smallmap.hip, pinned (no GPU needed: every call is a query).

tests/golden/wino_plan_pins.json holds arguments and results of the five workspace queries (3x3, 3x3 weight gradient, 4x4 on 3x3
tiles with geometry 0 / 1 x mode 0..2, 4x4 stride 2 x mode 0..2, small maps), of ipsr_conv3x3_winograd_filter_floats and of
ipsr_wino_gemm_split.  The values were recorded from the library of the commit BEFORE the four Winograd planners became one
(wino_plan_gemm), not from the code under test, so the file keeps the differential check of that refactor alive now that the old
library is gone (`tools/wino_host_ab.py pins OLD.so OUT.json` wrote it; its `sweep` is the full comparison).  The shapes sit on the
boundaries of the plan rule: produced channels 63 / 64 / 65 / 128 / 129 (both values of wino_rows_padded), reduction channels 15 / 16 / 24 and a cut of 129 stages, tile counts either side of 128 and 256, odd and too small
extents, nh / nw of 1, 4, 5, 6, 40, 41, 80, 81, every branch of wino_choose_split, refused codes; then a quarter of them again under
two forced cuts.  A byte count pins the padded rows and columns, the reduction and the slab count of the cut together.
"""
import ctypes
import json
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deepinpainting_amd import _lib
    return _lib.lib()


def _ask(lib, fn, args):
    if fn == "ipsr_wino_gemm_split":
        out = (ctypes.c_int * 5)(-7, -7, -7, -7, -7)
        return [lib.ipsr_wino_gemm_split(*args, ctypes.cast(out, ctypes.c_void_p))] + list(out)
    return getattr(lib, fn)(*args)


def test_plans_match_the_values_recorded_before_the_planners_were_unified(lib, golden_dir):
    with open(os.path.join(golden_dir, "wino_plan_pins.json")) as fh:
        pins = json.load(fh)
    bad, n, answered = [], 0, 0
    try:
        for sec in pins["sections"]:
            assert lib.ipsr_debug_force_wino_split(*(sec["force"] or (0, 0, 0))) == 0
            for fn, calls in sec["calls"].items():
                for args, want in calls:
                    got = _ask(lib, fn, args)
                    n += 1
                    answered += (want[0] == 0) if isinstance(want, list) else (want > 0)
                    if got != want:
                        bad.append((sec["force"], fn, args, got, want))
    finally:
        lib.ipsr_debug_force_wino_split(0, 0, 0)
    print("%d pins, %d of them answered (the others are refusals), %d mismatches" % (n, answered, len(bad)))
    assert n == pins["entries"] and n > 1000 and answered > 600 and n - answered > 300, (n, answered)
    assert len(pins["sections"]) == 3 and [s["force"] for s in pins["sections"]] == [None, [2, 36, 2], [3, 32, 1]]
    assert not bad, bad[:10]
