"""The Winograd cut override and its query on the host (no GPU needed: the library loads with every GPU hidden).

ipsr_debug_force_wino_split(nsplit, xi_split, nsplit_t) replaces wino_choose_split's rule for every following call
(wino_choose_split and the entry itself in csrc/winograd.hip); ipsr_wino_gemm_split reports the cut.  tests/test_gpu_wino_cuts.py relies on
both: a force must round-trip through the query, an out-of-range force must be refused with IPSR_ERR_INVALID (and leave the
previous state in place), and (0, 0, 0) must restore the automatic rule exactly.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(ROOT)
IPSR_ERR_INVALID = -1
# (rows, cols, reduction) at which the rule takes each of its branches: uncut, head/tail, uniform
PROBES = [(128, 128, 256), (512, 512, 512), (256, 512, 1024), (256, 2048, 256), (128, 128, 8192)]
# forces and the stage count they are queried at
FORCES = [((1, 36, 1), 5), ((2, 36, 2), 5), ((2, 36, 2), 8), ((3, 36, 3), 8), ((8, 36, 8), 8), ((1, 1, 3), 6), ((6, 1, 2), 6),
          ((3, 32, 1), 7), ((2, 35, 7), 7), ((4, 36, 4), 512)]
BAD = [(0, 36, 1), (1, 36, 0), (1, 0, 1), (1, 37, 1), (-1, 36, 1), (2, -3, 2), (0, 0, 1), (1, 0, 0)]


def _child():
    sys.path.insert(0, ROOT)
    from deepinpainting_amd import _lib
    L = _lib.lib()

    def q(rows, cols, red):
        out = (ctypes.c_int * 5)()
        rc = L.ipsr_wino_gemm_split(rows, cols, red, ctypes.cast(out, ctypes.c_void_p))
        return [rc] + list(out)

    res = {"auto": [q(*p) for p in PROBES], "forced": [], "bad": []}
    for (a, x, b), S in FORCES:
        rc = L.ipsr_debug_force_wino_split(a, x, b)
        res["forced"].append([rc, q(128, 128, 16 * S), [q(*p) for p in PROBES]])
    L.ipsr_debug_force_wino_split(3, 32, 1)
    for a, x, b in BAD:
        rc = L.ipsr_debug_force_wino_split(a, x, b)
        res["bad"].append([rc, L.ipsr_last_error().decode("utf-8", "replace"), q(128, 128, 16 * 7)])
    res["reset_rc"] = L.ipsr_debug_force_wino_split(0, 0, 0)
    res["after"] = [q(*p) for p in PROBES]
    print(json.dumps(res))


@pytest.fixture(scope="module")
def result():
    import __graft_entry__ as g
    g.build()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def _cdiv(a, b):
    return -(-a // b)


def test_forced_cuts_round_trip(result):
    for ((a, x, b), S), (rc, got, probes) in zip(FORCES, result["forced"]):
        assert rc == 0
        pa, pb = _cdiv(S, a), _cdiv(S, b)
        assert got == [0, _cdiv(S, pa), pa, x, _cdiv(S, pb), pb], ((a, x, b), S, got)
        # the force holds at every shape whose stage count admits it (the rule's own branches no longer apply)
        for (rows, cols, red), p in zip(PROBES, probes):
            St = red // 16
            if a <= St and b <= St:
                qa, qb = _cdiv(St, a), _cdiv(St, b)
                assert p == [0, _cdiv(St, qa), qa, x, _cdiv(St, qb), qb], ((a, x, b), (rows, cols, red), p)


def test_out_of_range_forces_are_refused(result):
    for (a, x, b), (rc, msg, got) in zip(BAD, result["bad"]):
        assert rc == IPSR_ERR_INVALID and "bad split" in msg, ((a, x, b), rc, msg)
        assert got == [0, 3, 3, 32, 1, 7], ((a, x, b), got)        # the force in place before the refused call still holds


def test_reset_restores_the_rule(result):
    assert result["reset_rc"] == 0
    assert result["after"] == result["auto"]
    assert all(p[0] == 0 for p in result["auto"])
    # the automatic answers themselves: uncut small grid, head/tail on 8 / 16 tiles, uniform elsewhere
    assert result["auto"][0][1:] == [1, 16, 36, 1, 16]
    assert result["auto"][1][3] == 32 and result["auto"][2][3] == 32
    assert result["auto"][3][3] == 36 and result["auto"][4][3] == 36 and result["auto"][4][1] > 1


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    _child()
