#!/usr/bin/env python3
"""A/B of the InnerCos C entries of csrc/api.hip between two builds of libipsr_hip.so, on a machine WITHOUT a GPU.

    python tools/ab_innercos_entries.py OLD/libipsr_hip.so NEW/libipsr_hip.so > profiles/innercos_unify_host.txt

Both libraries are loaded into this one process and get the same calls: the five entries (innercos_loss, _fused, _backward, _masks,
_backward_masks) on every refusal path — each pointer null in turn, each of x / target / mask misaligned by 4, 8 and 12 bytes, B / Cuse /
N of 0 and -1 and Cx < Cuse, mask_bstride of 0, N and six other values, a workspace of 0 bytes and one byte short — then every PAIR of
those faults in one call, which is what shows the ORDER of the checks; and innercos_workspace_bytes over a sweep of shapes.  No call
passes all of valid arguments and a sufficient workspace, so none reaches a HIP call (asserted for the loss entries: none returns
IPSR_OK; the backward entries, which take no workspace, are only called with a fault); the pointers are made-up addresses.  Return
codes, byte counts and ipsr_last_error() texts must be equal.  Before each call a sentinel message is set, so a call that sets no
message shows as such.  Never run this where a GPU is visible.
"""
import ctypes
import itertools
import os
import sys
from ctypes import c_float, c_int, c_size_t, c_void_p

os.environ["HIP_VISIBLE_DEVICES"] = os.environ["ROCR_VISIBLE_DEVICES"] = "-1"
HEAD = [c_void_p, c_int, c_int, c_int, c_int, c_void_p]                       # x, B, Cx, Cuse, N, mask
SIGS = {                                                                      # name: (argtypes, takes mask_bstride, loss pass, ticket)
    "innercos_loss": (HEAD + [c_void_p, c_float, c_void_p, c_void_p, c_size_t, c_void_p], False, True, False),
    "innercos_loss_fused": (HEAD + [c_void_p, c_float, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p], False, True, True),
    "innercos_loss_backward": (HEAD + [c_void_p, c_float, c_void_p, c_void_p, c_void_p], False, False, False),
    "innercos_loss_masks": (HEAD + [c_int, c_void_p, c_float, c_void_p, c_void_p, c_size_t, c_void_p], True, True, False),
    "innercos_loss_backward_masks": (HEAD + [c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p], True, False, False),
}
A = 0x7F0000001000                                        # a made-up, 16-byte aligned address; nothing dereferences it on the host
GOOD = dict(x=A, mask=A + 0x100000, target=A + 0x200000, out_a=A + 0x300000, out_b=A + 0x400000, ticket=A + 0x500000,
            B=2, Cx=12, Cuse=7, N=8, bstride=0, ws_short=0)


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL)
    lib.ipsr_last_error.restype = ctypes.c_char_p
    for name, (args, _, _, _) in SIGS.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = c_int, args
    lib.innercos_workspace_bytes.restype, lib.innercos_workspace_bytes.argtypes = c_size_t, [c_int] * 3
    lib.ipsr_patch_normalize.restype, lib.ipsr_patch_normalize.argtypes = c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
    return lib


def call(lib, name, v):
    """v: GOOD with faults put in.  out_a / out_b: loss and workspace, or grad_loss and grad_x.  ws_short: bytes missing (None: 0 given)."""
    _, strided, loss_pass, ticket = SIGS[name]
    lib.ipsr_patch_normalize(None, 0, 0, 0, None, None, None)                 # the sentinel: another entry's refusal
    args = [v["x"], v["B"], v["Cx"], v["Cuse"], v["N"], v["mask"]] + ([v["bstride"]] if strided else []) + [v["target"], 1.0, v["out_a"], v["out_b"]]
    if loss_pass:
        need = lib.innercos_workspace_bytes(v["B"], v["Cuse"], v["N"])
        args.append(0 if v["ws_short"] is None else need - v["ws_short"])
        if ticket:
            args.append(v["ticket"])
    r = getattr(lib, name)(*(args + [None]))
    return r, lib.ipsr_last_error()


def faults(name):
    """{label: {field: value}}, each a single reason for the entry to refuse."""
    _, strided, loss_pass, ticket = SIGS[name]
    f = {}
    for p in ("x", "mask", "target", "out_a", "out_b") + (("ticket",) if ticket else ()):
        f["null " + p] = {p: None}
    for p, off in itertools.product(("x", "target", "mask"), (4, 8, 12)):     # refused by the loss entries, taken by the backward entries
        if loss_pass:
            f["%s + %d" % (p, off)] = {p: GOOD[p] + off}
    for d, bad in itertools.product(("B", "Cuse", "N"), (0, -1)):
        f["%s = %d" % (d, bad)] = {d: bad}
    f["Cx < Cuse"] = {"Cx": GOOD["Cuse"] - 1}
    if strided:
        for s in (1, -1, GOOD["N"] - 1, GOOD["N"] + 1, 2 * GOOD["N"], -GOOD["N"]):
            f["bstride %d" % s] = {"bstride": s}
    if loss_pass:
        f["workspace 1 short"] = {"ws_short": 1}
        f["workspace 0"] = {"ws_short": None}
    return f


def calls():
    for name in SIGS:
        _, strided, loss_pass, _ = SIGS[name]
        f = faults(name)
        strides = (0, GOOD["N"]) if strided else (0,)
        for s in strides:                                  # every fault, and every pair of faults, under both accepted strides
            for k in f:
                yield name, {**GOOD, "bstride": s, **f[k]}
            for k1, k2 in itertools.combinations(f, 2):
                yield name, {**GOOD, "bstride": s, **f[k1], **f[k2]}


def main(old_path, new_path):
    old, new = load(old_path), load(new_path)
    assert old._handle != new._handle, "the two paths name one library"
    n = diff = 0
    msgs, per, codes = set(), {}, {}
    for name, v in calls():
        a, b = call(old, name, v), call(new, name, v)
        assert a[0] != 0 and b[0] != 0, ("an entry returned IPSR_OK", name, v)
        n += 1
        per[name] = per.get(name, 0) + 1
        codes[b[0]] = codes.get(b[0], 0) + 1
        msgs.add(b[1])
        if a != b:
            diff += 1
            if diff <= 10:
                print("DIFF", name, v, a, b)
    q = qdiff = 0
    for B, C, N in itertools.product((-1, 0, 1, 2, 8, 64), (-1, 0, 1, 7, 512, 4097), (-1, 0, 1, 15, 1024, 65536)):
        q += 1
        qdiff += old.innercos_workspace_bytes(B, C, N) != new.innercos_workspace_bytes(B, C, N)
    print("%d refused calls on each library %s" % (n, per))
    print("return codes of the new library %s; %d distinct messages" % (dict(sorted(codes.items())), len(msgs)))
    print("%d calls differ in return code or message" % diff)
    print("%d innercos_workspace_bytes queries, %d differ" % (q, qdiff))
    return 1 if diff or qdiff else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
