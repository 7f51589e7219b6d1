#!/usr/bin/env python3
"""A/B of the data-pass C entries of csrc/conv_bf16.hip between two builds of libipsr_hip.so, on a machine WITHOUT a GPU.

    python tools/ab_conv_bf16_entries.py OLD/libipsr_hip.so NEW/libipsr_hip.so

Both libraries are loaded into this one process and get the same calls: the five launch entries (ipsr_conv3x3_bf16, its io = 2 route,
_packed, ipsr_conv4x4s2_bf16, ipsr_conv4x4s2_bf16x3) and the four workspace queries, on null and misaligned pointers, op / mode / io codes
-1 .. 6, zero and negative dimensions, widths 8 .. 512 with rows that do and do not divide, workspaces of 0, 255 and need - 1 bytes, and the
queries over a sweep of shapes.  No call passes both valid pointers and a sufficient workspace, so none reaches a HIP call (asserted: no
launch entry returns IPSR_OK); the pointers are made-up addresses.  Return codes, byte counts and ipsr_last_error() texts must be equal.
Before each call a sentinel message is set, so a call that sets no message shows as such.  Never run this where a GPU is visible.
"""
import ctypes
import itertools
import os
import sys
from ctypes import c_int, c_size_t, c_void_p

os.environ["HIP_VISIBLE_DEVICES"] = os.environ["ROCR_VISIBLE_DEVICES"] = "-1"
PTR = [c_void_p] * 3
SIGS = {
    "k3": ("ipsr_conv3x3_bf16", c_int, [c_int] + PTR + [c_int] * 6 + [c_void_p, c_size_t, c_void_p]),
    "k3p": ("ipsr_conv3x3_bf16_packed", c_int, [c_int] + PTR + [c_int] * 7 + [c_void_p, c_size_t, c_void_p]),
    "s2": ("ipsr_conv4x4s2_bf16", c_int, [c_int] + PTR + [c_int] * 6 + [c_void_p, c_size_t, c_void_p]),
    "s2x": ("ipsr_conv4x4s2_bf16x3", c_int, [c_int] + PTR + [c_int] * 5 + [c_void_p, c_size_t, c_void_p]),
    "k3_ws": ("ipsr_conv3x3_bf16_workspace_bytes", c_size_t, [c_int] * 6),
    "k3x_ws": ("ipsr_conv3x3_bf16x3_workspace_bytes", c_size_t, [c_int] * 6),
    "s2_ws": ("ipsr_conv4x4s2_bf16_workspace_bytes", c_size_t, [c_int] * 6),
    "s2x_ws": ("ipsr_conv4x4s2_bf16x3_workspace_bytes", c_size_t, [c_int] * 6),
}
A = 0x7F0000001000                                        # a made-up, 16-byte aligned address; nothing dereferences it on the host


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL)
    lib.ipsr_last_error.restype = ctypes.c_char_p
    for name, res, args in SIGS.values():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    lib.ipsr_conv3x3_bf16_wrw.restype = c_int
    lib.ipsr_conv3x3_bf16_wrw.argtypes = [c_int] + PTR + [c_int] * 5 + [c_void_p, c_size_t, c_void_p]
    return lib


def call(lib, key, args):
    lib.ipsr_conv3x3_bf16_wrw(-7, None, None, None, 1, 1, 1, 1, 1, None, 0, None)      # the sentinel: "form code -7"
    r = getattr(lib, SIGS[key][0])(*args)
    return r, lib.ipsr_last_error()


def launch_args(key, code, ptrs, dims, extra, ws_bytes):
    """(op | mode, in, w, out, five dims, io / out_bf16 [, pack_valid], ws, ws_bytes, stream)"""
    i, w, o, ws = ptrs
    return (code, i, w, o) + tuple(dims) + tuple(extra) + (ws, ws_bytes, None)


def need(lib, key, code, dims, extra):
    if key in ("k3", "k3p"):
        return getattr(lib, SIGS["k3x_ws" if extra[0] == 2 else "k3_ws"][0])(code, *dims)
    return getattr(lib, SIGS[key + "_ws"][0])(code, *dims)


def calls(new):
    """Yield (key, args).  dims: k3 (B, Cin, H, W, Cout), s2 (B, Kc, Cf, nh, nw)."""
    good = (A, A + 0x100000, A + 0x200000, A + 0x300000)
    extras = {"k3": [(0,), (1,), (2,)], "k3p": [(0, 0), (2, 1), (1, 1)], "s2": [(0,), (1,)], "s2x": [()]}
    dims0 = (2, 32, 16, 16, 48)
    for key, ex in extras.items():
        codes = (0, 1, 2, 3) if key in ("k3", "k3p") else (0, 1, 4, 5)
        for e in ex:
            # null and misaligned pointers
            for code, slot in itertools.product(codes, range(4)):
                for bad in (None,) if slot == 1 else (None, good[slot] + 2, good[slot] + 4, good[slot] + 8):      # the weight is read as scalars
                    p = list(good); p[slot] = bad
                    yield key, launch_args(key, code, p, dims0, e, 1 << 30)
            # op / mode / io codes, zero and negative dimensions: the workspace is too short for any accepted shape
            for code in range(-1, 7):
                yield key, launch_args(key, code, good, dims0, e, 0)
                for io in range(-1, 7):
                    if e:
                        yield key, launch_args(key, code, good, dims0, (io,) + e[1:], 255)
            for code, slot, v in itertools.product(codes, range(5), (0, -1, -16)):
                d = list(dims0); d[slot] = v
                yield key, launch_args(key, code, good, d, e, 0)
                yield key + "_ws" if key != "k3p" else "k3_ws", (code,) + tuple(d)
            # widths 8 .. 512, rows that do and do not divide, channels that are and are not a multiple of 16
            for code, W, H, (ca, cb), B in itertools.product(codes, range(8, 513, 8), (1, 2, 3, 4, 6, 16, 32), ((16, 16), (48, 80), (24, 64), (256, 64)), (1, 8)):
                if W & (W - 1) and (H != 4 or B != 1):
                    continue
                d = (B, ca, H, W, cb) if key in ("k3", "k3p") else (B, ca, cb, H, W)
                n = need(new, key, code, d, e)
                for ws_bytes in {0, 255, max(n - 1, 0)}:
                    yield key, launch_args(key, code, good, d, e, ws_bytes)
    # the queries over a sweep of shapes
    for q, B, (ca, cb), H, W in itertools.product(("k3_ws", "k3x_ws", "s2_ws", "s2x_ws"), (1, 2, 8, 16),
                                                  ((16, 16), (64, 64), (48, 80), (128, 64), (64, 128), (256, 256), (512, 512), (208, 48), (1024, 256), (24, 64)),
                                                  (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 64, 128, 256), (16, 32, 64, 128, 256)):
        for code in ((0, 1, 2, 3) if q.startswith("k3") else (0, 1, 4, 5)):
            yield q, (code, B, ca, H, W, cb) if q.startswith("k3") else (code, B, ca, cb, H, W)


def main(old_path, new_path):
    old, new = load(old_path), load(new_path)
    assert old._handle != new._handle, "the two paths name one library"
    n = diff = accepted = 0
    msgs, per = set(), {}
    for key, args in calls(new):
        a, b = call(old, key, args), call(new, key, args)
        n += 1
        per[key] = per.get(key, 0) + 1
        msgs.add(b[1])
        if key.endswith("_ws"):
            accepted += b[0] > 0
        else:
            assert a[0] != 0 and b[0] != 0, ("a launch entry returned IPSR_OK", key, args)
        if a != b:
            diff += 1
            if diff <= 10:
                print("DIFF", key, args, a, b)
    print("%d calls on each library %s" % (n, per))
    print("%d differ; %d distinct messages; %d accepted workspace queries" % (diff, len(msgs), accepted))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
