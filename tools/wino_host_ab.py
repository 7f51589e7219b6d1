"""Differential check of the host side of csrc/winograd.hip and csrc/smallmap.hip against another build of the library.

    wino_host_ab.py sweep OLD.so NEW.so   both libraries are loaded side by side and called with the same arguments: the five workspace
                                          queries, ipsr_conv3x3_winograd_filter_floats, ipsr_wino_gemm_split and the refusal paths of the
                                          four _mp entries and ipsr_conv_smallmap, under the automatic cut and two forced ones.  Return
                                          codes, byte counts and ipsr_last_error() texts are compared; the counts are printed
                                          (profiles/winograd_plan_refactor_ab.txt).  Exit status 1 if anything differs.
    wino_host_ab.py pins OLD.so OUT.json  records tests/golden/wino_plan_pins.json (tests/test_wino_plan_pins.py) from OLD.so

Run it with every GPU hidden (HIP_VISIBLE_DEVICES=-1): the pointers are fake device addresses and every launcher call is built to be
refused before any HIP call; a library that lost a check then fails to launch instead of launching on them.
"""
import collections, ctypes, itertools, json, re, sys
from ctypes import c_int, c_size_t, c_void_p

I, P, Z = c_int, c_void_p, c_size_t
SIG = {
    "ipsr_last_error": (ctypes.c_char_p, []),
    "ipsr_conv3x3_winograd_workspace_bytes": (Z, [I] * 6),
    "ipsr_conv3x3_winograd_filter_floats": (Z, [I] * 3),
    "ipsr_conv3x3_winograd_wrw_workspace_bytes": (Z, [I] * 6),
    "ipsr_conv4x4_winograd_workspace_bytes": (Z, [I] * 7),
    "ipsr_conv4x4s2_winograd_workspace_bytes": (Z, [I] * 6),
    "ipsr_conv_smallmap_workspace_bytes": (Z, [I] * 12),
    "ipsr_conv_smallmap": (I, [I, P, P, P] + [I] * 11 + [P, Z, P]),
    "ipsr_conv3x3_winograd_mp": (I, [I, P, P, P, I, P, I, P, I, I, I, I, I, I, I, P, Z, P]),
    "ipsr_conv3x3_winograd_wrw_mp": (I, [I, P, P, P, I, I, I, I, I, I, I, P, Z, P]),
    "ipsr_conv4x4_winograd_mp": (I, [I, I, P, P, P, I, I, I, I, I, I, I, P, Z, P]),
    "ipsr_conv4x4s2_winograd_mp": (I, [I, P, P, P, I, I, I, I, I, I, I, P, Z, P]),
    "ipsr_wino_gemm_split": (I, [I, I, I, P]),
    "ipsr_debug_force_wino_split": (I, [I, I, I]),
}
A = lambda slot: (1 << 40) + slot * (1 << 24)          # fake device addresses
CH = [15, 16, 24, 63, 64, 65, 128, 129, 256, 512, 1024, 2048, 2064]
CH_S = [16, 24, 64, 65, 128, 129, 512]                 # for the launcher refusals (accepted reductions and not)


class Run:
    """Calls the parent's library and the new one with the same arguments, one after the other, and compares as it goes."""
    def __init__(self, parent, new):
        self.libs = []
        for path in (parent, new):
            L = ctypes.CDLL(path)
            for n, (r, a) in SIG.items():
                f = getattr(L, n); f.restype = r; f.argtypes = a
            self.libs.append(L)
        # the two libraries are separate images with separate state: a message set in one does not show in the other
        self.libs[0].ipsr_debug_force_wino_split(-1, -1, -1)
        self.libs[1].ipsr_wino_gemm_split(0, 0, 0, None)
        m0, m1 = (L.ipsr_last_error().decode() for L in self.libs)
        assert "bad split" in m0 and "ipsr_wino_gemm_split" in m1, (m0, m1)
        self.section = None
        self.n = collections.Counter(); self.diffs = []; self.msgs = set(); self.accepted = collections.Counter(); self.rcs = collections.Counter()

    def force(self, f):
        for L in self.libs:
            assert L.ipsr_debug_force_wino_split(*(f or (0, 0, 0))) == 0

    def record(self, fn, args, res):
        self.n[(self.section, fn)] += 1
        if res[0] != res[1]:
            self.diffs.append((self.section, fn, args, res))
        r, e = res[0]
        self.msgs.add(e)
        if fn.endswith("workspace_bytes") and r > 0:
            self.accepted[fn] += 1
        if fn.endswith("_mp") or fn == "ipsr_conv_smallmap":
            self.rcs[(fn, r)] += 1

    def call(self, fn, *args):
        res = []
        for L in self.libs:
            L.ipsr_wino_gemm_split(0, 0, 0, None)       # sentinel message: a call that sets none shows
            r = getattr(L, fn)(*args)
            res.append((r, L.ipsr_last_error().decode("utf-8", "replace")))
        self.record(fn, args, res)
        return res[0]

    def split(self, rows, cols, red, null=False):
        res = []
        for L in self.libs:
            o = (c_int * 5)(-7, -7, -7, -7, -7)
            L.ipsr_debug_force_wino_split(-9, -9, -9)   # sentinel
            r = L.ipsr_wino_gemm_split(rows, cols, red, None if null else ctypes.cast(o, c_void_p))
            res.append((tuple([r] + list(o)), L.ipsr_last_error().decode("utf-8", "replace")))
        self.record("ipsr_wino_gemm_split", (rows, cols, red, null), res)


def need_of(msg):
    m = re.search(r"workspace \d+ < (\d+)", msg)
    return int(m.group(1)) if m else None


def sweep(R, full):
    c = R.call
    # ---- queries -------------------------------------------------------------------------------------------------------------------
    HW3 = [(1, 1), (4, 4), (5, 7), (32, 32), (44, 44), (32, 64), (4, 516), (44, 48), (45, 45), (64, 60), (64, 64), (64, 68), (128, 128), (0, 4), (4, -1)]
    for op in range(-1, 5):
        for B in (1, 2):
            for ci in CH:
                for co in CH:
                    for h, w in HW3:
                        c("ipsr_conv3x3_winograd_workspace_bytes", op, B, ci, h, w, co)
    for tr in (0, 1, 2):
        for B in (0, 1, 2):
            for ci in CH + [0]:
                for co in CH + [-1]:
                    for h, w in HW3:
                        c("ipsr_conv3x3_winograd_wrw_workspace_bytes", tr, B, ci, h, w, co)
    for op in range(-1, 5):
        for ci in CH + [0, -1, 1]:
            for co in CH + [0, -1, 1]:
                c("ipsr_conv3x3_winograd_filter_floats", op, ci, co)
    HW4 = [(1, 4), (2, 2), (3, 3), (3, 8), (4, 3), (4, 4), (5, 5), (6, 6), (7, 8), (16, 16), (32, 32), (33, 33), (34, 34), (46, 46), (48, 48), (50, 50),
           (64, 64), (66, 66), (68, 68), (90, 90), (92, 96), (96, 96), (98, 98), (128, 128), (130, 130), (0, 8), (8, -2)]
    for geom in range(-1, 3):
        for mode in range(-1, 4):
            for B in (1, 2):
                for ci in CH:
                    for co in CH:
                        for h, w in HW4:
                            c("ipsr_conv4x4_winograd_workspace_bytes", geom, mode, B, ci, h, w, co)
    NS = [1, 4, 5, 6, 9, 10, 11, 16, 32, 40, 41, 55, 56, 57, 64, 75, 79, 80, 81, 0, -1]
    KC = [15, 16, 24, 63, 64, 65, 128, 129, 512, 2048]
    CF = [3, 4, 6, 8, 15, 16, 17, 32, 33, 64, 128, 512]
    for mode in range(-1, 4):
        for B in (1, 2, 8):
            for kc in KC:
                for cf in CF:
                    for nh in NS:
                        for nw in (nh, 5, 40):
                            c("ipsr_conv4x4s2_winograd_workspace_bytes", mode, B, kc, cf, nh, nw)
    GEO = [(4, 2, 1, 1), (3, 1, 1, 1), (4, 2, 3, 2), (4, 1, 1, 1), (5, 1, 1, 1), (0, 1, 1, 1), (4, 3, 1, 1), (4, 0, 1, 1), (4, 2, -1, 1), (4, 2, 1, 0), (1, 1, 0, 1)]
    for op in range(-1, 4):
        for B in (1, 2, 3, 8, 0):
            for r in (32, 48, 64, 96, 512, 1024, 0):
                for cq in (8, 20, 32, 128, 512, 0):
                    for hf, wf in ((1, 1), (2, 2), (3, 3), (4, 4), (6, 6), (8, 8), (12, 12), (16, 16), (18, 14), (20, 20), (32, 32), (32, 34), (64, 64), (0, 4)):
                        for k, st, pad, dil in GEO:
                            ho = (hf + 2 * pad - dil * (k - 1) - 1) // st + 1 if st else 1
                            wo = (wf + 2 * pad - dil * (k - 1) - 1) // st + 1 if st else 1
                            c("ipsr_conv_smallmap_workspace_bytes", op, B, r, cq, ho, wo, hf, wf, k, st, pad, dil)
                            if (hf, wf) in ((4, 4), (18, 14)):
                                c("ipsr_conv_smallmap_workspace_bytes", op, B, r, cq, ho + 1, wo, hf, wf, k, st, pad, dil)
    for rows in (0, -128, 64, 128, 130, 256, 512, 1024, 2048):
        for cols in (0, 100, 128, 256, 384, 512, 1024, 2048, 4096, 8192):
            for red in (0, 15, 16, 24, 32, 48, 64, 128, 256, 496, 512, 528, 1024, 2048, 2064, 4096, 8192, 65536):
                R.split(rows, cols, red)
    R.split(128, 128, 256, null=True)
    if not full:
        return
    # ---- refusal paths of the launchers (fake addresses; every call must be refused) ------------------------------------------------------
    BIG = 1 << 40

    def refusals(fn, mk, ptrs, need_fn, ptr_tests):
        """mk(ptr dict, math, io, ws_bytes) -> args.  ptrs: names in slot order."""
        base = {n: A(i) for i, n in enumerate(ptrs)}
        for math, io in ((0, 0), (2, 0), (3, 0), (0, 3), (2, 1), (3, 2)):
            r, e = c(fn, *mk(base, math, io, 0))
            n = need_of(e)
            if r == -3 and n:
                c(fn, *mk(base, math, io, n - 1))
                c(fn, *mk(base, math, io, 255))
            need_fn(base, math, io, r, n)
        for math in (-1, 1, 4):
            c(fn, *mk(base, math, 0, BIG))
        for io in (-1, 4):
            c(fn, *mk(base, 0, io, BIG))
        if not ptr_tests:
            return
        for n in ptrs:                                   # ws_bytes 0: a pointer that no entry checks is refused by the workspace check
            c(fn, *mk(dict(base, **{n: None}), 0, 0, 0))
            for off in (2, 4, 8):
                c(fn, *mk(dict(base, **{n: base[n] + off}), 0, 0, 0))
                c(fn, *mk(dict(base, **{n: base[n] + off}), 2, 3, 0))

    none = lambda *a: None
    # 3x3 data passes
    for op in range(-1, 5):
        for B, h, w in ((1, 4, 4), (2, 16, 16), (1, 15, 16), (2, 16, 17), (1, 44, 48), (1, 64, 64), (1, 64, 68), (0, 8, 8), (1, 0, 8), (1, 8, -4)):
            for ci in CH_S + [0, -16]:
                for co in CH_S:
                    def mk(p, math, io, wsb, epi=0, fcv=0):
                        return (op, p["in"], p["weight"], p["bias"], epi, p["filter_cache"], fcv, p["out"], B, ci, h, w, co, math, io, p["ws"], wsb, None)

                    def epis(p, math, io, r, n):
                        if r != -3 or not n:
                            return
                        for epi in (-1, 1, 2, 3):
                            if epi in (1,) or (epi == 2 and not ((h | w) & 1)):
                                c("ipsr_conv3x3_winograd_mp", *mk(p, math, io, n - 1, epi))       # accepted epilogue: only with a short workspace
                            else:
                                c("ipsr_conv3x3_winograd_mp", *mk(p, math, io, n, epi))           # refused epilogue on an exact workspace
                                c("ipsr_conv3x3_winograd_mp", *mk(p, math, io, n - 1, epi))       # the workspace message comes first
                    refusals("ipsr_conv3x3_winograd_mp", mk, ["in", "weight", "out", "ws", "filter_cache", "bias"], epis, (ci, co) == (64, 128))
    # 3x3 weight gradient
    for tr in (0, 1):
        for B, h, w in ((1, 4, 4), (2, 16, 16), (1, 15, 17), (1, 44, 48), (1, 64, 64), (2, 64, 68), (0, 8, 8), (1, -8, 8)):
            for ci in CH_S + [15, 0]:
                for co in CH_S + [15]:
                    mk = lambda p, math, io, wsb: (tr, p["x"], p["dy"], p["dw"], B, ci, h, w, co, math, io, p["ws"], wsb, None)
                    refusals("ipsr_conv3x3_winograd_wrw_mp", mk, ["x", "dy", "dw", "ws"], none, (ci, co) == (64, 128))
    # 4x4 on 3x3 tiles
    for geom in range(-1, 3):
        for mode in range(-1, 4):
            for B, h, w in ((1, 4, 4), (1, 3, 8), (1, 7, 8), (2, 16, 16), (1, 34, 34), (1, 64, 64), (1, 68, 68), (2, 96, 96), (1, 1, 8), (0, 8, 8)):
                for ci in CH_S + [0]:
                    for co in CH_S:
                        mk = lambda p, math, io, wsb: (geom, mode, p["a"], p["b"], p["out"], B, ci, h, w, co, math, io, p["ws"], wsb, None)
                        refusals("ipsr_conv4x4_winograd_mp", mk, ["a", "b", "out", "ws"], none, (ci, co) == (64, 128))
    # 4x4 stride 2
    for mode in range(-1, 4):
        for B, nh, nw in ((1, 1, 1), (2, 4, 4), (1, 5, 5), (2, 6, 6), (8, 4, 5), (2, 40, 40), (2, 40, 41), (1, 80, 80), (1, 81, 80), (1, 0, 4), (0, 4, 4)):
            for kc in (15, 16, 24, 64, 65, 128, 512):
                for cf in (3, 4, 6, 8, 16, 32, 33, 128, 0):
                    mk = lambda p, math, io, wsb: (mode, p["a"], p["b"], p["out"], B, kc, cf, nh, nw, math, io, p["ws"], wsb, None)
                    refusals("ipsr_conv4x4s2_winograd_mp", mk, ["a", "b", "out", "ws"], none, (kc, cf) == (64, 32))
    # small maps
    base = {n: A(i) for i, n in enumerate(["a", "b", "out", "ws"])}
    for op in range(-1, 4):
        for B in (1, 2, 8, 0):
            for r in (32, 48, 512):
                for cq in (8, 20, 128):
                    for hf, wf in ((2, 2), (4, 4), (8, 8), (18, 14), (32, 32), (32, 34)):
                        for k, st, pad, dil in GEO:
                            ho = (hf + 2 * pad - dil * (k - 1) - 1) // st + 1 if st else 1
                            wo = (wf + 2 * pad - dil * (k - 1) - 1) // st + 1 if st else 1
                            mk = lambda p, wsb, dho=0: (op, p["a"], p["b"], p["out"], B, r, cq, ho + dho, wo, hf, wf, k, st, pad, dil, p["ws"], wsb, None)
                            rc, e = c("ipsr_conv_smallmap", *mk(base, 0))
                            n = need_of(e)
                            if rc == -3 and n:
                                c("ipsr_conv_smallmap", *mk(base, n - 1))
                            c("ipsr_conv_smallmap", *mk(base, 0, 1))
    for n in base:
        mk = lambda p: (2, p["a"], p["b"], p["out"], 2, 128, 128, 4, 4, 8, 8, 4, 2, 1, 1, p["ws"], 0, None)
        c("ipsr_conv_smallmap", *mk(dict(base, **{n: None})))
        for off in (4, 8):
            c("ipsr_conv_smallmap", *mk(dict(base, **{n: base[n] + off})))


def main(parent, new):
    R = Run(parent, new)
    secs = [("automatic", None), ("force 2,36,2", (2, 36, 2)), ("force 3,32,1", (3, 32, 1))]
    try:
        for name, f in secs:
            R.section = name
            R.force(f)
            sweep(R, full=True)
        R.section = "after reset"
        R.force(None)
        sweep(R, full=False)
    finally:
        R.force(None)
    total = sum(R.n.values())
    for d in R.diffs[:10]:
        print("DIFF", d)
    print("calls made to each library: %d   differing in return code, byte count or message: %d   distinct messages: %d" % (total, len(R.diffs), len(R.msgs)))
    names = [s[0] for s in secs] + ["after reset"]
    print("%-42s %10s %13s %13s %12s   %s" % ("entry", *names, "queries answered > 0"))
    for fn in sorted({k[1] for k in R.n}):
        print("%-42s %10d %13d %13d %12d   %s" % (fn, *[R.n[(s, fn)] for s in names], R.accepted.get(fn, "")))
    print("return codes of the launcher entries (0 = IPSR_OK must not occur: every call is refused before any HIP call):")
    for fn in sorted({k[0] for k in R.rcs}):
        print("  %-34s %s" % (fn, "   ".join("%d: %d" % (rc, cnt) for (f2, rc), cnt in sorted(R.rcs.items()) if f2 == fn)))
    return len(R.diffs)


def pin_queries():
    P = itertools.product
    q = []
    HW = [(5, 7), (44, 44), (44, 48), (64, 64), (64, 68)]                    # 4, 121, 132, 256, 272 tiles of 4x4
    for prod, red, (h, w) in P((63, 64, 65, 128, 129), (15, 16, 24, 256, 2048, 2064), HW):
        q.append(("ipsr_conv3x3_winograd_workspace_bytes", (0, 1, red, h, w, prod)))
    for op, B in P((-1, 1, 2, 3, 4), (1, 2)):
        q.append(("ipsr_conv3x3_winograd_workspace_bytes", (op, B, 64, 32, 32, 512)))
    q.append(("ipsr_conv3x3_winograd_workspace_bytes", (0, 1, 64, 0, 32, 64)))
    for tr, ci, co, (h, w) in P((0, 1), (63, 64, 65, 129), (64, 128), HW):
        q.append(("ipsr_conv3x3_winograd_wrw_workspace_bytes", (tr, 1, ci, h, w, co)))
    q.append(("ipsr_conv3x3_winograd_wrw_workspace_bytes", (0, 0, 64, 8, 8, 64)))
    for op, ci, co in P((-1, 0, 1, 4), (0, 15, 64, 129), (1, 63, 128)):
        q.append(("ipsr_conv3x3_winograd_filter_floats", (op, ci, co)))
    CC = [(16, 64), (24, 65), (15, 128), (64, 16), (129, 256), (512, 512)]
    for geom, mode, (ci, co), (h, w) in P((0, 1), (0, 1, 2), CC, ((3, 8), (7, 8), (32, 32), (66, 66), (68, 68), (96, 96), (98, 98))):
        q.append(("ipsr_conv4x4_winograd_workspace_bytes", (geom, mode, 1, ci, h, w, co)))
    for geom, mode in ((-1, 0), (2, 0), (0, -1), (0, 3)):
        q.append(("ipsr_conv4x4_winograd_workspace_bytes", (geom, mode, 1, 64, 32, 32, 64)))
    KF = [(16, 4), (24, 6), (15, 3), (64, 16), (65, 33), (128, 32), (512, 128)]
    for mode, (kc, cf), (B, nh, nw) in P((0, 1, 2), KF, ((1, 1, 1), (2, 4, 4), (1, 5, 5), (2, 6, 6), (2, 40, 40), (2, 40, 41), (1, 80, 80), (1, 81, 80))):
        q.append(("ipsr_conv4x4s2_winograd_workspace_bytes", (mode, B, kc, cf, nh, nw)))
    for mode in (-1, 3):
        q.append(("ipsr_conv4x4s2_winograd_workspace_bytes", (mode, 2, 64, 16, 8, 8)))
    for op, (B, r, cq, hf, wf), (k, st, pad, dil) in P((0, 1, 2), ((1, 32, 8, 4, 4), (8, 512, 512, 8, 8), (2, 48, 32, 18, 14), (3, 96, 128, 6, 6), (4, 64, 8, 32, 34)),
                                                      ((4, 2, 1, 1), (3, 1, 1, 1), (4, 2, 3, 2))):
        ho, wo = (hf + 2 * pad - dil * (k - 1) - 1) // st + 1, (wf + 2 * pad - dil * (k - 1) - 1) // st + 1
        q.append(("ipsr_conv_smallmap_workspace_bytes", (op, B, r, cq, ho, wo, hf, wf, k, st, pad, dil)))
    q.append(("ipsr_conv_smallmap_workspace_bytes", (3, 1, 32, 8, 2, 2, 4, 4, 4, 2, 1, 1)))
    q.append(("ipsr_conv_smallmap_workspace_bytes", (0, 1, 32, 8, 3, 2, 4, 4, 4, 2, 1, 1)))
    for rows, cols, red in P((128, 512, 1024), (128, 256, 512, 2048), (16, 256, 512, 2048, 2064, 8192)):
        q.append(("ipsr_wino_gemm_split", (rows, cols, red)))
    for a in ((0, 128, 16), (64, 128, 16), (128, 100, 16), (128, 128, 24)):
        q.append(("ipsr_wino_gemm_split", a))
    return q


def pins(old, out):
    L = ctypes.CDLL(old)
    for n, (r, a) in SIG.items():
        f = getattr(L, n); f.restype = r; f.argtypes = a

    def ask(fn, args):
        if fn == "ipsr_wino_gemm_split":
            o = (c_int * 5)(-7, -7, -7, -7, -7)
            return [L.ipsr_wino_gemm_split(*args, ctypes.cast(o, c_void_p))] + list(o)
        return getattr(L, fn)(*args)

    sections, Q = [], pin_queries()
    try:
        for force in (None, (2, 36, 2), (3, 32, 1)):
            assert L.ipsr_debug_force_wino_split(*(force or (0, 0, 0))) == 0
            qs = Q if force is None else [c for i, c in enumerate(Q) if i % 4 == 0 and "smallmap" not in c[0] and "filter_floats" not in c[0]]
            calls = {}
            for fn, args in qs:
                calls.setdefault(fn, []).append([list(args), ask(fn, args)])
            sections.append({"force": force, "calls": calls})
    finally:
        L.ipsr_debug_force_wino_split(0, 0, 0)
    n = sum(len(v) for s in sections for v in s["calls"].values())
    doc = {"recorded_from": "the library of the commit before winograd.hip's planners were unified (4cae96b)", "entries": n, "sections": sections}
    s = json.dumps(doc, separators=(",", ":")).replace('{"force"', '\n{"force"').replace('],[[', '],\n[[')
    open(out, "w").write(s + "\n")
    print(n, "pins,", len(s), "bytes")


if __name__ == "__main__":
    if sys.argv[1] == "sweep":
        sys.exit(1 if main(sys.argv[2], sys.argv[3]) else 0)
    pins(sys.argv[2], sys.argv[3])
