"""The edges of what the convolution dispatcher (models/hipconv.py) admits: each engine's own support query for one pass of one layer
(`takes`), and the corner table `ROWS` — elongated maps, batches 1 and 3, every rule's minimum channel counts — with the three engines each
row is expected to reach.  A plain module (like golden_cases.py), shared by tests/test_dispatch_envelope.py (host logic and workspace
probes, no GPU) and tests/test_gpu_dispatch_envelope.py (every row through `conv_nobias` and autograd against fp64).

The geometry arguments of every query are built with the dispatcher's own helpers, the ones the records of `hipconv._ENGINES` call, so the
mapping here cannot drift from what an engine is really asked to run.
"""
import contextlib
from collections import namedtuple

K3, S2, DIL, K4S1 = (3, 1, 1, 1), (4, 2, 1, 1), (4, 2, 3, 2), (4, 1, 1, 1)      # (k, stride, pad, dil)
OPT_IN_MATH = "direct_bf16x3_s2_dw"                                           # the widest of ops.DIRECT_PASSES
# `switches` name -> (set_direct_dilated_bf16, set_direct_dilated_bf16_dw): the two dilated switches for bf16 activations
BF16_DIL_SWITCHES = {"bf16_dil_data": (True, False), "bf16_dil_dw": (False, True), "bf16_dil": (True, True)}


def out_extents(lay):
    """(Ho, Wo) of the module's output, as torch computes them (no output padding)."""
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    if transposed:
        return tuple((n - 1) * stride - 2 * pad + dil * (k - 1) + 1 for n in (H, W))
    return tuple((n + 2 * pad - dil * (k - 1) - 1) // stride + 1 if n + 2 * pad - dil * (k - 1) - 1 >= 0 else 0 for n in (H, W))


def torch_accepts(lay):
    return min(out_extents(lay)) >= 1


def passes(lay):
    """The three passes of a layer as (kind, op): forward, input gradient, weight gradient."""
    from deepinpainting_amd import ops
    fop, bop = (ops.CONVT_FWD, ops.CONVT_BWD_DATA) if lay[0] else (ops.CONV_FWD, ops.CONV_BWD_DATA)
    return (("data", fop), ("data", bop), ("wrw", None))


def takes(engine, kind, op, lay, bf16):
    """The engine's own support query for one pass of one layer.  lay = the dispatcher's tuple (transposed, B, Cin, H, W, Cout, k, stride,
    pad, dil); kind "data" (op = the ops.* code of the forward / input-gradient pass) or "wrw" (op ignored).  An engine without such a pass,
    or a geometry its call cannot express, answers False."""
    from deepinpainting_amd import _lib, ops
    from deepinpainting_amd.models import hipconv as hc
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    geom = (k, stride, pad, dil)
    data = kind == "data"
    assert kind in ("data", "wrw") and (not data or op in ((ops.CONVT_FWD, ops.CONVT_BWD_DATA) if transposed else (ops.CONV_FWD, ops.CONV_BWD_DATA)))
    rec = hc._ENGINES[engine]
    if (rec.data if data else rec.wrw) is None:
        return False
    if engine == "winograd":
        if geom != K3:
            return False
        if data:
            return ops.winograd_supported(op, B, Cin, H, W, Cout)
        return _lib.lib().ipsr_conv3x3_winograd_wrw_workspace_bytes(int(transposed), B, Cin, H, W, Cout) > 0      # (no ops.*_supported)
    if engine == "wino_dil":
        g = ops.conv4x4_geometry(*geom)
        if g is None or transposed:
            return False
        return ops.dilated_winograd_supported(int(op != ops.CONV_FWD) if data else 2, B, Cin, H, W, Cout, geom=g)
    if engine == "wino_s2":
        g = hc._s2_geometry(lay)
        return g is not None and ops.s2_winograd_supported(hc._s2_mode(op) if data else ops.S2_WEIGHT_GRAD, B, *g)
    if engine == "thin":
        return geom == K3 and ops.thin_supported(op, Cin, H, W, Cout)
    if engine == "thin_f2m":
        return (pad, dil) == (1, 1) and ops.thin_f2m_mfma_supported(op, B, Cin, H, W, Cout, k, stride)
    if engine == "thin_mfma":
        return (pad, dil) == (1, 1) and ops.thin_wrw_mfma_supported(transposed, B, Cin, H, W, Cout, k, stride)
    if engine == "smallmap":
        return ops.smallmap_supported(hc._smallmap_op(op) if data else ops.SM_WRW, *hc._smallmap_geometry(lay))
    if engine == "direct":
        return ops.conv2d_supported(op, B, Cin, H, W, Cout, k, stride, pad, dil)
    if engine == "one":
        return not transposed and Cout == 1 and (not data or op == ops.CONV_FWD) and ops.conv_to_one_supported(B, Cin, H, W, k, stride, pad, dil)
    if engine in ("bf16d", "bf16x3d", "bf16x3w"):                # by geometry: k3; k4 s2 p1; dilated ("bf16d": each kind under its own switch)
        x3 = engine != "bf16d"
        if x3 == bool(bf16):
            return False             # "bf16d" reads bf16 activations, the split-bf16 pair fp32 ones
        if geom == K3:
            if data:
                return (ops.conv3x3_bf16x3_supported if x3 else ops.conv3x3_bf16_supported)(op, B, Cin, H, W, Cout)
            return (ops.conv3x3_bf16x3_wrw_supported if x3 else ops.conv3x3_bf16_wrw_supported)(transposed, B, Cin, H, W, Cout)
        if hc._is_dilated4(*geom):
            g = hc._dil_geometry(lay)
            if g is None:
                return False
            if x3:                   # the split-bf16 pair answers whatever `set_direct_dilated` / `set_direct_dilated_dw` say
                return ops.conv4x4s2_bf16x3_supported(hc._dil_mode(op), B, *g) if data else ops.conv4x4s2_bf16x3_dil_wrw_supported(B, *g)
            if data:                 # the bf16 entry takes the plain mode, without ops.S2_DILATED
                return hc.direct_dilated_bf16() and ops.conv4x4s2_bf16_dil_supported(ops.S2_FINE_TO_COARSE if op == ops.CONV_FWD else ops.S2_COARSE_TO_FINE, B, *g)
            return hc.direct_dilated_bf16_dw() and ops.conv4x4s2_bf16_dil_wrw_supported(B, *g)
        g = hc._s2_geometry(lay)
        if g is None:
            return False
        if data:
            return (ops.conv4x4s2_bf16x3_supported if x3 else ops.conv4x4s2_bf16_supported)(hc._s2_mode(op), B, *g)
        return (ops.conv4x4s2_bf16x3_wrw_supported if x3 else ops.conv4x4s2_bf16_wrw_supported)(B, *g)
    raise KeyError("no support query is mapped for engine %r" % (engine,))


@contextlib.contextmanager
def switches(hipconv, name):
    """Run under one setting of the in-process switches and put back what was there: "default" (fp32 arithmetic, the four dilated switches
    off), "opt_in" (`OPT_IN_MATH` with both fp32 dilated switches on), any name of ops.DIRECT_PASSES (that arithmetic, both fp32 dilated
    switches on) — these keep both bf16 dilated switches off — or a name of `BF16_DIL_SWITCHES` (those bf16 dilated switches on, the fp32
    arithmetic and the fp32 pair at their defaults)."""
    was = (hipconv._MATH["fp32"], hipconv.direct_dilated(), hipconv.direct_dilated_dw(), hipconv.direct_dilated_bf16(), hipconv.direct_dilated_bf16_dw())
    bf16_data, bf16_dw = BF16_DIL_SWITCHES.get(name, (False, False))
    on = name != "default" and name not in BF16_DIL_SWITCHES
    try:
        hipconv.set_conv_math(fp32="fp32" if not on else OPT_IN_MATH if name == "opt_in" else name)
        hipconv.set_direct_dilated(on)
        hipconv.set_direct_dilated_dw(on)
        hipconv.set_direct_dilated_bf16(bf16_data)
        hipconv.set_direct_dilated_bf16_dw(bf16_dw)
        yield
    finally:
        hipconv.set_conv_math(fp32=was[0])
        hipconv.set_direct_dilated(was[1])
        hipconv.set_direct_dilated_dw(was[2])
        hipconv.set_direct_dilated_bf16(was[3])
        hipconv.set_direct_dilated_bf16_dw(was[4])


def answers(hipconv, lay, bf16):
    """What `select` x 2 and `select_wrw` answer for the layer's forward, input gradient and weight gradient, under the current switches."""
    transposed, B, Cin, H, W, Cout, k, stride, pad, dil = lay
    (_, fop), (_, bop), _ = passes(lay)
    return (hipconv.select(fop, B, Cin, H, W, Cout, k, stride, pad, dil, bf16), hipconv.select(bop, B, Cin, H, W, Cout, k, stride, pad, dil, bf16),
            hipconv.select_wrw(transposed, B, Cin, H, W, Cout, k, stride, pad, dil, bf16))


# ---- the corner table ------------------------------------------------------------------------------------------------------------------
# One row = one module call: mod "conv" (nn.Conv2d) / "convT" (nn.ConvTranspose2d), cin -> cout of the MODULE, geom = (k, stride, pad, dil),
# the input map H x W at batch B, bf16 = the input is a bf16 tensor, switches = "default" / "opt_in" / a name of `BF16_DIL_SWITCHES` (see `switches`), engines = the triple
# (forward, input gradient, weight gradient) the dispatcher answers.  Every row sits at its rule's minimum channel counts and holds at most
# 16 384 pixels per image.
class Row(namedtuple("Row", "mod cin cout geom H W B bf16 switches engines")):
    @property
    def lay(self):
        return (self.mod == "convT", self.B, self.cin, self.H, self.W, self.cout) + self.geom

    @property
    def id(self):
        return "%s_k%ds%dp%dd%d_%dto%d_%dx%d_b%d_%s%s" % ((self.mod,) + self.geom + (self.cin, self.cout, self.H, self.W, self.B, "bf16" if self.bf16 else "fp32",
                                                                                 "" if self.switches == "default" else "_" + self.switches))


def _rows(geom, bf16, sw, table):
    return [Row(mod, cin, cout, geom, H, W, B, bf16, sw, tuple(eng.split())) for mod, cin, cout, H, W, B, eng in table]


ROWS = _rows(K3, False, "default", [
    ("conv", 64, 128, 1, 256, 1, "winograd winograd miopen"),
    ("conv", 128, 64, 256, 1, 3, "winograd winograd miopen"),
    ("convT", 128, 64, 2, 128, 1, "winograd winograd miopen"),
    ("conv", 64, 64, 5, 52, 2, "winograd winograd miopen"),
    ("conv", 128, 256, 1, 256, 1, "winograd winograd winograd"),
    ("conv", 256, 128, 1024, 4, 1, "winograd winograd winograd"),
    ("convT", 256, 64, 3, 86, 3, "winograd winograd winograd"),
    ("conv", 256, 128, 1, 4096, 1, "winograd winograd winograd"),
    ("convT", 128, 256, 4096, 1, 1, "winograd winograd winograd"),
    ("conv", 256, 256, 1, 32, 1, "smallmap smallmap miopen"),
    ("conv", 256, 256, 32, 1, 1, "smallmap smallmap miopen"),
    ("convT", 256, 256, 2, 5, 3, "smallmap smallmap miopen"),
    ("conv", 3, 64, 1, 4096, 1, "thin thin thin_mfma"),
    ("convT", 64, 3, 3, 1366, 1, "miopen thin miopen"),
    ("conv", 6, 64, 2, 2048, 1, "miopen thin thin_mfma"),
    ("convT", 128, 6, 1, 4096, 1, "thin miopen thin_mfma"),
    ("conv", 70, 1, 1, 64, 3, "one miopen one"),
    ("convT", 64, 3, 1024, 4, 3, "thin thin miopen"),
]) + _rows(DIL, False, "default", [
    ("conv", 64, 64, 32, 2, 1, "wino_dil wino_dil miopen"),
    ("conv", 64, 65, 34, 6, 3, "wino_dil miopen miopen"),
    ("conv", 80, 64, 256, 2, 1, "wino_dil wino_dil miopen"),
    ("conv", 128, 128, 32, 2, 1, "wino_dil wino_dil wino_dil"),
    ("conv", 128, 130, 128, 6, 3, "wino_dil direct wino_dil"),
    ("conv", 128, 128, 130, 4, 1, "wino_dil wino_dil miopen"),
    ("conv", 128, 128, 16, 2, 1, "miopen direct miopen"),
    ("conv", 128, 32, 31, 8, 1, "miopen direct miopen"),
    ("conv", 256, 256, 2, 64, 1, "smallmap smallmap smallmap"),
    ("conv", 256, 256, 512, 2, 1, "miopen miopen smallmap"),
    ("conv", 128, 128, 32, 66, 3, "wino_dil wino_dil wino_dil"),
    ("conv", 128, 128, 16, 64, 1, "miopen direct miopen"),
]) + _rows(K4S1, False, "default", [
    ("conv", 128, 128, 16, 4, 1, "wino_dil wino_dil wino_dil"),
    ("conv", 128, 129, 17, 5, 3, "wino_dil miopen wino_dil"),
    ("conv", 128, 144, 128, 4, 1, "wino_dil wino_dil wino_dil"),
    ("conv", 128, 128, 16, 130, 3, "wino_dil wino_dil wino_dil"),
    ("conv", 128, 128, 16, 3, 1, "miopen miopen miopen"),            # W < 4: below the F(3x3,4x4) kernel, torch computes it (output width 2)
    ("conv", 256, 256, 4, 4, 1, "smallmap smallmap miopen"),
    ("conv", 64, 1, 2, 1024, 1, "one miopen one"),
    ("conv", 64, 1, 3, 40, 1, "one miopen one"),
    ("conv", 512, 1, 31, 5, 1, "one miopen one"),
]) + _rows(S2, False, "default", [
    ("conv", 64, 128, 32, 128, 1, "wino_s2 wino_s2 wino_s2"),
    ("conv", 64, 128, 34, 66, 3, "wino_s2 wino_s2 wino_s2"),
    ("convT", 128, 64, 17, 33, 2, "wino_s2 wino_s2 wino_s2"),
    ("convT", 128, 64, 64, 16, 1, "wino_s2 wino_s2 wino_s2"),
    ("convT", 64, 64, 16, 128, 1, "wino_s2 miopen miopen"),
    ("convT", 64, 64, 128, 16, 1, "wino_s2 miopen miopen"),
    ("conv", 64, 128, 32, 130, 1, "miopen wino_s2 miopen"),
    ("conv", 512, 512, 16, 16, 16, "miopen wino_s2 miopen"),          # the `B >= 16` rule of `_s2_wins`
    ("conv", 256, 256, 2, 64, 1, "smallmap smallmap smallmap"),
    ("convT", 256, 256, 1, 32, 1, "smallmap smallmap smallmap"),
    ("conv", 256, 256, 2, 512, 1, "miopen miopen smallmap"),
    ("conv", 256, 256, 10, 34, 3, "miopen miopen smallmap"),
    ("convT", 512, 256, 256, 1, 1, "miopen miopen smallmap"),
    ("conv", 3, 64, 2, 4096, 1, "miopen miopen thin_mfma"),
    ("convT", 64, 3, 2, 2048, 1, "miopen miopen thin_mfma"),
]) + _rows(K3, True, "default", [                                    # bf16 activations: the input is a bf16 tensor
    ("conv", 64, 64, 1, 256, 2, "bf16d bf16d miopen"),
    ("conv", 512, 512, 1, 256, 1, "bf16d bf16d winograd"),
    ("conv", 3, 64, 1, 4096, 1, "thin miopen thin_mfma"),
    ("conv", 3, 3, 16, 64, 1, "miopen miopen bf16d"),
    ("conv", 3, 3, 64, 16, 3, "miopen miopen bf16d"),
    ("conv", 64, 64, 16, 64, 3, "bf16d bf16d bf16d"),
]) + _rows(S2, True, "default", [
    ("conv", 3, 64, 2, 4096, 1, "thin_f2m miopen thin_mfma"),
    ("convT", 128, 128, 1, 64, 1, "miopen miopen bf16d"),
    ("convT", 64, 3, 1, 256, 1, "bf16d miopen miopen"),
    ("conv", 3, 64, 66, 64, 3, "thin_f2m miopen thin_mfma"),
    ("conv", 3, 64, 128, 32, 1, "miopen bf16d thin_mfma"),
]) + _rows(DIL, True, "default", [
    ("conv", 256, 256, 32, 2, 1, "wino_dil wino_dil wino_dil"),
]) + _rows(K4S1, True, "default", [
    ("conv", 256, 256, 16, 4, 1, "wino_dil wino_dil wino_dil"),
]) + _rows(K3, False, "opt_in", [                                    # fp32 activations on the direct split-bf16 kernels
    ("conv", 64, 64, 1, 256, 1, "bf16x3d bf16x3d miopen"),
    ("conv", 64, 64, 32, 16, 3, "bf16x3d bf16x3d miopen"),
    ("conv", 3, 3, 16, 64, 1, "miopen miopen bf16x3w"),
    ("conv", 3, 3, 64, 16, 3, "miopen miopen bf16x3w"),
]) + _rows(S2, False, "opt_in", [
    ("convT", 64, 64, 16, 32, 1, "bf16x3d miopen miopen"),
    ("convT", 64, 64, 32, 16, 1, "bf16x3d miopen miopen"),
    ("convT", 128, 128, 24, 16, 1, "wino_s2 wino_s2 bf16x3w"),
    ("convT", 128, 128, 16, 32, 1, "bf16x3d bf16x3d bf16x3w"),
]) + _rows(DIL, False, "opt_in", [
    ("conv", 64, 64, 32, 64, 1, "bf16x3d bf16x3d miopen"),
    ("conv", 64, 64, 64, 32, 1, "bf16x3d bf16x3d miopen"),
    ("conv", 128, 128, 48, 32, 1, "wino_dil wino_dil bf16x3w"),
    ("conv", 128, 128, 32, 64, 1, "bf16x3d bf16x3d bf16x3w"),
]) + _rows(DIL, True, "bf16_dil", [                                  # bf16 activations, the dilated layer on the direct bf16 kernels
    ("conv", 64, 64, 32, 64, 1, "bf16d bf16d bf16d"),                # base: MIOpen
    ("conv", 64, 64, 64, 32, 3, "bf16d bf16d bf16d"),
    ("conv", 256, 256, 32, 64, 1, "bf16d bf16d bf16d"),              # base: "wino_dil"
    ("conv", 128, 130, 16, 256, 1, "bf16d miopen bf16d"),            # the input gradient refuses a produced count that is no tile multiple
    ("conv", 256, 256, 16, 32, 1, "miopen miopen smallmap"),         # the "smallmap" grid stays
    ("conv", 64, 64, 34, 64, 1, "miopen miopen miopen"),             # odd coarse height: the kernel refuses
]) + _rows(DIL, True, "bf16_dil_data", [
    ("conv", 256, 256, 64, 32, 3, "bf16d bf16d wino_dil"),
    ("conv", 64, 64, 8, 256, 3, "bf16d bf16d miopen"),               # the 128-wide coarse grid
]) + _rows(DIL, True, "bf16_dil_dw", [
    ("conv", 256, 256, 32, 64, 1, "wino_dil wino_dil bf16d"),
])
